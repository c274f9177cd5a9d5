// Host check of the park kernel's hop (render.hip PARK_HOP) and of the hop
// bits in the cell records (context.hip cell32_hop_kernel).  Built as a
// shared library by tests/test_hop.py.
//
// hop_words: the six mask words of every cell as the two record passes write
// them, restated; hop_encoding_check reads them back against the old masks.
// hop_trace_check: the sequential traceRay walk with the entry-face masks,
// without the hop and with it (first-cell hop bits excluded / included), and
// two controls that must change some ray (the bits decoded non-inverted; the
// bit of a wrong face): identical (t, u, v, ref) bits, parks, hops and the
// run lengths of useless parks.
// hop_tie_check: the kernel's own rule -- the axis read off the stepped packed
// word against the field masks of hm -- on rays through cell edges and
// corners (tests/cpp/dda_walk_check.cpp's rays), against the axis DDA_STEP
// stepped.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <random>
#include <vector>

#include "dda.h"
#include "escape.h"

using namespace zrt;

namespace {

constexpr uint32_t kHopMaxRefs = 26, kHopShift = 26;    // render_context.h

struct Scn {
    const float *bmin, *bmax, *cs;
    const uint32_t *res, *cells;
    const float* pos;   // 9 per ref: v0, e1, e2
    GridK gk;
};

uint32_t low_bits(uint32_t n) { return n >= 32u ? ~0u : (1u << n) - 1u; }

bool test_tri(const Scn& S, uint32_t j, v3 o, v3 d, float* t, float* u, float* v) {
    const float* q = S.pos + 9ull * j;
    return tri_ray(mk(q[0], q[1], q[2]), mk(q[3], q[4], q[5]), mk(q[6], q[7], q[8]), o, d, t, u, v);
}

// the neighbour of cell ci one step in the direction of face index f, or -1
int64_t neighbour(const Scn& S, uint32_t ci, uint32_t f) {
    const uint32_t r0 = S.res[0], r1 = S.res[1], r2 = S.res[2];
    const uint32_t x = ci % r0, y = (ci / r0) % r1, z = ci / r0 / r1;
    const uint32_t axis = f >> 1, neg = f & 1u;
    const uint32_t cc = axis == 0 ? x : (axis == 1 ? y : z), rr = axis == 0 ? r0 : (axis == 1 ? r1 : r2);
    if (neg ? cc == 0u : cc + 1u >= rr) return -1;
    const uint32_t step = axis == 0 ? 1u : (axis == 1 ? r0 : r0 * r1);
    return neg ? (int64_t)ci - step : (int64_t)ci + step;
}

// the entry-face mask of (cell, face) as cell32_kernel (pass 1) writes it
uint32_t face_mask(const Scn& S, uint32_t ci, uint32_t f) {
    const uint32_t b = S.cells[2 * ci], n = S.cells[2 * ci + 1] - b;
    uint32_t m = low_bits(n);
    const int64_t pci = neighbour(S, ci, f ^ 1u);        // the cell left: one step back
    if (pci >= 0 && n > 0 && n <= 32) {
        for (uint32_t k = 0; k < n; ++k)
            for (uint32_t q = S.cells[2 * pci]; q < S.cells[2 * pci + 1]; ++q)
                if (!memcmp(S.pos + 9ull * (b + k), S.pos + 9ull * q, 36)) { m &= ~(1u << k); break; }
    }
    return m;
}

// old[6 ci + f]: pass 1's masks; words[6 ci + f]: the records after pass 2
void build_words(const Scn& S, std::vector<uint32_t>& old, std::vector<uint32_t>& words) {
    const uint32_t nc = S.res[0] * S.res[1] * S.res[2];
    old.resize(6ull * nc);
    words.resize(6ull * nc);
    for (uint32_t ci = 0; ci < nc; ++ci)
        for (uint32_t f = 0; f < 6; ++f) old[6ull * ci + f] = face_mask(S, ci, f);
    for (uint32_t ci = 0; ci < nc; ++ci) {
        const uint32_t n = S.cells[2 * ci + 1] - S.cells[2 * ci];
        for (uint32_t f = 0; f < 6; ++f) words[6ull * ci + f] = old[6ull * ci + f];
        if (n >= 32u) continue;
        if (n > kHopMaxRefs) {
            for (uint32_t f = 0; f < 6; ++f) words[6ull * ci + f] |= ~low_bits(n);
            continue;
        }
        uint32_t hop = 0x3Fu;
        for (uint32_t f = 0; f < 6 && n != 0u; ++f) {
            const int64_t nb = neighbour(S, ci, f);
            if (nb < 0) continue;
            const uint32_t nn = S.cells[2 * nb + 1] - S.cells[2 * nb];
            if (nn == 0u || nn > 32u) continue;
            if ((old[6ull * nb + f] & low_bits(nn)) == 0u) hop &= ~(1u << f);
        }
        for (uint32_t f = 0; f < 6; ++f)
            words[6ull * ci + f] = (words[6ull * ci + f] & ((1u << kHopShift) - 1u)) | (hop << kHopShift);
    }
}

// the kernel's decode of a landed mask word of a cell of cnt refs
uint32_t hop_decode(uint32_t word, uint32_t cnt) { return cnt <= kHopMaxRefs ? ~word >> kHopShift : 0u; }

enum { kNoHop = 0, kHop = 1, kHopFirst = 2, kCtlNotInverted = 3, kCtlWrongFace = 4, kVariants = 5 };

struct Cnt {
    uint64_t parks = 0, useless = 0, hops = 0;
    uint64_t runs[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // useless runs of length 1..7, 8+
};

// Scene.traceRay with the entry-face masks; a cell with refs is a park.  After
// a park the lane holds the hop bits of that cell's word; if the bit of the
// face its next step crosses is set, the next cell is walked through untested
// (its break test runs as for any cell).
void trace(const Scn& S, const std::vector<uint32_t>& words, int variant, v3 o, v3 d, float out[4], Cnt& c) {
    float nearest = kInf, hu = 0, hv = 0;
    uint32_t hidx = 0;
    Dda s;
    if (dda_init(S.bmin, S.bmax, S.res, S.cs, o, d, s)) {
        int face = -1;
        uint32_t hb = 0, run = 0;
        bool skip = false;
        for (;;) {
            const uint32_t b = S.cells[2 * s.lin], e = S.cells[2 * s.lin + 1], n = e - b;
            if (n > 0 && !skip) {
                // the landed word: the entry face's; the first cell's is all ones,
                // or (the cull table's, cells of at most 26 refs) ones with the hop bits
                uint32_t word = ~0u;
                if (face >= 0) word = words[6ull * s.lin + (uint32_t)face];
                else if (variant == kHopFirst && n <= kHopMaxRefs) word = words[6ull * s.lin] | ((1u << kHopShift) - 1u);
                const uint32_t keep = n <= 32u ? word & low_bits(n) : ~0u;
                c.parks += 1;
                if (n <= 32u && keep == 0u) {
                    c.useless += 1;
                    run += 1;
                } else {
                    if (run) c.runs[run > 8 ? 7 : run - 1] += 1;
                    run = 0;
                }
                for (uint32_t j = b; j < e; ++j) {
                    if (j - b < 32 && !((keep >> (j - b)) & 1u)) continue;
                    float t, u, v;
                    if (test_tri(S, j, o, d, &t, &u, &v) && nearest > t && t > 0.0f) {
                        nearest = t; hu = u; hv = v; hidx = j;
                    }
                }
                hb = variant == kNoHop ? 0u : (variant == kCtlNotInverted ? (n <= kHopMaxRefs ? word >> kHopShift : 0u)
                                                                          : hop_decode(word, n));
            } else {
                if (n > 0) c.hops += 1;
                hb = 0;
            }
            const uint32_t c0 = s.c0, c1 = s.c1;
            bool crossed;
            float t_exit;
            DDA_STEP(s, S.gk, 2, crossed, t_exit);
            (void)crossed;
            if (nearest <= t_exit) break;
            const int axis = s.c0 != c0 ? 0 : (s.c1 != c1 ? 1 : 2);
            face = 2 * axis + (int)((s.neg >> axis) & 1u);
            const int used = variant == kCtlWrongFace ? 2 * ((axis + 1) % 3) + (int)((s.neg >> ((axis + 1) % 3)) & 1u) : face;
            skip = ((hb >> used) & 1u) != 0u;
        }
        if (run) c.runs[run > 8 ? 7 : run - 1] += 1;
    }
    out[0] = nearest; out[1] = hu; out[2] = hv;
    memcpy(&out[3], &hidx, 4);
}

Scn make_scn(const float* bmin, const float* bmax, const uint32_t* res, const float* cs, const uint32_t* cells,
             const float* pos) {
    return Scn{bmin, bmax, cs, res, cells, pos, GridK{res[0] - 1, res[1] - 1, res[2] - 1, res[0], res[0] * res[1]}};
}

}  // namespace

// out[0] (cell, face) words whose low n bits differ from the old mask;
// out[1] words of cells of 0 or 27..31 refs with a zero bit among bits 26..31
// above the mask's own, or words of cells of 32 refs or more that differ
// from the old word; out[2] such cells whose decode yields a hop;
// out[3] faces of occupied cells, out[4] those with a zero low mask in the new
// words, out[5] the same in the old words (the release statistic's counts);
// out[6] cleared hop bits (hops offered), out[7] cells of 1..26 refs;
// out[8] words of cells of 1..26 refs whose six hop bits differ between faces.
extern "C" void hop_encoding_check(const float* bmin, const float* bmax, const uint32_t* res, const float* cs,
                                   const uint32_t* cells, const float* pos, uint64_t* out) {
    const Scn S = make_scn(bmin, bmax, res, cs, cells, pos);
    std::vector<uint32_t> old, words;
    build_words(S, old, words);
    memset(out, 0, 9 * sizeof(uint64_t));
    const uint32_t nc = res[0] * res[1] * res[2];
    for (uint32_t ci = 0; ci < nc; ++ci) {
        const uint32_t n = cells[2 * ci + 1] - cells[2 * ci];
        for (uint32_t f = 0; f < 6; ++f) {
            const uint32_t w = words[6ull * ci + f], m = old[6ull * ci + f];
            if ((w & low_bits(n)) != (m & low_bits(n))) ++out[0];
            if (n == 0u || (n > kHopMaxRefs && n < 32u)) {
                const uint32_t above = ~low_bits(n) & ~((1u << kHopShift) - 1u);
                if ((w & above) != above) ++out[1];
                if (n != 0u && hop_decode(w, n) != 0u) ++out[2];
                if (n == 0u && (~w >> kHopShift) != 0u) ++out[2];
            } else if (n >= 32u) {
                if (w != m) ++out[1];
                if (hop_decode(w, n) != 0u) ++out[2];
            } else {
                out[6] += (uint64_t)__builtin_popcount(hop_decode(w, n));
                if ((w >> kHopShift) != (words[6ull * ci] >> kHopShift)) ++out[8];
            }
            if (n > 0u) {
                ++out[3];
                if ((w & low_bits(n)) == 0u) ++out[4];
                if (m == 0u) ++out[5];
            }
        }
        if (n >= 1u && n <= kHopMaxRefs) ++out[7];
    }
    if (hop_decode(~0u, 1u) != 0u || hop_decode(~0u, kHopMaxRefs) != 0u) ++out[2];      // all ones: no hop
}

// rays: 6 floats per ray; units: 3 floats per ray and bounce (the bounce
// directions normalize(n_geo + unit)).  Every ray and `bounces` generations
// of rays spawned at the hits are traced in every variant.
// bad[v]: rays whose variant v differs from kNoHop in any bit;
// stats[8 v ..]: parks, useless parks, hops of variant v; stats[40 ..47]: the
// useless-run histogram of kNoHop (runs of 1..7, 8 and more); stats[48]: rays.
extern "C" void hop_trace_check(const float* bmin, const float* bmax, const uint32_t* res, const float* cs,
                                const uint32_t* cells, const float* pos, uint32_t nrays, const float* rays,
                                const float* units, uint32_t bounces, uint64_t* bad, uint64_t* stats) {
    const Scn S = make_scn(bmin, bmax, res, cs, cells, pos);
    std::vector<uint32_t> old, words;
    build_words(S, old, words);
    Cnt cnt[kVariants];
    memset(bad, 0, kVariants * sizeof(uint64_t));
    memset(stats, 0, 49 * sizeof(uint64_t));
    for (uint32_t i = 0; i < nrays; ++i) {
        v3 o = mk(rays[6 * i], rays[6 * i + 1], rays[6 * i + 2]);
        v3 d = mk(rays[6 * i + 3], rays[6 * i + 4], rays[6 * i + 5]);
        for (uint32_t depth = 0; depth <= bounces; ++depth) {
            float a[4], b[4];
            trace(S, words, kNoHop, o, d, a, cnt[kNoHop]);
            for (int v = 1; v < kVariants; ++v) {
                trace(S, words, v, o, d, b, cnt[v]);
                if (memcmp(a, b, 16)) ++bad[v];
            }
            ++stats[48];
            if (!(a[0] < kInf) || depth == bounces) break;
            uint32_t j;
            memcpy(&j, &a[3], 4);
            const float* q = S.pos + 9ull * j;
            v3 n = normalize(cross(mk(q[3], q[4], q[5]), mk(q[6], q[7], q[8])));
            if (dot(n, d) > 0.0f) n = scale(n, -1.0f);
            const float* un = units + 3ull * ((uint64_t)i * bounces + depth);
            o = add(o, scale(d, a[0]));
            d = normalize(add(n, mk(un[0], un[1], un[2])));
        }
    }
    for (int v = 0; v < kVariants; ++v) {
        stats[8 * v] = cnt[v].parks;
        stats[8 * v + 1] = cnt[v].useless;
        stats[8 * v + 2] = cnt[v].hops;
    }
    for (int k = 0; k < 8; ++k) stats[40 + k] = cnt[kNoHop].runs[k];
}

// ---- the kernel's face rule on ties ----
namespace {

// PARK_HOP: the field masks of the axes along which the lane's next step may
// hop, from the record's hop bits and the lane's step signs
uint32_t hop_hm(uint32_t hb, const DdaV& s, uint32_t f0, uint32_t f1, uint32_t f2) {
    const uint32_t hb1 = hb >> 1;
    const uint32_t e0 = (int32_t)s.d0 < 0 ? hb1 : hb, e1 = (int32_t)s.d1 < 0 ? hb1 : hb, e2 = (int32_t)s.d2 < 0 ? hb1 : hb;
    auto sbfe1 = [](uint32_t x, uint32_t bit) { return ((x >> bit) & 1u) ? ~0u : 0u; };
    return (sbfe1(e0, 0) & f0) | (sbfe1(e1, 2) & f1) | (sbfe1(e2, 4) & f2);
}

template <bool PK_BM>
void tie_walk(const GridK& k, const PackK& pk, Dda s, std::mt19937_64& rng, uint64_t* out) {
    DdaV y;
    ddav_from(s, k, pk, y);
    for (int guard = 0; guard < 100000; ++guard) {
        const uint32_t c0 = s.c0, c1 = s.c1;
        const bool tie = s.tn0 == s.tn1 || s.tn1 == s.tn2 || s.tn0 == s.tn2;
        bool crossed;
        float t_exit;
        DDA_STEP(s, k, 2, crossed, t_exit);
        (void)crossed;
        const uint32_t prev = y.pc;
        LaneM ex;
        float tc;
        DDAV_STEPM(y, pk.f0, pk.f1, pk.f2, ex, tc);
        if (t_exit == kInf) return;                 // the exit step: the trip ends the segment before any hop
        const uint32_t axis = s.c0 != c0 ? 0u : (s.c1 != c1 ? 1u : 2u);
        const uint32_t face = 2u * axis + ((s.neg >> axis) & 1u);
        const uint32_t x = y.pc ^ prev;
        // the stepped word changes inside exactly the stepped axis's field
        const uint32_t in = ((x & pk.f0) ? 1u : 0u) | ((x & pk.f1) ? 2u : 0u) | ((x & pk.f2) ? 4u : 0u);
        ++out[0];
        out[1] += tie ? 1 : 0;
        if (in != (1u << axis)) ++out[2];
        // the trip's test against hm, for random hop bits and for each single bit
        for (int r = 0; r < 8; ++r) {
            const uint32_t hb = r < 6 ? 1u << r : (uint32_t)(rng() & 63u);
            const bool hop = (x & hop_hm(hb, y, pk.f0, pk.f1, pk.f2)) != 0u;
            if (hop != (((hb >> face) & 1u) != 0u)) ++out[3];
        }
    }
}

}  // namespace

// dda_walk_check.cpp's grids and rays (random, zero components, exact
// diagonals from cell corners).  out[0] steps, out[1] steps taken at a tie of
// crossing ts, out[2] steps whose packed word changed outside the stepped
// axis's field, out[3] (step, hop bits) pairs where the trip's hm test differs
// from the hop bit of the face DDA_STEP crossed, out[4] rays.
extern "C" void hop_tie_check(uint32_t n_grids, uint32_t n_rays, uint64_t* out) {
    std::mt19937_64 rng(12345);
    std::uniform_real_distribution<float> U(0.0f, 1.0f);
    memset(out, 0, 5 * sizeof(uint64_t));
    for (uint32_t gi = 0; gi < n_grids; ++gi) {
        float bmin[3], bmax[3], cs[3];
        uint32_t res[3];
        const bool pow2 = gi % 3 == 0;     // exact arithmetic -> many crossing ties
        const bool bm = gi % 2 == 1;       // grids the brick-major words pack
        for (int a = 0; a < 3; ++a) {
            res[a] = gi == 0 ? 128u : 1u + (uint32_t)(rng() % 40);
            if (bm) res[a] = 4u << (rng() % 5);
            bmin[a] = pow2 ? 0.0f : -5.0f + 10.0f * U(rng);
            cs[a] = pow2 ? 0.25f : 0.05f + U(rng);
            bmax[a] = bmin[a] + cs[a] * (float)res[a];
        }
        GridK k{res[0] - 1, res[1] - 1, res[2] - 1, res[0], res[0] * res[1]};
        PackK pk;
        if (!pack_layout(res, pk, bm)) continue;
        for (uint32_t r = 0; r < n_rays; ++r) {
            const int kind = (int)(r % 4);
            float c[3];
            for (int a = 0; a < 3; ++a) {
                const float ext = bmax[a] - bmin[a];
                c[a] = bmin[a] - 0.5f * ext + 2.0f * ext * U(rng);
                if (kind >= 2) c[a] = bmin[a] + cs[a] * (float)(rng() % (res[a] + 1));   // on cell corners
            }
            const v3 o = mk(c[0], c[1], c[2]);
            v3 d;
            if (kind == 0) {
                d = normalize(mk(U(rng) - 0.5f, U(rng) - 0.5f, U(rng) - 0.5f));
            } else if (kind == 1) {                 // one or two zero components
                float v[3] = {U(rng) - 0.5f, U(rng) - 0.5f, U(rng) - 0.5f};
                v[rng() % 3] = 0.0f;
                if (rng() & 1) v[rng() % 3] = 0.0f;
                if (v[0] == 0 && v[1] == 0 && v[2] == 0) v[0] = 1.0f;
                d = normalize(mk(v[0], v[1], v[2]));
            } else {                                // exact diagonals: equal |d| per axis
                const float sx = (rng() & 1) ? 1.0f : -1.0f, sy = (rng() & 1) ? 1.0f : -1.0f,
                            sz = (rng() & 1) ? 1.0f : -1.0f;
                d = kind == 2 ? normalize(mk(sx, sy, sz)) : normalize(mk(sx, 2.0f * sy, sz));
            }
            Dda s;
            if (!dda_init(bmin, bmax, res, cs, o, d, s)) continue;
            ++out[4];
            if (pk.bm) tie_walk<true>(k, pk, s, rng, out);
            else tie_walk<false>(k, pk, s, rng, out);
        }
    }
}
