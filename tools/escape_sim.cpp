// Host model of an escape table for traceRay's grid walk: per 4^3 brick and
// direction bin, whether every ray that starts in the brick with a direction
// in the bin leaves the grid through empty cells only (its swept region,
// dilated by one cell, holds no occupied cell).  A walk that reaches such a
// brick can stop there: no later cell holds a triangle, so traceRay's result
// is the nearest hit so far (stage3.zig:152-185).  Reports, per ray, the
// steps the walk would save and checks soundness (no occupied cell visited
// after the escape point).
//   g++ -O2 -std=c++17 -fopenmp -ffp-contract=off -Izig_raytracing_contest_amd/csrc -Iinclude tools/escape_sim.cpp -o /tmp/escape_sim
//   escape_sim <scene.bin> <rays.bin> <out.bin> [bins_per_face_axis=4] [gx gy gz = 4 4 4] [per_brick=0] [n_cam=60000]
//              [dir=0] [start=0]
// gx gy gz: the start region, a sub-block of the 4^3 brick of 1, 2 or 4 cells
// per axis (csrc/escape.h EscShape); per_brick = 1: the walk asks the table
// once per 4^3 brick it enters, for the region of the cell it enters it in
// (the park kernel's query), not in every cell.
// dir = 1: occupancy per direction bin (escape.h, the direction-aware table):
// a cell counts as occupied for a bin iff it holds a ref that bfc_cull cannot
// reject for the whole cone of the bin's cull bin (kBfcBins x kBfcBins per
// face; bins_per_face_axis must be a multiple of kBfcBins).  A ray then
// "escapes" where every later cell is empty or holds only refs whose
// determinant test fails; the soundness check compares the hit at the escape
// point with the full walk's.
// start = 1: the walk also asks in its start cell, before testing it (the park
// kernel's query at refill): a set bit ends the ray with no cell visited.
// (tools/dump_sim_inputs.py writes scene.bin and rays.bin.)
// out.bin: per ray: steps u32, saved u32, unsound u32; stderr: the means
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "dda.h"
#include "escape.h"

using namespace zrt;

struct Esc {
    uint32_t res[3], nb[3], nbin;   // nbin per face axis
    // per occupancy (plain: one per axis a; dir: one per cull bin, a its face's axis): per cell slab of a, 2-D
    // inclusive prefix sums over the other two axes
    std::vector<std::vector<uint32_t>> pre;
    uint32_t g[3], nr[3], nreg;     // region cells per axis, regions per brick axis, per brick
    std::vector<uint8_t> bits;      // [brick][region][6 * nbin * nbin]
};

// direction bin: face = dominant axis and sign, (u, v) = the other two
// components over |d_a| in [-1, 1], nbin x nbin cells
static uint32_t dir_bin(v3 d, uint32_t nbin) {
    const float ax = fabsf(d.x), ay = fabsf(d.y), az = fabsf(d.z);
    uint32_t a;
    float m, u, v;
    if (ax >= ay && ax >= az) { a = 0; m = d.x; u = d.y / ax; v = d.z / ax; }
    else if (ay >= az) { a = 1; m = d.y; u = d.x / ay; v = d.z / ay; }
    else { a = 2; m = d.z; u = d.x / az; v = d.y / az; }
    const uint32_t f = 2 * a + (m < 0.0f ? 1 : 0);
    uint32_t iu = (uint32_t)fminf(fmaxf((u + 1.0f) * 0.5f * nbin, 0.0f), nbin - 1.0f);
    uint32_t iv = (uint32_t)fminf(fmaxf((v + 1.0f) * 0.5f * nbin, 0.0f), nbin - 1.0f);
    return (f * nbin + iu) * nbin + iv;
}

int main(int argc, char** argv) {
    if (argc < 4) return 2;
    const uint32_t nbin = argc > 4 ? atoi(argv[4]) : 4;
    uint32_t rgn[3] = {4, 4, 4};
    if (argc > 7)
        for (int a = 0; a < 3; ++a) rgn[a] = (uint32_t)atoi(argv[5 + a]);
    for (int a = 0; a < 3; ++a)
        if (rgn[a] != 1 && rgn[a] != 2 && rgn[a] != 4) return 2;
    const bool per_brick = argc > 8 && atoi(argv[8]) != 0;
    const bool dir_occ = argc > 10 && atoi(argv[10]) != 0, ask_start = argc > 11 && atoi(argv[11]) != 0;
    if (dir_occ && nbin % kBfcBins != 0) return 2;
    FILE* f = fopen(argv[1], "rb");
    float bmin[3], bmax[3], cs[3];
    uint32_t res[3], ncells, nrefs;
    if (fread(bmin, 4, 3, f) != 3 || fread(bmax, 4, 3, f) != 3 || fread(res, 4, 3, f) != 3 ||
        fread(cs, 4, 3, f) != 3 || fread(&ncells, 4, 1, f) != 1 || fread(&nrefs, 4, 1, f) != 1)
        return 3;
    std::vector<uint32_t> cells(2ull * ncells);
    std::vector<float> tp(9ull * nrefs);
    if (fread(cells.data(), 8, ncells, f) != ncells || fread(tp.data(), 36, nrefs, f) != nrefs) return 3;
    fclose(f);
    // per cell, the cull bins for which it holds a ref that cannot be rejected (dir), else occupancy in bit 0
    static_assert(kBfcNBin <= 128, "two words per cell");
    std::vector<uint64_t> cmask(2ull * ncells, 0);
    uint64_t n_ref_bin = 0, n_ref_cull = 0;
#pragma omp parallel for schedule(dynamic, 1024) reduction(+ : n_ref_bin, n_ref_cull)
    for (int64_t c = 0; c < (int64_t)ncells; ++c)
        for (uint32_t j = cells[2 * c]; j < cells[2 * c + 1]; ++j) {
            if (!dir_occ) { cmask[2 * c] = 1; break; }
            for (uint32_t cb = 0; cb < kBfcNBin; ++cb) {
                ++n_ref_bin;
                if (bfc_cull(&tp[9ull * j + 3], &tp[9ull * j + 6], cb)) ++n_ref_cull;
                else cmask[2 * c + (cb >> 6)] |= 1ull << (cb & 63u);
            }
        }
    // the cull bin of a walk bin (escape.h bfc_bin_of with nbin for kEscBins)
    auto cull_of = [&](uint32_t bin) {
        const uint32_t q = nbin / kBfcBins, fc = bin / (nbin * nbin), iu = (bin / nbin) % nbin, iv = bin % nbin;
        return (fc * kBfcBins + iu / q) * kBfcBins + iv / q;
    };
    const uint32_t nocc = dir_occ ? kBfcNBin : 3u;
    auto occ = [&](uint32_t k, uint32_t x, uint32_t y, uint32_t z) {
        const uint32_t c = (z * res[1] + y) * res[0] + x;
        return dir_occ ? ((cmask[2 * c + (k >> 6)] >> (k & 63u)) & 1u) != 0u : cmask[2 * c] != 0u;
    };
    Esc E;
    for (int a = 0; a < 3; ++a) { E.res[a] = res[a]; E.nb[a] = (res[a] + 3) / 4; }
    E.nbin = nbin;
    for (int a = 0; a < 3; ++a) { E.g[a] = rgn[a]; E.nr[a] = 4 / rgn[a]; }
    E.nreg = E.nr[0] * E.nr[1] * E.nr[2];
    // prefix sums: axis a's slab i, 2-D over (b, c) = the other axes in order
    E.pre.resize(nocc);
#pragma omp parallel for schedule(dynamic, 1)
    for (int k = 0; k < (int)nocc; ++k) {
        const int a = dir_occ ? k / (int)(2 * kBfcBins * kBfcBins) : k;
        const int b = a == 0 ? 1 : 0, c = a == 2 ? 1 : 2;
        const uint32_t R = res[b] + 1, S = res[c] + 1;
        E.pre[k].assign((size_t)res[a] * R * S, 0);
        for (uint32_t i = 0; i < res[a]; ++i)
            for (uint32_t y = 0; y < res[b]; ++y)
                for (uint32_t z = 0; z < res[c]; ++z) {
                    uint32_t p[3];
                    p[a] = i; p[b] = y; p[c] = z;
                    uint32_t* P = &E.pre[k][(size_t)i * R * S];
                    P[(y + 1) * S + z + 1] = (occ((uint32_t)k, p[0], p[1], p[2]) ? 1 : 0) + P[y * S + z + 1] + P[(y + 1) * S + z] -
                                             P[y * S + z];
                }
    }
    const uint32_t nbr = E.nb[0] * E.nb[1] * E.nb[2], nb6 = 6 * nbin * nbin;
    E.bits.assign((size_t)nbr * E.nreg * nb6, 0);
#pragma omp parallel for schedule(dynamic, 64)
    for (int64_t rg = 0; rg < (int64_t)nbr * E.nreg; ++rg) {
        const int64_t br = rg / E.nreg;
        const uint32_t sub = (uint32_t)(rg % E.nreg);
        const uint32_t B[3] = {(uint32_t)(br % E.nb[0]), (uint32_t)((br / E.nb[0]) % E.nb[1]),
                               (uint32_t)(br / (E.nb[0] * E.nb[1]))};
        const uint32_t R[3] = {sub % E.nr[0], (sub / E.nr[0]) % E.nr[1], sub / (E.nr[0] * E.nr[1])};
        uint32_t c0[3];
        for (int a = 0; a < 3; ++a) c0[a] = 4 * B[a] + R[a] * E.g[a];
        if (c0[0] >= res[0] || c0[1] >= res[1] || c0[2] >= res[2]) continue;   // past the grid's edge
        for (uint32_t bin = 0; bin < nb6; ++bin) {
            const uint32_t fc = bin / (nbin * nbin), iu = (bin / nbin) % nbin, iv = bin % nbin;
            const int a = fc / 2, sg = (fc & 1) ? -1 : 1;
            const int b = a == 0 ? 1 : 0, c = a == 2 ? 1 : 2;
            const double eps = 1e-3;
            const double u0 = -1.0 + 2.0 * iu / nbin - eps, u1 = -1.0 + 2.0 * (iu + 1) / nbin + eps;
            const double v0 = -1.0 + 2.0 * iv / nbin - eps, v1 = -1.0 + 2.0 * (iv + 1) / nbin + eps;
            // the region in cell units
            const double lo[3] = {(double)c0[0], (double)c0[1], (double)c0[2]};
            const double hi[3] = {fmin((double)c0[0] + E.g[0], res[0]), fmin((double)c0[1] + E.g[1], res[1]),
                                  fmin((double)c0[2] + E.g[2], res[2])};
            bool ok = true;
            const uint32_t R = res[b] + 1, S = res[c] + 1;
            for (int i = sg > 0 ? (int)lo[a] : (int)hi[a] - 1; ok && i >= 0 && i < (int)res[a]; i += sg) {
                // a-distance from the brick to slab i (cell units)
                double smin, smax;
                if (sg > 0) { smin = fmax(0.0, i - hi[a]); smax = fmax(0.0, i + 1 - lo[a]); }
                else { smin = fmax(0.0, lo[a] - (i + 1)); smax = fmax(0.0, hi[a] - i); }
                // (u, v are slopes in world units: a cell-unit step along a moves
                // cs_a / cs_b cells along b)
                const double kb = (double)cs[a] / cs[b], kc = (double)cs[a] / cs[c];
                const double ylo = lo[b] + kb * fmin(smin * u0, smax * u0), yhi = hi[b] + kb * fmax(smin * u1, smax * u1);
                const double zlo = lo[c] + kc * fmin(smin * v0, smax * v0), zhi = hi[c] + kc * fmax(smin * v1, smax * v1);
                // cells overlapping [ylo, yhi] dilated by one cell
                const int y0 = (int)std::max(0.0, floor(ylo) - 1), y1 = (int)std::min((double)res[b] - 1, ceil(yhi));
                const int z0 = (int)std::max(0.0, floor(zlo) - 1), z1 = (int)std::min((double)res[c] - 1, ceil(zhi));
                if (y0 > y1 || z0 > z1) break;       // the region has left the grid sideways
                const uint32_t* P = &E.pre[dir_occ ? cull_of(bin) : (uint32_t)a][(size_t)i * R * S];
                const uint32_t cnt = P[(y1 + 1) * S + z1 + 1] - P[y0 * S + z1 + 1] - P[(y1 + 1) * S + z0] + P[y0 * S + z0];
                if (cnt) ok = false;
            }
            E.bits[(size_t)rg * nb6 + bin] = ok;
        }
    }
    uint64_t nesc = 0;
    for (auto x : E.bits) nesc += x;
    if (dir_occ)
        fprintf(stderr, "occupancy per cull bin (%u bins): %.3f of the (ref, bin) pairs rejected for the whole cone\n",
                kBfcNBin, n_ref_bin ? (double)n_ref_cull / (double)n_ref_bin : 0.0);
    fprintf(stderr, "region %u x %u x %u, %s: escape bits set: %.3f of %u x %u x %u, table %.1f MB at 1 bit per bin\n",
            E.g[0], E.g[1], E.g[2], per_brick ? "asked per brick entered" : "asked in every cell",
            (double)nesc / E.bits.size(), nbr, E.nreg, nb6, (double)nbr * E.nreg * ((nb6 + 31) / 32) * 4e-6);

    GridK g;
    g.rm0 = res[0] - 1; g.rm1 = res[1] - 1; g.rm2 = res[2] - 1;
    g.str1 = res[0]; g.str2 = res[0] * res[1];
    // one ray: cells visited, those after the escape point, soundness, the hit
    struct Walk {
        uint32_t steps, saved, unsound, ref;
        float t;
        uint32_t at_start;
    };
    auto walk = [&](const v3 o, const v3 d) {
        const uint32_t bin = dir_bin(d, nbin);
        Walk w{0, 0, 0, ~0u, kInf, 0};
        uint32_t esc_at = 0, asked = ~0u, esc_ref = ~0u;
        float esc_t = kInf;
        bool escaped = false;
        Dda s;
        if (!dda_init(bmin, bmax, res, cs, o, d, s)) return w;
        for (;;) {
            const uint32_t brk = ((s.c2 / 4) * E.nb[1] + s.c1 / 4) * E.nb[0] + s.c0 / 4;
            const uint32_t sub = ((s.c2 & 3) / E.g[2] * E.nr[1] + (s.c1 & 3) / E.g[1]) * E.nr[0] + (s.c0 & 3) / E.g[0];
            if (ask_start && w.steps == 0 && E.bits[((size_t)brk * E.nreg + sub) * nb6 + bin]) {
                escaped = true;
                w.at_start = 1;
                asked = brk;
            }
            ++w.steps;
            struct { uint32_t x, y; } cr = {cells[2 * s.lin], cells[2 * s.lin + 1]};
            if (escaped && !dir_occ && cr.y > cr.x) w.unsound = 1;
            for (uint32_t j = cr.x; j < cr.y; ++j) {
                const float* q = &tp[9ull * j];
                float t, u, v;
                if (tri_ray(mk(q[0], q[1], q[2]), mk(q[3], q[4], q[5]), mk(q[6], q[7], q[8]), o, d, &t, &u, &v))
                    if (w.t > t && t > 0.0f) { w.t = t; w.ref = j; }
            }
            if (!escaped && (!per_brick || brk != asked) && E.bits[((size_t)brk * E.nreg + sub) * nb6 + bin]) {
                escaped = true;
                esc_at = w.steps;
                esc_t = w.t;
                esc_ref = w.ref;
            }
            asked = brk;
            bool crossed;
            float te;
            DDA_STEP(s, g, 2, crossed, te);
            (void)crossed;
            if (w.t <= te) break;
        }
        w.saved = escaped ? w.steps - esc_at : 0;
        // (the hit at the escape point must be the walk's: bitwise t, and the ref)
        if (escaped && (memcmp(&esc_t, &w.t, 4) != 0 || esc_ref != w.ref)) w.unsound = 1;
        return w;
    };
    // the rays: a rays.bin (n u32, then origin and direction per ray), or a
    // cam.bin of dump_sim_inputs.py (14 floats): then argv[9] (default 60000)
    // camera rays through random pixels are traced here and the rays measured
    // are their bounce rays, spawned at the hit as normalize(normal + uniform
    // unit vector) (the normal turned against the incoming ray), first
    // generation then second
    std::vector<float> rays;
    uint32_t n = 0, n_gen1 = 0;
    f = fopen(argv[2], "rb");
    if (!f) return 3;
    fseek(f, 0, SEEK_END);
    const long fsz = ftell(f);
    fseek(f, 0, SEEK_SET);
    if (fsz == 14 * 4) {
        float cam[14];
        if (fread(cam, 4, 14, f) != 14) return 3;
        const uint32_t n_cam = argc > 9 ? (uint32_t)atoi(argv[9]) : 60000u;
        std::mt19937_64 rng(1);
        std::uniform_real_distribution<float> U(0.0f, 1.0f);
        const float diag = sqrtf((bmax[0] - bmin[0]) * (bmax[0] - bmin[0]) + (bmax[1] - bmin[1]) * (bmax[1] - bmin[1]) +
                                 (bmax[2] - bmin[2]) * (bmax[2] - bmin[2]));
        std::vector<float> cur;
        for (uint32_t k = 0; k < n_cam; ++k) {
            const float px = cam[12] * U(rng), py = cam[13] * U(rng);
            const v3 d = normalize(mk(cam[3] + cam[6] * px + cam[9] * py, cam[4] + cam[7] * px + cam[10] * py,
                                      cam[5] + cam[8] * px + cam[11] * py));
            const float r6[6] = {cam[0], cam[1], cam[2], d.x, d.y, d.z};
            cur.insert(cur.end(), r6, r6 + 6);
        }
        for (int gen = 0; gen < 2; ++gen) {
            std::vector<float> next;
            for (size_t k = 0; k < cur.size() / 6; ++k) {
                const v3 o = mk(cur[6 * k], cur[6 * k + 1], cur[6 * k + 2]), d = mk(cur[6 * k + 3], cur[6 * k + 4], cur[6 * k + 5]);
                const Walk w = walk(o, d);
                if (w.ref == ~0u) continue;
                const float* q = &tp[9ull * w.ref];
                v3 nr = cross(mk(q[3], q[4], q[5]), mk(q[6], q[7], q[8]));
                if (!(dot(nr, nr) > 0.0f)) continue;
                nr = normalize(nr);
                if (dot(nr, d) > 0.0f) nr = scale(nr, -1.0f);
                v3 u;
                do u = mk(2.0f * U(rng) - 1.0f, 2.0f * U(rng) - 1.0f, 2.0f * U(rng) - 1.0f);
                while (dot(u, u) > 1.0f || dot(u, u) < 1e-6f);
                const v3 nd = normalize(add(nr, normalize(u)));
                const v3 no = add(add(o, scale(d, w.t)), scale(nr, 1e-5f * diag));
                const float r6[6] = {no.x, no.y, no.z, nd.x, nd.y, nd.z};
                next.insert(next.end(), r6, r6 + 6);
            }
            rays.insert(rays.end(), next.begin(), next.end());
            if (gen == 0) n_gen1 = (uint32_t)(next.size() / 6);
            cur.swap(next);
        }
        n = (uint32_t)(rays.size() / 6);
        fprintf(stderr, "%u camera rays, %u first-generation and %u second-generation bounce rays\n", n_cam, n_gen1,
                n - n_gen1);
    } else {
        if (fread(&n, 4, 1, f) != 1) return 3;
        rays.resize(6ull * n);
        if (fread(rays.data(), 24, n, f) != n) return 3;
        n_gen1 = n;
    }
    fclose(f);
    std::vector<uint32_t> out(3ull * n);
    std::vector<uint8_t> at_start(n, 0);
#pragma omp parallel for schedule(dynamic, 256)
    for (int64_t r = 0; r < (int64_t)n; ++r) {
        const Walk w = walk(mk(rays[6 * r], rays[6 * r + 1], rays[6 * r + 2]),
                            mk(rays[6 * r + 3], rays[6 * r + 4], rays[6 * r + 5]));
        out[3 * r] = w.steps;
        out[3 * r + 1] = w.saved;
        out[3 * r + 2] = w.unsound;
        at_start[r] = (uint8_t)w.at_start;
    }
    for (int part = 0; part < 2; ++part) {
        const uint32_t r0 = part ? n_gen1 : 0, r1 = part ? n : n_gen1;
        if (r0 == r1) continue;
        uint64_t st = 0, sv = 0, un = 0, as = 0, fr = 0;
        for (uint32_t r = r0; r < r1; ++r) {
            st += out[3 * r]; sv += out[3 * r + 1]; un += out[3 * r + 2];
            as += at_start[r];
            fr += out[3 * r + 1] != 0u && out[3 * r + 1] + 1u >= out[3 * r] ? 1u : 0u;   // free after the first cell at the latest
        }
        fprintf(stderr, "rays [%u, %u): cells per ray without the table %.2f, with it %.2f, unsound rays %llu; "
                "ended in the start cell %.3f, free after the first cell at the latest %.3f\n", r0, r1,
                (double)st / (r1 - r0), (double)(st - sv) / (r1 - r0), (unsigned long long)un, (double)as / (r1 - r0),
                (double)fr / (r1 - r0));
    }
    f = fopen(argv[3], "wb");
    fwrite(out.data(), 12, n, f);
    fclose(f);
    return 0;
}
