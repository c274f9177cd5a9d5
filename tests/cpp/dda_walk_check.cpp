// Host check of the walk steps and the fast-forward of csrc/dda.h: on random
// grids and rays (including axis-aligned and exact-diagonal ones that produce
// crossing ties), DDAW_STEP (the unpacked walk), DDAV_STEPX and DDAV_STEPM
// (the packed walks) must step exactly like the cell-by-cell walk of
// Iterator.next (DDA_STEP), and DDAV_FFN (the primary walk's fast-forward)
// must reach that walk's state, bit for bit.
//   g++ -O2 -std=c++17 -ffp-contract=off -I<csrc> dda_walk_check.cpp
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>

#include "dda.h"

using namespace zrt;

// PK_BM_TEST=1: the brick-major packed words (dda.h; the step macros name PK_BM)
#ifndef PK_BM_TEST
#define PK_BM_TEST 0
#endif
constexpr bool PK_BM = PK_BM_TEST != 0;

struct TestGrid {
    float bmin[3], bmax[3], cs[3];
    uint32_t res[3];
};

static uint64_t g_walk_fails = 0, g_walk_steps = 0;

// DDAW_STEP (the unpacked walk) against DDA_STEP, step by step: cells,
// linear index, crossing flag, T_EXIT and the next crossing ts bit for bit;
// and DDAV_STEPX (the packed walks, per-grid field widths) the same way: the
// packed word equals the cell's packing (and, on power-of-two grids, the
// linear index), the crossing flag, T_EXIT = EXITED ? +inf : TC and the ts bit
// for bit up to the exit step (past it the packed fields may carry; the walk
// has ended there), and the in-brick index of the park walk's OccX test;
// DDAV_STEPM (the same step on lane masks) must equal DDAV_STEPX bit for bit.
static void walk_w(const GridK& k, Dda s) {
    DdaW w;
    ddaw_from(s, k, w);
    const uint32_t res[3] = {k.rm0 + 1, k.rm1 + 1, k.rm2 + 1};
    PackK pk;
    const bool packs = pack_layout(res, pk, PK_BM);
    if (!packs || pk.bm != (uint32_t)PK_BM) {    // (brick-major words pack power-of-two grids only)
        if (!PK_BM) ++g_walk_fails;
        return;
    }
    const bool linear = pack_is_linear(res, pk);
    DdaV x;
    ddav_from(s, k, pk, x);
    DdaV y = x;                              // DDAV_STEPM (lane-mask form of the park walk trip)
    for (int guard = 0; guard < 100000; ++guard) {
        bool c1, c2, c4, ex4;
        float e1, e2, tc4;
        const uint32_t pc_before = x.pc;
        DDA_STEP(s, k, 2, c1, e1);
        DDAW_STEP(w, 2, c2, e2);
        DDAV_STEPX(x, pk, pk.low2, c4, ex4, tc4);
        LaneM ex5;
        float tc5;
        const bool y_in_step = y.pc == pc_before;
        DDAV_STEPM(y, pk.f0, pk.f1, pk.f2, ex5, tc5);
        if (!y_in_step || ex5 != ex4 || memcmp(&tc5, &tc4, 4) || y.pc != x.pc || memcmp(&y.tn0, &x.tn0, 4) ||
            memcmp(&y.tn1, &x.tn1, 4) || memcmp(&y.tn2, &x.tn2, 4)) {
            ++g_walk_fails;
            return;
        }
        ++g_walk_steps;
        const bool same = c1 == c2 && !memcmp(&e1, &e2, 4) && s.c0 == w.c0 && s.c1 == w.c1 && s.c2 == w.c2 &&
                          s.lin == w.lin && !memcmp(&s.tn0, &w.tn0, 4) && !memcmp(&s.tn1, &w.tn1, 4) &&
                          !memcmp(&s.tn2, &w.tn2, 4);
        const float e4 = ex4 ? kInf : tc4;
        bool same_v = !memcmp(&e1, &e4, 4) && !memcmp(&s.tn0, &x.tn0, 4) && !memcmp(&s.tn1, &x.tn1, 4) &&
                      !memcmp(&s.tn2, &x.tn2, 4);
        if (e1 != kInf) {
            const uint32_t kk = (((x.pc & pk.low2) * pk.kmul) >> pk.kshr) & 63u;
            const uint32_t kw = (s.c0 & 3u) | (s.c1 & 3u) << 2 | (s.c2 & 3u) << 4;
            same_v = same_v && c1 == c4 && x.pc == pack_cellv(pk, s.c0, s.c1, s.c2) && kk == kw &&
                     (!linear || x.pc == s.lin);
        }
        if (!same || !same_v) {
            ++g_walk_fails;
            return;
        }
        if (e1 == kInf) return;
    }
}

// DDAV_FFN (the primary walk's fast-forward) against the cell walk: from
// random points of the walk, the packed state after every crossing with
// t < tau must be the cell walk's state after its steps with TC < tau (ts bit
// for bit, same cell), and EXITED must be set exactly when the cell walk meets
// its exit crossing among them.
static uint64_t g_ff_fails = 0, g_ff = 0, g_ff_steps = 0;
static void walk_ff(const GridK& k, const Dda& s0, std::mt19937_64& rng) {
    const uint32_t res[3] = {k.rm0 + 1, k.rm1 + 1, k.rm2 + 1};
    PackK pk;
    if (!pack_layout(res, pk, PK_BM) || pk.bm != (uint32_t)PK_BM || s0.neg >= 8u) return;
    Dda q = s0;
    for (int guard = 0; guard < 100000; ++guard) {
        if (rng() % 3 == 0) {                       // fast-forward from here
            DdaV xn;
            ddav_from(q, k, pk, xn);
            const float tmin = fminf(q.tn0, fminf(q.tn1, q.tn2));
            const float dmin = fminf(q.td0, fminf(q.td1, q.td2));
            const float tau = tmin + (float)(1 + rng() % 120) * dmin;
            bool exitedn;
            DDAV_FFN(xn, pk, pk.f0, pk.f1, pk.f2, tau, exitedn);
            Dda r = q;                              // the cell walk: steps with TC < tau
            bool rexit = false;
            for (int g2 = 0; g2 < 100000; ++g2) {
                Dda t = r;
                bool cr;
                float te;
                DDA_STEP(t, k, 2, cr, te);
                const float tc = fminf(r.tn0, fminf(r.tn1, r.tn2));   // the step's crossing t
                if (!(tc < tau)) break;
                if (te == kInf) { rexit = true; break; }
                r = t;
                ++g_ff_steps;
            }
            ++g_ff;
            if (exitedn != rexit ||
                (!exitedn && (xn.pc != pack_cellv(pk, r.c0, r.c1, r.c2) || memcmp(&xn.tn0, &r.tn0, 4) ||
                              memcmp(&xn.tn1, &r.tn1, 4) || memcmp(&xn.tn2, &r.tn2, 4)))) {
                ++g_ff_fails;
                return;
            }
        }
        bool cr;
        float te;
        DDA_STEP(q, k, 2, cr, te);
        if (te == kInf) return;
    }
}

int main(int argc, char** argv) {
    const int n_grids = argc > 1 ? atoi(argv[1]) : 40;
    const int n_rays = argc > 2 ? atoi(argv[2]) : 4000;
    std::mt19937_64 rng(12345);
    std::uniform_real_distribution<float> U(0.0f, 1.0f);
    uint64_t total = 0, ties = 0, g_layout_grids = 0;
    for (int gi = 0; gi < n_grids; ++gi) {
        TestGrid g;
        const bool pow2 = gi % 3 == 0;     // exact arithmetic -> many crossing ties
        for (int a = 0; a < 3; ++a) {
            g.res[a] = gi == 0 ? 128u : 1u + (uint32_t)(rng() % 40);
            if (PK_BM && gi % 2 == 1) g.res[a] = 4u << (rng() % 5);   // (grids the brick-major words pack)
            g.bmin[a] = pow2 ? 0.0f : -5.0f + 10.0f * U(rng);
            g.cs[a] = pow2 ? 0.25f : 0.05f + U(rng);
            g.bmax[a] = g.bmin[a] + g.cs[a] * (float)g.res[a];
        }
        // one discarded draw per 4^3 brick (they were a brick occupancy once):
        // the rays below stay the ones every earlier run of this check drew
        for (size_t b = (size_t)((g.res[0] + 3) / 4) * ((g.res[1] + 3) / 4) * ((g.res[2] + 3) / 4); b > 0; --b)
            (void)U(rng);
        GridK k{g.res[0] - 1, g.res[1] - 1, g.res[2] - 1, g.res[0], g.res[0] * g.res[1]};
        {   // grids whose packed words take this build's layout (the packed-word checks run on them)
            PackK pk;
            if (pack_layout(g.res, pk, PK_BM) && pk.bm == (uint32_t)PK_BM) ++g_layout_grids;
        }
        for (int r = 0; r < n_rays; ++r) {
            v3 o, d;
            const int kind = r % 4;
            float c[3];
            for (int a = 0; a < 3; ++a) {
                const float ext = g.bmax[a] - g.bmin[a];
                c[a] = g.bmin[a] - 0.5f * ext + 2.0f * ext * U(rng);
                if (kind >= 2) c[a] = g.bmin[a] + g.cs[a] * (float)(rng() % (g.res[a] + 1));   // on cell corners
            }
            o = mk(c[0], c[1], c[2]);
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
            if (!dda_init(g.bmin, g.bmax, g.res, g.cs, o, d, s)) continue;
            ++total;
            if (s.tn0 == s.tn1 || s.tn1 == s.tn2 || s.tn0 == s.tn2) ++ties;
            walk_w(k, s);
            walk_ff(k, s, rng);
        }
    }
    const uint64_t fails = g_walk_fails + g_ff_fails;
    printf("{\"rays\": %llu, \"tie_starts\": %llu, \"walk_steps\": %llu, \"walk_fails\": %llu, \"ff\": %llu, "
           "\"ff_steps\": %llu, \"ff_fails\": %llu, \"layout_grids\": %llu, \"fails\": %llu}\n",
           (unsigned long long)total, (unsigned long long)ties, (unsigned long long)g_walk_steps,
           (unsigned long long)g_walk_fails, (unsigned long long)g_ff, (unsigned long long)g_ff_steps,
           (unsigned long long)g_ff_fails, (unsigned long long)g_layout_grids, (unsigned long long)fails);
    return fails ? 1 : 0;
}
