// Host check of the escape table keyed by sub-brick regions (csrc/escape.h
// EscShape): on random anisotropic grids (blobs and planes; among them 8^3,
// 12 x 5 x 9 and 16 x 16 x 4, so that clipped edge regions and both packed
// layouts' grids occur) and random rays walked cell by cell with the kernels'
// f32 DDA (DDA_STEP), the walk asks once per 4^3 brick it enters, for the
// region that holds the cell it is in when it asks (the park kernel asks at the
// end of a trip, up to a few cells into the brick: the ray's delay).
//   (a) no occupied cell is visited after an escape point;
//   (b) a region's bit is set wherever its brick's bit is;
//   (c) the 4 x 4 x 4 shape is esc_compute's table, bit for bit;
//   (d) controls: the same walk over tables built without the one-cell
//       dilation, and over tables built for a region's first cell only, must
//       find violations (the check can fail).
// What the dilation is for, and the rays that show it.  Without it a start
// box's region in slab i ends at ceil(hi_b + kb (i + 1 - lo_a) (u_hi + kEscEps)):
// the ray through the box's edge (lo_a, hi_b) with the bin's last slope u_hi
// runs along it.  A walk leaves it only where its f32 crossing times put the
// b crossing before the a crossing that exactly comes first, so it needs
//   * a ray on a bin's edge through a cell corner: the face ties (+-1, +-1,
//     +-1), u_hi = 1, from corner origins;
//   * cells for which that ray's two crossings nearly coincide but the slope
//     margin does not reach the next cell: nearly cubic ones, kb = 1 / 1.002
//     (kNearCube), where the crossings are 0.002 (i + 1) cells apart and the
//     margin kEscEps = 0.001 a cell is half of that;
//   * crossing times coarser than that gap: an origin 2^18 cell sizes away
//     (kFarLog2) has t in [2^18, 2^19) cells, one ulp of it is 1/32 of a cell,
//     and the sums t + dt of a 20-cell walk stay within a third of a cell of
//     the line, well inside the dilation.
// The last four grids have such cells, and two ray classes in five on them are
// such rays; a tenth of every grid's rays start as far away.  The other grids'
// rays alone (cells of unrelated sizes, origins near the grid) find nothing
// without the dilation: there the slope margin covers the walk's rounding.
//   g++ -O2 -std=c++17 -ffp-contract=off -I<csrc> -I<include> escape_region_check.cpp
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "dda.h"
#include "escape.h"

using namespace zrt;

namespace {

struct TGrid {
    uint32_t res[3], nb[3];
    float bmin[3], bmax[3], cs[3];
    bool near_cube;
    std::vector<uint8_t> occ;
    std::vector<uint32_t> sat;
};

// near_cube: cells 0.2% and 0.4% longer along y and z than along x (kNearCube)
constexpr float kNearCube = 2e-3f;
constexpr int kFarLog2 = 18;           // a far ray starts 2^18 smallest-cell sizes before the point it aims at
void make_grid(std::mt19937_64& rng, const uint32_t res[3], bool near_cube, TGrid& g) {
    std::uniform_real_distribution<float> U(0.0f, 1.0f);
    g.near_cube = near_cube;
    for (int a = 0; a < 3; ++a) {
        g.res[a] = res[a];
        g.nb[a] = (res[a] + 3) / 4;
        g.bmin[a] = -5.0f + 10.0f * U(rng);
        g.cs[a] = 0.05f + U(rng);
        if (near_cube) g.cs[a] = g.cs[0] * (1.0f + kNearCube * (float)a);
        g.bmax[a] = g.bmin[a] + g.cs[a] * (float)res[a];
    }
    g.occ.assign((size_t)res[0] * res[1] * res[2], 0);
    const int nblob = 1 + (int)(rng() % 4);
    for (int k = 0; k < nblob; ++k) {
        uint32_t c[3], r[3];
        for (int a = 0; a < 3; ++a) { c[a] = rng() % res[a]; r[a] = rng() % (res[a] / 4 + 1); }
        const bool plane = k == 0 || rng() % 3 == 0;       // (every grid has a plane: rays skim it)
        if (plane) {
            const int ax = (int)(rng() % 3);
            r[ax] = 0;
            for (int a = 0; a < 3; ++a)
                if (a != ax) r[a] = res[a];
        }
        for (uint32_t z = c[2] > r[2] ? c[2] - r[2] : 0; z <= std::min(res[2] - 1, c[2] + r[2]); ++z)
            for (uint32_t y = c[1] > r[1] ? c[1] - r[1] : 0; y <= std::min(res[1] - 1, c[1] + r[1]); ++y)
                for (uint32_t x = c[0] > r[0] ? c[0] - r[0] : 0; x <= std::min(res[0] - 1, c[0] + r[0]); ++x)
                    if (plane || U(rng) < 0.4f) g.occ[((size_t)z * res[1] + y) * res[0] + x] = 1;
    }
    const uint32_t n0 = res[0] + 1, n1 = res[1] + 1, n2 = res[2] + 1;
    g.sat.assign((size_t)n0 * n1 * n2, 0);
    for (uint32_t z = 0; z < res[2]; ++z)
        for (uint32_t y = 0; y < res[1]; ++y)
            for (uint32_t x = 0; x < res[0]; ++x)
                g.sat[((size_t)(z + 1) * n1 + y + 1) * n0 + x + 1] = g.occ[((size_t)z * res[1] + y) * res[0] + x];
    for (uint32_t z = 0; z < n2; ++z)
        for (uint32_t y = 0; y < n1; ++y)
            for (uint32_t x = 1; x < n0; ++x) g.sat[((size_t)z * n1 + y) * n0 + x] += g.sat[((size_t)z * n1 + y) * n0 + x - 1];
    for (uint32_t z = 0; z < n2; ++z)
        for (uint32_t y = 1; y < n1; ++y)
            for (uint32_t x = 0; x < n0; ++x) g.sat[((size_t)z * n1 + y) * n0 + x] += g.sat[((size_t)z * n1 + y - 1) * n0 + x];
    for (uint32_t z = 1; z < n2; ++z)
        for (uint32_t y = 0; y < n1; ++y)
            for (uint32_t x = 0; x < n0; ++x) g.sat[((size_t)z * n1 + y) * n0 + x] += g.sat[((size_t)(z - 1) * n1 + y) * n0 + x];
}

// table[region][bin], regions as the device table orders them
enum Mode { kProof, kNoDilation, kFirstCell };
void build_table(const TGrid& g, const EscShape& h, Mode mode, std::vector<uint8_t>& tab) {
    const EscSat S{g.sat.data(), g.res[0] + 1, (g.res[0] + 1) * (g.res[1] + 1)};
    const uint32_t lg = esc_regions_lg(h), nbr = g.nb[0] * g.nb[1] * g.nb[2];
    tab.assign(((size_t)nbr << lg) * kEscNBin, 0);
    for (uint32_t rg = 0; rg < nbr << lg; ++rg) {
        const uint32_t br = rg >> lg, sub = rg & ((1u << lg) - 1u);
        const uint32_t bx = br % g.nb[0], by = (br / g.nb[0]) % g.nb[1], bz = br / (g.nb[0] * g.nb[1]);
        for (uint32_t bin = 0; bin < kEscNBin; ++bin) {
            bool e;
            if (mode == kFirstCell) {
                uint32_t c0[3], c1[3];
                e = esc_region_box(h, g.res, bx, by, bz, sub, c0, c1);
                for (int k = 0; k < 3; ++k) c1[k] = c0[k] + 1;
                e = e && esc_compute_box(S, g.res, g.cs, c0, c1, bin);
            } else {
                e = esc_compute_region(S, g.res, g.cs, h, bx, by, bz, sub, bin, mode == kNoDilation ? 0.0 : 1.0);
            }
            tab[(size_t)rg * kEscNBin + bin] = e;
        }
    }
}

}  // namespace

int main(int argc, char** argv) {
    const int n_rays = argc > 1 ? atoi(argv[1]) : 12000;      // per grid and shape
    std::mt19937_64 rng(4242);
    std::uniform_real_distribution<float> U(0.0f, 1.0f);
    const uint32_t fixed[][3] = {{8, 8, 8}, {12, 5, 9}, {16, 16, 4}, {16, 16, 16}, {7, 13, 6}};
    const uint32_t shapes[][3] = {{4, 4, 4}, {2, 2, 2}, {1, 1, 1}, {1, 4, 1}, {4, 1, 1}, {1, 1, 4}, {2, 4, 1}, {4, 2, 2}};
    const int n_shapes = (int)(sizeof shapes / sizeof shapes[0]);
    const int n_grids = 13, n_near_cube = 4;                  // the last four: nearly cubic cells
    int rc = 0;
    // the shape rule and the park walk's key: the masks pick esc_sub_of's
    // sub-index for every in-brick cell, the long axis is the smallest cell's
    uint64_t key_fails = 0;
    for (int m = 0; m < 3; ++m) {
        float cs[3] = {0.5f, 0.5f, 0.5f};
        cs[m] = 0.25f;
        const EscShape h = esc_shape_for(cs);
        const uint32_t l[3] = {h.l0, h.l1, h.l2};
        for (int a = 0; a < 3; ++a) key_fails += l[a] != (a == m ? 2u : 0u);
        const uint32_t key = esc_walk_key(h);
        key_fails += (key & 0xFFu) != esc_regions_lg(h);
        for (uint32_t i = 0; i < 64; ++i) key_fails += esc_key_sub(key, i) != esc_sub_of(h, i);
    }
    {
        const float cube[3] = {0.5f, 0.5f, 0.5f};
        key_fails += esc_shape_for(cube).l0 != 2u || esc_walk_key(kEscBrick) != 0u || esc_regions_lg(kEscBrick) != 0u;
        for (uint32_t i = 0; i < 64; ++i) key_fails += esc_key_sub(0u, i) != 0u || esc_sub_of(kEscBrick, i) != 0u;
    }
    printf("{\"key_fails\": %llu}\n", (unsigned long long)key_fails);
    if (key_fails) rc = 1;
    std::vector<TGrid> grids(n_grids);
    for (int gi = 0; gi < n_grids; ++gi) {
        uint32_t res[3];
        for (int a = 0; a < 3; ++a) res[a] = gi < 5 ? fixed[gi][a] : 4u + (uint32_t)(rng() % 17);
        make_grid(rng, res, gi >= n_grids - n_near_cube, grids[gi]);
    }
    for (int si = 0; si < n_shapes; ++si) {
        const EscShape h{esc_log2(shapes[si][0]), esc_log2(shapes[si][1]), esc_log2(shapes[si][2])};
        const uint32_t lg = esc_regions_lg(h);
        uint64_t rays = 0, steps = 0, queries = 0, escapes = 0, saved = 0, unsound = 0, subset_fails = 0, brick_diff = 0;
        uint64_t bits_set = 0, bits = 0, brick_bits_set = 0, clipped = 0;
        uint64_t ctl_nodil = 0, ctl_first = 0;
        for (int gi = 0; gi < n_grids; ++gi) {
            const TGrid& g = grids[gi];
            const EscSat S{g.sat.data(), g.res[0] + 1, (g.res[0] + 1) * (g.res[1] + 1)};
            std::vector<uint8_t> tab[3];
            build_table(g, h, kProof, tab[0]);
            build_table(g, h, kNoDilation, tab[1]);
            build_table(g, h, kFirstCell, tab[2]);
            const uint32_t nbr = g.nb[0] * g.nb[1] * g.nb[2];
            for (uint32_t br = 0; br < nbr; ++br) {
                const uint32_t bx = br % g.nb[0], by = (br / g.nb[0]) % g.nb[1], bz = br / (g.nb[0] * g.nb[1]);
                for (uint32_t bin = 0; bin < kEscNBin; ++bin) {
                    const bool eb = esc_compute(S, g.res, g.cs, bx, by, bz, bin);
                    brick_bits_set += eb;
                    for (uint32_t sub = 0; sub < 1u << lg; ++sub) {
                        uint32_t c0[3], c1[3];
                        const bool in = esc_region_box(h, g.res, bx, by, bz, sub, c0, c1);
                        const bool e = tab[0][(((size_t)br << lg) + sub) * kEscNBin + bin];
                        if (!in) {                                  // a region past the grid's edge: no bit
                            clipped += bin == 0;
                            subset_fails += e;
                            continue;
                        }
                        ++bits;
                        bits_set += e;
                        if (eb && !e) ++subset_fails;               // (b)
                        if (lg == 0 && e != eb) ++brick_diff;       // (c)
                    }
                }
            }
            const GridK k{g.res[0] - 1, g.res[1] - 1, g.res[2] - 1, g.res[0], g.res[0] * g.res[1]};
            for (int r = 0; r < n_rays; ++r) {
                // the rays the dilation is for (see the header): on nearly cubic
                // cells, two classes in five run along a face tie through a
                // cell corner from far away
                const bool graze = g.near_cube && (r % 5 == 0 || r % 5 == 3);
                float c[3];
                for (int a = 0; a < 3; ++a) {
                    const float ext = g.bmax[a] - g.bmin[a];
                    c[a] = r % 3 == 0 ? g.bmin[a] - 0.5f * ext + 2.0f * ext * U(rng) : g.bmin[a] + ext * U(rng);
                    if (r % 7 == 0 || graze) c[a] = g.bmin[a] + g.cs[a] * (float)(rng() % (g.res[a] + 1));   // on cell corners
                }
                v3 d;
                if (r % 5 == 0 || graze) {                          // face ties
                    d = normalize(mk((rng() & 1) ? 1.0f : -1.0f, (rng() & 1) ? 1.0f : -1.0f, (rng() & 1) ? 1.0f : -1.0f));
                } else if (r % 5 == 1) {                            // through the lattice's corners
                    d = normalize(mk((rng() & 1) ? g.cs[0] : -g.cs[0], (rng() & 1) ? g.cs[1] : -g.cs[1],
                                     (rng() & 1) ? g.cs[2] : -g.cs[2]));
                } else if (r % 5 == 2) {                            // skimming: one small component
                    float v[3] = {U(rng) - 0.5f, U(rng) - 0.5f, U(rng) - 0.5f};
                    v[rng() % 3] *= 0.02f;
                    d = normalize(mk(v[0], v[1], v[2]));
                } else {
                    d = normalize(mk(U(rng) - 0.5f, U(rng) - 0.5f, U(rng) - 0.5f));
                }
                if (r % 10 == 0 || graze) {                         // from far away: the walk's t are coarse
                    const float far = ldexpf(fminf(g.cs[0], fminf(g.cs[1], g.cs[2])), kFarLog2);
                    for (int a = 0; a < 3; ++a) c[a] -= far * (a == 0 ? d.x : (a == 1 ? d.y : d.z));
                }
                Dda s0;
                if (!dda_init(g.bmin, g.bmax, g.res, g.cs, mk(c[0], c[1], c[2]), d, s0)) continue;
                ++rays;
                const bool usable = s0.neg < 8u;
                const uint32_t bin = esc_dir_bin(d);
                const uint32_t delay = (uint32_t)(r % 4);          // cells into a brick before the walk asks
                for (int t = 0; t < 3; ++t) {                       // the proof's table, then the controls
                    Dda s = s0;
                    bool escaped = false;
                    uint32_t eb = ~0u, asked = ~0u, wait = 0;
                    for (int guard = 0; guard < 100000; ++guard) {
                        const bool o = g.occ[((size_t)s.c2 * g.res[1] + s.c1) * g.res[0] + s.c0] != 0;
                        if (t == 0) ++steps;
                        if (escaped) {
                            if (t == 0) ++saved;
                            if (o) {
                                ++(t == 0 ? unsound : (t == 1 ? ctl_nodil : ctl_first));
                                break;
                            }
                        }
                        const uint32_t br = ((s.c2 / 4) * g.nb[1] + s.c1 / 4) * g.nb[0] + s.c0 / 4;
                        if (br != eb) { eb = br; wait = delay; }
                        if (!escaped && usable && asked != br && wait-- == 0u) {
                            asked = br;
                            const uint32_t sub = esc_sub_of(h, (s.c0 & 3u) | ((s.c1 & 3u) << 2) | ((s.c2 & 3u) << 4));
                            if (t == 0) ++queries;
                            if (tab[t][(((size_t)br << lg) + sub) * kEscNBin + bin]) {
                                escaped = true;
                                if (t == 0) ++escapes;
                            }
                        }
                        bool crossed;
                        float te;
                        DDA_STEP(s, k, 2, crossed, te);
                        (void)crossed;
                        if (te == kInf) break;
                    }
                }
            }
        }
        printf("{\"shape\": [%u, %u, %u], \"rays\": %llu, \"steps\": %llu, \"queries\": %llu, \"escapes\": %llu, "
               "\"steps_after_escape\": %llu, \"bits_set\": %.4f, \"brick_bits_set\": %llu, \"clipped_regions\": %llu, "
               "\"unsound\": %llu, \"subset_fails\": %llu, \"brick_diff\": %llu, \"control_no_dilation\": %llu, "
               "\"control_first_cell\": %llu}\n",
               shapes[si][0], shapes[si][1], shapes[si][2], (unsigned long long)rays, (unsigned long long)steps,
               (unsigned long long)queries, (unsigned long long)escapes, (unsigned long long)saved,
               bits ? (double)bits_set / bits : 0.0, (unsigned long long)brick_bits_set, (unsigned long long)clipped,
               (unsigned long long)unsound, (unsigned long long)subset_fails, (unsigned long long)brick_diff,
               (unsigned long long)ctl_nodil, (unsigned long long)ctl_first);
        if (unsound || subset_fails || brick_diff) rc = 1;
    }
    return rc;
}
