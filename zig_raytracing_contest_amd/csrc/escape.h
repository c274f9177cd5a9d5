// Escape table for the park walk (render.hip wf_park_kernel), shared by the
// device build kernel and the host check tests/cpp/escape_check.cpp.
//
// traceRay (stage3.zig:152-185) tests the triangles of every cell the DDA
// visits until nearest <= t_next_crossing.  If no cell after the current one
// holds a triangle, nothing after it can change the result: the walk may
// stop there with the nearest hit so far (a miss stays +inf).  The table
// proves that conservatively, per start box B (a 4^3 brick, or a region of
// one: EscShape below) and direction bin:
//   * a bin is a cone of directions: the dominant axis a and its sign (the
//     cube face), and the slopes u = d_b / |d_a|, v = d_c / |d_a| of the
//     other two axes in one of kEscBins x kEscBins cells of [-1, 1]^2;
//   * the bit is set when the region swept by every ray that starts in B with
//     a direction in the cone (its slopes widened by kEscEps), dilated by one
//     cell on every side, holds no occupied cell of the grid.
// A DDA walk is the ray's line up to f32 rounding, far below a cell, so every
// cell it visits after one in B lies in that region: a set bit means every
// later cell is empty.  Rays whose crossing sequences start at -inf / NaN (a
// zero direction component on a cell boundary, Dda.neg bit 3) never use it.
//
// The region is tested slab by slab along a: the cells of slab i that the
// cone can reach form a rectangle in the other two axes, and a summed-area
// table of cell occupancy answers "any occupied cell in it" with 8 loads.
#pragma once
#include <stdint.h>

#include "zrt_math.h"

namespace zrt {

#ifndef ZRT_ESC_BINS
#define ZRT_ESC_BINS 8
#endif
constexpr uint32_t kEscBins = ZRT_ESC_BINS;                    // per face axis
constexpr uint32_t kEscNBin = 6 * kEscBins * kEscBins;         // 384 bins (r04q: 8 x 8 per face vs 4 x 4: cfg3 +0.9%)
constexpr uint32_t kEscWords = kEscNBin <= 128 ? 4 : (kEscNBin + 31) / 32;   // u32 words per brick
constexpr double kEscEps = 1e-3;                               // slope margin of a bin's cone

// The bin of a direction (any consistent face choice on |d_a| ties: both
// faces' cones hold the direction, their slopes reach +-1 + kEscEps).
ZHD uint32_t esc_dir_bin(v3 d) {
    const float ax = fabsf(d.x), ay = fabsf(d.y), az = fabsf(d.z);
    uint32_t a;
    float m, u, v;
    // (the slopes need not be exact: a bin's cone is kEscEps wider than its
    // cell, far more than the reciprocal's error)
#if defined(__HIP_DEVICE_COMPILE__)
#define ZRT_ESC_RCP(x) __builtin_amdgcn_rcpf(x)
#else
#define ZRT_ESC_RCP(x) (1.0f / (x))
#endif
    if (ax >= ay && ax >= az) { a = 0; m = d.x; const float r = ZRT_ESC_RCP(ax); u = d.y * r; v = d.z * r; }
    else if (ay >= az) { a = 1; m = d.y; const float r = ZRT_ESC_RCP(ay); u = d.x * r; v = d.z * r; }
    else { a = 2; m = d.z; const float r = ZRT_ESC_RCP(az); u = d.x * r; v = d.y * r; }
#undef ZRT_ESC_RCP
    const uint32_t f = 2u * a + (m < 0.0f ? 1u : 0u);
    const float fb = (float)kEscBins;
    const uint32_t iu = (uint32_t)fminf(fmaxf((u + 1.0f) * 0.5f * fb, 0.0f), fb - 1.0f);
    const uint32_t iv = (uint32_t)fminf(fmaxf((v + 1.0f) * 0.5f * fb, 0.0f), fb - 1.0f);
    return (f * kEscBins + iu) * kEscBins + iv;
}

// Summed-area table of cell occupancy, (res0 + 1) x (res1 + 1) x (res2 + 1):
// S[z][y][x] = occupied cells in [0, x) x [0, y) x [0, z).
struct EscSat {
    const uint32_t* s;
    uint32_t n0, n01;      // res0 + 1, (res0 + 1) (res1 + 1)
};
// occupied cells in the inclusive cell box [x0, x1] x [y0, y1] x [z0, z1]
ZHD uint32_t esc_box(const EscSat& S, uint32_t x0, uint32_t x1, uint32_t y0, uint32_t y1, uint32_t z0, uint32_t z1) {
    const uint64_t X0 = x0, X1 = x1 + 1ull, Y0 = (uint64_t)y0 * S.n0, Y1 = (uint64_t)(y1 + 1) * S.n0;
    const uint64_t Z0 = (uint64_t)z0 * S.n01, Z1 = (uint64_t)(z1 + 1) * S.n01;
    return S.s[Z1 + Y1 + X1] - S.s[Z1 + Y1 + X0] - S.s[Z1 + Y0 + X1] + S.s[Z1 + Y0 + X0] - S.s[Z0 + Y1 + X1] +
           S.s[Z0 + Y1 + X0] + S.s[Z0 + Y0 + X1] - S.s[Z0 + Y0 + X0];
}

// A grid with a zero-extent (or non-finite) axis -- every triangle in one
// plane, Grid.init's cell_size 0 (linalg.zig:412-441) -- has walks whose
// crossings on that axis do not advance t, which the cell-unit geometry below
// does not model: such grids get no proof (no escape bit, no frustum bound).
ZHD bool esc_cells_regular(const float cs[3]) {
    return cs[0] > 0.0f && cs[1] > 0.0f && cs[2] > 0.0f && cs[0] < kInf && cs[1] < kInf && cs[2] < kInf;
}

// The bit of the start box of cells [c0, c1) (per axis, inside the grid) and
// `bin`: the header's proof with that box for B.  `dil`: the dilation in
// cells, 1 everywhere but in the host check's control (0: walks whose f32
// crossing times are coarse then leave the region along a bin's edge,
// tests/cpp/escape_region_check.cpp).
ZHD bool esc_compute_box(const EscSat& S, const uint32_t res[3], const float cs[3], const uint32_t c0[3],
                         const uint32_t c1[3], uint32_t bin, double dil = 1.0) {
    if (!esc_cells_regular(cs)) return false;
    const uint32_t fc = bin / (kEscBins * kEscBins), iu = (bin / kEscBins) % kEscBins, iv = bin % kEscBins;
    const int a = (int)(fc / 2u), sg = (fc & 1u) ? -1 : 1;
    const int b = a == 0 ? 1 : 0, c = a == 2 ? 1 : 2;
    const double nb = (double)kEscBins;
    const double u0 = -1.0 + 2.0 * iu / nb - kEscEps, u1 = -1.0 + 2.0 * (iu + 1) / nb + kEscEps;
    const double v0 = -1.0 + 2.0 * iv / nb - kEscEps, v1 = -1.0 + 2.0 * (iv + 1) / nb + kEscEps;
    double lo[3], hi[3];
    for (int k = 0; k < 3; ++k) {
        lo[k] = (double)c0[k];
        hi[k] = (double)c1[k];
    }
    // a cell-unit step along a moves cs_a / cs_b cells along b
    const double kb = (double)cs[a] / (double)cs[b], kc = (double)cs[a] / (double)cs[c];
    const int ra = (int)res[a];
    for (int i = sg > 0 ? (int)lo[a] : (int)hi[a] - 1; i >= 0 && i < ra; i += sg) {
        double smin, smax;                      // a-distance from the brick to slab i
        if (sg > 0) { smin = fmax(0.0, i - hi[a]); smax = fmax(0.0, i + 1.0 - lo[a]); }
        else { smin = fmax(0.0, lo[a] - (i + 1.0)); smax = fmax(0.0, hi[a] - i); }
        const double ylo = lo[b] + kb * fmin(smin * u0, smax * u0), yhi = hi[b] + kb * fmax(smin * u1, smax * u1);
        const double zlo = lo[c] + kc * fmin(smin * v0, smax * v0), zhi = hi[c] + kc * fmax(smin * v1, smax * v1);
        // the cells the interval touches, one more on each side
        const double yf0 = floor(ylo) - dil, yf1 = ceil(yhi) - 1.0 + dil;
        const double zf0 = floor(zlo) - dil, zf1 = ceil(zhi) - 1.0 + dil;
        if (yf1 < 0.0 || yf0 > res[b] - 1.0 || zf1 < 0.0 || zf0 > res[c] - 1.0) {
            // the region lies beside the grid in this slab; it only moves
            // further out when neither slope range straddles 0 on that side
            const bool out_y = (yf1 < 0.0 && u1 <= 0.0) || (yf0 > res[b] - 1.0 && u0 >= 0.0);
            const bool out_z = (zf1 < 0.0 && v1 <= 0.0) || (zf0 > res[c] - 1.0 && v0 >= 0.0);
            if (out_y || out_z) break;
            continue;
        }
        const uint32_t y0 = (uint32_t)fmax(0.0, yf0), y1 = (uint32_t)fmin(res[b] - 1.0, yf1);
        const uint32_t z0 = (uint32_t)fmax(0.0, zf0), z1 = (uint32_t)fmin(res[c] - 1.0, zf1);
        uint32_t lo3[3], hi3[3];
        lo3[a] = hi3[a] = (uint32_t)i;
        lo3[b] = y0; hi3[b] = y1;
        lo3[c] = z0; hi3[c] = z1;
        if (esc_box(S, lo3[0], hi3[0], lo3[1], hi3[1], lo3[2], hi3[2]) != 0u) return false;
    }
    return true;
}
// The bit of brick (bx, by, bz) and `bin`: the brick's cells as the start box.
ZHD bool esc_compute(const EscSat& S, const uint32_t res[3], const float cs[3], uint32_t bx, uint32_t by,
                     uint32_t bz, uint32_t bin) {
    const uint32_t B[3] = {bx, by, bz};
    uint32_t c0[3], c1[3];
    for (int k = 0; k < 3; ++k) {
        c0[k] = 4u * B[k];
        c1[k] = 4u * B[k] + 4u < res[k] ? 4u * B[k] + 4u : res[k];
    }
    return esc_compute_box(S, res, cs, c0, c1, bin);
}

// Start regions smaller than the brick.  The smaller the start box, the
// narrower its swept region and the more bits are set: rays that skim a
// ground plane leave a 4^3 brick's dilated region (6 cells wide) through
// occupied cells, a single cell's (3 wide) often not.  A brick is cut into
// regions of 2^l0 x 2^l1 x 2^l2 cells (EscShape, each l in 0..2; {2, 2, 2} is
// the brick itself), and the table holds kEscWords words per region, a
// brick's regions together: region (brick br, sub-index sub) at word
// (br * esc_regions + sub) * kEscWords.  The walk still asks once per brick
// entered, for the region that holds the cell it is in: every cell it visits
// after that cell lies in that region's swept cone, dilated (the proof above
// with the region for B), so a set bit ends the walk as a brick's does.  A
// region is a subset of its brick, its swept region in every slab a subset of
// the brick's (every bound above is monotone in the box), so a region's bit
// is set wherever its brick's is.
struct EscShape {
    uint32_t l0, l1, l2;
};
constexpr uint32_t esc_log2(uint32_t g) { return g == 4u ? 2u : (g == 2u ? 1u : 0u); }
constexpr EscShape kEscBrick = {2u, 2u, 2u};
// log2 of the regions per brick
ZHD constexpr uint32_t esc_regions_lg(const EscShape& h) { return 6u - h.l0 - h.l1 - h.l2; }
// The sub-index of the region that holds the brick's cell i = x | y << 2 | z << 4.
ZHD constexpr uint32_t esc_sub_of(const EscShape& h, uint32_t i) {
    return ((i & 3u) >> h.l0) | ((((i >> 2) & 3u) >> h.l1) << (2u - h.l0)) |
           ((((i >> 4) & 3u) >> h.l2) << (4u - h.l0 - h.l1));
}
// The cells [c0, c1) of region `sub` of brick (bx, by, bz), clipped to the
// grid; false: the region lies outside it (no cell, no walk ever asks).
ZHD bool esc_region_box(const EscShape& h, const uint32_t res[3], uint32_t bx, uint32_t by, uint32_t bz, uint32_t sub,
                        uint32_t c0[3], uint32_t c1[3]) {
    const uint32_t B[3] = {bx, by, bz}, l[3] = {h.l0, h.l1, h.l2};
    const uint32_t s[3] = {sub & ((4u >> h.l0) - 1u), (sub >> (2u - h.l0)) & ((4u >> h.l1) - 1u),
                           sub >> (4u - h.l0 - h.l1)};
    for (int k = 0; k < 3; ++k) {
        c0[k] = 4u * B[k] + (s[k] << l[k]);
        if (c0[k] >= res[k]) return false;
        c1[k] = c0[k] + (1u << l[k]) < res[k] ? c0[k] + (1u << l[k]) : res[k];
    }
    return true;
}
// The shape a context builds: one cell along the two axes with the larger
// cells, the brick's four along the axis with the smallest (the first such
// axis): 16 regions per brick.  On the contest stand-in (128^3, 1 x 4 x 1)
// against the brick-level table, full frames, alternating processes:
// 1 x 4 x 1 +2.6%, 1 x 1 x 1 +2.7% at 4 times the memory and build time,
// 2 x 2 x 2 +1.4% (profiles/r10).
ZHD EscShape esc_shape_for(const float cs[3]) {
    int m = 0;
    for (int k = 1; k < 3; ++k)
        if (cs[k] < cs[m]) m = k;
    return EscShape{m == 0 ? 2u : 0u, m == 1 ? 2u : 0u, m == 2 ? 2u : 0u};
}
// What the park walk needs of the table's shape, in one word (WfParams::esc_key):
// lg = log2 of the regions per brick in bits [0, 8), and two masks that pick
// the sub-index out of the in-brick cell index i = x | y << 2 | z << 4:
//     sub = (i & m_lo) | ((i >> 2) & m_hi), m_lo in bits [8, 16), m_hi from 16.
// 0: the brick-level table.  For esc_shape_for's shapes and the brick only
// (of the three axes' 2-bit groups two are kept whole).
ZHD uint32_t esc_walk_key(const EscShape& h) {
    if (h.l0 == 2u && h.l1 == 0u && h.l2 == 0u) return 4u | (0u << 8) | (15u << 16);
    if (h.l0 == 0u && h.l1 == 2u && h.l2 == 0u) return 4u | (3u << 8) | (12u << 16);
    if (h.l0 == 0u && h.l1 == 0u && h.l2 == 2u) return 4u | (15u << 8) | (0u << 16);
    return 0u;
}
ZHD uint32_t esc_key_sub(uint32_t key, uint32_t i) { return (i & ((key >> 8) & 0xFFu)) | ((i >> 2) & (key >> 16)); }
ZHD bool esc_compute_region(const EscSat& S, const uint32_t res[3], const float cs[3], const EscShape& h, uint32_t bx,
                            uint32_t by, uint32_t bz, uint32_t sub, uint32_t bin, double dil = 1.0) {
    uint32_t c0[3], c1[3];
    if (!esc_region_box(h, res, bx, by, bz, sub, c0, c1)) return false;
    return esc_compute_box(S, res, cs, c0, c1, bin, dil);
}

// Primary-ray frustum bound (the primary launch, render.hip frustum_kernel).
// Every camera ray of the pixel block [u0, u1) x [v0, v1) (pixel x + jitter,
// stage3.zig:234-238) starts at the camera origin o with direction
// normalize(llc + right u + up v): the points o + s D(u, v), s >= 0, form a
// cone over the parallelogram of D's, and its slice s in [s0, s1] is the
// convex hull of the eight corner points.  Marching slices of about two cells
// along the cone's dominant axis, the first slice whose box (dilated by one
// cell) holds an occupied cell ends the march: every point of the block's
// rays with normalized t < s0 |D|min lies in earlier, empty slices, so a walk
// may fast-forward (DDAV_FFN) over every crossing below that t.  +inf: the cone
// meets no occupied cell at all, so every ray of the block misses
// (traceRay's +inf).  0: no bound (a degenerate cone).
// hi: the march goes on to the last slice [s0, s1] that holds an occupied
// cell: every point of the block's rays with t >= s1 |D|max lies in later,
// empty slices, so once the walk has tested a cell whose exit crossing is at
// or past hi no later cell can change the result (+inf: no bound).
// [ga, gb]: the longest run of at least kFrustumGapSlices empty slices
// between occupied ones, as t: every point of the block's rays with t in
// [ga, gb] lies in it (ga = s_start |D|max rounded up, gb = s_end |D|min
// rounded down), so a walk that enters a cell at a crossing in [ga, gb) may
// fast-forward over every crossing below gb (+inf, +inf: no gap).
constexpr int kFrustumGapSlices = 2;
struct FrustumBound {
    float lo, hi, ga, gb;
};
ZHD bool s_far_finite(double x) { return x * 0.0 == 0.0; }

// The block's cone: corner directions, |D| bounds, the march's slice width
// along the dominant axis and its end (frustum_bound; frustum_kernel runs the
// slices over a wave's lanes with the same arithmetic).
struct FrustumCone {
    double D[4][3];
    double dmin, dmax, s_far, ds;
    bool ok;
};
ZHD FrustumCone frustum_cone(const float bmin[3], const float bmax[3], const float cs[3], const float org[3],
                             const float llc[3], const float right[3], const float up[3], double u0, double u1,
                             double v0, double v1) {
    FrustumCone q;
    q.ok = false;
    q.dmax = 0.0;
    q.s_far = q.ds = 0.0;
    const double uu[2] = {u0, u1}, vv[2] = {v0, v1};
    double dmin = 1e300, mid[3] = {0, 0, 0};
    for (int c = 0; c < 4; ++c) {
        double n2 = 0.0;
        for (int k = 0; k < 3; ++k) {
            q.D[c][k] = (double)llc[k] + (double)right[k] * uu[c & 1] + (double)up[k] * vv[c >> 1];
            n2 += q.D[c][k] * q.D[c][k];
            mid[k] += 0.25 * q.D[c][k];
        }
        dmin = fmin(dmin, sqrt(n2));
        q.dmax = fmax(q.dmax, sqrt(n2));
    }
    // |D| over the parallelogram >= the corners' least |D| minus its diagonals
    double rl = 0.0, ul = 0.0;
    for (int k = 0; k < 3; ++k) {
        rl += (double)right[k] * right[k];
        ul += (double)up[k] * up[k];
    }
    dmin -= sqrt(rl) * (u1 - u0) + sqrt(ul) * (v1 - v0);
    q.dmin = dmin;
    if (!(dmin > 0.0) || !esc_cells_regular(cs)) return q;
    // beyond s_far every point of the cone is farther from o than any grid point
    double far2 = 0.0;
    for (int k = 0; k < 3; ++k) {
        const double a = fabs((double)bmin[k] - org[k]), b = fabs((double)bmax[k] - org[k]);
        far2 += fmax(a, b) * fmax(a, b);
    }
    q.s_far = sqrt(far2) / dmin;
    int ax = 0;
    for (int k = 1; k < 3; ++k)
        if (fabs(mid[k]) / cs[k] > fabs(mid[ax]) / cs[ax]) ax = k;
    q.ds = 2.0 * (double)cs[ax] / fmax(fabs(mid[ax]), 1e-30);
    // the march must reach s_far within its 2^16 slices
    q.ok = q.ds > 0.0 && s_far_finite(q.s_far) && (double)(1 << 16) * q.ds > q.s_far;
    return q;
}
// Slice it of the march: [it ds, it ds + ds]; whether its box (the eight
// corner points, dilated by one cell) holds an occupied cell.
ZHD bool frustum_slice(const EscSat& S, const FrustumCone& q, const uint32_t res[3], const float bmin[3],
                       const float cs[3], const float org[3], int it) {
    const double s0 = it * q.ds, s1 = s0 + q.ds;
    double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
    for (int c = 0; c < 4; ++c)
        for (int k = 0; k < 3; ++k) {
            const double p0 = org[k] + s0 * q.D[c][k], p1 = org[k] + s1 * q.D[c][k];
            lo[k] = fmin(lo[k], fmin(p0, p1));
            hi[k] = fmax(hi[k], fmax(p0, p1));
        }
    uint32_t c0[3], c1[3];
    if (!esc_cells_regular(cs)) return true;                  // (no bound: frustum_cone refuses these)
    for (int k = 0; k < 3; ++k) {
        const double a = floor((lo[k] - bmin[k]) / cs[k]) - 1.0, b = floor((hi[k] - bmin[k]) / cs[k]) + 1.0;
        if (b < 0.0 || a > res[k] - 1.0) return false;
        c0[k] = (uint32_t)fmax(0.0, a);
        c1[k] = (uint32_t)fmin(res[k] - 1.0, b);
    }
    return esc_box(S, c0[0], c1[0], c0[1], c1[1], c0[2], c1[2]) != 0u;
}
// lo and hi from the first and last occupied slices (-1: none).
ZHD void frustum_finish(const FrustumCone& q, int first, int last, FrustumBound& fb) {
    if (first < 0) {
        fb.lo = kInf;
        return;
    }
    const double tl = (first * q.ds) * q.dmin, th = (last * q.ds + q.ds) * q.dmax;
    fb.lo = (float)tl;
    if ((double)fb.lo > tl) fb.lo = nextafterf(fb.lo, 0.0f);     // round down
    fb.hi = (float)th;
    if ((double)fb.hi < th) fb.hi = nextafterf(fb.hi, kInf);     // round up
}
ZHD FrustumBound frustum_bound(const EscSat& S, const uint32_t res[3], const float bmin[3], const float bmax[3],
                               const float cs[3], const float org[3], const float llc[3], const float right[3],
                               const float up[3], double u0, double u1, double v0, double v1) {
    FrustumBound fb{0.0f, kInf, kInf, kInf};
    const FrustumCone q = frustum_cone(bmin, bmax, cs, org, llc, right, up, u0, u1, v0, v1);
    if (!q.ok) return fb;                                          // no bound
    int first = -1, last = -1, gap_it = -1, best0 = 0, best1 = 0, run = 0;
    double best_len = -1.0;
    for (int it = 0; it < 1 << 16 && !(it * q.ds > q.s_far); ++it) {
        if (frustum_slice(S, q, res, bmin, cs, org, it)) {
            const double len = (it * q.ds) * q.dmin - (gap_it * q.ds) * q.dmax;
            if (first >= 0 && run >= kFrustumGapSlices && len > best_len) {
                best_len = len;
                best0 = gap_it;
                best1 = it;
            }
            if (first < 0) first = it;
            last = it;
            run = 0;
        } else {
            if (run == 0) gap_it = it;
            ++run;
        }
    }
    frustum_finish(q, first, last, fb);
    if (first >= 0 && best_len > 0.0) {
        const double ta = (best0 * q.ds) * q.dmax, tb = (best1 * q.ds) * q.dmin;
        float ga = (float)ta, gb = (float)tb;
        if ((double)ga < ta) ga = nextafterf(ga, kInf);          // round up
        if ((double)gb > tb) gb = nextafterf(gb, 0.0f);          // round down
        if (ga < gb) {
            fb.ga = ga;
            fb.gb = gb;
        }
    }
    return fb;
}

// ---------------------------------------------------------------------------
// Back-face cull masks (context.hip bfc_build_kernel, the park kernel's first
// cell; tests/cpp/bfcull_check.cpp).
//
// tri_ray rejects a ref as soon as det = dot(e1, cross(d, e2)) < 1e-8.  Per
// (cell, direction bin) the table holds one u32: bit r stays set when ref r of
// the cell must still be tested for some direction of the bin; a cleared bit
// means det < 1e-8 for EVERY direction the device can assign to the bin, so
// the test could only have been rejected.  Cells of more than 32 refs keep
// all ones (as the entry-face masks do).
//
// Bins: esc_dir_bin's, merged kEscBins / kBfcBins to a side (a coarse bin's
// cone is the union of its fine bins' cones, widened by kEscEps like them).
// esc_dir_bin computes the slopes u = d_b * rcp(|d_a|) and the cell index
// floor((u + 1) * 0.5 * K) in f32: a reciprocal within 2 ulp and four
// roundings of values <= K move the index boundary by less than 3e-6 in u,
// far inside kEscEps = 1e-3; that needs a normal dominant component with a
// normal reciprocal, which bfc_dir_ok guarantees (and the caller checks).
//
// The bound.  With D = d / |d_a| = (+-1, u, v) (dominant axis first) and
// s = |d_a| > 0, the exact determinant is s * det(D), and det(D) =
// -(e1 x e2) . D is linear in (u, v).  tri_ray evaluates it in f32 without
// contraction: each of the six products e1_i * (d_j * e2_k) passes through at
// most five roundings (d_j e2_k, the subtraction, the product with e1_i, two
// additions), so
//     |det_f32 - s det(D)| <= ((1 + 2^-24)^5 - 1) s S(D) + 9 * 2^-126,
//     S(D) = sum_i |e1_i| (|D_j| |e2_k| + |D_k| |e2_j|)
// (the last term: every operation that underflows adds at most 2^-126,
// flushed or not).  S scales with |e1| |e2| |D|, not with |e1 x e2|: a
// sliver's normal is tiny, its rounding error is not.  g(D) = det(D) +
// kBfcMargin S(D), kBfcMargin = 2^-21 = 8 * 2^-24, is convex in (u, v)
// (linear plus a sum of absolute values of linear forms), so its maximum over
// the bin's square is at a corner.  The four corners are evaluated in double
// (relative error 2^-50 of S, inside the 3 * 2^-24 of slack over the five
// roundings); if g < 0 at all four, det_f32 <= s g(D) + 9 * 2^-126 < 1e-8 for
// every d of the cone.  No intermediate may overflow either: with the
// caller's |d_x| + |d_y| + |d_z| <= 4 (bfc_dir_ok) every partial sum is below
// 4 S (1 + 2^-20), so S <= 2^120 at the corners keeps them finite.  A ref
// with a non-finite edge component is never culled.
#ifndef ZRT_BFC_BINS
#define ZRT_BFC_BINS 4
#endif
constexpr uint32_t kBfcBins = ZRT_BFC_BINS;                    // per face axis
static_assert(kBfcBins >= 1 && kEscBins % kBfcBins == 0, "a cull bin is a union of escape bins");
constexpr uint32_t kBfcNBin = 6 * kBfcBins * kBfcBins;         // u32 words per cell
constexpr double kBfcMargin = 0x1p-21;

// The cull bin of esc_dir_bin's bin.
ZHD uint32_t bfc_bin_of(uint32_t esc_bin) {
    constexpr uint32_t q = kEscBins / kBfcBins;
    const uint32_t f = esc_bin / (kEscBins * kEscBins), iu = (esc_bin / kEscBins) % kEscBins, iv = esc_bin % kEscBins;
    return (f * kBfcBins + iu / q) * kBfcBins + iv / q;
}
// Directions the masks hold for: finite, dominant component normal with a
// normal reciprocal (>= 3.3e-31), components within the overflow bound above.
ZHD bool bfc_dir_ok(v3 d) {
    const float s = (fabsf(d.x) + fabsf(d.y)) + fabsf(d.z);
    return s >= 1e-30f && s <= 4.0f;                           // (a NaN fails both)
}
// Whether the ref with edges e1, e2 can be skipped for every direction of
// cull bin `bin`.  margin and eps are kBfcMargin and kEscEps everywhere but in
// the host check's controls (0: the check must then find violations).
ZHD bool bfc_cull(const float e1[3], const float e2[3], uint32_t bin, double margin = kBfcMargin,
                  double eps = kEscEps) {
    for (int k = 0; k < 3; ++k)
        if (!(fabsf(e1[k]) < kInf) || !(fabsf(e2[k]) < kInf)) return false;
    const uint32_t fc = bin / (kBfcBins * kBfcBins), iu = (bin / kBfcBins) % kBfcBins, iv = bin % kBfcBins;
    const int a = (int)(fc / 2u), b = a == 0 ? 1 : 0, c = a == 2 ? 1 : 2;
    const double nb = (double)kBfcBins;
    const double uu[2] = {-1.0 + 2.0 * iu / nb - eps, -1.0 + 2.0 * (iu + 1) / nb + eps};
    const double vv[2] = {-1.0 + 2.0 * iv / nb - eps, -1.0 + 2.0 * (iv + 1) / nb + eps};
    const double ax = e1[0], ay = e1[1], az = e1[2], bx = e2[0], by = e2[1], bz = e2[2];
    for (int k = 0; k < 4; ++k) {
        double D[3];
        D[a] = (fc & 1u) ? -1.0 : 1.0;
        D[b] = uu[k & 1];
        D[c] = vv[k >> 1];
        const double det = ax * (D[1] * bz - D[2] * by) + ay * (D[2] * bx - D[0] * bz) + az * (D[0] * by - D[1] * bx);
        const double S = fabs(ax) * (fabs(D[1] * bz) + fabs(D[2] * by)) + fabs(ay) * (fabs(D[2] * bx) + fabs(D[0] * bz)) +
                         fabs(az) * (fabs(D[0] * by) + fabs(D[1] * bx));
        if (!(S <= 0x1p120) || !(det + margin * S < 0.0)) return false;
    }
    return true;
}

// ---------------------------------------------------------------------------
// The direction-aware escape table (context.hip context_escape; host check
// tests/cpp/escape_dir_check.cpp).
//
// The table above ends a walk only when no later cell HOLDS a ref.  But a ref
// that bfc_cull rejects for a bin's whole cone cannot pass tri_ray for any ray
// of that bin: a cell whose every ref is rejected that way cannot change
// `nearest`, a tie or the break test, so for that bin it is an empty cell.
// The region table is therefore built from one occupancy per cull bin
// (kBfcNBin of them, each serving its (kEscBins / kBfcBins)^2 escape bins,
// whose cones lie inside the cull bin's): a cell is occupied for the bin iff
// it holds at least one ref that bfc_cull cannot reject (esc_dir_occupied; no
// 32-ref limit, refs with non-finite edges or S > 2^120 are never rejected).
// esc_compute_box runs unchanged on that occupancy's summed-area table.
// Soundness is the header's argument with one more line: every cell the ray
// visits from its start region on lies in the swept region, and every cell
// there is empty or holds only refs with det_f32 < 1e-8 for every direction
// of the cone, so no test there can pass and the hit so far stands.  Unlike
// the plain table's, the start region itself may hold such refs, so a bit can
// be set for a ray that starts on a surface and leaves it.  The cone argument
// needs the direction inside bfc_cull's domain: a ray with !bfc_dir_ok(d)
// never uses a bit (the park kernel's emask).  Plain occupancy is the union
// over bins, every bound is monotone in the occupancy, so every bit of the
// plain table is set in this one.
// The brick-level table, its density statistic and the gate stay plain.
// Cull bins, not the 384 escape bins' own narrower cones: a quarter of the
// transient volumes and prefix passes; on the contest stand-in the cull bins
// already reject 37% of the (ref, bin) pairs (tools/escape_sim.cpp).
//
// Whether a ray may use the table at all: Dda.neg without bit 3 (the header's
// -inf / NaN crossing sequences) and a direction inside bfc_cull's domain.
ZHD bool esc_ray_usable(uint32_t neg, v3 d) { return neg < 8u && bfc_dir_ok(d); }
// Whether the cell with refs [rb, re) is occupied for cull bin `cb`;
// edges(r, e1, e2) gives ref r's edges as tri_ray reads them.
template <class Edges>
ZHD bool esc_dir_occupied(uint32_t rb, uint32_t re, Edges edges, uint32_t cb, double margin = kBfcMargin,
                          double eps = kEscEps) {
    for (uint32_t r = rb; r < re; ++r) {
        float e1[3], e2[3];
        edges(r, e1, e2);
        if (!bfc_cull(e1, e2, cb, margin, eps)) return true;
    }
    return false;
}
// The q-th escape bin served by cull bin `cb`, q < (kEscBins / kBfcBins)^2
// (bfc_bin_of's inverse).
constexpr uint32_t kEscPerCull = (kEscBins / kBfcBins) * (kEscBins / kBfcBins);
ZHD uint32_t esc_bin_of_cull(uint32_t cb, uint32_t q) {
    constexpr uint32_t m = kEscBins / kBfcBins;
    const uint32_t f = cb / (kBfcBins * kBfcBins), cu = (cb / kBfcBins) % kBfcBins, cv = cb % kBfcBins;
    return (f * kEscBins + cu * m + q / m) * kEscBins + cv * m + q % m;
}

}  // namespace zrt
