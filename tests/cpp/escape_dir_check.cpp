// Host check of the direction-aware escape table (csrc/escape.h
// esc_dir_occupied; context.hip builds the same table on the device): small
// anisotropic grids (8^3, 12 x 5 x 9, 16 x 16 x 4 among them) of a few hundred
// triangles each -- a ground, a wall that faces away from most bounce rays,
// boxes, slivers, a coincident opposite-facing pair, zero-area triangles,
// triangles with NaN / inf edges -- and over 10^5 rays per grid: rays that
// start on a triangle's surface inside an occupied cell and leave it as a
// bounce ray does, random rays, axis-parallel and zero-component directions,
// unnormalised and non-finite ones.  Every ray is binned five times, with the
// slope's reciprocal moved by -2 .. +2 ulp (the device's v_rcp_f32).
//
// The walk is the sequential traceRay (stage3.zig:152-185) with the kernels'
// f32 DDA.  It asks the table in EVERY cell it visits, its start cell
// included, before the cell is tested (the park kernel asks once per brick
// entered, a subset).  For every ray, bin and cell whose bit is set:
//   (a) the walk truncated before that cell returns the full walk's
//       (t, u, v, ref), bit for bit  ("unsound_result");
//   (b) the lemma the proof rests on: no cell from there on holds a ref whose
//       f32 determinant, as tri_ray evaluates it for this ray, passes
//       det >= 1e-8 (or is NaN)  ("unsound_lemma": implies (a)).
// Also:
//   (c) every bit of the plain table is set in the direction-aware one;
//   (d) controls: the same walks over a table built with the cull margin at 0
//       and over one built with unwidened cull cones must break the lemma.
//       What breaks them is rare, so each grid holds the triangles and rays
//       that do it.  Margin: a large triangle whose first edge runs along a
//       corner direction of a cull bin's cone, so that det is 0 there up to
//       rounding, with rays along that corner.  Widening: a wall whose plane
//       holds the dominant axis and is tilted by 1e-8 against a bin boundary
//       at slope 0, so that it is rejected for every slope >= 0, with rays of
//       slope -2.9e-8: u + 1 rounds to 1, the device bins them with slope 0;
//   (e) a direction outside bfc_dir_ok never uses a bit (esc_ray_usable);
//   (f) against a vacuous pass: at least 20% of a grid's surface-start rays are
//       ended in their start cell.
//   g++ -O2 -std=c++17 -ffp-contract=off -I<csrc> -I<include> escape_dir_check.cpp
#include <algorithm>
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

using Gen = std::mt19937_64;
double uni(Gen& g, double a, double b) { return a + (b - a) * (double)(g() >> 11) * 0x1p-53; }

float ulps(float x, int n) {
    for (; n > 0; --n) x = nextafterf(x, kInf);
    for (; n < 0; ++n) x = nextafterf(x, -kInf);
    return x;
}
// esc_dir_bin with the reciprocal moved by p ulp (p = 0 is esc_dir_bin itself)
uint32_t dir_bin_rcp(v3 d, int p) {
    const float ax = fabsf(d.x), ay = fabsf(d.y), az = fabsf(d.z);
    uint32_t a;
    float m, u, v;
    if (ax >= ay && ax >= az) { a = 0; m = d.x; const float r = ulps(1.0f / ax, p); u = d.y * r; v = d.z * r; }
    else if (ay >= az) { a = 1; m = d.y; const float r = ulps(1.0f / ay, p); u = d.x * r; v = d.z * r; }
    else { a = 2; m = d.z; const float r = ulps(1.0f / az, p); u = d.x * r; v = d.y * r; }
    const uint32_t f = 2u * a + (m < 0.0f ? 1u : 0u);
    const float fb = (float)kEscBins;
    const uint32_t iu = (uint32_t)fminf(fmaxf((u + 1.0f) * 0.5f * fb, 0.0f), fb - 1.0f);
    const uint32_t iv = (uint32_t)fminf(fmaxf((v + 1.0f) * 0.5f * fb, 0.0f), fb - 1.0f);
    return (f * kEscBins + iu) * kEscBins + iv;
}

struct Tri {
    double p[3][3];       // vertices
    bool surf;            // rays may start on it
    bool has_e;           // the controls': the edges below as they are (v1 - v0 in f32 would round their tilt away)
    float e1[3], e2[3];
};
struct Ray {
    v3 o, d;
    bool surf;
};

struct Scene {
    uint32_t res[3], nb[3];
    float bmin[3], bmax[3], cs[3];
    int up;
    std::vector<float> tp;          // 9 per ref: v0, e1, e2
    std::vector<uint32_t> cells;    // 2 per cell
    std::vector<Tri> tris;
    std::vector<Ray> aimed;         // the controls' rays
    EscShape h;
};

void quad(std::vector<Tri>& out, const double a[3], const double b[3], const double c[3], const double d[3], bool surf) {
    Tri t{};
    t.surf = surf;
    for (int k = 0; k < 3; ++k) { t.p[0][k] = a[k]; t.p[1][k] = b[k]; t.p[2][k] = c[k]; }
    out.push_back(t);
    for (int k = 0; k < 3; ++k) { t.p[0][k] = a[k]; t.p[1][k] = c[k]; t.p[2][k] = d[k]; }
    out.push_back(t);
}

// the corner (iu + su, iv + sv) of cull bin cb's cone, widened by eps, as a direction
void cull_corner(uint32_t cb, int su, int sv, double eps, double D[3]) {
    const uint32_t fc = cb / (kBfcBins * kBfcBins), iu = (cb / kBfcBins) % kBfcBins, iv = cb % kBfcBins;
    const int a = (int)(fc / 2u), b = a == 0 ? 1 : 0, c = a == 2 ? 1 : 2;
    D[a] = (fc & 1u) ? -1.0 : 1.0;
    D[b] = -1.0 + 2.0 * (iu + su) / kBfcBins + (su ? eps : -eps);
    D[c] = -1.0 + 2.0 * (iv + sv) / kBfcBins + (sv ? eps : -eps);
}

// kind 0: the scene; 1: one triangle of the margin control alone; 2: one wall of the widening control alone
void make_scene(Gen& g, const uint32_t res[3], int kind, Scene& S) {
    int up = 0;
    for (int a = 1; a < 3; ++a)
        if (res[a] < res[up]) up = a;
    if (res[0] == res[1] && res[1] == res[2]) up = 1;
    S.up = up;
    const int s1 = (up + 1) % 3, s2 = (up + 2) % 3;
    double ext[3];
    for (int a = 0; a < 3; ++a) {
        S.res[a] = res[a];
        S.nb[a] = (res[a] + 3) / 4;
        S.bmin[a] = (float)uni(g, -50, 50);
        S.cs[a] = (float)uni(g, 2.0, 4.5);
        S.bmax[a] = S.bmin[a] + S.cs[a] * (float)res[a];
        ext[a] = (double)S.cs[a] * res[a];
    }
    S.h = esc_shape_for(S.cs);
    auto at = [&](double fu, double f1, double f2, double* o) {
        o[up] = S.bmin[up] + fu * ext[up];
        o[s1] = S.bmin[s1] + f1 * ext[s1];
        o[s2] = S.bmin[s2] + f2 * ext[s2];
    };
    // winding: (a, b, c, d) with b - a along s1 and d - a along s2 has the
    // normal s1 x s2 = +up for a cyclic (up, s1, s2)
    std::vector<Tri>& T = S.tris;
    double a[3], b[3], c[3], d[3];
    const double csm = fmin(S.cs[0], fmin(S.cs[1], S.cs[2]));
    if (kind == 0) {
    // the ground: a quad low in the lowest cell layer, facing up
    const double gy = 0.3 / res[up];
    // (8 x 8 quads)
    for (int i = 0; i < 8; ++i)
        for (int j = 0; j < 8; ++j) {
            const double x0 = 0.02 + 0.12 * i, x1 = x0 + 0.12, z0 = 0.02 + 0.12 * j, z1 = z0 + 0.12;
            at(gy, x0, z0, a); at(gy, x1, z0, b); at(gy, x1, z1, c); at(gy, x0, z1, d);
            quad(T, a, b, c, d, true);
        }
    // a wall along one side, standing on the ground, facing outwards (away
    // from the rays that bounce off the ground)
    at(gy, 0.04, 0.04, a); at(0.2, 0.04, 0.04, b); at(0.2, 0.4, 0.04, c); at(gy, 0.4, 0.04, d);
    quad(T, a, b, c, d, true);
    // a coincident opposite-facing pair, standing
    at(gy, 0.15, 0.8, a); at(0.15, 0.15, 0.8, b); at(0.15, 0.15, 0.95, c); at(gy, 0.15, 0.95, d);
    quad(T, a, b, c, d, true);
    quad(T, a, d, c, b, true);
    // low boxes' tops and sides, slivers, zero-area and non-finite triangles near the ground
    for (int k = 0; k < 40; ++k) {
        const double f1 = uni(g, 0.1, 0.9), f2 = uni(g, 0.1, 0.9), w = uni(g, 0.01, 0.06), hh = uni(g, gy, gy + 0.08);
        at(hh, f1, f2, a); at(hh, f1 + w, f2, b); at(hh, f1 + w, f2 + w, c); at(hh, f1, f2 + w, d);
        quad(T, a, b, c, d, true);
    }
    // (in one corner: none of them can be rejected, each blocks the regions around it)
    for (int k = 0; k < 12; ++k) {
        Tri t{};
        t.surf = false;
        double o[3];
        at(uni(g, gy, gy + 0.05), uni(g, 0.05, 0.2), uni(g, 0.8, 0.95), o);
        const int kind = k % 4;
        double e1[3], e2[3];
        for (int j = 0; j < 3; ++j) { e1[j] = uni(g, -1, 1) * 0.03 * ext[j]; e2[j] = uni(g, -1, 1) * 0.03 * ext[j]; }
        if (kind == 0) for (int j = 0; j < 3; ++j) e2[j] = 1.5 * e1[j] + 1e-6 * e2[j];          // sliver
        if (kind == 1) for (int j = 0; j < 3; ++j) e2[j] = (k & 4) ? 0.0 : 2.0 * e1[j];         // zero area
        for (int j = 0; j < 3; ++j) { t.p[0][j] = o[j]; t.p[1][j] = o[j] + e1[j]; t.p[2][j] = o[j] + e2[j]; }
        if (kind == 2) {                                                                        // non-finite
            const double bad[] = {(double)kInf, -(double)kInf, (double)NAN, 3e38};
            t.p[1 + (k & 1)][g() % 3u] = bad[g() % 4u];
        }
        T.push_back(t);
    }
    }
    // the margin control: per triangle a cull bin's widened corner direction
    // Dc, e1 = L Dc, e2 = L (n x Dc) / |n x Dc| with n's slope components
    // pointing into the cone: det(D) = -|e1|^2 n . D <= 0 over the cone, 0 at Dc
    for (int k = 0; k < (kind == 1 ? 1 : 0); ++k) {
        const uint32_t cb = (uint32_t)(g() % kBfcNBin);
        const int su = (int)(g() & 1), sv = (int)(g() & 1);
        double Dc[3];
        cull_corner(cb, su, sv, kEscEps, Dc);
        const uint32_t fc = cb / (kBfcBins * kBfcBins);
        const int ax = (int)(fc / 2u), bx = ax == 0 ? 1 : 0, cx = ax == 2 ? 1 : 2;
        double n[3];
        n[bx] = (su ? -1.0 : 1.0) * uni(g, 0.3, 1.0);
        n[cx] = (sv ? -1.0 : 1.0) * uni(g, 0.3, 1.0);
        n[ax] = -(n[bx] * Dc[bx] + n[cx] * Dc[cx]) / Dc[ax];
        double w[3] = {n[1] * Dc[2] - n[2] * Dc[1], n[2] * Dc[0] - n[0] * Dc[2], n[0] * Dc[1] - n[1] * Dc[0]};
        const double wl = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]), dl = sqrt(Dc[0] * Dc[0] + Dc[1] * Dc[1] + Dc[2] * Dc[2]);
        const double L = uni(g, 0.8, 1.6) * csm;
        Tri t{};
        t.surf = false;
        double o[3];
        at(uni(g, 0.4, 0.6), uni(g, 0.4, 0.6), uni(g, 0.4, 0.6), o);
        // (a sliver: |e1 x e2| = 1e-6 |e1| |e2|, so that the rounding of det,
        // which scales with |e1| |e2|, outweighs det itself across the bin)
        t.has_e = true;
        for (int j = 0; j < 3; ++j) {
            t.e1[j] = (float)(L * Dc[j] / dl);
            t.e2[j] = (float)(L * (1.3 * Dc[j] / dl + 1e-6 * w[j] / wl));
            t.p[0][j] = o[j];
            t.p[1][j] = o[j] + t.e1[j];
            t.p[2][j] = o[j] + t.e2[j];
        }
        T.push_back(t);
        for (int r = 0; r < 400; ++r) {                    // rays along the corner, just inside the cone
            double D[3] = {Dc[0], Dc[1], Dc[2]};
            D[bx] += (su ? -1.0 : 1.0) * (kEscEps + uni(g, 0.0, 0.05));      // inside the bin itself, near the corner
            D[cx] += (sv ? -1.0 : 1.0) * (kEscEps + uni(g, 0.0, 0.05));
            const double f = uni(g, 0.05, 0.6), back = uni(g, 0.0, 1.0) * csm;
            Ray q;
            q.surf = false;
            const double sc = (g() & 1) ? 1.0 / dl : 1.0;
            q.d = mk((float)(D[0] * sc), (float)(D[1] * sc), (float)(D[2] * sc));
            q.o = mk((float)(o[0] + f * L * Dc[0] / dl - back * D[0] + 1e-4 * csm * n[0]),
                     (float)(o[1] + f * L * Dc[1] / dl - back * D[1] + 1e-4 * csm * n[1]),
                     (float)(o[2] + f * L * Dc[2] / dl - back * D[2] + 1e-4 * csm * n[2]));
            S.aimed.push_back(q);
        }
    }
    // the widening control: walls e1 = L c-axis, e2 = L (a-axis -+ 1e-8 b-axis):
    // n . D = +-L^2 (u +- 1e-8), rejected for every slope u >= 0 (or <= 0) of
    // the unwidened cone; rays with slope -+2.9e-8, which the device bins as 0
    for (int k0 = 0; k0 < (kind == 2 ? 1 : 0); ++k0) {
        const int k = (int)(g() % 32u);
        const int ax = k % 3, bx = (ax + 1 + (k / 3) % 2) % 3, cx = 3 - ax - bx;
        const double sa = (k & 8) ? -1.0 : 1.0, sb = 1.0;     // the ray's a sign; rejected for slopes >= 0 (u + 1 rounds
        // to 1 only from below 0 within the rays' 2.9e-8)
        const double L = uni(g, 0.8, 1.6) * csm;
        // e1 x e2 must have n_b = sb * (positive), n_a = 1e-8 * sa * (positive): rejected for sb * u >= 0
        double e1[3] = {0, 0, 0}, e2[3] = {0, 0, 0};
        e1[cx] = L;
        e2[ax] = L * sa;
        e2[bx] = -L * sb * 1e-8;
        // orient: n = e1 x e2; n . (sa, u, v) must be > 0 for sb u >= 0
        double n[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
        if (n[bx] * sb < 0.0) {
            for (int j = 0; j < 3; ++j) { const double x = e1[j]; e1[j] = e2[j]; e2[j] = x; }
            for (int j = 0; j < 3; ++j) n[j] = -n[j];
        }
        Tri t{};
        t.surf = false;
        double o[3];
        at(uni(g, 0.4, 0.6), uni(g, 0.4, 0.6), uni(g, 0.4, 0.6), o);
        // the wall's plane at b = 0 inside a cell, so that a ray can start 1e-9 L
        // from it and reach it: such rays HIT the wall the control's table skips
        S.bmin[bx] = -S.cs[bx] * ((float)(res[bx] / 2) + 0.37f);
        S.bmax[bx] = S.bmin[bx] + S.cs[bx] * (float)res[bx];
        o[bx] = 0.0;
        t.has_e = true;
        for (int j = 0; j < 3; ++j) {
            t.e1[j] = (float)e1[j];
            t.e2[j] = (float)e2[j];
            t.p[0][j] = o[j]; t.p[1][j] = o[j] + e1[j]; t.p[2][j] = o[j] + e2[j];
        }
        T.push_back(t);
        for (int r = 0; r < 400; ++r) {
            double D[3];
            D[ax] = sa;
            D[bx] = -sb * 2.9e-8;
            D[cx] = uni(g, -0.9, 0.9);
            const double f = uni(g, 0.1, 0.9), back = uni(g, 0.0, 1.0) * csm;
            Ray q;
            q.surf = false;
            q.d = mk((float)D[0], (float)D[1], (float)D[2]);
            double p[3];
            for (int j = 0; j < 3; ++j) p[j] = o[j] + f * 0.5 * (e1[j] + e2[j]) - back * D[j];
            p[bx] += sb * 1e-3 * csm;
            if (r & 1) {                                   // grazing hits
                for (int j = 0; j < 3; ++j) p[j] = o[j] + 0.3 * e1[j] + 0.2 * e2[j];
                p[bx] = sb * uni(g, 0.2, 1.0) * 1e-9 * L;
            }
            q.o = mk((float)p[0], (float)p[1], (float)p[2]);
            S.aimed.push_back(q);
        }
    }
    // refs per cell: every cell the triangle's box touches (a non-finite
    // triangle: the cell of its first vertex)
    const uint32_t ncell = res[0] * res[1] * res[2];
    std::vector<std::vector<uint32_t>> per(ncell);
    std::vector<float> pos(9 * T.size());
    for (size_t i = 0; i < T.size(); ++i) {
        float v[3][3];
        for (int k = 0; k < 3; ++k)
            for (int j = 0; j < 3; ++j) v[k][j] = (float)T[i].p[k][j];
        bool fin = true;
        uint32_t lo[3], hi[3];
        for (int j = 0; j < 3; ++j) {
            pos[9 * i + j] = v[0][j];
            pos[9 * i + 3 + j] = T[i].has_e ? T[i].e1[j] : v[1][j] - v[0][j];
            pos[9 * i + 6 + j] = T[i].has_e ? T[i].e2[j] : v[2][j] - v[0][j];
            const float mn = fminf(v[0][j], fminf(v[1][j], v[2][j])), mx = fmaxf(v[0][j], fmaxf(v[1][j], v[2][j]));
            fin = fin && std::isfinite(v[0][j]) && std::isfinite(v[1][j]) && std::isfinite(v[2][j]);
            const double l = floor(((double)mn - S.bmin[j]) / S.cs[j]), h = floor(((double)mx - S.bmin[j]) / S.cs[j]);
            lo[j] = (uint32_t)fmin(fmax(l, 0.0), res[j] - 1.0);
            hi[j] = (uint32_t)fmin(fmax(h, 0.0), res[j] - 1.0);
        }
        if (!fin)
            for (int j = 0; j < 3; ++j) {
                const double l = std::isfinite(v[0][j]) ? floor(((double)v[0][j] - S.bmin[j]) / S.cs[j]) : 0.0;
                lo[j] = hi[j] = (uint32_t)fmin(fmax(l, 0.0), res[j] - 1.0);
            }
        for (uint32_t z = lo[2]; z <= hi[2]; ++z)
            for (uint32_t y = lo[1]; y <= hi[1]; ++y)
                for (uint32_t x = lo[0]; x <= hi[0]; ++x) per[(z * res[1] + y) * res[0] + x].push_back((uint32_t)i);
    }
    S.cells.assign(2 * ncell, 0);
    for (uint32_t ci = 0; ci < ncell; ++ci) {
        S.cells[2 * ci] = (uint32_t)(S.tp.size() / 9);
        for (uint32_t i : per[ci]) S.tp.insert(S.tp.end(), pos.begin() + 9 * i, pos.begin() + 9 * i + 9);
        S.cells[2 * ci + 1] = (uint32_t)(S.tp.size() / 9);
    }
}

void sat_of(const Scene& S, const std::vector<uint8_t>& occ, std::vector<uint32_t>& sat) {
    const uint32_t* res = S.res;
    const uint32_t n0 = res[0] + 1, n1 = res[1] + 1, n2 = res[2] + 1;
    sat.assign((size_t)n0 * n1 * n2, 0);
    for (uint32_t z = 0; z < res[2]; ++z)
        for (uint32_t y = 0; y < res[1]; ++y)
            for (uint32_t x = 0; x < res[0]; ++x)
                sat[((size_t)(z + 1) * n1 + y + 1) * n0 + x + 1] = occ[((size_t)z * res[1] + y) * res[0] + x];
    for (uint32_t z = 0; z < n2; ++z)
        for (uint32_t y = 0; y < n1; ++y)
            for (uint32_t x = 1; x < n0; ++x) sat[((size_t)z * n1 + y) * n0 + x] += sat[((size_t)z * n1 + y) * n0 + x - 1];
    for (uint32_t z = 0; z < n2; ++z)
        for (uint32_t y = 1; y < n1; ++y)
            for (uint32_t x = 0; x < n0; ++x) sat[((size_t)z * n1 + y) * n0 + x] += sat[((size_t)z * n1 + y - 1) * n0 + x];
    for (uint32_t z = 1; z < n2; ++z)
        for (uint32_t y = 0; y < n1; ++y)
            for (uint32_t x = 0; x < n0; ++x) sat[((size_t)z * n1 + y) * n0 + x] += sat[((size_t)(z - 1) * n1 + y) * n0 + x];
}

// tab[region][bin] as the device orders it.  dir: one occupancy per cull bin
// (escape.h esc_dir_occupied) with the given margin and widening; else plain.
void build_table(const Scene& S, bool dir, double margin, double eps, std::vector<uint8_t>& tab) {
    const uint32_t ncell = S.res[0] * S.res[1] * S.res[2], nocc = dir ? kBfcNBin : 1u;
    std::vector<std::vector<uint32_t>> sat(nocc);
    std::vector<uint8_t> occ(ncell);
    for (uint32_t cb = 0; cb < nocc; ++cb) {
        for (uint32_t ci = 0; ci < ncell; ++ci) {
            const uint32_t rb = S.cells[2 * ci], re = S.cells[2 * ci + 1];
            occ[ci] = !dir ? rb < re : esc_dir_occupied(rb, re, [&](uint32_t r, float* e1, float* e2) {
                memcpy(e1, &S.tp[9ull * r + 3], 12);
                memcpy(e2, &S.tp[9ull * r + 6], 12);
            }, cb, margin, eps);
        }
        sat_of(S, occ, sat[cb]);
    }
    const uint32_t lg = esc_regions_lg(S.h), nbr = S.nb[0] * S.nb[1] * S.nb[2];
    tab.assign(((size_t)nbr << lg) * kEscNBin, 0);
    for (uint32_t rg = 0; rg < nbr << lg; ++rg) {
        const uint32_t br = rg >> lg, sub = rg & ((1u << lg) - 1u);
        const uint32_t bx = br % S.nb[0], by = (br / S.nb[0]) % S.nb[1], bz = br / (S.nb[0] * S.nb[1]);
        for (uint32_t bin = 0; bin < kEscNBin; ++bin) {
            const EscSat T{sat[dir ? bfc_bin_of(bin) : 0u].data(), S.res[0] + 1, (S.res[0] + 1) * (S.res[1] + 1)};
            tab[(size_t)rg * kEscNBin + bin] = esc_compute_region(T, S.res, S.cs, S.h, bx, by, bz, sub, bin);
        }
    }
}

v3 unit_vec(Gen& g) {
    for (;;) {
        const v3 u = mk((float)uni(g, -1, 1), (float)uni(g, -1, 1), (float)uni(g, -1, 1));
        if (dot(u, u) <= 1.0f && dot(u, u) > 1e-6f) return normalize(u);
    }
}

}  // namespace

int main(int argc, char** argv) {
    const int n_rays = argc > 1 ? atoi(argv[1]) : 120000;     // per scene (nine in ten meet the grid), beside the controls' aimed rays
    Gen g(977);
    // five scenes, then the controls' grids: one control triangle each, alone
    const uint32_t grids[][3] = {{8, 8, 8}, {12, 5, 9}, {16, 16, 4}, {16, 16, 16}, {10, 7, 13}};
    const int n_scenes = 5, n_controls = 16;
    int rc = 0;
    for (int gi = 0; gi < n_scenes + n_controls; ++gi) {
        const uint32_t* gr = grids[gi < n_scenes ? gi : (gi & 1)];
        const int kind = gi < n_scenes ? 0 : 1 + (gi & 1);
        Scene S;
        make_scene(g, gr, kind, S);
        std::vector<uint8_t> tab[4];                          // the proof's, margin 0, unwidened cones, plain
        build_table(S, true, kBfcMargin, kEscEps, tab[0]);
        build_table(S, true, 0.0, kEscEps, tab[1]);
        build_table(S, true, kBfcMargin, 0.0, tab[2]);
        build_table(S, false, 0.0, 0.0, tab[3]);
        uint64_t bits = tab[0].size(), bits_dir = 0, bits_plain = 0, subset_fails = 0;
        for (size_t i = 0; i < tab[0].size(); ++i) {
            bits_dir += tab[0][i];
            bits_plain += tab[3][i];
            subset_fails += tab[3][i] && !tab[0][i];
        }
        const uint32_t lg = esc_regions_lg(S.h);
        const GridK gk{S.res[0] - 1, S.res[1] - 1, S.res[2] - 1, S.res[0], S.res[0] * S.res[1]};
        std::vector<uint32_t> surf_tris;
        for (size_t i = 0; i < S.tris.size(); ++i)
            if (S.tris[i].surf) surf_tris.push_back((uint32_t)i);
        const float diag = sqrtf((S.bmax[0] - S.bmin[0]) * (S.bmax[0] - S.bmin[0]) + (S.bmax[1] - S.bmin[1]) * (S.bmax[1] - S.bmin[1]) +
                                 (S.bmax[2] - S.bmin[2]) * (S.bmax[2] - S.bmin[2]));
        uint64_t rays = 0, surf_rays = 0, surf_start_end = 0, surf_in_occupied = 0, escapes = 0, hits = 0;
        uint64_t unsound_result = 0, unsound_lemma = 0, ctl[2][2] = {{0, 0}, {0, 0}}, outside = 0, outside_used = 0;
        uint64_t moved_bins = 0;
        std::vector<uint32_t> vis;
        const int n_here = kind == 0 ? n_rays : n_rays / 50;
        const int total = n_here + (int)S.aimed.size();
        for (int r = 0; r < total; ++r) {
            Ray q;
            q.surf = false;
            if (r >= n_here) {
                q = S.aimed[r - n_here];
            } else if (r % 2 == 0 && !surf_tris.empty()) {
                // a bounce ray from a triangle's surface: on it, or lifted by
                // 1e-5 of the diagonal, about the normal of either side
                const Tri& t = S.tris[surf_tris[g() % surf_tris.size()]];
                double b0 = uni(g, 0, 1), b1 = uni(g, 0, 1);
                if (b0 + b1 > 1.0) { b0 = 1.0 - b0; b1 = 1.0 - b1; }
                const v3 A = mk((float)t.p[0][0], (float)t.p[0][1], (float)t.p[0][2]);
                const v3 e1 = sub(mk((float)t.p[1][0], (float)t.p[1][1], (float)t.p[1][2]), A);
                const v3 e2 = sub(mk((float)t.p[2][0], (float)t.p[2][1], (float)t.p[2][2]), A);
                v3 n = normalize(cross(e1, e2));
                if (r % 16 == 2) n = scale(n, -1.0f);         // (from the back side)
                q.o = add(A, add(scale(e1, (float)b0), scale(e2, (float)b1)));
                if (r % 4 == 0) q.o = add(q.o, scale(n, 1e-5f * diag));
                q.d = normalize(add(n, unit_vec(g)));
                q.surf = true;
            } else {
                double c[3];
                for (int a = 0; a < 3; ++a) {
                    const double ext = (double)S.bmax[a] - S.bmin[a];
                    c[a] = r % 3 == 0 ? S.bmin[a] - 0.5 * ext + 2.0 * ext * uni(g, 0, 1) : S.bmin[a] + ext * uni(g, 0, 1);
                    if (r % 7 == 0) c[a] = S.bmin[a] + S.cs[a] * (float)(g() % (S.res[a] + 1));   // on cell corners
                }
                q.o = mk((float)c[0], (float)c[1], (float)c[2]);
                const int kind = (r / 2) % 8;
                q.d = unit_vec(g);
                float* dv[3] = {&q.d.x, &q.d.y, &q.d.z};
                if (kind == 0) { *dv[g() % 3u] = 0.0f; }                                      // a zero component
                else if (kind == 1) { const int a = (int)(g() % 3u); for (int j = 0; j < 3; ++j) if (j != a) *dv[j] = 0.0f;
                                      *dv[a] = (g() & 1) ? 1.0f : -1.0f; }                    // axis-parallel
                else if (kind == 2) { q.d = scale(q.d, (float)uni(g, 2.5, 40.0)); }           // unnormalised, |d|_1 > 4 mostly
                else if (kind == 3 && r % 5 == 0) { const float bad[] = {kInf, -kInf, NAN, 1e-35f};
                                                    *dv[g() % 3u] = bad[g() % 4u]; }          // non-finite, tiny
                else if (kind == 4) { q.d = scale(q.d, (float)uni(g, 0.3, 1.3)); }
                else if (kind == 5) {                                                         // on a bin's edge, +- a few ulp
                    const int a = fabsf(q.d.x) >= fabsf(q.d.y) && fabsf(q.d.x) >= fabsf(q.d.z) ? 0 : (fabsf(q.d.y) >= fabsf(q.d.z) ? 1 : 2);
                    const int b = (a + 1 + (int)(g() & 1)) % 3;
                    const float edge = -1.0f + 2.0f * (float)(g() % (kEscBins + 1)) / (float)kEscBins;
                    *dv[b] = ulps(fabsf(*dv[a]) * edge, (int)(g() % 7u) - 3);
                }
            }
            Dda s0;
            if (!dda_init(S.bmin, S.bmax, S.res, S.cs, q.o, q.d, s0)) continue;
            ++rays;
            const bool dir_ok = bfc_dir_ok(q.d), usable = esc_ray_usable(s0.neg, q.d);
            if (!dir_ok) { ++outside; outside_used += usable; }
            // the full walk: the regions visited, the last cell that changed the
            // hit, the last cell holding a ref whose determinant test passes
            vis.clear();
            int last_change = -1, last_pass = -1;
            float nearest = kInf;
            {
                Dda s = s0;
                for (;;) {
                    const uint32_t br = ((s.c2 / 4) * S.nb[1] + s.c1 / 4) * S.nb[0] + s.c0 / 4;
                    const uint32_t sub = esc_sub_of(S.h, (s.c0 & 3u) | ((s.c1 & 3u) << 2) | ((s.c2 & 3u) << 4));
                    vis.push_back((br << lg) | sub);
                    for (uint32_t j = S.cells[2 * s.lin]; j < S.cells[2 * s.lin + 1]; ++j) {
                        const float* p = &S.tp[9ull * j];
                        const v3 e1 = mk(p[3], p[4], p[5]), e2 = mk(p[6], p[7], p[8]);
                        if (!(dot(e1, cross(q.d, e2)) < 0.00000001f)) last_pass = (int)vis.size() - 1;
                        float t, u, v;
                        if (tri_ray(mk(p[0], p[1], p[2]), e1, e2, q.o, q.d, &t, &u, &v) && nearest > t && t > 0.0f) {
                            nearest = t;
                            last_change = (int)vis.size() - 1;
                        }
                    }
                    bool crossed;
                    float t_exit;
                    DDA_STEP(s, gk, 2, crossed, t_exit);
                    (void)crossed;
                    if (nearest <= t_exit) break;
                }
            }
            hits += nearest < kInf;
            if (q.surf) {
                ++surf_rays;
                surf_in_occupied += S.cells[2 * s0.lin] < S.cells[2 * s0.lin + 1];
            }
            if (!usable) continue;
            uint32_t bins[5];
            int nb = 0;
            for (int p = -2; p <= 2; ++p) {
                const uint32_t b = dir_bin_rcp(q.d, p);
                if (std::find(bins, bins + nb, b) == bins + nb) bins[nb++] = b;
            }
            moved_bins += nb > 1;
            for (int t = 0; t < 3; ++t)
                for (int k = 0; k < nb; ++k) {
                    int first = -1;
                    for (size_t i = 0; i < vis.size() && first < 0; ++i)
                        if (tab[t][(size_t)vis[i] * kEscNBin + bins[k]]) first = (int)i;
                    if (first < 0) continue;
                    const bool bad_result = first <= last_change, bad_lemma = first <= last_pass;
                    if (t == 0) {
                        ++escapes;
                        unsound_result += bad_result;
                        unsound_lemma += bad_lemma;
                        if (q.surf && bins[k] == bins[0] && first == 0) ++surf_start_end;
                    } else {
                        ctl[t - 1][0] += bad_lemma;
                        ctl[t - 1][1] += bad_result;
                    }
                }
        }
        printf("{\"kind\": %d, \"grid\": [%u, %u, %u], \"refs\": %llu, \"rays\": %llu, \"hits\": %llu, \"escapes\": %llu, "
               "\"bits_plain\": %.4f, \"bits_dir\": %.4f, \"subset_fails\": %llu, \"unsound_result\": %llu, "
               "\"unsound_lemma\": %llu, \"control_margin_lemma\": %llu, \"control_margin_result\": %llu, "
               "\"control_cone_lemma\": %llu, \"control_cone_result\": %llu, \"outside\": %llu, \"outside_used\": %llu, "
               "\"moved_bins\": %llu, \"surface_rays\": %llu, \"surface_in_occupied_cell\": %llu, "
               "\"surface_ended_at_start\": %llu}\n",
               kind, S.res[0], S.res[1], S.res[2], (unsigned long long)(S.tp.size() / 9), (unsigned long long)rays,
               (unsigned long long)hits, (unsigned long long)escapes, (double)bits_plain / bits, (double)bits_dir / bits,
               (unsigned long long)subset_fails, (unsigned long long)unsound_result, (unsigned long long)unsound_lemma,
               (unsigned long long)ctl[0][0], (unsigned long long)ctl[0][1], (unsigned long long)ctl[1][0],
               (unsigned long long)ctl[1][1], (unsigned long long)outside, (unsigned long long)outside_used,
               (unsigned long long)moved_bins, (unsigned long long)surf_rays, (unsigned long long)surf_in_occupied,
               (unsigned long long)surf_start_end);
        if (unsound_result || unsound_lemma || subset_fails || outside_used) rc = 1;
    }
    return rc;
}
