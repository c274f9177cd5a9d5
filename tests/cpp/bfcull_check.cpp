// Host check of the back-face cull masks (csrc/escape.h bfc_cull, the park
// kernel's first cell).  Built as a shared library by tests/test_bfcull.py.
//
// bfc_fuzz: random and adversarial triangles against directions of every
// bin -- a cleared bit must imply tri_ray's own f32 det < 1e-8 for every
// direction the device can assign to the bin (its reciprocal perturbed by up
// to 2 ulp either way).  Run with the margin or the cone's widening set to 0
// it must find violations (the check is not vacuous).
// bfc_trace_check: the sequential traceRay walk over a baked scene with and
// without the masks, camera-like rays and the bounce rays spawned at their
// hits: bit-identical (t, u, v, ref).
#include <cmath>
#include <cstdint>
#include <cstring>
#include <random>
#include <vector>

#include "dda.h"
#include "escape.h"

using namespace zrt;

namespace {

float ulps(float x, int n) {
    for (; n > 0; --n) x = nextafterf(x, kInf);
    for (; n < 0; ++n) x = nextafterf(x, -kInf);
    return x;
}

// esc_dir_bin with the reciprocal moved by p ulp (the device's v_rcp_f32 is
// within 1 ulp of the host's division; p = 0 is esc_dir_bin itself)
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

// tri_ray's determinant, its own f32 operations in its own order
float det_f32(const float e1[3], const float e2[3], v3 d) {
    return dot(mk(e1[0], e1[1], e1[2]), cross(d, mk(e2[0], e2[1], e2[2])));
}

struct Dir {
    v3 d;
    uint32_t bins[5];    // the cull bins of the five reciprocal perturbations
};

using Gen = std::mt19937_64;
double uni(Gen& g, double a, double b) { return a + (b - a) * (double)(g() >> 11) * 0x1p-53; }
double logu(Gen& g, double a, double b) { return pow(10.0, uni(g, a, b)); }

v3 from_face(uint32_t fc, double u, double v, double scale) {
    const int a = (int)(fc / 2u), b = a == 0 ? 1 : 0, c = a == 2 ? 1 : 2;
    double D[3];
    D[a] = (fc & 1u) ? -1.0 : 1.0;
    D[b] = u;
    D[c] = v;
    return mk((float)(D[0] * scale), (float)(D[1] * scale), (float)(D[2] * scale));
}

// Directions for every escape bin: the cell's corners (the exact boundaries
// and a few ulp either side), its interior, zero and tiny slopes, exact ties
// between axes; normalised, unnormalised and scaled.
std::vector<Dir> make_dirs(Gen& g, uint32_t per_bin, uint64_t* outside) {
    std::vector<Dir> out;
    const double nb = (double)kEscBins;
    const double tiny[] = {0.0, 1e-9, -1e-9, 1e-8, -1e-8, 3e-8, -3e-8, 1e-20, -1e-20, 1e-40, -1e-40, 1e-6, -1e-6};
    auto push = [&](v3 d) {
        if (!bfc_dir_ok(d)) { ++*outside; return; }
        Dir q;
        q.d = d;
        for (int p = -2; p <= 2; ++p) q.bins[p + 2] = bfc_bin_of(dir_bin_rcp(d, p));
        out.push_back(q);
    };
    for (uint32_t fc = 0; fc < 6; ++fc)
        for (uint32_t iu = 0; iu < kEscBins; ++iu)
            for (uint32_t iv = 0; iv < kEscBins; ++iv) {
                const double u0 = -1.0 + 2.0 * iu / nb, u1 = -1.0 + 2.0 * (iu + 1) / nb;
                const double v0 = -1.0 + 2.0 * iv / nb, v1 = -1.0 + 2.0 * (iv + 1) / nb;
                for (uint32_t k = 0; k < per_bin; ++k) {
                    double u, v;
                    const uint32_t kind = k % 8u;
                    if (k < 4) { u = (k & 1) ? u1 : u0; v = (k & 2) ? v1 : v0; }
                    else if (kind == 0) { u = ((g() & 1) ? u1 : u0) * (1.0 + uni(g, -4, 4) * 0x1p-23); v = uni(g, v0, v1); }
                    else if (kind == 1) { v = ((g() & 1) ? v1 : v0) * (1.0 + uni(g, -4, 4) * 0x1p-23); u = uni(g, u0, u1); }
                    else if (kind == 2) { u = tiny[g() % 13] + ((g() & 1) ? 0.0 : (g() & 1 ? u0 : u1)); v = uni(g, v0, v1); }
                    else if (kind == 3) { v = tiny[g() % 13] + ((g() & 1) ? 0.0 : (g() & 1 ? v0 : v1)); u = uni(g, u0, u1); }
                    else { u = uni(g, u0, u1); v = uni(g, v0, v1); }
                    u = fmin(fmax(u, -1.0), 1.0);
                    v = fmin(fmax(v, -1.0), 1.0);
                    double scale = 1.0;
                    const uint32_t sk = (uint32_t)(g() % 8u);
                    if (sk < 5) scale = 1.0 / sqrt(1.0 + u * u + v * v);          // unit length
                    else if (sk == 5) scale = uni(g, 0.3, 1.3);
                    else if (sk == 6) scale = logu(g, -29.5, 0.0);
                    push(from_face(fc, u, v, scale));
                }
            }
    return out;
}

struct Tri { float e1[3], e2[3]; };

void set3(float* o, double x, double y, double z) { o[0] = (float)x; o[1] = (float)y; o[2] = (float)z; }

std::vector<Tri> make_tris(Gen& g, uint32_t n, const std::vector<Dir>& dirs) {
    std::vector<Tri> out;
    auto rv = [&](double s, double* o) { for (int k = 0; k < 3; ++k) o[k] = uni(g, -1, 1) * s; };
    for (uint32_t i = 0; i < n; ++i) {
        Tri t;
        double a[3], b[3];
        const uint32_t kind = i % 10u;
        if (kind == 0) {                                   // random, any scale
            rv(logu(g, -3, 3), a); rv(logu(g, -3, 3), b);
        } else if (kind == 1) {                            // extreme edge lengths, 1e-20 .. 1e20
            rv(logu(g, -20, 20), a); rv(logu(g, -20, 20), b);
        } else if (kind == 2 || kind == 3) {               // slivers down to 1e-7 aspect
            const double L = logu(g, -2, 3), asp = logu(g, -7, -1), k2 = uni(g, -2, 2);
            rv(L, a);
            double p[3]; rv(L * asp, p);
            for (int k = 0; k < 3; ++k) b[k] = k2 * a[k] + p[k];
        } else if (kind == 4) {                            // zero area
            rv(logu(g, -3, 3), a);
            const double exact[] = {0.0, 1.0, -1.0, 2.0, -0.5};         // (exactly parallel in f32)
            const double k2 = (g() & 1) ? uni(g, -2, 2) : exact[g() % 5u];
            for (int k = 0; k < 3; ++k) b[k] = (float)(k2 * (float)a[k]);
            if (g() % 5u == 0) a[0] = a[1] = a[2] = 0.0;
        } else if (kind == 5 || kind == 6) {               // axis-aligned normal, exact or tilted a little
            const int ax = (int)(g() % 3u), bx = (ax + 1) % 3, cx = (ax + 2) % 3;
            const double L = kind == 5 ? logu(g, -2, 3) : 100.0;
            const double tilt = (g() & 1) ? 0.0 : logu(g, -13, -6) * ((g() & 1) ? 1 : -1);
            a[0] = a[1] = a[2] = b[0] = b[1] = b[2] = 0.0;
            a[bx] = L * ((g() & 1) ? 1 : -1);
            b[cx] = L * ((g() & 1) ? 1 : -1);
            ((g() & 1) ? a : b)[ax] = L * tilt;
            if (g() & 1) { a[cx] = uni(g, -1, 1) * L; }
        } else if (kind == 7) {                            // the plane nearly holds a test direction
            const v3 d = dirs[g() % dirs.size()].d;
            const double L = logu(g, -1, 3), ea = logu(g, -7, -1), eb = logu(g, -7, -1);
            double p[3], q[3]; rv(ea, p); rv(eb, q);
            const double s = 1.0 / fmax(fabs(d.x) + fabs(d.y) + fabs(d.z), 1e-30);
            a[0] = L * (d.x * s + p[0]); a[1] = L * (d.y * s + p[1]); a[2] = L * (d.z * s + p[2]);
            b[0] = L * (uni(g, -1, 1) + q[0]); b[1] = L * (uni(g, -1, 1) + q[1]); b[2] = L * (uni(g, -1, 1) + q[2]);
            if (g() & 1) for (int k = 0; k < 3; ++k) { const double x = a[k]; a[k] = b[k]; b[k] = x; }
        } else if (kind == 8) {                            // non-finite edges
            rv(1.0, a); rv(1.0, b);
            const double bad[] = {(double)kInf, -(double)kInf, (double)NAN, 3e38, -3e38, 1e30};
            ((g() & 1) ? a : b)[g() % 3u] = bad[g() % 6u];
            if (g() & 1) ((g() & 1) ? a : b)[g() % 3u] = bad[g() % 6u];
        } else {                                           // unit-scale scene triangles
            rv(1.0, a); rv(1.0, b);
        }
        set3(t.e1, a[0], a[1], a[2]);
        set3(t.e2, b[0], b[1], b[2]);
        out.push_back(t);
    }
    return out;
}

}  // namespace

// out[0] (triangle, direction, perturbation) triples whose bin is cleared,
// out[1] those with det >= 1e-8 or NaN (violations), out[2] (triangle, bin)
// bits, out[3] those cleared, out[4] directions outside bfc_dir_ok (not
// used), out[5] directions, out[6] directions whose bin moves under the
// reciprocal's perturbation, out[7] cleared bits of refs with a non-finite edge.
extern "C" void bfc_fuzz(uint64_t seed, uint32_t ntri, uint32_t per_bin, double margin, double eps, uint64_t* out) {
    Gen g(seed);
    memset(out, 0, 8 * sizeof(uint64_t));
    const std::vector<Dir> dirs = make_dirs(g, per_bin, &out[4]);
    const std::vector<Tri> tris = make_tris(g, ntri, dirs);
    out[5] = dirs.size();
    for (const Dir& q : dirs)
        for (int p = 0; p < 5; ++p)
            if (q.bins[p] != q.bins[2]) { ++out[6]; break; }
    for (const Tri& t : tris) {
        bool cull[kBfcNBin];
        bool finite = true;
        for (int k = 0; k < 3; ++k) finite = finite && std::isfinite(t.e1[k]) && std::isfinite(t.e2[k]);
        for (uint32_t b = 0; b < kBfcNBin; ++b) {
            cull[b] = bfc_cull(t.e1, t.e2, b, margin, eps);
            out[2] += 1;
            out[3] += cull[b] ? 1 : 0;
            if (cull[b] && !finite) ++out[7];
        }
        for (const Dir& q : dirs) {
            bool any = false;
            for (int p = 0; p < 5; ++p) any = any || cull[q.bins[p]];
            if (!any) continue;
            const float det = det_f32(t.e1, t.e2, q.d);
            for (int p = 0; p < 5; ++p)
                if (cull[q.bins[p]]) {
                    ++out[0];
                    if (!(det < 0.00000001f)) ++out[1];
                }
        }
    }
}

// ---- sequential traceRay over a baked scene, with and without the masks ----
namespace {

struct Scn {
    const float *bmin, *bmax, *cs;
    const uint32_t *res, *cells;
    const float* pos;   // 9 per ref: v0, e1, e2
    GridK gk;
};

bool test_tri(const Scn& S, uint32_t j, v3 o, v3 d, float* t, float* u, float* v) {
    const float* q = S.pos + 9ull * j;
    return tri_ray(mk(q[0], q[1], q[2]), mk(q[3], q[4], q[5]), mk(q[6], q[7], q[8]), o, d, t, u, v);
}

// the cull mask of (cell, bin) as bfc_build_kernel writes it
uint32_t bin_mask(const Scn& S, uint32_t lin, uint32_t bin) {
    const uint32_t b = S.cells[2 * lin], n = S.cells[2 * lin + 1] - b;
    if (n < 1u || n > 32u) return ~0u;
    uint32_t m = ~0u;
    for (uint32_t r = 0; r < n; ++r)
        if (bfc_cull(S.pos + 9ull * (b + r) + 3, S.pos + 9ull * (b + r) + 6, bin)) m &= ~(1u << r);
    return m;
}

// the entry-face mask of (cell, face) as cell32_kernel writes it
uint32_t face_mask(const Scn& S, uint32_t ci, uint32_t f) {
    const uint32_t r0 = S.res[0], r1 = S.res[1], r2 = S.res[2];
    const uint32_t x = ci % r0, y = (ci / r0) % r1, z = ci / r0 / r1;
    const uint32_t b = S.cells[2 * ci], n = S.cells[2 * ci + 1] - b;
    const uint32_t all = n >= 32u ? ~0u : (1u << n) - 1u;
    const uint32_t axis = f >> 1, neg = f & 1u;
    const uint32_t cc = axis == 0 ? x : (axis == 1 ? y : z), rr = axis == 0 ? r0 : (axis == 1 ? r1 : r2);
    const bool inside = neg ? cc + 1u < rr : cc > 0u;
    uint32_t m = all;
    if (inside && n > 0 && n <= 32) {
        const uint32_t step = axis == 0 ? 1u : (axis == 1 ? r0 : r0 * r1);
        const uint32_t pci = neg ? ci + step : ci - step;
        for (uint32_t k = 0; k < n; ++k)
            for (uint32_t q = S.cells[2 * pci]; q < S.cells[2 * pci + 1]; ++q)
                if (!memcmp(S.pos + 9ull * (b + k), S.pos + 9ull * q, 36)) { m &= ~(1u << k); break; }
    }
    return m;
}

// mode 0: every ref of every cell (stage3.zig:152-186); 1: the entry-face
// masks (the park kernel without the cull masks); 2: as 1, with the cull mask
// in the segment's first cell (the park kernel with them); 3: entry-face mask
// & cull mask in every cell.  tests: refs a mode-0 walk tries, kept: refs
// this mode tries, in the first cell and in all.
void trace(const Scn& S, int mode, v3 o, v3 d, float out[4], uint64_t cnt[4]) {
    float nearest = kInf, hu = 0, hv = 0;
    uint32_t hidx = 0;
    Dda s;
    if (dda_init(S.bmin, S.bmax, S.res, S.cs, o, d, s)) {
        const bool ok = bfc_dir_ok(d);
        const uint32_t bin = bfc_bin_of(esc_dir_bin(d));
        int face = -1;
        for (;;) {
            const uint32_t b = S.cells[2 * s.lin], e = S.cells[2 * s.lin + 1], n = e - b;
            uint32_t m = ~0u;
            if (n <= 32 && n > 0) {
                if (mode >= 1 && face >= 0) m &= face_mask(S, s.lin, (uint32_t)face);
                if (ok && ((mode == 2 && face < 0) || mode == 3)) m &= bin_mask(S, s.lin, bin);
            }
            for (uint32_t j = b; j < e; ++j) {
                cnt[face < 0 ? 0 : 1] += 1;
                if (j - b < 32 && !((m >> (j - b)) & 1u)) continue;
                cnt[face < 0 ? 2 : 3] += 1;
                float t, u, v;
                if (test_tri(S, j, o, d, &t, &u, &v) && nearest > t && t > 0.0f) {
                    nearest = t; hu = u; hv = v; hidx = j;
                }
            }
            const uint32_t c0 = s.c0, c1 = s.c1;
            bool crossed;
            float t_exit;
            DDA_STEP(s, S.gk, 2, crossed, t_exit);
            (void)crossed;
            if (nearest <= t_exit) break;
            const int axis = s.c0 != c0 ? 0 : (s.c1 != c1 ? 1 : 2);
            face = 2 * axis + (int)((s.neg >> axis) & 1u);
        }
    }
    out[0] = nearest; out[1] = hu; out[2] = hv;
    memcpy(&out[3], &hidx, 4);
}

}  // namespace

// rays: 6 floats per camera-like ray; units: 3 floats per ray and bounce, the
// unit vectors of the bounce directions normalize(n_geo + unit).  Every ray
// and the `bounces` generations of rays spawned at the hits are traced in
// modes 0..3; returns the rays whose modes disagree in any bit.
// stats[0..1]: mode-0 tests (first cell, later cells) of the bounce rays;
// stats[2 + 2 m ..]: the same kept by mode m = 1, 2, 3; stats[8]: bounce rays.
extern "C" int bfc_trace_check(const float* bmin, const float* bmax, const uint32_t* res, const float* cs,
                               const uint32_t* cells, const float* pos, uint32_t nrays, const float* rays,
                               const float* units, uint32_t bounces, uint64_t* stats) {
    Scn S{bmin, bmax, cs, res, cells, pos, GridK{res[0] - 1, res[1] - 1, res[2] - 1, res[0], res[0] * res[1]}};
    uint32_t bad = 0;
    memset(stats, 0, 9 * sizeof(uint64_t));
    for (uint32_t i = 0; i < nrays; ++i) {
        v3 o = mk(rays[6 * i], rays[6 * i + 1], rays[6 * i + 2]);
        v3 d = mk(rays[6 * i + 3], rays[6 * i + 4], rays[6 * i + 5]);
        for (uint32_t depth = 0; depth <= bounces; ++depth) {
            float a[4], b[4];
            uint64_t c0[4] = {0, 0, 0, 0};
            trace(S, 0, o, d, a, c0);
            bool same = true;
            for (int m = 1; m <= 3; ++m) {
                uint64_t c[4] = {0, 0, 0, 0};
                trace(S, m, o, d, b, c);
                same = same && !memcmp(a, b, 16);
                if (depth > 0) { stats[2 * m] += c[2]; stats[2 * m + 1] += c[3]; }
            }
            if (depth > 0) { stats[0] += c0[0]; stats[1] += c0[1]; stats[8] += 1; }
            if (!same) ++bad;
            if (!(a[0] < kInf) || depth == bounces) break;
            // the bounce ray (stage3.zig:195-219's shape: from the hit point,
            // about the geometric normal of the side the ray came from)
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
    return (int)bad;
}
