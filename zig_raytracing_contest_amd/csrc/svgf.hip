// svgf.hip -- zrt_context_illumination and zrt_context_svgf (include/zrt.h,
// DESIGN 5.24): albedo demodulation with luminance moments, and the
// variance-guided a-trous filter over a reprojected illumination frame.
//
// zrt_context_illumination is one kernel:
//   illumination_kernel     one thread per pixel k of the planes' own order
//                           (the call is per pixel: no pixel list), the film's
//                           rows as denoise_gather_kernel reads them.
// zrt_context_svgf is four kernels on the context's stream, iterations + 3
// launches per call:
//   svgf_gather_kernel      one thread per packed pixel k, p = pix[k]: the
//                           planes scattered into row-major 16-byte records
//                             A[p] = (illumination rgb, variance)
//                             B[p] = (normal xyz, depth)
//                             M[p] = (moments x y, length bits, 0), in the
//                                    second A array, which is free until the
//                                    first level writes it
//                           so a tap is two dwordx4 loads; iz = 1 / max(depth,
//                           2^-20) is recomputed per pixel.
//   svgf_variance_kernel    16x16 pixels per workgroup: v_0 into A[p].w.  A
//                           workgroup whose pixels all take the temporal
//                           branch -- a ballot per wave, then an LDS flag --
//                           skips the 22x22 halo and the 49 taps.  The taps
//                           read an LDS tile of luminances and B records.
//   svgf_level_kernel,      one launch per level, one thread per row-major
//   ..._tiled_kernel        pixel, 16x16 pixels per workgroup.  Colour and
//                           variance ping-pong together between the two A
//                           arrays; B is read-only.  Steps 1 and 2 stage the
//                           workgroup's halo in LDS (as denoise.hip does); the
//                           3x3 Gaussian of the variance reads the same tile
//                           (the halo is 2 step >= 2), the plain kernel loads
//                           its eight neighbours' variances.  The taps are
//                           one function.
//   svgf_present_kernel     one thread per packed k: the final record at
//                           pix[k], remodulated, into `linear`, `rgb`,
//                           `variance`, packed order.
// Every operation is written as the header states it; the unit is compiled
// with -ffp-contract=off like the rest, so nothing fuses.
#include "render_context.h"

using namespace zrt;

namespace {

// The count of pixels with a temporal variance: spread counters, as
// reproject.hip counts its pixels with history (one address would queue every
// wave's atomic at one L2 channel).  The host adds the slots up.
constexpr uint32_t kHitSlots = 64, kHitStride = 32;       // (slots; u32 words between them: 128 B)
constexpr uint32_t kHitWords = kHitSlots * kHitStride;    // 8 KB at the end of the records
constexpr uint32_t kSvTile = 16;                          // workgroup edge in pixels (kSvTile^2 = kBlock threads)
constexpr float kAlbedoMin = 0x1p-4f;

__device__ __forceinline__ float lum(float x, float y, float z) { return (0.2126f * x + 0.7152f * y) + 0.0722f * z; }
__device__ __forceinline__ float dmod(float a) { return fmaxf(a, kAlbedoMin); }

// fmaxf(1 - x2 * k, 0)^2 of a squared distance x2
__device__ __forceinline__ float sv_weight(float x2, float k) {
    const float w = fmaxf(1.0f - x2 * k, 0.0f);
    return w * w;
}

struct IlluminationParams {
    const float* color;        // P * 3, or null: the film's
    const float4* sum;         // the film's sums, packed order
    const float4* state;       // its adaptive state (w: kFilmFrozen | n), or null
    uint32_t samples;          // its samples
    const float* albedo;       // P * 3 or null
    uint32_t P;
    float* illumination;       // P * 3 or null
    float* moments;            // P * 3 or null
};

__global__ __launch_bounds__(kBlock) void illumination_kernel(const IlluminationParams g) {
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= g.P) return;
    float cx, cy, cz;
    if (g.color) {
        cx = g.color[3 * (size_t)k];
        cy = g.color[3 * (size_t)k + 1];
        cz = g.color[3 * (size_t)k + 2];
    } else {                                               // film_present_kernel's linear
        const uint32_t w = g.state ? __float_as_uint(g.state[k].w) : 0u;
        const uint32_t N = (w & kFilmFrozen) ? (w & ~kFilmFrozen) : g.samples;
        const float4 a = g.sum[k];
        const float inv = 1.0f / (float)N;
        cx = a.x * inv;
        cy = a.y * inv;
        cz = a.z * inv;
    }
    if (g.albedo) {
        cx = cx / dmod(g.albedo[3 * (size_t)k]);
        cy = cy / dmod(g.albedo[3 * (size_t)k + 1]);
        cz = cz / dmod(g.albedo[3 * (size_t)k + 2]);
    }
    if (g.illumination) {
        g.illumination[3 * (size_t)k] = cx;
        g.illumination[3 * (size_t)k + 1] = cy;
        g.illumination[3 * (size_t)k + 2] = cz;
    }
    if (g.moments) {
        const float l = lum(cx, cy, cz);
        g.moments[3 * (size_t)k] = l;
        g.moments[3 * (size_t)k + 1] = l * l;
        g.moments[3 * (size_t)k + 2] = 0.0f;
    }
}

struct GatherParams {
    const float* color;        // P * 3
    const float* moments;      // P * 3 or null
    const uint32_t* length;    // P or null
    const float* normal;       // P * 3 or null
    const float* depth;        // P or null
    const uint32_t* pix;       // packed k -> row-major p; null: p = k
    uint32_t P;
    float4* A;
    float4* B;
    float4* M;
    uint32_t* hits;            // zeroed here for the variance launch
};

__global__ __launch_bounds__(kBlock) void svgf_gather_kernel(const GatherParams g) {
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
    if (k < kHitSlots) g.hits[k * kHitStride] = 0u;          // (block 0 is whole: kBlock >= kHitSlots)
    if (k >= g.P) return;
    const uint32_t p = g.pix ? g.pix[k] : k;
    g.A[p] = make_float4(g.color[3 * (size_t)k], g.color[3 * (size_t)k + 1], g.color[3 * (size_t)k + 2], 0.0f);
    const float len = __uint_as_float(g.length ? g.length[k] : 1u);
    g.M[p] = g.moments ? make_float4(g.moments[3 * (size_t)k], g.moments[3 * (size_t)k + 1], len, 0.0f)
                       : make_float4(0.0f, 0.0f, len, 0.0f);
    if (g.normal || g.depth) {
        const float z = g.depth ? g.depth[k] : 0.0f;
        g.B[p] = g.normal ? make_float4(g.normal[3 * (size_t)k], g.normal[3 * (size_t)k + 1],
                                        g.normal[3 * (size_t)k + 2], z)
                          : make_float4(0.0f, 0.0f, 0.0f, z);
    }
}

struct LevelParams {
    const float4* in;          // A of this level
    float4* out;               // A of the next
    const float4* B;
    uint32_t w, h, step;
    uint32_t nbx;              // workgroups per row of workgroups
    float sl, kn, kz;          // sigma_luminance; 1 / sigma^2 of the guides
    float* kl;                 // ZRT_SV_PREPASS: the luminance factor per pixel, from a launch of its own
};

// The plain levels (step >= 4) take each pixel's kl from a launch before them (1) or compute it from eight
// loads of the neighbours' variances (0: 0.67 against 0.72 ms per 5-level call at 1080p)
#ifndef ZRT_SV_PREPASS
#define ZRT_SV_PREPASS 0
#endif

struct VarianceParams {
    float4* A;                 // .w written
    const float4* B;
    const float4* M;
    uint32_t w, h, nbx;
    float kn, kz;
    uint32_t* hits;
};

// wn * wz of a tap's B record against the centre's (an absent factor left out; both absent: 1)
template <bool NRM, bool DEP>
__device__ __forceinline__ float guide_weight(const float4 b, const float4 bq, float iz, float kn, float kz) {
    float wt = 1.0f;
    if (NRM) {
        const float n0 = b.x - bq.x, n1 = b.y - bq.y, n2 = b.z - bq.z;
        wt = sv_weight((n0 * n0 + n1 * n1) + n2 * n2, kn);
    }
    if (DEP) {
        const float r = (b.w - bq.w) * iz;
        const float wz = sv_weight(r * r, kz);
        wt = NRM ? wt * wz : wz;
    }
    return wt;
}

constexpr uint32_t kVarHalo = 3, kVarT = kSvTile + 2 * kVarHalo;   // the 7 x 7 taps' tile: 22 x 22

template <bool NRM, bool DEP, bool MOM>
__global__ __launch_bounds__(kBlock) void svgf_variance_kernel(const VarianceParams V) {
    __shared__ float sL[kVarT * kVarT];
    __shared__ float4 sB[(NRM || DEP) ? kVarT * kVarT : 1];
    __shared__ uint32_t sSpatial;
    const uint32_t bx = (blockIdx.x % V.nbx) * kSvTile, by = (blockIdx.x / V.nbx) * kSvTile;
    const uint32_t tx = threadIdx.x & (kSvTile - 1), ty = threadIdx.x / kSvTile;
    const uint32_t x = bx + tx, y = by + ty;
    const bool inside = x < V.w && y < V.h;
    const size_t p = (size_t)y * (size_t)V.w + (size_t)x;
    uint32_t N = 1u;
    float m1 = 0.0f, m2 = 0.0f;
    if (inside) {
        const float4 m = V.M[p];
        m1 = m.x;
        m2 = m.y;
        N = __float_as_uint(m.z);
    }
    const bool temporal = MOM && inside && N >= 4u;
    bool taps = true;                                      // does any pixel of the workgroup need the neighbourhood?
    if (MOM) {
        if (threadIdx.x == 0) sSpatial = 0u;
        __syncthreads();
        const unsigned long long need = __ballot(inside && !temporal);
        if ((threadIdx.x & 63u) == 0u && need != 0ull) atomicOr(&sSpatial, 1u);
        __syncthreads();
        taps = sSpatial != 0u;                             // (uniform over the workgroup)
    }
    if (taps) {
        for (uint32_t i = threadIdx.x; i < kVarT * kVarT; i += kBlock) {
            const uint32_t gx = bx + i % kVarT - kVarHalo, gy = by + i / kVarT - kVarHalo;   // (left of / above: wraps past w, h)
            if (gx < V.w && gy < V.h) {
                const size_t g = (size_t)gy * (size_t)V.w + (size_t)gx;
                const float4 a = V.A[g];
                sL[i] = lum(a.x, a.y, a.z);
                if (NRM || DEP) sB[i] = V.B[g];
            }
        }
        __syncthreads();
    }
    if (inside) {
        float v;
        if (temporal) {
            v = fmaxf(m2 - m1 * m1, 0.0f);
        } else {
            const int at0 = (int)((ty + kVarHalo) * kVarT + tx + kVarHalo);
            float4 b = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (NRM || DEP) b = sB[at0];
            const float iz = 1.0f / fmaxf(b.w, 0x1p-20f);
            float S1 = 0.0f, S2 = 0.0f, W = 0.0f;
            for (int dy = -3; dy <= 3; ++dy) {
#pragma unroll
                for (int dx = -3; dx <= 3; ++dx) {
                    const uint32_t qx = x + (uint32_t)dx, qy = y + (uint32_t)dy;   // (outside: wraps past w, h)
                    if (qx >= V.w || qy >= V.h) continue;
                    const int at = at0 + dy * (int)kVarT + dx;
                    float wt = 1.0f;
                    if (NRM || DEP) wt = guide_weight<NRM, DEP>(b, sB[at], iz, V.kn, V.kz);
                    const float lq = sL[at];
                    if (wt > 0.0f && fabsf(lq) < kInf) {
                        S1 = S1 + lq * wt;
                        S2 = S2 + (lq * lq) * wt;
                        W = W + wt;
                    }
                }
            }
            v = 0.0f;
            if (W > 0.0f) {
                const float e1 = S1 / W, e2 = S2 / W;
                v = fmaxf(e2 - e1 * e1, 0.0f) * (4.0f / (float)min(max(N, 1u), 4u));
            }
        }
        V.A[p].w = v;
    }
    // every lane of the wave arrives here; the count is an integer: the same in any order
    if (MOM) {
        const unsigned long long m = __ballot(temporal);
        if ((threadIdx.x & 63u) == 0u && m != 0ull)
            atomicAdd(V.hits + ((blockIdx.x * (kBlock / 64u) + (threadIdx.x >> 6)) & (kHitSlots - 1u)) * kHitStride,
                      (uint32_t)__popcll(m));
    }
}

// kl of pixel (x, y): 1 / (sigma_luminance * sqrt(the 3x3 Gaussian of the variance) + 2^-16)^2.
template <typename Fetch>
__device__ __forceinline__ float sv_kl(const LevelParams& L, uint32_t x, uint32_t y, const Fetch& f) {
    constexpr float gk[3] = {0.25f, 0.5f, 0.25f};          // kk[dy + 1][dx + 1] = gk[dy + 1] * gk[dx + 1], exact
    float Sg = 0.0f, Wg = 0.0f;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const uint32_t qx = x + (uint32_t)dx, qy = y + (uint32_t)dy;     // (outside: wraps past w, h)
            if (qx >= L.w || qy >= L.h) continue;
            const float kk = gk[dx + 1] * gk[dy + 1];
            Sg = Sg + f.V(dx, dy, qx, qy) * kk;
            Wg = Wg + kk;
        }
    }
    const float g = Sg / Wg;
    const float den = L.sl * sqrtf(g) + 0x1p-16f;
    return 1.0f / (den * den);
}

// The next level's A record of pixel (x, y) with centre records a, b and the
// pixel's kl.  `f` fetches a tap's records and a neighbour's variance: from the
// arrays (GlobalFetch) or from a workgroup's LDS tile (TileFetch); the
// arithmetic is these two functions'.
template <bool NRM, bool DEP, typename Fetch>
__device__ __forceinline__ float4 sv_pixel(const LevelParams& L, uint32_t x, uint32_t y, const float4 a, const float4 b,
                                           const float kl, const Fetch& f) {
    constexpr float hk[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    const float la = lum(a.x, a.y, a.z);
    const float iz = 1.0f / fmaxf(b.w, 0x1p-20f);
    float Sx = 0.0f, Sy = 0.0f, Sz = 0.0f, W = 0.0f, Vs = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            // (x, y < 2^31 and step <= 128: a tap left of or above the image wraps to above 2^31 >= w, h)
            const uint32_t qx = x + (uint32_t)dx * L.step, qy = y + (uint32_t)dy * L.step;
            if (qx >= L.w || qy >= L.h) continue;
            const float k = hk[dx + 2] * hk[dy + 2];
            const float4 aq = f.A(dx, dy, qx, qy);
            const float dl = la - lum(aq.x, aq.y, aq.z);
            float wt = k * sv_weight(dl * dl, kl);
            if (NRM || DEP) {
                const float4 bq = f.B(dx, dy, qx, qy);
                if (NRM) {
                    const float n0 = b.x - bq.x, n1 = b.y - bq.y, n2 = b.z - bq.z;
                    wt = wt * sv_weight((n0 * n0 + n1 * n1) + n2 * n2, L.kn);
                }
                if (DEP) {
                    const float r = (b.w - bq.w) * iz;
                    wt = wt * sv_weight(r * r, L.kz);
                }
            }
            if (wt > 0.0f) {
                Sx = Sx + aq.x * wt;
                Sy = Sy + aq.y * wt;
                Sz = Sz + aq.z * wt;
                W = W + wt;
                Vs = Vs + aq.w * (wt * wt);
            }
        }
    }
    return W > 0.0f ? make_float4(Sx / W, Sy / W, Sz / W, Vs / (W * W)) : a;
}

struct GlobalFetch {
    const LevelParams& L;
    __device__ __forceinline__ size_t at(uint32_t qx, uint32_t qy) const { return (size_t)qy * (size_t)L.w + (size_t)qx; }
    __device__ __forceinline__ float4 A(int, int, uint32_t qx, uint32_t qy) const { return L.in[at(qx, qy)]; }
    __device__ __forceinline__ float4 B(int, int, uint32_t qx, uint32_t qy) const { return L.B[at(qx, qy)]; }
    __device__ __forceinline__ float V(int, int, uint32_t qx, uint32_t qy) const { return L.in[at(qx, qy)].w; }
};

template <bool NRM, bool DEP>
__global__ __launch_bounds__(kBlock) void svgf_level_kernel(const LevelParams L) {
    const uint32_t x = (blockIdx.x % L.nbx) * kSvTile + (threadIdx.x & (kSvTile - 1));
    const uint32_t y = (blockIdx.x / L.nbx) * kSvTile + threadIdx.x / kSvTile;
    if (x >= L.w || y >= L.h) return;
    const size_t p = (size_t)y * (size_t)L.w + (size_t)x;
    const float4 a = L.in[p];
    float4 b = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (NRM || DEP) b = L.B[p];
    const GlobalFetch f{L};
    const float kl = ZRT_SV_PREPASS ? L.kl[p] : sv_kl(L, x, y, f);
    L.out[p] = sv_pixel<NRM, DEP>(L, x, y, a, b, kl, f);
}

#if ZRT_SV_PREPASS
__global__ __launch_bounds__(kBlock) void svgf_kl_kernel(const LevelParams L) {
    const uint32_t x = (blockIdx.x % L.nbx) * kSvTile + (threadIdx.x & (kSvTile - 1));
    const uint32_t y = (blockIdx.x / L.nbx) * kSvTile + threadIdx.x / kSvTile;
    if (x >= L.w || y >= L.h) return;
    L.kl[(size_t)y * (size_t)L.w + (size_t)x] = sv_kl(L, x, y, GlobalFetch{L});
}
#endif

// The levels with step 1 and 2: the workgroup first copies the
// (16 + 4 step)^2 halo of records its 16 x 16 pixels tap into LDS, and the
// taps and the variance's 3x3 neighbours read that.  Records outside the image
// are not loaded and never read: every tap is bounded by its image coordinates.
template <uint32_t STEP>
struct TileFetch {
    static constexpr uint32_t T = kSvTile + 4u * STEP;     // tile edge with its halo of 2 STEP
    const float4* sA;
    const float4* sB;
    int at0;                                               // the thread's own record in the tile
    __device__ __forceinline__ int at(int dx, int dy) const { return at0 + (dy * (int)T + dx) * (int)STEP; }
    __device__ __forceinline__ float4 A(int dx, int dy, uint32_t, uint32_t) const { return sA[at(dx, dy)]; }
    __device__ __forceinline__ float4 B(int dx, int dy, uint32_t, uint32_t) const { return sB[at(dx, dy)]; }
    __device__ __forceinline__ float V(int dx, int dy, uint32_t, uint32_t) const { return sA[at0 + dy * (int)T + dx].w; }
};

template <uint32_t STEP, bool NRM, bool DEP>
__global__ __launch_bounds__(kBlock) void svgf_level_tiled_kernel(const LevelParams L) {
    constexpr uint32_t T = TileFetch<STEP>::T, H = 2u * STEP;
    __shared__ float4 sA[T * T];
    __shared__ float4 sB[(NRM || DEP) ? T * T : 1];
    const uint32_t bx = (blockIdx.x % L.nbx) * kSvTile, by = (blockIdx.x / L.nbx) * kSvTile;
    for (uint32_t i = threadIdx.x; i < T * T; i += kBlock) {
        const uint32_t gx = bx + i % T - H, gy = by + i / T - H;     // (left of / above the image: wraps past w, h)
        if (gx < L.w && gy < L.h) {
            const size_t g = (size_t)gy * (size_t)L.w + (size_t)gx;
            sA[i] = L.in[g];
            if (NRM || DEP) sB[i] = L.B[g];
        }
    }
    __syncthreads();
    const uint32_t tx = threadIdx.x & (kSvTile - 1), ty = threadIdx.x / kSvTile;
    const uint32_t x = bx + tx, y = by + ty;
    if (x >= L.w || y >= L.h) return;
    const size_t p = (size_t)y * (size_t)L.w + (size_t)x;
    const int at0 = (int)((ty + H) * T + tx + H);
    const float4 a = sA[at0];
    float4 b = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (NRM || DEP) b = sB[at0];
    const TileFetch<STEP> f{sA, sB, at0};
    L.out[p] = sv_pixel<NRM, DEP>(L, x, y, a, b, sv_kl(L, x, y, f), f);
}

__global__ __launch_bounds__(kBlock) void svgf_present_kernel(const float4* __restrict__ A, const uint32_t* __restrict__ pix,
                                                              uint32_t P, const float* albedo, float* lin, uint8_t* rgb,
                                                              float* variance) {
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= P) return;
    float4 a = A[pix ? pix[k] : k];
    if (albedo) {
        a.x = a.x * dmod(albedo[3 * (size_t)k]);
        a.y = a.y * dmod(albedo[3 * (size_t)k + 1]);
        a.z = a.z * dmod(albedo[3 * (size_t)k + 2]);
    }
    if (lin) { lin[3 * (size_t)k] = a.x; lin[3 * (size_t)k + 1] = a.y; lin[3 * (size_t)k + 2] = a.z; }
    if (rgb) {
        uint8_t c[3];
        to_rgb(mk(a.x, a.y, a.z), c);
        rgb[3 * (size_t)k + 0] = c[0];
        rgb[3 * (size_t)k + 1] = c[1];
        rgb[3 * (size_t)k + 2] = c[2];
    }
    if (variance) variance[k] = a.w;
}

using LevelFn = void (*)(const LevelParams);
// The kernel of the level with this step for the guides present.
LevelFn level_kernel(uint32_t step, bool nrm, bool dep) {
    static const LevelFn plain[4] = {svgf_level_kernel<false, false>, svgf_level_kernel<true, false>,
                                     svgf_level_kernel<false, true>, svgf_level_kernel<true, true>};
    static const LevelFn tiled1[4] = {svgf_level_tiled_kernel<1, false, false>, svgf_level_tiled_kernel<1, true, false>,
                                      svgf_level_tiled_kernel<1, false, true>, svgf_level_tiled_kernel<1, true, true>};
    static const LevelFn tiled2[4] = {svgf_level_tiled_kernel<2, false, false>, svgf_level_tiled_kernel<2, true, false>,
                                      svgf_level_tiled_kernel<2, false, true>, svgf_level_tiled_kernel<2, true, true>};
    const int g = (nrm ? 1 : 0) | (dep ? 2 : 0);
    return step == 1u ? tiled1[g] : step == 2u ? tiled2[g] : plain[g];
}

using VarianceFn = void (*)(const VarianceParams);
template <int V> constexpr VarianceFn variance_variant() {
    return svgf_variance_kernel<(V & 1) != 0, (V & 2) != 0, (V & 4) != 0>;
}
VarianceFn variance_kernel(bool nrm, bool dep, bool mom) {
    static const VarianceFn f[8] = {variance_variant<0>(), variance_variant<1>(), variance_variant<2>(),
                                    variance_variant<3>(), variance_variant<4>(), variance_variant<5>(),
                                    variance_variant<6>(), variance_variant<7>()};
    return f[(nrm ? 1 : 0) | (dep ? 2 : 0) | (mom ? 4 : 0)];
}

int ensure_events(zrt_context* c) {
    while (c->ev_trace.size() < 2) {
        hipEvent_t e;
        HIP_TRY(hipEventCreateWithFlags(&e, hipEventDefault));
        c->ev_trace.push_back(e);
    }
    return ZRT_OK;
}

}  // namespace

extern "C" int zrt_context_illumination(zrt_context* c, const zrt_illumination_batch* b, zrt_stats* stats) {
    if (!c || !illumination_batch_ok(b)) return ZRT_ERR_INVALID_ARG;
    const uint32_t tile = b->tile_size ? b->tile_size : 64u;
    const uint32_t P = (uint32_t)((uint64_t)b->w * b->h);      // (<= 2^31: illumination_batch_ok)
    const zrt_film* f = b->film;
    // (a film of rank 0 of 1 with this w, h and tile holds zrt_tile_pixels' P pixels in the planes' order)
    if (f && (f->ctx != c || f->w != b->w || f->h != b->h || f->tile != tile || f->rank != 0u || f->nranks != 1u ||
              f->samples == 0u || f->n_owned != P))
        return ZRT_ERR_INVALID_ARG;
    const bool host = b->on_device == 0u;
    DeviceGuard g(c->device);

    int rc;
    // a host call's planes in, then out: colour 3P | albedo 3P; illumination 3P | moments 3P floats
    if (host && (rc = grow(&c->d_svio, &c->svio_cap, 12ull * P)) != ZRT_OK) return rc;
    if ((rc = ensure_events(c)) != ZRT_OK) return rc;
    // capacity guard: every buffer the launch below writes holds what it writes
    if ((host && (!c->d_svio || c->svio_cap < 12ull * P)) || (f && !f->d_sum)) return ZRT_ERR_INVALID_ARG;

    IlluminationParams G{};
    G.color = b->color;
    G.albedo = b->albedo;
    G.illumination = b->illumination;
    G.moments = b->moments;
    G.P = P;
    HIP_TRY(hipEventRecord(c->ev_begin, c->stream));
    if (host) {
        float* const s = c->d_svio;
        if (b->color) {
            HIP_TRY(copy_sync(s, b->color, 12ull * P, hipMemcpyHostToDevice, c->stream));
            G.color = s;
        }
        if (b->albedo) {
            HIP_TRY(copy_sync(s + 3ull * P, b->albedo, 12ull * P, hipMemcpyHostToDevice, c->stream));
            G.albedo = s + 3ull * P;
        }
        G.illumination = b->illumination ? s + 6ull * P : nullptr;
        G.moments = b->moments ? s + 9ull * P : nullptr;
    }
    if (f) {
        G.sum = f->d_sum;
        G.state = f->d_state && !f->state_stale ? f->d_state : nullptr;
        G.samples = f->samples;
    }
    const uint32_t blocks = (P + kBlock - 1) / kBlock;
    HIP_TRY(hipEventRecord(c->ev_trace[0], c->stream));
    hipLaunchKernelGGL(illumination_kernel, dim3(blocks), dim3(kBlock), 0, c->stream, G);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->ev_trace[1], c->stream));
    if (host) {
        if (b->illumination)
            HIP_TRY(copy_sync(b->illumination, G.illumination, 12ull * P, hipMemcpyDeviceToHost, c->stream));
        if (b->moments) HIP_TRY(copy_sync(b->moments, G.moments, 12ull * P, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(hipEventRecord(c->ev_end, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    zrt_stats st{};
    float ms = 0.0f;
    HIP_TRY(hipEventElapsedTime(&ms, c->ev_begin, c->ev_end));
    st.render_ms = ms;
    if (host) HIP_TRY(hipEventElapsedTime(&ms, c->ev_trace[0], c->ev_trace[1]));   // (without the staging copies)
    st.trace_kernel_ms = ms;
    st.samples = P;
    st.trace_launches = 1u;
    if (stats) *stats = st;
    return ZRT_OK;
}

extern "C" int zrt_context_svgf(zrt_context* c, const zrt_svgf_batch* b, zrt_stats* stats) {
    if (!c || !svgf_batch_ok(b)) return ZRT_ERR_INVALID_ARG;
    const bool row_major = (b->flags & ZRT_SVGF_ROW_MAJOR) != 0u;
    const uint32_t tile = b->tile_size ? b->tile_size : 64u;
    const uint32_t P = (uint32_t)((uint64_t)b->w * b->h);      // (<= 2^31: svgf_batch_ok)
    const bool host = b->on_device == 0u;
    const bool nrm = b->normal != nullptr, dep = b->depth != nullptr;
    const bool mom = b->moments != nullptr && b->length != nullptr;    // (no lengths: N = 1, never temporal)
    DeviceGuard g(c->device);

    int rc;
    if (!row_major) {
        zrt_camera cam{};
        zrt_render_config cfg{};
        cam.w = b->w;
        cam.h = b->h;
        cfg.tile_size = tile;
        if ((rc = rank_pixels(c, &cam, &cfg, 1)) != ZRT_OK) return rc;
        if (c->pix.size() != P) return ZRT_ERR_INVALID_ARG;
    }
    // the records: A (two, ping-pong), B, and the counters; a host call's planes in, then out:
    // colour 3P | moments 3P | length P | normal 3P | depth P | albedo 3P; linear 3P | variance P floats | rgb 3P bytes
    const size_t recs = 3ull * P + kHitWords / 4u + (ZRT_SV_PREPASS ? (size_t)P / 4u + 1u : 0u);
    if ((rc = grow(&c->d_sv, &c->sv_cap, recs)) != ZRT_OK) return rc;
    if (host && (rc = grow(&c->d_svio, &c->svio_cap, 19ull * P)) != ZRT_OK) return rc;
    if ((rc = ensure_events(c)) != ZRT_OK) return rc;
    // capacity guard: every buffer a launch below writes holds what it writes
    if (!c->d_sv || c->sv_cap < recs || (host && (!c->d_svio || c->svio_cap < 19ull * P)) ||
        (!row_major && (!c->d_pix || c->pix_cap < P)))
        return ZRT_ERR_INVALID_ARG;

    GatherParams G{};
    G.color = b->color;
    G.moments = b->moments;
    G.length = b->length;
    G.normal = b->normal;
    G.depth = b->depth;
    const float* albedo = b->albedo;
    float* lin = b->linear;
    float* var = b->variance;
    uint8_t* rgb = b->rgb;
    HIP_TRY(hipEventRecord(c->ev_begin, c->stream));
    if (host) {
        float* const s = c->d_svio;
        const struct { const void** dev; const void* src; size_t at, words; } in[6] = {
            {(const void**)&G.color, b->color, 0, 3ull * P},       {(const void**)&G.moments, b->moments, 3ull * P, 3ull * P},
            {(const void**)&G.length, b->length, 6ull * P, P},     {(const void**)&G.normal, b->normal, 7ull * P, 3ull * P},
            {(const void**)&G.depth, b->depth, 10ull * P, P},      {(const void**)&albedo, b->albedo, 11ull * P, 3ull * P}};
        for (const auto& k : in) {
            if (!k.src) continue;
            HIP_TRY(copy_sync(s + k.at, k.src, 4ull * k.words, hipMemcpyHostToDevice, c->stream));
            *k.dev = s + k.at;
        }
        lin = b->linear ? s + 14ull * P : nullptr;
        var = b->variance ? s + 17ull * P : nullptr;
        rgb = b->rgb ? reinterpret_cast<uint8_t*>(s + 18ull * P) : nullptr;
    }
    float4* const A0 = c->d_sv;
    float4* const A1 = A0 + P;
    G.pix = row_major ? nullptr : c->d_pix;
    G.P = P;
    G.A = A0;
    G.M = A1;
    G.B = A0 + 2ull * P;
    G.hits = reinterpret_cast<uint32_t*>(A0 + 3ull * P);

    const uint32_t blocks = (P + kBlock - 1) / kBlock;
    HIP_TRY(hipEventRecord(c->ev_trace[0], c->stream));
    hipLaunchKernelGGL(svgf_gather_kernel, dim3(blocks), dim3(kBlock), 0, c->stream, G);
    HIP_TRY(hipGetLastError());

    LevelParams L{};
    L.B = G.B;
    L.w = b->w;
    L.h = b->h;
    L.nbx = (b->w + kSvTile - 1) / kSvTile;
    const uint64_t nblk = (uint64_t)L.nbx * ((b->h + kSvTile - 1) / kSvTile);
    if (nblk > 0x7FFFFFFFull) return ZRT_ERR_INVALID_ARG;    // (never for P <= 2^31: at most 2^27 + 2^23 workgroups)
    L.sl = b->sigma_luminance;
    L.kn = nrm ? 1.0f / (b->sigma_normal * b->sigma_normal) : 0.0f;
    L.kz = dep ? 1.0f / (b->sigma_depth * b->sigma_depth) : 0.0f;

    VarianceParams V{};
    V.A = A0;
    V.B = G.B;
    V.M = A1;
    V.w = b->w;
    V.h = b->h;
    V.nbx = L.nbx;
    V.kn = L.kn;
    V.kz = L.kz;
    V.hits = G.hits;
    hipLaunchKernelGGL(variance_kernel(nrm, dep, mom), dim3((uint32_t)nblk), dim3(kBlock), 0, c->stream, V);
    HIP_TRY(hipGetLastError());

    for (uint32_t i = 0; i < b->iterations; ++i) {
        L.in = (i & 1u) ? A1 : A0;
        L.out = (i & 1u) ? A0 : A1;
        L.step = 1u << i;
#if ZRT_SV_PREPASS
        if (L.step > 2u) {
            L.kl = reinterpret_cast<float*>(A0 + 3ull * P + kHitWords / 4u);
            hipLaunchKernelGGL(svgf_kl_kernel, dim3((uint32_t)nblk), dim3(kBlock), 0, c->stream, L);
            HIP_TRY(hipGetLastError());
        }
#endif
        hipLaunchKernelGGL(level_kernel(L.step, nrm, dep), dim3((uint32_t)nblk), dim3(kBlock), 0, c->stream, L);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(svgf_present_kernel, dim3(blocks), dim3(kBlock), 0, c->stream,
                       (const float4*)((b->iterations & 1u) ? A1 : A0), G.pix, P, albedo, lin, rgb, var);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->ev_trace[1], c->stream));
    if (host) {
        if (b->linear) HIP_TRY(copy_sync(b->linear, lin, 12ull * P, hipMemcpyDeviceToHost, c->stream));
        if (b->rgb) HIP_TRY(copy_sync(b->rgb, rgb, 3ull * P, hipMemcpyDeviceToHost, c->stream));
        if (b->variance) HIP_TRY(copy_sync(b->variance, var, 4ull * P, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(hipEventRecord(c->ev_end, c->stream));
    uint32_t slots[kHitWords], hits = 0;
    HIP_TRY(copy_sync(slots, G.hits, sizeof slots, hipMemcpyDeviceToHost, c->stream));
    for (uint32_t i = 0; i < kHitSlots; ++i) hits += slots[i * kHitStride];
    zrt_stats st{};
    float ms = 0.0f;
    HIP_TRY(hipEventElapsedTime(&ms, c->ev_begin, c->ev_end));
    st.render_ms = ms;
    if (host) HIP_TRY(hipEventElapsedTime(&ms, c->ev_trace[0], c->ev_trace[1]));   // (without the staging copies)
    st.trace_kernel_ms = ms;
    st.samples = P;
    st.hits = hits;
    st.trace_launches = b->iterations + 3u;
    if (stats) *stats = st;
    return ZRT_OK;
}
