// denoise.hip -- zrt_context_denoise (include/zrt.h): the
// edge-avoiding a-trous filter over a colour frame and its feature planes.
//
// Three kernels on the context's stream, iterations + 2 launches per call:
//   denoise_gather_kernel   one thread per packed pixel k, p = pix[k]: the
//                           planes (or the film's sums) scattered into
//                           row-major 16-byte records
//                             A[p] = (colour rgb, depth)
//                             B[p] = (normal xyz, iz = 1 / max(depth, 2^-20))
//                             C[p] = (albedo rgb, 0)
//   denoise_atrous_kernel,  one launch per level, one thread per row-major
//   ..._tiled_kernel        pixel, 16x16 pixels per workgroup: a wave covers
//                           16x4, so a tap row of a wave is 256 contiguous
//                           bytes per record.  The colour ping-pongs between
//                           two A arrays (the depth rides along); B and C are
//                           read-only.  Templated on the guides present: an
//                           absent guide costs no load and no factor.  The
//                           levels with step 1 and 2 run the tiled kernel,
//                           which stages the workgroup's halo of records in
//                           LDS first (0.74 against 0.91 ms per 5-level call
//                           at 1080p); the taps are one function.
//   denoise_present_kernel  one thread per packed k: the final record at
//                           pix[k] into `linear` and / or `rgb`, packed order.
// Every operation is written as the header states it; the unit is compiled
// with -ffp-contract=off like the rest, so nothing fuses.
#include "render_context.h"

using namespace zrt;

namespace {

struct GatherParams {
    const float* color;        // P * 3, or null: the film's
    const float4* sum;         // the film's sums, packed order
    const float4* state;       // its adaptive state (w: kFilmFrozen | n), or null
    uint32_t samples;          // its samples
    const float* normal;       // P * 3 / P / P * 3, or null
    const float* depth;
    const float* albedo;
    const uint32_t* pix;       // packed k -> row-major p; null: p = k
    uint32_t P;
    float4* A;
    float4* B;
    float4* C;
};

__global__ __launch_bounds__(kBlock) void denoise_gather_kernel(const GatherParams g) {
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= g.P) return;
    const uint32_t p = g.pix ? g.pix[k] : k;
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
    const float z = g.depth ? g.depth[k] : 0.0f;
    g.A[p] = make_float4(cx, cy, cz, z);
    if (g.normal || g.depth) {
        const float iz = 1.0f / fmaxf(z, 0x1p-20f);
        g.B[p] = g.normal ? make_float4(g.normal[3 * (size_t)k], g.normal[3 * (size_t)k + 1],
                                        g.normal[3 * (size_t)k + 2], iz)
                          : make_float4(0.0f, 0.0f, 0.0f, iz);
    }
    if (g.albedo)
        g.C[p] = make_float4(g.albedo[3 * (size_t)k], g.albedo[3 * (size_t)k + 1], g.albedo[3 * (size_t)k + 2], 0.0f);
}

struct LevelParams {
    const float4* in;          // A of this level
    float4* out;               // A of the next
    const float4* B;
    const float4* C;
    uint32_t w, h, step;
    uint32_t nbx;              // workgroups per row of workgroups
    float kc, kn, kz, ka;
};

// The levels with step 1 and 2 through the LDS-tiled kernel (0: every level through the plain gather;
// the A/B of DESIGN 5.22)
#ifndef ZRT_DN_TILED
#define ZRT_DN_TILED 1
#endif
constexpr uint32_t kDnTile = 16;    // workgroup edge in pixels (kDnTile^2 = kBlock threads)

// fmaxf(1 - x2 * k, 0)^2 of a squared distance x2
__device__ __forceinline__ float dn_weight(float x2, float k) {
    const float w = fmaxf(1.0f - x2 * k, 0.0f);
    return w * w;
}

// The 25 taps of pixel (x, y) with centre records a, b, c: the next level's A
// record.  `f` fetches a tap's records: from the arrays (GlobalFetch) or from
// a workgroup's LDS tile (TileFetch); the arithmetic is this one function's.
template <bool NRM, bool DEP, bool ALB, typename Fetch>
__device__ __forceinline__ float4 dn_pixel(const LevelParams& L, uint32_t x, uint32_t y, const float4 a, const float4 b,
                                           const float4 c, const Fetch& f) {
    constexpr float hk[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    float Sx = 0.0f, Sy = 0.0f, Sz = 0.0f, W = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            // (x, y < 2^31 and step <= 128: a tap left of or above the image wraps to above 2^31 >= w, h)
            const uint32_t qx = x + (uint32_t)dx * L.step, qy = y + (uint32_t)dy * L.step;
            if (qx >= L.w || qy >= L.h) continue;
            const float k = hk[dx + 2] * hk[dy + 2];
            const float4 aq = f.A(dx, dy, qx, qy);
            const float d0 = a.x - aq.x, d1 = a.y - aq.y, d2 = a.z - aq.z;
            float wt = k * dn_weight((d0 * d0 + d1 * d1) + d2 * d2, L.kc);
            if (NRM) {
                const float4 bq = f.B(dx, dy, qx, qy);
                const float n0 = b.x - bq.x, n1 = b.y - bq.y, n2 = b.z - bq.z;
                wt = wt * dn_weight((n0 * n0 + n1 * n1) + n2 * n2, L.kn);
            }
            if (DEP) {
                const float r = (a.w - aq.w) * b.w;
                wt = wt * dn_weight(r * r, L.kz);
            }
            if (ALB) {
                const float4 cq = f.C(dx, dy, qx, qy);
                const float a0 = c.x - cq.x, a1 = c.y - cq.y, a2 = c.z - cq.z;
                wt = wt * dn_weight((a0 * a0 + a1 * a1) + a2 * a2, L.ka);
            }
            if (wt > 0.0f) {
                Sx = Sx + aq.x * wt;
                Sy = Sy + aq.y * wt;
                Sz = Sz + aq.z * wt;
                W = W + wt;
            }
        }
    }
    return W > 0.0f ? make_float4(Sx / W, Sy / W, Sz / W, a.w) : a;
}

struct GlobalFetch {
    const LevelParams& L;
    __device__ __forceinline__ size_t at(uint32_t qx, uint32_t qy) const { return (size_t)qy * (size_t)L.w + (size_t)qx; }
    __device__ __forceinline__ float4 A(int, int, uint32_t qx, uint32_t qy) const { return L.in[at(qx, qy)]; }
    __device__ __forceinline__ float4 B(int, int, uint32_t qx, uint32_t qy) const { return L.B[at(qx, qy)]; }
    __device__ __forceinline__ float4 C(int, int, uint32_t qx, uint32_t qy) const { return L.C[at(qx, qy)]; }
};

template <bool NRM, bool DEP, bool ALB>
__global__ __launch_bounds__(kBlock) void denoise_atrous_kernel(const LevelParams L) {
    const uint32_t x = (blockIdx.x % L.nbx) * kDnTile + (threadIdx.x & (kDnTile - 1));
    const uint32_t y = (blockIdx.x / L.nbx) * kDnTile + threadIdx.x / kDnTile;
    if (x >= L.w || y >= L.h) return;
    const size_t p = (size_t)y * (size_t)L.w + (size_t)x;
    const float4 a = L.in[p];
    float4 b = make_float4(0.0f, 0.0f, 0.0f, 0.0f), c = b;
    if (NRM || DEP) b = L.B[p];
    if (ALB) c = L.C[p];
    L.out[p] = dn_pixel<NRM, DEP, ALB>(L, x, y, a, b, c, GlobalFetch{L});
}

// The levels with step 1 and 2 (ZRT_DN_TILED): the workgroup first copies the
// (16 + 4 step)^2 halo of records its 16 x 16 pixels tap into LDS -- 1.6 and
// 2.3 records loaded per pixel and array instead of 25 -- and the taps read
// that.  Records outside the image are not loaded and never read: the tap loop
// bounds every tap by its image coordinates, as the plain kernel does.
template <uint32_t STEP>
struct TileFetch {
    static constexpr uint32_t T = kDnTile + 4u * STEP;     // tile edge with its halo of 2 STEP
    const float4* sA;
    const float4* sB;
    const float4* sC;
    int at0;                                               // the thread's own record in the tile
    __device__ __forceinline__ int at(int dx, int dy) const { return at0 + (dy * (int)T + dx) * (int)STEP; }
    __device__ __forceinline__ float4 A(int dx, int dy, uint32_t, uint32_t) const { return sA[at(dx, dy)]; }
    __device__ __forceinline__ float4 B(int dx, int dy, uint32_t, uint32_t) const { return sB[at(dx, dy)]; }
    __device__ __forceinline__ float4 C(int dx, int dy, uint32_t, uint32_t) const { return sC[at(dx, dy)]; }
};

template <uint32_t STEP, bool NRM, bool DEP, bool ALB>
__global__ __launch_bounds__(kBlock) void denoise_atrous_tiled_kernel(const LevelParams L) {
    constexpr uint32_t T = TileFetch<STEP>::T, H = 2u * STEP;
    __shared__ float4 sA[T * T];
    __shared__ float4 sB[NRM ? T * T : 1];
    __shared__ float4 sC[ALB ? T * T : 1];
    const uint32_t bx = (blockIdx.x % L.nbx) * kDnTile, by = (blockIdx.x / L.nbx) * kDnTile;
    for (uint32_t i = threadIdx.x; i < T * T; i += kBlock) {
        const uint32_t gx = bx + i % T - H, gy = by + i / T - H;     // (left of / above the image: wraps past w, h)
        if (gx < L.w && gy < L.h) {
            const size_t g = (size_t)gy * (size_t)L.w + (size_t)gx;
            sA[i] = L.in[g];
            if (NRM) sB[i] = L.B[g];
            if (ALB) sC[i] = L.C[g];
        }
    }
    __syncthreads();
    const uint32_t tx = threadIdx.x & (kDnTile - 1), ty = threadIdx.x / kDnTile;
    const uint32_t x = bx + tx, y = by + ty;
    if (x >= L.w || y >= L.h) return;
    const size_t p = (size_t)y * (size_t)L.w + (size_t)x;
    const int at0 = (int)((ty + H) * T + tx + H);
    const float4 a = sA[at0];
    float4 b = make_float4(0.0f, 0.0f, 0.0f, 0.0f), c = b;
    if (NRM) b = sB[at0];
    else if (DEP) b = L.B[p];
    if (ALB) c = sC[at0];
    L.out[p] = dn_pixel<NRM, DEP, ALB>(L, x, y, a, b, c, TileFetch<STEP>{sA, sB, sC, at0});
}

__global__ __launch_bounds__(kBlock) void denoise_present_kernel(const float4* __restrict__ A,
                                                                 const uint32_t* __restrict__ pix, uint32_t P,
                                                                 float* lin, uint8_t* rgb) {
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= P) return;
    const float4 a = A[pix ? pix[k] : k];
    if (lin) { lin[3 * (size_t)k] = a.x; lin[3 * (size_t)k + 1] = a.y; lin[3 * (size_t)k + 2] = a.z; }
    if (rgb) {
        uint8_t c[3];
        to_rgb(mk(a.x, a.y, a.z), c);
        rgb[3 * (size_t)k + 0] = c[0];
        rgb[3 * (size_t)k + 1] = c[1];
        rgb[3 * (size_t)k + 2] = c[2];
    }
}

using LevelFn = void (*)(const LevelParams);
template <template <bool, bool, bool> class K>
LevelFn pick_level(bool nrm, bool dep, bool alb) {
    static const LevelFn f[8] = {K<false, false, false>::fn, K<true, false, false>::fn, K<false, true, false>::fn,
                                 K<true, true, false>::fn,   K<false, false, true>::fn, K<true, false, true>::fn,
                                 K<false, true, true>::fn,   K<true, true, true>::fn};
    return f[(nrm ? 1 : 0) | (dep ? 2 : 0) | (alb ? 4 : 0)];
}
template <bool N, bool D, bool A> struct PlainLevel { static constexpr LevelFn fn = denoise_atrous_kernel<N, D, A>; };
template <bool N, bool D, bool A> struct Tiled1Level { static constexpr LevelFn fn = denoise_atrous_tiled_kernel<1, N, D, A>; };
template <bool N, bool D, bool A> struct Tiled2Level { static constexpr LevelFn fn = denoise_atrous_tiled_kernel<2, N, D, A>; };

// The kernel of the level with this step for the guides present.
LevelFn level_kernel(uint32_t step, bool nrm, bool dep, bool alb) {
#if ZRT_DN_TILED
    if (step == 1u) return pick_level<Tiled1Level>(nrm, dep, alb);
    if (step == 2u) return pick_level<Tiled2Level>(nrm, dep, alb);
#endif
    return pick_level<PlainLevel>(nrm, dep, alb);
}

}  // namespace

extern "C" int zrt_context_denoise(zrt_context* c, const zrt_denoise_batch* b, zrt_stats* stats) {
    if (!c || !denoise_batch_ok(b)) return ZRT_ERR_INVALID_ARG;
    const bool row_major = (b->flags & ZRT_DENOISE_ROW_MAJOR) != 0u;
    const uint32_t tile = b->tile_size ? b->tile_size : 64u;
    const zrt_film* f = b->film;
    if (f && (f->ctx != c || f->w != b->w || f->h != b->h || f->tile != tile || f->rank != 0u || f->nranks != 1u ||
              f->samples == 0u))
        return ZRT_ERR_INVALID_ARG;
    const uint32_t P = (uint32_t)((uint64_t)b->w * b->h);      // (<= 2^31: denoise_batch_ok)
    const bool host = b->on_device == 0u;
    const bool nrm = b->normal != nullptr, dep = b->depth != nullptr, alb = b->albedo != nullptr;
    DeviceGuard g(c->device);

    int rc;
    if (!row_major) {
        zrt_camera cam{};
        zrt_render_config cfg{};
        cam.w = b->w;
        cam.h = b->h;
        cfg.tile_size = tile;
        if ((rc = rank_pixels(c, &cam, &cfg, 1)) != ZRT_OK) return rc;
        if (c->pix.size() != P || (f && f->n_owned != P)) return ZRT_ERR_INVALID_ARG;
    }
    // the records: A (two, ping-pong), B, C; a host call's planes in, then out:
    // colour 3P | normal 3P | depth P | albedo 3P floats; linear 3P floats | rgb 3P bytes
    if ((rc = grow(&c->d_dn, &c->dn_cap, 4ull * P)) != ZRT_OK) return rc;
    if (host && (rc = grow(&c->d_dnio, &c->dnio_cap, 10ull * P)) != ZRT_OK) return rc;
    while (c->ev_trace.size() < 2) {
        hipEvent_t e;
        HIP_TRY(hipEventCreateWithFlags(&e, hipEventDefault));
        c->ev_trace.push_back(e);
    }
    // capacity guard: every buffer a launch below writes holds what it writes
    if (!c->d_dn || c->dn_cap < 4ull * P || (host && (!c->d_dnio || c->dnio_cap < 10ull * P)) ||
        (!row_major && (!c->d_pix || c->pix_cap < P)) || (f && !f->d_sum))
        return ZRT_ERR_INVALID_ARG;

    GatherParams G{};
    G.color = b->color;
    G.normal = b->normal;
    G.depth = b->depth;
    G.albedo = b->albedo;
    float* lin = b->linear;
    uint8_t* rgb = b->rgb;
    HIP_TRY(hipEventRecord(c->ev_begin, c->stream));
    if (host) {
        float* const s = c->d_dnio;
        const struct { const float** dev; const float* src; size_t at, words; } in[4] = {
            {&G.color, b->color, 0, 3ull * P},      {&G.normal, b->normal, 3ull * P, 3ull * P},
            {&G.depth, b->depth, 6ull * P, P},      {&G.albedo, b->albedo, 7ull * P, 3ull * P}};
        for (const auto& k : in) {
            if (!k.src) continue;
            HIP_TRY(copy_sync(s + k.at, k.src, 4ull * k.words, hipMemcpyHostToDevice, c->stream));
            *k.dev = s + k.at;
        }
        lin = b->linear ? s : nullptr;
        rgb = b->rgb ? reinterpret_cast<uint8_t*>(s + 3ull * P) : nullptr;
    }
    if (f) {
        G.sum = f->d_sum;
        G.state = f->d_state && !f->state_stale ? f->d_state : nullptr;
        G.samples = f->samples;
    }
    float4* const A0 = c->d_dn;
    float4* const A1 = A0 + P;
    G.pix = row_major ? nullptr : c->d_pix;
    G.P = P;
    G.A = A0;
    G.B = A0 + 2ull * P;
    G.C = A0 + 3ull * P;

    const uint32_t blocks = (P + kBlock - 1) / kBlock;
    HIP_TRY(hipEventRecord(c->ev_trace[0], c->stream));
    hipLaunchKernelGGL(denoise_gather_kernel, dim3(blocks), dim3(kBlock), 0, c->stream, G);
    HIP_TRY(hipGetLastError());

    LevelParams L{};
    L.B = G.B;
    L.C = G.C;
    L.w = b->w;
    L.h = b->h;
    L.nbx = (b->w + kDnTile - 1) / kDnTile;
    const uint64_t nblk = (uint64_t)L.nbx * ((b->h + kDnTile - 1) / kDnTile);
    if (nblk > 0x7FFFFFFFull) return ZRT_ERR_INVALID_ARG;    // (never for P <= 2^31: at most 2^27 + 2^23 workgroups)
    L.kn = nrm ? 1.0f / (b->sigma_normal * b->sigma_normal) : 0.0f;
    L.kz = dep ? 1.0f / (b->sigma_depth * b->sigma_depth) : 0.0f;
    L.ka = alb ? 1.0f / (b->sigma_albedo * b->sigma_albedo) : 0.0f;
    float s_i = b->sigma_color;
    for (uint32_t i = 0; i < b->iterations; ++i) {
        L.in = (i & 1u) ? A1 : A0;
        L.out = (i & 1u) ? A0 : A1;
        L.step = 1u << i;
        L.kc = 1.0f / (s_i * s_i);
        hipLaunchKernelGGL(level_kernel(L.step, nrm, dep, alb), dim3((uint32_t)nblk), dim3(kBlock), 0, c->stream, L);
        HIP_TRY(hipGetLastError());
        s_i = s_i * 0.5f;                                  // sigma_color * 2^-i, exact
    }
    hipLaunchKernelGGL(denoise_present_kernel, dim3(blocks), dim3(kBlock), 0, c->stream,
                       (const float4*)((b->iterations & 1u) ? A1 : A0), G.pix, P, lin, rgb);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->ev_trace[1], c->stream));
    if (host) {
        if (b->linear) HIP_TRY(copy_sync(b->linear, lin, 12ull * P, hipMemcpyDeviceToHost, c->stream));
        if (b->rgb) HIP_TRY(copy_sync(b->rgb, rgb, 3ull * P, hipMemcpyDeviceToHost, c->stream));
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
    st.trace_launches = b->iterations + 2u;
    if (stats) *stats = st;
    return ZRT_OK;
}
