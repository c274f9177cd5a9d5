// sky.hip -- sky-light queries on CDNA4 (gfx950), DESIGN 5.26: the two item
// kernels of zrt_context_sky_light (sky_gen_kernel, sky_reduce_kernel).  The
// call's plan, first hits and chains are render.hip's (light_items);
// emitters.h holds what the two share.
#include "emitters.h"

using namespace zrt;

namespace {

constexpr uint32_t kSkyGenItems = 4;           // items per thread of sky_gen_kernel
constexpr float kPi = 0x1.921fb6p+1f;          // pi rounded to f32, 0x40490FDB

// A block takes kSkyGenItems * kBlock consecutive items, a wave 64 consecutive
// ones at a time.  The normal and the position are surface_kernel's
// (surface_gather's texel loads fall away), the draws and the direction
// occlusion_gen_kernel's about the normalised normal.  Almost every item of a
// ray that hit is traced, so the list is about as long as the item range; the
// append is one returning atomic per wave all the same, and the order inside
// the list is free: sky_reduce_kernel finds an item's entry through its slot.
__global__ __launch_bounds__(kBlock) void sky_gen_kernel(const SkyParams r) {
    __shared__ double s_zig[514];
    for (uint32_t i = threadIdx.x; i < 514; i += blockDim.x) s_zig[i] = r.zig[i];
    __syncthreads();
    const double* zx = s_zig;
    const double* zf = s_zig + 257;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t below = (1ull << lane) - 1ull;
    const bool aligned = (reinterpret_cast<uintptr_t>(r.hits) & 15u) == 0u;   // (uniform: the context's own records always are)
    for (uint32_t k = 0; k < kSkyGenItems; ++k) {
        const uint32_t j = (blockIdx.x * kSkyGenItems + k) * kBlock + threadIdx.x;
        if (__ballot(j < r.m) == 0ull) break;                                   // (wave-uniform)
        bool live = false;
        v3 o = mk(0, 0, 0), d = mk(0, 0, 0);
        if (j < r.m) {
            const uint32_t I = j + r.s0, qr = I / r.S;
            const uint32_t ray = r.ray0 + qr, s = I - qr * r.S;
            uint4 h = make_uint4(0x7F800000u, 0u, 0u, 0xFFFFFFFFu);
            if (ray < r.n) h = hit_load(r.hits, aligned, ray);                  // (always: m items of n rays)
            const float t = __uint_as_float(h.x);
            if (t != kInf) {                                                    // a hit (query_store)
                v3 ro, rd;
                ray_load(r.rays, ray, ro, rd);
                const SurfaceInputs g = surface_gather(r.tri_data, r.mats, r.texels, __uint_as_float(h.y),
                                                       __uint_as_float(h.z), h.w);
                o = add(ro, scale(rd, t + kFltEps));
                const v3 N = normalize_rn(g.nrm);
                if (finite3(o) && finite3(N)) {                                 // shaded
                    Rng rng;
                    rng.s = path_key(r.seed, r.key0 + ray, s);
                    const float nx = (float)rng_norm64(rng, zx, zf);
                    const float ny = (float)rng_norm64(rng, zx, zf);
                    const float nz = (float)rng_norm64(rng, zx, zf);
                    d = normalize_rn(add(N, normalize_rn(mk(nx, ny, nz))));
                    live = finite3(d) && (d.x != 0.0f || d.y != 0.0f || d.z != 0.0f);
                }
            }
        }
        const uint64_t ml = __ballot(live);
        uint32_t pos = 0xFFFFFFFFu;
        if (ml != 0ull) {
            const uint32_t lead = (uint32_t)__builtin_ctzll(ml);
            uint32_t ob = 0;
            if (lane == lead) ob = atomicAdd(&r.ctr[4], (uint32_t)__popcll(ml));
            ob = (uint32_t)__builtin_amdgcn_readlane((int)ob, (int)lead);
            if (live) pos = ob + (uint32_t)__popcll(ml & below);
            if (pos >= r.m) pos = 0xFFFFFFFFu;                                  // (never: at most m live items)
            if (pos != 0xFFFFFFFFu) {
                float* q = r.irays + 6ull * pos;
                q[3] = d.x; q[4] = d.y; q[5] = d.z;
                if (r.unshadowed == 0u) {
                    q[0] = o.x; q[1] = o.y; q[2] = o.z;
                    r.ibound[pos] = kInf;
                }
            }
        }
        if (j < r.m) r.slot[j] = pos;
    }
}

// One thread per ray of the sub-chunk, ray0 + i: its items [a, e) of the
// sub-chunk in sample order.  A and V start at +0 with the ray's sample 0 and
// are read back from their rows otherwise; an item that is not traced adds
// nothing.  The sky's colour is env_color of the entry's direction, of which
// only y enters.  With the ray's last sample the sums are divided by S, the
// irradiance is pi * mean and, `radiance` asked, the surface is gathered once
// more for its base colour and emission.  Thread 0 moves the walk launches'
// segment and crossing counts to the call's own two, as area_reduce_kernel
// does.
__global__ __launch_bounds__(kBlock) void sky_reduce_kernel(const SkyParams r) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i == 0u && r.fold != 0u) {
        r.stats[kAreaStat] += r.stats[0];
        r.stats[kAreaStat + 1] += r.stats[3];
        r.stats[0] = 0ull;
        r.stats[3] = 0ull;
    }
    const uint32_t end = r.s0 + r.m;                                            // (< 2^21: s0 < S < 2^16)
    const uint32_t ray = r.ray0 + i;
    if ((uint64_t)i * r.S >= end || ray >= r.n) return;                         // (ray < n: always)
    const uint32_t first = i * r.S;
    const uint32_t a = max(first, r.s0), e = min(first + r.S, end);
    const bool aligned = (reinterpret_cast<uintptr_t>(r.hits) & 15u) == 0u;
    const uint4 h = hit_load(r.hits, aligned, ray);
    const float t = __uint_as_float(h.x);
    float* const Ep = r.E + 3ull * ray;
    const bool last = e == first + r.S;
    v3 A = mk(0.0f, 0.0f, 0.0f);
    float V = 0.0f;
    if (t != kInf) {
        if (a != first) {
            A = ld3(Ep);
            V = r.V[ray];
        }
        for (uint32_t x = a; x < e; ++x) {
            const uint32_t s = r.slot[x - r.s0];
            if (s == 0xFFFFFFFFu) continue;
            const float T = r.unshadowed != 0u ? 1.0f : r.T[s];
            const v3 L = env_color(mk(0.0f, r.irays[6ull * s + 4], 0.0f));
            A = add(A, scale(L, T));
            V = V + T;
        }
    }
    if (!last) {
        Ep[0] = A.x; Ep[1] = A.y; Ep[2] = A.z;
        r.V[ray] = V;
        return;
    }
    const float fs = (float)r.S;
    const v3 mean = mk(A.x / fs, A.y / fs, A.z / fs);
    Ep[0] = mean.x * kPi; Ep[1] = mean.y * kPi; Ep[2] = mean.z * kPi;
    r.V[ray] = V / fs;
    if (!r.radiance) return;
    v3 out = mk(0.0f, 0.0f, 0.0f);
    if (t != kInf) {
        v3 ro, rd;
        ray_load(r.rays, ray, ro, rd);
        const SurfaceInputs g = surface_gather(r.tri_data, r.mats, r.texels, __uint_as_float(h.y), __uint_as_float(h.z),
                                               h.w);
        const bool shaded = finite3(add(ro, scale(rd, t + kFltEps))) && finite3(normalize_rn(g.nrm));
        out = shaded ? add(g.emissive, mul(g.albedo, mean)) : g.emissive;
    }
    float* const Rp = r.radiance + 3ull * ray;
    Rp[0] = out.x; Rp[1] = out.y; Rp[2] = out.z;
}

}  // namespace

int sky_gen_launch(const SkyParams& p, hipStream_t stream) {
    const uint32_t mblk = (p.m + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(sky_gen_kernel, dim3((mblk + kSkyGenItems - 1) / kSkyGenItems), dim3(kBlock), 0, stream, p);
    HIP_TRY(hipGetLastError());
    return ZRT_OK;
}

int sky_reduce_launch(const SkyParams& p, uint32_t rays, hipStream_t stream) {
    hipLaunchKernelGGL(sky_reduce_kernel, dim3((rays + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, p);
    HIP_TRY(hipGetLastError());
    return ZRT_OK;
}
