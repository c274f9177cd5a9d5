// emitters.hip -- area-light queries on CDNA4 (gfx950), DESIGN 5.25: the
// emitter set (zrt_emitters_*: the scene's emissive source triangles as an
// integer distribution, built on the device from the context's own material
// table and texel pool) and the two item kernels of zrt_context_area_lights
// (area_gen_kernel, area_reduce_kernel).  The call's plan, first hits and
// chains are render.hip's; emitters.h holds what the two share.
#include <new>

#include "emitters.h"

using namespace zrt;

namespace {

constexpr uint32_t kScanTile = kBlock;         // elements per block of a scan level: one per thread
constexpr uint32_t kMaxEmitters = 1u << 28;    // Q < 2^52: (float)Q has one rounding

// ---------------------------------------------------------------------------
// The set build.

// m of every material: the fmaxf fold from +0 over every component of every
// texel of its emissive texture.  One workgroup per material, strided over the
// texture's floats; a maximum is order-free, so the tree's shape is free.  A
// 1x1 texture's texel rides in its descriptor (dev_tex_inline).
__global__ __launch_bounds__(kBlock) void emit_matmax_kernel(const DevMat* mats, const float* texels, float* mmax) {
    __shared__ float s_m[kBlock / 64];
    const DevTex t = mats[blockIdx.x].tex[1];
    float m = 0.0f;
    if (t.w == 1 && t.h == 1) {
        if (threadIdx.x == 0)
            m = fmaxf(fmaxf(fmaxf(m, __int_as_float(t.umin)), __int_as_float(t.umax)), __int_as_float(t.vmin));
    } else {
        const float* b = texels + t.off;
        const uint64_t nf = 3ull * (uint64_t)(uint32_t)t.w * (uint64_t)(uint32_t)t.h;
        for (uint64_t i = threadIdx.x; i < nf; i += kBlock) m = fmaxf(m, b[i]);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
    if ((threadIdx.x & 63u) == 0u) s_m[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (uint32_t k = 1; k < kBlock / 64; ++k) m = fmaxf(m, s_m[k]);
        mmax[blockIdx.x] = m;
    }
}

struct EmitBuild {
    const float* pos;         // n * 9
    const float* uv;          // n * 6, or null: zeros
    const uint32_t* mat;      // n
    const float* mmax;        // per material
    uint32_t nmat;
    uint32_t n;
    float* w;                 // n: a * m
    uint32_t* flag;           // n: 1 an emitter, else 0; then, scanned in place, its rank
    uint32_t* wmax;           // the bits of the largest emitter weight (positive floats order as their bits)
    uint32_t count;           // emit_record_kernel: emitters
    float4* rec;              // count * 5
    unsigned long long* q64;  // count: q, then, scanned in place, C
};

__device__ __forceinline__ void emit_edges(const float* pos, uint32_t i, v3& v0, v3& e1, v3& e2) {
    const float* p = pos + 9ull * i;
    v0 = mk(p[0], p[1], p[2]);
    e1 = sub(mk(p[3], p[4], p[5]), v0);
    e2 = sub(mk(p[6], p[7], p[8]), v0);
}

// One thread per source triangle: w = (0.5f * length(cross(e1, e2))) * m.
__global__ __launch_bounds__(kBlock) void emit_weight_kernel(const EmitBuild r) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    bool em = false;
    float w = 0.0f;
    if (i < r.n) {
        v3 v0, e1, e2;
        emit_edges(r.pos, i, v0, e1, e2);
        const float a = 0.5f * length(cross(e1, e2));
        const uint32_t mi = r.mat[i];
        w = a * (mi < r.nmat ? r.mmax[mi] : 0.0f);                  // (always in range: the host checked)
        em = w > 0.0f && w < kInf;                                  // (false for a NaN)
        r.w[i] = w;
        r.flag[i] = em ? 1u : 0u;
    }
    uint32_t wb = em ? __float_as_uint(w) : 0u;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) wb = max(wb, (uint32_t)__shfl_xor((int)wb, off));
    if ((threadIdx.x & 63u) == 0u && wb != 0u) atomicMax(r.wmax, wb);
}

// One level of an exclusive scan: block b scans elements [b * kScanTile,
// (b + 1) * kScanTile) in place and leaves its total in sums[b] (null: one
// block).  Integer sums: any tree gives the serial sum's bits.
__device__ __forceinline__ uint32_t shfl_up_t(uint32_t x, int off) { return (uint32_t)__shfl_up((int)x, off); }
__device__ __forceinline__ unsigned long long shfl_up_t(unsigned long long x, int off) {
    const unsigned lo = (unsigned)__shfl_up((int)(unsigned)x, off);
    const unsigned hi = (unsigned)__shfl_up((int)(unsigned)(x >> 32), off);
    return ((unsigned long long)hi << 32) | lo;
}
template <typename T>
__global__ __launch_bounds__(kBlock) void scan_block_kernel(T* data, T* sums, uint32_t n) {
    __shared__ T s_w[kBlock / 64];
    const uint32_t i = blockIdx.x * kScanTile + threadIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const T v = i < n ? data[i] : (T)0;
    T x = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const T y = shfl_up_t(x, off);
        if ((int)lane >= off) x += y;
    }
    if (lane == 63u) s_w[wave] = x;
    __syncthreads();
    T base = 0;
    for (uint32_t k = 0; k < wave; ++k) base += s_w[k];
    if (i < n) data[i] = base + x - v;
    if (sums && threadIdx.x == kBlock - 1) sums[blockIdx.x] = base + x;
}
template <typename T>
__global__ __launch_bounds__(kBlock) void scan_add_kernel(T* data, const T* offs, uint32_t n) {
    const uint32_t i = blockIdx.x * kScanTile + threadIdx.x;
    if (i < n) data[i] += offs[blockIdx.x];
}
// words of T a scan of n elements needs beside them: one per block of every level
uint64_t scan_scratch(uint64_t n) {
    uint64_t w = 0;
    while (n > kScanTile) {
        n = (n + kScanTile - 1) / kScanTile;
        w += n;
    }
    return w + 1;
}
// data[0..n) -> its exclusive prefix sums, in place; levels until one block is left
template <typename T>
int scan_exclusive(T* data, uint32_t n, T* scratch, hipStream_t sm) {
    if (n == 0) return ZRT_OK;
    const uint32_t nb = (n + kScanTile - 1) / kScanTile;
    hipLaunchKernelGGL(scan_block_kernel<T>, dim3(nb), dim3(kBlock), 0, sm, data, nb > 1 ? scratch : (T*)nullptr, n);
    HIP_TRY(hipGetLastError());
    if (nb == 1) return ZRT_OK;
    const int rc = scan_exclusive(scratch, nb, scratch + nb, sm);
    if (rc != ZRT_OK) return rc;
    hipLaunchKernelGGL(scan_add_kernel<T>, dim3(nb), dim3(kBlock), 0, sm, data, (const T*)scratch, n);
    HIP_TRY(hipGetLastError());
    return ZRT_OK;
}

// One thread per source triangle, after the scan of the flags: emitter k =
// flag[i] of an emitting triangle i gets its record and its q.
__global__ __launch_bounds__(kBlock) void emit_record_kernel(const EmitBuild r) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= r.n) return;
    const float w = r.w[i];
    if (!(w > 0.0f && w < kInf)) return;
    const uint32_t k = r.flag[i];
    if (k >= r.count) return;                                       // (never: the scan's own ranks)
    v3 v0, e1, e2;
    emit_edges(r.pos, i, v0, e1, e2);
    const float a = 0.5f * length(cross(e1, e2));
    const float wmax = __uint_as_float(*r.wmax);
    const uint32_t q = max(1u, (uint32_t)((w / wmax) * 0x1p24f));
    float tc[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (r.uv)
        for (int j = 0; j < 6; ++j) tc[j] = r.uv[6ull * i + j];
    float4* const o = r.rec + 5ull * k;
    o[0] = make_float4(v0.x, v0.y, v0.z, a);
    o[1] = make_float4(e1.x, e1.y, e1.z, __uint_as_float(q));
    o[2] = make_float4(e2.x, e2.y, e2.z, __uint_as_float(r.mat[i]));
    o[3] = make_float4(tc[0], tc[1], tc[2], tc[3]);
    o[4] = make_float4(tc[4], tc[5], __uint_as_float(i), __uint_as_float(0u));
    r.q64[k] = q;
}

// ---------------------------------------------------------------------------
// The call's item kernels.
constexpr uint32_t kAreaGenItems = 4;          // items per thread of area_gen_kernel
constexpr float kAreaBound = 0x1.ff8p-1f;      // 1 - 2^-10: the chain ends short of the emitter itself

// A block takes kAreaGenItems * kBlock consecutive items, a wave 64 consecutive
// ones at a time.  The normal and the position are surface_kernel's.  The
// search runs `steps` rounds in every lane (branch-uniform); C and the records
// are read-only and shared by all lanes.  The three draws are whole words of
// the render's stream; the 64 x 64 -> high 64 product is one per item.
__global__ __launch_bounds__(kBlock) void area_gen_kernel(const AreaParams r) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t below = (1ull << lane) - 1ull;
    const bool aligned = (reinterpret_cast<uintptr_t>(r.hits) & 15u) == 0u;   // (uniform: the context's own records always are)
    for (uint32_t k = 0; k < kAreaGenItems; ++k) {
        const uint32_t j = (blockIdx.x * kAreaGenItems + k) * kBlock + threadIdx.x;
        if (__ballot(j < r.m) == 0ull) break;                                   // (wave-uniform)
        bool live = false;
        v3 o = mk(0, 0, 0), w = mk(0, 0, 0), con = mk(0, 0, 0);
        float bound = 0.0f;
        if (j < r.m && r.count != 0u) {
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
                    Rng rng{path_key(r.seed, r.key0 + ray, s)};
                    const uint64_t x0 = rng.next(), x1 = rng.next(), x2 = rng.next();
                    const uint64_t rsel = __umul64hi(x0, r.Q);
                    uint32_t e = 0;                                             // the last emitter with C <= rsel
                    for (uint32_t st = r.steps; st-- != 0u;) {
                        const uint32_t c = e + (1u << st);
                        if (c < r.count && r.C[c] <= rsel) e = c;
                    }
                    const float4* rp = r.rec + 5ull * e;
                    const float4 r0 = rp[0], r1 = rp[1], r2 = rp[2], r3 = rp[3], r4 = rp[4];
                    const v3 v0 = mk(r0.x, r0.y, r0.z), e1 = mk(r1.x, r1.y, r1.z), e2 = mk(r2.x, r2.y, r2.z);
                    float bu = (float)(uint32_t)(x1 >> 40) * 0x1p-24f, bv = (float)(uint32_t)(x2 >> 40) * 0x1p-24f;
                    if (bu + bv > 1.0f) {
                        bu = 1.0f - bu;
                        bv = 1.0f - bv;
                    }
                    const v3 y = add(add(v0, scale(e1, bu)), scale(e2, bv));
                    const float w0 = 1.0f - bu - bv;
                    const float tc0 = (r3.x * w0 + r3.z * bu) + r4.x * bv;
                    const float tc1 = (r3.y * w0 + r3.w * bu) + r4.y * bv;
                    const DevMat& m = r.mats[__float_as_uint(r2.w)];
                    const v3 Le = sample3(r.texels, m.tex[1], tc0, tc1);
                    const float alpha = sample1(r.texels, m.tex[2], tc0, tc1);
                    const v3 v = sub(y, o);
                    const float d2 = dot(v, v);
                    w = normalize_rn(v);
                    const float c = dot(N, w);
                    const float cl = -dot(normalize_rn(cross(e1, e2)), w);
                    live = c > 0.0f && cl > 0.0f;                               // (false for a NaN)
                    const float gg = ((c * cl) / d2) * ((r.Qf / (float)__float_as_uint(r1.w)) * r0.w);
                    con = scale(scale(Le, alpha), gg);
                    bound = length(v) * kAreaBound;
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
            if (pos != 0xFFFFFFFFu && r.unshadowed == 0u) {
                float* q = r.irays + 6ull * pos;
                q[0] = o.x; q[1] = o.y; q[2] = o.z;
                q[3] = w.x; q[4] = w.y; q[5] = w.z;
                r.ibound[pos] = bound;
            }
        }
        if (j < r.m) {
            r.contrib[j] = pos != 0xFFFFFFFFu ? make_float4(con.x, con.y, con.z, 0.0f) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            r.slot[j] = pos;
        }
    }
}

// One thread per ray of the sub-chunk, ray0 + i: its items [a, e) of the
// sub-chunk in sample order.  E starts at +0 with the ray's sample 0 and is
// read back from the row otherwise; an item that is not traced adds nothing.
// With the ray's last sample E is divided by S and, `radiance` asked, the
// surface is gathered once more for its base colour and emission.  Thread 0
// moves the walk launches' segment and crossing counts (stats[0], stats[3],
// which the first hits' kernels also add to and the host cleared after them)
// to the call's own two.
__global__ __launch_bounds__(kBlock) void area_reduce_kernel(const AreaParams r) {
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
    v3 E = mk(0.0f, 0.0f, 0.0f);
    if (t != kInf) {
        if (a != first) E = ld3(Ep);
        for (uint32_t x = a; x < e; ++x) {
            const uint32_t j = x - r.s0, s = r.slot[j];
            if (s == 0xFFFFFFFFu) continue;
            const float T = r.unshadowed != 0u ? 1.0f : r.T[s];
            const float4 cn = r.contrib[j];
            E = add(E, scale(mk(cn.x, cn.y, cn.z), T));
        }
        if (last) {
            const float fs = (float)r.S;
            E = mk(E.x / fs, E.y / fs, E.z / fs);
        }
    }
    Ep[0] = E.x; Ep[1] = E.y; Ep[2] = E.z;
    if (!last || !r.radiance) return;
    v3 out = mk(0.0f, 0.0f, 0.0f);
    if (t != kInf) {
        v3 ro, rd;
        ray_load(r.rays, ray, ro, rd);
        const SurfaceInputs g = surface_gather(r.tri_data, r.mats, r.texels, __uint_as_float(h.y), __uint_as_float(h.z),
                                               h.w);
        const bool shaded = finite3(add(ro, scale(rd, t + kFltEps))) && finite3(normalize_rn(g.nrm));
        out = shaded ? add(g.emissive, scale(mul(g.albedo, E), kInvPi)) : g.emissive;
    }
    float* const Rp = r.radiance + 3ull * ray;
    Rp[0] = out.x; Rp[1] = out.y; Rp[2] = out.z;
}

// frees the build's temporaries on every way out
struct DevFree {
    std::vector<void*> p;
    ~DevFree() {
        for (void* q : p)
            if (q) (void)hipFree(q);
    }
    template <typename T>
    int alloc(T** out, uint64_t n) {
        HIP_TRY(hipMalloc((void**)out, std::max<uint64_t>(n, 1) * sizeof(T)));
        p.push_back(*out);
        return ZRT_OK;
    }
};

}  // namespace

int area_gen_launch(const AreaParams& p, hipStream_t stream) {
    const uint32_t mblk = (p.m + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(area_gen_kernel, dim3((mblk + kAreaGenItems - 1) / kAreaGenItems), dim3(kBlock), 0, stream, p);
    HIP_TRY(hipGetLastError());
    return ZRT_OK;
}

int area_reduce_launch(const AreaParams& p, uint32_t rays, hipStream_t stream) {
    hipLaunchKernelGGL(area_reduce_kernel, dim3((rays + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, p);
    HIP_TRY(hipGetLastError());
    return ZRT_OK;
}

extern "C" int zrt_emitters_create(zrt_context* c, const float* positions, const float* texcoords,
                                   const uint32_t* material, uint32_t n, zrt_emitters** out) {
    if (!c || !out || (n != 0u && (!positions || !material))) return ZRT_ERR_INVALID_ARG;
    for (uint32_t i = 0; i < n; ++i)
        if (material[i] >= c->nmat) return ZRT_ERR_INVALID_ARG;
    *out = nullptr;
    zrt_emitters* es = new (std::nothrow) zrt_emitters();
    if (!es) return ZRT_ERR_OUT_OF_MEMORY;
    es->ctx = c;
    es->device = c->device;
    es->num_triangles = n;
    if (n == 0u) { *out = es; return ZRT_OK; }
    DeviceGuard g(c->device);
    struct Undo {
        zrt_emitters* es;
        ~Undo() { if (es) zrt_emitters_destroy(es); }
    } undo{es};
    DevFree tmp;
    EmitBuild B{};
    float *d_pos = nullptr, *d_uv = nullptr, *d_mmax = nullptr;
    uint32_t *d_mat = nullptr, *d_scr32 = nullptr;
    int rc;
    if ((rc = tmp.alloc(&d_pos, 9ull * n)) != ZRT_OK || (rc = tmp.alloc(&d_mat, n)) != ZRT_OK ||
        (rc = tmp.alloc(&d_mmax, c->nmat)) != ZRT_OK || (rc = tmp.alloc(&B.w, n)) != ZRT_OK ||
        (rc = tmp.alloc(&B.flag, n)) != ZRT_OK || (rc = tmp.alloc(&B.wmax, 1)) != ZRT_OK ||
        (rc = tmp.alloc(&d_scr32, scan_scratch(n))) != ZRT_OK)
        return rc;
    if (texcoords && (rc = tmp.alloc(&d_uv, 6ull * n)) != ZRT_OK) return rc;
    hipStream_t sm = c->stream;
    HIP_TRY(hipMemcpyAsync(d_pos, positions, 36ull * n, hipMemcpyHostToDevice, sm));
    HIP_TRY(hipMemcpyAsync(d_mat, material, 4ull * n, hipMemcpyHostToDevice, sm));
    if (texcoords) HIP_TRY(hipMemcpyAsync(d_uv, texcoords, 24ull * n, hipMemcpyHostToDevice, sm));
    HIP_TRY(hipMemsetAsync(B.wmax, 0, 4, sm));
    B.pos = d_pos;
    B.uv = d_uv;
    B.mat = d_mat;
    B.mmax = d_mmax;
    B.nmat = c->nmat;
    B.n = n;
    const uint32_t nblk = (n + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(emit_matmax_kernel, dim3(c->nmat), dim3(kBlock), 0, sm, c->d_mats, c->d_texels, d_mmax);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(emit_weight_kernel, dim3(nblk), dim3(kBlock), 0, sm, B);
    HIP_TRY(hipGetLastError());
    // the last triangle's flag, before the scan overwrites it with its rank
    uint32_t last_flag = 0, last_rank = 0;
    HIP_TRY(copy_sync(&last_flag, B.flag + (n - 1), 4, hipMemcpyDeviceToHost, sm));
    if ((rc = scan_exclusive(B.flag, n, d_scr32, sm)) != ZRT_OK) return rc;
    HIP_TRY(copy_sync(&last_rank, B.flag + (n - 1), 4, hipMemcpyDeviceToHost, sm));
    const uint32_t count = last_rank + last_flag;
    if (count > n) return ZRT_ERR_HIP;                              // (never)
    if (count > kMaxEmitters) return ZRT_ERR_UNSUPPORTED;
    es->count = count;
    if (count != 0u) {
        unsigned long long* d_scr64 = nullptr;
        if ((rc = tmp.alloc(&d_scr64, scan_scratch(count))) != ZRT_OK) return rc;
        HIP_TRY(hipMalloc((void**)&es->d_rec, 80ull * count));
        HIP_TRY(hipMalloc((void**)&es->d_C, 8ull * count));
        B.count = count;
        B.rec = reinterpret_cast<float4*>(es->d_rec);
        B.q64 = es->d_C;
        hipLaunchKernelGGL(emit_record_kernel, dim3(nblk), dim3(kBlock), 0, sm, B);
        HIP_TRY(hipGetLastError());
        unsigned long long last_q = 0, last_c = 0;
        HIP_TRY(copy_sync(&last_q, es->d_C + (count - 1), 8, hipMemcpyDeviceToHost, sm));
        if ((rc = scan_exclusive(es->d_C, count, d_scr64, sm)) != ZRT_OK) return rc;
        HIP_TRY(copy_sync(&last_c, es->d_C + (count - 1), 8, hipMemcpyDeviceToHost, sm));
        es->Q = last_c + last_q;
    }
    HIP_TRY(hipStreamSynchronize(sm));
    undo.es = nullptr;
    *out = es;
    return ZRT_OK;
}

extern "C" int zrt_emitters_info(const zrt_emitters* es, uint32_t* num_emitters, uint64_t* total_q,
                                 uint32_t* num_triangles) {
    if (!es) return ZRT_ERR_INVALID_ARG;
    if (num_emitters) *num_emitters = es->count;
    if (total_q) *total_q = es->Q;
    if (num_triangles) *num_triangles = es->num_triangles;
    return ZRT_OK;
}

extern "C" int zrt_emitters_read(const zrt_emitters* es, zrt_emitter* records, uint64_t* prefix) {
    if (!es || !es->ctx) return ZRT_ERR_INVALID_ARG;
    if (es->count == 0u) return ZRT_OK;
    DeviceGuard g(es->device);
    if (records) HIP_TRY(copy_sync(records, es->d_rec, 80ull * es->count, hipMemcpyDeviceToHost, es->ctx->stream));
    if (prefix) HIP_TRY(copy_sync(prefix, es->d_C, 8ull * es->count, hipMemcpyDeviceToHost, es->ctx->stream));
    return ZRT_OK;
}

extern "C" void zrt_emitters_destroy(zrt_emitters* es) {
    if (!es) return;
    if (es->d_rec || es->d_C) {
        DeviceGuard g(es->device);
        if (es->d_rec) (void)hipFree(es->d_rec);
        if (es->d_C) (void)hipFree(es->d_C);
    }
    delete es;
}
