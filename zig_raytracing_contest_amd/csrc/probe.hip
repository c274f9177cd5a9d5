// probe.hip -- device-function parity probes behind zrt_probe (include/zrt.h).
#include <vector>

#include "render_context.h"

using namespace zrt;

// ---------------------------------------------------------------------------
// Device-function parity probes: the exact __device__ code paths of the
// kernel, evaluated on the GPU for the Tier-1 tests.
namespace {

__global__ void probe_kernel(int which, const void* in, void* out, uint32_t n, const void* aux,
                             const double* zig) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    switch (which) {
        case ZRT_PROBE_TRIANGLE: {
            const float* a = (const float*)in + 15ull * i;
            float* o = (float*)out + 4ull * i;
            const v3 v0 = ld3(a), v1 = ld3(a + 3), v2 = ld3(a + 6);
            float t = 0, u = 0, v = 0;
            const bool h = tri_ray(v0, sub(v1, v0), sub(v2, v0), ld3(a + 9), ld3(a + 12), &t, &u, &v);
            o[0] = h ? 1.0f : 0.0f; o[1] = t; o[2] = u; o[3] = v;
            break;
        }
        case ZRT_PROBE_TRIANGLE_EXACT: {  // the IEEE-division test of the mt_exact kernels
            const float* a = (const float*)in + 15ull * i;
            float* o = (float*)out + 4ull * i;
            const v3 v0 = ld3(a), v1 = ld3(a + 3), v2 = ld3(a + 6);
            float t = 0, u = 0, v = 0;
            const bool h = tri_ray<true>(v0, sub(v1, v0), sub(v2, v0), ld3(a + 9), ld3(a + 12), &t, &u, &v);
            o[0] = h ? 1.0f : 0.0f; o[1] = t; o[2] = u; o[3] = v;
            break;
        }
        case ZRT_PROBE_TRIANGLE_FLAT: {   // wf_park_kernel's branch-free test
            const float* a = (const float*)in + 15ull * i;
            float* o = (float*)out + 4ull * i;
            const v3 v0 = ld3(a), v1 = ld3(a + 3), v2 = ld3(a + 6);
            float t = 0, u = 0, v = 0;
            const bool h = tri_ray_flat(v0, sub(v1, v0), sub(v2, v0), ld3(a + 9), ld3(a + 12), &t, &u, &v);
            o[0] = h ? 1.0f : 0.0f; o[1] = h ? t : 0.0f; o[2] = h ? u : 0.0f; o[3] = h ? v : 0.0f;
            break;
        }
        case ZRT_PROBE_BBOX: {
            const float* a = (const float*)in + 12ull * i;
            float* o = (float*)out + 2ull * i;
            Bbox b; b.min = ld3(a); b.max = ld3(a + 3);
            float t = 0;
            const bool h = bbox_ray(b, ld3(a + 6), ld3(a + 9), &t);
            o[0] = h ? 1.0f : 0.0f; o[1] = h ? t : 0.0f;
            break;
        }
        case ZRT_PROBE_DDA: {
            // the kernels' own DDA: dda_init (Grid.traceRay) + DDA_STEP
            // (Iterator.next).  out: [0] steps (-1: misses the bbox, -2: the
            // incremental linear index disagreed with linearlizeCellIdx),
            // [1..3] first cell, then per step (cell after next(), t): the
            // reference's it.cell / it.next() pairs (linalg.zig:583-681)
            const float* a = (const float*)in + 12ull * i;
            const uint32_t* res = (const uint32_t*)aux;
            float* o = (float*)out + (4ull + 4ull * 64) * i;
            Bbox bb; bb.min = ld3(a); bb.max = ld3(a + 3);
            const uint32_t r3[3] = {res[0], res[1], res[2]};
            const Grid g = grid_init(bb, r3);
            const float bmin[3] = {bb.min.x, bb.min.y, bb.min.z}, bmax[3] = {bb.max.x, bb.max.y, bb.max.z};
            const float cs[3] = {g.cell_size.x, g.cell_size.y, g.cell_size.z};
            Dda s;
            // the park kernel's dda_init (dda_init_fq: the quotients from one
            // reciprocal per axis where exact, else dda_init)
            const float ics[3] = {1.0f / cs[0], 1.0f / cs[1], 1.0f / cs[2]};
            bool cs_ok = true;
            for (int k = 0; k < 3; ++k) cs_ok = cs_ok && fabsf(cs[k]) >= 0x1p-32f && fabsf(cs[k]) <= 0x1p32f;
            const bool in = dda_init_fq(bmin, bmax, r3, cs, ics, cs_ok, ld3(a + 6), ld3(a + 9), s);
            if (!in) { o[0] = -1.0f; break; }
            GridK gk;
            gk.rm0 = r3[0] - 1u; gk.rm1 = r3[1] - 1u; gk.rm2 = r3[2] - 1u;
            gk.str1 = r3[0]; gk.str2 = r3[0] * r3[1];
            o[1] = (float)s.c0; o[2] = (float)s.c1; o[3] = (float)s.c2;
            int nsteps = 0;
            bool lin_ok = true;
            while (nsteps < 64) {
                const uint32_t c0 = s.c0, c1 = s.c1, c2 = s.c2;
                lin_ok = lin_ok && s.lin == (c2 * r3[1] + c1) * r3[0] + c0;
                bool crossed;
                float te;
                DDA_STEP(s, gk, 0u, crossed, te);
                (void)crossed;
                float* e = o + 4 + 4 * nsteps;
                // at the exit cell next() returns +inf and leaves the cell
                if (te == kInf) { e[0] = (float)c0; e[1] = (float)c1; e[2] = (float)c2; }
                else { e[0] = (float)s.c0; e[1] = (float)s.c1; e[2] = (float)s.c2; }
                e[3] = te;
                ++nsteps;
                if (te == kInf) break;
            }
            o[0] = lin_ok ? (float)nsteps : -2.0f;
            break;
        }
        case ZRT_PROBE_TO_RGB: {
            const float* a = (const float*)in + 3ull * i;
            uint8_t c[3];
            to_rgb(ld3(a), c);
            float* o = (float*)out + 3ull * i;
            o[0] = c[0]; o[1] = c[1]; o[2] = c[2];
            break;
        }
        case ZRT_PROBE_RNG_F32:
        case ZRT_PROBE_RNG_NORM: {
            const uint32_t* a = (const uint32_t*)in + 3ull * i;
            Rng r;
            r.s = path_key((uint64_t)a[0], a[1], a[2]);
            float* o = (float*)out + 16ull * i;
            for (int k = 0; k < 16; ++k)
                o[k] = which == ZRT_PROBE_RNG_F32 ? rng_float(r) : (float)rng_norm64(r, zig, zig + 257);
            break;
        }
        case ZRT_PROBE_EXP_LOG: {
            const double x = ((const double*)in)[i];
            double* o = (double*)out + 2ull * i;
            o[0] = det_exp(x);
            o[1] = det_log(x);
            break;
        }
        case ZRT_PROBE_TEXTURE: {
            // aux: int32 {chans, w, h, umin, umax, vmin, vmax, 0} then texels
            const int32_t* h = (const int32_t*)aux;
            DevTex t;
            t.off = 0; t.w = h[1]; t.h = h[2]; t.umin = h[3]; t.umax = h[4]; t.vmin = h[5]; t.vmax = h[6];
            const float* tex = (const float*)(h + 8);
            dev_tex_inline(t, tex, h[0]);
            const float* a = (const float*)in + 2ull * i;
            float* o = (float*)out + 3ull * i;
            if (h[0] == 3) {
                const v3 r = sample3(tex, t, a[0], a[1]);
                o[0] = r.x; o[1] = r.y; o[2] = r.z;
            } else {
                o[0] = sample1(tex, t, a[0], a[1]); o[1] = 0; o[2] = 0;
            }
            break;
        }
        case ZRT_PROBE_QUOT: {
            const float* a = (const float*)in + 2ull * i;
            float* o = (float*)out + 2ull * i;
            o[0] = quot_rn(a[0], a[1], mt_inv_det<false>(a[1]));
            o[1] = a[0] / a[1];
            break;
        }
        case ZRT_PROBE_RECIP: {
            const float x = ((const float*)in)[i];
            float* o = (float*)out + 2ull * i;
            o[0] = mt_inv_det<false>(x);
            o[1] = mt_inv_det<true>(x);
            break;
        }
        default:
            break;
    }
}

// ZRT_PROBE_RECIP_SWEEP: every float bit pattern of [lo, lo + count), the
// short reciprocal against the IEEE division, bit for bit (NaN == NaN).
__global__ __launch_bounds__(kBlock) void recip_sweep_kernel(uint32_t lo, uint32_t count, uint32_t* out) {
    uint32_t bad = 0, first = 0xFFFFFFFFu;
    // (a 64-bit index: count + the grid's stride can pass 2^32, and a wrapped
    // 32-bit k would stay below count for ever)
    for (uint64_t k = (uint64_t)blockIdx.x * kBlock + threadIdx.x; k < count; k += (uint64_t)gridDim.x * kBlock) {
        const float x = __uint_as_float(lo + (uint32_t)k);
        const float a = mt_inv_det<false>(x), b = mt_inv_det<true>(x);
        const bool same = __float_as_uint(a) == __float_as_uint(b) || (a != a && b != b);
        if (!same) { ++bad; first = min(first, lo + (uint32_t)k); }
    }
    for (int o = 32; o > 0; o >>= 1) {
        bad += __shfl_xor(bad, o);
        first = min(first, (uint32_t)__shfl_xor(first, o));
    }
    if ((threadIdx.x & 63u) == 0 && bad) {
        atomicAdd(&out[0], bad);
        atomicMin(&out[1], first);
    }
}

// ZRT_PROBE_QUOT_SWEEP: every significand pair (a in [1, 2), b = 1 + s /
// 2^23 for s in [s0, s0 + ns)), quot_rn against the IEEE division, bit for bit.
__global__ __launch_bounds__(kBlock) void quot_sweep_kernel(uint32_t s0, uint32_t ns, uint32_t* out) {
    const uint64_t total = (uint64_t)ns << 23;
    uint32_t bad = 0;
    unsigned long long first = ~0ull;
    for (uint64_t k = (uint64_t)blockIdx.x * kBlock + threadIdx.x; k < total; k += (uint64_t)gridDim.x * kBlock) {
        const uint32_t ab = 0x3F800000u | (uint32_t)(k & 0x7FFFFFu);
        const uint32_t bb = 0x3F800000u | (s0 + (uint32_t)(k >> 23));
        const float a = __uint_as_float(ab), b = __uint_as_float(bb);
        const float q = quot_rn(a, b, mt_inv_det<false>(b));
        if (__float_as_uint(q) != __float_as_uint(a / b)) {
            ++bad;
            first = min(first, ((unsigned long long)bb << 32) | ab);
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        bad += __shfl_xor(bad, o);
        const unsigned lo = __shfl_xor((unsigned)first, o), hi = __shfl_xor((unsigned)(first >> 32), o);
        first = min(first, ((unsigned long long)hi << 32) | lo);
    }
    if ((threadIdx.x & 63u) == 0 && bad) {
        atomicAdd(&out[0], bad);
        atomicMin(reinterpret_cast<unsigned long long*>(out + 2), first);
    }
}

}  // namespace

extern "C" int zrt_probe(int which, const void* in, void* out, uint32_t n, const void* aux, int device) {
    if (!in || !out || n == 0) return ZRT_ERR_INVALID_ARG;
    size_t in_sz = 0, out_sz = 0, aux_sz = 0;
    switch (which) {
        case ZRT_PROBE_TRIANGLE:
        case ZRT_PROBE_TRIANGLE_EXACT:
        case ZRT_PROBE_TRIANGLE_FLAT: in_sz = 60; out_sz = 16; break;
        case ZRT_PROBE_BBOX: in_sz = 48; out_sz = 8; break;
        case ZRT_PROBE_DDA: in_sz = 48; out_sz = 4 * (4 + 4 * 64); aux_sz = 12; break;
        case ZRT_PROBE_TO_RGB: in_sz = 12; out_sz = 12; break;
        case ZRT_PROBE_RNG_F32:
        case ZRT_PROBE_RNG_NORM: in_sz = 12; out_sz = 64; break;
        case ZRT_PROBE_EXP_LOG: in_sz = 8; out_sz = 16; break;
        case ZRT_PROBE_RECIP: in_sz = 4; out_sz = 8; break;
        case ZRT_PROBE_RECIP_SWEEP: in_sz = 8; out_sz = 16; break;
        case ZRT_PROBE_QUOT: in_sz = 8; out_sz = 8; break;
        case ZRT_PROBE_QUOT_SWEEP: in_sz = 8; out_sz = 16; break;
        case ZRT_PROBE_TEXTURE: {
            in_sz = 8; out_sz = 12;
            if (!aux) return ZRT_ERR_INVALID_ARG;
            const int32_t* h = (const int32_t*)aux;
            if ((h[0] != 1 && h[0] != 3) || h[1] <= 0 || h[2] <= 0) return ZRT_ERR_INVALID_ARG;
            aux_sz = 32 + 4ull * h[0] * h[1] * h[2];
            break;
        }
        default: return ZRT_ERR_INVALID_ARG;
    }
    if (aux_sz && !aux) return ZRT_ERR_INVALID_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return ZRT_ERR_NO_DEVICE;
    DeviceGuard g(device);
    void *d_in = nullptr, *d_out = nullptr, *d_aux = nullptr;
    double* d_zig = nullptr;
    double zig[514];
    zig_tables(zig, zig + 257);
    int rc = ZRT_OK;
    auto cleanup = [&]() {
        if (d_in) (void)hipFree(d_in);
        if (d_out) (void)hipFree(d_out);
        if (d_aux) (void)hipFree(d_aux);
        if (d_zig) (void)hipFree(d_zig);
    };
    auto run = [&]() -> int {
        HIP_TRY(hipMalloc(&d_in, in_sz * n));
        HIP_TRY(hipMalloc(&d_out, out_sz * n));
        HIP_TRY(hipMalloc((void**)&d_zig, sizeof zig));
        HIP_TRY(hipMemcpy(d_in, in, in_sz * n, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d_zig, zig, sizeof zig, hipMemcpyHostToDevice));
        if (aux_sz) {
            HIP_TRY(hipMalloc(&d_aux, aux_sz));
            HIP_TRY(hipMemcpy(d_aux, aux, aux_sz, hipMemcpyHostToDevice));
        }
        if (which == ZRT_PROBE_QUOT_SWEEP) {
            // out per range: {mismatches, 0, first (a bits, b bits) as a u64 min}
            const uint32_t* r = (const uint32_t*)in;
            std::vector<uint32_t> init(4ull * n, 0u);
            for (uint32_t k = 0; k < n; ++k) init[4ull * k + 2] = init[4ull * k + 3] = 0xFFFFFFFFu;
            HIP_TRY(hipMemcpy(d_out, init.data(), out_sz * n, hipMemcpyHostToDevice));
            for (uint32_t k = 0; k < n; ++k) {
                if (r[2 * k + 1] == 0) continue;
                if ((uint64_t)r[2 * k] + r[2 * k + 1] > (1ull << 23)) return ZRT_ERR_INVALID_ARG;
                hipLaunchKernelGGL(quot_sweep_kernel, dim3(16384), dim3(kBlock), 0, 0, r[2 * k], r[2 * k + 1],
                                   (uint32_t*)d_out + 4ull * k);
                HIP_TRY(hipGetLastError());
            }
        } else if (which == ZRT_PROBE_RECIP_SWEEP) {
            const uint32_t* r = (const uint32_t*)in;
            std::vector<uint32_t> init(4ull * n, 0u);
            for (uint32_t k = 0; k < n; ++k) init[4ull * k + 1] = 0xFFFFFFFFu;
            HIP_TRY(hipMemcpy(d_out, init.data(), out_sz * n, hipMemcpyHostToDevice));
            for (uint32_t k = 0; k < n; ++k) {
                if (r[2 * k + 1] == 0) continue;
                if ((uint64_t)r[2 * k] + r[2 * k + 1] > 0x100000000ull) return ZRT_ERR_INVALID_ARG;
                const uint32_t blocks = std::min<uint32_t>(8192u, (r[2 * k + 1] + kBlock - 1) / kBlock);
                hipLaunchKernelGGL(recip_sweep_kernel, dim3(blocks), dim3(kBlock), 0, 0, r[2 * k], r[2 * k + 1],
                                   (uint32_t*)d_out + 4ull * k);
                HIP_TRY(hipGetLastError());
            }
        } else {
            hipLaunchKernelGGL(probe_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, which, d_in, d_out, n,
                               d_aux, d_zig);
        }
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipMemcpy(out, d_out, out_sz * n, hipMemcpyDeviceToHost));
        return ZRT_OK;
    };
    rc = run();
    cleanup();
    return rc;
}
