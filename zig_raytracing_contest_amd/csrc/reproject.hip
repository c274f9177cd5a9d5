// reproject.hip -- zrt_context_reproject (include/zrt.h): the
// previous frame's colour fetched where each pixel of the current frame was
// seen from the previous camera, blended by 1 / history length.
//
// Two kernels on the context's stream, two launches per call:
//   reproject_gather_kernel   one thread per packed pixel k, p = pix[k]: the
//                             previous planes scattered into row-major 16-byte
//                             records
//                               R0[p] = (colour rgb, depth)
//                               R1[p] = (normal xyz, length bits), only if the
//                                       normals guide or lengths are given
//                             so that a tap is one or two dwordx4 loads, and so
//                             that the previous planes are read completely
//                             before anything is written (the outputs may be the
//                             previous colour and length planes themselves).
//   reproject_kernel          one thread per packed k: the camera vectors and
//                             the per-call constants are kernel arguments
//                             (SGPRs), the current planes load coalesced at k,
//                             the four taps' records -- packed order walks
//                             8 x 8 blocks, so a wave's taps stay close -- are
//                             loaded together before any tap is judged, and the
//                             colour, length and motion stores go at k.  The pixels with history are counted by a
//                             ballot per wave and one integer atomic per wave.
//                             Templated on what is given: an absent normal
//                             guide, length plane, film or motion output costs
//                             no load, no store and no branch.
// Every operation is written as the header states it; the unit is compiled
// with -ffp-contract=off like the rest, so nothing fuses.
#include "render_context.h"

using namespace zrt;

namespace {

// The count of pixels with history: kHitSlots counters, one cache line apart,
// a wave adding to the slot of its number -- every wave's atomic on one address
// queues at one L2 channel (0.225 against 0.063 ms per 1080p call, DESIGN
// 5.23).  The host adds the slots up.
constexpr uint32_t kHitSlots = 64, kHitStride = 32;       // (slots; u32 words between them: 128 B)
constexpr uint32_t kHitWords = kHitSlots * kHitStride;    // 8 KB at the end of the records

struct GatherParams {
    const float* color;        // previous planes, packed order
    const float* depth;
    const float* normal;       // or null: not a guide in this call
    const uint32_t* length;    // or null
    const uint32_t* pix;       // packed k -> row-major p; null: p = k
    uint32_t P;
    float4* R0;
    float4* R1;
    uint32_t* hits;            // zeroed here for the launch that follows
};

__global__ __launch_bounds__(kBlock) void reproject_gather_kernel(const GatherParams g) {
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
    if (k < kHitSlots) g.hits[k * kHitStride] = 0u;          // (block 0 is whole: kBlock >= kHitSlots)
    if (k >= g.P) return;
    const uint32_t p = g.pix ? g.pix[k] : k;
    g.R0[p] = make_float4(g.color[3 * (size_t)k], g.color[3 * (size_t)k + 1], g.color[3 * (size_t)k + 2], g.depth[k]);
    if (g.normal || g.length) {
        const float len = __uint_as_float(g.length ? g.length[k] : 1u);
        g.R1[p] = g.normal ? make_float4(g.normal[3 * (size_t)k], g.normal[3 * (size_t)k + 1],
                                         g.normal[3 * (size_t)k + 2], len)
                           : make_float4(0.0f, 0.0f, 0.0f, len);
    }
}

struct ReprojectParams {
    // the current camera, the previous origin, and A, B, Cv of the previous one (negated if D < 0)
    v3 O, L, R, U, Op, A, B, Cv;
    float tn2, dtol;
    uint32_t usable;           // D is neither zero nor NaN
    uint32_t w, h, P;
    uint32_t max_m1;           // max_history - 1
    const uint32_t* pix;       // packed k -> row-major p; null: p = k
    const float* color;        // P * 3, or the film's:
    const float4* sum;         // its sums, packed order
    const float4* state;       // its adaptive state (w: kFilmFrozen | n), or null
    uint32_t samples;          // its samples
    const float* depth;
    const float* normal;
    const float4* R0;
    const float4* R1;
    float* color_out;
    uint32_t* length_out;      // or null
    float* motion;
    uint32_t* hits;
};

__device__ __forceinline__ bool is_finite(float x) { return fabsf(x) < kInf; }    // (false for a NaN)

template <bool NRM, bool LEN, bool FILM, bool MOTION>
__global__ __launch_bounds__(kBlock) void reproject_kernel(const ReprojectParams r) {
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
    bool has = false;
    if (k < r.P) {
        const uint32_t p = r.pix ? r.pix[k] : k;
        const uint32_t y = p / r.w, x = p - y * r.w;
        float cx, cy, cz;
        if (FILM) {                                            // film_present_kernel's linear
            const uint32_t sw = r.state ? __float_as_uint(r.state[k].w) : 0u;
            const uint32_t n = (sw & kFilmFrozen) ? (sw & ~kFilmFrozen) : r.samples;
            const float4 a = r.sum[k];
            const float inv = 1.0f / (float)n;
            cx = a.x * inv;
            cy = a.y * inv;
            cz = a.z * inv;
        } else {
            cx = r.color[3 * (size_t)k];
            cy = r.color[3 * (size_t)k + 1];
            cz = r.color[3 * (size_t)k + 2];
        }
        const float z = r.depth[k];
        float nx = 0.0f, ny = 0.0f, nz = 0.0f;
        if (NRM) {
            nx = r.normal[3 * (size_t)k];
            ny = r.normal[3 * (size_t)k + 1];
            nz = r.normal[3 * (size_t)k + 2];
        }
        const float px = (float)x + 0.5f, py = (float)y + 0.5f;
        const float nan = __uint_as_float(0x7FC00000u);
        float mx = nan, my = nan;
        float Sx = 0.0f, Sy = 0.0f, Sz = 0.0f, W = 0.0f;
        uint32_t M = 0xFFFFFFFFu;
        if (r.usable && z > 0.0f && z < kInf) {
            const v3 d = normalize(add(add(r.L, scale(r.R, px)), scale(r.U, py)));
            const v3 q = sub(add(r.O, scale(d, z)), r.Op);
            const float g = dot(q, r.Cv);
            if (g > 0.0f) {
                const float a = dot(q, r.A) / g, b = dot(q, r.B) / g;
                const float zq = sqrtf(dot(q, q));
                mx = a - px;
                my = b - py;
                const float fx = a - 0.5f, fy = b - 0.5f;
                if (fx > -1.0f && fx < (float)r.w && fy > -1.0f && fy < (float)r.h) {
                    // (-1 <= floorf < w, h <= 2^31: the conversions are in range)
                    const int x0 = (int)floorf(fx), y0 = (int)floorf(fy);
                    const float tx = fx - (float)x0, ty = fy - (float)y0;
                    // the four taps' records first, all loads in flight together (a tap outside the image
                    // loads the pixel's own record, which is not used); the skips then run on registers, in order
                    float4 r0[4], r1[4];
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        // (a tap left of or above the image wraps to 2^32 - 1 >= w, h)
                        const uint32_t qx = (uint32_t)(x0 + (t & 1)), qy = (uint32_t)(y0 + (t >> 1));
                        const size_t at = (qx < r.w && qy < r.h) ? (size_t)qy * (size_t)r.w + (size_t)qx : (size_t)p;
                        r0[t] = r.R0[at];
                        if (NRM || LEN) r1[t] = r.R1[at];
                    }
                    const float ztol = r.dtol * zq;
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
#pragma unroll
                        for (int i = 0; i < 2; ++i) {
                            const uint32_t qx = (uint32_t)(x0 + i), qy = (uint32_t)(y0 + j);
                            if (qx >= r.w || qy >= r.h) continue;
                            const float bw = (i ? tx : 1.0f - tx) * (j ? ty : 1.0f - ty);
                            if (!(bw > 0.0f)) continue;
                            const float4 t0 = r0[2 * j + i];
                            if (!(t0.w > 0.0f)) continue;
                            if (!(fabsf(t0.w - zq) <= ztol)) continue;
                            uint32_t lp = 1u;
                            if (NRM || LEN) {
                                const float4 t1 = r1[2 * j + i];
                                if (NRM) {
                                    const float d0 = nx - t1.x, d1 = ny - t1.y, d2 = nz - t1.z;
                                    if (!(((d0 * d0 + d1 * d1) + d2 * d2) <= r.tn2)) continue;
                                }
                                if (LEN) lp = __float_as_uint(t1.w);
                            }
                            if (!(is_finite(t0.x) && is_finite(t0.y) && is_finite(t0.z))) continue;
                            if (lp == 0u) continue;
                            Sx = Sx + t0.x * bw;
                            Sy = Sy + t0.y * bw;
                            Sz = Sz + t0.z * bw;
                            W = W + bw;
                            M = min(M, lp);
                        }
                    }
                }
            }
        }
        uint32_t N = 1u;
        has = W > 0.0f;
        if (has) {
            N = min(M, r.max_m1) + 1u;
            if (N > 1u) {                                      // (N == 1: the current colour's bits)
                const float alpha = 1.0f / (float)N, keep = 1.0f - alpha;
                cx = ((Sx / W) * keep) + (cx * alpha);
                cy = ((Sy / W) * keep) + (cy * alpha);
                cz = ((Sz / W) * keep) + (cz * alpha);
            }
        }
        r.color_out[3 * (size_t)k] = cx;
        r.color_out[3 * (size_t)k + 1] = cy;
        r.color_out[3 * (size_t)k + 2] = cz;
        if (r.length_out) r.length_out[k] = N;
        if (MOTION) {
            r.motion[2 * (size_t)k] = mx;
            r.motion[2 * (size_t)k + 1] = my;
        }
    }
    // every lane of the wave arrives here; the count is an integer: the same in any order
    const unsigned long long m = __ballot(has);
    if ((threadIdx.x & 63u) == 0u && m != 0ull)
        atomicAdd(r.hits + ((k >> 6) & (kHitSlots - 1u)) * kHitStride, (uint32_t)__popcll(m));
}

using ReprojectFn = void (*)(const ReprojectParams);
template <int V> constexpr ReprojectFn variant() {
    return reproject_kernel<(V & 1) != 0, (V & 2) != 0, (V & 4) != 0, (V & 8) != 0>;
}
// The kernel for what this call is given.
ReprojectFn reproject_variant(bool nrm, bool len, bool film, bool motion) {
    static const ReprojectFn f[16] = {variant<0>(),  variant<1>(),  variant<2>(),  variant<3>(), variant<4>(),  variant<5>(),
                                      variant<6>(),  variant<7>(),  variant<8>(),  variant<9>(), variant<10>(), variant<11>(),
                                      variant<12>(), variant<13>(), variant<14>(), variant<15>()};
    return f[(nrm ? 1 : 0) | (len ? 2 : 0) | (film ? 4 : 0) | (motion ? 8 : 0)];
}

}  // namespace

extern "C" int zrt_context_reproject(zrt_context* c, const zrt_reproject_batch* b, zrt_stats* stats) {
    if (!c || !reproject_batch_ok(b)) return ZRT_ERR_INVALID_ARG;
    const bool row_major = (b->flags & ZRT_REPROJECT_ROW_MAJOR) != 0u;
    const uint32_t tile = b->tile_size ? b->tile_size : 64u;
    const uint32_t w = b->camera->w, h = b->camera->h;
    const zrt_film* f = b->film;
    if (f && (f->ctx != c || f->w != w || f->h != h || f->tile != tile || f->rank != 0u || f->nranks != 1u ||
              f->samples == 0u))
        return ZRT_ERR_INVALID_ARG;
    const uint32_t P = (uint32_t)((uint64_t)w * h);            // (<= 2^31: reproject_batch_ok)
    const bool host = b->on_device == 0u;
    const bool nrm = b->normal && b->prev_normal, len = b->prev_length != nullptr;
    DeviceGuard g(c->device);

    int rc;
    if (!row_major) {
        zrt_camera cam{};
        zrt_render_config cfg{};
        cam.w = w;
        cam.h = h;
        cfg.tile_size = tile;
        if ((rc = rank_pixels(c, &cam, &cfg, 1)) != ZRT_OK) return rc;
        if (c->pix.size() != P || (f && f->n_owned != P)) return ZRT_ERR_INVALID_ARG;
    }
    // the records R0, R1 and the counters; a host call's planes in, then out:
    // colour 3P | depth P | normal 3P | previous colour 3P | depth P | normal 3P | length P floats;
    // colour 3P | length P | motion 2P
    if ((rc = grow(&c->d_rp, &c->rp_cap, 2ull * P + kHitWords / 4u)) != ZRT_OK) return rc;
    if (host && (rc = grow(&c->d_rpio, &c->rpio_cap, 21ull * P)) != ZRT_OK) return rc;
    while (c->ev_trace.size() < 2) {
        hipEvent_t e;
        HIP_TRY(hipEventCreateWithFlags(&e, hipEventDefault));
        c->ev_trace.push_back(e);
    }
    // capacity guard: every buffer a launch below writes holds what it writes
    if (!c->d_rp || c->rp_cap < 2ull * P + kHitWords / 4u || (host && (!c->d_rpio || c->rpio_cap < 21ull * P)) ||
        (!row_major && (!c->d_pix || c->pix_cap < P)) || (f && !f->d_sum))
        return ZRT_ERR_INVALID_ARG;

    // the per-call constants, in f32 as the header writes them
    const v3 Lp = ld3(b->prev_camera->lower_left_corner), Rp = ld3(b->prev_camera->right), Up = ld3(b->prev_camera->up);
    ReprojectParams R{};
    R.O = ld3(b->camera->origin);
    R.L = ld3(b->camera->lower_left_corner);
    R.R = ld3(b->camera->right);
    R.U = ld3(b->camera->up);
    R.Op = ld3(b->prev_camera->origin);
    R.A = cross(Up, Lp);
    R.B = cross(Lp, Rp);
    R.Cv = cross(Rp, Up);
    const float D = dot(Lp, R.Cv);
    if (D < 0.0f) {
        R.A = scale(R.A, -1.0f);
        R.B = scale(R.B, -1.0f);
        R.Cv = scale(R.Cv, -1.0f);
    }
    R.usable = (D < 0.0f || D > 0.0f) ? 1u : 0u;
    R.tn2 = nrm ? b->normal_tolerance * b->normal_tolerance : 0.0f;
    R.dtol = b->depth_tolerance;
    R.w = w;
    R.h = h;
    R.P = P;
    R.max_m1 = b->max_history - 1u;

    GatherParams G{};
    G.color = b->prev_color;
    G.depth = b->prev_depth;
    G.normal = nrm ? b->prev_normal : nullptr;
    G.length = b->prev_length;
    R.color = b->color;
    R.depth = b->depth;
    R.normal = nrm ? b->normal : nullptr;
    R.color_out = b->color_out;
    R.length_out = b->length_out;
    R.motion = b->motion;
    HIP_TRY(hipEventRecord(c->ev_begin, c->stream));
    float* const s = c->d_rpio;
    if (host) {
        const struct { const void** dev; const void* src; size_t at, words; } in[7] = {
            {(const void**)&R.color, b->color, 0, 3ull * P},
            {(const void**)&R.depth, b->depth, 3ull * P, P},
            {(const void**)&R.normal, R.normal, 4ull * P, 3ull * P},
            {(const void**)&G.color, b->prev_color, 7ull * P, 3ull * P},
            {(const void**)&G.depth, b->prev_depth, 10ull * P, P},
            {(const void**)&G.normal, G.normal, 11ull * P, 3ull * P},
            {(const void**)&G.length, b->prev_length, 14ull * P, P}};
        for (const auto& k : in) {
            if (!k.src) continue;
            HIP_TRY(copy_sync(s + k.at, k.src, 4ull * k.words, hipMemcpyHostToDevice, c->stream));
            *k.dev = s + k.at;
        }
        R.color_out = s + 15ull * P;
        R.length_out = b->length_out ? reinterpret_cast<uint32_t*>(s + 18ull * P) : nullptr;
        R.motion = b->motion ? s + 19ull * P : nullptr;
    }
    if (f) {
        R.sum = f->d_sum;
        R.state = f->d_state && !f->state_stale ? f->d_state : nullptr;
        R.samples = f->samples;
    }
    G.pix = R.pix = row_major ? nullptr : c->d_pix;
    G.P = P;
    G.R0 = c->d_rp;
    G.R1 = c->d_rp + P;
    R.R0 = G.R0;
    R.R1 = G.R1;
    G.hits = R.hits = reinterpret_cast<uint32_t*>(c->d_rp + 2ull * P);

    const uint32_t blocks = (P + kBlock - 1) / kBlock;
    HIP_TRY(hipEventRecord(c->ev_trace[0], c->stream));
    hipLaunchKernelGGL(reproject_gather_kernel, dim3(blocks), dim3(kBlock), 0, c->stream, G);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(reproject_variant(nrm, len, f != nullptr, b->motion != nullptr), dim3(blocks), dim3(kBlock), 0,
                       c->stream, R);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->ev_trace[1], c->stream));
    if (host) {
        HIP_TRY(copy_sync(b->color_out, R.color_out, 12ull * P, hipMemcpyDeviceToHost, c->stream));
        if (b->length_out) HIP_TRY(copy_sync(b->length_out, R.length_out, 4ull * P, hipMemcpyDeviceToHost, c->stream));
        if (b->motion) HIP_TRY(copy_sync(b->motion, R.motion, 8ull * P, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(hipEventRecord(c->ev_end, c->stream));
    uint32_t slots[kHitWords], hits = 0;
    HIP_TRY(copy_sync(slots, R.hits, sizeof slots, hipMemcpyDeviceToHost, c->stream));
    for (uint32_t i = 0; i < kHitSlots; ++i) hits += slots[i * kHitStride];
    zrt_stats st{};
    float ms = 0.0f;
    HIP_TRY(hipEventElapsedTime(&ms, c->ev_begin, c->ev_end));
    st.render_ms = ms;
    if (host) HIP_TRY(hipEventElapsedTime(&ms, c->ev_trace[0], c->ev_trace[1]));   // (without the staging copies)
    st.trace_kernel_ms = ms;
    st.samples = P;
    st.hits = hits;
    st.trace_launches = 2u;
    if (stats) *stats = st;
    return ZRT_OK;
}
