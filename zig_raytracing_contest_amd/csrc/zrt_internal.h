// zrt_internal.h -- types shared by the host code and the CDNA4 kernels.
#pragma once
#include <cstring>

#include "../../include/zrt.h"
#include "zrt_math.h"

// An emitter set (zrt_emitters_*, emitters.hip): device memory on
// its context's device, read-only once built.
struct zrt_emitters {
    zrt_context* ctx = nullptr;
    int device = 0;                    // ctx's (zrt_emitters_destroy does not touch ctx)
    uint32_t num_triangles = 0;        // of the source soup
    uint32_t count = 0;                // emitters
    uint64_t Q = 0;                    // the total of q
    float* d_rec = nullptr;            // count zrt_emitter records (16-byte aligned)
    unsigned long long* d_C = nullptr; // count exclusive prefix sums of q
};

namespace zrt {

// Device texture descriptor (stage3.zig:82-92): offset in floats into the
// texel pool; chans = 3 for colour, 1 for transparency.
struct DevTex {
    uint32_t off;
    int32_t w, h, umin, umax, vmin, vmax;
    uint32_t pad;
};
struct DevMat { DevTex tex[3]; };   // base_color, emissive, transparency
// A 1x1 texture (every material slot without an image, stage1.zig:411-425)
// needs no clamp range (any clamp and @mod by 1 give texel 0), so its texel
// rides in those fields instead: channel k's f32 bits in (umin, umax,
// vmin)[k].  Sampling then reads it from the material (LDS in the shade
// kernel) instead of the texel pool.
ZHD void dev_tex_inline(DevTex& d, const float* texels, int chans) {
    if (d.w != 1 || d.h != 1) return;
    int32_t* f[3] = {&d.umin, &d.umax, &d.vmin};
    for (int k = 0; k < chans; ++k) memcpy(f[k], texels + d.off + k, 4);
}

#if defined(__HIPCC__)
// Texture(T).sample (stage3.zig:111-123).  A 1x1 texture -- the dummy of
// every material slot without an image (stage1.zig:411-425) -- has all four
// texel indices 0 (any clamp, @mod by 1), so it loads its texel once and
// runs the same bilinear arithmetic on it (bit-identical: x - x is not
// folded, NaN/inf weights propagate as before), instead of the index
// arithmetic and four loads per channel.
__device__ __forceinline__ v3 sample3(const float* texels, const DevTex& t, float u, float v) {
    const float* b = texels + t.off;
    if (t.w == 1 && t.h == 1) {
        const float fu = tex_frac(u), fv = tex_frac(v);
        // the texel, inlined in the descriptor (dev_tex_inline)
        const float x = __int_as_float(t.umin), y = __int_as_float(t.umax), z = __int_as_float(t.vmin);
        return mk(bilerp(x, x, x, x, fu, fv), bilerp(y, y, y, y, fu, fv), bilerp(z, z, z, z, fu, fv));
    }
    const TexCoords c = tex_coords(t.w, t.h, t.umin, t.umax, t.vmin, t.vmax, u, v);
    v3 r;
    r.x = bilerp(b[3 * c.i11 + 0], b[3 * c.i21 + 0], b[3 * c.i12 + 0], b[3 * c.i22 + 0], c.fu, c.fv);
    r.y = bilerp(b[3 * c.i11 + 1], b[3 * c.i21 + 1], b[3 * c.i12 + 1], b[3 * c.i22 + 1], c.fu, c.fv);
    r.z = bilerp(b[3 * c.i11 + 2], b[3 * c.i21 + 2], b[3 * c.i12 + 2], b[3 * c.i22 + 2], c.fu, c.fv);
    return r;
}
__device__ __forceinline__ float sample1(const float* texels, const DevTex& t, float u, float v) {
    const float* b = texels + t.off;
    if (t.w == 1 && t.h == 1) {                           // the 1x1 dummy (see sample3)
        const float x = __int_as_float(t.umin);
        return bilerp(x, x, x, x, tex_frac(u), tex_frac(v));
    }
    const TexCoords c = tex_coords(t.w, t.h, t.umin, t.umax, t.vmin, t.vmax, u, v);
    return bilerp(b[c.i11], b[c.i21], b[c.i12], b[c.i22], c.fu, c.fv);
}
#endif

// Ziggurat NormDist tables (Zig std ziggurat.zig ZigTableGen), computed on the
// host with the deterministic exp/log of zrt_math.h.
void zig_tables(double zx[257], double zf[257]);

// Host threads for "all CPUs" (config.json num_threads null, main.zig:90
// getCpuCount): the CPUs this process may run on, capped by OMP_NUM_THREADS
// when set (the per-GPU CPU share on shared GPU hosts).
unsigned host_threads();

// Whether the park kernel's exact per-cell occupancy (OccX) serves a grid:
// its 4^3-cell bricks need 24-bit indices (__umul24 in the kernels), the
// occupied-brick count before a 32-brick word must fit the u16 prefix, and
// the blob must fit the LDS left beside the per-wave slots.  Otherwise the
// bounces take the lane walk (wf_kernel, coarsened brick bits): the render
// still runs, on every grid the reference accepts (u32 resolution, < 2^31
// cells), with the same image.
inline bool occx_usable(uint64_t bricks, uint64_t occupied, uint64_t lds_bytes, uint64_t budget) {
    return bricks <= (1ull << 24) && occupied < 0xFFFFull && lds_bytes <= budget;
}

// Host-side packed pixel order of one rank (zrt_tile_pixels).
int tile_pixels(uint32_t w, uint32_t h, uint32_t tile, uint32_t rank, uint32_t nranks,
                uint32_t* out, uint32_t* count);

// zrt_context_direct's argument checks, which need no device (capi.cpp): the
// batch's scalar fields, then -- num_rays != 0 -- its pointers and the lights'
// types.  `trace_flags`: the flags zrt_context_trace accepts.
bool direct_batch_ok(const zrt_direct_batch* b, uint32_t trace_flags);

// zrt_context_area_lights', likewise: the batch's scalar fields, then --
// num_rays != 0 -- its pointers and whether the set was made on `c`.
bool area_light_batch_ok(const zrt_context* c, const zrt_area_light_batch* b, uint32_t trace_flags);

// zrt_context_sky_light's, likewise: the batch's scalar fields, then --
// num_rays != 0 -- its pointers.
bool sky_light_batch_ok(const zrt_sky_light_batch* b, uint32_t trace_flags);

// zrt_context_light_probes' argument checks, which need no device (capi.cpp):
// the batch's scalar fields, then -- num_probes != 0 -- its size (at most 2^47
// probes) and its pointers.
// `probe_flags`: the flags the call accepts (zrt_context_radiance's without
// ZRT_RADIANCE_PER_SAMPLE).  max_bounce > 32 is not refused here: it is
// ZRT_ERR_UNSUPPORTED, the caller's to tell apart.
bool light_probe_batch_ok(const zrt_light_probe_batch* b, uint32_t probe_flags);

// zrt_context_denoise's argument checks, which need no device (capi.cpp): every
// refusal of the header but those that read the film.
bool denoise_batch_ok(const zrt_denoise_batch* b);

// zrt_context_reproject's, likewise.
bool reproject_batch_ok(const zrt_reproject_batch* b);

// zrt_context_illumination's and zrt_context_svgf's, likewise.
bool illumination_batch_ok(const zrt_illumination_batch* b);
bool svgf_batch_ok(const zrt_svgf_batch* b);

// The packed RGB8 of a context's last render (device memory on its device,
// 3 * pixels bytes in its rank's zrt_tile_pixels order): what a device group
// gathers (group.hip).
int context_device_rgb(const zrt_context* c, const uint8_t** d_rgb, uint32_t* pixels, int* device);

// Contexts of one group that share a device render at the same time: each
// sizes its passes from 1/share of the device's queue budget (group.hip sets
// share = how often the device appears in the list).
void context_set_mem_share(zrt_context* c, uint32_t share);

// The context's main HIP stream (as a void*: this header has no HIP types):
// a group gathers on its first context's stream instead of creating one of
// its own (a stream's first hardware queue cost ~10-17 ms of the CLI's
// start-up, r06d).
void* context_stream(const zrt_context* c);

}  // namespace zrt
