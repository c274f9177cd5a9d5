// emitters.h -- what render.hip (the query entry points) and emitters.hip (the
// emitter set and the area-light item kernels) share: the device
// functions of a hit's shading inputs, each defined once, and the two launches
// zrt_context_area_lights makes between its first hits and its chains.
#pragma once
#include "render_context.h"

namespace {

using namespace zrt;

constexpr float kFltEps = 1.1920928955078125e-07f;   // std.math.floatEps(f32)
constexpr float kInvPi = 0x1.45f306p-2f;       // 1 / pi rounded to f32, 0x3EA2F983

__device__ __forceinline__ void ray_load(const float* rays, uint32_t i, v3& o, v3& d) {
    const float* q = rays + 6ull * i;
    o = mk(q[0], q[1], q[2]);
    d = mk(q[3], q[4], q[5]);
}

// The shading inputs of a hit, stage3.zig:199-206: the arithmetic is
// shade_segment's (its lines "stage3.zig:199-206" to `nrm`), restated here
// because shade_segment is welded to the RNG draw and the queue append: keep
// the two in step.  surface_kernel and feature_walk_kernel share this one.  The
// four Data loads of a hit lane are issued together before any texel load
// (tri_rec's reason).  The materials are read from global memory whatever
// their number: a copy in LDS for up to kLdsMats of them, the shade kernel's
// LMATS, was built and measured beside surface_kernel and did not win in every
// round, so one path serves both sides of that limit.
struct SurfaceInputs {
    v3 nrm, albedo, emissive;
    float transparency, tc0, tc1;
    float mat;                // Data.material_idx, the bits of d3.w
};
__device__ __forceinline__ SurfaceInputs surface_gather(const float4* tri_data, const DevMat* mats, const float* texels,
                                                        float hu, float hv, uint32_t ref) {
    const float4* tdp = tri_data + 4ull * ref;
    const float4 d0 = tdp[0], d1 = tdp[1], d2 = tdp[2], d3 = tdp[3];   // stage3.zig:199-206
    SurfaceInputs g;
    const float w0 = 1.0f - hu - hv;
    g.tc0 = (d2.y * w0 + d2.w * hu) + d3.y * hv;
    g.tc1 = (d2.z * w0 + d3.x * hu) + d3.z * hv;
    const DevMat& m = mats[__float_as_uint(d3.w)];
    g.albedo = sample3(texels, m.tex[0], g.tc0, g.tc1);
    g.emissive = sample3(texels, m.tex[1], g.tc0, g.tc1);
    g.transparency = sample1(texels, m.tex[2], g.tc0, g.tc1);
    g.nrm = add(add(scale(mk(d0.x, d0.y, d0.z), w0), scale(mk(d0.w, d1.x, d1.y), hu)),
                scale(mk(d1.z, d1.w, d2.x), hv));
    g.mat = d3.w;
    return g;
}

__device__ __forceinline__ bool finite3(v3 a) {
    return fabsf(a.x) < kInf && fabsf(a.y) < kInf && fabsf(a.z) < kInf;       // (false for a NaN)
}

__device__ __forceinline__ uint4 hit_load(const uint32_t* hits, bool aligned, uint32_t ray) {
    if (aligned) return reinterpret_cast<const uint4*>(hits)[ray];
    const uint32_t* hq = hits + 4ull * ray;
    return make_uint4(hq[0], hq[1], hq[2], hq[3]);
}

}  // namespace

// Area-light queries (zrt_context_area_lights): zrt_context_direct
// with the (ray, light) item replaced by a (ray, sample) item whose light is
// drawn from the emitter set.  An item is item j of a sub-chunk of at most
// kAreaItems: (ray0 + (s0 + j) / S, (s0 + j) % S).  area_gen_kernel draws the
// emitter and the point on it, computes the item's direction, bound and
// contribution (include/zrt.h) and appends the traced items to a list of plain
// rays and bounds that the transmit_walk_kernel instantiations walk; every
// item keeps its contribution ((Le * alpha) * g, w unused) and its list slot
// (0xFFFFFFFF: not traced) in two dense rows.  area_reduce_kernel, one thread
// per ray, folds contribution * T in sample order into the ray's running E,
// which waits in the chunk's irradiance row between sub-chunks; with the ray's
// last sample it divides by S and writes the radiance.
struct AreaParams {
    const float* rays;        // this chunk: 6 floats per ray (origin, direction as given)
    const uint32_t* hits;     // this chunk: the zrt_hit of every ray as 4 u32 (4-byte aligned)
    const float4* tri_data;   // TraceParams::tri_data
    const zrt::DevMat* mats;
    const float* texels;
    const float4* rec;        // the set: 5 float4 (a zrt_emitter) per emitter
    const unsigned long long* C;   // ... and the exclusive prefix sums of q
    unsigned long long Q;     // their total
    unsigned long long seed;
    float Qf;                 // (float)Q
    uint32_t count;           // emitters (0: nothing is traced)
    uint32_t steps;           // ceil(log2(count + 1)): the search's trip count
    uint32_t key0;            // stream key of the chunk's ray 0, (uint32_t)(index_base + offset)
    uint32_t S;               // samples per ray, 1..65535
    uint32_t n;               // rays of this chunk
    uint32_t ray0, s0;        // the sub-chunk's first item: sample s0 of ray ray0
    uint32_t m;               // items of this sub-chunk (<= kAreaItems)
    uint32_t unshadowed;      // ZRT_AREA_UNSHADOWED: no list is written, T = 1
    uint32_t fold;            // area_reduce_kernel: the walk launches ran; move their counts
    float* irays;             // the list: 6 floats and a bound per entry
    float* ibound;
    const float* T;           // the walk's transmittance per list entry
    float4* contrib;          // the contribution of every item of the sub-chunk
    uint32_t* slot;           //   and its list entry, or 0xFFFFFFFF
    uint32_t* ctr;            // [4]: entries of the list
    float* E;                 // this chunk: the irradiance of every ray, 3 floats
    float* radiance;          // this chunk: 3 floats per ray, or null
    unsigned long long* stats;   // [kAreaStat]: the chains' segments, [kAreaStat + 1]: their crossings
};
constexpr uint32_t kAreaItems = 1u << 20;      // items per sub-chunk
constexpr uint32_t kAreaStat = 16;             // (stats[0..3] are the walk kernels', [0..15] the counting render's)

// emitters.hip's, for zrt_context_area_lights (hidden: not part of libzrt.so's interface)
#pragma GCC visibility push(hidden)
int area_gen_launch(const AreaParams& p, hipStream_t stream);
int area_reduce_launch(const AreaParams& p, uint32_t rays, hipStream_t stream);
#pragma GCC visibility pop

// Sky-light queries (zrt_context_sky_light): the area-light call
// with the emitter drawn replaced by the direction the path tracer scatters
// along, zrt_context_occlusion's draw about the normalised normal, and the
// bound by +inf.  sky_gen_kernel appends the traced items to the list and
// keeps every item's list slot (0xFFFFFFFF: not traced); the sky's colour
// depends on the direction's y alone, which is in the list entry, so no
// contribution row is kept: sky_reduce_kernel reads y back and computes
// env_color.  An unshadowed call therefore still writes the entries'
// directions (not their origins and bounds).  The running sums A and V of a
// ray wait in the chunk's irradiance and visibility rows between sub-chunks.
struct SkyParams {
    const float* rays;        // this chunk: 6 floats per ray (origin, direction as given)
    const uint32_t* hits;     // this chunk: the zrt_hit of every ray as 4 u32 (4-byte aligned)
    const float4* tri_data;   // TraceParams::tri_data
    const zrt::DevMat* mats;
    const float* texels;
    const double* zig;        // the ziggurat's tables (TraceParams::zig)
    unsigned long long seed;
    uint32_t key0;            // stream key of the chunk's ray 0, (uint32_t)(index_base + offset)
    uint32_t S;               // samples per ray, 1..65535
    uint32_t n;               // rays of this chunk
    uint32_t ray0, s0;        // the sub-chunk's first item: sample s0 of ray ray0
    uint32_t m;               // items of this sub-chunk (<= kAreaItems)
    uint32_t unshadowed;      // ZRT_SKY_UNSHADOWED: T = 1, the list holds directions only
    uint32_t fold;            // sky_reduce_kernel: the walk launches ran; move their counts
    float* irays;             // the list: 6 floats and a bound per entry
    float* ibound;
    const float* T;           // the walk's transmittance per list entry
    uint32_t* slot;           // the list entry of every item of the sub-chunk, or 0xFFFFFFFF
    uint32_t* ctr;            // [4]: entries of the list
    float* E;                 // this chunk: A, then the irradiance of every ray, 3 floats
    float* V;                 // this chunk: V, then the visibility of every ray
    float* radiance;          // this chunk: 3 floats per ray, or null
    unsigned long long* stats;   // [kAreaStat]: the chains' segments, [kAreaStat + 1]: their crossings
};

// sky.hip's, for zrt_context_sky_light (hidden, as above)
#pragma GCC visibility push(hidden)
int sky_gen_launch(const SkyParams& p, hipStream_t stream);
int sky_reduce_launch(const SkyParams& p, uint32_t rays, hipStream_t stream);
#pragma GCC visibility pop
