/*
 * zrt.h -- C ABI of the MI355X-native render hot path (libzrt.so).
 *
 * Drop-in boundary for the reference's render seam
 *     pub fn render(self: Scene, threads: []std.Thread, camera: Camera,
 *                   img: []RGB) !void                  (src/stage3.zig:247)
 * called once from src/main.zig:126.  The reference has no plugin registry;
 * its only FFI mechanism is @cImport of C headers (src/c.zig:1-5) plus a
 * static C library linked by build.zig:29-48, so a Zig host binds this
 * header the same way.
 *
 * Zig's @Vector(3, f32) (16-byte padded) and std.MultiArrayList are not
 * C-ABI, so the Scene is passed FLATTENED: plain pointers and sizes, caller
 * owned, read-only for the duration of the call.  All functions are
 * synchronous, return 0 (ZRT_OK) or a negative zrt_status, and never throw.
 * No torch types appear anywhere in this interface.
 */
#ifndef ZRT_H
#define ZRT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ZRT_ABI_VERSION 2      /* 2: device list in zrt_render_config, zrt_group_* */

typedef enum zrt_status {
    ZRT_OK = 0,
    ZRT_ERR_INVALID_ARG = -1,     /* null pointer, zero size, inconsistent scene */
    ZRT_ERR_NO_DEVICE = -2,       /* no HIP device / bad ordinal */
    ZRT_ERR_HIP = -3,             /* a HIP runtime call failed */
    ZRT_ERR_OUT_OF_MEMORY = -4,   /* host or device allocation failed */
    ZRT_ERR_UNSUPPORTED = -5,     /* e.g. max_bounce above the compiled stack depth */
    ZRT_ERR_IO = -6,              /* file open/read/write failed */
    ZRT_ERR_PARSE = -7,           /* glTF / JSON / PNG malformed */
    ZRT_ERR_NOT_FOUND = -8,       /* camera name not found, no cameras (stage1.zig:282-307) */
    ZRT_ERR_CAMERA = -9,          /* stage1.zig:322-342 width/height/aspect-ratio rules */
} zrt_status;

/* ---- scene (stage3.zig:136-143 Scene, flattened) ------------------------ */

/* linalg.zig:407-410 Grid */
typedef struct zrt_grid {
    float bbox_min[3];
    float bbox_max[3];
    uint32_t resolution[3];
    float cell_size[3];              /* (bbox_max - bbox_min) / resolution, f32 */
} zrt_grid;

/* stage3.zig:82-92 Texture(T).  `offset` indexes zrt_scene.texels in floats;
 * colour textures hold 3 floats per texel (linear RGB, factor applied),
 * transparency textures 1 float per texel.  Rows top to bottom.
 * u/v_min/max: [0, w-1] for CLAMP_TO_EDGE, [INT32_MIN, INT32_MAX] for repeat
 * (stage1.zig:381-409); a missing texture is a 1x1 texel = factor
 * (stage1.zig:411-425). */
typedef struct zrt_texture {
    uint64_t offset;
    int32_t w, h;
    int32_t u_min, u_max, v_min, v_max;
    int32_t _pad;
} zrt_texture;

/* stage3.zig:125-129 Material */
typedef struct zrt_material {
    zrt_texture base_color;          /* 3 floats/texel */
    zrt_texture emissive;            /* 3 floats/texel */
    zrt_texture transparency;        /* 1 float/texel  */
} zrt_material;

typedef struct zrt_scene {
    zrt_grid grid;
    uint32_t num_cells;              /* resolution[0]*resolution[1]*resolution[2] */
    const uint32_t* cells;           /* num_cells * {begin, end}   (stage3.zig:131-134) */
    uint32_t num_triangles;          /* baked refs: cell order, duplicated (stage2.zig:137-164) */
    const float* triangles_pos;      /* num_triangles * 9: v0, e1 = v1-v0, e2 = v2-v0 (linalg.zig:683-694) */
    const float* triangles_data;     /* num_triangles * 15: normal[3] x3, texcoord[2] x3 (stage3.zig:44-51) */
    const uint32_t* triangles_material; /* num_triangles (Data.material_idx) */
    uint32_t num_materials;
    const zrt_material* materials;
    const float* texels;
    uint64_t num_texel_floats;
} zrt_scene;

/* stage3.zig:19-26 Camera (built by stage1.zig:309-371) */
typedef struct zrt_camera {
    uint32_t w, h;
    float origin[3];
    float lower_left_corner[3];
    float right[3];
    float up[3];                     /* points world-down: row 0 is the top image row */
} zrt_camera;

/* main.zig:56-61 Config (num_samples/max_bounce) + device-side knobs that
 * the reference's config.json does not have (kept out of config.json). */
typedef struct zrt_render_config {
    uint32_t num_samples;            /* spp, 1..65535 (u16 in the reference) */
    uint32_t max_bounce;             /* recursion depth of traceRayRecursive */
    uint64_t seed;                   /* counter-RNG key (0 = default) */
    int32_t device;                  /* HIP ordinal, -1 = current device */
    uint32_t rank;                   /* this process's shard of the image */
    uint32_t num_ranks;              /* tiles t with t % num_ranks == rank */
    uint32_t tile_size;              /* square tile edge in pixels, 0 = 64 (32 over several devices) */
    uint32_t flags;                  /* ZRT_FLAG_* */
    uint32_t samples_per_pass;       /* samples of every pixel per device pass, 0 = automatic: as few
                                        passes as 144 GiB of path queues allow, at least two for frames
                                        of 2^23 samples or more (the image is the same for any value) */
    /* zrt_render only (ABI 2, in what were reserved words; zero = `device`
     * alone, one = devices[0] alone): the image's tiles split over
     * num_devices HIP ordinals, tile t
     * rendered on devices[t % num_devices] (repeats allowed), gathered into
     * rgb_out over xGMI -- the multi-device fan-out and join that
     * Scene.render does with its worker threads (stage3.zig:247-256). */
    uint32_t num_devices;
    uint32_t _reserved0;
    const int32_t* devices;
} zrt_render_config;

#define ZRT_FLAG_COUNT_STATS  0x1u   /* count cells/tests/hits (slower kernel variant) */
#define ZRT_FLAG_LANE_WALK    0x2u   /* every launch walks + tests per lane (no park kernel) */
/* 0x4: reserved (a round-2 kernel variant that was measured slower and removed) */
#define ZRT_FLAG_NO_HOP       0x8u   /* the park kernel never hops (wins over ZRT_FLAG_HOP); same image */
#define ZRT_FLAG_ONE_SET      0x10u  /* every pass on the context's one stream (no second pass set, no
                                        lead): kernels never overlap, so their durations are exclusive
                                        (the roofline measurement); same image */
#define ZRT_FLAG_KERNEL_TIMES 0x20u  /* HIP events around every kernel launch: per-kernel device times
                                        in zrt_context_profile (adds ~10 us per launch) */
#define ZRT_FLAG_ESCAPE       0x40u  /* the park walk always uses the escape table (by default only on
                                        scenes where enough of it is set to pay); same image */
#define ZRT_FLAG_NO_ESCAPE    0x80u  /* the park walk never uses the escape table; same image */
#define ZRT_FLAG_FRUSTUM      0x100u /* the primary launch always uses the frustum bounds (by default
                                        only for frames of 2^23 samples or more, where their build pays);
                                        same image */
#define ZRT_FLAG_NO_FRUSTUM   0x200u /* the primary launch never uses the frustum bounds (wins over
                                        ZRT_FLAG_FRUSTUM); same image */
#define ZRT_FLAG_MT_EXACT     0x400u /* every launch walks + tests per lane with the IEEE f32 division in
                                        Moller-Trumbore: what a context does by itself for a scene with
                                        an edge component of 2^62 or more or infinite (the other kernels'
                                        short reciprocal of the determinant holds for |det| < 2^126);
                                        same image */
#define ZRT_FLAG_RELEASE      0x800u /* the park kernel always skips test rounds with too few parked lanes
                                        that have refs to test (by default only on scenes where enough
                                        entry faces of the occupied cells have nothing left to test); same
                                        image */
#define ZRT_FLAG_NO_RELEASE   0x1000u /* never (wins over ZRT_FLAG_RELEASE); same image */
#define ZRT_FLAG_BFCULL       0x2000u /* the park kernel skips, in a segment's first cell, the refs whose
                                        determinant test fails for every direction of the ray's direction
                                        bin (back-face cull masks, built at the first such call if they fit
                                        the memory budget; by default only on scenes whose statistic says
                                        they pay); same image */
#define ZRT_FLAG_NO_BFCULL    0x4000u /* never (wins over ZRT_FLAG_BFCULL); same image */
#define ZRT_FLAG_HOP          0x8000u /* a park-kernel lane that walks on from a parked cell passes through
                                        the next cell without parking there when the parked cell's record
                                        says that a ray arriving from it has no ref left to test in that
                                        cell (hop bits; the default wherever the park kernel runs); same
                                        image */

/* Per-call statistics.  segments = Scene.traceRay calls (primary + bounce +
 * transparency pass-through); Mrays/s = segments / render time. */
typedef struct zrt_stats {
    uint64_t segments;
    uint64_t cells_visited;          /* only with ZRT_FLAG_COUNT_STATS */
    uint64_t triangle_tests;         /* only with ZRT_FLAG_COUNT_STATS */
    uint64_t hits;                   /* only with ZRT_FLAG_COUNT_STATS */
    uint64_t samples;                /* pixels x spp rendered by this call */
    double render_ms;                /* device time: all kernels of the render */
    double trace_kernel_ms;          /* device time: path-trace kernel launches only */
    uint32_t trace_launches;
    uint32_t _pad;
} zrt_stats;

const char* zrt_error_string(int status);
int zrt_abi_version(void);
int zrt_device_count(int* count);
/* Optional: create the device's context and load the library's kernels now
 * (otherwise the first GPU call pays ~0.1-0.2 s), e.g. on a thread while the
 * host loads the scene.  device -1 = 0. */
int zrt_device_warmup(int device);

/* ---- stage 2: grid build + bake (stage2.zig:44-164) --------------------- */
typedef struct zrt_geometry zrt_geometry;

/* positions n*9 (v0,v1,v2 world space), normals n*9, texcoords n*6,
 * material n.  Inputs are read during the call only.  Deterministic:
 * identical to the single-threaded reference order (triangle order within
 * a cell), whatever the host thread count. */
int zrt_geometry_build(const float* positions, const float* normals, const float* texcoords,
                       const uint32_t* material, uint32_t num_triangles,
                       const uint32_t resolution[3], uint32_t num_threads, zrt_geometry** out);
/* The same build on a GPU: SAT binning, cell order and
 * bake as HIP kernels on device `device` (-1 = current).  Output identical
 * to zrt_geometry_build, bit for bit; the result lives in host memory like
 * the host build's.  Replaces Geometry.build + bakeInto (stage2.zig:131-164,
 * called at main.zig:117-118). */
int zrt_geometry_build_device(const float* positions, const float* normals, const float* texcoords,
                              const uint32_t* material, uint32_t num_triangles,
                              const uint32_t resolution[3], int device, zrt_geometry** out);
/* Fills grid/cells/triangle arrays of *scene (views into the geometry,
 * valid until zrt_geometry_free); leaves the material fields untouched. */
int zrt_geometry_scene(const zrt_geometry* g, zrt_scene* scene);
/* Source triangle index of each baked ref (stage2 Geometry.indices). */
int zrt_geometry_indices(const zrt_geometry* g, const uint32_t** indices, uint32_t* count);
void zrt_geometry_free(zrt_geometry* g);

/* ---- stage 3: the render seam ------------------------------------------ */

/* One-shot drop-in for Scene.render: uploads the scene, renders the whole
 * image on `cfg->device` -- or, with cfg->num_devices > 1, on every device of
 * cfg->devices (one host thread and one context per entry, interleaved 32x32
 * tiles by default -- cfg->tile_size overrides -- the packed tiles gathered
 * to the first device over xGMI) -- writes
 * w*h*3 RGB8 into rgb_out (caller-allocated, row 0 = top), frees device
 * memory, returns.  The image is bit-identical for any device list. */
int zrt_render(const zrt_scene* scene, const zrt_camera* camera, const zrt_render_config* cfg,
               uint8_t* rgb_out, zrt_stats* stats);

/* Device-resident path (scene uploaded once, many renders).  A context owns
 * its HIP streams: frames of 2^23 samples or more run their passes on two
 * streams (two pass sets, each with its own queues); zrt_context_render
 * returns once every stream is done, and device_rgb_packed is written on the
 * context's main stream after the join.  One thread at a time per context. */
typedef struct zrt_context zrt_context;

typedef struct zrt_outputs {
    uint8_t* rgb_image;              /* host w*h*3; only this rank's pixels are written */
    uint8_t* rgb_packed;             /* host n_owned*3 in zrt_tile_pixels order */
    float* linear_packed;            /* host n_owned*3: pixel sum * (1/spp), pre-toRGB */
    void* device_rgb_packed;         /* device n_owned*3 on the context's device */
} zrt_outputs;

/* Every finite, infinite or NaN coordinate is taken, as in the reference
 * (linalg.zig:696-722).  A scene with a triangle edge component
 * (scene->triangles_pos e1, e2) of magnitude 2^62 or more or infinite -- a
 * vertex component (positions) of 2^61 or more for the device build --
 * renders through the lane walk with the IEEE division (ZRT_FLAG_MT_EXACT),
 * since the other kernels' short reciprocal of the Moller-Trumbore
 * determinant is exact for |det| < 2^126 only. */
int zrt_context_create(const zrt_scene* scene, int device, zrt_context** out);
/* Geometry.build + bakeInto (stage2.zig:44-164, main.zig:117-118) and the
 * stage-3 upload in one step: the grid is built on `device` straight into the
 * context's HBM arrays (no host copy of the baked scene).  Renders exactly as
 * zrt_geometry_build + zrt_geometry_scene + zrt_context_create. */
int zrt_context_create_built(const float* positions, const float* normals, const float* texcoords,
                             const uint32_t* material, uint32_t num_triangles, const uint32_t resolution[3],
                             uint32_t num_materials, const zrt_material* materials, const float* texels,
                             uint64_t num_texel_floats, int device, zrt_context** out);
int zrt_context_render(zrt_context* ctx, const zrt_camera* camera, const zrt_render_config* cfg,
                       const zrt_outputs* outputs, zrt_stats* stats);
void zrt_context_destroy(zrt_context* ctx);

/* ---- batch ray queries (ABI 2, added) ----------------------------------- */

/* Scene.traceRay (stage3.zig:152-186) for a batch of rays against the
 * context's scene: the grid DDA (linalg.zig:443-496), Moller-Trumbore over the
 * refs of every visited cell in cell order begin -> end, a hit kept when
 * `nearest > t and t > 0` (strict: the first ref among equal t wins), the walk
 * stopped once nearest <= the next crossing -- the function the render kernels
 * implement, bit for bit, without a camera or shading around it. */
typedef struct zrt_hit {
    float t;                         /* nearest t > 0 among the refs the walk tests; +inf: miss */
    float u, v;                      /* barycentrics of that ref (0 on a miss) */
    uint32_t triangle;               /* baked ref: indexes zrt_scene.triangles_pos / triangles_data
                                        (the reference's Hit.triangle_idx); 0xFFFFFFFF on a miss */
} zrt_hit;                           /* 16 B */

#define ZRT_TRACE_PARK 0x10000u      /* zrt_ray_batch.flags only: take the park kernel whatever the batch
                                        size, where the context can run it (else the lane walk, silently).
                                        Unasked, batches of 2^19 rays or more take it and smaller ones the
                                        lane walk (ZRT_FLAG_LANE_WALK: always); incoherent rays are faster
                                        through the park kernel at any size */

typedef struct zrt_ray_batch {
    uint64_t num_rays;
    const float* rays;               /* num_rays * 6: origin xyz, direction xyz.  Any finite direction
                                        with a non-zero component (need not be unit length); for others
                                        (NaN, infinite, all zero) the result is unspecified, the call
                                        still returns */
    zrt_hit* hits;                   /* num_rays */
    uint32_t on_device;              /* 0: host pointers; 1: both are device pointers on the context's
                                        device (4-byte aligned), complete once the call returns */
    uint32_t flags;                  /* ZRT_FLAG_COUNT_STATS | ZRT_FLAG_LANE_WALK | ZRT_FLAG_MT_EXACT |
                                        ZRT_FLAG_ESCAPE / NO_ESCAPE / RELEASE / NO_RELEASE / BFCULL / NO_BFCULL as in a render
                                        (same hits either way) | ZRT_TRACE_PARK; any other bit is
                                        ZRT_ERR_INVALID_ARG */
} zrt_ray_batch;

/* Synchronous; one thread at a time per context, like a render (the two share
 * the context's stream and work buffers, so they may alternate freely).
 * num_rays == 0 returns ZRT_OK and touches nothing; null rays or hits with
 * num_rays > 0 is ZRT_ERR_INVALID_ARG.  Batches of any size: the rays run in
 * chunks of at most 2^20, so no index wraps and the staging memory is bounded.
 * stats (may be null): segments = num_rays, samples = 0, render_ms the device
 * time of the call; cells_visited, triangle_tests and hits with
 * ZRT_FLAG_COUNT_STATS, counted as a counting render counts them. */
int zrt_context_trace(zrt_context* ctx, const zrt_ray_batch* batch, zrt_stats* stats_or_null);

/* ---- segment queries (ABI 2, added) ------------------------------------- */

/* Rays with an end: shadow rays to a light, ambient-occlusion rays of a short
 * radius, line-of-sight tests between two points.  For ray (o, d) with bound
 * t_max this is Scene.traceRay (stage3.zig:152-186) with nearest_hit.t
 * initialised to t_max instead of +inf (stage3.zig:154) and nothing else
 * changed: cells in DDA order, a cell's refs begin -> end, a hit kept when
 * `nearest > t and t > 0`, the walk stopped once nearest <= the next crossing
 * and in any case at the grid's exit.  So
 *   - a ref with t == t_max is NOT kept (the comparison is strict);
 *   - the first cell is always tested, and the walk ends at the first
 *     crossing at or beyond t_max: a short ray walks a few cells, not the grid;
 *   - t_max = +inf is zrt_context_trace, bit for bit;
 *   - t_max <= 0, -inf or NaN is a miss (for NaN no comparison is ever true,
 *     and the walk ends at the grid's exit as every walk does);
 *   - t and t_max are in the ray's own parameter, as zrt_hit.t is; directions
 *     need not be unit length.  A shadow ray written as d = L - P, t_max = 1 is
 *     correct, but such a d leaves the fast kernels' domain (0.5 <= d.d <= 1.5)
 *     and takes the exact, slower walk: a caller who wants the fast kernels
 *     normalises d and passes the distance as t_max.
 * Closest mode: hits[i] is the zrt_hit of that walk; a miss is (+inf, 0, 0,
 * 0xFFFFFFFF) as in zrt_context_trace, whatever t_max was.
 * Any mode (ZRT_SEGMENT_ANY): occluded[i] = 1 if closest mode would report a
 * hit, else 0.  The walk of a ray may end after the first cell in which a hit
 * was kept (until then both modes hold nearest = t_max, visit the same cells
 * and test the same refs; afterwards closest mode can never return to a miss);
 * a counting call's does, the timed kernels run the closest walk, which
 * measured as fast. */
#define ZRT_SEGMENT_ANY 0x40000u     /* zrt_segment_batch.flags only */
typedef struct zrt_segment_batch {
    uint64_t num_rays;
    const float* rays;               /* num_rays * 6, as zrt_ray_batch */
    const float* t_max;              /* num_rays, or null: t_max_all for every ray */
    zrt_hit* hits;                   /* closest mode: num_rays, or null if only `occluded` is wanted */
    uint8_t* occluded;               /* num_rays bytes (0 / 1), or null in closest mode */
    uint32_t on_device;              /* as zrt_ray_batch; applies to all four pointers */
    uint32_t flags;                  /* zrt_ray_batch's flags | ZRT_SEGMENT_ANY */
    float t_max_all;
    uint32_t _reserved;              /* 0 */
} zrt_segment_batch;                 /* 56 B */

/* Synchronous, one thread at a time per context; alternates freely with
 * renders, zrt_context_trace and zrt_context_radiance; chunks of at most 2^20
 * rays (the staging of a host batch grows by the bound and the byte: 5 B per
 * ray), the park kernel as in zrt_context_trace (ZRT_TRACE_PARK,
 * ZRT_FLAG_LANE_WALK), unasked from 2^16 rays.
 * num_rays == 0 returns ZRT_OK and touches nothing.  ZRT_ERR_INVALID_ARG before
 * any device work: a null context or batch, null rays, both outputs null,
 * ZRT_SEGMENT_ANY with non-null hits or null occluded, a non-zero _reserved, a
 * flag zrt_context_trace would refuse.
 * stats (may be null): segments = num_rays, samples = 0, render_ms,
 * trace_kernel_ms and trace_launches as in zrt_context_trace.  hits = the rays
 * not missed: in closest mode with ZRT_FLAG_COUNT_STATS only, in any mode in
 * EVERY call (the bytes give it for free).  cells_visited and triangle_tests
 * with ZRT_FLAG_COUNT_STATS, counted as the walk above runs, any mode's stop
 * after the first cell with a kept hit included. */
int zrt_context_segments(zrt_context* ctx, const zrt_segment_batch* batch, zrt_stats* stats_or_null);

/* ---- radiance queries (ABI 2, added) ------------------------------------ */

/* Scene.traceRayRecursive (stage3.zig:188-220) -- the path tracer itself --
 * for rays the caller chooses: light and irradiance probes, lightmap texels,
 * cameras of the caller's own (panoramic, fisheye, orthographic, thin lens), a
 * handful of pixels again.  For ray i (o_i, d_i) of the batch and sample s in
 * [0, num_samples):
 *   direction  what Camera.getRay (stage3.zig:27-35) computes for the camera
 *              origin = o_i, lower_left_corner = d_i, right = up = 0: +0 added
 *              to every component of d_i twice (so -0 becomes +0), then the
 *              camera's normalisation; the origin is o_i;
 *   RNG        the stream of (seed, pixel (uint32_t)(index_base + i), sample s)
 *              with its first two floats drawn and dropped (the jitter draws);
 *   path       traceRayRecursive(ray, max_bounce) as a render traces a sample;
 *   result     radiance[i] = (the samples' radiances summed in sample order)
 *              * (1 / num_samples), a render's linear_packed value, and
 *              rgb[i] = toRGB(radiance[i]).
 * So radiance[i] is, bit for bit, pixel 0 of a 1x1 zrt_context_render with
 * that camera and seed if that pixel's index were index_base + i.  The first
 * segment of a ray's num_samples paths is one Scene.traceRay call: it is
 * traced once per ray and shaded once per sample. */
#define ZRT_RADIANCE_PER_SAMPLE 0x20000u  /* zrt_radiance_batch.flags only: trace the first segment once per
                                             sample instead of once per ray (same result; the A/B baseline) */
typedef struct zrt_radiance_batch {
    uint64_t num_rays;
    const float* rays;               /* num_rays * 6: origin xyz, direction xyz.  Any finite direction whose
                                        squared length neither overflows nor vanishes; for others (NaN,
                                        infinite, all zero) the result is unspecified, the call still returns */
    float* radiance;                 /* num_rays * 3, linear */
    uint8_t* rgb;                    /* num_rays * 3, or null */
    uint32_t on_device;              /* 0: host pointers; 1: device pointers on the context's device (rays and
                                        radiance 4-byte aligned), complete once the call returns */
    uint32_t flags;                  /* ZRT_FLAG_LANE_WALK | ZRT_FLAG_MT_EXACT | ZRT_FLAG_ESCAPE / NO_ESCAPE /
                                        RELEASE / NO_RELEASE / BFCULL / NO_BFCULL as in a render |
                                        ZRT_TRACE_PARK (the first segment's kernel, as in zrt_context_trace) |
                                        ZRT_RADIANCE_PER_SAMPLE; any other bit is ZRT_ERR_INVALID_ARG */
    uint32_t num_samples;            /* 1..65535 */
    uint32_t max_bounce;             /* 0..32 (0: every radiance is +0); above: ZRT_ERR_UNSUPPORTED, as a render */
    uint64_t seed;
    uint64_t index_base;             /* stream key of ray 0; keys wrap at 2^32 */
} zrt_radiance_batch;                /* 64 B */

/* Synchronous; one thread at a time per context.  It shares the context's
 * stream and work buffers with renders and zrt_context_trace and may
 * alternate freely with them (every use writes what it reads first).
 * num_rays == 0 returns ZRT_OK and touches nothing; null rays or radiance with
 * num_rays > 0, a bad flag (ZRT_FLAG_COUNT_STATS included) or num_samples
 * outside 1..65535 is ZRT_ERR_INVALID_ARG before any device work.  Batches of
 * any size: the rays run in chunks of at most 2^20, fewer where num_samples
 * paths per ray would not fit the memory budget of a render's pass.
 * stats (may be null): segments = the Scene.traceRay calls of these paths as
 * the reference makes them (a shared first segment counts num_samples times;
 * the same number in both modes), samples = num_rays * num_samples, render_ms
 * the device time of the call, trace_kernel_ms and trace_launches as in
 * zrt_context_trace. */
int zrt_context_radiance(zrt_context* ctx, const zrt_radiance_batch* batch, zrt_stats* stats_or_null);

/* ---- surface queries (ABI 2, added) ------------------------------------- */

/* What is at a ray's first hit: the shading inputs traceRayRecursive computes
 * between stage3.zig:199 and :206 -- the interpolated normal and texture
 * coordinate, the material, and its base colour, emission and transparency
 * sampled there -- and the origin it continues from (stage3.zig:209 / :216).
 * G-buffer planes, the hit points of a direct-light pass (shadow rays through
 * zrt_context_segments), lightmap and probe baking, picking.  For ray i:
 *   hits[i]      zrt_context_trace's record of the ray, bit for bit;
 *   surfaces[i]  from that record's (t, u, v, ref), in the reference's
 *                operation order: left to right, nothing contracted, the third
 *                weight 1 - u - v as (1 - u) - v.
 * Directions are taken as given, as in zrt_context_trace, and position is in
 * the ray's own parameter.  A NaN or inf the arithmetic produces is stored as
 * it is.  A miss stores fifteen zero words and material = 0xFFFFFFFF: the sky
 * colour is the caller's (getEnvColor presumes a unit direction, this call
 * does not).  A transparent hit is reported like any other: whether a path
 * passes through it is a random draw of the path tracer's. */
typedef struct zrt_surface {
    float position[3];               /* ray.at(t + floatEps(f32)): o + d * (t + eps), stage3.zig:209/216 --
                                        the origin the reference continues from, ready for shadow / AO rays */
    uint32_t material;               /* Data.material_idx of the hit ref; 0xFFFFFFFF on a miss */
    float normal[3];                 /* interpolate("normal", u, v), stage3.zig:59; NOT normalised, as there */
    float transparency;              /* material.transparency.sample(texcoord) */
    float base_color[3];             /* material.base_color.sample(texcoord) */
    float texcoord_s;                /* interpolate("texcoord", u, v)[0], stage3.zig:63 */
    float emissive[3];               /* material.emissive.sample(texcoord) */
    float texcoord_t;                /* ...[1], stage3.zig:64 */
} zrt_surface;                       /* 64 B */

typedef struct zrt_surface_batch {
    uint64_t num_rays;
    const float* rays;               /* num_rays * 6, as zrt_ray_batch */
    zrt_surface* surfaces;           /* num_rays; on_device: 16-byte aligned, else ZRT_ERR_INVALID_ARG */
    zrt_hit* hits;                   /* num_rays, or null */
    uint32_t on_device;              /* as zrt_ray_batch; applies to all three pointers */
    uint32_t flags;                  /* exactly zrt_ray_batch's flags */
} zrt_surface_batch;                 /* 40 B */

/* Synchronous, one thread at a time per context; alternates freely with
 * renders and the three other queries (every use writes what it reads first).
 * The rays are traced as zrt_context_trace traces them -- the same kernels
 * under the same thresholds and flags -- and one gather launch per chunk of at
 * most 2^20 rays fills the records (the staging of a host batch grows by the
 * 64-byte record; a device batch with null hits keeps its hit records in the
 * context, 16 B per ray).
 * num_rays == 0 returns ZRT_OK and touches nothing.  ZRT_ERR_INVALID_ARG before
 * any device work: a null context or batch, null rays or surfaces, a flag
 * zrt_context_trace would refuse, on_device > 1, a device `surfaces` pointer
 * that is not 16-byte aligned.
 * stats (may be null): as zrt_context_trace (segments = num_rays, samples = 0;
 * cells_visited, triangle_tests and hits with ZRT_FLAG_COUNT_STATS);
 * trace_launches counts the gather launch too. */
int zrt_context_surface(zrt_context* ctx, const zrt_surface_batch* batch, zrt_stats* stats_or_null);

/* ---- transmittance queries (ABI 2, added) ------------------------------- */

/* Shadow rays that pass through transparent hits as the path tracer does.  At
 * a hit traceRayRecursive draws U and continues straight from ray.at(t + eps)
 * when U > transparency (stage3.zig:207-212; the field holds the alpha, 1 is
 * opaque).  This call returns the expected value of that chain along a bounded
 * ray: the product of the pass probabilities of every surface the path tracer
 * would meet on the way -- deterministic, no draw.  For ray (o, d), bound
 * t_max and cap max_crossings, in f32, nothing contracted, in this order:
 *   T = 1; n = 0; o_0 = o; b_0 = t_max
 *   loop k = 0, 1, ...:
 *       h = the closest-mode zrt_context_segments result of (o_k, d, b_k)
 *       if h is a miss: stop
 *       a = zrt_surface.transparency of (o_k, d, h)
 *       n = n + 1
 *       p = 1.0f - a
 *       if !(p > 0): T = +0; stop        -- opaque, or a NaN alpha (`!(U > NaN)`
 *                                           scatters in the path tracer too)
 *       T = T * min(p, 1.0f)
 *       if n == max_crossings: stop      -- the product so far stands
 *       s = h.t + floatEps(f32)
 *       o_{k+1} = o_k + d * s            -- zrt_surface.position
 *       b_{k+1} = b_k - s                -- +inf stays +inf; <= 0: the next
 *                                           segment is a miss
 * transmittance[i] = T, crossings[i] = n.  Directions are taken as given, as in
 * zrt_context_trace; t_max is in the ray's own parameter, per ray or t_max_all
 * when the pointer is null; +inf, <= 0 and NaN behave as in
 * zrt_context_segments (NaN or <= 0: T = 1, n = 0).  The cap is part of the
 * contract, not a safety net: at large coordinates o + d * s can round back to
 * o and the same surface is hit again; the path tracer is bounded by max_bounce
 * there, this call by max_crossings, and crossings[i] == max_crossings tells
 * the caller that the chain was cut. */
typedef struct zrt_transmittance_batch {
    uint64_t num_rays;
    const float* rays;               /* num_rays * 6, as zrt_ray_batch */
    const float* t_max;              /* num_rays, or null: t_max_all for every ray */
    float* transmittance;            /* num_rays */
    uint32_t* crossings;             /* num_rays (n above), or null */
    uint32_t on_device;              /* as zrt_ray_batch; applies to all four pointers */
    uint32_t flags;                  /* exactly zrt_ray_batch's flags */
    float t_max_all;
    uint32_t max_crossings;          /* 1..256 */
} zrt_transmittance_batch;           /* 56 B */

/* Synchronous, one thread at a time per context; alternates freely with
 * renders and the four other queries (every use writes what it reads first);
 * chunks of at most 2^20 rays.  The lane walk traces a ray's whole chain in one
 * launch, and is what every batch takes unasked: it measured as fast or faster
 * at 2^16 and 2^20 rays.  The park path (ZRT_TRACE_PARK only)
 * runs one park launch and one step launch per crossing round over the rays
 * still under way, at most max_crossings rounds, and hands a small remainder
 * to one lane launch.
 * num_rays == 0 returns ZRT_OK and touches nothing.  ZRT_ERR_INVALID_ARG before
 * any device work: a null context or batch, null rays or transmittance, a flag
 * zrt_context_trace would refuse, on_device > 1, max_crossings 0 or above 256.
 * stats (may be null), in every call: segments = the Scene.traceRay calls the
 * loop above makes, hits = the sum of n, samples = 0, render_ms,
 * trace_kernel_ms and trace_launches as in zrt_context_trace.  With
 * ZRT_FLAG_COUNT_STATS cells_visited and triangle_tests, summed over those
 * segments, each counted as a closest-mode counting zrt_context_segments call
 * counts it. */
int zrt_context_transmittance(zrt_context* ctx, const zrt_transmittance_batch* batch, zrt_stats* stats_or_null);

/* ---- feature planes (ABI 2, added) -------------------------------------- */

/* The auxiliary planes of a frame: base colour, normal, emission, depth and
 * transparency of the first hit and the hit count, per pixel, averaged over
 * exactly the jittered camera samples a zrt_context_render of the same camera,
 * seed and sample count traces -- what a denoiser or a compositor reads beside
 * the beauty image.  The camera rays are made on the device (their jitter is
 * the library's own RNG stream), so nothing per ray crosses the bus.
 *
 * All planes are packed in zrt_tile_pixels(w, h, tile_size, rank, num_ranks)
 * order, n_owned that call's count, as zrt_outputs.linear_packed is.
 *
 * For an owned pixel with image index `pixel` = (px, py) and for
 * s = 0 .. num_samples - 1 in this order:
 *   ray_s  the ray a zrt_context_render of the same camera, seed and pixel
 *          traces for sample s: origin camera.origin, direction
 *          normalize(llc + right * ((float)px + U0) + up * ((float)py + U1))
 *          (Camera.getRay, stage3.zig:27-35, :238), U0 and U1 the first two
 *          floats of the stream (seed, pixel, s), normalised as the render
 *          does: scaled by 1.0f / sqrt((x*x + y*y) + z*z);
 *   h_s    the zrt_context_trace record of ray_s;
 *   r_s    the zrt_surface of (ray_s, h_s).
 * Five f32 sums and one counter start at +0 and 0.  A miss adds nothing.  A hit
 * adds r_s.base_color, r_s.normal and r_s.emissive, component by component;
 * h_s.t to the depth sum (the direction is unit length, so t is the distance
 * from the camera); r_s.transparency; and 1 to hits.  The normal is added as
 * interpolated, not normalised: that is what stage3.zig:214 uses.  Each float
 * plane stores sum * (1.0f / (float)num_samples), the render's own
 * inv_num_samples rule (stage3.zig:223, :242); hits stores the count.  A NaN or
 * inf the arithmetic produces is stored as it is.  A transparent first hit
 * counts like any other hit.  No sky colour on a miss: hits / num_samples is the
 * pixel's coverage, the sky is the caller's. */
typedef struct zrt_feature_outputs {
    float* base_color;       /* n_owned * 3, or null */
    float* normal;           /* n_owned * 3, or null */
    float* emissive;         /* n_owned * 3, or null */
    float* depth;            /* n_owned, or null */
    float* transparency;     /* n_owned, or null */
    uint32_t* hits;          /* n_owned, or null */
    uint32_t on_device;      /* 0: host pointers; 1: device pointers on the context's device, 4-byte aligned */
    uint32_t _reserved;      /* 0 */
} zrt_feature_outputs;       /* 56 B */

/* cfg: seed, num_samples (1..65535), rank, num_ranks, tile_size and
 * samples_per_pass mean what they mean in zrt_context_render; max_bounce,
 * device, num_devices and devices are ignored.  cfg->flags accepts what a
 * render accepts: the flags of the bounce launches (ESCAPE, RELEASE, BFCULL,
 * HOP, their NO_ forms, ONE_SET, KERNEL_TIMES) do nothing here;
 * ZRT_FLAG_MT_EXACT, ZRT_FLAG_LANE_WALK and ZRT_FLAG_FRUSTUM /
 * ZRT_FLAG_NO_FRUSTUM select kernels as they do for a render's primary launch
 * (the planes are the same either way); ZRT_FLAG_COUNT_STATS selects the
 * counting instantiation.  The planes are the same bits for any
 * samples_per_pass; unasked, a pass takes as many samples as 4 GiB of item
 * records (48 B per sample) hold, below 2^31 items.
 * Synchronous, one thread at a time per context; alternates freely with
 * renders and the five queries (every use writes what it reads first) and
 * leaves zrt_context_profile's record of the last render untouched.
 * ZRT_ERR_INVALID_ARG before any device work, the outputs untouched: a null
 * context, camera, cfg or outputs, all six plane pointers null, on_device > 1,
 * a non-zero _reserved, num_samples outside 1..65535, and whatever camera, rank
 * or tile value zrt_context_render refuses.  A rank that owns no pixel returns
 * ZRT_OK and touches nothing.
 * stats (may be null), in every call: segments = samples = n_owned *
 * num_samples, hits = the sum of the hits plane, render_ms, trace_kernel_ms
 * and trace_launches as in zrt_context_trace (the launches: the frustum bounds
 * if used, then a walk and a resolve per pass).  With ZRT_FLAG_COUNT_STATS
 * cells_visited and triangle_tests too: a counting render's at max_bounce = 1,
 * which traces exactly these segments. */
int zrt_context_features(zrt_context* ctx, const zrt_camera* camera, const zrt_render_config* cfg,
                         const zrt_feature_outputs* out, zrt_stats* stats_or_null);

/* ---- occlusion queries (ABI 2, added) ----------------------------------- */

/* Hemisphere visibility at each ray's first hit: ambient occlusion, baking,
 * probe lighting.  The sample directions are the ones the path tracer scatters
 * along (stage3.zig:214, normalize(normal + randomUnitVector)) and come from
 * the library's own RNG stream, made on the device: nothing per sample crosses
 * the bus.  Everything is f32, nothing contracted.  For ray i:
 *   h = the zrt_context_trace record of ray i (stored to hits[i] if asked)
 *   r = the zrt_surface of (ray i, h)
 *   a miss: occluded[i] = 0
 *   a hit, for s = 0 .. num_samples - 1:
 *     (a, b, c) = the first three floatNorm draws of the stream
 *                 (seed, (uint32_t)(index_base + i), s), from the stream's
 *                 start, nothing dropped: Vec3.randomUnitVector,
 *                 linalg.zig:140-148
 *     d_s = normalize(r.normal + normalize((a, b, c))), where normalize(x) is
 *           x * (1.0f / sqrt((x.x*x.x + x.y*x.y) + x.z*x.z)) with the correctly
 *           rounded reciprocal, the render's own form; r.normal is used as
 *           interpolated, not normalised, as the reference does
 *     sample s is traced iff every component of r.position and of d_s is
 *           finite and d_s is not all zero (a huge normal makes the squared
 *           length overflow and the direction +0; a NaN or infinite normal
 *           makes it NaN); a sample that is not traced counts as unoccluded
 *     a traced sample is occluded iff the closest-mode zrt_context_segments
 *           result of (r.position, d_s, radius_i) is a hit: the radius follows
 *           the t_max rules as they stand -- strict at equality, +inf is open
 *           sky, <= 0, -inf or NaN is never occluded
 *   occluded[i]   = the number of occluded samples
 *   visibility[i] = (float)(num_samples - occluded[i]) / (float)num_samples, by
 *                   the IEEE division: a miss or a fully open point is exactly
 *                   1.0f (x * (1 / S) is not, for every S)
 * For a unit normal the plain average of these samples is the cosine-weighted
 * visibility: normal + a uniform unit vector, normalised, is cosine-distributed
 * about the normal. */
typedef struct zrt_occlusion_batch {
    uint64_t num_rays;
    const float* rays;        /* num_rays * 6, as zrt_ray_batch */
    const float* radius;      /* num_rays, or null: radius_all for every ray */
    float* visibility;        /* num_rays, or null */
    uint32_t* occluded;       /* num_rays, or null (visibility and occluded not both null) */
    zrt_hit* hits;            /* num_rays, or null: the first hits, as zrt_context_trace */
    uint32_t on_device;       /* as zrt_ray_batch; applies to all five pointers */
    uint32_t flags;           /* exactly zrt_ray_batch's flags */
    float radius_all;
    uint32_t num_samples;     /* 1..65535 */
    uint64_t seed;
    uint64_t index_base;      /* stream key of ray 0; keys wrap at 2^32, as zrt_radiance_batch */
} zrt_occlusion_batch;        /* 80 B */

/* Synchronous, one thread at a time per context; alternates freely with
 * renders and the other queries (every use writes what it reads first) and
 * leaves zrt_context_profile's record untouched.  The first hits are traced as
 * zrt_context_trace traces them, in chunks of at most 2^20 rays; a chunk's
 * (ray, sample) items run in sub-chunks of at most 2^20 items, made on the
 * device.  Items that cannot be occluded -- those of a ray that missed, samples
 * that are not traced -- are never walked.  The samples take the lane walk or,
 * from 2^16 items in the batch or with ZRT_TRACE_PARK, the park kernel in its
 * bounded closest mode; the answer is the same.
 * num_rays == 0 returns ZRT_OK and touches nothing.  ZRT_ERR_INVALID_ARG before
 * any device work, the outputs untouched: a null context or batch, null rays,
 * visibility and occluded both null, a flag zrt_context_trace would refuse,
 * on_device > 1, num_samples outside 1..65535.
 * stats (may be null), in every call: segments = num_rays + the traced samples,
 * hits = the sum of occluded, samples = 0, render_ms, trace_kernel_ms and
 * trace_launches as in zrt_context_trace.  With ZRT_FLAG_COUNT_STATS
 * cells_visited and triangle_tests: the sum of a counting zrt_context_trace
 * call over the rays and a counting ZRT_SEGMENT_ANY zrt_context_segments call
 * over exactly the traced samples; samples that are not traced add nothing. */
int zrt_context_occlusion(zrt_context* ctx, const zrt_occlusion_batch* batch, zrt_stats* stats_or_null);

/* ---- direct-light queries (ABI 2, added) -------------------------------- */

/* The light of punctual lights at each ray's first hit, shadowed through
 * transparent hits as the path tracer sees them: what zrt_context_surface and
 * zrt_context_transmittance were added for, assembled.  The reference scene has
 * no punctual lights -- only emissive surfaces and the sky -- so the lights are
 * the caller's, a small host array per call.  The shadow rays are made, culled,
 * traced and summed on the device: nothing per (ray, light) item crosses the
 * bus, and the sum's order is fixed.
 * Everything is f32, nothing is contracted (no FMA), operations run left to
 * right as written.  dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z; length(a) is
 * the IEEE sqrt of dot(a, a); normalize_rn(a) = a * (1.0f / length(a)) with the
 * correctly rounded reciprocal, the render's own form.  For ray i:
 *   h = the zrt_context_trace record of ray i (stored to hits[i] if asked)
 *   r = the zrt_surface of (ray i, h)
 *   a miss: irradiance[i] and radiance[i] are three +0
 *   a hit: N = normalize_rn(r.normal).  The ray is shaded iff every component
 *     of r.position and of N is finite (a zero, NaN or infinite interpolated
 *     normal makes N NaN: not shaded); a ray that is not shaded has no traced
 *     item and E = +0.  A huge normal, whose squared length overflows, makes
 *     N = (+0, +0, +0): c = 0 for every light, so it has no traced item and
 *     E = +0 just the same
 *   E = (+0, +0, +0); for l = 0 .. num_lights - 1, in this order:
 *     POINT, SPOT:  v = light.position - r.position;  d2 = dot(v, v)
 *                   w = normalize_rn(v);  b = length(v)
 *     DIRECTIONAL:  w = normalize_rn((-dir.x, -dir.y, -dir.z));  b = +inf
 *     c = dot(N, w).  The item is traced iff c > 0, and for a SPOT also iff
 *         k > 0 (below).  That one test skips a light behind the surface, a
 *         light at the hit point (w is NaN) and a light at overflow distance
 *         (w is 0)
 *     f = c / d2 by the IEEE division (POINT, SPOT);  f = c (DIRECTIONAL)
 *     SPOT:  s = -dot(normalize_rn(light.direction), w)
 *            k = fminf(fmaxf(s * angle_scale + angle_offset, 0.0f), 1.0f) --
 *                two roundings; a NaN becomes 0
 *            f = f * (k * k)
 *     T = the zrt_context_transmittance result of (r.position, w, b,
 *         max_crossings), its rules as they stand: strict at t == b, and the
 *         cap is part of the contract.  With ZRT_DIRECT_UNSHADOWED T = 1 and no
 *         segment is traced
 *     g = f * T;  E.k = E.k + light.color[k] * g for k = 0, 1, 2
 *     an item that is not traced adds nothing
 *   irradiance[i] = E
 *   radiance[i].k = r.emissive[k] + (r.base_color[k] * E.k) * 0x1.45f306p-2f --
 *     1 / pi rounded to f32, bits 0x3EA2F983: the Lambertian surface the path
 *     tracer's diffuse branch stands for.  A transparent first hit is shaded
 *     like any other, as in zrt_context_surface.  For a hit that is not shaded
 *     radiance is r.emissive.  A NaN or inf the arithmetic produces is stored
 *     as it is.
 * Non-finite light fields are taken as given; the arithmetic above decides. */
enum { ZRT_LIGHT_POINT = 0, ZRT_LIGHT_DIRECTIONAL = 1, ZRT_LIGHT_SPOT = 2 };
typedef struct zrt_light {
    uint32_t type;
    float position[3];        /* POINT, SPOT */
    float direction[3];       /* DIRECTIONAL, SPOT: the way the light travels; any length */
    float color[3];           /* POINT / SPOT: intensity (W/sr, linear RGB); DIRECTIONAL: irradiance on a
                                 facing surface */
    float angle_scale;        /* SPOT: 1 / max(0.001, cos_inner - cos_outer) ... */
    float angle_offset;       /* ... and -cos_outer * angle_scale (the caller computes them) */
} zrt_light;                  /* 48 B */

#define ZRT_DIRECT_UNSHADOWED 0x80000u   /* zrt_direct_batch.flags only: T = 1 for every traced item, no
                                            shadow segment */

typedef struct zrt_direct_batch {
    uint64_t num_rays;
    const float* rays;        /* num_rays * 6, as zrt_ray_batch */
    const zrt_light* lights;  /* num_lights, ALWAYS a host pointer (copied per call) */
    float* irradiance;        /* num_rays * 3, or null */
    float* radiance;          /* num_rays * 3, or null (irradiance and radiance not both null) */
    zrt_hit* hits;            /* num_rays, or null: the first hits, as zrt_context_trace */
    uint32_t on_device;       /* as zrt_ray_batch; applies to rays, irradiance, radiance, hits */
    uint32_t flags;           /* zrt_ray_batch's flags | ZRT_DIRECT_UNSHADOWED */
    uint32_t num_lights;      /* 1..65535 */
    uint32_t max_crossings;   /* 1..256, as zrt_transmittance_batch */
} zrt_direct_batch;           /* 64 B */

/* Synchronous, one thread at a time per context; alternates freely with
 * renders and the other queries (every use writes what it reads first) and
 * leaves zrt_context_profile's record untouched.  The first hits are traced as
 * zrt_context_trace traces them, in chunks of at most 2^20 rays, under the
 * trace call's own thresholds; ZRT_TRACE_PARK and the escape, release and cull
 * flags govern the first hits only.  A chunk's (ray, light) items run in
 * sub-chunks of at most 2^20 items, made on the device; a ray's lights may
 * straddle a cut, and its sum still adds in light order.  Items that are not
 * traced are never walked.  The chains take the transmittance call's lane walk
 * -- a ray's whole chain in one launch -- at every size: the park-and-step
 * rounds measured no faster for chains and are not built for
 * the items.
 * num_rays == 0 returns ZRT_OK and touches nothing.  ZRT_ERR_INVALID_ARG before
 * any device work, the outputs untouched: a null context or batch, null rays or
 * lights, irradiance and radiance both null, num_lights 0 or above 65535, a
 * light type above 2, max_crossings 0 or above 256, on_device > 1, a flag
 * zrt_context_trace would refuse.
 * stats (may be null), in every call: segments = num_rays + the Scene.traceRay
 * calls of all chains, samples = the traced items, hits = the sum of the
 * chains' crossings, render_ms, trace_kernel_ms and trace_launches as in
 * zrt_context_trace.  With ZRT_FLAG_COUNT_STATS cells_visited and
 * triangle_tests: the sum of a counting zrt_context_trace call over the rays
 * and a counting zrt_context_transmittance call over exactly the traced items;
 * items that are not traced add nothing. */
int zrt_context_direct(zrt_context* ctx, const zrt_direct_batch* batch, zrt_stats* stats_or_null);

/* ---- area-light queries (ABI 2, added) ---------------------------------- */

/* Direct light from the scene's own lights: its emissive triangles, sampled by
 * next-event estimation and shadowed through transparent hits as the path
 * tracer sees them.  Two pieces: an emitter set, built once on the device from
 * the caller's source triangles and the context's materials, and the call,
 * zrt_context_direct's sibling.  Nothing per (ray, sample) item crosses the
 * bus, and both are specified bit for bit.
 *
 * The emitter set.  The input is the caller's source triangle soup, the arrays
 * zrt_context_create_built takes, as HOST pointers: positions n * 9 floats
 * (v0, v1, v2), texcoords n * 6 floats or null for zeros, material n entries
 * indexing the context's materials (an index at or above their number is
 * ZRT_ERR_INVALID_ARG).  It is NOT the context's baked refs: those are
 * duplicated per grid cell and carry no source id.  A triangle that appears
 * twice in the soup counts as two lights.  Everything below runs on the device
 * from the context's own material table and texel pool, in f32, nothing
 * contracted, left to right:
 *   per material  m = the fmaxf fold, starting from +0, over every component of
 *                 every texel of its emissive texture (a maximum is order-free;
 *                 NaN and negative texels fall away, +inf stays)
 *   per triangle  e1 = v1 - v0;  e2 = v2 - v0;  n = cross(e1, e2) (linalg.zig:173)
 *                 a = 0.5f * length(n);  w = a * m
 *                 an emitter iff w > 0 and w is finite
 * Emitters keep source-triangle order.  Over them:
 *   wmax = the maximum w
 *   q_k  = max(1, (uint32_t)((w_k / wmax) * 0x1p24f)) -- the IEEE division, the
 *          conversion truncating
 *   C_k  = the exclusive prefix sum of q as uint64_t;  Q = their total
 * The distribution is made of integers on purpose: integer sums are
 * associative, so the device's parallel scans agree with a serial sum bit for
 * bit.  More than 2^28 emitters is ZRT_ERR_UNSUPPORTED: Q stays below 2^52 and
 * (float)Q has one rounding however it is computed.  A set with zero emitters
 * is valid (Q = 0). */
typedef struct zrt_emitters zrt_emitters;
typedef struct zrt_emitter {
    float v0[3];              /* the source triangle's first vertex */
    float a;                  /* its area, as above */
    float e1[3];
    uint32_t q;
    float e2[3];
    uint32_t material;
    float texcoords[6];       /* of v0, v1, v2 */
    uint32_t triangle;        /* index into the caller's soup */
    uint32_t _reserved;       /* 0 */
} zrt_emitter;                /* 80 B */

/* Synchronous, on the context's stream, one thread at a time per context.  The
 * set belongs to the context it was made on and must be destroyed before it;
 * it holds no reference to the caller's arrays and is not changed by renders
 * or queries.  ZRT_ERR_INVALID_ARG before any device work: a null context, out
 * or material, null positions with num_triangles > 0, a material index out of
 * range.  num_triangles == 0 gives the empty set. */
int zrt_emitters_create(zrt_context* ctx, const float* positions, const float* texcoords, const uint32_t* material,
                        uint32_t num_triangles, zrt_emitters** out);
/* Any of the three outputs may be null. */
int zrt_emitters_info(const zrt_emitters* set, uint32_t* num_emitters, uint64_t* total_q, uint32_t* num_triangles);
/* records: num_emitters zrt_emitter, prefix: num_emitters uint64_t (C); host
 * pointers, either may be null. */
int zrt_emitters_read(const zrt_emitters* set, zrt_emitter* records, uint64_t* prefix);
void zrt_emitters_destroy(zrt_emitters* set);

/* The call.  dot, length and normalize_rn as in zrt_context_direct; all
 * arithmetic f32, nothing contracted, left to right.  For ray i:
 *   h = the zrt_context_trace record of ray i (stored to hits[i] if asked)
 *   r = the zrt_surface of (ray i, h)
 *   a miss: irradiance[i] and radiance[i] are three +0
 *   a hit: N = normalize_rn(r.normal); the ray is shaded iff every component of
 *     r.position and of N is finite, as in zrt_context_direct; a ray that is
 *     not shaded has no traced item, E = +0 and radiance = r.emissive
 *   E = (+0, +0, +0); for s = 0 .. num_samples - 1, in this order:
 *     x0, x1, x2 = the first three raw 64-bit outputs of the stream (seed,
 *       (uint32_t)(index_base + i), s) -- the render's SplitMix64 stream, whole
 *       words, so that no float draw's word count enters
 *     rsel = the high 64 bits of the 128-bit product x0 * Q
 *     k = the emitter with C_k <= rsel < C_k + q_k
 *     bu = (float)(x1 >> 40) * 0x1p-24f;  bv = (float)(x2 >> 40) * 0x1p-24f
 *     if bu + bv > 1: bu = 1 - bu; bv = 1 - bv            (the fold: no square root)
 *     y = (v0 + e1 * bu) + e2 * bv
 *     texcoord = zrt_surface's interpolation with (u, v) = (bu, bv): weights
 *       w0 = (1 - bu) - bv, (tc0 * w0 + tc1 * bu) + tc2 * bv per component
 *     Le, alpha = the emitter's material's emissive and transparency textures
 *       sampled there.  The path tracer scatters off a surface -- and so sees
 *       its emission -- when `U > transparency` fails (stage3.zig:207): an
 *       emitter shows alpha * Le, the rest passes through
 *     v = y - r.position;  d2 = dot(v, v);  wdir = normalize_rn(v)
 *     c = dot(N, wdir);  cl = -dot(normalize_rn(cross(e1, e2)), wdir) --
 *       emitters are one-sided: the reference culls back faces
 *     the item is traced iff c > 0 and cl > 0 (a NaN fails both)
 *     g = ((c * cl) / d2) * (((float)Q / (float)q_k) * a_k)
 *     T = the zrt_context_transmittance result of (r.position, wdir, b,
 *       max_crossings) with b = length(v) * 0x1.ff8p-1f (1 - 2^-10).  The
 *       emitter itself lies at t ~ length(v) and a traced item always faces its
 *       front, so an unshortened bound would let rounding decide whether the
 *       lamp shadows itself.  The price: an occluder within 0.1% of the
 *       distance in front of the lamp is not seen.  With ZRT_AREA_UNSHADOWED
 *       T = 1 and nothing is traced
 *     E.j = E.j + ((Le.j * alpha) * g) * T  for j = 0, 1, 2
 *     an item that is not traced adds nothing
 *   irradiance[i].j = E.j / (float)num_samples -- the IEEE division
 *   radiance[i].j = r.emissive[j] + (r.base_color[j] * irradiance[i].j) * 0x1.45f306p-2f
 * A NaN or inf the arithmetic produces is stored as it is.  An empty set
 * stores +0 irradiance (radiance = r.emissive + (base_color * 0) / pi as
 * above) and traces nothing. */
#define ZRT_AREA_UNSHADOWED 0x800000u    /* zrt_area_light_batch.flags only: T = 1 for every traced item, no
                                            shadow segment */

typedef struct zrt_area_light_batch {
    uint64_t num_rays;
    const float* rays;        /* num_rays * 6, as zrt_ray_batch */
    const zrt_emitters* emitters;
    float* irradiance;        /* num_rays * 3, or null */
    float* radiance;          /* num_rays * 3, or null (irradiance and radiance not both null) */
    zrt_hit* hits;            /* num_rays, or null: the first hits, as zrt_context_trace */
    uint32_t on_device;       /* as zrt_ray_batch; applies to rays, irradiance, radiance, hits */
    uint32_t flags;           /* zrt_ray_batch's flags | ZRT_AREA_UNSHADOWED */
    uint32_t num_samples;     /* 1..65535 */
    uint32_t max_crossings;   /* 1..256, as zrt_transmittance_batch */
    uint64_t seed;
    uint64_t index_base;      /* stream key of ray 0; keys wrap at 2^32 */
} zrt_area_light_batch;       /* 80 B */

/* Synchronous, one thread at a time per context; alternates freely with
 * renders and the other queries and leaves zrt_context_profile's record
 * untouched.  First hits, chunks, sub-chunks of at most 2^20 (ray, sample)
 * items (a ray's samples may straddle a cut and still add in sample order) and
 * the chains' lane walk are zrt_context_direct's.
 * num_rays == 0 returns ZRT_OK and touches nothing.  ZRT_ERR_INVALID_ARG before
 * any device work, the outputs untouched: a null context or batch, null rays or
 * emitters, a set made on another context, irradiance and radiance both null,
 * num_samples 0 or above 65535, max_crossings 0 or above 256, on_device > 1, a
 * flag zrt_context_trace would refuse.
 * stats (may be null), in every call: segments = num_rays + the chains'
 * segments, samples = the traced items, hits = the chains' crossings; with
 * ZRT_FLAG_COUNT_STATS cells_visited and triangle_tests: the sum of a counting
 * zrt_context_trace call over the rays and a counting
 * zrt_context_transmittance call over exactly the traced items. */
int zrt_context_area_lights(zrt_context* ctx, const zrt_area_light_batch* batch, zrt_stats* stats_or_null);

/* ---- sky-light queries (ABI 2, added) ------------------------------------ */

/* Direct light from the sky: the environment every path that leaves the grid
 * returns (getEnvColor, stage3.zig:144-150), sampled over the cosine-weighted
 * hemisphere at each ray's first hit and shadowed through transparent hits as
 * the path tracer sees them.  zrt_context_area_lights' sibling: with it,
 * emissive + area lights + sky is, in expectation, the path tracer at
 * max_bounce = 2 on opaque scenes.  Nothing per (ray, sample) item crosses the
 * bus.  dot, length and normalize_rn as in zrt_context_direct; all arithmetic
 * f32, nothing contracted, left to right.  For ray i:
 *   h = the zrt_context_trace record of ray i (stored to hits[i] if asked)
 *   r = the zrt_surface of (ray i, h)
 *   a miss: irradiance[i], radiance[i] and visibility[i] are all +0.  This
 *     visibility is not zrt_context_occlusion's: it is the estimator's weight
 *     sum, and a miss has no estimator
 *   a hit: N = normalize_rn(r.normal); the ray is shaded iff every component of
 *     r.position and of N is finite, as in zrt_context_direct; a ray that is
 *     not shaded has no traced item, irradiance = visibility = +0 and
 *     radiance = r.emissive.  N is normalised here, unlike in
 *     zrt_context_occlusion, on purpose: N + a uniform unit vector, normalised,
 *     is cosine-distributed about N only for a unit N, and the estimator
 *     divides by that density
 *   A = (+0, +0, +0), V = +0; for s = 0 .. num_samples - 1, in this order:
 *     (a, b, c) = the first three floatNorm draws of the stream (seed,
 *       (uint32_t)(index_base + i), s) from its start -- zrt_context_occlusion's
 *       draws
 *     d_s = normalize_rn(N + normalize_rn((a, b, c)))
 *     the item is traced iff every component of d_s is finite and d_s is not
 *       all zero; an item that is not traced adds nothing
 *     L_s = getEnvColor(d_s):  t = 0.5f * (d_s.y + 1.0f);
 *       L_s.k = (1.0f - t) + c_k * t  with c = (0.5f, 0.7f, 1.0f)
 *     T_s = the zrt_context_transmittance result of (r.position, d_s, +inf,
 *       max_crossings), its rules as they stand.  With ZRT_SKY_UNSHADOWED
 *       T_s = 1 and no segment is traced
 *     A.k = A.k + L_s.k * T_s  for k = 0, 1, 2;  V = V + T_s
 *   mean.k = A.k / (float)num_samples;  visibility[i] = V / (float)num_samples
 *     -- the IEEE division
 *   irradiance[i].k = mean.k * 0x1.921fb6p+1f -- pi rounded to f32, bits
 *     0x40490FDB: the density is cos / pi, so E = pi * mean
 *   radiance[i].k = r.emissive[k] + r.base_color[k] * mean.k -- the Lambertian
 *     radiance base_color * E / pi without the round trip through pi
 * A NaN or inf the arithmetic produces is stored as it is. */
#define ZRT_SKY_UNSHADOWED 0x1000000u   /* zrt_sky_light_batch.flags only: T = 1 for every traced item, nothing
                                           traced */

typedef struct zrt_sky_light_batch {
    uint64_t num_rays;
    const float* rays;        /* num_rays * 6, as zrt_ray_batch */
    float* irradiance;        /* num_rays * 3, or null */
    float* radiance;          /* num_rays * 3, or null */
    float* visibility;        /* num_rays, or null (the three not all null) */
    zrt_hit* hits;            /* num_rays, or null: the first hits, as zrt_context_trace */
    uint32_t on_device;       /* as zrt_ray_batch; applies to all six pointers */
    uint32_t flags;           /* zrt_ray_batch's flags | ZRT_SKY_UNSHADOWED */
    uint32_t num_samples;     /* S, 1..65535 */
    uint32_t max_crossings;   /* 1..256, as zrt_transmittance_batch */
    uint64_t seed;
    uint64_t index_base;      /* stream key of ray 0; keys wrap at 2^32 */
} zrt_sky_light_batch;        /* 80 B */

/* Synchronous, one thread at a time per context; alternates freely with
 * renders and the other queries and leaves zrt_context_profile's record
 * untouched.  First hits, chunks of at most 2^20 rays, sub-chunks of at most
 * 2^20 (ray, sample) items made on the device and the chains' lane walk are
 * zrt_context_direct's.  A ray whose samples straddle a cut still adds in
 * sample order, A and V alike, whichever outputs are asked for.
 * num_rays == 0 returns ZRT_OK and touches nothing.  ZRT_ERR_INVALID_ARG before
 * any device work, the outputs untouched: a null context, batch or rays,
 * irradiance, radiance and visibility all null, num_samples 0 or above 65535,
 * max_crossings 0 or above 256, on_device > 1, a flag zrt_context_trace would
 * refuse.
 * stats (may be null), in every call: segments = num_rays + the Scene.traceRay
 * calls of all chains, samples = the traced items, hits = the sum of the
 * chains' crossings, render_ms, trace_kernel_ms and trace_launches as in
 * zrt_context_trace.  With ZRT_FLAG_COUNT_STATS cells_visited and
 * triangle_tests: the sum of a counting zrt_context_trace call over the rays
 * and a counting zrt_context_transmittance call over exactly the traced items. */
int zrt_context_sky_light(zrt_context* ctx, const zrt_sky_light_batch* batch, zrt_stats* stats_or_null);

/* ---- light-probe queries (ABI 2, added) --------------------------------- */

/* The light arriving at a point from all directions: per probe position the
 * order-2 spherical-harmonics projection of the path-traced radiance field,
 * the first-hit distance moments and the hit count -- zrt_context_radiance's
 * first use, with the directions drawn, traced, projected and summed on the
 * device.  Nothing per (probe, direction) item crosses the bus unless the
 * caller asks for the raw directions or radiance, and the sum's order is fixed.
 * Everything is f32, nothing is contracted (no FMA), operations run left to
 * right as written.  normalize_rn(a) = a * (1.0f / sqrt((a.x*a.x + a.y*a.y) +
 * a.z*a.z)) with the IEEE square root and the correctly rounded reciprocal, the
 * render's own form.  For probe p at x_p = positions[p] and direction
 * j = 0 .. D - 1 (D = num_directions), in this order:
 *   key  = (uint32_t)(index_base + p * D + j), the product taken in 64 bits
 *   d_j  = normalize_rn((a, b, c)): a, b, c the first three floatNorm draws of
 *          the stream (seed, key, sample 65535) taken from its start
 *          (Vec3.randomUnitVector, linalg.zig:140-148).  Sample index 65535 is
 *          never a path's: a call's paths use samples 0 .. num_samples - 1 <=
 *          65534 and the stream key gives the sample 16 bits, so the directions
 *          are independent of every path stream under the same seed and key
 *   L_j  = the radiance[i] zrt_context_radiance specifies for the ray (x_p, d_j)
 *          with stream key `key`, num_samples, max_bounce and seed, bit for bit.
 *          That call adds +0 twice to d_j and normalises it again: u_j.  The
 *          first segment is traced once per direction, as there
 *   h_j  = the zrt_context_trace record of (x_p, u_j)
 *   the basis on d_j (not u_j), (x, y, z) = d_j, the constants f32 literals:
 *     C0 = 0x1.20dd76p-2f (0x3E906EBB)   C1 = 0x1.f45438p-2f (0x3EFA2A1C)
 *     C2 = 0x1.17b142p+0f (0x3F8BD8A1)   C3 = 0x1.42f602p-2f (0x3EA17B01)
 *     C4 = 0x1.17b142p-1f (0x3F0BD8A1)
 *     Y0 = C0          Y1 = C1*y        Y2 = C1*z        Y3 = C1*x
 *     Y4 = (C2*x)*y    Y5 = (C2*y)*z    Y6 = C3*((3.0f*(z*z)) - 1.0f)
 *     Y7 = (C2*x)*z    Y8 = C4*((x*x) - (y*y))
 *   the sums, from +0 and 0, in direction order:
 *     A[k][c] = A[k][c] + L_j[c] * Y_k          k = 0..8, c = 0..2
 *     a hit (h_j.t != +inf):  T1 += h_j.t;  T2 += h_j.t * h_j.t;  n += 1
 *     a miss adds nothing to T1, T2 or n
 * and then
 *   sh[p][k][c]  = A[k][c] * w,  w = 0x1.921fb6p+3f / (float)D -- 4 pi rounded
 *                  to f32 (0x41490FDB), by the IEEE division
 *   distance[p]  = (T1 * r, T2 * r),  r = 1.0f / (float)D
 *   hits[p]      = n
 *   directions[p * D + j] = d_j,  radiance[p * D + j] = L_j
 * A NaN or inf the arithmetic produces is stored as it is.  A non-finite
 * position or a NaN direction gives an unspecified result; the call still
 * returns. */
typedef struct zrt_light_probe_batch {
    uint64_t num_probes;
    const float* positions;   /* num_probes * 3 */
    float* sh;                /* num_probes * 27: [k][c], k = 0..8, c = RGB; or null */
    float* distance;          /* num_probes * 2: mean t, mean t*t of the first hits; or null */
    uint32_t* hits;           /* num_probes: directions whose first segment hit; or null */
    float* directions;        /* num_probes * num_directions * 3: d_j as generated; or null */
    float* radiance;          /* num_probes * num_directions * 3: L_j; or null */
    uint32_t on_device;       /* as zrt_ray_batch; applies to positions and all five outputs */
    uint32_t flags;           /* zrt_radiance_batch's flags without ZRT_RADIANCE_PER_SAMPLE */
    uint32_t num_directions;  /* D, 1..65535 */
    uint32_t num_samples;     /* S, 1..65535 paths per direction */
    uint32_t max_bounce;      /* 1..32 */
    uint32_t _reserved;       /* 0 */
    uint64_t seed;
    uint64_t index_base;      /* stream key of probe 0's direction 0; keys wrap at 2^32 */
} zrt_light_probe_batch;      /* 96 B; offsets 0 8 16 24 32 40 48 56 60 64 68 72 76 80 88 */

/* Synchronous, one thread at a time per context; alternates freely with
 * renders and the other queries (every use writes what it reads first) and
 * leaves zrt_context_profile's record untouched.  The (probe, direction) items
 * run through the radiance call's launches in chunks of at most 2^20 items,
 * fewer where num_samples paths per item would not fit the memory budget of a
 * render's pass.  The summation order is part of the contract: a probe's
 * directions may straddle a cut and still add in direction order, so the result
 * is the same bits for any chunking.
 * num_probes == 0 returns ZRT_OK and touches nothing.  ZRT_ERR_INVALID_ARG
 * before any device work, the outputs untouched: a null context or batch, null
 * positions, all five outputs null, on_device > 1, a non-zero _reserved,
 * num_directions or num_samples outside 1..65535, num_probes above 2^47 (the
 * item count num_probes * num_directions stays below 2^63), max_bounce == 0,
 * any flag outside the accepted set (ZRT_RADIANCE_PER_SAMPLE and
 * ZRT_FLAG_COUNT_STATS included).  max_bounce > 32 is ZRT_ERR_UNSUPPORTED, as in the radiance call.
 * stats (may be null), in every call: segments = what a zrt_context_radiance
 * call over the same num_probes * D rays reports, samples = num_probes * D * S,
 * hits = the sum of the hits plane whether or not `hits` was asked for,
 * render_ms, trace_kernel_ms and trace_launches as in zrt_context_trace. */
int zrt_context_light_probes(zrt_context* ctx, const zrt_light_probe_batch* batch, zrt_stats* stats_or_null);

/* ---- films: progressive renders (ABI 2, added) -------------------------- */

/* A film keeps a frame's per-pixel sample sums between calls, so that a frame
 * can be shown after a few samples and refined, rendered until a deadline,
 * stopped and resumed, or given more samples without paying for the first ones
 * again.  It is renderWorker's `pixel` of every pixel (stage3.zig:222-245: the
 * `pixel = pixel.add(...)` chain over the samples, then `inv_num_samples`),
 * stopped after any sample and picked up again.
 *
 * A film is the accumulator of one rank's share of a w x h frame: one f32 RGB
 * sum per pixel of zrt_tile_pixels(w, h, tile_size, rank, num_ranks), in that
 * order, and the number of samples summed so far (0 after create and reset).
 * tile_size 0 = 64, num_ranks 0 = 1, as in zrt_render_config.  It lives on its
 * context's device: destroy it before that context (zrt_film_destroy itself
 * does not touch the context).  zrt_film_create refuses what zrt_tile_pixels
 * refuses and a frame of more than 2^32 - 1 pixels. */
typedef struct zrt_film zrt_film;
int zrt_film_create(zrt_context* ctx, uint32_t w, uint32_t h, uint32_t tile_size, uint32_t rank,
                    uint32_t num_ranks, zrt_film** out);
/* samples = 0.  The sums are not cleared: the next call starts from +0 and
 * never reads them. */
int zrt_film_reset(zrt_film* film);
/* Either pointer may be null. */
int zrt_film_info(const zrt_film* film, uint32_t* n_owned, uint32_t* samples);
/* Checkpoint and resume: host arrays of n_owned * 3 floats, the sums as they
 * are stored (no division), bit for bit.  A film read after s samples and
 * written into another film of the same shape -- of this or another context
 * of the same scene -- continues exactly as the first would have.  Reading an
 * empty film gives +0 everywhere.  zrt_film_write with samples 0 is a reset
 * (sums may be null); samples > 65535 is ZRT_ERR_INVALID_ARG, the film
 * untouched.  Both are synchronous on the context's stream. */
int zrt_film_read(zrt_film* film, float* sums, uint32_t* samples_or_null);
int zrt_film_write(zrt_film* film, const float* sums, uint32_t samples);
void zrt_film_destroy(zrt_film* film);

/* zrt_context_render for the next cfg->num_samples samples of a film.  With
 * b = the film's samples and n = cfg->num_samples, for every owned pixel:
 *   - the call traces the paths of samples b .. b + n - 1: exactly the paths a
 *     zrt_context_render of the same camera, seed and max_bounce traces for
 *     those sample indices, with the stream (seed, pixel, s);
 *   - it adds their radiances to the pixel's sum in sample order
 *     (stage3.zig:236-241), starting from the stored sum, or from +0 when
 *     b == 0 (the stored bits are ignored then);
 *   - it stores the sum and sets the film's samples to b + n;
 *   - the outputs, if asked, are linear = sum * (1.0f / (float)(b + n))
 *     (stage3.zig:223, :242 inv_num_samples) and rgb = toRGB(linear).  All four
 *     zrt_outputs fields mean what they mean in a render; outputs may be null,
 *     and a call that asks for none writes none on the device either.
 * Consequence: after calls with counts n_1 .. n_k and one camera, seed and
 * max_bounce, the outputs of the last call are, bit for bit, those of one
 * zrt_context_render with num_samples = n_1 + .. + n_k -- in every kernel mode
 * (cfg->flags) and for any samples_per_pass in any call, which may differ from
 * call to call.
 * The film stores nothing of the camera: a caller who changes it between calls
 * gets the sum over the cameras (motion blur, lens sampling).  The same holds
 * for seed and max_bounce.
 * cfg: every field and flag means what it means in zrt_context_render,
 * ZRT_FLAG_COUNT_STATS and ZRT_FLAG_KERNEL_TIMES included; num_devices and
 * devices are ignored.  The kernels are chosen from this call's own
 * n_owned * n (the 2^23-sample thresholds of the two pass sets and of the
 * frustum bounds), and the tables a first big render builds are built as there.
 * ZRT_ERR_INVALID_ARG before any device work, film and outputs untouched: a
 * null context, film, camera or cfg; a film of another context; n == 0 or
 * b + n > 65535 (the stream key gives the sample index 16 bits); camera->w or
 * camera->h, cfg->tile_size, cfg->rank or cfg->num_ranks (after their defaults)
 * that differ from the film's; whatever zrt_context_render refuses.
 * max_bounce > 32 is ZRT_ERR_UNSUPPORTED, likewise.  A rank that owns no pixel
 * returns ZRT_OK, and its film's samples still advance.  If a HIP call fails
 * midway the film's contents are unspecified until zrt_film_reset or
 * zrt_film_write.
 * stats (may be null): of this call alone, as a render of n samples reports
 * them -- samples = n_owned * n; segments, and with ZRT_FLAG_COUNT_STATS
 * cells_visited, triangle_tests and hits, those of the paths of samples
 * b .. b + n - 1, so that over a sequence of calls they add up to the one
 * render's.  zrt_context_profile records the call as it records a render.
 * Synchronous, one thread at a time per context; alternates freely with
 * renders, every query and other films of the same context (the sums live in
 * the film, not in the context's buffers). */
int zrt_context_accumulate(zrt_context* ctx, zrt_film* film, const zrt_camera* camera,
                           const zrt_render_config* cfg, const zrt_outputs* outputs_or_null,
                           zrt_stats* stats_or_null);

/* ---- adaptive films: sample only unconverged pixels (ABI 2, added) ------- */

/* zrt_context_refine is zrt_context_accumulate for the pixels of a film whose
 * image is still changing.  Beside its sums the film keeps, from its first
 * refine call on: per pixel a frozen flag and the count n[q] it was frozen at;
 * per pixel the checkpoint, its linear value when the previous refine call
 * started tracing; and the checkpoint's sample count c (0: none).  A pixel that
 * is not frozen holds the film's samples.
 *
 * A call does, in this order, with b = the film's samples and
 * n = cfg->num_samples (all f32, nothing contracted, left to right as written,
 * sqrt and / IEEE-rounded):
 * 1. Decide.  If c == 0 or b < min_samples nothing changes.  Otherwise, for
 *    every pixel q that is not frozen:
 *      cur = sum[q] * (1.0f / (float)b)        the image a film shows at b
 *      p   = checkpoint[q]                     the image it showed at c
 *      d   = (|cur.x - p.x| + |cur.y - p.y|) + |cur.z - p.z|
 *      m   = (cur.x + cur.y) + cur.z
 *      k   = (float)b / (float)(b - c)         "last batch's mean vs the mean before it"
 *      err = (d * k) / sqrt(fmaxf(m, 0x1p-10f))
 *    and the pixel is frozen iff !(err > threshold) (a NaN error freezes).  A
 *    frozen pixel keeps n[q] = b and its sum and is not traced again until
 *    zrt_film_reset / zrt_film_write.
 * 2. Compact.  The active pixels in zrt_tile_pixels order are the call's pixel
 *    list; A is their number, *active_or_null = A.
 * 3. Trace.  If A == 0 nothing is traced and the film's samples, c and the
 *    checkpoints stay.  Otherwise, for every active pixel, checkpoint[q] = cur
 *    (not when b == 0), c = b, and samples b .. b + n - 1 -- the paths a
 *    zrt_context_render of this camera, seed and max_bounce traces for that
 *    pixel and those indices -- are added to sum[q] in sample order (from +0
 *    when b == 0); the film's samples become b + n.
 * 4. Present.  For EVERY owned pixel linear = sum[q] * (1.0f / (float)N) with
 *    N = n[q] if frozen, else the film's samples, and rgb = toRGB(linear), into
 *    whichever zrt_outputs fields are set (they mean what they mean in a
 *    render); sample_counts[q] = N.  A call that asks for none of them runs no
 *    present pass.
 * So every pixel's outputs are, bit for bit, the one-shot render's pixel at N
 * samples, in every kernel mode and for any samples_per_pass; and while nothing
 * is frozen (min_samples above the frame's final count) the calls are
 * zrt_context_accumulate's, outputs and stats.
 * The kernels are chosen as a render of A pixels and n samples chooses them
 * (A * n against the 2^23-sample thresholds).  stats are those of the traced
 * paths only: samples = A * n, segments and the counting build's counters of
 * samples b .. b + n - 1 of the active pixels, trace_launches of a render of A
 * pixels; A == 0 gives all zero.  zrt_context_profile records the trace as a
 * render.
 * ZRT_ERR_INVALID_ARG (max_bounce > 32: ZRT_ERR_UNSUPPORTED) before any device
 * work, film and outputs untouched: what zrt_context_accumulate refuses, a null
 * refine, a NaN threshold, b + n > 65535.
 * zrt_context_accumulate on a film with a frozen pixel is ZRT_ERR_INVALID_ARG;
 * on a film without one it leaves c and the checkpoints alone.  zrt_film_reset
 * and zrt_film_write clear the frozen flags and c.  zrt_film_read returns the
 * sums as stored; zrt_film_counts says how many samples each holds. */
typedef struct zrt_refine_config {
    uint32_t* sample_counts;  /* host, n_owned, or null: every owned pixel's count after the call */
    float threshold;          /* a pixel stays active iff err > threshold; NaN: ZRT_ERR_INVALID_ARG */
    uint32_t min_samples;     /* no pixel is frozen while the film holds fewer samples than this */
} zrt_refine_config;          /* 16 B */

int zrt_context_refine(zrt_context* ctx, zrt_film* film, const zrt_camera* camera,
                       const zrt_render_config* cfg, const zrt_refine_config* refine,
                       const zrt_outputs* outputs_or_null, zrt_stats* stats_or_null,
                       uint32_t* active_or_null);
/* counts: host n_owned or null; active: pixels not frozen, or null */
int zrt_film_counts(zrt_film* film, uint32_t* counts, uint32_t* active);

/* ---- denoise: edge-avoiding a-trous filter (ABI 2, added) ---------------- */

/* The last stage of a progressive frame: a colour frame of a few samples --
 * a plane, or a film's sums -- smoothed under the guidance of the feature
 * planes zrt_context_features gives, on the device, into an image one can look
 * at.  It is the edge-avoiding a-trous wavelet filter (Dammertz et al. 2010):
 * `iterations` levels of a 5x5 B3-spline kernel with holes, each tap weighted
 * by how far its colour, normal, depth and albedo are from the centre pixel's.
 * The weights are compact polynomials, not exp: every operation is an IEEE f32
 * + - * /, fmaxf or a comparison, left to right as written, nothing contracted
 * (no FMA); `/` is the IEEE division and fmaxf is C's (a NaN operand gives the
 * other operand).  So the result is the same bits everywhere.
 *
 * P = w * h.  All planes, in and out, are in zrt_tile_pixels(w, h, tile_size,
 * 0, 1) order -- the order zrt_context_features and a film of rank 0 of 1 use;
 * with ZRT_DENOISE_ROW_MAJOR they are in row-major image order and tile_size
 * is ignored (a caller who gathered several ranks' tiles).  The filter needs
 * every pixel's neighbours: one call covers one whole frame, there is no rank.
 *
 * Colour source: exactly one of `color` and `film`.  A film must belong to
 * ctx, have the same w, h and tile_size (after defaults), be rank 0 of 1 and
 * hold at least one sample; ZRT_DENOISE_ROW_MAJOR with a film is refused.  The
 * colour of the film's pixel q is step 4 of zrt_context_refine:
 * sum[q] * (1.0f / (float)N), N = the pixel's frozen count if it is frozen,
 * else the film's samples.  The film is read, never written.
 *
 * With c_0 the colour frame and h = (1/16, 1/4, 3/8, 1/4, 1/16), for level
 * i = 0 .. iterations - 1, step = 1 << i:
 *   s_i = sigma_color * 2^-i (exact);  kc = 1.0f / (s_i * s_i)
 *   kn = 1.0f / (sigma_normal * sigma_normal);  kz, ka likewise from
 *   sigma_depth, sigma_albedo
 *   for every pixel p = (x, y):
 *     iz = 1.0f / fmaxf(depth[p], 0x1p-20f)      the depth guide is relative
 *     S = (+0, +0, +0), W = +0
 *     for dy = -2 .. 2 (outer), dx = -2 .. 2 (inner), q = (x + dx * step,
 *     y + dy * step), in this order:
 *       a tap outside the image is skipped
 *       k  = h[dx + 2] * h[dy + 2]                (exact)
 *       dc = c_i[p] - c_i[q] per component
 *       xc = ((dc.x * dc.x + dc.y * dc.y) + dc.z * dc.z) * kc
 *       wc = fmaxf(1.0f - xc, 0.0f);  wc = wc * wc
 *       wn likewise from normal[p] - normal[q] and kn
 *       wa likewise from albedo[p] - albedo[q] and ka
 *       r  = (depth[p] - depth[q]) * iz;  xz = (r * r) * kz
 *       wz = fmaxf(1.0f - xz, 0.0f);  wz = wz * wz
 *       wt = (((k * wc) * wn) * wz) * wa -- an absent guide's factor is left
 *            out, not multiplied as 1.0f
 *       if !(wt > 0) the tap is skipped: a NaN anywhere in a tap's guides or
 *       colour difference drops that tap and does not poison the sum; a NaN
 *       centre pixel drops every tap
 *       S.k = S.k + c_i[q].k * wt for k = 0, 1, 2;  W = W + wt
 *     c_{i+1}[p] = (S.x / W, S.y / W, S.z / W) if W > 0, else c_i[p] bit for bit
 * The guides are the same at every level; only the colour is filtered.
 * linear = c_iterations, rgb = toRGB(linear) with the render's own toRGB.  An
 * inf the arithmetic produces is stored as it is.  A sigma of +inf is allowed:
 * its k is 0 and the guide drops only taps whose difference is not finite. */
#define ZRT_DENOISE_ROW_MAJOR 0x100000u  /* zrt_denoise_batch.flags only: planes in row-major image order */

typedef struct zrt_denoise_batch {
    uint32_t w, h, tile_size; /* the frame; tile_size 0 = 64 */
    uint32_t iterations;      /* 1..8 */
    float sigma_color, sigma_normal, sigma_depth, sigma_albedo;   /* > 0, +inf allowed; an absent guide's
                                                                     is not read */
    const float* color;       /* P * 3 linear, or null when `film` is given */
    zrt_film* film;           /* or null */
    const float* normal;      /* P * 3, or null: that guide's weight is 1 */
    const float* depth;       /* P, or null */
    const float* albedo;      /* P * 3, or null */
    float* linear;            /* P * 3, or null */
    uint8_t* rgb;             /* P * 3, or null (linear and rgb not both null) */
    uint32_t on_device;       /* as zrt_ray_batch; applies to color, normal, depth, albedo, linear, rgb
                                 (4-byte aligned, rgb 1-byte) */
    uint32_t flags;           /* ZRT_DENOISE_ROW_MAJOR; any other bit is ZRT_ERR_INVALID_ARG */
    uint32_t _reserved;       /* 0 */
} zrt_denoise_batch;          /* 104 B; offsets 0 4 8 12 16 20 24 28 32 40 48 56 64 72 80 88 92 96 */

/* Synchronous, one thread at a time per context; alternates freely with
 * renders, films and every query (the work buffers are its own: four 16-byte
 * records per pixel, grow-only, freed with the context) and leaves
 * zrt_context_profile's record untouched.
 * ZRT_ERR_INVALID_ARG before any device work, the outputs untouched: a null
 * context or batch; w or h of 0, or P above 2^31; a tile_size zrt_tile_pixels
 * refuses (not with ZRT_DENOISE_ROW_MAJOR, which ignores it); iterations 0 or
 * above 8; sigma_color, or the sigma of a present guide, that is NaN, zero or
 * negative; color and film both set or both null; a film that breaks the rules
 * above; linear and rgb both null; on_device > 1; a non-zero _reserved; any
 * other flag bit.
 * stats (may be null): samples = P; segments = cells_visited = triangle_tests =
 * hits = 0; render_ms the device time of the call, trace_kernel_ms that of its
 * kernels (the same for device pointers; a host call's render_ms includes the
 * staging copies); trace_launches = iterations + 2: one gather, one launch per
 * level, one present. */
int zrt_context_denoise(zrt_context* ctx, const zrt_denoise_batch* batch, zrt_stats* stats_or_null);

/* ---- reproject: carry a frame's history across a camera change (ABI 2, added) */

/* The stage between the film and the denoiser when the camera moves: the
 * previous frame's colour is fetched where each pixel of the current frame was
 * seen from the previous camera, and blended with the current colour by
 * 1 / history length.  The materials are diffuse, transparent or emissive and
 * the sky depends on direction only, so the radiance leaving a surface point
 * does not depend on the view: reprojected history is unbiased except at
 * disocclusions and over the bilinear footprint.  For every pixel: the world
 * point it sees from the current depth plane and camera; that point projected
 * into the previous camera; the previous colour there from four bilinear taps,
 * a tap counting only if the previous depth (and normal, if given) agrees.
 * Every operation is an IEEE f32 + - * /, sqrt, floorf, fabsf or a comparison,
 * left to right as written, nothing contracted (no FMA): the same bits
 * everywhere.
 *
 * w, h come from `camera`; P = w * h.  All planes, in and out, are in
 * zrt_tile_pixels(w, h, tile_size, 0, 1) order; with ZRT_REPROJECT_ROW_MAJOR
 * they are row-major and tile_size is ignored.  One call covers a whole
 * frame: there is no rank.
 *   dot(a, b)   = (a.x*b.x + a.y*b.y) + a.z*b.z
 *   cross(a, b) = (a.y*b.z - a.z*b.y, a.z*b.x - a.x*b.z, a.x*b.y - a.y*b.x)
 *
 * Colour source: exactly one of `color` and `film`.  The film's rules and its
 * presented value are zrt_context_denoise's: it must belong to ctx, have the
 * same w, h and tile_size (after defaults), be rank 0 of 1 and hold at least
 * one sample; ZRT_REPROJECT_ROW_MAJOR with a film is refused; its colour is
 * sum * (1.0f / (float)N) at the pixel's own count N; it is read, never
 * written.
 *
 * Per-call constants, computed once in f32 as written.  O, L, R, U are the
 * current camera's origin, lower_left_corner, right and up; primes are the
 * previous camera's:
 *   A = cross(U', L'), B = cross(L', R'), Cv = cross(R', U'), D = dot(L', Cv)
 *   if D < 0: A, B and Cv are negated (exact)
 *   if D is zero or NaN no pixel has a projection
 *   tn2 = normal_tolerance * normal_tolerance
 *
 * Projection.  For pixel p = (x, y) with packed index k, c its current colour
 * and z = depth[k], the projection is defined iff z > 0 and z < +inf, D is
 * usable and g > 0 below:
 *   v  = (L + R * ((float)x + 0.5f)) + U * ((float)y + 0.5f)    the render's getRay order, at the pixel centre
 *   d  = v * (1.0f / sqrt((v.x*v.x + v.y*v.y) + v.z*v.z))        the render's normalisation
 *   X  = O + d * z;   q = X - O'
 *   g  = dot(q, Cv);  a = dot(q, A) / g;  b = dot(q, B) / g;  zq = sqrt(dot(q, q))
 * (a, b) are the previous camera's continuous pixel coordinates of X and zq
 * the depth the previous frame should hold there.
 * motion[k] = (a - ((float)x + 0.5f), b - ((float)y + 0.5f)); without a
 * projection motion[k] is two 0x7FC00000.
 *
 * History needs a projection.  fx = a - 0.5f, fy = b - 0.5f, and all four of
 * fx > -1.0f, fx < (float)w, fy > -1.0f, fy < (float)h (a NaN fails).
 * x0 = (int)floorf(fx), tx = fx - (float)x0; y0 and ty likewise.
 * S = (+0, +0, +0), W = +0, M = 0xFFFFFFFF; for j = 0, 1 (outer), i = 0, 1
 * (inner), in this order, tap t = (x0 + i, y0 + j):
 *   a tap outside the image is skipped
 *   bw = (i ? tx : 1.0f - tx) * (j ? ty : 1.0f - ty);            skipped if !(bw > 0)
 *   zp = prev_depth[t];                                           skipped if !(zp > 0)
 *   skipped if !(fabsf(zp - zq) <= depth_tolerance * zq)
 *   if normal and prev_normal are both given:
 *     dn = normal[p] - prev_normal[t];   skipped if !(((dn.x*dn.x + dn.y*dn.y) + dn.z*dn.z) <= tn2)
 *   cp = prev_color[t];                                           skipped if a component is NaN or infinite
 *   lp = prev_length ? prev_length[t] : 1;                        skipped if lp == 0
 *   S.k = S.k + cp.k * bw (k = 0, 1, 2);  W = W + bw;  M = min(M, lp)
 *
 * Blend.  If W > 0: hist = (S.x / W, S.y / W, S.z / W), N = min(M,
 * max_history - 1) + 1, alpha = 1.0f / (float)N, out = (hist * (1.0f - alpha))
 * + (c * alpha) per component -- when N == 1, out is c bit for bit.  Else
 * out = c bit for bit and N = 1.  color_out[k] = out, length_out[k] = N.  A
 * NaN or inf the arithmetic produces is stored as it is; it heals at the next
 * call, because such a tap is skipped.
 *
 * Aliasing: the call reads the previous planes completely before it writes
 * anything.  color_out may be the same pointer as prev_color or as color, and
 * length_out the same pointer as prev_length; any other overlap is
 * unspecified.  So a caller keeps one history buffer and passes this frame's
 * depth and normal planes as the next call's prev_*. */
#define ZRT_REPROJECT_ROW_MAJOR 0x200000u   /* zrt_reproject_batch.flags only: planes in row-major image order */

typedef struct zrt_reproject_batch {
    uint32_t tile_size;          /* 0 = 64 */
    uint32_t max_history;        /* 1..65535: N never exceeds it, so alpha >= 1 / max_history */
    float depth_tolerance;       /* >= 0, +inf allowed; relative */
    float normal_tolerance;      /* >= 0, +inf allowed; not read unless both normal planes are given */
    uint32_t on_device;          /* applies to every plane pointer; the cameras are always host */
    uint32_t flags;              /* ZRT_REPROJECT_ROW_MAJOR; any other bit is ZRT_ERR_INVALID_ARG */
    const zrt_camera* camera;        /* current */
    const zrt_camera* prev_camera;   /* same w, h */
    const float* color;          /* P * 3, or null when film is given */
    zrt_film* film;              /* or null */
    const float* depth;          /* P */
    const float* normal;         /* P * 3 or null */
    const float* prev_color;     /* P * 3 */
    const float* prev_depth;     /* P */
    const float* prev_normal;    /* P * 3 or null */
    const uint32_t* prev_length; /* P or null: 1 everywhere */
    float* color_out;            /* P * 3 */
    uint32_t* length_out;        /* P or null */
    float* motion;               /* P * 2 or null */
    uint64_t _reserved;          /* 0 */
} zrt_reproject_batch;           /* 136 B; offsets 0 4 8 12 16 20 24 32 40 48 56 64 72 80 88 96 104 112 120 128 */

/* Synchronous, one thread at a time per context; alternates freely with every
 * other call (the work buffers are its own: two 16-byte records per pixel,
 * grow-only, freed with the context) and leaves zrt_context_profile's record
 * untouched.
 * ZRT_ERR_INVALID_ARG before any device work, the outputs untouched: a null
 * context or batch, or either camera null; w or h of 0, P above 2^31, or a
 * previous camera of another size; a tile_size zrt_tile_pixels refuses (not
 * with ZRT_REPROJECT_ROW_MAJOR); max_history of 0 or above 65535; a tolerance
 * that is NaN or negative (normal_tolerance only when both normals are given);
 * color and film both set or both null; a film that breaks the rules above;
 * null depth, prev_color, prev_depth or color_out; on_device > 1; a non-zero
 * _reserved; any other flag bit.
 * stats (may be null): samples = P; hits = the pixels with W > 0; segments =
 * cells_visited = triangle_tests = 0; render_ms the device time of the call,
 * trace_kernel_ms that of its kernels (the same for device pointers; a host
 * call's render_ms includes the staging copies); trace_launches = 2: the
 * gather of the previous planes into row-major records, and the reprojection. */
int zrt_context_reproject(zrt_context* ctx, const zrt_reproject_batch* batch, zrt_stats* stats_or_null);

/* ---- svgf: luminance moments and a variance-guided a-trous filter (ABI 2, added) */

/* zrt_context_denoise weighs colour by one absolute sigma for the whole frame;
 * it does not know how noisy a pixel is.  These two calls add what it lacks
 * (SVGF, Schied et al. 2017): the colour is divided by the first-hit albedo so
 * that texture is not filtered, the first two moments of its luminance are
 * kept beside it, and the filter's luminance weight is scaled by each pixel's
 * own standard deviation -- estimated from the moments' history where it is
 * long enough, from the pixel's 7x7 neighbourhood where not -- and the
 * variance is filtered along with the colour, so that later levels narrow as
 * the image cleans up.  The temporal half needs no call of its own:
 * zrt_context_reproject blends any 3-channel plane by 1 / N, the moments
 * plane (l, l*l, 0) included.  One frame of a preview:
 *   zrt_context_features -> zrt_context_illumination (film, albedo) ->
 *   zrt_context_reproject (illumination) -> zrt_context_reproject (moments,
 *   same previous guides, camera and lengths) -> zrt_context_svgf.
 * Every operation is an IEEE f32 + - * /, sqrt, fmaxf, fabsf or a comparison,
 * left to right as written, nothing contracted (no FMA); fmaxf is C's (a NaN
 * operand gives the other operand): the same bits everywhere.
 *
 *   lum(c)  = (0.2126f * c.x + 0.7152f * c.y) + 0.0722f * c.z
 *   dmod(a) = fmaxf(a, 0x1p-4f) per component; a NaN albedo gives 0x1p-4f
 *
 * P = w * h.  All planes, in and out, are in zrt_tile_pixels(w, h, tile_size,
 * 0, 1) order; with ZRT_SVGF_ROW_MAJOR they are in row-major image order and
 * tile_size is ignored.  One call covers one whole frame: there is no rank.
 *
 * zrt_context_illumination.  Colour source: exactly one of `color` and
 * `film`.  The film's rules and its presented value are zrt_context_denoise's:
 * it must belong to ctx, have the same w, h and tile_size (after defaults), be
 * rank 0 of 1 and hold at least one sample; ZRT_SVGF_ROW_MAJOR with a film is
 * refused; its colour is sum * (1.0f / (float)N) at the pixel's own count N;
 * it is read, never written.  For every pixel, c its colour:
 *   I.k = c.k / dmod(albedo.k) for k = 0, 1, 2; without an albedo I is c bit
 *   for bit
 *   l = lum(I);  illumination = I;  moments = (l, l * l, +0)
 * The moments take three channels so that the plane goes through
 * zrt_context_reproject as a colour plane. */
#define ZRT_SVGF_ROW_MAJOR 0x400000u   /* zrt_illumination_batch.flags and zrt_svgf_batch.flags only: planes in
                                          row-major image order */

typedef struct zrt_illumination_batch {
    uint32_t w, h, tile_size; /* the frame; tile_size 0 = 64 */
    const float* color;       /* P * 3 linear, or null when `film` is given */
    zrt_film* film;           /* or null */
    const float* albedo;      /* P * 3, or null: no demodulation */
    float* illumination;      /* P * 3, or null */
    float* moments;           /* P * 3, or null (illumination and moments not both null) */
    uint32_t on_device;       /* as zrt_ray_batch; applies to color, albedo, illumination, moments */
    uint32_t flags;           /* ZRT_SVGF_ROW_MAJOR; any other bit is ZRT_ERR_INVALID_ARG */
    uint32_t _reserved;       /* 0 */
} zrt_illumination_batch;     /* 72 B; offsets 0 4 8 16 24 32 40 48 56 60 64 */

/* Synchronous, one thread at a time per context; alternates freely with every
 * other call (a host call's planes are staged in the svgf work buffer,
 * grow-only, freed with the context) and leaves zrt_context_profile's record
 * untouched.
 * ZRT_ERR_INVALID_ARG before any device work, the outputs untouched: a null
 * context or batch; w or h of 0, or P above 2^31; a tile_size zrt_tile_pixels
 * refuses (not with ZRT_SVGF_ROW_MAJOR, which ignores it); color and film both
 * set or both null; a film that breaks the rules above; illumination and
 * moments both null; on_device > 1; a non-zero _reserved; any other flag bit.
 * stats (may be null): samples = P; segments = cells_visited = triangle_tests =
 * hits = 0; render_ms the device time of the call, trace_kernel_ms that of its
 * kernel (the same for device pointers; a host call's render_ms includes the
 * staging copies); trace_launches = 1. */
int zrt_context_illumination(zrt_context* ctx, const zrt_illumination_batch* batch, zrt_stats* stats_or_null);

/* zrt_context_svgf.  `color` is the illumination, normally after
 * reprojection; `moments` the reprojected moments (component 2 is ignored) and
 * `length` the history lengths zrt_context_reproject wrote (null: 1
 * everywhere).  `normal` and `depth` are the guides; `albedo` is not a guide:
 * the output is remodulated by it.  With h = (1/16, 1/4, 3/8, 1/4, 1/16),
 * kn = 1.0f / (sigma_normal * sigma_normal), kz likewise from sigma_depth, and
 * for a centre p and a tap q, exactly as zrt_context_denoise defines them:
 *   iz = 1.0f / fmaxf(depth[p], 0x1p-20f)
 *   dn = normal[p] - normal[q];  xn = ((dn.x*dn.x + dn.y*dn.y) + dn.z*dn.z) * kn
 *   wn = fmaxf(1.0f - xn, 0.0f);  wn = wn * wn
 *   r  = (depth[p] - depth[q]) * iz;  xz = (r * r) * kz
 *   wz = fmaxf(1.0f - xz, 0.0f);  wz = wz * wz
 *
 * Variance estimate v_0[p].  N = length[p], or 1 when length is null;
 * m = moments[p].
 *   if moments is given and N >= 4:  v_0 = fmaxf(m.y - m.x * m.x, 0.0f)
 *     (the sign of a zero v_0 is unspecified when m.y is -0)
 *   otherwise the spatial estimate:  S1 = S2 = W = +0
 *     for dy = -3 .. 3 (outer), dx = -3 .. 3 (inner), q = (x + dx, y + dy):
 *       a tap outside the image is skipped
 *       wt = wn * wz -- an absent guide's factor is left out; with both absent
 *            wt = 1.0f
 *       lq = lum(color[q])
 *       the tap is skipped if !(wt > 0) or !(fabsf(lq) < +inf)
 *       S1 = S1 + lq * wt;  S2 = S2 + (lq * lq) * wt;  W = W + wt
 *     if W > 0:  m1 = S1 / W;  m2 = S2 / W
 *                v_0 = fmaxf(m2 - m1 * m1, 0.0f) * (4.0f / (float)min(max(N, 1), 4))
 *     else       v_0 = +0
 * A short history widens the spatial estimate: it saw few samples.
 *
 * Level i = 0 .. iterations - 1, step = 1 << i, for every pixel p = (x, y):
 *   g = the 3x3 Gaussian of v_i around p at step 1:  Sg = Wg = +0
 *     for dy = -1 .. 1 (outer), dx = -1 .. 1 (inner), q = (x + dx, y + dy):
 *       kk = {1/16, 1/8, 1/16; 1/8, 1/4, 1/8; 1/16, 1/8, 1/16}[dy + 1][dx + 1]
 *       a tap outside the image is skipped
 *       Sg = Sg + v_i[q] * kk;  Wg = Wg + kk
 *     g = Sg / Wg
 *   den = sigma_luminance * sqrt(g) + 0x1p-16f;  kl = 1.0f / (den * den)
 *   S = (+0, +0, +0), W = +0, V = +0
 *   for dy = -2 .. 2 (outer), dx = -2 .. 2 (inner), q = (x + dx * step,
 *   y + dy * step), zrt_context_denoise's order:
 *     a tap outside the image is skipped
 *     k  = h[dx + 2] * h[dy + 2]                  (exact)
 *     dl = lum(c_i[p]) - lum(c_i[q]);  xl = (dl * dl) * kl
 *     wl = fmaxf(1.0f - xl, 0.0f);  wl = wl * wl
 *     wt = ((k * wl) * wn) * wz -- an absent guide's factor is left out
 *     the tap is skipped if !(wt > 0)
 *     S.k = S.k + c_i[q].k * wt for k = 0, 1, 2;  W = W + wt
 *     V = V + v_i[q] * (wt * wt)
 *   if W > 0:  c_{i+1}[p] = (S.x / W, S.y / W, S.z / W);  v_{i+1}[p] = V / (W * W)
 *   else both keep their input bits
 * What follows from the rules: a NaN centre colour makes every wl 0, drops
 * every tap and returns its bits; a NaN in g makes kl NaN, so that pixel
 * passes through for that level; a NaN tap colour drops that tap only.  A NaN
 * tap variance does not drop the tap: it reaches V.
 *
 * Present.  f = c_iterations[p]; with albedo f.k = f.k * dmod(albedo.k);
 * linear = f, rgb = toRGB(f) with the render's own toRGB, variance =
 * v_iterations[p] (of the illumination: it is not remodulated).  A NaN or inf
 * the arithmetic produces is stored as it is.  A sigma of +inf is allowed. */
typedef struct zrt_svgf_batch {
    uint32_t w, h, tile_size; /* the frame; tile_size 0 = 64 */
    uint32_t iterations;      /* 1..8 */
    float sigma_luminance, sigma_normal, sigma_depth;   /* > 0, +inf allowed; an absent guide's is not read */
    const float* color;       /* P * 3: the illumination */
    const float* moments;     /* P * 3, or null: the spatial estimate everywhere */
    const uint32_t* length;   /* P, or null: 1 everywhere */
    const float* normal;      /* P * 3, or null: that guide's weight is left out */
    const float* depth;       /* P, or null */
    const float* albedo;      /* P * 3, or null: no remodulation */
    float* linear;            /* P * 3, or null */
    uint8_t* rgb;             /* P * 3, or null (linear and rgb not both null) */
    float* variance;          /* P, or null */
    uint32_t on_device;       /* as zrt_ray_batch; applies to every plane pointer (4-byte aligned, rgb 1-byte) */
    uint32_t flags;           /* ZRT_SVGF_ROW_MAJOR; any other bit is ZRT_ERR_INVALID_ARG */
    uint32_t _reserved;       /* 0 */
} zrt_svgf_batch;             /* 120 B; offsets 0 4 8 12 16 20 24 32 40 48 56 64 72 80 88 96 104 108 112 */

/* Synchronous, one thread at a time per context; alternates freely with every
 * other call (the work buffers are its own: three 16-byte records per pixel
 * and 8 KB of counters, grow-only, freed with the context) and leaves
 * zrt_context_profile's record untouched.
 * ZRT_ERR_INVALID_ARG before any device work, the outputs untouched: a null
 * context or batch; w or h of 0, or P above 2^31; a tile_size zrt_tile_pixels
 * refuses (not with ZRT_SVGF_ROW_MAJOR, which ignores it); iterations 0 or
 * above 8; sigma_luminance, or the sigma of a present guide, that is NaN, zero
 * or negative; a null color; linear and rgb both null; on_device > 1; a
 * non-zero _reserved; any other flag bit.
 * stats (may be null): samples = P; hits = the pixels whose v_0 came from the
 * moments; segments = cells_visited = triangle_tests = 0; render_ms the device
 * time of the call, trace_kernel_ms that of its kernels (the same for device
 * pointers; a host call's render_ms includes the staging copies);
 * trace_launches = iterations + 3: one gather, the variance estimate, one
 * launch per level, one present. */
int zrt_context_svgf(zrt_context* ctx, const zrt_svgf_batch* batch, zrt_stats* stats_or_null);

/* A device group: one context per entry of `devices` (HIP ordinals, repeats
 * allowed), the scene resident on each, rendered by one call -- Scene.render's
 * spawn + join of its workers (stage3.zig:247-256) across GPUs in one
 * process.  zrt_group_render splits this process's share of the image (the
 * tiles t with t % cfg->num_ranks == cfg->rank; cfg->device is ignored) over
 * the devices, device i taking sub-rank i, on one host thread each; with
 * num_ranks <= 1 the devices' packed tiles are copied to devices[0] (peer copy
 * over xGMI), scattered into the image there and copied to rgb_out once,
 * otherwise each device's pixels are written into rgb_out from the host (other
 * pixels untouched).  stats: sums over devices; render_ms = the slowest. */
typedef struct zrt_group zrt_group;
int zrt_group_create(const zrt_scene* scene, const int32_t* devices, uint32_t num_devices, zrt_group** out);
/* Geometry.build + bakeInto on every device of the group (as
 * zrt_context_create_built; the builds run in parallel, bit-identical). */
int zrt_group_create_built(const float* positions, const float* normals, const float* texcoords,
                           const uint32_t* material, uint32_t num_triangles, const uint32_t resolution[3],
                           uint32_t num_materials, const zrt_material* materials, const float* texels,
                           uint64_t num_texel_floats, const int32_t* devices, uint32_t num_devices,
                           zrt_group** out);
int zrt_group_render(zrt_group* g, const zrt_camera* camera, const zrt_render_config* cfg, uint8_t* rgb_out,
                     zrt_stats* stats);
/* The group's i-th context (owned by the group), e.g. for zrt_context_grid_info. */
int zrt_group_context(zrt_group* g, uint32_t i, zrt_context** out);
void zrt_group_destroy(zrt_group* g);

/* Per-kernel breakdown of the context's last zrt_context_render (bench.py's
 * roofline: the dominant kernel's launch time and algorithmic work).
 * ms / launches per kernel class; ms only with ZRT_FLAG_KERNEL_TIMES (else 0).
 * primary_counts: segments, cells visited, triangle tests, hits of the
 * primary (camera) segments, counting renders (ZRT_FLAG_COUNT_STATS) only --
 * the bounce launches' work is zrt_stats' totals minus these. */
enum {
    ZRT_KERNEL_PRIMARY = 0,   /* wf_kernel, primary launch (camera rays) */
    ZRT_KERNEL_PARK = 1,      /* wf_park_kernel, bounce trace */
    ZRT_KERNEL_SHADE = 2,     /* wf_shade_kernel, bounce shading */
    ZRT_KERNEL_BOUNCE = 3,    /* wf_kernel, bounce launch (lane walk / no OccX) */
    ZRT_KERNEL_RESOLVE = 4,   /* wf_resolve_kernel / resolve_kernel (a film's call: their film forms) */
    ZRT_KERNEL_COUNT = 5,     /* trace_kernel (counting build) */
    ZRT_KERNEL_CLASSES = 8
};
typedef struct zrt_kernel_profile {
    double ms[ZRT_KERNEL_CLASSES];
    uint32_t launches[ZRT_KERNEL_CLASSES];
    uint32_t passes;                 /* passes of the frame */
    uint32_t sets;                   /* pass sets (streams) it ran on */
    uint64_t primary_counts[4];
} zrt_kernel_profile;
int zrt_context_profile(const zrt_context* ctx, zrt_kernel_profile* out);

/* The context's grid and {num_refs, empty cells, min refs of a non-empty cell
 * (0xFFFFFFFF if none), max refs of a cell}: the grid statistics the
 * reference logs after Geometry.build (main.zig:117-118), without a host copy
 * of the cells. */
int zrt_context_grid_info(zrt_context* ctx, zrt_grid* grid, uint32_t info[4]);

/* Pixels owned by `rank` (row-major image indices) in the packed output
 * order: tiles t = rank, rank+num_ranks, ... (row-major tile order), each
 * tile walked in 8x8 blocks.  pixels may be NULL to query *count. */
int zrt_tile_pixels(uint32_t w, uint32_t h, uint32_t tile_size, uint32_t rank,
                    uint32_t num_ranks, uint32_t* pixels, uint32_t* count);

/* ---- stage 1: glTF scene load + camera (stage1.zig) --------------------- */
typedef struct zrt_gltf zrt_gltf;

/* Loads .gltf (+ .bin, + PNG images) or .glb; triangle soup in node order
 * (stage1.zig:217-259), materials (stage1.zig:381-496), cameras. */
int zrt_gltf_load(const char* path, uint32_t num_threads, zrt_gltf** out);
int zrt_gltf_soup(const zrt_gltf* g, const float** positions, const float** normals,
                  const float** texcoords, const uint32_t** material, uint32_t* num_triangles);
/* Fills the material/texel fields of *scene (views valid until free). */
int zrt_gltf_materials(const zrt_gltf* g, zrt_scene* scene);
/* stage1.zig:309-371; width/height < 0 mean "not given". */
int zrt_gltf_camera(const zrt_gltf* g, const char* camera_name, int32_t width, int32_t height,
                    zrt_camera* out);
void zrt_gltf_free(zrt_gltf* g);

/* stage1.zig:309-371 from an explicit node matrix (column-major 16). */
int zrt_camera_from_matrix(const float matrix[16], float yfov, int has_aspect_ratio,
                           float aspect_ratio, int32_t width, int32_t height, zrt_camera* out);

/* ---- device-function parity probes (tests only; run on the GPU) -------- */
enum {
    ZRT_PROBE_TRIANGLE = 0,   /* in n*15 (v0,v1,v2,orig,dir) -> out n*4 (hit,t,u,v) */
    ZRT_PROBE_BBOX = 1,       /* in n*12 (min,max,orig,dir) -> out n*2 (hit,t) */
    ZRT_PROBE_DDA = 2,        /* in n*12 (min,max,orig,dir) + res u32[3] in aux -> out n*(4+4*64):
                                 steps (-1 miss, -2 bad linear index), first cell, (cell, t) per next() */
    ZRT_PROBE_TO_RGB = 3,     /* in n*3 -> out n*3 (as float) */
    ZRT_PROBE_RNG_F32 = 4,    /* in n*3 u32 (seed_lo,pixel,sample) -> out n*16 floats */
    ZRT_PROBE_RNG_NORM = 5,   /* same -> out n*16 floats */
    ZRT_PROBE_EXP_LOG = 6,    /* in n doubles -> out n*2 doubles (exp, log) */
    ZRT_PROBE_TEXTURE = 7,    /* in n*2 (u,v) + aux texture -> out n*3 */
    ZRT_PROBE_TRIANGLE_FLAT = 8, /* as TRIANGLE, through the branch-free test of the park kernel */
    ZRT_PROBE_RECIP = 9,      /* in n floats det -> out n*2: the park / packed kernels' short 1/det
                                 (rcp + six FMAs), the IEEE-division kernels' 1.0f/det */
    ZRT_PROBE_RECIP_SWEEP = 10, /* in n*2 u32 {first float bits, count} -> out n*4 u32 {floats whose
                                 short 1/det differs in any bit from the device's IEEE 1.0f/det (NaN
                                 equals NaN), the smallest such bits (0xFFFFFFFF: none), 0, 0};
                                 every float of each range, on the device */
    ZRT_PROBE_TRIANGLE_EXACT = 11, /* as TRIANGLE, with the IEEE division of the ZRT_FLAG_MT_EXACT kernels */
    ZRT_PROBE_QUOT = 12,      /* in n*2 floats (a, b) -> out n*2: dda_init_fq's quotient quot_rn(a, b,
                                 1/b by the short reciprocal), the IEEE a / b */
    ZRT_PROBE_QUOT_SWEEP = 13, /* in n*2 u32 {first significand s_b, count} -> out n*4 u32 {pairs whose
                                 quot_rn differs in any bit from the IEEE quotient, the first such a's
                                 bits, its b's bits, 0}: every a in [1, 2) against every
                                 b = 1 + s / 2^23, s in [s_b, s_b + count), on the device */
};
int zrt_probe(int which, const void* in, void* out, uint32_t n, const void* aux, int device);
/* Comma-separated substrings of the mangled names of the timed kernel
 * instantiations in the gfx950 code object (build checks; no HIP call). */
const char* zrt_timed_kernels(void);

#ifdef __cplusplus
}
#endif
#endif /* ZRT_H */
