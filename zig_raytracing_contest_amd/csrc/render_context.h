// render_context.h -- what render.hip (kernels, launch plan, entry points),
// context.hip (building a zrt_context) and probe.hip share, each defined once.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "zrt_internal.h"
#include "dda.h"

#define HIP_TRY(expr)                                                            \
    do {                                                                         \
        hipError_t _e = (expr);                                                  \
        if (_e != hipSuccess) {                                                  \
            if (getenv("ZRT_DEBUG"))                                             \
                fprintf(stderr, "zrt: %s failed: %s (%s:%d)\n", #expr,           \
                        hipGetErrorString(_e), __FILE__, __LINE__);              \
            return _e == hipErrorOutOfMemory ? ZRT_ERR_OUT_OF_MEMORY : ZRT_ERR_HIP; \
        }                                                                        \
    } while (0)

// The tuning knobs read by this header or context.hip (an A/B build compiles
// both units with them, Makefile variant); the others: render.hip.
#ifndef ZRT_PARK_BLOCK_T
#define ZRT_PARK_BLOCK_T 1024
#endif
#ifndef ZRT_OCC_LDS_KB
#define ZRT_OCC_LDS_KB 16
#endif
#ifndef ZRT_OCC_SH0
#define ZRT_OCC_SH0 2
#endif
#ifndef ZRT_BFC_BUDGET_MB
#define ZRT_BFC_BUDGET_MB 2048
#endif
#ifndef ZRT_BFC_MIN_CLEARED
#define ZRT_BFC_MIN_CLEARED 1.0
#endif

namespace {

constexpr int kBlock = 256;                          // resolve / probes / helpers
constexpr int kParkBlock = ZRT_PARK_BLOCK_T;         // wf_park_kernel: one workgroup per CU
constexpr int kParkWaves = kParkBlock / 64;
constexpr uint32_t kTriFloats = 12u;                 // floats per ref of a context's triangle positions
constexpr uint32_t kMaxPassSets = 4;                 // pass sets (streams) of a render at most
// hop bits of a cell record's mask words (context.hip cell32_hop_kernel): six
// inverted bits from kHopShift up, in cells of at most kHopMaxRefs refs
constexpr uint32_t kHopMaxRefs = 26, kHopShift = 26;

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned lo = __shfl_xor((unsigned)x, off);
        const unsigned hi = __shfl_xor((unsigned)(x >> 32), off);
        x += ((unsigned long long)hi << 32) | lo;
    }
    return x;
}

// Per-wave LDS of the test rounds.
struct ParkSlot {
    float4 o[64];                    // lane's ray origin; w: nearest entering the round
    float4 d[64];                    // lane's ray direction; w (bits): the hop bits of its parked cell
    unsigned long long best[64];     // per parked lane: (t bits << 32) | ref of its best pair
    float2 uv[64];                   // (u, v) of that pair
    uint32_t mark[64];               // lane + 1 of the parked lane whose pairs start at this slot
};

struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (dev >= 0) (void)hipSetDevice(dev);
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

template <typename T>
int grow(T** p, size_t* cap, size_t n) {
    if (*cap >= n && *p) return ZRT_OK;
    if (*p) (void)hipFree(*p);
    *p = nullptr;
    *cap = 0;
    HIP_TRY(hipMalloc((void**)p, std::max<size_t>(n, 1) * sizeof(T)));
    *cap = n;
    return ZRT_OK;
}

// OccX (wf_park_kernel): LDS left for the blob in one 1024-thread workgroup
// per CU after the per-wave ParkSlots and the static ziggurat tables.
constexpr size_t kLdsPerCu = 160 * 1024;
constexpr size_t kParkSlotsBytes = (kParkBlock / 64) * sizeof(ParkSlot);
constexpr size_t kOccxBudget = kLdsPerCu - kParkSlotsBytes - 514 * sizeof(double) - kParkWaves * 192 * 4 - 256 -
                                256 * 8 -   // the select table
                                kParkWaves * 64 * 4;   // the escape slots

// OccX blob layout for nb bricks (nbw 32-brick words) and `occupied` masks:
// bits | u16 (1 + prefix) per word | (8-byte aligned) the zero mask + masks.
static void occx_layout(uint64_t nbw, uint64_t occupied, uint64_t* moff, uint64_t* words) {
    const uint64_t pw = (nbw + 1) / 2;                   // prefix words
    *moff = (nbw + pw + 1) & ~1ull;
    *words = *moff + 2 * (occupied + 1);
}
// u32 words of the LDS copy: 8-byte (bits, prefix) entries, then the masks
static uint64_t occx_lds_words(uint64_t nbw, uint64_t moff, uint64_t words) {
    return (2 * nbw + (words - moff) + 3) & ~3ull;
}

}  // namespace

// Nothing in this header depends on ZRT_SWEEP: the sweep library compiles
// only render.hip with -DZRT_SWEEP and links the other objects as built.
struct zrt_context {
    int device = 0;
    uint32_t mem_share = 1;            // contexts rendering on this device at once (a group's repeats)
    hipStream_t stream = nullptr;
    hipEvent_t ev_begin = nullptr, ev_end = nullptr;
    std::vector<hipEvent_t> ev_trace;
    zrt_grid grid{};
    uint32_t ncells = 0, nrefs = 0, nmat = 0;
    uint2* d_cells = nullptr;
    // packed walks (DdaV): the layout and the cells indexed by the packed word
    zrt::PackK pk{};
    bool packed = false;
    uint32_t* d_cell32 = nullptr;      // cell records at the packed index (cell32_kernel)
    float* d_pos = nullptr;
    float4* d_data = nullptr;
    zrt::DevMat* d_mats = nullptr;
    float* d_texels = nullptr;
    double* d_zig = nullptr;
    uint32_t* d_occ = nullptr;
    uint32_t occ_shift = 0, occ_nb[3] = {0, 0, 0}, occ_words = 0;
    uint32_t* d_occx = nullptr;     // exact per-cell occupancy blob (OccX), if it fits the LDS budget
    unsigned long long* d_bmask = nullptr;   // every 4^3 brick's cell mask, linear brick order (TraceParams::bmask)
    uint32_t* d_esc = nullptr;      // escape table (escape.h), with OccX
    uint32_t* d_sat = nullptr;      // summed-area table of cell occupancy (escape.h EscSat), or null
    // the primary frustum bounds (frustum_kernel) per 8x8 pixel block
    float4* d_tlo = nullptr; size_t tlo_cap = 0;
    bool esc_on = false;            // the park launches use it (dense enough to pay, context_escape)
    // park release (wf_park_kernel): the fraction of the occupied cells'
    // entry-face masks that are 0, and whether the launches use it
    double rel_frac = 0.0;
    bool rel_on = false;
    bool esc_tried = false;         // context_escape ran (at the first render that can use it)
    double esc_density = 0.0;       // fraction of its (brick, bin) bits set
    uint32_t esc_key = 0;           // the table's shape for the walk (escape.h esc_walk_key; 0: brick-level)
    bool esc_dir = false;           // ... built from one occupancy per cull bin (escape.h, the direction-aware table)
    size_t esc_extra = 0;           // its bytes beyond the brick-level table's (counted as held)
    // back-face cull masks (escape.h, context_bfcull): built at the first
    // render that can use them, if they fit kBfcBudget / mem_share
    uint32_t* d_bfc = nullptr;
    size_t bfc_bytes = 0;
    bool bfc_tried = false, bfc_tried_forced = false;
    bool bfc_stat = false;          // the statistic below is known
    bool bfc_on = false;            // the park launches use them unasked
    double bfc_frac = 0.0;          // cleared bits / ref bits of the cells of 1..32 refs
    double bfc_cleared = 0.0;       // cleared bits per (cell, bin) word of those cells
    uint32_t occx_words = 0, occx_nbw = 0, occx_moff = 0, occx_nb[3] = {0, 0, 0};
    bool occx_ok = false;
    // an edge component of 2^62 or more, or infinite: every launch takes the
    // lane walk with the IEEE division in Moller-Trumbore (kWf*Exact), since
    // the park and packed kernels' short reciprocal holds for |det| < 2^126
    // only (zrt_math.h mt_inv_det)
    bool mt_exact = false;
    // grow-only work buffers
    uint32_t* d_pix = nullptr; size_t pix_cap = 0;
    float4* d_out = nullptr; size_t out_cap = 0;     // counting build
    // wavefront buffers of one pass set (queues, terminal radiance, bounce
    // planes, counters, hit records); set k > 0 runs on its own stream
    struct PassSet {
        hipStream_t stream = nullptr;      // set 0: the context stream
        float4* q0 = nullptr; size_t q0_cap = 0;
        float4* q1 = nullptr; size_t q1_cap = 0;
        float4* term = nullptr; size_t term_cap = 0;
        float4* stk4 = nullptr; size_t stk4_cap = 0;   // bounce planes: (a, has e) per (slot, item)
        float2* stk2 = nullptr; size_t stk2_cap = 0;   //   e as a float4 (two float2) per (slot, item)
        uint32_t* wfc = nullptr; size_t wfc_cap = 0;
        float4* hit = nullptr; size_t hit_cap = 0;
        hipEvent_t ev_join = nullptr;      // set k > 0: its last pass is done
    };
    PassSet set[kMaxPassSets];
    float4* d_acc = nullptr; size_t acc_cap = 0;
    uint8_t* d_rgb = nullptr; size_t rgb_cap = 0;
    float* d_lin = nullptr; size_t lin_cap = 0;
    // zrt_context_trace: a host batch's chunk on the device (6 floats, 4 u32 per ray)
    float* d_rays = nullptr; size_t rays_cap = 0;
    uint32_t* d_hits = nullptr; size_t hits_cap = 0;
    // zrt_context_surface: a host batch's chunk of records (4 float4 per ray)
    float4* d_surf = nullptr; size_t surf_cap = 0;
    // zrt_context_features: the sums between passes (3 float4 per pixel) and a
    // host call's planes (12 words per pixel)
    float4* d_facc = nullptr; size_t facc_cap = 0;
    float* d_fout = nullptr; size_t fout_cap = 0;
    // zrt_context_denoise: the filter's records (4 float4 per pixel: colour +
    // depth twice, ping-pong; normal + 1/depth; albedo) and a host call's
    // planes in and out (10 words per pixel)
    float4* d_dn = nullptr; size_t dn_cap = 0;
    float* d_dnio = nullptr; size_t dnio_cap = 0;
    // zrt_context_radiance: a chunk's rays with normalised directions (6 floats per ray)
    float* d_nrays = nullptr; size_t nrays_cap = 0;
    std::vector<hipEvent_t> ev_pass;   // per pass: its resolve done
    hipEvent_t ev_fork = nullptr;
    uint32_t* d_counter = nullptr;
    unsigned long long* d_stats = nullptr;
    int num_cus = 0;
    // ZRT_FLAG_KERNEL_TIMES: an event pair per kernel launch and its class
    std::vector<hipEvent_t> ev_k;
    std::vector<uint8_t> ev_k_cls;
    zrt_kernel_profile prof{};         // of the last render (zrt_context_profile)
    // cached pixel list
    std::vector<uint32_t> pix;
    uint32_t pix_key[5] = {0, 0, 0, 0, 0};
    bool pix_valid = false;
    // zrt_context_reproject: the previous frame's records (2 float4 per pixel:
    // colour + depth; normal + length) and 8 KB of counters of the pixels with
    // history, and a host call's planes in and out (21 words per pixel)
    float4* d_rp = nullptr; size_t rp_cap = 0;
    float* d_rpio = nullptr; size_t rpio_cap = 0;
    // zrt_context_svgf: the filter's records (3 float4 per pixel: colour +
    // variance twice, ping-pong; normal + depth) and 8 KB of counters of the
    // pixels with a temporal variance, and a host call's planes in and out
    // (19 words per pixel; zrt_context_illumination's 12)
    float4* d_sv = nullptr; size_t sv_cap = 0;
    float* d_svio = nullptr; size_t svio_cap = 0;
};

// The accumulator of one rank's share of a frame (zrt_film_*):
// what d_acc is between the passes of one render, kept between calls.
struct zrt_film {
    zrt_context* ctx = nullptr;
    int device = 0;                    // ctx's (zrt_film_destroy does not touch ctx)
    uint32_t w = 0, h = 0, tile = 0, rank = 0, nranks = 0;   // tile, nranks: after their defaults
    uint32_t n_owned = 0;              // pixels of zrt_tile_pixels(w, h, tile, rank, nranks)
    uint32_t samples = 0;              // samples summed so far; 0: d_sum's bits are not read
    float4* d_sum = nullptr;           // n_owned (x, y, z: the f32 sums; w: 0)
    // Adaptive state (zrt_context_refine), allocated by the first
    // refine call.  d_state[q]: x, y, z the checkpoint (the pixel's linear value
    // when the previous refine call started tracing), w the bits kFilmFrozen |
    // n[q] of a frozen pixel, 0 of an active one.
    float4* d_state = nullptr;         // n_owned
    uint32_t* d_list = nullptr;        // the active pixels' image indices, packed order (a call's pixlist)
    uint32_t* d_slot = nullptr;        // ... and their rows in d_sum / d_state
    uint32_t* d_blk = nullptr;         // per compaction block: its active count, then its base; [nblk]: A
    uint32_t* d_cnt = nullptr;         // n_owned sample counts, when a caller asks for them
    size_t cnt_cap = 0;
    uint32_t checkpoint = 0;          // c: the samples the checkpoints were taken at (0: none)
    uint32_t active = 0;               // pixels not frozen (n_owned without state)
    bool state_stale = false;          // d_state holds flags of before a reset / write
    bool list_valid = false;           // d_list / d_slot are the compaction of d_state's flags as they are
};
constexpr uint32_t kFilmFrozen = 0x80000000u;

// A copy on the context's stream, waited for: the product path never uses
// HIP's null stream, whose first use in a process creates its hardware
// queue (~10 ms of the CLI's start-up, r06d)
static hipError_t copy_sync(void* dst, const void* src, size_t n, hipMemcpyKind kind, hipStream_t st) {
    const hipError_t e = hipMemcpyAsync(dst, src, n, kind, st);
    return e != hipSuccess ? e : hipStreamSynchronize(st);
}

// context.hip's for resolve_plan, render.hip's for zrt_device_warmup and for
// denoise.hip's pixel list (hidden: not part of libzrt.so's interface)
#pragma GCC visibility push(hidden)
int rank_pixels(zrt_context* c, const zrt_camera* cam, const zrt_render_config* cfg, uint32_t nranks);
int context_escape(zrt_context* c, bool forced);
int context_bfcull(zrt_context* c, bool forced);
int render_warmup();
#pragma GCC visibility pop
