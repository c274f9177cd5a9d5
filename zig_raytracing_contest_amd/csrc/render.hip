// render.hip -- the render hot path on CDNA4 (gfx950): wavefront path-trace
// kernels + in-order sample resolve, the launch plan and the render, trace and
// radiance entry points of include/zrt.h.  Building a context is context.hip's,
// the parity probes are probe.hip's; render_context.h holds what they share.
//
// Reference: Scene.render / renderWorker / traceRayRecursive / traceRay
// (src/stage3.zig:152-256) over Grid.traceRay + Iterator.next
// (src/linalg.zig:443-496) and Triangle.rayIntersection (linalg.zig:696-722).
//
// Organisation (MI355X-first, not the reference's thread blocks):
//   * a work item is ONE path sample (pixel, sample); items are numbered
//     pixel-major over this rank's packed pixel list (tile_size tiles, 64x64 by
//     default on one device, walked in 8x8 blocks), item = pixel * S + sample of the pass, so one wave64 of
//     the primary launch = 64 samples of one pixel (coherent primary rays)
//     and its records are contiguous;
//   * bounce k of every path of a pass is one launch over a compacted queue
//     of the paths still alive (wavefront organisation); each lane traces one
//     Scene.traceRay segment and shades it (traceRayRecursive's body);
//   * the per-bounce (emissive, albedo) pairs go to HBM planes and the resolve
//     kernel folds them back to front per sample, then sums the samples IN
//     SAMPLE ORDER (renderWorker's `pixel = pixel.add(ray_color)`), scales by
//     the f32 reciprocal of spp and quantizes with toRGB: the image is
//     bit-identical to the recursion's for any scheduling.
#include <new>

#include "render_context.h"
#include "emitters.h"
#include "escape.h"

using namespace zrt;

namespace {

constexpr int kTraceBlock = 512;                     // launch bound of wf_kernel / trace_kernel
constexpr int kTraceThreads = 256;                   // threads per wf_kernel / trace_kernel block
// (r03ze, full spp: 1 -1.3 / -0.6 / -1.5%, 3 -0.6 / -0.2 / -0.6% on cfg3 /
// cfg2 / cfg5; 3 spills inside the primary's cell walk).  Round 6, with the
// entry-face skip testing fewer refs per cell: 1 at 7 waves per SIMD (70
// VGPRs, no spill) against 2 at 6 (r06bi + r06bj, 5 rounds): cfg3 +1.7 /
// -0.05%, cfg2 +2.2 / +1.0%, cfg5 +0.35 / +0.5%; 1 at 6 waves: cfg3 -0.6%
#ifndef ZRT_TRI_BATCH
#define ZRT_TRI_BATCH 1
#endif
constexpr int kTriBatch = ZRT_TRI_BATCH;             // triangle loads in flight per lane
// (3 entries since r05t: 113 VGPRs, which fit beside the park kernel at 96,
// ZRT_PARK_WPE; one-stream shade 18.9 -> 17.1 ms per cfg3 frame)
#ifndef ZRT_SHADE_N
#define ZRT_SHADE_N 3
#endif
constexpr int kShadeEntries = ZRT_SHADE_N;           // wf_shade_kernel: queue entries per lane per fetch
#ifndef ZRT_WF_CHUNK
#define ZRT_WF_CHUNK 3
#endif
// wf_kernel: 64-entry batches per work atomic (r02d1: 2 vs 1 cfg3 +0.35%,
// cfg2 +0.9%, cfg5 +0.2%; 4: +0.6 / +0.5 / 0%; on round 5's final tree 3 vs
// 2: cfg3 6548 / 6540 vs 6489 / 6499 (+0.8%), cfg2 +0.8%, cfg5 +0.1%,
// profiles/r05/r05ay_ab_chunks_lead.log)
constexpr uint32_t kWfChunk = ZRT_WF_CHUNK;

// Triangle positions per ref (bakeInto's Pos: v0, e1 = v1 - v0, e2 = v2 - v0)
// as 3 float4 (48 B, w unused).  36-byte records touch 25% fewer cache lines
// per cell but cost the park kernel 9 VGPRs (r05f: cfg3 -9%).
// A scattering hit's bounce-plane record is (albedo, has emissive) in one
// float4 (16 B, one store) plus a float4 emissive record only when the
// material emits; the alternative, 24 B in two stores (stk4 + a float2 in
// stk2), lost: the lamps are the only emissive materials of the stand-in
// scenes.  r05j, alternating processes, 2 rounds, images identical: cfg3
// 5894 / 5899 vs 5819 / 5812 (+1.4%), cfg5 +1.0%, cfg2 +1.1%; one-stream
// resolve 6.1 -> 4.3 ms per cfg3 frame (profiles/r05/r05j_ab_planes16.log)
//
// The primary walk fast-forwards (DDAV_FFN, dda.h: per axis predicated adds
// and a count, the packed coordinate written once, against a packed step per
// crossing) over the crossings below its pixel block's frustum bound
// (escape.h frustum_bound lo), and stops once it has tested the cell whose
// exit is at or past the block's far bound (hi); cfg3 camera rays cross 85.6
// cells below their block's bound (tools/frustum_sim.cpp), cfg5 75.5, cfg2
// 62.8.
//
// The timed kernels normalise with normalize_rn: 1/length by recip_rn
// (zrt_math.h; the same vector as normalize, bit for bit).
//
// The packed lane walk (primary, lane-walk bounces) on brick-major words
// reads, on entering an occupied brick, the brick's 64-bit cell mask from
// global memory and loads a cell's record only when its own bit is set.
// With the brick bit alone every cell of an occupied brick cost a dependent
// record load and an empty test: cfg3 camera rays walk 44 cells after the
// frustum bound, 18.9 in occupied bricks, 4.2 non-empty (host model,
// tools/frustum_sim.cpp on the bench scenes; cfg5 27.3 / 11.5 / 2.8)
//
// The packed lane walk also skips a cell's refs that the cell it left already
// tested (test_cell_keep), as the park kernel's test rounds do.  The r06aa
// A/B, before the exact cell bits and the counted fast-forward, had it at
// -0.1% (cfg3); on the tree after them (r06af, r06ag, 5 rounds) cfg3 +1.2%,
// cfg5 +0.3%, cfg2 +0.5%, with 6 VGPRs of the 7-wave primary spilled outside
// its walk (6 waves: no spill, cfg3 +0.9%)
//
// The primary / lane-walk wf_kernel sets its walk up with dda_init_fq (dda.h),
// as the park kernel's refill does.
// primary frustum bounds per (1 << ZRT_FRUSTUM_SHIFT)^2 pixel block: 4x4
// since round 6, when the counted fast-forward (DDAV_FFN) made the crossings
// below the bound cheap (r05ae had 8x8 = 4x4 = 2x2 at ~10 VALU per crossing);
// r06ai / r06ak, 5 rounds: cfg3 +0.8 / +0.5%, cfg2 -0.3 / +0.1%, cfg5 0 / +0.1%
#ifndef ZRT_FRUSTUM_SHIFT
#define ZRT_FRUSTUM_SHIFT 2
#endif
constexpr uint32_t kFrustShift = ZRT_FRUSTUM_SHIFT;
static_assert(kFrustShift <= 3, "a frustum block lies inside one tile (tile edges are multiples of 8)");

constexpr double kFrustB = (double)(1u << ZRT_FRUSTUM_SHIFT);
// DDA steps per park walk trip, every cell's brick lookup in flight at once
// (r03h/r03i, full spp: 4 vs 2 cfg3 +2.6%, cfg5 +2.2%, cfg2 -0.2%; 6: cfg3
// +0.4%, cfg5 +4.1%; 8: -8 to -10% everywhere)
#ifndef ZRT_WALK_STEPS
#define ZRT_WALK_STEPS 4
#endif
// the park kernel without the escape table (cfg2, cfg5) at 5 steps: r06ba, 2
// rounds, cfg5 +0.55%, cfg2 +0.4%; with the table 5 steps spill in the walk
// (cfg3 -6.7%) and 6 spill everywhere (cfg5 -8%)
#ifndef ZRT_WALK_STEPS_NOESC
#define ZRT_WALK_STEPS_NOESC 5
#endif

struct TraceParams {
    float bmin[3], bmax[3];
    uint32_t res[3];
    float cs[3];
    float ics[3];             // RN(1 / cs) (host division), for dda_init_fq
    uint32_t cs_ok;           // every cs in [2^-32, 2^32]: dda_init_fq may use ics
    const uint2* cells;
    const float* tri_pos;     // kTriFloats per ref (see kTriFloats)
    const float4* tri_data;   // 4 per ref: n0 n1 n2 uv0 uv1 uv2 mat
    const DevMat* mats;
    uint32_t nmat;
    const float* texels;
    const double* zig;        // zx[257], zf[257]
    const uint32_t* occ;      // brick occupancy bits (brick = 2^occ_shift cells per axis)
    uint32_t occ_shift, occ_nb0, occ_nb01, occ_words;
    // per 4^3 brick in linear brick order (= pc >> 6 of a brick-major word)
    // its 64-bit cell mask (occx_mask_kernel's), for the packed lane walk
    const unsigned long long* bmask;
    // primary launch: per 2^kFrustShift-square pixel block of the image (row-major, tlo_nbx
    // blocks per row) the frustum bounds (lo, hi, unused, unused) of escape.h
    // frustum_bound, or null
    const float4* tlo;
    uint32_t tlo_nbx;
    // packed walks (DdaV): the layout, the cells indexed by the packed word
    // (the cells themselves for power-of-two grids, else a padded copy), the
    // coarse-brick fields of the packed word (offset, width per axis) and
    // their in-brick bits; the 4^3-brick fields for OccX
    PackK pk;
    const uint32_t* cell32;   // 8 u32 per packed cell: begin, end, entry-face masks (see cell32_kernel)
    uint32_t occ_o1, occ_o2, occ_w0, occ_w1, occ_w2, occ_lowm;
    uint32_t ox1, ox2, ow0, ow1, ow2;
    float org[3], llc[3], right[3], up[3];
    uint32_t w;
    const uint32_t* pixlist;
    uint32_t P;               // pixels of this rank
    uint32_t s0;              // first sample index of this pass
    uint32_t total;           // items in this pass: S * P, pixel-major (item = q * S + s)
    uint32_t S;               // samples of every pixel in this pass
    DivS sdiv;                // item / S by multiply and shift (div_magic)
    uint32_t max_bounce;
    uint64_t seed;
    float4* out;              // counting build: sample radiance per item
    uint32_t* counter;
    unsigned long long* stats;   // segments, cells, tests, hits, diagnostics
};

// Ref j's v0, e1, e2.
__device__ __forceinline__ void load_tri(const TraceParams& p, uint32_t j, v3& v0, v3& e1, v3& e2) {
    const float* q = p.tri_pos + (uint64_t)kTriFloats * j;
    const float4 a = *reinterpret_cast<const float4*>(q), b = *reinterpret_cast<const float4*>(q + 4),
                 c = *reinterpret_cast<const float4*>(q + 8);
    v0 = mk(a.x, a.y, a.z); e1 = mk(b.x, b.y, b.z); e2 = mk(c.x, c.y, c.z);
}

// Per-bounce (emissive, albedo) pairs of one path (counting megakernel only).
// The fold reads them back to front: e0 + a0*(e1 + a1*(...)) is
// traceRayRecursive's arithmetic (stage3.zig:219); pass-through bounces
// (stage3.zig:212) add no pair.
template <int N>
struct Stack {
    float e[3 * N], a[3 * N];
    uint32_t used;
    __device__ __forceinline__ void init() { used = 0u; }
    __device__ __forceinline__ void set(uint32_t slot, v3 ee, v3 aa) {
        e[3 * slot] = ee.x; e[3 * slot + 1] = ee.y; e[3 * slot + 2] = ee.z;
        a[3 * slot] = aa.x; a[3 * slot + 1] = aa.y; a[3 * slot + 2] = aa.z;
        used |= 1u << slot;
    }
    __device__ __forceinline__ v3 fold(v3 L) const {
        for (int i = N - 1; i >= 0; --i) {
            if ((used >> i) & 1u) {
                L = add(mk(e[3 * i], e[3 * i + 1], e[3 * i + 2]),
                        mul(mk(a[3 * i], a[3 * i + 1], a[3 * i + 2]), L));
            }
        }
        return L;
    }
};

__device__ __forceinline__ bool brick_occupied(const TraceParams& p, const uint32_t* occ, uint32_t c0,
                                               uint32_t c1, uint32_t c2) {
    const uint32_t s = p.occ_shift;
    const uint32_t b = __umul24(c2 >> s, p.occ_nb01) + __umul24(c1 >> s, p.occ_nb0) + (c0 >> s);   // nb <= 2^24 (context check)
    return (occ[b >> 5] >> (b & 31u)) & 1u;
}

// brick_occupied for a packed cell (DdaV): the brick coordinates are bit
// fields of the word (width 0 when a brick spans the whole axis)
// (brick-major words: the occupancy bricks are 4^3, context_packed, so the
// brick is the word's high part)
template <bool BM>
__device__ __forceinline__ bool brick_occupied_v(const TraceParams& p, const uint32_t* occ, uint32_t pc) {
    if (BM) {
        return __builtin_amdgcn_ubfe(occ[pc >> 11], pc >> 6, 1u);
    }
    const uint32_t b = __umul24(__builtin_amdgcn_ubfe(pc, p.occ_o2, p.occ_w2), p.occ_nb01) +
                       __umul24(__builtin_amdgcn_ubfe(pc, p.occ_o1, p.occ_w1), p.occ_nb0) +
                       __builtin_amdgcn_ubfe(pc, p.occ_shift, p.occ_w0);
    return (occ[b >> 5] >> (b & 31u)) & 1u;
}

// The in-brick cell index k = x | y << 2 | z << 4 of a packed cell: one
// 24-bit multiply of the fields' low two bits sums them, shifted into place
// (pack_layout picks the multiplier and checks every in-brick cell), and the
// 64-bit shift reads only k[5:0].  (6 VALU; 9 with the fields moved by shifts
// and masks.)
template <bool BM>
__device__ __forceinline__ bool occx_cell(unsigned long long bm, const DdaV& s, const PackK& k) {
    if (BM) return (uint32_t)(bm >> (s.pc & 63u)) & 1u;   // (brick-major: the word's low six bits)
    const uint32_t i = __umul24(s.pc & k.low2, k.kmul) >> k.kshr;
    return (uint32_t)(bm >> (i & 63u)) & 1u;
}

// Grid constants as wave-uniform registers (see GridK).
__device__ __forceinline__ GridK grid_consts(const TraceParams& p) {
    GridK g;
    g.rm0 = __builtin_amdgcn_readfirstlane(p.res[0] - 1u);
    g.rm1 = __builtin_amdgcn_readfirstlane(p.res[1] - 1u);
    g.rm2 = __builtin_amdgcn_readfirstlane(p.res[2] - 1u);
    g.str1 = __builtin_amdgcn_readfirstlane(p.res[0]);
    g.str2 = __builtin_amdgcn_readfirstlane(p.res[0] * p.res[1]);
    return g;
}

__device__ __forceinline__ bool first_active_lane() {
    return (threadIdx.x & 63u) == (uint32_t)__builtin_ctzll(__ballot(1));
}

// All triangles of one cell in reference order (stage3.zig:164-178), TB at
// a time: the TB loads are issued before the first test so their latencies
// overlap (one memory round trip per TB triangles instead of per triangle).
template <int TB, bool STATS, bool MTX = false>
__device__ __forceinline__ void test_cell(const TraceParams& p, uint32_t b, uint32_t e, v3 o, v3 d,
                                          float& nearest, float& hu, float& hv, uint32_t& hidx,
                                          uint32_t& n_tests, uint64_t* wstat) {
    for (uint32_t i = b; i < e; i += TB) {
        if (STATS && first_active_lane()) ++wstat[1];   // wave trips of this loop
        v3 A[TB], B[TB], Cc[TB];
#pragma unroll
        for (int k = 0; k < TB; ++k) load_tri(p, min(i + (uint32_t)k, e - 1u), A[k], B[k], Cc[k]);
#pragma unroll
        for (int k = 0; k < TB; ++k) {
            if (i + (uint32_t)k < e) {
                if (STATS) ++n_tests;
                float t, u, v;
                if (tri_ray<MTX>(A[k], B[k], Cc[k], o, d, &t, &u, &v)) {
                    if (nearest > t && t > 0.0f) { nearest = t; hu = u; hv = v; hidx = i + k; }
                }
            }
        }
    }
}

// test_cell for the packed walk's cells, with the entry-face skip of the
// park kernel's test rounds (cell32_kernel): `keep` is the mask of the cell's
// refs (bit k: ref b + k) still to test for the face the ray entered across,
// all ones for a segment's first cell or cells above 32 refs.  A skipped ref
// is bit-identical to one of the cell the ray just left, already tested
// there, so the kept refs give the same nearest hit, in the same order.
template <int TB, bool MTX>
__device__ __forceinline__ void test_cell_keep(const TraceParams& p, uint32_t b, uint32_t e, uint32_t keep, v3 o,
                                               v3 d, float& nearest, float& hu, float& hv, uint32_t& hidx) {
    const uint32_t cnt = e - b;
    if (cnt > 32u || keep == ~0u) {
        uint32_t dummy = 0;
        test_cell<TB, false, MTX>(p, b, e, o, d, nearest, hu, hv, hidx, dummy, nullptr);
        return;
    }
    uint32_t m = keep & ((cnt < 32u ? (1u << cnt) : 0u) - 1u);
    while (m) {
        uint32_t k[TB];
        bool has[TB];
#pragma unroll
        for (int j = 0; j < TB; ++j) {
            has[j] = m != 0u;
            k[j] = has[j] ? (uint32_t)__builtin_ctz(m) : k[0];
            m &= m - 1u;
        }
        v3 A[TB], B[TB], Cc[TB];
#pragma unroll
        for (int j = 0; j < TB; ++j) load_tri(p, b + k[j], A[j], B[j], Cc[j]);
#pragma unroll
        for (int j = 0; j < TB; ++j) {
            if (has[j]) {
                float t, u, v;
                if (tri_ray<MTX>(A[j], B[j], Cc[j], o, d, &t, &u, &v)) {
                    if (nearest > t && t > 0.0f) { nearest = t; hu = u; hv = v; hidx = b + k[j]; }
                }
            }
        }
    }
}

// Scene.traceRay (stage3.zig:152-186) with empty-space skipping that changes
// nothing in the result: the DDA arithmetic runs for every cell exactly as
// Iterator.next does; only the 8-byte Cell load is skipped when the cell's
// brick holds no triangle (its range would be empty).
// STATS (counting build): n_cells / n_tests per lane; prof[] per wave:
// [6] cell loads, [7] non-empty cells, [8] wave trips of the cell loop,
// [9] wave trips of the triangle-batch loop, [10] cell trips with any test,
// [4] 64-wide rounds if each trip's tests were shared evenly.
// PACKED: the walk state with the cell packed into one word (DdaV, grids of
// at most 1024 cells per axis; same cells, same order, same t_exit), which
// also indexes the cell records (cell32).
// TAU (packed walk): a frustum bound (escape.h frustum_bound lo) for this ray: the
// crossings below it enter only empty cells; +inf: the ray meets no
// occupied cell at all.
// NEAREST0 (segment queries, zrt_context_segments): the value nearest_hit.t
// starts at (stage3.zig:154), +inf for every other caller; nothing else of
// the walk changes.  The return value is bit-equal to it exactly when no ref
// was kept (a kept t is below it, and nothing is below or above a NaN).
// BOUNDED is set with it (the code for it is compiled into no other caller).
// ANY: the walk also ends after the first cell in which a ref was kept.
template <bool STATS, int TB, bool PACKED = false, bool PK_BM = false, bool MTX = false, bool ANY = false,
          bool BOUNDED = false>
__device__ __forceinline__ float trace_ray(const TraceParams& p, const uint32_t* occ, v3 o, v3 d,
                                           float& hu, float& hv, uint32_t& hidx, uint32_t& n_cells,
                                           uint32_t& n_tests, uint64_t* prof, uint32_t* wcnt = nullptr,
                                           float tau = 0.0f, float tfar = kInf, const float nearest0 = kInf) {
    float nearest = nearest0;
    Dda s0;
    // (the counting build and the IEEE-division kernels keep dda_init's
    // divisions; the timed kernels take dda_init_fq's quotients: same state)
    if (!MTX && !STATS) {
        if (!dda_init_fq(p.bmin, p.bmax, p.res, p.cs, p.ics, p.cs_ok != 0u, o, d, s0)) return nearest;
    } else if (!dda_init(p.bmin, p.bmax, p.res, p.cs, o, d, s0)) {
        return nearest;
    }
    const uint32_t sh = p.occ_shift;
    const GridK gk = grid_consts(p);
    if constexpr (PACKED) {
        static_assert(!STATS, "the counting build walks unpacked");
        DdaV s;
        ddav_from_t<PK_BM>(s0, gk, p.pk, s);
        // the field masks as laundered registers: selected straight from the
        // kernel arguments they became a vector load at a selected offset
        // (v_cndmask of 0x94/0x98/0x9c, global_load_dword, vmcnt(0)) in
        // every step (r03 ISA)
        uint32_t f0 = p.pk.f0, f1 = p.pk.f1, f2 = p.pk.f2;
        asm("" : "+s"(f0), "+s"(f1), "+s"(f2));
        if (s0.neg < 8u) {
            // the cells before tau are empty (the pixel block's frustum bound):
            // their crossings as plain adds, the walk's exact state after them
            // (DDAV_FFN); nearest is +inf here, so no break test fires among them
            if (tau == kInf) return nearest;               // no occupied cell on the ray: the miss
            if (tau > fminf(s.tn0, fminf(s.tn1, s.tn2))) {
                bool exited;
                // (four branch-free crossings per loop trip: r04s, cfg3 5730 vs
                // 5695 Mrays/s with one per trip)
                DDAV_FFN(s, p.pk, f0, f1, f2, tau, exited);
                if (exited) return nearest;
            }
        }
        bool occupied = brick_occupied_v<PK_BM>(p, occ, s.pc);
        unsigned long long q = 0ull;        // PK_BM: the current brick's cell mask
        if (PK_BM && occupied) q = p.bmask[s.pc >> 6];
        // the walk's stop: the nearest hit so far, or (TFAR, a frustum far
        // bound) the t past which every cell of the ray is empty
        float lim = s0.neg < 8u ? tfar : kInf;
        // (a bounded segment stops at its bound from the first cell on, empty
        // cells included; never true for nearest0 = +inf or NaN)
        if constexpr (BOUNDED) {
            if (nearest0 < lim) lim = nearest0;
        }
        // the entry-face skip: the crossing t of the step into the current
        // cell (NaN: the segment's first tested cell, every ref tested)
        float tcl = __builtin_nanf("");
        for (;;) {
            if (PK_BM ? ((q >> (s.pc & 63u)) & 1ull) != 0ull : occupied) {
                const uint32_t* rec = p.cell32 + 8ull * s.pc;
                const uint2 cell = *reinterpret_cast<const uint2*>(rec);
                // the face entered: the stepped axis a is the one whose
                // next crossing is this step's own tc + td_a; exactly one
                // such axis, or (a tie at tc) every ref is tested
                const bool x0 = s.tn0 == tcl + s.td0, x1 = s.tn1 == tcl + s.td1, x2 = s.tn2 == tcl + s.td2;
                uint32_t keep = ~0u;
                if ((uint32_t)x0 + (uint32_t)x1 + (uint32_t)x2 == 1u) {
                    const uint32_t face = x0 ? (s.d0 >> 31) : (x1 ? 2u + (s.d1 >> 31) : 4u + (s.d2 >> 31));
                    keep = rec[2 + face];
                }
                test_cell_keep<TB, MTX>(p, cell.x, cell.y, keep, o, d, nearest, hu, hv, hidx);
                lim = fminf(lim, nearest);                 // = min(nearest, far bound)
            }
            bool crossed, exited;
            float tc;
            PackK pkl = p.pk;
            pkl.f0 = f0; pkl.f1 = f1; pkl.f2 = f2;
            DDAV_STEPX(s, pkl, p.occ_lowm, crossed, exited, tc);
            if (exited || lim <= tc) break;                // stage3.zig:179-182 (T_EXIT = +inf at the exit)
            if (ANY && __float_as_uint(nearest) != __float_as_uint(nearest0)) break;   // a ref was kept
            tcl = tc;
            if (crossed) {
                occupied = brick_occupied_v<PK_BM>(p, occ, s.pc);
                if (PK_BM) q = occupied ? p.bmask[s.pc >> 6] : 0ull;
            }
        }
        return nearest;
    }
    DdaW s;
    ddaw_from(s0, gk, s);
    bool occupied = brick_occupied(p, occ, s.c0, s.c1, s.c2);
    for (;;) {
        if (STATS) ++n_cells;
        if (STATS && first_active_lane()) ++prof[8];
        uint32_t ncell = 0;
        if (occupied) {
            const uint2 cell = p.cells[s.lin];
            if (STATS) { prof[6] += 1; prof[7] += cell.y > cell.x ? 1 : 0; ncell = cell.y - cell.x; }
            test_cell<TB, STATS, MTX>(p, cell.x, cell.y, o, d, nearest, hu, hv, hidx, n_tests, prof + 8);
        }
        if (STATS) {
            // wave-shared work of this trip: sum of the lanes' triangle counts
            uint32_t* wc = wcnt + 2 * (threadIdx.x >> 6);
            const bool first = first_active_lane();
            if (first) wc[0] = 0;
            __builtin_amdgcn_wave_barrier();
            atomicAdd(&wc[0], ncell);
            __builtin_amdgcn_wave_barrier();
            if (first) {
                const uint32_t N = wc[0];
                prof[10] += N ? 1 : 0;
                prof[4] += (N + 63) / 64;
            }
        }
        bool crossed;
        float t_exit;
        DDAW_STEP(s, sh, crossed, t_exit);
        if (nearest <= t_exit) break;                      // stage3.zig:179-182
        if (ANY && __float_as_uint(nearest) != __float_as_uint(nearest0)) break;       // a ref was kept
        // a NaN bound makes no comparison true, the one with T_EXIT = +inf
        // included, which ends every other walk at the grid's exit: there the
        // step out of the exit cell itself (the stepped axis's cell index left
        // [0, res - 1], in either direction mod 2^32) ends it
        if constexpr (BOUNDED) {
            if (nearest0 != nearest0 && (s.c0 > gk.rm0 || s.c1 > gk.rm1 || s.c2 > gk.rm2)) break;
        }
        if (crossed) occupied = brick_occupied(p, occ, s.c0, s.c1, s.c2);
    }
    return nearest;
}

// renderWorker: camera.getRay(x + U, y + U) (stage3.zig:238, :27-35) for
// pass item `item` (= packed pixel * S + s_local: pixel-major, so one
// pixel's samples are consecutive items and a wave's records are
// contiguous); leaves rng after the jitter.
__device__ __forceinline__ void camera_ray(const TraceParams& p, uint32_t item, Rng& rng, v3& o, v3& d,
                                           uint32_t* block = nullptr) {
    const uint32_t q = div_by(item, p.sdiv);
    const uint32_t s_local = item - q * p.S;
    const uint32_t pixel = p.pixlist[q];
    const uint32_t py = pixel / p.w;
    const uint32_t px = pixel - py * p.w;
    if (block) *block = (py >> kFrustShift) * p.tlo_nbx + (px >> kFrustShift);
    rng.s = path_key(p.seed, pixel, p.s0 + s_local);
    const float jx = rng_float(rng);
    const float jy = rng_float(rng);
    o = mk(p.org[0], p.org[1], p.org[2]);
    d = normalize_rn(add(add(mk(p.llc[0], p.llc[1], p.llc[2]),
                            scale(mk(p.right[0], p.right[1], p.right[2]), (float)px + jx)),
                        scale(mk(p.up[0], p.up[1], p.up[2]), (float)py + jy)));
}

// The RNG state camera_ray leaves (after the jitter draws), without the ray.
__device__ __forceinline__ Rng camera_rng(const TraceParams& p, uint32_t item) {
    const uint32_t q = div_by(item, p.sdiv);
    const uint32_t s_local = item - q * p.S;
    const uint32_t pixel = p.pixlist[q];
    Rng rng;
    rng.s = path_key(p.seed, pixel, p.s0 + s_local);
    (void)rng_float(rng);
    (void)rng_float(rng);
    return rng;
}

// The counting megakernel: renderWorker's per-sample body (stage3.zig:237-241)
// + traceRayRecursive (stage3.zig:188-220) made iterative, one lane = one
// path from camera to sky, with exact per-lane work counters (segments,
// cells, triangle tests, hits).  Same RNG -> same paths as the timed
// wavefront kernels, so its counts are the timed frame's algorithmic work
// (bench.py's roofline) and the parity tests' traversal counters.
template <int MAXB>
__global__ __launch_bounds__(kTraceBlock, 1) void trace_kernel(const TraceParams p) {
    __shared__ double s_zig[514];
    extern __shared__ __attribute__((aligned(16))) uint32_t s_occ[];
    uint64_t prof[11] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    __shared__ uint32_t s_wcnt[2 * (kTraceBlock / 64)];
    for (uint32_t i = threadIdx.x; i < 514; i += blockDim.x) s_zig[i] = p.zig[i];
    for (uint32_t i = threadIdx.x; i < p.occ_words; i += blockDim.x) s_occ[i] = p.occ[i];
    __syncthreads();
    const double* zx = s_zig;
    const double* zf = s_zig + 257;

    const uint32_t lane = threadIdx.x & 63u;
    uint32_t n_seg = 0, n_cells = 0, n_tests = 0, n_hits = 0;
    uint32_t p_seg = 0, p_cells = 0, p_tests = 0, p_hits = 0;   // the primary (camera) segments' share

    for (;;) {
        uint32_t base = 0;
        if (lane == 0) base = atomicAdd(p.counter, 64u);
        base = __builtin_amdgcn_readfirstlane(base);
        if (base >= p.total) break;
        const uint32_t item = base + lane;
        if (item >= p.total) continue;

        Rng rng;
        v3 o, d;
        camera_ray(p, item, rng, o, d);
        Stack<MAXB> stk;
        stk.init();
        v3 L = mk(0, 0, 0);
        uint32_t slot = 0;
        for (uint32_t depth = p.max_bounce; depth > 0; --depth, ++slot) {
            ++n_seg;
            float hu = 0.0f, hv = 0.0f;
            uint32_t hidx = 0;
            const uint32_t c_before = n_cells, t_before = n_tests;
            // (the plain IEEE division in Moller-Trumbore: the counting build is
            // the timed kernels' checker and serves every scene, mt_inv_det)
            const float t = trace_ray<true, kTriBatch, false, false, true>(p, s_occ, o, d, hu, hv, hidx, n_cells,
                                                                           n_tests, prof, s_wcnt);
            if (slot == 0) { ++p_seg; p_cells += n_cells - c_before; p_tests += n_tests - t_before; }
            if (t == kInf) { L = env_color(d); break; }       // stage3.zig:195-197
            ++n_hits;
            if (slot == 0) ++p_hits;
            // stage3.zig:199-206
            const float4* tdp = p.tri_data + 4ull * hidx;
            const float4 d0 = tdp[0], d1 = tdp[1], d2 = tdp[2], d3 = tdp[3];
            const float w0 = 1.0f - hu - hv;
            const float tc0 = (d2.y * w0 + d2.w * hu) + d3.y * hv;
            const float tc1 = (d2.z * w0 + d3.x * hu) + d3.z * hv;
            const DevMat& m = p.mats[__float_as_uint(d3.w)];
            const v3 albedo = sample3(p.texels, m.tex[0], tc0, tc1);
            const v3 emissive = sample3(p.texels, m.tex[1], tc0, tc1);
            const float transparency = sample1(p.texels, m.tex[2], tc0, tc1);
            const v3 nrm = add(add(scale(mk(d0.x, d0.y, d0.z), w0), scale(mk(d0.w, d1.x, d1.y), hu)),
                               scale(mk(d1.z, d1.w, d2.x), hv));
            const v3 no = add(o, scale(d, t + kFltEps));        // ray.at(hit.t + eps)
            if (!(rng_float(rng) > transparency)) {             // stage3.zig:207
                // randomUnitVector (linalg.zig:140-148): 3 x floatNorm, normalize
                const float nx = (float)rng_norm64(rng, zx, zf);
                const float ny = (float)rng_norm64(rng, zx, zf);
                const float nz = (float)rng_norm64(rng, zx, zf);
                d = normalize(add(nrm, normalize(mk(nx, ny, nz))));
                stk.set(slot, emissive, albedo);                // stage3.zig:214-219
            }                                                   // else pass-through :208-212
            o = no;
        }
        L = stk.fold(L);
        p.out[item] = make_float4(L.x, L.y, L.z, 0.0f);
    }
    const unsigned long long s0 = wave_sum(n_seg), s1 = wave_sum(n_cells), s2 = wave_sum(n_tests),
                             s3 = wave_sum(n_hits), s4 = wave_sum(prof[6]), s5 = wave_sum(prof[7]),
                             s6 = wave_sum(prof[8]), s7 = wave_sum(prof[9]), s8 = wave_sum(prof[10]),
                             s9 = wave_sum(prof[4]);
    const unsigned long long q0 = wave_sum(p_seg), q1 = wave_sum(p_cells), q2 = wave_sum(p_tests),
                             q3 = wave_sum(p_hits);
    if (lane == 0) {
        atomicAdd(&p.stats[8], q0);
        atomicAdd(&p.stats[9], q1);
        atomicAdd(&p.stats[10], q2);
        atomicAdd(&p.stats[11], q3);
        atomicAdd(&p.stats[0], s0);
        atomicAdd(&p.stats[1], s1);
        atomicAdd(&p.stats[2], s2);
        atomicAdd(&p.stats[3], s3);
        atomicAdd(&p.stats[4], s4);
        atomicAdd(&p.stats[5], s5);
        atomicAdd(&p.stats[6], s6);
        atomicAdd(&p.stats[7], s7);
        atomicAdd(&p.stats[14], s8);
        atomicAdd(&p.stats[15], s9);
    }
}

// ---------------------------------------------------------------------------
// Wavefront organisation: one launch per bounce over a compacted queue of
// live paths.
//
// A megakernel keeps a lane on one path from camera to sky, so a wave lives
// as long as its longest path.  Here bounce k is its own launch over the
// paths still alive after bounce k-1: every lane traces one segment and
// shades it; a continuing path is appended to the next queue (one returning
// atomic per wave and region, ballot + popcount ranks), a finished one
// stores its terminal radiance (env / 0) and the mask of bounce slots that
// scattered.  The per-bounce (emissive, albedo) pairs go to HBM in
// [slot][item] planes and wf_resolve_kernel folds them back to front.
// Items are pixel-major (item = packed pixel * S + sample of the pass).
//
// A queue record is 48 B: (o.xyz, item) (d.xyz, depth | slot << 16)
// (rng lo, rng hi, mask, 0).
//
// XCD split: blocks are dispatched round-robin over the 8 XCDs, so block
// group g = blockIdx % 8 shares one L2.  The packed pixel list is cut into 8
// ranges (8x8-block aligned) and every queue into 8 regions, region g holding
// the paths of pixel range g (capacity S * P_g).  Group g takes pixel range
// g / region g first, then helps the other groups: a screen region's paths
// stay on one XCD from bounce to bounce.  Same items, other order: same image.
struct WfParams {
    TraceParams t;
    const float4* q_in;
    float4* q_out;
    float4* stk4;             // bounce planes, slot-major: float4 (a, emissive bits != 0) at [slot * T + item]
    float2* stk2;             //   and float4 records e at [slot * T + item], written for emissive
                              //   hits only (still declared float2*, two per record: the type is
                              //   part of wf_resolve_kernel's symbol name)
    float4* term;             // [item]: terminal L.xyz, scatter mask bits
    uint32_t T;               // items in this pass
    uint32_t esc_key;         // escape table (below): its shape (escape.h esc_walk_key; 0: a word
                              //   group per brick).  In T's padding, so that no other field moves
    uint32_t* fetch8;         // work counter per group of this launch
    const uint32_t* n_in8;    // paths per region of q_in
    uint32_t* n_out8;         // paths per region of q_out
    float4* hit;              // split launches: [entry] (t, u, v, ref) of the segment just traced
    uint32_t* fetch8s;        // split launches: work counter per group of the shade kernel
    // wf_park_kernel: exact per-cell occupancy blob (see OccX) and schedule
    const uint32_t* occx;
    uint32_t occx_words, occx_nbw, occx_moff, occx_nb0, occx_nb01;
    uint32_t occx_ldsw;       // u32 words OccX takes in LDS (multiple of 4): entries + masks
    uint32_t test_min;        // parked lanes before a wave runs a test round
    uint32_t refill_min;      // finished lanes before a wave shades and refills
    uint32_t rel_min;         // park release: a round with fewer parked lanes with refs is skipped (0: off)
    uint32_t rel_emin;        //   ... if at least this many parked lanes have none
    uint32_t hop;             // refs of a cell at most whose record's hop bits a lane uses (kHopMaxRefs; 0: no hop)
    // escape table (escape.h): kEscWords u32 per region of a 4^3 brick, a
    // brick's regions together (esc_key), bit b of word w = direction bin
    // 32 w + b; null: not built (the walk never stops early)
    const uint32_t* esc;
    // back-face cull masks (escape.h): kBfcNBin u32 per packed cell word, then
    // one all-ones word; null: the first cell of a segment tests every ref
    const uint32_t* bfc;
    uint64_t bfc_ones;        // index of the all-ones word (cells x kBfcNBin)
};

// Work / append counters: one per 128-byte line (32 u32), so the waves'
// atomics on different counters do not queue on one line (packed counters
// made the region queues 2.4x slower, round 1).
constexpr uint32_t kCtr = 32;

// XCD split: first pixel (packed order) of group g, 8x8-block aligned.
__device__ __forceinline__ uint32_t xcd_q0(uint32_t P, uint32_t g) {
    const uint32_t nblk = (P + 63u) >> 6;
    return min(P, (nblk * g / 8u) * 64u);
}

// First queue entry of region g: S * (the first pixel of pixel range g).
__device__ __forceinline__ uint32_t region_base(const WfParams& w, uint32_t g) { return w.t.S * xcd_q0(w.t.P, g); }

// traceRayRecursive's body after the hit (stage3.zig:195-219) for one
// segment: env colour on a miss, else material lookup, (e, a) pair to the
// bounce planes on a scatter, pass-through otherwise.  Returns true when the
// path continues (o, d, depth, slot, rng, mask updated); false with L set
// when it terminates.
// `mats`: the material descriptors (p.mats, or the shade kernel's LDS copy).
// `sp` (ZRT_SWEEP builds, the shade kernel only): per-wave s_memtime cycles
// and active lanes of the phases (SHADE_STAMP), else null.
#ifdef ZRT_SWEEP
// phase k: cycles into sp[k], active lanes into sp[8 + k]; sp[16] the last
// tick.  `sp` is the wave's row in LDS, updated by the first active lane, so
// a stamp inside a divergent branch (the hit path) counts for the wave
// whichever lanes run it.  `v`: a value the phase produced, so the stamp
// waits for it.
#define SHADE_STAMP(k, v) do { if (sp) { asm volatile("" :: "v"(v)); const uint64_t t_ = __builtin_amdgcn_s_memtime(); \
    const uint32_t n_ = (uint32_t)__popcll(__ballot(1)); \
    if (first_active_lane()) { sp[k] += t_ - sp[16]; sp[16] = t_; sp[8 + (k)] += n_; } } } while (0)
#else
#define SHADE_STAMP(k, v) do { (void)sp; } while (0)
#endif
// The hit triangle's Data record (stage3.zig:199-206: normals, uvs, material),
// loaded by the caller so that a lane shading several entries can issue every
// entry's load before the first entry's texel loads (r05c: -4% shade time
// alone, but the kernel no longer fits beside the park kernel).
struct TriRec {
    float4 d0, d1, d2, d3;
};
__device__ __forceinline__ TriRec tri_rec(const TraceParams& p, float t, uint32_t hidx) {
    TriRec r;
    if (t == kInf) {
        r.d0 = r.d1 = r.d2 = r.d3 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        return r;
    }
    const float4* tdp = p.tri_data + 4ull * hidx;
    r.d0 = tdp[0]; r.d1 = tdp[1]; r.d2 = tdp[2]; r.d3 = tdp[3];
    return r;
}
// LAST: the segment is the path's last (depth 1, the last bounce launch):
// traceRayRecursive at depth 1 returns e + a * (the depth-0 call's 0) on a
// scatter and 0 on a pass-through (stage3.zig:188-219), so the terminal
// radiance is e + a * 0 itself -- the resolve's fold step add(e, mul(a, L))
// at L = 0, the same f32 operations, with e = +0 exactly when the material
// emits nothing -- and no bounce plane, scatter bit, normal draws (the
// ziggurat) or queue append is needed.
template <bool LAST = false>
__device__ __forceinline__ bool shade_segment(const WfParams& w, const double* zx, const double* zf,
                                              const DevMat* mats, uint32_t item, float t, float hu, float hv,
                                              const TriRec& tr, v3& o, v3& d, uint32_t& depth, uint32_t& slot,
                                              Rng& rng, uint32_t& mask, v3& L,
                                              unsigned long long* sp = nullptr) {
    SHADE_STAMP(1, t);                                      // the hit record landed
    if (t == kInf) { L = env_color(d); return false; }     // stage3.zig:195-197
    const TraceParams& p = w.t;
    const float4 d0 = tr.d0, d1 = tr.d1, d2 = tr.d2, d3 = tr.d3;   // stage3.zig:199-206
    const float w0 = 1.0f - hu - hv;
    const float tc0 = (d2.y * w0 + d2.w * hu) + d3.y * hv;
    const float tc1 = (d2.z * w0 + d3.x * hu) + d3.z * hv;
    SHADE_STAMP(2, tc1);                                    // triangle data
    const DevMat& m = mats[__float_as_uint(d3.w)];
    const v3 albedo = sample3(p.texels, m.tex[0], tc0, tc1);
    const v3 emissive = sample3(p.texels, m.tex[1], tc0, tc1);
    const float transparency = sample1(p.texels, m.tex[2], tc0, tc1);
    SHADE_STAMP(3, transparency);                           // material + texels
    const v3 nrm = add(add(scale(mk(d0.x, d0.y, d0.z), w0), scale(mk(d0.w, d1.x, d1.y), hu)),
                       scale(mk(d1.z, d1.w, d2.x), hv));
    const v3 no = add(o, scale(d, t + kFltEps));
    const float u_tr = rng_float(rng);
    SHADE_STAMP(4, u_tr);                                   // transparency draw
    if (LAST) {
        // the fold's last step at L = 0 (e = +0 exactly when no
        // e was stored, i.e. when every bit of the sampled e is zero: then
        // the sample is that +0)
        L = !(u_tr > transparency) ? add(emissive, mul(albedo, mk(0.0f, 0.0f, 0.0f))) : mk(0, 0, 0);
        return false;
    }
    if (!(u_tr > transparency)) {                           // stage3.zig:207, :214-219
        // the (e, a) pair goes out before the normal draws, so the ziggurat
        // (f64, 64-bit RNG) runs without the six colour registers live.
        // (a, has_e) in 16 B; e only for emissive hits (its own plane).  (24 B
        // per pair beat two float4 in r03zk: cfg3 +0.5%, cfg2 +1.6%, cfg5
        // +1.3%: this write and wf_resolve_kernel's read are HBM-bound; the
        // 16 B record beat the 24 B one in r05j, at the top of this file)
        const uint32_t eb = __float_as_uint(emissive.x) | __float_as_uint(emissive.y) | __float_as_uint(emissive.z);
        w.stk4[(uint64_t)slot * w.T + item] = make_float4(albedo.x, albedo.y, albedo.z, __uint_as_float(eb));
        if (eb != 0u)
            reinterpret_cast<float4*>(w.stk2)[(uint64_t)slot * w.T + item] =
                make_float4(emissive.x, emissive.y, emissive.z, 0.0f);
        const float nx = (float)rng_norm64(rng, zx, zf);
        const float ny = (float)rng_norm64(rng, zx, zf);
        const float nz = (float)rng_norm64(rng, zx, zf);
        d = normalize_rn(add(nrm, normalize_rn(mk(nx, ny, nz))));
        mask |= 1u << slot;
        SHADE_STAMP(5, d.x);                                // pair store + ziggurat draws
    }
    o = no;
    --depth;
    ++slot;
    L = mk(0, 0, 0);
    return depth != 0;                                      // depth 0: recursion returns 0
}

__device__ __forceinline__ void q_store(const WfParams& w, uint32_t pos, v3 o, v3 d, uint32_t item, uint32_t depth,
                                        uint32_t slot, const Rng& rng, uint32_t mask) {
    w.q_out[3ull * pos] = make_float4(o.x, o.y, o.z, __uint_as_float(item));
    w.q_out[3ull * pos + 1] = make_float4(d.x, d.y, d.z, __uint_as_float(depth | (slot << 16)));
    w.q_out[3ull * pos + 2] = make_float4(__uint_as_float((uint32_t)rng.s), __uint_as_float((uint32_t)(rng.s >> 32)),
                                          __uint_as_float(mask), 0.0f);
}

// Append the continuing paths of the wave (lanes with `cont`) to the next
// queue, each to the region `reg` of its pixel range: one returning atomic
// per distinct region of the wave, ranks from ballot + popcount.
__device__ __forceinline__ void wf_append(const WfParams& w, bool cont, uint64_t below, v3 o, v3 d, uint32_t item,
                                          uint32_t depth, uint32_t slot, const Rng& rng, uint32_t mask,
                                          uint32_t reg) {
    uint64_t pend = __ballot(cont);
    while (pend) {
        const uint32_t lead = (uint32_t)__builtin_ctzll(pend);
        const uint32_t g = (uint32_t)__builtin_amdgcn_readlane((int)reg, (int)lead);
        const uint64_t m = __ballot(cont && reg == g);
        uint32_t ob = 0;
        if ((threadIdx.x & 63u) == lead) ob = atomicAdd(&w.n_out8[g * kCtr], (uint32_t)__popcll(m));
        ob = (uint32_t)__builtin_amdgcn_readlane((int)ob, (int)lead) + region_base(w, g);
        if (cont && reg == g) q_store(w, ob + (uint32_t)__popcll(m & below), o, d, item, depth, slot, rng, mask);
        pend &= ~m;
    }
}

// Fetch work for a wave from the XCD group queues, group `grp` first: one
// returning atomic takes `want` consecutive entries of group grp's range
// (primary launch: items of pixel range g for every sample of the pass;
// bounce launches: region g of q_in).  Returns false once every group is
// exhausted.  On true, entries [base, min(base + want, lim)) of group grp
// belong to this wave; entry j maps to the item / queue index of ent_index().
template <bool PRIMARY>
__device__ __forceinline__ bool wf_fetch(const WfParams& w, uint32_t want, uint32_t& grp, uint32_t& tried,
                                         uint32_t& base, uint32_t& lim) {
    const TraceParams& p = w.t;
    const uint32_t S = p.S;
    for (;;) {
        const uint32_t q0 = xcd_q0(p.P, grp);
        const uint32_t pg = xcd_q0(p.P, grp + 1u) - q0;
        lim = PRIMARY ? S * pg : w.n_in8[grp * kCtr];
        uint32_t b = 0;
        if ((threadIdx.x & 63u) == 0) b = atomicAdd(&w.fetch8[grp * kCtr], want);
        base = __builtin_amdgcn_readfirstlane(b);
        if (base < lim) return true;
        if (++tried == 8u) return false;
        grp = (grp + 1u) & 7u;
    }
}
// Primary launch: entry j of group g is sample j % S of pixel q0 + j / S
// (pixel-major), so a wave traces 64 samples of one pixel (or all S samples
// of 64 / S neighbouring pixels in the packed 8x8-block order): rays that
// stay within one pixel's footprint walk the same cells and test the same
// triangles side by side.  Against 64 pixels of one sample (8x8 blocks,
// sample-major) the primary launch took 17.0 vs 22.4-23.2 ms at cfg3 64 spp
// (r02at: cfg3 +6.3%, cfg5 +3.6%, cfg2 +0.5%).  Since r04 the item number
// (what term / the bounce planes / the resolve index) is pixel-major too,
// item = S * pixel + sample = S * q0 + j: a wave's terminal and bounce-pair
// stores are contiguous (sample-major, its 64 lanes stored 64 lines P items
// apart: 126 B of DRAM writes per primary item for <= 72 B of records, r03zm).
// Bounce launches: entry j of region g is queue index S * q0 + j.
template <bool PRIMARY>
__device__ __forceinline__ uint32_t ent_index(const WfParams& w, uint32_t grp, uint32_t j) {
    return region_base(w, grp) + j;
}

// The path state of queue entry / primary item `i` that shading needs.
template <bool PRIMARY>
__device__ __forceinline__ void path_state(const WfParams& w, uint32_t i, uint32_t& item, uint32_t& depth,
                                           uint32_t& slot, Rng& rng, uint32_t& mask) {
    if (PRIMARY) {
        item = i;
        depth = w.t.max_bounce;
        slot = 0;
        mask = 0;
        rng = camera_rng(w.t, i);
    } else {
        const float4 a = w.q_in[3ull * i], b = w.q_in[3ull * i + 1], c = w.q_in[3ull * i + 2];
        item = __float_as_uint(a.w);
        depth = __float_as_uint(b.w) & 0xFFFFu;
        slot = __float_as_uint(b.w) >> 16;
        rng.s = ((uint64_t)__float_as_uint(c.y) << 32) | __float_as_uint(c.x);
        mask = __float_as_uint(c.z);
    }
}

// wf_kernel: one lane = one segment, walked and tested by the lane itself.
// MTX: Moller-Trumbore with the plain IEEE division (mt_inv_det), for the
// scenes whose edges leave the short reciprocal's domain (zrt_context::mt_exact).
template <int MINW, bool PRIMARY, bool PACKED, bool PK_BM = false, bool MTX = false>
__global__ __launch_bounds__(kTraceBlock, MINW) void wf_kernel(const WfParams w) {
    const TraceParams& p = w.t;
    __shared__ double s_zig[514];
    extern __shared__ __attribute__((aligned(16))) uint32_t s_occ[];
    for (uint32_t i = threadIdx.x; i < 514; i += blockDim.x) s_zig[i] = p.zig[i];
    for (uint32_t i = threadIdx.x; i < p.occ_words; i += blockDim.x) s_occ[i] = p.occ[i];
    __syncthreads();
    const double* zx = s_zig;
    const double* zf = s_zig + 257;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t below = lane ? (~0ull >> (64u - lane)) : 0ull;
    uint32_t n_seg = 0, dummy = 0;
    uint32_t grp = blockIdx.x & 7u, tried = 0;
#ifdef ZRT_SWEEP
    // ZRT_SWEEP builds: per-wave s_memtime cycles of the walk (camera ray +
    // traceRay), the shading (+ terminal store) and the fetch + append
    unsigned long long wprof[3] = {0, 0, 0};
    uint64_t wtick = __builtin_amdgcn_s_memtime();
#define WF_STAMP(k) do { const uint64_t t_ = __builtin_amdgcn_s_memtime(); wprof[k] += t_ - wtick; wtick = t_; } while (0)
#else
#define WF_STAMP(k) do { } while (0)
#endif

    for (;;) {
        uint32_t base = 0, lim = 0;
        if (!wf_fetch<PRIMARY>(w, 64u * kWfChunk, grp, tried, base, lim)) break;
      for (uint32_t sub = 0; sub < kWfChunk && base + 64u * sub < lim; ++sub) {
        const uint32_t j = base + 64u * sub + lane;
        const bool valid = j < lim;
        const uint32_t i = valid ? ent_index<PRIMARY>(w, grp, j) : 0u;
        bool cont = false;
        uint32_t mask = 0, r_item = 0, r_depth = 0, r_slot = 0;
        v3 r_o = mk(0, 0, 0), r_d = mk(0, 0, 0);
        Rng r_rng;
        r_rng.s = 0;
        if (valid) {
            // the ray only: the rest of the path's state (item, slot, RNG,
            // mask) is re-read after the walk, so it holds no VGPRs in it
            v3 o, d;
            uint32_t depth;
            float tau = 0.0f, tfar = kInf;
            if (PRIMARY) {
                Rng rng0;
                uint32_t blk = 0;
                camera_ray(p, i, rng0, o, d, &blk);
                if (p.tlo) {
                    const float4 fb = p.tlo[blk];
                    tau = fb.x;
                    tfar = fb.y;
                }
                depth = p.max_bounce;
            } else {
                const float4 a = w.q_in[3ull * i], b = w.q_in[3ull * i + 1];
                o = mk(a.x, a.y, a.z);
                d = mk(b.x, b.y, b.z);
                depth = __float_as_uint(b.w) & 0xFFFFu;
            }
            float t = kInf, hu = 0.0f, hv = 0.0f;
            uint32_t hidx = 0;
            WF_STAMP(2);
            if (depth != 0)
                t = trace_ray<false, kTriBatch, PACKED, PK_BM, MTX>(p, s_occ, o, d, hu, hv, hidx, dummy, dummy, nullptr,
                                                                    nullptr, tau, tfar);
            WF_STAMP(0);
            uint32_t item, slot;
            Rng rng;
            path_state<PRIMARY>(w, i, item, depth, slot, rng, mask);
            v3 L = mk(0, 0, 0);
            if (depth != 0) {
                ++n_seg;
                cont = shade_segment(w, zx, zf, p.mats, item, t, hu, hv, tri_rec(p, t, hidx), o, d, depth, slot, rng,
                                     mask, L);
            }
            if (!cont) w.term[item] = make_float4(L.x, L.y, L.z, __uint_as_float(mask));
            r_item = item; r_depth = depth; r_slot = slot; r_o = o; r_d = d; r_rng = rng;
            WF_STAMP(1);
        }
        wf_append(w, cont, below, r_o, r_d, r_item, r_depth, r_slot, r_rng, mask, grp);
        WF_STAMP(2);
      }
    }
    const unsigned long long s0 = wave_sum(n_seg);
    if (lane == 0) atomicAdd(&p.stats[0], s0);
#ifdef ZRT_SWEEP
    if (PRIMARY && lane == 0)
        for (int k = 0; k < 3; ++k) atomicAdd(&p.stats[29 + k], wprof[k]);
#endif
#undef WF_STAMP
}

// ---------------------------------------------------------------------------
// wf_park_kernel: Scene.traceRay as walk / park / test rounds with exact
// per-cell occupancy in LDS: the bounce launches' kernel.
//
// Counted on the contest stand-in (cfg3, round 1): a segment visits 85
// cells, 4.3 of them non-empty, and tests 18.2 triangles; per wave the
// per-lane triangle loop ran 134 two-triangle trips for 9.1 per lane (6.8%
// of the lanes busy) and the walk 184 trips for 85 steps per lane.  Here:
//  * the exact occupancy of every cell sits in LDS (OccX), so a lane loads a
//    cell's [begin, end) only when the cell holds triangles, and the walk of
//    empty cells is DDA arithmetic plus one LDS lookup per 4^3 brick entered;
//  * a lane that reaches a non-empty cell issues the range load and PARKS
//    (its load is in flight while the others walk on);
//  * once `test_min` lanes are parked (or none walks) the wave runs one test
//    round: the (parked lane, triangle) pairs of all parked lanes are laid
//    out in lane order and tested 64 at a time, one pair per lane; each
//    parked lane keeps the lexicographic min of (t, ref) over its pairs with
//    0 < t < nearest -- exactly what the reference's in-order
//    `nearest > t and t > 0` loop keeps (stage3.zig:164-178: the smallest t,
//    the first ref among equal t; t > 0 orders like its bit pattern) -- and
//    walks on from that cell;
//  * finished lanes wait until `refill_min` of them are done, then write
//    their hit records (t, u, v, ref) together and take fresh paths from the
//    wave's chunk of the queue (persistent waves, dynamic fetch);
//    wf_shade_kernel then shades the hit records with whole waves
//    (traceRayRecursive's body, stage3.zig:195-219) and appends.
// Per lane the cells, the tests, their order semantics and the break test
// after every cell (stage3.zig:179-182) are the reference's: same hit.
//
// OccX (4^3-cell bricks): one bit per brick, 1 + the u16 number of
// occupied bricks before each 32-brick word, the zero mask, then one 64-bit
// cell mask per occupied brick.
// In LDS each 32-brick word sits beside its prefix as one 8-byte entry, so a
// lookup is two dependent LDS reads: (bits, prefix), then the mask.  The
// mask index is (1 + prefix + occupied bricks below b in the word) x (b's
// bit): an empty brick reads the zero mask at index 0, so nothing is
// selected after the load (5 VALU from the entry to the mask address,
// against 11 with the loaded mask zeroed by selects; the bit-field
// extracts use the hardware's 5-bit offset/width, so b needs no & 31).
struct OccX {
    const uint2* ent;                    // (brick bits, 1 + occupied bricks before the word)
    const unsigned long long* masks;     // [0]: zero mask
};
__device__ __forceinline__ unsigned long long occx_mask_at(const OccX& L, uint2 e, uint32_t b) {
    const uint32_t low = __builtin_amdgcn_ubfe(e.x, 0u, b);        // bits of the bricks below b
    const uint32_t bit = __builtin_amdgcn_ubfe(e.x, b, 1u);
    return L.masks[__umul24((uint32_t)__popc(low) + e.y, bit)];
}

__device__ __forceinline__ unsigned long long occx_mask(const OccX& L, uint32_t b) {
    return occx_mask_at(L, L.ent[b >> 5], b);
}
// occx_mask for a brick index that may lie past the grid (a speculative
// step beyond the exit cell): the word index is clamped into the blob, so
// the read stays inside it; the result of such a lookup is never used
__device__ __forceinline__ unsigned long long occx_mask_clamped(const OccX& L, uint32_t b, uint32_t nbw) {
    return occx_mask_at(L, L.ent[min(b >> 5, nbw - 1u)], b);
}
// occx_mask for a brick-major word (no clamp: the word stays inside the
// grid's packed range).  Laundering pc >> 11 saves the compiler's third
// address VALU ((pc >> 8) & ~7 + base) but measured neutral (r05al:
// cfg3 -0.2%, cfg2 / cfg5 +0.5%)
__device__ __forceinline__ unsigned long long occx_mask_bm(const OccX& L, uint32_t pc) {
    return occx_mask_at(L, L.ent[pc >> 11], pc >> 6);
}
// The 4^3 brick of a packed cell (DdaV): its coordinates are the fields'
// bits above their low two.  24-bit multiplies (full rate; v_mul_lo_u32 is
// quarter rate), exact because OccX serves only grids of at most 2^24
// bricks (occx_usable).
template <bool BM>
__device__ __forceinline__ uint32_t occx_brick(const WfParams& w, const DdaV& s) {
    if (BM) return s.pc >> 6;                              // (brick-major: the brick's linear index)
    const TraceParams& p = w.t;
    return __umul24(__builtin_amdgcn_ubfe(s.pc, p.ox2, p.ow2), w.occx_nb01) +
           __umul24(__builtin_amdgcn_ubfe(s.pc, p.ox1, p.ow1), w.occx_nb0) + __builtin_amdgcn_ubfe(s.pc, 2u, p.ow0);
}

// A parked lane's cell range [begin, end) is loaded by LDS-DMA into its
// wave's slots (begin at rng[lane], end at rng[64 + lane]): the load writes
// no VGPR, so the walk loop that keeps stepping the other lanes never waits
// on it (a VGPR destination made the compiler put a vmcnt(0) in the walk:
// its address registers doubled as the previous step's load destination,
// r02k ISA).  Nothing orders an LDS read behind a pending LDS-DMA but the
// wave's own vmcnt, so the test round drains vmcnt(0) before reading them.
#ifndef ZRT_PARK_CHUNK
#define ZRT_PARK_CHUNK 256
#endif
// queue entries per work atomic of a park wave (r02d0, two pass sets: 128 vs
// 64 cfg3 +0.8%, cfg2 +1.1%, cfg5 +0.3%; 32 -2%; 256 +1.0 / -0.1 / +0.5%;
// r03za, on the round-3 kernels: 256 vs 128 cfg3 +0.5%, cfg5 +0.4%, cfg2
// -0.5%; 64 -0.7 / -1.0 / -0.5%)
constexpr uint32_t kParkChunk = ZRT_PARK_CHUNK;
// A launch with few entries per wave (the last bounces, an 8-rank tile set)
// takes smaller chunks, down to 64, so the waves' last chunks end closer
// together (the launch tail).  r05e, alternating processes, 2 rounds, images
// identical: cfg3 5801 / 5810 vs 5765 / 5749 (+0.8%) against fixed chunks,
// cfg2 +0.6%, cfg5 +0.1% (profiles/r05/r05e_ab_p96_park_adapt.log)
// Park release (round 6): a parked lane whose cell has no ref left to test
// for the face it entered across (the entry-face mask is 0: every ref was
// tested in the cell it left) costs a test round nothing but its latency,
// and 54% of the parks on cfg3 are such (r06n).  Once a round's ranges have
// landed, a round with fewer than `rel_min` parked lanes that have refs to
// test is not run while lanes still walk: the empty ones walk on (what the
// round would have done with them), the others stay parked for the next
// round.  The context turns it on for scenes where enough of the occupied
// cells' entry faces have empty masks (context_release; ZRT_FLAG_RELEASE /
// ZRT_FLAG_NO_RELEASE force it): images identical either way.
//
// Issued by inline asm, not the builtin: the compiler treats an LDS-DMA like
// a store whose VGPR operands are read late, so whenever the register
// allocator reuses the address registers inside the walk it guards the reuse
// with a vmcnt(0) there -- every step then waits for the range load just
// issued (r02p ISA: the two-step walk got one after a register shuffle).
// The address is read when the instruction issues; the only consumer of the
// data is the test round, behind its explicit vmcnt(0), and the kernel drains
// vmcnt before it ends.  M0 cannot be declared clobbered (a reserved
// register: the clobber is ignored), so nothing else in the park kernel may
// rely on it: tests/test_codegen.py checks that every M0 access in its code
// object is this sequence.
// Range only (the segment's first cell: no cell was left, every ref is
// tested; the caller writes the all-ones mask itself).
__device__ __forceinline__ void park_load_range(const TraceParams& p, uint32_t pc, uint32_t* rng) {
    const uint32_t* c = p.cell32 + 8ull * pc;
    const uint32_t m0 = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)rng);
    // (an instruction offset would move the LDS destination too: the end
    // word gets its own address)
    asm volatile("s_mov_b32 m0, %2\n\t"
                 "global_load_lds_dword %0, off\n\t"
                 "s_add_u32 m0, m0, 0x100\n\t"
                 "global_load_lds_dword %1, off"
                 :
                 : "v"(c), "v"(c + 1), "s"(m0)
                 : "memory");
}
// Range and the mask of the refs to test for a ray that entered the cell
// across `face` (cell32_kernel) into rng[lane], rng[64 + lane], rng[128 + lane].
// Range and one mask word (`mask`: any u32 in global memory) into the same slots.
__device__ __forceinline__ void park_load_masked(const TraceParams& p, uint32_t pc, const uint32_t* mask,
                                                 uint32_t* rng) {
    const uint32_t* c = p.cell32 + 8ull * pc;
    const uint32_t m0 = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)rng);
    asm volatile("s_mov_b32 m0, %3\n\t"
                 "global_load_lds_dword %0, off\n\t"
                 "s_add_u32 m0, m0, 0x100\n\t"
                 "global_load_lds_dword %1, off\n\t"
                 "s_add_u32 m0, m0, 0x100\n\t"
                 "global_load_lds_dword %2, off"
                 :
                 : "v"(c), "v"(c + 1), "v"(mask), "s"(m0)
                 : "memory");
}
__device__ __forceinline__ void park_load_cell(const TraceParams& p, uint32_t pc, uint32_t face, uint32_t* rng) {
    park_load_masked(p, pc, p.cell32 + 8ull * pc + 2 + face, rng);
}

// The escape-table word of a walking lane's current brick into its wave's
// escape slot esc[lane] (same LDS-DMA as park_load_range: no VGPR is written,
// the walk never waits for it; the lane reads the slot at the next trips,
// and a word for an earlier brick of the same ray is as valid as the current
// one: every cell after it lies on the ray further on).
__device__ __forceinline__ void park_load_esc(const uint32_t* word, uint32_t* esc) {
    const uint32_t m0 = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)esc);
    asm volatile("s_mov_b32 m0, %1\n\t"
                 "global_load_lds_dword %0, off"
                 :
                 : "v"(word), "s"(m0)
                 : "memory");
}

// Exclusive prefix sum over the wave (the whole wave must be active: every
// DPP read below runs under full EXEC).  Row scans by DPP row_shr with
// bound_ctrl (a source lane outside the row reads 0), rows joined through
// their last lanes.  NOT written as `rl >= k ? dpp(x) : 0`: that puts the
// DPP read under a partial EXEC, and gfx9 DPP treats a disabled source lane
// as invalid (tools/dpp_probe.hip; the cause of round 1's park-mode fault).
__device__ __forceinline__ uint32_t wave_excl_sum(uint32_t x, uint32_t lane, uint32_t& total) {
    uint32_t s = x;
    s += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)s, 0x111, 0xf, 0xf, true);   // row_shr:1
    s += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)s, 0x112, 0xf, 0xf, true);   // row_shr:2
    s += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)s, 0x114, 0xf, 0xf, true);   // row_shr:4
    s += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)s, 0x118, 0xf, 0xf, true);   // row_shr:8
    const uint32_t r0 = (uint32_t)__builtin_amdgcn_readlane((int)s, 15);
    const uint32_t r1 = (uint32_t)__builtin_amdgcn_readlane((int)s, 31);
    const uint32_t r2 = (uint32_t)__builtin_amdgcn_readlane((int)s, 47);
    const uint32_t r3 = (uint32_t)__builtin_amdgcn_readlane((int)s, 63);
    const uint32_t row = lane >> 4;
    s += row == 0u ? 0u : (row == 1u ? r0 : (row == 2u ? r0 + r1 : r0 + r1 + r2));
    total = r0 + r1 + r2 + r3;
    return s - x;
}

// ZRT_SWEEP builds only: per-wave s_memtime cycles of the three rounds and
// their activity (printed by zrt_context_render as zrt_park_profile; the
// stamps cost ~10% and never run in the product build).
#ifdef ZRT_SWEEP
#define PARK_PROF_DECL unsigned long long pprof[23] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}; \
    uint64_t ptick = __builtin_amdgcn_s_memtime();
#define PARK_STAMP(k) do { const uint64_t t_ = __builtin_amdgcn_s_memtime(); pprof[k] += t_ - ptick; ptick = t_; } while (0)
#define PARK_COUNT(k, v) (pprof[k] += (v))
#else
#define PARK_PROF_DECL
#define PARK_STAMP(k) do { } while (0)
#define PARK_COUNT(k, v) do { } while (0)
#endif

// The hop (one-cell lookahead): two parks in three find nothing to test on
// cfg3 (r10e) -- the cell's refs were all tested in the cell the ray just
// left -- and each such park is directly preceded by a park in that adjacent
// cell.  The earlier cell's record says so (its hop bits, context.hip
// cell32_hop_kernel), and a lane walking on from a parked cell reads them from
// its own landed mask word, behind the round's vmcnt(0).  It keeps, in `hm`,
// the field masks of the axes along which its next step may pass through the
// cell it enters (the hop bit of that axis's face, by the lane's own step
// sign); the lane's next trip then ignores the occupancy of its first step's
// cell if that step ran along such an axis.  The axis is read off the stepped
// word (pc ^ previous pc lies inside one field), so ties step as DDAV_STEPM
// steps them, and nothing else of the trip changes: a first step that leaves
// the grid or passes `nearest` ends the segment as before, the hopped cell's
// own break test (nearest <= its exit t) runs at the second step as for an
// empty cell, the escape query and `prev` see an ordinary walked cell.  Hits,
// ties and break tests are the reference's.
// hm is 0 except between a lane's release from a parked cell and its next
// trip, which clears it (a lane parks, finishes or idles only from a trip or
// a refill, so it is 0 whenever a lane starts a segment).
// Against committing one DDAV_STEPM step at the release (45 VALU per round and
// release, about as many of those as trips): DESIGN 5.2e.
// GO: the lane walks on from its parked cell; HB: its record's hop bits.
#define PARK_HOP(GO, HB)                                                                          \
    do {                                                                                          \
        PARK_COUNT(22, __popcll(__ballot(GO)));                                                   \
        if (__ballot((GO) && (HB) != 0u) != 0ull) {                                               \
            const uint32_t hb_ = (HB), hb1_ = hb_ >> 1;       /* bit 2a: toward plus, 2a + 1: minus */ \
            const uint32_t e0_ = lm_selu(lm_of((int32_t)s.d0 < 0), hb1_, hb_);                    \
            const uint32_t e1_ = lm_selu(lm_of((int32_t)s.d1 < 0), hb1_, hb_);                    \
            const uint32_t e2_ = lm_selu(lm_of((int32_t)s.d2 < 0), hb1_, hb_);                    \
            const uint32_t m_ = ((uint32_t)__builtin_amdgcn_sbfe((int32_t)e0_, 0, 1) & fv0) |     \
                                ((uint32_t)__builtin_amdgcn_sbfe((int32_t)e1_, 2, 1) & fv1) |     \
                                ((uint32_t)__builtin_amdgcn_sbfe((int32_t)e2_, 4, 1) & fv2);      \
            hm = lm_selu(lm_of(GO), m_, hm);                                                      \
        }                                                                                         \
    } while (0)

// ZRT_PARK_WPE: the park kernel compiled for 5 waves per SIMD (at most 96
// VGPRs; it still runs 4, one 1024-thread workgroup per CU), so 4 x 96 leave
// 128 VGPRs per SIMD lane for a shade wave of 3 entries per lane (113) or a
// primary wave (80) of the other pass set.  r05t, 2 rounds, images identical:
// with ZRT_SHADE_N 3, cfg3 6014 / 6034 vs 6011 / 6017, cfg2 3902 / 3897 vs
// 3878 / 3838, cfg5 3584 / 3590 vs 3582 / 3594 (profiles/r05/r05t_ab_park96_shade3.log)
#ifndef ZRT_PARK_WPE
#define ZRT_PARK_WPE 5
#endif
#if ZRT_PARK_WPE
#define ZRT_PARK_ATTR __attribute__((amdgpu_waves_per_eu(ZRT_PARK_WPE, 8)))
#else
#define ZRT_PARK_ATTR
#endif
// ESC: with the escape table (context_escape decides per scene); PK_BM:
// brick-major packed words (dda.h)
// QM, the query mode: kParkRender, a render's and zrt_context_trace's
// segments (nearest starts at +inf); kParkClosest, the bounded segments of
// zrt_context_segments: nearest starts at the queue record's second .w word
// (the bound; a render keeps the depth there and this kernel never used it)
// and the hit record's ref starts at 0xFFFFFFFF, which no baked ref is, so a
// miss shows in the record whatever the bound was.  Any-hit calls run this
// mode too and keep the record's yes / no: a third mode, in which a parked lane
// whose test round kept a candidate was done at once, answered the same and
// was not faster (measured and dropped).
// What the kernel skips stays valid for any initial nearest, because each
// skip drops only refs or cells that cannot produce a KEPT hit at all:
//  * entry-face masks: the skipped ref was tested, with the same ray and so
//    the same t, in the cell just left; not kept there (t >= nearest or
//    t <= 0) it is not kept here, nearest only falls;
//  * cull masks: the skipped ref fails Moller-Trumbore's determinant test for
//    every direction of the bin: no t at all, whatever nearest is;
//  * the escape stop: no cell further along the ray holds a ref, so no test
//    follows and the hit so far, or the miss, stands;
//  * the park release only delays lanes with nothing to test.
constexpr int kParkRender = 0, kParkClosest = 1;
template <bool ESC, bool PK_BM, int QM = kParkRender>
__global__ __launch_bounds__(kParkBlock) ZRT_PARK_ATTR void wf_park_kernel(const WfParams w) {
    const TraceParams& p = w.t;
    extern __shared__ __attribute__((aligned(16))) uint32_t s_dyn[];
    __shared__ uint32_t s_rng[kParkWaves * 192];            // LDS-DMA range + mask slots
    uint32_t* const rng_slot = s_rng + 192u * (threadIdx.x >> 6);
    __shared__ uint32_t s_esc[kParkWaves * 64];             // escape-table words (park_load_esc)
    uint32_t* const esc_slot = s_esc + 64u * (threadIdx.x >> 6);
    __shared__ uint8_t s_sel8[256 * 8];                     // bit position of the r-th set bit of a byte
    for (uint32_t i = threadIdx.x; i < 256u * 8u; i += blockDim.x) {
        SEL8_ENTRY(i, pos);
        s_sel8[i] = (uint8_t)pos;
    }
    // OccX into LDS: (bits, prefix) entries, then the masks
    {
        const uint16_t* pre = reinterpret_cast<const uint16_t*>(w.occx + w.occx_nbw);
        uint2* ent = reinterpret_cast<uint2*>(s_dyn);
        for (uint32_t i = threadIdx.x; i < w.occx_nbw; i += blockDim.x) ent[i] = make_uint2(w.occx[i], pre[i]);
        for (uint32_t i = threadIdx.x; i < w.occx_words - w.occx_moff; i += blockDim.x)
            s_dyn[2 * w.occx_nbw + i] = w.occx[w.occx_moff + i];
    }
    __syncthreads();
    OccX L;
    L.ent = reinterpret_cast<const uint2*>(s_dyn);
    L.masks = reinterpret_cast<const unsigned long long*>(s_dyn + 2 * w.occx_nbw);
    ParkSlot& W = reinterpret_cast<ParkSlot*>(s_dyn + w.occx_ldsw)[threadIdx.x >> 6];

    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t test_min = w.test_min, refill_min = w.refill_min, rel_min = w.rel_min;
    const uint32_t hop_max = w.hop;        // cells of at most this many refs carry hop bits (PARK_HOP); 0: no hop
    const GridK gk = grid_consts(p);
    constexpr uint32_t kIdle = 0, kWalk = 1, kPark = 2, kDone = 3;
    uint32_t st = kIdle;
    bool more = true;
    uint32_t grp = blockIdx.x & 7u, tried = 0;
    uint32_t cb = 0, ce = 0, cgrp = 0;     // the wave's current chunk of queue entries
    uint32_t chunk = kParkChunk;
    {                                      // (wave-uniform: the previous launch's final counts)
        uint32_t ntot = 0;
        for (uint32_t g = 0; g < 8u; ++g) ntot += w.n_in8[g * kCtr];
        const uint32_t per = ntot / (gridDim.x * (blockDim.x >> 6) * 4u);
        chunk = __builtin_amdgcn_readfirstlane(max(64u, min(kParkChunk, per & ~63u)));
    }
    // the segment: ray, DDA state, best hit, range
    v3 o = mk(0, 0, 0), d = mk(0, 0, 0);
    DdaV s;                                // grids of <= 1024 cells per axis (zrt_context_render)
    const PackK pk = p.pk;
    uint32_t fv0 = pk.f0, fv1 = pk.f1, fv2 = pk.f2;        // field masks in VGPRs (DDAV_STEPM)
    asm("" : "+v"(fv0), "+v"(fv1), "+v"(fv2));
    memset(&s, 0, sizeof s);
    float nearest = kInf, hu = 0.0f, hv = 0.0f;
    uint32_t hidx = 0;
    uint32_t qi = 0;                       // the path's queue entry
    // the ray's escape-table word (byte offset in a brick's kEscWords) and
    // bit; emask 0: the ray never stops early (no table, or a -inf / NaN
    // crossing sequence)
    uint32_t eoff = 0, emask = 0;
    uint32_t eb = ~0u;                     // the brick of the lane's last escape-table query
    uint32_t hm = 0;                       // the hop's field masks (PARK_HOP)
    // the table's shape (escape.h esc_walk_key), wave-uniform
    const uint32_t esc_key = ESC ? __builtin_amdgcn_readfirstlane(w.esc_key) : 0u;
    const uint32_t esc_lg = esc_key & 0xFFu, esc_mlo = (esc_key >> 8) & 0xFFu, esc_mhi = esc_key >> 16;
    PARK_PROF_DECL

    for (;;) {
        // ---- hit records + refill round, once enough lanes are finished or idle
        const uint64_t busy = __ballot(st == kWalk || st == kPark);
        if ((uint32_t)(64 - __popcll(busy)) >= refill_min || busy == 0ull) {
            PARK_COUNT(8, 1);
            PARK_COUNT(9, __popcll(__ballot(st == kDone)));
            if (__ballot(st == kDone) != 0ull) {
                // the hit record for wf_shade_kernel; its stores are drained
                // before the walk (at the end of this round): otherwise the
                // compiler guards the walk loop's reuse of their data registers
                // with a vmcnt(0) INSIDE the loop, which then also waits for
                // the previous step's range load, every step (r02f ISA; walk
                // 1304 cycles per step)
                const bool done = st == kDone;
                if (done) {
                    w.hit[qi] = make_float4(nearest, hu, hv, __uint_as_float(hidx));
                    st = kIdle;
                }
            }
            bool loaded = false;                                   // (wave-uniform)
            PARK_STAMP(10);
            // idle lanes take entries of the wave's chunk [cb, ce) of group
            // cgrp, a new chunk of kParkChunk entries once it is used up: one
            // returning atomic per chunk instead of one per refill round
            uint64_t idle = __ballot(st == kIdle);
            while (idle != 0ull && (ce > cb || more)) {
                if (cb == ce) {
                    uint32_t base = 0, lim = 0;
                    more = wf_fetch<false>(w, chunk, grp, tried, base, lim);
                    PARK_STAMP(11);
                    if (!more) break;
                    cb = base;
                    ce = min(base + chunk, lim);
                    cgrp = grp;
                }
                const uint32_t take = min((uint32_t)__popcll(idle), ce - cb);
                // the idle lanes below this one (mbcnt: no per-lane 64-bit mask
                // held in a VGPR pair over the walk trips)
                const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(idle >> 32),
                                                                __builtin_amdgcn_mbcnt_lo((uint32_t)idle, 0u));
                if (st == kIdle && rank < take) {
                    {
                        qi = ent_index<false>(w, cgrp, cb + rank);
                        float bound = kInf;                        // (a query's: the record's second .w)
                        {
                            const float4 qa = w.q_in[3ull * qi], qb = w.q_in[3ull * qi + 1];
                            o = mk(qa.x, qa.y, qa.z);
                            d = mk(qb.x, qb.y, qb.z);
                            if (QM != kParkRender) bound = qb.w;
                        }
                        {                                          // queued paths have depth >= 1
                            nearest = bound;
                            hu = hv = 0.0f;
                            hidx = QM != kParkRender ? 0xFFFFFFFFu : 0u;
                            W.o[lane] = make_float4(o.x, o.y, o.z, 0.0f);
                            W.d[lane] = make_float4(d.x, d.y, d.z, 0.0f);
                            Dda s0;
                            // stage3.zig:153-156
                            if (dda_init_fq(p.bmin, p.bmax, p.res, p.cs, p.ics, p.cs_ok != 0u, o, d, s0)) {
                                ddav_from_t<PK_BM>(s0, gk, pk, s);
                                const uint32_t bin = (ESC || w.bfc) ? esc_dir_bin(d) : 0u;
                                if (ESC) {
                                    // (every DMA into this slot from the lane's last
                                    // ray has landed before this store: that ray's
                                    // escape DMAs were issued before this refill's
                                    // q_in loads, vector memory completes in order
                                    // (vmcnt), and this store runs only after
                                    // dda_init consumed o and d, i.e. after the
                                    // compiler's wait for those loads.  No kDone
                                    // drain sits between them (it comes after the
                                    // refill); the parity suite renders every scene
                                    // with the table forced on)
                                    eoff = (bin >> 5) * 4u;
                                    // (a direction outside bfc_cull's domain never
                                    // uses a bit: the direction-aware table's cone
                                    // argument, escape.h)
                                    emask = w.esc && esc_ray_usable(s0.neg, d) ? 1u << (bin & 31u) : 0u;
                                    eb = ~0u;
                                    esc_slot[lane] = 0u;
                                }
                                if (occx_cell<PK_BM>(occx_mask(L, occx_brick<PK_BM>(w, s)), s, pk)) {
                                    if (w.bfc) {
                                        // first cell: no cell was left, so no entry-face
                                        // mask; the refs that the ray's direction bin
                                        // cannot reject by their determinant alone
                                        // (escape.h bfc_cull; every ref for a direction
                                        // outside the proof's domain).  The lane's last
                                        // DMA into this slot was drained by the test
                                        // round that let its last ray leave its last cell
                                        const uint64_t wi = bfc_dir_ok(d) ? (uint64_t)s.pc * kBfcNBin + bfc_bin_of(bin)
                                                                          : w.bfc_ones;
                                        park_load_masked(p, s.pc, w.bfc + wi, rng_slot);
                                    } else {
                                        park_load_range(p, s.pc, rng_slot);
                                        rng_slot[128 + lane] = ~0u;    // first cell: every ref
                                    }
                                    st = kPark;
                                } else {
                                    st = kWalk;
                                }
                            } else {
                                st = kDone;                        // misses the grid: nearest = +inf
                            }
                        }
                    }
                }
                PARK_STAMP(12);
                cb += take;
                loaded = loaded || take != 0u;
                idle = __ballot(st == kIdle);
            }
            // the hit-record stores drain with the new paths' record loads
            // (vector memory completes in order); only a round that loaded
            // nothing drains them explicitly (vmcnt(0)).  Against a drain
            // right after the stores: r05q, 2 rounds, images identical: cfg5
            // 3576 / 3587 vs 3551 / 3553 (+0.8%, park -1%), cfg3 +0.1%, cfg2
            // +0.5% (profiles/r05/r05q_ab_park_late_drain.log)
            if (!loaded) __builtin_amdgcn_s_waitcnt(0x3f70);
            // No prefetch of the chunk's next 64 queue entries here.  Pulling
            // their lines into L2 at the end of a refill round (one LDS-DMA
            // dword per lane into a per-wave slot that nothing reads, so that
            // the next round's record loads hit L2 instead of HBM; the walk
            // trips that follow do not wait for vector memory) lost: r06ab, 2
            // rounds, images identical: cfg3 6972 vs 6992 (-0.3%), cfg2 -0.4%,
            // cfg5 3845 vs 3892 (-1.2%)
            // (profiles/r06/r06ab_ab_queue_prefetch.log): the extra request
            // per lane and refill costs more than the record loads' HBM
            // latency, which the SIMD's other park waves already hide
            PARK_STAMP(0);
            if (__ballot(st != kIdle) == 0ull) {
                if (!more) break;
                continue;
            }
        }
        // ---- walk until test_min lanes are parked or nobody walks
        for (;;) {
            const uint64_t wk = __ballot(st == kWalk);
            if (wk == 0ull || (uint32_t)__popcll(__ballot(st == kPark)) >= test_min) break;
            PARK_COUNT(3, 1);
            PARK_COUNT(4, __popcll(wk));
            if (st == kWalk) {
                // ZRT_WALK_STEPS DDA steps per trip, every cell's lookup in
                // flight before any is used; the trip ends in the first cell
                // that ends the segment or holds triangles (steps after it
                // are speculative and dropped; their lookups read a clamped
                // brick).  Every boolean of the trip is a lane mask and every
                // select one v_cndmask on it (DDAV_STEPM: 179 VALU and no
                // branch per four-step trip, against 202 VALU, 14 v_mov and
                // four execz branches with per-lane booleans, r03p)
                constexpr int kS = ESC ? ZRT_WALK_STEPS : ZRT_WALK_STEPS_NOESC;
                static_assert(kS >= 2, "the trip keeps the cell before its last step");
                // the escape words landed so far (used at the trip's end, so the
                // read's latency hides behind the trip)
                const uint32_t ew = ESC ? esc_slot[lane] & emask : 0u;
                DdaV ss[kS];
                LaneM ex[kS], stop[kS], dd[kS];
                float te[kS];
                unsigned long long q[kS];
#pragma unroll
                for (int k = 0; k < kS; ++k) {
                    ss[k] = k ? ss[k - 1] : s;
                    DDAV_STEPM(ss[k], fv0, fv1, fv2, ex[k], te[k]);
                }
#pragma unroll
                // (brick-major words never leave the grid's packed range, pk_add
                // wraps inside a field, so their speculative lookups need no clamp)
                for (int k = 0; k < kS; ++k)
                    q[k] = PK_BM ? occx_mask_bm(L, ss[k].pc)
                                 : occx_mask_clamped(L, occx_brick<PK_BM>(w, ss[k]), w.occx_nbw);
#pragma unroll
                for (int k = 0; k < kS; ++k) asm volatile("" : "+v"(q[k]));
#pragma unroll
                for (int k = 0; k < kS; ++k) {
                    dd[k] = lm_or(ex[k], lm_of(nearest <= te[k]));
                    stop[k] = lm_or(dd[k], lm_of(occx_cell<PK_BM>(q[k], ss[k], pk)));
                }
                {   // the hop (PARK_HOP): the first step's cell is passed through if
                    // the step ran along an axis of hm
                    // (sweep builds count the hops here, where only walking lanes are
                    // active: like the trip's other counters, the wave's count is kept
                    // only if its lane 0 walks)
                    const LaneM hop = lm_of(((ss[0].pc ^ s.pc) & hm) != 0u);
                    PARK_COUNT(21, __popcll(lm_and(hop, lm_andn(stop[0], dd[0]))));
                    stop[0] = lm_or(dd[0], lm_andn(stop[0], hop));
                    hm = 0u;
                }
                // the first stopping step wins: from the last step back (the
                // last step's selects are identities)
                DdaV sel = ss[kS - 1];
                uint32_t prev = ss[kS - 2].pc;
                LaneM pkd = lm_andn(stop[kS - 1], dd[kS - 1]), dn = dd[kS - 1];
#pragma unroll
                for (int k = kS - 2; k >= 0; --k) {
                    sel.tn0 = lm_sel(stop[k], ss[k].tn0, sel.tn0);
                    sel.tn1 = lm_sel(stop[k], ss[k].tn1, sel.tn1);
                    sel.tn2 = lm_sel(stop[k], ss[k].tn2, sel.tn2);
                    sel.pc = lm_selu(stop[k], ss[k].pc, sel.pc);
                    prev = lm_selu(stop[k], k ? ss[k - 1].pc : s.pc, prev);
                    pkd = lm_or(lm_andn(pkd, stop[k]), lm_andn(stop[k], dd[k]));
                    dn = lm_or(lm_andn(dn, stop[k]), dd[k]);
                }
#ifdef ZRT_SWEEP
                {   // lane steps taken (up to the stopping one), those into cells of
                    // empty bricks, and those that entered an empty brick
                    LaneM alive = lm_of(true);
                    uint32_t pcp = s.pc;
#pragma unroll
                    for (int k = 0; k < kS; ++k) {
                        const LaneM emp = lm_of(q[k] == 0ull);
                        const LaneM ent = lm_of(((pcp ^ ss[k].pc) & ~pk.low2) != 0u);
                        PARK_COUNT(13, __popcll(alive));
                        PARK_COUNT(14, __popcll(lm_and(alive, emp)));
                        PARK_COUNT(15, __popcll(lm_and(lm_and(alive, emp), ent)));
                        alive = lm_andn(alive, stop[k]);
                        pcp = ss[k].pc;
                    }
                }
#endif
                st = lm_selu(dn, kDone, st);
                s = sel;
                if (lm_selu(pkd, 1u, 0u)) {
                    const uint32_t x = s.pc ^ prev;
                    const uint32_t face = (x & pk.f0) ? (s.d0 >> 31)
                                                      : ((x & pk.f1) ? 2u + (s.d1 >> 31) : 4u + (s.d2 >> 31));
                    park_load_cell(p, s.pc, face, rng_slot);
                    st = kPark;
                }
                if (ESC) {
                    // a set escape bit: no cell of the ray after the queried
                    // brick holds a triangle, so the hit so far stands (this
                    // trip cannot have parked the lane: escape.h)
                    const LaneM esc = lm_and(lm_of(st == kWalk), lm_of(ew != 0u));
                    PARK_COUNT(16, __popcll(esc));
                    st = lm_selu(esc, kDone, st);
                    // one query per brick the ray enters (its word does not
                    // change while the lane walks inside the brick)
                    const uint32_t b = occx_brick<PK_BM>(w, s);
                    if (__builtin_expect(st == kWalk && emask != 0u && b != eb, 0)) {   // (kept out of the trip's straight line)
                        // the region of the brick that holds the lane's cell
                        // (escape.h EscShape: its sub-index is bits of the
                        // in-brick cell index x | y << 2 | z << 4, the low six
                        // bits of a brick-major word, the fields' low bits
                        // summed by occx_cell's multiply otherwise); with the
                        // brick-level table (key 0) the brick itself
                        const uint32_t ci = PK_BM ? s.pc : __umul24(s.pc & pk.low2, pk.kmul) >> pk.kshr;
                        const uint32_t rg = (b << esc_lg) | (ci & esc_mlo) | ((ci >> 2) & esc_mhi);
                        park_load_esc(reinterpret_cast<const uint32_t*>(reinterpret_cast<const uint8_t*>(w.esc) +
                                                                        rg * (4u * kEscWords) + eoff),
                                      esc_slot);
                        eb = b;
                    }
                }
            }
        }
        PARK_STAMP(1);
        // ---- test round: the parked lanes' cells, all pairs over all lanes
        if (__ballot(st == kPark) != 0ull) {
            __builtin_amdgcn_s_waitcnt(0x3f70);                    // vmcnt(0): the ranges landed
            PARK_STAMP(20);                                        // (sweep: the round's wait for them)
            const bool ready = st == kPark;
            // the parked cell's refs still to test: those the mask keeps
            // (cells of at most 32 refs; larger ones test every ref)
            const uint32_t rb = rng_slot[lane], re = rng_slot[64 + lane], cnt = re - rb;
            const uint32_t mw = rng_slot[128 + lane];
            const uint32_t keep = cnt < 32u ? mw & ((1u << cnt) - 1u) : mw;
            const uint32_t n = ready ? (cnt <= 32u ? (uint32_t)__popc(keep) : cnt) : 0u;
            // the record's hop bits (PARK_HOP): inverted, in a word of a cell
            // of at most 26 refs; an all-ones word (the first cell's) has none
            const uint32_t hb = cnt <= hop_max ? ~mw >> kHopShift : 0u;
            // park release (above): a round with fewer than rel_min parked
            // lanes that have refs to test is not run while lanes walk
            if (rel_min != 0u && __ballot(st == kWalk) != 0ull &&
                (uint32_t)__popcll(__ballot(ready && n != 0u)) < rel_min &&
                (uint32_t)__popcll(__ballot(ready && n == 0u)) >= w.rel_emin) {
                PARK_COUNT(19, __popcll(__ballot(ready && n == 0u)));
                if (ready && n == 0u) st = kWalk;
                PARK_HOP(ready && n == 0u, hb);
                continue;
            }
            uint32_t tot = 0;
            // the lane index of the round's own address arithmetic (the scan's row,
            // the best / uv slots): an opaque copy, so that what derives from it
            // is computed here and not kept in registers over the walk trips,
            // which sit at the 96-VGPR edge (with the hop's hm two such values
            // went to scratch)
            uint32_t rl = lane;
            asm volatile("" : "+v"(rl));
            const uint32_t off = wave_excl_sum(n, rl, tot);
            PARK_COUNT(5, 1);
            PARK_COUNT(6, (tot + 63u) / 64u);
            PARK_COUNT(7, tot);
            PARK_COUNT(17, __popcll(__ballot(ready)));               // parked lanes tested
            PARK_COUNT(18, __popcll(__ballot(ready && n == 0u)));    // ... with no ref left to test
            W.o[lane].w = nearest;
            rng_slot[lane] = rb;                                   // (the slots are free until the walk)
            rng_slot[64 + lane] = off;
            rng_slot[128 + lane] = cnt <= 32u ? keep : ~0u;
            W.d[rl].w = __uint_as_float(hb);                       // (kept in LDS over the sub-rounds, not in a VGPR)
            W.best[rl] = ~0ull;
            uint32_t carry = 0;
            for (uint32_t r = 0; r < tot; r += 64u) {
                // owner of pair slot r + lane: the last parked lane starting
                // at or before it (mark), or the one running over from r - 1
                W.mark[lane] = 0u;
                __builtin_amdgcn_wave_barrier();
                if (n != 0u && off >= r && off < r + 64u) W.mark[off - r] = lane + 1u;
                __builtin_amdgcn_wave_barrier();
                const uint64_t starts = __ballot(W.mark[lane] != 0u);
                const uint64_t upto = starts & (~0ull >> (63u - lane));
                const uint32_t owner = upto ? W.mark[63u - (uint32_t)__builtin_clzll(upto)] - 1u : carry;
                carry = (uint32_t)__builtin_amdgcn_readlane((int)owner, 63);
                const uint32_t g = r + lane;
                const float4 ro = W.o[owner], rd = W.d[owner];
                // pair g is the owner's (g - off)-th kept ref
                const uint32_t kr = g - rng_slot[64 + owner];
                const uint32_t j = rng_slot[owner] + (kr < 32u ? select_bit(s_sel8, rng_slot[128 + owner], kr) : kr);
                bool cand = false;
                float t = 0.0f, u = 0.0f, v = 0.0f;
                if (g < tot) {
                    v3 A, B, C;
                    load_tri(p, j, A, B, C);
                    cand = tri_ray_flat(A, B, C, mk(ro.x, ro.y, ro.z), mk(rd.x, rd.y, rd.z), &t, &u, &v) &&
                           ro.w > t && t > 0.0f;                   // stage3.zig:172
                }
                const unsigned long long key = ((unsigned long long)__float_as_uint(t) << 32) | j;
                if (cand) atomicMin(&W.best[owner], key);
                __builtin_amdgcn_wave_barrier();
                if (cand && W.best[owner] == key) W.uv[owner] = make_float2(u, v);
                __builtin_amdgcn_wave_barrier();
            }
            if (n != 0u) {
                const unsigned long long k = W.best[rl];
                if (k != ~0ull) {
                    nearest = __uint_as_float((uint32_t)(k >> 32));
                    hidx = (uint32_t)k;
                    const float2 uv = W.uv[rl];
                    hu = uv.x;
                    hv = uv.y;
                }
            }
            if (ready) st = kWalk;                                 // the cell is done: step out of it next
            if (hop_max != 0u) PARK_HOP(ready, __float_as_uint(W.d[rl].w));
        }
        PARK_STAMP(2);
    }
    __builtin_amdgcn_s_waitcnt(0x3f70);                            // vmcnt(0): no LDS-DMA outlives the wave
#ifdef ZRT_SWEEP
    if (lane == 0)
        for (int k = 0; k < 13; ++k) atomicAdd(&p.stats[16 + k], pprof[k]);
    if (lane == 0)
        for (int k = 13; k < 23; ++k) atomicAdd(&p.stats[48 + k - 13], pprof[k]);   // (21, 22: PARK_HOP)
#endif
}

// Split launches: the shading half of a bounce (traceRayRecursive's body
// after traceRay, stage3.zig:195-219) over the hit records wf_park_kernel
// wrote, one lane per path with every lane of the wave busy, appending the
// continuing paths to the next queue.  Same XCD group order as the trace.
//
// Early append: whether a path continues is known from its records
// alone (shade_segment: a hit with depth >= 2 continues, whether it scatters
// or passes through; a miss ends), so the wave reserves its appends with one
// returning atomic right after the records land and the atomic's latency
// overlaps the shading chain (triangle data -> texels -> RNG) instead of
// following it; the path is stored at its reserved position.  Against an
// append after each entry's shading: r05m, alternating processes, 2 rounds,
// images identical: cfg3 6019 / 6008 vs 5895 / 5877 (+2.2%), cfg5 +0.6%, cfg2
// ±0; one-stream shade 23.3-27.0 -> 18.3-18.6 ms per cfg3 frame
// (profiles/r05/r05m_ab_shade_early_append.log)
//
// The last bounce's launch has a kernel of its own (wf_shade_kernel's LAST);
// its entries per lane per fetch and launch bound: r06f, 3 rounds of
// alternating processes at full spp, images identical, against no LAST
// kernel (6518 / 3851 / 4165 Mrays/s cfg3 / cfg5 / cfg2): 4 entries (78
// VGPRs) 6586 / 3859 / 4193 (+1.0 / +0.2 / +0.7%); 3 entries (65) 6580 /
// 3845 / 4170; 2 entries at 8 waves per SIMD (52 VGPRs: two waves fit beside
// four park waves) 6564 / 3832 / 4123 (profiles/r06/r06f_ab_shade_last.log)
#ifndef ZRT_SHADE_LAST_MINW
#define ZRT_SHADE_LAST_MINW 1
#endif
#ifndef ZRT_SHADE_LAST_N
#define ZRT_SHADE_LAST_N 4
#endif
__device__ __forceinline__ bool shade_continues(bool valid, float4 b, float4 h) {
    return valid && h.x != kInf && (__float_as_uint(b.w) & 0xFFFFu) >= 2u;
}
// One entry (records loaded) shaded: an ending path writes its terminal
// radiance; a continuing one is left in (o, d, item, depth, slot, rng, mask)
// for the caller to store at its reserved position.  Returns shade_segment's
// answer (false for an invalid entry), which must equal shade_continues':
// the ZRT_SWEEP build counts disagreements (stats[60]) and fails the render
// on any.
struct ShadeOut {
    v3 o, d;
    uint32_t item, depth, slot, mask;
    Rng rng;
};
template <bool LAST = false>
__device__ __forceinline__ bool shade_entry_keep(const WfParams& w, const double* zx, const double* zf,
                                                 const DevMat* mats, bool valid, float4 a, float4 b, float4 c,
                                                 float4 h, const TriRec& tr, ShadeOut& so, uint32_t& n_seg,
                                                 unsigned long long* sp = nullptr) {
    if (!valid) return false;
    so.rng.s = ((uint64_t)__float_as_uint(c.y) << 32) | __float_as_uint(c.x);
    so.item = __float_as_uint(a.w);
    so.o = mk(a.x, a.y, a.z);
    so.d = mk(b.x, b.y, b.z);
    so.depth = __float_as_uint(b.w) & 0xFFFFu;
    so.slot = __float_as_uint(b.w) >> 16;
    so.mask = __float_as_uint(c.z);
    v3 L = mk(0, 0, 0);
    ++n_seg;
    const bool cont = shade_segment<LAST>(w, zx, zf, mats, so.item, h.x, h.y, h.z, tr, so.o, so.d, so.depth,
                                          so.slot, so.rng, so.mask, L, sp);
    if (!cont) w.term[so.item] = make_float4(L.x, L.y, L.z, __uint_as_float(so.mask));
    return cont;
}

// LMATS: the material descriptors (at most kLdsMats) copied to dynamic LDS
// (nmat x 96 B: the shade kernel's LDS stays small, so its workgroups still
// fit beside the other pass set's park kernel), so the dependent chain
// hit -> triangle data -> material -> texels takes its material hop from LDS
// instead of L2.
constexpr uint32_t kLdsMats = 64;
// LAST: the launch of a pass's last bounce (every entry has depth 1): the
// terminal radiance only (shade_segment<true>), no append
template <bool LMATS, bool LAST = false>
#ifndef ZRT_SHADE_MINW
#define ZRT_SHADE_MINW 1
#endif
__global__ __launch_bounds__(kTraceBlock, LAST ? ZRT_SHADE_LAST_MINW : ZRT_SHADE_MINW) void wf_shade_kernel(const WfParams w) {
    constexpr int NE = LAST ? ZRT_SHADE_LAST_N : kShadeEntries;   // entries per lane per fetch
    const TraceParams& p = w.t;
    __shared__ double s_zig[514];
    extern __shared__ __attribute__((aligned(16))) uint32_t s_dynm[];    // LMATS: p.nmat DevMat
    DevMat* const s_mats = reinterpret_cast<DevMat*>(s_dynm);
    for (uint32_t i = threadIdx.x; i < 514; i += blockDim.x) s_zig[i] = p.zig[i];
    if (LMATS)
        for (uint32_t i = threadIdx.x; i < p.nmat * (uint32_t)(sizeof(DevMat) / 4); i += blockDim.x)
            reinterpret_cast<uint32_t*>(s_mats)[i] = reinterpret_cast<const uint32_t*>(p.mats)[i];
    __syncthreads();
    const DevMat* const mats = LMATS ? s_mats : p.mats;
    const double* zx = s_zig;
    const double* zf = s_zig + 257;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t below = lane ? (~0ull >> (64u - lane)) : 0ull;
    uint32_t n_seg = 0;
    uint32_t grp = blockIdx.x & 7u, tried = 0;
    WfParams ws = w;
    ws.fetch8 = w.fetch8s;
    const float4 z4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#ifdef ZRT_SWEEP
    // ZRT_SWEEP builds: per-wave cycles and active lanes of the shading phases
    // (SHADE_STAMP; printed as zrt_shade_profile with ZRT_PARK_PROFILE)
    __shared__ unsigned long long s_sprof[kTraceBlock / 64][17];
    unsigned long long* const sp = s_sprof[threadIdx.x >> 6];
    if (lane < 16) sp[lane] = 0;
    if (lane == 16) sp[16] = __builtin_amdgcn_s_memtime();
    __builtin_amdgcn_wave_barrier();
#else
    unsigned long long* const sp = nullptr;
#endif
    // NE entries per lane per fetch: every entry's records are
    // loaded before the first is shaded, so their latency overlaps the
    // earlier entries' dependent chains (2: cfg3 +1.2%, cfg2 / cfg5 within
    // noise, 112 VGPRs, r02c6)
    for (;;) {
        uint32_t base = 0, lim = 0;
        if (!wf_fetch<false>(ws, 64u * NE, grp, tried, base, lim)) break;
        SHADE_STAMP(0, base);                  // work atomic
        float4 a[NE], b[NE], c[NE], h[NE];
        bool hit[NE];
        {
#pragma unroll
            for (int e = 0; e < NE; ++e) {
                const uint32_t j = base + 64u * e + lane;
                a[e] = b[e] = c[e] = h[e] = z4;
                hit[e] = j < lim;
                if (j < lim) {
                    const uint32_t i = ent_index<false>(w, grp, j);
                    a[e] = w.q_in[3ull * i]; b[e] = w.q_in[3ull * i + 1]; c[e] = w.q_in[3ull * i + 2]; h[e] = w.hit[i];
                }
            }
        }
        if (LAST) {
#pragma unroll
            for (int e = 0; e < NE; ++e) {
                ShadeOut so;
                (void)shade_entry_keep<true>(w, zx, zf, mats, hit[e], a[e], b[e], c[e], h[e],
                                             tri_rec(p, hit[e] ? h[e].x : kInf, __float_as_uint(h[e].w)), so, n_seg,
                                             sp);
            }
        } else {
            bool pc[NE];
            uint64_t m[NE];
            uint32_t tot = 0;
#pragma unroll
            for (int e = 0; e < NE; ++e) {
                pc[e] = shade_continues(hit[e], b[e], h[e]);
                m[e] = __ballot(pc[e]);
                tot += (uint32_t)__popcll(m[e]);
            }
            uint32_t ob = 0;
            if (lane == 0 && tot != 0u) ob = atomicAdd(&w.n_out8[grp * kCtr], tot);
            uint32_t before = 0;
            // (each entry's triangle record loaded as its shading starts: all
            // of them up front took 100 VGPRs and lost co-residency, r05c)
#pragma unroll
            for (int e = 0; e < NE; ++e) {
                ShadeOut so;
                const bool cont = shade_entry_keep(w, zx, zf, mats, hit[e], a[e], b[e], c[e], h[e],
                                                   tri_rec(p, hit[e] ? h[e].x : kInf, __float_as_uint(h[e].w)), so,
                                                   n_seg, sp);
#ifdef ZRT_SWEEP
                if (cont != pc[e]) atomicAdd(&p.stats[60], 1ull);
#else
                (void)cont;
#endif
                // (converged again: lane 0's reservation, long returned, reaches every lane)
                const uint32_t base = __builtin_amdgcn_readfirstlane(ob) + region_base(w, grp) + before;
                if (pc[e]) q_store(w, base + (uint32_t)__popcll(m[e] & below), so.o, so.d, so.item, so.depth, so.slot,
                                   so.rng, so.mask);
                before += (uint32_t)__popcll(m[e]);
            }
        }
    }
    const unsigned long long s0 = wave_sum(n_seg);
    if (lane == 0) atomicAdd(&p.stats[0], s0);
#ifdef ZRT_SWEEP
    if (lane == 0)
        for (int k = 0; k < 16; ++k) atomicAdd(&p.stats[32 + k], sp[k]);
#endif
}

// Fold + ordered sample sum + toRGB for wavefront mode (stage3.zig:219,
// :236-242): per sample, L = terminal radiance, then e + a*L for every slot
// that scattered, from the last bounce back to the first.  Items are
// pixel-major, so a block takes kResPix pixels and folds their samples
// kResSmp at a time with consecutive lanes on consecutive items (16 lanes
// read one pixel's 16 records: 256-byte runs), parks the radiances in LDS,
// and one thread per pixel then adds them in sample order (renderWorker's
// `pixel = pixel.add(...)` chain, unchanged: the same f32 sum).
constexpr uint32_t kResPix = 64, kResSmp = 16, kResRow = kResSmp * 3 + 1;   // +1: no LDS bank conflict
__global__ __launch_bounds__(kBlock) void wf_resolve_kernel(const float4* __restrict__ term,
                                                            const float4* __restrict__ stk4,
                                                            const float2* __restrict__ stk2, uint32_t T,
                                                            uint32_t P, uint32_t S, uint32_t max_bounce,
                                                            float4* acc, int first, int last,
                                                            float inv_spp, uint8_t* rgb, float* lin) {
    __shared__ float s_l[kResPix * kResRow];
    const uint32_t q0 = blockIdx.x * kResPix;
    const uint32_t np = min(kResPix, P - q0);
    const uint32_t tid = threadIdx.x;
    const uint32_t q = q0 + tid;
    v3 px = mk(0, 0, 0);
    if (tid < np && !first) { const float4 a = acc[q]; px = mk(a.x, a.y, a.z); }
    for (uint32_t c = 0; c < S; c += kResSmp) {
        const uint32_t ns = min(kResSmp, S - c);
        for (uint32_t m = tid; m < kResPix * kResSmp; m += kBlock) {
            const uint32_t i = m / kResSmp, k = m % kResSmp;   // the block's pixel i, sample c + k
            if (i < np && k < ns) {
                const uint32_t item = (q0 + i) * S + c + k;
                const float4 tm = term[item];
                v3 L = mk(tm.x, tm.y, tm.z);
                const uint32_t mask = __float_as_uint(tm.w);
                for (int slot = (int)max_bounce - 1; slot >= 0; --slot) {
                    if ((mask >> slot) & 1u) {
                        // e = +0 exactly when the hit stored no emissive plane
                        const float4 a = stk4[(uint64_t)slot * T + item];
                        v3 e = mk(0.0f, 0.0f, 0.0f);
                        if (__float_as_uint(a.w) != 0u) {
                            const float4 ee = reinterpret_cast<const float4*>(stk2)[(uint64_t)slot * T + item];
                            e = mk(ee.x, ee.y, ee.z);
                        }
                        L = add(e, mul(mk(a.x, a.y, a.z), L));
                    }
                }
                float* dst = s_l + i * kResRow + 3u * k;
                dst[0] = L.x; dst[1] = L.y; dst[2] = L.z;
            }
        }
        __syncthreads();
        if (tid < np) {
            const float* src = s_l + tid * kResRow;
            for (uint32_t k = 0; k < ns; ++k) px = add(px, mk(src[3 * k], src[3 * k + 1], src[3 * k + 2]));
        }
        __syncthreads();
    }
    if (tid >= np) return;
    if (!last) { acc[q] = make_float4(px.x, px.y, px.z, 0.0f); return; }
    const v3 l = mul(px, mk(inv_spp, inv_spp, inv_spp));
    uint8_t c[3];
    to_rgb(l, c);
    rgb[3 * (size_t)q + 0] = c[0];
    rgb[3 * (size_t)q + 1] = c[1];
    rgb[3 * (size_t)q + 2] = c[2];
    if (lin) { lin[3 * (size_t)q] = l.x; lin[3 * (size_t)q + 1] = l.y; lin[3 * (size_t)q + 2] = l.z; }
}

// renderWorker tail (stage3.zig:236-242) for the counting megakernel:
// ordered per-pixel sum over this pass's samples, then (last pass) * (1/spp)
// and toRGB.
__global__ __launch_bounds__(kBlock) void resolve_kernel(const float4* __restrict__ out, uint32_t P,
                                                         uint32_t S, float4* acc, int first, int last,
                                                         float inv_spp, uint8_t* rgb, float* lin) {
    const uint32_t q = blockIdx.x * kBlock + threadIdx.x;
    if (q >= P) return;
    v3 px = mk(0, 0, 0);
    if (!first) { const float4 a = acc[q]; px = mk(a.x, a.y, a.z); }
    for (uint32_t s = 0; s < S; ++s) {
        const float4 c = out[(size_t)q * S + s];          // pixel-major items
        px = add(px, mk(c.x, c.y, c.z));
    }
    if (!last) { acc[q] = make_float4(px.x, px.y, px.z, 0.0f); return; }
    const v3 l = mul(px, mk(inv_spp, inv_spp, inv_spp));
    uint8_t c[3];
    to_rgb(l, c);
    rgb[3 * (size_t)q + 0] = c[0];
    rgb[3 * (size_t)q + 1] = c[1];
    rgb[3 * (size_t)q + 2] = c[2];
    if (lin) { lin[3 * (size_t)q] = l.x; lin[3 * (size_t)q + 1] = l.y; lin[3 * (size_t)q + 2] = l.z; }
}

// The resolves of zrt_context_accumulate (a film): the two
// kernels above with the sum kept AND shown.  `film` is the film's row of
// per-pixel sums where those read and write d_acc; `first`: the film holds no
// sample yet (the stored bits are not read); every pass stores the sum back,
// and the call's last pass then also writes the image so far, sum * inv_spp
// with inv_spp = 1 / (samples in the film after this call), into whichever of
// rgb / lin is not null (a call that asked for no output stores 16 B per pixel
// and nothing else).  wf_film_resolve_kernel's fold and its ordered per-pixel
// add are wf_resolve_kernel's, statement for statement: the bit contract
// (any split of N samples over calls == one render of N) rests on the same
// f32 operations in the same order, so the two are kept apart rather than
// templated into one body whose code for the render could shift.
__global__ __launch_bounds__(kBlock) void wf_film_resolve_kernel(const float4* __restrict__ term,
                                                                 const float4* __restrict__ stk4,
                                                                 const float2* __restrict__ stk2, uint32_t T,
                                                                 uint32_t P, uint32_t S, uint32_t max_bounce,
                                                                 float4* film, int first, int last,
                                                                 float inv_spp, uint8_t* rgb, float* lin) {
    __shared__ float s_l[kResPix * kResRow];
    const uint32_t q0 = blockIdx.x * kResPix;
    const uint32_t np = min(kResPix, P - q0);
    const uint32_t tid = threadIdx.x;
    const uint32_t q = q0 + tid;
    v3 px = mk(0, 0, 0);
    if (tid < np && !first) { const float4 a = film[q]; px = mk(a.x, a.y, a.z); }
    for (uint32_t c = 0; c < S; c += kResSmp) {
        const uint32_t ns = min(kResSmp, S - c);
        for (uint32_t m = tid; m < kResPix * kResSmp; m += kBlock) {
            const uint32_t i = m / kResSmp, k = m % kResSmp;   // the block's pixel i, sample c + k
            if (i < np && k < ns) {
                const uint32_t item = (q0 + i) * S + c + k;
                const float4 tm = term[item];
                v3 L = mk(tm.x, tm.y, tm.z);
                const uint32_t mask = __float_as_uint(tm.w);
                for (int slot = (int)max_bounce - 1; slot >= 0; --slot) {
                    if ((mask >> slot) & 1u) {
                        const float4 a = stk4[(uint64_t)slot * T + item];
                        v3 e = mk(0.0f, 0.0f, 0.0f);
                        if (__float_as_uint(a.w) != 0u) {
                            const float4 ee = reinterpret_cast<const float4*>(stk2)[(uint64_t)slot * T + item];
                            e = mk(ee.x, ee.y, ee.z);
                        }
                        L = add(e, mul(mk(a.x, a.y, a.z), L));
                    }
                }
                float* dst = s_l + i * kResRow + 3u * k;
                dst[0] = L.x; dst[1] = L.y; dst[2] = L.z;
            }
        }
        __syncthreads();
        if (tid < np) {
            const float* src = s_l + tid * kResRow;
            for (uint32_t k = 0; k < ns; ++k) px = add(px, mk(src[3 * k], src[3 * k + 1], src[3 * k + 2]));
        }
        __syncthreads();
    }
    if (tid >= np) return;
    film[q] = make_float4(px.x, px.y, px.z, 0.0f);
    if (!last || (!rgb && !lin)) return;
    const v3 l = mul(px, mk(inv_spp, inv_spp, inv_spp));
    if (rgb) {
        uint8_t c[3];
        to_rgb(l, c);
        rgb[3 * (size_t)q + 0] = c[0];
        rgb[3 * (size_t)q + 1] = c[1];
        rgb[3 * (size_t)q + 2] = c[2];
    }
    if (lin) { lin[3 * (size_t)q] = l.x; lin[3 * (size_t)q + 1] = l.y; lin[3 * (size_t)q + 2] = l.z; }
}

// ... and resolve_kernel's, for the counting megakernel.
__global__ __launch_bounds__(kBlock) void film_resolve_kernel(const float4* __restrict__ out, uint32_t P,
                                                              uint32_t S, float4* film, int first, int last,
                                                              float inv_spp, uint8_t* rgb, float* lin) {
    const uint32_t q = blockIdx.x * kBlock + threadIdx.x;
    if (q >= P) return;
    v3 px = mk(0, 0, 0);
    if (!first) { const float4 a = film[q]; px = mk(a.x, a.y, a.z); }
    for (uint32_t s = 0; s < S; ++s) {
        const float4 c = out[(size_t)q * S + s];          // pixel-major items
        px = add(px, mk(c.x, c.y, c.z));
    }
    film[q] = make_float4(px.x, px.y, px.z, 0.0f);
    if (!last || (!rgb && !lin)) return;
    const v3 l = mul(px, mk(inv_spp, inv_spp, inv_spp));
    if (rgb) {
        uint8_t c[3];
        to_rgb(l, c);
        rgb[3 * (size_t)q + 0] = c[0];
        rgb[3 * (size_t)q + 1] = c[1];
        rgb[3 * (size_t)q + 2] = c[2];
    }
    if (lin) { lin[3 * (size_t)q] = l.x; lin[3 * (size_t)q + 1] = l.y; lin[3 * (size_t)q + 2] = l.z; }
}

// The resolves of zrt_context_refine on a sparse pixel list: the
// two film resolves above for the A active pixels of a film.  Item pixel q < A
// is the list's q-th pixel and its sums are the film's row slot[q]; the image
// is written by film_present_kernel for every owned pixel afterwards, so these
// take no outputs.  Separate kernels with the fold and the per-pixel add
// statement for statement, for the reason given above.
__global__ __launch_bounds__(kBlock) void wf_film_sparse_resolve_kernel(const float4* __restrict__ term,
                                                                        const float4* __restrict__ stk4,
                                                                        const float2* __restrict__ stk2, uint32_t T,
                                                                        uint32_t P, uint32_t S, uint32_t max_bounce,
                                                                        float4* film,
                                                                        const uint32_t* __restrict__ slots,
                                                                        int first) {
    __shared__ float s_l[kResPix * kResRow];
    const uint32_t q0 = blockIdx.x * kResPix;
    const uint32_t np = min(kResPix, P - q0);
    const uint32_t tid = threadIdx.x;
    const uint32_t row = tid < np ? slots[q0 + tid] : 0u;
    v3 px = mk(0, 0, 0);
    if (tid < np && !first) { const float4 a = film[row]; px = mk(a.x, a.y, a.z); }
    for (uint32_t c = 0; c < S; c += kResSmp) {
        const uint32_t ns = min(kResSmp, S - c);
        for (uint32_t m = tid; m < kResPix * kResSmp; m += kBlock) {
            const uint32_t i = m / kResSmp, k = m % kResSmp;   // the block's pixel i, sample c + k
            if (i < np && k < ns) {
                const uint32_t item = (q0 + i) * S + c + k;
                const float4 tm = term[item];
                v3 L = mk(tm.x, tm.y, tm.z);
                const uint32_t mask = __float_as_uint(tm.w);
                for (int slot = (int)max_bounce - 1; slot >= 0; --slot) {
                    if ((mask >> slot) & 1u) {
                        const float4 a = stk4[(uint64_t)slot * T + item];
                        v3 e = mk(0.0f, 0.0f, 0.0f);
                        if (__float_as_uint(a.w) != 0u) {
                            const float4 ee = reinterpret_cast<const float4*>(stk2)[(uint64_t)slot * T + item];
                            e = mk(ee.x, ee.y, ee.z);
                        }
                        L = add(e, mul(mk(a.x, a.y, a.z), L));
                    }
                }
                float* dst = s_l + i * kResRow + 3u * k;
                dst[0] = L.x; dst[1] = L.y; dst[2] = L.z;
            }
        }
        __syncthreads();
        if (tid < np) {
            const float* src = s_l + tid * kResRow;
            for (uint32_t k = 0; k < ns; ++k) px = add(px, mk(src[3 * k], src[3 * k + 1], src[3 * k + 2]));
        }
        __syncthreads();
    }
    if (tid >= np) return;
    film[row] = make_float4(px.x, px.y, px.z, 0.0f);
}

__global__ __launch_bounds__(kBlock) void film_sparse_resolve_kernel(const float4* __restrict__ out, uint32_t P,
                                                                     uint32_t S, float4* film,
                                                                     const uint32_t* __restrict__ slots, int first) {
    const uint32_t q = blockIdx.x * kBlock + threadIdx.x;
    if (q >= P) return;
    const uint32_t row = slots[q];
    v3 px = mk(0, 0, 0);
    if (!first) { const float4 a = film[row]; px = mk(a.x, a.y, a.z); }
    for (uint32_t s = 0; s < S; ++s) {
        const float4 c = out[(size_t)q * S + s];          // pixel-major items
        px = add(px, mk(c.x, c.y, c.z));
    }
    film[row] = make_float4(px.x, px.y, px.z, 0.0f);
}

// zrt_context_refine's decision (include/zrt.h), one thread per
// owned pixel.  An active pixel's image at b samples, cur = sum * (1 / b), is
// compared with its checkpoint, the image it showed at c samples; with
// `decide`, a pixel whose error is not above the threshold is frozen at b
// samples (a NaN error freezes).  A pixel that stays active takes cur as its
// new checkpoint.  blk[block] = the block's active pixels, for the scan.
// Everything f32, left to right as the header writes it; / and sqrtf are
// IEEE-rounded and nothing contracts (the build's flags).
__global__ __launch_bounds__(kBlock) void film_decide_kernel(const float4* __restrict__ sum, float4* state, uint32_t n,
                                                             uint32_t b, uint32_t c, float threshold, int decide,
                                                             uint32_t* __restrict__ blk) {
    __shared__ uint32_t s_w[kBlock / 64];
    const uint32_t q = blockIdx.x * kBlock + threadIdx.x;
    bool act = false;
    if (q < n) {
        const float4 st = state[q];
        act = (__float_as_uint(st.w) & kFilmFrozen) == 0u;
        if (act) {
            const float4 s = sum[q];
            const float inv = 1.0f / (float)b;
            const v3 cur = mul(mk(s.x, s.y, s.z), mk(inv, inv, inv));
            if (decide) {
                const float d = (fabsf(cur.x - st.x) + fabsf(cur.y - st.y)) + fabsf(cur.z - st.z);
                const float m = (cur.x + cur.y) + cur.z;
                const float k = (float)b / (float)(b - c);
                const float err = (d * k) / sqrtf(fmaxf(m, 0x1p-10f));
                act = err > threshold;
            }
            state[q] = act ? make_float4(cur.x, cur.y, cur.z, 0.0f)
                           : make_float4(st.x, st.y, st.z, __uint_as_float(kFilmFrozen | b));
        }
    }
    const uint64_t bal = __ballot(act);
    if ((threadIdx.x & 63u) == 0u) s_w[threadIdx.x >> 6] = (uint32_t)__popcll(bal);
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (uint32_t v = 0; v < kBlock / 64; ++v) t += s_w[v];
        blk[blockIdx.x] = t;
    }
}

// The blocks' counts into their exclusive bases, in place, and the total A
// into blk[nblk]: one workgroup walks the counts kBlock at a time (a 1080p
// rank has 8100), so no block ever waits for another.
__global__ __launch_bounds__(kBlock) void film_scan_kernel(uint32_t* blk, uint32_t nblk) {
    __shared__ uint32_t s_v[kBlock];
    __shared__ uint32_t s_carry;
    const uint32_t tid = threadIdx.x;
    if (tid == 0) s_carry = 0;
    __syncthreads();
    for (uint32_t i0 = 0; i0 < nblk; i0 += kBlock) {
        const uint32_t i = i0 + tid;
        const uint32_t v = i < nblk ? blk[i] : 0u;
        s_v[tid] = v;
        __syncthreads();
        for (uint32_t off = 1; off < kBlock; off <<= 1) {       // inclusive scan of the chunk
            const uint32_t a = tid >= off ? s_v[tid - off] : 0u;
            __syncthreads();
            s_v[tid] += a;
            __syncthreads();
        }
        const uint32_t carry = s_carry;
        if (i < nblk) blk[i] = carry + s_v[tid] - v;
        __syncthreads();
        if (tid == kBlock - 1) s_carry = carry + s_v[tid];
        __syncthreads();
    }
    if (tid == 0) blk[nblk] = s_carry;
}

// The active pixels in packed order: pixel q's place is its block's base, the
// active pixels of the block's waves before its own, and its rank among its
// wave's (ballot and mbcnt).  list: the image pixel (a call's pixlist), slot:
// the film row.  base + rank < A <= n: the flags are those the counts were
// taken from.
__global__ __launch_bounds__(kBlock) void film_scatter_kernel(const float4* __restrict__ state,
                                                              const uint32_t* __restrict__ pix, uint32_t n,
                                                              const uint32_t* __restrict__ blk,
                                                              uint32_t* __restrict__ list,
                                                              uint32_t* __restrict__ slot) {
    __shared__ uint32_t s_w[kBlock / 64];
    const uint32_t q = blockIdx.x * kBlock + threadIdx.x;
    const bool act = q < n && (__float_as_uint(state[q].w) & kFilmFrozen) == 0u;
    const uint64_t bal = __ballot(act);
    const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0u) s_w[wave] = (uint32_t)__popcll(bal);
    __syncthreads();
    if (!act) return;
    uint32_t at = blk[blockIdx.x] + rank;
    for (uint32_t v = 0; v < wave; ++v) at += s_w[v];
    if (at >= n) return;                   // (cannot happen; a list of n entries is what was allocated)
    list[at] = pix[q];
    slot[at] = q;
}

// The frame a film shows, every owned pixel at its own sample count: N = the
// count a frozen pixel was frozen at, else the film's samples; linear = sum *
// (1 / N), rgb = toRGB(linear).  state null: no pixel is frozen.  Null outputs
// are skipped; cnt: N itself.
__global__ __launch_bounds__(kBlock) void film_present_kernel(const float4* __restrict__ sum,
                                                              const float4* __restrict__ state, uint32_t n,
                                                              uint32_t samples, uint8_t* rgb, float* lin,
                                                              uint32_t* cnt) {
    const uint32_t q = blockIdx.x * kBlock + threadIdx.x;
    if (q >= n) return;
    const uint32_t w = state ? __float_as_uint(state[q].w) : 0u;
    const uint32_t N = (w & kFilmFrozen) ? (w & ~kFilmFrozen) : samples;
    if (cnt) cnt[q] = N;
    if (!rgb && !lin) return;
    const float4 a = sum[q];
    const float inv = 1.0f / (float)N;
    const v3 l = mul(mk(a.x, a.y, a.z), mk(inv, inv, inv));
    if (rgb) {
        uint8_t c[3];
        to_rgb(l, c);
        rgb[3 * (size_t)q + 0] = c[0];
        rgb[3 * (size_t)q + 1] = c[1];
        rgb[3 * (size_t)q + 2] = c[2];
    }
    if (lin) { lin[3 * (size_t)q] = l.x; lin[3 * (size_t)q + 1] = l.y; lin[3 * (size_t)q + 2] = l.z; }
}

using TraceFn = void (*)(const TraceParams);
using WfFn = void (*)(const WfParams);

// wf_kernel occupancy (waves per SIMD, __launch_bounds__).  The primary
// launch at 7 (72 VGPRs, no scratch access inside the cell walk): r02ah, one
// box, cfg3 64 spp at 5 / 6 / 7 / 8 waves 3127 / 3155 / 3197 / 3193 Mrays/s
// (8 reloads spills inside the walk).  The lane-walk bounce launches
// (ZRT_FLAG_LANE_WALK) at 6: 7 waves put 2-3 spill reloads in that walk and
// ran cfg3 at 1933 vs 2108 (round 1).  tests/test_codegen.py checks every
// instantiation zrt_timed_kernels names.
#ifndef ZRT_WF_MINW
#define ZRT_WF_MINW 6
#endif
// r04pw (the frustum-bound primary): 6 / 7 / 8 waves cfg3 5732 / 5724 / 5692,
// cfg5 3491 / 3489 / 3493, cfg2 3778 / 3739 / 3725 Mrays/s; at 6 the primary
// has no scratch access at all (12 at 7, 26 and walk reloads at 8).  Built
// without SLP pairing (Makefile) the packed primary fits 7 waves (72 VGPRs,
// no spill): r05ap, cfg3 6412 / 6400 vs 6346 / 6357 (+0.9%), cfg2 +0.7%,
// cfg5 +0.3% (profiles/r05/r05ap_ab_primary7_select.log).  Round 6: the
// entry-face skip (trace_ray) spills 6-10 VGPRs at 7 waves, some in
// the walk loop of the frustum instantiation; at 6 waves it spills nothing
// and measured the same (r06af / r06ag: cfg3 +0.9 / +1.3% vs +1.3 / +1.2%
// at 7 over the 7-wave tree without the skip).  With one triangle load in
// flight per lane (ZRT_TRI_BATCH 1) the primary fits 7 waves again (70
// VGPRs, no spill): r06bi / r06bj
#ifndef ZRT_WF_MINW0
#define ZRT_WF_MINW0 7
#endif
constexpr int kWfMinWaves = ZRT_WF_MINW;
constexpr int kWfMinWaves0 = ZRT_WF_MINW0;
// wf_park_kernel schedule: a test round once 14 lanes are parked, a shade +
// refill round once 16 lanes are finished (cfg3 64 spp sweep, r02d: T 4-16 x
// R 8/16/32; T 12 R 16 3110 Mrays/s, T 8-16 R 16 within 1.3%, R 8 -15%,
// R 32 -13%; cfg5 T 16 R 16 2075, T 8 2055; full spp after the lane-mask
// trip, r03z: T 14 vs 12 cfg3 +0.3%, cfg2 +0.6%, cfg5 +0.5%; T 10 / 16,
// R 12 / 20 no better).  On round 5's final tree (cheaper walk trips and
// test rounds) R 20 is ahead everywhere: r05au / r05av, 2 + 2 rounds, cfg3
// +0.9 / +0.5%, cfg5 +0.25 / +0.3%, cfg2 +0.3 / +0.2%; T 12 / 16 / 18 and
// R 12 / 24 are not (profiles/r05/r05au_ab_o2_park_schedule.log,
// r05av_ab_park_schedule2.log).  ZRT_SWEEP builds read ZRT_PARK_T / ZRT_PARK_R.
#ifndef ZRT_PARK_T
#define ZRT_PARK_T 14
#endif
#ifndef ZRT_PARK_R
#define ZRT_PARK_R 20
#endif
constexpr uint32_t kParkTestMin = ZRT_PARK_T;
#ifndef ZRT_PARK_T_REL
#define ZRT_PARK_T_REL 12
#endif
constexpr uint32_t kParkTestMinRel = ZRT_PARK_T_REL;   // with the park release
constexpr uint32_t kParkRefillMin = ZRT_PARK_R;
// packed walk state when every axis has at most kPackMaxRes cells
const WfFn kWfPrimary = (WfFn)wf_kernel<kWfMinWaves0, true, true>;
const WfFn kWfBounce = (WfFn)wf_kernel<kWfMinWaves, false, true>;
const WfFn kWfPrimaryBM = (WfFn)wf_kernel<kWfMinWaves0, true, true, true>;
const WfFn kWfBounceBM = (WfFn)wf_kernel<kWfMinWaves, false, true, true>;
const WfFn kWfPrimaryWide = (WfFn)wf_kernel<kWfMinWaves, true, false>;   // (6 waves: at 7 it spills)
const WfFn kWfBounceWide = (WfFn)wf_kernel<kWfMinWaves, false, false>;
// scenes with an edge component of 2^62 or more, or infinite
// (zrt_context::mt_exact): the unpacked lane walk with the IEEE division in
// Moller-Trumbore, for every launch
const WfFn kWfPrimaryExact = (WfFn)wf_kernel<kWfMinWaves, true, false, false, true>;
const WfFn kWfBounceExact = (WfFn)wf_kernel<kWfMinWaves, false, false, false, true>;

// ---------------------------------------------------------------------------
// Batch ray queries (zrt_context_trace) and segment queries
// (zrt_context_segments): Scene.traceRay (stage3.zig:152-186) for caller-given
// rays through the render's own walks -- trace_ray per lane, or wf_park_kernel
// over an identity queue (ray i = queue entry i).  One set of kernels: the
// segment call's are the SEG instantiations, in which nearest_hit.t starts at
// the ray's bound t_max instead of +inf (stage3.zig:154), in closest or
// any-hit form.  Three things differ: the initial nearest
// (trace_ray's nearest0, the park kernel's query modes), the any-hit exit, and
// the result: a miss is what left nearest bit-equal to the bound (lane walk)
// or the ref at 0xFFFFFFFF (park records), not t == +inf -- the bound may be
// anything, NaN included -- and is stored as (+inf, 0, 0, 0xFFFFFFFF) and / or
// the byte 0.
//
// Directions need not be unit length, which the render's are.  Its kernels
// lean on that in three places:
//  * Moller-Trumbore's short reciprocal (mt_inv_det) is the division for
//    |det| < 2^126, and |det| <= |e1| |e2| |d| stays below that for edge
//    components below 2^62 (the contexts' mt_exact threshold) when |d| < 4/3;
//  * dda_init_fq's quotients are the divisions for divisors |d_a| <= 2^32
//    (quot_rn; its own guards cover small components and the numerators);
//  * the escape table bins a direction by its slopes over the reciprocal of
//    its dominant component (esc_dir_bin), which has to be a normal float
//    with a normal reciprocal.
// A ray with 0.5 <= d.d <= 1.5 (ray_fast; the f32 dot product's rounding is
// far inside that slack, and an overflow, an underflow to zero or a NaN fails
// it) meets all three: every |d_a| <= |d| < 1.23 and the dominant |d_a| >=
// 0.4.  Such rays take the fast kernels; the others (and every ray of an
// mt_exact context, of ZRT_FLAG_MT_EXACT or of a counting call) take the
// unpacked lane walk with dda_init and the IEEE division, which is the
// reference's arithmetic for any direction.  The frustum bounds do not apply
// to a query: tau = -inf (no fast-forward, not even over crossings at
// negative t, which tau = 0 would skip) and tfar = +inf.
struct QueryParams {
    WfParams w;               // w.t: grid and scene; the park path's queue, hit records and counters
    const float* rays;        // this chunk: 6 floats per ray (origin, direction)
    uint32_t* hits;           // this chunk: a zrt_hit per ray as 4 u32 (4-byte aligned); a segment call: or null
    float4* q;                // query_pack_kernel: the queue (w.q_in)
    uint32_t* n_in8;          // query_pack_kernel: the queue's region counts (w.n_in8)
    uint32_t n;               // rays of this chunk (the host cuts a batch into chunks of <= kTraceChunk)
    uint32_t which;           // kRaysAll, kRaysFast or kRaysRest
    uint32_t* ctr;            // [0], [1]: work counters of the chunk's two walk launches;
                              // [2]: its rays outside the fast domain
    // a segment call (the SEG kernels; zero in every other)
    const float* t_max;       // this chunk: a bound per ray, or null: t_max_all
    float t_max_all;
    uint8_t* occ;             // this chunk: a byte per ray (1: not missed), or null
    uint32_t count;           // query_walk_kernel: count the rays not missed (any-hit calls; STATS counts anyway)
};
constexpr uint32_t kRaysAll = 0, kRaysFast = 1, kRaysRest = 2;

__device__ __forceinline__ bool ray_fast(v3 d) {
    const float n2 = dot(d, d);
    return n2 >= 0.5f && n2 <= 1.5f;
}
__device__ __forceinline__ float query_bound(const QueryParams& q, uint32_t i) { return q.t_max ? q.t_max[i] : q.t_max_all; }
// The zrt_hit of a ray and / or its byte (a lane's own plain store:
// global_store_byte); a miss is (+inf, 0, 0, 0xFFFFFFFF), which the reference
// leaves undefined.  Without SEG a miss is t == +inf (nearest stayed there: a
// kept t is below it), hits is not null and there is no byte.
template <bool SEG>
__device__ __forceinline__ void query_store(const QueryParams& q, uint32_t i, bool miss, float t, float u, float v,
                                            uint32_t ref) {
    if (!SEG || q.hits) {
        uint32_t* h = q.hits + 4ull * i;
        h[0] = __float_as_uint(miss ? kInf : t);
        h[1] = miss ? 0u : __float_as_uint(u);
        h[2] = miss ? 0u : __float_as_uint(v);
        h[3] = miss ? 0xFFFFFFFFu : ref;
    }
    if (SEG && q.occ) q.occ[i] = miss ? (uint8_t)0 : (uint8_t)1;
}

// One lane = one ray, walked and tested by the lane itself (trace_ray), on a
// persistent grid: a wave takes 64 * kWfChunk consecutive rays per work atomic.
// `which`: kRaysFast leaves (and counts) the rays outside the fast domain,
// kRaysRest traces only those -- the chunk's second launch, which ends at once
// when the first counted none -- and kRaysAll every ray.
// The walk ends for any input, NaN and infinite components included: a step
// moves one axis's cell by one towards that axis's exit cell (0 or res - 1,
// fixed by the direction's sign at the start; the start cell is clamped into
// the grid), whatever the crossing values compare like, and the step out of
// an exit cell ends the walk (T_EXIT = +inf, `exited`), so a ray takes at
// most res0 + res1 + res2 steps; a cell's tests are bounded by its range.
// STATS: per-lane work counters, the counting render's conventions
// (trace_kernel): a cell per loop trip, a test per ref tried.
// SEG: trace_ray's BOUNDED code, compiled into these instantiations only; the
// rays not missed are also counted (stats[3]) by every any-hit call (r.count).
// ANY: the any-hit exit of trace_ray, instantiated for the counting kernel
// only, whose counters it defines; the timed any-hit walks were measured
// against the closest ones and dropped.
template <bool STATS, bool PACKED, bool PK_BM, bool MTX, bool ANY, bool SEG>
__global__ __launch_bounds__(kTraceBlock, STATS ? 1 : kWfMinWaves) void query_walk_kernel(const QueryParams r) {
    static_assert(SEG || !ANY, "the any-hit exit is a segment call's");
    const TraceParams& p = r.w.t;
    extern __shared__ __attribute__((aligned(16))) uint32_t s_occ[];
    __shared__ uint32_t s_wcnt[2 * (kTraceBlock / 64)];
    if (r.which == kRaysRest && r.ctr[2] == 0u) return;            // (the whole grid: nothing left)
    for (uint32_t i = threadIdx.x; i < p.occ_words; i += blockDim.x) s_occ[i] = p.occ[i];
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t* const work = r.ctr + (r.which == kRaysRest ? 1u : 0u);
    uint64_t prof[11] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t n_seg = 0, n_cells = 0, n_tests = 0, n_hits = 0, n_rest = 0;
    for (;;) {
        uint32_t base = 0;
        if (lane == 0) base = atomicAdd(work, 64u * kWfChunk);
        base = __builtin_amdgcn_readfirstlane(base);
        if (base >= r.n) break;
        for (uint32_t sub = 0; sub < kWfChunk; ++sub) {
            const uint32_t i = base + 64u * sub + lane;
            if (i >= r.n) continue;
            v3 o, d;
            ray_load(r.rays, i, o, d);
            const bool fast = ray_fast(d);
            if (r.which == kRaysFast && !fast) { ++n_rest; continue; }
            if (r.which == kRaysRest && fast) continue;
            const float bound = SEG ? query_bound(r, i) : kInf;
            float hu = 0.0f, hv = 0.0f;
            uint32_t hidx = 0;
            const float t = trace_ray<STATS, kTriBatch, PACKED, PK_BM, MTX, ANY, SEG>(p, s_occ, o, d, hu, hv, hidx,
                                                                                      n_cells, n_tests, prof, s_wcnt,
                                                                                      -kInf, kInf, bound);
            const bool miss = SEG ? __float_as_uint(t) == __float_as_uint(bound) : t == kInf;
            ++n_seg;
            if (!miss) ++n_hits;
            query_store<SEG>(r, i, miss, t, hu, hv, hidx);
        }
    }
    if (r.which == kRaysFast) {
        const unsigned long long s = wave_sum(n_rest);
        if (lane == 0 && s != 0ull) atomicAdd(&r.ctr[2], (uint32_t)s);
    }
    if (STATS) {
        const unsigned long long s0 = wave_sum(n_seg), s1 = wave_sum(n_cells), s2 = wave_sum(n_tests);
        if (lane == 0) {
            atomicAdd(&p.stats[0], s0);
            atomicAdd(&p.stats[1], s1);
            atomicAdd(&p.stats[2], s2);
        }
    }
    if (STATS || (SEG && r.count != 0u)) {
        const unsigned long long s3 = wave_sum(n_hits);
        if (lane == 0 && s3 != 0ull) atomicAdd(&p.stats[3], s3);
    }
}

// The park path's queue for a chunk of n rays: ray i is queue entry i.  With
// S = 1 and P = n, region g of the queue (region_base) is entries
// [xcd_q0(n, g), xcd_q0(n, g + 1)), so eight full regions are the identity
// layout and their counts the differences.  A record's (o, item) and
// (d, depth) words are all wf_park_kernel reads; the hit record of entry i is
// w.hit[i].  Rays outside the fast domain are counted for the launch that
// retraces them (query_walk_kernel, kRaysRest); the park kernel walks them
// like any ray (it ends for any input, as above: its exit test compares cell
// fields) and their records are overwritten.
// The body of a one-thread-per-ray kernel: thread i < n writes entry i from
// what ray(i, o, d, w) gives it -- the ray and the (d, .) word: the depth 1, or
// a segment's bound, where the park kernel's query modes take it from.
template <class Ray>
__device__ __forceinline__ void identity_queue_fill(float4* q, uint32_t* n_in8, uint32_t* ctr, uint32_t n, Ray ray) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i < 8u) n_in8[i * kCtr] = xcd_q0(n, i + 1u) - xcd_q0(n, i);
    bool rest = false;
    if (i < n) {
        v3 o, d;
        float w;
        ray(i, o, d, w);
        q[3ull * i] = make_float4(o.x, o.y, o.z, __uint_as_float(i));
        q[3ull * i + 1] = make_float4(d.x, d.y, d.z, w);
        rest = !ray_fast(d);
    }
    const uint64_t m = __ballot(rest);
    if (m != 0ull && (threadIdx.x & 63u) == (uint32_t)__builtin_ctzll(m)) atomicAdd(&ctr[2], (uint32_t)__popcll(m));
}

template <bool SEG>
__global__ __launch_bounds__(kBlock) void query_pack_kernel(const QueryParams r) {
    identity_queue_fill(r.q, r.n_in8, r.ctr, r.n, [&](uint32_t i, v3& o, v3& d, float& w) {
        ray_load(r.rays, i, o, d);
        w = SEG ? query_bound(r, i) : __uint_as_float(1u);
    });
}

// The park kernel's hit records (t, u, v, ref) as zrt_hit and / or the byte:
// the same refs as the lane walk's, the miss fields set.  COUNT (any-hit
// calls): the rays not missed into stats[3], those outside the fast domain
// left to the kRaysRest launch that retraces them and counts them itself.
// A counting block takes kOutCountRays * kBlock consecutive rays and adds its
// count with one atomic (one per wave of 64 rays queued 65536 atomics of a
// 2^22-ray call on one address: 0.75 ms, more than a third of the park kernel's
// own time, profiles/segment_bench_cfg3_first.log).
constexpr uint32_t kOutCountRays = 8;
template <bool SEG, bool COUNT>
__global__ __launch_bounds__(kBlock) void query_out_kernel(const QueryParams r) {
    static_assert(SEG || !COUNT, "only an any-hit segment call counts here");
    __shared__ uint32_t s_n;
    constexpr uint32_t per = COUNT ? kOutCountRays : 1u;
    if (COUNT) {
        if (threadIdx.x == 0) s_n = 0u;
        __syncthreads();
    }
    const bool some_rest = COUNT && r.ctr[2] != 0u;
    uint32_t cnt = 0;
    for (uint32_t k = 0; k < per; ++k) {
        const uint32_t i = (blockIdx.x * per + k) * kBlock + threadIdx.x;
        if (i >= r.n) continue;
        const float4 h = r.w.hit[i];
        const uint32_t ref = __float_as_uint(h.w);
        const bool miss = SEG ? ref == 0xFFFFFFFFu : h.x == kInf;
        query_store<SEG>(r, i, miss, h.x, h.y, h.z, ref);
        if (COUNT && !miss) {
            bool mine = true;
            if (some_rest) {
                v3 o, d;
                ray_load(r.rays, i, o, d);
                mine = ray_fast(d);
            }
            cnt += mine ? 1u : 0u;
        }
    }
    if (COUNT) {
        const unsigned long long s = wave_sum(cnt);
        if ((threadIdx.x & 63u) == 0u && s != 0ull) atomicAdd(&s_n, (uint32_t)s);
        __syncthreads();
        if (threadIdx.x == 0 && s_n != 0u) atomicAdd(&r.w.t.stats[3], (unsigned long long)s_n);
    }
}

using QueryFn = void (*)(const QueryParams);
// The kernels of a call, [0] zrt_context_trace (and a radiance call's first
// segments), [1] / [2] zrt_context_segments in closest / any-hit form.  walk:
// brick-major packed, packed, wide, the IEEE division, counting.  Any-hit calls
// take the closest walks, the yes / no kept; only a counting call walks with
// the any-hit exit, which its counters are defined by.
struct QueryKernels {
    QueryFn walk[5], pack, out;
    uint32_t out_rays;        // rays per thread of `out`
};
template <bool SEG, bool ANY>
static QueryKernels query_kernels() {
    return {{(QueryFn)query_walk_kernel<false, true, true, false, false, SEG>,
             (QueryFn)query_walk_kernel<false, true, false, false, false, SEG>,
             (QueryFn)query_walk_kernel<false, false, false, false, false, SEG>,
             (QueryFn)query_walk_kernel<false, false, false, true, false, SEG>,
             (QueryFn)query_walk_kernel<true, false, false, true, ANY, SEG>},
            (QueryFn)query_pack_kernel<SEG>, (QueryFn)query_out_kernel<SEG, ANY>, ANY ? kOutCountRays : 1u};
}
const QueryKernels kQuery[3] = {query_kernels<false, false>(), query_kernels<true, false>(), query_kernels<true, true>()};
// rays per chunk of a batch: queue indices and work counters stay far below
// 2^32, and the staging and queue memory of a call is bounded (104 B per ray)
constexpr uint64_t kTraceChunk = 1ull << 20;
// batch size from which a call takes the park path unasked (ZRT_TRACE_PARK
// forces it, ZRT_FLAG_LANE_WALK forbids it): 2^19, the smallest size at which
// the park path won in both repeats on BOTH ray sets of tools/trace_bench.py
// (cfg3 scene, profiles/trace_bench_cfg3.json: camera rays 0.100 vs 0.137 ms,
// incoherent rays 0.48 vs 1.12 ms per call).  Below it the winner depends on
// the rays, which the call cannot know: incoherent rays are 2-3.6x faster
// through the park path at every size from 2^10 up, coherent rays that all
// miss 1.2-5x faster through the lane walk
constexpr uint64_t kTraceParkMin = 1ull << 19;
constexpr uint32_t kTraceFlags = ZRT_FLAG_COUNT_STATS | ZRT_FLAG_LANE_WALK | ZRT_FLAG_MT_EXACT | ZRT_FLAG_ESCAPE |
                                 ZRT_FLAG_NO_ESCAPE | ZRT_FLAG_RELEASE | ZRT_FLAG_NO_RELEASE | ZRT_FLAG_BFCULL |
                                 ZRT_FLAG_NO_BFCULL | ZRT_FLAG_HOP | ZRT_FLAG_NO_HOP | ZRT_TRACE_PARK;
static_assert((ZRT_SEGMENT_ANY & (kTraceFlags | ZRT_RADIANCE_PER_SAMPLE | 0xFFFFu)) == 0u, "a bit of its own");
static_assert((ZRT_DIRECT_UNSHADOWED & (kTraceFlags | ZRT_RADIANCE_PER_SAMPLE | ZRT_SEGMENT_ANY | 0xFFFFu)) == 0u,
              "a bit of its own");
static_assert(sizeof(zrt_light) == 48 && sizeof(zrt_direct_batch) == 64, "include/zrt.h");

// batch size from which a segment call takes the park path unasked: 2^16, the
// smallest size tools/segment_bench.py measures; there and at 2^20 and 2^22 the
// park path won on all three bounded ray sets (ao at two radii, shadow) in
// both rounds, 3.5-3.8x at 2^16 on ao (profiles/segment_bench_cfg3.json).
// Bounded rays start on surfaces and spread: the incoherent kind, which the
// park path serves better at any size (kTraceParkMin's comment)
constexpr uint64_t kSegParkMin = 1ull << 16;
// bytes per ray a segment call adds to a batch query's staging: the bound and the byte
constexpr uint64_t kSegStageBytes = 5;

// ---------------------------------------------------------------------------
// Surface queries (zrt_context_surface): the shading inputs at a
// ray's first hit -- traceRayRecursive between stage3.zig:199 and :206 and the
// continuation origin of :209 / :216 -- gathered from the hit records a trace
// call's kernels left for the chunk.  One lane per ray on a plain grid, one
// pass: hit record -> triangle Data -> material -> texels.
struct SurfaceParams {
    const float* rays;        // this chunk: 6 floats per ray (origin, direction as given)
    const uint32_t* hits;     // this chunk: the zrt_hit of every ray as 4 u32 (4-byte aligned)
    float4* surf;             // this chunk: a zrt_surface per ray as 4 float4 (16-byte aligned)
    const float4* tri_data;   // TraceParams::tri_data
    const DevMat* mats;
    const float* texels;
    uint32_t n;               // rays of this chunk
};
// The shading inputs of a hit (SurfaceInputs, surface_gather): emitters.h, shared with emitters.hip.
// One lane per ray; a miss lane loads nothing after its hit record and ray.
__global__ __launch_bounds__(kBlock) void surface_kernel(const SurfaceParams r) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= r.n) return;
    uint4 h;
    if ((reinterpret_cast<uintptr_t>(r.hits) & 15u) == 0u) {        // (uniform: the context's own records always are)
        h = reinterpret_cast<const uint4*>(r.hits)[i];
    } else {
        const uint32_t* q = r.hits + 4ull * i;
        h = make_uint4(q[0], q[1], q[2], q[3]);
    }
    v3 o, d;
    ray_load(r.rays, i, o, d);
    float4* const out = r.surf + 4ull * i;
    const float t = __uint_as_float(h.x), hu = __uint_as_float(h.y), hv = __uint_as_float(h.z);
    if (t == kInf) {                                                // a miss (query_store)
        const float4 z4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        out[0] = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(0xFFFFFFFFu));
        out[1] = z4;
        out[2] = z4;
        out[3] = z4;
        return;
    }
    const SurfaceInputs g = surface_gather(r.tri_data, r.mats, r.texels, hu, hv, h.w);
    const v3 no = add(o, scale(d, t + kFltEps));
    out[0] = make_float4(no.x, no.y, no.z, g.mat);
    out[1] = make_float4(g.nrm.x, g.nrm.y, g.nrm.z, g.transparency);
    out[2] = make_float4(g.albedo.x, g.albedo.y, g.albedo.z, g.tc0);
    out[3] = make_float4(g.emissive.x, g.emissive.y, g.emissive.z, g.tc1);
}

// ---------------------------------------------------------------------------
// Feature planes (zrt_context_features): base colour, normal,
// emission, depth, transparency and hit count of the first hit per pixel, over
// the camera samples of a render.  A pass is a render's pass without the path
// tracer: feature_walk_kernel is the primary launch's fetch, camera ray and
// lane walk followed by surface_kernel's gather, and leaves one record per
// item; feature_resolve_kernel is wf_resolve_kernel's ordered per-pixel sum
// over those records.  No RNG state beyond the two jitter floats, no scatter,
// no queue append.
//
// An item's record, three float4 at rec[3 * item] (items pixel-major, as the
// render's): (base colour, t) (normal, transparency) (emissive, 0).  t = +inf
// marks a miss, whose other two words are not written and not used.
struct FeatureParams {
    WfParams w;               // w.t: grid, scene, camera and pass; w.fetch8: the pass's eight work counters
    float4* rec;
};
// Launch bounds and instantiations are wf_kernel's primary ones (kWfPrimary*):
// the packed walks at kWfMinWaves0 waves, the wide and IEEE-division walks at
// kWfMinWaves; STATS is the counting build's walk (trace_kernel's trace_ray).
// The hits are counted in every instantiation (zrt_stats.hits).
template <bool STATS, bool PACKED, bool PK_BM, bool MTX>
__global__ __launch_bounds__(kTraceBlock, STATS ? 1 : (PACKED ? kWfMinWaves0 : kWfMinWaves))
void feature_walk_kernel(const FeatureParams r) {
    const WfParams& w = r.w;
    const TraceParams& p = w.t;
    extern __shared__ __attribute__((aligned(16))) uint32_t s_occ[];
    __shared__ uint32_t s_wcnt[2 * (kTraceBlock / 64)];
    for (uint32_t i = threadIdx.x; i < p.occ_words; i += blockDim.x) s_occ[i] = p.occ[i];
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    uint64_t prof[11] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t n_cells = 0, n_tests = 0, n_hits = 0;
    uint32_t grp = blockIdx.x & 7u, tried = 0;
    for (;;) {
        uint32_t base = 0, lim = 0;
        if (!wf_fetch<true>(w, 64u * kWfChunk, grp, tried, base, lim)) break;
        for (uint32_t sub = 0; sub < kWfChunk && base + 64u * sub < lim; ++sub) {
            const uint32_t j = base + 64u * sub + lane;
            if (j >= lim) continue;
            const uint32_t i = ent_index<true>(w, grp, j);
            v3 o, d;
            Rng rng0;
            uint32_t blk = 0;
            float tau = 0.0f, tfar = kInf;
            camera_ray(p, i, rng0, o, d, &blk);
            if (p.tlo) {
                const float4 fb = p.tlo[blk];
                tau = fb.x;
                tfar = fb.y;
            }
            float hu = 0.0f, hv = 0.0f;
            uint32_t hidx = 0;
            const float t = trace_ray<STATS, kTriBatch, PACKED, PK_BM, MTX>(p, s_occ, o, d, hu, hv, hidx, n_cells, n_tests,
                                                                            prof, s_wcnt, tau, tfar);
            float4* const out = r.rec + 3ull * i;
            if (t == kInf) {
                out[0] = make_float4(0.0f, 0.0f, 0.0f, kInf);
                continue;
            }
            ++n_hits;
            const SurfaceInputs g = surface_gather(p.tri_data, p.mats, p.texels, hu, hv, hidx);
            out[0] = make_float4(g.albedo.x, g.albedo.y, g.albedo.z, t);
            out[1] = make_float4(g.nrm.x, g.nrm.y, g.nrm.z, g.transparency);
            out[2] = make_float4(g.emissive.x, g.emissive.y, g.emissive.z, 0.0f);
        }
    }
    if (STATS) {
        const unsigned long long s1 = wave_sum(n_cells), s2 = wave_sum(n_tests);
        if (lane == 0) {
            atomicAdd(&p.stats[1], s1);
            atomicAdd(&p.stats[2], s2);
        }
    }
    const unsigned long long s3 = wave_sum(n_hits);
    if (lane == 0 && s3 != 0ull) atomicAdd(&p.stats[3], s3);
}

// The planes a call asked for (null: not asked), n_owned entries each.
struct FeaturePlanes {
    float *base_color, *normal, *emissive, *depth, *transparency;
    uint32_t* hits;
};
// The ordered per-pixel sums, wf_resolve_kernel's shape: a block takes kResPix
// pixels and loads their records kResSmp samples at a time, consecutive lanes
// on consecutive float4 of the items (a pixel's 16 records: a 768-byte run),
// parks the eleven values of each in LDS, and one thread per pixel then adds
// them in sample order, a miss adding nothing.  Between passes the sums and
// the count wait in acc (three float4 per pixel, the record's layout with the
// count's bits in the last word); the last pass scales by 1 / spp
// (stage3.zig:223, :242) and writes the planes asked for.
constexpr uint32_t kFeatVals = 11, kFeatRow = kResSmp * kFeatVals + 1;   // +1: no LDS bank conflict
__global__ __launch_bounds__(kBlock) void feature_resolve_kernel(const float4* __restrict__ rec, uint32_t P, uint32_t S,
                                                                 float4* acc, int first, int last, float inv_spp,
                                                                 const FeaturePlanes out) {
    __shared__ float s_r[kResPix * kFeatRow];
    const uint32_t q0 = blockIdx.x * kResPix;
    const uint32_t np = min(kResPix, P - q0);
    const uint32_t tid = threadIdx.x;
    const uint32_t q = q0 + tid;
    v3 bc = mk(0, 0, 0), nr = mk(0, 0, 0), em = mk(0, 0, 0);
    float dp = 0.0f, tr = 0.0f;
    uint32_t nh = 0;
    if (tid < np && !first) {
        const float4 a0 = acc[3ull * q], a1 = acc[3ull * q + 1], a2 = acc[3ull * q + 2];
        bc = mk(a0.x, a0.y, a0.z); dp = a0.w;
        nr = mk(a1.x, a1.y, a1.z); tr = a1.w;
        em = mk(a2.x, a2.y, a2.z); nh = __float_as_uint(a2.w);
    }
    for (uint32_t c = 0; c < S; c += kResSmp) {
        const uint32_t ns = min(kResSmp, S - c);
        for (uint32_t m = tid; m < kResPix * kResSmp * 3u; m += kBlock) {
            const uint32_t i = m / (kResSmp * 3u), k3 = m % (kResSmp * 3u);   // the block's pixel i, word k3 of its run
            if (i < np && k3 < 3u * ns) {
                const float4 v = rec[3ull * ((uint64_t)(q0 + i) * S + c) + k3];
                const uint32_t k = k3 / 3u, f = k3 % 3u;                      // sample c + k, its word f
                float* dst = s_r + i * kFeatRow + kFeatVals * k + 4u * f;
                dst[0] = v.x; dst[1] = v.y; dst[2] = v.z;
                if (f < 2u) dst[3] = v.w;
            }
        }
        __syncthreads();
        if (tid < np) {
            const float* src = s_r + tid * kFeatRow;
            for (uint32_t k = 0; k < ns; ++k, src += kFeatVals) {
                if (src[3] == kInf) continue;                                // a miss: its other words are stale
                bc = add(bc, mk(src[0], src[1], src[2]));
                dp += src[3];
                nr = add(nr, mk(src[4], src[5], src[6]));
                tr += src[7];
                em = add(em, mk(src[8], src[9], src[10]));
                ++nh;
            }
        }
        __syncthreads();
    }
    if (tid >= np) return;
    if (!last) {
        acc[3ull * q] = make_float4(bc.x, bc.y, bc.z, dp);
        acc[3ull * q + 1] = make_float4(nr.x, nr.y, nr.z, tr);
        acc[3ull * q + 2] = make_float4(em.x, em.y, em.z, __uint_as_float(nh));
        return;
    }
    const v3 inv = mk(inv_spp, inv_spp, inv_spp);
    auto put3 = [&](float* plane, v3 sum) {
        const v3 l = mul(sum, inv);
        plane[3 * (size_t)q] = l.x; plane[3 * (size_t)q + 1] = l.y; plane[3 * (size_t)q + 2] = l.z;
    };
    if (out.base_color) put3(out.base_color, bc);
    if (out.normal) put3(out.normal, nr);
    if (out.emissive) put3(out.emissive, em);
    if (out.depth) out.depth[q] = dp * inv_spp;
    if (out.transparency) out.transparency[q] = tr * inv_spp;
    if (out.hits) out.hits[q] = nh;
}

using FeatureFn = void (*)(const FeatureParams);
// staging of a pass unasked: 4 GiB of item records (zrt_context_features)
constexpr uint64_t kFeatStageBytes = 4ull << 30, kFeatItemBytes = 48;

// ---------------------------------------------------------------------------
// Transmittance queries (zrt_context_transmittance): the expected
// value of the path tracer's pass-through chain (stage3.zig:207-212) along a
// bounded ray.  Per ray: T = 1, n = 0, then closest-mode bounded segments
// (trace_ray BOUNDED, or the park kernel's kParkClosest mode), each hit's alpha
// a = material.transparency.sample(texcoord) folded in as p = 1 - a -- opaque
// or NaN ends the chain at T = +0, else T *= min(p, 1) -- and the next segment
// started at ray.at(t + eps) with the bound shortened by t + eps, until a miss
// or max_crossings crossings.  Every loop over crossings, on the device and on
// the host, is also bounded by max_crossings (1..256, checked by the entry
// point): at large coordinates o + d * s can round back to o.
struct TransmitParams {
    QueryParams q;            // rays, bounds, n, which, ctr; q.w.t the scene; the park path: q.w.hit, q.w.n_in8
    float* T;                 // this chunk: the transmittance of every ray
    uint32_t* cross;          // this chunk: the crossings of every ray (the lane path: or null)
    uint32_t max_cross;       // 1..256
    uint32_t first;           // transmit_step_kernel: the chunk's first round (T = 1, n = 0 are not read)
    const float4* q_in;       // transmit_step_kernel: the queue the park kernel just traced
    float4* q_out;            //   and the one the surviving rays go to, with its region counts
    uint32_t* n_out8;
};
// The alpha at a hit.  The arithmetic is surface_kernel's / shade_segment's
// (their lines `w0`, `tc0`, `tc1` and the transparency sample), restated here
// with only the loads the alpha needs -- Data words d2 and d3, the material,
// texture 2: keep the three in step.
__device__ __forceinline__ float transmit_alpha(const TraceParams& p, float hu, float hv, uint32_t ref) {
    const float4* tdp = p.tri_data + 4ull * ref;
    const float4 d2 = tdp[2], d3 = tdp[3];                          // stage3.zig:199-206
    const float w0 = 1.0f - hu - hv;
    const float tc0 = (d2.y * w0 + d2.w * hu) + d3.y * hv;
    const float tc1 = (d2.z * w0 + d3.x * hu) + d3.z * hv;
    const DevMat& m = p.mats[__float_as_uint(d3.w)];
    return sample1(p.texels, m.tex[2], tc0, tc1);
}
// One crossing at parameter t with alpha a.  True: the chain goes on from
// (o, bound) as updated -- `no = o + d * (t + kFltEps)` as surface_kernel and
// shade_segment compute it, the same operations in the same order.
__device__ __forceinline__ bool transmit_cross(float a, float t, uint32_t cap, v3& o, v3 d, float& bound, float& T,
                                               uint32_t& n) {
    ++n;
    const float pp = 1.0f - a;
    if (!(pp > 0.0f)) {                                             // opaque, or a NaN alpha: `!(U > NaN)` scatters too
        T = 0.0f;
        return false;
    }
    T = T * fminf(pp, 1.0f);
    if (n == cap) return false;
    const float s = t + kFltEps;
    o = add(o, scale(d, s));
    bound = bound - s;                                              // (+inf stays +inf; <= 0: the next segment misses)
    return true;
}

// The lane path: query_walk_kernel<.., SEG = true> with the whole chain of a
// ray in its lane, one launch for every crossing (same `which` split, same
// walk variants, same work counters).  Segments and crossings are counted in
// every call (stats[0], stats[3]); STATS adds cells and tests, each segment
// counted as a closest-mode counting segment call counts it.
// `which` = kRaysQueue (the park path's tail): the rays are the live entries of
// a queue transmit_step_kernel appended -- (o_k, ray) (d, b_k), T and n so far
// in r.T / r.cross -- and their chains are finished here, k starting at n.
constexpr uint32_t kRaysQueue = 3;
// Slot j of a queue of nq slots (P = nq, S = 1): its region g, and whether
// that region's count (n8) reaches it.
__device__ __forceinline__ bool queue_slot_live(uint32_t nq, const uint32_t* n8, uint32_t j, uint32_t& g) {
    g = 0;
    for (uint32_t k = 1; k < 8u; ++k) g += j >= xcd_q0(nq, k) ? 1u : 0u;
    return j < nq && j - xcd_q0(nq, g) < n8[g * kCtr];
}
// 5 waves per SIMD: at query_walk_kernel's 6 (80 VGPRs) the chain state around
// the walk spills 3-7 VGPRs in the three fast instantiations; at 5 none does.
constexpr int kTransmitMinWaves = 5;
template <bool STATS, bool PACKED, bool PK_BM, bool MTX>
__global__ __launch_bounds__(kTraceBlock, STATS ? 1 : kTransmitMinWaves) void transmit_walk_kernel(const TransmitParams r) {
    const TraceParams& p = r.q.w.t;
    extern __shared__ __attribute__((aligned(16))) uint32_t s_occ[];
    __shared__ uint32_t s_wcnt[2 * (kTraceBlock / 64)];
    if (r.q.which == kRaysRest && r.q.ctr[2] == 0u) return;         // (the whole grid: nothing left)
    for (uint32_t i = threadIdx.x; i < p.occ_words; i += blockDim.x) s_occ[i] = p.occ[i];
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const bool tail = r.q.which == kRaysQueue;                      // (uniform)
    uint32_t* const work = r.q.ctr + (r.q.which == kRaysRest ? 1u : tail ? 3u : 0u);
    uint64_t prof[11] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t n_seg = 0, n_cells = 0, n_tests = 0, n_hits = 0, n_rest = 0;
    for (;;) {
        uint32_t base = 0;
        if (lane == 0) base = atomicAdd(work, 64u * kWfChunk);
        base = __builtin_amdgcn_readfirstlane(base);
        if (base >= r.q.n) break;
        for (uint32_t sub = 0; sub < kWfChunk; ++sub) {
            uint32_t i = base + 64u * sub + lane;                   // the ray; the tail: the queue slot, then its ray
            if (i >= r.q.n) continue;
            v3 o, d;
            float bound, T = 1.0f;
            uint32_t n = 0;
            if (tail) {
                uint32_t g;
                if (!queue_slot_live(r.q.n, r.q.w.n_in8, i, g)) continue;
                const float4 qa = r.q_in[3ull * i], qb = r.q_in[3ull * i + 1];
                o = mk(qa.x, qa.y, qa.z);
                d = mk(qb.x, qb.y, qb.z);
                bound = qb.w;
                i = __float_as_uint(qa.w);
                if (i >= r.q.n) continue;                           // (never: no store without it)
                T = r.T[i];
                n = r.cross[i];
                n_hits -= n;                                        // (counted by the rounds before)
            } else {
                ray_load(r.q.rays, i, o, d);
                const bool fast = ray_fast(d);
                if (r.q.which == kRaysFast && !fast) { ++n_rest; continue; }
                if (r.q.which == kRaysRest && fast) continue;
                bound = query_bound(r.q, i);
            }
            for (uint32_t k = n; k < r.max_cross; ++k) {
                float hu = 0.0f, hv = 0.0f;
                uint32_t hidx = 0;
                const float t = trace_ray<STATS, kTriBatch, PACKED, PK_BM, MTX, false, true>(p, s_occ, o, d, hu, hv, hidx,
                                                                                             n_cells, n_tests, prof, s_wcnt,
                                                                                             -kInf, kInf, bound);
                ++n_seg;
                if (__float_as_uint(t) == __float_as_uint(bound)) break;       // a miss (trace_ray, NEAREST0)
                if (!transmit_cross(transmit_alpha(p, hu, hv, hidx), t, r.max_cross, o, d, bound, T, n)) break;
            }
            n_hits += n;
            r.T[i] = T;
            if (r.cross) r.cross[i] = n;
        }
    }
    if (r.q.which == kRaysFast) {
        const unsigned long long s = wave_sum(n_rest);
        if (lane == 0 && s != 0ull) atomicAdd(&r.q.ctr[2], (uint32_t)s);
    }
    const unsigned long long s0 = wave_sum(n_seg), s3 = wave_sum(n_hits);
    if (lane == 0 && s0 != 0ull) atomicAdd(&p.stats[0], s0);
    if (lane == 0 && s3 != 0ull) atomicAdd(&p.stats[3], s3);
    if (STATS) {
        const unsigned long long s1 = wave_sum(n_cells), s2 = wave_sum(n_tests);
        if (lane == 0) {
            atomicAdd(&p.stats[1], s1);
            atomicAdd(&p.stats[2], s2);
        }
    }
}

// The park path's step between two park launches: one thread per slot of the
// queue the park kernel just traced (region g holds q.w.n_in8[g] entries from
// xcd_q0(n, g) on, as query_pack_kernel left them or as this kernel's previous
// round appended them).  A live entry's hit record (q.w.hit[slot]) is folded
// into T and n of its ray (the record's item word), and a chain that goes on is
// appended to the same region of the other queue as (o', ray) (d, bound'):
// region g never receives more than it held, so it fits.  The order inside a
// region is free, results are per ray.  Rays outside the fast domain were
// walked by the park kernel like any ray and are dropped here, T and n
// untouched: the kRaysRest launch of the lane path owns their chains.  A
// wave's 64 slots lie in one region (region bounds are multiples of 64 or n).
// Returns at once on an empty queue.
__global__ __launch_bounds__(kBlock) void transmit_step_kernel(const TransmitParams r) {
    __shared__ uint32_t s_cnt[2];
    const WfParams& w = r.q.w;
    const uint32_t nq = r.q.n;
    uint32_t live_any = 0;
    for (uint32_t g = 0; g < 8u; ++g) live_any |= w.n_in8[g * kCtr];
    if (live_any == 0u) return;                                     // (uniform over the grid)
    if (threadIdx.x < 2u) s_cnt[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    uint32_t g;
    bool live = queue_slot_live(nq, w.n_in8, j, g);
    v3 o = mk(0, 0, 0), d = mk(0, 0, 0);
    float bound = 0.0f;
    uint32_t i = 0;
    if (live) {
        const float4 qa = r.q_in[3ull * j], qb = r.q_in[3ull * j + 1];
        o = mk(qa.x, qa.y, qa.z);
        d = mk(qb.x, qb.y, qb.z);
        i = __float_as_uint(qa.w);
        bound = qb.w;
        live = ray_fast(d) && i < nq;                               // (i < nq: holds for every record written; no store without it)
    }
    bool cont = false;
    uint32_t hit = 0;
    if (live) {
        const float4 h = w.hit[j];
        const uint32_t ref = __float_as_uint(h.w);
        float T = r.first ? 1.0f : r.T[i];
        uint32_t n = r.first ? 0u : r.cross[i];
        if (ref != 0xFFFFFFFFu) {                                   // (a miss: the park kernel's kParkClosest record)
            hit = 1u;
            cont = transmit_cross(transmit_alpha(w.t, h.y, h.z, ref), h.x, r.max_cross, o, d, bound, T, n);
        }
        r.T[i] = T;
        r.cross[i] = n;
    }
    // append the survivors: one returning atomic per region of the wave (wf_append's scheme)
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t below = (1ull << lane) - 1ull;
    uint64_t pend = __ballot(cont);
    while (pend) {
        const uint32_t lead = (uint32_t)__builtin_ctzll(pend);
        const uint32_t gl = (uint32_t)__builtin_amdgcn_readlane((int)g, (int)lead);
        const uint64_t m = __ballot(cont && g == gl);
        uint32_t ob = 0;
        if (lane == lead) ob = atomicAdd(&r.n_out8[gl * kCtr], (uint32_t)__popcll(m));
        ob = (uint32_t)__builtin_amdgcn_readlane((int)ob, (int)lead) + xcd_q0(nq, gl);
        if (cont && g == gl) {
            const uint32_t pos = ob + (uint32_t)__popcll(m & below);
            if (pos < xcd_q0(nq, gl + 1u)) {                        // (always: a region receives at most what it held)
                r.q_out[3ull * pos] = make_float4(o.x, o.y, o.z, __uint_as_float(i));
                r.q_out[3ull * pos + 1] = make_float4(d.x, d.y, d.z, bound);
            }
        }
        pend &= ~m;
    }
    const unsigned long long s0 = wave_sum(live ? 1u : 0u), s3 = wave_sum(hit);
    if (lane == 0) {
        if (s0 != 0ull) atomicAdd(&s_cnt[0], (uint32_t)s0);
        if (s3 != 0ull) atomicAdd(&s_cnt[1], (uint32_t)s3);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_cnt[0] != 0u) atomicAdd(&w.t.stats[0], (unsigned long long)s_cnt[0]);
        if (s_cnt[1] != 0u) atomicAdd(&w.t.stats[3], (unsigned long long)s_cnt[1]);
    }
}

// The park path's tail: once a round leaves this many rays or fewer under way,
// one kRaysQueue launch of the lane kernel finishes their chains instead of
// further (park, step) rounds, whose fixed cost per round (the park workgroups'
// LDS fill, two launches and the read-back) outweighs the park kernel's
// advantage on few rays (tools/transmit_bench.py).
// ZRT_TRANSMIT_TAIL in the environment overrides it (0: never), for that bench
// and for the tests that run every round.
constexpr uint64_t kTransmitTailMax = 1ull << 16;
using TransmitFn = void (*)(const TransmitParams);
// walk: brick-major packed, packed, wide, the IEEE division, counting (QueryKernels' order)
const TransmitFn kTransmitWalk[5] = {(TransmitFn)transmit_walk_kernel<false, true, true, false>,
                                     (TransmitFn)transmit_walk_kernel<false, true, false, false>,
                                     (TransmitFn)transmit_walk_kernel<false, false, false, false>,
                                     (TransmitFn)transmit_walk_kernel<false, false, false, true>,
                                     (TransmitFn)transmit_walk_kernel<true, false, false, true>};

// ---------------------------------------------------------------------------
// Occlusion queries (zrt_context_occlusion): per ray the number of
// S hemisphere samples at its first hit that meet something within a radius.
// A sample is the direction the path tracer scatters along (stage3.zig:214,
// shade_segment's `normalize_rn(add(nrm, normalize_rn(...)))`) from the start of
// the stream (seed, key, s), as a bounded segment from zrt_surface.position.
// An item is a (ray, sample) pair; a chunk's items run in sub-chunks of at most
// kOccItems, item j of a sub-chunk being (ray0 + (s0 + j) / S, (s0 + j) % S).
// occlusion_gen_kernel makes the segments of the items that can be occluded --
// the ray hit and the sample is traced (include/zrt.h) -- and leaves the others
// out, so that no walk, counting or timed, ever sees them:
//   the park path: an item of the fast domain (ray_fast) is appended to the
//   region of queue slot j (P = m, S = 1) as (o, j) (d, bound), which
//   wf_park_kernel's bounded closest mode reads as it stands;
//   every other live item, and every live item of the lane path, is appended to
//   a list of plain rays, bounds and item indices that the query_walk_kernel
//   SEG instantiations walk as a segment call's.
// The appends are wf_append's: a ballot, one returning atomic per wave (and
// region), ranks by popcount.  The order inside a region or the list is free:
// occlusion_reduce_kernel adds an occluded item to its ray's count, and integer
// sums do not depend on the order.  ctr[4] counts the list, ctr[5] every live
// item; the host reads both back per sub-chunk (the list launches' size, and
// zrt_stats.segments).
struct OcclusionParams {
    const float* rays;        // this chunk: 6 floats per ray (origin, direction as given)
    const uint32_t* hits;     // this chunk: the zrt_hit of every ray as 4 u32 (4-byte aligned)
    const float* radius;      // this chunk: a bound per ray, or null: radius_all
    float radius_all;
    uint32_t S;               // samples per ray, 1..65535
    const float4* tri_data;   // TraceParams::tri_data
    const DevMat* mats;
    const float* texels;
    const double* zig;        // the ziggurat's tables (TraceParams::zig)
    uint64_t seed;
    uint32_t key0;            // RNG stream key of the chunk's ray 0; keys wrap at 2^32
    uint32_t n;               // rays of this chunk
    uint32_t nl;              // occlusion_reduce_kernel, kOccList: the list's entries
    uint32_t ray0, s0;        // the sub-chunk's first item: sample s0 of ray ray0
    uint32_t m;               // items of this sub-chunk (<= kOccItems)
    uint32_t park;            // occlusion_gen_kernel: items of the fast domain go to the queue
    uint32_t mode;            // occlusion_reduce_kernel: kOccQueue, kOccList or kOccFinish
    float4* q;                // the queue (m slots) and its region counts
    uint32_t* n_in8;
    const float4* hit;        // the park kernel's hit record per queue slot
    float* irays;             // the list: 6 floats, a bound and an item index per entry
    float* ibound;
    uint32_t* iitem;
    const uint8_t* occ;       // the lane walk's byte per list entry
    uint32_t* ctr;            // [4]: entries of the list, [5]: live items
    uint32_t* occluded;       // this chunk: the occluded samples of every ray so far
    float* visibility;        // this chunk, or null
    unsigned long long* stats;   // [kOccStat]: the occluded samples of the call
};
constexpr uint32_t kOccItems = 1u << 20;       // items per sub-chunk
constexpr uint32_t kOccGenItems = 4;           // items per thread of occlusion_gen_kernel
constexpr uint32_t kOccQueue = 0, kOccList = 1, kOccFinish = 2;
constexpr uint32_t kOccStat = 16;              // (stats[0..3] are the walk kernels', [0..15] the counting render's)

// A block takes kOccGenItems * kBlock consecutive items, a wave 64 consecutive
// ones at a time (one queue region: region bounds are multiples of 64 or m).
// The normal and the position are surface_kernel's: surface_gather's `nrm`
// (the texel loads it does not use fall away) and `add(o, scale(d, t + eps))`.
__global__ __launch_bounds__(kBlock) void occlusion_gen_kernel(const OcclusionParams r) {
    __shared__ double s_zig[514];
    for (uint32_t i = threadIdx.x; i < 514; i += blockDim.x) s_zig[i] = r.zig[i];
    __syncthreads();
    const double* zx = s_zig;
    const double* zf = s_zig + 257;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t below = (1ull << lane) - 1ull;
    const bool aligned = (reinterpret_cast<uintptr_t>(r.hits) & 15u) == 0u;   // (uniform: the context's own records always are)
    for (uint32_t k = 0; k < kOccGenItems; ++k) {
        const uint32_t j = (blockIdx.x * kOccGenItems + k) * kBlock + threadIdx.x;
        if (__ballot(j < r.m) == 0ull) break;                                   // (wave-uniform)
        bool live = false;
        v3 o = mk(0, 0, 0), d = mk(0, 0, 0);
        float bound = 0.0f;
        if (j < r.m) {
            const uint32_t L = j + r.s0, ql = L / r.S;
            const uint32_t ray = r.ray0 + ql, s = L - ql * r.S;
            uint4 h = make_uint4(0x7F800000u, 0u, 0u, 0xFFFFFFFFu);
            if (ray < r.n) {                                                    // (always: m items of n rays)
                if (aligned) {
                    h = reinterpret_cast<const uint4*>(r.hits)[ray];
                } else {
                    const uint32_t* hq = r.hits + 4ull * ray;
                    h = make_uint4(hq[0], hq[1], hq[2], hq[3]);
                }
            }
            const float t = __uint_as_float(h.x);
            if (t != kInf) {                                                    // a hit (query_store)
                v3 ro, rd;
                ray_load(r.rays, ray, ro, rd);
                const SurfaceInputs g = surface_gather(r.tri_data, r.mats, r.texels, __uint_as_float(h.y),
                                                       __uint_as_float(h.z), h.w);
                o = add(ro, scale(rd, t + kFltEps));
                Rng rng;
                rng.s = path_key(r.seed, r.key0 + ray, s);
                const float nx = (float)rng_norm64(rng, zx, zf);
                const float ny = (float)rng_norm64(rng, zx, zf);
                const float nz = (float)rng_norm64(rng, zx, zf);
                d = normalize_rn(add(g.nrm, normalize_rn(mk(nx, ny, nz))));
                live = finite3(o) && finite3(d) && (d.x != 0.0f || d.y != 0.0f || d.z != 0.0f);
                bound = r.radius ? r.radius[ray] : r.radius_all;
            }
        }
        const bool to_q = live && r.park != 0u && ray_fast(d);
        const bool to_l = live && !to_q;
        const uint64_t ma = __ballot(live);
        if (ma != 0ull && lane == (uint32_t)__builtin_ctzll(ma)) atomicAdd(&r.ctr[5], (uint32_t)__popcll(ma));
        const uint64_t ml = __ballot(to_l);
        if (ml != 0ull) {
            const uint32_t lead = (uint32_t)__builtin_ctzll(ml);
            uint32_t ob = 0;
            if (lane == lead) ob = atomicAdd(&r.ctr[4], (uint32_t)__popcll(ml));
            ob = (uint32_t)__builtin_amdgcn_readlane((int)ob, (int)lead);
            const uint32_t pos = ob + (uint32_t)__popcll(ml & below);
            if (to_l && pos < r.m) {                                            // (always: at most m live items)
                float* q = r.irays + 6ull * pos;
                q[0] = o.x; q[1] = o.y; q[2] = o.z;
                q[3] = d.x; q[4] = d.y; q[5] = d.z;
                r.ibound[pos] = bound;
                r.iitem[pos] = j;
            }
        }
        // the queue: region g of slot j receives at most the items of its own slots
        uint32_t g = 0;
        for (uint32_t x = 1; x < 8u; ++x) g += j >= xcd_q0(r.m, x) ? 1u : 0u;
        uint64_t pend = __ballot(to_q);
        while (pend) {
            const uint32_t lead = (uint32_t)__builtin_ctzll(pend);
            const uint32_t gl = (uint32_t)__builtin_amdgcn_readlane((int)g, (int)lead);
            const uint64_t mq = __ballot(to_q && g == gl);
            uint32_t ob = 0;
            if (lane == lead) ob = atomicAdd(&r.n_in8[gl * kCtr], (uint32_t)__popcll(mq));
            ob = (uint32_t)__builtin_amdgcn_readlane((int)ob, (int)lead) + xcd_q0(r.m, gl);
            if (to_q && g == gl) {
                const uint32_t pos = ob + (uint32_t)__popcll(mq & below);
                if (pos < xcd_q0(r.m, gl + 1u)) {                               // (always)
                    r.q[3ull * pos] = make_float4(o.x, o.y, o.z, __uint_as_float(j));
                    r.q[3ull * pos + 1] = make_float4(d.x, d.y, d.z, bound);
                }
            }
            pend &= ~mq;
        }
    }
}

// kOccQueue: one thread per queue slot of the sub-chunk, the park kernel's hit
// record of a live slot (a miss: the ref at 0xFFFFFFFF); kOccList: one thread
// per list entry, the lane walk's byte.  An occluded item adds one to its ray's
// count -- with S >= 64 a wave's items are a few rays', and each distinct ray of
// the wave takes one atomic; below that one per item -- and the block's total
// goes to stats[kOccStat] with one atomic.  kOccFinish, once per chunk after
// its last sub-chunk: one thread per ray, visibility = (S - occluded) / S by
// the IEEE division.
__global__ __launch_bounds__(kBlock) void occlusion_reduce_kernel(const OcclusionParams r) {
    __shared__ uint32_t s_n;
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (r.mode == kOccFinish) {
        if (i < r.n && r.visibility) r.visibility[i] = (float)(r.S - r.occluded[i]) / (float)r.S;
        return;
    }
    if (threadIdx.x == 0) s_n = 0u;
    __syncthreads();
    bool hit = false;
    uint32_t j = 0;
    if (r.mode == kOccQueue) {
        uint32_t g;
        if (queue_slot_live(r.m, r.n_in8, i, g)) {
            j = __float_as_uint(r.q[3ull * i].w);
            hit = __float_as_uint(r.hit[i].w) != 0xFFFFFFFFu;
        }
    } else if (i < r.nl) {
        j = r.iitem[i];
        hit = r.occ[i] != (uint8_t)0;
    }
    const uint32_t ray = r.ray0 + (j + r.s0) / r.S;
    hit = hit && ray < r.n;                                         // (always: no store without it)
    const uint32_t lane = threadIdx.x & 63u;
    if (r.S >= 64u) {
        uint64_t pend = __ballot(hit);
        while (pend) {
            const uint32_t lead = (uint32_t)__builtin_ctzll(pend);
            const uint32_t rl = (uint32_t)__builtin_amdgcn_readlane((int)ray, (int)lead);
            const uint64_t mr = __ballot(hit && ray == rl);
            if (lane == lead) atomicAdd(&r.occluded[rl], (uint32_t)__popcll(mr));
            pend &= ~mr;
        }
    } else if (hit) {
        atomicAdd(&r.occluded[ray], 1u);
    }
    const unsigned long long s = wave_sum(hit ? 1u : 0u);
    if (lane == 0 && s != 0ull) atomicAdd(&s_n, (uint32_t)s);
    __syncthreads();
    if (threadIdx.x == 0 && s_n != 0u) atomicAdd(&r.stats[kOccStat], (unsigned long long)s_n);
}
// total items (rays x samples) from which a call takes the park path unasked
// for its samples (ZRT_TRACE_PARK forces it, ZRT_FLAG_LANE_WALK forbids it;
// the first hits follow zrt_context_trace's kTraceParkMin): 2^16, the smallest
// size tools/occlusion_bench.py measures; there, at 2^18 and at 2^20 the park
// path won in both rounds on cfg3 and the Cornell box at both radii, at 2^16 by
// 26% and by 2-14% (profiles/occlusion_bench.json, samples_lane / samples_park)
constexpr uint64_t kOccParkMin = kSegParkMin;

// ---------------------------------------------------------------------------
// Direct-light queries (zrt_context_direct): per ray the
// irradiance of L punctual lights at its first hit, each light shadowed by the
// transmittance chain of the segment towards it, and the Lambertian radiance
// that irradiance gives.  An item is a (ray, light) pair; a chunk's items run
// in sub-chunks of at most kDirItems, item j of a sub-chunk being
// (ray0 + (s0 + j) / L, (s0 + j) % L).  direct_gen_kernel computes the item's
// direction w, bound b and factor f (include/zrt.h) and appends the traced
// items -- the ray hit and is shaded, the light is in front of the surface and,
// a spot, inside its cone -- to a list of plain rays and bounds that the
// transmit_walk_kernel instantiations walk as a transmittance call's, T of a
// list entry landing at its slot; the others are never walked and never
// counted.  The append is wf_append's: a ballot, one returning atomic per wave,
// ranks by popcount.  The order inside the list is free: every item keeps its
// factor and its slot (0xFFFFFFFF: not traced) in two dense rows, and
// direct_reduce_kernel, one thread per ray, walks the ray's items of the
// sub-chunk in light order and folds colour * (f * T) into the ray's running E,
// which waits in the chunk's irradiance row between sub-chunks: a ray whose
// lights straddle a cut is summed in the same order as any other.  ctr[4]
// counts the list; the host reads it back per sub-chunk (the walk launches'
// size, and zrt_stats.samples).
struct DirectParams {
    const float* rays;        // this chunk: 6 floats per ray (origin, direction as given)
    const uint32_t* hits;     // this chunk: the zrt_hit of every ray as 4 u32 (4-byte aligned)
    const float4* tri_data;   // TraceParams::tri_data
    const DevMat* mats;
    const float* texels;
    const zrt_light* lights;  // L lights, on the device
    uint32_t L;               // lights per ray, 1..65535
    uint32_t n;               // rays of this chunk
    uint32_t ray0, s0;        // the sub-chunk's first item: light s0 of ray ray0
    uint32_t m;               // items of this sub-chunk (<= kDirItems)
    uint32_t unshadowed;      // ZRT_DIRECT_UNSHADOWED: no list is written, T = 1
    uint32_t fold;            // direct_reduce_kernel: the walk launches ran; move their counts
    float* irays;             // the list: 6 floats and a bound per entry
    float* ibound;
    const float* T;           // the walk's transmittance per list entry
    float* f;                 // the factor of every item of the sub-chunk
    uint32_t* slot;           //   and its list entry, or 0xFFFFFFFF
    uint32_t* ctr;            // [4]: entries of the list
    float* E;                 // this chunk: the irradiance of every ray, 3 floats
    float* radiance;          // this chunk: 3 floats per ray, or null
    unsigned long long* stats;   // [kDirStat]: the chains' segments, [kDirStat + 1]: their crossings
};
constexpr uint32_t kDirItems = 1u << 20;       // items per sub-chunk
constexpr uint32_t kDirGenItems = 4;           // items per thread of direct_gen_kernel
constexpr uint32_t kDirStat = 16;              // (stats[0..3] are the walk kernels', [0..15] the counting render's)

// A block takes kDirGenItems * kBlock consecutive items, a wave 64 consecutive
// ones at a time.  The normal and the position are surface_kernel's:
// surface_gather's `nrm` (the texel loads it does not use fall away) and
// `add(o, scale(d, t + eps))`.  The divisions and the square root are IEEE's.
__global__ __launch_bounds__(kBlock) void direct_gen_kernel(const DirectParams r) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t below = (1ull << lane) - 1ull;
    const bool aligned = (reinterpret_cast<uintptr_t>(r.hits) & 15u) == 0u;   // (uniform: the context's own records always are)
    for (uint32_t k = 0; k < kDirGenItems; ++k) {
        const uint32_t j = (blockIdx.x * kDirGenItems + k) * kBlock + threadIdx.x;
        if (__ballot(j < r.m) == 0ull) break;                                   // (wave-uniform)
        bool live = false;
        v3 o = mk(0, 0, 0), w = mk(0, 0, 0);
        float bound = 0.0f, f = 0.0f;
        if (j < r.m) {
            const uint32_t I = j + r.s0, qr = I / r.L;
            const uint32_t ray = r.ray0 + qr, l = I - qr * r.L;
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
                    const zrt_light& lt = r.lights[l];
                    float d2 = 1.0f;
                    if (lt.type == ZRT_LIGHT_DIRECTIONAL) {
                        w = normalize_rn(mk(-lt.direction[0], -lt.direction[1], -lt.direction[2]));
                        bound = kInf;
                    } else {
                        const v3 v = sub(ld3(lt.position), o);
                        d2 = dot(v, v);
                        w = normalize_rn(v);
                        bound = length(v);
                    }
                    const float c = dot(N, w);
                    live = c > 0.0f;                                            // (false for a NaN)
                    f = lt.type == ZRT_LIGHT_DIRECTIONAL ? c : c / d2;
                    if (lt.type == ZRT_LIGHT_SPOT) {
                        const float s = -dot(normalize_rn(ld3(lt.direction)), w);
                        const float kk = fminf(fmaxf(s * lt.angle_scale + lt.angle_offset, 0.0f), 1.0f);
                        f = f * (kk * kk);
                        live = live && kk > 0.0f;
                    }
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
            r.f[j] = pos != 0xFFFFFFFFu ? f : 0.0f;
            r.slot[j] = pos;
        }
    }
}

// One thread per ray of the sub-chunk, ray0 + i: its items [a, e) of the
// sub-chunk in light order.  E starts at +0 with the ray's light 0 and is read
// back from the row otherwise; an item that is not traced adds nothing.  With
// the ray's last light, and `radiance` asked, the surface is gathered once more
// for its base colour and emission.  Thread 0 moves the walk launches' segment
// and crossing counts (stats[0], stats[3], which the first hits' kernels also
// add to and the host cleared after them) to the call's own two.
__global__ __launch_bounds__(kBlock) void direct_reduce_kernel(const DirectParams r) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i == 0u && r.fold != 0u) {
        r.stats[kDirStat] += r.stats[0];
        r.stats[kDirStat + 1] += r.stats[3];
        r.stats[0] = 0ull;
        r.stats[3] = 0ull;
    }
    const uint32_t end = r.s0 + r.m;                                            // (< 2^21: s0 < L < 2^16)
    const uint32_t ray = r.ray0 + i;
    if ((uint64_t)i * r.L >= end || ray >= r.n) return;                         // (ray < n: always)
    const uint32_t first = i * r.L;
    const uint32_t a = max(first, r.s0), e = min(first + r.L, end);
    const bool aligned = (reinterpret_cast<uintptr_t>(r.hits) & 15u) == 0u;
    const uint4 h = hit_load(r.hits, aligned, ray);
    const float t = __uint_as_float(h.x);
    float* const Ep = r.E + 3ull * ray;
    v3 E = mk(0.0f, 0.0f, 0.0f);
    if (t != kInf) {
        if (a != first) E = ld3(Ep);
        for (uint32_t x = a; x < e; ++x) {
            const uint32_t j = x - r.s0, s = r.slot[j];
            if (s == 0xFFFFFFFFu) continue;
            const float T = r.unshadowed != 0u ? 1.0f : r.T[s];
            const float g = r.f[j] * T;
            const zrt_light& lt = r.lights[x - first];
            E = add(E, scale(ld3(lt.color), g));
        }
    }
    Ep[0] = E.x; Ep[1] = E.y; Ep[2] = E.z;
    if (e != first + r.L || !r.radiance) return;
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

// ---------------------------------------------------------------------------
// Radiance queries (zrt_context_radiance): Scene.traceRayRecursive
// (stage3.zig:188-220) for caller-given rays, S samples each, through the
// render's own queues, park, shade and resolve kernels.  A chunk
// of n rays is a "frame" of P = n pixels in one pass of S samples: item =
// ray * S + s, pixel-major, so the XCD regions, the bounce planes and the
// resolve are a render's.  What a render does not have is S paths that start
// with the SAME ray (its samples are jittered): their first segment is one
// Scene.traceRay call, traced once per ray -- as zrt_context_trace traces a
// chunk -- and fanned out into S shaded continuations (rad_fanout_kernel).
struct RadParams {
    WfParams w;               // w.t: P = n rays, S samples per ray; queues, planes, counters of the launch
    const float* rays;        // this chunk: 6 floats per ray (origin, direction as given)
    float* nrays;             // rad_pack_kernel: the rays with their directions normalised, 6 floats each
                              // (query_walk_kernel's input)
    float4* q;                // the pack kernels: the queue they fill (launch 0's q_in)
    uint32_t* n_in8;          //   and its region counts
    uint32_t* ctr;            // [2]: rays outside the fast domain (query_walk_kernel, kRaysRest)
    uint32_t n;               // rays of this chunk
    uint32_t key0;            // RNG stream key ("pixel") of the chunk's ray 0; keys wrap at 2^32
};

// Camera.getRay (stage3.zig:27-35) for the camera lower_left_corner = d,
// right = up = 0: d + right * x + up * y adds +0 twice (x, y >= 0: the
// products are +0; a -0 component becomes +0), then camera_ray's normalize.
__device__ __forceinline__ v3 rad_direction(v3 d) {
    const v3 z = mk(0.0f, 0.0f, 0.0f);
    return normalize_rn(add(add(d, z), z));
}
// What camera_rng leaves for (pixel key, sample s): the stream after the two
// jitter draws.
__device__ __forceinline__ Rng rad_rng(uint64_t seed, uint32_t key, uint32_t s) {
    Rng rng;
    rng.s = path_key(seed, key, s);
    (void)rng_float(rng);
    (void)rng_float(rng);
    return rng;
}

// One thread per ray: ray i, its direction normalised, as queue entry i of the
// identity layout (identity_queue_fill: P = n, S = 1) for the park kernel, and
// as six floats for the lane walk.  A normalised direction is in the fast domain
// (ray_fast) unless the given one was NaN, infinite, zero or of a squared
// length that overflows or vanishes; those are counted for the kRaysRest launch.
__global__ __launch_bounds__(kBlock) void rad_pack_kernel(const RadParams r) {
    identity_queue_fill(r.q, r.n_in8, r.ctr, r.n, [&](uint32_t i, v3& o, v3& d, float& w) {
        ray_load(r.rays, i, o, d);
        d = rad_direction(d);
        float* q = r.nrays + 6ull * i;
        q[0] = o.x; q[1] = o.y; q[2] = o.z;
        q[3] = d.x; q[4] = d.y; q[5] = d.z;
        w = __uint_as_float(1u);
    });
}

// ZRT_RADIANCE_PER_SAMPLE: one thread per item = ray * S + s, its path record
// as queue entry `item` (region g of the identity layout with P = n, S = S is
// full: S paths per ray of pixel range g): depth max_bounce, slot 0, no scatter
// yet, the stream after its two jitter draws.  Launch 0 then runs over them as
// a bounce launch does.
__global__ __launch_bounds__(kBlock) void rad_pack_samples_kernel(const RadParams r) {
    const TraceParams& p = r.w.t;
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;          // (items of a chunk stay below 2^31)
    if (i < 8u) r.n_in8[i * kCtr] = p.S * (xcd_q0(r.n, i + 1u) - xcd_q0(r.n, i));
    if (i >= p.total) return;
    const uint32_t ray = div_by(i, p.sdiv);
    const uint32_t s = i - ray * p.S;
    v3 o, d;
    ray_load(r.rays, ray, o, d);
    d = rad_direction(d);
    const Rng rng = rad_rng(p.seed, r.key0 + ray, s);
    r.q[3ull * i] = make_float4(o.x, o.y, o.z, __uint_as_float(i));
    r.q[3ull * i + 1] = make_float4(d.x, d.y, d.z, __uint_as_float(p.max_bounce));
    r.q[3ull * i + 2] = make_float4(__uint_as_float((uint32_t)rng.s), __uint_as_float((uint32_t)(rng.s >> 32)),
                                    __uint_as_float(0u), 0.0f);
}

// The fan-out: traceRayRecursive's body after the first traceRay
// (stage3.zig:195-219) for the S paths of every ray, from the ONE hit record
// (t, u, v, ref) its first segment left in w.hit[ray] and its normalised ray
// in queue entry `ray` of w.q_in.  Items ray * S + s are fetched per XCD group
// like a primary launch's (wf_fetch<PRIMARY>, P = n), so a wave of 64 samples
// of one ray reads one hit record, one ray and one triangle record (every
// lane the same address: one request), and its terminal and bounce-plane
// stores are contiguous.  Each lane builds the stream of (ray, s) and shades:
// a path that ends writes term[item], one that goes on writes its bounce plane
// (shade_segment) and joins region g of the bounce-1 queue.  LMATS, LAST: as
// wf_shade_kernel (LAST: max_bounce == 1, the terminal radiance only).
// n_seg counts the segment traced, once per ray.
template <bool LMATS, bool LAST>
__global__ __launch_bounds__(kTraceBlock, 1) void rad_fanout_kernel(const RadParams r) {
    const WfParams& w = r.w;
    const TraceParams& p = w.t;
    __shared__ double s_zig[514];
    extern __shared__ __attribute__((aligned(16))) uint32_t s_dynm[];    // LMATS: p.nmat DevMat
    DevMat* const s_mats = reinterpret_cast<DevMat*>(s_dynm);
    for (uint32_t i = threadIdx.x; i < 514; i += blockDim.x) s_zig[i] = p.zig[i];
    if (LMATS)
        for (uint32_t i = threadIdx.x; i < p.nmat * (uint32_t)(sizeof(DevMat) / 4); i += blockDim.x)
            reinterpret_cast<uint32_t*>(s_mats)[i] = reinterpret_cast<const uint32_t*>(p.mats)[i];
    __syncthreads();
    const DevMat* const mats = LMATS ? s_mats : p.mats;
    const double* zx = s_zig;
    const double* zf = s_zig + 257;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t below = lane ? (~0ull >> (64u - lane)) : 0ull;
    uint32_t n_seg = 0;
    uint32_t grp = blockIdx.x & 7u, tried = 0;
    for (;;) {
        uint32_t base = 0, lim = 0;
        if (!wf_fetch<true>(w, 64u * kWfChunk, grp, tried, base, lim)) break;
        for (uint32_t sub = 0; sub < kWfChunk && base + 64u * sub < lim; ++sub) {
            const uint32_t j = base + 64u * sub + lane;
            bool cont = false;
            uint32_t item = 0, depth = 0, slot = 0, mask = 0;
            v3 o = mk(0, 0, 0), d = mk(0, 0, 0);
            Rng rng;
            rng.s = 0;
            if (j < lim) {
                item = ent_index<true>(w, grp, j);
                const uint32_t ray = div_by(item, p.sdiv);
                const uint32_t s = item - ray * p.S;
                const float4 a = w.q_in[3ull * ray], b = w.q_in[3ull * ray + 1], h = w.hit[ray];
                o = mk(a.x, a.y, a.z);
                d = mk(b.x, b.y, b.z);
                rng = rad_rng(p.seed, r.key0 + ray, s);
                depth = p.max_bounce;                              // >= 1 (the host never launches this at 0)
                n_seg += s == 0u ? 1u : 0u;
                v3 L = mk(0, 0, 0);
                cont = shade_segment<LAST>(w, zx, zf, mats, item, h.x, h.y, h.z, tri_rec(p, h.x, __float_as_uint(h.w)),
                                           o, d, depth, slot, rng, mask, L);
                if (!cont) w.term[item] = make_float4(L.x, L.y, L.z, __uint_as_float(mask));
            }
            if (!LAST) wf_append(w, cont, below, o, d, item, depth, slot, rng, mask, grp);
        }
    }
    const unsigned long long s0 = wave_sum(n_seg);
    if (lane == 0) atomicAdd(&p.stats[0], s0);
}

// ---------------------------------------------------------------------------
// Light-probe queries (zrt_context_light_probes): per probe
// position the order-2 SH projection of the radiance zrt_context_radiance
// computes along D directions made on the device, the first hits' distance
// moments and their count.  An item is a (probe, direction) pair; a chunk's n
// items are the radiance call's n rays: item i of a chunk that starts at
// direction j0 of probe p0 is (p0 + (j0 + i) / D, (j0 + i) % D), its stream key
// key0 + i.  light_probe_gen_kernel writes the chunk's ray row, which
// rad_pack_kernel, the first segments, rad_fanout_kernel, the bounce launches
// and wf_resolve_kernel then run over as they stand.
// light_probe_reduce_kernel has two modes:
//   kLpTake, right after the fan-out (the first segments' records in w.hit are
//   valid until bounce launch 1's park kernel reuses the array): t of every
//   item copied to a 4-byte row, kLpTakeItems items per thread, and the hits of
//   the call counted with one atomic per block (one per wave of 64 items took
//   0.2 ms of a 2^20-item chunk on one address);
//   kLpFold, after the resolve: 32 lanes per probe of the chunk, lane 3 * k + c
//   the sum A[k][c], lane 27 T1, lane 28 T2, lane 29 n; every lane walks its
//   probe's items of the chunk in direction order, 32 at a time: the half-wave
//   loads a tile of L_j, d_j and t into LDS, one item per lane, and every lane
//   reads the items from there.  A sum starts at +0 where the probe's direction 0
//   lies in this chunk and is read back from the carry row `carry_in` otherwise
//   -- only a chunk's first probe can have begun before it; only its last can
//   go on after it, and leaves its sums in `carry_out`.  The two are different
//   rows, which the host swaps from chunk to chunk: in a chunk whose first
//   probe reads and whose last probe writes, the two half-waves run in no order.
//   A probe whose last direction was added is scaled and stored.  So a probe
//   whose directions straddle a cut, or many cuts, is summed in the same order
//   as any other.
struct LightProbeParams {
    const float* pos;         // 3 floats per probe, from the chunk's first probe p0 on
    float* rays;              // the chunk's ray row: 6 floats per item (x_p, d_j)
    float* dirs;              // this chunk: d_j, 3 floats per item, or null
    const double* zig;        // the ziggurat's tables (TraceParams::zig)
    uint64_t seed;
    uint32_t key0;            // RNG stream key of the chunk's item 0; keys wrap at 2^32
    uint32_t D;               // directions per probe, 1..65535
    uint32_t j0;              // the chunk's item 0 is direction j0 of probe p0
    uint32_t n;               // items of this chunk (<= kTraceChunk)
    uint32_t np;              // probes with an item in this chunk
    uint32_t mode;            // light_probe_reduce_kernel: kLpTake or kLpFold
    const float4* hit;        // kLpTake: the first segments' records, one per item
    float* t;                 // the chunk's first-hit distances, one per item (+inf: a miss)
    const float* lin;         // kLpFold: L_j, 3 floats per item (wf_resolve_kernel's linear row)
    const float* carry_in;    // 32 words: the sums of the probe the previous chunk left unfinished
    float* carry_out;         // 32 words, another row: the sums of a probe that goes on in the next chunk
    float* sh;                // from probe p0 on: 27 floats per probe, or null
    float* dist;              //   2 floats per probe, or null
    uint32_t* hits;           //   a count per probe, or null
    unsigned long long* stats;   // [kLpStat]: the hits of the call
};
constexpr uint32_t kLpGenItems = 4;            // items per thread of light_probe_gen_kernel
constexpr uint32_t kLpTakeItems = 8;           // items per thread of light_probe_reduce_kernel, kLpTake
constexpr uint32_t kLpTake = 0, kLpFold = 1;
constexpr uint32_t kLpStat = 16;               // (stats[0..3] are the walk kernels', [0..15] the counting render's)
constexpr uint32_t kLpDirSample = 65535;       // the sample index of a direction's stream: never a path's
constexpr float kLpFourPi = 0x1.921fb6p+3f;    // 4 pi rounded to f32, 0x41490FDB
constexpr float kShC0 = 0x1.20dd76p-2f, kShC1 = 0x1.f45438p-2f, kShC2 = 0x1.17b142p+0f, kShC3 = 0x1.42f602p-2f,
                kShC4 = 0x1.17b142p-1f;

// A block takes kLpGenItems * kBlock consecutive items.  The direction is
// Vec3.randomUnitVector from the start of the stream (seed, key, 65535), as
// occlusion_gen_kernel draws a sample's.
__global__ __launch_bounds__(kBlock) void light_probe_gen_kernel(const LightProbeParams r) {
    __shared__ double s_zig[514];
    for (uint32_t i = threadIdx.x; i < 514; i += blockDim.x) s_zig[i] = r.zig[i];
    __syncthreads();
    const double* zx = s_zig;
    const double* zf = s_zig + 257;
    for (uint32_t k = 0; k < kLpGenItems; ++k) {
        const uint32_t i = (blockIdx.x * kLpGenItems + k) * kBlock + threadIdx.x;
        if (i >= r.n) break;
        const uint32_t q = (i + r.j0) / r.D;                                    // (i + j0 < 2^20 + 2^16)
        if (q >= r.np) break;                                                   // (never: n items of np probes)
        const float* x = r.pos + 3ull * q;
        Rng rng;
        rng.s = path_key(r.seed, r.key0 + i, kLpDirSample);
        const float nx = (float)rng_norm64(rng, zx, zf);
        const float ny = (float)rng_norm64(rng, zx, zf);
        const float nz = (float)rng_norm64(rng, zx, zf);
        const v3 d = normalize_rn(mk(nx, ny, nz));
        float* o = r.rays + 6ull * i;
        o[0] = x[0]; o[1] = x[1]; o[2] = x[2];
        o[3] = d.x; o[4] = d.y; o[5] = d.z;
        if (r.dirs) {
            float* w = r.dirs + 3ull * i;
            w[0] = d.x; w[1] = d.y; w[2] = d.z;
        }
    }
}

__global__ __launch_bounds__(kBlock) void light_probe_reduce_kernel(const LightProbeParams r) {
    __shared__ uint32_t s_n;
    __shared__ __attribute__((aligned(16))) float s_tile[kBlock / 32][32][8];
    const uint32_t lane = threadIdx.x & 63u;
    if (r.mode == kLpTake) {
        if (threadIdx.x == 0) s_n = 0u;
        __syncthreads();
        uint32_t n_hit = 0;
        for (uint32_t k = 0; k < kLpTakeItems; ++k) {
            const uint32_t i = (blockIdx.x * kLpTakeItems + k) * kBlock + threadIdx.x;
            if (i >= r.n) break;
            const float t = r.hit[i].x;
            r.t[i] = t;
            n_hit += t != kInf ? 1u : 0u;
        }
        const unsigned long long s = wave_sum(n_hit);
        if (lane == 0 && s != 0ull) atomicAdd(&s_n, (uint32_t)s);
        __syncthreads();
        if (threadIdx.x == 0 && s_n != 0u) atomicAdd(&r.stats[kLpStat], (unsigned long long)s_n);
        return;
    }
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    const uint32_t q = i >> 5, l = i & 31u;
    if (q >= r.np) return;                                                      // (a whole half-wave)
    const uint32_t first = q * r.D, end = r.j0 + r.n;                           // (q * D <= j0 + n < 2^21)
    const uint32_t a = max(first, r.j0), e = min(first + r.D, end);
    const uint32_t kk = l / 3u, c = min(l - 3u * kk, 2u);
    const bool is_sh = l < 27u;
    float acc = 0.0f;
    uint32_t cnt = 0u;
    if (a != first && l < 30u) {
        acc = r.carry_in[l];
        cnt = __float_as_uint(acc);
    }
    // a tile of 32 items: lane l of the half-wave loads item x0 + l (coalesced
    // rows) and lays it into the half-wave's LDS tile as (d, t) (L, -); then
    // every lane takes the tile's items in order, every read one address or
    // three per half-wave.  The next tile's loads are in flight meanwhile.  The
    // lanes of a half-wave run in lockstep (one wave, one control flow): a
    // tile's writes are done before its reads, its reads before the next writes.
    float(*const tile)[8] = s_tile[threadIdx.x >> 5];
    struct Item { float4 dt, L; };
    auto load = [&](uint32_t x0) {
        Item m = {make_float4(0.0f, 0.0f, 0.0f, kInf), make_float4(0.0f, 0.0f, 0.0f, 0.0f)};
        const uint32_t x = x0 + l;
        if (x < e) {
            const uint32_t it = x - r.j0;
            const float* dp = r.rays + 6ull * it + 3;
            const float* lp = r.lin + 3ull * it;
            m.dt = make_float4(dp[0], dp[1], dp[2], r.t[it]);
            m.L = make_float4(lp[0], lp[1], lp[2], 0.0f);
        }
        return m;
    };
    Item cur = load(a);
    for (uint32_t x0 = a; x0 < e; x0 += 32u) {
        *reinterpret_cast<float4*>(&tile[l][0]) = cur.dt;
        *reinterpret_cast<float4*>(&tile[l][4]) = cur.L;
        __builtin_amdgcn_wave_barrier();
        cur = load(x0 + 32u);
        const uint32_t m = min(32u, e - x0);
#pragma unroll 4
        for (uint32_t s = 0; s < m; ++s) {
            const float4 dt = *reinterpret_cast<const float4*>(&tile[s][0]);
            const float Lc = tile[s][4 + c];
            const float dx = dt.x, dy = dt.y, dz = dt.z, t = dt.w;
            // all nine, then the lane's own: selects, no branch
            const float y1 = kShC1 * dy, y2 = kShC1 * dz, y3 = kShC1 * dx;
            const float y4 = (kShC2 * dx) * dy, y5 = (kShC2 * dy) * dz, y7 = (kShC2 * dx) * dz;
            const float y6 = kShC3 * ((3.0f * (dz * dz)) - 1.0f);
            const float y8 = kShC4 * ((dx * dx) - (dy * dy));
            float Y = kk == 0u ? kShC0 : kk == 1u ? y1 : kk == 2u ? y2 : kk == 3u ? y3 : y4;
            Y = kk == 5u ? y5 : kk == 6u ? y6 : kk == 7u ? y7 : kk == 8u ? y8 : Y;
            const float term = is_sh ? Lc * Y : l == 27u ? t : t * t;
            const bool hit = t != kInf;
            acc = is_sh || hit ? acc + term : acc;
            cnt += hit ? 1u : 0u;
        }
        __builtin_amdgcn_wave_barrier();
    }
    if (l >= 30u) return;
    if (e != first + r.D) {                                                     // goes on in the next chunk
        r.carry_out[l] = l == 29u ? __uint_as_float(cnt) : acc;
        return;
    }
    const float fD = (float)r.D;
    if (l < 27u) {
        if (r.sh) r.sh[27ull * q + l] = acc * (kLpFourPi / fD);
    } else if (l < 29u) {
        if (r.dist) r.dist[2ull * q + (l - 27u)] = acc * (1.0f / fD);
    } else if (r.hits) {
        r.hits[q] = cnt;
    }
}

using RadFn = void (*)(const RadParams);
constexpr uint32_t kRadianceFlags = ZRT_FLAG_LANE_WALK | ZRT_FLAG_MT_EXACT | ZRT_FLAG_ESCAPE | ZRT_FLAG_NO_ESCAPE |
                                    ZRT_FLAG_RELEASE | ZRT_FLAG_NO_RELEASE | ZRT_FLAG_BFCULL | ZRT_FLAG_NO_BFCULL |
                                    ZRT_FLAG_HOP | ZRT_FLAG_NO_HOP | ZRT_TRACE_PARK | ZRT_RADIANCE_PER_SAMPLE;

// max_bounce picks the stack depth the counting kernel is compiled for.
TraceFn count_fn(uint32_t max_bounce) {
    if (max_bounce <= 4) return (TraceFn)trace_kernel<4>;
    if (max_bounce <= 8) return (TraceFn)trace_kernel<8>;
    if (max_bounce <= 16) return (TraceFn)trace_kernel<16>;
    if (max_bounce <= 32) return (TraceFn)trace_kernel<32>;
    return nullptr;
}

// pass sets in flight (streams) by default, and at most (ZRT_SWEEP: ZRT_SETS)
constexpr uint32_t kPassSets = 2;
constexpr uint64_t kSetsMinSamples = 1ull << 23;   // samples of a frame that runs kPassSets
constexpr uint64_t kFrustumMinSamples = 1ull << 23; // samples of a frame that computes the frustum bounds
// % of a pass moved from the last pass to the first when two sets run (r02d7,
// vs 0: 20% cfg3 +3.2%, cfg5 +0.2%, cfg2 -1.0%; 16% cfg3 +1.4%; 25% cfg3
// +3.2%, cfg2 -1.7%; the response is bumpy: r02d5/d6 sweeps)
#ifndef ZRT_LEAD_PCT
#define ZRT_LEAD_PCT 20
#endif
constexpr uint32_t kLeadPct = ZRT_LEAD_PCT;

}  // namespace

// The timed wf_kernel instantiations, as the substrings of their mangled
// names that tools/spill_check.py / tests/test_codegen.py look for in the
// gfx950 code object (primary launch, then bounce launches).  No HIP call.
extern "C" const char* zrt_timed_kernels(void) {
#define ZRT_STR2(x) #x
#define ZRT_STR(x) ZRT_STR2(x)
    // the default launch set: primary wf_kernel, then per bounce the
    // trace-only park kernel + the whole-wave shade kernel (or wf_kernel when
    // the scene's OccX does not fit the LDS)
    // (brick-major packed words, then field words: dda.h)
    // (the last bool of wf_kernel: MTX, the IEEE-division instantiations
    // of the scenes with edges of 2^62 or more, not timed)
    return "wf_kernelILi" ZRT_STR(ZRT_WF_MINW0) "ELb1ELb1ELb1ELb0EE,wf_kernelILi" ZRT_STR(ZRT_WF_MINW0)
           "ELb1ELb1ELb0ELb0EE,"
           // (the park kernel's last argument: the query mode, a render's first,
           // then zrt_context_segments', under the same rules)
           "wf_park_kernelILb1ELb1ELi0E,wf_park_kernelILb0ELb1ELi0E,wf_park_kernelILb1ELb0ELi0E,wf_park_kernelILb0ELb0ELi0E,"
           "wf_park_kernelILb1ELb1ELi1E,wf_park_kernelILb0ELb1ELi1E,wf_park_kernelILb1ELb0ELi1E,wf_park_kernelILb0ELb0ELi1E,"
           "wf_shade_kernelILb1ELb0EE,wf_shade_kernelILb1ELb1EE,wf_kernelILi" ZRT_STR(ZRT_WF_MINW) "ELb0ELb1ELb1ELb0EE,wf_kernelILi" ZRT_STR(
               ZRT_WF_MINW) "ELb0ELb1ELb0ELb0EE,"
           // zrt_context_features' walk (STATS, PACKED, PK_BM, MTX), under the primary's rules
           "feature_walk_kernelILb0ELb1ELb1ELb0EE,feature_walk_kernelILb0ELb1ELb0ELb0EE";
#undef ZRT_STR
#undef ZRT_STR2
}

// Load this unit's code object on the current device (zrt_device_warmup).
int render_warmup() {
    hipFuncAttributes fa;
    HIP_TRY(hipFuncGetAttributes(&fa, (const void*)resolve_kernel));
    return ZRT_OK;
}

// The grid and scene part of a launch's TraceParams (everything but the
// camera, the pass and the output fields, which are left zero).
static void scene_params(const zrt_context* c, TraceParams& tp) {
    memset(&tp, 0, sizeof tp);
    for (int i = 0; i < 3; ++i) {
        tp.bmin[i] = c->grid.bbox_min[i];
        tp.bmax[i] = c->grid.bbox_max[i];
        tp.res[i] = c->grid.resolution[i];
        tp.cs[i] = c->grid.cell_size[i];
        tp.ics[i] = 1.0f / c->grid.cell_size[i];          // IEEE: RN(1 / cs)
    }
    tp.cs_ok = 1u;
    for (int i = 0; i < 3; ++i)
        if (!(fabsf(tp.cs[i]) >= 0x1p-32f && fabsf(tp.cs[i]) <= 0x1p32f)) tp.cs_ok = 0u;
    tp.cells = c->d_cells;
    tp.pk = c->pk;
    tp.cell32 = c->d_cell32;
    {
        const uint32_t sh = c->occ_shift, b[3] = {c->pk.b0, c->pk.b1, c->pk.b2};
        tp.occ_w0 = b[0] > sh ? b[0] - sh : 0u;
        tp.occ_w1 = b[1] > sh ? b[1] - sh : 0u;
        tp.occ_w2 = b[2] > sh ? b[2] - sh : 0u;
        auto lowbits = [&](int a) { return (1u << std::min(sh, b[a])) - 1u; };
        tp.occ_o1 = c->pk.o1 + sh;
        tp.occ_o2 = c->pk.o2 + sh;
        // (brick-major words: occupancy bricks of 4^3, the word's low six bits)
        tp.occ_lowm = c->pk.bm ? 63u : lowbits(0) | (lowbits(1) << c->pk.o1) | (lowbits(2) << c->pk.o2);
        tp.ox1 = c->pk.o1 + 2u;
        tp.ox2 = c->pk.o2 + 2u;
        tp.ow0 = b[0] - 2u;
        tp.ow1 = b[1] - 2u;
        tp.ow2 = b[2] - 2u;
    }
    tp.tri_pos = c->d_pos;
    tp.tri_data = c->d_data;
    tp.mats = c->d_mats;
    tp.nmat = c->nmat;
    tp.texels = c->d_texels;
    tp.zig = c->d_zig;
    tp.occ = c->d_occ;
    tp.bmask = c->d_bmask;
    tp.occ_shift = c->occ_shift;
    tp.occ_nb0 = c->occ_nb[0];
    tp.occ_nb01 = c->occ_nb[0] * c->occ_nb[1];
    tp.occ_words = c->occ_words;
}

// ---------------------------------------------------------------------------
// The launch plan.  zrt_context_render, zrt_context_trace and
// zrt_context_radiance launch the same park, shade and lane-walk kernels over
// the same pass-set buffers.  What they decide alike before a launch, and the
// layout the kernels expect of a set's queues and counters, is written once
// here; an entry point keeps only what is its own.

// `v` grown to n events.
static int event_pool(std::vector<hipEvent_t>& v, size_t n, unsigned flags = hipEventDefault) {
    while (v.size() < n) {
        hipEvent_t e;
        HIP_TRY(hipEventCreateWithFlags(&e, flags));
        v.push_back(e);
    }
    return ZRT_OK;
}

// Blocks of a persistent launch of `f`: what the device holds at once.
static int resident_blocks(const zrt_context* c, const void* f, int threads, size_t lds, uint32_t* blocks) {
    int bpc = 0;
    HIP_TRY(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&bpc, f, threads, lds));
    if (getenv("ZRT_WF_DEBUG"))
        fprintf(stderr, "{\"zrt_grid\": {\"threads\": %d, \"lds\": %zu, \"blocks_per_cu\": %d}}\n", threads, lds, bpc);
    bpc = std::max(1, std::min(bpc, 2048 / threads));
    *blocks = (uint32_t)(c->num_cus * bpc);
    return ZRT_OK;
}

// The device memory a call may spend on its work buffers: 144 GiB (HBM is
// 288 GB), at most 60% of the free device memory, shared between the contexts
// of a group on this device.  `held`: the bytes of grow-only buffers the
// context already holds and this call reuses, counted as free: otherwise a
// split would depend on the calls before (a warm context saw less free memory
// and rendered 3 passes on 2 sets, the last one alone).  A call reads it
// before it grows any buffer.
static size_t device_budget(const zrt_context* c, size_t held) {
    size_t budget = (size_t)144 << 30;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b) budget = std::min(budget, (free_b + held) / 10 * 6);
    return budget / std::max<uint32_t>(c->mem_share, 1u);
}

// The bytes of a pass set's wavefront buffers.
static size_t held_bytes(const zrt_context::PassSet& ps) {
    return 16ull * (ps.q0_cap + ps.q1_cap + ps.term_cap + ps.stk4_cap + ps.hit_cap) + 8ull * ps.stk2_cap +
           4ull * ps.wfc_cap;
}

// Capacity guard: every buffer a launch writes holds what that launch writes
// (round 2's counting render once wrote through an unallocated d_out after a
// refactor of the pass logic; a stale, smaller buffer must not pass silently
// either).  True if `ptr` does not hold `need` elements.
static bool shortfall(const char* what, const void* ptr, size_t cap, uint64_t need) {
    if (ptr && cap >= need) return false;
    if (getenv("ZRT_DEBUG"))
        fprintf(stderr, "zrt: capacity guard: %s holds %zu, the launch writes %llu\n", what, ptr ? cap : 0,
                (unsigned long long)need);
    return true;
}

// A pass set's counters, kCtr words each (a contract with the kernels): per
// launch k = 0 .. max_bounce + 1, 8 work counters, then 8 region counts of the
// paths entering launch k (written by launch k - 1); after those, 8 work
// counters of launch k's shade kernel.
static size_t wfc_words(uint32_t mb) { return kCtr * 2ull * (16 * (mb + 2)); }
static uint32_t* region_counts(const zrt_context::PassSet& ps, uint32_t k) { return ps.wfc + kCtr * (16 * k + 8); }

// Launch k of a pass: the queue it reads and the one it appends to (ping-pong;
// launch 0 reads q1), and its counters.
static void bounce_params(WfParams& W, const zrt_context::PassSet& ps, uint32_t k, uint32_t mb) {
    W.q_in = (k & 1) ? ps.q0 : ps.q1;
    W.q_out = (k & 1) ? ps.q1 : ps.q0;
    W.fetch8 = ps.wfc + kCtr * (16 * k);
    W.n_in8 = region_counts(ps, k);
    W.n_out8 = region_counts(ps, k + 1);
    W.fetch8s = ps.wfc + wfc_words(mb) / 2 + kCtr * (8 * k);
}

// A pass set's wavefront buffers grown to T items of nb bounce slots each and
// the counters of max_bounce mb, then the capacity guard over them.  Queues 3
// float4 per item, bounce planes a float4 + a float2 per (slot, item), terminal
// radiance 1 per item; `hit_items` hit records (the park kernel hands one per
// item to the shade kernel; a query's first segments leave one per ray), 0: none.
static int grow_pass_set(zrt_context::PassSet& ps, uint64_t T, uint32_t nb, uint32_t mb, uint64_t hit_items) {
    const uint64_t planes2 = T * nb * 2;
    int rc;
    if ((rc = grow(&ps.q0, &ps.q0_cap, 3 * T)) != ZRT_OK) return rc;
    if ((rc = grow(&ps.q1, &ps.q1_cap, 3 * T)) != ZRT_OK) return rc;
    if ((rc = grow(&ps.term, &ps.term_cap, T)) != ZRT_OK) return rc;
    if ((rc = grow(&ps.stk4, &ps.stk4_cap, T * nb)) != ZRT_OK) return rc;
    if ((rc = grow(&ps.stk2, &ps.stk2_cap, planes2)) != ZRT_OK) return rc;
    if ((rc = grow(&ps.wfc, &ps.wfc_cap, wfc_words(mb))) != ZRT_OK) return rc;
    if (hit_items && (rc = grow(&ps.hit, &ps.hit_cap, hit_items)) != ZRT_OK) return rc;
    const bool bad = shortfall("q0", ps.q0, ps.q0_cap, 3 * T) || shortfall("q1", ps.q1, ps.q1_cap, 3 * T) ||
                     shortfall("term", ps.term, ps.term_cap, T) || shortfall("planes4", ps.stk4, ps.stk4_cap, T * nb) ||
                     shortfall("planes2", ps.stk2, ps.stk2_cap, planes2) ||
                     shortfall("counters", ps.wfc, ps.wfc_cap, wfc_words(mb)) ||
                     (hit_items && shortfall("hit records", ps.hit, ps.hit_cap, hit_items));
    return bad ? ZRT_ERR_INVALID_ARG : ZRT_OK;
}

// What a call's flags and the context settle for its bounce launches.
struct LaunchPlan {
    bool mtx;                 // Moller-Trumbore with the IEEE division in every launch (kWf*Exact)
    bool packed, pbm;         // packed walk state; brick-major packed words (dda.h)
    bool park_ok;             // the context and the flags allow the park kernel
    bool park;                //   ... and this call launches it
    bool rel, esc, bfc, hop;  // the park launches use the release, the escape table, the cull masks, the hop
    WfFn f_park, f_walk;      // a bounce launch: the park kernel (+ the shading half), or the lane walk
    WfFn s_next, s_last;      // the shading half; of a pass's last bounce (terminal radiance only, LAST)
    int park_block;           // threads of a park workgroup
    uint32_t occx_ldsw;       // u32 words OccX takes in LDS
    size_t lds_wf, lds_park, lds_shade;
    // the park schedule (WfParams): parked lanes before a test round, finished
    // lanes before a shade + refill round, the release's two thresholds
    uint32_t test_min, refill_min, rel_min, rel_emin;
};

// The park kernel of a plan (escape table, word layout) in query mode QM.
template <int QM>
static WfFn park_fn(bool esc, bool pbm) {
    return pbm ? (esc ? (WfFn)wf_park_kernel<true, true, QM> : (WfFn)wf_park_kernel<false, true, QM>)
               : (esc ? (WfFn)wf_park_kernel<true, false, QM> : (WfFn)wf_park_kernel<false, false, QM>);
}

static void plan_park_block(LaunchPlan& pl, int block) {
    pl.park_block = block;
    pl.lds_park = 4ull * pl.occx_ldsw + (size_t)(block / 64) * sizeof(ParkSlot);
}

// Kernel per bounce launch: the park kernel (traces, writes hit records) +
// wf_shade_kernel (incoherent rays) when the scene's OccX fits the LDS budget
// (the park walk packs a cell into one word: at most 1024 cells per axis);
// else, and with ZRT_FLAG_LANE_WALK, wf_kernel (round 1's path, and the
// fallback).  mtx: scenes whose edges leave the short reciprocal's domain, or
// as the flag forces: the unpacked lane walk.
// `want_park`: what the entry point asks besides (a small query takes the lane
// walk unasked); `big`: a call of kSetsMinSamples samples or more.
// The escape table and the back-face cull masks are built here, at the first
// big call that parks or the first a flag forces: 2.5 ms on cfg3 at 384 bins
// and 35 ms more for its region table where the launches use it (r10d), more
// than the table saves a 3-spp 1080p frame.  Each is used where
// the scene's statistic says it pays (context_escape, context_bfcull) or as
// the flags force it; the image is the same either way.
static int resolve_plan(zrt_context* c, uint32_t flags, bool counting, bool want_park, bool big, LaunchPlan& pl) {
    int rc;
    pl.mtx = c->mt_exact || (flags & ZRT_FLAG_MT_EXACT);
    pl.packed = c->packed && !pl.mtx;
    pl.pbm = pl.packed && c->pk.bm;
    pl.park_ok = c->occx_ok && !counting && !(flags & ZRT_FLAG_LANE_WALK) && pl.packed;
    pl.park = pl.park_ok && want_park;
    // the park release (wf_park_kernel): where enough entry faces are empty
    // (context_packed), or as the flags force it (same image either way);
    // with it the test rounds start at 12 parked lanes instead of 14 (r06u,
    // in one process, images identical: cfg3 7004 vs 6979, cfg2 4795 vs
    // 4632 Mrays/s; 10: 6987 / 4815, 8: 6927 / 4748;
    // profiles/r06/r06u_knobs_release_trigger.log)
    pl.rel = !(flags & ZRT_FLAG_NO_RELEASE) && (c->rel_on || (flags & ZRT_FLAG_RELEASE));
    if (!c->esc_tried && pl.park && !(flags & ZRT_FLAG_NO_ESCAPE) && (big || (flags & ZRT_FLAG_ESCAPE))) {
        c->esc_tried = true;
        if ((rc = context_escape(c, (flags & ZRT_FLAG_ESCAPE) != 0)) != ZRT_OK) return rc;
    }
    pl.esc = c->d_esc && !(flags & ZRT_FLAG_NO_ESCAPE) && (c->esc_on || (flags & ZRT_FLAG_ESCAPE));
    if (pl.park && !(flags & ZRT_FLAG_NO_BFCULL)) {
        const bool forced = (flags & ZRT_FLAG_BFCULL) != 0;
        if (forced ? !c->bfc_tried_forced : (big && !c->bfc_tried)) {
            c->bfc_tried = true;
            c->bfc_tried_forced = c->bfc_tried_forced || forced;
            if ((rc = context_bfcull(c, forced)) != ZRT_OK) return rc;
        }
    }
    pl.bfc = c->d_bfc && !(flags & ZRT_FLAG_NO_BFCULL) && (c->bfc_on || (flags & ZRT_FLAG_BFCULL));
    // the hop (PARK_HOP): wherever the packed cell records exist, unless the
    // flags say otherwise (same image either way)
    pl.hop = !(flags & ZRT_FLAG_NO_HOP);
    pl.f_park = park_fn<kParkRender>(pl.esc, pl.pbm);
    pl.f_walk = pl.mtx ? kWfBounceExact : (pl.packed ? (pl.pbm ? kWfBounceBM : kWfBounce) : kWfBounceWide);
    const bool lmats = c->nmat <= kLdsMats;
    pl.s_next = lmats ? (WfFn)wf_shade_kernel<true> : (WfFn)wf_shade_kernel<false>;
    pl.s_last = lmats ? (WfFn)wf_shade_kernel<true, true> : (WfFn)wf_shade_kernel<false, true>;
    pl.lds_wf = 4ull * c->occ_words;
    pl.lds_shade = lmats ? c->nmat * sizeof(DevMat) : 0;
    pl.occx_ldsw = (uint32_t)occx_lds_words(c->occx_nbw, c->occx_moff, c->occx_words);
    plan_park_block(pl, kParkBlock);
    pl.test_min = pl.rel ? kParkTestMinRel : kParkTestMin;
    pl.refill_min = kParkRefillMin;
    pl.rel_min = pl.test_min;              // park release: the parked lanes with refs a round needs
    pl.rel_emin = 1;                       //   and the empty ones that make skipping it worth it
    return ZRT_OK;
}

// The park kernel's fields of a launch's WfParams: OccX, the schedule, the
// escape table and the cull masks.
static void park_params(const zrt_context* c, const LaunchPlan& pl, WfParams& W) {
    W.occx = c->d_occx;
    W.occx_words = c->occx_words;
    W.occx_ldsw = pl.occx_ldsw;
    W.occx_nbw = c->occx_nbw;
    W.occx_moff = c->occx_moff;
    W.occx_nb0 = c->occx_nb[0];
    W.occx_nb01 = c->occx_nb[0] * c->occx_nb[1];
    W.test_min = pl.test_min;
    W.refill_min = pl.refill_min;
    W.rel_min = pl.rel ? pl.rel_min : 0u;
    W.rel_emin = pl.rel_emin;
    W.hop = pl.hop ? kHopMaxRefs : 0u;
    W.esc = c->d_esc;
    W.esc_key = c->esc_key;
    W.bfc = pl.bfc ? c->d_bfc : nullptr;
    W.bfc_ones = c->bfc_bytes ? c->bfc_bytes / 4 - 1 : 0;
}

// The occupancy-sized persistent grids of a call's bounce launches.
struct BounceGrids {
    uint32_t park, shade, shade_last, walk;
};
static int bounce_grids(const zrt_context* c, const LaunchPlan& pl, bool park, bool walk, BounceGrids& g) {
    int rc;
    g = BounceGrids{};
    if (park) {
        if ((rc = resident_blocks(c, (const void*)pl.f_park, pl.park_block, pl.lds_park, &g.park)) != ZRT_OK) return rc;
        if ((rc = resident_blocks(c, (const void*)pl.s_next, kTraceThreads, pl.lds_shade, &g.shade)) != ZRT_OK) return rc;
        if ((rc = resident_blocks(c, (const void*)pl.s_last, kTraceThreads, pl.lds_shade, &g.shade_last)) != ZRT_OK)
            return rc;
    }
    if (walk && (rc = resident_blocks(c, (const void*)pl.f_walk, kTraceThreads, pl.lds_wf, &g.walk)) != ZRT_OK) return rc;
    return ZRT_OK;
}

// ZRT_FLAG_KERNEL_TIMES: an event pair of the context's pool around every
// kernel launch of a render, and the launch's class; the launches per class
// are counted either way.
struct KernelTimes {
    zrt_context* c;
    bool on;
    size_t n = 0;                              // kernels timed
    zrt_kernel_profile kp{};
    int begin(int cls, hipStream_t sm) {
        ++kp.launches[cls];
        if (!on) return ZRT_OK;
        c->ev_k_cls[n] = (uint8_t)cls;
        HIP_TRY(hipEventRecord(c->ev_k[2 * n], sm));
        return ZRT_OK;
    }
    int end(hipStream_t sm) {
        if (!on) return ZRT_OK;
        HIP_TRY(hipEventRecord(c->ev_k[2 * n + 1], sm));
        ++n;
        return ZRT_OK;
    }
};

// A bounce launch on stream sm: the park kernel and the shading half of the
// same bounce (`last`: a pass's last), or the lane walk.  `kt`: a render's
// per-kernel events, or null.
static int launch_bounce(const LaunchPlan& pl, const BounceGrids& g, const WfParams& W, hipStream_t sm, bool park,
                         bool last, KernelTimes* kt) {
    int rc;
    if (kt && (rc = kt->begin(park ? ZRT_KERNEL_PARK : ZRT_KERNEL_BOUNCE, sm)) != ZRT_OK) return rc;
    if (park)
        hipLaunchKernelGGL(pl.f_park, dim3(g.park), dim3(pl.park_block), pl.lds_park, sm, W);
    else
        hipLaunchKernelGGL(pl.f_walk, dim3(g.walk), dim3(kTraceThreads), pl.lds_wf, sm, W);
    HIP_TRY(hipGetLastError());
    if (kt && (rc = kt->end(sm)) != ZRT_OK) return rc;
    if (!park) return ZRT_OK;
    if (kt && (rc = kt->begin(ZRT_KERNEL_SHADE, sm)) != ZRT_OK) return rc;
    if (last)
        hipLaunchKernelGGL(pl.s_last, dim3(g.shade_last), dim3(kTraceThreads), pl.lds_shade, sm, W);
    else
        hipLaunchKernelGGL(pl.s_next, dim3(g.shade), dim3(kTraceThreads), pl.lds_shade, sm, W);
    HIP_TRY(hipGetLastError());
    return kt ? kt->end(sm) : ZRT_OK;
}

// The launches that trace a query chunk's first segments, Scene.traceRay per
// ray: rays in the fast domain (ray_fast) through the park kernel or the
// context's fast lane walk, the others through the IEEE-division walk.
struct RayLaunch {
    QueryFn f_fast;           // null (mtx, a counting call): every ray takes f_exact
    QueryFn f_exact;
    QueryFn f_pack, f_out;    // the park path's queue fill and results
    uint32_t out_rays;        // rays per thread of f_out
    bool park;
    uint32_t grid_fast, grid_exact, grid_park;
    WfFn f_park;              // the plan's park kernel in this call's query mode
};
// `seg`: -1 a batch or radiance query, 0 / 1 a segment call in closest / any-hit form
static int ray_launch(const zrt_context* c, const LaunchPlan& pl, bool counting, bool park, RayLaunch& rl,
                      int seg = -1) {
    int rc;
    rl = RayLaunch{};
    const QueryKernels& k = kQuery[seg + 1];
    rl.park = park;
    // (any-hit calls: the closest park kernel, the yes / no kept)
    rl.f_park = seg >= 0 ? park_fn<kParkClosest>(pl.esc, pl.pbm) : pl.f_park;
    rl.f_fast = counting || pl.mtx ? nullptr : k.walk[pl.packed ? (pl.pbm ? 0 : 1) : 2];
    rl.f_exact = k.walk[counting ? 4 : 3];
    rl.f_pack = k.pack;
    rl.f_out = k.out;
    rl.out_rays = k.out_rays;
    // occupancy-sized persistent grids
    if (park && (rc = resident_blocks(c, (const void*)rl.f_park, pl.park_block, pl.lds_park, &rl.grid_park)) != ZRT_OK)
        return rc;
    if (rl.f_fast && !park &&
        (rc = resident_blocks(c, (const void*)rl.f_fast, kTraceThreads, pl.lds_wf, &rl.grid_fast)) != ZRT_OK)
        return rc;
    return resident_blocks(c, (const void*)rl.f_exact, kTraceThreads, pl.lds_wf, &rl.grid_exact);
}

// A chunk's n first segments on the context's stream, over the identity queue
// (ray i = entry i: P = n, S = 1) and the rays of Q: wf_park_kernel, or the
// fast lane walk, then the kRaysRest launch over the rays those left (it ends
// at once when they counted none); without a fast kernel the kRaysAll launch
// alone.  `pack_out`: Q.rays are the caller's rays as given, so
// query_pack_kernel fills the queue before the park kernel and
// query_out_kernel writes its hit records to Q.hits / Q.occ after it.
static void identity_queue(QueryParams& Q, uint32_t n) {
    Q.n = n;
    Q.w.t.P = n;
    Q.w.t.S = 1;
    Q.w.t.total = n;
    Q.w.t.sdiv = div_magic(1);
}
static int trace_first_segments(const zrt_context* c, const LaunchPlan& pl, const RayLaunch& rl, QueryParams& Q, uint32_t n,
                                bool pack_out, uint32_t* launches) {
    const uint32_t nblk = (n + kBlock - 1) / kBlock;             // one thread per ray; also all a walk launch needs
    identity_queue(Q, n);
    auto walk = [&](QueryFn f, uint32_t grid) {
        hipLaunchKernelGGL(f, dim3(std::min(grid, nblk)), dim3(kTraceThreads), pl.lds_wf, c->stream, Q);
    };
    if (rl.park) {
        Q.which = kRaysAll;
        if (pack_out) hipLaunchKernelGGL(rl.f_pack, dim3(nblk), dim3(kBlock), 0, c->stream, Q);
        hipLaunchKernelGGL(rl.f_park, dim3(rl.grid_park), dim3(pl.park_block), pl.lds_park, c->stream, Q.w);
        if (pack_out)
            hipLaunchKernelGGL(rl.f_out, dim3((nblk + rl.out_rays - 1) / rl.out_rays), dim3(kBlock), 0, c->stream, Q);
        *launches += pack_out ? 3 : 1;
    } else if (rl.f_fast) {
        Q.which = kRaysFast;
        walk(rl.f_fast, rl.grid_fast);
        ++*launches;
    }
    Q.which = rl.park || rl.f_fast ? kRaysRest : kRaysAll;
    walk(rl.f_exact, rl.grid_exact);
    ++*launches;
    HIP_TRY(hipGetLastError());
    return ZRT_OK;
}

// The lane kernels that walk whole transmittance chains (transmit_walk_kernel),
// chosen as ray_launch chooses a query's, and their occupancy-sized persistent
// grids; `grids` false: a call that launches none of them and so asks for none.
struct TransmitLaunch {
    TransmitFn f_fast;        // null (mtx, a counting call): every ray takes f_exact
    TransmitFn f_exact;
    uint32_t grid_fast, grid_exact;
};
static int transmit_launch(const zrt_context* c, const LaunchPlan& pl, bool counting, bool grids, TransmitLaunch& tl) {
    int rc;
    tl = TransmitLaunch{};
    tl.f_fast = counting || pl.mtx ? nullptr : kTransmitWalk[pl.packed ? (pl.pbm ? 0 : 1) : 2];
    tl.f_exact = kTransmitWalk[counting ? 4 : 3];
    if (!grids) return ZRT_OK;
    if (tl.f_fast && (rc = resident_blocks(c, (const void*)tl.f_fast, kTraceThreads, pl.lds_wf, &tl.grid_fast)) != ZRT_OK)
        return rc;
    return resident_blocks(c, (const void*)tl.f_exact, kTraceThreads, pl.lds_wf, &tl.grid_exact);
}

// One launch of a chain kernel over the rays `which` names, no more blocks than `nblk`.
static void transmit_walk(const zrt_context* c, const LaunchPlan& pl, TransmitFn f, uint32_t grid, uint32_t nblk,
                          TransmitParams& R, uint32_t which, uint32_t* launches) {
    R.q.which = which;
    hipLaunchKernelGGL(f, dim3(std::min(grid, nblk)), dim3(kTraceThreads), pl.lds_wf, c->stream, R);
    ++*launches;
}

// The whole chains of R's first `live` rays, over the identity queue: the fast
// kernel (kRaysFast), then the IEEE-division kernel over the rays it left
// (kRaysRest); without a fast kernel that one over every ray (kRaysAll).
static void transmit_chains(const zrt_context* c, const LaunchPlan& pl, const TransmitLaunch& tl, TransmitParams& R,
                            uint32_t live, uint32_t* launches) {
    const uint32_t lblk = (live + kBlock - 1) / kBlock;
    identity_queue(R.q, live);
    if (tl.f_fast) transmit_walk(c, pl, tl.f_fast, tl.grid_fast, lblk, R, kRaysFast, launches);
    transmit_walk(c, pl, tl.f_exact, tl.grid_exact, lblk, R, tl.f_fast ? kRaysRest : kRaysAll, launches);
}

// ---------------------------------------------------------------------------
// What the first-hit query calls (query_rays, zrt_context_transmittance,
// zrt_context_occlusion, light_items) do alike on the host.  Each reads top to
// bottom as: validate -> plan and buffers -> parameters -> chunk loop -> stats.

// The bytes of the grow-only buffers every such call reuses: the staging
// buffers, and of pass set 0 the queue and the hit records only.
static size_t query_held(const zrt_context* c) {
    const zrt_context::PassSet& ps = c->set[0];
    return 4ull * (c->rays_cap + c->hits_cap) + 16ull * (ps.q0_cap + ps.hit_cap) + c->bfc_bytes + c->esc_extra;
}

// Rays per chunk: at most kTraceChunk, fewer (but 64) if the device is short of
// memory for `per_ray` bytes of work buffers per ray (0: the call grows none).
// The budget is read before any buffer grows (device_budget), so call this
// first; `held`: query_held and whatever else of the context the call reuses.
static uint64_t query_chunk(const zrt_context* c, uint64_t num_rays, uint64_t per_ray, size_t held) {
    const size_t budget = device_budget(c, held);
    uint64_t chunk = std::min<uint64_t>(kTraceChunk, num_rays);
    if (per_ray) chunk = std::max<uint64_t>(64, std::min<uint64_t>(chunk, budget / per_ray));
    return chunk;
}

// A buffer grown to `need` elements, then the capacity guard (shortfall) over
// the same count: what a launch writes is what was asked for.
template <class T>
static int grow_checked(const char* what, T** p, size_t* cap, uint64_t need) {
    const int rc = grow(p, cap, need);
    if (rc != ZRT_OK) return rc;
    return shortfall(what, *p, *cap, need) ? ZRT_ERR_INVALID_ARG : ZRT_OK;
}

// Pass set 0's buffers for a query's park path: queues of `q0` / `q1` slots (3
// float4 each; 0: not used), `hits` hit records and `ctr_words` counter words.
static int grow_park_buffers(zrt_context::PassSet& ps, uint64_t q0, uint64_t q1, uint64_t hits, size_t ctr_words) {
    int rc;
    if (q0 && (rc = grow_checked("q0", &ps.q0, &ps.q0_cap, 3 * q0)) != ZRT_OK) return rc;
    if (q1 && (rc = grow_checked("q1", &ps.q1, &ps.q1_cap, 3 * q1)) != ZRT_OK) return rc;
    if ((rc = grow_checked("hit records", &ps.hit, &ps.hit_cap, hits)) != ZRT_OK) return rc;
    return grow_checked("counters", &ps.wfc, &ps.wfc_cap, ctr_words);
}

// A zeroed QueryParams' scene, counters and statistics: one segment per ray.
static void query_params(const zrt_context* c, QueryParams& Q) {
    scene_params(c, Q.w.t);
    Q.w.t.max_bounce = 1;
    Q.w.t.counter = c->d_counter;
    Q.w.t.stats = c->d_stats;
    Q.ctr = c->d_counter;
}

// ... and, for a call whose first hits or items take the park path, pass set
// 0's queue, hit records and counters (launch 0's, bounce_params' layout).
static void query_park_params(const zrt_context* c, const LaunchPlan& pl, const zrt_context::PassSet& ps, QueryParams& Q) {
    Q.w.q_in = ps.q0;
    Q.w.hit = ps.hit;
    Q.w.fetch8 = ps.wfc;
    Q.w.n_in8 = region_counts(ps, 0);
    park_params(c, pl, Q.w);
    Q.q = ps.q0;
    Q.n_in8 = region_counts(ps, 0);
}

// A host batch's chunk on its way in: its n rays at the head of d_rays and, if
// the call has one, its per-ray row (bounds, radii) behind a whole chunk's rays,
// at d_rays + 6 * chunk; then the mark the chunk's kernel time counts from.
static int stage_chunk(zrt_context* c, const float* rays, const float* row, uint64_t chunk, uint32_t n) {
    HIP_TRY(hipMemcpyAsync(c->d_rays, rays, 24ull * n, hipMemcpyHostToDevice, c->stream));
    if (row) HIP_TRY(hipMemcpyAsync(c->d_rays + 6 * chunk, row, 4ull * n, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipEventRecord(c->ev_trace[0], c->stream));
    return ZRT_OK;
}
// ... and after its copies back: the time from that mark to the one the caller
// recorded (ev_trace[1]) before them.
static int chunk_kernel_time(zrt_context* c, zrt_stats& st) {
    float t = 0.0f;
    HIP_TRY(hipEventElapsedTime(&t, c->ev_trace[0], c->ev_trace[1]));
    st.trace_kernel_ms += t;
    return ZRT_OK;
}

// The end of a query call: the call's time, and the kernel time of a batch
// that stayed on the device (a host batch sums its chunks' between the copies).
static int finish_query(zrt_context* c, bool on_device, uint32_t launches, zrt_stats& st) {
    HIP_TRY(hipEventRecord(c->ev_end, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    float ms = 0.0f;
    HIP_TRY(hipEventElapsedTime(&ms, c->ev_begin, c->ev_end));
    st.render_ms = ms;
    if (on_device) st.trace_kernel_ms = ms;
    st.trace_launches = launches;
    return ZRT_OK;
}
// ... with the first `words` of the call's statistics read to `hs` (0: none);
// a counting call's cells and tests are words 1 and 2.  The caller sets
// segments, samples and hits, which differ per call.
static int query_stats(zrt_context* c, bool on_device, uint32_t launches, bool counting, unsigned long long* hs,
                       size_t words, zrt_stats& st) {
    int rc;
    if ((rc = finish_query(c, on_device, launches, st)) != ZRT_OK) return rc;
    if (!words) return ZRT_OK;
    HIP_TRY(copy_sync(hs, c->d_stats, 8 * words, hipMemcpyDeviceToHost, c->stream));
    if (counting) {
        st.cells_visited = hs[1];
        st.triangle_tests = hs[2];
    }
    return ZRT_OK;
}

// Samples per pass: the caller's cfg->samples_per_pass, else as few passes
// as the queue budget allows but at least one per pass set (the sets' kernels
// overlap on their streams), split evenly: cfg3 256 spp = 2 x 128 (r02bq, two
// streams: 2 x 128 265.5 ms, 4 x 64 269.2, 8 x 32 273.1; cfg2 64 spp: 2 x 32
// 18.1 ms vs one pass 20.1).  The budget (device_budget) covers every set.
// `held`: the bytes of pass buffers this context already holds.  The pass
// count is a multiple of the sets (when spp allows), so the streams stay
// balanced to the end of the frame.
static uint64_t pass_samples(const zrt_context* c, const zrt_render_config* cfg, uint64_t per_item, uint32_t P,
                             uint32_t sets, size_t held) {
    const uint64_t spp = cfg->num_samples;
    const uint64_t cap = std::max<uint64_t>(1, 0x7FFFFF00ull / P);     // items of a pass < 2^31
    if (cfg->samples_per_pass) return std::min<uint64_t>(std::min<uint64_t>(cfg->samples_per_pass, spp), cap);
    const size_t budget = device_budget(c, held);
    const uint64_t fit = std::min<uint64_t>(cap, std::max<uint64_t>(1, budget / sets / (per_item * P)));
    uint64_t npass = std::max<uint64_t>(std::min<uint64_t>(sets, spp), (spp + fit - 1) / fit);
    npass = std::min<uint64_t>(spp, (npass + sets - 1) / sets * sets);
    const uint64_t s_pass = (spp + npass - 1) / npass;
    return s_pass;
}

// The packed pixel order of this rank (tile_pixels) in c->pix and d_pix,
// cached across calls.
int rank_pixels(zrt_context* c, const zrt_camera* cam, const zrt_render_config* cfg, uint32_t nranks) {
    const uint32_t key[5] = {cam->w, cam->h, cfg->tile_size ? cfg->tile_size : 64, cfg->rank, nranks};
    if (c->pix_valid && memcmp(key, c->pix_key, sizeof key) == 0) return ZRT_OK;
    uint32_t n = 0;
    int rc = tile_pixels(key[0], key[1], key[2], key[3], key[4], nullptr, &n);
    if (rc != ZRT_OK) return rc;
    c->pix.resize(std::max<uint32_t>(n, 1));
    tile_pixels(key[0], key[1], key[2], key[3], key[4], c->pix.data(), &n);
    c->pix.resize(n);
    if ((rc = grow(&c->d_pix, &c->pix_cap, std::max<size_t>(n, 1))) != ZRT_OK) return rc;
    if (n) HIP_TRY(copy_sync(c->d_pix, c->pix.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    memcpy(c->pix_key, key, sizeof key);
    c->pix_valid = true;
    return ZRT_OK;
}

// A render's spp samples as npasses passes of s_pass samples (pass_samples) on
// nsets pass sets, planned for plan_sets; lead: samples moved from the last pass
// to the first; T: items of the first pass, the largest.
struct PassSplit {
    uint32_t spp, npasses, plan_sets, nsets, lead;
    uint64_t s_pass, T;
};
static uint32_t pass_first(const PassSplit& sp, uint32_t pass) {
    return pass == 0 ? 0u : (uint32_t)(pass * sp.s_pass + sp.lead);
}
static uint32_t pass_count(const PassSplit& sp, uint32_t pass) {
    return pass == 0 ? (uint32_t)std::min<uint64_t>(sp.spp, sp.s_pass + sp.lead)
                     : (uint32_t)std::min<uint64_t>(sp.s_pass, sp.spp - pass_first(sp, pass));
}
// `big`: a frame of kSetsMinSamples samples or more; per_item: bytes of a
// pass's buffers per item.  Holds the tuning builds' ZRT_SETS and ZRT_LEAD.
static PassSplit split_passes(const zrt_context* c, const zrt_render_config* cfg, uint32_t P, bool counting, bool big,
                              uint64_t per_item) {
    PassSplit sp{};
    const uint32_t spp = sp.spp = cfg->num_samples;
    // small frames run one set: a second stream costs its first launches
    // (the zrt CLI's 3-spp 1080p frame rendered in 30-39 vs 12.5-13.3 ms on a
    // fresh process) and does not pay back (cfg3 at 3 spp, warm: 7.1 vs 6.8
    // ms), while cfg2 (16.8 M samples) gains 10% (r02c4)
    uint32_t want_sets = big ? kPassSets : 1u;
#if defined(ZRT_SWEEP) || defined(ZRT_SETS_ENV)
    if (const char* e = getenv("ZRT_SETS")) want_sets = (uint32_t)std::max(1, std::min((int)kMaxPassSets, atoi(e)));
#endif
    size_t held = 16ull * c->out_cap + c->bfc_bytes + c->esc_extra;   // (the cull masks, the escape table's regions: the split must not depend on them)
    for (const zrt_context::PassSet& ps : c->set) held += held_bytes(ps);
    sp.s_pass = pass_samples(c, cfg, per_item, P, counting ? 1u : want_sets, held);
    sp.npasses = (uint32_t)((spp + sp.s_pass - 1) / sp.s_pass);
    // pass sets: pass p runs on set p % nsets, each set with its own stream
    // and buffers, so one pass's launches fill the machine while another's
    // drain (tails, the latency-bound shade kernel beside the park kernel):
    // two sets cfg3 -5%, cfg2 -9%, cfg5 -7% frame time, images identical
    // (r02c1, profiles/r02/r02c1_ab_two_streams.log)
    sp.plan_sets = counting ? 1u : std::min<uint32_t>(sp.npasses, want_sets);
    // ZRT_FLAG_ONE_SET: the same passes (split and lead as planned for the
    // sets) run one after another on the context's stream, so no kernel
    // overlaps another: exclusive kernel durations for bench.py's roofline,
    // the same per-launch work as the frame it stands for
    sp.nsets = (cfg->flags & ZRT_FLAG_ONE_SET) ? 1u : sp.plan_sets;
    // lead: samples moved from the last pass to the first.  The second set's
    // first primary launch waits for the first's (it fills every CU), so the
    // second set ends behind the first unless the first has more work.
    uint32_t lead_pct = sp.plan_sets > 1 ? kLeadPct : 0u;
#if defined(ZRT_SWEEP) || defined(ZRT_SETS_ENV)
    if (const char* e = getenv("ZRT_LEAD")) lead_pct = sp.plan_sets > 1 ? (uint32_t)std::max(0, std::min(50, atoi(e))) : 0u;
#endif
    const uint64_t last_n = spp - (uint64_t)(sp.npasses - 1) * sp.s_pass;     // samples of the last pass
    const uint64_t cap_items = std::max<uint64_t>(1, 0x7FFFFF00ull / P);
    sp.lead = sp.npasses > 1 ? (uint32_t)std::min<uint64_t>({sp.s_pass * lead_pct / 100, last_n - 1,
                                                          cap_items - std::min(cap_items, sp.s_pass)})
                             : 0u;
    sp.T = (sp.s_pass + sp.lead) * P;
    return sp;
}

// Primary frustum bounds (escape.h frustum_bound): one thread per 8x8 pixel
// block of the w x h image.
struct FrustumArgs {
    uint32_t res[3];
    float bmin[3], bmax[3], cs[3], org[3], llc[3], right[3], up[3];
    uint32_t w, h, nbx, nby;
    // this rank's tiles (capi.cpp tile_pixels: tile t of the tx-wide row-major
    // grid belongs to rank t % nranks): tile edge in blocks, tiles per row,
    // the rank and the rank count; the kernel bounds only their blocks.
    // whole: one wave per block of the image, those of other ranks' tiles
    // leaving at once (tiles larger than the image: fewer waves that way)
    uint32_t tb, tx, rank, nranks, whole;
};
__global__ __launch_bounds__(kBlock) void frustum_kernel(const uint32_t* __restrict__ sat, const FrustumArgs a,
                                                         float4* __restrict__ tlo) {
    const EscSat S{sat, a.res[0] + 1u, (a.res[0] + 1u) * (a.res[1] + 1u)};
    // one wave per block: lane l tests slices l, l + 64, ... of the same
    // march (frustum_cone / frustum_slice), the wave takes the first and
    // last occupied ones (a 1080p frame: 32 K waves of ~4 slices per lane
    // instead of 32 K threads of ~200 dependent slices, 0.42 ms, r04eb2)
    const uint32_t lane = threadIdx.x & 63u;
    // wave i: block i % tb^2 (row-major in the tile) of this rank's tile i / tb^2
    const uint32_t i = (blockIdx.x * kBlock + threadIdx.x) >> 6, bpt = a.tb * a.tb;
    uint32_t bx, by;
    if (a.whole) {                                         // (uniform over the wave)
        if (i >= a.nbx * a.nby) return;
        bx = i % a.nbx;
        by = i / a.nbx;
        if (((by / a.tb) * a.tx + bx / a.tb) % a.nranks != a.rank) return;
    } else {
        const uint32_t t = a.rank + (i / bpt) * a.nranks, k = i % bpt;
        bx = (t % a.tx) * a.tb + k % a.tb;
        by = (t / a.tx) * a.tb + k / a.tb;
        if (bx >= a.nbx || by >= a.nby) return;
    }
    const uint32_t b = by * a.nbx + bx;
    const FrustumCone q = frustum_cone(a.bmin, a.bmax, a.cs, a.org, a.llc, a.right, a.up, kFrustB * bx,
                                       kFrustB * bx + kFrustB, kFrustB * by, kFrustB * by + kFrustB);
    int first = 1 << 30, last = -1;
    if (q.ok)
        for (int it = (int)lane; it < (1 << 16) && !(it * q.ds > q.s_far); it += 64)
            if (frustum_slice(S, q, a.res, a.bmin, a.cs, a.org, it)) {
                first = min(first, it);
                last = max(last, it);
            }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        first = min(first, __shfl_xor(first, off));
        last = max(last, __shfl_xor(last, off));
    }
    if (lane == 0) {
        FrustumBound fb{0.0f, kInf, kInf, kInf};
        if (q.ok) frustum_finish(q, first == (1 << 30) ? -1 : first, last, fb);
        tlo[b] = make_float4(fb.lo, fb.hi, kInf, kInf);
    }
}

// The primary frustum bounds of this camera into d_tlo, every render (inside
// the timed region: one wave per 4x4 pixel block, 130 K waves at 1080p), and
// the primary launch's pointers to them.
static int launch_frustum(zrt_context* c, const zrt_camera* cam, const zrt_render_config* cfg, uint32_t nranks,
                          TraceParams& tp) {
    const uint32_t nbx = (cam->w + (1u << kFrustShift) - 1u) >> kFrustShift;
    const uint32_t nby = (cam->h + (1u << kFrustShift) - 1u) >> kFrustShift;
    const int rc = grow(&c->d_tlo, &c->tlo_cap, (size_t)nbx * nby);
    if (rc != ZRT_OK) return rc;
    FrustumArgs fa;
    for (int k = 0; k < 3; ++k) {
        fa.res[k] = c->grid.resolution[k];
        fa.bmin[k] = c->grid.bbox_min[k];
        fa.bmax[k] = c->grid.bbox_max[k];
        fa.cs[k] = c->grid.cell_size[k];
        fa.org[k] = cam->origin[k];
        fa.llc[k] = cam->lower_left_corner[k];
        fa.right[k] = cam->right[k];
        fa.up[k] = cam->up[k];
    }
    fa.w = cam->w; fa.h = cam->h; fa.nbx = nbx; fa.nby = nby;
    // only the blocks of this rank's tiles (a tile edge is a multiple of 8
    // pixels, so of a block edge): an 8-rank frame bounds 1/8 of them
    const uint32_t tile = cfg->tile_size ? cfg->tile_size : 64u;
    fa.tb = tile >> kFrustShift;
    fa.tx = (cam->w + tile - 1u) / tile;
    fa.rank = cfg->rank;
    fa.nranks = nranks;
    const uint64_t ntiles = (uint64_t)fa.tx * ((cam->h + tile - 1u) / tile);
    // (a rank with pixels owns tile `rank`, so ntiles > rank here)
    const uint64_t per_tile = (ntiles - cfg->rank + nranks - 1u) / nranks * fa.tb * fa.tb;
    fa.whole = per_tile > (uint64_t)nbx * nby ? 1u : 0u;
    const uint64_t fthreads = (fa.whole ? (uint64_t)nbx * nby : per_tile) * 64u;
    hipLaunchKernelGGL(frustum_kernel, dim3((uint32_t)((fthreads + kBlock - 1) / kBlock)), dim3(kBlock), 0, c->stream,
                       (const uint32_t*)c->d_sat, fa, c->d_tlo);
    HIP_TRY(hipGetLastError());
    tp.tlo = c->d_tlo;
    tp.tlo_nbx = nbx;
    return ZRT_OK;
}

// A render's stats words on stderr (debugging only): the counting build's walk
// and test trip counts; ZRT_SWEEP builds: the kernels' cycle profiles.
static int report_stats(const unsigned long long* hs, bool counting, bool park) {
    if (getenv("ZRT_CELL_STATS") && counting)
        fprintf(stderr, "{\"zrt_profile_cells\": {\"visited\": %llu, \"loaded\": %llu, \"non_empty\": %llu, "
                "\"tests\": %llu, \"wave_cell_trips\": %llu, \"wave_tri_trips\": %llu, \"trips_with_tests\": %llu, "
                "\"shared_rounds\": %llu}}\n",
                hs[1], hs[4], hs[5], hs[2], hs[6], hs[7], hs[14], hs[15]);
#ifdef ZRT_SWEEP
    if (hs[60]) {       // the early append's reservation disagreed with shading (shade_entry_keep)
        fprintf(stderr, "zrt: %llu shade continuations differ from their reservations\n", hs[60]);
        return ZRT_ERR_HIP;
    }
    if (getenv("ZRT_PARK_PROFILE") && park)
        fprintf(stderr, "{\"zrt_park_profile\": {\"cyc_shade_refill\": %llu, \"cyc_walk\": %llu, \"cyc_test\": %llu, "
                "\"walk_iters\": %llu, \"walk_lanes\": %llu, \"test_rounds\": %llu, \"sub_rounds\": %llu, "
                "\"pairs\": %llu, \"refill_rounds\": %llu, \"shaded_lanes\": %llu, \"cyc_drain\": %llu, "
                "\"cyc_atomic\": %llu, \"cyc_setup\": %llu}}\n",
                hs[16], hs[17], hs[18], hs[19], hs[20], hs[21], hs[22], hs[23], hs[24], hs[25], hs[26], hs[27], hs[28]);
    if (getenv("ZRT_PARK_PROFILE") && park)
        fprintf(stderr, "{\"zrt_walk_steps\": {\"lane_steps\": %llu, \"empty_brick_steps\": %llu, "
                "\"empty_brick_entries\": %llu, \"escapes\": %llu, \"parked_tested\": %llu, \"parked_no_refs\": %llu, "
                "\"released_early\": %llu, \"cyc_round_wait\": %llu, \"hops_taken\": %llu, \"hops_refused\": %llu}}\n",
                hs[48], hs[49], hs[50], hs[51], hs[52], hs[53], hs[54], hs[55], hs[56], hs[57] - hs[56]);
    if (getenv("ZRT_PARK_PROFILE") && !counting)
        fprintf(stderr, "{\"zrt_primary_profile\": {\"cyc_walk\": %llu, \"cyc_shade\": %llu, \"cyc_fetch_append\": %llu}}\n",
                hs[29], hs[30], hs[31]);
    if (getenv("ZRT_PARK_PROFILE") && park)   // wf_shade_kernel phases: wave cycles, active-lane sums
        fprintf(stderr, "{\"zrt_shade_profile\": {\"cyc\": [%llu, %llu, %llu, %llu, %llu, %llu, %llu, %llu], "
                "\"lanes\": [%llu, %llu, %llu, %llu, %llu, %llu, %llu, %llu], \"phases\": [\"fetch\", \"records\", "
                "\"tri_data\", \"texels\", \"u_draw\", \"pair_ziggurat\", \"tail\", \"append\"]}}\n",
                hs[32], hs[33], hs[34], hs[35], hs[36], hs[37], hs[38], hs[39], hs[40], hs[41], hs[42], hs[43],
                hs[44], hs[45], hs[46], hs[47]);
#endif
    return ZRT_OK;
}

// The end of a render, the stream waited for: the stats, the times of its
// ne / 2 trace launches and of the kernels kt timed, the caller's outputs.
static int finish_render(zrt_context* c, const zrt_outputs* outs, KernelTimes& kt, const PassSplit& sp, uint32_t P,
                         bool counting, bool park, uint32_t ne, uint32_t launches, zrt_stats& st) {
    unsigned long long hs[64];
    HIP_TRY(copy_sync(hs, c->d_stats, sizeof hs, hipMemcpyDeviceToHost, c->stream));
    const int rc = report_stats(hs, counting, park);
    if (rc != ZRT_OK) return rc;
    float ms = 0.0f;
    HIP_TRY(hipEventElapsedTime(&ms, c->ev_begin, c->ev_end));
    st.render_ms = ms;
    const bool wf_debug = getenv("ZRT_WF_DEBUG") != nullptr;
    for (uint32_t e = 0; e + 1 < ne; e += 2) {   // trace launches only (not resolve)
        float t = 0.0f;
        HIP_TRY(hipEventElapsedTime(&t, c->ev_trace[e], c->ev_trace[e + 1]));
        st.trace_kernel_ms += t;
        if (wf_debug) fprintf(stderr, "{\"zrt_launch\": %u, \"ms\": %.3f}\n", e / 2, t);
    }
    st.trace_launches = launches;
    for (size_t k = 0; k < kt.n; ++k) {
        float t = 0.0f;
        HIP_TRY(hipEventElapsedTime(&t, c->ev_k[2 * k], c->ev_k[2 * k + 1]));
        kt.kp.ms[c->ev_k_cls[k]] += t;
    }
    kt.kp.passes = sp.npasses;
    kt.kp.sets = counting ? 1u : sp.nsets;
    if (counting)
        for (int k = 0; k < 4; ++k) kt.kp.primary_counts[k] = hs[8 + k];
    c->prof = kt.kp;
    st.segments = hs[0];
    st.cells_visited = hs[1];
    st.triangle_tests = hs[2];
    st.hits = hs[3];
    st.samples = (uint64_t)P * sp.spp;

    if (outs && (outs->rgb_packed || outs->rgb_image)) {
        std::vector<uint8_t> tmp;
        uint8_t* dst = outs->rgb_packed;
        if (!dst) { tmp.resize(3ull * P); dst = tmp.data(); }
        HIP_TRY(copy_sync(dst, c->d_rgb, 3ull * P, hipMemcpyDeviceToHost, c->stream));
        if (outs->rgb_image)
            for (uint32_t q = 0; q < P; ++q) memcpy(outs->rgb_image + 3ull * c->pix[q], dst + 3ull * q, 3);
    }
    if (outs && outs->linear_packed)
        HIP_TRY(copy_sync(outs->linear_packed, c->d_lin, 3ull * P * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    return ZRT_OK;
}

// zrt_context_render and zrt_context_accumulate: samples base .. base +
// cfg->num_samples - 1 of every owned pixel (the stream key's sample index;
// the passes split the call's own num_samples).  Without a film, base is 0 and
// the sums live in d_acc between the passes of a frame of several; with one
// they are read from (base > 0) and left in the film, the film's resolve
// kernels take the places of wf_resolve_kernel / resolve_kernel with
// 1 / (base + num_samples) as inv_spp, and d_rgb / d_lin are written only if
// the call asked for them.  Everything else -- the split, the plan, the launch
// sequence, the stats -- is the render's.
//
// zrt_context_refine traces a film's active pixels only: `sparse`
// names A of the rank's pixels (image indices, the kernels' pixlist) and their
// rows in the film.  The call is then a render of those A pixels -- P = A in
// the split, the plan, the thresholds and the stats -- whose resolves are the
// sparse film resolves; it writes no outputs (the caller presents the film).
struct SparsePixels {
    const uint32_t* list;    // device, A image pixels in packed order
    const uint32_t* slot;    // device, their rows in the film
    uint32_t A;              // 0 < A <= the rank's pixels
};

// What a render refuses before any device work.
static int render_args(const zrt_context* c, const zrt_camera* cam, const zrt_render_config* cfg, uint32_t base) {
    if (!c || !cam || !cfg) return ZRT_ERR_INVALID_ARG;
    // (the stream key gives the sample index 16 bits)
    if (cfg->num_samples == 0 || (uint64_t)base + cfg->num_samples > 65535) return ZRT_ERR_INVALID_ARG;
    if (cam->w == 0 || cam->h == 0 || (uint64_t)cam->w * cam->h > 0xFFFFFFFFull) return ZRT_ERR_INVALID_ARG;
    const uint32_t nranks = cfg->num_ranks ? cfg->num_ranks : 1;
    if (cfg->rank >= nranks) return ZRT_ERR_INVALID_ARG;
    // the scatter mask holds one bit per bounce slot, the queue 16 bits of depth
    if (cfg->max_bounce > 32) return ZRT_ERR_UNSUPPORTED;
    if ((cfg->flags & ZRT_FLAG_COUNT_STATS) != 0 && !count_fn(cfg->max_bounce)) return ZRT_ERR_UNSUPPORTED;
    return ZRT_OK;
}

static int render_samples(zrt_context* c, const zrt_camera* cam, const zrt_render_config* cfg,
                          const zrt_outputs* outs, zrt_stats* stats, uint32_t base, zrt_film* film,
                          const SparsePixels* sparse = nullptr) {
    int rc;
    if ((rc = render_args(c, cam, cfg, base)) != ZRT_OK) return rc;
    const uint32_t nranks = cfg->num_ranks ? cfg->num_ranks : 1;
    const bool counting = (cfg->flags & ZRT_FLAG_COUNT_STATS) != 0;
    const TraceFn cfn = count_fn(cfg->max_bounce);
    DeviceGuard g(c->device);

    if ((rc = rank_pixels(c, cam, cfg, nranks)) != ZRT_OK) return rc;
    const uint32_t owned = (uint32_t)c->pix.size();
    zrt_stats st{};
    if (film && film->n_owned != owned) return ZRT_ERR_INVALID_ARG;
    if (sparse && (!film || outs || sparse->A == 0 || sparse->A > owned || !sparse->list || !sparse->slot))
        return ZRT_ERR_INVALID_ARG;
    const uint32_t P = sparse ? sparse->A : owned;
    if (P == 0) {
        if (film) film->samples = base + cfg->num_samples;
        if (stats) *stats = st;
        return ZRT_OK;
    }

    const uint32_t spp = cfg->num_samples;
    const uint32_t mb = cfg->max_bounce;
    const uint32_t nb = std::max<uint32_t>(mb, 1);
    // per-item bytes of a pass: counting megakernel = the float4 sample
    // radiance; wavefront = 2 queues x 48 B + terminal 16 B + the bounce
    // planes per slot ((a, has_e) 16 B + e 16 B)
    // (+ the 16 B hit record the park kernel hands the shade kernel)
    const uint64_t per_item = counting ? 16ull : 96ull + 16ull + 16ull + 32ull * nb;
    const bool big = (uint64_t)P * cfg->num_samples >= kSetsMinSamples;
    const bool ktimes = (cfg->flags & ZRT_FLAG_KERNEL_TIMES) != 0;
    const PassSplit sp = split_passes(c, cfg, P, counting, big, per_item);
    const uint32_t npasses = sp.npasses, nsets = sp.nsets;
    const uint64_t T = sp.T;
    // the bounce launches (resolve_plan), after the budget was read: a first
    // big frame builds the escape table and the cull masks here
    LaunchPlan pl;
    if ((rc = resolve_plan(c, cfg->flags, counting, true, big, pl)) != ZRT_OK) return rc;
    const bool park_next = pl.park;
    // the tuning builds' schedule, for renders only
#if defined(ZRT_SWEEP) || defined(ZRT_SETS_ENV)
    if (const char* e = getenv("ZRT_PARK_T")) pl.test_min = pl.rel_min = (uint32_t)std::max(1, std::min(64, atoi(e)));
    if (const char* e = getenv("ZRT_PARK_R")) pl.refill_min = (uint32_t)std::max(1, std::min(64, atoi(e)));
    if (const char* e = getenv("ZRT_PARK_REL")) pl.rel_min = (uint32_t)std::max(1, std::min(64, atoi(e)));
    if (const char* e = getenv("ZRT_PARK_REL_E")) pl.rel_emin = (uint32_t)std::max(1, std::min(64, atoi(e)));
#endif
#ifdef ZRT_SWEEP
    if (const char* e = getenv("ZRT_PARK_BLOCK")) plan_park_block(pl, std::max(64, std::min(kParkBlock, atoi(e) / 64 * 64)));
#endif
    if (getenv("ZRT_WF_DEBUG"))
        fprintf(stderr, "{\"zrt_park_lds\": {\"occx_bytes\": %u, \"block\": %d, \"lds_per_block\": %zu, "
                "\"release_frac\": %.4f, \"release\": %d}}\n",
                4u * pl.occx_ldsw, pl.park_block, pl.lds_park, c->rel_frac, pl.rel ? 1 : 0);
    // the primary launch: wf_kernel (coherent 8x8-pixel waves: 22 vs 42 ms
    // for the park kernel at cfg3 64 spp, r02d)
    const WfFn f_first = pl.mtx ? kWfPrimaryExact : pl.packed ? (pl.pbm ? kWfPrimaryBM : kWfPrimary) : kWfPrimaryWide;

    if (counting && (rc = grow(&c->d_out, &c->out_cap, (size_t)T)) != ZRT_OK) return rc;
    for (uint32_t k = 0; k < nsets && !counting; ++k) {
        zrt_context::PassSet& ps = c->set[k];
        if ((rc = grow_pass_set(ps, T, nb, mb, park_next ? T : 0)) != ZRT_OK) return rc;
        if (k == 0) {
            ps.stream = c->stream;
        } else {
            if (!ps.stream) HIP_TRY(hipStreamCreateWithFlags(&ps.stream, hipStreamNonBlocking));
            if (!ps.ev_join) HIP_TRY(hipEventCreateWithFlags(&ps.ev_join, hipEventDisableTiming));
        }
    }
    if (nsets > 1) {
        if (!c->ev_fork) HIP_TRY(hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
        if ((rc = event_pool(c->ev_pass, npasses, hipEventDisableTiming)) != ZRT_OK) return rc;
    }
    // a film's sums live in the film, not in d_acc, which a render of several
    // passes between two of its calls overwrites
    const bool use_acc = !film && npasses > 1;
    if (use_acc && (rc = grow(&c->d_acc, &c->acc_cap, P)) != ZRT_OK) return rc;
    float4* const acc = film ? film->d_sum : c->d_acc;
    // a render always leaves its image in d_rgb (a group gathers it from
    // there); a film's call only when it asked for an RGB8 output
    const bool want_rgb = !film || (outs && (outs->rgb_image || outs->rgb_packed || outs->device_rgb_packed));
    if (want_rgb && (rc = grow(&c->d_rgb, &c->rgb_cap, 3ull * P)) != ZRT_OK) return rc;
    const bool want_lin = outs && outs->linear_packed;
    if (want_lin && (rc = grow(&c->d_lin, &c->lin_cap, 3ull * P)) != ZRT_OK) return rc;
    const uint32_t launches_per_pass = counting ? 1 : nb;
    if ((rc = event_pool(c->ev_trace, 2ull * npasses * launches_per_pass)) != ZRT_OK) return rc;
    // per-kernel events: per pass the primary, nb - 1 bounces of up to two
    // kernels, the resolve
    KernelTimes kt{c, ktimes};
    const size_t nk = ktimes ? (size_t)npasses * (2 * nb + 1) : 0;
    if ((rc = event_pool(c->ev_k, 2 * nk)) != ZRT_OK) return rc;
    c->ev_k_cls.assign(nk, 0);

    // capacity guard (shortfall) of what grow_pass_set does not cover: the
    // frame's buffers, the counting output 1 per item, the other sets'
    // streams, and every pass's items S * P <= T
    {
        bool bad = shortfall("pixel list", c->d_pix, c->pix_cap, P) ||
                   (want_rgb && shortfall("rgb", c->d_rgb, c->rgb_cap, 3ull * P)) ||
                   (use_acc && shortfall("accumulator", c->d_acc, c->acc_cap, P)) || (film && !film->d_sum) ||
                   (want_lin && shortfall("linear", c->d_lin, c->lin_cap, 3ull * P)) ||
                   (counting && shortfall("counting output", c->d_out, c->out_cap, T));
        for (uint32_t k = 1; k < nsets && !counting && !bad; ++k) bad = !c->set[k].stream || !c->set[k].ev_join;
        for (uint32_t pass = 0; pass < npasses && !bad; ++pass)
            bad = (uint64_t)pass_count(sp, pass) * P > T || pass_first(sp, pass) + pass_count(sp, pass) > spp;
        if (bad) return ZRT_ERR_INVALID_ARG;
    }

    // occupancy-sized persistent grids
    uint32_t grid_first = 0, grid_count = 0;
    BounceGrids grids{};
    if (counting) {
        if ((rc = resident_blocks(c, (const void*)cfn, kTraceThreads, pl.lds_wf, &grid_count)) != ZRT_OK) return rc;
    } else {
        if ((rc = resident_blocks(c, (const void*)f_first, kTraceThreads, pl.lds_wf, &grid_first)) != ZRT_OK) return rc;
        if ((rc = bounce_grids(c, pl, park_next, !park_next, grids)) != ZRT_OK) return rc;
    }

    TraceParams tp;
    scene_params(c, tp);
    for (int i = 0; i < 3; ++i) {
        tp.org[i] = cam->origin[i];
        tp.llc[i] = cam->lower_left_corner[i];
        tp.right[i] = cam->right[i];
        tp.up[i] = cam->up[i];
    }
    tp.w = cam->w;
    tp.pixlist = sparse ? sparse->list : c->d_pix;
    tp.P = P;
    tp.max_bounce = mb;
    tp.seed = cfg->seed;
    tp.out = c->d_out;
    tp.counter = c->d_counter;
    tp.stats = c->d_stats;
    // stage3.zig:223 inv_num_samples = ones / splat(spp)  (f32 division); a
    // film's image so far: over the samples it holds after this call
    const float inv_spp = 1.0f / (float)(base + spp);
    uint8_t* const rgb_dst = want_rgb ? c->d_rgb : nullptr;
    const auto wf_res = film ? wf_film_resolve_kernel : wf_resolve_kernel;
    const auto count_res = film ? film_resolve_kernel : resolve_kernel;

    HIP_TRY(hipMemsetAsync(c->d_stats, 0, 512, c->stream));
    HIP_TRY(hipEventRecord(c->ev_begin, c->stream));
    // the frustum bounds cost a 78-us launch per render (1080p, one wave per
    // block, r04fk3; 0.42 ms one thread per block) and save ~18% of the
    // primary launch: frames of 2^23 samples or more (a 3-spp 1080p frame's
    // primary takes ~0.5 ms: break-even)
    if (c->d_sat && !counting && pl.packed && !(cfg->flags & ZRT_FLAG_NO_FRUSTUM) &&
        ((uint64_t)P * cfg->num_samples >= kFrustumMinSamples || (cfg->flags & ZRT_FLAG_FRUSTUM)) &&
        (rc = launch_frustum(c, cam, cfg, nranks, tp)) != ZRT_OK)
        return rc;
    if (nsets > 1) {                           // the other sets start after the stats reset
        HIP_TRY(hipEventRecord(c->ev_fork, c->stream));
        for (uint32_t k = 1; k < nsets; ++k) HIP_TRY(hipStreamWaitEvent(c->set[k].stream, c->ev_fork, 0));
    }
    uint32_t launches = 0, ne = 0;
    for (uint32_t pass = 0; pass < npasses; ++pass) {
        // pass set pass % nsets: its own stream and buffers
        const zrt_context::PassSet& ps = c->set[counting ? 0u : pass % nsets];
        hipStream_t sm = counting ? c->stream : ps.stream;
        const uint32_t s0 = pass_first(sp, pass);
        const uint32_t S = pass_count(sp, pass);
        tp.s0 = base + s0;
        tp.total = S * P;
        tp.S = S;
        tp.sdiv = div_magic(S);
        // first: nothing summed yet.  Pass 0 of a continuing call (base > 0)
        // reads the film's sums, which the previous call -- synchronous, it
        // returned after its streams were waited for -- left complete, so that
        // resolve waits for nothing but its own stream, as pass 0 always did;
        // the later passes chain through ev_pass below, film or not.
        const int first = pass == 0 && base == 0 ? 1 : 0, last = pass + 1 == npasses ? 1 : 0;
        if (!counting) {
            HIP_TRY(hipMemsetAsync(ps.wfc, 0, 4ull * wfc_words(mb), sm));
            WfParams W;
            memset(&W, 0, sizeof W);
            W.t = tp;
            W.stk4 = ps.stk4;
            W.stk2 = ps.stk2;
            W.term = ps.term;
            W.hit = ps.hit;
            W.T = (uint32_t)T;
            park_params(c, pl, W);
            for (uint32_t k = 0; k < nb; ++k) {
                bounce_params(W, ps, k, mb);
                HIP_TRY(hipEventRecord(c->ev_trace[ne++], sm));
                if (k == 0) {
                    if ((rc = kt.begin(ZRT_KERNEL_PRIMARY, sm)) != ZRT_OK) return rc;
                    hipLaunchKernelGGL(f_first, dim3(grid_first), dim3(kTraceThreads), pl.lds_wf, sm, W);
                    HIP_TRY(hipGetLastError());
                    if ((rc = kt.end(sm)) != ZRT_OK) return rc;
                } else if ((rc = launch_bounce(pl, grids, W, sm, park_next, k + 1 == nb, &kt)) != ZRT_OK) {
                    return rc;
                }
                HIP_TRY(hipEventRecord(c->ev_trace[ne++], sm));
                ++launches;
            }
            // the passes' sums into acc stay in pass order (stage3.zig:236-242)
            if (nsets > 1 && pass > 0) HIP_TRY(hipStreamWaitEvent(sm, c->ev_pass[pass - 1], 0));
            if ((rc = kt.begin(ZRT_KERNEL_RESOLVE, sm)) != ZRT_OK) return rc;
            if (sparse)
                hipLaunchKernelGGL(wf_film_sparse_resolve_kernel, dim3((P + kResPix - 1) / kResPix), dim3(kBlock), 0,
                                   sm, ps.term, ps.stk4, ps.stk2, (uint32_t)T, P, S, mb, acc, sparse->slot, first);
            else
                hipLaunchKernelGGL(wf_res, dim3((P + kResPix - 1) / kResPix), dim3(kBlock), 0, sm,
                                   ps.term, ps.stk4, ps.stk2, (uint32_t)T, P, S, mb, acc, first, last, inv_spp,
                                   rgb_dst, want_lin ? c->d_lin : nullptr);
            if ((rc = kt.end(sm)) != ZRT_OK) return rc;
            if (nsets > 1) HIP_TRY(hipEventRecord(c->ev_pass[pass], sm));
        } else {
            HIP_TRY(hipMemsetAsync(c->d_counter, 0, 4, c->stream));
            HIP_TRY(hipEventRecord(c->ev_trace[ne++], c->stream));
            if ((rc = kt.begin(ZRT_KERNEL_COUNT, c->stream)) != ZRT_OK) return rc;
            hipLaunchKernelGGL(cfn, dim3(grid_count), dim3(kTraceThreads), pl.lds_wf, c->stream, tp);
            HIP_TRY(hipGetLastError());
            if ((rc = kt.end(c->stream)) != ZRT_OK) return rc;
            ++launches;
            HIP_TRY(hipEventRecord(c->ev_trace[ne++], c->stream));
            if ((rc = kt.begin(ZRT_KERNEL_RESOLVE, c->stream)) != ZRT_OK) return rc;
            if (sparse)
                hipLaunchKernelGGL(film_sparse_resolve_kernel, dim3((P + kBlock - 1) / kBlock), dim3(kBlock), 0,
                                   c->stream, c->d_out, P, S, acc, sparse->slot, first);
            else
                hipLaunchKernelGGL(count_res, dim3((P + kBlock - 1) / kBlock), dim3(kBlock), 0, c->stream,
                                   c->d_out, P, S, acc, first, last, inv_spp, rgb_dst,
                                   want_lin ? c->d_lin : nullptr);
            if ((rc = kt.end(c->stream)) != ZRT_OK) return rc;
        }
        HIP_TRY(hipGetLastError());
    }
    for (uint32_t k = 1; k < nsets; ++k) {     // join: the other sets' passes are done
        HIP_TRY(hipEventRecord(c->set[k].ev_join, c->set[k].stream));
        HIP_TRY(hipStreamWaitEvent(c->stream, c->set[k].ev_join, 0));
    }
    HIP_TRY(hipEventRecord(c->ev_end, c->stream));
    if (outs && outs->device_rgb_packed)
        HIP_TRY(hipMemcpyAsync(outs->device_rgb_packed, c->d_rgb, 3ull * P, hipMemcpyDeviceToDevice,
                               c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));

    if ((rc = finish_render(c, outs, kt, sp, P, counting, park_next, ne, launches, st)) != ZRT_OK) return rc;
    if (film) film->samples = base + spp;
    if (stats) *stats = st;
    return ZRT_OK;
}

extern "C" int zrt_context_render(zrt_context* c, const zrt_camera* cam, const zrt_render_config* cfg,
                                  const zrt_outputs* outs, zrt_stats* stats) {
    return render_samples(c, cam, cfg, outs, stats, 0u, nullptr);
}

// ---------------------------------------------------------------------------
// Films (include/zrt.h): a frame's per-pixel sums kept between
// calls, so that zrt_context_accumulate continues them where a render would
// start at sample 0 and forget them.
extern "C" int zrt_film_create(zrt_context* c, uint32_t w, uint32_t h, uint32_t tile_size, uint32_t rank,
                               uint32_t num_ranks, zrt_film** out) {
    if (!c || !out) return ZRT_ERR_INVALID_ARG;
    *out = nullptr;
    if (w == 0 || h == 0 || (uint64_t)w * h > 0xFFFFFFFFull) return ZRT_ERR_INVALID_ARG;
    const uint32_t nranks = num_ranks ? num_ranks : 1, tile = tile_size ? tile_size : 64;
    uint32_t n = 0;
    int rc = tile_pixels(w, h, tile, rank, nranks, nullptr, &n);       // (refuses rank >= nranks, tile % 8)
    if (rc != ZRT_OK) return rc;
    DeviceGuard g(c->device);
    zrt_film* f = new (std::nothrow) zrt_film;
    if (!f) return ZRT_ERR_OUT_OF_MEMORY;
    size_t cap = 0;
    if ((rc = grow(&f->d_sum, &cap, std::max<size_t>(n, 1))) != ZRT_OK) { delete f; return rc; }
    f->ctx = c;
    f->device = c->device;
    f->w = w; f->h = h; f->tile = tile; f->rank = rank; f->nranks = nranks;
    f->n_owned = f->active = n;
    *out = f;
    return ZRT_OK;
}

// No pixel frozen, no checkpoint (reset, write): the next refine call clears
// the flags on the device before it reads them.
static void film_thaw(zrt_film* f) {
    f->checkpoint = 0;
    f->active = f->n_owned;
    f->state_stale = true;
    f->list_valid = false;
}

extern "C" int zrt_film_reset(zrt_film* f) {
    if (!f) return ZRT_ERR_INVALID_ARG;
    f->samples = 0;               // the next call starts from +0 (first): the sums need no clearing
    film_thaw(f);
    return ZRT_OK;
}

extern "C" int zrt_film_info(const zrt_film* f, uint32_t* n_owned, uint32_t* samples) {
    if (!f) return ZRT_ERR_INVALID_ARG;
    if (n_owned) *n_owned = f->n_owned;
    if (samples) *samples = f->samples;
    return ZRT_OK;
}

// The sums as stored (float4 rows on the device, 3 floats per pixel for the
// caller), no division: a checkpoint written back continues bit for bit.
extern "C" int zrt_film_read(zrt_film* f, float* sums, uint32_t* samples) {
    if (!f || (!sums && f->n_owned)) return ZRT_ERR_INVALID_ARG;
    DeviceGuard g(f->device);
    if (f->n_owned && f->samples) {
        std::vector<float4> tmp(f->n_owned);
        HIP_TRY(copy_sync(tmp.data(), f->d_sum, tmp.size() * sizeof(float4), hipMemcpyDeviceToHost, f->ctx->stream));
        for (uint32_t q = 0; q < f->n_owned; ++q) {
            sums[3ull * q] = tmp[q].x; sums[3ull * q + 1] = tmp[q].y; sums[3ull * q + 2] = tmp[q].z;
        }
    } else {
        // an empty film: the stored bits are never read; +0 is what the next call starts from
        for (uint64_t k = 0; k < 3ull * f->n_owned; ++k) sums[k] = 0.0f;
    }
    if (samples) *samples = f->samples;
    return ZRT_OK;
}

extern "C" int zrt_film_write(zrt_film* f, const float* sums, uint32_t samples) {
    if (!f || samples > 65535 || (!sums && f->n_owned && samples)) return ZRT_ERR_INVALID_ARG;
    DeviceGuard g(f->device);
    if (f->n_owned && samples) {
        std::vector<float4> tmp(f->n_owned);
        for (uint32_t q = 0; q < f->n_owned; ++q)
            tmp[q] = make_float4(sums[3ull * q], sums[3ull * q + 1], sums[3ull * q + 2], 0.0f);
        HIP_TRY(copy_sync(f->d_sum, tmp.data(), tmp.size() * sizeof(float4), hipMemcpyHostToDevice, f->ctx->stream));
    }
    f->samples = samples;
    film_thaw(f);
    return ZRT_OK;
}

extern "C" void zrt_film_destroy(zrt_film* f) {
    if (!f) return;
    DeviceGuard g(f->device);
    if (f->d_sum) (void)hipFree(f->d_sum);
    if (f->d_state) (void)hipFree(f->d_state);
    if (f->d_list) (void)hipFree(f->d_list);
    if (f->d_slot) (void)hipFree(f->d_slot);
    if (f->d_blk) (void)hipFree(f->d_blk);
    if (f->d_cnt) (void)hipFree(f->d_cnt);
    delete f;
}

extern "C" int zrt_context_accumulate(zrt_context* c, zrt_film* f, const zrt_camera* cam, const zrt_render_config* cfg,
                                      const zrt_outputs* outs, zrt_stats* stats) {
    if (!c || !f || !cam || !cfg || f->ctx != c) return ZRT_ERR_INVALID_ARG;
    if (cam->w != f->w || cam->h != f->h || (cfg->tile_size ? cfg->tile_size : 64u) != f->tile ||
        cfg->rank != f->rank || (cfg->num_ranks ? cfg->num_ranks : 1u) != f->nranks)
        return ZRT_ERR_INVALID_ARG;
    // a frozen pixel holds fewer samples than the film: only refine continues such a film
    if (f->active != f->n_owned) return ZRT_ERR_INVALID_ARG;
    return render_samples(c, cam, cfg, outs, stats, f->samples, f);
}

// ---------------------------------------------------------------------------
// Adaptive films (include/zrt.h): zrt_context_refine freezes the
// pixels whose image stopped changing and traces the rest.

// The adaptive state of a film, allocated by its first refine call, and all
// flags cleared where a reset or a write made them stale.
static int film_state(zrt_film* f) {
    int rc;
    const size_t n = std::max<size_t>(f->n_owned, 1), nblk = (n + kBlock - 1) / kBlock;
    if (!f->d_state) {
        size_t cap = 0;
        if ((rc = grow(&f->d_state, &cap, n)) != ZRT_OK) return rc;
        cap = 0;
        if ((rc = grow(&f->d_list, &cap, n)) != ZRT_OK) return rc;
        cap = 0;
        if ((rc = grow(&f->d_slot, &cap, n)) != ZRT_OK) return rc;
        cap = 0;
        if ((rc = grow(&f->d_blk, &cap, nblk + 1)) != ZRT_OK) return rc;
        f->state_stale = true;
    }
    if (f->state_stale) {
        HIP_TRY(hipMemsetAsync(f->d_state, 0, n * sizeof(float4), f->ctx->stream));
        f->state_stale = false;
        f->list_valid = false;
        f->active = f->n_owned;
        f->checkpoint = 0;
    }
    return ZRT_OK;
}

// Every owned pixel at its own count into the context's output buffers and on
// to the caller (what finish_render does with a render's), and the counts.
static int film_present(zrt_context* c, zrt_film* f, const zrt_outputs* outs, uint32_t* counts) {
    const uint32_t n = f->n_owned;
    const bool want_rgb = outs && (outs->rgb_image || outs->rgb_packed || outs->device_rgb_packed);
    const bool want_lin = outs && outs->linear_packed;
    if (n == 0 || (!want_rgb && !want_lin && !counts)) return ZRT_OK;
    int rc;
    if (want_rgb && (rc = grow(&c->d_rgb, &c->rgb_cap, 3ull * n)) != ZRT_OK) return rc;
    if (want_lin && (rc = grow(&c->d_lin, &c->lin_cap, 3ull * n)) != ZRT_OK) return rc;
    if (counts && (rc = grow(&f->d_cnt, &f->cnt_cap, n)) != ZRT_OK) return rc;
    if ((want_rgb && shortfall("rgb", c->d_rgb, c->rgb_cap, 3ull * n)) ||
        (want_lin && shortfall("linear", c->d_lin, c->lin_cap, 3ull * n)) ||
        (counts && shortfall("counts", f->d_cnt, f->cnt_cap, n)) || !f->d_sum)
        return ZRT_ERR_INVALID_ARG;
    hipLaunchKernelGGL(film_present_kernel, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, c->stream, f->d_sum,
                       f->d_state, n, f->samples, want_rgb ? c->d_rgb : nullptr, want_lin ? c->d_lin : nullptr,
                       counts ? f->d_cnt : nullptr);
    HIP_TRY(hipGetLastError());
    if (outs && outs->device_rgb_packed)
        HIP_TRY(hipMemcpyAsync(outs->device_rgb_packed, c->d_rgb, 3ull * n, hipMemcpyDeviceToDevice, c->stream));
    if (outs && (outs->rgb_packed || outs->rgb_image)) {
        std::vector<uint8_t> tmp;
        uint8_t* dst = outs->rgb_packed;
        if (!dst) { tmp.resize(3ull * n); dst = tmp.data(); }
        HIP_TRY(copy_sync(dst, c->d_rgb, 3ull * n, hipMemcpyDeviceToHost, c->stream));
        if (outs->rgb_image)
            for (uint32_t q = 0; q < n; ++q) memcpy(outs->rgb_image + 3ull * c->pix[q], dst + 3ull * q, 3);
    }
    if (want_lin)
        HIP_TRY(copy_sync(outs->linear_packed, c->d_lin, 3ull * n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (counts) HIP_TRY(copy_sync(counts, f->d_cnt, n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return ZRT_OK;
}

extern "C" int zrt_context_refine(zrt_context* c, zrt_film* f, const zrt_camera* cam, const zrt_render_config* cfg,
                                  const zrt_refine_config* rf, const zrt_outputs* outs, zrt_stats* stats,
                                  uint32_t* active) {
    if (!c || !f || !cam || !cfg || !rf || f->ctx != c) return ZRT_ERR_INVALID_ARG;
    if (cam->w != f->w || cam->h != f->h || (cfg->tile_size ? cfg->tile_size : 64u) != f->tile ||
        cfg->rank != f->rank || (cfg->num_ranks ? cfg->num_ranks : 1u) != f->nranks)
        return ZRT_ERR_INVALID_ARG;
    if (rf->threshold != rf->threshold) return ZRT_ERR_INVALID_ARG;       // NaN
    int rc;
    const uint32_t b = f->samples, n = f->n_owned;
    if ((rc = render_args(c, cam, cfg, b)) != ZRT_OK) return rc;
    DeviceGuard g(c->device);
    if ((rc = rank_pixels(c, cam, cfg, f->nranks)) != ZRT_OK) return rc;
    if (c->pix.size() != n) return ZRT_ERR_INVALID_ARG;
    zrt_stats st{};
    if ((rc = film_state(f)) != ZRT_OK) return rc;

    // 1. decide, 2. compact.  Without a decision the flags, A and the lists
    // stay what the previous call left; the kernel then only takes the
    // checkpoints (there is none to take of an empty film).
    const bool decide = f->checkpoint != 0 && b >= rf->min_samples;
    const uint32_t nblk = (n + kBlock - 1) / kBlock;
    uint32_t A = f->active;
    if (b != 0 && A != 0) {
        if (shortfall("pixel list", c->d_pix, c->pix_cap, n) || !f->d_state || !f->d_list || !f->d_slot || !f->d_blk)
            return ZRT_ERR_INVALID_ARG;
        hipLaunchKernelGGL(film_decide_kernel, dim3(nblk), dim3(kBlock), 0, c->stream, f->d_sum, f->d_state, n, b,
                           f->checkpoint, rf->threshold, decide ? 1 : 0, f->d_blk);
        HIP_TRY(hipGetLastError());
        if (decide) {
            hipLaunchKernelGGL(film_scan_kernel, dim3(1), dim3(kBlock), 0, c->stream, f->d_blk, nblk);
            HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(film_scatter_kernel, dim3(nblk), dim3(kBlock), 0, c->stream, f->d_state, c->d_pix, n,
                               f->d_blk, f->d_list, f->d_slot);
            HIP_TRY(hipGetLastError());
            HIP_TRY(copy_sync(&A, f->d_blk + nblk, sizeof A, hipMemcpyDeviceToHost, c->stream));
            if (A > f->active) return ZRT_ERR_HIP;                        // (a frozen pixel never thaws)
            f->active = A;
            f->list_valid = true;
        }
    }
    // 3. trace: a render of the A active pixels' next samples into the film
    if (A != 0) {
        if (A != n && !f->list_valid) return ZRT_ERR_INVALID_ARG;
        const SparsePixels sparse{f->d_list, f->d_slot, A};
        f->checkpoint = b;
        if ((rc = render_samples(c, cam, cfg, nullptr, &st, b, f, A != n ? &sparse : nullptr)) != ZRT_OK) return rc;
    }
    // 4. present
    if ((rc = film_present(c, f, outs, rf->sample_counts)) != ZRT_OK) return rc;
    if (stats) *stats = st;
    if (active) *active = A;
    return ZRT_OK;
}

extern "C" int zrt_film_counts(zrt_film* f, uint32_t* counts, uint32_t* active) {
    if (!f) return ZRT_ERR_INVALID_ARG;
    if (active) *active = f->active;
    if (!counts || f->n_owned == 0) return ZRT_OK;
    if (!f->d_state || f->state_stale || f->active == f->n_owned) {        // no pixel frozen
        for (uint32_t q = 0; q < f->n_owned; ++q) counts[q] = f->samples;
        return ZRT_OK;
    }
    DeviceGuard g(f->device);
    return film_present(f->ctx, f, nullptr, counts);
}

extern "C" int zrt_context_profile(const zrt_context* c, zrt_kernel_profile* out) {
    if (!c || !out) return ZRT_ERR_INVALID_ARG;
    *out = c->prof;
    return ZRT_OK;
}

// The feature planes of a frame: see include/zrt.h and DESIGN 5.16.  A render
// without the path tracer, on the context's stream and one set of buffers: per
// pass feature_walk_kernel (the instantiation the plan gives a primary launch)
// over the pass's items, then feature_resolve_kernel.  The item records are
// staged in pass set 0's first queue (3 float4 per item, the queue's own
// shape), the work counters are that set's, so a context that renders holds
// nothing twice; the sums between passes and a host call's planes have buffers
// of their own.  c->prof is a render's and stays.
extern "C" int zrt_context_features(zrt_context* c, const zrt_camera* cam, const zrt_render_config* cfg,
                                    const zrt_feature_outputs* out, zrt_stats* stats) {
    if (!c || !cam || !cfg || !out) return ZRT_ERR_INVALID_ARG;
    if (!out->base_color && !out->normal && !out->emissive && !out->depth && !out->transparency && !out->hits)
        return ZRT_ERR_INVALID_ARG;
    if (out->on_device > 1u || out->_reserved != 0u) return ZRT_ERR_INVALID_ARG;
    if (cfg->num_samples == 0 || cfg->num_samples > 65535) return ZRT_ERR_INVALID_ARG;
    if (cam->w == 0 || cam->h == 0 || (uint64_t)cam->w * cam->h > 0xFFFFFFFFull) return ZRT_ERR_INVALID_ARG;
    const uint32_t nranks = cfg->num_ranks ? cfg->num_ranks : 1;
    if (cfg->rank >= nranks || (cfg->tile_size ? cfg->tile_size : 64u) % 8u != 0u) return ZRT_ERR_INVALID_ARG;   // (tile_pixels' rules)
    const bool counting = (cfg->flags & ZRT_FLAG_COUNT_STATS) != 0;
    DeviceGuard g(c->device);

    int rc;
    if ((rc = rank_pixels(c, cam, cfg, nranks)) != ZRT_OK) return rc;
    const uint32_t P = (uint32_t)c->pix.size();
    zrt_stats st{};
    if (P == 0) { if (stats) *stats = st; return ZRT_OK; }
    const uint32_t spp = cfg->num_samples;

    // samples per pass: as given, else as few passes as kFeatStageBytes of item
    // records (and the device budget) allow, split evenly; items of a pass < 2^31
    zrt_context::PassSet& ps = c->set[0];
    const uint64_t cap = std::max<uint64_t>(1, 0x7FFFFF00ull / P);
    uint64_t s_pass;
    if (cfg->samples_per_pass) {
        s_pass = std::min<uint64_t>(std::min<uint64_t>(cfg->samples_per_pass, spp), cap);
    } else {
        size_t held = 16ull * (c->out_cap + c->facc_cap) + 4ull * c->fout_cap + c->bfc_bytes + c->esc_extra;
        for (const zrt_context::PassSet& s : c->set) held += held_bytes(s);
        const uint64_t budget = std::min<uint64_t>(kFeatStageBytes, device_budget(c, held));
        const uint64_t fit = std::min<uint64_t>(cap, std::max<uint64_t>(1, budget / (kFeatItemBytes * P)));
        const uint64_t np = (spp + fit - 1) / fit;
        s_pass = (spp + np - 1) / np;
    }
    const uint32_t npasses = (uint32_t)((spp + s_pass - 1) / s_pass);
    const uint64_t T = s_pass * P;

    // the walk a primary launch of this context and these flags takes
    LaunchPlan pl;
    if ((rc = resolve_plan(c, cfg->flags, counting, false, false, pl)) != ZRT_OK) return rc;
    const FeatureFn f_walk = counting  ? (FeatureFn)feature_walk_kernel<true, false, false, true>
                             : pl.mtx  ? (FeatureFn)feature_walk_kernel<false, false, false, true>
                             : !pl.packed ? (FeatureFn)feature_walk_kernel<false, false, false, false>
                             : pl.pbm  ? (FeatureFn)feature_walk_kernel<false, true, true, false>
                                       : (FeatureFn)feature_walk_kernel<false, true, false, false>;

    const bool host = out->on_device == 0u;
    if ((rc = grow(&ps.q0, &ps.q0_cap, 3 * T)) != ZRT_OK) return rc;
    if ((rc = grow(&ps.wfc, &ps.wfc_cap, wfc_words(0))) != ZRT_OK) return rc;
    if (npasses > 1 && (rc = grow(&c->d_facc, &c->facc_cap, 3ull * P)) != ZRT_OK) return rc;
    if (host && (rc = grow(&c->d_fout, &c->fout_cap, 12ull * P)) != ZRT_OK) return rc;
    if ((rc = event_pool(c->ev_trace, 2)) != ZRT_OK) return rc;
    // capacity guard: every buffer a launch below writes holds what it writes
    if (shortfall("pixel list", c->d_pix, c->pix_cap, P) || shortfall("item records", ps.q0, ps.q0_cap, 3 * T) ||
        shortfall("counters", ps.wfc, ps.wfc_cap, 8ull * kCtr) ||
        (npasses > 1 && shortfall("feature sums", c->d_facc, c->facc_cap, 3ull * P)) ||
        (host && shortfall("feature planes", c->d_fout, c->fout_cap, 12ull * P)) ||
        (uint64_t)npasses * s_pass < spp || s_pass * P > T)
        return ZRT_ERR_INVALID_ARG;
    uint32_t grid = 0;
    if ((rc = resident_blocks(c, (const void*)f_walk, kTraceThreads, pl.lds_wf, &grid)) != ZRT_OK) return rc;

    // a host call's planes: base colour, normal, emissive (3 P floats each),
    // depth, transparency, hits (P each) in d_fout; only those asked for are written
    FeaturePlanes planes{out->base_color, out->normal, out->emissive, out->depth, out->transparency, out->hits};
    if (host) {
        float* const b = c->d_fout;
        planes = FeaturePlanes{out->base_color ? b : nullptr,
                               out->normal ? b + 3ull * P : nullptr,
                               out->emissive ? b + 6ull * P : nullptr,
                               out->depth ? b + 9ull * P : nullptr,
                               out->transparency ? b + 10ull * P : nullptr,
                               out->hits ? reinterpret_cast<uint32_t*>(b + 11ull * P) : nullptr};
    }

    FeatureParams F;
    memset(&F, 0, sizeof F);
    TraceParams& tp = F.w.t;
    scene_params(c, tp);
    for (int i = 0; i < 3; ++i) {
        tp.org[i] = cam->origin[i];
        tp.llc[i] = cam->lower_left_corner[i];
        tp.right[i] = cam->right[i];
        tp.up[i] = cam->up[i];
    }
    tp.w = cam->w;
    tp.pixlist = c->d_pix;
    tp.P = P;
    tp.max_bounce = 1;
    tp.seed = cfg->seed;
    tp.counter = c->d_counter;
    tp.stats = c->d_stats;
    F.w.T = (uint32_t)T;
    F.w.fetch8 = ps.wfc;
    F.rec = ps.q0;
    const float inv_spp = 1.0f / (float)spp;               // stage3.zig:223

    HIP_TRY(hipMemsetAsync(c->d_stats, 0, 512, c->stream));
    HIP_TRY(hipEventRecord(c->ev_begin, c->stream));
    uint32_t launches = 0;
    // the frustum bounds, under the render's rule (zrt_context_render)
    if (c->d_sat && !counting && pl.packed && !(cfg->flags & ZRT_FLAG_NO_FRUSTUM) &&
        ((uint64_t)P * spp >= kFrustumMinSamples || (cfg->flags & ZRT_FLAG_FRUSTUM))) {
        if ((rc = launch_frustum(c, cam, cfg, nranks, tp)) != ZRT_OK) return rc;
        ++launches;
    }
    for (uint32_t pass = 0; pass < npasses; ++pass) {
        const uint32_t s0 = (uint32_t)(pass * s_pass);
        const uint32_t S = (uint32_t)std::min<uint64_t>(s_pass, spp - s0);
        tp.s0 = s0;
        tp.total = S * P;
        tp.S = S;
        tp.sdiv = div_magic(S);
        HIP_TRY(hipMemsetAsync(ps.wfc, 0, 4ull * 8 * kCtr, c->stream));
        hipLaunchKernelGGL(f_walk, dim3(grid), dim3(kTraceThreads), pl.lds_wf, c->stream, F);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(feature_resolve_kernel, dim3((P + kResPix - 1) / kResPix), dim3(kBlock), 0, c->stream,
                           (const float4*)ps.q0, P, S, c->d_facc, pass == 0 ? 1 : 0, pass + 1 == npasses ? 1 : 0,
                           inv_spp, planes);
        HIP_TRY(hipGetLastError());
        launches += 2;
    }
    HIP_TRY(hipEventRecord(c->ev_trace[1], c->stream));
    if (host) {
        const float* const b = c->d_fout;
        const struct { void* dst; const float* src; size_t words; } cp[6] = {
            {out->base_color, b, 3ull * P},        {out->normal, b + 3ull * P, 3ull * P},
            {out->emissive, b + 6ull * P, 3ull * P}, {out->depth, b + 9ull * P, P},
            {out->transparency, b + 10ull * P, P},  {out->hits, b + 11ull * P, P}};
        for (const auto& k : cp)
            if (k.dst) HIP_TRY(copy_sync(k.dst, k.src, 4ull * k.words, hipMemcpyDeviceToHost, c->stream));
    }
    if ((rc = finish_query(c, !host, launches, st)) != ZRT_OK) return rc;
    if (host) {                                            // the kernels' time, without the copies
        float ms = 0.0f;
        HIP_TRY(hipEventElapsedTime(&ms, c->ev_begin, c->ev_trace[1]));
        st.trace_kernel_ms = ms;
    }
    unsigned long long hs[4];
    HIP_TRY(copy_sync(hs, c->d_stats, sizeof hs, hipMemcpyDeviceToHost, c->stream));
    st.segments = st.samples = (uint64_t)P * spp;
    st.hits = hs[3];
    if (counting) {
        st.cells_visited = hs[1];
        st.triangle_tests = hs[2];
    }
    if (stats) *stats = st;
    return ZRT_OK;
}

// Scene.traceRay (stage3.zig:152-186) for a batch of rays: see include/zrt.h
// and the kernels' comment (query_walk_kernel).  The launch plan is the one a
// render resolves (resolve_plan); the park path from kTraceParkMin rays, or as
// ZRT_TRACE_PARK asks.  Per chunk of at most kTraceChunk rays, all on the
// context's stream (trace_first_segments):
//   lane walk:  query_walk_kernel (fast kernel of the context, kRaysFast), then
//               the IEEE-division kernel over the rays it left (kRaysRest);
//               an mt_exact context, ZRT_FLAG_MT_EXACT or a counting call:
//               that kernel alone over every ray (kRaysAll);
//   park path:  query_pack_kernel -> wf_park_kernel (the render's, unchanged)
//               -> query_out_kernel, then the kRaysRest launch as above.
// The park path shares pass set 0's queue, hit records and counters with the
// renders; each use writes what it reads first, so nothing carries over.
//
// zrt_context_segments is the same call -- plan, chunk loop,
// launches, stats -- with the kernels' SEG instantiations (ray_launch's `seg`) and two
// more per-ray arrays: the bounds, staged behind a chunk's rays, and the
// occlusion bytes, staged behind its hit records.
//
// zrt_context_surface is the trace call with one more launch per
// chunk, surface_kernel over the chunk's hit records, and one more per-ray
// array: the records, staged in a buffer of their own.  A device batch without
// `hits` keeps the chunk's hit records in the context's staging buffer.
struct RayQuery {
    uint64_t num_rays;
    const float* rays;
    zrt_hit* hits;            // (a segment call: may be null)
    uint32_t on_device, flags;
    int seg;                  // -1: zrt_context_trace; 0 / 1: segments, closest / any-hit
    const float* t_max;
    float t_max_all;
    uint8_t* occ;
    zrt_surface* surf;        // zrt_context_surface: a record per ray (seg = -1), else null
};
static int query_rays(zrt_context* c, const RayQuery* b, zrt_stats* stats) {
    zrt_stats st{};
    DeviceGuard g(c->device);
    const bool seg = b->seg >= 0;

    const bool counting = (b->flags & ZRT_FLAG_COUNT_STATS) != 0;
    LaunchPlan pl;
    int rc;
    if ((rc = resolve_plan(c, b->flags, counting,
                           (b->flags & ZRT_TRACE_PARK) || b->num_rays >= (seg ? kSegParkMin : kTraceParkMin),
                           b->num_rays >= kSetsMinSamples, pl)) != ZRT_OK)
        return rc;
    const bool park = pl.park;

    // chunk size (query_chunk; this call also reuses the surface records), then
    // the buffers a launch below writes, each grown to a chunk and guarded
    zrt_context::PassSet& ps = c->set[0];
    const bool host = !b->on_device;
    const bool own_hits = b->surf && b->on_device && !b->hits;    // the gather reads records the caller did not ask for
    const uint64_t per_ray = (host ? 40ull + (seg ? kSegStageBytes : 0ull) + (b->surf ? 64ull : 0ull)
                                   : own_hits ? 16ull : 0ull) +
                             (park ? 64ull : 0ull);
    const uint64_t chunk = query_chunk(c, b->num_rays, per_ray, query_held(c) + 16ull * c->surf_cap);
    // staging words of a host batch's chunk: rays (+ bounds), hit records (+ bytes)
    const uint64_t rays_words = 6 * chunk + (seg ? chunk : 0), hits_words = 4 * chunk + (seg ? (chunk + 3) / 4 : 0);
    if (host && (rc = grow_checked("rays", &c->d_rays, &c->rays_cap, rays_words)) != ZRT_OK) return rc;
    if ((host || own_hits) && (rc = grow_checked("hits", &c->d_hits, &c->hits_cap, hits_words)) != ZRT_OK) return rc;
    if (host && b->surf && (rc = grow_checked("surfaces", &c->d_surf, &c->surf_cap, 4 * chunk)) != ZRT_OK) return rc;
    // (the counters: a render's smallest; this call uses 16)
    if (park && (rc = grow_park_buffers(ps, chunk, 0, chunk, wfc_words(0))) != ZRT_OK) return rc;
    if ((rc = event_pool(c->ev_trace, 2)) != ZRT_OK) return rc;

    // occupancy-sized persistent grids (no more blocks than a chunk has work for)
    RayLaunch rl;
    if ((rc = ray_launch(c, pl, counting, park, rl, b->seg)) != ZRT_OK) return rc;

    QueryParams R;
    memset(&R, 0, sizeof R);
    R.t_max_all = b->t_max_all;
    R.count = b->seg == 1 ? 1u : 0u;               // an any-hit call: its kernels count the rays not missed
    query_params(c, R);
    if (park) query_park_params(c, pl, ps, R);

    HIP_TRY(hipMemsetAsync(c->d_stats, 0, 512, c->stream));
    HIP_TRY(hipEventRecord(c->ev_begin, c->stream));
    SurfaceParams S;
    memset(&S, 0, sizeof S);
    S.tri_data = c->d_data;
    S.mats = c->d_mats;
    S.texels = c->d_texels;
    uint32_t launches = 0;
    for (uint64_t off = 0; off < b->num_rays; off += chunk) {
        const uint32_t n = (uint32_t)std::min<uint64_t>(chunk, b->num_rays - off);
        if (b->on_device) {
            R.rays = b->rays + 6 * off;
            R.hits = b->hits ? reinterpret_cast<uint32_t*>(b->hits + off) : own_hits ? c->d_hits : nullptr;
            S.surf = reinterpret_cast<float4*>(b->surf + off);
            R.t_max = b->t_max ? b->t_max + off : nullptr;
            R.occ = b->occ ? b->occ + off : nullptr;
        } else {
            if ((rc = stage_chunk(c, b->rays + 6 * off, b->t_max ? b->t_max + off : nullptr, chunk, n)) != ZRT_OK) return rc;
            R.rays = c->d_rays;
            R.hits = b->hits || b->surf ? c->d_hits : nullptr;
            S.surf = c->d_surf;
            if (b->t_max) R.t_max = c->d_rays + 6 * chunk;
            if (b->occ) R.occ = reinterpret_cast<uint8_t*>(c->d_hits + 4 * chunk);
        }
        HIP_TRY(hipMemsetAsync(c->d_counter, 0, 64, c->stream));
        // the work counters; query_pack_kernel writes the region counts
        if (park) HIP_TRY(hipMemsetAsync(ps.wfc, 0, 4ull * 16 * kCtr, c->stream));
        if ((rc = trace_first_segments(c, pl, rl, R, n, true, &launches)) != ZRT_OK) return rc;
        if (b->surf) {                                 // the gather: one thread per ray over the records just written
            S.rays = R.rays;
            S.hits = R.hits;
            S.n = n;
            hipLaunchKernelGGL(surface_kernel, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, c->stream, S);
            ++launches;
            HIP_TRY(hipGetLastError());
        }
        if (!b->on_device) {
            HIP_TRY(hipEventRecord(c->ev_trace[1], c->stream));
            if (b->hits) HIP_TRY(copy_sync(b->hits + off, c->d_hits, 16ull * n, hipMemcpyDeviceToHost, c->stream));
            if (b->surf) HIP_TRY(copy_sync(b->surf + off, c->d_surf, 64ull * n, hipMemcpyDeviceToHost, c->stream));
            if (b->occ) HIP_TRY(copy_sync(b->occ + off, R.occ, n, hipMemcpyDeviceToHost, c->stream));
            if ((rc = chunk_kernel_time(c, st)) != ZRT_OK) return rc;
        }
    }
    unsigned long long hs[4];
    const bool read = counting || b->seg == 1;     // (an any-hit call counts its bytes in every call)
    if ((rc = query_stats(c, b->on_device != 0, launches, counting, hs, read ? 4 : 0, st)) != ZRT_OK) return rc;
    st.segments = b->num_rays;
    if (read) st.hits = hs[3];
    if (stats) *stats = st;
    return ZRT_OK;
}

extern "C" int zrt_context_trace(zrt_context* c, const zrt_ray_batch* b, zrt_stats* stats) {
    if (!c || !b) return ZRT_ERR_INVALID_ARG;
    if ((b->flags & ~kTraceFlags) != 0u || b->on_device > 1u) return ZRT_ERR_INVALID_ARG;
    if (b->num_rays == 0) { if (stats) *stats = zrt_stats{}; return ZRT_OK; }
    if (!b->rays || !b->hits) return ZRT_ERR_INVALID_ARG;
    const RayQuery q{b->num_rays, b->rays, b->hits, b->on_device, b->flags, -1, nullptr, 0.0f, nullptr, nullptr};
    return query_rays(c, &q, stats);
}

// The shading inputs at each ray's first hit: see include/zrt.h and DESIGN 5.14.
extern "C" int zrt_context_surface(zrt_context* c, const zrt_surface_batch* b, zrt_stats* stats) {
    if (!c || !b) return ZRT_ERR_INVALID_ARG;
    if ((b->flags & ~kTraceFlags) != 0u || b->on_device > 1u) return ZRT_ERR_INVALID_ARG;
    if (b->num_rays == 0) { if (stats) *stats = zrt_stats{}; return ZRT_OK; }
    if (!b->rays || !b->surfaces) return ZRT_ERR_INVALID_ARG;
    // surface_kernel stores a record as four 16-byte words
    if (b->on_device && (reinterpret_cast<uintptr_t>(b->surfaces) & 15u) != 0u) return ZRT_ERR_INVALID_ARG;
    const RayQuery q{b->num_rays, b->rays, b->hits, b->on_device, b->flags, -1, nullptr, 0.0f, nullptr, b->surfaces};
    return query_rays(c, &q, stats);
}

// Bounded segments, closest or any-hit: see include/zrt.h and DESIGN 5.13.
extern "C" int zrt_context_segments(zrt_context* c, const zrt_segment_batch* b, zrt_stats* stats) {
    if (!c || !b) return ZRT_ERR_INVALID_ARG;
    if ((b->flags & ~(kTraceFlags | ZRT_SEGMENT_ANY)) != 0u || b->on_device > 1u || b->_reserved != 0u)
        return ZRT_ERR_INVALID_ARG;
    const bool any = (b->flags & ZRT_SEGMENT_ANY) != 0;
    if (any && b->hits) return ZRT_ERR_INVALID_ARG;
    if (b->num_rays == 0) { if (stats) *stats = zrt_stats{}; return ZRT_OK; }
    if (!b->rays || (!b->hits && !b->occluded)) return ZRT_ERR_INVALID_ARG;
    const RayQuery q{b->num_rays, b->rays, b->hits, b->on_device, b->flags & ~ZRT_SEGMENT_ANY, any ? 1 : 0,
                     b->t_max, b->t_max_all, b->occluded, nullptr};
    return query_rays(c, &q, stats);
}

// Transmittance along bounded rays: see include/zrt.h, the kernels' comment
// (TransmitParams) and DESIGN 5.15.  query_rays' plan, chunk loop, staging and
// stats (the helpers above); its launches per chunk differ:
//   lane path:  transmit_walk_kernel as query_rays launches query_walk_kernel
//               (transmit_chains: kRaysFast then kRaysRest, or kRaysAll), whole
//               chains per lane;
//   park path:  query_pack_kernel<SEG> -> per round k < max_crossings:
//               wf_park_kernel (bounded closest mode, unchanged) over queue
//               k & 1 -> transmit_step_kernel, which appends the surviving
//               rays to the other queue; the host reads that queue's eight
//               region counts back, leaves the loop when they are all zero and
//               hands kTransmitTailMax survivors or fewer to one kRaysQueue
//               launch of the fast lane kernel (ZRT_TRANSMIT_ROUNDS=fixed in
//               the environment: no read-back, max_crossings rounds whose
//               kernels return on an empty queue; measured in DESIGN 5.15);
//               then the kRaysRest launch of the IEEE-division lane kernel for
//               the rays outside the fast domain.
// Round k has its own work counters and region counts in pass set 0's counter
// block (bounce_params' layout), zeroed once per chunk.  Staging of a host
// batch: rays and bounds in d_rays, T and n in d_hits; a device batch without
// `crossings` on the park path keeps n there.
extern "C" int zrt_context_transmittance(zrt_context* c, const zrt_transmittance_batch* b, zrt_stats* stats) {
    if (!c || !b) return ZRT_ERR_INVALID_ARG;
    if ((b->flags & ~kTraceFlags) != 0u || b->on_device > 1u || b->max_crossings == 0u || b->max_crossings > 256u)
        return ZRT_ERR_INVALID_ARG;
    if (b->num_rays == 0) { if (stats) *stats = zrt_stats{}; return ZRT_OK; }
    if (!b->rays || !b->transmittance) return ZRT_ERR_INVALID_ARG;
    zrt_stats st{};
    DeviceGuard g(c->device);
    const bool counting = (b->flags & ZRT_FLAG_COUNT_STATS) != 0;
    const uint32_t cap = b->max_crossings;
    LaunchPlan pl;
    int rc;
    // The park path only where ZRT_TRACE_PARK asks for it: unlike a segment
    // call's (kSegParkMin), this call's lane path was as fast or faster at
    // 2^16 and 2^20 rays on both scenes of tools/transmit_bench.py (DESIGN
    // 5.15: the chains' later rounds hold few rays, which the park launches'
    // fixed cost does not suit), so no batch size takes it unasked.
    if ((rc = resolve_plan(c, b->flags, counting, (b->flags & ZRT_TRACE_PARK) != 0, b->num_rays >= kSetsMinSamples,
                           pl)) != ZRT_OK)
        return rc;
    const bool park = pl.park;
    const char* rounds_env = getenv("ZRT_TRANSMIT_ROUNDS");
    const bool fixed_rounds = rounds_env && strcmp(rounds_env, "fixed") == 0;
    uint64_t tail_max = kTransmitTailMax;
    if (const char* e = getenv("ZRT_TRANSMIT_TAIL")) tail_max = (uint64_t)std::max(0ll, atoll(e));

    // chunk size (query_chunk; the park path's two queues and hit records are
    // 2 * 48 + 16 B per ray, and the second queue is reused too), then the
    // buffers a launch below writes, each grown to a chunk and guarded
    zrt_context::PassSet& ps = c->set[0];
    const bool host = !b->on_device;
    const bool own_n = b->on_device && park && !b->crossings;
    const uint64_t per_ray = (host ? 36ull : own_n ? 4ull : 0ull) + (park ? 112ull : 0ull);
    const uint64_t chunk = query_chunk(c, b->num_rays, per_ray, query_held(c) + 16ull * ps.q1_cap);
    if (host && (rc = grow_checked("rays", &c->d_rays, &c->rays_cap, 7 * chunk)) != ZRT_OK) return rc;
    if ((host || own_n) && (rc = grow_checked("T, n", &c->d_hits, &c->hits_cap, host ? 2 * chunk : chunk)) != ZRT_OK)
        return rc;
    // counters of a chunk's rounds: 8 work counters and 8 region counts per round, one more round's region counts
    const size_t ctr_words = kCtr * 16ull * (cap + 1ull);
    if (park && (rc = grow_park_buffers(ps, chunk, chunk, chunk, ctr_words)) != ZRT_OK) return rc;
    if ((rc = event_pool(c->ev_trace, 2)) != ZRT_OK) return rc;

    // the kernels and their occupancy-sized persistent grids (the park path launches the fast one for its tail)
    const WfFn f_park = park_fn<kParkClosest>(pl.esc, pl.pbm);
    uint32_t grid_park = 0;
    if (park && (rc = resident_blocks(c, (const void*)f_park, pl.park_block, pl.lds_park, &grid_park)) != ZRT_OK) return rc;
    TransmitLaunch tl;
    if ((rc = transmit_launch(c, pl, counting, true, tl)) != ZRT_OK) return rc;

    TransmitParams R;
    memset(&R, 0, sizeof R);
    R.q.t_max_all = b->t_max_all;
    R.max_cross = cap;
    query_params(c, R.q);
    if (park) {                                        // (the rounds below wire the queues and counters)
        R.q.w.hit = ps.hit;
        park_params(c, pl, R.q.w);
    }

    HIP_TRY(hipMemsetAsync(c->d_stats, 0, 512, c->stream));
    HIP_TRY(hipEventRecord(c->ev_begin, c->stream));
    uint32_t launches = 0;
    for (uint64_t off = 0; off < b->num_rays; off += chunk) {
        const uint32_t n = (uint32_t)std::min<uint64_t>(chunk, b->num_rays - off);
        const uint32_t nblk = (n + kBlock - 1) / kBlock;
        if (b->on_device) {
            R.q.rays = b->rays + 6 * off;
            R.q.t_max = b->t_max ? b->t_max + off : nullptr;
            R.T = b->transmittance + off;
            R.cross = b->crossings ? b->crossings + off : own_n ? c->d_hits : nullptr;
        } else {
            if ((rc = stage_chunk(c, b->rays + 6 * off, b->t_max ? b->t_max + off : nullptr, chunk, n)) != ZRT_OK) return rc;
            R.q.rays = c->d_rays;
            if (b->t_max) R.q.t_max = c->d_rays + 6 * chunk;
            R.T = reinterpret_cast<float*>(c->d_hits);
            R.cross = c->d_hits + chunk;
        }
        HIP_TRY(hipMemsetAsync(c->d_counter, 0, 64, c->stream));
        if (park) {
            identity_queue(R.q, n);
            HIP_TRY(hipMemsetAsync(ps.wfc, 0, 4ull * ctr_words, c->stream));
            QueryParams Q = R.q;                       // the queue fill: query_pack_kernel<SEG>, (d, bound) records
            Q.which = kRaysAll;
            Q.q = ps.q0;
            Q.n_in8 = region_counts(ps, 0);
            hipLaunchKernelGGL(kQuery[1].pack, dim3(nblk), dim3(kBlock), 0, c->stream, Q);
            ++launches;
            for (uint32_t k = 0; k < cap; ++k) {       // (bounded by the cap whatever the device says)
                float4* const qin = (k & 1u) ? ps.q1 : ps.q0;
                R.q.w.q_in = qin;
                R.q.w.fetch8 = ps.wfc + kCtr * (16 * k);
                R.q.w.n_in8 = region_counts(ps, k);
                R.q_in = qin;
                R.q_out = (k & 1u) ? ps.q0 : ps.q1;
                R.n_out8 = region_counts(ps, k + 1);
                R.first = k == 0u ? 1u : 0u;
                hipLaunchKernelGGL(f_park, dim3(grid_park), dim3(pl.park_block), pl.lds_park, c->stream, R.q.w);
                hipLaunchKernelGGL(transmit_step_kernel, dim3(nblk), dim3(kBlock), 0, c->stream, R);
                launches += 2;
                HIP_TRY(hipGetLastError());
                if (k + 1u == cap) break;              // (a ray that got this far has n == cap: none was appended)
                if (!fixed_rounds) {
                    uint32_t left[8 * kCtr];
                    HIP_TRY(copy_sync(left, R.n_out8, sizeof left, hipMemcpyDeviceToHost, c->stream));
                    uint64_t alive = 0;
                    for (uint32_t gq = 0; gq < 8u; ++gq) alive += left[gq * kCtr];
                    if (alive == 0u) break;
                    if (alive <= tail_max) {           // the tail: the survivors' whole chains in one lane launch
                        R.q_in = R.q_out;
                        R.q.w.n_in8 = R.n_out8;
                        transmit_walk(c, pl, tl.f_fast, tl.grid_fast, nblk, R, kRaysQueue, &launches);
                        break;
                    }
                }
            }
            transmit_walk(c, pl, tl.f_exact, tl.grid_exact, nblk, R, kRaysRest, &launches);
        } else {
            transmit_chains(c, pl, tl, R, n, &launches);
        }
        HIP_TRY(hipGetLastError());
        if (host) {
            HIP_TRY(hipEventRecord(c->ev_trace[1], c->stream));
            HIP_TRY(copy_sync(b->transmittance + off, R.T, 4ull * n, hipMemcpyDeviceToHost, c->stream));
            if (b->crossings) HIP_TRY(copy_sync(b->crossings + off, R.cross, 4ull * n, hipMemcpyDeviceToHost, c->stream));
            if ((rc = chunk_kernel_time(c, st)) != ZRT_OK) return rc;
        }
    }
    unsigned long long hs[4];
    if ((rc = query_stats(c, !host, launches, counting, hs, 4, st)) != ZRT_OK) return rc;
    st.segments = hs[0];
    st.hits = hs[3];
    if (stats) *stats = st;
    return ZRT_OK;
}

// Hemisphere occlusion at each ray's first hit: see include/zrt.h, the kernels'
// comment (OcclusionParams) and DESIGN 5.17.  query_rays' plan, chunk loop,
// staging and stats (the helpers above) and its first hits; the items' loop --
// two live counts, a park path of its own, a finish pass -- is this call's
// alone.  Per chunk of at most kTraceChunk rays, all on the context's stream:
//   the first hits as zrt_context_trace traces them (trace_first_segments, the
//   park path from kTraceParkMin rays or as ZRT_TRACE_PARK asks), their records
//   in `hits` or in the context's staging buffer; the counts zeroed;
//   per sub-chunk of at most kOccItems items:
//     occlusion_gen_kernel, then the two live counts read back;
//     park path:  wf_park_kernel (bounded closest mode, unchanged) over the
//                 queue the gen kernel appended -> occlusion_reduce_kernel
//                 (kOccQueue); then, if the list holds any item (outside the
//                 fast domain), the IEEE-division lane kernel over it (kRaysAll)
//                 -> occlusion_reduce_kernel (kOccList);
//     lane path:  the segment call's query_walk_kernel launches over the list
//                 (kRaysFast then kRaysRest; an mt_exact context, a flag or a
//                 counting call: kRaysAll, a counting call with the any-hit
//                 exit) -> occlusion_reduce_kernel (kOccList);
//   occlusion_reduce_kernel (kOccFinish): the visibilities.
// The park path is pass set 0's queue, hit records and counters; the list and a
// host batch's rays and radii lie in d_rays, the hit records, counts,
// visibilities and the list's bytes in d_hits.  Each use writes what it reads
// first.
extern "C" int zrt_context_occlusion(zrt_context* c, const zrt_occlusion_batch* b, zrt_stats* stats) {
    if (!c || !b) return ZRT_ERR_INVALID_ARG;
    if ((b->flags & ~kTraceFlags) != 0u || b->on_device > 1u || b->num_samples == 0u || b->num_samples > 65535u)
        return ZRT_ERR_INVALID_ARG;
    if (b->num_rays == 0) { if (stats) *stats = zrt_stats{}; return ZRT_OK; }
    if (!b->rays || (!b->visibility && !b->occluded)) return ZRT_ERR_INVALID_ARG;
    zrt_stats st{};
    DeviceGuard g(c->device);
    const bool counting = (b->flags & ZRT_FLAG_COUNT_STATS) != 0;
    const uint32_t S = b->num_samples;
    const bool asked = (b->flags & ZRT_TRACE_PARK) != 0;
    const bool want_first = asked || b->num_rays >= kTraceParkMin;
    // (ZRT_OCCLUSION_PARK_MIN in the environment overrides the samples' threshold, for tools/occlusion_bench.py)
    uint64_t park_min = kOccParkMin;
    if (const char* e = getenv("ZRT_OCCLUSION_PARK_MIN")) park_min = (uint64_t)std::max(0ll, atoll(e));
    const bool want_items = asked || b->num_rays * S >= park_min;
    LaunchPlan pl;
    int rc;
    if ((rc = resolve_plan(c, b->flags, counting, want_first || want_items, b->num_rays * S >= kSetsMinSamples, pl)) !=
        ZRT_OK)
        return rc;
    const bool park_first = pl.park_ok && want_first, park_items = pl.park_ok && want_items;

    // chunk size (query_chunk); a sub-chunk's buffers are bounded by kOccItems
    zrt_context::PassSet& ps = c->set[0];
    const bool dev = b->on_device != 0;
    const bool own_hits = !dev || !b->hits, own_occ = !dev || !b->occluded, own_vis = !dev && b->visibility;
    const uint64_t per_ray = (dev ? 0ull : 28ull) + (own_hits ? 16ull : 0ull) + (own_occ ? 4ull : 0ull) +
                             (own_vis ? 4ull : 0ull) + (park_first ? 64ull : 0ull);
    const uint64_t chunk = query_chunk(c, b->num_rays, per_ray, query_held(c));
    const uint64_t M = std::min<uint64_t>(kOccItems, chunk * S);          // items of a sub-chunk
    // words of d_rays: a host batch's rays and radii, then the list
    const uint64_t off_list = dev ? 0 : 7 * chunk, rays_words = off_list + 8 * M;
    // words of d_hits: hit records, counts, visibilities, the list's bytes
    const uint64_t off_occ = own_hits ? 4 * chunk : 0, off_vis = off_occ + (own_occ ? chunk : 0),
                   off_bytes = off_vis + (own_vis ? chunk : 0), hits_words = off_bytes + (M + 3) / 4;
    const uint64_t q_slots = std::max<uint64_t>(park_first ? chunk : 0, park_items ? M : 0);
    // every buffer a launch below writes, grown to a chunk / a sub-chunk and guarded
    if ((rc = grow_checked("rays, list", &c->d_rays, &c->rays_cap, rays_words)) != ZRT_OK) return rc;
    if ((rc = grow_checked("hits, counts", &c->d_hits, &c->hits_cap, hits_words)) != ZRT_OK) return rc;
    if (q_slots && (rc = grow_park_buffers(ps, q_slots, 0, q_slots, wfc_words(0))) != ZRT_OK) return rc;
    if ((rc = event_pool(c->ev_trace, 2)) != ZRT_OK) return rc;

    RayLaunch rl, ri;                              // the first hits: a trace call's; the items: a segment call's
    if ((rc = ray_launch(c, pl, counting, park_first, rl, -1)) != ZRT_OK) return rc;
    if ((rc = ray_launch(c, pl, counting, false, ri, counting ? 1 : 0)) != ZRT_OK) return rc;
    if (park_items && (rc = resident_blocks(c, (const void*)ri.f_park, pl.park_block, pl.lds_park, &ri.grid_park)) != ZRT_OK)
        return rc;

    QueryParams R;
    memset(&R, 0, sizeof R);
    query_params(c, R);
    if (q_slots) query_park_params(c, pl, ps, R);
    OcclusionParams O;
    memset(&O, 0, sizeof O);
    O.radius_all = b->radius_all;
    O.S = S;
    O.tri_data = c->d_data;
    O.mats = c->d_mats;
    O.texels = c->d_texels;
    O.zig = c->d_zig;
    O.seed = b->seed;
    O.park = park_items ? 1u : 0u;
    O.q = ps.q0;
    O.n_in8 = q_slots ? region_counts(ps, 0) : nullptr;
    O.hit = ps.hit;
    O.irays = c->d_rays + off_list;
    O.ibound = O.irays + 6 * M;
    O.iitem = reinterpret_cast<uint32_t*>(O.ibound + M);
    O.occ = reinterpret_cast<const uint8_t*>(c->d_hits + off_bytes);
    O.ctr = c->d_counter;
    O.stats = c->d_stats;
    // the items' walks: the list as a segment call's rays, bounds and bytes
    QueryParams I = R;
    I.rays = O.irays;
    I.t_max = O.ibound;
    I.occ = reinterpret_cast<uint8_t*>(c->d_hits + off_bytes);

    HIP_TRY(hipMemsetAsync(c->d_stats, 0, 512, c->stream));
    HIP_TRY(hipEventRecord(c->ev_begin, c->stream));
    uint32_t launches = 0;
    uint64_t traced = 0;
    for (uint64_t off = 0; off < b->num_rays; off += chunk) {
        const uint32_t n = (uint32_t)std::min<uint64_t>(chunk, b->num_rays - off);
        const uint32_t nblk = (n + kBlock - 1) / kBlock;
        if (dev) {
            R.rays = b->rays + 6 * off;
            O.radius = b->radius ? b->radius + off : nullptr;
        } else {
            if ((rc = stage_chunk(c, b->rays + 6 * off, b->radius ? b->radius + off : nullptr, chunk, n)) != ZRT_OK) return rc;
            R.rays = c->d_rays;
            if (b->radius) O.radius = c->d_rays + 6 * chunk;
        }
        R.hits = own_hits ? c->d_hits : reinterpret_cast<uint32_t*>(b->hits + off);
        O.occluded = own_occ ? c->d_hits + off_occ : b->occluded + off;
        O.visibility = own_vis ? reinterpret_cast<float*>(c->d_hits + off_vis) : dev && b->visibility ? b->visibility + off
                                                                                                      : nullptr;
        HIP_TRY(hipMemsetAsync(c->d_counter, 0, 64, c->stream));
        if (park_first) HIP_TRY(hipMemsetAsync(ps.wfc, 0, 4ull * 16 * kCtr, c->stream));
        if ((rc = trace_first_segments(c, pl, rl, R, n, true, &launches)) != ZRT_OK) return rc;
        HIP_TRY(hipMemsetAsync(O.occluded, 0, 4ull * n, c->stream));
        O.rays = R.rays;
        O.hits = R.hits;
        O.n = n;
        O.key0 = (uint32_t)(b->index_base + off);
        const uint64_t items = (uint64_t)n * S;
        for (uint64_t i0 = 0; i0 < items; i0 += kOccItems) {
            const uint32_t m = (uint32_t)std::min<uint64_t>(kOccItems, items - i0);
            const uint32_t mblk = (m + kBlock - 1) / kBlock;
            O.ray0 = (uint32_t)(i0 / S);
            O.s0 = (uint32_t)(i0 % S);
            O.m = m;
            HIP_TRY(hipMemsetAsync(c->d_counter, 0, 64, c->stream));
            // the park kernel's work counters and the region counts the gen kernel adds to
            if (park_items) HIP_TRY(hipMemsetAsync(ps.wfc, 0, 4ull * 16 * kCtr, c->stream));
            hipLaunchKernelGGL(occlusion_gen_kernel, dim3((mblk + kOccGenItems - 1) / kOccGenItems), dim3(kBlock), 0,
                               c->stream, O);
            ++launches;
            HIP_TRY(hipGetLastError());
            uint32_t live[2] = {0, 0};                 // the list's entries, every live item
            HIP_TRY(copy_sync(live, c->d_counter + 4, sizeof live, hipMemcpyDeviceToHost, c->stream));
            if (live[0] > m || live[1] > m || live[0] > live[1]) return ZRT_ERR_HIP;   // (never: the kernel's own bounds)
            traced += live[1];
            if (park_items && live[1] > live[0]) {
                identity_queue(I, m);                  // (I.n: the list walks below set their own)
                hipLaunchKernelGGL(ri.f_park, dim3(ri.grid_park), dim3(pl.park_block), pl.lds_park, c->stream, I.w);
                O.mode = kOccQueue;
                hipLaunchKernelGGL(occlusion_reduce_kernel, dim3(mblk), dim3(kBlock), 0, c->stream, O);
                launches += 2;
            }
            if (live[0] != 0u) {
                const uint32_t lblk = (live[0] + kBlock - 1) / kBlock;
                I.n = live[0];
                auto walk = [&](QueryFn f, uint32_t grid, uint32_t which) {
                    I.which = which;
                    hipLaunchKernelGGL(f, dim3(std::min(grid, lblk)), dim3(kTraceThreads), pl.lds_wf, c->stream, I);
                    ++launches;
                };
                if (!park_items && ri.f_fast) {
                    walk(ri.f_fast, ri.grid_fast, kRaysFast);
                    walk(ri.f_exact, ri.grid_exact, kRaysRest);
                } else {
                    walk(ri.f_exact, ri.grid_exact, kRaysAll);
                }
                O.mode = kOccList;
                O.nl = live[0];
                hipLaunchKernelGGL(occlusion_reduce_kernel, dim3(lblk), dim3(kBlock), 0, c->stream, O);
                ++launches;
            }
            HIP_TRY(hipGetLastError());
        }
        if (O.visibility) {
            O.mode = kOccFinish;
            hipLaunchKernelGGL(occlusion_reduce_kernel, dim3(nblk), dim3(kBlock), 0, c->stream, O);
            ++launches;
            HIP_TRY(hipGetLastError());
        }
        if (!dev) {
            HIP_TRY(hipEventRecord(c->ev_trace[1], c->stream));
            if (b->hits) HIP_TRY(copy_sync(b->hits + off, c->d_hits, 16ull * n, hipMemcpyDeviceToHost, c->stream));
            if (b->occluded) HIP_TRY(copy_sync(b->occluded + off, O.occluded, 4ull * n, hipMemcpyDeviceToHost, c->stream));
            if (b->visibility)
                HIP_TRY(copy_sync(b->visibility + off, O.visibility, 4ull * n, hipMemcpyDeviceToHost, c->stream));
            if ((rc = chunk_kernel_time(c, st)) != ZRT_OK) return rc;
        }
    }
    unsigned long long hs[kOccStat + 1];
    if ((rc = query_stats(c, dev, launches, counting, hs, kOccStat + 1, st)) != ZRT_OK) return rc;
    st.segments = b->num_rays + traced;
    st.hits = hs[kOccStat];
    if (stats) *stats = st;
    return ZRT_OK;
}

// The fields of their own that the two item-parameter structs of light_items
// get there: the call's own rows in d_rays (`rows`: behind a host batch's rays;
// `extra`: the row between T and the slots), and the stream key of a chunk's
// ray 0.  Direct: the lights and the items' factors; area lights: the items'
// contributions, a float4 each.
static void light_rows(DirectParams& D, float* rows, float* extra) {
    D.lights = reinterpret_cast<const zrt_light*>(rows);
    D.f = extra;
}
static void light_key(DirectParams&, uint64_t) {}          // (its items draw nothing)
static void light_rows(AreaParams& D, float* rows, float*) { D.contrib = reinterpret_cast<float4*>(rows); }
static void light_key(AreaParams& D, uint64_t key) { D.key0 = (uint32_t)key; }
static void light_rows(SkyParams&, float*, float*) {}      // (the sky's colour is read off the list)
static void light_key(SkyParams& D, uint64_t key) { D.key0 = (uint32_t)key; }
// ... and the per-ray visibility row, which the sky-light call alone has
static void light_vis(DirectParams&, float*) {}
static void light_vis(AreaParams&, float*) {}
static void light_vis(SkyParams& D, float* v) { D.V = v; }
static_assert(kAreaItems == kDirItems && kAreaStat == kDirStat, "light_items: one sub-chunk size, one pair of statistics");

// What zrt_context_direct, zrt_context_area_lights and zrt_context_sky_light
// share (light_items): per ray the irradiance of `per` light items at its first
// hit, each shadowed by a transmittance chain, and the radiance it gives (the
// sky-light call: the visibility too).  The plan, chunk loop,
// staging and stats are zrt_context_occlusion's.  Per chunk of at most
// kTraceChunk rays, all on the context's stream:
//   the first hits as zrt_context_trace traces them (trace_first_segments, the
//   park path from kTraceParkMin rays or as ZRT_TRACE_PARK asks), their records
//   in `hits` or in the context's staging buffer; the walk counters those
//   launches added to (stats[0], stats[3]) cleared;
//   per sub-chunk of at most kDirItems items:
//     the call's gen kernel, then the list's size read back;
//     the transmittance call's lane launches over the list (transmit_chains:
//     kRaysFast then kRaysRest; an mt_exact context, a flag or a counting call:
//     kRaysAll), unless the list is empty or the call is unshadowed;
//     the call's reduce kernel.
// The chains never take the park-and-step rounds (DESIGN 5.15 measured the lane
// chain as fast or faster).  d_rays holds a host batch's rays, then the call's
// own rows (light_rows: `head_words` words, and `item_words` per item from a
// 16-byte boundary), then the list (rays, bounds), T, `extra_rows` rows of the
// call's own and the slots; d_hits the hit records and a host batch's (or an
// unasked) irradiance and radiance and, for a call with a per-ray visibility
// (`has_vis`: the sky-light call), that row on the same terms: a ray's sum
// waits in it across a sub-chunk cut whether it was asked for or not.  Each use
// writes what it reads first.
struct LightCall {
    uint64_t num_rays;
    const float* rays;
    zrt_hit* hits;            // may be null
    float* irradiance;        // may be null
    float* radiance;          // may be null (one of irradiance, radiance and visibility is not)
    bool dev;                 // the batch's pointers are the device's
    uint32_t flags;           // the batch's, without the call's own bits
    bool unshadowed;
    bool any;                 // false: no item can be traced (an empty set)
    uint32_t per;             // items per ray: lights, samples
    uint32_t max_crossings;
    uint64_t index_base;      // stream key of ray 0 (light_key)
    const void* head;         // uploaded once to the head of the call's own rows, or null
    uint64_t head_words;
    uint32_t item_words, extra_rows;
    bool has_vis;             // the call has a per-ray visibility (light_vis)
    float* visibility;        // may be null
};
template <class P>
static int light_items(zrt_context* c, const LightCall& k, P& D, int (*gen)(const P&, hipStream_t),
                       int (*reduce)(const P&, uint32_t, hipStream_t), zrt_stats* stats) {
    zrt_stats st{};
    const bool counting = (k.flags & ZRT_FLAG_COUNT_STATS) != 0;
    const uint32_t per = k.per;
    const bool want_first = (k.flags & ZRT_TRACE_PARK) != 0 || k.num_rays >= kTraceParkMin;
    LaunchPlan pl;
    int rc;
    if ((rc = resolve_plan(c, k.flags, counting, want_first, k.num_rays >= kSetsMinSamples, pl)) != ZRT_OK) return rc;
    const bool park_first = pl.park_ok && want_first;

    // chunk size (query_chunk); a sub-chunk's buffers are bounded by kDirItems
    zrt_context::PassSet& ps = c->set[0];
    const bool dev = k.dev;
    const bool own_hits = !dev || !k.hits, own_E = !dev || !k.irradiance, own_rad = !dev && k.radiance;
    const bool own_V = k.has_vis && (!dev || !k.visibility);
    const uint64_t per_ray = (dev ? 0ull : 24ull) + (own_hits ? 16ull : 0ull) + (own_E ? 12ull : 0ull) +
                             (own_rad ? 12ull : 0ull) + (own_V ? 4ull : 0ull) + (park_first ? 64ull : 0ull);
    const uint64_t chunk = query_chunk(c, k.num_rays, per_ray, query_held(c));
    const uint64_t M = std::min<uint64_t>(kDirItems, chunk * per);        // items of a sub-chunk
    // words of d_rays: a host batch's rays, the call's own rows, the list (rays, bounds), T, its extra rows, slots
    const uint64_t off_rows = k.item_words ? ((dev ? 0 : 6 * chunk) + 3) & ~3ull : dev ? 0 : 6 * chunk,
                   off_list = off_rows + k.head_words + k.item_words * M, rays_words = off_list + (9 + k.extra_rows) * M;
    // words of d_hits: hit records, irradiance, radiance, visibility
    const uint64_t off_E = own_hits ? 4 * chunk : 0, off_rad = off_E + (own_E ? 3 * chunk : 0),
                   off_V = off_rad + (own_rad ? 3 * chunk : 0), hits_words = off_V + (own_V ? chunk : 0);
    // every buffer a launch below writes, grown to a chunk / a sub-chunk and guarded
    if ((rc = grow_checked("rays, rows, list", &c->d_rays, &c->rays_cap, rays_words)) != ZRT_OK) return rc;
    if (hits_words && (rc = grow_checked("hits, irradiance", &c->d_hits, &c->hits_cap, hits_words)) != ZRT_OK) return rc;
    if (park_first && (rc = grow_park_buffers(ps, chunk, 0, chunk, wfc_words(0))) != ZRT_OK) return rc;
    if ((rc = event_pool(c->ev_trace, 2)) != ZRT_OK) return rc;

    RayLaunch rl;                                  // the first hits: a trace call's
    if ((rc = ray_launch(c, pl, counting, park_first, rl, -1)) != ZRT_OK) return rc;
    TransmitLaunch tl;                             // the chains: a transmittance call's lane kernels
    if ((rc = transmit_launch(c, pl, counting, !k.unshadowed && k.any, tl)) != ZRT_OK) return rc;

    QueryParams R;
    memset(&R, 0, sizeof R);
    query_params(c, R);
    if (park_first) query_park_params(c, pl, ps, R);
    D.tri_data = c->d_data;
    D.mats = c->d_mats;
    D.texels = c->d_texels;
    D.unshadowed = k.unshadowed ? 1u : 0u;
    D.irays = c->d_rays + off_list;
    D.ibound = D.irays + 6 * M;
    float* const dT = D.ibound + M;
    D.T = dT;
    D.slot = reinterpret_cast<uint32_t*>(dT + (1 + k.extra_rows) * M);
    D.ctr = c->d_counter;
    D.stats = c->d_stats;
    light_rows(D, c->d_rays + off_rows, dT + M);
    // the chains' walks: the list as a transmittance call's rays and bounds
    TransmitParams I;
    memset(&I, 0, sizeof I);
    query_params(c, I.q);
    I.q.rays = D.irays;
    I.q.t_max = D.ibound;
    I.T = dT;
    I.max_cross = k.max_crossings;

    HIP_TRY(hipMemsetAsync(c->d_stats, 0, 512, c->stream));
    HIP_TRY(hipEventRecord(c->ev_begin, c->stream));
    if (k.head)
        HIP_TRY(hipMemcpyAsync(c->d_rays + off_rows, k.head, 4 * k.head_words, hipMemcpyHostToDevice, c->stream));
    uint32_t launches = 0;
    uint64_t traced = 0;
    for (uint64_t off = 0; off < k.num_rays; off += chunk) {
        const uint32_t n = (uint32_t)std::min<uint64_t>(chunk, k.num_rays - off);
        if (dev) {
            R.rays = k.rays + 6 * off;
        } else {
            if ((rc = stage_chunk(c, k.rays + 6 * off, nullptr, chunk, n)) != ZRT_OK) return rc;
            R.rays = c->d_rays;
        }
        R.hits = own_hits ? c->d_hits : reinterpret_cast<uint32_t*>(k.hits + off);
        D.E = own_E ? reinterpret_cast<float*>(c->d_hits + off_E) : k.irradiance + 3 * off;
        D.radiance = own_rad ? reinterpret_cast<float*>(c->d_hits + off_rad) : dev && k.radiance ? k.radiance + 3 * off
                                                                                                 : nullptr;
        float* const dV = own_V ? reinterpret_cast<float*>(c->d_hits + off_V) : k.visibility ? k.visibility + off : nullptr;
        light_vis(D, dV);
        HIP_TRY(hipMemsetAsync(c->d_counter, 0, 64, c->stream));
        if (park_first) HIP_TRY(hipMemsetAsync(ps.wfc, 0, 4ull * 16 * kCtr, c->stream));
        if ((rc = trace_first_segments(c, pl, rl, R, n, true, &launches)) != ZRT_OK) return rc;
        // the first hits' segments and hits are not the chains'
        HIP_TRY(hipMemsetAsync(c->d_stats, 0, 8, c->stream));
        HIP_TRY(hipMemsetAsync(c->d_stats + 3, 0, 8, c->stream));
        D.rays = R.rays;
        D.hits = R.hits;
        D.n = n;
        light_key(D, k.index_base + off);
        const uint64_t items = (uint64_t)n * per;
        for (uint64_t i0 = 0; i0 < items; i0 += kDirItems) {
            const uint32_t m = (uint32_t)std::min<uint64_t>(kDirItems, items - i0);
            D.ray0 = (uint32_t)(i0 / per);
            D.s0 = (uint32_t)(i0 % per);
            D.m = m;
            HIP_TRY(hipMemsetAsync(c->d_counter, 0, 64, c->stream));
            if ((rc = gen(D, c->stream)) != ZRT_OK) return rc;
            ++launches;
            uint32_t live = 0;                         // the list's entries: the traced items
            HIP_TRY(copy_sync(&live, c->d_counter + 4, sizeof live, hipMemcpyDeviceToHost, c->stream));
            if (live > m) return ZRT_ERR_HIP;          // (never: the kernel's own bounds)
            traced += live;
            D.fold = 0u;
            if (live != 0u && !k.unshadowed) {
                transmit_chains(c, pl, tl, I, live, &launches);
                D.fold = 1u;
            }
            const uint32_t nr = (uint32_t)((D.s0 + (uint64_t)m + per - 1) / per);   // rays with an item in the sub-chunk
            if ((rc = reduce(D, nr, c->stream)) != ZRT_OK) return rc;
            ++launches;
        }
        if (!dev) {
            HIP_TRY(hipEventRecord(c->ev_trace[1], c->stream));
            if (k.hits) HIP_TRY(copy_sync(k.hits + off, c->d_hits, 16ull * n, hipMemcpyDeviceToHost, c->stream));
            if (k.irradiance) HIP_TRY(copy_sync(k.irradiance + 3 * off, D.E, 12ull * n, hipMemcpyDeviceToHost, c->stream));
            if (k.radiance) HIP_TRY(copy_sync(k.radiance + 3 * off, D.radiance, 12ull * n, hipMemcpyDeviceToHost, c->stream));
            if (k.visibility) HIP_TRY(copy_sync(k.visibility + off, dV, 4ull * n, hipMemcpyDeviceToHost, c->stream));
            if ((rc = chunk_kernel_time(c, st)) != ZRT_OK) return rc;
        }
    }
    unsigned long long hs[kDirStat + 2];
    if ((rc = query_stats(c, dev, launches, counting, hs, kDirStat + 2, st)) != ZRT_OK) return rc;
    st.segments = k.num_rays + hs[kDirStat];
    st.samples = traced;
    st.hits = hs[kDirStat + 1];
    if (stats) *stats = st;
    return ZRT_OK;
}

// Direct light of punctual lights at each ray's first hit: see include/zrt.h,
// the kernels' comment (DirectParams) and DESIGN 5.18.  light_items with a
// (ray, light) item: the lights, uploaded once, lie behind a host batch's rays,
// the items' factors in a row of their own between T and the slots; the gen
// and reduce launches are direct_gen_kernel and direct_reduce_kernel.
static int direct_gen_launch(const DirectParams& D, hipStream_t stream) {
    const uint32_t mblk = (D.m + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(direct_gen_kernel, dim3((mblk + kDirGenItems - 1) / kDirGenItems), dim3(kBlock), 0, stream, D);
    HIP_TRY(hipGetLastError());
    return ZRT_OK;
}
static int direct_reduce_launch(const DirectParams& D, uint32_t rays, hipStream_t stream) {
    hipLaunchKernelGGL(direct_reduce_kernel, dim3((rays + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, D);
    HIP_TRY(hipGetLastError());
    return ZRT_OK;
}
static_assert(sizeof(zrt_light) == 48, "light_items counts a light as 12 words");
extern "C" int zrt_context_direct(zrt_context* c, const zrt_direct_batch* b, zrt_stats* stats) {
    if (!c || !direct_batch_ok(b, kTraceFlags)) return ZRT_ERR_INVALID_ARG;
    if (b->num_rays == 0) { if (stats) *stats = zrt_stats{}; return ZRT_OK; }
    DeviceGuard g(c->device);
    const bool unshadowed = (b->flags & ZRT_DIRECT_UNSHADOWED) != 0;
    const LightCall k{b->num_rays, b->rays, b->hits, b->irradiance, b->radiance, b->on_device != 0,
                      b->flags & ~ZRT_DIRECT_UNSHADOWED, unshadowed, true, b->num_lights, b->max_crossings, 0, b->lights,
                      12ull * b->num_lights, 0, 1, false, nullptr};
    DirectParams D;
    memset(&D, 0, sizeof D);
    D.L = b->num_lights;
    return light_items(c, k, D, direct_gen_launch, direct_reduce_launch, stats);
}

// zrt_context_area_lights (include/zrt.h): next-event estimation over an
// emitter set; the (ray, sample) items, the set and the two item kernels are
// emitters.hip's (emitters.h).  light_items with the lights' row
// replaced by the set, which lives in memory of its own, and the factors' row
// by the items' contributions, a float4 each, behind a host batch's rays.
static_assert((ZRT_AREA_UNSHADOWED & (kTraceFlags | ZRT_RADIANCE_PER_SAMPLE | ZRT_SEGMENT_ANY | ZRT_DIRECT_UNSHADOWED |
                                      ZRT_DENOISE_ROW_MAJOR | ZRT_REPROJECT_ROW_MAJOR | ZRT_SVGF_ROW_MAJOR | 0xFFFFu)) == 0u,
              "a bit of its own");
static_assert(sizeof(zrt_emitter) == 80 && sizeof(zrt_area_light_batch) == 80, "include/zrt.h");
extern "C" int zrt_context_area_lights(zrt_context* c, const zrt_area_light_batch* b, zrt_stats* stats) {
    if (!c || !area_light_batch_ok(c, b, kTraceFlags)) return ZRT_ERR_INVALID_ARG;
    if (b->num_rays == 0) { if (stats) *stats = zrt_stats{}; return ZRT_OK; }
    DeviceGuard g(c->device);
    const zrt_emitters* const es = b->emitters;
    const bool unshadowed = (b->flags & ZRT_AREA_UNSHADOWED) != 0;
    const LightCall k{b->num_rays, b->rays, b->hits, b->irradiance, b->radiance, b->on_device != 0,
                      b->flags & ~ZRT_AREA_UNSHADOWED, unshadowed, es->count != 0u, b->num_samples, b->max_crossings,
                      b->index_base, nullptr, 0, 4, 0, false, nullptr};
    AreaParams D;
    memset(&D, 0, sizeof D);
    D.rec = reinterpret_cast<const float4*>(es->d_rec);
    D.C = es->d_C;
    D.Q = es->Q;
    D.Qf = (float)es->Q;
    D.count = es->count;
    while ((1ull << D.steps) <= es->count) ++D.steps;
    D.seed = b->seed;
    D.S = b->num_samples;
    return light_items(c, k, D, area_gen_launch, area_reduce_launch, stats);
}

// zrt_context_sky_light (include/zrt.h): the sky's light over the cosine-
// weighted hemisphere at each first hit; the (ray, sample) items and the two
// item kernels are sky.hip's (emitters.h).  light_items with no
// row of the call's own -- the reduce reads the direction's y off the list --
// and the per-ray visibility beside the irradiance.
static_assert((ZRT_SKY_UNSHADOWED & (kTraceFlags | ZRT_RADIANCE_PER_SAMPLE | ZRT_SEGMENT_ANY | ZRT_DIRECT_UNSHADOWED |
                                     ZRT_AREA_UNSHADOWED | ZRT_DENOISE_ROW_MAJOR | ZRT_REPROJECT_ROW_MAJOR |
                                     ZRT_SVGF_ROW_MAJOR | 0xFFFFu)) == 0u,
              "a bit of its own");
static_assert(sizeof(zrt_sky_light_batch) == 80, "include/zrt.h");
extern "C" int zrt_context_sky_light(zrt_context* c, const zrt_sky_light_batch* b, zrt_stats* stats) {
    if (!c || !sky_light_batch_ok(b, kTraceFlags)) return ZRT_ERR_INVALID_ARG;
    if (b->num_rays == 0) { if (stats) *stats = zrt_stats{}; return ZRT_OK; }
    DeviceGuard g(c->device);
    const bool unshadowed = (b->flags & ZRT_SKY_UNSHADOWED) != 0;
    const LightCall k{b->num_rays, b->rays, b->hits, b->irradiance, b->radiance, b->on_device != 0,
                      b->flags & ~ZRT_SKY_UNSHADOWED, unshadowed, true, b->num_samples, b->max_crossings, b->index_base,
                      nullptr, 0, 0, 0, true, b->visibility};
    SkyParams D;
    memset(&D, 0, sizeof D);
    D.zig = c->d_zig;
    D.seed = b->seed;
    D.S = b->num_samples;
    return light_items(c, k, D, sky_gen_launch, sky_reduce_launch, stats);
}

// What zrt_context_radiance and zrt_context_light_probes settle alike before
// their chunk loops (rad_plan) and launch alike per chunk (rad_chunk_first,
// rad_chunk_rest): the plan, the chunk size, pass set 0's buffers, the grids
// and the launch parameters of a call of S samples per ray and max_bounce mb.
struct RadCall {
    uint32_t S, mb, nb;
    bool per_sample, park_first, park_next, park_any;
    LaunchPlan pl;
    BounceGrids grids;
    RayLaunch rl;
    RadFn f_fan;
    uint32_t grid_fan;
    uint64_t chunk;           // rays per chunk
    float inv_spp;
    RadParams R;
};

// `stage_per_ray`: the bytes per ray of a chunk the caller stages beyond the
// radiance launches' own; `stage_held`: the bytes of grow-only buffers it
// stages them in (device_budget's `held`).  The caller grows those after this
// returns: the budget is read before any buffer grows.
static int rad_plan(zrt_context* c, uint32_t flags, uint64_t num_rays, uint32_t S, uint32_t mb, uint64_t seed,
                    uint64_t stage_per_ray, size_t stage_held, RadCall& k) {
    const uint32_t nb = std::max<uint32_t>(mb, 1);
    k.S = S;
    k.mb = mb;
    k.nb = nb;
    k.per_sample = (flags & ZRT_RADIANCE_PER_SAMPLE) != 0;
    const bool per_sample = k.per_sample;
    const uint64_t first_n = per_sample ? num_rays * S : num_rays;
    const bool want_first = (flags & ZRT_TRACE_PARK) || first_n >= kTraceParkMin;
    LaunchPlan& pl = k.pl;
    int rc;
    if ((rc = resolve_plan(c, flags, false, want_first || nb > 1, num_rays * S >= kSetsMinSamples, pl)) != ZRT_OK)
        return rc;
    k.park_next = pl.park_ok;
    k.park_first = pl.park_ok && want_first;
    k.park_any = pl.park;
    const bool lmats = c->nmat <= kLdsMats;
    k.f_fan = nb == 1 ? (lmats ? (RadFn)rad_fanout_kernel<true, true> : (RadFn)rad_fanout_kernel<false, true>)
                      : (lmats ? (RadFn)rad_fanout_kernel<true, false> : (RadFn)rad_fanout_kernel<false, false>);

    // chunk size: at most kTraceChunk rays, its n * S items below 2^31 and
    // within the memory budget of a render's pass (its per-item bytes,
    // device_budget); S <= 65535 always fits at 64 rays
    zrt_context::PassSet& ps = c->set[0];
    const uint64_t per_item = 96ull + 16ull + 16ull + 32ull * nb;
    const uint64_t per_ray = per_item * S + 24ull + 15ull + stage_per_ray;
    const size_t held = stage_held + 4ull * (c->nrays_cap + c->lin_cap) + c->rgb_cap + c->bfc_bytes + c->esc_extra + held_bytes(ps);
    const size_t budget = device_budget(c, held);
    uint64_t chunk = std::min<uint64_t>(kTraceChunk, 0x7FFFFF00ull / S);
    chunk = std::max<uint64_t>(64, std::min<uint64_t>(chunk, budget / per_ray));
    chunk = std::min<uint64_t>(chunk, num_rays);
    k.chunk = chunk;
    const uint64_t T = chunk * S;                  // items of the largest chunk
    const uint64_t hit_need = std::max<uint64_t>(k.park_any ? T : 0, per_sample ? 0 : chunk);
    if (!per_sample && (rc = grow(&c->d_nrays, &c->nrays_cap, 6 * chunk)) != ZRT_OK) return rc;
    if ((rc = grow(&c->d_lin, &c->lin_cap, 3 * chunk)) != ZRT_OK) return rc;
    if ((rc = grow(&c->d_rgb, &c->rgb_cap, 3 * chunk)) != ZRT_OK) return rc;
    if ((rc = grow_pass_set(ps, T, nb, mb, hit_need)) != ZRT_OK) return rc;
    // capacity guard of the rest: every buffer a launch below writes holds
    // what a chunk's launches write; a chunk's items fit 31 bits
    if ((!per_sample && shortfall("unit rays", c->d_nrays, c->nrays_cap, 6 * chunk)) ||
        shortfall("linear", c->d_lin, c->lin_cap, 3 * chunk) || shortfall("rgb", c->d_rgb, c->rgb_cap, 3 * chunk) ||
        chunk == 0 || chunk > kTraceChunk || T > 0x7FFFFF00ull)
        return ZRT_ERR_INVALID_ARG;
    if ((rc = event_pool(c->ev_trace, 2)) != ZRT_OK) return rc;

    // occupancy-sized persistent grids
    if ((rc = bounce_grids(c, pl, k.park_any, (!k.park_next && nb > 1) || (per_sample && !k.park_first), k.grids)) !=
        ZRT_OK)
        return rc;
    k.rl = RayLaunch{};
    k.grid_fan = 0;
    if (!per_sample) {
        if ((rc = ray_launch(c, pl, false, k.park_first, k.rl)) != ZRT_OK) return rc;
        if ((rc = resident_blocks(c, (const void*)k.f_fan, kTraceThreads, pl.lds_shade, &k.grid_fan)) != ZRT_OK)
            return rc;
    }

    RadParams& R = k.R;
    memset(&R, 0, sizeof R);
    WfParams& W = R.w;
    scene_params(c, W.t);
    W.t.max_bounce = mb;
    W.t.seed = seed;
    W.t.counter = c->d_counter;
    W.t.stats = c->d_stats;
    W.stk4 = ps.stk4;
    W.stk2 = ps.stk2;
    W.term = ps.term;
    W.hit = ps.hit;
    park_params(c, pl, W);
    R.ctr = c->d_counter;
    R.nrays = c->d_nrays;
    R.q = ps.q1;                                   // launch 0 reads q1 (bounce_params)
    R.n_in8 = region_counts(ps, 0);
    // stage3.zig:223 inv_num_samples = ones / splat(spp)  (f32 division)
    k.inv_spp = 1.0f / (float)S;
    return ZRT_OK;
}

// A chunk of n rays (on the device, 6 floats each) up to the paths entering
// launch 1: the pack kernel, the shared first segments (their records in
// ps.hit[ray] until launch 1 reuses the array) and the fan-out; with
// ZRT_RADIANCE_PER_SAMPLE the per-sample pack kernel alone.
static int rad_chunk_first(zrt_context* c, RadCall& k, const float* rays, uint32_t n, uint32_t key0, uint32_t* launches) {
    zrt_context::PassSet& ps = c->set[0];
    RadParams& R = k.R;
    WfParams& W = R.w;
    const uint32_t items = n * k.S;                // <= T < 2^31
    int rc;
    R.rays = rays;
    R.n = n;
    R.key0 = key0;
    // the counters of every launch (wfc_words); the pack kernels write launch 0's region counts
    HIP_TRY(hipMemsetAsync(ps.wfc, 0, 4ull * wfc_words(k.mb), c->stream));
    HIP_TRY(hipMemsetAsync(c->d_counter, 0, 64, c->stream));
    W.t.P = n;
    W.t.S = k.S;
    W.t.total = items;
    W.t.sdiv = div_magic(k.S);
    W.T = items;
    bounce_params(W, ps, 0, k.mb);
    if (k.per_sample) {
        hipLaunchKernelGGL(rad_pack_samples_kernel, dim3((items + kBlock - 1) / kBlock), dim3(kBlock), 0, c->stream, R);
        ++*launches;
        HIP_TRY(hipGetLastError());
        return ZRT_OK;
    }
    hipLaunchKernelGGL(rad_pack_kernel, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, c->stream, R);
    ++*launches;
    // the first segments: one per ray, launch 0's queue as the identity queue
    QueryParams Q;
    memset(&Q, 0, sizeof Q);
    Q.w = W;
    Q.w.t.max_bounce = 1;
    Q.rays = c->d_nrays;
    Q.hits = reinterpret_cast<uint32_t*>(ps.hit);
    Q.ctr = c->d_counter;
    if ((rc = trace_first_segments(c, k.pl, k.rl, Q, n, false, launches)) != ZRT_OK) return rc;
    // the fan-out: items fetched like a primary launch's, on launch 0's
    // shade counter, appended to launch 1's queue
    W.fetch8 = W.fetch8s;
    hipLaunchKernelGGL(k.f_fan, dim3(k.grid_fan), dim3(kTraceThreads), k.pl.lds_shade, c->stream, R);
    ++*launches;
    HIP_TRY(hipGetLastError());
    return ZRT_OK;
}

// The rest of the chunk: launch k as a render runs a bounce launch (launch 0
// of the per-sample records by the first segment's rule), then
// wf_resolve_kernel (P = n, one pass) into d_lin / d_rgb.
static int rad_chunk_rest(zrt_context* c, RadCall& k, uint32_t n, uint32_t* launches) {
    zrt_context::PassSet& ps = c->set[0];
    WfParams& W = k.R.w;
    const uint32_t items = n * k.S;
    int rc;
    for (uint32_t i = k.per_sample ? 0u : 1u; i < k.nb; ++i) {
        const bool park = i == 0 ? k.park_first : k.park_next;
        bounce_params(W, ps, i, k.mb);
        if ((rc = launch_bounce(k.pl, k.grids, W, c->stream, park, i + 1 == k.nb, nullptr)) != ZRT_OK) return rc;
        *launches += park ? 2 : 1;
    }
    hipLaunchKernelGGL(wf_resolve_kernel, dim3((n + kResPix - 1) / kResPix), dim3(kBlock), 0, c->stream, ps.term,
                       ps.stk4, ps.stk2, items, n, k.S, k.mb, c->d_acc, 1, 1, k.inv_spp, c->d_rgb, c->d_lin);
    ++*launches;
    HIP_TRY(hipGetLastError());
    return ZRT_OK;
}

// Scene.traceRayRecursive (stage3.zig:188-220) for a batch of rays: see
// include/zrt.h, the kernels' comment (RadParams) and DESIGN 5.12.  The launch
// plan is the one a render resolves (resolve_plan); the first segment takes
// the park kernel by zrt_context_trace's rule, on the segments launch 0 traces
// (n rays, or n * S with ZRT_RADIANCE_PER_SAMPLE).  Per chunk of n rays, S
// samples each, all on the context's stream and pass set 0:
//   shared first segment (default):
//     rad_pack_kernel -> the chunk's first segments as zrt_context_trace traces
//     them (trace_first_segments: wf_park_kernel over the identity queue, or
//     query_walk_kernel; then the kRaysRest launch) -> rad_fanout_kernel: n * S
//     shaded continuations;
//   ZRT_RADIANCE_PER_SAMPLE:
//     rad_pack_samples_kernel -> launch 0 as a bounce launch over n * S records;
//   then bounces 1 .. max_bounce - 1 as a render launches them (launch_bounce)
//   and wf_resolve_kernel (P = n, one pass), d_lin / d_rgb copied to the outputs.
extern "C" int zrt_context_radiance(zrt_context* c, const zrt_radiance_batch* b, zrt_stats* stats) {
    if (!c || !b) return ZRT_ERR_INVALID_ARG;
    if ((b->flags & ~kRadianceFlags) != 0u || b->on_device > 1u) return ZRT_ERR_INVALID_ARG;
    if (b->num_samples == 0 || b->num_samples > 65535) return ZRT_ERR_INVALID_ARG;
    // the scatter mask holds one bit per bounce slot, the queue 16 bits of depth
    if (b->max_bounce > 32) return ZRT_ERR_UNSUPPORTED;
    zrt_stats st{};
    if (b->num_rays == 0) { if (stats) *stats = st; return ZRT_OK; }
    if (!b->rays || !b->radiance) return ZRT_ERR_INVALID_ARG;
    DeviceGuard g(c->device);

    const uint32_t S = b->num_samples, mb = b->max_bounce;
    st.samples = b->num_rays * S;
    if (mb == 0) {
        // traceRayRecursive at depth 0 returns 0: the sum of S zeros times 1 / S, and toRGB(0) = 0
        if (b->on_device) {
            HIP_TRY(hipMemsetAsync(b->radiance, 0, 12ull * b->num_rays, c->stream));
            if (b->rgb) HIP_TRY(hipMemsetAsync(b->rgb, 0, 3ull * b->num_rays, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
        } else {
            memset(b->radiance, 0, 12ull * b->num_rays);
            if (b->rgb) memset(b->rgb, 0, 3ull * b->num_rays);
        }
        if (stats) *stats = st;
        return ZRT_OK;
    }

    RadCall k;
    int rc;
    if ((rc = rad_plan(c, b->flags, b->num_rays, S, mb, b->seed, b->on_device ? 0ull : 24ull, 4ull * c->rays_cap, k)) !=
        ZRT_OK)
        return rc;
    const uint64_t chunk = k.chunk;
    if (!b->on_device) {
        if ((rc = grow(&c->d_rays, &c->rays_cap, 6 * chunk)) != ZRT_OK) return rc;
        if (shortfall("rays", c->d_rays, c->rays_cap, 6 * chunk)) return ZRT_ERR_INVALID_ARG;
    }

    HIP_TRY(hipMemsetAsync(c->d_stats, 0, 512, c->stream));
    HIP_TRY(hipEventRecord(c->ev_begin, c->stream));
    uint32_t launches = 0;
    for (uint64_t off = 0; off < b->num_rays; off += chunk) {
        const uint32_t n = (uint32_t)std::min<uint64_t>(chunk, b->num_rays - off);
        const float* rays = b->rays + 6 * off;
        if (!b->on_device) {
            HIP_TRY(hipMemcpyAsync(c->d_rays, b->rays + 6 * off, 24ull * n, hipMemcpyHostToDevice, c->stream));
            rays = c->d_rays;
            HIP_TRY(hipEventRecord(c->ev_trace[0], c->stream));
        }
        if ((rc = rad_chunk_first(c, k, rays, n, (uint32_t)(b->index_base + off), &launches)) != ZRT_OK) return rc;
        if ((rc = rad_chunk_rest(c, k, n, &launches)) != ZRT_OK) return rc;
        if (b->on_device) {
            HIP_TRY(hipMemcpyAsync(b->radiance + 3 * off, c->d_lin, 12ull * n, hipMemcpyDeviceToDevice, c->stream));
            if (b->rgb)
                HIP_TRY(hipMemcpyAsync(b->rgb + 3 * off, c->d_rgb, 3ull * n, hipMemcpyDeviceToDevice, c->stream));
        } else {
            HIP_TRY(hipEventRecord(c->ev_trace[1], c->stream));
            HIP_TRY(copy_sync(b->radiance + 3 * off, c->d_lin, 12ull * n, hipMemcpyDeviceToHost, c->stream));
            if (b->rgb) HIP_TRY(copy_sync(b->rgb + 3 * off, c->d_rgb, 3ull * n, hipMemcpyDeviceToHost, c->stream));
            float t = 0.0f;
            HIP_TRY(hipEventElapsedTime(&t, c->ev_trace[0], c->ev_trace[1]));
            st.trace_kernel_ms += t;
        }
    }
    if ((rc = finish_query(c, b->on_device != 0, launches, st)) != ZRT_OK) return rc;
    unsigned long long hs[1];
    HIP_TRY(copy_sync(hs, c->d_stats, sizeof hs, hipMemcpyDeviceToHost, c->stream));
    // the reference traces a shared first segment once per sample
    st.segments = hs[0] + (k.per_sample ? 0ull : b->num_rays * (uint64_t)(S - 1));
    if (stats) *stats = st;
    return ZRT_OK;
}

// Light probes: see include/zrt.h, the kernels' comment (LightProbeParams) and
// DESIGN 5.19.  The N * D (probe, direction) items are a radiance call's rays,
// made on the device; per chunk of n items, all on the context's stream and
// pass set 0:
//   light_probe_gen_kernel -> the chunk's ray row in d_rays;
//   rad_chunk_first (rad_pack_kernel, the first segments, rad_fanout_kernel);
//   light_probe_reduce_kernel, kLpTake: t of the first hits, before launch 1
//   reuses their records;
//   rad_chunk_rest (the bounce launches, wf_resolve_kernel);
//   light_probe_reduce_kernel, kLpFold: the chunk's items into the sums of its
//   probes; the probes that end in the chunk are stored.
// d_rays holds the ray row and a host batch's positions of the chunk's probes;
// d_hits the t row, the two carry rows and a host batch's output rows (sh, distance,
// hits of the chunk's probes, the directions of its items); a device batch's
// outputs are written in place.  Each use writes what it reads first.
extern "C" int zrt_context_light_probes(zrt_context* c, const zrt_light_probe_batch* b, zrt_stats* stats) {
    if (!c || !light_probe_batch_ok(b, kRadianceFlags & ~ZRT_RADIANCE_PER_SAMPLE)) return ZRT_ERR_INVALID_ARG;
    // the scatter mask holds one bit per bounce slot, the queue 16 bits of depth
    if (b->max_bounce > 32) return ZRT_ERR_UNSUPPORTED;
    zrt_stats st{};
    if (b->num_probes == 0) { if (stats) *stats = st; return ZRT_OK; }
    DeviceGuard g(c->device);

    const uint32_t D = b->num_directions, S = b->num_samples, mb = b->max_bounce;
    const uint64_t N = b->num_probes, total = N * D;
    const bool dev = b->on_device != 0;
    st.samples = total * S;
    // bytes per item beyond a device radiance call's: the ray row and t; a host
    // batch's directions; with D = 1 an item is a probe: its position and rows
    const uint64_t stage = 24ull + 4ull + (dev ? 0ull : 12ull + (12ull + 120ull + D - 1) / D);
    RadCall k;
    int rc;
    if ((rc = rad_plan(c, b->flags, total, S, mb, b->seed, stage, 4ull * (c->rays_cap + c->hits_cap), k)) != ZRT_OK)
        return rc;
    const uint64_t chunk = k.chunk;
    const uint64_t npmax = std::min<uint64_t>(N, (chunk + D - 1) / D + 1);   // probes with an item in one chunk
    // words of d_rays: the ray row, a host batch's positions
    const uint64_t off_pos = 6 * chunk, rays_words = off_pos + (dev ? 0 : 3 * npmax);
    // words of d_hits: t, the two carry rows, a host batch's sh, distance, hits and directions
    const uint64_t off_carry = chunk, off_sh = off_carry + 64, off_dist = off_sh + (!dev && b->sh ? 27 * npmax : 0),
                   off_hits = off_dist + (!dev && b->distance ? 2 * npmax : 0),
                   off_dirs = off_hits + (!dev && b->hits ? npmax : 0),
                   hits_words = off_dirs + (!dev && b->directions ? 3 * chunk : 0);
    if ((rc = grow(&c->d_rays, &c->rays_cap, rays_words)) != ZRT_OK) return rc;
    if ((rc = grow(&c->d_hits, &c->hits_cap, hits_words)) != ZRT_OK) return rc;
    // capacity guard: every buffer a launch below writes holds a chunk
    if (shortfall("rays, positions", c->d_rays, c->rays_cap, rays_words) ||
        shortfall("t, carry, rows", c->d_hits, c->hits_cap, hits_words))
        return ZRT_ERR_INVALID_ARG;

    LightProbeParams P;
    memset(&P, 0, sizeof P);
    P.rays = c->d_rays;
    P.zig = c->d_zig;
    P.seed = b->seed;
    P.D = D;
    P.hit = c->set[0].hit;
    P.t = reinterpret_cast<float*>(c->d_hits);
    P.lin = c->d_lin;
    P.stats = c->d_stats;
    float* const s_pos = c->d_rays + off_pos;
    float* const s_sh = reinterpret_cast<float*>(c->d_hits + off_sh);
    float* const s_dist = reinterpret_cast<float*>(c->d_hits + off_dist);
    uint32_t* const s_hits = c->d_hits + off_hits;
    float* const s_dirs = reinterpret_cast<float*>(c->d_hits + off_dirs);

    HIP_TRY(hipMemsetAsync(c->d_stats, 0, 512, c->stream));
    HIP_TRY(hipEventRecord(c->ev_begin, c->stream));
    uint32_t launches = 0, parity = 0;
    for (uint64_t off = 0; off < total; off += chunk) {
        const uint32_t n = (uint32_t)std::min<uint64_t>(chunk, total - off);
        const uint64_t p0 = off / D, p1 = (off + n - 1) / D;
        const uint32_t np = (uint32_t)(p1 - p0 + 1);                  // <= npmax
        const uint32_t done = np - ((p1 + 1) * D <= off + n ? 0u : 1u);   // probes p0 .. that end in this chunk
        if (np > npmax) return ZRT_ERR_INVALID_ARG;                   // (never)
        if (dev) {
            P.pos = b->positions + 3 * p0;
            P.dirs = b->directions ? b->directions + 3 * off : nullptr;
            P.sh = b->sh ? b->sh + 27 * p0 : nullptr;
            P.dist = b->distance ? b->distance + 2 * p0 : nullptr;
            P.hits = b->hits ? b->hits + p0 : nullptr;
        } else {
            HIP_TRY(hipMemcpyAsync(s_pos, b->positions + 3 * p0, 12ull * np, hipMemcpyHostToDevice, c->stream));
            HIP_TRY(hipEventRecord(c->ev_trace[0], c->stream));
            P.pos = s_pos;
            P.dirs = b->directions ? s_dirs : nullptr;
            P.sh = b->sh ? s_sh : nullptr;
            P.dist = b->distance ? s_dist : nullptr;
            P.hits = b->hits ? s_hits : nullptr;
        }
        P.key0 = (uint32_t)(b->index_base + off);
        P.j0 = (uint32_t)(off - p0 * D);
        P.n = n;
        P.np = np;
        // the carry rows alternate: the fold's first probe reads what the previous chunk's last one left,
        // its last probe writes the other row -- two half-waves of one launch, in no order
        P.carry_in = reinterpret_cast<const float*>(c->d_hits + off_carry + 32 * (parity ^ 1u));
        P.carry_out = reinterpret_cast<float*>(c->d_hits + off_carry + 32 * parity);
        parity ^= 1u;
        const uint32_t nblk = (n + kBlock - 1) / kBlock;
        hipLaunchKernelGGL(light_probe_gen_kernel, dim3((nblk + kLpGenItems - 1) / kLpGenItems), dim3(kBlock), 0, c->stream,
                           P);
        ++launches;
        HIP_TRY(hipGetLastError());
        if ((rc = rad_chunk_first(c, k, c->d_rays, n, P.key0, &launches)) != ZRT_OK) return rc;
        P.mode = kLpTake;
        hipLaunchKernelGGL(light_probe_reduce_kernel, dim3((nblk + kLpTakeItems - 1) / kLpTakeItems), dim3(kBlock), 0,
                           c->stream, P);
        ++launches;
        HIP_TRY(hipGetLastError());
        if ((rc = rad_chunk_rest(c, k, n, &launches)) != ZRT_OK) return rc;
        P.mode = kLpFold;
        hipLaunchKernelGGL(light_probe_reduce_kernel, dim3((32u * np + kBlock - 1) / kBlock), dim3(kBlock), 0, c->stream, P);
        ++launches;
        HIP_TRY(hipGetLastError());
        if (dev) {
            if (b->radiance)
                HIP_TRY(hipMemcpyAsync(b->radiance + 3 * off, c->d_lin, 12ull * n, hipMemcpyDeviceToDevice, c->stream));
        } else {
            HIP_TRY(hipEventRecord(c->ev_trace[1], c->stream));
            if (b->radiance) HIP_TRY(copy_sync(b->radiance + 3 * off, c->d_lin, 12ull * n, hipMemcpyDeviceToHost, c->stream));
            if (b->directions)
                HIP_TRY(copy_sync(b->directions + 3 * off, s_dirs, 12ull * n, hipMemcpyDeviceToHost, c->stream));
            if (done != 0u) {
                if (b->sh) HIP_TRY(copy_sync(b->sh + 27 * p0, s_sh, 108ull * done, hipMemcpyDeviceToHost, c->stream));
                if (b->distance)
                    HIP_TRY(copy_sync(b->distance + 2 * p0, s_dist, 8ull * done, hipMemcpyDeviceToHost, c->stream));
                if (b->hits) HIP_TRY(copy_sync(b->hits + p0, s_hits, 4ull * done, hipMemcpyDeviceToHost, c->stream));
            }
            HIP_TRY(hipStreamSynchronize(c->stream));   // (a chunk that copied nothing back: the events)
            float t = 0.0f;
            HIP_TRY(hipEventElapsedTime(&t, c->ev_trace[0], c->ev_trace[1]));
            st.trace_kernel_ms += t;
        }
    }
    if ((rc = finish_query(c, dev, launches, st)) != ZRT_OK) return rc;
    unsigned long long hs[kLpStat + 1];
    HIP_TRY(copy_sync(hs, c->d_stats, sizeof hs, hipMemcpyDeviceToHost, c->stream));
    // the reference traces a shared first segment once per sample
    st.segments = hs[0] + total * (uint64_t)(S - 1);
    st.hits = hs[kLpStat];
    if (stats) *stats = st;
    return ZRT_OK;
}

extern "C" int zrt_render(const zrt_scene* scene, const zrt_camera* cam, const zrt_render_config* cfg,
                          uint8_t* rgb_out, zrt_stats* stats) {
    if (!scene || !cam || !cfg || !rgb_out) return ZRT_ERR_INVALID_ARG;
    if (cfg->num_devices > 1) {                // the image's tiles over a device list (group.hip)
        if (!cfg->devices) return ZRT_ERR_INVALID_ARG;
        zrt_group* g = nullptr;
        int rc = zrt_group_create(scene, cfg->devices, cfg->num_devices, &g);
        if (rc != ZRT_OK) return rc;
        zrt_render_config whole = *cfg;
        whole.rank = 0;
        whole.num_ranks = 1;
        rc = zrt_group_render(g, cam, &whole, rgb_out, stats);
        zrt_group_destroy(g);
        return rc;
    }
    // a one-entry list names the device; a null list keeps
    // cfg->device, as ABI-1 callers that set num_devices = 1 for "one device"
    // expect
    const int32_t dev = cfg->num_devices == 1 && cfg->devices ? cfg->devices[0] : cfg->device;
    zrt_context* c = nullptr;
    int rc = zrt_context_create(scene, dev, &c);
    if (rc != ZRT_OK) return rc;
    zrt_render_config one = *cfg;
    one.rank = 0;
    one.num_ranks = 1;
    zrt_outputs o{};
    o.rgb_image = rgb_out;
    rc = zrt_context_render(c, cam, &one, &o, stats);
    zrt_context_destroy(c);
    return rc;
}
