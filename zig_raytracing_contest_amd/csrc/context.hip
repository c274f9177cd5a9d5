// context.hip -- everything that builds, describes or destroys a zrt_context,
// with the build-time kernels only this code launches (a kernel lives in the
// translation unit that launches it), and the device warm-up.
#include <ctime>
#include <new>

#include "render_context.h"
#include "escape.h"
#include "device_geometry.h"

using namespace zrt;

static int validate_materials(const zrt_scene* s);

// ZRT_TIMING=1: context creation's stages on stderr ("timing:" lines), each
// closed by a stream sync (the start-up split of VERDICT r5 #6)
struct StageClock {
    bool on = getenv("ZRT_TIMING") != nullptr;
    double t = 0.0;
    static double now_ms() {
        timespec ts;
        clock_gettime(CLOCK_MONOTONIC, &ts);
        return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6;
    }
    StageClock() { t = now_ms(); }
    void mark(const zrt_context* c, const char* what);
};

void StageClock::mark(const zrt_context* c, const char* what) {
    if (!on) return;
    (void)hipStreamSynchronize(c->stream);
    const double n = now_ms();
    fprintf(stderr, "timing: context %s %.3f ms\n", what, n - t);
    t = n;
}

static int validate_scene(const zrt_scene* s) {
    if (!s) return ZRT_ERR_INVALID_ARG;
    const uint64_t nc = (uint64_t)s->grid.resolution[0] * s->grid.resolution[1] * s->grid.resolution[2];
    if (nc == 0 || nc != s->num_cells || nc > 0x7FFFFFFFull || !s->cells) return ZRT_ERR_INVALID_ARG;
    if (s->num_triangles && (!s->triangles_pos || !s->triangles_data || !s->triangles_material))
        return ZRT_ERR_INVALID_ARG;
    for (uint64_t c = 0; c < nc; ++c) {
        const uint32_t b = s->cells[2 * c], e = s->cells[2 * c + 1];
        if (b > e || e > s->num_triangles) return ZRT_ERR_INVALID_ARG;
    }
    for (uint32_t i = 0; i < s->num_triangles; ++i)
        if (s->triangles_material[i] >= s->num_materials) return ZRT_ERR_INVALID_ARG;
    return validate_materials(s);
}

// Whether a scene needs the IEEE-division kernels (zrt_context::mt_exact):
// `n` floats of which those with k % stride in [first, stride) are checked
// (baked refs: the e1, e2 components of v0 e1 e2; source triangles: every
// vertex component, at 2^61, so that their differences stay below 2^62).
// NaN components need nothing: both forms propagate them.
static bool needs_mt_exact(const float* v, uint64_t n, uint32_t stride, uint32_t first, float lim) {
    for (uint64_t k = 0; k < n; ++k)
        if (k % stride >= first && fabsf(v[k]) >= lim) return true;
    return false;
}

// Materials and texels only (textures inside the texel array).
static int validate_materials(const zrt_scene* s) {
    if (s->num_materials == 0 || !s->materials || !s->texels) return ZRT_ERR_INVALID_ARG;
    for (uint32_t m = 0; m < s->num_materials; ++m) {
        const zrt_texture* t[3] = {&s->materials[m].base_color, &s->materials[m].emissive,
                                   &s->materials[m].transparency};
        for (int k = 0; k < 3; ++k) {
            const uint64_t ch = k < 2 ? 3 : 1;
            if (t[k]->w <= 0 || t[k]->h <= 0) return ZRT_ERR_INVALID_ARG;
            if (t[k]->offset + (uint64_t)t[k]->w * t[k]->h * ch > s->num_texel_floats)
                return ZRT_ERR_INVALID_ARG;
            if (t[k]->offset > 0xFFFFFFFFull) return ZRT_ERR_UNSUPPORTED;
        }
    }
    return ZRT_OK;
}

int grid_build_warmup();   // grid_build.hip

extern "C" int zrt_device_count(int* count) {
    if (!count) return ZRT_ERR_INVALID_ARG;
    *count = 0;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return ZRT_ERR_NO_DEVICE;
    *count = n;
    return ZRT_OK;
}

extern "C" void zrt_context_destroy(zrt_context* c) {
    if (!c) return;
    DeviceGuard g(c->device);
    if (c->d_cell32) (void)hipFree(c->d_cell32);
    void* bufs[] = {c->d_cells, c->d_pos, c->d_data, c->d_mats, c->d_texels, c->d_zig, c->d_occ, c->d_occx, c->d_esc,
                    c->d_bfc, c->d_bmask, c->d_sat, c->d_tlo,
                    c->d_pix, c->d_out, c->d_acc, c->d_rgb, c->d_lin, c->d_rays, c->d_hits, c->d_surf, c->d_nrays, c->d_counter,
                    c->d_stats, c->d_facc, c->d_fout, c->d_dn, c->d_dnio, c->d_rp, c->d_rpio,
                    c->d_sv, c->d_svio};
    for (void* b : bufs)
        if (b) (void)hipFree(b);
    for (zrt_context::PassSet& ps : c->set) {
        void* sb[] = {ps.q0, ps.q1, ps.term, ps.stk4, ps.stk2, ps.wfc, ps.hit};
        for (void* b : sb)
            if (b) (void)hipFree(b);
        if (ps.ev_join) (void)hipEventDestroy(ps.ev_join);
        if (ps.stream && ps.stream != c->stream) (void)hipStreamDestroy(ps.stream);
    }
    for (hipEvent_t e : c->ev_trace) (void)hipEventDestroy(e);
    for (hipEvent_t e : c->ev_pass) (void)hipEventDestroy(e);
    for (hipEvent_t e : c->ev_k) (void)hipEventDestroy(e);
    if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
    if (c->ev_begin) (void)hipEventDestroy(c->ev_begin);
    if (c->ev_end) (void)hipEventDestroy(c->ev_end);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

namespace {

// OccX on the device, pass 1: one thread per 4^3 brick -> its 64-bit cell
// mask (bit (z&3)<<4 | (y&3)<<2 | (x&3) = cell non-empty) and the brick bit.
__global__ __launch_bounds__(kBlock) void occx_mask_kernel(const uint2* __restrict__ cells, uint32_t r0, uint32_t r1,
                                                           uint32_t r2, uint32_t nb0, uint32_t nb1, uint32_t nb,
                                                           unsigned long long* __restrict__ masks,
                                                           uint32_t* __restrict__ bits) {
    const uint32_t b = blockIdx.x * kBlock + threadIdx.x;
    unsigned long long m = 0ull;
    if (b < nb) {
        const uint32_t bx = b % nb0, by = (b / nb0) % nb1, bz = b / (nb0 * nb1);
        for (uint32_t k = 0; k < 64; ++k) {
            const uint32_t x = bx * 4 + (k & 3u), y = by * 4 + ((k >> 2) & 3u), z = bz * 4 + (k >> 4);
            if (x < r0 && y < r1 && z < r2) {
                const uint2 c = cells[((uint64_t)z * r1 + y) * r0 + x];
                if (c.x < c.y) m |= 1ull << k;
            }
        }
        masks[b] = m;
    }
    const uint64_t bal = __ballot(b < nb && m != 0ull);
    const uint32_t lane = threadIdx.x & 63u;
    if (b < nb && (lane == 0 || lane == 32)) bits[b >> 5] = (uint32_t)(bal >> lane);
}

// Pass 2 (one block): 1 + the u16 prefix of occupied bricks per 32-brick
// word, the zero mask, then the occupied masks compacted in brick order;
// out[0] = the number of occupied bricks.
__global__ __launch_bounds__(1024) void occx_pack_kernel(const uint32_t* __restrict__ bits, uint32_t nbw,
                                                         const unsigned long long* __restrict__ masks,
                                                         uint16_t* __restrict__ prefix,
                                                         unsigned long long* __restrict__ packed,
                                                         uint32_t* __restrict__ out) {
    __shared__ uint32_t part[1024];
    const uint32_t per = (nbw + 1023u) / 1024u;
    const uint32_t w0 = threadIdx.x * per, w1 = min(w0 + per, nbw);
    uint32_t sum = 0;
    for (uint32_t wd = w0; wd < w1; ++wd) sum += (uint32_t)__popc(bits[wd]);
    part[threadIdx.x] = sum;
    __syncthreads();
    for (uint32_t off = 1; off < 1024u; off <<= 1) {            // inclusive Hillis-Steele scan
        const uint32_t v = threadIdx.x >= off ? part[threadIdx.x - off] : 0u;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    uint32_t run = part[threadIdx.x] - sum;
    for (uint32_t wd = w0; wd < w1; ++wd) {
        prefix[wd] = (uint16_t)min(run + 1u, 0xFFFFu);
        for (uint32_t wb = bits[wd]; wb; wb &= wb - 1u)
            packed[1u + run++] = masks[32u * wd + (uint32_t)__builtin_ctz(wb)];
    }
    if (threadIdx.x == 0) packed[0] = 0ull;
    if (threadIdx.x == 1023) out[0] = run;
}

}  // namespace

static int context_base(zrt_context* c) {
    StageClock sc;
    HIP_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    sc.mark(c, "stream");
    HIP_TRY(hipEventCreate(&c->ev_begin));
    HIP_TRY(hipEventCreate(&c->ev_end));
    sc.mark(c, "events");
    // one attribute, not hipGetDeviceProperties (which fills ~100 fields and
    // took ~10 ms of the CLI's start-up, r06c)
    HIP_TRY(hipDeviceGetAttribute(&c->num_cus, hipDeviceAttributeMultiprocessorCount, c->device));
    sc.mark(c, "CU count");
    return ZRT_OK;
}

static int context_materials(zrt_context* c, const zrt_scene* s);
static int context_occupancy(zrt_context* c, const uint32_t* host_cells);

// Word i of ref k's (v0, e1, e2) in the context's triangle layout.
__device__ __forceinline__ uint32_t tri_word(const float* pos, uint32_t k, uint32_t i) {
    return __float_as_uint(pos[(uint64_t)kTriFloats * k + i + i / 3]);
}
__device__ __forceinline__ bool same_tri(const float* pos, uint32_t a, uint32_t b) {
    for (uint32_t i = 0; i < 9; ++i)
        if (tri_word(pos, a, i) != tri_word(pos, b, i)) return false;
    return true;
}

// The packed walks' cell records: 8 u32 per cell at its packed-word index
// (x | y << o1 | z << o2; the padding of a non-power-of-two grid stays empty):
// begin, end, then for each entry face f = 2 * axis + (the ray steps toward
// -axis) the mask of the refs (bit k: ref begin + k) that a ray entering the
// cell across f must still test.
//
// A ray enters a cell only from the cell it has just left, across the face
// they share, and leaves a cell only after testing all of its refs
// (stage3.zig:164-182).  A ref whose (v0, e1, e2) bits equal those of a ref
// of that neighbour gives the same (hit, t, u, v) as the one already tested
// there: if that one was taken, nearest == t and `nearest > t` fails; if not,
// nearest has only shrunk since.  So skipping it changes no hit, no tie
// (ties resolve within the cell by ref order, and the kept refs keep their
// order and index) and no break test.  Refs of cells with more than 32 refs
// are all kept (mask all ones), and so are those of a face on the grid
// boundary (no ray steps in across it).  About half of all triangle tests on
// the contest stand-in repeat the previous cell's (triangles span ~5.6
// cells), a third on the Sponza-scale one.
__global__ __launch_bounds__(kBlock) void cell32_kernel(const uint2* __restrict__ cells, uint32_t r0, uint32_t r1,
                                                        uint32_t r2, uint32_t ncells, const PackK pk,
                                                        const float* __restrict__ pos, uint32_t* __restrict__ out) {
    for (uint32_t ci = blockIdx.x * kBlock + threadIdx.x; ci < ncells; ci += gridDim.x * kBlock) {
        const uint2 c = cells[ci];
        const uint32_t x = ci % r0, y = (ci / r0) % r1, z = ci / r0 / r1;
        uint32_t* rec = out + 8ull * pack_cellv(pk, x, y, z);
        rec[0] = c.x;
        rec[1] = c.y;
        const uint32_t n = c.y - c.x;
        const uint32_t all = n >= 32u ? ~0u : (1u << n) - 1u;
        for (uint32_t f = 0; f < 6; ++f) {
            const uint32_t axis = f >> 1, toward_neg = f & 1u;
            const uint32_t cc = axis == 0 ? x : (axis == 1 ? y : z), rr = axis == 0 ? r0 : (axis == 1 ? r1 : r2);
            // the cell left: one step back against the ray's direction
            const bool inside = toward_neg ? cc + 1u < rr : cc > 0u;
            uint32_t m = all;
            if (inside && n > 0u && n <= 32u) {
                const uint32_t step = axis == 0 ? 1u : (axis == 1 ? r0 : r0 * r1);
                const uint2 pc = cells[toward_neg ? ci + step : ci - step];
                for (uint32_t k = 0; k < n; ++k)
                    for (uint32_t q = pc.x; q < pc.y; ++q)
                        if (same_tri(pos, c.x + k, q)) {
                            m &= ~(1u << k);
                            break;
                        }
            }
            rec[2 + f] = m;
        }
    }
}

// Hop bits (wf_park_kernel's one-cell lookahead), second pass over the cell
// records.  Bits 26..31 of the six mask words of a cell of 1..26 refs are
// free: every reader takes a mask's low `n` bits.  They hold six hop bits,
// INVERTED: bit 26 + f CLEARED says that a ray leaving this cell by a step
// in the direction of face index f (2 * axis + toward minus) may walk
// through the next cell as if it were empty -- that neighbour lies inside
// the grid, holds 1..32 refs, and its entry-face mask for the same f keeps
// none of them: each was tested in this cell, which the ray leaves only
// after testing all of its own.  Inverted, so that every all-ones word (the
// first cell's, the cull table's, a boundary face, a cell of 32 refs or more)
// reads as "no hop".  Cells of 27 refs or more have no room: the kernel takes
// no hop bit from them; like the words of an empty cell, theirs get ones in
// every bit above the mask's own, so that any word reads "no hop" by its bits
// alone.
// The neighbour's word may be rewritten by its own thread meanwhile, in bits
// the bits above its n only; its low n bits, all that is read here, were
// final when pass 1 ended.
__global__ __launch_bounds__(kBlock) void cell32_hop_kernel(const uint2* __restrict__ cells, uint32_t r0, uint32_t r1,
                                                            uint32_t r2, uint32_t ncells, const PackK pk,
                                                            uint32_t* __restrict__ out) {
    for (uint32_t ci = blockIdx.x * kBlock + threadIdx.x; ci < ncells; ci += gridDim.x * kBlock) {
        const uint2 c = cells[ci];
        const uint32_t n = c.y - c.x;
        if (n >= 32u) continue;
        const uint32_t x = ci % r0, y = (ci / r0) % r1, z = ci / r0 / r1;
        uint32_t* rec = out + 8ull * pack_cellv(pk, x, y, z);
        if (n > kHopMaxRefs) {                     // no room: the bits above the mask's read "no hop" all the same
            for (uint32_t f = 0; f < 6; ++f) rec[2 + f] |= ~((1u << n) - 1u);
            continue;
        }
        uint32_t hop = 0x3Fu;
        for (uint32_t f = 0; f < 6 && n != 0u; ++f) {
            const uint32_t axis = f >> 1, toward_neg = f & 1u;
            const uint32_t cc = axis == 0 ? x : (axis == 1 ? y : z), rr = axis == 0 ? r0 : (axis == 1 ? r1 : r2);
            // the cell entered: one step along the ray's direction
            if (toward_neg ? cc == 0u : cc + 1u >= rr) continue;
            const uint32_t d = toward_neg ? ~0u : 1u;
            const uint32_t* nrec = out + 8ull * pack_cellv(pk, axis == 0 ? x + d : x, axis == 1 ? y + d : y,
                                                           axis == 2 ? z + d : z);
            const uint32_t nn = nrec[1] - nrec[0];
            if (nn == 0u || nn > 32u) continue;
            const uint32_t low = nn == 32u ? ~0u : (1u << nn) - 1u;
            if ((nrec[2 + f] & low) == 0u) hop &= ~(1u << f);
        }
        for (uint32_t f = 0; f < 6; ++f) rec[2 + f] = (rec[2 + f] & ((1u << kHopShift) - 1u)) | (hop << kHopShift);
    }
}

// Park release statistic (context_release): over the occupied cells of the
// packed records, how many (cell, entry face) masks are 0 in the cell's low n
// bits (the bits above them of a cell of at most 26 refs are hop bits) --
// out[0] masks of occupied cells, out[1] zero masks among them.
__global__ __launch_bounds__(kBlock) void release_stat_kernel(const uint32_t* __restrict__ rec, uint64_t n,
                                                              unsigned long long* __restrict__ out) {
    unsigned long long faces = 0, zero = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
        const uint32_t* r = rec + 8 * i;
        if (r[1] > r[0]) {
            faces += 6;
            const uint32_t n = r[1] - r[0], low = n >= 32u ? ~0u : (1u << n) - 1u;
            for (int f = 0; f < 6; ++f) zero += (r[2 + f] & low) == 0u ? 1 : 0;
        }
    }
    faces = wave_sum(faces);
    zero = wave_sum(zero);
    if ((threadIdx.x & 63u) == 0) {
        atomicAdd(&out[0], faces);
        atomicAdd(&out[1], zero);
    }
}

// The packed walks' layout (DdaV) and their cell records (cell32_kernel;
// none beyond 16 GiB, or beyond 1 GiB and 16x the cells' own 8 B -- flat
// grids whose narrow axis pack_layout widened: such a grid walks unpacked).
constexpr uint64_t kCell32Max = 16ull << 30;
constexpr double kRelMinFrac = 0.25;   // park release from this fraction of empty entry-face masks
static int context_packed(zrt_context* c) {
    const uint32_t* r = c->grid.resolution;
    // brick-major words where the grid allows them and the primary's
    // occupancy bricks are 4^3 (it reads them by pc >> 6); else field words
    // (and the dense brick masks exist: trace_ray reads them by pc >> 6)
    c->packed = pack_layout(r, c->pk, c->occ_shift == 2u && c->d_bmask != nullptr);
    if (!c->packed) return ZRT_OK;
    const uint64_t n = 1ull << (c->pk.b0 + c->pk.b1 + c->pk.b2);
    if (32 * n > kCell32Max || (n > 16ull * c->ncells && 32 * n > (1ull << 30))) {
        c->packed = false;
        return ZRT_OK;
    }
    HIP_TRY(hipMalloc((void**)&c->d_cell32, 32 * n));
    if (!pack_is_linear(r, c->pk)) HIP_TRY(hipMemsetAsync(c->d_cell32, 0, 32 * n, c->stream));
    hipLaunchKernelGGL(cell32_kernel, dim3(std::min<uint32_t>((c->ncells + kBlock - 1) / kBlock, 16384)), dim3(kBlock),
                       0, c->stream, c->d_cells, r[0], r[1], r[2], c->ncells, c->pk, c->d_pos,
                       c->d_cell32);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(cell32_hop_kernel, dim3(std::min<uint32_t>((c->ncells + kBlock - 1) / kBlock, 16384)),
                       dim3(kBlock), 0, c->stream, c->d_cells, r[0], r[1], r[2], c->ncells, c->pk, c->d_cell32);
    HIP_TRY(hipGetLastError());
    // the park release pays on scenes whose rays often park in a cell with
    // nothing left to test for their entry face: r06q/r06r, alternating
    // processes, images identical: Cornell box (65% of the occupied cells'
    // entry faces empty) +7%, contest stand-in (29%) +3%, Sponza-scale
    // stand-in (18%) -1.5% (profiles/r06/r06q_ab_park_release.log)
    {
        unsigned long long h[2] = {0, 0};
        unsigned long long* d = nullptr;
        HIP_TRY(hipMalloc((void**)&d, sizeof h));
        hipError_t e = hipMemsetAsync(d, 0, sizeof h, c->stream);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(release_stat_kernel, dim3(std::min<uint64_t>((n + kBlock - 1) / kBlock, 4096)),
                               dim3(kBlock), 0, c->stream, (const uint32_t*)c->d_cell32, n, d);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpyAsync(h, d, sizeof h, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        (void)hipFree(d);
        HIP_TRY(e);
        c->rel_frac = h[0] ? (double)h[1] / (double)h[0] : 0.0;
        c->rel_on = c->rel_frac >= kRelMinFrac;
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    return ZRT_OK;
}

// Back-face cull masks (escape.h bfc_cull): word pc * kBfcNBin + bin for
// every packed cell word pc and cull bin, then one all-ones word.  Bit r of
// a cell of 1..32 refs is cleared when ref begin + r cannot pass tri_ray's
// determinant test for any direction of the bin; every other cell keeps all
// ones.  stat[0]: ref bits of the cells of 1..32 refs over all bins, stat[1]:
// those cleared, stat[2]: (such cell, bin) words, stat[3]: those left empty.
__global__ __launch_bounds__(kBlock) void bfc_build_kernel(const uint32_t* __restrict__ rec, uint64_t ncell,
                                                           const float* __restrict__ pos, uint32_t* __restrict__ out,
                                                           unsigned long long* __restrict__ stat) {
    const uint64_t total = ncell * kBfcNBin;
    unsigned long long bits = 0, cleared = 0, words = 0, empty = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (uint64_t)gridDim.x * kBlock) {
        const uint64_t pc = i / kBfcNBin;
        const uint32_t bin = (uint32_t)(i - pc * kBfcNBin);
        const uint32_t b = rec[8 * pc], n = rec[8 * pc + 1] - b;
        uint32_t m = ~0u;
        if (n >= 1u && n <= 32u) {
            for (uint32_t r = 0; r < n; ++r) {
                float e1[3], e2[3];
                for (uint32_t k = 0; k < 3; ++k) {
                    e1[k] = __uint_as_float(tri_word(pos, b + r, 3 + k));
                    e2[k] = __uint_as_float(tri_word(pos, b + r, 6 + k));
                }
                if (bfc_cull(e1, e2, bin)) m &= ~(1u << r);
            }
            const uint32_t all = n == 32u ? ~0u : (1u << n) - 1u;
            bits += n;
            cleared += n - (uint32_t)__popc(m & all);
            words += 1;
            empty += (m & all) == 0u ? 1 : 0;
            // the cell's hop bits (cell32_hop_kernel; the same six in each of its
            // mask words), so that a lane walking on from its first cell may hop too
            if (n <= kHopMaxRefs) m = (m & ((1u << kHopShift) - 1u)) | (rec[8 * pc + 2] & ~((1u << kHopShift) - 1u));
        }
        if (out) out[i] = m;                       // (null: the statistic only)
    }
    if (out && blockIdx.x == 0 && threadIdx.x == 0) out[total] = ~0u;
    bits = wave_sum(bits);
    cleared = wave_sum(cleared);
    words = wave_sum(words);
    empty = wave_sum(empty);
    if ((threadIdx.x & 63u) == 0) {
        atomicAdd(&stat[0], bits);
        atomicAdd(&stat[1], cleared);
        atomicAdd(&stat[2], words);
        atomicAdd(&stat[3], empty);
    }
}

// The table is packed cells x kBfcNBin x 4 B (the contest stand-in at 128^3:
// 0.8 GB at 4 x 4 bins per face, 3.2 GB at 8 x 8): built only if it fits
// kBfcBudget over the contexts sharing the device, else the park kernel
// renders without it.
constexpr uint64_t kBfcBudget = (uint64_t)ZRT_BFC_BUDGET_MB << 20;
// Unasked, the park launches use the masks when they remove at least this
// many triangle tests from a first-cell park on average (cleared bits per
// (cell, bin) word over the cells of 1..32 refs): the park pays one more
// gather for them.  Measured (r07b): Cornell box 0.36, -2.6%;
// contest stand-in 1.78, +1.1%; Sponza-scale stand-in 2.39, +3.8%.
constexpr double kBfcMinCleared = ZRT_BFC_MIN_CLEARED;
// forced: build the table whatever the statistic says (ZRT_FLAG_BFCULL).
int context_bfcull(zrt_context* c, bool forced) {
    if (c->d_bfc || !c->packed || !c->d_cell32) return ZRT_OK;
    const uint64_t n = 1ull << (c->pk.b0 + c->pk.b1 + c->pk.b2);
    const uint64_t bytes = 4ull * (n * kBfcNBin + 1);
    if (bytes > kBfcBudget / std::max<uint32_t>(c->mem_share, 1u)) return ZRT_OK;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || free_b / 4 < bytes) return ZRT_OK;
    // one pass for the statistic alone (no table), one that writes the table
    // if the scene uses it
    unsigned long long* d = nullptr;
    HIP_TRY(hipMalloc((void**)&d, 4 * sizeof(unsigned long long)));
    const uint64_t blocks = (n * kBfcNBin + kBlock - 1) / kBlock;
    auto pass = [&](uint32_t* out, unsigned long long* h) -> hipError_t {
        hipError_t e = hipMemsetAsync(d, 0, 4 * sizeof(unsigned long long), c->stream);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(bfc_build_kernel, dim3((uint32_t)std::min<uint64_t>(blocks, 1u << 16)), dim3(kBlock), 0,
                           c->stream, (const uint32_t*)c->d_cell32, n, (const float*)c->d_pos, out, d);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        if ((e = hipMemcpyAsync(h, d, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream)) != hipSuccess)
            return e;
        return hipStreamSynchronize(c->stream);
    };
    unsigned long long h[4] = {0, 0, 0, 0};
    hipError_t e = hipSuccess;
    if (!c->bfc_stat) {
        e = pass(nullptr, h);
        if (e == hipSuccess) {
            c->bfc_stat = true;
            c->bfc_frac = h[0] ? (double)h[1] / (double)h[0] : 0.0;
            c->bfc_cleared = h[2] ? (double)h[1] / (double)h[2] : 0.0;
            c->bfc_on = c->bfc_cleared >= kBfcMinCleared;
            if (getenv("ZRT_WF_DEBUG"))
                fprintf(stderr, "{\"zrt_bfcull\": {\"bytes\": %llu, \"bins\": %u, \"cleared_frac\": %.4f, "
                        "\"cleared_per_word\": %.4f, \"empty_word_frac\": %.4f, \"on\": %d}}\n",
                        (unsigned long long)bytes, kBfcNBin, c->bfc_frac, c->bfc_cleared,
                        h[2] ? (double)h[3] / (double)h[2] : 0.0, c->bfc_on ? 1 : 0);
        }
    }
    uint32_t* tab = nullptr;
    if (e == hipSuccess && (c->bfc_on || forced)) {
        e = hipMalloc((void**)&tab, bytes);
        if (e == hipSuccess) e = pass(tab, h);
        if (e != hipSuccess && tab) (void)hipFree(tab);
    }
    (void)hipFree(d);
    HIP_TRY(e);
    if (tab) {
        c->d_bfc = tab;
        c->bfc_bytes = bytes;
    }
    return ZRT_OK;
}

static int context_counters(zrt_context* c) {
    StageClock sc;
    int rc = context_packed(c);
    if (rc != ZRT_OK) return rc;
    sc.mark(c, "cell records (cell32_kernel)");
    HIP_TRY(hipMalloc((void**)&c->d_counter, 64));
    HIP_TRY(hipMalloc((void**)&c->d_stats, 512));
    return ZRT_OK;
}

static int context_init(zrt_context* c, const zrt_scene* s) {
    int rc = context_base(c);
    if (rc != ZRT_OK) return rc;
    c->grid = s->grid;
    c->ncells = s->num_cells;
    c->nrefs = s->num_triangles;
    c->nmat = s->num_materials;
    c->mt_exact = needs_mt_exact(s->triangles_pos, 9ull * s->num_triangles, 9u, 3u, 0x1p62f);
    HIP_TRY(hipMalloc((void**)&c->d_cells, 8ull * c->ncells));
    HIP_TRY(copy_sync(c->d_cells, s->cells, 8ull * c->ncells, hipMemcpyHostToDevice, c->stream));
    const size_t nr = std::max<size_t>(c->nrefs, 1);
    std::vector<float> pos(kTriFloats * nr, 0.0f);
    std::vector<float4> dat(4 * nr);
    for (uint32_t i = 0; i < c->nrefs; ++i) {
        const float* q = s->triangles_pos + 9ull * i;
        float* o = pos.data() + (size_t)kTriFloats * i;
        memcpy(o, q, 12); memcpy(o + 4, q + 3, 12); memcpy(o + 8, q + 6, 12);
        float tmp[16];
        memcpy(tmp, s->triangles_data + 15ull * i, 15 * sizeof(float));
        memcpy(&tmp[15], &s->triangles_material[i], 4);
        memcpy(&dat[4 * i], tmp, 64);
    }
    HIP_TRY(hipMalloc((void**)&c->d_pos, pos.size() * sizeof(float)));
    HIP_TRY(copy_sync(c->d_pos, pos.data(), pos.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMalloc((void**)&c->d_data, dat.size() * sizeof(float4)));
    HIP_TRY(copy_sync(c->d_data, dat.data(), dat.size() * sizeof(float4), hipMemcpyHostToDevice, c->stream));
    if ((rc = context_materials(c, s)) != ZRT_OK) return rc;
    return context_occupancy(c, s->cells);
}

// Materials, texels, ziggurat tables (stage3.zig:125-129, Zig std ziggurat).
static int context_materials(zrt_context* c, const zrt_scene* s) {
    c->nmat = s->num_materials;
    std::vector<DevMat> mats(c->nmat);
    for (uint32_t m = 0; m < c->nmat; ++m) {
        const zrt_texture* t[3] = {&s->materials[m].base_color, &s->materials[m].emissive,
                                   &s->materials[m].transparency};
        for (int k = 0; k < 3; ++k) {
            DevTex& d = mats[m].tex[k];
            d.off = (uint32_t)t[k]->offset;
            d.w = t[k]->w; d.h = t[k]->h;
            d.umin = t[k]->u_min; d.umax = t[k]->u_max;
            d.vmin = t[k]->v_min; d.vmax = t[k]->v_max;
            d.pad = 0;
            dev_tex_inline(d, s->texels, k < 2 ? 3 : 1);
        }
    }
    StageClock sc;
    HIP_TRY(hipMalloc((void**)&c->d_mats, mats.size() * sizeof(DevMat)));
    HIP_TRY(copy_sync(c->d_mats, mats.data(), mats.size() * sizeof(DevMat), hipMemcpyHostToDevice, c->stream));
    sc.mark(c, "materials");
    HIP_TRY(hipMalloc((void**)&c->d_texels, s->num_texel_floats * sizeof(float)));
    HIP_TRY(copy_sync(c->d_texels, s->texels, s->num_texel_floats * sizeof(float), hipMemcpyHostToDevice, c->stream));
    sc.mark(c, "texels");
    double zig[514];
    zig_tables(zig, zig + 257);
    sc.mark(c, "ziggurat tables (host)");
    HIP_TRY(hipMalloc((void**)&c->d_zig, sizeof zig));
    HIP_TRY(copy_sync(c->d_zig, zig, sizeof zig, hipMemcpyHostToDevice, c->stream));
    sc.mark(c, "ziggurat upload");
    return ZRT_OK;
}

// Brick occupancy and OccX, from the host cells or (host_cells null) from
// c->d_cells on the device; then the work counters.
//  * OccX (the park kernel) is built on 4^3-cell bricks and used when it fits
//    the LDS budget.
//  * wf_kernel's brick bits sit in LDS beside 7 waves' worth of workgroups:
//    4^3-cell bricks (4 KB of bits for a 128^3 grid, round 1's best) while
//    the bits take at most kOccLdsMax bytes, coarser bricks (8^3, 16^3, ...:
//    OR of the 4^3 ones) for larger grids -- result-invariant, an empty brick
//    only lets the walk skip the range loads of its cells.
constexpr uint64_t kOccLdsMax = (uint64_t)ZRT_OCC_LDS_KB << 10;

__global__ __launch_bounds__(kBlock) void occ_coarsen_kernel(const uint32_t* __restrict__ bits4, uint32_t nb0,
                                                             uint32_t nb1, uint32_t nb, uint32_t dsh, uint32_t cn0,
                                                             uint32_t cn01, uint32_t* __restrict__ out) {
    const uint32_t b = blockIdx.x * kBlock + threadIdx.x;
    if (b >= nb || !((bits4[b >> 5] >> (b & 31u)) & 1u)) return;
    const uint32_t bx = b % nb0, by = (b / nb0) % nb1, bz = b / (nb0 * nb1);
    const uint32_t cb = (bz >> dsh) * cn01 + (by >> dsh) * cn0 + (bx >> dsh);
    atomicOr(&out[cb >> 5], 1u << (cb & 31u));
}

// Coarse brick bits straight from the cells (device-built grids whose 4^3
// bricks are too many for OccX): one thread per cell, atomicOr per non-empty one.
__global__ __launch_bounds__(kBlock) void occ_cells_kernel(const uint2* __restrict__ cells, uint32_t r0, uint32_t r1,
                                                           uint32_t ncells, uint32_t sh, uint32_t cn0, uint32_t cn01,
                                                           uint32_t* __restrict__ out) {
    for (uint32_t ci = blockIdx.x * kBlock + threadIdx.x; ci < ncells; ci += gridDim.x * kBlock) {
        const uint2 c = cells[ci];
        if (c.x >= c.y) continue;
        const uint32_t x = ci % r0, y = (ci / r0) % r1, z = ci / r0 / r1;
        const uint32_t cb = (z >> sh) * cn01 + (y >> sh) * cn0 + (x >> sh);
        atomicOr(&out[cb >> 5], 1u << (cb & 31u));
    }
}

// Escape table (escape.h): a summed-area table of cell occupancy, then one
// thread per (region of a 4^3 brick, direction bin).
__global__ __launch_bounds__(kBlock) void esc_sat_fill_kernel(const uint2* __restrict__ cells, uint32_t r0, uint32_t r1,
                                                              uint32_t ncells, uint32_t n0, uint32_t n01,
                                                              uint32_t* __restrict__ sat) {
    for (uint32_t ci = blockIdx.x * kBlock + threadIdx.x; ci < ncells; ci += gridDim.x * kBlock) {
        const uint2 c = cells[ci];
        const uint32_t x = ci % r0, y = (ci / r0) % r1, z = ci / r0 / r1;
        sat[(uint64_t)(z + 1) * n01 + (uint64_t)(y + 1) * n0 + x + 1] = c.x < c.y ? 1u : 0u;
    }
}
// The same for a batch of per-direction occupancies (escape.h
// esc_dir_occupied): volume k of the batch is cull bin cb0 + k's.
__global__ __launch_bounds__(kBlock) void esc_dir_fill_kernel(const uint2* __restrict__ cells,
                                                              const float* __restrict__ pos, uint32_t r0, uint32_t r1,
                                                              uint32_t ncells, uint32_t n0, uint32_t n01, uint64_t vol,
                                                              uint32_t cb0, uint32_t ncb, uint32_t* __restrict__ sat) {
    const uint64_t total = (uint64_t)ncells * ncb;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (uint64_t)gridDim.x * kBlock) {
        const uint32_t k = (uint32_t)(i / ncells), ci = (uint32_t)(i - (uint64_t)k * ncells);
        const uint2 c = cells[ci];
        const uint32_t x = ci % r0, y = (ci / r0) % r1, z = ci / r0 / r1;
        const bool occ = esc_dir_occupied(c.x, c.y, [&](uint32_t r, float* e1, float* e2) {
            for (uint32_t j = 0; j < 3; ++j) {
                e1[j] = __uint_as_float(tri_word(pos, r, 3 + j));
                e2[j] = __uint_as_float(tri_word(pos, r, 6 + j));
            }
        }, cb0 + k);
        sat[k * vol + (uint64_t)(z + 1) * n01 + (uint64_t)(y + 1) * n0 + x + 1] = occ ? 1u : 0u;
    }
}
// prefix sums along one axis of the (n0 x n1 x n2) volume: one thread per
// line; blockIdx.y: the volume of a batch
__global__ __launch_bounds__(kBlock) void esc_sat_scan_kernel(uint32_t* __restrict__ sat, uint32_t n0, uint32_t n1,
                                                              uint32_t n2, uint32_t axis) {
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    const uint64_t n01 = (uint64_t)n0 * n1;
    sat += (uint64_t)blockIdx.y * n01 * n2;
    uint64_t base, stride;
    uint32_t len;
    if (axis == 0) {
        if (t >= n1 * n2) return;
        base = (uint64_t)(t / n1) * n01 + (uint64_t)(t % n1) * n0; stride = 1; len = n0;
    } else if (axis == 1) {
        if (t >= n0 * n2) return;
        base = (uint64_t)(t / n0) * n01 + t % n0; stride = n0; len = n1;
    } else {
        if (t >= n0 * n1) return;
        base = t; stride = n01; len = n2;
    }
    uint32_t acc = 0;
    for (uint32_t i = 0; i < len; ++i) {
        acc += sat[base + i * stride];
        sat[base + i * stride] = acc;
    }
}
__global__ __launch_bounds__(kBlock) void esc_build_kernel(const uint32_t* __restrict__ sat, uint32_t r0, uint32_t r1,
                                                           uint32_t r2, float cs0, float cs1, float cs2, uint32_t nb0,
                                                           uint32_t nb1, uint32_t nbr, EscShape sh,
                                                           uint32_t* __restrict__ esc) {
    const uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const uint32_t lg = esc_regions_lg(sh);
    if (t >= ((uint64_t)nbr << lg) * kEscNBin) return;
    const uint32_t rg = (uint32_t)(t / kEscNBin), bin = (uint32_t)(t % kEscNBin);
    const uint32_t br = rg >> lg, sub = rg & ((1u << lg) - 1u);
    const uint32_t res[3] = {r0, r1, r2};
    const float cs[3] = {cs0, cs1, cs2};
    const EscSat S{sat, r0 + 1u, (r0 + 1u) * (r1 + 1u)};
    if (esc_compute_region(S, res, cs, sh, br % nb0, (br / nb0) % nb1, br / (nb0 * nb1), sub, bin))
        atomicOr(&esc[(uint64_t)rg * kEscWords + (bin >> 5)], 1u << (bin & 31u));
}
// The direction-aware table (escape.h): one thread per (cull bin of the
// batch, region, escape bin of the cull bin), cull bin outermost so that
// neighbouring threads read the same summed-area table.
__global__ __launch_bounds__(kBlock) void esc_build_dir_kernel(const uint32_t* __restrict__ sat, uint64_t vol,
                                                               uint32_t cb0, uint32_t ncb, uint32_t r0, uint32_t r1,
                                                               uint32_t r2, float cs0, float cs1, float cs2,
                                                               uint32_t nb0, uint32_t nb1, uint32_t nbr, EscShape sh,
                                                               uint32_t* __restrict__ esc) {
    const uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const uint32_t lg = esc_regions_lg(sh);
    const uint64_t per = ((uint64_t)nbr << lg) * kEscPerCull;
    if (t >= per * ncb) return;
    const uint32_t k = (uint32_t)(t / per);
    const uint64_t rem = t - (uint64_t)k * per;
    const uint32_t rg = (uint32_t)(rem / kEscPerCull), bin = esc_bin_of_cull(cb0 + k, (uint32_t)(rem % kEscPerCull));
    const uint32_t br = rg >> lg, sub = rg & ((1u << lg) - 1u);
    const uint32_t res[3] = {r0, r1, r2};
    const float cs[3] = {cs0, cs1, cs2};
    const EscSat S{sat + k * vol, r0 + 1u, (r0 + 1u) * (r1 + 1u)};
    if (esc_compute_region(S, res, cs, sh, br % nb0, (br / nb0) % nb1, br / (nb0 * nb1), sub, bin))
        atomicOr(&esc[(uint64_t)rg * kEscWords + (bin >> 5)], 1u << (bin & 31u));
}

// Least fraction of set escape bits for the park launches to use the table.
constexpr double kEscMinDensity = 0.12;

// The summed-area table of cell occupancy (escape.h EscSat): kept in the
// context for the escape table and the primary frustum bounds; none for grids
// whose table would pass 2^28 entries (1 GiB).
static int context_sat(zrt_context* c) {
    const uint32_t* r = c->grid.resolution;
    const uint64_t n0 = r[0] + 1ull, n1 = r[1] + 1ull, n2 = r[2] + 1ull;
    if (n0 * n1 * n2 > (1ull << 28)) return ZRT_OK;
    HIP_TRY(hipMalloc((void**)&c->d_sat, 4ull * n0 * n1 * n2));
    HIP_TRY(hipMemsetAsync(c->d_sat, 0, 4ull * n0 * n1 * n2, c->stream));
    hipLaunchKernelGGL(esc_sat_fill_kernel, dim3(4096), dim3(kBlock), 0, c->stream, c->d_cells, r[0], r[1], c->ncells,
                       (uint32_t)n0, (uint32_t)(n0 * n1), c->d_sat);
    const uint64_t lines[3] = {n1 * n2, n0 * n2, n0 * n1};
    for (uint32_t a = 0; a < 3; ++a)
        hipLaunchKernelGGL(esc_sat_scan_kernel, dim3((uint32_t)((lines[a] + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                           c->stream, c->d_sat, (uint32_t)n0, (uint32_t)n1, (uint32_t)n2, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    return ZRT_OK;
}

// The escape table (escape.h) for a context with OccX (the park walk); none
// for grids whose summed-area table would pass 2^28 entries (the walk then
// never stops early, as before).
int context_escape(zrt_context* c, bool forced) {
    if (!c->occx_ok || !c->d_sat) return ZRT_OK;
    const uint32_t* r = c->grid.resolution;
    const uint64_t nbr = (uint64_t)c->occx_nb[0] * c->occx_nb[1] * c->occx_nb[2];
    StageClock sc;
    // one table at shape `sh` into *out (threads < 2^31 blocks: the caller's budget)
    auto build = [&](const EscShape& sh, uint32_t** out) -> int {
        const uint64_t bytes = (4ull * kEscWords * nbr) << esc_regions_lg(sh);
        HIP_TRY(hipMalloc((void**)out, bytes));
        HIP_TRY(hipMemsetAsync(*out, 0, bytes, c->stream));
        const uint64_t nthr = (nbr << esc_regions_lg(sh)) * kEscNBin;
        hipLaunchKernelGGL(esc_build_kernel, dim3((uint32_t)((nthr + kBlock - 1) / kBlock)), dim3(kBlock), 0, c->stream,
                           (const uint32_t*)c->d_sat, r[0], r[1], r[2], c->grid.cell_size[0], c->grid.cell_size[1],
                           c->grid.cell_size[2], c->occx_nb[0], c->occx_nb[1], (uint32_t)nbr, sh, *out);
        HIP_TRY(hipGetLastError());
        return ZRT_OK;
    };
    // The brick-level table: the park kernel's, unless a finer shape fits below.
    int rc;
    if ((rc = build(kEscBrick, &c->d_esc)) != ZRT_OK) return rc;
    // Use it when enough of its bits are set: each walk trip of the park
    // kernel then issues a table query per brick entered (~4% of a launch on
    // scenes whose rays never escape, r04g), and the check itself costs ~1.5%.
    // Measured (r04): contest stand-in 23% of the bits set, +8% frame rate;
    // Cornell box 6%, -1.5%; Sponza-scale 1.6%, -4%.
    // (The statistic stays the brick-level one whatever shape the walk asks.)
    std::vector<uint32_t> h(kEscWords * nbr);
    HIP_TRY(hipMemcpyAsync(h.data(), c->d_esc, 4ull * kEscWords * nbr, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    uint64_t set = 0;
    for (uint32_t x : h) set += (uint64_t)__builtin_popcount(x);
    c->esc_density = (double)set / ((double)nbr * kEscNBin);
    c->esc_on = c->esc_density >= kEscMinDensity;
    sc.mark(c, "escape table (bricks)");
    // The table the walk asks: keyed by sub-brick regions (escape.h
    // esc_shape_for: 16 per brick, 16 times the bytes and the build time, once
    // per context; cfg3: 25 MB, 35 ms against 1.6 MB, 2.5 ms), if it fits a
    // quarter of the free memory, the park kernel's 32-bit byte offsets and a
    // launch's 2^31 blocks; else the brick-level table stays.  Only where the
    // launches will use it: the scene's statistic says so, or this call's flag.
    // ZRT_ESC_BRICK=1 keeps it too (tools/ A/B runs and the tests).
    const float cs[3] = {c->grid.cell_size[0], c->grid.cell_size[1], c->grid.cell_size[2]};
    const EscShape sh = esc_shape_for(cs);
    const uint32_t lg = esc_regions_lg(sh);
    const uint64_t bytes = (4ull * kEscWords * nbr) << lg;
    size_t free_b = 0, total_b = 0;
    const bool fits = (c->esc_on || forced) && esc_cells_regular(cs) && !getenv("ZRT_ESC_BRICK") &&
                      hipMemGetInfo(&free_b, &total_b) == hipSuccess && bytes <= free_b / 4 && bytes < (1ull << 32) &&
                      ((nbr << lg) * kEscNBin) / kBlock < (1ull << 31);
    if (fits) {
        // Direction-aware (escape.h): one occupancy and summed-area table per
        // cull bin, transient, in batches of as many volumes as fit a quarter
        // of the memory that is free beside the table itself; if not even one
        // fits, the plain region table as before.  ZRT_ESC_PLAIN=1 keeps the
        // plain one too (tools/ A/B runs and the tests).
        const uint64_t n0 = r[0] + 1ull, n1 = r[1] + 1ull, n2 = r[2] + 1ull, vol = n0 * n1 * n2;
        uint32_t batch = 0;
        if (!getenv("ZRT_ESC_PLAIN") && c->d_pos && free_b >= bytes)
            batch = (uint32_t)std::min<uint64_t>(kBfcNBin, (free_b - bytes) / 4 / (4ull * vol));
        // (a launch's 2^31 blocks)
        while (batch && ((nbr << lg) * kEscPerCull * batch) / kBlock >= (1ull << 31)) batch /= 2;
        uint32_t* fine = nullptr;
        struct Volumes {
            uint32_t* p = nullptr;
            ~Volumes() {
                if (p) (void)hipFree(p);
            }
        } tmp;
        if (batch && hipMalloc((void**)&tmp.p, 4ull * vol * batch) != hipSuccess) {
            (void)hipGetLastError();
            tmp.p = nullptr;
            batch = 0;
        }
        if (!batch) {
            if ((rc = build(sh, &fine)) != ZRT_OK) {
                (void)hipFree(fine);
                return rc;
            }
        } else {
            hipError_t e = hipMalloc((void**)&fine, bytes);
            if (e == hipSuccess) e = hipMemsetAsync(fine, 0, bytes, c->stream);
            const uint64_t lines[3] = {n1 * n2, n0 * n2, n0 * n1};
            for (uint32_t cb0 = 0; e == hipSuccess && cb0 < kBfcNBin; cb0 += batch) {
                const uint32_t ncb = std::min<uint32_t>(batch, kBfcNBin - cb0);
                e = hipMemsetAsync(tmp.p, 0, 4ull * vol * ncb, c->stream);
                if (e != hipSuccess) break;
                hipLaunchKernelGGL(esc_dir_fill_kernel, dim3(16384), dim3(kBlock), 0, c->stream, c->d_cells,
                                   (const float*)c->d_pos, r[0], r[1], c->ncells, (uint32_t)n0, (uint32_t)(n0 * n1), vol,
                                   cb0, ncb, tmp.p);
                sc.mark(c, "escape table (per-direction occupancies)");
                for (uint32_t a = 0; a < 3; ++a)
                    hipLaunchKernelGGL(esc_sat_scan_kernel, dim3((uint32_t)((lines[a] + kBlock - 1) / kBlock), ncb),
                                       dim3(kBlock), 0, c->stream, tmp.p, (uint32_t)n0, (uint32_t)n1, (uint32_t)n2, a);
                sc.mark(c, "escape table (their prefix sums)");
                const uint64_t nthr = (nbr << lg) * kEscPerCull * ncb;
                hipLaunchKernelGGL(esc_build_dir_kernel, dim3((uint32_t)((nthr + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                                   c->stream, (const uint32_t*)tmp.p, vol, cb0, ncb, r[0], r[1], r[2],
                                   c->grid.cell_size[0], c->grid.cell_size[1], c->grid.cell_size[2], c->occx_nb[0],
                                   c->occx_nb[1], (uint32_t)nbr, sh, fine);
                e = hipGetLastError();
            }
            if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
            if (e != hipSuccess) {
                (void)hipFree(fine);
                HIP_TRY(e);
            }
        }
        HIP_TRY(hipStreamSynchronize(c->stream));
        (void)hipFree(c->d_esc);
        c->d_esc = fine;
        c->esc_extra = bytes - 4ull * kEscWords * nbr;
        c->esc_key = esc_walk_key(sh);
        c->esc_dir = batch != 0;
        sc.mark(c, c->esc_dir ? "escape table (regions, per direction bin)" : "escape table (regions)");
        if (getenv("ZRT_WF_DEBUG")) {
            std::vector<uint32_t> hf(bytes / 4);
            HIP_TRY(hipMemcpy(hf.data(), fine, bytes, hipMemcpyDeviceToHost));
            uint64_t nset = 0;
            for (uint32_t x : hf) nset += (uint64_t)__builtin_popcount(x);
            fprintf(stderr, "{\"zrt_escape\": {\"bytes\": %llu, \"per_direction\": %d, \"batch\": %u, "
                    "\"brick_density\": %.4f, \"region_density\": %.4f}}\n", (unsigned long long)bytes,
                    c->esc_dir ? 1 : 0, batch, c->esc_density, (double)nset / ((double)(nbr << lg) * kEscNBin));
        }
    }
    return ZRT_OK;
}

static int context_occupancy(zrt_context* c, const uint32_t* host_cells) {
    StageClock sc_occ;
    const uint32_t* r = c->grid.resolution;
    for (int i = 0; i < 3; ++i) c->occx_nb[i] = (r[i] + 3u) >> 2;
    const uint64_t nb = (uint64_t)c->occx_nb[0] * c->occx_nb[1] * c->occx_nb[2];
    // more than 2^24 4^3 bricks (> 2^30 cells): no OccX (24-bit brick
    // indices), the bounces take the lane walk over the coarse bits below
    const bool occx_possible = occx_usable(nb, 0, 0, 1);
    const uint64_t nbw = (nb + 31) / 32;
    uint32_t sh = ZRT_OCC_SH0;
    auto words_at = [&](uint32_t k) {
        const uint64_t n = (uint64_t)((r[0] + (1u << k) - 1) >> k) * ((r[1] + (1u << k) - 1) >> k) *
                           ((r[2] + (1u << k) - 1) >> k);
        return (n + 31) / 32;
    };
    while (words_at(sh) * 4 > kOccLdsMax) ++sh;
    c->occ_shift = sh;
    for (int i = 0; i < 3; ++i) c->occ_nb[i] = (r[i] + (1u << sh) - 1) >> sh;
    c->occ_words = (uint32_t)words_at(sh);
    HIP_TRY(hipMalloc((void**)&c->d_occ, 4ull * c->occ_words));
    if (host_cells) {
        std::vector<unsigned long long> mask(occx_possible ? nb : 0, 0ull);
        std::vector<uint32_t> coarse(c->occ_words, 0u);
        for (uint32_t z = 0; z < r[2]; ++z)
            for (uint32_t y = 0; y < r[1]; ++y)
                for (uint32_t x = 0; x < r[0]; ++x) {
                    const uint64_t ci = ((uint64_t)z * r[1] + y) * r[0] + x;
                    if (host_cells[2 * ci] < host_cells[2 * ci + 1]) {
                        const uint64_t b = ((uint64_t)(z >> 2) * c->occx_nb[1] + (y >> 2)) * c->occx_nb[0] + (x >> 2);
                        if (occx_possible) mask[b] |= 1ull << (((z & 3u) << 4) | ((y & 3u) << 2) | (x & 3u));
                        const uint64_t cb = ((uint64_t)(z >> sh) * c->occ_nb[1] + (y >> sh)) * c->occ_nb[0] + (x >> sh);
                        coarse[cb >> 5] |= 1u << (cb & 31);
                    }
                }
        HIP_TRY(copy_sync(c->d_occ, coarse.data(), 4ull * c->occ_words, hipMemcpyHostToDevice, c->stream));
        if (!occx_possible) {
            c->occx_ok = false;
            const int rc = context_sat(c);
            if (rc != ZRT_OK) return rc;
            return context_counters(c);
        }
        HIP_TRY(hipMalloc((void**)&c->d_bmask, nb * 8));
        HIP_TRY(copy_sync(c->d_bmask, mask.data(), nb * 8, hipMemcpyHostToDevice, c->stream));
        std::vector<uint32_t> bits(nbw, 0u);
        std::vector<uint16_t> prefix(nbw, 0);
        std::vector<unsigned long long> masks;
        uint64_t run = 0;
        for (uint64_t wd = 0; wd < nbw; ++wd) {
            prefix[wd] = (uint16_t)std::min<uint64_t>(run + 1, 0xFFFF);
            for (uint64_t b = wd * 32; b < std::min<uint64_t>(nb, wd * 32 + 32); ++b)
                if (mask[b]) { bits[wd] |= 1u << (b & 31); masks.push_back(mask[b]); ++run; }
        }
        masks.insert(masks.begin(), 0ull);
        uint64_t moff, words;
        occx_layout(nbw, run, &moff, &words);
        c->occx_ok = occx_usable(nb, run, occx_lds_words(nbw, moff, words) * 4, kOccxBudget);
        if (c->occx_ok) {
            std::vector<uint32_t> blob(words, 0u);
            memcpy(blob.data(), bits.data(), nbw * 4);
            memcpy(blob.data() + nbw, prefix.data(), nbw * 2);
            memcpy(blob.data() + moff, masks.data(), masks.size() * 8);
            c->occx_words = (uint32_t)words;
            c->occx_nbw = (uint32_t)nbw;
            c->occx_moff = (uint32_t)moff;
            HIP_TRY(hipMalloc((void**)&c->d_occx, words * 4));
            HIP_TRY(copy_sync(c->d_occx, blob.data(), words * 4, hipMemcpyHostToDevice, c->stream));
        }
    } else if (!occx_possible) {
        HIP_TRY(hipMemsetAsync(c->d_occ, 0, 4ull * c->occ_words, c->stream));
        hipLaunchKernelGGL(occ_cells_kernel, dim3(4096), dim3(kBlock), 0, c->stream, c->d_cells, r[0], r[1], c->ncells,
                           sh, c->occ_nb[0], c->occ_nb[0] * c->occ_nb[1], c->d_occ);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(c->stream));
        c->occx_ok = false;
    } else {
        // the blob for the largest possible occupancy, then the real size
        uint64_t moff, words;
        occx_layout(nbw, nb, &moff, &words);
        // the scratch buffers are freed on every exit path (the blob belongs
        // to the context as soon as it exists)
        struct Scratch {
            uint32_t* n = nullptr;
            ~Scratch() {
                if (n) (void)hipFree(n);
            }
        } tmp;
        uint32_t* d_blob = nullptr;
        HIP_TRY(hipMalloc((void**)&c->d_bmask, nb * 8));   // the dense masks stay (TraceParams::bmask)
        HIP_TRY(hipMalloc((void**)&tmp.n, 4));
        HIP_TRY(hipMalloc((void**)&d_blob, words * 4));
        c->d_occx = d_blob;            // freed with the context from here on
        unsigned long long* const d_masks = c->d_bmask;
        uint32_t* const d_n = tmp.n;
        HIP_TRY(hipMemsetAsync(d_blob, 0, words * 4, c->stream));
        hipLaunchKernelGGL(occx_mask_kernel, dim3((uint32_t)((nb + kBlock - 1) / kBlock)), dim3(kBlock), 0, c->stream,
                           c->d_cells, r[0], r[1], r[2], c->occx_nb[0], c->occx_nb[1], (uint32_t)nb, d_masks, d_blob);
        hipLaunchKernelGGL(occx_pack_kernel, dim3(1), dim3(1024), 0, c->stream, (const uint32_t*)d_blob,
                           (uint32_t)nbw, (const unsigned long long*)d_masks,
                           reinterpret_cast<uint16_t*>(d_blob + nbw),
                           reinterpret_cast<unsigned long long*>(d_blob + moff), d_n);
        hipError_t le = hipGetLastError();
        if (sh == 2) {
            HIP_TRY(hipMemcpyAsync(c->d_occ, d_blob, nbw * 4, hipMemcpyDeviceToDevice, c->stream));
        } else if (sh < 2) {                   // (ZRT_OCC_SH0 builds) bricks finer than OccX's
            HIP_TRY(hipMemsetAsync(c->d_occ, 0, 4ull * c->occ_words, c->stream));
            hipLaunchKernelGGL(occ_cells_kernel, dim3(4096), dim3(kBlock), 0, c->stream, c->d_cells, r[0], r[1],
                               c->ncells, sh, c->occ_nb[0], c->occ_nb[0] * c->occ_nb[1], c->d_occ);
            if (le == hipSuccess) le = hipGetLastError();
        } else {
            HIP_TRY(hipMemsetAsync(c->d_occ, 0, 4ull * c->occ_words, c->stream));
            hipLaunchKernelGGL(occ_coarsen_kernel, dim3((uint32_t)((nb + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                               c->stream, (const uint32_t*)d_blob, c->occx_nb[0], c->occx_nb[1], (uint32_t)nb, sh - 2u,
                               c->occ_nb[0], c->occ_nb[0] * c->occ_nb[1], c->d_occ);
            if (le == hipSuccess) le = hipGetLastError();
        }
        uint32_t run = 0;
        HIP_TRY(hipMemcpyAsync(&run, d_n, 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        HIP_TRY(le);
        occx_layout(nbw, run, &moff, &words);
        c->occx_ok = occx_usable(nb, run, occx_lds_words(nbw, moff, words) * 4, kOccxBudget);
        c->occx_words = (uint32_t)words;
        c->occx_nbw = (uint32_t)nbw;
        c->occx_moff = (uint32_t)moff;
    }
    // (the escape table itself is built by the first render whose frame is
    // large enough to pay for it: context_escape)
    sc_occ.mark(c, "occupancy bits + OccX");
    const int rc = context_sat(c);
    sc_occ.mark(c, "summed-area table");
    if (rc != ZRT_OK) return rc;
    return context_counters(c);
}

extern "C" int zrt_context_create(const zrt_scene* s, int device, zrt_context** out) {
    if (!out) return ZRT_ERR_INVALID_ARG;
    *out = nullptr;
    int rc = validate_scene(s);
    if (rc != ZRT_OK) return rc;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return ZRT_ERR_NO_DEVICE;
    if (device < 0) {
        if (hipGetDevice(&device) != hipSuccess) return ZRT_ERR_NO_DEVICE;
    }
    if (device >= n) return ZRT_ERR_NO_DEVICE;
    DeviceGuard g(device);
    zrt_context* c = new (std::nothrow) zrt_context();
    if (!c) return ZRT_ERR_OUT_OF_MEMORY;
    c->device = device;
    rc = context_init(c, s);
    if (rc != ZRT_OK) { zrt_context_destroy(c); return rc; }
    *out = c;
    return ZRT_OK;
}

// Device-built context: Geometry.build + bakeInto (stage2.zig:44-164) on the
// GPU straight into the context's arrays (grid_build.hip), no host copy of the
// baked scene.  Same render results as zrt_geometry_build + zrt_context_create.
extern "C" int zrt_context_create_built(const float* positions, const float* normals, const float* texcoords,
                                        const uint32_t* material, uint32_t num_triangles,
                                        const uint32_t resolution[3], uint32_t num_materials,
                                        const zrt_material* materials, const float* texels,
                                        uint64_t num_texel_floats, int device, zrt_context** out) {
    if (!out) return ZRT_ERR_INVALID_ARG;
    *out = nullptr;
    if (!material) return ZRT_ERR_INVALID_ARG;
    zrt_scene ms{};
    ms.num_materials = num_materials;
    ms.materials = materials;
    ms.texels = texels;
    ms.num_texel_floats = num_texel_floats;
    int rc = validate_materials(&ms);
    if (rc != ZRT_OK) return rc;
    for (uint32_t i = 0; i < num_triangles; ++i)
        if (material[i] >= num_materials) return ZRT_ERR_INVALID_ARG;
    if (num_triangles && !positions) return ZRT_ERR_INVALID_ARG;
    // vertex components of 2^61 or more (or infinite) may give edge
    // components of 2^62 or more: the IEEE-division kernels (mt_exact)
    const bool mt_exact = needs_mt_exact(positions, 9ull * num_triangles, 1u, 0u, 0x1p61f);
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return ZRT_ERR_NO_DEVICE;
    if (device < 0) {
        if (hipGetDevice(&device) != hipSuccess) return ZRT_ERR_NO_DEVICE;
    }
    if (device >= n) return ZRT_ERR_NO_DEVICE;
    DeviceGuard g(device);
    zrt_context* c = new (std::nothrow) zrt_context();
    if (!c) return ZRT_ERR_OUT_OF_MEMORY;
    c->device = device;
    c->mt_exact = mt_exact;
    StageClock sc;
    rc = context_base(c);
    if (rc == ZRT_OK) {
        sc.mark(c, "stream + device properties");
        zrt::Grid grid;
        DeviceGeometry dg;
        rc = grid_build_into_device(positions, normals, texcoords, material, num_triangles, resolution, c->stream,
                                    &grid, &dg);
        if (rc == ZRT_OK) sc.mark(c, "grid build + bake (grid_build.hip)");
        if (rc == ZRT_OK) {
            for (int i = 0; i < 3; ++i) {
                c->grid.bbox_min[i] = (&grid.bbox.min.x)[i];
                c->grid.bbox_max[i] = (&grid.bbox.max.x)[i];
                c->grid.resolution[i] = grid.res[i];
                c->grid.cell_size[i] = (&grid.cell_size.x)[i];
            }
            c->ncells = resolution[0] * resolution[1] * resolution[2];
            c->nrefs = dg.refs;
            c->d_cells = dg.cells;
            c->d_data = dg.data;               // the context owns both from here (freed by destroy)
            c->d_pos = reinterpret_cast<float*>(dg.pos);   // the device bake's 3 float4 per ref
            if (rc == ZRT_OK && (rc = context_materials(c, &ms)) == ZRT_OK) {
                sc.mark(c, "materials + texels");
                rc = context_occupancy(c, nullptr);
            }
        }
    }
    if (rc != ZRT_OK) { zrt_context_destroy(c); return rc; }
    *out = c;
    return ZRT_OK;
}

// Empty cells and min/max refs of the non-empty ones (the CLI's grid log,
// main.zig:117-118 + stage2 logging), reduced on the device.
__global__ __launch_bounds__(kBlock) void grid_info_kernel(const uint2* __restrict__ cells, uint32_t ncells,
                                                           uint32_t* __restrict__ out) {
    uint32_t empty = 0, mn = 0xFFFFFFFFu, mx = 0;
    for (uint32_t ci = blockIdx.x * kBlock + threadIdx.x; ci < ncells; ci += gridDim.x * kBlock) {
        const uint2 c = cells[ci];
        const uint32_t k = c.y - c.x;
        if (!k) ++empty;
        else { mn = min(mn, k); mx = max(mx, k); }
    }
    for (int o = 32; o > 0; o >>= 1) {
        empty += __shfl_xor(empty, o);
        mn = min(mn, (uint32_t)__shfl_xor(mn, o));
        mx = max(mx, (uint32_t)__shfl_xor(mx, o));
    }
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&out[0], empty);
        atomicMin(&out[1], mn);
        atomicMax(&out[2], mx);
    }
}

extern "C" int zrt_context_grid_info(zrt_context* c, zrt_grid* grid, uint32_t info[4]) {
    if (!c || !info) return ZRT_ERR_INVALID_ARG;
    DeviceGuard g(c->device);
    if (grid) *grid = c->grid;
    uint32_t h[3] = {0u, 0xFFFFFFFFu, 0u};
    HIP_TRY(hipMemcpyAsync(c->d_counter, h, sizeof h, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(grid_info_kernel, dim3(std::min<uint32_t>((c->ncells + kBlock - 1) / kBlock, 2048)),
                       dim3(kBlock), 0, c->stream, c->d_cells, c->ncells, c->d_counter);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h, c->d_counter, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    info[0] = c->nrefs;
    info[1] = h[0];
    info[2] = h[1];
    info[3] = h[2];
    return ZRT_OK;
}

void* zrt::context_stream(const zrt_context* c) { return c ? (void*)c->stream : nullptr; }

void zrt::context_set_mem_share(zrt_context* c, uint32_t share) {
    if (c) c->mem_share = std::max<uint32_t>(share, 1u);
}

int zrt::context_device_rgb(const zrt_context* c, const uint8_t** d_rgb, uint32_t* pixels, int* device) {
    if (!c || !d_rgb || !pixels || !device) return ZRT_ERR_INVALID_ARG;
    *d_rgb = c->d_rgb;
    *pixels = c->pix_valid ? (uint32_t)c->pix.size() : 0u;
    *device = c->device;
    return ZRT_OK;
}

// Start-up work of the first GPU call, done ahead: the device's context and
// the code objects of render.hip, grid_build.hip and this unit (loaded on first
// use: ~0.1-0.2 s on MI355X).  Lets a host overlap it with file loading.
extern "C" int zrt_device_warmup(int device) {
    // ZRT_TIMING: the split of the HIP start-up (runtime initialisation,
    // device context, the three code objects) on stderr
    const bool timing = getenv("ZRT_TIMING") != nullptr;
    const double t0 = StageClock::now_ms();
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return ZRT_ERR_NO_DEVICE;
    const double t1 = StageClock::now_ms();
    if (device < 0) device = 0;
    if (device >= n) return ZRT_ERR_NO_DEVICE;
    DeviceGuard g(device);
    HIP_TRY(hipFree(nullptr));
    const double t2 = StageClock::now_ms();
    int rc = render_warmup();
    if (rc != ZRT_OK) return rc;
    const double t3 = StageClock::now_ms();
    rc = grid_build_warmup();
    const double t4 = StageClock::now_ms();
    hipFuncAttributes fa;
    if (rc == ZRT_OK) HIP_TRY(hipFuncGetAttributes(&fa, (const void*)grid_info_kernel));
    if (timing)
        fprintf(stderr, "timing: warm-up: runtime init (hipGetDeviceCount) %.3f ms, device context %.3f ms, "
                "render.hip code object %.3f ms, grid_build.hip code object %.3f ms, "
                "context.hip code object %.3f ms\n",
                t1 - t0, t2 - t1, t3 - t2, t4 - t3, StageClock::now_ms() - t4);
    return rc;
}
