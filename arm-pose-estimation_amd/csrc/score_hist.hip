// The shape of the errors: counts of per-frame values over fixed edges, per recording and column (ape_score_hist; the
// reference has no counterpart).  Any rows that lie on the device -- score rows [F, 7], a lag sweep's [F, L, 7], motion rows [C, F, 12],
// strided views -- against one list of recordings with a window each; include/ape_hip.h states the slots.
//
// ape_score_hist_kernel  grid (tiles x column chunks, groups, sets), 256 frames per workgroup, one lane per frame.  A workgroup takes up
//                        to 8 columns of its rows (a wider row is split into equal chunks, the chunks of a tile next to each other in
//                        the grid so that they meet in L2): the edges of its columns go to LDS, each wave stages its 64 rows at an odd
//                        stride (score_device.h's stage_rows), and a lane finds the slot of each of its values by binary search over the
//                        edges in LDS, at most 9 compares.
//
// Counts: neighbouring lanes of a wave with the same recording and slot are one run; the run's first lane adds the run's length, the
// others nothing (a shuffle, a ballot and a find-first-set per column: consecutive frames of a replay mostly share a bin, and 64 adds to
// one address would serialise -- DESIGN.md 4.40 has both forms' figures).  A tile that holds frames of at most 4 recordings goes
// recording by recording: the recording's run heads add to a 32-bit LDS histogram, and the non-zero counts go to the output with one
// 64-bit atomic add each.  A tile with more recordings than that has at most 64 frames per recording on average and little to sum on
// chip: its run heads add to the output directly, and the LDS histogram is neither zeroed nor flushed.  The output is zeroed on the
// stream in front of the kernel.  Integer adds: the bits do not depend on the order.  No inline assembly.
#include "ape_internal.h"
#include "../../include/ape_hip.h"
#include "bank_host.h"
#include "score_host.h"

#include <cmath>
#include <cstdio>
#include <cstring>

#pragma clang fp contract(off)
#include "score_device.h"

namespace {

using namespace ape_scoredev;

constexpr int SH_BLOCK = 256, SH_WAVES = SH_BLOCK / 64;
constexpr int SH_CW = 8;                                // columns of a workgroup at most
constexpr int SH_LDS_RECS = 4;                          // recordings of a tile up to which the counts go through the LDS histogram

static_assert(SH_CW <= STAGE_COLS, "stage_rows' rounds cover a chunk");
static_assert(APE_HIST_MAX_WIDTH <= 2 * SH_CW, "at most two chunks: (chunks - 1) * cw < width");

struct HistParams {
    const void* values;
    const int* starts;                                  // [R]
    const int* trim;                                    // [R, 2]
    const double* edges;                                // [W, B + 1]
    unsigned long long* hist;                           // [n_sets, R, G, W, B + 3]
    long long set_stride, frame_stride, group_stride;
    int F, R, G, W, B, chunks, cw;
};

// doubles of LDS in front of the histogram: the edges of a chunk, then the waves' staging blocks
__host__ __device__ constexpr int sh_stage_at(int cw, int B) { return cw * (B + 1); }
__host__ __device__ constexpr int sh_hist_at(int cw, int B) { return sh_stage_at(cw, B) + SH_WAVES * 64 * (cw | 1); }
__host__ __device__ constexpr size_t sh_lds_bytes(int cw, int B) { return (size_t)sh_hist_at(cw, B) * sizeof(double) + (size_t)cw * (B + 3) * sizeof(unsigned); }
static_assert(sh_lds_bytes(SH_CW, APE_HIST_MAX_BINS) <= 64 * 1024, "the largest workgroup's LDS");

template <typename T>
__global__ __launch_bounds__(SH_BLOCK) void ape_score_hist_kernel(const HistParams p) {
    extern __shared__ double sh_mem[];                  // edges [ncols][B + 1] | staging [4][64][lstride] | counts u32 [ncols][B + 3]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int chunk = (int)(blockIdx.x % (unsigned)p.chunks), g = blockIdx.y, set = blockIdx.z;
    const long long tile0 = (long long)(blockIdx.x / (unsigned)p.chunks) * SH_BLOCK;
    const int c0 = chunk * p.cw;
    const int ncols = p.W - c0 < p.cw ? p.W - c0 : p.cw;
    const int lstride = ncols | 1, nb1 = p.B + 1, ns = p.B + 3;
    double* ledges = sh_mem;
    double* stage = sh_mem + sh_stage_at(p.cw, p.B) + wave * 64 * (p.cw | 1);
    unsigned* counts = reinterpret_cast<unsigned*>(sh_mem + sh_hist_at(p.cw, p.B));

    const long long row0 = tile0 + wave * 64;
    const long long f = row0 + lane;
    const bool valid = f < p.F;
    const long long left = (long long)p.F - row0;
    const int nrows = left >= 64 ? 64 : (left > 0 ? (int)left : 0);

    // the recordings of the tile's first and last frame: two searches with a uniform argument, so once per wave and through the scalar
    // cache, not a chain of vector loads per lane.  (tile0 < F: the grid has no tile past the rows)
    const long long last = tile0 + SH_BLOCK - 1 < (long long)p.F - 1 ? tile0 + SH_BLOCK - 1 : (long long)p.F - 1;
    const int first = find_rec(p.starts, p.R, tile0), nrec = find_rec(p.starts, p.R, last) - first + 1;
    // the frame's recording -- searched for among the tile's only, and not at all where the tile has one -- and whether the frame lies in
    // the recording's window
    int rec = first;
    bool in = false;
    if (valid) {
        int hi = first + nrec - 1;
        while (rec < hi) {
            const int mid = (rec + hi + 1) >> 1;
            if ((long long)p.starts[mid] <= f) rec = mid; else hi = mid - 1;
        }
        const long long lo = (long long)p.starts[rec] + p.trim[2 * rec];
        const long long up = (long long)(rec + 1 < p.R ? p.starts[rec + 1] : p.F) - p.trim[2 * rec + 1];
        in = f >= lo && f < up;
    }

    const int nedges = ncols * nb1;
    const double* esrc = p.edges + (size_t)c0 * nb1;
    for (int i = threadIdx.x; i < nedges; i += SH_BLOCK) ledges[i] = esrc[i];
    const long long base = (p.G > 1 ? (long long)g * p.group_stride : 0) + c0;
    const T* src = static_cast<const T*>(p.values) + (long long)set * p.set_stride + base;
    if (nrows > 0) stage_rows(stage, src, p.frame_stride, ncols, lstride, row0, nrows, lane);
    __syncthreads();

    int slot[SH_CW];
#pragma unroll
    for (int c = 0; c < SH_CW; ++c) slot[c] = (in && c < ncols) ? find_slot(ledges + c * nb1, p.B, stage[lane * lstride + c]) : 0;

    // what a lane adds: the length of the run of equal (recording, slot) that it heads, 0 inside a run
    unsigned cnt[SH_CW];
    {
        const int prec = __shfl_up(rec, 1, 64), pin = __shfl_up((int)in, 1, 64);
        const bool brk = lane == 0 || prec != rec || pin != (int)in;
#pragma unroll
        for (int c = 0; c < SH_CW; ++c) {
            const int ps = __shfl_up(slot[c], 1, 64);
            const bool head = brk || ps != slot[c];
            const unsigned long long heads = __ballot(head);
            const unsigned long long above = lane < 63 ? heads >> (lane + 1) : 0ull;    // the next head above the lane, or the wave's end
            const int len = above ? __ffsll((long long)above) : 64 - lane;
            cnt[c] = (in && head && c < ncols) ? (unsigned)len : 0u;
        }
    }
    // row [set][r][g][c0] of the output
    const size_t rec_step = (size_t)p.G * (size_t)p.W * (size_t)ns;
    unsigned long long* out0 = p.hist + (((size_t)set * (size_t)p.R * (size_t)p.G + (size_t)g) * (size_t)p.W + (size_t)c0) * (size_t)ns;
    const int ncounts = ncols * ns;

    if (nrec > SH_LDS_RECS) {                           // (uniform) many short recordings: nothing worth summing on chip
        if (in) {
            unsigned long long* dst = out0 + (size_t)rec * rec_step;
#pragma unroll
            for (int c = 0; c < SH_CW; ++c)
                if (cnt[c] != 0u) atomicAdd(dst + c * ns + slot[c], (unsigned long long)cnt[c]);
        }
        return;
    }
    for (int r = first; r < first + nrec; ++r) {        // (uniform)
        for (int i = threadIdx.x; i < ncounts; i += SH_BLOCK) counts[i] = 0u;
        __syncthreads();
        if (in && rec == r) {
#pragma unroll
            for (int c = 0; c < SH_CW; ++c)
                if (cnt[c] != 0u) atomicAdd(counts + c * ns + slot[c], cnt[c]);
        }
        __syncthreads();
        unsigned long long* dst = out0 + (size_t)r * rec_step;
        for (int i = threadIdx.x; i < ncounts; i += SH_BLOCK) {
            const unsigned v = counts[i];
            if (v != 0u) atomicAdd(dst + i, (unsigned long long)v);
        }
        __syncthreads();                                // (the counts are read before the next recording zeroes them)
    }
}

// the staging of a call: starts, trims and edges (score_host.h)
ApeSlotPool g_pool("score_hist");

}  // namespace

int ape_score_hist(const void* values_dev, int32_t values_dtype, int32_t width, int32_t n_sets, int64_t set_stride, int32_t F,
                   int64_t frame_stride, int32_t n_groups, int64_t group_stride, const int32_t* seg_starts_host, int32_t R,
                   const int32_t* trim_host, const double* edges_host, int32_t n_bins, int64_t* hist_dev, void* stream) {
    const char* who = "score_hist";
    if (!values_dev || !seg_starts_host || !edges_host || !hist_dev) return ape_fail(APE_ERR_INVALID_ARG, "%s: NULL argument", who);
    if (values_dtype != APE_F32 && values_dtype != APE_F64) return ape_fail(APE_ERR_INVALID_ARG, "%s: unknown dtype selector %d", who, values_dtype);
    if (int rc = ape_check_segments(who, F, seg_starts_host, R)) return rc;
    if (trim_host)
        for (int r = 0; r < R; ++r)
            if (trim_host[2 * r] < 0 || trim_host[2 * r + 1] < 0)
                return ape_fail(APE_ERR_INVALID_ARG, "%s: trim[%d] = (%d, %d) is negative", who, r, trim_host[2 * r], trim_host[2 * r + 1]);
    if (width < 1 || width > APE_HIST_MAX_WIDTH) return ape_fail(APE_ERR_INVALID_ARG, "%s: width %d, between 1 and %d", who, width, APE_HIST_MAX_WIDTH);
    if (n_bins < 1 || n_bins > APE_HIST_MAX_BINS) return ape_fail(APE_ERR_INVALID_ARG, "%s: n_bins %d, between 1 and %d", who, n_bins, APE_HIST_MAX_BINS);
    if (n_sets < 1 || n_sets > APE_POST_MAX_CONFIGS)
        return ape_fail(APE_ERR_INVALID_ARG, "%s: n_sets %d, between 1 and %d", who, n_sets, APE_POST_MAX_CONFIGS);
    if (n_groups < 1 || n_groups > APE_SCORE_MAX_LAGS)
        return ape_fail(APE_ERR_INVALID_ARG, "%s: n_groups %d, between 1 and %d", who, n_groups, APE_SCORE_MAX_LAGS);
    if (frame_stride < width) return ape_fail(APE_ERR_INVALID_ARG, "%s: frame_stride %lld below the width %d", who, (long long)frame_stride, width);
    if (n_groups > 1 && group_stride < width)
        return ape_fail(APE_ERR_INVALID_ARG, "%s: group_stride %lld below the width %d", who, (long long)group_stride, width);
    // the last element read, in elements from values_dev: every stride is positive from here on
    long long extent = 0, term = 0;
    bool fits = !__builtin_mul_overflow((long long)(F - 1), (long long)frame_stride, &extent);
    if (n_groups > 1) fits = fits && !__builtin_mul_overflow((long long)(n_groups - 1), (long long)group_stride, &term) && !__builtin_add_overflow(extent, term, &extent);
    if (n_sets > 1) {
        long long rows = 0;
        if (__builtin_mul_overflow((long long)F, (long long)frame_stride, &rows) || set_stride < rows)
            return ape_fail(APE_ERR_INVALID_ARG, "%s: set_stride %lld below F * frame_stride", who, (long long)set_stride);
        fits = fits && !__builtin_mul_overflow((long long)(n_sets - 1), (long long)set_stride, &term) && !__builtin_add_overflow(extent, term, &extent);
    }
    const long long esize = values_dtype == APE_F32 ? 4 : 8;
    fits = fits && !__builtin_add_overflow(extent, (long long)width, &extent) && !__builtin_mul_overflow(extent, esize, &extent);
    if (!fits) return ape_fail(APE_ERR_INVALID_ARG, "%s: the extent of the values does not fit 63 bits", who);
    if (((uintptr_t)values_dev & (uintptr_t)(esize - 1)) || ((uintptr_t)hist_dev & 7u))
        return ape_fail(APE_ERR_INVALID_ARG, "%s: a pointer is not aligned to its element", who);
    for (int w = 0; w < width; ++w) {
        const double* e = edges_host + (size_t)w * (size_t)(n_bins + 1);
        for (int i = 0; i <= n_bins; ++i)
            if (!std::isfinite(e[i]) || (i > 0 && !(e[i] > e[i - 1])))
                return ape_fail(APE_ERR_INVALID_ARG, "%s: edges[%d][%d] = %g (finite and strictly increasing)", who, w, i, e[i]);
    }
    const long long out_elems = (long long)n_sets * R * n_groups * width * (n_bins + 3);      // (at most 64 * 2^31 * 65 * 16 * 259 < 2^63)
    if (out_elems > 2147483647LL) return ape_fail(APE_ERR_INVALID_ARG, "%s: %lld output elements, at most 2^31 - 1", who, out_elems);
    const uintptr_t va = (uintptr_t)values_dev, ha = (uintptr_t)hist_dev;
    const uintptr_t vb = va + (uintptr_t)extent, hb = ha + (uintptr_t)out_elems * sizeof(int64_t);
    if (va < hb && ha < vb) return ape_fail(APE_ERR_INVALID_ARG, "%s: hist_dev overlaps values_dev", who);
    const hipStream_t st = (hipStream_t)stream;
    if (int rc = ape_check_not_capturing(st, who, "host arrays are staged per call")) return rc;
    int device = 0;
    APE_SCORE_TRY(g_pool.prefix, hipGetDevice(&device));

    const size_t ints_bytes = (((size_t)R * 3 * sizeof(int)) + 7) & ~(size_t)7;          // starts [R], trims [R, 2]; then the edges
    const size_t edges_bytes = (size_t)width * (size_t)(n_bins + 1) * sizeof(double);
    const size_t host_bytes = ints_bytes + edges_bytes;

    std::lock_guard<std::mutex> lock(g_pool.mu);
    ApeSlot* slot = nullptr;
    if (int rc = g_pool.take(device, host_bytes, host_bytes, &slot)) return rc;
    char* pin = static_cast<char*>(slot->pinned);
    memcpy(pin, seg_starts_host, (size_t)R * sizeof(int));
    if (trim_host) memcpy(pin + (size_t)R * sizeof(int), trim_host, (size_t)R * 2 * sizeof(int));
    else memset(pin + (size_t)R * sizeof(int), 0, (size_t)R * 2 * sizeof(int));
    memcpy(pin + ints_bytes, edges_host, edges_bytes);
    // (a copy that fails leaves through finish() like a launch that fails: the slot's event is recorded either way)
    hipError_t e = hipMemcpyAsync(slot->dev, slot->pinned, host_bytes, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemsetAsync(hist_dev, 0, (size_t)out_elems * sizeof(int64_t), st);
    if (e != hipSuccess) return g_pool.finish(who, slot, e, st);

    HistParams p{};
    char* dev = static_cast<char*>(slot->dev);
    p.values = values_dev;
    p.starts = reinterpret_cast<const int*>(dev);
    p.trim = p.starts + R;
    p.edges = reinterpret_cast<const double*>(dev + ints_bytes);
    p.hist = reinterpret_cast<unsigned long long*>(hist_dev);
    p.set_stride = n_sets > 1 ? (long long)set_stride : 0; p.frame_stride = frame_stride; p.group_stride = n_groups > 1 ? (long long)group_stride : 0;
    p.F = F; p.R = R; p.G = n_groups; p.W = width; p.B = n_bins;
    p.chunks = (width + SH_CW - 1) / SH_CW;
    p.cw = (width + p.chunks - 1) / p.chunks;

    const unsigned tiles = (unsigned)(((long long)F + SH_BLOCK - 1) / SH_BLOCK);
    const dim3 grid(tiles * (unsigned)p.chunks, (unsigned)n_groups, (unsigned)n_sets);
    const size_t lds = sh_lds_bytes(p.cw, n_bins);
    if (values_dtype == APE_F32) hipLaunchKernelGGL(ape_score_hist_kernel<float>, grid, dim3(SH_BLOCK), lds, st, p);
    else hipLaunchKernelGGL(ape_score_hist_kernel<double>, grid, dim3(SH_BLOCK), lds, st, p);
    return g_pool.finish(who, slot, hipGetLastError(), st);
}
