// Errors by condition: per-slot count, sum, sum of squares and maximum of any per-frame column keyed by any other (ape_score_by;
// DESIGN.md 4.42; the reference has no counterpart).  Keys and values are any rows that lie on the device -- joint angles [C, F, 7],
// score rows [F, 7], motion rows [C, F, 12], the sigmas of the spread record, strided views -- against one list of recordings with a
// window each; include/ape_hip.h states the slots, the cells and the ORDER of every sum, which is part of the contract.
//
// ape_score_by_kernel  grid (pieces, key columns, sets), 256 threads.  A piece is APE_BY_PIECE = 1024 consecutive frames of one
//                      recording's window, counted from the window's first frame; the workgroup finds its recording by a search over the
//                      recordings' first pieces.  It takes the piece in sub-tiles of 256 frames: a lane per frame finds the slot of its
//                      key by binary search over the column's edges in LDS (at most 7 compares) and the waves stage their 64 value rows
//                      at an odd stride (score_device.h's stage_rows).  Then the four waves split the value columns (wave w: columns w,
//                      w + 4, ...), a lane owns the slots `lane` and `lane + 64`, and walks the sub-tile's frames in order with its
//                      accumulators in registers: every read of LDS is a broadcast, no lane waits for another, and the order of a
//                      cell's terms is the frames'.  A frame that is not the lane's adds +0.0, which a sum that started at +0.0 cannot
//                      see (such a sum is never -0.0), so there is no branch.  The piece's record goes to the staging slot's device block.
// ape_score_by_fold    grid (recordings x chunks of 256 accumulators, key columns, sets): the piece records of a recording in piece
//                      order, from +0.0 (the maxima from -inf).  A recording without a window gets its zeros and -inf here: the call
//                      writes all of by_dev with no memset.
// No atomics, no workgroup waits for another, no inline assembly.
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

constexpr int SB_BLOCK = 256, SB_WAVES = SB_BLOCK / 64;
constexpr int SB_TILE = SB_BLOCK;                       // frames of a sub-tile: a lane per frame
constexpr int SB_WCOLS = APE_BY_MAX_VALUES / SB_WAVES;  // value columns of a wave at most
constexpr long long SB_MAX_PART_BYTES = 1LL << 30;

static_assert(APE_BY_PIECE % SB_TILE == 0, "whole sub-tiles but the last");
static_assert(APE_BY_MAX_BINS + 3 <= 128, "two slots per lane");
static_assert(APE_BY_MAX_VALUES <= STAGE_COLS && APE_BY_MAX_VALUES % SB_WAVES == 0, "stage_rows' rounds cover a row; the waves' share");

struct ByParams {
    const void* keys;
    const void* values;
    const int* win_lo;                                  // [R] first frame of the window
    const int* win_len;                                 // [R] frames of the window (0: none)
    const int* piece_at;                                // [R + 1] first piece of the recording; [R] = P
    const double* edges;                                // [K, B + 1]
    double* part;                                       // [n_sets, P, K, B + 3, V, 4]
    double* by;                                         // [n_sets, R, K, B + 3, V, 4]
    long long kset, kframe, vset, vframe;
    int R, K, V, B, P;
};

// doubles of LDS: the edges of the column, then the sub-tile's value rows; the slots (int) behind them
__host__ __device__ constexpr int sb_vals_at(int B) { return B + 1; }
__host__ __device__ constexpr int sb_slots_at(int B, int V) { return sb_vals_at(B) + SB_TILE * (V | 1); }
__host__ __device__ constexpr size_t sb_lds_bytes(int B, int V) { return (size_t)sb_slots_at(B, V) * sizeof(double) + SB_TILE * sizeof(int); }
static_assert(sb_lds_bytes(APE_BY_MAX_BINS, APE_BY_MAX_VALUES) <= 40 * 1024, "four workgroups per CU by LDS at the limits");

// what a lane holds: per value column of its wave and per slot it owns, the count and the three floating accumulators
template <int S>
struct ByAcc {
    int n[SB_WCOLS][S];
    double s[SB_WCOLS][S], q[SB_WCOLS][S], m[SB_WCOLS][S];
};

// frames 0 .. nt - 1 of the sub-tile in order, NV columns v0, v0 + SB_WAVES, ...
template <int NV, int S>
__device__ __forceinline__ void walk(ByAcc<S>& a, const int* slots, const double* vals, int lstride, int v0, int nt, int lane) {
#pragma unroll 4
    for (int t = 0; t < nt; ++t) {
        const int sl = slots[t];                        // (uniform addresses: broadcasts)
        const double* row = vals + t * lstride + v0;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const double x = row[i * SB_WAVES];
            const double xx = x * x;                    // rounded here, added below
            const bool ok = x == x;
#pragma unroll
            for (int j = 0; j < S; ++j) {
                const bool hit = ok && sl == lane + 64 * j;
                a.n[i][j] += hit ? 1 : 0;
                a.s[i][j] = a.s[i][j] + (hit ? x : 0.0);
                a.q[i][j] = a.q[i][j] + (hit ? xx : 0.0);
                a.m[i][j] = (hit && x > a.m[i][j]) ? x : a.m[i][j];
            }
        }
    }
}

template <typename TK, typename TV, int S>
__global__ __launch_bounds__(SB_BLOCK) void ape_score_by_kernel(const ByParams p) {
    extern __shared__ double sb_mem[];                  // edges [B + 1] | values [256][V | 1] | slots int [256]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int piece = blockIdx.x, k = blockIdx.y, set = blockIdx.z;
    const int lstride = p.V | 1, ns = p.B + 3;
    double* ledges = sb_mem;
    double* vals = sb_mem + sb_vals_at(p.B);
    int* slots = reinterpret_cast<int*>(sb_mem + sb_slots_at(p.B, p.V));

    // the piece's recording: the last whose first piece is <= piece (a recording without pieces shares its successor's and is passed over)
    const int r = find_rec(p.piece_at, p.R, piece);
    const int j0 = piece - p.piece_at[r];
    const long long f0 = (long long)p.win_lo[r] + (long long)j0 * APE_BY_PIECE;
    const int left = p.win_len[r] - j0 * APE_BY_PIECE;  // >= 1
    const int n = left < APE_BY_PIECE ? left : APE_BY_PIECE;

    for (int i = threadIdx.x; i <= p.B; i += SB_BLOCK) ledges[i] = p.edges[(size_t)k * (p.B + 1) + i];
    const TK* ksrc = static_cast<const TK*>(p.keys) + (long long)set * p.kset + k;
    const TV* vsrc = static_cast<const TV*>(p.values) + (long long)set * p.vset;

    ByAcc<S> a;
#pragma unroll
    for (int i = 0; i < SB_WCOLS; ++i)
#pragma unroll
        for (int j = 0; j < S; ++j) { a.n[i][j] = 0; a.s[i][j] = 0.0; a.q[i][j] = 0.0; a.m[i][j] = -INFINITY; }
    const int nv = wave < p.V ? (p.V - wave + SB_WAVES - 1) / SB_WAVES : 0;      // (wave-uniform) columns wave, wave + 4, ...

    for (int t0 = 0; t0 < n; t0 += SB_TILE) {           // (uniform)
        const int nt = n - t0 < SB_TILE ? n - t0 : SB_TILE;
        __syncthreads();                                // the edges are written; the last sub-tile has been walked
        const int nrows = nt - wave * 64 >= 64 ? 64 : nt - wave * 64;
        if (nrows > 0) stage_rows(vals + wave * 64 * lstride, vsrc, p.vframe, p.V, lstride, f0 + t0 + wave * 64, nrows, lane);
        if ((int)threadIdx.x < nt) slots[threadIdx.x] = find_slot(ledges, p.B, (double)ksrc[(f0 + t0 + threadIdx.x) * p.kframe]);
        __syncthreads();
        switch (nv) {                                   // (wave-uniform; no barrier inside)
            case 1: walk<1, S>(a, slots, vals, lstride, wave, nt, lane); break;
            case 2: walk<2, S>(a, slots, vals, lstride, wave, nt, lane); break;
            case 3: walk<3, S>(a, slots, vals, lstride, wave, nt, lane); break;
            case 4: walk<4, S>(a, slots, vals, lstride, wave, nt, lane); break;
            default: break;
        }
    }

    // record [set][piece][k][slot][v][0 .. 3]
    double* rec = p.part + (((size_t)set * (size_t)p.P + (size_t)piece) * (size_t)p.K + (size_t)k) * (size_t)ns * (size_t)p.V * 4;
#pragma unroll
    for (int i = 0; i < SB_WCOLS; ++i) {
        if (i < nv) {
#pragma unroll
            for (int j = 0; j < S; ++j) {
                const int slot = lane + 64 * j;
                if (slot < ns) {
                    double* dst = rec + ((size_t)slot * p.V + (wave + i * SB_WAVES)) * 4;
                    dst[0] = (double)a.n[i][j]; dst[1] = a.s[i][j]; dst[2] = a.q[i][j]; dst[3] = a.m[i][j];
                }
            }
        }
    }
}

__global__ __launch_bounds__(SB_BLOCK) void ape_score_by_fold(const ByParams p, int chunks) {
    const int chunk = (int)(blockIdx.x % (unsigned)chunks), r = (int)(blockIdx.x / (unsigned)chunks), k = blockIdx.y, set = blockIdx.z;
    const int cells = (p.B + 3) * p.V * 4;
    const int e = chunk * SB_BLOCK + threadIdx.x;
    if (e >= cells) return;
    const int p0 = p.piece_at[r], p1 = p.piece_at[r + 1];
    const bool is_max = (e & 3) == 3;
    const size_t step = (size_t)p.K * (size_t)cells;
    const double* src = p.part + (((size_t)set * (size_t)p.P + (size_t)p0) * (size_t)p.K + (size_t)k) * (size_t)cells + e;
    double acc = is_max ? -INFINITY : 0.0;
#pragma unroll 4
    for (int i = p0; i < p1; ++i, src += step) {        // in piece order
        const double x = *src;
        acc = is_max ? (x > acc ? x : acc) : acc + x;
    }
    p.by[(((size_t)set * (size_t)p.R + (size_t)r) * (size_t)p.K + (size_t)k) * (size_t)cells + e] = acc;
}

// the staging of a call: windows, first pieces and edges, and behind them the piece records (score_host.h)
ApeSlotPool g_pool("score_by");

// One side's checks; *extent: bytes from the side's pointer to the end of the last element read
int check_side(const char* who, const char* side, const void* dev, int32_t dtype, int32_t width, int32_t max_width, int32_t n_sets,
               int64_t set_stride, int32_t F, int64_t frame_stride, long long* extent) {
    if (dtype != APE_F32 && dtype != APE_F64) return ape_fail(APE_ERR_INVALID_ARG, "%s: unknown %s dtype selector %d", who, side, dtype);
    if (width < 1 || width > max_width) return ape_fail(APE_ERR_INVALID_ARG, "%s: n_%s %d, between 1 and %d", who, side, width, max_width);
    if (frame_stride < width)
        return ape_fail(APE_ERR_INVALID_ARG, "%s: %s_frame_stride %lld below the %d columns", who, side, (long long)frame_stride, width);
    long long ext = 0, term = 0;
    bool fits = !__builtin_mul_overflow((long long)(F - 1), (long long)frame_stride, &ext);
    if (n_sets > 1 && set_stride != 0) {
        long long rows = 0;
        if (__builtin_mul_overflow((long long)F, (long long)frame_stride, &rows) || set_stride < rows)
            return ape_fail(APE_ERR_INVALID_ARG, "%s: %s_set_stride %lld is neither 0 (shared) nor at least F * frame_stride", who, side,
                            (long long)set_stride);
        fits = fits && !__builtin_mul_overflow((long long)(n_sets - 1), (long long)set_stride, &term) && !__builtin_add_overflow(ext, term, &ext);
    }
    const long long esize = dtype == APE_F32 ? 4 : 8;
    fits = fits && !__builtin_add_overflow(ext, (long long)width, &ext) && !__builtin_mul_overflow(ext, esize, &ext);
    if (!fits) return ape_fail(APE_ERR_INVALID_ARG, "%s: the extent of the %s does not fit 63 bits", who, side);
    if ((uintptr_t)dev & (uintptr_t)(esize - 1)) return ape_fail(APE_ERR_INVALID_ARG, "%s: %s_dev is not aligned to its element", who, side);
    *extent = ext;
    return APE_OK;
}

template <typename TK, typename TV>
void launch_by(const ByParams& p, dim3 grid, size_t lds, hipStream_t st) {
    if (p.B + 3 <= 64) hipLaunchKernelGGL((ape_score_by_kernel<TK, TV, 1>), grid, dim3(SB_BLOCK), lds, st, p);
    else hipLaunchKernelGGL((ape_score_by_kernel<TK, TV, 2>), grid, dim3(SB_BLOCK), lds, st, p);
}

}  // namespace

int ape_score_by(const void* keys_dev, int32_t keys_dtype, int32_t n_keys, int64_t keys_set_stride, int64_t keys_frame_stride,
                 const void* values_dev, int32_t values_dtype, int32_t n_values, int64_t values_set_stride, int64_t values_frame_stride,
                 int32_t n_sets, int32_t F, const int32_t* seg_starts_host, int32_t R, const int32_t* trim_host, const double* edges_host,
                 int32_t n_bins, double* by_dev, void* stream) {
    const char* who = "score_by";
    if (!keys_dev || !values_dev || !seg_starts_host || !edges_host || !by_dev) return ape_fail(APE_ERR_INVALID_ARG, "%s: NULL argument", who);
    if (int rc = ape_check_segments(who, F, seg_starts_host, R)) return rc;
    if (trim_host)
        for (int r = 0; r < R; ++r)
            if (trim_host[2 * r] < 0 || trim_host[2 * r + 1] < 0)
                return ape_fail(APE_ERR_INVALID_ARG, "%s: trim[%d] = (%d, %d) is negative", who, r, trim_host[2 * r], trim_host[2 * r + 1]);
    if (n_sets < 1 || n_sets > APE_POST_MAX_CONFIGS)
        return ape_fail(APE_ERR_INVALID_ARG, "%s: n_sets %d, between 1 and %d", who, n_sets, APE_POST_MAX_CONFIGS);
    if (n_bins < 1 || n_bins > APE_BY_MAX_BINS) return ape_fail(APE_ERR_INVALID_ARG, "%s: n_bins %d, between 1 and %d", who, n_bins, APE_BY_MAX_BINS);
    long long kext = 0, vext = 0;
    if (int rc = check_side(who, "keys", keys_dev, keys_dtype, n_keys, APE_BY_MAX_KEYS, n_sets, keys_set_stride, F, keys_frame_stride, &kext)) return rc;
    if (int rc = check_side(who, "values", values_dev, values_dtype, n_values, APE_BY_MAX_VALUES, n_sets, values_set_stride, F, values_frame_stride, &vext))
        return rc;
    if ((uintptr_t)by_dev & 7u) return ape_fail(APE_ERR_INVALID_ARG, "%s: by_dev is not aligned to its element", who);
    for (int k = 0; k < n_keys; ++k) {
        const double* e = edges_host + (size_t)k * (size_t)(n_bins + 1);
        for (int i = 0; i <= n_bins; ++i)
            if (!std::isfinite(e[i]) || (i > 0 && !(e[i] > e[i - 1])))
                return ape_fail(APE_ERR_INVALID_ARG, "%s: edges[%d][%d] = %g (finite and strictly increasing)", who, k, i, e[i]);
    }
    const long long cells = (long long)(n_bins + 3) * n_values * 4;                      // doubles of a (set, recording | piece, key) record
    const long long out_elems = (long long)n_sets * R * n_keys * cells;                  // (at most 64 * 2^31 * 8 * 8192 < 2^63)
    if (out_elems > 2147483647LL) return ape_fail(APE_ERR_INVALID_ARG, "%s: %lld output elements, at most 2^31 - 1", who, out_elems);
    // the windows and their pieces
    long long pieces = 0;
    for (int r = 0; r < R; ++r) {
        const long long lo = (long long)seg_starts_host[r] + (trim_host ? trim_host[2 * r] : 0);
        const long long up = (long long)(r + 1 < R ? seg_starts_host[r + 1] : F) - (trim_host ? trim_host[2 * r + 1] : 0);
        if (up > lo) pieces += (up - lo + APE_BY_PIECE - 1) / APE_BY_PIECE;
    }
    const long long part_bytes = (long long)n_sets * pieces * n_keys * cells * (long long)sizeof(double);     // (64 * 2^31 * 8 * 8192 * 8 < 2^63)
    if (part_bytes > SB_MAX_PART_BYTES)
        return ape_fail(APE_ERR_INVALID_ARG, "%s: %lld bytes of piece records (%lld pieces of %d frames), at most %lld", who, part_bytes, pieces,
                        APE_BY_PIECE, SB_MAX_PART_BYTES);
    const uintptr_t ba = (uintptr_t)by_dev, bb = ba + (uintptr_t)out_elems * sizeof(double);
    const uintptr_t ka = (uintptr_t)keys_dev, va = (uintptr_t)values_dev;
    if (ka < bb && ba < ka + (uintptr_t)kext) return ape_fail(APE_ERR_INVALID_ARG, "%s: by_dev overlaps keys_dev", who);
    if (va < bb && ba < va + (uintptr_t)vext) return ape_fail(APE_ERR_INVALID_ARG, "%s: by_dev overlaps values_dev", who);
    const hipStream_t st = (hipStream_t)stream;
    if (int rc = ape_check_not_capturing(st, who, "host arrays are staged per call")) return rc;
    int device = 0;
    APE_SCORE_TRY(g_pool.prefix, hipGetDevice(&device));

    const size_t ints_bytes = (((size_t)R * 3 + 1) * sizeof(int) + 7) & ~(size_t)7;      // win_lo [R], win_len [R], piece_at [R + 1]; then the edges
    const size_t edges_bytes = (size_t)n_keys * (size_t)(n_bins + 1) * sizeof(double);
    const size_t host_bytes = ints_bytes + edges_bytes;

    std::lock_guard<std::mutex> lock(g_pool.mu);
    ApeSlot* slot = nullptr;
    if (int rc = g_pool.take(device, host_bytes, host_bytes + (size_t)part_bytes, &slot)) return rc;
    char* pin = static_cast<char*>(slot->pinned);
    int* win_lo = reinterpret_cast<int*>(pin);
    int* win_len = win_lo + R;
    int* piece_at = win_len + R;
    int at = 0;
    for (int r = 0; r < R; ++r) {
        const long long lo = (long long)seg_starts_host[r] + (trim_host ? trim_host[2 * r] : 0);
        const long long up = (long long)(r + 1 < R ? seg_starts_host[r + 1] : F) - (trim_host ? trim_host[2 * r + 1] : 0);
        const bool any = up > lo;
        win_lo[r] = any ? (int)lo : 0;
        win_len[r] = any ? (int)(up - lo) : 0;
        piece_at[r] = at;
        at += any ? (int)((up - lo + APE_BY_PIECE - 1) / APE_BY_PIECE) : 0;
    }
    piece_at[R] = at;
    memcpy(pin + ints_bytes, edges_host, edges_bytes);
    // (a copy that fails leaves through finish() like a launch that fails: the slot's event is recorded either way)
    hipError_t e = hipMemcpyAsync(slot->dev, slot->pinned, host_bytes, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return g_pool.finish(who, slot, e, st);

    ByParams p{};
    char* dev = static_cast<char*>(slot->dev);
    p.keys = keys_dev; p.values = values_dev;
    p.win_lo = reinterpret_cast<const int*>(dev);
    p.win_len = p.win_lo + R;
    p.piece_at = p.win_len + R;
    p.edges = reinterpret_cast<const double*>(dev + ints_bytes);
    p.part = reinterpret_cast<double*>(dev + host_bytes);
    p.by = by_dev;
    p.kset = n_sets > 1 ? (long long)keys_set_stride : 0; p.kframe = keys_frame_stride;
    p.vset = n_sets > 1 ? (long long)values_set_stride : 0; p.vframe = values_frame_stride;
    p.R = R; p.K = n_keys; p.V = n_values; p.B = n_bins; p.P = (int)pieces;

    if (pieces > 0) {
        const dim3 grid((unsigned)pieces, (unsigned)n_keys, (unsigned)n_sets);
        const size_t lds = sb_lds_bytes(n_bins, n_values);
        const bool k32 = keys_dtype == APE_F32, v32 = values_dtype == APE_F32;
        if (k32 && v32) launch_by<float, float>(p, grid, lds, st);
        else if (k32) launch_by<float, double>(p, grid, lds, st);
        else if (v32) launch_by<double, float>(p, grid, lds, st);
        else launch_by<double, double>(p, grid, lds, st);
        e = hipGetLastError();
        if (e != hipSuccess) return g_pool.finish(who, slot, e, st);
    }
    const int chunks = (int)((cells + SB_BLOCK - 1) / SB_BLOCK);
    hipLaunchKernelGGL(ape_score_by_fold, dim3((unsigned)R * (unsigned)chunks, (unsigned)n_keys, (unsigned)n_sets), dim3(SB_BLOCK), 0, st, p, chunks);
    return g_pool.finish(who, slot, hipGetLastError(), st);
}
