// A rung of a ladder of windows for every frame, from a per-frame key such as the hand speed (ape_select_rungs; the
// reference has no counterpart).  Keys that lie on the device -- a strided column of motion rows, S sets of them -- are binned over
// fixed edges, the bin names a rung r0, and an envelope keeps a frame's reach from exceeding the reach chosen at any frame g of its
// recording by more than |f - g| / k: a hold frame next to a reach does not get a window that covers the reach.  include/ape_hip.h
// states the rule.
//
// ape_select_rungs_kernel  grid (tiles, sets), 256 frames per workgroup, one lane per frame.  The edges and the three small tables
//                          (rung of a slot, reach of a rung, widest rung of a reach) go to LDS; then the workgroup finds r0 of its 256
//                          frames and of the halo = k (reach[L - 1] - reach[0]) <= 504 frames on either side (clipped to [0, F)) and
//                          keeps their reaches in LDS, one byte each.  A frame further away cannot lower the cap below the widest
//                          reach.  Each lane walks outwards from its frame on both sides, within its recording and the halo, and takes
//                          the minimum of reach + distance / k (the quotient counted up, no division in the loop); neighbouring lanes
//                          read neighbouring bytes.  A halo frame's r0 is found again by the neighbouring workgroup: a binary search
//                          over at most 256 edges, cheaper than a pass of its own with a round trip through device memory.
//
// All integer, every output byte one lane's own minimum: the same inputs give the same bits.  No inline assembly.
#include "ape_internal.h"
#include "../../include/ape_hip.h"
#include "bank_host.h"
#include "score_host.h"

#include <cmath>
#include <cstring>

#include "score_device.h"

namespace {

using ape_scoredev::find_rec;

constexpr int SR_BLOCK = 256;
constexpr int SR_MAX_REACH = APE_POST_MAX_WINDOW - 1;   // max(back, ahead) of a window of at most APE_POST_MAX_WINDOW frames
constexpr int SR_MAX_HALO = APE_SELECT_MAX_SLOPE * SR_MAX_REACH;
constexpr int SR_TABLES = (APE_SELECT_MAX_EDGES + 1 + 7) / 8 * 8;      // bytes of the slot table, padded

struct SrParams {
    const void* keys;
    const int* starts;                                  // [R]
    const double* edges;                                // [B]
    const unsigned char* tables;                        // rung_of_slot [SR_TABLES] | reach [64] | widest rung of a reach [64]
    unsigned char* sel;                                 // [S, F]
    long long set_stride, frame_stride;
    int F, R, B, k, halo, nan_rung;
};

template <typename T>
__global__ __launch_bounds__(SR_BLOCK) void ape_select_rungs_kernel(const SrParams p) {
    __shared__ double ledges[APE_SELECT_MAX_EDGES];
    __shared__ unsigned char ltab[SR_TABLES + 2 * APE_POST_MAX_WINDOW];
    __shared__ unsigned char lreach[SR_BLOCK + 2 * SR_MAX_HALO];       // reach[r0] of frame t0 - halo + i
    const unsigned char* rung_of_slot = ltab;
    const unsigned char* reach = ltab + SR_TABLES;
    const unsigned char* widest = reach + APE_POST_MAX_WINDOW;
    const int tid = threadIdx.x, set = blockIdx.y;
    const long long t0 = (long long)blockIdx.x * SR_BLOCK;

    for (int i = tid; i < p.B; i += SR_BLOCK) ledges[i] = p.edges[i];
    for (int i = tid; i < SR_TABLES + 2 * APE_POST_MAX_WINDOW; i += SR_BLOCK) ltab[i] = p.tables[i];
    __syncthreads();

    const T* keys = static_cast<const T*>(p.keys) + (long long)set * p.set_stride;
    auto rung_of = [&](long long g) -> int {
        const double v = (double)keys[g * p.frame_stride];
        if (!(v >= -1.7976931348623157e308 && v <= 1.7976931348623157e308)) return p.nan_rung;     // NaN, +-inf
        int lo = 0, n = p.B;                            // the edges below v are ledges[0 .. lo) once n == 0
        while (n > 0) {
            const int half = n >> 1;
            if (ledges[lo + half] < v) { lo += half + 1; n -= half + 1; } else n = half;
        }
        return (int)rung_of_slot[lo];
    };

    const long long f = t0 + tid;
    int r0 = 0;
    if (f < p.F) {
        r0 = rung_of(f);
        lreach[p.halo + tid] = reach[r0];
    }
    // the halos: `halo` frames below the tile, then `halo` frames above it
    for (int j = tid; j < 2 * p.halo; j += SR_BLOCK) {
        const bool below = j < p.halo;
        const long long g = below ? t0 - p.halo + j : t0 + SR_BLOCK + (j - p.halo);
        if (g >= 0 && g < p.F) lreach[below ? j : SR_BLOCK + j] = reach[rung_of(g)];
    }
    __syncthreads();
    if (f >= p.F) return;

    int r = r0;
    if (p.halo > 0) {
        const int rec = find_rec(p.starts, p.R, f);
        const long long seg = p.starts[rec], end = rec + 1 < p.R ? p.starts[rec + 1] : p.F;
        const int below = (int)(f - seg < p.halo ? f - seg : p.halo), above = (int)(end - 1 - f < p.halo ? end - 1 - f : p.halo);
        const unsigned char* at = lreach + p.halo + tid;
        int cap = (int)at[0];
        for (int d = 1, q = 0, rem = 0; d <= below; ++d) {
            if (++rem == p.k) { rem = 0; ++q; }         // q = d / k
            const int c = (int)at[-d] + q;
            cap = c < cap ? c : cap;
        }
        for (int d = 1, q = 0, rem = 0; d <= above; ++d) {
            if (++rem == p.k) { rem = 0; ++q; }
            const int c = (int)at[d] + q;
            cap = c < cap ? c : cap;
        }
        const int w = (int)widest[cap];                 // (reach[0] <= cap <= reach[r0]: a rung exists)
        r = w < r0 ? w : r0;
    }
    p.sel[(size_t)set * (size_t)p.F + (size_t)f] = (unsigned char)r;
}

// the staging of a call: starts, edges and the tables (score_host.h)
ApeSlotPool g_pool("select_rungs");

}  // namespace

int ape_select_rungs(const void* keys_dev, int32_t keys_dtype, int32_t n_sets, int64_t set_stride, int32_t F, int64_t frame_stride,
                     const int32_t* seg_starts_host, int32_t R, const double* edges_host, int32_t n_edges, const int32_t* rung_of_slot_host,
                     int32_t nan_rung, const int32_t* reach_host, int32_t L, int32_t slope, uint8_t* sel_dev, void* stream) {
    const char* who = "select_rungs";
    if (!keys_dev || !seg_starts_host || !edges_host || !rung_of_slot_host || !reach_host || !sel_dev)
        return ape_fail(APE_ERR_INVALID_ARG, "%s: NULL argument", who);
    if (keys_dtype != APE_F32 && keys_dtype != APE_F64) return ape_fail(APE_ERR_INVALID_ARG, "%s: unknown dtype selector %d", who, keys_dtype);
    if (int rc = ape_check_segments(who, F, seg_starts_host, R)) return rc;
    if (n_sets < 1 || n_sets > APE_POST_MAX_CONFIGS) return ape_fail(APE_ERR_INVALID_ARG, "%s: S=%d sets (1 .. %d)", who, n_sets, APE_POST_MAX_CONFIGS);
    if (L < 1 || L > APE_POST_MAX_CONFIGS) return ape_fail(APE_ERR_INVALID_ARG, "%s: L=%d rungs (1 .. %d)", who, L, APE_POST_MAX_CONFIGS);
    if (n_edges < 1 || n_edges > APE_SELECT_MAX_EDGES) return ape_fail(APE_ERR_INVALID_ARG, "%s: B=%d edges (1 .. %d)", who, n_edges, APE_SELECT_MAX_EDGES);
    if (slope < 0 || slope > APE_SELECT_MAX_SLOPE) return ape_fail(APE_ERR_INVALID_ARG, "%s: slope %d outside 0..%d", who, slope, APE_SELECT_MAX_SLOPE);
    for (int i = 0; i < n_edges; ++i)
        if (!std::isfinite(edges_host[i]) || (i > 0 && !(edges_host[i] > edges_host[i - 1])))
            return ape_fail(APE_ERR_INVALID_ARG, "%s: edges[%d] = %g (finite and strictly increasing)", who, i, edges_host[i]);
    for (int r = 0; r < L; ++r) {
        if (reach_host[r] < 0 || reach_host[r] > SR_MAX_REACH)
            return ape_fail(APE_ERR_INVALID_ARG, "%s: reach[%d] = %d outside 0..%d", who, r, reach_host[r], SR_MAX_REACH);
        if (r > 0 && reach_host[r] < reach_host[r - 1])
            return ape_fail(APE_ERR_INVALID_ARG, "%s: reach[%d] = %d below reach[%d] = %d (the ladder runs narrow to wide)", who, r, reach_host[r],
                            r - 1, reach_host[r - 1]);
    }
    for (int i = 0; i <= n_edges; ++i)
        if (rung_of_slot_host[i] < 0 || rung_of_slot_host[i] >= L)
            return ape_fail(APE_ERR_INVALID_ARG, "%s: rung_of_slot[%d] = %d outside 0..L-1 = %d", who, i, rung_of_slot_host[i], L - 1);
    if (nan_rung < 0 || nan_rung >= L) return ape_fail(APE_ERR_INVALID_ARG, "%s: nan_rung %d outside 0..L-1 = %d", who, nan_rung, L - 1);
    if (frame_stride < 1) return ape_fail(APE_ERR_INVALID_ARG, "%s: frame_stride %lld below 1", who, (long long)frame_stride);
    // the last element read, in elements from keys_dev: every stride is positive from here on
    long long extent = 0, term = 0;
    bool fits = !__builtin_mul_overflow((long long)(F - 1), (long long)frame_stride, &extent);
    if (n_sets > 1) {
        if (!fits || set_stride <= extent)
            return ape_fail(APE_ERR_INVALID_ARG, "%s: set_stride %lld does not clear a set of F frames", who, (long long)set_stride);
        fits = !__builtin_mul_overflow((long long)(n_sets - 1), (long long)set_stride, &term) && !__builtin_add_overflow(extent, term, &extent);
    }
    const long long esize = keys_dtype == APE_F32 ? 4 : 8;
    fits = fits && !__builtin_add_overflow(extent, 1ll, &extent) && !__builtin_mul_overflow(extent, esize, &extent);
    if (!fits) return ape_fail(APE_ERR_INVALID_ARG, "%s: the extent of the keys does not fit 63 bits", who);
    if ((uintptr_t)keys_dev & (uintptr_t)(esize - 1)) return ape_fail(APE_ERR_INVALID_ARG, "%s: keys_dev is not aligned to its element", who);
    const uintptr_t ka = (uintptr_t)keys_dev, sa = (uintptr_t)sel_dev;
    const uintptr_t kb = ka + (uintptr_t)extent, sb = sa + (uintptr_t)n_sets * (uintptr_t)F;
    if (ka < sb && sa < kb) return ape_fail(APE_ERR_INVALID_ARG, "%s: sel_dev overlaps keys_dev", who);
    const hipStream_t st = (hipStream_t)stream;
    if (int rc = ape_check_not_capturing(st, who, "host arrays are staged per call")) return rc;
    int device = 0;
    APE_SCORE_TRY(g_pool.prefix, hipGetDevice(&device));

    const size_t edges_bytes = (size_t)n_edges * sizeof(double);                        // the edges, then the tables, then the starts
    const size_t tables_bytes = SR_TABLES + 2 * APE_POST_MAX_WINDOW;
    const size_t host_bytes = edges_bytes + tables_bytes + (size_t)R * sizeof(int);

    std::lock_guard<std::mutex> lock(g_pool.mu);
    ApeSlot* slot = nullptr;
    if (int rc = g_pool.take(device, host_bytes, host_bytes, &slot)) return rc;
    char* pin = static_cast<char*>(slot->pinned);
    memcpy(pin, edges_host, edges_bytes);
    unsigned char* tab = reinterpret_cast<unsigned char*>(pin + edges_bytes);
    memset(tab, 0, tables_bytes);
    for (int i = 0; i <= n_edges; ++i) tab[i] = (unsigned char)rung_of_slot_host[i];
    unsigned char* reach = tab + SR_TABLES;
    unsigned char* widest = reach + APE_POST_MAX_WINDOW;
    for (int r = 0; r < L; ++r) reach[r] = (unsigned char)reach_host[r];
    for (int c = 0, r = 0; c < APE_POST_MAX_WINDOW; ++c) {                              // the largest r with reach[r] <= c (0 below reach[0]: never read)
        while (r + 1 < L && reach_host[r + 1] <= c) ++r;
        widest[c] = (unsigned char)r;
    }
    memcpy(pin + edges_bytes + tables_bytes, seg_starts_host, (size_t)R * sizeof(int));
    // (a copy that fails leaves through finish() like a launch that fails: the slot's event is recorded either way)
    hipError_t e = hipMemcpyAsync(slot->dev, slot->pinned, host_bytes, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return g_pool.finish(who, slot, e, st);

    SrParams p{};
    char* dev = static_cast<char*>(slot->dev);
    p.keys = keys_dev;
    p.edges = reinterpret_cast<const double*>(dev);
    p.tables = reinterpret_cast<const unsigned char*>(dev + edges_bytes);
    p.starts = reinterpret_cast<const int*>(dev + edges_bytes + tables_bytes);
    p.sel = sel_dev;
    p.set_stride = n_sets > 1 ? (long long)set_stride : 0; p.frame_stride = frame_stride;
    p.F = F; p.R = R; p.B = n_edges; p.k = slope; p.nan_rung = nan_rung;
    p.halo = slope * (reach_host[L - 1] - reach_host[0]);

    const dim3 grid((unsigned)(((long long)F + SR_BLOCK - 1) / SR_BLOCK), (unsigned)n_sets);
    if (keys_dtype == APE_F32) hipLaunchKernelGGL(ape_select_rungs_kernel<float>, grid, dim3(SR_BLOCK), 0, st, p);
    else hipLaunchKernelGGL(ape_select_rungs_kernel<double>, grid, dim3(SR_BLOCK), 0, st, p);
    return g_pool.finish(who, slot, hipGetLastError(), st);
}
