// Spectra of a replay: Welch sums of |X|^2, |Y|^2 and conj(Y) X per recording, column and frequency bin, on the float64 matrix cores
// (ape_spectra; the reference has no counterpart).  Any columns of up to 64 sets of per-frame rows against an optional
// truth, one list of recordings; segments of N frames, hop frames apart, never across a recording boundary.
//
// ape_spectra_kernel  grid (R, V, sets), 256 threads.  A workgroup owns one (recording, column, set) and walks the recording's tiles of 16
//                     segments in order.  Per tile it copies the tile's frame span (N + 15 hop samples per side, float32 widened) into
//                     LDS, takes every segment's mean and finiteness (a wave per four segments), and then each wave forms the DFT of the
//                     16 segments for its blocks of 16 bins on v_mfma_f64_16x16x4_f64: A = 16 segments x 4 samples, read from the span
//                     with mean and taper applied on the way, B = 4 samples x 16 bins from the N-entry cos / sin table in LDS at
//                     (k n) mod N, stepped by 4 k mod N.  Four accumulators: cos and sin block for x and for y, so a lane holds the real
//                     and imaginary parts of the same (segment, bin) of both sides and forms the products itself.  Where N is a multiple
//                     of 32, bin N/2 would sit alone in a ninth, seventeenth, ... block: it is a_n (-1)^n summed beside the means.
//
// The f64 C/D map is col = lane & 15, row = (lane >> 4) + 4 reg: a lane holds segments q, q + 4, q + 8, q + 12 (q = lane >> 4) of bin
// lane & 15.  Sums: no atomics.  A lane adds its four segments in that order, lane q = 0 adds the four q in order, and the tile's sum is
// added to the record so far, tile after tile; the record is written by the lane that reads it back.  Segments left out enter as exact
// zeros.  float64 with separate roundings for a * b + c (the products of the MFMA's own chain are fused, which the tests' bound covers):
// contraction is off in this file.
#include "ape_internal.h"
#include "../../include/ape_hip.h"
#include "bank_host.h"
#include "score_host.h"

#include <cmath>
#include <cstdio>
#include <cstring>

#pragma clang fp contract(off)

namespace {

constexpr int SP_BLOCK = 256, SP_WAVES = SP_BLOCK / 64;
constexpr int SP_TILE = 16;                             // segments of a tile: the rows of A
constexpr size_t SP_STATIC_LDS = 64 * 1024;             // dynamic LDS above this is asked for by attribute

typedef double f64x4 __attribute__((ext_vector_type(4)));

// Timing-only switches of `make spectra_ablate` (diagnostic libraries that the package never loads; 0 in the product, where every one of
// them folds away): 1 the step loop is not run (no operand reads, no MFMA), 2 the span is filled with ones in place of the strided reads
// of the rows, 4 the pass over the segments' means, finiteness and bin N/2 is not run.  tools/spectra_bench.py --ablate times them.
#ifndef APE_SPECTRA_ABLATE
#define APE_SPECTRA_ABLATE 0
#endif
constexpr bool AB_NO_STEPS = (APE_SPECTRA_ABLATE & 1) != 0, AB_NO_GATHER = (APE_SPECTRA_ABLATE & 2) != 0, AB_NO_MEANS = (APE_SPECTRA_ABLATE & 4) != 0;

struct SpectraParams {
    const void* x;
    const void* y;                                      // NULL: no truth
    const int* starts;                                  // [R]
    const int* xcols;                                   // [V]
    const int* ycols;                                   // [V]
    const double* table;                                // cos [N] | sin [N] | taper [N]
    double* acc;                                        // [n_sets, R, V, N/2 + 1, W]
    int* counts;                                        // [n_sets, R, V, 2]
    long long xset, xframe, yset, yframe;
    int F, R, V, skip, N, hop, detrend, span;           // span = N + 15 hop
};

// where sample a of the span lies in LDS: one double of padding per 32, so that the 16 segments of a lane group, hop apart, do not all
// meet in one bank when hop is a multiple of 32
__device__ __forceinline__ int skew(int a) { return a + (a >> 5); }
inline int skew_host(int a) { return a + (a >> 5); }

__device__ __forceinline__ bool fin(double v) { return fabs(v) <= 1.7976931348623157e308; }

// the sum of the 64 lanes' values, the same in every lane: a butterfly, each level's pairs commute
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = v + __shfl_xor(v, off, 64);
    return v;
}

// the four lane groups' values of column j in group order, from lane j of each
__device__ __forceinline__ double groups_sum(double v, int j) {
    const double a = __shfl(v, j, 64), b = __shfl(v, j + 16, 64), c = __shfl(v, j + 32, 64), d = __shfl(v, j + 48, 64);
    return ((a + b) + c) + d;
}

template <typename TX, typename TY, bool TRUTH>
__global__ __launch_bounds__(SP_BLOCK) void ape_spectra_kernel(const SpectraParams p) {
    extern __shared__ double sp_mem[];                  // cos [N] | sin [N] | taper [N] | span of x | span of y
    __shared__ double mean_s[2][SP_TILE];
    __shared__ int ok_s[SP_TILE];
    __shared__ double nyq_s[2][SP_TILE];
    constexpr int W = TRUTH ? 4 : 1;
    const int N = p.N, hop = p.hop;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = blockIdx.x, v = blockIdx.y, set = blockIdx.z;
    const int span_lds = skew(p.span) + 1;
    const double* cs = sp_mem;
    const double* sn = sp_mem + N;
    const double* tp = sp_mem + 2 * N;
    double* sx = sp_mem + 3 * N;
    double* sy = sx + span_lds;
    for (int i = threadIdx.x; i < 3 * N; i += SP_BLOCK) sp_mem[i] = p.table[i];

    const int s = p.starts[r], e = r + 1 < p.R ? p.starts[r + 1] : p.F;
    const long long len = (long long)e - (long long)s - (long long)p.skip;
    const int J = len >= (long long)N ? (int)((len - N) / hop) + 1 : 0;
    // N / 2 + 1 bins.  Where N is a multiple of 32 the last one would be alone in a block of 16: bins 0 .. N/2 - 1 fill N / 32 blocks and
    // bin N/2, whose cosine is (-1)^n and whose sine is 0, is summed on the vector unit beside the means
    const bool nyq = (N & 31) == 0;
    const int bins = N / 2 + 1, nblk = nyq ? N / 32 : (bins + 15) / 16;
    const size_t rec = ((size_t)set * (size_t)p.R + (size_t)r) * (size_t)p.V + (size_t)v;
    double* acc = p.acc + rec * (size_t)bins * W;
    const TX* xs = static_cast<const TX*>(p.x) + (long long)set * p.xset + p.xcols[v];
    const TY* ys = TRUTH ? static_cast<const TY*>(p.y) + (long long)set * p.yset + p.ycols[v] : nullptr;

    if (J == 0) {
        for (int i = threadIdx.x; i < bins * W; i += SP_BLOCK) acc[i] = 0.0;
    }
    int summed = 0;                                     // (thread 0's)
    const int j = lane & 15, q = lane >> 4;             // A: segment j, sample q of the step; B: sample q, bin j of the block
    for (int t0 = 0; t0 < J; t0 += SP_TILE) {
        const int nseg = J - t0 < SP_TILE ? J - t0 : SP_TILE;
        const long long f0 = (long long)s + p.skip + (long long)t0 * hop;
        const int have = (nseg - 1) * hop + N;          // samples the tile's segments cover: all inside the recording
        __syncthreads();                                // (the tile before has been read)
        for (int i = threadIdx.x; i < p.span; i += SP_BLOCK) {
            const bool in = i < have;
            if constexpr (AB_NO_GATHER) {
                sx[skew(i)] = in ? 1.0 : 0.0;
                if constexpr (TRUTH) sy[skew(i)] = in ? 1.0 : 0.0;
                continue;
            }
            sx[skew(i)] = in ? (double)xs[(f0 + i) * p.xframe] : 0.0;
            if constexpr (TRUTH) sy[skew(i)] = in ? (double)ys[(f0 + i) * p.yframe] : 0.0;
        }
        __syncthreads();
        // mean and finiteness of segments wave, wave + 4, ...: lane l adds samples l, l + 64, ... in order, then the butterfly
        if constexpr (AB_NO_MEANS) {
            if (threadIdx.x < SP_TILE) {
                mean_s[0][threadIdx.x] = 0.0; mean_s[1][threadIdx.x] = 0.0; nyq_s[0][threadIdx.x] = 0.0; nyq_s[1][threadIdx.x] = 0.0;
                ok_s[threadIdx.x] = (int)threadIdx.x < nseg ? 1 : 0;
            }
        }
        for (int g = wave; g < (AB_NO_MEANS ? 0 : SP_TILE); g += SP_WAVES) {
            double ax = 0.0, ay = 0.0;
            bool fine = g < nseg;
            if (g < nseg) {
                for (int n = lane; n < N; n += 64) {
                    const double a = sx[skew(g * hop + n)];
                    fine = fine && fin(a);
                    ax = ax + a;
                    if constexpr (TRUTH) {
                        const double b = sy[skew(g * hop + n)];
                        fine = fine && fin(b);
                        ay = ay + b;
                    }
                }
            }
            ax = wave_sum(ax);
            if constexpr (TRUTH) ay = wave_sum(ay);
            const bool all_fine = __all(fine) != 0;
            const double mxg = p.detrend ? ax / (double)N : 0.0, myg = p.detrend ? ay / (double)N : 0.0;
            if (lane == 0) {
                mean_s[0][g] = mxg;
                mean_s[1][g] = myg;
                ok_s[g] = all_fine ? 1 : 0;
            }
            if (nyq) {                                  // (uniform) X(N/2) = sum_n a_n (-1)^n: lane l adds n = l, l + 64, ... (all of one sign), then the butterfly
                double nx = 0.0, ny = 0.0;
                if (all_fine) {
                    for (int n = lane; n < N; n += 64) {
                        const double w = tp[n];
                        const double a = w * (sx[skew(g * hop + n)] - mxg);
                        nx = nx + ((n & 1) ? -a : a);
                        if constexpr (TRUTH) {
                            const double b = w * (sy[skew(g * hop + n)] - myg);
                            ny = ny + ((n & 1) ? -b : b);
                        }
                    }
                }
                nx = wave_sum(nx);
                if constexpr (TRUTH) ny = wave_sum(ny);
                if (lane == 0) { nyq_s[0][g] = nx; nyq_s[1][g] = ny; }
            }
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int g = 0; g < nseg; ++g) summed += ok_s[g];
            if (nyq) {                                  // bin N/2 in the order of the other bins: segments q, q + 4, q + 8, q + 12, then q = 0 .. 3
                double txx = 0.0, tyy = 0.0, tre = 0.0;
                for (int g = 0; g < 4; ++g) {
                    double pxx = 0.0, pyy = 0.0, pre = 0.0;
                    for (int i = 0; i < 4; ++i) {
                        const double xr = nyq_s[0][g + 4 * i], yr = nyq_s[1][g + 4 * i];
                        pxx = i == 0 ? xr * xr : pxx + xr * xr;
                        pyy = i == 0 ? yr * yr : pyy + yr * yr;
                        pre = i == 0 ? yr * xr : pre + yr * xr;
                    }
                    txx = g == 0 ? pxx : txx + pxx;
                    tyy = g == 0 ? pyy : tyy + pyy;
                    tre = g == 0 ? pre : tre + pre;
                }
                double* o = acc + (size_t)(N / 2) * W;
                const bool first = t0 == 0;
                o[0] = (first ? 0.0 : o[0]) + txx;
                if constexpr (TRUTH) {
                    o[1] = (first ? 0.0 : o[1]) + tyy;
                    o[2] = (first ? 0.0 : o[2]) + tre;
                    o[3] = first ? 0.0 : o[3];          // (real spectra at this bin: the imaginary part of the cross term is +0.0)
                }
            }
        }
        const bool okj = ok_s[j] != 0;
        const double mx = mean_s[0][j], my = mean_s[1][j];
        const int abase = j * hop + q;
        for (int blk = wave; blk < nblk; blk += SP_WAVES) {
            const int bin = blk * 16 + j;               // (bins past N/2 pad the last block where N is no multiple of 32: computed, not written)
            int idx = (bin * q) % N;
            const int inc = (4 * bin) % N;
            f64x4 cx = {0.0, 0.0, 0.0, 0.0}, zx = {0.0, 0.0, 0.0, 0.0}, cy = {0.0, 0.0, 0.0, 0.0}, zy = {0.0, 0.0, 0.0, 0.0};
            for (int n = 0; n < (AB_NO_STEPS ? 0 : N); n += 4) {
                const double w = tp[n + q], c = cs[idx], z = sn[idx];
                const int at = skew(abase + n);
                const double dx = w * (sx[at] - mx);
                const double a = okj ? dx : 0.0;
                cx = __builtin_amdgcn_mfma_f64_16x16x4f64(a, c, cx, 0, 0, 0);
                zx = __builtin_amdgcn_mfma_f64_16x16x4f64(a, z, zx, 0, 0, 0);
                if constexpr (TRUTH) {
                    const double dy = w * (sy[at] - my);
                    const double b = okj ? dy : 0.0;
                    cy = __builtin_amdgcn_mfma_f64_16x16x4f64(b, c, cy, 0, 0, 0);
                    zy = __builtin_amdgcn_mfma_f64_16x16x4f64(b, z, zy, 0, 0, 0);
                }
                idx += inc;
                idx = idx >= N ? idx - N : idx;
            }
            // X = cx - i zx, Y = cy - i zy of segment q + 4 i, bin `bin`: |X|^2, |Y|^2, Re and Im of conj(Y) X
            double pxx = 0.0, pyy = 0.0, pre = 0.0, pim = 0.0;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const double t = cx[i] * cx[i] + zx[i] * zx[i];
                pxx = i == 0 ? t : pxx + t;
                if constexpr (TRUTH) {
                    const double u = cy[i] * cy[i] + zy[i] * zy[i];
                    const double re = cy[i] * cx[i] + zy[i] * zx[i];
                    const double im = zy[i] * cx[i] - cy[i] * zx[i];
                    pyy = i == 0 ? u : pyy + u;
                    pre = i == 0 ? re : pre + re;
                    pim = i == 0 ? im : pim + im;
                }
            }
            const double txx = groups_sum(pxx, j);
            double tyy = 0.0, tre = 0.0, tim = 0.0;
            if constexpr (TRUTH) { tyy = groups_sum(pyy, j); tre = groups_sum(pre, j); tim = groups_sum(pim, j); }
            if (q == 0 && bin < (nyq ? N / 2 : bins)) {
                double* o = acc + (size_t)bin * W;
                const bool first = t0 == 0;
                o[0] = (first ? 0.0 : o[0]) + txx;
                if constexpr (TRUTH) {
                    o[1] = (first ? 0.0 : o[1]) + tyy;
                    o[2] = (first ? 0.0 : o[2]) + tre;
                    o[3] = (first ? 0.0 : o[3]) + tim;
                }
            }
        }
    }
    if (threadIdx.x == 0) {
        p.counts[rec * 2] = summed;
        p.counts[rec * 2 + 1] = J - summed;
    }
}

// the staging of a call: starts, column offsets, then the cos / sin table and the taper (score_host.h)
ApeSlotPool g_pool("spectra");

// (called with the pool's lock held: `asked` holds, per device, the largest dynamic LDS this instantiation has been granted, so the
// attribute is set when a call outgrows it and not on every call)
template <typename TX, typename TY, bool TRUTH>
hipError_t launch_spectra(const SpectraParams& p, dim3 grid, size_t lds, int device, hipStream_t st) {
    static std::vector<size_t> asked;
    if (lds > SP_STATIC_LDS) {
        if (asked.size() <= (size_t)device) asked.resize((size_t)device + 1, 0);
        if (lds > asked[device]) {
            const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&ape_spectra_kernel<TX, TY, TRUTH>),
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) return e;
            asked[device] = lds;
        }
    }
    hipLaunchKernelGGL((ape_spectra_kernel<TX, TY, TRUTH>), grid, dim3(SP_BLOCK), lds, st, p);
    return hipGetLastError();
}

// one side's addressing: dtype, strides, column offsets; *ext: bytes from the side's first element to past its last
int check_side(const char* who, const char* side, int32_t dtype, int64_t set_stride, int64_t frame_stride, const int32_t* cols, int32_t V,
               int32_t n_sets, int32_t F, bool shared_ok, long long* ext) {
    if (dtype != APE_F32 && dtype != APE_F64) return ape_fail(APE_ERR_INVALID_ARG, "%s: %s: unknown dtype selector", who, side);
    if (frame_stride < 1) return ape_fail(APE_ERR_INVALID_ARG, "%s: %s: frame stride %lld below 1", who, side, (long long)frame_stride);
    for (int v = 0; v < V; ++v)
        if (cols[v] < 0 || (int64_t)cols[v] >= frame_stride)
            return ape_fail(APE_ERR_INVALID_ARG, "%s: %s: column offset %d (entry %d) outside [0, frame stride %lld)", who, side, cols[v], v,
                            (long long)frame_stride);
    const bool shared = shared_ok && set_stride == 0;
    long long frames = 0, span = 0, bytes = 0;          // F * frame stride; the sets before the last, then the last; in bytes
    if (__builtin_mul_overflow((long long)F, (long long)frame_stride, &frames))
        return ape_fail(APE_ERR_INVALID_ARG, "%s: %s: F * frame stride does not fit 63 bits", who, side);
    if (n_sets > 1 && !shared && set_stride < frames)
        return ape_fail(APE_ERR_INVALID_ARG, "%s: %s: set stride %lld below F * frame stride = %lld: the sets overlap", who, side,
                        (long long)set_stride, frames);
    const long long sets = (n_sets > 1 && !shared) ? n_sets - 1 : 0;
    if (__builtin_mul_overflow(sets, (long long)set_stride, &span) || __builtin_add_overflow(span, frames, &span) ||
        __builtin_mul_overflow(span, (long long)(dtype == APE_F32 ? 4 : 8), &bytes))
        return ape_fail(APE_ERR_INVALID_ARG, "%s: %s: an extent of %d sets does not fit 63 bits", who, side, n_sets);
    *ext = bytes;
    return APE_OK;
}

bool overlaps(const void* a, long long abytes, const void* b, long long bbytes) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + (uintptr_t)bbytes && b0 < a0 + (uintptr_t)abytes;
}

}  // namespace

int ape_spectra(const void* x_dev, int32_t x_dtype, int64_t x_set_stride, int64_t x_frame_stride, const int32_t* x_cols_host,
                const void* y_dev, int32_t y_dtype, int64_t y_set_stride, int64_t y_frame_stride, const int32_t* y_cols_host, int32_t V,
                int32_t n_sets, int32_t F, const int32_t* seg_starts_host, int32_t R, int32_t skip, int32_t N, int32_t hop,
                const double* taper_host, uint32_t flags, double* acc_dev, int32_t* counts_dev, void* stream) {
    const char* who = "spectra";
    if (!x_dev || !x_cols_host || !seg_starts_host || !taper_host || !acc_dev || !counts_dev || (y_dev && !y_cols_host))
        return ape_fail(APE_ERR_INVALID_ARG, "%s: NULL argument", who);
    if (int rc = ape_check_segments(who, F, seg_starts_host, R)) return rc;
    if (skip < 0) return ape_fail(APE_ERR_INVALID_ARG, "%s: skip %d is negative", who, skip);
    if (N < 16 || N > APE_SPECTRA_MAX_N || (N & 15)) return ape_fail(APE_ERR_INVALID_ARG, "%s: N %d, a multiple of 16 in 16 .. %d", who, N, APE_SPECTRA_MAX_N);
    if (hop < 1 || hop > N) return ape_fail(APE_ERR_INVALID_ARG, "%s: hop %d, between 1 and N = %d", who, hop, N);
    if (V < 1 || V > APE_SPECTRA_MAX_COLS) return ape_fail(APE_ERR_INVALID_ARG, "%s: V %d, between 1 and %d", who, V, APE_SPECTRA_MAX_COLS);
    if (n_sets < 1 || n_sets > APE_POST_MAX_CONFIGS)
        return ape_fail(APE_ERR_INVALID_ARG, "%s: n_sets %d, between 1 and %d", who, n_sets, APE_POST_MAX_CONFIGS);
    if (flags & ~(uint32_t)APE_SPECTRA_DETREND) return ape_fail(APE_ERR_INVALID_ARG, "%s: unknown flags 0x%x", who, flags);
    long long xext = 0, yext = 0;
    if (int rc = check_side(who, "x", x_dtype, x_set_stride, x_frame_stride, x_cols_host, V, n_sets, F, false, &xext)) return rc;
    if (y_dev)
        if (int rc = check_side(who, "y", y_dtype, y_set_stride, y_frame_stride, y_cols_host, V, n_sets, F, true, &yext)) return rc;
    const int bins = N / 2 + 1, W = y_dev ? 4 : 1;
    const long long acc_bytes = (long long)n_sets * R * V * bins * W * (long long)sizeof(double);      // (64 * 2^31 * 16 * 257 * 4 * 8 < 2^63)
    const long long counts_bytes = (long long)n_sets * R * V * 2 * (long long)sizeof(int32_t);
    if (overlaps(acc_dev, acc_bytes, x_dev, xext) || overlaps(counts_dev, counts_bytes, x_dev, xext))
        return ape_fail(APE_ERR_INVALID_ARG, "%s: an output overlaps x_dev", who);
    if (y_dev && (overlaps(acc_dev, acc_bytes, y_dev, yext) || overlaps(counts_dev, counts_bytes, y_dev, yext)))
        return ape_fail(APE_ERR_INVALID_ARG, "%s: an output overlaps y_dev", who);
    if (overlaps(acc_dev, acc_bytes, counts_dev, counts_bytes)) return ape_fail(APE_ERR_INVALID_ARG, "%s: acc_dev overlaps counts_dev", who);
    const hipStream_t st = (hipStream_t)stream;
    if (int rc = ape_check_not_capturing(st, who, "host arrays are staged per call")) return rc;
    int device = 0;
    APE_SCORE_TRY(g_pool.prefix, hipGetDevice(&device));

    const size_t ints_bytes = (((size_t)R + 2 * (size_t)V) * sizeof(int) + 7) & ~(size_t)7;       // starts [R], x cols [V], y cols [V]; then the table
    const size_t table_bytes = 3 * (size_t)N * sizeof(double);
    const size_t host_bytes = ints_bytes + table_bytes;

    std::lock_guard<std::mutex> lock(g_pool.mu);
    ApeSlot* slot = nullptr;
    if (int rc = g_pool.take(device, host_bytes, host_bytes, &slot)) return rc;
    char* pin = static_cast<char*>(slot->pinned);
    int* ints = reinterpret_cast<int*>(pin);
    memcpy(ints, seg_starts_host, (size_t)R * sizeof(int));
    memcpy(ints + R, x_cols_host, (size_t)V * sizeof(int));
    memcpy(ints + R + V, y_dev ? y_cols_host : x_cols_host, (size_t)V * sizeof(int));
    double* table = reinterpret_cast<double*>(pin + ints_bytes);
    for (int i = 0; i < N; ++i) {                       // the float64 nearest to cos and sin of 2 pi i / N
        const long double th = 2.0L * 3.14159265358979323846264338327950288L * (long double)i / (long double)N;
        table[i] = (double)cosl(th);
        table[N + i] = (double)sinl(th);
    }
    memcpy(table + 2 * N, taper_host, (size_t)N * sizeof(double));
    // (a copy that fails leaves through finish() like a launch that fails: the slot's event is recorded either way)
    hipError_t e = hipMemcpyAsync(slot->dev, slot->pinned, host_bytes, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return g_pool.finish(who, slot, e, st);

    SpectraParams p{};
    char* dev = static_cast<char*>(slot->dev);
    p.x = x_dev; p.y = y_dev;
    p.starts = reinterpret_cast<const int*>(dev);
    p.xcols = p.starts + R;
    p.ycols = p.xcols + V;
    p.table = reinterpret_cast<const double*>(dev + ints_bytes);
    p.acc = acc_dev; p.counts = counts_dev;
    p.xset = n_sets > 1 ? (long long)x_set_stride : 0; p.xframe = x_frame_stride;
    p.yset = n_sets > 1 ? (long long)y_set_stride : 0; p.yframe = y_frame_stride;
    p.F = F; p.R = R; p.V = V; p.skip = skip; p.N = N; p.hop = hop;
    p.detrend = (flags & APE_SPECTRA_DETREND) ? 1 : 0;
    p.span = N + (SP_TILE - 1) * hop;

    const size_t lds = (3 * (size_t)N + (size_t)(y_dev ? 2 : 1) * (size_t)(skew_host(p.span) + 1)) * sizeof(double);
    const dim3 grid((unsigned)R, (unsigned)V, (unsigned)n_sets);
    const bool x32 = x_dtype == APE_F32, y32 = y_dtype == APE_F32;
    if (!y_dev) e = x32 ? launch_spectra<float, float, false>(p, grid, lds, device, st) : launch_spectra<double, double, false>(p, grid, lds, device, st);
    else if (x32 && y32) e = launch_spectra<float, float, true>(p, grid, lds, device, st);
    else if (x32) e = launch_spectra<float, double, true>(p, grid, lds, device, st);
    else if (y32) e = launch_spectra<double, float, true>(p, grid, lds, device, st);
    else e = launch_spectra<double, double, true>(p, grid, lds, device, st);
    return g_pool.finish(who, slot, e, st);
}
