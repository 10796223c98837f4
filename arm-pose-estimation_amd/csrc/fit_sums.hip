// Normal-equation sums for re-fitting the output layer to a wearer (ape_fit_sums; the reference has no counterpart): per
// recording the Gram matrix of z_f = [x_f (P), 1, (t_{f-l} - shift) / scale (Q)] over the recording's support, on the float64 matrix cores.
// include/ape_hip.h states the support, the pairing, the layout of a record and the ORDER of every sum, which is part of the contract.
//
// ape_fit_sums_kernel  grid (pieces, row blocks), 256 threads.  A piece is APE_FIT_PIECE consecutive frames of one recording's support,
//                      counted from the support's first frame; the workgroup finds its recording by a search over the recordings' first
//                      pieces.  It takes the piece in sub-tiles of 16 frames: the 16 rows z_f are converted once and staged in LDS
//                      [16][S] (a pair with a non-finite value among its P + Q becomes a row of zeros, the 1 included: 0 * NaN is not
//                      zero), their values fetched into registers a sub-tile ahead, under the MFMAs; both operands of v_mfma_f64_16x16x4_f64 are read from that image: the frames are K, four per
//                      instruction; lane (c = lane & 15, k = lane >> 4) holds z[4 s + k][16 tile + c] for A and for B alike.  The M x M
//                      output is NT x NT tiles of 16 x 16 (M rounded up to 16, the padding columns zero); only tiles with column >= row
//                      are computed.  A wave owns the row tiles ta and NT - 1 - ta against all their column tiles (NT + 1 tiles, the same
//                      for every wave) with the accumulators in registers for the whole piece; a row block is four waves.  S, the row
//                      stride in doubles, is 16 mod 32: the 32 lanes that ds_read_b64 serves together read two frames, 16 columns each, on
//                      disjoint banks.  The piece's tiles go to the staging slot's device block.
// ape_fit_sums_fold    grid (recordings, chunks of 256 entries): entry (i, j) is the piece records' element (min, max) in piece order from
//                      +0.0, so (i, j) and (j, i) hold the same bits; the two counts from [P, P] and the support's length.  A recording
//                      without a support gets its zeros here: the call writes all of acc_dev with no memset.
// No atomics, no workgroup waits for another, no inline assembly.  The f64 C/D map is col = lane & 15, row = (lane >> 4) + 4 reg.
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

using ape_scoredev::find_rec;

constexpr int FS_BLOCK = 256, FS_WAVES = FS_BLOCK / 64;
constexpr int FS_TILE = 16;                             // frames of a sub-tile: four MFMA steps
constexpr long long FS_MAX_PART_BYTES = 1LL << 30;

static_assert(APE_FIT_PIECE % FS_TILE == 0, "whole sub-tiles but the last");

typedef double f64x4 __attribute__((ext_vector_type(4)));

struct FitParams {
    const void* x;
    const void* t;
    const int* sup_lo;                                  // [R] first frame of the support
    const int* sup_len;                                 // [R] frames of the support (0: none)
    const int* lag;                                     // [R]
    const int* piece_at;                                // [R + 1] first piece of the recording; [R] = pieces
    const double* shift;                                // [Q]
    const double* scale;                                // [Q]
    double* part;                                       // [pieces, NT (NT + 1) / 2, 16, 16]
    double* acc;                                        // [R, M * M + 2]
    long long xs, ts;
    int R, P, Q, M, NT, S;
};

__host__ __device__ constexpr int fs_stride(int NT) { return (NT & 1) ? 16 * NT : 16 * NT + 16; }       // 16 mod 32, >= 16 NT
__host__ __device__ constexpr int fs_tile_at(int NT, int ti, int tj) { return ti * NT - ti * (ti - 1) / 2 + (tj - ti); }   // ti <= tj
__host__ __device__ constexpr size_t fs_lds_bytes(int NT) { return (size_t)FS_TILE * fs_stride(NT) * sizeof(double) + 2 * FS_TILE * sizeof(int); }
static_assert(fs_lds_bytes(19) <= 40 * 1024, "under the static limit at M = 289");

__device__ __forceinline__ bool fin(double v) { return fabs(v) <= 1.7976931348623157e308; }

// NA: column tiles of a wave's first row tile at most (NT); NB: of its second ((NT + 1) / 2)
template <typename TX, typename TT, int NA, int NB>
__global__ __launch_bounds__(FS_BLOCK) void ape_fit_sums_kernel(const FitParams p) {
    extern __shared__ double fs_mem[];                  // z [16][S] | bad int [2][16]
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int piece = blockIdx.x;
    const int NT = p.NT, S = p.S, P = p.P, W = 16 * NT;
    double* zt = fs_mem;
    int* bad = reinterpret_cast<int*>(fs_mem + FS_TILE * S);

    const int r = find_rec(p.piece_at, p.R, piece);
    const int j0 = piece - p.piece_at[r];
    const long long f0 = (long long)p.sup_lo[r] + (long long)j0 * APE_FIT_PIECE;
    const int left = p.sup_len[r] - j0 * APE_FIT_PIECE;     // >= 1
    const int n = left < APE_FIT_PIECE ? left : APE_FIT_PIECE;
    const long long lag = p.lag[r];
    const TX* xsrc = static_cast<const TX*>(p.x);
    const TT* tsrc = static_cast<const TT*>(p.t);

    // the wave's job: row tiles ta and tb = NT - 1 - ta (one tile where they meet); jobs past the middle have nothing to do
    const int job = (int)blockIdx.y * FS_WAVES + wave;
    const int ta = job, tb = NT - 1 - job;
    const bool work = ta <= tb, two = ta < tb;
    const int na = NT - ta;                             // column tiles NT - 1 - e, e < na, of row ta; e <= ta of row tb

    f64x4 acc_a[NA], acc_b[NB];
#pragma unroll
    for (int e = 0; e < NA; ++e) acc_a[e] = f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int e = 0; e < NB; ++e) acc_b[e] = f64x4{0.0, 0.0, 0.0, 0.0};
    const int c = lane & 15, k = lane >> 4;

    // A sub-tile's values are fetched into registers a sub-tile ahead, all loads of a thread in flight together and under the MFMAs of
    // the sub-tile before: x element tid + 256 i (frame e / P, column e % P: a wave reads runs of a row), t element tid + 256 j
    constexpr int XI = APE_FIT_MAX_P / 16, TJ = (FS_TILE * APE_FIT_MAX_Q + FS_BLOCK - 1) / FS_BLOCK;
    const int ni = P / 16, Q = p.Q, extra = W - P - Q;  // extra: the column of ones and the padding behind t, 1 .. 16
    TX xv[XI];
    TT tv[TJ];
    auto fetch = [&](int t0) {
        const int nt = n - t0 < FS_TILE ? n - t0 : FS_TILE;
#pragma unroll
        for (int i = 0; i < XI; ++i) {
            const int e = (int)threadIdx.x + FS_BLOCK * i, fr = e / P, col = e - fr * P;
            xv[i] = (TX)0;
            if (i < ni && fr < nt) xv[i] = xsrc[(f0 + t0 + fr) * p.xs + col];
        }
#pragma unroll
        for (int j = 0; j < TJ; ++j) {
            const int e = (int)threadIdx.x + FS_BLOCK * j, fr = e / Q, q = e - fr * Q;
            tv[j] = (TT)0;
            if (fr < nt) tv[j] = tsrc[(f0 + t0 + fr - lag) * p.ts + q];      // (fr < nt <= 16 bounds e below 16 Q)
        }
    };
    if (threadIdx.x < 2 * FS_TILE) bad[threadIdx.x] = 0;
    fetch(0);

    for (int t0 = 0; t0 < n; t0 += FS_TILE) {           // (uniform)
        const int nt = n - t0 < FS_TILE ? n - t0 : FS_TILE;
        int* flag = bad + ((t0 / FS_TILE) & 1) * FS_TILE;   // this sub-tile's flags; the other half is cleared for the next
        __syncthreads();                                // the sub-tile before has been read (first round: the flags are cleared)
#pragma unroll
        for (int i = 0; i < XI; ++i) {
            if (i < ni) {
                const int e = (int)threadIdx.x + FS_BLOCK * i, fr = e / P, col = e - fr * P;
                const double v = (double)xv[i];
                if (!fin(v)) flag[fr] = 1;              // (every writer writes 1)
                zt[fr * S + col] = v;
            }
        }
#pragma unroll
        for (int j = 0; j < TJ; ++j) {
            const int e = (int)threadIdx.x + FS_BLOCK * j, fr = e / Q, q = e - fr * Q;
            if (fr < FS_TILE) {
                const double raw = (double)tv[j];       // judged as it lies, and again under shift and scale
                const double v = fr < nt ? (raw - p.shift[q]) / p.scale[q] : 0.0;
                if (!fin(raw) || !fin(v)) flag[fr] = 1;
                zt[fr * S + P + 1 + q] = v;
            }
        }
        {                                               // the column of ones, the padding columns
            const int fr = (int)threadIdx.x >> 4, cc = (int)threadIdx.x & 15;
            if (cc < extra) zt[fr * S + (cc == 0 ? P : P + Q + cc)] = (cc == 0 && fr < nt) ? 1.0 : 0.0;
        }
        __syncthreads();
        for (int e = threadIdx.x; e < FS_TILE * W; e += FS_BLOCK) {     // a pair left out: exact zeros, its 1 included
            const int fr = e / W, col = e - fr * W;
            if (flag[fr]) zt[fr * S + col] = 0.0;
        }
        if (threadIdx.x < FS_TILE) bad[(((t0 / FS_TILE) & 1) ^ 1) * FS_TILE + threadIdx.x] = 0;
        __syncthreads();
        if (t0 + FS_TILE < n) fetch(t0 + FS_TILE);
        if (work) {                                     // (wave-uniform; no barrier inside)
#pragma unroll
            for (int s = 0; s < FS_TILE / 4; ++s) {
                const double* row = zt + (4 * s + k) * S + c;
                const double a_a = row[16 * ta], a_b = row[16 * tb];
#pragma unroll
                for (int e = 0; e < NA; ++e) {
                    if (e < na) {
                        const double b = row[16 * (NT - 1 - e)];
                        acc_a[e] = __builtin_amdgcn_mfma_f64_16x16x4f64(a_a, b, acc_a[e], 0, 0, 0);
                        constexpr int NBL = NB - 1;     // (e beyond NB is never a column of row tb: the index is clamped for the compiler alone)
                        if (e < NB && two && e <= ta)
                            acc_b[e < NB ? e : NBL] = __builtin_amdgcn_mfma_f64_16x16x4f64(a_b, b, acc_b[e < NB ? e : NBL], 0, 0, 0);
                    }
                }
            }
        }
    }

    if (!work) return;
    // tile (ti, tj), element (row q + 4 i, column c): 16 lanes write 16 consecutive doubles
    const size_t tiles = (size_t)NT * (NT + 1) / 2;
    double* rec = p.part + (size_t)piece * tiles * 256;
#pragma unroll
    for (int e = 0; e < NA; ++e) {
        if (e < na) {
            double* dst = rec + (size_t)fs_tile_at(NT, ta, NT - 1 - e) * 256;
#pragma unroll
            for (int i = 0; i < 4; ++i) dst[(k + 4 * i) * 16 + c] = acc_a[e][i];
        }
    }
#pragma unroll
    for (int e = 0; e < NB; ++e) {
        if (two && e <= ta) {
            double* dst = rec + (size_t)fs_tile_at(NT, tb, NT - 1 - e) * 256;
#pragma unroll
            for (int i = 0; i < 4; ++i) dst[(k + 4 * i) * 16 + c] = acc_b[e][i];
        }
    }
}

__global__ __launch_bounds__(FS_BLOCK) void ape_fit_sums_fold(const FitParams p) {
    const int r = blockIdx.x;
    const long long cells = (long long)p.M * p.M + 2;
    const long long e = (long long)blockIdx.y * FS_BLOCK + threadIdx.x;
    if (e >= cells) return;
    const bool count = e >= cells - 2;
    const int i = count ? p.P : (int)(e / p.M), j = count ? p.P : (int)(e - (long long)i * p.M);
    const int a = i < j ? i : j, b = i < j ? j : i;     // the element that was computed: row <= column
    const size_t tiles = (size_t)p.NT * (p.NT + 1) / 2;
    const int p0 = p.piece_at[r], p1 = p.piece_at[r + 1];
    const double* src = p.part + ((size_t)p0 * tiles + (size_t)fs_tile_at(p.NT, a >> 4, b >> 4)) * 256 + (a & 15) * 16 + (b & 15);
    double acc = 0.0;
#pragma unroll 4
    for (int q = p0; q < p1; ++q, src += tiles * 256) acc = acc + *src;     // in piece order
    double* out = p.acc + (size_t)r * (size_t)cells;
    if (!count) out[e] = acc;
    else if (e == cells - 2) out[e] = acc;              // pairs summed: the sum of their ones, exact
    else out[e] = (double)p.sup_len[r] - acc;           // pairs left out
}

// the staging of a call: supports, lags and first pieces, shift and scale, and behind them the piece records (score_host.h)
ApeSlotPool g_pool("fit_sums");

int check_side(const char* who, const char* side, const void* dev, int32_t dtype, int32_t width, int64_t stride, int32_t F, long long* extent) {
    if (dtype != APE_F32 && dtype != APE_F64) return ape_fail(APE_ERR_INVALID_ARG, "%s: unknown %s dtype selector %d", who, side, dtype);
    if (stride < width) return ape_fail(APE_ERR_INVALID_ARG, "%s: %s_stride %lld below the %d columns", who, side, (long long)stride, width);
    const long long esize = dtype == APE_F32 ? 4 : 8;
    long long ext = 0;
    if (__builtin_mul_overflow((long long)(F - 1), (long long)stride, &ext) || __builtin_add_overflow(ext, (long long)width, &ext) ||
        __builtin_mul_overflow(ext, esize, &ext))
        return ape_fail(APE_ERR_INVALID_ARG, "%s: the extent of %s does not fit 63 bits", who, side);
    if ((uintptr_t)dev & (uintptr_t)(esize - 1)) return ape_fail(APE_ERR_INVALID_ARG, "%s: %s_dev is not aligned to its element", who, side);
    *extent = ext;
    return APE_OK;
}

template <typename TX, typename TT>
void launch_fit(const FitParams& p, dim3 grid, size_t lds, hipStream_t st) {
    if (p.NT <= 11) hipLaunchKernelGGL((ape_fit_sums_kernel<TX, TT, 11, 6>), grid, dim3(FS_BLOCK), lds, st, p);
    else hipLaunchKernelGGL((ape_fit_sums_kernel<TX, TT, 19, 10>), grid, dim3(FS_BLOCK), lds, st, p);
}

}  // namespace

int ape_fit_sums(const void* x_dev, int64_t x_stride, int32_t x_dtype, int32_t P, const void* t_dev, int64_t t_stride, int32_t t_dtype,
                 int32_t Q, const double* t_shift_host, const double* t_scale_host, int32_t F, const int32_t* seg_starts_host, int32_t R,
                 int32_t skip, const int32_t* rec_lag_host, double* acc_dev, void* stream) {
    const char* who = "fit_sums";
    if (!x_dev || !t_dev || !seg_starts_host || !acc_dev) return ape_fail(APE_ERR_INVALID_ARG, "%s: NULL argument", who);
    if (P < 16 || P > APE_FIT_MAX_P || (P & 15)) return ape_fail(APE_ERR_INVALID_ARG, "%s: P %d, a multiple of 16 in 16 .. %d", who, P, APE_FIT_MAX_P);
    if (Q < 1 || Q > APE_FIT_MAX_Q) return ape_fail(APE_ERR_INVALID_ARG, "%s: Q %d, between 1 and %d", who, Q, APE_FIT_MAX_Q);
    if (int rc = ape_check_segments(who, F, seg_starts_host, R)) return rc;
    if (skip < 0) return ape_fail(APE_ERR_INVALID_ARG, "%s: skip %d is negative", who, skip);
    long long xext = 0, text = 0;
    if (int rc = check_side(who, "x", x_dev, x_dtype, P, x_stride, F, &xext)) return rc;
    if (int rc = check_side(who, "t", t_dev, t_dtype, Q, t_stride, F, &text)) return rc;
    for (int q = 0; q < Q; ++q) {
        if (t_shift_host && !std::isfinite(t_shift_host[q])) return ape_fail(APE_ERR_INVALID_ARG, "%s: t_shift[%d] = %g is not finite", who, q, t_shift_host[q]);
        if (t_scale_host && (!std::isfinite(t_scale_host[q]) || t_scale_host[q] == 0.0))
            return ape_fail(APE_ERR_INVALID_ARG, "%s: t_scale[%d] = %g (finite and not zero)", who, q, t_scale_host[q]);
    }
    int nl = 0, back = 0, fwd = 0;
    if (int rc = ape_check_lag_sweep(who, 0, 0, rec_lag_host, R, &nl, &back, &fwd)) return rc;
    if ((uintptr_t)acc_dev & 7u) return ape_fail(APE_ERR_INVALID_ARG, "%s: acc_dev is not aligned to its element", who);
    const int M = P + 1 + Q, NT = (M + 15) / 16;
    const long long cells = (long long)M * M + 2;
    const uintptr_t aa = (uintptr_t)acc_dev, ab = aa + (uintptr_t)((long long)R * cells) * sizeof(double);     // (2^31 * 83523 * 8 < 2^63)
    const uintptr_t xa = (uintptr_t)x_dev, ta = (uintptr_t)t_dev;
    if (xa < ab && aa < xa + (uintptr_t)xext) return ape_fail(APE_ERR_INVALID_ARG, "%s: acc_dev overlaps x_dev", who);
    if (ta < ab && aa < ta + (uintptr_t)text) return ape_fail(APE_ERR_INVALID_ARG, "%s: acc_dev overlaps t_dev", who);
    // the supports and their pieces: frames f >= s + skip of the recording [s, e) whose pair f - l lies in [s, e)
    long long pieces = 0;
    for (int r = 0; r < R; ++r) {
        const long long s = seg_starts_host[r], e = r + 1 < R ? seg_starts_host[r + 1] : F, l = rec_lag_host ? rec_lag_host[r] : 0;
        const long long lo = s + (skip > l ? skip : l), up = e + (l < 0 ? l : 0);
        if (up > lo) pieces += (up - lo + APE_FIT_PIECE - 1) / APE_FIT_PIECE;
    }
    const long long tiles = (long long)NT * (NT + 1) / 2;
    const long long part_bytes = pieces * tiles * 256 * (long long)sizeof(double);       // (2^31 / 512 + 2^31 pieces at most: < 2^63)
    if (part_bytes > FS_MAX_PART_BYTES)
        return ape_fail(APE_ERR_INVALID_ARG, "%s: %lld bytes of piece records (%lld pieces of %d frames), at most %lld", who, part_bytes, pieces,
                        APE_FIT_PIECE, FS_MAX_PART_BYTES);
    const hipStream_t st = (hipStream_t)stream;
    if (int rc = ape_check_not_capturing(st, who, "host arrays are staged per call")) return rc;
    int device = 0;
    APE_SCORE_TRY(g_pool.prefix, hipGetDevice(&device));

    const size_t ints_bytes = (((size_t)R * 4 + 1) * sizeof(int) + 7) & ~(size_t)7;      // sup_lo [R], sup_len [R], lag [R], piece_at [R + 1]
    const size_t host_bytes = ints_bytes + 2 * (size_t)Q * sizeof(double);               // then shift [Q], scale [Q]

    std::lock_guard<std::mutex> lock(g_pool.mu);
    ApeSlot* slot = nullptr;
    if (int rc = g_pool.take(device, host_bytes, host_bytes + (size_t)part_bytes, &slot)) return rc;
    char* pin = static_cast<char*>(slot->pinned);
    int* sup_lo = reinterpret_cast<int*>(pin);
    int* sup_len = sup_lo + R;
    int* lag = sup_len + R;
    int* piece_at = lag + R;
    int at = 0;
    for (int r = 0; r < R; ++r) {
        const long long s = seg_starts_host[r], e = r + 1 < R ? seg_starts_host[r + 1] : F, l = rec_lag_host ? rec_lag_host[r] : 0;
        const long long lo = s + (skip > l ? skip : l), up = e + (l < 0 ? l : 0);
        const bool any = up > lo;
        sup_lo[r] = any ? (int)lo : 0;
        sup_len[r] = any ? (int)(up - lo) : 0;
        lag[r] = (int)l;
        piece_at[r] = at;
        at += any ? (int)((up - lo + APE_FIT_PIECE - 1) / APE_FIT_PIECE) : 0;
    }
    piece_at[R] = at;
    double* ss = reinterpret_cast<double*>(pin + ints_bytes);
    for (int q = 0; q < Q; ++q) { ss[q] = t_shift_host ? t_shift_host[q] : 0.0; ss[Q + q] = t_scale_host ? t_scale_host[q] : 1.0; }
    // (a copy that fails leaves through finish() like a launch that fails: the slot's event is recorded either way)
    hipError_t e = hipMemcpyAsync(slot->dev, slot->pinned, host_bytes, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return g_pool.finish(who, slot, e, st);

    FitParams p{};
    char* dev = static_cast<char*>(slot->dev);
    p.x = x_dev; p.t = t_dev;
    p.sup_lo = reinterpret_cast<const int*>(dev);
    p.sup_len = p.sup_lo + R;
    p.lag = p.sup_len + R;
    p.piece_at = p.lag + R;
    p.shift = reinterpret_cast<const double*>(dev + ints_bytes);
    p.scale = p.shift + Q;
    p.part = reinterpret_cast<double*>(dev + host_bytes);
    p.acc = acc_dev;
    p.xs = x_stride; p.ts = t_stride;
    p.R = R; p.P = P; p.Q = Q; p.M = M; p.NT = NT; p.S = fs_stride(NT);

    if (pieces > 0) {
        const int jobs = (NT + 1) / 2;                  // pairs of row tiles
        const dim3 grid((unsigned)pieces, (unsigned)((jobs + FS_WAVES - 1) / FS_WAVES));
        const size_t lds = fs_lds_bytes(NT);
        const bool x32 = x_dtype == APE_F32, t32 = t_dtype == APE_F32;
        if (x32 && t32) launch_fit<float, float>(p, grid, lds, st);
        else if (x32) launch_fit<float, double>(p, grid, lds, st);
        else if (t32) launch_fit<double, float>(p, grid, lds, st);
        else launch_fit<double, double>(p, grid, lds, st);
        e = hipGetLastError();
        if (e != hipSuccess) return g_pool.finish(who, slot, e, st);
    }
    hipLaunchKernelGGL(ape_fit_sums_fold, dim3((unsigned)R, (unsigned)((cells + FS_BLOCK - 1) / FS_BLOCK)), dim3(FS_BLOCK), 0, st, p);
    return g_pool.finish(who, slot, hipGetLastError(), st);
}
