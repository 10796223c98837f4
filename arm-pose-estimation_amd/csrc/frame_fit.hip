// Each recording's heading and frame offset against the truth (ape_frame_sums, ape_rotate_rows; the reference has no
// counterpart).  For a world-side rotation G with truth ~ G . estimate, the least-squares G of a recording is read off a handful of sums
// of 3x3 products (score.py: best_frame); ape_frame_sums takes those sums for every lag of a sweep in one pass, ape_rotate_rows applies
// the rotation found to replay rows.
//
// ape_frame_sums_kernel      256 frames per workgroup, one lane per message frame, the window of ape_score_lags_kernel (score.hip): every
//                            truth row the workgroup's frames can be paired with -- its own 256 and the halo, at most 512 -- is converted
//                            to a 19-value pose exactly once and kept in LDS.  A lane forms the matrices of its message's three quaternions
//                            once, then walks the L lags: the truth's matrices from the pose of row f - l, the 51 terms of the pair.  One
//                            partial record per (workgroup, recording, lag).
// ape_frame_sums_acc_kernel  one workgroup per (recording, lag): its partial records combined in a fixed order.
// ape_rotate_rows_kernel     one lane per frame, one wave per workgroup: g (x) q for the four quaternions, G p for the three origins,
//                            G m and G S G' for a spread record.
//
// Sums: no atomics and no shuffles.  A wave's 64 x 51 terms are transposed through LDS in two halves (27 + 24 columns, stride 27): lane c
// adds column c over the wave's frames in frame order and cuts at recording boundaries (the boundaries are a wave-uniform ballot mask, so
// the walk has no divergence); across the four waves in wave order, across workgroups in the order of ape_frame_sums_acc_kernel: the same
// inputs give the same bits.  Loads are staged as in score.hip (lanes run along the rows); every staged stride is odd.
//
// The helpers the scoring kernels share (row staging, truth row -> pose, the column sums, the ordered sum of the partial records) are
// score_device.h's, the staging slots and argument checks score_host.h's.
// float64 with separate roundings for a * b + c, like the numpy statement (score.py): contraction is off in this file.
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

constexpr int FF_BLOCK = 256, FF_WAVES = FF_BLOCK / 64;
constexpr int ACCW = APE_FRAME_ACC_WIDTH;
constexpr int FF_HALF_A = 27, FF_HALF_B = ACCW - FF_HALF_A;   // the rotation blocks; the position blocks, the norms and the counts
constexpr int FF_TSTRIDE = 27;                          // stride of a frame's terms in the transposition buffer; odd
constexpr int FF_WINDOW = FF_BLOCK + 2 * APE_SCORE_MAX_LAG;
constexpr int RR_OUT_STRIDE = 25 + APE_SPREAD_WIDTH + 1;      // LDS stride of a rotated row (46 values at most); odd

static_assert(FF_HALF_B <= FF_TSTRIDE && STAGE_COLS <= FF_TSTRIDE, "the transposition buffer also stages the input rows");

struct FrameParams {
    const void* msg;
    const void* truth;
    double* part;                                       // [(workgroups + R), L, 51] partial records, pair (b, r) at rows (b + r) * L ..
    const int* starts;                                  // [R]
    const int* offs;                                    // [R] the recordings' offsets o_r
    const double* bodies;                               // [n_bodies, 9] (APE_TRUTH_TARGETS)
    long long msg_stride;
    int F, R, skip, layout, n_bodies, truth_w;
    int lag_min, L;
    int back, fwd;                                      // how far below / above its own rows a workgroup's truth window reaches, each <= 128
};

// out[3 a + b] = sum_k t[3 a + k] e[3 b + k]: T E', row-major
__device__ __forceinline__ void mat_abt(const double* t, const double* e, double* out) {
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) out[3 * a + b] = t[3 * a] * e[3 * b] + t[3 * a + 1] * e[3 * b + 1] + t[3 * a + 2] * e[3 * b + 2];
}

template <typename TM, typename TT, int KIND>
__global__ __launch_bounds__(FF_BLOCK) void ape_frame_sums_kernel(const FrameParams p) {
    __shared__ double tbuf[FF_WAVES][64 * FF_TSTRIDE];  // input staging, then the transposition buffer of the wave's terms
    __shared__ double poses[FF_WINDOW * POSE];
    __shared__ double wfirst[FF_WAVES][ACCW];
    __shared__ int wrec[FF_WAVES][2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long tile0 = (long long)blockIdx.x * FF_BLOCK;
    const long long row0 = tile0 + wave * 64;
    const long long f = row0 + lane;
    const bool valid = f < p.F;
    const long long left = (long long)p.F - row0;
    const int nrows = left >= 64 ? 64 : (left > 0 ? (int)left : 0);
    double* lds = tbuf[wave];

    // the frame's recording [start, end) and offset; lanes past F form a recording of their own
    int rec = p.R, start = 0, end = 0, off = 0;
    if (valid) {
        rec = find_rec(p.starts, p.R, f);
        start = p.starts[rec];
        end = rec + 1 < p.R ? p.starts[rec + 1] : p.F;
        off = p.offs[rec];
    }

    // ---- truth poses of the window [wlo, whi), 256 rows a round, each row converted once with its own recording's body ----
    const long long wlo = tile0 - p.back > 0 ? tile0 - p.back : 0;
    const long long whi = tile0 + FF_BLOCK + p.fwd < (long long)p.F ? tile0 + FF_BLOCK + p.fwd : (long long)p.F;
    const int tw = p.truth_w, tls = tw | 1;
    for (long long base = wlo; base < whi; base += FF_BLOCK) {                         // (uniform; at most twice)
        const long long r0 = base + wave * 64, lw = whi - r0;
        const int nr = lw >= 64 ? 64 : (lw > 0 ? (int)lw : 0);
        if (nr > 0) stage_rows(lds, static_cast<const TT*>(p.truth), (long long)tw, tw, tls, r0, nr, lane);
        __syncthreads();
        const bool tv = lane < nr;
        double t[21];
#pragma unroll
        for (int c = 0; c < 21; ++c) t[c] = (tv && c < tw) ? lds[lane * tls + c] : 0.0;
        __syncthreads();
        if (tv) {
            const long long tr = r0 + lane;
            const int trec = (KIND == APE_TRUTH_TARGETS && p.n_bodies > 1) ? find_rec(p.starts, p.R, tr) : 0;
            truth_pose<KIND>(t, tw, p.layout, p.bodies + 9 * (size_t)trec, poses + (size_t)(tr - wlo) * POSE);
        }
    }

    // ---- the message: its three matrices, two origins and their squares, formed once and held over the lags ----
    const bool hips = p.layout != APE_LAYOUT_ORI_CAL_LARM_UARM;
    bool ok_m = valid;
    if (nrows > 0) stage_rows(lds, static_cast<const TM*>(p.msg), p.msg_stride, 25, 25, row0, nrows, lane);
    __syncthreads();                                    // (also: every pose is written)
    double E[27], eh[3], ee[3];
    {
        double m[25];
#pragma unroll
        for (int c = 0; c < 25; ++c) { m[c] = valid ? lds[lane * 25 + c] : 0.0; ok_m = ok_m && fin(m[c]); }
        quat_matrix(m + 7, E); quat_matrix(m + 14, E + 9); quat_matrix(m + 21, E + 18);
#pragma unroll
        for (int k = 0; k < 3; ++k) { eh[k] = m[4 + k]; ee[k] = m[11 + k]; }
    }
    const double eh2 = eh[0] * eh[0] + eh[1] * eh[1] + eh[2] * eh[2], ee2 = ee[0] * ee[0] + ee[1] * ee[1] + ee[2] * ee[2];
    const int prev = __shfl_up(rec, 1, 64);
    const unsigned long long bmask = __ballot(lane > 0 && rec != prev);
    if (lane == 0) wrec[wave][0] = rec;
    if (lane == 63) wrec[wave][1] = rec;
    __syncthreads();                                    // (the staged message is read; wrec is written)
    const int prev_last = wave > 0 ? wrec[wave - 1][1] : -1;

    // the support: past the skipped frames, and paired at every lag of the sweep
    const int l_lo = off + p.lag_min, l_hi = l_lo + p.L - 1;
    const bool sup = valid && (f - start) >= (long long)p.skip && f - l_hi >= (long long)start && f - l_lo < (long long)end;
    const size_t rec_step = (size_t)p.L * ACCW;

    for (int j = 0; j < p.L; ++j) {                     // (uniform)
        const long long tr = f - (l_lo + j);
        const bool ex = valid && tr >= (long long)start && tr < (long long)end;        // the pair exists: tr is inside [wlo, whi)
        const double* ps = poses + (ex ? (size_t)(tr - wlo) : 0) * POSE;
        double t[POSE];
#pragma unroll
        for (int c = 0; c < POSE; ++c) t[c] = ex ? ps[c] : 0.0;
        double T[9], v[ACCW];
        quat_matrix(t + 6, T); mat_abt(T, E, v);
        quat_matrix(t + 10, T); mat_abt(T, E + 9, v + 9);
        if (hips) {
            quat_matrix(t + 14, T); mat_abt(T, E + 18, v + 18);
        } else {
#pragma unroll
            for (int c = 18; c < 27; ++c) v[c] = 0.0;
        }
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) { v[27 + 3 * a + b] = t[a] * eh[b]; v[36 + 3 * a + b] = t[3 + a] * ee[b]; }
        v[45] = t[0] * t[0] + t[1] * t[1] + t[2] * t[2];
        v[46] = eh2;
        v[47] = t[3] * t[3] + t[4] * t[4] + t[5] * t[5];
        v[48] = ee2;
        bool in = sup && ok_m && ex && t[18] != 0.0;
#pragma unroll
        for (int c = 0; c < 49; ++c) in = in && fin(v[c]);
#pragma unroll
        for (int c = 0; c < 49; ++c) v[c] = in ? v[c] : 0.0;
        v[49] = in ? 1.0 : 0.0;
        v[50] = (sup && !in) ? 1.0 : 0.0;

        double* part_row0 = p.part + ((size_t)blockIdx.x * (size_t)p.L + (size_t)j) * ACCW;       // + r * rec_step: the pair (b, r)
        double held_a = 0.0, held_b = 0.0;
        bool holds = false;
        int held_rec = -1;
#pragma unroll
        for (int c = 0; c < FF_HALF_A; ++c) lds[lane * FF_TSTRIDE + c] = v[c];
        __syncthreads();
        sum_columns<FF_TSTRIDE, FF_WAVES>(lds, FF_HALF_A, 0, rec, bmask, lane, wave, p.R, prev_last, wfirst[wave], part_row0, rec_step, &held_a, &holds, &held_rec);
        __syncthreads();
#pragma unroll
        for (int c = 0; c < FF_HALF_B; ++c) lds[lane * FF_TSTRIDE + c] = v[FF_HALF_A + c];
        __syncthreads();
        sum_columns<FF_TSTRIDE, FF_WAVES>(lds, FF_HALF_B, FF_HALF_A, rec, bmask, lane, wave, p.R, prev_last, wfirst[wave], part_row0, rec_step, &held_b, &holds, &held_rec);
        __syncthreads();                                // (every wave's leading run is in wfirst; the buffer is free for the next lag)
        // the wave whose last run starts a (workgroup, recording) pair takes the following waves' leading runs in wave order
        if (holds) {                                    // (uniform)
            for (int w = wave + 1; w < FF_WAVES; ++w) {
                if (wrec[w][0] != held_rec) break;
                if (lane < FF_HALF_A) held_a = held_a + wfirst[w][lane];
                if (lane < FF_HALF_B) held_b = held_b + wfirst[w][FF_HALF_A + lane];
                if (wrec[w][1] != held_rec) break;
            }
            double* dst = part_row0 + (size_t)held_rec * rec_step;
            if (lane < FF_HALF_A) dst[lane] = held_a;
            if (lane < FF_HALF_B) dst[FF_HALF_A + lane] = held_b;
        }
    }
}

// workgroup (r, j): recording r at sweep index j, its pairs (b, r) at rows (b + r) * L + j.  Thread (g, c): column c of the pairs
// g, g + 4, ... in order; then the four groups in order.
__global__ __launch_bounds__(FF_BLOCK) void ape_frame_sums_acc_kernel(const double* __restrict__ part, const int* __restrict__ starts, int R, int F,
                                                                      int L, double* __restrict__ acc) {
    sums_acc<ACCW, FF_BLOCK>(part, starts, R, F, L, acc);
}

// ---- ape_rotate_rows ---------------------------------------------------------------------------------------------------------------------
struct RotateParams {
    const void* msg;
    const void* spread;                                 // or NULL
    void* out;                                          // [F, 25] or [F, 46]
    const int* starts;                                  // [R]
    const double* quats;                                // [n_quats, 4] unit quaternions
    long long msg_stride, spread_stride;
    int F, R, n_quats, out_f32;
};

template <typename TM, bool SPR>
__global__ __launch_bounds__(64) void ape_rotate_rows_kernel(const RotateParams p) {
    constexpr int OW = SPR ? 25 + APE_SPREAD_WIDTH : 25;
    constexpr int OS = SPR ? RR_OUT_STRIDE : 25;        // odd
    __shared__ double lds[64 * OS];
    const int lane = threadIdx.x;
    const long long row0 = (long long)blockIdx.x * 64;
    const long long f = row0 + lane;
    const bool valid = f < p.F;
    const long long left = (long long)p.F - row0;
    const int nrows = left >= 64 ? 64 : (int)left;      // (>= 1: the grid covers F)

    const int rec = (valid && p.n_quats > 1) ? find_rec(p.starts, p.R, f) : 0;
    const double* gq = p.quats + 4 * (size_t)rec;
    const Quat g{gq[0], gq[1], gq[2], gq[3]};
    double G[9];
    quat_matrix(gq, G);

    stage_rows(lds, static_cast<const TM*>(p.msg), p.msg_stride, 25, 25, row0, nrows, lane);
    __syncthreads();
    double m[25];
#pragma unroll
    for (int c = 0; c < 25; ++c) m[c] = valid ? lds[lane * 25 + c] : 0.0;
    __syncthreads();
    double s[APE_SPREAD_WIDTH];
    if constexpr (SPR) {
        stage_rows(lds, static_cast<const TM*>(p.spread), p.spread_stride, APE_SPREAD_WIDTH, APE_SPREAD_WIDTH, row0, nrows, lane);
        __syncthreads();
#pragma unroll
        for (int c = 0; c < APE_SPREAD_WIDTH; ++c) s[c] = valid ? lds[lane * APE_SPREAD_WIDTH + c] : 0.0;
        __syncthreads();
    }

    double o[OW];
#pragma unroll
    for (int k = 0; k < 4; ++k) {                       // the quaternions at 0, 7, 14, 21: g (x) q
        const int c = 7 * k;
        const Quat q = qmul(g, Quat{m[c], m[c + 1], m[c + 2], m[c + 3]});
        o[c] = q.w; o[c + 1] = q.x; o[c + 2] = q.y; o[c + 3] = q.z;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {                       // the origins at 4, 11, 18: G p
        const int c = 4 + 7 * k;
#pragma unroll
        for (int a = 0; a < 3; ++a) o[c + a] = G[3 * a] * m[c] + G[3 * a + 1] * m[c + 1] + G[3 * a + 2] * m[c + 2];
    }
    if constexpr (SPR) {
#pragma unroll
        for (int k = 0; k < 2; ++k) {                   // mean and covariance of the hand at 0, of the elbow at 9
            const double* r = s + 9 * k;
            double* d = o + 25 + 9 * k;
#pragma unroll
            for (int a = 0; a < 3; ++a) d[a] = G[3 * a] * r[0] + G[3 * a + 1] * r[1] + G[3 * a + 2] * r[2];
            const double S[9] = {r[3], r[4], r[5], r[4], r[6], r[7], r[5], r[7], r[8]};
            double A[9];                                // G S
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int b = 0; b < 3; ++b) A[3 * a + b] = G[3 * a] * S[b] + G[3 * a + 1] * S[3 + b] + G[3 * a + 2] * S[6 + b];
            int e = 3;
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int b = a; b < 3; ++b) d[e++] = A[3 * a] * G[3 * b] + A[3 * a + 1] * G[3 * b + 1] + A[3 * a + 2] * G[3 * b + 2];      // (G S) G'
        }
#pragma unroll
        for (int c = 18; c < APE_SPREAD_WIDTH; ++c) o[25 + c] = s[c];
    }

    // through LDS so that the wave writes its 64 x OW values as one run
#pragma unroll
    for (int c = 0; c < OW; ++c) lds[lane * OS + c] = o[c];
    __syncthreads();
    const int total = nrows * OW;
#pragma unroll
    for (int it = 0; it < OW; ++it) {
        const int idx = it * 64 + lane;
        if (idx < total) {
            const int r = idx / OW, c = idx - r * OW;
            const size_t at = (size_t)row0 * OW + idx;
            if (p.out_f32) static_cast<float*>(p.out)[at] = (float)lds[r * OS + c];
            else static_cast<double*>(p.out)[at] = lds[r * OS + c];
        }
    }
}

// the staging of both entries: the host arrays in, the partial records behind them (score_host.h)
ApeSlotPool g_pool("frame_fit");

template <typename TM, typename TT>
void launch_sums(const FrameParams& p, int kind, unsigned blocks, hipStream_t st) {
    if (kind == APE_TRUTH_TARGETS) hipLaunchKernelGGL((ape_frame_sums_kernel<TM, TT, APE_TRUTH_TARGETS>), dim3(blocks), dim3(FF_BLOCK), 0, st, p);
    else hipLaunchKernelGGL((ape_frame_sums_kernel<TM, TT, APE_TRUTH_EST>), dim3(blocks), dim3(FF_BLOCK), 0, st, p);
}

template <typename TM>
void launch_rotate(const RotateParams& p, unsigned blocks, hipStream_t st) {
    if (p.spread != nullptr) hipLaunchKernelGGL((ape_rotate_rows_kernel<TM, true>), dim3(blocks), dim3(64), 0, st, p);
    else hipLaunchKernelGGL((ape_rotate_rows_kernel<TM, false>), dim3(blocks), dim3(64), 0, st, p);
}

}  // namespace

int ape_frame_sums(int32_t layout, const void* msg_dev, int32_t msg_stride, int32_t msg_dtype, const void* truth_dev, int32_t truth_kind,
                   int32_t truth_dtype, int32_t F, const int32_t* seg_starts_host, int32_t R, int32_t skip, const double* bodies_host,
                   int32_t n_bodies, int32_t lag_min, int32_t lag_max, const int32_t* rec_lag_host, double* acc_dev, void* stream) {
    const char* who = "frame_sums";
    if (!msg_dev || !truth_dev || !seg_starts_host || !bodies_host || !acc_dev) return ape_fail(APE_ERR_INVALID_ARG, "%s: NULL argument", who);
    if (!ape_scoring_layout(layout)) return ape_fail(APE_ERR_INVALID_ARG, "%s: layout %d has no pose to score", who, layout);
    if (truth_kind != APE_TRUTH_TARGETS && truth_kind != APE_TRUTH_EST) return ape_fail(APE_ERR_INVALID_ARG, "%s: unknown truth kind %d", who, truth_kind);
    if ((msg_dtype != APE_F32 && msg_dtype != APE_F64) || (truth_dtype != APE_F32 && truth_dtype != APE_F64))
        return ape_fail(APE_ERR_INVALID_ARG, "%s: unknown dtype selector", who);
    if (int rc = ape_check_segments(who, F, seg_starts_host, R)) return rc;
    if (msg_stride < 25) return ape_fail(APE_ERR_INVALID_ARG, "%s: msg_stride %d below 25", who, msg_stride);
    if (skip < 0) return ape_fail(APE_ERR_INVALID_ARG, "%s: skip %d is negative", who, skip);
    if (n_bodies != 1 && n_bodies != R) return ape_fail(APE_ERR_INVALID_ARG, "%s: n_bodies %d is neither 1 nor R = %d", who, n_bodies, R);
    int L = 0, back = 0, fwd = 0;
    if (int rc = ape_check_lag_sweep(who, lag_min, lag_max, rec_lag_host, R, &L, &back, &fwd)) return rc;
    const hipStream_t st = (hipStream_t)stream;
    if (int rc = ape_check_not_capturing(st, who, "host arrays are staged per call")) return rc;
    int device = 0;
    APE_SCORE_TRY(g_pool.prefix, hipGetDevice(&device));

    const unsigned blocks = (unsigned)(((long long)F + FF_BLOCK - 1) / FF_BLOCK);
    const size_t starts_bytes = (((size_t)R * sizeof(int)) + 7) & ~(size_t)7;       // starts, then the offsets, then the bodies
    const size_t bodies_bytes = (size_t)n_bodies * 9 * sizeof(double);
    const size_t host_bytes = 2 * starts_bytes + bodies_bytes;
    const size_t part_bytes = ((size_t)blocks + (size_t)R) * (size_t)L * ACCW * sizeof(double);

    std::lock_guard<std::mutex> lock(g_pool.mu);
    ApeSlot* slot = nullptr;
    if (int rc = g_pool.take(device, host_bytes, host_bytes + part_bytes, &slot)) return rc;
    char* pin = static_cast<char*>(slot->pinned);
    memcpy(pin, seg_starts_host, (size_t)R * sizeof(int));
    if (rec_lag_host) memcpy(pin + starts_bytes, rec_lag_host, (size_t)R * sizeof(int));
    else memset(pin + starts_bytes, 0, (size_t)R * sizeof(int));
    memcpy(pin + 2 * starts_bytes, bodies_host, bodies_bytes);
    APE_SCORE_TRY(g_pool.prefix, hipMemcpyAsync(slot->dev, slot->pinned, host_bytes, hipMemcpyHostToDevice, st));

    FrameParams p{};
    char* dev = static_cast<char*>(slot->dev);
    p.msg = msg_dev; p.truth = truth_dev;
    p.starts = reinterpret_cast<const int*>(dev);
    p.offs = reinterpret_cast<const int*>(dev + starts_bytes);
    p.bodies = reinterpret_cast<const double*>(dev + 2 * starts_bytes);
    p.part = reinterpret_cast<double*>(dev + host_bytes);
    p.msg_stride = msg_stride;
    p.F = F; p.R = R; p.skip = skip; p.layout = layout; p.n_bodies = n_bodies;
    p.truth_w = ape_truth_width(layout, truth_kind);
    p.lag_min = lag_min; p.L = L;
    p.back = back; p.fwd = fwd;

    if (msg_dtype == APE_F32 && truth_dtype == APE_F32) launch_sums<float, float>(p, truth_kind, blocks, st);
    else if (msg_dtype == APE_F32) launch_sums<float, double>(p, truth_kind, blocks, st);
    else if (truth_dtype == APE_F32) launch_sums<double, float>(p, truth_kind, blocks, st);
    else launch_sums<double, double>(p, truth_kind, blocks, st);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) {
        hipLaunchKernelGGL(ape_frame_sums_acc_kernel, dim3((unsigned)R, (unsigned)L), dim3(FF_BLOCK), 0, st, p.part, p.starts, R, F, L, acc_dev);
        e = hipGetLastError();
    }
    return g_pool.finish(who, slot, e, st);
}

int ape_rotate_rows(int32_t layout, const void* msg_dev, int32_t msg_stride, const void* spread_dev, int32_t spread_stride, int32_t msg_dtype,
                    int32_t F, const int32_t* seg_starts_host, int32_t R, const double* quats_host, int32_t n_quats, void* out_dev,
                    int32_t out_dtype, void* stream) {
    const char* who = "rotate_rows";
    if (!msg_dev || !seg_starts_host || !quats_host || !out_dev) return ape_fail(APE_ERR_INVALID_ARG, "%s: NULL argument", who);
    if (!ape_scoring_layout(layout)) return ape_fail(APE_ERR_INVALID_ARG, "%s: layout %d has no pose to rotate", who, layout);
    if ((msg_dtype != APE_F32 && msg_dtype != APE_F64) || (out_dtype != APE_F32 && out_dtype != APE_F64))
        return ape_fail(APE_ERR_INVALID_ARG, "%s: unknown dtype selector", who);
    if (int rc = ape_check_segments(who, F, seg_starts_host, R)) return rc;
    if (msg_stride < 25) return ape_fail(APE_ERR_INVALID_ARG, "%s: msg_stride %d below 25", who, msg_stride);
    if (spread_dev && spread_stride < APE_SPREAD_WIDTH) return ape_fail(APE_ERR_INVALID_ARG, "%s: spread_stride %d below %d", who, spread_stride, APE_SPREAD_WIDTH);
    if (n_quats != 1 && n_quats != R) return ape_fail(APE_ERR_INVALID_ARG, "%s: n_quats %d is neither 1 nor R = %d", who, n_quats, R);
    if (out_dev == msg_dev || out_dev == spread_dev) return ape_fail(APE_ERR_INVALID_ARG, "%s: out_dev aliases an input", who);
    std::vector<double> unit((size_t)n_quats * 4);
    for (int r = 0; r < n_quats; ++r) {
        const double* q = quats_host + 4 * (size_t)r;
        const double n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
        if (!std::isfinite(n) || !(n > 0.0)) return ape_fail(APE_ERR_INVALID_ARG, "%s: quaternion %d is zero or not finite", who, r);
        for (int k = 0; k < 4; ++k) unit[4 * (size_t)r + k] = q[k] / n;
    }
    const hipStream_t st = (hipStream_t)stream;
    if (int rc = ape_check_not_capturing(st, who, "host arrays are staged per call")) return rc;
    int device = 0;
    APE_SCORE_TRY(g_pool.prefix, hipGetDevice(&device));

    const unsigned blocks = (unsigned)(((long long)F + 63) / 64);
    const size_t quats_bytes = (size_t)n_quats * 4 * sizeof(double);                 // the quaternions, then the starts
    const size_t host_bytes = quats_bytes + (size_t)R * sizeof(int);

    std::lock_guard<std::mutex> lock(g_pool.mu);
    ApeSlot* slot = nullptr;
    if (int rc = g_pool.take(device, host_bytes, host_bytes, &slot)) return rc;
    char* pin = static_cast<char*>(slot->pinned);
    memcpy(pin, unit.data(), quats_bytes);
    memcpy(pin + quats_bytes, seg_starts_host, (size_t)R * sizeof(int));
    APE_SCORE_TRY(g_pool.prefix, hipMemcpyAsync(slot->dev, slot->pinned, host_bytes, hipMemcpyHostToDevice, st));

    RotateParams p{};
    char* dev = static_cast<char*>(slot->dev);
    p.msg = msg_dev; p.spread = spread_dev; p.out = out_dev;
    p.quats = reinterpret_cast<const double*>(dev);
    p.starts = reinterpret_cast<const int*>(dev + quats_bytes);
    p.msg_stride = msg_stride; p.spread_stride = spread_stride;
    p.F = F; p.R = R; p.n_quats = n_quats; p.out_f32 = out_dtype == APE_F32 ? 1 : 0;
    if (msg_dtype == APE_F32) launch_rotate<float>(p, blocks, st);
    else launch_rotate<double>(p, blocks, st);
    return g_pool.finish(who, slot, hipGetLastError(), st);
}
