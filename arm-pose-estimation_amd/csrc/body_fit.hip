// Each recording's arm lengths and shoulder origin against the truth (ape_body_sums, ape_rebody_rows; the reference has
// no counterpart).  Every position of a message is forward kinematics of its own quaternions through nine numbers (larm_vec, uarm_vec,
// uarm_orig): elbow = R_h o + R_u v_u, hand = elbow + R_l v_l.  The body enters linearly, so the least-squares body of a recording solves
// a 9 x 9 system whose entries are sums over the frames (score.py: best_body); ape_body_sums takes those sums for every lag of a sweep in
// one pass, ape_rebody_rows rewrites the positions of replay rows under the body found.
//
// ape_body_sums_kernel      the shape of ape_frame_sums_kernel (frame_fit.hip): 256 frames per workgroup, one lane per message frame;
//                           every truth row the workgroup's frames can be paired with -- its own 256 and the halo, at most 512 -- is
//                           converted to a 19-value pose exactly once and kept in LDS.  APE_BODY_ROT_MSG: a lane forms the matrices of
//                           its message's three quaternions and their 27 product terms once, then walks the L lags, where only the 17
//                           terms with the truth's positions are formed and all 44 are masked.  APE_BODY_ROT_TRUTH: the single lag 0,
//                           the matrices are those of the paired truth row.  One partial record per (workgroup, recording, lag).
// ape_body_sums_acc_kernel  one workgroup per (recording, lag): its partial records combined in a fixed order.
// ape_rebody_rows_kernel    one lane per frame, one wave per workgroup: the four quaternions copied, the three origins made again from
//                           them and the recording's body.
//
// Sums: no atomics and no shuffles.  A wave's 64 x 46 terms are transposed through LDS in two halves (27 + 19 columns, stride 27): lane c
// adds column c over the wave's frames in frame order and cuts at recording boundaries (a wave-uniform ballot mask); across the four
// waves in wave order, across workgroups in the order of ape_body_sums_acc_kernel: the same inputs give the same bits.  The helpers the
// scoring kernels share are score_device.h's, the staging slots and argument checks score_host.h's.  float64 with separate roundings
// for a * b + c, like the numpy statement (score.py): contraction is off in this file.
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

constexpr int BF_BLOCK = 256, BF_WAVES = BF_BLOCK / 64;
constexpr int ACCW = APE_BODY_ACC_WIDTH;
constexpr int BF_HALF_A = 27, BF_HALF_B = ACCW - BF_HALF_A;   // the products of the rotations; the position terms, the norms and the counts
constexpr int BF_TSTRIDE = 27;                          // stride of a frame's terms in the transposition buffer; odd
constexpr int BF_WINDOW = BF_BLOCK + 2 * APE_SCORE_MAX_LAG;

static_assert(BF_HALF_B <= BF_TSTRIDE && STAGE_COLS <= BF_TSTRIDE, "the transposition buffer also stages the input rows");
static_assert(BF_HALF_A <= 64 && ACCW <= 64, "one lane per column");

struct BodyParams {
    const void* msg;                                    // NULL with APE_BODY_ROT_TRUTH
    const void* truth;
    double* part;                                       // [(workgroups + R), L, 46] partial records, pair (b, r) at rows (b + r) * L ..
    const int* starts;                                  // [R]
    const int* offs;                                    // [R] the recordings' offsets o_r
    long long msg_stride;
    int F, R, skip, layout, truth_w;
    int lag_min, L;
    int back, fwd;                                      // how far below / above its own rows a workgroup's truth window reaches, each <= 128
};

// out[3 a + b] = sum_k x[3 k + a] y[3 k + b]: X' Y, row-major
__device__ __forceinline__ void mat_atb(const double* x, const double* y, double* out) {
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) out[3 * a + b] = x[a] * y[b] + x[3 + a] * y[3 + b] + x[6 + a] * y[6 + b];
}

// out[a] = sum_k x[3 k + a] t[k]: X' t
__device__ __forceinline__ void mat_atv(const double* x, const double* t, double* out) {
#pragma unroll
    for (int a = 0; a < 3; ++a) out[a] = x[a] * t[0] + x[3 + a] * t[1] + x[6 + a] * t[2];
}

// the three matrices Rm[0:9], Rm[9:18], Rm[18:27] of the lower-arm, upper-arm and hips quaternions at q, q + 4 (and q + 8 with hips; the
// identity without) and their products Pm = R_l'R_u, R_l'R_h, R_u'R_h
__device__ __forceinline__ void rotations_and_products(const double* ql, const double* qu, const double* qh, bool hips, double* Rm, double* Pm) {
    quat_matrix(ql, Rm); quat_matrix(qu, Rm + 9);
    if (hips) {
        quat_matrix(qh, Rm + 18);
    } else {
#pragma unroll
        for (int c = 0; c < 9; ++c) Rm[18 + c] = (c == 0 || c == 4 || c == 8) ? 1.0 : 0.0;
    }
    mat_atb(Rm, Rm + 9, Pm); mat_atb(Rm, Rm + 18, Pm + 9); mat_atb(Rm + 9, Rm + 18, Pm + 18);
}

template <typename TM, typename TT, int KIND, int ROT>
__global__ __launch_bounds__(BF_BLOCK) void ape_body_sums_kernel(const BodyParams p) {
    __shared__ double tbuf[BF_WAVES][64 * BF_TSTRIDE];  // input staging, then the transposition buffer of the wave's terms
    __shared__ double poses[BF_WINDOW * POSE];
    __shared__ double wfirst[BF_WAVES][ACCW];
    __shared__ int wrec[BF_WAVES][2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long tile0 = (long long)blockIdx.x * BF_BLOCK;
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

    // ---- truth poses of the window [wlo, whi), 256 rows a round, each row converted once ----
    const long long wlo = tile0 - p.back > 0 ? tile0 - p.back : 0;
    const long long whi = tile0 + BF_BLOCK + p.fwd < (long long)p.F ? tile0 + BF_BLOCK + p.fwd : (long long)p.F;
    const int tw = p.truth_w, tls = tw | 1;
    for (long long base = wlo; base < whi; base += BF_BLOCK) {                         // (uniform; at most twice)
        const long long r0 = base + wave * 64, lw = whi - r0;
        const int nr = lw >= 64 ? 64 : (lw > 0 ? (int)lw : 0);
        if (nr > 0) stage_rows(lds, static_cast<const TT*>(p.truth), (long long)tw, tw, tls, r0, nr, lane);
        __syncthreads();
        const bool tv = lane < nr;
        double t[21];
#pragma unroll
        for (int c = 0; c < 21; ++c) t[c] = (tv && c < tw) ? lds[lane * tls + c] : 0.0;
        __syncthreads();
        // Target rows carry their positions: the host refuses the two layouts whose positions would be made with the body being fitted,
        // so the layout of a target row is stated here, and the body truth_pose takes is nine zeros: in that layout it reaches no pose value
        const int tl = KIND == APE_TRUTH_TARGETS ? (int)APE_LAYOUT_ORI_POS_CAL_LARM_UARM_HIPS : p.layout;
        const double no_body[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (tv) truth_pose<KIND>(t, tw, tl, no_body, poses + (size_t)(r0 + lane - wlo) * POSE);
    }

    // ---- APE_BODY_ROT_MSG: the message's three matrices and their products, formed once and held over the lags ----
    const bool hips = p.layout != APE_LAYOUT_ORI_CAL_LARM_UARM;
    bool ok_m = valid;
    double Rm[27], Pm[27];
    if constexpr (ROT == APE_BODY_ROT_MSG) {
        if (nrows > 0) stage_rows(lds, static_cast<const TM*>(p.msg), p.msg_stride, 25, 25, row0, nrows, lane);
        __syncthreads();                                // (also: every pose is written)
        double q[12];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            q[c] = valid ? lds[lane * 25 + 7 + c] : 0.0;
            q[4 + c] = valid ? lds[lane * 25 + 14 + c] : 0.0;
            q[8 + c] = (valid && hips) ? lds[lane * 25 + 21 + c] : 0.0;       // without hips columns 21:25 are not used
        }
#pragma unroll
        for (int c = 0; c < 12; ++c) ok_m = ok_m && fin(q[c]);
        rotations_and_products(q, q + 4, q + 8, hips, Rm, Pm);
    }
    const int prev = __shfl_up(rec, 1, 64);
    const unsigned long long bmask = __ballot(lane > 0 && rec != prev);
    if (lane == 0) wrec[wave][0] = rec;
    if (lane == 63) wrec[wave][1] = rec;
    __syncthreads();                                    // (the staged message is read; every pose and wrec are written)
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
        if constexpr (ROT == APE_BODY_ROT_TRUTH) rotations_and_products(t + 6, t + 10, t + 14, hips, Rm, Pm);
        double v[ACCW];
#pragma unroll
        for (int c = 0; c < 27; ++c) v[c] = Pm[c];
        mat_atv(Rm, t, v + 27); mat_atv(Rm + 9, t, v + 30); mat_atv(Rm + 18, t, v + 33);
        mat_atv(Rm + 9, t + 3, v + 36); mat_atv(Rm + 18, t + 3, v + 39);
        v[42] = t[0] * t[0] + t[1] * t[1] + t[2] * t[2];
        v[43] = t[3] * t[3] + t[4] * t[4] + t[5] * t[5];
        bool in = sup && ok_m && ex && t[18] != 0.0;
#pragma unroll
        for (int c = 0; c < 44; ++c) in = in && fin(v[c]);
#pragma unroll
        for (int c = 0; c < 44; ++c) v[c] = in ? v[c] : 0.0;
        v[44] = in ? 1.0 : 0.0;
        v[45] = (sup && !in) ? 1.0 : 0.0;

        double* part_row0 = p.part + ((size_t)blockIdx.x * (size_t)p.L + (size_t)j) * ACCW;       // + r * rec_step: the pair (b, r)
        double held_a = 0.0, held_b = 0.0;
        bool holds = false;
        int held_rec = -1;
#pragma unroll
        for (int c = 0; c < BF_HALF_A; ++c) lds[lane * BF_TSTRIDE + c] = v[c];
        __syncthreads();
        sum_columns<BF_TSTRIDE, BF_WAVES>(lds, BF_HALF_A, 0, rec, bmask, lane, wave, p.R, prev_last, wfirst[wave], part_row0, rec_step, &held_a, &holds, &held_rec);
        __syncthreads();
#pragma unroll
        for (int c = 0; c < BF_HALF_B; ++c) lds[lane * BF_TSTRIDE + c] = v[BF_HALF_A + c];
        __syncthreads();
        sum_columns<BF_TSTRIDE, BF_WAVES>(lds, BF_HALF_B, BF_HALF_A, rec, bmask, lane, wave, p.R, prev_last, wfirst[wave], part_row0, rec_step, &held_b, &holds, &held_rec);
        __syncthreads();                                // (every wave's leading run is in wfirst; the buffer is free for the next lag)
        // the wave whose last run starts a (workgroup, recording) pair takes the following waves' leading runs in wave order
        if (holds) {                                    // (uniform)
            for (int w = wave + 1; w < BF_WAVES; ++w) {
                if (wrec[w][0] != held_rec) break;
                if (lane < BF_HALF_A) held_a = held_a + wfirst[w][lane];
                if (lane < BF_HALF_B) held_b = held_b + wfirst[w][BF_HALF_A + lane];
                if (wrec[w][1] != held_rec) break;
            }
            double* dst = part_row0 + (size_t)held_rec * rec_step;
            if (lane < BF_HALF_A) dst[lane] = held_a;
            if (lane < BF_HALF_B) dst[BF_HALF_A + lane] = held_b;
        }
    }
}

// workgroup (r, j): recording r at sweep index j, its pairs (b, r) at rows (b + r) * L + j.  Thread (g, c): column c of the pairs
// g, g + 4, ... in order; then the four groups in order.
__global__ __launch_bounds__(BF_BLOCK) void ape_body_sums_acc_kernel(const double* __restrict__ part, const int* __restrict__ starts, int R, int F,
                                                                     int L, double* __restrict__ acc) {
    sums_acc<ACCW, BF_BLOCK>(part, starts, R, F, L, acc);
}

// ---- ape_rebody_rows ---------------------------------------------------------------------------------------------------------------------
struct RebodyParams {
    const void* msg;
    void* out;                                          // [F, 25]
    const int* starts;                                  // [R]
    const double* bodies;                               // [n_bodies, 9]
    long long msg_stride;
    int F, R, n_bodies, out_f32, hips;
};

template <typename TM>
__global__ __launch_bounds__(64) void ape_rebody_rows_kernel(const RebodyParams p) {
    __shared__ double lds[64 * 25];
    const int lane = threadIdx.x;
    const long long row0 = (long long)blockIdx.x * 64;
    const long long f = row0 + lane;
    const bool valid = f < p.F;
    const long long left = (long long)p.F - row0;
    const int nrows = left >= 64 ? 64 : (int)left;      // (>= 1: the grid covers F)

    const int rec = (valid && p.n_bodies > 1) ? find_rec(p.starts, p.R, f) : 0;
    const double* body = p.bodies + 9 * (size_t)rec;
    const Vec3 larm_vec{body[0], body[1], body[2]}, uarm_vec{body[3], body[4], body[5]}, uarm_orig{body[6], body[7], body[8]};

    stage_rows(lds, static_cast<const TM*>(p.msg), p.msg_stride, 25, 25, row0, nrows, lane);
    __syncthreads();
    double o[25];
#pragma unroll
    for (int c = 0; c < 25; ++c) o[c] = valid ? lds[lane * 25 + c] : 0.0;
    __syncthreads();

    // (compose_msg.py:59-61, 92-93) the shoulder, the elbow behind it, the hand behind the elbow
    Vec3 uo = uarm_orig;
    if (p.hips) uo = qrot(Quat{o[21], o[22], o[23], o[24]}, uarm_orig);
    const Vec3 r1 = qrot(Quat{o[14], o[15], o[16], o[17]}, uarm_vec);
    const Vec3 el{r1.x + uo.x, r1.y + uo.y, r1.z + uo.z};
    const Vec3 r2 = qrot(Quat{o[7], o[8], o[9], o[10]}, larm_vec);
    o[18] = uo.x; o[19] = uo.y; o[20] = uo.z;
    o[11] = el.x; o[12] = el.y; o[13] = el.z;
    o[4] = r2.x + el.x; o[5] = r2.y + el.y; o[6] = r2.z + el.z;

    // through LDS so that the wave writes its 64 x 25 values as one run
#pragma unroll
    for (int c = 0; c < 25; ++c) lds[lane * 25 + c] = o[c];
    __syncthreads();
    const int total = nrows * 25;
#pragma unroll
    for (int it = 0; it < 25; ++it) {
        const int idx = it * 64 + lane;
        if (idx < total) {
            const size_t at = (size_t)row0 * 25 + idx;
            if (p.out_f32) static_cast<float*>(p.out)[at] = (float)lds[idx];
            else static_cast<double*>(p.out)[at] = lds[idx];
        }
    }
}

// the staging of both entries: the host arrays in, the partial records behind them (score_host.h)
ApeSlotPool g_pool("body_fit");

template <typename TM, typename TT>
void launch_sums_msg(const BodyParams& p, int kind, unsigned blocks, hipStream_t st) {
    if (kind == APE_TRUTH_TARGETS)
        hipLaunchKernelGGL((ape_body_sums_kernel<TM, TT, APE_TRUTH_TARGETS, APE_BODY_ROT_MSG>), dim3(blocks), dim3(BF_BLOCK), 0, st, p);
    else hipLaunchKernelGGL((ape_body_sums_kernel<TM, TT, APE_TRUTH_EST, APE_BODY_ROT_MSG>), dim3(blocks), dim3(BF_BLOCK), 0, st, p);
}

template <typename TT>
void launch_sums_truth(const BodyParams& p, int kind, unsigned blocks, hipStream_t st) {      // (no message is read: one message type)
    if (kind == APE_TRUTH_TARGETS)
        hipLaunchKernelGGL((ape_body_sums_kernel<double, TT, APE_TRUTH_TARGETS, APE_BODY_ROT_TRUTH>), dim3(blocks), dim3(BF_BLOCK), 0, st, p);
    else hipLaunchKernelGGL((ape_body_sums_kernel<double, TT, APE_TRUTH_EST, APE_BODY_ROT_TRUTH>), dim3(blocks), dim3(BF_BLOCK), 0, st, p);
}

}  // namespace

int ape_body_sums(int32_t layout, const void* msg_dev, int32_t msg_stride, int32_t msg_dtype, const void* truth_dev, int32_t truth_kind,
                  int32_t truth_dtype, int32_t F, const int32_t* seg_starts_host, int32_t R, int32_t skip, int32_t rot_source,
                  int32_t lag_min, int32_t lag_max, const int32_t* rec_lag_host, double* acc_dev, void* stream) {
    const char* who = "body_sums";
    if (rot_source != APE_BODY_ROT_MSG && rot_source != APE_BODY_ROT_TRUTH)
        return ape_fail(APE_ERR_INVALID_ARG, "%s: unknown rotation source %d", who, rot_source);
    const bool from_msg = rot_source == APE_BODY_ROT_MSG;
    if ((from_msg && !msg_dev) || !truth_dev || !seg_starts_host || !acc_dev) return ape_fail(APE_ERR_INVALID_ARG, "%s: NULL argument", who);
    if (!ape_scoring_layout(layout)) return ape_fail(APE_ERR_INVALID_ARG, "%s: layout %d has no pose to fit", who, layout);
    if (truth_kind != APE_TRUTH_TARGETS && truth_kind != APE_TRUTH_EST) return ape_fail(APE_ERR_INVALID_ARG, "%s: unknown truth kind %d", who, truth_kind);
    if (truth_kind == APE_TRUTH_TARGETS && layout != APE_LAYOUT_ORI_POS_CAL_LARM_UARM_HIPS)
        return ape_fail(APE_ERR_INVALID_ARG, "%s: target truth of layout %d: its positions would be made with the body being fitted (give est rows)",
                        who, layout);
    if ((msg_dtype != APE_F32 && msg_dtype != APE_F64) || (truth_dtype != APE_F32 && truth_dtype != APE_F64))
        return ape_fail(APE_ERR_INVALID_ARG, "%s: unknown dtype selector", who);
    if (int rc = ape_check_segments(who, F, seg_starts_host, R)) return rc;
    if (msg_dev && msg_stride < 25) return ape_fail(APE_ERR_INVALID_ARG, "%s: msg_stride %d below 25", who, msg_stride);
    if (skip < 0) return ape_fail(APE_ERR_INVALID_ARG, "%s: skip %d is negative", who, skip);
    int L = 0, back = 0, fwd = 0;
    if (!from_msg) {                                    // (the sweep without recordings first: its shape is judged before this source's rule)
        if (int rc = ape_check_lag_sweep(who, lag_min, lag_max, nullptr, 0, &L, &back, &fwd)) return rc;
        if (lag_min != 0 || lag_max != 0)
            return ape_fail(APE_ERR_INVALID_ARG, "%s: rotations from the truth: the sweep must be the single lag 0, got %d .. %d", who, lag_min, lag_max);
        if (rec_lag_host) return ape_fail(APE_ERR_INVALID_ARG, "%s: rotations from the truth: rec_lag_host must be NULL", who);
    }
    if (int rc = ape_check_lag_sweep(who, lag_min, lag_max, rec_lag_host, R, &L, &back, &fwd)) return rc;
    const hipStream_t st = (hipStream_t)stream;
    if (int rc = ape_check_not_capturing(st, who, "host arrays are staged per call")) return rc;
    int device = 0;
    APE_SCORE_TRY(g_pool.prefix, hipGetDevice(&device));

    const unsigned blocks = (unsigned)(((long long)F + BF_BLOCK - 1) / BF_BLOCK);
    const size_t starts_bytes = (((size_t)R * sizeof(int)) + 7) & ~(size_t)7;       // starts, then the offsets
    const size_t host_bytes = 2 * starts_bytes;
    const size_t part_bytes = ((size_t)blocks + (size_t)R) * (size_t)L * ACCW * sizeof(double);

    std::lock_guard<std::mutex> lock(g_pool.mu);
    ApeSlot* slot = nullptr;
    if (int rc = g_pool.take(device, host_bytes, host_bytes + part_bytes, &slot)) return rc;
    char* pin = static_cast<char*>(slot->pinned);
    memcpy(pin, seg_starts_host, (size_t)R * sizeof(int));
    if (rec_lag_host) memcpy(pin + starts_bytes, rec_lag_host, (size_t)R * sizeof(int));
    else memset(pin + starts_bytes, 0, (size_t)R * sizeof(int));
    APE_SCORE_TRY(g_pool.prefix, hipMemcpyAsync(slot->dev, slot->pinned, host_bytes, hipMemcpyHostToDevice, st));

    BodyParams p{};
    char* dev = static_cast<char*>(slot->dev);
    p.msg = from_msg ? msg_dev : nullptr; p.truth = truth_dev;
    p.starts = reinterpret_cast<const int*>(dev);
    p.offs = reinterpret_cast<const int*>(dev + starts_bytes);
    p.part = reinterpret_cast<double*>(dev + host_bytes);
    p.msg_stride = msg_stride;
    p.F = F; p.R = R; p.skip = skip; p.layout = layout;
    p.truth_w = ape_truth_width(layout, truth_kind);
    p.lag_min = lag_min; p.L = L;
    p.back = back; p.fwd = fwd;

    if (!from_msg) {
        if (truth_dtype == APE_F32) launch_sums_truth<float>(p, truth_kind, blocks, st);
        else launch_sums_truth<double>(p, truth_kind, blocks, st);
    } else if (msg_dtype == APE_F32 && truth_dtype == APE_F32) launch_sums_msg<float, float>(p, truth_kind, blocks, st);
    else if (msg_dtype == APE_F32) launch_sums_msg<float, double>(p, truth_kind, blocks, st);
    else if (truth_dtype == APE_F32) launch_sums_msg<double, float>(p, truth_kind, blocks, st);
    else launch_sums_msg<double, double>(p, truth_kind, blocks, st);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) {
        hipLaunchKernelGGL(ape_body_sums_acc_kernel, dim3((unsigned)R, (unsigned)L), dim3(BF_BLOCK), 0, st, p.part, p.starts, R, F, L, acc_dev);
        e = hipGetLastError();
    }
    return g_pool.finish(who, slot, e, st);
}

int ape_rebody_rows(int32_t layout, const void* msg_dev, int32_t msg_stride, int32_t msg_dtype, int32_t F, const int32_t* seg_starts_host,
                    int32_t R, const double* bodies_host, int32_t n_bodies, void* out_dev, int32_t out_dtype, void* stream) {
    const char* who = "rebody_rows";
    if (!msg_dev || !seg_starts_host || !bodies_host || !out_dev) return ape_fail(APE_ERR_INVALID_ARG, "%s: NULL argument", who);
    if (!ape_scoring_layout(layout)) return ape_fail(APE_ERR_INVALID_ARG, "%s: layout %d has no pose to rebuild", who, layout);
    if (layout == APE_LAYOUT_ORI_POS_CAL_LARM_UARM_HIPS)
        return ape_fail(APE_ERR_INVALID_ARG, "%s: layout %d: its positions are predicted, not made from a body", who, layout);
    if ((msg_dtype != APE_F32 && msg_dtype != APE_F64) || (out_dtype != APE_F32 && out_dtype != APE_F64))
        return ape_fail(APE_ERR_INVALID_ARG, "%s: unknown dtype selector", who);
    if (int rc = ape_check_segments(who, F, seg_starts_host, R)) return rc;
    if (msg_stride < 25) return ape_fail(APE_ERR_INVALID_ARG, "%s: msg_stride %d below 25", who, msg_stride);
    if (n_bodies != 1 && n_bodies != R) return ape_fail(APE_ERR_INVALID_ARG, "%s: n_bodies %d is neither 1 nor R = %d", who, n_bodies, R);
    if (out_dev == msg_dev) return ape_fail(APE_ERR_INVALID_ARG, "%s: out_dev aliases the input", who);
    const hipStream_t st = (hipStream_t)stream;
    if (int rc = ape_check_not_capturing(st, who, "host arrays are staged per call")) return rc;
    int device = 0;
    APE_SCORE_TRY(g_pool.prefix, hipGetDevice(&device));

    const unsigned blocks = (unsigned)(((long long)F + 63) / 64);
    const size_t bodies_bytes = (size_t)n_bodies * 9 * sizeof(double);              // the bodies, then the starts
    const size_t host_bytes = bodies_bytes + (size_t)R * sizeof(int);

    std::lock_guard<std::mutex> lock(g_pool.mu);
    ApeSlot* slot = nullptr;
    if (int rc = g_pool.take(device, host_bytes, host_bytes, &slot)) return rc;
    char* pin = static_cast<char*>(slot->pinned);
    memcpy(pin, bodies_host, bodies_bytes);
    memcpy(pin + bodies_bytes, seg_starts_host, (size_t)R * sizeof(int));
    APE_SCORE_TRY(g_pool.prefix, hipMemcpyAsync(slot->dev, slot->pinned, host_bytes, hipMemcpyHostToDevice, st));

    RebodyParams p{};
    char* dev = static_cast<char*>(slot->dev);
    p.msg = msg_dev; p.out = out_dev;
    p.bodies = reinterpret_cast<const double*>(dev);
    p.starts = reinterpret_cast<const int*>(dev + bodies_bytes);
    p.msg_stride = msg_stride;
    p.F = F; p.R = R; p.n_bodies = n_bodies; p.out_f32 = out_dtype == APE_F32 ? 1 : 0;
    p.hips = layout != APE_LAYOUT_ORI_CAL_LARM_UARM ? 1 : 0;
    if (msg_dtype == APE_F32) hipLaunchKernelGGL(ape_rebody_rows_kernel<float>, dim3(blocks), dim3(64), 0, st, p);
    else hipLaunchKernelGGL(ape_rebody_rows_kernel<double>, dim3(blocks), dim3(64), 0, st, p);
    return g_pool.finish(who, slot, hipGetLastError(), st);
}
