// Scoring replayed poses against ground truth (ape_score_rows; over a sweep of time lags: ape_score_lags, 4.32, further
// down; the reference has no counterpart).
//
// ape_score_kernel      one lane per frame: the truth pose (est columns as given, or NN targets through the float64 forward kinematics of
//                       fk_device.h, its quaternions refined to the reference's eigenvector: score_device.h's truth_pose), the five errors of
//                       the frame's message against it, the two squared Mahalanobis distances under the frame's spread record; then the
//                       workgroup's 256 frames reduced per recording into one partial record for every (workgroup, recording) pair
// ape_score_acc_kernel  one workgroup per recording: its partial records combined in a fixed order
//
// Loads: a wave's 64 rows are fetched with the lanes running ALONG the rows (element i of the wave's rows x columns block is lane i % 64 of
// load i / 64), so every load instruction reads whole runs of 25 / 21 / O neighbouring values and the 6N values between the message and
// the record of a packed row are never touched; the block is staged in LDS and each lane then takes its own row from there.
// Sums: no atomics.  Within a wave a segmented shuffle tree (lane l takes lane l + 1, 2, 4, ... while that lane is in the same recording),
// across the four waves in wave order, across workgroups in the order of ape_score_acc_kernel: the same inputs give the same bits.
//
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

constexpr int SC_BLOCK = 256, SC_WAVES = SC_BLOCK / 64;
constexpr int SC_LDS_ROW = STAGE_COLS;                  // widest staged row (the message); every staged stride is odd: no bank conflicts
constexpr int ACC = APE_SCORE_ACC_WIDTH;
constexpr double CHI2_3_Q50 = 2.3659738843753377, CHI2_3_Q90 = 6.251388631170325;

struct ScoreParams {
    const void* msg;
    const void* spread;
    const void* truth;
    void* score;                                        // [F, 7] or NULL
    double* part;                                       // [(workgroups + R), 25] partial records, pair (b, r) at row b + r; NULL: no accumulators
    const int* starts;                                  // [R]
    const double* bodies;                               // [n_bodies, 9] (APE_TRUTH_TARGETS)
    long long msg_stride, spread_stride;
    int F, R, skip, layout, n_bodies, truth_w, score_f32;
};

__device__ __forceinline__ double dist3(const double* a, const Vec3 t) {
    const double dx = a[0] - t.x, dy = a[1] - t.y, dz = a[2] - t.z;
    return sqrt(dx * dx + dy * dy + dz * dz);
}

// 4 asin(min(1, |q - s qt| / 2)), s = -1 where q . qt < 0.0: well conditioned from 1e-9 rad to pi
__device__ __forceinline__ double ang_err(const double* q, const Quat t) {
    const double d = q[0] * t.w + q[1] * t.x + q[2] * t.y + q[3] * t.z;
    const double s = d < 0.0 ? -1.0 : 1.0;
    const double a = q[0] - s * t.w, b = q[1] - s * t.x, c = q[2] - s * t.y, e = q[3] - s * t.z;
    const double h = sqrt(a * a + b * b + c * c + e * e) / 2.0;
    return 4.0 * asin(h < 1.0 ? h : 1.0);
}

// (t - m)' S^-1 (t - m), S^-1 by the adjugate; NaN where the covariance is not usable (include/ape_hip.h)
__device__ __forceinline__ double mahalanobis(const double* rec, const Vec3 t) {
    const double a = rec[3], b = rec[4], c = rec[5], d = rec[6], e = rec[7], f = rec[8];
    const double tr = a + d + f;
    const double A00 = d * f - e * e, A01 = c * e - b * f, A02 = b * e - c * d;
    const double A11 = a * f - c * c, A12 = b * c - a * e, A22 = a * d - b * b;
    const double det = a * A00 + b * A01 + c * A02;
    const double third = tr / 3.0;
    const bool usable = fin(a) && fin(b) && fin(c) && fin(d) && fin(e) && fin(f) && tr > 0.0 && det > 1e-12 * (third * third * third);
    if (!usable) return NAN;
    const double x = t.x - rec[0], y = t.y - rec[1], z = t.z - rec[2];
    const double quad = A00 * x * x + A11 * y * y + A22 * z * z + 2.0 * (A01 * x * y + A02 * x * z + A12 * y * z);
    return quad / det;
}

__device__ __forceinline__ bool is_max_col(int c) { return c < 15 && c % 3 == 2; }

__device__ __forceinline__ void acc_combine(double* v, const double* o) {
#pragma unroll
    for (int c = 0; c < ACC; ++c) v[c] = is_max_col(c) ? fmax(v[c], o[c]) : v[c] + o[c];
}

template <typename TM, typename TT, int KIND, bool SPR>
__global__ __launch_bounds__(SC_BLOCK) void ape_score_kernel(const ScoreParams p) {
    __shared__ double stage[SC_WAVES][64 * SC_LDS_ROW];
    __shared__ double wfirst[SC_WAVES][ACC];
    __shared__ int wrec[SC_WAVES][2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long row0 = (long long)blockIdx.x * SC_BLOCK + wave * 64;
    const long long f = row0 + lane;
    const bool valid = f < p.F;
    const long long left = (long long)p.F - row0;
    const int nrows = left >= 64 ? 64 : (left > 0 ? (int)left : 0);
    double* lds = stage[wave];

    // the frame's recording: the last start <= f (starts[0] == 0, strictly rising); lanes past F form a recording of their own
    int rec = p.R, start = 0;
    if (valid) {
        rec = find_rec(p.starts, p.R, f);
        start = p.starts[rec];
    }

    // ---- truth pose ----
    // (every wave stages into its own slice of `stage`, so a wave-level wait would do between the phases; the workgroup barrier is the
    //  plain form of it and costs nothing measurable beside the loads)
    const int tw = p.truth_w, tls = tw | 1;
    if (nrows > 0) stage_rows(lds, static_cast<const TT*>(p.truth), (long long)tw, tw, tls, row0, nrows, lane);
    __syncthreads();
    double t[21];
#pragma unroll
    for (int c = 0; c < 21; ++c) t[c] = (valid && c < tw) ? lds[lane * tls + c] : 0.0;    // lanes past F, columns past tw: never-written LDS is not read
    __syncthreads();
    const bool hips = p.layout != APE_LAYOUT_ORI_CAL_LARM_UARM;
    // truth_pose's statements with `valid` at the head of the chain, not behind its flag: through truth_pose (ok = valid && pose[18] != 0.0)
    // the est-kind kernel with a spread record takes 176 VGPRs for 148 and loses a wave per SIMD (profiles/score_headers.md)
    Vec3 t_hand, t_elbow;
    Quat t_lq, t_uq, t_hq{1.0, 0.0, 0.0, 0.0};
    bool ok = valid;
    if constexpr (KIND == APE_TRUTH_TARGETS) {
#pragma unroll
        for (int c = 0; c < 20; ++c)
            if (c < tw) ok = ok && fin(t[c]);
        const TargetPose o = targets_to_pose(t, p.layout, p.bodies + 9 * (size_t)(p.n_bodies > 1 && valid ? rec : 0));
        t_hand = o.hand; t_elbow = o.elbow; t_lq = o.lq; t_uq = o.uq; t_hq = o.hq;
    } else {
        const int ql = hips ? 9 : 6, qu = hips ? 13 : 10;
        t_hand = Vec3{t[0], t[1], t[2]}; t_elbow = Vec3{t[3], t[4], t[5]};
        t_lq = Quat{t[ql], t[ql + 1], t[ql + 2], t[ql + 3]};
        t_uq = Quat{t[qu], t[qu + 1], t[qu + 2], t[qu + 3]};
        if (hips) t_hq = Quat{t[17], t[18], t[19], t[20]};
    }
    ok = ok && fin(t_hand.x) && fin(t_hand.y) && fin(t_hand.z) && fin(t_elbow.x) && fin(t_elbow.y) && fin(t_elbow.z) &&
         fin(t_lq.w) && fin(t_lq.x) && fin(t_lq.y) && fin(t_lq.z) && fin(t_uq.w) && fin(t_uq.x) && fin(t_uq.y) && fin(t_uq.z) &&
         fin(t_hq.w) && fin(t_hq.x) && fin(t_hq.y) && fin(t_hq.z);

    // ---- the message against it ----
    if (nrows > 0) stage_rows(lds, static_cast<const TM*>(p.msg), p.msg_stride, 25, 25, row0, nrows, lane);
    __syncthreads();
    double m[25];
#pragma unroll
    for (int c = 0; c < 25; ++c) { m[c] = valid ? lds[lane * 25 + c] : 0.0; ok = ok && fin(m[c]); }
    __syncthreads();
    double s[APE_SCORE_WIDTH];
    s[0] = dist3(m + 4, t_hand);
    s[1] = dist3(m + 11, t_elbow);
    s[2] = ang_err(m + 7, t_lq);
    s[3] = ang_err(m + 14, t_uq);
    s[4] = hips ? ang_err(m + 21, t_hq) : 0.0;
    s[5] = NAN; s[6] = NAN;
    if constexpr (SPR) {
        if (nrows > 0) stage_rows(lds, static_cast<const TM*>(p.spread), p.spread_stride, 21, 21, row0, nrows, lane);
        __syncthreads();
        double r18[18];
#pragma unroll
        for (int c = 0; c < 18; ++c) r18[c] = valid ? lds[lane * 21 + c] : 0.0;
        __syncthreads();
        s[5] = mahalanobis(r18, t_hand);
        s[6] = mahalanobis(r18 + 9, t_elbow);
    }
    if (!ok) {
#pragma unroll
        for (int c = 0; c < APE_SCORE_WIDTH; ++c) s[c] = NAN;
    }

    // ---- per-frame rows: through LDS so that the wave writes its 64 x 7 values as one run ----
    if (p.score != nullptr) {
#pragma unroll
        for (int c = 0; c < APE_SCORE_WIDTH; ++c) lds[lane * APE_SCORE_WIDTH + c] = s[c];
        __syncthreads();
        const int total = nrows * APE_SCORE_WIDTH;
#pragma unroll
        for (int it = 0; it < APE_SCORE_WIDTH; ++it) {
            const int idx = it * 64 + lane;
            if (idx < total) {
                const size_t o = (size_t)row0 * APE_SCORE_WIDTH + idx;
                if (p.score_f32) static_cast<float*>(p.score)[o] = (float)lds[idx];
                else static_cast<double*>(p.score)[o] = lds[idx];
            }
        }
    }
    if (p.part == nullptr) return;                      // (uniform)

    // ---- the frame's contribution, then the workgroup's frames per recording ----
    const bool past = valid && (f - start) >= (long long)p.skip;
    const bool in = past && ok;
    double v[ACC];
#pragma unroll
    for (int c = 0; c < 5; ++c) {
        const double e = in ? s[c] : 0.0;
        v[3 * c] = e; v[3 * c + 1] = e * e; v[3 * c + 2] = e;
    }
    v[15] = in ? 1.0 : 0.0;
    v[16] = (past && !ok) ? 1.0 : 0.0;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const double d2 = s[5 + k];
        const bool has = in && fin(d2);
        v[17 + 4 * k] = has ? 1.0 : 0.0;
        v[18 + 4 * k] = has ? d2 : 0.0;
        v[19 + 4 * k] = (has && d2 <= CHI2_3_Q50) ? 1.0 : 0.0;
        v[20 + 4 * k] = (has && d2 <= CHI2_3_Q90) ? 1.0 : 0.0;
    }
    // segmented tree: after the round with offset o, lane l holds the frames [l, l + 2 o) of its recording within the wave
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int orec = __shfl_down(rec, off, 64);
        const bool take = lane + off < 64 && orec == rec;
        double o[ACC];
#pragma unroll
        for (int c = 0; c < ACC; ++c) o[c] = __shfl_down(v[c], off, 64);
        if (take) acc_combine(v, o);
    }
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < ACC; ++c) wfirst[wave][c] = v[c];
        wrec[wave][0] = rec;
    }
    if (lane == 63) wrec[wave][1] = rec;
    __syncthreads();
    // the first frame of every (workgroup, recording) pair takes the following waves' leading pieces in wave order and writes the pair's record
    if (valid && (f == start || threadIdx.x == 0)) {
        if (wrec[wave][1] == rec) {
            for (int w = wave + 1; w < SC_WAVES; ++w) {
                if (wrec[w][0] != rec) break;
                acc_combine(v, wfirst[w]);
                if (wrec[w][1] != rec) break;
            }
        }
        double* dst = p.part + ((size_t)blockIdx.x + (size_t)rec) * ACC;
#pragma unroll
        for (int c = 0; c < ACC; ++c) dst[c] = v[c];
    }
}

// recording r = workgroup r: its pairs (b, r), b = first .. last workgroup of its frames, at rows b + r.  Thread (g, c): column c of the
// pairs g, g + 8, ... in order; then the eight groups in order.
__global__ __launch_bounds__(SC_BLOCK) void ape_score_acc_kernel(const double* __restrict__ part, const int* __restrict__ starts, int R, int F,
                                                                 double* __restrict__ acc) {
    __shared__ double grp[SC_BLOCK / 32][32];
    const int r = blockIdx.x, c = threadIdx.x & 31, g = threadIdx.x >> 5;
    const int s = starts[r], e = (r + 1 < R ? starts[r + 1] : F) - 1;
    const int b0 = s / SC_BLOCK, n = e / SC_BLOCK - b0 + 1;
    const bool mx = is_max_col(c);
    double a = 0.0;
    if (c < ACC) {
        const double* src = part + ((size_t)b0 + (size_t)r) * ACC + c;
        int i = g;
        for (; i + 24 < n; i += 32) {                   // four independent loads in flight, combined in order
            const double x0 = src[(size_t)i * ACC], x1 = src[(size_t)(i + 8) * ACC], x2 = src[(size_t)(i + 16) * ACC],
                         x3 = src[(size_t)(i + 24) * ACC];
            if (mx) a = fmax(fmax(fmax(fmax(a, x0), x1), x2), x3);
            else a = (((a + x0) + x1) + x2) + x3;
        }
        for (; i < n; i += 8) {
            const double x = src[(size_t)i * ACC];
            a = mx ? fmax(a, x) : a + x;
        }
    }
    grp[g][c] = a;
    __syncthreads();
    if (g == 0 && c < ACC) {
        double o = grp[0][c];
#pragma unroll
        for (int k = 1; k < SC_BLOCK / 32; ++k) o = mx ? fmax(o, grp[k][c]) : o + grp[k][c];
        acc[(size_t)r * ACC + c] = o;
    }
}

// ---- the lag sweep (ape_score_lags) --------------------------------------------------------------------------------------
// ape_score_lags_kernel      256 frames per workgroup and one lane per message frame, as above.  The workgroup first converts every truth
//                            row its frames can be paired with -- its own 256 and the halo its recordings' lags reach, at most 512 -- to a
//                            pose (hand, elbow, three quaternions, usable flag) exactly once and keeps the poses in LDS; a lane then holds
//                            its message and spread row in registers and walks the L lags, taking the pose of row f - l from LDS.  One
//                            partial record per (workgroup, recording, lag), reduced as above.
// ape_score_lags_acc_kernel  one workgroup per (recording, lag): ape_score_acc_kernel's order over that lag's partial records.
// For the sweep {0} without offsets the window is the workgroup's own 256 rows, the support is `f - start >= skip`, and every value and
// every sum is formed by the operations of ape_score_kernel in their order: the bits are those of ape_score_rows.
constexpr int SL_WINDOW = SC_BLOCK + 2 * APE_SCORE_MAX_LAG;

struct LagParams {
    ScoreParams s;                                      // score [F, L, 7]; part [(workgroups + R), L, 25], pair (b, r) at rows (b + r) * L ..
    const int* offs;                                    // [R] the recordings' offsets o_r
    int lag_min, L;
    int back, fwd;                                      // how far below / above its own rows a workgroup's truth window reaches:
};                                                      // max(0, max_r(o_r + lag_max)) and max(0, -min_r(o_r + lag_min)), each <= 128

template <typename TM, typename TT, int KIND, bool SPR>
__global__ __launch_bounds__(SC_BLOCK) void ape_score_lags_kernel(const LagParams q) {
    __shared__ double stage[SC_WAVES][64 * SC_LDS_ROW];
    __shared__ double poses[SL_WINDOW * POSE];
    __shared__ double wfirst[2][SC_WAVES][ACC];         // two buffers: one barrier per lag
    __shared__ int wrec[SC_WAVES][2];
    const ScoreParams& p = q.s;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long tile0 = (long long)blockIdx.x * SC_BLOCK;
    const long long row0 = tile0 + wave * 64;
    const long long f = row0 + lane;
    const bool valid = f < p.F;
    const long long left = (long long)p.F - row0;
    const int nrows = left >= 64 ? 64 : (left > 0 ? (int)left : 0);
    double* lds = stage[wave];

    // the frame's recording [start, end) and offset; lanes past F form a recording of their own
    int rec = p.R, start = 0, end = 0, off = 0;
    if (valid) {
        rec = find_rec(p.starts, p.R, f);
        start = p.starts[rec];
        end = rec + 1 < p.R ? p.starts[rec + 1] : p.F;
        off = q.offs[rec];
    }

    // ---- truth poses of the window [wlo, whi), 256 rows a round, each row converted once with its own recording's body ----
    const long long wlo = tile0 - q.back > 0 ? tile0 - q.back : 0;
    const long long whi = tile0 + SC_BLOCK + q.fwd < (long long)p.F ? tile0 + SC_BLOCK + q.fwd : (long long)p.F;
    const int tw = p.truth_w, tls = tw | 1;
    for (long long base = wlo; base < whi; base += SC_BLOCK) {                         // (uniform; at most twice)
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

    // ---- the message and its spread record, held in registers over the lags ----
    const bool hips = p.layout != APE_LAYOUT_ORI_CAL_LARM_UARM;
    bool ok_m = valid;
    if (nrows > 0) stage_rows(lds, static_cast<const TM*>(p.msg), p.msg_stride, 25, 25, row0, nrows, lane);
    __syncthreads();                                    // (also: every pose is written)
    double m[25];
#pragma unroll
    for (int c = 0; c < 25; ++c) { m[c] = valid ? lds[lane * 25 + c] : 0.0; ok_m = ok_m && fin(m[c]); }
    __syncthreads();
    double r18[18];
    if constexpr (SPR) {
        if (nrows > 0) stage_rows(lds, static_cast<const TM*>(p.spread), p.spread_stride, 21, 21, row0, nrows, lane);
        __syncthreads();
#pragma unroll
        for (int c = 0; c < 18; ++c) r18[c] = valid ? lds[lane * 21 + c] : 0.0;
        __syncthreads();
    }
    if (lane == 0) wrec[wave][0] = rec;
    if (lane == 63) wrec[wave][1] = rec;                // (read behind the first barrier of the lag loop)

    // the support: past the skipped frames, and paired at every lag of the sweep
    const int l_lo = off + q.lag_min, l_hi = l_lo + q.L - 1;
    const bool sup = valid && (f - start) >= (long long)p.skip && f - l_hi >= (long long)start && f - l_lo < (long long)end;

    for (int j = 0; j < q.L; ++j) {                     // (uniform)
        const long long tr = f - (l_lo + j);
        const bool ex = valid && tr >= (long long)start && tr < (long long)end;        // the pair exists: tr is inside [wlo, whi)
        const double* ps = poses + (ex ? (size_t)(tr - wlo) : 0) * POSE;
        double t[POSE];
#pragma unroll
        for (int c = 0; c < POSE; ++c) t[c] = ex ? ps[c] : 0.0;
        const Vec3 t_hand{t[0], t[1], t[2]}, t_elbow{t[3], t[4], t[5]};
        const Quat t_lq{t[6], t[7], t[8], t[9]}, t_uq{t[10], t[11], t[12], t[13]}, t_hq{t[14], t[15], t[16], t[17]};
        const bool ok = ok_m && ex && t[18] != 0.0;
        double s[APE_SCORE_WIDTH];
        s[0] = dist3(m + 4, t_hand);
        s[1] = dist3(m + 11, t_elbow);
        s[2] = ang_err(m + 7, t_lq);
        s[3] = ang_err(m + 14, t_uq);
        s[4] = hips ? ang_err(m + 21, t_hq) : 0.0;
        s[5] = NAN; s[6] = NAN;
        if constexpr (SPR) {
            s[5] = mahalanobis(r18, t_hand);
            s[6] = mahalanobis(r18 + 9, t_elbow);
        }
        if (!ok) {
#pragma unroll
            for (int c = 0; c < APE_SCORE_WIDTH; ++c) s[c] = NAN;
        }

        // per-frame rows [f, j, 0:7]: through LDS, neighbouring lanes write neighbouring values of a frame's run of seven
        if (p.score != nullptr) {
#pragma unroll
            for (int c = 0; c < APE_SCORE_WIDTH; ++c) lds[lane * APE_SCORE_WIDTH + c] = s[c];
            __syncthreads();
            const int total = nrows * APE_SCORE_WIDTH;
#pragma unroll
            for (int it = 0; it < APE_SCORE_WIDTH; ++it) {
                const int idx = it * 64 + lane;
                if (idx < total) {
                    const int r = idx / APE_SCORE_WIDTH, c = idx - r * APE_SCORE_WIDTH;
                    const size_t o = ((size_t)(row0 + r) * (size_t)q.L + (size_t)j) * APE_SCORE_WIDTH + c;
                    if (p.score_f32) static_cast<float*>(p.score)[o] = (float)lds[idx];
                    else static_cast<double*>(p.score)[o] = lds[idx];
                }
            }
            __syncthreads();
        }
        if (p.part == nullptr) continue;                // (uniform)

        const bool in = sup && ok;
        double v[ACC];
#pragma unroll
        for (int c = 0; c < 5; ++c) {
            const double e = in ? s[c] : 0.0;
            v[3 * c] = e; v[3 * c + 1] = e * e; v[3 * c + 2] = e;
        }
        v[15] = in ? 1.0 : 0.0;
        v[16] = (sup && !ok) ? 1.0 : 0.0;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const double d2 = s[5 + k];
            const bool has = in && fin(d2);
            v[17 + 4 * k] = has ? 1.0 : 0.0;
            v[18 + 4 * k] = has ? d2 : 0.0;
            v[19 + 4 * k] = (has && d2 <= CHI2_3_Q50) ? 1.0 : 0.0;
            v[20 + 4 * k] = (has && d2 <= CHI2_3_Q90) ? 1.0 : 0.0;
        }
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {              // the segmented tree of ape_score_kernel
            const int orec = __shfl_down(rec, o, 64);
            const bool take = lane + o < 64 && orec == rec;
            double w[ACC];
#pragma unroll
            for (int c = 0; c < ACC; ++c) w[c] = __shfl_down(v[c], o, 64);
            if (take) acc_combine(v, w);
        }
        double (*wf)[ACC] = wfirst[j & 1];
        if (lane == 0) {
#pragma unroll
            for (int c = 0; c < ACC; ++c) wf[wave][c] = v[c];
        }
        __syncthreads();
        if (valid && (f == start || threadIdx.x == 0)) {
            if (wrec[wave][1] == rec) {
                for (int w = wave + 1; w < SC_WAVES; ++w) {
                    if (wrec[w][0] != rec) break;
                    acc_combine(v, wf[w]);
                    if (wrec[w][1] != rec) break;
                }
            }
            double* dst = p.part + (((size_t)blockIdx.x + (size_t)rec) * (size_t)q.L + (size_t)j) * ACC;
#pragma unroll
            for (int c = 0; c < ACC; ++c) dst[c] = v[c];
        }
    }
}

// workgroup (r, j): recording r at sweep index j, its pairs (b, r) at rows (b + r) * L + j, combined as ape_score_acc_kernel combines
__global__ __launch_bounds__(SC_BLOCK) void ape_score_lags_acc_kernel(const double* __restrict__ part, const int* __restrict__ starts, int R, int F,
                                                                      int L, double* __restrict__ acc) {
    __shared__ double grp[SC_BLOCK / 32][32];
    const int r = blockIdx.x, j = blockIdx.y, c = threadIdx.x & 31, g = threadIdx.x >> 5;
    const int s = starts[r], e = (r + 1 < R ? starts[r + 1] : F) - 1;
    const int b0 = s / SC_BLOCK, n = e / SC_BLOCK - b0 + 1;
    const size_t step = (size_t)L * ACC;
    const bool mx = is_max_col(c);
    double a = 0.0;
    if (c < ACC) {
        const double* src = part + (((size_t)b0 + (size_t)r) * (size_t)L + (size_t)j) * ACC + c;
        int i = g;
        for (; i + 24 < n; i += 32) {
            const double x0 = src[(size_t)i * step], x1 = src[(size_t)(i + 8) * step], x2 = src[(size_t)(i + 16) * step],
                         x3 = src[(size_t)(i + 24) * step];
            if (mx) a = fmax(fmax(fmax(fmax(a, x0), x1), x2), x3);
            else a = (((a + x0) + x1) + x2) + x3;
        }
        for (; i < n; i += 8) {
            const double x = src[(size_t)i * step];
            a = mx ? fmax(a, x) : a + x;
        }
    }
    grp[g][c] = a;
    __syncthreads();
    if (g == 0 && c < ACC) {
        double o = grp[0][c];
#pragma unroll
        for (int k = 1; k < SC_BLOCK / 32; ++k) o = mx ? fmax(o, grp[k][c]) : o + grp[k][c];
        acc[((size_t)r * (size_t)L + (size_t)j) * ACC + c] = o;
    }
}

// the staging of both entries: starts, offsets and bodies in, the partial records behind them (score_host.h)
ApeSlotPool g_pool("score_rows");

template <typename TM, typename TT, int KIND>
void launch_score(const ScoreParams& p, unsigned blocks, hipStream_t st) {
    if (p.spread != nullptr) hipLaunchKernelGGL((ape_score_kernel<TM, TT, KIND, true>), dim3(blocks), dim3(SC_BLOCK), 0, st, p);
    else hipLaunchKernelGGL((ape_score_kernel<TM, TT, KIND, false>), dim3(blocks), dim3(SC_BLOCK), 0, st, p);
}

template <typename TM, typename TT>
void launch_score_kind(const ScoreParams& p, int kind, unsigned blocks, hipStream_t st) {
    if (kind == APE_TRUTH_TARGETS) launch_score<TM, TT, APE_TRUTH_TARGETS>(p, blocks, st);
    else launch_score<TM, TT, APE_TRUTH_EST>(p, blocks, st);
}

template <typename TM, typename TT, int KIND>
void launch_lags(const LagParams& q, unsigned blocks, hipStream_t st) {
    if (q.s.spread != nullptr) hipLaunchKernelGGL((ape_score_lags_kernel<TM, TT, KIND, true>), dim3(blocks), dim3(SC_BLOCK), 0, st, q);
    else hipLaunchKernelGGL((ape_score_lags_kernel<TM, TT, KIND, false>), dim3(blocks), dim3(SC_BLOCK), 0, st, q);
}

template <typename TM, typename TT>
void launch_lags_kind(const LagParams& q, int kind, unsigned blocks, hipStream_t st) {
    if (kind == APE_TRUTH_TARGETS) launch_lags<TM, TT, APE_TRUTH_TARGETS>(q, blocks, st);
    else launch_lags<TM, TT, APE_TRUTH_EST>(q, blocks, st);
}

// what ape_score_rows and ape_score_lags both refuse; `who` names the entry in the message
int check_score_args(const char* who, int32_t layout, const void* msg_dev, int32_t msg_stride, const void* spread_dev, int32_t spread_stride,
                     int32_t msg_dtype, const void* truth_dev, int32_t truth_kind, int32_t truth_dtype, int32_t F, const int32_t* seg_starts_host,
                     int32_t R, int32_t skip, const double* bodies_host, int32_t n_bodies, const void* score_dev, int32_t score_dtype,
                     const void* acc_dev) {
    if (!msg_dev || !truth_dev || !seg_starts_host || !bodies_host) return ape_fail(APE_ERR_INVALID_ARG, "%s: NULL argument", who);
    if (!score_dev && !acc_dev) return ape_fail(APE_ERR_INVALID_ARG, "%s: score_dev and acc_dev are both NULL", who);
    if (!ape_scoring_layout(layout))
        return ape_fail(APE_ERR_INVALID_ARG, "%s: layout %d has no pose to score", who, layout);
    if (truth_kind != APE_TRUTH_TARGETS && truth_kind != APE_TRUTH_EST) return ape_fail(APE_ERR_INVALID_ARG, "%s: unknown truth kind %d", who, truth_kind);
    if ((msg_dtype != APE_F32 && msg_dtype != APE_F64) || (truth_dtype != APE_F32 && truth_dtype != APE_F64) ||
        (score_dtype != APE_F32 && score_dtype != APE_F64))
        return ape_fail(APE_ERR_INVALID_ARG, "%s: unknown dtype selector", who);
    if (int rc = ape_check_segments(who, F, seg_starts_host, R)) return rc;      // (NULL starts: refused above)
    if (msg_stride < 25) return ape_fail(APE_ERR_INVALID_ARG, "%s: msg_stride %d below 25", who, msg_stride);
    if (spread_dev && spread_stride < APE_SPREAD_WIDTH) return ape_fail(APE_ERR_INVALID_ARG, "%s: spread_stride %d below %d", who, spread_stride, APE_SPREAD_WIDTH);
    if (skip < 0) return ape_fail(APE_ERR_INVALID_ARG, "%s: skip %d is negative", who, skip);
    if (n_bodies != 1 && n_bodies != R) return ape_fail(APE_ERR_INVALID_ARG, "%s: n_bodies %d is neither 1 nor R = %d", who, n_bodies, R);
    return APE_OK;
}

}  // namespace

int ape_score_rows(int32_t layout, const void* msg_dev, int32_t msg_stride, const void* spread_dev, int32_t spread_stride,
                   int32_t msg_dtype, const void* truth_dev, int32_t truth_kind, int32_t truth_dtype, int32_t F,
                   const int32_t* seg_starts_host, int32_t R, int32_t skip, const double* bodies_host, int32_t n_bodies,
                   void* score_dev, int32_t score_dtype, double* acc_dev, void* stream) {
    if (int rc = check_score_args("score_rows", layout, msg_dev, msg_stride, spread_dev, spread_stride, msg_dtype, truth_dev, truth_kind, truth_dtype, F,
                                  seg_starts_host, R, skip, bodies_host, n_bodies, score_dev, score_dtype, acc_dev))
        return rc;
    const hipStream_t st = (hipStream_t)stream;
    if (int rc = ape_check_not_capturing(st, "score_rows", "host arrays are staged per call")) return rc;
    int device = 0;
    APE_SCORE_TRY(g_pool.prefix, hipGetDevice(&device));

    const unsigned blocks = (unsigned)(((long long)F + SC_BLOCK - 1) / SC_BLOCK);
    const size_t starts_bytes = (((size_t)R * sizeof(int)) + 7) & ~(size_t)7;
    const size_t bodies_bytes = (size_t)n_bodies * 9 * sizeof(double);
    const size_t host_bytes = starts_bytes + bodies_bytes;
    const size_t part_bytes = acc_dev ? ((size_t)blocks + (size_t)R) * ACC * sizeof(double) : 0;

    std::lock_guard<std::mutex> lock(g_pool.mu);
    ApeSlot* slot = nullptr;
    if (int rc = g_pool.take(device, host_bytes, host_bytes + part_bytes, &slot)) return rc;
    memcpy(slot->pinned, seg_starts_host, (size_t)R * sizeof(int));
    memcpy(static_cast<char*>(slot->pinned) + starts_bytes, bodies_host, bodies_bytes);
    APE_SCORE_TRY(g_pool.prefix, hipMemcpyAsync(slot->dev, slot->pinned, host_bytes, hipMemcpyHostToDevice, st));

    ScoreParams p{};
    p.msg = msg_dev; p.spread = spread_dev; p.truth = truth_dev; p.score = score_dev;
    p.starts = static_cast<const int*>(slot->dev);
    p.bodies = reinterpret_cast<const double*>(static_cast<const char*>(slot->dev) + starts_bytes);
    p.part = acc_dev ? reinterpret_cast<double*>(static_cast<char*>(slot->dev) + host_bytes) : nullptr;
    p.msg_stride = msg_stride; p.spread_stride = spread_stride;
    p.F = F; p.R = R; p.skip = skip; p.layout = layout; p.n_bodies = n_bodies;
    p.truth_w = ape_truth_width(layout, truth_kind);
    p.score_f32 = score_dtype == APE_F32 ? 1 : 0;

    if (msg_dtype == APE_F32 && truth_dtype == APE_F32) launch_score_kind<float, float>(p, truth_kind, blocks, st);
    else if (msg_dtype == APE_F32) launch_score_kind<float, double>(p, truth_kind, blocks, st);
    else if (truth_dtype == APE_F32) launch_score_kind<double, float>(p, truth_kind, blocks, st);
    else launch_score_kind<double, double>(p, truth_kind, blocks, st);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && acc_dev) {
        hipLaunchKernelGGL(ape_score_acc_kernel, dim3((unsigned)R), dim3(SC_BLOCK), 0, st, p.part, p.starts, R, F, acc_dev);
        e = hipGetLastError();
    }
    return g_pool.finish("score_rows", slot, e, st);
}

int ape_score_lags(int32_t layout, const void* msg_dev, int32_t msg_stride, const void* spread_dev, int32_t spread_stride,
                   int32_t msg_dtype, const void* truth_dev, int32_t truth_kind, int32_t truth_dtype, int32_t F,
                   const int32_t* seg_starts_host, int32_t R, int32_t skip, const double* bodies_host, int32_t n_bodies,
                   int32_t lag_min, int32_t lag_max, const int32_t* rec_lag_host, void* score_dev, int32_t score_dtype, double* acc_dev,
                   void* stream) {
    if (int rc = check_score_args("score_lags", layout, msg_dev, msg_stride, spread_dev, spread_stride, msg_dtype, truth_dev, truth_kind, truth_dtype, F,
                                  seg_starts_host, R, skip, bodies_host, n_bodies, score_dev, score_dtype, acc_dev))
        return rc;
    int L = 0, back = 0, fwd = 0;
    if (int rc = ape_check_lag_sweep("score_lags", lag_min, lag_max, rec_lag_host, R, &L, &back, &fwd)) return rc;
    const hipStream_t st = (hipStream_t)stream;
    if (int rc = ape_check_not_capturing(st, "score_lags", "host arrays are staged per call")) return rc;
    int device = 0;
    APE_SCORE_TRY(g_pool.prefix, hipGetDevice(&device));

    const unsigned blocks = (unsigned)(((long long)F + SC_BLOCK - 1) / SC_BLOCK);
    const size_t starts_bytes = (((size_t)R * sizeof(int)) + 7) & ~(size_t)7;       // starts, then the offsets, then the bodies
    const size_t bodies_bytes = (size_t)n_bodies * 9 * sizeof(double);
    const size_t host_bytes = 2 * starts_bytes + bodies_bytes;
    const size_t part_bytes = acc_dev ? ((size_t)blocks + (size_t)R) * (size_t)L * ACC * sizeof(double) : 0;

    std::lock_guard<std::mutex> lock(g_pool.mu);
    ApeSlot* slot = nullptr;
    if (int rc = g_pool.take(device, host_bytes, host_bytes + part_bytes, &slot)) return rc;
    char* pin = static_cast<char*>(slot->pinned);
    memcpy(pin, seg_starts_host, (size_t)R * sizeof(int));
    if (rec_lag_host) memcpy(pin + starts_bytes, rec_lag_host, (size_t)R * sizeof(int));
    else memset(pin + starts_bytes, 0, (size_t)R * sizeof(int));
    memcpy(pin + 2 * starts_bytes, bodies_host, bodies_bytes);
    APE_SCORE_TRY(g_pool.prefix, hipMemcpyAsync(slot->dev, slot->pinned, host_bytes, hipMemcpyHostToDevice, st));

    LagParams q{};
    ScoreParams& p = q.s;
    char* dev = static_cast<char*>(slot->dev);
    p.msg = msg_dev; p.spread = spread_dev; p.truth = truth_dev; p.score = score_dev;
    p.starts = reinterpret_cast<const int*>(dev);
    q.offs = reinterpret_cast<const int*>(dev + starts_bytes);
    p.bodies = reinterpret_cast<const double*>(dev + 2 * starts_bytes);
    p.part = acc_dev ? reinterpret_cast<double*>(dev + host_bytes) : nullptr;
    p.msg_stride = msg_stride; p.spread_stride = spread_stride;
    p.F = F; p.R = R; p.skip = skip; p.layout = layout; p.n_bodies = n_bodies;
    p.truth_w = ape_truth_width(layout, truth_kind);
    p.score_f32 = score_dtype == APE_F32 ? 1 : 0;
    q.lag_min = lag_min; q.L = L;
    q.back = back; q.fwd = fwd;

    if (msg_dtype == APE_F32 && truth_dtype == APE_F32) launch_lags_kind<float, float>(q, truth_kind, blocks, st);
    else if (msg_dtype == APE_F32) launch_lags_kind<float, double>(q, truth_kind, blocks, st);
    else if (truth_dtype == APE_F32) launch_lags_kind<double, float>(q, truth_kind, blocks, st);
    else launch_lags_kind<double, double>(q, truth_kind, blocks, st);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && acc_dev) {
        hipLaunchKernelGGL(ape_score_lags_acc_kernel, dim3((unsigned)R, (unsigned)L), dim3(SC_BLOCK), 0, st, p.part, p.starts, R, F, L, acc_dev);
        e = hipGetLastError();
    }
    return g_pool.finish("score_lags", slot, e, st);
}
