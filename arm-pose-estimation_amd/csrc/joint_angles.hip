// Joint angles of every frame, and their errors against truth (ape_joint_angles; the reference has no counterpart).
// Rows that state an arm pose -- messages, est rows or NN targets -- of up to 64 sets against one list of recordings; truth rows of any
// of the three kinds, shared by all sets, paired at a lag per recording.
//
// ape_truth_angles_kernel  grid (tiles): the seven angles of every truth row once, float64, into the call's scratch [F, 7] (the sets share
//                          them: a set reads seven doubles per frame instead of converting the truth row again).
// ape_joint_angles_kernel  grid (tiles, sets), 256 frames per workgroup, one lane per frame.  A wave stages its 64 rows (32 per round),
//                          each lane converts its own row to the three unit quaternions and states the seven angles (include/ape_hip.h
//                          states every operation), takes the truth's angles of frame f - l_r and forms the errors.
// ape_angles_acc_kernel    one workgroup per (recording, set): its partial records folded in a fixed order.
//
// Sums: no atomics.  The 14 angle sums and the 21 error sums of a wave's frames are transposed through LDS (stride 21, two passes): lane c
// adds column c in frame order and cuts at recording boundaries (score_device.h's sum_columns), across the four waves in wave order,
// across workgroups in the order of ape_angles_acc_kernel.  Minima, maxima and counts do not depend on the order: a segmented shuffle
// tree per wave, as motion.hip's.  float64 with separate roundings for a * b + c, like the numpy statement (score.py:
// joint_angles_numpy): contraction is off in this file.
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

constexpr int JA_BLOCK = 256, JA_WAVES = JA_BLOCK / 64;
constexpr int AW = APE_ANGLE_WIDTH, JACC = APE_ANGLE_ACC_WIDTH;
constexpr int JA_ASUMS = 2 * AW;                        // a partial record: [2k] sum, [2k + 1] sum of squares of angle k,
constexpr int JA_ESUMS = 3 * AW;                        // [14 + 3k ..] sum, sum of magnitudes, sum of squares of error k,
constexpr int JA_SUMS = JA_ASUMS + JA_ESUMS;            // then the rest: 7 minima, 7 maxima, 7 counts of the angles, 7 largest magnitudes and
constexpr int JA_REST = 5 * AW + 1;                     // 7 counts of the errors, the frames of the support
constexpr int JA_TSTRIDE = JA_ESUMS;                    // stride of a frame's terms in the transposition buffer; odd
constexpr int JA_STAGE_ROWS = 32;
constexpr int JA_WAVE_LDS = 64 * JA_TSTRIDE;            // a wave's block: 32 staged rows, its 64 x 7 rows on their way out, its 64 x 21 terms
constexpr int JA_ACC_BLOCK = 512, JA_ACC_GROUPS = JA_ACC_BLOCK / 128;

static_assert(JA_SUMS + JA_REST == JACC && JACC <= 128, "a partial record has the width of the accumulators; one lane per column");
static_assert(JA_STAGE_ROWS * STAGE_COLS <= JA_WAVE_LDS && 64 * AW <= JA_WAVE_LDS && (JA_TSTRIDE & 1) == 1, "what lies in a wave's block fits");

struct AngleParams {
    const void* rows;
    const double* tang;                                 // [F, 7] the truth's angles, or NULL
    void* angles;                                       // [n_sets, F, 7] or NULL
    void* errors;                                       // [n_sets, F, 7] or NULL
    double* part;                                       // [n_sets, (workgroups + R), 71] partial records, pair (b, r) at row b + r; or NULL
    const int* starts;                                  // [R]
    const int* lags;                                    // [R]
    const double* bodies;                               // [n_bodies, 9] (APE_ROWS_TARGETS)
    long long rows_stride, set_stride;
    double sh, sf;                                      // sin(min_swing / 2), sin(min_swing)
    int F, R, skip, layout, n_bodies, row_w;
};

struct SwingTwist { double rho, n, swing, twist, azimuth; };

// r = swing (x) twist about x, r negated first where r.w < 0.0
__device__ __forceinline__ SwingTwist swing_twist(Quat r) {
    if (r.w < 0.0) r = Quat{-r.w, -r.x, -r.y, -r.z};
    SwingTwist o;
    o.rho = sqrt(r.w * r.w + r.x * r.x);
    o.n = sqrt(r.y * r.y + r.z * r.z);
    o.swing = 2.0 * atan2(o.n, o.rho);
    o.twist = 2.0 * atan2(r.x, r.w);
    o.azimuth = atan2(r.y * r.x + r.z * r.w, r.y * r.w - r.z * r.x);
    return o;
}

// |q|, and q / |q| in place; false where the norm is not finite or not positive
__device__ __forceinline__ bool unit4(Quat& q) {
    const double n = sqrt(q.w * q.w + q.x * q.x + q.y * q.y + q.z * q.z);
    q = Quat{q.w / n, q.x / n, q.y / n, q.z / n};
    return fin(n) && n > 0.0;
}

// the seven angles of a row t of KIND (include/ape_hip.h); all NaN where the row states no pose
template <int KIND>
__device__ __forceinline__ void row_angles(const double* t, int rw, int layout, const double* body, double sh, double sf, double* a) {
    const bool hips = layout != APE_LAYOUT_ORI_CAL_LARM_UARM;
    Quat ql, qu, qh{1.0, 0.0, 0.0, 0.0};
    bool ok = true;
    if constexpr (KIND == APE_ROWS_TARGETS) {
        double pose[POSE];
        truth_pose<APE_TRUTH_TARGETS>(t, rw, layout, body, pose);
        ql = Quat{pose[6], pose[7], pose[8], pose[9]}; qu = Quat{pose[10], pose[11], pose[12], pose[13]};
        qh = Quat{pose[14], pose[15], pose[16], pose[17]};
        ok = pose[18] != 0.0;
    } else {
        if constexpr (KIND == APE_ROWS_MSG) {           // message columns [7:11], [14:18], [21:25]
            ql = Quat{t[7], t[8], t[9], t[10]}; qu = Quat{t[14], t[15], t[16], t[17]};
            if (hips) qh = Quat{t[21], t[22], t[23], t[24]};
        } else {                                        // est columns [9:13], [13:17], [17:21]; without hips [6:10], [10:14]
            ql = hips ? Quat{t[9], t[10], t[11], t[12]} : Quat{t[6], t[7], t[8], t[9]};
            qu = hips ? Quat{t[13], t[14], t[15], t[16]} : Quat{t[10], t[11], t[12], t[13]};
            if (hips) qh = Quat{t[17], t[18], t[19], t[20]};
        }
        ok =fin(ql.w) && fin(ql.x) && fin(ql.y) && fin(ql.z) && fin(qu.w) && fin(qu.x) && fin(qu.y) && fin(qu.z) &&
             fin(qh.w) && fin(qh.x) && fin(qh.y) && fin(qh.z);
    }
    const bool nl = unit4(ql), nu = unit4(qu), nh = unit4(qh);
    ok = ok && nl && nu && nh;
    const SwingTwist e = swing_twist(qmul(Quat{qu.w, -qu.x, -qu.y, -qu.z}, ql));
    const Quat s = qmul(Quat{qh.w, -qh.x, -qh.y, -qh.z}, qu);
    const SwingTwist st = swing_twist(s);
    const double dx = -((s.w * s.w + s.x * s.x) - (s.y * s.y + s.z * s.z));
    const double dy = -(2.0 * (s.x * s.y + s.w * s.z));
    const double dz = -(2.0 * (s.x * s.z - s.w * s.y));
    const double hd = sqrt(dx * dx + dz * dz);
    if (qh.w < 0.0) qh = Quat{-qh.w, -qh.x, -qh.y, -qh.z};
    a[0] = e.swing;
    a[1] = e.n < sh ? NAN : e.azimuth;
    a[2] = e.rho < sh ? NAN : e.twist;
    a[3] = atan2(hd, -dy);
    a[4] = hd < sf ? NAN : atan2(dz, -dx);
    a[5] = st.rho < sh ? NAN : st.twist;
    a[6] = 2.0 * atan2(qh.y, qh.w);
    if (!ok) {
#pragma unroll
        for (int c = 0; c < AW; ++c) a[c] = NAN;
    }
}

// The wave's rows row0 .. row0 + nrows - 1 staged through its block (32 per round), lane i's row converted to its angles.  Called by
// every wave of the workgroup (it meets the others at four barriers); a lane past nrows gets NaN.
template <typename T, int KIND>
__device__ __forceinline__ void wave_angles(double* lds, const T* src, long long stride, int rw, int layout, long long row0, int nrows, int lane,
                                            const int* starts, int R, const double* bodies, int n_bodies, double sh, double sf, double* a) {
    const int rls = rw | 1;
    double t[STAGE_COLS];
#pragma unroll
    for (int c = 0; c < STAGE_COLS; ++c) t[c] = 0.0;
#pragma unroll
    for (int round = 0; round < 64 / JA_STAGE_ROWS; ++round) {
        const int left = nrows - round * JA_STAGE_ROWS;
        const int nr = left > JA_STAGE_ROWS ? JA_STAGE_ROWS : (left > 0 ? left : 0);
        if (nr > 0) stage_rows(lds, src, stride, rw, rls, row0 + round * JA_STAGE_ROWS, nr, lane);
        __syncthreads();
        const int i = lane - round * JA_STAGE_ROWS;
        if (i >= 0 && i < nr) {
#pragma unroll
            for (int c = 0; c < STAGE_COLS; ++c)
                if (c < rw) t[c] = lds[i * rls + c];
        }
        __syncthreads();
    }
    const double* body = bodies;
    if constexpr (KIND == APE_ROWS_TARGETS) {
        if (n_bodies > 1 && lane < nrows) body = bodies + 9 * (size_t)find_rec(starts, R, row0 + lane);
    }
    row_angles<KIND>(t, rw, layout, body, sh, sf, a);
    if (lane >= nrows) {
#pragma unroll
        for (int c = 0; c < AW; ++c) a[c] = NAN;
    }
}

template <typename T, int KIND>
__global__ __launch_bounds__(JA_BLOCK) void ape_truth_angles_kernel(const T* __restrict__ truth, long long stride, int tw, int layout, int F,
                                                                    const int* __restrict__ starts, int R, const double* __restrict__ bodies,
                                                                    int n_bodies, double sh, double sf, double* __restrict__ tang) {
    __shared__ double mem[JA_WAVES * JA_WAVE_LDS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long row0 = (long long)blockIdx.x * JA_BLOCK + wave * 64;
    const long long left = (long long)F - row0;
    const int nrows = left >= 64 ? 64 : (left > 0 ? (int)left : 0);
    double* lds = mem + wave * JA_WAVE_LDS;
    double a[AW];
    wave_angles<T, KIND>(lds, truth, stride, tw, layout, row0, nrows, lane, starts, R, bodies, n_bodies, sh, sf, a);
#pragma unroll
    for (int c = 0; c < AW; ++c) lds[lane * AW + c] = a[c];
    __syncthreads();
    const int total = nrows * AW;
    double* out = tang + (size_t)row0 * AW;
#pragma unroll
    for (int it = 0; it < AW; ++it) {
        const int idx = it * 64 + lane;
        if (idx < total) out[idx] = lds[idx];
    }
}

// how column c of the rest folds: the smaller, the larger, or the sum
__device__ __forceinline__ double rest_fold(int c, double a, double b) {
    if (c < AW) return fmin(a, b);
    if (c < 2 * AW || (c >= 3 * AW && c < 4 * AW)) return fmax(a, b);
    return a + b;
}

// the wave's 64 x 7 values, through its block, as one run
template <typename TOut>
__device__ __forceinline__ void write_rows(double* lds, const double* v, void* dst, size_t first, int nrows, int lane) {
#pragma unroll
    for (int c = 0; c < AW; ++c) lds[lane * AW + c] = v[c];
    __syncthreads();
    const int total = nrows * AW;
    TOut* out = static_cast<TOut*>(dst) + first * AW;
#pragma unroll
    for (int it = 0; it < AW; ++it) {
        const int idx = it * 64 + lane;
        if (idx < total) out[idx] = (TOut)lds[idx];
    }
    __syncthreads();
}

template <typename TRows, int KIND, typename TOut>
__global__ __launch_bounds__(JA_BLOCK) void ape_joint_angles_kernel(const AngleParams p) {
    __shared__ double mem[JA_WAVES * JA_WAVE_LDS];
    __shared__ double wfirst[JA_WAVES][JA_SUMS];
    __shared__ double wrest[JA_WAVES][JA_REST];
    __shared__ int wrec[JA_WAVES][2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int set = blockIdx.y;
    const long long row0 = (long long)blockIdx.x * JA_BLOCK + wave * 64;
    const long long f = row0 + lane;
    const bool valid = f < p.F;
    const long long left = (long long)p.F - row0;
    const int nrows = left >= 64 ? 64 : (left > 0 ? (int)left : 0);
    double* lds = mem + wave * JA_WAVE_LDS;

    // the frame's recording; lanes past F form a recording of their own
    int rec = p.R, start = 0, end = 0;
    if (valid) {
        rec = find_rec(p.starts, p.R, f);
        start = p.starts[rec];
        end = rec + 1 < p.R ? p.starts[rec + 1] : p.F;
    }

    // ---- the frame's seven angles, and its errors against the truth's angles of frame f - l_r ----
    const TRows* src = static_cast<const TRows*>(p.rows) + (long long)set * p.set_stride;
    double a[AW], e[AW];
    wave_angles<TRows, KIND>(lds, src, p.rows_stride, p.row_w, p.layout, row0, nrows, lane, p.starts, p.R, p.bodies, p.n_bodies, p.sh, p.sf, a);
    const bool truth = p.tang != nullptr;               // (uniform)
    if (truth) {
        const long long tf = valid ? f - (long long)p.lags[rec] : -1;
        const bool paired = valid && tf >= (long long)start && tf < (long long)end;
        const double pi = 3.141592653589793, two_pi = 6.283185307179586;
#pragma unroll
        for (int c = 0; c < AW; ++c) {
            const double ta = paired ? p.tang[(size_t)tf * AW + c] : NAN;
            double d = a[c] - ta;
            if (c != 0 && c != 3) {
                if (d > pi) d = d - two_pi;
                else if (d <= -pi) d = d + two_pi;
            }
            e[c] = d;
        }
    } else {
#pragma unroll
        for (int c = 0; c < AW; ++c) e[c] = NAN;
    }
    if (p.angles != nullptr) write_rows<TOut>(lds, a, p.angles, (size_t)set * (size_t)p.F + (size_t)row0, nrows, lane);
    if (p.errors != nullptr) write_rows<TOut>(lds, e, p.errors, (size_t)set * (size_t)p.F + (size_t)row0, nrows, lane);
    if (p.part == nullptr) return;                      // (uniform)

    // ---- the frame's contribution; the support: f - start >= skip ----
    const int prev = __shfl_up(rec, 1, 64);
    const unsigned long long bmask = __ballot(lane > 0 && rec != prev);
    if (lane == 0) wrec[wave][0] = rec;
    if (lane == 63) wrec[wave][1] = rec;
    const bool sup = valid && (f - start) >= (long long)p.skip;
    double v[JA_REST];
#pragma unroll
    for (int c = 0; c < AW; ++c) {
        const bool in = sup && fin(a[c]);
        const double x = in ? a[c] : 0.0;
        lds[lane * JA_TSTRIDE + 2 * c] = x;
        lds[lane * JA_TSTRIDE + 2 * c + 1] = x * x;
        v[c] = in ? a[c] : INFINITY;
        v[AW + c] = in ? a[c] : -INFINITY;
        v[2 * AW + c] = in ? 1.0 : 0.0;
        const bool ein = sup && fin(e[c]);
        v[3 * AW + c] = ein ? fabs(e[c]) : 0.0;
        v[4 * AW + c] = ein ? 1.0 : 0.0;
    }
    v[5 * AW] = sup ? 1.0 : 0.0;
    __syncthreads();                                    // (the terms and wrec are written)
    const int prev_last = wave > 0 ? wrec[wave - 1][1] : -1;
    double* part_row0 = p.part + ((size_t)set * ((size_t)gridDim.x + (size_t)p.R) + (size_t)blockIdx.x) * JACC;       // + r * JACC: the pair (b, r)
    double held_a = 0.0, held_e = 0.0;
    bool holds = false;
    int held_rec = -1;
    sum_columns<JA_TSTRIDE, JA_WAVES>(lds, JA_ASUMS, 0, rec, bmask, lane, wave, p.R, prev_last, wfirst[wave], part_row0, (size_t)JACC, &held_a, &holds, &held_rec);
    if (truth) {
        __syncthreads();                                // (every lane has read the angles' terms)
#pragma unroll
        for (int c = 0; c < AW; ++c) {
            const double x = (sup && fin(e[c])) ? e[c] : 0.0;
            lds[lane * JA_TSTRIDE + 3 * c] = x;
            lds[lane * JA_TSTRIDE + 3 * c + 1] = fabs(x);
            lds[lane * JA_TSTRIDE + 3 * c + 2] = x * x;
        }
        __syncthreads();
        sum_columns<JA_TSTRIDE, JA_WAVES>(lds, JA_ESUMS, JA_ASUMS, rec, bmask, lane, wave, p.R, prev_last, wfirst[wave], part_row0, (size_t)JACC, &held_e, &holds, &held_rec);
    }

    // minima, maxima and counts: after the round with offset o, lane l holds the frames [l, l + 2 o) of its recording within the wave
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int orec = __shfl_down(rec, off, 64);
        const bool take = lane + off < 64 && orec == rec;
#pragma unroll
        for (int c = 0; c < JA_REST; ++c) {
            const double o = __shfl_down(v[c], off, 64);
            if (take) v[c] = rest_fold(c, v[c], o);
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < JA_REST; ++c) wrest[wave][c] = v[c];
    }
    __syncthreads();                                    // (every wave's leading run is in wfirst and wrest)
    // the wave whose last run starts a (workgroup, recording) pair takes the following waves' leading runs in wave order
    if (holds) {                                        // (uniform)
        for (int w = wave + 1; w < JA_WAVES; ++w) {
            if (wrec[w][0] != held_rec) break;
            if (lane < JA_ASUMS) held_a = held_a + wfirst[w][lane];
            if (truth && lane < JA_ESUMS) held_e = held_e + wfirst[w][JA_ASUMS + lane];
            if (wrec[w][1] != held_rec) break;
        }
        if (lane < JA_ASUMS) part_row0[(size_t)held_rec * JACC + lane] = held_a;
        if (truth && lane < JA_ESUMS) part_row0[(size_t)held_rec * JACC + JA_ASUMS + lane] = held_e;
    }
    // the first frame of every (workgroup, recording) pair does the same for the rest
    if (valid && (f == start || threadIdx.x == 0)) {
        if (wrec[wave][1] == rec) {
            for (int w = wave + 1; w < JA_WAVES; ++w) {
                if (wrec[w][0] != rec) break;
#pragma unroll
                for (int c = 0; c < JA_REST; ++c) v[c] = rest_fold(c, v[c], wrest[w][c]);
                if (wrec[w][1] != rec) break;
            }
        }
        double* dst = part_row0 + (size_t)rec * JACC + JA_SUMS;
#pragma unroll
        for (int c = 0; c < JA_REST; ++c) dst[c] = v[c];
    }
}

// workgroup (r, set): recording r's pairs (b, r), b = first .. last workgroup of its frames, at rows b + r of the set's partial records.
// Thread (g, c): column c of the pairs g, g + 4, ... in order; then the four groups in order.  Column c of a partial record lands in its
// slot of the 71; without truth the error sums were not written and are stated as zeros.
__global__ __launch_bounds__(JA_ACC_BLOCK) void ape_angles_acc_kernel(const double* __restrict__ part, const int* __restrict__ starts, int R, int F,
                                                                      int blocks, int truth, double* __restrict__ acc) {
    __shared__ double grp[JA_ACC_GROUPS][128];
    const int r = blockIdx.x, set = blockIdx.y, c = threadIdx.x & 127, g = threadIdx.x >> 7;
    const int s = starts[r], e = (r + 1 < R ? starts[r + 1] : F) - 1;
    const int b0 = s / JA_BLOCK, n = e / JA_BLOCK - b0 + 1;
    const int cr = c - JA_SUMS;                         // the column among the rest
    const bool esum = c >= JA_ASUMS && c < JA_SUMS;
    const bool live = c < JACC && (truth != 0 || !esum);
    double a = cr >= 0 && cr < AW ? INFINITY : (cr >= AW && cr < 2 * AW ? -INFINITY : 0.0);
    if (live) {
        const double* src = part + ((size_t)set * ((size_t)blocks + (size_t)R) + (size_t)b0 + (size_t)r) * JACC + c;
        for (int i = g; i < n; i += JA_ACC_GROUPS) {
            const double x = src[(size_t)i * JACC];
            a = cr < 0 ? a + x : rest_fold(cr, a, x);
        }
    }
    grp[g][c] = a;
    __syncthreads();
    if (g == 0 && c < JACC) {
        double o = grp[0][c];
#pragma unroll
        for (int k = 1; k < JA_ACC_GROUPS; ++k) o = cr < 0 ? o + grp[k][c] : rest_fold(cr, o, grp[k][c]);
        int slot = JACC - 1;                            // the frames of the support
        if (c < JA_ASUMS) slot = 5 * (c >> 1) + (c & 1);
        else if (c < JA_SUMS) slot = 5 * AW + 5 * ((c - JA_ASUMS) / 3) + (c - JA_ASUMS) % 3;
        else if (cr < 3 * AW) slot = 5 * (cr % AW) + 2 + cr / AW;
        else if (cr < 5 * AW) slot = 5 * AW + 5 * (cr % AW) + cr / AW;
        acc[((size_t)set * (size_t)R + (size_t)r) * JACC + slot] = o;
    }
}

// the staging of a call: starts, lags and bodies in, the truth's angles and the partial records behind them (score_host.h)
ApeSlotPool g_pool("joint_angles");

template <typename TRows, typename TOut>
void launch_angles(const AngleParams& p, int kind, dim3 grid, hipStream_t st) {
    if (kind == APE_ROWS_MSG) hipLaunchKernelGGL((ape_joint_angles_kernel<TRows, APE_ROWS_MSG, TOut>), grid, dim3(JA_BLOCK), 0, st, p);
    else if (kind == APE_ROWS_EST) hipLaunchKernelGGL((ape_joint_angles_kernel<TRows, APE_ROWS_EST, TOut>), grid, dim3(JA_BLOCK), 0, st, p);
    else hipLaunchKernelGGL((ape_joint_angles_kernel<TRows, APE_ROWS_TARGETS, TOut>), grid, dim3(JA_BLOCK), 0, st, p);
}

template <typename T>
void launch_truth(const void* truth, int kind, long long stride, int tw, const AngleParams& p, double* tang, unsigned blocks, hipStream_t st) {
    const T* t = static_cast<const T*>(truth);
    if (kind == APE_ROWS_MSG)
        hipLaunchKernelGGL((ape_truth_angles_kernel<T, APE_ROWS_MSG>), dim3(blocks), dim3(JA_BLOCK), 0, st, t, stride, tw, p.layout, p.F, p.starts, p.R,
                           p.bodies, p.n_bodies, p.sh, p.sf, tang);
    else if (kind == APE_ROWS_EST)
        hipLaunchKernelGGL((ape_truth_angles_kernel<T, APE_ROWS_EST>), dim3(blocks), dim3(JA_BLOCK), 0, st, t, stride, tw, p.layout, p.F, p.starts, p.R,
                           p.bodies, p.n_bodies, p.sh, p.sf, tang);
    else
        hipLaunchKernelGGL((ape_truth_angles_kernel<T, APE_ROWS_TARGETS>), dim3(blocks), dim3(JA_BLOCK), 0, st, t, stride, tw, p.layout, p.F, p.starts,
                           p.R, p.bodies, p.n_bodies, p.sh, p.sf, tang);
}

bool rows_kind_known(int32_t kind) { return kind == APE_ROWS_MSG || kind == APE_ROWS_EST || kind == APE_ROWS_TARGETS; }

// values of a row of a scoring layout
int rows_width(int32_t layout, int32_t kind) {
    if (kind == APE_ROWS_MSG) return 25;
    return ape_truth_width(layout, kind == APE_ROWS_TARGETS ? APE_TRUTH_TARGETS : APE_TRUTH_EST);
}

}  // namespace

int ape_joint_angles(int32_t layout, const void* rows_dev, int32_t rows_kind, int32_t rows_stride, int32_t rows_dtype, int32_t n_sets,
                     int64_t set_stride, const void* truth_dev, int32_t truth_kind, int32_t truth_stride, int32_t truth_dtype,
                     const int32_t* rec_lag_host, int32_t F, const int32_t* seg_starts_host, int32_t R, int32_t skip, const double* bodies_host,
                     int32_t n_bodies, double min_swing, void* angles_dev, void* errors_dev, int32_t out_dtype, double* acc_dev, void* stream) {
    const char* who = "joint_angles";
    if (!rows_dev || !seg_starts_host) return ape_fail(APE_ERR_INVALID_ARG, "%s: NULL argument", who);
    if (!angles_dev && !errors_dev && !acc_dev) return ape_fail(APE_ERR_INVALID_ARG, "%s: no output (angles_dev, errors_dev and acc_dev are NULL)", who);
    if (errors_dev && !truth_dev) return ape_fail(APE_ERR_INVALID_ARG, "%s: errors_dev without truth", who);
    if (!ape_scoring_layout(layout)) return ape_fail(APE_ERR_INVALID_ARG, "%s: layout %d has no pose to take angles of", who, layout);
    if (!rows_kind_known(rows_kind) || (truth_dev && !rows_kind_known(truth_kind)))
        return ape_fail(APE_ERR_INVALID_ARG, "%s: unknown rows kind %d / truth kind %d", who, rows_kind, truth_kind);
    if ((rows_dtype != APE_F32 && rows_dtype != APE_F64) || (out_dtype != APE_F32 && out_dtype != APE_F64) ||
        (truth_dev && truth_dtype != APE_F32 && truth_dtype != APE_F64))
        return ape_fail(APE_ERR_INVALID_ARG, "%s: unknown dtype selector", who);
    if (int rc = ape_check_segments(who, F, seg_starts_host, R)) return rc;
    if (skip < 0) return ape_fail(APE_ERR_INVALID_ARG, "%s: skip %d is negative", who, skip);
    if (!(min_swing >= 0.0 && min_swing < 1.5707963267948966))
        return ape_fail(APE_ERR_INVALID_ARG, "%s: min_swing %g outside [0, pi / 2)", who, min_swing);
    const int rw = rows_width(layout, rows_kind), tw = truth_dev ? rows_width(layout, truth_kind) : 0;
    if (rows_stride < rw) return ape_fail(APE_ERR_INVALID_ARG, "%s: rows_stride %d below the row width %d", who, rows_stride, rw);
    if (truth_dev && truth_stride < tw) return ape_fail(APE_ERR_INVALID_ARG, "%s: truth_stride %d below the row width %d", who, truth_stride, tw);
    if (n_sets < 1 || n_sets > APE_POST_MAX_CONFIGS)
        return ape_fail(APE_ERR_INVALID_ARG, "%s: n_sets %d, between 1 and %d", who, n_sets, APE_POST_MAX_CONFIGS);
    if (n_sets > 1 && set_stride < (int64_t)F * (int64_t)rows_stride)
        return ape_fail(APE_ERR_INVALID_ARG, "%s: set_stride %lld below F * rows_stride = %lld", who, (long long)set_stride,
                        (long long)F * (long long)rows_stride);
    const bool targets = rows_kind == APE_ROWS_TARGETS || (truth_dev && truth_kind == APE_ROWS_TARGETS);
    if (targets) {
        if (!bodies_host) return ape_fail(APE_ERR_INVALID_ARG, "%s: NULL bodies_host with target rows", who);
        if (n_bodies != 1 && n_bodies != R) return ape_fail(APE_ERR_INVALID_ARG, "%s: n_bodies %d is neither 1 nor R = %d", who, n_bodies, R);
    }
    const void* outs[3] = {angles_dev, errors_dev, acc_dev};
    for (int i = 0; i < 3; ++i) {
        if (!outs[i]) continue;
        if (outs[i] == rows_dev || outs[i] == truth_dev) return ape_fail(APE_ERR_INVALID_ARG, "%s: an output aliases an input", who);
        for (int j = 0; j < i; ++j)
            if (outs[i] == outs[j]) return ape_fail(APE_ERR_INVALID_ARG, "%s: two outputs alias", who);
    }
    const hipStream_t st = (hipStream_t)stream;
    if (int rc = ape_check_not_capturing(st, who, "host arrays are staged per call")) return rc;
    int device = 0;
    APE_SCORE_TRY(g_pool.prefix, hipGetDevice(&device));

    const unsigned blocks = (unsigned)(((long long)F + JA_BLOCK - 1) / JA_BLOCK);
    const size_t ints_bytes = (((size_t)R * sizeof(int)) + 7) & ~(size_t)7;         // starts, lags, then the bodies
    const size_t bodies_bytes = targets ? (size_t)n_bodies * 9 * sizeof(double) : 0;
    const size_t host_bytes = 2 * ints_bytes + bodies_bytes;
    const size_t tang_bytes = truth_dev ? (size_t)F * AW * sizeof(double) : 0;
    const size_t part_bytes = acc_dev ? (size_t)n_sets * ((size_t)blocks + (size_t)R) * JACC * sizeof(double) : 0;

    std::lock_guard<std::mutex> lock(g_pool.mu);
    ApeSlot* slot = nullptr;
    if (int rc = g_pool.take(device, host_bytes, host_bytes + tang_bytes + part_bytes, &slot)) return rc;
    char* pin = static_cast<char*>(slot->pinned);
    memcpy(pin, seg_starts_host, (size_t)R * sizeof(int));
    if (rec_lag_host) memcpy(pin + ints_bytes, rec_lag_host, (size_t)R * sizeof(int));
    else memset(pin + ints_bytes, 0, (size_t)R * sizeof(int));
    if (targets) memcpy(pin + 2 * ints_bytes, bodies_host, bodies_bytes);
    // (a copy that fails leaves through finish() like a launch that fails: the slot's event is recorded either way)
    const hipError_t copied = hipMemcpyAsync(slot->dev, slot->pinned, host_bytes, hipMemcpyHostToDevice, st);
    if (copied != hipSuccess) return g_pool.finish(who, slot, copied, st);

    AngleParams p{};
    char* dev = static_cast<char*>(slot->dev);
    double* tang = truth_dev ? reinterpret_cast<double*>(dev + host_bytes) : nullptr;
    p.rows = rows_dev; p.tang = tang; p.angles = angles_dev; p.errors = errors_dev;
    p.starts = reinterpret_cast<const int*>(dev);
    p.lags = reinterpret_cast<const int*>(dev + ints_bytes);
    p.bodies = reinterpret_cast<const double*>(dev + 2 * ints_bytes);
    p.part = acc_dev ? reinterpret_cast<double*>(dev + host_bytes + tang_bytes) : nullptr;
    p.rows_stride = rows_stride; p.set_stride = n_sets > 1 ? (long long)set_stride : 0;
    p.sh = sin(min_swing / 2.0); p.sf = sin(min_swing);
    p.F = F; p.R = R; p.skip = skip; p.layout = layout; p.n_bodies = targets ? n_bodies : 1; p.row_w = rw;

    hipError_t e = hipSuccess;
    if (truth_dev) {
        if (truth_dtype == APE_F32) launch_truth<float>(truth_dev, truth_kind, truth_stride, tw, p, tang, blocks, st);
        else launch_truth<double>(truth_dev, truth_kind, truth_stride, tw, p, tang, blocks, st);
        e = hipGetLastError();
    }
    if (e == hipSuccess) {
        const dim3 grid(blocks, (unsigned)n_sets);
        if (rows_dtype == APE_F32 && out_dtype == APE_F32) launch_angles<float, float>(p, rows_kind, grid, st);
        else if (rows_dtype == APE_F32) launch_angles<float, double>(p, rows_kind, grid, st);
        else if (out_dtype == APE_F32) launch_angles<double, float>(p, rows_kind, grid, st);
        else launch_angles<double, double>(p, rows_kind, grid, st);
        e = hipGetLastError();
    }
    if (e == hipSuccess && acc_dev) {
        hipLaunchKernelGGL(ape_angles_acc_kernel, dim3((unsigned)R, (unsigned)n_sets), dim3(JA_ACC_BLOCK), 0, st, p.part, p.starts, R, F, (int)blocks,
                           truth_dev ? 1 : 0, acc_dev);
        e = hipGetLastError();
    }
    return g_pool.finish(who, slot, e, st);
}
