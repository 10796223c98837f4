// How smooth a replay is: linear and angular speed, acceleration and jerk of every frame, on the frames' own clock (ape_motion_sums;
// DESIGN.md 4.39; the reference has no counterpart).  Rows that state an arm pose -- messages, est rows or NN targets -- of up to 64
// sets (repost's [C, F, 25]) against one list of recordings and one clock; no truth is read.
//
// ape_motion_kernel      grid (tiles, sets), 256 frames per workgroup, one lane per frame.  The workgroup stages its 256 rows and the three
//                        below them (clipped at row 0; 32 rows per wave and round), converts each once to the 19-value pose record
//                        (quaternions normalised) and keeps the 259 poses and stamps in LDS; a lane then reads the poses of f-3 .. f
//                        and forms the 12 values from divided differences (include/ape_hip.h states every operation).  A frame never
//                        reads below its recording's start.
// ape_motion_acc_kernel  one workgroup per (recording, set): its partial records folded in a fixed order.
//
// Sums: no atomics.  The 24 sums and sums of squares of a wave's frames are transposed through LDS (stride 25): lane c adds column c in
// frame order and cuts at recording boundaries (score_device.h's sum_columns), across the four waves in wave order, across workgroups
// in the order of ape_motion_acc_kernel (sums_acc's).  The 12 maxima and the two counts do not depend on the order: a segmented shuffle
// tree per wave, as score.hip's.  float64 with separate roundings for a * b + c, like the numpy statement (score.py: motion_sums_numpy):
// contraction is off in this file.
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

constexpr int MO_BLOCK = 256, MO_WAVES = MO_BLOCK / 64;
constexpr int MO_HALO = 3;                              // rows below a frame that its third difference reads
constexpr int MO_WINDOW = MO_BLOCK + MO_HALO;
constexpr int MW = APE_MOTION_WIDTH, MACC = APE_MOTION_ACC_WIDTH;
constexpr int MO_SUMS = 2 * MW;                         // a partial record: [2k] sum, [2k + 1] sum of squares of value k,
constexpr int MO_REST = MW + 2;                         // then the 12 maxima and the two counts
constexpr int MO_TSTRIDE = STAGE_COLS;                  // stride of a frame's terms in the transposition buffer; odd
// LDS, in doubles.  Rows are staged 32 per wave and round, two rounds (64 would put the workgroup at 94 KB and alone on its CU); wave 0
// takes the three rows below the tile with its first 32.  Once every lane holds its 12 values the poses are dead, and the waves' 64 x 25
// term blocks lie over the staging blocks and the poses.
constexpr int MO_STAGE_ROWS = 32, MO_ROUND = MO_WAVES * MO_STAGE_ROWS;
constexpr int MO_STAGE = (MO_STAGE_ROWS + MO_HALO) * STAGE_COLS;   // a wave's staging block; also its 64 x 12 per-frame rows on their way out
constexpr int MO_POSES_AT = MO_WAVES * MO_STAGE, MO_STAMPS_AT = MO_POSES_AT + MO_WINDOW * POSE, MO_LDS = MO_STAMPS_AT + MO_WINDOW + 1;

static_assert(MO_SUMS <= MO_TSTRIDE && MO_SUMS + MO_REST == MACC && MO_SUMS <= 64, "one lane per column of the sums");
static_assert(64 * MW <= MO_STAGE && MO_WAVES * 64 * MO_TSTRIDE <= MO_STAMPS_AT, "what lies over the staging blocks and the poses fits");

struct MotionParams {
    const void* rows;
    const double* times;                                // [F] or NULL: the index clock
    void* motion;                                       // [n_sets, F, 12] or NULL
    double* part;                                       // [n_sets, (workgroups + R), 38] partial records, pair (b, r) at row b + r
    const int* starts;                                  // [R]
    const double* bodies;                               // [n_bodies, 9] (APE_ROWS_TARGETS)
    long long rows_stride, set_stride;
    int F, R, skip, layout, n_bodies, row_w;
};

__device__ __forceinline__ double norm3(double x, double y, double z) { return sqrt(x * x + y * y + z * z); }

// a message row -> the pose record of truth_pose: columns [4:7], [11:14], [7:11], [14:18], [21:25] (without hips: the identity, not read)
__device__ __forceinline__ void msg_pose(const double* m, bool hips, double* pose) {
    bool ok = true;
#pragma unroll
    for (int c = 0; c < 3; ++c) { pose[c] = m[4 + c]; pose[3 + c] = m[11 + c]; }
#pragma unroll
    for (int c = 0; c < 4; ++c) { pose[6 + c] = m[7 + c]; pose[10 + c] = m[14 + c]; pose[14 + c] = hips ? m[21 + c] : (c == 0 ? 1.0 : 0.0); }
#pragma unroll
    for (int c = 0; c < 18; ++c) ok = ok && fin(pose[c]);
    pose[18] = ok ? 1.0 : 0.0;
}

__device__ __forceinline__ void normalise4(double* q) {
    const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    q[0] = q[0] / n; q[1] = q[1] / n; q[2] = q[2] / n; q[3] = q[3] / n;
}

// the world-frame angular velocity over the step h from b to a (unit quaternions at a, b): d = a (x) conj(b), negated where d.w < 0.0,
// v its vector part, n = |v|: (2 atan2(n, d.w) / n) v / h, and 2 v / h below n = 1e-8
__device__ __forceinline__ Vec3 ang_vel(const double* a, const double* b, double h) {
    Quat d = qmul(Quat{a[0], a[1], a[2], a[3]}, Quat{b[0], -b[1], -b[2], -b[3]});
    if (d.w < 0.0) d = Quat{-d.w, -d.x, -d.y, -d.z};
    const double n = norm3(d.x, d.y, d.z);
    const double s = n >= 1e-8 ? (2.0 * atan2(n, d.w)) / n : 2.0;
    return Vec3{(s * d.x) / h, (s * d.y) / h, (s * d.z) / h};
}

// speed, acceleration and jerk of a position at p0 (frame f) .. p3 (frame f - 3): |d1|, 2 |d2|, 6 |d3| of the divided differences
__device__ __forceinline__ void lin_motion(const double* p0, const double* p1, const double* p2, const double* p3, double h1, double h2, double h3,
                                           double s2a, double s2b, double s3, double* out) {
    double d1a[3], d2a[3], d3a[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double a = (p0[c] - p1[c]) / h1, b = (p1[c] - p2[c]) / h2, e = (p2[c] - p3[c]) / h3;
        const double a2 = (a - b) / s2a, b2 = (b - e) / s2b;
        d1a[c] = a; d2a[c] = a2; d3a[c] = (a2 - b2) / s3;
    }
    out[0] = norm3(d1a[0], d1a[1], d1a[2]);
    out[1] = 2.0 * norm3(d2a[0], d2a[1], d2a[2]);
    out[2] = 6.0 * norm3(d3a[0], d3a[1], d3a[2]);
}

template <typename TRows, int KIND, typename TOut>
__global__ __launch_bounds__(MO_BLOCK) void ape_motion_kernel(const MotionParams p) {
    __shared__ double mem[MO_LDS];                      // staging blocks | poses | stamps; later the waves' term blocks from the front
    __shared__ double wfirst[MO_WAVES][MO_SUMS];
    __shared__ double wrest[MO_WAVES][MO_REST];
    __shared__ int wrec[MO_WAVES][2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int set = blockIdx.y;
    const long long tile0 = (long long)blockIdx.x * MO_BLOCK;
    const long long row0 = tile0 + wave * 64;
    const long long f = row0 + lane;
    const bool valid = f < p.F;
    const long long left = (long long)p.F - row0;
    const int nrows = left >= 64 ? 64 : (left > 0 ? (int)left : 0);
    double* lds = mem + wave * MO_STAGE;
    double* poses = mem + MO_POSES_AT;
    double* stamps = mem + MO_STAMPS_AT;
    const bool hips = p.layout != APE_LAYOUT_ORI_CAL_LARM_UARM;

    // the frame's recording; lanes past F form a recording of their own
    int rec = p.R, start = 0;
    if (valid) {
        rec = find_rec(p.starts, p.R, f);
        start = p.starts[rec];
    }

    // ---- poses and stamps of the window [wlo, whi): the tile's rows and the three below them, each row converted once ----
    const long long wlo = tile0 - MO_HALO > 0 ? tile0 - MO_HALO : 0;
    const long long whi = tile0 + MO_BLOCK < (long long)p.F ? tile0 + MO_BLOCK : (long long)p.F;
    const TRows* src = static_cast<const TRows*>(p.rows) + (long long)set * p.set_stride;
    const int rw = p.row_w, rls = rw | 1;
    if (p.times != nullptr) {
        for (long long i = wlo + threadIdx.x; i < whi; i += MO_BLOCK) stamps[i - wlo] = p.times[i];       // (at most twice)
    }
    const int halo = (int)(tile0 - wlo), wrows = (int)(whi - wlo);                      // rows of the window below the tile; all of them
    for (int base = 0; base < MO_BLOCK; base += MO_ROUND) {                            // (uniform) window rows [a, b): the wave's 32 of the round,
        const int own = base + wave * MO_STAGE_ROWS;                                    // counted from the tile's first; the first block takes the halo
        const int a = own == 0 ? 0 : own + halo, b = own + halo + MO_STAGE_ROWS < wrows ? own + halo + MO_STAGE_ROWS : wrows;
        const long long r0 = wlo + a;
        const int nr = b > a ? b - a : 0;               // (at most 35)
        if (nr > 0) stage_rows(lds, src, p.rows_stride, rw, rls, r0, nr, lane);
        __syncthreads();
        const bool tv = lane < nr;
        double t[STAGE_COLS];
#pragma unroll
        for (int c = 0; c < STAGE_COLS; ++c) t[c] = (tv && c < rw) ? lds[lane * rls + c] : 0.0;
        __syncthreads();
        if (tv) {
            const long long tr = r0 + lane;
            double* pose = poses + (size_t)(tr - wlo) * POSE;
            if constexpr (KIND == APE_ROWS_MSG) {
                msg_pose(t, hips, pose);
            } else if constexpr (KIND == APE_ROWS_EST) {
                truth_pose<APE_TRUTH_EST>(t, rw, p.layout, nullptr, pose);
            } else {
                const int trec = p.n_bodies > 1 ? find_rec(p.starts, p.R, tr) : 0;
                truth_pose<APE_TRUTH_TARGETS>(t, rw, p.layout, p.bodies + 9 * (size_t)trec, pose);
            }
            normalise4(pose + 6); normalise4(pose + 10); normalise4(pose + 14);
        }
    }
    const int prev = __shfl_up(rec, 1, 64);
    const unsigned long long bmask = __ballot(lane > 0 && rec != prev);
    if (lane == 0) wrec[wave][0] = rec;
    if (lane == 63) wrec[wave][1] = rec;
    __syncthreads();                                    // (every pose, every stamp and wrec are written)
    const int prev_last = wave > 0 ? wrec[wave - 1][1] : -1;

    // ---- the frame's 12 values from the poses of f, f-1, f-2, f-3 (all inside its recording, so inside the window) ----
    const bool deep = valid && (f - start) >= (long long)MO_HALO;
    const int at = deep ? (int)(f - wlo) : MO_HALO;      // (a lane that is not differenced reads rows 0 .. 3 of the window, or nothing it uses)
    const double* p0 = poses + (size_t)at * POSE;
    const double* p1 = p0 - POSE;
    const double* p2 = p1 - POSE;
    const double* p3 = p2 - POSE;
    bool ok = deep;
    double t0, t1, t2, t3;
    if (p.times != nullptr) {
        t0 = deep ? stamps[at] : 3.0; t1 = deep ? stamps[at - 1] : 2.0; t2 = deep ? stamps[at - 2] : 1.0; t3 = deep ? stamps[at - 3] : 0.0;
    } else {
        const double i0 = deep ? (double)(f - start) : 3.0;
        t0 = i0; t1 = i0 - 1.0; t2 = i0 - 2.0; t3 = i0 - 3.0;
    }
    const double h1 = t0 - t1, h2 = t1 - t2, h3 = t2 - t3;
    const double s2a = t0 - t2, s2b = t1 - t3, s3 = t0 - t3;
    ok = ok && fin(h1) && fin(h2) && fin(h3) && h1 > 0.0 && h2 > 0.0 && h3 > 0.0;
    double s[MW];
    if (deep) {
        ok = ok && p0[18] != 0.0 && p1[18] != 0.0 && p2[18] != 0.0 && p3[18] != 0.0;
        lin_motion(p0, p1, p2, p3, h1, h2, h3, s2a, s2b, s3, s);
        lin_motion(p0 + 3, p1 + 3, p2 + 3, p3 + 3, h1, h2, h3, s2a, s2b, s3, s + 3);
        const double half = s2a / 2.0;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            if (j == 2 && !hips) { s[8] = 0.0; s[11] = 0.0; continue; }
            const int q = 6 + 4 * j;
            const Vec3 wa = ang_vel(p0 + q, p1 + q, h1), wb = ang_vel(p1 + q, p2 + q, h2);
            s[6 + j] = norm3(wa.x, wa.y, wa.z);
            s[9 + j] = norm3(wa.x - wb.x, wa.y - wb.y, wa.z - wb.z) / half;
        }
#pragma unroll
        for (int c = 0; c < MW; ++c) ok = ok && fin(s[c]);
    }
    if (!ok) {
#pragma unroll
        for (int c = 0; c < MW; ++c) s[c] = NAN;
    }

    // ---- per-frame rows: through LDS so that the wave writes its 64 x 12 values as one run ----
    if (p.motion != nullptr) {
#pragma unroll
        for (int c = 0; c < MW; ++c) lds[lane * MW + c] = s[c];
        __syncthreads();
        const int total = nrows * MW;
        TOut* out = static_cast<TOut*>(p.motion) + ((size_t)set * (size_t)p.F + (size_t)row0) * MW;
#pragma unroll
        for (int it = 0; it < MW; ++it) {
            const int idx = it * 64 + lane;
            if (idx < total) out[idx] = (TOut)lds[idx];
        }
    }

    // ---- the frame's contribution; the support: f - start >= skip + 3 ----
    __syncthreads();                                    // (every lane has read its poses: the term blocks may lie over them)
    lds = mem + wave * (64 * MO_TSTRIDE);
    const bool sup = valid && (f - start) >= (long long)p.skip + MO_HALO;
    const bool in = sup && ok;
    double v[MO_REST];
#pragma unroll
    for (int c = 0; c < MW; ++c) {
        const double e = in ? s[c] : 0.0;
        lds[lane * MO_TSTRIDE + 2 * c] = e;
        lds[lane * MO_TSTRIDE + 2 * c + 1] = e * e;
        v[c] = e;
    }
    v[MW] = in ? 1.0 : 0.0;
    v[MW + 1] = (sup && !ok) ? 1.0 : 0.0;
    __syncthreads();
    double* part_row0 = p.part + ((size_t)set * ((size_t)gridDim.x + (size_t)p.R) + (size_t)blockIdx.x) * MACC;       // + r * MACC: the pair (b, r)
    double held = 0.0;
    bool holds = false;
    int held_rec = -1;
    sum_columns<MO_TSTRIDE, MO_WAVES>(lds, MO_SUMS, 0, rec, bmask, lane, wave, p.R, prev_last, wfirst[wave], part_row0, (size_t)MACC, &held, &holds, &held_rec);

    // maxima and counts: after the round with offset o, lane l holds the frames [l, l + 2 o) of its recording within the wave
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int orec = __shfl_down(rec, off, 64);
        const bool take = lane + off < 64 && orec == rec;
#pragma unroll
        for (int c = 0; c < MO_REST; ++c) {
            const double o = __shfl_down(v[c], off, 64);
            if (take) v[c] = c < MW ? fmax(v[c], o) : v[c] + o;
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < MO_REST; ++c) wrest[wave][c] = v[c];
    }
    __syncthreads();                                    // (every wave's leading run is in wfirst and wrest)
    // the wave whose last run starts a (workgroup, recording) pair takes the following waves' leading runs in wave order
    if (holds) {                                        // (uniform)
        for (int w = wave + 1; w < MO_WAVES; ++w) {
            if (wrec[w][0] != held_rec) break;
            if (lane < MO_SUMS) held = held + wfirst[w][lane];
            if (wrec[w][1] != held_rec) break;
        }
        if (lane < MO_SUMS) part_row0[(size_t)held_rec * MACC + lane] = held;
    }
    // the first frame of every (workgroup, recording) pair does the same for the maxima and counts
    if (valid && (f == start || threadIdx.x == 0)) {
        if (wrec[wave][1] == rec) {
            for (int w = wave + 1; w < MO_WAVES; ++w) {
                if (wrec[w][0] != rec) break;
#pragma unroll
                for (int c = 0; c < MO_REST; ++c) v[c] = c < MW ? fmax(v[c], wrest[w][c]) : v[c] + wrest[w][c];
                if (wrec[w][1] != rec) break;
            }
        }
        double* dst = part_row0 + (size_t)rec * MACC + MO_SUMS;
#pragma unroll
        for (int c = 0; c < MO_REST; ++c) dst[c] = v[c];
    }
}

// workgroup (r, set): recording r's pairs (b, r), b = first .. last workgroup of its frames, at rows b + r of the set's partial records.
// Thread (g, c): column c of the pairs g, g + 4, ... in order; then the four groups in order (sums_acc's order).  Column c of a partial
// record lands in its slot of the 38: sums and squares at 3k, 3k + 1, maxima at 3k + 2, the counts at 36, 37.
__global__ __launch_bounds__(MO_BLOCK) void ape_motion_acc_kernel(const double* __restrict__ part, const int* __restrict__ starts, int R, int F,
                                                                  int blocks, double* __restrict__ acc) {
    __shared__ double grp[MO_BLOCK / 64][64];
    const int r = blockIdx.x, set = blockIdx.y, c = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int s = starts[r], e = (r + 1 < R ? starts[r + 1] : F) - 1;
    const int b0 = s / MO_BLOCK, n = e / MO_BLOCK - b0 + 1;
    const bool mx = c >= MO_SUMS && c < MO_SUMS + MW;
    double a = 0.0;
    if (c < MACC) {
        const double* src = part + ((size_t)set * ((size_t)blocks + (size_t)R) + (size_t)b0 + (size_t)r) * MACC + c;
        int i = g;
        for (; i + 12 < n; i += 16) {                   // four independent loads in flight, combined in order
            const double x0 = src[(size_t)i * MACC], x1 = src[(size_t)(i + 4) * MACC], x2 = src[(size_t)(i + 8) * MACC],
                         x3 = src[(size_t)(i + 12) * MACC];
            if (mx) a = fmax(fmax(fmax(fmax(a, x0), x1), x2), x3);
            else a = (((a + x0) + x1) + x2) + x3;
        }
        for (; i < n; i += 4) {
            const double x = src[(size_t)i * MACC];
            a = mx ? fmax(a, x) : a + x;
        }
    }
    grp[g][c] = a;
    __syncthreads();
    if (g == 0 && c < MACC) {
        double o = grp[0][c];
#pragma unroll
        for (int k = 1; k < MO_BLOCK / 64; ++k) o = mx ? fmax(o, grp[k][c]) : o + grp[k][c];
        const int slot = c < MO_SUMS ? 3 * (c >> 1) + (c & 1) : (mx ? 3 * (c - MO_SUMS) + 2 : c);
        acc[((size_t)set * (size_t)R + (size_t)r) * MACC + slot] = o;
    }
}

// the staging of a call: starts and bodies in, the partial records behind them (score_host.h)
ApeSlotPool g_pool("motion_sums");

template <typename TRows, typename TOut>
void launch_motion(const MotionParams& p, int kind, dim3 grid, hipStream_t st) {
    if (kind == APE_ROWS_MSG) hipLaunchKernelGGL((ape_motion_kernel<TRows, APE_ROWS_MSG, TOut>), grid, dim3(MO_BLOCK), 0, st, p);
    else if (kind == APE_ROWS_EST) hipLaunchKernelGGL((ape_motion_kernel<TRows, APE_ROWS_EST, TOut>), grid, dim3(MO_BLOCK), 0, st, p);
    else hipLaunchKernelGGL((ape_motion_kernel<TRows, APE_ROWS_TARGETS, TOut>), grid, dim3(MO_BLOCK), 0, st, p);
}

// values of a row of a scoring layout
int rows_width(int32_t layout, int32_t kind) {
    if (kind == APE_ROWS_MSG) return 25;
    return ape_truth_width(layout, kind == APE_ROWS_TARGETS ? APE_TRUTH_TARGETS : APE_TRUTH_EST);
}

}  // namespace

int ape_motion_sums(int32_t layout, const void* rows_dev, int32_t rows_kind, int32_t rows_stride, int32_t rows_dtype, int32_t n_sets,
                    int64_t set_stride, int32_t F, const int32_t* seg_starts_host, int32_t R, int32_t skip, const double* times_dev,
                    const double* bodies_host, int32_t n_bodies, void* motion_dev, int32_t out_dtype, double* acc_dev, void* stream) {
    const char* who = "motion_sums";
    if (!rows_dev || !seg_starts_host || !acc_dev) return ape_fail(APE_ERR_INVALID_ARG, "%s: NULL argument", who);
    if (!ape_scoring_layout(layout)) return ape_fail(APE_ERR_INVALID_ARG, "%s: layout %d has no pose to difference", who, layout);
    if (rows_kind != APE_ROWS_MSG && rows_kind != APE_ROWS_EST && rows_kind != APE_ROWS_TARGETS)
        return ape_fail(APE_ERR_INVALID_ARG, "%s: unknown rows kind %d", who, rows_kind);
    if ((rows_dtype != APE_F32 && rows_dtype != APE_F64) || (out_dtype != APE_F32 && out_dtype != APE_F64))
        return ape_fail(APE_ERR_INVALID_ARG, "%s: unknown dtype selector", who);
    if (int rc = ape_check_segments(who, F, seg_starts_host, R)) return rc;
    if (skip < 0) return ape_fail(APE_ERR_INVALID_ARG, "%s: skip %d is negative", who, skip);
    const int rw = rows_width(layout, rows_kind);
    if (rows_stride < rw) return ape_fail(APE_ERR_INVALID_ARG, "%s: rows_stride %d below the row width %d", who, rows_stride, rw);
    if (n_sets < 1 || n_sets > APE_POST_MAX_CONFIGS)
        return ape_fail(APE_ERR_INVALID_ARG, "%s: n_sets %d, between 1 and %d", who, n_sets, APE_POST_MAX_CONFIGS);
    if (n_sets > 1 && set_stride < (int64_t)F * (int64_t)rows_stride)
        return ape_fail(APE_ERR_INVALID_ARG, "%s: set_stride %lld below F * rows_stride = %lld", who, (long long)set_stride,
                        (long long)F * (long long)rows_stride);
    if (rows_kind == APE_ROWS_TARGETS) {
        if (!bodies_host) return ape_fail(APE_ERR_INVALID_ARG, "%s: NULL bodies_host with target rows", who);
        if (n_bodies != 1 && n_bodies != R) return ape_fail(APE_ERR_INVALID_ARG, "%s: n_bodies %d is neither 1 nor R = %d", who, n_bodies, R);
    }
    if ((const void*)acc_dev == rows_dev || (const void*)acc_dev == (const void*)times_dev)
        return ape_fail(APE_ERR_INVALID_ARG, "%s: acc_dev aliases an input", who);
    if (motion_dev && ((const void*)motion_dev == rows_dev || (const void*)motion_dev == (const void*)times_dev || motion_dev == (void*)acc_dev))
        return ape_fail(APE_ERR_INVALID_ARG, "%s: motion_dev aliases an input or acc_dev", who);
    const hipStream_t st = (hipStream_t)stream;
    if (int rc = ape_check_not_capturing(st, who, "host arrays are staged per call")) return rc;
    int device = 0;
    APE_SCORE_TRY(g_pool.prefix, hipGetDevice(&device));

    const bool targets = rows_kind == APE_ROWS_TARGETS;
    const unsigned blocks = (unsigned)(((long long)F + MO_BLOCK - 1) / MO_BLOCK);
    const size_t starts_bytes = (((size_t)R * sizeof(int)) + 7) & ~(size_t)7;       // starts, then the bodies
    const size_t bodies_bytes = targets ? (size_t)n_bodies * 9 * sizeof(double) : 0;
    const size_t host_bytes = starts_bytes + bodies_bytes;
    const size_t part_bytes = (size_t)n_sets * ((size_t)blocks + (size_t)R) * MACC * sizeof(double);

    std::lock_guard<std::mutex> lock(g_pool.mu);
    ApeSlot* slot = nullptr;
    if (int rc = g_pool.take(device, host_bytes, host_bytes + part_bytes, &slot)) return rc;
    char* pin = static_cast<char*>(slot->pinned);
    memcpy(pin, seg_starts_host, (size_t)R * sizeof(int));
    if (targets) memcpy(pin + starts_bytes, bodies_host, bodies_bytes);
    // (a copy that fails leaves through finish() like a launch that fails: the slot's event is recorded either way)
    const hipError_t copied = hipMemcpyAsync(slot->dev, slot->pinned, host_bytes, hipMemcpyHostToDevice, st);
    if (copied != hipSuccess) return g_pool.finish(who, slot, copied, st);

    MotionParams p{};
    char* dev = static_cast<char*>(slot->dev);
    p.rows = rows_dev; p.times = times_dev; p.motion = motion_dev;
    p.starts = reinterpret_cast<const int*>(dev);
    p.bodies = reinterpret_cast<const double*>(dev + starts_bytes);
    p.part = reinterpret_cast<double*>(dev + host_bytes);
    p.rows_stride = rows_stride; p.set_stride = n_sets > 1 ? (long long)set_stride : 0;
    p.F = F; p.R = R; p.skip = skip; p.layout = layout; p.n_bodies = targets ? n_bodies : 1; p.row_w = rw;

    const dim3 grid(blocks, (unsigned)n_sets);
    if (rows_dtype == APE_F32 && out_dtype == APE_F32) launch_motion<float, float>(p, rows_kind, grid, st);
    else if (rows_dtype == APE_F32) launch_motion<float, double>(p, rows_kind, grid, st);
    else if (out_dtype == APE_F32) launch_motion<double, float>(p, rows_kind, grid, st);
    else launch_motion<double, double>(p, rows_kind, grid, st);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) {
        hipLaunchKernelGGL(ape_motion_acc_kernel, dim3((unsigned)R, (unsigned)n_sets), dim3(MO_BLOCK), 0, st, p.part, p.starts, R, F, (int)blocks, acc_dev);
        e = hipGetLastError();
    }
    return g_pool.finish(who, slot, e, st);
}
