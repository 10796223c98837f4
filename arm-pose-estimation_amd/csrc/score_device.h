// Device helpers of the scoring kernels (score.hip, frame_fit.hip, body_fit.hip, resample.hip, post_sweep.hip, motion.hip), each
// stated once: row staging, the recording of a frame, the slot of a value over edges, one truth row -> pose, the rotation a quaternion stands for, the ordered column
// sums of a wave's terms and the ordered sum of a recording's partial records.
// float64 with separate roundings for a * b + c, like the numpy statements (score.py): the including file turns contraction off BEFORE
// it includes this header (there is no pragma here: a file that forgot would contract these statements, not half of them).
#pragma once
#include "../../include/ape_hip.h"
#include "fk_device.h"

namespace ape_scoredev {

using namespace ape_fkdev;

constexpr int STAGE_COLS = 25;                          // widest staged input row (the message); the rounds of stage_rows
constexpr int POSE = 19;                                // 18 pose values + the usable flag; odd: no bank conflicts

// rows row0 .. row0 + nrows - 1 (nrows >= 1), columns 0 .. ncols - 1 of src -> lds[r * lstride + c] as float64.  Every lane loads in
// every round (the index is clamped, a partial wave reads its last element again): no branch between the loads
template <typename T>
__device__ __forceinline__ void stage_rows(double* lds, const T* src, long long stride, int ncols, int lstride, long long row0, int nrows,
                                           int lane) {
    const int last = nrows * ncols - 1;
#pragma unroll
    for (int it = 0; it < STAGE_COLS; ++it) {
        if (it < ncols) {                               // uniform
            int idx = it * 64 + lane;
            idx = idx < last ? idx : last;
            const int r = idx / ncols, c = idx - r * ncols;
            lds[r * lstride + c] = (double)src[(row0 + r) * stride + c];
        }
    }
}

__device__ __forceinline__ bool fin(double v) { return isfinite(v); }

__device__ __forceinline__ int find_rec(const int* starts, int R, long long f) {      // the last start <= f
    int lo = 0, hi = R - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if ((long long)starts[mid] <= f) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// the slot of v over the edges e[0 .. B] (LDS), as include/ape_hip.h states it for ape_score_hist: comparisons only
__device__ __forceinline__ int find_slot(const double* e, int B, double v) {
    if (v != v) return B + 2;
    int lo = 0, n = B + 1;                              // the edges below v are e[0 .. lo) once n == 0
    while (n > 0) {                                     // (at most 9 rounds for 257 edges)
        const int half = n >> 1;
        if (e[lo + half] < v) { lo += half + 1; n -= half + 1; } else n = half;
    }
    return lo == 0 ? B : (lo > B ? B + 1 : lo - 1);
}

// The truth's 6D rotation -> unit quaternion, in the reference's sense.  rot_mat_to_quat (transformations.py:521-545) takes the dominant
// eigenvector of the symmetric 4x4 matrix K(R) / 3; six_drr_to_quat (fk_device.h) is its closed form for an orthonormal R.  Where the two
// 6D columns are nearly parallel, Gram-Schmidt leaves R up to 1e-11 off orthonormal and the two pick quaternions up to 4e-12 apart --
// nothing beside a prediction's own error, but truth is compared at 1e-13.  So the closed form is the start of two power steps on
// K + I, whose eigenvalues are 4 and three of the size of R's defect: each step multiplies the distance to the eigenvector by that
// defect, and the result is the reference's to rounding (7e-16 on the fixtures after one step).  NaN propagates as in six_drr_to_quat.
__device__ inline Quat truth_six_drr_to_quat(const double* s) {
    const Quat q0 = six_drr_to_quat(s);
    // R = [b1 b2 b3] as columns, the arithmetic of six_drr_to_quat (transformations.py:602-637)
    const double a1x = s[0], a1y = s[2], a1z = s[4], a2x = s[1], a2y = s[3], a2z = s[5];
    const double n1 = sqrt(a1x * a1x + a1y * a1y + a1z * a1z);
    const double m00 = a1x / n1, m10 = a1y / n1, m20 = a1z / n1;
    const double d = m00 * a2x + m10 * a2y + m20 * a2z;
    const double ux = a2x - d * m00, uy = a2y - d * m10, uz = a2z - d * m20;
    const double n2 = sqrt(ux * ux + uy * uy + uz * uz);
    const double m01 = ux / n2, m11 = uy / n2, m21 = uz / n2;
    const double m02 = m10 * m21 - m20 * m11, m12 = m20 * m01 - m00 * m21, m22 = m00 * m11 - m10 * m01;
    // K + I in the reference's (x, y, z, w) order (transformations.py:575-584, times 3)
    const double k00 = m00 - m11 - m22 + 1.0, k11 = m11 - m00 - m22 + 1.0, k22 = m22 - m00 - m11 + 1.0, k33 = m00 + m11 + m22 + 1.0;
    const double k01 = m01 + m10, k02 = m02 + m20, k12 = m12 + m21, k03 = m21 - m12, k13 = m02 - m20, k23 = m10 - m01;
    double x = q0.x, y = q0.y, z = q0.z, w = q0.w;
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const double nx = k00 * x + k01 * y + k02 * z + k03 * w, ny = k01 * x + k11 * y + k12 * z + k13 * w;
        const double nz = k02 * x + k12 * y + k22 * z + k23 * w, nw = k03 * x + k13 * y + k23 * z + k33 * w;
        const double nn = sqrt(nx * nx + ny * ny + nz * nz + nw * nw);
        x = nx / nn; y = ny / nn; z = nz / nn; w = nw / nn;
    }
    return w < 0.0 ? Quat{-w, -x, -y, -z} : Quat{w, x, y, z};
}

// What a row of NN targets stands for: hand and elbow, the shoulder origin under the hips rotation (uo; the body's own without hips),
// the lower-arm, upper-arm and hips quaternion (the identity without hips).  NaN propagates.
struct TargetPose {
    Vec3 hand, elbow, uo;
    Quat lq, uq, hq;
};

// body = larm_vec, uarm_vec, uarm_orig.  A caller that does not use `uo` pays nothing for it where the positions are targets.
__device__ __forceinline__ TargetPose targets_to_pose(const double* t, int layout, const double* body) {
    const bool hips = layout != APE_LAYOUT_ORI_CAL_LARM_UARM;
    const Vec3 larm_vec{body[0], body[1], body[2]}, uarm_vec{body[3], body[4], body[5]}, uarm_orig{body[6], body[7], body[8]};
    TargetPose o;
    o.uo = uarm_orig;
    o.hq = Quat{1.0, 0.0, 0.0, 0.0};
    if (layout == APE_LAYOUT_ORI_POS_CAL_LARM_UARM_HIPS) {             // estimate_joints.py:20-45: positions are targets
        o.lq = truth_six_drr_to_quat(t + 3); o.uq = truth_six_drr_to_quat(t + 12); o.hq = hips_quat(t[18], t[19]);
        o.hand = Vec3{t[0], t[1], t[2]}; o.elbow = Vec3{t[9], t[10], t[11]};
        o.uo = qrot(o.hq, uarm_orig);
    } else {                                                           // estimate_joints.py:48-71, 74-92
        o.lq = truth_six_drr_to_quat(t); o.uq = truth_six_drr_to_quat(t + 6);
        if (hips) { o.hq = hips_quat(t[12], t[13]); o.uo = qrot(o.hq, uarm_orig); }
        const Vec3 r1 = qrot(o.uq, uarm_vec);
        o.elbow = Vec3{r1.x + o.uo.x, r1.y + o.uo.y, r1.z + o.uo.z};
        const Vec3 r2 = qrot(o.lq, larm_vec);
        o.hand = Vec3{r2.x + o.elbow.x, r2.y + o.elbow.y, r2.z + o.elbow.z};
    }
    return o;
}

// one truth row -> pose[0:18] = hand, elbow, lower-arm, upper-arm and hips quaternion, pose[18] = 1.0 iff every value used is finite.
// APE_TRUTH_EST: the est columns as given (body is not read).  APE_TRUTH_TARGETS: the first tw of t must be finite, then
// targets_to_pose with the recording's body.
template <int KIND>
__device__ __forceinline__ void truth_pose(const double* t, int tw, int layout, const double* body, double* pose) {
    const bool hips = layout != APE_LAYOUT_ORI_CAL_LARM_UARM;
    Vec3 t_hand, t_elbow;
    Quat t_lq, t_uq, t_hq{1.0, 0.0, 0.0, 0.0};
    bool ok = true;
    if constexpr (KIND == APE_TRUTH_TARGETS) {
#pragma unroll
        for (int c = 0; c < 20; ++c)
            if (c < tw) ok = ok && fin(t[c]);
        const TargetPose o = targets_to_pose(t, layout, body);
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
    pose[0] = t_hand.x; pose[1] = t_hand.y; pose[2] = t_hand.z; pose[3] = t_elbow.x; pose[4] = t_elbow.y; pose[5] = t_elbow.z;
    pose[6] = t_lq.w; pose[7] = t_lq.x; pose[8] = t_lq.y; pose[9] = t_lq.z;
    pose[10] = t_uq.w; pose[11] = t_uq.x; pose[12] = t_uq.y; pose[13] = t_uq.z;
    pose[14] = t_hq.w; pose[15] = t_hq.x; pose[16] = t_hq.y; pose[17] = t_hq.z;
    pose[18] = ok ? 1.0 : 0.0;
}

// the rotation a quaternion [w, x, y, z] stands for, row-major, with the factor 2 / |q|^2: an unnormalised quaternion gives the same
// matrix as its unit form, the zero quaternion gives non-finite entries (score.py: _quat_matrix states the same operations)
__device__ __forceinline__ void quat_matrix(const double* q, double* m) {
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    const double s = 2.0 / (w * w + x * x + y * y + z * z);
    const double xx = x * x, yy = y * y, zz = z * z, xy = x * y, xz = x * z, yz = y * z, wx = w * x, wy = w * y, wz = w * z;
    m[0] = 1.0 - s * (yy + zz); m[1] = s * (xy - wz);       m[2] = s * (xz + wy);
    m[3] = s * (xy + wz);       m[4] = 1.0 - s * (xx + zz); m[5] = s * (yz - wx);
    m[6] = s * (xz - wy);       m[7] = s * (yz + wx);       m[8] = 1.0 - s * (xx + yy);
}

// Column c0 + lane (lane < nc) of the wave's terms tb[frame * TSTRIDE + lane], summed in frame order per run of one recording.
// A run that continues the previous wave's last recording goes to wf[c0 + lane]; the wave's last run is returned in `held` when a
// following wave may continue it (*holds, wave-uniform); every other run is a complete (workgroup, recording) pair and goes to its
// partial record.  rec: the lane's recording (R: past F); bmask: bit i set iff frame i > 0 starts a run; WAVES: waves of the workgroup.
template <int TSTRIDE, int WAVES>
__device__ __forceinline__ void sum_columns(const double* tb, int nc, int c0, int rec, unsigned long long bmask, int lane, int wave, int R,
                                            int prev_last, double* wf, double* part_row0, size_t rec_step, double* held, bool* holds, int* held_rec) {
    int a = 0;
    while (a < 64) {                                    // (uniform)
        const int b = bmask ? __ffsll((long long)bmask) - 1 : 64;
        bmask &= bmask - 1;
        const int r = __shfl(rec, a, 64);
        if (r < R) {
            double s = 0.0;
            if (lane < nc) {
                const double* src = tb + lane;
                int i = a;
                for (; i + 8 <= b; i += 8) {            // eight loads in flight, added in frame order
                    const double x0 = src[(i + 0) * TSTRIDE], x1 = src[(i + 1) * TSTRIDE], x2 = src[(i + 2) * TSTRIDE],
                                 x3 = src[(i + 3) * TSTRIDE], x4 = src[(i + 4) * TSTRIDE], x5 = src[(i + 5) * TSTRIDE],
                                 x6 = src[(i + 6) * TSTRIDE], x7 = src[(i + 7) * TSTRIDE];
                    s = (((((((s + x0) + x1) + x2) + x3) + x4) + x5) + x6) + x7;
                }
                for (; i < b; ++i) s = s + src[i * TSTRIDE];
            }
            if (a == 0 && wave > 0 && prev_last == r) {
                if (lane < nc) wf[c0 + lane] = s;
            } else if (b == 64 && wave + 1 < WAVES) {
                *held = s; *holds = true; *held_rec = r;
            } else if (lane < nc) {
                part_row0[(size_t)r * rec_step + c0 + lane] = s;
            }
        }
        a = b;
    }
}

// The body of a sums-acc kernel.  Workgroup (r, j) of BLOCK threads: recording r at sweep index j, its pairs (b, r), b = first .. last
// workgroup (of BLOCK frames) of its frames, at rows (b + r) * L + j of W columns.  Thread (g, c): column c of the pairs g, g + 4, ...
// in order; then the groups in order.
template <int W, int BLOCK>
__device__ __forceinline__ void sums_acc(const double* __restrict__ part, const int* __restrict__ starts, int R, int F, int L,
                                         double* __restrict__ acc) {
    static_assert(W <= 64 && BLOCK % 64 == 0, "one lane per column");
    __shared__ double grp[BLOCK / 64][64];
    const int r = blockIdx.x, j = blockIdx.y, c = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int s = starts[r], e = (r + 1 < R ? starts[r + 1] : F) - 1;
    const int b0 = s / BLOCK, n = e / BLOCK - b0 + 1;
    const size_t step = (size_t)L * W;
    double a = 0.0;
    if (c < W) {
        const double* src = part + (((size_t)b0 + (size_t)r) * (size_t)L + (size_t)j) * W + c;
        int i = g;
        for (; i + 12 < n; i += 16) {                   // four independent loads in flight, added in order
            const double x0 = src[(size_t)i * step], x1 = src[(size_t)(i + 4) * step], x2 = src[(size_t)(i + 8) * step],
                         x3 = src[(size_t)(i + 12) * step];
            a = (((a + x0) + x1) + x2) + x3;
        }
        for (; i < n; i += 4) a = a + src[(size_t)i * step];
    }
    grp[g][c] = a;
    __syncthreads();
    if (g == 0 && c < W) {
        double o = grp[0][c];
#pragma unroll
        for (int k = 1; k < BLOCK / 64; ++k) o = o + grp[k][c];
        acc[((size_t)r * (size_t)L + (size_t)j) * W + c] = o;
    }
}

}  // namespace ape_scoredev
