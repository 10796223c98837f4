// Device helpers of body_fit.hip: row staging, the recording of a frame, one truth row -> pose, the rotation a quaternion
// stands for.  They state what score.hip and frame_fit.hip state in their own copies (stage_rows, find_rec, truth_pose, quat_matrix):
// those files keep their copies, so that their object code stays what it was; switching them to this header is a change of its own.
// float64 with separate roundings for a * b + c: the including file turns contraction off before it includes this one.
#pragma once
#include "../../include/ape_hip.h"
#include "fk_device.h"

namespace ape_bodydev {

using namespace ape_fkdev;

constexpr int STAGE_COLS = 25;                          // widest staged input row (the message)
constexpr int POSE = 19;                                // 18 pose values + the usable flag; odd

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

// (score.hip: truth_six_drr_to_quat) the closed form refined by two power steps on K + I to the eigenvector the reference takes
__device__ inline Quat truth_six_drr_to_quat(const double* s) {
    const Quat q0 = six_drr_to_quat(s);
    const double a1x = s[0], a1y = s[2], a1z = s[4], a2x = s[1], a2y = s[3], a2z = s[5];
    const double n1 = sqrt(a1x * a1x + a1y * a1y + a1z * a1z);
    const double m00 = a1x / n1, m10 = a1y / n1, m20 = a1z / n1;
    const double d = m00 * a2x + m10 * a2y + m20 * a2z;
    const double ux = a2x - d * m00, uy = a2y - d * m10, uz = a2z - d * m20;
    const double n2 = sqrt(ux * ux + uy * uy + uz * uz);
    const double m01 = ux / n2, m11 = uy / n2, m21 = uz / n2;
    const double m02 = m10 * m21 - m20 * m11, m12 = m20 * m01 - m00 * m21, m22 = m00 * m11 - m10 * m01;
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

// one truth row -> pose[0:18] = hand, elbow, lower-arm, upper-arm and hips quaternion, pose[18] = 1.0 iff every value used is finite.
// APE_TRUTH_TARGETS: the targets of APE_LAYOUT_ORI_POS_CAL_LARM_UARM_HIPS only, which carry their positions (the two other layouts'
// positions would be made with a body: the host refuses them)
template <int KIND>
__device__ __forceinline__ void truth_pose(const double* t, int tw, int layout, double* pose) {
    const bool hips = layout != APE_LAYOUT_ORI_CAL_LARM_UARM;
    Vec3 t_hand, t_elbow;
    Quat t_lq, t_uq, t_hq{1.0, 0.0, 0.0, 0.0};
    bool ok = true;
    if constexpr (KIND == APE_TRUTH_TARGETS) {
#pragma unroll
        for (int c = 0; c < 20; ++c)
            if (c < tw) ok = ok && fin(t[c]);
        t_lq = truth_six_drr_to_quat(t + 3); t_uq = truth_six_drr_to_quat(t + 12); t_hq = hips_quat(t[18], t[19]);
        t_hand = Vec3{t[0], t[1], t[2]}; t_elbow = Vec3{t[9], t[10], t[11]};
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

}  // namespace ape_bodydev
