// The post-filter pass over a replay's stored targets, behind its three entries ape_post_sweep (post_sweep.hip),
// ape_post_window (post_window.hip) and ape_post_select (post_select.hip): the driver the fronts call, the
// conversion of sample rows to est rows, done once per call, and the per-device workspace the converted rows live in.
//
// post_filter   the one plan and host driver, defined in post_window.hip beside the kernels.  A front checks its own arguments, states
//               its configurations as windows (back, ahead, samples) and calls it under its own name.
// post_window_args  the checks of a list of windows and of what goes with it, for the two fronts that take one.
// post_fk_rows  the body of the conversion kernel: sample rows k < Mx of a run of frames -> est rows.  ape_fk3_kernel's
//               decomposition (fk.hip: a row's three chains side by side, 32 rows per workgroup of two waves) and its statements, with
//               the row index mapped: compact row r = frame r / Mx, sample r % Mx.  Launch with 128 threads and
//               ceil(rows / POST_FK_ROWS) workgroups.
// PostWorkspace the chunk buffers and the staged host arrays of one device.  Kept and grown on demand; a call waits (on its stream) for
//               the event recorded behind the last one, so calls on different streams do not share it at the same time.  post_filter
//               owns the one list and its mutex: the library keeps one buffer per device, and a sweep and a window call on different
//               streams of one device are ordered after one another, as two sweeps are.
//
// float64 with separate roundings for a * b + c, like numpy: contraction is off inside every device function here.
#pragma once
#include "ape_internal.h"
#include "../../include/ape_hip.h"
#include "stream_post_device.h"
#include "score_device.h"

#include <vector>

namespace ape_postcommon {

constexpr int POST_FK_ROWS = 32;                        // rows per workgroup of the conversion (FK3_ROWS of fk.hip)

struct PostFkParams {
    const float* y;                                     // [F, M, O]
    double* est;                                        // the first fresh row of the chunk buffer
    const double* yy_m;
    const double* yy_s;
    const int* starts;                                  // [R]
    const double* bodies;                               // [R, 9] or nullptr: `body` for every row
    double body[9];
    int rows;                                           // fresh frames x Mx
    int f_lo;                                           // the first fresh frame
    int R, M, Mx, O, W, layout;
};

__device__ __forceinline__ void post_fk_rows(const PostFkParams& p) {
#pragma clang fp contract(off)
    using namespace ape_postdev;
    using ape_scoredev::find_rec;
    __shared__ double rot[POST_FK_ROWS][3][3];             // [row][lower arm, upper arm, shoulder origin][xyz]
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const bool hips = p.layout != APE_LAYOUT_ORI_CAL_LARM_UARM;
    const bool full = p.layout != APE_LAYOUT_ORI_CAL_LARM_UARM_HIPS && hips;
    const int c_l = full ? 3 : 0, c_u = full ? 12 : 6, c_h = full ? 18 : 12;
    const int e_lq = hips ? 9 : 6, e_uq = hips ? 13 : 10, e_hq = 17;
    auto load = [&](const float* src, int c) -> double {
        double v = (double)src[c];
        v = v * p.yy_s[c] + p.yy_m[c];                     // de-normalisation in f64: estimator.py:108-109
        return v;
    };
    auto src_of = [&](int row, int* frame) -> const float* {
        const int fc = row / p.Mx, k = row - fc * p.Mx;
        *frame = p.f_lo + fc;
        return p.y + ((size_t)(p.f_lo + fc) * p.M + k) * p.O;
    };
    auto body_of = [&](int frame) -> const double* {
        return p.bodies != nullptr ? p.bodies + 9 * (size_t)find_rec(p.starts, p.R, frame) : p.body;
    };
    if (wave == 0) {
        const int r = lane >> 1, sub = lane & 1;
        const int row = blockIdx.x * POST_FK_ROWS + r;
        if (row < p.rows) {
            int frame;
            const float* src = src_of(row, &frame);
            double* dst = p.est + (size_t)row * p.W;
            double s6[6];
#pragma unroll
            for (int c = 0; c < 6; ++c) s6[c] = load(src, (sub ? c_u : c_l) + c);
            const Quat q = six_drr_to_quat(s6);
            const double* const body = body_of(frame);
            const Vec3 bone = sub ? Vec3{body[3], body[4], body[5]} : Vec3{body[0], body[1], body[2]};
            const Vec3 v = qrot(q, bone);
            rot[r][sub][0] = v.x; rot[r][sub][1] = v.y; rot[r][sub][2] = v.z;
            const int eq = sub ? e_uq : e_lq;
            dst[eq] = q.w; dst[eq + 1] = q.x; dst[eq + 2] = q.y; dst[eq + 3] = q.z;
        }
    } else {
        const int r = lane & 31;
        const int row = blockIdx.x * POST_FK_ROWS + r;
        if (row < p.rows) {
            int frame;
            const float* src = src_of(row, &frame);
            double* dst = p.est + (size_t)row * p.W;
            if (lane < 32) {
                const double* const body = body_of(frame);
                Vec3 uo{body[6], body[7], body[8]};
                if (hips) {
                    const Quat hq = hips_quat(load(src, c_h), load(src, c_h + 1));
                    uo = qrot(hq, uo);
                    dst[e_hq] = hq.w; dst[e_hq + 1] = hq.x; dst[e_hq + 2] = hq.y; dst[e_hq + 3] = hq.z;
                    dst[6] = uo.x; dst[7] = uo.y; dst[8] = uo.z;
                }
                rot[r][2][0] = uo.x; rot[r][2][1] = uo.y; rot[r][2][2] = uo.z;
            } else if (full) {                               // hand and lower-arm positions are network outputs here
#pragma unroll
                for (int c = 0; c < 3; ++c) { dst[c] = load(src, c); dst[3 + c] = load(src, 9 + c); }
            }
        }
    }
    __syncthreads();
    if (wave == 0 && !full) {
        const int r = lane >> 1, c = lane & 1;             // two lanes per row: the lower-arm origin / the hand origin
        const int row = blockIdx.x * POST_FK_ROWS + r;
        if (row < p.rows) {
            double* dst = p.est + (size_t)row * p.W;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double lo = rot[r][1][k] + rot[r][2][k];                 // qrot(uq, uarm_vec) + uo
                if (c == 0) dst[3 + k] = lo;
                else dst[k] = rot[r][0][k] + lo;                               // qrot(lq, larm_vec) + lo
            }
        }
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------
// The pass itself, for arguments the front has checked on their own: refuses what the model does not allow, plans, stages the host
// arrays and launches.  `who` / `sets`: the front's name and its word for its list, for the error texts.  windows_host int32 [C, 3]
// (back, ahead, samples); weights_host [C, APE_POST_MAX_WINDOW] frame weights or nullptr; tapered [C] (nullptr: none): which windows
// take their row of the weights, every other one is uniform.  sel_dev nullptr: every frame at every window, out [C, F, ...].  sel_dev
// uint8 [S, F] on the device: the windows are a ladder kept in the caller's order, frame f of set s runs window sel[s, f] alone, out
// [S, F, ...], a value >= C gives a row of NaN; the plan counts S where it counts lanes and C where it sizes the weight table.
// workspace_bytes 0: the default bound.  On success last4 receives the plan: passes, frames per pass, frames per tile, staged in LDS.
int post_filter(const char* who, const char* sets, ape_model_t* m, const float* y_dev, int F, int n_mc, const int32_t* seg_starts_host, int R,
                const int32_t* windows_host, const double* weights_host, const bool* tapered, int C, const unsigned char* sel_dev, int S,
                uint32_t flags, const double* bodies_host, int n_bodies, void* out_dev, int out_dtype, long long workspace_bytes, void* stream,
                int last4[4]);

// What ape_post_window refuses on the arguments alone (no device needed), under the name `who`: the recordings, n_mc, the C windows
// windows_host [C, 3] with weights_host [C, APE_POST_MAX_WINDOW] or nullptr, the bodies rule, flags, out_dtype, workspace_bytes.
// tapered [APE_POST_MAX_CONFIGS], all false on entry, receives which windows take their row of the weights (not all of its entries
// bit-equal).
int post_window_args(const char* who, const void* y_dev, const void* out_dev, int F, int n_mc, const int32_t* seg_starts_host, int R,
                     const int32_t* windows_host, const double* weights_host, int C, uint32_t flags, const double* bodies_host, int n_bodies,
                     int out_dtype, long long workspace_bytes, bool* tapered);

struct PostWorkspace {
    void* dev = nullptr;
    size_t cap = 0;
    hipEvent_t done = nullptr;
    bool used = false;
};

// the workspace of `device` in the caller's list `all` (by device index), at least `bytes` long, ordered behind its last user on `st`;
// call with the list's mutex held
inline int take_post_workspace(std::vector<PostWorkspace*>& all, const char* who, int device, size_t bytes, hipStream_t st,
                               PostWorkspace** out) {
    if ((size_t)device >= all.size()) all.resize((size_t)device + 1, nullptr);
    PostWorkspace*& w = all[(size_t)device];
    hipError_t e = hipSuccess;
    if (w == nullptr) {
        w = new PostWorkspace();
        e = hipEventCreateWithFlags(&w->done, hipEventDisableTiming);
        if (e != hipSuccess) {
            delete w; w = nullptr;
            return ape_fail(APE_ERR_HIP, "%s: hipEventCreate failed: %s", who, hipGetErrorString(e));
        }
    }
    if (w->cap < bytes) {
        if (w->used && (e = hipEventSynchronize(w->done)) != hipSuccess)
            return ape_fail(APE_ERR_HIP, "%s: hipEventSynchronize failed: %s", who, hipGetErrorString(e));
        if (w->dev) (void)hipFree(w->dev);
        w->dev = nullptr; w->cap = 0; w->used = false;
        if ((e = hipMalloc(&w->dev, bytes)) != hipSuccess) return ape_fail(APE_ERR_HIP, "%s: hipMalloc failed: %s", who, hipGetErrorString(e));
        w->cap = bytes;
    } else if (w->used) {
        if ((e = hipStreamWaitEvent(st, w->done, 0)) != hipSuccess)
            return ape_fail(APE_ERR_HIP, "%s: hipStreamWaitEvent failed: %s", who, hipGetErrorString(e));
    }
    *out = w;
    return APE_OK;
}

}  // namespace ape_postcommon
