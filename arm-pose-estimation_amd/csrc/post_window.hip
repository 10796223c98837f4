// Windowed post-filter (ape_post_window): the normalised targets y [F, M, O] of ONE replay re-smoothed at C windows
// (back_c, ahead_c, m_c, weights_c) in one call -- stack row i = sample i % m_c of frame min(e - 1, max(s, f - back_c + i / m_c)) of the
// frame's recording [s, e).  A window that looks ahead as far as it looks back has no group delay; per-frame weights taper it.  The
// reference smooths over the past alone (estimator.py:112-118) and has no counterpart beyond the per-frame arithmetic
// (estimator.py:108-118,122-137; compose_msg.py:13-108; transformations.py:32-51).
//
// This file holds the one implementation of the post-filter pass over stored targets: the kernels, the plan and the host driver
// post_filter (declared in post_common.h).  ape_post_window below, ape_post_sweep (post_sweep.hip, DESIGN.md 4.33: configuration
// (smooth, m) is the uniform window (smooth - 1, 0, m)) and ape_post_select (post_select.hip, DESIGN.md 4.44: a window per frame from a
// ladder) are fronts that check their arguments and call it.
//
// ape_post_window_fk_kernel  the work the windows share (post_common.h): sample rows k < Mx = max m_c -> est rows, once per call.
// ape_post_window_kernel     all C reductions of a tile of frames.  A lane takes (frame, window) pairs, the
//                            windows in the order of falling stack height so that a wave's lanes run stacks of like length, frames fastest
//                            so that a wave's lanes read neighbouring frames.  LDS = true: the workgroup first copies the tile's est
//                            rows, the H = max back frames before and the A = max ahead frames after them (clipped to [0, F): one
//                            contiguous run of the chunk, read once) and the table of row weights into LDS; the frame stride there is
//                            odd (in float64 words), so lanes on neighbouring frames hit distinct banks of the 64-bit reads, and the
//                            lanes of a wave mostly share a window, so a weight is read as a broadcast.  LDS = false (a tile with
//                            its halos does not fit, or C is so small that a tile would leave lanes idle): rows and weights come from
//                            the workspace in device memory.  Same statements and same bits either way.
// ape_post_select_kernel     the selecting sibling (ape_post_select, post_select.hip): the windows are a ladder in the
//                            caller's order, a lane takes (frame, set) pairs and looks its window up in sel [S, F]; the same tile, the
//                            same pair function, so row (s, f) holds the bits the kernel above writes for window sel[s, f] at frame f.
//                            A selector value >= C fills its own row with NaN.  Any frame may pick any rung: the halos are the ladder's
//                            longest, and the lanes of a wave run stacks of whatever lengths the selector gives them.
// The chunk: est rows of H carried-over frames, `chunk` frames and A frames ahead, two buffers used in turn: the last H + A frames of a
// buffer are copied to the front of the other one, so a row is converted once per call.  Both sizes follow from the caller's byte bound.
//
// Order of the sums (uniform windows): ape_replay_msg_kernel's -- row 0 times 1/N first, every further row added with +-1/N by the
// strict `dot < 0.0` rule against row 0 (the dot as ape_msg_kernel's FMA chain), the origin means summed and then divided by N, then one
// more in-order pass for the spread record.  The three quaternions share one pass over the rows (each accumulator still sees its own
// additions in the same order: the same bits).  Tapered windows keep the order and the sign rule and put the row weight
// u_i = w_{i / m} / m where 1 / N stands.  A call whose windows are all uniform with ahead = 0 (every sweep) runs the SWEEP
// instantiations, which hold neither the tapered form nor the upper clamp of the frame index (it cannot act there: the same bits);
// profiles/post_window.md has the figures that decided it.
// No inline assembly, no read-modify-write on shared memory between lanes: every output value is one lane's own in-order sum.
//
// float64 with separate roundings for a * b + c, like numpy (and replay.hip): contraction is off in this file.
#include "ape_internal.h"
#include "ape_model.h"
#include "../../include/ape_hip.h"
#include "stream_post_device.h"
#include "bank_host.h"
#include "score_host.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <mutex>
#include <vector>

#pragma clang fp contract(off)
#include "score_device.h"
#include "post_common.h"

namespace {

using namespace ape_postdev;
using ape_scoredev::find_rec;
using namespace ape_postcommon;

constexpr int PW_BLOCK = 256;
constexpr int PW_LDS_WORDS = APE_LDS_BYTES / 8;         // float64 words of a CU's LDS
constexpr long long PW_DEFAULT_BYTES = 128ll << 20;
constexpr int NW = APE_POST_MAX_WINDOW;

struct PwParams {
    const double* est;                                  // the chunk buffer: frame f_lo - H at est[0], Mx rows of W per frame
    const int* starts;                                  // [R]
    const double* bodies;                               // [R, 9] or nullptr
    const double* wts;                                  // [C, NW] row weights u of the windows as ordered below; nullptr: every window is uniform
    double body[9];
    void* out;                                          // [C, F, out_stride]
    int F, R;
    int f_lo, f_hi;                                     // the chunk's frames
    int H, A, Mx, W, layout, C, TF, out_stride;
    int lds_fs;                                         // LDS: float64 words between frames (odd)
    short m[APE_POST_MAX_CONFIGS];                      // the windows by falling (back + ahead + 1) * m ...
    unsigned char back[APE_POST_MAX_CONFIGS], ahead[APE_POST_MAX_CONFIGS], tapered[APE_POST_MAX_CONFIGS];
    unsigned char idx[APE_POST_MAX_CONFIGS];            // ... and their positions in the caller's list
};

__global__ __launch_bounds__(128) void ape_post_window_fk_kernel(const PostFkParams p) { post_fk_rows(p); }

// the weighted sums of a tapered window's record: per origin sum u p and sum u (p_a p_b), per joint sum u (q_a q_b), in the layout of
// spread_add_pos / spread_add_quat
__device__ __forceinline__ void taper_add_pos(double* t, const double* v, double u) {
    t[0] += u * v[0]; t[1] += u * v[1]; t[2] += u * v[2];
    t[3] += u * (v[0] * v[0]); t[4] += u * (v[0] * v[1]); t[5] += u * (v[0] * v[2]);
    t[6] += u * (v[1] * v[1]); t[7] += u * (v[1] * v[2]); t[8] += u * (v[2] * v[2]);
}
__device__ __forceinline__ void taper_add_quat(double* t, const double* q, double u) {
    t[0] += u * (q[0] * q[0]); t[1] += u * (q[0] * q[1]); t[2] += u * (q[0] * q[2]); t[3] += u * (q[0] * q[3]);
    t[4] += u * (q[1] * q[1]); t[5] += u * (q[1] * q[2]); t[6] += u * (q[1] * q[3]);
    t[7] += u * (q[2] * q[2]); t[8] += u * (q[2] * q[3]); t[9] += u * (q[3] * q[3]);
}
// the weights sum to 1: the first sum is the mean, the second less the product of means the covariance
__device__ __forceinline__ void taper_pos_out(const double* t, double* o) {
    const double mx = t[0], my = t[1], mz = t[2];
    o[0] = mx; o[1] = my; o[2] = mz;
    o[3] = t[3] - mx * mx; o[4] = t[4] - mx * my; o[5] = t[5] - mx * mz;
    o[6] = t[6] - my * my; o[7] = t[7] - my * mz; o[8] = t[8] - mz * mz;
}
// 2 asin(sqrt(1 - qm^T (sum u q q^T) qm)); the clamp by comparisons, as spread_angle_out's
__device__ __forceinline__ double taper_angle_out(const double* t, const double* qm) {
    const double w = qm[0], x = qm[1], y = qm[2], z = qm[3];
    const double diag = t[0] * (w * w) + t[4] * (x * x) + t[7] * (y * y) + t[9] * (z * z);
    const double off = t[1] * (w * x) + t[2] * (w * y) + t[3] * (w * z) + t[5] * (x * y) + t[6] * (x * z) + t[8] * (y * z);
    double a = 1.0 - (diag + 2.0 * off);
    a = a < 0.0 ? 0.0 : (a > 1.0 ? 1.0 : a);
    return 2.0 * asin(sqrt(a));
}

// One (frame, window) pair: the stack of frame f of the recording [seg, end) at (back, n - back - 1, M) -> 25 message values and, SPR,
// the 21 of its spread record.  `fb` is the first row of frame `fbase` (fbase <= every frame the stack reaches), frames `fs` words
// apart, a frame's samples W apart.  TAP: `u` holds the n row weights of the window's frames; otherwise every row weighs 1 / N.
// CAUSAL: no window of the call looks ahead, so no frame index reaches `end` (which is then not read).  (Inlined into each of its
// call sites: out of line, `body` -- which may point into the kernel's parameters -- made every lane keep a private copy of PwParams,
// 560 bytes of scratch.)
template <typename TMsg, bool SPR, bool TAP, bool CAUSAL>
__device__ __forceinline__ void window_pair(const double* fb, int fbase, int fs, int W, int layout, int f, int seg, int end, int back, int n, int M,
                            const double* u, const double* body, TMsg* dst, int out_stride) {
    const int N = n * M;
    auto frame_rows = [&](int j) -> const double* {
        int h = f - back + j;
        if (h < seg) h = seg;
        if constexpr (!CAUSAL) {
            if (h > end - 1) h = end - 1;
        }
        return fb + (long long)(h - fbase) * fs;
    };
    const bool hips = layout != APE_LAYOUT_ORI_CAL_LARM_UARM;
    const int nq = hips ? 3 : 2;
    const int qc[3] = {hips ? 9 : 6, hips ? 13 : 10, 17};
    const double* e0 = frame_rows(0);
    double out_q[3][4] = {}, orig_mean[9] = {};
    if (N > 1) {
        const bool pos = layout == APE_LAYOUT_ORI_POS_CAL_LARM_UARM_HIPS;
        const double wgt = TAP ? u[0] : 1.0 / (double)N;
        double r[3][4] = {}, a[3][4] = {};
#pragma unroll
        for (int q = 0; q < 3; ++q)
            if (q < nq) {
#pragma unroll
                for (int c = 0; c < 4; ++c) { r[q][c] = e0[qc[q] + c]; a[q][c] = r[q][c] * wgt; }
            }
        for (int j = 0; j < n; ++j) {
            const double* fr = frame_rows(j);
            const double wj = TAP ? u[j] : wgt;
            for (int k = (j == 0 ? 1 : 0); k < M; ++k) {
                const double* e = fr + k * W;
#pragma unroll
                for (int q = 0; q < 3; ++q)
                    if (q < nq) {
                        const double* qi = e + qc[q];
                        // the FMA chain of ape_msg_kernel: numpy's dot hands the 4 products to BLAS ddot (fk.hip)
                        const double d = fma(qi[3], r[q][3], fma(qi[2], r[q][2], fma(qi[1], r[q][1], qi[0] * r[q][0])));
                        const double sg = d < 0.0 ? -wj : wj;
                        a[q][0] = a[q][0] + qi[0] * sg; a[q][1] = a[q][1] + qi[1] * sg;
                        a[q][2] = a[q][2] + qi[2] * sg; a[q][3] = a[q][3] + qi[3] * sg;
                    }
            }
        }
#pragma unroll
        for (int q = 0; q < 3; ++q)
            if (q < nq) {
                const double nrm = sqrt(a[q][0] * a[q][0] + a[q][1] * a[q][1] + a[q][2] * a[q][2] + a[q][3] * a[q][3]);
                out_q[q][0] = a[q][0] / nrm; out_q[q][1] = a[q][1] / nrm; out_q[q][2] = a[q][2] / nrm; out_q[q][3] = a[q][3] / nrm;
            }
        if (pos) {                                      // compose_msg.py:26-29: means of the three origins, the rows in order
            for (int j = 0; j < n; ++j) {
                const double* fr = frame_rows(j);
                for (int k = 0; k < M; ++k) {
                    const double* e = fr + k * W;
                    if constexpr (TAP) {
                        const double uj = u[j];
#pragma unroll
                        for (int c = 0; c < 9; ++c) orig_mean[c] += uj * e[c];
                    } else {
#pragma unroll
                        for (int c = 0; c < 9; ++c) orig_mean[c] += e[c];
                    }
                }
            }
            if constexpr (!TAP) {
#pragma unroll
                for (int c = 0; c < 9; ++c) orig_mean[c] /= (double)N;
            }
        }
    }
    double m[25];
    finish_msg(layout, N, out_q, orig_mean, e0, body, m);
#pragma unroll
    for (int c = 0; c < 25; ++c) dst[c] = (TMsg)m[c];
    if constexpr (SPR) {
        TMsg* sd = dst + (out_stride - APE_SPREAD_WIDTH);
        if (N == 1) {
#pragma unroll
            for (int c = 0; c < APE_SPREAD_WIDTH; ++c) sd[c] = (TMsg)spread_single(e0, c);
            return;
        }
        double pos[18] = {}, qq[3][10] = {};
        for (int j = 0; j < n; ++j) {
            const double* fr = frame_rows(j);
            for (int k = 0; k < M; ++k) {
                const double* e = fr + k * W;
                if constexpr (TAP) {
                    const double uj = u[j];
                    taper_add_pos(pos, e, uj); taper_add_pos(pos + 9, e + 3, uj);
#pragma unroll
                    for (int q = 0; q < 3; ++q)
                        if (q < nq) taper_add_quat(qq[q], e + qc[q], uj);
                } else {
                    spread_add_pos(pos, e); spread_add_pos(pos + 9, e + 3);
#pragma unroll
                    for (int q = 0; q < 3; ++q)
                        if (q < nq) spread_add_quat(qq[q], e + qc[q]);
                }
            }
        }
        double out[APE_SPREAD_WIDTH];
        if constexpr (TAP) {
            taper_pos_out(pos, out); taper_pos_out(pos + 9, out + 9);
#pragma unroll
            for (int q = 0; q < 3; ++q) out[18 + q] = q < nq ? taper_angle_out(qq[q], m + 7 + 7 * q) : 0.0;
        } else {
            spread_pos_out(pos, N, out); spread_pos_out(pos + 9, N, out + 9);
#pragma unroll
            for (int q = 0; q < 3; ++q) out[18 + q] = q < nq ? spread_angle_out(qq[q], N, m + 7 + 7 * q) : 0.0;
        }
#pragma unroll
        for (int c = 0; c < APE_SPREAD_WIDTH; ++c) sd[c] = (TMsg)out[c];
    }
}

// SWEEP: the host's choice for a call in which no window looks ahead and none is tapered (A = 0, wts = nullptr): the kernel a sweep runs
// where the lanes of a workgroup find the rows of the tile [t0, t1) and the weight table
struct TileRows {
    const double* fb;                                   // the first row of frame fbase
    const double* wt;
    int fbase, fs;                                      // float64 words between frames
};

// LDS: copies the tile's rows with their halos and the weight table into `tile` and waits for the workgroup; otherwise the chunk itself
template <bool LDS>
__device__ __forceinline__ TileRows tile_rows(const PwParams& p, int t0, int t1, double* tile) {
    const int MW = p.Mx * p.W;
    const double* fb = p.est;
    const double* wt = p.wts;
    int fbase = p.f_lo - p.H, fs = MW;
    if constexpr (LDS) {
        // frames [max(t0 - H, 0), min(t1 + A, F)): one contiguous run of the chunk (no frame outside [0, F) is ever part of a stack)
        const int hs = t0 - p.H > 0 ? t0 - p.H : 0;
        const int he = t1 + p.A < p.F ? t1 + p.A : p.F;
        const double* src = p.est + (long long)(hs - (p.f_lo - p.H)) * MW;
        double* dst = tile + (hs - (t0 - p.H)) * p.lds_fs;
        const int total = (he - hs) * MW;
        for (int i = threadIdx.x; i < total; i += PW_BLOCK) {
            const int fr = i / MW, off = i - fr * MW;
            dst[fr * p.lds_fs + off] = src[i];
        }
        if (p.wts != nullptr) {                          // the weight table next to the tile
            double* w = tile + (p.TF + p.H + p.A) * p.lds_fs;
            for (int i = threadIdx.x; i < p.C * NW; i += PW_BLOCK) w[i] = p.wts[i];
            wt = w;
        }
        __syncthreads();
        fb = tile; fbase = t0 - p.H; fs = p.lds_fs;
    }
    return TileRows{fb, wt, fbase, fs};
}

template <typename TMsg, bool SPR, bool LDS, bool SWEEP>
__global__ __launch_bounds__(PW_BLOCK) void ape_post_window_kernel(const PwParams p) {
    extern __shared__ __attribute__((aligned(16))) double tile[];
    const int t0 = p.f_lo + (int)blockIdx.x * p.TF;
    const int t1 = t0 + p.TF < p.f_hi ? t0 + p.TF : p.f_hi;
    const int nf = t1 - t0;
    const TileRows tr = tile_rows<LDS>(p, t0, t1, tile);
    const double* fb = tr.fb;
    const double* wt = tr.wt;
    const int fbase = tr.fbase, fs = tr.fs;
    const int pairs = nf * p.C;
    for (int pr = threadIdx.x; pr < pairs; pr += PW_BLOCK) {
        const int ci = pr / nf, f = t0 + (pr - ci * nf);
        const int rec = find_rec(p.starts, p.R, f);
        const int seg = p.starts[rec];
        const int end = SWEEP ? 0 : (rec + 1 < p.R ? p.starts[rec + 1] : p.F);
        const double* body = p.bodies != nullptr ? p.bodies + 9 * (size_t)rec : p.body;
        TMsg* dst = static_cast<TMsg*>(p.out) + ((size_t)p.idx[ci] * (size_t)p.F + (size_t)f) * (size_t)p.out_stride;
        const int back = (int)p.back[ci], n = back + (int)p.ahead[ci] + 1;
        if (!SWEEP && p.tapered[ci])
            window_pair<TMsg, SPR, true, false>(fb, fbase, fs, p.W, p.layout, f, seg, end, back, n, (int)p.m[ci], wt + ci * NW, body, dst, p.out_stride);
        else
            window_pair<TMsg, SPR, false, SWEEP>(fb, fbase, fs, p.W, p.layout, f, seg, end, back, n, (int)p.m[ci], nullptr, body, dst, p.out_stride);
    }
}

// The selecting form: p's windows are the ladder in the caller's order (p.idx is not read), sel [S, F] names the rung of every
// (set, frame), out [S, F, out_stride].  Sets slowest, frames fastest: a wave's lanes read neighbouring frames and neighbouring selector
// bytes.  The general form of the pair alone (two-sided clamp, tapered where the rung is): the bits ape_post_window_kernel writes.
template <typename TMsg, bool SPR, bool LDS>
__global__ __launch_bounds__(PW_BLOCK) void ape_post_select_kernel(const PwParams p, const unsigned char* sel, int S) {
    extern __shared__ __attribute__((aligned(16))) double tile[];
    const int t0 = p.f_lo + (int)blockIdx.x * p.TF;
    const int t1 = t0 + p.TF < p.f_hi ? t0 + p.TF : p.f_hi;
    const int nf = t1 - t0;
    const TileRows tr = tile_rows<LDS>(p, t0, t1, tile);
    const double* fb = tr.fb;
    const double* wt = tr.wt;
    const int fbase = tr.fbase, fs = tr.fs;
    const int pairs = nf * S;
    for (int pr = threadIdx.x; pr < pairs; pr += PW_BLOCK) {
        const int s = pr / nf, f = t0 + (pr - s * nf);
        const size_t at = (size_t)s * (size_t)p.F + (size_t)f;
        TMsg* dst = static_cast<TMsg*>(p.out) + at * (size_t)p.out_stride;
        const int ci = (int)sel[at];
        if (ci >= p.C) {                                // no such rung: the row says so, nothing else is touched
            for (int c = 0; c < p.out_stride; ++c) dst[c] = (TMsg)__builtin_nan("");
            continue;
        }
        const int rec = find_rec(p.starts, p.R, f);
        const int seg = p.starts[rec];
        const int end = rec + 1 < p.R ? p.starts[rec + 1] : p.F;
        const double* body = p.bodies != nullptr ? p.bodies + 9 * (size_t)rec : p.body;
        const int back = (int)p.back[ci], n = back + (int)p.ahead[ci] + 1;
        if (p.tapered[ci])
            window_pair<TMsg, SPR, true, false>(fb, fbase, fs, p.W, p.layout, f, seg, end, back, n, (int)p.m[ci], wt + ci * NW, body, dst, p.out_stride);
        else
            window_pair<TMsg, SPR, false, false>(fb, fbase, fs, p.W, p.layout, f, seg, end, back, n, (int)p.m[ci], nullptr, body, dst, p.out_stride);
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------
// what follows from the arguments alone (include/ape_hip.h states the rule)
struct Plan {
    int W, H, A, Mx;
    long long frame_bytes;
    int chunk, passes;                                  // frames per pass, passes
    int TF, lds, lds_fs, table_words;                   // frames per tile; staged in LDS; LDS words between frames; words of the weight table
};

// `lanes`: what a frame of a tile gives the workgroup's lanes to do -- the C windows, or the S sets of a selecting call
int make_plan(const char* who, const char* sets, int layout, int F, const int32_t* win, int C, int lanes, bool any_tapered, long long bound, Plan* out) {
    Plan q{};
    q.W = layout == APE_LAYOUT_ORI_CAL_LARM_UARM ? 14 : 21;
    for (int c = 0; c < C; ++c) {
        q.H = std::max(q.H, (int)win[3 * c]); q.A = std::max(q.A, (int)win[3 * c + 1]); q.Mx = std::max(q.Mx, (int)win[3 * c + 2]);
    }
    q.frame_bytes = 8ll * q.W * q.Mx;
    const long long fit = bound / (2 * q.frame_bytes) - q.H - q.A;
    if (fit < 1)
        return ape_fail(APE_ERR_INVALID_ARG, "%s: workspace_bytes %lld holds no frame (at least %lld for these %s)", who, bound,
                        2 * q.frame_bytes * (q.H + q.A + 1), sets);
    q.chunk = (int)std::min<long long>(fit, F);
    q.passes = (F + q.chunk - 1) / q.chunk;
    q.lds_fs = (q.Mx * q.W) | 1;
    q.table_words = any_tapered ? C * NW : 0;
    const int tf_fit = (PW_LDS_WORDS - q.table_words) / q.lds_fs - q.H - q.A;       // the tile is sized for the table beside it
    q.lds = tf_fit >= 1 && (long long)tf_fit * lanes >= PW_BLOCK;
    if (q.lds) q.TF = std::min(tf_fit, std::max((1024 + lanes - 1) / lanes, q.H + q.A + 1));   // enough pairs for every lane, halos no longer than the tile
    else q.TF = std::max(1, PW_BLOCK / lanes);
    *out = q;
    return APE_OK;
}

// The workspace of a device (post_common.h): one list and one mutex for every caller of post_filter.
std::mutex g_mu;
std::vector<PostWorkspace*> g_ws;                       // by device index
// The staging of a call (score_host.h): bodies, row weights and starts go through a pinned slot, so that they are consumed when the
// call returns and the one copy to the workspace neither waits for the stream nor reads the caller's memory later.  (A copy straight
// from pageable memory is staged by the runtime itself while the call is made, but only up to a size: measured, at once up to 295 KB,
// and at 1.44 MB -- the bodies of 20 000 recordings -- the call was held until the stream had reached the copy, behind everything
// queued before it; profiles/calls_in_flight.md.)  The slots have no device block: the device side is the workspace's tail.  Locked
// inside g_mu.
ApeSlotPool g_pool("post_filter");

template <typename TMsg, bool SPR, bool SWEEP>
hipError_t launch_window(const PwParams& p, unsigned blocks, size_t lds_bytes, hipStream_t st) {
    if (lds_bytes > 0) {
        static hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(&ape_post_window_kernel<TMsg, SPR, true, SWEEP>),
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, APE_LDS_BYTES);
        if (attr != hipSuccess) return attr;
        hipLaunchKernelGGL((ape_post_window_kernel<TMsg, SPR, true, SWEEP>), dim3(blocks), dim3(PW_BLOCK), lds_bytes, st, p);
    } else {
        hipLaunchKernelGGL((ape_post_window_kernel<TMsg, SPR, false, SWEEP>), dim3(blocks), dim3(PW_BLOCK), 0, st, p);
    }
    return hipGetLastError();
}

template <bool SWEEP>
hipError_t launch_window(bool spread, int out_dtype, const PwParams& p, unsigned blocks, size_t lds_bytes, hipStream_t st) {
    if (spread) return out_dtype == APE_F32 ? launch_window<float, true, SWEEP>(p, blocks, lds_bytes, st) : launch_window<double, true, SWEEP>(p, blocks, lds_bytes, st);
    return out_dtype == APE_F32 ? launch_window<float, false, SWEEP>(p, blocks, lds_bytes, st) : launch_window<double, false, SWEEP>(p, blocks, lds_bytes, st);
}

template <typename TMsg, bool SPR>
hipError_t launch_select(const PwParams& p, const unsigned char* sel, int S, unsigned blocks, size_t lds_bytes, hipStream_t st) {
    if (lds_bytes > 0) {
        static hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(&ape_post_select_kernel<TMsg, SPR, true>),
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, APE_LDS_BYTES);
        if (attr != hipSuccess) return attr;
        hipLaunchKernelGGL((ape_post_select_kernel<TMsg, SPR, true>), dim3(blocks), dim3(PW_BLOCK), lds_bytes, st, p, sel, S);
    } else {
        hipLaunchKernelGGL((ape_post_select_kernel<TMsg, SPR, false>), dim3(blocks), dim3(PW_BLOCK), 0, st, p, sel, S);
    }
    return hipGetLastError();
}

hipError_t launch_select(bool spread, int out_dtype, const PwParams& p, const unsigned char* sel, int S, unsigned blocks, size_t lds_bytes, hipStream_t st) {
    if (spread) return out_dtype == APE_F32 ? launch_select<float, true>(p, sel, S, blocks, lds_bytes, st) : launch_select<double, true>(p, sel, S, blocks, lds_bytes, st);
    return out_dtype == APE_F32 ? launch_select<float, false>(p, sel, S, blocks, lds_bytes, st) : launch_select<double, false>(p, sel, S, blocks, lds_bytes, st);
}

thread_local int g_last[4] = {0, 0, 0, 0};

}  // namespace

int ape_postcommon::post_filter(const char* who, const char* sets, ape_model_t* m, const float* y_dev, int F, int n_mc, const int32_t* seg_starts_host,
                                int R, const int32_t* windows_host, const double* weights_host, const bool* tapered, int C,
                                const unsigned char* sel_dev, int S, uint32_t flags, const double* bodies_host, int n_bodies, void* out_dev,
                                int out_dtype, long long workspace_bytes, void* stream, int last4[4]) {
    if (!m) return ape_fail(ape_device_count() == 0 ? APE_ERR_NO_DEVICE : APE_ERR_INVALID_ARG,
                            "%s: NULL model (no gfx950 device: there is no CPU fallback)", who);
    const int layout = m->dims.target_layout;
    if (layout == APE_LAYOUT_NONE) return ape_fail(APE_ERR_INVALID_ARG, "%s: model has no target layout", who);
    if (!m->has_stats) return ape_fail(APE_ERR_NOT_READY, "%s: norm stats not set (y is normalised)", who);
    bool any_tapered = false;
    for (int c = 0; c < C && tapered != nullptr; ++c) any_tapered = any_tapered || tapered[c];
    Plan q;
    if (int rc = make_plan(who, sets, layout, F, windows_host, C, sel_dev != nullptr ? S : C, any_tapered, workspace_bytes > 0 ? workspace_bytes : PW_DEFAULT_BYTES, &q)) return rc;
    hipError_t e = hipSetDevice(m->dims.device);
    if (e != hipSuccess) return ape_fail(APE_ERR_HIP, "%s: hipSetDevice failed: %s", who, hipGetErrorString(e));
    const hipStream_t st = (hipStream_t)stream;
    if (int rc = ape_check_not_capturing(st, who, "host arrays are staged per call")) return rc;

    const bool spread = (flags & APE_FLAG_SPREAD) != 0;
    const bool table = n_bodies > 1;                    // (n_bodies == R == 1: one body for all, by value)
    const size_t fw = (size_t)q.Mx * q.W;               // float64 words of a frame
    const size_t buf_words = (size_t)(q.H + q.chunk + q.A) * fw;
    const size_t bodies_bytes = table ? (size_t)R * 9 * sizeof(double) : 0;
    const size_t wts_bytes = (size_t)q.table_words * sizeof(double);
    const size_t starts_bytes = (((size_t)R * sizeof(int)) + 7) & ~(size_t)7;
    const size_t total = 2 * buf_words * sizeof(double) + bodies_bytes + wts_bytes + starts_bytes;

    PwParams p{};
    std::vector<int> order((size_t)C);
    for (int c = 0; c < C; ++c) order[(size_t)c] = c;
    auto height = [&](int c) { return (windows_host[3 * c] + windows_host[3 * c + 1] + 1) * windows_host[3 * c + 2]; };
    // (a ladder stays in the caller's order: the sort serves the grouping of lanes, which the selector decides there)
    if (sel_dev == nullptr) std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return height(a) > height(b); });
    for (int c = 0; c < C; ++c) {
        const int o = order[(size_t)c];
        p.back[c] = (unsigned char)windows_host[3 * o]; p.ahead[c] = (unsigned char)windows_host[3 * o + 1];
        p.m[c] = (short)windows_host[3 * o + 2]; p.idx[c] = (unsigned char)o; p.tapered[c] = any_tapered && tapered[o] ? 1 : 0;
    }

    std::lock_guard<std::mutex> lock(g_mu);
    PostWorkspace* ws = nullptr;
    if (int rc = take_post_workspace(g_ws, who, m->dims.device, total, st, &ws)) return rc;
    // the host arrays in the order of the workspace's tail: bodies, row weights, starts
    const size_t host_bytes = bodies_bytes + wts_bytes + (size_t)R * sizeof(int);
    std::lock_guard<std::mutex> pool_lock(g_pool.mu);
    ApeSlot* slot = nullptr;
    if (int rc = g_pool.take(m->dims.device, host_bytes, 0, &slot)) return rc;
    char* const pin = static_cast<char*>(slot->pinned);
    if (table) memcpy(pin, bodies_host, bodies_bytes);
    double* const wts = reinterpret_cast<double*>(pin + bodies_bytes);     // row weights u = w / m: one float64 division, here
    for (size_t i = 0; i < (size_t)q.table_words; ++i) wts[i] = 0.0;
    for (int c = 0; c < C; ++c)
        if (p.tapered[c])
            for (int j = 0; j <= (int)p.back[c] + (int)p.ahead[c]; ++j)
                wts[(size_t)c * NW + j] = weights_host[(size_t)p.idx[c] * NW + j] / (double)p.m[c];
    memcpy(pin + bodies_bytes + wts_bytes, seg_starts_host, (size_t)R * sizeof(int));
    double* est[2] = {static_cast<double*>(ws->dev), static_cast<double*>(ws->dev) + buf_words};
    double* bodies_d = reinterpret_cast<double*>(static_cast<char*>(ws->dev) + 2 * buf_words * sizeof(double));
    double* wts_d = reinterpret_cast<double*>(reinterpret_cast<char*>(bodies_d) + bodies_bytes);
    int* starts_d = reinterpret_cast<int*>(reinterpret_cast<char*>(wts_d) + wts_bytes);
    // (one copy from pinned memory; a copy that fails leaves through the records below like a launch that fails)
    e = hipMemcpyAsync(bodies_d, pin, host_bytes, hipMemcpyHostToDevice, st);

    PostFkParams fk{};
    fk.y = y_dev;
    fk.yy_m = m->stats + 2 * m->dims.input_size;
    fk.yy_s = fk.yy_m + m->dims.output_size;
    fk.starts = starts_d; fk.bodies = table ? bodies_d : nullptr;
    memcpy(fk.body, bodies_host ? bodies_host : m->body, sizeof(fk.body));
    fk.R = R; fk.M = n_mc; fk.Mx = q.Mx; fk.O = m->dims.output_size; fk.W = q.W; fk.layout = layout;

    p.starts = starts_d; p.bodies = fk.bodies; p.wts = any_tapered ? wts_d : nullptr;
    memcpy(p.body, fk.body, sizeof(p.body));
    p.out = out_dev; p.F = F; p.R = R;
    p.H = q.H; p.A = q.A; p.Mx = q.Mx; p.W = q.W; p.layout = layout; p.C = C; p.TF = q.TF; p.lds_fs = q.lds_fs;
    p.out_stride = 25 + (spread ? APE_SPREAD_WIDTH : 0);
    const size_t lds_bytes = q.lds ? ((size_t)(q.TF + q.H + q.A) * q.lds_fs + q.table_words) * sizeof(double) : 0;
    const bool sweep = q.A == 0 && !any_tapered;        // every sweep: the instantiations without the upper clamp and the tapered form

    const size_t carry_words = (size_t)(q.H + q.A) * fw;
    int prev_frames = 0;
    for (int f_lo = 0, c = 0; f_lo < F && e == hipSuccess; f_lo += q.chunk, ++c) {
        const int frames = std::min(q.chunk, F - f_lo);
        double* cur = est[c & 1];
        // the buffer holds frames [f_lo - H, f_lo + frames + A).  Its first H + A are the last H + A of the buffer just used ...
        if (c > 0 && carry_words > 0)
            e = hipMemcpyAsync(cur, est[(c + 1) & 1] + (size_t)prev_frames * fw, carry_words * sizeof(double), hipMemcpyDeviceToDevice, st);
        if (e != hipSuccess) break;
        // ... the rest is converted now, as far as the recordings go
        const int fresh_lo = c == 0 ? 0 : std::min(F, f_lo + q.A), fresh_hi = std::min(F, f_lo + frames + q.A);
        if (fresh_hi > fresh_lo) {
            fk.est = cur + (size_t)(fresh_lo - (f_lo - q.H)) * fw; fk.rows = (fresh_hi - fresh_lo) * q.Mx; fk.f_lo = fresh_lo;
            hipLaunchKernelGGL(ape_post_window_fk_kernel, dim3((unsigned)((fk.rows + POST_FK_ROWS - 1) / POST_FK_ROWS)), dim3(128), 0, st, fk);
            e = hipGetLastError();
            if (e != hipSuccess) break;
        }
        p.est = cur; p.f_lo = f_lo; p.f_hi = f_lo + frames;
        const unsigned blocks = (unsigned)((frames + q.TF - 1) / q.TF);
        if (sel_dev != nullptr) e = launch_select(spread, out_dtype, p, sel_dev, S, blocks, lds_bytes, st);
        else e = sweep ? launch_window<true>(spread, out_dtype, p, blocks, lds_bytes, st) : launch_window<false>(spread, out_dtype, p, blocks, lds_bytes, st);
        prev_frames = frames;
    }
    const hipError_t er = hipEventRecord(ws->done, st);    // the workspace is in flight whatever became of the launches
    ws->used = er == hipSuccess;
    if (int rc = g_pool.finish(who, slot, e, st)) return rc;      // the slot's event behind the same launches; a failed launch is reported here
    if (er != hipSuccess) {
        (void)hipStreamSynchronize(st);
        return ape_fail(APE_ERR_HIP, "%s: hipEventRecord failed: %s", who, hipGetErrorString(er));
    }
    last4[0] = q.passes; last4[1] = q.chunk; last4[2] = q.TF; last4[3] = q.lds;
    return APE_OK;
}

int ape_postcommon::post_window_args(const char* who, const void* y_dev, const void* out_dev, int F, int n_mc, const int32_t* seg_starts_host,
                                     int R, const int32_t* windows_host, const double* weights_host, int C, uint32_t flags,
                                     const double* bodies_host, int n_bodies, int out_dtype, long long workspace_bytes, bool* tapered) {
    if (!y_dev || !out_dev || !seg_starts_host || !windows_host) return ape_fail(APE_ERR_INVALID_ARG, "%s: NULL argument", who);
    if (int rc = ape_check_segments(who, F, seg_starts_host, R)) return rc;
    if (n_mc < 1) return ape_fail(APE_ERR_INVALID_ARG, "%s: n_mc=%d must be >= 1", who, n_mc);
    if ((long long)F * n_mc >= (1ll << 31)) return ape_fail(APE_ERR_UNSUPPORTED, "%s: F*n_mc = %lld sample rows (< 2^31)", who, (long long)F * n_mc);
    if (C < 1 || C > APE_POST_MAX_CONFIGS) return ape_fail(APE_ERR_INVALID_ARG, "%s: C=%d windows (1 .. %d)", who, C, APE_POST_MAX_CONFIGS);
    for (int c = 0; c < C; ++c) {
        const int b = windows_host[3 * c], a = windows_host[3 * c + 1], k = windows_host[3 * c + 2];
        if (b < 0) return ape_fail(APE_ERR_INVALID_ARG, "%s: window %d: back %d is negative", who, c, b);
        if (a < 0) return ape_fail(APE_ERR_INVALID_ARG, "%s: window %d: ahead %d is negative", who, c, a);
        const long long n = (long long)b + a + 1;
        if (n > NW) return ape_fail(APE_ERR_INVALID_ARG, "%s: window %d: back + ahead + 1 = %lld frames above %d", who, c, n, NW);
        if (k < 1 || k > n_mc) return ape_fail(APE_ERR_INVALID_ARG, "%s: window %d: %d samples outside 1..n_mc = %d", who, c, k, n_mc);
        if (n * k > 4096) return ape_fail(APE_ERR_INVALID_ARG, "%s: window %d: frames*samples = %lld above 4096", who, c, n * k);
        if (weights_host != nullptr) {
            const double* w = weights_host + (size_t)c * NW;
            double sum = 0.0;
            for (int j = 0; j < (int)n; ++j) {
                if (!std::isfinite(w[j]) || w[j] < 0.0)
                    return ape_fail(APE_ERR_INVALID_ARG, "%s: window %d: weight %d = %g is not a finite value >= 0", who, c, j, w[j]);
                sum += w[j];
                if (memcmp(&w[j], &w[0], sizeof(double)) != 0) tapered[c] = true;      // uniform: all n entries bit-equal
            }
            if (!(std::fabs(sum - 1.0) <= 1e-9))
                return ape_fail(APE_ERR_INVALID_ARG, "%s: window %d: weights sum to %.17g, not to 1 within 1e-9 (the library does not normalise)", who, c, sum);
        }
    }
    if ((bodies_host == nullptr) != (n_bodies == 0) || (n_bodies != 0 && n_bodies != 1 && n_bodies != R))
        return ape_fail(APE_ERR_INVALID_ARG, "%s: n_bodies %d is neither 0 (NULL bodies), 1 nor R = %d", who, n_bodies, R);
    if (flags & ~(uint32_t)APE_FLAG_SPREAD) return ape_fail(APE_ERR_INVALID_ARG, "%s: only the SPREAD flag is accepted", who);
    if (out_dtype != APE_F32 && out_dtype != APE_F64) return ape_fail(APE_ERR_INVALID_ARG, "%s: unknown dtype selector", who);
    if (workspace_bytes < 0) return ape_fail(APE_ERR_INVALID_ARG, "%s: workspace_bytes %lld is negative (0 = default)", who, (long long)workspace_bytes);
    return APE_OK;
}

int ape_post_window_last(int32_t out4[4]) {
    if (!out4) return ape_fail(APE_ERR_INVALID_ARG, "post_window_last: NULL argument");
    for (int i = 0; i < 4; ++i) out4[i] = g_last[i];
    return APE_OK;
}

int ape_post_window(ape_model_t* m, const float* y_dev, int32_t F, int32_t n_mc, const int32_t* seg_starts_host, int32_t R,
                    const int32_t* windows_host, const double* weights_host, int32_t C, uint32_t flags, const double* bodies_host,
                    int32_t n_bodies, void* out_dev, int32_t out_dtype, int64_t workspace_bytes, void* stream) {
    // the arguments on their own (no device needed to refuse them); post_filter checks them against the model
    bool tapered[APE_POST_MAX_CONFIGS] = {};
    if (int rc = post_window_args("post_window", y_dev, out_dev, F, n_mc, seg_starts_host, R, windows_host, weights_host, C, flags, bodies_host,
                                  n_bodies, out_dtype, workspace_bytes, tapered)) return rc;
    return post_filter("post_window", "windows", m, y_dev, F, n_mc, seg_starts_host, R, windows_host, weights_host, tapered, C, nullptr, 0, flags,
                       bodies_host, n_bodies, out_dev, out_dtype, workspace_bytes, stream, g_last);
}
