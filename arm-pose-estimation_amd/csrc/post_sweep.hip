// Post-filter sweep (ape_post_sweep): the normalised targets y [F, M, O] of ONE replay re-smoothed at C configurations
// (smooth_c, m_c) in one pass -- for every c and frame the message (and spread record) ape_replay writes with smooth = smooth_c and
// m_c samples, stack row i = sample i % m_c of frame max(seg, f - smooth_c + 1 + i / m_c).  The reference has no counterpart beyond the
// per-frame arithmetic (estimator.py:108-118,122-137; compose_msg.py:13-108; transformations.py:32-51).
//
// ape_post_sweep_fk_kernel  the work the configurations share: sample rows k < Mx = max m_c of a chunk of frames -> est rows, once per
//                           call (its body, post_fk_rows, is in post_common.h: post_window.hip runs it too).  ape_fk3_kernel's decomposition (fk.hip: a row's three chains side by side, 32 rows per workgroup of two
//                           waves) and its statements, with the row index mapped: compact row r = frame r / Mx, sample r % Mx.
// ape_post_sweep_kernel     all C reductions of a tile of frames.  A lane takes (frame, configuration) pairs, the configurations in the
//                           order of falling stack height so that a wave's lanes run stacks of like length, frames fastest so that a
//                           wave's lanes read neighbouring frames.  LDS = true: the workgroup first copies the tile's est rows and the
//                           H = max smooth - 1 frames before them from the chunk into LDS (one contiguous run of the chunk, read once);
//                           every row is then read smooth_c times by each configuration from there.  The frame stride in LDS is odd
//                           (in float64 words), so lanes on neighbouring frames hit distinct banks of the 64-bit reads.  LDS = false
//                           (a tile with its halo does not fit, or C is so small that a tile would leave lanes idle): the rows come
//                           from the chunk in device memory, as ape_replay_msg_kernel's do.
// The chunk: est rows of `chunk` frames behind H carried-over frames, two buffers used in turn (ape_replay's ping-pong): the last H
// frames of a chunk are copied to the front of the other buffer.  Both sizes follow from the caller's byte bound alone.
//
// Order of the sums: ape_replay_msg_kernel's -- row 0 times 1/N first, every further row added with +-1/N by the strict `dot < 0.0` rule
// against row 0 (the dot as ape_msg_kernel's FMA chain), then one more in-order pass for the spread record.  The three quaternions share
// one pass over the rows here (each accumulator still sees its own additions in the same order: the same bits).  No atomics.
//
// float64 with separate roundings for a * b + c, like numpy (and replay.hip): contraction is off in this file.
#include "ape_internal.h"
#include "ape_model.h"
#include "../../include/ape_hip.h"
#include "stream_post_device.h"
#include "bank_host.h"

#include <algorithm>
#include <mutex>
#include <vector>

#pragma clang fp contract(off)
#include "score_device.h"
#include "post_common.h"

namespace {

using namespace ape_postdev;
using ape_scoredev::find_rec;
using namespace ape_postcommon;

constexpr int PS_BLOCK = 256;
constexpr int PS_LDS_WORDS = APE_LDS_BYTES / 8;         // float64 words of a CU's LDS
constexpr long long PS_DEFAULT_BYTES = 128ll << 20;

struct PsParams {
    const double* est;                                  // the chunk buffer: frame f_lo - H at est[0], Mx rows of W per frame
    const int* starts;                                  // [R]
    const double* bodies;                               // [R, 9] or nullptr
    double body[9];
    void* out;                                          // [C, F, out_stride]
    int F, R;
    int f_lo, f_hi;                                     // the chunk's frames
    int H, Mx, W, layout, C, TF, out_stride;
    int lds_fs;                                         // LDS: float64 words between frames (odd)
    short smooth[APE_POST_MAX_CONFIGS], m[APE_POST_MAX_CONFIGS];      // the configurations by falling smooth * m ...
    unsigned char idx[APE_POST_MAX_CONFIGS];                          // ... and their positions in the caller's list
};

__global__ __launch_bounds__(128) void ape_post_sweep_fk_kernel(const PostFkParams p) { post_fk_rows(p); }

// One (frame, configuration) pair: the stack of frame f at (smooth, M) -> 25 message values and, SPR, the 21 of its spread record.
// `fb` is the first row of frame `fbase` (fbase <= every frame the stack reaches), frames `fs` words apart, a frame's samples W apart.
template <typename TMsg, bool SPR>
__device__ __forceinline__ void sweep_pair(const double* fb, int fbase, int fs, int W, int layout, int f, int seg, int smooth, int M,
                                           const double* body, TMsg* dst, int out_stride) {
    const int N = smooth * M;
    auto frame_rows = [&](int j) -> const double* {
        int h = f - smooth + 1 + j;
        if (h < seg) h = seg;
        return fb + (long long)(h - fbase) * fs;
    };
    const bool hips = layout != APE_LAYOUT_ORI_CAL_LARM_UARM;
    const int nq = hips ? 3 : 2;
    const int qc[3] = {hips ? 9 : 6, hips ? 13 : 10, 17};
    const double* e0 = frame_rows(0);
    double out_q[3][4] = {}, orig_mean[9] = {};
    if (N > 1) {
        const bool pos = layout == APE_LAYOUT_ORI_POS_CAL_LARM_UARM_HIPS;
        const double wgt = 1.0 / (double)N;
        double r[3][4] = {}, a[3][4] = {};
#pragma unroll
        for (int q = 0; q < 3; ++q)
            if (q < nq) {
#pragma unroll
                for (int c = 0; c < 4; ++c) { r[q][c] = e0[qc[q] + c]; a[q][c] = r[q][c] * wgt; }
            }
        for (int j = 0; j < smooth; ++j) {
            const double* fr = frame_rows(j);
            for (int k = (j == 0 ? 1 : 0); k < M; ++k) {
                const double* e = fr + k * W;
#pragma unroll
                for (int q = 0; q < 3; ++q)
                    if (q < nq) {
                        const double* qi = e + qc[q];
                        // the FMA chain of ape_msg_kernel: numpy's dot hands the 4 products to BLAS ddot (fk.hip)
                        const double d = fma(qi[3], r[q][3], fma(qi[2], r[q][2], fma(qi[1], r[q][1], qi[0] * r[q][0])));
                        const double sg = d < 0.0 ? -wgt : wgt;
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
        if (pos) {                                      // compose_msg.py:26-29: plain means of the three origins, the rows in order
            for (int j = 0; j < smooth; ++j) {
                const double* fr = frame_rows(j);
                for (int k = 0; k < M; ++k) {
                    const double* e = fr + k * W;
#pragma unroll
                    for (int c = 0; c < 9; ++c) orig_mean[c] += e[c];
                }
            }
#pragma unroll
            for (int c = 0; c < 9; ++c) orig_mean[c] /= (double)N;
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
        for (int j = 0; j < smooth; ++j) {
            const double* fr = frame_rows(j);
            for (int k = 0; k < M; ++k) {
                const double* e = fr + k * W;
                spread_add_pos(pos, e); spread_add_pos(pos + 9, e + 3);
#pragma unroll
                for (int q = 0; q < 3; ++q)
                    if (q < nq) spread_add_quat(qq[q], e + qc[q]);
            }
        }
        double out[APE_SPREAD_WIDTH];
        spread_pos_out(pos, N, out); spread_pos_out(pos + 9, N, out + 9);
#pragma unroll
        for (int q = 0; q < 3; ++q) out[18 + q] = q < nq ? spread_angle_out(qq[q], N, m + 7 + 7 * q) : 0.0;
#pragma unroll
        for (int c = 0; c < APE_SPREAD_WIDTH; ++c) sd[c] = (TMsg)out[c];
    }
}

template <typename TMsg, bool SPR, bool LDS>
__global__ __launch_bounds__(PS_BLOCK) void ape_post_sweep_kernel(const PsParams p) {
    extern __shared__ __attribute__((aligned(16))) double tile[];
    const int t0 = p.f_lo + (int)blockIdx.x * p.TF;
    const int t1 = t0 + p.TF < p.f_hi ? t0 + p.TF : p.f_hi;
    const int nf = t1 - t0;
    const int MW = p.Mx * p.W;
    const double* fb = p.est;
    int fbase = p.f_lo - p.H, fs = MW;
    if constexpr (LDS) {
        // frames [max(t0 - H, 0), t1): one contiguous run of the chunk (no frame below 0 is ever part of a stack)
        const int hs = t0 - p.H > 0 ? t0 - p.H : 0;
        const double* src = p.est + (long long)(hs - (p.f_lo - p.H)) * MW;
        double* dst = tile + (hs - (t0 - p.H)) * p.lds_fs;
        const int total = (t1 - hs) * MW;
        for (int i = threadIdx.x; i < total; i += PS_BLOCK) {
            const int fr = i / MW, off = i - fr * MW;
            dst[fr * p.lds_fs + off] = src[i];
        }
        __syncthreads();
        fb = tile; fbase = t0 - p.H; fs = p.lds_fs;
    }
    const int pairs = nf * p.C;
    for (int pr = threadIdx.x; pr < pairs; pr += PS_BLOCK) {
        const int ci = pr / nf, f = t0 + (pr - ci * nf);
        const int rec = find_rec(p.starts, p.R, f);
        const int seg = p.starts[rec];
        const double* body = p.bodies != nullptr ? p.bodies + 9 * (size_t)rec : p.body;
        TMsg* dst = static_cast<TMsg*>(p.out) + ((size_t)p.idx[ci] * (size_t)p.F + (size_t)f) * (size_t)p.out_stride;
        sweep_pair<TMsg, SPR>(fb, fbase, fs, p.W, p.layout, f, seg, (int)p.smooth[ci], (int)p.m[ci], body, dst, p.out_stride);
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------
#define PS_TRY(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) return ape_fail(APE_ERR_HIP, "post_sweep: %s failed: %s", #expr, hipGetErrorString(_e)); } while (0)

// what follows from the arguments alone (include/ape_hip.h states the rule)
struct Plan {
    int W, S, Mx, H;
    long long frame_bytes;
    int chunk, passes;                                  // frames per pass, passes
    int TF, lds, lds_fs;                                // frames per tile; staged in LDS; LDS words between frames
};

int make_plan(int layout, int F, const int32_t* cfg, int C, long long bound, Plan* out) {
    Plan q{};
    q.W = layout == APE_LAYOUT_ORI_CAL_LARM_UARM ? 14 : 21;
    for (int c = 0; c < C; ++c) { q.S = std::max(q.S, (int)cfg[2 * c]); q.Mx = std::max(q.Mx, (int)cfg[2 * c + 1]); }
    q.H = q.S - 1;
    q.frame_bytes = 8ll * q.W * q.Mx;
    const long long fit = bound / (2 * q.frame_bytes) - q.H;
    if (fit < 1)
        return ape_fail(APE_ERR_INVALID_ARG, "post_sweep: workspace_bytes %lld holds no frame (at least %lld for these configurations)", bound,
                        2 * q.frame_bytes * (q.H + 1));
    q.chunk = (int)std::min<long long>(fit, F);
    q.passes = (F + q.chunk - 1) / q.chunk;
    q.lds_fs = (q.Mx * q.W) | 1;
    const int tf_fit = PS_LDS_WORDS / q.lds_fs - q.H;
    q.lds = tf_fit >= 1 && (long long)tf_fit * C >= PS_BLOCK;
    if (q.lds) q.TF = std::min(tf_fit, std::max((1024 + C - 1) / C, q.H + 1));   // enough pairs for every lane, a halo no longer than the tile
    else q.TF = std::max(1, PS_BLOCK / C);
    *out = q;
    return APE_OK;
}

// The workspace of a device (post_common.h): the two chunk buffers and the staged host arrays.
std::mutex g_mu;
std::vector<PostWorkspace*> g_ws;                          // by device index
thread_local int g_last[4] = {0, 0, 0, 0};

template <typename TMsg, bool SPR>
hipError_t launch_sweep(const PsParams& p, unsigned blocks, size_t lds_bytes, hipStream_t st) {
    if (lds_bytes > 0) {
        static hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(&ape_post_sweep_kernel<TMsg, SPR, true>),
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, APE_LDS_BYTES);
        if (attr != hipSuccess) return attr;
        hipLaunchKernelGGL((ape_post_sweep_kernel<TMsg, SPR, true>), dim3(blocks), dim3(PS_BLOCK), lds_bytes, st, p);
    } else {
        hipLaunchKernelGGL((ape_post_sweep_kernel<TMsg, SPR, false>), dim3(blocks), dim3(PS_BLOCK), 0, st, p);
    }
    return hipGetLastError();
}

}  // namespace

int ape_post_sweep_last(int32_t out4[4]) {
    if (!out4) return ape_fail(APE_ERR_INVALID_ARG, "post_sweep_last: NULL argument");
    for (int i = 0; i < 4; ++i) out4[i] = g_last[i];
    return APE_OK;
}

int ape_post_sweep(ape_model_t* m, const float* y_dev, int32_t F, int32_t n_mc, const int32_t* seg_starts_host, int32_t R,
                   const int32_t* configs_host, int32_t C, uint32_t flags, const double* bodies_host, int32_t n_bodies,
                   void* out_dev, int32_t out_dtype, int64_t workspace_bytes, void* stream) {
    // the arguments on their own first (no device needed to refuse them)
    if (!y_dev || !out_dev || !seg_starts_host || !configs_host) return ape_fail(APE_ERR_INVALID_ARG, "post_sweep: NULL argument");
    if (int rc = ape_check_segments("post_sweep", F, seg_starts_host, R)) return rc;
    if (n_mc < 1) return ape_fail(APE_ERR_INVALID_ARG, "post_sweep: n_mc=%d must be >= 1", n_mc);
    if ((long long)F * n_mc >= (1ll << 31)) return ape_fail(APE_ERR_UNSUPPORTED, "post_sweep: F*n_mc = %lld sample rows (< 2^31)", (long long)F * n_mc);
    if (C < 1 || C > APE_POST_MAX_CONFIGS) return ape_fail(APE_ERR_INVALID_ARG, "post_sweep: C=%d configurations (1 .. %d)", C, APE_POST_MAX_CONFIGS);
    for (int c = 0; c < C; ++c) {
        const int s = configs_host[2 * c], k = configs_host[2 * c + 1];
        if (s < 1 || s > 64) return ape_fail(APE_ERR_INVALID_ARG, "post_sweep: configuration %d: smooth %d outside 1..64", c, s);
        if (k < 1 || k > n_mc) return ape_fail(APE_ERR_INVALID_ARG, "post_sweep: configuration %d: %d samples outside 1..n_mc = %d", c, k, n_mc);
        if (s * k > 4096) return ape_fail(APE_ERR_INVALID_ARG, "post_sweep: configuration %d: smooth*samples = %d above 4096", c, s * k);
    }
    if ((bodies_host == nullptr) != (n_bodies == 0) || (n_bodies != 0 && n_bodies != 1 && n_bodies != R))
        return ape_fail(APE_ERR_INVALID_ARG, "post_sweep: n_bodies %d is neither 0 (NULL bodies), 1 nor R = %d", n_bodies, R);
    if (flags & ~(uint32_t)APE_FLAG_SPREAD) return ape_fail(APE_ERR_INVALID_ARG, "post_sweep: only the SPREAD flag is accepted");
    if (out_dtype != APE_F32 && out_dtype != APE_F64) return ape_fail(APE_ERR_INVALID_ARG, "post_sweep: unknown dtype selector");
    if (workspace_bytes < 0) return ape_fail(APE_ERR_INVALID_ARG, "post_sweep: workspace_bytes %lld is negative (0 = default)", (long long)workspace_bytes);
    if (!m) return ape_fail(ape_device_count() == 0 ? APE_ERR_NO_DEVICE : APE_ERR_INVALID_ARG,
                            "post_sweep: NULL model (no gfx950 device: there is no CPU fallback)");
    // ... then against the model
    const int layout = m->dims.target_layout;
    if (layout == APE_LAYOUT_NONE) return ape_fail(APE_ERR_INVALID_ARG, "post_sweep: model has no target layout");
    if (!m->has_stats) return ape_fail(APE_ERR_NOT_READY, "post_sweep: norm stats not set (y is normalised)");
    Plan q;
    if (int rc = make_plan(layout, F, configs_host, C, workspace_bytes > 0 ? (long long)workspace_bytes : PS_DEFAULT_BYTES, &q)) return rc;
    PS_TRY(hipSetDevice(m->dims.device));
    const hipStream_t st = (hipStream_t)stream;
    if (int rc = ape_check_not_capturing(st, "post_sweep", "host arrays are staged per call")) return rc;

    const bool spread = (flags & APE_FLAG_SPREAD) != 0;
    const bool table = n_bodies > 1;                    // (n_bodies == R == 1: one body for all, by value)
    const size_t buf_words = (size_t)(q.H + q.chunk) * q.Mx * q.W;
    const size_t bodies_bytes = table ? (size_t)R * 9 * sizeof(double) : 0;
    const size_t starts_bytes = (((size_t)R * sizeof(int)) + 7) & ~(size_t)7;
    const size_t total = 2 * buf_words * sizeof(double) + bodies_bytes + starts_bytes;

    std::lock_guard<std::mutex> lock(g_mu);
    PostWorkspace* ws = nullptr;
    if (int rc = take_post_workspace(g_ws, "post_sweep", m->dims.device, total, st, &ws)) return rc;
    double* est[2] = {static_cast<double*>(ws->dev), static_cast<double*>(ws->dev) + buf_words};
    double* bodies_d = reinterpret_cast<double*>(static_cast<char*>(ws->dev) + 2 * buf_words * sizeof(double));
    int* starts_d = reinterpret_cast<int*>(reinterpret_cast<char*>(bodies_d) + bodies_bytes);
    // (pageable host memory: the copies have read it when they return)
    hipError_t e = hipMemcpyAsync(starts_d, seg_starts_host, (size_t)R * sizeof(int), hipMemcpyHostToDevice, st);
    if (e == hipSuccess && table) e = hipMemcpyAsync(bodies_d, bodies_host, bodies_bytes, hipMemcpyHostToDevice, st);

    PostFkParams fk{};
    fk.y = y_dev;
    fk.yy_m = m->stats + 2 * m->dims.input_size;
    fk.yy_s = fk.yy_m + m->dims.output_size;
    fk.starts = starts_d; fk.bodies = table ? bodies_d : nullptr;
    memcpy(fk.body, bodies_host ? bodies_host : m->body, sizeof(fk.body));
    fk.R = R; fk.M = n_mc; fk.Mx = q.Mx; fk.O = m->dims.output_size; fk.W = q.W; fk.layout = layout;

    PsParams p{};
    p.starts = starts_d; p.bodies = fk.bodies;
    memcpy(p.body, fk.body, sizeof(p.body));
    p.out = out_dev; p.F = F; p.R = R;
    p.H = q.H; p.Mx = q.Mx; p.W = q.W; p.layout = layout; p.C = C; p.TF = q.TF; p.lds_fs = q.lds_fs;
    p.out_stride = 25 + (spread ? APE_SPREAD_WIDTH : 0);
    std::vector<int> order((size_t)C);
    for (int c = 0; c < C; ++c) order[(size_t)c] = c;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) {
        return configs_host[2 * a] * configs_host[2 * a + 1] > configs_host[2 * b] * configs_host[2 * b + 1];
    });
    for (int c = 0; c < C; ++c) {
        const int o = order[(size_t)c];
        p.smooth[c] = (short)configs_host[2 * o]; p.m[c] = (short)configs_host[2 * o + 1]; p.idx[c] = (unsigned char)o;
    }
    const size_t lds_bytes = q.lds ? (size_t)(q.TF + q.H) * q.lds_fs * sizeof(double) : 0;

    const size_t carry_words = (size_t)q.H * q.Mx * q.W;
    int prev_frames = 0;
    for (int f_lo = 0, c = 0; f_lo < F && e == hipSuccess; f_lo += q.chunk, ++c) {
        const int frames = std::min(q.chunk, F - f_lo);
        double* cur = est[c & 1];
        if (c > 0 && carry_words > 0)                   // the last H frames of the buffer just used: the frames before f_lo
            e = hipMemcpyAsync(cur, est[(c + 1) & 1] + (size_t)prev_frames * q.Mx * q.W, carry_words * sizeof(double), hipMemcpyDeviceToDevice, st);
        if (e != hipSuccess) break;
        fk.est = cur + carry_words; fk.rows = frames * q.Mx; fk.f_lo = f_lo;
        hipLaunchKernelGGL(ape_post_sweep_fk_kernel, dim3((unsigned)((fk.rows + POST_FK_ROWS - 1) / POST_FK_ROWS)), dim3(128), 0, st, fk);
        e = hipGetLastError();
        if (e != hipSuccess) break;
        p.est = cur; p.f_lo = f_lo; p.f_hi = f_lo + frames;
        const unsigned blocks = (unsigned)((frames + q.TF - 1) / q.TF);
        if (spread) e = out_dtype == APE_F32 ? launch_sweep<float, true>(p, blocks, lds_bytes, st) : launch_sweep<double, true>(p, blocks, lds_bytes, st);
        else e = out_dtype == APE_F32 ? launch_sweep<float, false>(p, blocks, lds_bytes, st) : launch_sweep<double, false>(p, blocks, lds_bytes, st);
        prev_frames = frames;
    }
    const hipError_t er = hipEventRecord(ws->done, st);    // the workspace is in flight whatever became of the launches
    ws->used = er == hipSuccess;
    if (e != hipSuccess) return ape_fail(APE_ERR_HIP, "post_sweep: launch failed: %s", hipGetErrorString(e));
    if (er != hipSuccess) {
        (void)hipStreamSynchronize(st);
        return ape_fail(APE_ERR_HIP, "post_sweep: hipEventRecord failed: %s", hipGetErrorString(er));
    }
    g_last[0] = q.passes; g_last[1] = q.chunk; g_last[2] = q.TF; g_last[3] = q.lds;
    return APE_OK;
}
