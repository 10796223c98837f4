// Offline replay (ape_replay): the kernels a whole recording needs beyond the per-frame ones --
//
// ape_replay_seg_kernel     frame -> first frame of its recording (the cold-start boundary), once per call
// ape_replay_window_kernel  the windows of a chunk of sample rows, [R][T][I], every row's window assembled by the clamped-index rule of
//                           Estimator._push_padded (estimator.py:96-100): window row t of frame f is feature row max(seg, f - T + 1 + t);
//                           sample row r is sample r % n_mc of frame r / n_mc, so a frame's n_mc windows are copies
// ape_replay_msg_kernel     the sliding smoothing stack of every frame whose rows are complete (estimator.py:112-118) reduced to its message
//                           (compose_msg.py:13-108): stack row i = sample i % n_mc of frame max(seg, f - smooth + 1 + i / n_mc)
// ape_replay_tail_kernel    the hand / elbow xyz of every stacked row behind the message (estimator.py:131-137)
//
// float64 with separate roundings for a * b + c, like numpy (and the bank's post-filter): contraction is off in this file.
#include "ape_internal.h"
#include "../../include/ape_hip.h"
#include "stream_post_device.h"

#pragma clang fp contract(off)

namespace {

using namespace ape_postdev;

// first frame of the recording frame f belongs to: the last start <= f (starts[0] == 0, strictly rising)
__global__ __launch_bounds__(256) void ape_replay_seg_kernel(const int* __restrict__ starts, int n_starts, int F, int* __restrict__ seg_of) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    int lo = 0, hi = n_starts - 1;                      // invariant: starts[lo] <= f
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (starts[mid] <= f) lo = mid; else hi = mid - 1;
    }
    seg_of[f] = starts[lo];
}

// the same search for the recording's index: the replays with one body per recording (ape_replay_bodies) read row
// rec_of[f] of their [R,9] table
__global__ __launch_bounds__(256) void ape_replay_rec_kernel(const int* __restrict__ starts, int n_starts, int F, int* __restrict__ rec_of) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    int lo = 0, hi = n_starts - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (starts[mid] <= f) lo = mid; else hi = mid - 1;
    }
    rec_of[f] = lo;
}

// one thread per output float: consecutive threads write consecutive floats and read the same feature row's columns
// CARRY (ape_replay_resume): a row before the recording's first frame is the matching row of the record the recording came in with,
// counted back from its newest; a recording whose window bit is clear is clamped as without carry
template <bool CARRY = false>
__global__ __launch_bounds__(256) void ape_replay_window_kernel(const ReplayWindowParams p, const ReplayCarryParams c) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long per_row = (long long)p.T * p.I;
    if (idx >= (long long)p.R * per_row) return;
    const long long r = p.r0 + idx / per_row;
    const int rem = (int)(idx % per_row);
    const int t = rem / p.I, i = rem - t * p.I;
    const int f = (int)(r / p.n_mc);
    const int seg = p.seg_of[f];
    int src = f - p.T + 1 + t;
    if constexpr (CARRY) {
        if (src < seg) {
            const int rec = c.rec_of[f];
            if (c.warm[rec] & APE_STATE_WINDOW_WARM) {
                p.xw[idx] = c.state_in[(size_t)rec * c.words + (size_t)(p.T + src - seg) * p.I + i];
                return;
            }
        }
    }
    if (src < seg) src = seg;
    p.xw[idx] = p.xx[(size_t)src * p.I + i];
}

// One lane per frame, the stack's rows in the reference's order (average_quaternions, transformations.py:32-51: row 0 times 1/N, then
// every further row added with +-1/N by the strict `dot < 0.0` rule against row 0).  Adjacent frames share all but n_mc of their rows:
// the est rows come from L2.
// TAB: the frame's body is row rec_of[f] of bodies [R,9] (neighbouring lanes mostly share it), else the uniform p.body
// CARRY (ape_replay_resume): a stack row before the recording's first frame is the matching est row of the stack the recording came in
// with (c.est_in, counted back from its newest); a recording whose stack bit is clear is clamped as without carry
// SPR (APE_FLAG_SPREAD): the frame's spread record (include/ape_hip.h, APE_SPREAD_WIDTH) in the last columns of its row, fused here
// rather than a kernel of its own: the lane holds the message's float64 quaternions and the row accessor (CARRY included).  One more
// pass over row(0 .. N-1) in order, so a recording replayed in pieces gives the bits of the one call.
template <typename TMsg, bool TAB = false, bool CARRY = false, bool SPR = false>
__global__ __launch_bounds__(256) void ape_replay_msg_kernel(const ReplayMsgParams p, const double* __restrict__ bodies,
                                                             const int* __restrict__ rec_of, const ReplayCarryParams c) {
    const long long f = p.f_lo + (long long)blockIdx.x * 256 + threadIdx.x;
    if (f >= p.f_hi) return;
    const int M = p.n_mc, N = p.smooth * M, W = p.W;
    const long long seg = p.seg_of[f];
    int crec = -1;                                      // CARRY: the frame's recording where it came in with a warm stack
    if constexpr (CARRY) {
        const int rec = c.rec_of[f];
        if (c.warm[rec] & APE_STATE_STACK_WARM) crec = rec;
    }
    auto row = [&](int i) -> const double* {
        const int j = i / M, k = i - j * M;
        long long h = f - p.smooth + 1 + j;
        if constexpr (CARRY) {
            if (h < seg && crec >= 0) return c.est_in + (((size_t)crec * p.smooth + (size_t)(p.smooth + h - seg)) * M + k) * W;
        }
        if (h < seg) h = seg;
        return p.est + (h * M + k - p.est_base) * W;
    };
    const double* e0 = row(0);
    double out_q[3][4] = {}, orig_mean[9] = {};
    if (N > 1) {
        const bool hips = p.layout != APE_LAYOUT_ORI_CAL_LARM_UARM;
        const int nq = hips ? 3 : 2;
        const int qc[3] = {hips ? 9 : 6, hips ? 13 : 10, 17};
        const double wgt = 1.0 / (double)N;
        for (int q = 0; q < nq; ++q) {
            const double r0 = e0[qc[q]], r1 = e0[qc[q] + 1], r2 = e0[qc[q] + 2], r3 = e0[qc[q] + 3];
            double a0 = r0 * wgt, a1 = r1 * wgt, a2 = r2 * wgt, a3 = r3 * wgt;
            for (int i = 1; i < N; ++i) {
                const double* qi = row(i) + qc[q];
                // the FMA chain of ape_msg_kernel: numpy's dot hands the 4 products to BLAS ddot (fk.hip)
                const double d = fma(qi[3], r3, fma(qi[2], r2, fma(qi[1], r1, qi[0] * r0)));
                const double sg = d < 0.0 ? -wgt : wgt;
                a0 = a0 + qi[0] * sg; a1 = a1 + qi[1] * sg; a2 = a2 + qi[2] * sg; a3 = a3 + qi[3] * sg;
            }
            const double nrm = sqrt(a0 * a0 + a1 * a1 + a2 * a2 + a3 * a3);
            out_q[q][0] = a0 / nrm; out_q[q][1] = a1 / nrm; out_q[q][2] = a2 / nrm; out_q[q][3] = a3 / nrm;
        }
        if (p.layout == APE_LAYOUT_ORI_POS_CAL_LARM_UARM_HIPS) {       // compose_msg.py:26-29: plain means of the three origins
            for (int i = 0; i < N; ++i) {
                const double* e = row(i);
#pragma unroll
                for (int c = 0; c < 9; ++c) orig_mean[c] += e[c];
            }
#pragma unroll
            for (int c = 0; c < 9; ++c) orig_mean[c] /= (double)N;
        }
    }
    double m[25];
    finish_msg(p.layout, N, out_q, orig_mean, e0, TAB ? bodies + 9 * (size_t)rec_of[f] : p.body, m);
    TMsg* dst = static_cast<TMsg*>(p.out) + f * p.out_stride;
#pragma unroll
    for (int c = 0; c < 25; ++c) dst[c] = (TMsg)m[c];
    if constexpr (SPR) {
        TMsg* sd = dst + (p.out_stride - APE_SPREAD_WIDTH);
        if (N == 1) {
#pragma unroll
            for (int c = 0; c < APE_SPREAD_WIDTH; ++c) sd[c] = (TMsg)spread_single(e0, c);
            return;
        }
        const bool hips = p.layout != APE_LAYOUT_ORI_CAL_LARM_UARM;
        const int nq = hips ? 3 : 2;
        const int qc[3] = {hips ? 9 : 6, hips ? 13 : 10, 17};
        double pos[18] = {}, qq[3][10] = {};
        for (int i = 0; i < N; ++i) {
            const double* e = row(i);
            spread_add_pos(pos, e); spread_add_pos(pos + 9, e + 3);
#pragma unroll
            for (int k = 0; k < 3; ++k)
                if (k < nq) spread_add_quat(qq[k], e + qc[k]);
        }
        double out[APE_SPREAD_WIDTH];
        spread_pos_out(pos, N, out); spread_pos_out(pos + 9, N, out + 9);
#pragma unroll
        for (int k = 0; k < 3; ++k) out[18 + k] = k < nq ? spread_angle_out(qq[k], N, m + 7 + 7 * k) : 0.0;
#pragma unroll
        for (int c = 0; c < APE_SPREAD_WIDTH; ++c) sd[c] = (TMsg)out[c];
    }
}


// one thread per (frame, stacked row): six values each, neighbouring threads write neighbouring groups
template <typename TMsg, bool CARRY = false>
__global__ __launch_bounds__(256) void ape_replay_tail_kernel(const ReplayMsgParams p, const ReplayCarryParams c) {
    const int M = p.n_mc, N = p.smooth * M;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (p.f_hi - p.f_lo) * N) return;
    const long long f = p.f_lo + idx / N;
    const int i = (int)(idx % N);
    const int j = i / M, k = i - j * M;
    long long h = f - p.smooth + 1 + j;
    const long long seg = p.seg_of[f];
    const double* e = nullptr;
    if constexpr (CARRY) {
        if (h < seg) {
            const int rec = c.rec_of[f];
            if (c.warm[rec] & APE_STATE_STACK_WARM) e = c.est_in + (((size_t)rec * p.smooth + (size_t)(p.smooth + h - seg)) * M + k) * p.W;
        }
    }
    if (h < seg) h = seg;
    if (e == nullptr) e = p.est + (h * M + k - p.est_base) * p.W;
    TMsg* dst = static_cast<TMsg*>(p.out) + f * p.out_stride + 25 + (long long)i * 6;
#pragma unroll
    for (int c = 0; c < 6; ++c) dst[c] = (TMsg)e[c];
}

// the stacks of R canonical records, [smooth][n_mc][O] behind each record's window words -> contiguous rows for the carried rows' FK launch
__global__ __launch_bounds__(256) void ape_replay_carry_rows_kernel(const float* __restrict__ state_in, int R, int words, int x_words,
                                                                    int stack_words, float* __restrict__ y_in) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)R * stack_words) return;
    const int r = (int)(idx / stack_words), w = (int)(idx - (long long)r * stack_words);
    y_in[idx] = state_in[(size_t)r * words + x_words + w];
}

// the recordings' final windows and stacks in the canonical form of the banks: one thread per word; a row before the recording's first
// frame comes from the record it came in with, or -- cold -- is the clamped first frame, exactly what the kernels above read
__global__ __launch_bounds__(256) void ape_replay_state_out_kernel(const ReplayStateOutParams p) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)p.R * p.words) return;
    const int r = (int)(idx / p.words), w = (int)(idx - (long long)r * p.words);
    const int seg = p.starts[r], e = (r + 1 < p.R ? p.starts[r + 1] : p.F) - 1;
    const int nx = p.T * p.I, MO = p.n_mc * p.O;
    const int warm = p.warm != nullptr ? p.warm[r] : 0;
    const float* in = p.state_in != nullptr ? p.state_in + (size_t)r * p.words : nullptr;
    float v = 0.0f;
    if (w < nx) {
        const int t = w / p.I, i = w - t * p.I;
        const int src = e - p.T + 1 + t;
        if (src >= seg) v = p.xx[(size_t)src * p.I + i];
        else if (warm & APE_STATE_WINDOW_WARM) v = in[(size_t)(p.T + src - seg) * p.I + i];
        else v = p.xx[(size_t)seg * p.I + i];
    } else if (w < nx + p.smooth * MO) {
        const int q = w - nx, j = q / MO, ko = q - j * MO;
        const int h = e - p.smooth + 1 + j;
        if (h >= seg) v = p.y[(size_t)h * MO + ko];
        else if ((warm & APE_STATE_STACK_WARM) && (warm & APE_STATE_WINDOW_WARM)) v = in[nx + (size_t)(p.smooth + h - seg) * MO + ko];
        else v = p.y[(size_t)seg * MO + ko];
    }
    p.state_out[idx] = v;
}

unsigned blocks_for(long long n) { return (unsigned)((n + 255) / 256); }

}  // namespace

hipError_t ape_launch_replay_carry_rows(const float* state_in, int R, int words, int x_words, int stack_words, float* y_in, hipStream_t stream) {
    hipLaunchKernelGGL(ape_replay_carry_rows_kernel, dim3(blocks_for((long long)R * stack_words)), dim3(256), 0, stream, state_in, R, words,
                       x_words, stack_words, y_in);
    return hipGetLastError();
}

hipError_t ape_launch_replay_state_out(const ReplayStateOutParams& p, hipStream_t stream) {
    hipLaunchKernelGGL(ape_replay_state_out_kernel, dim3(blocks_for((long long)p.R * p.words)), dim3(256), 0, stream, p);
    return hipGetLastError();
}

hipError_t ape_launch_replay_segments(const int* starts, int n_starts, int F, int* seg_of, hipStream_t stream, int* rec_of) {
    hipLaunchKernelGGL(ape_replay_seg_kernel, dim3(blocks_for(F)), dim3(256), 0, stream, starts, n_starts, F, seg_of);
    if (rec_of != nullptr) hipLaunchKernelGGL(ape_replay_rec_kernel, dim3(blocks_for(F)), dim3(256), 0, stream, starts, n_starts, F, rec_of);
    return hipGetLastError();
}

hipError_t ape_launch_replay_windows(const ReplayWindowParams& p, hipStream_t stream, const ReplayCarryParams* carry) {
    const dim3 grid(blocks_for((long long)p.R * p.T * p.I));
    if (carry != nullptr) hipLaunchKernelGGL(ape_replay_window_kernel<true>, grid, dim3(256), 0, stream, p, *carry);
    else hipLaunchKernelGGL(ape_replay_window_kernel<false>, grid, dim3(256), 0, stream, p, ReplayCarryParams{});
    return hipGetLastError();
}

// one instantiation per (dtype, per-recording bodies, carry, spread)
template <typename TMsg, bool SPR>
static void launch_replay_msg_typed(const ReplayMsgParams& p, unsigned blocks, hipStream_t stream, const double* bodies, const int* rec_of,
                                    const ReplayCarryParams* carry) {
    const ReplayCarryParams none{};
    if (carry != nullptr) {
        if (bodies != nullptr) hipLaunchKernelGGL((ape_replay_msg_kernel<TMsg, true, true, SPR>), dim3(blocks), dim3(256), 0, stream, p, bodies, rec_of, *carry);
        else hipLaunchKernelGGL((ape_replay_msg_kernel<TMsg, false, true, SPR>), dim3(blocks), dim3(256), 0, stream, p, bodies, rec_of, *carry);
    } else if (bodies != nullptr) hipLaunchKernelGGL((ape_replay_msg_kernel<TMsg, true, false, SPR>), dim3(blocks), dim3(256), 0, stream, p, bodies, rec_of, none);
    else hipLaunchKernelGGL((ape_replay_msg_kernel<TMsg, false, false, SPR>), dim3(blocks), dim3(256), 0, stream, p, bodies, rec_of, none);
}

hipError_t ape_launch_replay_msg(const ReplayMsgParams& p, bool tail, hipStream_t stream, const double* bodies, const int* rec_of,
                                 const ReplayCarryParams* carry, bool spread) {
    const long long frames = p.f_hi - p.f_lo;
    if (frames <= 0) return hipSuccess;
    if (spread) {                                      // (p.out_stride counts the record's columns: they are the row's last)
        if (p.out_dtype == APE_F32) launch_replay_msg_typed<float, true>(p, blocks_for(frames), stream, bodies, rec_of, carry);
        else launch_replay_msg_typed<double, true>(p, blocks_for(frames), stream, bodies, rec_of, carry);
    } else if (p.out_dtype == APE_F32) launch_replay_msg_typed<float, false>(p, blocks_for(frames), stream, bodies, rec_of, carry);
    else launch_replay_msg_typed<double, false>(p, blocks_for(frames), stream, bodies, rec_of, carry);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !tail) return e;
    const long long n = frames * p.smooth * p.n_mc;
    const ReplayCarryParams none{};
    if (carry != nullptr) {
        if (p.out_dtype == APE_F32) hipLaunchKernelGGL((ape_replay_tail_kernel<float, true>), dim3(blocks_for(n)), dim3(256), 0, stream, p, *carry);
        else hipLaunchKernelGGL((ape_replay_tail_kernel<double, true>), dim3(blocks_for(n)), dim3(256), 0, stream, p, *carry);
    } else if (p.out_dtype == APE_F32) hipLaunchKernelGGL((ape_replay_tail_kernel<float, false>), dim3(blocks_for(n)), dim3(256), 0, stream, p, none);
    else hipLaunchKernelGGL((ape_replay_tail_kernel<double, false>), dim3(blocks_for(n)), dim3(256), 0, stream, p, none);
    return hipGetLastError();
}
