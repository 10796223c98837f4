// Subset frames of the stream bank (ape_streams_frame_subset): K listed streams, one raw row each, every stream with its
// own window slot, stack slot and cold flags (a SubsetDesc per list entry, built on the host from per-stream counters).
//
// Launch 1 (here): row -> features (parse_device.h) -> copy 0 of the stream's window ring (all T slots on a cold start) AND the stream's
// time-ordered window, n_mc times, into a compact [K * n_mc][T][I] workspace: the newest row from the block's LDS, the older ones from
// the ring.  The regressor (launch 2) is lstm_forward_impl over those rows with x_ring = 0, every existing route unchanged.
// Launch 3 (here): the bank's post-filter (stream_post_device.h) in its indexed form.
#include "ape_internal.h"
#include "../../include/ape_hip.h"
#include "parse_device.h"
#include "stream_post_device.h"

#pragma clang fp contract(off)

namespace {

using namespace ape_parsedev;
using namespace ape_postdev;

constexpr int SB_BLOCK = 128;                   // threads per workgroup
constexpr int SB_ROWS = 8;                      // list entries per workgroup: a row's features are one dependent f64 chain (parse_rows.hip),
                                                // few entries per block = more CUs busy and a short copy loop behind the chain
constexpr int XW = 39;                          // feature row stride in LDS (odd: conflict-free per-thread rows)

// LAND (host subset frames): p.rows and p.desc are the frame's pinned staging block in host memory; the entries' descriptors
// are also stored to `land`, the bank's device table, where the frame's later launches (and a re-issue) read them
template <bool LAND>
__global__ __launch_bounds__(SB_BLOCK) void ape_subset_rows_kernel(const SubsetRowsParams p, SubsetDesc* __restrict__ land) {
    __shared__ float slab[SB_ROWS * 57];
    __shared__ double xout[SB_ROWS * XW];
    __shared__ int dsc[SB_ROWS][3];             // stream, ring slot, cold
    const int tid = threadIdx.x;
    const int r0 = (int)blockIdx.x * SB_ROWS;
    const int n = min(SB_ROWS, p.K - r0);
    for (int idx = tid; idx < n * p.width; idx += SB_BLOCK) {
        const int rr = idx / p.width, c = idx - rr * p.width;
        float v = p.rows[(size_t)r0 * p.width + idx];
        if (p.big_endian) v = __builtin_bit_cast(float, __builtin_bswap32(__builtin_bit_cast(unsigned, v)));
        slab[rr * 57 + c] = v;
    }
    if (tid < n) {
        const SubsetDesc d = p.desc[r0 + tid];
        dsc[tid][0] = d.stream; dsc[tid][1] = d.slot; dsc[tid][2] = d.cold;
        if constexpr (LAND) land[r0 + tid] = d;
    }
    __syncthreads();
    if (tid < n) [[clang::always_inline]] parse_row(slab + tid * 57, p.width, p.kind, xout + tid * XW);     // (two kernels call it: inline in both, as in the one)
    __syncthreads();
    // element (entry rr, step t, feature i) of the time-ordered window: step T-1 is the new row, step t < T-1 ring slot slot+1+t (mod T);
    // consecutive threads = consecutive elements of one window, so every copy's stores are contiguous
    const int T = p.T, I = p.I, per = T * I;
    const size_t ring_stride = (size_t)p.n_mc * per;
    for (int idx = tid; idx < n * per; idx += SB_BLOCK) {
        const int rr = idx / per, rem = idx - rr * per, t = rem / I, i = rem - t * I;
        const int slot = dsc[rr][1], cold = dsc[rr][2];
        float* ring = p.xring + (size_t)dsc[rr][0] * ring_stride;          // copy 0 of the stream's windows
        const float fresh = (float)xout[rr * XW + i];
        float v;
        if (cold) {                                 // first row since the cold start: every slot (estimator.py:96-97)
            ring[rem] = fresh;
            v = fresh;
        } else if (t == T - 1) {
            ring[slot * I + i] = fresh;
            v = fresh;
        } else {
            int sl = slot + 1 + t;
            if (sl >= T) sl -= T;
            v = ring[sl * I + i];                   // (never the slot written above: sl != slot for t < T - 1)
        }
        float* w = p.xw + (size_t)(r0 + rr) * p.n_mc * per + rem;
        for (int c = 0; c < p.n_mc; ++c) w[(size_t)c * per] = v;
    }
}

// the post-filter's three forms over a list: workgroup / lane = list position (stream_post_device.h, IDX = true)
template <typename TMsg>
__global__ __launch_bounds__(256) void ape_subset_post_kernel(const StreamPostParams p, const SubsetDesc* d) {
    stream_post<TMsg, false, true>(p, (int)blockIdx.x, 0, 1, d);
}
template <typename TMsg>
__global__ __launch_bounds__(256) void ape_subset_post_split_kernel(const StreamPostParams p, const int chunks, const SubsetDesc* d) {
    stream_post<TMsg, true, true>(p, (int)blockIdx.x / chunks, (int)blockIdx.x % chunks, chunks, d);
}
template <typename TMsg>
__global__ __launch_bounds__(256) void ape_subset_post_wide_kernel(const StreamPostParams p, const SubsetDesc* d) {
    stream_post_wide<TMsg, true>(p, (int)blockIdx.x * 64, d);
}
// ... and over the bank's body table: row d[j].stream, whatever the list position (stream_post_device.h, TAB)
template <typename TMsg>
__global__ __launch_bounds__(256) void ape_subset_post_bodies_kernel(const StreamPostParams p, const SubsetDesc* d, const double* bodies) {
    stream_post<TMsg, false, true, true>(p, (int)blockIdx.x, 0, 1, d, bodies);
}
template <typename TMsg>
__global__ __launch_bounds__(256) void ape_subset_post_split_bodies_kernel(const StreamPostParams p, const int chunks, const SubsetDesc* d,
                                                                         const double* bodies) {
    stream_post<TMsg, true, true, true>(p, (int)blockIdx.x / chunks, (int)blockIdx.x % chunks, chunks, d, bodies);
}
template <typename TMsg>
__global__ __launch_bounds__(256) void ape_subset_post_wide_bodies_kernel(const StreamPostParams p, const SubsetDesc* d, const double* bodies) {
    stream_post_wide<TMsg, true, true>(p, (int)blockIdx.x * 64, d, bodies);
}

// ... and with the spread record behind every message row (stream_post_device.h, SPR; TAB: the bank's body table)
template <typename TMsg, bool TAB>
__global__ __launch_bounds__(256) void ape_subset_post_spread_kernel(const StreamPostParams p, const SubsetDesc* d, const double* bodies,
                                                                     const SpreadArgs sp) {
    stream_post<TMsg, false, true, TAB, true>(p, (int)blockIdx.x, 0, 1, d, bodies, sp);
}
template <typename TMsg, bool TAB>
__global__ __launch_bounds__(256) void ape_subset_post_split_spread_kernel(const StreamPostParams p, const int chunks, const SubsetDesc* d,
                                                                           const double* bodies, const SpreadArgs sp) {
    stream_post<TMsg, true, true, TAB, true>(p, (int)blockIdx.x / chunks, (int)blockIdx.x % chunks, chunks, d, bodies, sp);
}
template <typename TMsg, bool TAB>
__global__ __launch_bounds__(256) void ape_subset_post_wide_spread_kernel(const StreamPostParams p, const SubsetDesc* d, const double* bodies) {
    stream_post_wide<TMsg, true, TAB, true>(p, (int)blockIdx.x * 64, d, bodies);
}

template <typename TMsg, bool TAB>
hipError_t launch_subset_post_spread(const StreamPostParams& p, const SubsetDesc* d, const SpreadArgs& sp, int form, const double* bodies,
                                     hipStream_t stream) {
    if (form == 0) {
        hipLaunchKernelGGL((ape_subset_post_wide_spread_kernel<TMsg, TAB>), dim3((p.S + 63) / 64), dim3(256), 0, stream, p, d, bodies);
        return hipGetLastError();
    }
    const int chunks = form;
    if (chunks > 1) {
        hipLaunchKernelGGL((ape_subset_post_split_spread_kernel<TMsg, TAB>), dim3(p.S * chunks), dim3(256), 0, stream, p, chunks, d, bodies, sp);
        return hipGetLastError();
    }
    hipLaunchKernelGGL((ape_subset_post_spread_kernel<TMsg, TAB>), dim3(p.S), dim3(256), 0, stream, p, d, bodies, sp);
    return hipGetLastError();
}

// ... and of a bank with per-stream smoothing lengths (stream_post_device.h, SMT): the length of entry j is sm.smooths[d[j].stream]
template <typename TMsg, bool SPR>
__global__ __launch_bounds__(256) void ape_subset_post_smooths_kernel(const StreamPostParams p, const SubsetDesc* d, const double* bodies,
                                                                      const SpreadArgs sp, const SmoothArgs sm) {
    stream_post<TMsg, false, true, false, SPR, true>(p, (int)blockIdx.x, 0, 1, d, bodies, sp, sm);
}
template <typename TMsg, bool SPR>
__global__ __launch_bounds__(256) void ape_subset_post_split_smooths_kernel(const StreamPostParams p, const int chunks, const SubsetDesc* d,
                                                                            const double* bodies, const SpreadArgs sp, const SmoothArgs sm) {
    stream_post<TMsg, true, true, false, SPR, true>(p, (int)blockIdx.x / chunks, (int)blockIdx.x % chunks, chunks, d, bodies, sp, sm);
}

template <typename TMsg, bool SPR>
hipError_t launch_subset_post_smooths(const StreamPostParams& p, const SubsetDesc* d, const SmoothArgs& sm, const SpreadArgs& sp, int form,
                                      const double* bodies, hipStream_t stream) {
    if (form > 1) hipLaunchKernelGGL((ape_subset_post_split_smooths_kernel<TMsg, SPR>), dim3(p.S * form), dim3(256), 0, stream, p, form, d, bodies, sp, sm);
    else hipLaunchKernelGGL((ape_subset_post_smooths_kernel<TMsg, SPR>), dim3(p.S), dim3(256), 0, stream, p, d, bodies, sp, sm);
    return hipGetLastError();
}

hipError_t launch_subset_post_bodies(const StreamPostParams& p, const SubsetDesc* d, const double* bodies, hipStream_t stream) {
    if (p.smooth == 1 && p.n_mc == 1 && p.S >= 8) {
        const int wide = (p.S + 63) / 64;
        if (p.msg_dtype == APE_F32) hipLaunchKernelGGL(ape_subset_post_wide_bodies_kernel<float>, dim3(wide), dim3(256), 0, stream, p, d, bodies);
        else hipLaunchKernelGGL(ape_subset_post_wide_bodies_kernel<double>, dim3(wide), dim3(256), 0, stream, p, d, bodies);
        return hipGetLastError();
    }
    const int chunks = ape_stream_post_chunks(p.smooth * p.n_mc);
    if (p.part != nullptr && chunks > 1) {
        if (p.msg_dtype == APE_F32) hipLaunchKernelGGL(ape_subset_post_split_bodies_kernel<float>, dim3(p.S * chunks), dim3(256), 0, stream, p, chunks, d, bodies);
        else hipLaunchKernelGGL(ape_subset_post_split_bodies_kernel<double>, dim3(p.S * chunks), dim3(256), 0, stream, p, chunks, d, bodies);
        return hipGetLastError();
    }
    if (p.msg_dtype == APE_F32) hipLaunchKernelGGL(ape_subset_post_bodies_kernel<float>, dim3(p.S), dim3(256), 0, stream, p, d, bodies);
    else hipLaunchKernelGGL(ape_subset_post_bodies_kernel<double>, dim3(p.S), dim3(256), 0, stream, p, d, bodies);
    return hipGetLastError();
}

}  // namespace

hipError_t ape_launch_subset_rows(const SubsetRowsParams& p, hipStream_t stream) {
    if (p.K < 1) return hipSuccess;
    hipLaunchKernelGGL(ape_subset_rows_kernel<false>, dim3((p.K + SB_ROWS - 1) / SB_ROWS), dim3(SB_BLOCK), 0, stream, p, (SubsetDesc*)nullptr);
    return hipGetLastError();
}

// a host subset frame's first launch: rows and descriptors from pinned host memory, the descriptors landed in `land` [K] on the device
hipError_t ape_launch_subset_rows_host(const SubsetRowsParams& p, SubsetDesc* land, hipStream_t stream) {
    if (p.K < 1) return hipSuccess;
    hipLaunchKernelGGL(ape_subset_rows_kernel<true>, dim3((p.K + SB_ROWS - 1) / SB_ROWS), dim3(SB_BLOCK), 0, stream, p, land);
    return hipGetLastError();
}

// the same choice of form on the SPR instantiations
hipError_t ape_launch_stream_post_subset_spread(const StreamPostParams& p, const SubsetDesc* d, const SpreadArgs& sp, int form, hipStream_t stream,
                                                const double* bodies) {
    if (p.S < 1) return hipSuccess;
    if (form > 1 && (p.part == nullptr || sp.part == nullptr)) return hipErrorInvalidValue;
    if (bodies != nullptr)
        return p.msg_dtype == APE_F32 ? launch_subset_post_spread<float, true>(p, d, sp, form, bodies, stream)
                                      : launch_subset_post_spread<double, true>(p, d, sp, form, bodies, stream);
    return p.msg_dtype == APE_F32 ? launch_subset_post_spread<float, false>(p, d, sp, form, nullptr, stream)
                                  : launch_subset_post_spread<double, false>(p, d, sp, form, nullptr, stream);
}

// the same choice of form as ape_launch_stream_post (fk.hip), with p.S = the list's length
hipError_t ape_launch_stream_post_subset(const StreamPostParams& p, const SubsetDesc* d, hipStream_t stream, const double* bodies) {
    if (p.S < 1) return hipSuccess;
    if (bodies != nullptr) return launch_subset_post_bodies(p, d, bodies, stream);
    if (p.smooth == 1 && p.n_mc == 1 && p.S >= 8) {
        const int wide = (p.S + 63) / 64;
        if (p.msg_dtype == APE_F32) hipLaunchKernelGGL(ape_subset_post_wide_kernel<float>, dim3(wide), dim3(256), 0, stream, p, d);
        else hipLaunchKernelGGL(ape_subset_post_wide_kernel<double>, dim3(wide), dim3(256), 0, stream, p, d);
        return hipGetLastError();
    }
    const int chunks = ape_stream_post_chunks(p.smooth * p.n_mc);
    if (p.part != nullptr && chunks > 1) {
        if (p.msg_dtype == APE_F32) hipLaunchKernelGGL(ape_subset_post_split_kernel<float>, dim3(p.S * chunks), dim3(256), 0, stream, p, chunks, d);
        else hipLaunchKernelGGL(ape_subset_post_split_kernel<double>, dim3(p.S * chunks), dim3(256), 0, stream, p, chunks, d);
        return hipGetLastError();
    }
    if (p.msg_dtype == APE_F32) hipLaunchKernelGGL(ape_subset_post_kernel<float>, dim3(p.S), dim3(256), 0, stream, p, d);
    else hipLaunchKernelGGL(ape_subset_post_kernel<double>, dim3(p.S), dim3(256), 0, stream, p, d);
    return hipGetLastError();
}

// the table forms over a list (as ape_launch_stream_post_smooths, fk.hip)
hipError_t ape_launch_stream_post_subset_smooths(const StreamPostParams& p, const SubsetDesc* d, const SmoothArgs& sm, const SpreadArgs* sp, int form,
                                                 hipStream_t stream, const double* bodies) {
    if (p.S < 1) return hipSuccess;
    if (form < 1 || sm.smooths == nullptr) return hipErrorInvalidValue;
    if (form > 1 && (p.part == nullptr || (sp != nullptr && sp->part == nullptr))) return hipErrorInvalidValue;
    if (sp != nullptr)
        return p.msg_dtype == APE_F32 ? launch_subset_post_smooths<float, true>(p, d, sm, *sp, form, bodies, stream)
                                      : launch_subset_post_smooths<double, true>(p, d, sm, *sp, form, bodies, stream);
    return p.msg_dtype == APE_F32 ? launch_subset_post_smooths<float, false>(p, d, sm, SpreadArgs{}, form, bodies, stream)
                                  : launch_subset_post_smooths<double, false>(p, d, sm, SpreadArgs{}, form, bodies, stream);
}
