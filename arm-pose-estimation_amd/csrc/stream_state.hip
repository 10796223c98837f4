// Stream state hand-over (ape_streams_export / ape_streams_import): the window and the smoothing stack of K listed
// streams between the bank's rings and the canonical records [K][words] -- window[T][I], stack[smooth][n_mc * O], oldest first, zero
// words up to a multiple of 4.
//
// ape_state_export_kernel   rings -> records (a cold part as zeros)
// ape_state_import_kernel   records -> copy 0 of the window ring and the stack ring, time order = slot order (the host sets the stream's
//                           counters to multiples of T / smooth); a cold part is not written
//
// One thread per 16 bytes of a record: the canonical side is one 16-byte access per thread, consecutive threads consecutive units; the
// ring side is four 4-byte accesses whose slot comes from the index arithmetic (canonical row t lives in slot (oldest + t) mod size),
// contiguous within a row.  A few hundred bytes per stream: these launches are latency-bound, nothing here is tuned beyond that.
#include "ape_internal.h"
#include "../../include/ape_hip.h"

namespace {

constexpr int ST_BLOCK = 256;

// word w of stream d's record <-> its place in the rings (nullptr: padding, or a cold part)
// k: the stream's smoothing length (a bank with per-stream lengths, DESIGN.md 4.35: the record keeps the capacity's size, the stream's k
// predictions oldest first, zeros behind them; the ring keeps the capacity's stride and the stream lives in its slots 0 .. k-1)
template <bool SMT>
__device__ __forceinline__ float* ring_word(const StateParams& p, const StateDesc& d, int w, const int k) {
    const int nx = p.T * p.I;
    if (w < nx) {
        if (!(d.warm & APE_STATE_WINDOW_WARM)) return nullptr;
        const int t = w / p.I, i = w - t * p.I;
        int slot = d.wslot + t;
        if (slot >= p.T) slot -= p.T;
        return p.xring + (size_t)d.stream * p.x_stream_stride + (size_t)slot * p.I + i;
    }
    w -= nx;
    if (w >= p.smooth * p.MO || !(d.warm & APE_STATE_STACK_WARM)) return nullptr;
    const int j = w / p.MO, r = w - j * p.MO;
    if (SMT && j >= k) return nullptr;
    int slot = d.sslot + j;
    if (slot >= k) slot -= k;
    return p.yring + ((size_t)d.stream * p.smooth + slot) * p.MO + r;
}

__device__ __forceinline__ float* ring_word(const StateParams& p, const StateDesc& d, int w) { return ring_word<false>(p, d, w, p.smooth); }

// SMT: the stream's length is smooths[d.stream] (the bank's device table) instead of p.smooth
template <bool IMPORT>
__global__ __launch_bounds__(ST_BLOCK) void ape_state_smooths_kernel(const StateParams p, const int* __restrict__ smooths) {
    const int units = p.words / 4;
    const long long idx = (long long)blockIdx.x * ST_BLOCK + threadIdx.x;
    if (idx >= (long long)p.K * units) return;
    const int j = (int)(idx / units), u = (int)(idx - (long long)j * units);
    const StateDesc d = p.desc[j];
    const int k = smooths[d.stream];
    f32x4 v;
    if constexpr (IMPORT) v = reinterpret_cast<const f32x4*>(p.state)[idx];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        float* r = ring_word<true>(p, d, 4 * u + c, k);
        if constexpr (IMPORT) { if (r) *r = v[c]; }
        else v[c] = r ? *r : 0.0f;
    }
    if constexpr (!IMPORT) reinterpret_cast<f32x4*>(p.state)[idx] = v;
}

__global__ __launch_bounds__(ST_BLOCK) void ape_state_export_kernel(const StateParams p) {
    const int units = p.words / 4;
    const long long idx = (long long)blockIdx.x * ST_BLOCK + threadIdx.x;
    if (idx >= (long long)p.K * units) return;
    const int j = (int)(idx / units), u = (int)(idx - (long long)j * units);
    const StateDesc d = p.desc[j];
    f32x4 v;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const float* src = ring_word(p, d, 4 * u + c);
        v[c] = src ? *src : 0.0f;
    }
    reinterpret_cast<f32x4*>(p.state)[idx] = v;
}

__global__ __launch_bounds__(ST_BLOCK) void ape_state_import_kernel(const StateParams p) {
    const int units = p.words / 4;
    const long long idx = (long long)blockIdx.x * ST_BLOCK + threadIdx.x;
    if (idx >= (long long)p.K * units) return;
    const int j = (int)(idx / units), u = (int)(idx - (long long)j * units);
    const StateDesc d = p.desc[j];
    const f32x4 v = reinterpret_cast<const f32x4*>(p.state)[idx];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        float* dst = ring_word(p, d, 4 * u + c);
        if (dst) *dst = v[c];
    }
}

unsigned blocks_for(long long n) { return (unsigned)((n + ST_BLOCK - 1) / ST_BLOCK); }

}  // namespace

hipError_t ape_launch_state_export(const StateParams& p, hipStream_t stream) {
    if (p.K < 1) return hipSuccess;
    hipLaunchKernelGGL(ape_state_export_kernel, dim3(blocks_for((long long)p.K * (p.words / 4))), dim3(ST_BLOCK), 0, stream, p);
    return hipGetLastError();
}

hipError_t ape_launch_state_import(const StateParams& p, hipStream_t stream) {
    if (p.K < 1) return hipSuccess;
    hipLaunchKernelGGL(ape_state_import_kernel, dim3(blocks_for((long long)p.K * (p.words / 4))), dim3(ST_BLOCK), 0, stream, p);
    return hipGetLastError();
}

// ... of a bank with per-stream smoothing lengths (smooths: its device table [S])
hipError_t ape_launch_state_smooths(const StateParams& p, const int* smooths, bool import, hipStream_t stream) {
    if (p.K < 1) return hipSuccess;
    const dim3 grid(blocks_for((long long)p.K * (p.words / 4)));
    if (import) hipLaunchKernelGGL(ape_state_smooths_kernel<true>, grid, dim3(ST_BLOCK), 0, stream, p, smooths);
    else hipLaunchKernelGGL(ape_state_smooths_kernel<false>, grid, dim3(ST_BLOCK), 0, stream, p, smooths);
    return hipGetLastError();
}
