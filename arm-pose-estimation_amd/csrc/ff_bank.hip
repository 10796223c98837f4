// The regressor stage of a DropoutFF / ImuPoseLSTM stream-bank frame and replay.
//
// DropoutFF inside an estimator (reference estimate/estimator.py:93-120 -> watch_phone_pocket_nn.py:98-112 -> nn_models.py:340-370): the
// window [1,T,I] is repeated n_mc times, the MLP runs on every row and [:, -1, :] keeps the newest row -- so per frame and stream only
// the newest feature row counts, and the n_mc rows differ by nothing but the Bernoulli(1-p) mask (scaled 1/(1-p)) over the H outputs of
// the last hidden layer, in front of _output_layer.  The trunk (input layer + hidden layers, leaky_relu) is therefore computed ONCE per
// stream -- ape_mlp_tile16 with `hidden_out`, f64 z-score fused into its load -- and the kernel here is the n_mc masked heads:
//
//   ape_ff_bank_head   one wave64 per tile of 16 SAMPLE rows (global row r = stream * n_mc + sample; a tile may straddle streams):
//                      A = the row's stream's hidden row [H] times the row's mask, B = W_out^T padded to 16 or 32 columns, on
//                      v_mfma_f32_16x16x4_f32 (exact f32), bias as the initial accumulator.  The k-order inside a 16-block is the one
//                      ape_mlp_tile16 uses (lane group g feeds k = 16q + 4g + j to instruction j), so A and B are plain 16-byte loads:
//                      the hidden rows and W_out (<= 32 KB) come from L2 / L1, no LDS, no barrier.
//                      Masks: injected multipliers [rows, H] (test hook) or Philox4x32-10 with counter (row lo, row hi, k / 4, 0xFE) and the
//                      call's key -- four consecutive hidden units per draw; keep where u >= p like every other dropout kernel here.
//                      Work per sample row: 2*H*O FLOP, H*4 bytes in (L2-resident: n_mc rows share one hidden row), O*4 bytes out.
//
// ImuPoseLSTM inside an estimator (nn_models.py:236-251): no repeat, no dropout -- the frame is the plain forward over every stream's
// window.  ape_ring_windows_kernel undoes the ring order of the bank's feature windows ([S][T][I], step t in slot (t + x_ring) mod T, the
// cold-start pad already in the slots) into the time-ordered [S,T,I] image that the existing forward consumes with x_ring = 0: the frame
// then takes exactly the launches of a subset frame over compact windows (input layer on ape_mlp_tile16, the LSTM on the first-generation
// wide cluster kernel up to 512 windows and layer-split on lstm_upper32.hip above), which is what makes lockstep and subset frames of one
// schedule bit-equal.
#include "ape_internal.h"
#include "../../include/ape_hip.h"

namespace {

template <int NTO>
__global__ __launch_bounds__(256) void ape_ff_bank_head(const FfHeadParams p) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int r = lane & 15, g = lane >> 4;
    const long long tile0 = ((long long)blockIdx.x * 4 + wave) * 16;
    if (tile0 >= p.rows) return;                                   // (the whole wave: no barrier in this kernel)
    // A operand: lane (r, g) feeds row tile0 + r; rows behind the last one repeat it and are never stored
    long long lr = tile0 + r;
    if (lr >= p.rows) lr = p.rows - 1;
    const long long grow = p.row_base + lr;                        // global sample row: stream grow / n_mc, sample grow % n_mc
    const int H = p.H, O = p.O;
    const float* hrow = p.hidden + (size_t)(grow / p.n_mc - p.g_base) * H;
    const float* mrow = p.masks != nullptr ? p.masks + (size_t)grow * H : nullptr;
    const bool philox = mrow == nullptr && p.dropout_p > 0.0f;
    const float keep = 1.0f / (1.0f - p.dropout_p);
    f32x4 acc[NTO];
    const float* wrow[NTO];
#pragma unroll
    for (int n = 0; n < NTO; ++n) {
        const int col = n * 16 + r;
        const float bv = col < O ? p.b_out[col] : 0.0f;
        acc[n] = f32x4{bv, bv, bv, bv};
        wrow[n] = col < O ? p.w_out + (size_t)col * H : nullptr;   // padded columns of W_out^T are zero
    }
    for (int q = 0; q < H / 16; ++q) {
        const int k0 = 16 * q + 4 * g;
        f32x4 a = *reinterpret_cast<const f32x4*>(hrow + k0);
        if (mrow != nullptr) {
            const f32x4 mk = *reinterpret_cast<const f32x4*>(mrow + k0);
            a = a * mk;
        } else if (philox) {
            uint32_t rnd[4];
            const unsigned long long prow = (unsigned long long)(grow + p.philox_base);
            philox4x32((uint32_t)prow, (uint32_t)(prow >> 32), (uint32_t)(k0 >> 2), 0xFEu, (uint32_t)p.seed,
                       (uint32_t)(p.seed >> 32), rnd);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float uf = (float)(rnd[i] >> 8) * (1.0f / 16777216.0f);
                a[i] *= (uf >= p.dropout_p) ? keep : 0.0f;
            }
        }
        f32x4 b[NTO];
#pragma unroll
        for (int n = 0; n < NTO; ++n)
            b[n] = wrow[n] != nullptr ? *reinterpret_cast<const f32x4*>(wrow[n] + k0) : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int n = 0; n < NTO; ++n) acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], b[n][j], acc[n], 0, 0, 0);
    }
    // accumulator register i of lane (r, g) = (row 4g + i, column r) of the tile
#pragma unroll
    for (int n = 0; n < NTO; ++n) {
        const int col = n * 16 + r;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const long long row = tile0 + 4 * g + i;
            if (row < p.rows && col < O) p.y[(size_t)row * O + col] = acc[n][i];
        }
    }
}

// time-ordered copy of every stream's window ring: xw[s][t][:] = xring[s][(t + x_ring) mod T][:]
__global__ __launch_bounds__(256) void ape_ring_windows_kernel(const float* __restrict__ xring, float* __restrict__ xw, long long n, int T,
                                                               int I, int x_ring) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n) return;
    const int per = T * I;
    const long long s = idx / per;
    const int rem = (int)(idx - s * per), t = rem / I, i = rem - t * I;
    const int slot = (t + x_ring >= T) ? t + x_ring - T : t + x_ring;
    xw[idx] = xring[s * per + (long long)slot * I + i];
}

}  // namespace

hipError_t ape_launch_ff_bank_head(const FfHeadParams& p, hipStream_t stream) {
    if (p.rows < 1) return hipSuccess;
    if (p.H % 16 != 0 || p.O < 1 || p.O > 32 || p.n_mc < 1) return hipErrorInvalidValue;
    const unsigned blocks = (unsigned)((p.rows + 63) / 64);
    if (p.O <= 16) hipLaunchKernelGGL(ape_ff_bank_head<1>, dim3(blocks), dim3(256), 0, stream, p);
    else hipLaunchKernelGGL(ape_ff_bank_head<2>, dim3(blocks), dim3(256), 0, stream, p);
    return hipGetLastError();
}

hipError_t ape_launch_ring_windows(const float* xring, float* xw, int S, int T, int I, int x_ring, hipStream_t stream) {
    const long long n = (long long)S * T * I;
    if (n < 1) return hipSuccess;
    hipLaunchKernelGGL(ape_ring_windows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, xring, xw, n, T, I, x_ring);
    return hipGetLastError();
}
