// The register images of a model's weights, as the kernels' waves stream them: pure host arithmetic, no HIP (tests/host/weight_pack_main.cpp
// compiles this header alone with a host compiler).  One packer per image, each writing exactly its *_elems() elements into the caller's
// storage; ape_model_create plans the device buffers with the same *_elems(), ape_model_load_weights (api_weights.hip) walks the blob,
// calls the packers and copies.  Every LSTM image reads Wcat = [W_ih | 0-pad to KXl | W_hh] of one layer through ONE accessor, WCat.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>

#ifndef APE_C32_HSHIFT
#define APE_C32_HSHIFT 15         // (ape_internal.h's value: a different one there is a redefinition error)
#endif

// Wcat[row][k] of one LSTM layer: columns [0, in_l) of W_ih [4H, in_l], zeros up to KXl, then W_hh [4H, H]
struct WCat {
    const float* w_ih; int in_l; const float* w_hh; int H, KXl;
    float operator()(int row, int k) const {
        if (k < KXl) return (k < in_l) ? w_ih[(size_t)row * in_l + k] : 0.0f;
        return w_hh[(size_t)row * H + (k - KXl)];
    }
};

// ---- batch-tile LSTM kernel (lstm_tile16.hip) -------------------------------------------------------------------------------------
// [W_ih | W_hh] of one layer in the order the kernel's waves stream it:
//   packed[((w*Q + q)*NT + n)*64 + lane][j] = Wcat[gate*H + w*H/4 + u*16 + (lane&15)][16q + 4(lane>>4) + j]
// with n = gate*UB + u, UB = H / 64, NT = 4 UB, Q = (KXl + H) / 16
static inline size_t wpack_elems(int H, int KXl) { return (size_t)4 * ((KXl + H) / 16) * (4 * (H / 64)) * 64 * 4; }
static inline void pack_wpack(const WCat& wcat, float* out) {
    const int H = wcat.H, UB = H / 64, NT = 4 * UB, Q = (wcat.KXl + H) / 16;
    for (int w = 0; w < 4; ++w)
        for (int q = 0; q < Q; ++q)
            for (int n = 0; n < NT; ++n) {
                const int gate = n / UB, u = n % UB;
                for (int lane = 0; lane < 64; ++lane) {
                    const int row = gate * H + w * (H / 4) + u * 16 + (lane & 15);
                    float* dst = out + ((((size_t)w * Q + q) * NT + n) * 64 + lane) * 4;
                    for (int j = 0; j < 4; ++j) dst[j] = wcat(row, 16 * q + 4 * (lane >> 4) + j);
                }
            }
}

// ---- MLP kernel (mlp_tile16.hip): DropoutFF's layers and ImuPoseLSTM's input layer ---------------------------------------------------
// one layer W [H, in_j], its input zero-padded to K: [wave 4][k-block q][tile n][lane][4], lane holds
// W[w*H/4 + n*16 + (lane&15)][16q + 4(lane>>4) + j]
static inline size_t ff_wpack_elems(int H, int K) { return (size_t)K * H; }
static inline void pack_ff_wpack(const float* wj, int in_j, int H, int K, float* out) {
    const int NTF = H / 64, Q = K / 16;
    for (int w = 0; w < 4; ++w)
        for (int q = 0; q < Q; ++q)
            for (int n = 0; n < NTF; ++n)
                for (int lane = 0; lane < 64; ++lane) {
                    const int col = w * (H / 4) + n * 16 + (lane & 15);
                    for (int jj = 0; jj < 4; ++jj) {
                        const int k = 16 * q + 4 * (lane >> 4) + jj;
                        out[((((size_t)w * Q + q) * NTF + n) * 64 + lane) * 4 + jj] = (k < in_j) ? wj[(size_t)col * in_j + k] : 0.0f;
                    }
                }
}

// ---- MLP pipeline (mlp_pipe.hip): the four register files of its two stages -----------------------------------------------------------
// layers 0..2 (three images): v_mfma_f32_32x32x2_f32 A fragments, register 4 kb + j of lane (unit column = lane & 31, hh = lane >> 5) =
// W[64 wave + 32 ct + (lane & 31)][8 kb + 4 hh + j]; [wave][ct][kb][lane][4], kbl k-blocks of 8 (the input zero-padded to 8 kbl)
static inline size_t mlp_pipe_elems(int kbl) { return (size_t)4 * 2 * kbl * 64 * 4; }
static inline void pack_mlp_pipe(const float* wl, int inl, int kbl, float* out) {
    for (int w = 0; w < 4; ++w)
        for (int ct = 0; ct < 2; ++ct)
            for (int kb = 0; kb < kbl; ++kb)
                for (int lane = 0; lane < 64; ++lane)
                    for (int jj = 0; jj < 4; ++jj) {
                        const int unit = 64 * w + 32 * ct + (lane & 31), k = 8 * kb + 4 * (lane >> 5) + jj;
                        out[((((size_t)w * 2 + ct) * kbl + kb) * 64 + lane) * 4 + jj] = (k < inl) ? wl[(size_t)unit * inl + k] : 0.0f;
                    }
}
// the head W_out [O, H] (H = 256), rows zero-padded to 32: register 4 kb + j of lane (o = lane & 31, hh) = W_out[o][64 wave + 8 kb + 4 hh + j];
// [wave][kb 8][lane][4]
static inline size_t mlp_pipe_head_elems() { return (size_t)4 * 8 * 64 * 4; }
static inline void pack_mlp_pipe_head(const float* w_out, int O, int H, float* out) {
    for (int w = 0; w < 4; ++w)
        for (int kb = 0; kb < 8; ++kb)
            for (int lane = 0; lane < 64; ++lane)
                for (int jj = 0; jj < 4; ++jj) {
                    const int o = lane & 31, k = 64 * w + 8 * kb + 4 * (lane >> 5) + jj;
                    out[(((size_t)w * 8 + kb) * 64 + lane) * 4 + jj] = (o < O) ? w_out[(size_t)o * H + k] : 0.0f;
                }
}

// ---- first-generation cluster kernel (lstm_cluster.hip; also lstm_cluster16.hip, lstm_level16.hip): wcl ------------------------------
// [member GH = H/16][wave 4][i/4][lane][i%4] with i = 4q + j; lane = (g << 4) | (u << 2) | gate holds
// Wcat[gate*H + member*16 + wave*4 + u][16q + 4g + j] -- the register file of that wave (register i of that lane; stored
// [k-quad i/4][lane][i%4] so a lane fetches 4 registers per load)
static inline size_t wcl_elems(int H, int KXl) { return (size_t)(H / 16) * 4 * ((KXl + H) / 4) * 64; }
static inline void pack_wcl(const WCat& wcat, float* out) {
    const int H = wcat.H, GH = H / 16, NW = (wcat.KXl + H) / 4;
    for (int mem = 0; mem < GH; ++mem)
        for (int w = 0; w < 4; ++w)
            for (int i = 0; i < NW; ++i)
                for (int lane = 0; lane < 64; ++lane) {
                    const int c = lane & 15, g = lane >> 4, u = c >> 2, gate = c & 3;   // tile row = unit*4 + gate
                    const int row = gate * H + mem * 16 + w * 4 + u;
                    out[((((size_t)(mem * 4 + w) * (NW / 4)) + i / 4) * 64 + lane) * 4 + (i % 4)] = wcat(row, 16 * (i / 4) + 4 * g + (i % 4));
                }
}

// ---- latency kernel, H/8 members (lstm_cluster_small.hip, layer 0 of lstm_mc_small.hip): wcls ------------------------------------------
// a wave owns 2 units = 8 columns, 8 k-groups; lane = (g << 3) | (u << 2) | gate holds Wcat[gate*H + (member*4 + wave)*2 + u][32q + 4g + j]
// in register 4q + j; same [i/4][lane][i%4] storage
static inline size_t wcls_elems(int H, int KXl) { return (size_t)(H / 8) * 4 * ((KXl + H) / 8) * 64; }
static inline void pack_wcls(const WCat& wcat, float* out) {
    const int H = wcat.H, GS = H / 8, NWS = (wcat.KXl + H) / 8;
    for (int mem = 0; mem < GS; ++mem)
        for (int w = 0; w < 4; ++w)
            for (int i = 0; i < NWS; ++i)
                for (int lane = 0; lane < 64; ++lane) {
                    const int c = lane & 7, g = lane >> 3, u = c >> 2, gate = c & 3;
                    const int row = gate * H + (mem * 4 + w) * 2 + u;
                    out[((((size_t)(mem * 4 + w) * (NWS / 4)) + i / 4) * 64 + lane) * 4 + (i % 4)] = wcat(row, 32 * (i / 4) + 4 * g + (i % 4));
                }
}

// ---- Monte-Carlo latency kernel, layers above layer 0 (lstm_mc_small.hip; KXl = H): wmc and wmc16 --------------------------------------
// wmc (v_mfma_f32_4x4x1_16b_f32): H/8 members x 4 waves, wave w = K quarter w of [W_ih | W_hh]; lane = (block b = lane >> 2: unit b & 7 of
// the member, k slice ks = b >> 3; gate = lane & 3) holds Wcat[gate*H + member*8 + (b & 7)][w*H/2 + 8 (i/4) + 4 ks + (i%4)] in register i;
// stored [member][wave][i/4][lane][i%4]
static inline size_t wmc_elems(int H) { return (size_t)(H / 8) * 4 * (H / 4) * 64; }
static inline void pack_wmc(const WCat& wcat, float* out) {
    const int H = wcat.H, GM = H / 8, NI4 = H / 4;
    for (int mem = 0; mem < GM; ++mem)
        for (int w = 0; w < 4; ++w)
            for (int i = 0; i < NI4; ++i)
                for (int lane = 0; lane < 64; ++lane) {
                    const int gate = lane & 3, ub = (lane >> 2) & 7, ks = lane >> 5;
                    const int row = gate * H + mem * 8 + ub;
                    out[((((size_t)(mem * 4 + w) * (NI4 / 4)) + i / 4) * 64 + lane) * 4 + (i % 4)] = wcat(row, w * (H / 2) + 8 * (i / 4) + 4 * ks + (i % 4));
                }
}
// wmc16, the 16 x 16 x 4 image of its 16-row form: wave = (column tile ct = w & 1, K half kh = w >> 1); lane = (g << 4) | (u << 2) | gate
// holds Wcat[gate*H + member*8 + ct*4 + u][kh*H + 16q + 4g + j] in register 4q + j; stored [member][wave][q][lane][4]
static inline size_t wmc16_elems(int H) { return (size_t)(H / 8) * 4 * (H / 16) * 64 * 4; }
static inline void pack_wmc16(const WCat& wcat, float* out) {
    const int H = wcat.H, GM = H / 8, NQm = H / 16;
    for (int mem = 0; mem < GM; ++mem)
        for (int w = 0; w < 4; ++w)
            for (int q = 0; q < NQm; ++q)
                for (int lane = 0; lane < 64; ++lane) {
                    const int c = lane & 15, g = lane >> 4, u = c >> 2, gate = c & 3, ct = w & 1, kh = w >> 1;
                    const int row = gate * H + mem * 8 + ct * 4 + u;
                    for (int j = 0; j < 4; ++j) out[((((size_t)(mem * 4 + w) * NQm) + q) * 64 + lane) * 4 + j] = wcat(row, kh * H + 16 * q + 4 * g + j);
                }
}

// ---- fp16 cluster kernels (lstm_cluster_f16.hip, lstm_cluster_f16v2.hip): wcl16 -------------------------------------------------------
// [member H/16][wave][32-deep k-block q][lane][8]: lane = (g << 4) | (u << 2) | gate holds Wcat[gate*H + member*16 + wave*4 + u][32q + 8g + j]
// as binary16
static inline size_t wcl16_elems(int H, int KXl) { return (size_t)(H / 16) * 4 * ((KXl + H) / 32) * 64 * 8; }
static inline void pack_wcl16(const WCat& wcat, _Float16* out) {
    const int H = wcat.H, GH = H / 16, NB = (wcat.KXl + H) / 32;
    for (int mem = 0; mem < GH; ++mem)
        for (int w = 0; w < 4; ++w)
            for (int q = 0; q < NB; ++q)
                for (int lane = 0; lane < 64; ++lane) {
                    const int c = lane & 15, g = lane >> 4, u = c >> 2, gate = c & 3;
                    const int row = gate * H + mem * 16 + w * 4 + u;
                    for (int j = 0; j < 8; ++j) out[((((size_t)(mem * 4 + w) * NB) + q) * 64 + lane) * 8 + j] = (_Float16)wcat(row, 32 * q + 8 * g + j);
                }
}

// ---- 32-row clusters on v_mfma_f32_32x32x2_f32, weights = A operand: wcl32 (lstm_cluster32.hip, lstm_upper32.hip), wup128 ---------------
// `members` x 4 waves, a wave owns 8 units = 32 columns ordered gate * 8 + unit.  [member][wave][i / 4][lane][i % 4] with register
// i = 4 kb + j of lane (column m = lane & 31, half hh = lane >> 5) = Wcat[gate(m) * H + member*32 + wave*8 + (m & 7)][8 kb + 4 hh + j];
// (KXl + H) / 2 registers per lane: 32 columns x K / 64 lanes
static inline size_t wfrag32_elems(int members, int H, int KXl) { return (size_t)members * 4 * ((KXl + H) / 2) * 64; }
template <typename At>
static inline void pack_wfrag32(int members, int H, int KXl, At at, float* out) {
    const int NW = (KXl + H) / 2;
    for (int mem = 0; mem < members; ++mem)
        for (int w = 0; w < 4; ++w)
            for (int i = 0; i < NW; ++i)
                for (int lane = 0; lane < 64; ++lane) {
                    const int mcol = lane & 31, hh = lane >> 5;
                    const int row = (mcol >> 3) * H + mem * 32 + w * 8 + (mcol & 7);
                    out[((((size_t)(mem * 4 + w) * (NW / 4)) + i / 4) * 64 + lane) * 4 + (i % 4)] = at(row, 8 * (i / 4) + 4 * hh + (i % 4));
                }
}
// wcl32: the 8 members of an H = 256 layer
static inline size_t wcl32_elems(int H, int KXl) { return wfrag32_elems(8, H, KXl); }
static inline void pack_wcl32(const WCat& wcat, float* out) { pack_wfrag32(8, wcat.H, wcat.KXl, wcat, out); }
// wup128 (lstm_upper128.hip): the four members of a layer >= 1 of the 3 x 128 model.  Such a layer has no padding (in_l = KXl = H), and the
// image says so: W_ih is read without the zero-pad branch
static inline size_t wup128_elems(int H, int KXl) { return wfrag32_elems(4, H, KXl); }
static inline void pack_wup128(const WCat& wcat, float* out) {
    const float* w_ih = wcat.w_ih; const float* w_hh = wcat.w_hh;
    const int in_l = wcat.in_l, H = wcat.H, KXl = wcat.KXl;
    pack_wfrag32(4, H, KXl, [=](int row, int k) { return k < KXl ? w_ih[(size_t)row * in_l + k] : w_hh[(size_t)row * H + (k - KXl)]; }, out);
}

// ---- split register image of lstm_cluster32.hip: wcl32s --------------------------------------------------------------------------------
// (the recurrent products on v_mfma_f32_32x32x16_f16): the same size and the same [member 8][wave 4][group][lane 64][4 dwords] order as
// the f32 image (wcl32), one wave's 32 columns ordered gate * 8 + unit (column m = lane & 31, half hh = lane >> 5).  The first `kx_f32`
// columns of Wcat = [W_ih | W_hh] (layer 0's input columns) stay f32, as in the f32 image: group kb, dword j = Wcat[row][8 kb + 4 hh + j] * 2^S.
// The remaining columns come in K = 16 slices s, two groups each: group kx_f32 / 8 + 2 s holds hi = f16(W * 2^sw) and group + 1
// lo = f16(W * 2^sw - hi), both in the 32x32x16 A-fragment order -- element e = 0..7 of lane (m, hh) is k = kx_f32 + 16 s + 8 hh + e,
// element 2 d in the low half of dword d.  The power-of-two 2^sw puts max|W| of the split columns in [2^14, 2^15), so every lo of a weight
// above max|W| * 2^-17 is a normal f16 and hi + lo = W * 2^sw to 2^-22 relative.  The kernel stores h * 2^APE_C32_HSHIFT in the same
// split (|h| <= 1), so its accumulators hold 2^S times the gate pre-activations, S = sw + APE_C32_HSHIFT; it starts them at
// 2^S (b_ih + b_hh) and folds 2^-S into the gate constants.
// Returns S, or -1 when the layer cannot take the split: a non-finite weight, or a scale outside [0, 64] / f32 input columns that would
// overflow (the model then stays off this kernel).
static inline size_t wcl32s_elems(int H, int KXl) { return wcl32_elems(H, KXl); }
static inline int pack_c32_split(const float* w_ih, int in_l, const float* w_hh, int H, int KXl, int kx_f32, unsigned* out) {
    const WCat wcat{w_ih, in_l, w_hh, H, KXl};
    const int K = KXl + H;
    float wmax = 0.0f, xmax = 0.0f;
    for (int row = 0; row < 4 * H; ++row)
        for (int k = 0; k < K; ++k) {
            const float v = wcat(row, k);
            if (!std::isfinite(v)) return -1;
            if (k < kx_f32) xmax = std::max(xmax, std::fabs(v));
            else wmax = std::max(wmax, std::fabs(v));
        }
    int ex = 0;
    if (wmax > 0.0f) (void)std::frexp(wmax, &ex);          // wmax in [2^(ex-1), 2^ex)
    const int sw = (wmax > 0.0f) ? 15 - ex : 0;
    const int S = sw + APE_C32_HSHIFT;
    if (S < 0 || S > 64 || std::ldexp((double)xmax, S) >= 0x1p100) return -1;
    const int NG = kx_f32 / 8 + 2 * ((K - kx_f32) / 16);
    for (int mem = 0; mem < 8; ++mem)
        for (int w = 0; w < 4; ++w)
            for (int g = 0; g < NG; ++g)
                for (int lane = 0; lane < 64; ++lane) {
                    const int mcol = lane & 31, hh = lane >> 5;
                    const int row = (mcol >> 3) * H + mem * 32 + w * 8 + (mcol & 7);
                    unsigned* dst = out + ((((size_t)(mem * 4 + w) * NG) + g) * 64 + lane) * 4;
                    if (g < kx_f32 / 8) {
                        for (int j = 0; j < 4; ++j) {
                            const float v = std::ldexp(wcat(row, 8 * g + 4 * hh + j), S);
                            std::memcpy(&dst[j], &v, 4);
                        }
                        continue;
                    }
                    const int s = (g - kx_f32 / 8) / 2, lo = (g - kx_f32 / 8) & 1;
                    for (int d = 0; d < 4; ++d) {
                        unsigned short hw[2];
                        for (int e2 = 0; e2 < 2; ++e2) {
                            const float v = std::ldexp(wcat(row, kx_f32 + 16 * s + 8 * hh + 2 * d + e2), sw);     // exact: |v| < 2^15
                            const _Float16 hi = (_Float16)v;
                            const _Float16 part = lo ? (_Float16)(v - (float)hi) : hi;
                            std::memcpy(&hw[e2], &part, 2);
                        }
                        dst[d] = (unsigned)hw[0] | ((unsigned)hw[1] << 16);
                    }
                }
    return S;
}
