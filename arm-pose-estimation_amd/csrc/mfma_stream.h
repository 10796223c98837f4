// The inline-asm primitives of the hand-scheduled LSTM / MLP kernels, one copy each: the gate non-linearities, the f32 MFMA statements with
// their drains, and the k-block spans that keep a dependent MFMA chain fed from LDS.  (The memory side -- descriptor, LDS-DMA, asm stores --
// is async_look.h.)
//
// hipcc sees an asm statement as a black box that is done when it ends.  It models neither the operand nor the result hazards of an MFMA
// written in asm, and tools/check_mfma_hazards.py scans the assembly of every kernel that uses these for what follows from that:
//   * RESULT: the compiler takes the accumulator for ready behind the statement.  It is read only behind a drain -- mfma_drain(), which
//     takes the accumulator as an in/out operand so that nothing that reads it can be scheduled above, or the `s_nop` that the LAST MFMA of
//     a section carries inside its own statement (mfma16_last): with the drain in a second statement the phi copies of a branch merge
//     landed between the two (lstm_cluster16.hip: the second row tile one k-step short, 1e-4).
//   * OPERANDS: a weight that does not fit the VGPR budget is an accumulation-register operand BY NAME ("a", AG = true).  Never let the
//     compiler park an operand there by itself: its v_accvgpr_read right in front of the MFMA is a VALU write -> SrcA read without the wait
//     states the hardware needs (lstm_cluster16.hip: the first row tile of the top layer off by 2e-3).
#pragma once
#include "ape_internal.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned u32x4 __attribute__((__vector_size__(4 * sizeof(unsigned))));

constexpr unsigned SPIN_LIMIT = 1u << 22;   // bounded polls (~seconds) before giving up

// sigmoid(v), or tanh(v) = 2 * sigmoid(2 v) - 1 on the g-gate lanes: one branch-free formula so that all 64 lanes (four different gates per
// 16-lane row) stay converged.  Hardware v_exp_f32 (2^x) and v_rcp_f32, both ~1 ulp: absolute error of the activation ~1e-7; the libm forms
// cost about 10x the instructions, a fifth of a step's time beside the MFMAs of lstm_tile16.hip
__device__ __forceinline__ float gate_act(float v, bool is_tanh) {
    const float e = __builtin_amdgcn_exp2f((is_tanh ? -2.885390081777927f : -1.4426950408889634f) * v);
    const float s = __builtin_amdgcn_rcpf(1.0f + e);
    return is_tanh ? 2.0f * s - 1.0f : s;
}
// the same two formulas where a lane knows its gate at compile time
__device__ __forceinline__ float sigm(float v) { return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.4426950408889634f * v)); }
__device__ __forceinline__ float tanh_(float v) { return 2.0f * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-2.885390081777927f * v)) - 1.0f; }

// v_mfma_f32_32x32x2_f32, weight operand (A) in the accumulator file (AG) or in an architectural VGPR; the accumulators are read only
// behind mfma_drain()
template <bool AG>
__device__ __forceinline__ void mfma32(f32x16& acc, float w, float a) {
    if constexpr (AG) asm volatile("v_mfma_f32_32x32x2_f32 %0, %1, %2, %0" : "+v"(acc) : "a"(w), "v"(a));
    else asm volatile("v_mfma_f32_32x32x2_f32 %0, %1, %2, %0" : "+v"(acc) : "v"(w), "v"(a));
}
__device__ __forceinline__ void mfma_drain(f32x16& acc) { asm volatile("s_nop 15\n\ts_nop 7" : "+v"(acc)); }

// NB k-blocks of 8: acc += W (registers w[w0 ...]) x activations (LDS, one ds_read_b128 per block: this lane's window, units 4 hh .. 4 hh + 3
// of the block; `stride` floats between blocks), fragments fetched two blocks ahead.  `mid(kb)` runs after the MFMAs of block kb (kb a
// constant after unrolling): the caller hangs exchange work there.
template <int NB, bool AG, int NW, typename Mid>
__device__ __forceinline__ void span32(f32x16& acc, const float* __restrict__ src, int stride, const float (&w)[NW], int w0, Mid&& mid) {
    f32x4 a0 = *reinterpret_cast<const f32x4*>(src);
    f32x4 a1 = (NB > 1) ? *reinterpret_cast<const f32x4*>(src + stride) : a0;
    f32x4 a2 = a1;
#pragma unroll
    for (int kb = 0; kb < NB; ++kb) {
        if (kb + 2 < NB) a2 = *reinterpret_cast<const f32x4*>(src + stride * (kb + 2));
#pragma unroll
        for (int j = 0; j < 4; ++j) mfma32<AG>(acc, w[w0 + 4 * kb + j], a0[j]);
        mid(kb);
        a0 = a1;
        a1 = a2;
    }
}

// v_mfma_f32_16x16x4_f32: A = a weight register (row lane & 15 = unit * 4 + gate), B = an activation (column lane & 15 = window of the row
// tile), k = lane >> 4; the accumulators are read only behind mfma16_last()
template <bool AG>
__device__ __forceinline__ void mfma16(f32x4& acc, float w, float a) {
    if constexpr (AG) asm volatile("v_mfma_f32_16x16x4_f32 %0, %1, %2, %0" : "+v"(acc) : "a"(w), "v"(a));
    else asm volatile("v_mfma_f32_16x16x4_f32 %0, %1, %2, %0" : "+v"(acc) : "v"(w), "v"(a));
}
// the last MFMA of a span that ends a section, with the drain in the SAME statement
template <bool AG>
__device__ __forceinline__ void mfma16_last(f32x4& acc, float w, float a) {
    if constexpr (AG) asm volatile("v_mfma_f32_16x16x4_f32 %0, %1, %2, %0\n\ts_nop 15" : "+v"(acc) : "a"(w), "v"(a));
    else asm volatile("v_mfma_f32_16x16x4_f32 %0, %1, %2, %0\n\ts_nop 15" : "+v"(acc) : "v"(w), "v"(a));
}

// NB k-blocks of 16: acc += W (registers w[w0 + 4 kb + j]) x activations (LDS: block kb at src + kb * stride, this lane's 16 bytes),
// fragments fetched one block ahead; mid(kb) behind block kb, fine(4 kb + j) behind every single MFMA.  DR: the span ends the section --
// its last MFMA drains.  (DR is a template argument and the caller branches AROUND whole spans: a branch merge between the last MFMA and
// its drain is where hipcc puts phi copies of the accumulator.)
template <int NB, bool AG, bool DR, int NW, typename Mid, typename Fine>
__device__ __forceinline__ void span16(f32x4& acc, const float* __restrict__ src, int stride, const float (&w)[NW], int w0, Mid&& mid, Fine&& fine) {
    f32x4 a0 = *reinterpret_cast<const f32x4*>(src);
    f32x4 a1 = a0;
#pragma unroll
    for (int kb = 0; kb < NB; ++kb) {
        if (kb + 1 < NB) a1 = *reinterpret_cast<const f32x4*>(src + stride * (kb + 1));
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (DR && kb == NB - 1 && j == 3) mfma16_last<AG>(acc, w[w0 + 4 * kb + j], a0[j]);
            else {
                mfma16<AG>(acc, w[w0 + 4 * kb + j], a0[j]);
                fine(4 * kb + j);
            }
        }
        mid(kb);
        a0 = a1;
    }
}
// the same span with nothing hung into it
template <int NB, bool AG, bool DR, int NW>
__device__ __forceinline__ void span16(f32x4& acc, const float* __restrict__ src, int stride, const float (&w)[NW], int w0) {
    span16<NB, AG, DR, NW>(acc, src, stride, w, w0, [](int) {}, [](int) {});
}
