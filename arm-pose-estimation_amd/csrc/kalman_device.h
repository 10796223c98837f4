// Device functions shared by kalman.hip and kalman_bank.hip: the standard-normal draw behind the flipout perturbations and
// format_state (Box-Muller on Philox words), so that a bank frame's draws are those of a forward / format_state with the same seed.
#pragma once
#include "ape_internal.h"

namespace ape_kfdev {

__device__ __forceinline__ float u01(uint32_t x) { return ((float)(x >> 8) + 1.0f) * 5.9604644775390625e-08f; }   // (0, 1], 24 bits

// standard normal number `idx` of stream (tag, seed): Box-Muller on Philox words
__device__ __forceinline__ float philox_normal(unsigned idx, unsigned tag, unsigned long long seed) {
    uint32_t w[4];
    philox4x32(idx >> 2, tag, 0x4B414C4Du, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), w);
    const int pair = (idx >> 1) & 1;
    const float r = sqrtf(-2.0f * logf(u01(w[2 * pair])));
    const float a = 6.283185307179586f * (float)w[2 * pair + 1] * 2.3283064365386963e-10f;
    return (idx & 1) ? r * sinf(a) : r * cosf(a);
}

}  // namespace ape_kfdev
