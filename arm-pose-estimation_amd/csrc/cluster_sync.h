// The co-residency protocol of the cluster kernels, one copy of each step: who a workgroup is (class ticket), whether its
// cluster really shares an XCD (rendezvous), how a wave waits for its peers' flag words, and how a bounded spin gives up.  None of the
// give-up paths runs in a test -- they execute only when co-residency has already failed -- so that every kernel says the same thing here
// is their only protection.  Plain functions, included at file scope like mfma_stream.h; the workgroup's LDS control words are
// ctl[0] abort, [1] ticket, [2] last-out, [3] same XCD.
//
// The rule for moving these steps here was byte-identical device code in every build flavour (profiles/cluster_sync_header.md), and three
// things in the signatures are there for it.  They change nothing a caller sees; hipcc's scheduler and register allocator break ties by
// the order in which values first appear:
//   * `status` (and ape_same_xcd's `words`) is a REFERENCE to the caller's pointer.  The kernels pass `p.status`, a field of the kernel
//     argument: by value it would be loaded at the call, in front of the loop; by reference it is loaded where it is used, inside the loop,
//     as in the spelled-out copies.
//   * the word count is a template argument and the row (cluster) an argument of its own: the address is formed in here, inside the loop.
//   * ape_take_class_ticket leaves the readfirstlane of the ticket to its caller.
#pragma once
#include "ape_internal.h"
#include "mfma_stream.h"

// a wave gives up: the workgroup's abort flag and the model's sticky status word (ApeAbort; only the first code of a launch matters to the host)
__device__ __forceinline__ void ape_give_up(int* ctl, unsigned* const& status, unsigned code, int lane) {
    if (lane == 0) {
        ctl[0] = 1;
        __hip_atomic_store(status, code, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// the XCD (accelerator complex die) this wave runs on
__device__ __forceinline__ unsigned ape_xcc_id() {
    unsigned xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    return xcc & 0xFu;
}

// Arrival ticket within the workgroup's block-index class (`class_ticket`: 8 counters, one per 64-byte line), as every thread reads it
// behind the workgroup barrier in here.  Negative: the workgroup leaves at once -- the status word was set already (an earlier launch on
// this model aborted and skipped its self-cleaning), or the ticket lies outside the grid (then the word says so).
// (The caller tests the sign and makes the ticket uniform: `if (drawn < 0) return; ticket = readfirstlane(drawn)`.  With the readfirstlane
//  in here hipcc names the scalar registers of lstm_upper32.hip's whole steady state differently.)
__device__ __forceinline__ int ape_take_class_ticket(int* ctl, unsigned* const& status, unsigned* class_ticket, int cls, int tid) {
    if (tid == 0) {
        ctl[0] = 0;
        ctl[1] = -1;
        if (__hip_atomic_load(status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u) {
            const unsigned tk = __hip_atomic_fetch_add(class_ticket + cls * 16, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (tk < gridDim.x / 8) ctl[1] = (int)tk;
            else __hip_atomic_store(status, APE_ABORT_TICKET, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    __syncthreads();
    return ctl[1];
}

// One wave: poll the XCD words of the cluster's N members, words[cluster * N ...] (0x10 | XCC id, zero until written), until all are
// there, then ctl[3] = all of them name `my_xcc`.  Bounded; the caller's barrier and its look at ctl[0] follow.
// (the lane is added in front of the cluster's row: the order hipcc had given the spelled-out copies' address)
template <int N, int SLEEP, unsigned CODE>
__device__ __forceinline__ void ape_same_xcd(unsigned* const& words, int cluster, unsigned my_xcc, unsigned* const& status, int* ctl, int lane) {
    unsigned spins = 0, v = 0u;
    while (true) {
        v = 0x10u | my_xcc;
        if (lane < N) v = __hip_atomic_load(words + lane + cluster * N, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (__all((int)(v != 0u))) break;
        if (++spins > SPIN_LIMIT || __hip_atomic_load(status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) {
            ape_give_up(ctl, status, CODE, lane);
            break;
        }
        __builtin_amdgcn_s_sleep(SLEEP);
    }
    const int same = __all((int)((v & 0xFu) == my_xcc));
    if (lane == 0) ctl[3] = same;
}

// Every wave polls for itself: have all N words of row `row` of words[][N] (epochs, one per lane) reached `want`?  Bounded, and it ends
// when the status word is set (looked at every STATUS_EVERY-th spin, a power of two: a second dependent load per spin doubles what a
// late word costs).
template <int N, int SLEEP, unsigned STATUS_EVERY>
__device__ __forceinline__ void ape_wait_words(const unsigned* words, int row, unsigned want, unsigned* const& status, int* ctl, int lane) {
    unsigned spins = 0;
    while (true) {
        unsigned v = want;
        if (lane < N) v = __hip_atomic_load(words + row * N + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (__all((int)(v >= want))) return;
        if (++spins > SPIN_LIMIT || ((STATUS_EVERY == 1u || (spins & (STATUS_EVERY - 1u)) == 0u) &&
                                     __hip_atomic_load(status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u)) {
            ape_give_up(ctl, status, APE_ABORT_SPIN, lane);
            return;
        }
        __builtin_amdgcn_s_sleep(SLEEP);
    }
}

// workgroup barrier that waits for this wave's LDS traffic only (not for loads, stores or LDS-DMA in flight to memory)
__device__ __forceinline__ void ape_bar_lds() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
