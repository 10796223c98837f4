// Host-side plumbing shared by the stream banks (api_streams.hip, api_subset.hip, fk_streams.hip, kalman_bank.hip) and score.hip: the
// argument checks every bank entry repeats, the pinned descriptor ring of the staged frames and hand-overs, coherent pinned memory, and
// the completion words of a host frame.  Inline host functions only, no device code; errors go through ape_fail.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <atomic>
#include <vector>
#include "../../include/ape_hip.h"

// (ape_internal.h's declaration, repeated: this header also compiles on its own, in a host-only program that brings its own ape_fail)
int ape_fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));

// ---- argument checks; `what` names the entry in the message -------------------------------------------------------------------------
// a list of K stream indices of a bank of S: K in range, indices in range, distinct.  null_means_all: no list stands for all S streams
// in order, so K must be S; otherwise the caller has refused (or replaced) a NULL list before
inline int ape_check_stream_list(const char* what, const int32_t* streams_host, int32_t K, int32_t S, bool null_means_all) {
    if (K < 0 || K > S) return ape_fail(APE_ERR_INVALID_ARG, "%s: K=%d outside [0, S=%d]", what, K, S);
    if (!streams_host && null_means_all) {
        if (K != S) return ape_fail(APE_ERR_INVALID_ARG, "%s: no stream list: K=%d must be S=%d", what, K, S);
        return APE_OK;
    }
    std::vector<char> seen((size_t)S, 0);
    for (int j = 0; j < K; ++j) {
        const int s = streams_host[j];
        if (s < 0 || s >= S) return ape_fail(APE_ERR_INVALID_ARG, "%s: stream index %d (entry %d) outside [0, %d)", what, s, j, S);
        if (seen[s]) return ape_fail(APE_ERR_INVALID_ARG, "%s: stream %d listed twice", what, s);
        seen[s] = 1;
    }
    return APE_OK;
}

// the R recording starts of a replay or a scoring over F frames: starts[0] == 0, strictly rising, below F
inline int ape_check_segments(const char* what, int32_t F, const int32_t* seg_starts_host, int32_t R) {
    if (F < 1) return ape_fail(APE_ERR_INVALID_ARG, "%s: F=%d must be >= 1", what, F);
    if (R < 1 || R > F) return ape_fail(APE_ERR_INVALID_ARG, "%s: %d recording starts for %d frames (1 <= R <= F)", what, R, F);
    if (!seg_starts_host) return ape_fail(APE_ERR_INVALID_ARG, "%s: NULL seg_starts", what);
    if (seg_starts_host[0] != 0) return ape_fail(APE_ERR_INVALID_ARG, "%s: seg_starts[0] = %d, must be 0", what, seg_starts_host[0]);
    for (int i = 1; i < R; ++i)
        if (seg_starts_host[i] <= seg_starts_host[i - 1] || seg_starts_host[i] >= F)
            return ape_fail(APE_ERR_INVALID_ARG, "%s: seg_starts[%d] = %d (strictly rising, below F = %d)", what, i, seg_starts_host[i], F);
    return APE_OK;
}

// refuses a capturing stream (and fails when the query itself fails); why: what the entry stages per call, or nullptr for the blocking
// entries' own sentence
inline int ape_check_not_capturing(hipStream_t st, const char* what, const char* why) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    const hipError_t e = hipStreamIsCapturing(st, &cap);
    if (e != hipSuccess) return ape_fail(APE_ERR_HIP, "%s failed: %s", "hipStreamIsCapturing(st, &cap)", hipGetErrorString(e));
    if (cap == hipStreamCaptureStatusNone) return APE_OK;
    if (!why) return ape_fail(APE_ERR_INVALID_ARG, "%s: blocking call on a capturing stream", what);
    return ape_fail(APE_ERR_INVALID_ARG, "%s: the stream is capturing (%s)", what, why);
}

// ---- pinned descriptor ring ------------------------------------------------------------------------------------------------------------
// Frames and hand-overs go back to back with no host synchronisation, so the descriptors of a call are written into the next of
// APE_DESC_STAGES pinned slots (S descriptors each) and copied to the device on the call's stream; the event recorded behind the copy
// tells when the slot may be written again.  take() -> fill -> send().
#define APE_DESC_STAGES 8
struct ApeDescStage {
    char* slots = nullptr;                  // [APE_DESC_STAGES][slot_bytes]
    size_t slot_bytes = 0;
    hipEvent_t ev[APE_DESC_STAGES] = {};    // the newest copy out of each slot
    int next = 0;
    bool on() const { return slots != nullptr; }

    hipError_t alloc(int S, size_t elem_bytes) {
        slot_bytes = (size_t)S * elem_bytes;
        hipError_t e = hipHostMalloc((void**)&slots, APE_DESC_STAGES * slot_bytes, hipHostMallocDefault);
        for (int i = 0; i < APE_DESC_STAGES && e == hipSuccess; ++i) e = hipEventCreateWithFlags(&ev[i], hipEventDisableTiming);
        return e;
    }
    // the next slot, once the copy that last read it has completed
    void* take(hipError_t* e) {
        *e = hipEventSynchronize(ev[next]);
        return slots + (size_t)next * slot_bytes;
    }
    // the first `bytes` of the slot taken to `dev` on `st`; the ring moves on
    hipError_t send(void* dev, size_t bytes, hipStream_t st) {
        hipError_t e = hipMemcpyAsync(dev, slots + (size_t)next * slot_bytes, bytes, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipEventRecord(ev[next], st);
        if (e == hipSuccess) next = (next + 1) % APE_DESC_STAGES;
        return e;
    }
    void free() {
        for (hipEvent_t& v : ev)
            if (v) { (void)hipEventSynchronize(v); (void)hipEventDestroy(v); v = nullptr; }
        if (slots) (void)hipHostFree(slots);
        slots = nullptr;
    }
};

// ---- coherent pinned memory and the completion words of a host frame -----------------------------------------------------------------
// A host frame polls words the device writes into pinned memory and reads its output rows without a stream synchronisation: the buffers
// are allocated COHERENT (fine-grained) and mapped explicitly -- with hipHostMallocDefault that property hangs on the HIP_HOST_COHERENT
// environment variable, and non-coherent pinned memory shows the host a kernel's writes only at its end.
#define APE_PINNED (hipHostMallocCoherent | hipHostMallocMapped)

// a zero-filled coherent block on first use (*p still null), else nothing
template <typename T>
inline hipError_t ape_pinned_zeroed(T** p, size_t bytes) {
    if (*p) return hipSuccess;
    const hipError_t e = hipHostMalloc((void**)p, bytes, APE_PINNED);
    if (e == hipSuccess) memset((void*)*p, 0, bytes);
    return e;
}

// a coherent block of at least `need` bytes: kept while it is large enough, else freed and allocated anew (contents are not carried over)
// (hidden: an inline function the compiler keeps out of line would otherwise join the library's exported symbols)
__attribute__((visibility("hidden"))) inline hipError_t ape_pinned_grow(void** p, size_t* cap, size_t need) {
    if (need <= *cap) return hipSuccess;
    if (*p) {
        const hipError_t e = hipHostFree(*p);
        if (e != hipSuccess) return e;
        *p = nullptr; *cap = 0;
    }
    const hipError_t e = hipHostMalloc(p, need, APE_PINNED);
    if (e == hipSuccess) *cap = need;
    return e;
}

// the value the next frame's completion words take: never 0, which the fresh words hold
inline void ape_done_next(unsigned* val) {
    *val += 1;
    if (*val == 0) *val = 1;
}

// looks for `val` in all n words (written by the frame's last kernel behind its outputs): ~50 ms at the default bound, where a frame
// takes microseconds.  false: not all there -- the caller waits for the stream itself
inline bool ape_done_wait(const volatile unsigned* words, int n, unsigned val, long spins = 20000000L) {
    bool seen = false;
    for (long spin = 0; spin < spins && !seen; ++spin) {
        seen = true;
        for (int k = 0; k < n; ++k) seen = seen && words[k] == val;
        if (!seen) __builtin_ia32_pause();
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    return seen;
}
