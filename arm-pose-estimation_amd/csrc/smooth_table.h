// Per-stream smoothing lengths of a bank: the host side shared by the NN bank (api_streams.hip) and the forward-kinematics
// bank (fk_streams.hip).  Replaces, for S estimators at once, the `smooth` every reference Estimator is built with (estimate/estimator.py:45,
// max(1, smooth); the stack of :112-118 holds that many predictions): a bank keeps one int32 per stream.
//
// A bank without a table (dev == nullptr) runs the kernels it always ran, with the `smooth` it was created with -- from the first set() on
// that value is the CAPACITY.  The first set() allocates the device table, a pinned image and the host mirror, all initialised to the
// capacity; every set() overwrites the listed rows of the mirror and copies the WHOLE image to the device on the caller's stream: one copy
// command whatever K, ordered between the frames enqueued before and after it (body_table.h's scheme).  The host mirror is what the
// launchers take `n mod k` with: the listed streams are cold-started by the caller in the same call, so a frame enqueued earlier never
// meets a position computed with the new value.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <vector>
#include "bank_host.h"

struct ApeSmoothTable {
    int* dev = nullptr;          // [S]
    int* stage = nullptr;        // pinned image
    hipEvent_t ev = nullptr;     // the newest copy out of `stage`
    std::vector<int32_t> host;   // [S] mirror: what ape_*_get_smooths returns and the descriptors are built from
    bool on() const { return dev != nullptr; }
    // stream s's smoothing length in a bank of capacity `cap`
    int of(int s, int cap) const { return on() ? host[(size_t)s] : cap; }
};

inline void ape_smooth_table_free(ApeSmoothTable& t) {
    if (t.ev) { (void)hipEventSynchronize(t.ev); (void)hipEventDestroy(t.ev); }
    if (t.dev) (void)hipFree(t.dev);
    if (t.stage) (void)hipHostFree(t.stage);
    t.dev = t.stage = nullptr; t.ev = nullptr;
    t.host.clear();
}

// what both banks refuse before anything is written; `what` names the entry
inline int ape_smooth_table_check(const char* what, const void* bank, const int32_t* streams, int32_t K, int32_t S, const int32_t* vals, int cap) {
    if (!bank || !vals) return ape_fail(APE_ERR_INVALID_ARG, "%s: NULL argument", what);
    if (int rc = ape_check_stream_list(what, streams, K, S, true)) return rc;
    for (int j = 0; j < K; ++j)
        if (vals[j] < 1 || vals[j] > cap)
            return ape_fail(APE_ERR_INVALID_ARG, "%s: smooth %d (entry %d) outside [1, %d], the smooth the bank was created with", what, vals[j], j, cap);
    return APE_OK;
}

// K values (streams == nullptr: rows 0 .. K-1) into the table of S streams; the arguments are checked by the caller
inline hipError_t ape_smooth_table_set(ApeSmoothTable& t, int S, int cap, const int32_t* streams, int K, const int32_t* vals, hipStream_t st) {
    const size_t bytes = (size_t)S * sizeof(int);
    if (!t.on()) {
        hipError_t e = hipMalloc((void**)&t.dev, bytes);
        if (e == hipSuccess) e = hipHostMalloc((void**)&t.stage, bytes, hipHostMallocDefault);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&t.ev, hipEventDisableTiming);
        if (e != hipSuccess) { ape_smooth_table_free(t); return e; }
        t.host.assign((size_t)S, cap);
    }
    hipError_t e = hipEventSynchronize(t.ev);
    if (e != hipSuccess) return e;
    for (int j = 0; j < K; ++j) t.host[(size_t)(streams ? streams[j] : j)] = vals[j];
    memcpy(t.stage, t.host.data(), bytes);
    e = hipMemcpyAsync(t.dev, t.stage, bytes, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipEventRecord(t.ev, st);
    return e;
}

// the [S] mirror, or S copies of the capacity before the first set()
inline void ape_smooth_table_get(const ApeSmoothTable& t, int S, int cap, int32_t* out) {
    for (int s = 0; s < S; ++s) out[s] = t.of(s, cap);
}
