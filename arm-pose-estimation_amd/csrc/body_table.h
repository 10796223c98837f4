// Per-stream body measurements of a bank: the host side shared by the three banks (api_streams.hip, fk_streams.hip,
// kalman_bank.hip).  Replaces, for S estimators at once, Estimator._body_measurements (reference estimate/estimator.py:57-68): every
// reference Estimator is built with its own bonemap, a bank keeps one row of nine float64 values per stream.
//
// A bank without a table (dev == nullptr) passes its uniform body by value in the kernel arguments, as ever.  The first set() allocates
// the device table, a pinned image of it and the host mirror, all initialised from the uniform body; every set() overwrites the listed
// rows of the mirror and copies the WHOLE image to the device on the caller's stream: one copy command whatever K, ordered between the
// frames enqueued before and after it, and the caller's buffer is free on return (the copy reads the pinned image, not the argument).
// The image is reused only once the copy that last read it has completed (set_bodies is a rare call: the wait is not on a frame's path).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <vector>

struct ApeBodyTable {
    double* dev = nullptr;       // [S,9] row-major, or (transposed) [9,S] component-major
    double* stage = nullptr;     // pinned image in the device layout
    hipEvent_t ev = nullptr;     // the newest copy out of `stage`
    std::vector<double> host;    // [S,9] mirror: what ape_*_get_bodies returns and the launchers of by-value forms read
    bool on() const { return dev != nullptr; }
};

inline void ape_body_table_free(ApeBodyTable& t) {
    if (t.ev) { (void)hipEventSynchronize(t.ev); (void)hipEventDestroy(t.ev); }
    if (t.dev) (void)hipFree(t.dev);
    if (t.stage) (void)hipHostFree(t.stage);
    t.dev = t.stage = nullptr; t.ev = nullptr;
    t.host.clear();
}

// K rows (streams == nullptr: rows 0 .. K-1) of vals [K,9] into the table of S streams; the arguments are checked by the caller
inline hipError_t ape_body_table_set(ApeBodyTable& t, int S, bool transposed, const double uniform[9], const int32_t* streams, int K,
                                     const double* vals, hipStream_t st) {
    const size_t bytes = (size_t)S * 9 * sizeof(double);
    if (!t.on()) {
        hipError_t e = hipMalloc((void**)&t.dev, bytes);
        if (e == hipSuccess) e = hipHostMalloc((void**)&t.stage, bytes, hipHostMallocDefault);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&t.ev, hipEventDisableTiming);
        if (e != hipSuccess) { ape_body_table_free(t); return e; }
        t.host.resize((size_t)S * 9);
        for (int s = 0; s < S; ++s) memcpy(&t.host[(size_t)s * 9], uniform, 9 * sizeof(double));
    }
    for (int j = 0; j < K; ++j) memcpy(&t.host[(size_t)(streams ? streams[j] : j) * 9], vals + (size_t)j * 9, 9 * sizeof(double));
    hipError_t e = hipEventSynchronize(t.ev);
    if (e != hipSuccess) return e;
    if (!transposed) memcpy(t.stage, t.host.data(), bytes);
    else
        for (int s = 0; s < S; ++s)
            for (int c = 0; c < 9; ++c) t.stage[(size_t)c * S + s] = t.host[(size_t)s * 9 + c];
    e = hipMemcpyAsync(t.dev, t.stage, bytes, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipEventRecord(t.ev, st);
    return e;
}

// the [S,9] mirror, or S copies of the uniform body before the first set()
inline void ape_body_table_get(const ApeBodyTable& t, int S, const double uniform[9], double* out) {
    if (t.on()) memcpy(out, t.host.data(), (size_t)S * 9 * sizeof(double));
    else
        for (int s = 0; s < S; ++s) memcpy(out + (size_t)s * 9, uniform, 9 * sizeof(double));
}
