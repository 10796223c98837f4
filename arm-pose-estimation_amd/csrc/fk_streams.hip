// The estimator without a regressor (WatchPhoneUarm, reference estimate/watch_phone_uarm.py:10-108): a frame is the
// feature builder (parse_row), the two calibrated 6D columns of the features turned into quaternions, the smoothing stack
// (estimator.py:112-118) and the message (Estimator.msg_from_pred with est_to_ori_cal_larm_uarm, compose_msg.py:82-108).
//
// ape_fk_bank_kernel         one frame for K listed streams of a bank (lane per stream): parse, the row's two quaternions into the
//                            stream's ring slot (all `smooth` slots on a cold start), the ring reduced in stack order to the message
// ape_fk_replay_rows_kernel  every frame of recordings: the frame's two quaternions into an [F, 8] workspace, once
// ape_fk_replay_msg_kernel   ... and per frame the stack, row i = frame max(seg, f - smooth + 1 + i), to the message
//
// The ring keeps quaternions (8 doubles a row), not the 6D columns: a row's 6D -> quaternion chain runs once, with the same function on
// the same inputs, so the bits are those of recomputing it.  Lane per stream, not a workgroup per stream: one-lane waves of float64
// chains are issue-bound (stream_post_wide).  No co-residency: no journal, no recovery.
// float64 with separate roundings for a * b + c, like numpy: contraction is off in this file.
#include <cstring>
#include <new>
#include <vector>

#include "ape_internal.h"
#include "../../include/ape_hip.h"
#include "parse_device.h"
#include "stream_post_device.h"
#include "body_table.h"
#include "smooth_table.h"
#include "bank_host.h"

#pragma clang fp contract(off)

namespace {

using namespace ape_postdev;

constexpr int FK_BLOCK = 64;          // lanes = streams (frames); one wave per workgroup spreads the chains over the CUs
constexpr int FK_WIDTH = 55;          // APE_PARSE_WATCH_PHONE_UARM message

struct FkDesc { int stream, pos, cold, pad; };

struct FkBankParams {
    const float* rows;                // [K, 55]
    const FkDesc* desc;               // [K] or nullptr: lane j = stream j, uniform pos / cold
    double* ring;                     // [S, smooth, 8]
    void* out;                        // [K, 25]
    unsigned* done;                   // host frames: a word per lane written behind its message (nullptr: none)
    unsigned done_val;
    int K, smooth, pos, cold, big_endian;
    double body[9];
};

struct FkReplayParams {
    const float* rows;                // [F, 55]
    const int* seg_of;                // [F]
    double* ws;                       // [F, 8]
    void* out;                        // [F, 25]
    int F, smooth, big_endian;
    double body[9];
};

// raw message -> the row's lower-arm and upper-arm quaternions (watch_phone_uarm.py:64-108: features 13:19 and 32:38)
__device__ inline void row_quats(const float* src, int big_endian, double* q8) {
    float r[FK_WIDTH];
#pragma unroll
    for (int c = 0; c < FK_WIDTH; ++c) {
        float v = src[c];
        if (big_endian) v = __builtin_bit_cast(float, __builtin_bswap32(__builtin_bit_cast(unsigned, v)));
        r[c] = v;
    }
    double xx[38];
    ape_parsedev::parse_row(r, FK_WIDTH, APE_PARSE_WATCH_PHONE_UARM, xx);
    const Quat lq = six_drr_to_quat(xx + 13), uq = six_drr_to_quat(xx + 32);
    put_q(q8, lq);
    put_q(q8 + 4, uq);
}

// the stack (row i via `row(i)`, oldest first) -> message: for N > 1 the mean sequence of ape_replay_msg_kernel (row 0 times 1/N, every
// further row added with +-1/N by the strict `dot < 0.0` rule against row 0), for N == 1 est row 0 (estimate_joints.py:74-92)
template <typename Row>
__device__ inline void stack_msg(int N, Row row, const double* body, double* m) {
    const double* q0 = row(0);
    double out_q[3][4] = {}, orig_mean[9] = {}, e0[21] = {};
    if (N > 1) {
        const double wgt = 1.0 / (double)N;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const double r0 = q0[4 * q], r1 = q0[4 * q + 1], r2 = q0[4 * q + 2], r3 = q0[4 * q + 3];
            double a0 = r0 * wgt, a1 = r1 * wgt, a2 = r2 * wgt, a3 = r3 * wgt;
            for (int i = 1; i < N; ++i) {
                const double* qi = row(i) + 4 * q;
                const double d = fma(qi[3], r3, fma(qi[2], r2, fma(qi[1], r1, qi[0] * r0)));
                const double sg = d < 0.0 ? -wgt : wgt;
                a0 = a0 + qi[0] * sg; a1 = a1 + qi[1] * sg; a2 = a2 + qi[2] * sg; a3 = a3 + qi[3] * sg;
            }
            const double nrm = sqrt(a0 * a0 + a1 * a1 + a2 * a2 + a3 * a3);
            out_q[q][0] = a0 / nrm; out_q[q][1] = a1 / nrm; out_q[q][2] = a2 / nrm; out_q[q][3] = a3 / nrm;
        }
    } else {
        const Quat lq{q0[0], q0[1], q0[2], q0[3]}, uq{q0[4], q0[5], q0[6], q0[7]};
        const Vec3 lo = vadd(qrot(uq, Vec3{body[3], body[4], body[5]}), Vec3{body[6], body[7], body[8]});
        const Vec3 ho = vadd(qrot(lq, Vec3{body[0], body[1], body[2]}), lo);
        put_v(e0, ho); put_v(e0 + 3, lo); put_q(e0 + 6, lq); put_q(e0 + 10, uq);
    }
    finish_msg(APE_LAYOUT_ORI_CAL_LARM_UARM, N, out_q, orig_mean, e0, body, m);
}

// TAB (per-stream bodies): stream s takes bodies[c * S + s], c = 0 .. 8 -- the table is component-major [9,S], so that
// the 64 lanes of a lockstep wave read nine runs of 512 contiguous bytes (a row-major [S,9] would be nine 72-byte-strided gathers);
// indexed by the stream, never by the list position.  Else the uniform p.body.
template <typename TMsg, bool TAB = false>
__global__ __launch_bounds__(FK_BLOCK) void ape_fk_bank_kernel(const FkBankParams p, const double* __restrict__ bodies, const int S) {
    const int j = blockIdx.x * FK_BLOCK + threadIdx.x;
    if (j >= p.K) return;
    const int s = p.desc ? p.desc[j].stream : j;
    const int pos = p.desc ? p.desc[j].pos : p.pos;
    const bool cold = p.desc ? p.desc[j].cold != 0 : p.cold != 0;
    const int S8 = p.smooth * 8;
    double* ring = p.ring + (size_t)s * S8;
    double q8[8];
    row_quats(p.rows + (size_t)j * FK_WIDTH, p.big_endian, q8);
    for (int t = cold ? 0 : pos; t < (cold ? p.smooth : pos + 1); ++t)
#pragma unroll
        for (int c = 0; c < 8; ++c) ring[t * 8 + c] = q8[c];
    // stack row i (oldest first) sits in slot (pos + 1 + i) mod smooth: the newest in `pos`, on a cold start copies everywhere
    double m[25], own[9];
    if constexpr (TAB) {
#pragma unroll
        for (int c = 0; c < 9; ++c) own[c] = bodies[(size_t)c * S + s];
    }
    stack_msg(p.smooth, [&](int i) -> const double* { int t = pos + 1 + i; if (t >= p.smooth) t -= p.smooth; return ring + t * 8; },
              TAB ? own : p.body, m);
    TMsg* dst = static_cast<TMsg*>(p.out) + (size_t)j * 25;
#pragma unroll
    for (int c = 0; c < 25; ++c) dst[c] = (TMsg)m[c];
    if (p.done != nullptr) {                                   // host frames: the message first (system scope), then the word
        __threadfence_system();
        __hip_atomic_store(p.done + j, p.done_val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// The same frame for a bank with per-stream smoothing lengths: stream s stacks its last k = sm.smooths[s] rows instead
// of p.smooth -- the S estimators of the reference built with S values of `smooth` (estimator.py:45,112-118).  p.smooth stays the capacity
// and the ring's stride; the stream lives in slots 0 .. k-1.  Lockstep frames without descriptors take the slot from the count itself
// (sm.count mod k: not uniform over the streams); descriptors carry a slot taken mod k on the host.  A kernel of its own (the frame is
// thirty lines): the kernel above keeps its instruction stream.
template <typename TMsg, bool TAB = false>
__global__ __launch_bounds__(FK_BLOCK) void ape_fk_bank_smooths_kernel(const FkBankParams p, const double* __restrict__ bodies, const int S,
                                                                       const SmoothArgs sm) {
    const int j = blockIdx.x * FK_BLOCK + threadIdx.x;
    if (j >= p.K) return;
    const int s = p.desc ? p.desc[j].stream : j;
    const int k = sm.smooths[s];
    const int pos = p.desc ? p.desc[j].pos : (int)(sm.count % (unsigned long long)k);
    const bool cold = p.desc ? p.desc[j].cold != 0 : p.cold != 0;
    double* ring = p.ring + (size_t)s * (p.smooth * 8);
    double q8[8];
    row_quats(p.rows + (size_t)j * FK_WIDTH, p.big_endian, q8);
    for (int t = cold ? 0 : pos; t < (cold ? k : pos + 1); ++t)
#pragma unroll
        for (int c = 0; c < 8; ++c) ring[t * 8 + c] = q8[c];
    double m[25], own[9];
    if constexpr (TAB) {
#pragma unroll
        for (int c = 0; c < 9; ++c) own[c] = bodies[(size_t)c * S + s];
    }
    stack_msg(k, [&](int i) -> const double* { int t = pos + 1 + i; if (t >= k) t -= k; return ring + t * 8; }, TAB ? own : p.body, m);
    TMsg* dst = static_cast<TMsg*>(p.out) + (size_t)j * 25;
#pragma unroll
    for (int c = 0; c < 25; ++c) dst[c] = (TMsg)m[c];
    if (p.done != nullptr) {
        __threadfence_system();
        __hip_atomic_store(p.done + j, p.done_val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

__global__ __launch_bounds__(FK_BLOCK) void ape_fk_replay_rows_kernel(const FkReplayParams p) {
    const int f = blockIdx.x * FK_BLOCK + threadIdx.x;
    if (f >= p.F) return;
    row_quats(p.rows + (size_t)f * FK_WIDTH, p.big_endian, p.ws + (size_t)f * 8);
}

// TAB (ape_fk_replay_bodies): the frame's body is row rec_of[f] of bodies [R,9] -- neighbouring lanes mostly share it
template <typename TMsg, bool TAB = false>
__global__ __launch_bounds__(FK_BLOCK) void ape_fk_replay_msg_kernel(const FkReplayParams p, const double* __restrict__ bodies,
                                                                     const int* __restrict__ rec_of) {
    const int f = blockIdx.x * FK_BLOCK + threadIdx.x;
    if (f >= p.F) return;
    const int seg = p.seg_of[f];
    double m[25];
    stack_msg(p.smooth, [&](int i) -> const double* { int h = f - p.smooth + 1 + i; if (h < seg) h = seg; return p.ws + (size_t)h * 8; },
              TAB ? bodies + 9 * (size_t)rec_of[f] : p.body, m);
    TMsg* dst = static_cast<TMsg*>(p.out) + (size_t)f * 25;
#pragma unroll
    for (int c = 0; c < 25; ++c) dst[c] = (TMsg)m[c];
}

// State hand-over: the stacks of K listed streams between the ring and the canonical records [K][smooth][8] f64, oldest
// row first.  One thread per 16 bytes (a pair of doubles) of a record: record row i lives in ring slot (desc.pos + i) mod smooth, desc.pos
// = the slot of the stream's oldest row; desc.cold: the stream has no stack -- zeros out, nothing in.
typedef double f64x2 __attribute__((ext_vector_type(2)));
template <bool IMPORT>
__global__ __launch_bounds__(FK_BLOCK) void ape_fk_state_kernel(double* __restrict__ ring, double* __restrict__ state,
                                                                const FkDesc* __restrict__ desc, const int K, const int smooth) {
    const int units = smooth * 4;
    const long long idx = (long long)blockIdx.x * FK_BLOCK + threadIdx.x;
    if (idx >= (long long)K * units) return;
    const int j = (int)(idx / units), u = (int)(idx - (long long)j * units);
    const FkDesc d = desc[j];
    const int i = u >> 2, c = (u & 3) * 2;
    int slot = d.pos + i;
    if (slot >= smooth) slot -= smooth;
    f64x2* r = reinterpret_cast<f64x2*>(ring + ((size_t)d.stream * smooth + slot) * 8 + c);
    f64x2* s = reinterpret_cast<f64x2*>(state) + idx;
    if constexpr (IMPORT) {
        if (!d.cold) *r = *s;
    } else {
        const f64x2 zero = {0.0, 0.0};
        *s = d.cold ? zero : *r;
    }
}

// ... of a bank with per-stream smoothing lengths: the record keeps the capacity's [smooth][8], stream s's k = smooths[s] rows oldest
// first and zeros behind them; in the ring the stream lives in slots 0 .. k-1 (desc.pos was taken mod k)
template <bool IMPORT>
__global__ __launch_bounds__(FK_BLOCK) void ape_fk_state_smooths_kernel(double* __restrict__ ring, double* __restrict__ state,
                                                                        const FkDesc* __restrict__ desc, const int K, const int smooth,
                                                                        const int* __restrict__ smooths) {
    const int units = smooth * 4;
    const long long idx = (long long)blockIdx.x * FK_BLOCK + threadIdx.x;
    if (idx >= (long long)K * units) return;
    const int j = (int)(idx / units), u = (int)(idx - (long long)j * units);
    const FkDesc d = desc[j];
    const int k = smooths[d.stream];
    const int i = u >> 2, c = (u & 3) * 2;
    int slot = d.pos + i;
    if (slot >= k) slot -= k;
    const bool live = i < k && !d.cold;
    f64x2* r = reinterpret_cast<f64x2*>(ring + ((size_t)d.stream * smooth + (live ? slot : 0)) * 8 + c);
    f64x2* s = reinterpret_cast<f64x2*>(state) + idx;
    if constexpr (IMPORT) {
        if (live) *r = *s;
    } else {
        const f64x2 zero = {0.0, 0.0};
        *s = live ? *r : zero;
    }
}

unsigned blocks_for(long long n) { return (unsigned)((n + FK_BLOCK - 1) / FK_BLOCK); }

int check_device(int32_t device, const char* what) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0) {
        (void)hipGetLastError();
        return ape_fail(APE_ERR_NO_DEVICE, "%s: no HIP device visible: libape_hip has no CPU fallback", what);
    }
    if (device < 0 || device >= n) return ape_fail(APE_ERR_INVALID_ARG, "%s: device %d of %d", what, device, n);
    hipDeviceProp_t prop;
    APE_TRY(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return ape_fail(APE_ERR_NO_DEVICE, "%s: device %d is %s; this library is built for gfx950 only", what, device, prop.gcnArchName);
    return APE_OK;
}

int check_kind(int32_t kind, const char* what) {
    if ((kind & ~APE_PARSE_BIG_ENDIAN) != APE_PARSE_WATCH_PHONE_UARM)
        return ape_fail(APE_ERR_INVALID_ARG, "%s: kind %d: the forward-kinematics estimator reads APE_PARSE_WATCH_PHONE_UARM rows only", what, kind);
    return APE_OK;
}

int check_capture(hipStream_t st, const char* what) {
    return ape_check_not_capturing(st, what, "ring positions and stream lists are staged per call");
}

template <typename K32, typename K64, typename... Args>
hipError_t launch_typed(K32 k32, K64 k64, int out_dtype, long long n, hipStream_t st, Args... args) {
    if (out_dtype == APE_F32) hipLaunchKernelGGL(k32, dim3(blocks_for(n)), dim3(FK_BLOCK), 0, st, args...);
    else hipLaunchKernelGGL(k64, dim3(blocks_for(n)), dim3(FK_BLOCK), 0, st, args...);
    return hipGetLastError();
}

}  // namespace

// ---- the bank: ring on the device, per-stream row counts since the cold start on the host --------------------------------------
struct ape_fk_bank {
    int S = 0, smooth = 1, device = 0;
    double body[9] = {};
    double* ring = nullptr;            // [S, smooth, 8]
    FkDesc* desc = nullptr;            // [S] device descriptors of the current frame
    // uniform: every stream has seen `ucount` rows since its cold start (lockstep history) -- frames then carry pos / cold as arguments
    bool uniform = true;
    long long ucount = 0;
    std::vector<long long> cnt;        // per stream, once the history is not uniform
    ApeDescStage stage;                // pinned slots of S descriptors (bank_host.h)
    float* h_rows = nullptr;           // frame_host: pinned rows, message words and completion words
    void* h_out = nullptr;
    unsigned* h_done = nullptr;
    unsigned done_val = 0;
    char* hs_block = nullptr;          // frame_subset_host: ONE pinned block of completion words, descriptors and rows
    ApeBodyTable bodies;               // per-stream bodies, component-major [9,S] on the device (off until ape_fk_bank_set_bodies)
    ApeSmoothTable smooths;            // per-stream smoothing lengths [S] (off until ape_fk_bank_set_smooths: `smooth` is then the capacity)
    int smooth_of(int s) const { return smooths.of(s, smooth); }
};

namespace {

void bank_free(ape_fk_bank* b) {
    ape_body_table_free(b->bodies);
    ape_smooth_table_free(b->smooths);
    if (b->ring) (void)hipFree(b->ring);
    if (b->desc) (void)hipFree(b->desc);
    b->stage.free();
    if (b->h_rows) (void)hipHostFree(b->h_rows);
    if (b->h_out) (void)hipHostFree(b->h_out);
    if (b->h_done) (void)hipHostFree(b->h_done);
    if (b->hs_block) (void)hipHostFree(b->hs_block);
    delete b;
}

void leave_uniform(ape_fk_bank* b) {
    if (!b->uniform) return;
    b->cnt.assign((size_t)b->S, b->ucount);
    b->uniform = false;
}

// one frame for K streams (streams_host nullptr: all S in order) on `st`; the counters move on once the launch is enqueued
// pinned_desc (host subset frames): the descriptors are written there and the kernel reads them from there -- no copy, no event
int bank_frame(ape_fk_bank* b, int32_t kind, const float* rows, const int32_t* streams_host, int32_t K, void* out, int32_t out_dtype,
               hipStream_t st, unsigned* done, const char* what, FkDesc* pinned_desc = nullptr) {
    FkBankParams p{};
    p.rows = rows; p.ring = b->ring; p.out = out; p.K = K; p.smooth = b->smooth;
    p.big_endian = (kind & APE_PARSE_BIG_ENDIAN) ? 1 : 0;
    p.done = done; p.done_val = b->done_val;
    memcpy(p.body, b->body, sizeof(p.body));
    if (!streams_host && b->uniform) {
        p.desc = nullptr;
        p.pos = (int)(b->ucount % b->smooth); p.cold = b->ucount == 0 ? 1 : 0;      // (a table bank: the kernel takes ucount mod k itself)
    } else {
        if (streams_host) leave_uniform(b);
        // the descriptors into the next pinned slot -- once the copy that last read it has completed
        hipError_t slot_wait = hipSuccess;
        FkDesc* h = pinned_desc ? pinned_desc : static_cast<FkDesc*>(b->stage.take(&slot_wait));
        APE_TRY(slot_wait);
        for (int j = 0; j < K; ++j) {
            const int s = streams_host ? streams_host[j] : j;
            const long long c = b->cnt[s];
            h[j] = FkDesc{s, (int)(c % b->smooth_of(s)), c == 0 ? 1 : 0, 0};
        }
        if (pinned_desc) p.desc = pinned_desc;
        else {
            APE_TRY(b->stage.send(b->desc, (size_t)K * sizeof(FkDesc), st));
            p.desc = b->desc;
        }
    }
    const double* const none = nullptr;
    const SmoothArgs sm{b->smooths.dev, (unsigned long long)b->ucount};
    const hipError_t e = b->smooths.on()
                             ? (b->bodies.on() ? launch_typed(ape_fk_bank_smooths_kernel<float, true>, ape_fk_bank_smooths_kernel<double, true>, out_dtype, K, st, p,
                                                              (const double*)b->bodies.dev, b->S, sm)
                                               : launch_typed(ape_fk_bank_smooths_kernel<float, false>, ape_fk_bank_smooths_kernel<double, false>, out_dtype, K, st, p,
                                                              none, 0, sm))
                         : b->bodies.on() ? launch_typed(ape_fk_bank_kernel<float, true>, ape_fk_bank_kernel<double, true>, out_dtype, K, st, p, (const double*)b->bodies.dev, b->S)
                                        : launch_typed(ape_fk_bank_kernel<float, false>, ape_fk_bank_kernel<double, false>, out_dtype, K, st, p, none, 0);
    if (e != hipSuccess) return ape_fail(APE_ERR_HIP, "%s: launch failed: %s", what, hipGetErrorString(e));
    if (p.desc == nullptr) b->ucount += 1;
    else if (streams_host) for (int j = 0; j < K; ++j) b->cnt[streams_host[j]] += 1;
    else for (int j = 0; j < K; ++j) b->cnt[j] += 1;
    return APE_OK;
}

}  // namespace

int ape_fk_bank_create(int32_t n_streams, int32_t smooth, const double body9[9], int32_t device, ape_fk_bank_t** out) {
    if (!out || !body9) return ape_fail(APE_ERR_INVALID_ARG, "fk_bank_create: NULL argument");
    *out = nullptr;
    if (n_streams < 1) return ape_fail(APE_ERR_INVALID_ARG, "fk_bank_create: n_streams=%d must be >= 1", n_streams);
    if (smooth < 1) smooth = 1;                                 // estimator.py:45: max(1, smooth)
    if (smooth > 64) return ape_fail(APE_ERR_UNSUPPORTED, "fk_bank_create: smooth %d outside 1..64", smooth);
    if (int rc = check_device(device, "fk_bank_create")) return rc;
    APE_TRY(hipSetDevice(device));
    ape_fk_bank* b = new (std::nothrow) ape_fk_bank();
    if (!b) return ape_fail(APE_ERR_HIP, "fk_bank_create: out of host memory");
    b->S = n_streams; b->smooth = smooth; b->device = device;
    memcpy(b->body, body9, sizeof(b->body));
    hipError_t e = hipMalloc((void**)&b->ring, (size_t)n_streams * smooth * 8 * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void**)&b->desc, (size_t)n_streams * sizeof(FkDesc));
    if (e == hipSuccess) e = b->stage.alloc(n_streams, sizeof(FkDesc));
    if (e != hipSuccess) {
        bank_free(b);
        return ape_fail(APE_ERR_HIP, "fk_bank_create: allocation failed: %s", hipGetErrorString(e));
    }
    *out = b;
    return APE_OK;
}

int ape_fk_bank_destroy(ape_fk_bank_t* b) {
    if (!b) return APE_OK;
    (void)hipSetDevice(b->device);
    (void)hipDeviceSynchronize();          // frames may still read the ring and the staged descriptors
    bank_free(b);
    return APE_OK;
}

int ape_fk_bank_reset(ape_fk_bank_t* b) {
    if (!b) return ape_fail(APE_ERR_INVALID_ARG, "fk_bank_reset: NULL bank");
    b->uniform = true;
    b->ucount = 0;
    b->cnt.clear();
    return APE_OK;
}

int ape_fk_bank_reset_subset(ape_fk_bank_t* b, const int32_t* streams_host, int32_t K) {
    if (!b || !streams_host) return ape_fail(APE_ERR_INVALID_ARG, "fk_bank_reset_subset: NULL argument");
    if (int rc = ape_check_stream_list("fk_bank_reset_subset", streams_host, K, b->S, true)) return rc;
    if (K == 0) return APE_OK;
    leave_uniform(b);
    for (int j = 0; j < K; ++j) b->cnt[streams_host[j]] = 0;
    return APE_OK;
}

int ape_fk_bank_frame(ape_fk_bank_t* b, int32_t kind, const float* rows_dev, const int32_t* streams_host, int32_t K, void* out_dev,
                      int32_t out_dtype, void* stream) {
    if (!b || !rows_dev || !out_dev) return ape_fail(APE_ERR_INVALID_ARG, "fk_bank_frame: NULL argument");
    if (int rc = check_kind(kind, "fk_bank_frame")) return rc;
    if (out_dtype != APE_F32 && out_dtype != APE_F64) return ape_fail(APE_ERR_INVALID_ARG, "fk_bank_frame: unknown dtype selector");
    if (int rc = ape_check_stream_list("fk_bank_frame", streams_host, K, b->S, true)) return rc;
    APE_TRY(hipSetDevice(b->device));
    const hipStream_t st = (hipStream_t)stream;
    if (int rc = check_capture(st, "fk_bank_frame")) return rc;
    if (K == 0) return APE_OK;
    return bank_frame(b, kind, rows_dev, streams_host, K, out_dev, out_dtype, st, nullptr, "fk_bank_frame");
}

int ape_fk_bank_frame_host(ape_fk_bank_t* b, int32_t kind, const float* rows_host, void* out_host, int32_t out_dtype, void* stream) {
    if (!b || !rows_host || !out_host) return ape_fail(APE_ERR_INVALID_ARG, "fk_bank_frame_host: NULL argument");
    if (int rc = check_kind(kind, "fk_bank_frame_host")) return rc;
    if (out_dtype != APE_F32 && out_dtype != APE_F64) return ape_fail(APE_ERR_INVALID_ARG, "fk_bank_frame_host: unknown dtype selector");
    APE_TRY(hipSetDevice(b->device));                         // (the consumer thread of an estimator starts on device 0)
    const hipStream_t st = (hipStream_t)stream;
    if (int rc = check_capture(st, "fk_bank_frame_host")) return rc;
    const size_t rows_bytes = (size_t)b->S * FK_WIDTH * sizeof(float);
    const size_t out_bytes = (size_t)b->S * 25 * sizeof(double);
    // the kernel reads the rows from and writes the messages to pinned host memory; up to 64 streams it writes a word per stream
    // behind its message, and the host takes the frame when all are there instead of waiting for the stream (as ape_streams_frame_host)
    if (!b->h_rows) APE_TRY(hipHostMalloc((void**)&b->h_rows, rows_bytes, APE_PINNED));
    if (!b->h_out) APE_TRY(hipHostMalloc(&b->h_out, out_bytes, APE_PINNED));
    if (b->S <= 64) APE_TRY(ape_pinned_zeroed(&b->h_done, 64 * sizeof(unsigned)));
    ape_done_next(&b->done_val);
    memcpy(b->h_rows, rows_host, rows_bytes);
    if (int rc = bank_frame(b, kind, b->h_rows, nullptr, b->S, b->h_out, out_dtype, st, b->h_done, "fk_bank_frame_host")) return rc;
    if (!(b->h_done && ape_done_wait(b->h_done, b->S, b->done_val))) APE_TRY(hipStreamSynchronize(st));
    memcpy(out_host, b->h_out, (size_t)b->S * 25 * (out_dtype == APE_F64 ? sizeof(double) : sizeof(float)));
    return APE_OK;
}

// Host subset frame: the frame is ONE kernel, so the pinned block is all it reads -- rows and descriptors -- and all
// it writes: the messages and, for K <= 64, a completion word per entry behind each.  Nothing runs behind that kernel, so the
// descriptors need not land in b->desc.  Layout of the block: [64] words, [S] descriptors, [S, 55] rows; messages in h_out.
int ape_fk_bank_frame_subset_host(ape_fk_bank_t* b, int32_t kind, const float* rows_host, const int32_t* streams_host, int32_t K,
                                  void* out_host, int32_t out_dtype, void* stream) {
    if (!b || !rows_host || !out_host) return ape_fail(APE_ERR_INVALID_ARG, "fk_bank_frame_subset_host: NULL argument");
    if (int rc = check_kind(kind, "fk_bank_frame_subset_host")) return rc;
    if (out_dtype != APE_F32 && out_dtype != APE_F64) return ape_fail(APE_ERR_INVALID_ARG, "fk_bank_frame_subset_host: unknown dtype selector");
    if (int rc = ape_check_stream_list("fk_bank_frame_subset_host", streams_host, K, b->S, true)) return rc;
    APE_TRY(hipSetDevice(b->device));
    const hipStream_t st = (hipStream_t)stream;
    if (int rc = check_capture(st, "fk_bank_frame_subset_host")) return rc;
    if (K == 0) return APE_OK;
    APE_TRY(ape_pinned_zeroed(&b->hs_block, 64 * sizeof(unsigned) + (size_t)b->S * sizeof(FkDesc) + (size_t)b->S * FK_WIDTH * sizeof(float)));
    if (!b->h_out) APE_TRY(hipHostMalloc(&b->h_out, (size_t)b->S * 25 * sizeof(double), APE_PINNED));
    unsigned* const h_done = reinterpret_cast<unsigned*>(b->hs_block);
    FkDesc* const h_desc = reinterpret_cast<FkDesc*>(b->hs_block + 64 * sizeof(unsigned));
    float* const h_rows = reinterpret_cast<float*>(b->hs_block + 64 * sizeof(unsigned) + (size_t)b->S * sizeof(FkDesc));
    const bool words = K <= 64;
    ape_done_next(&b->done_val);
    memcpy(h_rows, rows_host, (size_t)K * FK_WIDTH * sizeof(float));
    if (int rc = bank_frame(b, kind, h_rows, streams_host, K, b->h_out, out_dtype, st, words ? h_done : nullptr, "fk_bank_frame_subset_host", h_desc))
        return rc;
    if (!(words && ape_done_wait(h_done, K, b->done_val))) APE_TRY(hipStreamSynchronize(st));
    memcpy(out_host, b->h_out, (size_t)K * 25 * (out_dtype == APE_F64 ? sizeof(double) : sizeof(float)));
    return APE_OK;
}

int ape_fk_bank_set_bodies(ape_fk_bank_t* b, const int32_t* streams_host, int32_t K, const double* body9s_host, void* stream) {
    if (!b || !body9s_host) return ape_fail(APE_ERR_INVALID_ARG, "fk_bank_set_bodies: NULL argument");
    if (int rc = ape_check_stream_list("fk_bank_set_bodies", streams_host, K, b->S, true)) return rc;
    APE_TRY(hipSetDevice(b->device));
    const hipStream_t st = (hipStream_t)stream;
    if (int rc = check_capture(st, "fk_bank_set_bodies")) return rc;
    APE_TRY(ape_body_table_set(b->bodies, b->S, true, b->body, streams_host, K, body9s_host, st));
    return APE_OK;
}

// per-stream smoothing lengths (semantics at ape_streams_set_smooths): a cold start of the listed streams
int ape_fk_bank_set_smooths(ape_fk_bank_t* b, const int32_t* streams_host, int32_t K, const int32_t* smooths_host, void* stream) {
    if (int rc = ape_smooth_table_check("fk_bank_set_smooths", b, streams_host, K, b ? b->S : 0, smooths_host, b ? b->smooth : 0)) return rc;
    APE_TRY(hipSetDevice(b->device));
    const hipStream_t st = (hipStream_t)stream;
    if (int rc = check_capture(st, "fk_bank_set_smooths")) return rc;
    APE_TRY(ape_smooth_table_set(b->smooths, b->S, b->smooth, streams_host, K, smooths_host, st));
    if (!streams_host) return ape_fk_bank_reset(b);
    return ape_fk_bank_reset_subset(b, streams_host, K);
}

int ape_fk_bank_get_smooths(ape_fk_bank_t* b, int32_t* out_host) {
    if (!b || !out_host) return ape_fail(APE_ERR_INVALID_ARG, "fk_bank_get_smooths: NULL argument");
    ape_smooth_table_get(b->smooths, b->S, b->smooth, out_host);
    return APE_OK;
}

int ape_fk_bank_get_bodies(ape_fk_bank_t* b, double* out_host) {
    if (!b || !out_host) return ape_fail(APE_ERR_INVALID_ARG, "fk_bank_get_bodies: NULL argument");
    ape_body_table_get(b->bodies, b->S, b->body, out_host);
    return APE_OK;
}

// ---- state hand-over: the bank's record of a stream is its stack alone, [smooth][8] f64 ---------------------------
namespace {

void fk_state_desc_of(const ape_fk_bank* b, ape_stream_state_desc_t* d) {
    d->version = APE_STATE_VERSION;
    d->T = 0; d->I = 0; d->smooth = b->smooth; d->n_mc = 1; d->O = 8;
    d->words_per_stream = 16 * b->smooth;
}

// descriptors through the next pinned slot (as bank_frame), then the one launch; fill(stream) -> {oldest slot, cold}
template <bool IMPORT, typename Fill>
int fk_state_launch(ape_fk_bank* b, const int32_t* streams_host, int32_t K, double* state, hipStream_t st, const char* what, Fill fill) {
    hipError_t slot_wait;
    FkDesc* h = static_cast<FkDesc*>(b->stage.take(&slot_wait));
    APE_TRY(slot_wait);
    for (int j = 0; j < K; ++j) h[j] = fill(j, streams_host[j]);
    APE_TRY(b->stage.send(b->desc, (size_t)K * sizeof(FkDesc), st));
    if (b->smooths.on())
        hipLaunchKernelGGL(ape_fk_state_smooths_kernel<IMPORT>, dim3(blocks_for((long long)K * b->smooth * 4)), dim3(FK_BLOCK), 0, st, b->ring, state,
                           (const FkDesc*)b->desc, (int)K, b->smooth, (const int*)b->smooths.dev);
    else
    hipLaunchKernelGGL(ape_fk_state_kernel<IMPORT>, dim3(blocks_for((long long)K * b->smooth * 4)), dim3(FK_BLOCK), 0, st, b->ring, state,
                       (const FkDesc*)b->desc, (int)K, b->smooth);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return ape_fail(APE_ERR_HIP, "%s: launch failed: %s", what, hipGetErrorString(e));
    return APE_OK;
}

int fk_state_check_call(ape_fk_bank* b, const int32_t* streams_host, int32_t K, const void* state_dev, const void* warm_host, hipStream_t st,
                        const char* what) {
    if (!b || !streams_host || !state_dev || !warm_host) return ape_fail(APE_ERR_INVALID_ARG, "%s: NULL argument", what);
    if (int rc = ape_check_stream_list(what, streams_host, K, b->S, true)) return rc;
    if (((uintptr_t)state_dev & 15u) != 0) return ape_fail(APE_ERR_INVALID_ARG, "%s: state_dev must be 16-byte aligned", what);
    APE_TRY(hipSetDevice(b->device));
    return check_capture(st, what);
}

}  // namespace

int ape_fk_bank_state_desc(ape_fk_bank_t* b, ape_stream_state_desc_t* out) {
    if (!b || !out) return ape_fail(APE_ERR_INVALID_ARG, "fk_bank_state_desc: NULL argument");
    fk_state_desc_of(b, out);
    return APE_OK;
}

int ape_fk_bank_export(ape_fk_bank_t* b, const int32_t* streams_host, int32_t K, void* state_dev, uint8_t* warm_host, void* stream) {
    const hipStream_t st = (hipStream_t)stream;
    if (int rc = fk_state_check_call(b, streams_host, K, state_dev, warm_host, st, "fk_bank_export")) return rc;
    if (K == 0) return APE_OK;
    // read-only: a uniform bank stays uniform.  No window: a stream that has seen a row has both bits set
    return fk_state_launch<false>(b, streams_host, K, (double*)state_dev, st, "fk_bank_export", [&](int j, int s) {
        const long long c = b->uniform ? b->ucount : b->cnt[s];
        warm_host[j] = c > 0 ? (uint8_t)(APE_STATE_WINDOW_WARM | APE_STATE_STACK_WARM) : (uint8_t)0;
        return FkDesc{s, (int)(c % b->smooth_of(s)), c == 0 ? 1 : 0, 0};
    });
}

int ape_fk_bank_import(ape_fk_bank_t* b, const ape_stream_state_desc_t* desc, const int32_t* streams_host, int32_t K,
                       const void* state_dev, const uint8_t* warm_host, void* stream) {
    const hipStream_t st = (hipStream_t)stream;
    if (!desc) return ape_fail(APE_ERR_INVALID_ARG, "fk_bank_import: NULL argument");
    if (int rc = fk_state_check_call(b, streams_host, K, state_dev, warm_host, st, "fk_bank_import")) return rc;
    ape_stream_state_desc_t own;
    fk_state_desc_of(b, &own);
    if (desc->version != own.version || desc->T != own.T || desc->I != own.I || desc->smooth != own.smooth || desc->n_mc != own.n_mc ||
        desc->O != own.O || desc->words_per_stream != own.words_per_stream)
        return ape_fail(APE_ERR_INVALID_ARG, "fk_bank_import: the records are {v%d T=%d I=%d smooth=%d n_mc=%d O=%d words=%d}, the bank's {v%d T=0 I=0 smooth=%d n_mc=1 O=8 words=%d}",
                     desc->version, desc->T, desc->I, desc->smooth, desc->n_mc, desc->O, desc->words_per_stream, own.version, own.smooth,
                     own.words_per_stream);
    if (K == 0) return APE_OK;
    // a stream needs both bits to carry a stack (the record has no window); time order = slot order, the count at `smooth`
    auto warm = [&](int j) { return (warm_host[j] & APE_STATE_STACK_WARM) != 0 && (warm_host[j] & APE_STATE_WINDOW_WARM) != 0; };
    if (int rc = fk_state_launch<true>(b, streams_host, K, (double*)const_cast<void*>(state_dev), st, "fk_bank_import",
                                       [&](int j, int s) { return FkDesc{s, 0, warm(j) ? 0 : 1, 0}; }))
        return rc;
    leave_uniform(b);
    for (int j = 0; j < K; ++j) b->cnt[streams_host[j]] = warm(j) ? b->smooth_of(streams_host[j]) : 0;
    return APE_OK;
}

int ape_fk_replay(int32_t kind, const float* rows_dev, int32_t F, const int32_t* seg_starts_host, int32_t R, int32_t smooth,
                  const double body9[9], int32_t device, void* out_dev, int32_t out_dtype, void* stream) {
    return ape_fk_replay_bodies(kind, rows_dev, F, seg_starts_host, R, smooth, body9, device, out_dev, out_dtype, stream, nullptr);
}

int ape_fk_replay_bodies(int32_t kind, const float* rows_dev, int32_t F, const int32_t* seg_starts_host, int32_t R, int32_t smooth,
                         const double body9[9], int32_t device, void* out_dev, int32_t out_dtype, void* stream, const double* bodies_host) {
    if (!rows_dev || !out_dev || (!body9 && !bodies_host)) return ape_fail(APE_ERR_INVALID_ARG, "fk_replay: NULL argument");
    if (int rc = check_kind(kind, "fk_replay")) return rc;
    if (int rc = ape_check_segments("fk_replay", F, seg_starts_host, R)) return rc;
    if (smooth < 1) smooth = 1;
    if (smooth > 64) return ape_fail(APE_ERR_UNSUPPORTED, "fk_replay: smooth %d outside 1..64", smooth);
    if (out_dtype != APE_F32 && out_dtype != APE_F64) return ape_fail(APE_ERR_INVALID_ARG, "fk_replay: unknown dtype selector");
    if (int rc = check_device(device, "fk_replay")) return rc;
    APE_TRY(hipSetDevice(device));
    const hipStream_t st = (hipStream_t)stream;
    if (int rc = ape_check_not_capturing(st, "fk_replay", nullptr)) return rc;
    // workspaces: the frames' quaternions, their recording starts; freed behind the call's own synchronisation
    struct Scratch {
        void* p[5] = {};
        ~Scratch() { for (void* q : p) if (q) (void)hipFree(q); }
    } ws;
    APE_TRY(hipMalloc(&ws.p[0], (size_t)F * 8 * sizeof(double)));
    APE_TRY(hipMalloc(&ws.p[1], (size_t)F * sizeof(int)));
    APE_TRY(hipMalloc(&ws.p[2], (size_t)R * sizeof(int)));
    APE_TRY(hipMemcpyAsync(ws.p[2], seg_starts_host, (size_t)R * sizeof(int), hipMemcpyHostToDevice, st));
    FkReplayParams p{};
    p.rows = rows_dev; p.seg_of = (const int*)ws.p[1]; p.ws = (double*)ws.p[0]; p.out = out_dev;
    p.F = F; p.smooth = smooth; p.big_endian = (kind & APE_PARSE_BIG_ENDIAN) ? 1 : 0;
    if (body9) memcpy(p.body, body9, sizeof(p.body));
    if (bodies_host) {                                        // one body per recording: the values and every frame's recording index
        APE_TRY(hipMalloc(&ws.p[3], (size_t)R * 9 * sizeof(double)));
        APE_TRY(hipMalloc(&ws.p[4], (size_t)F * sizeof(int)));
        APE_TRY(hipMemcpyAsync(ws.p[3], bodies_host, (size_t)R * 9 * sizeof(double), hipMemcpyHostToDevice, st));
    }
    hipError_t e = ape_launch_replay_segments((const int*)ws.p[2], R, F, (int*)ws.p[1], st, (int*)ws.p[4]);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(ape_fk_replay_rows_kernel, dim3(blocks_for(F)), dim3(FK_BLOCK), 0, st, p);
        e = hipGetLastError();
    }
    if (e == hipSuccess)
        e = bodies_host ? launch_typed(ape_fk_replay_msg_kernel<float, true>, ape_fk_replay_msg_kernel<double, true>, out_dtype, F, st, p,
                                       (const double*)ws.p[3], (const int*)ws.p[4])
                        : launch_typed(ape_fk_replay_msg_kernel<float, false>, ape_fk_replay_msg_kernel<double, false>, out_dtype, F, st, p,
                                       (const double*)nullptr, (const int*)nullptr);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(st);
        return ape_fail(APE_ERR_HIP, "fk_replay: launch failed: %s", hipGetErrorString(e));
    }
    APE_TRY(hipStreamSynchronize(st));
    return APE_OK;
}
