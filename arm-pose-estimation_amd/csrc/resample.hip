// Mocap truth on each frame's clock (ape_frame_times, ape_resample_truth; the reference has no counterpart).
//
// ape_frame_times: a recording's clock from its sw_dt column, t[s_r] = 0, t[f] = dt[s_r + 1] + ... + dt[f]: a segmented inclusive scan in
// float64, reduce-then-scan over tiles of FT_TILE frames, no workgroup waits for another:
//   ape_frame_tile_kernel<.., false>  one workgroup per tile: the tile's aggregate (does it hold a recording's first frame; the sum since
//                                     the last of them, or over the whole tile)
//   ape_frame_carry_kernel            ONE workgroup: the segmented scan of the aggregates, FT_BLOCK at a time -> each tile's carry-in
//   ape_frame_tile_kernel<.., true>   one workgroup per tile: the scan again, plus the carry-in for the frames before the tile's first
//                                     recording start
// (F <= FT_TILE: the last launch alone.)  Within a tile: the dt values come in with the lanes running along the frames and are staged
// in LDS; a lane then scans its FT_PER consecutive frames, the wave scans the lane aggregates by shuffles, the four wave totals go
// through LDS.  The operator is (head, sum): a piece that holds a head discards what came before it by selection, never by arithmetic,
// so a non-finite dt stays inside its recording.  The association is fixed by F and the starts alone: the same inputs give the same bits.
//
// ape_resample_truth: one lane per output frame: the frame's recording by binary search in the starts, its query time, the last truth row
// at or before it by binary search inside the recording's rows, the two neighbouring rows converted (est columns as given, or NN
// targets through the float64 forward kinematics with refined quaternions: score_device.h's targets_to_pose, which the scoring
// kernels use), positions interpolated linearly and quaternions along the arc.  The rows leave through LDS so that a wave writes its
// 64 x 21 | 14 values as one run.
//
// float64 with separate roundings for a * b + c, like the numpy statements (score.py): contraction is off in this file.
#include "ape_internal.h"
#include "../../include/ape_hip.h"
#include "bank_host.h"
#include "score_host.h"

#include <cmath>
#include <cstdio>
#include <cstring>

#pragma clang fp contract(off)
#include "score_device.h"

namespace {

using namespace ape_scoredev;

// ---- ape_frame_times ------------------------------------------------------------------------------------------------------------------------
constexpr int FT_BLOCK = 256, FT_WAVES = FT_BLOCK / 64, FT_PER = 4, FT_TILE = FT_BLOCK * FT_PER;
constexpr int FT_PAD = FT_PER + 1;                      // a lane's frames at an odd stride in LDS: no bank conflicts

struct TimesParams {
    const void* dt;
    const int* starts;                                  // [R]
    double* times;                                      // [F]
    double* agg_sum;                                    // [tiles] the tiles' aggregates ...
    int* agg_head;                                      // [tiles]
    double* carry;                                      // [tiles] ... and carry-ins (NULL: one tile)
    long long stride;
    int F, R, big_endian;
};

// (head, sum) of a piece followed by the piece (oh, os): a head discards what came before it
__device__ __forceinline__ void seg_append(bool& head, double& sum, bool oh, double os) {
    sum = oh ? os : sum + os;
    head = head || oh;
}

template <typename T, bool WRITE>
__global__ __launch_bounds__(FT_BLOCK) void ape_frame_tile_kernel(const TimesParams p) {
    __shared__ double vals[FT_BLOCK * FT_PAD];
    __shared__ double wsum[FT_WAVES];
    __shared__ int whead[FT_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long tile0 = (long long)blockIdx.x * FT_TILE;

    // the tile's dt values as float64, neighbouring lanes on neighbouring frames; frames past F count as 0
    const T* src = static_cast<const T*>(p.dt);
#pragma unroll
    for (int k = 0; k < FT_PER; ++k) {
        const int e = k * FT_BLOCK + tid;
        const long long f = tile0 + e;
        double v = 0.0;
        if (f < p.F) {
            T raw = src[f * p.stride];
            if constexpr (sizeof(T) == 4) {
                if (p.big_endian) raw = __builtin_bit_cast(float, __builtin_bswap32(__builtin_bit_cast(unsigned, raw)));
            }
            v = (double)raw;
        }
        vals[(e / FT_PER) * FT_PAD + (e % FT_PER)] = v;
    }
    __syncthreads();

    // the lane's FT_PER consecutive frames: a recording's first frame is a head and counts 0 (its dt points before the recording)
    const long long f0 = tile0 + (long long)tid * FT_PER;
    int rec = 0;
    long long next = p.F;                               // the next recording start after f0
    if (f0 < p.F) {
        rec = find_rec(p.starts, p.R, f0);
        next = (long long)p.starts[rec] == f0 ? f0 : (rec + 1 < p.R ? (long long)p.starts[rec + 1] : (long long)p.F);
    }
    double loc[FT_PER];
    bool lhead[FT_PER];                                 // a head at or before frame k of the lane
    bool head = false;
    double sum = 0.0;
#pragma unroll
    for (int k = 0; k < FT_PER; ++k) {
        const long long f = f0 + k;
        const bool h = f < p.F && f == next;
        if (h) {
            rec = f == f0 ? rec : rec + 1;
            next = rec + 1 < p.R ? (long long)p.starts[rec + 1] : (long long)p.F;
        }
        seg_append(head, sum, h, h ? 0.0 : vals[tid * FT_PAD + k]);
        loc[k] = sum;
        lhead[k] = head;
    }

    // the wave's inclusive scan of the lane aggregates
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const double os = __shfl_up(sum, off, 64);
        const int oh = __shfl_up((int)head, off, 64);
        if (lane >= off) {
            const bool mh = head;
            const double ms = sum;
            head = oh != 0; sum = os;
            seg_append(head, sum, mh, ms);
        }
    }
    if (lane == 63) { wsum[wave] = sum; whead[wave] = (int)head; }
    // what precedes the lane inside its wave
    double ps = __shfl_up(sum, 1, 64);
    bool ph = __shfl_up((int)head, 1, 64) != 0;
    if (lane == 0) { ps = 0.0; ph = false; }
    __syncthreads();
    // ... inside its tile: the waves before it in order, then the lanes before it
    bool bh = false;
    double bs = 0.0;
    for (int w = 0; w < wave; ++w) seg_append(bh, bs, whead[w] != 0, wsum[w]);
    seg_append(bh, bs, ph, ps);

    if constexpr (!WRITE) {
        if (tid == FT_BLOCK - 1) {                      // the last lane's inclusive aggregate is the tile's
            const bool mh = lhead[FT_PER - 1];
            seg_append(bh, bs, mh, loc[FT_PER - 1]);
            p.agg_sum[blockIdx.x] = bs;
            p.agg_head[blockIdx.x] = (int)bh;
        }
    } else {
        // ... and before the tile: the carry-in counts where no head lies between the tile's first frame and this one
        if (!bh && p.carry != nullptr) bs = p.carry[blockIdx.x] + bs;
        double* lds = vals;                             // (every lane has read its values: the barrier above)
#pragma unroll
        for (int k = 0; k < FT_PER; ++k) {
            bool h = bh;
            double s = bs;
            seg_append(h, s, lhead[k], loc[k]);
            lds[tid * FT_PAD + k] = s;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < FT_PER; ++k) {
            const int e = k * FT_BLOCK + tid;
            const long long f = tile0 + e;
            if (f < p.F) p.times[f] = lds[(e / FT_PER) * FT_PAD + (e % FT_PER)];
        }
    }
}

// one workgroup: carry[t] = the sum since the last recording start before tile t (frame 0 is one, so every tile but the first has a
// head before it), FT_BLOCK tiles a round in tile order
__global__ __launch_bounds__(FT_BLOCK) void ape_frame_carry_kernel(const double* __restrict__ agg_sum, const int* __restrict__ agg_head,
                                                                   int tiles, double* __restrict__ carry) {
    __shared__ double wsum[FT_WAVES];
    __shared__ int whead[FT_WAVES];
    __shared__ double run_s;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) run_s = 0.0;
    __syncthreads();
    for (int base = 0; base < tiles; base += FT_BLOCK) {    // (uniform)
        const int t = base + tid;
        bool head = t < tiles && agg_head[t] != 0;
        double sum = t < tiles ? agg_sum[t] : 0.0;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const double os = __shfl_up(sum, off, 64);
            const int oh = __shfl_up((int)head, off, 64);
            if (lane >= off) {
                const bool mh = head;
                const double ms = sum;
                head = oh != 0; sum = os;
                seg_append(head, sum, mh, ms);
            }
        }
        if (lane == 63) { wsum[wave] = sum; whead[wave] = (int)head; }
        double ps = __shfl_up(sum, 1, 64);
        bool ph = __shfl_up((int)head, 1, 64) != 0;
        if (lane == 0) { ps = 0.0; ph = false; }
        __syncthreads();
        bool bh = false;
        double bs = run_s;                              // the rounds before this one
        for (int w = 0; w < wave; ++w) seg_append(bh, bs, whead[w] != 0, wsum[w]);
        seg_append(bh, bs, ph, ps);
        if (t < tiles) carry[t] = bs;                   // exclusive: the tiles before t
        __syncthreads();                                // (every lane has read run_s)
        if (tid == FT_BLOCK - 1) {
            bool h = bh;
            double s = bs;
            seg_append(h, s, t < tiles && agg_head[t] != 0, t < tiles ? agg_sum[t] : 0.0);
            run_s = s;
        }
        __syncthreads();
    }
}

// ---- ape_resample_truth ---------------------------------------------------------------------------------------------------------------------
constexpr int RS_BLOCK = 256, RS_WAVES = RS_BLOCK / 64, RS_W = 21;

struct ResampleParams {
    const void* truth;
    const double* truth_times;                          // [Ft] or NULL: the index clock
    const double* times;                                // [F] or NULL: the index clock
    void* out;
    const int* starts;                                  // [R]
    const int* tstarts;                                 // [R]
    const double* shifts;                               // [R]
    const double* bodies;                               // [n_bodies, 9] (APE_TRUTH_TARGETS)
    double max_gap;
    int F, Ft, R, layout, n_bodies, truth_w, out_w, out_f32;
};

__device__ __forceinline__ void put_v(double* e, const Vec3 v) { e[0] = v.x; e[1] = v.y; e[2] = v.z; }
__device__ __forceinline__ void put_q(double* e, const Quat q) { e[0] = q.w; e[1] = q.x; e[2] = q.y; e[3] = q.z; }

// one truth row -> its est row e[0 : 21 | 14]: as given, or the pose its targets stand for (score_device.h: targets_to_pose) with the
// shoulder origin [6:9] that ape_fk writes (the hips quaternion applied to the body's).  NaN propagates.
template <typename TT, int KIND>
__device__ __forceinline__ void converted_row(const TT* row, int tw, int layout, const double* body, double* e) {
    double t[RS_W];
#pragma unroll
    for (int c = 0; c < RS_W; ++c) t[c] = c < tw ? (double)row[c] : 0.0;
    if constexpr (KIND == APE_TRUTH_EST) {
#pragma unroll
        for (int c = 0; c < RS_W; ++c) e[c] = t[c];
    } else {
        const bool hips = layout != APE_LAYOUT_ORI_CAL_LARM_UARM;
        const TargetPose o = targets_to_pose(t, layout, body);
#pragma unroll
        for (int c = 0; c < RS_W; ++c) e[c] = 0.0;
        put_v(e, o.hand); put_v(e + 3, o.elbow);
        if (hips) { put_v(e + 6, o.uo); put_q(e + 9, o.lq); put_q(e + 13, o.uq); put_q(e + 17, o.hq); }
        else { put_q(e + 6, o.lq); put_q(e + 10, o.uq); }
    }
}

// The quaternion between a and b at weight w (score.py: _slerp states the same operations): both normalised, b flipped where a . b < 0.0,
// theta = 2 asin(min(1, |a - s b| / 2)) <= pi / 2, the chord below 1e-6 rad, otherwise the arc; normalised again
__device__ __forceinline__ void slerp(const double* a_in, const double* b_in, double w, double* q) {
    const double na = sqrt(a_in[0] * a_in[0] + a_in[1] * a_in[1] + a_in[2] * a_in[2] + a_in[3] * a_in[3]);
    const double nb = sqrt(b_in[0] * b_in[0] + b_in[1] * b_in[1] + b_in[2] * b_in[2] + b_in[3] * b_in[3]);
    double a[4], b[4], v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) { a[k] = a_in[k] / na; b[k] = b_in[k] / nb; }
    const double dot = a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3];
    const double s = dot < 0.0 ? -1.0 : 1.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) { b[k] = s * b[k]; v[k] = a[k] - b[k]; }
    const double h = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3]) / 2.0;
    const double theta = 2.0 * asin(h < 1.0 ? h : 1.0);
    if (theta < 1e-6) {
#pragma unroll
        for (int k = 0; k < 4; ++k) q[k] = a[k] + w * (b[k] - a[k]);
    } else {
        const double sa = sin((1.0 - w) * theta), sb = sin(w * theta), st = sin(theta);
#pragma unroll
        for (int k = 0; k < 4; ++k) q[k] = (sa * a[k] + sb * b[k]) / st;
    }
    const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
#pragma unroll
    for (int k = 0; k < 4; ++k) q[k] = q[k] / n;
}

template <typename TT, int KIND>
__global__ __launch_bounds__(RS_BLOCK) void ape_resample_kernel(const ResampleParams p) {
    __shared__ double stage[RS_WAVES][64 * RS_W];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long row0 = (long long)blockIdx.x * RS_BLOCK + wave * 64;
    const long long f = row0 + lane;
    const long long left = (long long)p.F - row0;
    const int nrows = left >= 64 ? 64 : (left > 0 ? (int)left : 0);
    const int W = p.out_w, tw = p.truth_w;
    const bool hips = p.layout != APE_LAYOUT_ORI_CAL_LARM_UARM;

    double o[RS_W];
#pragma unroll
    for (int c = 0; c < RS_W; ++c) o[c] = NAN;
    if (f < p.F) {
        const int rec = find_rec(p.starts, p.R, f);
        const int ts = p.tstarts[rec], te = rec + 1 < p.R ? p.tstarts[rec + 1] : p.Ft;
        const double tq = p.times != nullptr ? p.times[f] : (double)(f - (long long)p.starts[rec]);
        const double u = tq - p.shifts[rec];
        const double* tt = p.truth_times;
        // the first row of [ts, te) with u < tt(row), as numpy's searchsorted(side="right") walks: lo stays inside [ts, te] whatever the
        // times hold
        int lo = ts, hi = te;
        if (fin(u)) {
            while (lo < hi) {
                const int mid = lo + ((hi - lo) >> 1);
                const double tm = tt != nullptr ? tt[mid] : (double)(mid - ts);
                if (u < tm) hi = mid; else lo = mid + 1;
            }
        }
        const int i = lo - 1;                           // the last row at or before u; ts - 1: none
        if (fin(u) && i >= ts) {
            const double ti = tt != nullptr ? tt[i] : (double)(i - ts);
            const TT* src = static_cast<const TT*>(p.truth);
            const double* body = p.bodies + 9 * (size_t)(p.n_bodies > 1 ? rec : 0);
            double a[RS_W];
            converted_row<TT, KIND>(src + (size_t)i * tw, tw, p.layout, body, a);
            if (u == ti) {                              // an exact hit: the row itself, whatever it holds
#pragma unroll
                for (int c = 0; c < RS_W; ++c) o[c] = a[c];
            } else if (i + 1 < te) {
                const double tn = tt != nullptr ? tt[i + 1] : (double)(i + 1 - ts);
                const double gap = tn - ti;
                if (!(p.max_gap > 0.0 && gap > p.max_gap)) {
                    double b[RS_W];
                    converted_row<TT, KIND>(src + (size_t)(i + 1) * tw, tw, p.layout, body, b);
                    bool ok = true;
#pragma unroll
                    for (int c = 0; c < RS_W; ++c)
                        if (c < W) ok = ok && fin(a[c]) && fin(b[c]);
                    if (ok) {
                        const double w = (u - ti) / gap;
#pragma unroll
                        for (int c = 0; c < 9; ++c)
                            if (c < (hips ? 9 : 6)) o[c] = a[c] + w * (b[c] - a[c]);
                        if (hips) {
                            slerp(a + 9, b + 9, w, o + 9); slerp(a + 13, b + 13, w, o + 13); slerp(a + 17, b + 17, w, o + 17);
                        } else {
                            slerp(a + 6, b + 6, w, o + 6); slerp(a + 10, b + 10, w, o + 10);
                        }
                    }
                }
            }
        }
    }

    // through LDS: the wave writes its rows as one run
    double* lds = stage[wave];
#pragma unroll
    for (int c = 0; c < RS_W; ++c)
        if (c < W) lds[lane * RS_W + c] = o[c];
    __syncthreads();
    const int total = nrows * W;
#pragma unroll
    for (int it = 0; it < RS_W; ++it) {
        const int idx = it * 64 + lane;
        if (idx < total) {
            const int r = idx / W, c = idx - r * W;
            const size_t at = (size_t)row0 * (size_t)W + (size_t)idx;
            if (p.out_f32) static_cast<float*>(p.out)[at] = (float)lds[r * RS_W + c];
            else static_cast<double*>(p.out)[at] = lds[r * RS_W + c];
        }
    }
}

// the staging of both entries: the host arrays in, the tile aggregates behind them (score_host.h)
ApeSlotPool g_pool("resample");

size_t pad8(size_t bytes) { return (bytes + 7) & ~(size_t)7; }

template <typename T>
hipError_t launch_times(const TimesParams& p, unsigned tiles, hipStream_t st) {
    if (tiles > 1) {
        hipLaunchKernelGGL((ape_frame_tile_kernel<T, false>), dim3(tiles), dim3(FT_BLOCK), 0, st, p);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(ape_frame_carry_kernel, dim3(1), dim3(FT_BLOCK), 0, st, p.agg_sum, p.agg_head, (int)tiles, p.carry);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((ape_frame_tile_kernel<T, true>), dim3(tiles), dim3(FT_BLOCK), 0, st, p);
    return hipGetLastError();
}

template <typename TT>
void launch_resample(const ResampleParams& p, int kind, unsigned blocks, hipStream_t st) {
    if (kind == APE_TRUTH_TARGETS) hipLaunchKernelGGL((ape_resample_kernel<TT, APE_TRUTH_TARGETS>), dim3(blocks), dim3(RS_BLOCK), 0, st, p);
    else hipLaunchKernelGGL((ape_resample_kernel<TT, APE_TRUTH_EST>), dim3(blocks), dim3(RS_BLOCK), 0, st, p);
}

}  // namespace

int ape_frame_times(const void* dt_dev, int32_t dt_stride, int32_t dt_dtype, uint32_t flags, int32_t F, const int32_t* seg_starts_host,
                    int32_t R, double* times_dev, void* stream) {
    const char* who = "frame_times";
    if (!dt_dev || !seg_starts_host || !times_dev) return ape_fail(APE_ERR_INVALID_ARG, "%s: NULL argument", who);
    if (int rc = ape_check_segments(who, F, seg_starts_host, R)) return rc;
    if (dt_stride < 1) return ape_fail(APE_ERR_INVALID_ARG, "%s: dt_stride %d below 1", who, dt_stride);
    if (dt_dtype != APE_F32 && dt_dtype != APE_F64) return ape_fail(APE_ERR_INVALID_ARG, "%s: unknown dtype selector", who);
    if (flags & ~(uint32_t)APE_PARSE_BIG_ENDIAN) return ape_fail(APE_ERR_INVALID_ARG, "%s: unknown flags 0x%x", who, flags);
    if (flags && dt_dtype != APE_F32) return ape_fail(APE_ERR_INVALID_ARG, "%s: the big-endian flag is for APE_F32 rows", who);
    if (static_cast<const void*>(times_dev) == dt_dev) return ape_fail(APE_ERR_INVALID_ARG, "%s: times_dev aliases dt_dev", who);
    const hipStream_t st = (hipStream_t)stream;
    if (int rc = ape_check_not_capturing(st, who, "host arrays are staged per call")) return rc;
    int device = 0;
    APE_SCORE_TRY(g_pool.prefix, hipGetDevice(&device));

    const unsigned tiles = (unsigned)(((long long)F + FT_TILE - 1) / FT_TILE);
    const size_t starts_bytes = pad8((size_t)R * sizeof(int));
    const size_t heads_bytes = pad8((size_t)tiles * sizeof(int));
    const size_t work_bytes = 2 * (size_t)tiles * sizeof(double) + heads_bytes;      // aggregates' sums, carries, aggregates' heads

    std::lock_guard<std::mutex> lock(g_pool.mu);
    ApeSlot* slot = nullptr;
    if (int rc = g_pool.take(device, starts_bytes, starts_bytes + work_bytes, &slot)) return rc;
    memcpy(slot->pinned, seg_starts_host, (size_t)R * sizeof(int));
    APE_SCORE_TRY(g_pool.prefix, hipMemcpyAsync(slot->dev, slot->pinned, starts_bytes, hipMemcpyHostToDevice, st));

    TimesParams p{};
    char* dev = static_cast<char*>(slot->dev);
    p.dt = dt_dev; p.times = times_dev;
    p.starts = reinterpret_cast<const int*>(dev);
    p.agg_sum = reinterpret_cast<double*>(dev + starts_bytes);
    p.carry = tiles > 1 ? reinterpret_cast<double*>(dev + starts_bytes + (size_t)tiles * sizeof(double)) : nullptr;
    p.agg_head = reinterpret_cast<int*>(dev + starts_bytes + 2 * (size_t)tiles * sizeof(double));
    p.stride = dt_stride; p.F = F; p.R = R; p.big_endian = flags ? 1 : 0;
    const hipError_t e = dt_dtype == APE_F32 ? launch_times<float>(p, tiles, st) : launch_times<double>(p, tiles, st);
    return g_pool.finish(who, slot, e, st);
}

int ape_resample_truth(int32_t layout, const void* truth_dev, int32_t truth_kind, int32_t truth_dtype, int32_t Ft,
                       const int32_t* truth_starts_host, const double* truth_times_dev, const double* times_dev, int32_t F,
                       const int32_t* seg_starts_host, int32_t R, const double* shift_host, double max_gap, const double* bodies_host,
                       int32_t n_bodies, void* out_dev, int32_t out_dtype, void* stream) {
    const char* who = "resample_truth";
    if (!truth_dev || !truth_starts_host || !seg_starts_host || !bodies_host || !out_dev) return ape_fail(APE_ERR_INVALID_ARG, "%s: NULL argument", who);
    if (!ape_scoring_layout(layout))
        return ape_fail(APE_ERR_INVALID_ARG, "%s: layout %d has no pose to resample", who, layout);
    if (truth_kind != APE_TRUTH_TARGETS && truth_kind != APE_TRUTH_EST) return ape_fail(APE_ERR_INVALID_ARG, "%s: unknown truth kind %d", who, truth_kind);
    if ((truth_dtype != APE_F32 && truth_dtype != APE_F64) || (out_dtype != APE_F32 && out_dtype != APE_F64))
        return ape_fail(APE_ERR_INVALID_ARG, "%s: unknown dtype selector", who);
    if (int rc = ape_check_segments(who, F, seg_starts_host, R)) return rc;
    if (Ft < 1) return ape_fail(APE_ERR_INVALID_ARG, "%s: Ft=%d must be >= 1", who, Ft);
    if (int rc = ape_check_segments("resample_truth (truth rows)", Ft, truth_starts_host, R)) return rc;
    if (n_bodies != 1 && n_bodies != R) return ape_fail(APE_ERR_INVALID_ARG, "%s: n_bodies %d is neither 1 nor R = %d", who, n_bodies, R);
    if (max_gap != max_gap) return ape_fail(APE_ERR_INVALID_ARG, "%s: max_gap is NaN", who);
    if (shift_host)
        for (int r = 0; r < R; ++r)
            if (!std::isfinite(shift_host[r])) return ape_fail(APE_ERR_INVALID_ARG, "%s: shift %d is not finite", who, r);
    if (out_dev == truth_dev || out_dev == static_cast<const void*>(truth_times_dev) || out_dev == static_cast<const void*>(times_dev))
        return ape_fail(APE_ERR_INVALID_ARG, "%s: out_dev aliases an input", who);
    const hipStream_t st = (hipStream_t)stream;
    if (int rc = ape_check_not_capturing(st, who, "host arrays are staged per call")) return rc;
    int device = 0;
    APE_SCORE_TRY(g_pool.prefix, hipGetDevice(&device));

    const unsigned blocks = (unsigned)(((long long)F + RS_BLOCK - 1) / RS_BLOCK);
    const size_t starts_bytes = pad8((size_t)R * sizeof(int));                       // starts, truth starts, shifts, bodies
    const size_t shifts_bytes = (size_t)R * sizeof(double);
    const size_t bodies_bytes = (size_t)n_bodies * 9 * sizeof(double);
    const size_t host_bytes = 2 * starts_bytes + shifts_bytes + bodies_bytes;

    std::lock_guard<std::mutex> lock(g_pool.mu);
    ApeSlot* slot = nullptr;
    if (int rc = g_pool.take(device, host_bytes, host_bytes, &slot)) return rc;
    char* pin = static_cast<char*>(slot->pinned);
    memcpy(pin, seg_starts_host, (size_t)R * sizeof(int));
    memcpy(pin + starts_bytes, truth_starts_host, (size_t)R * sizeof(int));
    if (shift_host) memcpy(pin + 2 * starts_bytes, shift_host, shifts_bytes);
    else memset(pin + 2 * starts_bytes, 0, shifts_bytes);
    memcpy(pin + 2 * starts_bytes + shifts_bytes, bodies_host, bodies_bytes);
    APE_SCORE_TRY(g_pool.prefix, hipMemcpyAsync(slot->dev, slot->pinned, host_bytes, hipMemcpyHostToDevice, st));

    ResampleParams p{};
    const char* dev = static_cast<const char*>(slot->dev);
    p.truth = truth_dev; p.truth_times = truth_times_dev; p.times = times_dev; p.out = out_dev;
    p.starts = reinterpret_cast<const int*>(dev);
    p.tstarts = reinterpret_cast<const int*>(dev + starts_bytes);
    p.shifts = reinterpret_cast<const double*>(dev + 2 * starts_bytes);
    p.bodies = reinterpret_cast<const double*>(dev + 2 * starts_bytes + shifts_bytes);
    p.max_gap = max_gap;
    p.F = F; p.Ft = Ft; p.R = R; p.layout = layout; p.n_bodies = n_bodies;
    p.out_w = ape_truth_width(layout, APE_TRUTH_EST);   // (the rows go out as est rows)
    p.truth_w = ape_truth_width(layout, truth_kind);
    p.out_f32 = out_dtype == APE_F32 ? 1 : 0;
    if (truth_dtype == APE_F32) launch_resample<float>(p, truth_kind, blocks, st);
    else launch_resample<double>(p, truth_kind, blocks, st);
    return g_pool.finish(who, slot, hipGetLastError(), st);
}
