// The frame of WatchPhonePocketKalman (reference estimate/watch_phone_pocket_kalman.py:57-63, 133-169 inside Estimator, estimator.py:93-137)
// for a bank of S streams with every history on the device.  PARITY UNPINNED like kalman.hip: the checker of the
// bookkeeping here is oracle/kalman_oracle.py's KalmanFrameLogic chained with oracle/ape_oracle.py's WindowOracle and post-filter.
//
// A frame for K listed streams is three parts on one stream, nothing returns to the host in between:
//   ape_kalman_bank_head_kernel   (workgroup per list entry) raw row -> 22 features (parse_device.h) -> the stream's window ring (all W
//                                 slots on a cold start) -> float64 z-score -> the model's dense [K, 22 W] input; and the stream's state
//                                 ring [E, W, 14], read in time order through its head, into the model's dense [K E, 14 W] input (zeros,
//                                 and a zeroed ring, on a cold start).  This gather is both the row indirection of subset frames and the
//                                 state shift: the ring is never moved, the copy the model needs anyway is rotated.
//   ape_kalman_forward            kalman.hip's eight launches on the dense inputs, untouched: one flipout draw per call, signs per dense
//                                 row (list position j, member e), the update per list entry
//   ape_kalman_bank_tail_kernel   (workgroup per list entry) the sensor mean z (the stream's first W + 1 frames; format_state of it into
//                                 the state ring) or the corrected ensemble (afterwards; itself into the ring), the smoothing stack with
//                                 ragged entries (1 or E rows, padded with the newest on a cold start), float64 de-normalisation, FK of
//                                 every stacked row (thread per row), the sign-aligned quaternion means and the 25-value message
//                                 (stream_post_device.h's finish_msg), the packed tail, n_rows, and the stream's frame counter.
//                                 SPR (APE_FLAG_SPREAD): the spread record of the same stacked rows behind the row.
// Frame counters live on the device; the host only remembers which streams have a cold start pending and hands that over in the
// staged stream list (or, for lockstep frames, as one kernel argument).
//   ape_kalman_state_kernel       (thread per 16 bytes) a stream's rings <-> its canonical record: the state hand-over of DESIGN.md 4.27
//                                 (ape_kalman_bank_export / _import, ape_kalman_replay_resume); for it the host also keeps each
//                                 stream's age, min(frames since the cold start, W + 1)
// float64 with separate roundings for a * b + c, like numpy: contraction is off in this file.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

#include "ape_internal.h"
#include "../../include/ape_hip.h"
#include "parse_device.h"
#include "stream_post_device.h"
#include "body_table.h"
#include "bank_host.h"
#include "kalman_device.h"

#pragma clang fp contract(off)

namespace {

using namespace ape_postdev;

constexpr int DX = 14, RAW = 22;
constexpr int KB_WIDTH = 55;          // APE_PARSE_WATCH_PHONE_POCKET message
constexpr int KB_BLOCK = 256;
constexpr int KB_MAX_SMOOTH = 64;     // the post-filter's limits (ape_streams_create)
constexpr int KB_MAX_ROWS = 4096;
constexpr uint32_t KB_FLAGS = APE_FLAG_PACKED_MSG | APE_FLAG_SPREAD;      // what the frame and replay entries accept

// one list entry of a frame: the stream, whether this is its first frame since a cold start, the row it reads and the row it writes
struct KbDesc { int stream, cold, row_in, row_out; };

struct KbHeadParams {
    const float* rows;                // [*, 55] raw messages, entry j reads row desc[j].row_in
    const KbDesc* desc;               // [K] or nullptr: entry j = stream j, row j, cold = cold_all
    const int* cnt;                   // [S] frames since the stream's cold start
    double* xwin;                     // [S, W, 22] window rings (features as parse_row_to_xx returns them: float64)
    float* state;                     // [S, E, W, 14] state rings
    float* raw;                       // [K, W, 22] the model's sensor input
    float* dense;                     // [K, E, W, 14] the model's state input
    int K, E, W, big_endian, normalize, cold_all;
    double xx_m[RAW], xx_s[RAW];
};

struct KbTailParams {
    const KbDesc* desc;
    int* cnt;
    const float* z;                   // [K, 14] sensor-model mean of this frame
    const float* corrected;           // [K, E, 14]
    const float* init_noise;          // [K, E, 14] injected format_state draws, or nullptr: Philox
    unsigned long long seed;
    float* state;
    float* yring;                     // [S, smooth, E, 14] the last `smooth` predictions (normalised), 1 or E rows each
    int* nring;                       // [S, smooth] their row counts
    void* out;                        // [*, out_stride]
    int* n_rows;                      // [*]
    float* y_out;                     // [*, E, 14] or nullptr
    int K, E, W, smooth, packed, normalize, cold_all, out_stride, wrap;
    double yy_m[DX], yy_s[DX], body[9];
};

// LAND (host subset frames): p.rows and p.desc are the frame's pinned staging block in host memory; entry j's descriptor
// is also stored to land[j], the bank's device table, where the tail reads it
template <bool LAND = false>
__global__ __launch_bounds__(KB_BLOCK) void ape_kalman_bank_head_kernel(const KbHeadParams p, KbDesc* __restrict__ land) {
    __shared__ double xx[RAW];
    const int j = blockIdx.x, tid = threadIdx.x;
    const KbDesc d = p.desc ? p.desc[j] : KbDesc{j, p.cold_all, j, j};
    if constexpr (LAND) {
        if (tid == 64) land[j] = d;
    }
    const bool cold = d.cold != 0;
    const int c = cold ? 0 : p.cnt[d.stream];
    const int E = p.E, W = p.W;
    if (tid == 0) {                                     // the feature chain: one lane (parse_rows.hip)
        float r[KB_WIDTH];
        const float* src = p.rows + (size_t)d.row_in * KB_WIDTH;
#pragma unroll
        for (int k = 0; k < KB_WIDTH; ++k) {
            float v = src[k];
            if (p.big_endian) v = __builtin_bit_cast(float, __builtin_bswap32(__builtin_bit_cast(unsigned, v)));
            r[k] = v;
        }
        [[clang::always_inline]] ape_parsedev::parse_row(r, KB_WIDTH, APE_PARSE_WATCH_PHONE_POCKET, xx);     // (inline in both instantiations, as in the one)
    } else if (tid >= 64) {
        // beside it, waves 1-3: the state history in time order.  The ring's oldest entry sits in slot c mod W (the slot this frame's
        // tail overwrites); 8-byte pieces (a state is 14 floats = 56 bytes).  Cold start: zeros, and the ring is zeroed for the frames to come.
        const int per = W * 7, n = E * per, h = c % W;
        float2* ring = reinterpret_cast<float2*>(p.state + (size_t)d.stream * E * W * DX);
        float2* dst = reinterpret_cast<float2*>(p.dense + (size_t)j * E * W * DX);
        for (int idx = tid - 64; idx < n; idx += KB_BLOCK - 64) {
            float2 v = {0.0f, 0.0f};
            if (cold) ring[idx] = v;
            else {
                const int e = idx / per, rem = idx - e * per, i = rem / 7, q = rem - i * 7;
                int sl = h + i;
                if (sl >= W) sl -= W;
                v = ring[e * per + sl * 7 + q];
            }
            dst[idx] = v;
        }
    }
    __syncthreads();
    // the window: step W-1 is the new row, step t < W-1 ring slot slot+1+t (mod W); z-score in float64, cast (estimator.py:96-104)
    const int slot = c % W;
    double* win = p.xwin + (size_t)d.stream * W * RAW;
    float* raw = p.raw + (size_t)j * W * RAW;
    for (int idx = tid; idx < W * RAW; idx += KB_BLOCK) {
        const int t = idx / RAW, f = idx - t * RAW;
        double v;
        if (cold) { v = xx[f]; win[idx] = v; }
        else if (t == W - 1) { v = xx[f]; win[slot * RAW + f] = v; }
        else {
            int sl = slot + 1 + t;
            if (sl >= W) sl -= W;
            v = win[sl * RAW + f];                  // (never the slot written above: sl != slot for t < W - 1)
        }
        if (p.normalize) v = (v - p.xx_m[f]) / p.xx_s[f];
        raw[idx] = (float)v;
    }
}

// TAB (per-stream bodies): the nine body values are row `stream` of bodies [S,9], uniform over the workgroup, instead of
// the uniform p.body
// SPR (APE_FLAG_SPREAD): the row is APE_SPREAD_WIDTH columns longer (p.out_stride counts them) and ENDS in the spread
// record of the N stacked rows (stream_post_device.h).  Beside acc every thread keeps 48 sums over its act rows -- the
// 9 + 9 moments of the hand and elbow origins, the 10 + 10 + 10 sums of q q^T of the three joints -- reduced like acc: a thread's rows
// in order, the wave tree, the four waves in wave order, so the order of every sum is fixed by (N, thread, wave) alone.  Wave 1 closes
// the record while thread 0 composes the message: lanes 0 / 1 the two origins, lanes 2 .. 4 one joint's angle each against the
// message's quaternion, which they form from `red` by thread 0's very operations (IEEE operations, contraction off: the same bits).
// A parameter of the template: KbTailParams and the other forms' object code stay what they were.
// DONE (host subset frames of up to 64 entries): p.out and p.n_rows are pinned host memory; behind the entry's row and
// count -- system-scope release -- the workgroup writes word j of dn.words, which the host is watching (stream_post_device.h, done_out)
struct KbDone { unsigned* words; unsigned val; };
template <typename TMsg, bool TAB = false, bool SPR = false, bool DONE = false>
__global__ __launch_bounds__(KB_BLOCK) void ape_kalman_bank_tail_kernel(const KbTailParams p, const double* __restrict__ bodies, const KbDone dn) {
    __shared__ int ent_slot[KB_MAX_SMOOTH], ent_first[KB_MAX_SMOOTH + 1];   // stack entries, oldest first: ring slot (-1: this frame's), first stacked row
    __shared__ double ref_s[3][4], e0_s[21], red[KB_BLOCK / 64][12];
    __shared__ double spr_red[SPR ? KB_BLOCK / 64 : 1][SPR ? 48 : 1];       // SPR: the waves' partial spread sums (unused otherwise)
    const int j = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const KbDesc d = p.desc ? p.desc[j] : KbDesc{j, p.cold_all, j, j};
    const bool cold = d.cold != 0;
    const int s = d.stream, E = p.E, W = p.W, smooth = p.smooth;
    const int c = cold ? 0 : p.cnt[s];
    // watch_phone_pocket_kalman.py:141-156: the first W + 1 frames return the sensor model's mean and feed format_state of it back
    const bool init = c <= W;
    const int n_new = init ? 1 : E;
    const int pos = c % smooth;
    const float* src_new = init ? p.z + (size_t)j * DX : p.corrected + (size_t)j * E * DX;
    {   // this frame's entry of the state history (slot c mod W: the oldest one's)
        float* ring = p.state + (size_t)s * E * W * DX;
        const int slot = c % W;
        for (int idx = tid; idx < E * DX; idx += KB_BLOCK) {
            const int e = idx / DX, cc = idx - e * DX;
            float v;
            if (init) {                             // kalman_models.py:164-173: N(0, 0.1 I) around z, a draw per (list entry, member)
                const size_t g = (size_t)j * E * DX + idx;
                const float nz = p.init_noise ? p.init_noise[g] : ape_kfdev::philox_normal((unsigned)g, 0x300u, p.seed);
                v = p.z[(size_t)j * DX + cc] + 0.31622776601683794f * nz;
            } else v = p.corrected[(size_t)j * E * DX + idx];
            ring[(e * W + slot) * DX + cc] = v;
        }
    }
    // the prediction: to the caller and into the smoothing stack (every slot on a cold start, estimator.py:114-115)
    for (int idx = tid; idx < n_new * DX; idx += KB_BLOCK) {
        const float v = src_new[idx];
        if (p.y_out) p.y_out[(size_t)d.row_out * E * DX + idx] = v;
        for (int t = cold ? 0 : pos; t < (cold ? smooth : pos + 1); ++t) p.yring[((size_t)(s * smooth + t) * E) * DX + idx] = v;
    }
    if (tid < smooth) {
        int sl = pos + 1 + tid;
        if (sl >= smooth) sl -= smooth;
        const bool fresh = cold || tid == smooth - 1;
        ent_slot[tid] = fresh ? -1 : sl;
        ent_first[tid + 1] = fresh ? n_new : p.nring[s * smooth + sl];      // (row counts; summed below)
    }
    __syncthreads();
    if (tid == 0) {
        ent_first[0] = 0;
        for (int k = 0; k < smooth; ++k) ent_first[k + 1] += ent_first[k];
        for (int t = cold ? 0 : pos; t < (cold ? smooth : pos + 1); ++t) p.nring[s * smooth + t] = n_new;
    }
    __syncthreads();
    const int N = ent_first[smooth];
    const double wgt = 1.0 / (double)N;
    const double* const body = TAB ? bodies + 9 * (size_t)s : p.body;
    const Vec3 larm_vec{body[0], body[1], body[2]}, uarm_vec{body[3], body[4], body[5]}, orig{body[6], body[7], body[8]};
    TMsg* out = static_cast<TMsg*>(p.out) + (size_t)d.row_out * p.out_stride;
    double acc[12] = {};
    double ss[SPR ? 48 : 1] = {};                           // SPR: hand 0:9, elbow 9:18, lower arm 18:28, upper arm 28:38, hips 38:48
    for (int base = 0; base < N; base += KB_BLOCK) {        // thread per stacked row, oldest entry first (trip count uniform)
        const int i = base + tid;
        const bool act = i < N;
        double q[12] = {};
        if (act) {
            int k = 0;
            while (i >= ent_first[k + 1]) ++k;
            const int r = i - ent_first[k];
            const float* src = ent_slot[k] < 0 ? src_new + (size_t)r * DX : p.yring + ((size_t)(s * smooth + ent_slot[k]) * E + r) * DX;
            double y[DX];
#pragma unroll
            for (int cc = 0; cc < DX; ++cc) {
                double v = (double)src[cc];
                if (p.normalize) v = v * p.yy_s[cc] + p.yy_m[cc];              // estimator.py:108-109
                y[cc] = v;
            }
            // estimate_joints.py:48-71 (ORI_CAL_LARM_UARM_HIPS)
            const Quat lq = six_drr_to_quat(y), uq = six_drr_to_quat(y + 6), hq = hips_quat(y[12], y[13]);
            const Vec3 uo = qrot(hq, orig);
            const Vec3 lo = vadd(qrot(uq, uarm_vec), uo);
            const Vec3 ho = vadd(qrot(lq, larm_vec), lo);
            put_q(q, lq); put_q(q + 4, uq); put_q(q + 8, hq);
            if constexpr (SPR) {
                double h3[3], l3[3];
                put_v(h3, ho); put_v(l3, lo);
                spread_add_pos(ss, h3); spread_add_pos(ss + 9, l3);
                spread_add_quat(ss + 18, q); spread_add_quat(ss + 28, q + 4); spread_add_quat(ss + 38, q + 8);
            }
            if (p.packed) {                                                  // estimator.py:131-137: est[i, :6] of every row
                TMsg* t = out + 25 + (size_t)i * 6;
                t[0] = (TMsg)ho.x; t[1] = (TMsg)ho.y; t[2] = (TMsg)ho.z; t[3] = (TMsg)lo.x; t[4] = (TMsg)lo.y; t[5] = (TMsg)lo.z;
            }
            if (i == 0) {                                                    // row 0: the sign reference, and the N == 1 message
#pragma unroll
                for (int cc = 0; cc < 12; ++cc) ref_s[cc >> 2][cc & 3] = q[cc];
                put_v(e0_s, ho); put_v(e0_s + 3, lo); put_v(e0_s + 6, uo);
#pragma unroll
                for (int cc = 0; cc < 12; ++cc) e0_s[9 + cc] = q[cc];
            }
        }
        if (base == 0) __syncthreads();
        if (act && N > 1) {                                                  // transformations.py:32-51
#pragma unroll
            for (int g = 0; g < 3; ++g) {
                const double r0 = ref_s[g][0], r1 = ref_s[g][1], r2 = ref_s[g][2], r3 = ref_s[g][3];
                const double dt = fma(q[4 * g + 3], r3, fma(q[4 * g + 2], r2, fma(q[4 * g + 1], r1, q[4 * g] * r0)));
                const double sg = (i > 0 && dt < 0.0) ? -wgt : wgt;
#pragma unroll
                for (int cc = 0; cc < 4; ++cc) acc[4 * g + cc] += q[4 * g + cc] * sg;
            }
        }
    }
    if (N > 1) {
#pragma unroll
        for (int cc = 0; cc < 12; ++cc) {
            const double v = wave_sum(acc[cc]);
            if (lane == 0) red[wave][cc] = v;
        }
        if constexpr (SPR) {
#pragma unroll
            for (int cc = 0; cc < 48; ++cc) {
                const double v = wave_sum(ss[cc]);
                if (lane == 0) spr_red[wave][cc] = v;
            }
        }
    }
    if (p.packed)                                                            // beyond the stacked rows: zeros (SPR: up to the record)
        for (int idx = 25 + 6 * N + tid; idx < p.out_stride - (SPR ? APE_SPREAD_WIDTH : 0); idx += KB_BLOCK) out[idx] = (TMsg)0.0;
    __syncthreads();
    if constexpr (SPR) {
        TMsg* rec = out + (p.out_stride - APE_SPREAD_WIDTH);
        const int u = tid - 64;
        if (N == 1) {                                                        // the row's two origins, zeros by rule
            if (u >= 0 && u < APE_SPREAD_WIDTH) rec[u] = (TMsg)spread_single(e0_s, u);
        } else if (u == 0 || u == 1) {
            double t[9], o[9];
#pragma unroll
            for (int cc = 0; cc < 9; ++cc)
                t[cc] = ((spr_red[0][9 * u + cc] + spr_red[1][9 * u + cc]) + spr_red[2][9 * u + cc]) + spr_red[3][9 * u + cc];
            spread_pos_out(t, N, o);
#pragma unroll
            for (int cc = 0; cc < 9; ++cc) rec[9 * u + cc] = (TMsg)o[cc];
        } else if (u >= 2 && u < 5) {
            const int g = u - 2;
            double a[4], qm[4], t[10];
#pragma unroll
            for (int cc = 0; cc < 4; ++cc) a[cc] = ((red[0][4 * g + cc] + red[1][4 * g + cc]) + red[2][4 * g + cc]) + red[3][4 * g + cc];
            const double nrm = sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2] + a[3] * a[3]);
#pragma unroll
            for (int cc = 0; cc < 4; ++cc) qm[cc] = a[cc] / nrm;
#pragma unroll
            for (int cc = 0; cc < 10; ++cc) {
                const int k = 18 + 10 * g + cc;
                t[cc] = ((spr_red[0][k] + spr_red[1][k]) + spr_red[2][k]) + spr_red[3][k];
            }
            rec[18 + g] = (TMsg)spread_angle_out(t, N, qm);
        }
    }
    if (tid == 0) {
        double out_q[3][4] = {}, orig_mean[9] = {}, e0[21], m[25];
        if (N > 1) {
#pragma unroll
            for (int g = 0; g < 3; ++g) {
                double a[4];
#pragma unroll
                for (int cc = 0; cc < 4; ++cc) a[cc] = ((red[0][4 * g + cc] + red[1][4 * g + cc]) + red[2][4 * g + cc]) + red[3][4 * g + cc];
                const double nrm = sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2] + a[3] * a[3]);
#pragma unroll
                for (int cc = 0; cc < 4; ++cc) out_q[g][cc] = a[cc] / nrm;
            }
        }
#pragma unroll
        for (int cc = 0; cc < 21; ++cc) e0[cc] = e0_s[cc];
        finish_msg(APE_LAYOUT_ORI_CAL_LARM_UARM_HIPS, N, out_q, orig_mean, e0, body, m);
#pragma unroll
        for (int cc = 0; cc < 25; ++cc) out[cc] = (TMsg)m[cc];
        p.n_rows[d.row_out] = N;
        int next = c + 1;                           // (kept below 2^30 with its residues mod W and mod smooth, and above W)
        if (next >= (1 << 30)) next -= p.wrap;
        p.cnt[s] = next;
    }
    if constexpr (DONE) {
        __threadfence_system();
        __syncthreads();
        if (tid == 0) __hip_atomic_store(dn.words + j, dn.val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// ---- state hand-over: a stream's rings <-> its canonical record, every part oldest first ---------------------------
//   window  f64 [W][22]          44 W words, 11 W 16-byte units
//   history f32 [E][W][14]       E W 7 8-byte pieces; entries older than the cold start (canonical index < W - age) are zeros
//   stack   f32 [smooth][E][14]  smooth E 7 pieces; rows at or beyond the entry's count are zeros
//   counts  i32 [smooth]         1 or E; then zero words up to a multiple of 4
// One thread per 16-byte unit of a record, consecutive threads consecutive units (the canonical side: one 16-byte access).  A unit of
// the window is one 16-byte access on the ring side too; every later unit is two 8-byte pieces, each of which lies in ONE part (the
// history and the stack are whole pieces, the counts begin at an even word), so a unit that straddles two parts needs no special case.
// With the stream's count c (export: read from p.cnt here; import: the descriptor's c', which the kernel also stores) canonical index i
// of a part lives in ring slot (c + i) mod size: slot c mod size is the one the next frame overwrites, the oldest (head and tail above).
struct KsDesc { int stream, age, c, pad; };   // age = min(frames since the cold start, W + 1); 0: export zeros / import nothing

struct KsParams {
    const KsDesc* desc;               // [K]
    int* cnt;
    double* xwin;
    float* state;
    float* yring;
    int* nring;
    float* rec;                       // [K, 4 * units] the records
    int K, E, W, smooth, units;
};

template <bool IMPORT>
__global__ __launch_bounds__(KB_BLOCK) void ape_kalman_state_kernel(const KsParams p) {
    const long long idx = (long long)blockIdx.x * KB_BLOCK + threadIdx.x;
    if (idx >= (long long)p.K * p.units) return;
    const int j = (int)(idx / p.units), u = (int)(idx - (long long)j * p.units);
    const KsDesc d = p.desc[j];
    f32x4* rec = reinterpret_cast<f32x4*>(p.rec) + idx;
    if (d.age <= 0) {
        if (!IMPORT) *rec = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        return;
    }
    const int s = d.stream, E = p.E, W = p.W, smooth = p.smooth;
    int c = IMPORT ? d.c : p.cnt[s];
    if (c < 0) c = 0;
    if (IMPORT && u == 0) p.cnt[s] = c;
    const int nwin = 11 * W;
    if (u < nwin) {                                     // a row is 22 doubles = 11 units
        const int t = u / 11, q = u - 11 * t;
        f32x4* ring = reinterpret_cast<f32x4*>(p.xwin + ((size_t)s * W + (c + t) % W) * RAW) + q;
        if (IMPORT) *ring = *rec;
        else *rec = *ring;
        return;
    }
    const int nh = E * W * 7, ns = smooth * E * 7;
    f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
    if (IMPORT) v = *rec;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int piece = 2 * (u - nwin) + h;
        float2 x = {v[2 * h], v[2 * h + 1]};
        if (piece < nh) {
            const int e = piece / (W * 7), rem = piece - e * W * 7, i = rem / 7, q = rem - 7 * i;
            const bool live = i >= W - d.age;
            float2* ring = reinterpret_cast<float2*>(p.state + (((size_t)s * E + e) * W + (c + i) % W) * DX) + q;
            if (IMPORT) *ring = live ? x : float2{0.0f, 0.0f};
            else x = live ? *ring : float2{0.0f, 0.0f};
        } else if (piece < nh + ns) {
            const int r2 = piece - nh, k = r2 / (E * 7), rem = r2 - k * E * 7, r = rem / 7, q = rem - 7 * r;
            const int slot = (c + k) % smooth;
            // the entry's count: the ring's on export, the record's own count word on import
            const int n = IMPORT ? reinterpret_cast<const int*>(p.rec)[(size_t)j * p.units * 4 + 4 * nwin + 2 * (nh + ns) + k]
                                 : p.nring[s * smooth + slot];
            const bool live = r < (n == E ? E : 1);
            float2* ring = reinterpret_cast<float2*>(p.yring + (((size_t)s * smooth + slot) * E + r) * DX) + q;
            if (IMPORT) *ring = live ? x : float2{0.0f, 0.0f};
            else x = live ? *ring : float2{0.0f, 0.0f};
        } else {
            float w[2] = {x.x, x.y};
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                const int k = 2 * (piece - nh - ns) + b;
                if (k < smooth) {                       // anything but E is stored as 1: the tail kernel never reads past an entry
                    int* cell = p.nring + s * smooth + (c + k) % smooth;
                    if (IMPORT) *cell = __builtin_bit_cast(int, w[b]) == E ? E : 1;
                    else w[b] = __builtin_bit_cast(float, *cell == E ? E : 1);
                } else w[b] = 0.0f;
            }
            x = float2{w[0], w[1]};
        }
        v[2 * h] = x.x;
        v[2 * h + 1] = x.y;
    }
    if (!IMPORT) *rec = v;
}


int check_kind(int32_t kind, const char* what) {
    if ((kind & ~APE_PARSE_BIG_ENDIAN) != APE_PARSE_WATCH_PHONE_POCKET)
        return ape_fail(APE_ERR_INVALID_ARG, "%s: kind %d: the Kalman estimator reads APE_PARSE_WATCH_PHONE_POCKET rows only", what, kind);
    return APE_OK;
}

int check_capture(hipStream_t st, const char* what) {
    return ape_check_not_capturing(st, what, "stream lists and draw keys are staged per call");
}

}  // namespace

struct ape_kalman_bank {
    ape_kalman* model = nullptr;
    int S = 0, E = 0, W = 0, smooth = 1, device = 0;
    bool normalize = false;
    double xx_m[RAW] = {}, xx_s[RAW] = {}, yy_m[DX] = {}, yy_s[DX] = {}, body[9] = {};
    unsigned long long seed = 0x5EED, calls = 0;
    // per-stream state
    double* xwin = nullptr;
    float* state = nullptr;
    float* yring = nullptr;
    int* nring = nullptr;
    int* cnt = nullptr;
    // per-frame images and the model's outputs
    float *raw = nullptr, *dense = nullptr, *corrected = nullptr, *ensz = nullptr, *mcorr = nullptr, *mpred = nullptr, *z = nullptr;
    // cold starts not yet handed to the device (a fresh bank: all), the staged stream lists
    std::vector<char> pending;
    int n_pending = 0;
    KbDesc* desc = nullptr;
    ApeDescStage stage;               // pinned slots of S KbDesc (bank_host.h)
    // frame_host: pinned rows, messages and row counts
    float* h_rows = nullptr;
    void* h_out = nullptr;
    int* h_n = nullptr;
    // frame_subset_host: ONE pinned block of [64] completion words, [S] descriptors and [S, 55] rows; the value awaited
    char* hs_block = nullptr;
    unsigned hs_done_val = 0;
    ApeBodyTable bodies;              // per-stream bodies [S,9] (off until ape_kalman_bank_set_bodies)
    // state hand-over: min(frames since the cold start, W + 1) per stream, kept where `pending` is kept, and the
    // export / import kernel's own descriptors (b->desc may still be read by a frame in flight); allocated by the first hand-over
    std::vector<int> age;
    KsDesc* ks_desc = nullptr;
    ApeDescStage ks_stage;            // pinned slots of S KsDesc
};

namespace {

void bank_free(ape_kalman_bank* b) {
    ape_body_table_free(b->bodies);
    void* dev[] = {b->xwin, b->state, b->yring, b->nring, b->cnt, b->raw, b->dense, b->corrected, b->ensz, b->mcorr, b->mpred, b->z, b->desc,
                   b->ks_desc};
    for (void* q : dev) if (q) (void)hipFree(q);
    void* host[] = {b->h_rows, b->h_out, b->h_n, b->hs_block};
    for (void* q : host) if (q) (void)hipHostFree(q);
    b->stage.free();
    b->ks_stage.free();
    delete b;
}

// argument checks that need no device, then the allocations; `what` names the entry in messages
int bank_make(ape_kalman* model, int32_t n_streams, int32_t smooth, const char* what, ape_kalman_bank** out) {
    if (n_streams < 1 || n_streams > 65535) return ape_fail(APE_ERR_INVALID_ARG, "%s: n_streams=%d outside [1, 65535]", what, n_streams);
    if (smooth < 1) smooth = 1;                                 // estimator.py:45: max(1, smooth)
    if (smooth > KB_MAX_SMOOTH) return ape_fail(APE_ERR_UNSUPPORTED, "%s: smooth %d outside 1..%d", what, smooth, KB_MAX_SMOOTH);
    ApeKalmanInfo mi;
    ape_kalman_info(model, &mi);
    if (!mi.has_weights) return ape_fail(APE_ERR_NOT_READY, "%s: the model's weights are not loaded", what);
    if (smooth * mi.E > KB_MAX_ROWS)
        return ape_fail(APE_ERR_UNSUPPORTED, "%s: smooth %d x %d members = %d stacked rows, more than %d", what, smooth, mi.E, smooth * mi.E, KB_MAX_ROWS);
    APE_TRY(hipSetDevice(mi.device));
    ape_kalman_bank* b = new (std::nothrow) ape_kalman_bank();
    if (!b) return ape_fail(APE_ERR_HIP, "%s: out of host memory", what);
    b->model = model; b->S = n_streams; b->E = mi.E; b->W = mi.W; b->smooth = smooth; b->device = mi.device;
    b->pending.assign((size_t)n_streams, 1);
    b->n_pending = n_streams;
    b->age.assign((size_t)n_streams, 0);
    const size_t S = (size_t)n_streams, E = (size_t)mi.E, W = (size_t)mi.W;
    hipError_t e = hipMalloc((void**)&b->xwin, S * W * RAW * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void**)&b->state, S * E * W * DX * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void**)&b->yring, S * smooth * E * DX * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void**)&b->nring, S * smooth * sizeof(int));
    if (e == hipSuccess) e = hipMalloc((void**)&b->cnt, S * sizeof(int));
    if (e == hipSuccess) e = hipMalloc((void**)&b->raw, S * W * RAW * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void**)&b->dense, S * E * W * DX * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void**)&b->corrected, S * E * DX * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void**)&b->ensz, S * E * DX * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void**)&b->mcorr, S * DX * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void**)&b->mpred, S * DX * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void**)&b->z, S * DX * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void**)&b->desc, S * sizeof(KbDesc));
    if (e == hipSuccess) e = b->stage.alloc(n_streams, sizeof(KbDesc));
    if (e != hipSuccess) {
        bank_free(b);
        return ape_fail(APE_ERR_HIP, "%s: allocation failed: %s", what, hipGetErrorString(e));
    }
    *out = b;
    return APE_OK;
}

// head -> model -> tail for K list entries on `st`.  desc_dev nullptr: entry j = stream j, row j, all cold or none
// hf (host subset frames): the head reads hf->desc (pinned) and lands it in desc_dev; hf->done: the tail's completion words, or nullptr
struct KbHostFrame { const KbDesc* desc; unsigned* done; unsigned done_val; };
int frame_launch(ape_kalman_bank* b, int big_endian, const float* rows, const KbDesc* desc_dev, int cold_all, int32_t K,
                 const float* noise, const float* init_noise, uint32_t flags, void* out, int32_t out_dtype, int* n_rows, float* y,
                 hipStream_t st, const char* what, const KbHostFrame* hf = nullptr) {
    b->calls += 1;
    const unsigned long long seed = b->seed + 0xD1342543DE82EF95ull * b->calls;       // a key per call
    KbHeadParams h{};
    h.rows = rows; h.desc = desc_dev; h.cnt = b->cnt; h.xwin = b->xwin; h.state = b->state; h.raw = b->raw; h.dense = b->dense;
    h.K = K; h.E = b->E; h.W = b->W; h.big_endian = big_endian; h.normalize = b->normalize ? 1 : 0; h.cold_all = cold_all;
    memcpy(h.xx_m, b->xx_m, sizeof(h.xx_m));
    memcpy(h.xx_s, b->xx_s, sizeof(h.xx_s));
    if (hf) {
        h.desc = hf->desc;
        hipLaunchKernelGGL(ape_kalman_bank_head_kernel<true>, dim3(K), dim3(KB_BLOCK), 0, st, h, const_cast<KbDesc*>(desc_dev));
    } else hipLaunchKernelGGL(ape_kalman_bank_head_kernel<false>, dim3(K), dim3(KB_BLOCK), 0, st, h, (KbDesc*)nullptr);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return ape_fail(APE_ERR_HIP, "%s: head launch failed: %s", what, hipGetErrorString(e));
    if (int rc = ape_kalman_forward(b->model, b->raw, b->dense, K, seed, noise, b->corrected, b->mcorr, b->mpred, b->z, b->ensz, st)) return rc;
    KbTailParams t{};
    t.desc = desc_dev; t.cnt = b->cnt; t.z = b->z; t.corrected = b->corrected; t.init_noise = init_noise; t.seed = seed;
    t.state = b->state; t.yring = b->yring; t.nring = b->nring; t.out = out; t.n_rows = n_rows; t.y_out = y;
    t.K = K; t.E = b->E; t.W = b->W; t.smooth = b->smooth; t.packed = (flags & APE_FLAG_PACKED_MSG) ? 1 : 0;
    t.normalize = h.normalize; t.cold_all = cold_all;
    const bool spr = (flags & APE_FLAG_SPREAD) != 0;                                   // the record: the row's last columns
    t.out_stride = (t.packed ? 25 + 6 * b->smooth * b->E : 25) + (spr ? APE_SPREAD_WIDTH : 0);
    const int period = b->W * b->smooth;
    t.wrap = period * ((1 << 29) / period);
    memcpy(t.yy_m, b->yy_m, sizeof(t.yy_m));
    memcpy(t.yy_s, b->yy_s, sizeof(t.yy_s));
    memcpy(t.body, b->body, sizeof(t.body));
    // one instantiation per (message type, body table, record)
    using TailFn = void (*)(const KbTailParams, const double*, const KbDone);
    static const TailFn tails[2][2][2] = {
        {{ape_kalman_bank_tail_kernel<double, false, false>, ape_kalman_bank_tail_kernel<double, false, true>},
         {ape_kalman_bank_tail_kernel<double, true, false>, ape_kalman_bank_tail_kernel<double, true, true>}},
        {{ape_kalman_bank_tail_kernel<float, false, false>, ape_kalman_bank_tail_kernel<float, false, true>},
         {ape_kalman_bank_tail_kernel<float, true, false>, ape_kalman_bank_tail_kernel<float, true, true>}}};
    static const TailFn tails_done[2][2][2] = {
        {{ape_kalman_bank_tail_kernel<double, false, false, true>, ape_kalman_bank_tail_kernel<double, false, true, true>},
         {ape_kalman_bank_tail_kernel<double, true, false, true>, ape_kalman_bank_tail_kernel<double, true, true, true>}},
        {{ape_kalman_bank_tail_kernel<float, false, false, true>, ape_kalman_bank_tail_kernel<float, false, true, true>},
         {ape_kalman_bank_tail_kernel<float, true, false, true>, ape_kalman_bank_tail_kernel<float, true, true, true>}}};
    const bool tab = b->bodies.on();
    const bool done = hf != nullptr && hf->done != nullptr;
    hipLaunchKernelGGL((done ? tails_done : tails)[out_dtype == APE_F32 ? 1 : 0][tab ? 1 : 0][spr ? 1 : 0], dim3(K), dim3(KB_BLOCK), 0, st, t,
                       tab ? (const double*)b->bodies.dev : (const double*)nullptr, done ? KbDone{hf->done, hf->done_val} : KbDone{nullptr, 0u});
    e = hipGetLastError();
    if (e != hipSuccess) return ape_fail(APE_ERR_HIP, "%s: tail launch failed: %s", what, hipGetErrorString(e));
    return APE_OK;
}

// one frame of a bank: the pending cold starts of the listed streams travel with the list
int bank_frame(ape_kalman_bank* b, int32_t kind, const float* rows, const int32_t* streams_host, int32_t K, const float* noise,
               const float* init_noise, uint32_t flags, void* out, int32_t out_dtype, int* n_rows, float* y, hipStream_t st, const char* what,
               KbDesc* pinned_desc = nullptr, unsigned* done = nullptr, unsigned done_val = 0) {
    const KbDesc* desc_dev = nullptr;
    int cold_all = 0;
    KbHostFrame hf{pinned_desc, done, done_val};
    if (pinned_desc) {
        // host subset frame: the list into the frame's pinned block, which the head kernel reads and lands in b->desc -- no copy, no event
        for (int j = 0; j < K; ++j) {
            const int s = streams_host ? streams_host[j] : j;
            pinned_desc[j] = KbDesc{s, b->pending[s] ? 1 : 0, j, j};
        }
        desc_dev = b->desc;
    } else if (!streams_host && (b->n_pending == 0 || b->n_pending == b->S)) cold_all = b->n_pending ? 1 : 0;
    else {
        // the list into the next pinned slot -- once the copy that last read it has completed
        hipError_t slot_wait;
        KbDesc* h = static_cast<KbDesc*>(b->stage.take(&slot_wait));
        APE_TRY(slot_wait);
        for (int j = 0; j < K; ++j) {
            const int s = streams_host ? streams_host[j] : j;
            h[j] = KbDesc{s, b->pending[s] ? 1 : 0, j, j};
        }
        APE_TRY(b->stage.send(b->desc, (size_t)K * sizeof(KbDesc), st));
        desc_dev = b->desc;
    }
    if (int rc = frame_launch(b, (kind & APE_PARSE_BIG_ENDIAN) ? 1 : 0, rows, desc_dev, cold_all, K, noise, init_noise, flags, out, out_dtype,
                              n_rows, y, st, what, pinned_desc ? &hf : nullptr))
        return rc;
    for (int j = 0; j < K; ++j) {
        const int s = streams_host ? streams_host[j] : j;
        if (b->pending[s]) { b->pending[s] = 0; b->n_pending -= 1; b->age[s] = 1; }
        else if (b->age[s] <= b->W) b->age[s] += 1;
    }
    return APE_OK;
}

// ---- state hand-over ------------------------------------------------------------------------------------------------
int state_words(int E, int W, int smooth) { return (2 * W * RAW + E * W * DX + smooth * E * DX + smooth + 3) & ~3; }

void state_desc_of(const ape_kalman_bank* b, ape_kalman_state_desc_t* d) {
    d->version = APE_KALMAN_STATE_VERSION;
    d->E = b->E; d->W = b->W; d->smooth = b->smooth;
    d->words_per_stream = state_words(b->E, b->W, b->smooth);
}

// the count an imported stream of that age continues from: its true count while `init` depends on it, else the smallest positive
// multiple of W * smooth above W -- every ring then has slot order = time order, and the tail kernel's wrap rule keeps its residues
int import_count(const ape_kalman_bank* b, int age) {
    if (age <= b->W) return age;
    const int period = b->W * b->smooth;
    return period * (b->W / period + 1);
}

// K records <-> the listed streams' rings in ONE launch on `st`; the ages are those of ages_host (validated by the caller).
// streams_host nullptr: stream j (the replay's bank)
template <bool IMPORT>
int state_launch(ape_kalman_bank* b, const int32_t* streams_host, int32_t K, const int32_t* ages_host, float* rec, hipStream_t st,
                 const char* what) {
    if (!b->ks_desc) {
        hipError_t e = hipMalloc((void**)&b->ks_desc, (size_t)b->S * sizeof(KsDesc));
        if (e == hipSuccess) e = b->ks_stage.alloc(b->S, sizeof(KsDesc));
        if (e != hipSuccess) return ape_fail(APE_ERR_HIP, "%s: allocation failed: %s", what, hipGetErrorString(e));
    }
    // the descriptors into the next pinned slot -- once the copy that last read it has completed (as bank_frame's lists)
    hipError_t slot_wait;
    KsDesc* h = static_cast<KsDesc*>(b->ks_stage.take(&slot_wait));
    APE_TRY(slot_wait);
    for (int j = 0; j < K; ++j) h[j] = KsDesc{streams_host ? streams_host[j] : j, ages_host[j], IMPORT ? import_count(b, ages_host[j]) : 0, 0};
    APE_TRY(b->ks_stage.send(b->ks_desc, (size_t)K * sizeof(KsDesc), st));
    KsParams p{};
    p.desc = b->ks_desc; p.cnt = b->cnt; p.xwin = b->xwin; p.state = b->state; p.yring = b->yring; p.nring = b->nring; p.rec = rec;
    p.K = K; p.E = b->E; p.W = b->W; p.smooth = b->smooth; p.units = state_words(b->E, b->W, b->smooth) / 4;
    const unsigned blocks = (unsigned)(((long long)K * p.units + KB_BLOCK - 1) / KB_BLOCK);
    hipLaunchKernelGGL(ape_kalman_state_kernel<IMPORT>, dim3(blocks), dim3(KB_BLOCK), 0, st, p);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return ape_fail(APE_ERR_HIP, "%s: launch failed: %s", what, hipGetErrorString(e));
    return APE_OK;
}

int check_ages(const ape_kalman_bank* b, const int32_t* ages_host, int32_t K, const char* what) {
    for (int j = 0; j < K; ++j)
        if (ages_host[j] < 0 || ages_host[j] > b->W + 1)
            return ape_fail(APE_ERR_INVALID_ARG, "%s: age %d (entry %d) outside [0, W + 1 = %d]", what, ages_host[j], j, b->W + 1);
    return APE_OK;
}

int check_state_desc(const ape_kalman_bank* b, const ape_kalman_state_desc_t* desc, const char* what) {
    ape_kalman_state_desc_t own;
    state_desc_of(b, &own);
    if (desc->version != own.version || desc->E != own.E || desc->W != own.W || desc->smooth != own.smooth ||
        desc->words_per_stream != own.words_per_stream)
        return ape_fail(APE_ERR_INVALID_ARG, "%s: the records are {v%d E=%d W=%d smooth=%d words=%d}, the bank's {v%d E=%d W=%d smooth=%d words=%d}", what,
                     desc->version, desc->E, desc->W, desc->smooth, desc->words_per_stream, own.version, own.E, own.W, own.smooth,
                     own.words_per_stream);
    return APE_OK;
}

// the host side of an import: what the device will hold once the launch has run
void adopt_ages(ape_kalman_bank* b, const int32_t* streams_host, int32_t K, const int32_t* ages_host) {
    for (int j = 0; j < K; ++j) {
        const int s = streams_host ? streams_host[j] : j;
        const char cold = ages_host[j] == 0 ? 1 : 0;
        b->n_pending += (int)cold - (int)b->pending[s];
        b->pending[s] = cold;
        b->age[s] = ages_host[j];
    }
}

}  // namespace

extern "C" {

int ape_kalman_bank_create(ape_kalman_t* model, int32_t n_streams, int32_t smooth, ape_kalman_bank_t** out) {
    if (!model || !out) return ape_fail(APE_ERR_INVALID_ARG, "kalman_bank_create: NULL argument");
    *out = nullptr;
    return bank_make(model, n_streams, smooth, "kalman_bank_create", out);
}

int ape_kalman_bank_destroy(ape_kalman_bank_t* b) {
    if (!b) return APE_OK;
    (void)hipSetDevice(b->device);
    (void)hipDeviceSynchronize();          // frames may still read the rings and the staged lists
    bank_free(b);
    return APE_OK;
}

int ape_kalman_bank_reset(ape_kalman_bank_t* b) {
    if (!b) return ape_fail(APE_ERR_INVALID_ARG, "kalman_bank_reset: NULL bank");
    b->pending.assign((size_t)b->S, 1);
    b->n_pending = b->S;
    b->age.assign((size_t)b->S, 0);
    return APE_OK;
}

int ape_kalman_bank_reset_subset(ape_kalman_bank_t* b, const int32_t* streams_host, int32_t K) {
    if (!b || !streams_host) return ape_fail(APE_ERR_INVALID_ARG, "kalman_bank_reset_subset: NULL argument");
    if (int rc = ape_check_stream_list("kalman_bank_reset_subset", streams_host, K, b->S, true)) return rc;
    for (int j = 0; j < K; ++j) {
        if (!b->pending[streams_host[j]]) { b->pending[streams_host[j]] = 1; b->n_pending += 1; }
        b->age[streams_host[j]] = 0;
    }
    return APE_OK;
}

int ape_kalman_bank_set_norm_stats(ape_kalman_bank_t* b, const double* xx_m, const double* xx_s, const double* yy_m, const double* yy_s) {
    if (!b || !xx_m || !xx_s || !yy_m || !yy_s) return ape_fail(APE_ERR_INVALID_ARG, "kalman_bank_set_norm_stats: NULL argument");
    memcpy(b->xx_m, xx_m, sizeof(b->xx_m));
    memcpy(b->xx_s, xx_s, sizeof(b->xx_s));
    memcpy(b->yy_m, yy_m, sizeof(b->yy_m));
    memcpy(b->yy_s, yy_s, sizeof(b->yy_s));
    b->normalize = true;
    return APE_OK;
}

int ape_kalman_bank_set_body(ape_kalman_bank_t* b, const double body9[9]) {
    if (!b || !body9) return ape_fail(APE_ERR_INVALID_ARG, "kalman_bank_set_body: NULL argument");
    memcpy(b->body, body9, sizeof(b->body));
    if (b->bodies.on()) {                          // table mode: every row (ordered on the null stream: behind every blocking stream's frames)
        std::vector<double> all((size_t)b->S * 9);
        for (int s = 0; s < b->S; ++s) memcpy(&all[(size_t)s * 9], body9, 9 * sizeof(double));
        APE_TRY(hipSetDevice(b->device));
        APE_TRY(ape_body_table_set(b->bodies, b->S, false, b->body, nullptr, b->S, all.data(), nullptr));
    }
    return APE_OK;
}

int ape_kalman_bank_set_bodies(ape_kalman_bank_t* b, const int32_t* streams_host, int32_t K, const double* body9s_host, void* stream) {
    if (!b || !body9s_host) return ape_fail(APE_ERR_INVALID_ARG, "kalman_bank_set_bodies: NULL argument");
    if (int rc = ape_check_stream_list("kalman_bank_set_bodies", streams_host, K, b->S, true)) return rc;
    APE_TRY(hipSetDevice(b->device));
    const hipStream_t st = (hipStream_t)stream;
    if (int rc = check_capture(st, "kalman_bank_set_bodies")) return rc;
    APE_TRY(ape_body_table_set(b->bodies, b->S, false, b->body, streams_host, K, body9s_host, st));
    return APE_OK;
}

int ape_kalman_bank_get_bodies(ape_kalman_bank_t* b, double* out_host) {
    if (!b || !out_host) return ape_fail(APE_ERR_INVALID_ARG, "kalman_bank_get_bodies: NULL argument");
    ape_body_table_get(b->bodies, b->S, b->body, out_host);
    return APE_OK;
}

int ape_kalman_bank_set_seed(ape_kalman_bank_t* b, uint64_t seed) {
    if (!b) return ape_fail(APE_ERR_INVALID_ARG, "kalman_bank_set_seed: NULL bank");
    b->seed = seed;
    b->calls = 0;
    return APE_OK;
}

int ape_kalman_bank_get_draw_position(ape_kalman_bank_t* b, uint64_t* seed, uint64_t* calls) {
    if (!b || !seed || !calls) return ape_fail(APE_ERR_INVALID_ARG, "kalman_bank_get_draw_position: NULL argument");
    *seed = b->seed;
    *calls = b->calls;
    return APE_OK;
}

int ape_kalman_bank_set_draw_position(ape_kalman_bank_t* b, uint64_t seed, uint64_t calls) {
    if (!b) return ape_fail(APE_ERR_INVALID_ARG, "kalman_bank_set_draw_position: NULL bank");
    b->seed = seed;
    b->calls = calls;
    return APE_OK;
}

int ape_kalman_bank_state_desc(ape_kalman_bank_t* b, ape_kalman_state_desc_t* out) {
    if (!b || !out) return ape_fail(APE_ERR_INVALID_ARG, "kalman_bank_state_desc: NULL argument");
    state_desc_of(b, out);
    return APE_OK;
}

int ape_kalman_bank_export(ape_kalman_bank_t* b, const int32_t* streams_host, int32_t K, void* state_dev, int32_t* age_host, void* stream) {
    if (!b || !streams_host || !state_dev || !age_host) return ape_fail(APE_ERR_INVALID_ARG, "kalman_bank_export: NULL argument");
    if (int rc = ape_check_stream_list("kalman_bank_export", streams_host, K, b->S, true)) return rc;
    if (((uintptr_t)state_dev & 15u) != 0) return ape_fail(APE_ERR_INVALID_ARG, "kalman_bank_export: state_dev must be 16-byte aligned");
    APE_TRY(hipSetDevice(b->device));
    const hipStream_t st = (hipStream_t)stream;
    if (int rc = check_capture(st, "kalman_bank_export")) return rc;
    if (K == 0) return APE_OK;
    for (int j = 0; j < K; ++j) age_host[j] = b->age[streams_host[j]];
    return state_launch<false>(b, streams_host, K, age_host, (float*)state_dev, st, "kalman_bank_export");
}

int ape_kalman_bank_import(ape_kalman_bank_t* b, const ape_kalman_state_desc_t* desc, const int32_t* streams_host, int32_t K,
                           const void* state_dev, const int32_t* age_host, void* stream) {
    if (!b || !desc || !streams_host || !state_dev || !age_host) return ape_fail(APE_ERR_INVALID_ARG, "kalman_bank_import: NULL argument");
    if (int rc = check_state_desc(b, desc, "kalman_bank_import")) return rc;
    if (int rc = ape_check_stream_list("kalman_bank_import", streams_host, K, b->S, true)) return rc;
    if (int rc = check_ages(b, age_host, K, "kalman_bank_import")) return rc;
    if (((uintptr_t)state_dev & 15u) != 0) return ape_fail(APE_ERR_INVALID_ARG, "kalman_bank_import: state_dev must be 16-byte aligned");
    APE_TRY(hipSetDevice(b->device));
    const hipStream_t st = (hipStream_t)stream;
    if (int rc = check_capture(st, "kalman_bank_import")) return rc;
    bool carried = false;
    for (int j = 0; j < K; ++j) carried = carried || age_host[j] > 0;
    if (carried)                                              // (age 0 everywhere: ape_kalman_bank_reset_subset, nothing to write)
        if (int rc = state_launch<true>(b, streams_host, K, age_host, (float*)const_cast<void*>(state_dev), st, "kalman_bank_import")) return rc;
    adopt_ages(b, streams_host, K, age_host);
    return APE_OK;
}

int ape_kalman_bank_frame(ape_kalman_bank_t* b, int32_t kind, const float* rows_dev, const int32_t* streams_host, int32_t K,
                          const float* noise_dev, const float* init_noise_dev, uint32_t flags, void* out_dev, int32_t out_dtype,
                          int32_t* n_rows_dev, float* y_dev, void* stream) {
    if (!b || !rows_dev || !out_dev || !n_rows_dev) return ape_fail(APE_ERR_INVALID_ARG, "kalman_bank_frame: NULL argument");
    if (int rc = check_kind(kind, "kalman_bank_frame")) return rc;
    if (out_dtype != APE_F32 && out_dtype != APE_F64) return ape_fail(APE_ERR_INVALID_ARG, "kalman_bank_frame: unknown dtype selector");
    if (flags & ~KB_FLAGS) return ape_fail(APE_ERR_INVALID_ARG, "kalman_bank_frame: flags 0x%x: APE_FLAG_PACKED_MSG and / or APE_FLAG_SPREAD, or 0", flags);
    if (int rc = ape_check_stream_list("kalman_bank_frame", streams_host, K, b->S, true)) return rc;
    APE_TRY(hipSetDevice(b->device));
    const hipStream_t st = (hipStream_t)stream;
    if (int rc = check_capture(st, "kalman_bank_frame")) return rc;
    if (K == 0) return APE_OK;
    return bank_frame(b, kind, rows_dev, streams_host, K, noise_dev, init_noise_dev, flags, out_dev, out_dtype, n_rows_dev, y_dev, st,
                      "kalman_bank_frame");
}

int ape_kalman_bank_frame_host(ape_kalman_bank_t* b, int32_t kind, const float* rows_host, uint32_t flags, void* out_host, int32_t out_dtype,
                               int32_t* n_rows_host, void* stream) {
    if (!b || !rows_host || !out_host || !n_rows_host) return ape_fail(APE_ERR_INVALID_ARG, "kalman_bank_frame_host: NULL argument");
    if (int rc = check_kind(kind, "kalman_bank_frame_host")) return rc;
    if (out_dtype != APE_F32 && out_dtype != APE_F64) return ape_fail(APE_ERR_INVALID_ARG, "kalman_bank_frame_host: unknown dtype selector");
    if (flags & ~KB_FLAGS) return ape_fail(APE_ERR_INVALID_ARG, "kalman_bank_frame_host: flags 0x%x: APE_FLAG_PACKED_MSG and / or APE_FLAG_SPREAD, or 0", flags);
    APE_TRY(hipSetDevice(b->device));                         // (the consumer thread of an estimator starts on device 0)
    const hipStream_t st = (hipStream_t)stream;
    if (int rc = check_capture(st, "kalman_bank_frame_host")) return rc;
    // the head kernel reads the rows from and the tail kernel writes the messages to pinned host memory: no copy commands in the frame
    const size_t rows_bytes = (size_t)b->S * KB_WIDTH * sizeof(float);
    const size_t width = 25 + 6 * (size_t)b->smooth * b->E;                      // (h_out: room for the widest row, record included)
    if (!b->h_rows) APE_TRY(hipHostMalloc((void**)&b->h_rows, rows_bytes, APE_PINNED));
    if (!b->h_out) APE_TRY(hipHostMalloc(&b->h_out, (size_t)b->S * (width + APE_SPREAD_WIDTH) * sizeof(double), APE_PINNED));
    if (!b->h_n) APE_TRY(hipHostMalloc((void**)&b->h_n, (size_t)b->S * sizeof(int), APE_PINNED));
    memcpy(b->h_rows, rows_host, rows_bytes);
    if (int rc = bank_frame(b, kind, b->h_rows, nullptr, b->S, nullptr, nullptr, flags, b->h_out, out_dtype, b->h_n, nullptr, st,
                            "kalman_bank_frame_host"))
        return rc;
    APE_TRY(hipStreamSynchronize(st));
    const size_t w = ((flags & APE_FLAG_PACKED_MSG) ? width : 25) + ((flags & APE_FLAG_SPREAD) ? APE_SPREAD_WIDTH : 0);
    memcpy(out_host, b->h_out, (size_t)b->S * w * (out_dtype == APE_F64 ? sizeof(double) : sizeof(float)));
    memcpy(n_rows_host, b->h_n, (size_t)b->S * sizeof(int));
    return APE_OK;
}

// Host subset frame: the head kernel reads rows and list from the pinned block and lands the list in b->desc for the
// tail, which writes rows, counts and -- K <= 64 -- a completion word per entry into pinned memory.  BLOCKING; the block is reused.
int ape_kalman_bank_frame_subset_host(ape_kalman_bank_t* b, int32_t kind, const float* rows_host, const int32_t* streams_host, int32_t K,
                                      uint32_t flags, void* out_host, int32_t out_dtype, int32_t* n_rows_host, void* stream) {
    if (!b || !rows_host || !out_host || !n_rows_host) return ape_fail(APE_ERR_INVALID_ARG, "kalman_bank_frame_subset_host: NULL argument");
    if (int rc = check_kind(kind, "kalman_bank_frame_subset_host")) return rc;
    if (out_dtype != APE_F32 && out_dtype != APE_F64) return ape_fail(APE_ERR_INVALID_ARG, "kalman_bank_frame_subset_host: unknown dtype selector");
    if (flags & ~KB_FLAGS)
        return ape_fail(APE_ERR_INVALID_ARG, "kalman_bank_frame_subset_host: flags 0x%x: APE_FLAG_PACKED_MSG and / or APE_FLAG_SPREAD, or 0", flags);
    if (int rc = ape_check_stream_list("kalman_bank_frame_subset_host", streams_host, K, b->S, true)) return rc;
    APE_TRY(hipSetDevice(b->device));
    const hipStream_t st = (hipStream_t)stream;
    if (int rc = check_capture(st, "kalman_bank_frame_subset_host")) return rc;
    if (K == 0) return APE_OK;
    const size_t width = 25 + 6 * (size_t)b->smooth * b->E;                      // (h_out: room for the widest row, record included)
    APE_TRY(ape_pinned_zeroed(&b->hs_block, 64 * sizeof(unsigned) + (size_t)b->S * sizeof(KbDesc) + (size_t)b->S * KB_WIDTH * sizeof(float)));
    if (!b->h_out) APE_TRY(hipHostMalloc(&b->h_out, (size_t)b->S * (width + APE_SPREAD_WIDTH) * sizeof(double), APE_PINNED));
    if (!b->h_n) APE_TRY(hipHostMalloc((void**)&b->h_n, (size_t)b->S * sizeof(int), APE_PINNED));
    unsigned* const h_done = reinterpret_cast<unsigned*>(b->hs_block);
    KbDesc* const h_desc = reinterpret_cast<KbDesc*>(b->hs_block + 64 * sizeof(unsigned));
    float* const h_rows = reinterpret_cast<float*>(b->hs_block + 64 * sizeof(unsigned) + (size_t)b->S * sizeof(KbDesc));
    const bool words = K <= 64;
    ape_done_next(&b->hs_done_val);
    memcpy(h_rows, rows_host, (size_t)K * KB_WIDTH * sizeof(float));
    if (int rc = bank_frame(b, kind, h_rows, streams_host, K, nullptr, nullptr, flags, b->h_out, out_dtype, b->h_n, nullptr, st,
                            "kalman_bank_frame_subset_host", h_desc, words ? h_done : nullptr, b->hs_done_val)) {
        (void)hipStreamSynchronize(st);                                          // (a launched head may still read the block the next call rewrites)
        return rc;
    }
    if (!(words && ape_done_wait(h_done, K, b->hs_done_val))) APE_TRY(hipStreamSynchronize(st));   // (as ape_streams_frame_host)
    const size_t w = ((flags & APE_FLAG_PACKED_MSG) ? width : 25) + ((flags & APE_FLAG_SPREAD) ? APE_SPREAD_WIDTH : 0);
    memcpy(out_host, b->h_out, (size_t)K * w * (out_dtype == APE_F64 ? sizeof(double) : sizeof(float)));
    memcpy(n_rows_host, b->h_n, (size_t)K * sizeof(int));
    return APE_OK;
}

int ape_kalman_replay(ape_kalman_t* model, int32_t kind, const float* rows_dev, int32_t F, const int32_t* seg_starts_host, int32_t R,
                      int32_t smooth, const double* xx_m, const double* xx_s, const double* yy_m, const double* yy_s, const double body9[9],
                      uint64_t seed, uint32_t flags, void* out_dev, int32_t out_dtype, int32_t* n_rows_dev, float* y_dev, void* stream) {
    return ape_kalman_replay_resume(model, kind, rows_dev, F, seg_starts_host, R, smooth, xx_m, xx_s, yy_m, yy_s, body9, seed, flags, out_dev,
                                    out_dtype, n_rows_dev, y_dev, stream, nullptr, nullptr, nullptr, nullptr, nullptr, 0);
}

int ape_kalman_replay_bodies(ape_kalman_t* model, int32_t kind, const float* rows_dev, int32_t F, const int32_t* seg_starts_host, int32_t R,
                             int32_t smooth, const double* xx_m, const double* xx_s, const double* yy_m, const double* yy_s,
                             const double body9[9], uint64_t seed, uint32_t flags, void* out_dev, int32_t out_dtype, int32_t* n_rows_dev,
                             float* y_dev, void* stream, const double* bodies_host) {
    return ape_kalman_replay_resume(model, kind, rows_dev, F, seg_starts_host, R, smooth, xx_m, xx_s, yy_m, yy_s, body9, seed, flags, out_dev,
                                    out_dtype, n_rows_dev, y_dev, stream, bodies_host, nullptr, nullptr, nullptr, nullptr, 0);
}

int ape_kalman_replay_resume(ape_kalman_t* model, int32_t kind, const float* rows_dev, int32_t F, const int32_t* seg_starts_host, int32_t R,
                             int32_t smooth, const double* xx_m, const double* xx_s, const double* yy_m, const double* yy_s,
                             const double body9[9], uint64_t seed, uint32_t flags, void* out_dev, int32_t out_dtype, int32_t* n_rows_dev,
                             float* y_dev, void* stream, const double* bodies_host, const void* state_in_dev, const int32_t* age_in_host,
                             void* state_out_dev, int32_t* age_out_host, uint64_t call_base) {
    if (!model || !rows_dev || !out_dev || !n_rows_dev || (!body9 && !bodies_host)) return ape_fail(APE_ERR_INVALID_ARG, "kalman_replay: NULL argument");
    if (int rc = check_kind(kind, "kalman_replay")) return rc;
    if (int rc = ape_check_segments("kalman_replay", F, seg_starts_host, R)) return rc;
    if (smooth > KB_MAX_SMOOTH) return ape_fail(APE_ERR_UNSUPPORTED, "kalman_replay: smooth %d outside 1..%d", smooth, KB_MAX_SMOOTH);
    if (out_dtype != APE_F32 && out_dtype != APE_F64) return ape_fail(APE_ERR_INVALID_ARG, "kalman_replay: unknown dtype selector");
    if (flags & ~KB_FLAGS) return ape_fail(APE_ERR_INVALID_ARG, "kalman_replay: flags 0x%x: APE_FLAG_PACKED_MSG and / or APE_FLAG_SPREAD, or 0", flags);
    const bool any = xx_m || xx_s || yy_m || yy_s;
    if (any && !(xx_m && xx_s && yy_m && yy_s)) return ape_fail(APE_ERR_INVALID_ARG, "kalman_replay: all four statistics or none");
    if (R > 65535) return ape_fail(APE_ERR_INVALID_ARG, "kalman_replay: %d recordings, at most 65535 in one call", R);
    if (!state_in_dev != !age_in_host) return ape_fail(APE_ERR_INVALID_ARG, "kalman_replay: state_in and age_in come together or not at all");
    if (!state_out_dev != !age_out_host) return ape_fail(APE_ERR_INVALID_ARG, "kalman_replay: state_out and age_out come together or not at all");
    if ((((uintptr_t)state_in_dev) | ((uintptr_t)state_out_dev)) & 15u)
        return ape_fail(APE_ERR_INVALID_ARG, "kalman_replay: the record buffers must be 16-byte aligned");
    // ---- from here on the model is read.  The replay is a fresh bank of R streams: frame t lists the recordings that have a row t
    struct Holder {
        ape_kalman_bank* b = nullptr;
        void* descs = nullptr;
        ~Holder() { if (descs) (void)hipFree(descs); if (b) bank_free(b); }
    } hold;
    if (int rc = bank_make(model, R, smooth, "kalman_replay", &hold.b)) return rc;
    ape_kalman_bank* b = hold.b;
    const hipStream_t st = (hipStream_t)stream;
    if (int rc = check_capture(st, "kalman_replay")) return rc;
    if (age_in_host)
        if (int rc = check_ages(b, age_in_host, R, "kalman_replay")) return rc;
    if (any) (void)ape_kalman_bank_set_norm_stats(b, xx_m, xx_s, yy_m, yy_s);
    if (body9) memcpy(b->body, body9, sizeof(b->body));
    // one body per recording: the replay's bank has a stream per recording, so the table's row r is recording r's
    if (bodies_host) APE_TRY(ape_body_table_set(b->bodies, R, false, b->body, nullptr, R, bodies_host, st));
    b->seed = seed;
    b->calls = call_base;
    // recordings that carry a state continue from it: the import writes their rings and counts, their first frame is no cold start
    bool carried = false;
    for (int r = 0; r < R && age_in_host; ++r) carried = carried || age_in_host[r] > 0;
    if (carried)
        if (int rc = state_launch<true>(b, nullptr, R, age_in_host, (float*)const_cast<void*>(state_in_dev), st, "kalman_replay")) return rc;
    std::vector<int> len((size_t)R);
    int longest = 0;
    for (int r = 0; r < R; ++r) {
        len[r] = (r + 1 < R ? seg_starts_host[r + 1] : F) - seg_starts_host[r];
        if (len[r] > longest) longest = len[r];
    }
    std::vector<KbDesc> descs;
    descs.reserve((size_t)F);
    std::vector<int> first((size_t)longest + 1, 0);
    for (int t = 0; t < longest; ++t) {
        for (int r = 0; r < R; ++r)
            if (len[r] > t)
                descs.push_back(KbDesc{r, t == 0 && !(age_in_host && age_in_host[r] > 0) ? 1 : 0, seg_starts_host[r] + t, seg_starts_host[r] + t});
        first[t + 1] = (int)descs.size();
    }
    APE_TRY(hipMalloc(&hold.descs, descs.size() * sizeof(KbDesc)));
    APE_TRY(hipMemcpyAsync(hold.descs, descs.data(), descs.size() * sizeof(KbDesc), hipMemcpyHostToDevice, st));
    int rc = APE_OK;
    for (int t = 0; t < longest && rc == APE_OK; ++t)
        rc = frame_launch(b, (kind & APE_PARSE_BIG_ENDIAN) ? 1 : 0, rows_dev, (const KbDesc*)hold.descs + first[t], 0, first[t + 1] - first[t],
                          nullptr, nullptr, flags, out_dev, out_dtype, n_rows_dev, y_dev, st, "kalman_replay");
    if (rc == APE_OK && state_out_dev) {                      // every recording has a row: no age is 0
        for (int r = 0; r < R; ++r) {
            const long long a = (long long)(age_in_host ? age_in_host[r] : 0) + len[r];
            age_out_host[r] = (int32_t)(a > b->W + 1 ? b->W + 1 : a);
        }
        rc = state_launch<false>(b, nullptr, R, age_out_host, (float*)state_out_dev, st, "kalman_replay");
    }
    const hipError_t e = hipStreamSynchronize(st);            // the bank and the lists are freed behind this
    if (rc != APE_OK) return rc;
    if (e != hipSuccess) return ape_fail(APE_ERR_HIP, "kalman_replay: synchronise failed: %s", hipGetErrorString(e));
    return APE_OK;
}

}  // extern "C"
