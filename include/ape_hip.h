/*
 * ape_hip.h -- C ABI of libape_hip.so: the MI355X (gfx950) implementation of the per-frame
 * arm-pose inference path of wear_mocap_ape.
 *
 * The reference (pure Python) has no FFI; its boundary for this path is the Python
 * `Estimator` template-method contract.  The entry points below are
 * exactly what a reference-side ctypes binding for that path would call; each one names the
 * reference code it replaces (paths relative to /root/reference/src/wear_mocap_ape).  The
 * binding a maintainer would add is shown in INTEGRATION.md; the host-side mirror of the
 * reference classes that uses it lives in arm-pose-estimation_amd/wear_mocap_ape_amd/.
 *
 * Conventions
 *   - plain C: opaque handle, raw pointers, sizes; no torch / C++ types.
 *   - every `*_dev` pointer is DEVICE memory on the model's GPU (e.g. tensor.data_ptr()),
 *     row-major, contiguous.  `stream` is a hipStream_t passed as void* (NULL = default
 *     stream).  Calls enqueue work on `stream` and return without synchronising; they
 *     perform no allocation once `ape_model_reserve` covers the batch (graph-capture safe).
 *   - return value 0 = success; anything else is an APE_ERR_* code and `ape_last_error()`
 *     (thread-local) describes it.  The Python mirror raises `UserWarning` for a non-zero
 *     status, the reference's exception convention (nn_models.py:385-400, transformations.py:98-116).
 *   - ONE model handle serialises on ONE stream at a time: the handle owns the exchange buffers, flag words, arrival
 *     tickets and workspaces its kernels use, so two calls on the same handle (ape_lstm_forward, ape_infer,
 *     ape_streams_step of any bank built on it) must not run concurrently -- enqueue them on the same stream, or
 *     order the streams with events.  Use one handle per concurrently running stream/thread (reference: one
 *     Estimator, with its own model, per consumer thread, estimator.py:139-143).  Different handles are independent.
 *   - a launch of the weight-stationary kernels that cannot make progress (its workgroups never all resident, e.g. on
 *     a GPU shared with other long-running kernels) gives up after a bounded wait, sets a sticky status word and
 *     leaves its outputs unwritten; every later launch on that handle then leaves at once, also without writing.
 *     ape_model_check() reports (and clears) that state; ape_model_recover() does the same and then RE-ISSUES every
 *     call made on the handle since its last successful check on the kernels that need no co-residency (the batch-tile
 *     LSTM / MLP kernels), on the streams the calls named, so that no frame is lost: call one of them wherever results
 *     are consumed on the host (the Python mirror calls ape_model_recover whenever it copies results to host memory).
 *   - quaternions are [w,x,y,z]; all joint/column indices are fixed by the layouts below.
 */
#ifndef APE_HIP_H
#define APE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define APE_ABI_VERSION 7

/* ---- status codes ---------------------------------------------------------------------- */
enum {
    APE_OK = 0,
    APE_ERR_INVALID_ARG = 1,   /* NULL pointer, non-positive size, unknown enum value           */
    APE_ERR_UNSUPPORTED = 2,   /* dims outside what the gfx950 kernels are built for            */
    APE_ERR_NOT_READY = 3,     /* weights / norm stats not loaded yet                           */
    APE_ERR_HIP = 4,           /* a HIP runtime call failed (message carries hipGetErrorString) */
    APE_ERR_NO_DEVICE = 5,     /* no usable gfx950 device: there is NO CPU fallback             */
    APE_ERR_CAPACITY = 6       /* batch larger than ape_model_reserve()d workspace during capture */
};

/* ---- NN-target layouts: utility/names.py:4-29 (NNS_TARGETS) -------------------------------
 * est row layouts: estimate/estimate_joints.py:48-71 / :74-92 / :20-45
 *   APE_LAYOUT_ORI_CAL_LARM_UARM_HIPS      O=14 -> est[21] = hand(0:3) larm_orig(3:6) uarm_orig(6:9)
 *                                                           larm_q(9:13) uarm_q(13:17) hips_q(17:21)
 *   APE_LAYOUT_ORI_CAL_LARM_UARM           O=12 -> est[14] = hand(0:3) larm_orig(3:6) larm_q(6:10) uarm_q(10:14)
 *   APE_LAYOUT_ORI_POS_CAL_LARM_UARM_HIPS  O=20 -> est[21] (same columns as the first)
 * message layout (all three): estimate/compose_msg.py:72-78
 *   msg[25] = hand_rot(0:4, == larm_rot) hand_orig(4:7) larm_rot(7:11) larm_orig(11:14)
 *             uarm_rot(14:18) uarm_orig(18:21) hips_rot(21:25)
 */
enum {
    APE_LAYOUT_NONE = -1,                    /* regressor only: ape_fk / ape_msg_reduce / ape_infer refuse */
    APE_LAYOUT_ORI_CAL_LARM_UARM_HIPS = 0,
    APE_LAYOUT_ORI_CAL_LARM_UARM = 1,
    APE_LAYOUT_ORI_POS_CAL_LARM_UARM_HIPS = 2
};

enum { APE_F32 = 0, APE_F64 = 1 };   /* element type selector for preds / est buffers */

/* ---- flags for ape_lstm_forward / ape_infer ---------------------------------------------- */
#define APE_FLAG_NORMALIZE_INPUT 0x1u /* x is raw features: z-score in f64, cast f32 (estimator.py:103-104,
                                         watch_phone_pocket_nn.py:100); else x is already normalised  */
#define APE_FLAG_ALL_STEPS       0x2u /* y is [B,T,O] like DropoutLSTM.forward (nn_models.py:188-189);
                                         else only the last step [B,O] (watch_phone_pocket_nn.py:111)   */
#define APE_FLAG_DROPOUT_MASKS   0x4u /* inter-layer dropout with caller-supplied masks (train-mode LSTM
                                         after monte_carlo_predictions, nn_models.py:204)               */
#define APE_FLAG_DROPOUT_PHILOX  0x8u /* inter-layer dropout with an in-kernel counter-based generator  */

/* ---- Random numbers: the counter and key layout of every device-side draw (PART OF THE CONTRACT) ------------------------------------
 * Every draw is Philox4x32-10 (Salmon et al. 2011; multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85) of a
 * 128-bit counter (c0, c1, c2, c3) under the 64-bit key of the call: k0 = seed & 0xFFFFFFFF, k1 = seed >> 32.  A draw is therefore a
 * function of (row, step, unit, layer, seed) alone -- never of the kernel, the launch split or the placement -- which is what
 * sample_row_base, the chunked launches and the stream-state hand-over rely on, and what lets a host compute the very numbers
 * (oracle/philox.py; tests/test_philox_routes_gpu.py and tests/test_kalman_draws_gpu.py hold every route to it).
 *   LSTM dropout     multiplier on the output of model layer l < L-1, global row b of the call, step t, hidden unit u:
 *                    counter (b & ~3, t, u, l), word b & 3;  uf = float(w >> 8) * 2^-24;  keep iff uf >= dropout_p, multiplier
 *                    1.0f / (1.0f - dropout_p).  Global row: the row of the caller's batch whatever the launch split; stream * n_mc + sample
 *                    in a lockstep bank frame; list position * n_mc + sample in a subset frame; frame * n_mc + sample (+ sample_row_base)
 *                    in a replay.  Keys: `seed` as given to ape_lstm_forward / ape_replay*; seed + c in a bank, c = the Monte-Carlo
 *                    frames the bank has issued since ape_streams_set_mc (lockstep and subset frames count alike; no reset rewinds it).
 *   DropoutFF        batch kernel: counter (row & ~3, 0, column, 0xFF), word row & 3, row = the row of the call;
 *                    bank / replay head: counter (lo32(r), hi32(r), unit >> 2, 0xFE), word unit & 3, r = global sample row + sample_row_base.
 *                    Same uf, comparison and multiplier.
 *   Kalman normals   standard normal number idx of stream `tag`: counter (idx >> 2, tag, 0x4B414C4D, 0), Box-Muller on the word pair
 *                    (idx >> 1) & 1:  u = (float(w[2 pair] >> 8) + 1) * 2^-24,  r = sqrtf(-2 logf(u)),
 *                    a = (6.2831855f * float(w[2 pair + 1])) * 2^-32,  r cosf(a) for even idx, r sinf(a) for odd.
 *                    tag 0x100 + 2 j: weight perturbation of flipout layer j (idx = n * K + k), 0x101 + 2 j: its bias perturbation;
 *                    tag 0x300: format_state and the bank's init draws (idx = flat index of [K, E, 14]).
 *   Kalman signs     +-1 number (row r, column c) of sign stream `tag`: counter (c >> 7, r, tag, 0x5349474E), word (c >> 5) & 3,
 *                    bit c & 31, set = -1.  tag 0x200 + 2 i: sign_in of the layer with blob index i, 0x201 + 2 i: its sign_out.
 *   Kalman keys      call number n (1 for the first) after the seed was set: seed + 0xD1342543DE82EF95 * n mod 2^64; one key for all
 *                    draws of a forward / format_state / bank frame. */

/* LSTM kernel selection (ape_model_set_kernel).  AUTO = the weight-stationary cluster kernel where it is
 * built (H=256/L=2/I<=32 and H=128/L=3/32<I<=64; dropout up to 32 windows per cluster), else the batch-tile kernel. */
enum { APE_KERNEL_AUTO = 0, APE_KERNEL_TILE16 = 1, APE_KERNEL_CLUSTER = 2,
       APE_KERNEL_CLUSTER_GEN1 = 3 /* the cluster kernels, first generation only: A/B runs against lstm_cluster32.hip */,
       APE_KERNEL_AUTO_GEN1 = 4    /* AUTO's dispatch without the second-generation kernels (lstm_cluster32.hip, and
                                      lstm_upper32.hip in a Monte-Carlo stream bank): A/B runs, tests */ };

/* Storage precision of W, x and h inside the LSTM (ape_model_set_precision).  F32 (default): exact float32
 * MFMA.  F16: binary16 weights / inputs / hidden state with float32 accumulate, cell state and head
 * (BASELINE.json configs[4]); last-step output without dropout; parity to a stated tolerance only.
 * F16_GEN1: the same arithmetic on the first-generation fp16 kernel for every batch size (A/B runs, tests); F16
 * serves batches above 256 rows of the 2 x 256 models with the row-set-pipelined kernel. */
enum { APE_PRECISION_F32 = 0, APE_PRECISION_F16 = 1, APE_PRECISION_F16_GEN1 = 2 };

#define APE_FLAG_PACKED_MSG      0x20u /* ape_streams_step only: message and tail of a stream packed in one row  */
#define APE_FLAG_SPREAD          0x40u /* frames, banks and replays (NOT ape_lstm_forward / ape_infer, which refuse it): every output row
                                         grows by APE_SPREAD_WIDTH columns at its end, the Monte-Carlo spread record below             */
#define APE_FLAG_BROADCAST_X     0x10u /* x_dev is ONE window [1,T,I] shared by all B rows: the x.repeat((n,1,1)) of
                                         monte_carlo_predictions (nn_models.py:206) without materialising it    */

/* Exchange-form selectors of the weight-stationary kernels, for A/B runs and tests (ape_lstm_forward, ape_infer, ape_streams_step).  They
 * change HOW the workgroups of a cluster hand their slices over, never the arithmetic: results are bit-equal (ALT_FORM: equal up to
 * float32 summation order).  Every other undeclared bit is refused.
 * DEFAULT hand-over of every flag-based kernel (round 5): payload by write-through (`sc1`) stores, every storing wave waits for its
 * stores, then its flag (an agent-scope store); every load of handed-off bytes is an `sc1` load -- the form the MI355X guide lists as
 * valid wherever the workgroups run. */
#define APE_FLAG_ANY_PLACEMENT   0x08000000u /* the two tagged-granule latency kernels (lstm_cluster_small / lstm_mc_small): write-through
                                               granule stores also where the members share an XCD.  A no-op for the flag-based kernels,
                                               whose default it names since round 5 */
#define APE_FLAG_IN_XCD_PLAIN    0x00400000u /* OPT-IN, A/B runs and tests only: payload by plain (write-back) stores where all members of a
                                               cluster were verified to share an XCD (the default until round 4; 1-2 % faster in float32,
                                               10 % in fp16).  OUTSIDE the guide's table of valid forms: a plain store behind
                                               `s_waitcnt vmcnt(0)` is no agent-scope release.  Same bits when it holds */
#define APE_FLAG_NO_XCD_CLASSES  0x02000000u /* first-generation cluster kernel: clusters by global arrival ticket instead of within
                                               block-index classes (one XCD each) */
#define APE_FLAG_ALT_FORM        0x01000000u /* the alternative decomposition where a kernel has two: the latency kernel's H/16-member form,
                                               lstm_cluster16's one-workgroup-per-CU form, the fp16 kernel's 16-unit-member form (two
                                               workgroups per CU; measured slower), ImuPoseLSTM's one-tile clusters on the
                                               blocking exchange instead of the gather under the input span (same bits) */

typedef struct ape_model ape_model_t;

/* DropoutLSTM(input_size, hidden_layer_size, hidden_layer_count, output_size) -- nn_models.py:160-178,
 * constructed as load_deployed_model_from_hash does (nn_models.py:402-408). */
/* regressor architectures the reference loader dispatches (nn_models.py:393-400) */
enum {
    APE_MODEL_LSTM = 0,   /* DropoutLSTM  nn_models.py:160-207 */
    APE_MODEL_FF = 1,     /* DropoutFF    nn_models.py:313-370 : Linear, n x Linear (leaky_relu), dropout, Linear */
    APE_MODEL_IMUPOSE = 2 /* ImuPoseLSTM  nn_models.py:210-249 : Linear(I,256)+ReLU, fixed 2 x 256 LSTM, Linear(256,O);
                             hidden_size must be 256 and num_layers 2 (the reference ignores its ctor arguments) */
};

typedef struct ape_dims {
    int32_t input_size;    /* I: 20 / 22 / 38 (<= 64)                      */
    int32_t hidden_size;   /* H: 128 or 256                                */
    int32_t num_layers;    /* L: 1..3                                      */
    int32_t output_size;   /* O: 12 / 14 / 20 (<= 32)                      */
    int32_t target_layout; /* APE_LAYOUT_*; O must match it (unless NONE)  */
    int32_t device;        /* HIP device ordinal                           */
    int32_t model_kind;    /* APE_MODEL_*; for APE_MODEL_FF num_layers is hidden_layer_count (0..7) */
} ape_dims_t;

/* library / device --------------------------------------------------------------------------- */
int ape_abi_version(void);
const char* ape_last_error(void);
/* number of visible HIP devices whose arch is gfx950 (0 on a CPU-only host; never fails) */
int ape_device_count(void);

/* lifetime ------------------------------------------------------------------------------------ */
/* replaces: nn_models.DropoutLSTM.__init__ (nn_models.py:161-178) + Estimator.__init__ defaults
 * (estimator.py:57-68: default body measurements are installed) */
int ape_model_create(const ape_dims_t* dims, ape_model_t** out_model);
int ape_model_destroy(ape_model_t* model);
/* pre-allocate the [max_batch, O] intermediate so that later calls do not allocate */
int ape_model_reserve(ape_model_t* model, int32_t max_batch);

/* replaces: nn_model.load_state_dict(model_state) (nn_models.py:410-411).
 * `blob` = float32 tensors concatenated in state_dict order:
 *   for k in 0..L-1: lstm.weight_ih_l{k} [4H, I or H], lstm.weight_hh_l{k} [4H,H],
 *                    lstm.bias_ih_l{k} [4H], lstm.bias_hh_l{k} [4H];
 *   then output_layer.weight [O,H], output_layer.bias [O].
 * APE_MODEL_FF: _input_layer.weight [H,I], .bias [H]; _hidden_layers.{k}.weight [H,H], .bias [H] for k in
 *   0..hidden_layer_count-1; _output_layer.weight [O,H], .bias [O]   (state_dict order of DropoutFF).
 * APE_MODEL_IMUPOSE: input_layer.weight [256,I], .bias [256]; then the APE_MODEL_LSTM tensors with a 256-wide
 *   layer-0 input (state_dict order of ImuPoseLSTM).
 * `blob` may be host or device memory (e.g. the buffer an RCCL broadcast just filled);
 * `n_floats` must equal ape_weight_blob_floats(dims).  Synchronous; init-time only. */
int ape_model_load_weights(ape_model_t* model, const float* blob, size_t n_floats);
size_t ape_weight_blob_floats(const ape_dims_t* dims);

/* replaces: Estimator.__init__ stats load / Estimator.set_norm_stats (estimator.py:35-42,72-77).
 * Host pointers, float64: xx_m, xx_s [I]; yy_m, yy_s [O]. */
int ape_model_set_norm_stats(ape_model_t* model, const double* xx_m, const double* xx_s,
                             const double* yy_m, const double* yy_s);
/* replaces: Estimator._body_measurements (estimator.py:57-68): [larm_vec(3), uarm_vec(3), uarm_orig_rh(3)] */
int ape_model_set_body(ape_model_t* model, const double body9[9]);

/* hot path ------------------------------------------------------------------------------------ */
/* replaces: DropoutLSTM.forward / monte_carlo_predictions (nn_models.py:180-207) as called from
 * make_prediction_from_row_hist (watch_phone_pocket_nn.py:98-112, watch_only.py:84-97,
 * watch_phone_uarm_nn.py:107-121).  h0 = c0 = 0 for every window (hs=None).
 *   x_dev      f32 [B,T,I]
 *   masks_dev  f32 [L-1,B,T,H] holding 0 or 1/(1-p)   (APE_FLAG_DROPOUT_MASKS; else NULL)
 *   dropout_p, seed                                   (APE_FLAG_DROPOUT_PHILOX)
 *   y_dev      f32 [B,O] or [B,T,O] (APE_FLAG_ALL_STEPS): normalised NN targets
 * APE_MODEL_FF (DropoutFF.forward / monte_carlo_predictions, nn_models.py:340-370): the MLP is applied to the
 *   last step of every window (or to all B*T rows with APE_FLAG_ALL_STEPS); masks_dev is f32 [rows,H], the
 *   dropout in front of the output layer.
 * APE_MODEL_IMUPOSE (ImuPoseLSTM.forward, nn_models.py:236-244): as APE_MODEL_LSTM, no dropout modes (its
 *   monte_carlo_predictions is the plain forward, :246-251). */
int ape_lstm_forward(ape_model_t* model, const float* x_dev, int32_t B, int32_t T, uint32_t flags,
                     const float* masks_dev, float dropout_p, uint64_t seed,
                     float* y_dev, void* stream);
/* the same with a caller-given initial state: DropoutLSTM.forward(x, hs=(h0, c0)) (nn_models.py:180-189 hands hs to
 * nn.LSTM).  h0_dev, c0_dev: f32 [L,B,H] (both or neither; NULL, NULL = ape_lstm_forward).  Not for APE_MODEL_FF
 * and not with the fp16 variant. */
int ape_lstm_forward_hs(ape_model_t* model, const float* x_dev, int32_t B, int32_t T, uint32_t flags,
                        const float* masks_dev, float dropout_p, uint64_t seed,
                        const float* h0_dev, const float* c0_dev, float* y_dev, void* stream);

/* replaces: estimate_joints.arm_pose_from_nn_targets (estimate_joints.py:16-17) and, with
 * `denormalize` != 0, the `pred * yy_s + yy_m` of estimator.py:108-109 in front of it.
 *   preds_dev  [N,O] of preds_dtype;  est_dev [N,W] of est_dtype (W = 21 or 14).
 * All arithmetic is float64 on the device whatever the storage types. */
int ape_fk(ape_model_t* model, const void* preds_dev, int32_t preds_dtype, int32_t N,
           int32_t denormalize, void* est_dev, int32_t est_dtype, void* stream);

/* replaces: compose_msg.msg_from_nn_targets_est (compose_msg.py:13-14): N est rows -> msg[25].
 * N > 1: sign-aligned quaternion means (transformations.py:32-51) and origins recomputed from
 * them; N == 1: row 0 copied into the message layout.  est_dev f64 [N,W]; msg_dev f64 [25]. */
int ape_msg_reduce(ape_model_t* model, const double* est_dev, int32_t N, double* msg_dev, void* stream);

/* feature builder, batched.  replaces: parse_row_to_xx of WatchPhonePocketNN
 * (watch_phone_pocket_nn.py:41-96), WatchOnlyNN (watch_only.py:46-82; also with the 55-float watch+phone
 * message, watch_only.py:29-32) and WatchPhoneUarmNN (watch_phone_uarm_nn.py:43-105).
 *   rows_dev f32 [N,55] (or [N,28] for APE_PARSE_WATCH_ONLY): raw messages, data_types/messaging.py layouts
 *   xx_dev   [N,22|20|20|38] of xx_dtype (the reference returns float32, float64 for the upper-arm variant)
 * float64 arithmetic on the device.  Needs no model: runs on the current HIP device. */
enum {
    APE_PARSE_WATCH_PHONE_POCKET = 0,   /* 55 -> 22 */
    APE_PARSE_WATCH_ONLY = 1,           /* 28 -> 20 */
    APE_PARSE_WATCH_ONLY_PHONE_MSG = 2, /* 55 -> 20 */
    APE_PARSE_WATCH_PHONE_UARM = 3,     /* 55 -> 38 */
    /* OR-ed into a kind: the rows are UDP payloads as received -- big-endian float32
     * (stream_listener/imu.py:53,68-69 unpacks them with '>f'); default is native float32 */
    APE_PARSE_BIG_ENDIAN = 0x100
};
int ape_parse_rows(int32_t kind, const float* rows_dev, int32_t N, void* xx_dev, int32_t xx_dtype, void* stream);

/* the whole batched path in one call: x -> [normalise] -> LSTM -> last step ->
 * de-normalise -> FK.  y_dev (f32 [B,O], normalised NN targets) may be NULL. */
/* stream bank: the per-frame step of S independent wearable streams, state resident on the device (SURVEY.md 8a-1,
 * 8a-15, 8f-2).  replaces, for all streams at once, Estimator.add_xx_to_row_hist_and_make_prediction
 * (estimator.py:93-120: window of the last seq_len feature rows, padded with the newest row on a cold start :96-97;
 * z-score; model; de-normalise; smoothing stack of the last `smooth` predictions, padded the same way :112-118) and
 * Estimator.msg_from_pred (:122-137) with one Monte-Carlo sample per stream (deterministic weights).
 *   ape_streams_push_rows      rows_dev f32 [S,55|28] raw messages of `kind` (ape_parse_rows kinds, may carry
 *                              APE_PARSE_BIG_ENDIAN) -> features -> next slot of every stream's window ring
 *   ape_streams_push_features  xx_dev f32 [S,I]: the same for callers that build features themselves
 *   ape_streams_step           one prediction per stream from the current windows:
 *                              msg_dev  [S,25] of out_dtype, layout of compose_msg.py:72-78
 *                              tail_dev [S,smooth,6] of out_dtype or NULL: hand and elbow xyz of every smoothing row
 *                              (what msg_from_pred appends to the message when add_mc_samples is set and smooth > 1)
 *                              flags: APE_FLAG_NORMALIZE_INPUT and / or APE_FLAG_PACKED_MSG.  PACKED_MSG:
 *                              msg_dev is [S, 25+6N] of out_dtype (N = smooth*n_mc stacked rows), every row the
 *                              message followed by its tail = the list Estimator.msg_from_pred returns
 *                              (estimator.py:131-137); as APE_F32 it is byte for byte the payload the reference sends
 *                              per estimator (pose_est_udp.py:47 struct.pack('f'*len(msg))); tail_dev must be NULL
 *   ape_streams_reset          cold start: the next row fills the whole window, the next prediction the whole stack
 *   ape_streams_set_mc         Monte-Carlo dropout per stream, as every reference estimator runs it
 *                              (monte_carlo_samples, watch_phone_pocket_nn.py:105-110 -> nn_models.py:191-207): each
 *                              frame runs every stream's window n_mc times with independent inter-layer dropout
 *                              masks (in-kernel Philox, keyed by `seed` + the bank's frame counter: "Random numbers" above), the smoothing stack
 *                              holds smooth x n_mc rows per stream in the reference's order (estimator.py:112-118:
 *                              oldest prediction first, its n_mc samples in order), tail_dev becomes
 *                              [S, smooth*n_mc, 6].  dropout_p = 0 gives n_mc identical samples.  Call it before the
 *                              first row is pushed or right after ape_streams_reset (it re-allocates the rings and
 *                              implies a reset); smooth*n_mc <= 4096.
 * One bank = one model handle = one HIP stream at a time.  smooth <= 64. */
typedef struct ape_streams ape_streams_t;
int ape_streams_create(ape_model_t* model, int32_t n_streams, int32_t seq_len, int32_t smooth, ape_streams_t** out_bank);
int ape_streams_destroy(ape_streams_t* bank);
int ape_streams_reset(ape_streams_t* bank);
int ape_streams_set_mc(ape_streams_t* bank, int32_t n_mc, float dropout_p, uint64_t seed);
int ape_streams_push_rows(ape_streams_t* bank, int32_t kind, const float* rows_dev, void* stream);
int ape_streams_push_features(ape_streams_t* bank, const float* xx_dev, void* stream);
int ape_streams_step(ape_streams_t* bank, uint32_t flags, void* msg_dev, void* tail_dev, int32_t out_dtype, void* stream);
/* ONE iteration of Estimator.processing_loop (estimator.py:174-177: parse_row_to_xx -> add_xx_to_row_hist_and_make_prediction
 * -> msg_from_pred) for every stream of the bank, with HOST buffers (ABI 6): what the drop-in Estimator classes call per frame.
 *   rows_host  f32 [S,55|28] raw messages of `kind` (may carry APE_PARSE_BIG_ENDIAN), ordinary host memory
 *   out_host   [S, 25+6N] of out_dtype (N = smooth*n_mc): message + tail of every stream, ordinary host memory
 *   flags      APE_FLAG_NORMALIZE_INPUT or 0
 * = ape_streams_push_rows + ape_streams_step(PACKED_MSG) + the copies either side, BLOCKING: the rows travel through pinned
 * staging the kernels read and write directly (no copy command on the stream), the call returns when out_host is filled.
 * The health of the frame's launches is part of the frame: an aborted weight-stationary launch is re-issued as by
 * ape_model_recover before the call returns, and a clean frame clears the handle's journal. */
int ape_streams_frame_host(ape_streams_t* bank, int32_t kind, const float* rows_host, uint32_t flags, void* out_host,
                           int32_t out_dtype, void* stream);
/* where a host frame's time goes (ABI 7; bench.py `batch1.estimator_loop`): ape_streams_frame_host keeps, for the last 4096 frames, the
 * host time spent (us) in [0] the rows' copy into pinned staging + the frame's launch calls, [1] the wait from the last launch call's
 * return to all completion words seen (or the stream synchronised), [2] the copy of the pinned output into out_host; and counts the frames
 * whose completion words were NOT seen within the poll budget and fell through to hipStreamSynchronize.  `trace_us` (may be NULL):
 * [n][3] floats, oldest frame first, n = min(frames since the last reset, capacity_frames, 4096) -> *n_out.  reset != 0 clears. */
typedef struct ape_frame_stats {
    uint64_t frames;           /* ape_streams_frame_host calls since the last reset        */
    uint64_t fallback_syncs;   /* ... of them, frames that ended in hipStreamSynchronize   */
    uint64_t recovered;        /* ... frames whose cooperative launch gave up and was re-issued */
} ape_frame_stats_t;
int ape_streams_frame_stats(ape_streams_t* bank, ape_frame_stats_t* out, float* trace_us, int32_t capacity_frames, int32_t* n_out,
                            int32_t reset);
/* measurement aid (bench.py `stream_bank_T6.*.roofline`): with profiling on, every launch of the step's dominant kernel (the
 * regressor: ape_lstm_upper32 in a Monte-Carlo bank, else the LSTM launch) is bracketed by a pair of HIP events on the
 * step's own stream; ape_streams_profile_read synchronises, returns the summed duration and the number of launches since
 * the last read, and re-arms.  At most 256 launches are recorded between two reads; off by default (two event records
 * per launch otherwise). */
int ape_streams_profile(ape_streams_t* bank, int32_t enable);
int ape_streams_profile_read(ape_streams_t* bank, double* kernel_ms_sum, int32_t* launches);

int ape_infer(ape_model_t* model, const float* x_dev, int32_t B, int32_t T, uint32_t flags,
              float* y_dev, void* est_dev, int32_t est_dtype, void* stream);

/* offline replay (additive in ABI 7).  replaces, for every row of one or more recordings, what
 * Estimator.processing_loop does per row (parse_row_to_xx -> add_xx_to_row_hist_and_make_prediction -> msg_from_pred,
 * estimator.py:93-137), with no row skipped (the live loop's queue skip-ahead, estimator.py:159-161, is not applied).
 *   kind            ape_parse_rows kind, may carry APE_PARSE_BIG_ENDIAN
 *   rows_dev        f32 [F, 55|28] raw rows, the recordings back to back
 *   seg_starts_host R >= 1 recording starts (host memory): [0] == 0, strictly rising, < F.  Every recording starts cold, as
 *                   after ape_streams_reset: windows and smoothing stacks never reach across a start
 *   seq_len, smooth window length and smoothing stack (smooth <= 64, smooth*n_mc <= 4096)
 *   n_mc, dropout_p, seed  Monte-Carlo samples: those of ONE ape_lstm_forward(APE_FLAG_DROPOUT_PHILOX, dropout_p, seed) over the
 *                   explicitly repeated windows [F*n_mc, T, I], sample row f*n_mc + k = sample k of frame f (F*n_mc < 2^31);
 *                   independent of max_rows_per_launch and of the kernel route.  dropout_p = 0 (or one layer): no dropout
 *   flags           APE_FLAG_NORMALIZE_INPUT, APE_FLAG_PACKED_MSG
 *   out_dev         [F, 25] of out_dtype; with APE_FLAG_PACKED_MSG and N = smooth*n_mc > 1, [F, 25+6N]: row f is what a fresh
 *                   estimator fed that recording's rows in order returns for its row f (message + hand / elbow xyz of every
 *                   stacked row, the layout of ape_streams_step's PACKED_MSG rows)
 *   y_dev           optional f32 [F, n_mc, O]: the normalised NN targets
 *   max_rows_per_launch  bound on the sample rows of one regressor launch (0 = default, else >= 16): device workspace is
 *                   O(F) for the features plus O(max_rows_per_launch), whatever F*n_mc
 * BLOCKING: returns after the model's health check; an aborted weight-stationary launch is run again on the kernels that
 * need no co-residency before the call returns.  Refused (non-zero, ape_last_error): bad kind / width, F < 1, bad starts,
 * fp16 precision on the model, APE_MODEL_FF / APE_MODEL_IMUPOSE models (ape_replay_regressor below serves those), a capturing stream. */
int ape_replay(ape_model_t* model, int32_t kind, const float* rows_dev, int32_t F, const int32_t* seg_starts_host, int32_t R,
               int32_t seq_len, int32_t smooth, int32_t n_mc, float dropout_p, uint64_t seed, uint32_t flags,
               void* out_dev, int32_t out_dtype, float* y_dev, int32_t max_rows_per_launch, void* stream);

/* subset frames of a stream bank (additive in ABI 7): each stream behaves like its own reference Estimator fed only
 * the rows addressed to it -- its own window, its own smoothing stack, its own cold start (estimator.py:93-137).
 * ape_streams_frame_subset: for each of K DISTINCT streams listed in streams_host (host memory), what process_row does with one row:
 * parse it, push it onto that stream's window (the first row since its cold start pads the whole window), run the regressor (n_mc
 * samples in Monte-Carlo mode), push the prediction onto that stream's stack (the first since its cold start pads the whole stack),
 * reduce the stack to the message.  Streams not listed stay bit for bit untouched.
 *   kind           ape_parse_rows kind, may carry APE_PARSE_BIG_ENDIAN
 *   rows_dev       f32 [K, 55|28] on the device: row j belongs to stream streams_host[j]
 *   flags          APE_FLAG_NORMALIZE_INPUT, APE_FLAG_PACKED_MSG
 *   out_dev        [K, 25] of out_dtype in list order; with APE_FLAG_PACKED_MSG and N = smooth*n_mc > 1, [K, 25+6N] in the packed-row
 *                  layout of ape_streams_step
 * Monte-Carlo samples: those of ONE ape_lstm_forward(APE_FLAG_DROPOUT_PHILOX, dropout_p, seed + c) over the explicitly repeated
 * windows [K*n_mc, T, I] in list order, c = the bank's call counter (one per frame) -- a stream's samples depend on its position in
 * the list.  K = 0 is a no-op.  Asynchronous on `stream` (frames may be enqueued back to back); journaled like a step:
 * ape_model_recover re-issues the newest subset frame of a bank (regressor and post-filter only) when called behind it, before the
 * bank's next frame is enqueued.
 * Per-stream mode: the first subset call (either entry) seeds per-stream counters from the bank's lockstep ones, so that a lockstep
 * history carries on; from then on ape_streams_push_rows / push_features / step / frame_host are refused with APE_ERR_NOT_READY until
 * ape_streams_reset (or ape_streams_set_mc) cold-starts every stream and returns the bank to lockstep.
 * ape_streams_reset_subset: cold-starts the K listed streams only.
 * Refused (non-zero, ape_last_error): NULL arguments, K < 0 or K > S, an index outside [0, S), a duplicate index, an unknown kind or
 * one whose feature width does not match the model, a bank that lost its rings in a failed set_mc, a capturing stream. */
int ape_streams_reset_subset(ape_streams_t* bank, const int32_t* streams_host, int32_t K);
int ape_streams_frame_subset(ape_streams_t* bank, int32_t kind, const float* rows_dev, const int32_t* streams_host, int32_t K,
                             uint32_t flags, void* out_dev, int32_t out_dtype, void* stream);

/* per-stream body measurements (additive in ABI 7).  replaces: the bonemap every reference Estimator is built with
 * (estimator.py:57-68: lower-arm vector, upper-arm vector, shoulder origin), whose nine values enter every origin of its messages
 * (estimate_joints.py:48-92, compose_msg.py:54-61,92-94) -- S estimators with S bonemaps in one bank.
 * A bank that was never given bodies passes its uniform body (ape_model_set_body; body9 of ape_fk_bank_create; ape_kalman_bank_set_body)
 * to its kernels by value, as before.  The first ape_*_set_bodies call gives the bank a device table of S rows, initialised from that
 * uniform body, and overwrites the listed rows; from then on every frame of the bank (lockstep, subset, host frames, and the frames
 * ape_model_recover issues again) takes stream s's body from row s, and a later ape_model_set_body no longer reaches the bank.
 *   streams_host   K DISTINCT stream indices (host memory), or NULL: all S streams in order, K == S
 *   body9s_host    f64 [K,9] (host memory): row j = [larm_vec, uarm_vec, uarm_orig_rh] of stream streams_host[j]; not validated (the
 *                  reference does not either: NaN propagates as there); free for reuse on return
 * Ordered on `stream`: frames enqueued before the call see the old values, frames enqueued after it the new ones.  NO cold start:
 * windows, state histories and smoothing stacks hold features and NN targets, which do not depend on the body -- the stream's next
 * message is computed from its existing stack with the new body; a slot handed to a new wearer is set_bodies + a reset of that stream.
 * K = 0 changes no row (and still switches the bank to its table).  ape_kalman_bank_set_body on a bank in table mode overwrites every
 * row (ordered on the null stream).  ape_*_get_bodies: the host mirror [S,9]; S copies of the uniform body before the first set.
 * Refused (non-zero, ape_last_error): NULL bank or values, K < 0 or K > S, NULL list with K != S, an index outside [0, S), a duplicate
 * index, a capturing stream.  ape_infer, ape_fk and ape_msg_reduce keep the model's one body. */
int ape_streams_set_bodies(ape_streams_t* bank, const int32_t* streams_host, int32_t K, const double* body9s_host, void* stream);
int ape_streams_get_bodies(ape_streams_t* bank, double* out_host);
/* ape_replay with one body per recording: bodies_host f64 [R,9] (host memory), row r for the recording that starts at seg_starts_host[r];
 * row f of out_dev is what a fresh estimator BUILT WITH that recording's bonemap returns for its row f.  NULL: ape_replay (the model's
 * body for every recording, on the same kernels as before). */
int ape_replay_bodies(ape_model_t* model, int32_t kind, const float* rows_dev, int32_t F, const int32_t* seg_starts_host, int32_t R,
                      int32_t seq_len, int32_t smooth, int32_t n_mc, float dropout_p, uint64_t seed, uint32_t flags,
                      void* out_dev, int32_t out_dtype, float* y_dev, int32_t max_rows_per_launch, void* stream,
                      const double* bodies_host);

/* ---- DropoutFF and ImuPoseLSTM behind the frames, banks and replays (additive in ABI 7) -----------------------------
 * ape_streams_create accepts APE_MODEL_FF and APE_MODEL_IMUPOSE handles with a target layout, and every ape_streams_* entry above then
 * works on such a bank with the contracts stated there (a bank without ape_streams_set_mc is the eval bank, one row per stream).
 * What the reference does with these models inside Estimator.add_xx_to_row_hist_and_make_prediction (estimator.py:93-120,
 * watch_phone_pocket_nn.py:98-112) and what the banks reproduce:
 *   APE_MODEL_FF       nn_models.py:340-370: the MLP runs on every row of the repeated window and [:, -1, :] keeps the newest row, so
 *                      the window, seq_len and the cold-start padding have no influence: the bank keeps the newest feature row per
 *                      stream.  The n_mc samples of a stream differ only by an independent Bernoulli(1-p) mask, scaled 1/(1-p), over
 *                      the H outputs of the last hidden layer; dropout_p = 0 gives n_mc identical rows.  The trunk runs once per stream,
 *                      the n_mc masked heads behind it (ff_bank.hip).  Masks: in-kernel Philox keyed by (seed + the bank's frame
 *                      counter; row = stream * n_mc + sample; hidden unit) -- in a subset frame `stream` is the list position, like the
 *                      LSTM banks' samples.  Not DropoutFF.forward's own random stream.  No cooperative kernel: such frames need no
 *                      co-residency and ape_model_recover finds nothing to re-issue.
 *   APE_MODEL_IMUPOSE  monte_carlo_predictions(n_samples, x) is self(x, None) (nn_models.py:246-251): no repeat, no dropout, the sample
 *                      count is IGNORED.  ape_streams_set_mc(n_mc, ...) succeeds and leaves the bank at one row per stream and frame
 *                      (N = smooth stacked rows; packed rows are [25 + 6*smooth]); it is still a cold start.  The window matters: T rows,
 *                      padded with the newest on a cold start.  Lockstep and subset frames of one schedule give the same bits.  Frames
 *                      ride the cooperative LSTM kernels and are journaled and re-issued like the LSTM banks' (ape_model_recover).
 * ape_replay_regressor: ape_replay_bodies (same arguments, same semantics; bodies_host may be NULL) for every model kind.  APE_MODEL_LSTM
 * handles are forwarded to ape_replay_bodies.  APE_MODEL_FF: seq_len is accepted and has no influence; the masks are those of ONE pass
 * over all F * n_mc sample rows keyed by `seed`, independent of max_rows_per_launch.  APE_MODEL_IMUPOSE: the effective n_mc is 1 --
 * out_dev rows are [25] or, packed with smooth > 1, [25 + 6*smooth]; y_dev is [F, 1, O].  ape_replay / ape_replay_bodies keep refusing
 * non-LSTM handles.  Refusals otherwise as ape_replay (fp16 precision, no target layout, bad starts, a capturing stream). */
int ape_replay_regressor(ape_model_t* model, int32_t kind, const float* rows_dev, int32_t F, const int32_t* seg_starts_host, int32_t R,
                         int32_t seq_len, int32_t smooth, int32_t n_mc, float dropout_p, uint64_t seed, uint32_t flags,
                         void* out_dev, int32_t out_dtype, float* y_dev, int32_t max_rows_per_launch, void* stream,
                         const double* bodies_host);

/* ---- the estimator without a regressor: WatchPhoneUarm (additive in ABI 7) -------------------------------------
 * Replaces estimate/watch_phone_uarm.py:10-108 behind Estimator (estimator.py:93-137): per frame the 38 features of
 * APE_PARSE_WATCH_PHONE_UARM, the watch's and the phone's calibrated 6D columns (features 13:19 and 32:38) as the 12 targets of
 * APE_LAYOUT_ORI_CAL_LARM_UARM, float64 with no model and no de-normalisation, the smoothing stack (`smooth` rows, padded with the
 * newest on a cold start, estimator.py:112-118) and the 25-value message (compose_msg.py:82-108).  float64 throughout; an F32 output
 * is the float64 message rounded (the PoseEstPublisherUDP payload, pose_est_udp.py:47).
 * A bank holds S streams, each with its own stack and its own count of rows since its cold start: lockstep frames (all S in order)
 * and subset frames mix freely.  smooth is clamped to max(1, smooth) like the reference; smooth <= 64.  body9 = [larm_vec, uarm_vec,
 * uarm_orig_rh] (Estimator.body_measurements).
 * ape_fk_bank_frame: rows_dev f32 [K,55] on the device (kind APE_PARSE_WATCH_PHONE_UARM, may carry APE_PARSE_BIG_ENDIAN), row j for
 *   stream streams_host[j] (K distinct indices in host memory; NULL => K == S, all streams in order); out_dev [K,25] of out_dtype in
 *   list order.  Streams not listed stay untouched.  K = 0 is a no-op.  Asynchronous on `stream`; ONE bank serialises on ONE stream.
 * ape_fk_bank_frame_host: one lockstep frame from host rows [S,55] to host messages [S,25]; BLOCKING (what process_row calls).
 * ape_fk_bank_reset: cold-starts every stream; ape_fk_bank_reset_subset: the K listed streams only.
 * ape_fk_replay: every frame of R recordings back to back in rows_dev [F,55] (seg_starts_host: their first rows, [0] first,
 *   strictly rising, below F), each from a cold start -> out_dev [F,25]: what a fresh bank stream fed each recording returns.  BLOCKING.
 * Refused (non-zero, ape_last_error): NULL arguments, a kind other than APE_PARSE_WATCH_PHONE_UARM, K < 0 or K > S, an index outside
 * [0, S), a duplicate index, bad replay starts, F < 1, smooth > 64, a capturing stream (frames stage ring positions per call). */
typedef struct ape_fk_bank ape_fk_bank_t;
int ape_fk_bank_create(int32_t n_streams, int32_t smooth, const double body9[9], int32_t device, ape_fk_bank_t** out);
int ape_fk_bank_destroy(ape_fk_bank_t* bank);
int ape_fk_bank_reset(ape_fk_bank_t* bank);
int ape_fk_bank_reset_subset(ape_fk_bank_t* bank, const int32_t* streams_host, int32_t K);
int ape_fk_bank_frame(ape_fk_bank_t* bank, int32_t kind, const float* rows_dev, const int32_t* streams_host, int32_t K,
                      void* out_dev, int32_t out_dtype, void* stream);
int ape_fk_bank_frame_host(ape_fk_bank_t* bank, int32_t kind, const float* rows_host, void* out_host, int32_t out_dtype, void* stream);
int ape_fk_replay(int32_t kind, const float* rows_dev, int32_t F, const int32_t* seg_starts_host, int32_t R, int32_t smooth,
                  const double body9[9], int32_t device, void* out_dev, int32_t out_dtype, void* stream);
/* per-stream bodies of the bank and one body per recording of a replay (semantics above at ape_streams_set_bodies):
 * the FK-only estimator's bonemap (watch_phone_uarm.py behind estimator.py:57-68).  ape_fk_replay_bodies: bodies_host f64 [R,9] or
 * NULL = body9 for every recording (ape_fk_replay); with bodies_host given body9 may be NULL. */
int ape_fk_bank_set_bodies(ape_fk_bank_t* bank, const int32_t* streams_host, int32_t K, const double* body9s_host, void* stream);
int ape_fk_bank_get_bodies(ape_fk_bank_t* bank, double* out_host);
int ape_fk_replay_bodies(int32_t kind, const float* rows_dev, int32_t F, const int32_t* seg_starts_host, int32_t R, int32_t smooth,
                         const double body9[9], int32_t device, void* out_dev, int32_t out_dtype, void* stream,
                         const double* bodies_host);

/* ---- stream state hand-over: a stream's history leaves its bank (additive in ABI 7) -------------------------------
 * replaces: nothing in the reference, whose one Estimator keeps `_row_hist` / `_smooth_hist` (estimator.py:93-118) for its lifetime.
 * After a stream's first row its window always holds T rows and its stack `smooth` predictions (the cold-start padding is
 * materialised), so a stream's state is a time-ordered window, a time-ordered stack and two warm bits.  The canonical record of one
 * stream is `words_per_stream` 4-byte words on the device, independent of ring phase, slot and bank:
 *   window[T][I]            f32, the feature rows as copy 0 of the stream's window ring holds them, oldest first
 *   stack[smooth][n_mc][O]  f32, the model outputs (normalised NN targets) as the smoothing ring holds them, oldest frame first
 *   zero words up to the next multiple of 4 (records are 16-byte units; state_dev must be 16-byte aligned)
 * words_per_stream = (T*I + smooth*n_mc*O + 3) & ~3.  APE_MODEL_FF banks have T = 1, APE_MODEL_IMUPOSE banks n_mc = 1.
 * The FK-only bank's record is its stack alone: T = I = 0, n_mc = 1, O = 8, stack[smooth][8] of FLOAT64 quaternion pairs (lower arm,
 * upper arm: what its ring holds), words_per_stream = 16*smooth.
 * warm_host: one byte per stream in HOST memory, from the bank's host counters (nothing is read back from the device):
 *   APE_STATE_WINDOW_WARM  at least one row since the cold start; clear: the window words are zeros on export, ignored on import
 *   APE_STATE_STACK_WARM   at least one prediction since the cold start; clear: likewise for the stack words
 * NOT in the record: the per-stream bodies (ape_*_get_bodies / ape_*_set_bodies move them) and the Philox position (seed and call
 * counter stay properties of the bank: an imported stream draws the samples of its NEW bank and list position).
 * ape_*_state_desc: the bank's own descriptor.
 * ape_streams_export / ape_fk_bank_export: read-only, ONE launch on `stream`, no host synchronisation; the bank keeps its mode (a
 *   lockstep bank derives the slots from its global counters).  Record j belongs to stream streams_host[j].  Like a frame, an export
 *   behind a frame that ape_model_recover may still re-issue sees that frame's results only after the recover.
 * ape_streams_import / ape_fk_bank_import: puts the bank into per-stream mode as the first subset call does (the other streams'
 *   counters are seeded from the lockstep ones), writes copy 0 of the listed streams' window rings and their stack rings in ONE launch
 *   and sets their host counters: a warm window behaves as after >= T rows, a warm stack as after >= smooth predictions; a stream
 *   with APE_STATE_WINDOW_WARM clear is cold-started like ape_streams_reset_subset (its stack too); one with only
 *   APE_STATE_STACK_WARM clear keeps the window and gets a cold stack.  Streams not listed stay bit for bit untouched.  Journal: as a
 *   newer frame does, an import drops the bank's pending step / subset frame from the journal (recover BEFORE the import if that
 *   frame's outputs are still wanted).
 * K = 0 is a no-op.  Refused (non-zero, ape_last_error) before any launch: NULL arguments, a descriptor that differs from the bank's
 * own in any field, K < 0 or K > S, an index outside [0, S), a duplicate index, a bank that lost its rings, a capturing stream.
 * The Kalman bank's record is its own (ragged stack, state history: ape_kalman_bank_export below). */
#define APE_STATE_VERSION 1
#define APE_STATE_WINDOW_WARM 1
#define APE_STATE_STACK_WARM 2
typedef struct ape_stream_state_desc {
    int32_t version;              /* APE_STATE_VERSION */
    int32_t T, I, smooth, n_mc, O;
    int32_t words_per_stream;
} ape_stream_state_desc_t;
int ape_streams_state_desc(ape_streams_t* bank, ape_stream_state_desc_t* out);
int ape_streams_export(ape_streams_t* bank, const int32_t* streams_host, int32_t K, void* state_dev, uint8_t* warm_host, void* stream);
int ape_streams_import(ape_streams_t* bank, const ape_stream_state_desc_t* desc, const int32_t* streams_host, int32_t K,
                       const void* state_dev, const uint8_t* warm_host, void* stream);
int ape_fk_bank_state_desc(ape_fk_bank_t* bank, ape_stream_state_desc_t* out);
int ape_fk_bank_export(ape_fk_bank_t* bank, const int32_t* streams_host, int32_t K, void* state_dev, uint8_t* warm_host, void* stream);
int ape_fk_bank_import(ape_fk_bank_t* bank, const ape_stream_state_desc_t* desc, const int32_t* streams_host, int32_t K,
                       const void* state_dev, const uint8_t* warm_host, void* stream);
/* One bank's exports and imports share one device descriptor buffer (as its subset frames share theirs): issue a bank's calls on ONE
 * stream, or order the streams yourself.
 *
 * ape_replay_resume: ape_replay_regressor (every model kind; same arguments, same semantics, bodies_host may be NULL) that can start from
 * and end in the canonical records above, so that a recording replayed in pieces, or handed over between a replay and a bank, continues
 * without a cold start.  The records' shape is {T = seq_len (1 for APE_MODEL_FF), I, smooth, n_mc (1 for APE_MODEL_IMUPOSE), O} of the
 * call; 16-byte aligned device buffers of [R][words_per_stream] words, warm bytes [R] in host memory.
 *   state_in_dev / warm_in_host   NULL, or one record per LISTED recording: recording r does not start cold -- window row t of its frame
 *                  f is feature row f - T + 1 + t where that is at or after the recording's first row of this call, else the matching row
 *                  of the record's window counted back from its newest; its stack likewise (the carried model outputs go through the same
 *                  de-normalisation and FK as fresh ones, once per call, with the recording's body).  A clear warm bit: that part starts
 *                  cold exactly as in ape_replay.
 *   state_out_dev / warm_out_host NULL, or they receive each recording's final window and stack (warm = 3: every listed recording has a
 *                  row).  The call then keeps the targets of all F * n_mc rows on the device (O(F), like the features).
 *   sample_row_base  added to the Philox row counter of every launch; base + F*n_mc < 2^31, and a multiple of 4 where an LSTM
 *                  model runs with dropout (without dropout it is not read).
 * Chunk contract, ONE recording (R = 1): calls over rows [0, a), [a, b), ... that chain each state_out into the next state_in with
 * sample_row_base = a * n_mc, b * n_mc, ... return the rows of the single call over [0, F), Monte-Carlo samples included where the
 * regressor kernel's row granule divides every base: 4 rows on the batch-tile kernel (ape_model_set_kernel(APE_KERNEL_TILE16)), 16 on
 * the cluster kernels, 1 for APE_MODEL_FF.  For R > 1 the deterministic results are equal; the samples are valid draws but not those of
 * the one call, whose row index is global over the concatenation.  A recording that ended in an earlier call is simply not listed:
 * every listed recording has at least one row.  NULL states and base 0: ape_replay_regressor, on the instantiations it always ran.
 * BLOCKING.  Refused as ape_replay, and: state_in without warm_in, state_out without warm_out, a misaligned buffer, a bad base. */
int ape_replay_resume(ape_model_t* model, int32_t kind, const float* rows_dev, int32_t F, const int32_t* seg_starts_host, int32_t R,
                      int32_t seq_len, int32_t smooth, int32_t n_mc, float dropout_p, uint64_t seed, uint32_t flags,
                      void* out_dev, int32_t out_dtype, float* y_dev, int32_t max_rows_per_launch, void* stream,
                      const double* bodies_host, const void* state_in_dev, const uint8_t* warm_in_host, void* state_out_dev,
                      uint8_t* warm_out_host, uint64_t sample_row_base);

/* ---- per-stream smoothing lengths (additive in ABI 7) -----------------------------------------------------------------
 * replaces: the `smooth` every reference Estimator is built with (estimator.py:45, max(1, smooth)), the stack of that many predictions
 * (estimator.py:112-118) and the tail of est[i, :6] of every stacked row (estimator.py:131-137) -- S estimators built with S values of
 * `smooth` in one bank, on ONE regressor launch: stream s of the bank behaves like an estimator built with smooth = smooths[s].
 * CAPACITY: the smooth a bank was created with is its capacity `cap`.  Rings, tails and packed rows keep the sizes and strides they
 * have (yring [S,cap,n_mc,O], FK ring [S,cap,8]); every limit (cap <= 64, cap * n_mc <= 4096) is stated on cap.
 * A bank that was never given smooths runs exactly what it ran.  The first ape_*_set_smooths call gives the bank a device table of S
 * int32 values, initialised to cap, plus a host mirror, and overwrites the listed rows; the table survives ape_streams_reset and
 * ape_streams_set_mc.
 *   streams_host   K DISTINCT stream indices (host memory), or NULL: all S streams in order, K == S
 *   smooths_host   int32 [K] (host memory), each in [1, cap]; free for reuse on return
 * COLD START: the reference fixes smooth at construction, so a change has no defined transition -- the call cold-starts the listed
 * streams, window and stack: with a list what ape_streams_reset_subset / ape_fk_bank_reset_subset do for them (the NN bank's mode rules
 * apply), with NULL an ape_streams_reset / ape_fk_bank_reset (every stream cold, the NN bank in lockstep).  K = 0 changes no row and still
 * switches the bank to its table.  Ordered on `stream`: frames enqueued before the call see the old values, frames after it the new.
 * EVERY FRAME of a table bank (lockstep step, ape_streams_frame_host, subset frames on device and host, the FK bank's four frame
 * entries, and the frames ape_model_recover issues again -- a re-issued step goes through ape_streams_step, a re-issued subset frame
 * through its post-filter launch, and both read the bank's table), with k = smooths[s], M = n_mc, N_s = k * M:
 *   stream s uses ring slots 0 .. k-1 of its cap slots; its newest prediction goes to slot n_s mod k (n_s: predictions since its cold
 *   start), its first prediction after a cold start to all k slots; stack row i is sample i % M of the prediction k - 1 - i / M frames
 *   back, weight 1 / N_s, flip against row 0, the summation order of a uniform bank of k; N_s == 1 takes the single-row copy path.
 *   tail_dev and APE_FLAG_PACKED_MSG rows keep the stride of cap: row s holds 25 + 6 N_s live values (tail: N_s rows of 6), everything
 *   between them and the end of the row is written as exact zeros every frame; with APE_FLAG_SPREAD the record stays in the last
 *   APE_SPREAD_WIDTH columns of the fixed-stride row.  As APE_F32 the first 25 + 6 N_s floats of a packed row are byte for byte the
 *   payload the reference sends for an estimator built with smooth = k.
 * Post-filter form of a table bank (ape_streams_last_post_form): 1, or -- where the bank holds the split form's workspaces -- the chunk
 * count of cap * n_mc; chunks past a stream's rows arrive with zero partial sums.  A bank of cap == 1 accepts the call and keeps its forms.
 * STATE HAND-OVER: records keep words_per_stream of cap and ape_*_state_desc's smooth stays cap.  Export of stream s: the stack part holds
 * its k predictions oldest first, followed by zeros.  Import into stream t: the record is read with smooths[t] -- the records do not carry
 * k.  A caller who moves a stream FIRST gives the target slot the source's value (set_smooths cold-starts the slot) and THEN imports
 * (the import warms it).
 * ape_*_get_smooths: the host mirror [S]; S copies of cap before the first set.
 * Refused (non-zero, ape_last_error) before anything is written: NULL bank or values, K < 0 or K > S, a NULL list with K != S, an index
 * outside [0, S), a duplicate index, a value outside [1, cap], a capturing stream. */
int ape_streams_set_smooths(ape_streams_t* bank, const int32_t* streams_host, int32_t K, const int32_t* smooths_host, void* stream);
int ape_streams_get_smooths(ape_streams_t* bank, int32_t* out_host /* [S] */);
int ape_fk_bank_set_smooths(ape_fk_bank_t* bank, const int32_t* streams_host, int32_t K, const int32_t* smooths_host, void* stream);
int ape_fk_bank_get_smooths(ape_fk_bank_t* bank, int32_t* out_host);

/* ---- Monte-Carlo spread record (additive in ABI 7) --------------------------------------------------------------------
 * replaces: nothing.  The reference has NO counterpart of this record: the only form in which it lets the sample spread out is the raw
 * cloud, est[i, :6] of every stacked row appended to the message (estimator.py:131-137; APE_FLAG_PACKED_MSG / tail_dev here).  The
 * record is a fixed-width summary of the same N = smooth * n_mc stacked est rows the message averages -- the rows
 * arm_pose_from_nn_targets returns for the stack Estimator.add_xx_to_row_hist_and_make_prediction builds (estimator.py:112-118), reduced
 * by msg_from_pred (estimator.py:122-137) through compose_msg.msg_from_nn_targets_est (compose_msg.py:48-108) -- in the reference's stack
 * order.  APE_SPREAD_WIDTH values per stream and frame:
 *   [0:3]    plain mean of est[:, 0:3], the hand origin.  Deliberately NOT msg[4:7]: for the two orientation layouts the message
 *            recomputes its origins from the MEAN QUATERNIONS (compose_msg.py:54-61), which is not the mean of the rows' origins
 *   [3:9]    population covariance (divisor 1/N) of the hand origin, upper triangle xx, xy, xz, yy, yz, zz
 *   [9:12]   plain mean of est[:, 3:6], the elbow (lower-arm origin)
 *   [12:18]  its covariance, same order
 *   [18:21]  angular spread in radians of the lower-arm, upper-arm and hips quaternions about the message's quaternion qm of that joint
 *            (msg[7:11], msg[14:18], msg[21:25]): 2 asin(sqrt(1 - (1/N) sum_i (q_i . qm)^2)), the angle whose sin^2(t/2) is the mean
 *            sin^2(t_i/2) of the rows; independent of the sign of q_i.  The sqrt argument is clamped to [0, 1] letting NaN through
 * N == 1: means are the row, covariances and angles exactly 0 by rule.  APE_LAYOUT_ORI_CAL_LARM_UARM (no hips): [20] is exactly 0.
 * One pass in float64: covariance = mean of products - product of means, so its absolute error is ~N 2^-53 max(1, |x|^2); a NaN est
 * row makes the entries it touches NaN.  An APE_F32 output is the float64 record rounded once.
 * APE_FLAG_SPREAD is accepted by ape_streams_step, ape_streams_frame_subset, ape_streams_frame_host, ape_replay, ape_replay_bodies,
 * ape_replay_regressor and ape_replay_resume (and by the Kalman bank's frames and replays, see there): every output row grows by APE_SPREAD_WIDTH columns at its END -- plain rows become
 * [., 25 + 21], PACKED_MSG rows [., 25 + 6N + 21]; where an entry writes 25-column rows for PACKED_MSG at N == 1 (subset frames, replays)
 * the flagged row is [., 25 + 21].  A separate tail_dev stays separate.  The record is written for every N.  Without the flag nothing
 * changes, and the unflagged calls run the kernels they always ran.
 * ape_spread_reduce: the stand-alone reduction beside ape_msg_reduce.  est_dev f64 [N,W] rows of the model's layout, msg_dev f64 [25]
 * the message of the same rows (ape_msg_reduce; only its three quaternions are read), spread_dev f64 [APE_SPREAD_WIDTH]. */
#define APE_SPREAD_WIDTH 21
/* which form of the post-filter the bank's newest lockstep or subset frame ran (tests, profiles): *form = -1 no frame yet, 0 the wide form
 * (lanes = streams, banks without stacking), 1 one workgroup per stream, c > 1 a stream's stack split over c workgroups.  For a flagged
 * frame it is the value the launch was made with; for an unflagged one, the same rule's answer. */
int ape_streams_last_post_form(ape_streams_t* bank, int32_t* form);
int ape_spread_reduce(ape_model_t* model, const double* est_dev, int32_t N, const double* msg_dev, double* spread_dev, void* stream);

/* kernel selection for A/B runs and tests; no effect on results beyond float32 summation order */
int ape_model_set_kernel(ape_model_t* model, int32_t choice);
int ape_model_set_precision(ape_model_t* model, int32_t precision);
/* BLOCKING health check (hipDeviceSynchronize, i.e. every stream of the device): non-zero if a cluster-kernel launch
 * since the last check gave up waiting for a peer workgroup (its bounded spins expired) -- the outputs of that launch
 * and of every later one on this handle are invalid.  A failing check also resets the handle: the next launch works. */
int ape_model_check(ape_model_t* model);
/* ape_model_check that survives an abort.  The handle keeps a journal of the compute calls made on it since the last
 * successful check / recover (ape_lstm_forward[_hs], ape_fk, ape_msg_reduce, ape_infer, ape_streams_step; up to 64).  When
 * the blocking check finds an aborted weight-stationary launch, the handle is reset as by ape_model_check and every
 * journaled call is issued again, in order, on its own stream, with the cooperative kernels switched off (batch-tile LSTM
 * kernel, tile MLP kernel: no workgroup waits for another; same arithmetic up to float32 summation order, so results
 * agree with the aborted kernels' to ~1e-6 -- an fp16-precision model is re-run in exact float32), then the device is
 * synchronised: 0 = nothing was aborted, or everything was re-issued and the outputs are valid now.  The CALLER'S PART:
 * the device buffers those calls read must still hold the same data (recover before re-using them; a Python mirror that
 * copies outputs to the host right behind a call satisfies this by construction).  A stream-bank step can be re-issued
 * only while it is the bank's newest step and no row was pushed behind it; otherwise, or when more than 64 calls are
 * pending, the function returns APE_ERR_HIP like ape_model_check and counts the calls as lost.  Never a CPU path: the
 * re-issue is a fresh launch of HIP kernels in this process. */
int ape_model_recover(ape_model_t* model);
typedef struct ape_model_stats {
    uint64_t aborted_checks;      /* checks / recovers that found an aborted launch                       */
    uint64_t reissued_calls;      /* calls ape_model_recover issued again on the non-cooperative kernels  */
    uint64_t lost_calls;          /* calls pending at an abort that could not be re-issued                */
} ape_model_stats_t;
int ape_model_stats(const ape_model_t* model, ape_model_stats_t* out);

/* introspection for benchmarks: name of the dominant kernel for (B,T) and its algorithmic
 * FLOP per window (sum_layers 2*4H*(in_l+H) per step, + 2*O*H head once). */
const char* ape_lstm_kernel_name(const ape_model_t* model, int32_t B, int32_t T);
/* the regressor kernel the newest call on this handle launched last ("ape_lstm_mc_small", "ape_lstm_cluster32", "ape_lstm_tile16", ...;
 * the MLP regressor: "ape_mlp_pipe" or "ape_mlp_tile16" for a forward call, "ape_ff_bank_head" for a bank frame or replay chunk;
 * "" before the first call): tests and benchmarks assert the route they mean to measure */
const char* ape_model_last_kernel(const ape_model_t* model);
double ape_flops_per_window(const ape_dims_t* dims, int32_t T);

/* ---- ensemble Kalman estimator (tail; ABI 4) ----------------------------------------
 * Replaces KalmanSmartwatchModel (reference estimate/kalman_models.py:139-220: ProcessModelWindow :8-50,
 * ObservationNoise :53-80, SensorModelWindow :83-136) behind WatchPhonePocketKalman (watch_phone_pocket_kalman.py:12-169).
 * PARITY UNPINNED: the reference module imports bayesian_torch (absent) and its checkpoint is absent; the checker is
 * oracle/kalman_oracle.py, a restatement of the cited lines and of the published LinearFlipout algorithm.
 *
 * Rows are (stream s, ensemble member e), batch-major.  One forward = one draw of the flipout weight perturbations,
 * shared by all rows of the call (LinearFlipout draws eps once per call), and per-element +-1 signs; the Kalman update
 * (means, observation noise, 14 x 14 innovation, inverse, gain: kalman_models.py:181-208) is per stream, i.e. the
 * reference's batch size 1 (watch_phone_pocket_kalman.py:135) for every stream.
 *
 * Weight blob (float32, ape_kalman_weight_floats values), layers in this order with the reference's names:
 *   process_model.bayes1, process_model.bayes3 (flipout), process_model.bayes_m2 (linear),
 *   sensor_model.fc2 (linear), sensor_model.fc3, .fc5, .fc6 (flipout), observation_noise.fc1, .fc2 (linear);
 *   a flipout layer contributes mu_weight [N,K], rho_weight [N,K], mu_bias [N], rho_bias [N]; a linear one weight [N,K], bias [N].
 * noise_dev: NULL (device-side Philox draws from `seed`) or ape_kalman_noise_floats(S) floats of injected draws, per flipout
 *   layer in blob order: eps_weight [N,K], eps_bias [N] (standard normal), sign_in [S*E,K], sign_out [S*E,N] (+-1).
 * win_size must be even (rows are read 16 bytes at a time). */
typedef struct ape_kalman ape_kalman_t;
typedef struct {
    int32_t num_ensemble;   /* E: ensemble members (watch_phone_pocket_kalman.py:16; 2..128) */
    int32_t win_size;       /* W: window of previous states / raw observations (:17) */
    int32_t device;
} ape_kalman_dims_t;
int ape_kalman_create(const ape_kalman_dims_t* dims, ape_kalman_t** out_model);
int ape_kalman_destroy(ape_kalman_t* model);
size_t ape_kalman_weight_floats(const ape_kalman_t* model);
size_t ape_kalman_noise_floats(const ape_kalman_t* model, int32_t S);
int ape_kalman_load_weights(ape_kalman_t* model, const float* blob_host, size_t n_floats);
/* KalmanSmartwatchModel.forward (kalman_models.py:175-220): raw_obs [S,W,22], state_prev [S,E,W,14] ->
 * state_corrected [S,E,14], m_state_corrected [S,14], m_state_pred [S,14], z [S,14], ensemble_z [S,E,14] (all device, f32) */
int ape_kalman_forward(ape_kalman_t* model, const float* raw_obs_dev, const float* state_prev_dev, int32_t S, uint64_t seed,
                       const float* noise_dev, float* state_corrected_dev, float* m_state_corrected_dev,
                       float* m_state_pred_dev, float* z_dev, float* ensemble_z_dev, void* stream);
/* KalmanSmartwatchModel.format_state (kalman_models.py:164-173): state [S,14] -> [S,E,14] = state + N(0, 0.1 I);
 * noise_dev NULL or [S,E,14] standard-normal draws */
int ape_kalman_format_state(ape_kalman_t* model, const float* state_dev, int32_t S, uint64_t seed, const float* noise_dev,
                            float* out_dev, void* stream);
/* BLOCKING: non-zero if a forward since the last check met an exactly singular innovation matrix (torch.linalg.inv raises) */
int ape_kalman_check(ape_kalman_t* model);

/* ---- the Kalman estimator's frame: device stream bank, one-call frames, offline replay (additive in ABI 7) --------
 * PARITY UNPINNED like the entries above: what is added is the bookkeeping around ape_kalman_forward -- the frame of
 * WatchPhonePocketKalman (watch_phone_pocket_kalman.py:57-63, 133-169) inside Estimator (estimator.py:93-137) -- and its checker is
 * oracle/kalman_oracle.py's KalmanFrameLogic chained with oracle/ape_oracle.py's WindowOracle and post-filter.
 * A bank is bound to a loaded ape_kalman_t (which must outlive it) and holds S streams, each with its own window of W feature rows,
 * state history [E,W,14], smoothing stack and count of frames since its cold start, all on the device.  For every listed stream a
 * frame parses the row (APE_PARSE_WATCH_PHONE_POCKET, may carry APE_PARSE_BIG_ENDIAN), pushes the features (the first row after a
 * cold start fills the window), z-scores in float64, runs the model on the window and the stream's state history (zeros after a
 * cold start), takes the sensor model's mean z [1,14] on the stream's first W + 1 frames (format_state(z) joins the history) and
 * the corrected ensemble [E,14] afterwards (it joins the history), de-normalises in float64, pushes onto the stack of `smooth`
 * entries (padded with the newest on a cold start; entries have 1 or E rows) and runs FK (APE_LAYOUT_ORI_CAL_LARM_UARM_HIPS) and
 * the 25-value message over all stacked rows.
 *   rows_dev     f32 [K,55], row j for stream streams_host[j] (K distinct indices in host memory; NULL => K == S, all in order).
 *                Lockstep and subset frames mix freely; streams not listed stay bit for bit untouched.  K = 0 is a no-op.
 *   noise_dev    NULL (Philox) or ape_kalman_noise_floats(K) injected draws of this call, rows = (list position j, member e)
 *   init_noise_dev  NULL (Philox) or f32 [K,E,14] standard-normal draws for format_state
 *   flags        0, APE_FLAG_PACKED_MSG and / or APE_FLAG_SPREAD (every other flag is refused)
 *   out_dev      [K,25] of out_dtype; APE_FLAG_PACKED_MSG: [K, 25 + 6*smooth*E], the message, then hand and elbow xyz of the
 *                n_rows[j] stacked rows, oldest entry first (estimator.py:131-137), then zeros.  F32 is the float64 message rounded.
 *                APE_FLAG_SPREAD: every row is APE_SPREAD_WIDTH columns longer and ENDS in the spread record of its n_rows[j] stacked
 *                rows (below, "the Kalman bank's spread record"): [K, 25 + 21], with APE_FLAG_PACKED_MSG [K, 25 + 6*smooth*E + 21]
 *                (the zeros stop in front of the record).
 *   n_rows_dev   int32 [K]: stacked rows of entry j, between smooth and smooth*E
 *   y_dev        NULL or f32 [K,E,14]: the frame's normalised prediction (row 0 alone on the first W + 1 frames, the rest unspecified)
 * One flipout perturbation draw per call, shared by all its rows (as ape_kalman_forward for S > 1).  Device draws are keyed by the
 * bank's seed (ape_kalman_bank_set_seed, which also restarts the call counter) and the number of the call: no two frames of a bank
 * share a key, two banks with one seed fed the same calls give the same bits.  ape_kalman_bank_set_norm_stats: xx [22], yy [14];
 * never called = no normalisation.  ape_kalman_bank_set_body: [larm_vec, uarm_vec, uarm_orig_rh]; zeros until set.
 * ape_kalman_bank_frame is asynchronous on `stream` (ONE bank serialises on ONE stream); ape_kalman_bank_frame_host is one lockstep
 * frame from host rows [S,55] to host messages and row counts, BLOCKING (what process_row calls).
 * ape_kalman_replay: every frame of R recordings back to back in rows_dev [F,55] (seg_starts_host: their first rows, [0] first,
 *   strictly rising, below F): a fresh bank of R streams with seed `seed`, frame t lists in ascending order the recordings that have
 *   a row t; outputs in recording order (row seg_starts[r] + t of out_dev [F, 25 | 25 + 6*smooth*E], n_rows_dev [F], y_dev
 *   [F,E,14]).  xx_m .. yy_s all NULL: no normalisation.  BLOCKING.  Flags and row widths as ape_kalman_bank_frame.
 * Refused (non-zero, ape_last_error): NULL arguments, weights not loaded, a kind other than APE_PARSE_WATCH_PHONE_POCKET, K < 0 or
 * K > S, an index outside [0, S) or listed twice, smooth > 64 or smooth*E > 4096, bad replay starts, F < 1, a capturing stream.
 * ape_kalman_check reports a singular innovation of any bank frame. */
typedef struct ape_kalman_bank ape_kalman_bank_t;
int ape_kalman_bank_create(ape_kalman_t* model, int32_t n_streams, int32_t smooth, ape_kalman_bank_t** out);
int ape_kalman_bank_destroy(ape_kalman_bank_t* bank);
int ape_kalman_bank_reset(ape_kalman_bank_t* bank);
int ape_kalman_bank_reset_subset(ape_kalman_bank_t* bank, const int32_t* streams_host, int32_t K);
int ape_kalman_bank_set_norm_stats(ape_kalman_bank_t* bank, const double* xx_m, const double* xx_s, const double* yy_m, const double* yy_s);
int ape_kalman_bank_set_body(ape_kalman_bank_t* bank, const double body9[9]);
int ape_kalman_bank_set_seed(ape_kalman_bank_t* bank, uint64_t seed);
/* ---- the Kalman bank's spread record (additive in ABI 7) ----
 * replaces: nothing (the record of DESIGN.md 4.28 above -- layout, rules and arithmetic unchanged, layout ORI_CAL_LARM_UARM_HIPS -- taken
 * over the N = n_rows stacked rows the Kalman tail walks: 1 row per stack entry during a stream's first W + 1 frames, E rows per entry
 * afterwards, entries oldest first, padded with the newest on a cold start).  Once the filter is initialised the rows are its corrected
 * ensemble and the record is the filter's own spread; during the init frames with smooth > 1 they are the last `smooth` sensor means
 * and the record is their smoothing lag; n_rows tells the phases apart.  N == 1: the row's two origins and exact zeros.
 * APE_FLAG_SPREAD, alone or with APE_FLAG_PACKED_MSG, is accepted by the five entries below; every other flag stays refused.  The 21
 * values are the LAST columns of each output row.  A flagged and an unflagged frame of the same bank state write the same message,
 * tail, n_rows, y_dev and rings; draws, counters and the state hand-over do not know the flag.
 * ape_kalman_bank_frame: flags 0, APE_FLAG_PACKED_MSG, APE_FLAG_SPREAD or both; rows [K, 25 (+ 6*smooth*E) (+ 21)]. */
int ape_kalman_bank_frame(ape_kalman_bank_t* bank, int32_t kind, const float* rows_dev, const int32_t* streams_host, int32_t K,
                          const float* noise_dev, const float* init_noise_dev, uint32_t flags, void* out_dev, int32_t out_dtype,
                          int32_t* n_rows_dev, float* y_dev, void* stream);
/* ape_kalman_bank_frame_host: the same flags; out_host is [S, 25 (+ 6*smooth*E with APE_FLAG_PACKED_MSG) (+ 21 with APE_FLAG_SPREAD)]
 * of out_dtype, the width the flags of THIS call give (the bank's pinned row buffer has room for the widest). */
int ape_kalman_bank_frame_host(ape_kalman_bank_t* bank, int32_t kind, const float* rows_host, uint32_t flags, void* out_host,
                               int32_t out_dtype, int32_t* n_rows_host, void* stream);
/* ape_kalman_replay: flags 0, APE_FLAG_PACKED_MSG and / or APE_FLAG_SPREAD; out_dev [F, 25 (+ 6*smooth*E) (+ 21)], the record of frame
 * f in the last APE_SPREAD_WIDTH columns of row f. */
int ape_kalman_replay(ape_kalman_t* model, int32_t kind, const float* rows_dev, int32_t F, const int32_t* seg_starts_host, int32_t R,
                      int32_t smooth, const double* xx_m, const double* xx_s, const double* yy_m, const double* yy_s,
                      const double body9[9], uint64_t seed, uint32_t flags, void* out_dev, int32_t out_dtype, int32_t* n_rows_dev,
                      float* y_dev, void* stream);
/* per-stream bodies of the Kalman bank and one body per recording of its replay (semantics above at
 * ape_streams_set_bodies): the bonemap of WatchPhonePocketKalman's Estimator (estimator.py:57-68).  ape_kalman_replay_bodies:
 * bodies_host f64 [R,9] or NULL = body9 for every recording (ape_kalman_replay); with bodies_host given body9 may be NULL. */
int ape_kalman_bank_set_bodies(ape_kalman_bank_t* bank, const int32_t* streams_host, int32_t K, const double* body9s_host, void* stream);
int ape_kalman_bank_get_bodies(ape_kalman_bank_t* bank, double* out_host);
/* ape_kalman_replay_bodies: flags and row widths as ape_kalman_replay (APE_FLAG_PACKED_MSG and / or APE_FLAG_SPREAD: +21 columns) */
int ape_kalman_replay_bodies(ape_kalman_t* model, int32_t kind, const float* rows_dev, int32_t F, const int32_t* seg_starts_host, int32_t R,
                             int32_t smooth, const double* xx_m, const double* xx_s, const double* yy_m, const double* yy_s,
                             const double body9[9], uint64_t seed, uint32_t flags, void* out_dev, int32_t out_dtype, int32_t* n_rows_dev,
                             float* y_dev, void* stream, const double* bodies_host);

/* ---- the Kalman bank's state hand-over: a stream's history leaves its bank (additive in ABI 7) ----------------------
 * replaces: nothing in the reference, whose one estimator keeps its window, `__input_state` and `__init_step`
 * (watch_phone_pocket_kalman.py:57-63, 133-169) for its lifetime.  PARITY UNPINNED like the bank.
 * The canonical record of one stream is `words_per_stream` 4-byte words on the device, independent of ring phase, slot and bank, every
 * part oldest first:
 *   window         f64 [W][22]          the W feature rows the stream's latest frame saw (the cold-start padding is materialised)
 *   state history  f32 [E][W][14]       the last W entries, time step minor; entries that do not exist yet (age < W) are zeros
 *   stack          f32 [smooth][E][14]  the last `smooth` predictions, normalised; rows at or beyond an entry's count are zeros
 *   counts         i32 [smooth]         1 (a sensor-mean frame) or E (an ensemble frame) per stack entry
 *   zero words up to the next multiple of 4 (records are 16-byte units; state_dev must be 16-byte aligned)
 * words_per_stream = (2*W*22 + E*W*14 + smooth*E*14 + smooth + 3) & ~3  (E = 48, W = 10, smooth = 1: 7836 words).
 * age_host: int32 per stream in HOST memory, min(frames since the stream's cold start, W + 1): 0 cold, 1..W the init phase (the
 *   frame returns the sensor mean), W + 1 mature.  The bank keeps it on the host (advanced by every frame, zeroed by the resets), so
 *   neither call reads anything back from the device.
 * NOT in the record: the per-stream bodies (ape_kalman_bank_get_bodies / _set_bodies move them) and the draw position, which belongs to
 *   the bank: the key of a bank's call n is seed + 0xD1342543DE82EF95 * n, draws are indexed by list position and member.
 *   ape_kalman_bank_get_draw_position / _set_draw_position read and write (seed, number of calls so far).  A bank with the same seed
 *   and call count that steps an imported stream at the same list position draws what the source bank would have drawn; anywhere else
 *   the stream draws valid samples of its new bank.
 * ape_kalman_bank_export: read-only, ONE launch on `stream`, no host synchronisation.  Record j and age_host[j] belong to stream
 *   streams_host[j]; a cold stream gives a zero record and age 0.
 * ape_kalman_bank_import: ONE launch that writes the listed streams' rings, row counts and frame counters (an imported mature stream
 *   continues at the smallest multiple of W * smooth above W: slot order = time order); a count word that is not E is stored as 1.
 *   Clears the pending cold start of streams with age > 0; age 0 is ape_kalman_bank_reset_subset for that stream and writes nothing.
 *   Streams not listed stay bit for bit untouched.
 * K = 0 is a no-op.  Refused (non-zero, ape_last_error) before any launch: NULL arguments, a descriptor that differs from the bank's
 * own in any field, an age outside [0, W + 1], K < 0 or K > S, an index outside [0, S) or listed twice, a record buffer that is not
 * 16-byte aligned, a capturing stream.  One bank's exports and imports share one device descriptor buffer: issue them on ONE stream.
 *
 * ape_kalman_replay_resume: ape_kalman_replay_bodies (same arguments, same semantics) that can start from and end in such records;
 * [R][words_per_stream] words in 16-byte aligned device buffers, ages [R] in host memory, each pair NULL or given together.
 *   state_in_dev / age_in_host    recording r with age > 0 does not start cold: the replay's fresh bank imports its record.  Age 0, or
 *                  no state: a cold start as in ape_kalman_replay.
 *   state_out_dev / age_out_host  receive every recording's record after its last frame, age_out = min(age_in + length, W + 1)
 *   call_base      the bank's call count starts here (ape_kalman_replay: 0), so frame t of the call draws with key number
 *                  call_base + t + 1
 * Chunk contract, ONE recording: calls over rows [0, a), [a, b), ... that chain state and age with call_base = a, b, ... return the
 * rows of the one call over [0, F), device draws included.  The same holds for R > 1 when every piece lists the same recordings cut at
 * the same offsets (list positions and call numbers then agree); otherwise the results are valid draws but not the one call's. */
#define APE_KALMAN_STATE_VERSION 1
typedef struct ape_kalman_state_desc {
    int32_t version;              /* APE_KALMAN_STATE_VERSION */
    int32_t E, W, smooth;
    int32_t words_per_stream;
} ape_kalman_state_desc_t;
int ape_kalman_bank_state_desc(ape_kalman_bank_t* bank, ape_kalman_state_desc_t* out);
int ape_kalman_bank_export(ape_kalman_bank_t* bank, const int32_t* streams_host, int32_t K, void* state_dev, int32_t* age_host, void* stream);
int ape_kalman_bank_import(ape_kalman_bank_t* bank, const ape_kalman_state_desc_t* desc, const int32_t* streams_host, int32_t K,
                           const void* state_dev, const int32_t* age_host, void* stream);
int ape_kalman_bank_get_draw_position(ape_kalman_bank_t* bank, uint64_t* seed, uint64_t* calls);
int ape_kalman_bank_set_draw_position(ape_kalman_bank_t* bank, uint64_t seed, uint64_t calls);
/* ape_kalman_replay_resume: flags and row widths as ape_kalman_replay (APE_FLAG_PACKED_MSG and / or APE_FLAG_SPREAD: +21 columns); the
 * order of every sum of the record depends on (N, thread, wave) alone, so chained pieces give the records of the one call bit for bit */
int ape_kalman_replay_resume(ape_kalman_t* model, int32_t kind, const float* rows_dev, int32_t F, const int32_t* seg_starts_host, int32_t R,
                             int32_t smooth, const double* xx_m, const double* xx_s, const double* yy_m, const double* yy_s,
                             const double body9[9], uint64_t seed, uint32_t flags, void* out_dev, int32_t out_dtype, int32_t* n_rows_dev,
                             float* y_dev, void* stream, const double* bodies_host, const void* state_in_dev, const int32_t* age_in_host,
                             void* state_out_dev, int32_t* age_out_host, uint64_t call_base);

/* host subset frames (additive in ABI 7): any K of a bank's S streams, host rows in, host datagrams out.
 * replaces: one iteration of the receive loop of a server that holds S reference Estimators -- for every datagram that arrived since
 * the last tick one Estimator.process_row (estimator.py:93-137; WatchPhoneUarm.process_row, watch_phone_uarm.py:64-108;
 * WatchPhonePocketKalman.process_row, watch_phone_pocket_kalman.py:141-156) and the message PoseEstPublisherUDP sends for it.
 * Semantics: EXACTLY those of the matching device subset frame (ape_streams_frame_subset, ape_fk_bank_frame with a list,
 * ape_kalman_bank_frame with a list and no injected draws) -- flags, row widths (25 columns at N == 1 whatever APE_FLAG_PACKED_MSG
 * says on the NN bank), mode rules (the NN bank enters per-stream mode; the FK and Kalman banks mix lockstep and subset frames), the
 * call counter behind the Monte-Carlo / Kalman draw keys, the refusals, K = 0 a no-op, unlisted streams bit for bit untouched: a bank
 * fed by either entry returns the same bits.
 *   rows_host      f32 [K, width] ordinary host memory: row j belongs to stream streams_host[j]
 *   streams_host   K DISTINCT stream indices (NULL is refused on the NN bank; on the FK / Kalman banks NULL means all S in order)
 *   out_host       [K, row width of the device entry] of out_dtype, ordinary host memory, list order
 *   n_rows_host    i32 [K] (Kalman bank): the stacked rows behind each message
 * BLOCKING, like the lockstep host frames: the call returns with out_host (and n_rows_host) filled.  On the NN bank an aborted
 * cooperative launch has been re-issued first (as by ape_model_recover) and a clean frame clears the journal; the frame is counted and
 * traced by ape_streams_frame_stats ({launch, wait, copy} microseconds).  On the Kalman bank a singular innovation is still reported
 * by ape_kalman_check.  The frame puts NO copy command and NO event on the stream: rows and descriptors are read by the frame's
 * first kernel from a pinned block, outputs are written by its last kernel into pinned memory followed -- for K <= 64 -- by one
 * completion word per entry, which the host polls; a larger K waits for the stream.
 * Refused (non-zero, ape_last_error) before any launch: what the device entry refuses. */
int ape_streams_frame_subset_host(ape_streams_t* bank, int32_t kind, const float* rows_host, const int32_t* streams_host, int32_t K,
                                  uint32_t flags, void* out_host, int32_t out_dtype, void* stream);
int ape_fk_bank_frame_subset_host(ape_fk_bank_t* bank, int32_t kind, const float* rows_host, const int32_t* streams_host, int32_t K,
                                  void* out_host, int32_t out_dtype, void* stream);
int ape_kalman_bank_frame_subset_host(ape_kalman_bank_t* bank, int32_t kind, const float* rows_host, const int32_t* streams_host,
                                      int32_t K, uint32_t flags, void* out_host, int32_t out_dtype, int32_t* n_rows_host, void* stream);

/* ---- scoring replayed poses against ground truth (additive in ABI 7) ---------------------------------------------------
 * replaces: nothing.  The reference has NO counterpart: it never compares a message with the mocap truth its recordings carry (the gt_*
 * columns NNS_TARGETS names).  ape_score_rows compares the message msg[25] (compose_msg.py:72-78) of every frame with the truth pose of
 * that frame and, optionally, accumulates per recording.  float64 arithmetic with separate roundings for a * b + c.
 * Per frame, APE_SCORE_WIDTH values:
 *   [0]      |msg[4:7] - t_hand| (metres)              [1]  |msg[11:14] - t_larm_orig|
 *   [2:5]    angular error in [0, pi] of the lower-arm, upper-arm and hips quaternions msg[7:11], msg[14:18], msg[21:25] against the
 *            truth's: with s = -1 where q . q_t < 0.0, else +1 (the flip rule of average_quaternions), 4 asin(min(1, |q - s q_t| / 2)).
 *            APE_LAYOUT_ORI_CAL_LARM_UARM (no hips): [4] is exactly 0
 *   [5], [6] squared Mahalanobis distance (t - m)' S^-1 (t - m) of the true hand / elbow under the frame's spread record: m = record
 *            [0:3] and S from [3:9] for the hand, [9:12] and [12:18] for the elbow; S^-1 by the adjugate of the symmetric 3x3.  A
 *            covariance is usable iff its six entries are finite, its trace is > 0 and det > 1e-12 (trace / 3)^3 (so N = 1 records and
 *            rank-deficient stacks are not); with spread_dev NULL or an unusable covariance the value is NaN
 * A frame is scored iff every truth value it uses and all 25 message values are finite; otherwise its seven values are NaN.
 * Truth, truth_dev of truth_dtype, one row per frame:
 *   APE_TRUTH_TARGETS  [F, O] de-normalised NN targets in the layout's column order (O = 14 / 12 / 20), taken through the float64
 *                      forward kinematics of ape_fk with the recording's body (arm_pose_from_nn_targets, estimate_joints.py:16-92);
 *                      the closed-form quaternions are refined to the eigenvector rot_mat_to_quat takes (transformations.py:521-545),
 *                      so ill-conditioned 6D columns give the reference's est rows to 1e-15, not to 4e-12
 *   APE_TRUTH_EST      [F, 21 | 14] est rows in the layout's est columns, quaternions as given (the shoulder origin [6:9] is not read)
 * Per recording, APE_SCORE_ACC_WIDTH raw accumulators (float64, so pieces of a recording merge on the host by adding sums and counts
 * and taking the larger maximum): [3c], [3c+1], [3c+2] for c = 0..4 the sum, sum of squares and maximum of value c over the
 * recording's scored frames; [15] scored frames; [16] frames that could not be scored; [17:21] hand: frames with a usable d^2, the
 * sum of d^2, frames with d^2 <= 2.3659738843753377 and with d^2 <= 6.251388631170325 (the 50 % and 90 % quantiles of chi^2 with
 * 3 degrees of freedom); [21:25] the same for the elbow.  The first `skip` frames of every recording (cold-start frames) are left out
 * of all 25; they still get their per-frame values.  A recording with nothing scored gives zeros.  No floating-point atomics and a
 * fixed order of summation: the same inputs give the same bits.
 *   msg_dev / msg_stride        the message at the front of rows msg_stride (>= 25) elements apart, of msg_dtype: plain, packed or
 *                               spread-flagged rows of any replay or bank go in as they are; nothing past column 24 is read
 *   spread_dev / spread_stride  the frames' spread records (APE_SPREAD_WIDTH), spread_stride (>= 21) elements apart, of msg_dtype; or NULL
 *   seg_starts_host             the R recordings' first frames: [0] == 0, strictly rising, below F
 *   bodies_host                 f64 [n_bodies, 9], n_bodies 1 (one body for all) or R; read for APE_TRUTH_TARGETS only
 *   score_dev                   [F, APE_SCORE_WIDTH] of score_dtype, or NULL;  acc_dev f64 [R, APE_SCORE_ACC_WIDTH], or NULL (not both)
 * Needs no model handle and runs on the current HIP device.  The launches go on `stream` and the call does not wait for them; the host
 * arrays have been consumed when it returns.  (The first call on a device, and a call with more recordings or frames than any before,
 * allocates its staging block and workspace first, which may wait for the device; up to 8 calls may be in flight per device.)  Refused with APE_ERR_INVALID_ARG before anything is written: NULL msg_dev / truth_dev /
 * seg_starts_host / bodies_host, F < 1, R < 1, bad starts, strides too small, skip < 0, n_bodies not 1 or R, APE_LAYOUT_NONE or an
 * unknown layout / kind / dtype, a capturing stream. */
#define APE_SCORE_WIDTH 7
#define APE_SCORE_ACC_WIDTH 25
enum { APE_TRUTH_TARGETS = 0, APE_TRUTH_EST = 1 };
int ape_score_rows(int32_t layout, const void* msg_dev, int32_t msg_stride, const void* spread_dev, int32_t spread_stride,
                   int32_t msg_dtype, const void* truth_dev, int32_t truth_kind, int32_t truth_dtype, int32_t F,
                   const int32_t* seg_starts_host, int32_t R, int32_t skip, const double* bodies_host, int32_t n_bodies,
                   void* score_dev, int32_t score_dtype, double* acc_dev, void* stream);

/* ---- scoring over a sweep of time lags (additive in ABI 7) ---------------------------------------------------------------
 * replaces: nothing; the reference has no counterpart.  ape_score_rows pairs message f with truth f.  A smoothed estimate trails the
 * motion (the mean of the last `smooth` frames by (smooth - 1) / 2 frames) and the mocap and IMU clocks are not aligned to the frame;
 * ape_score_lags scores every message against the truth rows of L = lag_max - lag_min + 1 lags in one pass, within recordings only.
 * Arguments up to n_bodies, score_dtype and stream: those of ape_score_rows, with the same meaning.
 *   Lag.   Recording r holds the frames [s_r, e_r) (s_r = seg_starts_host[r], e_r = the next start or F).  Its offset is
 *          o_r = rec_lag_host ? rec_lag_host[r] : 0.  Sweep index j = 0 .. L-1 stands, in recording r, for the lag l = o_r + lag_min + j.
 *          A positive lag means the estimate is late: message row f and spread row f are compared with truth row f - l.
 *   Pair.  The pair (f, l) of a frame f of recording r exists iff s_r <= f - l < e_r: a pair never crosses a recording boundary, and
 *          the truth row is converted (APE_TRUTH_TARGETS) with the body of that same recording.
 *   score_dev [F, L, APE_SCORE_WIDTH] of score_dtype, or NULL: [f, j, 0:7] are the seven values ape_score_rows defines, computed for the
 *          pair (f, l_j) -- message f, spread record f, truth f - l_j.  All seven are NaN if the pair does not exist or is not scorable
 *          (a non-finite value among the 25 of the message, or a non-finite truth value that is used).
 *   acc_dev f64 [R, L, APE_SCORE_ACC_WIDTH], or NULL (not both NULL): the accumulators run over a support common to all L lags, so
 *          that lags are compared on the same frames.  Frame f of recording r is in the support iff f - s_r >= skip and
 *          f - (o_r + lag_max) >= s_r and f - (o_r + lag_min) < e_r (then every one of its L pairs exists).  acc[r, j, 0:25] are the 25
 *          raw accumulators of ape_score_rows over the pairs (f, l_j), f in the support; [15] + [16] is therefore the same for every j
 *          of a recording (the size of its support) while a gap in the truth meets a different f at every lag.  A recording with an
 *          empty support (shorter than skip, or than the span of the sweep) gives zeros.
 * No floating-point atomics and a fixed order of summation: the same inputs give the same bits.  With lag_min = lag_max = 0 and no
 * offsets, score_dev and acc_dev receive the bits ape_score_rows writes for the same arguments.
 * Needs no model handle, runs on the current HIP device, does not wait; the host arrays (seg_starts_host, bodies_host, rec_lag_host)
 * have been consumed when it returns; the staging slots are those of ape_score_rows, taken and reused in the same way.
 * Refused with APE_ERR_INVALID_ARG on the host, before anything is written: everything ape_score_rows refuses; lag_min > lag_max;
 * L > APE_SCORE_MAX_LAGS; any |o_r + lag_min| or |o_r + lag_max| above APE_SCORE_MAX_LAG. */
#define APE_SCORE_MAX_LAG  128   /* bound on |lag| of any pair */
#define APE_SCORE_MAX_LAGS 65    /* bound on L = lag_max - lag_min + 1 */
int ape_score_lags(int32_t layout, const void* msg_dev, int32_t msg_stride, const void* spread_dev, int32_t spread_stride,
                   int32_t msg_dtype, const void* truth_dev, int32_t truth_kind, int32_t truth_dtype, int32_t F,
                   const int32_t* seg_starts_host, int32_t R, int32_t skip, const double* bodies_host, int32_t n_bodies,
                   int32_t lag_min, int32_t lag_max, const int32_t* rec_lag_host /* [R] or NULL */,
                   void* score_dev /* [F, L, 7] or NULL */, int32_t score_dtype, double* acc_dev /* f64 [R, L, 25] or NULL */,
                   void* stream);

/* ---- post-filter sweep: one replay's targets re-smoothed at many (smooth, samples) (additive in ABI 7) ------------------
 * replaces: for every configuration c and frame f, the tail of Estimator.add_xx_to_row_hist_and_make_prediction and
 * Estimator.msg_from_pred (estimate/estimator.py:108-118,122-137) of an estimator built with smooth = smooth_c and m_c Monte-Carlo
 * samples, incl. compose_msg.msg_from_nn_targets_est (estimate/compose_msg.py:13-108) and average_quaternions
 * (utility/transformations.py:32-51) -- from the normalised targets a replay returned (ape_replay*'s y_dev), without the regressor.
 *   y_dev f32 [F, n_mc, O]: frame f, sample k is row f * n_mc + k.  Sample k of a frame is the same draw whatever smooth is, and the
 *   first m samples of a frame are a valid m-sample estimate: one replay at the largest sample count holds every smaller configuration.
 *   configs_host int32 [C, 2]: (smooth_c, m_c), 1 <= smooth_c <= 64, 1 <= m_c <= n_mc, smooth_c * m_c <= 4096 (the limits of ape_replay).
 *   Stack.  Stack row i < smooth_c * m_c of frame f of a recording starting at s is sample i % m_c of frame
 *          max(s, f - smooth_c + 1 + i / m_c): ape_replay's rule with n_mc = m_c; samples k >= m_c of any frame are never read, and
 *          samples k >= max_c m_c are not even converted.  Every row goes through pred * yy_s + yy_m in float64 and the forward
 *          kinematics of ape_fk (the recording's body), once per call whatever C is; the sums run in ape_replay's order (row 0 first,
 *          the strict `dot < 0.0` flip against row 0, the FMA chain for the dot, one more in-order pass for the spread record).
 *   out_dev [C, F, 25] of out_dtype, with APE_FLAG_SPREAD [C, F, 25 + APE_SPREAD_WIDTH] (the record in the last 21 columns of a row).
 *          For m_c == n_mc, out[c] holds the bits ape_replay_bodies(smooth_c, n_mc, the same flag) writes into those columns.
 *   bodies_host f64 [n_bodies, 9] with n_bodies 1 or R, or NULL with n_bodies 0: the model's body (ape_model_set_body).
 *   workspace_bytes: bound on the device workspace for converted rows, whatever F is; 0 = 128 MiB.  With W = 21 (14 without hips),
 *          Mx = max_c m_c, H = max_c smooth_c - 1 and frame_bytes = 8 W Mx, a pass covers chunk = min(F, workspace_bytes /
 *          (2 frame_bytes) - H) frames (two buffers of H carried-over + chunk frames); ceil(F / chunk) passes; chunk < 1 is refused.
 *          Beside it the call keeps copies of its host arrays (4 R + 72 n_bodies bytes).  The result does not depend on the bound.
 *          Within a pass a workgroup stages its tile of frames and the H frames before it in LDS where that fits (and the tile gives
 *          its lanes enough (frame, configuration) pairs); otherwise the rows are read from the workspace.  Same bits either way.
 * The model handle supplies the target layout, yy_m / yy_s and the default body; no weights are read, and a DropoutFF or ImuPoseLSTM
 * handle serves as a DropoutLSTM one.  Not journaled: there is nothing for ape_model_recover to re-issue.  No floating-point atomics
 * and a fixed order of summation: the same inputs give the same bits.  The launches go on `stream` and the call does not wait for
 * them; the host arrays (seg_starts_host, configs_host, bodies_host) have been consumed when it returns.  (The workspace is kept per
 * device, shared with ape_post_window, and grows on demand, which may wait for the device; a call on another stream is ordered behind
 * the last user of either entry by an event.  The host arrays travel through pinned staging slots as ape_score_rows keeps them, the
 * post-filter's own: a call with more recordings or tapered windows than any before allocates its slot first, which may wait for the
 * device, and up to 8 calls may be in flight per device.)
 * Refused on the host before anything is written: NULL model / y_dev / out_dev / seg_starts_host / configs_host; F < 1, R < 1, bad
 * starts; F * n_mc >= 2^31; C < 1 or C > APE_POST_MAX_CONFIGS; smooth outside [1, 64], m outside [1, n_mc], smooth * m > 4096;
 * n_bodies not 0 / 1 / R (0 iff bodies_host is NULL); flags other than APE_FLAG_SPREAD; an unknown dtype; workspace_bytes < 0 or too
 * small for one frame (APE_ERR_INVALID_ARG); norm stats not set (APE_ERR_NOT_READY); APE_LAYOUT_NONE; a capturing stream.
 * ape_post_sweep_last: debug counter -- the plan of this thread's last successful ape_post_sweep: out4 = {passes, frames per pass,
 * frames per tile, 1 if the tiles were staged in LDS}. */
#define APE_POST_MAX_CONFIGS 64
int ape_post_sweep(ape_model_t* model, const float* y_dev, int32_t F, int32_t n_mc,
                   const int32_t* seg_starts_host, int32_t R,
                   const int32_t* configs_host /* [C,2]: smooth, samples */, int32_t C,
                   uint32_t flags /* APE_FLAG_SPREAD or 0 */,
                   const double* bodies_host /* [n_bodies,9] or NULL: the model's body */, int32_t n_bodies,
                   void* out_dev /* [C, F, 25 (+21)] */, int32_t out_dtype,
                   int64_t workspace_bytes, void* stream);
int ape_post_sweep_last(int32_t out4[4]);

/* ---- windowed post-filter: centred and tapered windows over one replay's targets (additive in ABI 7) -------------------
 * replaces: nothing; the reference smooths over the past alone (estimate/estimator.py:112-118), so its estimate trails the motion by
 * (smooth - 1) / 2 frames.  A recording processed offline can look ahead as far as it looks back (no group delay), and a window that
 * tapers towards its ends follows the motion's curvature where a boxcar of the same width flattens it.  ape_post_window re-smooths the
 * stored targets of ONE replay (ape_replay*'s y_dev, as ape_post_sweep) at C windows (back_c, ahead_c, m_c, weights_c) in one call.
 *   y_dev f32 [F, n_mc, O], seg_starts_host, bodies_host / n_bodies, flags, out_dtype, stream: those of ape_post_sweep.
 *   windows_host int32 [C, 3]: (back_c, ahead_c, m_c).  Window c takes n_c = back_c + ahead_c + 1 frames and m_c samples of each.
 *   Limits. back_c, ahead_c >= 0, n_c <= APE_POST_MAX_WINDOW, 1 <= m_c <= n_mc, n_c * m_c <= 4096, 1 <= C <= APE_POST_MAX_CONFIGS.
 *   Stack.  Frame f belongs to a recording [s, e).  Stack row i < N = n_c * m_c is sample i % m_c of frame
 *          min(e - 1, max(s, f - back_c + i / m_c)): both ends are clamped -- ape_replay's cold-start rule and its mirror image -- so N
 *          is the same for every frame and nothing is ever read across a recording boundary.  Samples k >= m_c of any frame are never
 *          read, and samples k >= max_c m_c are not converted.  Every row goes through pred * yy_s + yy_m in float64 and the forward
 *          kinematics of ape_fk (the recording's body), once per call whatever C is.
 *   Weights.  weights_host f64 [C, APE_POST_MAX_WINDOW], or NULL: uniform weights in every window.  The first n_c entries of row c are
 *          the weights w_0 .. w_{n_c - 1} of the window's frames, oldest frame first; the rest of the row is not read.  Every entry
 *          read must be finite and >= 0, and |sum_j w_j - 1| <= 1e-9 (summed in order, in float64), else the call is refused: the
 *          library does not normalise, the sum is a condition on the caller.  The weight of stack row i is u_i = w_{i / m_c} / m_c,
 *          one float64 division done on the host.
 *   Uniform windows.  A window is uniform if weights_host is NULL or the n_c entries of its row are bit-equal.  It runs the statements
 *          of ape_post_sweep / ape_replay unchanged apart from the two-sided clamp: row 0 times 1.0 / N first, every further row added
 *          with +-1/N by the strict `dot < 0.0` rule against row 0 (the dot as the FMA chain), the 20-target layout's origins summed in
 *          an in-order pass of their own and divided by N, one more in-order pass for the spread record.  So a uniform (smooth - 1, 0, m)
 *          holds the bits ape_post_sweep writes for (smooth, m), and a uniform (b, a, m) at frame f those of (b + a + 1, m) at frame
 *          f + a wherever f + a is a frame of the same recording.
 *   Tapered windows.  The same order and the same sign rule with u_i in place of 1/N: a = q_0 u_0, then a += q_i (+-u_i), i = 1 ..
 *          N - 1, the sign by `dot(q_i, q_0) < 0.0`; a row 0 of weight zero is still the sign reference.  The message's quaternions are
 *          a / |a|.  The 20-target layout's origins are sum_i u_i e_i, summed from +0.0 in stack order.  The spread record comes from
 *          the weighted sums sum u p, sum u (p_a p_b) and sum u (q_a q_b) taken in one in-order pass: the mean is the first sum, the
 *          covariance sum u p p' - mean mean', the angle 2 asin(sqrt(clip(1 - qm' (sum u q q') qm, 0, 1))) with the clamp by
 *          comparisons (a NaN passes, as through numpy.clip).  The weights sum to 1, so these are the weighted mean, the weighted
 *          population covariance and the weighted angular spread.
 *          N == 1 (a window of one frame and one sample; its one weight is 1): the row is copied, the record has zeros by rule.
 *   out_dev [C, F, 25] of out_dtype, with APE_FLAG_SPREAD [C, F, 25 + APE_SPREAD_WIDTH] (the record in the last 21 columns of a row).
 *   workspace_bytes: bound on the device workspace for converted rows, whatever F is; 0 = 128 MiB.  With W = 21 (14 without hips),
 *          Mx = max_c m_c, H = max_c back_c, A = max_c ahead_c and frame_bytes = 8 W Mx, a pass covers chunk = min(F, workspace_bytes /
 *          (2 frame_bytes) - H - A) frames (two buffers of H + chunk + A frames); ceil(F / chunk) passes; chunk < 1 is refused and the
 *          message names the smallest bound that works, 2 frame_bytes (H + A + 1).  The last H + A frames of a pass are carried to the
 *          front of the other buffer, so a row is converted once per call.  Beside the buffers the call keeps copies of its host arrays
 *          (4 R + 72 n_bodies bytes, and 8 APE_POST_MAX_WINDOW C bytes of row weights when a window is tapered).  The result does not
 *          depend on the bound.  Within a pass a workgroup stages its tile of frames, the H frames before and the A frames after it
 *          (clipped to [0, F)) and the weight table in LDS where that fits (and the tile gives its lanes enough (frame, window) pairs);
 *          otherwise rows and weights are read from the workspace.  Same statements and same bits either way.
 * The model handle supplies the target layout, yy_m / yy_s and the default body; no weights of the network are read.  Not journaled:
 * there is nothing for ape_model_recover to re-issue.  No floating-point atomics and a fixed order of summation: the same inputs give
 * the same bits.  The launches go on `stream` and the call does not wait for them; the host arrays (seg_starts_host, windows_host,
 * weights_host, bodies_host) have been consumed when it returns.  (The workspace is kept per device, the one ape_post_sweep uses, and
 * grows on demand, which may wait for the device; a call on another stream is ordered behind the last user by an event.  The host
 * arrays travel through the pinned staging slots ape_post_sweep names, taken and reused in the same way.)
 * Refused on the host before anything is written: NULL model / y_dev / out_dev / seg_starts_host / windows_host; F < 1, R < 1, bad
 * starts; n_mc < 1; F * n_mc >= 2^31; C < 1 or C > APE_POST_MAX_CONFIGS; back < 0, ahead < 0, n > APE_POST_MAX_WINDOW, m outside
 * [1, n_mc], n * m > 4096; a weight that is not finite or negative, a row that does not sum to 1 within 1e-9; n_bodies not 0 / 1 / R
 * (0 iff bodies_host is NULL); flags other than APE_FLAG_SPREAD; an unknown dtype; workspace_bytes < 0 or too small for one frame
 * (APE_ERR_INVALID_ARG); norm stats not set (APE_ERR_NOT_READY); APE_LAYOUT_NONE; a capturing stream.
 * ape_post_window_last: debug counter -- the plan of this thread's last successful ape_post_window: out4 = {passes, frames per pass,
 * frames per tile, 1 if the tiles were staged in LDS}. */
#define APE_POST_MAX_WINDOW 64
int ape_post_window(ape_model_t* model, const float* y_dev, int32_t F, int32_t n_mc,
                    const int32_t* seg_starts_host, int32_t R,
                    const int32_t* windows_host /* [C,3]: back, ahead, samples */,
                    const double* weights_host /* [C, APE_POST_MAX_WINDOW] or NULL */, int32_t C,
                    uint32_t flags /* APE_FLAG_SPREAD or 0 */,
                    const double* bodies_host /* [n_bodies,9] or NULL: the model's body */, int32_t n_bodies,
                    void* out_dev /* [C, F, 25 (+21)] */, int32_t out_dtype,
                    int64_t workspace_bytes, void* stream);
int ape_post_window_last(int32_t out4[4]);   /* passes, frames per pass, frames per tile, staged in LDS */

/* ---- speed-adaptive offline smoothing: a window per frame from a ladder (additive in ABI 7) -----------------------------
 * replaces: nothing; the reference smooths every frame over the same number of past frames (estimate/estimator.py:112-118).  Arm motion
 * is holds joined by reaches: a hold wants a wide window (noise averages away), a reach a narrow one (a wide one rounds the corner), and
 * any fixed width is a compromise.  Two device steps: ape_select_rungs chooses a rung of a ladder of windows for every frame from a
 * per-frame key (the hand speed), ape_post_select runs the post-filter at the rung chosen.
 *
 * ape_post_select: ape_post_window with a window per frame.
 *   y_dev, F, n_mc, seg_starts_host / R, flags, bodies_host / n_bodies, out_dtype, workspace_bytes, stream: those of ape_post_window.
 *   windows_host int32 [L, 3], weights_host f64 [L, APE_POST_MAX_WINDOW] or NULL: the ladder -- ape_post_window's list of windows under
 *          ape_post_window's limits and refusals, 1 <= L <= APE_POST_MAX_CONFIGS, kept in the caller's order.
 *   sel_dev uint8 [S, F] on the device, 1 <= S <= APE_POST_MAX_CONFIGS: sel[s, f] is the rung of frame f in set s.
 *   out_dev [S, F, 25] of out_dtype, with APE_FLAG_SPREAD [S, F, 25 + APE_SPREAD_WIDTH].  Row (s, f) holds the bits ape_post_window
 *          writes for window sel[s, f] of the same ladder at frame f, message and record.  A selector value >= L gives a row of NaN
 *          for that (s, f) and touches nothing else: the selector lives on the device and the call does not wait, so a bad value is
 *          not refused, it stays in its own row.
 *   The workspace rule is ape_post_window's with H, A and Mx the ladder's maxima (any frame may pick any rung); the result does not
 *          depend on the bound.  A tile is staged in LDS where it gives the lanes enough (frame, set) pairs: S counts where
 *          ape_post_window's C counts lanes, L where it sizes the weight table.
 * Not journaled; does not wait; the host arrays have been consumed when it returns; the workspace is the one ape_post_sweep and
 * ape_post_window use.  Refused on the host: everything ape_post_window refuses (under this entry's name); NULL sel_dev; S < 1 or
 * S > APE_POST_MAX_CONFIGS.
 * ape_post_select_last: debug counter -- the plan of this thread's last successful ape_post_select, as ape_post_window_last.
 *
 * ape_select_rungs: the selector, on the device, from device arrays alone (no model).
 *   keys_dev [S sets of F values] of keys_dtype (APE_F32 / APE_F64): key (s, f) is element s * set_stride + f * frame_stride, so a
 *          column of ape_motion_sums' per-frame rows [S, F, 12] goes in as it is (frame_stride 12, set_stride 12 F).
 *   edges_host f64 [B], finite and strictly increasing, 1 <= B <= APE_SELECT_MAX_EDGES; rung_of_slot_host int32 [B + 1], nan_rung:
 *          rungs, 0 .. L - 1.  reach_host int32 [L], 1 <= L <= APE_POST_MAX_CONFIGS: max(back, ahead) of every rung, 0 ..
 *          APE_POST_MAX_WINDOW - 1, non-decreasing -- the ladder runs narrow to wide.  slope k, 0 .. APE_SELECT_MAX_SLOPE.
 *   Rule.  slot = the number of edges strictly below the key (right-closed bins, ape_score_hist's rule); r0[f] = rung_of_slot[slot],
 *          or nan_rung for a key that is not finite.  k == 0: sel = r0.  Otherwise, with [s, e) the recording of f,
 *          cap[f] = min over g in [s, e) of reach[r0[g]] + |f - g| / k (integer division) and
 *          sel[f] = min(r0[f], the largest r with reach[r] <= cap[f]): a frame's reach does not exceed the reach chosen at g by more
 *          than |f - g| / k.  Nothing is read across a recording boundary.  Only frames within k (reach[L - 1] - reach[0]) <= 504
 *          frames of f can lower its cap; a workgroup stages the reaches of its 256 frames and that halo in LDS and every lane takes
 *          the minimum over its neighbourhood.  All integer: the same inputs give the same bits.
 *   sel_dev uint8 [S, F].
 * The launch goes on `stream` and the call does not wait; the host arrays have been consumed when it returns.
 * Refused on the host: a NULL pointer; an unknown dtype; F < 1, R < 1, bad starts; S or L outside 1 .. APE_POST_MAX_CONFIGS; B < 1 or
 * B > APE_SELECT_MAX_EDGES; slope outside 0 .. APE_SELECT_MAX_SLOPE; an edge that is not finite or not above the one before; a reach
 * outside 0 .. APE_POST_MAX_WINDOW - 1 or below the one before; a rung_of_slot entry or nan_rung outside 0 .. L - 1; frame_stride < 1,
 * a set_stride that does not clear a set; keys_dev not aligned to its element; sel_dev overlapping the keys; a capturing stream. */
#define APE_SELECT_MAX_EDGES 256
#define APE_SELECT_MAX_SLOPE 8
int ape_post_select(ape_model_t* model, const float* y_dev, int32_t F, int32_t n_mc,
                    const int32_t* seg_starts_host, int32_t R,
                    const int32_t* windows_host /* [L,3]: back, ahead, samples */,
                    const double* weights_host /* [L, APE_POST_MAX_WINDOW] or NULL */, int32_t L,
                    const uint8_t* sel_dev /* [S, F] */, int32_t S,
                    uint32_t flags /* APE_FLAG_SPREAD or 0 */,
                    const double* bodies_host /* [n_bodies,9] or NULL: the model's body */, int32_t n_bodies,
                    void* out_dev /* [S, F, 25 (+21)] */, int32_t out_dtype,
                    int64_t workspace_bytes, void* stream);
int ape_post_select_last(int32_t out4[4]);   /* passes, frames per pass, frames per tile, staged in LDS */
int ape_select_rungs(const void* keys_dev, int32_t keys_dtype, int32_t n_sets, int64_t set_stride, int32_t F, int64_t frame_stride,
                     const int32_t* seg_starts_host, int32_t R,
                     const double* edges_host /* [B] */, int32_t n_edges,
                     const int32_t* rung_of_slot_host /* [B + 1] */, int32_t nan_rung,
                     const int32_t* reach_host /* [L] */, int32_t L, int32_t slope,
                     uint8_t* sel_dev /* [S, F] */, void* stream);

/* ---- reaches and holds: segment a replay on the device and score each segment (additive in ABI 7) -------------------------
 * replaces: nothing; the reference has no counterpart.  4.43 and 4.44 treat arm motion as holds joined by reaches; these three entries say
 * where they are and reduce per-frame columns over each of them.  Device arrays only, no model handle; they run on the current HIP
 * device, launch on `stream` and do not wait; the host arrays have been consumed when they return.  Integers throughout in the first
 * two; no atomics on device memory and a stated order of summation in the third: the same inputs give the same bits.
 *
 * ape_segment_frames: a label per frame (0 hold, 1 move) from a key with hysteresis and minimum lengths.
 *   keys_dev, keys_dtype, n_sets S, set_stride, F, frame_stride, seg_starts_host / R: those of ape_select_rungs.
 *   thresholds_host f64 [P, 2] of (lo, hi), finite, lo <= hi; mins_host int32 [P, 2] of (min_hold, min_move), each 1 ..
 *          APE_SEGMENT_MAX_MIN; P = 1 (every set) or P = S (row s for set s).  first_label 0 or 1.
 *   Rule, per set and per recording [a, b), on the key widened to float64:
 *     1. frame f is decisive with d = 1 if v > hi, with d = 0 if v <= lo, and undecided otherwise.  NaN fails both compares and is
 *        undecided; infinities decide; lo == hi is a plain threshold.
 *     2. s[f] = d[g] at the last decisive g in [a, f], or first_label if there is none.  A recording never inherits from the one before.
 *     3. fill: a maximal run of s == 0 shorter than min_hold with a 1 on both sides inside the recording becomes 1; a run that touches
 *        either end of the recording stays.
 *     4. drop: after the fill, a maximal run of 1 shorter than min_move becomes 0, at the ends of the recording too.
 *   (1, 1) makes steps 3 and 4 no-ops.  Step 2 is a segmented scan in the reduce-then-scan shape of ape_frame_times: tiles of 1024 frames,
 *   a two-bit aggregate per tile and set, one workgroup per set scanning the aggregates, no workgroup waiting for another.  Steps 3 and 4
 *   read s within (min_hold - 1) + (min_move - 1) <= 510 frames on either side; a tile stages them in LDS, one byte each, from a scratch
 *   s in the call's slot.
 *   labels_dev uint8 [S, F].
 * ape_segment_runs: the run-length table of any uint8 labels (0 .. 255; ape_select_rungs' sel goes in as well).  A segment is a maximal
 *   run of equal labels inside one recording.
 *   seg_of_frame_dev int32 [S, F] or NULL: the id of the frame's segment, counted from 0 per set in frame order.
 *   n_segs_dev int32 [S]: the number of segments, at most F, whatever cap is.
 *   table_dev int32 [S, cap, APE_SEG_TABLE_WIDTH]: (recording, first frame, length, label) of segment id < cap.  Rows at or beyond cap are
 *          not written and nothing else changes: a caller that finds n_segs > cap calls again.  Rows n_segs .. cap - 1 are not written.
 *   A count of boundary flags gives the id and a running maximum of boundary positions the first frame, both in one reduce-then-scan
 *   pass; the last frame of a run writes its row.  No lane reads what another lane of the same launch wrote to device memory.
 * ape_segment_stats: per-segment reductions of V per-frame columns.
 *   values_dev of values_dtype (APE_F32 / APE_F64): value (s, f, v) is element s * set_stride + f * frame_stride + v * col_stride;
 *          n_value_sets = 1 (shared by all sets; set_stride is not read) or S.  1 <= V <= APE_SEG_MAX_VALUES.
 *   seg_of_frame_dev, table_dev, n_segs_dev, cap: what ape_segment_runs wrote for the same S, F and cap.
 *   out_dev f64 [S, cap, V, APE_SEG_STAT_WIDTH], per segment and column: the count of values that are not NaN; their sum; the sum of
 *          their squares; their maximum (-inf when the count is 0); the batch frame of the first occurrence of the maximum as a float64
 *          (-1 when the count is 0); the maximum is the value at that frame (of +0.0 and -0.0, which compare equal, the earlier one).
 *          A NaN is left out of its own cell only; infinities follow IEEE.  The rows of segments below
 *          min(n_segs, cap) are written whole and no other byte is touched.
 *   Order of summation (part of the contract).  A value is widened to float64; its square is rounded before it is added; a segment is cut
 *          into pieces of APE_SEG_PIECE frames counted from its own first frame; a piece is summed in frame order from +0.0 and the pieces
 *          are added in order from +0.0.  So a segment's record has the same bits wherever it lies in a batch and whichever set it is
 *          in, and a segment of up to APE_SEG_PIECE frames is a plain left-to-right sum.  score.py: segment_stats_numpy states it.
 *   A workgroup per aligned tile of APE_SEG_PIECE batch frames owns the pieces that start in it and its lanes take (piece, column) pairs;
 *   a first piece goes straight to out_dev, any other (at most one starts in a tile) to a workspace in the call's slot, and a second
 *   launch folds the pieces of every segment longer than one piece in order.  No atomics on device memory, no memset.
 * Refused with APE_ERR_INVALID_ARG on the host, before anything is written: a NULL pointer (but seg_of_frame_dev of ape_segment_runs);
 * an unknown dtype; F < 1, R < 1, bad starts; S outside 1 .. APE_POST_MAX_CONFIGS; P not 1 or S; n_value_sets not 1 or S; V outside
 * 1 .. APE_SEG_MAX_VALUES; a threshold that is not finite, hi < lo; a minimum length outside 1 .. APE_SEGMENT_MAX_MIN; first_label not 0
 * or 1; cap < 1; a stride below 1, a set_stride that does not clear a set; an extent past 63 bits; a pointer not aligned to its element;
 * an output overlapping an input or another output; a capturing stream. */
#define APE_SEGMENT_MAX_MIN 256
#define APE_SEG_TABLE_WIDTH 4
#define APE_SEG_MAX_VALUES 16
#define APE_SEG_STAT_WIDTH 5
#define APE_SEG_PIECE 1024
int ape_segment_frames(const void* keys_dev, int32_t keys_dtype, int32_t n_sets, int64_t set_stride, int32_t F, int64_t frame_stride,
                       const int32_t* seg_starts_host, int32_t R,
                       const double* thresholds_host /* [P, 2]: lo, hi */, const int32_t* mins_host /* [P, 2]: min_hold, min_move */,
                       int32_t P, int32_t first_label, uint8_t* labels_dev /* [S, F] */, void* stream);
int ape_segment_runs(const uint8_t* labels_dev /* [S, F] */, int32_t n_sets, int32_t F, const int32_t* seg_starts_host, int32_t R,
                     int32_t* seg_of_frame_dev /* [S, F] or NULL */, int32_t* n_segs_dev /* [S] */,
                     int32_t* table_dev /* [S, cap, 4] */, int32_t cap, void* stream);
int ape_segment_stats(const void* values_dev, int32_t values_dtype, int32_t n_value_sets, int64_t set_stride, int64_t frame_stride,
                      int64_t col_stride, int32_t V, int32_t n_sets, int32_t F,
                      const int32_t* seg_of_frame_dev /* [S, F] */, const int32_t* table_dev /* [S, cap, 4] */,
                      const int32_t* n_segs_dev /* [S] */, int32_t cap, double* out_dev /* [S, cap, V, 5] */, void* stream);

/* ---- each recording's heading and frame offset against the truth (additive in ABI 7) -------------------------------------
 * replaces: nothing; the reference has no counterpart.  Every input is calibrated against a forward direction taken from a calibration
 * pose; a wearer who stood a few degrees off, or a mocap frame that is not levelled, leaves the whole estimate of a recording turned
 * against the truth by a constant world-side rotation G, truth ~ G . estimate, which ape_score_rows books as error on every frame and
 * which ape_score_lags fits a lag to.  The least-squares G of a recording is read off sums of 3x3 products (score.py: best_frame);
 * ape_frame_sums takes those sums for every lag of a sweep in one pass, ape_rotate_rows applies a rotation to replay rows.
 * ape_frame_sums.  Arguments: those of ape_score_lags up to rec_lag_host with the same meaning, without spread_dev / spread_stride
 * (no spread record is read).  Pairing, the sign of a lag, the per-recording offsets, the support of the accumulators (skip, lag_max,
 * lag_min) and the bounds APE_SCORE_MAX_LAG / APE_SCORE_MAX_LAGS are ape_score_lags's; truth rows go through the same conversion; all
 * three layouts are served.
 *   Rotation of a quaternion q = [w, x, y, z]: with s = 2 / (w^2 + x^2 + y^2 + z^2), the rows [1 - s (yy + zz), s (xy - wz), s (xz + wy)],
 *   [s (xy + wz), 1 - s (xx + zz), s (yz - wx)], [s (xz - wy), s (yz + wx), 1 - s (xx + yy)]: an unnormalised quaternion is used as the
 *   rotation it stands for.  float64 with separate roundings.
 *   Per pair (message f, truth f - l), with E_j the matrices of msg[7:11], msg[14:18], msg[21:25], T_j those of the truth's lower-arm,
 *   upper-arm and hips quaternions, e_hand = msg[4:7], e_elbow = msg[11:14], t_hand and t_elbow the truth's positions,
 *   acc_dev f64 [R, L, APE_FRAME_ACC_WIDTH] receives over the support:
 *     [0:9], [9:18], [18:27]  sum of T_j E_j', row-major, j = lower arm, upper arm, hips.  APE_LAYOUT_ORI_CAL_LARM_UARM (no hips): the
 *                             hips block is exactly 0 (both sides are the identity there and would pull every fit towards "no turn")
 *     [27:36], [36:45]        sum of t_hand e_hand', sum of t_elbow e_elbow'
 *     [45:49]                 sum of |t_hand|^2, |e_hand|^2, |t_elbow|^2, |e_elbow|^2
 *     [49], [50]              pairs of the support that were summed / that were not
 *   A pair is summed iff ape_score_lags would score it (25 finite message values, every used truth value finite) and all of its 49
 *   terms are finite (a zero quaternion makes them non-finite).  [49] + [50] is the same for every lag of a recording; a recording
 *   with an empty support gives zeros.  No floating-point atomics and a fixed order of summation: the same inputs give the same bits.
 * Needs no model handle, runs on the current HIP device, does not wait; the host arrays have been consumed when it returns; staging
 * slots as ape_score_rows keeps them (its own: the first call of a size allocates, later ones do not).  Refused with
 * APE_ERR_INVALID_ARG on the host, before anything is written: everything ape_score_lags refuses (less the spread arguments and the
 * score dtype), a NULL acc_dev, a capturing stream.
 * ape_rotate_rows.  With g = quats_host[r] (one for all recordings, or one per recording), normalised on the host, and G its matrix:
 *   the four message quaternions [0:4], [7:11], [14:18], [21:25] become g (x) q (no sign flip: scoring is sign-blind); the three origins
 *   [4:7], [11:14], [18:21] become G p; of a spread record (spread_dev, or NULL) the two means become G m, the two covariances G S G'
 *   (six stored entries each, APE_SPREAD_WIDTH's order), the three angular spreads are copied.  NaN propagates.  Nothing past column 24
 *   of a message row is read (a packed row's cloud is not carried over).  APE_LAYOUT_ORI_CAL_LARM_UARM: the message's hips quaternion
 *   and constant shoulder origin are rotated like the rest -- the result describes the pose in the truth's frame.
 *   out_dev [F, 25] of out_dtype, with spread_dev [F, 25 + APE_SPREAD_WIDTH] (the record in the last 21 columns); it must not alias the
 *   inputs.  float64 arithmetic whatever the storage; one lane per frame, one launch.
 * Host behaviour as above.  Refused with APE_ERR_INVALID_ARG before anything is written: NULL msg_dev / seg_starts_host / quats_host /
 * out_dev, F < 1, R < 1, bad starts, strides too small, n_quats not 1 or R, a zero or non-finite quaternion, APE_LAYOUT_NONE or an
 * unknown layout / dtype, out_dev equal to an input, a capturing stream. */
#define APE_FRAME_ACC_WIDTH 51
int ape_frame_sums(int32_t layout, const void* msg_dev, int32_t msg_stride, int32_t msg_dtype, const void* truth_dev, int32_t truth_kind,
                   int32_t truth_dtype, int32_t F, const int32_t* seg_starts_host, int32_t R, int32_t skip, const double* bodies_host,
                   int32_t n_bodies, int32_t lag_min, int32_t lag_max, const int32_t* rec_lag_host /* [R] or NULL */,
                   double* acc_dev /* f64 [R, L, 51] */, void* stream);
int ape_rotate_rows(int32_t layout, const void* msg_dev, int32_t msg_stride, const void* spread_dev, int32_t spread_stride,
                    int32_t msg_dtype, int32_t F, const int32_t* seg_starts_host, int32_t R,
                    const double* quats_host /* [n_quats, 4], n_quats 1 or R, [w,x,y,z] */, int32_t n_quats,
                    void* out_dev /* [F, 25] or, with spread_dev, [F, 25 + 21] */, int32_t out_dtype, void* stream);

/* ---- mocap truth on each frame's clock (additive in ABI 7) -----------------------------------------------------------------
 * replaces: nothing; the reference has no counterpart.  Every scorer above pairs message row f with truth row f - l for an integer l
 * and expects one truth row per IMU frame.  A watch's frames sit on a jittered clock (column 0 of every raw row is sw_dt, the seconds
 * since the previous message) and a mocap system runs at its own rate with its own stamps and dropouts; and the lag best_lag refines
 * to a fraction of a frame cannot be applied by an integer pairing.  ape_frame_times builds a recording's clock on the device,
 * ape_resample_truth produces est-kind truth rows at each frame's time, which every scorer accepts; a row it cannot produce is all NaN,
 * which the scorers count as "could not be scored".  float64 with separate roundings for a * b + c; no floating-point atomics; no
 * workgroup waits for another inside a launch.
 * ape_frame_times.  dt_dev: one value per frame, dt_stride (>= 1) elements apart, of dt_dtype APE_F32 or APE_F64: column 0 of raw
 *   [F, 55 | 28] rows goes in without a copy (dt_stride 55 | 28).  flags: 0 or APE_PARSE_BIG_ENDIAN (APE_F32 only: the rows are UDP
 *   payloads as received).  For a recording [s_r, e_r) (seg_starts_host as in ape_score_rows): times_dev[s_r] = 0 and times_dev[f] = the
 *   sum of (double)dt[i] over s_r < i <= f; the first row's dt points before the recording and is not read into any sum.  A segmented
 *   inclusive scan in float64 whose association is fixed by F and the starts: |t[f] - exact| <= (f - s_r) 2^-53 sum|dt|, and the same
 *   inputs give the same bits.  A non-finite dt makes the times non-finite from its frame to the end of ITS recording and never reaches
 *   into the next one.  Three launches (per-tile aggregates, one workgroup scanning them, per-tile scan plus carry-in); one for F <= 1024.
 *   Refused with APE_ERR_INVALID_ARG on the host before anything is written: NULL dt_dev / seg_starts_host / times_dev, F < 1, R < 1,
 *   bad starts, dt_stride < 1, an unknown dtype or flag, the big-endian flag with APE_F64, times_dev equal to dt_dev, a capturing stream.
 * ape_resample_truth.  Recording r is the frames [s_r, e_r) of the estimate (seg_starts_host, F) and the rows [ts_r, te_r) of the truth
 *   (truth_starts_host, Ft), in the same order on both sides.  Frame clock tq(f) = times_dev[f], or with NULL the index clock
 *   (double)(f - s_r); truth clock tt(i) = truth_times_dev[i], or with NULL (double)(i - ts_r).  The query is u = tq(f) - shift_r
 *   (shift_host[r]; 0 with NULL): a positive shift means the estimate is late, the sign convention of ape_score_lags; with both clocks
 *   NULL the shift is a lag in frames, otherwise it is in the clocks' unit.  Truth times are assumed finite and non-decreasing inside a
 *   recording (the host cannot see them); whatever they hold, the search stays inside [ts_r, te_r) and nothing outside the buffers is
 *   read.  Frame times need not be monotonic.
 *   Conversion.  APE_TRUTH_TARGETS: a truth row [O] is first converted exactly as ape_score_rows converts it (the float64 forward
 *   kinematics with the recording's body, eigenvector-refined quaternions), est columns [6:9] being the hips quaternion applied to the
 *   body's shoulder origin, as ape_fk writes them.  APE_TRUTH_EST: the row [21 | 14] is taken as given.  bodies_host f64 [n_bodies, 9],
 *   n_bodies 1 or R, must be valid for either kind, as for ape_score_rows (it is staged with the other host arrays); its values
 *   are used for APE_TRUTH_TARGETS only.
 *   Output row f, out_dev [F, 21 | 14] of out_dtype, by these rules in this order:
 *     1. u is not finite: all NaN.
 *     2. i = the last row of [ts_r, te_r) with tt(i) <= u (binary search; of equal stamps the last); none: all NaN.
 *     3. u == tt(i): the converted row i itself, no arithmetic (est kind, float64 in and out: the bits of the input row, NaN included).
 *     4. i == te_r - 1 (past the last sample): all NaN.
 *     5. max_gap > 0 and tt(i+1) - tt(i) > max_gap: all NaN (a mocap dropout is not bridged).
 *     6. any value of the converted rows i or i + 1 is non-finite: all NaN.
 *     7. w = (u - tt(i)) / (tt(i+1) - tt(i)); position columns (hand, elbow, shoulder origin) a + w (b - a); each quaternion (lower arm,
 *        upper arm, and hips where the layout has them): a and b normalised, s = -1 where a . b < 0.0 else +1 (the flip rule of
 *        average_quaternions), theta = 2 asin(min(1, |a - s b| / 2)) (<= pi / 2 after the flip); theta < 1e-6: q = a + w (s b - a);
 *        otherwise q = (sin((1 - w) theta) a + sin(w theta) s b) / sin(theta); then q / |q|.
 *   An APE_F32 output is the float64 row rounded once.  One lane per output frame, one launch.
 * Both need no model handle, run on the current HIP device and do not wait; the host arrays have been consumed when they return;
 * staging slots as ape_score_rows keeps them (this file's own: the first call of a size allocates, later ones do not).
 * ape_resample_truth refuses with APE_ERR_INVALID_ARG on the host, before anything is written: everything ape_score_rows refuses about
 * layout, kind, dtypes, starts (both lists, each against its own row count) and bodies; Ft < 1; a NaN max_gap; a non-finite shift;
 * out_dev equal to an input; a capturing stream. */
int ape_frame_times(const void* dt_dev, int32_t dt_stride, int32_t dt_dtype, uint32_t flags, int32_t F,
                    const int32_t* seg_starts_host, int32_t R, double* times_dev /* f64 [F] */, void* stream);
int ape_resample_truth(int32_t layout, const void* truth_dev, int32_t truth_kind, int32_t truth_dtype, int32_t Ft,
                       const int32_t* truth_starts_host /* [R] */, const double* truth_times_dev /* f64 [Ft] or NULL */,
                       const double* times_dev /* f64 [F] or NULL */, int32_t F, const int32_t* seg_starts_host /* [R] */, int32_t R,
                       const double* shift_host /* f64 [R] or NULL */, double max_gap,
                       const double* bodies_host, int32_t n_bodies,
                       void* out_dev /* [F, 21 | 14] of out_dtype */, int32_t out_dtype, void* stream);

/* ---- each recording's arm lengths and shoulder origin against the truth (additive in ABI 7) -------------------------------
 * replaces: nothing; the reference reads a wearer's body from a skeleton file and has no fit.  Every position of a message is forward
 * kinematics of the message's own quaternions through nine numbers (larm_vec, uarm_vec, uarm_orig): with R_l, R_u, R_h the matrices of
 * the lower-arm, upper-arm and hips quaternions, elbow = R_h o + R_u v_u and hand = elbow + R_l v_l.  A wearer whose arm is not the
 * default's is booked as error on every frame.  The body enters linearly: the least-squares body of a recording solves a 9 x 9 system
 * whose entries are sums over the frames (score.py: best_body).  ape_body_sums takes those sums for every lag of a sweep in one pass,
 * ape_rebody_rows makes the positions of replay rows again under a body.
 * ape_body_sums.  Pairing (message f, truth f - l), the sign of a lag, the per-recording offsets, the support of the accumulators (skip,
 *   lag_max, lag_min), the bounds APE_SCORE_MAX_LAG / APE_SCORE_MAX_LAGS, strided message rows and the dtypes are ape_frame_sums's.
 *   rot_source APE_BODY_ROT_MSG: R_l, R_u, R_h are the matrices (ape_frame_sums's formula, an unnormalised quaternion is the rotation it
 *   stands for) of msg[7:11], msg[14:18], msg[21:25] -- the body that makes THIS estimator's positions fit; nothing else of a message
 *   row is read.  APE_BODY_ROT_TRUTH: they are those of the paired truth row's quaternions -- the wearer's skeleton from mocap alone;
 *   msg_dev may be NULL and is not read, the sweep must be the single lag 0 with rec_lag_host NULL.  APE_LAYOUT_ORI_CAL_LARM_UARM (no
 *   hips): R_h = I and msg[21:25] is not read.
 *   Truth: APE_TRUTH_EST rows [21 | 14] for every scoring layout (est columns [6:9], the shoulder origin, are not read); APE_TRUTH_TARGETS
 *   only for APE_LAYOUT_ORI_POS_CAL_LARM_UARM_HIPS, whose targets carry positions (converted as ape_score_rows converts them).
 *   With X'Y: out[3 a + b] = sum_k X[k, a] Y[k, b], X't: out[a] = sum_k X[k, a] t[k], t_h and t_e the truth's hand and elbow origins,
 *   acc_dev f64 [R, L, APE_BODY_ACC_WIDTH] receives over the support:
 *     [0:9], [9:18], [18:27]     sum of R_l'R_u, R_l'R_h, R_u'R_h
 *     [27:30], [30:33], [33:36]  sum of R_l't_h, R_u't_h, R_h't_h
 *     [36:39], [39:42]           sum of R_u't_e, R_h't_e
 *     [42], [43]                 sum of |t_h|^2, |t_e|^2
 *     [44], [45]                 pairs of the support that were summed / that were left out
 *   A pair is summed iff every quaternion value read for the rotations is finite, the truth row is one ape_score_lags would use (every
 *   used value finite) and all of its 44 terms are finite (a zero quaternion among the rotations makes them non-finite); a pair that is
 *   left out contributes exact zeros.  [44] + [45] is the same for every lag of a recording; an empty support gives zeros.  float64
 *   with separate roundings; no floating-point atomics and a fixed order of summation: the same inputs give the same bits.
 *   Refused with APE_ERR_INVALID_ARG on the host, before anything is written: what ape_frame_sums refuses about pointers (msg_dev only
 *   with APE_BODY_ROT_MSG), layout, kind, dtypes, starts, stride, skip and lags; an unknown rot_source; target truth of the two layouts
 *   whose positions would be made with the body being fitted; APE_BODY_ROT_TRUTH with a sweep or with rec_lag_host; a capturing stream.
 * ape_rebody_rows.  With b = bodies_host[r] (one for all recordings, or one per recording) = larm_vec, uarm_vec, uarm_orig and q (x) v
 *   the rotation of fk_device.h (q (0, v) q*, as ape_fk applies it): the four quaternions [0:4], [7:11], [14:18], [21:25] are copied;
 *   [18:21] = msg[21:25] (x) uarm_orig (APE_LAYOUT_ORI_CAL_LARM_UARM: uarm_orig itself), [11:14] = msg[14:18] (x) uarm_vec + [18:21],
 *   [4:7] = msg[7:11] (x) larm_vec + [11:14].  A non-finite quaternion makes only the positions that depend on it non-finite.  Nothing
 *   past column 24 of a message row is read; a spread record is not rewritten (its covariances cannot be made again from 21 values).
 *   out_dev [F, 25] of out_dtype, float64 arithmetic rounded once; it must not alias the input.  One lane per frame, one launch.
 *   Refused with APE_ERR_INVALID_ARG before anything is written: NULL msg_dev / seg_starts_host / bodies_host / out_dev, F < 1, R < 1,
 *   bad starts, msg_stride < 25, n_bodies not 1 or R, APE_LAYOUT_NONE or an unknown layout / dtype, APE_LAYOUT_ORI_POS_CAL_LARM_UARM_HIPS
 *   (its positions are predicted, not made from a body), out_dev equal to msg_dev, a capturing stream.
 * Both need no model handle, run on the current HIP device and do not wait; the host arrays have been consumed when they return; staging
 * slots as ape_score_rows keeps them (this file's own: the first call of a size allocates, later ones do not). */
#define APE_BODY_ACC_WIDTH 46
#define APE_BODY_ROT_MSG   0   /* rotations from the message's quaternions: the body that makes THIS estimator's positions fit */
#define APE_BODY_ROT_TRUTH 1   /* rotations from the truth's quaternions: the wearer's skeleton from mocap alone */
int ape_body_sums(int32_t layout, const void* msg_dev, int32_t msg_stride, int32_t msg_dtype, const void* truth_dev, int32_t truth_kind,
                  int32_t truth_dtype, int32_t F, const int32_t* seg_starts_host, int32_t R, int32_t skip, int32_t rot_source,
                  int32_t lag_min, int32_t lag_max, const int32_t* rec_lag_host, double* acc_dev /* [R, L, 46] */, void* stream);
int ape_rebody_rows(int32_t layout, const void* msg_dev, int32_t msg_stride, int32_t msg_dtype, int32_t F, const int32_t* seg_starts_host,
                    int32_t R, const double* bodies_host, int32_t n_bodies /* 1 | R */, void* out_dev /* [F, 25] */, int32_t out_dtype,
                    void* stream);

/* ---- how smooth a replay is: speed, acceleration and jerk of every frame (additive in ABI 7) ---------------------------------
 * replaces: nothing; the reference has no counterpart.  A longer `smooth` makes the arm stop shaking and costs lag; ape_score_lags measures
 * the lag, ape_motion_sums what it buys: the jerk of the joint positions (the literature's jitter), with the speeds and accelerations
 * beside it.  It needs no truth, so it is also the one score of a recording made without a mocap system.  It takes any rows that state an
 * arm pose, on the frames' own clock, for up to 64 sets of rows in one pass, and never pairs frames across a recording boundary.
 *   Sets.   Set c = 0 .. n_sets-1 (1 <= n_sets <= APE_POST_MAX_CONFIGS) is the F rows that start c * set_stride elements after rows_dev,
 *           rows_stride (>= the row width) elements apart, of rows_dtype: ape_post_sweep's out [C, F, 25] goes in as one call, strided
 *           views go in without a copy.  set_stride is not read with n_sets == 1.  The recordings (seg_starts_host, as ape_score_rows:
 *           recording r holds the frames [s_r, e_r)), the clock and the bodies are shared by all sets.
 *   Clock.  t(f) = times_dev[f] (ape_frame_times's output); with NULL the index clock (double)(f - s_r), and the results are in per-frame
 *           units (ape_resample_truth's convention).
 *   Pose of a row: hand p_h, elbow p_e, quaternions q_l, q_u, q_h of the lower arm, the upper arm and the hips.
 *           APE_ROWS_MSG      [25] message columns [4:7], [11:14], [7:11], [14:18], [21:25]; nothing else of the row is read
 *           APE_ROWS_EST      [21 | 14] est rows, as APE_TRUTH_EST (the shoulder origin [6:9] is not read)
 *           APE_ROWS_TARGETS  [O] de-normalised NN targets, converted as ape_score_rows converts truth, with the recording's body:
 *                             bodies_host f64 [n_bodies, 9], n_bodies 1 or R; read for this kind only, may be NULL otherwise
 *           APE_LAYOUT_ORI_CAL_LARM_UARM has no hips: q_h is the identity (message columns [21:25] are not read) and its three hips
 *           values are exactly 0.  Every quaternion is normalised before use: n = sqrt(w*w + x*x + y*y + z*z), each component / n.
 *   Per frame, APE_MOTION_WIDTH values.  h1 = t(f) - t(f-1), h2 = t(f-1) - t(f-2), h3 = t(f-2) - t(f-3).  All arithmetic is float64 with
 *           separate roundings, in the order written here (score.py: motion_sums_numpy repeats it operation for operation).  For a
 *           position p, per component, the divided differences
 *             d1(f) = (p(f) - p(f-1)) / h1,  d2(f) = (d1(f) - d1(f-1)) / (t(f) - t(f-2)),  d3(f) = (d2(f) - d2(f-1)) / (t(f) - t(f-3))
 *           (d1(f-1), d1(f-2) and d2(f-1) the same expressions one and two frames down, with h2, h3 and t(f-1) - t(f-3)) give the speed
 *           |d1(f)|, the acceleration 2 |d2(f)| and the jerk 6 |d3(f)|, |v| = sqrt(x*x + y*y + z*z) summed left to right.  On a uniform
 *           clock the jerk is |p(f) - 3 p(f-1) + 3 p(f-2) - p(f-3)| / h^3.  For a joint with unit quaternion q: d = q(f) (x) conj(q(f-1))
 *           (the product of fk_device.h), negated where d.w < 0.0; v its vector part, n = |v|; the world-frame angular velocity over the
 *           step is w(f) = (s v) / h1 with s = (2 atan2(n, d.w)) / n for n >= 1e-8 and s = 2 otherwise.  The angular speed is |w(f)|, the
 *           angular acceleration |w(f) - w(f-1)| / ((t(f) - t(f-2)) / 2), w(f-1) from q(f-1), q(f-2) and h2.
 *             [0:3]  hand speed, acceleration, jerk            [3:6]   elbow speed, acceleration, jerk
 *             [6:9]  angular speed of q_l, q_u, q_h            [9:12]  angular acceleration of q_l, q_u, q_h
 *   Row validity.  A row is all or nothing: it holds the 12 values iff f - s_r >= 3, every pose value used from rows f-3 .. f is finite
 *           (for target rows: every target of those rows), h1, h2 and h3 are finite and > 0 (a repeated or backward stamp is not
 *           differenced) and all 12 results are finite; otherwise all 12 are NaN.
 *   motion_dev [n_sets, F, APE_MOTION_WIDTH] of out_dtype (APE_F32: the float64 value rounded once), or NULL.
 *   acc_dev f64 [n_sets, R, APE_MOTION_ACC_WIDTH]: [3k], [3k+1], [3k+2] for k = 0..11 the sum, the sum of squares and the maximum of value
 *           k over the support of recording r, the frames with f - s_r >= skip + 3; [36] frames of the support that were summed, [37]
 *           frames of the support that were left out (NaN rows), which contribute exact zeros.  [36] + [37] = max(0, e_r - s_r - skip - 3),
 *           the same in every set; an empty support gives zeros.  No floating-point atomics; the order of summation is fixed by F, the
 *           starts and n_sets only, so the same inputs give the same bits, and each set's record has the bits of a call with n_sets = 1 on
 *           that set alone.  Raw accumulators, so pieces of a recording merge on the host (score.py: merge_motion).
 * Needs no model handle, runs on the current HIP device and does not wait; the host arrays have been consumed when it returns; staging
 * slots as ape_score_rows keeps them (this file's own: the first call of a size allocates, later ones do not).  Two launches; no
 * workgroup waits for another.  Refused with APE_ERR_INVALID_ARG on the host, before anything is written: NULL rows_dev / seg_starts_host /
 * acc_dev; F < 1, R < 1, bad starts, skip < 0; an unknown kind, dtype or layout, APE_LAYOUT_NONE; rows_stride below the row width; n_sets
 * outside 1 .. 64; n_sets > 1 with set_stride < F * rows_stride; APE_ROWS_TARGETS with NULL bodies_host or n_bodies not 1 or R; motion_dev
 * or acc_dev equal to an input (or to each other); a capturing stream. */
#define APE_MOTION_WIDTH      12
#define APE_MOTION_ACC_WIDTH  38
#define APE_ROWS_MSG      0   /* [25] message columns (compose_msg.py:72-78) */
#define APE_ROWS_EST      1   /* [21 | 14] est rows, as APE_TRUTH_EST */
#define APE_ROWS_TARGETS  2   /* [O] de-normalised NN targets, converted as ape_score_rows converts truth */
int ape_motion_sums(int32_t layout, const void* rows_dev, int32_t rows_kind, int32_t rows_stride, int32_t rows_dtype,
                    int32_t n_sets, int64_t set_stride, int32_t F, const int32_t* seg_starts_host, int32_t R, int32_t skip,
                    const double* times_dev /* f64 [F] or NULL */, const double* bodies_host, int32_t n_bodies,
                    void* motion_dev /* [n_sets, F, 12] of out_dtype, or NULL */, int32_t out_dtype,
                    double* acc_dev /* f64 [n_sets, R, 38] */, void* stream);

/* ---- the shape of the errors: a histogram per recording and column over fixed edges (additive in ABI 7) ----------------------
 * replaces: nothing; the reference has no counterpart.  The accumulators of ape_score_rows and ape_motion_sums give a mean, an RMS and one
 * worst frame; a median, a 95th percentile, the share of frames within 5 cm and the coverage of the spread record at every level are read
 * off counts over fixed edges.  Counts are raw, integers, and add across the pieces of a chained replay (score.py: merge_hist, quantiles,
 * fraction_within, pit).  ape_score_hist counts any per-frame rows that lie on the device: ape_score_rows' [F, 7], ape_score_lags'
 * [F, L, 7], ape_motion_sums' [n_sets, F, 12], strided views of wider rows.
 *   Values.  Value (c, f, g, w), c < n_sets, f < F, g < n_groups, w < width, is the element c * set_stride + f * frame_stride +
 *           g * group_stride + w of values_dev, of values_dtype (APE_F32 is widened exactly).  set_stride is not read with n_sets == 1,
 *           group_stride is not read with n_groups == 1.
 *   Window. Recording r holds the frames [s_r, e_r) (seg_starts_host, as ape_score_rows); its window is [s_r + trim[r][0], e_r - trim[r][1])
 *           (trim_host i32 [R, 2], both >= 0; NULL: zeros).  A window that is empty or inverted gives exact zeros.  The entry knows nothing
 *           of lags: the trims of a lag sweep's common support are made by the caller (score.py: lag_trim).
 *   Bins.   Column w has its own strictly increasing finite edges e[0 .. B] = edges_host[w][0 .. n_bins], B = n_bins.  Bins are closed on
 *           the right.  A value v is counted in exactly one of the B + 3 slots of its column:
 *             slot b, 0 <= b < B   e[b] < v <= e[b+1]
 *             slot B   (below)     v <= e[0]
 *             slot B+1 (above)     v > e[B], +inf included
 *             slot B+2             v is NaN
 *           Comparisons only, no arithmetic on v: -inf and -0.0 fall where <= puts them.  On the host: np.searchsorted(e, v, side="left").
 *           Every row [c][r][g][w][:] of the output therefore sums to the length of recording r's window.
 *   hist_dev i64 [n_sets, R, n_groups, width, n_bins + 3], all of it written by the call (the caller need not zero it: the zeroing is
 *           ordered on the stream in front of the kernel).  Integer counts, added with 64-bit integer atomics: the same inputs give the same
 *           bits whatever the order, and each (set, group) slice has the bits of a call on that slice alone.
 * Needs no model handle, runs on the current HIP device and does not wait; the host arrays have been consumed when it returns; staging
 * slots as ape_score_rows keeps them (this file's own).  One memset and one launch; no workgroup waits for another.  Refused with
 * APE_ERR_INVALID_ARG on the host, before anything is written: NULL values_dev / seg_starts_host / edges_host / hist_dev; F < 1, R < 1, bad
 * starts, a negative trim; width outside 1 .. APE_HIST_MAX_WIDTH; n_bins outside 1 .. APE_HIST_MAX_BINS; n_sets outside 1 ..
 * APE_POST_MAX_CONFIGS; n_groups outside 1 .. APE_SCORE_MAX_LAGS; frame_stride < width; n_groups > 1 with group_stride < width; n_sets > 1
 * with set_stride < F * frame_stride; an unknown dtype; a pointer not aligned to its element; edges that are not finite or not strictly
 * increasing; more than 2^31 - 1 output elements; values whose extent does not fit 63 bits; hist_dev overlapping values_dev; a capturing
 * stream. */
#define APE_HIST_MAX_BINS   256
#define APE_HIST_MAX_WIDTH  16
int ape_score_hist(const void* values_dev, int32_t values_dtype, int32_t width,
                   int32_t n_sets, int64_t set_stride, int32_t F, int64_t frame_stride,
                   int32_t n_groups, int64_t group_stride,
                   const int32_t* seg_starts_host, int32_t R, const int32_t* trim_host /* [R, 2] or NULL */,
                   const double* edges_host /* f64 [width, n_bins + 1] */, int32_t n_bins,
                   int64_t* hist_dev /* [n_sets, R, n_groups, width, n_bins + 3] */, void* stream);

/* ---- joint angles of every frame, and their errors against truth (additive in ABI 7) -------------------------------------
 * replaces: nothing; the reference has no counterpart.  ape_score_rows speaks in metres and whole-rotation angles; ape_joint_angles states
 * a pose as the angles its users ask in: elbow flexion, forearm twist, shoulder elevation and its plane, humeral twist, hips yaw.
 *   Sets, recordings, rows.  As ape_motion_sums: set c is the F rows c * set_stride elements after rows_dev, rows_stride apart, of
 *           rows_dtype; rows_kind APE_ROWS_MSG / APE_ROWS_EST / APE_ROWS_TARGETS (the last converted with bodies_host f64 [n_bodies, 9],
 *           n_bodies 1 or R, as ape_score_rows converts truth).  Only the quaternions q_l, q_u, q_h are used: of a message columns [7:11],
 *           [14:18], [21:25], of an est row [9:13], [13:17], [17:21] (without hips [6:10], [10:14]); no other column of such a row is
 *           read.  APE_LAYOUT_ORI_CAL_LARM_UARM has no hips: q_h is the identity.  Every quaternion is normalised before use:
 *           n = sqrt(w*w + x*x + y*y + z*z), each component / n.  A row states no pose, and all its seven values are NaN, where one of the
 *           twelve components is not finite (a target row: one of its targets or of the pose they convert to) or one of the three norms is
 *           not finite or not > 0.
 *   Conventions.  A bone's long axis is its local -x (larm_vec and uarm_vec are (-L, 0, 0)); the world is X right, Y up, Z forward.  With
 *           (x) the product of fk_device.h:  e = conj(q_u) (x) q_l, the forearm in the upper arm's frame;  s = conj(q_h) (x) q_u, the upper
 *           arm in the thorax frame.  All arithmetic is float64 with separate roundings, sums left to right, in the order written here
 *           (score.py: joint_angles_numpy repeats it operation for operation).
 *   Swing and twist of r = (w, x, y, z), all four negated first where w < 0.0:  rho = sqrt(w*w + x*x),  n = sqrt(y*y + z*z),
 *           swing = 2 atan2(n, rho) in [0, pi],  twist = 2 atan2(x, w) in [-pi, pi],  azimuth = atan2(y*x + z*w, y*w - z*x): the direction of
 *           the swing axis in the parent's y-z plane, r = swing (x) twist.
 *   Upper-arm direction in the thorax frame, from s = (w, x, y, z) as the product gave it:  dx = -((w*w + x*x) - (y*y + z*z)),
 *           dy = -(2 (x*y + w*z)),  dz = -(2 (x*z - w*y)),  h = sqrt(dx*dx + dz*dz).
 *   Per frame, APE_ANGLE_WIDTH values in radians:
 *             [0] elbow flexion = swing of e; 0 is a straight arm; the angle between the two bone axes         [0, pi]
 *             [1] hinge azimuth = azimuth of e                                                                  periodic
 *             [2] forearm twist = twist of e                                                                    periodic
 *             [3] shoulder elevation = atan2(h, -dy); 0 is hanging down                                         [0, pi]
 *             [4] plane of elevation = atan2(dz, -dx); 0 is out to the left, +pi/2 forward                      periodic
 *             [5] humeral twist = twist of s                                                                    periodic
 *             [6] hips yaw = 2 atan2(y_h, w_h), q_h negated first where w_h < 0.0; exactly 0 without hips       periodic
 *   Conditioning.  sh = sin(min_swing / 2), sf = sin(min_swing), computed on the host.  [1] is NaN iff n(e) < sh; [2] iff rho(e) < sh; [5]
 *           iff rho(s) < sh; [4] iff h < sf; every other value of a row that states a pose is stated.  min_swing = 0 states everything
 *           (atan2(0, 0) = 0).
 *   Errors, with truth_dev only: F truth rows of truth_kind (any of the three, whatever rows_kind is), truth_stride apart, of truth_dtype,
 *           shared by all sets; rec_lag_host i32 [R] (NULL: zeros).  Frame f of recording r is paired with truth row f - l_r, which must lie
 *           in [s_r, e_r), else its seven errors are NaN.  err_k = a_k(row) - a_k(truth); for the periodic columns it is folded once (> pi:
 *           less 2 pi; <= -pi: plus 2 pi); NaN where either side is NaN.
 *   angles_dev, errors_dev [n_sets, F, APE_ANGLE_WIDTH] of out_dtype (APE_F32: the float64 value rounded once), or NULL.
 *   acc_dev f64 [n_sets, R, APE_ANGLE_ACC_WIDTH] or NULL, over the support f - s_r >= skip:  [5k .. 5k+4] the sum, the sum of squares, the
 *           minimum, the maximum and the count of the finite values of angle k (none: +inf and -inf);  [35+5k .. 35+5k+4] the sum of the
 *           finite errors of angle k, the sum of their magnitudes, the sum of their squares, the largest magnitude and their count (all
 *           zeros without truth);  [70] the frames of the support, max(0, e_r - s_r - skip).  Counts are exact.  No floating-point atomics;
 *           the order of summation is fixed by F and the starts, so the same inputs give the same bits, and each set's record has the bits
 *           of a call on that set alone.  Raw accumulators: pieces of a recording merge on the host (score.py: merge_angles).
 * A frame of a live bank is the same call: [S, 25] messages, R = 1, no accumulators.  Needs no model handle, runs on the current HIP device
 * and does not wait; the host arrays have been consumed when it returns; staging slots as ape_score_rows keeps them (this file's own).  At
 * most three launches (the truth's angles once for all sets, the frames, the accumulators); no workgroup waits for another.  Refused with
 * APE_ERR_INVALID_ARG on the host, before anything is written: NULL rows_dev / seg_starts_host; all three outputs NULL; errors_dev without
 * truth_dev; F < 1, R < 1, bad starts, skip < 0; an unknown kind, dtype or layout, APE_LAYOUT_NONE; rows_stride or truth_stride below the
 * row width; n_sets outside 1 .. 64; n_sets > 1 with set_stride < F * rows_stride; APE_ROWS_TARGETS on either side with NULL bodies_host or
 * n_bodies not 1 or R; min_swing not in [0, pi / 2); an output equal to an input or to another output; a capturing stream. */
#define APE_ANGLE_WIDTH      7
#define APE_ANGLE_ACC_WIDTH  71
int ape_joint_angles(int32_t layout, const void* rows_dev, int32_t rows_kind, int32_t rows_stride, int32_t rows_dtype,
                     int32_t n_sets, int64_t set_stride,
                     const void* truth_dev /* or NULL */, int32_t truth_kind, int32_t truth_stride, int32_t truth_dtype,
                     const int32_t* rec_lag_host /* [R] or NULL */,
                     int32_t F, const int32_t* seg_starts_host, int32_t R, int32_t skip,
                     const double* bodies_host, int32_t n_bodies, double min_swing,
                     void* angles_dev /* [n_sets, F, 7] or NULL */, void* errors_dev /* [n_sets, F, 7] or NULL */, int32_t out_dtype,
                     double* acc_dev /* f64 [n_sets, R, 71] or NULL */, void* stream);

/* ---- errors by condition: per-slot sums of any per-frame column keyed by any other (additive in ABI 7) --------------------
 * replaces: nothing; the reference has no counterpart.  The scorers state their numbers per recording; ape_score_by states one per-frame
 * column as a function of another: the hand error over the elbow flexion, the error over the hand speed, each sigma bin's RMS error (a
 * reliability curve).  Keys are binned over fixed edges as ape_score_hist bins values; per slot, every value column gets a count, a sum, a
 * sum of squares and a maximum.
 *   Keys.   Key (c, f, k), c < n_sets, f < F, k < n_keys <= APE_BY_MAX_KEYS, is the element c * keys_set_stride + f * keys_frame_stride + k
 *           of keys_dev, of keys_dtype (APE_F32 is widened exactly).  A set stride of 0 shares the one key set among all sets; it is not
 *           read with n_sets == 1.
 *   Values. Value (c, f, v), v < n_values <= APE_BY_MAX_VALUES, is the element c * values_set_stride + f * values_frame_stride + v of
 *           values_dev, of values_dtype; its set stride may be 0 as well.
 *   Window. Recordings, seg_starts_host, trim_host [R, 2] and empty or inverted windows exactly as ape_score_hist states them.
 *   Slots.  Key column k has its own strictly increasing finite edges e[0 .. B] = edges_host[k][0 .. n_bins], B = n_bins <=
 *           APE_BY_MAX_BINS.  A key falls into one of B + 3 slots by ape_score_hist's rule -- bins closed on the right, then below (B),
 *           above (B + 1), NaN (B + 2) -- by comparisons only.  (125 bins: ape_score_hist's 72 angle bins fit, and B + 3 <= 128.)
 *   Cell.   For every (set, recording, key column, slot, value column), four float64 accumulators over the frames f of the recording's
 *           window whose key k lies in the slot and whose value x = value (c, f, v) is not NaN:
 *             [0] n, the count of such frames          [1] the sum of x
 *             [2] the sum of x * x, the product rounded to float64, then added (no fused multiply-add)
 *             [3] the maximum of x; -inf for an empty cell
 *           A NaN value is left out of its own cell only.  +-inf are counted and follow IEEE (a cell that holds both has a NaN sum).
 *   Order.  This is part of the contract.  The window is cut into pieces of APE_BY_PIECE consecutive frames, counted from the window's
 *           first frame (not from the batch's or the recording's).  Within a piece a cell's terms are added in frame order, starting from
 *           +0.0; a cell's piece sums are added in piece order, starting from +0.0.  A recording's record therefore has the same bits
 *           wherever it lies in the batch, whatever else is in the batch and whatever the grid is; a call with a trim has the bits of a
 *           call on the sliced tensors; each set has the bits of a call on that set alone.  On the host: score.py, stats_by_numpy.
 *   by_dev  f64 [n_sets, R, n_keys, n_bins + 3, n_values, 4], all of it written by the call (no zeroing needed).  No floating-point
 *           atomics; no workgroup waits for another.
 * Needs no model handle, runs on the current HIP device and does not wait; the host arrays have been consumed when it returns.  The piece
 * records, n_sets * pieces * n_keys * (n_bins + 3) * n_values * 4 doubles, live in the staging slot's device block (slots as
 * ape_score_rows keeps them, this file's own), as ape_motion_sums' partial records do.  Two launches.  Refused with APE_ERR_INVALID_ARG on
 * the host, before anything is written: NULL keys_dev / values_dev / seg_starts_host / edges_host / by_dev; F < 1, R < 1, bad starts, a
 * negative trim; n_sets outside 1 .. APE_POST_MAX_CONFIGS; n_bins outside 1 .. APE_BY_MAX_BINS; n_keys outside 1 .. APE_BY_MAX_KEYS;
 * n_values outside 1 .. APE_BY_MAX_VALUES; an unknown dtype; a frame stride below its side's columns; n_sets > 1 with a set stride that is
 * neither 0 nor at least F * frame_stride; an extent that does not fit 63 bits; a pointer not aligned to its element; edges that are not
 * finite or not strictly increasing; more than 2^31 - 1 output elements; more than 1 GiB of piece records (the message states the size);
 * by_dev overlapping keys_dev or values_dev; a capturing stream. */
#define APE_BY_MAX_KEYS    8
#define APE_BY_MAX_VALUES  16
#define APE_BY_MAX_BINS    125
#define APE_BY_PIECE       1024
int ape_score_by(const void* keys_dev, int32_t keys_dtype, int32_t n_keys, int64_t keys_set_stride, int64_t keys_frame_stride,
                 const void* values_dev, int32_t values_dtype, int32_t n_values, int64_t values_set_stride, int64_t values_frame_stride,
                 int32_t n_sets, int32_t F, const int32_t* seg_starts_host, int32_t R, const int32_t* trim_host /* [R, 2] or NULL */,
                 const double* edges_host /* f64 [n_keys, n_bins + 1] */, int32_t n_bins,
                 double* by_dev /* f64 [n_sets, R, n_keys, n_bins + 3, n_values, 4] */, void* stream);

/* ---- spectra of a replay: Welch sums of power, truth power and cross spectrum per frequency (additive in ABI 7) --------------
 * replaces: nothing; the reference has no counterpart.  The scorers say how wrong a replay is, at which lag and how much it shakes;
 * ape_spectra says at which frequencies: the raw sums from which the host forms a power spectral density, the gain and phase of the
 * estimate against the truth, the coherence and the spectrum of the error (score.py: summarise_spectra, bandwidth, band_power).  Without
 * truth it gives the power spectrum of any per-frame column.
 *   Rows.   Element (s, f, v), s < n_sets, f < F, v < V, of x lies x_set_stride * s + x_frame_stride * f + x_cols_host[v] elements after
 *           x_dev, of x_dtype (APE_F32 is widened exactly first): messages [C, F, 25], est rows, ape_motion_sums' [C, F, 12] and
 *           ape_joint_angles' [C, F, 7] go in as they lie.  x_set_stride is not read with n_sets == 1.  y_dev (the truth; NULL: none, and
 *           the y arguments are not read) is addressed the same way with its own dtype, strides and y_cols_host; y_set_stride == 0 is one
 *           truth shared by all sets.
 *   Segments.  Recording r holds the frames [s_r, e_r) (seg_starts_host, as ape_score_rows).  Segment j of recording r is the N frames
 *           s_r + skip + j * hop + [0, N), j < J_r = max(0, floor((e_r - s_r - skip - N) / hop) + 1): a segment never crosses a recording
 *           boundary.  N is a multiple of 16 in 16 .. APE_SPECTRA_MAX_N, hop in 1 .. N.
 *   Per segment and column, in float64.  m = the mean of the segment's N values with APE_SPECTRA_DETREND (the sum of the N values, then
 *           / N), else 0.  a_n = w_n * (x_n - m), w = taper_host f64 [N].  X(k) = sum_n a_n (cos t - i sin t), t = 2 pi ((k n) mod N) / N,
 *           k = 0 .. N/2; cos and sin from a table of N entries made on the host (the float64 nearest to each).  Y(k) likewise from y.  The
 *           sum over n is the chain of v_mfma_f64_16x16x4_f64, fused multiply-adds in rising n from +0.0; where N is a multiple of 32, bin
 *           N/2 is sum_n a_n (-1)^n (its sine is 0) added on the vector unit, 64 interleaved partial sums and a butterfly over them.
 *   acc_dev f64 [n_sets, R, V, N/2 + 1, W], raw sums over the recording's segments: [0] sum |X|^2 = re * re + im * im; with truth (W = 4)
 *           [1] sum |Y|^2, [2] and [3] the real and imaginary part of sum conj(Y) X, re(Y) re(X) + im(Y) im(X) and re(Y) im(X) - im(Y) re(X):
 *           the cross spectrum from the truth to the estimate.  Without truth W = 1.  Separate roundings in the products and sums.
 *   counts_dev i32 [n_sets, R, V, 2]: segments summed, segments left out; the two add to J_r.  A segment is left out for a column, and for
 *           that column only, if any of its N values on either side is not finite; it contributes exact zeros.
 *   Order.  This is part of the contract.  A recording's segments are taken in tiles of 16, counted from its first.  Within a tile, bin
 *           k's terms of segments q, q + 4, q + 8, q + 12 are added in that order for q = 0 .. 3, the four sums in the order of q; the
 *           tile's sum is added to the sum of the tiles before it, the first tile to +0.0.  No floating-point atomics.  The same inputs
 *           give the same bits; a set's record has the bits of a call with n_sets = 1 on that set; a recording's record has the same bits
 *           wherever it lies in a batch; [0] of a call with truth whose truth is finite has the bits of the call without.
 * Needs no model handle, runs on the current HIP device and does not wait; the host arrays have been consumed when it returns; staging
 * slots as ape_score_rows keeps them (this file's own).  One launch, all of both outputs written; no workgroup waits for another.
 * Refused with APE_ERR_INVALID_ARG on the host, before anything is written: NULL x_dev / x_cols_host / seg_starts_host / taper_host /
 * acc_dev / counts_dev, y_dev with NULL y_cols_host; F < 1, R < 1, bad starts, skip < 0; N not a multiple of 16 in 16 .. 512; hop outside
 * 1 .. N; V outside 1 .. APE_SPECTRA_MAX_COLS; n_sets outside 1 .. APE_POST_MAX_CONFIGS; unknown flags or dtype; a frame stride below 1; a
 * column offset below 0 or at or beyond its side's frame stride; n_sets > 1 with a set stride below F * frame_stride (x; y unless 0): the
 * sets overlap; an extent that does not fit 63 bits; an output overlapping an input or the other output; a capturing stream. */
#define APE_SPECTRA_DETREND   0x1u
#define APE_SPECTRA_MAX_N     512
#define APE_SPECTRA_MAX_COLS  16
int ape_spectra(const void* x_dev, int32_t x_dtype, int64_t x_set_stride, int64_t x_frame_stride, const int32_t* x_cols_host /* [V] */,
                const void* y_dev /* or NULL */, int32_t y_dtype, int64_t y_set_stride, int64_t y_frame_stride,
                const int32_t* y_cols_host /* [V] */, int32_t V, int32_t n_sets, int32_t F, const int32_t* seg_starts_host, int32_t R,
                int32_t skip, int32_t N, int32_t hop, const double* taper_host /* f64 [N] */, uint32_t flags,
                double* acc_dev /* f64 [n_sets, R, V, N/2 + 1, W] */, int32_t* counts_dev /* i32 [n_sets, R, V, 2] */, void* stream);

/* ---- the output layer fitted to a wearer: hidden features, fit sums, installing a head (additive in ABI 7) -------------------
 * replaces: nothing; the reference has no counterpart.  The scorers say how wrong a replay is and ape_score_lags / ape_frame_sums /
 * ape_body_sums take three wearer-specific errors out of it; the regressor's own error stays, its output_layer being the same for every
 * wearer.  A linear probe keeps the LSTM and fits the head again on a recording of the wearer with truth: the features h of every frame
 * (ape_lstm_features, ape_replay_features), the normal-equation sums of [h, 1, t] per recording (ape_fit_sums), a small solve on the host
 * (score.py: best_head, sweep_ridge) and the new head installed (ape_model_set_head).  DropoutLSTM handles only: APE_MODEL_FF and
 * APE_MODEL_IMUPOSE are refused with APE_ERR_UNSUPPORTED by the four entries that take a handle.
 * ape_lstm_features.  ape_lstm_forward's arguments and meaning with one more output: h_dev f32 [B, H] receives h^{L-1}_{T-1}, the top
 *   layer's output of the last step -- the vector the head multiplies -- and y_dev f32 [B, O] (or NULL) what the same launch's head makes
 *   of it.  Every row runs on ape_lstm_tile16<H, L, 4, true>, the batch-tile kernel with the store (ape_model_last_kernel: "ape_lstm_tile16<hout>"), whatever ape_lstm_forward's planner would
 *   pick for (B, T): y_dev has the bits of ape_lstm_forward under ape_model_set_kernel(APE_KERNEL_TILE16), with the same Philox masks.
 *   Flags: APE_FLAG_NORMALIZE_INPUT and the two dropout modes.  Refused: APE_FLAG_ALL_STEPS and every other flag bit
 *   (APE_ERR_INVALID_ARG), fp16 precision set on the model (APE_ERR_UNSUPPORTED), and what ape_lstm_forward refuses.  Stream, capture,
 *   journal and recover rules are ape_lstm_forward's: it does not wait, may be captured, and is re-issued behind an aborted launch.
 * ape_replay_features.  h_dev f32 [F, H] and y_dev f32 [F, O] (or NULL) of every frame of R recordings: ape_replay's feature rows and
 *   windows (kind, rows_dev, seg_starts_host, seq_len, max_rows_per_launch and APE_FLAG_NORMALIZE_INPUT as there; every recording starts
 *   cold exactly as ape_replay starts it), then ape_lstm_features per chunk.  One row per frame, no dropout, no post-filter, no state in
 *   or out: y_dev is ape_replay's y_dev at n_mc = 1 up to the kernels' rounding, and the bits do not depend on the chunking.  Blocking,
 *   like ape_replay; not on a capturing stream.
 * ape_fit_sums.  M = P + 1 + Q.  Recording r holds the frames [s_r, e_r) and has the lag l_r = rec_lag_host ? rec_lag_host[r] : 0;
 *   pairing and the sign of a lag are ape_score_lags's: x row f goes with t row f - l_r.  Its support is the frames f with
 *   f - s_r >= skip and s_r <= f - l_r < e_r.  With z_f = [x_f (P values), 1, (t_{f - l} - shift) / scale (Q values)] in float64 (f32 is
 *   widened exactly; shift = t_shift_host or zeros, scale = t_scale_host or ones: an estimator's yy_m / yy_s, so that de-normalised
 *   targets are fitted in the head's own units), acc_dev f64 [R, M * M + 2] receives
 *     [i * M + j]     sum over the support of z_f[i] z_f[j], the full symmetric matrix: G = x'x in [0:P, 0:P], sum x in row / column P,
 *                     the count at [P, P], C = x't in [0:P, P+1:M], sum t in [P, P+1:M], t't in [P+1:M, P+1:M]
 *     [M * M], [M * M + 1]   pairs of the support that were summed / that were left out
 *   x element (f, i) lies x_stride * f + i elements after x_dev (x_dtype), t element (f, q) t_stride * f + q after t_dev (t_dtype): any
 *   columns of wider rows go in as they lie.  A pair is left out iff any of its P + Q values is not finite (or a finite truth value
 *   overflows under shift and scale); it contributes exact zeros to every sum, the count included.
 *   Order.  This is part of the contract.  A support is cut into pieces of APE_FIT_PIECE frames counted from its first frame.  Within a
 *   piece every sum is one chain of v_mfma_f64_16x16x4_f64 from +0.0 in rising f, four frames per instruction (fused multiply-adds);
 *   the pieces' sums are added in piece order, the first to +0.0.  Entry (i, j) with i > j is a copy of (j, i).  No floating-point
 *   atomics, no memset: the same inputs give the same bits, a recording's record has the same bits wherever it lies in a batch, and the
 *   records of a recording cut at a multiple of APE_FIT_PIECE frames of its support add up to the pieces of the whole (score.py:
 *   merge_fit).
 *   Needs no model handle, runs on the current HIP device and does not wait; the host arrays have been consumed when it returns; staging
 *   slots as ape_score_rows keeps them (this file's own).  Two launches, all of acc_dev written.
 *   Refused with APE_ERR_INVALID_ARG on the host, before anything is written: NULL x_dev / t_dev / seg_starts_host / acc_dev; P not a
 *   multiple of 16 in 16 .. APE_FIT_MAX_P; Q outside 1 .. APE_FIT_MAX_Q; F < 1, R < 1, bad starts, skip < 0; an unknown dtype; x_stride
 *   below P or t_stride below Q; a pointer not aligned to its element; a shift that is not finite, a scale that is not finite or zero;
 *   |l_r| above APE_SCORE_MAX_LAG; acc_dev overlapping an input; more than 1 GiB of piece records; a capturing stream.
 * ape_model_set_head / ape_model_get_head.  w_out_host f32 [O, H], b_out_host f32 [O]: output_layer.weight and .bias, the tail of
 *   ape_model_load_weights' blob.  Synchronous, like ape_model_load_weights: the handle is first made healthy and idle (ape_model_recover,
 *   then a wait for the device), so every call issued before runs on the head it was issued with; every call after runs on the new one,
 *   on every route, in banks and replays too -- no kernel of a DropoutLSTM handle keeps a packed copy of the head.  APE_ERR_NOT_READY
 *   before weights are loaded. */
#define APE_FIT_PIECE  512
#define APE_FIT_MAX_P  256
#define APE_FIT_MAX_Q  32
int ape_lstm_features(ape_model_t* model, const float* x_dev, int32_t B, int32_t T, uint32_t flags, const float* masks_dev,
                      float dropout_p, uint64_t seed, float* h_dev /* f32 [B, H] */, float* y_dev /* f32 [B, O] or NULL */, void* stream);
int ape_replay_features(ape_model_t* model, int32_t kind, const float* rows_dev, int32_t F, const int32_t* seg_starts_host, int32_t R,
                        int32_t seq_len, uint32_t flags, float* h_dev /* f32 [F, H] */, float* y_dev /* f32 [F, O] or NULL */,
                        int32_t max_rows_per_launch, void* stream);
int ape_fit_sums(const void* x_dev, int64_t x_stride, int32_t x_dtype, int32_t P, const void* t_dev, int64_t t_stride, int32_t t_dtype,
                 int32_t Q, const double* t_shift_host /* f64 [Q] or NULL */, const double* t_scale_host /* f64 [Q] or NULL */, int32_t F,
                 const int32_t* seg_starts_host, int32_t R, int32_t skip, const int32_t* rec_lag_host /* i32 [R] or NULL */,
                 double* acc_dev /* f64 [R, M * M + 2] */, void* stream);
int ape_model_set_head(ape_model_t* model, const float* w_out_host /* f32 [O, H] */, const float* b_out_host /* f32 [O] */);
int ape_model_get_head(ape_model_t* model, float* w_out_host /* f32 [O, H] */, float* b_out_host /* f32 [O] */);

#ifdef __cplusplus
}
#endif
#endif /* APE_HIP_H */
