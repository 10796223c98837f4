// Internal declarations shared by the C-ABI (ape_api.hip, api_*.hip) and the gfx950 kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/ape_hip.h"

#define APE_MAX_LAYERS 3
#define APE_MAX_INPUT 64
#define APE_MAX_OUTPUT 32
#define APE_TILE_ROWS 16          // windows per workgroup in the batch-tile LSTM kernel
#define APE_XCC_WORDS 1024
#define APE_C32_HSHIFT 15         // lstm_cluster32.hip: exchanged h values are split as f16 hi / lo of h * 2^15 (|h| <= 1: hi stays below 65504)
#define APE_C32_ENDS_MAX_T 8      // lstm_cluster32.hip: windows of up to this many steps run the instantiation with the end forms
#define APE_LDS_BYTES (160 * 1024) // LDS of a gfx950 CU: the dynamic-LDS limit every kernel instantiation is raised to, once
// internal timing-only ablation switches: the diagnostic builds alone (make diag / make ablate) read them, outputs are wrong.  Their bit
// values overlap with NO public flag or selector of include/ape_hip.h (round 5: two of them used to).
#define APE_DIAG_NO_EXCHANGE 0x40000000u
#define APE_DIAG_NO_ACT      0x20000000u
#define APE_DIAG_STAMP       0x10000000u
#define APE_DIAG_NO_MFMA     0x04000000u   // fp16 v2 / upper-layer kernel: skip the matrix work
#define APE_DIAG_NO_XSTAGE   0x00200000u   // ... skip the staging / fetch of the next step's inputs
#define APE_DIAG_NO_BARRIER  0x00100000u   // upper-layer kernel: no workgroup barrier at a section's top

#define APE_FLAG_XCD_CLASSES 0x00800000u   // internal (set by the launcher): the first-generation kernel forms its clusters within block-index classes
#define APE_FLAG_LV16_SINGLE 0x00800000u   // internal (set by the launcher, lstm_level16.hip only -- the same bit means nothing else there): one row tile per cluster

// Hand-over form of a flag-based kernel, in one place: plain (write-back) payload stores ONLY when the caller opted in with
// APE_FLAG_IN_XCD_PLAIN AND the cluster verified at run time that all its members share an XCD (`same_xcd`); otherwise write-through.
#define APE_HANDOVER_IN_L2(flags, same_xcd) ((same_xcd) && ((flags) & APE_FLAG_IN_XCD_PLAIN) != 0u && ((flags) & APE_FLAG_ANY_PLACEMENT) == 0u)

typedef float f32x4 __attribute__((ext_vector_type(4)));

// What a kernel that gives up leaves in its model's sticky status word (cluster_sync.h: ape_give_up).  Zero between
// launches; the host tests != 0 only (ape_model_check reports the number and resets), the codes are for whoever reads that report.
enum ApeAbort : unsigned {
    APE_ABORT_SPIN = 1,             // a bounded spin gave up: a peer's flags, granules or XCD word never came -- not all workgroups were resident
    APE_ABORT_TICKET = 2,           // a workgroup drew a ticket outside the grid: the counters are those of an earlier aborted launch
    APE_ABORT_XCD_RENDEZVOUS = 5,   // lstm_mc_small.hip: the members' XCD words never came
    APE_ABORT_BUILDER_ROW = 6,      // lstm_mc_small.hip: the feature builder's row never came
    APE_ABORT_COLLECT = 16,         // lstm_mc_small.hip: + phase -- a peer's values of that phase never came
};

// Kernel arguments of the batch-tile LSTM kernel (passed by value).
struct LstmParams {
    const float* x;                     // [B,T,I]
    float* y;                           // [B,O] or [B,T,O]
    const f32x4* wpack[APE_MAX_LAYERS]; // per layer: MFMA-fragment-ordered [W_ih | W_hh]
    const float* bias[APE_MAX_LAYERS];  // per layer [4H] = b_ih + b_hh
    const float* w_out;                 // [O,H]
    const float* b_out;                 // [O]
    const double* xx_m;                 // [I] (device) or nullptr
    const double* xx_s;                 // [I]
    const float* masks;                 // [L-1,B,T,H] or nullptr
    int B, T, I, O;
    int KX;                             // input width padded to a multiple of 32
    int x_ring;                         // time step t lives in slot (t + x_ring) mod T of a window (0: linear)
    unsigned flags;
    float dropout_p;
    unsigned long long seed;
    size_t x_row_stride;                // floats between the windows of consecutive rows (0: T*I, a dense [B,T,I])
    float* hseq;                        // [B,T,H]: every step's top-layer output goes here too (or nullptr)
    int x_group;                        // wide-input instantiations: row b reads window b / x_group of x, and with
                                        // DROPOUT_PHILOX the input is masked as the output of a layer 0 would be
                                        // (0: row b reads window b, no mask)
    int layer_base;                     // model layer that this launch's layer 0 is (a launch over the UPPER layers of a
                                        // model keeps the model's layer numbers in its Philox counters)
    const float* h0;                    // [L,hs_rows,H] initial hidden state (DropoutLSTM.forward(x, hs), nn_models.py:180-189)
    const float* c0;                    // [L,hs_rows,H] initial cell state; both nullptr: zeros
    int hs_rows;                        // batch size of h0 / c0
    long long row_base;                 // DROPOUT_PHILOX: global index of this launch's row 0 in the caller's batch (a multiple of 4;
                                        // 0 for every caller but a chunked one -- ape_replay -- whose chunks must draw the masks of ONE call)
    float* hout;                        // the HOUT instantiations only: [B,H] the top layer's output of the last step, the vector the head
                                        // multiplies (last, so that the fields the other instantiations read stay where they were)
};

// Kernel arguments of the weight-stationary cluster LSTM kernel.
struct ClusterParams {
    const float* x;                     // [B,T,I]
    float* y;                           // [B,O]
    const float* wcl[APE_MAX_LAYERS];   // per layer [member GH][wave 4][NW_l][lane 64]: B-fragment registers
    const float* bias[APE_MAX_LAYERS];  // per layer [4H] = b_ih + b_hh
    const float* w_out;                 // [O,H]
    const float* b_out;                 // [O]
    const double* xx_m;
    const double* xx_s;
    const double* xx_r;                 // [I] 1 / xx_s, rounded once on the host
    float* hx;                          // exchange slices [cluster][L][parity 2][member GH][wave 4][row MR][4 units] (f32 cluster kernel)
    size_t hx_bytes;
    unsigned* xflags;                   // [cluster][L][GH] epoch flags, zeroed before every launch
    unsigned* ticket;                   // [1] arrival counter (re-zeroed by the last workgroup out)
    unsigned* done;                     // [1] departure counter
    unsigned* status;                   // [1] sticky: an ApeAbort code once a launch gave up
    const float* masks;                 // [L-1,B,T,H] injected dropout masks or nullptr
    int B, T, I, O;
    int x_ring;                         // time step t lives in slot (t + x_ring) mod T of a window (0: linear)
    unsigned flags;
    float dropout_p;
    unsigned long long seed;
    float* hseq;                        // [B,T,H] every step's top-layer output (all-steps mode), or nullptr
    size_t x_row_stride;                // first-generation f32 kernel: floats between consecutive rows of x (0: T * I; a Monte-Carlo bank's ring
                                        // keeps n_mc window slots per stream and layer 0 reads the first of each)
    int row_base;                       // first-generation kernel, Philox dropout: global index of this launch's row 0 in the caller's batch
                                        // (the counters name GLOBAL rows: the samples of a call do not depend on how it is split over launches)
    unsigned long long* dbg_wg;         // diagnostic builds only: 8 words per workgroup (ticket, XCC, clocks)
    unsigned* seq;                      // latency kernel: [1] launch number of this model (the upper bits of its granule tags)
    // latency kernel only: the post-filter in the same launch (ape_infer at B <= 4).  est row b = FK of y row b, de-normalised when
    // fk_yy_m is set; nullptr: no tail
    void* fk_est;                       // [B,W] of fk_est_dtype
    const double* fk_yy_m;
    const double* fk_yy_s;
    double fk_body[9];                  // larm_vec, uarm_vec, uarm_orig_rh
    int fk_layout, fk_W, fk_est_dtype;
    float gate_scale[APE_MAX_LAYERS];   // lstm_cluster32.hip: 2^S of layer l's split weights (its accumulators start at 2^S (b_ih + b_hh))
    float gate_descale[APE_MAX_LAYERS]; //                     2^-S, folded into the gate constants
    unsigned* xcc_slots;                // APE_XCC_WORDS words, zero between launches.  [0,64): small-batch kernel, (0x10 | XCC id) of
                                        // its members; [64,192): fp16 v2 kernel's 8 class tickets, one per 64-byte line;
                                        // [192, ...): its per-workgroup XCD words
};

// Kernel arguments of the weight-stationary upper-layer kernel of the Monte-Carlo stream bank (lstm_upper32.hip): one chunk of
// sample rows, tiles of 32.
struct UpperParams {
    const float* xfrag;                 // [n_tiles][T][k-block 32][window 32][8 units] masked input, MFMA fragment order
    size_t xfrag_bytes;                 // < 4 GiB (one buffer descriptor)
    float* ypart;                       // [n_tiles * 32][member 8][16] head partial sums
    const float* w;                     // [member 8][wave 4][64][lane 64][4]: 256 weight registers per lane ([W_ih | W_hh], wcl32 layout)
    const float* bias;                  // [4H] = b_ih + b_hh
    const float* w_out;                 // [O,H]
    float* hx;                          // exchange slices [cluster][set 2][parity 2][member 8][wave 4][window 32][8 units]
    size_t hx_bytes;
    unsigned* xflags;                   // [cluster][set 2][32] epoch flags, zero between launches
    unsigned* done;                     // [1] departure counter
    unsigned* status;                   // [1] sticky: an ApeAbort code once a launch gave up
    unsigned* xcc_slots;                // as ClusterParams::xcc_slots (class tickets + per-workgroup XCD words)
    unsigned long long* dbg_wg;         // diagnostic builds only
    float* hseq;                        // layer-0 form only: [n_tiles][T][32 KB] every step's slices (fragment order)
    size_t hseq_bytes;
    int T, O, n_tiles;
    unsigned flags;                     // APE_FLAG_IN_XCD_PLAIN / APE_FLAG_ANY_PLACEMENT only
};

// Kernel arguments of the weight-stationary kernel for layers 1 and 2 of the 3 x 128 model in a Monte-Carlo stream bank
// (lstm_upper128.hip): one chunk of sample rows, tiles of 32.
struct Upper128Params {
    const float* xfrag;                 // [n_tiles][T][k-block 16][row 32][8 units]: layer 0's output under the rows' masks, fragment order
    size_t xfrag_bytes;
    const unsigned* maskbits;           // [n_tiles][T][unit 128]: bit n = row n of the tile keeps layer 1's output of that unit and step
    float* ypart;                       // [n_tiles * 32][member 4][16] head partial sums
    const float* w[2];                  // layers 1, 2: [member 4][wave 4][32][lane 64][4] = 128 weight registers per lane each
    const float* bias[2];               // [4H] = b_ih + b_hh
    const float* w_out;                 // [O,H]
    float* hx;                          // exchange [cluster][set 2][kind 3: h_1, h_1 masked, h_2][parity 2][16 KB]
    size_t hx_bytes;
    unsigned* xflags;                   // [cluster][set 2][layer 2][16] epoch flags, zero between launches
    unsigned* done;
    unsigned* status;
    unsigned* xcc_slots;
    int T, O, n_tiles;
    unsigned flags;                     // APE_FLAG_IN_XCD_PLAIN / APE_FLAG_ANY_PLACEMENT only
    float dropout_p;
    unsigned long long* dbg_wg;         // diagnostic build only (APE_CLUSTER_STAMPS): shader-clock sums of cluster 0 / member 0 / wave 0
};

// Kernel arguments of the input builder of the layer-0 launch (ape_x_frag_kernel, lstm_upper32.hip).
struct XFragParams {
    const float* x;                     // window rings: stream s at x + s * x_row_stride, [T][I]
    float* xfrag;                       // [tiles][T][4 KB]
    const double* xx_m;                 // [I] or nullptr (no z-score)
    const double* xx_s;
    size_t x_row_stride;
    int S, T, I, x_ring;
};

// Kernel arguments of the input builder of that launch (ape_mc_expand_kernel, lstm_upper32.hip).
struct ExpandParams {
    const float* hseq;                  // [S,T,H] layer-0 output sequence of every stream (launch A)
    float* xfrag;                       // as UpperParams::xfrag
    long long row_base;                 // global index of this chunk's first sample row (a multiple of 32)
    int rows;                           // sample rows in this chunk
    int T, n_mc;
    int layer;                          // model layer whose output hseq is (Philox counter word)
    float dropout_p;
    unsigned long long seed;
    int hseq_frag;                      // 1: hseq is the layer-0 cluster kernel's [S / 32][T][k-block 32][stream 32][8] (fragment order)
    const float* masks;                 // injected multipliers [L-1, masks_rows, T, H] instead of the Philox draws (test hooks only), or nullptr
    long long masks_rows;               // sample rows of the whole bank (the masks' row stride)
};

#define APE_MAX_FF_LAYERS 8          // input layer + up to 7 hidden layers of the MLP regressor

// Kernel arguments of the MLP (DropoutFF) kernel.
struct MlpParams {
    const float* x;                        // rows at x[n * row_stride + row_offset + k]
    float* y;                              // [N,O]
    const f32x4* wpack[APE_MAX_FF_LAYERS]; // per layer MFMA-fragment-ordered weights
    const float* bias[APE_MAX_FF_LAYERS];  // per layer [H]
    const float* w_out;                    // [O,H]
    const float* b_out;                    // [O]
    const double* xx_m;
    const double* xx_s;
    const float* mask;                     // [N,H] dropout mask in front of the output layer, or nullptr
    float* hidden_out;                     // [N,H]: write the last hidden activation here INSTEAD of the output layer
    float neg_slope;                       // 0.01 leaky_relu (DropoutFF), 0 relu (ImuPoseLSTM's input layer)
    size_t row_stride, row_offset;
    int N, I, O, KX, n_hidden;
    unsigned flags;
    float dropout_p;
    unsigned long long seed;
};

// Kernel arguments of the masked heads of a DropoutFF bank frame / replay (ape_ff_bank_head, ff_bank.hip): `rows` sample rows, global row
// row_base + r = sample (row_base + r) % n_mc of stream / frame (row_base + r) / n_mc, whose hidden row is hidden[that - g_base].
struct FfHeadParams {
    const float* hidden;                // [groups,H] last hidden activation (the trunk, once per stream); row 0 = group g_base
    const float* w_out;                 // [O,H]
    const float* b_out;                 // [O]
    const float* masks;                 // injected multipliers [all rows, H] indexed by the GLOBAL row (test hooks), or nullptr
    float* y;                           // [rows,O] normalised NN targets; row 0 = global row row_base
    long long row_base, g_base;
    int rows, n_mc, H, O;
    float dropout_p;                    // > 0 without masks: Philox draws keyed by `seed`
    unsigned long long seed;
    long long philox_base;              // added to the global row in the Philox counter only (ape_replay_resume's sample_row_base; else 0)
};

struct FkParams {
    const void* preds;   // [N,O] f32 or f64
    void* est;           // [N,W] f32 or f64
    const double* yy_m;  // [O] device, or nullptr (no de-normalisation)
    const double* yy_s;
    double body[9];      // larm_vec, uarm_vec, uarm_orig_rh
    int N, O, W, layout;
};

// ape_replay_bodies: which body a row of an FK launch takes -- sample row row_base + r belongs to frame (row_base + r) / n_mc, that
// frame to recording rec_of[frame], whose nine values are row rec_of[frame] of bodies [R,9]
struct FkBodyRows {
    const double* bodies;
    const int* rec_of;   // [F]
    long long row_base;
    int n_mc;
};

// Kernel arguments of the per-stream smoothing + message kernel (stream bank).
struct StreamPostParams {
    const float* y_new;  // [S,n_mc,O] NN targets of this step (model output, still normalised)
    float* yring;        // [S,smooth,n_mc,O] the last `smooth` predictions (n_mc samples each) of every stream
    void* msg;           // [S,25] of msg_dtype
    void* tail;          // [S,smooth*n_mc,6] of msg_dtype (hand xyz, elbow xyz of every stacked row) or nullptr
    const double* yy_m;  // [O] or nullptr (no de-normalisation)
    const double* yy_s;
    double body[9];
    int S, O, W, layout, smooth;
    int n_mc;            // Monte-Carlo samples per stream and step (1: deterministic bank)
    int pos;             // ring slot of this step's prediction
    int cold;            // 1: first step after a reset -- every slot takes this prediction (estimator.py:114-115)
    int msg_dtype;
    int packed;          // 1: msg rows are [25 + 6*smooth*n_mc] wide and carry the tail behind the message
    const unsigned* status_in;   // host frames: the model's sticky status word ...
    unsigned* status_out;        // ... copied here (pinned host memory) by the step's last kernel, or nullptr
    unsigned* done_out;          // host frames: [S] pinned words; stream s's workgroup writes done_val behind its (system-fenced) outputs,
    unsigned done_val;           // so that the host can take the frame the moment it is there instead of waiting for the stream to drain
    double* part;                // split form (stream_post_device.h): [S][chunks][21] partial sums, or nullptr (one workgroup per stream)
    unsigned* part_cnt;          // ... and [S] arrival tickets, zero between launches
};
// 64-row chunks of a stack of N rows in the split form: rows 0 .. 63, then 63 per chunk (lane 63 repeats row 0)
static inline int ape_stream_post_chunks(int N) { return N <= 64 ? 1 : 1 + (N - 64 + 62) / 63; }

// APE_FLAG_SPREAD forms of the post-filter (stream_post_device.h, SPR): what they need beyond StreamPostParams, as a kernel argument of
// their own -- the struct above and with it the other forms' object code stay what they were
struct SpreadArgs {
    double* part;        // split form: [S][chunks][4 role waves][18] partial spread sums beside p.part, or nullptr
};

// Per-stream smoothing lengths (stream_post_device.h, SMT): what the table forms need beyond StreamPostParams, as a kernel
// argument of their own -- the struct above and the other forms' object code stay what they were
struct SmoothArgs {
    const int* smooths;          // [S] device table, each in [1, p.smooth]; indexed by the stream
    unsigned long long count;    // lockstep frames: predictions since the cold start (subset frames: the descriptors carry the slots)
};

// the form the post-filter's launchers pick for a frame: 0 = wide (lanes = streams), 1 = one workgroup per stream, c > 1 = split over c
// workgroups per stream (have_part: the bank holds the split form's workspaces)
static inline int ape_stream_post_form(const StreamPostParams& p, bool have_part) {
    if (p.smooth == 1 && p.n_mc == 1 && p.S >= 8) return 0;
    const int chunks = ape_stream_post_chunks(p.smooth * p.n_mc);
    return (have_part && chunks > 1) ? chunks : 1;
}

struct MsgParams {
    const double* est;   // [N,W]
    double* msg;         // [25]
    double body[9];
    int N, W, layout;
};

// Offline replay (replay.hip, ape_replay): a chunk of sample rows [r0, r0 + R) of a call over F frames x n_mc samples
struct ReplayWindowParams {
    const float* xx;     // [F,I] features of every frame of the call
    const int* seg_of;   // [F] first frame of each frame's recording
    float* xw;           // [R,T,I] windows of the chunk's sample rows
    long long r0;
    int R, T, I, n_mc;
};
struct ReplayMsgParams {
    const double* est;   // f64 est rows; row `est_base` of the call's sample rows is est[0]
    long long est_base;
    const int* seg_of;   // [F]
    void* out;           // [F, out_stride] of out_dtype: message, then (tail) 6 values per stacked row
    long long out_stride;
    long long f_lo, f_hi;   // frames [f_lo, f_hi) whose stacks are complete in this chunk
    double body[9];
    int W, layout, smooth, n_mc, out_dtype;
};

// Resumable replay (ape_replay_resume): what the CARRY instantiations of the replay kernels read where a window or a stack
// reaches back before its recording's first frame of this call -- the canonical records the recordings came in with
struct ReplayCarryParams {
    const float* state_in;        // [R][words] canonical records
    const double* est_in;         // [R][smooth][n_mc][W] the carried stacks de-normalised and through FK, once per call
    const int* rec_of;            // [F] index of each frame's recording
    const unsigned char* warm;    // [R] APE_STATE_WINDOW_WARM | APE_STATE_STACK_WARM (a clear bit: that part starts cold, as without carry)
    int words;
};
// the recordings' final windows and stacks as canonical records (ape_replay_state_out_kernel)
struct ReplayStateOutParams {
    const float* xx;              // [F,I]
    const float* y;               // [F*n_mc,O] normalised NN targets of the whole call
    const int* starts;            // [R]
    const float* state_in;        // [R][words] or nullptr
    const unsigned char* warm;    // [R] or nullptr
    float* state_out;             // [R][words]
    int R, F, T, I, smooth, n_mc, O, words;
};

// Subset frames of the stream bank (streams_subset.hip, ape_streams_frame_subset): one descriptor per listed stream, built on the host
struct SubsetDesc {
    int stream;          // the bank's stream index
    int slot;            // window-ring slot of this frame's row (rows since the stream's cold start, mod T)
    int cold;            // 1: first row since the cold start -- the row fills all T slots
    int pos;             // smoothing-stack slot of this frame's prediction (predictions since the cold start, mod smooth)
    int pcold;           // 1: first prediction since the cold start -- it fills the whole stack
};
struct SubsetRowsParams {
    const float* rows;   // [K, width] raw rows, row j for desc[j]
    const SubsetDesc* desc;
    float* xring;        // the bank's [S, n_mc, T, I] window rings: only copy 0 of a stream is read and written
    float* xw;           // [K * n_mc, T, I] compact windows, time-ordered, list order, each window n_mc times
    int K, width, kind, big_endian, T, I, n_mc;
};

// Stream state hand-over (stream_state.hip, ape_streams_export / ape_streams_import): one descriptor per listed stream,
// built on the host from the stream's counters
struct StateDesc {
    int stream;          // the bank's stream index
    int wslot;           // window-ring slot of the stream's OLDEST row (rows since the cold start, mod T)
    int sslot;           // smoothing-stack slot of the stream's OLDEST prediction (predictions since the cold start, mod smooth)
    int warm;            // APE_STATE_WINDOW_WARM | APE_STATE_STACK_WARM: a cold part is exported as zeros and not imported
};
struct StateParams {
    float* xring;        // the bank's [S, copies, T, I] window rings: copy 0 of a stream is read / written
    float* yring;        // [S, smooth, n_mc, O]
    float* state;        // [K, words] canonical records, 16-byte aligned
    const StateDesc* desc;
    size_t x_stream_stride;   // floats between the rings of consecutive streams (copies * T * I)
    int K, T, I, smooth, MO /* n_mc * O */, words;
};

// Kernel arguments of the Monte-Carlo latency kernel (lstm_mc_small.hip): n_streams windows x n_mc dropout samples, dealt over the
// 8 XCDs -- cluster c serves stream c / cps, sample rows [part * R, part * R + R) of it (part = c % cps).
struct McSmallParams {
    const float* x;                     // windows: stream s at x + s * x_stream_stride, [T][I]
    size_t x_stream_stride;
    float* y;                           // [rows, O] normalised NN targets of the last step
    const float* w0;                    // layer 0: the latency kernel's H/8-member register image (ape_model::wcls[0])
    const float* w[APE_MAX_LAYERS];     // layers >= 1 (index = layer): [member H/8][wave 4][H/16][lane 64][4], the 4x4x1 MFMA's A fragments
    const float* w16[APE_MAX_LAYERS];   // the same layers as 16 x 16 x 4 fragments (16-row clusters): wave = column tile x K half
    const float* bias[APE_MAX_LAYERS];
    const float* w_out;
    const float* b_out;
    const double* xx_m;
    const double* xx_s;
    const double* xx_r;
    char* gx;                           // granules {value, tag}: [cluster 8][parity 2][pair][16 B]
    unsigned gx_cluster_bytes;
    unsigned* seq;                      // [1] launch number of this kernel on this model (upper bits of the tags)
    unsigned* done;                     // [1] departure counter
    unsigned* status;                   // [1] sticky: an ApeAbort code once a launch gave up
    unsigned* xcc_slots;                // as ClusterParams::xcc_slots: words [192, 448) hold (0x10 | XCC id) of the 8 x 32 workgroups
    const float* masks;                 // injected [L-1, rows, T, H] or nullptr
    int rows;                           // n_streams * n_mc
    int n_mc, n_streams;
    int cps;                            // clusters per stream
    int R;                              // sample rows per cluster (<= 16)
    int T, I, O, x_ring;
    unsigned flags;                     // NORMALIZE_INPUT, DROPOUT_MASKS | DROPOUT_PHILOX, APE_FLAG_ANY_PLACEMENT
    float dropout_p;
    unsigned long long seed;
    unsigned long long* dbg_wg;         // diagnostic builds only
    // ---- the frame's feature builder in the same launch (ape_streams_frame_host, small banks)
    const float* raw_rows;              // [n_streams][raw_width] raw messages, device-visible (pinned host memory will do), or nullptr: the
                                        // windows are complete.  One extra workgroup per stream builds the new row (parse_device.h), hands it
                                        // to the clusters as tagged granules and writes it into the stream's ring for the frames to come
    int raw_width, raw_kind, raw_big_endian;
    int cold;                           // first row after a reset: every step of the window is the new row (estimator.py:96-97)
    float* ring_out;                    // stream 0's first target slot; stream n at + n * ring_stream_stride, copy j at + j * ring_rep_stride
    size_t ring_stream_stride, ring_rep_stride;
    int ring_rep;
    char* xg;                           // feature granules {value, tag}: [n_streams][64] x 8 bytes
};


#ifdef __HIPCC__
// Philox4x32-10 counter-based generator (Salmon et al. 2011) for in-kernel dropout masks.
__device__ __forceinline__ void philox4x32(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                           uint32_t k0, uint32_t k1, uint32_t (&out)[4]) {
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        // (one 32 x 32 -> 64 product per multiplier: a single quarter-rate v_mad_u64_u32 instead of v_mul_hi_u32 + v_mul_lo_u32)
        const uint64_t p0 = (uint64_t)0xD2511F53u * (uint64_t)c0, p1 = (uint64_t)0xCD9E8D57u * (uint64_t)c2;
        const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0;
        const uint32_t hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

#endif

// formats the thread's error string (ape_last_error) and returns `code`; defined in ape_api.hip, where the string lives
int ape_fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
#define APE_TRY(expr)                                                                                     \
    do {                                                                                                  \
        hipError_t _e = (expr);                                                                           \
        if (_e != hipSuccess) return ape_fail(APE_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(_e)); \
    } while (0)

// kalman.hip's model as kalman_bank.hip sees it
struct ape_kalman;
struct ApeKalmanInfo { int E, W, device, has_weights; };
void ape_kalman_info(const ape_kalman* m, ApeKalmanInfo* out);

// launchers implemented in the .hip files --------------------------------------------------
// returns hipSuccess or the launch error; `smem_bytes` out for diagnostics
hipError_t ape_launch_lstm_tile16(int H, int L, const LstmParams& p, hipStream_t stream);
size_t ape_lstm_tile16_smem_bytes(int H, int L, int KX, int O, bool dropout);
hipError_t ape_prepare_lstm_tile16(int H, int L, size_t smem_bytes);
hipError_t ape_prepare_lstm_tile16_wide(size_t smem_bytes);
hipError_t ape_prepare_lstm_tile16_hout(int H, int L, size_t smem_bytes);     // ape_lstm_features' kernel: the narrow body + p.hout
hipError_t ape_launch_lstm_tile16_hout(int H, int L, const LstmParams& p, hipStream_t stream);
hipError_t ape_prepare_lstm_tile16_upper(int H, int L, size_t smem_bytes);   // layers 1.. of a model on their own: <256,1,wide>, <128,2,wide>
bool ape_cluster_supported(int H, int L, int KX);
bool ape_cluster_layer0_supported(int H, int KX);
hipError_t ape_prepare_lstm_cluster(int H, int L, int KX);
hipError_t ape_launch_lstm_cluster(int H, int L, int KX, int nmt, bool dropout, int clusters, const ClusterParams& p,
                                   hipStream_t stream);
hipError_t ape_launch_lstm_cluster_small(int H, int L, int KX, int nr, int uw, const ClusterParams& p, hipStream_t stream);
hipError_t ape_prepare_lstm_cluster_f16(int H, int L, int KX);
hipError_t ape_launch_lstm_cluster_f16(int H, int L, int KX, int nmt, int clusters, const ClusterParams& p, hipStream_t stream);
bool ape_cluster32_supported(int H, int L, int KX);
hipError_t ape_prepare_lstm_cluster32(int H, int L, int KX);
hipError_t ape_launch_lstm_cluster32(int H, int L, int KX, int clusters, const ClusterParams& p, hipStream_t stream);
// second generation for 16-unit members (lstm_cluster16.hip: the 3 x 128 upper-arm model; first-generation register image wcl)
bool ape_cluster16_supported(int H, int L, int KX);
hipError_t ape_prepare_lstm_cluster16(int H, int L, int KX);
hipError_t ape_launch_lstm_cluster16(int H, int L, int KX, int rows, const ClusterParams& p, hipStream_t stream);
// level-synchronous kernel for short windows of the 3 x 128 model (lstm_level16.hip: 32-window clusters of 8 members, ONE
// eight-wave workgroup per CU -- __launch_bounds__(512, 1), 115 KB of LDS; T + L - 1 <= APE_TAG_MAX_PHASES or the launcher refuses)
bool ape_level16_supported(int H, int L, int KX);
int ape_level16_max_clusters(int n_cus);
size_t ape_level16_gx_bytes(int n_cus);
hipError_t ape_prepare_lstm_level16(int H, int L, int KX);
hipError_t ape_launch_lstm_level16(int H, int L, int KX, int rows, const ClusterParams& p, hipStream_t stream);
bool ape_upper32_supported(int H, int L, int O);
size_t ape_upper32_xfrag_bytes(int rows, int T);
size_t ape_upper32_ypart_bytes(int rows);
size_t ape_lower32_xfrag_bytes(int streams, int T);
size_t ape_lower32_hseq_bytes(int streams, int T);
hipError_t ape_launch_lstm_lower32(const UpperParams& p, const XFragParams& xq, int max_clusters, hipStream_t stream);
hipError_t ape_prepare_lstm_upper32();
// ImuPoseLSTM's 2 x 256 LSTM behind its input layer, one layer per launch: z [B * T][256] row-major -> p0.xfrag (fragment order) ->
// layer 0 (every step to p0.hseq) -> layer 1 reading p1.xfrag == p0.hseq -> head partials -> y [B,O]
hipError_t ape_launch_lstm_split32(const float* z, int B, const UpperParams& p0, const UpperParams& p1, const float* b_out, float* y,
                                   int max_clusters, hipStream_t stream);
hipError_t ape_launch_lstm_upper32(const UpperParams& p, const ExpandParams& q, const float* b_out, float* y, int max_clusters,
                                   hipStream_t stream, hipEvent_t ev_begin = nullptr, hipEvent_t ev_end = nullptr);
bool ape_mc_small_supported(int H, int L, int KX);
size_t ape_mc_small_cluster_bytes(int H, int L);
hipError_t ape_prepare_lstm_mc_small(int H, int L, int KX);
hipError_t ape_launch_lstm_mc_small(int H, int L, int KX, const McSmallParams& p, hipStream_t stream);
bool ape_upper128_supported(int H, int L, int O);
size_t ape_upper128_xfrag_bytes(int rows, int T);
size_t ape_upper128_maskbits_bytes(int rows, int T);
size_t ape_upper128_ypart_bytes(int rows);
size_t ape_upper128_hx_bytes(int clusters);
size_t ape_upper128_flag_words(int clusters);
hipError_t ape_prepare_lstm_upper128();
hipError_t ape_launch_lstm_upper128(const Upper128Params& p, const ExpandParams& q, const float* b_out, float* y, int max_clusters,
                                    hipStream_t stream, hipEvent_t ev_begin = nullptr, hipEvent_t ev_end = nullptr);
bool ape_cluster_f16v2_supported(int H, int L, int KX);
hipError_t ape_prepare_lstm_cluster_f16v2(int H, int L, int KX);
hipError_t ape_launch_lstm_cluster_f16v2(int H, int L, int KX, int clusters, const ClusterParams& p, hipStream_t stream, bool duo = false);
hipError_t ape_launch_parse_rows(const float* rows, int N, int width, int kind, void* out, int out_dtype, int I,
                                 size_t out_stride, int rep, size_t rep_stride, int big_endian, hipStream_t stream);
hipError_t ape_launch_ring_write(const float* xx, int N, int I, float* out, size_t out_stride, int rep,
                                 size_t rep_stride, hipStream_t stream);
// bodies: nullptr (every stream p.body) or the bank's device table [S,9] of per-stream body measurements
hipError_t ape_launch_stream_post(const StreamPostParams& p, hipStream_t stream, const double* bodies = nullptr);
// ... with APE_FLAG_SPREAD: p.msg rows are APE_SPREAD_WIDTH columns longer and end in the spread record (the SPR instantiations)
// (form: ape_stream_post_form's answer, which the caller keeps for ape_streams_last_post_form -- what is reported is what was launched)
hipError_t ape_launch_stream_post_spread(const StreamPostParams& p, const SpreadArgs& sp, int form, hipStream_t stream, const double* bodies = nullptr);
// stand-alone: est [N,W] f64 + msg [25] f64 -> spread [APE_SPREAD_WIDTH] f64 (ape_spread_reduce)
hipError_t ape_launch_spread_reduce(const MsgParams& p, const double* msg, double* spread, hipStream_t stream);
hipError_t ape_launch_mlp_tile16(int H, const MlpParams& p, hipStream_t stream, int n_cus = 0);
hipError_t ape_prepare_mlp_tile16(int H);     // per device: dynamic-LDS limits of the MLP and head-rows kernels (from ape_model_create)
// two-stage weight-stationary pipeline for chip-filling eval batches of the 2-hidden-layer MLP (mlp_pipe.hip)
bool ape_mlp_pipe_supported(int H, int n_hidden, int KX, int O);
size_t ape_mlp_pipe_ring_bytes(int n_cus);
size_t ape_mlp_pipe_ctl_words(int n_cus);
hipError_t ape_prepare_mlp_pipe();
hipError_t ape_launch_mlp_pipe(const MlpParams& q, const float* wa0, const float* wa1, const float* wb2, const float* wbo, float* ring,
                               size_t ring_bytes, unsigned* ctl, int n_cus, hipStream_t stream);
hipError_t ape_launch_head_rows(const float* hseq, int N, int H, int O, const float* w_out, const float* b_out, float* y,
                                hipStream_t stream);
hipError_t ape_launch_fk(const FkParams& p, int preds_dtype, int est_dtype, hipStream_t stream, const FkBodyRows* bodies = nullptr);
hipError_t ape_launch_msg_reduce(const MsgParams& p, hipStream_t stream);
// rec_of (optional): [F] index of each frame's recording, for the replays with one body per recording
hipError_t ape_launch_replay_segments(const int* starts, int n_starts, int F, int* seg_of, hipStream_t stream, int* rec_of = nullptr);
// carry: nullptr (every recording starts cold: the instantiations ape_replay always ran) or the carried-in state
hipError_t ape_launch_replay_windows(const ReplayWindowParams& p, hipStream_t stream, const ReplayCarryParams* carry = nullptr);
// bodies / rec_of: nullptr (p.body for every frame) or [R,9] values and [F] recording indices
hipError_t ape_launch_replay_msg(const ReplayMsgParams& p, bool tail, hipStream_t stream, const double* bodies = nullptr,
                                 const int* rec_of = nullptr, const ReplayCarryParams* carry = nullptr, bool spread = false);
// the stacks of R records -> contiguous rows [R * smooth * n_mc, O] (the input of the carried rows' FK launch)
hipError_t ape_launch_replay_carry_rows(const float* state_in, int R, int words, int x_words, int stack_words, float* y_in, hipStream_t stream);
hipError_t ape_launch_replay_state_out(const ReplayStateOutParams& p, hipStream_t stream);
hipError_t ape_launch_subset_rows(const SubsetRowsParams& p, hipStream_t stream);
hipError_t ape_launch_subset_rows_host(const SubsetRowsParams& p, SubsetDesc* land, hipStream_t stream);
// ring order <-> the canonical time-ordered records of the listed streams, one launch each (stream_state.hip)
hipError_t ape_launch_state_export(const StateParams& p, hipStream_t stream);
hipError_t ape_launch_state_import(const StateParams& p, hipStream_t stream);
hipError_t ape_launch_state_smooths(const StateParams& p, const int* smooths, bool import, hipStream_t stream);
// DropoutFF / ImuPoseLSTM banks (ff_bank.hip): the n_mc masked heads over a trunk computed once per stream; the time-ordered copy of the
// window rings [S][T][I] (step t in slot (t + x_ring) mod T)
hipError_t ape_launch_ff_bank_head(const FfHeadParams& p, hipStream_t stream);
hipError_t ape_launch_ring_windows(const float* xring, float* xw, int S, int T, int I, int x_ring, hipStream_t stream);
// the bank's post-filter over a list: p.S = K entries, y_new / msg in list order, stack slot and cold flag of entry j from desc[j]
// (bodies: as ape_launch_stream_post -- indexed by desc[j].stream)
hipError_t ape_launch_stream_post_subset(const StreamPostParams& p, const SubsetDesc* desc, hipStream_t stream, const double* bodies = nullptr);
hipError_t ape_launch_stream_post_subset_spread(const StreamPostParams& p, const SubsetDesc* desc, const SpreadArgs& sp, int form, hipStream_t stream,
                                                const double* bodies = nullptr);
// ... of a bank with per-stream smoothing lengths (stream_post_device.h, SMT): form = 1 or the split's chunk count, sp = nullptr without
// APE_FLAG_SPREAD, bodies = the bank's table or nullptr (p.body); the subset form reads sm.smooths[desc[j].stream]
hipError_t ape_launch_stream_post_smooths(const StreamPostParams& p, const SmoothArgs& sm, const SpreadArgs* sp, int form, hipStream_t stream,
                                          const double* bodies = nullptr);
hipError_t ape_launch_stream_post_subset_smooths(const StreamPostParams& p, const SubsetDesc* desc, const SmoothArgs& sm, const SpreadArgs* sp, int form,
                                                 hipStream_t stream, const double* bodies = nullptr);
