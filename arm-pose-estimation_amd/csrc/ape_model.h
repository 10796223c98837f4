// The model and stream-bank handles behind the C ABI: shared by the host files (ape_api.hip, api_*.hip) and by the test-hooks translation unit
// (ape_debug.hip, linked into lib/diag/libape_hip_testhooks.so only).
#pragma once
#include <string>
#include <vector>

#include "../../include/ape_hip.h"
#include "ape_internal.h"
#include "ape_plan.h"
#include "body_table.h"
#include "smooth_table.h"
#include "bank_host.h"

struct ape_streams;

// One compute call on a model since its last successful check, kept so that ape_model_recover can re-issue it on the
// kernels that need no co-residency when a weight-stationary launch gave up (include/ape_hip.h, "Aborted launches").
struct ApeJournalEntry {
    enum Kind { FORWARD, FORWARD_HS, FK, MSG, INFER, STEP, SUBSET, FEATURES } kind;
    const void* in0;                 // x / preds / est
    const void* in1;                 // masks / h0
    const void* in2;                 // c0
    void* out0;                      // y / est / msg / h (features)
    void* out1;                      // est (infer) / tail (step) / y (features)
    int32_t B, T, i0, i1, i2;        // sizes and dtype selectors
    uint32_t flags;
    float dropout_p;
    uint64_t seed;
    void* stream;
    ape_streams* bank;               // STEP / SUBSET: the bank and its counters in front of the step (SUBSET: B = list length)
    long long bank_frames, bank_steps;
    unsigned long long bank_mc_calls;
};
#define APE_JOURNAL_CAP 64

struct ape_model {
    ape_dims_t dims{};
    void* slab = nullptr;          // the one device allocation every fixed-size buffer below points into
    size_t slab_bytes = 0;
    int n_cus = 0;                 // hipDeviceProp_t::multiProcessorCount of the model's device (256 on a whole MI355X)
    ApeCaps caps;                  // what this model can run there (ape_plan.h): ape_caps(dims, n_cus) minus what failed to set up
    int KX = 0;                    // LSTM layer-0 input width, padded to the kernels' k-blocking
    int lstm_in = 0;               // LSTM layer-0 input width (input_size; 256 behind ImuPoseLSTM's input layer)
    int KXpre = 0;                 // ImuPoseLSTM: padded width of the input layer's input
    float* z_ws = nullptr;         // ImuPoseLSTM: [cap rows, 256] activations of the input layer
    float* hseq_ws = nullptr;      // all-steps mode of the cluster kernel: [cap rows = B*T, H] top-layer outputs
    size_t hseq_cap = 0;
    size_t z_cap = 0;
    f32x4* wpack[APE_MAX_LAYERS] = {nullptr, nullptr, nullptr};
    float* bias[APE_MAX_LAYERS] = {nullptr, nullptr, nullptr};
    float* w_out = nullptr;
    float* b_out = nullptr;
    double* stats = nullptr;       // device: xx_m[I] xx_s[I] yy_m[O] yy_s[O] 1/xx_s[I]
    bool has_weights = false, has_stats = false;
    double body[9];
    float* y_ws = nullptr;         // [cap, O] intermediate of ape_infer
    int y_cap = 0;
    // weight-stationary cluster kernel (lstm_cluster.hip)
    int kernel_choice = APE_KERNEL_AUTO;
    float* wcl[APE_MAX_LAYERS] = {nullptr, nullptr, nullptr};
    void* wcl16[APE_MAX_LAYERS] = {nullptr, nullptr, nullptr};   // binary16 fragments of the fp16 variant
    float* wcl32[APE_MAX_LAYERS] = {nullptr, nullptr, nullptr};  // 32x32x2 fragments of the second-generation f32 cluster kernel
    unsigned* wcl32s[APE_MAX_LAYERS] = {nullptr, nullptr, nullptr};  // ... the same image with the recurrent columns as f16 hi / lo (lstm_cluster32.hip)
    float c32_scale[APE_MAX_LAYERS] = {1.0f, 1.0f, 1.0f};          // ... 2^S per layer (pack_c32_split)
    float c32_descale[APE_MAX_LAYERS] = {1.0f, 1.0f, 1.0f};
    float* wcls[APE_MAX_LAYERS] = {nullptr, nullptr, nullptr};   // the latency kernel's H/8-member form (two units per wave)
    char* hxs = nullptr;             // latency kernel: [256 B: launch number][granules {h, tag}: layer, parity, 4 rows, H units]
    size_t hxs_bytes = 0;
    float* wmc[APE_MAX_LAYERS] = {nullptr, nullptr, nullptr};    // Monte-Carlo latency kernel: layers >= 1, wave = K quarter (4x4x1 MFMA fragments)
    float* wmc16[APE_MAX_LAYERS] = {nullptr, nullptr, nullptr};  // ... and as 16 x 16 x 4 fragments (16-row clusters: wave = column tile x K half)
    char* gxm = nullptr;             // ... [256 B: launch number][8 clusters of granules]
    size_t gxm_cluster_bytes = 0;
    int small_uw = 4;                // hidden units per wave of the latency kernel: 2 when one XCD holds H/8 members
    bool c32_on = true;             // ... and is not switched off (APE_KERNEL_CLUSTER_GEN1)
    bool gen1_classes = true;       // first-generation f32 kernel: XCD-class cluster formation where the grid allows it
    char* gx16 = nullptr;           // lstm_level16.hip: [256 B: launch number][granules {h, tag}: cluster, row tile, parity, layer]
    size_t gx16_bytes = 0;
    int precision = APE_PRECISION_F32;
    bool small_batch_path = true;   // B <= 4 on the VALU/shuffle variant of the cluster kernel
    bool f16_v2 = true;             // fp16 precision: batches > 256 rows on the row-set-pipelined kernel (lstm_cluster_f16v2.hip)
    float* zfrag_ws = nullptr;      // ImuPoseLSTM on lstm_upper32.hip (caps.split32), its workspaces: the input layer's activations in fragment order [tiles][T][32 KB],
    float* hfrag_ws = nullptr;      //     layer 0's output sequence (same shape, layer 1's input),
    float* ypart_ws = nullptr;      //     head partial sums [tiles * 32][8][16]
    size_t split_tiles_cap = 0, split_steps_cap = 0;      // tiles x steps the first two hold
    float* wup128[APE_MAX_LAYERS] = {nullptr, nullptr, nullptr};   // its register image of layers 1, 2
    float* hx = nullptr;           // exchange slices
    size_t hx_bytes = 0;
    unsigned long long* dbg_wg = nullptr;   // 256 x 8 words, written by diagnostic builds of the cluster kernel only
    unsigned* xcc_slots = nullptr; // small-batch kernel: 64 words its members publish their XCD in (zero between launches)
    unsigned* xflags = nullptr;    // [flag words..., status word]
    size_t xflag_bytes = 0;        // bytes of the flag block (multiple of 16), status word follows
    // MLP regressor (APE_MODEL_FF)
    float *ffp_wa0 = nullptr, *ffp_wa1 = nullptr, *ffp_wb2 = nullptr, *ffp_wbo = nullptr;   // mlp_pipe.hip: the two stages' register files
    float* ffp_ring = nullptr;       // ... its ring of tiles between the stages
    size_t ffp_ring_bytes = 0;
    unsigned* ffp_ctl = nullptr;     // ... class tickets, status, departure counter, per-pair full / empty words (zero between launches)
    size_t ffp_ctl_words = 0;
    bool ffp_ok = false, ffp_on = true;
    f32x4* ff_wpack[APE_MAX_FF_LAYERS] = {};
    float* ff_bias[APE_MAX_FF_LAYERS] = {};
    std::string kernel_name, cluster_name;
    const char* last_kernel = "";   // the regressor kernel (LSTM or MLP) the newest compute call launched last (ape_model_last_kernel)
    // calls since the last successful check (ape_model_recover replays them), and what became of aborted launches
    ApeJournalEntry journal[APE_JOURNAL_CAP];
    int journal_n = 0;
    bool journal_overflow = false;
    bool replaying = false;         // ape_model_recover is re-issuing: no journaling, no cooperative kernel
    ape_model_stats_t stats_counts{};
};

// the control words behind the flag block: the only place that knows where they sit
struct CtlWords { unsigned *status, *ticket, *done; };
inline CtlWords ctl_words(const ape_model* m) {
    unsigned* status = m->xflags + m->xflag_bytes / sizeof(unsigned);
    return {status, status - 4, status - 3};
}

struct ape_streams {
    ape_model* model = nullptr;
    int S = 0, T = 0, smooth = 0;
    int n_mc = 1;                // Monte-Carlo samples per stream and step
    bool mc = false;             // dropout on (ape_streams_set_mc was called)
    float dropout_p = 0.0f;
    unsigned long long seed = 0, mc_calls = 0;
    float* xring = nullptr;      // [S,n_mc,T,I] feature rows, slot = frame mod T (a stream's n_mc windows are copies)
    float* yring = nullptr;      // [S,smooth,n_mc,O] model outputs, slot = step mod smooth
    float* y_new = nullptr;      // [S,n_mc,O]
    double* post_part = nullptr; // split post-filter (stream_post_device.h): [S][chunks][21] partial sums + [S] tickets behind them, or
    unsigned* post_cnt = nullptr; //   nullptr where every stream keeps a workgroup of its own (many streams, or stacks of <= 64 rows)
    int last_post_form = -1;     // ape_streams_last_post_form: -1 no frame yet, 0 wide, 1 one workgroup per stream, c > 1 split over c
    double* post_spread = nullptr; // ... and, in the same allocation, [S][chunks][72] partial spread sums (APE_FLAG_SPREAD frames)
    // what ape_streams_set_mc planned (ape_plan.h) -- the weight-stationary routes (lstm_upper32.hip / lstm_upper128.hip) only once their
    // workspaces below exist: the sample rows go through them in chunks of plan.chunk_rows (a multiple of 32), each expand -> LSTM -> head reduce
    BankPlan plan;
    unsigned* maskbits = nullptr;   // ... keep bits of layer 1's outputs [chunk tiles][T][128]
    float* xfrag = nullptr;      // [chunk tiles][T][32 KB] masked layer-0 output in MFMA fragment order
    float* ypart = nullptr;      // [chunk rows][8][16] head partial sums
    float* xfrag0 = nullptr;     // [S / 32][T][4 KB] layer 0's input tiles, fragment order
    float* hfrag = nullptr;      // [S / 32][T][32 KB] layer 0's output sequence, fragment order (launch B's input builder reads it)
    // DropoutFF / ImuPoseLSTM banks (ff_bank.hip).  A DropoutFF bank keeps T = 1 whatever seq_len it was created with: the
    // reference's [:, -1, :] leaves the newest row as the only one that counts; both kinds keep ONE window per stream (xring [S,T,I])
    float* ffhid = nullptr;      // DropoutFF: [S,H] the trunk's last hidden activation, once per stream and frame
    float* xwin = nullptr;       // ImuPoseLSTM: [S,T,I] the windows of a lockstep frame in time order
    bool prof_on = false;        // ape_streams_profile: event pairs around the dominant kernel's launches
    int prof_n = 0;
    std::vector<hipEvent_t> prof_ev;
    const float* inj_masks = nullptr;   // test hooks only (ape_debug_set_bank_masks): injected multipliers [L-1, S*n_mc, T, H] instead of Philox
    long long frames = 0;        // rows pushed since the last reset
    long long steps = 0;         // predictions made since the last reset
    // host frames (ape_streams_frame_host): pinned, device-visible staging the kernels read the raw rows from and write the
    // datagram rows (+ the model's status word) to -- no copy command in the frame, one stream synchronisation
    float* h_rows = nullptr;     // [S, 55|28]
    void* h_out = nullptr;       // [S, 25 + 6 * smooth * n_mc] of the frame's dtype
    unsigned* h_status = nullptr;
    unsigned* h_done = nullptr;  // [64] pinned: the post kernel's per-stream "outputs are there" words of a host frame
    unsigned h_done_val = 0;     // ... and the value this frame's are awaited with
    size_t h_rows_bytes = 0, h_out_bytes = 0;
    // where a host frame's time goes (ape_streams_frame_stats): a ring of the last 4096 frames' {launch, wait, copy} microseconds
    std::vector<float> fs_trace;
    uint64_t fs_frames = 0, fs_fallback = 0, fs_recovered = 0;
    // subset frames (ape_streams_frame_subset): per-stream mode and its per-stream counters
    bool per_stream = false;     // set by the first subset call; ape_streams_reset / set_mc return the bank to lockstep
    std::vector<long long> s_frames, s_steps;   // [S] rows / predictions since each stream's cold start
    float* sub_x = nullptr;      // [S * n_mc, T, I] compact windows of the newest subset frame (lazily, sized for K = S)
    float* sub_y = nullptr;      // [S * n_mc, O] its targets
    SubsetDesc* sub_desc = nullptr;   // [S] its descriptors on the device
    int sub_n_mc = 0;            // n_mc the three were sized for
    // host staging of the descriptors: a ring of pinned slots, each reused only once the copy out of it has completed
    ApeDescStage sub_stage;      // slots of S SubsetDesc (bank_host.h)
    // host subset frames (ape_streams_frame_subset_host): ONE pinned, device-visible block the host writes and launch 1 reads --
    // [64] completion words the post kernel writes, [S] descriptors, [S, 57] raw rows; reused every frame (the call is blocking)
    char* hs_block = nullptr;
    unsigned hs_done_val = 0;    // the value this frame's completion words are awaited with
    // state hand-over (ape_streams_export / import): descriptors of their own on the device -- sub_desc belongs to the
    // newest subset frame, which ape_model_recover may still re-issue; staged through the pinned ring above
    StateDesc* state_desc = nullptr;  // [S]
    // per-stream body measurements (ape_streams_set_bodies): off until the first call -- the frames then read model->body
    ApeBodyTable bodies;         // [S,9] on the device
    // per-stream smoothing lengths (ape_streams_set_smooths): off until the first call -- `smooth` is then the capacity
    ApeSmoothTable smooths;      // [S] on the device
};
