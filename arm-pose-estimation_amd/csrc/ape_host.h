// What the host files of the C ABI share (ape_api.hip and api_*.hip; no device code in any of them): the functions that cross from one
// file to another and the small structs they pass.  Everything here stays inside the library (hidden visibility).  The public entries
// are declared extern "C" by include/ape_hip.h, so their definitions in the api_*.hip files need no linkage block.
//   ape_api.hip      error string, dims check, ape_caps, model create / destroy / setters, journal, check / recover / stats
//   api_weights.hip  ape_model_load_weights over the packers of weight_pack.h
//   api_forward.hip  the LSTM / MLP dispatch (lstm_forward_impl, ff_bank_forward) and the forward, fk, reduce, parse, infer entries
//   api_streams.hip  the NN stream bank: lifecycle, pushes, the lockstep step and host frame, statistics
//   api_subset.hip   subset frames (device and host) and the state hand-over
//   api_replay.hip   offline replay and the journal's re-issue
//   api_debug.hip    the ape_debug_* entries of the product library
#pragma once
#include <algorithm>
#include <chrono>

#include "../../include/ape_hip.h"
#include "ape_internal.h"
#include "ape_model.h"

#pragma GCC visibility push(hidden)

// ---- ape_api.hip ------------------------------------------------------------------------------------------------------------------------
inline int layout_est_width(int layout) { return layout == APE_LAYOUT_ORI_CAL_LARM_UARM ? 14 : 21; }
// columns of a raw row of `kind` and the features the builder makes of it
inline bool parse_kind_dims(int kind, int* width, int* I) {
    switch (kind) {
        case APE_PARSE_WATCH_PHONE_POCKET: *width = 55; *I = 22; return true;
        case APE_PARSE_WATCH_ONLY: *width = 28; *I = 20; return true;
        case APE_PARSE_WATCH_ONLY_PHONE_MSG: *width = 55; *I = 20; return true;
        case APE_PARSE_WATCH_PHONE_UARM: *width = 55; *I = 38; return true;
    }
    return false;
}
// What a model of `dims` can run on a device with n_cus CUs (the kernels' own predicates); the routing on top of it is csrc/ape_plan.h
ApeCaps ape_caps(const ape_dims_t* dims, int n_cus);
// the blocking part ape_model_check, ape_model_recover and the replay share: 0 = no aborted launch since the last check; else the
// handle has been reset and the thread's error string describes what happened
int check_and_reset(ape_model_t* m);
// every successfully enqueued compute call of a handle is remembered until its next successful check (ape_model_recover)
inline void journal_add(ape_model* m, const ApeJournalEntry& e) {
    if (!m || m->replaying) return;
    if (m->journal_n < APE_JOURNAL_CAP) m->journal[m->journal_n++] = e;
    else m->journal_overflow = true;
}
inline void journal_clear(ape_model* m) { m->journal_n = 0; m->journal_overflow = false; }

// plan_bank's `l0_bytes`: the larger of launch A's two buffers on lstm_upper32.hip
inline unsigned long long bank_l0_bytes(int S, int T) { return std::max(ape_lower32_hseq_bytes(S, T), ape_lower32_xfrag_bytes(S, T)); }

// ---- api_forward.hip ----------------------------------------------------------------------------------------------------------------------
// the post-filter ape_infer wants behind the regressor: the latency kernel runs it in its own launch (done = true), every other
// kernel leaves it to the caller
struct FkTail {
    void* est;
    int est_dtype;
    bool denormalize;
    bool done;
};
// what a host frame adds to the regressor's launch: the raw rows of the frame (feature builder workgroups)
struct McFrameParts {
    const float* raw_rows = nullptr;
    int raw_width = 0, raw_kind = 0, raw_big_endian = 0, cold = 0;
    float* ring_out = nullptr;
    size_t ring_stream_stride = 0, ring_rep_stride = 0;
    int ring_rep = 0;
};
// head and input statistics, as every kernel's parameter block names them
template <typename P>
inline void head_and_stats(const ape_model* m, P* p) { p->w_out = m->w_out; p->b_out = m->b_out; p->xx_m = m->stats; p->xx_s = m->stats + m->dims.input_size; }
// may a first-generation launch form XCD-local clusters?  (APE_FLAG_NO_XCD_CLASSES: selector, A/B on one box)
inline bool xcd_classes_on(const ape_model* m, uint32_t flags) { return m->gen1_classes && !(flags & APE_FLAG_NO_XCD_CLASSES); }
// the call's switches as the planner reads them
LstmCall lstm_call(const ape_model* m, int B, int T, uint32_t flags, bool have_hs, int x_ring);
// the fields every launch of a cluster kernel shares, with `layers` of the weight image of `route` (PLAN_* of ape_plan.h)
ClusterParams cluster_params(const ape_model* m, int route, int layers, const float* x, float* y, int B, int T, uint32_t flags, int x_ring);
// ... and of the persistent upper-layer clusters (lstm_upper32.hip, lstm_upper128.hip); the caller adds the layers' weights and buffers
template <typename U = UpperParams>
inline U upper_params(const ape_model* m, int T, int tiles, uint32_t flags) {
    U u{};
    u.w_out = m->w_out;
    u.hx = m->hx; u.hx_bytes = m->hx_bytes;
    u.xflags = m->xflags; u.status = ctl_words(m).status; u.done = ctl_words(m).done;
    u.xcc_slots = m->xcc_slots; u.dbg_wg = m->dbg_wg;
    u.T = T; u.O = m->dims.output_size; u.n_tiles = tiles; u.flags = flags;
    return u;
}
// Monte-Carlo latency kernel (lstm_mc_small.hip): n_streams windows (stream s at x + s * x_stream_stride) x n_mc dropout samples each,
// rows dealt over the 8 XCD clusters; y [n_streams * n_mc, O].  The caller has checked mc_small_fits().
int mc_small_launch(ape_model_t* m, const float* x, size_t x_stream_stride, int n_streams, int n_mc, int T, uint32_t flags,
                    const float* masks_dev, float dropout_p, uint64_t seed, float* y_dev, void* stream, int x_ring,
                    const McFrameParts* fr = nullptr);
// x_ring: time step t of every window lives in slot (t + x_ring) mod T (0 = the linear layout of the public entry)
// row_base (DROPOUT_PHILOX, a multiple of 16): the global row of x_dev's row 0 when a caller serves one batch in several calls
int lstm_forward_impl(ape_model_t* m, const float* x_dev, int32_t B, int32_t T, uint32_t flags, const float* masks_dev, float dropout_p,
                      uint64_t seed, float* y_dev, void* stream, int x_ring, const float* h0_dev = nullptr, const float* c0_dev = nullptr,
                      FkTail* fk = nullptr, long long row_base = 0);
// ape_lstm_features without its journal entry: h^{L-1}_{T-1} [B,H] and (y_dev != NULL) the head's y [B,O], every row on ape_lstm_tile16<H, L, 4, true>
int lstm_features_impl(ape_model_t* m, const float* x_dev, int32_t B, int32_t T, uint32_t flags, const float* masks_dev, float dropout_p,
                       uint64_t seed, float* h_dev, float* y_dev, void* stream);
// the regressor of a DropoutFF frame or replay chunk (ff_bank.hip)
int ff_bank_forward(ape_model* m, const float* x, size_t x_stride, long long row_base, int rows, int n_mc, bool norm, const float* masks,
                    float dropout_p, uint64_t seed, float* hid, float* y, void* stream, hipEvent_t ev_a = nullptr, hipEvent_t ev_z = nullptr,
                    long long philox_base = 0);
int fk_impl(ape_model_t* m, const void* preds_dev, int32_t preds_dtype, int32_t N, int32_t denormalize, void* est_dev, int32_t est_dtype,
            void* stream, const FkBodyRows* bodies = nullptr);

// ---- api_streams.hip ------------------------------------------------------------------------------------------------------------------------
// window copies a stream keeps in the feature ring: n_mc for the LSTM banks ([S,n_mc,T,I], one window per sample row of the fused dropout
// kernels), one for DropoutFF (the trunk runs once per stream) and ImuPoseLSTM (one row per stream)
inline int bank_copies(const ape_streams* b) { return b->model->dims.model_kind == APE_MODEL_LSTM ? b->n_mc : 1; }
// per-stream smoothing lengths
// (a capacity of one row holds nothing but ones: such a bank keeps its table and goes on running the forms it ran)
inline bool bank_smooths_on(const ape_streams* b) { return b->smooths.on() && b->smooth > 1; }
inline int bank_smooth_of(const ape_streams* b, int s) { return bank_smooths_on(b) ? b->smooths.host[(size_t)s] : b->smooth; }

// Where a host frame's status and completion words go: the pinned words the post-filter writes behind its rows -- the model's status
// word, a completion word per stream / list entry -- and the entry's name for ape_last_error.  All null: a device frame.
struct HostFrameWords { unsigned* status_out = nullptr; unsigned* done_out = nullptr; unsigned done_val = 0; const char* what = "streams_frame_subset"; };
// the post-filter's parameters for `rows` streams (or list entries) of the bank with targets y_new; pos, cold and tail stay zero for the
// caller (the lockstep step sets them, a subset frame's descriptors carry them)
StreamPostParams bank_post_params(const ape_streams* b, const float* y_new, int rows, bool norm, void* msg, int out_dtype, bool packed,
                                  const HostFrameWords& hw);
int streams_step_impl(ape_streams_t* b, uint32_t flags, void* msg_dev, void* tail_dev, int32_t out_dtype, void* stream,
                      const HostFrameWords& hw = HostFrameWords{}, const McFrameParts* fuse = nullptr);

// The tail both host frames share, in two halves.  host_frame_wait: watches the `n` completion words (none: done == nullptr), else waits
// for the stream; reads the status word and, where the launch aborted, waits for the stream again.  Between the halves the caller may
// re-issue what the aborted launch should have done in front of the regressor.  host_frame_finish: ape_model_recover or journal_clear,
// the rows to out_host, the trace ring and the three counters.
struct HostFrameTail { double t_begin = 0.0, t_launched = 0.0; bool fell_through = false, aborted = false; };
inline double now_us() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
int host_frame_wait(ape_streams* b, hipStream_t st, const unsigned* done, int n, unsigned done_val, HostFrameTail* t);
int host_frame_finish(ape_streams* b, const HostFrameTail& t, void* out_host, size_t out_bytes);

// ---- api_subset.hip ---------------------------------------------------------------------------------------------------------------------------
// frees the subset frames' device workspaces; a pending subset frame of the bank can no longer be re-issued
void subset_free(ape_streams* b);
// launches 2 and 3 of a subset frame over the compact windows and descriptors in the bank's workspace (also the journal's re-issue)
int subset_regress_post(ape_streams* b, int K, uint32_t flags, void* out_dev, int out_dtype, void* stream, unsigned long long mc_call,
                        const HostFrameWords& hw = HostFrameWords{});

// ---- api_replay.hip ---------------------------------------------------------------------------------------------------------------------------
// one journaled call again, on the kernels that need no co-residency (m->replaying is set)
int replay_entry(ape_model_t* m, const ApeJournalEntry& e);

#pragma GCC visibility pop
