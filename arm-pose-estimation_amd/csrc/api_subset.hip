// Subset frames of the NN stream bank, device and host, and the state hand-over (4.26).
#include <cstring>

#include "ape_host.h"

// ---- subset frames: per-stream rows, slots and cold starts -----------------------------------------------------------
// A frame names K distinct streams with one raw row each; every listed stream does what one Estimator.process_row does, the others stay
// untouched.  Three launches: rows -> rings + compact windows (streams_subset.hip), the regressor over the K * n_mc compact rows
// (lstm_forward_impl, x_ring = 0: every route applies), the indexed post-filter.  Window slot, stack slot and cold flags come from
// per-stream counters on the host (per-stream mode), sent as one descriptor per entry.

// the pinned descriptor ring of the subset frames and the state hand-over, on first use
static int subset_stage_alloc(ape_streams* b) {
    if (!b->sub_stage.on()) APE_TRY(b->sub_stage.alloc(b->S, sizeof(SubsetDesc)));
    return APE_OK;
}

// the first subset call: per-stream counters seeded from the lockstep ones, so that a lockstep history carries on
static void subset_enter(ape_streams* b) {
    if (b->per_stream) return;
    b->s_frames.assign((size_t)b->S, b->frames);
    b->s_steps.assign((size_t)b->S, b->steps);
    b->per_stream = true;
}

int ape_streams_reset_subset(ape_streams_t* b, const int32_t* streams_host, int32_t K) {
    if (!b || !streams_host) return ape_fail(APE_ERR_INVALID_ARG, "streams_reset_subset: NULL argument");
    if (int rc = ape_check_stream_list("streams_reset_subset", streams_host, K, b->S, false)) return rc;
    if (K == 0) return APE_OK;
    subset_enter(b);
    for (int j = 0; j < K; ++j) { b->s_frames[streams_host[j]] = 0; b->s_steps[streams_host[j]] = 0; }
    return APE_OK;
}

// the subset frames' device workspaces (sized for the bank's S and n_mc); a pending subset frame of the bank can no longer be re-issued
void subset_free(ape_streams* b) {
    if (b->sub_x) (void)hipFree(b->sub_x);
    if (b->sub_y) (void)hipFree(b->sub_y);
    if (b->sub_desc) (void)hipFree(b->sub_desc);
    b->sub_x = b->sub_y = nullptr; b->sub_desc = nullptr; b->sub_n_mc = 0;
    if (ape_model* m = b->model) {
        int k = 0;
        for (int i = 0; i < m->journal_n; ++i) {
            if (m->journal[i].kind == ApeJournalEntry::SUBSET && m->journal[i].bank == b) { m->journal_overflow = true; continue; }
            m->journal[k++] = m->journal[i];
        }
        m->journal_n = k;
    }
}

// launches 2 and 3 of a subset frame over the compact windows and descriptors in the bank's workspace (also the journal's re-issue)
int subset_regress_post(ape_streams* b, int K, uint32_t flags, void* out_dev, int out_dtype, void* stream, unsigned long long mc_call,
                        const HostFrameWords& hw) {
    ape_model* m = b->model;
    const bool norm = (flags & APE_FLAG_NORMALIZE_INPUT) != 0;
    const bool packed = (flags & APE_FLAG_PACKED_MSG) != 0 && b->smooth * b->n_mc > 1;
    const bool drop = b->mc && b->dropout_p > 0.0f && m->dims.num_layers > 1 && m->dims.model_kind == APE_MODEL_LSTM;
    if (m->dims.model_kind == APE_MODEL_FF) {
        // (the compact "windows" of a DropoutFF bank are the K newest rows [K,I]; masks keyed by list position)
        if (int rc = ff_bank_forward(m, b->sub_x, (size_t)m->dims.input_size, 0, K * b->n_mc, b->n_mc, norm, nullptr, b->mc ? b->dropout_p : 0.0f,
                                     b->seed + mc_call, b->ffhid, b->sub_y, stream))
            return rc;
    } else if (int rc = lstm_forward_impl(m, b->sub_x, K * b->n_mc, b->T, (norm ? APE_FLAG_NORMALIZE_INPUT : 0u) | (drop ? APE_FLAG_DROPOUT_PHILOX : 0u),
                                   nullptr, drop ? b->dropout_p : 0.0f, b->seed + mc_call, b->sub_y, stream, 0))
        return rc;
    // (pos, cold and tail stay zero: the descriptors carry every entry's stack slot)
    const StreamPostParams q = bank_post_params(b, b->sub_y, K, norm, out_dev, out_dtype, packed, hw);
    b->last_post_form = ape_stream_post_form(q, q.part != nullptr && (!(flags & APE_FLAG_SPREAD) || b->post_spread != nullptr));
    const SpreadArgs spa{b->post_spread};
    hipError_t e = bank_smooths_on(b)
                       ? ape_launch_stream_post_subset_smooths(q, b->sub_desc, SmoothArgs{b->smooths.dev, 0ull}, (flags & APE_FLAG_SPREAD) ? &spa : nullptr,
                                                               b->last_post_form, (hipStream_t)stream, b->bodies.dev)
                   : (flags & APE_FLAG_SPREAD)
                       ? ape_launch_stream_post_subset_spread(q, b->sub_desc, SpreadArgs{b->post_spread}, b->last_post_form, (hipStream_t)stream,
                                                              b->bodies.dev)
                       : ape_launch_stream_post_subset(q, b->sub_desc, (hipStream_t)stream, b->bodies.dev);
    if (e != hipSuccess) return ape_fail(APE_ERR_HIP, "%s: post-filter launch failed: %s", hw.what, hipGetErrorString(e));
    return APE_OK;
}

// what both subset entries check before anything is launched or counted; `what` names the entry
static int subset_frame_check(ape_streams* b, int32_t kind, const void* rows, const int32_t* streams_host, int32_t K, uint32_t flags, const void* out,
                              int32_t out_dtype, void* stream, const char* what, int* width_out, int* I_out) {
    if (!b || !rows || !streams_host || !out) return ape_fail(APE_ERR_INVALID_ARG, "%s: NULL argument", what);
    if (int rc = ape_check_stream_list(what, streams_host, K, b->S, false)) return rc;
    int width, I;
    if (!parse_kind_dims(kind & ~APE_PARSE_BIG_ENDIAN, &width, &I)) return ape_fail(APE_ERR_INVALID_ARG, "%s: unknown kind %d", what, kind);
    ape_model* m = b->model;
    if (I != m->dims.input_size)
        return ape_fail(APE_ERR_INVALID_ARG, "%s: kind %d builds %d features, the model takes %d", what, kind & ~APE_PARSE_BIG_ENDIAN, I, m->dims.input_size);
    if (flags & ~(uint32_t)(APE_FLAG_NORMALIZE_INPUT | APE_FLAG_PACKED_MSG | APE_FLAG_SPREAD))
        return ape_fail(APE_ERR_INVALID_ARG, "%s: only NORMALIZE_INPUT, PACKED_MSG and SPREAD are accepted", what);
    if (out_dtype != APE_F32 && out_dtype != APE_F64) return ape_fail(APE_ERR_INVALID_ARG, "%s: unknown dtype selector", what);
    if (!b->xring || !b->yring || (m->dims.model_kind == APE_MODEL_FF && !b->ffhid))
        return ape_fail(APE_ERR_NOT_READY, "%s: the bank lost its rings in a failed ape_streams_set_mc", what);
    if ((flags & APE_FLAG_NORMALIZE_INPUT) && !m->has_stats) return ape_fail(APE_ERR_NOT_READY, "%s: NORMALIZE_INPUT without norm stats", what);
    if (!m->has_weights) return ape_fail(APE_ERR_NOT_READY, "%s: weights not loaded", what);
    if (b->inj_masks) return ape_fail(APE_ERR_UNSUPPORTED, "%s: injected masks (test hook) are indexed by the lockstep rows", what);
    APE_TRY(hipSetDevice(m->dims.device));
    if (int rc = ape_check_not_capturing((hipStream_t)stream, what, "the descriptors are staged per call")) return rc;
    *width_out = width; *I_out = I;
    return APE_OK;
}

// the subset frames' device workspaces on the first subset call, sized for K = S
static int subset_workspace(ape_streams* b, int I) {
    if (b->sub_n_mc == b->n_mc && b->sub_x) return APE_OK;
    subset_free(b);
    APE_TRY(hipMalloc((void**)&b->sub_x, (size_t)b->S * bank_copies(b) * b->T * I * sizeof(float)));
    APE_TRY(hipMalloc((void**)&b->sub_y, (size_t)b->S * b->n_mc * b->model->dims.output_size * sizeof(float)));
    APE_TRY(hipMalloc((void**)&b->sub_desc, (size_t)b->S * sizeof(SubsetDesc)));
    b->sub_n_mc = b->n_mc;
    return APE_OK;
}

// launch 1's parameters: the frame's rows and descriptors (device memory, or the host frame's pinned block) into rings and compact windows
static SubsetRowsParams subset_rows_params(const ape_streams* b, int kind, int width, int I, const float* rows, const SubsetDesc* desc, int K) {
    SubsetRowsParams rp{};
    rp.rows = rows; rp.desc = desc; rp.xring = b->xring; rp.xw = b->sub_x;
    rp.K = K; rp.width = width; rp.kind = kind & ~APE_PARSE_BIG_ENDIAN; rp.big_endian = (kind & APE_PARSE_BIG_ENDIAN) ? 1 : 0; rp.T = b->T; rp.I = I;
    rp.n_mc = bank_copies(b);
    return rp;
}

// the K descriptors of a frame from the per-stream counters, into `h`
static void subset_fill_desc(const ape_streams* b, const int32_t* streams_host, int K, SubsetDesc* h) {
    for (int j = 0; j < K; ++j) {
        const int s = streams_host[j];
        const long long f = b->s_frames[s], p = b->s_steps[s];
        h[j].stream = s;
        h[j].slot = (int)(f % b->T); h[j].cold = f == 0 ? 1 : 0;
        h[j].pos = (int)(p % bank_smooth_of(b, s)); h[j].pcold = p == 0 ? 1 : 0;
    }
}

// journaled like a step: re-issued by ape_model_recover while it is the bank's newest frame (an older pending one is lost)
static void subset_journal(ape_streams* b, int K, uint32_t flags, void* out, int out_dtype, void* stream, unsigned long long mc_call) {
    ape_model* m = b->model;
    int n = 0;
    for (int i = 0; i < m->journal_n; ++i) {
        const ApeJournalEntry& o = m->journal[i];
        if ((o.kind == ApeJournalEntry::SUBSET || o.kind == ApeJournalEntry::STEP) && o.bank == b) { m->journal_overflow = true; continue; }
        m->journal[n++] = o;
    }
    m->journal_n = n;
    ApeJournalEntry je{};
    je.kind = ApeJournalEntry::SUBSET; je.out0 = out; je.B = K; je.flags = flags; je.i2 = out_dtype; je.stream = stream;
    je.bank = b; je.bank_mc_calls = mc_call;
    journal_add(m, je);
}

int ape_streams_frame_subset(ape_streams_t* b, int32_t kind, const float* rows_dev, const int32_t* streams_host, int32_t K,
                             uint32_t flags, void* out_dev, int32_t out_dtype, void* stream) {
    int width, I;
    if (int rc = subset_frame_check(b, kind, rows_dev, streams_host, K, flags, out_dev, out_dtype, stream, "streams_frame_subset", &width, &I)) return rc;
    const hipStream_t st = (hipStream_t)stream;
    if (K == 0) return APE_OK;
    if (int rc = subset_workspace(b, I)) return rc;
    if (int rc = subset_stage_alloc(b)) return rc;
    subset_enter(b);
    // the descriptors into the next pinned slot -- once the copy that last read it has completed (frames go back to back, no host sync)
    hipError_t slot_wait;
    SubsetDesc* h = static_cast<SubsetDesc*>(b->sub_stage.take(&slot_wait));
    APE_TRY(slot_wait);
    subset_fill_desc(b, streams_host, K, h);
    APE_TRY(b->sub_stage.send(b->sub_desc, (size_t)K * sizeof(SubsetDesc), st));
    hipError_t e = ape_launch_subset_rows(subset_rows_params(b, kind, width, I, rows_dev, b->sub_desc, K), st);
    if (e != hipSuccess) return ape_fail(APE_ERR_HIP, "streams_frame_subset: row launch failed: %s", hipGetErrorString(e));
    // the rows are in the rings: the counters move on whatever the regressor does (a failed launch is reported, the rows stay pushed)
    for (int j = 0; j < K; ++j) { b->s_frames[streams_host[j]] += 1; b->s_steps[streams_host[j]] += 1; }
    const unsigned long long mc_call = b->mc_calls++;
    if (int rc = subset_regress_post(b, K, flags, out_dev, out_dtype, stream, mc_call)) return rc;
    subset_journal(b, K, flags, out_dev, out_dtype, stream, mc_call);
    return APE_OK;
}

// Host subset frame: the device entry's frame with host rows in and host rows out, BLOCKING, and with no copy command
// and no event on the stream.  The host writes rows and descriptors into one pinned block; launch 1 reads both from there and lands the
// descriptors in sub_desc, so launches 2 and 3 -- and the journal's re-issue -- read device memory as ever; launch 3 writes the rows,
// the model's status word and (K <= 64) a completion word per entry into pinned memory, as the lockstep host frame's post kernel does.
// The block is reused every frame: the call returns only when the frame is done.  Layout: [64] completion words, [S] descriptors,
// [S, 57] rows (57: the widest raw message).
static constexpr int SUBSET_HOST_ROW_MAX = 57;
int ape_streams_frame_subset_host(ape_streams_t* b, int32_t kind, const float* rows_host, const int32_t* streams_host, int32_t K,
                                  uint32_t flags, void* out_host, int32_t out_dtype, void* stream) {
    int width, I;
    if (int rc = subset_frame_check(b, kind, rows_host, streams_host, K, flags, out_host, out_dtype, stream, "streams_frame_subset_host", &width, &I))
        return rc;
    if (width > SUBSET_HOST_ROW_MAX) return ape_fail(APE_ERR_UNSUPPORTED, "streams_frame_subset_host: rows of %d columns", width);
    const hipStream_t st = (hipStream_t)stream;
    if (K == 0) return APE_OK;
    ape_model* m = b->model;
    if (int rc = subset_workspace(b, I)) return rc;
    const size_t N = (size_t)b->smooth * b->n_mc;
    const bool packed = (flags & APE_FLAG_PACKED_MSG) != 0 && N > 1;
    const size_t row_w = (packed ? 25 + 6 * N : 25) + ((flags & APE_FLAG_SPREAD) ? APE_SPREAD_WIDTH : 0);
    const size_t esz = out_dtype == APE_F64 ? sizeof(double) : sizeof(float);
    APE_TRY(ape_pinned_zeroed(&b->hs_block, 64 * sizeof(unsigned) + (size_t)b->S * sizeof(SubsetDesc) + (size_t)b->S * SUBSET_HOST_ROW_MAX * sizeof(float)));
    const size_t out_cap = (size_t)b->S * row_w * esz;          // (sized for K = S, so that the buffer settles with the first frame of a kind)
    APE_TRY(ape_pinned_grow(&b->h_out, &b->h_out_bytes, out_cap));
    APE_TRY(ape_pinned_zeroed(&b->h_status, 64));
    unsigned* const h_done = reinterpret_cast<unsigned*>(b->hs_block);
    SubsetDesc* const h_desc = reinterpret_cast<SubsetDesc*>(b->hs_block + 64 * sizeof(unsigned));
    float* const h_rows = reinterpret_cast<float*>(b->hs_block + 64 * sizeof(unsigned) + (size_t)b->S * sizeof(SubsetDesc));
    const bool words = K <= 64;                                  // a word per entry the host can watch; a longer list waits for the stream
    ape_done_next(&b->hs_done_val);
    subset_enter(b);
    HostFrameTail t;
    t.t_begin = now_us();
    memcpy(h_rows, rows_host, (size_t)K * width * sizeof(float));
    subset_fill_desc(b, streams_host, K, h_desc);
    *b->h_status = m->caps.cluster_ok ? 0xFFFFFFFFu : 0u;            // (a sentinel where a kernel writes the word: ape_streams_frame_host)
    hipError_t e = ape_launch_subset_rows_host(subset_rows_params(b, kind, width, I, h_rows, h_desc, K), b->sub_desc, st);
    if (e != hipSuccess) return ape_fail(APE_ERR_HIP, "streams_frame_subset_host: row launch failed: %s", hipGetErrorString(e));
    for (int j = 0; j < K; ++j) { b->s_frames[streams_host[j]] += 1; b->s_steps[streams_host[j]] += 1; }
    const unsigned long long mc_call = b->mc_calls++;
    const HostFrameWords hw{b->h_status, words ? h_done : nullptr, b->hs_done_val, "streams_frame_subset_host"};
    if (int rc = subset_regress_post(b, K, flags, b->h_out, out_dtype, stream, mc_call, hw)) {
        (void)hipStreamSynchronize(st);                          // (launch 1 may still read the block the next call rewrites)
        return rc;
    }
    subset_journal(b, K, flags, b->h_out, out_dtype, stream, mc_call);
    // aborted: the frame's windows and descriptors are on the device -- the journal runs regressor and post-filter again
    if (int rc = host_frame_wait(b, st, hw.done_out, K, hw.done_val, &t)) return rc;
    return host_frame_finish(b, t, out_host, (size_t)K * row_w * esz);
}

// ---- stream state hand-over: the canonical record of a stream, out of and into the rings -------------------------
// Slots and warm bits come from the host counters alone.  The descriptors travel through the subset frames' pinned ring into a device
// buffer of their own (sub_desc still belongs to the newest subset frame, which ape_model_recover may re-issue).

static void state_desc_of(const ape_streams* b, ape_stream_state_desc_t* d) {
    d->version = APE_STATE_VERSION;
    d->T = b->T; d->I = b->model->dims.input_size; d->smooth = b->smooth; d->n_mc = b->n_mc; d->O = b->model->dims.output_size;
    d->words_per_stream = (d->T * d->I + d->smooth * d->n_mc * d->O + 3) & ~3;
}

int ape_streams_state_desc(ape_streams_t* b, ape_stream_state_desc_t* out) {
    if (!b || !out) return ape_fail(APE_ERR_INVALID_ARG, "streams_state_desc: NULL argument");
    state_desc_of(b, out);
    return APE_OK;
}

// the K descriptors `h` (next pinned slot, already filled by `fill`) to the device, then one launch
template <typename Fill>
static int state_launch(ape_streams* b, const char* what, int K, float* state, hipStream_t st, bool import, Fill fill) {
    if (!b->state_desc) APE_TRY(hipMalloc((void**)&b->state_desc, (size_t)b->S * sizeof(StateDesc)));
    if (int rc = subset_stage_alloc(b)) return rc;
    static_assert(sizeof(StateDesc) <= sizeof(SubsetDesc), "a pinned slot holds S descriptors of either kind");
    hipError_t slot_wait;
    StateDesc* h = static_cast<StateDesc*>(b->sub_stage.take(&slot_wait));     // (waits for the copy that read this slot APE_DESC_STAGES calls ago)
    APE_TRY(slot_wait);
    for (int j = 0; j < K; ++j) fill(j, h[j]);
    APE_TRY(b->sub_stage.send(b->state_desc, (size_t)K * sizeof(StateDesc), st));
    ape_stream_state_desc_t d;
    state_desc_of(b, &d);
    StateParams p{};
    p.xring = b->xring; p.yring = b->yring; p.state = state; p.desc = b->state_desc;
    p.x_stream_stride = (size_t)bank_copies(b) * d.T * d.I;
    p.K = K; p.T = d.T; p.I = d.I; p.smooth = d.smooth; p.MO = d.n_mc * d.O; p.words = d.words_per_stream;
    const hipError_t e = bank_smooths_on(b) ? ape_launch_state_smooths(p, b->smooths.dev, import, st)
                         : import           ? ape_launch_state_import(p, st) : ape_launch_state_export(p, st);
    if (e != hipSuccess) return ape_fail(APE_ERR_HIP, "%s: launch failed: %s", what, hipGetErrorString(e));
    return APE_OK;
}

static int state_check_call(ape_streams* b, const int32_t* streams_host, int32_t K, const void* state_dev, const void* warm_host, void* stream,
                            const char* what) {
    if (!b || !streams_host || !state_dev || !warm_host) return ape_fail(APE_ERR_INVALID_ARG, "%s: NULL argument", what);
    if (int rc = ape_check_stream_list(what, streams_host, K, b->S, false)) return rc;
    if (((uintptr_t)state_dev & 15u) != 0) return ape_fail(APE_ERR_INVALID_ARG, "%s: state_dev must be 16-byte aligned", what);
    if (!b->xring || !b->yring) return ape_fail(APE_ERR_NOT_READY, "%s: the bank lost its rings in a failed ape_streams_set_mc", what);
    APE_TRY(hipSetDevice(b->model->dims.device));
    return ape_check_not_capturing((hipStream_t)stream, what, "the descriptors are staged per call");
}

int ape_streams_export(ape_streams_t* b, const int32_t* streams_host, int32_t K, void* state_dev, uint8_t* warm_host, void* stream) {
    if (int rc = state_check_call(b, streams_host, K, state_dev, warm_host, stream, "streams_export")) return rc;
    if (K == 0) return APE_OK;
    // read-only: a lockstep bank stays in lockstep mode, its streams share the global counters
    auto fill = [&](int j, StateDesc& d) {
        const int s = streams_host[j];
        const long long f = b->per_stream ? b->s_frames[s] : b->frames, p = b->per_stream ? b->s_steps[s] : b->steps;
        // the newest row sits in slot (f - 1) mod T, so the oldest of the T rows in slot f mod T (all T slots are filled from the first row on)
        d.stream = s; d.wslot = (int)(f % b->T); d.sslot = (int)(p % bank_smooth_of(b, s));
        d.warm = (f > 0 ? APE_STATE_WINDOW_WARM : 0) | (f > 0 && p > 0 ? APE_STATE_STACK_WARM : 0);
        warm_host[j] = (uint8_t)d.warm;
    };
    return state_launch(b, "streams_export", K, (float*)state_dev, (hipStream_t)stream, false, fill);
}

int ape_streams_import(ape_streams_t* b, const ape_stream_state_desc_t* desc, const int32_t* streams_host, int32_t K,
                       const void* state_dev, const uint8_t* warm_host, void* stream) {
    if (!desc) return ape_fail(APE_ERR_INVALID_ARG, "streams_import: NULL argument");
    if (int rc = state_check_call(b, streams_host, K, state_dev, warm_host, stream, "streams_import")) return rc;
    ape_stream_state_desc_t own;
    state_desc_of(b, &own);
    if (desc->version != own.version || desc->T != own.T || desc->I != own.I || desc->smooth != own.smooth || desc->n_mc != own.n_mc ||
        desc->O != own.O || desc->words_per_stream != own.words_per_stream)
        return ape_fail(APE_ERR_INVALID_ARG, "streams_import: the records are {v%d T=%d I=%d smooth=%d n_mc=%d O=%d words=%d}, the bank's {v%d T=%d I=%d smooth=%d n_mc=%d O=%d words=%d}",
                    desc->version, desc->T, desc->I, desc->smooth, desc->n_mc, desc->O, desc->words_per_stream, own.version, own.T, own.I,
                    own.smooth, own.n_mc, own.O, own.words_per_stream);
    if (K == 0) return APE_OK;
    // time order = slot order: row t into slot t, the counters at T / smooth -- the next row lands on slot 0, the oldest
    auto fill = [&](int j, StateDesc& d) {
        const int w = warm_host[j] & APE_STATE_WINDOW_WARM;
        d.stream = streams_host[j]; d.wslot = 0; d.sslot = 0;
        d.warm = w ? (warm_host[j] & (APE_STATE_WINDOW_WARM | APE_STATE_STACK_WARM)) : 0;
    };
    if (int rc = state_launch(b, "streams_import", K, (float*)const_cast<void*>(state_dev), (hipStream_t)stream, true, fill)) return rc;
    subset_enter(b);
    for (int j = 0; j < K; ++j) {
        const int s = streams_host[j];
        const bool w = (warm_host[j] & APE_STATE_WINDOW_WARM) != 0, p = w && (warm_host[j] & APE_STATE_STACK_WARM) != 0;
        b->s_frames[s] = w ? b->T : 0;
        b->s_steps[s] = p ? bank_smooth_of(b, s) : 0;        // (the record was read with the slot's own length: that many predictions)
    }
    // the rings changed behind the bank's pending frame: like a newer frame, the import takes it off the journal
    ape_model* m = b->model;
    int n = 0;
    for (int i = 0; i < m->journal_n; ++i) {
        const ApeJournalEntry& o = m->journal[i];
        if ((o.kind == ApeJournalEntry::SUBSET || o.kind == ApeJournalEntry::STEP) && o.bank == b) { m->journal_overflow = true; continue; }
        m->journal[n++] = o;
    }
    m->journal_n = n;
    return APE_OK;
}

