// The NN stream bank (ape_streams_*): lifecycle, Monte-Carlo mode, bodies and smoothing lengths, the pushes, the lockstep
// step with its routes, the lockstep host frame, and the frame statistics.  Subset frames and the state hand-over: api_subset.hip.
#include <cstring>
#include <new>

#include "ape_host.h"

static void bank_free_regressor_ws(ape_streams* b) {
    if (b->ffhid) (void)hipFree(b->ffhid);
    if (b->xwin) (void)hipFree(b->xwin);
    b->ffhid = b->xwin = nullptr;
}

// (re)allocates the three rings for the bank's current S, T, smooth, n_mc
static hipError_t bank_alloc(ape_streams* b) {
    const size_t I = b->model->dims.input_size, O = b->model->dims.output_size, R = (size_t)b->S * b->n_mc;
    if (b->xring) (void)hipFree(b->xring);
    if (b->yring) (void)hipFree(b->yring);
    if (b->y_new) (void)hipFree(b->y_new);
    b->xring = b->yring = b->y_new = nullptr;
    bank_free_regressor_ws(b);
    hipError_t e = hipMalloc((void**)&b->xring, (size_t)b->S * bank_copies(b) * b->T * I * sizeof(float));
    if (e == hipSuccess && b->model->dims.model_kind == APE_MODEL_FF)
        e = hipMalloc((void**)&b->ffhid, (size_t)b->S * b->model->dims.hidden_size * sizeof(float));
    if (e == hipSuccess && b->model->dims.model_kind == APE_MODEL_IMUPOSE)
        e = hipMalloc((void**)&b->xwin, (size_t)b->S * b->T * I * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void**)&b->yring, R * b->smooth * O * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void**)&b->y_new, R * O * sizeof(float));
    // a few streams with tall smoothing stacks: the post-filter deals a stream's stack over several workgroups (one CU each)
    if (b->post_part) (void)hipFree(b->post_part);
    b->post_part = nullptr; b->post_cnt = nullptr; b->post_spread = nullptr;
    const int chunks = ape_stream_post_chunks(b->smooth * b->n_mc);
    if (e == hipSuccess && chunks > 1 && (long long)b->S * chunks <= b->model->n_cus) {
        const size_t part_bytes = (size_t)b->S * chunks * 21 * sizeof(double);
        // (behind the tickets, 8-byte aligned: the spread record's partial sums, four role waves x 18 per chunk -- APE_FLAG_SPREAD frames)
        const size_t cnt_bytes = ((size_t)b->S * sizeof(unsigned) + 7) & ~(size_t)7;
        const size_t spread_bytes = (size_t)b->S * chunks * 72 * sizeof(double);
        e = hipMalloc((void**)&b->post_part, part_bytes + cnt_bytes + spread_bytes);
        if (e == hipSuccess) e = hipMemset(b->post_part, 0, part_bytes + cnt_bytes + spread_bytes);
        if (e == hipSuccess) b->post_cnt = reinterpret_cast<unsigned*>(reinterpret_cast<char*>(b->post_part) + part_bytes);
        if (e == hipSuccess) b->post_spread = reinterpret_cast<double*>(reinterpret_cast<char*>(b->post_part) + part_bytes + cnt_bytes);
    }
    return e;
}

int ape_streams_create(ape_model_t* m, int32_t n_streams, int32_t seq_len, int32_t smooth, ape_streams_t** out) {
    if (!out) return ape_fail(APE_ERR_INVALID_ARG, "streams_create: out is NULL");
    *out = nullptr;
    if (!m) return ape_fail(APE_ERR_INVALID_ARG, "streams_create: NULL model");
    if (m->dims.target_layout == APE_LAYOUT_NONE) return ape_fail(APE_ERR_INVALID_ARG, "streams_create: model has no target layout");
    if (n_streams < 1 || seq_len < 1) return ape_fail(APE_ERR_INVALID_ARG, "streams_create: n_streams=%d seq_len=%d", n_streams, seq_len);
    if (smooth < 1 || smooth > 64) return ape_fail(APE_ERR_UNSUPPORTED, "streams_create: smooth %d outside 1..64", smooth);
    ape_streams* b = new (std::nothrow) ape_streams();
    if (!b) return ape_fail(APE_ERR_HIP, "out of host memory");
    b->model = m; b->S = n_streams; b->T = seq_len; b->smooth = smooth;
    // DropoutFF (nn_models.py:340-352 behind watch_phone_pocket_nn.py:111): [:, -1, :] of a row-wise MLP -- the window, its length and its
    // cold-start padding have no influence on the output, so the bank keeps the newest row only
    if (m->dims.model_kind == APE_MODEL_FF) b->T = 1;
    hipError_t e = hipSetDevice(m->dims.device);
    if (e == hipSuccess) e = bank_alloc(b);
    if (e != hipSuccess) {
        ape_streams_destroy(b);
        return ape_fail(APE_ERR_HIP, "streams_create: allocation failed: %s", hipGetErrorString(e));
    }
    *out = b;
    return APE_OK;
}

// Sample rows per launch of a Monte-Carlo bank's weight-stationary route (pure arithmetic: ape_debug_bank_chunks, tests/test_plan_cpu.py).
// The pre-laid input is T x 1 KiB per sample row of a 2 x 256 model (lstm_upper32.hip), T x 512 B of the 3 x 128 model
// (lstm_upper128.hip); it and -- 2 x 256 models -- launch A's sequence and input tiles sit behind ONE 32-bit buffer descriptor each, so
// a bank that outgrows 2 GiB of any of them is chunked (launch B) or keeps the batch-tile route (launch A: 65 536 streams of 64 steps).
int ape_streams_set_mc(ape_streams_t* b, int32_t n_mc, float dropout_p, uint64_t seed) {
    if (!b) return ape_fail(APE_ERR_INVALID_ARG, "streams_set_mc: NULL bank");
    if (n_mc < 1 || (long long)n_mc * b->smooth > 4096)
        return ape_fail(APE_ERR_INVALID_ARG, "streams_set_mc: n_mc=%d with smooth=%d (1 <= smooth*n_mc <= 4096)", n_mc, b->smooth);
    if (!(dropout_p >= 0.0f && dropout_p < 1.0f)) return ape_fail(APE_ERR_INVALID_ARG, "streams_set_mc: dropout_p %g outside [0,1)", (double)dropout_p);
    APE_TRY(hipSetDevice(b->model->dims.device));
    APE_TRY(hipDeviceSynchronize());             // the rings may still be read by an earlier step
    // ImuPoseLSTM.monte_carlo_predictions(n_samples, x) is self(x, None) (nn_models.py:246-251): the count is ignored and there is no
    // dropout -- the bank keeps one row per stream and frame (the call is still the cold start it is for the other banks)
    if (b->model->dims.model_kind == APE_MODEL_IMUPOSE) { n_mc = 1; dropout_p = 0.0f; }
    b->n_mc = n_mc; b->mc = b->model->dims.model_kind != APE_MODEL_IMUPOSE; b->dropout_p = dropout_p; b->seed = seed; b->mc_calls = 0;
    b->frames = 0; b->steps = 0;
    b->per_stream = false;
    subset_free(b);
    hipError_t e = bank_alloc(b);
    if (e != hipSuccess) {
        // the old rings are gone and the new ones are incomplete: the bank stays unusable (every push / step refuses)
        // until a later ape_streams_set_mc succeeds
        if (b->xring) (void)hipFree(b->xring);
        if (b->yring) (void)hipFree(b->yring);
        if (b->y_new) (void)hipFree(b->y_new);
        b->xring = b->yring = b->y_new = nullptr;
        bank_free_regressor_ws(b);
        return ape_fail(APE_ERR_HIP, "streams_set_mc: allocation failed: %s", hipGetErrorString(e));
    }
    // the route (csrc/ape_plan.h).  The [S,T,H] sequence of a shared layer 0 lives in the model's all-steps workspace, sized here so
    // that the step itself never allocates.
    ape_model* m = b->model;
    const BankPlan want = plan_bank(m->caps, m->dims, b->S, b->T, n_mc, dropout_p, m->kernel_choice, m->precision, m->c32_on, bank_l0_bytes(b->S, b->T));
    b->plan = want;
    if (want.route == BANK_UPPER32 || want.route == BANK_UPPER128) { b->plan.route = BANK_SHARED_TILE16; b->plan.a_form = BANK_A_TILE16; }   // (until its workspaces exist)
    for (void** ws : {(void**)&b->xfrag, (void**)&b->ypart, (void**)&b->xfrag0, (void**)&b->hfrag, (void**)&b->maskbits})
        if (*ws) { (void)hipFree(*ws); *ws = nullptr; }
    if (want.shared_l0) {
        const size_t rows = (size_t)b->S * b->T;
        if (rows > m->hseq_cap) {
            if (m->hseq_ws) { APE_TRY(hipFree(m->hseq_ws)); m->hseq_ws = nullptr; m->hseq_cap = 0; }
            APE_TRY(hipMalloc((void**)&m->hseq_ws, rows * m->dims.hidden_size * sizeof(float)));
            m->hseq_cap = rows;
        }
        const int chunk = (int)want.chunk_rows;
        if (want.route == BANK_UPPER128) {
            // the 3 x 128 model: launch A stays on the batch-tile kernel ([S,T,H] in the model's sequence workspace), launch B =
            // layers 1 and 2 on lstm_upper128.hip
            APE_TRY(hipMalloc((void**)&b->xfrag, ape_upper128_xfrag_bytes(chunk, b->T)));
            APE_TRY(hipMalloc((void**)&b->ypart, ape_upper128_ypart_bytes(chunk)));
            APE_TRY(hipMalloc((void**)&b->maskbits, ape_upper128_maskbits_bytes(chunk, b->T)));
        } else if (want.route == BANK_UPPER32) {
            APE_TRY(hipMalloc((void**)&b->xfrag, ape_upper32_xfrag_bytes(chunk, b->T)));
            APE_TRY(hipMalloc((void**)&b->ypart, ape_upper32_ypart_bytes(chunk)));
            // layer 0 on the same cluster structure (its SEQ form): input tiles and the [tile][step] sequence, fragment order
            APE_TRY(hipMalloc((void**)&b->xfrag0, ape_lower32_xfrag_bytes(b->S, b->T)));
            APE_TRY(hipMalloc((void**)&b->hfrag, ape_lower32_hseq_bytes(b->S, b->T)));
        }
        b->plan = want;
    }
    return APE_OK;
}

int ape_streams_destroy(ape_streams_t* b) {
    if (!b) return APE_OK;
    if (b->xring) (void)hipFree(b->xring);
    if (b->yring) (void)hipFree(b->yring);
    if (b->y_new) (void)hipFree(b->y_new);
    if (b->post_part) (void)hipFree(b->post_part);
    bank_free_regressor_ws(b);
    if (b->xfrag) (void)hipFree(b->xfrag);
    if (b->ypart) (void)hipFree(b->ypart);
    if (b->xfrag0) (void)hipFree(b->xfrag0);
    if (b->hfrag) (void)hipFree(b->hfrag);
    if (b->maskbits) (void)hipFree(b->maskbits);
    if (b->h_rows) (void)hipHostFree(b->h_rows);
    if (b->h_out) (void)hipHostFree(b->h_out);
    if (b->h_status) (void)hipHostFree(b->h_status);
    if (b->h_done) (void)hipHostFree(b->h_done);
    if (b->hs_block) (void)hipHostFree(b->hs_block);
    for (auto ev : b->prof_ev) if (ev) (void)hipEventDestroy(ev);
    subset_free(b);                     // (takes the bank's pending subset frame off the journal, as the steps below)
    ape_body_table_free(b->bodies);
    ape_smooth_table_free(b->smooths);
    b->sub_stage.free();
    if (b->state_desc) (void)hipFree(b->state_desc);
    if (ape_model* m = b->model) {      // pending steps of this bank can no longer be re-issued
        int k = 0;
        for (int i = 0; i < m->journal_n; ++i) {
            if (m->journal[i].kind == ApeJournalEntry::STEP && m->journal[i].bank == b) { m->journal_overflow = true; continue; }
            m->journal[k++] = m->journal[i];
        }
        m->journal_n = k;
    }
    delete b;
    return APE_OK;
}

int ape_streams_reset(ape_streams_t* b) {
    if (!b) return ape_fail(APE_ERR_INVALID_ARG, "streams_reset: NULL bank");
    b->frames = 0; b->steps = 0;
    b->per_stream = false;                       // every stream cold: the lockstep calls serve the bank again
    return APE_OK;
}

// per-stream body measurements: replaces the bonemap every reference Estimator is built with (estimator.py:57-68).
// No cold start: windows and stacks hold features and NN targets, which do not depend on the body.
int ape_streams_set_bodies(ape_streams_t* b, const int32_t* streams_host, int32_t K, const double* body9s_host, void* stream) {
    if (!b || !body9s_host) return ape_fail(APE_ERR_INVALID_ARG, "streams_set_bodies: NULL argument");
    if (streams_host) {
        if (int rc = ape_check_stream_list("streams_set_bodies", streams_host, K, b->S, false)) return rc;
    } else if (K != b->S) return ape_fail(APE_ERR_INVALID_ARG, "streams_set_bodies: no stream list: K=%d must be S=%d", K, b->S);
    APE_TRY(hipSetDevice(b->model->dims.device));
    if (int rc = ape_check_not_capturing((hipStream_t)stream, "streams_set_bodies", "the table's image is staged per call")) return rc;
    APE_TRY(ape_body_table_set(b->bodies, b->S, false, b->model->body, streams_host, K, body9s_host, (hipStream_t)stream));
    return APE_OK;
}

int ape_streams_get_bodies(ape_streams_t* b, double* out_host) {
    if (!b || !out_host) return ape_fail(APE_ERR_INVALID_ARG, "streams_get_bodies: NULL argument");
    ape_body_table_get(b->bodies, b->S, b->model->body, out_host);
    return APE_OK;
}

// per-stream smoothing lengths: replaces the `smooth` every reference Estimator is built with (estimator.py:45,112-118).
// A cold start of the listed streams: the reference fixes the value at construction, a change has no defined transition.
int ape_streams_set_smooths(ape_streams_t* b, const int32_t* streams_host, int32_t K, const int32_t* smooths_host, void* stream) {
    if (int rc = ape_smooth_table_check("streams_set_smooths", b, streams_host, K, b ? b->S : 0, smooths_host, b ? b->smooth : 0)) return rc;
    APE_TRY(hipSetDevice(b->model->dims.device));
    if (int rc = ape_check_not_capturing((hipStream_t)stream, "streams_set_smooths", "the table's image is staged per call")) return rc;
    APE_TRY(ape_smooth_table_set(b->smooths, b->S, b->smooth, streams_host, K, smooths_host, (hipStream_t)stream));
    if (!streams_host) return ape_streams_reset(b);
    return ape_streams_reset_subset(b, streams_host, K);
}

int ape_streams_get_smooths(ape_streams_t* b, int32_t* out_host) {
    if (!b || !out_host) return ape_fail(APE_ERR_INVALID_ARG, "streams_get_smooths: NULL argument");
    ape_smooth_table_get(b->smooths, b->S, b->smooth, out_host);
    return APE_OK;
}

// where the next row goes: one slot of each of the stream's n_mc windows (stride T*I apart), or -- first row after
// a reset -- all n_mc*T slots, which are contiguous
static void next_slot(const ape_streams* b, size_t I, float** out, int* rep, size_t* rep_stride) {
    const bool cold = b->frames == 0;
    *out = b->xring + (cold ? 0 : (size_t)(b->frames % b->T) * I);
    const int copies = b->plan.shared_l0 ? 1 : bank_copies(b);      // layer 0 shared: only a stream's first window copy is ever read
    *rep = cold ? b->T * copies : copies;
    *rep_stride = cold ? I : (size_t)b->T * I;
}

int ape_streams_push_rows(ape_streams_t* b, int32_t kind, const float* rows_dev, void* stream) {
    if (!b || !rows_dev) return ape_fail(APE_ERR_INVALID_ARG, "streams_push_rows: NULL argument");
    if (!b->xring) return ape_fail(APE_ERR_NOT_READY, "streams_push_rows: the bank lost its rings in a failed ape_streams_set_mc");
    if (b->per_stream) return ape_fail(APE_ERR_NOT_READY, "streams_push_rows: the bank is in per-stream mode (subset frames); ape_streams_reset first");
    int width, I;
    const int big_endian = (kind & APE_PARSE_BIG_ENDIAN) ? 1 : 0;
    kind &= ~APE_PARSE_BIG_ENDIAN;
    if (!parse_kind_dims(kind, &width, &I)) return ape_fail(APE_ERR_INVALID_ARG, "streams_push_rows: unknown kind %d", kind);
    if (I != b->model->dims.input_size)
        return ape_fail(APE_ERR_INVALID_ARG, "streams_push_rows: kind %d builds %d features, the model takes %d", kind, I,
                    b->model->dims.input_size);
    float* out; int rep; size_t rep_stride;
    next_slot(b, (size_t)I, &out, &rep, &rep_stride);
    hipError_t e = ape_launch_parse_rows(rows_dev, b->S, width, kind, out, APE_F32, I, (size_t)bank_copies(b) * b->T * I, rep,
                                         rep_stride, big_endian, (hipStream_t)stream);
    if (e != hipSuccess) return ape_fail(APE_ERR_HIP, "streams_push_rows launch failed: %s", hipGetErrorString(e));
    ++b->frames;
    return APE_OK;
}

int ape_streams_push_features(ape_streams_t* b, const float* xx_dev, void* stream) {
    if (!b || !xx_dev) return ape_fail(APE_ERR_INVALID_ARG, "streams_push_features: NULL argument");
    if (!b->xring) return ape_fail(APE_ERR_NOT_READY, "streams_push_features: the bank lost its rings in a failed ape_streams_set_mc");
    if (b->per_stream) return ape_fail(APE_ERR_NOT_READY, "streams_push_features: the bank is in per-stream mode (subset frames); ape_streams_reset first");
    const int I = b->model->dims.input_size;
    float* out; int rep; size_t rep_stride;
    next_slot(b, (size_t)I, &out, &rep, &rep_stride);
    hipError_t e = ape_launch_ring_write(xx_dev, b->S, I, out, (size_t)bank_copies(b) * b->T * I, rep, rep_stride, (hipStream_t)stream);
    if (e != hipSuccess) return ape_fail(APE_ERR_HIP, "streams_push_features launch failed: %s", hipGetErrorString(e));
    ++b->frames;
    return APE_OK;
}

// a few streams in Monte-Carlo mode (one estimator's frame: S = 1) step on the Monte-Carlo latency kernel
static bool bank_on_mc_small(const ape_streams* b) {
    const ape_model* m = b->model;
    return m->dims.model_kind == APE_MODEL_LSTM && !b->plan.shared_l0 && b->mc && b->dropout_p > 0.0f && m->dims.num_layers > 1 && b->S <= 8 && m->caps.cluster_ok && b->T <= 64 &&
           mc_small_fits(m->caps, m->dims, m->kernel_choice, m->precision, m->c32_on, m->replaying, b->S, b->n_mc);       // (mc_small_launch's condition)
}
// can the feature builder's workgroups become resident beside the clusters?  A cluster member takes a CU's worth of LDS only in the
// 16-row form; with 8-row clusters two workgroups share a CU, and the 3 x 128 model leaves half the CUs free anyway
static bool mc_small_builder_fits(const ape_model* m, int n_streams, int n_mc, int T) {
    const int cps = 8 / n_streams;
    // (8-row clusters: 39 KB of B tiles and sums + 0.5 KB of mask bits per step + 10.5 KB static per member -- two workgroups per CU up to T = 32)
    return m->dims.hidden_size == 128 || ((n_mc + cps - 1) / cps <= 8 && T <= 32);
}
// measurement aid (ape_streams_profile): the next pair of events, around a launch of the step's dominant kernel (null: off, or all used)
struct ProfPair { hipEvent_t a = nullptr, z = nullptr; };
static ProfPair prof_pair(ape_streams* b) {
    ProfPair ev;
    if (!b->prof_on || b->prof_n >= (int)b->prof_ev.size() / 2) return ev;
    ev.a = b->prof_ev[2 * b->prof_n]; ev.z = b->prof_ev[2 * b->prof_n + 1];
    b->prof_n += 1;
    return ev;
}
// ... recorded around `launch`, which answers an APE_* code (a failed launch leaves the pair open: its step is refused)
template <typename Launch>
static int profiled(ape_streams* b, void* stream, Launch launch) {
    const ProfPair ev = prof_pair(b);
    if (ev.a) (void)hipEventRecord(ev.a, (hipStream_t)stream);
    if (int rc = launch()) return rc;
    if (ev.z) (void)hipEventRecord(ev.z, (hipStream_t)stream);
    return APE_OK;
}

StreamPostParams bank_post_params(const ape_streams* b, const float* y_new, int rows, bool norm, void* msg, int out_dtype, bool packed,
                                  const HostFrameWords& hw) {
    const ape_model* m = b->model;
    StreamPostParams q{};
    q.y_new = y_new; q.yring = b->yring; q.msg = msg;
    q.yy_m = norm ? m->stats + 2 * m->dims.input_size : nullptr;      // one switch (estimator.py:103-109)
    q.yy_s = norm ? m->stats + 2 * m->dims.input_size + m->dims.output_size : nullptr;
    memcpy(q.body, m->body, sizeof(q.body));
    q.S = rows; q.O = m->dims.output_size; q.W = layout_est_width(m->dims.target_layout); q.layout = m->dims.target_layout;
    q.smooth = b->smooth; q.n_mc = b->n_mc;
    q.msg_dtype = out_dtype; q.packed = packed ? 1 : 0;
    if (hw.status_out != nullptr && m->caps.cluster_ok) { q.status_in = ctl_words(m).status; q.status_out = hw.status_out; }
    if (hw.done_out != nullptr) { q.done_out = hw.done_out; q.done_val = hw.done_val; }      // (word j behind row j)
    q.part = b->post_part; q.part_cnt = b->post_cnt;     // (sized for S >= rows entries)
    return q;
}

// hw (host frames): the pinned words that receive the model's sticky status word and the completion words behind the step's kernels
int streams_step_impl(ape_streams_t* b, uint32_t flags, void* msg_dev, void* tail_dev, int32_t out_dtype, void* stream, const HostFrameWords& hw,
                      const McFrameParts* fuse) {
    if (!b || !msg_dev) return ape_fail(APE_ERR_INVALID_ARG, "streams_step: NULL argument");
    if (!b->xring || !b->yring || !b->y_new)
        return ape_fail(APE_ERR_NOT_READY, "streams_step: the bank lost its rings in a failed ape_streams_set_mc");
    if (b->per_stream) return ape_fail(APE_ERR_NOT_READY, "streams_step: the bank is in per-stream mode (subset frames); ape_streams_reset first");
    if (b->frames == 0) return ape_fail(APE_ERR_NOT_READY, "streams_step: no row pushed since the last reset");
    // the exchange-form selectors of include/ape_hip.h travel to the frame's LSTM launches unchanged (same bits whichever is set)
    const uint32_t diag_wt = flags & (APE_FLAG_ANY_PLACEMENT | APE_FLAG_IN_XCD_PLAIN | APE_FLAG_NO_XCD_CLASSES);
    flags &= ~diag_wt;
    if (flags & ~(uint32_t)(APE_FLAG_NORMALIZE_INPUT | APE_FLAG_PACKED_MSG | APE_FLAG_SPREAD))
        return ape_fail(APE_ERR_INVALID_ARG, "streams_step: NORMALIZE_INPUT, PACKED_MSG, SPREAD and the exchange-form selectors ANY_PLACEMENT, "
                    "IN_XCD_PLAIN, NO_XCD_CLASSES are accepted");
    const bool spread = (flags & APE_FLAG_SPREAD) != 0;     // every msg row APE_SPREAD_WIDTH columns longer (post-filter, SPR forms)
    flags &= ~(uint32_t)APE_FLAG_SPREAD;
    if (out_dtype != APE_F32 && out_dtype != APE_F64) return ape_fail(APE_ERR_INVALID_ARG, "streams_step: unknown dtype selector");
    const bool packed = (flags & APE_FLAG_PACKED_MSG) != 0;
    if (packed && tail_dev)
        return ape_fail(APE_ERR_INVALID_ARG, "streams_step: PACKED_MSG rows carry the tail themselves (tail_dev must be NULL)");
    flags &= ~(uint32_t)APE_FLAG_PACKED_MSG;
    ape_model* m = b->model;
    const bool norm = (flags & APE_FLAG_NORMALIZE_INPUT) != 0;
    if (norm && !m->has_stats) return ape_fail(APE_ERR_NOT_READY, "streams_step: NORMALIZE_INPUT without norm stats");
    // oldest row of every window: the slot after the newest one
    const int x_ring = (int)(b->frames % b->T);
    const bool drop = b->mc && b->dropout_p > 0.0f && m->dims.num_layers > 1;
    ApeJournalEntry je{};
    je.kind = ApeJournalEntry::STEP; je.out0 = msg_dev; je.out1 = tail_dev; je.flags = flags | (packed ? APE_FLAG_PACKED_MSG : 0u) | (spread ? APE_FLAG_SPREAD : 0u);
    je.i2 = out_dtype; je.stream = stream; je.bank = b; je.bank_frames = b->frames; je.bank_steps = b->steps; je.bank_mc_calls = b->mc_calls;
    if (m->dims.model_kind == APE_MODEL_FF) {
        // DropoutFF: the newest row of every stream (T = 1: slot 0) -> trunk once per stream -> n_mc masked heads -> y_new in the row
        // order the post-filter reads.  Masks keyed by (seed + frame counter; row = stream * n_mc + sample; hidden unit)
        if (!b->ffhid) return ape_fail(APE_ERR_NOT_READY, "streams_step: the bank lost its rings in a failed ape_streams_set_mc");
        if (b->inj_masks && !b->mc)
            return ape_fail(APE_ERR_UNSUPPORTED, "streams_step: injected masks (test hook) on a DropoutFF bank without ape_streams_set_mc");
        const ProfPair ev = prof_pair(b);           // (handed into the launch pair: recorded around the trunk and the heads)
        if (int rc = ff_bank_forward(m, b->xring, (size_t)m->dims.input_size, 0, b->S * b->n_mc, b->n_mc, norm, b->inj_masks,
                                     b->mc ? b->dropout_p : 0.0f, b->seed + b->mc_calls, b->ffhid, b->y_new, stream, ev.a, ev.z))
            return rc;
    } else if (m->dims.model_kind == APE_MODEL_IMUPOSE) {
        // ImuPoseLSTM: the rings in time order (cold-start pad included), then the forward a subset frame runs over its compact windows
        // (x_ring = 0: the layer-split route above 512 windows applies) -- the same launches, hence the same bits
        if (!b->xwin) return ape_fail(APE_ERR_NOT_READY, "streams_step: the bank lost its rings in a failed ape_streams_set_mc");
        hipError_t e = ape_launch_ring_windows(b->xring, b->xwin, b->S, b->T, m->dims.input_size, x_ring, (hipStream_t)stream);
        if (e != hipSuccess) return ape_fail(APE_ERR_HIP, "streams_step: window launch failed: %s", hipGetErrorString(e));
        if (int rc = profiled(b, stream, [&] { return lstm_forward_impl(m, b->xwin, b->S, b->T, flags | diag_wt, nullptr, 0.0f, 0, b->y_new, stream, 0); }))
            return rc;
    } else if (b->plan.shared_l0) {
        if (!m->has_weights) return ape_fail(APE_ERR_NOT_READY, "streams_step: weights not loaded");
        if ((size_t)b->S * b->T > m->hseq_cap) return ape_fail(APE_ERR_CAPACITY, "streams_step: the layer-0 sequence workspace is gone");
        const int H = m->dims.hidden_size, I = m->dims.input_size, O = m->dims.output_size;
        // (the cooperative routes were planned by ape_streams_set_mc; a later set_kernel(TILE16 / AUTO_GEN1 / CLUSTER) or set_precision --
        //  the documented ways to keep persistent clusters off a shared GPU -- sends the step to the batch-tile route like a replay)
        const bool coop = !m->replaying && m->kernel_choice == APE_KERNEL_AUTO && m->c32_on && m->precision == APE_PRECISION_F32;
        const int route = coop ? b->plan.route : BANK_SHARED_TILE16, a_form = coop ? b->plan.a_form : BANK_A_TILE16;
        hipError_t e = hipSuccess;
        if (a_form == BANK_A_ONE_LAYER) {
            // launch A on the first-generation cluster kernel's one-layer form (lstm_cluster.hip <H, 1, KX, 2>): 32 streams per cluster of H / 16
            // members, every step's output -> [S,T,H] in the model's sequence workspace, as the batch-tile launch writes it
            // (2 x 256 models, small banks: the one-layer form's 16-member clusters have half the matrix work per CU and step of the 8-member
            //  SEQ form below and the same exposed exchange; APE_BANK_A_ONE_LAYER_MAX_STREAMS)
            // (the 3 x 128 bank, round 5: 1024 streams are 64 tiles of the batch-tile kernel -- a quarter
            // of the chip for 54 us; here every CU holds 16 units of a cluster: 30.8 us).  Every bank size that fits the chip's clusters:
            // 21 x 50 rows 141.6 -> 121.0 us per frame, 100 x 25 188.1 -> 164.5, 127 x 25 190.2 -> 166.4 against the batch-tile launch.
            ClusterParams c = cluster_params(m, PLAN_GEN1, 1, b->xring, nullptr, b->S, b->T, (flags & APE_FLAG_NORMALIZE_INPUT) | diag_wt, x_ring);
            c.x_row_stride = (size_t)bank_copies(b) * b->T * I;
            c.hseq = m->hseq_ws;
            bool classes = false;
            const int clusters = xcd_class_clusters((b->S + 31) / 32, m->caps.cluster_capacity, xcd_classes_on(m, diag_wt), &classes);
            if (classes) c.flags |= APE_FLAG_XCD_CLASSES;
            e = ape_launch_lstm_cluster(H, 1, m->KX, 2, false, clusters, c, (hipStream_t)stream);
            if (e != hipSuccess) return ape_fail(APE_ERR_HIP, "streams_step: layer-0 cluster launch failed: %s", hipGetErrorString(e));
        } else if (a_form == BANK_A_SEQ32) {
            // launch A on the weight-stationary structure (lstm_upper32.hip, SEQ form): S streams in tiles of 32 on the clusters,
            // every step's output in the fragment order launch B's input builder reads
            XFragParams xq{};
            xq.x = b->xring; xq.xfrag = b->xfrag0; xq.x_row_stride = (size_t)bank_copies(b) * b->T * I;
            xq.xx_m = norm ? m->stats : nullptr; xq.xx_s = norm ? m->stats + I : nullptr;
            xq.S = b->S; xq.T = b->T; xq.I = I; xq.x_ring = x_ring;
            UpperParams u = upper_params(m, b->T, (b->S + 31) / 32, diag_wt);
            u.xfrag = b->xfrag0; u.xfrag_bytes = ape_lower32_xfrag_bytes(b->S, b->T);
            u.w = m->wcl32[0]; u.bias = m->bias[0];
            u.hseq = b->hfrag; u.hseq_bytes = ape_lower32_hseq_bytes(b->S, b->T);
            e = ape_launch_lstm_lower32(u, xq, m->caps.f16v2_capacity, (hipStream_t)stream);
            if (e != hipSuccess) return ape_fail(APE_ERR_HIP, "streams_step: layer-0 cluster launch failed: %s", hipGetErrorString(e));
        } else {
        // launch A: layer 0 alone over the S windows (first copy of every stream's ring), all steps -> [S,T,H]
        LstmParams a{};
        a.x = b->xring; a.x_row_stride = (size_t)bank_copies(b) * b->T * I;
        a.y = nullptr; a.hseq = m->hseq_ws;
        a.wpack[0] = m->wpack[0]; a.bias[0] = m->bias[0];
        head_and_stats(m, &a);
        a.B = b->S; a.T = b->T; a.I = I; a.O = O; a.KX = m->KX; a.x_ring = x_ring;
        a.flags = flags & APE_FLAG_NORMALIZE_INPUT;
        e = ape_launch_lstm_tile16(H, 1, a, (hipStream_t)stream);
        if (e != hipSuccess) return ape_fail(APE_ERR_HIP, "streams_step: layer-0 launch failed: %s", hipGetErrorString(e));
        }
        // launch B: the layers above as an LSTM of their own over the S x n_mc sample rows; row r reads stream
        // r / n_mc's sequence under its own Philox mask (the counters of a fused launch over the same rows)
        if (route == BANK_UPPER32 || route == BANK_UPPER128) {
            // weight-stationary forms, per chunk of sample rows: the masked input in fragment order, the persistent cluster kernel, the head reduce
            const long long total = (long long)b->S * b->n_mc;
            const bool a_frag = a_form == BANK_A_SEQ32;          // (launch A left its sequence in fragment order: lstm_upper32.hip only)
            for (long long r0 = 0; r0 < total; r0 += b->plan.chunk_rows) {
                const int rows = (int)((total - r0 < b->plan.chunk_rows) ? total - r0 : b->plan.chunk_rows);
                ExpandParams xq{};
                xq.hseq = a_frag ? b->hfrag : m->hseq_ws; xq.hseq_frag = a_frag ? 1 : 0;
                xq.xfrag = b->xfrag; xq.row_base = r0; xq.rows = rows; xq.T = b->T; xq.n_mc = b->n_mc;
                xq.layer = 0; xq.dropout_p = b->dropout_p; xq.seed = b->seed + b->mc_calls;
                xq.masks = b->inj_masks; xq.masks_rows = total;      // (test hooks: the caller's masks for every mask layer)
                const ProfPair ev = prof_pair(b);       // (handed into the launch: recorded around the cluster kernel alone)
                if (route == BANK_UPPER32) {
                    UpperParams u = upper_params(m, b->T, (rows + 31) / 32, diag_wt);
                    u.xfrag = b->xfrag; u.xfrag_bytes = ape_upper32_xfrag_bytes(rows, b->T); u.ypart = b->ypart;
                    u.w = m->wcl32[1]; u.bias = m->bias[1];
#ifdef APE_ABLATE
                    // timing experiments of the ablation library only (tests/tools/ablate_upper32.py; results are garbage)
                    if (const char* ab = getenv("APE_UP32_ABLATE")) u.flags = (unsigned)strtoul(ab, nullptr, 0);
#endif
                    m->last_kernel = "ape_lstm_upper32";
                    e = ape_launch_lstm_upper32(u, xq, m->b_out, b->y_new + (size_t)r0 * O, m->caps.f16v2_capacity, (hipStream_t)stream, ev.a, ev.z);
                } else {
                    // the 3 x 128 model: layers 1 and 2 on the four-member clusters of lstm_upper128.hip, with layer 1's keep bits
                    Upper128Params u = upper_params<Upper128Params>(m, b->T, (rows + 31) / 32, diag_wt);
                    u.xfrag = b->xfrag; u.xfrag_bytes = ape_upper128_xfrag_bytes(rows, b->T); u.maskbits = b->maskbits; u.ypart = b->ypart;
                    u.w[0] = m->wup128[1]; u.w[1] = m->wup128[2]; u.bias[0] = m->bias[1]; u.bias[1] = m->bias[2]; u.dropout_p = b->dropout_p;
                    m->last_kernel = "ape_lstm_upper128";
                    e = ape_launch_lstm_upper128(u, xq, m->b_out, b->y_new + (size_t)r0 * O, m->caps.up128_classes, (hipStream_t)stream, ev.a, ev.z);
                }
                if (e != hipSuccess) return ape_fail(APE_ERR_HIP, "streams_step: upper-layer cluster launch failed: %s", hipGetErrorString(e));
            }
        } else {
        if (b->inj_masks) return ape_fail(APE_ERR_UNSUPPORTED, "streams_step: injected masks (test hook) on the batch-tile shared-layer-0 route");
        LstmParams q{};
        const int LU = m->dims.num_layers - 1;
        q.x = m->hseq_ws; q.y = b->y_new;
        for (int j = 0; j < LU; ++j) { q.wpack[j] = m->wpack[j + 1]; q.bias[j] = m->bias[j + 1]; }
        q.w_out = m->w_out; q.b_out = m->b_out;
        q.B = b->S * b->n_mc; q.T = b->T; q.I = H; q.O = O; q.KX = H; q.x_ring = 0;
        q.flags = APE_FLAG_DROPOUT_PHILOX; q.dropout_p = b->dropout_p; q.seed = b->seed + b->mc_calls;
        q.x_group = b->n_mc; q.layer_base = 1;
        m->last_kernel = "ape_lstm_tile16";
        const int rc = profiled(b, stream, [&] {
            e = ape_launch_lstm_tile16(H, LU, q, (hipStream_t)stream);
            return e == hipSuccess ? APE_OK : ape_fail(APE_ERR_HIP, "streams_step: upper-layer launch failed: %s", hipGetErrorString(e));
        });
        if (rc != APE_OK) return rc;
        }
    } else if (bank_on_mc_small(b)) {
        // a few streams in Monte-Carlo mode (one estimator's frame: S = 1): the latency kernel reads the first copy of every
        // stream's window and deals the sample rows over the XCDs; from ape_streams_frame_host the feature builder rides in the same
        // launch as extra workgroups (`fuse`: the row has NOT been pushed by a launch of its own)
        if (!m->has_weights) return ape_fail(APE_ERR_NOT_READY, "streams_step: weights not loaded");
        McFrameParts fr{};
        if (fuse) fr = *fuse;
        const int rc = profiled(b, stream, [&] {
            return mc_small_launch(m, b->xring, (size_t)b->n_mc * b->T * m->dims.input_size, b->S, b->n_mc, b->T,
                                   flags | diag_wt | (b->inj_masks ? APE_FLAG_DROPOUT_MASKS : APE_FLAG_DROPOUT_PHILOX), b->inj_masks,
                                   b->dropout_p, b->seed + b->mc_calls, b->y_new, stream, x_ring, &fr);
        });
        if (rc != APE_OK) return rc;
    } else {
        const int rc = profiled(b, stream, [&] {
            return lstm_forward_impl(m, b->xring, b->S * b->n_mc, b->T,
                                     flags | diag_wt | (!drop ? 0u : b->inj_masks ? APE_FLAG_DROPOUT_MASKS : APE_FLAG_DROPOUT_PHILOX),
                                     drop ? b->inj_masks : nullptr, drop ? b->dropout_p : 0.0f, b->seed + b->mc_calls, b->y_new, stream, x_ring);
        });
        if (rc != APE_OK) return rc;
    }
    ++b->mc_calls;       // (every branch above enqueued one forward under seed + mc_calls)
    // the lockstep form: every stream at the bank's own stack slot (a subset frame's descriptors carry one per entry)
    StreamPostParams q = bank_post_params(b, b->y_new, b->S, norm, msg_dev, out_dtype, packed, hw);
    q.tail = tail_dev;
    q.pos = (int)(b->steps % b->smooth);
    q.cold = b->steps == 0 ? 1 : 0;
    b->last_post_form = ape_stream_post_form(q, q.part != nullptr && (!spread || b->post_spread != nullptr));
    const SpreadArgs spa{b->post_spread};
    // (per-stream smoothing lengths: the table forms, with the count itself -- n mod k differs from stream to stream; a re-issued step
    //  comes through here with b->steps set back, and reads the bank's table like any frame)
    hipError_t e = bank_smooths_on(b) ? ape_launch_stream_post_smooths(q, SmoothArgs{b->smooths.dev, (unsigned long long)b->steps}, spread ? &spa : nullptr,
                                                                       b->last_post_form, (hipStream_t)stream, b->bodies.dev)
                   : spread       ? ape_launch_stream_post_spread(q, spa, b->last_post_form, (hipStream_t)stream, b->bodies.dev)
                                  : ape_launch_stream_post(q, (hipStream_t)stream, b->bodies.dev);      // (table mode: row s for stream s, q.body unread)
    if (e != hipSuccess) return ape_fail(APE_ERR_HIP, "streams_step launch failed: %s", hipGetErrorString(e));
    ++b->steps;
    journal_add(m, je);
    return APE_OK;
}

int ape_streams_step(ape_streams_t* b, uint32_t flags, void* msg_dev, void* tail_dev, int32_t out_dtype, void* stream) {
    return streams_step_impl(b, flags, msg_dev, tail_dev, out_dtype, stream);
}

// ---- the tail both host frames share (ape_host.h) -------------------------------------------------------------------------------------
int host_frame_wait(ape_streams* b, hipStream_t st, const unsigned* done, int n, unsigned done_val, HostFrameTail* t) {
    t->t_launched = now_us();
    // (a frame is tens of microseconds; a launch that gives up takes seconds: the stream wait below covers it)
    const bool seen = done != nullptr && ape_done_wait(done, n, done_val);
    t->fell_through = !seen && done != nullptr;
    if (!seen) APE_TRY(hipStreamSynchronize(st));
    t->aborted = *(volatile unsigned*)b->h_status != 0u;
    if (t->aborted) APE_TRY(hipStreamSynchronize(st));
    return APE_OK;
}

int host_frame_finish(ape_streams* b, const HostFrameTail& t, void* out_host, size_t out_bytes) {
    ape_model* m = b->model;
    // aborted: the regressor launch gave up (bounded spins).  The frame is still the bank's newest one, so the journal issues it again on
    // the kernels that need no co-residency -- into the same pinned rows.  Else: the status word was read behind the frame's kernels on
    // the frame's own stream and one handle serialises on one stream -- nothing aborted since the last check, what the journal holds is done
    if (t.aborted) {
        if (int rc = ape_model_recover(m)) return rc;
    } else {
        journal_clear(m);
    }
    const double t_there = now_us();
    memcpy(out_host, b->h_out, out_bytes);
    const double t_end = now_us();
    if (b->fs_trace.empty()) b->fs_trace.resize(4096 * 3, 0.0f);
    float* tr = b->fs_trace.data() + (b->fs_frames % 4096) * 3;
    tr[0] = (float)(t.t_launched - t.t_begin); tr[1] = (float)(t_there - t.t_launched); tr[2] = (float)(t_end - t_there);
    b->fs_frames += 1;
    b->fs_fallback += t.fell_through ? 1 : 0;
    b->fs_recovered += t.aborted ? 1 : 0;
    return APE_OK;
}

// One iteration of Estimator.processing_loop (estimator.py:174-177) for every stream of the bank, HOST buffers in and out.
// The raw rows are copied into pinned, device-visible staging the feature builder reads directly; the post kernel writes the
// datagram rows and the model's status word straight into pinned host memory: the frame holds no copy command, just the
// step's kernels and one stream synchronisation.  An aborted cooperative launch is recovered here (ape_model_recover).
// The frame call polls words the device writes into pinned memory (h_done, h_status) and reads h_out without a stream synchronisation:
// the buffers are APE_PINNED (bank_host.h).
int ape_streams_frame_host(ape_streams_t* b, int32_t kind, const float* rows_host, uint32_t flags, void* out_host,
                           int32_t out_dtype, void* stream) {
    if (!b || !rows_host || !out_host) return ape_fail(APE_ERR_INVALID_ARG, "streams_frame_host: NULL argument");
    if (b->per_stream) return ape_fail(APE_ERR_NOT_READY, "streams_frame_host: the bank is in per-stream mode (subset frames); ape_streams_reset first");
    if (out_dtype != APE_F32 && out_dtype != APE_F64) return ape_fail(APE_ERR_INVALID_ARG, "streams_frame_host: unknown dtype selector");
    if (flags & ~(uint32_t)(APE_FLAG_NORMALIZE_INPUT | APE_FLAG_SPREAD))
        return ape_fail(APE_ERR_INVALID_ARG, "streams_frame_host: only NORMALIZE_INPUT and SPREAD are accepted");
    int width, I;
    if (!parse_kind_dims(kind & ~APE_PARSE_BIG_ENDIAN, &width, &I)) return ape_fail(APE_ERR_INVALID_ARG, "streams_frame_host: unknown kind %d", kind);
    ape_model* m = b->model;
    APE_TRY(hipSetDevice(m->dims.device));           // (the consumer thread of an estimator starts on device 0)
    const size_t N = (size_t)b->smooth * b->n_mc;
    const size_t rows_bytes = (size_t)b->S * width * sizeof(float);
    const size_t out_bytes = (size_t)b->S * (25 + 6 * N + ((flags & APE_FLAG_SPREAD) ? APE_SPREAD_WIDTH : 0)) *
                             (out_dtype == APE_F64 ? sizeof(double) : sizeof(float));
    APE_TRY(ape_pinned_grow((void**)&b->h_rows, &b->h_rows_bytes, rows_bytes));
    APE_TRY(ape_pinned_grow(&b->h_out, &b->h_out_bytes, out_bytes));
    APE_TRY(ape_pinned_zeroed(&b->h_status, 64));
    // up to 64 streams: a word per stream that the post kernel's workgroup writes behind its outputs -- the host takes the frame when
    // all are there instead of waiting for the stream's completion signal to travel (a larger bank waits for the stream)
    if (b->S <= 64) APE_TRY(ape_pinned_zeroed(&b->h_done, 64 * sizeof(unsigned)));
    ape_done_next(&b->h_done_val);
    HostFrameTail t;
    t.t_begin = now_us();
    memcpy(b->h_rows, rows_host, rows_bytes);
    // (a sentinel, not zero: in the single-launch frame an aborted launch never reaches the tail that writes the word)
    *b->h_status = m->caps.cluster_ok ? 0xFFFFFFFFu : 0u;       // (no cooperative kernel on this model: nothing writes the word, nothing can abort)
    // where the bank steps on the Monte-Carlo latency kernel its extra workgroups build the rows' features (two launches per frame);
    // else the feature builder's own launch in front of the step
    const bool one_launch = bank_on_mc_small(b) && b->inj_masks == nullptr && mc_small_builder_fits(m, b->S, b->n_mc, b->T) && I == m->dims.input_size && b->xring != nullptr;
    float* slot_out; int slot_rep; size_t slot_rep_stride;
    next_slot(b, (size_t)I, &slot_out, &slot_rep, &slot_rep_stride);
    const HostFrameWords hw{b->h_status, b->h_done, b->h_done_val, "streams_frame_host"};
    if (one_launch) {
        McFrameParts fr{};
        fr.raw_rows = b->h_rows; fr.raw_width = width; fr.raw_kind = kind & ~APE_PARSE_BIG_ENDIAN; fr.raw_big_endian = (kind & APE_PARSE_BIG_ENDIAN) ? 1 : 0;
        fr.cold = b->frames == 0 ? 1 : 0;
        fr.ring_out = slot_out; fr.ring_stream_stride = (size_t)bank_copies(b) * b->T * I; fr.ring_rep_stride = slot_rep_stride; fr.ring_rep = slot_rep;
        ++b->frames;                                   // (what ape_streams_push_rows does behind its launch)
        if (int rc = streams_step_impl(b, flags | APE_FLAG_PACKED_MSG, b->h_out, nullptr, out_dtype, stream, hw, &fr)) { --b->frames; return rc; }
    } else {
        if (int rc = ape_streams_push_rows(b, kind, b->h_rows, stream)) return rc;
        if (int rc = streams_step_impl(b, flags | APE_FLAG_PACKED_MSG, b->h_out, nullptr, out_dtype, stream, hw)) return rc;
    }
    if (int rc = host_frame_wait(b, (hipStream_t)stream, b->h_done, b->S, b->h_done_val, &t)) return rc;
    if (t.aborted && one_launch) {
        // single-launch frame: the builder workgroup may not have run; its row goes into the ring by the feature builder's own kernel
        // in front of the re-issued step -- the same slot, the same values
        hipError_t e = ape_launch_parse_rows(b->h_rows, b->S, width, kind & ~APE_PARSE_BIG_ENDIAN, slot_out, APE_F32, I, (size_t)bank_copies(b) * b->T * I,
                                             slot_rep, slot_rep_stride, (kind & APE_PARSE_BIG_ENDIAN) ? 1 : 0, (hipStream_t)stream);
        if (e != hipSuccess) return ape_fail(APE_ERR_HIP, "streams_frame_host: feature builder launch failed: %s", hipGetErrorString(e));
    }
    return host_frame_finish(b, t, out_host, out_bytes);
}

int ape_streams_last_post_form(ape_streams_t* b, int32_t* form) {
    if (!b || !form) return ape_fail(APE_ERR_INVALID_ARG, "streams_last_post_form: NULL argument");
    *form = b->last_post_form;
    return APE_OK;
}

int ape_streams_frame_stats(ape_streams_t* b, ape_frame_stats_t* out, float* trace_us, int32_t capacity_frames, int32_t* n_out, int32_t reset) {
    if (!b || !out) return ape_fail(APE_ERR_INVALID_ARG, "streams_frame_stats: NULL argument");
    out->frames = b->fs_frames; out->fallback_syncs = b->fs_fallback; out->recovered = b->fs_recovered;
    int32_t n = 0;
    if (trace_us && capacity_frames > 0 && !b->fs_trace.empty()) {
        const uint64_t have = b->fs_frames < 4096 ? b->fs_frames : 4096;
        n = (int32_t)(have < (uint64_t)capacity_frames ? have : (uint64_t)capacity_frames);
        for (int32_t i = 0; i < n; ++i) {
            const uint64_t frame = b->fs_frames - (uint64_t)n + (uint64_t)i;
            memcpy(trace_us + 3 * (size_t)i, b->fs_trace.data() + (frame % 4096) * 3, 3 * sizeof(float));
        }
    }
    if (n_out) *n_out = n;
    if (reset) { b->fs_frames = b->fs_fallback = b->fs_recovered = 0; }
    return APE_OK;
}

int ape_streams_profile(ape_streams_t* b, int32_t enable) {
    if (!b) return ape_fail(APE_ERR_INVALID_ARG, "streams_profile: NULL bank");
    APE_TRY(hipSetDevice(b->model->dims.device));
    if (enable && b->prof_ev.empty()) {
        b->prof_ev.resize(512, nullptr);
        for (auto& ev : b->prof_ev) APE_TRY(hipEventCreate(&ev));
    }
    b->prof_on = enable != 0;
    b->prof_n = 0;
    return APE_OK;
}

int ape_streams_profile_read(ape_streams_t* b, double* kernel_ms_sum, int32_t* launches) {
    if (!b || !kernel_ms_sum || !launches) return ape_fail(APE_ERR_INVALID_ARG, "streams_profile_read: NULL argument");
    double sum = 0.0;
    for (int i = 0; i < b->prof_n; ++i) {
        APE_TRY(hipEventSynchronize(b->prof_ev[2 * i + 1]));
        float ms = 0.0f;
        APE_TRY(hipEventElapsedTime(&ms, b->prof_ev[2 * i], b->prof_ev[2 * i + 1]));
        sum += ms;
    }
    *kernel_ms_sum = sum; *launches = b->prof_n;
    b->prof_n = 0;
    return APE_OK;
}

