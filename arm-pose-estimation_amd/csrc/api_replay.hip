// Offline replay (ape_replay*) and replay_entry, the journal's re-issue of one call behind an aborted launch.
#include <cstring>
#include <vector>

#include "ape_host.h"

// ---- offline replay: every frame of one or more recordings in one call --------------------------------------
// Chunks of sample rows [r0, r0 + R): windows (replay.hip) -> regressor (lstm_forward_impl with the chunk's global row base, so that the
// Philox masks are those of ONE call over all F * n_mc rows) -> FK with de-normalisation into f64 est rows -> the messages of every frame
// whose rows are all there.  The est buffer of a chunk starts with the last `carry` rows of the one before (two buffers, ping-pong): the
// stacks of the chunk's first frames reach back into them.
#ifndef APE_REPLAY_WINDOW_BYTES
#define APE_REPLAY_WINDOW_BYTES (64ll << 20)      // default bound of a chunk's window image
#endif

struct ApeDeviceScratch {                         // the call's device workspaces, freed on every way out
    std::vector<void*> bufs;
    ~ApeDeviceScratch() { for (void* b : bufs) (void)hipFree(b); }
    hipError_t alloc(void** out, size_t bytes) {
        *out = nullptr;
        hipError_t e = hipMalloc(out, bytes > 0 ? bytes : 1);
        if (e == hipSuccess) bufs.push_back(*out);
        return e;
    }
};

// ape_replay_resume's extra arguments; nullptr for the entries that start cold and keep no state
struct ApeReplayResume {
    const void* state_in; const uint8_t* warm_in; void* state_out; uint8_t* warm_out; uint64_t sample_row_base;
};

// bodies_host [R,9]: recording r's rows as a fresh estimator BUILT WITH recording r's bonemap returns them (estimator.py:57-68); NULL: the
// model's body for every recording, on the kernels ape_replay always ran
static int replay_impl(ape_model_t* m, int32_t kind, const float* rows_dev, int32_t F, const int32_t* seg_starts_host, int32_t R,
                       int32_t seq_len, int32_t smooth, int32_t n_mc, float dropout_p, uint64_t seed, uint32_t flags,
                       void* out_dev, int32_t out_dtype, float* y_dev, int32_t max_rows_per_launch, void* stream, const double* bodies_host,
                       bool any_regressor, const ApeReplayResume* rs = nullptr) {
    // the arguments on their own first (no device needed to refuse them)
    if (!rows_dev || !out_dev) return ape_fail(APE_ERR_INVALID_ARG, "replay: NULL argument");
    int width, I;
    const int big_endian = (kind & APE_PARSE_BIG_ENDIAN) ? 1 : 0;
    if (!parse_kind_dims(kind & ~APE_PARSE_BIG_ENDIAN, &width, &I)) return ape_fail(APE_ERR_INVALID_ARG, "replay: unknown kind %d", kind);
    if (int rc = ape_check_segments("replay", F, seg_starts_host, R)) return rc;
    if (seq_len < 1) return ape_fail(APE_ERR_INVALID_ARG, "replay: seq_len=%d must be >= 1", seq_len);
    if (smooth < 1 || smooth > 64) return ape_fail(APE_ERR_UNSUPPORTED, "replay: smooth %d outside 1..64", smooth);
    if (n_mc < 1 || (long long)n_mc * smooth > 4096)
        return ape_fail(APE_ERR_INVALID_ARG, "replay: n_mc=%d with smooth=%d (1 <= smooth*n_mc <= 4096)", n_mc, smooth);
    if ((long long)F * n_mc >= (1ll << 31)) return ape_fail(APE_ERR_UNSUPPORTED, "replay: F*n_mc = %lld sample rows (< 2^31)", (long long)F * n_mc);
    if (!(dropout_p >= 0.0f && dropout_p < 1.0f)) return ape_fail(APE_ERR_INVALID_ARG, "replay: dropout_p %g outside [0,1)", (double)dropout_p);
    if (flags & ~(uint32_t)(APE_FLAG_NORMALIZE_INPUT | APE_FLAG_PACKED_MSG | APE_FLAG_SPREAD))
        return ape_fail(APE_ERR_INVALID_ARG, "replay: only NORMALIZE_INPUT, PACKED_MSG and SPREAD are accepted");
    if (out_dtype != APE_F32 && out_dtype != APE_F64) return ape_fail(APE_ERR_INVALID_ARG, "replay: unknown dtype selector");
    if (max_rows_per_launch < 0 || (max_rows_per_launch > 0 && max_rows_per_launch < 16))
        return ape_fail(APE_ERR_INVALID_ARG, "replay: max_rows_per_launch=%d (0 = default, else >= 16)", max_rows_per_launch);
    const bool carry_in = rs && rs->state_in, keep_out = rs && rs->state_out;
    const long long pbase = rs ? (long long)rs->sample_row_base : 0;
    if (carry_in && !rs->warm_in) return ape_fail(APE_ERR_INVALID_ARG, "replay_resume: state_in without warm_in");
    if (keep_out && !rs->warm_out) return ape_fail(APE_ERR_INVALID_ARG, "replay_resume: state_out without warm_out");
    if (rs && (((uintptr_t)rs->state_in | (uintptr_t)rs->state_out) & 15u) != 0)
        return ape_fail(APE_ERR_INVALID_ARG, "replay_resume: state buffers must be 16-byte aligned");
    if (pbase < 0 || pbase + (long long)F * n_mc >= (1ll << 31))
        return ape_fail(APE_ERR_INVALID_ARG, "replay_resume: sample_row_base %lld (base + F*n_mc < 2^31)", pbase);
    if (!m) return ape_fail(ape_device_count() == 0 ? APE_ERR_NO_DEVICE : APE_ERR_INVALID_ARG,
                        "replay: NULL model (no gfx950 device: there is no CPU fallback)");
    // ... then against the model
    if (m->dims.model_kind != APE_MODEL_LSTM && !any_regressor)
        return ape_fail(APE_ERR_UNSUPPORTED, "replay: LSTM estimator models only (not FF / ImuPose: ape_replay_regressor serves those)");
    const bool is_ff = m->dims.model_kind == APE_MODEL_FF, is_imu = m->dims.model_kind == APE_MODEL_IMUPOSE;
    if (is_imu) { n_mc = 1; dropout_p = 0.0f; }            // the reference ignores the sample count and has no dropout mode
    if (m->dims.target_layout == APE_LAYOUT_NONE) return ape_fail(APE_ERR_INVALID_ARG, "replay: model has no target layout");
    if (m->precision != APE_PRECISION_F32) return ape_fail(APE_ERR_UNSUPPORTED, "replay: fp16 precision is set on the model (float32 only)");
    if (I != m->dims.input_size)
        return ape_fail(APE_ERR_INVALID_ARG, "replay: kind %d builds %d features, the model takes %d", kind & ~APE_PARSE_BIG_ENDIAN, I, m->dims.input_size);
    if (!m->has_weights) return ape_fail(APE_ERR_NOT_READY, "replay: weights not loaded");
    const bool norm = (flags & APE_FLAG_NORMALIZE_INPUT) != 0;
    if (norm && !m->has_stats) return ape_fail(APE_ERR_NOT_READY, "replay: NORMALIZE_INPUT without norm stats");
    // (the LSTM kernels draw their masks per group of 4 rows; without dropout the base is not read)
    if (dropout_p > 0.0f && m->dims.num_layers > 1 && !is_ff && pbase % 4 != 0)
        return ape_fail(APE_ERR_INVALID_ARG, "replay_resume: sample_row_base %lld must be a multiple of 4 with dropout on", pbase);
    APE_TRY(hipSetDevice(m->dims.device));
    if (int rc = ape_check_not_capturing((hipStream_t)stream, "replay", nullptr)) return rc;
    // what was issued on the handle before is healthy (and off the journal) before the replay's launches follow it
    if (int rc = ape_model_recover(m)) return rc;

    const hipStream_t st = (hipStream_t)stream;
    const int T = is_ff ? 1 : seq_len, O = m->dims.output_size, W = layout_est_width(m->dims.target_layout);   // (DropoutFF: the newest row alone counts)
    const int N = smooth * n_mc;
    const long long total = (long long)F * n_mc;
    const bool tail = (flags & APE_FLAG_PACKED_MSG) && N > 1;
    const bool spread = (flags & APE_FLAG_SPREAD) != 0;     // the record in the last APE_SPREAD_WIDTH columns of every row
    const long long out_stride = (tail ? 25 + 6ll * N : 25) + (spread ? APE_SPREAD_WIDTH : 0);
    // sample rows per chunk: a multiple of 16 (the cluster kernels' row base), the window image bounded
    long long rmax = max_rows_per_launch > 0 ? max_rows_per_launch : APE_REPLAY_WINDOW_BYTES / ((long long)T * I * sizeof(float));
    rmax = rmax / 16 * 16;
    if (rmax < 16) rmax = 16;
    if (rmax > (total + 15) / 16 * 16) rmax = (total + 15) / 16 * 16;
    const long long carry = N;                    // >= (smooth - 1) * n_mc rows of older frames + the newest frame's first n_mc - 1
    ApeDeviceScratch ws;
    float *xx, *xw = nullptr, *yws = nullptr, *ffhid = nullptr;
    int *starts_d, *seg_of;
    double* est[2];
    APE_TRY(ws.alloc((void**)&xx, (size_t)F * I * sizeof(float)));
    APE_TRY(ws.alloc((void**)&seg_of, (size_t)F * sizeof(int)));
    APE_TRY(ws.alloc((void**)&starts_d, (size_t)R * sizeof(int)));
    if (!is_ff) APE_TRY(ws.alloc((void**)&xw, (size_t)rmax * T * I * sizeof(float)));
    else APE_TRY(ws.alloc((void**)&ffhid, (size_t)(rmax / n_mc + 2) * m->dims.hidden_size * sizeof(float)));
    if (!y_dev) APE_TRY(ws.alloc((void**)&yws, (size_t)rmax * O * sizeof(float)));
    APE_TRY(ws.alloc((void**)&est[0], (size_t)(carry + rmax) * W * sizeof(double)));
    APE_TRY(ws.alloc((void**)&est[1], (size_t)(carry + rmax) * W * sizeof(double)));
    APE_TRY(hipMemcpyAsync(starts_d, seg_starts_host, (size_t)R * sizeof(int), hipMemcpyHostToDevice, st));
    double* bodies_d = nullptr;                   // one body per recording: the values and every frame's recording index
    int* rec_of = nullptr;
    if (bodies_host) {
        APE_TRY(ws.alloc((void**)&bodies_d, (size_t)R * 9 * sizeof(double)));
        APE_TRY(ws.alloc((void**)&rec_of, (size_t)F * sizeof(int)));
        APE_TRY(hipMemcpyAsync(bodies_d, bodies_host, (size_t)R * 9 * sizeof(double), hipMemcpyHostToDevice, st));
    }

    // resumable replay: the carried-in records' stacks as est rows (once per call), the whole call's targets for the records going out
    const int x_words = T * I, stack_words = smooth * n_mc * O, words = (x_words + stack_words + 3) & ~3;
    ReplayCarryParams cp{};
    float* y_in = nullptr;
    int* rec_carry = nullptr;
    unsigned char* warm_d = nullptr;
    std::vector<unsigned char> warm_h;
    std::vector<int> rec_carry_h;
    if (carry_in || keep_out) {
        if (!rec_of) APE_TRY(ws.alloc((void**)&rec_of, (size_t)F * sizeof(int)));
        if (keep_out && !y_dev) { APE_TRY(ws.alloc((void**)&y_dev, (size_t)total * O * sizeof(float))); yws = nullptr; }
    }
    if (carry_in) {
        double* est_in;
        APE_TRY(ws.alloc((void**)&est_in, (size_t)R * N * W * sizeof(double)));
        APE_TRY(ws.alloc((void**)&y_in, (size_t)R * stack_words * sizeof(float)));
        APE_TRY(ws.alloc((void**)&warm_d, (size_t)R));
        APE_TRY(ws.alloc((void**)&rec_carry, (size_t)R * smooth * sizeof(int)));
        warm_h.resize((size_t)R);
        for (int r = 0; r < R; ++r)       // (a stack without a window does not exist: as ape_streams_import)
            warm_h[r] = (rs->warm_in[r] & APE_STATE_WINDOW_WARM) ? (rs->warm_in[r] & (APE_STATE_WINDOW_WARM | APE_STATE_STACK_WARM)) : 0;
        rec_carry_h.resize((size_t)R * smooth);
        for (int r = 0; r < R; ++r) for (int j = 0; j < smooth; ++j) rec_carry_h[(size_t)r * smooth + j] = r;
        APE_TRY(hipMemcpyAsync(warm_d, warm_h.data(), (size_t)R, hipMemcpyHostToDevice, st));
        APE_TRY(hipMemcpyAsync(rec_carry, rec_carry_h.data(), (size_t)R * smooth * sizeof(int), hipMemcpyHostToDevice, st));
        cp.state_in = (const float*)rs->state_in; cp.est_in = est_in; cp.rec_of = rec_of; cp.warm = warm_d; cp.words = words;
    }
    const ReplayCarryParams* cin = carry_in ? &cp : nullptr;

    const bool drop = dropout_p > 0.0f && m->dims.num_layers > 1 && !is_ff;
    const uint32_t lflags = (norm ? APE_FLAG_NORMALIZE_INPUT : 0u) | (drop ? APE_FLAG_DROPOUT_PHILOX : 0u);
    auto pass = [&]() -> int {
        hipError_t e = ape_launch_parse_rows(rows_dev, F, width, kind & ~APE_PARSE_BIG_ENDIAN, xx, APE_F32, I, (size_t)I, 1, 0, big_endian, st);
        if (e == hipSuccess) e = ape_launch_replay_segments(starts_d, R, F, seg_of, st, rec_of);
        if (e != hipSuccess) return ape_fail(APE_ERR_HIP, "replay: feature launch failed: %s", hipGetErrorString(e));
        if (cin) {                        // the carried stacks through the same de-normalisation and FK as fresh rows, once
            e = ape_launch_replay_carry_rows(cp.state_in, R, words, x_words, stack_words, y_in, st);
            if (e != hipSuccess) return ape_fail(APE_ERR_HIP, "replay_resume: carry launch failed: %s", hipGetErrorString(e));
            const FkBodyRows fc{bodies_d, rec_carry, 0, n_mc};
            if (int rc = fk_impl(m, y_in, APE_F32, R * N, norm ? 1 : 0, const_cast<double*>(cp.est_in), APE_F64, stream, bodies_d ? &fc : nullptr))
                return rc;
        }
        long long prev_rows = 0;
        for (long long r0 = 0, c = 0; r0 < total; r0 += rmax, ++c) {
            const int rows = (int)(total - r0 < rmax ? total - r0 : rmax);
            float* y = y_dev ? y_dev + (size_t)r0 * O : yws;
            if (is_ff) {
                if (int rc = ff_bank_forward(m, xx + (size_t)(r0 / n_mc) * I, (size_t)I, r0, rows, n_mc, norm, nullptr, dropout_p, seed, ffhid, y, stream,
                                             nullptr, nullptr, pbase))
                    return rc;
            } else {
            ReplayWindowParams wp{};
            wp.xx = xx; wp.seg_of = seg_of; wp.xw = xw; wp.r0 = r0; wp.R = rows; wp.T = T; wp.I = I; wp.n_mc = n_mc;
            e = ape_launch_replay_windows(wp, st, cin);
            if (e != hipSuccess) return ape_fail(APE_ERR_HIP, "replay: window launch failed: %s", hipGetErrorString(e));
            if (int rc = lstm_forward_impl(m, xw, rows, T, lflags, nullptr, drop ? dropout_p : 0.0f, seed, y, stream, 0, nullptr, nullptr,
                                           nullptr, r0 + pbase))
                return rc;
            }
            double* cur = est[c & 1];
            if (c > 0)
                APE_TRY(hipMemcpyAsync(cur, est[(c + 1) & 1] + (size_t)prev_rows * W, (size_t)carry * W * sizeof(double),
                                       hipMemcpyDeviceToDevice, st));
            const FkBodyRows fb{bodies_d, rec_of, r0, n_mc};
            if (int rc = fk_impl(m, y, APE_F32, rows, norm ? 1 : 0, cur + (size_t)carry * W, APE_F64, stream, bodies_d ? &fb : nullptr)) return rc;
            ReplayMsgParams mp{};
            mp.est = cur; mp.est_base = r0 - carry; mp.seg_of = seg_of; mp.out = out_dev; mp.out_stride = out_stride;
            mp.f_lo = r0 / n_mc; mp.f_hi = (r0 + rows) / n_mc;
            memcpy(mp.body, m->body, sizeof(mp.body));
            mp.W = W; mp.layout = m->dims.target_layout; mp.smooth = smooth; mp.n_mc = n_mc; mp.out_dtype = out_dtype;
            e = ape_launch_replay_msg(mp, tail, st, bodies_d, bodies_d ? rec_of : nullptr, cin, spread);
            if (e != hipSuccess) return ape_fail(APE_ERR_HIP, "replay: message launch failed: %s", hipGetErrorString(e));
            prev_rows = rows;
        }
        if (keep_out) {
            ReplayStateOutParams sp{};
            sp.xx = xx; sp.y = y_dev; sp.starts = starts_d; sp.state_in = cin ? cp.state_in : nullptr; sp.warm = cin ? cp.warm : nullptr;
            sp.state_out = (float*)rs->state_out;
            sp.R = R; sp.F = F; sp.T = T; sp.I = I; sp.smooth = smooth; sp.n_mc = n_mc; sp.O = O; sp.words = words;
            e = ape_launch_replay_state_out(sp, st);
            if (e != hipSuccess) return ape_fail(APE_ERR_HIP, "replay_resume: state launch failed: %s", hipGetErrorString(e));
        }
        return APE_OK;
    };
    if (int rc = pass()) return rc;
    APE_TRY(hipStreamSynchronize(st));
    // blocking and healthy on return: a weight-stationary launch that gave up is run again on the kernels that need no co-residency
    int rc = check_and_reset(m);
    if (rc == APE_ERR_HIP) {
        m->stats_counts.aborted_checks += 1;
        m->replaying = true;
        rc = pass();
        m->replaying = false;
        if (rc != APE_OK) { m->stats_counts.lost_calls += 1; return rc; }
        APE_TRY(hipStreamSynchronize(st));
        m->stats_counts.reissued_calls += 1;
        rc = check_and_reset(m);
    }
    if (rc == APE_OK && keep_out)
        for (int r = 0; r < R; ++r) rs->warm_out[r] = (uint8_t)(APE_STATE_WINDOW_WARM | APE_STATE_STACK_WARM);   // every recording has a frame
    return rc;
}

int ape_replay(ape_model_t* m, int32_t kind, const float* rows_dev, int32_t F, const int32_t* seg_starts_host, int32_t R,
               int32_t seq_len, int32_t smooth, int32_t n_mc, float dropout_p, uint64_t seed, uint32_t flags,
               void* out_dev, int32_t out_dtype, float* y_dev, int32_t max_rows_per_launch, void* stream) {
    return ape_replay_bodies(m, kind, rows_dev, F, seg_starts_host, R, seq_len, smooth, n_mc, dropout_p, seed, flags, out_dev, out_dtype, y_dev,
                             max_rows_per_launch, stream, nullptr);
}

int ape_replay_bodies(ape_model_t* m, int32_t kind, const float* rows_dev, int32_t F, const int32_t* seg_starts_host, int32_t R,
                      int32_t seq_len, int32_t smooth, int32_t n_mc, float dropout_p, uint64_t seed, uint32_t flags,
                      void* out_dev, int32_t out_dtype, float* y_dev, int32_t max_rows_per_launch, void* stream, const double* bodies_host) {
    return replay_impl(m, kind, rows_dev, F, seg_starts_host, R, seq_len, smooth, n_mc, dropout_p, seed, flags, out_dev, out_dtype, y_dev,
                       max_rows_per_launch, stream, bodies_host, false);
}

// ape_replay_bodies for every regressor the loader dispatches: DropoutLSTM handles take the path above unchanged;
// DropoutFF: no windows at all -- the trunk over the frames' own rows, the n_mc masked heads (masks those of ONE pass over all F * n_mc
// rows, whatever the chunking); ImuPoseLSTM: one row per frame whatever n_mc says (nn_models.py:246-251), no dropout
int ape_replay_regressor(ape_model_t* m, int32_t kind, const float* rows_dev, int32_t F, const int32_t* seg_starts_host, int32_t R,
                         int32_t seq_len, int32_t smooth, int32_t n_mc, float dropout_p, uint64_t seed, uint32_t flags,
                         void* out_dev, int32_t out_dtype, float* y_dev, int32_t max_rows_per_launch, void* stream, const double* bodies_host) {
    return replay_impl(m, kind, rows_dev, F, seg_starts_host, R, seq_len, smooth, n_mc, dropout_p, seed, flags, out_dev, out_dtype, y_dev,
                       max_rows_per_launch, stream, bodies_host, true);
}

int ape_replay_resume(ape_model_t* m, int32_t kind, const float* rows_dev, int32_t F, const int32_t* seg_starts_host, int32_t R,
                      int32_t seq_len, int32_t smooth, int32_t n_mc, float dropout_p, uint64_t seed, uint32_t flags,
                      void* out_dev, int32_t out_dtype, float* y_dev, int32_t max_rows_per_launch, void* stream, const double* bodies_host,
                      const void* state_in_dev, const uint8_t* warm_in_host, void* state_out_dev, uint8_t* warm_out_host,
                      uint64_t sample_row_base) {
    const ApeReplayResume rs{state_in_dev, warm_in_host, state_out_dev, warm_out_host, sample_row_base};
    return replay_impl(m, kind, rows_dev, F, seg_starts_host, R, seq_len, smooth, n_mc, dropout_p, seed, flags, out_dev, out_dtype, y_dev,
                       max_rows_per_launch, stream, bodies_host, true, &rs);
}

// The hidden features of every frame of whole recordings: replay_impl's front half -- feature rows, every frame's
// recording, the windows of a chunk, each recording starting cold as ape_replay starts it -- then ape_lstm_features per chunk.  One row
// per frame, no dropout, no post-filter, no state in or out.  The batch-tile kernel cannot abort: one pass, then the wait.
int ape_replay_features(ape_model_t* m, int32_t kind, const float* rows_dev, int32_t F, const int32_t* seg_starts_host, int32_t R,
                        int32_t seq_len, uint32_t flags, float* h_dev, float* y_dev, int32_t max_rows_per_launch, void* stream) {
    if (!rows_dev || !h_dev) return ape_fail(APE_ERR_INVALID_ARG, "replay_features: NULL argument");
    int width, I;
    const int big_endian = (kind & APE_PARSE_BIG_ENDIAN) ? 1 : 0;
    if (!parse_kind_dims(kind & ~APE_PARSE_BIG_ENDIAN, &width, &I)) return ape_fail(APE_ERR_INVALID_ARG, "replay_features: unknown kind %d", kind);
    if (int rc = ape_check_segments("replay_features", F, seg_starts_host, R)) return rc;
    if (seq_len < 1) return ape_fail(APE_ERR_INVALID_ARG, "replay_features: seq_len=%d must be >= 1", seq_len);
    if (flags & ~(uint32_t)APE_FLAG_NORMALIZE_INPUT) return ape_fail(APE_ERR_INVALID_ARG, "replay_features: only NORMALIZE_INPUT is accepted");
    if (max_rows_per_launch < 0 || (max_rows_per_launch > 0 && max_rows_per_launch < 16))
        return ape_fail(APE_ERR_INVALID_ARG, "replay_features: max_rows_per_launch=%d (0 = default, else >= 16)", max_rows_per_launch);
    if (!m) return ape_fail(ape_device_count() == 0 ? APE_ERR_NO_DEVICE : APE_ERR_INVALID_ARG,
                        "replay_features: NULL model (no gfx950 device: there is no CPU fallback)");
    if (m->dims.model_kind != APE_MODEL_LSTM)
        return ape_fail(APE_ERR_UNSUPPORTED, "replay_features: DropoutLSTM handles only (not FF / ImuPose)");
    if (m->precision != APE_PRECISION_F32) return ape_fail(APE_ERR_UNSUPPORTED, "replay_features: fp16 precision is set on the model (float32 only)");
    if (I != m->dims.input_size)
        return ape_fail(APE_ERR_INVALID_ARG, "replay_features: kind %d builds %d features, the model takes %d", kind & ~APE_PARSE_BIG_ENDIAN, I,
                        m->dims.input_size);
    if (!m->has_weights) return ape_fail(APE_ERR_NOT_READY, "replay_features: weights not loaded");
    if ((flags & APE_FLAG_NORMALIZE_INPUT) && !m->has_stats) return ape_fail(APE_ERR_NOT_READY, "replay_features: NORMALIZE_INPUT without norm stats");
    APE_TRY(hipSetDevice(m->dims.device));
    if (int rc = ape_check_not_capturing((hipStream_t)stream, "replay_features", nullptr)) return rc;
    if (int rc = ape_model_recover(m)) return rc;

    const hipStream_t st = (hipStream_t)stream;
    const int T = seq_len, H = m->dims.hidden_size, O = m->dims.output_size;
    long long rmax = max_rows_per_launch > 0 ? max_rows_per_launch : APE_REPLAY_WINDOW_BYTES / ((long long)T * I * sizeof(float));
    rmax = rmax / 16 * 16;
    if (rmax < 16) rmax = 16;
    if (rmax > ((long long)F + 15) / 16 * 16) rmax = ((long long)F + 15) / 16 * 16;
    ApeDeviceScratch ws;
    float *xx, *xw;
    int *starts_d, *seg_of;
    APE_TRY(ws.alloc((void**)&xx, (size_t)F * I * sizeof(float)));
    APE_TRY(ws.alloc((void**)&seg_of, (size_t)F * sizeof(int)));
    APE_TRY(ws.alloc((void**)&starts_d, (size_t)R * sizeof(int)));
    APE_TRY(ws.alloc((void**)&xw, (size_t)rmax * T * I * sizeof(float)));
    APE_TRY(hipMemcpyAsync(starts_d, seg_starts_host, (size_t)R * sizeof(int), hipMemcpyHostToDevice, st));
    hipError_t e = ape_launch_parse_rows(rows_dev, F, width, kind & ~APE_PARSE_BIG_ENDIAN, xx, APE_F32, I, (size_t)I, 1, 0, big_endian, st);
    if (e == hipSuccess) e = ape_launch_replay_segments(starts_d, R, F, seg_of, st, nullptr);
    if (e != hipSuccess) return ape_fail(APE_ERR_HIP, "replay_features: feature launch failed: %s", hipGetErrorString(e));
    for (long long r0 = 0; r0 < F; r0 += rmax) {
        const int rows = (int)(F - r0 < rmax ? F - r0 : rmax);
        ReplayWindowParams wp{};
        wp.xx = xx; wp.seg_of = seg_of; wp.xw = xw; wp.r0 = r0; wp.R = rows; wp.T = T; wp.I = I; wp.n_mc = 1;
        e = ape_launch_replay_windows(wp, st, nullptr);
        if (e != hipSuccess) return ape_fail(APE_ERR_HIP, "replay_features: window launch failed: %s", hipGetErrorString(e));
        if (int rc = lstm_features_impl(m, xw, rows, T, flags, nullptr, 0.0f, 0, h_dev + (size_t)r0 * H, y_dev ? y_dev + (size_t)r0 * O : nullptr, stream))
            return rc;
    }
    APE_TRY(hipStreamSynchronize(st));
    return APE_OK;
}

// one journaled call again, on the kernels that need no co-residency (m->replaying is set)
int replay_entry(ape_model_t* m, const ApeJournalEntry& e) {
    switch (e.kind) {
        case ApeJournalEntry::FORWARD:
            return ape_lstm_forward(m, (const float*)e.in0, e.B, e.T, e.flags, (const float*)e.in1, e.dropout_p, e.seed, (float*)e.out0, e.stream);
        case ApeJournalEntry::FORWARD_HS:
            return ape_lstm_forward_hs(m, (const float*)e.in0, e.B, e.T, e.flags, nullptr, e.dropout_p, e.seed, (const float*)e.in1,
                                       (const float*)e.in2, (float*)e.out0, e.stream);
        case ApeJournalEntry::FEATURES:
            return ape_lstm_features(m, (const float*)e.in0, e.B, e.T, e.flags, (const float*)e.in1, e.dropout_p, e.seed, (float*)e.out0,
                                     (float*)e.out1, e.stream);
        case ApeJournalEntry::FK:
            return ape_fk(m, e.in0, e.i0, e.B, e.i1, e.out0, e.i2, e.stream);
        case ApeJournalEntry::MSG:
            return ape_msg_reduce(m, (const double*)e.in0, e.B, (double*)e.out0, e.stream);
        case ApeJournalEntry::INFER:
            return ape_infer(m, (const float*)e.in0, e.B, e.T, e.flags, (float*)e.out0, e.out1, e.i2, e.stream);
        case ApeJournalEntry::STEP: {
            ape_streams* b = e.bank;
            b->steps = e.bank_steps; b->mc_calls = e.bank_mc_calls;         // (frames unchanged: checked by the caller)
            return ape_streams_step(b, e.flags, e.out0, e.out1, e.i2, e.stream);
        }
        case ApeJournalEntry::SUBSET:        // regressor + post-filter again over the windows and descriptors the frame left behind
            return subset_regress_post(e.bank, e.B, e.flags, e.out0, e.i2, e.stream, e.bank_mc_calls);
    }
    return ape_fail(APE_ERR_INVALID_ARG, "recover: unknown journal entry");
}

