// The regressor dispatch behind the C ABI: what csrc/ape_plan.h planned for a call is executed here (lstm_forward_impl and its routes,
// ff_bank_forward), with the forward, forward-kinematics, reduce, parse and infer entries on top.
#include <algorithm>
#include <cstring>

#include "ape_host.h"

// the call's switches as the planner reads them
LstmCall lstm_call(const ape_model* m, int B, int T, uint32_t flags, bool have_hs, int x_ring) {
    LstmCall c;
    c.B = B; c.T = T;
    c.masks = (flags & APE_FLAG_DROPOUT_MASKS) != 0; c.philox = (flags & APE_FLAG_DROPOUT_PHILOX) != 0; c.drop = c.masks || c.philox;
    c.all_steps = (flags & APE_FLAG_ALL_STEPS) != 0; c.broadcast = (flags & APE_FLAG_BROADCAST_X) != 0; c.alt_form = (flags & APE_FLAG_ALT_FORM) != 0;
    c.have_hs = have_hs; c.x_ring = x_ring;
    c.kernel_choice = m->kernel_choice; c.precision = m->precision; c.replaying = m->replaying;
    c.c32_on = m->c32_on; c.small_batch_path = m->small_batch_path; c.f16_v2 = m->f16_v2;
    return c;
}

// the fields every launch of a cluster kernel shares, with `layers` of the weight image of `route` (PLAN_* of ape_plan.h; lstm_x / lstm_in:
// the LSTM's own input -- ImuPoseLSTM's is the 256-wide activation of its input layer).  No memset in the launch path: the kernels' last
// workgroup re-zeroes every polled word (self-cleaning)
ClusterParams cluster_params(const ape_model* m, int route, int layers, const float* x, float* y, int B, int T, uint32_t flags, int x_ring) {
    ClusterParams c{};
    const bool f16 = route == PLAN_F16 || route == PLAN_F16V2, small2 = route == PLAN_SMALL && !(flags & APE_FLAG_ALT_FORM) && m->small_uw == 2;
    c.x = x; c.y = y;
    for (int l = 0; l < layers; ++l) {
        const void* w = route == PLAN_C32 ? (const void*)m->wcl32s[l] : f16 ? m->wcl16[l] : small2 ? m->wcls[l] : m->wcl[l];
        c.wcl[l] = static_cast<const float*>(w); c.bias[l] = m->bias[l];
    }
    head_and_stats(m, &c);
    c.xx_r = m->stats + 2 * m->dims.input_size + 2 * m->dims.output_size;
    c.hx = m->hx; c.hx_bytes = m->hx_bytes;
    const CtlWords cw = ctl_words(m);
    c.xflags = m->xflags; c.status = cw.status; c.ticket = cw.ticket; c.done = cw.done;
    c.B = B; c.T = T; c.I = m->lstm_in; c.O = m->dims.output_size;
    c.flags = flags; c.x_ring = x_ring;
    c.xcc_slots = m->xcc_slots; c.dbg_wg = m->dbg_wg;
    return c;
}

static bool stream_capturing(void* stream) {
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    (void)hipStreamIsCapturing((hipStream_t)stream, &st);
    return st != hipStreamCaptureStatusNone;
}
// grow a device workspace to `need` elements of `elem_bytes`; a capturing stream cannot allocate: APE_ERR_CAPACITY with the message
// `what_fmt`, a format with exactly one %zu, which receives `need`
static int grow_ws(void* stream, void** ptr, size_t* cap, size_t need, size_t elem_bytes, const char* what_fmt) {
    if (need <= *cap) return APE_OK;
    if (stream_capturing(stream)) return ape_fail(APE_ERR_CAPACITY, what_fmt, need);
    if (*ptr) { APE_TRY(hipFree(*ptr)); *ptr = nullptr; *cap = 0; }
    APE_TRY(hipMalloc(ptr, need * elem_bytes));
    *cap = need;
    return APE_OK;
}
// Monte-Carlo latency kernel (lstm_mc_small.hip): n_streams windows (stream s at x + s * x_stream_stride) x n_mc dropout samples each,
// rows dealt over the 8 XCD clusters; y [n_streams * n_mc, O].  The caller has checked mc_small_fits().
int mc_small_launch(ape_model_t* m, const float* x, size_t x_stream_stride, int n_streams, int n_mc, int T, uint32_t flags,
                    const float* masks_dev, float dropout_p, uint64_t seed, float* y_dev, void* stream, int x_ring, const McFrameParts* fr) {
    McSmallParams q{};
    const int L = m->dims.num_layers, I = m->dims.input_size, O = m->dims.output_size;
    q.x = x; q.x_stream_stride = x_stream_stride; q.y = y_dev;
    q.w0 = m->wcls[0];
    for (int l = 0; l < L; ++l) { q.w[l] = m->wmc[l]; q.w16[l] = m->wmc16[l]; q.bias[l] = m->bias[l]; }
    head_and_stats(m, &q);
    q.xx_r = m->stats + 2 * I + 2 * O;
    q.gx = m->gxm + 256; q.gx_cluster_bytes = (unsigned)m->gxm_cluster_bytes;
    q.seq = reinterpret_cast<unsigned*>(m->gxm);
    q.status = ctl_words(m).status; q.done = ctl_words(m).done;
    q.xcc_slots = m->xcc_slots;
    q.masks = masks_dev;
    q.rows = n_streams * n_mc; q.n_mc = n_mc; q.n_streams = n_streams;
    q.cps = 8 / n_streams; q.R = (n_mc + q.cps - 1) / q.cps;
    q.T = T; q.I = I; q.O = O; q.x_ring = x_ring;
    q.flags = flags & (APE_FLAG_NORMALIZE_INPUT | APE_FLAG_DROPOUT_MASKS | APE_FLAG_DROPOUT_PHILOX | APE_FLAG_ANY_PLACEMENT);
    q.dropout_p = (flags & APE_FLAG_DROPOUT_PHILOX) ? dropout_p : 0.0f; q.seed = seed;
    q.dbg_wg = m->dbg_wg;
    q.xg = m->gxm + 256 + 8 * m->gxm_cluster_bytes;
    if (fr) {
        q.raw_rows = fr->raw_rows; q.raw_width = fr->raw_width; q.raw_kind = fr->raw_kind; q.raw_big_endian = fr->raw_big_endian;
        q.cold = fr->cold; q.ring_out = fr->ring_out; q.ring_stream_stride = fr->ring_stream_stride; q.ring_rep_stride = fr->ring_rep_stride;
        q.ring_rep = fr->ring_rep;
    }
    m->last_kernel = "ape_lstm_mc_small";
    hipError_t e = ape_launch_lstm_mc_small(m->dims.hidden_size, L, m->KX, q, (hipStream_t)stream);
    if (e != hipSuccess) return ape_fail(APE_ERR_HIP, "Monte-Carlo latency kernel launch failed: %s", hipGetErrorString(e));
    return APE_OK;
}

// ImuPoseLSTM on lstm_upper32.hip's persistent clusters (plan route PLAN_SPLIT32): z_ws holds the input layer's activations
static int split32_forward(ape_model_t* m, const LstmPlan& plan, int B, int T, uint32_t flags, float* y_dev, void* stream) {
    const int H = m->dims.hidden_size, chunk = plan.rows_per_launch;
    const int tiles_max = ((B < chunk ? B : chunk) + 31) / 32;
    if ((size_t)tiles_max > m->split_tiles_cap || (size_t)T > m->split_steps_cap) {
        if (stream_capturing(stream))
            return ape_fail(APE_ERR_CAPACITY, "lstm_forward: the layer workspaces (%d tiles x %d steps) cannot grow during stream capture", tiles_max, T);
        APE_TRY(hipStreamSynchronize((hipStream_t)stream));
        // (both dimensions only ever grow: a caller alternating between many short and few long windows does not reallocate)
        const size_t tc = std::max((size_t)tiles_max, m->split_tiles_cap), sc = std::max((size_t)T, m->split_steps_cap);
        m->split_tiles_cap = m->split_steps_cap = 0;
        void** const ws[3] = {(void**)&m->zfrag_ws, (void**)&m->hfrag_ws, (void**)&m->ypart_ws};
        const size_t bytes[3] = {tc * sc * 32768, tc * sc * 32768, ape_upper32_ypart_bytes((int)tc * 32)};
        for (void** w : ws) if (*w) { APE_TRY(hipFree(*w)); *w = nullptr; }
        for (int i = 0; i < 3; ++i) APE_TRY(hipMalloc(ws[i], bytes[i]));
        m->split_tiles_cap = tc; m->split_steps_cap = sc;
    }
    for (int b0 = 0; b0 < B; b0 += chunk) {
        const int nb = (B - b0 < chunk) ? B - b0 : chunk;
        const int tiles = (nb + 31) / 32;
        UpperParams u0 = upper_params(m, T, tiles, flags & APE_FLAG_ALT_FORM);      // (selector: one-tile clusters on the blocking form, for A/B)
        u0.xfrag = m->zfrag_ws; u0.xfrag_bytes = (size_t)tiles * T * 32768;
        u0.w = m->wcl32[0]; u0.bias = m->bias[0];
        u0.hseq = m->hfrag_ws; u0.hseq_bytes = (size_t)tiles * T * 32768;
        UpperParams u1 = u0;
        u1.xfrag = m->hfrag_ws; u1.hseq = nullptr; u1.hseq_bytes = 0;
        u1.w = m->wcl32[1]; u1.bias = m->bias[1]; u1.ypart = m->ypart_ws;
        m->last_kernel = plan.last_kernel;
        hipError_t e2 = ape_launch_lstm_split32(m->z_ws + (size_t)b0 * T * H, nb, u0, u1, m->b_out,
                                                y_dev + (size_t)b0 * m->dims.output_size, m->caps.f16v2_capacity, (hipStream_t)stream);
        if (e2 != hipSuccess) return ape_fail(APE_ERR_HIP, "layer-split lstm launch failed: %s", hipGetErrorString(e2));
    }
    return APE_OK;
}

// x_ring: time step t of every window lives in slot (t + x_ring) mod T (0 = the linear layout of the public entry)
int lstm_forward_impl(ape_model_t* m, const float* x_dev, int32_t B, int32_t T, uint32_t flags, const float* masks_dev, float dropout_p,
                      uint64_t seed, float* y_dev, void* stream, int x_ring, const float* h0_dev, const float* c0_dev, FkTail* fk,
                      long long row_base) {
    // row_base (DROPOUT_PHILOX, a multiple of 16): the global row of x_dev's row 0 when a caller serves one batch in several calls
    if (!m || !x_dev || !y_dev) return ape_fail(APE_ERR_INVALID_ARG, "lstm_forward: NULL argument");
    if (B < 1 || T < 1) return ape_fail(APE_ERR_INVALID_ARG, "lstm_forward: B=%d T=%d must be >= 1", B, T);
    flags &= ~(uint32_t)APE_FLAG_XCD_CLASSES;            // (the launcher's own bit)
#if !defined(APE_ABLATE) && !defined(APE_CLUSTER_STAMPS)
    // the product library knows the documented flags and the four exchange-form selectors of include/ape_hip.h; the timing-only
    // ablation bits (results are garbage) exist in the diagnostic builds alone
    if (flags & ~(uint32_t)(APE_FLAG_NORMALIZE_INPUT | APE_FLAG_ALL_STEPS | APE_FLAG_DROPOUT_MASKS | APE_FLAG_DROPOUT_PHILOX | APE_FLAG_BROADCAST_X |
                            APE_FLAG_ANY_PLACEMENT | APE_FLAG_IN_XCD_PLAIN | APE_FLAG_NO_XCD_CLASSES | APE_FLAG_ALT_FORM))
        return ape_fail(APE_ERR_INVALID_ARG, "lstm_forward: unknown flag bits 0x%x", flags);
#endif
    if (!m->has_weights) return ape_fail(APE_ERR_NOT_READY, "lstm_forward: weights not loaded");
    if ((flags & APE_FLAG_NORMALIZE_INPUT) && !m->has_stats)
        return ape_fail(APE_ERR_NOT_READY, "lstm_forward: NORMALIZE_INPUT without norm stats");
    if ((flags & APE_FLAG_DROPOUT_MASKS) && (flags & APE_FLAG_DROPOUT_PHILOX))
        return ape_fail(APE_ERR_INVALID_ARG, "lstm_forward: choose one dropout mode");
    if ((flags & APE_FLAG_DROPOUT_MASKS) && m->dims.num_layers > 1 && !masks_dev)
        return ape_fail(APE_ERR_INVALID_ARG, "lstm_forward: DROPOUT_MASKS without masks");
    if ((flags & APE_FLAG_DROPOUT_PHILOX) && !(dropout_p >= 0.0f && dropout_p < 1.0f))
        return ape_fail(APE_ERR_INVALID_ARG, "lstm_forward: dropout_p %f outside [0,1)", dropout_p);
    const int H = m->dims.hidden_size, L = m->dims.num_layers;
    const bool drop = (flags & (APE_FLAG_DROPOUT_MASKS | APE_FLAG_DROPOUT_PHILOX)) != 0;
    const bool have_hs = h0_dev != nullptr || c0_dev != nullptr;
    if (have_hs && (!h0_dev || !c0_dev)) return ape_fail(APE_ERR_INVALID_ARG, "lstm_forward: h0 and c0 come together");
    if (have_hs && m->dims.model_kind == APE_MODEL_FF)
        return ape_fail(APE_ERR_INVALID_ARG, "lstm_forward: the MLP regressor has no recurrent state");
    if (m->dims.model_kind == APE_MODEL_FF) {
        if (flags & APE_FLAG_BROADCAST_X) return ape_fail(APE_ERR_UNSUPPORTED, "lstm_forward: BROADCAST_X is an LSTM-path flag");
        if ((flags & APE_FLAG_DROPOUT_MASKS) && !masks_dev)
            return ape_fail(APE_ERR_INVALID_ARG, "lstm_forward: DROPOUT_MASKS without masks");
        MlpParams q{};
        const bool all = (flags & APE_FLAG_ALL_STEPS) != 0;
        q.x = x_dev; q.y = y_dev;
        for (int j = 0; j <= L; ++j) { q.wpack[j] = m->ff_wpack[j]; q.bias[j] = m->ff_bias[j]; }
        head_and_stats(m, &q);
        q.mask = masks_dev;
        q.row_stride = all ? (size_t)m->dims.input_size : (size_t)T * m->dims.input_size;
        q.row_offset = all ? 0 : (size_t)(T - 1) * m->dims.input_size;
        q.N = all ? B * T : B;
        q.I = m->dims.input_size; q.O = m->dims.output_size; q.KX = m->KX; q.n_hidden = L;
        q.flags = flags; q.dropout_p = dropout_p; q.seed = seed;
        q.neg_slope = 0.01f;                      // torch's leaky_relu default (nn_models.py:347,349)
        // chip-filling eval batches: the weight-stationary two-stage pipeline (mlp_pipe.hip)
        // (x and y each behind one 32-bit buffer descriptor whose span stays UNDER 2 GiB: the kernel's out-of-range
        //  sentinel for padded columns and spare lanes is the offset 0x80000000, which must lie outside num_records)
        const bool one_descriptor = ((size_t)(q.N - 1) * q.row_stride + q.row_offset + q.I) * sizeof(float) < 0x80000000ull &&
                                    (size_t)q.N * q.O * sizeof(float) < 0x80000000ull;
        if (m->ffp_ok && m->ffp_on && !m->replaying && !drop && q.hidden_out == nullptr && q.mask == nullptr && one_descriptor && q.N >= 64 * m->n_cus) {
            m->last_kernel = "ape_mlp_pipe";
            hipError_t e2 = ape_launch_mlp_pipe(q, m->ffp_wa0, m->ffp_wa1, m->ffp_wb2, m->ffp_wbo, m->ffp_ring, m->ffp_ring_bytes, m->ffp_ctl,
                                               m->n_cus, (hipStream_t)stream);
            if (e2 != hipSuccess) return ape_fail(APE_ERR_HIP, "mlp pipeline launch failed: %s", hipGetErrorString(e2));
            return APE_OK;
        }
        m->last_kernel = "ape_mlp_tile16";
        hipError_t e = ape_launch_mlp_tile16(H, q, (hipStream_t)stream, m->n_cus);
        if (e != hipSuccess) return ape_fail(APE_ERR_HIP, "mlp kernel launch failed: %s", hipGetErrorString(e));
        return APE_OK;
    }
    const float* lstm_x = x_dev;
    if (m->dims.model_kind == APE_MODEL_IMUPOSE) {
        // relu(input_layer(x)) for every row of every window (nn_models.py:242), then the LSTM reads those 256 columns
        if (drop) return ape_fail(APE_ERR_UNSUPPORTED, "lstm_forward: ImuPoseLSTM has no Monte-Carlo dropout mode "
                              "(its monte_carlo_predictions is the plain forward, nn_models.py:246-251)");
        const size_t rows = (size_t)((flags & APE_FLAG_BROADCAST_X) ? 1 : B) * T;
        if (int rc = grow_ws(stream, (void**)&m->z_ws, &m->z_cap, rows, H * sizeof(float),
                             "lstm_forward: %zu input-layer rows exceed the workspace during stream capture")) return rc;
        MlpParams q{};
        q.x = x_dev; q.y = nullptr; q.hidden_out = m->z_ws;
        q.wpack[0] = m->ff_wpack[0]; q.bias[0] = m->ff_bias[0];
        q.xx_m = m->stats; q.xx_s = m->stats + m->dims.input_size;
        q.row_stride = (size_t)m->dims.input_size; q.row_offset = 0;
        q.N = (int)rows; q.I = m->dims.input_size; q.O = m->dims.output_size; q.KX = m->KXpre; q.n_hidden = 0;
        q.flags = flags & APE_FLAG_NORMALIZE_INPUT; q.neg_slope = 0.0f;
        hipError_t e = ape_launch_mlp_tile16(H, q, (hipStream_t)stream, m->n_cus);
        if (e != hipSuccess) return ape_fail(APE_ERR_HIP, "input-layer kernel launch failed: %s", hipGetErrorString(e));
        lstm_x = m->z_ws;
        flags &= ~(uint32_t)APE_FLAG_NORMALIZE_INPUT;        // done in front of the input layer
    }
    // which kernels serve the call: csrc/ape_plan.h; from here on the plan is executed
    const LstmCall call = lstm_call(m, B, T, flags, have_hs, x_ring);
    const LstmPlan plan = plan_lstm(m->caps, m->dims, call);
    if (plan.route == PLAN_SPLIT32) return split32_forward(m, plan, B, T, flags, y_dev, stream);
    if (ape_lstm_tile16_smem_bytes(H, L, m->KX, m->dims.output_size, drop) > 160 * 1024)
        return ape_fail(APE_ERR_UNSUPPORTED, "lstm_forward: H=%d L=%d with dropout exceeds the 160 KiB LDS of a CU", H, L);
    if (plan.route == PLAN_UNSUPPORTED)        // (err == nullptr: the one message that names B)
        return plan.err ? ape_fail(plan.err_code, "%s", plan.err) : ape_fail(plan.err_code, "lstm_forward: injected masks with B=%d exceed one cluster launch", B);
    if (plan.route == PLAN_MC_SMALL)
        return mc_small_launch(m, x_dev, 0, 1, B, T, flags, masks_dev, dropout_p, seed, y_dev, stream, x_ring);
    if (plan.n16 > 0) {
        LstmParams p{};
        p.x = lstm_x; p.y = y_dev;
        for (int l = 0; l < L; ++l) { p.wpack[l] = m->wpack[l]; p.bias[l] = m->bias[l]; }
        head_and_stats(m, &p);
        p.masks = masks_dev; p.flags = flags; p.dropout_p = dropout_p; p.seed = seed;
        p.B = plan.n16; p.T = T; p.I = m->lstm_in; p.O = m->dims.output_size; p.KX = m->KX; p.x_ring = x_ring;
        p.h0 = h0_dev; p.c0 = c0_dev; p.hs_rows = B; p.row_base = row_base;
        m->last_kernel = "ape_lstm_tile16";
        hipError_t e = ape_launch_lstm_tile16(H, L, p, (hipStream_t)stream);
        if (e != hipSuccess) return ape_fail(APE_ERR_HIP, "lstm kernel launch failed: %s", hipGetErrorString(e));
        if (plan.n16 == B) return APE_OK;
    }
    // rows [n16, B) in launches of plan.rows_per_launch: each route brings its weight image, its exchange buffer and its launcher
    const bool all_steps = call.all_steps, small = plan.route == PLAN_SMALL;
    const int O = m->dims.output_size;
    if (all_steps)
        if (int rc = grow_ws(stream, (void**)&m->hseq_ws, &m->hseq_cap, (size_t)B * T, H * sizeof(float),
                             "lstm_forward: the all-steps workspace (%zu rows) cannot grow during stream capture")) return rc;
    const int small_uw = call.alt_form ? 4 : m->small_uw;
    m->last_kernel = plan.last_kernel;
    for (int b0 = plan.n16; b0 < B; b0 += plan.rows_per_launch) {
        const int nb = (B - b0 < plan.rows_per_launch) ? B - b0 : plan.rows_per_launch;
        const float* xb = call.broadcast ? lstm_x : lstm_x + (size_t)b0 * T * m->lstm_in;
        float* yb = y_dev + (size_t)b0 * O;
        ClusterParams c = cluster_params(m, plan.route, L, xb, yb, nb, T, flags, x_ring);
        hipError_t e = hipSuccess;
        const char* what = "cluster";
        switch (plan.route) {
            case PLAN_C32:
                for (int l = 0; l < L; ++l) { c.gate_scale[l] = m->c32_scale[l]; c.gate_descale[l] = m->c32_descale[l]; }
                e = ape_launch_lstm_cluster32(H, L, m->KX, (nb + 31) / 32, c, (hipStream_t)stream); what = "cluster32";
                break;
            case PLAN_C16:
                e = ape_launch_lstm_cluster16(H, L, m->KX, nb, c, (hipStream_t)stream); what = "cluster16";
                break;
            case PLAN_LV16:
                c.hx = reinterpret_cast<float*>(m->gx16 + 256); c.hx_bytes = m->gx16_bytes; c.seq = reinterpret_cast<unsigned*>(m->gx16);
                c.flags = (flags & ~APE_FLAG_LV16_SINGLE) | (plan.lv16_single ? APE_FLAG_LV16_SINGLE : 0u);
                e = ape_launch_lstm_level16(H, L, m->KX, nb, c, (hipStream_t)stream); what = "level16";
                break;
            case PLAN_F16V2:
                e = ape_launch_lstm_cluster_f16v2(H, L, m->KX, (nb + 31) / 32, c, (hipStream_t)stream, plan_f16v2_duo(m->caps, call, nb)); what = "fp16 cluster";
                break;
            default: {        // the first-generation kernel, its fp16 variant, the latency kernel
                if (all_steps) { c.y = nullptr; c.hseq = m->hseq_ws + (size_t)b0 * T * H; }
                if (small) { c.hx = reinterpret_cast<float*>(m->hxs + 256); c.hx_bytes = m->hxs_bytes; c.seq = reinterpret_cast<unsigned*>(m->hxs); }
                c.flags = flags & ~(uint32_t)APE_FLAG_ALL_STEPS;
                c.masks = masks_dev; c.dropout_p = dropout_p; c.seed = seed;
                if (small && fk != nullptr) {             // (B <= 4: one launch)
                    c.fk_est = fk->est; c.fk_est_dtype = fk->est_dtype;
                    if (fk->denormalize) {
                        c.fk_yy_m = m->stats + 2 * m->dims.input_size;
                        c.fk_yy_s = c.fk_yy_m + O;
                    }
                    memcpy(c.fk_body, m->body, sizeof(c.fk_body));
                    c.fk_layout = m->dims.target_layout; c.fk_W = layout_est_width(c.fk_layout);
                    fk->done = true;
                }
                c.row_base = (int)(row_base + b0);        // Philox counters over the call's global rows, whatever the split
                bool classes = false;
                const int clusters = xcd_class_clusters((nb + 16 * plan.nmt - 1) / (16 * plan.nmt), plan.capacity,
                                                        plan.xcd_classes && xcd_classes_on(m, flags), &classes);
                if (classes) c.flags |= APE_FLAG_XCD_CLASSES;
                e = small ? ape_launch_lstm_cluster_small(H, L, m->KX, B == 1 ? 1 : (B == 2 ? 2 : 4), small_uw, c, (hipStream_t)stream)
                    : plan.route == PLAN_F16 ? ape_launch_lstm_cluster_f16(H, L, m->KX, plan.nmt, clusters, c, (hipStream_t)stream)
                                             : ape_launch_lstm_cluster(H, L, m->KX, plan.nmt, plan.cdrop, clusters, c, (hipStream_t)stream);
            }
        }
        if (e != hipSuccess) return ape_fail(APE_ERR_HIP, "%s lstm launch failed: %s", what, hipGetErrorString(e));
    }
    if (all_steps) {
        hipError_t e = ape_launch_head_rows(m->hseq_ws, B * T, H, O, m->w_out, m->b_out, y_dev, (hipStream_t)stream);
        if (e != hipSuccess) return ape_fail(APE_ERR_HIP, "head kernel launch failed: %s", hipGetErrorString(e));
    }
    return APE_OK;
}

int ape_lstm_forward(ape_model_t* m, const float* x_dev, int32_t B, int32_t T, uint32_t flags,
                     const float* masks_dev, float dropout_p, uint64_t seed, float* y_dev, void* stream) {
    const int rc = lstm_forward_impl(m, x_dev, B, T, flags, masks_dev, dropout_p, seed, y_dev, stream, 0);
    if (rc == APE_OK) {
        ApeJournalEntry e{};
        e.kind = ApeJournalEntry::FORWARD; e.in0 = x_dev; e.in1 = masks_dev; e.out0 = y_dev; e.B = B; e.T = T; e.flags = flags;
        e.dropout_p = dropout_p; e.seed = seed; e.stream = stream;
        journal_add(m, e);
    }
    return rc;
}

// ape_lstm_features behind its journal entry (ape_replay_features runs it per chunk): every row on ape_lstm_tile16<H, L, 4, true>, whatever the
// planner would pick for (B, T) -- the kernel that has h^{L-1}_{T-1} in LDS at the head, is not cooperative and cannot abort
int lstm_features_impl(ape_model_t* m, const float* x_dev, int32_t B, int32_t T, uint32_t flags, const float* masks_dev, float dropout_p,
                       uint64_t seed, float* h_dev, float* y_dev, void* stream) {
    if (!m || !x_dev || !h_dev) return ape_fail(APE_ERR_INVALID_ARG, "lstm_features: NULL argument");
    if (B < 1 || T < 1) return ape_fail(APE_ERR_INVALID_ARG, "lstm_features: B=%d T=%d must be >= 1", B, T);
    if (flags & APE_FLAG_ALL_STEPS) return ape_fail(APE_ERR_INVALID_ARG, "lstm_features: ALL_STEPS is refused (the last step's vector is the feature)");
    if (flags & ~(uint32_t)(APE_FLAG_NORMALIZE_INPUT | APE_FLAG_DROPOUT_MASKS | APE_FLAG_DROPOUT_PHILOX))
        return ape_fail(APE_ERR_INVALID_ARG, "lstm_features: flag bits 0x%x (NORMALIZE_INPUT and the two dropout modes are accepted)", flags);
    if (m->dims.model_kind != APE_MODEL_LSTM)
        return ape_fail(APE_ERR_UNSUPPORTED, "lstm_features: DropoutLSTM handles only (not FF / ImuPose)");
    if (m->precision != APE_PRECISION_F32) return ape_fail(APE_ERR_UNSUPPORTED, "lstm_features: fp16 precision is set on the model (float32 only)");
    if (!m->has_weights) return ape_fail(APE_ERR_NOT_READY, "lstm_features: weights not loaded");
    if ((flags & APE_FLAG_NORMALIZE_INPUT) && !m->has_stats)
        return ape_fail(APE_ERR_NOT_READY, "lstm_features: NORMALIZE_INPUT without norm stats");
    if ((flags & APE_FLAG_DROPOUT_MASKS) && (flags & APE_FLAG_DROPOUT_PHILOX))
        return ape_fail(APE_ERR_INVALID_ARG, "lstm_features: choose one dropout mode");
    if ((flags & APE_FLAG_DROPOUT_MASKS) && m->dims.num_layers > 1 && !masks_dev)
        return ape_fail(APE_ERR_INVALID_ARG, "lstm_features: DROPOUT_MASKS without masks");
    if ((flags & APE_FLAG_DROPOUT_PHILOX) && !(dropout_p >= 0.0f && dropout_p < 1.0f))
        return ape_fail(APE_ERR_INVALID_ARG, "lstm_features: dropout_p %f outside [0,1)", dropout_p);
    const int H = m->dims.hidden_size, L = m->dims.num_layers;
    const bool drop = (flags & (APE_FLAG_DROPOUT_MASKS | APE_FLAG_DROPOUT_PHILOX)) != 0;
    if (ape_lstm_tile16_smem_bytes(H, L, m->KX, m->dims.output_size, drop) > 160 * 1024)
        return ape_fail(APE_ERR_UNSUPPORTED, "lstm_features: H=%d L=%d with dropout exceeds the 160 KiB LDS of a CU", H, L);
    LstmParams p{};
    p.x = x_dev; p.y = y_dev; p.hout = h_dev;
    for (int l = 0; l < L; ++l) { p.wpack[l] = m->wpack[l]; p.bias[l] = m->bias[l]; }
    head_and_stats(m, &p);
    p.masks = masks_dev; p.flags = flags; p.dropout_p = dropout_p; p.seed = seed;
    p.B = B; p.T = T; p.I = m->lstm_in; p.O = m->dims.output_size; p.KX = m->KX;
    p.hs_rows = B;
    m->last_kernel = "ape_lstm_tile16<hout>";
    hipError_t e = ape_launch_lstm_tile16_hout(H, L, p, (hipStream_t)stream);
    if (e != hipSuccess) return ape_fail(APE_ERR_HIP, "lstm features kernel launch failed: %s", hipGetErrorString(e));
    return APE_OK;
}

int ape_lstm_features(ape_model_t* m, const float* x_dev, int32_t B, int32_t T, uint32_t flags, const float* masks_dev, float dropout_p,
                      uint64_t seed, float* h_dev, float* y_dev, void* stream) {
    const int rc = lstm_features_impl(m, x_dev, B, T, flags, masks_dev, dropout_p, seed, h_dev, y_dev, stream);
    if (rc == APE_OK) {      // (reads what an aborted launch in front of it may have left unwritten: re-issued behind it like a forward)
        ApeJournalEntry e{};
        e.kind = ApeJournalEntry::FEATURES; e.in0 = x_dev; e.in1 = masks_dev; e.out0 = h_dev; e.out1 = y_dev; e.B = B; e.T = T; e.flags = flags;
        e.dropout_p = dropout_p; e.seed = seed; e.stream = stream;
        journal_add(m, e);
    }
    return rc;
}

int ape_lstm_forward_hs(ape_model_t* m, const float* x_dev, int32_t B, int32_t T, uint32_t flags,
                        const float* masks_dev, float dropout_p, uint64_t seed, const float* h0_dev,
                        const float* c0_dev, float* y_dev, void* stream) {
    // (an initial state is served by the batch-tile kernel, which cannot abort: journaled all the same, a later call may)
    const int rc = lstm_forward_impl(m, x_dev, B, T, flags, masks_dev, dropout_p, seed, y_dev, stream, 0, h0_dev, c0_dev);
    if (rc == APE_OK && masks_dev == nullptr) {
        ApeJournalEntry e{};
        e.kind = ApeJournalEntry::FORWARD_HS; e.in0 = x_dev; e.in1 = h0_dev; e.in2 = c0_dev; e.out0 = y_dev; e.B = B; e.T = T;
        e.flags = flags; e.dropout_p = dropout_p; e.seed = seed; e.stream = stream;
        journal_add(m, e);
    } else if (rc == APE_OK && m) {
        m->journal_overflow = true;          // (initial state AND injected masks: not representable in an entry)
    }
    return rc;
}

// The regressor of a DropoutFF frame or replay chunk (ff_bank.hip): sample rows [row_base, row_base + rows) of a call whose
// global row r is sample r % n_mc of group (stream / frame) r / n_mc.  `x`: the newest feature row of group g_base + j at x + j * x_stride,
// g_base = row_base / n_mc.  The trunk once per group (ape_mlp_tile16 with hidden_out: f64 z-score, input layer, hidden layers) into
// `hid` [groups,H], then the n_mc masked heads.  No cooperative kernel: nothing here waits for another workgroup.
int ff_bank_forward(ape_model* m, const float* x, size_t x_stride, long long row_base, int rows, int n_mc, bool norm, const float* masks,
                    float dropout_p, uint64_t seed, float* hid, float* y, void* stream, hipEvent_t ev_a, hipEvent_t ev_z, long long philox_base) {
    if (!m->has_weights) return ape_fail(APE_ERR_NOT_READY, "ff bank: weights not loaded");
    const int H = m->dims.hidden_size, L = m->dims.num_layers, I = m->dims.input_size;
    const long long g_base = row_base / n_mc;
    const int groups = (int)((row_base + rows + n_mc - 1) / n_mc - g_base);
    MlpParams q{};
    q.x = x; q.y = nullptr; q.hidden_out = hid;
    for (int j = 0; j <= L; ++j) { q.wpack[j] = m->ff_wpack[j]; q.bias[j] = m->ff_bias[j]; }
    q.w_out = m->w_out; q.b_out = m->b_out;
    q.xx_m = m->stats; q.xx_s = m->stats + I;
    q.row_stride = x_stride; q.row_offset = 0;
    q.N = groups; q.I = I; q.O = m->dims.output_size; q.KX = m->KX; q.n_hidden = L;
    q.flags = norm ? APE_FLAG_NORMALIZE_INPUT : 0u;
    q.neg_slope = 0.01f;                      // torch's leaky_relu default (nn_models.py:347,349)
    if (ev_a) (void)hipEventRecord(ev_a, (hipStream_t)stream);
    hipError_t e = ape_launch_mlp_tile16(H, q, (hipStream_t)stream, m->n_cus);
    if (e != hipSuccess) return ape_fail(APE_ERR_HIP, "ff bank: trunk launch failed: %s", hipGetErrorString(e));
    FfHeadParams hp{};
    hp.hidden = hid; hp.w_out = m->w_out; hp.b_out = m->b_out; hp.masks = masks; hp.y = y;
    hp.row_base = row_base; hp.g_base = g_base; hp.rows = rows; hp.n_mc = n_mc; hp.H = H; hp.O = m->dims.output_size;
    hp.dropout_p = dropout_p; hp.seed = seed; hp.philox_base = philox_base;
    m->last_kernel = "ape_ff_bank_head";
    e = ape_launch_ff_bank_head(hp, (hipStream_t)stream);
    if (ev_z) (void)hipEventRecord(ev_z, (hipStream_t)stream);
    if (e != hipSuccess) return ape_fail(APE_ERR_HIP, "ff bank: head launch failed: %s", hipGetErrorString(e));
    return APE_OK;
}

int fk_impl(ape_model_t* m, const void* preds_dev, int32_t preds_dtype, int32_t N, int32_t denormalize, void* est_dev,
                   int32_t est_dtype, void* stream, const FkBodyRows* bodies) {
    if (!m || !preds_dev || !est_dev) return ape_fail(APE_ERR_INVALID_ARG, "fk: NULL argument");
    if (N < 1) return ape_fail(APE_ERR_INVALID_ARG, "fk: N=%d must be >= 1", N);
    if ((preds_dtype != APE_F32 && preds_dtype != APE_F64) || (est_dtype != APE_F32 && est_dtype != APE_F64))
        return ape_fail(APE_ERR_INVALID_ARG, "fk: unknown dtype selector");
    if (m->dims.target_layout == APE_LAYOUT_NONE) return ape_fail(APE_ERR_INVALID_ARG, "fk: model has no target layout");
    if (denormalize && !m->has_stats) return ape_fail(APE_ERR_NOT_READY, "fk: denormalize without norm stats");
    FkParams p{};
    p.preds = preds_dev;
    p.est = est_dev;
    if (denormalize) {
        p.yy_m = m->stats + 2 * m->dims.input_size;
        p.yy_s = p.yy_m + m->dims.output_size;
    }
    memcpy(p.body, m->body, sizeof(p.body));
    p.N = N; p.O = m->dims.output_size; p.layout = m->dims.target_layout; p.W = layout_est_width(p.layout);
    hipError_t e = ape_launch_fk(p, preds_dtype, est_dtype, (hipStream_t)stream, bodies);
    if (e != hipSuccess) return ape_fail(APE_ERR_HIP, "fk kernel launch failed: %s", hipGetErrorString(e));
    return APE_OK;
}

int ape_fk(ape_model_t* m, const void* preds_dev, int32_t preds_dtype, int32_t N, int32_t denormalize, void* est_dev,
           int32_t est_dtype, void* stream) {
    const int rc = fk_impl(m, preds_dev, preds_dtype, N, denormalize, est_dev, est_dtype, stream);
    if (rc == APE_OK) {      // (consumes what an aborted launch may have left unwritten: re-issued behind it)
        ApeJournalEntry e{};
        e.kind = ApeJournalEntry::FK; e.in0 = preds_dev; e.out0 = est_dev; e.B = N; e.i0 = preds_dtype; e.i1 = denormalize; e.i2 = est_dtype;
        e.stream = stream;
        journal_add(m, e);
    }
    return rc;
}

int ape_msg_reduce(ape_model_t* m, const double* est_dev, int32_t N, double* msg_dev, void* stream) {
    if (!m || !est_dev || !msg_dev) return ape_fail(APE_ERR_INVALID_ARG, "msg_reduce: NULL argument");
    if (N < 1) return ape_fail(APE_ERR_INVALID_ARG, "msg_reduce: N=%d must be >= 1", N);
    if (m->dims.target_layout == APE_LAYOUT_NONE) return ape_fail(APE_ERR_INVALID_ARG, "msg_reduce: model has no target layout");
    MsgParams p{};
    p.est = est_dev;
    p.msg = msg_dev;
    memcpy(p.body, m->body, sizeof(p.body));
    p.N = N; p.layout = m->dims.target_layout; p.W = layout_est_width(p.layout);
    hipError_t e = ape_launch_msg_reduce(p, (hipStream_t)stream);
    if (e != hipSuccess) return ape_fail(APE_ERR_HIP, "msg kernel launch failed: %s", hipGetErrorString(e));
    ApeJournalEntry je{};
    je.kind = ApeJournalEntry::MSG; je.in0 = est_dev; je.out0 = msg_dev; je.B = N; je.stream = stream;
    journal_add(m, je);
    return APE_OK;
}

int ape_spread_reduce(ape_model_t* m, const double* est_dev, int32_t N, const double* msg_dev, double* spread_dev, void* stream) {
    if (!m || !est_dev || !msg_dev || !spread_dev) return ape_fail(APE_ERR_INVALID_ARG, "spread_reduce: NULL argument");
    if (N < 1) return ape_fail(APE_ERR_INVALID_ARG, "spread_reduce: N=%d must be >= 1", N);
    if (m->dims.target_layout == APE_LAYOUT_NONE) return ape_fail(APE_ERR_INVALID_ARG, "spread_reduce: model has no target layout");
    MsgParams p{};
    p.est = est_dev;
    p.N = N; p.layout = m->dims.target_layout; p.W = layout_est_width(p.layout);
    // (not journaled: no cooperative kernel in front of it can abort it, and it reads what ape_fk / ape_msg_reduce re-issue into)
    hipError_t e = ape_launch_spread_reduce(p, msg_dev, spread_dev, (hipStream_t)stream);
    if (e != hipSuccess) return ape_fail(APE_ERR_HIP, "spread kernel launch failed: %s", hipGetErrorString(e));
    return APE_OK;
}

int ape_parse_rows(int32_t kind, const float* rows_dev, int32_t N, void* xx_dev, int32_t xx_dtype, void* stream) {
    if (!rows_dev || !xx_dev) return ape_fail(APE_ERR_INVALID_ARG, "parse_rows: NULL argument");
    if (N < 1) return ape_fail(APE_ERR_INVALID_ARG, "parse_rows: N=%d must be >= 1", N);
    if (xx_dtype != APE_F32 && xx_dtype != APE_F64) return ape_fail(APE_ERR_INVALID_ARG, "parse_rows: unknown dtype selector");
    int width, I;
    const int big_endian = (kind & APE_PARSE_BIG_ENDIAN) ? 1 : 0;
    kind &= ~APE_PARSE_BIG_ENDIAN;
    if (!parse_kind_dims(kind, &width, &I)) return ape_fail(APE_ERR_INVALID_ARG, "parse_rows: unknown kind %d", kind);
    hipError_t e = ape_launch_parse_rows(rows_dev, N, width, kind, xx_dev, xx_dtype, I, (size_t)I, 1, 0, big_endian,
                                         (hipStream_t)stream);
    if (e != hipSuccess) return ape_fail(APE_ERR_HIP, "parse_rows launch failed: %s", hipGetErrorString(e));
    return APE_OK;
}

int ape_infer(ape_model_t* m, const float* x_dev, int32_t B, int32_t T, uint32_t flags, float* y_dev, void* est_dev,
              int32_t est_dtype, void* stream) {
    if (!m || !x_dev || !est_dev) return ape_fail(APE_ERR_INVALID_ARG, "infer: NULL argument");
    if (flags & (APE_FLAG_ALL_STEPS | APE_FLAG_DROPOUT_MASKS | APE_FLAG_DROPOUT_PHILOX | APE_FLAG_SPREAD))
        return ape_fail(APE_ERR_INVALID_ARG, "infer: only NORMALIZE_INPUT is accepted (use ape_lstm_forward + ape_fk)");
    float* y = y_dev;
    if (!y) {
        if (B > m->y_cap) {
            hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
            (void)hipStreamIsCapturing((hipStream_t)stream, &st);
            if (st != hipStreamCaptureStatusNone)
                return ape_fail(APE_ERR_CAPACITY, "infer: B=%d exceeds reserved %d during stream capture", B, m->y_cap);
            if (int rc = ape_model_reserve(m, B)) return rc;
        }
        y = m->y_ws;
    }
    // de-normalise exactly when the inputs were normalised (estimator.py:103-109: one switch)
    const bool denorm = (flags & APE_FLAG_NORMALIZE_INPUT) != 0;
    if (est_dtype != APE_F32 && est_dtype != APE_F64) return ape_fail(APE_ERR_INVALID_ARG, "fk: unknown dtype selector");
    if (m->dims.target_layout == APE_LAYOUT_NONE) return ape_fail(APE_ERR_INVALID_ARG, "fk: model has no target layout");
    if (denorm && !m->has_stats) return ape_fail(APE_ERR_NOT_READY, "fk: denormalize without norm stats");
    FkTail tail{est_dev, est_dtype, denorm, false};
    if (int rc = lstm_forward_impl(m, x_dev, B, T, flags, nullptr, 0.0f, 0, y, stream, 0, nullptr, nullptr, &tail)) return rc;
    if (!tail.done)                                        // (else the latency kernel finished the rows itself)
        if (int rc = fk_impl(m, y, APE_F32, B, denorm ? 1 : 0, est_dev, est_dtype, stream)) return rc;
    ApeJournalEntry e{};
    e.kind = ApeJournalEntry::INFER; e.in0 = x_dev; e.out0 = y_dev; e.out1 = est_dev; e.B = B; e.T = T; e.flags = flags; e.i2 = est_dtype;
    e.stream = stream;
    journal_add(m, e);
    return APE_OK;
}

// the kernel that serves an eval-mode call of (B, T) -- under AUTO the one that takes the larger part -- by its instantiation's name
const char* ape_lstm_kernel_name(const ape_model_t* m, int32_t B, int32_t T) {
    if (!m) return "";
    if (m->dims.model_kind == APE_MODEL_FF)        // (B rows of the last step, eval mode)
        return (m->ffp_ok && m->ffp_on && B >= 64 * m->n_cus) ? "ape_mlp_pipe" : m->kernel_name.c_str();
    if (B < 1 || T < 1) return m->kernel_name.c_str();
    const LstmPlan p = plan_lstm(m->caps, m->dims, lstm_call(m, B, T, 0, false, 0));
    if (2LL * p.n16 > B) return m->kernel_name.c_str();
    switch (p.route) {
        case PLAN_SPLIT32: return "ape_lstm_upper32<32, true> + <32, false>";
        case PLAN_F16V2: return "ape_lstm_cluster_f16v2";
        case PLAN_F16: return "ape_lstm_cluster_f16";
        case PLAN_C32: return T <= APE_C32_ENDS_MAX_T ? "ape_lstm_cluster32<256, 2, 32, true>" : "ape_lstm_cluster32<256, 2, 32, false>";   // (two instantiations: lstm_cluster32.hip on ENDS)
        case PLAN_LV16: return "ape_lstm_level16<128, 3, 64>";
        case PLAN_C16: return "ape_lstm_cluster16<128, 3, 64, 2>";
        case PLAN_GEN1: case PLAN_SMALL: return m->cluster_name.c_str();      // (the latency kernel shares the first generation's register image)
    }
    return m->kernel_name.c_str();
}

