// Post-filter sweep (ape_post_sweep): the normalised targets y [F, M, O] of ONE replay re-smoothed at C configurations
// (smooth_c, m_c) in one pass -- for every c and frame the message (and spread record) ape_replay writes with smooth = smooth_c and
// m_c samples, stack row i = sample i % m_c of frame max(seg, f - smooth_c + 1 + i / m_c).  The reference has no counterpart beyond the
// per-frame arithmetic (estimator.py:108-118,122-137; compose_msg.py:13-108; transformations.py:32-51).
//
// This file is the entry's front: its argument checks, and the translation of configuration (smooth, m) to the uniform window
// (smooth - 1, 0, m), whose stack is the same rows in the same order.  The pass itself -- ape_post_window_fk_kernel,
// ape_post_window_kernel, the plan, the workspace and the launches -- is post_filter (post_common.h, defined in post_window.hip, which
// states the order of the sums); a sweep runs the kernel's SWEEP instantiations, which hold neither the upper clamp nor the tapered form.
//
// The only device code compiled here is post_common.h's; contraction is off for it as for every file of the post-filter.
#include "ape_internal.h"
#include "ape_model.h"
#include "../../include/ape_hip.h"
#include "bank_host.h"

#pragma clang fp contract(off)
#include "post_common.h"

namespace {
thread_local int g_last[4] = {0, 0, 0, 0};
}  // namespace

int ape_post_sweep_last(int32_t out4[4]) {
    if (!out4) return ape_fail(APE_ERR_INVALID_ARG, "post_sweep_last: NULL argument");
    for (int i = 0; i < 4; ++i) out4[i] = g_last[i];
    return APE_OK;
}

int ape_post_sweep(ape_model_t* m, const float* y_dev, int32_t F, int32_t n_mc, const int32_t* seg_starts_host, int32_t R,
                   const int32_t* configs_host, int32_t C, uint32_t flags, const double* bodies_host, int32_t n_bodies,
                   void* out_dev, int32_t out_dtype, int64_t workspace_bytes, void* stream) {
    // the arguments on their own (no device needed to refuse them); post_filter checks them against the model
    if (!y_dev || !out_dev || !seg_starts_host || !configs_host) return ape_fail(APE_ERR_INVALID_ARG, "post_sweep: NULL argument");
    if (int rc = ape_check_segments("post_sweep", F, seg_starts_host, R)) return rc;
    if (n_mc < 1) return ape_fail(APE_ERR_INVALID_ARG, "post_sweep: n_mc=%d must be >= 1", n_mc);
    if ((long long)F * n_mc >= (1ll << 31)) return ape_fail(APE_ERR_UNSUPPORTED, "post_sweep: F*n_mc = %lld sample rows (< 2^31)", (long long)F * n_mc);
    if (C < 1 || C > APE_POST_MAX_CONFIGS) return ape_fail(APE_ERR_INVALID_ARG, "post_sweep: C=%d configurations (1 .. %d)", C, APE_POST_MAX_CONFIGS);
    int32_t windows[3 * APE_POST_MAX_CONFIGS];
    for (int c = 0; c < C; ++c) {
        const int s = configs_host[2 * c], k = configs_host[2 * c + 1];
        if (s < 1 || s > 64) return ape_fail(APE_ERR_INVALID_ARG, "post_sweep: configuration %d: smooth %d outside 1..64", c, s);
        if (k < 1 || k > n_mc) return ape_fail(APE_ERR_INVALID_ARG, "post_sweep: configuration %d: %d samples outside 1..n_mc = %d", c, k, n_mc);
        if (s * k > 4096) return ape_fail(APE_ERR_INVALID_ARG, "post_sweep: configuration %d: smooth*samples = %d above 4096", c, s * k);
        windows[3 * c] = s - 1; windows[3 * c + 1] = 0; windows[3 * c + 2] = k;
    }
    if ((bodies_host == nullptr) != (n_bodies == 0) || (n_bodies != 0 && n_bodies != 1 && n_bodies != R))
        return ape_fail(APE_ERR_INVALID_ARG, "post_sweep: n_bodies %d is neither 0 (NULL bodies), 1 nor R = %d", n_bodies, R);
    if (flags & ~(uint32_t)APE_FLAG_SPREAD) return ape_fail(APE_ERR_INVALID_ARG, "post_sweep: only the SPREAD flag is accepted");
    if (out_dtype != APE_F32 && out_dtype != APE_F64) return ape_fail(APE_ERR_INVALID_ARG, "post_sweep: unknown dtype selector");
    if (workspace_bytes < 0) return ape_fail(APE_ERR_INVALID_ARG, "post_sweep: workspace_bytes %lld is negative (0 = default)", (long long)workspace_bytes);
    return ape_postcommon::post_filter("post_sweep", "configurations", m, y_dev, F, n_mc, seg_starts_host, R, windows, nullptr, nullptr, C, nullptr, 0,
                                       flags, bodies_host, n_bodies, out_dev, out_dtype, workspace_bytes, stream, g_last);
}
