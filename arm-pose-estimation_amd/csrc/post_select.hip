// Selecting post-filter (ape_post_select): the normalised targets y [F, M, O] of ONE replay re-smoothed with a window per
// frame -- the windows are a ladder of L rungs (ape_post_window's list), sel [S, F] on the device names the rung of every frame of each
// of S sets, and row (s, f) of the output holds the bits ape_post_window writes for window sel[s, f] of that ladder at frame f.  The
// reference has no counterpart: it smooths every frame over the same number of past frames (estimator.py:112-118).
//
// This file is the entry's front: its argument checks -- ape_post_window's, under this entry's name (post_window_args), and its own for
// the selector.  The pass itself -- ape_post_window_fk_kernel, ape_post_select_kernel, the plan, the workspace and the launches -- is
// post_filter (post_common.h, defined in post_window.hip, which states the order of the sums).  The selector is never read on the host:
// the call does not wait, and a value >= L stays in its own row as NaN.
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

int ape_post_select_last(int32_t out4[4]) {
    if (!out4) return ape_fail(APE_ERR_INVALID_ARG, "post_select_last: NULL argument");
    for (int i = 0; i < 4; ++i) out4[i] = g_last[i];
    return APE_OK;
}

int ape_post_select(ape_model_t* m, const float* y_dev, int32_t F, int32_t n_mc, const int32_t* seg_starts_host, int32_t R,
                    const int32_t* windows_host, const double* weights_host, int32_t L, const uint8_t* sel_dev, int32_t S, uint32_t flags,
                    const double* bodies_host, int32_t n_bodies, void* out_dev, int32_t out_dtype, int64_t workspace_bytes, void* stream) {
    // the arguments on their own (no device needed to refuse them); post_filter checks them against the model
    bool tapered[APE_POST_MAX_CONFIGS] = {};
    if (int rc = ape_postcommon::post_window_args("post_select", y_dev, out_dev, F, n_mc, seg_starts_host, R, windows_host, weights_host, L, flags,
                                                  bodies_host, n_bodies, out_dtype, workspace_bytes, tapered)) return rc;
    if (!sel_dev) return ape_fail(APE_ERR_INVALID_ARG, "post_select: NULL selector");
    if (S < 1 || S > APE_POST_MAX_CONFIGS) return ape_fail(APE_ERR_INVALID_ARG, "post_select: S=%d selector rows (1 .. %d)", S, APE_POST_MAX_CONFIGS);
    return ape_postcommon::post_filter("post_select", "windows", m, y_dev, F, n_mc, seg_starts_host, R, windows_host, weights_host, tapered, L,
                                       sel_dev, S, flags, bodies_host, n_bodies, out_dev, out_dtype, workspace_bytes, stream, g_last);
}
