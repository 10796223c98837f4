// Stand-alone check of csrc/score_host.h's helpers that make no HIP call: which layouts have a pose to score, the width of a truth row,
// and the check of a lag sweep with its exact messages and the window reach it returns.  Brings its own ape_fail, which records code
// and text.  Built and run by tests/test_score_host_cpu.py (address + undefined-behaviour sanitizers where the runtime is installed).
#include <cstdarg>
#include <cstdio>
#include <string>

#include "../../arm-pose-estimation_amd/csrc/score_host.h"

static int g_code = 0;
static std::string g_text;

int ape_fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_code = code;
    g_text = buf;
    return code;
}

static int g_bad = 0;

static void expect(bool ok, const char* what) {
    if (ok) return;
    printf("FAILED: %s (last error %d \"%s\")\n", what, g_code, g_text.c_str());
    g_bad += 1;
}

static void refused(int rc, const char* text, const char* what) {
    expect(rc == APE_ERR_INVALID_ARG && g_code == APE_ERR_INVALID_ARG && g_text == text, what);
}

int main() {
    static_assert(APE_SCORE_MAX_LAG == 128 && APE_SCORE_MAX_LAGS == 65, "the messages below spell these bounds out");

    // ---- the width of a truth row: 3 layouts x 2 kinds
    expect(ape_truth_width(APE_LAYOUT_ORI_CAL_LARM_UARM_HIPS, APE_TRUTH_TARGETS) == 14, "width: hips layout, targets");
    expect(ape_truth_width(APE_LAYOUT_ORI_CAL_LARM_UARM, APE_TRUTH_TARGETS) == 12, "width: layout without hips, targets");
    expect(ape_truth_width(APE_LAYOUT_ORI_POS_CAL_LARM_UARM_HIPS, APE_TRUTH_TARGETS) == 20, "width: position layout, targets");
    expect(ape_truth_width(APE_LAYOUT_ORI_CAL_LARM_UARM_HIPS, APE_TRUTH_EST) == 21, "width: hips layout, est rows");
    expect(ape_truth_width(APE_LAYOUT_ORI_CAL_LARM_UARM, APE_TRUTH_EST) == 14, "width: layout without hips, est rows");
    expect(ape_truth_width(APE_LAYOUT_ORI_POS_CAL_LARM_UARM_HIPS, APE_TRUTH_EST) == 21, "width: position layout, est rows");

    // ---- the layouts with a pose
    expect(ape_scoring_layout(APE_LAYOUT_ORI_CAL_LARM_UARM_HIPS), "layout 0 has a pose");
    expect(ape_scoring_layout(APE_LAYOUT_ORI_CAL_LARM_UARM), "layout 1 has a pose");
    expect(ape_scoring_layout(APE_LAYOUT_ORI_POS_CAL_LARM_UARM_HIPS), "layout 2 has a pose");
    expect(!ape_scoring_layout(APE_LAYOUT_NONE), "APE_LAYOUT_NONE has none");
    expect(!ape_scoring_layout(3), "layout 3 has none");

    // ---- the lag sweep
    int L = -1, back = -1, fwd = -1;
    refused(ape_check_lag_sweep("e", 3, 2, nullptr, 2, &L, &back, &fwd), "e: lag_min 3 above lag_max 2", "sweep: lag_min > lag_max");
    refused(ape_check_lag_sweep("e", -32, 33, nullptr, 2, &L, &back, &fwd), "e: 66 lags in the sweep, at most 65", "sweep: 66 lags");
    expect(L == -1 && back == -1 && fwd == -1, "sweep: a refused sweep writes nothing");
    expect(ape_check_lag_sweep("e", -32, 32, nullptr, 2, &L, &back, &fwd) == APE_OK && L == 65 && back == 32 && fwd == 32, "sweep: 65 lags");

    // a recording's offset that puts one end of its lags one past the bound
    const int32_t high[3] = {0, 119, 0};               // 119 + 10 = 129
    refused(ape_check_lag_sweep("e", -5, 10, high, 3, &L, &back, &fwd), "e: recording 1: lags 114 .. 129, |lag| is at most 128",
            "sweep: upper end at +129");
    const int32_t low[2] = {-124, 0};                   // -124 - 5 = -129
    refused(ape_check_lag_sweep("e", -5, 10, low, 2, &L, &back, &fwd), "e: recording 0: lags -129 .. -114, |lag| is at most 128",
            "sweep: lower end at -129");
    const int32_t edge[2] = {118, -123};                // 128 and -128: the bound itself
    expect(ape_check_lag_sweep("e", -5, 10, edge, 2, &L, &back, &fwd) == APE_OK && L == 16 && back == 128 && fwd == 128, "sweep: ends at +-128");
    // (offsets near the ends of int32: the sums are formed in 64 bits)
    const int32_t far[1] = {2147483647};
    refused(ape_check_lag_sweep("e", 1, 1, far, 1, &L, &back, &fwd), "e: recording 0: lags 2147483648 .. 2147483648, |lag| is at most 128",
            "sweep: offset INT32_MAX");

    // no offsets: the sweep alone
    expect(ape_check_lag_sweep("e", -5, 7, nullptr, 5, &L, &back, &fwd) == APE_OK && L == 13 && back == 7 && fwd == 5, "sweep: NULL offsets");
    expect(ape_check_lag_sweep("e", 3, 9, nullptr, 1, &L, &back, &fwd) == APE_OK && L == 7 && back == 9 && fwd == 0, "sweep: all lags positive");
    expect(ape_check_lag_sweep("e", -9, -3, nullptr, 1, &L, &back, &fwd) == APE_OK && L == 7 && back == 0 && fwd == 9, "sweep: all lags negative");

    // mixed signs, by hand: lags -5 .. 7 on offsets 0, 2, -3, 0, 1 -> per recording -5..7, -3..9, -8..4, -5..7, -4..8:
    // the largest lag of any pair is 9 (back), the smallest -8 (fwd = 8)
    const int32_t mixed[5] = {0, 2, -3, 0, 1};
    expect(ape_check_lag_sweep("e", -5, 7, mixed, 5, &L, &back, &fwd) == APE_OK && L == 13 && back == 9 && fwd == 8, "sweep: mixed offsets");
    // every recording's lags on one side: offsets 10, 20 with lags -2 .. 2 -> 8..12, 18..22: back 22, nothing forward
    const int32_t up[2] = {10, 20};
    expect(ape_check_lag_sweep("e", -2, 2, up, 2, &L, &back, &fwd) == APE_OK && L == 5 && back == 22 && fwd == 0, "sweep: offsets all positive");

    if (g_bad == 0) printf("score_host ok\n");
    return g_bad == 0 ? 0 : 1;
}
