// The ape_debug_* entries that ship in the product library (not in the public header): read-outs of diagnostic words, and the pure host
// arithmetic the CPU tests call -- the planner, the bank routes, the split weight image.  (The test hooks that poke state: ape_debug.hip.)
#include "ape_host.h"
#include "weight_pack.h"

extern "C" {

// internal diagnostic accessor (not part of the public header): copies the 2 stamp words
int ape_debug_read_stamps(ape_model_t* m, unsigned long long out[14]) {
    if (!m || !m->caps.cluster_ok) return APE_ERR_INVALID_ARG;
    APE_TRY(hipMemcpy(out, ctl_words(m).status + 4, 112, hipMemcpyDeviceToHost));
    return APE_OK;
}

int ape_debug_read_wg(ape_model_t* m, unsigned long long out[256 * 8]) {
    if (!m || !m->dbg_wg) return APE_ERR_INVALID_ARG;
    APE_TRY(hipMemcpy(out, m->dbg_wg, 256 * 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return APE_OK;
}

// internal: read `n` control words of the MLP pipeline from word `first` on (its segment stamps, tests/tools/pipe_stamps.py)
int ape_debug_peek_pipe(ape_model_t* m, int first, unsigned* out, int n) {
    if (!m || !m->ffp_ok || !out || first < 0 || n < 1 || (size_t)(first + n) > m->ffp_ctl_words) return APE_ERR_INVALID_ARG;
    APE_TRY(hipSetDevice(m->dims.device));
    APE_TRY(hipDeviceSynchronize());
    APE_TRY(hipMemcpy(out, m->ffp_ctl + first, (size_t)n * sizeof(unsigned), hipMemcpyDeviceToHost));
    return APE_OK;
}

// internal: pack_c32_split for one layer (no GPU needed); `out` holds (KXl + H) / 2 * 8 * 4 * 64 dwords.  Returns S or -1.
int ape_debug_pack_c32_split(const float* w_ih, int in_l, const float* w_hh, int H, int KXl, int kx_f32, unsigned* out) {
    if (!w_ih || !w_hh || !out || H < 32 || H % 32 != 0 || KXl % 8 != 0 || kx_f32 % 8 != 0 || (KXl + H - kx_f32) % 16 != 0) return -1;
    return pack_c32_split(w_ih, in_l, w_hh, H, KXl, kx_f32, out);
}

// internal: the batch split of lstm_forward for a device with `n_cus` CUs, no GPU needed: plan_lstm for a healthy model under
// APE_KERNEL_AUTO, float32, last-step output.  `cdrop`: a dropout call; `c32` = 0: the second-generation kernels switched off.
// out = {rows to the batch-tile kernel, row tiles per cluster, clusters of the first launch, cluster launches, cluster capacity,
// the kernel that serves the rest (PLAN_* of ape_plan.h)}; with the second-generation kernels out[1] (row tiles) is 2 = their 32-row clusters.
// The dims' model_kind counts: an APE_MODEL_FF model has no LSTM route (out = {B, 0, 0, 0, capacity, PLAN_NONE}), ImuPoseLSTM dims are planned
// with their 256-wide LSTM input and can answer out[5] = PLAN_SPLIT32 (6), a value beyond the six the 2 x 256 / 3 x 128 LSTMs produce
int ape_debug_plan2(const ape_dims_t* dims, int n_cus, int B, int T, int cdrop, int c32, int out[6]) {
    if (!dims || !out || n_cus < 1 || B < 1 || T < 1) return APE_ERR_INVALID_ARG;
    const ApeCaps caps = ape_caps(dims, n_cus);
    LstmCall call;
    call.B = B; call.T = T; call.drop = call.philox = cdrop != 0; call.c32_on = c32 != 0;
    const LstmPlan p = plan_lstm(caps, *dims, call);
    out[0] = p.n16; out[1] = p.nmt; out[2] = p.clusters; out[3] = p.launches; out[4] = caps.cluster_capacity; out[5] = p.route;
    return APE_OK;
}
int ape_debug_bank_chunks(int up128, int S, int T, int n_mc, long long out[3]) {
    if (!out || S < 1 || T < 1 || n_mc < 1) return APE_ERR_INVALID_ARG;
    long long chunk = 0;
    out[0] = bank_chunk_plan(up128 != 0, S, T, n_mc, bank_l0_bytes(S, T), &chunk) ? 1 : 0;
    out[1] = chunk;
    out[2] = out[0] ? ((long long)S * n_mc + chunk - 1) / chunk : 0;
    return APE_OK;
}

// the route ape_streams_set_mc plans for a Monte-Carlo bank of S streams x n_mc samples on a healthy model under APE_KERNEL_AUTO, float32,
// dropout on (pure host arithmetic, for the CPU tests): out = {layer 0 shared 0/1, route BANK_*, launch A's kernel BANK_A_*, chunk rows}
int ape_debug_bank_route(const ape_dims_t* dims, int n_cus, int S, int T, int n_mc, long long out[4]) {
    if (!dims || !out || n_cus < 1 || S < 1 || T < 1 || n_mc < 1) return APE_ERR_INVALID_ARG;
    const BankPlan p = plan_bank(ape_caps(dims, n_cus), *dims, S, T, n_mc, 0.5f, APE_KERNEL_AUTO, APE_PRECISION_F32, true, bank_l0_bytes(S, T));
    out[0] = p.shared_l0 ? 1 : 0; out[1] = p.route; out[2] = p.a_form; out[3] = p.chunk_rows;
    return APE_OK;
}

// internal: what the launcher of a kernel with 12-bit phase tags answers to a window that does not fit them, no GPU needed (the launchers
// refuse in front of every HIP call).  kernel 0: lstm_level16.hip (3 x 128), 1: lstm_cluster_small.hip (2 x 256), 2: the same (3 x 128).
// Nothing is ever launched from here: where the window fits, the answer is -1 and the launcher is not called; else its hipError_t.
int ape_debug_launch_refusal(int kernel, int T) {
    if (kernel < 0 || kernel > 2) return -2;
    const int L = kernel == 1 ? 2 : 3;
    if (plan_tag_phases_fit(T, L)) return -1;
    ClusterParams p{};
    p.T = T;
    if (kernel == 0) return (int)ape_launch_lstm_level16(128, 3, 64, 16, p, nullptr);
    if (kernel == 1) return (int)ape_launch_lstm_cluster_small(256, 2, 32, 1, 4, p, nullptr);
    return (int)ape_launch_lstm_cluster_small(128, 3, 64, 1, 4, p, nullptr);
}

int ape_debug_plan(const ape_dims_t* dims, int n_cus, int B, int T, int cdrop, int out[5]) {
    int o6[6];
    const int rc = ape_debug_plan2(dims, n_cus, B, T, cdrop, 0, o6);
    if (rc == APE_OK) for (int i = 0; i < 5; ++i) out[i] = o6[i];
    return rc;
}


}  // extern "C"
