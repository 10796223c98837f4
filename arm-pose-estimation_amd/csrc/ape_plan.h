// Which kernels serve an LSTM call or a Monte-Carlo bank: the whole decision as pure host arithmetic (no HIP here: tests/tools/plan_sweep.cpp
// compiles this header alone with the host compiler).  ape_api.hip builds an ApeCaps per model (ape_caps); the host files ask plan_lstm / plan_bank and
// launch what they answer; ape_debug_plan*, ape_debug_bank_* and ape_lstm_kernel_name answer from the same functions.
// A new kernel form: a capability bit in ApeCaps, a route here, a case in lstm_forward_impl's launch switch.
#pragma once
#include <cstdlib>

#include "../../include/ape_hip.h"

// ---- what a model on a device with n_cus CUs can run ----
struct ApeCaps {
    // capability bits (ape_caps: the kernels' own *_supported() predicates + the CU count; ape_model_create clears what failed to set up)
    bool cluster_ok = false;        // the first-generation cluster kernel (and with it every cooperative route)
    bool c32 = false;               // lstm_cluster32.hip (2 x 256)
    bool c16 = false;               // lstm_cluster16.hip (3 x 128)
    bool lv16 = false;              // ... and lstm_level16.hip for its short windows
    bool up32 = false;              // bank: the layer above layer 0 on lstm_upper32.hip
    bool up128 = false;             // bank: layers 1 and 2 of the 3 x 128 model on lstm_upper128.hip
    bool upper_ok = false;          // layers 1.. can run on their own over a shared layer-0 sequence
    bool split32 = false;           // ImuPoseLSTM: one layer per launch on lstm_upper32.hip's persistent clusters
    bool mc_small = false;          // lstm_mc_small.hip
    bool f16v2 = false;             // lstm_cluster_f16v2.hip
    bool layer0_one_layer = false;  // the first-generation kernel's one-layer form (launch A of a bank)
    bool wide = false;              // ImuPoseLSTM: the first-generation kernel with a 256-wide layer-0 input, nothing else
    // capacities
    int n_cus = 0;
    int cluster_capacity = 0;       // first-generation clusters (H / 16 workgroups each) resident at once
    int f16v2_capacity = 0;         // 8-member clusters of 32 rows, whole block-index classes of 8
    int level16_max_clusters = 0;   // lstm_level16.hip's 32-window clusters
    int up128_classes = 0;          // lstm_upper128.hip's four-member clusters, whole classes of 8
    // diagnostic overrides for A/B runs (plan_read_overrides)
    int c16_min_t = 12, lv16_max_t = 48, lv16_min_rows = 5;
};

// ---- how a batch is split over the device's CUs (pure arithmetic: unit-tested on the CPU via ape_debug_plan) ----
// A cluster is GH = H/16 workgroups, one per CU, so a device with n_cus CUs runs n_cus / GH clusters at once
// (16 on a whole MI355X at H = 256); a batch-tile "wave" is one 16-row workgroup per CU (4096 rows on 256 CUs).
constexpr int APE_PLAN_TILE_ROWS = 16;          // windows per workgroup in the batch-tile LSTM kernel
inline int cluster_capacity(int n_cus, int H) { return n_cus / (H / 16); }
inline int tile16_wave_rows(int n_cus) { return APE_PLAN_TILE_ROWS * n_cus; }
// smallest row-tile count (16 rows each) per cluster that fits `rows` into one launch; the dropout variants are
// built for at most 2 tiles
inline int cluster_nmt(int cap, int rows, bool cdrop) {
    const int cands[] = {1, 2, 4};
    for (int cand : cands)
        if ((!cdrop || cand <= 2) && (rows + 16 * cand - 1) / (16 * cand) <= cap) return cand;
    return cdrop ? 2 : 4;
}
// fp16 v2 kernel: 8-member clusters of 32 rows, formed within the 8 block-index classes, so a launch carries whole
// groups of 8 clusters = 64 workgroups, all of which must be able to be resident together
inline int f16v2_capacity(int n_cus) { return (n_cus / 64) * 8; }
inline int cluster_rows_per_launch(int cap, bool cdrop) { return 16 * (cdrop ? 2 : 4) * cap; }
// f32 first-generation kernel: whole groups of 8 clusters (if the device holds them) form XCD-local clusters and hand
// their slices over inside that XCD's L2 (lstm_cluster.hip, APE_FLAG_XCD_CLASSES); the extra clusters own no rows
// (a launch of fewer than four clusters -- one stream's 25 Monte-Carlo rows -- stays as it is: there the rendezvous costs
//  more than the shorter hops save, 44.7 vs 43.8 us)
inline int xcd_class_clusters(int clusters, int cap, bool on, bool* formed) {
    const int c8 = (clusters + 7) / 8 * 8;
    *formed = on && clusters >= 4 && c8 <= cap;
    return *formed ? c8 : clusters;
}

inline double plan_flops_per_window(const ape_dims_t* d, int32_t T) {
    const double H = d->hidden_size, I = d->input_size, O = d->output_size;
    if (d->model_kind == APE_MODEL_FF) return 2.0 * (I * H + d->num_layers * H * H + O * H);   // last step only
    double step = 0;
    const double in0 = (d->model_kind == APE_MODEL_IMUPOSE) ? H : I;
    if (d->model_kind == APE_MODEL_IMUPOSE) step += 2.0 * I * H;
    for (int l = 0; l < d->num_layers; ++l) step += 2.0 * 4.0 * H * ((l == 0 ? in0 : H) + H);
    return step * T + 2.0 * O * H;
}

// APE_KERNEL_AUTO: how many whole waves of the batch-tile kernel to peel off the front of a batch.  Measured on a
// whole MI355X (microseconds): a batch-tile wave sustains 125 TFLOP/s at H = 256 and 109 at H = 128 whatever T and
// the dropout mode (a partial wave costs a whole one); a cluster launch costs 25 + 13.7 T (12.5 + 8.3 T for the 2-tile
// dropout variant with XCD-local clusters) however few of its rows are used.  Both rates scale with the CU count of the device.
// `wide` (ImuPoseLSTM, 256-wide layer-0 input): a full batch-tile wave sustains 123 TFLOP/s, the two-tile cluster launch
// (512 rows) costs 20 + 11 T -- 95 TFLOP/s when full, so whole waves go to the batch-tile kernel and the rest to the cluster.
// which cluster kernel serves `rest` rows behind the batch-tile waves (the ONE rule plan_lstm and its cost model share, and through
// plan_lstm the launches, ape_debug_plan and ape_lstm_kernel_name): the second-generation f32 kernel from 513 rows on where the model
// and the call allow it (`c32`: a 2 x 256 model, eval mode, last-step output), else the first-generation kernel
// `gen2`: the second-generation kernel the model and the call are eligible for -- 32: lstm_cluster32.hip (2 x 256), 16:
// lstm_cluster16.hip (3 x 128: a launch costs 24.6 + 6.6 T against the first generation's 15.5 + 7.5 T at 513 .. 1024 rows -- with
// its XCD-local clusters; 15.1 + 7.75 T before them --, so it serves windows of 12 steps and more), 0: none
// (round 6) 48 = 16 + the level-synchronous kernel lstm_level16.hip: T + 2 hand-overs per launch instead of a three-layer pipeline with four
// fill / drain phases.  It serves ONE launch's worth of rows: 5 .. 512 with one row tile per cluster at every window length, 513 .. 1024 with
// two row tiles per cluster (two agents per workgroup) up to 48 steps; lstm_cluster16.hip keeps the longer windows and the larger batches
// (the first six values are ape_debug_plan2's public out[5])
enum { PLAN_NONE = 0, PLAN_GEN1 = 1, PLAN_C32 = 2, PLAN_SMALL = 3, PLAN_C16 = 4, PLAN_LV16 = 5, PLAN_SPLIT32 = 6, PLAN_MC_SMALL = 7,
       PLAN_F16 = 8, PLAN_F16V2 = 9, PLAN_UNSUPPORTED = 10 };
#define APE_LV16_MIN_ROWS 5          // (up to 4 rows: the latency kernel)
#define APE_LV16_MAX_T 48           // two row tiles per cluster, 513 .. 1024 rows: 170.6 / 222.2 / 327.8 us at 24 / 32 / 48 steps against
                                    // lstm_cluster16.hip's 179.5 / 231.7 / 339.8; a tie at 64
#define APE_LV16_MAX_T_SINGLE 4000  // one row tile per cluster, up to 512 rows: faster than the first generation at every window measured
                                    // (512 rows: 40.0 / 66.9 / 123.2 / 231.5 / 304.9 us at 6 / 12 / 24 / 48 / 64 steps against 42.8 / 70.4 / 129.7 /
                                    // 245.3 / 323.2; 5 rows: 34.3 against 42.8); a level's tag holds 12 bits of step count
#define APE_LV16_COST_US0 14.0      // a launch of up to 1024 rows: microseconds = US0 + US_T x T (measured)
#define APE_LV16_COST_US_T 6.8
#define APE_LV16_COST1_US0 13.0     // ... of up to 512 rows (one row tile per cluster)
#define APE_LV16_COST1_US_T 4.5
// the most phases (hand-overs) a launch of the kernels with 12-bit phase tags may run: lstm_level16.hip, lstm_cluster_small.hip and
// lstm_mc_small.hip tag a granule (launch number << 12) | (phase + 1), phase + 1 <= T + L - 1 -- one phase more and the count spills
// into the launch number, where it collides with the stale granules of other launches.  The planner keeps every such route below it and
// the launchers refuse what is above (hipErrorInvalidValue, nothing launched).
#define APE_TAG_MAX_PHASES 4095
// does a window of T steps on an L-layer model fit the 12-bit phase count?  The ONE comparison: the planner's gate of the latency kernel, the
// launchers' refusal and ape_debug_launch_refusal (tests/test_long_windows_cpu.py walks both sides of it) ask here
// (written without T + L: a window length near INT_MAX must not wrap into the range)
inline bool plan_tag_phases_fit(int T, int L) { return T >= 1 && L >= 1 && T <= APE_TAG_MAX_PHASES - (L - 1); }
inline int plan_clamp(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }
// the overrides move thresholds between routes that all serve the shape; none of them can send a window to a kernel beyond its limits:
// lv16_max_t stays within the one-tile form's own limit, the others within the ranges their comparisons have a meaning for
inline void plan_clamp_overrides(ApeCaps* caps) {
    caps->c16_min_t = plan_clamp(caps->c16_min_t, 1, 1 << 20);
    caps->lv16_max_t = plan_clamp(caps->lv16_max_t, 0, APE_LV16_MAX_T_SINGLE);
    caps->lv16_min_rows = plan_clamp(caps->lv16_min_rows, 1, 1 << 20);
}
inline void plan_read_overrides(ApeCaps* caps) {
    static const int c16_min_t = getenv("APE_C16_MIN_T") ? atoi(getenv("APE_C16_MIN_T")) : 12;      // (diagnostic overrides for A/B runs)
    static const int lv16_max_t = getenv("APE_LV16_MAX_T") ? atoi(getenv("APE_LV16_MAX_T")) : APE_LV16_MAX_T;
    static const int lv16_min_rows = getenv("APE_LV16_MIN_ROWS") ? atoi(getenv("APE_LV16_MIN_ROWS")) : APE_LV16_MIN_ROWS;
    caps->c16_min_t = c16_min_t; caps->lv16_max_t = lv16_max_t; caps->lv16_min_rows = lv16_min_rows;
    plan_clamp_overrides(caps);
}
inline int rest_kernel(const ApeCaps& caps, int rest, int T, int gen2) {
    if (rest <= 0) return PLAN_NONE;
    if (gen2 == 32 && rest > 512) return PLAN_C32;
    // (ONE launch only: its workgroups take a CU's whole LDS, so a second launch cannot start under the first one's tail as the first
    //  generation's do -- 2048 x 6: 108 us in two launches against 100)
    if (gen2 == 48 && rest >= caps.lv16_min_rows) {
        if (rest <= 16 * caps.level16_max_clusters && T <= APE_LV16_MAX_T_SINGLE) return PLAN_LV16;       // one row tile per cluster
        if (rest <= 32 * caps.level16_max_clusters && T <= caps.lv16_max_t) return PLAN_LV16;
    }
    if ((gen2 == 16 || gen2 == 48) && rest > 512 && T >= caps.c16_min_t) return PLAN_C16;
    return PLAN_GEN1;
}

// ---- one LSTM call ----
struct LstmCall {
    int B = 0, T = 0;
    bool drop = false;              // DROPOUT_MASKS or DROPOUT_PHILOX
    bool masks = false, philox = false, all_steps = false, broadcast = false, alt_form = false;
    bool have_hs = false;           // caller-given (h0, c0)
    int x_ring = 0;
    int kernel_choice = APE_KERNEL_AUTO, precision = APE_PRECISION_F32;
    bool replaying = false;         // a re-issue by ape_model_recover: the batch-tile kernel, exact float32
    bool c32_on = true;             // the second-generation kernels are not switched off (APE_KERNEL_*_GEN1)
    bool small_batch_path = true, f16_v2 = true;
};

struct LstmPlan {
    int n16 = 0;                    // leading rows for the batch-tile kernel
    int route = PLAN_NONE;          // what serves rows [n16, B)
    int rows_per_launch = 0, nmt = 0 /* row tiles of 16 per cluster */, launches = 0;
    int clusters = 0;               // clusters of the first launch that own rows
    int capacity = 0;               // clusters of the route's kind the device holds
    bool xcd_classes = false;       // a first-generation route: its launches form XCD-local clusters where the call allows them and xcd_class_clusters() finds room
    bool lv16_single = false, cdrop = false;
    const char* last_kernel = "";   // ape_model_last_kernel after the call (static storage)
    int err_code = APE_OK;          // PLAN_UNSUPPORTED: the status and the message (nullptr: injected masks beyond one cluster launch)
    const char* err = nullptr;
};

// the second-generation kernel a call is eligible for (rest_kernel's `gen2`): the ONE gate, for the cost model and for the route
inline int plan_gen2(const ApeCaps& caps, const LstmCall& c) {
    if (c.drop || c.all_steps || caps.wide || !c.c32_on || caps.f16v2_capacity <= 0) return 0;
    if (caps.c32) return 32;
    if (caps.c16) return (caps.lv16 && caps.level16_max_clusters > 0) ? 48 : 16;
    return 0;
}

inline int auto_tile16_waves(const ApeCaps& caps, const ape_dims_t* dims, int B, int T, bool cdrop, int gen2) {
    const int n_cus = caps.n_cus;
    const bool wide = caps.wide;
    const int wave = tile16_wave_rows(n_cus), rpl = cluster_rows_per_launch(caps.cluster_capacity, cdrop || wide);
    if (rpl == 0) return (B + wave - 1) / wave;          // no cluster fits on this device
    const double rate = (wide ? 1.23e14 : dims->hidden_size == 256 ? 1.25e14 : 1.09e14) * n_cus / 256.0;
    const double t16 = (double)wave * plan_flops_per_window(dims, T) / rate * 1e6;
    // first-generation launches: 25 + 13.7 T (12.5 + 8.3 T with dropout, 20 + 11 T wide); second-generation f32 kernel, eval mode:
    // 16 + 12.4 T per launch of up to 32 x f16v2_capacity rows -- priced only where rest_kernel() really picks it
    // (round 4: the dropout form is priced at what it measures with XCD-local clusters, 12.5 + 8.3 T -- the Philox counters name global
    //  rows in every kernel now, so the route a Monte-Carlo call takes no longer decides which samples it draws)
    const double tcl1 = wide ? 20.0 + 11.0 * T : cdrop ? 12.5 + 8.3 * T : 25.0 + 13.7 * T;
    const int rpl2 = 32 * caps.f16v2_capacity;
    auto cost = [&](int w) {
        const int rest = B - wave * w;
        if (rest <= 0) return w * t16;
        const int k = rest_kernel(caps, rest, T, gen2);
        if (k == PLAN_C32) return w * t16 + (double)((rest + rpl2 - 1) / rpl2) * (16.0 + 12.4 * T);
        if (k == PLAN_C16) return w * t16 + (double)((rest + rpl2 - 1) / rpl2) * (24.6 + 6.6 * T);
        if (k == PLAN_LV16) {
            if (rest <= 16 * caps.level16_max_clusters) return w * t16 + APE_LV16_COST1_US0 + APE_LV16_COST1_US_T * T;
            return w * t16 + APE_LV16_COST_US0 + APE_LV16_COST_US_T * T;
        }
        return w * t16 + (double)((rest + rpl - 1) / rpl) * tcl1;
    };
    int best = 0;
    double best_cost = cost(0);
    const int waves[] = {B / wave, (B + wave - 1) / wave};
    for (int w : waves)
        if (w > 0 && cost(w) < best_cost) { best = w; best_cost = cost(w); }
    return best;
}

// Monte-Carlo latency kernel (lstm_mc_small.hip): n_streams windows x n_mc dropout samples each, rows dealt over the 8 XCD clusters
inline bool mc_small_fits(const ApeCaps& caps, const ape_dims_t& dims, int kernel_choice, int precision, bool c32_on, bool replaying,
                          int n_streams, int n_mc) {
    if (!caps.mc_small || !c32_on || kernel_choice != APE_KERNEL_AUTO || precision != APE_PRECISION_F32 || replaying) return false;
    if (n_streams < 1 || n_streams > 8 || n_mc < 1) return false;
    // (its head gives 16 lanes of a 256-thread workgroup to every target: targets 16 .. of the 20-target position layout would stay
    //  unwritten -- such a bank steps on the general route)
    if (dims.output_size > 16) return false;
    const int cps = 8 / n_streams;
    return (n_mc + cps - 1) / cps <= 16;
}

// fp16 v2 kernel, APE_FLAG_ALT_FORM: the 16-unit-member form, two workgroups per CU -- needs 2 x 16 x clusters workgroups resident
inline bool plan_f16v2_duo(const ApeCaps& caps, const LstmCall& c, int nb) {
    return c.alt_form && caps.n_cus * 2 >= 16 * (((nb + 31) / 32 + 7) / 8 * 8);
}

// Two kernels serve an LSTM batch.  The weight-stationary cluster kernel fills the chip from one launch of
// 1..1024 rows (512 with inter-layer dropout) and is the faster one per row on long windows; the batch-tile kernel
// needs 4096 rows (256 workgroups x 16) to fill the chip, but then runs dropout at no extra cost and pays no
// per-launch prologue / head, which decides short windows.  Under APE_KERNEL_AUTO the front of the batch goes to
// the batch-tile kernel in whole 4096-row waves and the rest to the cluster kernel, by a cost model calibrated
// on MI355X (tests/tools/time_big_batch.py).
inline LstmPlan plan_lstm(const ApeCaps& caps, const ape_dims_t& dims, const LstmCall& c) {
    LstmPlan p;
    const int L = dims.num_layers, B = c.B, T = c.T;
    const bool cluster_ok = caps.cluster_ok && caps.cluster_capacity >= 1;
    auto unsupported = [&p](const char* msg) { p = LstmPlan(); p.route = PLAN_UNSUPPORTED; p.err_code = APE_ERR_UNSUPPORTED; p.err = msg; return p; };
    auto chunks = [&p, B](int rows_per_launch, int nmt, int capacity) {
        const int rest = B - p.n16, first = rest < rows_per_launch ? rest : rows_per_launch;
        p.rows_per_launch = rows_per_launch; p.nmt = nmt; p.capacity = capacity;
        p.launches = (rest + rows_per_launch - 1) / rows_per_launch;
        p.clusters = (first + 16 * nmt - 1) / (16 * nmt);
    };
    // ImuPoseLSTM above 512 windows (where the first-generation kernel needs a second launch: 1480 us for 513 .. 1024 windows x 64 steps against
    // 1020-1060 here): the LSTM runs one layer per launch on the persistent clusters of lstm_upper32.hip: layer 0 in the SEQ form
    // with the wide input, layer 1 reading its sequence as is -- K = 512 per layer is the clusters' whole register image; the
    // first-generation kernel's 16-member clusters re-read nothing either but spend 16 CUs on 32 rows.
    // Chunks of 4096 windows bound the workspaces.
    if (caps.split32 && caps.f16v2_capacity >= 8 && B > 512 && c.kernel_choice == APE_KERNEL_AUTO && c.c32_on && c.precision == APE_PRECISION_F32 &&
        !c.replaying && !c.have_hs && !c.all_steps && !c.broadcast && c.x_ring == 0 && T >= 1 && 128ull * T * 32768 < (1ull << 32)) {
        p.route = PLAN_SPLIT32;
        chunks(4096, 2, caps.f16v2_capacity);
        if (p.clusters > p.capacity) p.clusters = p.capacity;       // (persistent clusters walk the 32-row tiles)
        p.last_kernel = "ape_lstm_upper32";
        return p;
    }
    // (a re-issue by ape_model_recover runs on the batch-tile kernel, in exact float32 whatever the precision switch)
    const bool f16 = c.precision == APE_PRECISION_F16 && !c.replaying;
    const bool cdrop = p.cdrop = c.drop && L > 1;
    // injected masks are indexed over the whole batch, so such a call is served by ONE launch of one kernel
    const bool masks_fit = !c.masks || !cdrop || B <= cluster_rows_per_launch(caps.cluster_capacity, cdrop || caps.wide) ||
                           c.kernel_choice == APE_KERNEL_CLUSTER;
    // a caller-given initial state (h0, c0) is served by the batch-tile kernel, which loads it at step 0
    // (all-steps output: the cluster kernel also writes every step's top-layer output to a [B,T,H] workspace and the
    //  head runs over those rows in a second, HBM-bound launch -- in float32 only)
    bool use_cluster = cluster_ok && masks_fit && c.kernel_choice != APE_KERNEL_TILE16 && !(c.all_steps && f16) && !c.have_hs && !c.replaying;
    if (c.have_hs && f16) return unsupported("lstm_forward: the fp16 variant starts from the zero state only");
    if (f16 && (!cluster_ok || c.drop || c.all_steps))
        return unsupported("lstm_forward: the fp16 variant covers last-step output without dropout on "
                           "the cluster-kernel shapes only");
    if (f16) use_cluster = true;
    if (c.kernel_choice == APE_KERNEL_CLUSTER && !use_cluster && !c.replaying)
        return unsupported("lstm_forward: the cluster kernel does not cover this model / these flags");
    // one window, n dropout samples (monte_carlo_predictions, nn_models.py:191-207) up to 128 rows: the Monte-Carlo latency kernel
    if (use_cluster && cdrop && c.broadcast && !c.all_steps && !f16 && B <= 128 && T <= 64 &&
        mc_small_fits(caps, dims, c.kernel_choice, c.precision, c.c32_on, c.replaying, 1, B)) {
        p.route = PLAN_MC_SMALL; p.rows_per_launch = B; p.launches = 1; p.clusters = p.capacity = 8;
        p.last_kernel = "ape_lstm_mc_small";
        return p;
    }
    const int gen2 = plan_gen2(caps, c);
    p.n16 = use_cluster ? 0 : B;
    if (use_cluster && c.kernel_choice == APE_KERNEL_AUTO && !f16 && !c.all_steps && !c.masks && B > 4) {
        const long long front = (long long)tile16_wave_rows(caps.n_cus) * auto_tile16_waves(caps, &dims, B, T, cdrop, gen2);
        p.n16 = (front < B) ? (int)front : B;
    }
    p.last_kernel = "ape_lstm_tile16";
    if (p.n16 == B) return p;
    const int rest = B - p.n16;
    const bool small = !f16 && !cdrop && !c.all_steps && B <= 4 && plan_tag_phases_fit(T, L) && c.small_batch_path && !caps.wide;   // latency path: VALU GEMV, one exchange per phase
    p.route = f16 ? PLAN_F16 : small ? PLAN_SMALL : rest_kernel(caps, rest, T, gen2);
    // second-generation fp16 kernel: 8-member clusters x 2 row sets of 16 that take turns (lstm_cluster_f16v2.hip)
    if (f16 && c.f16_v2 && caps.f16v2 && caps.f16v2_capacity > 0 && B > 256) p.route = PLAN_F16V2;
    switch (p.route) {
        case PLAN_C32:        // second-generation f32 kernel: 8-member clusters of 32 windows, 32x32x2 MFMA chain (lstm_cluster32.hip)
        case PLAN_C16:        // second-generation kernel of the 3 x 128 model: 8-member clusters of 32 windows (lstm_cluster16.hip)
        case PLAN_F16V2:
            chunks(32 * caps.f16v2_capacity, 2, caps.f16v2_capacity);
            p.last_kernel = p.route == PLAN_C32 ? "ape_lstm_cluster32" : p.route == PLAN_C16 ? "ape_lstm_cluster16" :
                            plan_f16v2_duo(caps, c, rest - (p.launches - 1) * p.rows_per_launch) ? "ape_lstm_cluster_f16v2<duo>" : "ape_lstm_cluster_f16v2";
            break;
        case PLAN_LV16:       // short windows of the 3 x 128 model: level-synchronous 32-window clusters, one eight-wave workgroup per CU (lstm_level16.hip)
            // up to 16 rows per cluster of the device: one row tile per cluster, so that the rows spread over every CU
            p.lv16_single = rest <= 16 * caps.level16_max_clusters;
            chunks(16 * (p.lv16_single ? 1 : 2) * caps.level16_max_clusters, p.lv16_single ? 1 : 2, caps.level16_max_clusters);
            p.last_kernel = "ape_lstm_level16";
            break;
        default: {            // the first-generation kernel, its fp16 variant, the latency kernel
            // smallest row tile count that still fits the batch on the chip: more clusters = more CUs busy
            const int nmt = cluster_nmt(caps.cluster_capacity, rest, cdrop || caps.wide);      // (wide: at most two row tiles, like dropout)
            chunks(16 * nmt * caps.cluster_capacity, nmt, caps.cluster_capacity);
            // injected masks are indexed [L-1, B, T, H] over the WHOLE batch: chunks need the full B stride,
            // so a masked call is served by one launch only
            if (c.masks && cdrop && p.launches > 1) return unsupported(nullptr);
            p.xcd_classes = p.route == PLAN_GEN1;
            p.last_kernel = small ? "ape_lstm_cluster_small" : f16 ? "ape_lstm_cluster_f16" : "ape_lstm_cluster";
        }
    }
    return p;
}

// ---- which route a Monte-Carlo bank takes, as pure arithmetic on (model shape, CU count, bank size): planned by ape_streams_set_mc,
// read by streams_step_impl and, for the CPU tests of the thresholds, by ape_debug_bank_route ---------------------------------------------
// Sample rows from which a Monte-Carlo bank of a 2 x 256 model takes the weight-stationary route (layer 0 once per stream, the layer above
// over the sample rows, both on lstm_upper32.hip): above 512 -- where the fused first-generation dropout kernel needs a second launch.
// (Until round 5: 2048, two tiles per cluster -- a cluster with ONE tile paid its exchange in the open; with the SOLO form it does not.
//  Measured, pocket, T = 6, frame of all streams: 21 x 25 rows 159 -> 117 us, 41 x 25 221 -> 160, 80 x 25 290 -> 168, 34 x 60 318 -> 167;
//  up to 512 rows the one fused launch stays ahead: 20 x 25 97.5 against 116.)
enum { BANK_FUSED = 0, BANK_SHARED_TILE16 = 1, BANK_UPPER32 = 2, BANK_UPPER128 = 3 };              // route of the layers above layer 0
enum { BANK_A_NONE = 0, BANK_A_TILE16 = 1, BANK_A_SEQ32 = 2, BANK_A_ONE_LAYER = 3 };                // kernel of launch A (layer 0 once per stream)
#ifndef APE_BANK_SHARE_MIN_ROWS_128
// the 3 x 128 model's route (lstm_upper128.hip; no one-tile form, every exchange of a one-tile cluster is exposed): from where the fused
// first-generation dropout kernel needs a THIRD launch.  Measured, T = 6, frame of all streams, fused launches / this route: 11 x 50 rows
// 125.4 / 137.9 us -- 21 x 50 213.8 / 141.6, 30 x 50 213.8 / 146.1, 40 x 50 215.8 / 150.2, 64 x 25 179.9 / 147.2 (2048 until round 5)
#define APE_BANK_SHARE_MIN_ROWS_128 1025
#endif
#ifndef APE_BANK_A_ONE_LAYER_MAX_STREAMS
// 2 x 256 banks: launch A on the first-generation kernel's one-layer form up to this many streams (three any-placement clusters of 32;
// from four clusters on that kernel forms XCD classes and the rendezvous eats the gain).  Measured, pocket, T = 6, frame of all streams,
// one-layer form against the SEQ form of lstm_upper32.hip: 21 x 25 108.1 / 118.7 us, 41 x 25 155.3 / 165.7, 64 x 25 157.2 / 165.2,
// 80 x 25 173.0 / 178.7 -- 100 x 25 220.3 / 215.8, 200 x 25 341.5 / 338.3, 512 x 25 767.4 / 748.4.
#define APE_BANK_A_ONE_LAYER_MAX_STREAMS 96
#endif
#ifndef APE_BANK_SHARE_MIN_ROWS
#define APE_BANK_SHARE_MIN_ROWS 513
#endif
struct BankPlan {
    bool shared_l0 = false;         // layer 0 once per stream (two launches per step)
    int route = BANK_FUSED, a_form = BANK_A_NONE;
    long long chunk_rows = 0;       // sample rows per launch B of the weight-stationary routes
};
// chunks of equal size whose expanded input (T KiB per sample row) stays under 2 GiB -- inside one 32-bit buffer
// descriptor with offsets to spare; whole 1024-row waves of clusters where that costs nothing.  (Measured at
// 8192 x 25, T = 6: one 1.26 GB chunk 9.30 ms per frame, five 256 MB chunks -- the Infinity Cache's size -- 9.38 ms: a
// launch's prologue and tail cost more than the cache residency of the tiles buys; 288 GB of HBM make the footprint
// a non-issue.)
// `l0_bytes`: the larger of launch A's two buffers on lstm_upper32.hip (sequence, input tiles), each behind one 32-bit descriptor
inline bool bank_chunk_plan(bool up128, int S, int T, int n_mc, unsigned long long l0_bytes, long long* chunk_rows) {
    const long long total = (long long)S * n_mc;
    const long long max_chunk = ((2047ll << 20) / ((long long)T * (up128 ? 512 : 1024))) / 1024 * 1024;
    const bool l0_fits = up128 || l0_bytes < (2047ull << 20);
    if (max_chunk < 1024 || total >= (1ll << 31) || !l0_fits) return false;       // (the input builder indexes sample rows with 32 bits)
    const long long n_chunks = (total + max_chunk - 1) / max_chunk;
    long long chunk = ((total + n_chunks - 1) / n_chunks + 1023) / 1024 * 1024;
    if (chunk > total) chunk = (total + 31) / 32 * 32;
    *chunk_rows = chunk;
    return true;
}
inline bool bank_shares_layer0(long long sample_rows, int n_cus, bool can_up32, bool can_up128) {
    return sample_rows >= 2LL * tile16_wave_rows(n_cus) ||
           (can_up32 && sample_rows >= (can_up128 ? APE_BANK_SHARE_MIN_ROWS_128 : APE_BANK_SHARE_MIN_ROWS));
}
// launch A of a bank on `route` (a cooperative step on a healthy model; a replay or a forced kernel takes the batch-tile launch)
inline int bank_launch_a_form(const ApeCaps& caps, int route, int S) {
    if (route == BANK_FUSED) return BANK_A_NONE;
    const bool one_layer_fits = caps.cluster_ok && caps.layer0_one_layer && (S + 31) / 32 <= caps.cluster_capacity;
    if (route == BANK_UPPER32) return (one_layer_fits && S <= APE_BANK_A_ONE_LAYER_MAX_STREAMS) ? BANK_A_ONE_LAYER : BANK_A_SEQ32;
    if (route == BANK_UPPER128) return one_layer_fits ? BANK_A_ONE_LAYER : BANK_A_TILE16;
    return BANK_A_TILE16;
}
// Layer 0 once per stream (nn.LSTM's dropout sits BETWEEN the layers, so h_0(t) is the same for all samples of a
// stream): worth its extra launch from two batch-tile waves of sample rows on.
// (on the weight-stationary route -- lstm_upper32.hip, both launches -- the sharing pays from APE_BANK_SHARE_MIN_ROWS sample rows on;
//  the 3 x 128 model's route, lstm_upper128.hip, from APE_BANK_SHARE_MIN_ROWS_128)
inline BankPlan plan_bank(const ApeCaps& caps, const ape_dims_t& dims, int S, int T, int n_mc, float dropout_p, int kernel_choice,
                          int precision, bool c32_on, unsigned long long l0_bytes) {
    BankPlan p;
    const bool can_up128 = caps.up128 && caps.up128_classes >= 8 && c32_on;
    const bool can_up32 = (caps.up32 && c32_on && caps.f16v2_capacity >= 8) || can_up128;
    p.shared_l0 = dims.model_kind == APE_MODEL_LSTM && caps.upper_ok && kernel_choice == APE_KERNEL_AUTO && precision == APE_PRECISION_F32 &&
                  dropout_p > 0.0f && n_mc >= 2 && bank_shares_layer0((long long)S * n_mc, caps.n_cus, can_up32, can_up128);
    if (p.shared_l0)
        p.route = (can_up32 && bank_chunk_plan(can_up128, S, T, n_mc, l0_bytes, &p.chunk_rows)) ? (can_up128 ? BANK_UPPER128 : BANK_UPPER32) : BANK_SHARED_TILE16;
    p.a_form = bank_launch_a_form(caps, p.route, S);
    return p;
}
