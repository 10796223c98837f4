// Stand-alone sweep of csrc/ape_plan.h (host compiler only, built and run by tests/test_plan_grid_cpu.py under the address and
// undefined-behaviour sanitizers): hand-built ApeCaps with every capability bit on and off -- bits on with ZERO capacities included --
// x n_cus 1..320 x batch sizes x window lengths x every flag combination.  Every plan must serve every row exactly once, never start
// more clusters than the device holds, and cover the rest with its launches.
#include <cstdio>
#include <initializer_list>

#include "../../arm-pose-estimation_amd/csrc/ape_plan.h"

static long long g_plans = 0, g_failures = 0;

#define CHECK(cond)                                                                                                              \
    do {                                                                                                                         \
        if (!(cond)) {                                                                                                           \
            if (g_failures++ < 20)                                                                                               \
                fprintf(stderr, "FAILED %s: H=%d n_cus=%d bits=0x%x zero=%d B=%d T=%d call=0x%x -> route %d n16 %d rpl %d nmt %d launches %d clusters %d cap %d\n", \
                        #cond, dims.hidden_size, n_cus, bits, zero_caps, B, T, cb, p.route, p.n16, p.rows_per_launch, p.nmt, p.launches, p.clusters,            \
                        p.capacity);                                                                          \
        }                                                                                                                        \
    } while (0)

static const int kRows[] = {1, 4, 5, 16, 17, 256, 257, 512, 513, 1024, 1025, 2048, 2460, 4096, 4097, 4396, 8292, 12345};
static const int kSteps[] = {1, 6, 11, 12, 48, 49, 64, 200};

static ApeCaps make_caps(const ape_dims_t& dims, int n_cus, unsigned bits, bool zero_caps) {
    ApeCaps c;
    c.cluster_ok = bits & 1; c.c32 = bits & 2; c.c16 = bits & 4; c.lv16 = bits & 8; c.up32 = bits & 16; c.up128 = bits & 32;
    c.upper_ok = bits & 64; c.split32 = bits & 128; c.mc_small = bits & 256; c.f16v2 = bits & 512; c.layer0_one_layer = bits & 1024;
    c.wide = bits & 2048;
    c.n_cus = n_cus;
    if (!zero_caps) {
        c.cluster_capacity = cluster_capacity(n_cus, dims.hidden_size);
        c.f16v2_capacity = f16v2_capacity(n_cus);
        c.level16_max_clusters = (n_cus / 8) / 8 * 8;
        c.up128_classes = (n_cus / 4) / 8 * 8;
    }
    return c;
}

static void sweep_lstm(const ape_dims_t& dims, int n_cus, unsigned bits, bool zero_caps) {
    const ApeCaps caps = make_caps(dims, n_cus, bits, zero_caps);
    for (int B : kRows)
        for (int T : kSteps)
            for (int cb = 0; cb < 6 * 64; ++cb) {
                // every combination of the call's flags: dropout mode 0 none / 1 masks / 2 Philox, all_steps, broadcast, alt_form, have_hs ...
                const int mode = cb & 3, sw = cb >> 6;
                if (mode == 3) continue;
                LstmCall c;
                c.B = B; c.T = T;
                c.masks = mode == 1; c.philox = mode == 2; c.drop = mode != 0;
                c.all_steps = cb & 4; c.broadcast = cb & 8; c.alt_form = cb & 16; c.have_hs = cb & 32;
                // ... under each setting of the model's switches: default, CLUSTER, TILE16, fp16, second generation off, a re-issue with the rest off
                c.kernel_choice = sw == 1 ? APE_KERNEL_CLUSTER : sw == 2 ? APE_KERNEL_TILE16 : APE_KERNEL_AUTO;
                c.precision = sw == 3 ? APE_PRECISION_F16 : APE_PRECISION_F32;
                c.c32_on = sw != 4;
                c.replaying = sw == 5;
                c.small_batch_path = c.f16_v2 = sw != 5;
                {
                    const LstmPlan p = plan_lstm(caps, dims, c);
                    ++g_plans;
                    if (p.route == PLAN_UNSUPPORTED) { CHECK(p.err_code != APE_OK); continue; }
                    CHECK(p.last_kernel != nullptr && p.last_kernel[0] != 0);
                    CHECK(p.n16 >= 0 && p.n16 <= B);
                    const int rest = B - p.n16;
                    if (rest == 0) { CHECK(p.route == PLAN_NONE && p.launches == 0); continue; }
                    CHECK(p.route != PLAN_NONE);
                    // every row exactly once: the launches tile [n16, B) without a gap, and the last one is not empty
                    CHECK(p.rows_per_launch > 0 && p.launches > 0);
                    if (p.rows_per_launch <= 0 || p.launches <= 0) continue;
                    CHECK((long long)p.launches * p.rows_per_launch >= rest);
                    CHECK((long long)(p.launches - 1) * p.rows_per_launch < rest);
                    if (p.route == PLAN_MC_SMALL) continue;         // (its rows are dealt over 8 fixed clusters by the kernel)
                    CHECK(p.capacity > 0 && p.clusters > 0);
                    bool formed = false;          // (what the launch starts: whole XCD classes of 8 where they fit)
                    const int started = xcd_class_clusters(p.clusters, p.capacity, p.xcd_classes, &formed);
                    CHECK(p.clusters <= p.capacity && started <= p.capacity && started >= p.clusters);
                    CHECK(p.nmt == 1 || p.nmt == 2 || p.nmt == 4);
                    const int first = rest < p.rows_per_launch ? rest : p.rows_per_launch;
                    CHECK((long long)p.clusters * 16 * p.nmt >= first || p.route == PLAN_SPLIT32);       // the first launch's clusters hold its rows
                    CHECK(p.rows_per_launch <= p.capacity * 16 * p.nmt || p.route == PLAN_SPLIT32);   // (split32: persistent clusters walk the tiles)
                }
            }
}

static void sweep_bank(const ape_dims_t& dims, int n_cus, unsigned bits, bool zero_caps) {
    const ApeCaps caps = make_caps(dims, n_cus, bits, zero_caps);
    static const int kMc[] = {1, 2, 19, 25, 50};
    for (int n_mc : kMc)
        for (int R : kRows)
            for (int S : {R / n_mc, (R + n_mc - 1) / n_mc}) {
                if (S < 1) continue;
                for (int T : kSteps)
                    for (int sw = 0; sw < 8; ++sw) {
                        const BankPlan p = plan_bank(caps, dims, S, T, n_mc, (sw & 1) ? 0.0f : 0.2f, (sw & 2) ? APE_KERNEL_TILE16 : APE_KERNEL_AUTO,
                                                     APE_PRECISION_F32, !(sw & 4),
                                                     (unsigned long long)((S + 31) / 32) * T * 32768);
                        ++g_plans;
                        const int B = S * n_mc, cb = sw;
                        bool ok = true;
                        if (!p.shared_l0) ok = ok && p.route == BANK_FUSED && p.a_form == BANK_A_NONE && p.chunk_rows == 0;
                        if (p.route == BANK_UPPER32 || p.route == BANK_UPPER128) {
                            ok = ok && p.chunk_rows >= 32 && p.chunk_rows % 32 == 0;
                            ok = ok && p.chunk_rows * (long long)T * (p.route == BANK_UPPER128 ? 512 : 1024) <= (2047ll << 20);
                        } else {
                            ok = ok && p.chunk_rows == 0;
                        }
                        if (p.a_form == BANK_A_ONE_LAYER) ok = ok && (S + 31) / 32 <= caps.cluster_capacity;
                        if (!ok && g_failures++ < 20)
                            fprintf(stderr, "FAILED bank: H=%d n_cus=%d bits=0x%x zero=%d S=%d n_mc=%d B=%d T=%d sw=%d -> shared %d route %d a %d chunk %lld\n",
                                    dims.hidden_size, n_cus, bits, zero_caps, S, n_mc, B, T, cb, p.shared_l0, p.route, p.a_form, p.chunk_rows);
                    }
            }
}

int main() {
    const ape_dims_t shapes[] = {{22, 256, 2, 14, APE_LAYOUT_ORI_CAL_LARM_UARM_HIPS, 0, APE_MODEL_LSTM},
                                 {38, 128, 3, 12, APE_LAYOUT_ORI_CAL_LARM_UARM, 0, APE_MODEL_LSTM},
                                 {22, 256, 2, 14, APE_LAYOUT_ORI_CAL_LARM_UARM_HIPS, 0, APE_MODEL_IMUPOSE}};
    // every capability bit on over the whole CU range 1..320 for all three shapes, every bit off for one.  The mixed sets -- those a model can
    // show, single bits on their own -- run on CU counts on both sides of every step of a capacity (a first-generation cluster at 8 / 16
    // CUs, whole classes of eight 32-row clusters at 64, 128, 256, a partial class at 40 and 304, none at 7) and, with ZERO capacities
    // (a division by a capacity would show here), on four counts, since the capacities no longer follow the count: a full cross product of
    // 17 sets x 320 counts x 41 472 calls would run for minutes under the sanitizers
    const unsigned bit_sets[] = {0xfffu, 0u, 0x7ffu, 1u, 1u | 2u | 16u | 64u | 256u | 512u | 1024u, 1u | 4u | 8u | 32u | 64u | 256u | 1024u,
                                 1u | 4u | 32u | 64u, 1u | 128u | 2048u, 1u | 2048u, 2u, 4u | 8u, 128u, 256u, 512u, 1u | 512u, 1u | 2u, 1u | 8u};
    for (int n_cus = 1; n_cus <= 320; ++n_cus) {
        for (const ape_dims_t& dims : shapes) sweep_lstm(dims, n_cus, 0xfffu, false);
        sweep_lstm(shapes[0], n_cus, 0u, false);         // (no capability: every shape plans the batch-tile kernel alone)
    }
    for (const ape_dims_t& dims : shapes)
        for (unsigned bits : bit_sets) {
            for (int n_cus : {7, 16, 40, 64, 256, 304}) {
                sweep_lstm(dims, n_cus, bits, false);
                sweep_bank(dims, n_cus, bits, false);
            }
            for (int n_cus : {8, 64, 256, 304}) {
                sweep_lstm(dims, n_cus, bits, true);
                sweep_bank(dims, n_cus, bits, true);
            }
        }
    printf("plan_sweep: %lld plans, %lld failures\n", g_plans, g_failures);
    return g_failures == 0 ? 0 : 1;
}
