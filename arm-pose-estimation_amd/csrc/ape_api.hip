// C ABI of libape_hip.so (see include/ape_hip.h).  Host side: handle, weight packing, checks,
// kernel dispatch.  No CPU fallback: every compute entry point needs a gfx950 device.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstring>
#include <new>
#include <string>
#include <utility>
#include <vector>

#include "../../include/ape_hip.h"
#include "ape_internal.h"
#include "ape_model.h"

namespace {
thread_local std::string g_err;
}

int ape_fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

namespace {

int layout_targets(int layout) {
    switch (layout) {
        case APE_LAYOUT_ORI_CAL_LARM_UARM_HIPS: return 14;
        case APE_LAYOUT_ORI_CAL_LARM_UARM: return 12;
        case APE_LAYOUT_ORI_POS_CAL_LARM_UARM_HIPS: return 20;
    }
    return -1;
}
int layout_est_width(int layout) { return layout == APE_LAYOUT_ORI_CAL_LARM_UARM ? 14 : 21; }

int check_dims(const ape_dims_t* d) {
    if (!d) return ape_fail(APE_ERR_INVALID_ARG, "dims is NULL");
    if (d->input_size < 1 || d->input_size > APE_MAX_INPUT)
        return ape_fail(APE_ERR_UNSUPPORTED, "input_size %d outside 1..%d", d->input_size, APE_MAX_INPUT);
    if (d->hidden_size != 128 && d->hidden_size != 256)
        return ape_fail(APE_ERR_UNSUPPORTED, "hidden_size %d: kernels are built for 128 and 256", d->hidden_size);
    if (d->model_kind != APE_MODEL_LSTM && d->model_kind != APE_MODEL_FF && d->model_kind != APE_MODEL_IMUPOSE)
        return ape_fail(APE_ERR_INVALID_ARG, "unknown model_kind %d", d->model_kind);
    if (d->model_kind == APE_MODEL_IMUPOSE && (d->hidden_size != 256 || d->num_layers != 2))
        return ape_fail(APE_ERR_INVALID_ARG, "ImuPoseLSTM is a fixed 2 x 256 LSTM behind a 256-wide input layer "
                    "(nn_models.py:222-229), got hidden_size %d num_layers %d", d->hidden_size, d->num_layers);
    if (d->model_kind != APE_MODEL_FF && (d->num_layers < 1 || d->num_layers > APE_MAX_LAYERS))
        return ape_fail(APE_ERR_UNSUPPORTED, "num_layers %d outside 1..%d", d->num_layers, APE_MAX_LAYERS);
    if (d->model_kind == APE_MODEL_FF && (d->num_layers < 0 || d->num_layers > APE_MAX_FF_LAYERS - 1))
        return ape_fail(APE_ERR_UNSUPPORTED, "hidden_layer_count %d outside 0..%d", d->num_layers, APE_MAX_FF_LAYERS - 1);
    if (d->output_size < 1 || d->output_size > APE_MAX_OUTPUT)
        return ape_fail(APE_ERR_UNSUPPORTED, "output_size %d outside 1..%d", d->output_size, APE_MAX_OUTPUT);
    if (d->target_layout == APE_LAYOUT_NONE) return APE_OK;      // regressor only, no post-filter
    const int want = layout_targets(d->target_layout);
    if (want < 0) return ape_fail(APE_ERR_INVALID_ARG, "unknown target_layout %d", d->target_layout);
    if (want != d->output_size)
        return ape_fail(APE_ERR_INVALID_ARG, "target_layout %d needs output_size %d, got %d", d->target_layout, want,
                    d->output_size);
    return APE_OK;
}

int padded_input(int I) { return ((I + 31) / 32) * 32; }

bool parse_kind_dims(int kind, int* width, int* I) {
    switch (kind) {
        case APE_PARSE_WATCH_PHONE_POCKET: *width = 55; *I = 22; return true;
        case APE_PARSE_WATCH_ONLY: *width = 28; *I = 20; return true;
        case APE_PARSE_WATCH_ONLY_PHONE_MSG: *width = 55; *I = 20; return true;
        case APE_PARSE_WATCH_PHONE_UARM: *width = 55; *I = 38; return true;
    }
    return false;
}

}  // namespace

static_assert(APE_PLAN_TILE_ROWS == APE_TILE_ROWS, "ape_plan.h prices the batch-tile kernel's waves");

// What a model of `dims` can run on a device with n_cus CUs: the kernels' own predicates, in ONE place (ape_model_create, which then
// clears what failed to set up, and the ape_debug_* entry points).  The routing on top of it is csrc/ape_plan.h.
static ApeCaps ape_caps(const ape_dims_t* dims, int n_cus) {
    ApeCaps c;
    const int H = dims->hidden_size, L = dims->num_layers, O = dims->output_size;
    const bool imupose = dims->model_kind == APE_MODEL_IMUPOSE;
    const int KX = padded_input(imupose ? H : dims->input_size);
    c.n_cus = n_cus;
    c.cluster_capacity = cluster_capacity(n_cus, H);
    c.f16v2_capacity = f16v2_capacity(n_cus);
    c.level16_max_clusters = ape_level16_max_clusters(n_cus);
    c.up128_classes = (n_cus / 4) / 8 * 8;
    plan_read_overrides(&c);
    if (dims->model_kind == APE_MODEL_FF) return c;
    c.upper_ok = !imupose && ((H == 256 && L == 2) || (H == 128 && L == 3));     // the deployed shapes: layers 1.. can run on their own
    // the cluster kernels need one whole cluster (GH workgroups, one per CU) resident at once: a device with fewer
    // CUs than that gets the batch-tile kernel only (set_kernel(CLUSTER) then answers APE_ERR_UNSUPPORTED)
    c.cluster_ok = ape_cluster_supported(H, L, KX) && c.cluster_capacity >= 1;
    if (!c.cluster_ok) return c;
    c.wide = imupose;
    c.layer0_one_layer = ape_cluster_layer0_supported(H, KX);
    c.f16v2 = ape_cluster_f16v2_supported(H, L, KX) && c.f16v2_capacity > 0;
    // Monte-Carlo latency kernel (lstm_mc_small.hip): 8 clusters of H/8 members, one per XCD, layer 0 on the latency kernel's
    // H/8-member register image (only where an XCD has that many CUs)
    c.mc_small = ape_mc_small_supported(H, L, KX) && n_cus / 8 >= H / 8 && n_cus >= 8 * (H / 8) && !imupose;
    c.c32 = ape_cluster32_supported(H, L, KX) && c.f16v2_capacity > 0;
    c.up32 = c.c32 && ape_upper32_supported(H, L, O) && !imupose;       // shares the layer-1 register image, the exchange buffer and the flags
    // ImuPoseLSTM (2 x 256 behind a 256-wide input layer): each layer is exactly one register image of lstm_upper32.hip's clusters
    // (K = 256 + 256); above 512 windows the LSTM runs there, one layer per launch
    c.split32 = imupose && H == 256 && L == 2 && KX == 256 && ape_upper32_supported(H, L, O) && c.f16v2_capacity >= 8;
    // the Monte-Carlo bank's weight-stationary route for the 3 x 128 model (lstm_upper128.hip): four-member clusters, whole classes of 8
    c.up128 = ape_upper128_supported(H, L, O) && c.up128_classes >= 8 && !imupose;
    c.c16 = ape_cluster16_supported(H, L, KX) && c.f16v2_capacity > 0 && !imupose;
    // the level-synchronous kernel (one workgroup of two agents per CU, 32-window clusters of 8 members), if the device holds a whole
    // block-index class of its clusters -- 64 CUs -- (else the first generation serves those calls)
    c.lv16 = c.c16 && ape_level16_supported(H, L, KX) && c.level16_max_clusters > 0;
    return c;
}

// plan_bank's `l0_bytes`: the larger of launch A's two buffers on lstm_upper32.hip
static unsigned long long bank_l0_bytes(int S, int T) { return std::max(ape_lower32_hseq_bytes(S, T), ape_lower32_xfrag_bytes(S, T)); }
// the call's switches as the planner reads them
static LstmCall lstm_call(const ape_model* m, int B, int T, uint32_t flags, bool have_hs, int x_ring) {
    LstmCall c;
    c.B = B; c.T = T;
    c.masks = (flags & APE_FLAG_DROPOUT_MASKS) != 0; c.philox = (flags & APE_FLAG_DROPOUT_PHILOX) != 0; c.drop = c.masks || c.philox;
    c.all_steps = (flags & APE_FLAG_ALL_STEPS) != 0; c.broadcast = (flags & APE_FLAG_BROADCAST_X) != 0; c.alt_form = (flags & APE_FLAG_ALT_FORM) != 0;
    c.have_hs = have_hs; c.x_ring = x_ring;
    c.kernel_choice = m->kernel_choice; c.precision = m->precision; c.replaying = m->replaying;
    c.c32_on = m->c32_on; c.small_batch_path = m->small_batch_path; c.f16_v2 = m->f16_v2;
    return c;
}

// head and input statistics, as every kernel's parameter block names them
template <typename P>
static void head_and_stats(const ape_model* m, P* p) { p->w_out = m->w_out; p->b_out = m->b_out; p->xx_m = m->stats; p->xx_s = m->stats + m->dims.input_size; }
// may a first-generation launch form XCD-local clusters?  (APE_FLAG_NO_XCD_CLASSES: selector, A/B on one box)
static bool xcd_classes_on(const ape_model* m, uint32_t flags) { return m->gen1_classes && !(flags & APE_FLAG_NO_XCD_CLASSES); }
// the fields every launch of a cluster kernel shares, with `layers` of the weight image of `route` (PLAN_* of ape_plan.h; lstm_x / lstm_in:
// the LSTM's own input -- ImuPoseLSTM's is the 256-wide activation of its input layer).  No memset in the launch path: the kernels' last
// workgroup re-zeroes every polled word (self-cleaning)
static ClusterParams cluster_params(const ape_model* m, int route, int layers, const float* x, float* y, int B, int T, uint32_t flags, int x_ring) {
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
// ... and of the persistent upper-layer clusters (lstm_upper32.hip, lstm_upper128.hip); the caller adds the layers' weights and buffers
template <typename U = UpperParams>
static U upper_params(const ape_model* m, int T, int tiles, uint32_t flags) {
    U u{};
    u.w_out = m->w_out;
    u.hx = m->hx; u.hx_bytes = m->hx_bytes;
    u.xflags = m->xflags; u.status = ctl_words(m).status; u.done = ctl_words(m).done;
    u.xcc_slots = m->xcc_slots; u.dbg_wg = m->dbg_wg;
    u.T = T; u.O = m->dims.output_size; u.n_tiles = tiles; u.flags = flags;
    return u;
}

// every successfully enqueued compute call of a handle is remembered until its next successful check (ape_model_recover)
static void journal_add(ape_model* m, const ApeJournalEntry& e) {
    if (!m || m->replaying) return;
    if (m->journal_n < APE_JOURNAL_CAP) m->journal[m->journal_n++] = e;
    else m->journal_overflow = true;
}
static void journal_clear(ape_model* m) { m->journal_n = 0; m->journal_overflow = false; }

// Split register image of lstm_cluster32.hip (the recurrent products on v_mfma_f32_32x32x16_f16): the same size and the same
// [member 8][wave 4][group][lane 64][4 dwords] order as the f32 image (m->wcl32), one wave's 32 columns ordered gate * 8 + unit (column
// m = lane & 31, half hh = lane >> 5).  The first `kx_f32` columns of Wcat = [W_ih | W_hh] (layer 0's input columns) stay f32, as in
// the f32 image: group kb, dword j = Wcat[row][8 kb + 4 hh + j] * 2^S.  The remaining columns come in K = 16 slices s, two groups each:
// group kx_f32 / 8 + 2 s holds hi = f16(W * 2^sw) and group + 1 lo = f16(W * 2^sw - hi), both in the 32x32x16 A-fragment order -- element
// e = 0..7 of lane (m, hh) is k = kx_f32 + 16 s + 8 hh + e, element 2 d in the low half of dword d.  The power-of-two 2^sw puts max|W| of
// the split columns in [2^14, 2^15), so every lo of a weight above max|W| * 2^-17 is a normal f16 and hi + lo = W * 2^sw to 2^-22 relative.
// The kernel stores h * 2^APE_C32_HSHIFT in the same split (|h| <= 1), so its accumulators hold 2^S times the gate pre-activations,
// S = sw + APE_C32_HSHIFT; it starts them at 2^S (b_ih + b_hh) and folds 2^-S into the gate constants.
// Returns S, or -1 when the layer cannot take the split: a non-finite weight, or a scale outside [0, 64] / f32 input columns that would
// overflow (the model then stays off this kernel).
static int pack_c32_split(const float* w_ih, int in_l, const float* w_hh, int H, int KXl, int kx_f32, unsigned* out) {
    auto wcat = [&](int row, int k) -> float {
        if (k < KXl) return (k < in_l) ? w_ih[(size_t)row * in_l + k] : 0.0f;
        return w_hh[(size_t)row * H + (k - KXl)];
    };
    const int K = KXl + H;
    float wmax = 0.0f, xmax = 0.0f;
    for (int row = 0; row < 4 * H; ++row)
        for (int k = 0; k < K; ++k) {
            const float v = wcat(row, k);
            if (!std::isfinite(v)) return -1;
            if (k < kx_f32) xmax = std::max(xmax, std::fabs(v));
            else wmax = std::max(wmax, std::fabs(v));
        }
    int ex = 0;
    if (wmax > 0.0f) (void)std::frexp(wmax, &ex);          // wmax in [2^(ex-1), 2^ex)
    const int sw = (wmax > 0.0f) ? 15 - ex : 0;
    const int S = sw + APE_C32_HSHIFT;
    if (S < 0 || S > 64 || std::ldexp((double)xmax, S) >= 0x1p100) return -1;
    const int NG = kx_f32 / 8 + 2 * ((K - kx_f32) / 16);
    for (int mem = 0; mem < 8; ++mem)
        for (int w = 0; w < 4; ++w)
            for (int g = 0; g < NG; ++g)
                for (int lane = 0; lane < 64; ++lane) {
                    const int mcol = lane & 31, hh = lane >> 5;
                    const int row = (mcol >> 3) * H + mem * 32 + w * 8 + (mcol & 7);
                    unsigned* dst = out + ((((size_t)(mem * 4 + w) * NG) + g) * 64 + lane) * 4;
                    if (g < kx_f32 / 8) {
                        for (int j = 0; j < 4; ++j) {
                            const float v = std::ldexp(wcat(row, 8 * g + 4 * hh + j), S);
                            std::memcpy(&dst[j], &v, 4);
                        }
                        continue;
                    }
                    const int s = (g - kx_f32 / 8) / 2, lo = (g - kx_f32 / 8) & 1;
                    for (int d = 0; d < 4; ++d) {
                        unsigned short hw[2];
                        for (int e2 = 0; e2 < 2; ++e2) {
                            const float v = std::ldexp(wcat(row, kx_f32 + 16 * s + 8 * hh + 2 * d + e2), sw);     // exact: |v| < 2^15
                            const _Float16 hi = (_Float16)v;
                            const _Float16 part = lo ? (_Float16)(v - (float)hi) : hi;
                            std::memcpy(&hw[e2], &part, 2);
                        }
                        dst[d] = (unsigned)hw[0] | ((unsigned)hw[1] << 16);
                    }
                }
    return S;
}

extern "C" {

int ape_abi_version(void) { return APE_ABI_VERSION; }
const char* ape_last_error(void) { return g_err.c_str(); }

int ape_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
    int ok = 0;
    for (int i = 0; i < n; ++i) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, i) == hipSuccess && strncmp(prop.gcnArchName, "gfx950", 6) == 0) ++ok;
    }
    return ok;
}

size_t ape_weight_blob_floats(const ape_dims_t* d) {
    if (check_dims(d) != APE_OK) return 0;
    const size_t H = d->hidden_size, I = d->input_size, O = d->output_size;
    if (d->model_kind == APE_MODEL_FF) return H * I + H + (size_t)d->num_layers * (H * H + H) + O * H + O;
    size_t n = 0;
    const size_t in0 = (d->model_kind == APE_MODEL_IMUPOSE) ? H : I;          // LSTM layer 0 reads the input layer's output
    if (d->model_kind == APE_MODEL_IMUPOSE) n += H * I + H;
    for (int l = 0; l < d->num_layers; ++l) n += 4 * H * (l == 0 ? in0 : H) + 4 * H * H + 8 * H;
    return n + O * H + O;
}

double ape_flops_per_window(const ape_dims_t* d, int32_t T) {
    if (check_dims(d) != APE_OK || T < 1) return 0.0;
    return plan_flops_per_window(d, T);
}

int ape_model_create(const ape_dims_t* dims, ape_model_t** out) {
    if (!out) return ape_fail(APE_ERR_INVALID_ARG, "out_model is NULL");
    *out = nullptr;
    if (int rc = check_dims(dims)) return rc;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0) {
        (void)hipGetLastError();
        return ape_fail(APE_ERR_NO_DEVICE, "no HIP device visible: libape_hip has no CPU fallback");
    }
    if (dims->device < 0 || dims->device >= n) return ape_fail(APE_ERR_INVALID_ARG, "device %d of %d", dims->device, n);
    hipDeviceProp_t prop;
    APE_TRY(hipGetDeviceProperties(&prop, dims->device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return ape_fail(APE_ERR_NO_DEVICE, "device %d is %s; this library is built for gfx950 only", dims->device,
                    prop.gcnArchName);
    APE_TRY(hipSetDevice(dims->device));

    ape_model* m = new (std::nothrow) ape_model();
    if (!m) return ape_fail(APE_ERR_HIP, "out of host memory");
    m->dims = *dims;
    m->n_cus = prop.multiProcessorCount;            // 256 on a whole MI355X; fewer on a partitioned / CU-masked device
    m->caps = ape_caps(dims, m->n_cus);             // (below: the bits whose set-up fails are cleared again)
    const bool imupose = dims->model_kind == APE_MODEL_IMUPOSE;
    m->lstm_in = imupose ? dims->hidden_size : dims->input_size;
    m->KX = padded_input(m->lstm_in);
    m->KXpre = padded_input(dims->input_size);
    const double def_body[9] = {-0.22, 0, 0, -0.26, 0, 0, -0.1704612, 0.4309841, -0.00670862};  // bone_map.py:42-45
    memcpy(m->body, def_body, sizeof(def_body));
    const int H = dims->hidden_size, L = dims->num_layers, O = dims->output_size, I = dims->input_size;
    const int NT = 4 * (H / 64);
    // per-device kernel attributes of the MLP / head-rows kernels (every model kind can reach one of them)
    hipError_t e = ape_prepare_mlp_tile16(H);
    // every fixed-size device buffer of the model comes out of ONE allocation (planned first, carved after at
    // 256-byte boundaries, zero-filled): one driver call to create, one to free, and the flag / ticket words start
    // at zero without separate memsets
    std::vector<std::pair<void**, size_t>> plan_list;
    auto plan = [&](void** ptr, size_t bytes) { plan_list.emplace_back(ptr, bytes); return hipSuccess; };
    auto commit_plan = [&]() -> hipError_t {
        size_t total = 0;
        for (auto& it : plan_list) total += (it.second + 255) / 256 * 256;
        hipError_t ee = hipMalloc(&m->slab, total);
        if (ee != hipSuccess) return ee;
        m->slab_bytes = total;
        ee = hipMemset(m->slab, 0, total);
        if (ee != hipSuccess) return ee;
        size_t off = 0;
        for (auto& it : plan_list) { *it.first = static_cast<char*>(m->slab) + off; off += (it.second + 255) / 256 * 256; }
        return hipSuccess;
    };
    if (dims->model_kind == APE_MODEL_FF) {
        for (int j = 0; j <= L && e == hipSuccess; ++j) {
            const size_t K = (j == 0) ? m->KX : H;
            e = plan((void**)&m->ff_wpack[j], K * H * sizeof(float));
            if (e == hipSuccess) e = plan((void**)&m->ff_bias[j], H * sizeof(float));
        }
        if (e == hipSuccess) e = plan((void**)&m->w_out, (size_t)O * H * sizeof(float));
        if (e == hipSuccess) e = plan((void**)&m->b_out, O * sizeof(float));
        if (e == hipSuccess) e = plan((void**)&m->stats, (3 * I + 2 * O) * sizeof(double));
        if (e == hipSuccess && ape_mlp_pipe_supported(H, L, m->KX, O) && m->n_cus >= 16) {
            e = plan((void**)&m->ffp_wa0, (size_t)4 * 2 * 4 * 64 * 4 * sizeof(float));
            if (e == hipSuccess) e = plan((void**)&m->ffp_wa1, (size_t)4 * 2 * 32 * 64 * 4 * sizeof(float));
            if (e == hipSuccess) e = plan((void**)&m->ffp_wb2, (size_t)4 * 2 * 32 * 64 * 4 * sizeof(float));
            if (e == hipSuccess) e = plan((void**)&m->ffp_wbo, (size_t)4 * 8 * 64 * 4 * sizeof(float));
            m->ffp_ring_bytes = ape_mlp_pipe_ring_bytes(m->n_cus);
            m->ffp_ctl_words = ape_mlp_pipe_ctl_words(m->n_cus);
            if (e == hipSuccess) e = plan((void**)&m->ffp_ring, m->ffp_ring_bytes);
            if (e == hipSuccess) e = plan((void**)&m->ffp_ctl, m->ffp_ctl_words * sizeof(unsigned));
            if (e == hipSuccess) e = ape_prepare_mlp_pipe();
            m->ffp_ok = e == hipSuccess;
        }
        if (e == hipSuccess) e = commit_plan();
        if (e != hipSuccess) {
            ape_model_destroy(m);
            return ape_fail(APE_ERR_HIP, "model allocation failed: %s", hipGetErrorString(e));
        }
        m->kernel_name = H == 256 ? "ape_mlp_tile16<256>" : "ape_mlp_tile16<128>";
        *out = m;
        return APE_OK;
    }
    for (int l = 0; l < L && e == hipSuccess; ++l) {
        const size_t Q = ((l == 0 ? m->KX : H) + H) / 16;
        e = plan((void**)&m->wpack[l], 4 * Q * NT * 64 * sizeof(f32x4));
        if (e == hipSuccess) e = plan((void**)&m->bias[l], 4 * H * sizeof(float));
    }
    if (e == hipSuccess) e = plan((void**)&m->w_out, (size_t)O * H * sizeof(float));
    if (e == hipSuccess) e = plan((void**)&m->b_out, O * sizeof(float));
    if (e == hipSuccess) e = plan((void**)&m->stats, (3 * I + 2 * O) * sizeof(double));
    if (imupose) {       // input layer: the MLP kernel's packing and launch, with the activation as its result
        if (e == hipSuccess) e = plan((void**)&m->ff_wpack[0], (size_t)m->KXpre * H * sizeof(float));
        if (e == hipSuccess) e = plan((void**)&m->ff_bias[0], H * sizeof(float));
        if (e == hipSuccess) e = ape_prepare_lstm_tile16_wide(ape_lstm_tile16_smem_bytes(H, L, m->KX, O, false));
    }
    // the kernel may carve its largest LDS layout (with dropout buffers)
    const size_t smem = ape_lstm_tile16_smem_bytes(H, L, m->KX, O, true);
    if (imupose) {}
    else if (e == hipSuccess && smem <= 160 * 1024) e = ape_prepare_lstm_tile16(H, L, smem);
    else if (e == hipSuccess) e = ape_prepare_lstm_tile16(H, L, ape_lstm_tile16_smem_bytes(H, L, m->KX, O, false));
    if (e != hipSuccess) {
        ape_model_destroy(m);
        return ape_fail(APE_ERR_HIP, "model allocation failed: %s", hipGetErrorString(e));
    }
    if (m->caps.upper_ok) {
        e = ape_prepare_lstm_tile16_upper(H, L - 1, ape_lstm_tile16_smem_bytes(H, L - 1, H, O, true));
        if (e != hipSuccess) {
            ape_model_destroy(m);
            return ape_fail(APE_ERR_HIP, "model allocation failed: %s", hipGetErrorString(e));
        }
    }
    char nm[64];
    snprintf(nm, sizeof(nm), "ape_lstm_tile16<%d, %d, %d>", H, L, imupose ? 16 : 4);
    m->kernel_name = nm;
    snprintf(nm, sizeof(nm), "ape_lstm_cluster<%d, %d, %d", H, L, m->KX);
    m->cluster_name = nm;
    if (m->caps.cluster_ok) {
        const int GH = H / 16, max_clusters = m->caps.cluster_capacity;
        for (int l = 0; l < L && e == hipSuccess; ++l)
            e = plan((void**)&m->wcl[l], (size_t)4 * H * ((l == 0 ? m->KX : H) + H) * sizeof(float));
        const size_t cap32 = (size_t)m->caps.f16v2_capacity;
        m->hx_bytes = (size_t)max_clusters * L * 2 * GH * 64 * 16 * sizeof(float);
        // one flag per (cluster, layer, member, wave) + the ticket / departure words; on top of both what the other kernels need:
        size_t flag_words = (size_t)max_clusters * L * GH * 4;
        if (ape_upper32_supported(H, L, O)) {       // 32-row clusters x 2 sets x 2 parities x 32 KB; one flag per (cluster, set, member wave)
            m->hx_bytes = std::max(m->hx_bytes, cap32 * 2 * 2 * 32768);
            flag_words = std::max(flag_words, cap32 * 2 * 32);
        }
        // fp16 v2 kernel: per (32-row cluster, row set, member wave), 64 flags per cluster and set in the 16-member form
        if (ape_cluster_f16v2_supported(H, L, m->KX)) flag_words = std::max(flag_words, cap32 * 2 * 64);
        // (second-generation kernel of the 3 x 128 model: one flag per (32-row cluster, layer, member, one of eight waves))
        if (ape_cluster16_supported(H, L, m->KX)) flag_words = std::max(flag_words, cap32 * L * 64);
        if (ape_upper128_supported(H, L, O) && !imupose) {
            flag_words = std::max(flag_words, (size_t)ape_upper128_flag_words(m->caps.up128_classes));
            m->hx_bytes = std::max(m->hx_bytes, (size_t)ape_upper128_hx_bytes(m->caps.up128_classes));
        }
        m->xflag_bytes = ((flag_words * sizeof(unsigned)) + 15) / 16 * 16 + 16;
        if (e == hipSuccess) e = plan((void**)&m->hx, m->hx_bytes);
        if (e == hipSuccess) e = plan((void**)&m->dbg_wg, 256 * 8 * sizeof(unsigned long long));
        if (e == hipSuccess) e = plan((void**)&m->xflags, m->xflag_bytes + 256);
        if (e == hipSuccess) e = plan((void**)&m->xcc_slots, APE_XCC_WORDS * sizeof(unsigned));
        m->hxs_bytes = (size_t)L * 2 * 4 * H * 8;
        if (e == hipSuccess) e = plan((void**)&m->hxs, 256 + m->hxs_bytes);
        for (int l = 0; l < L && e == hipSuccess && !imupose; ++l)
            e = plan(&m->wcl16[l], (size_t)4 * H * ((l == 0 ? m->KX : H) + H) * sizeof(_Float16));
        if (e == hipSuccess) e = ape_prepare_lstm_cluster(H, L, m->KX);
        if (e == hipSuccess && ((H == 128 && L == 3) || (H == 256 && L == 2 && m->KX == 32)))
            e = ape_prepare_lstm_cluster(H, 1, m->KX);       // layer 0 alone: launch A of a Monte-Carlo bank
        if (e == hipSuccess && !imupose) e = ape_prepare_lstm_cluster_f16(H, L, m->KX);
        if (e == hipSuccess && !imupose) e = ape_prepare_lstm_cluster_f16v2(H, L, m->KX);
        // latency kernel with H/8 members (every CU of a 32-CU XCD at H = 256): only where an XCD has that many CUs
        if (m->n_cus / 8 >= H / 8 && !imupose) {
            for (int l = 0; l < L && e == hipSuccess; ++l)
                e = plan((void**)&m->wcls[l], (size_t)4 * H * ((l == 0 ? m->KX : H) + H) * sizeof(float));
            m->small_uw = 2;
        }
        if (m->caps.mc_small) {
            for (int l = 1; l < L && e == hipSuccess; ++l) e = plan((void**)&m->wmc[l], (size_t)8 * H * H * sizeof(float));
            for (int l = 1; l < L && e == hipSuccess; ++l) e = plan((void**)&m->wmc16[l], (size_t)8 * H * H * sizeof(float));
            m->gxm_cluster_bytes = ape_mc_small_cluster_bytes(H, L);
            if (e == hipSuccess) e = plan((void**)&m->gxm, 256 + 8 * m->gxm_cluster_bytes + 8 * 64 * 8);      // + the feature granules of 8 streams
            if (e == hipSuccess) e = ape_prepare_lstm_mc_small(H, L, m->KX);
        }
        if (m->caps.c32) {
            for (int l = 0; l < L && e == hipSuccess; ++l)
                e = plan((void**)&m->wcl32[l], (size_t)4 * H * ((l == 0 ? m->KX : H) + H) * sizeof(float));
            for (int l = 0; l < L && e == hipSuccess; ++l)         // the f16 hi / lo image of lstm_cluster32.hip (same size, pack_c32_split)
                e = plan((void**)&m->wcl32s[l], (size_t)4 * H * ((l == 0 ? m->KX : H) + H) * sizeof(float));
            if (e == hipSuccess) e = ape_prepare_lstm_cluster32(H, L, m->KX);
            if (e == hipSuccess && m->caps.up32) e = ape_prepare_lstm_upper32();
        }
        if (m->caps.split32) {
            for (int l = 0; l < L && e == hipSuccess; ++l)
                e = plan((void**)&m->wcl32[l], (size_t)4 * H * (H + H) * sizeof(float));
            if (e == hipSuccess) e = ape_prepare_lstm_upper32();
            m->caps.split32 = (e == hipSuccess);
        }
        if (m->caps.up128) {
            for (int l = 1; l < L && e == hipSuccess; ++l) e = plan((void**)&m->wup128[l], (size_t)4 * H * 2 * H * sizeof(float));
            if (e == hipSuccess) e = ape_prepare_lstm_upper128();
        }
        if (m->caps.c16) {
            if (e == hipSuccess) e = ape_prepare_lstm_cluster16(H, L, m->KX);
            if (e == hipSuccess && m->caps.lv16) {
                m->gx16_bytes = ape_level16_gx_bytes(m->n_cus);
                e = plan((void**)&m->gx16, 256 + m->gx16_bytes);
                if (e == hipSuccess) e = ape_prepare_lstm_level16(H, L, m->KX);
                m->caps.lv16 = (e == hipSuccess);
            }
        }
        if (e != hipSuccess) {
            ape_model_destroy(m);
            return ape_fail(APE_ERR_HIP, "cluster kernel set-up failed: %s", hipGetErrorString(e));
        }
    }
    e = commit_plan();
    if (e != hipSuccess) {
        ape_model_destroy(m);
        return ape_fail(APE_ERR_HIP, "model allocation failed: %s", hipGetErrorString(e));
    }
    *out = m;
    return APE_OK;
}

int ape_model_destroy(ape_model_t* m) {
    if (!m) return APE_OK;
    (void)hipSetDevice(m->dims.device);
    if (m->slab) (void)hipFree(m->slab);             // weights, packs, statistics, exchange buffers, flags: one allocation
    if (m->y_ws) (void)hipFree(m->y_ws);             // workspaces grow on demand and are their own allocations
    if (m->z_ws) (void)hipFree(m->z_ws);
    if (m->zfrag_ws) (void)hipFree(m->zfrag_ws);
    if (m->hfrag_ws) (void)hipFree(m->hfrag_ws);
    if (m->ypart_ws) (void)hipFree(m->ypart_ws);
    if (m->hseq_ws) (void)hipFree(m->hseq_ws);
    delete m;
    return APE_OK;
}

int ape_model_reserve(ape_model_t* m, int32_t max_batch) {
    if (!m || max_batch < 1) return ape_fail(APE_ERR_INVALID_ARG, "reserve: bad arguments");
    if (max_batch <= m->y_cap) return APE_OK;
    APE_TRY(hipSetDevice(m->dims.device));
    if (m->y_ws) { APE_TRY(hipFree(m->y_ws)); m->y_ws = nullptr; m->y_cap = 0; }
    APE_TRY(hipMalloc((void**)&m->y_ws, (size_t)max_batch * m->dims.output_size * sizeof(float)));
    m->y_cap = max_batch;
    return APE_OK;
}

// Pack [W_ih | W_hh] of one layer into the order the kernel's waves stream it:
//   packed[((w*Q + q)*NT + n)*64 + lane][j] = Wcat[gate*H + w*H/4 + u*16 + (lane&15)][16q + 4(lane>>4) + j]
// with n = gate*UB + u, Wcat columns = input part zero-padded to KXl, then the recurrent part.
int ape_model_load_weights(ape_model_t* m, const float* blob, size_t n_floats) {
    if (!m || !blob) return ape_fail(APE_ERR_INVALID_ARG, "load_weights: NULL argument");
    const size_t want = ape_weight_blob_floats(&m->dims);
    if (n_floats != want) return ape_fail(APE_ERR_INVALID_ARG, "weight blob has %zu floats, expected %zu", n_floats, want);
    APE_TRY(hipSetDevice(m->dims.device));
    std::vector<float> host(n_floats);
    APE_TRY(hipMemcpy(host.data(), blob, n_floats * sizeof(float), hipMemcpyDefault));   // host or device source

    const int H = m->dims.hidden_size, L = m->dims.num_layers, O = m->dims.output_size, I = m->dims.input_size;
    const int UB = H / 64, NT = 4 * UB;
    const float* cur = host.data();
    if (m->dims.model_kind == APE_MODEL_FF || m->dims.model_kind == APE_MODEL_IMUPOSE) {
        // per layer [wave 4][k-block q][tile n][lane][4]: lane holds W[w*H/4 + n*16 + (lane&15)][16q + 4(lane>>4) + j]
        const int NTF = H / 64;
        const bool pre_only = m->dims.model_kind == APE_MODEL_IMUPOSE;      // just the input layer, then the LSTM below
        for (int j = 0; j <= (pre_only ? 0 : L); ++j) {
            const int in_j = (j == 0) ? I : H, K = (j == 0) ? (pre_only ? m->KXpre : m->KX) : H, Q = K / 16;
            const float* wj = cur;  cur += (size_t)H * in_j;
            const float* bj = cur;  cur += H;
            std::vector<float> packed((size_t)K * H);
            for (int w = 0; w < 4; ++w)
                for (int q = 0; q < Q; ++q)
                    for (int n = 0; n < NTF; ++n)
                        for (int lane = 0; lane < 64; ++lane) {
                            const int col = w * (H / 4) + n * 16 + (lane & 15);
                            for (int jj = 0; jj < 4; ++jj) {
                                const int k = 16 * q + 4 * (lane >> 4) + jj;
                                packed[((((size_t)w * Q + q) * NTF + n) * 64 + lane) * 4 + jj] =
                                    (k < in_j) ? wj[(size_t)col * in_j + k] : 0.0f;
                            }
                        }
            APE_TRY(hipMemcpy(m->ff_wpack[j], packed.data(), packed.size() * sizeof(float), hipMemcpyHostToDevice));
            APE_TRY(hipMemcpy(m->ff_bias[j], bj, H * sizeof(float), hipMemcpyHostToDevice));
        }
        if (!pre_only && m->ffp_ok) {
            // mlp_pipe.hip: v_mfma_f32_32x32x2_f32 A fragments, register 4 kb + j of lane (unit column = lane & 31, hh = lane >> 5) =
            // W[64 wave + 32 ct + (lane & 31)][8 kb + 4 hh + j]; [wave][ct][kb][lane][4]
            const float* wl[3];
            int inl[3], kbl[3];
            const float* c2 = host.data();
            for (int j = 0; j <= 2; ++j) { inl[j] = (j == 0) ? I : H; kbl[j] = (j == 0) ? m->KX / 8 : H / 8; wl[j] = c2; c2 += (size_t)H * inl[j] + H; }
            const float* w_out_h = c2;
            float* dst[3] = {m->ffp_wa0, m->ffp_wa1, m->ffp_wb2};
            for (int j = 0; j <= 2; ++j) {
                std::vector<float> pk((size_t)4 * 2 * kbl[j] * 64 * 4);
                for (int w = 0; w < 4; ++w)
                    for (int ct = 0; ct < 2; ++ct)
                        for (int kb = 0; kb < kbl[j]; ++kb)
                            for (int lane = 0; lane < 64; ++lane)
                                for (int jj = 0; jj < 4; ++jj) {
                                    const int unit = 64 * w + 32 * ct + (lane & 31), k = 8 * kb + 4 * (lane >> 5) + jj;
                                    pk[((((size_t)w * 2 + ct) * kbl[j] + kb) * 64 + lane) * 4 + jj] = (k < inl[j]) ? wl[j][(size_t)unit * inl[j] + k] : 0.0f;
                                }
                APE_TRY(hipMemcpy(dst[j], pk.data(), pk.size() * sizeof(float), hipMemcpyHostToDevice));
            }
            std::vector<float> po((size_t)4 * 8 * 64 * 4);
            for (int w = 0; w < 4; ++w)
                for (int kb = 0; kb < 8; ++kb)
                    for (int lane = 0; lane < 64; ++lane)
                        for (int jj = 0; jj < 4; ++jj) {
                            const int o = lane & 31, k = 64 * w + 8 * kb + 4 * (lane >> 5) + jj;
                            po[(((size_t)w * 8 + kb) * 64 + lane) * 4 + jj] = (o < O) ? w_out_h[(size_t)o * H + k] : 0.0f;
                        }
            APE_TRY(hipMemcpy(m->ffp_wbo, po.data(), po.size() * sizeof(float), hipMemcpyHostToDevice));
        }
        if (!pre_only) {
            APE_TRY(hipMemcpy(m->w_out, cur, (size_t)O * H * sizeof(float), hipMemcpyHostToDevice));
            cur += (size_t)O * H;
            APE_TRY(hipMemcpy(m->b_out, cur, O * sizeof(float), hipMemcpyHostToDevice));
            m->has_weights = true;
            return APE_OK;
        }
    }
    for (int l = 0; l < L; ++l) {
        const int in_l = (l == 0) ? m->lstm_in : H;
        const int KXl = (l == 0) ? m->KX : H;
        const int Q = (KXl + H) / 16;
        const float* w_ih = cur;  cur += (size_t)4 * H * in_l;
        const float* w_hh = cur;  cur += (size_t)4 * H * H;
        const float* b_ih = cur;  cur += 4 * H;
        const float* b_hh = cur;  cur += 4 * H;
        std::vector<float> packed((size_t)4 * Q * NT * 64 * 4);
        for (int w = 0; w < 4; ++w)
            for (int q = 0; q < Q; ++q)
                for (int n = 0; n < NT; ++n) {
                    const int gate = n / UB, u = n % UB;
                    for (int lane = 0; lane < 64; ++lane) {
                        const int row = gate * H + w * (H / 4) + u * 16 + (lane & 15);
                        float* dst = &packed[((((size_t)w * Q + q) * NT + n) * 64 + lane) * 4];
                        for (int j = 0; j < 4; ++j) {
                            const int k = 16 * q + 4 * (lane >> 4) + j;
                            float v;
                            if (k < KXl) v = (k < in_l) ? w_ih[(size_t)row * in_l + k] : 0.0f;
                            else v = w_hh[(size_t)row * H + (k - KXl)];
                            dst[j] = v;
                        }
                    }
                }
        if (m->caps.cluster_ok) {
            // cluster kernel: [member GH][wave 4][i/4][lane][i%4] with i = 4q + j; lane = (g << 4) | (u << 2) | gate holds
            // Wcat[gate*H + member*16 + wave*4 + u][16q + 4g + j] -- the register file of that wave
            const int GH = H / 16, NW = (KXl + H) / 4;
            std::vector<float> pc((size_t)GH * 4 * NW * 64);
            for (int mem = 0; mem < GH; ++mem)
                for (int w = 0; w < 4; ++w)
                    for (int i = 0; i < NW; ++i)
                        for (int lane = 0; lane < 64; ++lane) {
                            const int c = lane & 15, g = lane >> 4, u = c >> 2, gate = c & 3;   // tile row = unit*4 + gate
                            const int row = gate * H + mem * 16 + w * 4 + u;
                            const int k = 16 * (i / 4) + 4 * g + (i % 4);
                            float v;
                            if (k < KXl) v = (k < in_l) ? w_ih[(size_t)row * in_l + k] : 0.0f;
                            else v = w_hh[(size_t)row * H + (k - KXl)];
                            // register i of that lane; stored [k-quad i/4][lane][i%4] so a lane fetches 4 registers per load
                            pc[((((size_t)(mem * 4 + w) * (NW / 4)) + i / 4) * 64 + lane) * 4 + (i % 4)] = v;
                        }
            APE_TRY(hipMemcpy(m->wcl[l], pc.data(), pc.size() * sizeof(float), hipMemcpyHostToDevice));
            if (m->small_uw == 2) {
                // latency kernel, H/8 members: a wave owns 2 units = 8 columns, 8 k-groups; lane = (g << 3) | (u << 2) | gate holds
                // Wcat[gate*H + (member*4 + wave)*2 + u][32q + 4g + j] in register 4q + j; same [i/4][lane][i%4] storage
                const int GS = H / 8, NWS = (KXl + H) / 8;
                std::vector<float> ps((size_t)GS * 4 * NWS * 64);
                for (int mem = 0; mem < GS; ++mem)
                    for (int w = 0; w < 4; ++w)
                        for (int i = 0; i < NWS; ++i)
                            for (int lane = 0; lane < 64; ++lane) {
                                const int c = lane & 7, g = lane >> 3, u = c >> 2, gate = c & 3;
                                const int row = gate * H + (mem * 4 + w) * 2 + u;
                                const int k = 32 * (i / 4) + 4 * g + (i % 4);
                                float v;
                                if (k < KXl) v = (k < in_l) ? w_ih[(size_t)row * in_l + k] : 0.0f;
                                else v = w_hh[(size_t)row * H + (k - KXl)];
                                ps[((((size_t)(mem * 4 + w) * (NWS / 4)) + i / 4) * 64 + lane) * 4 + (i % 4)] = v;
                            }
                APE_TRY(hipMemcpy(m->wcls[l], ps.data(), ps.size() * sizeof(float), hipMemcpyHostToDevice));
            }
            if (m->caps.mc_small && l >= 1) {
                // Monte-Carlo latency kernel, layers above layer 0 (v_mfma_f32_4x4x1_16b_f32): H/8 members x 4 waves, wave w = K quarter w of
                // [W_ih | W_hh]; lane = (block b = lane >> 2: unit b & 7 of the member, k slice ks = b >> 3; gate = lane & 3) holds
                // Wcat[gate*H + member*8 + (b & 7)][w*H/2 + 8 (i/4) + 4 ks + (i%4)] in register i; stored [member][wave][i/4][lane][i%4]
                const int GM = H / 8, NI4 = H / 4;
                std::vector<float> pm((size_t)GM * 4 * NI4 * 64);
                for (int mem = 0; mem < GM; ++mem)
                    for (int w = 0; w < 4; ++w)
                        for (int i = 0; i < NI4; ++i)
                            for (int lane = 0; lane < 64; ++lane) {
                                const int gate = lane & 3, ub = (lane >> 2) & 7, ks = lane >> 5;
                                const int row = gate * H + mem * 8 + ub;
                                const int k = w * (H / 2) + 8 * (i / 4) + 4 * ks + (i % 4);
                                pm[((((size_t)(mem * 4 + w) * (NI4 / 4)) + i / 4) * 64 + lane) * 4 + (i % 4)] =
                                    k < H ? w_ih[(size_t)row * H + k] : w_hh[(size_t)row * H + (k - H)];
                            }
                APE_TRY(hipMemcpy(m->wmc[l], pm.data(), pm.size() * sizeof(float), hipMemcpyHostToDevice));
                // ... and the 16 x 16 x 4 image of its 16-row form: wave = (column tile ct = w & 1, K half kh = w >> 1); lane = (g << 4) | (u << 2) |
                // gate holds Wcat[gate*H + member*8 + ct*4 + u][kh*H + 16q + 4g + j] in register 4q + j; stored [member][wave][q][lane][4]
                const int NQm = H / 16;
                for (int mem = 0; mem < GM; ++mem)
                    for (int w = 0; w < 4; ++w)
                        for (int q = 0; q < NQm; ++q)
                            for (int lane = 0; lane < 64; ++lane) {
                                const int c = lane & 15, g = lane >> 4, u = c >> 2, gate = c & 3, ct = w & 1, kh = w >> 1;
                                const int row = gate * H + mem * 8 + ct * 4 + u;
                                for (int j = 0; j < 4; ++j) {
                                    const int k = 16 * q + 4 * g + j;
                                    pm[((((size_t)(mem * 4 + w) * NQm) + q) * 64 + lane) * 4 + j] =
                                        kh == 0 ? w_ih[(size_t)row * H + k] : w_hh[(size_t)row * H + k];
                                }
                            }
                APE_TRY(hipMemcpy(m->wmc16[l], pm.data(), pm.size() * sizeof(float), hipMemcpyHostToDevice));
            }
            // fp16 variant: [member][wave][32-deep k-block q][lane][8]: lane holds Wcat[row][32q + 8g + j] as binary16
            const int NB = (KXl + H) / 32;
            std::vector<_Float16> ph((size_t)GH * 4 * NB * 64 * 8);
            for (int mem = 0; mem < GH; ++mem)
                for (int w = 0; w < 4; ++w)
                    for (int q = 0; q < NB; ++q)
                        for (int lane = 0; lane < 64; ++lane) {
                            const int c = lane & 15, g = lane >> 4, u = c >> 2, gate = c & 3;
                            const int row = gate * H + mem * 16 + w * 4 + u;
                            for (int j = 0; j < 8; ++j) {
                                const int k = 32 * q + 8 * g + j;
                                float v;
                                if (k < KXl) v = (k < in_l) ? w_ih[(size_t)row * in_l + k] : 0.0f;
                                else v = w_hh[(size_t)row * H + (k - KXl)];
                                ph[((((size_t)(mem * 4 + w) * NB) + q) * 64 + lane) * 8 + j] = (_Float16)v;
                            }
                        }
            if (m->wcl16[l]) APE_TRY(hipMemcpy(m->wcl16[l], ph.data(), ph.size() * sizeof(_Float16), hipMemcpyHostToDevice));
        }
        if (m->wcl32[l] != nullptr) {
            // second-generation f32 cluster kernel (v_mfma_f32_32x32x2_f32, weights = A operand): 8 members x 4 waves, a wave owns
            // 8 units = 32 columns ordered gate * 8 + unit.  [member][wave][i / 4][lane][i % 4] with register i = 4 kb + j of
            // lane (column m = lane & 31, half hh = lane >> 5) = Wcat[gate(m) * H + member*32 + wave*8 + (m & 7)][8 kb + 4 hh + j]
            const int NW = (KXl + H) / 2;                   // registers per lane: 32 columns x K / 64 lanes
            std::vector<float> pc((size_t)8 * 4 * NW * 64);
            for (int mem = 0; mem < 8; ++mem)
                for (int w = 0; w < 4; ++w)
                    for (int i = 0; i < NW; ++i)
                        for (int lane = 0; lane < 64; ++lane) {
                            const int mcol = lane & 31, hh = lane >> 5;
                            const int row = (mcol >> 3) * H + mem * 32 + w * 8 + (mcol & 7);
                            const int k = 8 * (i / 4) + 4 * hh + (i % 4);
                            float v;
                            if (k < KXl) v = (k < in_l) ? w_ih[(size_t)row * in_l + k] : 0.0f;
                            else v = w_hh[(size_t)row * H + (k - KXl)];
                            pc[((((size_t)(mem * 4 + w) * (NW / 4)) + i / 4) * 64 + lane) * 4 + (i % 4)] = v;
                        }
            APE_TRY(hipMemcpy(m->wcl32[l], pc.data(), pc.size() * sizeof(float), hipMemcpyHostToDevice));
        }
        if (m->wcl32s[l] != nullptr) {
            std::vector<unsigned> ps((size_t)8 * 4 * ((KXl + H) / 2) * 64);
            const int S = pack_c32_split(w_ih, in_l, w_hh, H, KXl, l == 0 ? KXl : 0, ps.data());
            if (l == 0) m->caps.c32 = true;        // (weights that refuse the split keep the model off lstm_cluster32.hip)
            if (S < 0) m->caps.c32 = false;
            else {
                m->c32_scale[l] = std::ldexp(1.0f, S);
                m->c32_descale[l] = std::ldexp(1.0f, -S);
                APE_TRY(hipMemcpy(m->wcl32s[l], ps.data(), ps.size() * sizeof(unsigned), hipMemcpyHostToDevice));
            }
        }
        if (m->caps.up128 && l >= 1) {
            // lstm_upper128.hip: four members x 4 waves, a wave owns 8 units = 32 columns ordered gate * 8 + unit (v_mfma_f32_32x32x2_f32,
            // weights = A operand); register i = 4 kb + j of lane (column mcol = lane & 31, half hh) = Wcat[gate(mcol) * H + member*32 +
            // wave*8 + (mcol & 7)][8 kb + 4 hh + j]; [member][wave][i / 4][lane][i % 4]
            const int NW = (KXl + H) / 2;
            std::vector<float> pc((size_t)4 * 4 * NW * 64);
            for (int mem = 0; mem < 4; ++mem)
                for (int w = 0; w < 4; ++w)
                    for (int i = 0; i < NW; ++i)
                        for (int lane = 0; lane < 64; ++lane) {
                            const int mcol = lane & 31, hh = lane >> 5;
                            const int row = (mcol >> 3) * H + mem * 32 + w * 8 + (mcol & 7);
                            const int k = 8 * (i / 4) + 4 * hh + (i % 4);
                            pc[((((size_t)(mem * 4 + w) * (NW / 4)) + i / 4) * 64 + lane) * 4 + (i % 4)] =
                                k < KXl ? w_ih[(size_t)row * in_l + k] : w_hh[(size_t)row * H + (k - KXl)];
                        }
            APE_TRY(hipMemcpy(m->wup128[l], pc.data(), pc.size() * sizeof(float), hipMemcpyHostToDevice));
        }
        std::vector<float> bsum(4 * H);
        for (int i = 0; i < 4 * H; ++i) bsum[i] = b_ih[i] + b_hh[i];
        APE_TRY(hipMemcpy(m->wpack[l], packed.data(), packed.size() * sizeof(float), hipMemcpyHostToDevice));
        APE_TRY(hipMemcpy(m->bias[l], bsum.data(), bsum.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    APE_TRY(hipMemcpy(m->w_out, cur, (size_t)O * H * sizeof(float), hipMemcpyHostToDevice));
    cur += (size_t)O * H;
    APE_TRY(hipMemcpy(m->b_out, cur, O * sizeof(float), hipMemcpyHostToDevice));
    m->has_weights = true;
    return APE_OK;
}

int ape_model_set_norm_stats(ape_model_t* m, const double* xx_m, const double* xx_s, const double* yy_m,
                             const double* yy_s) {
    if (!m || !xx_m || !xx_s || !yy_m || !yy_s) return ape_fail(APE_ERR_INVALID_ARG, "set_norm_stats: NULL argument");
    const int I = m->dims.input_size, O = m->dims.output_size;
    std::vector<double> h(3 * I + 2 * O);
    for (int i = 0; i < I; ++i) h[2 * I + 2 * O + i] = 1.0 / xx_s[i];     // reciprocal for the in-kernel z-score
    memcpy(&h[0], xx_m, I * sizeof(double));
    memcpy(&h[I], xx_s, I * sizeof(double));
    memcpy(&h[2 * I], yy_m, O * sizeof(double));
    memcpy(&h[2 * I + O], yy_s, O * sizeof(double));
    APE_TRY(hipSetDevice(m->dims.device));
    APE_TRY(hipMemcpy(m->stats, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice));
    m->has_stats = true;
    return APE_OK;
}

int ape_model_set_body(ape_model_t* m, const double body9[9]) {
    if (!m || !body9) return ape_fail(APE_ERR_INVALID_ARG, "set_body: NULL argument");
    memcpy(m->body, body9, 9 * sizeof(double));
    return APE_OK;
}

// the post-filter ape_infer wants behind the regressor: the latency kernel runs it in its own launch (fk_done = true), every other
// kernel leaves it to the caller
struct FkTail {
    void* est;
    int est_dtype;
    bool denormalize;
    bool done;
};

// Monte-Carlo latency kernel (lstm_mc_small.hip): n_streams windows (stream s at x + s * x_stream_stride) x n_mc dropout samples each,
// rows dealt over the 8 XCD clusters; y [n_streams * n_mc, O].  The caller has checked mc_small_fits().
static bool mc_small_fits(const ape_model* m, int n_streams, int n_mc) {
    return mc_small_fits(m->caps, m->dims, m->kernel_choice, m->precision, m->c32_on, m->replaying, n_streams, n_mc);
}
// what a host frame adds to the regressor's launch: the raw rows of the frame (feature builder workgroups)
struct McFrameParts {
    const float* raw_rows = nullptr;
    int raw_width = 0, raw_kind = 0, raw_big_endian = 0, cold = 0;
    float* ring_out = nullptr;
    size_t ring_stream_stride = 0, ring_rep_stride = 0;
    int ring_rep = 0;
};
// can the feature builder's workgroups become resident beside the clusters?  A cluster member takes a CU's worth of LDS only in the
// 16-row form; with 8-row clusters two workgroups share a CU, and the 3 x 128 model leaves half the CUs free anyway
static bool mc_small_builder_fits(const ape_model* m, int n_streams, int n_mc, int T) {
    const int cps = 8 / n_streams;
    // (8-row clusters: 39 KB of B tiles and sums + 0.5 KB of mask bits per step + 10.5 KB static per member -- two workgroups per CU up to T = 32)
    return m->dims.hidden_size == 128 || ((n_mc + cps - 1) / cps <= 8 && T <= 32);
}
static int mc_small_launch(ape_model_t* m, const float* x, size_t x_stream_stride, int n_streams, int n_mc, int T, uint32_t flags,
                           const float* masks_dev, float dropout_p, uint64_t seed, float* y_dev, void* stream, int x_ring,
                           const McFrameParts* fr = nullptr) {
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
static int lstm_forward_impl(ape_model_t* m, const float* x_dev, int32_t B, int32_t T, uint32_t flags,
                             const float* masks_dev, float dropout_p, uint64_t seed, float* y_dev, void* stream,
                             int x_ring, const float* h0_dev = nullptr, const float* c0_dev = nullptr, FkTail* fk = nullptr,
                             long long row_base = 0) {
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
            hipError_t e2 = ape_launch_mlp_pipe(q, m->ffp_wa0, m->ffp_wa1, m->ffp_wb2, m->ffp_wbo, m->ffp_ring, m->ffp_ring_bytes, m->ffp_ctl,
                                               m->n_cus, (hipStream_t)stream);
            if (e2 != hipSuccess) return ape_fail(APE_ERR_HIP, "mlp pipeline launch failed: %s", hipGetErrorString(e2));
            return APE_OK;
        }
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

int ape_model_set_kernel(ape_model_t* m, int32_t choice) {
    if (!m) return ape_fail(APE_ERR_INVALID_ARG, "set_kernel: NULL model");
    if (choice != APE_KERNEL_AUTO && choice != APE_KERNEL_TILE16 && choice != APE_KERNEL_CLUSTER && choice != APE_KERNEL_CLUSTER_GEN1 &&
        choice != APE_KERNEL_AUTO_GEN1)
        return ape_fail(APE_ERR_INVALID_ARG, "set_kernel: unknown choice %d", choice);
    m->c32_on = choice != APE_KERNEL_CLUSTER_GEN1 && choice != APE_KERNEL_AUTO_GEN1;
    m->ffp_on = choice != APE_KERNEL_TILE16;           // (MLP regressor: TILE16 pins the tile kernel)
    if (choice == APE_KERNEL_CLUSTER_GEN1) choice = APE_KERNEL_CLUSTER;
    if (choice == APE_KERNEL_AUTO_GEN1) choice = APE_KERNEL_AUTO;
    if (choice == APE_KERNEL_CLUSTER && !m->caps.cluster_ok)
        return ape_fail(APE_ERR_UNSUPPORTED, "set_kernel: no cluster kernel for H=%d L=%d on a device with %d CUs (a cluster "
                    "needs %d)", m->dims.hidden_size, m->dims.num_layers, m->n_cus, m->dims.hidden_size / 16);
    m->kernel_choice = choice;
    m->small_batch_path = (choice == APE_KERNEL_AUTO);
    return APE_OK;
}

int ape_model_set_precision(ape_model_t* m, int32_t precision) {
    if (!m) return ape_fail(APE_ERR_INVALID_ARG, "set_precision: NULL model");
    if (precision != APE_PRECISION_F32 && precision != APE_PRECISION_F16 && precision != APE_PRECISION_F16_GEN1)
        return ape_fail(APE_ERR_INVALID_ARG, "set_precision: unknown precision %d", precision);
    m->f16_v2 = precision != APE_PRECISION_F16_GEN1;
    if (precision == APE_PRECISION_F16_GEN1) precision = APE_PRECISION_F16;
    if (precision == APE_PRECISION_F16 && (!m->caps.cluster_ok || m->caps.wide))
        return ape_fail(APE_ERR_UNSUPPORTED, "set_precision: no fp16 kernel for H=%d L=%d", m->dims.hidden_size,
                    m->dims.num_layers);
    m->precision = precision;
    return APE_OK;
}

// the blocking part both ape_model_check and ape_model_recover share: 0 = no aborted launch since the last check; else the
// handle has been reset and g_err describes what happened
static int check_and_reset(ape_model_t* m);

int ape_model_check(ape_model_t* m) {
    if (!m) return ape_fail(APE_ERR_INVALID_ARG, "check: NULL model");
    const int rc = check_and_reset(m);
    if (rc != APE_OK && rc != APE_ERR_INVALID_ARG) {
        m->stats_counts.aborted_checks += 1;
        m->stats_counts.lost_calls += (uint64_t)m->journal_n + (m->journal_overflow ? 1u : 0u);
    }
    journal_clear(m);
    return rc;
}

int ape_model_stats(const ape_model_t* m, ape_model_stats_t* out) {
    if (!m || !out) return ape_fail(APE_ERR_INVALID_ARG, "stats: NULL argument");
    *out = m->stats_counts;
    return APE_OK;
}

static int replay_entry(ape_model_t* m, const ApeJournalEntry& e);
// (host subset frames: the pinned words the post-filter writes behind its rows -- the model's status word, a completion word per entry --
//  and the entry's name for ape_last_error)
struct SubsetHostWords { unsigned* status_out = nullptr; unsigned* done_out = nullptr; unsigned done_val = 0; const char* what = "streams_frame_subset"; };
static int subset_regress_post(ape_streams* b, int K, uint32_t flags, void* out_dev, int out_dtype, void* stream, unsigned long long mc_call,
                               const SubsetHostWords& hw = SubsetHostWords{});

int ape_model_recover(ape_model_t* m) {
    if (!m) return ape_fail(APE_ERR_INVALID_ARG, "recover: NULL model");
    const int rc = check_and_reset(m);
    if (rc == APE_OK) { journal_clear(m); return APE_OK; }
    if (rc == APE_ERR_INVALID_ARG) return rc;
    const std::string what = g_err;
    m->stats_counts.aborted_checks += 1;
    // can every pending call be issued again?  A bank step only while it is that bank's newest step with no row behind it.
    bool ok = !m->journal_overflow;
    for (int i = 0; i < m->journal_n && ok; ++i) {
        const ApeJournalEntry& e = m->journal[i];
        if (e.kind != ApeJournalEntry::STEP) continue;
        if (e.bank->frames != e.bank_frames || e.bank->steps != e.bank_steps + 1) ok = false;
        for (int j = i + 1; j < m->journal_n; ++j)
            if (m->journal[j].kind == ApeJournalEntry::STEP && m->journal[j].bank == e.bank) ok = false;
    }
    if (!ok) {
        const int n = m->journal_n + (m->journal_overflow ? 1 : 0);
        m->stats_counts.lost_calls += (uint64_t)n;
        const bool over = m->journal_overflow;
        journal_clear(m);
        return ape_fail(APE_ERR_HIP, "%d pending call(s) could not be re-issued (%s) behind an aborted launch: %s", n,
                    over ? "more than 64 calls since the last check, or a call the journal cannot hold"
                         : "a stream bank has moved on since the aborted step", what.c_str());
    }
    m->replaying = true;
    int bad = APE_OK;
    for (int i = 0; i < m->journal_n && bad == APE_OK; ++i) {
        bad = replay_entry(m, m->journal[i]);
        if (bad == APE_OK) m->stats_counts.reissued_calls += 1;
    }
    m->replaying = false;
    const int n = m->journal_n;
    journal_clear(m);
    if (bad != APE_OK) { m->stats_counts.lost_calls += (uint64_t)n; return bad; }
    APE_TRY(hipDeviceSynchronize());
    return APE_OK;
}

static int check_and_reset(ape_model_t* m) {
    if (!m) return ape_fail(APE_ERR_INVALID_ARG, "check: NULL model");
    if (m->ffp_ok) {                                // the MLP pipeline's status word (bounded spins between its two stages)
        APE_TRY(hipSetDevice(m->dims.device));
        APE_TRY(hipDeviceSynchronize());
        unsigned st = 0;
        APE_TRY(hipMemcpy(&st, m->ffp_ctl + 8 * 16, sizeof(st), hipMemcpyDeviceToHost));
        if (st != 0) {
            APE_TRY(hipMemset(m->ffp_ctl, 0, m->ffp_ctl_words * sizeof(unsigned)));
            APE_TRY(hipDeviceSynchronize());
            return ape_fail(APE_ERR_HIP, "mlp pipeline launch aborted (status %u); outputs since the last successful check are invalid; the model "
                        "is usable again", st);
        }
    }
    if (!m->caps.cluster_ok) return APE_OK;
    APE_TRY(hipSetDevice(m->dims.device));
    // every stream of the device, non-blocking ones included: a launch that is still spinning must have ended (its
    // status word written) before the word is read, and nothing may be in flight when the flags are reset below
    APE_TRY(hipDeviceSynchronize());
    unsigned st = 0;
    APE_TRY(hipMemcpy(&st, ctl_words(m).status, sizeof(st), hipMemcpyDeviceToHost));
    if (st != 0) {
        // an aborted launch skipped its self-cleaning: reset flags, counters and the status word from the host
        APE_TRY(hipMemset(m->xflags, 0, m->xflag_bytes + 16));
        APE_TRY(hipMemset(m->xcc_slots, 0, APE_XCC_WORDS * sizeof(unsigned)));
        APE_TRY(hipMemset(m->hxs, 0, 256 + m->hxs_bytes));     // the aborted launch's granules carry tags the next launch would await
        if (m->gxm) APE_TRY(hipMemset(m->gxm, 0, 256 + 8 * m->gxm_cluster_bytes + 8 * 64 * 8));
        if (m->gx16) APE_TRY(hipMemset(m->gx16, 0, 256 + m->gx16_bytes));
        APE_TRY(hipDeviceSynchronize());
        return ape_fail(APE_ERR_HIP, "cluster kernel launch aborted (status %u: %s); outputs of every launch on this model "
                    "since the last successful check are invalid; the model is usable again", st,
                    st == 1 ? "a workgroup gave up waiting for a peer -- not all workgroups of a cluster were resident"
                    : st == 5 ? "the Monte-Carlo latency kernel gave up waiting for the members of a cluster -- not all workgroups were resident"
                    : st >= 16 ? "the Monte-Carlo latency kernel gave up waiting for a peer's values (16 + phase)"
                            : "a launch found the state of an earlier aborted launch");
    }
    return APE_OK;
}

static int fk_impl(ape_model_t* m, const void* preds_dev, int32_t preds_dtype, int32_t N, int32_t denormalize, void* est_dev,
                   int32_t est_dtype, void* stream, const FkBodyRows* bodies = nullptr);

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

static int fk_impl(ape_model_t* m, const void* preds_dev, int32_t preds_dtype, int32_t N, int32_t denormalize, void* est_dev,
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


// ---- stream bank ------------------------------------------------------------------------------------------

// (re)allocates the three rings for the bank's current S, T, smooth, n_mc
// window copies a stream keeps in the feature ring: n_mc for the LSTM banks ([S,n_mc,T,I], one window per sample row of the fused dropout
// kernels), one for DropoutFF (the trunk runs once per stream) and ImuPoseLSTM (one row per stream)
static int bank_copies(const ape_streams* b) { return b->model->dims.model_kind == APE_MODEL_LSTM ? b->n_mc : 1; }

// The regressor of a DropoutFF frame or replay chunk (ff_bank.hip): sample rows [row_base, row_base + rows) of a call whose
// global row r is sample r % n_mc of group (stream / frame) r / n_mc.  `x`: the newest feature row of group g_base + j at x + j * x_stride,
// g_base = row_base / n_mc.  The trunk once per group (ape_mlp_tile16 with hidden_out: f64 z-score, input layer, hidden layers) into
// `hid` [groups,H], then the n_mc masked heads.  No cooperative kernel: nothing here waits for another workgroup.
static int ff_bank_forward(ape_model* m, const float* x, size_t x_stride, long long row_base, int rows, int n_mc, bool norm, const float* masks,
                           float dropout_p, uint64_t seed, float* hid, float* y, void* stream, hipEvent_t ev_a = nullptr, hipEvent_t ev_z = nullptr,
                           long long philox_base = 0) {
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

static void bank_free_regressor_ws(ape_streams* b) {
    if (b->ffhid) (void)hipFree(b->ffhid);
    if (b->xwin) (void)hipFree(b->xwin);
    b->ffhid = b->xwin = nullptr;
}

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
// the subset frames' device workspaces (sized for the bank's S and n_mc); a pending subset frame of the bank can no longer be re-issued
static void subset_free(ape_streams* b) {
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
    subset_free(b);                     // (drops the bank's pending subset frame as below)
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
// (a capacity of one row holds nothing but ones: such a bank keeps its table and goes on running the forms it ran)
static bool bank_smooths_on(const ape_streams* b) { return b->smooths.on() && b->smooth > 1; }
static int bank_smooth_of(const ape_streams* b, int s) { return bank_smooths_on(b) ? b->smooths.host[(size_t)s] : b->smooth; }

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

struct McFrameParts;
static int streams_step_impl(ape_streams_t* b, uint32_t flags, void* msg_dev, void* tail_dev, int32_t out_dtype, void* stream,
                             unsigned* status_out, const McFrameParts* fuse = nullptr);

int ape_streams_step(ape_streams_t* b, uint32_t flags, void* msg_dev, void* tail_dev, int32_t out_dtype, void* stream) {
    return streams_step_impl(b, flags, msg_dev, tail_dev, out_dtype, stream, nullptr);
}

// status_out (host frames): pinned word that receives the model's sticky status word behind the step's kernels
// a few streams in Monte-Carlo mode (one estimator's frame: S = 1) step on the Monte-Carlo latency kernel
static bool bank_on_mc_small(const ape_streams* b) {
    const ape_model* m = b->model;
    return m->dims.model_kind == APE_MODEL_LSTM && !b->plan.shared_l0 && b->mc && b->dropout_p > 0.0f && m->dims.num_layers > 1 && b->S <= 8 && m->caps.cluster_ok && b->T <= 64 &&
           mc_small_fits(m, b->S, b->n_mc);
}

static int streams_step_impl(ape_streams_t* b, uint32_t flags, void* msg_dev, void* tail_dev, int32_t out_dtype, void* stream,
                             unsigned* status_out, const McFrameParts* fuse) {
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
    // measurement aid (ape_streams_profile): a pair of events around every launch of the step's dominant kernel
    auto prof_pair = [&](hipEvent_t* a, hipEvent_t* z) {
        *a = *z = nullptr;
        if (!b->prof_on || b->prof_n >= (int)b->prof_ev.size() / 2) return;
        *a = b->prof_ev[2 * b->prof_n]; *z = b->prof_ev[2 * b->prof_n + 1];
        b->prof_n += 1;
    };
    auto post_params = [&]() {
        StreamPostParams q{};
        q.y_new = b->y_new; q.yring = b->yring; q.msg = msg_dev; q.tail = tail_dev;
        q.yy_m = norm ? m->stats + 2 * m->dims.input_size : nullptr;      // one switch (estimator.py:103-109)
        q.yy_s = norm ? m->stats + 2 * m->dims.input_size + m->dims.output_size : nullptr;
        memcpy(q.body, m->body, sizeof(q.body));
        q.S = b->S; q.O = m->dims.output_size; q.W = layout_est_width(m->dims.target_layout); q.layout = m->dims.target_layout;
        q.smooth = b->smooth; q.n_mc = b->n_mc;
        q.pos = (int)(b->steps % b->smooth);
        q.cold = b->steps == 0 ? 1 : 0;
        q.msg_dtype = out_dtype; q.packed = packed ? 1 : 0;
        if (status_out != nullptr && m->caps.cluster_ok) { q.status_in = ctl_words(m).status; q.status_out = status_out; }
        if (status_out != nullptr && b->h_done != nullptr) { q.done_out = b->h_done; q.done_val = b->h_done_val; }
        q.part = b->post_part; q.part_cnt = b->post_cnt;
        return q;
    };
    if (m->dims.model_kind == APE_MODEL_FF) {
        // DropoutFF: the newest row of every stream (T = 1: slot 0) -> trunk once per stream -> n_mc masked heads -> y_new in the row
        // order the post-filter reads.  Masks keyed by (seed + frame counter; row = stream * n_mc + sample; hidden unit)
        if (!b->ffhid) return ape_fail(APE_ERR_NOT_READY, "streams_step: the bank lost its rings in a failed ape_streams_set_mc");
        if (b->inj_masks && !b->mc)
            return ape_fail(APE_ERR_UNSUPPORTED, "streams_step: injected masks (test hook) on a DropoutFF bank without ape_streams_set_mc");
        hipEvent_t ev_a, ev_z;
        prof_pair(&ev_a, &ev_z);
        if (int rc = ff_bank_forward(m, b->xring, (size_t)m->dims.input_size, 0, b->S * b->n_mc, b->n_mc, norm, b->inj_masks,
                                     b->mc ? b->dropout_p : 0.0f, b->seed + b->mc_calls, b->ffhid, b->y_new, stream, ev_a, ev_z))
            return rc;
    } else if (m->dims.model_kind == APE_MODEL_IMUPOSE) {
        // ImuPoseLSTM: the rings in time order (cold-start pad included), then the forward a subset frame runs over its compact windows
        // (x_ring = 0: the layer-split route above 512 windows applies) -- the same launches, hence the same bits
        if (!b->xwin) return ape_fail(APE_ERR_NOT_READY, "streams_step: the bank lost its rings in a failed ape_streams_set_mc");
        hipError_t e = ape_launch_ring_windows(b->xring, b->xwin, b->S, b->T, m->dims.input_size, x_ring, (hipStream_t)stream);
        if (e != hipSuccess) return ape_fail(APE_ERR_HIP, "streams_step: window launch failed: %s", hipGetErrorString(e));
        hipEvent_t ev_a, ev_z;
        prof_pair(&ev_a, &ev_z);
        if (ev_a) (void)hipEventRecord(ev_a, (hipStream_t)stream);
        if (int rc = lstm_forward_impl(m, b->xwin, b->S, b->T, flags | diag_wt, nullptr, 0.0f, 0, b->y_new, stream, 0)) return rc;
        if (ev_z) (void)hipEventRecord(ev_z, (hipStream_t)stream);
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
                hipEvent_t ev_a, ev_z;
                prof_pair(&ev_a, &ev_z);
                if (route == BANK_UPPER32) {
                    UpperParams u = upper_params(m, b->T, (rows + 31) / 32, diag_wt);
                    u.xfrag = b->xfrag; u.xfrag_bytes = ape_upper32_xfrag_bytes(rows, b->T); u.ypart = b->ypart;
                    u.w = m->wcl32[1]; u.bias = m->bias[1];
#ifdef APE_ABLATE
                    // timing experiments of the ablation library only (tests/tools/ablate_upper32.py; results are garbage)
                    if (const char* ab = getenv("APE_UP32_ABLATE")) u.flags = (unsigned)strtoul(ab, nullptr, 0);
#endif
                    m->last_kernel = "ape_lstm_upper32";
                    e = ape_launch_lstm_upper32(u, xq, m->b_out, b->y_new + (size_t)r0 * O, m->caps.f16v2_capacity, (hipStream_t)stream, ev_a, ev_z);
                } else {
                    // the 3 x 128 model: layers 1 and 2 on the four-member clusters of lstm_upper128.hip, with layer 1's keep bits
                    Upper128Params u = upper_params<Upper128Params>(m, b->T, (rows + 31) / 32, diag_wt);
                    u.xfrag = b->xfrag; u.xfrag_bytes = ape_upper128_xfrag_bytes(rows, b->T); u.maskbits = b->maskbits; u.ypart = b->ypart;
                    u.w[0] = m->wup128[1]; u.w[1] = m->wup128[2]; u.bias[0] = m->bias[1]; u.bias[1] = m->bias[2]; u.dropout_p = b->dropout_p;
                    m->last_kernel = "ape_lstm_upper128";
                    e = ape_launch_lstm_upper128(u, xq, m->b_out, b->y_new + (size_t)r0 * O, m->caps.up128_classes, (hipStream_t)stream, ev_a, ev_z);
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
        hipEvent_t ev_a, ev_z;
        prof_pair(&ev_a, &ev_z);
        if (ev_a) (void)hipEventRecord(ev_a, (hipStream_t)stream);
        m->last_kernel = "ape_lstm_tile16";
        e = ape_launch_lstm_tile16(H, LU, q, (hipStream_t)stream);
        if (ev_z) (void)hipEventRecord(ev_z, (hipStream_t)stream);
        if (e != hipSuccess) return ape_fail(APE_ERR_HIP, "streams_step: upper-layer launch failed: %s", hipGetErrorString(e));
        }
    } else if (bank_on_mc_small(b)) {
        // a few streams in Monte-Carlo mode (one estimator's frame: S = 1): the latency kernel reads the first copy of every
        // stream's window and deals the sample rows over the XCDs; from ape_streams_frame_host the feature builder rides in the same
        // launch as extra workgroups (`fuse`: the row has NOT been pushed by a launch of its own)
        if (!m->has_weights) return ape_fail(APE_ERR_NOT_READY, "streams_step: weights not loaded");
        McFrameParts fr{};
        if (fuse) fr = *fuse;
        hipEvent_t ev_a, ev_z;
        prof_pair(&ev_a, &ev_z);
        if (ev_a) (void)hipEventRecord(ev_a, (hipStream_t)stream);
        if (int rc = mc_small_launch(m, b->xring, (size_t)b->n_mc * b->T * m->dims.input_size, b->S, b->n_mc, b->T,
                                     flags | diag_wt | (b->inj_masks ? APE_FLAG_DROPOUT_MASKS : APE_FLAG_DROPOUT_PHILOX), b->inj_masks,
                                     b->dropout_p, b->seed + b->mc_calls, b->y_new, stream, x_ring, &fr))
            return rc;
        if (ev_z) (void)hipEventRecord(ev_z, (hipStream_t)stream);
    } else {
        hipEvent_t ev_a, ev_z;
        prof_pair(&ev_a, &ev_z);
        if (ev_a) (void)hipEventRecord(ev_a, (hipStream_t)stream);
        if (int rc = lstm_forward_impl(m, b->xring, b->S * b->n_mc, b->T,
                                       flags | diag_wt | (!drop ? 0u : b->inj_masks ? APE_FLAG_DROPOUT_MASKS : APE_FLAG_DROPOUT_PHILOX),
                                       drop ? b->inj_masks : nullptr, drop ? b->dropout_p : 0.0f, b->seed + b->mc_calls, b->y_new, stream, x_ring))
            return rc;
        if (ev_z) (void)hipEventRecord(ev_z, (hipStream_t)stream);
    }
    ++b->mc_calls;       // (every branch above enqueued one forward under seed + mc_calls)
    StreamPostParams q = post_params();
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

// One iteration of Estimator.processing_loop (estimator.py:174-177) for every stream of the bank, HOST buffers in and out.
// The raw rows are copied into pinned, device-visible staging the feature builder reads directly; the post kernel writes the
// datagram rows and the model's status word straight into pinned host memory: the frame holds no copy command, just the
// step's kernels and one stream synchronisation.  An aborted cooperative launch is recovered here (ape_model_recover).
// The frame call polls words the device writes into pinned memory (h_done, h_status) and reads h_out without a stream synchronisation:
// the buffers are APE_PINNED (bank_host.h).
static inline double now_us() {
    return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

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
    if (rows_bytes > b->h_rows_bytes) {
        if (b->h_rows) { APE_TRY(hipHostFree(b->h_rows)); b->h_rows = nullptr; b->h_rows_bytes = 0; }
        APE_TRY(hipHostMalloc((void**)&b->h_rows, rows_bytes, APE_PINNED));
        b->h_rows_bytes = rows_bytes;
    }
    if (out_bytes > b->h_out_bytes) {
        if (b->h_out) { APE_TRY(hipHostFree(b->h_out)); b->h_out = nullptr; b->h_out_bytes = 0; }
        APE_TRY(hipHostMalloc(&b->h_out, out_bytes, APE_PINNED));
        b->h_out_bytes = out_bytes;
    }
    APE_TRY(ape_pinned_zeroed(&b->h_status, 64));
    // up to 64 streams: a word per stream that the post kernel's workgroup writes behind its outputs -- the host takes the frame when
    // all are there instead of waiting for the stream's completion signal to travel (a larger bank waits for the stream)
    if (b->S <= 64) APE_TRY(ape_pinned_zeroed(&b->h_done, 64 * sizeof(unsigned)));
    ape_done_next(&b->h_done_val);
    const double t_begin = now_us();
    memcpy(b->h_rows, rows_host, rows_bytes);
    // (a sentinel, not zero: in the single-launch frame an aborted launch never reaches the tail that writes the word)
    *b->h_status = m->caps.cluster_ok ? 0xFFFFFFFFu : 0u;       // (no cooperative kernel on this model: nothing writes the word, nothing can abort)
    // where the bank steps on the Monte-Carlo latency kernel its extra workgroups build the rows' features (two launches per frame);
    // else the feature builder's own launch in front of the step
    const bool one_launch = bank_on_mc_small(b) && b->inj_masks == nullptr && mc_small_builder_fits(m, b->S, b->n_mc, b->T) && I == m->dims.input_size && b->xring != nullptr;
    float* slot_out; int slot_rep; size_t slot_rep_stride;
    next_slot(b, (size_t)I, &slot_out, &slot_rep, &slot_rep_stride);
    if (one_launch) {
        McFrameParts fr{};
        fr.raw_rows = b->h_rows; fr.raw_width = width; fr.raw_kind = kind & ~APE_PARSE_BIG_ENDIAN; fr.raw_big_endian = (kind & APE_PARSE_BIG_ENDIAN) ? 1 : 0;
        fr.cold = b->frames == 0 ? 1 : 0;
        fr.ring_out = slot_out; fr.ring_stream_stride = (size_t)bank_copies(b) * b->T * I; fr.ring_rep_stride = slot_rep_stride; fr.ring_rep = slot_rep;
        ++b->frames;                                   // (what ape_streams_push_rows does behind its launch)
        if (int rc = streams_step_impl(b, flags | APE_FLAG_PACKED_MSG, b->h_out, nullptr, out_dtype, stream, b->h_status, &fr)) { --b->frames; return rc; }
    } else {
        if (int rc = ape_streams_push_rows(b, kind, b->h_rows, stream)) return rc;
        if (int rc = streams_step_impl(b, flags | APE_FLAG_PACKED_MSG, b->h_out, nullptr, out_dtype, stream, b->h_status)) return rc;
    }
    const double t_launched = now_us();
    // (a frame is tens of microseconds; a launch that gives up takes seconds: the stream wait below covers it)
    const bool seen = b->h_done != nullptr && ape_done_wait(b->h_done, b->S, b->h_done_val);
    bool recovered = false;
    const bool fell_through = !seen && b->h_done != nullptr;
    if (!seen) APE_TRY(hipStreamSynchronize((hipStream_t)stream));
    if (*(volatile unsigned*)b->h_status != 0u) {
        recovered = true;
        APE_TRY(hipStreamSynchronize((hipStream_t)stream));
        // the regressor launch gave up (bounded spins): the step is still the bank's newest one, so it can be issued again on
        // the kernels that need no co-residency -- into the same pinned rows.  (Single-launch frame: the builder workgroup may not
        // have run; its row goes into the ring by the feature builder's own kernel first -- the same slot, the same values.)
        if (one_launch) {
            hipError_t e = ape_launch_parse_rows(b->h_rows, b->S, width, kind & ~APE_PARSE_BIG_ENDIAN, slot_out, APE_F32, I, (size_t)bank_copies(b) * b->T * I,
                                                 slot_rep, slot_rep_stride, (kind & APE_PARSE_BIG_ENDIAN) ? 1 : 0, (hipStream_t)stream);
            if (e != hipSuccess) return ape_fail(APE_ERR_HIP, "streams_frame_host: feature builder launch failed: %s", hipGetErrorString(e));
        }
        if (int rc = ape_model_recover(m)) return rc;
    } else {
        // the status word was read behind the step's kernels on the step's own stream and one handle serialises on one
        // stream: nothing aborted since the last check, what the journal holds is done
        journal_clear(m);
    }
    const double t_there = now_us();
    memcpy(out_host, b->h_out, out_bytes);
    const double t_end = now_us();
    if (b->fs_trace.empty()) b->fs_trace.resize(4096 * 3, 0.0f);
    float* tr = b->fs_trace.data() + (b->fs_frames % 4096) * 3;
    tr[0] = (float)(t_launched - t_begin); tr[1] = (float)(t_there - t_launched); tr[2] = (float)(t_end - t_there);
    b->fs_frames += 1;
    b->fs_fallback += fell_through ? 1 : 0;
    b->fs_recovered += recovered ? 1 : 0;
    return APE_OK;
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

// launches 2 and 3 of a subset frame over the compact windows and descriptors in the bank's workspace (also the journal's re-issue)
static int subset_regress_post(ape_streams* b, int K, uint32_t flags, void* out_dev, int out_dtype, void* stream, unsigned long long mc_call,
                               const SubsetHostWords& hw) {
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
    StreamPostParams q{};
    q.y_new = b->sub_y; q.yring = b->yring; q.msg = out_dev; q.tail = nullptr;
    q.yy_m = norm ? m->stats + 2 * m->dims.input_size : nullptr;
    q.yy_s = norm ? m->stats + 2 * m->dims.input_size + m->dims.output_size : nullptr;
    memcpy(q.body, m->body, sizeof(q.body));
    q.S = K; q.O = m->dims.output_size; q.W = layout_est_width(m->dims.target_layout); q.layout = m->dims.target_layout;
    q.smooth = b->smooth; q.n_mc = b->n_mc;
    q.msg_dtype = out_dtype; q.packed = packed ? 1 : 0;
    q.part = b->post_part; q.part_cnt = b->post_cnt;     // (sized for S >= K entries)
    if (hw.status_out != nullptr && m->caps.cluster_ok) { q.status_in = ctl_words(m).status; q.status_out = hw.status_out; }
    if (hw.done_out != nullptr) { q.done_out = hw.done_out; q.done_val = hw.done_val; }      // (word j behind list entry j's row)
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
    SubsetRowsParams rp{};
    rp.rows = rows_dev; rp.desc = b->sub_desc; rp.xring = b->xring; rp.xw = b->sub_x;
    rp.K = K; rp.width = width; rp.kind = kind & ~APE_PARSE_BIG_ENDIAN; rp.big_endian = (kind & APE_PARSE_BIG_ENDIAN) ? 1 : 0; rp.T = b->T; rp.I = I;
    rp.n_mc = bank_copies(b);
    hipError_t e = ape_launch_subset_rows(rp, st);
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
    if (out_cap > b->h_out_bytes) {
        if (b->h_out) { APE_TRY(hipHostFree(b->h_out)); b->h_out = nullptr; b->h_out_bytes = 0; }
        APE_TRY(hipHostMalloc(&b->h_out, out_cap, APE_PINNED));
        b->h_out_bytes = out_cap;
    }
    APE_TRY(ape_pinned_zeroed(&b->h_status, 64));
    unsigned* const h_done = reinterpret_cast<unsigned*>(b->hs_block);
    SubsetDesc* const h_desc = reinterpret_cast<SubsetDesc*>(b->hs_block + 64 * sizeof(unsigned));
    float* const h_rows = reinterpret_cast<float*>(b->hs_block + 64 * sizeof(unsigned) + (size_t)b->S * sizeof(SubsetDesc));
    const bool words = K <= 64;                                  // a word per entry the host can watch; a longer list waits for the stream
    ape_done_next(&b->hs_done_val);
    subset_enter(b);
    const double t_begin = now_us();
    memcpy(h_rows, rows_host, (size_t)K * width * sizeof(float));
    subset_fill_desc(b, streams_host, K, h_desc);
    *b->h_status = m->caps.cluster_ok ? 0xFFFFFFFFu : 0u;            // (as ape_streams_frame_host: a sentinel where a kernel writes the word)
    SubsetRowsParams rp{};
    rp.rows = h_rows; rp.desc = h_desc; rp.xring = b->xring; rp.xw = b->sub_x;
    rp.K = K; rp.width = width; rp.kind = kind & ~APE_PARSE_BIG_ENDIAN; rp.big_endian = (kind & APE_PARSE_BIG_ENDIAN) ? 1 : 0; rp.T = b->T; rp.I = I;
    rp.n_mc = bank_copies(b);
    hipError_t e = ape_launch_subset_rows_host(rp, b->sub_desc, st);
    if (e != hipSuccess) return ape_fail(APE_ERR_HIP, "streams_frame_subset_host: row launch failed: %s", hipGetErrorString(e));
    for (int j = 0; j < K; ++j) { b->s_frames[streams_host[j]] += 1; b->s_steps[streams_host[j]] += 1; }
    const unsigned long long mc_call = b->mc_calls++;
    SubsetHostWords hw;
    hw.status_out = b->h_status; hw.done_out = words ? h_done : nullptr; hw.done_val = b->hs_done_val; hw.what = "streams_frame_subset_host";
    if (int rc = subset_regress_post(b, K, flags, b->h_out, out_dtype, stream, mc_call, hw)) {
        (void)hipStreamSynchronize(st);                          // (launch 1 may still read the block the next call rewrites)
        return rc;
    }
    subset_journal(b, K, flags, b->h_out, out_dtype, stream, mc_call);
    const double t_launched = now_us();
    const bool seen = words && ape_done_wait(h_done, K, b->hs_done_val);   // else the stream's own completion (as ape_streams_frame_host)
    bool recovered = false;
    const bool fell_through = !seen && words;
    if (!seen) APE_TRY(hipStreamSynchronize(st));
    if (*(volatile unsigned*)b->h_status != 0u) {
        // the regressor launch gave up (bounded spins): the frame is the bank's newest, its windows and descriptors are on the device --
        // regressor and post-filter again on the kernels that need no co-residency, into the same pinned rows
        recovered = true;
        APE_TRY(hipStreamSynchronize(st));
        if (int rc = ape_model_recover(m)) return rc;
    } else {
        journal_clear(m);                                        // (read behind the frame's kernels on the frame's stream: what the journal holds is done)
    }
    const double t_there = now_us();
    memcpy(out_host, b->h_out, (size_t)K * row_w * esz);
    const double t_end = now_us();
    if (b->fs_trace.empty()) b->fs_trace.resize(4096 * 3, 0.0f);
    float* tr = b->fs_trace.data() + (b->fs_frames % 4096) * 3;
    tr[0] = (float)(t_launched - t_begin); tr[1] = (float)(t_there - t_launched); tr[2] = (float)(t_end - t_there);
    b->fs_frames += 1;
    b->fs_fallback += fell_through ? 1 : 0;
    b->fs_recovered += recovered ? 1 : 0;
    return APE_OK;
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
extern "C++" template <typename Fill>
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

int ape_replay(ape_model_t* m, int32_t kind, const float* rows_dev, int32_t F, const int32_t* seg_starts_host, int32_t R,
               int32_t seq_len, int32_t smooth, int32_t n_mc, float dropout_p, uint64_t seed, uint32_t flags,
               void* out_dev, int32_t out_dtype, float* y_dev, int32_t max_rows_per_launch, void* stream) {
    return ape_replay_bodies(m, kind, rows_dev, F, seg_starts_host, R, seq_len, smooth, n_mc, dropout_p, seed, flags, out_dev, out_dtype, y_dev,
                             max_rows_per_launch, stream, nullptr);
}

// ape_replay_resume's extra arguments; nullptr for the entries that start cold and keep no state
struct ApeReplayResume {
    const void* state_in; const uint8_t* warm_in; void* state_out; uint8_t* warm_out; uint64_t sample_row_base;
};

// bodies_host [R,9]: recording r's rows as a fresh estimator BUILT WITH recording r's bonemap returns them (estimator.py:57-68); NULL: the
// model's body for every recording, on the kernels ape_replay always ran
static int replay_impl(ape_model_t* m, int32_t kind, const float* rows_dev, int32_t F, const int32_t* seg_starts_host, int32_t R,
                       int32_t seq_len, int32_t smooth, int32_t n_mc, float dropout_p, uint64_t seed, uint32_t flags,
                       void* out_dev, int32_t out_dtype, float* y_dev, int32_t max_rows_per_launch, void* stream, const double* bodies_host,
                       bool any_regressor, const ApeReplayResume* rs = nullptr);

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

static int replay_impl(ape_model_t* m, int32_t kind, const float* rows_dev, int32_t F, const int32_t* seg_starts_host, int32_t R,
                       int32_t seq_len, int32_t smooth, int32_t n_mc, float dropout_p, uint64_t seed, uint32_t flags,
                       void* out_dev, int32_t out_dtype, float* y_dev, int32_t max_rows_per_launch, void* stream, const double* bodies_host,
                       bool any_regressor, const ApeReplayResume* rs) {
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

int ape_replay_resume(ape_model_t* m, int32_t kind, const float* rows_dev, int32_t F, const int32_t* seg_starts_host, int32_t R,
                      int32_t seq_len, int32_t smooth, int32_t n_mc, float dropout_p, uint64_t seed, uint32_t flags,
                      void* out_dev, int32_t out_dtype, float* y_dev, int32_t max_rows_per_launch, void* stream, const double* bodies_host,
                      const void* state_in_dev, const uint8_t* warm_in_host, void* state_out_dev, uint8_t* warm_out_host,
                      uint64_t sample_row_base) {
    const ApeReplayResume rs{state_in_dev, warm_in_host, state_out_dev, warm_out_host, sample_row_base};
    return replay_impl(m, kind, rows_dev, F, seg_starts_host, R, seq_len, smooth, n_mc, dropout_p, seed, flags, out_dev, out_dtype, y_dev,
                       max_rows_per_launch, stream, bodies_host, true, &rs);
}

// one journaled call again, on the kernels that need no co-residency (m->replaying is set)
static int replay_entry(ape_model_t* m, const ApeJournalEntry& e) {
    switch (e.kind) {
        case ApeJournalEntry::FORWARD:
            return ape_lstm_forward(m, (const float*)e.in0, e.B, e.T, e.flags, (const float*)e.in1, e.dropout_p, e.seed, (float*)e.out0, e.stream);
        case ApeJournalEntry::FORWARD_HS:
            return ape_lstm_forward_hs(m, (const float*)e.in0, e.B, e.T, e.flags, nullptr, e.dropout_p, e.seed, (const float*)e.in1,
                                       (const float*)e.in2, (float*)e.out0, e.stream);
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

const char* ape_model_last_kernel(const ape_model_t* m) { return m ? m->last_kernel : ""; }

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

}  // extern "C"
