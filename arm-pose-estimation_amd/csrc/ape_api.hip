// C ABI of libape_hip.so (see include/ape_hip.h), host side: the thread's error string, the model handle (dims check, capabilities,
// create / destroy / setters), the journal's check / recover / stats.  The other entries live in the api_*.hip files (ape_host.h lists
// them).  No CPU fallback: every compute entry point needs a gfx950 device.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <algorithm>
#include <cstring>
#include <new>
#include <string>
#include <utility>
#include <vector>

#include "ape_host.h"
#include "weight_pack.h"

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

}  // namespace

static_assert(APE_PLAN_TILE_ROWS == APE_TILE_ROWS, "ape_plan.h prices the batch-tile kernel's waves");

// What a model of `dims` can run on a device with n_cus CUs: the kernels' own predicates, in ONE place (ape_model_create, which then
// clears what failed to set up, and the ape_debug_* entry points).  The routing on top of it is csrc/ape_plan.h.
ApeCaps ape_caps(const ape_dims_t* dims, int n_cus) {
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
    auto KXl = [&](int l) { return l == 0 ? m->KX : H; };       // padded input width of LSTM layer l; the images' sizes: weight_pack.h
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
            e = plan((void**)&m->ff_wpack[j], ff_wpack_elems(H, (j == 0) ? m->KX : H) * sizeof(float));
            if (e == hipSuccess) e = plan((void**)&m->ff_bias[j], H * sizeof(float));
        }
        if (e == hipSuccess) e = plan((void**)&m->w_out, (size_t)O * H * sizeof(float));
        if (e == hipSuccess) e = plan((void**)&m->b_out, O * sizeof(float));
        if (e == hipSuccess) e = plan((void**)&m->stats, (3 * I + 2 * O) * sizeof(double));
        if (e == hipSuccess && ape_mlp_pipe_supported(H, L, m->KX, O) && m->n_cus >= 16) {
            e = plan((void**)&m->ffp_wa0, mlp_pipe_elems(m->KX / 8) * sizeof(float));
            if (e == hipSuccess) e = plan((void**)&m->ffp_wa1, mlp_pipe_elems(H / 8) * sizeof(float));
            if (e == hipSuccess) e = plan((void**)&m->ffp_wb2, mlp_pipe_elems(H / 8) * sizeof(float));
            if (e == hipSuccess) e = plan((void**)&m->ffp_wbo, mlp_pipe_head_elems() * sizeof(float));
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
        e = plan((void**)&m->wpack[l], wpack_elems(H, KXl(l)) * sizeof(float));
        if (e == hipSuccess) e = plan((void**)&m->bias[l], 4 * H * sizeof(float));
    }
    if (e == hipSuccess) e = plan((void**)&m->w_out, (size_t)O * H * sizeof(float));
    if (e == hipSuccess) e = plan((void**)&m->b_out, O * sizeof(float));
    if (e == hipSuccess) e = plan((void**)&m->stats, (3 * I + 2 * O) * sizeof(double));
    if (imupose) {       // input layer: the MLP kernel's packing and launch, with the activation as its result
        if (e == hipSuccess) e = plan((void**)&m->ff_wpack[0], ff_wpack_elems(H, m->KXpre) * sizeof(float));
        if (e == hipSuccess) e = plan((void**)&m->ff_bias[0], H * sizeof(float));
        if (e == hipSuccess) e = ape_prepare_lstm_tile16_wide(ape_lstm_tile16_smem_bytes(H, L, m->KX, O, false));
    }
    // the kernel may carve its largest LDS layout (with dropout buffers)
    const size_t smem = ape_lstm_tile16_smem_bytes(H, L, m->KX, O, true);
    if (imupose) {}
    else if (e == hipSuccess && smem <= 160 * 1024) e = ape_prepare_lstm_tile16(H, L, smem);
    else if (e == hipSuccess) e = ape_prepare_lstm_tile16(H, L, ape_lstm_tile16_smem_bytes(H, L, m->KX, O, false));
    // ... and ape_lstm_features' instantiation of the same body (DropoutLSTM handles only)
    if (!imupose && e == hipSuccess) e = ape_prepare_lstm_tile16_hout(H, L, ape_lstm_tile16_smem_bytes(H, L, m->KX, O, smem <= 160 * 1024));
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
            e = plan((void**)&m->wcl[l], wcl_elems(H, KXl(l)) * sizeof(float));
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
            e = plan(&m->wcl16[l], wcl16_elems(H, KXl(l)) * sizeof(_Float16));
        if (e == hipSuccess) e = ape_prepare_lstm_cluster(H, L, m->KX);
        if (e == hipSuccess && ((H == 128 && L == 3) || (H == 256 && L == 2 && m->KX == 32)))
            e = ape_prepare_lstm_cluster(H, 1, m->KX);       // layer 0 alone: launch A of a Monte-Carlo bank
        if (e == hipSuccess && !imupose) e = ape_prepare_lstm_cluster_f16(H, L, m->KX);
        if (e == hipSuccess && !imupose) e = ape_prepare_lstm_cluster_f16v2(H, L, m->KX);
        // latency kernel with H/8 members (every CU of a 32-CU XCD at H = 256): only where an XCD has that many CUs
        if (m->n_cus / 8 >= H / 8 && !imupose) {
            for (int l = 0; l < L && e == hipSuccess; ++l)
                e = plan((void**)&m->wcls[l], wcls_elems(H, KXl(l)) * sizeof(float));
            m->small_uw = 2;
        }
        if (m->caps.mc_small) {
            for (int l = 1; l < L && e == hipSuccess; ++l) e = plan((void**)&m->wmc[l], wmc_elems(H) * sizeof(float));
            for (int l = 1; l < L && e == hipSuccess; ++l) e = plan((void**)&m->wmc16[l], wmc16_elems(H) * sizeof(float));
            m->gxm_cluster_bytes = ape_mc_small_cluster_bytes(H, L);
            if (e == hipSuccess) e = plan((void**)&m->gxm, 256 + 8 * m->gxm_cluster_bytes + 8 * 64 * 8);      // + the feature granules of 8 streams
            if (e == hipSuccess) e = ape_prepare_lstm_mc_small(H, L, m->KX);
        }
        if (m->caps.c32) {
            for (int l = 0; l < L && e == hipSuccess; ++l)
                e = plan((void**)&m->wcl32[l], wcl32_elems(H, KXl(l)) * sizeof(float));
            for (int l = 0; l < L && e == hipSuccess; ++l)         // the f16 hi / lo image of lstm_cluster32.hip (same size, pack_c32_split)
                e = plan((void**)&m->wcl32s[l], wcl32s_elems(H, KXl(l)) * sizeof(unsigned));
            if (e == hipSuccess) e = ape_prepare_lstm_cluster32(H, L, m->KX);
            if (e == hipSuccess && m->caps.up32) e = ape_prepare_lstm_upper32();
        }
        if (m->caps.split32) {
            for (int l = 0; l < L && e == hipSuccess; ++l)
                e = plan((void**)&m->wcl32[l], wcl32_elems(H, KXl(l)) * sizeof(float));
            if (e == hipSuccess) e = ape_prepare_lstm_upper32();
            m->caps.split32 = (e == hipSuccess);
        }
        if (m->caps.up128) {
            for (int l = 1; l < L && e == hipSuccess; ++l) e = plan((void**)&m->wup128[l], wup128_elems(H, H) * sizeof(float));
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
int check_and_reset(ape_model_t* m) {
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
                    st == APE_ABORT_SPIN ? "a workgroup gave up waiting for a peer -- not all workgroups of a cluster were resident"
                    : st == APE_ABORT_XCD_RENDEZVOUS ? "the Monte-Carlo latency kernel gave up waiting for the members of a cluster -- not all workgroups were resident"
                    : st >= APE_ABORT_COLLECT ? "the Monte-Carlo latency kernel gave up waiting for a peer's values (16 + phase)"
                            : "a launch found the state of an earlier aborted launch");
    }
    return APE_OK;
}

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

const char* ape_model_last_kernel(const ape_model_t* m) { return m ? m->last_kernel : ""; }

