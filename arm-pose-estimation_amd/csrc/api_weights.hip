// ape_model_load_weights: walk the blob, build every register image the model's kernels read (weight_pack.h), copy.  The images' sizes
// are the *_elems() of weight_pack.h, which ape_model_create planned the device buffers with.
#include <algorithm>
#include <cmath>
#include <vector>

#include "ape_host.h"
#include "weight_pack.h"

namespace {

// one image: `elems` elements of T built by `pack` on the host, then copied to `dev`
template <typename T, typename Pack>
hipError_t upload(void* dev, size_t elems, Pack pack) {
    std::vector<T> img(elems);
    pack(img.data());
    return hipMemcpy(dev, img.data(), elems * sizeof(T), hipMemcpyHostToDevice);
}

// DropoutFF's layers 0..L, or ImuPoseLSTM's input layer alone (`pre_only`, then the LSTM follows in the blob): the MLP kernel's images,
// and the MLP pipeline's four where it is set up.  *cur moves behind the layers.
int load_mlp_layers(ape_model* m, const float* blob, const float** cur, bool pre_only) {
    const int H = m->dims.hidden_size, L = m->dims.num_layers, O = m->dims.output_size, I = m->dims.input_size;
    for (int j = 0; j <= (pre_only ? 0 : L); ++j) {
        const int in_j = (j == 0) ? I : H, K = (j == 0) ? (pre_only ? m->KXpre : m->KX) : H;
        const float* wj = *cur;  *cur += (size_t)H * in_j;
        const float* bj = *cur;  *cur += H;
        APE_TRY(upload<float>(m->ff_wpack[j], ff_wpack_elems(H, K), [&](float* out) { pack_ff_wpack(wj, in_j, H, K, out); }));
        APE_TRY(hipMemcpy(m->ff_bias[j], bj, H * sizeof(float), hipMemcpyHostToDevice));
    }
    if (pre_only || !m->ffp_ok) return APE_OK;
    const float* c2 = blob;
    float* dst[3] = {m->ffp_wa0, m->ffp_wa1, m->ffp_wb2};
    for (int j = 0; j <= 2; ++j) {
        const int inl = (j == 0) ? I : H, kbl = (j == 0) ? m->KX / 8 : H / 8;
        const float* wl = c2;  c2 += (size_t)H * inl + H;
        APE_TRY(upload<float>(dst[j], mlp_pipe_elems(kbl), [&](float* out) { pack_mlp_pipe(wl, inl, kbl, out); }));
    }
    APE_TRY(upload<float>(m->ffp_wbo, mlp_pipe_head_elems(), [&](float* out) { pack_mlp_pipe_head(c2, O, H, out); }));
    return APE_OK;
}

// every image of LSTM layer l; what the model has no buffer for is not built
int load_lstm_layer(ape_model* m, int l, const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh) {
    const int H = m->dims.hidden_size;
    const int in_l = (l == 0) ? m->lstm_in : H, KXl = (l == 0) ? m->KX : H;
    const WCat wcat{w_ih, in_l, w_hh, H, KXl};
    if (m->caps.cluster_ok) {
        APE_TRY(upload<float>(m->wcl[l], wcl_elems(H, KXl), [&](float* out) { pack_wcl(wcat, out); }));
        if (m->small_uw == 2) APE_TRY(upload<float>(m->wcls[l], wcls_elems(H, KXl), [&](float* out) { pack_wcls(wcat, out); }));
        if (m->caps.mc_small && l >= 1) {
            std::vector<float> pm(std::max(wmc_elems(H), wmc16_elems(H)));       // (one host buffer serves both)
            pack_wmc(wcat, pm.data());
            APE_TRY(hipMemcpy(m->wmc[l], pm.data(), wmc_elems(H) * sizeof(float), hipMemcpyHostToDevice));
            pack_wmc16(wcat, pm.data());
            APE_TRY(hipMemcpy(m->wmc16[l], pm.data(), wmc16_elems(H) * sizeof(float), hipMemcpyHostToDevice));
        }
        if (m->wcl16[l]) APE_TRY(upload<_Float16>(m->wcl16[l], wcl16_elems(H, KXl), [&](_Float16* out) { pack_wcl16(wcat, out); }));
    }
    if (m->wcl32[l] != nullptr) APE_TRY(upload<float>(m->wcl32[l], wcl32_elems(H, KXl), [&](float* out) { pack_wcl32(wcat, out); }));
    if (m->wcl32s[l] != nullptr) {
        std::vector<unsigned> ps(wcl32s_elems(H, KXl));
        const int S = pack_c32_split(w_ih, in_l, w_hh, H, KXl, l == 0 ? KXl : 0, ps.data());
        if (l == 0) m->caps.c32 = true;        // (weights that refuse the split keep the model off lstm_cluster32.hip)
        if (S < 0) m->caps.c32 = false;
        else {
            m->c32_scale[l] = std::ldexp(1.0f, S);
            m->c32_descale[l] = std::ldexp(1.0f, -S);
            APE_TRY(hipMemcpy(m->wcl32s[l], ps.data(), ps.size() * sizeof(unsigned), hipMemcpyHostToDevice));
        }
    }
    if (m->caps.up128 && l >= 1) APE_TRY(upload<float>(m->wup128[l], wup128_elems(H, KXl), [&](float* out) { pack_wup128(wcat, out); }));
    APE_TRY(upload<float>(m->wpack[l], wpack_elems(H, KXl), [&](float* out) { pack_wpack(wcat, out); }));
    std::vector<float> bsum(4 * H);
    for (int i = 0; i < 4 * H; ++i) bsum[i] = b_ih[i] + b_hh[i];
    APE_TRY(hipMemcpy(m->bias[l], bsum.data(), bsum.size() * sizeof(float), hipMemcpyHostToDevice));
    return APE_OK;
}

}  // namespace

int ape_model_load_weights(ape_model_t* m, const float* blob, size_t n_floats) {
    if (!m || !blob) return ape_fail(APE_ERR_INVALID_ARG, "load_weights: NULL argument");
    const size_t want = ape_weight_blob_floats(&m->dims);
    if (n_floats != want) return ape_fail(APE_ERR_INVALID_ARG, "weight blob has %zu floats, expected %zu", n_floats, want);
    APE_TRY(hipSetDevice(m->dims.device));
    std::vector<float> host(n_floats);
    APE_TRY(hipMemcpy(host.data(), blob, n_floats * sizeof(float), hipMemcpyDefault));   // host or device source

    const int H = m->dims.hidden_size, L = m->dims.num_layers, O = m->dims.output_size;
    const float* cur = host.data();
    if (m->dims.model_kind != APE_MODEL_LSTM)
        if (int rc = load_mlp_layers(m, host.data(), &cur, m->dims.model_kind == APE_MODEL_IMUPOSE)) return rc;
    if (m->dims.model_kind != APE_MODEL_FF)
        for (int l = 0; l < L; ++l) {
            const float* w_ih = cur;  cur += (size_t)4 * H * ((l == 0) ? m->lstm_in : H);
            const float* w_hh = cur;  cur += (size_t)4 * H * H;
            const float* b_ih = cur;  cur += 4 * H;
            const float* b_hh = cur;  cur += 4 * H;
            if (int rc = load_lstm_layer(m, l, w_ih, w_hh, b_ih, b_hh)) return rc;
        }
    APE_TRY(hipMemcpy(m->w_out, cur, (size_t)O * H * sizeof(float), hipMemcpyHostToDevice));
    cur += (size_t)O * H;
    APE_TRY(hipMemcpy(m->b_out, cur, O * sizeof(float), hipMemcpyHostToDevice));
    m->has_weights = true;
    return APE_OK;
}

// ---- the output layer on its own ------------------------------------------------------------------------------------
// Every kernel of a DropoutLSTM handle reads the head through m->w_out / m->b_out (head_and_stats; no route packs it), so a new head is
// two copies.  The handle is made healthy and idle first: what was issued before runs on the head it was issued with.
static int head_ready(ape_model_t* m, const void* w, const void* b, const char* who) {
    if (!m || !w || !b) return ape_fail(APE_ERR_INVALID_ARG, "%s: NULL argument", who);
    if (m->dims.model_kind != APE_MODEL_LSTM)
        return ape_fail(APE_ERR_UNSUPPORTED, "%s: DropoutLSTM handles only (the other kinds' kernels read packed copies of the head)", who);
    if (!m->has_weights) return ape_fail(APE_ERR_NOT_READY, "%s: weights not loaded", who);
    APE_TRY(hipSetDevice(m->dims.device));
    if (int rc = ape_model_recover(m)) return rc;
    APE_TRY(hipDeviceSynchronize());
    return APE_OK;
}

int ape_model_set_head(ape_model_t* m, const float* w_out_host, const float* b_out_host) {
    if (int rc = head_ready(m, w_out_host, b_out_host, "set_head")) return rc;
    const size_t O = (size_t)m->dims.output_size, H = (size_t)m->dims.hidden_size;
    APE_TRY(hipMemcpy(m->w_out, w_out_host, O * H * sizeof(float), hipMemcpyHostToDevice));
    APE_TRY(hipMemcpy(m->b_out, b_out_host, O * sizeof(float), hipMemcpyHostToDevice));
    return APE_OK;
}

int ape_model_get_head(ape_model_t* m, float* w_out_host, float* b_out_host) {
    if (int rc = head_ready(m, w_out_host, b_out_host, "get_head")) return rc;
    const size_t O = (size_t)m->dims.output_size, H = (size_t)m->dims.hidden_size;
    APE_TRY(hipMemcpy(w_out_host, m->w_out, O * H * sizeof(float), hipMemcpyDeviceToHost));
    APE_TRY(hipMemcpy(b_out_host, m->b_out, O * sizeof(float), hipMemcpyDeviceToHost));
    return APE_OK;
}
