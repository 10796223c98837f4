// Stand-alone check of csrc/weight_pack.h (no GPU, no HIP): every register image of every deployed model shape, packed from weights of a
// small integer generator, printed as one 64-bit FNV-1a hash per image.  tests/test_weight_pack_cpu.py compares the lines with
// tests/golden/weight_images.json, which was recorded from the packing loops as they stood inside ape_model_load_weights before they
// moved into the header.  Every image is packed twice, into storage prefilled with 0x00 and with 0xFF: the two must agree (each of the
// *_elems() elements was written) and the canary behind each buffer must survive (nothing beyond them was).  Built with the address and
// undefined-behaviour sanitizers where they link.
//   weight_pack_main            the hash lines, then "weight_pack ok"
//   weight_pack_main --time N   the 2 x 256 pocket shape's images N times, milliseconds per pass (no checks)
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../arm-pose-estimation_amd/csrc/weight_pack.h"

// weight i of a blob: distinct for i < 2^28 (an odd multiplier permutes 28 bits), finite, either sign, magnitudes 2^-17 .. 2^-2
static float gen(uint32_t i) {
    const uint32_t h = (i * 0x9E3779B1u) & 0x0FFFFFFFu;
    const uint32_t bits = ((h >> 27) << 31) | ((110u + ((h >> 23) & 15u)) << 23) | (h & 0x7FFFFFu);
    float v;
    memcpy(&v, &bits, 4);
    return v;
}

static uint64_t fnv1a(const void* p, size_t bytes) {
    uint64_t h = 0xcbf29ce484222325ull;
    const unsigned char* c = static_cast<const unsigned char*>(p);
    for (size_t i = 0; i < bytes; ++i) { h ^= c[i]; h *= 0x100000001b3ull; }
    return h;
}

static int g_bad = 0;
static bool g_quiet = false;           // --time: pack only

static const unsigned char CANARY[8] = {0xC3, 0x5A, 0x96, 0x0F, 0xF0, 0x69, 0xA5, 0x3C};

// packs one image of `elems` elements of T twice, checks it and prints "<label> <hash>"
template <typename T, typename Pack>
static void image(const std::string& label, size_t elems, Pack pack) {
    const size_t bytes = elems * sizeof(T);
    std::vector<unsigned char> a(bytes + 8, 0x00), b(g_quiet ? 0 : bytes + 8, 0xFF);
    memcpy(a.data() + bytes, CANARY, 8);
    pack(reinterpret_cast<T*>(a.data()));
    if (g_quiet) return;
    memcpy(b.data() + bytes, CANARY, 8);
    pack(reinterpret_cast<T*>(b.data()));
    if (memcmp(a.data(), b.data(), bytes) != 0) { printf("FAILED: %s: not every one of %zu elements was written\n", label.c_str(), elems); g_bad += 1; }
    if (memcmp(a.data() + bytes, CANARY, 8) != 0 || memcmp(b.data() + bytes, CANARY, 8) != 0) {
        printf("FAILED: %s: wrote behind its %zu elements\n", label.c_str(), elems);
        g_bad += 1;
    }
    printf("%s %016llx\n", label.c_str(), (unsigned long long)fnv1a(a.data(), bytes));
}

static int pad32(int I) { return (I + 31) / 32 * 32; }

enum Kind { LSTM, FF, IMUPOSE };
struct Shape { const char* name; Kind kind; int I, H, L, O; };

// the blob as ape_model_load_weights walks it: [input layer: W, b] (ImuPose) / [layers 0..L: W, b] (FF); per LSTM layer W_ih, W_hh, b_ih, b_hh;
// W_out, b_out
static void shape_images(const Shape& s) {
    const int I = s.I, H = s.H, L = s.L, O = s.O;
    const size_t in0 = s.kind == IMUPOSE ? H : I;
    size_t n = 0;
    if (s.kind == FF) n = (size_t)H * I + H + (size_t)L * ((size_t)H * H + H);
    else {
        if (s.kind == IMUPOSE) n += (size_t)H * I + H;
        for (int l = 0; l < L; ++l) n += (size_t)4 * H * (l == 0 ? in0 : H) + (size_t)4 * H * H + 8 * H;
    }
    n += (size_t)O * H + O;
    std::vector<float> blob(n);
    for (size_t i = 0; i < n; ++i) blob[i] = gen((uint32_t)i);
    const std::string nm = std::string(s.name) + ".";
    const float* cur = blob.data();
    if (s.kind != LSTM) {
        const bool pre_only = s.kind == IMUPOSE;
        const int KX = pad32(I);
        for (int j = 0; j <= (pre_only ? 0 : L); ++j) {
            const int in_j = (j == 0) ? I : H, K = (j == 0) ? KX : H;
            const float* wj = cur;  cur += (size_t)H * in_j + H;
            image<float>(nm + "ff_wpack" + std::to_string(j), ff_wpack_elems(H, K), [&](float* out) { pack_ff_wpack(wj, in_j, H, K, out); });
        }
        if (!pre_only) {           // (a shape the MLP pipeline accepts: H = 256, two hidden layers, KX = 32, O <= 16)
            const float* c2 = blob.data();
            const char* names[3] = {"ffp_wa0", "ffp_wa1", "ffp_wb2"};
            for (int j = 0; j <= 2; ++j) {
                const int inl = (j == 0) ? I : H, kbl = (j == 0) ? KX / 8 : H / 8;
                const float* wl = c2;  c2 += (size_t)H * inl + H;
                image<float>(nm + names[j], mlp_pipe_elems(kbl), [&](float* out) { pack_mlp_pipe(wl, inl, kbl, out); });
            }
            image<float>(nm + "ffp_wbo", mlp_pipe_head_elems(), [&](float* out) { pack_mlp_pipe_head(c2, O, H, out); });
            return;
        }
    }
    // the LSTM layers; which images a shape gets is what ape_model_create sets up for it on a whole device
    const bool plain = s.kind == LSTM;
    for (int l = 0; l < L; ++l) {
        const int in_l = (l == 0) ? (int)in0 : H, KXl = (l == 0) ? pad32((int)in0) : H;
        const float* w_ih = cur;  cur += (size_t)4 * H * in_l;
        const float* w_hh = cur;  cur += (size_t)4 * H * H + 8 * H;
        const WCat wcat{w_ih, in_l, w_hh, H, KXl};
        const std::string ls = std::to_string(l);
        image<float>(nm + "wcl" + ls, wcl_elems(H, KXl), [&](float* out) { pack_wcl(wcat, out); });
        if (plain) image<float>(nm + "wcls" + ls, wcls_elems(H, KXl), [&](float* out) { pack_wcls(wcat, out); });
        if (plain && l >= 1) {
            image<float>(nm + "wmc" + ls, wmc_elems(H), [&](float* out) { pack_wmc(wcat, out); });
            image<float>(nm + "wmc16" + ls, wmc16_elems(H), [&](float* out) { pack_wmc16(wcat, out); });
        }
        if (plain) image<_Float16>(nm + "wcl16" + ls, wcl16_elems(H, KXl), [&](_Float16* out) { pack_wcl16(wcat, out); });
        if (H == 256) image<float>(nm + "wcl32" + ls, wcl32_elems(H, KXl), [&](float* out) { pack_wcl32(wcat, out); });
        if (H == 256 && plain) {
            int S = 0;
            image<unsigned>(nm + "wcl32s" + ls, wcl32s_elems(H, KXl), [&](unsigned* out) { S = pack_c32_split(w_ih, in_l, w_hh, H, KXl, l == 0 ? KXl : 0, out); });
            if (!g_quiet) printf("%swcl32s%s.S %d\n", nm.c_str(), ls.c_str(), S);
        }
        if (H == 128 && plain && l >= 1) image<float>(nm + "wup128" + ls, wup128_elems(H, KXl), [&](float* out) { pack_wup128(wcat, out); });
        image<float>(nm + "wpack" + ls, wpack_elems(H, KXl), [&](float* out) { pack_wpack(wcat, out); });
    }
}

int main(int argc, char** argv) {
    const Shape shapes[] = {{"pocket_2x256", LSTM, 22, 256, 2, 14},  {"watch_2x256", LSTM, 20, 256, 2, 12}, {"uarm_3x128", LSTM, 38, 128, 3, 20},
                            {"imupose_2x256", IMUPOSE, 22, 256, 2, 14}, {"ff_pipe", FF, 22, 256, 2, 14}};
    if (argc == 3 && strcmp(argv[1], "--time") == 0) {
        g_quiet = true;
        const int reps = atoi(argv[2]) > 0 ? atoi(argv[2]) : 1;
        const auto t0 = std::chrono::steady_clock::now();
        for (int r = 0; r < reps; ++r) shape_images(shapes[0]);
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        printf("%s: %.2f ms per pass over %d (blob fill included)\n", shapes[0].name, ms / reps, reps);
        return 0;
    }
    for (const Shape& s : shapes) shape_images(s);
    if (g_bad) { printf("%d check(s) failed\n", g_bad); return 1; }
    printf("weight_pack ok\n");
    return 0;
}
