// Host-only check of the training handles' shared core (sdfa-2019_amd/csrc/trainstate.h), which frees and copies: without a device,
// for each of sdfa_headtrain, sdfa_attntrain, sdfa_lstmtrain, sdfa_freqtrain and sdfa_convtrain: create, set_tensor (good name, bad name, short numel, null
// data), the finalize-with-a-missing-tensor refusal, the calls an unfinalised handle refuses, and destroy of the unfinalised handle.
// Meant to run under AddressSanitizer and UBSan on the host side only, from sdfa-2019_amd/csrc:
//
//   hipcc -std=c++17 --offload-arch=gfx950 -g -O1 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//       -x hip ../../tools/trainstate_host_check.cpp api_core.cpp api_headtrain.cpp api_attntrain.cpp api_lstmtrain.cpp \
//       api_freqtrain.cpp api_convtrain.cpp headtrain.hip attntrain.hip lstmtrain.hip freqtrain.hip convtrain.hip \
//       -o trainstate_host_check && ./trainstate_host_check
//
// It launches nothing; exit status 0 and "trainstate host check: ok" is a pass, a sanitizer report is a failure.
#include "../include/sdfa_attntrain.h"
#include "../include/sdfa_convtrain.h"
#include "../include/sdfa_freqtrain.h"
#include "../include/sdfa_headtrain.h"
#include "../include/sdfa_hip.h"
#include "../include/sdfa_lstmtrain.h"

#include <stdio.h>
#include <string.h>

#include <vector>

thread_local int g_sdfa_gemm_variant = 0;      // gemm.hip's, which api_core.cpp's option table names; not linked here

static int failures = 0;

static void expect(const char *what, long long rc, long long want, const char *fragment) {
    const char *msg = rc < 0 ? sdfa_last_error() : "";
    const bool ok = rc == want && (!fragment || strstr(msg, fragment));
    printf("%-58s rc %lld %s%s\n", what, rc, msg, ok ? "" : "   <-- UNEXPECTED");
    failures += !ok;
}

// One module's entry points behind the signatures the three share.
struct Api {
    const char *mod;
    void *(*create)();
    void (*destroy)(void *);
    int (*set_tensor)(void *, const char *, const float *, int64_t);
    int (*finalize)(void *, void *);
    int64_t (*numel)(const void *);
    int (*adam)(void *, double, double, double, double, void *);
    int (*zero_grad)(void *, void *);
    int (*get_tensor)(void *, const char *, int, float *, int64_t);
    int (*set_state)(void *, const char *, int, const float *, int64_t);
    int64_t (*step_count)(const void *);
    int (*set_step_count)(void *, int64_t);
    std::vector<std::pair<const char *, int64_t>> tensors;      // name, numel: the first two and the last of the module
};

#define API(M, CREATE)                                                                                                              \
    [] { return (void *)CREATE; }, [](void *h) { sdfa_##M##_destroy((sdfa_##M *)h); },                                              \
    [](void *h, const char *n, const float *s, int64_t k) { return sdfa_##M##_set_tensor((sdfa_##M *)h, n, s, k); },                 \
    [](void *h, void *st) { return sdfa_##M##_finalize((sdfa_##M *)h, st); },                                                       \
    [](const void *h) { return sdfa_##M##_numel((const sdfa_##M *)h); },                                                            \
    [](void *h, double a, double b, double c, double d, void *st) { return sdfa_##M##_adam((sdfa_##M *)h, a, b, c, d, st); },        \
    [](void *h, void *st) { return sdfa_##M##_zero_grad((sdfa_##M *)h, st); },                                                      \
    [](void *h, const char *n, int w, float *d, int64_t k) { return sdfa_##M##_get_tensor((sdfa_##M *)h, n, w, d, k); },             \
    [](void *h, const char *n, int w, const float *s, int64_t k) { return sdfa_##M##_set_state((sdfa_##M *)h, n, w, s, k); },        \
    [](const void *h) { return sdfa_##M##_step_count((const sdfa_##M *)h); },                                                       \
    [](void *h, int64_t t) { return sdfa_##M##_set_step_count((sdfa_##M *)h, t); }

static void run(const Api &a) {
    char what[128];
    auto tag = [&](const char *s) {
        snprintf(what, sizeof what, "%s: %s", a.mod, s);
        return what;
    };
    void *h = a.create();
    if (!h) {
        expect(tag("create"), -1, 0, nullptr);
        return;
    }
    const auto &[name0, n0] = a.tensors[0];
    std::vector<float> buf((size_t)n0, 0.25f);                      // exactly numel floats: a copy past the end is a report
    expect(tag("set_tensor, good name"), a.set_tensor(h, name0, buf.data(), n0), SDFA_OK, nullptr);
    expect(tag("set_tensor, again"), a.set_tensor(h, name0, buf.data(), n0), SDFA_OK, nullptr);
    expect(tag("set_tensor, bad name"), a.set_tensor(h, "_model.no.such.tensor", buf.data(), n0), SDFA_EINVAL, "has no tensor");
    expect(tag("set_tensor, short numel"), a.set_tensor(h, name0, buf.data(), n0 - 1), SDFA_EINVAL, "elements");
    expect(tag("set_tensor, null data"), a.set_tensor(h, name0, nullptr, n0), SDFA_EINVAL, "null pointer");
    expect(tag("set_tensor, null name"), a.set_tensor(h, nullptr, buf.data(), n0), SDFA_EINVAL, "null pointer");
    expect(tag("finalize, second tensor missing"), a.finalize(h, nullptr), SDFA_ESTATE, a.tensors[1].first);
    const auto &[nameL, nL] = a.tensors[2];
    std::vector<float> last((size_t)nL, -1.f);
    expect(tag("set_tensor, last tensor"), a.set_tensor(h, nameL, last.data(), nL), SDFA_OK, nullptr);
    expect(tag("finalize, still missing"), a.finalize(h, nullptr), SDFA_ESTATE, "is missing");
    expect(tag("numel"), a.numel(h) > nL, 1, nullptr);
    expect(tag("adam, unfinalised"), a.adam(h, 1e-4, 0.9, 0.999, 1e-8, nullptr), SDFA_ESTATE, "not finalised");
    expect(tag("zero_grad, unfinalised"), a.zero_grad(h, nullptr), SDFA_ESTATE, "not finalised");
    expect(tag("get_tensor, unfinalised"), a.get_tensor(h, name0, 0, buf.data(), n0), SDFA_ESTATE, "not finalised");
    expect(tag("set_state, unfinalised"), a.set_state(h, name0, 0, buf.data(), n0), SDFA_ESTATE, "not finalised");
    expect(tag("set_step_count(-1)"), a.set_step_count(h, -1), SDFA_EINVAL, "negative");
    expect(tag("set_step_count(7)"), a.set_step_count(h, 7), SDFA_OK, nullptr);
    expect(tag("step_count"), a.step_count(h), 7, nullptr);
    a.destroy(h);                                                   // of an unfinalised handle: the host copy, no device buffer
    a.destroy(nullptr);
    expect(tag("numel, null handle"), a.numel(nullptr), SDFA_EINVAL, "null handle");
}

int main() {
    const Api apis[] = {
        {"headtrain dgrad", API(headtrain, sdfa_headtrain_create(SDFA_HEADTRAIN_HEAD_DGRAD)),
         {{"_output_module._layers.0.weight_g", 512}, {"_output_module._layers.0.weight_v", 512 * 520}, {"_output_module._rotat_layers.2.bias", 180}}},
        {"headtrain offsets", API(headtrain, sdfa_headtrain_create(SDFA_HEADTRAIN_HEAD_OFFSETS)),
         {{"_output_module._layers.0.weight_g", 512}, {"_output_module._layers.0.weight_v", 512 * 520}, {"_output_module._layers.2.bias", 59}}},
        {"attntrain", API(attntrain, sdfa_attntrain_create()),
         {{"_audio_encoder._layers.10._conv_query.weight", 512 * 512 * 3}, {"_audio_encoder._layers.10.proj_qry.weight", 128 * 512}, {"_audio_encoder._layers.10.b", 128}}},
        {"lstmtrain layer 0", API(lstmtrain, sdfa_lstmtrain_create(256)),
         {{"_audio_encoder._layers.9.weight_ih_l0", 1024 * 256}, {"_audio_encoder._layers.9.weight_ih_l0_reverse", 1024 * 256}, {"_audio_encoder._layers.9.weight_hh_l0_reverse", 1024 * 256}}},
        {"lstmtrain layer 1", API(lstmtrain, sdfa_lstmtrain_create(512)),
         {{"_audio_encoder._layers.9.weight_ih_l1", 1024 * 512}, {"_audio_encoder._layers.9.weight_ih_l1_reverse", 1024 * 512}, {"_audio_encoder._layers.9.weight_hh_l1_reverse", 1024 * 256}}},
        {"freqtrain", API(freqtrain, sdfa_freqtrain_create()),
         {{"_audio_encoder._layers.6._lstm.weight_ih_l0", 512 * 64}, {"_audio_encoder._layers.6._lstm.weight_ih_l0_reverse", 512 * 64}, {"_audio_encoder._layers.6._proj.bias", 256}}},
        {"convtrain", API(convtrain, sdfa_convtrain_create()),
         {{"_audio_encoder._layers.1.weight_g", 32}, {"_audio_encoder._layers.1.weight_v", 32 * 9}, {"_audio_encoder._layers.5._ext_post_bn.bias", 64}}},
    };
    for (const Api &a : apis) run(a);
    expect("headtrain_create(7)", sdfa_headtrain_create(7) ? 0 : -1, -1, "unknown head");
    expect("lstmtrain_create(384)", sdfa_lstmtrain_create(384) ? 0 : -1, -1, "input width");
    // the frequency-LSTM handle's own calls: the step and the encoder exit refuse before they look at a device
    {
        sdfa_freqtrain *h = sdfa_freqtrain_create();
        std::vector<float> wp((size_t)256 * 8192, 0.5f);            // the largest tensor of any handle, copied whole
        expect("freqtrain: set_tensor, _proj.weight", sdfa_freqtrain_set_tensor(h, "_audio_encoder._layers.6._proj.weight", wp.data(), (int64_t)wp.size()), SDFA_OK, nullptr);
        expect("freqtrain: set_tensor, the BiLSTM's name", sdfa_freqtrain_set_tensor(h, "_audio_encoder._layers.9.weight_hh_l0", wp.data(), 1024 * 256), SDFA_EINVAL,
               "the frequency LSTM has no tensor");
        expect("freqtrain: forward, unfinalised", sdfa_freqtrain_forward(h, nullptr, 1, nullptr, nullptr, 0, nullptr), SDFA_ESTATE, "not finalised");
        expect("freqtrain: backward, unfinalised", sdfa_freqtrain_backward(h, nullptr, nullptr, 1, nullptr, nullptr, 0, nullptr), SDFA_ESTATE, "not finalised");
        expect("freqtrain: workspace_bytes(0)", sdfa_freqtrain_workspace_bytes(h, 0), SDFA_EINVAL, "frames outside");
        expect("freqtrain: workspace_bytes(MAX + 1)", sdfa_freqtrain_workspace_bytes(h, SDFA_FREQTRAIN_MAX_FRAMES + 1), SDFA_EINVAL, "frames outside");
        expect("freqtrain: workspace_bytes(MAX) > 2^34", sdfa_freqtrain_workspace_bytes(h, SDFA_FREQTRAIN_MAX_FRAMES) > ((int64_t)1 << 34), 1, nullptr);
        sdfa_freqtrain_destroy(h);                                      // before finalize
        expect("freqtrain: forward, null handle", sdfa_freqtrain_forward(nullptr, nullptr, 1, nullptr, nullptr, 0, nullptr), SDFA_EINVAL, "null handle");
    }
    // the conv-stack handle's own calls: its constants, which lie outside the flat buffers, and the step's refusals
    {
        sdfa_convtrain *h = sdfa_convtrain_create();
        std::vector<float> v((size_t)64 * 32 * 3, 0.5f), c32(32, 1.f), c64(64, 1.f);      // exactly numel floats each
        const char *mean1 = "_audio_encoder._layers.1._ext_post_bn.running_mean", *var5 = "_audio_encoder._layers.5._ext_post_bn.running_var";
        expect("convtrain: set_tensor, layer 3's weight_v", sdfa_convtrain_set_tensor(h, "_audio_encoder._layers.3.weight_v", v.data(), (int64_t)v.size()), SDFA_OK, nullptr);
        expect("convtrain: set_tensor, a constant", sdfa_convtrain_set_tensor(h, mean1, c32.data(), 32), SDFA_OK, nullptr);
        expect("convtrain: set_tensor, the last constant", sdfa_convtrain_set_tensor(h, var5, c64.data(), 64), SDFA_OK, nullptr);
        expect("convtrain: set_tensor, a constant, short numel", sdfa_convtrain_set_tensor(h, var5, c64.data(), 63), SDFA_EINVAL, "elements");
        expect("convtrain: set_tensor, the frequency LSTM's name", sdfa_convtrain_set_tensor(h, "_audio_encoder._layers.6._proj.bias", c64.data(), 256), SDFA_EINVAL,
               "the conv stack has no tensor");
        expect("convtrain: set_state on a constant", sdfa_convtrain_set_state(h, mean1, 0, c32.data(), 32), SDFA_EINVAL, "is a constant");
        expect("convtrain: set_grad on a constant", sdfa_convtrain_set_grad(h, var5, c64.data(), 64), SDFA_EINVAL, "is a constant");
        expect("convtrain: get_tensor of a constant, unfinalised", sdfa_convtrain_get_tensor(h, mean1, 0, c32.data(), 32), SDFA_ESTATE, "not finalised");
        expect("convtrain: finalize, a trainable tensor missing", sdfa_convtrain_finalize(h, nullptr), SDFA_ESTATE, "_layers.1.weight_g");
        expect("convtrain: forward, unfinalised", sdfa_convtrain_forward(h, nullptr, 1, nullptr, nullptr, 0, nullptr), SDFA_ESTATE, "not finalised");
        expect("convtrain: backward, unfinalised", sdfa_convtrain_backward(h, nullptr, nullptr, 1, nullptr, 0, nullptr), SDFA_ESTATE, "not finalised");
        expect("convtrain: workspace_bytes(0)", sdfa_convtrain_workspace_bytes(h, 0), SDFA_EINVAL, "frames outside");
        expect("convtrain: workspace_bytes(MAX + 1)", sdfa_convtrain_workspace_bytes(h, SDFA_CONVTRAIN_MAX_FRAMES + 1), SDFA_EINVAL, "frames outside");
        expect("convtrain: workspace_bytes(MAX) > 2^33", sdfa_convtrain_workspace_bytes(h, SDFA_CONVTRAIN_MAX_FRAMES) > ((int64_t)1 << 33), 1, nullptr);
        sdfa_convtrain_destroy(h);                                      // before finalize
        expect("convtrain: forward, null handle", sdfa_convtrain_forward(nullptr, nullptr, 1, nullptr, nullptr, 0, nullptr), SDFA_EINVAL, "null handle");
    }
    printf(failures ? "trainstate host check: %d UNEXPECTED\n" : "trainstate host check: ok\n", failures);
    return failures ? 1 : 0;
}
