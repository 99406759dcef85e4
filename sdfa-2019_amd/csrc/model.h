// struct sdfa_model: what sdfa_model_finalize packs (api_model.cpp) and the forward calls read (api_forward.cpp).
#pragma once
#include "../../include/sdfa_hip.h"

#include <hip/hip_runtime.h>
#include <atomic>
#include <map>
#include <mutex>
#include <string>
#include <vector>

struct sdfa_model {
    int head = SDFA_HEAD_DGRAD;
    bool finalized = false;
    bool keep = false;      // debug: no workspace aliasing, so taps stay valid
    bool profile = false;
    std::map<std::string, std::vector<float>> host;
    void *blob = nullptr;   // all packed weights
    // device pointers into blob
    const float *w1, *b1, *s1, *t1, *w2, *b2, *s2, *t2, *w3, *b3, *s3, *t3;
    const float *fl_w, *fl_b, *fp_w, *fp_b;
    const void *fl_wb = nullptr;   // frequency-LSTM weights as bf16 hi/lo planes (mixed-precision modes)
    const void *cv_wb = nullptr;   // conv stack weights as bf16 planes in the K order of conv123_bf16_kernel (mixed-precision modes)
    int precision = SDFA_PREC_FP32;
    const float *gx_w[2], *tl_w[2];
    const void *tl_wb[2] = {nullptr, nullptr};   // BiLSTM recurrent weights as bf16 hi/lo planes (mixed-precision modes)
    const float *tl_w16[2] = {nullptr, nullptr}; // BiLSTM recurrent weights in the operand order of time_lstm_split16_kernel
    const float *tl_wxh1 = nullptr;              // layer 1 of the BiLSTM: [W_ih | W_hh] along K per direction, the operand image of time_lstm_fused_kernel
    const float *kp_w, *qc_w, *qp_w, *at_v, *at_b;
    struct Fc { const float *w, *b, *cw; int K, P, Ppad, Pstore; int act; };
    Fc trunk, br[2][3], off[3];
    // PCA expansion: dgrad = two bases (scale K 96 -> 6 of every 9 output columns, rotat K 192 -> the other 3);
    // offsets = one basis (K 64)
    int pca_n = 0;
    const float *pca_q[2], *pca_bias[2];
    const void *pca_qb = nullptr;              // dgrad head: both bases as bf16 octets (hi | lo planes) for the split-bf16 PCA kernel (pack_pca_bf16)
    int pca_K[2], pca_k0[2], pca_group[2], pca_off[2];
    std::atomic<int> freq_shape{9};   // launch form of the fp32 frequency LSTM (kernels.h FreqLstmArgs::shape); sdfa_model_autotune measures and sets it
                                      // (atomic: forwards on other threads may read it while an autotune call stores the winner)
    std::atomic<int> reserved_cus{0}; // CUs the persistent kernels leave free (sdfa_model_set_reserved_cus)
    int64_t pca_ld[2], pca_cols[2];
    int64_t out_dim, coef_dim;
    // profiling
    struct Ev { std::string stage; hipEvent_t a, b; };
    mutable std::vector<Ev> events;
    mutable std::mutex ev_mu;   // profiling appends events from const forward calls, possibly on several threads
};
