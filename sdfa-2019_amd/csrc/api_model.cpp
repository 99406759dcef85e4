// C ABI of libsdfa_hip.so (include/sdfa_hip.h): model creation -- tensor staging, weight packing, upload.
#include "host.h"
#include "kernels.h"
#include "model.h"

#include <cmath>
#include <cstring>

namespace {

const std::vector<float> *get(const sdfa_model *m, const std::string &name, size_t numel) {
    auto it = m->host.find(name);
    if (it == m->host.end()) { sdfa_fail(SDFA_ESTATE, "tensor '%s' missing", name.c_str()); return nullptr; }
    if (it->second.size() != numel) {
        sdfa_fail(SDFA_ESTATE, "tensor '%s' has %zu elements, expected %zu", name.c_str(), it->second.size(), numel);
        return nullptr;
    }
    return &it->second;
}

// The host image of the weight blob, and the model's device pointers into it: bind() notes which pointer a slot is for, patch() sets
// them all once the blob has its device address.
struct Packer {
    std::vector<float> buf;
    struct Bind { const float **f; const void **v; size_t o; };
    std::vector<Bind> binds;
    size_t add(size_t n) {   // 256-byte aligned slots
        size_t o = (buf.size() + 63) / 64 * 64;
        buf.resize(o + n, 0.f);
        return o;
    }
    size_t bind(const float *&p, size_t o) { binds.push_back({&p, nullptr, o}); return o; }
    size_t bind(const void *&p, size_t o) { binds.push_back({nullptr, &p, o}); return o; }
    void patch(const float *d) const {
        for (const Bind &b : binds) {
            if (b.f) *b.f = d + b.o;
            else *b.v = d + b.o;
        }
    }
};

// W [P][K] row-major (+ row permutation) -> K4 [K/4][Ppad][4], zero padded
size_t pack_k4(Packer &pk, const float *W, int P, int K, int ldw, int col0, int Kpad, int Ppad, const int *perm = nullptr) {
    size_t o = pk.add((size_t)Kpad * Ppad);
    for (int p = 0; p < P; ++p) {
        const float *row = W + (size_t)(perm ? perm[p] : p) * ldw + col0;
        for (int k = 0; k < K; ++k) pk.buf[o + ((size_t)(k / 4) * Ppad + p) * 4 + (k % 4)] = row[k];
    }
    return o;
}

// packed gate row p = w*128 + gate*32 + jj  <->  torch row gate*H + 32*w + jj
std::vector<int> gate_perm(int H) {
    std::vector<int> perm(4 * H);
    for (int w = 0; w < H / 32; ++w)
        for (int g = 0; g < 4; ++g)
            for (int jj = 0; jj < 32; ++jj) perm[w * 128 + g * 32 + jj] = g * H + 32 * w + jj;
    return perm;
}

uint16_t bf16_rne_bits(float x) {   // round-to-nearest-even, as the device's float -> __bf16 conversion
    uint32_t u;
    memcpy(&u, &x, 4);
    if ((u & 0x7F800000u) == 0x7F800000u) return (uint16_t)(u >> 16);
    u += 0x7FFFu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
float bf16_bits_to_float(uint16_t b) {
    const uint32_t u = (uint32_t)b << 16;
    float x;
    memcpy(&x, &u, 4);
    return x;
}
// x = hi + mid + lo to about 24 bits, each term a bf16: what the split-bf16 kernels multiply (two terms: three products, three terms: six)
struct Bf16x3 { uint16_t hi, mid, lo; };
Bf16x3 bf16_split(float x) {
    Bf16x3 s;
    s.hi = bf16_rne_bits(x);
    const float r1 = x - bf16_bits_to_float(s.hi);
    s.mid = bf16_rne_bits(r1);
    s.lo = bf16_rne_bits(r1 - bf16_bits_to_float(s.mid));
    return s;
}
// Element e of hidden-state octet o = 4w + 2q + hh of the bf16 recurrences: hidden units 32w+16q+4hh+{0..3} and 32w+16q+8+4hh+{0..3} -- the
// order in which a lane of the kernels owns its accumulator rows (lstm.hip)
int rec_octet_k(int o, int e) {
    const int w = o >> 2, q = (o >> 1) & 1, hh = o & 1;
    return 32 * w + 16 * q + 4 * hh + (e & 3) + 8 * (e >> 2);
}

// log2 e and 2 log2 e: the frequency LSTM's gate rows are scaled by them at pack time (sdfa_model_finalize)
constexpr float LOG2E = 1.4426950408889634f, TWO_LOG2E = 2.8853900817779268f;

// Conv stack weights for conv123_bf16_kernel (conv.hip): three planes (hi | mid | lo) of 1344 octets of 8 bf16 each,
//   w1 [2 halves][32 co]            k = 8 hh + e: tap df = k / 3, channel c = k % 3 (k >= 9: zero)
//   w2 [6 k-steps][2 halves][64 co] tap df = ks / 2, input channel 8 (2 (ks % 2) + e / 4) + 4 hh + e % 4
//   w3 [4 k-steps][2 halves][64 co] input channel 32 (ks / 2) + 8 (2 (ks % 2) + e / 4) + 4 hh + e % 4
// -- the order in which an accumulator lane of the kernel owns its channels.  Torch layout of w: [co][ci][kf].
void pack_conv_bf16(uint16_t *dst, const float *w1, const float *w2, const float *w3) {
    constexpr size_t PLANE = (size_t)1344 * 8;
    auto put = [&](size_t octet, int e, float x) {
        const Bf16x3 b = bf16_split(x);
        dst[octet * 8 + e] = b.hi; dst[PLANE + octet * 8 + e] = b.mid; dst[2 * PLANE + octet * 8 + e] = b.lo;
    };
    for (int hh = 0; hh < 2; ++hh)
        for (int co = 0; co < 32; ++co)
            for (int e = 0; e < 8; ++e) {
                const int k = 8 * hh + e;
                put((size_t)hh * 32 + co, e, k < 9 ? w1[((size_t)co * 3 + k % 3) * 3 + k / 3] : 0.f);
            }
    for (int ks = 0; ks < 6; ++ks)
        for (int hh = 0; hh < 2; ++hh)
            for (int co = 0; co < 64; ++co)
                for (int e = 0; e < 8; ++e) {
                    const int df = ks >> 1, ci = 8 * (2 * (ks & 1) + (e >> 2)) + 4 * hh + (e & 3);
                    put(64 + ((size_t)ks * 2 + hh) * 64 + co, e, w2[((size_t)co * 32 + ci) * 3 + df]);
                }
    for (int ks = 0; ks < 4; ++ks)
        for (int hh = 0; hh < 2; ++hh)
            for (int co = 0; co < 64; ++co)
                for (int e = 0; e < 8; ++e) {
                    const int ci = 32 * (ks >> 1) + 8 * (2 * (ks & 1) + (e >> 2)) + 4 * hh + (e & 3);
                    put(64 + 768 + ((size_t)ks * 2 + hh) * 64 + co, e, w3[(size_t)co * 64 + ci]);
                }
}

// PCA bases of the dgrad head for pca_dgrad_res_kernel<true> (pca.hip): per triangle block tb (32 triangles: 192 scale + 96 rotat columns)
//   [plane hi | lo] x ( scale: 12 rows r = 2 ks + h of 192 octets | rotat: 24 rows of 96 octets ),  octet e = basis[k = 16 ks + 8 h + e][column]
// -- the B operand of v_mfma_f32_32x32x16_bf16 as a lane reads it.  comp: torch layout [column][k]; k >= kreal and columns past the end are 0.
void pack_pca_bf16(uint16_t *dst, const float *comp_s, const float *comp_r, int64_t cols_s, int64_t cols_r, int64_t ntb) {
    constexpr size_t PLANE = (size_t)(12 * 192 + 24 * 96) * 8;       // bf16 values per plane and triangle block
    for (int64_t tb = 0; tb < ntb; ++tb) {
        uint16_t *blk = dst + (size_t)tb * 2 * PLANE;
        auto put = [&](size_t octet, int e, float x) {
            const Bf16x3 b = bf16_split(x);      // two planes: the second term is this kernel's "lo"
            blk[octet * 8 + e] = b.hi;
            blk[PLANE + octet * 8 + e] = b.mid;
        };
        for (int r = 0; r < 12; ++r)
            for (int c = 0; c < 192; ++c)
                for (int e = 0; e < 8; ++e) {
                    const int k = 8 * r + e;                         // 16 ks + 8 h + e with r = 2 ks + h
                    const int64_t q = tb * 192 + c;
                    put((size_t)r * 192 + c, e, (k < 85 && q < cols_s) ? comp_s[(size_t)q * 85 + k] : 0.f);
                }
        for (int r = 0; r < 24; ++r)
            for (int c = 0; c < 96; ++c)
                for (int e = 0; e < 8; ++e) {
                    const int k = 8 * r + e;
                    const int64_t q = tb * 96 + c;
                    put((size_t)12 * 192 + (size_t)r * 96 + c, e, (k < 180 && q < cols_r) ? comp_r[(size_t)q * 180 + k] : 0.f);
                }
    }
}

// Frequency-LSTM weights for freq_lstm_bf16_kernel / freq_lstm_bf16x6_kernel: per direction [plane hi | mid | lo][24 octets][512 gate rows][8] bf16.
// cat = [W_ih | W_hh] rows in torch order, perm = packed gate row -> torch row.  Octets 0..7 are the 64 input features
// in order; octet 8 + o' holds the hidden units of rec_octet_k(o', .).
void pack_freq_lstm_bf16(uint16_t *dst, const float *cat, const int *perm) {
    for (int O = 0; O < 24; ++O)
        for (int p = 0; p < 512; ++p)
            for (int e = 0; e < 8; ++e) {
                const int k = O < 8 ? 8 * O + e : 64 + rec_octet_k(O - 8, e);
                const Bf16x3 b = bf16_split(cat[(size_t)perm[p] * 192 + k]);
                dst[((size_t)O * 512 + p) * 8 + e] = b.hi;
                dst[((size_t)(24 + O) * 512 + p) * 8 + e] = b.mid;      // the "lo" plane of the three-product split
                dst[((size_t)(48 + O) * 512 + p) * 8 + e] = b.lo;       // third term: six-product split only
            }
}

// Recurrent weights of one BiLSTM direction for time_lstm_bf16_kernel: [plane hi | mid | lo][32 octets][1024 gate rows][8] bf16,
// the K axis (256 hidden units) in the accumulator-row order of the kernel (rec_octet_k).
void pack_rec_bf16(uint16_t *dst, const float *whh, const int *perm) {
    for (int o = 0; o < 32; ++o)
        for (int p = 0; p < 1024; ++p)
            for (int e = 0; e < 8; ++e) {
                const Bf16x3 b = bf16_split(whh[(size_t)perm[p] * 256 + rec_octet_k(o, e)]);
                dst[((size_t)o * 1024 + p) * 8 + e] = b.hi;
                dst[((size_t)(32 + o) * 1024 + p) * 8 + e] = b.mid;
                dst[((size_t)(64 + o) * 1024 + p) * 8 + e] = b.lo;
            }
}

// Recurrent weights of one BiLSTM direction for time_lstm_split16_kernel (v_mfma_f32_16x16x4_f32): float4 [16 K16][4 g][1024 gate rows],
// element j of (K16, g, p) = W_hh[perm[p]][k], k = 8 kb + {0, 4, 1, 5}[g] (m = 0) / {2, 6, 3, 7}[g] (m = 1) with kb = 2 K16 + (j >> 1),
// m = j & 1 -- the order in which the 32x32x2 kernels add a gate row's products (lstm.hip), so both forms give the same bits.
void pack_rec_16x16x4(float *dst, const float *whh, const int *perm) {
    static const int kk[2][4] = {{0, 4, 1, 5}, {2, 6, 3, 7}};
    for (int K16 = 0; K16 < 16; ++K16)
        for (int g = 0; g < 4; ++g)
            for (int p = 0; p < 1024; ++p)
                for (int j = 0; j < 4; ++j) {
                    const int kb = 2 * K16 + (j >> 1), m = j & 1, k = 8 * kb + kk[m][g];
                    dst[(((size_t)K16 * 4 + g) * 1024 + p) * 4 + j] = whh[(size_t)perm[p] * 256 + k];
                }
}

int pack_fc(sdfa_model *m, Packer &pk, const std::string &key, int P, int Kin, bool cond, int act, sdfa_model::Fc &fc) {
    const int Ktot = cond ? Kin + 8 : Kin;
    auto *w = get(m, key + ".weight", (size_t)P * Ktot);
    auto *b = get(m, key + ".bias", P);
    if (!w || !b) return SDFA_ESTATE;
    fc.K = Kin; fc.P = P; fc.Ppad = (int)round_up(P, 128); fc.Pstore = (int)round_up(P, 32); fc.act = act;
    pk.bind(fc.w, pack_k4(pk, w->data(), P, Kin, Ktot, 0, Kin, fc.Ppad));
    memcpy(&pk.buf[pk.bind(fc.b, pk.add(fc.Ppad))], b->data(), P * 4);
    fc.cw = nullptr;
    if (cond) {
        const size_t o = pk.bind(fc.cw, pk.add((size_t)fc.Ppad * 8));
        for (int p = 0; p < P; ++p)
            for (int s = 0; s < 8; ++s) pk.buf[o + ((size_t)(p / 4) * 8 + s) * 4 + (p % 4)] = (*w)[(size_t)p * Ktot + Kin + s];
    }
    return SDFA_OK;
}

}  // namespace

extern "C" {

// ------------------------------------------------------------------------------------------------
sdfa_model *sdfa_model_create(int head) {
    if (head != SDFA_HEAD_DGRAD && head != SDFA_HEAD_OFFSETS) { sdfa_fail(SDFA_EINVAL, "unknown head %d", head); return nullptr; }
    auto *m = new sdfa_model();
    m->head = head;
    m->out_dim = head == SDFA_HEAD_DGRAD ? SDFA_DGRAD_DIM : SDFA_OFFSETS_DIM;
    m->coef_dim = head == SDFA_HEAD_DGRAD ? SDFA_COEF_SCALE + SDFA_COEF_ROTAT : SDFA_COEF_OFFSETS;
    return m;
}

void sdfa_model_destroy(sdfa_model *m) {
    if (!m) return;
    if (m->blob) (void)hipFree(m->blob);
    for (auto &e : m->events) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
    delete m;
}

int sdfa_model_set_tensor(sdfa_model *m, const char *name, const float *h_data, int64_t numel) {
    if (!m || !name || !h_data || numel <= 0) return sdfa_fail(SDFA_EINVAL, "set_tensor: bad argument");
    if (m->finalized) return sdfa_fail(SDFA_ESTATE, "set_tensor after finalize");
    m->host[name].assign(h_data, h_data + numel);
    return SDFA_OK;
}

int sdfa_model_head(const sdfa_model *m) { return m ? m->head : SDFA_EINVAL; }
int64_t sdfa_model_out_dim(const sdfa_model *m) { return m ? m->out_dim : SDFA_EINVAL; }
int64_t sdfa_model_coef_dim(const sdfa_model *m) { return m ? m->coef_dim : SDFA_EINVAL; }

int sdfa_model_finalize(sdfa_model *m, void *stream) {
    if (!m) return sdfa_fail(SDFA_EINVAL, "null model");
    if (m->finalized) return SDFA_OK;
    Packer pk;
    const std::string enc = "_audio_encoder._layers.";
    // ---- conv stack: fold eval BatchNorm (eps 1e-3) into scale/shift applied AFTER LeakyReLU (extend.py:94-101)
    const float **conv_p[3][4] = {{&m->w1, &m->b1, &m->s1, &m->t1}, {&m->w2, &m->b2, &m->s2, &m->t2}, {&m->w3, &m->b3, &m->s3, &m->t3}};   // weights, bias, BN scale, BN shift
    const std::vector<float> *conv_w[3] = {nullptr, nullptr, nullptr};
    const int cshape[3][3] = {{32, 3, 3}, {64, 32, 3}, {64, 64, 1}};   // co, ci, kf
    const int cidx[3] = {1, 3, 5};
    for (int l = 0; l < 3; ++l) {
        const int co = cshape[l][0], ci = cshape[l][1], kf = cshape[l][2];
        const std::string k = enc + std::to_string(cidx[l]);
        auto *w = get(m, k + ".weight", (size_t)co * ci * kf);
        auto *b = get(m, k + ".bias", co);
        auto *g = get(m, k + "._ext_post_bn.weight", co), *be = get(m, k + "._ext_post_bn.bias", co);
        auto *mu = get(m, k + "._ext_post_bn.running_mean", co), *var = get(m, k + "._ext_post_bn.running_var", co);
        if (!w || !b || !g || !be || !mu || !var) return SDFA_ESTATE;
        conv_w[l] = w;
        if (l == 0) {   // A operand [5 k-steps][2 halves][32 co], k = df*3 + c, k = 9 -> 0
            const size_t o_w1 = pk.bind(*conv_p[0][0], pk.add(5 * 2 * 32));
            for (int s = 0; s < 5; ++s)
                for (int hh = 0; hh < 2; ++hh)
                    for (int o = 0; o < 32; ++o) {
                        const int kk = 2 * s + hh;
                        float v = 0.f;
                        if (kk < 9) { const int df = kk / 3, c = kk % 3; v = (*w)[((size_t)o * 3 + c) * 3 + df]; }
                        pk.buf[o_w1 + (s * 2 + hh) * 32 + o] = v;
                    }
        } else {        // K4 [K/4][64][4], k = df*ci + c
            const int K = ci * kf;
            std::vector<float> flat((size_t)co * K);
            for (int o = 0; o < co; ++o)
                for (int c = 0; c < ci; ++c)
                    for (int df = 0; df < kf; ++df) flat[(size_t)o * K + df * ci + c] = (*w)[((size_t)o * ci + c) * kf + df];
            pk.bind(*conv_p[l][0], pack_k4(pk, flat.data(), co, K, K, 0, K, co));
        }
        size_t o_bst[3];
        for (int i = 0; i < 3; ++i) o_bst[i] = pk.bind(*conv_p[l][1 + i], pk.add(co));
        for (int o = 0; o < co; ++o) {
            const double sc = (double)(*g)[o] / std::sqrt((double)(*var)[o] + 1e-3);
            pk.buf[o_bst[0] + o] = (*b)[o];
            pk.buf[o_bst[1] + o] = (float)sc;
            pk.buf[o_bst[2] + o] = (float)((double)(*be)[o] - (double)(*mu)[o] * sc);
        }
    }
    const size_t o_cvwb = pk.bind(m->cv_wb, pk.add((size_t)3 * 1344 * 8 / 2));      // three bf16 planes of 1344 octets, two bf16 per float slot
    pack_conv_bf16(reinterpret_cast<uint16_t *>(&pk.buf[o_cvwb]), conv_w[0]->data(), conv_w[1]->data(), conv_w[2]->data());
    // ---- frequency LSTM: [W_ih | W_hh] concatenated along K, gate rows packed per wave; bias = b_ih + b_hh
    {
        const size_t o_flwb = pk.bind(m->fl_wb, pk.add((size_t)2 * 3 * 24 * 512 * 8 / 2));   // two directions x three bf16 planes, two bf16 per float slot
        const auto perm = gate_perm(128);
        const char *suf[2] = {"", "_reverse"};
        std::vector<float> cat((size_t)512 * 192);
        size_t first = 0;
        std::vector<float> bias(1024);
        auto gate_scale = [](int torch_row) { return torch_row / 128 == 2 ? TWO_LOG2E : LOG2E; };      // gate order i, f, g, o
        for (int d = 0; d < 2; ++d) {
            const std::string k = enc + "6._lstm.";
            auto *wih = get(m, k + "weight_ih_l0" + suf[d], 512 * 64), *whh = get(m, k + "weight_hh_l0" + suf[d], 512 * 128);
            auto *bih = get(m, k + "bias_ih_l0" + suf[d], 512), *bhh = get(m, k + "bias_hh_l0" + suf[d], 512);
            if (!wih || !whh || !bih || !bhh) return SDFA_ESTATE;
            // The cell update needs its gate pre-activations as exponents of two: sigmoid(x) = 1 / (1 + 2^(-x log2 e)), tanh(g) through
            // 2^(-2 g log2 e).  The scaling is folded into the weights and the bias here (rows i, f, o by log2 e, rows g by 2 log2 e:
            // torch gate order i, f, g, o), so the kernel's accumulators ARE the exponents and the update has five vector multiplies
            // per element pair less (round 4; lstm.hip: lstm_cell_quad<true>).  A weight picks up one more fp32 rounding; the stage
            // stays inside its 1e-4 tap tolerance (tests/test_gpu_parity.py) and all launch forms share the packed weights.
            for (int r = 0; r < 512; ++r) {
                const float k = gate_scale(r);
                for (int j = 0; j < 64; ++j) cat[(size_t)r * 192 + j] = (*wih)[(size_t)r * 64 + j] * k;
                for (int j = 0; j < 128; ++j) cat[(size_t)r * 192 + 64 + j] = (*whh)[(size_t)r * 128 + j] * k;
            }
            size_t o = pack_k4(pk, cat.data(), 512, 192, 192, 0, 192, 512, perm.data());
            pack_freq_lstm_bf16(reinterpret_cast<uint16_t *>(&pk.buf[o_flwb]) + (size_t)d * 3 * 24 * 512 * 8, cat.data(), perm.data());
            if (d == 0) first = pk.bind(m->fl_w, o);
            else if (o != first + (size_t)48 * 512 * 4) return sdfa_fail(SDFA_ESTATE, "internal: freq-lstm weights not contiguous");
            for (int p = 0; p < 512; ++p)
                bias[d * 512 + p] = ((*bih)[perm[p]] + (*bhh)[perm[p]]) * gate_scale(perm[p]);
        }
        memcpy(&pk.buf[pk.bind(m->fl_b, pk.add(1024))], bias.data(), 1024 * 4);
    }
    {
        auto *w = get(m, enc + "6._proj.weight", (size_t)256 * 8192), *b = get(m, enc + "6._proj.bias", 256);
        if (!w || !b) return SDFA_ESTATE;
        pk.bind(m->fp_w, pack_k4(pk, w->data(), 256, 8192, 8192, 0, 8192, 256));
        memcpy(&pk.buf[pk.bind(m->fp_b, pk.add(256))], b->data(), 256 * 4);
    }
    // ---- time BiLSTM (bias=False): input projections as one 2048-row GEMM per layer, recurrent weights K4
    {
        size_t o_tlb[2], o_tl16[2];
        const auto perm = gate_perm(256);
        for (int l = 0; l < 2; ++l) o_tlb[l] = pk.bind(m->tl_wb[l], pk.add((size_t)2 * 3 * 32 * 1024 * 8 / 2));   // two directions x three bf16 planes, two bf16 per float slot
        for (int l = 0; l < 2; ++l) o_tl16[l] = pk.bind(m->tl_w16[l], pk.add((size_t)2 * 16 * 4 * 1024 * 4));      // two directions, 16x16x4 operand order
        const char *suf[2] = {"", "_reverse"};
        for (int l = 0; l < 2; ++l) {
            const int Kin = l == 0 ? 256 : 512;
            std::vector<float> both((size_t)2048 * Kin);
            size_t first = 0;
            for (int d = 0; d < 2; ++d) {
                auto *wih = get(m, enc + "9.weight_ih_l" + std::to_string(l) + suf[d], (size_t)1024 * Kin);
                auto *whh = get(m, enc + "9.weight_hh_l" + std::to_string(l) + suf[d], (size_t)1024 * 256);
                if (!wih || !whh) return SDFA_ESTATE;
                for (int p = 0; p < 1024; ++p) memcpy(&both[((size_t)d * 1024 + p) * Kin], &(*wih)[(size_t)perm[p] * Kin], Kin * 4);
                size_t o = pack_k4(pk, whh->data(), 1024, 256, 256, 0, 256, 1024, perm.data());
                pack_rec_bf16(reinterpret_cast<uint16_t *>(&pk.buf[o_tlb[l]]) + (size_t)d * 3 * 32 * 1024 * 8, whh->data(), perm.data());
                pack_rec_16x16x4(&pk.buf[o_tl16[l]] + (size_t)d * 16 * 4 * 1024 * 4, whh->data(), perm.data());
                if (d == 0) first = pk.bind(m->tl_w[l], o);
                else if (o != first + (size_t)64 * 1024 * 4) return sdfa_fail(SDFA_ESTATE, "internal: time-lstm weights not contiguous");
            }
            pk.bind(m->gx_w[l], pack_k4(pk, both.data(), 2048, Kin, Kin, 0, Kin, 2048));
            if (l == 1) {
                // the fused recurrence (time_lstm_fused_kernel) contracts [x_t | h] itself: per direction ONE image, K4 [128 k-quads of
                // W_ih | 64 of W_hh][1024 packed gate rows][4], so its K loop walks the two parts without a break
                const size_t o_x = pk.bind(m->tl_wxh1, pk.add((size_t)2 * 192 * 1024 * 4));
                for (int d = 0; d < 2; ++d) {
                    auto *whh = get(m, enc + "9.weight_hh_l1" + suf[d], (size_t)1024 * 256);
                    float *img = &pk.buf[o_x + (size_t)d * 192 * 1024 * 4];
                    for (int p = 0; p < 1024; ++p) {
                        for (int k = 0; k < 512; ++k) img[((size_t)(k / 4) * 1024 + p) * 4 + k % 4] = both[((size_t)d * 1024 + p) * 512 + k];
                        for (int k = 0; k < 256; ++k) img[((size_t)(128 + k / 4) * 1024 + p) * 4 + k % 4] = (*whh)[(size_t)perm[p] * 256 + k];
                    }
                }
            }
        }
    }
    // ---- attention
    {
        const std::string k = enc + "10.";
        auto *cq = get(m, k + "_conv_query.weight", (size_t)512 * 512 * 3), *wk = get(m, k + "proj_key.weight", 128 * 512);
        auto *wq = get(m, k + "proj_qry.weight", 128 * 512), *v = get(m, k + "v.weight", 128), *b = get(m, k + "b", 128);
        if (!cq || !wk || !wq || !v || !b) return SDFA_ESTATE;
        pk.bind(m->kp_w, pack_k4(pk, wk->data(), 128, 512, 512, 0, 512, 128));
        pk.bind(m->qp_w, pack_k4(pk, wq->data(), 128, 512, 512, 0, 512, 128));
        std::vector<float> flat((size_t)512 * 1536);   // k = tap*512 + c
        for (int o = 0; o < 512; ++o)
            for (int c = 0; c < 512; ++c)
                for (int t = 0; t < 3; ++t) flat[(size_t)o * 1536 + t * 512 + c] = (*cq)[((size_t)o * 512 + c) * 3 + t];
        pk.bind(m->qc_w, pack_k4(pk, flat.data(), 512, 1536, 1536, 0, 1536, 512));
        memcpy(&pk.buf[pk.bind(m->at_v, pk.add(128))], v->data(), 512);
        memcpy(&pk.buf[pk.bind(m->at_b, pk.add(128))], b->data(), 512);
    }
    // ---- output module
    const std::string om = "_output_module.";
    // PCA basis b: compT [cols][kreal] as the K4 operand [pca_K / 4][pca_ld][4] (zero padded), means [pca_ld]
    auto pack_basis = [&](int b, const std::vector<float> &compT, int kreal, const std::vector<float> &means) {
        pk.bind(m->pca_q[b], pack_k4(pk, compT.data(), (int)m->pca_cols[b], kreal, kreal, 0, m->pca_K[b], (int)m->pca_ld[b]));
        memcpy(&pk.buf[pk.bind(m->pca_bias[b], pk.add(m->pca_ld[b]))], means.data(), m->pca_cols[b] * 4);
    };
    if (m->head == SDFA_HEAD_DGRAD) {
        if (pack_fc(m, pk, om + "_layers.0", 512, 512, true, ACT_LRELU, m->trunk)) return SDFA_ESTATE;
        const char *brn[2] = {"_scale_layers.", "_rotat_layers."};
        const int nco[2] = {SDFA_COEF_SCALE, SDFA_COEF_ROTAT};
        for (int b = 0; b < 2; ++b) {
            if (pack_fc(m, pk, om + brn[b] + "0", 512, 512, true, ACT_LRELU, m->br[b][0])) return SDFA_ESTATE;
            if (pack_fc(m, pk, om + brn[b] + "1", 256, 512, false, ACT_TANH, m->br[b][1])) return SDFA_ESTATE;
            if (pack_fc(m, pk, om + brn[b] + "2", nco[b], 256, false, ACT_NONE, m->br[b][2])) return SDFA_ESTATE;
        }
        auto *cs = get(m, om + "_scale_pca.compT", (size_t)59856 * 85), *ms = get(m, om + "_scale_pca.means", 59856);
        auto *cr = get(m, om + "_rotat_pca.compT", (size_t)29928 * 180), *mr = get(m, om + "_rotat_pca.means", 29928);
        if (!cs || !ms || !cr || !mr) return SDFA_ESTATE;
        // two bases; the GEMM epilogue scatters column q of basis b to output coordinate (q / g) * 9 + off + q % g,
        // which IS the [s0..s5 r0 r1 r2] interleave of data_to_anime_feat (model.py:246-257)
        m->pca_n = 2;
        const std::vector<float> *comp[2] = {cs, cr}, *mean[2] = {ms, mr};
        const int kreal[2] = {85, 180};
        for (int b = 0; b < 2; ++b) {
            m->pca_K[b] = b ? 192 : 96; m->pca_k0[b] = b ? 96 : 0; m->pca_group[b] = b ? 3 : 6; m->pca_off[b] = b ? 6 : 0;
            m->pca_cols[b] = b ? 29928 : 59856; m->pca_ld[b] = round_up(m->pca_cols[b], 128);
            pack_basis(b, *comp[b], kreal[b], *mean[b]);
        }
        {   // the same bases as bf16 octets for the split-bf16 form of the fused kernel
            const int64_t ntb = (m->pca_cols[1] + 95) / 96;
            const size_t o_pqb = pk.bind(m->pca_qb, pk.add((size_t)ntb * 2 * (12 * 192 + 24 * 96) * 8 / 2));      // two bf16 per float slot
            pack_pca_bf16(reinterpret_cast<uint16_t *>(&pk.buf[o_pqb]), cs->data(), cr->data(), m->pca_cols[0], m->pca_cols[1], ntb);
        }
    } else {
        if (pack_fc(m, pk, om + "_layers.0", 512, 512, true, ACT_LRELU, m->off[0])) return SDFA_ESTATE;
        if (pack_fc(m, pk, om + "_layers.1", 256, 512, false, ACT_TANH, m->off[1])) return SDFA_ESTATE;
        if (pack_fc(m, pk, om + "_layers.2", SDFA_COEF_OFFSETS, 256, false, ACT_NONE, m->off[2])) return SDFA_ESTATE;
        auto *cp = get(m, om + "_pca.compT", (size_t)SDFA_OFFSETS_DIM * 59), *mp = get(m, om + "_pca.means", SDFA_OFFSETS_DIM);
        if (!cp || !mp) return SDFA_ESTATE;
        m->pca_n = 1;
        m->pca_K[0] = 64; m->pca_k0[0] = 0; m->pca_group[0] = 0; m->pca_off[0] = 0;
        m->pca_cols[0] = SDFA_OFFSETS_DIM; m->pca_ld[0] = round_up(SDFA_OFFSETS_DIM, 128);
        pack_basis(0, *cp, 59, *mp);
    }
    // ---- upload
    HIP_TRY(hipMalloc(&m->blob, pk.buf.size() * 4));
    HIP_TRY(hipMemcpyAsync(m->blob, pk.buf.data(), pk.buf.size() * 4, hipMemcpyHostToDevice, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));   // host staging buffer dies with this call
    pk.patch((const float *)m->blob);
    m->host.clear();
    m->finalized = true;
    return SDFA_OK;
}

}  // extern "C"
