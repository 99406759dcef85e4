// C ABI of libsdfa_hip.so (include/sdfa_hip.h): the forward calls -- workspace layout and status, profiling, precision modes,
// autotune, encoder / regressor / PCA expansion, debug taps.
#include "common.h"
#include "host.h"
#include "kernels.h"
#include "model.h"
#include "../../include/sdfa_bilstm.h"
#include "../../include/sdfa_freqtrain.h"

#include <algorithm>

// A/B options this file reads (api_core.cpp)
extern thread_local int g_sdfa_gemm_variant, g_sdfa_freq_lstm_shape, g_sdfa_pca_lds, g_sdfa_pca_fp32, g_sdfa_conv_fp32, g_sdfa_share_gx0_off, g_sdfa_attn_unfused, g_sdfa_encoder_dedup_off,
    g_sdfa_freq_proj_tail, g_sdfa_share_hash_bits;

// ================================================================================================
// workspace layout (floats), per chunk of Nc frames, Mc = 64*Nc columns
// ================================================================================================
namespace {

constexpr int64_t CT_WORDS = 2048, CT_FLAGS = 16, ST_WORDS = SDFA_WS_STATUS_BYTES / 4;

struct Ws {
    int64_t P1, X3, HF, Z, GX, H0, H1, KP, QC, QP, ZK, SH, ZU, total;   // offsets in floats
    int64_t TRUNK, A0, A1, COEF;        // regressor scratch: K4 slabs of Nc columns
    int64_t CT_FREQ, CT_PCA, CT_FLAG;   // control words (ints)
};

Ws layout(int64_t Nc, bool keep) {
    const int64_t Mc = 64 * Nc;
    Ws w{};
    int64_t o = 0;
    auto take = [&](int64_t n) { int64_t r = o; o += round_up(n, 64); return r; };
    take(ST_WORDS);       // the status block (sdfa_workspace_init / sdfa_workspace_status*): always the first 256 bytes, whatever Nc
    if (keep) {   // debug: nothing aliased, taps stay valid after the forward
        w.P1 = take(2048 * Mc); w.X3 = take(2048 * Mc); w.HF = take((int64_t)HF_SLAB_ROWS * 4 * Mc); w.Z = take(256 * Mc);
        w.GX = take(2048 * Mc); w.H0 = take(512 * Mc); w.H1 = take(512 * Mc); w.KP = take(128 * Mc);
    } else {
        const int64_t A = take(2048 * Mc);   // P1, later GX
        const int64_t B = take(2048 * Mc);   // X3, later Z | H0 | H1 | KP
        w.HF = take((int64_t)HF_SLAB_ROWS * 4 * Mc);
        w.P1 = A; w.GX = A;
        w.X3 = B; w.Z = B; w.H0 = B + 256 * Mc; w.H1 = B + 768 * Mc; w.KP = B + 1280 * Mc;
    }
    w.QC = take(512 * Nc); w.QP = take(128 * Nc); w.ZK = take(512 * Nc);
    const int64_t R = take(2560 * Nc);   // regressor scratch: trunk 512 rows | a 512 | b 256 | coef up to 288 (the branches of the dgrad head share a / b)
    w.TRUNK = R; w.A0 = R + 512 * Nc; w.A1 = R + 1024 * Nc; w.COEF = R + 1280 * Nc;
    w.SH = take(sdfa_share_table_words(Nc) + 111);   // column-sharing tables (int32 / int64 counters), with the slack they have always had
    w.ZU = keep ? take(256 * Mc) : w.P1; // freq-proj output over distinct columns (pool1 is dead by then)
    const int64_t CT = take(CT_WORDS);   // ints: [0] / [1] work-queue heads of the persistent kernels (frequency LSTM / PCA expansion); [16 ..] the flag
                                         // block of time_lstm_split_kernel (timeout word + one flag per workgroup, at most 4 per CU-sized grid)
    w.CT_FREQ = CT; w.CT_PCA = CT + 1; w.CT_FLAG = CT + CT_FLAGS;
    w.total = o;
    return w;
}

int64_t capacity(int64_t bytes, bool keep) {   // largest Nc (multiple of 128) whose layout fits
    const int64_t per128 = layout(128, keep).total * 4;
    int64_t nc = (bytes / per128 + 2) * 128;   // per-frame cost shrinks slightly with Nc (fixed paddings): start above
    while (nc > 0 && layout(nc, keep).total * 4 > bytes) nc -= 128;
    return nc;
}

struct Prof {
    const sdfa_model *m;
    hipStream_t s;
    hipEvent_t pending = nullptr;
    void begin(const char *stage) {
        if (!m->profile) return;
        sdfa_model::Ev e; e.stage = stage;
        (void)hipEventCreate(&e.a); (void)hipEventCreate(&e.b);
        (void)hipEventRecord(e.a, s);
        pending = e.b;
        std::lock_guard<std::mutex> lk(m->ev_mu);
        m->events.push_back(e);
    }
    void end() {
        if (!m->profile || !pending) return;
        (void)hipEventRecord(pending, s);
        pending = nullptr;
    }
};

GemmArgs gemm_fc(const sdfa_model::Fc &fc, const float *Q, int64_t ldq, float *D, int64_t Nc, const int64_t *spk, int64_t nreal) {
    GemmArgs g = sdfa_gemm_k4(fc.w, fc.Ppad, Q, ldq, D, Nc, fc.K);
    g.bias = fc.b; g.cond_w = fc.cw; g.cond_idx = fc.cw ? spk : nullptr;
    g.Pstore = fc.Pstore; g.Qreal = nreal; g.act = fc.act;
    return g;
}

}  // namespace

extern "C" {

int64_t sdfa_workspace_bytes(const sdfa_model *m, int64_t max_frames) {
    if (!m || max_frames <= 0) return sdfa_fail(SDFA_EINVAL, "workspace_bytes: bad argument");
    return layout(round_up(max_frames, 128), m->keep).total * 4;
}

int sdfa_debug_keep_intermediates(sdfa_model *m, int on) {
    if (!m) return sdfa_fail(SDFA_EINVAL, "null model");
    m->keep = on != 0;
    return SDFA_OK;
}

int sdfa_profile_enable(sdfa_model *m, int on) {
    if (!m) return sdfa_fail(SDFA_EINVAL, "null model");
    std::lock_guard<std::mutex> lk(m->ev_mu);
    m->profile = on != 0;
    for (auto &e : m->events) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
    m->events.clear();
    return SDFA_OK;
}

float sdfa_profile_ms(const sdfa_model *m, const char *stage) {
    if (!m || !stage) return (float)sdfa_fail(SDFA_EINVAL, "profile_ms: bad argument");
    float total = 0.f;
    bool any = false;
    std::lock_guard<std::mutex> lk(m->ev_mu);
    for (auto &e : m->events)
        if (e.stage == stage) {
            float ms = 0.f;
            if (hipEventSynchronize(e.b) != hipSuccess || hipEventElapsedTime(&ms, e.a, e.b) != hipSuccess)
                return (float)sdfa_fail(SDFA_EHIP, "profile_ms: event query failed");
            total += ms; any = true;
        }
    return any ? total : (float)sdfa_fail(SDFA_EINVAL, "profile_ms: no such stage '%s'", stage);
}

int sdfa_profile_reset(sdfa_model *m) { return m ? sdfa_profile_enable(m, m->profile) : sdfa_fail(SDFA_EINVAL, "null model"); }

// Mixed-precision modes (BASELINE configs[3]).  Which MFMA each stage runs on: 0 = fp32, 1 = bf16 operands,
// 3 = split-bf16 (hi/lo operands, three MFMAs per product).  The conv stack, the fused dgrad PCA expansion, softmax/context
// and every accumulation, cell state, bias and activation stay fp32 in all modes.
enum { STAGE_BODY = 0, STAGE_ATTENTION = 1, STAGE_REGRESSOR = 2 };
static int stage_terms(const sdfa_model *m, int stage) {
    switch (m->precision) {
    case SDFA_PREC_BF16_ATTENTION: return stage == STAGE_ATTENTION ? 1 : 0;
    case SDFA_PREC_BF16X3_ATTENTION: return stage == STAGE_ATTENTION ? 3 : 0;
    case SDFA_PREC_BF16X6: return 6;
    case SDFA_PREC_BF16X3: return 3;
    case SDFA_PREC_BF16: return 1;
    default: return 0;
    }
}

int sdfa_model_set_precision(sdfa_model *m, int mode) {
    if (!m) return sdfa_fail(SDFA_EINVAL, "null model");
    if (mode < SDFA_PREC_FP32 || mode > SDFA_PREC_BF16X6) return sdfa_fail(SDFA_EINVAL, "unknown precision mode %d", mode);
    m->precision = mode;
    return SDFA_OK;
}

int sdfa_model_precision(const sdfa_model *m) { return m ? m->precision : SDFA_EINVAL; }

// The persistent / one-workgroup-per-CU kernels (frequency LSTM, the fat GEMMs, the PCA expansion) size their grids to the
// device's CU count; with k reserved they launch (CUs - k) workgroups, so that kernels of another stream (an RCCL
// all-gather, a copy kernel) find free CUs while they run.
int sdfa_model_set_reserved_cus(sdfa_model *m, int k) {
    if (!m) return sdfa_fail(SDFA_EINVAL, "null model");
    if (k < 0 || k > 128) return sdfa_fail(SDFA_EINVAL, "reserved_cus must be in [0, 128], got %d", k);
    m->reserved_cus.store(k);
    return SDFA_OK;
}

// ------------------------------------------------------------------------------------------------
static int encoder_impl(const sdfa_model *m, const float *d_audio_feat, int64_t n_frames, const int32_t *d_frame_clip,
                        const int64_t *d_frame_start, int hop, float *d_z, float *d_align, float *d_H, void *d_workspace,
                        int64_t workspace_bytes, void *stream, float *d_X1 = nullptr, float *d_X0 = nullptr, float *d_C = nullptr) {
    // d_H (sdfa_encoder_memory): every chunk's BiLSTM output leaves the K4 region as [n][64][512] before the next chunk reuses it;
    // d_z may then be null.  Null for every other entry point, which launch what they always launched.
    // d_X1 (sdfa_encoder_layer0): every chunk's layer-0 output leaves its K4 region the same way, and the chunk ends there: no
    // layer 1, no attention.  d_z, d_align and d_H are null then.
    // d_X0 (sdfa_encoder_x0): every chunk's frequency projection leaves its K4 region as [n][64][256], and the chunk ends there: no
    // BiLSTM.  The projection has to exist for every column then, so the chunk takes the expand-then-project order's first half.
    // d_C (sdfa_encoder_conv): every chunk's conv-stack output leaves X3 as [n][64][32][64], through the share map where X3 holds the
    // distinct columns only, and the chunk ends there: no frequency LSTM.
    if (!m || !m->finalized) return sdfa_fail(SDFA_ESTATE, "encoder_forward: model not finalised");
    if (n_frames == 0) return SDFA_OK;
    if (!d_audio_feat || (!d_z && !d_H && !d_X1 && !d_X0 && !d_C) || !d_workspace || n_frames < 0) return sdfa_fail(SDFA_EINVAL, "encoder_forward: bad argument");
    if (((uintptr_t)d_workspace | (uintptr_t)d_audio_feat | (uintptr_t)d_z | (uintptr_t)d_H | (uintptr_t)d_X1 | (uintptr_t)d_X0 | (uintptr_t)d_C) & 15) return sdfa_fail(SDFA_EINVAL, "encoder_forward: pointers must be 16-byte aligned");
    if ((uintptr_t)d_align & 3) return sdfa_fail(SDFA_EINVAL, "encoder_forward: d_align must be 4-byte aligned");
    const int64_t cap = capacity(workspace_bytes, m->keep);
    if (cap < 128) return sdfa_fail(SDFA_ENOSPACE, "encoder_forward: workspace of %lld bytes holds no 128-frame chunk", (long long)workspace_bytes);
    hipStream_t s = (hipStream_t)stream;
    Prof pf{m, s};
    float *ws = (float *)d_workspace;
    for (int64_t f0 = 0; f0 < n_frames; f0 += cap) {
        const int64_t N = std::min(cap, n_frames - f0);
        const int64_t Nc = round_up(N, 128), Mc = 64 * Nc;
        const Ws w = layout(Nc, m->keep);
        ConvArgs ca{};
        ca.audio_feat = d_audio_feat + f0 * (64 * 128 * 3); ca.N = N; ca.Nc = Nc; ca.Mc = Mc;
        ca.w1 = m->w1; ca.b1 = m->b1; ca.s1 = m->s1; ca.t1 = m->t1; ca.P1 = ws + w.P1;
        ca.w2 = m->w2; ca.b2 = m->b2; ca.s2 = m->s2; ca.t2 = m->t2;
        ca.w3 = m->w3; ca.b3 = m->b3; ca.s3 = m->s3; ca.t3 = m->t3; ca.X3 = ws + w.X3;
        // Column sharing (share.hip): with the frame table, the map comes from the table.  Without one it comes from the features
        // themselves -- every link compared in full on the device, per chunk, on every call -- unless the debug taps are on (they read
        // the every-column layout) or "encoder_dedup_off" asks for the every-column path.
        const bool table = d_frame_clip != nullptr;
        const bool share = table || (!m->keep && !g_sdfa_encoder_dedup_off);
        const int64_t *d_ulimit = nullptr;     // device scalar: number of distinct columns, padded to 256
        int32_t *col_to_u = nullptr;
        bool split_tail = false;               // the frequency projection as whole rounds of gemm_fat_kernel + sdfa_launch_gemm_tail
        int64_t fat_grid = 0;
        const int64_t *d_qfull = nullptr;
        if (share) {
            ShareArgs sa{};
            sa.N = N; sa.Nc = Nc; sa.Mc = Mc;
            sdfa_share_carve(sa, reinterpret_cast<int32_t *>(ws + w.SH));
            // the fat kernel is what multiplies the projection (gemm.hip: launch_any): its last partial round goes to the tail kernel
            split_tail = !m->keep && stage_terms(m, STAGE_BODY) == 0 && g_sdfa_gemm_variant == 0 && Mc / 256 >= 512 && g_sdfa_freq_proj_tail != 1;
            if (split_tail) {
                fat_grid = sdfa_fat_grid(256, Mc, sdfa_cu_count(), m->reserved_cus.load());
                sa.fat_grid = (int)fat_grid; sa.tail_mode = g_sdfa_freq_proj_tail;
            }
            pf.begin("share_map");
            if (table) {
                sa.frame_clip = d_frame_clip + f0; sa.frame_start = d_frame_start + f0; sa.hop = hop;
                sa.t_lo = 6; sa.t_hi = 58;      // feature columns: see share.hip
                HIP_TRY(sdfa_launch_share_map(sa, s));
            } else {
                // scratch of the scan (hashes + the group table, under 14 Mc words): the head of the frequency LSTM's hidden-state region, which
                // nobody has written yet in this chunk (the conv stack writes X3; the frequency LSTM is HF's first writer) and which is 8192 Mc words long
                sa.feat = ca.audio_feat;
                sa.hash = reinterpret_cast<uint64_t *>(ws + w.HF);
                sa.group_slots = sdfa_share_group_slots(N);
                sa.group_key = sa.hash + Mc; sa.group_first = reinterpret_cast<uint32_t *>(sa.group_key + sa.group_slots);
                sa.hash_bits = g_sdfa_share_hash_bits;
                HIP_TRY(sdfa_launch_share_map_content(sa, s));
            }
            pf.end();
            d_ulimit = sa.counts + 1; d_qfull = sa.counts + 2; col_to_u = sa.col_to_u;
            ca.col_src = sa.col_src; ca.col_limit = d_ulimit;
        }
        const int conv_terms = g_sdfa_conv_fp32 ? 0 : stage_terms(m, STAGE_BODY);
        if (m->keep && conv_terms) {
            // debug taps in a body precision mode: the X3 tap must be the arithmetic that ships -- conv123_bf16_kernel -- so a
            // packing or K-order bug in pack_conv_bf16 can be localised; the pool1 tap (which the fused kernel never writes) stays fp32
            pf.begin("conv1"); HIP_TRY(sdfa_launch_conv1(ca, s)); pf.end();
            ca.wb = m->cv_wb; ca.terms = conv_terms;
            pf.begin("conv23"); HIP_TRY(sdfa_launch_conv123(ca, s)); pf.end();
        } else if (m->keep) {   // the debug taps read pool1
            pf.begin("conv1"); HIP_TRY(sdfa_launch_conv1(ca, s)); pf.end();
            pf.begin("conv23"); HIP_TRY(sdfa_launch_conv23(ca, s)); pf.end();
        } else {
            ca.wb = m->cv_wb; ca.terms = conv_terms;      // the mixed-precision modes run the stack on bf16 MFMA too
            pf.begin("conv23"); HIP_TRY(sdfa_launch_conv123(ca, s)); pf.end();
        }

        if (d_C) {       // X3 holds the distinct columns on the shared path: col_to_u is null on the every-column path
            HIP_TRY(sdfa_launch_conv_rows(ws + w.X3, col_to_u, N, Nc, d_C + f0 * (64 * 2048), s));
            continue;
        }

        // launch form: the "freq_lstm_shape" option if set; else, for the fp32 kernel, what sdfa_model_autotune measured (the split-bf16
        // kernels have their own default: the autotuned fp32 form says nothing about them)
        const int fl_terms = stage_terms(m, STAGE_BODY);
        FreqLstmArgs fa{ws + w.X3, m->fl_w, m->fl_b, ws + w.HF, Mc, d_ulimit, m->fl_wb, fl_terms, reinterpret_cast<int *>(ws + w.CT_FREQ),
                        g_sdfa_freq_lstm_shape ? g_sdfa_freq_lstm_shape : (fl_terms ? 0 : m->freq_shape.load()), m->reserved_cus.load()};
        pf.begin("freq_lstm"); HIP_TRY(sdfa_launch_freq_lstm(fa, s)); pf.end();

        GemmArgs g = sdfa_gemm_k4(m->fp_w, 256, ws + w.HF, Mc, ws + w.Z, Mc, 8192);   // FreqLstm._proj: Linear(8192 -> 256) + bias
        g.bias = m->fp_b; g.q_tile_major = 1; g.q_slab_rows = HF_SLAB_ROWS;
        g.terms = stage_terms(m, STAGE_BODY);
        g.reserve_cus = m->reserved_cus.load();
        if (share) { g.D = ws + w.ZU; g.q_limit = split_tail ? d_qfull : d_ulimit; }
        pf.begin("freq_proj");
        HIP_TRY(sdfa_launch_gemm(g, s));
        if (split_tail) {      // columns [q_full, limit): at most fat_grid - 1 tiles, none when the rule declined
            GemmTailArgs gt{m->fp_w, ws + w.HF, m->fp_b, ws + w.ZU, Mc, HF_SLAB_ROWS, d_qfull, d_ulimit, (int)fat_grid - 1};
            HIP_TRY(sdfa_launch_gemm_tail(gt, s));
        }
        pf.end();
        // Column sharing reaches one stage further (round 4): the layer-0 input projection of the BiLSTM (rnn.py:20-21) is per column
        // too, so it runs over the DISTINCT columns and the layer-0 recurrence reads it through the share map -- the 256-feature
        // projection is then never expanded at all.  (fp32 kernels; the bf16 recurrences and the debug taps, which read the
        // expanded projection, keep the expand-then-project order.)  The projected columns live in the frequency LSTM's hidden-state
        // region, which is dead once the projection above has read it.
        const bool share_gx0 = share && !m->keep && stage_terms(m, STAGE_BODY) == 0 && !g_sdfa_share_gx0_off && !d_X0;
        if (share && !share_gx0) {   // scatter every distinct column's 256 features to all the (t, n) columns that contain it
            pf.begin("share_expand"); HIP_TRY(sdfa_launch_expand_cols(ws + w.ZU, col_to_u, ws + w.Z, 64, Mc, s)); pf.end();
        }

        if (d_X0) {      // Z (X3's place where nothing is kept: the frequency LSTM has read X3) holds every column's projection
            HIP_TRY(sdfa_launch_x0_rows(ws + w.Z, N, Nc, d_X0 + f0 * (64 * 256), s));
            continue;
        }

        const float *xin = share_gx0 ? ws + w.ZU : ws + w.Z;
        float *hout[2] = {ws + w.H0, ws + w.H1};
        const char *gxn[2] = {"gx0", "gx1"}, *lsn[2] = {"lstm0", "lstm1"};
        for (int l = 0; l < 2; ++l) {
            const bool mapped = share_gx0 && l == 0;
            float *gx = mapped ? ws + w.HF : ws + w.GX;
            GemmArgs gi = sdfa_gemm_k4(m->gx_w[l], 2048, xin, Mc, gx, Mc, l == 0 ? 256 : 512);
            gi.terms = stage_terms(m, STAGE_BODY);
            gi.reserve_cus = m->reserved_cus.load();
            if (mapped) gi.q_limit = d_ulimit;
            TimeLstmArgs ta{gx, m->tl_w[l], hout[l], Nc, Mc, m->tl_wb[l], stage_terms(m, STAGE_BODY),
                            reinterpret_cast<unsigned *>(ws + w.CT_FLAG), CT_WORDS - CT_FLAGS, m->tl_w16[l],
                            reinterpret_cast<unsigned *>(ws), m->reserved_cus.load(), mapped ? col_to_u : nullptr};
            // Layer 1, exact fp32, large chunks: the recurrence contracts [x_t | h] itself (time_lstm_fused_kernel), so the projection GEMM and
            // the round trip of its 2048 x Mc output through HBM go away; the GX region stays unused.  (The debug taps keep the two-kernel
            // path.)  The stage name stays, empty, for the profile readers; "lstm1" then carries the fused kernel's time.
            if (l == 1 && !m->keep) { ta.X = xin; ta.Wxh = m->tl_wxh1; }
            pf.begin(gxn[l]);
            if (!sdfa_time_lstm_fuses_x(ta)) HIP_TRY(sdfa_launch_gemm(gi, s));
            pf.end();
            pf.begin(lsn[l]); HIP_TRY(sdfa_launch_time_lstm(ta, s)); pf.end();
            xin = hout[l];
            if (d_X1) break;
        }
        if (d_X1) {
            HIP_TRY(sdfa_launch_tap(ws + w.H0, 3, N, Nc, d_X1 + f0 * (64 * 512), s));
            continue;
        }
        // attention: proj_key over all 64 keys, Conv1d query over time steps 31..33, proj_qry
        const int at_terms = stage_terms(m, STAGE_ATTENTION);
        // bf16 attention modes (BASELINE configs[3]): the key projection never leaves the matrix core's accumulators -- one HBM-bound
        // streaming pass over the BiLSTM output computes projection + tanh + v-dot and writes one score per column (attn.hip:
        // attn_key_score_kernel); attn_kernel then does softmax + context from the scores.  The query path runs first.
        // fp32 (round 6, second half): the same pass on v_mfma_f32_16x16x4_f32 -- matrix-bound there, at the MFMA rate.  The six-product
        // mode (fp32-equivalent products) takes the exact fp32 pass too: faster than six bf16 products through a GEMM, and exact.
        const bool key_fused = g_sdfa_attn_unfused != 1;
        pf.begin("attn_proj");
        GemmArgs gk = sdfa_gemm_k4(m->kp_w, 128, ws + w.H1, Mc, ws + w.KP, Mc, 512);
        gk.terms = at_terms;
        if (!key_fused) HIP_TRY(sdfa_launch_gemm(gk, s));
        GemmArgs gc = sdfa_gemm_k4(m->qc_w, 512, ws + w.H1 + 31 * Nc * 4, Mc, ws + w.QC, Nc, 1536);   // Nc output columns read out of H1's Mc
        gc.seg_k = 512; gc.seg_col = Nc; gc.terms = at_terms;                                        // three taps: time steps 31, 32, 33
        HIP_TRY(sdfa_launch_gemm(gc, s));
        GemmArgs gq = sdfa_gemm_k4(m->qp_w, 128, ws + w.QC, Nc, ws + w.QP, Nc, 512);
        gq.terms = at_terms;
        HIP_TRY(sdfa_launch_gemm(gq, s));
        // exact fp32, large chunks: the whole layer in ONE pass over H (running softmax + context while the tile is in LDS: attn_fused_f32_kernel);
        // "attn_unfused" = 2 keeps the two-kernel form
        const bool tail_fused = key_fused && (at_terms == 0 || at_terms == 6) && g_sdfa_attn_unfused != 2 && sdfa_attn_fuses_tail(Nc, m->reserved_cus.load());
        if (key_fused) {
            AttnKeyArgs ak{};
            ak.Wk = m->kp_w; ak.H = ws + w.H1; ak.QP = ws + w.QP; ak.v = m->at_v; ak.b = m->at_b;
            ak.S = ws + w.KP;                                  // the partial scores take the first 8 Mc floats of the (unused) key-projection region
            ak.Nc = Nc; ak.Mc = Mc; ak.terms = at_terms == 6 ? 0 : at_terms; ak.reserve_cus = m->reserved_cus.load();
            if (tail_fused) {
                ak.fuse_tail = 1; ak.Zk4 = ws + w.ZK; ak.z_out = d_z ? d_z + f0 * 512 : nullptr; ak.align_out = d_align ? d_align + f0 * 64 : nullptr; ak.N = N;
            }
            HIP_TRY(sdfa_launch_attn_key_score(ak, s));
        }
        pf.end();

        AttnArgs aa{};
        aa.KP = ws + w.KP; aa.QP = ws + w.QP; aa.H = ws + w.H1; aa.v = m->at_v; aa.b = m->at_b;
        aa.Zk4 = ws + w.ZK; aa.z_out = d_z ? d_z + f0 * 512 : nullptr; aa.align_out = d_align ? d_align + f0 * 64 : nullptr;
        aa.N = N; aa.Nc = Nc; aa.Mc = Mc;
        aa.S = key_fused ? ws + w.KP : nullptr;
        pf.begin("attn"); if (!tail_fused) HIP_TRY(sdfa_launch_attn(aa, s)); pf.end();
        if (d_H) HIP_TRY(sdfa_launch_tap(ws + w.H1, 3, N, Nc, d_H + f0 * (64 * 512), s));
    }
    return SDFA_OK;
}

// The kernels / launch forms of the fp32 frequency LSTM are bit-identical and within 1-3 % of each other; for the forms with
// two resident workgroups per CU the order is a property of how the two happen to interleave:
// measure, don't guess.
int sdfa_model_autotune(sdfa_model *m, int64_t n_frames, void *d_workspace, int64_t workspace_bytes, void *stream) {
    if (!m || !m->finalized) return sdfa_fail(SDFA_ESTATE, "autotune: model not finalised");
    if (!d_workspace || n_frames <= 0 || ((uintptr_t)d_workspace & 15)) return sdfa_fail(SDFA_EINVAL, "autotune: bad argument");
    const int64_t cap = capacity(workspace_bytes, m->keep);
    if (cap < 128) return sdfa_fail(SDFA_ENOSPACE, "autotune: workspace too small");
    const int64_t Nc = round_up(std::min(cap, n_frames), 128), Mc = 64 * Nc;
    const Ws w = layout(Nc, m->keep);
    float *ws = (float *)d_workspace;
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(ws + w.X3, 0, (size_t)2048 * Mc * sizeof(float), s));      // any finite input: the kernel's time does not depend on the data
    hipEvent_t e0, e1;
    HIP_TRY(hipEventCreate(&e0));
    HIP_TRY(hipEventCreate(&e1));
    static const int forms[] = {9, 8, 5, 3};      // third kernel persistent / hardware-dispatched; second kernel persistent / hardware-dispatched (two per CU)
    float best_ms = 0.f;
    int best = m->freq_shape.load(), rc = SDFA_OK;
    for (int form : forms) {
        FreqLstmArgs fa{ws + w.X3, m->fl_w, m->fl_b, ws + w.HF, Mc, nullptr, m->fl_wb, 0, reinterpret_cast<int *>(ws + w.CT_FREQ), form, m->reserved_cus.load()};
        float ms = 0.f;
        for (int rep = 0; rep < 3 && rc == SDFA_OK; ++rep) {      // one warm launch, two timed
            if (rep == 1 && hipEventRecord(e0, s) != hipSuccess) rc = SDFA_EHIP;
            if (sdfa_launch_freq_lstm(fa, s) != hipSuccess) rc = SDFA_EHIP;
        }
        if (rc == SDFA_OK && (hipEventRecord(e1, s) != hipSuccess || hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&ms, e0, e1) != hipSuccess)) rc = SDFA_EHIP;
        if (rc != SDFA_OK) break;
        if (best_ms == 0.f || ms < best_ms) { best_ms = ms; best = form; }
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (rc != SDFA_OK) return sdfa_fail(rc, "autotune: a HIP call failed: %s", hipGetErrorString(hipGetLastError()));
    m->freq_shape.store(best);
    return best;
}

int sdfa_encoder_forward(const sdfa_model *m, const float *d_audio_feat, int64_t n_frames, float *d_z, float *d_align,
                         void *d_workspace, int64_t workspace_bytes, void *stream) {
    return encoder_impl(m, d_audio_feat, n_frames, nullptr, nullptr, 0, d_z, d_align, nullptr, d_workspace, workspace_bytes, stream);
}

// include/sdfa_attntrain.h: the frozen encoder's forward that also hands out the attention layer's memory
int sdfa_encoder_memory(const sdfa_model *m, const float *d_audio_feat, int64_t n_frames, float *d_H, float *d_z, float *d_align,
                        void *d_workspace, int64_t workspace_bytes, void *stream) {
    if (!d_H) return sdfa_fail(SDFA_EINVAL, "encoder_memory: null pointer");
    return encoder_impl(m, d_audio_feat, n_frames, nullptr, nullptr, 0, d_z, d_align, d_H, d_workspace, workspace_bytes, stream);
}

// include/sdfa_lstmtrain.h: the frozen encoder up to and including the BiLSTM's layer 0, whose output the trained layer 1 reads
int sdfa_encoder_layer0(const sdfa_model *m, const float *d_audio_feat, int64_t n_frames, float *d_X1, void *d_workspace,
                        int64_t workspace_bytes, void *stream) {
    if (!d_X1) return sdfa_fail(SDFA_EINVAL, "encoder_layer0: null pointer");
    return encoder_impl(m, d_audio_feat, n_frames, nullptr, nullptr, 0, nullptr, nullptr, nullptr, d_workspace, workspace_bytes, stream, d_X1);
}

// include/sdfa_bilstm.h: the frozen encoder up to the BiLSTM's input, the 256-feature projection of every column as rows
int sdfa_bilstm_abi_version(void) { return SDFA_BILSTM_ABI_VERSION; }

int sdfa_encoder_x0(const sdfa_model *m, const float *d_audio_feat, int64_t n_frames, float *d_X0, void *d_workspace,
                    int64_t workspace_bytes, void *stream) {
    if (!d_X0) return sdfa_fail(SDFA_EINVAL, "encoder_x0: null pointer");
    return encoder_impl(m, d_audio_feat, n_frames, nullptr, nullptr, 0, nullptr, nullptr, nullptr, d_workspace, workspace_bytes, stream, nullptr, d_X0);
}

// include/sdfa_freqtrain.h: the frozen encoder up to and including the conv stack, every column's 32 x 64 features as rows
int sdfa_encoder_conv(const sdfa_model *m, const float *d_audio_feat, int64_t n_frames, float *d_C, void *d_workspace,
                      int64_t workspace_bytes, void *stream) {
    if (!d_C) return sdfa_fail(SDFA_EINVAL, "encoder_conv: null pointer");
    return encoder_impl(m, d_audio_feat, n_frames, nullptr, nullptr, 0, nullptr, nullptr, nullptr, d_workspace, workspace_bytes, stream, nullptr, nullptr, d_C);
}

int sdfa_encoder_forward_shared(const sdfa_model *m, const float *d_audio_feat, int64_t n_frames, const int32_t *d_frame_clip,
                                const int64_t *d_frame_start, int hop, float *d_z, float *d_align, void *d_workspace,
                                int64_t workspace_bytes, void *stream) {
    if (!d_frame_clip || !d_frame_start || hop <= 0) return sdfa_fail(SDFA_EINVAL, "encoder_forward_shared: frame table missing");
    return encoder_impl(m, d_audio_feat, n_frames, d_frame_clip, d_frame_start, hop, d_z, d_align, nullptr, d_workspace, workspace_bytes, stream);
}

// ------------------------------------------------------------------------------------------------
// PCA expansion of N frames' coefficients (K4, 288 / 64 rows): out[n][o] = sum_k coef[k][n] * basis[k][o] + means[o]
// (rows = frames), stored to every destination.  PcaInversion.forward, speech_anime/modules/output_module.py:94-116
static hipError_t expand_rows(const sdfa_model *m, const float *coef, int64_t N, int64_t Nc, int64_t f0,
                              float *const *h_d_outs, int n_outs, int *queue, hipStream_t s) {
    float *d_out = h_d_outs[0];
    if (m->pca_n == 2) {
        // dgrad head: both bases in one fp32 kernel (all precision modes) so that every output line is written
        // once, whole (pca.hip)
        PcaArgs pa{};
        pa.coef = coef; pa.basis_s = m->pca_q[0]; pa.basis_r = m->pca_q[1]; pa.mean_s = m->pca_bias[0]; pa.mean_r = m->pca_bias[1];
        pa.out = d_out + f0 * m->out_dim; pa.N = N; pa.Nc = Nc; pa.out_dim = m->out_dim;
        pa.n_extra = n_outs - 1;
        pa.reserve_cus = m->reserved_cus.load();
        // SDFA_PREC_BF16X3: the expansion on split-bf16 MFMA too (round 5; "pca_fp32" = 1 keeps it exact); every other mode: fp32
        pa.basis_b = m->pca_qb; pa.terms = (g_sdfa_pca_fp32 || m->precision != SDFA_PREC_BF16X3) ? 0 : 3;
        for (int x = 1; x < n_outs; ++x) pa.out_extra[x - 1] = h_d_outs[x] + f0 * m->out_dim;
        pa.ld_s = m->pca_ld[0]; pa.ld_r = m->pca_ld[1]; pa.cols_s = m->pca_cols[0]; pa.cols_r = m->pca_cols[1];
        // default: basis slab resident in LDS, persistent work units (pca_dgrad_res_kernel); "pca_lds" option 4 = the register-
        // direct two-workgroups-per-CU form of rounds 1-2 (bit-identical, slower: the fallback that shares a CU)
        if (g_sdfa_pca_lds != 4 && queue) return sdfa_launch_pca_dgrad_res(pa, queue, s);
        return sdfa_launch_pca_dgrad(pa, s);
    }
    for (int b = 0; b < m->pca_n; ++b) {
        GemmArgs g{};
        g.P = coef + (int64_t)m->pca_k0[b] * Nc; g.Q = m->pca_q[b]; g.D = d_out + f0 * m->out_dim;
        g.bias = m->pca_bias[b]; g.bias_on_q = 1;
        g.ldp = Nc; g.ldq = m->pca_ld[b]; g.ldd = m->out_dim; g.Ppad = Nc; g.Qpad = m->pca_ld[b]; g.Pstore = N;
        g.Qreal = m->pca_cols[b]; g.K = m->pca_K[b]; g.seg_k = g.K; g.act = ACT_NONE; g.out_mode = OUT_ROW;
        g.col_group = m->pca_group[b]; g.col_stride = 9; g.col_off = m->pca_off[b];
        g.n_extra = n_outs - 1;
        for (int x = 1; x < n_outs; ++x) g.D_extra[x - 1] = h_d_outs[x] + f0 * m->out_dim;
        g.terms = stage_terms(m, STAGE_REGRESSOR);
        hipError_t e = sdfa_launch_gemm(g, s);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

int sdfa_regress_forward(const sdfa_model *m, const float *d_z, const int64_t *d_speaker_id, int64_t n_frames,
                         float *d_coef, float *d_out, void *d_workspace, int64_t workspace_bytes, void *stream) {
    float *one[1] = {d_out};
    return sdfa_regress_forward_multi(m, d_z, d_speaker_id, n_frames, d_coef, one, d_out ? 1 : 0, d_workspace, workspace_bytes, stream);
}

int sdfa_regress_forward_multi(const sdfa_model *m, const float *d_z, const int64_t *d_speaker_id, int64_t n_frames,
                               float *d_coef, float *const *h_d_outs, int n_outs, void *d_workspace, int64_t workspace_bytes,
                               void *stream) {
    if (!m || !m->finalized) return sdfa_fail(SDFA_ESTATE, "regress_forward: model not finalised");
    if (n_outs < 0 || n_outs > SDFA_MAX_DESTS || (n_outs && !h_d_outs)) return sdfa_fail(SDFA_EINVAL, "regress_forward: 0..%d output destinations", SDFA_MAX_DESTS);
    for (int i = 0; i < n_outs; ++i) {
        if (!h_d_outs[i]) return sdfa_fail(SDFA_EINVAL, "regress_forward: output destination %d is null", i);
        if (m->head == SDFA_HEAD_DGRAD && ((uintptr_t)h_d_outs[i] & 15)) return sdfa_fail(SDFA_EINVAL, "regress_forward: d_out must be 16-byte aligned for the dgrad head");
        if ((uintptr_t)h_d_outs[i] & 3) return sdfa_fail(SDFA_EINVAL, "regress_forward: output pointers must be 4-byte aligned");
    }
    float *d_out = n_outs ? h_d_outs[0] : nullptr;
    if (n_frames == 0) return SDFA_OK;
    if (!d_z || !d_speaker_id || !d_workspace || n_frames < 0) return sdfa_fail(SDFA_EINVAL, "regress_forward: bad argument");
    if (((uintptr_t)d_workspace | (uintptr_t)d_z) & 15) return sdfa_fail(SDFA_EINVAL, "regress_forward: pointers must be 16-byte aligned");
    // the fused dgrad expansion writes whole rows with 16-byte stores (pca.hip); rows are 359,136 B apart, so the base decides
    if (m->head == SDFA_HEAD_DGRAD && d_out && ((uintptr_t)d_out & 15)) return sdfa_fail(SDFA_EINVAL, "regress_forward: d_out must be 16-byte aligned for the dgrad head");
    if (((uintptr_t)d_out | (uintptr_t)d_coef) & 3) return sdfa_fail(SDFA_EINVAL, "regress_forward: output pointers must be 4-byte aligned");
    const int64_t cap = capacity(workspace_bytes, m->keep);
    if (cap < 128) return sdfa_fail(SDFA_ENOSPACE, "regress_forward: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    Prof pf{m, s};
    float *ws = (float *)d_workspace;
    auto fcg = [m](const sdfa_model::Fc &fc, const float *Q, int64_t ldq, float *D, int64_t Nc, const int64_t *spk, int64_t nreal) {
        GemmArgs g = gemm_fc(fc, Q, ldq, D, Nc, spk, nreal);
        g.terms = stage_terms(m, STAGE_REGRESSOR);
        return g;
    };
    for (int64_t f0 = 0; f0 < n_frames; f0 += cap) {
        const int64_t N = std::min(cap, n_frames - f0);
        const int64_t Nc = round_up(N, 128);
        const Ws w = layout(Nc, m->keep);
        float *zk = ws + w.ZK, *trunk = ws + w.TRUNK, *a0 = ws + w.A0, *a1 = ws + w.A1, *coef = ws + w.COEF;
        const int64_t *spk = d_speaker_id + f0;
        pf.begin("mlp");
        HIP_TRY(sdfa_launch_rows_to_k4(d_z + f0 * 512, N, 512, zk, Nc, s));
        if (m->head == SDFA_HEAD_DGRAD) {
            HIP_TRY(sdfa_launch_gemm(fcg(m->trunk, zk, Nc, trunk, Nc, spk, N), s));
            for (int b = 0; b < 2; ++b) {
                HIP_TRY(sdfa_launch_gemm(fcg(m->br[b][0], trunk, Nc, a0, Nc, spk, N), s));
                HIP_TRY(sdfa_launch_gemm(fcg(m->br[b][1], a0, Nc, a1, Nc, spk, N), s));
                HIP_TRY(sdfa_launch_gemm(fcg(m->br[b][2], a1, Nc, coef + (b ? 96 * Nc : 0), Nc, spk, N), s));
            }
            if (d_coef) {
                HIP_TRY(sdfa_launch_k4_to_rows(coef, Nc, N, 288, 0, SDFA_COEF_SCALE, d_coef + f0 * m->coef_dim, m->coef_dim, s));
                HIP_TRY(sdfa_launch_k4_to_rows(coef, Nc, N, 288, 96, SDFA_COEF_ROTAT, d_coef + f0 * m->coef_dim + SDFA_COEF_SCALE, m->coef_dim, s));
            }
        } else {
            HIP_TRY(sdfa_launch_gemm(fcg(m->off[0], zk, Nc, a0, Nc, spk, N), s));
            HIP_TRY(sdfa_launch_gemm(fcg(m->off[1], a0, Nc, a1, Nc, spk, N), s));
            HIP_TRY(sdfa_launch_gemm(fcg(m->off[2], a1, Nc, coef, Nc, spk, N), s));
            if (d_coef) HIP_TRY(sdfa_launch_k4_to_rows(coef, Nc, N, 64, 0, SDFA_COEF_OFFSETS, d_coef + f0 * m->coef_dim, m->coef_dim, s));
        }
        pf.end();
        if (d_out) {
            pf.begin("pca");
            HIP_TRY(expand_rows(m, coef, N, Nc, f0, h_d_outs, n_outs, reinterpret_cast<int *>(ws + w.CT_PCA), s));
            pf.end();
        }
    }
    return SDFA_OK;
}

int sdfa_expand_coef(const sdfa_model *m, const float *d_coef, int64_t n_frames, float *d_out, void *d_workspace,
                     int64_t workspace_bytes, void *stream) {
    if (!m || !m->finalized) return sdfa_fail(SDFA_ESTATE, "expand_coef: model not finalised");
    if (n_frames == 0) return SDFA_OK;
    if (!d_coef || !d_out || !d_workspace || n_frames < 0) return sdfa_fail(SDFA_EINVAL, "expand_coef: bad argument");
    if ((uintptr_t)d_workspace & 15) return sdfa_fail(SDFA_EINVAL, "expand_coef: d_workspace must be 16-byte aligned");
    if (m->head == SDFA_HEAD_DGRAD && ((uintptr_t)d_out & 15)) return sdfa_fail(SDFA_EINVAL, "expand_coef: d_out must be 16-byte aligned for the dgrad head");
    if (((uintptr_t)d_out | (uintptr_t)d_coef) & 3) return sdfa_fail(SDFA_EINVAL, "expand_coef: pointers must be 4-byte aligned");
    const int64_t cap = capacity(workspace_bytes, m->keep);
    if (cap < 128) return sdfa_fail(SDFA_ENOSPACE, "expand_coef: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    Prof pf{m, s};
    float *ws = (float *)d_workspace;
    for (int64_t f0 = 0; f0 < n_frames; f0 += cap) {
        const int64_t N = std::min(cap, n_frames - f0);
        const int64_t Nc = round_up(N, 128);
        const Ws w = layout(Nc, m->keep);
        float *coef = ws + w.COEF;                           // the regressor's coefficient slab
        const float *src = d_coef + f0 * m->coef_dim;
        pf.begin("pca");
        if (m->head == SDFA_HEAD_DGRAD) {
            HIP_TRY(sdfa_launch_rows_seg_to_k4(src, m->coef_dim, N, 0, SDFA_COEF_SCALE, coef, Nc, 0, 96, s));
            HIP_TRY(sdfa_launch_rows_seg_to_k4(src, m->coef_dim, N, SDFA_COEF_SCALE, SDFA_COEF_ROTAT, coef, Nc, 96, 192, s));
        } else {
            HIP_TRY(sdfa_launch_rows_seg_to_k4(src, m->coef_dim, N, 0, SDFA_COEF_OFFSETS, coef, Nc, 0, 64, s));
        }
        float *outs[1] = {d_out};
        HIP_TRY(expand_rows(m, coef, N, Nc, f0, outs, 1, reinterpret_cast<int *>(ws + w.CT_PCA), s));
        pf.end();
    }
    return SDFA_OK;
}

// ------------------------------------------------------------------------------------------------
int64_t sdfa_debug_distinct_columns(const sdfa_model *m, int64_t n_frames, const void *d_workspace, void *stream) {
    if (!m || n_frames <= 0 || !d_workspace) return sdfa_fail(SDFA_EINVAL, "debug_distinct_columns: bad argument");
    const Ws w = layout(round_up(n_frames, 128), m->keep);
    int64_t counts[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(counts, (const float *)d_workspace + w.SH, sizeof counts, hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return counts[0];
}

// ---- workspace status block -----------------------------------------------------------------------------------------------
int sdfa_workspace_init(void *d_workspace, int64_t workspace_bytes, void *stream) {
    if (!d_workspace || workspace_bytes < SDFA_WS_STATUS_BYTES || ((uintptr_t)d_workspace & 15)) return sdfa_fail(SDFA_EINVAL, "workspace_init: bad argument");
    HIP_TRY(hipMemsetAsync(d_workspace, 0, SDFA_WS_STATUS_BYTES, (hipStream_t)stream));
    return SDFA_OK;
}

int sdfa_workspace_status_async(const void *d_workspace, uint32_t *h_status, void *stream) {
    if (!d_workspace || !h_status) return sdfa_fail(SDFA_EINVAL, "workspace_status_async: bad argument");
    HIP_TRY(hipMemcpyAsync(h_status, d_workspace, SDFA_WS_STATUS_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, (hipStream_t)stream));
    return SDFA_OK;
}

int64_t sdfa_workspace_status(const void *d_workspace, int word, void *stream) {
    if (!d_workspace || word < 0 || word >= SDFA_WS_STATUS_WORDS) return sdfa_fail(SDFA_EINVAL, "workspace_status: bad argument");
    uint32_t v = 0;
    HIP_TRY(hipMemcpyAsync(&v, reinterpret_cast<const uint32_t *>(d_workspace) + word, sizeof v, hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return (int64_t)v;
}

int sdfa_debug_tap(const sdfa_model *m, int what, int64_t n_frames, float *d_dst, const void *d_workspace, void *stream) {
    if (!m || !m->keep) return sdfa_fail(SDFA_ESTATE, "debug_tap needs sdfa_debug_keep_intermediates(model, 1) before the forward");
    if (what < 0 || what > 3 || n_frames <= 0 || !d_dst || !d_workspace) return sdfa_fail(SDFA_EINVAL, "debug_tap: bad argument");
    const int64_t Nc = round_up(n_frames, 128);
    const Ws w = layout(Nc, true);
    const float *ws = (const float *)d_workspace;
    const float *src = what == 0 ? ws + w.P1 : what == 1 ? ws + w.X3 : what == 2 ? ws + w.Z : ws + w.H1;
    HIP_TRY(sdfa_launch_tap(src, what, n_frames, Nc, d_dst, (hipStream_t)stream));
    return SDFA_OK;
}

}  // extern "C"
