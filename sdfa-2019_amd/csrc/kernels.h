// Internal launcher interface between the api_*.cpp files (host orchestration) and the .hip kernel files.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

enum { ACT_NONE = 0, ACT_LRELU = 1, ACT_TANH = 2 };

// Frequency-LSTM hidden states are stored tile-major: float4[column block of 128][HF_SLAB_ROWS][128], 8192/4 = 2048 rows
// per slab with no padding, so the slab stride (4 MiB) is a power of two.  Padding it off a power of two, so that the
// projection GEMM's workgroups would not all stream the same HBM channels at once, measured no difference
// (profiles/HISTORY.md, layout experiments on the hidden states).
constexpr int HF_SLAB_ROWS = 2048;
enum { OUT_K4 = 0, OUT_ROW = 1 };
constexpr int SDFA_MAX_DESTS = 8;   // output destinations of the regressor epilogues: the local buffer + up to 7 peers

struct GemmArgs {
    const float *P;      // K4 [K/4][ldp]
    const float *Q;      // K4 [K/4][ldq] (per segment)
    float *D;
    const float *bias;   // over p (K4 features) or over q (OUT_ROW)
    const float *cond_w; // K4-ish [Ppad/4][8][4]: column of the FC weight that the one-hot speaker selects
    const int64_t *cond_idx;  // [Qreal] speaker ids
    int64_t ldp, ldq, ldd;
    int64_t Ppad, Qpad;  // multiples of 128: tiles launched
    int64_t Pstore;      // rows actually stored (multiple of 4)
    int64_t Qreal;       // columns that exist (OUT_ROW store mask / bias_q / cond bounds)
    int K;               // total contraction length, multiple of 32
    int seg_k;           // contraction length per segment (= K when one segment)
    int64_t seg_col;     // Q column offset between segments
    int act, out_mode, bias_on_q;
    int terms;                // 0 = fp32 MFMA; 1 = operands rounded to bf16; 3 = split-bf16, three bf16 MFMAs per product
    int q_tile_major;         // Q is stored tile-major: float4[column block of 128][q_slab_rows >= K/4][128] (the freq-LSTM hidden states)
    int q_slab_rows;
    const int64_t *q_limit;   // device scalar: tiles whose first column is >= *q_limit exit at once (null = no limit)
    int col_group, col_stride, col_off;   // OUT_ROW only: column q is stored at (q / group) * stride + off + q % group (group 0 = identity)
    float *D_extra[SDFA_MAX_DESTS - 1];   // OUT_ROW only: further destinations with D's layout (see PcaArgs::out_extra)
    int n_extra;
    int reserve_cus;          // persistent kernel (gemm_fat_kernel): launch (CUs - reserve_cus) workgroups
};
hipError_t sdfa_launch_gemm(const GemmArgs &a, hipStream_t s);
// The plain product: K4 P [K/4][rows] x K4 Q [K/4][ldq] -> K4 D [rows][cols], one segment, every row and column stored, no bias, no
// activation, fp32.  Call sites set what differs from that (terms, reserve_cus, segments, a bias, ...) on the result.
inline GemmArgs sdfa_gemm_k4(const float *P, int64_t rows, const float *Q, int64_t ldq, float *D, int64_t cols, int K) {
    GemmArgs g{};
    g.P = P; g.Q = Q; g.D = D;
    g.ldp = rows; g.Ppad = rows; g.Pstore = rows;
    g.ldq = ldq; g.ldd = cols; g.Qpad = cols; g.Qreal = cols;
    g.K = K; g.seg_k = K; g.act = ACT_NONE; g.out_mode = OUT_K4;
    return g;
}

// ---- PCA expansion of the dgrad head, both bases fused (pca.hip) ---------------------------------
struct PcaArgs {
    const float *coef;               // K4 [288/4][Nc]: rows 0..95 scale coefficients (85 real), 96..287 rotat (180 real)
    const float *basis_s, *basis_r;  // K4 [96/4][ld_s], [192/4][ld_r]
    const float *mean_s, *mean_r;    // [cols_s], [cols_r]
    float *out;                      // [N][out_dim] row-major, triangle-interleaved [s0..s5 r0 r1 r2]
    int64_t N, Nc, out_dim, ld_s, ld_r, cols_s, cols_r;
    // one-shot direct all-gather: the same rows are ALSO stored to n_extra more base pointers --
    // this rank's slot in each peer GPU's gathered buffer, mapped over xGMI (or other buffers on this device)
    float *out_extra[SDFA_MAX_DESTS - 1];
    int n_extra;
    int reserve_cus;                 // pca_dgrad_res_kernel: launch (CUs - reserve_cus) workgroups
    // split-bf16 form of pca_dgrad_res_kernel (terms == 3): both bases as bf16 octets, per triangle block
    // [plane hi | lo][scale rows 2 ks + h (12) x 192 columns | rotat rows (24) x 96] (api_model.cpp: pack_pca_bf16); null / other terms = fp32
    const void *basis_b;
    int terms;
};
hipError_t sdfa_launch_pca_dgrad(const PcaArgs &a, hipStream_t s);
hipError_t sdfa_launch_pca_dgrad_res(const PcaArgs &a, int *queue, hipStream_t s);   // basis slab resident in LDS, persistent; queue: one int of workspace

// ---- front end -----------------------------------------------------------------------------
struct FrontendConsts {      // device pointers, built once per sample rate
    const float *hamm;       // [win]
    const float2 *twiddle;   // [win]  exp(-2*pi*i*m/win)
    const int *mel_bin0;     // [128]     first FFT bin of each mel band (the bins of a band are consecutive)
    const float *mel_w8;     // [8][128]  its weights, tap-major, zero padded to 8 taps
    int win, hop, sliding, nbins_used, nnz;
};
hipError_t sdfa_launch_frontend(const FrontendConsts &c, const float *pcm, const int64_t *clip_off,
                                const int64_t *clip_len, const int32_t *frame_clip, const int64_t *frame_start,
                                int64_t n_frames, float *audio_feat, hipStream_t s);
// augmented training windows (include/sdfa_augment.h): one workgroup per descriptor; noise / scale may be null
struct sdfa_augment_desc;
hipError_t sdfa_launch_augment(const FrontendConsts &c, const float *pcm, const int64_t *clip_off, const int64_t *clip_len, int n_clips,
                               const sdfa_augment_desc *desc, int64_t n, const float *noise, int64_t noise_stride, const float *scale,
                               float *audio_feat, hipStream_t s);
// the constants of `sample_rate` on the current device (api_frontend.cpp: built on first use, then cached)
int sdfa_frontend_consts(int sample_rate, FrontendConsts &c);
// "spectral gather" form: mel columns of the DISTINCT STFT columns (col_src / n_distinct from the share map with
// t in 1..63), then one gather + delta + store pass per frame
hipError_t sdfa_launch_mel_columns(const FrontendConsts &c, const float *pcm, const int64_t *clip_off, const int64_t *clip_len,
                                   const int32_t *frame_clip, const int64_t *frame_start, const int32_t *col_src,
                                   const int64_t *n_distinct, float *mel_table, hipStream_t s);
hipError_t sdfa_launch_mel_stream(const FrontendConsts &c, const float *pcm, const int64_t *clip_off, const int64_t *clip_len,
                                  const int32_t *frame_clip, const int64_t *frame_start, const int32_t *prev, const int32_t *shift,
                                  int64_t n_frames, int block, int slots, int producer_consumer, int spin_max, int *status, float *audio_feat, hipStream_t s);
// live streams (include/sdfa_stream.h): the spectral stream over views of per-stream rings of 2^r samples, and the ring append
hipError_t sdfa_launch_mel_ring(const FrontendConsts &c, const float *rings, int r, int n_rings, const int64_t *view_ring, const int64_t *view_hi,
                                const int32_t *frame_view, const int64_t *frame_start, const int32_t *prev, const int32_t *shift, int64_t n_frames,
                                int block, int slots, int producer_consumer, int spin_max, int *status, float *audio_feat, hipStream_t s);
hipError_t sdfa_launch_ring_append(float *rings, int r, int n_rings, const int64_t *seg, int n_seg, const float *src, int64_t n_src, hipStream_t s);
hipError_t sdfa_launch_gather_features(const float *mel_table, const int32_t *col_to_u, int64_t n_frames, int64_t Nc, int frame_major,
                                       float *audio_feat, hipStream_t s);   // frame_major: col_to_u is [n][t] (ShareArgs::frame_major)

// ---- conv stack ----------------------------------------------------------------------------
struct ConvArgs {
    const float *audio_feat;  // [N][64][128][3]
    int64_t N, Nc, Mc;        // real frames, padded frames per chunk, columns = 64*Nc
    // conv1: packed A operand [5 k-steps][2 halves][32 co] (k = df*3 + c, k = 9 -> 0), epilogue constants
    const float *w1, *b1, *s1, *t1;   // bias, BN scale, BN shift per co
    float *P1;                // K4 [2048/4][Mc]   rows f1*32 + co
    // conv2 / conv3: K4 weights [K/4][64][4]
    const float *w2, *b2, *s2, *t2;   // K = 96  (k = df*32 + ci)
    const float *w3, *b3, *s3, *t3;   // K = 64
    float *X3;                // K4 [2048/4][Mc]   rows f*64 + ch
    // column sharing: column m reads audio_feat row col_src[m] (-1 = zeros) instead of (m % Nc)*64 + m / Nc, and
    // workgroups whose first column is >= *col_limit exit at once.  Both null = every column of every frame.
    const int32_t *col_src;
    const int64_t *col_limit;
    // mixed-precision modes (sdfa_launch_conv123 only): bf16 planes [hi | mid | lo] of the three layers' weights in the K order of
    // conv123_bf16_kernel (api_model.cpp: pack_conv_bf16); terms 0 = fp32 MFMA, 1 / 3 / 6 as in FreqLstmArgs
    const void *wb;
    int terms;
};
hipError_t sdfa_launch_conv1(const ConvArgs &a, hipStream_t s);
hipError_t sdfa_launch_conv23(const ConvArgs &a, hipStream_t s);
hipError_t sdfa_launch_conv123(const ConvArgs &a, hipStream_t s);   // conv1_pool + conv23 fused (P1 is not written)

// ---- LSTM recurrences ----------------------------------------------------------------------
struct FreqLstmArgs {
    const float *X3;     // K4 [2048/4][Mc]
    const float *W;      // per direction: K4 [(64+128)/4][512][4], gate rows packed per wave
    const float *bias;   // per direction: [512] packed (b_ih + b_hh)
    float *HF;           // K4 [8192/4][Mc]  rows f*256 + dir*128 + j
    int64_t Mc;
    const int64_t *col_limit;   // see ConvArgs
    const void *Wb;      // mixed-precision modes: per direction bf16x8 [hi | lo][24 octets][512 rows] (lstm.hip)
    int terms;           // 0 = fp32 MFMA; 1 = bf16 MFMA; 3 = split-bf16 (hi/lo) MFMA
    int *tile_counter;   // one int of workspace: the persistent form's work queue head (zeroed by the launcher)
    int shape;           // fp32 kernel / launch form (all bit-identical): freq_lstm_v3_kernel 9 = persistent (tile queue), one workgroup per CU by
                         // design (default), 8 = one hardware-dispatched workgroup per tile; freq_lstm_v2_kernel 5 = persistent, two per CU,
                         // 3 = hardware-dispatched, two per CU (the fallback that shares a CU); anything else = 9
    int reserve_cus;     // persistent forms: launch (CUs - reserve_cus) workgroups (sdfa_model_set_reserved_cus)
};
hipError_t sdfa_launch_freq_lstm(const FreqLstmArgs &a, hipStream_t s);

struct TimeLstmArgs {
    const float *GX;     // K4 [2048/4][Mc]  rows dir*1024 + packed gate row  (input projections)
    const float *W;      // per direction: K4 [256/4][1024][4]
    float *H;            // K4 [512/4][Mc]   rows dir*256 + j
    int64_t Nc, Mc;
    const void *Wb;      // mixed-precision modes: per direction bf16x8 [hi | lo][32 octets][1024 rows] (lstm.hip)
    int terms;           // 0 = fp32 MFMA; 1 = bf16; 3 = split-bf16
    unsigned *flags;     // small-batch form (time_lstm_split_kernel): [0] this launch's time-out word, [4 ..] one flag per workgroup; null = never split
    int64_t flag_words;  // words available at `flags`
    const float *W16;    // time_lstm_split16_kernel: per direction float4 [16 K16][4 g][1024 rows] (api_model.cpp pack_rec_16x16x4); null = not packed
    unsigned *status;    // word 0 of the workspace's status block: counts the waits of the small-batch form that expired (null = not counted)
    int reserve_cus;     // the small-batch form is used while its grid fits (CUs - reserve_cus)
    const int32_t *col_map;   // column sharing, layer 0: GX holds the DISTINCT columns; column (t, n) reads GX column col_map[t * Nc + n] (null = its own)
    const float *X = nullptr;    // time_lstm_fused_kernel (layer 1): the layer's input, K4 [512/4][Mc]; null = the projection comes from GX
    const float *Wxh = nullptr;  // time_lstm_fused_kernel: per direction K4 [(512+256)/4][1024][4], W_ih then W_hh (api_model.cpp); null = not packed
};
hipError_t sdfa_launch_time_lstm(const TimeLstmArgs &a, hipStream_t s);
// 0 = the launch reads its input projection from GX (the caller runs the projection GEMM first); 1 / 2 = it contracts X itself, 32- / 64-frame tiles
int sdfa_time_lstm_fuses_x(const TimeLstmArgs &a);

// ---- attention scores / softmax / context ---------------------------------------------------
struct AttnArgs {
    const float *KP;     // K4 [128/4][Mc]  key projections
    const float *QP;     // K4 [128/4][Nc]  query projection
    const float *H;      // K4 [512/4][Mc]  values (BiLSTM output)
    const float *v;      // [128]
    const float *b;      // [128]
    float *Zk4;          // K4 [512/4][Nc]  context (feeds the output MLPs)
    float *z_out;        // [N][512] row-major (may be null)
    float *align_out;    // [N][64]  row-major (may be null)
    int64_t N, Nc, Mc;
    const float *S;      // [Mc][8] partial scores written by attn_key_score_kernel (then KP / QP / v / b are not read); null = computed here from KP
};
hipError_t sdfa_launch_attn(const AttnArgs &a, hipStream_t s);

// bf16 attention modes: key projection + scores in one streaming pass over H (attn.hip: attn_key_score_kernel)
struct AttnKeyArgs {
    const float *Wk;     // K4 [512/4][128]  proj_key weights, as the GEMM takes them
    const float *H;      // K4 [512/4][Mc]   BiLSTM output
    const float *QP;     // K4 [128/4][Nc]   query projection
    const float *v, *b;  // [128]
    float *S;            // out [Mc][8]  partial score (outputs 16w .. 16w+15) of column m = t * Nc + n per wave w
    int64_t Nc, Mc;
    int terms;           // 0 = exact fp32 (v_mfma_f32_16x16x4_f32), 1 = bf16 operands, 3 = split-bf16
    int reserve_cus;
    int ts_shift;        // set by the launcher: a work unit is 16 frames x (64 >> ts_shift) time steps
    // terms == 0 and fuse_tail: the whole attention layer in this launch (attn_fused_f32_kernel: running softmax + context while the tile
    // is in LDS); S is not written, sdfa_launch_attn is not needed.  Outputs as AttnArgs.
    int fuse_tail;
    float *Zk4, *z_out, *align_out;
    int64_t N;
};
// true when sdfa_launch_attn_key_score would take the one-launch form for this size (enough 16-frame units to give every CU two)
bool sdfa_attn_fuses_tail(int64_t Nc, int reserve_cus);
hipError_t sdfa_launch_attn_key_score(const AttnKeyArgs &a, hipStream_t s);

// ---- layout helpers --------------------------------------------------------------------------
// row-major [n][F] (n < N) -> K4 [F/4][ld]  (zero for n >= N), and back
hipError_t sdfa_launch_rows_to_k4(const float *src, int64_t N, int F, float *dst, int64_t ld, hipStream_t s);
hipError_t sdfa_launch_rows_seg_to_k4(const float *src, int64_t src_ld, int64_t N, int c0, int nf, float *dst, int64_t ld,
                                      int f0, int nf_pad, hipStream_t s);
hipError_t sdfa_launch_k4_to_rows(const float *src, int64_t ld, int64_t N, int F, int f0, int nf, float *dst,
                                  int64_t dst_ld, hipStream_t s);
// debug taps (tests): K4 [F/4][Mc] with m = t*Nc+n  ->  reference layouts
hipError_t sdfa_launch_tap(const float *src, int what, int64_t N, int64_t Nc, float *dst, hipStream_t s);

// ---- column sharing (share.hip) -----------------------------------------------------------------
struct ShareArgs {
    const int32_t *frame_clip;   // [N] clip id of each frame of the chunk
    const int64_t *frame_start;  // [N] window start sample inside its clip
    int hop;
    int t_lo, t_hi;              // window columns t_lo..t_hi are shareable between hop-aligned frames of a clip
    int frame_major;             // index order of owner / flag / uid / col_to_u AND numbering order of the distinct columns: 0 = time-step-major
                                 // (i = t * Nc + n), 1 = frame-major (i = n * 64 + t)
    int64_t N, Nc, Mc;
    int32_t *prev, *shift;       // [Nc]
    int32_t *owner, *flag, *uid; // [Mc]
    int32_t *tile_sum;           // [Mc/1024 + 1] scan scratch
    int32_t *col_src;            // [Mc] out: audio_feat row of each distinct column (-1 padding)
    int32_t *col_to_u;           // [Mc] out: distinct-column index of every column, in the index order above
    int64_t *counts;             // [3]  out: [0] number of distinct columns; [1] that rounded up to 256 (the column limit of every stage);
                                 // [2] q_full, where the persistent projection GEMM stops and sdfa_launch_gemm_tail starts (fat_grid)
    // sdfa_launch_share_map_content only (no frame table: the owners come from the features themselves; prev / shift unused)
    const float *feat;           // [N * 64][384] the chunk's audio_feat, one row per column
    uint64_t *hash;              // [N * 64] scratch: 64-bit hash of each column's bit pattern, frame-major
    uint64_t *group_key;         // [group_slots] scratch: open-addressing table of the chunk's hashes, stored complemented (all ones = empty slot)
    uint32_t *group_first;       // [group_slots] scratch: smallest column index (index order above) among the columns with the slot's hash
    int64_t group_slots;         // sdfa_share_group_slots(N)
    int hash_bits;               // "share_hash_bits": 0 = the whole hash, 1..32 = only that many low bits of it (tests: forces collisions)
    // numbering (both fronts)
    int fat_grid;                // workgroups G of the persistent projection GEMM behind this map: counts[2] = the whole rounds of G 256-column tiles
                                 // when the tail rule (tail_mode 0; 2 = always) hands the rest to sdfa_launch_gemm_tail, else counts[2] = counts[1].  0 = no split
    int tail_mode;
};
// All of a map's tables live in one int32 region: [counts: 16 words | prev | shift | owner | flag | uid | col_src | col_to_u | tile_sum].
// (counts takes the first six of its 16 words; the front end keeps its stream kernel's status in word 8.)
// sdfa_share_table_words is what that takes (tile_sum: one word per 1024 columns, share.hip: launch_share_numbering, and one to spare); a workspace
// layout reserves at least that much, sdfa_share_carve (N / Nc / Mc set before) points the arguments into it.
inline int64_t sdfa_share_table_words(int64_t Nc) { return 16 + 2 * Nc + 5 * (64 * Nc) + (64 * Nc) / 1024 + 1; }
// Slots of the content front's hash table: a power of two, at least twice the chunk's real columns (so a probe sequence always ends).  The
// front's scratch is hash | group_key | group_first = 2 * 64 N + 3 * slots words, less than 14 Mc.
inline int64_t sdfa_share_group_slots(int64_t N) { int64_t s = 1024; while (s < 2 * 64 * N) s <<= 1; return s; }
inline void sdfa_share_carve(ShareArgs &a, int32_t *base) {
    a.counts = reinterpret_cast<int64_t *>(base);
    a.prev = base + 16; a.shift = a.prev + a.Nc;
    a.owner = a.shift + a.Nc; a.flag = a.owner + a.Mc; a.uid = a.flag + a.Mc;
    a.col_src = a.uid + a.Mc; a.col_to_u = a.col_src + a.Mc; a.tile_sum = a.col_to_u + a.Mc;
}
hipError_t sdfa_launch_share_map(const ShareArgs &a, hipStream_t s);
hipError_t sdfa_launch_share_map_content(const ShareArgs &a, hipStream_t s);   // the same map, built from the contents of audio_feat (t_lo / t_hi / frame_clip / frame_start / hop unused)
hipError_t sdfa_launch_share_prev(const ShareArgs &a, hipStream_t s);     // prev / shift only (the spectral-stream front end reads the chains from them)
hipError_t sdfa_launch_expand_cols(const float *Zu, const int32_t *col_to_u, float *Z, int nquads, int64_t Mc, hipStream_t s);
// the expanded frequency projection Z, K4 [64][Mc] with m = t*Nc+n  ->  rows [N][64 t][256] (sdfa_encoder_x0); Z and dst 16-byte aligned
hipError_t sdfa_launch_x0_rows(const float *Z, int64_t N, int64_t Nc, float *dst, hipStream_t s);
// the conv stack's output X3, K4 [512][Mc] with m = t*Nc+n (or the distinct column col_to_u[m])  ->  rows [N][64 t][32 f][64 ch] (sdfa_encoder_conv)
hipError_t sdfa_launch_conv_rows(const float *X3, const int32_t *col_to_u, int64_t N, int64_t Nc, float *dst, hipStream_t s);

// Tail of the shared-column frequency projection (gemm_tail.hip): columns [*q_lo, *q_hi) -- device scalars, multiples of 256 -- of
//   D[p][q] = sum_k P[k][p] * Q[k][q] + bias[p]      fp32, K4 output, 256 rows, Q in the tile-major hidden-state layout, K = 8192,
// in 64 x 64 blocks, bit for bit what gemm_fat_kernel stores for them.  The grid covers max_tiles 256-column tiles; workgroups past *q_hi exit.
struct GemmTailArgs {
    const float *P, *Q, *bias;
    float *D;
    int64_t ldd;
    int q_slab_rows;
    const int64_t *q_lo, *q_hi;
    int max_tiles;
};
hipError_t sdfa_launch_gemm_tail(const GemmTailArgs &a, hipStream_t s);
// workgroups of gemm_fat_kernel for a K4 product of `rows` x `cols` (gemm.hip: launch_fat)
inline int64_t sdfa_fat_grid(int64_t rows, int64_t cols, int cus, int reserve_cus) {
    const int64_t ntiles = (rows / 256) * (cols / 256), wgs = cus - reserve_cus > 1 ? cus - reserve_cus : 1;
    return ntiles < wgs ? ntiles : wgs;
}

// ---- dgrad -> mesh (mesh.hip) -----------------------------------------------------------------------
struct MeshArgs {
    const float *dgrad;        // [rows][n_src_tris][9]
    int64_t n_frames;          // output frames (= rows without a seek plan, = queries with one)
    int n_tris, n_verts, n_free, free_pad;
    int n_src_tris;            // triangles per dgrad row (= n_tris without triangle correspondences)
    const int64_t *seek_src;   // [n_frames][2] dgrad rows blended into each output frame (null: frame f is row f)
    const float *seek_w;       // [n_frames][2] their float32 weights
    const float *reg_xt;       // [n_free][3] reg * template position of each free vertex
    const int *inc_ptr;        // [n_free + 1] CSR over free vertices
    const int *inc_tri;        // [nnz] SOURCE triangle of each incidence
    const float *inc_coef;     // [nnz][3] the A entries of that (triangle, vertex) pair
    const int *vert_col;       // [n_verts] free-vertex row or -1
    const float *tmpl;         // [n_verts][3] template positions
    float *rhs;                // K4 [free_pad/4][ld]   ld = columns = 3 * frames padded to 128
    const float *sol;          // K4 [free_pad/4][ld]   Inv * rhs
    float *verts;              // out [n_frames][n_verts][3]
    int64_t ld;
};
hipError_t sdfa_launch_mesh_rhs(const MeshArgs &a, hipStream_t s);
hipError_t sdfa_launch_mesh_scatter(const MeshArgs &a, hipStream_t s);
// saber.stream.seek on the device (mesh.hip): plan = (src rows, float32 weights) per query; rows = the blended rows
hipError_t sdfa_launch_seek_plan(const int32_t *tslist, const int64_t *frame_off, const int64_t *query_off, int n_clips, double fps,
                                 int64_t n_queries, int64_t *src, float *w, hipStream_t s);
hipError_t sdfa_launch_seek_rows(const float *rows, int64_t width, const int64_t *src, const float *w, int64_t nq, float *out, hipStream_t s);
// mesh -> dgrad (dgrad.hip): deformation gradients of per-frame target meshes against one source mesh, one thread per (frame, triangle)
struct DgradArgs {
    const float *src;          // [n_verts][3] source vertices
    const float *target;       // [n_frames][n_verts][3] target vertices, or offsets added to src (target_is_offsets)
    const uint32_t *faces;     // [n_tris][3]
    const uint8_t *mask;       // [n_tris] nonzero = 9 exact zeros (null: none)
    int64_t n_frames;
    int n_tris, n_verts, target_is_offsets;
    double eps;
    float *out32;              // [n_frames][n_tris * 9] when out64 is null
    double *out64;             // [n_frames][n_tris * 9]
};
hipError_t sdfa_launch_deform_grad(const DgradArgs &a, hipStream_t s);
// test-time ensembling: out = (a + b) / 2, element-wise, float32 roundings of numpy's `sum += x; sum / 2.0` (vector path for 16-byte aligned pointers)
hipError_t sdfa_launch_ensemble_mean(const float *a, const float *b, int64_t n, float *out, hipStream_t s);

// ---- audio ingest: kaiser_best resampling (resample.hip) --------------------------------------------------------
struct ResampleArgs {
    const float *x;            // [n_in] input samples
    int64_t n_in;
    float *y;                  // [n_out]
    int64_t n_res, n_out;      // int(n_in * ratio) filtered samples, then zeros up to n_out = ceil(n_in * ratio)
    const double *win, *delta; // [nwin] half filter (scaled by the ratio when downsampling) and its forward differences
    const double *treg;        // [n_res] time register of every output sample
    int64_t nwin, step;        // table length, table entries per input sample = int(min(1, ratio) * num_table)
    double scale;              // min(1, ratio)
    int num_table;             // table entries per zero crossing (512)
};
hipError_t sdfa_launch_resample(const ResampleArgs &a, hipStream_t s);
// live streams (include/sdfa_stream.h sdfa_stream_resample): input rings -> model rings, all streams of a step in one launch
constexpr int STREAM_RING_MIRROR = 2048;   // include/sdfa_stream.h SDFA_STREAM_RING_MIRROR
constexpr int STREAM_MAX_RATES = 8;        // include/sdfa_stream.h SDFA_STREAM_MAX_RATES
struct StreamRate {
    const double *win;         // [2 nwin] this rate pair's half filter, then its forward differences
    int64_t step;              // table entries per input sample; 0: input rate = model rate, the samples are copied
    double scale;              // min(1, ratio)
};
struct StreamResampleArgs {
    const float *in_rings;     // n_in_rings rings of 2^r_in + STREAM_RING_MIRROR floats
    float *rings;              // n_rings model rings of 2^r + STREAM_RING_MIRROR floats
    int r_in, n_in_rings, r, n_rings;
    const int64_t *seg;        // [n_seg][8], see stream_resample_kernel
    const double *treg;        // [n_treg] time registers of the outputs, segment by segment
    int64_t n_treg, nwin;
    int num_table, n_rates;
    StreamRate rate[STREAM_MAX_RATES];
};
hipError_t sdfa_launch_stream_resample(const StreamResampleArgs &a, int n_seg, int64_t max_count, hipStream_t s);
