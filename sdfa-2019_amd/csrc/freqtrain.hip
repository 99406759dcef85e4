// Training step of the frequency LSTM and its projection (include/sdfa_freqtrain.h): the input projection
// with the biases, the recurrence along the 32 frequency bins with the activated gates and the cell state kept, X0 = HF Wp^T + bp,
// and backwards dHF, back-propagation through the 32 steps, and the products dWp, dbp, dW_ih, dW_hh, db, dC.
//
// The two recurrences are lstmtrain.hip's with four waves instead of eight: a workgroup owns a (direction, tile of 32 columns) for
// all 32 steps and never waits for another workgroup; wave w owns hidden units 32 w .. 32 w + 31 with its gate rows packed
// [i | f | g | o] on the MFMA row axis (four accumulators of one register layout, so the cell update is elementwise in registers),
// columns on the lanes; an accumulator starts from pre_f (the biases are in it) and takes W_hh h_{f-1} with k ascending; h crosses
// waves through LDS in K4 layout.  W_hh of a direction is 256 KiB and streams from L2 every step out of an image [k-quad][gate row]
// that makes a wave's request contiguous (backward: W_hh^T out of [row-quad][unit]): both directions' images are 512 KiB, which
// every workgroup of the launch reads 32 times over, and 64 N columns are 4 N workgroups, so the stream is shared L2 traffic.
// Holding a part of it in LDS would leave the other part streaming in the same loop, with two address patterns in it.
//
// The dense products are the tile routine of tile_acc.h.  Rows are the R = 64 N columns, or the 32 R pairs g = 32 column + step:
// gates, c, C and HF are all [g][.] buffers, which is what makes the step shift of PrevH one row.  Ones is the operand of the bias
// sums: a tile against a matrix of ones, whose column 0 is kept -- the same chain, the same order.  Everything summed over the
// columns is split into row blocks of FT_BLOCK_FRAMES frames, written as float32 partials in the flat parameter layout and added
// in ascending block order by the reduce launch.  Every offset is formed in 64 bits: gates pass 2^31 floats at 1,024 frames.
#include "common.h"
#include "freqtrain.h"
#include "tile_acc.h"

namespace {

using namespace sdfa_tile;
constexpr int NS = FT_S, NI = FT_I, NH = FT_H, NG = FT_G, NY = FT_Y, NK = FT_K, NO = FT_O, CT = FT_TILE_COLS;
constexpr int FWD_LDS = 2 * (NH / 4) * CT * 16, BWD_LDS = (NG / 4) * CT * 16;
static_assert(CT == 32 && NH == 128 && NG == 4 * NH && NI == T && FT_COLS % T == 0 && FT_COLS % CT == 0 && (NS & (NS - 1)) == 0 && BWD_LDS <= 64 * 1024,
              "a recurrence tile is one MFMA column block; a frame's columns are whole tiles, so no lane is ever past the batch");

// ---------------------------------------------------------------------------------------------------- operands
// element (i, c): i the tile's row or column index (always inside its matrix here), c the contraction index < nc
struct Plain {                       // p[i si + c sc]
    const float *p;
    int64_t si, sc;
    int nc;
    __device__ const float *at(int i, int c) const { return p + i * si + (int64_t)(c < nc ? c : nc - 1) * sc; }
    __device__ float val(int, int c, float v) const { return c < nc ? v : 0.f; }
};

struct GatesCat {                    // c = d 512 + r: both directions' gate rows of pair i, forward direction first
    const float *p;                  // gates + g0 * 512
    int64_t dstride;                 // 32 R 512
    __device__ const float *at(int i, int c) const {
        const int cc = c < 2 * NG ? c : 2 * NG - 1;
        return p + (int64_t)(cc >> 9) * dstride + (int64_t)i * NG + (cc & (NG - 1));
    }
    __device__ float val(int, int c, float v) const { return c < 2 * NG ? v : 0.f; }
};

struct PrevH {                       // (j, c): h of unit j at the pair one step before g0 + c in the direction's order
    const float *p;                  // HF + d 128 + v0
    int64_t g0, pairs;               // the block's first pair, 32 R
    int shift, first, nc;            // -1 and step 0 (forward), +1 and step 31 (reverse)
    __device__ const float *at(int j, int c) const {
        int64_t g = g0 + (c < nc ? c : nc - 1) + shift;
        g = g < 0 ? 0 : g >= pairs ? pairs - 1 : g;
        return p + g * NY + j;
    }
    __device__ float val(int, int c, float v) const { return c < nc && ((g0 + c) & (NS - 1)) != first ? v : 0.f; }
};

struct Ones {                        // 1 for c < nc: the bias sums as a tile
    const float *p;                  // any readable address
    int nc;
    __device__ const float *at(int, int) const { return p; }
    __device__ float val(int, int c, float) const { return c < nc ? 1.f : 0.f; }
};

// ---------------------------------------------------------------------------------------------------- the weight images
// img[d][kq][row] = W_hh[d][row][4 kq .. 4 kq + 3];  imgT[d][rq][u] = W_hh[d][4 rq .. 4 rq + 3][u]
__global__ __launch_bounds__(256) void freqtrain_images_kernel(FtImagesArgs a) {
    const int e = blockIdx.x * 256 + threadIdx.x;             // < 2 * 32 * 512
    const int d = e >> 14;
    const float *W = a.Whh + (int64_t)d * NG * NH;
    {
        const int kq = (e >> 9) & 31, row = e & (NG - 1);
        st4(a.img + (int64_t)e * 4, ld4(W + row * NH + 4 * kq));
    }
    {
        const int rq = (e >> 7) & 127, u = e & (NH - 1);
        st4(a.imgT + (int64_t)e * 4, make_float4(W[(4 * rq + 0) * NH + u], W[(4 * rq + 1) * NH + u], W[(4 * rq + 2) * NH + u], W[(4 * rq + 3) * NH + u]));
    }
}

// ---------------------------------------------------------------------------------------------------- pre = C W_ih^T + (b_ih + b_hh)
// grid: x = 16 tile of pairs + tile along the 1,024 gate rows of both directions
__global__ __launch_bounds__(THREADS) void freqtrain_pre_kernel(FtPreArgs a) {
    __shared__ float sA[CH * LP], sB[CH * LP];
    const int64_t g0 = (int64_t)(blockIdx.x >> 4) * T, pairs = a.N * FT_COLS * NS;
    const int j0 = (blockIdx.x & 15) * T;
    f32x16 acc;
    zero(acc);
    tile_acc<true, true>(acc, NI, Plain{a.C + g0 * NI, NI, 1, NI}, Plain{a.P + FT_OFF_WIH + (int64_t)j0 * NI, NI, 1, NI}, sA, sB);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31, h = lane >> 5;
    const int j = j0 + 32 * (wave & 1) + l31;
    const float bias = fadd_exact(a.P[FT_OFF_BIH + j], a.P[FT_OFF_BHH + j]);
    float *out = a.gates + ((int64_t)(j0 >> 9) * pairs + g0) * NG + (j & (NG - 1));
#pragma unroll
    for (int r = 0; r < 16; ++r) out[(int64_t)(32 * (wave >> 1) + (r & 3) + 8 * (r >> 2) + 4 * h) * NG] = fadd_exact(acc[r], bias);
}

// ---------------------------------------------------------------------------------------------------- forward recurrence
// grid: x = 2 tile + direction; 64 N columns are whole tiles.
__global__ __launch_bounds__(256) void freqtrain_forward_kernel(FtFwdArgs a) {
    extern __shared__ float4 sH[];                            // [2][32 k-quads][32 columns]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, h = lane >> 5;
    const int dir = blockIdx.x & 1;
    const int64_t R = a.N * FT_COLS, col = (int64_t)(blockIdx.x >> 1) * CT + l31;
    const int u0 = 32 * wave + 4 * h;                         // this lane's quad g holds units u0 + 8 g .. + 3
    float *G = a.gates + ((int64_t)dir * R + col) * NS * NG + u0;
    float *Cn = a.c + ((int64_t)dir * R + col) * NS * NH + u0;
    float *Yn = a.HF + col * NK + dir * NH + u0;
    const float4 *W = reinterpret_cast<const float4 *>(a.img) + (size_t)dir * (NH / 4) * NG + 32 * wave + l31;

    f32x16 acc[4], c;
    zero(c);
#define FT_SEED(t_)                                                                                              \
    _Pragma("unroll") for (int gt = 0; gt < 4; ++gt) _Pragma("unroll") for (int g = 0; g < 4; ++g) {             \
        const float4 v = ld4(G + (t_) * NG + gt * NH + 8 * g);                                                   \
        acc[gt][4 * g + 0] = v.x; acc[gt][4 * g + 1] = v.y; acc[gt][4 * g + 2] = v.z; acc[gt][4 * g + 3] = v.w;  \
    }
    FT_SEED(dir ? NS - 1 : 0)
    for (int s = 0; s < NS; ++s) {
        const int t = dir ? NS - 1 - s : s;
        if (s > 0) {
            const float4 *b = sH + (size_t)(s & 1) * (NH / 4) * CT + h * CT + l31;
            const float4 *w = W + (size_t)h * NG;
#pragma unroll 2
            for (int kb = 0; kb < NH / 8; ++kb) {
                const float4 bq = b[kb * 2 * CT];
                float4 wq[4];
#pragma unroll
                for (int gt = 0; gt < 4; ++gt) wq[gt] = w[(size_t)kb * 2 * NG + gt * NH];
#pragma unroll
                for (int q = 0; q < 4; ++q)
#pragma unroll
                    for (int gt = 0; gt < 4; ++gt) acc[gt] = MFMA(f4c(wq[gt], q), f4c(bq, q), acc[gt]);
            }
        }
        float4 *sHn = sH + (size_t)((s & 1) ^ 1) * (NH / 4) * CT;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            float gi[4], gf[4], gg[4], go[4], cn[4], hn[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int r = 4 * g + q;
                gi[q] = sigmoidf_acc(acc[0][r]);
                gf[q] = sigmoidf_acc(acc[1][r]);
                gg[q] = tanhf_acc(acc[2][r]);
                go[q] = sigmoidf_acc(acc[3][r]);
                cn[q] = fmaf(gf[q], c[r], fmul_exact(gi[q], gg[q]));
                c[r] = cn[q];
                hn[q] = fmul_exact(go[q], tanhf_acc(cn[q]));
            }
            const float4 hq = make_float4(hn[0], hn[1], hn[2], hn[3]);
            sHn[(8 * wave + 2 * g + h) * CT + l31] = hq;
            float *Gt = G + t * NG + 8 * g;
            st4(Gt, make_float4(gi[0], gi[1], gi[2], gi[3]));
            st4(Gt + NH, make_float4(gf[0], gf[1], gf[2], gf[3]));
            st4(Gt + 2 * NH, make_float4(gg[0], gg[1], gg[2], gg[3]));
            st4(Gt + 3 * NH, make_float4(go[0], go[1], go[2], go[3]));
            st4(Cn + t * NH + 8 * g, make_float4(cn[0], cn[1], cn[2], cn[3]));
            st4(Yn + t * NY + 8 * g, hq);
        }
        if (s + 1 < NS) { FT_SEED(dir ? t - 1 : t + 1) }
        __syncthreads();                                      // h_s complete before anyone reads it; the other half is free
    }
#undef FT_SEED
}

// ---------------------------------------------------------------------------------------------------- X0 = HF Wp^T + bp
// grid: x = 4 tile of 64 columns (a frame) + tile along the 256 outputs
__global__ __launch_bounds__(THREADS) void freqtrain_proj_kernel(FtProjArgs a) {
    __shared__ float sA[CH * LP], sB[CH * LP];
    const int64_t r0 = (int64_t)(blockIdx.x >> 2) * T;
    const int o0 = (blockIdx.x & 3) * T;
    f32x16 acc;
    zero(acc);
    tile_acc<true, true>(acc, NK, Plain{a.HF + r0 * NK, NK, 1, NK}, Plain{a.P + FT_OFF_WP + (int64_t)o0 * NK, NK, 1, NK}, sA, sB);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31, h = lane >> 5;
    const int o = o0 + 32 * (wave & 1) + l31;
    const float bias = a.P[FT_OFF_BP + o];
    float *out = a.X0 + r0 * NO + o;
#pragma unroll
    for (int r = 0; r < 16; ++r) out[(int64_t)(32 * (wave >> 1) + (r & 3) + 8 * (r >> 2) + 4 * h) * NO] = fadd_exact(acc[r], bias);
}

// ---------------------------------------------------------------------------------------------------- dHF = dX0 Wp
// grid: x = 128 tile of 64 columns + tile along the 8,192 features
__global__ __launch_bounds__(THREADS) void freqtrain_dhf_kernel(FtDhfArgs a) {
    __shared__ float sA[CH * LP], sB[CH * LP];
    const int64_t r0 = (int64_t)(blockIdx.x >> 7) * T;
    const int k0 = (blockIdx.x & 127) * T;
    f32x16 acc;
    zero(acc);
    tile_acc<true, false>(acc, NO, Plain{a.dX0 + r0 * NO, NO, 1, NO}, Plain{a.P + FT_OFF_WP + k0, 1, NK, NO}, sA, sB);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31, h = lane >> 5;
    float *out = a.dHF + r0 * NK + k0 + 32 * (wave & 1) + l31;
#pragma unroll
    for (int r = 0; r < 16; ++r) out[(int64_t)(32 * (wave >> 1) + (r & 3) + 8 * (r >> 2) + 4 * h) * NK] = acc[r];
}

// ---------------------------------------------------------------------------------------------------- backward recurrence
// grid: x = 2 tile + direction; the steps run against the direction's order.
__global__ __launch_bounds__(256) void freqtrain_backward_kernel(FtBwdArgs a) {
    extern __shared__ float4 sG[];                            // [128 row-quads of dG][32 columns]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, h = lane >> 5;
    const int dir = blockIdx.x & 1;
    const int64_t R = a.N * FT_COLS, col = (int64_t)(blockIdx.x >> 1) * CT + l31;
    const int u0 = 32 * wave + 4 * h;
    float *G = a.gates + ((int64_t)dir * R + col) * NS * NG + u0;
    const float *Cn = a.c + ((int64_t)dir * R + col) * NS * NH + u0;
    const float *dYn = a.dHF + col * NK + dir * NH + u0;
    const float4 *W = reinterpret_cast<const float4 *>(a.imgT) + (size_t)dir * (NG / 4) * NH + 32 * wave + l31 + (size_t)h * NH;
    const float4 *b = sG + h * CT + l31;

    f32x16 acc, dc;
    zero(acc);
    zero(dc);
    for (int s = 0; s < NS; ++s) {
        const int t = dir ? s : NS - 1 - s;
        const bool first = dir ? t == NS - 1 : t == 0;        // the direction's first step: c_{f-1} = 0
        const int tp = first ? t : dir ? t + 1 : t - 1;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float *Gt = G + t * NG + 8 * g;
            const float4 vi = ld4(Gt), vf = ld4(Gt + NH), vg = ld4(Gt + 2 * NH), vo = ld4(Gt + 3 * NH);
            const float4 vc = ld4(Cn + t * NH + 8 * g), vp = ld4(Cn + tp * NH + 8 * g), vy = ld4(dYn + t * NY + 8 * g);
            float di[4], df[4], dg[4], dO[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int r = 4 * g + q;
                const float gi = f4c(vi, q), gf = f4c(vf, q), gg = f4c(vg, q), go = f4c(vo, q);
                const float cp = first ? 0.f : f4c(vp, q);
                const float dh = fadd_exact(f4c(vy, q), acc[r]);
                const float tc = tanhf_acc(f4c(vc, q));
                dO[q] = fmul_exact(fmul_exact(dh, tc), fmul_exact(go, 1.0f - go));
                const float d = fmaf(fmul_exact(dh, go), fmaf(-tc, tc, 1.0f), dc[r]);
                di[q] = fmul_exact(fmul_exact(d, gg), fmul_exact(gi, 1.0f - gi));
                df[q] = fmul_exact(fmul_exact(d, cp), fmul_exact(gf, 1.0f - gf));
                dg[q] = fmul_exact(fmul_exact(d, gi), fmaf(-gg, gg, 1.0f));
                dc[r] = fmul_exact(d, gf);
            }
            const float4 qi = make_float4(di[0], di[1], di[2], di[3]), qf = make_float4(df[0], df[1], df[2], df[3]);
            const float4 qg = make_float4(dg[0], dg[1], dg[2], dg[3]), qo = make_float4(dO[0], dO[1], dO[2], dO[3]);
            const int rq = 8 * wave + 2 * g + h;
            sG[rq * CT + l31] = qi;
            sG[(NH / 4 + rq) * CT + l31] = qf;
            sG[(2 * NH / 4 + rq) * CT + l31] = qg;
            sG[(3 * NH / 4 + rq) * CT + l31] = qo;
            float *Go = G + t * NG + 8 * g;
            st4(Go, qi);
            st4(Go + NH, qf);
            st4(Go + 2 * NH, qg);
            st4(Go + 3 * NH, qo);
        }
        if (s + 1 == NS) break;
        __syncthreads();                                      // dG_f complete
        zero(acc);
#pragma unroll 4
        for (int kb = 0; kb < NG / 8; ++kb) {
            const float4 bq = b[kb * 2 * CT], wq = W[(size_t)kb * 2 * NH];
#pragma unroll
            for (int q = 0; q < 4; ++q) acc = MFMA(f4c(wq, q), f4c(bq, q), acc);
        }
        __syncthreads();                                      // every wave has read dG_f
    }
}

// ---------------------------------------------------------------------------------------------------- backward, the products
// tiles of a row block, in this order
constexpr int N_IH = 2 * (NG / T), N_HH = 2 * (NG / T) * (NH / T), N_B = 2 * (NG / T), N_WP = (NO / T) * (NK / T), N_BP = NO / T;
constexpr int N_BLK = N_IH + N_HH + N_B + N_WP + N_BP;

// grid: x = [per row block: dW_ih | dW_hh | db | dWp | dbp partial tiles] [dC tiles, 32 N]
__global__ __launch_bounds__(THREADS) void freqtrain_products_kernel(FtProdArgs a) {
    __shared__ float sA[CH * LP], sB[CH * LP];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, h = lane >> 5;
    const int rr = 32 * (wave >> 1) + 4 * h, cj = 32 * (wave & 1) + l31;     // this lane's first row and its column in a tile
    const int64_t R = a.N * FT_COLS, pairs = R * NS, dstride = pairs * NG;
    int64_t bid = blockIdx.x;
    f32x16 acc;
    zero(acc);
    if (bid < (int64_t)a.nblk * N_BLK) {
        const int64_t blk = bid / N_BLK;
        int tile = (int)(bid % N_BLK);
        const int64_t r0 = blk * FT_BLOCK_FRAMES * FT_COLS, rleft = R - r0;
        const int Cr = (int)(rleft < FT_BLOCK_FRAMES * FT_COLS ? rleft : FT_BLOCK_FRAMES * FT_COLS);     // the block's columns
        const int64_t g0 = r0 * NS;
        const int Cg = Cr * NS;                                                                         // and its pairs
        float *part = a.part + blk * FT_NUMEL, *out, *out2 = nullptr;
        int ldo;
        bool col0 = false;                               // a bias sum: column 0 of the tile
        if (tile < N_IH) {
            // a row block's share of dW_ih[d][r][ch] = sum_pairs dG[d][g][r] C[g][ch]
            const int d = tile / (NG / T), q0 = tile % (NG / T) * T;
            tile_acc<false, false>(acc, Cg, Plain{a.gates + d * dstride + g0 * NG + q0, 1, NG, Cg}, Plain{a.C + g0 * NI, 1, NI, Cg}, sA, sB);
            out = part + FT_OFF_WIH + ((int64_t)d * NG + q0) * NI;
            ldo = NI;
        } else if ((tile -= N_IH) < N_HH) {
            // dW_hh[d][r][u] = sum_pairs dG[d][g][r] h_prev[d][g][u]
            const int d = tile / ((NG / T) * (NH / T)), q0 = (tile / (NH / T)) % (NG / T) * T, v0 = tile % (NH / T) * T;
            tile_acc<false, false>(acc, Cg, Plain{a.gates + d * dstride + g0 * NG + q0, 1, NG, Cg},
                                   PrevH{a.HF + d * NH + v0, g0, pairs, d ? 1 : -1, d ? NS - 1 : 0, Cg}, sA, sB);
            out = part + FT_OFF_WHH + ((int64_t)d * NG + q0) * NH + v0;
            ldo = NH;
        } else if ((tile -= N_HH) < N_B) {
            // db_ih[d][r] = db_hh[d][r] = sum_pairs dG[d][g][r]
            const int d = tile / (NG / T), q0 = tile % (NG / T) * T;
            tile_acc<false, false>(acc, Cg, Plain{a.gates + d * dstride + g0 * NG + q0, 1, NG, Cg}, Ones{a.gates, Cg}, sA, sB);
            out = part + FT_OFF_BIH + d * NG + q0;
            out2 = part + FT_OFF_BHH + d * NG + q0;
            ldo = 1;
            col0 = true;
        } else if ((tile -= N_B) < N_WP) {
            // dWp[o][k] = sum_columns dX0[r][o] HF[r][k]
            const int o0 = tile / (NK / T) * T, k0 = tile % (NK / T) * T;
            tile_acc<false, false>(acc, Cr, Plain{a.dX0 + r0 * NO + o0, 1, NO, Cr}, Plain{a.HF + r0 * NK + k0, 1, NK, Cr}, sA, sB);
            out = part + FT_OFF_WP + (int64_t)o0 * NK + k0;
            ldo = NK;
        } else {
            // dbp[o] = sum_columns dX0[r][o]
            const int o0 = (tile - N_WP) * T;
            tile_acc<false, false>(acc, Cr, Plain{a.dX0 + r0 * NO + o0, 1, NO, Cr}, Ones{a.dX0, Cr}, sA, sB);
            out = part + FT_OFF_BP + o0;
            ldo = 1;
            col0 = true;
        }
        if (col0) {
            if (cj == 0) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    out[rr + (r & 3) + 8 * (r >> 2)] = acc[r];
                    if (out2) out2[rr + (r & 3) + 8 * (r >> 2)] = acc[r];
                }
            }
            return;
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) out[(int64_t)(rr + (r & 3) + 8 * (r >> 2)) * ldo + cj] = acc[r];
        return;
    }
    bid -= (int64_t)a.nblk * N_BLK;
    // dC[g][ch] = sum_{d, r} dG[d][g][r] W_ih[d][r][ch]
    const int64_t g0 = bid * T;
    tile_acc<true, false>(acc, 2 * NG, GatesCat{a.gates + g0 * NG, dstride}, Plain{a.P + FT_OFF_WIH, 1, NI, 2 * NG}, sA, sB);
#pragma unroll
    for (int r = 0; r < 16; ++r) a.dC[(g0 + rr + (r & 3) + 8 * (r >> 2)) * NI + cj] = acc[r];
}

// the row blocks' partials, ascending.  An element per thread.
__global__ __launch_bounds__(256) void freqtrain_reduce_kernel(FtReduceArgs a) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;      // FT_NUMEL is a multiple of 256
    float s = 0.f;
    for (int b = 0; b < a.nblk; ++b) s = fadd_exact(s, a.part[(int64_t)b * FT_NUMEL + e]);
    a.grad[e] = s;
}

hipError_t grow_lds(const void *fn, int bytes) { return hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes); }

// 64 N columns in tiles of 32, both directions
unsigned recurrence_grid(int64_t N) { return (unsigned)(2 * (N * FT_COLS / CT)); }

}  // namespace

hipError_t freqtrain_images(const FtImagesArgs &a, hipStream_t st) {
    hipLaunchKernelGGL(freqtrain_images_kernel, dim3(2 * (NH / 4) * NG / 256), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t freqtrain_pre(const FtPreArgs &a, hipStream_t st) {
    hipLaunchKernelGGL(freqtrain_pre_kernel, dim3((unsigned)(a.N * FT_COLS * NS / T * (2 * NG / T))), dim3(THREADS), 0, st, a);
    return hipGetLastError();
}

hipError_t freqtrain_forward(const FtFwdArgs &a, hipStream_t st) {
    const hipError_t e = grow_lds(reinterpret_cast<const void *>(freqtrain_forward_kernel), FWD_LDS);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(freqtrain_forward_kernel, dim3(recurrence_grid(a.N)), dim3(256), FWD_LDS, st, a);
    return hipGetLastError();
}

hipError_t freqtrain_proj(const FtProjArgs &a, hipStream_t st) {
    hipLaunchKernelGGL(freqtrain_proj_kernel, dim3((unsigned)(a.N * (FT_COLS / T) * (NO / T))), dim3(THREADS), 0, st, a);
    return hipGetLastError();
}

hipError_t freqtrain_dhf(const FtDhfArgs &a, hipStream_t st) {
    hipLaunchKernelGGL(freqtrain_dhf_kernel, dim3((unsigned)(a.N * (FT_COLS / T) * (NK / T))), dim3(THREADS), 0, st, a);
    return hipGetLastError();
}

hipError_t freqtrain_backward(const FtBwdArgs &a, hipStream_t st) {
    const hipError_t e = grow_lds(reinterpret_cast<const void *>(freqtrain_backward_kernel), BWD_LDS);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(freqtrain_backward_kernel, dim3(recurrence_grid(a.N)), dim3(256), BWD_LDS, st, a);
    return hipGetLastError();
}

hipError_t freqtrain_products(const FtProdArgs &a, hipStream_t st) {
    int64_t blocks = (int64_t)a.nblk * N_BLK;
    if (a.dC) blocks += a.N * FT_COLS * NS / T;
    hipLaunchKernelGGL(freqtrain_products_kernel, dim3((unsigned)blocks), dim3(THREADS), 0, st, a);
    return hipGetLastError();
}

hipError_t freqtrain_reduce(const FtReduceArgs &a, hipStream_t st) {
    hipLaunchKernelGGL(freqtrain_reduce_kernel, dim3((unsigned)(FT_NUMEL / 256)), dim3(256), 0, st, a);
    return hipGetLastError();
}
