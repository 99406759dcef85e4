// What the two LSTM trainers' kernels share (lstmtrain.hip, freqtrain.hip): the kept-gate forward recurrence
// and back-propagation through time, the W_hh images they stream, the operands of their tile_acc.h products, and the partials sum.
//
// The recurrences are templates over <steps TS, hidden units NH, GUARD>; gates 4 NH, a row of Y 2 NH and NH / 32 waves follow.  A
// workgroup owns a (direction, tile of 32 rows) for all TS steps and never waits for another workgroup; a row is a frame of the
// time LSTM or a column of the frequency LSTM.  Forward, after time_lstm_body (lstm.hip): wave w owns hidden units 32 w .. 32 w + 31
// with its gate rows packed [i | f | g | o] on the MFMA row axis (four accumulators of one register layout, so the cell update is
// elementwise in registers), rows on the lanes; an accumulator starts from pre_t and takes W_hh h_{t-1} with k ascending; W_hh
// streams from L2 every step out of an image [k-quad][gate row] that makes a wave's request contiguous; h crosses waves through LDS
// in K4 layout.  Backward is its transpose: wave w owns dh_rec of units 32 w .. 32 w + 31 (one accumulator), K = 4 NH over the rows
// of dG = [di|df|dg|do], which the elementwise gate backward of a step leaves in LDS (K4) for the next step's contraction and in
// the kept gates' place for the products; W_hh^T streams from an image [row-quad][unit].  With GUARD the lanes past the last row
// repeat it and store nothing; without it the rows are whole tiles and the stores are unconditional.
#pragma once
#include "common.h"
#include "tile_acc.h"

namespace sdfa_rec {

using sdfa_tile::zero;
constexpr int REC_TILE = 32;                                   // rows of one workgroup of a recurrence: one MFMA column block

template <int NH> constexpr int rec_fwd_lds = 2 * (NH / 4) * REC_TILE * 16;
template <int NH> constexpr int rec_bwd_lds = NH * REC_TILE * 16;

// ---------------------------------------------------------------------------------------------------- operands of tile_acc
// element (i, c): i the tile's row or column index (always inside its matrix here), c the contraction index < nc
struct Plain {                       // p[i si + c sc]
    const float *p;
    int64_t si, sc;
    int nc;
    __device__ const float *at(int i, int c) const { return p + i * si + (int64_t)(c < nc ? c : nc - 1) * sc; }
    __device__ float val(int, int c, float v) const { return c < nc ? v : 0.f; }
};

template <int NG>
struct GatesCat {                    // c = d NG + r: both directions' gate rows of row i, forward direction first
    const float *p;                  // gates + row0 * NG
    int64_t dstride;                 // rows * steps * NG
    __device__ const float *at(int i, int c) const {
        const int cc = c < 2 * NG ? c : 2 * NG - 1;
        return p + (int64_t)(cc / NG) * dstride + (int64_t)i * NG + (cc & (NG - 1));
    }
    __device__ float val(int, int c, float v) const { return c < 2 * NG ? v : 0.f; }
};

template <int STEPS, int NY>
struct PrevH {                       // (j, c): h of unit j at the row one step before row0 + c in the direction's order
    static_assert((STEPS & (STEPS - 1)) == 0, "a row's step is its low bits");
    const float *p;                  // Y + d NH + u0, Y being [rows][NY]: a row is a (frame or column, step) pair
    int64_t row0, rows;              // the block's first row, all rows
    int shift, first, nc;            // -1 and step 0 (forward), +1 and step STEPS - 1 (reverse)
    __device__ const float *at(int j, int c) const {
        int64_t r = row0 + (c < nc ? c : nc - 1) + shift;
        r = r < 0 ? 0 : r >= rows ? rows - 1 : r;
        return p + r * NY + j;
    }
    __device__ float val(int, int c, float v) const { return c < nc && ((row0 + c) & (STEPS - 1)) != first ? v : 0.f; }
};

struct Ones {                        // 1 for c < nc: the bias sums as a tile
    const float *p;                  // any readable address
    int nc;
    __device__ const float *at(int, int) const { return p; }
    __device__ float val(int, int c, float) const { return c < nc ? 1.f : 0.f; }
};

// ---------------------------------------------------------------------------------------------------- the weight images
// img[d][kq][row] = W_hh[d][row][4 kq .. 4 kq + 3];  imgT[d][rq][u] = W_hh[d][4 rq .. 4 rq + 3][u].  256 threads, a float4 of each.
template <int NH>
__device__ __forceinline__ void whh_images(const float *Whh, float *img, float *imgT) {
    constexpr unsigned NG = 4 * NH, KQ = NH / 4, RQ = NG / 4; // unsigned: the divisions are shifts
    const unsigned e = blockIdx.x * 256 + threadIdx.x;        // < 2 * KQ * NG
    const int d = blockIdx.x / (KQ * NG / 256);               // a block lies in one direction
    const float *W = Whh + (int64_t)d * NG * NH;
    {
        const int kq = e / NG % KQ, row = e % NG;
        st4(img + (int64_t)e * 4, ld4(W + row * NH + 4 * kq));
    }
    {
        const int rq = e / NH % RQ, u = e % NH;
        st4(imgT + (int64_t)e * 4, make_float4(W[(4 * rq + 0) * NH + u], W[(4 * rq + 1) * NH + u], W[(4 * rq + 2) * NH + u], W[(4 * rq + 3) * NH + u]));
    }
}

// ---------------------------------------------------------------------------------------------------- forward recurrence
// step t's pre-activations into the four accumulators
template <int NH>
__device__ __forceinline__ void rec_seed(f32x16 (&acc)[4], const float *G, int t) {
#pragma unroll
    for (int gt = 0; gt < 4; ++gt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float4 v = ld4(G + t * (4 * NH) + gt * NH + 8 * g);
            acc[gt][4 * g + 0] = v.x; acc[gt][4 * g + 1] = v.y; acc[gt][4 * g + 2] = v.z; acc[gt][4 * g + 3] = v.w;
        }
}

// grid: x = 2 tile + direction; NH / 32 waves; rec_fwd_lds<NH> bytes.  gates [2][rows][TS][4 NH] hold pre and take the activated
// gates, c is [2][rows][TS][NH], Y is [rows][TS][2 NH].
template <int TS, int NH, bool GUARD>
__device__ __forceinline__ void rec_forward(const float *img, float *gates, float *cell, float *Y, const int64_t rows) {
    constexpr int NG = 4 * NH, NY = 2 * NH, FT = REC_TILE;
    static_assert(NH % 32 == 0 && NH <= 256 && (TS & (TS - 1)) == 0, "a wave owns 32 hidden units; at most eight waves");
    extern __shared__ float4 sH[];                            // [2][NH / 4 k-quads][32 rows]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, h = lane >> 5;
    const int dir = blockIdx.x & 1;
    const int64_t n0 = (int64_t)(blockIdx.x >> 1) * FT;
    const bool live = !GUARD || n0 + l31 < rows;
    const int64_t n = live ? n0 + l31 : rows - 1;
    const int u0 = 32 * wave + 4 * h;                         // this lane's quad g holds units u0 + 8 g .. + 3
    float *G = gates + ((int64_t)dir * rows + n) * TS * NG + u0;
    float *Cn = cell + ((int64_t)dir * rows + n) * TS * NH + u0;
    float *Yn = Y + n * TS * NY + dir * NH + u0;
    const float4 *W = reinterpret_cast<const float4 *>(img) + (size_t)dir * (NH / 4) * NG + 32 * wave + l31;

    f32x16 acc[4], c;
    zero(c);
    rec_seed<NH>(acc, G, dir ? TS - 1 : 0);
    for (int s = 0; s < TS; ++s) {
        const int t = dir ? TS - 1 - s : s;
        if (s > 0) {
            const float4 *b = sH + (size_t)(s & 1) * (NH / 4) * FT + h * FT + l31;
            const float4 *w = W + (size_t)h * NG;
#pragma unroll 2
            for (int kb = 0; kb < NH / 8; ++kb) {
                const float4 bq = b[kb * 2 * FT];
                float4 wq[4];
#pragma unroll
                for (int gt = 0; gt < 4; ++gt) wq[gt] = w[(size_t)kb * 2 * NG + gt * NH];
#pragma unroll
                for (int q = 0; q < 4; ++q)
#pragma unroll
                    for (int gt = 0; gt < 4; ++gt) acc[gt] = MFMA(f4c(wq[gt], q), f4c(bq, q), acc[gt]);
            }
        }
        float4 *sHn = sH + (size_t)((s & 1) ^ 1) * (NH / 4) * FT;
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
            sHn[(8 * wave + 2 * g + h) * FT + l31] = hq;
            if (live) {
                float *Gt = G + t * NG + 8 * g;
                st4(Gt, make_float4(gi[0], gi[1], gi[2], gi[3]));
                st4(Gt + NH, make_float4(gf[0], gf[1], gf[2], gf[3]));
                st4(Gt + 2 * NH, make_float4(gg[0], gg[1], gg[2], gg[3]));
                st4(Gt + 3 * NH, make_float4(go[0], go[1], go[2], go[3]));
                st4(Cn + t * NH + 8 * g, make_float4(cn[0], cn[1], cn[2], cn[3]));
                st4(Yn + t * NY + 8 * g, hq);
            }
        }
        if (s + 1 < TS) rec_seed<NH>(acc, G, dir ? t - 1 : t + 1);
        __syncthreads();                                      // h_s complete before anyone reads it; the other half is free
    }
}

// ---------------------------------------------------------------------------------------------------- backward recurrence
// grid: x = 2 tile + direction; the steps run against the direction's order; rec_bwd_lds<NH> bytes.  gates hold the activated
// gates and take dG; dY is [rows][TS][2 NH].
template <int TS, int NH, bool GUARD>
__device__ __forceinline__ void rec_backward(const float *imgT, const float *cell, const float *dY, float *gates, const int64_t rows) {
    constexpr int NG = 4 * NH, NY = 2 * NH, FT = REC_TILE;
    static_assert(NH % 32 == 0 && NH <= 256 && rec_bwd_lds<NH> <= 160 * 1024, "a wave owns 32 hidden units; dG of a step fits LDS");
    extern __shared__ float4 sG[];                            // [NH row-quads of dG][32 rows]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, h = lane >> 5;
    const int dir = blockIdx.x & 1;
    const int64_t n0 = (int64_t)(blockIdx.x >> 1) * FT;
    const bool live = !GUARD || n0 + l31 < rows;
    const int64_t n = live ? n0 + l31 : rows - 1;
    const int u0 = 32 * wave + 4 * h;
    float *G = gates + ((int64_t)dir * rows + n) * TS * NG + u0;
    const float *Cn = cell + ((int64_t)dir * rows + n) * TS * NH + u0;
    const float *dYn = dY + n * TS * NY + dir * NH + u0;
    const float4 *W = reinterpret_cast<const float4 *>(imgT) + (size_t)dir * (NG / 4) * NH + 32 * wave + l31 + (size_t)h * NH;
    const float4 *b = sG + h * FT + l31;

    f32x16 acc, dc;
    zero(acc);
    zero(dc);
    for (int s = 0; s < TS; ++s) {
        const int t = dir ? s : TS - 1 - s;
        const bool first = dir ? t == TS - 1 : t == 0;        // the direction's first step: c_{t-1} = 0
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
            sG[rq * FT + l31] = qi;
            sG[(NH / 4 + rq) * FT + l31] = qf;
            sG[(2 * NH / 4 + rq) * FT + l31] = qg;
            sG[(3 * NH / 4 + rq) * FT + l31] = qo;
            if (live) {
                float *Go = G + t * NG + 8 * g;
                st4(Go, qi);
                st4(Go + NH, qf);
                st4(Go + 2 * NH, qg);
                st4(Go + 3 * NH, qo);
            }
        }
        if (s + 1 == TS) break;
        __syncthreads();                                      // dG_t complete
        zero(acc);
#pragma unroll 4
        for (int kb = 0; kb < NG / 8; ++kb) {
            const float4 bq = b[kb * 2 * FT], wq = W[(size_t)kb * 2 * NH];
#pragma unroll
            for (int q = 0; q < 4; ++q) acc = MFMA(f4c(wq, q), f4c(bq, q), acc);
        }
        __syncthreads();                                      // every wave has read dG_t
    }
}

// ---------------------------------------------------------------------------------------------------- the partials' sum
// the row blocks' partials, ascending.  256 threads, an element each: numel is a multiple of 256.
__device__ __forceinline__ void reduce_partials(const float *part, float *grad, const int64_t numel, const int nblk) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    float s = 0.f;
    for (int b = 0; b < nblk; ++b) s = fadd_exact(s, part[(int64_t)b * numel + e]);
    grad[e] = s;
}

inline hipError_t grow_lds(const void *fn, int bytes) { return hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes); }

}  // namespace sdfa_rec
