// Training step of one bidirectional LSTM layer (include/sdfa_lstmtrain.h): the input projection, the
// recurrence with the activated gates and the cell state kept, back-propagation through time, and the products dW_ih, dW_hh, dX.
//
// The two recurrences own a (direction, tile of 32 frames) per workgroup for all 64 steps and never wait for another workgroup.
// Forward, after time_lstm_body (lstm.hip): eight waves, wave w owns hidden units 32 w .. 32 w + 31 with its gate rows packed
// [i | f | g | o] on the MFMA row axis (four accumulators of one register layout, so the cell update is elementwise in registers),
// frames on the lanes; an accumulator starts from pre_t and takes W_hh h_{t-1} with k ascending; W_hh streams from L2 every step
// out of an image [k-quad][gate row] that makes a wave's request contiguous; h crosses waves through LDS in K4 layout.  Backward is
// its transpose: wave w owns dh_rec of units 32 w .. 32 w + 31 (one accumulator), K = 1,024 over the rows of dG = [di|df|dg|do],
// which the elementwise gate backward of a step leaves in LDS (K4, 128 KiB) for the next step's contraction and in the kept
// gates' place for the products; W_hh^T streams from an image [row-quad][unit].
//
// The products are the tile routine of tile_acc.h.  Operands: rows are the 64 N pairs (n, t); Gates(d) is dG of one direction,
// GatesCat both directions' 2,048 rows as one contraction index, PrevY the direction's h one step back read from Y where it lies
// (the row shifted by one step in at(), the zero of a direction's first step in val()).  dW_ih and dW_hh are split into row blocks
// of LT_BLOCK_FRAMES frames, written as float32 partials and added in ascending block order by the reduce launch.
#include "common.h"
#include "lstmtrain.h"
#include "tile_acc.h"

namespace {

using namespace sdfa_tile;
constexpr int TS = LT_T, NH = LT_H, NG = LT_G, NY = LT_Y, FT = LT_TILE_FRAMES;
constexpr int FWD_LDS = 2 * (NH / 4) * FT * 16, BWD_LDS = (NG / 4) * FT * 16;
static_assert(TS == T && FT == 32 && NH == 256 && NG == 4 * NH && BWD_LDS <= 160 * 1024, "one frame is one row tile; a recurrence tile is one MFMA column block");

// ---------------------------------------------------------------------------------------------------- operands
// element (i, c): i the tile's row or column index (always inside its matrix here), c the contraction index < nc
struct Plain {                       // p[i si + c sc]
    const float *p;
    int64_t si, sc;
    int nc;
    __device__ const float *at(int i, int c) const { return p + i * si + (int64_t)(c < nc ? c : nc - 1) * sc; }
    __device__ float val(int, int c, float v) const { return c < nc ? v : 0.f; }
};

struct GatesCat {                    // c = d 1024 + r: both directions' gate rows of row i, forward direction first
    const float *p;                  // gates + row0 * 1024
    int64_t dstride;                 // N 64 1024
    __device__ const float *at(int i, int c) const {
        const int cc = c < 2 * NG ? c : 2 * NG - 1;
        return p + (int64_t)(cc >> 10) * dstride + (int64_t)i * NG + (cc & (NG - 1));
    }
    __device__ float val(int, int c, float v) const { return c < 2 * NG ? v : 0.f; }
};

struct PrevY {                       // (j, c): h of unit j at the row one step before row0 + c in the direction's order
    const float *p;                  // Y + d 256 + u0
    int64_t row0, rows;              // the block's first row, 64 N
    int shift, first, nc;            // -1 and step 0 (forward), +1 and step 63 (reverse)
    __device__ const float *at(int j, int c) const {
        int64_t r = row0 + (c < nc ? c : nc - 1) + shift;
        r = r < 0 ? 0 : r >= rows ? rows - 1 : r;
        return p + r * NY + j;
    }
    __device__ float val(int, int c, float v) const { return c < nc && ((row0 + c) & (TS - 1)) != first ? v : 0.f; }
};

// ---------------------------------------------------------------------------------------------------- the weight images
// img[d][kq][row] = W_hh[d][row][4 kq .. 4 kq + 3];  imgT[d][rq][u] = W_hh[d][4 rq .. 4 rq + 3][u]
__global__ __launch_bounds__(256) void lstmtrain_images_kernel(LtImagesArgs a) {
    const int e = blockIdx.x * 256 + threadIdx.x;             // < 2 * 64 * 1024
    const int d = e >> 16;
    const float *W = a.Whh + (int64_t)d * NG * NH;
    {
        const int kq = (e >> 10) & 63, row = e & (NG - 1);
        st4(a.img + (int64_t)e * 4, ld4(W + row * NH + 4 * kq));
    }
    {
        const int rq = (e >> 8) & 255, u = e & (NH - 1);
        st4(a.imgT + (int64_t)e * 4, make_float4(W[(4 * rq + 0) * NH + u], W[(4 * rq + 1) * NH + u], W[(4 * rq + 2) * NH + u], W[(4 * rq + 3) * NH + u]));
    }
}

// ---------------------------------------------------------------------------------------------------- pre = X W_ih^T
// grid: x = tile along the 2,048 gate rows of both directions, y = frame
__global__ __launch_bounds__(THREADS) void lstmtrain_pre_kernel(LtPreArgs a) {
    __shared__ float sA[CH * LP], sB[CH * LP];
    const int64_t n = blockIdx.y;
    const int j0 = blockIdx.x * T;
    f32x16 acc;
    zero(acc);
    tile_acc<true, true>(acc, a.I, Plain{a.X + n * TS * a.I, a.I, 1, a.I}, Plain{a.Wih + (int64_t)j0 * a.I, a.I, 1, a.I}, sA, sB);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31, h = lane >> 5;
    float *out = a.gates + ((int64_t)(j0 >> 10) * a.N + n) * TS * NG + (j0 & (NG - 1)) + 32 * (wave & 1) + l31;
#pragma unroll
    for (int r = 0; r < 16; ++r) out[(int64_t)(32 * (wave >> 1) + (r & 3) + 8 * (r >> 2) + 4 * h) * NG] = acc[r];
}

// ---------------------------------------------------------------------------------------------------- forward recurrence
// grid: x = 2 tile + direction.  Lanes past the batch repeat its last frame and store nothing.
__global__ __launch_bounds__(512) void lstmtrain_forward_kernel(LtFwdArgs a) {
    extern __shared__ float4 sH[];                            // [2][64 k-quads][32 frames]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, h = lane >> 5;
    const int dir = blockIdx.x & 1;
    const int64_t n0 = (int64_t)(blockIdx.x >> 1) * FT;
    const bool live = n0 + l31 < a.N;
    const int64_t n = live ? n0 + l31 : a.N - 1;
    const int u0 = 32 * wave + 4 * h;                         // this lane's quad g holds units u0 + 8 g .. + 3
    float *G = a.gates + ((int64_t)dir * a.N + n) * TS * NG + u0;
    float *Cn = a.c + ((int64_t)dir * a.N + n) * TS * NH + u0;
    float *Yn = a.Y + n * TS * NY + dir * NH + u0;
    const float4 *W = reinterpret_cast<const float4 *>(a.img) + (size_t)dir * (NH / 4) * NG + 32 * wave + l31;

    f32x16 acc[4], c;
    zero(c);
#define LT_SEED(t_)                                                                                              \
    _Pragma("unroll") for (int gt = 0; gt < 4; ++gt) _Pragma("unroll") for (int g = 0; g < 4; ++g) {             \
        const float4 v = ld4(G + (t_) * NG + gt * NH + 8 * g);                                                   \
        acc[gt][4 * g + 0] = v.x; acc[gt][4 * g + 1] = v.y; acc[gt][4 * g + 2] = v.z; acc[gt][4 * g + 3] = v.w;  \
    }
    LT_SEED(dir ? TS - 1 : 0)
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
        if (s + 1 < TS) { LT_SEED(dir ? t - 1 : t + 1) }
        __syncthreads();                                      // h_s complete before anyone reads it; the other half is free
    }
#undef LT_SEED
}

// ---------------------------------------------------------------------------------------------------- backward recurrence
// grid: x = 2 tile + direction; the steps run against the direction's order.
__global__ __launch_bounds__(512) void lstmtrain_backward_kernel(LtBwdArgs a) {
    extern __shared__ float4 sG[];                            // [256 row-quads of dG][32 frames]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, h = lane >> 5;
    const int dir = blockIdx.x & 1;
    const int64_t n0 = (int64_t)(blockIdx.x >> 1) * FT;
    const bool live = n0 + l31 < a.N;
    const int64_t n = live ? n0 + l31 : a.N - 1;
    const int u0 = 32 * wave + 4 * h;
    float *G = a.gates + ((int64_t)dir * a.N + n) * TS * NG + u0;
    const float *Cn = a.c + ((int64_t)dir * a.N + n) * TS * NH + u0;
    const float *dYn = a.dY + n * TS * NY + dir * NH + u0;
    const float4 *W = reinterpret_cast<const float4 *>(a.imgT) + (size_t)dir * (NG / 4) * NH + 32 * wave + l31 + (size_t)h * NH;
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

// ---------------------------------------------------------------------------------------------------- backward, the products
// grid: x = [per row block: dW_ih partial tiles 2 x 16 x I/64 | dW_hh partial tiles 2 x 16 x 4] [dX tiles N x I/64]
__global__ __launch_bounds__(THREADS) void lstmtrain_products_kernel(LtProdArgs a) {
    __shared__ float sA[CH * LP], sB[CH * LP];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, h = lane >> 5;
    const int rr = 32 * (wave >> 1) + 4 * h, cj = 32 * (wave & 1) + l31;     // this lane's first row and its column in a tile
    const int64_t N = a.N, rows = N * TS, dstride = rows * NG;
    const int I = a.I, ct = I / T, n_ih = 2 * (NG / T) * ct, n_hh = 2 * (NG / T) * (NH / T);
    const int64_t numel = 2 * (int64_t)NG * (I + NH);
    int64_t bid = blockIdx.x;
    f32x16 acc;
    zero(acc);
    if (bid < (int64_t)a.nblk * (n_ih + n_hh)) {
        const int64_t blk = bid / (n_ih + n_hh);
        int tile = (int)(bid % (n_ih + n_hh));
        const int64_t row0 = blk * LT_BLOCK_FRAMES * TS, left = rows - row0;
        const int C = (int)(left < LT_BLOCK_FRAMES * TS ? left : LT_BLOCK_FRAMES * TS);
        float *out;
        int ldo;
        if (tile < n_ih) {
            // a row block's share of dW_ih[d][r][c] = sum_rows dG[d][row][r] X[row][c]
            const int d = tile / ((NG / T) * ct), r0 = (tile / ct) % (NG / T) * T, c0 = tile % ct * T;
            tile_acc<false, false>(acc, C, Plain{a.gates + d * dstride + row0 * NG + r0, 1, NG, C}, Plain{a.X + row0 * I + c0, 1, I, C}, sA, sB);
            out = a.part + blk * numel + ((int64_t)d * NG + r0) * I + c0;
            ldo = I;
        } else {
            // a row block's share of dW_hh[d][r][u] = sum_rows dG[d][row][r] h_prev[d][row][u]
            tile -= n_ih;
            const int d = tile / ((NG / T) * (NH / T)), r0 = (tile / (NH / T)) % (NG / T) * T, v0 = tile % (NH / T) * T;
            tile_acc<false, false>(acc, C, Plain{a.gates + d * dstride + row0 * NG + r0, 1, NG, C},
                                   PrevY{a.Y + d * NH + v0, row0, rows, d ? 1 : -1, d ? TS - 1 : 0, C}, sA, sB);
            out = a.part + blk * numel + 2 * (int64_t)NG * I + ((int64_t)d * NG + r0) * NH + v0;
            ldo = NH;
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) out[(int64_t)(rr + (r & 3) + 8 * (r >> 2)) * ldo + cj] = acc[r];
        return;
    }
    bid -= (int64_t)a.nblk * (n_ih + n_hh);
    // dX[n][t][c] = sum_{d, r} dG[d][n][t][r] W_ih[d][r][c]
    const int64_t n = bid / ct;
    const int c0 = (int)(bid % ct) * T;
    tile_acc<true, false>(acc, 2 * NG, GatesCat{a.gates + n * TS * NG, dstride}, Plain{a.Wih + c0, 1, I, 2 * NG}, sA, sB);
#pragma unroll
    for (int r = 0; r < 16; ++r) a.dX[(n * TS + rr + (r & 3) + 8 * (r >> 2)) * I + c0 + cj] = acc[r];
}

// the row blocks' partials, ascending.  An element per thread.
__global__ __launch_bounds__(256) void lstmtrain_reduce_kernel(LtReduceArgs a) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;      // numel is a multiple of 256
    float s = 0.f;
    for (int b = 0; b < a.nblk; ++b) s = fadd_exact(s, a.part[(int64_t)b * a.numel + e]);
    a.grad[e] = s;
}

hipError_t grow_lds(const void *fn, int bytes) { return hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes); }

}  // namespace

hipError_t lstmtrain_images(const LtImagesArgs &a, hipStream_t st) {
    hipLaunchKernelGGL(lstmtrain_images_kernel, dim3(2 * (NH / 4) * NG / 256), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t lstmtrain_pre(const LtPreArgs &a, hipStream_t st) {
    hipLaunchKernelGGL(lstmtrain_pre_kernel, dim3(2 * NG / T, (unsigned)a.N), dim3(THREADS), 0, st, a);
    return hipGetLastError();
}

hipError_t lstmtrain_forward(const LtFwdArgs &a, hipStream_t st) {
    const hipError_t e = grow_lds(reinterpret_cast<const void *>(lstmtrain_forward_kernel), FWD_LDS);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(lstmtrain_forward_kernel, dim3((unsigned)(2 * ((a.N + FT - 1) / FT))), dim3(512), FWD_LDS, st, a);
    return hipGetLastError();
}

hipError_t lstmtrain_backward(const LtBwdArgs &a, hipStream_t st) {
    const hipError_t e = grow_lds(reinterpret_cast<const void *>(lstmtrain_backward_kernel), BWD_LDS);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(lstmtrain_backward_kernel, dim3((unsigned)(2 * ((a.N + FT - 1) / FT))), dim3(512), BWD_LDS, st, a);
    return hipGetLastError();
}

hipError_t lstmtrain_products(const LtProdArgs &a, hipStream_t st) {
    int64_t blocks = (int64_t)a.nblk * 2 * (NG / T) * (a.I / T + NH / T);
    if (a.dX) blocks += a.N * (a.I / T);
    hipLaunchKernelGGL(lstmtrain_products_kernel, dim3((unsigned)blocks), dim3(THREADS), 0, st, a);
    return hipGetLastError();
}

hipError_t lstmtrain_reduce(const LtReduceArgs &a, hipStream_t st) {
    hipLaunchKernelGGL(lstmtrain_reduce_kernel, dim3((unsigned)(a.numel / 256)), dim3(256), 0, st, a);
    return hipGetLastError();
}
