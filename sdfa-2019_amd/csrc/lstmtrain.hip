// Training step of one bidirectional LSTM layer (include/sdfa_lstmtrain.h): the input projection, the
// recurrence with the activated gates and the cell state kept, back-propagation through time, and the products dW_ih, dW_hh, dX.
//
// The two recurrences are lstm_train_rec.h's at 64 steps and 256 hidden units, eight waves, a tile of 32 frames per workgroup and
// the guard for the frames past the batch: dG of a step is 128 KiB of LDS.
//
// The products are the tile routine of tile_acc.h.  Operands (lstm_train_rec.h): rows are the 64 N pairs (n, t); Gates(d) is dG of
// one direction, GatesCat both directions' 2,048 rows as one contraction index, PrevH the direction's h one step back read from Y
// where it lies (the row shifted by one step in at(), the zero of a direction's first step in val()).  dW_ih and dW_hh are split
// into row blocks of LT_BLOCK_FRAMES frames, written as float32 partials and added in ascending block order by the reduce launch.
#include "common.h"
#include "lstm_train_rec.h"
#include "lstmtrain.h"
#include "tile_acc.h"

namespace {

using namespace sdfa_tile;
using namespace sdfa_rec;
constexpr int TS = LT_T, NH = LT_H, NG = LT_G, NY = LT_Y, FT = LT_TILE_FRAMES;
constexpr int FWD_LDS = rec_fwd_lds<NH>, BWD_LDS = rec_bwd_lds<NH>;
static_assert(TS == T && FT == REC_TILE && NH == 256 && NG == 4 * NH, "one frame is one row tile; the recurrences' 512 threads are eight waves");

__global__ __launch_bounds__(256) void lstmtrain_images_kernel(LtImagesArgs a) { whh_images<NH>(a.Whh, a.img, a.imgT); }

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
    for (int r = 0; r < 16; ++r) out[(int64_t)(32 * (wave >> 1) + tile_row(r, h)) * NG] = acc[r];
}

// ---------------------------------------------------------------------------------------------------- the recurrences
// grid: x = 2 tile + direction.  Lanes past the batch repeat its last frame and store nothing.
__global__ __launch_bounds__(512) void lstmtrain_forward_kernel(LtFwdArgs a) { rec_forward<TS, NH, true>(a.img, a.gates, a.c, a.Y, a.N); }

__global__ __launch_bounds__(512) void lstmtrain_backward_kernel(LtBwdArgs a) { rec_backward<TS, NH, true>(a.imgT, a.c, a.dY, a.gates, a.N); }

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
                                   PrevH<TS, NY>{a.Y + d * NH + v0, row0, rows, d ? 1 : -1, d ? TS - 1 : 0, C}, sA, sB);
            out = a.part + blk * numel + 2 * (int64_t)NG * I + ((int64_t)d * NG + r0) * NH + v0;
            ldo = NH;
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) out[(int64_t)(rr + tile_row(r, 0)) * ldo + cj] = acc[r];
        return;
    }
    bid -= (int64_t)a.nblk * (n_ih + n_hh);
    // dX[n][t][c] = sum_{d, r} dG[d][n][t][r] W_ih[d][r][c]
    const int64_t n = bid / ct;
    const int c0 = (int)(bid % ct) * T;
    tile_acc<true, false>(acc, 2 * NG, GatesCat<NG>{a.gates + n * TS * NG, dstride}, Plain{a.Wih + c0, 1, I, 2 * NG}, sA, sB);
#pragma unroll
    for (int r = 0; r < 16; ++r) a.dX[(n * TS + rr + tile_row(r, 0)) * I + c0 + cj] = acc[r];
}

__global__ __launch_bounds__(256) void lstmtrain_reduce_kernel(LtReduceArgs a) { reduce_partials(a.part, a.grad, a.numel, a.nblk); }

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
