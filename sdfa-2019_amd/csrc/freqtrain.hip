// Training step of the frequency LSTM and its projection (include/sdfa_freqtrain.h): the input projection
// with the biases, the recurrence along the 32 frequency bins with the activated gates and the cell state kept, X0 = HF Wp^T + bp,
// and backwards dHF, back-propagation through the 32 steps, and the products dWp, dbp, dW_ih, dW_hh, db, dC.
//
// The two recurrences are lstm_train_rec.h's at 32 steps and 128 hidden units, four waves, over the 64 N columns as rows and
// without the guard: a frame's columns are whole tiles.  The pre-activations have the biases in them.  W_hh of a direction is
// 256 KiB: both directions' images are 512 KiB, which every workgroup of the launch reads 32 times over, and 64 N columns are 4 N
// workgroups, so the stream is shared L2 traffic.  Holding a part of it in LDS would leave the other part streaming in the same
// loop, with two address patterns in it.
//
// The dense products are the tile routine of tile_acc.h, the operands lstm_train_rec.h's.  Rows are the R = 64 N columns, or the
// 32 R pairs g = 32 column + step: gates, c, C and HF are all [g][.] buffers, which is what makes the step shift of PrevH one row.
// Ones is the operand of the bias sums: a tile against a matrix of ones, whose column 0 is kept -- the same chain, the same order.
// Everything summed over the columns is split into row blocks of FT_BLOCK_FRAMES frames, written as float32 partials in the flat
// parameter layout and added in ascending block order by the reduce launch.  Every offset is formed in 64 bits: gates pass 2^31
// floats at 1,024 frames.
#include "common.h"
#include "freqtrain.h"
#include "lstm_train_rec.h"
#include "tile_acc.h"

namespace {

using namespace sdfa_tile;
using namespace sdfa_rec;
constexpr int NS = FT_S, NI = FT_I, NH = FT_H, NG = FT_G, NY = FT_Y, NK = FT_K, NO = FT_O, CT = FT_TILE_COLS;
constexpr int FWD_LDS = rec_fwd_lds<NH>, BWD_LDS = rec_bwd_lds<NH>;
static_assert(CT == REC_TILE && NH == 128 && NG == 4 * NH && NK == NS * NY && NI == T && FT_COLS % T == 0 && FT_COLS % CT == 0 && BWD_LDS <= 64 * 1024,
              "the recurrences' 256 threads are four waves; a frame's columns are whole tiles, so no lane is ever past the batch");

__global__ __launch_bounds__(256) void freqtrain_images_kernel(FtImagesArgs a) { whh_images<NH>(a.Whh, a.img, a.imgT); }

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
    for (int r = 0; r < 16; ++r) out[(int64_t)(32 * (wave >> 1) + tile_row(r, h)) * NG] = fadd_exact(acc[r], bias);
}

// ---------------------------------------------------------------------------------------------------- forward recurrence
// grid: x = 2 tile + direction; 64 N columns are whole tiles.
__global__ __launch_bounds__(256) void freqtrain_forward_kernel(FtFwdArgs a) { rec_forward<NS, NH, false>(a.img, a.gates, a.c, a.HF, a.N * FT_COLS); }

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
    for (int r = 0; r < 16; ++r) out[(int64_t)(32 * (wave >> 1) + tile_row(r, h)) * NO] = fadd_exact(acc[r], bias);
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
    for (int r = 0; r < 16; ++r) out[(int64_t)(32 * (wave >> 1) + tile_row(r, h)) * NK] = acc[r];
}

// ---------------------------------------------------------------------------------------------------- backward recurrence
__global__ __launch_bounds__(256) void freqtrain_backward_kernel(FtBwdArgs a) { rec_backward<NS, NH, false>(a.imgT, a.c, a.dHF, a.gates, a.N * FT_COLS); }

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
                                   PrevH<NS, NY>{a.HF + d * NH + v0, g0, pairs, d ? 1 : -1, d ? NS - 1 : 0, Cg}, sA, sB);
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
                    out[rr + tile_row(r, 0)] = acc[r];
                    if (out2) out2[rr + tile_row(r, 0)] = acc[r];
                }
            }
            return;
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) out[(int64_t)(rr + tile_row(r, 0)) * ldo + cj] = acc[r];
        return;
    }
    bid -= (int64_t)a.nblk * N_BLK;
    // dC[g][ch] = sum_{d, r} dG[d][g][r] W_ih[d][r][ch]
    const int64_t g0 = bid * T;
    tile_acc<true, false>(acc, 2 * NG, GatesCat<NG>{a.gates + g0 * NG, dstride}, Plain{a.P + FT_OFF_WIH, 1, NI, 2 * NG}, sA, sB);
#pragma unroll
    for (int r = 0; r < 16; ++r) a.dC[(g0 + rr + tile_row(r, 0)) * NI + cj] = acc[r];
}

__global__ __launch_bounds__(256) void freqtrain_reduce_kernel(FtReduceArgs a) { reduce_partials(a.part, a.grad, FT_NUMEL, a.nblk); }

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
