// Column sharing ("legal redundancy"): the conv stack, the frequency LSTM and its projection act
// on every (frame, time-step) column independently, and windows of the same clip whose starts differ by a whole
// number of hops contain the SAME columns (frames 12 apart at 60 fps / 16 kHz / hop 128 share 39 of 64).  A column
// is bit-for-bit the same feature vector in both frames when it is interior in both -- t in [6, 58]: the delta
// filters then see true neighbours (edge replication touches t < 4 and t > 59, get_features.py:199-207) and their
// 9-tap stencil [t-4, t+4] avoids window column 0 (its first sample is not pre-emphasised, misc.py:17), column 1
// (which may share column 0's FFT) and column 63 (which may be transformed alone): frontend.hip pairs STFT columns
// by absolute hop index, so every other column has the same FFT partner, hence the same bits, in every frame.  Each distinct column is then
// evaluated once and scattered to every frame that contains it.  The map is rebuilt on the device for every call;
// nothing is cached between calls.  It comes from one of two fronts, which share the numbering kernels:
//   * the per-frame (clip, start) table (sdfa_launch_share_map: share_prev_kernel + share_owner_kernel), where the
//     caller has one -- the argument above is then the proof that the linked columns are equal;
//   * the contents of audio_feat (sdfa_launch_share_map_content), where it has not (sdfa_encoder_forward).  Nothing
//     is assumed about where the features came from: a column is linked to another only after the two columns'
//     384 words have been compared in full, as bit patterns (-0.0 != +0.0, NaNs by payload).  All bit-equal columns of
//     the chunk go under ONE owner, wherever in the chunk they are -- there is no search over frames and shifts:
//       share_hash_kernel     one streaming pass: a 64-bit hash of every column, and in its tail the column's entry
//                             in an open-addressing table of the chunk's hashes (cleared by a memset before): the
//                             slot of a hash keeps the smallest column index (index order: col_index below) that
//                             carries it.  Hashes only PROPOSE, and a minimum does not depend on the order in which
//                             the atomics land: the map is the same on every run.
//       share_resolve_kernel  every column looks its hash up.  The column the slot names is an owner; any other
//                             column is read and compared word for word with that owner, and is linked to it only
//                             if the compare passes.  One that fails (two contents, one hash) stays its own owner,
//                             as do the other columns of its content: a collision costs time only.
//     Links are one level deep, so nothing is walked, and the owner of a group is its first column in index order:
//     on front-end features the distinct columns are those of the frame table's map or fewer (zero-padded columns
//     at a clip's ends and copies further than 64 frames apart are grouped too).  What the mapped layer-0 recurrence
//     (lstm.hip: time_lstm_body, MAP) then reads: the 32 frames of a half-wave at one time step are a few runs of
//     consecutive distinct columns, or -- zero padding, silence -- one and the same column, so a request stays a few 128-byte lines and a tile with a clip's
//     end in it reads no more lines than an interior one (profiles/encoder_group_ab.txt: lstm0).
#include "common.h"
#include "kernels.h"

namespace {

// [a.t_lo, a.t_hi]: 6..58 for feature columns (above); 1..63 for mel columns (frontend.hip: only window column 0 differs)

// prev[n] = nearest earlier frame of the same clip whose start differs by d whole hops, 1 <= d <= t_hi - t_lo
__global__ void share_prev_kernel(ShareArgs a) {
    const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= a.Nc) return;
    int prev = -1, shift = 0;
    if (n < a.N) {
        const int clip = a.frame_clip[n];
        const int64_t s = a.frame_start[n];
        for (int back = 1; back <= 64 && n - back >= 0; ++back) {
            const int64_t q = n - back;
            if (a.frame_clip[q] != clip) break;
            const int64_t diff = s - a.frame_start[q];
            if (diff <= 0) break;
            if (diff > (int64_t)(a.t_hi - a.t_lo) * a.hop) break;
            if (diff % a.hop == 0) { prev = (int)q; shift = (int)(diff / a.hop); break; }
        }
    }
    a.prev[n] = prev;
    a.shift[n] = shift;
}

// Index order of the per-column arrays (owner, flag, uid, col_to_u) and of the numbering scan: time-step-major, i = t * Nc + n (the
// encoder's map: consecutive distinct columns are consecutive FRAMES at one time step, which is what the time-LSTM kernels read
// through the map), or frame-major, i = n * 64 + t (the front end's map: consecutive distinct columns are consecutive HOPS of one
// clip, so that mel_columns_kernel walks the PCM front to back, a frame's table rows are three contiguous runs and its 64 map
// entries one 256-byte line).  Mc = 64 * Nc either way; every kernel below is coalesced in either order.
__device__ __forceinline__ int64_t col_index(const ShareArgs &a, int64_t n, int t) { return a.frame_major ? n * 64 + t : (int64_t)t * a.Nc + n; }
__device__ __forceinline__ void col_of(const ShareArgs &a, int64_t i, int64_t &n, int &t) {
    if (a.frame_major) { n = i >> 6; t = (int)(i & 63); } else { n = i % a.Nc; t = (int)(i / a.Nc); }
}

// owner[i] = index of the canonical column holding the same feature vector; flag[i] = 1 if column i is its own owner
__global__ void share_owner_kernel(ShareArgs a) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.Mc) return;
    int64_t n;
    int t;
    col_of(a, i, n, t);
    if (n >= a.N) { a.owner[i] = -1; a.flag[i] = 0; return; }     // padding frame: never computed
    while (t >= a.t_lo && t <= a.t_hi) {
        const int p = a.prev[n];
        if (p < 0) break;
        const int tt = t + a.shift[n];
        if (tt > a.t_hi) break;
        n = p; t = tt;
    }
    const int64_t o = col_index(a, n, t);
    a.owner[i] = (int)o;
    a.flag[i] = o == i ? 1 : 0;
}

// ---- the content-based front ------------------------------------------------------------------------------------------
// A column is 384 words = 96 16-byte quads = 1,536 contiguous bytes of audio_feat.  The hash and the full compare give a
// column to a half-wave: lane l of the half reads quads l, l + 32, l + 64, so a wave's load covers two adjacent columns.
constexpr int COL_QUADS = 96;
constexpr unsigned long long GROUP_EMPTY = ~0ull;

__device__ __forceinline__ uint64_t mix64(uint64_t x) {
    x ^= x >> 32; x *= 0xd6e8feb86659fd93ull;
    x ^= x >> 32; x *= 0xd6e8feb86659fd93ull;
    return x ^ (x >> 32);
}

// hash[n * 64 + t] = sum over the column's quads of a mix of (quad bits, quad position): one coalesced pass over the chunk.  The lane
// that stores a column's hash also enters it in the group table: group_key holds the complement of a slot's hash (a hash is never 0, so
// the memset's all-ones word is an empty slot and no key), group_first the smallest column index with that hash.  Both only ever move
// one way (empty -> key, index downwards), so a plain look first spares the atomic where it would change nothing -- in a chunk of equal
// columns that is nearly every one of them -- and a stale look only costs the atomic it could have spared.
__global__ __launch_bounds__(256) void share_hash_kernel(ShareArgs a) {
    const int l = threadIdx.x & 31;
    const int64_t col = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 5, M = a.N * 64;
    uint64_t h = 0;
    if (col < M) {
        const uint4 *row = reinterpret_cast<const uint4 *>(a.feat) + col * COL_QUADS;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int q = l + 32 * j;
            const uint4 v = row[q];
            const uint64_t lo = (uint64_t)v.x | (uint64_t)v.y << 32, hi = (uint64_t)v.z | (uint64_t)v.w << 32;
            h += mix64(lo + 0x9e3779b97f4a7c15ull * (uint64_t)(2 * q + 1)) + mix64(hi + 0x9e3779b97f4a7c15ull * (uint64_t)(2 * q + 2));
        }
    }
    for (int off = 16; off; off >>= 1) h += __shfl_xor(h, off);      // offsets < 32: stays inside the half-wave
    h = mix64(h);
    if (a.hash_bits) h &= (1ull << a.hash_bits) - 1;
    h |= 1;                                                          // never 0
    // A workgroup's 8 columns are consecutive time steps of one frame (the grid is exact: col < M).  Of those with one hash only the first,
    // which has the smallest index of them in either order, goes to the table: in a chunk of equal columns, where every column of the
    // chunk meets on one slot before the first key is seen there, that is an eighth of the atomics on that one address.
    __shared__ unsigned long long wg_hash[8];
    const int c = threadIdx.x >> 5;
    if (l == 0) { a.hash[col] = h; wg_hash[c] = h; }
    __syncthreads();
    if (l) return;
    for (int j = 0; j < c; ++j)
        if (wg_hash[j] == h) return;
    const unsigned long long key = ~h;
    const unsigned i = (unsigned)col_index(a, col >> 6, (int)(col & 63));
    unsigned long long *keys = reinterpret_cast<unsigned long long *>(a.group_key);
    const int64_t mask = a.group_slots - 1;
    for (int64_t slot = (int64_t)(h >> 1) & mask, k = 0; k <= mask; ++k, slot = (slot + 1) & mask) {     // the table is at most half full
        unsigned long long cur = __hip_atomic_load(&keys[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == GROUP_EMPTY) {
            cur = atomicCAS(&keys[slot], GROUP_EMPTY, key);
            if (cur == GROUP_EMPTY) cur = key;
        }
        if (cur != key) continue;
        if (__hip_atomic_load(&a.group_first[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > i) atomicMin(&a.group_first[slot], i);
        break;
    }
}

// owner / flag as share_owner_kernel writes them.  A column to a half-wave, as above; the column that its hash's slot names is an owner, any
// other is compared in full with that one.  Padding frames own nothing.
__global__ __launch_bounds__(256) void share_resolve_kernel(ShareArgs a) {
    const int l = threadIdx.x & 31, half = (threadIdx.x & 63) >> 5;
    const int64_t col = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 5, n = col >> 6;       // col < 64 Nc: the grid is exact
    const int64_t i = col_index(a, n, (int)(col & 63));
    if (n >= a.N) {                                                  // wave-uniform: a wave's two columns are of one frame
        if (l == 0) { a.owner[i] = -1; a.flag[i] = 0; }
        return;
    }
    const uint64_t h = a.hash[col], mask = (uint64_t)a.group_slots - 1;
    uint64_t slot = (h >> 1) & mask;
    for (uint64_t k = 0; k < mask && a.group_key[slot] != ~h; ++k) slot = (slot + 1) & mask;   // it is there: share_hash_kernel put it
    const int64_t cand = a.group_key[slot] == ~h ? (int64_t)a.group_first[slot] : i;           // (were it not, the column would own itself: no index is read from an empty slot)
    bool differ = false;
    if (cand != i) {
        int64_t cn;
        int ct;
        col_of(a, cand, cn, ct);
        const uint4 *x = reinterpret_cast<const uint4 *>(a.feat) + col * COL_QUADS, *y = reinterpret_cast<const uint4 *>(a.feat) + (cn * 64 + ct) * COL_QUADS;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const uint4 u = x[l + 32 * k], v = y[l + 32 * k];
            differ |= ((u.x ^ v.x) | (u.y ^ v.y) | (u.z ^ v.z) | (u.w ^ v.w)) != 0;
        }
    }
    const uint64_t bad = __ballot(differ) >> (32 * half) & 0xffffffffull;
    if (l == 0) {
        const int64_t o = bad ? i : cand;
        a.owner[i] = (int)o;
        a.flag[i] = o == i ? 1 : 0;
    }
}

// Exclusive scan of flag[0..Mc) -> uid in three small launches: per-tile (1024 columns) scan + tile sums, a
// single-workgroup scan of the tile sums, then the per-tile fix-up that also writes the compacted source rows.
__device__ __forceinline__ int block_inclusive_scan_1024(int v, int *part) {
    const int tid = threadIdx.x;
    part[tid] = v;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const int x = tid >= off ? part[tid - off] : 0;
        __syncthreads();
        part[tid] += x;
        __syncthreads();
    }
    return part[tid];
}

__global__ __launch_bounds__(1024) void share_scan_tiles_kernel(ShareArgs a) {
    __shared__ int part[1024];
    const int64_t i = (int64_t)blockIdx.x * 1024 + threadIdx.x;
    const int f = i < a.Mc ? a.flag[i] : 0;
    const int inc = block_inclusive_scan_1024(f, part);
    if (i < a.Mc) a.uid[i] = inc - f;                 // exclusive, tile-local
    if (threadIdx.x == 1023) a.tile_sum[blockIdx.x] = inc;
}

// the tail rule (below): split while (T mod G) / G <= TAIL_NUM / TAIL_DEN
constexpr int TAIL_NUM = 3, TAIL_DEN = 4;
__global__ __launch_bounds__(1024) void share_scan_sums_kernel(ShareArgs a, int ntiles) {
    __shared__ int part[1024];
    int carry = 0;
    for (int base = 0; base < ntiles; base += 1024) {
        const int t = base + threadIdx.x;
        const int v = t < ntiles ? a.tile_sum[t] : 0;
        const int inc = block_inclusive_scan_1024(v, part);
        if (t < ntiles) a.tile_sum[t] = carry + inc - v;   // exclusive offset of the tile
        carry += part[1023];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const int64_t mu = carry, pad = (mu + 255) / 256 * 256;
        a.counts[0] = mu;
        a.counts[1] = pad;
        // The projection GEMM behind this map is persistent, fat_grid = G workgroups over T = pad / 256 column tiles: T mod G tiles
        // left over cost it a whole round.  It stops at q_full, the whole rounds, and the tail kernel (gemm_tail.hip) multiplies the
        // r = T mod G tiles behind -- when that is the cheaper way.  Measured at G = 256 (profiles/encoder_tail_ab.txt): a round of the
        // fat kernel 1.80 ms, the tail kernel 0.20 ms + 7.9 us per tile -- 1.71 ms at r = 192, 2.0 ms at r = 224.
        int64_t q_full = pad;
        if (a.fat_grid > 0 && a.tail_mode != 1) {
            const int64_t T = pad / 256, G = a.fat_grid, r = T % G;
            if (a.tail_mode == 2 || r * TAIL_DEN <= G * TAIL_NUM) q_full = (T - r) * 256;
        }
        a.counts[2] = q_full;
    }
}

__global__ __launch_bounds__(1024) void share_scan_fix_kernel(ShareArgs a) {
    const int64_t i = (int64_t)blockIdx.x * 1024 + threadIdx.x;
    const int64_t mu = a.counts[0], pad = a.counts[1];
    if (i < a.Mc) {
        const int u = a.uid[i] + a.tile_sum[blockIdx.x];
        a.uid[i] = u;
        int64_t n;
        int t;
        col_of(a, i, n, t);
        if (a.flag[i]) a.col_src[u] = (int)(n * 64 + t);     // row of audio_feat viewed as [N*64][384]
    }
    if (i >= mu && i < pad) a.col_src[i] = -1;        // padding columns read zeros (disjoint from the writes above: u < mu)
}

__global__ void share_assign_kernel(ShareArgs a) {
    const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= a.Mc) return;
    const int o = a.owner[m];
    a.col_to_u[m] = o >= 0 ? a.uid[o] : 0;
}

// Z[q][m] = Zu[q][col_to_u[m]]  (K4 quads, ld = Mc on both sides)
__global__ void expand_cols_kernel(const float4 *__restrict__ Zu, const int32_t *__restrict__ col_to_u, float4 *__restrict__ Z,
                                   int nquads, int64_t Mc) {
    const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= Mc) return;
    const int64_t u = col_to_u[m];
    for (int q = 0; q < nquads; ++q) Z[(int64_t)q * Mc + m] = Zu[(int64_t)q * Mc + u];
}

}  // namespace

// owner / flag -> uid, col_src, col_to_u, counts: the same numbering behind either front
static void launch_share_numbering(const ShareArgs &a, hipStream_t s) {
    const int ntiles = (int)((a.Mc + 1023) / 1024);
    hipLaunchKernelGGL(share_scan_tiles_kernel, dim3(ntiles), dim3(1024), 0, s, a);
    hipLaunchKernelGGL(share_scan_sums_kernel, dim3(1), dim3(1024), 0, s, a, ntiles);
    hipLaunchKernelGGL(share_scan_fix_kernel, dim3(ntiles), dim3(1024), 0, s, a);
    hipLaunchKernelGGL(share_assign_kernel, dim3((unsigned)((a.Mc + 255) / 256)), dim3(256), 0, s, a);
}

hipError_t sdfa_launch_share_map_content(const ShareArgs &a, hipStream_t s) {
    const hipError_t e = hipMemsetAsync(a.group_key, 0xff, (size_t)a.group_slots * 12, s);      // group_key | group_first: every slot empty, no index yet
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(share_hash_kernel, dim3((unsigned)(a.N * 8)), dim3(256), 0, s, a);       // 8 columns per workgroup, 64 per frame
    hipLaunchKernelGGL(share_resolve_kernel, dim3((unsigned)(a.Nc * 8)), dim3(256), 0, s, a);
    launch_share_numbering(a, s);
    return hipGetLastError();
}

hipError_t sdfa_launch_share_map(const ShareArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(share_prev_kernel, dim3((unsigned)((a.Nc + 255) / 256)), dim3(256), 0, s, a);
    hipLaunchKernelGGL(share_owner_kernel, dim3((unsigned)((a.Mc + 255) / 256)), dim3(256), 0, s, a);
    launch_share_numbering(a, s);
    return hipGetLastError();
}

hipError_t sdfa_launch_share_prev(const ShareArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(share_prev_kernel, dim3((unsigned)((a.Nc + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t sdfa_launch_expand_cols(const float *Zu, const int32_t *col_to_u, float *Z, int nquads, int64_t Mc, hipStream_t s) {
    hipLaunchKernelGGL(expand_cols_kernel, dim3((unsigned)((Mc + 255) / 256)), dim3(256), 0, s,
                       reinterpret_cast<const float4 *>(Zu), col_to_u, reinterpret_cast<float4 *>(Z), nquads, Mc);
    return hipGetLastError();
}

// sdfa_encoder_x0 (include/sdfa_bilstm.h): the expanded frequency projection Z, K4 [64 quads][Mc], m = t*Nc + n  ->  rows
// (n, 64 t, 256), what layer 0 of the BiLSTM reads.  (The debug tap of Z writes the reference's (n, 256, 64 t), the transpose of this.)
// A block is one time step of four frames: a thread moves one quad, the four frames of a quad are read as one 64-byte run and a
// frame's 16 quads of a wave are written as one 256-byte run.
namespace {
__global__ void __launch_bounds__(256) x0_rows_kernel(const float4 *__restrict__ src, int64_t N, int64_t Nc, float4 *__restrict__ dst) {
    const int t = (int)(blockIdx.x & 63);
    const int64_t n = (int64_t)(blockIdx.x >> 6) * 4 + (threadIdx.x & 3);
    const int q = (int)(threadIdx.x >> 2);
    if (n >= N) return;
    dst[(n * 64 + t) * 64 + q] = src[(int64_t)q * 64 * Nc + (int64_t)t * Nc + n];
}
}  // namespace

hipError_t sdfa_launch_x0_rows(const float *Z, int64_t N, int64_t Nc, float *dst, hipStream_t s) {
    if (N < 1 || N > Nc || (N + 3) / 4 * 64 > 0x7fffffff) return hipErrorInvalidValue;
    hipLaunchKernelGGL(x0_rows_kernel, dim3((unsigned)((N + 3) / 4 * 64)), dim3(256), 0, s, reinterpret_cast<const float4 *>(Z), N, Nc,
                       reinterpret_cast<float4 *>(dst));
    return hipGetLastError();
}

// sdfa_encoder_conv (include/sdfa_freqtrain.h): the conv stack's output X3, K4 [512 quads][Mc] with rows f*64 + ch  ->  rows
// (n, 64 t, 32 f, 64 ch), what the frequency LSTM reads.  A column's 2,048 features are already in output order, so the copy is a
// transpose of [quad][column].  On the shared-column path X3 holds a chunk's distinct columns only: column (t, n) is then read at
// col_to_u[t*Nc + n], as expand_cols_kernel reads it; a null map is the every-column layout.  A block is one time step of four
// frames, as in x0_rows_kernel: a thread moves one quad of each of eight 64-quad slices.
namespace {
__global__ void __launch_bounds__(256) conv_rows_kernel(const float4 *__restrict__ src, const int32_t *__restrict__ col_to_u, int64_t N, int64_t Nc,
                                                        float4 *__restrict__ dst) {
    const int t = (int)(blockIdx.x & 63);
    const int64_t n = (int64_t)(blockIdx.x >> 6) * 4 + (threadIdx.x & 3);
    if (n >= N) return;
    const int64_t Mc = 64 * Nc, m = (int64_t)t * Nc + n, u = col_to_u ? col_to_u[m] : m;
    for (int q = (int)(threadIdx.x >> 2); q < 512; q += 64) dst[(n * 64 + t) * 512 + q] = src[(int64_t)q * Mc + u];
}
}  // namespace

hipError_t sdfa_launch_conv_rows(const float *X3, const int32_t *col_to_u, int64_t N, int64_t Nc, float *dst, hipStream_t s) {
    if (N < 1 || N > Nc || (N + 3) / 4 * 64 > 0x7fffffff) return hipErrorInvalidValue;
    hipLaunchKernelGGL(conv_rows_kernel, dim3((unsigned)((N + 3) / 4 * 64)), dim3(256), 0, s, reinterpret_cast<const float4 *>(X3), col_to_u, N, Nc,
                       reinterpret_cast<float4 *>(dst));
    return hipGetLastError();
}
