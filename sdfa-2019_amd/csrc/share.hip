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
//     384 words have been compared in full, as bit patterns (-0.0 != +0.0, NaNs by payload).  Four kernels:
//       share_hash_kernel     one streaming pass: a 64-bit hash of every column.  Hashes only PROPOSE.
//       share_match_kernel    per frame n, the earlier frame p = n - b (b <= 64, same chunk) and shift d >= 1 for
//                             which the most columns' hashes agree, hash(n, t) == hash(p, t + d): the table's
//                             prev / shift (frames 12 back, d = 25 at 16 kHz / 60 fps) without the table.  The
//                             table's own (p, d) is among the candidates, so on front-end features this front links
//                             at least as many columns per frame as the table does (53 - d of them), and the number
//                             of distinct columns -- the columns without a link -- is at most the table's.
//       share_verify_kernel   every proposed pair (n, t) ~ (p, t + d) with equal hashes is read and compared word
//                             for word; only a pair that passes gets its bit in linked[n].
//       share_owner_content_kernel  follows verified links to the canonical column.  A step goes to an earlier
//                             frame and a LATER time step (d >= 1, t + d <= 63), so a walk ends within 63 steps
//                             whatever the data (an all-zero chunk links every (n, t) to (n - 1, t + 1)).
//     Equality is transitive, so a chain of verified links is sound; a copy that is not found costs time only.
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

__device__ __forceinline__ uint64_t mix64(uint64_t x) {
    x ^= x >> 32; x *= 0xd6e8feb86659fd93ull;
    x ^= x >> 32; x *= 0xd6e8feb86659fd93ull;
    return x ^ (x >> 32);
}

// hash[n * 64 + t] = sum over the column's quads of a mix of (quad bits, quad position): one coalesced pass over the chunk
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
    if (col < M && l == 0) a.hash[col] = mix64(h) | 1;              // never 0: 0 marks an empty slot of share_match_kernel's table
}

// prev[n] / shift[n] = the (p, d), n - 64 <= p < n, 1 <= d <= 63, with the most t for which hash(n, t) == hash(p, t + d); ties go to the
// nearest frame, then to the smallest shift; prev = -1 when no hash of the frame reappears.  One wave per frame.  Most earlier frames
// hold no column of frame n at all (at 60 fps / hop 128 only every twelfth is hop-aligned with it), so the frame's 64 hashes go into
// a small open-addressing table in LDS first and a frame p is looked at further only if one of its hashes is in the table.  For such
// a p, lane tt holds hash(p, tt) and compares it with hash(n, tt - d) from LDS, for every d that could still beat the best so far (a
// shift of d has only 64 - d columns to offer, so the loop shrinks as soon as a good pair is known -- at once, in a chunk of equal
// columns).
constexpr int MATCH_SLOTS = 128;      // twice the keys: a probe sequence ends at an empty slot after at most 64 occupied ones
__global__ __launch_bounds__(256) void share_match_kernel(ShareArgs a) {
    __shared__ unsigned long long hn[4][64], tab[4][MATCH_SLOTS];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t n = (int64_t)blockIdx.x * 4 + w;
    const bool real = n < a.N && n > 0;                              // wave-uniform
    const unsigned long long mine = real ? a.hash[n * 64 + lane] : 1;
    hn[w][lane] = mine;
    tab[w][lane] = 0; tab[w][lane + 64] = 0;
    __syncthreads();
    for (int slot = (int)(mine >> 8) & (MATCH_SLOTS - 1), k = 0; k < MATCH_SLOTS; ++k, slot = (slot + 1) & (MATCH_SLOTS - 1)) {
        const unsigned long long old = atomicCAS(&tab[w][slot], 0ull, mine);
        if (old == 0 || old == mine) break;                          // mine now, or an equal column of this frame got there first
    }
    __syncthreads();
    if (n >= a.Nc) return;
    int best = 0, bp = -1, bd = 0;
    if (real) {
        const int64_t lo = n > 64 ? n - 64 : 0;
        unsigned long long hp = a.hash[(n - 1) * 64 + lane];
        for (int64_t p = n - 1; p >= lo && best < 63; --p) {
            const unsigned long long hq = p > lo ? a.hash[(p - 1) * 64 + lane] : 0;      // next frame's hashes: in flight during this one's work
            bool member = false;
            for (int slot = (int)(hp >> 8) & (MATCH_SLOTS - 1), k = 0; k < MATCH_SLOTS; ++k, slot = (slot + 1) & (MATCH_SLOTS - 1)) {
                const unsigned long long v = tab[w][slot];
                if (v == hp) member = true;
                if (v == hp || v == 0) break;
            }
            if (__ballot(member)) {
                for (int d0 = 1; d0 < 64 - best; d0 += 4) {          // four shifts per round: independent LDS reads
                    int c[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int d = d0 + k;
                        const bool eq = lane >= d && hn[w][lane >= d ? lane - d : 0] == hp;       // d > 63: no lane, count 0
                        c[k] = __popcll(__ballot(eq));
                    }
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (c[k] > best) { best = c[k]; bp = (int)p; bd = d0 + k; }
                }
            }
            hp = hq;
        }
    }
    if (lane == 0) { a.prev[n] = bp; a.shift[n] = bd; }
}

// linked[n] bit t = columns (n, t) and (prev[n], t + shift[n]) hold the same 384 words.  Only pairs whose hashes agree are read; every
// such pair is read in full.  One workgroup per frame, 16 columns per wave, two columns (one per half-wave) per step.
__global__ __launch_bounds__(256) void share_verify_kernel(ShareArgs a) {
    const int64_t n = blockIdx.x;
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, half = lane >> 5, l = lane & 31;
    const int p = a.prev[n], d = a.shift[n];
    unsigned bits = 0;                                               // wave-uniform: the verdicts of columns 16 w .. 16 w + 15
    if (p >= 0) {
        const uint64_t *hn = a.hash + n * 64, *hp = a.hash + (int64_t)p * 64;
        const uint4 *fn = reinterpret_cast<const uint4 *>(a.feat) + n * 64 * COL_QUADS;
        const uint4 *fp = reinterpret_cast<const uint4 *>(a.feat) + (int64_t)p * 64 * COL_QUADS;
        for (int j = 0; j < 8; ++j) {
            const int t = 16 * w + 2 * j + half, tt = t + d;
            const bool cand = tt < 64 && hn[t] == hp[tt];           // uniform over the half-wave
            bool differ = false;
            if (cand) {
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const uint4 x = fn[t * COL_QUADS + l + 32 * k], y = fp[tt * COL_QUADS + l + 32 * k];
                    differ |= ((x.x ^ y.x) | (x.y ^ y.y) | (x.z ^ y.z) | (x.w ^ y.w)) != 0;
                }
            }
            const uint64_t c = __ballot(cand), bad = __ballot(differ);
            if ((c & 1) && !(bad & 0xffffffffull)) bits |= 1u << (2 * j);
            if ((c >> 32 & 1) && !(bad >> 32)) bits |= 1u << (2 * j + 1);
        }
    }
    if (lane == 0) reinterpret_cast<uint16_t *>(a.linked)[n * 4 + w] = (uint16_t)bits;     // little-endian: bits 16 w .. 16 w + 15 of linked[n]
}

// owner / flag as share_owner_kernel writes them, from the verified links.  A set bit t of linked[n] implies t + shift[n] <= 63 and
// shift[n] >= 1 (share_match_kernel, share_verify_kernel), so t grows with every step: the walk is over within 63 steps for any input.
__global__ void share_owner_content_kernel(ShareArgs a) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.Mc) return;
    int64_t n;
    int t;
    col_of(a, i, n, t);
    if (n >= a.N) { a.owner[i] = -1; a.flag[i] = 0; return; }     // padding frame: never computed
    while (t < 63 && (a.linked[n] >> t & 1)) {
        t += a.shift[n];
        n = a.prev[n];
    }
    const int64_t o = col_index(a, n, t);
    a.owner[i] = (int)o;
    a.flag[i] = o == i ? 1 : 0;
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
    hipLaunchKernelGGL(share_hash_kernel, dim3((unsigned)(a.N * 8)), dim3(256), 0, s, a);       // 8 columns per workgroup, 64 per frame
    hipLaunchKernelGGL(share_match_kernel, dim3((unsigned)(a.Nc / 4)), dim3(256), 0, s, a);     // Nc is a multiple of 128
    hipLaunchKernelGGL(share_verify_kernel, dim3((unsigned)a.N), dim3(256), 0, s, a);
    hipLaunchKernelGGL(share_owner_content_kernel, dim3((unsigned)((a.Mc + 255) / 256)), dim3(256), 0, s, a);
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
