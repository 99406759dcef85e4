// Rendered video frames (on the device) -> baseline JPEG files, batched over frames, byte for byte what PIL writes.
//
// The format contract -- markers, quantisation, colour conversion, padding, islow DCT, entropy coding -- is written down
// in include/sdfa_jpeg.h and DESIGN.md "GPU JPEG"; tests/jpeg_oracle.py restates every stage in numpy.  All of it is
// integer arithmetic, so every stage is bitwise.
//
// Seven launches per call of n frames (and one memset of the bit buffer):
//   (1) jpeg_transform_kernel : 384 threads per (frame, 8 MCUs), 8 lanes per block.  A lane forms one row of its block
//       (colour conversion, 2x2 downsampling, edge padding, level shift) and runs the islow row pass; after an LDS
//       exchange it runs the column pass of one column, quantises and writes the int16 coefficients in zigzag order.
//       Dummy luma blocks take their DC from an LDS copy of their MCU's DCs.
//   (2) jpeg_bits_kernel<false> : one wave per block, one lane per coefficient.  A 64-bit ballot of the nonzero lanes
//       gives each symbol's run (and ZRL count), lane 0 codes the DC difference, the last nonzero lane appends EOB;
//       each lane's fields fit in 63 bits.  A wave sum gives the block's bit length.
//   (3) jpeg_scan_kernel : per frame, an exclusive scan of the block lengths -> bit offsets and the frame's bit count.
//   (4) jpeg_bits_kernel<true> : the same fields again, each lane ORs its bits at block offset + lane prefix into a
//       zeroed big-endian 64-bit word buffer (atomicOr commutes: the result does not depend on scheduling).
//   (5) jpeg_count_kernel : per frame, the 0xFF bytes of the data (last byte padded with 1-bits) -> file length.
//   (6) jpeg_scan_kernel : an exclusive scan of the file lengths -> file offsets in the packed output.
//   (7) jpeg_emit_kernel : per frame, header, the data with 0x00 after every 0xFF (a block scan of the 0xFF counts of
//       16-byte runs), EOI.
// No inter-workgroup waits anywhere.  Bounds: the output capacity is checked against n * max_frame_bytes on the host,
// and max_frame_bytes bounds every file (see the header), so no kernel can write past its buffers.
#include "../../include/sdfa_jpeg.h"
#include "../../include/sdfa_hip.h"
#include "host.h"
#include "kernels.h"

#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>
#include <vector>

namespace {

constexpr int MCUS_PER_WG = 8;                    // transform: 8 MCUs x 6 blocks x 8 lanes = 384 threads
constexpr int TF_THREADS = MCUS_PER_WG * 6 * 8;
constexpr int SCAN_THREADS = 1024;
constexpr int EMIT_RUN = 16;                      // bytes per thread and pass of the count / emit kernels

struct QuantDiv {
    int div[2][64];                               // 8 * quant table, natural order; [0] luma, [1] chroma
};

// Huffman code words: (length << 16) | code, length 0 for an absent symbol.
struct HuffTables {
    uint32_t dc[2][16];
    uint32_t ac[2][256];
};

__constant__ int kNaturalToZigzag[64] = {
    0, 1, 5, 6, 14, 15, 27, 28, 2, 4, 7, 13, 16, 26, 29, 42, 3, 8, 12, 17, 25, 30, 41, 43, 9, 11, 18, 24, 31, 40, 44, 53,
    10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};

const int kZigzag[64] = {
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55,
    62, 63};

// T.81 Annex K.1 / K.2 (natural order) and K.3 (code lengths, symbols).
const int kLumaQ[64] = {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                        14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                        49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
const int kChromaQ[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                          47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                          99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
const uint8_t kDcLumaBits[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
const uint8_t kDcChromaBits[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
const uint8_t kDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
const uint8_t kAcLumaBits[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d};
const uint8_t kAcLumaVals[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32,
    0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16,
    0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45,
    0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
    0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94,
    0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6,
    0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8,
    0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
    0xf9, 0xfa};
const uint8_t kAcChromaBits[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77};
const uint8_t kAcChromaVals[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81,
    0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34,
    0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44,
    0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68,
    0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92,
    0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4,
    0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
    0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
    0xf9, 0xfa};

struct Geometry {
    int W, H;
    int mcx, mcy;                                 // MCU columns, rows
    int bw, bh;                                   // luma blocks across / down inside the image
    int hc;                                       // chroma rows inside the (even-padded) image: ceil(H / 2)
    int nmcu;
};

// ---- (1) transform ----

__device__ __forceinline__ int luma(const uint8_t *p) {
    return (19595 * p[0] + 38470 * p[1] + 7471 * p[2] + 32768) >> 16;
}
__device__ __forceinline__ int chroma(const uint8_t *p, int cr) {
    return cr ? (32768 * p[0] - 27439 * p[1] - 5329 * p[2] + (128 << 16) + 32767) >> 16
              : (-11059 * p[0] - 21709 * p[1] + 32768 * p[2] + (128 << 16) + 32767) >> 16;
}

// One islow pass over d[0..7] in place: FIRST scales by 2^PASS1_BITS, the second pass removes it (outputs x 8).
template <bool FIRST>
__device__ __forceinline__ void fdct8(int d[8]) {
    constexpr int CB = 13, P1 = 2, SH = FIRST ? CB - P1 : CB + P1;
    const int tmp0 = d[0] + d[7], tmp7 = d[0] - d[7], tmp1 = d[1] + d[6], tmp6 = d[1] - d[6];
    const int tmp2 = d[2] + d[5], tmp5 = d[2] - d[5], tmp3 = d[3] + d[4], tmp4 = d[3] - d[4];
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    auto ds = [](int x, int n) { return (x + (1 << (n - 1))) >> n; };
    if (FIRST) {
        d[0] = (tmp10 + tmp11) << P1;
        d[4] = (tmp10 - tmp11) << P1;
    } else {
        d[0] = ds(tmp10 + tmp11, P1);
        d[4] = ds(tmp10 - tmp11, P1);
    }
    int z1 = (tmp12 + tmp13) * 4433;
    d[2] = ds(z1 + tmp13 * 6270, SH);
    d[6] = ds(z1 - tmp12 * 15137, SH);
    z1 = tmp4 + tmp7;
    int z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
    const int z5 = (z3 + z4) * 9633;
    const int t4 = tmp4 * 2446, t5 = tmp5 * 16819, t6 = tmp6 * 25172, t7 = tmp7 * 12299;
    z1 = -z1 * 7373;
    z2 = -z2 * 20995;
    z3 = -z3 * 16069 + z5;
    z4 = -z4 * 3196 + z5;
    d[7] = ds(t4 + z1 + z3, SH);
    d[5] = ds(t5 + z2 + z4, SH);
    d[3] = ds(t6 + z2 + z3, SH);
    d[1] = ds(t7 + z1 + z4, SH);
}

// Luma blocks of an MCU that lie outside the image take the DC of the block before them (sdfa_jpeg.h); -1: a real block.
__device__ __forceinline__ int dummy_source(const Geometry &g, int mx, int my, int b) {
    if (b >= 4) return -1;
    const bool right = 2 * mx + 1 >= g.bw, bottom = 2 * my + 1 >= g.bh;
    const int y01 = right ? 0 : 1;
    switch (b) {
        case 1: return right ? 0 : -1;
        case 2: return bottom ? y01 : -1;
        case 3: return bottom ? y01 : (right ? 2 : -1);
        default: return -1;
    }
}

__global__ void __launch_bounds__(TF_THREADS) jpeg_transform_kernel(const uint8_t *__restrict__ rgb, Geometry g, QuantDiv q,
                                                                    int16_t *__restrict__ coefs) {
    __shared__ int rows[MCUS_PER_WG * 6][8][9];   // [block][row][column], padded
    __shared__ int dcs[MCUS_PER_WG * 6];
    const int t = threadIdx.x, lb = t >> 3, lane = t & 7;
    const int mcu = blockIdx.x * MCUS_PER_WG + lb / 6, b = lb % 6;
    const int64_t f = blockIdx.y;
    const bool live = mcu < g.nmcu;
    const int mx = live ? mcu % g.mcx : 0, my = live ? mcu / g.mcx : 0;
    const uint8_t *img = rgb + f * g.H * (int64_t)g.W * 3;
    int d[8];
    if (live) {
        if (b < 4) {                                              // luma row: edge replication
            const int y = min(16 * my + 8 * (b >> 1) + lane, g.H - 1);
            const uint8_t *row = img + (int64_t)y * g.W * 3;
            const int x0 = 16 * mx + 8 * (b & 1);
#pragma unroll
            for (int c = 0; c < 8; ++c) d[c] = luma(row + 3 * min(x0 + c, g.W - 1)) - 128;
        } else {                                                  // chroma row: 2 x 2 average, bias 1, 2, 1, 2, ...
            const int cy = min(8 * my + lane, g.hc - 1);
            const uint8_t *r0 = img + (int64_t)(2 * cy) * g.W * 3;
            const uint8_t *r1 = img + (int64_t)min(2 * cy + 1, g.H - 1) * g.W * 3;
            const int cr = b - 4;
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const int cx = 8 * mx + c;
                const int xa = 3 * min(2 * cx, g.W - 1), xb = 3 * min(2 * cx + 1, g.W - 1);
                d[c] = ((chroma(r0 + xa, cr) + chroma(r0 + xb, cr) + chroma(r1 + xa, cr) + chroma(r1 + xb, cr) + 1 + (c & 1)) >> 2) - 128;
            }
        }
        fdct8<true>(d);
#pragma unroll
        for (int c = 0; c < 8; ++c) rows[lb][lane][c] = d[c];
    }
    __syncthreads();
    const int src = live ? dummy_source(g, mx, my, b) : -1;
    int16_t *out = coefs + ((f * g.nmcu + (live ? mcu : 0)) * 6 + b) * 64;
    if (live) {
#pragma unroll
        for (int r = 0; r < 8; ++r) d[r] = rows[lb][r][lane];
        fdct8<false>(d);
        const int *div = q.div[b < 4 ? 0 : 1];
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int nat = 8 * r + lane, dv = div[nat];
            const int a = (abs(d[r]) + (dv >> 1)) / dv;
            const int v = d[r] < 0 ? -a : a;
            if (nat == 0) dcs[lb] = v;
            out[kNaturalToZigzag[nat]] = (int16_t)(src >= 0 ? 0 : v);
        }
    }
    __syncthreads();
    if (live && src >= 0 && lane == 0) out[0] = (int16_t)dcs[lb - b + src];
}

// ---- (2), (4) entropy coding: one wave per block, one lane per coefficient ----

__device__ __forceinline__ int bit_size(int v) {
    const unsigned a = (unsigned)abs(v);
    return a ? 32 - __clz(a) : 0;
}

// The fields of coefficient `k` of block `blk` (frame-relative): appended MSB first into *bits, *nbits <= 63.
__device__ __forceinline__ void lane_fields(const int16_t *__restrict__ fc, int64_t blk, int k, const HuffTables &ht,
                                            uint64_t &bits, int &nbits) {
    const int16_t *c = fc + blk * 64;
    const int b = (int)(blk % 6);
    const int tab = b < 4 ? 0 : 1;
    const int v = c[k];
    const uint64_t nzmask = __ballot(k > 0 && v != 0);
    bits = 0;
    nbits = 0;
    auto put = [&](uint32_t cw) {
        const int len = cw >> 16;
        bits = (bits << len) | (cw & 0xffffu);
        nbits += len;
    };
    auto put_raw = [&](uint32_t val, int len) {
        bits = (bits << len) | (val & ((1u << len) - 1u));
        nbits += len;
    };
    const int last = nzmask ? 63 - __clzll(nzmask) : 0;
    if (k == 0) {
        int64_t prev_blk = -1;
        if (b == 1 || b == 2 || b == 3) prev_blk = blk - 1;
        else if (blk >= 6) prev_blk = b == 0 ? blk - 3 : blk - 6;
        const int diff = v - (prev_blk >= 0 ? fc[prev_blk * 64] : 0);
        const int s = min(bit_size(diff), 15);
        put(ht.dc[tab][s]);
        put_raw(diff < 0 ? diff - 1 : diff, s);
    } else if (v != 0) {
        const uint64_t below = nzmask & ((1ull << k) - 1ull);
        const int p = below ? 63 - __clzll(below) : 0;
        int run = k - p - 1;
        for (; run >= 16; run -= 16) put(ht.ac[tab][0xf0]);
        const int s = min(bit_size(v), 15);
        put(ht.ac[tab][(run << 4) | s]);
        put_raw(v < 0 ? v - 1 : v, s);
    }
    if (k == last && last < 63) put(ht.ac[tab][0x00]);
}

__device__ __forceinline__ void or_bits(unsigned long long *__restrict__ words, int64_t pos, uint64_t bits, int nbits) {
    const int64_t w = pos >> 6;
    const int off = (int)(pos & 63), end = off + nbits;
    if (end <= 64) {
        atomicOr(words + w, (unsigned long long)(bits << (64 - end)));
    } else {
        atomicOr(words + w, (unsigned long long)(bits >> (end - 64)));
        atomicOr(words + w + 1, (unsigned long long)(bits << (128 - end)));
    }
}

template <bool PACK>
__global__ void __launch_bounds__(256) jpeg_bits_kernel(const int16_t *__restrict__ coefs, int64_t nblk,
                                                        const HuffTables *__restrict__ ht_g, int *__restrict__ blen,
                                                        const int64_t *__restrict__ boff, unsigned long long *__restrict__ words,
                                                        int64_t cap_words) {
    const int k = threadIdx.x & 63;
    const int64_t blk = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t f = blockIdx.y;
    if (blk >= nblk) return;                                      // whole waves only: 4 blocks per workgroup
    uint64_t bits;
    int nbits;
    lane_fields(coefs + f * nblk * 64, blk, k, *ht_g, bits, nbits);
    if (!PACK) {
        int s = nbits;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
        if (k == 0) blen[f * nblk + blk] = s;
    } else {
        int pre = nbits;                                          // inclusive prefix over the lanes
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int u = __shfl_up(pre, o, 64);
            if (k >= o) pre += u;
        }
        if (nbits) or_bits(words + f * cap_words, boff[f * nblk + blk] + pre - nbits, bits, nbits);
    }
}

// ---- (3), (6) exclusive scans, one workgroup per segment ----

template <typename T>
__global__ void __launch_bounds__(SCAN_THREADS) jpeg_scan_kernel(const T *__restrict__ in, int64_t len,
                                                                 int64_t *__restrict__ out, int64_t *__restrict__ totals) {
    __shared__ int64_t part[SCAN_THREADS];
    const int t = threadIdx.x;
    const int64_t seg = blockIdx.x;
    const T *x = in + seg * len;
    int64_t *y = out + seg * len;
    const int64_t per = (len + SCAN_THREADS - 1) / SCAN_THREADS;
    const int64_t lo = min(len, t * per), hi = min(len, lo + per);
    int64_t s = 0;
    for (int64_t i = lo; i < hi; ++i) s += x[i];
    part[t] = s;
    __syncthreads();
    for (int o = 1; o < SCAN_THREADS; o <<= 1) {                  // Hillis-Steele, inclusive
        const int64_t u = t >= o ? part[t - o] : 0;
        __syncthreads();
        part[t] += u;
        __syncthreads();
    }
    int64_t run = part[t] - s;
    for (int64_t i = lo; i < hi; ++i) {
        const int64_t v = x[i];
        y[i] = run;
        run += v;
    }
    if (t == SCAN_THREADS - 1 && totals) totals[seg] = part[t];
}

// ---- (5), (7) byte stuffing and assembly ----

__device__ __forceinline__ int data_byte(const unsigned long long *__restrict__ words, int64_t i, int64_t nbits) {
    int v = (int)((words[i >> 3] >> (56 - 8 * (i & 7))) & 0xff);
    const int64_t tail = nbits - 8 * i;                           // bits of this byte that are data
    if (tail < 8) v |= 0xff >> tail;                              // pad with 1-bits
    return v;
}

__device__ int64_t block_sum(int64_t v, int64_t *red) {
    const int t = threadIdx.x;
    red[t] = v;
    __syncthreads();
    for (int o = SCAN_THREADS / 2; o > 0; o >>= 1) {
        if (t < o) red[t] += red[t + o];
        __syncthreads();
    }
    const int64_t s = red[0];
    __syncthreads();
    return s;
}

__global__ void __launch_bounds__(SCAN_THREADS) jpeg_count_kernel(const unsigned long long *__restrict__ words, int64_t cap_words,
                                                                  const int64_t *__restrict__ fbits, int64_t hdr_len,
                                                                  int64_t *__restrict__ lengths) {
    __shared__ int64_t red[SCAN_THREADS];
    const int64_t f = blockIdx.x, nbits = fbits[f], nbytes = (nbits + 7) >> 3;
    const unsigned long long *w = words + f * cap_words;
    int64_t ff = 0;
    for (int64_t i = threadIdx.x; i < nbytes; i += SCAN_THREADS) ff += data_byte(w, i, nbits) == 0xff;
    ff = block_sum(ff, red);
    if (threadIdx.x == 0) lengths[f] = hdr_len + nbytes + ff + 2;
}

__global__ void __launch_bounds__(SCAN_THREADS) jpeg_emit_kernel(const unsigned long long *__restrict__ words, int64_t cap_words,
                                                                 const int64_t *__restrict__ fbits, const uint8_t *__restrict__ hdr,
                                                                 int64_t hdr_len, const int64_t *__restrict__ offsets,
                                                                 const int64_t *__restrict__ lengths, uint8_t *__restrict__ out) {
    __shared__ int part[SCAN_THREADS];
    const int t = threadIdx.x;
    const int64_t f = blockIdx.x, nbits = fbits[f], nbytes = (nbits + 7) >> 3;
    const unsigned long long *w = words + f * cap_words;
    uint8_t *dst = out + offsets[f];
    for (int64_t i = t; i < hdr_len; i += SCAN_THREADS) dst[i] = hdr[i];
    dst += hdr_len;
    int64_t carry = 0;                                            // stuffed bytes before this pass
    for (int64_t base = 0; base < nbytes; base += (int64_t)SCAN_THREADS * EMIT_RUN) {
        const int64_t lo = base + (int64_t)t * EMIT_RUN;
        int v[EMIT_RUN];
        int n_ff = 0;
#pragma unroll
        for (int j = 0; j < EMIT_RUN; ++j) {
            v[j] = lo + j < nbytes ? data_byte(w, lo + j, nbits) : -1;
            n_ff += v[j] == 0xff;
        }
        part[t] = n_ff;
        __syncthreads();
        for (int o = 1; o < SCAN_THREADS; o <<= 1) {
            const int u = t >= o ? part[t - o] : 0;
            __syncthreads();
            part[t] += u;
            __syncthreads();
        }
        int64_t at = lo + carry + (part[t] - n_ff);
#pragma unroll
        for (int j = 0; j < EMIT_RUN; ++j) {
            if (v[j] < 0) break;
            dst[at++] = (uint8_t)v[j];
            if (v[j] == 0xff) dst[at++] = 0;
        }
        carry += part[SCAN_THREADS - 1];
        __syncthreads();
    }
    if (t == 0) {
        const int64_t end = lengths[f] - hdr_len;                 // = nbytes + 0xFF count + 2
        dst[end - 2] = 0xff;
        dst[end - 1] = 0xd9;
    }
}

}  // namespace

struct sdfa_jpeg_encoder {
    Geometry g;
    int quality;
    QuantDiv q;
    std::vector<uint8_t> header;
    uint8_t *d_header = nullptr;
    HuffTables *d_huff = nullptr;
    int64_t nblk = 0, cap_words = 0, max_frame_bytes = 0;
};

namespace {

struct Layout {
    int64_t coefs, blen, boff, fbits, words, total;
};

Layout layout(const sdfa_jpeg_encoder *e, int64_t n) {
    Layout l{};
    l.coefs = 0;
    l.blen = l.coefs + round_up(n * e->nblk * 64 * 2, 256);
    l.boff = l.blen + round_up(n * e->nblk * 4, 256);
    l.fbits = l.boff + round_up(n * e->nblk * 8, 256);
    l.words = l.fbits + round_up(n * 8, 256);
    l.total = l.words + round_up(n * e->cap_words * 8, 256);
    return l;
}

void huff_codes(const uint8_t bits[16], const uint8_t *vals, uint32_t *table) {
    uint32_t code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < bits[len - 1]; ++i) table[vals[k++]] = ((uint32_t)len << 16) | code++;
        code <<= 1;
    }
}

void segment(std::vector<uint8_t> &h, uint8_t marker, const std::vector<uint8_t> &body) {
    const size_t len = body.size() + 2;
    h.insert(h.end(), {0xff, marker, (uint8_t)(len >> 8), (uint8_t)len});
    h.insert(h.end(), body.begin(), body.end());
}

std::vector<uint8_t> with(std::vector<uint8_t> v, const uint8_t *a, int n) {
    v.insert(v.end(), a, a + n);
    return v;
}

int check_rgb(const sdfa_jpeg_encoder *e, const uint8_t *d_rgb, int64_t n, const char *who) {
    if (!e) return sdfa_fail(SDFA_EINVAL, "%s: null encoder", who);
    if (n < 0 || n > SDFA_JPEG_MAX_FRAMES) return sdfa_fail(SDFA_EINVAL, "%s: frame count %lld outside 0 .. %d", who, (long long)n, SDFA_JPEG_MAX_FRAMES);
    if (n > 0 && !d_rgb) return sdfa_fail(SDFA_EINVAL, "%s: null input", who);
    return SDFA_OK;
}

int launch_transform(const sdfa_jpeg_encoder *e, const uint8_t *d_rgb, int64_t n, int16_t *coefs, hipStream_t s) {
    const dim3 grid((unsigned)((e->g.nmcu + MCUS_PER_WG - 1) / MCUS_PER_WG), (unsigned)n);
    hipLaunchKernelGGL(jpeg_transform_kernel, grid, dim3(TF_THREADS), 0, s, d_rgb, e->g, e->q, coefs);
    HIP_TRY(hipGetLastError());
    return SDFA_OK;
}

}  // namespace

extern "C" {

int sdfa_jpeg_abi_version(void) { return SDFA_JPEG_ABI_VERSION; }

sdfa_jpeg_encoder *sdfa_jpeg_create(int width, int height, int quality, void *stream) {
    if (width < 1 || height < 1 || width > SDFA_JPEG_MAX_SIDE || height > SDFA_JPEG_MAX_SIDE) {
        sdfa_fail(SDFA_EINVAL, "jpeg_create: image size %d x %d outside 1 .. %d", width, height, SDFA_JPEG_MAX_SIDE);
        return nullptr;
    }
    if (quality < 1 || quality > 100) { sdfa_fail(SDFA_EINVAL, "jpeg_create: quality %d outside 1 .. 100", quality); return nullptr; }
    sdfa_jpeg_encoder *e = new sdfa_jpeg_encoder();
    Geometry &g = e->g;
    g.W = width; g.H = height;
    g.mcx = (width + 15) / 16; g.mcy = (height + 15) / 16;
    g.bw = (width + 7) / 8; g.bh = (height + 7) / 8;
    g.hc = (height + 1) / 2;
    g.nmcu = g.mcx * g.mcy;
    e->quality = quality;
    e->nblk = 6 * (int64_t)g.nmcu;
    e->cap_words = (e->nblk * SDFA_JPEG_MAX_BLOCK_BITS + 63) / 64 + 1;

    // quantisation: libjpeg's quality scaling, clamped to baseline
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    uint8_t qt[2][64];
    for (int t = 0; t < 2; ++t)
        for (int i = 0; i < 64; ++i) {
            int v = ((t ? kChromaQ : kLumaQ)[i] * scale + 50) / 100;
            v = v < 1 ? 1 : (v > 255 ? 255 : v);
            qt[t][i] = (uint8_t)v;
            e->q.div[t][i] = 8 * v;
        }

    std::vector<uint8_t> &h = e->header;
    h = {0xff, 0xd8};
    segment(h, 0xe0, {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0});
    for (int t = 0; t < 2; ++t) {
        std::vector<uint8_t> body{(uint8_t)t};
        for (int k = 0; k < 64; ++k) body.push_back(qt[t][kZigzag[k]]);
        segment(h, 0xdb, body);
    }
    segment(h, 0xc0, {8, (uint8_t)(height >> 8), (uint8_t)height, (uint8_t)(width >> 8), (uint8_t)width, 3, 1, 0x22, 0, 2,
                      0x11, 1, 3, 0x11, 1});
    segment(h, 0xc4, with(with({0x00}, kDcLumaBits, 16), kDcVals, 12));
    segment(h, 0xc4, with(with({0x10}, kAcLumaBits, 16), kAcLumaVals, 162));
    segment(h, 0xc4, with(with({0x01}, kDcChromaBits, 16), kDcVals, 12));
    segment(h, 0xc4, with(with({0x11}, kAcChromaBits, 16), kAcChromaVals, 162));
    segment(h, 0xda, {3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0});
    e->max_frame_bytes = (int64_t)h.size() + 2 * ((e->nblk * SDFA_JPEG_MAX_BLOCK_BITS + 7) / 8 + 1) + 2;

    HuffTables ht;
    memset(&ht, 0, sizeof(ht));
    huff_codes(kDcLumaBits, kDcVals, ht.dc[0]);
    huff_codes(kDcChromaBits, kDcVals, ht.dc[1]);
    huff_codes(kAcLumaBits, kAcLumaVals, ht.ac[0]);
    huff_codes(kAcChromaBits, kAcChromaVals, ht.ac[1]);

    hipStream_t s = (hipStream_t)stream;
    auto bail = [&](const char *what, hipError_t err) -> sdfa_jpeg_encoder * {
        sdfa_fail(SDFA_EHIP, "jpeg_create: %s failed: %s", what, hipGetErrorString(err));
        sdfa_jpeg_destroy(e);
        return nullptr;
    };
    hipError_t err;
    if ((err = hipMalloc(&e->d_header, h.size())) != hipSuccess) return bail("hipMalloc", err);
    if ((err = hipMalloc(&e->d_huff, sizeof(HuffTables))) != hipSuccess) return bail("hipMalloc", err);
    if ((err = hipMemcpyAsync(e->d_header, h.data(), h.size(), hipMemcpyHostToDevice, s)) != hipSuccess) return bail("hipMemcpyAsync", err);
    if ((err = hipMemcpyAsync(e->d_huff, &ht, sizeof(ht), hipMemcpyHostToDevice, s)) != hipSuccess) return bail("hipMemcpyAsync", err);
    if ((err = hipStreamSynchronize(s)) != hipSuccess) return bail("hipStreamSynchronize", err);
    return e;
}

void sdfa_jpeg_destroy(sdfa_jpeg_encoder *e) {
    if (!e) return;
    if (e->d_header) (void)hipFree(e->d_header);
    if (e->d_huff) (void)hipFree(e->d_huff);
    delete e;
}

int64_t sdfa_jpeg_header(const sdfa_jpeg_encoder *e, uint8_t *h_out, int64_t capacity) {
    if (!e || capacity < 0) return sdfa_fail(SDFA_EINVAL, "jpeg_header: bad argument");
    const int64_t len = (int64_t)e->header.size();
    if (h_out) memcpy(h_out, e->header.data(), (size_t)(capacity < len ? capacity : len));
    return len;
}

int64_t sdfa_jpeg_max_frame_bytes(const sdfa_jpeg_encoder *e) {
    if (!e) return sdfa_fail(SDFA_EINVAL, "jpeg_max_frame_bytes: null encoder");
    return e->max_frame_bytes;
}

int64_t sdfa_jpeg_workspace_bytes(const sdfa_jpeg_encoder *e, int64_t n) {
    if (!e || n < 0) return sdfa_fail(SDFA_EINVAL, "jpeg_workspace_bytes: bad argument");
    return layout(e, n).total;
}

int sdfa_jpeg_encode(sdfa_jpeg_encoder *e, const uint8_t *d_rgb, int64_t n, uint8_t *d_out, int64_t out_capacity,
                     int64_t *d_offsets, int64_t *d_lengths, void *d_ws, int64_t ws_bytes, void *stream) {
    int rc = check_rgb(e, d_rgb, n, "jpeg_encode");
    if (rc < 0 || n == 0) return rc;
    if (!d_out || !d_offsets || !d_lengths || !d_ws) return sdfa_fail(SDFA_EINVAL, "jpeg_encode: null pointer");
    if (out_capacity < n * e->max_frame_bytes)
        return sdfa_fail(SDFA_ENOSPACE, "jpeg_encode: output of %lld bytes, %lld frames need %lld", (long long)out_capacity, (long long)n,
                    (long long)(n * e->max_frame_bytes));
    if ((uintptr_t)d_ws & 255) return sdfa_fail(SDFA_EINVAL, "jpeg_encode: workspace must be 256-byte aligned");
    const Layout l = layout(e, n);
    if (ws_bytes < l.total)
        return sdfa_fail(SDFA_ENOSPACE, "jpeg_encode: workspace of %lld bytes, %lld needed for %lld frames", (long long)ws_bytes,
                    (long long)l.total, (long long)n);
    hipStream_t s = (hipStream_t)stream;
    char *ws = (char *)d_ws;
    int16_t *coefs = (int16_t *)(ws + l.coefs);
    int *blen = (int *)(ws + l.blen);
    int64_t *boff = (int64_t *)(ws + l.boff), *fbits = (int64_t *)(ws + l.fbits);
    unsigned long long *words = (unsigned long long *)(ws + l.words);
    const int64_t hdr_len = (int64_t)e->header.size();

    HIP_TRY(hipMemsetAsync(words, 0, (size_t)(n * e->cap_words * 8), s));
    if ((rc = launch_transform(e, d_rgb, n, coefs, s)) < 0) return rc;
    const dim3 gb((unsigned)((e->nblk + 3) / 4), (unsigned)n);
    hipLaunchKernelGGL(jpeg_bits_kernel<false>, gb, dim3(256), 0, s, coefs, e->nblk, e->d_huff, blen, nullptr, nullptr, e->cap_words);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(jpeg_scan_kernel<int>, dim3((unsigned)n), dim3(SCAN_THREADS), 0, s, blen, e->nblk, boff, fbits);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(jpeg_bits_kernel<true>, gb, dim3(256), 0, s, coefs, e->nblk, e->d_huff, nullptr, boff, words, e->cap_words);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(jpeg_count_kernel, dim3((unsigned)n), dim3(SCAN_THREADS), 0, s, words, e->cap_words, fbits, hdr_len, d_lengths);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(jpeg_scan_kernel<int64_t>, dim3(1), dim3(SCAN_THREADS), 0, s, d_lengths, n, d_offsets, nullptr);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(jpeg_emit_kernel, dim3((unsigned)n), dim3(SCAN_THREADS), 0, s, words, e->cap_words, fbits, e->d_header,
                       hdr_len, d_offsets, d_lengths, d_out);
    HIP_TRY(hipGetLastError());
    return SDFA_OK;
}

int sdfa_jpeg_debug_coefs(sdfa_jpeg_encoder *e, const uint8_t *d_rgb, int64_t n, int16_t *d_coefs, void *stream) {
    int rc = check_rgb(e, d_rgb, n, "jpeg_debug_coefs");
    if (rc < 0 || n == 0) return rc;
    if (!d_coefs) return sdfa_fail(SDFA_EINVAL, "jpeg_debug_coefs: null output");
    return launch_transform(e, d_rgb, n, d_coefs, (hipStream_t)stream);
}

}  // extern "C"
