// Vertices on the device -> the vertex block of a Wavefront OBJ file ("v X Y Z\n" per vertex, "{:.6f}" numbers), batched
// over frames, byte for byte what speech_anime.viewer.write_obj writes; and the face block ("f a b c\n"), on the host.
//
// The format contract -- float32 bits -> correctly rounded six-decimal text, the domain, the per-frame flag -- is
// written down in include/sdfa_obj.h and DESIGN.md "OBJ text"; tests/obj_oracle.py restates it in integer Python.  All of
// it is integer arithmetic, so the bytes are exact.
//
// Four launches per call of n frames, a tile being 256 consecutive vertices of one frame and a thread one vertex:
//   (1) obj_length_kernel  : line lengths -> the tile's byte count and whether it holds a value outside the domain.
//   (2) obj_frame_kernel   : per frame, an exclusive scan of its tile counts -> tile offsets inside the block, the
//       block's length and the frame's flag.
//   (3) obj_offsets_kernel : an exclusive scan of the block lengths -> block offsets in the packed output.
//   (4) obj_format_kernel  : the digits again; a workgroup scan of the line lengths places every line of the tile in
//       LDS, shifted by the low four bits of the tile's global address, so that 16-byte LDS pieces line up with
//       16-byte aligned global ones: the tile goes out as uint4 stores, with byte stores only in its first and last
//       piece.  Block offsets are arbitrary byte addresses; nothing assumes more.
// No workgroup waits on another, no atomics.  Bounds: a line is at most 59 bytes (the header), so a tile fits its LDS
// buffer and a block its 59 * n_verts bytes; the output capacity is checked against n * 59 * n_verts on the host.  A value
// outside the domain is formatted as 0 (its frame is flagged and its bytes are not used), so it cannot widen a line.
#include "../../include/sdfa_obj.h"
#include "../../include/sdfa_hip.h"
#include "host.h"

#include <hip/hip_runtime.h>
#include <cstring>
#include <vector>

namespace {

constexpr int TILE = 256;                                  // vertices per workgroup = threads
constexpr int SCAN_THREADS = 1024;
constexpr int TILE_LDS = TILE * SDFA_OBJ_MAX_LINE_BYTES + 16;   // the tile's text, shifted by up to 15 bytes

// One number: Q = round-half-even(|x| * 10^6) split at the decimal point.
struct Num {
    uint32_t ip, fp;                                       // Q / 10^6 (< 2^31), Q % 10^6
    int neg, nd;                                           // sign bit; decimal digits of ip (1 .. 10)
};

__device__ __forceinline__ int int_digits(uint32_t v) {
    int d = 1;
    d += v >= 10u;
    d += v >= 100u;
    d += v >= 1000u;
    d += v >= 10000u;
    d += v >= 100000u;
    d += v >= 1000000u;
    d += v >= 10000000u;
    d += v >= 100000000u;
    d += v >= 1000000000u;
    return d;
}

// x * 10^6 = m * 15625 * 2^(e + 6) with m the significand and e its exponent: N = m * 15625 < 2^38, shifted by k = e + 6.
// `bad` is set for a value outside the domain (not finite, or |x| >= 2^31), which is then formatted as +-0.
__device__ __forceinline__ Num decode(uint32_t bits, int &bad) {
    const uint32_t E = (bits >> 23) & 0xffu, M = bits & 0x7fffffu;
    Num r;
    r.neg = (int)(bits >> 31);
    uint64_t Q = 0;
    if (E >= 158u) {
        bad = 1;
    } else {
        const uint64_t N = (uint64_t)(E ? (M | 0x800000u) : M) * 15625u;
        const int k = (E ? (int)E - 150 : -149) + 6;
        if (k >= 0) {
            Q = N << k;                                    // k <= 13: below 2^51
        } else if (k > -40) {
            const int sh = -k;
            const uint64_t rem = N & ((1ull << sh) - 1), half = 1ull << (sh - 1);
            Q = N >> sh;
            Q += (rem > half) | ((rem == half) & (Q & 1));
        }
    }
    const uint64_t ip = Q / 1000000u;
    r.ip = (uint32_t)ip;
    r.fp = (uint32_t)(Q - ip * 1000000u);
    r.nd = int_digits(r.ip);
    return r;
}

__device__ __forceinline__ int num_length(const Num &a) { return a.neg + a.nd + 7; }     // [-] digits . six digits

// The three numbers of vertex `v` of a frame and their line's length ("v " + three numbers + two blanks + "\n").
__device__ __forceinline__ int decode_vertex(const float *__restrict__ frame, int64_t v, Num a[3], int &bad) {
    int len = 5;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        a[c] = decode(__float_as_uint(frame[v * 3 + c]), bad);
        len += num_length(a[c]);
    }
    return len;
}

__device__ __forceinline__ int put_num(uint8_t *s, int p, const Num &a) {
    if (a.neg) s[p++] = '-';
    uint32_t v = a.ip;
    for (int i = a.nd - 1; i >= 0; --i) {
        const uint32_t q = v / 10u;
        s[p + i] = (uint8_t)('0' + (v - q * 10u));
        v = q;
    }
    p += a.nd;
    s[p] = '.';
    v = a.fp;
#pragma unroll
    for (int i = 6; i >= 1; --i) {
        const uint32_t q = v / 10u;
        s[p + i] = (uint8_t)('0' + (v - q * 10u));
        v = q;
    }
    return p + 7;
}

// Inclusive scan of one int per thread over the TILE threads of a workgroup; `wsum` holds TILE / 64 ints.
__device__ __forceinline__ int tile_scan(int x, int *wsum, int &total) {
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(x, o, 64);
        if (lane >= o) x += u;
    }
    if (lane == 63) wsum[w] = x;
    __syncthreads();
    int before = 0;
    total = 0;
#pragma unroll
    for (int i = 0; i < TILE / 64; ++i) {
        const int s = wsum[i];
        before += i < w ? s : 0;
        total += s;
    }
    return x + before;
}

// ---- (1) line lengths ----

__global__ void __launch_bounds__(TILE) obj_length_kernel(const float *__restrict__ verts, int64_t n_verts, uint32_t tiles,
                                                          int *__restrict__ tile_len, int *__restrict__ tile_bad) {
    __shared__ int wsum[TILE / 64], wbad[TILE / 64];
    const int t = threadIdx.x;
    const uint32_t fi = blockIdx.x / tiles;                // n * tiles < 2^31 (check_shape)
    const int64_t f = fi, v = (int64_t)(blockIdx.x - fi * tiles) * TILE + t;
    int len = 0, bad = 0;
    if (v < n_verts) {
        Num a[3];
        len = decode_vertex(verts + f * n_verts * 3, v, a, bad);
    }
    int total;
    tile_scan(len, wsum, total);
    const int any = __any(bad);
    if ((t & 63) == 0) wbad[t >> 6] = any;
    __syncthreads();
    if (t == 0) {
        tile_len[blockIdx.x] = total;
        tile_bad[blockIdx.x] = wbad[0] | wbad[1] | wbad[2] | wbad[3];
    }
}

// ---- (2), (3) exclusive scans ----

// Exclusive scan of x[0 .. len) into y by one workgroup (a run per thread, Hillis-Steele over the runs); returns the sum.
template <typename T>
__device__ int64_t segment_scan(const T *__restrict__ x, int64_t len, int64_t *__restrict__ y, int64_t *part) {
    const int t = threadIdx.x;
    const int64_t per = (len + SCAN_THREADS - 1) / SCAN_THREADS;
    const int64_t lo = min(len, t * per), hi = min(len, lo + per);
    int64_t s = 0;
    for (int64_t i = lo; i < hi; ++i) s += x[i];
    part[t] = s;
    __syncthreads();
    for (int o = 1; o < SCAN_THREADS; o <<= 1) {
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
    return part[SCAN_THREADS - 1];
}

__global__ void __launch_bounds__(SCAN_THREADS) obj_frame_kernel(const int *__restrict__ tile_len, const int *__restrict__ tile_bad,
                                                                 int64_t tiles, int64_t *__restrict__ tile_off,
                                                                 int64_t *__restrict__ lengths, int32_t *__restrict__ flags) {
    __shared__ int64_t part[SCAN_THREADS];
    const int64_t f = blockIdx.x;
    int bad = 0;
    for (int64_t i = threadIdx.x; i < tiles; i += SCAN_THREADS) bad |= tile_bad[f * tiles + i];
    const int any = __syncthreads_or(bad);
    const int64_t total = segment_scan(tile_len + f * tiles, tiles, tile_off + f * tiles, part);
    if (threadIdx.x == 0) {
        lengths[f] = total;
        flags[f] = any ? 1 : 0;
    }
}

__global__ void __launch_bounds__(SCAN_THREADS) obj_offsets_kernel(const int64_t *__restrict__ lengths, int64_t n,
                                                                   int64_t *__restrict__ offsets) {
    __shared__ int64_t part[SCAN_THREADS];
    segment_scan(lengths, n, offsets, part);
}

// ---- (4) the text ----

__global__ void __launch_bounds__(TILE) obj_format_kernel(const float *__restrict__ verts, int64_t n_verts, uint32_t tiles,
                                                          const int64_t *__restrict__ tile_off, const int64_t *__restrict__ offsets,
                                                          uint8_t *__restrict__ out) {
    __shared__ uint4 text4[TILE_LDS / 16];
    __shared__ int wsum[TILE / 64];
    uint8_t *text = (uint8_t *)text4;
    const int t = threadIdx.x;
    const uint32_t fi = blockIdx.x / tiles;                // n * tiles < 2^31 (check_shape)
    const int64_t f = fi, v = (int64_t)(blockIdx.x - fi * tiles) * TILE + t;
    uint8_t *dst = out + offsets[f] + tile_off[blockIdx.x];
    const int skew = (int)((uintptr_t)dst & 15);           // text[skew + i] is byte i of the tile: LDS and global agree mod 16

    Num a[3];
    int len = 0, bad = 0;
    if (v < n_verts) len = decode_vertex(verts + f * n_verts * 3, v, a, bad);
    int total;
    const int end = tile_scan(len, wsum, total);
    if (v < n_verts) {
        int p = skew + end - len;
        text[p] = 'v';
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            text[p + 1] = ' ';
            p = put_num(text, p + 2, a[c]) - 1;
        }
        text[p + 1] = '\n';
    }
    __syncthreads();

    uint8_t *base = dst - skew;                            // 16-byte aligned
    const int lo = skew, hi = skew + total;                // the tile's bytes in `text`
    for (int c = t; c * 16 < hi; c += TILE) {
        const int b0 = c * 16;
        if (b0 >= lo && b0 + 16 <= hi) {
            *(uint4 *)(base + b0) = text4[c];
        } else {
            for (int b = max(b0, lo); b < min(b0 + 16, hi); ++b) base[b] = text[b];
        }
    }
}

struct Layout {
    int64_t tile_len, tile_bad, tile_off, total;
};

Layout layout(int64_t tiles, int64_t n) {
    Layout l{};
    l.tile_len = 0;
    l.tile_bad = l.tile_len + round_up(n * tiles * 4, 256);
    l.tile_off = l.tile_bad + round_up(n * tiles * 4, 256);
    l.total = l.tile_off + round_up(n * tiles * 8, 256);
    return l;
}

// n_verts and n within what the launches index: n * tiles workgroups on grid.x, 59 * n_verts * n bytes in an int64.
int check_shape(int64_t n_verts, int64_t n, const char *who) {
    if (n_verts < 1 || n_verts > (1ll << 40)) return sdfa_fail(SDFA_EINVAL, "%s: vertex count %lld outside 1 .. 2^40", who, (long long)n_verts);
    if (n < 0) return sdfa_fail(SDFA_EINVAL, "%s: negative frame count %lld", who, (long long)n);
    const int64_t tiles = (n_verts + TILE - 1) / TILE;
    if (n > 0x7fffffffll / tiles)
        return sdfa_fail(SDFA_EINVAL, "%s: %lld frames of %lld vertices are more than 2^31 - 1 tiles of %d", who, (long long)n, (long long)n_verts, TILE);
    return SDFA_OK;
}

int index_digits(uint64_t v) {
    int d = 1;
    for (; v >= 10; v /= 10) ++d;
    return d;
}

}  // namespace

extern "C" {

int sdfa_obj_abi_version(void) { return SDFA_OBJ_ABI_VERSION; }

int64_t sdfa_obj_max_frame_bytes(int64_t n_verts) {
    if (n_verts < 0 || n_verts > (1ll << 40)) return sdfa_fail(SDFA_EINVAL, "obj_max_frame_bytes: vertex count %lld outside 0 .. 2^40", (long long)n_verts);
    return SDFA_OBJ_MAX_LINE_BYTES * n_verts;
}

int64_t sdfa_obj_workspace_bytes(int64_t n_verts, int64_t n) {
    const int rc = check_shape(n_verts, n, "obj_workspace_bytes");
    if (rc < 0) return rc;
    return layout((n_verts + TILE - 1) / TILE, n).total;
}

int sdfa_obj_format_verts(const float *d_verts, int64_t n, int64_t n_verts, uint8_t *d_out, int64_t out_capacity,
                          int64_t *d_offsets, int64_t *d_lengths, int32_t *d_flags, void *d_ws, int64_t ws_bytes, void *stream) {
    const int rc = check_shape(n_verts, n, "obj_format_verts");
    if (rc < 0 || n == 0) return rc;
    if (!d_verts || !d_out || !d_offsets || !d_lengths || !d_flags || !d_ws) return sdfa_fail(SDFA_EINVAL, "obj_format_verts: null pointer");
    const int64_t need = n * SDFA_OBJ_MAX_LINE_BYTES * n_verts;
    if (out_capacity < need)
        return sdfa_fail(SDFA_EINVAL, "obj_format_verts: output of %lld bytes, %lld frames of %lld vertices need %lld", (long long)out_capacity,
                         (long long)n, (long long)n_verts, (long long)need);
    if ((uintptr_t)d_ws & 255) return sdfa_fail(SDFA_EINVAL, "obj_format_verts: workspace must be 256-byte aligned");
    const int64_t tiles = (n_verts + TILE - 1) / TILE;
    const Layout l = layout(tiles, n);
    if (ws_bytes < l.total)
        return sdfa_fail(SDFA_EINVAL, "obj_format_verts: workspace of %lld bytes, %lld needed for %lld frames", (long long)ws_bytes,
                         (long long)l.total, (long long)n);
    hipStream_t s = (hipStream_t)stream;
    char *ws = (char *)d_ws;
    int *tile_len = (int *)(ws + l.tile_len), *tile_bad = (int *)(ws + l.tile_bad);
    int64_t *tile_off = (int64_t *)(ws + l.tile_off);
    const dim3 grid((unsigned)(n * tiles));

    hipLaunchKernelGGL(obj_length_kernel, grid, dim3(TILE), 0, s, d_verts, n_verts, (uint32_t)tiles, tile_len, tile_bad);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(obj_frame_kernel, dim3((unsigned)n), dim3(SCAN_THREADS), 0, s, tile_len, tile_bad, tiles, tile_off, d_lengths, d_flags);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(obj_offsets_kernel, dim3(1), dim3(SCAN_THREADS), 0, s, d_lengths, n, d_offsets);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(obj_format_kernel, grid, dim3(TILE), 0, s, d_verts, n_verts, (uint32_t)tiles, tile_off, d_offsets, d_out);
    HIP_TRY(hipGetLastError());
    return SDFA_OK;
}

int64_t sdfa_obj_format_faces(const uint32_t *h_faces, int64_t n_tris, int64_t n_verts, uint8_t *h_out, int64_t capacity) {
    if (n_tris < 0 || n_verts < 0 || capacity < 0 || (n_tris > 0 && !h_faces)) return sdfa_fail(SDFA_EINVAL, "obj_format_faces: bad argument");
    int64_t length = 0;
    for (int64_t i = 0; i < n_tris * 3; ++i) {
        if ((int64_t)h_faces[i] >= n_verts)
            return sdfa_fail(SDFA_EINVAL, "obj_format_faces: triangle %lld names vertex %u of %lld", (long long)(i / 3), h_faces[i], (long long)n_verts);
        length += index_digits((uint64_t)h_faces[i] + 1);
    }
    length += n_tris * 5;                                  // "f", three blanks, "\n"
    if (!h_out || capacity == 0) return length;
    std::vector<uint8_t> text((size_t)length);
    uint8_t *p = text.data();
    for (int64_t i = 0; i < n_tris; ++i) {
        *p++ = 'f';
        for (int c = 0; c < 3; ++c) {
            uint64_t v = (uint64_t)h_faces[i * 3 + c] + 1;
            const int d = index_digits(v);
            *p++ = ' ';
            for (int k = d - 1; k >= 0; --k, v /= 10) p[k] = (uint8_t)('0' + v % 10);
            p += d;
        }
        *p++ = '\n';
    }
    memcpy(h_out, text.data(), (size_t)(length < capacity ? length : capacity));
    return length;
}

}  // extern "C"
