// Last stage of evaluate: vertices of every video frame (on the device) -> RGB images, batched over frames.
//
// Reference: speech_anime/viewer/render_py.py (pyrender, one OpenGL draw per frame).  The rendering contract -- rig
// values, projection, snapping, fill rule, depth order, sampling, shading -- is written down in
// include/sdfa_render.h and DESIGN.md "Rendering"; tests/render_oracle.py restates the vertex and raster stages in
// numpy float32 bit for bit, so every function below that feeds them is compiled with fp contraction off and in
// the operation order written.
//
// Three kernels per call of n frames:
//   (1) render_vertex_kernel : one thread per (frame, vertex): camera-space position, snapped screen position, 1/w,
//       validity, camera-space unit normal (the template's, or a gather over the vertex -> face list of this frame);
//   (2) render_setup_kernel  : one thread per (frame, triangle): drop invalid / degenerate / back-facing triangles,
//       conservative pixel bounding box (int16) of the rest;
//   (3) render_raster_kernel : one 256-thread workgroup per (frame, 32 x 32 tile).  Triangles stream through in
//       blocks of 256 in index order: a bounding-box test, ballot + prefix compaction of the overlapping ones into an
//       LDS list (order kept), edge setup relative to the tile origin, then every lane tests its 4 pixels x S samples
//       against the list with exact int64 edge functions and keeps the nearest (1/w, triangle) per sample in
//       registers.  Then each sample is shaded, the samples averaged, and the tile's RGB staged in LDS and written
//       as dwords (96 bytes per tile row).  No atomics anywhere: the result is independent of scheduling.
#include "../../include/sdfa_render.h"
#include "../../include/sdfa_hip.h"
#include "host.h"
#include "kernels.h"

#include <hip/hip_runtime.h>
#include <climits>
#include <cmath>
#include <cstdio>
#include <vector>

namespace {

constexpr int TILE = SDFA_RENDER_TILE;
constexpr int NT = 256;                 // threads of the raster workgroup: 4 pixels of a 32 x 32 tile each
constexpr int ROWS_PER_PASS = NT / TILE;

struct VertexConsts {
    float s;                            // 0.15 / max|template|
    float m[12];                        // world -> camera, row-major 3 x 4
    float fx, fy;                       // projection
    float hw, hh;                       // W / 2, H / 2
    float znear, guard;
};

struct ShadeConsts {
    float ka[3], kd[3];                 // albedo * ambient, albedo / pi
    float dir_i, pt_i;
    float bg[3];
};

// Area-weighted vertex normal (world space, unit length; zero for a vertex without area): the sum over the incident
// faces, in ascending face order, of cross(p1 - p0, p2 - p0), p = s * v.  One function for the template (at create
// time) and for every frame, so normals="frame" on the template is normals="template" bit for bit.
__device__ __forceinline__ float3 vertex_normal(const float *__restrict__ v, const int *__restrict__ csr_off,
                                                const int *__restrict__ csr_face, const uint32_t *__restrict__ faces,
                                                float s, int vtx) {
#pragma clang fp contract(off)
    float nx = 0.f, ny = 0.f, nz = 0.f;
    for (int k = csr_off[vtx]; k < csr_off[vtx + 1]; ++k) {
        const int f = csr_face[k];
        const uint32_t a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
        const float ax = s * v[3 * a], ay = s * v[3 * a + 1], az = s * v[3 * a + 2];
        const float bx = s * v[3 * b], by = s * v[3 * b + 1], bz = s * v[3 * b + 2];
        const float cx = s * v[3 * c], cy = s * v[3 * c + 1], cz = s * v[3 * c + 2];
        const float e1x = bx - ax, e1y = by - ay, e1z = bz - az;
        const float e2x = cx - ax, e2y = cy - ay, e2z = cz - az;
        nx = nx + (e1y * e2z - e1z * e2y);
        ny = ny + (e1z * e2x - e1x * e2z);
        nz = nz + (e1x * e2y - e1y * e2x);
    }
    const float l2 = (nx * nx + ny * ny) + nz * nz;
    if (l2 > 0.f) {
        const float inv = 1.0f / sqrtf(l2);
        nx = nx * inv; ny = ny * inv; nz = nz * inv;
    }
    return make_float3(nx, ny, nz);
}

__global__ void render_normals_kernel(const float *__restrict__ verts, int V, const int *__restrict__ csr_off,
                                      const int *__restrict__ csr_face, const uint32_t *__restrict__ faces, float s,
                                      float4 *__restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= V) return;
    const float3 n = vertex_normal(verts, csr_off, csr_face, faces, s, i);
    out[i] = make_float4(n.x, n.y, n.z, 0.f);
}

__global__ void render_vertex_kernel(const float *__restrict__ verts, int64_t total, int V,
                                     const float4 *__restrict__ tmpl_nrm,     // null: normals of this frame
                                     const int *__restrict__ csr_off, const int *__restrict__ csr_face,
                                     const uint32_t *__restrict__ faces, VertexConsts k,
                                     int4 *__restrict__ scr, float4 *__restrict__ pos, float4 *__restrict__ nrm) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int64_t f = i / V;
    const int vtx = (int)(i - f * V);
    const float *vf = verts + f * V * 3;
    const float px = k.s * vf[3 * vtx], py = k.s * vf[3 * vtx + 1], pz = k.s * vf[3 * vtx + 2];
    const float cx = ((k.m[0] * px + k.m[1] * py) + k.m[2] * pz) + k.m[3];
    const float cy = ((k.m[4] * px + k.m[5] * py) + k.m[6] * pz) + k.m[7];
    const float cz = ((k.m[8] * px + k.m[9] * py) + k.m[10] * pz) + k.m[11];
    const float w = -cz;
    const float iw = 1.0f / w;
    const float X = ((cx * k.fx) * iw + 1.0f) * k.hw;
    const float Y = (1.0f - (cy * k.fy) * iw) * k.hh;
    const bool ok = isfinite(cx) && isfinite(cy) && isfinite(cz) && w > k.znear && fabsf(X) <= k.guard && fabsf(Y) <= k.guard;
    scr[i] = ok ? make_int4((int)rintf(X * 256.0f), (int)rintf(Y * 256.0f), __float_as_int(iw), 1) : make_int4(0, 0, 0, 0);
    pos[i] = make_float4(cx, cy, cz, 0.f);
    float3 n;
    if (tmpl_nrm) {
        const float4 t = tmpl_nrm[vtx];
        n = make_float3(t.x, t.y, t.z);
    } else {
        n = vertex_normal(vf, csr_off, csr_face, faces, k.s, vtx);
    }
    nrm[i] = make_float4((k.m[0] * n.x + k.m[1] * n.y) + k.m[2] * n.z, (k.m[4] * n.x + k.m[5] * n.y) + k.m[6] * n.z,
                         (k.m[8] * n.x + k.m[9] * n.y) + k.m[10] * n.z, 0.f);
}

// Edge function of the directed edge a -> b at p, all in 1/256 pixel (screen space, y down); positive inside a
// triangle that is counter-clockwise in NDC.  Exact in int64 (|coordinates| <= 2^23).
__device__ __forceinline__ int64_t edge_fn(int ax, int ay, int bx, int by, int px, int py) {
    return (int64_t)(by - ay) * (px - ax) - (int64_t)(bx - ax) * (py - ay);
}

__global__ void render_setup_kernel(const int4 *__restrict__ scr, const uint32_t *__restrict__ faces, int64_t total,
                                    int V, int T, int W, int H, short4 *__restrict__ box) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int64_t f = i / T;
    const int t = (int)(i - f * T);
    const int4 *sf = scr + f * V;
    const int4 p0 = sf[faces[3 * t]], p1 = sf[faces[3 * t + 1]], p2 = sf[faces[3 * t + 2]];
    short4 b = make_short4(1, 1, 0, 0);                                         // empty
    if (p0.w && p1.w && p2.w && edge_fn(p0.x, p0.y, p1.x, p1.y, p2.x, p2.y) > 0) {
        // a pixel's samples lie within [px*256 + 32, px*256 + 224]: this range is conservative
        const int x0 = max((min(min(p0.x, p1.x), p2.x) >> 8) - 1, 0), x1 = min(max(max(p0.x, p1.x), p2.x) >> 8, W - 1);
        const int y0 = max((min(min(p0.y, p1.y), p2.y) >> 8) - 1, 0), y1 = min(max(max(p0.y, p1.y), p2.y) >> 8, H - 1);
        if (x0 <= x1 && y0 <= y1) b = make_short4((short)x0, (short)y0, (short)x1, (short)y1);
    }
    box[i] = b;
}

// Sample offsets in 1/16 pixel: the pixel centre, or the standard 4x rotated grid.
template <int S> __device__ __forceinline__ int sample_dx(int s);
template <int S> __device__ __forceinline__ int sample_dy(int s);
template <> __device__ __forceinline__ int sample_dx<1>(int) { return 0; }
template <> __device__ __forceinline__ int sample_dy<1>(int) { return 0; }
template <> __device__ __forceinline__ int sample_dx<4>(int s) { return s == 0 ? -2 : s == 1 ? 6 : s == 2 ? -6 : 2; }
template <> __device__ __forceinline__ int sample_dy<4>(int s) { return s == 0 ? -6 : s == 1 ? -2 : s == 2 ? 2 : 6; }

// Colour of triangle t at sample (sx, sy) (1/256 pixel): perspective-correct normal and position, Lambert, clamped.
__device__ __forceinline__ float3 shade(int t, int sx, int sy, const uint32_t *__restrict__ faces, const int4 *__restrict__ sf,
                                       const float4 *__restrict__ pf, const float4 *__restrict__ nf, const ShadeConsts &c) {
#pragma clang fp contract(off)
    const uint32_t i0 = faces[3 * t], i1 = faces[3 * t + 1], i2 = faces[3 * t + 2];
    const int4 a = sf[i0], b = sf[i1], d = sf[i2];
    const float rD = 1.0f / (float)edge_fn(a.x, a.y, b.x, b.y, d.x, d.y);
    const float w0 = (float)edge_fn(b.x, b.y, d.x, d.y, sx, sy) * rD;
    const float w1 = (float)edge_fn(d.x, d.y, a.x, a.y, sx, sy) * rD;
    const float w2 = (float)edge_fn(a.x, a.y, b.x, b.y, sx, sy) * rD;
    const float q0 = w0 * __int_as_float(a.z), q1 = w1 * __int_as_float(b.z), q2 = w2 * __int_as_float(d.z);
    const float iz = 1.0f / ((q0 + q1) + q2);
    const float c0 = q0 * iz, c1 = q1 * iz, c2 = q2 * iz;
    const float4 n0 = nf[i0], n1 = nf[i1], n2 = nf[i2];
    const float4 p0 = pf[i0], p1 = pf[i1], p2 = pf[i2];
    float nx = (c0 * n0.x + c1 * n1.x) + c2 * n2.x, ny = (c0 * n0.y + c1 * n1.y) + c2 * n2.y, nz = (c0 * n0.z + c1 * n1.z) + c2 * n2.z;
    const float px = (c0 * p0.x + c1 * p1.x) + c2 * p2.x, py = (c0 * p0.y + c1 * p1.y) + c2 * p2.y, pz = (c0 * p0.z + c1 * p1.z) + c2 * p2.z;
    const float l2 = (nx * nx + ny * ny) + nz * nz;
    if (l2 > 0.f) {
        const float inv = 1.0f / sqrtf(l2);
        nx = nx * inv; ny = ny * inv; nz = nz * inv;
    }
    const float d2 = (px * px + py * py) + pz * pz;
    const float ndl_dir = fmaxf(nz, 0.f);                                       // light travels along -Z: toward it is +Z
    const float ndl_pt = fmaxf(-((nx * px + ny * py) + nz * pz) * (1.0f / sqrtf(d2)), 0.f);
    const float e = c.dir_i * ndl_dir + (c.pt_i * ndl_pt) / d2;
    return make_float3(fminf(fmaxf(c.ka[0] + c.kd[0] * e, 0.f), 1.f), fminf(fmaxf(c.ka[1] + c.kd[1] * e, 0.f), 1.f),
                       fminf(fmaxf(c.ka[2] + c.kd[2] * e, 0.f), 1.f));
}

struct RasterArgs {
    const int4 *scr;
    const float4 *pos, *nrm;
    const short4 *box;
    const uint32_t *faces;
    int V, T, W, H;
    int wide;                           // W % 4 == 0 and the output dword-aligned: full tiles are stored as dwords
    uint8_t *rgb;
    int32_t *ids;
    ShadeConsts sc;
};

template <int S>
__global__ __launch_bounds__(NT) void render_raster_kernel(RasterArgs a) {
#pragma clang fp contract(off)
    __shared__ int sA[3][NT], sB[3][NT], sBias[3][NT], sTri[NT];
    __shared__ int64_t sC[3][NT];
    __shared__ float sIw[3][NT], sRD[NT];
    __shared__ int sWave[NT / 64];
    __shared__ uint32_t sRGB[TILE * TILE * 3 / 4];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t f = blockIdx.z;
    const int tx0 = blockIdx.x * TILE, ty0 = blockIdx.y * TILE;
    const int ox = tx0 * 256, oy = ty0 * 256;               // tile origin, 1/256 pixel
    const int col = tid & (TILE - 1), row0 = tid / TILE;    // pixels (col, row0 + 8 k), k = 0..3
    const int4 *sf = a.scr + f * a.V;
    const short4 *bf = a.box + f * a.T;

    float best[4][S];
    int btri[4][S];
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int s = 0; s < S; ++s) { best[k][s] = -INFINITY; btri[k][s] = INT_MAX; }

    for (int base = 0; base < a.T; base += NT) {
        const int t = base + tid;
        bool hit = false;
        if (t < a.T) {
            const short4 b = bf[t];
            hit = b.x <= b.z && b.x <= tx0 + TILE - 1 && b.z >= tx0 && b.y <= ty0 + TILE - 1 && b.w >= ty0;
        }
        const uint64_t m = __ballot(hit);
        if (lane == 0) sWave[wave] = __popcll(m);
        __syncthreads();
        int off = 0, total = 0;
#pragma unroll
        for (int w = 0; w < NT / 64; ++w) { off += w < wave ? sWave[w] : 0; total += sWave[w]; }
        if (hit) {
            const int slot = off + __popcll(m & ((1ull << lane) - 1ull));
            const int4 p[3] = {sf[a.faces[3 * t]], sf[a.faces[3 * t + 1]], sf[a.faces[3 * t + 2]]};
#pragma unroll
            for (int e = 0; e < 3; ++e) {                   // edge e is opposite vertex e: (e+1) -> (e+2)
                const int4 u = p[(e + 1) % 3], v = p[(e + 2) % 3];
                const int dy = v.y - u.y, dx = v.x - u.x;
                sA[e][slot] = dy;
                sB[e][slot] = -dx;
                sC[e][slot] = edge_fn(u.x, u.y, v.x, v.y, ox, oy);
                sBias[e][slot] = (dy > 0 || (dy == 0 && dx < 0)) ? 0 : 1;   // top-left rule: F >= bias covers
                sIw[e][slot] = __int_as_float(p[e].z);
            }
            sRD[slot] = 1.0f / (float)edge_fn(p[0].x, p[0].y, p[1].x, p[1].y, p[2].x, p[2].y);
            sTri[slot] = t;
        }
        __syncthreads();
        for (int j = 0; j < total; ++j) {
            const int A0 = sA[0][j], A1 = sA[1][j], A2 = sA[2][j], B0 = sB[0][j], B1 = sB[1][j], B2 = sB[2][j];
            const int64_t C0 = sC[0][j], C1 = sC[1][j], C2 = sC[2][j];
            const int b0 = sBias[0][j], b1 = sBias[1][j], b2 = sBias[2][j];
            const float rD = sRD[j], iw0 = sIw[0][j], iw1 = sIw[1][j], iw2 = sIw[2][j];
            const int tri = sTri[j];
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int s = 0; s < S; ++s) {
                    const int dx = col * 256 + 128 + 16 * sample_dx<S>(s), dy = (row0 + ROWS_PER_PASS * k) * 256 + 128 + 16 * sample_dy<S>(s);
                    const int64_t F0 = C0 + (int64_t)A0 * dx + (int64_t)B0 * dy;
                    const int64_t F1 = C1 + (int64_t)A1 * dx + (int64_t)B1 * dy;
                    const int64_t F2 = C2 + (int64_t)A2 * dx + (int64_t)B2 * dy;
                    if (F0 >= b0 && F1 >= b1 && F2 >= b2) {
                        const float z = ((float)F0 * rD * iw0 + (float)F1 * rD * iw1) + (float)F2 * rD * iw2;
                        if (z > best[k][s] || (z == best[k][s] && tri < btri[k][s])) { best[k][s] = z; btri[k][s] = tri; }
                    }
                }
        }
        __syncthreads();
    }

    const float4 *pf = a.pos + f * a.V, *nf = a.nrm + f * a.V;
    uint8_t *lds_rgb = reinterpret_cast<uint8_t *>(sRGB);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int r = row0 + ROWS_PER_PASS * k, px = tx0 + col, py = ty0 + r;
        float3 acc = make_float3(0.f, 0.f, 0.f);
#pragma unroll
        for (int s = 0; s < S; ++s) {
            float3 c = make_float3(a.sc.bg[0], a.sc.bg[1], a.sc.bg[2]);
            if (btri[k][s] != INT_MAX)
                c = shade(btri[k][s], ox + col * 256 + 128 + 16 * sample_dx<S>(s), oy + r * 256 + 128 + 16 * sample_dy<S>(s),
                          a.faces, sf, pf, nf, a.sc);
            if (s == 0) acc = c;
            else acc = make_float3(acc.x + c.x, acc.y + c.y, acc.z + c.z);
        }
        if (S > 1) acc = make_float3(acc.x * (1.0f / S), acc.y * (1.0f / S), acc.z * (1.0f / S));
        const int li = (r * TILE + col) * 3;
        lds_rgb[li] = (uint8_t)rintf(acc.x * 255.0f);
        lds_rgb[li + 1] = (uint8_t)rintf(acc.y * 255.0f);
        lds_rgb[li + 2] = (uint8_t)rintf(acc.z * 255.0f);
        if (a.ids && px < a.W && py < a.H) a.ids[(f * a.H + py) * a.W + px] = btri[k][0] == INT_MAX ? -1 : btri[k][0];
    }
    __syncthreads();
    uint8_t *img = a.rgb + f * a.H * a.W * 3;
    if (a.wide && tx0 + TILE <= a.W) {
        // one tile row is 96 contiguous bytes = 24 dwords; 32 rows = 768 dwords = 3 per thread
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int d = tid + NT * j, r = d / 24, c = d - r * 24;
            if (ty0 + r < a.H)
                reinterpret_cast<uint32_t *>(img + ((int64_t)(ty0 + r) * a.W + tx0) * 3)[c] = sRGB[r * 24 + c];
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int r = row0 + ROWS_PER_PASS * k, px = tx0 + col, py = ty0 + r;
            if (px < a.W && py < a.H) {
                const int li = (r * TILE + col) * 3;
                uint8_t *o = img + ((int64_t)py * a.W + px) * 3;
                o[0] = lds_rgb[li]; o[1] = lds_rgb[li + 1]; o[2] = lds_rgb[li + 2];
            }
        }
    }
}

}  // namespace

struct sdfa_renderer {
    int64_t V = 0, T = 0;
    int W = 0, H = 0, samples = 4, normals = SDFA_RENDER_NORMALS_TEMPLATE;
    VertexConsts vc{};
    ShadeConsts sc{};
    uint32_t *d_faces = nullptr;
    int *d_csr_off = nullptr, *d_csr_face = nullptr;
    float4 *d_tmpl_nrm = nullptr;
};

namespace {

struct Layout {
    int64_t scr, pos, nrm, box, total;
};

Layout layout(const sdfa_renderer *r, int64_t n) {
    Layout l{};
    l.scr = 0;
    l.pos = l.scr + round_up(n * r->V * 16, 256);
    l.nrm = l.pos + round_up(n * r->V * 16, 256);
    l.box = l.nrm + round_up(n * r->V * 16, 256);
    l.total = l.box + round_up(n * r->T * 8, 256);
    return l;
}

int check_call(const sdfa_renderer *r, const float *d_verts, int64_t n, void *ws, int64_t ws_bytes, const char *who) {
    if (!r) return sdfa_fail(SDFA_EINVAL, "%s: null renderer", who);
    if (n < 0) return sdfa_fail(SDFA_EINVAL, "%s: negative frame count", who);
    if (n == 0) return SDFA_OK;
    if (!d_verts || !ws) return sdfa_fail(SDFA_EINVAL, "%s: null pointer", who);
    if (n > 65535) return sdfa_fail(SDFA_EINVAL, "%s: at most 65535 frames per call (%lld given)", who, (long long)n);
    if ((uintptr_t)ws & 255) return sdfa_fail(SDFA_EINVAL, "%s: workspace must be 256-byte aligned", who);
    const int64_t need = layout(r, n).total;
    if (ws_bytes < need)
        return sdfa_fail(SDFA_ENOSPACE, "%s: workspace of %lld bytes, %lld needed for %lld frames", who, (long long)ws_bytes, (long long)need, (long long)n);
    return SDFA_OK;
}

int launch_vertex(sdfa_renderer *r, const float *d_verts, int64_t n, int4 *scr, float4 *pos, float4 *nrm, hipStream_t s) {
    const int64_t total = n * r->V;
    hipLaunchKernelGGL(render_vertex_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, d_verts, total, (int)r->V,
                       r->normals == SDFA_RENDER_NORMALS_TEMPLATE ? r->d_tmpl_nrm : nullptr, r->d_csr_off, r->d_csr_face,
                       r->d_faces, r->vc, scr, pos, nrm);
    HIP_TRY(hipGetLastError());
    return SDFA_OK;
}

}  // namespace

extern "C" {

int sdfa_render_abi_version(void) { return SDFA_RENDER_ABI_VERSION; }

int sdfa_render_default_params(sdfa_render_params *out) {
    if (!out) return sdfa_fail(SDFA_EINVAL, "render_default_params: null pointer");
    static const float pose[16] = {
        9.84561989e-01f, -1.14640632e-02f, 1.74657155e-01f, 7.99997887e-02f,
        -2.63421926e-08f, 9.97852584e-01f, 6.54966148e-02f, 3.00000020e-02f,
        -1.75033820e-01f, -6.44855109e-02f, 9.82448868e-01f, 4.49999897e-01f,
        0.f, 0.f, 0.f, 1.f};
    sdfa_render_params p{};
    for (int i = 0; i < 16; ++i) p.cam_pose[i] = pose[i];
    p.yfov = (float)(M_PI / 4.0);
    p.znear = 0.05f;
    p.ambient = 0.02f;
    p.dir_intensity = 3.5f;
    p.point_intensity = 0.5f;
    for (int c = 0; c < 3; ++c) { p.albedo[c] = 0.4f; p.background[c] = 1.0f; }
    *out = p;
    return SDFA_OK;
}

sdfa_renderer *sdfa_render_create(const float *h_template_verts, int64_t n_verts, const uint32_t *h_faces, int64_t n_tris,
                                  int width, int height, int samples, int normals_mode, const sdfa_render_params *params,
                                  void *stream) {
    if (!h_template_verts || !h_faces || n_verts <= 0 || n_tris <= 0 || n_verts >= (1 << 26) || n_tris >= (1 << 26)) {
        sdfa_fail(SDFA_EINVAL, "render_create: null pointer or bad vertex / triangle count");
        return nullptr;
    }
    if (width < 1 || height < 1 || width > 8192 || height > 8192) {
        sdfa_fail(SDFA_EINVAL, "render_create: image size %d x %d outside 1 .. 8192", width, height);
        return nullptr;
    }
    if (samples != 1 && samples != 4) { sdfa_fail(SDFA_EINVAL, "render_create: samples must be 1 or 4 (%d given)", samples); return nullptr; }
    if (normals_mode != SDFA_RENDER_NORMALS_TEMPLATE && normals_mode != SDFA_RENDER_NORMALS_FRAME) {
        sdfa_fail(SDFA_EINVAL, "render_create: unknown normals mode %d", normals_mode);
        return nullptr;
    }
    sdfa_render_params p;
    if (params) p = *params;
    else sdfa_render_default_params(&p);
    float vmax = 0.f;
    for (int64_t i = 0; i < 3 * n_verts; ++i) {
        const float a = std::fabs(h_template_verts[i]);
        if (!std::isfinite(a)) { sdfa_fail(SDFA_EINVAL, "render_create: non-finite template vertex"); return nullptr; }
        vmax = a > vmax ? a : vmax;
    }
    if (vmax == 0.f) { sdfa_fail(SDFA_EINVAL, "render_create: the template has no extent"); return nullptr; }
    std::vector<int> off(n_verts + 1, 0), face(3 * n_tris);
    for (int64_t i = 0; i < 3 * n_tris; ++i) {
        if (h_faces[i] >= (uint64_t)n_verts) { sdfa_fail(SDFA_EINVAL, "render_create: face %lld addresses vertex %u of %lld", (long long)(i / 3), h_faces[i], (long long)n_verts); return nullptr; }
        ++off[h_faces[i] + 1];
    }
    for (int64_t v = 0; v < n_verts; ++v) off[v + 1] += off[v];
    {
        std::vector<int> fill(off.begin(), off.end() - 1);
        for (int64_t i = 0; i < 3 * n_tris; ++i) face[fill[h_faces[i]]++] = (int)(i / 3);    // ascending face order per vertex
    }

    sdfa_renderer *r = new sdfa_renderer;
    r->V = n_verts; r->T = n_tris; r->W = width; r->H = height; r->samples = samples; r->normals = normals_mode;
    VertexConsts &k = r->vc;
    k.s = 0.15f / vmax;
    double R[3][3], t[3];
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) R[i][j] = (double)p.cam_pose[4 * i + j];
        t[i] = (double)p.cam_pose[4 * i + 3];
    }
    for (int i = 0; i < 3; ++i) {                       // rigid inverse of the camera-to-world pose: (R^T, -R^T t)
        for (int j = 0; j < 3; ++j) k.m[4 * i + j] = (float)R[j][i];
        k.m[4 * i + 3] = (float)(-((R[0][i] * t[0] + R[1][i] * t[1]) + R[2][i] * t[2]));
    }
    const double fy = 1.0 / std::tan((double)p.yfov * 0.5);
    k.fy = (float)fy;
    k.fx = (float)(fy / ((double)width / (double)height));
    k.hw = 0.5f * (float)width;
    k.hh = 0.5f * (float)height;
    k.znear = p.znear;
    k.guard = (float)SDFA_RENDER_GUARD_PX;
    for (int c = 0; c < 3; ++c) {
        r->sc.ka[c] = p.albedo[c] * p.ambient;
        r->sc.kd[c] = (float)((double)p.albedo[c] / M_PI);
        r->sc.bg[c] = p.background[c];
    }
    r->sc.dir_i = p.dir_intensity;
    r->sc.pt_i = p.point_intensity;

    hipStream_t s = (hipStream_t)stream;
    float *d_tv = nullptr;
    auto bail = [&](const char *what, hipError_t e) {
        sdfa_fail(SDFA_EHIP, "render_create: %s failed: %s", what, hipGetErrorString(e));
        if (d_tv) (void)hipFree(d_tv);
        sdfa_render_destroy(r);
        return (sdfa_renderer *)nullptr;
    };
    hipError_t e;
    if ((e = hipMalloc(&r->d_faces, 12 * n_tris)) != hipSuccess) return bail("hipMalloc", e);
    if ((e = hipMalloc(&r->d_csr_off, 4 * (n_verts + 1))) != hipSuccess) return bail("hipMalloc", e);
    if ((e = hipMalloc(&r->d_csr_face, 12 * n_tris)) != hipSuccess) return bail("hipMalloc", e);
    if ((e = hipMalloc(&r->d_tmpl_nrm, 16 * n_verts)) != hipSuccess) return bail("hipMalloc", e);
    if ((e = hipMalloc(&d_tv, 12 * n_verts)) != hipSuccess) return bail("hipMalloc", e);
    if ((e = hipMemcpyAsync(r->d_faces, h_faces, 12 * n_tris, hipMemcpyHostToDevice, s)) != hipSuccess) return bail("hipMemcpyAsync", e);
    if ((e = hipMemcpyAsync(r->d_csr_off, off.data(), 4 * (n_verts + 1), hipMemcpyHostToDevice, s)) != hipSuccess) return bail("hipMemcpyAsync", e);
    if ((e = hipMemcpyAsync(r->d_csr_face, face.data(), 12 * n_tris, hipMemcpyHostToDevice, s)) != hipSuccess) return bail("hipMemcpyAsync", e);
    if ((e = hipMemcpyAsync(d_tv, h_template_verts, 12 * n_verts, hipMemcpyHostToDevice, s)) != hipSuccess) return bail("hipMemcpyAsync", e);
    hipLaunchKernelGGL(render_normals_kernel, dim3((unsigned)((n_verts + 255) / 256)), dim3(256), 0, s, d_tv, (int)n_verts,
                       r->d_csr_off, r->d_csr_face, r->d_faces, k.s, r->d_tmpl_nrm);
    if ((e = hipGetLastError()) != hipSuccess) return bail("render_normals_kernel", e);
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return bail("hipStreamSynchronize", e);
    (void)hipFree(d_tv);
    return r;
}

void sdfa_render_destroy(sdfa_renderer *r) {
    if (!r) return;
    if (r->d_faces) (void)hipFree(r->d_faces);
    if (r->d_csr_off) (void)hipFree(r->d_csr_off);
    if (r->d_csr_face) (void)hipFree(r->d_csr_face);
    if (r->d_tmpl_nrm) (void)hipFree(r->d_tmpl_nrm);
    delete r;
}

int64_t sdfa_render_workspace_bytes(const sdfa_renderer *r, int64_t n_frames) {
    if (!r || n_frames < 0) return sdfa_fail(SDFA_EINVAL, "render_workspace_bytes: bad argument");
    return layout(r, n_frames).total;
}

int sdfa_render_frames(sdfa_renderer *r, const float *d_verts, int64_t n_frames, uint8_t *d_rgb, int32_t *d_tri_ids,
                       void *d_workspace, int64_t workspace_bytes, void *stream) {
    int rc = check_call(r, d_verts, n_frames, d_workspace, workspace_bytes, "render_frames");
    if (rc < 0 || n_frames == 0) return rc;
    if (!d_rgb) return sdfa_fail(SDFA_EINVAL, "render_frames: null output");
    hipStream_t s = (hipStream_t)stream;
    const Layout l = layout(r, n_frames);
    char *ws = (char *)d_workspace;
    int4 *scr = (int4 *)(ws + l.scr);
    float4 *pos = (float4 *)(ws + l.pos), *nrm = (float4 *)(ws + l.nrm);
    short4 *box = (short4 *)(ws + l.box);
    if ((rc = launch_vertex(r, d_verts, n_frames, scr, pos, nrm, s)) < 0) return rc;
    const int64_t nt = n_frames * r->T;
    hipLaunchKernelGGL(render_setup_kernel, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, s, scr, r->d_faces, nt,
                       (int)r->V, (int)r->T, r->W, r->H, box);
    HIP_TRY(hipGetLastError());
    RasterArgs a{scr, pos, nrm, box, r->d_faces, (int)r->V, (int)r->T, r->W, r->H,
                 (r->W % 4 == 0 && ((uintptr_t)d_rgb & 3) == 0) ? 1 : 0, d_rgb, d_tri_ids, r->sc};
    const dim3 grid((unsigned)((r->W + TILE - 1) / TILE), (unsigned)((r->H + TILE - 1) / TILE), (unsigned)n_frames);
    if (r->samples == 4) hipLaunchKernelGGL(render_raster_kernel<4>, grid, dim3(NT), 0, s, a);
    else hipLaunchKernelGGL(render_raster_kernel<1>, grid, dim3(NT), 0, s, a);
    HIP_TRY(hipGetLastError());
    return SDFA_OK;
}

int sdfa_render_debug_screen(sdfa_renderer *r, const float *d_verts, int64_t n_frames, int32_t *d_screen,
                             void *d_workspace, int64_t workspace_bytes, void *stream) {
    int rc = check_call(r, d_verts, n_frames, d_workspace, workspace_bytes, "render_debug_screen");
    if (rc < 0 || n_frames == 0) return rc;
    if (!d_screen) return sdfa_fail(SDFA_EINVAL, "render_debug_screen: null output");
    const Layout l = layout(r, n_frames);
    char *ws = (char *)d_workspace;
    return launch_vertex(r, d_verts, n_frames, (int4 *)d_screen, (float4 *)(ws + l.pos), (float4 *)(ws + l.nrm), (hipStream_t)stream);
}

}  // extern "C"
