/* C ABI of the batched triangle rasterizer in libsdfa_hip.so (sdfa-2019_amd/csrc/render.hip).
 *
 * It turns the vertices of n animation frames, already on the device ((n, V, 3) fp32, the layout
 * sdfa_mesh_from_dgrad_seek writes), into (n, H, W, 3) uint8 RGB images, row 0 at the top -- the last stage of the
 * reference's evaluate (speech_anime/viewer/render_py.py, pyrender) -- and optionally an (n, H, W) int32 visibility
 * buffer (triangle id of each pixel's first sample, -1 for background).
 *
 * Conventions are those of sdfa_hip.h: every call returns >= 0 on success and a negative SDFA_E* code on failure,
 * sdfa_last_error() describes the failure, work is enqueued on `stream` and only the constructor synchronises.
 * This surface is versioned on its own (SDFA_RENDER_ABI_VERSION); it does not change SDFA_ABI_VERSION.
 *
 * Rendering contract (the reference's rig values; DESIGN.md "Rendering"):
 *   scale    s = 0.15f / max|template_verts| (fp32, fixed at create time), world position p = s * v
 *   camera   cam_pose = camera-to-world 4x4 (render_py.py:14-19); the view transform is its rigid inverse
 *            (R^T, -R^T t) formed in fp64 and rounded to fp32 at create time; the camera looks down its -Z
 *   project  yfov = pi/4, aspect = W/H, znear = 0.05, infinite far plane (pyrender PerspectiveCamera);
 *            fy = 1/tan(yfov/2), fx = fy/aspect (fp64 -> fp32); w = -z_cam, iw = 1/w,
 *            ndc = (c * f) * iw, X = (ndc_x + 1) * (W/2), Y = (1 - ndc_y) * (H/2), snapped to 1/256 pixel with
 *            rintf into int32
 *   drop     a vertex is invalid if any camera coordinate is non-finite, if w <= znear or if |X| or |Y| exceeds the
 *            2^15-pixel guard band; a triangle with an invalid vertex, zero area or clockwise NDC winding (back face)
 *            is dropped
 *   coverage exact int64 edge functions of the snapped vertices with a top-left fill rule: a sample on an edge belongs
 *            to the triangle whose edge is a left edge (dy > 0 in screen space, y down) or a top edge (dy == 0, dx < 0)
 *   depth    w_i = (float)F_i * (1.0f / (float)D), iw = (w0*iw0 + w1*iw1) + w2*iw2; the larger iw is nearer, a tie
 *            goes to the smaller triangle index (a lexicographic compare, independent of scheduling)
 *   samples  1 (pixel centre) or 4 (rotated grid (-2,-6) (6,-2) (-6,2) (2,6) / 16 pixel); every sample is shaded,
 *            clamped to [0, 1], the samples averaged in fp32 and rounded to uint8 once
 *   normals  SDFA_RENDER_NORMALS_TEMPLATE: the template's area-weighted vertex normals for every frame (the reference
 *            only updates positions, render_py.py:58); SDFA_RENDER_NORMALS_FRAME: recomputed per frame by the same
 *            device function (a gather over a vertex -> face list in ascending face order, no atomics)
 *   shading  perspective-correct normal and camera-space position, Lambert: albedo * ambient + albedo / pi *
 *            (dir_intensity * max(0, n.z) + point_intensity * max(0, n.l) / d^2), the directional light along the
 *            camera's -Z, the point light at the camera; background where no triangle covers a sample
 * The vertex and raster stages are reproduced bit for bit by a numpy float32 restatement (tests/render_oracle.py).
 */
#ifndef SDFA_RENDER_H
#define SDFA_RENDER_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SDFA_RENDER_ABI_VERSION 1

#define SDFA_RENDER_NORMALS_TEMPLATE 0
#define SDFA_RENDER_NORMALS_FRAME    1

#define SDFA_RENDER_TILE      32      /* a workgroup rasterises one 32 x 32 pixel tile of one frame */
#define SDFA_RENDER_GUARD_PX  32768   /* 2^15-pixel guard band */

typedef struct sdfa_render_params {
    float cam_pose[16];        /* camera-to-world, row-major (render_py.py:14-19) */
    float yfov;                /* radians (pi/4) */
    float znear;               /* 0.05 */
    float ambient;             /* 0.02 */
    float dir_intensity;       /* 3.5, along the camera's -Z */
    float point_intensity;     /* 0.5, at the camera, 1/d^2 falloff */
    float albedo[3];           /* grey */
    float background[3];       /* white, in [0, 1] */
} sdfa_render_params;

typedef struct sdfa_renderer sdfa_renderer;

int sdfa_render_abi_version(void);

/* The reference's rig values (above) into *out. */
int sdfa_render_default_params(sdfa_render_params *out);

/* Template (host fp32 (n_verts, 3)) and triangles (host uint32 (n_tris, 3)); width, height in pixels (1 .. 8192);
 * samples 1 or 4; normals_mode SDFA_RENDER_NORMALS_*; params NULL for sdfa_render_default_params.  Uploads the faces
 * and the vertex -> face list, computes the template normals on the device and synchronises `stream`.
 * NULL on failure (sdfa_last_error()). */
sdfa_renderer *sdfa_render_create(const float *h_template_verts, int64_t n_verts, const uint32_t *h_faces, int64_t n_tris,
                                  int width, int height, int samples, int normals_mode, const sdfa_render_params *params,
                                  void *stream);
void sdfa_render_destroy(sdfa_renderer *r);

/* Device workspace of one sdfa_render_frames call of n_frames frames. */
int64_t sdfa_render_workspace_bytes(const sdfa_renderer *r, int64_t n_frames);

/* d_verts (n_frames, n_verts, 3) fp32 -> d_rgb (n_frames, height, width, 3) uint8 and, if d_tri_ids is not NULL,
 * (n_frames, height, width) int32.  n_frames == 0 is a no-op. */
int sdfa_render_frames(sdfa_renderer *r, const float *d_verts, int64_t n_frames, uint8_t *d_rgb, int32_t *d_tri_ids,
                       void *d_workspace, int64_t workspace_bytes, void *stream);

/* The vertex stage alone: d_screen (n_frames, n_verts, 4) int32 = {x, y (1/256 pixel), bits of fp32 iw, valid}. */
int sdfa_render_debug_screen(sdfa_renderer *r, const float *d_verts, int64_t n_frames, int32_t *d_screen,
                             void *d_workspace, int64_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif
