// mesh -> dgrad: the deformation gradient of a target mesh relative to a source mesh of the same topology, batched over
// frames -- the direction opposite to mesh.hip's solve.
//
// Reference (native C++/Eigen): deformation.get_deform_grad (deformation/cpp/src/pybind.cpp:78-99) ->
// TriangleDeformation::getDeformationGradients (deform_triangle_impl.hpp:143-213), _getTransform / _getGradFromMat (:447-470)
// and rotation_log_exp::log (rotation/utils_rotation.cpp:69-176).  Per triangle j, with float32 vertices promoted to double:
//     e1 = p2 - p1, e2 = p3 - p1, e3 = (e1 x e2) / max((e3.e3)^0.25, eps)        degenerate when |cos(e1, e2)| > 1 - eps
//     A = [ea1 ea2 ea3], B = [eb1 eb2 eb3], T = B A^-1
//     T = U S V^T (Eigen::JacobiSVD: two-sided Jacobi sweeps, singular values sorted descending), d = det(U V^T)
//     R = U diag(1,1,d) V^T, scale = V diag(1,1,d) S V^T
//     out = [s00-1 s01 s02 s11-1 s12 s22-1 logR01 logR02 logR12]
// A triangle that is degenerate on either mesh, or set in the optional mask (preload.py:778 zeroes the non-face triangles
// after the fact), gets 9 exact zeros.
//
// MI355X form: one thread per (frame, triangle), everything in fp64 registers, plain C++.  The SVD restates Eigen 3.3's
// JacobiSVD<MatrixXd> for a square 3x3 (no QR preconditioner, scale by max|T_ij|, sweeps over (1,0) (2,0) (2,1) with
// real_2x2_jacobi_svd, then sign fix and selection sort) with every index a compile-time constant, so nothing spills.
#include "common.h"
#include "kernels.h"
#include <cfloat>

namespace {

constexpr double kLogTol = 1.0e-6;         // rotation/utils_rotation.h:8 log_exp_tolerance
constexpr int kMaxSweeps = 64;             // Eigen has no bound; converged 3x3 sweeps number < 10.  A bound keeps a NaN-free
                                           // pathological input from spinning a wave forever.

struct M3 {
    double a[3][3];
};

__device__ __forceinline__ void rot_rows(M3 &m, int p, int q, double c, double s) {
    // apply_rotation_in_the_plane on rows p, q (Jacobi.h: x = c x + s y, y = -s x + c y)
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double x = m.a[p][i], y = m.a[q][i];
        m.a[p][i] = c * x + s * y;
        m.a[q][i] = -s * x + c * y;
    }
}

__device__ __forceinline__ void rot_cols(M3 &m, int p, int q, double c, double s) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double x = m.a[i][p], y = m.a[i][q];
        m.a[i][p] = c * x + s * y;
        m.a[i][q] = -s * x + c * y;
    }
}

// one (p, q) step of the sweep (JacobiSVD.h:704-731 with RealSvd2x2.h and Jacobi.h:83-113); returns true when it rotated
template <int p, int q>
__device__ __forceinline__ bool jacobi_step(M3 &W, M3 &U, M3 &V, double &max_diag) {
    const double threshold = fmax(DBL_MIN, 2.0 * DBL_EPSILON * max_diag);
    if (!(fabs(W.a[p][q]) > threshold || fabs(W.a[q][p]) > threshold)) return false;
    // real_2x2_jacobi_svd: rot1 symmetrises the 2x2 block, j_right diagonalises it
    double m00 = W.a[p][p], m01 = W.a[p][q], m10 = W.a[q][p], m11 = W.a[q][q];
    double c1 = 1.0, s1 = 0.0;
    const double t = m00 + m11, d = m10 - m01;
    if (!(fabs(d) < DBL_MIN)) {
        const double u = t / d, tmp = sqrt(1.0 + u * u);
        s1 = 1.0 / tmp;
        c1 = u / tmp;
    }
    {   // m.applyOnTheLeft(0, 1, rot1)
        const double x0 = m00, y0 = m10, x1 = m01, y1 = m11;
        m00 = c1 * x0 + s1 * y0; m10 = -s1 * x0 + c1 * y0;
        m01 = c1 * x1 + s1 * y1; m11 = -s1 * x1 + c1 * y1;
    }
    double cr = 1.0, sr = 0.0;                 // j_right.makeJacobi(m, 0, 1): x = m00, y = m01, z = m11
    const double deno = 2.0 * fabs(m01);
    if (!(deno < DBL_MIN)) {
        const double tau = (m00 - m11) / deno, w = sqrt(tau * tau + 1.0);
        const double tt = tau > 0.0 ? 1.0 / (tau + w) : 1.0 / (tau - w);
        const double sign_t = tt > 0.0 ? 1.0 : -1.0, n = 1.0 / sqrt(tt * tt + 1.0);
        sr = -sign_t * (m01 / fabs(m01)) * fabs(tt) * n;
        cr = n;
    }
    // j_left = rot1 * j_right^T, j_right^T = (cr, -sr)
    const double cl = c1 * cr - s1 * (-sr), sl = c1 * (-sr) + s1 * cr;
    rot_rows(W, p, q, cl, sl);                 // W.applyOnTheLeft(p, q, j_left)
    rot_cols(U, p, q, cl, sl);                 // U.applyOnTheRight(p, q, j_left^T): columns rotated by j_left
    rot_cols(W, p, q, cr, -sr);                // W.applyOnTheRight(p, q, j_right): columns rotated by j_right^T
    rot_cols(V, p, q, cr, -sr);
    max_diag = fmax(max_diag, fmax(fabs(W.a[p][p]), fabs(W.a[q][q])));
    return true;
}

__device__ __forceinline__ void swap_cols(M3 &m, int i, int j) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double t = m.a[r][i];
        m.a[r][i] = m.a[r][j];
        m.a[r][j] = t;
    }
}

__device__ __forceinline__ double det3(const M3 &m) {
    // Eigen determinant_impl<3>: bruteforce_det3_helper(0,1,2) - (1,0,2) + (2,0,1)
    return m.a[0][0] * (m.a[1][1] * m.a[2][2] - m.a[1][2] * m.a[2][1])
         - m.a[0][1] * (m.a[1][0] * m.a[2][2] - m.a[1][2] * m.a[2][0])
         + m.a[0][2] * (m.a[1][0] * m.a[2][1] - m.a[1][1] * m.a[2][0]);
}

__device__ __forceinline__ double cofactor(const M3 &m, int i, int j) {
    const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
    return m.a[i1][j1] * m.a[i2][j2] - m.a[i1][j2] * m.a[i2][j1];
}

// e3 of _getEdge3 (deform_triangle_impl.hpp:150-159); false = degenerate.  A zero-length edge makes the cosine NaN, which
// does NOT compare greater than 1 - eps: such a triangle goes on, as in the reference.
__device__ __forceinline__ bool edge3(const double e1[3], const double e2[3], double e3[3], double eps) {
    e3[0] = e1[1] * e2[2] - e1[2] * e2[1];
    e3[1] = e1[2] * e2[0] - e1[0] * e2[2];
    e3[2] = e1[0] * e2[1] - e1[1] * e2[0];
    const double len1 = sqrt(e1[0] * e1[0] + e1[1] * e1[1] + e1[2] * e1[2]);
    const double len2 = sqrt(e2[0] * e2[0] + e2[1] * e2[1] + e2[2] * e2[2]);
    const double abs_cos = fabs((e1[0] * e2[0] + e1[1] * e2[1] + e1[2] * e2[2]) / (len1 * len2));
    if (abs_cos > 1.0 - eps) return false;
    const double n = fmax(pow(e3[0] * e3[0] + e3[1] * e3[1] + e3[2] * e3[2], 0.25), eps);
    e3[0] /= n; e3[1] /= n; e3[2] /= n;
    return true;
}

// rotation_log_exp::log -> (log R)(0,1), (0,2), (1,2) = angle * (-axis2, axis1, -axis0)
__device__ __forceinline__ void rotation_log(const M3 &R, double out[3]) {
    out[0] = out[1] = out[2] = 0.0;
    double nrm2 = 0.0;                         // |R^T R - I|_F
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const double v = R.a[0][i] * R.a[0][j] + R.a[1][i] * R.a[1][j] + R.a[2][i] * R.a[2][j] - (i == j ? 1.0 : 0.0);
            nrm2 += v * v;
        }
    // Not orthogonal: the reference returns with angle / axis unset (uninitialised).  An R built from an SVD as above is
    // orthogonal to rounding, so this cannot fire for a finite input; zeros are written instead.
    if (sqrt(nrm2) > kLogTol) return;
    double csin = (R.a[0][0] + R.a[1][1] + R.a[2][2] - 1.0) / 2.0;
    if (csin < -1.0 || csin > 1.0) {
        if (fabs(csin - 1.0) > kLogTol && fabs(csin + 1.0) > kLogTol) return;   // unset in the reference, as above
        csin = fmax(fmin(1.0, csin), -1.0);
    }
    double tangle = acos(csin);
    if (fabs(tangle) < kLogTol) return;        // angle 0, axis 0: exact zeros
    double angle, ax[3];
    if (fabs(tangle - M_PI) < kLogTol) {
        angle = M_PI;
        const double b00 = (R.a[0][0] + 1.0) / 2.0, b01 = R.a[0][1] / 2.0, b02 = R.a[0][2] / 2.0;
        const double b11 = (R.a[1][1] + 1.0) / 2.0, b22 = (R.a[2][2] + 1.0) / 2.0;
        const double k1 = sqrt(b00);
        ax[0] = k1;
        ax[1] = k1 * b01 > 0.0 ? sqrt(b11) : -sqrt(b11);
        ax[2] = k1 * b02 > 0.0 ? sqrt(b22) : -sqrt(b22);
    } else {
        const double taxis[3] = {R.a[2][1] - R.a[1][2], R.a[0][2] - R.a[2][0], R.a[1][0] - R.a[0][1]};
        double sinv = sin(tangle);
        double t0 = taxis[0] / (2.0 * sinv), t1 = taxis[1] / (2.0 * sinv), t2 = taxis[2] / (2.0 * sinv);
        const double omc = 1.0 - csin;
        const double r01 = omc * t0 * t1 - t2 * sinv, r02 = omc * t0 * t2 + t1 * sinv, r10 = omc * t0 * t1 + t2 * sinv;
        const double r12 = omc * t1 * t2 - t0 * sinv, r20 = omc * t0 * t2 - t1 * sinv, r21 = omc * t1 * t2 + t0 * sinv;
        const double check = (R.a[0][1] - r01) * (R.a[0][1] - r01) + (R.a[0][2] - r02) * (R.a[0][2] - r02)
                           + (R.a[1][0] - r10) * (R.a[1][0] - r10) + (R.a[1][2] - r12) * (R.a[1][2] - r12)
                           + (R.a[2][0] - r20) * (R.a[2][0] - r20) + (R.a[2][1] - r21) * (R.a[2][1] - r21);
        if (!(check < kLogTol)) {              // "angle is larger than pi": the other half-turn
            tangle = 2 * M_PI - tangle;
            sinv = sin(tangle);
            t0 = taxis[0] / (2.0 * sinv); t1 = taxis[1] / (2.0 * sinv); t2 = taxis[2] / (2.0 * sinv);
        }
        angle = tangle;
        ax[0] = t0; ax[1] = t1; ax[2] = t2;
    }
    // cross_axis = temp - temp^T with temp(2,1) = a0, temp(0,2) = a1, temp(1,0) = a2
    out[0] = angle * (0.0 - ax[2]);
    out[1] = angle * (ax[1] - 0.0);
    out[2] = angle * (0.0 - ax[0]);
}

// _getTransform + _getGradFromMat for one non-degenerate triangle
__device__ __forceinline__ void grad_from_frames(const M3 &A, const M3 &B, double g[9]) {
    M3 Ainv, T;
    {   // Eigen compute_inverse_size3_helper: cofactors, det from column 0
        const double c00 = cofactor(A, 0, 0), c10 = cofactor(A, 1, 0), c20 = cofactor(A, 2, 0);
        const double invdet = 1.0 / (c00 * A.a[0][0] + c10 * A.a[1][0] + c20 * A.a[2][0]);
        Ainv.a[0][0] = c00 * invdet; Ainv.a[0][1] = c10 * invdet; Ainv.a[0][2] = c20 * invdet;
        Ainv.a[1][0] = cofactor(A, 0, 1) * invdet; Ainv.a[1][1] = cofactor(A, 1, 1) * invdet; Ainv.a[1][2] = cofactor(A, 2, 1) * invdet;
        Ainv.a[2][0] = cofactor(A, 0, 2) * invdet; Ainv.a[2][1] = cofactor(A, 1, 2) * invdet; Ainv.a[2][2] = cofactor(A, 2, 2) * invdet;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) T.a[i][j] = B.a[i][0] * Ainv.a[0][j] + B.a[i][1] * Ainv.a[1][j] + B.a[i][2] * Ainv.a[2][j];

    // ---- JacobiSVD (JacobiSVD.h:663-766), square case ----
    double scale = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) scale = fmax(scale, fabs(T.a[i][j]));
    if (scale == 0.0) scale = 1.0;
    M3 W, U, V;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            W.a[i][j] = T.a[i][j] / scale;
            U.a[i][j] = V.a[i][j] = i == j ? 1.0 : 0.0;
        }
    double max_diag = fmax(fmax(fabs(W.a[0][0]), fabs(W.a[1][1])), fabs(W.a[2][2]));
    for (int sweep = 0; sweep < kMaxSweeps; ++sweep) {
        bool rotated = jacobi_step<1, 0>(W, U, V, max_diag);
        rotated |= jacobi_step<2, 0>(W, U, V, max_diag);
        rotated |= jacobi_step<2, 1>(W, U, V, max_diag);
        if (!rotated) break;
    }
    double sv[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double a = W.a[i][i];
        sv[i] = fabs(a);
        if (a < 0.0)
#pragma unroll
            for (int r = 0; r < 3; ++r) U.a[r][i] = -U.a[r][i];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) sv[i] *= scale;
    // descending selection sort; maxCoeff returns the FIRST maximum; stops at a zero maximum
    {
        int pos = 0;
        if (sv[1] > sv[pos]) pos = 1;
        if (sv[2] > sv[pos]) pos = 2;
        if (sv[pos] != 0.0) {
            if (pos == 1) { const double t = sv[0]; sv[0] = sv[1]; sv[1] = t; swap_cols(U, 0, 1); swap_cols(V, 0, 1); }
            if (pos == 2) { const double t = sv[0]; sv[0] = sv[2]; sv[2] = t; swap_cols(U, 0, 2); swap_cols(V, 0, 2); }
            if (sv[2] > sv[1]) { const double t = sv[1]; sv[1] = sv[2]; sv[2] = t; swap_cols(U, 1, 2); swap_cols(V, 1, 2); }
        }
    }

    // ---- polar part (deform_triangle_impl.hpp:455-461) ----
    M3 UVt;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) UVt.a[i][j] = U.a[i][0] * V.a[j][0] + U.a[i][1] * V.a[j][1] + U.a[i][2] * V.a[j][2];
    const double d = det3(UVt);
    M3 R;
    double S[3][3];
    const double dd[3] = {1.0, 1.0, d};
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            R.a[i][j] = U.a[i][0] * V.a[j][0] + U.a[i][1] * V.a[j][1] + (U.a[i][2] * d) * V.a[j][2];
            S[i][j] = (V.a[i][0] * dd[0] * sv[0]) * V.a[j][0] + (V.a[i][1] * dd[1] * sv[1]) * V.a[j][1] + (V.a[i][2] * dd[2] * sv[2]) * V.a[j][2];
        }
    double lg[3];
    rotation_log(R, lg);
    g[0] = S[0][0] - 1.0; g[1] = S[0][1]; g[2] = S[0][2];
    g[3] = S[1][1] - 1.0; g[4] = S[1][2]; g[5] = S[2][2] - 1.0;
    g[6] = lg[0]; g[7] = lg[1]; g[8] = lg[2];
}

__device__ __forceinline__ void load3(const float *__restrict__ p, double v[3]) {
    v[0] = (double)p[0]; v[1] = (double)p[1]; v[2] = (double)p[2];
}

// the target vertex: per-frame vertices, or float32(source + offset) (preload.py:770 adds in float32) promoted to double
__device__ __forceinline__ void load_target(const DgradArgs &a, int64_t frame, uint32_t v, double out[3]) {
    const float *__restrict__ t = a.target + (frame * a.n_verts + v) * 3;
    if (a.target_is_offsets) {
        const float *__restrict__ s = a.src + (int64_t)v * 3;
#pragma unroll
        for (int k = 0; k < 3; ++k) out[k] = (double)(s[k] + t[k]);
    } else {
        load3(t, out);
    }
}

__global__ __launch_bounds__(256) void deform_grad_kernel(const DgradArgs a) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= a.n_frames * a.n_tris) return;
    const int64_t frame = idx / a.n_tris;
    const int j = (int)(idx - frame * a.n_tris);
    double g[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    const uint32_t i1 = a.faces[3 * j], i2 = a.faces[3 * j + 1], i3 = a.faces[3 * j + 2];
    if (i1 >= (uint32_t)a.n_verts || i2 >= (uint32_t)a.n_verts || i3 >= (uint32_t)a.n_verts) {
        // out-of-range face: never read; NaN marks the row (the host-side callers validate faces before upload)
#pragma unroll
        for (int k = 0; k < 9; ++k) g[k] = __builtin_nan("");
    } else if (!(a.mask && a.mask[j])) {
        double p1[3], p2[3], p3[3], q1[3], q2[3], q3[3];
        load3(a.src + (int64_t)i1 * 3, p1); load3(a.src + (int64_t)i2 * 3, p2); load3(a.src + (int64_t)i3 * 3, p3);
        load_target(a, frame, i1, q1); load_target(a, frame, i2, q2); load_target(a, frame, i3, q3);
        double ea1[3], ea2[3], ea3[3], eb1[3], eb2[3], eb3[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            ea1[k] = p2[k] - p1[k]; ea2[k] = p3[k] - p1[k];
            eb1[k] = q2[k] - q1[k]; eb2[k] = q3[k] - q1[k];
        }
        const bool good_a = edge3(ea1, ea2, ea3, a.eps);
        const bool good_b = edge3(eb1, eb2, eb3, a.eps);
        if (good_a && good_b) {
            M3 A, B;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                A.a[k][0] = ea1[k]; A.a[k][1] = ea2[k]; A.a[k][2] = ea3[k];
                B.a[k][0] = eb1[k]; B.a[k][1] = eb2[k]; B.a[k][2] = eb3[k];
            }
            grad_from_frames(A, B, g);
        }
    }
    const int64_t o = idx * 9;
    if (a.out64) {
#pragma unroll
        for (int k = 0; k < 9; ++k) a.out64[o + k] = g[k];
    } else {
#pragma unroll
        for (int k = 0; k < 9; ++k) a.out32[o + k] = (float)g[k];
    }
}

}  // namespace

hipError_t sdfa_launch_deform_grad(const DgradArgs &a, hipStream_t s) {
    const int64_t n = a.n_frames * a.n_tris;
    hipLaunchKernelGGL(deform_grad_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}
