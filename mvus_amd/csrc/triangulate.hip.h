// Two-view linear triangulation on the GPU: epipolar.triangulate_matlab (reference
// multiviewunsynch/reconstruction/epipolar.py:497-510) for N point pairs, one lane per pair, plus the two
// reprojection errors Scene.triangulate filters by (common.py:786-789, epipolar.py:639).
//
// The reference takes, per point, the right singular vector of the smallest singular value of the 4x4 matrix
//     A = [ u1 P1[2] - P1[0] ;  v1 P1[2] - P1[1] ;  u2 P2[2] - P2[0] ;  v2 P2[2] - P2[1] ]
// (np.linalg.svd, V[-1] / V[-1,-1]).  Here: one-sided Jacobi (Hestenes) on the columns of A -- plane rotations applied to
// A and accumulated in V until all column pairs are orthogonal; the column of smallest norm is that singular vector.
// It works on A itself (not on A^T A), so small singular values keep their relative accuracy like LAPACK's SVD does; the
// scale/sign ambiguity disappears in the division by the last component, as in the reference.
#pragma once
#include "ba_math.h"      // MVUS_HD; pulls in hip_runtime.h under hipcc (the test-only host harness compiles the pair math with g++)

namespace mvus {

MVUS_HD void triangulate_pair(const double P1[12], const double P2[12], double u1, double v1, double u2, double v2, double X[4]) {
  double G[4][4], V[4][4];                       // G[row][col]
  for (int j = 0; j < 4; ++j) {
    G[0][j] = u1 * P1[8 + j] - P1[j];
    G[1][j] = v1 * P1[8 + j] - P1[4 + j];
    G[2][j] = u2 * P2[8 + j] - P2[j];
    G[3][j] = v2 * P2[8 + j] - P2[4 + j];
    for (int i = 0; i < 4; ++i) V[i][j] = i == j ? 1.0 : 0.0;
  }
  for (int sweep = 0; sweep < 30; ++sweep) {
    bool rotated = false;
    for (int p = 0; p < 3; ++p)
      for (int q = p + 1; q < 4; ++q) {
        double al = 0.0, be = 0.0, ga = 0.0;
        for (int i = 0; i < 4; ++i) { al += G[i][p] * G[i][p]; be += G[i][q] * G[i][q]; ga += G[i][p] * G[i][q]; }
        if (fabs(ga) <= 1e-16 * sqrt(al * be) || ga == 0.0) continue;
        rotated = true;
        const double zeta = (be - al) / (2.0 * ga);
        const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
        const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
        for (int i = 0; i < 4; ++i) {
          const double gp = G[i][p], gq = G[i][q];
          G[i][p] = c * gp - s * gq; G[i][q] = s * gp + c * gq;
          const double vp = V[i][p], vq = V[i][q];
          V[i][p] = c * vp - s * vq; V[i][q] = s * vp + c * vq;
        }
      }
    if (!rotated) break;
  }
  int jm = 0;
  double nm = 0.0;
  for (int j = 0; j < 4; ++j) {
    double nj = 0.0;
    for (int i = 0; i < 4; ++i) nj += G[i][j] * G[i][j];
    if (j == 0 || nj < nm) { nm = nj; jm = j; }
  }
  // static indexing of V's columns (the column index is data dependent): select
  for (int i = 0; i < 4; ++i) X[i] = jm == 0 ? V[i][0] : (jm == 1 ? V[i][1] : (jm == 2 ? V[i][2] : V[i][3]));
  const double w = X[3];
  for (int i = 0; i < 4; ++i) X[i] = X[i] / w;
}

// Camera.projectPoint (common.py:1072-1079) + epipolar.reprojection_error (epipolar.py:639)
MVUS_HD double reprojection_distance(const double P[12], const double X[4], double u, double v) {
  const double a = P[0] * X[0] + P[1] * X[1] + P[2] * X[2] + P[3] * X[3];
  const double b = P[4] * X[0] + P[5] * X[1] + P[6] * X[2] + P[7] * X[3];
  const double c = P[8] * X[0] + P[9] * X[1] + P[10] * X[2] + P[11] * X[3];
  const double du = u - a / c, dv = v - b / c;
  return sqrt(du * du + dv * dv);
}

// Gauss-Newton covariance of a triangulated point: (A^T A)^-1 at X, A the four rows (P[r,:3] - x_r P[2,:3]) / (z sigma), r = 0, 1, of the two
// cameras -- the Jacobian of the reprojection (x_0, x_1) = (P[0] X, P[1] X) / z, z = P[2] X, over the pixel noise sigma of that camera.  To
// first order the covariance of the point of least reprojection error; the linear triangulation above is close to that point, not equal to it.
// cov: xx xy xz yy yz zz.  The 3x3 inverse goes through a Cholesky factor; all six entries are NaN when a pivot is at most 1e-14 of its diagonal
// entry (no parallax: the cameras coincide or the rays are parallel), X is not finite, or the point is not in front of both cameras (z <= 0).
MVUS_HD void triangulation_covariance(const double P1[12], const double P2[12], const double X[4], double sigma1, double sigma2, double cov[6]) {
  double m[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  bool ok = __builtin_isfinite(X[0]) && __builtin_isfinite(X[1]) && __builtin_isfinite(X[2]) && __builtin_isfinite(X[3]);
  for (int c = 0; c < 2; ++c) {
    const double* P = c == 0 ? P1 : P2;
    const double a = P[0] * X[0] + P[1] * X[1] + P[2] * X[2] + P[3] * X[3];
    const double b = P[4] * X[0] + P[5] * X[1] + P[6] * X[2] + P[7] * X[3];
    const double z = P[8] * X[0] + P[9] * X[1] + P[10] * X[2] + P[11] * X[3];
    ok = ok && z > 0.0;
    const double x0 = a / z, x1 = b / z, scale = 1.0 / (z * (c == 0 ? sigma1 : sigma2));
    double r0[3], r1[3];
    for (int k = 0; k < 3; ++k) { r0[k] = (P[k] - x0 * P[8 + k]) * scale; r1[k] = (P[4 + k] - x1 * P[8 + k]) * scale; }
    m[0] += r0[0] * r0[0] + r1[0] * r1[0]; m[1] += r0[0] * r0[1] + r1[0] * r1[1]; m[2] += r0[0] * r0[2] + r1[0] * r1[2];
    m[3] += r0[1] * r0[1] + r1[1] * r1[1]; m[4] += r0[1] * r0[2] + r1[1] * r1[2]; m[5] += r0[2] * r0[2] + r1[2] * r1[2];
  }
  for (int k = 0; k < 6; ++k) cov[k] = __builtin_nan("");
  if (!ok || !(m[0] > 0.0)) return;
  const double l00 = sqrt(m[0]), l10 = m[1] / l00, l20 = m[2] / l00;
  const double d1 = m[3] - l10 * l10;
  if (!(d1 > 1e-14 * m[3])) return;
  const double l11 = sqrt(d1), l21 = (m[4] - l20 * l10) / l11;
  const double d2 = m[5] - l20 * l20 - l21 * l21;
  if (!(d2 > 1e-14 * m[5])) return;
  const double l22 = sqrt(d2);
  // L^-1 (lower), then cov = L^-T L^-1
  const double i00 = 1.0 / l00, i11 = 1.0 / l11, i22 = 1.0 / l22;
  const double i10 = -l10 * i00 * i11, i21 = -l21 * i11 * i22, i20 = -(l20 * i00 + l21 * i10) * i22;
  cov[0] = i00 * i00 + i10 * i10 + i20 * i20; cov[1] = i10 * i11 + i20 * i21; cov[2] = i20 * i22;
  cov[3] = i11 * i11 + i21 * i21; cov[4] = i21 * i22; cov[5] = i22 * i22;
}

#if defined(__HIPCC__)
struct TriCams { double P1[12], P2[12]; };      // by value in the kernel arguments: wave-uniform -> SGPRs

// x1, x2: [2][N] (u row, v row); X: [4][N]; err1/err2: [N] or nullptr.  Every access is one contiguous 512-B segment per wavefront.
__global__ __launch_bounds__(256) void k_triangulate(TriCams cams, long long N, const double* __restrict__ x1, const double* __restrict__ x2,
                                                     double* __restrict__ X, double* __restrict__ err1, double* __restrict__ err2) {
  const long long i = blockIdx.x * 256ll + threadIdx.x;
  if (i >= N) return;
  const double u1 = x1[i], v1 = x1[N + i], u2 = x2[i], v2 = x2[N + i];
  double Xh[4];
  triangulate_pair(cams.P1, cams.P2, u1, v1, u2, v2, Xh);
  X[i] = Xh[0]; X[N + i] = Xh[1]; X[2 * N + i] = Xh[2]; X[3 * N + i] = Xh[3];
  if (err1) err1[i] = reprojection_distance(cams.P1, Xh, u1, v1);
  if (err2) err2[i] = reprojection_distance(cams.P2, Xh, u2, v2);
}

// k_triangulate with the covariance of every point (triangulation_covariance): cov [6][N], component-major like X
__global__ __launch_bounds__(256) void k_triangulate_cov(TriCams cams, double sigma1, double sigma2, long long N, const double* __restrict__ x1,
                                                         const double* __restrict__ x2, double* __restrict__ X, double* __restrict__ cov,
                                                         double* __restrict__ err1, double* __restrict__ err2) {
  const long long i = blockIdx.x * 256ll + threadIdx.x;
  if (i >= N) return;
  const double u1 = x1[i], v1 = x1[N + i], u2 = x2[i], v2 = x2[N + i];
  double Xh[4], C[6];
  triangulate_pair(cams.P1, cams.P2, u1, v1, u2, v2, Xh);
  X[i] = Xh[0]; X[N + i] = Xh[1]; X[2 * N + i] = Xh[2]; X[3 * N + i] = Xh[3];
  if (err1) err1[i] = reprojection_distance(cams.P1, Xh, u1, v1);
  if (err2) err2[i] = reprojection_distance(cams.P2, Xh, u2, v2);
  triangulation_covariance(cams.P1, cams.P2, Xh, sigma1, sigma2, C);
#pragma unroll
  for (int k = 0; k < 6; ++k) cov[k * N + i] = C[k];
}
#endif

}  // namespace mvus
