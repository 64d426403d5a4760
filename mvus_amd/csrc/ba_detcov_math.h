// Row routines of the per-detection prediction covariance (ba_detcov.hip.h), written once for the device and for the host build that
// pins them (tests/detcov_hostcheck.cpp).  Plain C++, no device intrinsics, one fixed order of summation; k_detcov only hands each
// lane its detection.
//
// For a detection of camera c with knot span p, J_i = [a | b]: a its two rows over the camera's B = 3 + P slots, b over the twelve
// coordinates of control points p .. p + 3 (the held analytic Jacobian: rows of the absolute residuals, D J_raw with D = diag(sign e)).
// With the covariance chain's names (ba_cov.hip.h) and everything divided by sigma^2,
//   Pi = a Scc a^T  -  (a T^T b^T + its transpose)  +  b G b^T,
// Scc = Sigma_cc[c, c] (B x B), T = T[3p .. 3p + 11, c B .. c B + B - 1] (12 x B), G = (sel + R)[p .. p + 3, p .. p + 3] (12 x 12, from
// the band blocks w <= 3).  The three terms cancel: they are formed and added in this order and no other.
#pragma once
#include <cmath>
#include <limits>

#include "ba_math.h"

// The outer loops stay loops on the device: unrolled, the B x B, 12 x B and band forms of the opt_calib kernel want more registers than
// a lane has (330 spilled VGPRs, 1324 B of scratch per lane).  Rolled, the slots of the opt_calib kernel that are indexed at run time
// live in 304 B of scratch (none without opt_calib) and both kernels run three wavefronts per SIMD; the order of summation is the same
// either way.
#if defined(__HIP_DEVICE_COMPILE__)
#define MVUS_DETCOV_ROLLED _Pragma("unroll 1")
#else
#define MVUS_DETCOV_ROLLED
#endif

namespace mvus {

// out[3] = (uu, uv, vv) of  v_x . (M v_x),  v_x . (M v_y),  v_y . (M v_y)  for a symmetric K x K matrix M given by rows (ld doubles apart)
template <int K>
MVUS_HD void detcov_sym_form(const double* M, long long ld, const double* vx, const double* vy, double* out) {
  double uu = 0.0, uv = 0.0, vv = 0.0;
  MVUS_DETCOV_ROLLED
  for (int j = 0; j < K; ++j) {
    const double* Mj = M + (long long)j * ld;
    double sx = 0.0, sy = 0.0;
    for (int k = 0; k < K; ++k) { sx += Mj[k] * vx[k]; sy += Mj[k] * vy[k]; }
    uu += vx[j] * sx; uv += vx[j] * sy; vv += vy[j] * sy;
  }
  out[0] = uu; out[1] = uv; out[2] = vv;
}

// out[3] = (uu, uv, vv) of  a T^T b^T + its transpose,  T 12 x B by rows (ld doubles apart)
template <int B>
MVUS_HD void detcov_cross_form(const double* T, long long ld, const double* ax, const double* ay, const double* bx, const double* by, double* out) {
  double xx = 0.0, xy = 0.0, yx = 0.0, yy = 0.0;
  MVUS_DETCOV_ROLLED
  for (int r = 0; r < 12; ++r) {
    const double* Tr = T + (long long)r * ld;
    double qx = 0.0, qy = 0.0;
    for (int k = 0; k < B; ++k) { qx += Tr[k] * ax[k]; qy += Tr[k] * ay[k]; }
    xx += qx * bx[r]; xy += qx * by[r]; yx += qy * bx[r]; yy += qy * by[r];
  }
  out[0] = 2.0 * xx; out[1] = xy + yx; out[2] = 2.0 * yy;
}

// out[3] = (uu, uv, vv) of  b G b^T,  G the 12 x 12 matrix of control points p .. p + 3 read from the band blocks bp = band + p * 36:
// block (p + a, p + b), b >= a, is bp[a * 36 + (b - a) * 9 ..], the other triangle its transpose (an off-diagonal block counts twice)
MVUS_HD void detcov_band_form(const double* bp, const double* bx, const double* by, double* out) {
  double uu = 0.0, uv = 0.0, vv = 0.0;
  MVUS_DETCOV_ROLLED
  for (int a = 0; a < 4; ++a)
    MVUS_DETCOV_ROLLED
    for (int b = a; b < 4; ++b) {
      const double* blk = bp + a * 36 + (b - a) * 9;
      double xx = 0.0, xy = 0.0, yx = 0.0, yy = 0.0;
      for (int r = 0; r < 3; ++r) {
        const double gx = blk[3 * r] * bx[3 * b] + blk[3 * r + 1] * bx[3 * b + 1] + blk[3 * r + 2] * bx[3 * b + 2];
        const double gy = blk[3 * r] * by[3 * b] + blk[3 * r + 1] * by[3 * b + 1] + blk[3 * r + 2] * by[3 * b + 2];
        xx += bx[3 * a + r] * gx; xy += bx[3 * a + r] * gy; yx += by[3 * a + r] * gx; yy += by[3 * a + r] * gy;
      }
      if (b == a) { uu += xx; uv += 0.5 * (xy + yx); vv += yy; }
      else { uu += 2.0 * xx; uv += xy + yx; vv += 2.0 * yy; }
    }
  out[0] = uu; out[1] = uv; out[2] = vv;
}

// Pi / sigma^2 = (uu, uv, vv) in the row frame; terms[9] (may be null): the three terms, for the tests
template <int B>
MVUS_HD void detcov_row(const double* ax, const double* ay, const double* bx, const double* by, const double* Scc, long long lds,
                        const double* T, long long ldt, const double* bp, double* pi, double* terms) {
  double t1[3], t2[3], t3[3];
  detcov_sym_form<B>(Scc, lds, ax, ay, t1);
  detcov_cross_form<B>(T, ldt, ax, ay, bx, by, t2);
  detcov_band_form(bp, bx, by, t3);
  for (int k = 0; k < 3; ++k) {
    pi[k] = (t1[k] - t2[k]) + t3[k];
    if (terms) { terms[k] = t1[k]; terms[3 + k] = t2[k]; terms[6 + k] = t3[k]; }
  }
}

// P = D Pi D in image axes, D = diag(su, sv) (+-1): only the off-diagonal entry can change sign
MVUS_HD void detcov_image_axes(const double* pi, double su, double sv, double* p) {
  p[0] = pi[0]; p[1] = (su * sv) * pi[1]; p[2] = pi[2];
}

// t^2 = r^T (sigma^2 I - Pi)^-1 r, r = (ru, rv) the absolute residuals, Pi = (uu, uv, vv) already scaled by sigma^2; NaN unless
// sigma^2 I - Pi is positive definite (Sylvester: both leading minors > 0)
MVUS_HD double detcov_t2(const double* pi, double sigma2, double ru, double rv) {
  const double q11 = sigma2 - pi[0], q12 = -pi[1], q22 = sigma2 - pi[2];
  const double det = q11 * q22 - q12 * q12;
  if (!(q11 > 0.0) || !(det > 0.0)) return std::numeric_limits<double>::quiet_NaN();
  return ((ru * ru) * q22 - 2.0 * (ru * rv) * q12 + (rv * rv) * q11) / det;
}

}  // namespace mvus
