// Kinematics of a trajectory spline (spline_ops.hip.h: k_spline_eval_der, k_spline_kin_cov_eval, k_span_length, k_spline_length), written
// once for the device and for the host build that pins it (tests/hostcheck/kin_hostcheck.cpp): the four cubic B-splines of a knot span
// with their first and second derivatives, the covariance of the state (X, X', X'') of one sample from the control points' band, the
// 1-sigma of the speed, and the length of the curve inside one knot span.  Plain C++, no device intrinsics.
#pragma once
#include "ba_math.h"

namespace mvus {

// ---- basis and derivatives ------------------------------------------------------------------------------------------------------
// FITPACK fpbspl.f for k = 3 as bspline_basis_w<true> runs it -- h and dh are its expressions, term for term -- keeping the two linear
// B-splines of the span as well: by the derivative formula (FITPACK splder.f / fpader.f) applied twice
//   B'_{m,2}  = 2 [ B_{m,1} / (t_{m+2} - t_m) - B_{m+1,1} / (t_{m+3} - t_{m+1}) ]
//   B''_{i,3} = 3 [ B'_{i,2} / (t_{i+3} - t_i) - B'_{i+1,2} / (t_{i+4} - t_{i+1}) ].
// tt[j] = t[l-2+j] with l from find_span (t[l] <= x < t[l+1], clamped at the end): on a knot the derivatives are those from the right,
// at the last knot of the spline those from the left, as scipy's splev(der=) gives them.
MVUS_HD void bspline_basis_d2_w(const double tt[6], double x, double h[4], double dh[4], double ddh[4]) {
  double hh[3];
  h[0] = 1.0;
  double lin[2] = {0.0, 0.0};     // linear basis B_{l-1,1}, B_{l,1}
  double q[3] = {0.0, 0.0, 0.0};  // quadratic basis B_{l-2,2}, B_{l-1,2}, B_{l,2}
  for (int j = 1; j <= 3; ++j) {
    for (int i = 0; i < j; ++i) hh[i] = h[i];
    h[0] = 0.0;
    for (int i = 0; i < j; ++i) {
      const double tli = tt[i + 3], tlj = tt[i + 3 - j];          // t[l+i+1], t[l+i+1-j]
      const double f = hh[i] / (tli - tlj);
      h[i] = h[i] + f * (tli - x);
      h[i + 1] = f * (x - tlj);
    }
    if (j == 1) { lin[0] = h[0]; lin[1] = h[1]; }
    if (j == 2) { q[0] = h[0]; q[1] = h[1]; q[2] = h[2]; }
  }
  const double e0 = 3.0 * q[0] / (tt[3] - tt[0]);
  const double e1 = 3.0 * q[1] / (tt[4] - tt[1]);
  const double e2 = 3.0 * q[2] / (tt[5] - tt[2]);
  dh[0] = -e0; dh[1] = e0 - e1; dh[2] = e1 - e2; dh[3] = e2;
  // B'_{l-2,2}, B'_{l-1,2}, B'_{l,2} = -g0, g0 - g1, g1 (B_{l-2,1} and B_{l+1,1} vanish on the span)
  const double g0 = 2.0 * lin[0] / (tt[3] - tt[1]);
  const double g1 = 2.0 * lin[1] / (tt[4] - tt[2]);
  const double f0 = 3.0 * (-g0) / (tt[3] - tt[0]);
  const double f1 = 3.0 * (g0 - g1) / (tt[4] - tt[1]);
  const double f2 = 3.0 * g1 / (tt[5] - tt[2]);
  ddh[0] = -f0; ddh[1] = f0 - f1; ddh[2] = f1 - f2; ddh[3] = f2;
}
MVUS_HD void bspline_basis_d2(const double* t, int l, double x, double h[4], double dh[4], double ddh[4]) {
  double tt[6];
  for (int j = 0; j < 6; ++j) tt[j] = t[l - 2 + j];
  bspline_basis_d2_w(tt, x, h, dh, ddh);
}

// ---- covariance of the state of one sample ----------------------------------------------------------------------------------------
// State (X, X', .., D^NDER X), D = 3 (NDER + 1) components, component 3 i + r = coordinate r of the i-th derivative:
//   Cov(D^i X, D^j X) = sum_{a, b} H[i][a] H[j][b] Sigma(p + a, p + b),   H[0] = h, H[1] = dh, H[2] = ddh  (H[4 * i + a]),
// from the four band rows cov_spline_sample reads (bp = band + p * 36; block (p + a, p + b), b >= a, at bp[a * 36 + (b - a) * 9 ..], the
// other triangle its transpose), the blocks taken in that routine's order.  ONE triangle is computed: tri[kin_tri(D, P, Q)], P <= Q.
constexpr int kin_dim(int nder) { return 3 * (nder + 1); }
constexpr int kin_tri_count(int nder) { return kin_dim(nder) * (kin_dim(nder) + 1) / 2; }
MVUS_HD int kin_tri(int D, int P, int Q) { return P * D - P * (P - 1) / 2 + (Q - P); }       // P <= Q
template <int NDER>
MVUS_HD void kin_state_cov_tri(const double* H, const double* bp, double* tri) {
  constexpr int D = kin_dim(NDER);
#pragma unroll
  for (int e = 0; e < kin_tri_count(NDER); ++e) tri[e] = 0.0;
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = a; b < 4; ++b) {
      const double* blk = bp + a * 36 + (b - a) * 9;
#pragma unroll
      for (int P = 0; P < D; ++P)
#pragma unroll
        for (int Q = P; Q < D; ++Q) {
          const int i = P / 3, r = P % 3, j = Q / 3, c = Q % 3, e = kin_tri(D, P, Q);
          tri[e] += H[4 * i + a] * H[4 * j + b] * blk[3 * r + c];
          if (b > a) tri[e] += H[4 * i + b] * H[4 * j + a] * blk[3 * c + r];
        }
    }
}
// the full matrix, row-major out[D * D]: the triangle mirrored, so exactly symmetric
template <int NDER>
MVUS_HD void kin_state_cov(const double* H, const double* bp, double* out) {
  constexpr int D = kin_dim(NDER);
  double tri[kin_tri_count(NDER)];
  kin_state_cov_tri<NDER>(H, bp, tri);
  for (int P = 0; P < D; ++P)
    for (int Q = P; Q < D; ++Q) { out[P * D + Q] = tri[kin_tri(D, P, Q)]; out[Q * D + P] = tri[kin_tri(D, P, Q)]; }
}

// ---- speed ------------------------------------------------------------------------------------------------------------------------
MVUS_HD double kin_speed(double vx, double vy, double vz) { return sqrt(vx * vx + vy * vy + vz * vz); }
// 1-sigma of s = |X'| by first-order propagation: u = X' / s, sigma_s^2 = u^T Cov(X') u.  C: the 3 x 3 velocity block, rows ld apart.
// NaN when s == 0 (the direction is undefined there).
MVUS_HD double kin_speed_std(const double v[3], const double* C, int ld) {
  const double s = kin_speed(v[0], v[1], v[2]);
  if (s == 0.0) return __builtin_nan("");
  const double u[3] = {v[0] / s, v[1] / s, v[2] / s};
  double var = 0.0;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) var += u[r] * C[r * ld + c] * u[c];
  return sqrt(var);
}

// ---- length of the curve inside one knot span -------------------------------------------------------------------------------------
// int_a^b |X'(tau)| dtau, t[l] <= a <= b <= t[l+1]: tt the knot window of span l, cx / cy / cz its four coefficients per coordinate.
// 8-point Gauss-Legendre rule on [-1, 1] (exact for polynomials of degree 15), the nodes summed in ascending order; b == a gives exactly 0.
MVUS_HD double kin_span_length(const double tt[6], const double* cx, const double* cy, const double* cz, double a, double b) {
  const double kGL8x[8] = {-0.96028985649753623168, -0.79666647741362673959, -0.52553240991632898582, -0.18343464249564980494,
                           0.18343464249564980494,  0.52553240991632898582,  0.79666647741362673959,  0.96028985649753623168};
  const double kGL8w[8] = {0.10122853629037625915, 0.22238103445337447054, 0.31370664587788728734, 0.36268378337836198297,
                           0.36268378337836198297, 0.31370664587788728734, 0.22238103445337447054, 0.10122853629037625915};
  const double half = 0.5 * (b - a), mid = 0.5 * (a + b);
  double sum = 0.0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    double h[4], dh[4];
    bspline_basis_w<true>(tt, mid + half * kGL8x[k], h, dh);
    double vx = 0.0, vy = 0.0, vz = 0.0;
    for (int q = 0; q < 4; ++q) { vx = vx + cx[q] * dh[q]; vy = vy + cy[q] * dh[q]; vz = vz + cz[q] * dh[q]; }
    sum = sum + kGL8w[k] * kin_speed(vx, vy, vz);
  }
  return half * sum;
}
// the part of span l (t[l] .. t[l+1]) of spline (t, n coefficients per coordinate in c = cx(n) cy(n) cz(n)) that lies inside [lo, hi]
// and left of x: its length, 0 when that part is empty (a span of no width among them)
MVUS_HD double kin_span_part(const double* t, int n, const double* c, int l, double lo, double hi, double x) {
  const double a = t[l] > lo ? t[l] : lo;
  double b = t[l + 1] < hi ? t[l + 1] : hi;
  if (x < b) b = x;
  if (!(b > a)) return 0.0;
  double tt[6];
  for (int j = 0; j < 6; ++j) tt[j] = t[l - 2 + j];
  const double* cc = c + (l - 3);
  return kin_span_length(tt, cc, cc + n, cc + 2 * n, a, b);
}

}  // namespace mvus
