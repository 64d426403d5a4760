// Two-view geometry of Scene.init_traj and synchronization.sync_bf (reference common.py:178-221, synchronization.py:133-178):
// the three OpenCV calls they make -- cv2.findFundamentalMat(p1, p2, FM_RANSAC, thresh), cv2.correctMatches(F, p1, p2) -- and
// the cheirality test of epipolar.triangulate_from_E (epipolar.py:568-588).  OpenCV is a third-party dependency that is absent
// from this image, so there is no reference output to pin against ("parity unpinned"): what is restated is the
// published contract of each call with OpenCV 4's defaults.
//
//   findFundamentalMat(FM_RANSAC): confidence 0.99, at most 1000 iterations; minimal samples of 7 pairs solved by the 7-point
//   algorithm (up to 3 models each), scored by the number of pairs whose error -- the larger of the two squared distances of a
//   point to the epipolar line of its partner -- is <= thresh^2; the best model is refitted by the normalised 8-point algorithm
//   on its inliers.  The mapping onto the GPU is this build's own, as for PnP (pnp.hip.h):
//     k_fm_normalise   one workgroup per problem: Hartley normalisation (centroid, mean distance sqrt(2)) of both views by a
//                      fixed-order reduction (per-lane strided sums, wave shuffles, four wave partials summed in order)
//     k_fm_hypotheses  one lane per (problem, hypothesis): 7 distinct indices from the counter-based sampler fm_sample7 (the
//                      same draw on the host and in a batched or single call), the 7-point algorithm in normalised
//                      coordinates -- the 2-D null space of the 7x9 system by Gauss-Jordan elimination with full pivoting,
//                      then the real roots of the cubic det(l F1 + (1-l) F2) (fm_cubic_roots) -- and up to 3 denormalised models; empty
//                      slots are marked invalid.  All hypotheses are evaluated: there is no adaptive early stop.
//     k_fm_score       one lane per model, the problem's pairs streamed through LDS in tiles (broadcast reads); the inlier
//                      count stays in a register, so no reduction.  fp64 with contraction off: the count is the oracle's.
//     k_fm_refit       the 9x9 normal matrix of the 8-point system over the winner's inliers (normalised coordinates), as
//                      per-block partials summed in a fixed order on the host, plus the winner's inlier mask; the smallest
//                      eigenvector and the rank-2 projection are computed on the host (mvus_fundamental_ransac)
//     k_fm_mask        inlier mask and per-block integer counts of the refitted matrix; it replaces the winner only when it
//                      keeps at least as many inliers.
//   Selection: the highest count wins, the lowest model index breaks ties.
//
//   correctMatches: Hartley & Zisserman, Algorithm 12.1 (optimal triangulation), one lane per pair (k_correct_matches): both
//   points moved to the origin, the epipoles rotated onto the x axis, the real roots of the degree-6 polynomial g(t) found by
//   Aberth iteration and polished by Newton steps, the cost evaluated at each of them and at t = infinity, the points on the two
//   epipolar lines of the minimum closest to the origin, mapped back.  Non-finite input gives NaN output; nothing else does.
//
//   triangulate_from_E: the four (R, t) candidates (decomposed on the host) in one launch (k_cheirality4): every pair
//   triangulated with the lane routine of triangulate.hip.h in normalised coordinates, P1 = [I|0], and the points in front
//   of each camera counted as per-block integer partials.  The winner is chosen on the host exactly as the reference does
//   (first candidate whose count exceeds the running maximum) and triangulated with k_triangulate.
#pragma once
#include <cfloat>
#include <cmath>
#include <cstdint>

#include "ba_math.h"
#include "pnp.hip.h"           // pnp_mix
#include "triangulate.hip.h"

namespace mvus {

MVUS_HD bool fm_finite(double x) { return std::isfinite(x); }

constexpr int kFmSlots = 3;    // models per 7-point hypothesis
constexpr int kFmModel = 10;   // doubles per model slot: F (9, row-major, pixel coordinates) and a valid flag

// the seven distinct sample indices of hypothesis h among N pairs (counter based: the same on every run, in every batch, on the host)
MVUS_HD void fm_sample7(unsigned long long seed, int h, long long N, long long* idx) {
  unsigned long long ctr = seed * 0x100000001b3ull + (unsigned long long)h * 1000003ull + 0x5851f42d4c957f2dull;
  for (int k = 0; k < 7;) {
    ctr = pnp_mix(ctr);
    const long long c = (long long)(ctr % (unsigned long long)N);
    bool dup = false;
    for (int j = 0; j < k; ++j) dup |= idx[j] == c;
    if (!dup) idx[k++] = c;
  }
}

// OpenCV's error of a fundamental matrix on one pair: max of the squared distances of each point to its epipolar line.
// Contraction off: the host oracle evaluates the same expression in the same order, without fused multiply-adds.
MVUS_HD double fm_error(const double* F, double x1, double y1, double x2, double y2) {
#pragma clang fp contract(off)
  double a = F[0] * x1 + F[1] * y1 + F[2];
  double b = F[3] * x1 + F[4] * y1 + F[5];
  double c = F[6] * x1 + F[7] * y1 + F[8];
  const double s2 = 1.0 / (a * a + b * b);
  const double d2 = x2 * a + y2 * b + c;
  a = F[0] * x2 + F[3] * y2 + F[6];
  b = F[1] * x2 + F[4] * y2 + F[7];
  c = F[2] * x2 + F[5] * y2 + F[8];
  const double s1 = 1.0 / (a * a + b * b);
  const double d1 = x1 * a + y1 * b + c;
  const double e1 = d1 * d1 * s1, e2 = d2 * d2 * s2;
  return e1 > e2 ? e1 : e2;
}

// one row of the epipolar constraint x2^T F x1 = 0 in the unknowns F (row-major)
MVUS_HD void fm_row(double x1, double y1, double x2, double y2, double* r) {
  r[0] = x2 * x1; r[1] = x2 * y1; r[2] = x2; r[3] = y2 * x1; r[4] = y2 * y1; r[5] = y2; r[6] = x1; r[7] = y1; r[8] = 1.0;
}

// F <- T2^T F T1 with T = [s 0 -s cx; 0 s -s cy; 0 0 1] (norm: cx1 cy1 s1 cx2 cy2 s2), then unit Frobenius norm, F[8] >= 0
MVUS_HD void fm_denormalise(const double* Fn, const double* norm, double* F) {
  const double T1[9] = {norm[2], 0.0, -norm[2] * norm[0], 0.0, norm[2], -norm[2] * norm[1], 0.0, 0.0, 1.0};
  const double T2[9] = {norm[5], 0.0, -norm[5] * norm[3], 0.0, norm[5], -norm[5] * norm[4], 0.0, 0.0, 1.0};
  double M[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) M[3 * i + j] = Fn[3 * i] * T1[j] + Fn[3 * i + 1] * T1[3 + j] + Fn[3 * i + 2] * T1[6 + j];
  double nn = 0.0;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      F[3 * i + j] = T2[i] * M[j] + T2[3 + i] * M[3 + j] + T2[6 + i] * M[6 + j];
      nn += F[3 * i + j] * F[3 * i + j];
    }
  double sc = nn > 0.0 ? 1.0 / sqrt(nn) : 0.0;
  if (F[8] < 0.0) sc = -sc;
  for (int a = 0; a < 9; ++a) F[a] *= sc;
}

MVUS_HD double fm_cubic_eval(double c3, double c2, double c1, double c0, double x) { return ((c3 * x + c2) * x + c1) * x + c0; }

// Real roots of q2 x^2 + q1 x + q0 (q2 != 0) by the stable formula.  A discriminant within 16 eps (q1^2 + 4 |q2 q0|) of zero --
// a bound on its own rounding error -- is a double root -q1 / (2 q2), returned once.  The coefficients are first scaled by a
// power of two (exact: the same bits wherever nothing under- or overflows) so that the largest is in [1, 2): the squares can
// neither underflow nor overflow.
MVUS_HD int fm_quadratic_roots(double q2, double q1, double q0, double* r) {
  const int e = ilogb(fmax(fabs(q2), fmax(fabs(q1), fabs(q0))));
  q2 = ldexp(q2, -e); q1 = ldexp(q1, -e); q0 = ldexp(q0, -e);
  const double disc = q1 * q1 - 4.0 * q2 * q0, tol = 16.0 * DBL_EPSILON * (q1 * q1 + 4.0 * fabs(q2 * q0));
  if (disc < -tol) return 0;
  if (disc <= tol) { r[0] = -0.5 * q1 / q2; return 1; }
  const double q = -0.5 * (q1 + (q1 >= 0.0 ? sqrt(disc) : -sqrt(disc)));
  r[0] = q / q2;
  if (q == 0.0) return 1;
  r[1] = q0 / q;
  return 2;
}

// two Newton steps on each of r[0..n), a step kept only when it does not increase |cubic| (near a double root f' is rounding
// noise and an unguarded step can jump off the pair)
MVUS_HD void fm_cubic_polish(double c3, double c2, double c1, double c0, double* r, int n) {
  for (int k = 0; k < n; ++k)
    for (int it = 0; it < 2; ++it) {
      const double x = r[k];
      const double f = fm_cubic_eval(c3, c2, c1, c0, x), df = (3.0 * c3 * x + 2.0 * c2) * x + c1;
      if (df == 0.0) break;
      const double xn = x - f / df;
      if (!fm_finite(xn) || !(fabs(fm_cubic_eval(c3, c2, c1, c0, xn)) <= fabs(f))) break;
      r[k] = xn;
    }
}

// Real roots of c3 l^3 + c2 l^2 + c1 l + c0 (at most 3).  |c3| <= 1e-12 max|c|: the quadratic (or linear) polynomial.  Otherwise
// one real root x0 by the closed form -- the largest in magnitude of the three of the trigonometric formula when R^2 < Q^3, else
// A + B - a/3 -- polished, then the cubic deflated by it (from the constant term when x0 is the largest root in magnitude, from
// the leading term otherwise) and the quadratic's roots by fm_quadratic_roots.  The closed form alone loses roots: a double or
// near-double pair that rounding moves to the R^2 >= Q^3 side, and the small roots next to a huge one (|c3| just above the
// cutoff), where cancellation against a/3 leaves no correct digit.  Every root is polished by fm_cubic_polish.
//
// delta: the absolute uncertainty of the coefficients (0: exact).  When the deflated quadratic has a complex pair m +- i y and m
// is a root of the cubic to within that uncertainty, |cubic(m)| <= delta (|m|^3 + |m|^2 + |m| + 1), the pair is a double root
// split by the coefficients' errors (|y| ~ sqrt(delta)), and m is returned as one root.
MVUS_HD int fm_cubic_roots(double c3, double c2, double c1, double c0, double* r, double delta = 0.0) {
  const double mx = fmax(fmax(fabs(c3), fabs(c2)), fmax(fabs(c1), fabs(c0)));
  if (!(mx > 0.0)) return 0;
  if (fabs(c3) <= 1e-12 * mx) {
    if (fabs(c2) <= 1e-12 * mx) {
      if (fabs(c1) <= 1e-12 * mx) return 0;
      r[0] = -c0 / c1;
      fm_cubic_polish(c3, c2, c1, c0, r, 1);
      return 1;
    }
    const int n = fm_quadratic_roots(c2, c1, c0, r);
    fm_cubic_polish(c3, c2, c1, c0, r, n);
    return n;
  }
  const double a = c2 / c3, b = c1 / c3, c = c0 / c3;
  const double Q = (a * a - 3.0 * b) / 9.0, R = (2.0 * a * a * a - 9.0 * a * b + 27.0 * c) / 54.0;
  const double Q3 = Q * Q * Q;
  double x0;
  if (R * R < Q3) {
    const double th = acos(fmin(1.0, fmax(-1.0, R / sqrt(Q3)))), sq = -2.0 * sqrt(Q);
    x0 = sq * cos(th / 3.0) - a / 3.0;
    const double t1 = sq * cos((th + 2.0 * M_PI) / 3.0) - a / 3.0, t2 = sq * cos((th - 2.0 * M_PI) / 3.0) - a / 3.0;
    if (fabs(t1) > fabs(x0)) x0 = t1;
    if (fabs(t2) > fabs(x0)) x0 = t2;
  } else {
    double A = cbrt(fabs(R) + sqrt(R * R - Q3));
    if (R > 0.0) A = -A;
    const double B = A != 0.0 ? Q / A : 0.0;
    x0 = A + B - a / 3.0;
  }
  r[0] = x0;
  fm_cubic_polish(c3, c2, c1, c0, r, 1);
  x0 = r[0];
  double q1, q0;
  if (x0 != 0.0 && fabs(x0) * x0 * x0 * fabs(c3) >= fabs(c0)) { q0 = -c0 / x0; q1 = (q0 - c1) / x0; }
  else { q1 = c2 + c3 * x0; q0 = c1 + q1 * x0; }
  int m = fm_quadratic_roots(c3, q1, q0, r + 1);
  if (m == 0 && delta > 0.0) {
    const double xm = -0.5 * (q1 / c3), ax = fabs(xm);
    if (fabs(fm_cubic_eval(c3, c2, c1, c0, xm)) <= delta * (((ax + 1.0) * ax + 1.0) * ax + 1.0)) { r[1] = xm; m = 1; }
  }
  fm_cubic_polish(c3, c2, c1, c0, r + 1, m);
  return 1 + m;
}

MVUS_HD double fm_det3(const double* A) {
  return A[0] * (A[4] * A[8] - A[5] * A[7]) - A[1] * (A[3] * A[8] - A[5] * A[6]) + A[2] * (A[3] * A[7] - A[4] * A[6]);
}

MVUS_HD double fm_perm3_abs(const double* A) {
  const double a0 = fabs(A[0]), a1 = fabs(A[1]), a2 = fabs(A[2]), a3 = fabs(A[3]), a4 = fabs(A[4]), a5 = fabs(A[5]);
  const double a6 = fabs(A[6]), a7 = fabs(A[7]), a8 = fabs(A[8]);
  return a0 * (a4 * a8 + a5 * a7) + a1 * (a3 * a8 + a5 * a6) + a2 * (a3 * a7 + a4 * a6);
}

// The 7-point algorithm on normalised pairs xs[7][4] = (x1 y1 x2 y2): up to 3 normalised models Fs[k][9]; returns their number.
MVUS_HD int fm_seven_point(const double (*xs)[4], double (*Fs)[9]) {
  double A[7][9];
  int perm[9];
  for (int j = 0; j < 9; ++j) perm[j] = j;
  double amax = 0.0;
  for (int i = 0; i < 7; ++i) {
    fm_row(xs[i][0], xs[i][1], xs[i][2], xs[i][3], A[i]);
    for (int j = 0; j < 9; ++j) amax = fmax(amax, fabs(A[i][j]));
  }
  if (!(amax > 0.0)) return 0;
  // Gauss-Jordan with full pivoting: A -> [I | B] in permuted columns
  for (int k = 0; k < 7; ++k) {
    int pi = k, pj = k;
    double best = -1.0;
    for (int i = k; i < 7; ++i)
      for (int j = k; j < 9; ++j)
        if (fabs(A[i][j]) > best) { best = fabs(A[i][j]); pi = i; pj = j; }
    if (!(best > 1e-10 * amax)) return 0;                                     // rank < 7: a degenerate sample
    if (pi != k) for (int j = 0; j < 9; ++j) { const double t = A[k][j]; A[k][j] = A[pi][j]; A[pi][j] = t; }
    if (pj != k) {
      for (int i = 0; i < 7; ++i) { const double t = A[i][k]; A[i][k] = A[i][pj]; A[i][pj] = t; }
      const int t = perm[k]; perm[k] = perm[pj]; perm[pj] = t;
    }
    const double ip = 1.0 / A[k][k];
    for (int j = k; j < 9; ++j) A[k][j] *= ip;
    for (int i = 0; i < 7; ++i) {
      if (i == k) continue;
      const double f = A[i][k];
      if (f != 0.0) for (int j = k; j < 9; ++j) A[i][j] -= f * A[k][j];
    }
  }
  double F1[9], F2[9];
  for (int i = 0; i < 7; ++i) { F1[perm[i]] = -A[i][7]; F2[perm[i]] = -A[i][8]; }
  F1[perm[7]] = 1.0; F1[perm[8]] = 0.0;
  F2[perm[7]] = 0.0; F2[perm[8]] = 1.0;
  // det(l F1 + (1 - l) F2) = c3 l^3 + c2 l^2 + c1 l + c0 from its values at l = 0, 1, -1, 2
  // delta: a bound on the coefficients' rounding errors, 128 eps times the largest permanent of |M| (the size of the terms of
  // the determinants) -- a double root of the exact sample must not be lost to them
  double M[9], dv[4], pmax = 0.0;
  const double ls[4] = {0.0, 1.0, -1.0, 2.0};
  for (int q = 0; q < 4; ++q) {
    for (int a = 0; a < 9; ++a) M[a] = ls[q] * F1[a] + (1.0 - ls[q]) * F2[a];
    dv[q] = fm_det3(M);
    pmax = fmax(pmax, fm_perm3_abs(M));
  }
  const double c0 = dv[0], c2 = 0.5 * (dv[1] + dv[2]) - c0, s = 0.5 * (dv[1] - dv[2]);
  const double c3 = (dv[3] - 4.0 * c2 - c0 - 2.0 * s) / 6.0, c1 = s - c3;
  double roots[3];
  const int nr = fm_cubic_roots(c3, c2, c1, c0, roots, 128.0 * DBL_EPSILON * pmax);
  int n = 0;
  for (int k = 0; k < nr; ++k) {
    const double l = roots[k];
    if (!fm_finite(l)) continue;
    double nn = 0.0;
    for (int a = 0; a < 9; ++a) { Fs[n][a] = l * F1[a] + (1.0 - l) * F2[a]; nn += Fs[n][a] * Fs[n][a]; }
    if (!(nn > 0.0) || !fm_finite(nn)) continue;
    ++n;
  }
  return n;
}

// ---- Hartley-Sturm (H&Z Algorithm 12.1) -------------------------------------------------------------------------------------
// g(t) = t ((a t + b)^2 + f2^2 (c t + d)^2)^2 - (a d - b c) (1 + f1^2 t^2)^2 (a t + b)(c t + d); coefficients ascending, 7 of them
MVUS_HD void hs_poly(double a, double b, double c, double d, double f1, double f2, double* g) {
  const double q0 = b * b + f2 * f2 * d * d, q1 = 2.0 * (a * b + f2 * f2 * c * d), q2 = a * a + f2 * f2 * c * c;   // (at+b)^2 + f2^2 (ct+d)^2
  const double qq[5] = {q0 * q0, 2.0 * q0 * q1, q1 * q1 + 2.0 * q0 * q2, 2.0 * q1 * q2, q2 * q2};
  const double f12 = f1 * f1;
  const double rr[5] = {1.0, 0.0, 2.0 * f12, 0.0, f12 * f12};                                                     // (1 + f1^2 t^2)^2
  const double pp[3] = {b * d, a * d + b * c, a * c};                                                              // (at+b)(ct+d)
  const double k = a * d - b * c;
  for (int i = 0; i < 7; ++i) g[i] = 0.0;
  for (int i = 0; i < 5; ++i) g[i + 1] += qq[i];
  for (int i = 0; i < 5; ++i)
    for (int j = 0; j < 3; ++j) g[i + j] -= k * rr[i] * pp[j];
}

MVUS_HD double hs_cost(double t, double a, double b, double c, double d, double f1, double f2) {
  const double ct = c * t + d, at = a * t + b;
  return t * t / (1.0 + f1 * f1 * t * t) + ct * ct / (at * at + f2 * f2 * ct * ct);
}

// real parts of all roots of g (degree <= 6, leading zeros trimmed) by Aberth iteration, each polished by Newton steps on g.
// Evaluating the cost at the real parts of complex roots too is harmless: the minimum over a superset of the real stationary
// points is the same minimum.  Returns the number of candidates written to ts.
MVUS_HD int hs_real_candidates(const double* g_in, double* ts) {
  double mx = 0.0;
  for (int i = 0; i < 7; ++i) mx = fmax(mx, fabs(g_in[i]));
  if (!(mx > 0.0) || !fm_finite(mx)) return 0;
  double g[7];
  for (int i = 0; i < 7; ++i) g[i] = g_in[i] / mx;
  int n = 6;
  while (n > 0 && g[n] == 0.0) --n;
  if (n == 0) return 0;
  // initial radius from the coefficient ratios (Fujiwara's bound / 2), points on a circle off the real axis
  double rad = 0.0;
  for (int i = 0; i < n; ++i) rad = fmax(rad, pow(fabs(g[i] / g[n]), 1.0 / (double)(n - i)));
  rad = fmax(rad, 1e-12);
  double zr[6], zi[6];
  for (int k = 0; k < n; ++k) { const double an = 2.0 * M_PI * k / n + 0.4; zr[k] = rad * cos(an); zi[k] = rad * sin(an); }
  for (int it = 0; it < 200; ++it) {
    double wmax = 0.0;
    for (int k = 0; k < n; ++k) {
      double pr = g[n], pi = 0.0, dr = 0.0, di = 0.0;                          // Horner: p and p'
      for (int i = n - 1; i >= 0; --i) {
        const double ndr = dr * zr[k] - di * zi[k] + pr, ndi = dr * zi[k] + di * zr[k] + pi;
        dr = ndr; di = ndi;
        const double npr = pr * zr[k] - pi * zi[k] + g[i], npi = pr * zi[k] + pi * zr[k];
        pr = npr; pi = npi;
      }
      const double dd = dr * dr + di * di;
      if (!(dd > 0.0)) continue;
      const double qr = (pr * dr + pi * di) / dd, qi = (pi * dr - pr * di) / dd;      // p / p'
      double sr = 0.0, si = 0.0;
      for (int j = 0; j < n; ++j) {
        if (j == k) continue;
        const double ur = zr[k] - zr[j], ui = zi[k] - zi[j], uu = ur * ur + ui * ui;
        if (uu > 0.0) { sr += ur / uu; si -= ui / uu; }
      }
      // w = q / (1 - q s)
      const double er = 1.0 - (qr * sr - qi * si), ei = -(qr * si + qi * sr), ee = er * er + ei * ei;
      if (!(ee > 0.0)) continue;
      const double wr = (qr * er + qi * ei) / ee, wi = (qi * er - qr * ei) / ee;
      if (!fm_finite(wr) || !fm_finite(wi)) continue;
      zr[k] -= wr; zi[k] -= wi;
      wmax = fmax(wmax, sqrt(wr * wr + wi * wi) / fmax(1.0, sqrt(zr[k] * zr[k] + zi[k] * zi[k])));
    }
    if (wmax < 1e-15) break;
  }
  for (int k = 0; k < n; ++k) {
    double t = zr[k];
    for (int it = 0; it < 4; ++it) {
      double p = g[n], dp = 0.0;
      for (int i = n - 1; i >= 0; --i) { dp = dp * t + p; p = p * t + g[i]; }
      if (dp == 0.0) break;
      const double tn = t - p / dp;
      if (!fm_finite(tn)) break;
      double pn = g[n];
      for (int i = n - 1; i >= 0; --i) pn = pn * tn + g[i];
      if (fabs(pn) > fabs(p)) break;
      t = tn;
    }
    ts[k] = t;
  }
  return n;
}

// Optimal correction of one pair under F (row-major) with the epipoles e1 (F e1 = 0) and e2 (e2^T F = 0) of F.
MVUS_HD void correct_pair(const double* F, const double* e1, const double* e2, double x1, double y1, double x2, double y2,
                          double* o1, double* o2) {
  if (!(fm_finite(x1) && fm_finite(y1) && fm_finite(x2) && fm_finite(y2))) { o1[0] = o1[1] = o2[0] = o2[1] = NAN; return; }
  // epipoles in the frames centred on the two points, scaled so that ex^2 + ey^2 = 1
  double a1 = e1[0] - x1 * e1[2], b1 = e1[1] - y1 * e1[2], c1 = e1[2];
  double a2 = e2[0] - x2 * e2[2], b2 = e2[1] - y2 * e2[2], c2 = e2[2];
  const double n1 = sqrt(a1 * a1 + b1 * b1), n2 = sqrt(a2 * a2 + b2 * b2);
  if (!(n1 > 0.0) || !(n2 > 0.0)) { o1[0] = x1; o1[1] = y1; o2[0] = x2; o2[1] = y2; return; }       // a point on its epipole
  a1 /= n1; b1 /= n1; c1 /= n1; a2 /= n2; b2 /= n2; c2 /= n2;
  // G = R2 T2^-T F T1^-1 R1^T; T^-1 = [1 0 x; 0 1 y; 0 0 1], R = [ex ey 0; -ey ex 0; 0 0 1]
  double M[9], G[9];
  for (int i = 0; i < 3; ++i) {                                                // M = F T1^-1
    M[3 * i] = F[3 * i]; M[3 * i + 1] = F[3 * i + 1]; M[3 * i + 2] = F[3 * i] * x1 + F[3 * i + 1] * y1 + F[3 * i + 2];
  }
  for (int j = 0; j < 3; ++j) M[6 + j] += x2 * M[j] + y2 * M[3 + j];          // T2^-T M: the last row gains x2 row0 + y2 row1
  for (int j = 0; j < 3; ++j) {                                                // R2 M
    const double r0 = a2 * M[j] + b2 * M[3 + j], r1 = -b2 * M[j] + a2 * M[3 + j];
    G[j] = r0; G[3 + j] = r1; G[6 + j] = M[6 + j];
  }
  for (int i = 0; i < 3; ++i) {                                                // G R1^T
    const double g0 = G[3 * i] * a1 + G[3 * i + 1] * b1, g1 = -G[3 * i] * b1 + G[3 * i + 1] * a1;
    G[3 * i] = g0; G[3 * i + 1] = g1;
  }
  const double f1 = c1, f2 = c2, a = G[4], b = G[5], c = G[7], d = G[8];
  double g[7], ts[6];
  hs_poly(a, b, c, d, f1, f2, g);
  const int nt = hs_real_candidates(g, ts);
  bool inf_best = false;
  double tbest = 0.0, sbest = hs_cost(0.0, a, b, c, d, f1, f2);
  for (int k = 0; k < nt; ++k) {
    const double s = hs_cost(ts[k], a, b, c, d, f1, f2);
    if (s < sbest) { sbest = s; tbest = ts[k]; }
  }
  if (f1 != 0.0) {
    const double sinf = 1.0 / (f1 * f1) + c * c / (a * a + f2 * f2 * c * c);
    if (sinf < sbest) inf_best = true;
  }
  double l1[3], l2[3];
  if (inf_best) { l1[0] = f1; l1[1] = 0.0; l1[2] = -1.0; l2[0] = -f2 * c; l2[1] = a; l2[2] = c; }
  else {
    const double t = tbest;
    l1[0] = t * f1; l1[1] = 1.0; l1[2] = -t;
    l2[0] = -f2 * (c * t + d); l2[1] = a * t + b; l2[2] = c * t + d;
  }
  // closest points of the lines to the origin, back through R^T and T^-1
  const double p1x = -l1[0] * l1[2], p1y = -l1[1] * l1[2], p1w = l1[0] * l1[0] + l1[1] * l1[1];
  const double p2x = -l2[0] * l2[2], p2y = -l2[1] * l2[2], p2w = l2[0] * l2[0] + l2[1] * l2[1];
  o1[0] = (a1 * p1x - b1 * p1y) / p1w + x1; o1[1] = (b1 * p1x + a1 * p1y) / p1w + y1;
  o2[0] = (a2 * p2x - b2 * p2y) / p2w + x2; o2[1] = (b2 * p2x + a2 * p2y) / p2w + y2;
}

#if defined(__HIPCC__)
__device__ __forceinline__ double fm_wave_sum(double v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}
__device__ __forceinline__ int fm_wave_sum_int(int v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// norm[6p..6p+5] = cx1 cy1 s1 cx2 cy2 s2 of problem p (s = 0: all points of a view coincide -- no model); one workgroup per problem
__global__ __launch_bounds__(256) void k_fm_normalise(const long long* __restrict__ offs, long long Ntot, const double* __restrict__ x1,
                                                      const double* __restrict__ x2, double* __restrict__ norm) {
  __shared__ double red[4][4];
  __shared__ double cen[4];
  const int p = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long o = offs[p], N = offs[p + 1] - o;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  for (long long i = threadIdx.x; i < N; i += 256) { s[0] += x1[o + i]; s[1] += x1[Ntot + o + i]; s[2] += x2[o + i]; s[3] += x2[Ntot + o + i]; }
  for (int k = 0; k < 4; ++k) { const double v = fm_wave_sum(s[k]); if (lane == 0) red[wave][k] = v; }
  __syncthreads();
  if (threadIdx.x < 4) cen[threadIdx.x] = (((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x]) / (double)N;
  __syncthreads();
  double d[2] = {0.0, 0.0};
  for (long long i = threadIdx.x; i < N; i += 256) {
    const double ax = x1[o + i] - cen[0], ay = x1[Ntot + o + i] - cen[1], bx = x2[o + i] - cen[2], by = x2[Ntot + o + i] - cen[3];
    d[0] += sqrt(ax * ax + ay * ay); d[1] += sqrt(bx * bx + by * by);
  }
  __syncthreads();
  for (int k = 0; k < 2; ++k) { const double v = fm_wave_sum(d[k]); if (lane == 0) red[wave][k] = v; }
  __syncthreads();
  if (threadIdx.x < 2) {
    const double md = (((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x]) / (double)N;
    const double sc = md > 0.0 ? sqrt(2.0) / md : 0.0;
    norm[6 * p + 3 * threadIdx.x] = cen[2 * threadIdx.x];
    norm[6 * p + 3 * threadIdx.x + 1] = cen[2 * threadIdx.x + 1];
    norm[6 * p + 3 * threadIdx.x + 2] = fm_finite(sc) ? sc : 0.0;
  }
}

// models[((p H + h) 3 + k) 10 + 0..9]: F (pixel coordinates, unit norm) and valid flag; grid (ceil(H / 64), P)
__global__ __launch_bounds__(64) void k_fm_hypotheses(int H, unsigned long long seed, const long long* __restrict__ offs, long long Ntot,
                                                      const double* __restrict__ x1, const double* __restrict__ x2,
                                                      const double* __restrict__ norm, double* __restrict__ models) {
  const int h = blockIdx.x * 64 + threadIdx.x, p = blockIdx.y;
  if (h >= H) return;
  const long long o = offs[p], N = offs[p + 1] - o;
  const double* nm = norm + 6 * p;
  double Fs[kFmSlots][9];
  int n = 0;
  if (nm[2] > 0.0 && nm[5] > 0.0) {
    long long idx[7];
    fm_sample7(seed, h, N, idx);
    double xs[7][4];
    for (int k = 0; k < 7; ++k) {
      const long long i = o + idx[k];
      xs[k][0] = (x1[i] - nm[0]) * nm[2]; xs[k][1] = (x1[Ntot + i] - nm[1]) * nm[2];
      xs[k][2] = (x2[i] - nm[3]) * nm[5]; xs[k][3] = (x2[Ntot + i] - nm[4]) * nm[5];
    }
    n = fm_seven_point(xs, Fs);
  }
  double* out = models + ((long long)p * H + h) * kFmSlots * kFmModel;
  for (int k = 0; k < kFmSlots; ++k) {
    double F[9];
    bool ok = k < n;
    if (ok) {
      fm_denormalise(Fs[k], nm, F);
      for (int a = 0; a < 9; ++a) ok = ok && fm_finite(F[a]);
    }
    for (int a = 0; a < 9; ++a) out[k * kFmModel + a] = ok ? F[a] : 0.0;
    out[k * kFmModel + 9] = ok ? 1.0 : 0.0;
  }
}

// counts[p 3H + m]: inliers of model m of problem p (-1: invalid slot); grid (ceil(3H / 256), P), the pairs through LDS
__global__ __launch_bounds__(256) void k_fm_score(int H, const long long* __restrict__ offs, long long Ntot, const double* __restrict__ x1,
                                                  const double* __restrict__ x2, const double* __restrict__ models, double thr2,
                                                  int32_t* __restrict__ counts) {
  __shared__ double tile[4][256];
  const int M = kFmSlots * H, p = blockIdx.y;
  const int m = blockIdx.x * 256 + threadIdx.x;
  const long long o = offs[p], N = offs[p + 1] - o;
  const bool live = m < M;
  double F[9];
  bool valid = false;
  if (live) {
    const double* md = models + ((long long)p * M + m) * kFmModel;
    for (int a = 0; a < 9; ++a) F[a] = md[a];
    valid = md[9] != 0.0;
  }
  int cnt = 0;
  for (long long base = 0; base < N; base += 256) {
    const long long i = base + threadIdx.x;
    __syncthreads();
    if (i < N) { tile[0][threadIdx.x] = x1[o + i]; tile[1][threadIdx.x] = x1[Ntot + o + i]; tile[2][threadIdx.x] = x2[o + i]; tile[3][threadIdx.x] = x2[Ntot + o + i]; }
    __syncthreads();
    const int nt = (int)(N - base < 256 ? N - base : 256);
    if (valid)
      for (int j = 0; j < nt; ++j) cnt += fm_error(F, tile[0][j], tile[1][j], tile[2][j], tile[3][j]) <= thr2 ? 1 : 0;
  }
  if (live) counts[(long long)p * M + m] = valid ? cnt : -1;
}

constexpr int kFmRefitBlocks = 32;   // workgroups per problem of k_fm_refit / k_fm_mask

// the winner's inlier mask, and per workgroup the upper triangle (45 entries) of the 8-point normal matrix over those inliers in
// normalised coordinates: parts[(p B + b) 45 + e]; grid (B, P)
__global__ __launch_bounds__(256) void k_fm_refit(const long long* __restrict__ offs, long long Ntot, const double* __restrict__ x1,
                                                  const double* __restrict__ x2, const double* __restrict__ norm, const double* __restrict__ Fwin,
                                                  double thr2, uint8_t* __restrict__ mask, double* __restrict__ parts) {
  __shared__ double red[4][45];
  const int p = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long o = offs[p], N = offs[p + 1] - o;
  const double* nm = norm + 6 * p;
  double F[9];
  for (int a = 0; a < 9; ++a) F[a] = Fwin[9 * p + a];
  double acc[45];
  for (int e = 0; e < 45; ++e) acc[e] = 0.0;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < N; i += 256ll * gridDim.x) {
    const double u1 = x1[o + i], v1 = x1[Ntot + o + i], u2 = x2[o + i], v2 = x2[Ntot + o + i];
    const bool in = fm_error(F, u1, v1, u2, v2) <= thr2;
    mask[o + i] = in ? 1 : 0;
    if (!in) continue;
    double r[9];
    fm_row((u1 - nm[0]) * nm[2], (v1 - nm[1]) * nm[2], (u2 - nm[3]) * nm[5], (v2 - nm[4]) * nm[5], r);
    int e = 0;
#pragma unroll
    for (int a = 0; a < 9; ++a)
#pragma unroll
      for (int b = a; b < 9; ++b) acc[e++] += r[a] * r[b];
  }
#pragma unroll
  for (int e = 0; e < 45; ++e) { const double v = fm_wave_sum(acc[e]); if (lane == 0) red[wave][e] = v; }
  __syncthreads();
  if (threadIdx.x < 45)
    parts[((long long)p * gridDim.x + blockIdx.x) * 45 + threadIdx.x] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

// inlier mask of F[9p..] and per-workgroup integer counts cnt[p B + b]; grid (B, P)
__global__ __launch_bounds__(256) void k_fm_mask(const long long* __restrict__ offs, long long Ntot, const double* __restrict__ x1,
                                                 const double* __restrict__ x2, const double* __restrict__ Fs, double thr2,
                                                 uint8_t* __restrict__ mask, int32_t* __restrict__ cnt) {
  __shared__ int red[4];
  const int p = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long o = offs[p], N = offs[p + 1] - o;
  double F[9];
  for (int a = 0; a < 9; ++a) F[a] = Fs[9 * p + a];
  int c = 0;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < N; i += 256ll * gridDim.x) {
    const bool in = fm_error(F, x1[o + i], x1[Ntot + o + i], x2[o + i], x2[Ntot + o + i]) <= thr2;
    mask[o + i] = in ? 1 : 0;
    c += in ? 1 : 0;
  }
  c = fm_wave_sum_int(c);
  if (lane == 0) red[wave] = c;
  __syncthreads();
  if (threadIdx.x == 0) cnt[(long long)p * gridDim.x + blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

struct EpiF { double F[9], e1[3], e2[3]; };      // by value in the kernel arguments: wave-uniform

// x: [2][N] (u row, v row) per view; xc likewise
__global__ __launch_bounds__(256) void k_correct_matches(EpiF f, long long N, const double* __restrict__ x1, const double* __restrict__ x2,
                                                         double* __restrict__ x1c, double* __restrict__ x2c) {
  const long long i = blockIdx.x * 256ll + threadIdx.x;
  if (i >= N) return;
  double o1[2], o2[2];
  correct_pair(f.F, f.e1, f.e2, x1[i], x1[N + i], x2[i], x2[N + i], o1, o2);
  x1c[i] = o1[0]; x1c[N + i] = o1[1]; x2c[i] = o2[0]; x2c[N + i] = o2[1];
}

struct EpiCand { double P2[4][12]; };

// points in front of both cameras for each of the four candidates: cnt[c B + b] = sum over the workgroup's pairs of
// (d1 > 0) + (d2 > 0), the reference's sum(d1 > 0) + sum(d2 > 0); grid (B, 4)
__global__ __launch_bounds__(256) void k_cheirality4(EpiCand cand, long long N, const double* __restrict__ x1, const double* __restrict__ x2,
                                                     int32_t* __restrict__ cnt) {
  __shared__ int red[4];
  const int c = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const double P1[12] = {1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0};
  double P2[12];
  for (int a = 0; a < 12; ++a) P2[a] = c == 0 ? cand.P2[0][a] : (c == 1 ? cand.P2[1][a] : (c == 2 ? cand.P2[2][a] : cand.P2[3][a]));
  int k = 0;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < N; i += 256ll * gridDim.x) {
    double X[4];
    triangulate_pair(P1, P2, x1[i], x1[N + i], x2[i], x2[N + i], X);
    const double d1 = X[2], d2 = P2[8] * X[0] + P2[9] * X[1] + P2[10] * X[2] + P2[11] * X[3];
    k += (d1 > 0.0 ? 1 : 0) + (d2 > 0.0 ? 1 : 0);
  }
  k = fm_wave_sum_int(k);
  if (lane == 0) red[wave] = k;
  __syncthreads();
  if (threadIdx.x == 0) cnt[c * gridDim.x + blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}
#endif

}  // namespace mvus
