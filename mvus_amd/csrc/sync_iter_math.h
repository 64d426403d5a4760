// Lane routines of the iterative time-shift search (sync_iter.hip.h): the sampler, the evaluation of a 2-D interpolating spline with
// splev's extension, the real eigenvalues of the 9 x 9 pencil A1 + beta A2 of Albl et al. (reference synchronization.py:29-36), the
// normalised 8-point fit of nine pairs and the squared Sampson error.  MVUS_HD: the kernels and the test-only host build
// (tests/sync_iter_hostcheck.cpp) compile this same text.
//
// Work arrays are addressed as w[k * ld]: ld = 1 on the host; on the device the arrays of one workgroup lie in LDS as [element][lane]
// and ld is the workgroup size, so the lanes of a wave read neighbouring words (no bank conflict) and nothing 9 x 9 lives in scratch.
//
// The eigenvalue route.  Columns 2, 5 and 8 of A2 are zero.  Householder reflections that triangularise those three columns of A1
// (s1x, s1y, 1) leave det(A1 + beta A2) = det(R) det(B1 + beta B2) with a 6 x 6 pencil (B1, B2): an orthogonal transformation, so
// the pencil's eigenvalues keep their conditioning.  Start values come from the standard problem C = B1^-1 B2 (LU with partial
// pivoting), mu = -1 / beta, by elimination to Hessenberg form and the Francis double-shift QR iteration, which also decides real
// against complex (the sign of a 2 x 2 block's discriminant, as LAPACK does).  B1^-1 costs cond(B1) digits, so each real start value
// is then refined ON THE PENCIL by two-sided Rayleigh-quotient iteration, beta <- -(u^T B1 v) / (u^T B2 v) with v, u from inverse
// iteration on B1 + beta B2 and its transpose: the error of the quotient is second order in the vectors' and its rounding error is
// eps |u||v| (|B1| + |beta||B2|) / |u^T B2 v|, the first-order bound of a backward-stable solve.  The characteristic polynomial with
// the Aberth routine of epipolar.hip.h was the alternative; it was not taken because its coefficients (six determinants) are not
// a backward-stable representation of the pencil and its roots carry no real / complex decision.  The points are Hartley-normalised
// first: beta is invariant under an affine map of either image (ds only sees the linear part).
#pragma once
#include <cfloat>
#include <cmath>
#include <cstdint>

#include "ba_math.h"
#include "pnp.hip.h"           // pnp_mix
#include "epipolar.hip.h"      // fm_row, fm_denormalise, fm_finite

namespace mvus {

constexpr int kSiSample = 9;       // pairs per hypothesis
constexpr int kSiSlots = 6;        // real shifts per hypothesis, at most
constexpr int kSiModel = 11;       // doubles per model: F (9, row-major, pixels, x2^T F x1 = 0), shift = beta d, valid flag
constexpr int kSiPencilWork = 9 * 15 + 36 + 36;   // doubles of work per lane of si_pencil_betas
constexpr int kSiFitWork = 81 + 81;               // ... of si_fundamental9

// nine distinct indices below n (n >= 9) of hypothesis h of (round, sign): counter based, a function of its arguments alone
MVUS_HD void si_sample9(unsigned long long seed, int round, int sign, int h, long long n, long long* idx) {
  unsigned long long ctr = seed * 0x100000001b3ull + (unsigned long long)round * 0x9e3779b1ull + (unsigned long long)sign * 0x632be5abull +
                           (unsigned long long)h * 1000003ull + 0x2545f4914f6cdd1dull;
  for (int k = 0; k < kSiSample;) {
    ctr = pnp_mix(ctr);
    const long long c = (long long)(ctr % (unsigned long long)n);
    bool dup = false;
    for (int j = 0; j < k; ++j) dup |= idx[j] == c;
    if (!dup) idx[k++] = c;
  }
}

// (x, y)(u) of an interpolating cubic spline t[n + 4], c = x coefficients (n) then y coefficients (n), on span l (find_span's, or the
// same value found another way).  Outside [t[3], t[n]] the span is the first or last one and the recurrence evaluates that piece's
// polynomial there: splev's ext = 0.
//
// The recurrence is bspline_basis_w's (ba_math.h: FITPACK fpbspl for k = 3, term for term) and the sum is splev's, restated here under
// contraction off: one rounding per operation, so the point has splev's bits on the host and on the device (measured on the host build:
// bit-identical to scipy inside and beyond the knots).  The counts of the scoring kernel depend on it, and so does the comparison of a
// model with the oracle's: a fused multiply-add in the extended end polynomial moves a sample by more than the 8-point fit forgives.
MVUS_HD void si_spline_at(const double* t, const double* c, int n, int l, double u, double* out) {
#pragma clang fp contract(off)
  double h[4], hh[3];
  h[0] = 1.0;
  for (int j = 1; j <= 3; ++j) {
    for (int i = 0; i < j; ++i) hh[i] = h[i];
    h[0] = 0.0;
    for (int i = 0; i < j; ++i) {
      const double tli = t[l + i + 1], tlj = t[l + i + 1 - j];
      const double f = hh[i] / (tli - tlj);
      h[i] = h[i] + f * (tli - u);
      h[i + 1] = f * (u - tlj);
    }
  }
  const double* cx = c + (l - 3);
  const double* cy = c + n + (l - 3);
  out[0] = ((h[0] * cx[0] + h[1] * cx[1]) + h[2] * cx[2]) + h[3] * cx[3];
  out[1] = ((h[0] * cy[0] + h[1] * cy[1]) + h[2] * cy[2]) + h[3] * cy[3];
}
MVUS_HD void si_spline_eval2(const double* t, const double* c, int n, double u, double* out) {
  if (!fm_finite(u)) { out[0] = out[1] = NAN; return; }
  si_spline_at(t, c, n, find_span(t, n, u), u, out);
}

// a + b x in two roundings (numpy's s2 + beta * ds): the shifted sample the 8-point fit sees has the oracle's bits
MVUS_HD double si_mul_add(double a, double b, double x) {
#pragma clang fp contract(off)
  const double bx = b * x;
  return a + bx;
}

// find_span from a uniform first guess and a short walk (the samples of the scoring kernel are sorted in time and the knots of an
// interpolating spline are nearly uniform); falls back to the bisection.  Same value as find_span for ascending interior knots.
MVUS_HD int si_find_span_guess(const double* t, int n, double u) {
  const double a = t[3], b = t[n];
  int l = 3;
  if (b > a) {
    const double g = 3.0 + (u - a) / (b - a) * (double)(n - 3);
    l = !(g >= 3.0) ? 3 : (g > (double)(n - 1) ? n - 1 : (int)g);      // (a NaN guess is span 3)
  }
  for (int it = 0; it < 8; ++it) {
    if (u < t[l] && l > 3) --l;
    else if (u >= t[l + 1] && l < n - 1) ++l;
    else return l;
  }
  return find_span(t, n, u);
}

// start <= tau < end for one of the K intervals iv[2k], iv[2k + 1]
MVUS_HD bool si_in_intervals(const double* iv, int K, double tau) {
  bool in = false;
  for (int k = 0; k < K; ++k) in = in || (tau >= iv[2 * k] && tau < iv[2 * k + 1]);
  return in;
}

// squared Sampson error of epipolar.py:258-265 (pixels^2): x1 = (u1, v1, 1), x2 = (u2, v2, 1), x2^T F x1.  Contraction off: one
// rounding per operation, the same bits on host and device.
MVUS_HD double si_sampson(const double* F, double u1, double v1, double u2, double v2) {
#pragma clang fp contract(off)
  const double a = F[0] * u1 + F[1] * v1 + F[2];
  const double b = F[3] * u1 + F[4] * v1 + F[5];
  const double c = F[6] * u1 + F[7] * v1 + F[8];
  const double p = F[0] * u2 + F[3] * v2 + F[6];
  const double q = F[1] * u2 + F[4] * v2 + F[7];
  const double w = a * a + b * b + p * p + q * q;
  const double r = u2 * a + v2 * b + c;
  return r * r / w;
}

// Hartley normalisation of nine points: T = (cx, cy, s), s = sqrt(2) / mean distance to the centroid; false when they coincide
MVUS_HD bool si_hartley9(const double* x, const double* y, double* T) {
  double cx = 0.0, cy = 0.0, md = 0.0;
  for (int k = 0; k < 9; ++k) { cx += x[k]; cy += y[k]; }
  cx /= 9.0; cy /= 9.0;
  for (int k = 0; k < 9; ++k) md += sqrt((x[k] - cx) * (x[k] - cx) + (y[k] - cy) * (y[k] - cy));
  md /= 9.0;
  T[0] = cx; T[1] = cy; T[2] = sqrt(2.0) / md;
  return md > 0.0 && fm_finite(T[2]) && fm_finite(cx) && fm_finite(cy);
}

// LU of the 6 x 6 matrix a (row-major, a[(6 i + j) ld], overwritten) with partial pivoting; piv[k] = row swapped with k.  A pivot
// below tiny is replaced by tiny (inverse iteration wants a nearly singular matrix); returns the smallest |pivot| before that.
MVUS_HD double si_lu6(double* a, int ld, int* piv, double tiny) {
  double pmin = HUGE_VAL;
  for (int k = 0; k < 6; ++k) {
    int p = k;
    double best = fabs(a[(6 * k + k) * ld]);
    for (int i = k + 1; i < 6; ++i) { const double v = fabs(a[(6 * i + k) * ld]); if (v > best) { best = v; p = i; } }
    piv[k] = p;
    if (p != k) for (int j = 0; j < 6; ++j) { const double s = a[(6 * k + j) * ld]; a[(6 * k + j) * ld] = a[(6 * p + j) * ld]; a[(6 * p + j) * ld] = s; }
    pmin = fmin(pmin, best);
    if (!(best > tiny)) a[(6 * k + k) * ld] = a[(6 * k + k) * ld] < 0.0 ? -tiny : tiny;
    const double ip = 1.0 / a[(6 * k + k) * ld];
    for (int i = k + 1; i < 6; ++i) {
      const double f = a[(6 * i + k) * ld] * ip;
      a[(6 * i + k) * ld] = f;
      if (f != 0.0) for (int j = k + 1; j < 6; ++j) a[(6 * i + j) * ld] -= f * a[(6 * k + j) * ld];
    }
  }
  return pmin;
}
MVUS_HD void si_lu6_solve(const double* a, int ld, const int* piv, double* b) {
  for (int k = 0; k < 6; ++k) {                                       // (the rows of L were swapped whole: all swaps first)
    const int p = piv[k];
    if (p != k) { const double s = b[k]; b[k] = b[p]; b[p] = s; }
  }
  for (int k = 0; k < 6; ++k)
    for (int i = k + 1; i < 6; ++i) b[i] -= a[(6 * i + k) * ld] * b[k];
  for (int i = 5; i >= 0; --i) {
    double v = b[i];
    for (int j = i + 1; j < 6; ++j) v -= a[(6 * i + j) * ld] * b[j];
    b[i] = v / a[(6 * i + i) * ld];
  }
}

// real eigenvalues of the 6 x 6 matrix a (row-major, a[(6 i + j) ld], destroyed): elimination to Hessenberg form with pivoting, then
// the Francis double-shift QR iteration (EISPACK hqr).  wr[0..return): the real ones, in the order they deflate; -1: no convergence.
MVUS_HD int si_real_eig6(double* a, int ld, double* wr) {
  const int n = 6;
#define SI_A(i, j) a[(6 * (i) + (j)) * ld]
  for (int m = 1; m < n - 1; ++m) {
    double x = 0.0;
    int i = m;
    for (int j = m; j < n; ++j) if (fabs(SI_A(j, m - 1)) > fabs(x)) { x = SI_A(j, m - 1); i = j; }
    if (i != m) {
      for (int j = m - 1; j < n; ++j) { const double s = SI_A(i, j); SI_A(i, j) = SI_A(m, j); SI_A(m, j) = s; }
      for (int j = 0; j < n; ++j) { const double s = SI_A(j, i); SI_A(j, i) = SI_A(j, m); SI_A(j, m) = s; }
    }
    if (x != 0.0)
      for (i = m + 1; i < n; ++i) {
        double y = SI_A(i, m - 1);
        if (y != 0.0) {
          y /= x;
          for (int j = m; j < n; ++j) SI_A(i, j) -= y * SI_A(m, j);
          for (int j = 0; j < n; ++j) SI_A(j, m) += y * SI_A(j, i);
        }
      }
  }
  for (int i = 2; i < n; ++i) for (int j = 0; j < i - 1; ++j) SI_A(i, j) = 0.0;
  double anorm = 0.0;
  for (int i = 0; i < n; ++i) for (int j = (i > 0 ? i - 1 : 0); j < n; ++j) anorm += fabs(SI_A(i, j));
  if (!fm_finite(anorm)) return -1;
  int nr = 0, nn = n - 1;
  double t = 0.0, p = 0.0, q = 0.0, r = 0.0;
  while (nn >= 0) {
    int its = 0, l;
    do {
      for (l = nn; l >= 1; --l) {
        double s = fabs(SI_A(l - 1, l - 1)) + fabs(SI_A(l, l));
        if (s == 0.0) s = anorm;
        if (fabs(SI_A(l, l - 1)) + s == s) { SI_A(l, l - 1) = 0.0; break; }
      }
      double x = SI_A(nn, nn);
      if (l == nn) { wr[nr++] = x + t; --nn; }
      else {
        double y = SI_A(nn - 1, nn - 1), w = SI_A(nn, nn - 1) * SI_A(nn - 1, nn);
        if (l == nn - 1) {
          p = 0.5 * (y - x);
          q = p * p + w;
          double z = sqrt(fabs(q));
          x += t;
          if (q >= 0.0) {
            z = p + (p >= 0.0 ? z : -z);
            wr[nr++] = x + z;
            wr[nr++] = z != 0.0 ? x - w / z : x + z;
          }
          nn -= 2;
        } else {
          if (its == 60) return -1;
          if (its == 10 || its == 20) {
            t += x;
            for (int i = 0; i <= nn; ++i) SI_A(i, i) -= x;
            const double s = fabs(SI_A(nn, nn - 1)) + fabs(SI_A(nn - 1, nn - 2));
            y = x = 0.75 * s;
            w = -0.4375 * s * s;
          }
          ++its;
          int m;
          double z;
          for (m = nn - 2; m >= l; --m) {
            z = SI_A(m, m);
            r = x - z;
            double s = y - z;
            p = (r * s - w) / SI_A(m + 1, m) + SI_A(m, m + 1);
            q = SI_A(m + 1, m + 1) - z - r - s;
            r = SI_A(m + 2, m + 1);
            s = fabs(p) + fabs(q) + fabs(r);
            p /= s; q /= s; r /= s;
            if (m == l) break;
            const double u = fabs(SI_A(m, m - 1)) * (fabs(q) + fabs(r));
            const double v = fabs(p) * (fabs(SI_A(m - 1, m - 1)) + fabs(z) + fabs(SI_A(m + 1, m + 1)));
            if (u + v == v) break;
          }
          for (int i = m + 2; i <= nn; ++i) { SI_A(i, i - 2) = 0.0; if (i != m + 2) SI_A(i, i - 3) = 0.0; }
          for (int k = m; k <= nn - 1; ++k) {
            if (k != m) {
              p = SI_A(k, k - 1);
              q = SI_A(k + 1, k - 1);
              r = k != nn - 1 ? SI_A(k + 2, k - 1) : 0.0;
              x = fabs(p) + fabs(q) + fabs(r);
              if (x != 0.0) { p /= x; q /= x; r /= x; }
            }
            const double sq = sqrt(p * p + q * q + r * r), s = p >= 0.0 ? sq : -sq;
            if (s != 0.0) {
              if (k == m) { if (l != m) SI_A(k, k - 1) = -SI_A(k, k - 1); }
              else SI_A(k, k - 1) = -s * x;
              p += s; x = p / s; y = q / s; z = r / s; q /= p; r /= p;
              for (int j = k; j <= nn; ++j) {
                p = SI_A(k, j) + q * SI_A(k + 1, j);
                if (k != nn - 1) { p += r * SI_A(k + 2, j); SI_A(k + 2, j) -= p * z; }
                SI_A(k + 1, j) -= p * y;
                SI_A(k, j) -= p * x;
              }
              const int mmin = nn < k + 3 ? nn : k + 3;
              for (int i = l; i <= mmin; ++i) {
                p = x * SI_A(i, k) + y * SI_A(i, k + 1);
                if (k != nn - 1) { p += z * SI_A(i, k + 2); SI_A(i, k + 2) -= p * r; }
                SI_A(i, k + 1) -= p * q;
                SI_A(i, k) -= p;
              }
            }
          }
        }
      }
    } while (l < nn - 1);
  }
#undef SI_A
  return nr;
}

// The finite real beta with det(A1 + beta A2) = 0 for the nine samples s1, s2, ds (each x[9] then y[9]): ascending in betas[],
// their number returned (0..6).  0 also for a non-finite or degenerate sample (coinciding points, collinear s1, singular B1).
// w: kSiPencilWork doubles at stride ld.
MVUS_HD int si_pencil_betas(const double* s1, const double* s2, const double* ds, double* w, int ld, double* betas) {
  for (int k = 0; k < 9; ++k)
    if (!(fm_finite(s1[k]) && fm_finite(s1[9 + k]) && fm_finite(s2[k]) && fm_finite(s2[9 + k]) && fm_finite(ds[k]) && fm_finite(ds[9 + k]))) return 0;
  double T1[3], T2[3];
  if (!si_hartley9(s1, s1 + 9, T1) || !si_hartley9(s2, s2 + 9, T2)) return 0;
  double* Z = w;                        // 9 x 15: [s1x s1y 1 | the six other columns of A1 | the six non-zero columns of A2]
  double* C = w + 135 * ld;             // 6 x 6
  double* L = w + 171 * ld;             // 6 x 6
#define SI_Z(i, j) Z[(15 * (i) + (j)) * ld]
  for (int k = 0; k < 9; ++k) {
    const double ax = (s1[k] - T1[0]) * T1[2], ay = (s1[9 + k] - T1[1]) * T1[2];
    const double bx = (s2[k] - T2[0]) * T2[2], by = (s2[9 + k] - T2[1]) * T2[2];
    const double dx = ds[k] * T2[2], dy = ds[9 + k] * T2[2];
    SI_Z(k, 0) = ax; SI_Z(k, 1) = ay; SI_Z(k, 2) = 1.0;
    SI_Z(k, 3) = ax * bx; SI_Z(k, 4) = ax * by; SI_Z(k, 5) = ay * bx; SI_Z(k, 6) = ay * by; SI_Z(k, 7) = bx; SI_Z(k, 8) = by;
    SI_Z(k, 9) = ax * dx; SI_Z(k, 10) = ax * dy; SI_Z(k, 11) = ay * dx; SI_Z(k, 12) = ay * dy; SI_Z(k, 13) = dx; SI_Z(k, 14) = dy;
  }
  // Householder reflections on columns 0..2, applied to all fifteen
  for (int c = 0; c < 3; ++c) {
    double nn = 0.0;
    for (int i = c; i < 9; ++i) nn += SI_Z(i, c) * SI_Z(i, c);
    const double nrm = sqrt(nn);
    if (!(nrm > 1e-12)) return 0;                                     // (normalised coordinates: the columns are O(1)) collinear s1
    const double x0 = SI_Z(c, c), al = x0 >= 0.0 ? -nrm : nrm;
    SI_Z(c, c) = x0 - al;                                             // v, kept in place
    const double vv = nn - x0 * x0 + SI_Z(c, c) * SI_Z(c, c);
    if (!(vv > 0.0)) return 0;
    for (int j = c + 1; j < 15; ++j) {
      double s = 0.0;
      for (int i = c; i < 9; ++i) s += SI_Z(i, c) * SI_Z(i, j);
      s *= 2.0 / vv;
      for (int i = c; i < 9; ++i) SI_Z(i, j) -= s * SI_Z(i, c);
    }
  }
  // B1 = Z[3.., 3..8], B2 = Z[3.., 9..14]; C = B1^-1 B2
  double n1 = 0.0, n2 = 0.0;
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j < 6; ++j) {
      L[(6 * i + j) * ld] = SI_Z(3 + i, 3 + j);
      n1 += SI_Z(3 + i, 3 + j) * SI_Z(3 + i, 3 + j);
      n2 += SI_Z(3 + i, 9 + j) * SI_Z(3 + i, 9 + j);
    }
  n1 = sqrt(n1); n2 = sqrt(n2);
  if (!(n1 > 0.0) || !(n2 > 0.0)) return 0;
  int piv[6];
  if (!(si_lu6(L, ld, piv, 0.0) > 1e-13 * n1)) return 0;
  for (int j = 0; j < 6; ++j) {
    double b[6];
    for (int i = 0; i < 6; ++i) b[i] = SI_Z(3 + i, 9 + j);
    si_lu6_solve(L, ld, piv, b);
    for (int i = 0; i < 6; ++i) C[(6 * i + j) * ld] = b[i];
  }
  double mu[6];
  const int nr = si_real_eig6(C, ld, mu);
  int n = 0;
  for (int k = 0; k < nr; ++k) {
    if (mu[k] == 0.0) continue;
    double beta = -1.0 / mu[k];
    if (!fm_finite(beta)) continue;
    // two-sided Rayleigh-quotient iteration on (B1, B2)
    double v[6], u[6];
    for (int i = 0; i < 6; ++i) { v[i] = 1.0; u[i] = 1.0; }
    for (int it = 0; it < 4; ++it) {
      const double tiny = DBL_EPSILON * (n1 + fabs(beta) * n2);
      for (int tr = 0; tr < 2; ++tr) {
        for (int i = 0; i < 6; ++i)
          for (int j = 0; j < 6; ++j) L[(6 * i + j) * ld] = tr ? SI_Z(3 + j, 3 + i) + beta * SI_Z(3 + j, 9 + i) : SI_Z(3 + i, 3 + j) + beta * SI_Z(3 + i, 9 + j);
        si_lu6(L, ld, piv, tiny);
        double* x = tr ? u : v;
        si_lu6_solve(L, ld, piv, x);
        double nx = 0.0;
        for (int i = 0; i < 6; ++i) nx = fmax(nx, fabs(x[i]));
        if (!(nx > 0.0) || !fm_finite(nx)) { for (int i = 0; i < 6; ++i) x[i] = 1.0; }
        else for (int i = 0; i < 6; ++i) x[i] /= nx;
      }
      double num = 0.0, den = 0.0;
      for (int i = 0; i < 6; ++i) {
        double a1 = 0.0, a2 = 0.0;
        for (int j = 0; j < 6; ++j) { a1 += SI_Z(3 + i, 3 + j) * v[j]; a2 += SI_Z(3 + i, 9 + j) * v[j]; }
        num += u[i] * a1; den += u[i] * a2;
      }
      if (den == 0.0) break;
      const double bn = -num / den;
      if (!fm_finite(bn)) break;
      const bool done = fabs(bn - beta) <= 4.0 * DBL_EPSILON * fabs(bn);
      beta = bn;
      if (done) break;
    }
    betas[n++] = beta;
  }
#undef SI_Z
  for (int i = 1; i < n; ++i) {                                       // ascending
    const double b = betas[i];
    int j = i - 1;
    while (j >= 0 && betas[j] > b) { betas[j + 1] = betas[j]; --j; }
    betas[j + 1] = b;
  }
  return n;
}

// one-sided Jacobi (Hestenes) on the columns of the n x n matrix a (a[(n i + j) ld], overwritten by U Sigma), the rotations accumulated
// in v (v[(n i + j) ld]): the column of smallest norm of a is returned, v's column of that index is the singular vector.  It works
// on the matrix itself, not on its Gram matrix, so a small singular value keeps its relative accuracy.
MVUS_HD int si_jacobi_svd(int n, double* a, double* v, int ld) {
  for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) v[(n * i + j) * ld] = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 40; ++sweep) {
    bool rotated = false;
    for (int p = 0; p < n - 1; ++p)
      for (int q = p + 1; q < n; ++q) {
        double al = 0.0, be = 0.0, ga = 0.0;
        for (int i = 0; i < n; ++i) { const double gp = a[(n * i + p) * ld], gq = a[(n * i + q) * ld]; al += gp * gp; be += gq * gq; ga += gp * gq; }
        if (fabs(ga) <= 1e-16 * sqrt(al * be) || ga == 0.0) continue;
        rotated = true;
        const double zeta = (be - al) / (2.0 * ga);
        const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
        const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
        for (int i = 0; i < n; ++i) {
          const double gp = a[(n * i + p) * ld], gq = a[(n * i + q) * ld];
          a[(n * i + p) * ld] = c * gp - s * gq; a[(n * i + q) * ld] = s * gp + c * gq;
          const double vp = v[(n * i + p) * ld], vq = v[(n * i + q) * ld];
          v[(n * i + p) * ld] = c * vp - s * vq; v[(n * i + q) * ld] = s * vp + c * vq;
        }
      }
    if (!rotated) break;
  }
  int jm = 0;
  double nm = 0.0;
  for (int j = 0; j < n; ++j) {
    double nj = 0.0;
    for (int i = 0; i < n; ++i) nj += a[(n * i + j) * ld] * a[(n * i + j) * ld];
    if (j == 0 || nj < nm) { nm = nj; jm = j; }
  }
  return jm;
}

// The normalised 8-point fit of nine pairs x1 -> x2 (each x[9] then y[9]; x2^T F x1 = 0): Hartley normalisation of both sets, the right
// singular vector of the smallest singular value of the 9 x 9 system, rank 2 (the smallest singular direction of the 3 x 3 removed),
// denormalised to pixels, unit Frobenius norm, F[8] >= 0.  False (and no F) for coinciding or non-finite points.  w: kSiFitWork at ld.
MVUS_HD bool si_fundamental9(const double* x1, const double* x2, double* w, int ld, double* F) {
  double T[6];
  if (!si_hartley9(x1, x1 + 9, T) || !si_hartley9(x2, x2 + 9, T + 3)) return false;
  double* A = w;
  double* V = w + 81 * ld;
  for (int k = 0; k < 9; ++k) {
    double r[9];
    fm_row((x1[k] - T[0]) * T[2], (x1[9 + k] - T[1]) * T[2], (x2[k] - T[3]) * T[5], (x2[9 + k] - T[4]) * T[5], r);
    for (int j = 0; j < 9; ++j) A[(9 * k + j) * ld] = r[j];
  }
  int jm = si_jacobi_svd(9, A, V, ld);
  double Fn[9];
  for (int i = 0; i < 9; ++i) Fn[i] = V[(9 * i + jm) * ld];
  for (int i = 0; i < 9; ++i) A[i * ld] = Fn[i];                     // 3 x 3, the same work arrays
  jm = si_jacobi_svd(3, A, V, ld);
  double v3[3], Fv[3];
  for (int i = 0; i < 3; ++i) v3[i] = V[(3 * i + jm) * ld];
  for (int i = 0; i < 3; ++i) Fv[i] = Fn[3 * i] * v3[0] + Fn[3 * i + 1] * v3[1] + Fn[3 * i + 2] * v3[2];
  for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) Fn[3 * i + j] -= Fv[i] * v3[j];
  fm_denormalise(Fn, T, F);
  bool ok = true;
  double nn = 0.0;
  for (int i = 0; i < 9; ++i) { ok = ok && fm_finite(F[i]); nn += F[i] * F[i]; }
  return ok && nn > 0.0;
}

}  // namespace mvus
