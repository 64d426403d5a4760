// Row routines of the covariance chain (ba_cov.hip.h), written once for the device and for the host build that pins them
// (tests/hostcheck/cov_hostcheck.cpp): the selected inverse of a banded Cholesky factor, the dense SPD inverse of the reduced camera
// system and the covariance of one spline sample.  Plain C++, no device intrinsics; the kernels only distribute these over threads.
#pragma once
#include "ba_math.h"

namespace mvus {

// A pivot p of either factorisation is refused when p <= kCovPivotTol * H_kk (H_kk: the unknown's own original diagonal entry): below
// that fewer than about six digits of a variance survive fp64 (eps / p >= 2e-6).  Anchored problems sit orders of magnitude above it,
// a free gauge at or below zero.
constexpr double kCovPivotTol = 1e-10;

// ---- selected inverse of a band (Takahashi) --------------------------------------------------------------------------------------
// Lb[i][j] = L(i, i - j), j = 0..BW, R = BW + 1 doubles per row: the factor k_band_chol_generic leaves.  Sigma = (L L^T)^-1 inside the
// band, from the last row up:
//   Sigma_ij = delta_ij / L_ii^2 - (1 / L_ii) sum_{k = i+1}^{i+BW} L_ki Sigma_kj,   j = i .. i + BW.
// win is the sliding window: Sigma(k, j) for i <= k, j <= i + BW at win[(k % R) * R + j % R], both triangles.  lcol[q] = L(i + q, i).
// Row i reads rows and columns i+1 .. i+BW of the window only and writes row and column i (the slots row i + R has left).
MVUS_HD double cov_selinv_entry(int i, int j, int n, int BW, const double* lcol, double lii, const double* win) {
  const int R = BW + 1;
  const int kmax = BW < n - 1 - i ? BW : n - 1 - i;
  double acc = 0.0;
  for (int q = 1; q <= kmax; ++q) acc += lcol[q] * win[((i + q) % R) * R + j % R];
  return (i == j ? 1.0 / (lii * lii) : 0.0) - acc / lii;
}
// pivot of row i recomputed from the finished factor: H_ii - sum_j L(i, i-j)^2 (what the factorisation took the square root of)
MVUS_HD double cov_band_pivot(int i, int BW, const double* Lb, double hii) {
  const double* Li = Lb + (long long)i * (BW + 1);
  const int jm = BW < i ? BW : i;
  double s = 0.0;
  for (int j = 1; j <= jm; ++j) s += Li[j] * Li[j];
  return hii - s;
}
// where entry (i, j), i <= j <= i + BW, goes in out[N][4][3][3] (blocks (p, p + w), w <= 3): -1 when it is outside those blocks
MVUS_HD long long cov_band_slot(int i, int j) {
  const int p = i / 3, a = i % 3, w = j / 3 - p, b = j % 3;
  return w <= 3 ? (((long long)p * 4 + w) * 3 + a) * 3 + b : -1;
}

// ---- dense SPD inverse ------------------------------------------------------------------------------------------------------------
// Right-looking blocked Cholesky of the lower triangle of S[m][ld], panels of kCovNB columns: the panel's diagonal block row by row
// (cov_chol_row with its own rows above it), the rows below it by the same routine against the finished diagonal block, then the
// trailing update S_ij -= sum_k L_ik L_jk.  Then L Y = I and L^T X = Y column by column.
constexpr int kCovNB = 32;
// One row against nb finished columns.  Lp: the diagonal block's rows (row j at Lp + j * ldp, its diagonal L_jj at [j]); row: this
// row's nb entries in the panel's columns, overwritten by L.  cols = how many of them lie left of the row's own diagonal (nb for a
// row below the block, its index inside the block for a row of the block).  Returns the pivot left on the diagonal for a row of the
// block (own = true: row[cols] holds S_ii), which the caller tests and replaces by its square root.
MVUS_HD double cov_chol_row(double* row, const double* Lp, int ldp, int cols, bool own) {
  for (int j = 0; j < cols; ++j) {
    const double* Lj = Lp + (long long)j * ldp;
    double v = row[j];
    for (int k = 0; k < j; ++k) v -= row[k] * Lj[k];
    row[j] = v / Lj[j];
  }
  if (!own) return 0.0;
  double p = row[cols];
  for (int k = 0; k < cols; ++k) p -= row[k] * row[k];
  return p;
}
// column c of Y = L^-1 (zero above row c), in place in Y[m][ldy]
MVUS_HD void cov_forward_col(int m, const double* L, int ld, double* Y, int ldy, int c) {
  for (int i = 0; i < c; ++i) Y[(long long)i * ldy + c] = 0.0;
  for (int i = c; i < m; ++i) {
    const double* Li = L + (long long)i * ld;
    double v = i == c ? 1.0 : 0.0;
    for (int k = c; k < i; ++k) v -= Li[k] * Y[(long long)k * ldy + c];
    Y[(long long)i * ldy + c] = v / Li[i];
  }
}
// column c of X = L^-T Y, in place
MVUS_HD void cov_backward_col(int m, const double* L, int ld, double* Y, int ldy, int c) {
  for (int i = m - 1; i >= 0; --i) {
    double v = Y[(long long)i * ldy + c];
    for (int k = i + 1; k < m; ++k) v -= L[(long long)k * ld + i] * Y[(long long)k * ldy + c];
    Y[(long long)i * ldy + c] = v / L[(long long)i * ld + i];
  }
}

// ---- covariance of one spline sample ----------------------------------------------------------------------------------------------
// Cov X(t) = sum_{a, b} h_a h_b Sigma(p + a, p + b) from the band blocks of control points p .. p + 3: bp = band + p * 36 points at
// block (p, p); block (p + a, p + b), b >= a, is bp[a * 36 + (b - a) * 9 ..], the other triangle its transpose.  out[9] row-major.
MVUS_HD void cov_spline_sample(const double* h, const double* bp, double* out) {
  for (int e = 0; e < 9; ++e) out[e] = 0.0;
  for (int a = 0; a < 4; ++a)
    for (int b = a; b < 4; ++b) {
      const double* blk = bp + a * 36 + (b - a) * 9;
      const double w = h[a] * h[b];
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
          out[3 * r + c] += w * blk[3 * r + c];
          if (b > a) out[3 * c + r] += w * blk[3 * r + c];
        }
    }
}

}  // namespace mvus
