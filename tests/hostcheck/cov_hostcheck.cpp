// TEST-ONLY host build of the covariance chain's row routines (mvus_amd/csrc/ba_cov_math.h): the loops the kernels of ba_cov.hip.h
// distribute over threads, run here in sequence so that tests/test_covariance_host.py can pin the arithmetic without a GPU.
#include <cmath>
#include <vector>

#include "../../mvus_amd/csrc/ba_cov_math.h"

using namespace mvus;

extern "C" {

// k_cov_selinv: the factor Lb[n][BW + 1] -> out[ceil(n / 3)][4][3][3] (cleared here)
void covcheck_selinv(int n, int BW, const double* Lb, double* out) {
  const int R = BW + 1;
  std::vector<double> win((size_t)R * R, 0.0), lcol((size_t)R, 0.0);
  for (long long e = 0; e < (long long)((n + 2) / 3) * 36; ++e) out[e] = 0.0;
  for (int i = n - 1; i >= 0; --i) {
    const int kmax = BW < n - 1 - i ? BW : n - 1 - i;
    for (int q = 0; q <= kmax; ++q) lcol[q] = Lb[(long long)(i + q) * R + q];
    const double lii = lcol[0];
    for (int q = 1; q <= kmax; ++q) {
      const int j = i + q;
      const double v = cov_selinv_entry(i, j, n, BW, lcol.data(), lii, win.data());
      win[(size_t)(i % R) * R + j % R] = v;
      win[(size_t)(j % R) * R + i % R] = v;
      const long long slot = cov_band_slot(i, j);
      if (slot >= 0) {
        out[slot] = v;
        if (j / 3 == i / 3) out[((long long)(i / 3) * 12 + j % 3) * 3 + i % 3] = v;
      }
    }
    const double v = cov_selinv_entry(i, i, n, BW, lcol.data(), lii, win.data());
    win[(size_t)(i % R) * R + i % R] = v;
    out[cov_band_slot(i, i)] = v;
  }
}

// k_cov_band_pivots: first refused row or -1
int covcheck_band_pivots(int n, int BW, const double* Lb, const double* hs) {
  for (int i = 0; i < n; ++i) if (!(cov_band_pivot(i, BW, Lb, hs[i]) > kCovPivotTol * hs[i])) return i;
  return -1;
}

// k_cov_potrf / k_cov_trsm / k_cov_syrk per panel, then k_cov_tri: S[m][m] (lower triangle read, overwritten by L), X[m][m] = S^-1
// (the lower triangle is what k_cov_expand takes).  hc[m]: the original diagonal the pivots are measured against.  Returns the first
// refused pivot or -1.
int covcheck_dense_inverse(int m, double* S, const double* hc, double* X) {
  int bad = -1;
  std::vector<double> blk((size_t)kCovNB * (kCovNB + 1)), row((size_t)kCovNB);
  for (int k0 = 0; k0 < m; k0 += kCovNB) {
    const int nb = kCovNB < m - k0 ? kCovNB : m - k0, ld = kCovNB + 1;
    for (int r = 0; r < nb; ++r) for (int c = 0; c < nb; ++c) blk[(size_t)r * ld + c] = c <= r ? S[(long long)(k0 + r) * m + k0 + c] : 0.0;
    for (int i = 0; i < nb; ++i) {
      double p = cov_chol_row(&blk[(size_t)i * ld], blk.data(), ld, i, true);
      if (!(p > kCovPivotTol * hc[k0 + i])) { if (bad < 0) bad = k0 + i; p = 1.0; }
      blk[(size_t)i * ld + i] = std::sqrt(p);
    }
    for (int r = 0; r < nb; ++r) for (int c = 0; c <= r; ++c) S[(long long)(k0 + r) * m + k0 + c] = blk[(size_t)r * ld + c];
    for (int i = k0 + nb; i < m; ++i) {
      for (int c = 0; c < nb; ++c) row[c] = S[(long long)i * m + k0 + c];
      cov_chol_row(row.data(), blk.data(), ld, nb, false);
      for (int c = 0; c < nb; ++c) S[(long long)i * m + k0 + c] = row[c];
    }
    for (int i = k0 + nb; i < m; ++i)
      for (int j = k0 + nb; j <= i; ++j) {
        double acc = 0.0;
        for (int k = 0; k < nb; ++k) acc += S[(long long)i * m + k0 + k] * S[(long long)j * m + k0 + k];
        S[(long long)i * m + j] -= acc;
      }
  }
  for (int c = 0; c < m; ++c) { cov_forward_col(m, S, m, X, m, c); cov_backward_col(m, S, m, X, m, c); }
  return bad;
}

// k_spline_cov_eval's formula for one sample: h[4], bp = &band[p][0][0][0] (four control points' blocks, 144 doubles), out[9]
void covcheck_sample(const double* h, const double* bp, double* out) { cov_spline_sample(h, bp, out); }

}  // extern "C"
