// The spline block as a general band: the damped scalar band pack every band solver starts from, and the one-workgroup Cholesky
// and substitution for bands wider than the partitioned solver (ba_band_part.hip.h) is built for.  The covariance chain
// (ba_cov.hip.h) factorises with these too.
#pragma once
#include <hip/hip_runtime.h>

#include "ba_assemble.hip.h"      // ne_diag_grad_entry
#include "ba_dev_problem.h"
#include "ba_ne_views.h"

namespace mvus {

// ---- the spline block as a GENERAL band (W > 6): Cholesky in place, then every right-hand side by substitution ----------------
// Lb[i][j] = M(i, i - j), j = 0..BW (the damped band of k_band_pack).  One workgroup: a sliding window of BW + 1 rows in LDS (row
// k + r in slot (k + r) mod (BW + 1)), column by column -- pivot, the column's BW entries, the rank-one update of the window's
// trailing triangle -- the finished row goes back to memory and the next one comes in.  A fallback for the rare wide band
// (the partitioned solver of ba_band_part.hip.h is built for W = 4 and 6): O(n BW^2) work on one CU.
__global__ __launch_bounds__(256) void k_band_chol_generic(int n, int BW, double* __restrict__ Lb, int* __restrict__ fail) {
  extern __shared__ double bwin[];                          // [(BW + 1)][(BW + 1)]
  __shared__ double dsh;
  const int R = BW + 1, tid = threadIdx.x;
  for (int e = tid; e < R * R; e += 256) { const int r = e / R, c = e % R; bwin[e] = r < n ? Lb[(long long)r * R + c] : 0.0; }
  __syncthreads();
  bool bad = false;
  for (int k = 0; k < n; ++k) {
    const int s0 = k % R;
    double* row0 = bwin + s0 * R;
    if (tid == 0) { const double p = row0[0]; bad = !(p > 0.0); dsh = sqrt(p > 0.0 ? p : 1.0); }
    __syncthreads();
    const double d = dsh;
    const int rows = min(BW, n - 1 - k);                    // rows k+1 .. k+rows hold column k
    if (tid == 0) row0[0] = d;
    for (int r = 1 + tid; r <= rows; r += 256) bwin[((k + r) % R) * R + r] /= d;     // M(k + r, k) sits at entry r of its row
    __syncthreads();
    for (int e = tid; e < rows * (rows + 1) / 2; e += 256) {                        // (r, s), 1 <= s <= r <= rows: M(k+r, k+s) -= l_r l_s
      int r = (int)((sqrt(8.0 * e + 1.0) - 1.0) * 0.5);
      while ((r + 1) * (r + 2) / 2 <= e) ++r;
      while (r * (r + 1) / 2 > e) --r;
      const int sidx = e - r * (r + 1) / 2 + 1, rr = r + 1;
      double* rowr = bwin + ((k + rr) % R) * R;
      rowr[rr - sidx] -= rowr[rr] * bwin[((k + sidx) % R) * R + sidx];
    }
    __syncthreads();
    // row k is final: back to memory; its slot takes row k + R
    for (int c = tid; c < R; c += 256) {
      Lb[(long long)k * R + c] = row0[c];
      const int nr = k + R;
      row0[c] = nr < n ? Lb[(long long)nr * R + c] : 0.0;
    }
    __syncthreads();
  }
  if (bad && tid == 0) fail[0] = 3;
}
// Z[i][c] <- (L L^T)^-1 Z[i][c]: one lane per right-hand side (64 per workgroup), the last BW solution entries in an LDS ring
__global__ __launch_bounds__(64) void k_band_solve_generic(int n, int BW, int ncols, const double* __restrict__ Lb, double* __restrict__ Z) {
  extern __shared__ double ring[];                          // [BW + 1][64]
  const int R = BW + 1, lane = threadIdx.x, c = blockIdx.x * 64 + lane;
  const bool on = c < ncols;
  for (int i = 0; i < n; ++i) {                             // forward: y_i = (b_i - sum_j L(i, i-j) y_{i-j}) / L(i, i)
    const double* Li = Lb + (long long)i * R;
    double sacc = on ? Z[(long long)i * ncols + c] : 0.0;
    const int jm = min(BW, i);
    for (int j = 1; j <= jm; ++j) sacc -= Li[j] * ring[((i - j) % R) * 64 + lane];
    const double y = sacc / Li[0];
    ring[(i % R) * 64 + lane] = y;
    if (on) Z[(long long)i * ncols + c] = y;
  }
  for (int i = n - 1; i >= 0; --i) {                        // backward: x_i = (y_i - sum_j L(i+j, i) x_{i+j}) / L(i, i)
    double sacc = on ? Z[(long long)i * ncols + c] : 0.0;
    const int jm = min(BW, n - 1 - i);
    for (int j = 1; j <= jm; ++j) sacc -= Lb[(long long)(i + j) * R + j] * ring[((i + j) % R) * 64 + lane];
    const double xv = sacc / Lb[(long long)i * R];
    ring[(i % R) * 64 + lane] = xv;
    if (on) Z[(long long)i * ncols + c] = xv;
  }
}

// scalar lower band of (C + lambda D_s): Lb[i][j] = (C + lambda D)(i, i-j), j = 0..BW
// with_diag: the launch also writes D = diag(H) and g in x order (k_ne_diag_grad's work, folded in: one launch less per
// linearisation; the first solve after an assembly carries it)
__device__ __forceinline__ void band_pack_entry(const NEView& ne, double lambda, int BW, double* __restrict__ Lb, int* __restrict__ fail, const DevProblem& dp,
                                                int with_diag, double* __restrict__ D, double* __restrict__ gx, long long idx) {
  if (idx == 0) { fail[0] = 0; fail[2] = 0; }   // first kernel of a solve: clears the failure flag the later ones may raise, and the sticky hand-over mark
  if (with_diag && idx < ne.CB + ne.N3) ne_diag_grad_entry(dp, ne, 0, (int)idx, D, gx);
  const long long total = (long long)ne.N3 * (BW + 1);
  if (idx >= total) return;
  const int i = (int)(idx / (BW + 1)), j = (int)(idx % (BW + 1));
  const int cidx = i - j;
  double v = 0.0;
  if (cidx >= 0) {
    const int gi = i / 3, ai = i % 3, gc_ = cidx / 3, ac = cidx % 3;
    const int w = gi - gc_;
    if (w < ne.W) v = ne.Cb[((long long)gc_ * ne.W + w) * 9 + 3 * ac + ai];
    if (j == 0) { const double h = v; v = h + lambda * (h > 0.0 ? h : 1.0); }
  }
  Lb[idx] = v;
}

}  // namespace mvus
