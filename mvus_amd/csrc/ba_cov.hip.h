// Covariance of the camera-side unknowns and of the trajectory's control points at a point x (mvus_ba_covariance): a chain of its
// own behind a linearisation.  It shares no launch with the LM step; from the solve chain it reuses the two general band kernels
// (k_band_chol_generic, k_band_solve_generic) as they are and nothing else.
//
// Definition.  H is the matrix mvus_ba_normal_equations exports at x with the loss and the frozen mask in force: J^T J (linear loss),
// scipy's J^T diag(s^2) J otherwise, motion rows included as the prior they are, frozen rows / columns zero with a unit diagonal.  An
// unknown is ESTIMATED when it is not frozen and its diagonal entry of H is non-zero (not: rs without rolling shutter, a control-point
// coordinate no row touches).  Sigma = sigma^2 (H restricted to the estimated unknowns)^-1, rows and columns of the others exactly 0.
// sigma^2: the caller's when > 0, else the a-posteriori factor 2 cost / (m_act - n_est) -- cost the (robust) cost at x, m_act the
// rows of f with a non-empty Jacobian row (every motion row, both rows of every detection with a span), n_est the estimated unknowns.
// Under a robust loss this is the usual Gauss-Newton approximation of the covariance (the curvature of rho enters through s only).
//
// Chain, in the solver's elimination order (spline block C first; H = [A E; E^T C], raw blocks, no damping, no partitions):
//   1 linearise             the path of mvus_ba_normal_equations, freeze pass included (HipSchur::assemble_held)
//   2 k_cov_pack            the undamped band in k_band_chol_generic's layout (unit diagonal for unestimated rows), Z = E^T row-major
//   3 band factor + solve   k_band_chol_generic, k_band_solve_generic (ncols = CB): Z = C^-1 E^T;  k_cov_band_pivots: the refusal test
//   4 k_cov_schur           S = A - E Z on the estimated camera unknowns (compact, lower triangle)
//   5 k_cov_potrf / _trsm / _syrk per panel of kCovNB columns (host loop), k_cov_tri (L Y = I, L^T X = Y), k_cov_expand:
//                           Sigma_cc = S^-1 put back at full size with zero rows / columns
//   6 k_cov_tz              T = Z Sigma_cc on the fp64 matrix cores, fused with the band of the low-rank term
//                           R(p, p + w) = T_p Z_{p+w}^T, w <= 3: a tile of kCovTP control points plus a halo of nine rows of Z; T itself
//                           is never stored by mvus_ba_covariance (k_cov_tz<true> keeps it, for the detection pass only)
//   7 k_cov_selinv          selected inverse of the band (Takahashi recurrence on the factor of stage 3), blocks w <= 3
//   8 k_cov_band_out, k_cov_cam_out: sigma^2 (selected inverse + R) in control-point order; sigma^2 Sigma_cc in the order of the head of x
// Stages 3, 5 (the panel's diagonal block) and 7 are sequential single-workgroup forms: the covariance is a one-off per BA.
// Behind stage 8, on request (mvus_ba_detection_covariance): k_detcov, the per-detection pass of ba_detcov.hip.h, with an event pair of its own.
// Refusal: a pivot p_k <= kCovPivotTol * H_kk of either factorisation (ba_cov_math.h) -> MVUS_E_NUMERIC naming the unknown.
#pragma once
#include <climits>
#include <cstring>

#include "api_common.h"      // MVUS_HIP
#include "ba_band_generic.hip.h"
#include "ba_cov_math.h"
#include "ba_detcov.hip.h"
#include "ba_dev_problem.h"
#include "ba_ne_views.h"
#include "ba_wave.hip.h"

namespace mvus {

// diag(H) in the solvers' internal order: [c * B + k] camera-side, then [3 g + d] control-point coordinates
__global__ void k_cov_diag(NEView ne, double* __restrict__ diag) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx < ne.CB) {
    const int c = idx / ne.B, k = idx % ne.B;
    diag[idx] = ne.A[((long long)c * ne.B + k) * ne.B + k];
  } else if (idx < ne.CB + ne.N3) {
    const int r = idx - ne.CB;
    diag[idx] = ne.Cb[((long long)(r / 3) * ne.W) * 9 + 4 * (r % 3)];
  }
}

// Lb[i][j] = C(i, i - j) undamped (1 on the diagonal of an unestimated row: its row and column of C are zero, the factor exists and
// the row stays out of everything else), hs[i] = that diagonal; Z[r][e] = E(e, r) from the camera-major cross block
__global__ void k_cov_pack(NEView ne, int BW, const uint8_t* __restrict__ est, double* __restrict__ Lb, double* __restrict__ hs, double* __restrict__ Z) {
  const long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  const int R = BW + 1;
  if (idx < (long long)ne.N3 * R) {
    const int i = (int)(idx / R), j = (int)(idx % R), cidx = i - j;
    double v = 0.0;
    if (cidx >= 0) {
      const int gi = i / 3, ai = i % 3, gc_ = cidx / 3, ac = cidx % 3, w = gi - gc_;
      if (w < ne.W) v = ne.Cb[((long long)gc_ * ne.W + w) * 9 + 3 * ac + ai];
      if (j == 0) { if (!est[ne.CB + i]) v = 1.0; hs[i] = v; }
    }
    Lb[idx] = v;
  }
  if (idx < (long long)ne.N3 * ne.CB) {
    const int r = (int)(idx / ne.CB), e = (int)(idx % ne.CB), c = e / ne.B, k = e % ne.B;
    Z[idx] = ne.Et[((long long)c * ne.N3 + r) * ne.B + k];
  }
}

// flags[0] = the first row of the band whose pivot is refused (INT_MAX: none)
__global__ void k_cov_band_pivots(int n, int BW, const double* __restrict__ Lb, const double* __restrict__ hs, int* __restrict__ flags) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double p = cov_band_pivot(i, BW, Lb, hs[i]);
  if (!(p > kCovPivotTol * hs[i])) atomicMin(&flags[0], i);
}

// S[i][j] = A(e_i, e_j) - sum_r E(e_i, r) Z(r, e_j), e = map[.] the estimated camera unknowns; tiles on and below the diagonal
__global__ __launch_bounds__(256) void k_cov_schur(NEView ne, int m, const int32_t* __restrict__ map, const double* __restrict__ Z, double* __restrict__ S) {
  if (blockIdx.x > blockIdx.y) return;
  __shared__ double Es[16][17], Zs[16][17];
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int i = blockIdx.y * 16 + ty, j = blockIdx.x * 16 + tx;
  const int ei = i < m ? map[i] : -1, ej = j < m ? map[j] : -1;
  const double* __restrict__ Erow = ei >= 0 ? ne.Et + (long long)(ei / ne.B) * ne.N3 * ne.B + ei % ne.B : nullptr;
  double acc = 0.0;
  for (int r0 = 0; r0 < ne.N3; r0 += 16) {
    Es[ty][tx] = (Erow && r0 + tx < ne.N3) ? Erow[(long long)(r0 + tx) * ne.B] : 0.0;
    Zs[ty][tx] = (ej >= 0 && r0 + ty < ne.N3) ? Z[(long long)(r0 + ty) * ne.CB + ej] : 0.0;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 16; ++k) acc += Es[ty][k] * Zs[k][tx];
    __syncthreads();
  }
  if (ei < 0 || ej < 0) return;
  const double a = ei / ne.B == ej / ne.B ? ne.A[((long long)(ei / ne.B) * ne.B + ei % ne.B) * ne.B + ej % ne.B] : 0.0;
  S[(long long)i * m + j] = a - acc;
}

// ---- dense Cholesky of S (lower triangle), one panel of nb <= kCovNB columns at k0 per round of three launches ---------------------
// the panel's diagonal block: rows in sequence by one thread (cov_chol_row); flags[1] = the first refused pivot (compact index)
__global__ __launch_bounds__(64) void k_cov_potrf(int m, int k0, int nb, double* __restrict__ S, const double* __restrict__ hc, int* __restrict__ flags) {
  __shared__ double blk[kCovNB][kCovNB + 1];
  for (int e = threadIdx.x; e < nb * nb; e += 64) { const int r = e / nb, c = e % nb; blk[r][c] = c <= r ? S[(long long)(k0 + r) * m + k0 + c] : 0.0; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 0; i < nb; ++i) {
      double p = cov_chol_row(&blk[i][0], &blk[0][0], kCovNB + 1, i, true);
      if (!(p > kCovPivotTol * hc[k0 + i])) { atomicMin(&flags[1], k0 + i); p = 1.0; }
      blk[i][i] = sqrt(p);
    }
  }
  __syncthreads();
  for (int e = threadIdx.x; e < nb * nb; e += 64) { const int r = e / nb, c = e % nb; if (c <= r) S[(long long)(k0 + r) * m + k0 + c] = blk[r][c]; }
}
// the rows below it: one thread per row against the finished diagonal block
__global__ __launch_bounds__(64) void k_cov_trsm(int m, int k0, int nb, double* __restrict__ S) {
  __shared__ double blk[kCovNB][kCovNB + 1], rows[64][kCovNB + 1];
  for (int e = threadIdx.x; e < nb * nb; e += 64) { const int r = e / nb, c = e % nb; blk[r][c] = c <= r ? S[(long long)(k0 + r) * m + k0 + c] : 0.0; }
  __syncthreads();
  const int i = k0 + nb + blockIdx.x * 64 + threadIdx.x;
  if (i >= m) return;
  double* row = &rows[threadIdx.x][0];
  double* __restrict__ Si = S + (long long)i * m + k0;
  for (int c = 0; c < nb; ++c) row[c] = Si[c];
  cov_chol_row(row, &blk[0][0], kCovNB + 1, nb, false);
  for (int c = 0; c < nb; ++c) Si[c] = row[c];
}
// trailing update S_ij -= sum_k L_ik L_jk, i >= j >= k0 + nb: 16 x 16 tiles on and below the diagonal
__global__ __launch_bounds__(256) void k_cov_syrk(int m, int k0, int nb, double* __restrict__ S) {
  if (blockIdx.x > blockIdx.y) return;
  __shared__ double Li[16][kCovNB + 1], Lj[16][kCovNB + 1];
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4, t0 = k0 + nb;
  const int ib = t0 + blockIdx.y * 16, jb = t0 + blockIdx.x * 16;
  for (int e = threadIdx.x; e < 16 * kCovNB; e += 256) {
    const int r = e / kCovNB, c = e % kCovNB;
    Li[r][c] = (ib + r < m && c < nb) ? S[(long long)(ib + r) * m + k0 + c] : 0.0;
    Lj[r][c] = (jb + r < m && c < nb) ? S[(long long)(jb + r) * m + k0 + c] : 0.0;
  }
  __syncthreads();
  const int i = ib + ty, j = jb + tx;
  if (i >= m || j > i) return;
  double acc = 0.0;
#pragma unroll
  for (int k = 0; k < kCovNB; ++k) acc += Li[ty][k] * Lj[tx][k];
  S[(long long)i * m + j] -= acc;
}
// X = L^-T L^-1: one lane per column through both substitutions of the identity
__global__ __launch_bounds__(64) void k_cov_tri(int m, const double* __restrict__ L, double* __restrict__ X) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= m) return;
  cov_forward_col(m, L, m, X, m, c);
  cov_backward_col(m, L, m, X, m, c);
}
// Sigma_cc at full size: rows and columns of unestimated unknowns zero (inv[e] = compact index or -1); both triangles from the lower one of X
__global__ void k_cov_expand(int CB, int m, const int32_t* __restrict__ inv, const double* __restrict__ X, double* __restrict__ Sig) {
  const long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (idx >= (long long)CB * CB) return;
  const int i1 = inv[idx / CB], i2 = inv[idx % CB];
  Sig[idx] = (i1 >= 0 && i2 >= 0) ? X[(long long)max(i1, i2) * m + min(i1, i2)] : 0.0;
}

// ---- stage 6: T = Z Sigma_cc on the matrix cores, fused with R(p, p + w) = T_p Z_{p+w}^T -------------------------------------------
// One workgroup per tile of kCovTP control points (48 rows of Z), four wavefronts; a wavefront takes every fourth chunk of 16 columns of
// T: three accumulator tiles of v_mfma_f64_16x16x4 over K = CB (lane l: A = Z[row0 + (l & 15)][k0 + (l >> 4)], B = Sigma[k0 + (l >> 4)]
// [col0 + (l & 15)], accumulator entry r = T[(l >> 4) + 4 r][l & 15]; fragments straight from memory, everything outside the matrices
// read as zero), the 48 x 16 piece of T and the 57 x 16 piece of Z (tile + halo) through the wavefront's own LDS, and each lane adds
// that chunk's share to its nine of the tile's 16 x 4 x 9 entries of R.  The wavefronts' sums are added in a fixed order at the end.
// STORE_T (launched with one more argument, Tm[N3][CB]): the wavefront also copies its 48 x 16 piece of T from LDS to Tm.  The
// instantiation without it takes no such argument and is the kernel it was.
constexpr int kCovTP = 16, kCovTR = 3 * kCovTP, kCovHalo = 9, kCovLd = 17;
constexpr int kCovWaveLds = (2 * kCovTR + kCovHalo) * kCovLd;        // doubles per wavefront: T piece [48][17] + Z piece [57][17]
constexpr int kCovTileOut = kCovTP * 36;
static_assert(kCovTileOut == 9 * 64 && kCovTileOut <= kCovWaveLds, "nine entries of R per lane; the reduction reuses the staging space");
inline __device__ double* cov_tm_arg() { return nullptr; }
inline __device__ double* cov_tm_arg(double* tm) { return tm; }
template <bool STORE_T = false, class... TM>
__global__ __launch_bounds__(256) void k_cov_tz(int N, int CB, const double* __restrict__ Z, const double* __restrict__ Sig, double* __restrict__ Rb, TM... tm_v) {
  static_assert(sizeof...(TM) == (STORE_T ? 1 : 0), "the storing instantiation is launched with Tm, the other one without");
  __shared__ double lds[4 * kCovWaveLds];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, lr = lane & 15, lk = lane >> 4;
  const int N3 = 3 * N, p0 = blockIdx.x * kCovTP, r0 = 3 * p0;
  double* Tt = lds + wave * kCovWaveLds;
  double* Zt = Tt + kCovTR * kCovLd;
  double racc[9];
#pragma unroll
  for (int q = 0; q < 9; ++q) racc[q] = 0.0;
  const int nchunk = (CB + 15) / 16, rounds = (nchunk + 3) / 4;
  for (int it = 0; it < rounds; ++it) {                     // (every wavefront makes every round: a chunk past the end reads zeros)
    const int j0 = (it * 4 + wave) * 16;
    d4 acc[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) acc[i] = d4{0.0, 0.0, 0.0, 0.0};
    const bool jok = j0 + lr < CB;
    for (int k0 = 0; k0 < CB; k0 += 4) {
      const int k = k0 + lk;
      const bool kok = k < CB;
      const double b = (kok && jok) ? Sig[(long long)k * CB + j0 + lr] : 0.0;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const int row = r0 + 16 * i + lr;
        const double a = (kok && row < N3) ? Z[(long long)row * CB + k] : 0.0;
        acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[i], 0, 0, 0);
      }
    }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) Tt[(16 * i + lk + 4 * r) * kCovLd + lr] = acc[i][r];
    for (int e = lane; e < (kCovTR + kCovHalo) * 16; e += 64) {
      const int rr = e >> 4, cc = e & 15, row = r0 + rr, col = j0 + cc;
      Zt[rr * kCovLd + cc] = (row < N3 && col < CB) ? Z[(long long)row * CB + col] : 0.0;
    }
    __syncthreads();
    if constexpr (STORE_T) {
      double* __restrict__ Tm = cov_tm_arg(tm_v...);
      for (int e = lane; e < kCovTR * 16; e += 64) {
        const int rr = e >> 4, cc = e & 15, row = r0 + rr, col = j0 + cc;
        if (row < N3 && col < CB) Tm[(long long)row * CB + col] = Tt[rr * kCovLd + cc];
      }
    }
#pragma unroll
    for (int q = 0; q < 9; ++q) {
      const int idx = lane + 64 * q, pl = idx / 36, w = (idx % 36) / 9, a = (idx % 9) / 3, b = idx % 3;
      const double* tr = Tt + (3 * pl + a) * kCovLd;
      const double* zr = Zt + (3 * (pl + w) + b) * kCovLd;
      double s = 0.0;
#pragma unroll
      for (int j = 0; j < 16; ++j) s += tr[j] * zr[j];
      racc[q] += s;
    }
    __syncthreads();
  }
#pragma unroll
  for (int q = 0; q < 9; ++q) lds[wave * kCovWaveLds + lane + 64 * q] = racc[q];
  __syncthreads();
  for (int idx = threadIdx.x; idx < kCovTileOut; idx += 256) {
    const int p = p0 + idx / 36;
    if (p >= N) continue;
    const double s = ((lds[idx] + lds[kCovWaveLds + idx]) + lds[2 * kCovWaveLds + idx]) + lds[3 * kCovWaveLds + idx];
    Rb[(long long)p * 36 + idx % 36] = s;
  }
}

// ---- stage 7: selected inverse of the band, one workgroup ----------------------------------------------------------------------------
// The sliding (BW + 1)^2 window of Sigma in LDS in the manner of k_band_chol_generic (cov_selinv_entry): per row the column of L, the
// row's off-diagonal entries side by side, then its diagonal.  Only the blocks w <= 3 go to sel[N][4][3][3] (cleared by the caller).
__global__ __launch_bounds__(256) void k_cov_selinv(int n, int BW, const double* __restrict__ Lb, double* __restrict__ sel) {
  extern __shared__ double cwin[];                          // [(BW + 1)][(BW + 1)] + [(BW + 1)]
  const int R = BW + 1, tid = threadIdx.x;
  double* lcol = cwin + R * R;
  for (int e = tid; e < R * R; e += 256) cwin[e] = 0.0;
  for (int i = n - 1; i >= 0; --i) {
    const int kmax = min(BW, n - 1 - i);
    __syncthreads();
    for (int q = tid; q <= kmax; q += 256) lcol[q] = Lb[(long long)(i + q) * R + q];
    __syncthreads();
    const double lii = lcol[0];
    for (int q = 1 + tid; q <= kmax; q += 256) {
      const int j = i + q;
      const double v = cov_selinv_entry(i, j, n, BW, lcol, lii, cwin);
      cwin[(i % R) * R + j % R] = v;
      cwin[(j % R) * R + i % R] = v;
      const long long slot = cov_band_slot(i, j);
      if (slot >= 0) {
        sel[slot] = v;
        if (j / 3 == i / 3) sel[((long long)(i / 3) * 12 + j % 3) * 3 + i % 3] = v;
      }
    }
    __syncthreads();
    if (tid == 0) {
      const double v = cov_selinv_entry(i, i, n, BW, lcol, lii, cwin);
      cwin[(i % R) * R + i % R] = v;
      sel[cov_band_slot(i, i)] = v;
    }
  }
}

// cov_band[p][w][a][b] = sigma^2 (selected inverse + R); zero where p + w >= N and in rows / columns of unestimated coordinates
__global__ void k_cov_band_out(int N, int CB, const uint8_t* __restrict__ est, double sigma2, const double* __restrict__ sel, const double* __restrict__ Rb, double* __restrict__ out) {
  const long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (idx >= (long long)N * 36) return;
  const int p = (int)(idx / 36), w = (int)(idx % 36) / 9, a = (int)(idx % 9) / 3, b = (int)(idx % 3);
  const bool on = p + w < N && est[CB + 3 * p + a] && est[CB + 3 * (p + w) + b];
  out[idx] = on ? sigma2 * (sel[idx] + Rb[idx]) : 0.0;
}
// cov_cam in the order of the head of x (alpha(C), beta(C), rs(C), then P per camera)
__global__ void k_cov_cam_out(int C, int P, double sigma2, const double* __restrict__ Sig, double* __restrict__ out) {
  const int B = 3 + P, CB = C * B;
  const long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (idx >= (long long)CB * CB) return;
  const int e1 = (int)(idx / CB), e2 = (int)(idx % CB);
  out[(long long)cam_col(C, P, e1 / B, e1 % B) * CB + cam_col(C, P, e2 / B, e2 % B)] = sigma2 * Sig[idx];
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------
constexpr int kCovStages = 8;
inline const char* cov_stage_name(int s) {
  static const char* const names[kCovStages] = {"linearise", "pack", "band factor + solve", "schur complement", "camera inverse", "T = Z Sigma + band of R",
                                                "selected inverse", "outputs"};
  return s >= 0 && s < kCovStages ? names[s] : "";
}

struct CovResult { double sigma2 = 0.0; int64_t dof = 0; };

// the chain's own buffers: allocated on first use (the handle's problem never changes size upwards), freed with the handle
template <class BE>
struct CovChain {
  BE& be;
  DeviceOwner own;                 // the buffers and the stage events: regrown together (ensure)
  hipEvent_t ev[kCovStages + 1] = {};
  double stage_ms[kCovStages] = {};
  bool timed = false;
  int N3 = 0, CB = 0, BW = 0;
  // the detection pass (mvus_ba_detection_covariance): its buffers exist from the first such call on, with the event pair of the pass
  DeviceOwner det_own;
  const char* who = "covariance";   // the entry point the messages name
  hipEvent_t det_ev[2] = {};
  double det_ms = 0.0;
  bool det_timed = false;
  long long det_M = -1;
  double *Tm = nullptr, *Gb = nullptr, *det_e = nullptr, *det_pcov = nullptr, *det_t2 = nullptr;
  double *diag = nullptr, *Lb = nullptr, *hs = nullptr, *Z = nullptr, *S = nullptr, *X = nullptr, *Sig = nullptr, *hc = nullptr, *Rb = nullptr, *sel = nullptr,
         *band_out = nullptr, *cam_out = nullptr;
  uint8_t* est = nullptr;
  int32_t *map = nullptr, *inv = nullptr;
  int* flags = nullptr;
  explicit CovChain(BE& b) : be(b) {}
  template <class T> T* device(size_t count) { return own.device<T>(count); }
  void ensure(const NEView& ne, int bw) {
    if (Lb && N3 == ne.N3 && CB == ne.CB && BW == bw) return;
    own.reset(); Lb = nullptr;
    det_own.reset(); Tm = nullptr; det_M = -1;
    N3 = ne.N3; CB = ne.CB; BW = bw;
    const size_t n3 = (size_t)N3, cb = (size_t)CB;
    diag = device<double>(cb + n3); est = device<uint8_t>(cb + n3);
    hs = device<double>(n3); Z = device<double>(n3 * cb);
    S = device<double>(cb * cb); X = device<double>(cb * cb); Sig = device<double>(cb * cb); hc = device<double>(cb);
    map = device<int32_t>(cb); inv = device<int32_t>(cb);
    Rb = device<double>((size_t)ne.N * 36); sel = device<double>((size_t)ne.N * 36); band_out = device<double>((size_t)ne.N * 36);
    cam_out = device<double>(cb * cb);
    flags = device<int>(3);                                  // [0] band, [1] reduced camera system: first refused pivot; [2] k_band_chol_generic's own word (unused)
    for (hipEvent_t& e : ev) e = own.event();
    Lb = device<double>(n3 * (size_t)(bw + 1));               // (last: a non-null Lb says that everything above exists)
  }
  void mark(int s) { MVUS_HIP(hipEventRecord(ev[s], be.stream)); }
  // Tm is as large as Z: its size (and the outputs') is bounded before anything is allocated, and a failed allocation leaves through
  // MVUS_HIP as MVUS_E_HIP
  int ensure_det(const NEView& ne, long long M) {
    if (Tm && det_M == M) return MVUS_OK;
    constexpr unsigned long long kMaxBytes = 1ull << 36;
    const unsigned long long tm_bytes = (unsigned long long)ne.N3 * (unsigned long long)ne.CB * sizeof(double);
    if (tm_bytes > kMaxBytes || (unsigned long long)M * 3 * sizeof(double) > kMaxBytes) { be.err = std::string(who) + ": T = Z Sigma_cc or the outputs exceed 64 GiB"; return MVUS_E_UNSUPPORTED; }
    det_own.reset(); Tm = nullptr; det_M = -1;
    const size_t m = (size_t)std::max<long long>(M, 1);
    Gb = det_own.device<double>((size_t)ne.N * 36);
    det_e = det_own.device<double>(2 * m); det_pcov = det_own.device<double>(3 * m); det_t2 = det_own.device<double>(m);
    for (hipEvent_t& e : det_ev) e = det_own.event();
    Tm = det_own.device<double>((size_t)ne.N3 * (size_t)ne.CB);      // (last: a non-null Tm says that everything above exists)
    det_M = M;
    return MVUS_OK;
  }

  static const char* cam_kind(int k) { return k == 0 ? "alpha" : k == 1 ? "beta" : k == 2 ? "rs" : "camera parameter"; }
  std::string refusal(const std::string& what) const {
    return std::string(who) + ": the pivot of " + what + " is below 1e-10 of its diagonal entry of H: the normal matrix is numerically singular there -- "
           "the gauge is probably free (settings ba_gauge: \"anchor\" / ba_freeze, mvus_ba_set_frozen)";
  }

  // be.x_cur holds x, the analytic Jacobian of x_cur is held, f_cur = f(x); cost = the (robust) cost at x.  Outputs are host pointers (any may be null).
  template <class SC>
  int run(SC& sc, double cost, double sigma2_in, double* cov_cam, double* cov_band, uint8_t* estimated, CovResult& res, const DetCovOut* det = nullptr) {
    const std::string pre = std::string(who) + ": ";
    const auto& hp = be.hp;
    const NEView& ne = sc.ne;
    const hipStream_t st = be.stream;
    const int R = sc.BW + 1;
    // every LDS size is bounded here, from W and CB, before anything is launched
    const size_t lds_chol = (size_t)R * R * sizeof(double), lds_solve = (size_t)R * 64 * sizeof(double), lds_sel = ((size_t)R * R + R) * sizeof(double);
    if (ne.W > kWideW || std::max(lds_chol, std::max(lds_solve, lds_sel)) > 64 * 1024) { be.err = pre + "band wider than " + std::to_string(kWideW) + " control points"; return MVUS_E_UNSUPPORTED; }
    if (ne.CB > 1152) { be.err = pre + "more than 1152 camera-side unknowns"; return MVUS_E_UNSUPPORTED; }
    if (ne.N < 1 || ne.CB < 1) { be.err = pre + "empty problem"; return MVUS_E_INVALID; }
    ensure(ne, sc.BW);
    if (det) { const int rc = ensure_det(ne, hp.M); if (rc != MVUS_OK) return rc; }
    const int tot = ne.CB + ne.N3;
    mark(0);
    sc.assemble_held(be);                                    // stage 1 (the Jacobian itself was evaluated by the caller)
    hipLaunchKernelGGL(k_cov_diag, dim3((tot + 255) / 256), dim3(256), 0, st, ne, diag);
    MVUS_HIP(hipGetLastError());
    std::vector<double> dh((size_t)tot);
    std::vector<int32_t> span_h((size_t)std::max<int64_t>(hp.M, 1));
    MVUS_HIP(hipMemcpyAsync(dh.data(), diag, sizeof(double) * tot, hipMemcpyDeviceToHost, st));
    if (hp.M > 0) MVUS_HIP(hipMemcpyAsync(span_h.data(), be.span, sizeof(int32_t) * hp.M, hipMemcpyDeviceToHost, st));
    MVUS_HIP(hipStreamSynchronize(st));
    // the estimated set, on the host: not frozen and a non-zero diagonal
    std::vector<uint8_t> eh((size_t)tot, 0);
    std::vector<int32_t> map_h, inv_h((size_t)ne.CB, -1);
    std::vector<double> hc_h;
    for (int e = 0; e < ne.CB; ++e) {
      const int64_t col = e % ne.B < 3 ? (int64_t)(e % ne.B) * hp.C + e / ne.B : 3 * (int64_t)hp.C + (int64_t)(e / ne.B) * hp.P + (e % ne.B - 3);
      const bool frozen = !be.frozen_mask.empty() && be.frozen_mask[(size_t)col] != 0;
      if (!frozen && dh[(size_t)e] != 0.0) { eh[(size_t)e] = 1; inv_h[(size_t)e] = (int32_t)map_h.size(); map_h.push_back(e); hc_h.push_back(dh[(size_t)e]); }
    }
    int64_t n_est = (int64_t)map_h.size();
    for (int r = 0; r < ne.N3; ++r) if (dh[(size_t)(ne.CB + r)] != 0.0) { eh[(size_t)(ne.CB + r)] = 1; ++n_est; }
    int64_t m_act = hp.T + be.prior_rows + be.lm_rows;      // (position priors: one row per active (prior, axis) with a weight; landmarks: per (observation, axis))
    for (int64_t i = 0; i < hp.M; ++i) if (span_h[(size_t)i] >= 0) m_act += 2;
    res.dof = m_act - n_est;
    if (estimated) {
      std::memset(estimated, 0, (size_t)hp.n);
      for (int e = 0; e < ne.CB; ++e) {
        const int64_t col = e % ne.B < 3 ? (int64_t)(e % ne.B) * hp.C + e / ne.B : 3 * (int64_t)hp.C + (int64_t)(e / ne.B) * hp.P + (e % ne.B - 3);
        estimated[col] = eh[(size_t)e];
      }
      for (int r = 0; r < ne.N3; ++r) estimated[hp.ctrl_x0[(size_t)(r / 3)] + (int64_t)(r % 3) * hp.ctrl_stride[(size_t)(r / 3)]] = eh[(size_t)(ne.CB + r)];
    }
    if (sigma2_in > 0.0) res.sigma2 = sigma2_in;
    else {
      if (m_act <= n_est) { be.err = pre + std::to_string(m_act) + " active residual rows for " + std::to_string(n_est) + " estimated unknowns: no a-posteriori variance factor (pass sigma2)"; return MVUS_E_INVALID; }
      res.sigma2 = 2.0 * cost / (double)(m_act - n_est);
    }
    const int m = (int)map_h.size();
    MVUS_HIP(hipMemcpyAsync(est, eh.data(), eh.size(), hipMemcpyHostToDevice, st));
    MVUS_HIP(hipMemcpyAsync(inv, inv_h.data(), inv_h.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    if (m > 0) {
      MVUS_HIP(hipMemcpyAsync(map, map_h.data(), map_h.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
      MVUS_HIP(hipMemcpyAsync(hc, hc_h.data(), hc_h.size() * sizeof(double), hipMemcpyHostToDevice, st));
    }
    MVUS_HIP(hipMemsetAsync(flags, 0x7f, 3 * sizeof(int), st));
    MVUS_HIP(hipMemsetAsync(sel, 0, sizeof(double) * (size_t)ne.N * 36, st));
    mark(1);
    // stage 2
    const long long npack = std::max<long long>((long long)ne.N3 * R, (long long)ne.N3 * ne.CB);
    hipLaunchKernelGGL(k_cov_pack, dim3((unsigned)((npack + 255) / 256)), dim3(256), 0, st, ne, sc.BW, (const uint8_t*)est, Lb, hs, Z);
    mark(2);
    // stage 3: the two general band kernels, unchanged (their failure word is the chain's own: the pivots are tested below)
    hipLaunchKernelGGL(k_band_chol_generic, dim3(1), dim3(256), lds_chol, st, ne.N3, sc.BW, Lb, flags + 2);
    hipLaunchKernelGGL(k_band_solve_generic, dim3((unsigned)((ne.CB + 63) / 64)), dim3(64), lds_solve, st, ne.N3, sc.BW, ne.CB, (const double*)Lb, Z);
    hipLaunchKernelGGL(k_cov_band_pivots, dim3((ne.N3 + 255) / 256), dim3(256), 0, st, ne.N3, sc.BW, (const double*)Lb, (const double*)hs, flags);
    mark(3);
    // stage 4
    const int mt = (m + 15) / 16;
    if (m > 0) hipLaunchKernelGGL(k_cov_schur, dim3(mt, mt), dim3(256), 0, st, ne, m, (const int32_t*)map, (const double*)Z, S);
    mark(4);
    // stage 5
    for (int k0 = 0; k0 < m; k0 += kCovNB) {
      const int nb = std::min(kCovNB, m - k0), below = m - (k0 + nb);
      hipLaunchKernelGGL(k_cov_potrf, dim3(1), dim3(64), 0, st, m, k0, nb, S, (const double*)hc, flags);
      if (below > 0) {
        hipLaunchKernelGGL(k_cov_trsm, dim3((below + 63) / 64), dim3(64), 0, st, m, k0, nb, S);
        const int bt = (below + 15) / 16;
        hipLaunchKernelGGL(k_cov_syrk, dim3(bt, bt), dim3(256), 0, st, m, k0, nb, S);
      }
    }
    if (m > 0) hipLaunchKernelGGL(k_cov_tri, dim3((m + 63) / 64), dim3(64), 0, st, m, (const double*)S, X);
    hipLaunchKernelGGL(k_cov_expand, dim3((unsigned)(((long long)ne.CB * ne.CB + 255) / 256)), dim3(256), 0, st, ne.CB, m, (const int32_t*)inv, (const double*)X, Sig);
    mark(5);
    // stage 6
    if (det) hipLaunchKernelGGL((k_cov_tz<true, double*>), dim3((ne.N + kCovTP - 1) / kCovTP), dim3(256), 0, st, ne.N, ne.CB, (const double*)Z, (const double*)Sig, Rb, Tm);
    else hipLaunchKernelGGL(k_cov_tz<>, dim3((ne.N + kCovTP - 1) / kCovTP), dim3(256), 0, st, ne.N, ne.CB, (const double*)Z, (const double*)Sig, Rb);
    mark(6);
    // stage 7
    hipLaunchKernelGGL(k_cov_selinv, dim3(1), dim3(256), lds_sel, st, ne.N3, sc.BW, (const double*)Lb, sel);
    mark(7);
    // stage 8
    hipLaunchKernelGGL(k_cov_band_out, dim3((unsigned)(((long long)ne.N * 36 + 255) / 256)), dim3(256), 0, st, ne.N, ne.CB, (const uint8_t*)est, res.sigma2, (const double*)sel, (const double*)Rb, band_out);
    hipLaunchKernelGGL(k_cov_cam_out, dim3((unsigned)(((long long)ne.CB * ne.CB + 255) / 256)), dim3(256), 0, st, hp.C, hp.P, res.sigma2, (const double*)Sig, cam_out);
    MVUS_HIP(hipGetLastError());
    mark(8);
    // the detection pass, on request: one lane per detection, the camera in the grid's second dimension (its LDS is B x B doubles, B <= 18)
    const bool det_run = det && hp.M > 0 && be.dp.n_chunks > 0;
    if (det_run) {
      int per_cam = 0;
      for (int c = 0; c < hp.C; ++c) per_cam = std::max(per_cam, (int)(hp.cam_chunk_off[(size_t)c + 1] - hp.cam_chunk_off[(size_t)c]));
      be.ensure_cams(be.x_cur);
      MVUS_HIP(hipEventRecord(det_ev[0], st));
      hipLaunchKernelGGL(k_cov_band_out, dim3((unsigned)(((long long)ne.N * 36 + 255) / 256)), dim3(256), 0, st, ne.N, ne.CB, (const uint8_t*)est, 1.0, (const double*)sel, (const double*)Rb, Gb);
      if (per_cam > 0)
        with_flag(hp.calib, [&](auto calib) {
          hipLaunchKernelGGL((k_detcov<calib()>), dim3(per_cam, hp.C), dim3(kThreads), 0, st, be.dp, (const CamState*)be.cams, (const double*)be.x_cur, (const double*)be.J, (const int32_t*)be.span,
                             ne.CB, (const double*)Sig, (const double*)Tm, (const double*)Gb, res.sigma2, det_e, det_pcov, det_t2);
        });
      MVUS_HIP(hipGetLastError());
      MVUS_HIP(hipEventRecord(det_ev[1], st));
    }
    int fl[2] = {INT_MAX, INT_MAX};
    MVUS_HIP(hipMemcpyAsync(fl, flags, sizeof(fl), hipMemcpyDeviceToHost, st));
    MVUS_HIP(hipStreamSynchronize(st));
    for (int s = 0; s < kCovStages; ++s) { float ms = 0.f; MVUS_HIP(hipEventElapsedTime(&ms, ev[s], ev[s + 1])); stage_ms[s] = ms; }
    timed = true;
    if (det) { float ms = 0.f; if (det_run) MVUS_HIP(hipEventElapsedTime(&ms, det_ev[0], det_ev[1])); det_ms = ms; det_timed = true; }
    if (fl[0] >= 0 && fl[0] < ne.N3) {
      be.err = refusal("coordinate " + std::to_string(fl[0] % 3) + " of control point " + std::to_string(fl[0] / 3) + " (spline block)");
      return MVUS_E_NUMERIC;
    }
    if (fl[1] >= 0 && fl[1] < m) {
      const int e = map_h[(size_t)fl[1]], k = e % ne.B;
      be.err = refusal(std::string(cam_kind(k)) + (k >= 3 ? " " + std::to_string(k - 3) : std::string()) + " of camera " + std::to_string(e / ne.B) + " (reduced camera system)");
      return MVUS_E_NUMERIC;
    }
    if (cov_cam) MVUS_HIP(hipMemcpyAsync(cov_cam, cam_out, sizeof(double) * (size_t)ne.CB * ne.CB, hipMemcpyDeviceToHost, st));
    if (cov_band) MVUS_HIP(hipMemcpyAsync(cov_band, band_out, sizeof(double) * (size_t)ne.N * 36, hipMemcpyDeviceToHost, st));
    if (det_run) {
      if (det->e) MVUS_HIP(hipMemcpyAsync(det->e, det_e, sizeof(double) * 2 * (size_t)hp.M, hipMemcpyDeviceToHost, st));
      if (det->pcov) MVUS_HIP(hipMemcpyAsync(det->pcov, det_pcov, sizeof(double) * 3 * (size_t)hp.M, hipMemcpyDeviceToHost, st));
      if (det->t2) MVUS_HIP(hipMemcpyAsync(det->t2, det_t2, sizeof(double) * (size_t)hp.M, hipMemcpyDeviceToHost, st));
    }
    MVUS_HIP(hipStreamSynchronize(st));
    return MVUS_OK;
  }
};

}  // namespace mvus
