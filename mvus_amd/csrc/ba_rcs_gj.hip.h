// Dense solve of the reduced camera system S x = b (nn <= 1152, SPD) by BLOCK GAUSS-JORDAN, 32-column panels, ONE
// launch per panel and no back substitution.  The right-hand side rides along as row nn of the (nn+1) x nn array
// (row-major, both triangles of S filled).  In column-operation form, with P_k the inverse of the current pivot block:
//     every row block I below the panel (the rhs row included), every column block J != k:
//         Q_I = M[I][k] P_k ;   M[I][J] -= Q_I M[k][J] ;   M[I][k] <- Q_I
// After the last panel the rhs row holds x.  Rows above the panel are never touched again, the trailing block stays the
// (symmetric positive definite) Schur complement.  Each step reads `src` and writes `dst` (ping-pong), so all tiles of a
// step are independent.  Against a blocked Cholesky this trades ~3x the (tiny, perfectly parallel) tile flops for the
// removal of the sequential back substitution (44 us at nn = 288: nine dependent round trips to data other XCDs wrote).
//
// The critical path per panel is the inverse of the 32x32 pivot block, done by ONE wavefront of the workgroup that
// produced that block (pivot_inverse_wave): 2x2 blocks of 16 -- Cholesky + inverse factor of a 16x16 block in registers
// (row of the block and of the identity per lane, multipliers by DPP row broadcast, 1/d by v_rcp_f64 + 2 Newton steps), the Schur complement, the off-diagonal block of L^-1 and P = L^-T L^-1 on the fp64 matrix cores.
// Round 2 history (cycle counters, MVUS_GJ_PROBE): a 32-step register Cholesky took 22k cycles and the tile update 13k
// (three 32-deep LDS dot products per thread: LDS-bandwidth bound); now 16-step halves + matrix-core tile products.

// The default solve of the reduced system is the blocked L D L^T of ba_rcs.hip.h; this one is selected by ba_switches.h.
#pragma once
#include <hip/hip_runtime.h>

#include "ba_rcs.hip.h"                // rcs_ldl16
#include "ba_schur_product.hip.h"      // kNB, kPivScratch
#include "ba_wave.hip.h"

namespace mvus {

// acc += op(A) op(B) for 16x16 blocks in LDS (stride lda / ldb), K = 16: ta: A is read transposed, tb: B is.
__device__ __forceinline__ d4 mma16(const double* __restrict__ A, int lda, bool ta, const double* __restrict__ B, int ldb, bool tb, d4 acc) {
  const int lane = threadIdx.x & 63, lr = lane & 15, lk = lane >> 4;
#pragma unroll
  for (int s_ = 0; s_ < 4; ++s_) {
    const int k = 4 * s_ + lk;
    const double av = ta ? A[k * lda + lr] : A[lr * lda + k];
    const double bv = tb ? B[lr * ldb + k] : B[k * ldb + lr];
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
  }
  return acc;
}
__device__ __forceinline__ void store16(double* __restrict__ M, int ld, d4 acc, double sign) {
  const int lane = threadIdx.x & 63, lr = lane & 15, lk = lane >> 4;
#pragma unroll
  for (int r = 0; r < 4; ++r) M[(lk + 4 * r) * ld + lr] = sign * acc[r];
}

// first wavefront of the workgroup: inverse P of the SPD block in Dm (lower part valid, identity padded beyond the
// block) -> Pout[r*kNB+c], both triangles.  2x2 blocks of 16:  A11^-1 = X1^T D1^-1 X1 (ldl_inv16),  T = A21 A11^-1,
// S = A22 - T A21^T,  P22 = S^-1 (ldl_inv16 again),  P21 = -P22 T,  P11 = A11^-1 - T^T P21.  W: kPivScratch doubles of LDS.
__device__ __forceinline__ void pivot_inverse_wave(double (*Dm)[kNB + 1], double* __restrict__ W, double* __restrict__ Pout, int* __restrict__ fail) {
  constexpr int LD = 17, LDD = kNB + 1;
  const int lane = threadIdx.x & 63, row = lane & 15, lr = lane & 15, lk = lane >> 4;
  const d4 zero{0.0, 0.0, 0.0, 0.0};
  double* M1 = W;                 // X (unit lower inverse factor of the block being inverted)
  double* M2 = W + 16 * LD;       // D^-1 X
  double* M3 = W + 2 * 16 * LD;   // A11^-1
  double* M4 = W + 3 * 16 * LD;   // T, later P21
  double* M5 = W + 4 * 16 * LD;   // S, later P22
  double a[16], x[16], rd[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) {          // unconditional LDS reads, then selects: no branch per element (every row of 16 lanes the same)
    const double t = Dm[row][k];
    a[k] = k <= row ? t : 0.0;
    x[k] = k == row ? 1.0 : 0.0;
  }
  rcs_ldl16(a, x, rd, lane, fail);
  if (lane < 32) {                        // lanes 0..15 store X, lanes 16..31 (the same values) D^-1 X
    double* dst = (lane < 16 ? M1 : M2) + row;
#pragma unroll
    for (int k = 0; k < 16; ++k) dst[k * LD] = lane < 16 ? x[k] : rd[k] * x[k];
  }
  lds_wave_sync();
  d4 a11 = mma16(M1, LD, true, M2, LD, false, zero);                 // A11^-1 = X^T (D^-1 X)
  store16(M3, LD, a11, 1.0);
  lds_wave_sync();
  d4 acc = mma16(&Dm[16][0], LDD, false, M3, LD, false, zero);       // T = A21 A11^-1
  store16(M4, LD, acc, 1.0);
  lds_wave_sync();
  acc = mma16(M4, LD, false, &Dm[16][0], LDD, true, zero);               // T A21^T
#pragma unroll
  for (int r = 0; r < 4; ++r) M5[(lk + 4 * r) * LD + lr] = Dm[16 + lk + 4 * r][16 + lr] - acc[r];
  lds_wave_sync();
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const double t = M5[row * LD + k];
    a[k] = k <= row ? t : 0.0;
    x[k] = k == row ? 1.0 : 0.0;
  }
  rcs_ldl16(a, x, rd, lane, fail);
  if (lane < 32) {
    double* dst = (lane < 16 ? M1 : M2) + row;
#pragma unroll
    for (int k = 0; k < 16; ++k) dst[k * LD] = lane < 16 ? x[k] : rd[k] * x[k];
  }
  lds_wave_sync();
  const d4 p22 = mma16(M1, LD, true, M2, LD, false, zero);           // S^-1
  store16(M5, LD, p22, 1.0);
  lds_wave_sync();
  const d4 p21 = mma16(M5, LD, false, M4, LD, false, zero);          // P22 T  (sign applied on use)
  lds_wave_sync();                                                       // every lane has read T before it is overwritten
  store16(M4, LD, p21, -1.0);
  lds_wave_sync();
  const d4 tp = mma16(&Dm[16][0], LDD, true, M4, LD, false, zero);   // A21^T P21;  T^T = A11^-1 A21^T  =>  T^T P21 = A11^-1 (A21^T P21)
  store16(M1, LD, tp, 1.0);
  lds_wave_sync();
  const d4 corr = mma16(M3, LD, false, M1, LD, false, zero);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int rw = lk + 4 * r;
    Pout[rw * kNB + lr] = a11[r] - corr[r];
    Pout[(16 + rw) * kNB + lr] = -p21[r];
    Pout[lr * kNB + 16 + rw] = -p21[r];
    Pout[(16 + rw) * kNB + 16 + lr] = p22[r];
  }
}

// one panel step; grid (row tiles below the panel incl. the rhs row, all column tiles); pc != nullptr on the last step.
// Four wavefronts, one 16x16 quarter of the tile each; both tile products on the fp64 matrix cores.
constexpr int kGjThreads = 256;
__global__ __launch_bounds__(kGjThreads) void k_gj_step(int nn, int kb, const double* __restrict__ src, double* __restrict__ dst,
                                                        double* __restrict__ Pinv, int* __restrict__ fail, double* __restrict__ pc) {
  constexpr int kTile = kNB * (kNB + 1);
  __shared__ double lds[4 * kTile];
  double (*Ai)[kNB + 1] = reinterpret_cast<double (*)[kNB + 1]>(lds);
  double (*Pk)[kNB + 1] = reinterpret_cast<double (*)[kNB + 1]>(lds + kTile);
  double (*Q)[kNB + 1] = reinterpret_cast<double (*)[kNB + 1]>(lds + 2 * kTile);
  double (*Bk)[kNB + 1] = reinterpret_cast<double (*)[kNB + 1]>(lds + 3 * kTile);      // Q and Bk: one contiguous scratch area later
  const int nb = min(kNB, nn - kb), base = kb + nb;
  const int i0 = base + blockIdx.x * kNB, j0 = blockIdx.y * kNB;
  const bool pivcol = j0 == kb;                              // this tile is column block k: it stores Q_I
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lr = lane & 15, lk = lane >> 4;
  const int br = (wave >> 1) * 16, bc = (wave & 1) * 16;     // this wavefront's quarter
#pragma unroll
  for (int q = 0; q < kNB * kNB / kGjThreads; ++q) {
    const int e = threadIdx.x + kGjThreads * q, r = e / kNB, c = e % kNB;
    // (indices clamped into the (nn + 1) x nn array, values outside the tile replaced afterwards: sixteen unconditional loads in
    // flight together instead of a branch around each -- the tile update is on the chain of every panel)
    const double ai = src[(long long)min(i0 + r, nn) * nn + min(kb + c, nn - 1)];
    const double bk = src[(long long)min(kb + r, nn) * nn + min(j0 + c, nn - 1)];
    Ai[r][c] = (i0 + r <= nn && c < nb) ? ai : 0.0;
    Pk[r][c] = Pinv[(long long)(kb / kNB) * kNB * kNB + e];
    Bk[r][c] = (r < nb && j0 + c < nn) ? bk : 0.0;
  }
  double v[4];                                               // the tile itself, in the accumulator layout
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = i0 + br + lk + 4 * r, j = j0 + bc + lr;
    const double t = src[(long long)min(i, nn) * nn + min(j, nn - 1)];
    v[r] = (i <= nn && j < nn && !pivcol) ? t : 0.0;
  }
  __syncthreads();
  d4 acc{0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int s_ = 0; s_ < kNB / 4; ++s_) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(Ai[br + lr][4 * s_ + lk], Pk[4 * s_ + lk][bc + lr], acc, 0, 0, 0);
#pragma unroll
  for (int r = 0; r < 4; ++r) Q[br + lk + 4 * r][bc + lr] = acc[r];
  __syncthreads();
  if (pivcol) {
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = acc[r];
  } else {
    d4 upd{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int s_ = 0; s_ < kNB / 4; ++s_) upd = __builtin_amdgcn_mfma_f64_16x16x4f64(Q[br + lr][4 * s_ + lk], Bk[4 * s_ + lk][bc + lr], upd, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] -= upd[r];
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = i0 + br + lk + 4 * r, j = j0 + bc + lr;
    if (i <= nn && j < nn && (!pivcol || bc + lr < nb)) {
      dst[(long long)i * nn + j] = v[r];
      if (pc && i == nn) pc[j] = -v[r];                      // last panel: the rhs row is the solution
    }
  }
  // the tile holding the next pivot block inverts it
  const int nb2 = min(kNB, nn - base);
  if (blockIdx.x != 0 || j0 != base || nb2 <= 0) return;
  __syncthreads();                                           // Ai is reused as the block to invert, Q and Bk as scratch
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int rr = br + lk + 4 * r, cc = bc + lr;
    Ai[rr][cc] = (rr < nb2 && cc < nb2 && cc <= rr) ? v[r] : ((rr < nb2 && cc < nb2) ? 0.0 : (rr == cc ? 1.0 : 0.0));
  }
  __syncthreads();
  static_assert(kPivScratch <= 2 * kNB * (kNB + 1), "pivot scratch must fit Q and Bk");
  if (threadIdx.x < 64) pivot_inverse_wave(Ai, &Q[0][0], Pinv + (long long)(base / kNB) * kNB * kNB, fail);
}

}  // namespace mvus
