// The separator system of the partitioned band solver (block tridiagonal, blocks of 3 (W - 1)): the sequential block Cholesky, block
// cyclic reduction (a launch per level, all wide levels in one launch, the one-workgroup tail), and the two-level elimination of time
// shards.  Which one runs is decided by the host (ba_schur_host.hip.h) from ba_switches.h.
#pragma once
#include <hip/hip_runtime.h>

#include "ba_band_part.hip.h"      // part_reduce_rhs
#include "ba_ne_views.h"
#include "ba_partition.h"
#include "ba_wave.hip.h"

namespace mvus {

// block-tridiagonal Cholesky of the separator system by ONE wavefront (no workgroup barriers needed between
// the tiny dependent steps): T[q] <- C_q (lower factor of the q-th pivot block), U[q] <- L(q+1,q) = U_q^T C_q^-T
template <int S3>
__global__ __launch_bounds__(64) void k_sep_factor(PartView pv, int* __restrict__ fail) {
  __shared__ double Cq[S3 * S3];
  __shared__ double Lq[S3 * S3];
  __shared__ double Uq[S3 * S3];
  const int nq = pv.m, lane = threadIdx.x;
  constexpr int kPer = (S3 * S3 + 63) / 64;          // entries of T_q / U_q held per lane
  double tn[kPer], un[kPer];                         // next step's blocks, fetched one step ahead
#pragma unroll
  for (int r = 0; r < kPer; ++r) {
    const int e = lane + 64 * r;
    tn[r] = (nq > 0 && e < S3 * S3) ? pv.T[e] : 0.0;
    un[r] = (nq > 0 && e < S3 * S3) ? pv.U[e] : 0.0;
  }
  for (int q = 0; q < nq; ++q) {
    double* Tq = pv.T + (long long)q * S3 * S3;
    double* Ug = pv.U + (long long)q * S3 * S3;
#pragma unroll
    for (int r = 0; r < kPer; ++r) {
      const int e = lane + 64 * r;
      if (e < S3 * S3) {
        const int a = e / S3, b = e % S3;
        double v = tn[r];
        if (q > 0) for (int k = 0; k < S3; ++k) v -= Lq[a * S3 + k] * Lq[b * S3 + k];
        Cq[e] = v;
        Uq[e] = un[r];
      }
    }
    if (q + 1 < nq) {
#pragma unroll
      for (int r = 0; r < kPer; ++r) {
        const int e = lane + 64 * r;
        if (e < S3 * S3) { tn[r] = Tq[S3 * S3 + e]; un[r] = Ug[S3 * S3 + e]; }
      }
    }
    __syncthreads();
    // right-looking Cholesky of the S3 x S3 block, lanes over the trailing entries
    for (int k = 0; k < S3; ++k) {
      double d = Cq[k * S3 + k];
      if (!(d > 0.0)) { if (lane == 0) fail[0] = 3; d = 1.0; }
      d = sqrt(d);
      __syncthreads();
      if (lane == 0) Cq[k * S3 + k] = d;
      if (lane > k && lane < S3) Cq[lane * S3 + k] /= d;
      __syncthreads();
      for (int e = lane; e < S3 * S3; e += 64) {
        const int a = e / S3, b = e % S3;
        if (a > k && b > k && b <= a) Cq[e] -= Cq[a * S3 + k] * Cq[b * S3 + k];
      }
      __syncthreads();
    }
    for (int e = lane; e < S3 * S3; e += 64) Tq[e] = (e / S3 == e % S3) ? 1.0 / Cq[e] : Cq[e];      // diagonal inverted for k_sep_rhs
    if (q + 1 < nq) {
      if (lane < S3) {                       // row `lane` of L(q+1,q): solve C_q l = U_q[:, lane]
        double l[S3];
        for (int k = 0; k < S3; ++k) {
          double sacc = Uq[k * S3 + lane];
          for (int jj = 0; jj < k; ++jj) sacc -= Cq[k * S3 + jj] * l[jj];
          l[k] = sacc / Cq[k * S3 + k];
        }
        for (int k = 0; k < S3; ++k) Lq[lane * S3 + k] = l[k];
      }
      __syncthreads();
      for (int e = lane; e < S3 * S3; e += 64) Ug[e] = Lq[e];
    }
    __syncthreads();
  }
}

// forward / backward substitution of every right-hand side through the factored separator system: one thread per
// column, no synchronisation (the factors are read-only and identical for all lanes, so they are fetched as
// broadcasts through the caches); the next step's right-hand-side rows are fetched before the current step's
// dependent chain, and the diagonal of C_q is stored inverted (k_sep_factor) so the chain has no divisions.
template <int S3>
__global__ __launch_bounds__(64) void k_sep_rhs(PartView pv, int ncols) {
  double* __restrict__ Rr = pv.R;
  const int col = blockIdx.x * blockDim.x + threadIdx.x;
  if (col >= ncols) return;
  const int nq = pv.m;
  double prev[S3], rv[S3], nx[S3];
#pragma unroll
  for (int a = 0; a < S3; ++a) { prev[a] = 0.0; nx[a] = Rr[((long long)(0) * S3 + a) * ncols + col]; }
  for (int q = 0; q < nq; ++q) {
    const double* __restrict__ Cq = pv.T + (long long)q * S3 * S3;
    const double* __restrict__ Lq = pv.U + (long long)(q - 1) * S3 * S3;     // L(q, q-1)
#pragma unroll
    for (int a = 0; a < S3; ++a) rv[a] = nx[a];
    if (q + 1 < nq) {
#pragma unroll
      for (int a = 0; a < S3; ++a) nx[a] = Rr[((long long)(q + 1) * S3 + a) * ncols + col];
    }
    if (q > 0) {
#pragma unroll
      for (int a = 0; a < S3; ++a)
#pragma unroll
        for (int k = 0; k < S3; ++k) rv[a] -= Lq[a * S3 + k] * prev[k];
    }
#pragma unroll
    for (int a = 0; a < S3; ++a) {
      double sacc = rv[a];
#pragma unroll
      for (int jj = 0; jj < S3; ++jj) if (jj < a) sacc -= Cq[a * S3 + jj] * rv[jj];
      rv[a] = sacc * Cq[a * S3 + a];            // diagonal stored as 1 / C(a,a)
    }
#pragma unroll
    for (int a = 0; a < S3; ++a) { prev[a] = rv[a]; Rr[((long long)(q) * S3 + a) * ncols + col] = rv[a]; }
  }
#pragma unroll
  for (int a = 0; a < S3; ++a) nx[a] = prev[a];
  for (int q = nq - 1; q >= 0; --q) {
    const double* __restrict__ Cq = pv.T + (long long)q * S3 * S3;
    const double* __restrict__ Ln = pv.U + (long long)q * S3 * S3;           // L(q+1, q)
#pragma unroll
    for (int a = 0; a < S3; ++a) rv[a] = nx[a];
    if (q > 0) {
#pragma unroll
      for (int a = 0; a < S3; ++a) nx[a] = Rr[((long long)(q - 1) * S3 + a) * ncols + col];
    }
    if (q + 1 < nq) {
#pragma unroll
      for (int k = 0; k < S3; ++k)
#pragma unroll
        for (int a = 0; a < S3; ++a) rv[a] -= Ln[k * S3 + a] * prev[k];
    }
#pragma unroll
    for (int a = S3 - 1; a >= 0; --a) {
      double sacc = rv[a];
#pragma unroll
      for (int jj = 0; jj < S3; ++jj) if (jj > a) sacc -= Cq[jj * S3 + a] * rv[jj];
      rv[a] = sacc * Cq[a * S3 + a];
    }
#pragma unroll
    for (int a = 0; a < S3; ++a) { prev[a] = rv[a]; Rr[((long long)(q) * S3 + a) * ncols + col] = rv[a]; }
  }
}

// ---- block cyclic reduction of the separator system ---------------------------------------------------------
// The sequential block-tridiagonal Cholesky above walks P-1 dependent steps.  Cyclic reduction needs only
// ceil(log2(P)) of them: at stride h the nodes j with (j+1)/h odd are eliminated, x_j = D_j^-1 (r_j - A_j x_{j-h} -
// C_j x_{j+h}), and folded into their neighbours at distance h, which form the next (half as long) block-tridiagonal
// system.  Every Schur complement of an SPD matrix is SPD, so no pivoting is needed.  Stored per node, at the level
// that eliminates it: Dinv_j (in U2), Ha_j = Dinv_j A_j, Hc_j = Dinv_j C_j; only the coupling to the right neighbour,
// C_j, is carried through the levels (A_j = C_{j-h}^T).
//   survivors i:  D_i -= C_{i-h}^T Hc_{i-h} + C_i Ha_{i+h},   C_i <- -C_i Hc_{i+h},   r_i -= Hc_{i-h}^T r_{i-h} + Ha_{i+h}^T r_{i+h}
// k_sep_bcr_level / k_sep_bcr_tail: the matrix part, a wavefront per survivor (bcr_survivor below);
// k_sep_bcr_rhs: the right-hand sides, kBcrCols columns per workgroup staged in LDS through all levels and back.
// One S3 x S3 product on the fp64 matrix cores, one wavefront: acc += op(A) op(B), the blocks zero-padded to 16 x 16.
// ta: A is read transposed; tb: B is read transposed.  Fragment layout of v_mfma_f64_16x16x4: lane l holds
// A[l&15][k0 + (l>>4)] and B[k0 + (l>>4)][l&15].
template <int S3>
struct BcrFrag { double a[(S3 + 3) / 4], b[(S3 + 3) / 4]; };
template <int S3>
__device__ __forceinline__ void bcr_load(BcrFrag<S3>& f, const double* __restrict__ A, bool ta, const double* __restrict__ Bm, bool tb, bool on) {
  const int lane = threadIdx.x & 63, lr = lane & 15, lk = lane >> 4;
#pragma unroll
  for (int s_ = 0; s_ < (S3 + 3) / 4; ++s_) {
    const int k = 4 * s_ + lk;
    const bool ok = on && lr < S3 && k < S3;
    f.a[s_] = ok ? (ta ? A[k * S3 + lr] : A[lr * S3 + k]) : 0.0;
    f.b[s_] = ok ? (tb ? Bm[lr * S3 + k] : Bm[k * S3 + lr]) : 0.0;
  }
}
template <int S3>
__device__ __forceinline__ d4 bcr_mma(const BcrFrag<S3>& f, d4 acc) {
#pragma unroll
  for (int s_ = 0; s_ < (S3 + 3) / 4; ++s_) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(f.a[s_], f.b[s_], acc, 0, 0, 0);
  return acc;
}

#ifndef MVUS_BCR_WAVES
#define MVUS_BCR_WAVES 16
#endif
#ifndef MVUS_BCR_TAIL_NS
#define MVUS_BCR_TAIL_NS 16
#endif
constexpr int kBcrWaves = MVUS_BCR_WAVES;      // wavefronts of the one workgroup that runs the last levels (S3 = 15: half, LDS)
constexpr int kBcrTailNs = MVUS_BCR_TAIL_NS;   // levels with more survivors than this get a launch of their own (one wavefront per survivor)


// One survivor of one level, by ONE wavefront and without any exchange with other wavefronts: the survivor i = 2h(s+1)-1
// inverts the diagonal blocks of BOTH eliminated neighbours jL = i-h and jR = i+h itself (its neighbours two places on
// do the same work again -- 2x redundant and free, the level is latency bound), forms Hc_jL, Ha_jR, Hc_jR on the matrix
// cores and applies them to its own D_i and C_i, in place: at one level D_i and C_i are touched by this wavefront only,
// the blocks of eliminated nodes are only read.  The inverses therefore go to a buffer of their own (U2), not over T.
// Stored for k_sep_bcr_rhs: Dinv_j, Ha_j, Hc_j of jR (and of jL for the first survivor, whose left neighbour nobody else
// owns).  s = 0 with no survivor at all is the last level: the one remaining node is inverted.
// w: 3 * S3 * S3 doubles of LDS private to the wavefront.
// The blocks read here may have been written by ANOTHER wavefront of the same workgroup one level earlier (k_sep_bcr_tail), and a
// 128-byte line can straddle two 648-byte blocks: a line fetched into the CU's L1 for one block before a neighbour's store to
// the other landed would be stale at the next level.  Agent-scope loads go to L2, where the stores are.
__device__ __forceinline__ double bcr_ld(const double* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// Gauss-Jordan inverse of an S3 x S3 SPD block held a row per lane (lane a of a row of 16 lanes: block row a; lanes >= S3 carry
// zeros): step K broadcasts the pivot row with DPP row_newbcast:K.  Template recursion: the DPP control is an immediate.
template <int S3, int K>
struct BcrGaussJordan {
  static __device__ __forceinline__ void run(double (&row)[S3], int a, bool& bad) {
    double pr[S3];
#pragma unroll
    for (int b = 0; b < S3; ++b) pr[b] = row_bcast<K>(row[b]);
    double piv = pr[K];
    bad |= !(piv > 0.0);
    piv = piv > 0.0 ? piv : 1.0;
    double ip = __builtin_amdgcn_rcp(piv);
    ip = ip * (2.0 - piv * ip);
    ip = ip * (2.0 - piv * ip);
    if (a == K) {
#pragma unroll
      for (int b = 0; b < S3; ++b) row[b] = (b == K) ? ip : row[b] * ip;
    } else {
      const double f = row[K] * ip;
#pragma unroll
      for (int b = 0; b < S3; ++b) row[b] = (b == K) ? -f : row[b] - f * pr[b];
    }
    BcrGaussJordan<S3, K + 1>::run(row, a, bad);
  }
};
template <int S3>
struct BcrGaussJordan<S3, S3> { static __device__ __forceinline__ void run(double (&)[S3], int, bool&) {} };

template <int S3, bool WT = false>      // WT: T_i and C_i leave as agent-scope write-through stores (readers in other workgroups of the SAME launch: k_sep_bcr_levels)
__device__ __forceinline__ void bcr_survivor(const PartView& pv, int h, int s, double* __restrict__ w, int* __restrict__ fail) {
  constexpr int SS = S3 * S3, KS = (S3 + 3) / 4;
  const int m = pv.m, lane = threadIdx.x & 63, lr = lane & 15, lk = lane >> 4;
  const int i = 2 * h * (s + 1) - 1, jL = i - h, jR = i + h;
  const bool has_i = i < m, right = jR < m, right2 = jR + h < m;
  double* __restrict__ Cc = pv.U;
  // ---- all global operands, issued together ----
  // (block row a of neighbour nl in lane 16 nl + a: each neighbour's rows inside one row of 16 lanes, so that the pivot row of the
  // elimination below is a DPP row broadcast -- v_mov_b64_dpp row_newbcast -- instead of two ds_bpermute per entry)
  static_assert(S3 <= 16, "a block row per lane inside one DPP row");
  const int nl = lane >> 4, a = lane & 15;
  const bool act = a < S3 && (nl == 0 || (nl == 1 && right));
  const double* Tsrc = pv.T + (long long)(nl == 0 ? jL : (right ? jR : 0)) * SS + (a < S3 ? a : 0) * S3;
  double row[S3];
#pragma unroll
  for (int b = 0; b < S3; ++b) row[b] = act ? bcr_ld(Tsrc + b) : (a == b ? 1.0 : 0.0);
  double cL[KS], ci[KS], cR[KS], ti[4];
#pragma unroll
  for (int s_ = 0; s_ < KS; ++s_) {
    const int k = 4 * s_ + lk;
    const bool ok = lr < S3 && k < S3;
    cL[s_] = (ok && has_i) ? bcr_ld(Cc + (long long)jL * SS + k * S3 + lr) : 0.0;        // C_jL[k][lr]: B operand of Hc_jL, A operand (transposed) of the D update
    ci[s_] = (ok && right) ? bcr_ld(Cc + (long long)i * SS + lr * S3 + k) : 0.0;         // C_i[lr][k]: B operand (transposed) of Ha_jR, A operand of both updates
    cR[s_] = (ok && right2) ? bcr_ld(Cc + (long long)jR * SS + k * S3 + lr) : 0.0;       // C_jR[k][lr]
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) { const int rw = lk + 4 * r; ti[r] = (has_i && rw < S3 && lr < S3) ? bcr_ld(pv.T + (long long)i * SS + rw * S3 + lr) : 0.0; }
  // ---- Dinv of both neighbours: a block row per lane, the pivot row of each Gauss-Jordan step broadcast with shuffles ----
  bool bad = false;
  BcrGaussJordan<S3, 0>::run(row, a, bad);
  if (bad && act) fail[0] = 3;
  if (nl < 2 && a < S3) {
#pragma unroll
    for (int b = 0; b < S3; ++b) w[nl * SS + a * S3 + b] = row[b];
    if (nl == 0 ? s == 0 : right) {
      double* Dg = pv.U2 + (long long)(nl == 0 ? jL : jR) * SS + a * S3;
#pragma unroll
      for (int b = 0; b < S3; ++b) Dg[b] = row[b];
    }
  }
  lds_wave_sync();
  // ---- Hc_jL = Dinv_jL C_jL, Ha_jR = Dinv_jR C_i^T, Hc_jR = Dinv_jR C_jR ----
  double aL[KS], aR[KS];
#pragma unroll
  for (int s_ = 0; s_ < KS; ++s_) {
    const int k = 4 * s_ + lk;
    const bool ok = lr < S3 && k < S3;
    aL[s_] = ok ? w[lr * S3 + k] : 0.0;
    aR[s_] = (ok && right) ? w[SS + lr * S3 + k] : 0.0;
  }
  d4 hcl{0.0, 0.0, 0.0, 0.0}, har{0.0, 0.0, 0.0, 0.0}, hcr{0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int s_ = 0; s_ < KS; ++s_) {
    hcl = __builtin_amdgcn_mfma_f64_16x16x4f64(aL[s_], cL[s_], hcl, 0, 0, 0);
    har = __builtin_amdgcn_mfma_f64_16x16x4f64(aR[s_], ci[s_], har, 0, 0, 0);
    hcr = __builtin_amdgcn_mfma_f64_16x16x4f64(aR[s_], cR[s_], hcr, 0, 0, 0);
  }
  lds_wave_sync();
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int rw = lk + 4 * r;
    if (rw < S3 && lr < S3) {
      const int e = rw * S3 + lr;
      w[e] = hcl[r]; w[SS + e] = har[r]; w[2 * SS + e] = hcr[r];
      if (s == 0) { pv.Ha[(long long)jL * SS + e] = 0.0; pv.Hc[(long long)jL * SS + e] = hcl[r]; }
      if (right) { pv.Ha[(long long)jR * SS + e] = har[r]; pv.Hc[(long long)jR * SS + e] = hcr[r]; }
    }
  }
  if (!has_i) return;                                  // wave-uniform: the last level has no survivor
  lds_wave_sync();
  // ---- D_i -= C_jL^T Hc_jL + C_i Ha_jR,  C_i <- -C_i Hc_jR ----
  d4 dacc{0.0, 0.0, 0.0, 0.0}, cacc{0.0, 0.0, 0.0, 0.0};
  double b1[KS], b2[KS], b3[KS];
#pragma unroll
  for (int s_ = 0; s_ < KS; ++s_) {
    const int k = 4 * s_ + lk;
    const bool ok = lr < S3 && k < S3;
    b1[s_] = ok ? w[k * S3 + lr] : 0.0;
    b2[s_] = ok ? w[SS + k * S3 + lr] : 0.0;
    b3[s_] = ok ? w[2 * SS + k * S3 + lr] : 0.0;
  }
#pragma unroll
  for (int s_ = 0; s_ < KS; ++s_) dacc = __builtin_amdgcn_mfma_f64_16x16x4f64(cL[s_], b1[s_], dacc, 0, 0, 0);
#pragma unroll
  for (int s_ = 0; s_ < KS; ++s_) dacc = __builtin_amdgcn_mfma_f64_16x16x4f64(ci[s_], b2[s_], dacc, 0, 0, 0);
#pragma unroll
  for (int s_ = 0; s_ < KS; ++s_) cacc = __builtin_amdgcn_mfma_f64_16x16x4f64(ci[s_], b3[s_], cacc, 0, 0, 0);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int rw = lk + 4 * r;
    if (rw < S3 && lr < S3) {
      if constexpr (WT) {
        __hip_atomic_store(pv.T + (long long)i * SS + rw * S3 + lr, ti[r] - dacc[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(Cc + (long long)i * SS + rw * S3 + lr, 0.0 - cacc[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      } else {
        pv.T[(long long)i * SS + rw * S3 + lr] = ti[r] - dacc[r];
        Cc[(long long)i * SS + rw * S3 + lr] = 0.0 - cacc[r];
      }
    }
  }
}

// one level in a launch of its own: one wavefront (= workgroup) per survivor
template <int S3>
__global__ __launch_bounds__(64) void k_sep_bcr_level(PartView pv, int h, int* __restrict__ fail) {
  __shared__ double w[3 * S3 * S3];
  bcr_survivor<S3>(pv, h, blockIdx.x, w, fail);
}
// ALL the wide levels in ONE launch (round 6): workgroup b is survivor s of level L (levels in launch order: the first ones have the
// lowest block indices), and a survivor of level L >= 1 waits until the three nodes it reads -- itself and its two neighbours, all
// survivors of level L - 1 -- carry the mark of that level.  Hand-over as in k_rcs_factor (the CDNA guide's Guideline 16): the
// producer's T_i and C_i go out as agent-scope (sc1, write-through) stores, s_waitcnt vmcnt(0), then ONE lane stores done[i] = epoch + L
// + 1 with a relaxed agent-scope atomic; the consumer polls with relaxed agent-scope loads (s_sleep, BOUNDED: a time-out raises
// fail[0] = kFailHandoverCode and the sticky fail[2], the host then repeats the solve with a launch per level) and reads the blocks with
// agent-scope loads (bcr_ld).  `epoch` grows by 8 per solve: the marks are never reset.  Three launches of ~5 us (a ramp and two or
// three memory round trips each) become one of ~7.
template <int S3>
__global__ __launch_bounds__(64) void k_sep_bcr_levels(PartView pv, BcrLevels lv, unsigned* __restrict__ done, unsigned epoch, unsigned spin_limit, int* __restrict__ fail) {
  __shared__ double w[3 * S3 * S3];
  int L = 0;
#pragma unroll
  for (int l = 1; l < 4; ++l) if (l < lv.nlev && (int)blockIdx.x >= lv.first[l]) L = l;
  const int h = lv.h[L], s = (int)blockIdx.x - lv.first[L];
  const int i = 2 * h * (s + 1) - 1, jL = i - h, jR = i + h;
  if (L > 0 && threadIdx.x == 0) {
    const unsigned want = epoch + (unsigned)L;
    unsigned spins = 0;
    while (true) {
      const unsigned a = __hip_atomic_load(done + jL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const unsigned b = i < pv.m ? __hip_atomic_load(done + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : want;
      const unsigned c = jR < pv.m ? __hip_atomic_load(done + jR, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : want;
      if ((int)(a - want) >= 0 && (int)(b - want) >= 0 && (int)(c - want) >= 0) break;
      __builtin_amdgcn_s_sleep(4);
      if (++spins > spin_limit) { fail[0] = kFailHandoverCode; fail[2] = 1; break; }
    }
  }
  __builtin_amdgcn_wave_barrier();
  bcr_survivor<S3, true>(pv, h, s, w, fail);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if (threadIdx.x == 0 && i < pv.m) __hip_atomic_store(done + i, epoch + (unsigned)L + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// the remaining levels from stride h0 on, one workgroup: a wavefront per survivor, one barrier per level
constexpr int bcr_tail_waves(int s3) { return s3 > 9 ? kBcrWaves / 2 : kBcrWaves; }
template <int S3>
__device__ __forceinline__ void bcr_tail_body(const PartView& pv, int h0, int* __restrict__ fail, double* __restrict__ w) {
  constexpr int NW = bcr_tail_waves(S3);
  const int wave = threadIdx.x >> 6;
  for (int h = h0; h <= pv.m; h <<= 1) {
    const int ns = pv.m / (2 * h), nt = ns > 0 ? ns : 1;
    for (int s = wave; s < nt; s += NW) bcr_survivor<S3>(pv, h, s, w + wave * 3 * S3 * S3, fail);
    // The next level's loads (bcr_ld: agent scope, they bypass the CU's L1 and read L2) must see this level's plain stores of the
    // OTHER wavefronts of this workgroup.  All of them run on one CU, hence behind one L2: what is needed is that the stores have
    // ARRIVED there before anybody passes the barrier, i.e. that their acknowledgements are in (vmcnt = 0) -- a workgroup-scope
    // barrier by itself does not wait for that.  (A full agent-scope release, __threadfence(), also writes the XCD's L2 back for the
    // benefit of other XCDs -- `buffer_wbl2 sc1` -- which nothing here needs: measured +15 us per solve.)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }
}
template <int S3>
__global__ __launch_bounds__(bcr_tail_waves(S3) * 64) void k_sep_bcr_tail(PartView pv, int h0, int* __restrict__ fail) {
  __shared__ double w[bcr_tail_waves(S3) * 3 * S3 * S3];
  bcr_tail_body<S3>(pv, h0, fail, w);
}
// The last levels of the cyclic reduction run in ONE workgroup (29 us of barriers); the right-hand sides of the separator system
// (k_part_reduce's second half, ~12 us over ~460 workgroups) need nothing from it: same launch, workgroup 0 = the tail.
template <int BW, int S3>
__global__ __launch_bounds__(bcr_tail_waves(S3) * 64) void k_bcr_tail_and_reduce_rhs(PartView pv, int h0, int run_tail, int* __restrict__ fail, int ncols,
                                                                                    const double* __restrict__ Lb, const double* __restrict__ Z, int ny) {
  __shared__ double w[bcr_tail_waves(S3) * 3 * S3 * S3];
  if (blockIdx.x == 0) { if (run_tail) bcr_tail_body<S3>(pv, h0, fail, w); return; }
  const int idx = (int)blockIdx.x - 1, t = idx / ny, by = idx % ny;
  part_reduce_rhs<BW>(pv, ncols, Lb, Z, t, (int)(by * blockDim.x + threadIdx.x), (int)(ny * blockDim.x));
}

#ifndef MVUS_BCR_COLS
#define MVUS_BCR_COLS 1
#endif
constexpr int kBcrCols = MVUS_BCR_COLS;       // columns per workgroup (one: more workgroups, fewer items per level and thread)
template <int S3, int TC>
__global__ __launch_bounds__(256) void k_sep_bcr_rhs(PartView pv, int ncols) {
  double* __restrict__ Rr = pv.R;
  constexpr int SS = S3 * S3;
  extern __shared__ double bcr_lds[];
  const int m = pv.m, tid = threadIdx.x;
  double* rs = bcr_lds;                       // [m][S3][TC]
  double* xs = bcr_lds + (size_t)m * S3 * TC;
  const int col0 = blockIdx.x * TC;
  for (int e = tid; e < m * S3 * TC; e += 256) {
    const int c = e % TC, a = (e / TC) % S3, q = e / (TC * S3);
    rs[e] = col0 + c < ncols ? Rr[((long long)q * S3 + a) * ncols + col0 + c] : 0.0;
  }
  __syncthreads();
  int h = 1;
  for (; 2 * h <= m; h <<= 1) {
    const int ns = m / (2 * h);
    for (int e = tid; e < ns * S3 * TC; e += 256) {
      const int c = e % TC, a = (e / TC) % S3, i = 2 * h * (e / (TC * S3) + 1) - 1;
      double acc = rs[(i * S3 + a) * TC + c];
      const double* Hl = pv.Hc + (long long)(i - h) * SS + a;
      const double* rl = rs + (i - h) * S3 * TC + c;
#pragma unroll
      for (int k = 0; k < S3; ++k) acc -= Hl[k * S3] * rl[k * TC];
      if (i + h < m) {
        const double* Hr = pv.Ha + (long long)(i + h) * SS + a;
        const double* rr = rs + (i + h) * S3 * TC + c;
#pragma unroll
        for (int k = 0; k < S3; ++k) acc -= Hr[k * S3] * rr[k * TC];
      }
      rs[(i * S3 + a) * TC + c] = acc;
    }
    __syncthreads();
  }
  for (; h >= 1; h >>= 1) {
    const int ne = (m / h + 1) / 2;
    for (int e = tid; e < ne * S3 * TC; e += 256) {
      const int c = e % TC, a = (e / TC) % S3, j = h * (2 * (e / (TC * S3)) + 1) - 1;
      const double* Di = pv.U2 + (long long)j * SS + a * S3;
      const double* rj = rs + j * S3 * TC + c;
      double acc = 0.0;
#pragma unroll
      for (int k = 0; k < S3; ++k) acc += Di[k] * rj[k * TC];
      if (j - h >= 0) {
        const double* Hl = pv.Ha + (long long)j * SS + a * S3;
        const double* xl = xs + (j - h) * S3 * TC + c;
#pragma unroll
        for (int k = 0; k < S3; ++k) acc -= Hl[k] * xl[k * TC];
      }
      if (j + h < m) {
        const double* Hr = pv.Hc + (long long)j * SS + a * S3;
        const double* xr = xs + (j + h) * S3 * TC + c;
#pragma unroll
        for (int k = 0; k < S3; ++k) acc -= Hr[k] * xr[k * TC];
      }
      xs[(j * S3 + a) * TC + c] = acc;
    }
    __syncthreads();
  }
  for (int e = tid; e < m * S3 * TC; e += 256) {
    const int c = e % TC, a = (e / TC) % S3, q = e / (TC * S3);
    if (col0 + c < ncols) Rr[((long long)q * S3 + a) * ncols + col0 + c] = xs[e];
  }
}

// ---- time shards, round 6: TWO-LEVEL elimination of the separators ------------------------------------------------------------------
// Rank r's chain of separators is  [ghost G = the cut closing rank r-1]  s_1 .. s_k  [cut K closing rank r]  (global numbers q0-1, q0 ..
// q0+k-1, q0+k; no ghost on the first rank, no cut on the last).  k_part_reduce has left every block of it in the globally numbered
// [T | U | R]: T_q, U_q = T(q, q+1), the reduced right-hand sides R_q -- of G only the part interior 0 contributes, of K only the part
// the last interior contributes.  Rounds 3-5 summed the WHOLE system over the ranks (3.4 MB at configs[3]) and every rank solved all m
// separators.  Here the local separators L = {s_1 .. s_k} are a second-level interior:
//     L [Y | V | W] = [R_L | C_LG | C_LK]      the rank's own block-tridiagonal system, solved by the cyclic reduction as it is, on a
//                                               right-hand side with 2 s3 extra columns (C_LG = U_G^T in s_1's rows, C_LK = U_{s_k} in s_k's)
//     T'_G += T_G - U_G V_1      U'_G (= T'(G,K)) += -U_G W_1      R'_G += R_G - U_G Y_1            (subscript: the node's rows of Y, V, W)
//     T'_K += T_K - U_{s_k}^T W_k                                  R'_K += R_K - U_{s_k}^T Y_k
// the (world - 1)-node cut system [T' | U' | R'] is what the ranks sum (0.3 MB), every rank solves it (k_sep_factor, k_sep_rhs), and
//     X_L = Y - V X_G - W X_K
// goes into the globally numbered R beside X_G and X_K: k_back_correct, k_part_back and the Schur product's correction rows read it there
// as before.  The correction term of a cut separator splits by itself: rank r adds (its part of R_K)^T X_K, rank r+1 (its part)^T X_K.
template <int S3>
__global__ __launch_bounds__(256) void k_sep2_build(PartView pv, int q0, int k, int has_ghost, int has_cut, int ncols, double* __restrict__ Rloc,
                                                    double* __restrict__ CG, double* __restrict__ CK, int corr_q0 = 0, int corr_rows = 0, int CB = 0) {
  constexpr int SS = S3 * S3;
  const int nc2 = ncols + 2 * S3;
  const long long total = (long long)k * S3 * nc2;
  // (the correction rows of the Schur product need this rank's parts of the reduced right-hand sides R_S as they are BEFORE the solve
  // overwrites them: their camera columns go to pv.Dl here -- a rectangle copy of its own until round 6)
  for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < (long long)corr_rows * CB; e += (long long)gridDim.x * blockDim.x) {
    const long long r = (long long)corr_q0 * S3 + e / CB;
    pv.Dl[r * CB + e % CB] = pv.R[r * ncols + e % CB];
  }
  for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < total + 2 * SS; e += (long long)gridDim.x * blockDim.x) {
    if (e >= total) {                                   // the two coupling blocks, saved: the cyclic reduction overwrites U of its last node
      const int t = (int)(e - total), which = t / SS, idx = t % SS;
      if (which == 0) CG[idx] = has_ghost ? pv.U[(long long)(q0 - 1) * SS + idx] : 0.0;
      else CK[idx] = (has_cut && k > 0) ? pv.U[(long long)(q0 + k - 1) * SS + idx] : 0.0;
      continue;
    }
    const int col = (int)(e % nc2), a = (int)((e / nc2) % S3), j = (int)(e / ((long long)nc2 * S3));
    double v = 0.0;
    if (col < ncols) v = pv.R[((long long)(q0 + j) * S3 + a) * ncols + col];
    else if (col < ncols + S3) { if (j == 0 && has_ghost) v = pv.U[(long long)(q0 - 1) * SS + (col - ncols) * S3 + a]; }            // U_G^T
    else if (j == k - 1 && has_cut) v = pv.U[(long long)(q0 + k - 1) * SS + a * S3 + (col - ncols - S3)];                          // U_{s_k}
    Rloc[e] = v;
  }
}
// the rank's contribution to the cut system (cut node c closes rank c: G = node rank - 1, K = node rank); EVERY entry of
// cutbuf = [T' | U' | R'] is written -- zeros for the nodes of other ranks (a memset of its own until round 6)
template <int S3>
__global__ __launch_bounds__(256) void k_sep2_reduce(PartView pv, int q0, int k, int has_ghost, int has_cut, int rank, int ncut, int ncols,
                                                     const double* __restrict__ Rloc, const double* __restrict__ CG, const double* __restrict__ CK,
                                                     double* __restrict__ cutbuf) {
  constexpr int SS = S3 * S3;
  const int nc2 = ncols + 2 * S3;
  const long long nT = (long long)ncut * SS, total = 2 * nT + (long long)ncut * S3 * ncols;
  for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
    const int sec = e < nT ? 0 : (e < 2 * nT ? 1 : 2);                         // T', U', R'
    const long long w = e - (sec == 0 ? 0 : (sec == 1 ? nT : 2 * nT));
    const int node = (int)(w / (sec == 2 ? S3 * ncols : SS)), o = (int)(w % (sec == 2 ? S3 * ncols : SS));
    const int side = (has_ghost && node == rank - 1) ? 0 : ((has_cut && node == rank) ? 1 : -1);      // 0: the ghost G, 1: the cut K
    double v = 0.0;
    if (side >= 0) {
      const long long gq = side == 0 ? q0 - 1 : q0 + k;
      if (sec == 0) {                                   // T'
        const int a = o / S3, b = o % S3;
        v = pv.T[gq * SS + o];
        if (k > 0) {
          if (side == 0) { for (int c = 0; c < S3; ++c) v -= CG[a * S3 + c] * Rloc[((long long)(0) * S3 + c) * nc2 + ncols + b]; }                   // U_G V_1
          else { for (int c = 0; c < S3; ++c) v -= CK[c * S3 + a] * Rloc[((long long)(k - 1) * S3 + c) * nc2 + ncols + S3 + b]; }                    // U_{s_k}^T W_k
        }
      } else if (sec == 1) {                            // U' = T'(G, K): through the local chain, or -- no local separator -- the direct coupling
        if (side == 0 && has_cut) {
          const int a = o / S3, b = o % S3;
          if (k > 0) { for (int c = 0; c < S3; ++c) v -= CG[a * S3 + c] * Rloc[((long long)(0) * S3 + c) * nc2 + ncols + S3 + b]; }                  // -U_G W_1
          else v = pv.U[gq * SS + o];
        }
      } else {                                          // R'
        const int a = o / ncols, col = o % ncols;
        v = pv.R[(gq * S3 + a) * ncols + col];
        if (k > 0) {
          if (side == 0) { for (int c = 0; c < S3; ++c) v -= CG[a * S3 + c] * Rloc[((long long)(0) * S3 + c) * nc2 + col]; }
          else { for (int c = 0; c < S3; ++c) v -= CK[c * S3 + a] * Rloc[((long long)(k - 1) * S3 + c) * nc2 + col]; }
        }
      }
    }
    cutbuf[e] = v;
  }
}
// X_L = Y - V X_G - W X_K and the two cut solutions, into the globally numbered R
template <int S3>
__global__ __launch_bounds__(256) void k_sep2_finish(PartView pv, int q0, int k, int has_ghost, int has_cut, int rank, int ncut, int ncols,
                                                     const double* __restrict__ Rloc, const double* __restrict__ cutbuf) {
  constexpr int SS = S3 * S3;
  const int nc2 = ncols + 2 * S3;
  const double* X2 = cutbuf + 2LL * ncut * SS;          // the solved cut system
  const long long total = (long long)(k + 2) * S3 * ncols;
  for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
    const int col = (int)(e % ncols), a = (int)((e / ncols) % S3), j = (int)(e / ((long long)ncols * S3));
    if (j >= k) {                                       // j = k: X_G, j = k + 1: X_K
      const bool g = j == k;
      if (g ? !has_ghost : !has_cut) continue;
      const int node = g ? rank - 1 : rank;
      const long long gq = g ? q0 - 1 : q0 + k;
      pv.R[(gq * S3 + a) * ncols + col] = X2[((long long)node * S3 + a) * ncols + col];
      continue;
    }
    const double* row = Rloc + ((long long)j * S3 + a) * nc2;
    double v = row[col];
    if (has_ghost) for (int b = 0; b < S3; ++b) v -= row[ncols + b] * X2[((long long)(rank - 1) * S3 + b) * ncols + col];
    if (has_cut) for (int b = 0; b < S3; ++b) v -= row[ncols + S3 + b] * X2[((long long)rank * S3 + b) * ncols + col];
    pv.R[((long long)(q0 + j) * S3 + a) * ncols + col] = v;
  }
}

}  // namespace mvus
