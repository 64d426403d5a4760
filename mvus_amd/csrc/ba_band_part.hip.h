// Partitioned band solver, the interiors' side (PartView and the scheme: ba_ne_views.h): factorisation and solves of the interiors,
// the reduction onto the separators, the back-correction, and the launches that build the right-hand sides and pack the band.
// The separator system itself is ba_sep.hip.h.
#pragma once
#include <hip/hip_runtime.h>

#include "ba_band_generic.hip.h"      // band_pack_entry
#include "ba_dev_problem.h"
#include "ba_ne_views.h"
#include "ba_partition.h"
#include "ba_wave.hip.h"

namespace mvus {

// original (damped) matrix entry H(i, c) read from the lower band; valid for separator rows/columns and for
// interior-separator couplings, which the interior factorisation never overwrites
template <int BW>
__device__ __forceinline__ double band_entry(const double* __restrict__ Lb, int i, int c) {
  const int hi = i > c ? i : c, d = i > c ? i - c : c - i;
  return d <= BW ? Lb[(long long)hi * (BW + 1) + d] : 0.0;
}
// the same without a conditional load (the row is always inside the band array): for the unconditioned batches of part_solve_block
template <int BW>
__device__ __forceinline__ double band_entry_nc(const double* __restrict__ Lb, int i, int c) {
  const int hi = i > c ? i : c, d = i > c ? i - c : c - i;
  const double v = Lb[(long long)hi * (BW + 1) + (d <= BW ? d : BW)];
  return d <= BW ? v : 0.0;
}

// banded Cholesky of interior p by ONE wavefront (lane = threadIdx.x & 63); T: (kPartRowsMax + 1) * (BW + 1) doubles of LDS private to it.
// (Only this wavefront touches T: the synchronisation is the wavefront-level one.)
__device__ __forceinline__ void part_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront", "local");
}
template <int BW>
__device__ __forceinline__ void part_cholesky_body(const PartView& pv, double* __restrict__ Lb, int* __restrict__ fail, double* __restrict__ T, int p, int lane) {
  constexpr int R = BW + 1;
  const int r0 = pv.i0[p], n = pv.i1[p] - r0;
  for (int e0 = lane; e0 < n * R; e0 += 64 * 8) {          // eight loads in flight per lane
    double v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = Lb[(long long)r0 * R + min(e0 + 64 * u, n * R - 1)];
#pragma unroll
    for (int u = 0; u < 8; ++u) if (e0 + 64 * u < n * R) T[e0 + 64 * u] = v[u];
  }
  // trailing-update pairs (rr >= ss >= 1) owned by this lane, as offsets from the pivot row: fixed for all columns
  constexpr int kPairs = BW * (BW + 1) / 2, kSlots = (kPairs + 63) / 64;
  int prr[kSlots], offA[kSlots], offB[kSlots], offC[kSlots];
#pragma unroll
  for (int sl = 0; sl < kSlots; ++sl) {
    const int e = lane + 64 * sl;
    int r = 0;
    while ((r + 1) * (r + 2) / 2 <= e) ++r;
    const int rr = r + 1, ss = e - r * (r + 1) / 2 + 1;
    prr[sl] = e < kPairs ? rr : BW + 1;
    offA[sl] = rr * R + (rr - ss); offB[sl] = rr * R + rr; offC[sl] = ss * R + ss;
  }
  part_lds_sync();
  // One LDS round trip per column (round 4; it was four: pivot, scaled column, its read-back, trailing update).  The trailing
  // update reads the UNSCALED column, A(k+r, k+s) -= T_r T_s / piv, so it does not wait for the scaled column; the next pivot is
  // the updated (1, 1) entry, which lane 0 holds in a register (pair 0) -- a v_readlane instead of an LDS read, and its
  // reciprocal square root runs under the latency of the next column's reads.
  // The loop body has no branch: a lane without work in a column reads the pivot's slot and writes to a spare slot behind the
  // matrix (T holds one more row than the interior can have), so the reads carry no exec-mask joins for s_waitcnt to stop at.
  constexpr int kSpare = kPartRowsMax * R;
  bool bad = false;
  double piv = T[0];
  for (int k = 0; k < n; ++k) {
    const int nb = min(BW, n - 1 - k);
    const int base = k * R;
    double a[kSlots], b[kSlots], c[kSlots];
    bool on[kSlots];
#pragma unroll
    for (int sl = 0; sl < kSlots; ++sl) {
      on[sl] = prr[sl] <= nb;
      a[sl] = T[base + (on[sl] ? offA[sl] : 0)]; b[sl] = T[base + (on[sl] ? offB[sl] : 0)]; c[sl] = T[base + (on[sl] ? offC[sl] : 0)];
    }
    const bool incol = lane >= 1 && lane <= nb;
    const int icol = incol ? lane * R + lane : 0;
    const double colv = T[base + icol];
    bad |= !(piv > 0.0);
    piv = piv > 0.0 ? piv : 1.0;
    double inv = __builtin_amdgcn_rsq(piv);              // two Newton steps on v_rsq_f64
    inv = inv * (1.5 - 0.5 * piv * inv * inv);
    inv = inv * (1.5 - 0.5 * piv * inv * inv);
    const double invp = inv * inv;
    double first = 0.0;
#pragma unroll
    for (int sl = 0; sl < kSlots; ++sl) {
      const double v = a[sl] - (b[sl] * invp) * c[sl];
      T[on[sl] ? base + offA[sl] : kSpare] = v;
      if (sl == 0) first = v;
    }
    T[incol ? base + icol : kSpare + 1] = colv * inv;     // the column of L (every read of it above precedes this store in program order)
    T[lane == 0 ? base : kSpare + 2] = inv;               // reciprocal of L(k,k)
    piv = bcast_lane(first, 0);                           // A(k+1, k+1) after this column's update (pair 0 = (1, 1)); unused when nb = 0
    part_lds_sync();
  }
  if (bad && lane == 0) fail[0] = 1;
  // write back only entries whose column lies inside the interior (j <= row - r0); couplings stay original
  for (int e = lane; e < n * R; e += 64) {
    const int row = e / R, j = e % R;
    if (j <= row) Lb[(long long)r0 * R + e] = T[e];
  }
}
template <int BW>
__global__ __launch_bounds__(64) void k_part_cholesky(PartView pv, double* __restrict__ Lb, int* __restrict__ fail) {
  __shared__ double T[(kPartRowsMax + 1) * (BW + 1)];
  part_cholesky_body<BW>(pv, Lb, fail, T, (int)blockIdx.x, (int)threadIdx.x);
}

// interior solves, one thread per column, one wavefront per (interior, 64 columns).  COUPLING = false: right-hand-side
// columns of Z, in place.  COUPLING = true (one extra wavefront per interior): the 2*s3 coupling columns
// V_p = B_p^-1 H[I_p, S_{p-1}], W_p = B_p^-1 H[I_p, S_p] -> pv.VW.
// A lone wavefront per SIMD issues in order, so the kernel is bound by its instruction count: the factor is staged in
// LDS once (entries reaching outside the interior zeroed, rows padded to whole batches with identity rows: the
// substitution loops are branch free) and read as broadcasts, rows are addressed by pointer increments, and the rows of
// the right-hand side are fetched one batch of kPf rows ahead (they are ncols*8 bytes apart: every row is a fresh
// cache line, ~1-2 us away).
#ifndef MVUS_PS_PF
#define MVUS_PS_PF 16
#endif
constexpr int kPsPf = MVUS_PS_PF;       // rows of right-hand side in flight per lane (a batch)
template <int BW, bool COUPLING>
__device__ __forceinline__ void part_solve_block(const PartView& pv, int ncols, const double* __restrict__ Lb, double* __restrict__ Z, double* Ls, int p, int by) {
  constexpr int R = BW + 1, kPf = kPsPf;
  const int tid = threadIdx.x;
  const int s3 = pv.s3;
  const int r0 = pv.i0[p], nr = pv.i1[p] - r0;
  const int nrp = (nr + kPf - 1) / kPf * kPf;                // rows padded to whole batches
  // (eight loads in flight per lane, none behind a condition: rows past the interior repeat its last row and are replaced afterwards)
  constexpr int kStage = 8;
  const int total = (nrp + kPf) * R;
  for (int e0 = tid; e0 < total; e0 += 64 * kStage) {
    double v[kStage];
#pragma unroll
    for (int u = 0; u < kStage; ++u) {
      const int e = min(e0 + 64 * u, total - 1), row = e / R, jj = e - row * R;
      v[u] = Lb[(long long)(r0 + min(row, nr - 1)) * R + jj];
    }
#pragma unroll
    for (int u = 0; u < kStage; ++u) {
      const int e = e0 + 64 * u, row = e / R, jj = e - row * R;
      if (e < total) Ls[e] = row < nr ? ((jj <= row) ? v[u] : 0.0) : (jj == 0 ? 1.0 : 0.0);   // column row-jj inside the interior
    }
  }
  __syncthreads();
  int ccol = 0;
  bool live;
  if (COUPLING) {
    live = tid < 2 * s3 && (tid < s3 ? pv.sl[p] >= 0 : pv.sr[p] >= 0);
    if (live) ccol = tid < s3 ? pv.sl[p] + tid : pv.sr[p] + (tid - s3);
  } else {
    live = (int)(by * 64 + tid) < ncols;
  }
  if (!live) return;                                         // no barrier below
  double* out = COUPLING ? pv.VW + ((long long)p * kPartRowsMax) * (2 * s3) + tid : Z + (long long)r0 * ncols + by * 64 + tid;
  const long long ostride = COUPLING ? 2 * s3 : ncols;
  // where the forward pass reads its right-hand side: the column's rows of Z (written by the right-hand-side copy), or -- pv.direct, one rank,
  // many columns -- the assembled blocks themselves: column (c, k) of the camera-major cross block, the spline gradient for the last
  // column.  The copy (a pass over all of E and Z) is then not launched at all.
  const double* src = out;
  long long sstride = ostride;
  if (!COUPLING && pv.direct) {
    const int col = min((int)(by * 64 + tid), ncols - 1);
    if (col < pv.CB) { src = pv.Et + ((long long)(col / pv.B) * pv.N3 + r0) * pv.B + col % pv.B; sstride = pv.B; }
    else { src = pv.gs + r0; sstride = 1; }
  }
  // Batches of kPf rows.  A FULL batch (all its rows inside the interior) is loaded, solved and stored without a single condition:
  // with a condition per row (`i < nr ? load : 0`) every load and store sat in its own scalar branch and the compiler closed each
  // batch of prefetches with s_waitcnt vmcnt(0) -- the wavefront then waited out the memory latency once per batch in both passes
  // (round 4: 45 -> see DESIGN section 5).  Only the last, partial batch keeps the conditions.
  using Full = std::true_type;
  using Part = std::false_type;
  auto load_rhs = [&](auto full, double (&dst)[kPf], int ib) {
#pragma unroll
    for (int k = 0; k < kPf; ++k) {
      const int i = ib + k;
      if constexpr (decltype(full)::value) dst[k] = COUPLING ? band_entry_nc<BW>(Lb, r0 + i, ccol) : src[(long long)i * sstride];
      else dst[k] = i < nr ? (COUPLING ? band_entry<BW>(Lb, r0 + i, ccol) : src[(long long)i * sstride]) : 0.0;
    }
  };
  auto load_y = [&](auto full, double (&dst)[kPf], int ib) {
#pragma unroll
    for (int k = 0; k < kPf; ++k) {
      const int i = ib + k;
      if constexpr (decltype(full)::value) dst[k] = out[(long long)i * ostride];
      else dst[k] = i < nr ? out[(long long)i * ostride] : 0.0;
    }
  };
  auto take = [&](double (&dst)[kPf], const double (&src)[kPf]) {
#pragma unroll
    for (int k = 0; k < kPf; ++k) dst[k] = src[k];
  };
  double yw[BW];           // yw[0] = newest value
  // forward: y(i) = (b(i) - sum_j L(i, i-j) y(i-j)) / L(i,i)
  auto forward = [&](auto full, const double (&cur)[kPf], int ib) {
    const double* Lr = Ls + ib * R;
    double* yo = out + (long long)ib * ostride;
#pragma unroll
    for (int k = 0; k < kPf; ++k) {
      // only the j = 1 term depends on the previous row's result: summing from the far end of the band leaves a
      // two-operation dependent chain per row
      double acc = cur[k];
#pragma unroll
      for (int j = BW; j >= 1; --j) acc -= Lr[k * R + j] * yw[j - 1];
      const double y = acc * Lr[k * R];
      if constexpr (decltype(full)::value) yo[(long long)k * ostride] = y;
      else if (ib + k < nr) yo[(long long)k * ostride] = y;
#pragma unroll
      for (int j = BW - 1; j >= 1; --j) yw[j] = yw[j - 1];
      yw[0] = y;
    }
  };
  // backward: x(i) = (y(i) - sum_j L(i+j, i) x(i+j)) / L(i,i); the padded rows give x = 0
  auto backward = [&](auto full, const double (&cur)[kPf], int ib) {
#pragma unroll
    for (int k = kPf - 1; k >= 0; --k) {
      const int i = ib + k;
      double acc = cur[k];
#pragma unroll
      for (int j = BW; j >= 1; --j) acc -= Ls[(i + j) * R + j] * yw[j - 1];     // rows up to nrp + BW - 1 are staged
      const double xv = acc * Ls[i * R];
      if constexpr (decltype(full)::value) out[(long long)i * ostride] = xv;
      else if (i < nr) out[(long long)i * ostride] = xv;
#pragma unroll
      for (int j = BW - 1; j >= 1; --j) yw[j] = yw[j - 1];
      yw[0] = xv;
    }
  };
  const int nfull = nr / kPf, tail0 = nfull * kPf;
  const bool has_tail = tail0 < nr;
  double cur[kPf], nxt[kPf];
#pragma unroll
  for (int j = 0; j < BW; ++j) yw[j] = 0.0;
  if (nfull > 0) {
    load_rhs(Full{}, nxt, 0);
    for (int bt = 0; bt + 1 < nfull; ++bt) {               // the rows of the next batch are fetched while this one is solved
      take(cur, nxt);
      load_rhs(Full{}, nxt, (bt + 1) * kPf);
      forward(Full{}, cur, bt * kPf);
    }
    take(cur, nxt);
    if (has_tail) load_rhs(Part{}, nxt, tail0);
    forward(Full{}, cur, tail0 - kPf);
  } else if (has_tail) {
    load_rhs(Part{}, nxt, 0);
  }
  if (has_tail) { take(cur, nxt); forward(Part{}, cur, tail0); }
#pragma unroll
  for (int j = 0; j < BW; ++j) yw[j] = 0.0;
  if (has_tail) {
    load_y(Part{}, cur, tail0);
    if (nfull > 0) load_y(Full{}, nxt, tail0 - kPf);
    backward(Part{}, cur, tail0);
  } else if (nfull > 0) {
    load_y(Full{}, nxt, tail0 - kPf);
  }
  for (int bt = nfull - 1; bt >= 1; --bt) {
    take(cur, nxt);
    load_y(Full{}, nxt, (bt - 1) * kPf);
    backward(Full{}, cur, bt * kPf);
  }
  if (nfull > 0) { take(cur, nxt); backward(Full{}, cur, 0); }
}

// column blocks 0 .. gy-2: 64 right-hand-side columns each; the last one: the coupling columns (same launch, so that they run
// beside the others instead of after them)
template <int BW>
__global__ __launch_bounds__(64) void k_part_solve(PartView pv, int ncols, const double* __restrict__ Lb, double* __restrict__ Z, int gy) {
  __shared__ double Ls[(kPartRowsMax + 2 * kPsPf) * (BW + 1)];
  // 1-D grid: the gy column blocks of one interior are consecutive tiles, runs of tiles per XCD (xcd_tile): 48.9 -> 46.6 us
  const int tiles = pv.P * gy;
  const int tile = xcd_tile(tiles);
  if (tile >= tiles) return;
  const int p = tile / gy, by = tile % gy;
  if (by + 1 == gy) part_solve_block<BW, true>(pv, ncols, Lb, Z, Ls, p, by);
  else part_solve_block<BW, false>(pv, ncols, Lb, Z, Ls, p, by);
}

// separator system: T(q,q), T(q,q+1) and the reduced right-hand sides (in place in the separator rows of Z)
// right-hand sides of separator task t: entries e0, e0 + estride, ... of its s3 x ncols block
template <int BW>
__device__ __forceinline__ void part_reduce_rhs(const PartView& pv, int ncols, const double* __restrict__ Lb, const double* __restrict__ Z, int t, int e0, int estride) {
  const int s3 = pv.s3;
  const int c0 = pv.tc0[t], pl = pv.tpl[t], pr = pv.tpr[t], gq = pv.tgq[t];
  const bool own = pv.town[t] != 0;
  const int a0 = pl >= 0 ? pv.i0[pl] : 0, a1 = pl >= 0 ? pv.i1[pl] : 0;
  const int b0 = pr >= 0 ? pv.i0[pr] : 0, b1 = pr >= 0 ? pv.i1[pr] : 0;
  for (int e = e0; e < s3 * ncols; e += estride) {
    const int a = e / ncols, col = e % ncols;
    double r = 0.0;
    if (own) {
      if (pv.Dl == nullptr) r = Z[(long long)(c0 + a) * ncols + col];
      else r = col < pv.CB ? pv.Et[((long long)(col / pv.B) * pv.N3 + (c0 + a)) * pv.B + col % pv.B] : pv.gs[c0 + a];    // (its rows of Z hold zeros)
    }
    if (pl >= 0) {                                       // (clamped rows, dropped products: every load unconditional, as in k_part_reduce)
      double f[BW], z[BW];
#pragma unroll
      for (int jj = 0; jj < BW; ++jj) {
        const int ic = max(a1 - BW + jj, a0);
        f[jj] = band_entry_nc<BW>(Lb, ic, c0 + a);
        z[jj] = Z[(long long)ic * ncols + col];
      }
#pragma unroll
      for (int jj = 0; jj < BW; ++jj) r -= (a1 - BW + jj >= a0) ? f[jj] * z[jj] : 0.0;
    }
    if (pr >= 0) {
      double f[BW], z[BW];
#pragma unroll
      for (int jj = 0; jj < BW; ++jj) {
        const int ic = min(b0 + jj, b1 - 1);
        f[jj] = band_entry_nc<BW>(Lb, ic, c0 + a);
        z[jj] = Z[(long long)ic * ncols + col];
      }
#pragma unroll
      for (int jj = 0; jj < BW; ++jj) r -= (b0 + jj < b1) ? f[jj] * z[jj] : 0.0;
    }
    pv.R[((long long)gq * s3 + a) * ncols + col] = r;
    if (pv.Dl != nullptr && col < pv.CB) pv.Dl[((long long)gq * s3 + a) * pv.CB + col] = r;
  }
}
// what: 1 = the matrix blocks T, U (workgroups with blockIdx.y == 0), 2 = the right-hand sides, 3 = both
template <int BW>
__global__ __launch_bounds__(256) void k_part_reduce(PartView pv, int ncols, const double* __restrict__ Lb, const double* __restrict__ Z, int what = 3) {
  const int t = blockIdx.x, s3 = pv.s3, st = 2 * s3;
  const int c0 = pv.tc0[t], pl = pv.tpl[t], pr = pv.tpr[t], gq = pv.tgq[t];
  const bool own = pv.town[t] != 0;
  const int a0 = pl >= 0 ? pv.i0[pl] : 0, a1 = pl >= 0 ? pv.i1[pl] : 0;     // interior before the separator
  const int b0 = pr >= 0 ? pv.i0[pr] : 0, b1 = pr >= 0 ? pv.i1[pr] : 0;     // interior after it
  // only the last BW rows of the interior before and the first BW rows of the one after couple to the separator; the
  // loops run over exactly BW rows with the out-of-range ones masked, so that all their loads are issued together
  const double* VWa = pv.VW + ((long long)(pl >= 0 ? pl : 0) * kPartRowsMax) * st;
  const double* VWb = pv.VW + ((long long)(pr >= 0 ? pr : 0) * kPartRowsMax) * st;
  for (int e = threadIdx.x; (what & 1) && blockIdx.y == 0 && e < s3 * s3; e += blockDim.x) {
    const int a = e / s3, b = e % s3;
    // (rows outside the interior are clamped to its edge and their products dropped: no load sits behind a condition, all 2 x BW
    // x 2 - 3 of them are in flight together -- with a branch per row this loop was a chain of ~30 memory round trips, 12 us)
    double tt = own ? band_entry<BW>(Lb, c0 + a, c0 + b) : 0.0, u = 0.0;
    if (pl >= 0) {
      double f[BW], w[BW];
#pragma unroll
      for (int jj = 0; jj < BW; ++jj) {
        const int ic = max(a1 - BW + jj, a0);
        f[jj] = band_entry_nc<BW>(Lb, ic, c0 + a);
        w[jj] = VWa[(long long)(ic - a0) * st + s3 + b];
      }
#pragma unroll
      for (int jj = 0; jj < BW; ++jj) tt -= (a1 - BW + jj >= a0) ? f[jj] * w[jj] : 0.0;                             // F_right(q)^T W_q
    }
    if (pr >= 0) {
      double f[BW], wv[BW], ww[BW];
#pragma unroll
      for (int jj = 0; jj < BW; ++jj) {
        const int ic = min(b0 + jj, b1 - 1);
        f[jj] = band_entry_nc<BW>(Lb, ic, c0 + a);
        wv[jj] = VWb[(long long)(ic - b0) * st + b];
        ww[jj] = VWb[(long long)(ic - b0) * st + s3 + b];
      }
#pragma unroll
      for (int jj = 0; jj < BW; ++jj) {
        const bool in = b0 + jj < b1;
        tt -= in ? f[jj] * wv[jj] : 0.0;                                                                             // F_left(q+1)^T V_{q+1}
        u -= in ? f[jj] * ww[jj] : 0.0;                                                                              // F_left(q+1)^T W_{q+1}
      }
    }
    pv.T[((long long)gq * s3 + a) * s3 + b] = tt;
    pv.U[((long long)gq * s3 + a) * s3 + b] = (gq + 1 < pv.m) ? u : 0.0;
  }
  // the right-hand sides: gridDim.y workgroups per separator share the entries (few dependent load rounds each)
  if (what & 2) part_reduce_rhs<BW>(pv, ncols, Lb, Z, t, (int)(blockIdx.y * blockDim.x + threadIdx.x), (int)(gridDim.y * blockDim.x));
}

// interiors: X = Y - V X_{S_{p-1}} - W X_{S_p}.  One thread per right-hand-side column: the 2*S3 separator values of
// its column stay in registers, the rows of V|W are the same for every lane (scalar loads), so each interior entry
// costs one coalesced load, 2*S3 FMAs and one store.
#ifndef MVUS_BACK_ROWS
#define MVUS_BACK_ROWS 16
#endif
constexpr int kBackRows = MVUS_BACK_ROWS;      // rows per workgroup: enough workgroups in flight to hide the load latency
template <int S3>
__global__ __launch_bounds__(64) void k_part_back(PartView pv, int ncols, double* __restrict__ Z, int gy, int gz) {
  // 1-D grid, tiles ordered column block fastest, then row block, then interior, handed to the XCDs in runs (xcd_tile):
  // one XCD reads and writes whole consecutive rows of Z (22.1 -> 20.3 us)
  const int tiles = pv.P * gy * gz;
  const int tile = xcd_tile(tiles);
  if (tile >= tiles) return;
  const int by = tile % gy, bz = (tile / gy) % gz, p = tile / (gy * gz);
  const int col = by * 64 + threadIdx.x;
  if (col >= ncols) return;
  constexpr int st = 2 * S3;
  const int r0 = pv.i0[p], n = pv.i1[p] - r0;
  const int ia = bz * kBackRows, ib = min(n, ia + kBackRows);      // rows of this workgroup
  if (ia >= n) return;
  const bool left = pv.sl[p] >= 0, right = pv.sr[p] >= 0;
  const double* __restrict__ VWp = pv.VW + ((long long)p * kPartRowsMax) * st;
  double zl[S3], zr[S3];
#pragma unroll
  for (int a = 0; a < S3; ++a) {
    zl[a] = left ? pv.R[((long long)(pv.q_off + p - 1) * S3 + a) * ncols + col] : 0.0;
    zr[a] = right ? pv.R[((long long)(pv.q_off + p) * S3 + a) * ncols + col] : 0.0;
  }
  if (right && bz == 0) {          // the solved separator right of this interior goes back into its rows of Z
#pragma unroll
    for (int a = 0; a < S3; ++a) Z[(long long)(pv.sr[p] + a) * ncols + col] = zr[a];
  }
  for (int i = ia; i < ib; ++i) {
    double v = Z[(long long)(r0 + i) * ncols + col];
    const double* __restrict__ vw = VWp + (long long)i * st;
    if (left) {
#pragma unroll
      for (int a = 0; a < S3; ++a) v -= vw[a] * zl[a];
    }
    if (right) {
#pragma unroll
      for (int a = 0; a < S3; ++a) v -= vw[S3 + a] * zr[a];
    }
    Z[(long long)(r0 + i) * ncols + col] = v;
  }
}

// Z[3N][ncols] = [E^T | gs]: the row-major copy of the camera-major cross block that the interior solves work on.  (Until round 5 a
// second copy, Erm[3N][CB], was written here as the Schur product's first operand: the product now reads the camera-major block
// itself -- 34 MB less written at configs[2], 138 MB at configs[3]: k_cholesky_and_rhs 69 -> 55 us there.)
// The same launch also packs the damped band (band_pack_entry: the two are independent element-wise passes over the assembled
// blocks, and every launch costs ~4.7 us before it does anything).
__global__ void k_build_rhs(NEView ne, int ncols, double* __restrict__ Z, const unsigned char* __restrict__ seprow, double lambda, int BW, double* __restrict__ Lb,
                            int* __restrict__ fail, DevProblem dp, int with_diag, double* __restrict__ D, double* __restrict__ gx, int tiles) {
  const long long idx = xcd_tile(tiles) * (long long)blockDim.x + threadIdx.x;      // XCD-aware order: 31.5 -> 25 us (see xcd_tile)
  band_pack_entry(ne, lambda, BW, Lb, fail, dp, with_diag, D, gx, idx);
  if (idx >= (long long)ne.N3 * ncols) return;
  const int r = (int)(idx / ncols), cidx = (int)(idx % ncols);
  if (seprow != nullptr && seprow[r]) Z[idx] = 0.0;            // (one rank: the separators' rows take no part in the product's main range)
  else if (cidx < ne.CB) {
    const int c = cidx / ne.B, k = cidx % ne.B;
    Z[idx] = ne.Et[((long long)c * ne.N3 + r) * ne.B + k];
  } else {
    Z[idx] = ne.gs[r];
  }
}

// The same work as two launches that OVERLAP: k_band_pack (the damped band, 0.2 M entries) first, then ONE launch whose first
// pad8(P) workgroups factorise the interiors (a lone wavefront each, ~37 us of dependent LDS round trips on 155 of 256 CUs)
// while all the others stream the right-hand-side copies (72 MB, bandwidth bound, ~22 us) -- the factorisation needs the
// band only, the copies need nothing from the factorisation.  25 + 37 us in sequence become ~40.
__global__ void k_band_pack(NEView ne, double lambda, int BW, double* __restrict__ Lb, int* __restrict__ fail, DevProblem dp, int with_diag,
                            double* __restrict__ D, double* __restrict__ gx) {
  band_pack_entry(ne, lambda, BW, Lb, fail, dp, with_diag, D, gx, blockIdx.x * (long long)blockDim.x + threadIdx.x);
}
template <int BW>
__global__ __launch_bounds__(256) void k_cholesky_and_rhs(PartView pv, double* __restrict__ Lb, int* __restrict__ fail, int chol_blocks,
                                                          NEView ne, int ncols, double* __restrict__ Z, int tiles, const unsigned char* __restrict__ seprow) {
  __shared__ double T[(kPartRowsMax + 1) * (BW + 1)];
  if ((int)blockIdx.x < chol_blocks) {                    // chol_blocks is a multiple of 8: the copy tiles keep their XCD mapping
    if ((int)blockIdx.x < pv.P && threadIdx.x < 64) part_cholesky_body<BW>(pv, Lb, fail, T, (int)blockIdx.x, (int)threadIdx.x);
    return;
  }
  const int b = (int)blockIdx.x - chol_blocks;
  const int run = xcd_run_for(tiles);
  const int xcd = b & 7, qq = b >> 3;
  const long long idx = (long long)(((qq / run) * 8 + xcd) * run + qq % run) * blockDim.x + threadIdx.x;     // xcd_tile for the shifted index
  if (idx >= (long long)ne.N3 * ncols) return;
  const int r = (int)(idx / ncols), cidx = (int)(idx % ncols);
  if (seprow != nullptr && seprow[r]) Z[idx] = 0.0;            // (one rank: the separators' rows take no part in the product's main range)
  else if (cidx < ne.CB) {
    const int c = cidx / ne.B, k = cidx % ne.B;
    Z[idx] = ne.Et[((long long)c * ne.N3 + r) * ne.B + k];        // (the product's first operand is read where the assembly left it)
  } else {
    Z[idx] = ne.gs[r];
  }
}

}  // namespace mvus
