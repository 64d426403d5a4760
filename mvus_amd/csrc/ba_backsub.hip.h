// Back-substitution: the step in x order from the camera step and the solved spline rows, and the correction of the interiors'
// columns that the one-rank route leaves to the end.
#pragma once
#include <hip/hip_runtime.h>

#include "ba_dev_problem.h"
#include "ba_ne_views.h"
#include "ba_partition.h"
#include "ba_wave.hip.h"

namespace mvus {

// p (x order) from p_c and p_s = -(z_g + Z_E p_c)
__global__ __launch_bounds__(kThreads) void k_back_substitute(DevProblem dp, NEView ne, int ncols, int row_lo, int row_hi, int cams,
                                                              const double* __restrict__ Z, const double* __restrict__ pc, double* __restrict__ px,
                                                              int* __restrict__ fail = nullptr, int* __restrict__ fail_mirror = nullptr,
                                                              double* __restrict__ fail_tail = nullptr) {
  // one wavefront per owned spline row: lanes stride over the row of Z (coalesced), then a shuffle reduction
  const int lane = threadIdx.x & 63;
  // last kernel of a solve: the two failure flags go to the host's mapped copy here (a device-to-host copy of 8 bytes is a launch)
  // (a hand-over time-out inside the solve -- fail[2], raised by a workgroup that gave up waiting for another one of its launch: k_rcs_factor's
  // rows, k_sep_bcr_levels -- outranks whatever a later kernel made of the unfinished data: it is reported as its own code, HipSchur::retry_same)
  if (fail != nullptr && blockIdx.x == 0 && threadIdx.x < 2) {
    int v = fail[threadIdx.x];
    if (threadIdx.x == 0 && fail[2] != 0) { v = kFailHandoverCode; fail[0] = v; }
    if (fail_mirror != nullptr) fail_mirror[threadIdx.x] = v;
    // time shards: the flags travel with the step through its sum over the ranks (fail_tail = px + n; decoded by fail_sum_code / fail_sum_flag)
    if (fail_tail != nullptr) fail_tail[threadIdx.x] = threadIdx.x == 0 ? (v == kFailHandoverCode ? kFailHandoverSum : (double)v)
                                                                        : (double)(v & 1) + ((v & 2) ? kFailSpanSum : 0.0);
  }
  const int r = row_lo + blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
  if (blockIdx.x == 0 && cams)
    for (int idx = threadIdx.x; idx < ne.CB; idx += kThreads) px[cam_col(dp.C, dp.P, idx / ne.B, idx % ne.B)] = pc[idx];
  if (r >= row_hi) return;
  const double* zr = Z + (long long)r * ncols;
  double acc = 0.0;
  for (int k = lane; k < ne.CB; k += 64) acc += zr[k] * pc[k];
  acc = wave_sum(acc);
  if (lane == 0) {
    const int g = r / 3 + ne.row0, d = r % 3;
    px[dp.mv.ctrl_x0[g] + d * dp.mv.ctrl_stride[g]] = -(acc + zr[ne.CB]);
  }
}

// One rank, round 5: the step's spline rows when the interiors' columns of Z were NOT corrected for the separators (k_part_back: a
// read-modify-write of all of Z) and the separators' rows of Z hold zeros.  k_back_substitute has written -(Z_i p_c + z_g,i) for the
// interiors' rows (and zeros for the separators'); one workgroup per interior finishes them:
//   s = X_S p_c + x_S,g  for the separators either side (rows of pv.R: 2 s3 dot products),
//   p_i += sum_a VW[i][a] s[a]  for its rows,   p_S = -s  for the separator after it.
template <int S3>
__global__ __launch_bounds__(256) void k_back_correct(DevProblem dp, NEView ne, PartView pv, int ncols, const double* __restrict__ pc, double* __restrict__ px) {
  const int p = blockIdx.x, i = threadIdx.x;
  constexpr int st = 2 * S3;
  const int r0 = pv.i0[p], nr = pv.i1[p] - r0;
  const int sl = pv.sl[p], sr = pv.sr[p];
  constexpr int nch = 256 / st;                               // threads per separator value: thread (a, ch) takes columns ch, ch + nch, ...
  __shared__ double part[st][nch];
  __shared__ double sx[st];
  // (everything the row needs at the end -- its coupling entries, its place in x, the value k_back_substitute left there -- is requested
  // before the dot products: the kernel is a chain of memory round trips)
  double vwv[st];
  const int ic = min(i, max(nr - 1, 0));
  {
    const double* __restrict__ vw = pv.VW + ((long long)p * kPartRowsMax + ic) * st;
#pragma unroll
    for (int a = 0; a < st; ++a) vwv[a] = vw[a];
  }
  const int rrow = r0 + ic, grow = rrow / 3 + ne.row0;
  const int xrow = dp.mv.ctrl_x0[grow] + (rrow % 3) * dp.mv.ctrl_stride[grow];
  const double pold = px[xrow];
  int xsep = 0;
  if (sr >= 0 && i < S3) { const int r = sr + i, g = r / 3 + ne.row0; xsep = dp.mv.ctrl_x0[g] + (r % 3) * dp.mv.ctrl_stride[g]; }
  {
    const int a = i / nch, ch = i - a * nch;
    if (a < st) {
      const bool on = (a < S3 ? sl : sr) >= 0;
      const long long gq = (long long)pv.q_off + p - (a < S3 ? 1 : 0);
      const double* __restrict__ xr = pv.R + ((on ? gq : 0) * S3 + (a % S3)) * ncols;
      double acc = 0.0;
      constexpr int kU = 12;
      for (int k0 = ch; k0 < ne.CB; k0 += nch * kU) {          // twelve products in flight per thread
        double xv[kU], pk[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) { const int k = min(k0 + nch * u, ne.CB - 1); xv[u] = xr[k]; pk[u] = pc[k]; }
#pragma unroll
        for (int u = 0; u < kU; ++u) acc += k0 + nch * u < ne.CB ? xv[u] * pk[u] : 0.0;
      }
      part[a][ch] = on ? acc : 0.0;
    }
    __syncthreads();
    if (i < st) {
      double t = 0.0;
#pragma unroll
      for (int w = 0; w < nch; ++w) t += part[i][w];
      const bool o = (i < S3 ? sl : sr) >= 0;
      const long long gq = (long long)pv.q_off + p - (i < S3 ? 1 : 0);
      sx[i] = o ? t + pv.R[(gq * S3 + (i % S3)) * ncols + ne.CB] : 0.0;
    }
    __syncthreads();
  }
  if (sr >= 0 && i < S3) px[xsep] = -sx[S3 + i];
  if (i >= nr) return;
  double acc = 0.0;
  if (sl >= 0) {
#pragma unroll
    for (int a = 0; a < S3; ++a) acc += vwv[a] * sx[a];
  }
  if (sr >= 0) {
#pragma unroll
    for (int a = 0; a < S3; ++a) acc += vwv[S3 + a] * sx[S3 + a];
  }
  px[xrow] = pold + acc;
}
static_assert(kPartRowsMax <= 256, "k_back_correct: one thread per row of an interior");

}  // namespace mvus
