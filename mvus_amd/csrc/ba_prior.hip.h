// Position priors on the trajectory (mvus_ba_set_position_priors): surveyed positions p_k at times t_k on the spline's own timeline,
// with weights w_k = 1 / sigma per axis, as three plain L2 rows each
//     r = w_k (.) (S(t_k) - p_k)
// beside the detection and motion rows.  A pass of their own at the two places the motion rows and the freeze pass use:
//   k_prior_setup   at set time: interval, knot span and the four B-spline weights of every prior (constants: t_k is no unknown);
//   k_prior_cost    behind k_motion in every residual evaluation of the LM driver: one more partial sum per workgroup;
//   k_prior_ne      behind every assembly (HipSchur::assemble, in front of the freeze pass): += on the spline gradient and the band.
// The rows touch four adjacent control points and nothing on the camera side: A, gc and the cross block are not read or written, and
// the band (W >= 4) is never widened.  A robust loss in force does not reach them.  A handle without active priors launches none of
// the three.  One rank only (refused on sharded handles before anything is launched).
#pragma once
#include <hip/hip_runtime.h>

#include "ba_assemble.hip.h"      // k_det_motion
#include "ba_dev_problem.h"
#include "ba_ne_views.h"
#include "ba_prior_math.h"
#include "ba_wave.hip.h"

namespace mvus {

// The priors of a handle on the device, sorted by (t, input order)
struct PriorView {
  int K;                     // all priors, inactive ones included
  const double* t;           // [K]
  const double* p;           // [3K] x(K) y(K) z(K)
  const double* w;           // [3K] 1 / sigma, same layout (0: that axis is unknown)
  int32_t* ctrl;             // [K] first control point (global index), -1 = inactive
  double* h;                 // [4K] h[4 k + a]: weight of control point ctrl[k] + a
  const int32_t* row_lo;     // [N] priors row_lo[g] .. row_hi[g] - 1 are the ones that can touch control point g (as MotionView::row_lo / row_hi)
  const int32_t* row_hi;
};

__global__ __launch_bounds__(kThreads) void k_prior_setup(SplineView sp, PriorView pv) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= pv.K) return;
  double h[4];
  pv.ctrl[k] = prior_setup_row(sp, pv.t[k], h);
#pragma unroll
  for (int a = 0; a < 4; ++a) pv.h[4 * k + a] = h[a];
}

// S(t_k) - p_k and w_k of prior k (active)
__device__ __forceinline__ void prior_load(const DevProblem& dp, const PriorView& pv, const double* __restrict__ x, int k, int c0, double h[4],
                                           double w[3], double diff[3]) {
  int32_t x0[4], st[4];
  double p[3];
#pragma unroll
  for (int a = 0; a < 4; ++a) { h[a] = pv.h[4 * k + a]; x0[a] = dp.mv.ctrl_x0[c0 + a]; st[a] = dp.mv.ctrl_stride[c0 + a]; }
#pragma unroll
  for (int d = 0; d < 3; ++d) { p[d] = pv.p[(long long)d * pv.K + k]; w[d] = pv.w[(long long)d * pv.K + k]; }
  prior_diff(x, x0, st, h, p, diff);
}

// Sum of r^2 over the priors: lane = prior (grid-stride, so the order of additions is fixed by K and the grid), one partial per workgroup
// in the residual kernels' own tree (wave_sum, then the wavefronts in order) -- sq_part continues the partials of k_observations and
// k_motion, and k_dot_final / sq_host_sum add them all.  r_out (the inspection hook only): the 3K rows in sorted order, NaN where inactive.
__global__ __launch_bounds__(kThreads) void k_prior_cost(DevProblem dp, PriorView pv, const double* __restrict__ x, double* __restrict__ sq_part,
                                                         double* __restrict__ r_out) {
  __shared__ double sq_red[kThreads / 64];
  double sq = 0.0;
  for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < pv.K; k += gridDim.x * blockDim.x) {
    const int c0 = pv.ctrl[k];
    double r[3] = {__builtin_nan(""), __builtin_nan(""), __builtin_nan("")};
    if (c0 >= 0) {
      double h[4], w[3], diff[3];
      prior_load(dp, pv, x, k, c0, h, w, diff);
#pragma unroll
      for (int d = 0; d < 3; ++d) { r[d] = w[d] * diff[d]; sq += r[d] * r[d]; }
    }
    if (r_out != nullptr) {
#pragma unroll
      for (int d = 0; d < 3; ++d) r_out[(long long)d * pv.K + k] = r[d];
    }
  }
  sq = wave_sum(sq);
  if ((threadIdx.x & 63) == 0) sq_red[threadIdx.x >> 6] = sq;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
#pragma unroll
    for (int w = 0; w < kThreads / 64; ++w) t += sq_red[w];
    sq_part[blockIdx.x] = t;
  }
}

// The priors' part of the normal equations, shaped like k_det_motion: one wavefront per control point g.  The priors that can touch g
// (row_lo[g] <= k < row_hi[g]) are taken 64 at a time: first lane = ROW -- with a = g - ctrl[k] the row's weight on g itself, its weights
// on g .. g + 3, w^2 and w^2 (S - p) go to LDS (zeros for a row that is inactive or does not reach g); then lane = ENTRY -- gradient
// coordinate d:  h_a w_d^2 (S - p)_d,  or band entry (v, d, d):  h_a h_{a+v} w_d^2 -- adds the rows in sorted order and issues one +=.
// One writer and one order of additions per entry, no atomics: the same bits on every run, and for every order the caller gave the
// priors in.  Off-diagonal entries of a 3 x 3 block and every camera-side entry are not touched.
constexpr int kPriorRv = 11;       // per row: h_a | h_a .. h_{a+3} | w^2 (3) | w^2 (S - p) (3)
__global__ __launch_bounds__(kThreads) void k_prior_ne(DevProblem dp, PriorView pv, const double* __restrict__ x, NEView ne) {
  constexpr int kWaves = kThreads / 64;
  __shared__ double rv[kWaves][64][kPriorRv];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = (int)blockIdx.x * kWaves + wave;
  if (g >= ne.N) return;                                // (wave-uniform; no workgroup barrier below)
  const int k0 = pv.row_lo[g], k1 = pv.row_hi[g];
  const bool grad = lane < 3;
  const int v = grad ? 0 : (lane - 3) / 3, d = grad ? lane : (lane - 3) % 3;      // lanes 3 .. 14: band block (g, g + v), diagonal entry d
  const bool mine = lane < 3 + 4 * 3 && g + v < ne.N;
  double acc = 0.0;
  for (int kb = k0; kb < k1; kb += 64) {
    const int k = kb + lane;
    double r[kPriorRv];
#pragma unroll
    for (int e = 0; e < kPriorRv; ++e) r[e] = 0.0;
    if (k < k1) {
      const int c0 = pv.ctrl[k], a = g - c0;
      if (c0 >= 0 && a >= 0 && a < 4) {
        double h[4], w[3], diff[3];
        prior_load(dp, pv, x, k, c0, h, w, diff);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          if (q == a) r[0] = h[q];
#pragma unroll
          for (int u = 0; u < 4; ++u) if (q == a + u) r[1 + u] = h[q];      // static indexing of h: select by comparison
        }
#pragma unroll
        for (int dd = 0; dd < 3; ++dd) { const double w2 = w[dd] * w[dd]; r[5 + dd] = w2; r[8 + dd] = w2 * diff[dd]; }
      }
    }
#pragma unroll
    for (int e = 0; e < kPriorRv; ++e) rv[wave][lane][e] = r[e];
    lds_wave_sync();
    const int nrow = min(64, k1 - kb);
    if (mine) {
      for (int t = 0; t < nrow; ++t) {
        const double ha = rv[wave][t][0];
        acc += grad ? ha * rv[wave][t][8 + d] : (ha * rv[wave][t][1 + v]) * rv[wave][t][5 + d];
      }
    }
    lds_wave_sync();
  }
  if (mine && acc != 0.0) {
    if (grad) ne.gs[3 * g + d] += acc;
    else ne.Cb[((long long)g * ne.W + v) * 9 + 4 * d] += acc;
  }
}

}  // namespace mvus
