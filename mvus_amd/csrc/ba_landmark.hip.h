// Surveyed landmarks (mvus_ba_set_landmarks): constant world points X_l clicked in the cameras' images, with weights w = 1 / sigma in
// pixels per axis, as two plain L2 rows each
//     r = w (.) (pi_c(X_l) - obs)
// beside the detection, motion and position-prior rows.  The position priors' design (ba_prior.hip.h) mirrored onto the camera side:
//   k_landmark_setup  at set time: the observed pixel under fixed calibration with undist_points, undistorted once;
//   k_landmark_cost   behind k_prior_cost in every residual evaluation of the LM driver: one more partial sum per workgroup;
//   k_landmark_ne     behind every assembly (HipSchur::assemble, in front of the freeze pass): += on the camera blocks and gradient.
// The rows touch the P parameters of ONE camera: the sync slots 0..2 of its block, the cross block, the band, the spline gradient and
// every other camera's block are not read or written.  A robust loss in force does not reach them.  A handle without a weighted
// observation launches none of the three.  One rank only (refused on sharded handles before anything is launched).
#pragma once
#include <hip/hip_runtime.h>

#include "ba_dev_problem.h"
#include "ba_landmark_math.h"
#include "ba_ne_views.h"
#include "ba_wave.hip.h"      // wave_sum

namespace mvus {

// The landmark observations of a handle on the device, sorted by (camera, landmark, input order)
struct LandmarkView {
  int K, L;                  // observations (weightless ones included), landmarks
  const double* X;           // [3L] x(L) y(L) z(L)
  const int32_t* cam;        // [K]
  const int32_t* point;      // [K]
  const double* uv;          // [2K] u(K) v(K), raw pixels
  double* uvo;               // [2K] the observed pixel of the row under fixed calibration (undistorted by k_landmark_setup, else = uv)
  const double* w;           // [2K] 1 / sigma, same layout (0: that axis is unknown)
  const int32_t* row_lo;     // [C] observations row_lo[c] .. row_hi[c] - 1 are camera c's
  const int32_t* row_hi;
};

__global__ __launch_bounds__(kThreads) void k_landmark_setup(DevProblem dp, LandmarkView lv) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= lv.K) return;
  double uo, vo;
  landmark_undistort_fixed(dp.Kfix, dp.dfix, lv.cam[k], lv.uv[k], lv.uv[lv.K + k], uo, vo);
  lv.uvo[k] = uo; lv.uvo[lv.K + k] = vo;
}

// observation k at the decoded cameras: the weighted residual pair, and with JAC the weighted 2 x P block through emit(axis, i, v)
template <bool JAC, class Emit>
__device__ __forceinline__ void landmark_eval(const DevProblem& dp, const LandmarkView& lv, const CamState& cam, int k, double r[2], Emit&& emit) {
  const int l = lv.point[k];
  const double X[3] = {lv.X[l], lv.X[lv.L + l], lv.X[2 * lv.L + l]};
  const double wu = lv.w[k], wv = lv.w[lv.K + k];
  double ru, rv;
  landmark_row<JAC>(cam, dp.calib != 0, dp.undist != 0, X, lv.uv[k], lv.uv[lv.K + k], lv.uvo[k], lv.uvo[lv.K + k], ru, rv,
                    [&](int axis, int i, double v) { const double w = axis ? wv : wu; emit(axis, i, w > 0.0 ? w * v : 0.0); });
  r[0] = wu > 0.0 ? wu * ru : 0.0;       // (a weightless axis is exactly 0, whatever the projection gives there)
  r[1] = wv > 0.0 ? wv * rv : 0.0;
}

// Sum of r^2 over the landmark rows: lane = observation (grid-stride, so the order of additions is fixed by K and the grid), one partial
// per workgroup in the residual kernels' own tree -- sq_part continues the partials of k_observations, k_motion and k_prior_cost.
// r_out / J_out (the inspection hooks only): r[2K] as u(K) v(K) and J[K][2][P], both in sorted order.
__global__ __launch_bounds__(kThreads) void k_landmark_cost(DevProblem dp, LandmarkView lv, const CamState* __restrict__ cams, double* __restrict__ sq_part,
                                                            double* __restrict__ r_out, double* __restrict__ J_out) {
  __shared__ double sq_red[kThreads / 64];
  double sq = 0.0;
  for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < lv.K; k += gridDim.x * blockDim.x) {
    const CamState cam = cams[lv.cam[k]];
    double r[2];
    if (J_out != nullptr) {
      double* Jk = J_out + (long long)k * 2 * dp.P;
      landmark_eval<true>(dp, lv, cam, k, r, [&](int axis, int i, double v) { Jk[axis * dp.P + i] = v; });
    } else {
      landmark_eval<false>(dp, lv, cam, k, r, [](int, int, double) {});
    }
    sq += r[0] * r[0]; sq += r[1] * r[1];
    if (r_out != nullptr) { r_out[k] = r[0]; r_out[lv.K + k] = r[1]; }
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

// The landmarks' part of the normal equations: one workgroup per camera c, its rows row_lo[c] .. row_hi[c] - 1 taken kThreads at a time.
// Phase one, thread = ROW: the weighted residual pair and 2 x P block go to LDS as the row's two augmented vectors [J_u | r_u], [J_v | r_v]
// (2P + 2 doubles, row stride 2P + 3: odd, so the 64 lanes of a store hit distinct banks).  Phase two, thread = ENTRY (a, b) of the
// triangle of [J | r]^T [J | r] without its corner (landmark_entry: P (P + 3) / 2 threads, 135 of 256 at P = 15): every thread reads the
// SAME row at the same time -- 2P + 2 consecutive doubles, one bank each, equal addresses broadcast -- and adds u_a u_b + v_a v_b in sorted
// order into four interleaved accumulators (row index mod 4) that live across the rounds, folded (0 + 1) + (2 + 3) at the end: the
// dependent chain per entry is half a row's two fused multiply-adds, whatever K is.  Then one += per entry on A (and its mirror) or gc:
// one writer and one order of additions per entry, no atomics -- the same bits on every run, and for every order the caller gave the
// observations in as long as no (camera, landmark) pair occurs twice.
constexpr int landmark_stride(int P) { return 2 * P + 3; }
constexpr size_t landmark_lds_bytes(int P) { return (size_t)kThreads * landmark_stride(P) * sizeof(double); }      // 67.6 KB at P = 15, 30.7 KB at P = 6
__global__ __launch_bounds__(kThreads) void k_landmark_ne(DevProblem dp, LandmarkView lv, const CamState* __restrict__ cams, NEView ne) {
  extern __shared__ double lm_rows[];
  const int c = blockIdx.x;
  const int k0 = lv.row_lo[c], k1 = lv.row_hi[c];
  if (k0 >= k1) return;                                   // (uniform over the workgroup)
  const int P = dp.P, stride = landmark_stride(P), tid = threadIdx.x;
  const CamState cam = cams[c];
  int a = 0, b = 0;
  const bool mine = tid < landmark_entries(P);
  if (mine) landmark_entry(P, tid, a, b);
  const int ia = a, ib = b, ja = P + 1 + a, jb = P + 1 + b;      // u_a, u_b, v_a, v_b inside a staged row
  double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0, acc3 = 0.0;
  for (int kb = k0; kb < k1; kb += kThreads) {
    const int k = kb + tid;
    if (k < k1) {
      double* row = lm_rows + tid * stride;
      double r[2];
      landmark_eval<true>(dp, lv, cam, k, r, [&](int axis, int i, double v) { row[axis * (P + 1) + i] = v; });
      row[P] = r[0]; row[2 * P + 1] = r[1];
    }
    __syncthreads();
    const int nrow = min(kThreads, k1 - kb);
    if (mine) {
      const double* row = lm_rows;
      int t = 0;
      for (; t + 4 <= nrow; t += 4, row += 4 * stride) {
        acc0 = fma(row[ja], row[jb], fma(row[ia], row[ib], acc0));
        acc1 = fma(row[stride + ja], row[stride + jb], fma(row[stride + ia], row[stride + ib], acc1));
        acc2 = fma(row[2 * stride + ja], row[2 * stride + jb], fma(row[2 * stride + ia], row[2 * stride + ib], acc2));
        acc3 = fma(row[3 * stride + ja], row[3 * stride + jb], fma(row[3 * stride + ia], row[3 * stride + ib], acc3));
      }
      // (only the last round has a remainder: kThreads is a multiple of 4, so t mod 4 is the camera's row index mod 4)
      if (t < nrow) acc0 = fma(row[ja], row[jb], fma(row[ia], row[ib], acc0));
      if (t + 1 < nrow) acc1 = fma(row[stride + ja], row[stride + jb], fma(row[stride + ia], row[stride + ib], acc1));
      if (t + 2 < nrow) acc2 = fma(row[2 * stride + ja], row[2 * stride + jb], fma(row[2 * stride + ia], row[2 * stride + ib], acc2));
    }
    __syncthreads();
  }
  const double acc = (acc0 + acc1) + (acc2 + acc3);
  if (!mine || acc == 0.0) return;
  if (b == P) { ne.gc[c * ne.B + 3 + a] += acc; return; }
  double* __restrict__ Ac = ne.A + (long long)c * ne.B * ne.B;
  Ac[(3 + a) * ne.B + 3 + b] += acc;
  if (a != b) Ac[(3 + b) * ne.B + 3 + a] += acc;
}

}  // namespace mvus
