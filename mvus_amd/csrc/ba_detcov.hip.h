// Per-detection prediction covariance and studentised residuals (mvus_ba_detection_covariance): one pass over the detections behind
// stage 8 of the covariance chain (ba_cov.hip.h, CovChain::run), from what the chain holds at that point:
//   Sig [CB][CB]   Sigma_cc at full size (stage 5),
//   Tm  [N3][CB]   T = Z Sigma_cc, kept by k_cov_tz<true> (stage 6) for this pass only,
//   Gb  [N][36]    the band blocks w <= 3 of sel + R with the rows / columns of unestimated coordinates zero (k_cov_band_out at sigma^2 = 1),
// and the analytic Jacobian of x the handle holds (chunk-major: j_chunk_offset).  Everything is in units of sigma^2 until the end.
//
// k_detcov: one lane per detection, one workgroup per chunk of at most kThreads detections, the camera in the grid's second dimension
// -- a chunk belongs to one camera, so a workgroup holds one B x B block of Sigma_cc in LDS.  A lane reads its 2 NS Jacobian slots
// (coalesced: slot rows of the chunk are kThreads doubles apart), its span, the 12 x B slice of Tm and the ten 3 x 3 blocks of Gb for
// control points p .. p + 3; neighbouring detections of a camera share slice and blocks, which the caches serve.  The three quadratic
// forms are detcov_row (ba_detcov_math.h).  The signs of the residual come from the row routine of k_observations itself,
// eval_observation_to<CALIB, false>: f and the held Jacobian no longer carry them.  No atomics: every output is an ordinary store by
// the lane that owns the detection.
#pragma once
#include "ba_detcov_math.h"
#include "ba_dev_problem.h"

namespace mvus {

// host pointers of one call (any may be null): e[2M] = u(M) v(M), pcov[3M] = uu(M) uv(M) vv(M), t2[M]
struct DetCovOut { double *e = nullptr, *pcov = nullptr, *t2 = nullptr; };

template <bool CALIB>
__global__ __launch_bounds__(kThreads) void k_detcov(DevProblem dp, const CamState* __restrict__ cams, const double* __restrict__ x,
                                                     const double* __restrict__ J, const int32_t* __restrict__ span, int CB,
                                                     const double* __restrict__ Sig, const double* __restrict__ Tm, const double* __restrict__ Gb,
                                                     double sigma2, double* __restrict__ e_out, double* __restrict__ pcov_out, double* __restrict__ t2_out) {
  constexpr int NS = 3 + (CALIB ? 15 : 6) + 12, B = NS - 12;
  static_assert(B <= 18 && B * B * sizeof(double) <= 64 * 1024, "one camera's block of Sigma_cc fits the LDS");
  __shared__ double Scc[B * B];
  const int c = blockIdx.y;
  const int chunk = dp.cam_chunk_off[c] + (int)blockIdx.x;
  if (chunk >= dp.cam_chunk_off[c + 1]) return;            // (wave-uniform: the whole workgroup leaves before the barrier)
  for (int e = threadIdx.x; e < B * B; e += kThreads) Scc[e] = Sig[((long long)c * B + e / B) * CB + (long long)c * B + e % B];
  __syncthreads();
  const ChunkInfo ci = dp.chunks[chunk];
  if ((int)threadIdx.x >= ci.count) return;
  const long long i = ci.start + threadIdx.x, M = dp.M;
  const CamState& cam = cams[c];
  const double uo = CALIB ? 0.0 : dp.u_obs[i], vo = CALIB ? 0.0 : dp.v_obs[i];
  const double ur = CALIB ? dp.u_raw[i] : 0.0;
  ArraySink none{nullptr, nullptr};                          // (residual only: the sink is never called)
  const ObsResult r = eval_observation_to<CALIB, false>(cam, dp.sp, x, dp.undist != 0, dp.rs_free != 0, dp.sync_free != 0, dp.frame[i], ur, dp.v_raw[i], uo, vo, none);
  const int p = span[i];
  const double nan = std::numeric_limits<double>::quiet_NaN();
  if (p < 0 || r.ctrl != p || p + 3 >= dp.N) {               // no span (the second and third never happen on a consistent handle: nothing is read)
    e_out[i] = 0.0; e_out[M + i] = 0.0;
    pcov_out[i] = nan; pcov_out[M + i] = nan; pcov_out[2 * M + i] = nan;
    t2_out[i] = nan;
    return;
  }
  const double* __restrict__ Jc = J + j_chunk_offset<NS>(chunk) + threadIdx.x;
  double ax[B], ay[B], bx[12], by[12];
#pragma unroll
  for (int k = 0; k < B; ++k) { ax[k] = Jc[(long long)k * kThreads]; ay[k] = Jc[(long long)(NS + k) * kThreads]; }
#pragma unroll
  for (int k = 0; k < 12; ++k) { bx[k] = Jc[(long long)(B + k) * kThreads]; by[k] = Jc[(long long)(NS + B + k) * kThreads]; }
  double pi[3], pc[3];
  detcov_row<B>(ax, ay, bx, by, Scc, B, Tm + (long long)(3 * p) * CB + (long long)c * B, CB, Gb + (long long)p * 36, pi, nullptr);
#pragma unroll
  for (int k = 0; k < 3; ++k) pi[k] *= sigma2;
  detcov_image_axes(pi, r.ru < 0.0 ? -1.0 : 1.0, r.rv < 0.0 ? -1.0 : 1.0, pc);
  e_out[i] = r.ru; e_out[M + i] = r.rv;
  pcov_out[i] = pc[0]; pcov_out[M + i] = pc[1]; pcov_out[2 * M + i] = pc[2];
  t2_out[i] = detcov_t2(pi, sigma2, r.ex, r.ey);
}

}  // namespace mvus
