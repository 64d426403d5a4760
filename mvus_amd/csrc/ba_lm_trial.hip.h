// The tail of an LM step (ba_schur.h): projected gradient norm, trial point and its scalars.
#pragma once
#include <hip/hip_runtime.h>

#include "ba_dev_problem.h"      // DevProblem (k_lm_trial_sum decodes the trial point's cameras)
#include "ba_math.h"             // CamState, load_cam_state
#include "ba_wave.hip.h"         // wave_sum_dpp, wave_max_dpp, last_block_done

namespace mvus {

// ---- LM driver (ba_schur.h): the two small vector reductions of an iteration --------------------------------
// One element per thread; every workgroup leaves its partial result in `part`, the last one to finish (ticket from an
// atomic counter, which it resets) combines them -- one launch, deterministic, no zero-initialised accumulator.
// projected gradient norm: a component pushing against an active bound does not count
__global__ __launch_bounds__(1024) void k_lm_gnorm(int n, const double* __restrict__ x, const double* __restrict__ lb, const double* __restrict__ ub,
                                                   const double* __restrict__ g, double* __restrict__ out, double* part, unsigned* counter) {
  __shared__ double red[16];
  double gn = 0.0;
  // batches of 8 elements per thread: all loads of a batch are issued before the first is used (one memory round trip per
  // batch instead of one per element -- a single workgroup would otherwise be latency bound)
  for (int i0 = blockIdx.x * 1024 + threadIdx.x; i0 < n; i0 += gridDim.x * 1024 * 8) {
    double gi[8], xi[8], lo[8], hi[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int i = i0 + u * gridDim.x * 1024;
      const bool in = i < n;
      gi[u] = in ? g[i] : 0.0; xi[u] = in ? x[i] : 0.0; lo[u] = in ? lb[i] : -INFINITY; hi[u] = in ? ub[i] : INFINITY;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const bool blocked = (xi[u] <= lo[u] && gi[u] > 0) || (xi[u] >= hi[u] && gi[u] < 0);
      if (!blocked) gn = fmax(gn, fabs(gi[u]));
    }
  }
  gn = wave_max_dpp(gn);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = gn;
  __syncthreads();
  if (threadIdx.x == 0) { double t = 0.0; for (int w = 0; w < 16; ++w) t = fmax(t, red[w]); part[blockIdx.x] = t; if (gridDim.x == 1) *out = t; }
  if (gridDim.x == 1) return;                              // one workgroup (n <= 128k): no cross-workgroup hand-off, no fences
  if (last_block_done(counter) && threadIdx.x == 0) {
    double t = 0.0;
    for (unsigned b = 0; b < gridDim.x; ++b) t = fmax(t, const_cast<volatile double*>(part)[b]);
    *out = t;
  }
}
// trial point x_new = P(x + p) and out = [g.step, step^T D step, |step|^2, |x|^2]; after a failed solve (fail flag)
// x_new = x, a non-finite component of p is not applied, and either way out[0] = NaN: the residual kernels never
// see a non-finite parameter and the driver rejects the trial
__global__ __launch_bounds__(1024) void k_lm_trial(int n, const double* __restrict__ x, const double* __restrict__ p, const double* __restrict__ lb,
                                                   const double* __restrict__ ub, const double* __restrict__ g, const double* __restrict__ D,
                                                   const int* __restrict__ fail, double* __restrict__ x_new, double* __restrict__ out,
                                                   double* __restrict__ gnorm_out, double* part, unsigned* counter, double* __restrict__ x_mirror,
                                                   const double* __restrict__ pn2 = nullptr, double delta = 0.0,
                                                   const double* __restrict__ fail_sum = nullptr, double* __restrict__ fail_out = nullptr) {
  // trust region (mvus_solve_opts.lm_trust_radius): a step longer than delta is cut back to delta along its direction
  const double cut = (pn2 != nullptr && delta > 0.0 && *pn2 > delta * delta) ? delta / sqrt(*pn2) : 1.0;
  if (pn2 != nullptr && blockIdx.x == 0 && threadIdx.x == 0) out[5] = *pn2;      // slot 7 of the driver's scalars
  // also delivers the projected gradient norm of k_lm_gnorm (x, g and the bounds are read here anyway): slot 4 = max
  __shared__ double red[5][16];
  // (time shards: fail_sum = the two failure flags of the solve SUMMED over the ranks -- they travelled with the step; any rank's failure
  // stops every rank's step, and the sums go on to the host with the trial's scalars)
  const bool dead = fail[0] != 0 || (fail_sum != nullptr && fail_sum[0] != 0.0);
  if (fail_sum != nullptr && blockIdx.x == 0 && threadIdx.x < 2) fail_out[threadIdx.x] = fail_sum[threadIdx.x];
  double s[5] = {dead ? __longlong_as_double(0x7ff8000000000000LL) : 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int i0 = blockIdx.x * 1024 + threadIdx.x; i0 < n; i0 += gridDim.x * 1024 * 4) {      // batches of 4: loads first, see k_lm_gnorm
    double xv[4], pv[4], gv[4], lo[4], hi[4], dv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = i0 + u * gridDim.x * 1024;
      const bool in = i < n;
      xv[u] = in ? x[i] : 0.0; pv[u] = in ? p[i] : 0.0; gv[u] = in ? g[i] : 0.0;
      lo[u] = in ? lb[i] : -INFINITY; hi[u] = in ? ub[i] : INFINITY; dv[u] = in ? D[i] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = i0 + u * gridDim.x * 1024;
      if (i >= n) break;
      const double xi = xv[u], pi = pv[u], gi = gv[u];
      const bool ok = isfinite(pi);
      const double xn = (dead || !ok) ? xi : fmin(fmax(xi + cut * pi, lo[u]), hi[u]);
      const double st = xn - xi;
      x_new[i] = xn;
      if (x_mirror) x_mirror[i] = xn;                    // mapped pinned host memory: the accepted point needs no download
      s[0] += ok ? gi * st : pi * 0.0; s[1] += st * dv[u] * st; s[2] += st * st; s[3] += xi * xi;
      const bool blocked = (xi <= lo[u] && gi > 0) || (xi >= hi[u] && gi < 0);
      s[4] = fmax(s[4], blocked ? 0.0 : fabs(gi));
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double v = wave_sum_dpp(s[k]);
    if ((threadIdx.x & 63) == 0) red[k][threadIdx.x >> 6] = v;
  }
  {
    const double v = wave_max_dpp(s[4]);
    if ((threadIdx.x & 63) == 0) red[4][threadIdx.x >> 6] = v;
  }
  __syncthreads();
  if (threadIdx.x < 5) {
    double t = 0.0;
    for (int w = 0; w < 16; ++w) t = threadIdx.x < 4 ? t + red[threadIdx.x][w] : fmax(t, red[4][w]);
    part[blockIdx.x * 5 + threadIdx.x] = t;
    if (gridDim.x == 1) { if (threadIdx.x < 4) out[threadIdx.x] = t; else *gnorm_out = t; }
  }
  if (gridDim.x == 1 || counter == nullptr) return;        // one workgroup, or k_lm_trial_sum follows: nothing to hand over
  if (last_block_done(counter) && threadIdx.x < 5) {
    double t = 0.0;
    for (unsigned b = 0; b < gridDim.x; ++b) {
      const double v = const_cast<volatile double*>(part)[b * 5 + threadIdx.x];
      t = threadIdx.x < 4 ? t + v : fmax(t, v);
    }
    if (threadIdx.x < 4) out[threadIdx.x] = t; else *gnorm_out = t;
  }
}

// second stage of k_lm_trial launched over several workgroups with counter == nullptr: the five partials per workgroup -> out
// cams != nullptr: the workgroup also decodes the camera states of the trial point (complete in memory by now) for the residual
// evaluation that follows -- k_cam_states' work without its launch
__global__ __launch_bounds__(64) void k_lm_trial_sum(int nparts, const double* __restrict__ part, double* __restrict__ out, double* __restrict__ gnorm_out,
                                                     DevProblem dp, const double* __restrict__ x_new, CamState* __restrict__ cams) {
  if (cams != nullptr)
    for (int c = threadIdx.x; c < dp.C; c += 64) {
      CamState s;
      load_cam_state(x_new, dp.C, c, dp.calib != 0, dp.Kfix, dp.dfix, dp.H[c], s);
      cams[c] = s;
    }
  if (threadIdx.x >= 5) return;
  double t = 0.0;
  for (int b = 0; b < nparts; ++b) {
    const double v = part[b * 5 + threadIdx.x];
    t = threadIdx.x < 4 ? t + v : fmax(t, v);
  }
  if (threadIdx.x < 4) out[threadIdx.x] = t; else *gnorm_out = t;
}

}  // namespace mvus
