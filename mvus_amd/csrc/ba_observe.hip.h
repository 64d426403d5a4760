// The per-observation kernels of the BA hot path: camera decode, the one-time undistortion, the fused residual + analytic Jacobian
// kernel with its store sink, the reference pattern, the motion-regulariser rows, the Jacobian's export and freeze, and the
// outlier mask with its stream compaction.  Layout and work decomposition: ba_kernels.hip.h.
#pragma once
#include <hip/hip_runtime.h>

#include "ba_dev_problem.h"
#include "ba_math.h"
#include "ba_wave.hip.h"      // wave_sum

namespace mvus {

// Decode every camera's parameters once per evaluation (C threads): Rodrigues + derivative matrix.
__global__ void k_cam_states(DevProblem dp, const double* __restrict__ x, CamState* __restrict__ cams) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= dp.C) return;
  CamState s;
  load_cam_state(x, dp.C, c, dp.calib != 0, dp.Kfix, dp.dfix, dp.H[c], s);
  cams[c] = s;
}

// Stage one camera state into LDS with the first sizeof(CamState)/8 lanes.
__device__ __forceinline__ void stage_cam(const CamState* __restrict__ cams, int c, CamState& lds_cam) {
  constexpr int kWords = sizeof(CamState) / sizeof(double);
  const double* src = reinterpret_cast<const double*>(cams + c);
  double* dst = reinterpret_cast<double*>(&lds_cam);
  if (threadIdx.x < kWords) dst[threadIdx.x] = src[threadIdx.x];
  __syncthreads();
}

// One-time undistortion of the observations when calibration is fixed (detection_to_global, common.py:126).
__global__ void k_undistort_fixed(DevProblem dp, double* __restrict__ u_obs, double* __restrict__ v_obs) {
  const int chunk = blockIdx.x;
  const int c = dp.chunk_cam[chunk];
  if ((int)threadIdx.x >= dp.chunk_count[chunk]) return;
  const long long i = dp.chunk_start[chunk] + threadIdx.x;
  const double fx = dp.Kfix[4 * c], fy = dp.Kfix[4 * c + 1], cx = dp.Kfix[4 * c + 2], cy = dp.Kfix[4 * c + 3];
  double xn, yn;
  undistort5<false>((dp.u_raw[i] - cx) / fx, (dp.v_raw[i] - cy) / fy, dp.dfix + 5 * c, xn, yn, nullptr, nullptr);
  u_obs[i] = fx * xn + cx;
  v_obs[i] = fy * yn + cy;
}

// Fused per-observation kernel: timestamp -> interval/span search -> de Boor -> R,t -> K -> |residual|
// and (JAC) the 2 x NS analytic Jacobian block.  masked != 0 keeps only the reference pattern (pat0).
#ifndef MVUS_JAC_WAVES
#define MVUS_JAC_WAVES 4
#endif
#ifndef MVUS_JAC_WAVES_CALIB
#define MVUS_JAC_WAVES_CALIB 3        // opt_calib (2 x 30 slots + the K, d tangents): at 4 wavefronts per SIMD (128 VGPRs) it spills 40 B per lane
#endif

// The Jacobian is written once and read by other kernels later: non-temporal stores.  With the chunk-major layout they take the
// kernel from 39.4 to 35.2 us when the outputs go to HBM (with the slot-major layout they cost +4 us, with plain stores into a
// cache-resident buffer they are 1 us slower; write-through sc1 stores were slower still): measured in rounds 2-3 with build variants
// (docs/NOTEBOOK.md section G); the shipped form is the only one in the source.
#define MVUS_JSTORE(ptr, val) __builtin_nontemporal_store((val), (ptr))
// Sink of eval_observation_to that stores each value of the 2 x NS block straight to the chunk-major Jacobian
// (masked: spline slots outside the pattern become zeros; an all-zero pattern row stores nothing).
struct JStoreSink {
  static constexpr bool kFactored = false;
  double *Jx, *Jy;
  long long stride;
  int32_t pat;
  int base;
  bool masked, live;
  int32_t ctrl;
  __device__ __forceinline__ void begin(int32_t c) { ctrl = c; live = !(masked && pat < 0); }
  __device__ __forceinline__ double keep(int k, double v) const {
    return (masked && k >= base && !pattern_has(pat, ctrl + (k - base) / 3)) ? 0.0 : v;
  }
  // Jx / Jy are wave-uniform (the chunk's first column of slot 0), lane the 32-bit column inside the chunk: the address is
  // an SGPR base plus a zero-extended VGPR offset, no per-lane 64-bit arithmetic and no address registers per store
  unsigned lane;
  __device__ __forceinline__ void x(int k, double v) { if (live) MVUS_JSTORE(&(Jx + (long long)k * stride)[lane], keep(k, v)); }
  __device__ __forceinline__ void y(int k, double v) { if (live) MVUS_JSTORE(&(Jy + (long long)k * stride)[lane], keep(k, v)); }
};

// ROBUST (residual-only launches with sq_part, a loss other than linear in force): the chunk's partial is the sum of f_scale^2 rho(z)
// instead of f^2 -- twice the robust cost, in the same layout and summation order; f itself stays the raw error_BA.
template <bool CALIB, bool JAC, bool ROBUST = false, class... L>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(JAC ? (CALIB ? MVUS_JAC_WAVES_CALIB : MVUS_JAC_WAVES) : 4, 8))) void k_observations(DevProblem dp, const CamState* __restrict__ cams,
                                                           const double* __restrict__ x, double* __restrict__ f,
                                                           double* __restrict__ J, int32_t* __restrict__ span,
                                                           const int32_t* __restrict__ pat0, int masked, double* __restrict__ sq_part = nullptr,
                                                           double* __restrict__ clr = nullptr, long long clr_len = 0, L... loss_v) {
  static_assert(sizeof...(L) == (ROBUST ? 1 : 0), "the robust instantiation is launched with its LossSpec, the linear one without");
  const LossSpec loss = loss_arg(loss_v...);
  constexpr int NS = 3 + (CALIB ? 15 : 6) + 12;
  // JAC: the grid is xcd_grid(n_chunks) workgroups and each XCD works on runs of consecutive chunks (xcd_tile): the kernel
  // is bound by its store stream, and an L2 that writes back runs of consecutive lines of each slot row reaches 12-14 %
  // more of the HBM write bandwidth than eight L2s interleaving 2 KB segments (50.6 -> 44.5 us at 504k detections)
  const int chunk = JAC ? xcd_tile(dp.n_chunks) : (int)blockIdx.x;
  if constexpr (!JAC) {
    // workgroups past the chunks (the LM driver's first evaluation of a solve): they zero the normal-equation storage the
    // linearisation that follows adds into -- a bandwidth-bound pass riding beside a latency-bound kernel instead of a launch of its own
    if (clr != nullptr && chunk >= dp.n_chunks) {
      const long long nb = (long long)gridDim.x - dp.n_chunks;
      for (long long i = (chunk - dp.n_chunks) * (long long)kThreads + threadIdx.x; i < clr_len; i += nb * kThreads) clr[i] = 0.0;
      return;
    }
  }
  if (chunk >= dp.n_chunks) return;
  const ChunkInfo ci = dp.chunks[chunk];                 // wave-uniform: one scalar load
  // the camera state is wave-uniform too: it is read through the scalar cache into SGPRs (34 doubles that would occupy
  // 68 VGPRs of every lane as hoisted LDS broadcasts, and no LDS staging + barrier before the first useful load)
  const CamState& cam = cams[ci.cam];
  if constexpr (!JAC) {
    // residual-only launches of the LM driver: the chunk's sum of squares is left in sq_part[chunk] (the driver needs |f|^2 of
    // every trial point; a separate pass over f for it costs a launch and 8 MB of reads).  Every lane stays for the reduction.
    if (sq_part != nullptr) {
      __shared__ double sq_red[kThreads / 64];
      double sq = 0.0;
      if ((int)threadIdx.x < ci.count) {
        const long long i = ci.start + threadIdx.x;
        const long long a = ci.cam_start, Mc = ci.cam_count;
        const double uo = CALIB ? 0.0 : dp.u_obs[i], vo = CALIB ? 0.0 : dp.v_obs[i];
        const double ur = CALIB ? dp.u_raw[i] : 0.0;
        JStoreSink sink{J, J, kThreads, 0, NS - 12, false, true, -1, threadIdx.x};
        const ObsResult r = eval_observation_to<CALIB, false>(cam, dp.sp, x, dp.undist != 0, dp.rs_free != 0, dp.sync_free != 0, dp.frame[i], ur, dp.v_raw[i], uo, vo, sink);
        f[2 * a + (i - a)] = r.ex;
        f[2 * a + Mc + (i - a)] = r.ey;
        if (span != nullptr) span[i] = r.ctrl;           // (residual-only launches: the span table the fused assembly starts from)
        if constexpr (ROBUST) sq = loss_rho(loss, r.ex) + loss_rho(loss, r.ey);
        else sq = r.ex * r.ex + r.ey * r.ey;
      }
      sq = wave_sum(sq);
      if ((threadIdx.x & 63) == 0) sq_red[threadIdx.x >> 6] = sq;
      __syncthreads();
      if (threadIdx.x == 0) {
        double t = 0.0;
#pragma unroll
        for (int w = 0; w < kThreads / 64; ++w) t += sq_red[w];
        sq_part[chunk] = t;
      }
      return;
    }
  }
  if ((int)threadIdx.x >= ci.count) return;
  const long long i = ci.start + threadIdx.x;
  const long long a = ci.cam_start, Mc = ci.cam_count;
  const double uo = CALIB ? 0.0 : dp.u_obs[i], vo = CALIB ? 0.0 : dp.v_obs[i];
  const double ur = CALIB ? dp.u_raw[i] : 0.0;
  // every Jacobian value goes to memory as soon as it exists: the row never sits in registers as a whole
  double* __restrict__ Jc = J + j_chunk_offset<NS>(chunk);          // wave-uniform
  JStoreSink sink{Jc, Jc + NS * kThreads, kThreads, (JAC && masked) ? pat0[i] : 0, NS - 12, JAC && masked != 0, true, -1, threadIdx.x};
  ObsResult r = eval_observation_to<CALIB, JAC>(cam, dp.sp, x, dp.undist != 0, dp.rs_free != 0, dp.sync_free != 0, dp.frame[i], ur, dp.v_raw[i], uo, vo, sink);
  f[2 * a + (i - a)] = r.ex;
  f[2 * a + Mc + (i - a)] = r.ey;
  if (JAC) span[i] = (r.ctrl >= 0 && sink.live) ? r.ctrl : -1;
  else if (span != nullptr) span[i] = r.ctrl;
}

// Reference sparsity pattern of the detection rows at x0 (jac_BA + compute_visibility).
__global__ __launch_bounds__(kThreads) void k_pattern(DevProblem dp, const CamState* __restrict__ cams, int32_t* __restrict__ pat0) {
  __shared__ CamState cam;
  const int chunk = blockIdx.x;
  const int c = dp.chunk_cam[chunk];
  stage_cam(cams, c, cam);
  if ((int)threadIdx.x >= dp.chunk_count[chunk]) return;
  const long long i = dp.chunk_start[chunk] + threadIdx.x;
  pat0[i] = observation_pattern(cam, dp.sp, dp.frame[i], dp.v_raw[i]);
}

// Motion-regulariser rows (error_motion / motion_prior): one thread per sample.
template <bool JAC, bool ROBUST = false, class... L>
__global__ __launch_bounds__(kThreads) void k_motion(DevProblem dp, const double* __restrict__ x, double* __restrict__ fm,
                                                     double* __restrict__ mJ, int32_t* __restrict__ mctrl, int masked, double* __restrict__ sq_part = nullptr,
                                                     L... loss_v) {
  static_assert(sizeof...(L) == (ROBUST ? 1 : 0), "the robust instantiation is launched with its LossSpec, the linear one without");
  const LossSpec loss = loss_arg(loss_v...);
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if constexpr (!JAC) {
    if (sq_part != nullptr) {                            // residual-only, with the workgroup's sum of squares (see k_observations)
      __shared__ double sq_red[kThreads / 64];
      double v = 0.0;
      if (j < dp.T) {
        const int key = dp.mv.ctrl[j];
        if (key >= dp.mot_lo && key < dp.mot_hi) { double jrow[36]; int32_t cidx[3]; v = eval_motion_row<false>(dp.mv, x, j, false, jrow, cidx); }
        fm[j] = v;
      }
      double sq = wave_sum(ROBUST ? loss_rho(loss, v) : v * v);
      if ((threadIdx.x & 63) == 0) sq_red[threadIdx.x >> 6] = sq;
      __syncthreads();
      if (threadIdx.x == 0) {
        double t = 0.0;
#pragma unroll
        for (int w = 0; w < kThreads / 64; ++w) t += sq_red[w];
        sq_part[blockIdx.x] = t;
      }
      return;
    }
  }
  if (j >= dp.T) return;
  int32_t cidx[3];
  const int key = dp.mv.ctrl[j];
  if (key < dp.mot_lo || key >= dp.mot_hi) {          // owned by another time shard: a row of zeros here
    fm[j] = 0.0;
    if (JAC) {
#pragma unroll
      for (int k = 0; k < 3; ++k) mctrl[(long long)k * dp.T + j] = -1;
    }
    return;
  }
  if (JAC) {
    // every entry goes to memory as it is produced (zeros first: the row function hands over the non-zero ones) -- the row never
    // sits in a local array (36 doubles + index arithmetic were 304 bytes of scratch per lane)
#pragma unroll
    for (int k = 0; k < 36; ++k) mJ[(long long)k * dp.T + j] = 0.0;
    double* mj = mJ + j;
    const long long T = dp.T;
    fm[j] = eval_motion_row_to<true>(dp.mv, x, j, masked != 0, [&](int k, int q, int d, double v) { mj[(long long)(12 * k + 3 * q + d) * T] = v; }, cidx);
#pragma unroll
    for (int k = 0; k < 3; ++k) mctrl[(long long)k * dp.T + j] = cidx[k];
  } else {
    double jrow[1];
    fm[j] = eval_motion_row<false>(dp.mv, x, j, false, jrow, cidx);
  }
}

// the C ABI's slot-major copy of the Jacobian, Jout[r * M + i], from the chunk-major device layout (inspection calls only)
template <int NS>
__global__ __launch_bounds__(kThreads) void k_j_export(DevProblem dp, const double* __restrict__ J, double* __restrict__ Jout) {
  const int chunk = blockIdx.x;
  if ((int)threadIdx.x >= dp.chunk_count[chunk]) return;
  const long long i = dp.chunk_start[chunk] + threadIdx.x;
  const double* __restrict__ Jc = J + j_chunk_offset<NS>(chunk) + threadIdx.x;
  for (int r = 0; r < 2 * NS; ++r) Jout[(long long)r * dp.M + i] = Jc[r * kThreads];
}

// Frozen camera-side unknowns in the stored Jacobian (mvus_ba_set_frozen, TRF + LSMR): slot k of camera c is, in the chunk-major
// layout, rows k and NS + k of every chunk of that camera.  slot_frozen[c * B + k] != 0 zeroes them (all kThreads lanes of the chunk:
// the block is allocated in full); J v and J^T u then never move x[k].  Launched only with a non-empty mask.
template <int NS>
__global__ __launch_bounds__(kThreads) void k_freeze_jacobian(DevProblem dp, const uint8_t* __restrict__ slot_frozen, double* __restrict__ J) {
  constexpr int B = NS - 12;
  const int chunk = blockIdx.x;
  if (chunk >= dp.n_chunks) return;
  const uint8_t* __restrict__ fz = slot_frozen + dp.chunk_cam[chunk] * B;
  double* __restrict__ Jc = J + j_chunk_offset<NS>(chunk) + threadIdx.x;
  for (int k = 0; k < B; ++k) {
    if (!fz[k]) continue;
    Jc[k * kThreads] = 0.0;
    Jc[(NS + k) * kThreads] = 0.0;
  }
}

// Scene.remove_outliers (common.py:709-713): keep = sqrt(ex^2 + ey^2) < thres.  Explicit round-to-nearest
// multiplies/adds (no FMA contraction) so the integer result is the one numpy computes from the same ex, ey.
__global__ __launch_bounds__(kThreads) void k_outlier_mask(DevProblem dp, const double* __restrict__ f, double thres,
                                                           uint8_t* __restrict__ keep) {
  const int chunk = blockIdx.x;
  const int c = dp.chunk_cam[chunk];
  if ((int)threadIdx.x >= dp.chunk_count[chunk]) return;
  const long long i = dp.chunk_start[chunk] + threadIdx.x;
  const long long a = dp.det_off[c], Mc = dp.det_off[c + 1] - a;
  const double ex = f[2 * a + (i - a)], ey = f[2 * a + Mc + (i - a)];
  const double e = __dsqrt_rn(__dadd_rn(__dmul_rn(ex, ex), __dmul_rn(ey, ey)));
  keep[i] = e < thres ? 1 : 0;
}

// ---- in-place removal of outliers (stable stream compaction per chunk) ----------------------------------------
__global__ __launch_bounds__(kThreads) void k_compact_count(DevProblem dp, const uint8_t* __restrict__ keep, int32_t* __restrict__ counts) {
  const int chunk = blockIdx.x;
  const bool k = (int)threadIdx.x < dp.chunk_count[chunk] && keep[dp.chunk_start[chunk] + threadIdx.x];
  const int c = __syncthreads_count(k ? 1 : 0);
  if (threadIdx.x == 0) counts[chunk] = c;
}
__global__ __launch_bounds__(kThreads) void k_compact_scatter(DevProblem dp, const uint8_t* __restrict__ keep, const long long* __restrict__ out_off,
                                                              double* __restrict__ frame, double* __restrict__ u_raw, double* __restrict__ v_raw,
                                                              double* __restrict__ u_obs, double* __restrict__ v_obs) {
  __shared__ int wave_cnt[kThreads / 64];
  const int chunk = blockIdx.x;
  const bool act = (int)threadIdx.x < dp.chunk_count[chunk];
  const long long i = dp.chunk_start[chunk] + (act ? threadIdx.x : 0);
  const bool k = act && keep[i];
  const unsigned long long bal = __ballot(k);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) wave_cnt[wave] = __popcll(bal);
  __syncthreads();
  int base = 0;
  for (int w = 0; w < wave; ++w) base += wave_cnt[w];
  if (k) {
    const long long o = out_off[chunk] + base + __popcll(bal & ((1ull << lane) - 1ull));
    frame[o] = dp.frame[i]; u_raw[o] = dp.u_raw[i]; v_raw[o] = dp.v_raw[i]; u_obs[o] = dp.u_obs[i]; v_obs[o] = dp.v_obs[i];
  }
}

}  // namespace mvus
