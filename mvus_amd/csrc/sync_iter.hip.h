// The iterative time-shift search of Albl et al. as the reference runs it (synchronization.py:13-130, "sync_method": "iter"), on the
// GPU: synchronization.sync_iter_gpu / "sync_method": "iter_gpu" through mvus_sync_iter_* (include/mvus_ba.h).
//
// Both cameras' interpolating splines are fitted once on the host (scipy splprep(s=0, k=3)), camera 2's on its own unshifted timeline:
// the reference refits spline 2 after every accepted step, but that refit is the same curve with shifted knots, so the device carries
// the scalar `shift` (the current beta) instead.  Camera 2's samples lie at t2 + shift on camera 1's timeline.  One round is
//   k_si_hypotheses   one lane per (sign of d, hypothesis): nine distinct sample indices (si_sample9, or indices handed in), s1 =
//                     S1(t2 + shift), s2 = S2(t2), ds = S2(t2 + d) - s2 (before the first knot for d < 0: splev's extension), the
//                     finite real eigenvalues of the pencil A1 + beta A2 (si_pencil_betas: 6 x 6 after projecting off the three
//                     columns that are zero in A2, Hessenberg + Francis QR for start values, Rayleigh-quotient refinement on the
//                     pencil).  Up to six beta, ascending, a valid flag per slot; a repeated timestamp, a non-finite sample or a
//                     degenerate one gives no model.  The lane's matrices lie in LDS as [element][lane].
//   k_si_models       one lane per (sign, hypothesis, slot): x2 = s2 + beta ds and the normalised 8-point fit with x2^T F s1 = 0 on
//                     the device (one-sided Jacobi on the 9 x 9 system and on the 3 x 3 for rank 2); model = (F, beta d, valid).
//   k_si_score        THE HOT ONE: models x samples.  One workgroup per (model, tile of 2048 camera-1 samples), lanes striding
//                     over the samples, which are sorted in time, so neighbouring lanes read neighbouring spline pieces: tau = t1 -
//                     shift + beta d, the overlap test start <= tau < end against camera 2's intervals, S2(tau) from a uniform
//                     first guess of the span plus a short walk, the squared Sampson error against the threshold.  Two integer
//                     counts stay in registers, then a wave reduction, four wave partials in LDS and one integer atomic add per
//                     count and workgroup.  No floating-point atomics; integer sums only, so the same bits on every run.
//   k_si_select       one workgroup per sign: ratio = inliers / overlap in double, the highest wins with strict >, in (hypothesis,
//                     slot) order, starting from 0; overlap 0 is skipped (the reference's `except: return None`).
// with one synchronisation and one read-back of eight doubles.  fp64 throughout.
#pragma once
#include "sync_iter_math.h"

namespace mvus {

struct SiView {                       // by value in the kernel arguments: wave-uniform
  const double *t1k, *c1;             // spline 1: knots [n1 + 4], coefficients x [n1] then y [n1]
  const double *t2k, *c2;             // spline 2, on camera 2's own timeline
  const double* iv;                   // camera 2's intervals, [start, end) pairs
  const double* d1;                   // camera 1: t [N1], x [N1], y [N1]
  const double* t2;                   // camera 2's timestamps [N2]
  long long N1, N2;
  int n1, n2, K;
};

constexpr int kSiSampDoubles = 54;    // per hypothesis: s1, s2, ds, each x[9] then y[9]
constexpr int kSiScoreTile = 2048;    // camera-1 samples per workgroup of k_si_score

#if defined(__HIPCC__)
// samp[((sg H + h) 54 ..], betas[(sg H + h) 6 + k], valid likewise; grid (ceil(H / 64), signs).  idx_in: explicit indices [H * 9]
// (already range-checked on the host) or NULL for the sampler with n indices to draw from.
__global__ __launch_bounds__(64) void k_si_hypotheses(SiView v, double shift, int d, int H, unsigned long long seed, int round, long long n,
                                                      const long long* __restrict__ idx_in, double* __restrict__ samp,
                                                      double* __restrict__ betas, uint8_t* __restrict__ valid) {
  __shared__ double wk[kSiPencilWork * 64];
  const int h = blockIdx.x * 64 + threadIdx.x, sg = blockIdx.y;
  if (h >= H) return;
  const double dd = sg ? -(double)d : (double)d;
  long long idx[kSiSample];
  if (idx_in) for (int k = 0; k < kSiSample; ++k) idx[k] = idx_in[(long long)h * kSiSample + k];
  else si_sample9(seed, round, sg, h, n, idx);
  double s1[18], s2[18], ds[18], u[kSiSample];
  bool ok = true;
  for (int k = 0; k < kSiSample; ++k) {
    u[k] = v.t2[idx[k]];
    for (int j = 0; j < k; ++j) ok = ok && u[j] != u[k];               // a repeated timestamp: two equal rows, no model
    double o[2], p[2];
    si_spline_eval2(v.t1k, v.c1, v.n1, u[k] + shift, o);
    s1[k] = o[0]; s1[9 + k] = o[1];
    si_spline_eval2(v.t2k, v.c2, v.n2, u[k], o);
    s2[k] = o[0]; s2[9 + k] = o[1];
    si_spline_eval2(v.t2k, v.c2, v.n2, u[k] + dd, p);
    ds[k] = p[0] - o[0]; ds[9 + k] = p[1] - o[1];
  }
  const long long base = (long long)sg * H + h;
  double* sp = samp + base * kSiSampDoubles;
  for (int k = 0; k < 18; ++k) { sp[k] = s1[k]; sp[18 + k] = s2[k]; sp[36 + k] = ds[k]; }
  double b[kSiSlots];
  const int nb = ok ? si_pencil_betas(s1, s2, ds, wk + threadIdx.x, 64, b) : 0;
  for (int k = 0; k < kSiSlots; ++k) {
    betas[base * kSiSlots + k] = k < nb ? b[k] : 0.0;
    valid[base * kSiSlots + k] = k < nb ? 1 : 0;
  }
}

// models[m 11 ..] for m = (sg H + h) 6 + slot; valid[] is cleared where the fit fails; grid ceil(signs H 6 / 64)
__global__ __launch_bounds__(64) void k_si_models(int d, int H, int signs, const double* __restrict__ samp, const double* __restrict__ betas,
                                                  uint8_t* __restrict__ valid, double* __restrict__ models) {
  __shared__ double wk[kSiFitWork * 64];
  const long long m = blockIdx.x * 64ll + threadIdx.x;
  if (m >= (long long)signs * H * kSiSlots) return;
  const long long base = m / kSiSlots;
  const double dd = base >= H ? -(double)d : (double)d;
  double F[9];
  bool ok = valid[m] != 0;
  const double beta = betas[m];
  if (ok) {
    const double* sp = samp + base * kSiSampDoubles;
    double s1[18], x2[18];
    for (int k = 0; k < 18; ++k) { s1[k] = sp[k]; x2[k] = si_mul_add(sp[18 + k], beta, sp[36 + k]); }
    ok = si_fundamental9(s1, x2, wk + threadIdx.x, 64, F);
  }
  double* out = models + m * kSiModel;
  for (int a = 0; a < 9; ++a) out[a] = ok ? F[a] : 0.0;
  out[9] = ok ? beta * dd : 0.0;
  out[10] = ok ? 1.0 : 0.0;
  if (!ok) valid[m] = 0;
}

__device__ __forceinline__ int si_wave_sum_int(int v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// counts[2 m] += inliers, counts[2 m + 1] += overlap of model m over the samples of tile blockIdx.y; grid (models, tiles); counts zeroed before
__global__ __launch_bounds__(256) void k_si_score(SiView v, double shift, const double* __restrict__ models, double threshold,
                                                  int32_t* __restrict__ counts) {
  __shared__ int red[2][4];
  const long long m = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const double* md = models + m * kSiModel;
  if (md[10] == 0.0) return;                                           // (uniform over the workgroup)
  double F[9];
  for (int a = 0; a < 9; ++a) F[a] = md[a];
  const double off = md[9];
  const long long i0 = (long long)blockIdx.y * kSiScoreTile;
  const long long i1 = i0 + kSiScoreTile < v.N1 ? i0 + kSiScoreTile : v.N1;
  int inl = 0, ovl = 0;
  for (long long i = i0 + threadIdx.x; i < i1; i += 256) {
    const double tau = v.d1[i] - shift + off;
    if (!si_in_intervals(v.iv, v.K, tau)) continue;                    // (false for a NaN)
    double x2[2];
    si_spline_at(v.t2k, v.c2, v.n2, si_find_span_guess(v.t2k, v.n2, tau), tau, x2);
    ++ovl;
    inl += si_sampson(F, v.d1[v.N1 + i], v.d1[2 * v.N1 + i], x2[0], x2[1]) < threshold ? 1 : 0;
  }
  inl = si_wave_sum_int(inl);
  ovl = si_wave_sum_int(ovl);
  if (lane == 0) { red[0][wave] = inl; red[1][wave] = ovl; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const int a = red[0][0] + red[0][1] + red[0][2] + red[0][3], b = red[1][0] + red[1][1] + red[1][2] + red[1][3];
    if (a) atomicAdd(counts + 2 * m, a);
    if (b) atomicAdd(counts + 2 * m + 1, b);
  }
}

// out[4 sg ..] = -shift of the winner, its ratio, inliers, overlap (zeros when no model has overlap); Mper models per sign; grid (signs)
__global__ __launch_bounds__(256) void k_si_select(long long Mper, const double* __restrict__ models, const int32_t* __restrict__ counts,
                                                   double* __restrict__ out) {
  __shared__ double br[256];
  __shared__ long long bi[256];
  const int sg = blockIdx.x;
  const long long chunk = (Mper + 255) / 256, lo = threadIdx.x * chunk, hi = lo + chunk < Mper ? lo + chunk : Mper;
  double best = 0.0;
  long long arg = -1;
  for (long long k = lo; k < hi; ++k) {
    const long long m = (long long)sg * Mper + k;
    const int ovl = counts[2 * m + 1];
    if (ovl <= 0) continue;
    const double r = (double)counts[2 * m] / (double)ovl;
    if (r > best) { best = r; arg = m; }
  }
  br[threadIdx.x] = best; bi[threadIdx.x] = arg;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int t = 1; t < 256; ++t) if (br[t] > best) { best = br[t]; arg = bi[t]; }      // ascending chunks: the first of equals stays
    out[4 * sg] = arg >= 0 ? -models[arg * kSiModel + 9] : 0.0;
    out[4 * sg + 1] = best;
    out[4 * sg + 2] = arg >= 0 ? (double)counts[2 * arg] : 0.0;
    out[4 * sg + 3] = arg >= 0 ? (double)counts[2 * arg + 1] : 0.0;
  }
}
#endif

}  // namespace mvus
