// Spline maintenance either side of BA, on the GPU:
//   k_spline_eval     Scene.spline_to_traj (reference common.py:273-301): X(t) of the interval each timestamp belongs to
//                     (closed ends, common.py:292) -- scipy splev == FITPACK splev.f/fpbspl.f, the same recurrence
//                     (bspline_basis) the BA kernels use
//   k_lsq_*           least-squares coefficients of a cubic spline on a FIXED knot vector for data (t_i, X_i): the banded
//                     normal equations B^T B c = B^T X (bandwidth 4) accumulated by one lane per data point, then a banded
//                     Cholesky solve by one wavefront.  The reference's traj_to_spline lets FITPACK choose the knots
//                     adaptively inside its smooth_factor loop (common.py:224-270); that search stays on the host
//                     (Scene.traj_to_spline), this is the refit on the knots it found -- scipy's make_lsq_spline is the oracle.
//   k_spline_cov_eval the covariance of the same samples from the control points' band of mvus_ba_covariance (cov_spline_sample)
//   k_spline_eval_der, k_spline_kin_cov_eval, k_span_length / k_span_prefix / k_spline_length
//                     kinematics of the same samples (spline_kin_math.h): X, X', X''; the covariance of that state from the band; the
//                     distance flown since the start of the interval
#pragma once
#include "ba_math.h"
#include "ba_cov_math.h"
#include "spline_kin_math.h"

namespace mvus {

#if defined(__HIPCC__)
struct SplineSet {               // S splines as they sit in device memory
  int S;
  const double* istart;          // [S]
  const double* iend;            // [S]
  const long long* knot_off;     // [S+1]
  const double* knots;
  const long long* coef_off;     // [S+1] offset of spline s' coefficient block (cx(n) cy(n) cz(n)) in coefs, in doubles
  const double* coefs;
};

__global__ __launch_bounds__(256) void k_spline_eval(SplineSet sp, long long nt, const double* __restrict__ t, double* __restrict__ X,
                                                     int32_t* __restrict__ which) {
  const long long i = blockIdx.x * 256ll + threadIdx.x;
  if (i >= nt) return;
  const double x = t[i];
  int lo = 0, hi = sp.S;                              // last interval whose start <= x
  while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (x >= sp.istart[mid]) lo = mid; else hi = mid; }
  const bool in = x >= sp.istart[lo] && x <= sp.iend[lo];        // closed at both ends (common.py:292)
  which[i] = in ? lo : -1;
  double o0 = 0.0, o1 = 0.0, o2 = 0.0;
  if (in) {
    const double* k = sp.knots + sp.knot_off[lo];
    const int n = (int)(sp.knot_off[lo + 1] - sp.knot_off[lo]) - 4;
    const int l = find_span(k, n, x);
    double h[4], dh[4];
    bspline_basis<false>(k, l, x, h, dh);
    const double* c = sp.coefs + sp.coef_off[lo] + (l - 3);
#pragma unroll
    for (int q = 0; q < 4; ++q) { o0 = o0 + c[q] * h[q]; o1 = o1 + c[n + q] * h[q]; o2 = o2 + c[2 * n + q] * h[q]; }
  }
  X[i] = o0; X[nt + i] = o1; X[2 * nt + i] = o2;
}

// Cov X(t) per sample from band[N][4][3][3] (blocks (p, p + w) of the control points' covariance, p over all splines): one lane per
// sample, NaN outside every interval.  ctrl_off[s] = index of spline s' first control point.
__global__ __launch_bounds__(256) void k_spline_cov_eval(SplineSet sp, const long long* __restrict__ ctrl_off, const double* __restrict__ band, long long nt,
                                                         const double* __restrict__ t, double* __restrict__ cov, int32_t* __restrict__ which) {
  const long long i = blockIdx.x * 256ll + threadIdx.x;
  if (i >= nt) return;
  const double x = t[i];
  int lo = 0, hi = sp.S;
  while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (x >= sp.istart[mid]) lo = mid; else hi = mid; }
  const bool in = x >= sp.istart[lo] && x <= sp.iend[lo];
  which[i] = in ? lo : -1;
  double o[9];
  if (in) {
    const double* k = sp.knots + sp.knot_off[lo];
    const int n = (int)(sp.knot_off[lo + 1] - sp.knot_off[lo]) - 4;
    const int l = find_span(k, n, x);
    double h[4], dh[4];
    bspline_basis<false>(k, l, x, h, dh);
    cov_spline_sample(h, band + (ctrl_off[lo] + (l - 3)) * 36, o);
  } else {
#pragma unroll
    for (int e = 0; e < 9; ++e) o[e] = __builtin_nan("");
  }
#pragma unroll
  for (int e = 0; e < 9; ++e) cov[i * 9 + e] = o[e];
}

// ---- kinematics ------------------------------------------------------------------------------------------------------------------
// interval of x as k_spline_eval finds it (closed at both ends), -1 outside
__device__ __forceinline__ int spline_interval_of(const SplineSet& sp, double x) {
  int lo = 0, hi = sp.S;
  while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (x >= sp.istart[mid]) lo = mid; else hi = mid; }
  return x >= sp.istart[lo] && x <= sp.iend[lo] ? lo : -1;
}

// X, X', .., D^nder X per sample, D[(nder + 1)][3][nt]: one span search and one recurrence per lane; order 0 is k_spline_eval's sum
__global__ __launch_bounds__(256) void k_spline_eval_der(SplineSet sp, long long nt, const double* __restrict__ t, int nder, double* __restrict__ D,
                                                         int32_t* __restrict__ which) {
  const long long i = blockIdx.x * 256ll + threadIdx.x;
  if (i >= nt) return;
  const double x = t[i];
  const int s = spline_interval_of(sp, x);
  which[i] = s;
  double o[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (s >= 0) {
    const double* k = sp.knots + sp.knot_off[s];
    const int n = (int)(sp.knot_off[s + 1] - sp.knot_off[s]) - 4;
    const int l = find_span(k, n, x);
    double H[3][4];
    bspline_basis_d2(k, l, x, H[0], H[1], H[2]);
    const double* c = sp.coefs + sp.coef_off[s] + (l - 3);
#pragma unroll
    for (int v = 0; v < 3; ++v)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        o[3 * v + 0] = o[3 * v + 0] + c[q] * H[v][q]; o[3 * v + 1] = o[3 * v + 1] + c[n + q] * H[v][q]; o[3 * v + 2] = o[3 * v + 2] + c[2 * n + q] * H[v][q];
      }
  }
#pragma unroll
  for (int v = 0; v < 3; ++v)
    if (v <= nder) {
#pragma unroll
      for (int d = 0; d < 3; ++d) D[(3 * v + d) * nt + i] = o[3 * v + d];
    }
}

// Covariance of the state (X, .., D^NDER X) per sample, cov[nt][D][D] from band[N][4][3][3] (as k_spline_cov_eval): one lane per sample
// computes the upper triangle (kin_state_cov_tri); a lane's matrix lies D * D * 8 bytes (648 for NDER = 2) from its neighbour's, so the
// workgroup's triangles go through LDS ([entry][lane]: the lanes of a wavefront write one bank row) and its stretch of cov is written
// in order, every entry and its mirror image from the same LDS word.  NaN outside every interval.
template <int NDER>
__global__ __launch_bounds__(256) void k_spline_kin_cov_eval(SplineSet sp, const long long* __restrict__ ctrl_off, const double* __restrict__ band, long long nt,
                                                             const double* __restrict__ t, double* __restrict__ cov, int32_t* __restrict__ which) {
  constexpr int D = kin_dim(NDER), T = kin_tri_count(NDER);
  __shared__ double stage[T * 256];
  const long long base = blockIdx.x * 256ll, i = base + threadIdx.x;
  if (i < nt) {
    const double x = t[i];
    const int s = spline_interval_of(sp, x);
    which[i] = s;
    double tri[T];
    if (s >= 0) {
      const double* k = sp.knots + sp.knot_off[s];
      const int n = (int)(sp.knot_off[s + 1] - sp.knot_off[s]) - 4;
      const int l = find_span(k, n, x);
      double H[12];
      bspline_basis_d2(k, l, x, H, H + 4, H + 8);
      kin_state_cov_tri<NDER>(H, band + (ctrl_off[s] + (l - 3)) * 36, tri);
    } else {
#pragma unroll
      for (int e = 0; e < T; ++e) tri[e] = __builtin_nan("");
    }
#pragma unroll
    for (int e = 0; e < T; ++e) stage[e * 256 + threadIdx.x] = tri[e];
  }
  __syncthreads();
  const long long left = nt - base;
  const int cnt = (int)(left < 256 ? left : 256) * (D * D);          // doubles this workgroup owns, contiguous from cov + base * D * D
  double* out = cov + base * (D * D);
  for (int e = threadIdx.x; e < cnt; e += 256) {
    const int lane = e / (D * D), pq = e % (D * D), P = pq / D, Q = pq % D;
    out[e] = stage[(P <= Q ? kin_tri(D, P, Q) : kin_tri(D, Q, P)) * 256 + lane];
  }
}

// Path length, step 1: one lane per knot span (all splines one behind the other, span_off[s] = index of spline s' first span, n_s - 3 each):
// the length of the span's part inside the interval
__global__ __launch_bounds__(256) void k_span_length(SplineSet sp, const long long* __restrict__ span_off, double* __restrict__ len) {
  const long long g = blockIdx.x * 256ll + threadIdx.x;
  if (g >= span_off[sp.S]) return;
  int lo = 0, hi = sp.S;                              // last spline whose first span <= g
  while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (g >= span_off[mid]) lo = mid; else hi = mid; }
  const double* k = sp.knots + sp.knot_off[lo];
  const int n = (int)(sp.knot_off[lo + 1] - sp.knot_off[lo]) - 4;
  const int l = 3 + (int)(g - span_off[lo]);
  len[g] = kin_span_part(k, n, sp.coefs + sp.coef_off[lo], l, sp.istart[lo], sp.iend[lo], sp.iend[lo]);
}
// step 2: exclusive prefix sum of a spline's span lengths, in place, and the interval's length.  One wavefront per spline loads 64 spans
// at a time and every lane adds them up in the order of the spans (lane k's value broadcast at step k), keeping the total it saw before its
// own span: prefix[j + 1] = prefix[j] + len[j] to the bit, total = prefix[count] -- one fixed order, no atomics
__global__ __launch_bounds__(64) void k_span_prefix(int S, const long long* __restrict__ span_off, double* __restrict__ len, double* __restrict__ total) {
  const int s = blockIdx.x, lane = threadIdx.x;
  const long long b = span_off[s], cnt = span_off[s + 1] - b;
  double carry = 0.0;
  for (long long j0 = 0; j0 < cnt; j0 += 64) {
    const long long j = j0 + lane;
    const double v = j < cnt ? len[b + j] : 0.0;
    double before = 0.0;
#pragma unroll
    for (int k = 0; k < 64; ++k) {
      if (lane == k) before = carry;
      carry = carry + __shfl(v, k, 64);
    }
    if (j < cnt) len[b + j] = before;
  }
  if (lane == 0) total[s] = carry;
}
// step 3: one lane per sample: the spans before its own (the prefix) plus the part of its own span up to the sample
__global__ __launch_bounds__(256) void k_spline_length(SplineSet sp, const long long* __restrict__ span_off, const double* __restrict__ prefix, long long nt,
                                                       const double* __restrict__ t, double* __restrict__ dist, int32_t* __restrict__ which) {
  const long long i = blockIdx.x * 256ll + threadIdx.x;
  if (i >= nt) return;
  const double x = t[i];
  const int s = spline_interval_of(sp, x);
  which[i] = s;
  double d = 0.0;
  if (s >= 0) {
    const double* k = sp.knots + sp.knot_off[s];
    const int n = (int)(sp.knot_off[s + 1] - sp.knot_off[s]) - 4;
    const int l = find_span(k, n, x);
    d = prefix[span_off[s] + (l - 3)] + kin_span_part(k, n, sp.coefs + sp.coef_off[s], l, sp.istart[s], sp.iend[s], x);
  }
  dist[i] = d;
}

// ---- least squares on fixed knots ------------------------------------------------------------------------------------
// Normal equations in lower banded storage: G[j][w] = (B^T B)(j, j - w), w = 0..3;  rhs[d][j] = (B^T X_d)(j).
__global__ __launch_bounds__(256) void k_lsq_accumulate(const double* __restrict__ knots, int n, long long m, const double* __restrict__ t,
                                                        const double* __restrict__ X, double* __restrict__ G, double* __restrict__ rhs) {
  const long long i = blockIdx.x * 256ll + threadIdx.x;
  if (i >= m) return;
  const double x = t[i];
  const int l = find_span(knots, n, x);
  double h[4], dh[4];
  bspline_basis<false>(knots, l, x, h, dh);
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const int ja = l - 3 + a;
#pragma unroll
    for (int b = 0; b <= a; ++b) unsafeAtomicAdd(&G[4 * ja + (a - b)], h[a] * h[b]);
#pragma unroll
    for (int d = 0; d < 3; ++d) unsafeAtomicAdd(&rhs[(long long)d * n + ja], h[a] * X[(long long)d * m + i]);
  }
}

// banded Cholesky G = L L^T (L keeps the band) and the three solves, one wavefront: lanes 0..2 carry the three right-hand
// sides through the substitutions, the factorisation itself is a 4-wide recurrence done redundantly by every lane.
// A pivot that is not above kLsqPivotTol times its diagonal entry of G fails the fit: the entry is a sum of m squares accumulated in
// any order, so the pivot carries an error of about sqrt(m) eps times it (7e-13 at m = 1e7) and a smaller one cannot be told from the
// zero of a rank-deficient system (Schoenberg-Whitney violated although every coefficient has data) -- whose rounding residue is
// positive as often as not and used to pass.  A full-rank system with such a pivot would have no correct digit left either.
constexpr double kLsqPivotTol = 1e-12;
__global__ __launch_bounds__(64) void k_lsq_solve(int n, double* __restrict__ G, double* __restrict__ rhs, int* __restrict__ fail) {
  const int lane = threadIdx.x;
  // factorise in place: L(j, j-w) in G[4j + w]
  for (int j = 0; j < n; ++j) {
    double row[4];
#pragma unroll
    for (int w = 0; w < 4; ++w) row[w] = G[4 * j + w];
    // L(j, j-w) for w = 3, 2, 1, then the diagonal
#pragma unroll
    for (int w = 3; w >= 1; --w) {
      const int k = j - w;
      if (k < 0) { row[w] = 0.0; continue; }
      double v = row[w];
      // subtract sum over p < k of L(j,p) L(k,p), p >= j-3
#pragma unroll
      for (int u = w + 1; u <= 3; ++u) {           // p = j - u
        const int p = j - u;
        if (p >= 0) v -= row[u] * G[4 * k + (u - w)];
      }
      row[w] = v / G[4 * k];
    }
    const double diag = row[0];
    double d = row[0];
#pragma unroll
    for (int u = 1; u <= 3; ++u) if (j - u >= 0) d -= row[u] * row[u];
    if (!(d > kLsqPivotTol * diag)) { if (lane == 0) fail[0] = 1; d = 1.0; }
    row[0] = sqrt(d);
    __syncthreads();                                 // every lane computed the same row; one writes it
    if (lane == 0) {
#pragma unroll
      for (int w = 0; w < 4; ++w) G[4 * j + w] = row[w];
    }
    __syncthreads();
  }
  if (lane >= 3) return;
  double* b = rhs + (long long)lane * n;
  for (int j = 0; j < n; ++j) {                      // L y = b
    double v = b[j];
#pragma unroll
    for (int u = 1; u <= 3; ++u) if (j - u >= 0) v -= G[4 * j + u] * b[j - u];
    b[j] = v / G[4 * j];
  }
  for (int j = n - 1; j >= 0; --j) {                 // L^T c = y
    double v = b[j];
#pragma unroll
    for (int u = 1; u <= 3; ++u) if (j + u < n) v -= G[4 * (j + u) + u] * b[j + u];
    b[j] = v / G[4 * j];
  }
}
#endif

}  // namespace mvus
