// The one-chain band solvers of the spline fit: banded Cholesky with both substitutions on one wavefront, and the sum of the
// factor's diagonal in the natural order.
#pragma once
#include "ba_math.h"      // hip_runtime.h under hipcc
#include "spline_dd.h"

namespace mvus {

#if defined(__HIPCC__)

// Banded Cholesky M = L L^T (lower band, row stride 5, HB = 3 or 4 sub-diagonals used) and the solves for the three
// right-hand sides, ONE wavefront: every lane runs the factor recurrence (no exchange between lanes), the previous HB rows
// of L stay in registers, the next row of M is fetched while the current one is processed; lanes 0..2 carry one right-hand
// side each.  L (stride 5) and the solution go to Lout / c; out[0] = sum of the diagonal of L (FITPACK's sum of a(i,1)).
template <int HB, class T>
__global__ __launch_bounds__(64) void k_band_solve(int n, const T* __restrict__ M, const T* __restrict__ rhs, T* __restrict__ Lout, T* __restrict__ ywork,
                                                   double* __restrict__ c, double* __restrict__ out, int* __restrict__ fail) {
  const int lane = threadIdx.x;
  const int d = lane < 3 ? lane : 0;
  const T* bvec = rhs + (long long)d * n;
  T* yv = ywork + (long long)d * n;
  double* cv = c + (long long)d * n;
  T Lp[HB + 1][HB + 1];               // Lp[u][w] = L(j-u, j-u-w), u = 1..HB
  T yp[HB + 1];                       // yp[u] = y(j-u)
#pragma unroll
  for (int u2 = 0; u2 <= HB; ++u2) {
    yp[u2] = T(0.0);
#pragma unroll
    for (int w = 0; w <= HB; ++w) Lp[u2][w] = (w == 0) ? T(1.0) : T(0.0);
  }
  T nxt[HB + 1], nb = T(0.0);
#pragma unroll
  for (int w = 0; w <= HB; ++w) nxt[w] = n > 0 ? M[w] : T(0.0);
  nb = n > 0 ? bvec[0] : T(0.0);
  double dsum = 0.0, dmin = 1e300, dmax = 0.0;
  bool bad = false;
  for (int j = 0; j < n; ++j) {
    T row[HB + 1];
#pragma unroll
    for (int w = 0; w <= HB; ++w) row[w] = nxt[w];
    const T bj = nb;
    if (j + 1 < n) {
#pragma unroll
      for (int w = 0; w <= HB; ++w) nxt[w] = M[5 * (long long)(j + 1) + w];
      nb = bvec[j + 1];
    }
#pragma unroll
    for (int w = HB; w >= 1; --w) {                 // L(j, j-w)
      T v = row[w];
#pragma unroll
      for (int u2 = w + 1; u2 <= HB; ++u2) v -= row[u2] * Lp[w][u2 - w];
      row[w] = (j - w >= 0) ? v / Lp[w][0] : T(0.0);
    }
    // A pivot that cancels to (almost) nothing means a direction the samples do not determine: FITPACK's knot search does
    // produce such knot sets close to interpolation, its Givens triangle then holds a rounding-noise diagonal entry.  The
    // residual does not depend on how that direction is resolved (the normal equations are consistent), so the pivot is
    // floored instead of failing; the caller repeats an fp64 pass with floored pivots in double-double.
    const T floor_ = T(pivot_floor(T()) * to_double(row[0]));
    T dg = row[0];
#pragma unroll
    for (int u2 = 1; u2 <= HB; ++u2) dg -= row[u2] * row[u2];
    const bool lost = !(to_double(dg) > to_double(floor_));
    bad |= lost;
    dg = lost ? (is_positive(floor_) ? floor_ : T(1.0)) : dg;
    row[0] = num_sqrt(dg);
    const double dl = to_double(row[0]);
    dsum += dl; dmin = fmin(dmin, dl); dmax = fmax(dmax, dl);
    T y = bj;
#pragma unroll
    for (int u2 = 1; u2 <= HB; ++u2) y -= row[u2] * yp[u2];
    y /= row[0];
    if (lane == 0) {
#pragma unroll
      for (int w = 0; w <= HB; ++w) Lout[5 * (long long)j + w] = row[w];
    }
    if (lane < 3) yv[j] = y;
#pragma unroll
    for (int u2 = HB; u2 >= 2; --u2) {
      yp[u2] = yp[u2 - 1];
#pragma unroll
      for (int w = 0; w <= HB; ++w) Lp[u2][w] = Lp[u2 - 1][w];
    }
    yp[1] = y;
#pragma unroll
    for (int w = 0; w <= HB; ++w) Lp[1][w] = row[w];
  }
  if (lane == 0) { out[0] = dsum; out[2] = dmin; out[3] = dmax; if (bad) fail[0] = 1; }
  __syncthreads();                                   // Lout / y written by this wavefront are read back below
  __threadfence_block();
  // L^T c = y: c(j) = (y(j) - sum_u L(j+u, j) c(j+u)) / L(j,j)
  T Ln[HB + 1][HB + 1];               // Ln[u][w] = L(j+u, j+u-w)
  T cn[HB + 1];
#pragma unroll
  for (int u2 = 0; u2 <= HB; ++u2) {
    cn[u2] = T(0.0);
#pragma unroll
    for (int w = 0; w <= HB; ++w) Ln[u2][w] = T(0.0);
  }
  for (int j = n - 1; j >= 0; --j) {
    T row[HB + 1];
#pragma unroll
    for (int w = 0; w <= HB; ++w) row[w] = Lout[5 * (long long)j + w];
    T v = lane < 3 ? yv[j] : T(0.0);
#pragma unroll
    for (int u2 = 1; u2 <= HB; ++u2) v -= Ln[u2][u2] * cn[u2];
    v /= row[0];
    if (lane < 3) cv[j] = to_double(v);
#pragma unroll
    for (int u2 = HB; u2 >= 2; --u2) {
      cn[u2] = cn[u2 - 1];
#pragma unroll
      for (int w = 0; w <= HB; ++w) Ln[u2][w] = Ln[u2 - 1][w];
    }
    cn[1] = v;
#pragma unroll
    for (int w = 0; w <= HB; ++w) Ln[1][w] = row[w];
  }
}

template <class T>
struct PivotStats {
  double dsum = 0.0, dmin = 1e300, dmax = 0.0;
  bool bad = false;
  // dg = what is left of the diagonal entry `full` after the eliminations: the pivot (floored when lost to rounding, see k_band_solve)
  __device__ __forceinline__ T pivot(T dg, T full) {
    const T floor_ = T(pivot_floor(T()) * to_double(full));
    const bool lost = !(to_double(dg) > to_double(floor_));
    bad |= lost;
    dg = lost ? (is_positive(floor_) ? floor_ : T(1.0)) : dg;
    const T l = num_sqrt(dg);
    const double dl = to_double(l);
    dsum += dl; dmin = fmin(dmin, dl); dmax = fmax(dmax, dl);
    return l;
  }
};

// sum of diag(L) of the banded Cholesky in the NATURAL order (FITPACK's sum of a(i,1), the initial p of the smoothing
// iteration) -- the factor recurrence of k_band_solve alone, with reciprocal pivots; every lane fetches one row of a 64-row
// chunk (coalesced, the next chunk while this one is processed) and the rows are broadcast from the lanes' registers.
__device__ __forceinline__ double lane_value(double v, int lane) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), lane), __builtin_amdgcn_readlane(__double2loint(v), lane));
}
__device__ __forceinline__ dd lane_value(dd v, int lane) { return dd(lane_value(v.hi, lane), lane_value(v.lo, lane)); }
template <int HB, class T>
__global__ __launch_bounds__(64) void k_band_diag_sum(int n, const T* __restrict__ M, double* __restrict__ out) {
  const int lane = threadIdx.x;
  T Lp[HB + 1][HB + 1], ip[HB + 1];
#pragma unroll
  for (int u = 0; u <= HB; ++u) {
    ip[u] = T(1.0);
#pragma unroll
    for (int w = 0; w <= HB; ++w) Lp[u][w] = (w == 0) ? T(1.0) : T(0.0);
  }
  PivotStats<T> ps;
  T cur[HB + 1], nxt[HB + 1];
#pragma unroll
  for (int w = 0; w <= HB; ++w) { cur[w] = lane < n ? M[5 * (long long)lane + w] : T(0.0); nxt[w] = T(0.0); }
  for (int base = 0; base < n; base += 64) {
    if (base + 64 + lane < n) {
#pragma unroll
      for (int w = 0; w <= HB; ++w) nxt[w] = M[5 * (long long)(base + 64 + lane) + w];
    }
    const int cnt = n - base < 64 ? n - base : 64;
    for (int k = 0; k < cnt; ++k) {
      T row[HB + 1];
#pragma unroll
      for (int w = 0; w <= HB; ++w) row[w] = lane_value(cur[w], k);
#pragma unroll
      for (int w = HB; w >= 1; --w) {
        T v = row[w];
#pragma unroll
        for (int u2 = w + 1; u2 <= HB; ++u2) v -= row[u2] * Lp[w][u2 - w];
        row[w] = (base + k - w >= 0) ? v * ip[w] : T(0.0);
      }
      const T full = row[0];
      T dg = row[0];
#pragma unroll
      for (int u2 = 1; u2 <= HB; ++u2) dg -= row[u2] * row[u2];
      row[0] = ps.pivot(dg, full);
#pragma unroll
      for (int u2 = HB; u2 >= 2; --u2) {
        ip[u2] = ip[u2 - 1];
#pragma unroll
        for (int w = 0; w <= HB; ++w) Lp[u2][w] = Lp[u2 - 1][w];
      }
      ip[1] = num_recip(row[0]);
#pragma unroll
      for (int w = 0; w <= HB; ++w) Lp[1][w] = row[w];
    }
#pragma unroll
    for (int w = 0; w <= HB; ++w) cur[w] = nxt[w];
  }
  if (lane == 0) out[0] = ps.dsum;
}
#endif

}  // namespace mvus
