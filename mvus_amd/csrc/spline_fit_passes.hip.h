// The smoothing fit's passes over samples and spans: the size rules (host), basis, span blocks, band assembly, penalty, combine,
// residual, per-span and total sums.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "ba_math.h"      // MVUS_HD, bspline_basis
#include "spline_band_parts.h"
#include "spline_dd.h"      // num_prod

namespace mvus {

constexpr int kFitBlk = 22;      // per span: 10 products h_a h_b (a >= b) + 12 products h_a x_d
// A span with many samples (the first passes of a fit: ONE span holds all 3.3 M samples of a long trajectory) is cut into
// gridDim.y slices, one workgroup each; slice `sl` of span `sp` goes to block sl * nspan + sp of SB and k_fit_slice_sum adds the
// slices in their order.  fit_slices() picks the count from the number of spans alone, so the order of every sum is fixed.
inline int fit_slices(int nspan) {
  static const int cap = [] { const char* e = std::getenv("MVUS_FIT_SLICES_MAX"); return e ? std::max(1, std::min(256, std::atoi(e))) : 256; }();
  return nspan >= 512 ? 1 : std::min(cap, (1024 + nspan - 1) / nspan);
}
constexpr int kFitSliceBlocks = 1536;              // nspan * fit_slices(nspan) - nspan stays below this
// the total f_p of m > kFitTotalOneStage samples takes two stages: this many workgroups of k_fit_total_partial, then k_fit_total
constexpr long long kFitTotalOneStage = 8192;
constexpr int kFitTotalParts = 1024;               // the size of tot_part
inline int fit_total_parts(long long m) { return (int)std::min<long long>(kFitTotalParts, (m + 2047) / 2048); }
// an explicit slice count (the inspection entry points): the blocks of SB and the partial sums of fp_part it writes fit what the fit allocates
inline bool fit_slices_legal(int nspan, int slices) {
  return slices >= 1 && slices <= 256 && (long long)nspan * (slices - 1) <= kFitSliceBlocks && (slices == 1 || (long long)nspan * slices <= 512 + kFitSliceBlocks);
}
// What the inspection entry points of the fit's passes accept as samples and knots: m > 3 strictly increasing finite u, n >= 8 knots with
// u[0] / u[m-1] four times at the ends, interior knots strictly increasing inside (u[0], u[m-1]), and no span without a sample (fppara
// cannot produce one -- every interior knot it places is a sample and opens its span -- so the half / half rule has no contract there).
// Returns NULL, or what is wrong.
inline const char* fit_samples_knots_wrong(long long m, const double* u, int n, const double* t) {
  if (m <= 3 || m > (1ll << 30) || !u || !t) return "m > 3 samples and a knot vector";
  if (n < 8 || n > m + 4) return "8 <= n <= m + 4 knots";
  for (long long i = 0; i < m; ++i) if (!std::isfinite(u[i])) return "non-finite timestamp";
  for (long long i = 1; i < m; ++i) if (!(u[i] > u[i - 1])) return "the timestamps must be strictly increasing";
  for (int j = 0; j < n; ++j) if (!std::isfinite(t[j])) return "non-finite knot";
  for (int j = 0; j < 4; ++j) if (t[j] != u[0] || t[n - 1 - j] != u[m - 1]) return "the boundary knots must be u[0] and u[m-1], four times each";
  for (int j = 4; j <= n - 4; ++j) if (!(t[j] > t[j - 1])) return "the interior knots must be strictly increasing inside (u[0], u[m-1])";
  long long i = 0;                                   // every span [t[3 + sp], t[4 + sp]) holds a sample (the last one: its right end too)
  for (int sp = 0; sp + 8 <= n; ++sp) {
    while (i < m && u[i] < t[3 + sp]) ++i;
    if (i >= m || (sp + 8 < n && !(u[i] < t[4 + sp]))) return "a span without a sample";
  }
  return nullptr;
}
#if defined(__HIPCC__)

__global__ __launch_bounds__(256) void k_fit_basis(long long m, const double* __restrict__ u, const double* __restrict__ t, int ncoef,
                                                   int32_t* __restrict__ span, double* __restrict__ q) {
  const long long i = blockIdx.x * 256ll + threadIdx.x;
  if (i >= m) return;
  const double x = u[i];
  const int l = find_span(t, ncoef, x);
  double h[4], dh[4];
  bspline_basis<false>(t, l, x, h, dh);
  span[i] = l - 3;
#pragma unroll
  for (int a = 0; a < 4; ++a) q[4 * i + a] = h[a];
}

// first sample of every span (samples are sorted): first[sp] = lower_bound(u, t[3 + sp]), first[nspan] = m
__global__ __launch_bounds__(256) void k_fit_first(long long m, const double* __restrict__ u, const double* __restrict__ t, int nspan,
                                                   long long* __restrict__ first) {
  const int sp = blockIdx.x * 256 + threadIdx.x;
  if (sp > nspan) return;
  if (sp == nspan) { first[sp] = m; return; }
  if (sp == 0) { first[0] = 0; return; }
  const double knot = t[3 + sp];
  long long lo = 0, hi = m;                          // first index with u >= knot
  while (lo < hi) { const long long mid = (lo + hi) >> 1; if (u[mid] < knot) lo = mid + 1; else hi = mid; }
  first[sp] = lo;
}

// fixed-order sum of NV values per thread over one workgroup of NT -> thread 0 holds the result in v[]
template <int NV, int NT = 256, class T = double>
__device__ __forceinline__ void block_sum(T (&v)[NV], T* lds) {
  const int tid = threadIdx.x;
  __syncthreads();
#pragma unroll
  for (int k = 0; k < NV; ++k) lds[k * NT + tid] = v[k];
  __syncthreads();
  for (int off = NT / 2; off > 0; off >>= 1) {
    if (tid < off) {
#pragma unroll
      for (int k = 0; k < NV; ++k) lds[k * NT + tid] = lds[k * NT + tid] + lds[k * NT + tid + off];
    }
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < NV; ++k) v[k] = lds[k * NT];
}

// one workgroup per (span, slice): see fit_slices above
template <class T, int NT>
__global__ __launch_bounds__(NT) void k_fit_blocks(long long m, const long long* __restrict__ first, const double* __restrict__ q,
                                                   const double* __restrict__ X, T* __restrict__ SB) {
  __shared__ T lds[kFitBlk * NT];
  const int sp = blockIdx.x;
  T v[kFitBlk];
#pragma unroll
  for (int k = 0; k < kFitBlk; ++k) v[k] = T(0.0);
  const long long span_lo = first[sp], span_hi = first[sp + 1];
  const long long per = (span_hi - span_lo + gridDim.y - 1) / gridDim.y;
  const long long lo = span_lo + per * blockIdx.y, hi = lo + per < span_hi ? lo + per : span_hi;
  for (long long i = lo + threadIdx.x; i < hi; i += NT) {
    double h[4], x[3];
#pragma unroll
    for (int a = 0; a < 4; ++a) h[a] = q[4 * i + a];
#pragma unroll
    for (int d = 0; d < 3; ++d) x[d] = X[(long long)d * m + i];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
#pragma unroll
      for (int b = 0; b <= a; ++b) v[a * (a + 1) / 2 + b] += num_prod(h[a], h[b], T());
#pragma unroll
      for (int d = 0; d < 3; ++d) v[10 + 3 * a + d] += num_prod(h[a], x[d], T());
    }
  }
  block_sum<kFitBlk, NT, T>(v, lds);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < kFitBlk; ++k) SB[((long long)blockIdx.y * gridDim.x + sp) * kFitBlk + k] = v[k];
  }
}

// the slices of k_fit_blocks added up in their order, into slice 0 (count = nspan * kFitBlk values per slice)
template <class T>
__global__ __launch_bounds__(256) void k_fit_slice_sum(long long count, int nslice, T* __restrict__ SB) {
  const long long e = blockIdx.x * 256ll + threadIdx.x;
  if (e >= count) return;
  T v = SB[e];
#pragma unroll 8
  for (int sl = 1; sl < nslice; ++sl) v += SB[(long long)sl * count + e];
  SB[e] = v;
}

// row j of the normal equations (g[w] = M(j, j - w), w < 4) and of the right-hand sides into the copy k_band_solve_parts<3> reads
// (see BandParts::at); separator rows have no place there
template <class T>
__device__ __forceinline__ void band_parts_scatter(const BandParts& bp, int j, const T* g, const T* r, T* __restrict__ Mt, T* __restrict__ rt) {
  int p, i;
  bp.locate(j, p, i);
  if (i < bp.length(p)) {
#pragma unroll
    for (int w = 0; w < 4; ++w) Mt[bp.at(p, i, w, 4)] = g[w];
#pragma unroll
    for (int d = 0; d < 3; ++d) rt[bp.at(p, i, d, 3)] = r[d];
  }
}

// lower banded storage, width W = HB + 1: G[j * W + w] = M(j, j - w).  Here the normal equations in a width-5 array (w = 4
// zero) so that the penalty can be added in place, and rhs[d * ncoef + j].
template <class T>
__global__ __launch_bounds__(256) void k_fit_band(int ncoef, int nspan, const T* __restrict__ SB, T* __restrict__ G5, T* __restrict__ rhs, BandParts bp,
                                                  T* __restrict__ Mt, T* __restrict__ rt) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= ncoef) return;
  T g[5] = {T(0.0), T(0.0), T(0.0), T(0.0), T(0.0)}, r[3] = {T(0.0), T(0.0), T(0.0)};
  for (int sp = max(0, j - 3); sp <= min(nspan - 1, j); ++sp) {          // spans whose four coefficients include j
    const int a = j - sp;
    const T* blk = SB + (long long)sp * kFitBlk;
#pragma unroll
    for (int w = 0; w < 4; ++w) if (a - w >= 0) g[w] += blk[a * (a + 1) / 2 + (a - w)];
#pragma unroll
    for (int d = 0; d < 3; ++d) r[d] += blk[10 + 3 * a + d];
  }
#pragma unroll
  for (int w = 0; w < 5; ++w) G5[5 * (long long)j + w] = g[w];
#pragma unroll
  for (int d = 0; d < 3; ++d) rhs[(long long)d * ncoef + j] = r[d];
  if (bp.P > 1) band_parts_scatter(bp, j, g, r, Mt, rt);
}
// the same copy from a system that is already in G5 / rhs (mvus_spline_band_solve with hb = 3: no span blocks to feed k_fit_band)
template <class T>
__global__ __launch_bounds__(256) void k_band_scatter(int ncoef, const T* __restrict__ G5, const T* __restrict__ rhs, BandParts bp, T* __restrict__ Mt,
                                                      T* __restrict__ rt) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= ncoef) return;
  T g[4], r[3];
#pragma unroll
  for (int w = 0; w < 4; ++w) g[w] = G5[5 * (long long)j + w];
#pragma unroll
  for (int d = 0; d < 3; ++d) r[d] = rhs[(long long)d * ncoef + j];
  band_parts_scatter(bp, j, g, r, Mt, rt);
}

// BtB[j * 5 + w] = (B^T B)(j, j - w) for the n8 x ncoef jump matrix B whose row `it` holds b[it * 5 + c] in column it + c
template <class T>
__global__ __launch_bounds__(256) void k_fit_penalty(int ncoef, int n8, const double* __restrict__ b, T* __restrict__ BtB) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= ncoef) return;
  T g[5] = {T(0.0), T(0.0), T(0.0), T(0.0), T(0.0)};
  for (int it = max(0, j - 4); it <= min(n8 - 1, j); ++it) {
    const int cj = j - it;
#pragma unroll
    for (int w = 0; w < 5; ++w) if (cj - w >= 0) g[w] += num_prod(b[5 * (long long)it + cj], b[5 * (long long)it + cj - w], T());
  }
#pragma unroll
  for (int w = 0; w < 5; ++w) BtB[5 * (long long)j + w] = g[w];
}

template <class T>
__global__ __launch_bounds__(256) void k_fit_combine(long long count, const T* __restrict__ G5, const T* __restrict__ BtB, double pinv, T* __restrict__ M,
                                                     int ncoef, const T* __restrict__ rhs, BandParts bp, T* __restrict__ Mt, T* __restrict__ rt) {
  const long long e = blockIdx.x * 256ll + threadIdx.x;
  if (e >= count) return;
  const T v = G5[e] + (T(pinv) * T(pinv)) * BtB[e];                  // fppara rotates the rows of B in with weight 1/p
  M[e] = v;
  if (bp.P > 1) {                                    // the copy k_band_solve_parts<4> reads, and the right-hand sides in ITS partition
    const int j = (int)(e / 5), w = (int)(e - 5ll * j);
    int p, i;
    bp.locate(j, p, i);
    if (i < bp.length(p)) {
      Mt[bp.at(p, i, w, 5)] = v;
      if (w < 3) rt[bp.at(p, i, w, 3)] = rhs[(long long)w * ncoef + j];
    }
  }
}

// squared residual of every sample, in fppara's order of operations (fac = sum_j c(j) q(it, j); term += (fac - x)^2)
__global__ __launch_bounds__(256) void k_fit_residual(long long m, int ncoef, const int32_t* __restrict__ span, const double* __restrict__ q,
                                                      const double* __restrict__ X, const double* __restrict__ c, double* __restrict__ term) {
  const long long i = blockIdx.x * 256ll + threadIdx.x;
  if (i >= m) return;
  const int sp = span[i];
  double tsum = 0.0;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    double fac = 0.0;
#pragma unroll
    for (int a = 0; a < 4; ++a) fac = fac + c[(long long)d * ncoef + sp + a] * q[4 * i + a];
    const double r = fac - X[(long long)d * m + i];
    tsum = tsum + r * r;
  }
  term[i] = tsum;
}

// per-span residual: the first sample of a span (it is the first with u >= the knot that opens the span) is shared half / half
// with the span before, like fppara's `new` / `store` bookkeeping
// (gridDim.y slices per span as in k_fit_blocks: with more than one, the slice sums go to part[sl * nspan + sp] and
// k_fit_fpint_final adds them in order)
__global__ __launch_bounds__(256) void k_fit_fpint(int nspan, const long long* __restrict__ first, const double* __restrict__ term, double* __restrict__ fpint,
                                                   double* __restrict__ part) {
  __shared__ double lds[256];
  const int sp = blockIdx.x;
  const long long a = first[sp], b = first[sp + 1];
  const long long span_lo = a + (sp > 0 ? 1 : 0);
  const long long per = (b - span_lo + gridDim.y - 1) / gridDim.y;
  const long long lo = span_lo + per * blockIdx.y, hi = lo + per < b ? lo + per : b;
  double v[1] = {0.0};
  for (long long i = lo + threadIdx.x; i < hi; i += 256) v[0] += term[i];
  block_sum<1>(v, lds);
  if (threadIdx.x == 0) {
    if (gridDim.y > 1) { part[(long long)blockIdx.y * nspan + sp] = v[0]; return; }
    double s = v[0];
    if (sp > 0 && a < b) s += 0.5 * term[a];
    if (sp + 1 < nspan && first[sp + 1] < first[sp + 2]) s += 0.5 * term[b];
    fpint[sp] = s;
  }
}
__global__ __launch_bounds__(256) void k_fit_fpint_final(int nspan, int nslice, const long long* __restrict__ first, const double* __restrict__ term,
                                                         const double* __restrict__ part, double* __restrict__ fpint) {
  const int sp = blockIdx.x * 256 + threadIdx.x;
  if (sp >= nspan) return;
  const long long a = first[sp], b = first[sp + 1];
  double s = 0.0;
  for (int sl = 0; sl < nslice; ++sl) s += part[(long long)sl * nspan + sp];
  if (sp > 0 && a < b) s += 0.5 * term[a];
  if (sp + 1 < nspan && first[sp + 1] < first[sp + 2]) s += 0.5 * term[b];
  fpint[sp] = s;
}

// total of `count` values in a fixed order: per-workgroup partial sums (grid-stride), then one workgroup over the partials
// (k_fit_total with `count` = the number of partials).  One workgroup over 550k samples took 517 us a pass -- 65 % of a fit.
__global__ __launch_bounds__(256) void k_fit_total_partial(long long count, const double* __restrict__ v_in, double* __restrict__ part) {
  __shared__ double lds[256];
  double v[1] = {0.0};
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < count; i += (long long)gridDim.x * 256) v[0] += v_in[i];
  block_sum<1>(v, lds);
  if (threadIdx.x == 0) part[blockIdx.x] = v[0];
}
__global__ __launch_bounds__(256) void k_fit_total(long long count, const double* __restrict__ v_in, double* __restrict__ out) {
  __shared__ double lds[256];
  double v[1] = {0.0};
  for (long long i = threadIdx.x; i < count; i += 256) v[0] += v_in[i];
  block_sum<1>(v, lds);
  if (threadIdx.x == 0) out[0] = v[0];
}
#endif

}  // namespace mvus
