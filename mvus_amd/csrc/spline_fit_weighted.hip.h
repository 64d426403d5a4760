// The passes of the weighted fit (FITPACK's w) that read the weights.
#pragma once
#include "ba_math.h"      // hip_runtime.h under hipcc
#include "spline_dd.h"
#include "spline_fit_passes.hip.h"      // kFitBlk

namespace mvus {

#if defined(__HIPCC__)

// ---- the weighted fit (FITPACK's w): the two passes that read the weights -------------------------------------------------------------
// block_sum, restated for k_fit_blocks_w: the same tree in the same order.  The compiler schedules k_fit_blocks differently once a second
// kernel instantiates the same block_sum (seen with tools/compare_device_code.py), and the unweighted fit keeps the device code it had.
template <int NV, int NT, class T>
__device__ __forceinline__ void block_sum_w(T (&v)[NV], T* lds) {
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
// k_fit_blocks of the weighted fit (FITPACK's w): the row of sample i is wt[i] h with right-hand side wt[i] x, both scaled before the
// products, as fppara does -- in the precision of the pass: one rounding each in fp64, exactly in double-double.  A kernel of its own and not a switch inside k_fit_blocks: a shared body does not compile
// to the device code the unweighted fit had.
template <class T, int NT>
__global__ __launch_bounds__(NT) void k_fit_blocks_w(long long m, const long long* __restrict__ first, const double* __restrict__ q,
                                                     const double* __restrict__ X, const double* __restrict__ wt, T* __restrict__ SB) {
  __shared__ T lds[kFitBlk * NT];
  const int sp = blockIdx.x;
  T v[kFitBlk];
#pragma unroll
  for (int k = 0; k < kFitBlk; ++k) v[k] = T(0.0);
  const long long span_lo = first[sp], span_hi = first[sp + 1];
  const long long per = (span_hi - span_lo + gridDim.y - 1) / gridDim.y;
  const long long lo = span_lo + per * blockIdx.y, hi = lo + per < span_hi ? lo + per : span_hi;
  for (long long i = lo + threadIdx.x; i < hi; i += NT) {
    const double wi = wt[i];
    T hw[4], xw[3];                                  // in T: one fp64 rounding each as fppara's in fp64, the exact products in double-double
#pragma unroll
    for (int a = 0; a < 4; ++a) hw[a] = num_prod(wi, q[4 * i + a], T());
#pragma unroll
    for (int d = 0; d < 3; ++d) xw[d] = num_prod(wi, X[(long long)d * m + i], T());
#pragma unroll
    for (int a = 0; a < 4; ++a) {
#pragma unroll
      for (int b = 0; b <= a; ++b) v[a * (a + 1) / 2 + b] += hw[a] * hw[b];
#pragma unroll
      for (int d = 0; d < 3; ++d) v[10 + 3 * a + d] += hw[a] * xw[d];
    }
  }
  block_sum_w<kFitBlk, NT, T>(v, lds);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < kFitBlk; ++k) SB[((long long)blockIdx.y * gridDim.x + sp) * kFitBlk + k] = v[k];
  }
}

// f_p of a least-squares pass of the weighted fit close to interpolation (2 ncoef > m, in double-double), formed as fppara forms it --
// from the factorisation, not from the coefficients: f_p = |w x|^2 - |y|^2 with L y = A^T (w x) the forward substitution k_band_solve<3, dd> leaves in its work array (count =
// 3 ncoef values) and bb = |w x|^2 from k_fit_wx2, once per session and only when such a pass comes.  Close to interpolation the least-squares coefficients of a
// direction the samples barely determine reach 1e13 (seed 6 of tests/test_gpu_weighted_fit.py at 339 knots for 349 samples): rounded to
// fp64 they no longer reproduce the residual (3e-5 relative in f_p, which the smoothing iteration starts from); y never sees them.
__global__ __launch_bounds__(256) void k_fit_wx2(long long m, const double* __restrict__ X, const double* __restrict__ wt, dd* __restrict__ bb) {
  __shared__ dd lds[256];
  dd v[1] = {dd(0.0)};
  for (long long i = threadIdx.x; i < 3 * m; i += 256) { const dd wx = dd_two_prod(wt[i % m], X[i]); v[0] += wx * wx; }
  block_sum_w<1, 256, dd>(v, lds);
  if (threadIdx.x == 0) bb[0] = v[0];
}
__global__ __launch_bounds__(256) void k_fit_fp_from_factor(int count, const dd* __restrict__ y, const dd* __restrict__ bb, double* __restrict__ out) {
  __shared__ dd lds[256];
  dd v[1] = {dd(0.0)};
  for (int i = threadIdx.x; i < count; i += 256) v[0] += y[i] * y[i];
  block_sum_w<1, 256, dd>(v, lds);
  if (threadIdx.x == 0) {
    const double f = to_double(bb[0] - v[0]);
    out[0] = f > 0.0 ? f : 0.0;
  }
}
// k_fit_residual of the weighted fit: term += (wt (fac - x))^2; q itself stays unweighted, as FITPACK stores it
__global__ __launch_bounds__(256) void k_fit_residual_w(long long m, int ncoef, const int32_t* __restrict__ span, const double* __restrict__ q,
                                                        const double* __restrict__ X, const double* __restrict__ wt, const double* __restrict__ c,
                                                        double* __restrict__ term) {
  const long long i = blockIdx.x * 256ll + threadIdx.x;
  if (i >= m) return;
  const int sp = span[i];
  const double wi = wt[i];
  double tsum = 0.0;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    double fac = 0.0;
#pragma unroll
    for (int a = 0; a < 4; ++a) fac = fac + c[(long long)d * ncoef + sp + a] * q[4 * i + a];
    const double r = wi * (fac - X[(long long)d * m + i]);
    tsum = tsum + r * r;
  }
  term[i] = tsum;
}
#endif

}  // namespace mvus
