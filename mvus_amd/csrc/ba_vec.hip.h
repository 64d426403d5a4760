// BLAS-1 on n- and m-sized device vectors: a x + b y, products, fills, the loss weights, and the deterministic two-stage dot
// product as kernels and as device functions.
#pragma once
#include <hip/hip_runtime.h>

#include "ba_dev_problem.h"      // kThreads, xcd_tile
#include "ba_math.h"             // LossSpec, loss_weight
#include "ba_wave.hip.h"         // wave_sum

namespace mvus {

// ---- small vector kernels (n- and m-sized) -------------------------------------------------------
__global__ void k_axpby(long long len, double a, const double* x, double b, const double* y, double* out) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < len; i += (long long)gridDim.x * blockDim.x)
    out[i] = a * x[i] + b * y[i];
}
__global__ void k_mul(long long len, const double* x, const double* y, double* out) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < len; i += (long long)gridDim.x * blockDim.x)
    out[i] = x[i] * y[i];
}
// grid = xcd_grid(tiles) workgroups; every pass of the grid-stride loop covers tiles * 256 consecutive elements, of which each
// XCD writes runs of consecutive 2 KB pieces (xcd_tile)
__global__ void k_fill(long long len, double v, double* out, int tiles) {
  const int t = xcd_tile(tiles);
  if (t >= tiles) return;
  for (long long i = t * (long long)blockDim.x + threadIdx.x; i < len; i += (long long)tiles * blockDim.x) out[i] = v;
}

// weights_out of mvus_ba_robust_cost: rho'((f_i / f_scale)^2) of every row
__global__ __launch_bounds__(kThreads) void k_loss_weights(long long m, const double* __restrict__ f, LossSpec loss, double* __restrict__ w) {
  const long long i = blockIdx.x * (long long)kThreads + threadIdx.x;
  if (i < m) w[i] = loss_weight(loss, f[i]);
}

// deterministic two-stage dot product: per-workgroup partials, then one workgroup sums them
__global__ __launch_bounds__(kThreads) void k_dot_partial(long long len, const double* __restrict__ a, const double* __restrict__ b,
                                                          double* __restrict__ partials) {
  __shared__ double red[kThreads / 64];
  double s = 0.0;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < len; i += (long long)gridDim.x * blockDim.x)
    s += a[i] * b[i];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int w = 0; w < kThreads / 64; ++w) t += red[w];
    partials[blockIdx.x] = t;
  }
}
__global__ __launch_bounds__(kThreads) void k_dot_final(int nb, const double* __restrict__ partials, double* __restrict__ out) {
  __shared__ double red[kThreads / 64];
  double s = 0.0;
  for (int i = threadIdx.x; i < nb; i += blockDim.x) s += partials[i];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int w = 0; w < kThreads / 64; ++w) t += red[w];
    *out = t;
  }
}

// the same two trees as device functions, for kernels that fold a sum into a pass of their own (ba_lsmr.hip.h)

__device__ __forceinline__ double dot_final_block(int nb, const double* __restrict__ partials) {     // k_dot_final's tree; blockDim.x == kThreads
  __shared__ double red_f[kThreads / 64];
  __shared__ double tot_f;
  double s = 0.0;
  for (int i = threadIdx.x; i < nb; i += kThreads) s += partials[i];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red_f[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int w = 0; w < kThreads / 64; ++w) t += red_f[w];
    tot_f = t;
  }
  __syncthreads();
  return tot_f;
}
__device__ __forceinline__ void dot_partial_store(double s, double* __restrict__ partials) {         // k_dot_partial's tree
  __shared__ double red_p[kThreads / 64];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red_p[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int w = 0; w < kThreads / 64; ++w) t += red_p[w];
    partials[blockIdx.x] = t;
  }
}

}  // namespace mvus
