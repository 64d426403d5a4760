// Wavefront-level primitives of the BA kernels: wavefront sums and maxima (shuffle and DPP forms), the LDS-only workgroup barrier,
// the last-workgroup ticket, the accumulator type of the fp64 matrix cores, the one-wavefront LDS fence, lane broadcasts, and the
// register L D L^T of a 16 x 16 block (the Gauss-Jordan pivot and the blocked L D L^T both use it).
#pragma once
#include <hip/hip_runtime.h>

namespace mvus {

using d4 = __attribute__((ext_vector_type(4))) double;      // four doubles per lane: a 16 x 16 fp64 matrix-core accumulator

__device__ __forceinline__ void lds_wave_sync() {      // orders the LDS traffic of ONE wavefront (writes of some lanes read by others)
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront", "local");
}

__device__ __forceinline__ int wave_min_i(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = min(v, __shfl_down(v, off, 64));
  return v;
}

__device__ __forceinline__ double bcast_lane(double v, int src) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), src);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), src);
  return __hiloint2double(hi, lo);
}

// lane J of every row of 16 lanes, to all lanes of that row (v_mov_b64_dpp row_newbcast:J -- the one DPP control 64-bit operands have here)
template <int J> __device__ __forceinline__ double row_bcast(double v) { return __builtin_amdgcn_update_dpp(v, v, 0x150 + J, 0xf, 0xf, false); }

// L D L^T of a 16x16 SPD block, every row of 16 lanes on its own copy: lane i of the row holds row i of the block (a, lower
// triangle) and row i of the identity (x).  Column operations col_j -= col_k * (a_jk / d_k) on both: on return x[k] of lane c is
// X[k][c] = (L^-1)[k][c] (unit lower, zero above) and rd[k] = 1 / d_k in every lane, so that block^-1 = X^T diag(rd) X.  No square
// root.  The multiplier A[j][k] comes from lane j by DPP (v_mov_b64_dpp row_newbcast:j -- the one DPP control 64-bit operands have
// on this part): a vector move per multiplier instead of two v_readlane through an SGPR pair with its wait states, which is what
// the 16-column chain was made of (tools/micro/ldl16_bench.hip: cycles of the two forms on one wavefront).  One basic block.
template <int K, int J> struct LdlColOps {
  static __device__ __forceinline__ void run(double (&a)[16], double (&x)[16], double ta, double tx) {
    const double m = row_bcast<J>(a[K]);
    a[J] -= ta * m;
    x[J] -= tx * m;
    LdlColOps<K, J + 1>::run(a, x, ta, tx);
  }
};
template <int K> struct LdlColOps<K, 16> { static __device__ __forceinline__ void run(double (&)[16], double (&)[16], double, double) {} };
template <int K> struct LdlCols {
  static __device__ __forceinline__ void run(double (&a)[16], double (&x)[16], double (&rd)[16], bool& bad) {
    double d = row_bcast<K>(a[K]);
    bad |= !(d > 0.0);
    d = d > 0.0 ? d : 1.0;
    double r = __builtin_amdgcn_rcp(d);
    r = r * (2.0 - d * r);
    r = r * (2.0 - d * r);
    rd[K] = r;
    LdlColOps<K, K + 1>::run(a, x, a[K] * r, x[K] * r);
    LdlCols<K + 1>::run(a, x, rd, bad);
  }
};
template <> struct LdlCols<16> { static __device__ __forceinline__ void run(double (&)[16], double (&)[16], double (&)[16], bool&) {} };
__device__ __forceinline__ void ldl_inv16(double (&a)[16], double (&x)[16], double (&rd)[16], int lane, int* __restrict__ fail) {
  bool bad = false;
  LdlCols<0>::run(a, x, rd, bad);
  if (bad && lane == 0) fail[0] = 2;
}

// Workgroup barrier that orders LDS traffic only.  __syncthreads() also waits for every outstanding global load
// (vmcnt(0): gfx9 counts loads and stores together), which defeats prefetching across a barrier; kernels that keep
// global loads in flight over LDS-only phases use this instead.  Global data written before it is NOT made visible.
__device__ __forceinline__ void lds_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}
// wave_sum's tree for callers that read the total from lane 0 only: the two steps that cross 16-lane rows go through the LDS
// crossbar like __shfl_down, the four inside row 0 are DPP row shifts (no LDS trip).  Lane 0 holds the same bits as wave_sum's.
__device__ __forceinline__ double wave_sum_lane0(double v);
// The same reductions on the DPP data path (VALU lane shifts inside 16-lane rows, then the two row broadcasts): no trip through
// the LDS crossbar per step.  With 16 wavefronts of one workgroup each reducing five values, the ds_bpermute version of
// k_lm_trial spent 21-25 k cycles in its reductions (MVUS_TRIAL_PROBE); the summation tree differs from wave_sum's, so these are
// used by the LM driver's kernels only, not by anything the TRF + LSMR parity path sums.  Result valid in every lane.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_shift(double v, double fill) {
  const int lo = __builtin_amdgcn_update_dpp(__double2loint(fill), __double2loint(v), CTRL, ROW_MASK, 0xF, false);
  const int hi = __builtin_amdgcn_update_dpp(__double2hiint(fill), __double2hiint(v), CTRL, ROW_MASK, 0xF, false);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double wave_sum_lane0(double v) {
  v += __shfl_down(v, 32, 64);
  v += __shfl_down(v, 16, 64);
  v += dpp_shift<0x108, 0xF>(v, 0.0);      // row_shl:8
  v += dpp_shift<0x104, 0xF>(v, 0.0);      // row_shl:4
  v += dpp_shift<0x102, 0xF>(v, 0.0);      // row_shl:2
  v += dpp_shift<0x101, 0xF>(v, 0.0);      // row_shl:1
  return v;
}
__device__ __forceinline__ double wave_sum_dpp(double v) {
  v += dpp_shift<0x111, 0xF>(v, 0.0);      // row_shr:1
  v += dpp_shift<0x112, 0xF>(v, 0.0);      // row_shr:2
  v += dpp_shift<0x114, 0xF>(v, 0.0);      // row_shr:4
  v += dpp_shift<0x118, 0xF>(v, 0.0);      // row_shr:8   -> lane 15 of every row holds the row's sum
  v += dpp_shift<0x142, 0xA>(v, 0.0);      // row_bcast:15 into rows 1 and 3
  v += dpp_shift<0x143, 0xC>(v, 0.0);      // row_bcast:31 into rows 2 and 3 -> lane 63 holds the total
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), 63), hi = __builtin_amdgcn_readlane(__double2hiint(v), 63);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double wave_max_dpp(double v) {       // for values >= 0 (fill 0)
  v = fmax(v, dpp_shift<0x111, 0xF>(v, 0.0));
  v = fmax(v, dpp_shift<0x112, 0xF>(v, 0.0));
  v = fmax(v, dpp_shift<0x114, 0xF>(v, 0.0));
  v = fmax(v, dpp_shift<0x118, 0xF>(v, 0.0));
  v = fmax(v, dpp_shift<0x142, 0xA>(v, 0.0));
  v = fmax(v, dpp_shift<0x143, 0xC>(v, 0.0));
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), 63), hi = __builtin_amdgcn_readlane(__double2hiint(v), 63);
  return __hiloint2double(hi, lo);
}

// True in every thread of the last workgroup of the grid to get here (ticket from an atomic counter, which that workgroup resets):
// it may then read what all the others wrote before their call.
__device__ __forceinline__ bool last_block_done(unsigned* counter) {
  __shared__ bool last_s;
  __threadfence();
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned ticket = atomicAdd(counter, 1u);
    last_s = ticket == gridDim.x - 1;
    if (last_s) *counter = 0u;
  }
  __syncthreads();
  if (last_s) __threadfence();
  return last_s;
}

}  // namespace mvus
