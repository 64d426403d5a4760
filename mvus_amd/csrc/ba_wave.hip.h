// Wavefront-level primitives of the Schur kernels: the accumulator type of the fp64 matrix cores, the one-wavefront LDS fence,
// lane broadcasts, and the register L D L^T of a 16 x 16 block (the Gauss-Jordan pivot and the blocked L D L^T both use it).
// The wave_sum* family lives in ba_kernels.hip.h.
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

}  // namespace mvus
