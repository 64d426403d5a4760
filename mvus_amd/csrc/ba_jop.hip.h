// The Jacobian as an operator on the stored chunk-major blocks: y = J v and the deterministic two-pass z = J^T u, detection and
// motion rows (what TRF + LSMR multiplies with).
#pragma once
#include <hip/hip_runtime.h>

#include "ba_dev_problem.h"
#include "ba_math.h"          // ChunkInfo
#include "ba_wave.hip.h"      // wave_sum_lane0

namespace mvus {

// y = J v on the detection rows.  Camera/sync entries of v are staged in LDS once per workgroup.
// row j of the motion regulariser times v
__device__ __forceinline__ double motion_row_times(const DevProblem& dp, const double* __restrict__ mJ, const int32_t* __restrict__ mctrl,
                                                   const double* __restrict__ v, int j) {
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int g = mctrl[(long long)k * dp.T + j];
    if (g < 0) continue;
    const int x0 = dp.mv.ctrl_x0[g], st = dp.mv.ctrl_stride[g];
    for (int q = 0; q < 4; ++q)
      for (int d = 0; d < 3; ++d) s += mJ[(long long)(12 * k + 3 * q + d) * dp.T + j] * v[x0 + q + d * st];
  }
  return s;
}
// (workgroups past xcd_grid(n_chunks), when mJ is given: the motion rows -- k_motion_jv beside the detection rows instead of
// after them: one launch less in every LSMR iteration of the default solver, which is launch bound at the reference's sizes)
template <int NS>
__global__ __launch_bounds__(kThreads) void k_jv(DevProblem dp, const double* __restrict__ J, const int32_t* __restrict__ span,
                                                 const double* __restrict__ v, double* __restrict__ y, const double* __restrict__ mJ = nullptr,
                                                 const int32_t* __restrict__ mctrl = nullptr, double* __restrict__ ym = nullptr) {
  constexpr int B = NS - 12;
  __shared__ double vc[B];
  if (mJ != nullptr && (int)blockIdx.x >= xcd_grid(dp.n_chunks)) {
    const int j = ((int)blockIdx.x - xcd_grid(dp.n_chunks)) * kThreads + threadIdx.x;
    if (j < dp.T) ym[j] = motion_row_times(dp, mJ, mctrl, v, j);
    return;
  }
    const int chunk = xcd_tile(dp.n_chunks);        // grid = xcd_grid(n_chunks): every XCD streams runs of consecutive chunks of J
  if (chunk >= dp.n_chunks) return;
  const int c = dp.chunk_cam[chunk];
  if (threadIdx.x < B) vc[threadIdx.x] = v[cam_col(dp.C, dp.P, c, threadIdx.x)];
  __syncthreads();
  if ((int)threadIdx.x >= dp.chunk_count[chunk]) return;
  const long long i = dp.chunk_start[chunk] + threadIdx.x;
  const long long a = dp.det_off[c], Mc = dp.det_off[c + 1] - a;
  const int g = span[i];
  const double* __restrict__ Jc = J + j_chunk_offset<NS>(chunk) + threadIdx.x;
  double sx = 0.0, sy = 0.0;
  if (g >= 0) {
#pragma unroll
    for (int k = 0; k < B; ++k) {
      sx += Jc[k * kThreads] * vc[k];
      sy += Jc[(NS + k) * kThreads] * vc[k];
    }
    const int x0 = dp.mv.ctrl_x0[g], st = dp.mv.ctrl_stride[g];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        const double vv = v[x0 + q + d * st];
        sx += Jc[(B + 3 * q + d) * kThreads] * vv;
        sy += Jc[(NS + B + 3 * q + d) * kThreads] * vv;
      }
  }
  y[2 * a + (i - a)] = sx;
  y[2 * a + Mc + (i - a)] = sy;
}

constexpr int kJtWin = 144;     // control points per chunk window of the J^T u gather

// ---- z = J^T u, DETERMINISTIC two-pass form (what the TRF + LSMR parity solver uses) ---------------------------------
// LSMR on these Jacobians amplifies last-bit differences of its products by ~10x every 1-2 iterations, so a J^T u whose
// fp64 atomics arrive in a different order on every run makes the whole optimiser irreproducible from run to run.  Here
// every output is written by exactly one thread that adds its contributions in a fixed order:
//   pass 1 (k_jtu_partial, one workgroup per chunk): the chunk's B camera sums and the sums of its control-point window
//          (the gather of k_jtu_gather) go to per-chunk buffers, nothing is added to z;
//   pass 2 (k_jtu_reduce, one thread per column of z): camera columns add their camera's chunks in order; a spline
//          column adds, camera by camera and chunk by chunk, the window entries that cover its control point, then the
//          motion rows that touch it (a contiguous row range known in advance).
// Chunks whose spans interleave (a large rolling-shutter coefficient) take an O(256) loop per output instead of the range
// tables -- still ordered; only a chunk whose detections spread over more than kJtWin control points (very sparse
// tracks) falls back to atomics, and raises *nondet so the caller can know.
template <int NS>
__global__ __launch_bounds__(kThreads) void k_jtu_partial(DevProblem dp, const double* __restrict__ J, const int32_t* __restrict__ span,
                                                          const double* __restrict__ u, double* __restrict__ z, double* __restrict__ zc,
                                                          double* __restrict__ zs, int32_t* __restrict__ zg0, int* __restrict__ nondet,
                                                          int32_t* __restrict__ zext = nullptr) {
  constexpr int B = NS - 12;
  constexpr int PS = kThreads + 1;
  __shared__ double part[kThreads / 64][B];
  __shared__ double prod[12 * PS];
  __shared__ int lo[kJtWin], hi[kJtWin], skey[kThreads];
  __shared__ int gmin_s[kThreads / 64];
  __shared__ int bad_s, wide_s, lmax_s;
    const int chunk = xcd_tile(dp.n_chunks);        // grid = xcd_grid(n_chunks): every XCD streams runs of consecutive chunks of J
  if (chunk >= dp.n_chunks) return;
  const ChunkInfo ci = dp.chunks[chunk];
  const bool active = (int)threadIdx.x < ci.count;
  const long long i = ci.start + (active ? threadIdx.x : 0);
  const long long a = ci.cam_start, Mc = ci.cam_count;
  const int g = active ? span[i] : -1;
  const double ux = g >= 0 ? u[2 * a + (i - a)] : 0.0;
  const double uy = g >= 0 ? u[2 * a + Mc + (i - a)] : 0.0;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const double* __restrict__ Jc = J + j_chunk_offset<NS>(chunk) + (active ? threadIdx.x : 0);
  for (int k = threadIdx.x; k < kJtWin; k += kThreads) { lo[k] = 0x7fffffff; hi[k] = 0; }
  if (threadIdx.x == 0) { bad_s = 0; wide_s = 0; lmax_s = -1; }
  skey[threadIdx.x] = g;
  int gm = g >= 0 ? g : 0x7fffffff;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) gm = min(gm, __shfl_xor(gm, off, 64));
  if (lane == 0) gmin_s[wave] = gm;
#pragma unroll
  for (int k = 0; k < B; ++k) {
    double val = 0.0;
    if (g >= 0) val = Jc[k * kThreads] * ux + Jc[(NS + k) * kThreads] * uy;
    val = wave_sum_lane0(val);
    if (lane == 0) part[wave][k] = val;
  }
  __syncthreads();
  int g0 = gmin_s[0];
#pragma unroll
  for (int w = 1; w < kThreads / 64; ++w) g0 = min(g0, gmin_s[w]);
  if (threadIdx.x < B) {
    double sacc = 0.0;
#pragma unroll
    for (int w = 0; w < kThreads / 64; ++w) sacc += part[w][threadIdx.x];
    zc[(long long)chunk * B + threadIdx.x] = sacc;
  }
  if (threadIdx.x == 0) { zg0[chunk] = g0; if (zext != nullptr && g0 == 0x7fffffff) zext[chunk] = 0; }
  double* zw = zs + (long long)chunk * (3 * kJtWin);
  if (g0 == 0x7fffffff) return;                       // nothing visible (uniform): pass 2 skips the chunk
  const int l = g - g0;
  double pv[12];
#pragma unroll
  for (int e = 0; e < 12; ++e) {
    pv[e] = g >= 0 ? Jc[(B + e) * kThreads] * ux + Jc[(NS + B + e) * kThreads] * uy : 0.0;
    prod[e * PS + threadIdx.x] = pv[e];
  }
  if (g >= 0) {
    if (l + 3 >= kJtWin) atomicOr(&wide_s, 1);
    else {
      // only the ends of a run of equal span can set the minimum / maximum of their span's index range (LDS atomics serialise
      // per address: a run of r detections cost 2 r of them, now 2)
      const int tid = threadIdx.x;
      if (tid == 0 || skey[tid - 1] != g) atomicMin(&lo[l], tid);
      if (tid == kThreads - 1 || skey[tid + 1] != g) { atomicMax(&hi[l], tid + 1); atomicMax(&lmax_s, l); }
    }
  }
  __syncthreads();
  // do the index ranges of consecutive non-empty spans overlap (detections not in span order)?  Each non-empty span looks for the
  // next one -- up to the last span in use only: scanning the empty tail of the 144-wide window took the last span's thread
  // ~60 dependent LDS reads, 15 of the kernel's 49 us
  if (threadIdx.x < kJtWin && hi[threadIdx.x] > 0) {
    const int last = lmax_s;
    for (int t = threadIdx.x + 1; t <= last; ++t)
      if (hi[t] > 0) { if (lo[t] < hi[threadIdx.x]) atomicOr(&bad_s, 1); break; }
  }
  __syncthreads();
  // how many control points of the window this chunk really reaches (k_jtu_index takes the maximum over the chunks: pass 2 then
  // looks only at chunks that can cover its control point instead of at all whose 144-wide window does)
  if (threadIdx.x == 0 && zext != nullptr) zext[chunk] = wide_s ? 0 : lmax_s + 4;
  if (wide_s) {                                        // detections spread over more control points than the window holds
    if (threadIdx.x == 0) { zg0[chunk] = 0x7fffffff; atomicAdd(nondet, 1); }
    if (g >= 0) {
      const int x0 = dp.mv.ctrl_x0[g], st = dp.mv.ctrl_stride[g];
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int d = 0; d < 3; ++d) unsafeAtomicAdd(&z[x0 + q + d * st], pv[3 * q + d]);
    }
    return;
  }
  for (int o = threadIdx.x; o < 3 * kJtWin; o += kThreads) {
    const int lc = o / 3, d = o % 3;
    double acc = 0.0;
    if (!bad_s) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int sidx = lc - q;
        if (sidx < 0) continue;
        const int b = lo[sidx], e = hi[sidx];
        for (int t = b; t < e; ++t) acc += prod[(3 * q + d) * PS + t];
      }
    } else {                                           // interleaved spans: every detection, in index order
      for (int t = 0; t < ci.count; ++t) {
        const int q = lc - (skey[t] - g0);
        if (skey[t] >= 0 && q >= 0 && q < 4) acc += prod[(3 * q + d) * PS + t];
      }
    }
    zw[o] = acc;
  }
}

// between the passes (one wavefront per camera): zfill[chunk] = running maximum of the window starts of the camera's chunks
// -- non-decreasing whatever the data, so pass 2 can binary-search it; chunks are time ordered, so zfill exceeds a
// chunk's own start by at most the few spans a rolling-shutter shift can reorder
// bounds[0] = max over the chunks of (running maximum - own window start): how far behind the running maximum a chunk can start;
// bounds[1] = max extent of a chunk's window in control points (zext).  Both zeroed by the caller before the launch.
__global__ __launch_bounds__(64) void k_jtu_index(DevProblem dp, const int32_t* __restrict__ zg0, int32_t* __restrict__ zfill,
                                                  const int32_t* __restrict__ zext = nullptr, int* __restrict__ bounds = nullptr) {
  const int c = blockIdx.x, lane = threadIdx.x;
  int carry = -0x7fffffff, slack = 0, ext = 0;
  for (int base = dp.cam_chunk_off[c]; base < dp.cam_chunk_off[c + 1]; base += 64) {
    const int ch = base + lane;
    const bool in = ch < dp.cam_chunk_off[c + 1];
    const int g0 = in ? zg0[ch] : 0x7fffffff;
    int v = g0 == 0x7fffffff ? -0x7fffffff : g0;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { const int o = __shfl_up(v, off, 64); if (lane >= off) v = max(v, o); }
    v = max(v, carry);
    if (in) zfill[ch] = v;
    if (in && g0 != 0x7fffffff) { slack = max(slack, v - g0); if (zext != nullptr) ext = max(ext, zext[ch]); }
    carry = __shfl(v, 63, 64);
  }
  if (bounds != nullptr) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { slack = max(slack, __shfl_xor(slack, off, 64)); ext = max(ext, __shfl_xor(ext, off, 64)); }
    if (lane == 0) { atomicMax(&bounds[0], slack); atomicMax(&bounds[1], ext); }
  }
}

// pass 2.  Blocks [0, C): the B camera columns of camera blockIdx.x, each summed over the camera's chunks in order.
// Blocks [C, ..): one wavefront per control point, lane = camera (cameras lane, lane + 64, ...): every lane adds, chunk by
// chunk, the window entries of its camera that cover the control point; the lanes are then combined by a butterfly whose
// pairing is fixed (the same bits every run), lane 0 adds the motion rows (a contiguous, precomputed row range) and writes z.
// first chunk of camera c whose running-max window start is within reach of control point g: what pass 2 finds by binary
// search.  It depends on the Jacobian's spans only, so a run of products with one Jacobian (LSMR) looks it up once.
// (win: no chunk reaches further than win control points past its window start -- kJtWin, or the measured bounds[1])
__device__ __forceinline__ int jtu_first_chunk(const DevProblem& dp, const int32_t* __restrict__ zfill, int c, int g, int win = kJtWin) {
  int lo = dp.cam_chunk_off[c], hi = dp.cam_chunk_off[c + 1];
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (zfill[mid] + win > g) hi = mid; else lo = mid + 1;
  }
  return lo;
}
__device__ __forceinline__ int jtu_window(const int* __restrict__ bounds) { return bounds != nullptr ? min(kJtWin, max(1, bounds[1])) : kJtWin; }
__global__ __launch_bounds__(kThreads) void k_jtu_first(DevProblem dp, const int32_t* __restrict__ zfill, int32_t* __restrict__ first,
                                                        const int* __restrict__ bounds = nullptr) {
  const long long e = blockIdx.x * (long long)kThreads + threadIdx.x;
  if (e >= (long long)dp.N * dp.C) return;
  first[e] = jtu_first_chunk(dp, zfill, (int)(e % dp.C), (int)(e / dp.C), jtu_window(bounds));
}
template <int NS>
__global__ __launch_bounds__(kThreads) void k_jtu_reduce(DevProblem dp, const double* __restrict__ zc, const double* __restrict__ zs,
                                                         const int32_t* __restrict__ zg0, const int32_t* __restrict__ zfill, const double* __restrict__ mJ,
                                                         const int32_t* __restrict__ mctrl, const double* __restrict__ um, int motion,
                                                         double* __restrict__ z, const int32_t* __restrict__ first = nullptr,
                                                         const int* __restrict__ bounds = nullptr) {
  constexpr int B = NS - 12;
  if ((int)blockIdx.x < dp.C) {
    const int c = blockIdx.x, k = threadIdx.x;
    if (k >= B) return;
    double acc = 0.0;
    // (sixteen loads in flight, then their adds in chunk order: the same sum, a sixteenth of the memory round trips)
    const int ch1 = dp.cam_chunk_off[c + 1];
    for (int ch0 = dp.cam_chunk_off[c]; ch0 < ch1; ch0 += 16) {
      double t[16];
#pragma unroll
      for (int q = 0; q < 16; ++q) t[q] = ch0 + q < ch1 ? zc[(long long)(ch0 + q) * B + k] : 0.0;
#pragma unroll
      for (int q = 0; q < 16; ++q) if (ch0 + q < ch1) acc += t[q];
    }
    z[cam_col(dp.C, dp.P, c, k)] += acc;
    return;
  }
  const int lane = threadIdx.x & 63;
  const int g = ((int)blockIdx.x - dp.C) * (kThreads / 64) + (threadIdx.x >> 6);
  if (g >= dp.N) return;
  double acc[3] = {0.0, 0.0, 0.0};
  const int mrow_lo = motion ? dp.mv.row_lo[g] : 0, mrow_hi = motion ? dp.mv.row_hi[g] : 0;      // (fetched beside the cameras' first loads)
  // a chunk starts at most bounds[0] control points below the running maximum of the starts: once that maximum is more than
  // bounds[0] past g, no later chunk starts at or before g (without the measured bound: a whole window)
  // (the MEASURED bound, not clipped to a window: a camera whose detections are not in time order -- nothing in the reference
  // forbids it -- has chunks that start arbitrarily far below the running maximum; the walk is then longer, never wrong)
  const int reach = bounds != nullptr ? bounds[0] : kJtWin;
  for (int c = lane; c < dp.C; c += 64) {
    // first chunk whose running-max window start is within reach of g (everything before ends left of g) ...
    const int end = dp.cam_chunk_off[c + 1];
    const int lo = first ? first[(long long)g * dp.C + c] : jtu_first_chunk(dp, zfill, c, g, jtu_window(bounds));
    // ... then forward until the running maximum is a whole window past g (a later chunk's own start is never that far
    // below the running maximum), adding the covering windows in chunk order
    // (four chunks at a time: their window starts together, then the entries of the covering ones together, then the adds in
    // chunk order -- the same sums as the one-chunk-at-a-time loop with a third of its dependent memory round trips; zfill is
    // non-decreasing, so "the loop has not stopped before chunk ch" is zfill[ch] <= g + kJtWin by itself)
    for (int ch0 = lo; ch0 < end; ch0 += 4) {
      int fill[4], g0[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const bool in = ch0 + q < end;
        fill[q] = in ? zfill[ch0 + q] : 0x7fffffff;
        g0[q] = in ? zg0[ch0 + q] : 0x7fffffff;
      }
      double w[4][3];
      bool use[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int lc = g - g0[q];
        use[q] = fill[q] <= g + reach && g0[q] != 0x7fffffff && lc >= 0 && lc < kJtWin;
        const double* wp = zs + (long long)(ch0 + q) * (3 * kJtWin) + 3 * (use[q] ? lc : 0);
#pragma unroll
        for (int d = 0; d < 3; ++d) w[q][d] = use[q] ? wp[d] : 0.0;
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) if (use[q]) { acc[0] += w[q][0]; acc[1] += w[q][1]; acc[2] += w[q][2]; }
      if (!(fill[3] <= g + reach)) break;
    }
  }
#pragma unroll
  for (int d = 0; d < 3; ++d)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc[d] += __shfl_xor(acc[d], off, 64);      // fixed pairing: deterministic
  if (motion) {
    // motion rows: lanes take rows row_lo + lane, + 64, ...; same butterfly
    double ma[3] = {0.0, 0.0, 0.0};
    for (int j = mrow_lo + lane; j < mrow_hi; j += 64) {
      const double uj = um[j];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const int cg = mctrl[(long long)k * dp.T + j];
        if (cg >= 0 && g >= cg && g <= cg + 3) {
#pragma unroll
          for (int d = 0; d < 3; ++d) ma[d] += mJ[(long long)(12 * k + 3 * (g - cg) + d) * dp.T + j] * uj;
        }
      }
    }
#pragma unroll
    for (int d = 0; d < 3; ++d) {
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) ma[d] += __shfl_xor(ma[d], off, 64);
      acc[d] += ma[d];
    }
  }
  if (lane < 3) z[dp.mv.ctrl_x0[g] + lane * dp.mv.ctrl_stride[g]] += (lane == 0 ? acc[0] : (lane == 1 ? acc[1] : acc[2]));
}

__global__ __launch_bounds__(kThreads) void k_motion_jv(DevProblem dp, const double* __restrict__ mJ, const int32_t* __restrict__ mctrl,
                                                        const double* __restrict__ v, double* __restrict__ ym) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= dp.T) return;
  ym[j] = motion_row_times(dp, mJ, mctrl, v, j);
}

}  // namespace mvus
