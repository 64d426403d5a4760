// What every stage of the BA device code needs, and no kernel: the workgroup size, the device problem record, the chunk-major
// Jacobian layout, the XCD tile map and the column of a camera unknown.
#pragma once
#include <cstddef>

#include "ba_math.h"      // MVUS_HD, SplineView, MotionView, ChunkInfo; hip_runtime.h under hipcc

namespace mvus {

constexpr int kThreads = 256;

struct DevProblem {  // trivially copyable: passed to kernels by value
  int C, P, NS, S, calib, undist, rs_free, sync_free, T, N;
  long long M;
  const double *frame, *u_raw, *v_raw, *u_obs, *v_obs, *H, *Kfix, *dfix;
  SplineView sp;
  MotionView mv;
  const int32_t *chunk_cam, *chunk_count;
  const ChunkInfo* chunks;    // the same launch table, one 32-byte record per chunk
  const int32_t* cam_chunk_off;   // [C+1] chunks of camera c are cam_chunk_off[c] .. cam_chunk_off[c+1]
  const long long *chunk_start, *det_off;
  int n_chunks;
  int mot_lo, mot_hi;   // motion rows whose first control point lies in [mot_lo, mot_hi) are evaluated (time shards), the rest are zero rows
};

// Chunk-major Jacobian: the 2*NS slot rows of one <=256-detection chunk are adjacent in memory,
//     J[(chunk * 2*NS + r) * kThreads + lane],   r = k (x row of slot k) or NS + k (y row),
// so a workgroup writes (and J v / J^T u / the assembly read) ONE contiguous 2*NS*2 KB block instead of 2*NS pieces M*8 bytes
// apart: the bare store pattern gains 8 % at 504k detections and 15 % at 2 M over the slot-major layout even with the XCD-aware
// order (tools/micro/store_bw.hip).  The C ABI keeps the slot-major layout (k_j_export converts on the way out).
template <int NS>
MVUS_HD long long j_chunk_offset(int chunk) { return (long long)chunk * (2 * NS * kThreads); }
inline size_t j_doubles(int NS, int n_chunks) { return (size_t)2 * NS * kThreads * (size_t)(n_chunks > 0 ? n_chunks : 1); }

// Workgroups are handed to the 8 XCDs round robin (blockIdx % 8), each XCD with its own L2.  xcd_tile maps blockIdx so that
// one XCD works on runs of kXcdRun consecutive tiles (shorter runs for small grids); launch xcd_grid(tiles) workgroups and
// skip tiles >= the real count.
#ifndef MVUS_XCD_RUN
#define MVUS_XCD_RUN 64
#endif
constexpr int kXcdRun = MVUS_XCD_RUN;
MVUS_HD int xcd_run_for(int tiles) { const int r = (tiles + 7) / 8; return r < kXcdRun ? (r > 0 ? r : 1) : kXcdRun; }
MVUS_HD int xcd_grid(int tiles) { const int per = 8 * xcd_run_for(tiles); return (tiles + per - 1) / per * per; }
#if defined(__HIPCC__)
__device__ __forceinline__ int xcd_tile(int tiles) {
  const int run = xcd_run_for(tiles);
  const int xcd = (int)blockIdx.x & 7, q = (int)blockIdx.x >> 3;          // q-th workgroup of this XCD
  return ((q / run) * 8 + xcd) * run + q % run;
}
__device__ __forceinline__ int cam_col(int C, int P, int c, int k) { return k < 3 ? k * C + c : 3 * C + c * P + (k - 3); }
#endif

}  // namespace mvus
