// Assembly of the normal equations (layout: ba_schur_hip.hip.h): the detection-major pass over half chunks, the camera-block
// reduction, the motion rows (three kernels by band width and route), diag(H) / g in x order, frozen unknowns and the halo exchange
// of time shards.  The window-major pass of the LM path is ba_assemble_win.hip.h.
#pragma once
#include <hip/hip_runtime.h>

#include "ba_dev_problem.h"
#include "ba_ne_views.h"
#include "ba_wave.hip.h"

namespace mvus {

// ---- assembly of the detection rows ------------------------------------------------------------------------
// One workgroup per HALF chunk (<=128 consecutive detections of one camera).  The 2*NS Jacobian slots and the two
// residuals of those detections are staged in LDS (row stride padded to 129 doubles).  Detections of one knot span
// touch the same four control points and (sorted by time) occupy one contiguous index range.
//   1. accumulate: thread (range, xyz d) forms, in registers, the outer products of its range -- 4 control points x
//      (B camera columns + the gradient) for the cross block and the 10 control-point pairs x 3 coordinates of the
//      spline band -- reading LDS ~0.4 times per FMA (a plain one-output-per-thread gather reads it twice per FMA and
//      was LDS bound); the camera block is split four ways over the detections and summed with two shuffles;
//   2. flush: the staged Jacobian is dead, its LDS is reused for the per-range partial blocks; every output entry is
//      then owned by ONE thread, which sums the (at most four) ranges that touch its control point and issues one
//      global fp64 atomic, consecutive threads on consecutive addresses.  (Measured: the L2 retires ~35 G atomic
//      cache-line transactions/s, so scattered per-range atomics cost 1 ms here while coalesced ones are free; LDS
//      fp64 atomics cost ~8 cycles per lane and are not used at all.)
// When a large rolling-shutter coefficient reorders the time stamps (spans interleave in index order) the staged
// columns are first rank-sorted by span in LDS.  Half chunks with more than kGaMaxR ranges (very sparse detections)
// take the slow path: per-range atomics straight from the registers.
// FUSED (the LM path with the analytic Jacobian): the 2 x NS blocks are not read from a materialised J at all -- the first
// two wavefronts evaluate their detection's residual and Jacobian (eval_observation_to, the arithmetic of k_observations)
// straight into the LDS staging area.  Per LM iteration this removes the Jacobian kernel, its 183 MB of stores and the
// 197 MB this kernel used to read back (BASELINE configs[2]); HBM traffic per observation falls to the 32 B of inputs.
#ifndef MVUS_GA_OBS
#define MVUS_GA_OBS 128
#endif
constexpr int kGaObs = MVUS_GA_OBS, kGaStride = kGaObs + 1, kGaThreads = 4 * kGaObs, kGaMaxR = kGaThreads / 6, kGaSplit = 8;
constexpr int kGaShift = kGaObs == 128 ? 7 : 6, kGaParts = 256 / kGaObs;      // detections per workgroup: 128 or 64 (parts of a 256-chunk)
static_assert(kGaObs == 128 || kGaObs == 64, "the assembly tile is 128 or 64 detections");
struct LdsRowSink {          // eval_observation_to sink: slot k of the x / y row of staged column t
  static constexpr bool kFactored = false;
  double* col;               // Js + t
  int ns;
  __device__ __forceinline__ void begin(int32_t) {}
  __device__ __forceinline__ void x(int k, double v) { col[k * kGaStride] = v; }
  __device__ __forceinline__ void y(int k, double v) { col[(ns + k) * kGaStride] = v; }
};
// ROBUST (a loss other than linear in force): every staged row is scaled as it is staged -- s J and rho' f / s of loss_scale_row --
// so the sums below are those of the robust system; f in memory stays the raw error_BA.
template <int NS, bool FUSED, bool ROBUST = false, class... L>
__global__ __launch_bounds__(kGaThreads) void k_assemble_spans(DevProblem dp, const double* __restrict__ J, const int32_t* __restrict__ span,
                                                             const double* __restrict__ f, NEView ne, const CamState* __restrict__ cams,
                                                             const double* __restrict__ x, L... loss_v) {
  static_assert(sizeof...(L) == (ROBUST ? 1 : 0), "the robust instantiation is launched with its LossSpec, the linear one without");
  const LossSpec loss = loss_arg(loss_v...);
  constexpr int B = NS - 12;
  constexpr int kJs = (2 * NS + 2) * kGaStride;
  constexpr int kEp = 4 * 3 * B, kGp = 12, kCp = 10 * 9;        // partial block sizes per range: cross, gradient, band
  constexpr int kRbE = kJs / (kEp + kGp), kRbC = kJs / kCp;     // ranges per flush round
  __shared__ double Js[kJs];                             // rows 0..NS-1: x-row slots, NS..2NS-1: y-row slots, then fx, fy
  __shared__ int meta[kGaObs + kGaObs / 2], rg[kGaObs];
  __shared__ int any_s, sort_s, nr_s;
  // flush: per owned control point of the round -- its index, the first range that reaches it and how many consecutive ranges do
  __shared__ int pt_ctrl[4 * kGaMaxR + 4];
  __shared__ unsigned char pt_rl[4 * kGaMaxR + 4], pt_cnt[4 * kGaMaxR + 4], pt_q[4 * kGaMaxR + 4];
  int* key = meta;                                                   // span per staged column
  unsigned char* rs = reinterpret_cast<unsigned char*>(meta + kGaObs);   // first / one-past-last column of a range
  unsigned char* re = rs + kGaObs;
  const int chunk = blockIdx.x / kGaParts, half = blockIdx.x % kGaParts;
  const int c = dp.chunk_cam[chunk];
  const int cnt = min(kGaObs, dp.chunk_count[chunk] - half * kGaObs);
  if (cnt <= 0) return;
  const long long i0 = dp.chunk_start[chunk] + half * kGaObs;
  const long long a0 = dp.det_off[c], Mc = dp.det_off[c + 1] - a0;
  const int tid = threadIdx.x;
  if (tid == 0) { any_s = 0; sort_s = 0; nr_s = 0; }
  const int t = tid & (kGaObs - 1);                    // detection handled while staging
  constexpr int kRowsPer = (2 * NS + 2 + 3) / 4;
  int g, kt;
  if (FUSED) {
    // every staged value starts as zero (invisible detections, columns past the end); then one lane per detection fills its column
#pragma unroll
    for (int k = 0; k < kRowsPer; ++k) {
      const int r = (tid >> kGaShift) + 4 * k;
      if (r < 2 * NS + 2) Js[r * kGaStride + t] = 0.0;
    }
    lds_barrier();
    g = -1;
    if (tid < kGaObs && t < cnt) {
      constexpr bool CALIB = NS == 30;
      const CamState& cam = cams[c];                    // wave-uniform: scalar loads
      const long long i = i0 + t;
      const double uo = CALIB ? 0.0 : dp.u_obs[i], vo = CALIB ? 0.0 : dp.v_obs[i];
      const double ur = CALIB ? dp.u_raw[i] : 0.0;
      LdsRowSink sink{Js + t, NS};
      const ObsResult r = eval_observation_to<CALIB, true>(cam, dp.sp, x, dp.undist != 0, dp.rs_free != 0, dp.sync_free != 0,
                                                           dp.frame[i], ur, dp.v_raw[i], uo, vo, sink);
      g = r.ctrl;
      if (g >= 0) {
        double fx = r.ex, fy = r.ey;
        if constexpr (ROBUST) {
          const double sx = loss_scale_row(loss, fx), sy = loss_scale_row(loss, fy);
#pragma unroll
          for (int k = 0; k < NS; ++k) { Js[k * kGaStride + t] *= sx; Js[(NS + k) * kGaStride + t] *= sy; }
        }
        Js[(2 * NS) * kGaStride + t] = fx; Js[(2 * NS + 1) * kGaStride + t] = fy;
      }
    }
    kt = g >= 0 ? g : 0x7fffffff;
    if (tid < kGaObs) key[tid] = kt;
  } else {
    g = t < cnt ? span[i0 + t] : -1;
    kt = g >= 0 ? g : 0x7fffffff;                      // invisible detections sort last
    if (tid < kGaObs) key[tid] = kt;
    // stage: thread (tid) loads rows tid/128, tid/128+4, ... for detection t
#pragma unroll
    for (int k = 0; k < kRowsPer; ++k) {
      const int r = (tid >> kGaShift) + 4 * k;
      if (r >= 2 * NS + 2) break;
      double v = 0.0;
      if (g >= 0) {
        if (r < 2 * NS) v = J[j_chunk_offset<NS>(chunk) + r * kThreads + half * kGaObs + t];
        else v = f[2 * a0 + (r - 2 * NS) * Mc + (i0 + t - a0)];
        if constexpr (ROBUST) {                          // the row's own residual decides its scale: x rows r < NS and 2 NS, y rows the others
          const bool yrow = r < 2 * NS ? r >= NS : r == 2 * NS + 1;
          double fr = f[2 * a0 + (yrow ? Mc : 0) + (i0 + t - a0)];
          const double sc = loss_scale_row(loss, fr);
          v = r < 2 * NS ? v * sc : fr;
        }
      }
      Js[r * kGaStride + t] = v;
    }
  }
  lds_barrier();
  if (FUSED) kt = key[t];                                // the key of column t, for the threads that did not evaluate it
  if (tid < kGaObs) {
    if (g >= 0) any_s = 1;
    if (tid > 0 && kt < key[tid - 1]) sort_s = 1;
  }
  lds_barrier();
  if (!any_s) return;      // nothing visible (uniform)
  if (sort_s) {
    int pos = 0;
    for (int u = 0; u < kGaObs; ++u) { const int ku = key[u]; pos += (ku < kt) || (ku == kt && u < t); }
    double tmp[kRowsPer];                                // this thread's rows: (tid >> 7) + 4k
#pragma unroll
    for (int k = 0; k < kRowsPer; ++k) { const int r = (tid >> kGaShift) + 4 * k; tmp[k] = r < 2 * NS + 2 ? Js[r * kGaStride + t] : 0.0; }
    lds_barrier();
#pragma unroll
    for (int k = 0; k < kRowsPer; ++k) { const int r = (tid >> kGaShift) + 4 * k; if (r < 2 * NS + 2) Js[r * kGaStride + pos] = tmp[k]; }
    if (tid < kGaObs) key[pos] = kt;
    lds_barrier();
  }
  // ranges of equal span, in span order (slot = number of range starts before this one, from the wave ballots)
  {
    const int ks = tid < kGaObs ? key[tid] : 0x7fffffff;
    // a run of equal span longer than kGaSplit columns (dense timelines: many detections per knot span) is cut into
    // pieces of kGaSplit so that the outer products below are spread over more threads
    int back = 0;
    if (tid < kGaObs && ks != 0x7fffffff) while (back < tid && key[tid - back - 1] == ks) ++back;
    const bool start = tid < kGaObs && ks != 0x7fffffff && back % kGaSplit == 0;
    const unsigned long long mask = __ballot(start);
    if (tid == 0) nr_s = __popcll(mask);                 // starts in the first wavefront
    lds_barrier();
    if (start) {
      int e = tid + 1;
      while (e < kGaObs && key[e] == ks && e - tid < kGaSplit) ++e;
      const int slot = (tid >= 64 ? nr_s : 0) + __popcll(mask & ((1ull << (tid & 63)) - 1ull));
      const int kl = ks - ne.row0;                       // local control point; a time shard must hold all four
      const bool inr = kl >= 0 && kl + 3 < ne.N;
      if (!inr) atomicOr(ne.err, 1);
      rs[slot] = (unsigned char)tid; re[slot] = (unsigned char)(inr ? e : tid); rg[slot] = inr ? kl : 0;
    }
    lds_barrier();
    if (tid == 64) nr_s += __popcll(mask);
  }
  lds_barrier();
  const int nr = nr_s;
  const double* fxs = Js + (2 * NS) * kGaStride;
  const double* fys = fxs + kGaStride;
  // camera block (lower triangle) and camera gradient on the fp64 matrix cores: G = R R^T with R = [camera slots; f]
  // ((B+1) x 2*128, x rows then y rows).  For v_mfma_f64_16x16x4 the A fragment (lane l: R[l&15][k0 + (l>>4)]) IS the
  // B fragment of R^T, so one LDS read feeds both operands.  The LAST wavefront does all of it (64 MFMAs per tile pair)
  // while the others go on to the outer products below, where it would have been idle.
  {
    // every wavefront takes 1/8 of the k-steps (one wavefront doing all 64 matrix-core instructions shared its SIMD with
    // three busy wavefronts and finished last: 13k cycles while the others needed 6k and waited) and leaves its own partial
    // block; k_cam_block_reduce adds the 8 x (workgroups of the camera) partials
    constexpr int TI = (B + 1 + 15) / 16;                 // 16-row tiles of R
    constexpr int kWaves = kGaThreads / 64, kStepsPerWave = (kGaObs / 4) / kWaves;
    const int lane = tid & 63, wave = tid >> 6;
    const int lr = lane & 15, lk = lane >> 4;
    d4 cacc[TI][TI];
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
      for (int j = 0; j < TI; ++j) cacc[i][j] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int xy = 0; xy < 2; ++xy)
#pragma unroll
      for (int kk = 0; kk < kStepsPerWave; ++kk) {
        const int u = (wave * kStepsPerWave + kk) * 4 + lk;
        double a[TI];
#pragma unroll
        for (int i = 0; i < TI; ++i) {
          // ONE unconditional LDS read per fragment (rows past B read row B and are zeroed by a select): a branch per case
          // serialises the unrolled reads
          const int row = 16 * i + lr;
          const int src = row < B ? xy * NS + row : 2 * NS + xy;
          const double v = Js[src * kGaStride + u];
          a[i] = row <= B ? v : 0.0;
        }
#pragma unroll
        for (int i = 0; i < TI; ++i)
#pragma unroll
          for (int j = 0; j <= i; ++j) cacc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], a[j], cacc[i][j], 0, 0, 0);
      }
    double* mine = ne.Apart + ((long long)blockIdx.x * kWaves + wave) * ((B + 1) * (B + 2) / 2);
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
      for (int j = 0; j <= i; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int ra = 16 * i + lk + 4 * r, rb = 16 * j + lr;      // C/D layout: row = (lane>>4) + 4 reg, col = lane&15
          if (ra > B || rb > ra) continue;
          mine[ra * (ra + 1) / 2 + rb] = cacc[i][j][r];              // plain stores: no contention on the camera's few lines
        }
  }
  const bool fast = nr <= kGaMaxR;                        // uniform
  // one register file for both roles -- E role: EA(q, k) cross block + gradient (k = B) of (range, d);
  // C role: CA(qa, w, d2) band blocks (w = qb - qa), row coordinate d
  constexpr int kAcc = 4 * (B + 1) > 48 ? 4 * (B + 1) : 48;
  double acc_[kAcc];
#define EA(q, k) acc_[(q) * (B + 1) + (k)]
#define CA(qa, w, d2) acc_[((qa) * 4 + (w)) * 3 + (d2)]
  int myr = -1, myd = 0;
  bool crole = false;
  for (int item = tid; item < 6 * nr; item += kGaThreads) {
    crole = item >= 3 * nr;
    const int it2 = crole ? item - 3 * nr : item;
    const int r = it2 / 3, d = it2 % 3;
    const int b = rs[r], e = re[r];
    const double* sx = Js + B * kGaStride;               // spline slot (q, d2) x-row: sx[(3q+d2)*stride + u]
    const double* sy = Js + (NS + B) * kGaStride;
    myr = r; myd = d;
    if (!crole) {
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int k = 0; k <= B; ++k) EA(q, k) = 0.0;
      for (int u = b; u < e; ++u) {
        double ax[4], ay[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) { ax[q] = sx[(3 * q + d) * kGaStride + u]; ay[q] = sy[(3 * q + d) * kGaStride + u]; }
#pragma unroll
        for (int k = 0; k <= B; ++k) {
          const double cx = k < B ? Js[k * kGaStride + u] : fxs[u];
          const double cy = k < B ? Js[(NS + k) * kGaStride + u] : fys[u];
#pragma unroll
          for (int q = 0; q < 4; ++q) EA(q, k) += cx * ax[q] + cy * ay[q];
        }
      }
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int w = 0; w < 4; ++w)
#pragma unroll
          for (int d2 = 0; d2 < 3; ++d2) CA(q, w, d2) = 0.0;
      for (int u = b; u < e; ++u) {
        double vx[12], vy[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) { vx[k] = sx[k * kGaStride + u]; vy[k] = sy[k * kGaStride + u]; }
#pragma unroll
        for (int qa = 0; qa < 4; ++qa) {                 // vx[3qa + d] with d a run-time value: select, keeps vx in registers
          const double ax = d == 0 ? vx[3 * qa] : (d == 1 ? vx[3 * qa + 1] : vx[3 * qa + 2]);
          const double ay = d == 0 ? vy[3 * qa] : (d == 1 ? vy[3 * qa + 1] : vy[3 * qa + 2]);
#pragma unroll
          for (int w = 0; qa + w < 4; ++w)
#pragma unroll
            for (int d2 = 0; d2 < 3; ++d2) CA(qa, w, d2) += ax * vx[3 * (qa + w) + d2] + ay * vy[3 * (qa + w) + d2];
        }
      }
    }
    if (!fast) {                                         // slow path: too many ranges to keep one per thread
      const int gq = rg[r];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (!crole) {
          const int row = 3 * (gq + q) + d;
          double* er = ne.Et + ((long long)c * ne.N3 + row) * B;
#pragma unroll
          for (int k = 0; k < B; ++k) if (EA(q, k) != 0.0) unsafeAtomicAdd(&er[k], EA(q, k));
          if (EA(q, B) != 0.0) unsafeAtomicAdd(&ne.gs[row], EA(q, B));
        } else {
#pragma unroll
          for (int w = 0; q + w < 4; ++w)
#pragma unroll
            for (int d2 = 0; d2 < 3; ++d2)
              if (CA(q, w, d2) != 0.0) unsafeAtomicAdd(&ne.Cb[((long long)(gq + q) * ne.W + w) * 9 + 3 * d + d2], CA(q, w, d2));
        }
      }
    }
  }
  if (!fast) return;
  lds_barrier();                                        // every thread holds its partials in registers: Js is dead
  // ---- owner tables of ALL flush rounds, built once ----------------------------------------------------------------
  // A round covers kRb consecutive ranges (as many per-range partial blocks as fit the dead staging LDS).  Inside a round a
  // control point is owned by the first range that reaches it: range t owns its last min(4, rg[t] - rg[t-1]) points (all four
  // when it opens a round).  The thread of range t writes, for each point it owns: the control point, itself as the first
  // reaching range, how many consecutive ranges of the round reach the point (ranges are span ordered) and the slot q2 of the
  // point inside the first four of them -- so a flush thread reads one table entry and then its partial sums, with no chain of
  // dependent look-ups per output (measured per workgroup of 68 ranges: 4 owner builds x 3k cycles + 2 x 2 loops x 4k cycles
  // before; one build now).
  constexpr int kRb = kRbE < kRbC ? kRbE : kRbC;
  __shared__ int round_off[8];                            // first owned point of round rho; [rounds] = total
  {
    const int t = tid;
    const bool has = t < nr;
    const int rl = has ? t % kRb : 0;
    const int mine = has ? (rl == 0 ? 4 : min(4, rg[t] - rg[t - 1])) : 0;
    int incl = mine;
    if (tid < 128) {
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) { const int o = __shfl_up(incl, off, 64); if ((tid & 63) >= off) incl += o; }
      if (tid == 63) round_off[7] = incl;                // total of the first wavefront (scratch)
    }
    lds_barrier();
    if (has) {
      const int bs = incl - mine + (tid >= 64 ? round_off[7] : 0);
      const int rend = min(nr, (t / kRb + 1) * kRb);     // one past the last range of this range's round
      for (int j = 0; j < mine; ++j) {
        const int ctrl = rg[t] + (4 - mine + j);
        int cnt = 0, qp = 0;
        while (t + cnt < rend && ctrl - rg[t + cnt] >= 0) { if (cnt < 4) qp |= (ctrl - rg[t + cnt]) << (2 * cnt); ++cnt; }
        pt_ctrl[bs + j] = ctrl; pt_rl[bs + j] = (unsigned char)rl; pt_cnt[bs + j] = (unsigned char)cnt; pt_q[bs + j] = (unsigned char)qp;
      }
      if (rl == 0) round_off[t / kRb] = bs;
      if (t == nr - 1) round_off[(nr - 1) / kRb + 1] = bs + mine;
    }
    lds_barrier();
  }
  // ---- flush of the cross block + gradient: Ep[rl][q][3][B], Gp[rl][q][3] ----
  for (int r0 = 0, rho = 0; r0 < nr; r0 += kRb, ++rho) {
    const int nb = min(kRb, nr - r0);
    double* Ep = Js;
    double* Gp = Js + kRb * kEp;
    if (!crole && myr >= r0 && myr < r0 + nb) {
      const int rl = myr - r0;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
#pragma unroll
        for (int k = 0; k < B; ++k) Ep[(rl * 4 + q) * 3 * B + myd * B + k] = EA(q, k);
        Gp[(rl * 4 + q) * 3 + myd] = EA(q, B);
      }
    }
    lds_barrier();
    const int p0 = round_off[rho], nown = round_off[rho + 1] - p0;
    constexpr int per = 3 * B + 3;                       // entries per owned control point: 3 x B cross + 3 gradient
    for (int o = tid; o < nown * per; o += kGaThreads) {
      const int i = p0 + o / per, dk = o % per;
      const int ctrl = pt_ctrl[i], rl = pt_rl[i], cnt = pt_cnt[i], qp = pt_q[i];
      const bool grad = dk >= 3 * B;
      double acc = 0.0;
#pragma unroll
      for (int j = 0; j < 4; ++j)                        // the first four reaching ranges: slots from the table, reads independent
        if (j < cnt) { const int q2 = (qp >> (2 * j)) & 3; acc += grad ? Gp[((rl + j) * 4 + q2) * 3 + dk - 3 * B] : Ep[((rl + j) * 4 + q2) * 3 * B + dk]; }
      for (int j = 4; j < cnt; ++j) {                    // (a span cut into many pieces: rare)
        const int q2 = ctrl - rg[r0 + rl + j];
        acc += grad ? Gp[((rl + j) * 4 + q2) * 3 + dk - 3 * B] : Ep[((rl + j) * 4 + q2) * 3 * B + dk];
      }
      if (acc != 0.0) {
        if (grad) unsafeAtomicAdd(&ne.gs[3 * ctrl + dk - 3 * B], acc);
        else unsafeAtomicAdd(&ne.Et[((long long)c * ne.N3 + 3 * ctrl) * B + dk], acc);
      }
    }
    lds_barrier();
  }
  // ---- flush of the spline band: Cp[rl][pair (qa, w)][3][3], pair = 4 qa - qa (qa - 1) / 2 + w ----
  for (int r0 = 0, rho = 0; r0 < nr; r0 += kRb, ++rho) {
    const int nb = min(kRb, nr - r0);
    double* Cp = Js;
    if (crole && myr >= r0 && myr < r0 + nb) {
      const int rl = myr - r0;
#pragma unroll
      for (int qa = 0; qa < 4; ++qa)
#pragma unroll
        for (int w = 0; qa + w < 4; ++w)
#pragma unroll
          for (int d2 = 0; d2 < 3; ++d2) Cp[(rl * 10 + 4 * qa - qa * (qa - 1) / 2 + w) * 9 + 3 * myd + d2] = CA(qa, w, d2);
    }
    lds_barrier();
    const int p0 = round_off[rho], nown = round_off[rho + 1] - p0;
    for (int o = tid; o < nown * 36; o += kGaThreads) {
      const int i = p0 + o / 36, wd = o % 36, w = wd / 9, dd = wd % 9;
      const int ctrl = pt_ctrl[i], rl = pt_rl[i], cnt = pt_cnt[i], qp = pt_q[i];
      double acc = 0.0;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (j < cnt) { const int q2 = (qp >> (2 * j)) & 3; if (q2 + w < 4) acc += Cp[((rl + j) * 10 + 4 * q2 - q2 * (q2 - 1) / 2 + w) * 9 + dd]; }
      for (int j = 4; j < cnt; ++j) {
        const int q2 = ctrl - rg[r0 + rl + j];
        if (q2 + w < 4) acc += Cp[((rl + j) * 10 + 4 * q2 - q2 * (q2 - 1) / 2 + w) * 9 + dd];
      }
      if (acc != 0.0) unsafeAtomicAdd(&ne.Cb[((long long)ctrl * ne.W) * 9 + wd], acc);
    }
    lds_barrier();
  }
#undef EA
#undef CA
}

// A[c] (both triangles) and gc[c] from the per-workgroup partial blocks of k_assemble_spans: one workgroup per camera, entry e
// of the packed lower triangle summed over the camera's assembly workgroups in index order by four threads (quarters, then a
// fixed combine) -- no atomics, the same bits every run.  Workgroups that had nothing to add left zeros (the buffer is
// cleared with the rest of the normal equations).
template <int B>
__global__ __launch_bounds__(1024) void k_cam_block_reduce(DevProblem dp, NEView ne) {
  constexpr int PSZ = (B + 1) * (B + 2) / 2, kLanes = PSZ <= 64 ? 64 : 256, kGroups = 1024 / kLanes;
  __shared__ double part[kGroups][kLanes];
  const int c = blockIdx.x;
  constexpr int kPer = kGaParts * (kGaThreads / 64);                      // partial blocks per 256-chunk: assembly workgroups x wavefronts
  // two workgroups per camera (blockIdx.y), each over half of the partial blocks; both add into the zeroed A / gc with atomics --
  // 0 + a + b has the same bits in either order, so the result stays deterministic
  const int wa = dp.cam_chunk_off[c] * kPer, wb = dp.cam_chunk_off[c + 1] * kPer, wm = wa + (wb - wa + 1) / 2;
  const int w0 = blockIdx.y == 0 ? wa : wm, w1 = blockIdx.y == 0 ? wm : wb;
  const int k = threadIdx.x % kLanes, grp = threadIdx.x / kLanes;
  // group grp adds the partial blocks w0 + grp, w0 + grp + kGroups, ... (independent loads, four in flight), then the groups are
  // added in index order: a fixed summation tree
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  if (k < PSZ) {
    int w = w0 + grp;
    for (; w + 3 * kGroups < w1; w += 4 * kGroups) {
      a0 += ne.Apart[(long long)w * PSZ + k];
      a1 += ne.Apart[(long long)(w + kGroups) * PSZ + k];
      a2 += ne.Apart[(long long)(w + 2 * kGroups) * PSZ + k];
      a3 += ne.Apart[(long long)(w + 3 * kGroups) * PSZ + k];
    }
    for (; w < w1; w += kGroups) a0 += ne.Apart[(long long)w * PSZ + k];
  }
  part[grp][k] = (a0 + a1) + (a2 + a3);
  __syncthreads();
  if (threadIdx.x < PSZ) {
    double v = 0.0;
#pragma unroll
    for (int g = 0; g < kGroups; ++g) v += part[g][threadIdx.x];
    const int kk = threadIdx.x;
    int ra = 0;
    while ((ra + 1) * (ra + 2) / 2 <= kk) ++ra;
    const int rb = kk - ra * (ra + 1) / 2;
    if (ra == B) { if (rb < B) unsafeAtomicAdd(&ne.gc[c * B + rb], v); }
    else {
      unsafeAtomicAdd(&ne.A[((long long)c * B + ra) * B + rb], v);
      if (ra != rb) unsafeAtomicAdd(&ne.A[((long long)c * B + rb) * B + ra], v);
    }
  }
}

// motion-regulariser rows: spline block and gradient only (the rows do not depend on camera parameters).
// 256 consecutive rows (= consecutive sample times) per workgroup; each row is first compacted to the <= 6
// distinct control points it touches, then accumulated into an LDS window like the detection rows.
constexpr int kMotW = 6;
// (ROBUST, here and in the two row-ordered kernels below: the row's coefficients times s, its residual rho' f / s -- loss_scale_row)
template <bool ROBUST = false, class... L>
__global__ __launch_bounds__(kThreads) void k_assemble_motion(DevProblem dp, const double* __restrict__ mJ, const int32_t* __restrict__ mctrl,
                                                              const double* __restrict__ fm, NEView ne, L... loss_v) {
  static_assert(sizeof...(L) == (ROBUST ? 1 : 0), "the robust instantiation is launched with its LossSpec, the linear one without");
  const LossSpec loss = loss_arg(loss_v...);
  __shared__ double Cw[kNWin * kMotW * 9];
  __shared__ double gsw[kNWin * 3];
  __shared__ int gmin_s[kThreads / 64];
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int k = threadIdx.x; k < kNWin * kMotW * 9; k += kThreads) Cw[k] = 0.0;
  for (int k = threadIdx.x; k < kNWin * 3; k += kThreads) gsw[k] = 0.0;
  // compact the row: control points lo .. lo+kMotW-1, 3 coordinates each
  int lo = 0x7fffffff, hi = -1;
  int cid[3] = {-1, -1, -1};
  if (j < dp.T) {
    bool outside = false;
    for (int k = 0; k < 3; ++k) {
      cid[k] = mctrl[(long long)k * dp.T + j];
      if (cid[k] >= 0) {
        cid[k] -= ne.row0;                               // local control point
        if (cid[k] < 0 || cid[k] + 3 >= ne.N) outside = true;
        lo = min(lo, cid[k]); hi = max(hi, cid[k] + 3);
      }
    }
    if (outside) { atomicOr(ne.err, 1); lo = 0x7fffffff; hi = -1; cid[0] = cid[1] = cid[2] = -1; }
  }
  double rv[kMotW * 3];
#pragma unroll
  for (int e = 0; e < kMotW * 3; ++e) rv[e] = 0.0;
  const bool live = hi >= 0 && hi - lo < kMotW;      // the band width W (<= 6) guarantees this for valid rows
  if (live)
    for (int k = 0; k < 3; ++k) {
      if (cid[k] < 0) continue;
      const int o = cid[k] - lo;
      for (int q = 0; q < 4; ++q)
        for (int d = 0; d < 3; ++d) {
          const double v = mJ[(long long)(12 * k + 3 * q + d) * dp.T + j];
          // static indexing of rv: select by comparison
#pragma unroll
          for (int e = 0; e < kMotW * 3; ++e) if (e == 3 * (o + q) + d) rv[e] += v;
        }
    }
  int gm = wave_min_i(live ? lo : 0x7fffffff);
  if (lane == 0) gmin_s[wave] = gm;
  __syncthreads();
  int g0 = gmin_s[0];
#pragma unroll
  for (int w = 1; w < kThreads / 64; ++w) g0 = min(g0, gmin_s[w]);
  if (g0 == 0x7fffffff) return;
  if (live) {
    double fj = fm[j];
    if constexpr (ROBUST) {
      const double sc = loss_scale_row(loss, fj);
#pragma unroll
      for (int e = 0; e < kMotW * 3; ++e) rv[e] *= sc;
    }
    const int l = lo - g0;
    const bool inwin = l + kMotW <= kNWin;
#pragma unroll
    for (int a = 0; a < kMotW; ++a) {
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        const double va = rv[3 * a + d];
        if (va == 0.0) continue;
        if (inwin) unsafeAtomicAdd(&gsw[3 * (l + a) + d], va * fj);
        else unsafeAtomicAdd(&ne.gs[3 * (lo + a) + d], va * fj);
#pragma unroll
        for (int b = a; b < kMotW; ++b) {
          if (b - a >= ne.W) continue;
#pragma unroll
          for (int d2 = 0; d2 < 3; ++d2) {
            const double vb = rv[3 * b + d2];
            if (vb == 0.0) continue;
            if (inwin) unsafeAtomicAdd(&Cw[((l + a) * kMotW + (b - a)) * 9 + 3 * d + d2], va * vb);
            else unsafeAtomicAdd(&ne.Cb[((long long)(lo + a) * ne.W + (b - a)) * 9 + 3 * d + d2], va * vb);
          }
        }
      }
    }
  }
  __syncthreads();
  for (int k = threadIdx.x; k < kNWin * 3; k += kThreads) {
    const int r = 3 * g0 + k;
    if (r < ne.N3 && gsw[k] != 0.0) unsafeAtomicAdd(&ne.gs[r], gsw[k]);
  }
  for (int k = threadIdx.x; k < kNWin * kMotW * 9; k += kThreads) {
    const int gg = g0 + k / (kMotW * 9), w = (k / 9) % kMotW;
    const double v = Cw[k];
    if (gg < ne.N && w < ne.W && v != 0.0) unsafeAtomicAdd(&ne.Cb[((long long)gg * ne.W + w) * 9 + (k % 9)], v);
  }
}

// The motion rows in the deterministic mode: one wavefront per control point g.  The rows that can touch g (row_lo[g] <= j <
// row_hi[g], as in k_jtu_reduce) are taken 64 at a time: first lane = ROW -- its coefficients of (g + a, coordinate d), a < W, i.e.
// the sum of its (<= 3) sample blocks that reach that control point (what k_assemble_motion compacts into rv[]), and its residual,
// go to LDS; then lane = ENTRY (gradient coordinate, or band entry (w, d, d2)) adds the rows in row order.  One order of additions
// per entry, no atomics.  Rows k_assemble_motion skips (outside the slice, wider than kMotW control points) are zeros here.
constexpr int kDetMotW = 6;                              // >= ne.W (the band solver supports at most six 3x3 blocks)
template <bool ROBUST = false, class... L>
__global__ __launch_bounds__(kThreads) void k_det_motion(DevProblem dp, const double* __restrict__ mJ, const int32_t* __restrict__ mctrl,
                                                         const double* __restrict__ fm, NEView ne, L... loss_v) {
  static_assert(sizeof...(L) == (ROBUST ? 1 : 0), "the robust instantiation is launched with its LossSpec, the linear one without");
  const LossSpec loss = loss_arg(loss_v...);
  constexpr int kWaves = kThreads / 64, kRv = kDetMotW * 3 + 1;       // per row: W x 3 coefficients + the residual
  __shared__ double rv[kWaves][64][kRv + 1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = (int)blockIdx.x * kWaves + wave;
  if (g >= ne.N) return;                                // (wave-uniform; no workgroup barrier below)
  const int gg = g + ne.row0;                            // row_lo / row_hi are indexed by the global control point
  const int j0 = dp.mv.row_lo[gg], j1 = dp.mv.row_hi[gg];
  const int per = 3 + ne.W * 9;
  const bool grad = lane < 3;
  const int w = grad ? 0 : (lane - 3) / 9, d = grad ? lane : ((lane - 3) % 9) / 3, d2 = grad ? 0 : (lane - 3) % 3;
  const bool mine = lane < per && g + w < ne.N;
  double acc = 0.0;
  for (int jb = j0; jb < j1; jb += 64) {
    const int j = jb + lane;
    double r[kRv];
#pragma unroll
    for (int e = 0; e < kRv; ++e) r[e] = 0.0;
    if (j < j1) {
      int cid[3], lo = 0x7fffffff, hi = -1;
      bool outside = false;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        cid[k] = mctrl[(long long)k * dp.T + j];
        if (cid[k] >= 0) {
          cid[k] -= ne.row0;
          if (cid[k] < 0 || cid[k] + 3 >= ne.N) outside = true;
          lo = min(lo, cid[k]); hi = max(hi, cid[k] + 3);
        }
      }
      if (!outside && hi >= 0 && hi - lo < kMotW) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          if (cid[k] < 0) continue;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int a = cid[k] + q - g;                // this block's control point q is g + a
            if (a < 0 || a >= kDetMotW) continue;
#pragma unroll
            for (int dd = 0; dd < 3; ++dd) {
              const double v = mJ[(long long)(12 * k + 3 * q + dd) * dp.T + j];
#pragma unroll
              for (int e = 0; e < kDetMotW * 3; ++e) if (e == 3 * a + dd) r[e] += v;      // static indexing of r: select by comparison
            }
          }
        }
        double fj = fm[j];
        if constexpr (ROBUST) {
          const double sc = loss_scale_row(loss, fj);
#pragma unroll
          for (int e = 0; e < kDetMotW * 3; ++e) r[e] *= sc;
        }
        r[kDetMotW * 3] = fj;
      }
    }
#pragma unroll
    for (int e = 0; e < kRv; ++e) rv[wave][lane][e] = r[e];
    lds_wave_sync();
    const int nrow = min(64, j1 - jb);
    if (mine) {
      for (int t = 0; t < nrow; ++t) {
        const double va = rv[wave][t][d];
        const double vb = grad ? rv[wave][t][kDetMotW * 3] : rv[wave][t][3 * w + d2];
        acc += va * vb;
      }
    }
    lds_wave_sync();
  }
  if (mine && acc != 0.0) {
    if (grad) ne.gs[3 * g + lane] += acc;
    else ne.Cb[((long long)g * ne.W) * 9 + (lane - 3)] += acc;
  }
}

// The same for motion rows that reach further than six control points (FITPACK knots less than a frame apart: the three samples of
// a row then span more than three knot spans; the band has W <= kWideW blocks per row): one wavefront per control point, the rows'
// coefficients built in LDS by the row's own lane, every lane adds up to three entries of the control point's band row.
constexpr int kWideW = 16;
template <bool ROBUST = false, class... L>
__global__ __launch_bounds__(64) void k_det_motion_wide(DevProblem dp, const double* __restrict__ mJ, const int32_t* __restrict__ mctrl,
                                                        const double* __restrict__ fm, NEView ne, L... loss_v) {
  static_assert(sizeof...(L) == (ROBUST ? 1 : 0), "the robust instantiation is launched with its LossSpec, the linear one without");
  const LossSpec loss = loss_arg(loss_v...);
  constexpr int kRv = kWideW * 3 + 1;                      // per row: W x 3 coefficients + the residual
  __shared__ double rv[64][kRv + 1];
  const int lane = threadIdx.x, g = blockIdx.x;
  if (g >= ne.N) return;
  const int gg = g + ne.row0;
  const int j0 = dp.mv.row_lo[gg], j1 = dp.mv.row_hi[gg];
  const int per = 3 + ne.W * 9;
  double acc[3] = {0.0, 0.0, 0.0};
  for (int jb = j0; jb < j1; jb += 64) {
    const int j = jb + lane;
    for (int e = 0; e < kRv; ++e) rv[lane][e] = 0.0;
    if (j < j1) {
      int cid[3], lo = 0x7fffffff, hi = -1;
      bool outside = false;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        cid[k] = mctrl[(long long)k * dp.T + j];
        if (cid[k] >= 0) {
          cid[k] -= ne.row0;
          if (cid[k] < 0 || cid[k] + 3 >= ne.N) outside = true;
          lo = min(lo, cid[k]); hi = max(hi, cid[k] + 3);
        }
      }
      if (!outside && hi >= 0 && hi - lo < kWideW) {
        for (int k = 0; k < 3; ++k) {
          if (cid[k] < 0) continue;
          for (int q = 0; q < 4; ++q) {
            const int a = cid[k] + q - g;                  // this block's control point q is g + a
            if (a < 0 || a >= kWideW) continue;
            for (int dd = 0; dd < 3; ++dd) rv[lane][3 * a + dd] += mJ[(long long)(12 * k + 3 * q + dd) * dp.T + j];
          }
        }
        double fj = fm[j];
        if constexpr (ROBUST) {
          const double sc = loss_scale_row(loss, fj);
          for (int e = 0; e < kWideW * 3; ++e) rv[lane][e] *= sc;
        }
        rv[lane][kWideW * 3] = fj;
      }
    }
    lds_wave_sync();
    const int nrow = min(64, j1 - jb);
#pragma unroll
    for (int t3 = 0; t3 < 3; ++t3) {
      const int e = lane + 64 * t3;
      if (e >= per) continue;
      const bool grad = e < 3;
      const int w = grad ? 0 : (e - 3) / 9, d = grad ? e : ((e - 3) % 9) / 3, d2 = grad ? 0 : (e - 3) % 3;
      if (g + w >= ne.N) continue;
      double a = 0.0;
      for (int t = 0; t < nrow; ++t) a += rv[t][d] * (grad ? rv[t][kWideW * 3] : rv[t][3 * w + d2]);
      acc[t3] += a;
    }
    lds_wave_sync();
  }
#pragma unroll
  for (int t3 = 0; t3 < 3; ++t3) {
    const int e = lane + 64 * t3;
    if (e >= per || acc[t3] == 0.0) continue;
    if (e < 3) ne.gs[3 * g + e] += acc[t3];
    else if (g + (e - 3) / 9 < ne.N) ne.Cb[((long long)g * ne.W) * 9 + (e - 3)] += acc[t3];
  }
}

// D = diag(H) in x order (0 -> 1 so that unused columns stay put), and g in x order
__device__ __forceinline__ void ne_diag_grad_entry(const DevProblem& dp, const NEView& ne, int raw, int idx, double* __restrict__ D, double* __restrict__ gx) {
  // raw (time shards): this rank's PARTIAL diagonal, to be summed over the ranks before the unpacking k_halo_copy replaces zeros by 1
  if (idx < ne.CB) {
    const int c = idx / ne.B, k = idx % ne.B;
    const double h = ne.A[((long long)c * ne.B + k) * ne.B + k];
    const int col = cam_col(dp.C, dp.P, c, k);
    D[col] = (raw || h > 0.0) ? h : 1.0;
    gx[col] = ne.gc[idx];
  } else if (idx < ne.CB + ne.N3) {
    const int r = idx - ne.CB, g = r / 3, d = r % 3;
    const double h = ne.Cb[((long long)g * ne.W) * 9 + 4 * d];
    const int gg = g + ne.row0;
    const int col = dp.mv.ctrl_x0[gg] + d * dp.mv.ctrl_stride[gg];
    D[col] = (raw || h > 0.0) ? h : 1.0;
    gx[col] = ne.gs[r];
  }
}
__global__ void k_ne_diag_grad(DevProblem dp, NEView ne, int raw, double* __restrict__ D, double* __restrict__ gx) {
  ne_diag_grad_entry(dp, ne, raw, blockIdx.x * blockDim.x + threadIdx.x, D, gx);
}

// Frozen camera-side unknowns (mvus_ba_set_frozen): behind an assembly, before anything reads the blocks.  One workgroup per frozen
// entry e = c * B + k (internal order: alpha, beta, rs, camera parameters): its cross row against the spline block, row and column k of
// camera block c and its gradient entry become 0, the diagonal 1 -- D = diag(H) is extracted afterwards (k_band_pack / k_ne_diag_grad)
// and comes out as 1, the damped system keeps (1 + lambda) p_k = 0 as an equation of its own and the step of that unknown is exactly 0.
// The cross block is kept camera-major with the B slots of one (camera, spline row) adjacent, Et[(c * N3 + r) * B + k]: a cross ROW of
// the exported layout is a column of stride B here, so each lane stores one double, B * 8 bytes from its neighbour's (N3 stores per
// entry: 0.12 MB at configs[2]).  Two frozen entries of one camera write the same zeros into the two off-diagonal entries they share.
// Launched only with a non-empty mask; never on a sharded handle (refused before).
constexpr int kFreezeThreads = 256;
__global__ __launch_bounds__(kFreezeThreads) void k_freeze_ne(NEView ne, const int32_t* __restrict__ frozen, int count) {
  if ((int)blockIdx.x >= count) return;
  const int e = frozen[blockIdx.x];
  if (e < 0 || e >= ne.CB) return;
  const int c = e / ne.B, k = e % ne.B;
  double* __restrict__ col = ne.Et + (long long)c * ne.N3 * ne.B + k;
  for (int r = threadIdx.x; r < ne.N3; r += kFreezeThreads) col[(long long)r * ne.B] = 0.0;
  double* __restrict__ Ac = ne.A + (long long)c * ne.B * ne.B;
  for (int t = threadIdx.x; t < ne.B; t += kFreezeThreads) {
    const double v = t == k ? 1.0 : 0.0;
    Ac[k * ne.B + t] = v;
    Ac[t * ne.B + k] = v;
  }
  if (threadIdx.x == 0) ne.gc[e] = 0.0;
}

// ---- time shards: the blocks of the control points within `halo` of a cut receive rows from both neighbours --------
// Packed exchange buffer: [boundary b = 1 .. world-1][2*halo control points from cut_b - halo][3*CB cross | W*9 band | 3 grad].
// pack: this rank's partial blocks of its (<= 2) boundaries, everything else stays zero; after the sum over the ranks
// unpack overwrites the local blocks with the totals.
// (round 6: the launch also carries what used to be two launches of their own either side of the sum -- pack: this rank's PARTIAL
// diag(H) and g in x order (k_ne_diag_grad, raw); unpack: zeros of the summed diagonal -> 1)
__global__ void k_halo_copy(NEView ne, int halo, int nb, const int* __restrict__ bcut, const int* __restrict__ bidx, int Ntot,
                            double* __restrict__ buf, int unpack, DevProblem dp, double* __restrict__ D, double* __restrict__ gx, long long n) {
  const int per = 3 * ne.CB + ne.W * 9 + 3;
  const long long total = (long long)nb * 2 * halo * per;
  if (!unpack) {
    for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < ne.CB + ne.N3; e += (long long)gridDim.x * blockDim.x)
      ne_diag_grad_entry(dp, ne, 1, (int)e, D, gx);
  } else {
    for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x)
      if (!(D[e] > 0.0)) D[e] = 1.0;
  }
  for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
    const int f = (int)(e % per);
    const int ci = (int)((e / per) % (2 * halo)), b = (int)(e / ((long long)per * 2 * halo));
    const int ctrl = bcut[b] - halo + ci;              // global control point
    if (ctrl < 0 || ctrl >= Ntot) continue;
    const int l = ctrl - ne.row0;
    if (l < 0 || l >= ne.N) continue;                  // cannot happen: the slice spans its own range +- halo
    double* slot;
    if (f < 3 * ne.CB) { const int c = f / (3 * ne.B), dk = f % (3 * ne.B); slot = ne.Et + ((long long)c * ne.N3 + 3 * l) * ne.B + dk; }
    else if (f < 3 * ne.CB + ne.W * 9) slot = ne.Cb + (long long)l * ne.W * 9 + (f - 3 * ne.CB);
    else slot = ne.gs + 3 * l + (f - 3 * ne.CB - ne.W * 9);
    double* dst = buf + ((long long)bidx[b] * 2 * halo + ci) * per + f;
    if (unpack) *slot = *dst; else *dst = *slot;
  }
}

}  // namespace mvus
