// Registering cameras against a held trajectory (mvus_ba_register_cameras / mvus_ba_register_linearize): a batch of small independent
// least-squares problems -- one camera's alpha, beta, rs and P parameters against the control points of x, which are constants -- each
// solved by Levenberg-Marquardt entirely on the device.  The host enqueues a fixed schedule and reads back once:
//
//     evaluate(start)   { round(k) ; evaluate(trial k) }  k = 1 .. max_nfev - 1     round(last)   counts        evaluate = k_cam_states + k_reg_linearize
//
//   k_cam_states      (ba_observe.hip.h, the library's own) decodes the point in flight of every problem -- the batch laid out as the head
//                     of an x of B cameras -- so that a camera state has the bits it has in every other evaluation of the library.
//   k_reg_linearize   grid = slabs x problems.  A slab is kRegSlab consecutive detections of the problem's camera, one per lane; the
//                     partition of a camera depends on its detection count only.  Every lane evaluates its observation at the point in
//                     flight (eval_observation_to with a sink that keeps the 3 + P camera-side slots), scales the two rows by the loss and
//                     leaves them in LDS; then lane = ENTRY of the packed triangle / of g adds the rows in their order.  One partial per
//                     slab: triangle | g | twice the cost | visible.  The evaluation of a trial point is this kernel too: its cost decides
//                     on the trial, and its H, g are the linearisation of the next iteration when the trial is accepted (dropped otherwise).
//   k_reg_round       one wavefront per problem: the slab partials summed in slab order, then lane 0 runs reg_round (ba_register_math.h):
//                     decide on the trial in flight, adopt or drop its linearisation, gradient test, damped Cholesky, next trial point.
//   k_reg_counts      slabs x problems at the result: detections with a span, and those below the inlier threshold (integer sums).
//
// Workgroups of a finished problem return at once.  No floating-point atomics, no waiting between workgroups inside a launch: the launch
// boundaries are the only synchronisation, and every sum has one order -- a problem's result has the same bits alone, anywhere in any
// batch, and from run to run.  The call works in buffers of its own (RegisterWork): nothing the handle holds is read except the
// detections, the splines, the loss and the frozen mask, and nothing is written.
#pragma once
#include <hip/hip_runtime.h>

#include <cstring>
#include <exception>
#include <vector>

#include "api_common.h"      // MVUS_HIP
#include "ba_backend.hip.h"
#include "ba_dev_problem.h"
#include "ba_observe.hip.h"      // k_cam_states
#include "ba_register_math.h"
#include "ba_wave.hip.h"         // wave_sum

namespace mvus {

// one chunk of the batch on the device
struct RegBatch {
  int B, n;
  const int32_t* cam;        // [B] camera of problem b
  const int32_t* slab_off;   // [B + 1] first slab partial of problem b
  const uint32_t* held;      // [B] bit k < 18: entry k is held; bit 31: rs is boxed to [0, 1]
  const int32_t* nfree;      // [B] free unknowns (not held, not switched off)
  double* x;                 // [B][kRegMaxN] the accepted point
  double* xt;                // [B][kRegMaxN] the point in flight (the start, then the trials)
  double* xsoa;              // [B * n] the point the next evaluation runs at, laid out as the head of an x of B cameras: alpha(B) beta(B) rs(B) P each
  double* Hp;                // [B][kRegMaxTri] packed triangle at x, held entries taken out
  double* g;                 // [B][kRegMaxN]
  RegState* st;              // [B]
  double* part;              // [slabs][kRegPartial]
  unsigned long long* counts;   // [B][2] visible, inliers
};

template <bool CALIB>
__global__ __launch_bounds__(kRegSlab) void k_reg_linearize(DevProblem dp, const CamState* __restrict__ cams, const double* __restrict__ x, RegBatch rb, LossSpec loss) {
  constexpr int N = 3 + (CALIB ? 15 : 6), NT = N * (N + 1) / 2;
  const int b = blockIdx.y, slab = blockIdx.x;
  if (rb.st[b].done) return;
  const int c = rb.cam[b];
  const long long a = dp.det_off[c], Mc = dp.det_off[c + 1] - a;
  const long long first = (long long)slab * kRegSlab;
  if (first >= Mc) return;
  const int cnt = (int)(Mc - first < kRegSlab ? Mc - first : kRegSlab);
  __shared__ double rows[2 * kRegSlab][N + 1];            // the two scaled rows of lane t: 2 t and 2 t + 1; column N is the residual
  __shared__ double red[2][kRegSlab / 64];
  const CamState& cam = cams[b];                          // wave-uniform, decoded by k_cam_states: the bits every other evaluation of the library sees
  const int t = threadIdx.x;
  double cost2 = 0.0, vis = 0.0;
  if (t < cnt) {
    const long long i = a + first + t;
    const double uo = CALIB ? 0.0 : dp.u_obs[i], vo = CALIB ? 0.0 : dp.v_obs[i];
    const double ur = CALIB ? dp.u_raw[i] : 0.0;
    RegSink<N> sink;
#pragma unroll
    for (int k = 0; k < N; ++k) { sink.jx[k] = 0.0; sink.jy[k] = 0.0; }
    const ObsResult r = eval_observation_to<CALIB, true>(cam, dp.sp, x, dp.undist != 0, dp.rs_free != 0, dp.sync_free != 0, dp.frame[i], ur, dp.v_raw[i], uo, vo, sink);
    double fx = r.ex, fy = r.ey, sx = 1.0, sy = 1.0;
    if (r.ctrl >= 0) {
      vis = 1.0;
      if (loss.kind != 0) {
        cost2 = loss_rho(loss, r.ex) + loss_rho(loss, r.ey);
        sx = loss_scale_row(loss, fx); sy = loss_scale_row(loss, fy);
      } else cost2 = r.ex * r.ex + r.ey * r.ey;
    }
#pragma unroll
    for (int k = 0; k < N; ++k) { rows[2 * t][k] = sx * sink.jx[k]; rows[2 * t + 1][k] = sy * sink.jy[k]; }
    rows[2 * t][N] = fx; rows[2 * t + 1][N] = fy;
  }
  cost2 = wave_sum(cost2); vis = wave_sum(vis);
  if ((t & 63) == 0) { red[0][t >> 6] = cost2; red[1][t >> 6] = vis; }
  __syncthreads();
  double* __restrict__ out = rb.part + ((long long)rb.slab_off[b] + slab) * kRegPartial;
  for (int e = t; e < NT + N; e += kRegSlab) {
    int i, j;
    if (e < NT) reg_tri_entry(e, i, j); else { i = e - NT; j = N; }
    double acc = 0.0;
    for (int r = 0; r < 2 * cnt; ++r) acc += rows[r][i] * rows[r][j];
    out[e] = acc;
  }
  if (t == 0) {
    double s0 = 0.0, s1 = 0.0;
#pragma unroll
    for (int w = 0; w < kRegSlab / 64; ++w) { s0 += red[0][w]; s1 += red[1][w]; }
    out[NT + N] = s0; out[NT + N + 1] = s1;
  }
}

__global__ __launch_bounds__(64) void k_reg_round(RegBatch rb, RegOpts o, int first, int last) {
  const int b = blockIdx.x, lane = threadIdx.x;
  if (!first && rb.st[b].done) return;
  const int n = rb.n, nt = reg_tri(n);
  __shared__ double lin[kRegPartial], Hs[kRegMaxTri], L[kRegMaxTri], gs[kRegMaxN], xs[kRegMaxN], xts[kRegMaxN], p[kRegMaxN];
  __shared__ int fin;
  const int s0 = rb.slab_off[b], s1 = rb.slab_off[b + 1];
  for (int e = lane; e < nt + n + 2; e += 64) {
    double acc = 0.0;
    for (int s = s0; s < s1; ++s) acc += rb.part[(long long)s * kRegPartial + e];
    lin[e] = acc;
  }
  for (int e = lane; e < nt; e += 64) Hs[e] = first ? 0.0 : rb.Hp[(long long)b * kRegMaxTri + e];
  if (lane < n) {
    gs[lane] = first ? 0.0 : rb.g[(long long)b * kRegMaxN + lane];
    xs[lane] = rb.x[(long long)b * kRegMaxN + lane];
    xts[lane] = rb.xt[(long long)b * kRegMaxN + lane];
  }
  __syncthreads();
  if (lane == 0) {
    RegState s = rb.st[b];
    const uint32_t hb = rb.held[b];
    reg_round(n, first != 0, last != 0, o, hb & 0x3ffffu, (hb >> 31) != 0, rb.nfree[b], lin, s, xs, xts, Hs, gs, L, p);
    rb.st[b] = s;
    fin = (s.done || last) ? 1 : 0;
  }
  __syncthreads();
  for (int e = lane; e < nt; e += 64) rb.Hp[(long long)b * kRegMaxTri + e] = Hs[e];
  if (lane < n) {
    rb.g[(long long)b * kRegMaxN + lane] = gs[lane];
    rb.x[(long long)b * kRegMaxN + lane] = xs[lane];
    rb.xt[(long long)b * kRegMaxN + lane] = xts[lane];
    // where the next evaluation runs: the new trial, or -- the problem has ended (later rounds return at once) -- the result, for k_reg_counts
    const long long at = lane < 3 ? (long long)lane * rb.B + b : 3ll * rb.B + (long long)b * (n - 3) + (lane - 3);
    rb.xsoa[at] = fin ? xs[lane] : xts[lane];
  }
}

template <bool CALIB>
__global__ __launch_bounds__(kRegSlab) void k_reg_counts(DevProblem dp, const CamState* __restrict__ cams, const double* __restrict__ x, RegBatch rb, double thres) {
  const int b = blockIdx.y, slab = blockIdx.x;
  const int c = rb.cam[b];
  const long long a = dp.det_off[c], Mc = dp.det_off[c + 1] - a;
  const long long first = (long long)slab * kRegSlab;
  if (first >= Mc) return;
  const int cnt = (int)(Mc - first < kRegSlab ? Mc - first : kRegSlab);
  const CamState& cam = cams[b];
  const int t = threadIdx.x;
  bool vis = false, in = false;
  if (t < cnt) {
    const long long i = a + first + t;
    const double uo = CALIB ? 0.0 : dp.u_obs[i], vo = CALIB ? 0.0 : dp.v_obs[i];
    const double ur = CALIB ? dp.u_raw[i] : 0.0;
    RegSink<1> sink;
    const ObsResult r = eval_observation_to<CALIB, false>(cam, dp.sp, x, dp.undist != 0, dp.rs_free != 0, dp.sync_free != 0, dp.frame[i], ur, dp.v_raw[i], uo, vo, sink);
    vis = r.ctrl >= 0;
    in = vis && thres > 0 && sqrt(r.ex * r.ex + r.ey * r.ey) < thres;
  }
  const unsigned long long bv = __ballot(vis), bi = __ballot(in);
  if ((t & 63) == 0) {                                   // (integer sums: any order gives the same count)
    if (bv) atomicAdd(rb.counts + 2 * b, (unsigned long long)__popcll(bv));
    if (bi) atomicAdd(rb.counts + 2 * b + 1, (unsigned long long)__popcll(bi));
  }
}

// The buffers of the two calls, kept from call to call and grown when a batch needs more.
struct RegisterWork {
  DeviceOwner own;
  int64_t cap_n = 0, cap_B = 0, cap_slabs = 0;
  double* xfull = nullptr;
  int32_t *cam = nullptr, *slab_off = nullptr, *nfree = nullptr;
  uint32_t* held = nullptr;
  double *x = nullptr, *xt = nullptr, *xsoa = nullptr, *Hp = nullptr, *g = nullptr, *part = nullptr;
  double *Hsel = nullptr, *Ksel = nullptr, *dsel = nullptr;      // image height, fixed K and d of each problem's camera (k_cam_states reads them per "camera" b)
  CamState* cams = nullptr;
  RegState* st = nullptr;
  unsigned long long* counts = nullptr;
  bool ensure(hipStream_t stream, int64_t n, int64_t B, int64_t slabs) {      // true: everything was allocated anew (contents gone)
    if (n <= cap_n && B <= cap_B && slabs <= cap_slabs) return false;
    MVUS_HIP(hipStreamSynchronize(stream));
    // an allocation below may throw (a full card): the capacities say 0 until the last one has succeeded, so that the next call
    // allocates again and never runs on pointers that were freed here
    const int64_t new_n = std::max(cap_n, n), new_B = std::max(cap_B, B), new_slabs = std::max(cap_slabs, slabs);
    own.reset();
    cap_n = cap_B = cap_slabs = 0;
    xfull = own.device<double>((size_t)new_n);
    cam = own.device<int32_t>((size_t)new_B); slab_off = own.device<int32_t>((size_t)new_B + 1); nfree = own.device<int32_t>((size_t)new_B);
    held = own.device<uint32_t>((size_t)new_B);
    x = own.device<double>((size_t)new_B * kRegMaxN); xt = own.device<double>((size_t)new_B * kRegMaxN); xsoa = own.device<double>((size_t)new_B * kRegMaxN);
    Hsel = own.device<double>((size_t)new_B); Ksel = own.device<double>((size_t)new_B * 4); dsel = own.device<double>((size_t)new_B * 5);
    cams = own.device<CamState>((size_t)new_B);
    Hp = own.device<double>((size_t)new_B * kRegMaxTri); g = own.device<double>((size_t)new_B * kRegMaxN);
    part = own.device<double>((size_t)new_slabs * kRegPartial);
    st = own.device<RegState>((size_t)new_B);
    counts = own.device<unsigned long long>((size_t)new_B * 2);
    cap_n = new_n; cap_B = new_B; cap_slabs = new_slabs;
    return true;
  }
};

constexpr int64_t kRegChunkSlabs = 16384;      // slab partials in flight at once (24 MiB): a larger batch runs in several chunks of problems

struct RegisterOutputs {
  double *cam_out, *cost_out, *cost0_out;
  int32_t *nfev_out, *status_out;
  int64_t *visible_out, *inliers_out;
  double *H_out, *g_out;            // mvus_ba_register_linearize
};

// The whole call behind both entry points (arguments validated by the caller).  linearize_only: the first evaluation and the first
// round's adoption only -- H, g and the cost exactly as the solver's first iteration forms them.
inline int register_run(HipBackend& be, RegisterWork& w, const double* x, int32_t B, const int32_t* cam, const double* start, RegOpts o,
                        bool linearize_only, const RegisterOutputs& out) {
  const HostProblem& hp = be.hp;
  const int C = hp.C, P = hp.P, n = 3 + P;
  // per problem: start vector, held bits, free unknowns
  std::vector<double> xs((size_t)B * kRegMaxN, 0.0);
  std::vector<uint32_t> held((size_t)B, 0u);
  std::vector<int32_t> nfree((size_t)B, 0), slabs((size_t)B, 0);
  for (int32_t b = 0; b < B; ++b) {
    const int c = cam[b];
    double* v = &xs[(size_t)b * kRegMaxN];
    if (start) std::memcpy(v, start + (size_t)b * n, sizeof(double) * n);
    else {
      v[0] = x[c]; v[1] = x[C + c]; v[2] = x[2 * C + c];
      for (int k = 0; k < P; ++k) v[3 + k] = x[3 * C + (size_t)c * P + k];
    }
    uint32_t hb = 0;
    if (!be.frozen_mask.empty()) {
      for (int k = 0; k < 3; ++k) if (be.frozen_mask[(size_t)k * C + c]) hb |= 1u << k;
      for (int k = 0; k < P; ++k) if (be.frozen_mask[(size_t)3 * C + (size_t)c * P + k]) hb |= 1u << (3 + k);
    }
    int nf = 0;
    for (int k = 0; k < n; ++k) {
      const bool off = (k < 2 && !hp.sync_free) || (k == 2 && !hp.rs_free);
      if (!((hb >> k) & 1u) && !off) ++nf;
    }
    const bool boxed = hp.rs_bounds && !((hb >> 2) & 1u);
    if (boxed && !(v[2] >= 0.0 && v[2] <= 1.0)) {
      be.err = "register: rs of problem " + std::to_string(b) + " starts outside [0, 1] under rs_bounds";
      return MVUS_E_NUMERIC;
    }
    held[(size_t)b] = hb | (boxed ? 0x80000000u : 0u);
    nfree[(size_t)b] = nf;
    slabs[(size_t)b] = reg_slabs(hp.det_off[(size_t)c + 1] - hp.det_off[(size_t)c]);
  }
  const LossSpec loss = be.loss;
  hipStream_t st = be.stream;
  std::vector<RegState> hst;
  std::vector<unsigned long long> hcounts;
  std::vector<double> hx, hHp, hg, hsoa, hH, hK, hd;
  std::vector<int32_t> off;
  bool x_up = false;
  // the small tables below are copied from pageable vectors of this function: an exit by exception waits for the stream before they go
  struct Drain { hipStream_t st; ~Drain() { if (std::uncaught_exceptions() > 0) (void)hipStreamSynchronize(st); } } drain{st};
  for (int32_t b0 = 0; b0 < B;) {
    // the chunk: problems b0 .. b1 - 1, at most kRegChunkSlabs slab partials (always at least one problem)
    int32_t b1 = b0;
    int64_t total = 0;
    int maxs = 0;
    off.assign(1, 0);
    while (b1 < B && (b1 == b0 || total + slabs[(size_t)b1] <= kRegChunkSlabs)) {
      total += slabs[(size_t)b1]; maxs = std::max(maxs, slabs[(size_t)b1]); off.push_back((int32_t)total); ++b1;
    }
    const int Bc = b1 - b0;
    if (w.ensure(st, hp.n, Bc, total)) x_up = false;               // (a grown work space is a new buffer: a later chunk can hold more problems)
    if (!x_up) { be.upload(w.xfull, x, hp.n); x_up = true; }
    MVUS_HIP(hipMemcpyAsync(w.cam, cam + b0, sizeof(int32_t) * Bc, hipMemcpyHostToDevice, st));
    MVUS_HIP(hipMemcpyAsync(w.slab_off, off.data(), sizeof(int32_t) * (Bc + 1), hipMemcpyHostToDevice, st));
    MVUS_HIP(hipMemcpyAsync(w.held, &held[(size_t)b0], sizeof(uint32_t) * Bc, hipMemcpyHostToDevice, st));
    MVUS_HIP(hipMemcpyAsync(w.nfree, &nfree[(size_t)b0], sizeof(int32_t) * Bc, hipMemcpyHostToDevice, st));
    MVUS_HIP(hipMemcpyAsync(w.xt, &xs[(size_t)b0 * kRegMaxN], sizeof(double) * Bc * kRegMaxN, hipMemcpyHostToDevice, st));
    MVUS_HIP(hipMemcpyAsync(w.x, &xs[(size_t)b0 * kRegMaxN], sizeof(double) * Bc * kRegMaxN, hipMemcpyHostToDevice, st));
    hsoa.assign((size_t)Bc * n, 0.0); hH.resize((size_t)Bc); hK.assign((size_t)Bc * 4, 0.0); hd.assign((size_t)Bc * 5, 0.0);
    for (int k = 0; k < Bc; ++k) {
      const double* v = &xs[(size_t)(b0 + k) * kRegMaxN];
      const int c = cam[b0 + k];
      for (int e = 0; e < 3; ++e) hsoa[(size_t)e * Bc + k] = v[e];
      for (int e = 0; e < P; ++e) hsoa[(size_t)3 * Bc + (size_t)k * P + e] = v[3 + e];
      hH[(size_t)k] = hp.H[(size_t)c];
      if (!hp.calib) {
        for (int e = 0; e < 4; ++e) hK[(size_t)4 * k + e] = hp.K[(size_t)4 * c + e];
        for (int e = 0; e < 5; ++e) hd[(size_t)5 * k + e] = hp.dist[(size_t)5 * c + e];
      }
    }
    MVUS_HIP(hipMemcpyAsync(w.xsoa, hsoa.data(), sizeof(double) * Bc * n, hipMemcpyHostToDevice, st));
    MVUS_HIP(hipMemcpyAsync(w.Hsel, hH.data(), sizeof(double) * Bc, hipMemcpyHostToDevice, st));
    MVUS_HIP(hipMemcpyAsync(w.Ksel, hK.data(), sizeof(double) * Bc * 4, hipMemcpyHostToDevice, st));
    MVUS_HIP(hipMemcpyAsync(w.dsel, hd.data(), sizeof(double) * Bc * 5, hipMemcpyHostToDevice, st));
    MVUS_HIP(hipMemsetAsync(w.st, 0, sizeof(RegState) * Bc, st));
    MVUS_HIP(hipMemsetAsync(w.counts, 0, sizeof(unsigned long long) * 2 * Bc, st));
    const RegBatch rb{Bc, n, w.cam, w.slab_off, w.held, w.nfree, w.x, w.xt, w.xsoa, w.Hp, w.g, w.st, w.part, w.counts};
    DevProblem dpb = be.dp;                        // the batch as a problem of Bc cameras, for k_cam_states only
    dpb.C = Bc; dpb.H = w.Hsel; dpb.Kfix = w.Ksel; dpb.dfix = w.dsel;
    auto cam_states = [&] { hipLaunchKernelGGL(k_cam_states, dim3((unsigned)((Bc + 63) / 64)), dim3(64), 0, st, dpb, (const double*)w.xsoa, w.cams); };
    const dim3 grid((unsigned)std::max(maxs, 1), (unsigned)Bc);
    auto evaluate = [&] {
      if (maxs <= 0) return;
      cam_states();
      with_flag(hp.calib != 0, [&](auto calib) { hipLaunchKernelGGL(k_reg_linearize<calib()>, grid, dim3(kRegSlab), 0, st, be.dp, (const CamState*)w.cams, (const double*)w.xfull, rb, loss); });
    };
    auto round = [&](bool first, bool last) { hipLaunchKernelGGL(k_reg_round, dim3((unsigned)Bc), dim3(64), 0, st, rb, o, first ? 1 : 0, last ? 1 : 0); };
    evaluate();
    for (int k = 1; k < o.max_nfev; ++k) { round(k == 1, false); evaluate(); }
    round(o.max_nfev == 1, true);
    if (maxs > 0) {
      cam_states();
      with_flag(hp.calib != 0, [&](auto calib) { hipLaunchKernelGGL(k_reg_counts<calib()>, grid, dim3(kRegSlab), 0, st, be.dp, (const CamState*)w.cams, (const double*)w.xfull, rb, o.inlier_thres); });
    }
    MVUS_HIP(hipGetLastError());
    // the one read-back
    hst.resize((size_t)Bc); hcounts.resize((size_t)2 * Bc); hx.resize((size_t)Bc * kRegMaxN);
    MVUS_HIP(hipMemcpyAsync(hst.data(), w.st, sizeof(RegState) * Bc, hipMemcpyDeviceToHost, st));
    MVUS_HIP(hipMemcpyAsync(hcounts.data(), w.counts, sizeof(unsigned long long) * 2 * Bc, hipMemcpyDeviceToHost, st));
    MVUS_HIP(hipMemcpyAsync(hx.data(), w.x, sizeof(double) * Bc * kRegMaxN, hipMemcpyDeviceToHost, st));
    if (linearize_only) {
      hHp.resize((size_t)Bc * kRegMaxTri); hg.resize((size_t)Bc * kRegMaxN);
      MVUS_HIP(hipMemcpyAsync(hHp.data(), w.Hp, sizeof(double) * Bc * kRegMaxTri, hipMemcpyDeviceToHost, st));
      MVUS_HIP(hipMemcpyAsync(hg.data(), w.g, sizeof(double) * Bc * kRegMaxN, hipMemcpyDeviceToHost, st));
    }
    MVUS_HIP(hipStreamSynchronize(st));
    for (int k = 0; k < Bc; ++k) {
      const size_t b = (size_t)b0 + k;
      const RegState& s = hst[(size_t)k];
      if (out.cam_out) std::memcpy(out.cam_out + b * n, &hx[(size_t)k * kRegMaxN], sizeof(double) * n);
      if (out.cost_out) out.cost_out[b] = s.cost;
      if (out.cost0_out) out.cost0_out[b] = s.cost0;
      if (out.nfev_out) out.nfev_out[b] = s.nfev;
      if (out.status_out) out.status_out[b] = s.status;
      if (out.visible_out) out.visible_out[b] = (int64_t)hcounts[(size_t)2 * k];
      if (out.inliers_out) out.inliers_out[b] = (int64_t)hcounts[(size_t)2 * k + 1];
      if (out.H_out)
        for (int i = 0; i < n; ++i)
          for (int j = 0; j < n; ++j) out.H_out[(b * n + i) * n + j] = hHp[(size_t)k * kRegMaxTri + reg_tri_index(i, j)];
      if (out.g_out) std::memcpy(out.g_out + b * n, &hg[(size_t)k * kRegMaxN], sizeof(double) * n);
    }
    b0 = b1;
  }
  return MVUS_OK;
}

}  // namespace mvus
