// HipBackend: the HIP backend of the templated optimiser (the Backend concept of ba_solver.h and ba_schur.h) -- the device-resident
// problem, its evaluation kernels' launches, the reductions and scalar block, the work-vector pool and everything else a handle owns.
// Every BA entry point of ba_api.hip, HipSchur and CovChain go through it.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "api_common.h"      // HipError, MVUS_HIP, RoctxRange
#include "ba_held.h"
#include "ba_kernels.hip.h"      // the umbrella of the evaluation, operator, vector, LSMR, LM-tail and finite-difference kernels: nearly all are launched here
#include "ba_problem.h"
#include "ba_solver.h"
#include "ba_schur.h"
#include "ba_switches.h"
#include "ba_prior.hip.h"
#include "ba_landmark.hip.h"

namespace mvus {

static inline int grid_for(long long len) { return (int)std::min<long long>(2048, std::max<long long>(1, (len + kThreads - 1) / kThreads)); }

struct HipBackend {
  HostProblem hp;
  DevProblem dp{};
  // the stream this handle created (none when the caller brought one): declared in front of every DeviceOwner, so destroyed after them
  struct OwnStream { hipStream_t s = nullptr; ~OwnStream() { if (s) (void)hipStreamDestroy(s); } } own_stream;
  hipStream_t stream = nullptr;
  int device = 0;
  DeviceOwner own;                    // what lives as long as the handle: device buffers, the pinned scalars and staging ring, events
  // evaluation state
  CamState* cams = nullptr;
  const double* cams_for = nullptr;   // device x buffer whose camera states `cams` holds (nullptr: none); cleared when that buffer is rewritten
  double *J = nullptr, *mJ = nullptr, *x_cur = nullptr, *f_cur = nullptr;
  int32_t *span = nullptr, *pat0 = nullptr, *mctrl = nullptr;
  // first control point per detection (-1: not visible) at the x of the last residual-only evaluation: the window-major fused
  // assembly evaluates with a known knot span (`span` belongs to the held Jacobian and must survive residual evaluations)
  int32_t* rspan = nullptr;
  const double* rspan_for = nullptr;
  bool has_pattern = false, has_jacobian = false;
  const double* jac_x = nullptr;      // device x the held Jacobian was evaluated at (the priors' pass behind an assembly from J needs the point)
  bool held_analytic_at_xcur = false; // the held Jacobian is the analytic one of x_cur (mvus_ba_residual_jacobian): its normal equations can be formed by the fused window-major assembly
  bool det_assembly = false;          // mvus_ba_set_deterministic (kept for the ABI: the window-major assembly is deterministic by construction)
  bool pattern_uploaded = false;     // the caller supplied the reference's pattern (mvus_ba_upload_pattern): solve keeps it
  int32_t* ms_pat_dev = nullptr;
  double* det_alt[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};   // second set of detection arrays (remove_outliers ping-pong)
  int64_t det_capacity = 0;
  // reductions
  double *partials = nullptr, *scal_dev = nullptr, *scal_host = nullptr;
  double* scal_map = nullptr;     // device address of scal_host (mapped pinned memory): scalar results a kernel writes there need no copy kernel
  // who owns which double of the scalar block (scal_dev / scal_host / scal_map)
  enum ScalSlot : int {
    kDotNSlot = 0,                            // dot_n
    kDotMSlot = 1,                            // dot_m
    kRowCountSlot = 2,                        // the global row count on its way over the ranks (reduce_row_count)
    kCostSlot = 3,                            // a one-off cost: mvus_ba_robust_cost, mvus_ba_covariance, mvus_ba_time_kernel
    kPriorCostSlot = 4,                       // mvus_ba_position_prior_cost
    kLandmarkCostSlot = 5,                    // mvus_ba_landmark_cost
    kLmBase = 8,                              // the LM driver's block (LmSlot of ba_schur.h): lm_scalars()
    kFailSumSlot = kLmBase + kLmFailSum,      // ... whose tail is a time shard's failure sums: fetched with the trial's scalars
    kHostSumEnd = kFailSumSlot,               // residual_sq leaves a sum written below this slot to the host (fetch adds the partials)
    kMarkSlot = 24,                           // the start mark of fetch_poll_begin
    kScalCount = 32
  };
  static_assert(kDotNSlot < kDotMSlot && kDotMSlot < kRowCountSlot && kRowCountSlot < kCostSlot && kCostSlot < kPriorCostSlot && kPriorCostSlot < kLandmarkCostSlot &&
                    kLandmarkCostSlot < kLmBase,
                "one user per slot in front of the LM block");
  static_assert(kLmFailSum == kLmStepPSq + 1 && kLmSlots == kLmFailSum + 2, "the failure sums directly follow the trial's scalars: one fetch covers both");
  static_assert(kCostSlot < kHostSumEnd && kLmBase + kLmTrialCost < kHostSumEnd && kHostSumEnd <= kMarkSlot, "the host-summed range holds every |f|^2 slot and not the mark");
  static_assert(kLmBase + kLmSlots <= kMarkSlot && kMarkSlot < kScalCount, "the mark lies behind the LM block, inside the allocation");
  // pinned staging ring for the n-vectors that cross PCIe every solve / iteration (x, gradient, bounds): a copy from pageable
  // memory costs ~30 us of host-side staging per call and a synchronisation; through a pinned slot the upload is asynchronous
  static constexpr int kStageSlots = 4;
  double* stage[kStageSlots] = {nullptr, nullptr, nullptr, nullptr};
  hipEvent_t stage_ev[kStageSlots] = {nullptr, nullptr, nullptr, nullptr};
  int64_t stage_cap = 0;
  int stage_next = 0;
  // multi-GPU
  mvus_allreduce_fn allreduce = nullptr;
  void* allreduce_user = nullptr;
  int is_root = 1;
  int64_t m_glob = 0;
  // time shard (mvus_ba_set_time_shard): this handle holds the detections of one time slice and owns the control points
  // cuts[rank] .. cuts[rank+1]; the LM/Schur path then keeps the spline blocks of that slice (+- halo) only
  struct TimeShard { bool on = false; int rank = 0, world = 1, halo = 8; std::vector<int> cuts; } tshard;
  HandleMemory mem;                  // what the handle remembers from one API call to the next (ba_held.h): resume point, carry, damping, blocks' token
  // MVUS_JAC_FD
  int32_t* fd_groups = nullptr;
  int fd_ngroups = 0;
  double *fd_F = nullptr, *fd_h = nullptr, *fd_dx = nullptr, *fd_xg = nullptr;
  std::string err;
  Switches sw;                       // ba_switches.h: read once, in init

  template <class T>
  T* dalloc(size_t count) { return own.device<T>(count); }
  template <class T>
  T* dupload(const std::vector<T>& v) {
    T* p = dalloc<T>(v.size());
    if (!v.empty()) MVUS_HIP(hipMemcpyAsync(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, stream));
    return p;
  }

  void init(const mvus_problem* p) {
    sw = read_switches();
    device = p->device;
    MVUS_HIP(hipSetDevice(device));
    if (p->stream) stream = static_cast<hipStream_t>(p->stream);
    else { MVUS_HIP(hipStreamCreateWithFlags(&own_stream.s, hipStreamNonBlocking)); stream = own_stream.s; }
    dp.C = hp.C; dp.P = hp.P; dp.NS = hp.NS; dp.S = hp.S; dp.calib = hp.calib; dp.undist = hp.undist;
    dp.rs_free = hp.rs_free; dp.sync_free = hp.sync_free; dp.T = hp.T; dp.M = hp.M; dp.N = hp.N;
    det_capacity = std::max<int64_t>(hp.M, 1);
    dp.frame = dupload(hp.frame); dp.u_raw = dupload(hp.u_raw); dp.v_raw = dupload(hp.v_raw);
    dp.H = dupload(hp.H); dp.Kfix = dupload(hp.K); dp.dfix = dupload(hp.dist);
    dp.sp.S = hp.S; dp.sp.istart = dupload(hp.istart); dp.sp.iend = dupload(hp.iend); dp.sp.knots = dupload(hp.knots);
    dp.sp.knot_off = dupload(hp.knot_off); dp.sp.ctrl_off = dupload(hp.ctrl_off); dp.sp.xoff = dupload(hp.xoff);
    dp.sp.lut = dupload(hp.lut); dp.sp.lut_off = dupload(hp.lut_off); dp.sp.lut_scale = dupload(hp.lut_scale);
    dp.sp.info = dupload(hp.sinfo);
    dp.mv.T = hp.T; dp.mv.type = hp.motion_type; dp.mv.w = hp.w;
    dp.mv.t = dupload(hp.ms_t); dp.mv.basis = dupload(hp.ms_basis); dp.mv.ctrl = dupload(hp.ms_ctrl);
    dp.mv.part = dupload(hp.ms_part); ms_pat_dev = dupload(hp.ms_pat); dp.mv.pat = ms_pat_dev;
    dp.mv.ctrl_x0 = dupload(hp.ctrl_x0); dp.mv.ctrl_stride = dupload(hp.ctrl_stride);
    dp.mv.row_lo = dupload(hp.ms_row_lo); dp.mv.row_hi = dupload(hp.ms_row_hi);
    dp.chunk_cam = dupload(hp.chunk_cam); dp.chunk_count = dupload(hp.chunk_count); dp.chunks = dupload(hp.chunks);
    dp.cam_chunk_off = dupload(hp.cam_chunk_off);
    std::vector<long long> cs(hp.chunk_start.begin(), hp.chunk_start.end()), doff(hp.det_off.begin(), hp.det_off.end());
    dp.chunk_start = dupload(cs); dp.det_off = dupload(doff);
    dp.n_chunks = (int)hp.chunk_cam.size();
    dp.mot_lo = 0; dp.mot_hi = 0x7fffffff;
    double* uo = dalloc<double>(hp.M); double* vo = dalloc<double>(hp.M);
    dp.u_obs = uo; dp.v_obs = vo;
    cams = dalloc<CamState>(hp.C);
    span = dalloc<int32_t>(hp.M); pat0 = dalloc<int32_t>(hp.M); rspan = dalloc<int32_t>(hp.M);
    mJ = dalloc<double>((size_t)36 * hp.T); mctrl = dalloc<int32_t>((size_t)3 * hp.T);
    x_cur = dalloc<double>(hp.n); f_cur = alloc(hp.m);      // (from the pool: an LM solve swaps it with its trial buffer)
    partials = dalloc<double>(2048); scal_dev = dalloc<double>(kScalCount);
    scal_host = own.mapped<double>(kScalCount);
    for (int i = 0; i < kScalCount; ++i) scal_host[i] = 0.0;
    if (hipHostGetDevicePointer(reinterpret_cast<void**>(&scal_map), scal_host, 0) != hipSuccess) scal_map = nullptr;
    stage_cap = std::max<int64_t>(hp.n, 1024);
    for (int i = 0; i < kStageSlots; ++i) {
      stage[i] = own.pinned<double>(stage_cap);
      stage_ev[i] = own.event(hipEventDisableTiming);
    }
    MVUS_HIP(hipMemsetAsync(span, 0xff, sizeof(int32_t) * std::max<int64_t>(hp.M, 1), stream));
    MVUS_HIP(hipMemsetAsync(pat0, 0xff, sizeof(int32_t) * std::max<int64_t>(hp.M, 1), stream));
    MVUS_HIP(hipMemsetAsync(mctrl, 0xff, sizeof(int32_t) * std::max<int64_t>(3 * hp.T, 1), stream));
    if (dp.n_chunks > 0) {
      if (!hp.calib && hp.undist) hipLaunchKernelGGL(k_undistort_fixed, dim3(dp.n_chunks), dim3(kThreads), 0, stream, dp, uo, vo);
      else {
        MVUS_HIP(hipMemcpyAsync(uo, dp.u_raw, sizeof(double) * hp.M, hipMemcpyDeviceToDevice, stream));
        MVUS_HIP(hipMemcpyAsync(vo, dp.v_raw, sizeof(double) * hp.M, hipMemcpyDeviceToDevice, stream));
      }
    }
    MVUS_HIP(hipGetLastError());
    MVUS_HIP(hipStreamSynchronize(stream));
    m_glob = hp.m;
  }

  ~HipBackend() {
    (void)hipSetDevice(device);
    if (stream) (void)hipStreamSynchronize(stream);      // (the owners free after this, the stream goes last: order of declaration)
  }

  // ---- Backend concept -------------------------------------------------------------------------
  int64_t n() const { return hp.n; }
  int64_t m_local() const { return hp.m; }
  int64_t m_global() const { return m_glob; }
  // work vectors come from a size-keyed free list: the solvers allocate and release the same handful of n- and
  // m-sized buffers on every call, and hipMalloc/hipFree cost far more than the kernels they feed
  std::map<size_t, std::vector<double*>> pool_free;
  std::map<double*, size_t> pool_size;
  DeviceOwner pool_own;               // the pool's memory; pool_size / pool_free are the size classes
  double* alloc(int64_t len) {
    const size_t bytes = (size_t)std::max<int64_t>(len, 1) * sizeof(double);
    auto it = pool_free.find(bytes);
    if (it != pool_free.end() && !it->second.empty()) { double* p = it->second.back(); it->second.pop_back(); touch(p); return p; }
    double* p = pool_own.device<double>(bytes / sizeof(double));
    pool_size[p] = bytes;
    return p;
  }
  // stream-ordered reuse: one stream per handle.  A buffer that leaves or re-enters the pool no longer names an x whose camera
  // states are cached (not every writer of an n-vector calls touch(): J^T u, the Schur kernels); the invariant is kept HERE
  void release(double* p) { if (p) { touch(p); pool_free[pool_size[p]].push_back(p); } }
  // decoded camera states are reused while the x buffer they came from is untouched (the accepted point of an LM iteration
  // is the trial point whose states are already there; a 2-evaluation solve evaluates and linearises at the same x)
  void touch(const double* d) { if (d == cams_for) cams_for = nullptr; if (d == rspan_for) rspan_for = nullptr; }
  void ensure_cams(const double* x) {
    if (cams_for == x) return;
    hipLaunchKernelGGL(k_cam_states, dim3((hp.C + 63) / 64), dim3(64), 0, stream, dp, x, cams);
    cams_for = x;
  }
  int stage_slot() {                          // next pinned slot, free again once the copy that last used it has run
    const int slot = stage_next;
    stage_next = (stage_next + 1) % kStageSlots;
    MVUS_HIP(hipEventSynchronize(stage_ev[slot]));
    return slot;
  }
  void upload(double* d, const double* s, int64_t len) {      // the host buffer may be reused right away
    touch(d);
    if (d == x_cur) held_analytic_at_xcur = false;
    if (len <= stage_cap) {
      const int slot = stage_slot();
      std::memcpy(stage[slot], s, len * sizeof(double));
      MVUS_HIP(hipMemcpyAsync(d, stage[slot], len * sizeof(double), hipMemcpyHostToDevice, stream));
      MVUS_HIP(hipEventRecord(stage_ev[slot], stream));
      return;
    }
    MVUS_HIP(hipMemcpyAsync(d, s, len * sizeof(double), hipMemcpyHostToDevice, stream));
    MVUS_HIP(hipStreamSynchronize(stream));
  }
  void download(double* d, const double* s, int64_t len) {
    if (len <= stage_cap) {
      const int slot = stage_slot();
      MVUS_HIP(hipMemcpyAsync(stage[slot], s, len * sizeof(double), hipMemcpyDeviceToHost, stream));
      MVUS_HIP(hipStreamSynchronize(stream));
      std::memcpy(d, stage[slot], len * sizeof(double));
      return;
    }
    MVUS_HIP(hipMemcpyAsync(d, s, len * sizeof(double), hipMemcpyDeviceToHost, stream));
    MVUS_HIP(hipStreamSynchronize(stream));
  }
  void copy(double* d, const double* s, int64_t len) { touch(d); if (d != s) MVUS_HIP(hipMemcpyAsync(d, s, len * sizeof(double), hipMemcpyDeviceToDevice, stream)); }
  void fill(double* d, double v, int64_t len) {
    touch(d);
    const int tiles = grid_for(len);
    if (len > 0) hipLaunchKernelGGL(k_fill, dim3(xcd_grid(tiles)), dim3(kThreads), 0, stream, (long long)len, v, d, tiles);
  }
  void axpby(int64_t len, double a, const double* x, double b, const double* y, double* out) {
    touch(out);
    if (len > 0) hipLaunchKernelGGL(k_axpby, dim3(grid_for(len)), dim3(kThreads), 0, stream, (long long)len, a, x, b, y, out);
  }
  void mul(int64_t len, const double* x, const double* y, double* out) {
    touch(out);
    if (len > 0) hipLaunchKernelGGL(k_mul, dim3(grid_for(len)), dim3(kThreads), 0, stream, (long long)len, x, y, out);
  }
  // two launches (partials, then their sum): a single launch with a last-workgroup ticket was measured at 22.9 us against
  // 2 x 4.9 us -- the agent-scope release fence every workgroup needs before its ticket costs more than a launch
  void dot_into(const double* a, const double* b, int64_t len, double* out) {
    const int nb = grid_for(len);
    if (len > 0) {
      hipLaunchKernelGGL(k_dot_partial, dim3(nb), dim3(kThreads), 0, stream, (long long)len, a, b, partials);
      hipLaunchKernelGGL(k_dot_final, dim3(1), dim3(kThreads), 0, stream, nb, partials, out);
    } else {
      MVUS_HIP(hipMemsetAsync(out, 0, sizeof(double), stream));
    }
  }
  // Where the scalars the host reads after every step are written.  One rank: straight into the mapped pinned mirror (the host
  // reads it after a stream synchronisation: no device-to-host copy kernel, ~4 us + a launch per fetch).  With an all-reduce
  // callback the scalars are summed over the ranks in device memory first, so they stay there and are copied.
  bool scal_direct() const { return scal_map != nullptr && !allreduce; }
  double* scal_out() { return scal_direct() ? scal_map : scal_dev; }
  void dot_to_slot(const double* a, const double* b, int64_t len, int slot) { dot_into(a, b, len, scal_out() + slot); }
  double read_slot(int slot) {
    if (!scal_direct()) MVUS_HIP(hipMemcpyAsync(scal_host + slot, scal_dev + slot, sizeof(double), hipMemcpyDeviceToHost, stream));
    MVUS_HIP(hipStreamSynchronize(stream));
    return scal_host[slot];
  }
  void reduce(double* buf, size_t count) {
    if (!allreduce) return;
    RoctxRange range("mvus all-reduce");
    if (allreduce(allreduce_user, buf, count, stream) != 0) throw HipError{"all-reduce callback failed", MVUS_E_COMM};
  }
  // a shard filters its own detections; only the global row count is shared: the shards' detection rows + the motion rows once
  void reduce_row_count() {
    const bool counts_motion = tshard.on ? tshard.rank == 0 : is_root != 0;
    scal_host[kRowCountSlot] = (double)(2 * hp.M + (counts_motion ? hp.T : 0));
    MVUS_HIP(hipMemcpyAsync(scal_dev + kRowCountSlot, scal_host + kRowCountSlot, sizeof(double), hipMemcpyHostToDevice, stream));
    reduce(scal_dev + kRowCountSlot, 1);
    m_glob = (int64_t)(read_slot(kRowCountSlot) + 0.5);
  }
  // device-resident LM driver (ba_schur.h)
  std::vector<double> lb_host, ub_host, lb_fixed, ub_fixed;
  bool fixed_bounds_on_device = false;
  double *lb_dev = nullptr, *ub_dev = nullptr;
  double* tr_pn2 = nullptr;         // |p|^2 of the damped step (trust region of the LM driver)
  bool reshard_flag = false;        // set by HipSchur::solve_ok when a row left the time slice
  bool reshard_pending() { const bool r = reshard_flag; reshard_flag = false; return r; }
  // current / trial point of the LM driver, kept from solve to solve; which of the two holds the point the last solve returned, and
  // what that solve left valid there, is the handle's memory (ba_held.h) -- the driver's names for it (ba_schur.h):
  double* lm_x[2] = {nullptr, nullptr};
  double* lm_xbuf(int k) { if (!lm_x[k]) lm_x[k] = dalloc<double>(std::max<int64_t>(hp.n, 1)); return lm_x[k]; }
  int lm_resume(const double* x_host) { return mem.resume(x_host, hp.n, !allreduce); }
  void lm_remember(const double* x_dev, const double* x_host, const double* mirror) { mem.remember(x_dev == lm_x[0] ? 0 : (x_dev == lm_x[1] ? 1 : -1), x_host, hp.n, mirror); }
  LmCarry lm_carry(int jac_mode) { return mem.take_carry(jac_mode, !allreduce && !sw.lm_no_carry); }
  void lm_keep(const LmCarry& c, int jac_mode) { mem.keep_carry(c, jac_mode); }
  // fetch_mark: the next fetch waits for the work enqueued so far only (an event), not for what is enqueued after the mark -- the
  // speculative linearisation of the LM driver.  Needs the scalars written straight into mapped memory (one rank).
  // fetch_poll_begin: the same without an event (hipEventRecord costs a 6 us bubble between the two kernels it separates): the FIRST
  // kernel enqueued after the point writes *mark = value when it starts -- it cannot start before everything in front of it has
  // finished and released its writes -- and the fetch spins on that word in mapped memory.
  double fetch_seq = 0.0;
  bool fetch_polled = false;
  bool fetch_poll_begin(double** mark, double* value) {
    if (scal_map == nullptr || sw.fetch_event) return false;      // (the mark itself is always written through mapped memory)
    fetch_seq += 1.0;
    *mark = scal_map + kMarkSlot; *value = fetch_seq;
    fetch_polled = true;
    return true;
  }
  // sharded handles (scalars in device memory, copied out): the copy a later fetch() reads is enqueued NOW, in front of speculative work
  bool fetch_queued = false;
  int64_t fq_off = 0;
  int fq_k = 0;
  void fetch_enqueue(const double* src, int k) {
    if (scal_direct()) return;
    fq_off = src - scal_out(); fq_k = k;
    MVUS_HIP(hipMemcpyAsync(scal_host + fq_off, src, sizeof(double) * k, hipMemcpyDeviceToHost, stream));
    fetch_queued = true;
  }
  bool spec_on_shards() const { return scal_map != nullptr && !sw.no_spec_shards; }
  hipEvent_t fetch_ev = nullptr;
  bool fetch_marked = false;
  void fetch_mark() {
    if (!fetch_ev) fetch_ev = own.event(hipEventDisableTiming);
    MVUS_HIP(hipEventRecord(fetch_ev, stream));
    fetch_marked = true;
  }
  unsigned* lm_counter = nullptr;   // ticket counter of the last-block reductions (k_lm_gnorm / k_lm_trial), kept at 0 between launches
  void set_bounds(const std::vector<double>& lb, const std::vector<double>& ub) {
    if (!lb_dev) {
      lb_dev = dalloc<double>(hp.n); ub_dev = dalloc<double>(hp.n); lm_counter = dalloc<unsigned>(1);
      MVUS_HIP(hipMemsetAsync(lm_counter, 0, sizeof(unsigned), stream));
    }
    if (&lb == &lb_fixed && &ub == &ub_fixed && fixed_bounds_on_device) return;      // (the handle's own vectors, uploaded before)
    if (lb != lb_host) { lb_host = lb; upload(lb_dev, lb_host.data(), hp.n); }
    if (ub != ub_host) { ub_host = ub; upload(ub_dev, ub_host.data(), hp.n); }
    fixed_bounds_on_device = &lb == &lb_fixed && &ub == &ub_fixed;
  }
  const double* lb_ptr() const { return lb_dev; }
  const double* ub_ptr() const { return ub_dev; }
  double* lm_scalars() { return scal_out() + kLmBase; }
  void dot_m_into(const double* a, const double* b, double* out) {
    dot_into(a, b, hp.m, out);
    reduce(out, 1);
  }
  // the two vector reductions of an LM iteration: one workgroup up to 128k parameters (no cross-workgroup fences), else one per 1024
  unsigned lm_grid() const { return hp.n <= (1 << 17) ? 1u : (unsigned)std::min<int64_t>(2048 / 5, (hp.n + 1023) / 1024); }
  void lm_gnorm(const double* x, const double* lb, const double* ub, const double* g, double* out) {
    hipLaunchKernelGGL(k_lm_gnorm, dim3(lm_grid()), dim3(1024), 0, stream, (int)hp.n, x, lb, ub, g, out, partials, lm_counter);
  }
  // Two mapped pinned mirrors of the trial point (ping-pong with the accepted / trial roles of the LM driver): the trial kernel
  // writes x_new there as well, so that the host holds the accepted point after the fetch that decides on it and the solve ends
  // without a device-to-host copy and its synchronisation.  One rank only (like the mapped scalars); else nullptr -> download.
  static constexpr bool kSwapResiduals = true;          // f at an accepted point: the trial buffer changes roles with f_cur, no copy
  double* xmir_host[2] = {nullptr, nullptr};
  double* xmir_dev[2] = {nullptr, nullptr};
  int64_t xmir_cap = 0;
  DeviceOwner xmir_own;
  double* mirror_dev(int k) {
    if (!scal_direct()) return nullptr;
    if (xmir_cap < hp.n) {
      xmir_own.reset();
      for (int i = 0; i < 2; ++i) xmir_host[i] = xmir_dev[i] = nullptr;
      for (int i = 0; i < 2; ++i) {
        xmir_host[i] = xmir_own.mapped<double>((size_t)hp.n);
        if (hipHostGetDevicePointer(reinterpret_cast<void**>(&xmir_dev[i]), xmir_host[i], 0) != hipSuccess) xmir_dev[i] = nullptr;
      }
      xmir_cap = hp.n;
    }
    return xmir_dev[k];
  }
  // (the mirror of slot k holds the trial point only while the trial kernel writes it: not once an all-reduce route was installed on
  // a handle that had solved on one rank before -- the caller then downloads x)
  const double* mirror_host(int k) const { return scal_direct() ? xmir_host[k] : nullptr; }
  void adopt_residual(double*& f_dev, double*& f_new) {       // both are pool buffers of one size class
    if (f_dev == f_cur) f_cur = f_new;
    std::swap(f_dev, f_new);
  }
  void lm_trial(const double* x, const double* p, const double* lb, const double* ub, const double* g, const double* D,
                const int* fail, double* x_new, double* out, double* gnorm_out, double* x_mirror, double* pn2 = nullptr, double delta = 0.0,
                const double* fail_sum = nullptr) {
    touch(x_new);
    double* const fail_out = scal_out() + kFailSumSlot;
    // trust region: |p|^2 first (two small launches), the trial kernel then cuts the step back to delta along its direction
    double* pn2_dev = nullptr;
    if (pn2) { if (!tr_pn2) tr_pn2 = dalloc<double>(1); pn2_dev = tr_pn2; dot_into(p, p, hp.n, pn2_dev); }
    // one workgroup is limited by what one CU can load (six n-vectors: 18 us at n = 15k); a few workgroups and a second, tiny
    // launch for their partials take 10 us.  Beyond 128k parameters: the one-launch form with the last-workgroup hand-over.
    const unsigned g2 = hp.n > 2048 && hp.n <= (1 << 17) ? (unsigned)std::min<int64_t>(32, (hp.n + 1023) / 1024) : 0u;
    if (g2 > 1) {
      hipLaunchKernelGGL(k_lm_trial, dim3(g2), dim3(1024), 0, stream, (int)hp.n, x, p, lb, ub, g, D, fail, x_new, out, gnorm_out, partials, (unsigned*)nullptr, x_mirror, (const double*)pn2_dev, delta, fail_sum, fail_out);
      hipLaunchKernelGGL(k_lm_trial_sum, dim3(1), dim3(64), 0, stream, (int)g2, partials, out, gnorm_out, dp, (const double*)x_new, cams);
      cams_for = x_new;                      // decoded by that launch: the trial residual needs no k_cam_states
      return;
    }
    hipLaunchKernelGGL(k_lm_trial, dim3(lm_grid()), dim3(1024), 0, stream, (int)hp.n, x, p, lb, ub, g, D, fail, x_new, out, gnorm_out, partials, lm_counter, x_mirror, (const double*)pn2_dev, delta, fail_sum, fail_out);
  }
  // (spinning on a sentinel in the mapped scalars instead of hipStreamSynchronize was measured in round 5: 0.509 against 0.509 ms per
  // step, three A/B pairs on one box -- the runtime's own wait already spins; not kept)
  void fetch(const double* src, int k, double* host) {       // src inside scal_out(): the pinned mirror itself, or staged through it
    const int64_t off = src - scal_out();
    const bool queued = fetch_queued && off >= fq_off && off + k <= fq_off + fq_k;
    if (!scal_direct() && !queued) MVUS_HIP(hipMemcpyAsync(scal_host + off, src, sizeof(double) * k, hipMemcpyDeviceToHost, stream));
    fetch_queued = false;
    if (fetch_polled && (scal_direct() || queued)) {
      const volatile double* m = scal_host + kMarkSlot;
      const auto t0 = std::chrono::steady_clock::now();
      unsigned spins = 0;
      while (*m != fetch_seq) {
        if ((++spins & 0xfff) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(5)) { MVUS_HIP(hipStreamSynchronize(stream)); break; }   // (never seen; the stream then tells)
        __builtin_ia32_pause();
      }
      std::atomic_thread_fence(std::memory_order_acquire);
    } else if (fetch_marked && (scal_direct() || queued)) MVUS_HIP(hipEventSynchronize(fetch_ev));
    else MVUS_HIP(hipStreamSynchronize(stream));
    fetch_marked = false; fetch_polled = false;
    for (SqPending& sp : sq_pend)                         // sums of squares left as per-workgroup partials in mapped memory (residual_sq)
      if (sp.slot >= off && sp.slot < off + k) { scal_host[sp.slot] = sq_host_sum(sqh_host[&sp - sq_pend], sp.n); sp.slot = -1; }
    for (int i = 0; i < k; ++i) host[i] = scal_host[off + i];
  }
  double dot_n(const double* a, const double* b, int64_t len) { dot_to_slot(a, b, len, kDotNSlot); return read_slot(kDotNSlot); }
  double dot_m(const double* a, const double* b) { dot_to_slot(a, b, hp.m, kDotMSlot); reduce(scal_out() + kDotMSlot, 1); return read_slot(kDotMSlot); }

  // the slot Jacobian (2*NS*M doubles) is allocated on first use: residual-only handles (Scene.error_cam, outlier masks) never pay for it
  void ensure_J() { if (!J) J = dalloc<double>(j_doubles(hp.NS, dp.n_chunks)); }      // sized at first use; outlier removal only ever shrinks the chunk table
  void eval(const double* x, double* f, bool jac, int jac_mode) {
    RoctxRange range(jac ? "mvus residual+jacobian" : "mvus residual");
    if (jac) ensure_J();
    const bool masked = jac && jac_mode == MVUS_JAC_PATTERN;
    if (masked && !has_pattern) throw HipError{"MVUS_JAC_PATTERN needs mvus_ba_set_pattern (or solve) first"};
    ensure_cams(x);
    if (dp.n_chunks > 0) {
      const dim3 g(dp.n_chunks), gj(xcd_grid(dp.n_chunks)), b(kThreads);
      with_flag(hp.calib, [&](auto calib) {
        if (jac) hipLaunchKernelGGL((k_observations<calib(), true>), gj, b, 0, stream, dp, cams, x, f, J, span, pat0, (int)masked);
        else hipLaunchKernelGGL((k_observations<calib(), false>), g, b, 0, stream, dp, cams, x, f, J, rspan, pat0, 0);
      });
      if (!jac) rspan_for = x;
    }
    if (hp.T > 0) {
      if (is_root || tshard.on) {
        const dim3 g((hp.T + kThreads - 1) / kThreads), b(kThreads);
        if (jac) hipLaunchKernelGGL(k_motion<true>, g, b, 0, stream, dp, x, f + 2 * hp.M, mJ, mctrl, (int)masked);
        else hipLaunchKernelGGL(k_motion<false>, g, b, 0, stream, dp, x, f + 2 * hp.M, mJ, mctrl, 0);
      } else {
        // sharded run: the (replicated) motion rows are owned by the root rank; here they are rows of zeros
        // (mctrl stays -1 from initialisation, so they contribute nothing to J v, J^T u or the normal equations)
        MVUS_HIP(hipMemsetAsync(f + 2 * hp.M, 0, sizeof(double) * hp.T, stream));
      }
    }
    MVUS_HIP(hipGetLastError());
    if (jac) { has_jacobian = true; jac_x = x; }
  }
  void residual(const double* x, double* f) { eval(x, f, false, 0); }
  // f = f(x) and out = |f|^2 (summed over the ranks): on one rank the residual kernels leave their workgroups' sums of squares
  // behind and one small launch adds them -- no separate pass over f
  double* sq_part = nullptr;
  size_t sq_cap = 0;
  // One rank (scalars in mapped memory): the workgroups' partial sums go to mapped pinned HOST memory and the host adds them after
  // the fetch's wait, in k_dot_final's own tree (sq_host_sum: the same bits) -- the 4.4 - 5 us launch of k_dot_final behind every
  // residual evaluation of the LM driver is gone.  Two sets: the start's |f|^2 and the first trial's are both outstanding at the
  // first fetch of a solve.  MVUS_SQ_DEVICE_SUM=1 keeps the launch (A/B).
  double* sqh_host[2] = {nullptr, nullptr};
  double* sqh_dev[2] = {nullptr, nullptr};
  size_t sqh_cap = 0;
  DeviceOwner sqh_own;
  struct SqPending { int64_t slot = -1; int n = 0; } sq_pend[2];
  static double sq_host_sum(const double* part, int nb) {
    double red[kThreads / 64];
    for (int w = 0; w < kThreads / 64; ++w) {
      double lane[64];
      for (int l = 0; l < 64; ++l) {                       // k_dot_final: thread t adds partials t, t + kThreads, ...
        double a = 0.0;
        for (int i = w * 64 + l; i < nb; i += kThreads) a += part[i];
        lane[l] = a;
      }
      for (int off = 32; off > 0; off >>= 1)                // wave_sum as lane 0 sees it
        for (int l = 0; l < off; ++l) lane[l] += lane[l + off];
      red[w] = lane[0];
    }
    double t = 0.0;
    for (int w = 0; w < kThreads / 64; ++w) t += red[w];
    return t;
  }
  // The loss in force (mvus_ba_set_loss; kind 0 = linear).  With another kind the partial sums below are those of f_scale^2 rho(z) -- the
  // LM driver's cost, trial cost and gain ratio are the robust ones with no change to the driver -- and HipSchur's assembly kernels scale
  // the rows as they read them; f in memory is the raw error_BA throughout.  (Sharded handles refuse a loss: mvus_ba_solve.)
  LossSpec loss{0, 1.0};
  bool robust() const { return loss.kind != 0; }
  // Camera-side unknowns held constant (mvus_ba_set_frozen), state of the handle like the loss.  frozen_mask: the caller's mask over the
  // head of x in pack_x order (empty = none); on the device the same set twice, in the solvers' internal order e = c * B + slot: the list
  // of frozen entries (k_freeze_ne, LM + Schur: one workgroup each) and a byte per entry (k_freeze_jacobian, TRF + LSMR).  An all-zero mask
  // is no mask: frozen_count = 0 and no kernel, argument or branch on the device differs from a handle that never had one.
  std::vector<uint8_t> frozen_mask;
  int32_t* frozen_idx = nullptr;
  uint8_t* frozen_slot = nullptr;
  int frozen_count = 0;
  bool freeze_stored_jacobian = false;      // inside mvus_ba_solve: every Jacobian evaluation is followed by k_freeze_jacobian
  void set_frozen(const uint8_t* mask, int64_t count) {
    const int B = 3 + hp.P, CB = hp.C * B;
    std::vector<int32_t> idx;
    std::vector<uint8_t> slot((size_t)CB, 0);
    for (int64_t k = 0; k < count; ++k) {
      if (!mask[k]) continue;
      const int e = k < 3 * hp.C ? (int)(k % hp.C) * B + (int)(k / hp.C) : (int)((k - 3 * hp.C) / hp.P) * B + 3 + (int)((k - 3 * hp.C) % hp.P);
      idx.push_back(e); slot[(size_t)e] = 1;
    }
    if (!idx.empty()) {
      if (!frozen_idx) { frozen_idx = dalloc<int32_t>((size_t)CB); frozen_slot = dalloc<uint8_t>((size_t)CB); }
      MVUS_HIP(hipMemcpyAsync(frozen_idx, idx.data(), idx.size() * sizeof(int32_t), hipMemcpyHostToDevice, stream));
      MVUS_HIP(hipMemcpyAsync(frozen_slot, slot.data(), slot.size(), hipMemcpyHostToDevice, stream));
      MVUS_HIP(hipStreamSynchronize(stream));
      frozen_mask.assign(mask, mask + count);
    } else frozen_mask.clear();
    frozen_count = (int)idx.size();
  }
  void freeze_jacobian() {
    if (frozen_count <= 0 || dp.n_chunks <= 0) return;
    with_flag(hp.calib, [&](auto calib) { hipLaunchKernelGGL(k_freeze_jacobian<calib() ? 30 : 21>, dim3(dp.n_chunks), dim3(kThreads), 0, stream, dp, (const uint8_t*)frozen_slot, J); });
    MVUS_HIP(hipGetLastError());
  }
  // Position priors on the trajectory (mvus_ba_set_position_priors, ba_prior.hip.h), state of the handle like the loss and the mask, kept
  // over remove_outliers (they hang on the control points, which outlier removal leaves alone).  prior.K counts what the caller set,
  // prior_active those whose time lies in an interval: with prior_active = 0 no kernel, argument or branch on the device differs from a
  // handle that never had any.
  PriorView prior{};
  DeviceOwner prior_own;
  std::vector<int64_t> prior_perm;          // sorted position -> the caller's index
  int prior_active = 0;
  uint64_t prior_gen = 0, prior_sets = 0;   // prior_gen names the set in force (HipSchur::assemble_held: which priors held blocks carry)
  int64_t prior_rows = 0;                   // active (prior, axis) pairs with w > 0: the rows the covariance's degrees of freedom count
  int prior_blocks() const { return prior_active > 0 ? (int)std::min<int64_t>(2048, ((int64_t)prior.K + kThreads - 1) / kThreads) : 0; }
  void clear_priors() {
    if (!prior_own.empty()) MVUS_HIP(hipStreamSynchronize(stream));
    prior_own.reset(); prior_perm.clear();
    prior = PriorView{}; prior_active = 0; prior_rows = 0;
  }
  template <class T>
  T* prior_upload(const std::vector<T>& v) {
    T* p = prior_own.device<T>(v.size());
    if (!v.empty()) MVUS_HIP(hipMemcpyAsync(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, stream));
    return p;
  }
  // t[K], P[3K], w[3K] in the caller's order (validated): sorted by (t, input order), span and weights by k_prior_setup, then the rows
  // per control point on the host from the spans it found
  void set_priors(int64_t K, const double* t, const double* P, const double* w) {
    if (K <= 0) { clear_priors(); return; }
    std::vector<int64_t> perm((size_t)K);
    for (int64_t k = 0; k < K; ++k) perm[(size_t)k] = k;
    std::stable_sort(perm.begin(), perm.end(), [&](int64_t a, int64_t b) { return t[a] < t[b]; });
    std::vector<double> ts((size_t)K), ps((size_t)3 * K), ws((size_t)3 * K);
    for (int64_t k = 0; k < K; ++k) {
      ts[(size_t)k] = t[perm[(size_t)k]];
      for (int d = 0; d < 3; ++d) { ps[(size_t)(d * K + k)] = P[d * K + perm[(size_t)k]]; ws[(size_t)(d * K + k)] = w[d * K + perm[(size_t)k]]; }
    }
    clear_priors();
    std::vector<int32_t> ctrl((size_t)K, -1);
    const std::vector<double> hz((size_t)4 * K, 0.0);      // (pageable sources of asynchronous copies: alive until the synchronisation below)
    PriorView pv{};      // built aside: a failure below leaves the handle without priors (the buffers go at the next clear_priors)
    pv.K = (int)K;
    pv.t = prior_upload(ts); pv.p = prior_upload(ps); pv.w = prior_upload(ws);
    pv.ctrl = prior_upload(ctrl); pv.h = prior_upload(hz);
    hipLaunchKernelGGL(k_prior_setup, dim3((unsigned)((K + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, dp.sp, pv);
    MVUS_HIP(hipGetLastError());
    MVUS_HIP(hipMemcpyAsync(ctrl.data(), pv.ctrl, sizeof(int32_t) * K, hipMemcpyDeviceToHost, stream));
    MVUS_HIP(hipStreamSynchronize(stream));
    const int N = hp.N;
    std::vector<int32_t> lo((size_t)std::max(N, 1), 0), hi((size_t)std::max(N, 1), 0);
    int active = 0;
    int64_t rows = 0;
    for (int64_t k = 0; k < K; ++k) {
      const int c0 = ctrl[(size_t)k];
      if (c0 < 0) continue;
      if (c0 + 3 >= N) throw HipError{"set_position_priors: a knot span outside the control points (internal error)"};
      ++active;
      for (int d = 0; d < 3; ++d) if (ws[(size_t)(d * K + k)] > 0.0) ++rows;
      for (int g = c0; g <= c0 + 3; ++g) {
        if (hi[(size_t)g] == 0) lo[(size_t)g] = (int32_t)k;
        hi[(size_t)g] = (int32_t)k + 1;
      }
    }
    pv.row_lo = prior_upload(lo); pv.row_hi = prior_upload(hi);
    MVUS_HIP(hipStreamSynchronize(stream));
    prior = pv; prior_perm = perm; prior_active = active; prior_rows = rows; prior_gen = ++prior_sets;
  }
  // behind an assembly at x (HipSchur::assemble): the priors' blocks are added to the spline gradient and the band
  void prior_normal_equations(const NEView& ne, const double* x) {
    if (x == nullptr || ne.W < 4 || ne.row0 != 0 || ne.N != hp.N) throw HipError{"position priors: the assembly has no point, or is not the whole spline block (internal error)"};
    constexpr int kWaves = kThreads / 64;
    hipLaunchKernelGGL(k_prior_ne, dim3((unsigned)((ne.N + kWaves - 1) / kWaves)), dim3(kThreads), 0, stream, dp, prior, x, ne);
    MVUS_HIP(hipGetLastError());
  }
  // Surveyed landmarks (mvus_ba_set_landmarks, ba_landmark.hip.h), state of the handle like the loss, the mask and the priors, kept over
  // remove_outliers (they hang on the cameras, which outlier removal leaves alone).  lm.K counts what the caller set, lm_active the
  // observations with a weight on at least one axis: with lm_active = 0 no kernel, argument or branch on the device differs from a
  // handle that never had any.
  LandmarkView lm{};
  DeviceOwner lm_own;
  std::vector<int64_t> lm_perm;             // sorted position -> the caller's index
  int lm_active = 0;
  uint64_t lm_gen = 0, lm_sets = 0;         // lm_gen names the set in force (HipSchur::assemble_held: which landmarks held blocks carry)
  int64_t lm_rows = 0;                      // (observation, axis) pairs with w > 0: the rows the covariance's degrees of freedom count
  bool lm_lds_set = false;
  int landmark_blocks() const { return lm_active > 0 ? (int)std::min<int64_t>(2048, ((int64_t)lm.K + kThreads - 1) / kThreads) : 0; }
  void clear_landmarks() {
    if (!lm_own.empty()) MVUS_HIP(hipStreamSynchronize(stream));
    lm_own.reset(); lm_perm.clear();
    lm = LandmarkView{}; lm_active = 0; lm_rows = 0;
  }
  template <class T>
  T* lm_upload(const std::vector<T>& v) {
    T* p = lm_own.device<T>(std::max<size_t>(v.size(), 1));
    if (!v.empty()) MVUS_HIP(hipMemcpyAsync(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, stream));
    return p;
  }
  // X[3L], cam[K], point[K], uv[2K], w[2K] in the caller's order (validated): sorted by (camera, landmark, input order), the rows per
  // camera from the sorted list, the observed pixels of the fixed-calibration row by k_landmark_setup
  void set_landmarks(int64_t L, const double* X, int64_t K, const int32_t* cam, const int32_t* point, const double* uv, const double* w) {
    if (K <= 0) { clear_landmarks(); return; }
    std::vector<int64_t> perm((size_t)K);
    for (int64_t k = 0; k < K; ++k) perm[(size_t)k] = k;
    std::stable_sort(perm.begin(), perm.end(), [&](int64_t a, int64_t b) { return cam[a] != cam[b] ? cam[a] < cam[b] : point[a] < point[b]; });
    std::vector<int32_t> cs((size_t)K), ps((size_t)K), lo((size_t)hp.C, 0), hi((size_t)hp.C, 0);
    std::vector<double> uvs((size_t)2 * K), ws((size_t)2 * K);
    const std::vector<double> Xs(X, X + 3 * L);
    int active = 0;
    int64_t rows = 0;
    for (int64_t k = 0; k < K; ++k) {
      const int64_t s = perm[(size_t)k];
      cs[(size_t)k] = cam[s]; ps[(size_t)k] = point[s];
      for (int d = 0; d < 2; ++d) { uvs[(size_t)(d * K + k)] = uv[d * K + s]; ws[(size_t)(d * K + k)] = w[d * K + s]; if (w[d * K + s] > 0.0) ++rows; }
      if (w[s] > 0.0 || w[K + s] > 0.0) ++active;
      if (hi[(size_t)cam[s]] == 0) lo[(size_t)cam[s]] = (int32_t)k;
      hi[(size_t)cam[s]] = (int32_t)k + 1;
    }
    clear_landmarks();
    LandmarkView lv{};      // built aside: a failure below leaves the handle without landmarks (the buffers go at the next clear_landmarks)
    lv.K = (int)K; lv.L = (int)L;
    lv.X = lm_upload(Xs); lv.cam = lm_upload(cs); lv.point = lm_upload(ps); lv.uv = lm_upload(uvs); lv.w = lm_upload(ws);
    lv.uvo = lm_upload(uvs);
    lv.row_lo = lm_upload(lo); lv.row_hi = lm_upload(hi);
    if (!hp.calib && hp.undist) {
      hipLaunchKernelGGL(k_landmark_setup, dim3((unsigned)((K + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, dp, lv);
      MVUS_HIP(hipGetLastError());
    }
    if (!lm_lds_set) {      // (the attribute belongs to the function, not to the handle: the larger of the two sizes, whatever this handle's P)
      MVUS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_landmark_ne), hipFuncAttributeMaxDynamicSharedMemorySize, (int)landmark_lds_bytes(15)));
      lm_lds_set = true;
    }
    MVUS_HIP(hipStreamSynchronize(stream));      // (pageable sources of asynchronous copies: alive until here)
    lm = lv; lm_perm = perm; lm_active = active; lm_rows = rows; lm_gen = ++lm_sets;
  }
  // behind an assembly at x (HipSchur::assemble): the landmarks' blocks are added to the camera blocks and the camera gradient
  void landmark_normal_equations(const NEView& ne, const double* x) {
    if (x == nullptr || ne.C != hp.C || ne.B != 3 + hp.P) throw HipError{"landmarks: the assembly has no point, or is not this handle's camera block (internal error)"};
    ensure_cams(x);
    hipLaunchKernelGGL(k_landmark_ne, dim3((unsigned)hp.C), dim3(kThreads), landmark_lds_bytes(hp.P), stream, dp, lm, (const CamState*)cams, ne);
    MVUS_HIP(hipGetLastError());
  }
  // clr / clr_len: storage to zero beside the evaluation (HipSchur's normal-equation blocks); returns false if it was not done
  // with_priors: the position priors' and the landmarks' rows are part of the sum (every cost the solver and the covariance use;
  // mvus_ba_robust_cost stays raw)
  bool residual_sq(const double* x, double* f, double* out, double* clr = nullptr, int64_t clr_len = 0, bool with_priors = true) {
    // (observation shards off the root rank: the replicated motion rows are rows of zeros there -- the general path)
    if (allreduce && hp.T > 0 && !(is_root || tshard.on)) { residual(x, f); dot_m_into(f, f, out); return false; }
    RoctxRange range("mvus residual");
    const int mb = hp.T > 0 ? (int)((hp.T + kThreads - 1) / kThreads) : 0;
    const int pb = with_priors ? prior_blocks() + landmark_blocks() : 0;      // (the landmarks' partials behind the priors')
    const size_t need = (size_t)dp.n_chunks + mb + pb + 1;
    const bool host_sum = scal_direct() && out >= scal_out() && out < scal_out() + kHostSumEnd && !sw.sq_device_sum;
    const int set = (out == lm_scalars() + kLmCostX0) ? 0 : 1;
    double* sq_part = this->sq_part;
    if (host_sum) {
      if (need > sqh_cap) {
        sqh_own.reset(); sqh_cap = 0;
        for (int i = 0; i < 2; ++i) {
          sqh_host[i] = sqh_own.mapped<double>(need);
          MVUS_HIP(hipHostGetDevicePointer(reinterpret_cast<void**>(&sqh_dev[i]), sqh_host[i], 0));
        }
        sqh_cap = need;
      }
      sq_part = sqh_dev[set];
    } else if (need > sq_cap) { this->sq_part = dalloc<double>(need); sq_cap = need; sq_part = this->sq_part; }
    ensure_cams(x);
    bool cleared = false;
    if (dp.n_chunks > 0) {
      const int fb = (clr && clr_len > 0) ? (int)std::min<int64_t>(2048, (clr_len + kThreads - 1) / kThreads) : 0;
      const dim3 g(dp.n_chunks + fb), b(kThreads);
      double* c = fb > 0 ? clr : (double*)nullptr;
      with_flag(hp.calib, [&](auto calib) {
        if (robust()) hipLaunchKernelGGL((k_observations<calib(), false, true>), g, b, 0, stream, dp, cams, x, f, J, rspan, pat0, 0, sq_part, c, (long long)clr_len, loss);
        else hipLaunchKernelGGL((k_observations<calib(), false>), g, b, 0, stream, dp, cams, x, f, J, rspan, pat0, 0, sq_part, c, (long long)clr_len);
      });
      rspan_for = x;
      cleared = fb > 0;
    }
    if (mb > 0 && robust()) hipLaunchKernelGGL((k_motion<false, true>), dim3(mb), dim3(kThreads), 0, stream, dp, x, f + 2 * hp.M, mJ, mctrl, 0, sq_part + dp.n_chunks, loss);
    else if (mb > 0) hipLaunchKernelGGL(k_motion<false>, dim3(mb), dim3(kThreads), 0, stream, dp, x, f + 2 * hp.M, mJ, mctrl, 0, sq_part + dp.n_chunks);
    if (with_priors && prior_blocks() > 0) hipLaunchKernelGGL(k_prior_cost, dim3(prior_blocks()), dim3(kThreads), 0, stream, dp, prior, x, sq_part + dp.n_chunks + mb, (double*)nullptr);
    if (with_priors && landmark_blocks() > 0)
      hipLaunchKernelGGL(k_landmark_cost, dim3(landmark_blocks()), dim3(kThreads), 0, stream, dp, lm, (const CamState*)cams, sq_part + dp.n_chunks + mb + prior_blocks(), (double*)nullptr, (double*)nullptr);
    if (host_sum) { sq_pend[set].slot = out - scal_out(); sq_pend[set].n = dp.n_chunks + mb + pb; }      // added up by fetch()
    else if (dp.n_chunks + mb + pb > 0) hipLaunchKernelGGL(k_dot_final, dim3(1), dim3(kThreads), 0, stream, dp.n_chunks + mb + pb, sq_part, out);
    else MVUS_HIP(hipMemsetAsync(out, 0, sizeof(double), stream));
    reduce(out, 1);                  // (sharded: the workgroups' partial sums replace a pass of k_dot_partial over f; the ranks' sums are added here)
    MVUS_HIP(hipGetLastError());
    return cleared;
  }
  // motion rows only: their residuals and Jacobian blocks (the fused LM path evaluates the detection rows elsewhere)
  void motion_jacobian(const double* x, double* f) {
    if (hp.T <= 0) return;
    if (is_root || tshard.on) hipLaunchKernelGGL(k_motion<true>, dim3((hp.T + kThreads - 1) / kThreads), dim3(kThreads), 0, stream, dp, x, f + 2 * hp.M, mJ, mctrl, 0);
    else MVUS_HIP(hipMemsetAsync(f + 2 * hp.M, 0, sizeof(double) * hp.T, stream));
    MVUS_HIP(hipGetLastError());
  }
  void jacobian(const double* x, double* f, int jac_mode) {
    if (jac_mode == MVUS_JAC_FD) jacobian_fd(x, f); else eval(x, f, true, jac_mode);
    if (freeze_stored_jacobian) freeze_jacobian();      // (a solve with a mask in force: analytic, pattern and FD alike)
  }

  void set_fd_groups(const int32_t* groups, int ngroups) {
    if (!fd_groups) { fd_groups = dalloc<int32_t>(hp.n); fd_h = dalloc<double>(hp.n); fd_dx = dalloc<double>(hp.n); fd_xg = dalloc<double>(hp.n); }
    MVUS_HIP(hipMemcpyAsync(fd_groups, groups, sizeof(int32_t) * hp.n, hipMemcpyHostToDevice, stream));
    MVUS_HIP(hipStreamSynchronize(stream));
    if (ngroups > fd_ngroups || !fd_F) { fd_F = dalloc<double>((size_t)ngroups * hp.m); }
    fd_ngroups = ngroups;
  }
  // scipy's approx_derivative(..., method='2-point', sparsity=(pattern, groups)): one residual per column group
  void jacobian_fd(const double* x, double* f) {
    if (!has_pattern || fd_ngroups <= 0) throw HipError{"MVUS_JAC_FD needs mvus_ba_set_pattern and mvus_ba_set_fd_groups first"};
    const int n = (int)hp.n;
    ensure_J();
    eval(x, f, false, 0);
    hipLaunchKernelGGL(k_fd_steps, dim3((n + 255) / 256), dim3(256), 0, stream, n, hp.C, hp.rs_bounds, x, fd_h, fd_dx);
    for (int g = 0; g < fd_ngroups; ++g) {
      touch(fd_xg);
      hipLaunchKernelGGL(k_fd_perturb, dim3((n + 255) / 256), dim3(256), 0, stream, n, g, x, fd_h, fd_groups, fd_xg);
      eval(fd_xg, fd_F + (size_t)g * hp.m, false, 0);
    }
    if (dp.n_chunks > 0)
      with_flag(hp.calib, [&](auto calib) { hipLaunchKernelGGL(k_fd_fill<calib() ? 30 : 21>, dim3(dp.n_chunks), dim3(kThreads), 0, stream, dp, (long long)hp.m, f, fd_F, fd_dx, fd_groups, pat0, J, span); });
    if (hp.T > 0) {
      if (is_root) hipLaunchKernelGGL(k_fd_fill_motion, dim3((hp.T + kThreads - 1) / kThreads), dim3(kThreads), 0, stream, dp, (long long)hp.m, f, fd_F, fd_dx, fd_groups, mJ, mctrl);
    }
    MVUS_HIP(hipGetLastError());
    has_jacobian = true; jac_x = x;
  }

  // Scene.remove_outliers on the resident data: mask at x, stable compaction, new launch tables.
  void remove_outliers(const double* x_dev, double thres, uint8_t* keep_out, int64_t* det_off_out) {
    residual(x_dev, f_cur);
    const int nc = dp.n_chunks;
    DeviceOwner tmp;                          // freed on every exit
    uint8_t* keep = tmp.device<uint8_t>((size_t)hp.M);
    int32_t* counts = tmp.device<int32_t>((size_t)nc);
    std::vector<int32_t> cnt_h(nc);
    std::vector<long long> off_h(nc);
    long long* off_d = tmp.device<long long>((size_t)nc);
    if (nc > 0) {
      hipLaunchKernelGGL(k_outlier_mask, dim3(nc), dim3(kThreads), 0, stream, dp, f_cur, thres, keep);
      hipLaunchKernelGGL(k_compact_count, dim3(nc), dim3(kThreads), 0, stream, dp, keep, counts);
      MVUS_HIP(hipMemcpyAsync(cnt_h.data(), counts, sizeof(int32_t) * nc, hipMemcpyDeviceToHost, stream));
    }
    if (keep_out && hp.M > 0) MVUS_HIP(hipMemcpyAsync(keep_out, keep, hp.M, hipMemcpyDeviceToHost, stream));
    MVUS_HIP(hipStreamSynchronize(stream));
    std::vector<int64_t> new_off(hp.C + 1, 0);
    long long run = 0;
    for (int k = 0; k < nc; ++k) { off_h[k] = run; run += cnt_h[k]; new_off[hp.chunk_cam[k] + 1] += cnt_h[k]; }
    for (int c = 0; c < hp.C; ++c) new_off[c + 1] += new_off[c];
    const int64_t newM = run;
    // the compacted copy goes into a second set of detection arrays (allocated once, sized for the original problem);
    // the two sets swap roles on every call
    if (!det_alt[0]) for (double*& p : det_alt) p = dalloc<double>(det_capacity);
    double *nf = det_alt[0], *nu = det_alt[1], *nv = det_alt[2], *nuo = det_alt[3], *nvo = det_alt[4];
    det_alt[0] = const_cast<double*>(dp.frame); det_alt[1] = const_cast<double*>(dp.u_raw); det_alt[2] = const_cast<double*>(dp.v_raw);
    det_alt[3] = const_cast<double*>(dp.u_obs); det_alt[4] = const_cast<double*>(dp.v_obs);
    if (nc > 0) {
      MVUS_HIP(hipMemcpyAsync(off_d, off_h.data(), sizeof(long long) * nc, hipMemcpyHostToDevice, stream));
      hipLaunchKernelGGL(k_compact_scatter, dim3(nc), dim3(kThreads), 0, stream, dp, keep, off_d, nf, nu, nv, nuo, nvo);
      MVUS_HIP(hipGetLastError());
    }
    MVUS_HIP(hipStreamSynchronize(stream));
    // the handle now describes the filtered problem
    hp.det_off = new_off; hp.M = newM; hp.m = 2 * newM + hp.T;
    hp.frame.clear(); hp.u_raw.clear(); hp.v_raw.clear();          // host copies are no longer current
    hp.build_chunks();
    dp.frame = nf; dp.u_raw = nu; dp.v_raw = nv; dp.u_obs = nuo; dp.v_obs = nvo;
    dp.M = newM;
    // the launch tables shrink (never more chunks per camera than before): rewritten in place
    std::vector<long long> cs(hp.chunk_start.begin(), hp.chunk_start.end()), doff(hp.det_off.begin(), hp.det_off.end());
    const size_t nck = hp.chunk_cam.size();
    if (nck > 0) {
      MVUS_HIP(hipMemcpyAsync(const_cast<int32_t*>(dp.chunk_cam), hp.chunk_cam.data(), nck * sizeof(int32_t), hipMemcpyHostToDevice, stream));
      MVUS_HIP(hipMemcpyAsync(const_cast<int32_t*>(dp.chunk_count), hp.chunk_count.data(), nck * sizeof(int32_t), hipMemcpyHostToDevice, stream));
      MVUS_HIP(hipMemcpyAsync(const_cast<long long*>(dp.chunk_start), cs.data(), nck * sizeof(long long), hipMemcpyHostToDevice, stream));
      MVUS_HIP(hipMemcpyAsync(const_cast<ChunkInfo*>(dp.chunks), hp.chunks.data(), nck * sizeof(ChunkInfo), hipMemcpyHostToDevice, stream));
    }
    MVUS_HIP(hipMemcpyAsync(const_cast<long long*>(dp.det_off), doff.data(), doff.size() * sizeof(long long), hipMemcpyHostToDevice, stream));
    MVUS_HIP(hipMemcpyAsync(const_cast<int32_t*>(dp.cam_chunk_off), hp.cam_chunk_off.data(), hp.cam_chunk_off.size() * sizeof(int32_t), hipMemcpyHostToDevice, stream));
    dp.n_chunks = (int)nck;
    MVUS_HIP(hipStreamSynchronize(stream));
    has_pattern = false; has_jacobian = false; fd_ngroups = 0; rspan_for = nullptr;
    if (pattern_uploaded && hp.T > 0) MVUS_HIP(hipMemcpyAsync(ms_pat_dev, hp.ms_pat.data(), sizeof(int32_t) * hp.T, hipMemcpyHostToDevice, stream));
    pattern_uploaded = false;
    m_glob = hp.m;
    if (det_off_out) std::memcpy(det_off_out, new_off.data(), sizeof(int64_t) * (hp.C + 1));
  }

  void set_pattern(const double* x0_dev) {
    ensure_cams(x0_dev);
    if (dp.n_chunks > 0) hipLaunchKernelGGL(k_pattern, dim3(dp.n_chunks), dim3(kThreads), 0, stream, dp, cams, pat0);
    MVUS_HIP(hipGetLastError());
    if (pattern_uploaded && hp.T > 0)      // back to the canonical motion-row codes
      MVUS_HIP(hipMemcpyAsync(ms_pat_dev, hp.ms_pat.data(), sizeof(int32_t) * hp.T, hipMemcpyHostToDevice, stream));
    has_pattern = true; pattern_uploaded = false;
  }
  // every point of a code must be a control point of ONE spline
  bool code_ok(int32_t code) const {
    if (code < 0) return code == -1;
    const int p = pattern_index(code), mk = pattern_mask(code);
    if (mk == 0 || p >= hp.N) return false;
    int top = 3; while (!((mk >> top) & 1)) --top;
    return p + top < hp.N && hp.ctrl_x0[p + top] == hp.ctrl_x0[p] + top;
  }
  std::string upload_pattern(const int32_t* pat, const int32_t* mpat) {
    for (int64_t i = 0; i < hp.M; ++i) if (!code_ok(pat[i])) return "upload_pattern: bad code in detection row " + std::to_string(i);
    if (hp.T > 0 && mpat) for (int j = 0; j < hp.T; ++j) if (mpat[j] < 0 || !code_ok(mpat[j])) return "upload_pattern: bad code in motion row " + std::to_string(j);
    if (hp.M > 0) MVUS_HIP(hipMemcpyAsync(pat0, pat, sizeof(int32_t) * hp.M, hipMemcpyHostToDevice, stream));
    if (hp.T > 0 && mpat) MVUS_HIP(hipMemcpyAsync(ms_pat_dev, mpat, sizeof(int32_t) * hp.T, hipMemcpyHostToDevice, stream));
    MVUS_HIP(hipStreamSynchronize(stream));
    has_pattern = true; pattern_uploaded = true; has_jacobian = false;
    return "";
  }

  void jv(const double* v, double* y) {
    const bool fused = dp.n_chunks > 0 && hp.T > 0;        // the motion rows in extra workgroups of k_jv
    if (dp.n_chunks > 0) {
      const unsigned grid = (unsigned)(xcd_grid(dp.n_chunks) + (fused ? (hp.T + kThreads - 1) / kThreads : 0));
      const double* mj = fused ? mJ : nullptr;
      with_flag(hp.calib, [&](auto calib) { hipLaunchKernelGGL(k_jv<calib() ? 30 : 21>, dim3(grid), dim3(kThreads), 0, stream, dp, J, span, v, y, mj, mctrl, y + 2 * hp.M); });
    }
    if (hp.T > 0 && !fused) hipLaunchKernelGGL(k_motion_jv, dim3((hp.T + kThreads - 1) / kThreads), dim3(kThreads), 0, stream, dp, mJ, mctrl, v, y + 2 * hp.M);
    MVUS_HIP(hipGetLastError());
  }
  // z = J^T u of this rank's rows: deterministic two-pass form (k_jtu_partial / k_jtu_reduce)
  double *zc = nullptr, *zs = nullptr;
  int32_t *zg0 = nullptr, *zfill = nullptr, *zext = nullptr;
  int* jt_bounds = nullptr;               // [2] measured by k_jtu_index: how far a chunk starts below the running maximum, how far a chunk reaches
  int* jt_nondet = nullptr;
  // z_is_zero: the caller guarantees z == 0 on entry (the device-resident LSMR loop clears it while consuming it);
  // reuse_index: zfill of the previous call is still valid (same Jacobian, hence the same window starts)
  int32_t* jt_first = nullptr;            // [N][C] first covering chunk per (control point, camera): valid while reuse_index calls follow one another
  void jtu_buffers() {
    if (!zc) {
      const size_t nc = std::max<size_t>(hp.chunks.size(), 1);
      zc = dalloc<double>(nc * (size_t)(hp.NS - 12)); zs = dalloc<double>(nc * 3 * (size_t)kJtWin); zg0 = dalloc<int32_t>(nc); zfill = dalloc<int32_t>(nc);
      zext = dalloc<int32_t>(nc); jt_bounds = dalloc<int>(2);
      jt_nondet = dalloc<int>(1);
      MVUS_HIP(hipMemsetAsync(jt_nondet, 0, sizeof(int), stream));
    }
  }
  void jtu_local(const double* u, double* z, bool z_is_zero = false, bool reuse_index = false, bool build_first = false) {
    jtu_buffers();
    if (!z_is_zero) MVUS_HIP(hipMemsetAsync(z, 0, sizeof(double) * hp.n, stream));
    if (!reuse_index) MVUS_HIP(hipMemsetAsync(jt_bounds, 0, 2 * sizeof(int), stream));
    const dim3 g2(hp.C + (hp.N + kThreads / 64 - 1) / (kThreads / 64)), b(kThreads);
    const int motion = hp.T > 0 ? 1 : 0;
    with_flag(hp.calib, [&](auto calib) {
      constexpr int NS = calib() ? 30 : 21;
      if (dp.n_chunks > 0) hipLaunchKernelGGL(k_jtu_partial<NS>, dim3(xcd_grid(dp.n_chunks)), b, 0, stream, dp, J, span, u, z, zc, zs, zg0, jt_nondet, zext);
      if (!reuse_index) hipLaunchKernelGGL(k_jtu_index, dim3(hp.C), dim3(64), 0, stream, dp, zg0, zfill, zext, jt_bounds);
      if (build_first) build_jt_first();
      hipLaunchKernelGGL(k_jtu_reduce<NS>, g2, b, 0, stream, dp, zc, zs, zg0, zfill, mJ, mctrl, u + 2 * hp.M, motion, z, (reuse_index || build_first) ? jt_first : (int32_t*)nullptr, jt_bounds);
    });
    MVUS_HIP(hipGetLastError());
  }
  void build_jt_first() {
    if (!jt_first) jt_first = dalloc<int32_t>((size_t)std::max<int64_t>(hp.N, 1) * hp.C);
    const long long e = (long long)hp.N * hp.C;
    if (e > 0) hipLaunchKernelGGL(k_jtu_first, dim3((unsigned)((e + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, dp, zfill, jt_first, jt_bounds);
  }
  void jtu(const double* u, double* z) { jtu_local(u, z); reduce(z, (size_t)hp.n); }

  // ---- device-resident LSMR iterations (Lsmr::run of ba_solver.h, unbounded case, one rank) ----
  static constexpr bool kDeviceLsmr = true;
  LsmrScalars* lsmr_state = nullptr;       // [2] device
  LsmrScalars* lsmr_host = nullptr;        // pinned
  double* lsmr_part = nullptr;             // [3][2048] partial sums (u.u, v.v, x.x) + beta
  double* lsmr_pu = nullptr;               // per-workgroup partials of |u'|^2 of the one-pass form (k_jvjtu)
  size_t lsmr_pu_cap = 0;
  bool lsmr_on_device() const { return !allreduce && !sw.lsmr_host; }
  bool lsmr_scaled_on_device() const { return !sw.lsmr_bounded_host; }      // (A/B: the bounded problem on the host-driven loop, rounds 3-5)
  // D, E: the column scaling and the extra diagonal rows of the bounded problem (trf_bounds), device n-vectors or null; ub: the n extra rows of u
  void lsmr_iterations(LsmrScalars& sc, double* ut, double* tm, double* v, double* tn, double* h, double* hbar, double* x,
                       const double* D = nullptr, const double* E = nullptr, double* ub = nullptr) {
    if (!lsmr_state) {
      lsmr_state = dalloc<LsmrScalars>(2);
      lsmr_part = dalloc<double>(4 * 2048 + 8);      // u.u, v.v, x.x, (ub.ub) partials + beta
      lsmr_host = own.pinned<LsmrScalars>(1);
    }
    const long long n = hp.n, m = hp.m;
    const int gm = grid_for(m), gn = grid_for(n);
    double *pu = lsmr_part, *pv = lsmr_part + 2048, *px = lsmr_part + 4096, *pub = lsmr_part + 6144, *beta_dev = lsmr_part + 8192;
    const bool scaled = D != nullptr || E != nullptr;
    double* dv = nullptr;                                   // D v (the scaled problem's argument of J)
    if (D) dv = alloc(n);
    *lsmr_host = sc;
    MVUS_HIP(hipMemcpyAsync(lsmr_state, lsmr_host, sizeof(LsmrScalars), hipMemcpyHostToDevice, stream));
    int cur = 0;
    const int batch = 8;
    long long launched = 0;
    MVUS_HIP(hipMemsetAsync(tn, 0, sizeof(double) * n, stream));        // J^T u adds into a zeroed vector; k_lsmr_v clears it again while reading it
    // MVUS_LSMR_ONE_PASS=1: one pass over J per iteration (k_jvjtu: u kept unnormalised, its norm in *ubeta).  Opt-in: the converged
    // answers stay inside the parity bars either way, but the unconverged 10-evaluation iterate of one fixture (dist_fixed_2cam) moves
    // outside the bars measured with the two-pass arithmetic
    const bool one_pass = dp.n_chunks > 0 && !scaled && lsmr_one_pass_now();
    const unsigned gj = (unsigned)(xcd_grid(dp.n_chunks) + (hp.T > 0 ? (hp.T + kThreads - 1) / kThreads : 0));
    double* ubeta = beta_dev + 1;
    if (one_pass) {
      if (lsmr_pu_cap < (size_t)gj) { lsmr_pu = dalloc<double>(gj); lsmr_pu_cap = gj; }
      jtu_buffers();
      const double one = 1.0;
      MVUS_HIP(hipMemcpyAsync(ubeta, &one, sizeof(double), hipMemcpyHostToDevice, stream));       // (ut arrives normalised)
      MVUS_HIP(hipMemsetAsync(jt_bounds, 0, 2 * sizeof(int), stream));
    }
    while (true) {
      for (int b = 0; b < batch && launched < sc.maxiter; ++b, ++launched) {
        const LsmrScalars* c = lsmr_state + cur;
        LsmrScalars* nx = lsmr_state + (cur ^ 1);
        if (one_pass) {
          const dim3 g2(hp.C + (hp.N + kThreads / 64 - 1) / (kThreads / 64)), bt(kThreads);
          const int motion = hp.T > 0 ? 1 : 0;
          with_flag(hp.calib, [&](auto calib) {
            constexpr int NS = calib() ? 30 : 21;
            hipLaunchKernelGGL(k_jvjtu<NS>, dim3(gj), bt, 0, stream, dp, J, span, v, ut, c, ubeta, lsmr_pu, tn, zc, zs, zg0, jt_nondet, zext, mJ, mctrl);
            if (launched == 0) { hipLaunchKernelGGL(k_jtu_index, dim3(hp.C), dim3(64), 0, stream, dp, zg0, zfill, zext, jt_bounds); build_jt_first(); }
            hipLaunchKernelGGL(k_jtu_reduce<NS>, g2, bt, 0, stream, dp, zc, zs, zg0, zfill, mJ, mctrl, ut + 2 * hp.M, motion, tn, jt_first, jt_bounds);
          });
          hipLaunchKernelGGL(k_lsmr_v1, dim3(gn), dim3(kThreads), 0, stream, n, tn, v, c, (int)gj, lsmr_pu, beta_dev, ubeta, pv);
        } else if (scaled) {
        // the bounded problem: A = [J diag(D); diag(E)] -- the host-driven loop's operations (Lsmr::run), launch for launch without its
        // three synchronisations per iteration
        if (D) { hipLaunchKernelGGL(k_lsmr_scale, dim3(gn), dim3(kThreads), 0, stream, n, D, (const double*)v, dv, c); jv(dv, tm); }
        else jv(v, tm);
        hipLaunchKernelGGL(k_lsmr_u, dim3(gm), dim3(kThreads), 0, stream, m, tm, ut, c, pu);
        if (E) {
          hipLaunchKernelGGL(k_lsmr_ub, dim3(gn), dim3(kThreads), 0, stream, n, E, (const double*)v, ub, c, pub);
          hipLaunchKernelGGL(k_lsmr_unorm2, dim3(gm), dim3(kThreads), 0, stream, m, ut, gm, pu, n, ub, gn, pub, c, beta_dev);
        } else hipLaunchKernelGGL(k_lsmr_unorm, dim3(gm), dim3(kThreads), 0, stream, m, ut, gm, pu, c, beta_dev);
        jtu_local(ut, tn, true, launched > 0, launched == 0);
        hipLaunchKernelGGL(k_lsmr_v_de, dim3(gn), dim3(kThreads), 0, stream, n, tn, v, D, E, (const double*)ub, c, beta_dev, pv);
        } else {
        jv(v, tm);
        hipLaunchKernelGGL(k_lsmr_u, dim3(gm), dim3(kThreads), 0, stream, m, tm, ut, c, pu);
        hipLaunchKernelGGL(k_lsmr_unorm, dim3(gm), dim3(kThreads), 0, stream, m, ut, gm, pu, c, beta_dev);
        jtu_local(ut, tn, true, launched > 0, launched == 0);
        hipLaunchKernelGGL(k_lsmr_v, dim3(gn), dim3(kThreads), 0, stream, n, tn, v, c, beta_dev, pv);
        }
        hipLaunchKernelGGL(k_lsmr_update, dim3(gn), dim3(kThreads), 0, stream, n, v, h, hbar, x, gn, pv, c, beta_dev, nx, px);
        hipLaunchKernelGGL(k_lsmr_test, dim3(1), dim3(kThreads), 0, stream, gn, px, c, nx);
        cur ^= 1;
      }
      MVUS_HIP(hipGetLastError());
      MVUS_HIP(hipMemcpyAsync(lsmr_host, lsmr_state + cur, sizeof(LsmrScalars), hipMemcpyDeviceToHost, stream));
      MVUS_HIP(hipStreamSynchronize(stream));
      if (lsmr_host->istop != 0 || launched >= sc.maxiter) break;
    }
    sc = *lsmr_host;
    if (dv) release(dv);
    touch(v); touch(x); touch(h); touch(hbar);
  }
};

}  // namespace mvus
