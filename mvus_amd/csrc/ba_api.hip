// libmvusba.so, bundle adjustment: the mvus_ba_* part of the C ABI of include/mvus_ba.h over the HIP backend of the templated optimiser
// (HipBackend: ba_backend.hip.h), and the RCCL loader
// (the spline stage is spline_api.hip, two-view geometry and PnP twoview_api.hip; api_common.h is what the three share).
// There is no CPU compute path in this library: every entry point that evaluates anything
// launches HIP kernels, and mvus_ba_create fails with MVUS_E_HIP when no device is usable.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <dlfcn.h>
#include <mutex>
#include <memory>
#include <string>
#include <vector>

#include "ba_backend.hip.h"
#include "ba_schur_hip.hip.h"
#include "ba_schur_host.hip.h"
#include "ba_cov.hip.h"
#include "ba_register.hip.h"

namespace mvus {

thread_local std::string g_create_error;      // declared in api_common.h: the one error string behind mvus_last_error(NULL)

}  // namespace mvus

using namespace mvus;

struct mvus_rccl_comm;
struct mvus_rccl_id { char internal[128]; };     // ncclUniqueId of rccl.h (passed by value to ncclCommInitRank)
struct mvus_rccl_handle { void* comm = nullptr; };
struct mvus_ba {
  HipBackend be;
  std::unique_ptr<HipSchur<HipBackend>> schur;   // normal-equation workspace, built on first use
  std::unique_ptr<CovChain<HipBackend>> cov;     // buffers of mvus_ba_covariance / mvus_ba_detection_covariance (ba_cov.hip.h), built on first use
  std::unique_ptr<RegisterWork> reg;             // buffers of mvus_ba_register_cameras / _linearize (ba_register.hip.h), built on first use
  mvus_rccl_handle rccl;                         // communicator of mvus_ba_set_rccl (destroyed with the handle)
  void drop_schur() { schur.reset(); be.mem.forget_blocks(); }      // the workspace goes (it is sized by the launch tables / the time slice), and with it the blocks it held
  ~mvus_ba();
};

// a mask on a sharded handle (set in either order) refuses: it is never solved unmasked
static bool frozen_on_shards(HipBackend& be, const char* who) {
  if (be.frozen_count <= 0 || !(be.allreduce || be.tshard.on)) return false;
  be.err = std::string(who) + ": frozen parameters (mvus_ba_set_frozen) are not supported on a sharded handle (set_allreduce / set_rccl / set_time_shard)";
  return true;
}

// the same for position priors
static bool priors_on_shards(HipBackend& be, const char* who) {
  if (be.prior.K <= 0 || !(be.allreduce || be.tshard.on)) return false;
  be.err = std::string(who) + ": position priors (mvus_ba_set_position_priors) are not supported on a sharded handle (set_allreduce / set_rccl / set_time_shard)";
  return true;
}

// and for landmarks
static bool landmarks_on_shards(HipBackend& be, const char* who) {
  if (be.lm.K <= 0 || !(be.allreduce || be.tshard.on)) return false;
  be.err = std::string(who) + ": landmarks (mvus_ba_set_landmarks) are not supported on a sharded handle (set_allreduce / set_rccl / set_time_shard)";
  return true;
}

// the two timing entry points: `warmup` runs of fn, then the stream time of `reps` runs between two events, in ms per run
template <class F>
static double time_on_stream(hipStream_t st, int warmup, int reps, F&& fn) {
  DeviceOwner ev;
  const hipEvent_t e0 = ev.event(), e1 = ev.event();
  for (int i = 0; i < warmup; ++i) fn();
  MVUS_HIP(hipEventRecord(e0, st));
  for (int i = 0; i < reps; ++i) fn();
  MVUS_HIP(hipEventRecord(e1, st));
  MVUS_HIP(hipEventSynchronize(e1));
  float ms = 0;
  MVUS_HIP(hipEventElapsedTime(&ms, e0, e1));
  return (double)ms / reps;
}

// Who keeps what of the handle's memory (ba_held.h).  An LM solve leaves f(x), its cost and maybe the normal equations
// for the point it returned (the carry); normal_equations and lm_step leave the blocks they assembled.  Both are valid for the very next
// call only, unless that call's row keeps them.  The row is applied on entry, so a refused or empty call keeps what a served one keeps.
// A new entry point picks its row here: kTransparent if it touches nothing the handle holds; kKeepsBlocks if the held Jacobian and the blocks
// in the Schur workspace are written by HipSchur::assemble_held or not at all; else kKeepsNothing.            {carry, blocks}
constexpr CallKeeps kTransparent{true, KeepBlocks::all};             // register_cameras, register_linearize
constexpr CallKeeps kKeepsBlocks{false, KeepBlocks::all};            // normal_equations, lm_step, deterministic_fallback, position_prior_cost, lsmr, set_position_priors,
                                                                     // set_landmarks, landmark_cost, landmark_rows
constexpr CallKeeps kKeepsRawBlocks{false, KeepBlocks::unfrozen};    // set_frozen: blocks with a freeze pass on them belong to the old mask
constexpr CallKeeps kKeepsNothing{false, KeepBlocks::none};          // every other entry point: solve, covariance, detection_covariance, set_loss, ...

template <class F>
static int guarded(mvus_ba* h, CallKeeps keeps, F&& fn) {
  if (!h) return MVUS_E_INVALID;
  try {
    (void)hipSetDevice(h->be.device);
    h->be.mem.begin_call(keeps);
    return fn();
  } catch (const HipError& e) {
    h->be.err = e.msg;
    return e.code;
  } catch (const std::exception& e) {
    h->be.err = e.what();
    return MVUS_E_INVALID;
  }
}

extern "C" {

void mvus_default_opts(mvus_solve_opts* o) {
  if (!o) return;
  o->solver = MVUS_SOLVER_TRF_LSMR; o->jac_mode = MVUS_JAC_PATTERN; o->max_nfev = 10;
  o->ftol = 1e-8; o->xtol = 1e-12; o->gtol = 1e-8;
  o->lsmr_atol = 1e-6; o->lsmr_btol = 1e-6; o->lsmr_conlim = 1e8; o->lsmr_maxiter = 0; o->verbose = 0; o->lm_lambda_min = 3e-3; o->lm_trust_radius = -1.0;
}

int32_t mvus_abi_sizes(int32_t* solve_opts_size, int32_t* result_size, int32_t* problem_size) {
  if (solve_opts_size) *solve_opts_size = (int32_t)sizeof(mvus_solve_opts);
  if (result_size) *result_size = (int32_t)sizeof(mvus_result);
  if (problem_size) *problem_size = (int32_t)sizeof(mvus_problem);
  return MVUS_ABI_VERSION;
}

int mvus_ba_create(const mvus_problem* p, mvus_ba** out) {
  if (!out) return MVUS_E_INVALID;
  *out = nullptr;
  mvus_ba* h = nullptr;
  try {
    h = new mvus_ba();
    std::string msg = h->be.hp.build(p);
    if (!msg.empty()) { g_create_error = msg; delete h; return MVUS_E_INVALID; }
  } catch (const std::exception& e) {          // bad_alloc / length_error on absurd sizes: nothing throws across the ABI
    g_create_error = e.what();
    delete h;
    return MVUS_E_INVALID;
  }
  try {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= p->device)
      throw HipError{"no usable HIP device (libmvusba has no CPU fallback)"};
    h->be.init(p);
  } catch (const HipError& e) {
    g_create_error = e.msg;
    delete h;
    return MVUS_E_HIP;
  } catch (const std::exception& e) {
    g_create_error = e.what();
    delete h;
    return MVUS_E_INVALID;
  }
  *out = h;
  return MVUS_OK;
}

void mvus_ba_destroy(mvus_ba* h) { delete h; }

const char* mvus_last_error(const mvus_ba* h) { return h ? h->be.err.c_str() : g_create_error.c_str(); }

int64_t mvus_ba_num_params(const mvus_ba* h) { return h ? h->be.hp.n : -1; }
int64_t mvus_ba_num_residuals(const mvus_ba* h) { return h ? h->be.hp.m : -1; }
int64_t mvus_ba_num_motion_rows(const mvus_ba* h) { return h ? h->be.hp.T : -1; }
int32_t mvus_ba_num_slots(const mvus_ba* h) { return h ? h->be.hp.NS : -1; }

int mvus_ba_set_x(mvus_ba* h, const double* x) {
  return guarded(h, kKeepsNothing, [&] { h->be.upload(h->be.x_cur, x, h->be.hp.n); return MVUS_OK; });
}

int mvus_ba_residual(mvus_ba* h, const double* x, double* f) {
  return guarded(h, kKeepsNothing, [&] {
    HipBackend& be = h->be;
    be.upload(be.x_cur, x, be.hp.n);
    be.residual(be.x_cur, be.f_cur);
    if (f) be.download(f, be.f_cur, be.hp.m);
    return MVUS_OK;
  });
}

int mvus_ba_residual_jacobian(mvus_ba* h, const double* x, int32_t jac_mode, double* f, double* J, int32_t* ctrl) {
  return guarded(h, kKeepsNothing, [&] {
    HipBackend& be = h->be;
    be.upload(be.x_cur, x, be.hp.n);
    // rows that stay invisible are never written by the kernel: clear so the host copy is well defined
    if (J) { be.ensure_J(); MVUS_HIP(hipMemsetAsync(be.J, 0, sizeof(double) * j_doubles(be.hp.NS, be.dp.n_chunks), be.stream)); }
    be.jacobian(be.x_cur, be.f_cur, jac_mode);
    be.held_analytic_at_xcur = jac_mode == MVUS_JAC_ANALYTIC;
    if (f) be.download(f, be.f_cur, be.hp.m);
    if (J) {                                 // the ABI's layout is slot-major (mvus_ba.h); the device keeps J chunk-major
      PoolGuard<HipBackend> pool(be);
      double* Jout = pool.get((int64_t)2 * be.hp.NS * std::max<int64_t>(be.hp.M, 1));
      MVUS_HIP(hipMemsetAsync(Jout, 0, sizeof(double) * 2 * be.hp.NS * be.hp.M, be.stream));
      if (be.dp.n_chunks > 0)
        with_flag(be.hp.calib, [&](auto calib) { hipLaunchKernelGGL(k_j_export<calib() ? 30 : 21>, dim3(be.dp.n_chunks), dim3(kThreads), 0, be.stream, be.dp, be.J, Jout); });
      be.download(J, Jout, (int64_t)2 * be.hp.NS * be.hp.M);
    }
    if (ctrl) {
      MVUS_HIP(hipMemcpyAsync(ctrl, be.span, sizeof(int32_t) * be.hp.M, hipMemcpyDeviceToHost, be.stream));
      MVUS_HIP(hipStreamSynchronize(be.stream));
    }
    return MVUS_OK;
  });
}

int mvus_ba_motion_rows(mvus_ba* h, const double* x, int32_t jac_mode, double* mf, double* mJ, int32_t* mctrl) {
  return guarded(h, kKeepsNothing, [&] {
    HipBackend& be = h->be;
    be.upload(be.x_cur, x, be.hp.n);
    be.jacobian(be.x_cur, be.f_cur, jac_mode);
    const int T = be.hp.T;
    if (mf && T) be.download(mf, be.f_cur + 2 * be.hp.M, T);
    if (mJ && T) be.download(mJ, be.mJ, (int64_t)36 * T);
    if (mctrl && T) {
      MVUS_HIP(hipMemcpyAsync(mctrl, be.mctrl, sizeof(int32_t) * 3 * T, hipMemcpyDeviceToHost, be.stream));
      MVUS_HIP(hipStreamSynchronize(be.stream));
    }
    return MVUS_OK;
  });
}

int mvus_ba_set_pattern(mvus_ba* h, const double* x0, int32_t* pat_out) {
  return guarded(h, kKeepsNothing, [&] {
    HipBackend& be = h->be;
    be.upload(be.x_cur, x0, be.hp.n);
    be.set_pattern(be.x_cur);
    if (pat_out) {
      MVUS_HIP(hipMemcpyAsync(pat_out, be.pat0, sizeof(int32_t) * be.hp.M, hipMemcpyDeviceToHost, be.stream));
      MVUS_HIP(hipStreamSynchronize(be.stream));
    }
    return MVUS_OK;
  });
}

int mvus_ba_upload_pattern(mvus_ba* h, const int32_t* pat, const int32_t* motion_pat) {
  return guarded(h, kKeepsNothing, [&] {
    HipBackend& be = h->be;
    if ((!pat && be.hp.M > 0)) { be.err = "upload_pattern: NULL pattern"; return MVUS_E_INVALID; }
    const std::string msg = be.upload_pattern(pat, motion_pat);
    if (!msg.empty()) { be.err = msg; return MVUS_E_INVALID; }
    return MVUS_OK;
  });
}

int mvus_ba_motion_pattern(mvus_ba* h, int32_t* motion_pat_out) {
  return guarded(h, kKeepsNothing, [&] {
    HipBackend& be = h->be;
    if (be.hp.T > 0) {
      if (!motion_pat_out) { be.err = "motion_pattern: NULL output"; return MVUS_E_INVALID; }
      MVUS_HIP(hipMemcpyAsync(motion_pat_out, be.ms_pat_dev, sizeof(int32_t) * be.hp.T, hipMemcpyDeviceToHost, be.stream));
      MVUS_HIP(hipStreamSynchronize(be.stream));
    }
    return MVUS_OK;
  });
}

int mvus_ba_set_deterministic(mvus_ba* h, int32_t on) {
  return guarded(h, kKeepsNothing, [&] { h->be.det_assembly = on != 0; return MVUS_OK; });
}
int mvus_ba_deterministic_fallback(mvus_ba* h, int32_t* fell_back) {
  return guarded(h, kKeepsBlocks, [&] {
    if (!fell_back) { h->be.err = "bad arguments"; return MVUS_E_INVALID; }
    *fell_back = (h->schur && h->schur->last_atomic) ? 1 : 0;
    return MVUS_OK;
  });
}

int mvus_ba_set_fd_groups(mvus_ba* h, const int32_t* groups, int32_t num_groups) {
  return guarded(h, kKeepsNothing, [&] {
    if (!groups || num_groups < 1) { h->be.err = "bad arguments"; return MVUS_E_INVALID; }
    for (int64_t j = 0; j < h->be.hp.n; ++j) if (groups[j] < 0 || groups[j] >= num_groups) { h->be.err = "group index out of range"; return MVUS_E_INVALID; }
    h->be.set_fd_groups(groups, num_groups);
    return MVUS_OK;
  });
}

}  // extern "C" (the two helpers below are C++)

// scipy/optimize/_group_columns.pyx: group_sparse over the CSC arrays of the permuted pattern; groups[order] = result
static int32_t group_sparse_permuted(int64_t m, int64_t n, const std::vector<int64_t>& indptr, const std::vector<int64_t>& indices, const int64_t* order, int32_t* groups) {
  std::vector<int32_t> gp((size_t)n, -1);
  std::vector<unsigned char> in_union((size_t)m);
  int32_t current = 0;
  for (int64_t i = 0; i < n; ++i) {
    if (gp[(size_t)i] >= 0) continue;
    gp[(size_t)i] = current;
    bool all_grouped = true;
    std::fill(in_union.begin(), in_union.end(), (unsigned char)0);
    for (int64_t k = indptr[(size_t)i]; k < indptr[(size_t)i + 1]; ++k) in_union[(size_t)indices[(size_t)k]] = 1;
    for (int64_t j = 0; j < n; ++j) {
      if (gp[(size_t)j] >= 0) continue;
      all_grouped = false;
      bool intersect = false;
      for (int64_t k = indptr[(size_t)j]; k < indptr[(size_t)j + 1]; ++k) if (in_union[(size_t)indices[(size_t)k]]) { intersect = true; break; }
      if (!intersect) {
        for (int64_t k = indptr[(size_t)j]; k < indptr[(size_t)j + 1]; ++k) in_union[(size_t)indices[(size_t)k]] = 1;
        gp[(size_t)j] = current;
      }
    }
    if (all_grouped) break;
    ++current;
  }
  int32_t ng = 0;
  for (int64_t j = 0; j < n; ++j) { groups[(size_t)order[j]] = gp[(size_t)j]; ng = std::max(ng, gp[(size_t)j] + 1); }      // groups[order] = groups.copy()
  return ng;
}
// A[:, order] in CSC from a generator of entries: for_each(emit) calls emit(row, col) for every entry, the same sequence every time it is called
template <class ForEach>
static int32_t group_columns_of(int64_t m, int64_t n, const int64_t* order, int32_t* groups, ForEach&& for_each) {
  std::vector<int64_t> where((size_t)n, -1);
  for (int64_t j = 0; j < n; ++j) {
    if (order[j] < 0 || order[j] >= n || where[(size_t)order[j]] >= 0) { g_create_error = "group_columns: order is not a permutation"; return MVUS_E_INVALID; }
    where[(size_t)order[j]] = j;
  }
  std::vector<int64_t> indptr((size_t)n + 1, 0);
  bool bad = false;
  int64_t nnz = 0;
  for_each([&](int64_t r, int64_t c) { if (r < 0 || r >= m || c < 0 || c >= n) { bad = true; return; } ++indptr[(size_t)where[(size_t)c] + 1]; ++nnz; });
  if (bad) { g_create_error = "group_columns: entry outside the matrix"; return MVUS_E_INVALID; }
  for (int64_t j = 0; j < n; ++j) indptr[(size_t)j + 1] += indptr[(size_t)j];
  std::vector<int64_t> fill(indptr.begin(), indptr.end() - 1), indices((size_t)nnz);
  for_each([&](int64_t r, int64_t c) { indices[(size_t)fill[(size_t)where[(size_t)c]]++] = r; });
  return group_sparse_permuted(m, n, indptr, indices, order, groups);
}

extern "C" {

int32_t mvus_group_columns(int64_t m, int64_t n, int64_t nnz, const int64_t* rows, const int64_t* cols, const int64_t* order, int32_t* groups) {
  if (m < 0 || n < 1 || nnz < 0 || n > (1ll << 31) - 2 || (nnz > 0 && (!rows || !cols)) || !order || !groups) { g_create_error = "group_columns: bad arguments"; return MVUS_E_INVALID; }
  try {
    return group_columns_of(m, n, order, groups, [&](auto&& emit) { for (int64_t k = 0; k < nnz; ++k) emit(rows[k], cols[k]); });
  } catch (const std::exception& e) {
    g_create_error = e.what();
    return MVUS_E_INVALID;
  }
}

int32_t mvus_fd_groups(const mvus_problem* p, const int32_t* pat, const int32_t* motion_pat, const int64_t* order, int32_t* groups) {
  if (!p || !pat || !order || !groups) { g_create_error = "fd_groups: bad arguments"; return MVUS_E_INVALID; }
  try {
    HostProblem hp;
    const std::string msg = hp.build(p);
    if (!msg.empty()) { g_create_error = msg; return MVUS_E_INVALID; }
    if (hp.T > 0 && !motion_pat) { g_create_error = "fd_groups: motion_reg needs the motion-row codes (mvus_ba_motion_pattern)"; return MVUS_E_INVALID; }
    const int C = hp.C, P = hp.P;
    const bool opt_sync = p->opt_sync != 0, rs_free = p->rs_free != 0;
    // control point p of the concatenated list -> its spline s, column of its x coefficient, stride between coordinates
    std::vector<int64_t> coff((size_t)p->num_splines + 1, 0), xoff((size_t)p->num_splines, 0), ncoef((size_t)p->num_splines, 0);
    {
      int64_t base = (int64_t)C * (3 + P);
      for (int s = 0; s < p->num_splines; ++s) {
        ncoef[(size_t)s] = p->knot_offsets[s + 1] - p->knot_offsets[s] - 4;
        coff[(size_t)s + 1] = coff[(size_t)s] + ncoef[(size_t)s];
        xoff[(size_t)s] = base;
        base += 3 * ncoef[(size_t)s];
      }
    }
    auto spline_cols = [&](int32_t code, auto&& emit_col) {          // the (<= 12) spline columns of a row with this pattern code
      const int32_t pc = pattern_index(code), mk = pattern_mask(code);
      const int s = (int)(std::upper_bound(coff.begin(), coff.end(), (int64_t)pc) - coff.begin()) - 1;
      if (s < 0 || s >= p->num_splines) return false;
      const int64_t base = xoff[(size_t)s] + (pc - coff[(size_t)s]);
      for (int k = 0; k < 4; ++k) if ((mk >> k) & 1) for (int d = 0; d < 3; ++d) emit_col(base + k + d * ncoef[(size_t)s]);
      return true;
    };
    bool bad_code = false;
    const int64_t M = hp.M;
    auto for_each = [&](auto&& emit) {
      for (int c = 0; c < C; ++c) {
        const int64_t a = p->det_offsets[c], b = p->det_offsets[c + 1];
        // Rows with the same set of columns are interchangeable for group_sparse (it only asks whether two columns share a row),
        // so ONE row stands for a run of them: the v row of a detection repeats its u row, and time-ordered detections of one
        // camera repeat the code of their neighbour for a whole knot span (200 k rows -> a few thousand at configs[1]; same groups).
        int32_t prev = -1;
        for (int64_t i = a; i < b; ++i) {
          if (pat[i] < 0 || pat[i] == prev) continue;
          prev = pat[i];
          const int64_t row = 2 * a + (i - a);
          if (opt_sync) { emit(row, (int64_t)c); emit(row, (int64_t)C + c); }
          if (rs_free) emit(row, 2 * (int64_t)C + c);
          for (int k = 0; k < P; ++k) emit(row, 3 * (int64_t)C + (int64_t)c * P + k);
          if (!spline_cols(pat[i], [&](int64_t col) { emit(row, col); })) bad_code = true;
        }
      }
      for (int64_t j = 0; j < hp.T; ++j) {
        if (motion_pat[j] < 0) continue;
        if (!spline_cols(motion_pat[j], [&](int64_t col) { emit(2 * M + j, col); })) bad_code = true;
      }
    };
    const int32_t ng = group_columns_of((int64_t)hp.m, (int64_t)hp.n, order, groups, for_each);
    if (bad_code) { g_create_error = "fd_groups: a pattern code points outside the control points"; return MVUS_E_INVALID; }
    return ng;
  } catch (const std::exception& e) {
    g_create_error = e.what();
    return MVUS_E_INVALID;
  }
}

int mvus_ba_jv(mvus_ba* h, const double* v, double* y) {
  return guarded(h, kKeepsNothing, [&] {
    HipBackend& be = h->be;
    if (!be.has_jacobian) { be.err = "no Jacobian held: call mvus_ba_residual_jacobian first"; return MVUS_E_INVALID; }
    double* vd = be.alloc(be.hp.n); double* yd = be.alloc(be.hp.m);
    be.upload(vd, v, be.hp.n);
    be.jv(vd, yd);
    be.download(y, yd, be.hp.m);
    be.release(vd); be.release(yd);
    return MVUS_OK;
  });
}

int mvus_ba_jtu(mvus_ba* h, const double* u, double* z) {
  return guarded(h, kKeepsNothing, [&] {
    HipBackend& be = h->be;
    if (!be.has_jacobian) { be.err = "no Jacobian held: call mvus_ba_residual_jacobian first"; return MVUS_E_INVALID; }
    double* ud = be.alloc(be.hp.m); double* zd = be.alloc(be.hp.n);
    be.upload(ud, u, be.hp.m);
    be.jtu(ud, zd);
    be.download(z, zd, be.hp.n);
    be.release(ud); be.release(zd);
    return MVUS_OK;
  });
}

int mvus_ba_normal_equations(mvus_ba* h, double* g, double* JtJ_cam, double* band, double* cross, int32_t* W_out) {
  return guarded(h, kKeepsBlocks, [&] {
    if (frozen_on_shards(h->be, "normal_equations") || priors_on_shards(h->be, "normal_equations") || landmarks_on_shards(h->be, "normal_equations")) return MVUS_E_UNSUPPORTED;
    if (!h->schur) h->schur.reset(new HipSchur<HipBackend>(h->be));
    return schur_export(h->be, *h->schur, g, JtJ_cam, band, cross, W_out);
  });
}

int mvus_ba_set_loss(mvus_ba* h, int32_t loss, double f_scale) {
  return guarded(h, kKeepsNothing, [&] {
    HipBackend& be = h->be;
    if (loss < MVUS_LOSS_LINEAR || loss > MVUS_LOSS_ARCTAN) { be.err = "set_loss: unknown loss " + std::to_string(loss); return MVUS_E_INVALID; }
    if (!std::isfinite(f_scale) || !(f_scale > 0)) { be.err = "set_loss: f_scale must be finite and positive"; return MVUS_E_INVALID; }
    // what an LM solve left for its point is the cost and the normal equations of the OLD loss: not kept (f(x) is evaluated again, the same
    // bits); a changed loss is another problem, so the damping starts where a fresh handle's does
    if (loss != be.loss.kind || f_scale != be.loss.fs) be.mem.reset_damping();
    be.loss = LossSpec{loss, f_scale};
    return MVUS_OK;
  });
}

int mvus_ba_set_frozen(mvus_ba* h, const uint8_t* frozen, int64_t count) {
  return guarded(h, kKeepsRawBlocks, [&] {
    HipBackend& be = h->be;
    const int64_t head = (int64_t)be.hp.C * (3 + be.hp.P);
    if (frozen == nullptr || count == 0) count = 0;
    else if (count != head) { be.err = "set_frozen: count must be C * (3 + P) = " + std::to_string(head) + ", not " + std::to_string(count); return MVUS_E_INVALID; }
    bool any = false;
    for (int64_t k = 0; k < count; ++k) {
      if (frozen[k] > 1) { be.err = "set_frozen: frozen[" + std::to_string(k) + "] = " + std::to_string((int)frozen[k]) + " is neither 0 nor 1"; return MVUS_E_INVALID; }
      any = any || frozen[k] != 0;
    }
    if (any && (be.allreduce || be.tshard.on)) {
      be.err = "set_frozen: frozen parameters are not supported on a sharded handle (set_allreduce / set_rccl / set_time_shard)";
      return MVUS_E_UNSUPPORTED;
    }
    // what an LM solve left for its point -- cost, normal equations, the speculative linearisation it adopted -- belongs to the OLD set of
    // unknowns: not kept (f(x) and the blocks are evaluated again; raw blocks of the held Jacobian stay usable); a changed set is another
    // problem, so the damping starts where a fresh handle's does
    const std::vector<uint8_t> before = be.frozen_mask;
    be.set_frozen(frozen, count);
    if (be.frozen_mask != before) be.mem.reset_damping();
    return MVUS_OK;
  });
}

int64_t mvus_ba_num_frozen(const mvus_ba* h) { return h ? h->be.frozen_count : -1; }

int mvus_ba_set_position_priors(mvus_ba* h, int64_t K, const double* t, const double* P, const double* w) {
  return guarded(h, kKeepsBlocks, [&] {
    HipBackend& be = h->be;
    if (K < 0) { be.err = "set_position_priors: K < 0"; return MVUS_E_INVALID; }
    if (K > (1ll << 28)) { be.err = "set_position_priors: more than 2^28 priors"; return MVUS_E_INVALID; }      // (4 K and 3 K stay inside int in the kernels' indices)
    if (t == nullptr || P == nullptr || w == nullptr) K = 0;
    for (int64_t k = 0; k < K; ++k)
      if (!std::isfinite(t[k])) { be.err = "set_position_priors: t[" + std::to_string(k) + "] is not finite"; return MVUS_E_INVALID; }
    for (int64_t k = 0; k < 3 * K; ++k) {
      if (!std::isfinite(P[k])) { be.err = "set_position_priors: P[" + std::to_string(k) + "] is not finite"; return MVUS_E_INVALID; }
      if (!std::isfinite(w[k]) || w[k] < 0.0) { be.err = "set_position_priors: w[" + std::to_string(k) + "] is not a finite weight >= 0"; return MVUS_E_INVALID; }
    }
    if (K > 0 && (be.allreduce || be.tshard.on)) {
      be.err = "set_position_priors: position priors are not supported on a sharded handle (set_allreduce / set_rccl / set_time_shard)";
      return MVUS_E_UNSUPPORTED;
    }
    // what an LM solve left for its point -- cost, normal equations, the speculative linearisation it adopted -- belongs to the OLD set of
    // rows: not kept, as with mvus_ba_set_loss (f(x) is evaluated again, the same bits; blocks of the held Jacobian stay usable: the priors'
    // pass goes on top, HipSchur::assemble_held); the damping history stays
    be.set_priors(K, t, P, w);
    return MVUS_OK;
  });
}

int64_t mvus_ba_num_position_priors(const mvus_ba* h, int64_t* active_out) {
  if (!h) return -1;
  if (active_out) *active_out = h->be.prior_active;
  return h->be.prior.K;
}

int mvus_ba_position_prior_cost(mvus_ba* h, const double* x, double* cost_out, double* r_out) {
  return guarded(h, kKeepsBlocks, [&] {
    HipBackend& be = h->be;
    if (!x || !cost_out) { be.err = "position_prior_cost: NULL argument"; return MVUS_E_INVALID; }
    if (priors_on_shards(be, "position_prior_cost")) return MVUS_E_UNSUPPORTED;
    const int64_t K = be.prior.K;
    *cost_out = 0.0;
    if (K <= 0) return MVUS_OK;
    // an inspection hook: x goes to a buffer of its own -- x_cur, the held Jacobian, f_cur and the blocks HipSchur holds stay as they are
    PoolGuard<HipBackend> pool(be);
    double* xd = pool.get(be.hp.n);
    be.upload(xd, x, be.hp.n);
    double* r = pool.get(3 * K);
    const int pb = (int)std::min<int64_t>(2048, (K + kThreads - 1) / kThreads);
    hipLaunchKernelGGL(k_prior_cost, dim3(pb), dim3(kThreads), 0, be.stream, be.dp, be.prior, (const double*)xd, be.partials, r);
    hipLaunchKernelGGL(k_dot_final, dim3(1), dim3(kThreads), 0, be.stream, pb, (const double*)be.partials, be.scal_out() + be.kPriorCostSlot);
    MVUS_HIP(hipGetLastError());
    *cost_out = 0.5 * be.read_slot(be.kPriorCostSlot);
    if (r_out) {
      std::vector<double> rs((size_t)3 * K);
      be.download(rs.data(), r, 3 * K);
      for (int64_t k = 0; k < K; ++k)
        for (int d = 0; d < 3; ++d) r_out[d * K + be.prior_perm[(size_t)k]] = rs[(size_t)(d * K + k)];
    }
    return MVUS_OK;
  });
}

int mvus_ba_set_landmarks(mvus_ba* h, int64_t L, const double* X, int64_t K, const int32_t* cam, const int32_t* point, const double* uv, const double* w) {
  return guarded(h, kKeepsBlocks, [&] {
    HipBackend& be = h->be;
    if (L < 0 || K < 0) { be.err = "set_landmarks: L or K < 0"; return MVUS_E_INVALID; }
    if (K > (1ll << 24)) { be.err = "set_landmarks: more than 2^24 observations"; return MVUS_E_INVALID; }      // (2 K P stays inside int in the kernels' indices)
    if (X == nullptr || cam == nullptr || point == nullptr || uv == nullptr || w == nullptr) K = 0;
    if (K > 0 && L > (1ll << 28)) { be.err = "set_landmarks: more than 2^28 landmarks"; return MVUS_E_INVALID; }
    for (int64_t k = 0; k < K; ++k) {
      if (cam[k] < 0 || cam[k] >= be.hp.C) { be.err = "set_landmarks: cam[" + std::to_string(k) + "] = " + std::to_string(cam[k]) + " is not a camera of this handle"; return MVUS_E_INVALID; }
      if (point[k] < 0 || point[k] >= L) { be.err = "set_landmarks: point[" + std::to_string(k) + "] = " + std::to_string(point[k]) + " is not a landmark"; return MVUS_E_INVALID; }
    }
    for (int64_t k = 0; k < (K > 0 ? 3 * L : 0); ++k)
      if (!std::isfinite(X[k])) { be.err = "set_landmarks: X[" + std::to_string(k) + "] is not finite"; return MVUS_E_INVALID; }
    for (int64_t k = 0; k < 2 * K; ++k) {
      if (!std::isfinite(uv[k])) { be.err = "set_landmarks: uv[" + std::to_string(k) + "] is not finite"; return MVUS_E_INVALID; }
      if (!std::isfinite(w[k]) || w[k] < 0.0) { be.err = "set_landmarks: w[" + std::to_string(k) + "] is not a finite weight >= 0"; return MVUS_E_INVALID; }
    }
    if (K > 0 && (be.allreduce || be.tshard.on)) {
      be.err = "set_landmarks: landmarks are not supported on a sharded handle (set_allreduce / set_rccl / set_time_shard)";
      return MVUS_E_UNSUPPORTED;
    }
    // what an LM solve left for its point belongs to the OLD set of rows: not kept, as with mvus_ba_set_position_priors (blocks of the held
    // Jacobian stay usable: the landmarks' pass goes on top, HipSchur::assemble_held); the damping history stays
    be.set_landmarks(L, X, K, cam, point, uv, w);
    return MVUS_OK;
  });
}

int64_t mvus_ba_num_landmark_observations(const mvus_ba* h, int64_t* rows_out) {
  if (!h) return -1;
  if (rows_out) *rows_out = h->be.lm_rows;
  return h->be.lm.K;
}

// the two inspection hooks: x goes to a buffer of its own and the cameras are decoded there -- x_cur, the held Jacobian, f_cur and the blocks
// HipSchur holds stay as they are (the cached camera states are decoded again by whoever needs them next)
static int landmark_inspect(mvus_ba* h, const char* who, const double* x, double* cost_out, double* r_out, double* J_out) {
  return guarded(h, kKeepsBlocks, [&] {
    HipBackend& be = h->be;
    if (!x || (!cost_out && !r_out && !J_out)) { be.err = std::string(who) + ": NULL argument"; return MVUS_E_INVALID; }
    if (landmarks_on_shards(be, who)) return MVUS_E_UNSUPPORTED;
    const int64_t K = be.lm.K, P = be.hp.P;
    if (cost_out) *cost_out = 0.0;
    if (K <= 0) return MVUS_OK;
    PoolGuard<HipBackend> pool(be);
    double* xd = pool.get(be.hp.n);
    be.upload(xd, x, be.hp.n);
    double* r = pool.get(2 * K);
    double* J = J_out ? pool.get(2 * K * P) : nullptr;
    be.ensure_cams(xd);
    const int lb = (int)std::min<int64_t>(2048, (K + kThreads - 1) / kThreads);
    hipLaunchKernelGGL(k_landmark_cost, dim3(lb), dim3(kThreads), 0, be.stream, be.dp, be.lm, (const CamState*)be.cams, be.partials, r, J);
    hipLaunchKernelGGL(k_dot_final, dim3(1), dim3(kThreads), 0, be.stream, lb, (const double*)be.partials, be.scal_out() + be.kLandmarkCostSlot);
    MVUS_HIP(hipGetLastError());
    const double twice = be.read_slot(be.kLandmarkCostSlot);
    if (cost_out) *cost_out = 0.5 * twice;
    if (r_out) {
      std::vector<double> rs((size_t)2 * K);
      be.download(rs.data(), r, 2 * K);
      for (int64_t k = 0; k < K; ++k)
        for (int d = 0; d < 2; ++d) r_out[d * K + be.lm_perm[(size_t)k]] = rs[(size_t)(d * K + k)];
    }
    if (J_out) {
      std::vector<double> Js((size_t)(2 * K * P));
      be.download(Js.data(), J, 2 * K * P);
      for (int64_t k = 0; k < K; ++k) std::memcpy(J_out + be.lm_perm[(size_t)k] * 2 * P, Js.data() + k * 2 * P, sizeof(double) * 2 * P);
    }
    return MVUS_OK;
  });
}

int mvus_ba_landmark_cost(mvus_ba* h, const double* x, double* cost_out, double* r_out) {
  if (h && !cost_out) { h->be.err = "landmark_cost: NULL argument"; return MVUS_E_INVALID; }
  return landmark_inspect(h, "landmark_cost", x, cost_out, r_out, nullptr);
}

int mvus_ba_landmark_rows(mvus_ba* h, const double* x, double* r_out, double* J_out) {
  return landmark_inspect(h, "landmark_rows", x, nullptr, r_out, J_out);
}

int mvus_ba_robust_cost(mvus_ba* h, const double* x, double* cost_out, double* weights_out) {
  return guarded(h, kKeepsNothing, [&] {
    HipBackend& be = h->be;
    if (!x || !cost_out) { be.err = "robust_cost: NULL argument"; return MVUS_E_INVALID; }
    if (be.allreduce || be.tshard.on) { be.err = "robust_cost: not supported on a sharded handle"; return MVUS_E_UNSUPPORTED; }
    be.upload(be.x_cur, x, be.hp.n);
    be.residual_sq(be.x_cur, be.f_cur, be.scal_out() + be.kCostSlot, nullptr, 0, false);      // (outside the LM driver's block, inside the host-summed range; error_BA's rows only)
    double twice = 0;
    be.fetch(be.scal_out() + be.kCostSlot, 1, &twice);
    *cost_out = 0.5 * twice;
    if (weights_out) {
      PoolGuard<HipBackend> pool(be);
      double* w = pool.get(be.hp.m);
      if (be.hp.m > 0) hipLaunchKernelGGL(k_loss_weights, dim3((unsigned)((be.hp.m + kThreads - 1) / kThreads)), dim3(kThreads), 0, be.stream, (long long)be.hp.m, (const double*)be.f_cur, be.loss, w);
      MVUS_HIP(hipGetLastError());
      be.download(weights_out, w, be.hp.m);
    }
    return MVUS_OK;
  });
}

// mvus_ba_covariance and mvus_ba_detection_covariance: one chain (CovChain::run), the second with the detection pass behind stage 8
static int covariance_call(mvus_ba* h, const char* who, const double* x, double sigma2, const DetCovOut* det, double* cov_cam, double* cov_band,
                           uint8_t* estimated, double* sigma2_out, int64_t* dof_out) {
  return guarded(h, kKeepsNothing, [&] {
    HipBackend& be = h->be;
    const std::string pre = std::string(who) + ": ";
    if (!x || !std::isfinite(sigma2)) { be.err = pre + "x is NULL or sigma2 is not finite"; return MVUS_E_INVALID; }
    if (be.allreduce || be.tshard.on) { be.err = pre + "not supported on a sharded handle (set_allreduce / set_rccl / set_time_shard): one rank only"; return MVUS_E_UNSUPPORTED; }
    // what an LM solve left for its point (cost, blocks, the speculative linearisation) is not kept, as with mvus_ba_set_loss -- the blocks
    // are overwritten below; the damping history stays: a later solve returns the bits it would have returned without this call
    if (be.hp.C * (3 + be.hp.P) > 1152) { be.err = pre + "more than 1152 camera-side unknowns"; return MVUS_E_UNSUPPORTED; }
    if (!h->schur) h->schur.reset(new HipSchur<HipBackend>(be));
    if (!h->cov) h->cov.reset(new CovChain<HipBackend>(be));
    // the (robust) cost at x, then the analytic Jacobian of x held as mvus_ba_residual_jacobian holds it
    be.upload(be.x_cur, x, be.hp.n);
    be.residual_sq(be.x_cur, be.f_cur, be.scal_out() + be.kCostSlot);
    double twice = 0;
    be.fetch(be.scal_out() + be.kCostSlot, 1, &twice);
    if (!std::isfinite(twice)) { be.err = pre + "residuals are not finite at x"; return MVUS_E_NUMERIC; }
    be.jacobian(be.x_cur, be.f_cur, MVUS_JAC_ANALYTIC);
    be.held_analytic_at_xcur = true;
    CovResult res;
    h->cov->who = who;
    const int rc = h->cov->run(*h->schur, 0.5 * twice, sigma2, cov_cam, cov_band, estimated, res, det);
    if (rc != MVUS_OK) return rc;
    if (sigma2_out) *sigma2_out = res.sigma2;
    if (dof_out) *dof_out = res.dof;
    return MVUS_OK;
  });
}

int mvus_ba_covariance(mvus_ba* h, const double* x, double sigma2, double* cov_cam, double* cov_band, uint8_t* estimated,
                       double* sigma2_out, int64_t* dof_out) {
  return covariance_call(h, "covariance", x, sigma2, nullptr, cov_cam, cov_band, estimated, sigma2_out, dof_out);
}

int mvus_ba_detection_covariance(mvus_ba* h, const double* x, double sigma2, double* e_out, double* pcov_out, double* t2_out, double* cov_cam,
                                 double* cov_band, uint8_t* estimated, double* sigma2_out, int64_t* dof_out) {
  const DetCovOut det{e_out, pcov_out, t2_out};
  return covariance_call(h, "detection_covariance", x, sigma2, &det, cov_cam, cov_band, estimated, sigma2_out, dof_out);
}

int32_t mvus_ba_detection_covariance_ms(mvus_ba* h, double* ms_out) {
  if (!h || !h->cov || !h->cov->det_timed) return MVUS_E_INVALID;
  if (ms_out) *ms_out = h->cov->det_ms;
  return MVUS_OK;
}

int32_t mvus_ba_covariance_stage_ms(mvus_ba* h, double* ms_out, const char** names_out, int32_t count) {
  if (!h || !h->cov || !h->cov->timed) return MVUS_E_INVALID;
  for (int s = 0; s < count && s < kCovStages; ++s) {
    if (ms_out) ms_out[s] = h->cov->stage_ms[s];
    if (names_out) names_out[s] = cov_stage_name(s);
  }
  return kCovStages;
}

int mvus_ba_lm_step(mvus_ba* h, double lambda, double* p_out) {
  return guarded(h, kKeepsBlocks, [&] {
    HipBackend& be = h->be;
    if (!p_out || !(lambda >= 0)) { be.err = "lm_step: bad arguments"; return MVUS_E_INVALID; }
    if (!be.has_jacobian) { be.err = "no Jacobian held: call mvus_ba_residual_jacobian first"; return MVUS_E_INVALID; }
    if (frozen_on_shards(be, "lm_step") || priors_on_shards(be, "lm_step") || landmarks_on_shards(be, "lm_step")) return MVUS_E_UNSUPPORTED;
    if (be.hp.C * (3 + be.hp.P) > 1152) throw HipError{"LM_SCHUR: reduced camera system larger than 1152 unknowns"};
    if (!h->schur) h->schur.reset(new HipSchur<HipBackend>(be));
    HipSchur<HipBackend>& sc = *h->schur;
    sc.assemble_held(be);
    sc.solve_async(lambda);
    be.download(p_out, sc.step_ptr(), be.hp.n);          // synchronises
    if (!sc.solve_ok() && sc.retry_same()) { sc.solve_async(lambda); be.download(p_out, sc.step_ptr(), be.hp.n); }
    if (!sc.solve_ok()) { be.err = "lm_step: the damped normal equations are not positive definite at this lambda"; return MVUS_E_NUMERIC; }
    return MVUS_OK;
  });
}

int mvus_ba_lsmr(mvus_ba* h, const double* b, const double* D, const double* E, double damp, double atol, double btol, double conlim,
                 int64_t maxiter, double* x_out, int32_t* itn_out, int32_t* istop_out, double* norms_out) {
  return guarded(h, kKeepsBlocks, [&] {
    HipBackend& be = h->be;
    if (!b || !x_out || !(damp >= 0)) { be.err = "lsmr: bad arguments"; return MVUS_E_INVALID; }
    if (be.allreduce || be.tshard.on) { be.err = "lsmr: not supported on a sharded handle (set_allreduce / set_rccl / set_time_shard): one rank only"; return MVUS_E_UNSUPPORTED; }
    if (!be.has_jacobian) { be.err = "no Jacobian held: call mvus_ba_residual_jacobian first"; return MVUS_E_INVALID; }
    // an inspection hook: b, D, E and x live in buffers of their own -- x_cur, f_cur, the held Jacobian and the blocks HipSchur holds stay
    // as they are.  With a mask in force the solver's Jacobian is the frozen one (k_freeze_jacobian, as inside a TRF solve): the held
    // blocks are set aside and put back, so mvus_ba_jv / jtu / lm_step after the call still see error_BA's own
    const int64_t n = be.hp.n, m = be.hp.m;
    PoolGuard<HipBackend> pool(be);
    double* bd = pool.get(m);
    double* xd = pool.get(n);
    double* Dd = D ? pool.get(n) : nullptr;
    double* Ed = E ? pool.get(n) : nullptr;
    be.upload(bd, b, m);
    if (D) be.upload(Dd, D, n);
    if (E) be.upload(Ed, E, n);
    const int64_t jlen = (int64_t)j_doubles(be.hp.NS, be.dp.n_chunks);
    double* Jsave = nullptr;
    if (be.frozen_count > 0 && be.dp.n_chunks > 0) {
      Jsave = pool.get(jlen);
      MVUS_HIP(hipMemcpyAsync(Jsave, be.J, sizeof(double) * jlen, hipMemcpyDeviceToDevice, be.stream));
      be.freeze_jacobian();
    }
    struct Restore {      // (also when the run throws)
      HipBackend& be; double* save; int64_t len;
      ~Restore() { if (save) { (void)hipMemcpyAsync(be.J, save, sizeof(double) * len, hipMemcpyDeviceToDevice, be.stream); (void)hipStreamSynchronize(be.stream); } }
    } restore{be, Jsave, jlen};
    LsmrScalars sc;
    int itn = 0, istop = 0;
    {
      Lsmr<HipBackend> lsmr(be);
      istop = lsmr.run(Dd, Ed, bd, damp, atol, btol, conlim, maxiter > 0 ? maxiter : std::min<int64_t>(m + (E ? n : 0), n), xd, &itn, &sc);
    }
    be.download(x_out, xd, n);
    if (itn_out) *itn_out = itn;
    if (istop_out) *istop_out = istop;
    if (norms_out) { norms_out[0] = sc.normr; norms_out[1] = sc.normar; norms_out[2] = sc.normA; norms_out[3] = sc.condA; }
    return MVUS_OK;
  });
}

int mvus_ba_solve(mvus_ba* h, double* x, const mvus_solve_opts* opts, mvus_result* res, double* f_out) {
  return guarded(h, kKeepsNothing, [&] {
    HipBackend& be = h->be;
    if (!x || !opts || !res) { be.err = "NULL argument"; return MVUS_E_INVALID; }
    const auto t0 = std::chrono::steady_clock::now();
    const int64_t n = be.hp.n;
    std::vector<double> xv;                          // (the TRF path works on a vector; the LM driver on the caller's buffer itself)
    if (opts->solver != MVUS_SOLVER_LM_SCHUR || opts->jac_mode == MVUS_JAC_PATTERN) xv.assign(x, x + n);
    if ((int64_t)be.lb_fixed.size() != n) {          // the box of the rs block (common.py:652-668): fixed for the handle, built once
      be.lb_fixed.assign(n, -INFINITY); be.ub_fixed.assign(n, INFINITY);
      if (be.hp.rs_bounds) for (int c = 0; c < be.hp.C; ++c) { be.lb_fixed[2 * be.hp.C + c] = 0.0; be.ub_fixed[2 * be.hp.C + c] = 1.0; }
    }
    // A held unknown has no box (both solvers): scipy's make_strictly_feasible would move an rs that sits ON its bound by 1e-10 before the
    // first evaluation, and a held rs outside [0, 1] is the caller's business.  Without a mask: the handle's own vectors, as always.
    std::vector<double> lbf, ubf;
    if (be.frozen_count > 0 && be.hp.rs_bounds) {
      lbf = be.lb_fixed; ubf = be.ub_fixed;
      for (int64_t k = 0; k < (int64_t)be.frozen_mask.size(); ++k) if (be.frozen_mask[k]) { lbf[k] = -INFINITY; ubf[k] = INFINITY; }
    }
    const std::vector<double>&lb = lbf.empty() ? be.lb_fixed : lbf, &ub = ubf.empty() ? be.ub_fixed : ubf;
    SolveOptions so;
    so.jac_mode = opts->jac_mode; so.max_nfev = opts->max_nfev; so.ftol = opts->ftol; so.xtol = opts->xtol; so.gtol = opts->gtol;
    so.lsmr_atol = opts->lsmr_atol; so.lsmr_btol = opts->lsmr_btol; so.lsmr_conlim = opts->lsmr_conlim;
    so.lsmr_maxiter = opts->lsmr_maxiter; so.verbose = opts->verbose; so.lm_lambda_min = opts->lm_lambda_min >= 0 ? opts->lm_lambda_min : 0.0;
    so.lm_trust_radius = opts->lm_trust_radius;
    if (so.jac_mode == MVUS_JAC_PATTERN && !be.pattern_uploaded) {
      be.upload(be.x_cur, xv.data(), n);
      be.set_pattern(be.x_cur);
    }
    if (so.jac_mode == MVUS_JAC_FD && (!be.has_pattern || be.fd_ngroups <= 0)) {
      be.err = "MVUS_JAC_FD: call mvus_ba_set_pattern(x0) and mvus_ba_set_fd_groups first";
      return MVUS_E_INVALID;
    }
    if (be.robust()) {               // what the loss does not reach refuses: it never silently solves the linear problem
      const char* what = opts->solver != MVUS_SOLVER_LM_SCHUR ? "MVUS_SOLVER_TRF_LSMR"
                         : so.jac_mode != MVUS_JAC_ANALYTIC   ? "a Jacobian mode other than MVUS_JAC_ANALYTIC"
                         : (be.allreduce || be.tshard.on)     ? "a sharded handle (set_allreduce / set_rccl / set_time_shard)"
                                                              : nullptr;
      if (what) { be.err = std::string("a robust loss (mvus_ba_set_loss) is not supported with ") + what + ": MVUS_SOLVER_LM_SCHUR with MVUS_JAC_ANALYTIC on one rank only"; return MVUS_E_UNSUPPORTED; }
    }
    if (frozen_on_shards(be, "solve") || priors_on_shards(be, "solve") || landmarks_on_shards(be, "solve")) return MVUS_E_UNSUPPORTED;
    if (be.lm_active > 0 && opts->solver != MVUS_SOLVER_LM_SCHUR) {         // never solved with the landmarks silently dropped
      be.err = "landmarks (mvus_ba_set_landmarks) are not supported with MVUS_SOLVER_TRF_LSMR: MVUS_SOLVER_LM_SCHUR only";
      return MVUS_E_UNSUPPORTED;
    }
    if (be.prior_active > 0 && opts->solver != MVUS_SOLVER_LM_SCHUR) {      // never solved with the priors silently dropped
      be.err = "position priors (mvus_ba_set_position_priors) are not supported with MVUS_SOLVER_TRF_LSMR: MVUS_SOLVER_LM_SCHUR only";
      return MVUS_E_UNSUPPORTED;
    }
    SolveResult sr;
    be.held_analytic_at_xcur = false;
    if (opts->solver == MVUS_SOLVER_LM_SCHUR) {
      if (be.hp.C * (3 + be.hp.P) > 1152) throw HipError{"LM_SCHUR: reduced camera system larger than 1152 unknowns"};
      if (!h->schur) h->schur.reset(new HipSchur<HipBackend>(be));
      so.lm_lambda0 = be.mem.damping().lambda; so.lm_nu0 = be.mem.damping().nu;
      // knots closer than a frame (band wider than six control points): more control points than detections -- the spline is
      // held by the motion regulariser alone between the data, and a converging LM whose damping falls to 3e-3 diag(H) follows
      // noise along those directions (the incremental loop then ends 3 m off; with 0.3 it ends where TRF + LSMR ends:
      // profiles/round4/r04_loop_lm_wide_band_damping.txt).  The floor of such problems is at least kLambdaMinWide.
      constexpr double kLambdaMinWide = 0.3;
      if (h->schur->wide && so.lm_trust_radius < 0) so.lm_lambda_min = std::max(so.lm_lambda_min, kLambdaMinWide);      // (a trust region bounds those steps itself)
      sr = lm_schur(be, *h->schur, x, lb, ub, so, be.f_cur);
      if (!sr.error) be.mem.store_damping(sr.lm_lambda, sr.lm_nu);
      if (sr.jac_stale) be.has_jacobian = false;      // mvus_ba_jv / jtu / lm_step must not pair J(x_old) with f(x_new)
    }
    else if (be.frozen_count > 0) {
      // TRF + LSMR with a mask: the frozen slots of the stored Jacobian are zeroed behind every evaluation (analytic, pattern, FD), so
      // g = J^T f, the LSMR solution started from zero and with them every step are exactly 0 there.
      struct Flag { bool& f; explicit Flag(bool& b) : f(b) { f = true; } ~Flag() { f = false; } } on(be.freeze_stored_jacobian);
      sr = trf_lsmr(be, xv, lb, ub, so, be.f_cur);
      be.has_jacobian = false;      // (the stored Jacobian is the masked one: mvus_ba_jv / jtu / lm_step take error_BA's own)
    }
    else sr = trf_lsmr(be, xv, lb, ub, so, be.f_cur);
    const bool lm = opts->solver == MVUS_SOLVER_LM_SCHUR;
    if (sr.error == -4) {            // a row left the time slice: the point reached so far goes back to the caller, who re-cuts there (already in x)
      MVUS_HIP(hipStreamSynchronize(be.stream));
      h->drop_schur();               // (the device flag is raised: the next solve on this handle starts from fresh storage)
      res->cost = sr.cost; res->optimality = 0; res->nfev = sr.nfev; res->njev = sr.njev; res->status = 0; res->lin_iters = sr.lin_iters;
      res->initial_cost = sr.initial_cost; res->solve_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
      be.err = "time shard: a detection or motion row reaches control points outside this rank's slice +- halo (the time stamps have drifted since the cuts were made): re-cut at the returned point";
      return MVUS_E_RESHARD;
    }
    if (sr.error) { be.err = "residuals are not finite in the initial point, or x0 is outside of the bounds"; return MVUS_E_NUMERIC; }
    if (!lm) std::memcpy(x, xv.data(), sizeof(double) * n);
    if (f_out) be.download(f_out, be.f_cur, be.hp.m);
    // (an LM solve that ends on its evaluation budget may leave the linearisation at the returned point running: x and the scalars are
    // on the host already -- mapped memory, fetched behind an event -- and whatever reads those blocks is a later call on this stream)
    if (!(lm && sr.async_tail && !f_out)) MVUS_HIP(hipStreamSynchronize(be.stream));
    res->cost = sr.cost; res->optimality = sr.optimality; res->nfev = sr.nfev; res->njev = sr.njev; res->status = sr.status;
    res->lin_iters = sr.lin_iters; res->initial_cost = sr.initial_cost;
    res->solve_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return MVUS_OK;
  });
}

// The two registration entry points share everything but the schedule's length and the outputs.  The scalar arguments are checked before
// the handle is looked at (so a NULL handle still gets their message, through mvus_last_error(NULL)), the batch against C and P next, and
// only then is the device touched.
static int register_call(mvus_ba* h, const char* who, const double* x, int32_t B, const int32_t* cam, const double* start, RegOpts o,
                         bool linearize_only, const RegisterOutputs& out) {
  char msg[160];
  if (reg_check_scalars(who, B, o.max_nfev, o.ftol, o.xtol, o.gtol, msg, sizeof msg)) {
    if (h) h->be.err = msg; else g_create_error = msg;
    return MVUS_E_INVALID;
  }
  if (B == 0) return MVUS_OK;                    // nothing to do: no state is looked at
  if (!h) { g_create_error = std::string(who) + ": NULL handle"; return MVUS_E_INVALID; }
  return guarded(h, kTransparent, [&] {      // nothing the handle holds is touched: what an LM solve left for the very next call stays valid for the call after this one
    HipBackend& be = h->be;
    if (reg_check_batch(who, be.hp.C, be.hp.P, B, cam, start, msg, sizeof msg)) { be.err = msg; return MVUS_E_INVALID; }
    if (!x) { be.err = std::string(who) + ": x is NULL"; return MVUS_E_INVALID; }
    if (be.allreduce || be.tshard.on) { be.err = std::string(who) + ": not supported on a sharded handle (set_allreduce / set_rccl / set_time_shard): one rank only"; return MVUS_E_UNSUPPORTED; }
    // the per-camera problems hold the detection rows only: with landmarks set they would drop rows that involve exactly that camera
    if (be.lm.K > 0) { be.err = std::string(who) + ": not supported while landmark observations are set (mvus_ba_set_landmarks): clear them first"; return MVUS_E_UNSUPPORTED; }
    if (!h->reg) h->reg.reset(new RegisterWork());
    return register_run(be, *h->reg, x, B, cam, start, o, linearize_only, out);
  });
}

int mvus_ba_register_cameras(mvus_ba* h, const double* x, int32_t B, const int32_t* cam, const double* start,
                             int32_t max_nfev, double ftol, double xtol, double gtol, double lambda0, double lambda_min, double inlier_thres,
                             double* cam_out, double* cost_out, double* cost0_out, int32_t* nfev_out, int32_t* status_out,
                             int64_t* visible_out, int64_t* inliers_out) {
  const RegOpts o{max_nfev, 0, ftol, xtol, gtol, lambda0, lambda_min >= 0 ? lambda_min : 0.0, inlier_thres};
  const RegisterOutputs out{cam_out, cost_out, cost0_out, nfev_out, status_out, visible_out, inliers_out, nullptr, nullptr};
  return register_call(h, "register_cameras", x, B, cam, start, o, false, out);
}

int mvus_ba_register_linearize(mvus_ba* h, const double* x, int32_t B, const int32_t* cam, const double* start,
                               double* H_out, double* g_out, double* cost_out, int64_t* visible_out) {
  const RegOpts o{1, 0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  const RegisterOutputs out{nullptr, nullptr, cost_out, nullptr, nullptr, visible_out, nullptr, H_out, g_out};
  return register_call(h, "register_linearize", x, B, cam, start, o, true, out);
}

int mvus_ba_outlier_mask(mvus_ba* h, const double* x, double thres, uint8_t* keep) {
  return guarded(h, kKeepsNothing, [&] {
    HipBackend& be = h->be;
    be.upload(be.x_cur, x, be.hp.n);
    be.residual(be.x_cur, be.f_cur);
    DeviceOwner tmp;
    uint8_t* kd = tmp.device<uint8_t>((size_t)be.hp.M);
    if (be.dp.n_chunks > 0) hipLaunchKernelGGL(k_outlier_mask, dim3(be.dp.n_chunks), dim3(kThreads), 0, be.stream, be.dp, be.f_cur, thres, kd);
    MVUS_HIP(hipMemcpyAsync(keep, kd, be.hp.M, hipMemcpyDeviceToHost, be.stream));
    MVUS_HIP(hipStreamSynchronize(be.stream));
    return MVUS_OK;
  });
}

int mvus_ba_remove_outliers(mvus_ba* h, const double* x, double thres, uint8_t* keep_out, int64_t* det_offsets_out) {
  return guarded(h, kKeepsNothing, [&] {
    HipBackend& be = h->be;
    be.upload(be.x_cur, x, be.hp.n);
    h->drop_schur();                        // sized by the launch tables
    be.remove_outliers(be.x_cur, thres, keep_out, det_offsets_out);
    if (be.allreduce) be.reduce_row_count();
    return MVUS_OK;
  });
}

// ---- RCCL from the library: librccl.so.1 opened at run time, five entry points ----
namespace {
struct RcclApi {
  void* lib = nullptr;
  int (*GetUniqueId)(void*) = nullptr;
  int (*CommInitRank)(void**, int, mvus_rccl_id, int) = nullptr;
  int (*AllReduce)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
  int (*CommDestroy)(void*) = nullptr;
  const char* (*GetErrorString)(int) = nullptr;
  std::string err;
  bool load() {
    if (lib) return true;
    lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
    if (!lib) lib = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL);
    if (!lib) { err = std::string("librccl.so.1 cannot be opened: ") + dlerror(); return false; }
    GetUniqueId = reinterpret_cast<decltype(GetUniqueId)>(dlsym(lib, "ncclGetUniqueId"));
    CommInitRank = reinterpret_cast<decltype(CommInitRank)>(dlsym(lib, "ncclCommInitRank"));
    AllReduce = reinterpret_cast<decltype(AllReduce)>(dlsym(lib, "ncclAllReduce"));
    CommDestroy = reinterpret_cast<decltype(CommDestroy)>(dlsym(lib, "ncclCommDestroy"));
    GetErrorString = reinterpret_cast<decltype(GetErrorString)>(dlsym(lib, "ncclGetErrorString"));
    if (!GetUniqueId || !CommInitRank || !AllReduce || !CommDestroy) { err = "librccl.so.1 lacks ncclGetUniqueId / ncclCommInitRank / ncclAllReduce / ncclCommDestroy"; dlclose(lib); lib = nullptr; return false; }
    return true;
  }
  std::string what(int rc) const { return GetErrorString ? std::string(GetErrorString(rc)) : ("ncclResult " + std::to_string(rc)); }
};
RcclApi g_rccl;
std::mutex g_rccl_mutex;
constexpr int kNcclFloat64 = 8, kNcclSum = 0;      // ncclDataType_t / ncclRedOp_t of rccl.h
}  // namespace

static int rccl_allreduce_cb(void* user, void* buf, size_t count, void* stream) {
  mvus_rccl_handle* c = static_cast<mvus_rccl_handle*>(user);
  return g_rccl.AllReduce(buf, buf, count, kNcclFloat64, kNcclSum, c->comm, static_cast<hipStream_t>(stream));
}

int mvus_ba_set_allreduce(mvus_ba* h, mvus_allreduce_fn fn, void* user, int32_t is_root) {
  return guarded(h, kKeepsNothing, [&] {
    HipBackend& be = h->be;
    if (fn != rccl_allreduce_cb && h->rccl.comm) {      // another route (or none) replaces the library's own communicator: tear it down
      MVUS_HIP(hipStreamSynchronize(be.stream));
      if (g_rccl.CommDestroy) (void)g_rccl.CommDestroy(h->rccl.comm);
      h->rccl.comm = nullptr;
    }
    be.allreduce = fn; be.allreduce_user = user; be.is_root = is_root;
    be.m_glob = be.hp.m;
    if (fn) be.reduce_row_count();
    return MVUS_OK;
  });
}

}  // extern "C"
mvus_ba::~mvus_ba() {
  reg.reset();
  cov.reset();
  schur.reset();
  if (rccl.comm && g_rccl.CommDestroy) { (void)hipStreamSynchronize(be.stream); (void)g_rccl.CommDestroy(rccl.comm); }
}
extern "C" {

int mvus_rccl_available(void) {
  std::lock_guard<std::mutex> lock(g_rccl_mutex);
  if (!g_rccl.load()) { g_create_error = g_rccl.err; return MVUS_E_COMM; }
  return MVUS_OK;
}

int mvus_rccl_unique_id(uint8_t id_out[128]) {
  if (!id_out) return MVUS_E_INVALID;
  std::lock_guard<std::mutex> lock(g_rccl_mutex);
  if (!g_rccl.load()) { g_create_error = g_rccl.err; return MVUS_E_COMM; }
  mvus_rccl_id id;
  const int rc = g_rccl.GetUniqueId(&id);
  if (rc != 0) { g_create_error = "ncclGetUniqueId: " + g_rccl.what(rc); return MVUS_E_COMM; }
  std::memcpy(id_out, id.internal, 128);
  return MVUS_OK;
}

int mvus_ba_set_rccl(mvus_ba* h, const uint8_t id[128], int32_t rank, int32_t world, int32_t is_root) {
  return guarded(h, kKeepsNothing, [&] {
    HipBackend& be = h->be;
    if (!id || world < 1 || rank < 0 || rank >= world) { be.err = "set_rccl: bad arguments"; return MVUS_E_INVALID; }
    {
      std::lock_guard<std::mutex> lock(g_rccl_mutex);
      if (!g_rccl.load()) { be.err = g_rccl.err; return MVUS_E_COMM; }
    }
    // the route is torn down BEFORE anything can fail: a failed call leaves the handle without a collective route (sums of one
    // rank), never with a callback that points at a destroyed or half-initialised communicator
    MVUS_HIP(hipStreamSynchronize(be.stream));
    if (be.allreduce == rccl_allreduce_cb) { be.allreduce = nullptr; be.allreduce_user = nullptr; }
    if (h->rccl.comm) { (void)g_rccl.CommDestroy(h->rccl.comm); h->rccl.comm = nullptr; }
    mvus_rccl_id uid;
    std::memcpy(uid.internal, id, 128);
    const int rc = g_rccl.CommInitRank(&h->rccl.comm, world, uid, rank);
    if (rc != 0) { h->rccl.comm = nullptr; be.err = "ncclCommInitRank: " + g_rccl.what(rc); return MVUS_E_COMM; }
    return mvus_ba_set_allreduce(h, rccl_allreduce_cb, &h->rccl, is_root);
  });
}

int mvus_ba_time_allreduce(mvus_ba* h, int64_t count, int32_t reps, double* avg_ms) {
  return guarded(h, kKeepsNothing, [&] {
    HipBackend& be = h->be;
    if (count < 1 || reps < 1 || !avg_ms) { be.err = "bad arguments"; return MVUS_E_INVALID; }
    if (!be.allreduce) { be.err = "time_allreduce: no all-reduce route installed"; return MVUS_E_INVALID; }
    PoolGuard<HipBackend> pool(be);
    double* buf = pool.get(count);
    be.fill(buf, 0.0, count);
    *avg_ms = time_on_stream(be.stream, 3, reps, [&] { be.reduce(buf, (size_t)count); });
    return MVUS_OK;
  });
}

int mvus_ba_set_time_shard(mvus_ba* h, int32_t rank, int32_t world, const int32_t* ctrl_cuts, int32_t halo) {
  return guarded(h, kKeepsNothing, [&] {
    HipBackend& be = h->be;
    if (world < 1 || rank < 0 || rank >= world || !ctrl_cuts || halo < 1) { be.err = "set_time_shard: bad arguments"; return MVUS_E_INVALID; }
    if (ctrl_cuts[0] != 0 || ctrl_cuts[world] != be.hp.N) { be.err = "set_time_shard: cuts must run from 0 to the number of control points"; return MVUS_E_INVALID; }
    for (int r = 0; r < world; ++r)
      if (ctrl_cuts[r + 1] <= ctrl_cuts[r]) { be.err = "set_time_shard: cuts must increase"; return MVUS_E_INVALID; }
    h->drop_schur();
    be.tshard.on = world > 1; be.tshard.rank = rank; be.tshard.world = world; be.tshard.halo = halo;
    be.tshard.cuts.assign(ctrl_cuts, ctrl_cuts + world + 1);
    be.dp.mot_lo = be.tshard.on ? ctrl_cuts[rank] : 0;
    be.dp.mot_hi = be.tshard.on ? ctrl_cuts[rank + 1] : 0x7fffffff;
    be.has_jacobian = false;
    return MVUS_OK;
  });
}

int mvus_ba_time_kernel(mvus_ba* h, int32_t which, int32_t launches, double* avg_ms) {
  return guarded(h, kKeepsNothing, [&] {
    HipBackend& be = h->be;
    if (launches < 1 || !avg_ms || which < 0 || which > 8) { be.err = "bad arguments"; return MVUS_E_INVALID; }
    if (which >= 7 && be.lm_active <= 0) { be.err = "time_kernel: which = 7 / 8 need landmark observations (mvus_ba_set_landmarks)"; return MVUS_E_INVALID; }
    be.ensure_J();
    PoolGuard<HipBackend> pool(be);
    double* vn = pool.get(be.hp.n); double* um = pool.get(be.hp.m); double* zn = pool.get(be.hp.n); double* ym = pool.get(be.hp.m);
    be.fill(vn, 1e-3, be.hp.n); be.fill(um, 1e-3, be.hp.m);
    be.ensure_cams(be.x_cur);
    if (which >= 2 && which <= 4 && !be.has_jacobian) be.jacobian(be.x_cur, be.f_cur, MVUS_JAC_ANALYTIC);
    if (which == 6) be.residual(be.x_cur, be.f_cur);
    const dim3 g(std::max(be.dp.n_chunks, 1)), b(kThreads);
    if ((which == 4 || which == 6 || which == 8) && !h->schur) h->schur.reset(new HipSchur<HipBackend>(be));
    HipSchur<HipBackend>* schur = h->schur.get();
    // which == 1: the outputs (J, span, f) rotate over enough buffer sets that the bytes written between two uses of a
    // set exceed the 256 MiB Infinity Cache several times -- every launch writes to HBM, not into lines the previous
    // launch left in the cache.  which == 5 is the same kernel re-launched into ONE set, for comparison.
    struct OutSet { double* J; int32_t* span; double* f; };
    std::vector<OutSet> sets{{be.J, be.span, be.f_cur}};
    DeviceOwner extra;                        // the sets in rotation besides the handle's own: freed on every exit
    if (which == 1) {
      const size_t jb = sizeof(double) * j_doubles(be.hp.NS, be.dp.n_chunks);
      const size_t want = (size_t)1 << 30;                                   // >= 1 GiB in rotation (4x the Infinity Cache)
      const int nrot = (int)std::min<size_t>(16, std::max<size_t>(3, (want + jb - 1) / jb));
      for (int r = 1; r < nrot; ++r) {
        double* pj = extra.device<double>(jb / sizeof(double));
        int32_t* ps = extra.device<int32_t>((size_t)be.hp.M);
        double* pf = extra.device<double>((size_t)be.hp.m);
        sets.push_back({pj, ps, pf});
      }
    }
    int turn = 0;
    auto launch = [&]() {
      switch (which) {
        case 0:
          if (be.robust()) { be.residual_sq(be.x_cur, be.f_cur, be.scal_dev + be.kCostSlot); break; }      // (the cost evaluation of a robust LM trial: + motion rows and the final sum)
          with_flag(be.hp.calib, [&](auto calib) { hipLaunchKernelGGL((k_observations<calib(), false>), g, b, 0, be.stream, be.dp, be.cams, be.x_cur, be.f_cur, be.J, be.rspan, be.pat0, 0); });
          break;
        case 1:
        case 5: {
          const OutSet& o = sets[turn];
          turn = (turn + 1) % (int)sets.size();
          const dim3 gj(xcd_grid(be.dp.n_chunks));
          with_flag(be.hp.calib, [&](auto calib) { hipLaunchKernelGGL((k_observations<calib(), true>), gj, b, 0, be.stream, be.dp, be.cams, be.x_cur, o.f, o.J, o.span, be.pat0, 0); });
          break;
        }
        case 2:
          with_flag(be.hp.calib, [&](auto calib) { hipLaunchKernelGGL(k_jv<calib() ? 30 : 21>, dim3(xcd_grid(be.dp.n_chunks)), b, 0, be.stream, be.dp, be.J, be.span, vn, ym); });
          break;
        case 3:
          be.jtu_local(um, zn);
          break;
        case 6:
          schur->assemble_local(be.f_cur, be.x_cur);       // Jacobian evaluated inside the assembly (the LM path)
          break;
        case 7:
          be.ensure_cams(be.x_cur);
          hipLaunchKernelGGL(k_landmark_cost, dim3(be.landmark_blocks()), b, 0, be.stream, be.dp, be.lm, (const CamState*)be.cams, be.partials, (double*)nullptr, (double*)nullptr);
          break;
        case 8:
          be.landmark_normal_equations(schur->ne, be.x_cur);      // (adds into the workspace over and over: the blocks there are no normal equations afterwards, and no call keeps them)
          break;
        default:
          schur->assemble_local(be.f_cur);
      }
    };
    if (be.dp.n_chunks == 0) { *avg_ms = 0; return MVUS_OK; }
    const double ms = time_on_stream(be.stream, (int)sets.size(), launches, launch);      // warm-up: every set touched once
    MVUS_HIP(hipGetLastError());
    *avg_ms = ms;
    if (which == 1 || which == 5) {            // the handle's own set holds J(x_cur) again (set 0 was written by one of the launches)
      be.has_jacobian = true;
    }
    return MVUS_OK;
  });
}
}  // extern "C"
