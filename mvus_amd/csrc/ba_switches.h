// Every runtime switch (environment variable) of the bundle-adjustment unit, in one table.  Plain C++17, no HIP: the host build of
// tests/hostcheck includes it (tests/test_switches_host.py checks the defaults, the parsing, and that no other file of the unit reads
// the environment).  HipBackend::init reads the table once per handle, HipSchur's constructor once per workspace (so again after
// remove_outliers, set_time_shard or a failed solve rebuilt it); nothing is read per solve, per trial or per fetch, except the two
// switches marked PER RUN below.  Set a switch before the handle it addresses is created.
// Not in the table: MVUS_ROCTX (api_common.h), the spline unit's own reads (spline_api.hip, spline_fit.hip.h), MVUS_LIB_PATH (Python).
#pragma once
#include <algorithm>
#include <cstdlib>
#include <cstring>

namespace mvus {

struct Switches {
  // ---- the backend (ba_api.hip) ----
  // MVUS_LM_NO_CARRY (set): a solve does not take over f(x), the cost and the normal equations the solve before it left on the device.
  // Default off.  test_gpu_schur.py (speculation and carry against the sequential driver).
  bool lm_no_carry = false;
  // MVUS_FETCH_EVENT (set): the fetch in front of a speculative linearisation waits behind an event instead of polling the start mark
  // in mapped memory.  Default off.  test_gpu_schur.py clears it; A/B by hand.
  bool fetch_event = false;
  // MVUS_NO_SPEC_SHARDS (set): no speculative linearisation on time shards.  Default off.  test_gpu_dist.py.
  bool no_spec_shards = false;
  // MVUS_SQ_DEVICE_SUM (set): |f|^2 finished by k_dot_final instead of the host-side sum of the partials.  Default off.  test_gpu_schur.py.
  bool sq_device_sum = false;
  // MVUS_LSMR_HOST (set): the host-driven LSMR loop instead of the device-resident one.  Default off.  test_gpu_lsmr.py (the two loops
  // bit for bit, through mvus_ba_lsmr).
  bool lsmr_host = false;
  // MVUS_LSMR_BOUNDED_HOST (set): the bounded problem's LSMR on the host-driven loop.  Default off.  test_gpu_parity.py, test_gpu_lsmr.py.
  bool lsmr_bounded_host = false;
  // MVUS_LSMR_ONE_PASS (set): one pass over J per LSMR iteration (k_jvjtu).  Default off.  PER RUN: bench.py sets and clears it on a
  // live handle, so the backend asks lsmr_one_pass_now() at every LSMR run; this field is the value when the table was read.
  // test_gpu_lsmr.py (against a longdouble LSMR at every branch of k_jvjtu), test_gpu_parity.py, bench.py.
  bool lsmr_one_pass = false;
  // MVUS_LSMR_TRACE (set): Lsmr::run prints its scalars every iteration.  Default off.  PER RUN (lsmr_trace_now(): ba_solver.h has no
  // handle to keep a table on).  Debugging by hand.
  bool lsmr_trace = false;

  // ---- HipSchur (ba_schur_host.hip.h) ----
  // MVUS_GEMM_SLABS=k (k > 0): K-slabs of the Schur product.  Default 0 = the cost model of plan_gemm.  test_gpu_schur.py,
  // test_gpu_schur_backward_error.py.
  int gemm_slabs = 0;
  // MVUS_RCS=gj: the reduced camera system by the block Gauss-Jordan (k_schur_finish, k_gj_step) instead of the blocked L D L^T.
  // Default off.  test_gpu_rcs.py, test_gpu_schur_backward_error.py.
  bool rcs_gj = false;
  // MVUS_RCS_TRSM=launch: the rows below a super-block in a launch of their own (k_rcs_trsm) instead of inside k_rcs_factor.
  // Default off.  test_gpu_rcs.py, test_gpu_schur_backward_error.py.
  bool rcs_trsm_launch = false;
  // MVUS_RCS_SPIN_LIMIT=n: polls before a waiting workgroup of k_rcs_factor / k_sep_bcr_levels gives up; 0 = the first poll that finds
  // the flag behind.  Default -1 = unset (kRcsSpinLimit).  Test hook: test_gpu_rcs.py, test_gpu_schur.py.
  long long rcs_spin_limit = -1;
  // MVUS_BCR_FUSED=0: a launch per wide cyclic-reduction level instead of one for all (k_sep_bcr_levels).  Default on.  test_gpu_schur.py,
  // test_gpu_schur_backward_error.py.
  bool bcr_fused = true;
  // MVUS_PART_LEN=n: control points per interior of the band solver.  Clamped to [two separators, kPartL].  Default 0 = unset (kPartL, half
  // of it up to 128 camera unknowns).
  // test_gpu_rcs.py, test_gpu_schur_backward_error.py (16, 32, and 6 = the longest separator chain a spline can have).
  int part_len = 0;
  // MVUS_PART_BACK (set): the interiors' columns are back-corrected (k_part_back) and the Schur product carries no correction rows.
  // Default off.  test_gpu_rcs.py, test_gpu_schur_backward_error.py.
  bool part_back = false;
  // MVUS_DIRECT_RHS=0: the right-hand-side copy Z = E is made instead of the interior solves reading the assembled blocks.
  // Default on.  test_gpu_rcs.py, test_gpu_schur_backward_error.py.
  bool direct_rhs = true;
  // MVUS_SEP_SEQUENTIAL (set): the sequential block-tridiagonal separator kernels instead of the cyclic reduction.  Default off.
  // test_gpu_schur.py, test_gpu_schur_backward_error.py.
  bool sep_sequential = false;
  // MVUS_SEP_TWO_LEVEL=0: time shards sum the whole separator system instead of the cut separators only.  Default on.  test_gpu_dist.py.
  bool sep_two_level = true;
  // MVUS_ASM_ATOMIC (set): the detection-major assembly (fp64 atomics) instead of the window-major one.  Default off.
  // test_gpu_det_assembly.py, test_gpu_robust_loss.py.
  bool asm_atomic = false;
  // MVUS_WIN=w (w > 0): control points per window of the window-major assembly.  Default 0 = the cost model of win_prepare.
  // test_gpu_det_assembly.py, test_gpu_robust_loss.py, tools/micro/time_win.py.
  int win = 0;
  // MVUS_WIN_GROUPS=g (g > 0): camera groups per window.  Default 0 = the cost model.  tools/micro/win_group_sweep.sh.
  int win_groups = 0;
  // MVUS_NO_SPEC (set): no speculative linearisation at the trial point.  Default off.  test_gpu_schur.py.
  bool no_spec = false;
  // MVUS_LM_MATERIALIZE_J (set): the LM path materialises the analytic Jacobian instead of fusing it into the assembly.  Default off.
  // A/B by hand.
  bool lm_materialize_j = false;
  // MVUS_NE_FROM_J (set): the normal equations of a held analytic Jacobian are formed from the stored blocks (detection-major kernel).
  // Default off.  test_gpu_det_assembly.py, test_gpu_frozen.py, test_gpu_jacobian_exact.py, test_gpu_robust_loss.py.
  bool ne_from_j = false;
  // MVUS_NO_OVERLAP (set): the interiors are not factorised beside the right-hand-side copies (k_build_rhs + k_part_cholesky).
  // Default off.  test_gpu_schur_backward_error.py.
  bool no_overlap = false;
  // MVUS_DEBUG (set): one line on stderr for the window plan, a failed solve and a hand-over time-out.  Default off.
  // test_gpu_rcs.py, test_gpu_schur.py (they count the time-out lines).
  bool debug = false;
};

namespace env {
inline bool is_set(const char* name) { return std::getenv(name) != nullptr; }
inline bool equals(const char* name, const char* value) { const char* e = std::getenv(name); return e && std::strcmp(e, value) == 0; }
inline bool flag(const char* name, bool unset) { const char* e = std::getenv(name); return e ? std::atoi(e) != 0 : unset; }      // "0" = off, any other number = on
inline int positive(const char* name) { const char* e = std::getenv(name); return e ? std::max(0, std::atoi(e)) : 0; }           // 0 = unset or not positive
}  // namespace env

inline bool lsmr_one_pass_now() { return env::is_set("MVUS_LSMR_ONE_PASS"); }
inline bool lsmr_trace_now() { return env::is_set("MVUS_LSMR_TRACE"); }

inline Switches read_switches() {
  Switches s;
  s.lm_no_carry = env::is_set("MVUS_LM_NO_CARRY");
  s.fetch_event = env::is_set("MVUS_FETCH_EVENT");
  s.no_spec_shards = env::is_set("MVUS_NO_SPEC_SHARDS");
  s.sq_device_sum = env::is_set("MVUS_SQ_DEVICE_SUM");
  s.lsmr_host = env::is_set("MVUS_LSMR_HOST");
  s.lsmr_bounded_host = env::is_set("MVUS_LSMR_BOUNDED_HOST");
  s.lsmr_one_pass = lsmr_one_pass_now();
  s.lsmr_trace = lsmr_trace_now();
  s.gemm_slabs = env::positive("MVUS_GEMM_SLABS");
  s.rcs_gj = env::equals("MVUS_RCS", "gj");
  s.rcs_trsm_launch = env::equals("MVUS_RCS_TRSM", "launch");
  if (const char* e = std::getenv("MVUS_RCS_SPIN_LIMIT")) s.rcs_spin_limit = (long long)(unsigned)std::strtoul(e, nullptr, 10);
  s.bcr_fused = env::flag("MVUS_BCR_FUSED", true);
  if (const char* e = std::getenv("MVUS_PART_LEN")) s.part_len = std::max(1, std::atoi(e));      // (the partition raises it to its shortest interior)
  s.part_back = env::is_set("MVUS_PART_BACK");
  s.direct_rhs = env::flag("MVUS_DIRECT_RHS", true);
  s.sep_sequential = env::is_set("MVUS_SEP_SEQUENTIAL");
  s.sep_two_level = env::flag("MVUS_SEP_TWO_LEVEL", true);
  s.asm_atomic = env::is_set("MVUS_ASM_ATOMIC");
  s.win = env::positive("MVUS_WIN");
  s.win_groups = env::positive("MVUS_WIN_GROUPS");
  s.no_spec = env::is_set("MVUS_NO_SPEC");
  s.lm_materialize_j = env::is_set("MVUS_LM_MATERIALIZE_J");
  s.ne_from_j = env::is_set("MVUS_NE_FROM_J");
  s.no_overlap = env::is_set("MVUS_NO_OVERLAP");
  s.debug = env::is_set("MVUS_DEBUG");
  return s;
}

}  // namespace mvus
