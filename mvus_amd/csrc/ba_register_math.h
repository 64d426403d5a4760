// Registering one camera against a held trajectory (mvus_ba_register_cameras, ba_register.hip.h): the small dense pieces of the batched
// Levenberg-Marquardt solver, written once for the device and for the host build that pins them (tests/register_hostcheck.cpp) -- the
// packed triangle of the 3 + P normal equations, the damped Cholesky solve, the projected trial point with its scalars, and the ONE
// function that decides on a trial (gain ratio, accept / reject, damping, termination).  Plain C++, no device intrinsics.
//
// A problem's unknowns are one camera's entries of x in the order of mvus_ba_set_frozen: alpha, beta, rs, then the P camera parameters
// (n = 3 + P <= 18).  The rules are lm_schur's (ba_schur.h) restated per problem; there is no trust region.
#pragma once
#include <cstdio>

#include "ba_math.h"

namespace mvus {

constexpr int kRegMaxN = 18;                                  // 3 + 15
constexpr int kRegMaxTri = kRegMaxN * (kRegMaxN + 1) / 2;     // 171
constexpr int kRegSlab = 128;                                 // detections per slab: a function of nothing, so a camera's partition depends on its count only
constexpr int kRegPartial = 192;                              // doubles per slab partial: triangle | g | twice the cost | visible
constexpr int kRegMaxBatch = 4096;
constexpr double kRegLambdaMax = 1e12;

// upper triangle packed by columns: entry (i, j), i <= j, independent of n
MVUS_HD int reg_tri(int n) { return n * (n + 1) / 2; }
MVUS_HD int reg_tri_index(int i, int j) { return i <= j ? j * (j + 1) / 2 + i : i * (i + 1) / 2 + j; }
MVUS_HD void reg_tri_entry(int e, int& i, int& j) {
  j = 0;
  while ((j + 1) * (j + 2) / 2 <= e) ++j;
  i = e - j * (j + 1) / 2;
}
MVUS_HD int reg_slabs(long long Mc) { return (int)((Mc + kRegSlab - 1) / kRegSlab); }

// One camera's CamState from its own 3 + P vector v = [alpha beta rs | camera parameters]: load_cam_state's work without the full x
// around it, for the host loop (the device decodes a batch with k_cam_states itself: ba_register.hip.h says why).
MVUS_HD void reg_load_cam_state(const double* v, bool calib, const double* Kfix4, const double* dfix5, double H, CamState& s) {
  s.alpha = v[0]; s.beta = v[1]; s.rs = v[2]; s.H = H;
  const double* q = v + 3;
  double rv[3];
  if (calib) {
    s.fx = q[0]; s.fy = q[1]; s.cx = q[2]; s.cy = q[3];
    rv[0] = q[4]; rv[1] = q[5]; rv[2] = q[6];
    s.t[0] = q[7]; s.t[1] = q[8]; s.t[2] = q[9];
    for (int k = 0; k < 5; ++k) s.d[k] = q[10 + k];
  } else {
    s.fx = Kfix4[0]; s.fy = Kfix4[1]; s.cx = Kfix4[2]; s.cy = Kfix4[3];
    rv[0] = q[0]; rv[1] = q[1]; rv[2] = q[2];
    s.t[0] = q[3]; s.t[1] = q[4]; s.t[2] = q[5];
    for (int k = 0; k < 5; ++k) s.d[k] = dfix5[k];
  }
  rodrigues(rv, s.R, s.W);
}

// Sink of eval_observation_to that keeps the N camera-side slots of the two rows and drops the twelve spline slots.
template <int N>
struct RegSink {
  static constexpr bool kFactored = false;
  double jx[N], jy[N];
  MVUS_HD void begin(int32_t) {}
  MVUS_HD void x(int k, double v) { if (k < N) jx[k] = v; }
  MVUS_HD void y(int k, double v) { if (k < N) jy[k] = v; }
};

// Held entries (bit k of `held`: the handle's frozen mask restricted to the camera) leave the system: g_k = 0, row and column k zero,
// H_kk = 1.  Switched-off groups have zero columns already and keep H_kk = 0.
MVUS_HD void reg_apply_held(int n, uint32_t held, double* Hp, double* g) {
  for (int j = 0; j < n; ++j)
    for (int i = 0; i <= j; ++i)
      if (((held >> i) | (held >> j)) & 1u) Hp[reg_tri_index(i, j)] = (i == j) ? 1.0 : 0.0;
  for (int k = 0; k < n; ++k) if ((held >> k) & 1u) g[k] = 0.0;
}

// D = diag(H), 1 where 0 (Marquardt scaling; HostSchur::damp_scale)
MVUS_HD double reg_damp_scale(double hii) { return hii > 0 ? hii : 1.0; }

// (H + lambda D) p = -g by Cholesky: Hp the packed upper triangle, L the factor's storage (reg_tri(n) doubles, U^T U = H + lambda D in
// the same packing).  Entries in the bit set `skip` are taken out for this solve as held ones are (row and column zero, H_kk = 1,
// g_k = 0: p_k = 0) -- an rs that sits on its bound with the gradient pushing outward.  Returns 0, or 1 on a pivot that is not positive
// (p is then not written).
MVUS_HD int reg_damped_solve(int n, const double* Hp, const double* g, double lambda, uint32_t skip, double* L, double* p) {
  for (int j = 0; j < n; ++j) {
    for (int i = 0; i <= j; ++i) {
      double s = Hp[reg_tri_index(i, j)];
      if (((skip >> i) | (skip >> j)) & 1u) s = (i == j) ? 1.0 : 0.0;
      if (i == j) s += lambda * reg_damp_scale(s);
      for (int k = 0; k < i; ++k) s -= L[reg_tri_index(k, i)] * L[reg_tri_index(k, j)];
      if (i == j) {
        if (!(s > 0)) return 1;
        L[reg_tri_index(j, j)] = sqrt(s);
      } else {
        L[reg_tri_index(i, j)] = s / L[reg_tri_index(i, i)];
      }
    }
  }
  for (int i = 0; i < n; ++i) {              // U^T y = -g
    double s = ((skip >> i) & 1u) ? 0.0 : -g[i];
    for (int k = 0; k < i; ++k) s -= L[reg_tri_index(k, i)] * p[k];
    p[i] = s / L[reg_tri_index(i, i)];
  }
  for (int i = n - 1; i >= 0; --i) {         // U p = y
    double s = p[i];
    for (int k = i + 1; k < n; ++k) s -= L[reg_tri_index(i, k)] * p[k];
    p[i] = s / L[reg_tri_index(i, i)];
  }
  return 0;
}

// The box: entry 2 (rs) in [0, 1] when `boxed` (rs_bounds, rs not held), nothing else.
MVUS_HD double reg_project(int k, bool boxed, double v) { return (boxed && k == 2) ? fmin(fmax(v, 0.0), 1.0) : v; }

// projected gradient norm (lm_gnorm_host): a component pushing against its active bound does not count
MVUS_HD double reg_gnorm(int n, const double* x, bool boxed, const double* g) {
  double gn = 0.0;
  for (int i = 0; i < n; ++i) {
    const bool blocked = boxed && i == 2 && ((x[i] <= 0.0 && g[i] > 0) || (x[i] >= 1.0 && g[i] < 0));
    if (!blocked) gn = fmax(gn, fabs(g[i]));
  }
  return gn;
}

// trial point x_new = P(x + p) and out = [g.step, step^T D step, |step|^2, |x|^2] (lm_trial_host); a non-finite p gives step 0 and
// out[0] = NaN
MVUS_HD void reg_trial(int n, const double* x, const double* p, bool boxed, const double* g, const double* Hp, double* x_new, double out[4]) {
  double gp = 0, pDp = 0, s2 = 0, x2 = 0;
  bool bad = false;
  for (int i = 0; i < n; ++i) bad = bad || !(fabs(p[i]) <= 1.7976931348623157e308);
  for (int i = 0; i < n; ++i) {
    const double xn = bad ? x[i] : reg_project(i, boxed, x[i] + p[i]);
    const double st = xn - x[i];
    x_new[i] = xn;
    gp += g[i] * st; pDp += st * reg_damp_scale(Hp[reg_tri_index(i, i)]) * st; s2 += st * st; x2 += x[i] * x[i];
  }
  out[0] = bad ? __builtin_nan("") : gp; out[1] = pDp; out[2] = s2; out[3] = x2;
}

// scipy's check_termination (ba_solver.h)
MVUS_HD int reg_check_termination(double dF, double F, double dx_norm, double x_norm, double ratio, double ftol, double xtol) {
  const bool f_ok = dF < ftol * F && ratio > 0.25;
  const bool x_ok = dx_norm < xtol * (xtol + x_norm);
  if (f_ok && x_ok) return 4;
  if (f_ok) return 2;
  if (x_ok) return 3;
  return -1;
}

struct RegOpts {
  int32_t max_nfev, pad;
  double ftol, xtol, gtol, lambda0, lambda_min, inlier_thres;
};

// What a problem carries from round to round.  status is meaningful once done != 0: -1 never started, 0 evaluation budget spent or the
// damping ran past 1e12, 1 - 4 scipy's.
struct RegState {
  double lambda, nu, cost, cost0;
  double trial[4];              // reg_trial's scalars of the trial in flight
  int32_t nfev, status, done, pad;
};

MVUS_HD void reg_state_init(RegState& s, const RegOpts& o) {
  s.lambda = fmax(o.lambda0 > 0 ? o.lambda0 : 1e-4, o.lambda_min);
  s.nu = 2.0; s.cost = 0.0; s.cost0 = 0.0;
  for (int k = 0; k < 4; ++k) s.trial[k] = 0.0;
  s.nfev = 0; s.status = 0; s.done = 0; s.pad = 0;
}

// The first evaluation: the cost at the start, and whether the problem starts at all (a finite cost, at least as many rows with a
// Jacobian -- two per visible detection -- as free unknowns).
MVUS_HD void reg_start(RegState& s, double cost, long long visible, int nfree) {
  s.nfev = 1; s.cost = cost; s.cost0 = cost;
  if (!(fabs(cost) <= 1.7976931348623157e308) || 2 * visible < (long long)nfree) { s.status = -1; s.done = 1; }
}

// a factorisation that failed (or a step that is not finite) at this damping: raise it, give up past 1e12
MVUS_HD void reg_solve_failed(RegState& s) {
  s.lambda *= 10.0;
  if (s.lambda > kRegLambdaMax) { s.status = 0; s.done = 1; }
}

// The trial in flight (s.trial) has been evaluated: cost_new.  Returns 1 when it is accepted (the caller moves x and adopts the
// linearisation of the trial point).  Counts the evaluation, updates the damping (Nielsen on a gain, x nu on none), and ends the problem
// on scipy's tests, on the budget, or on a damping past 1e12 after a non-finite cost.
MVUS_HD int reg_decide(RegState& s, const RegOpts& o, double cost_new) {
  int accept = 0;
  ++s.nfev;
  if (!(fabs(cost_new) <= 1.7976931348623157e308)) {
    s.lambda *= s.nu; s.nu *= 2.0;
    if (s.lambda > kRegLambdaMax) { s.status = 0; s.done = 1; }
  } else {
    const double predicted = 0.5 * (s.lambda * s.trial[1] - s.trial[0]);
    const double actual = s.cost - cost_new;
    const double ratio = predicted > 0 ? actual / predicted : (actual > 0 ? 1.0 : 0.0);
    const int term = reg_check_termination(actual, s.cost, sqrt(s.trial[2]), sqrt(s.trial[3]), ratio, o.ftol, o.xtol);
    if (actual > 0) {
      const double t = 2.0 * ratio - 1.0;
      s.lambda *= fmax(1.0 / 3.0, 1.0 - t * t * t);
      s.lambda = fmax(s.lambda, o.lambda_min);
      s.nu = 2.0;
      s.cost = cost_new;
      accept = 1;
    } else {
      s.lambda *= s.nu; s.nu *= 2.0;
    }
    if (term != -1) { s.status = term; s.done = 1; }
  }
  if (!s.done && s.nfev >= o.max_nfev) { s.status = 0; s.done = 1; }
  return accept;
}

// One round's small dense work for one problem, between two evaluations.  `lin`: the summed partial of the evaluation that has just run
// (triangle | g | twice the cost | visible) at xt -- the start in the first round, the trial in flight later.  Adopts it when it is the
// start or the trial is accepted (x <- xt, H, g <- lin with the held entries taken out), tests the projected gradient, and -- unless the
// problem has ended or `last` -- solves at the damping in force (raising it while the factorisation fails) and leaves the next trial
// point in xt with its scalars in s.trial.  L, p: work space (reg_tri(n), n).
MVUS_HD void reg_round(int n, bool first, bool last, const RegOpts& o, uint32_t held, bool boxed, int nfree, const double* lin,
                       RegState& s, double* x, double* xt, double* Hp, double* g, double* L, double* p) {
  if (!first && s.done) return;
  const int nt = reg_tri(n);
  const double cost_new = 0.5 * lin[nt + n];
  int adopt;
  if (first) { reg_state_init(s, o); reg_start(s, cost_new, (long long)lin[nt + n + 1], nfree); adopt = 1; }
  else adopt = reg_decide(s, o, cost_new);
  if (adopt) {
    for (int k = 0; k < n; ++k) { x[k] = xt[k]; g[k] = lin[nt + k]; }
    for (int e = 0; e < nt; ++e) Hp[e] = lin[e];
    reg_apply_held(n, held, Hp, g);
  }
  if (s.done) return;
  if (reg_gnorm(n, x, boxed, g) < o.gtol) { s.status = 1; s.done = 1; return; }
  if (s.nfev >= o.max_nfev) { s.status = 0; s.done = 1; return; }
  if (last) return;
  // an rs on its bound whose gradient pushes outward stays there: the step is that of the other unknowns alone (with rs in the system
  // the projection would cut its part of the step off and leave the others a step that assumed it)
  const uint32_t skip = (boxed && ((x[2] <= 0.0 && g[2] > 0) || (x[2] >= 1.0 && g[2] < 0))) ? 4u : 0u;
  while (!s.done) {
    if (reg_damped_solve(n, Hp, g, s.lambda, skip, L, p) == 0) {
      reg_trial(n, x, p, boxed, g, Hp, xt, s.trial);
      if (fabs(s.trial[0]) <= 1.7976931348623157e308 && fabs(s.trial[1]) <= 1.7976931348623157e308) break;
    }
    reg_solve_failed(s);
  }
}

// Arguments of mvus_ba_register_cameras / mvus_ba_register_linearize that can be refused without a device.  Returns 0 and leaves msg
// alone, or 1 with the reason in msg.  reg_check_scalars needs no handle; reg_check_batch needs C and P.
inline int reg_check_scalars(const char* who, int32_t B, int32_t max_nfev, double ftol, double xtol, double gtol, char* msg, size_t len) {
  if (B < 0) { std::snprintf(msg, len, "%s: B = %d is negative", who, (int)B); return 1; }
  if (B > kRegMaxBatch) { std::snprintf(msg, len, "%s: B = %d is more than %d problems in one call", who, (int)B, kRegMaxBatch); return 1; }
  if (max_nfev < 1) { std::snprintf(msg, len, "%s: max_nfev = %d, at least 1 is needed", who, (int)max_nfev); return 1; }
  if (!(ftol >= 0)) { std::snprintf(msg, len, "%s: ftol is negative or NaN", who); return 1; }
  if (!(xtol >= 0)) { std::snprintf(msg, len, "%s: xtol is negative or NaN", who); return 1; }
  if (!(gtol >= 0)) { std::snprintf(msg, len, "%s: gtol is negative or NaN", who); return 1; }
  return 0;
}
inline int reg_check_batch(const char* who, int C, int P, int32_t B, const int32_t* cam, const double* start, char* msg, size_t len) {
  if (B > 0 && cam == nullptr) { std::snprintf(msg, len, "%s: cam is NULL", who); return 1; }
  for (int32_t b = 0; b < B; ++b)
    if (cam[b] < 0 || cam[b] >= C) { std::snprintf(msg, len, "%s: cam[%d] = %d is not a camera of the handle (0 .. %d)", who, (int)b, (int)cam[b], C - 1); return 1; }
  if (start != nullptr)
    for (long long k = 0; k < (long long)B * (3 + P); ++k)
      if (!(fabs(start[k]) <= 1.7976931348623157e308)) { std::snprintf(msg, len, "%s: start[%lld] is not finite", who, k); return 1; }
  return 0;
}

}  // namespace mvus
