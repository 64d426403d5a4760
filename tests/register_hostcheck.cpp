// TEST-ONLY host build of the camera registration solver (mvus_amd/csrc/ba_register_math.h): the damped Cholesky solve, the decision on
// a trial and the argument checks as the kernels and the C ABI call them, plus a plain C++ loop that runs the whole registration of ONE
// problem on the host -- the rows from ba_math.h (eval_observation_to with the same sink), the rounds from reg_round -- so that
// tests/test_register_host.py can pin the arithmetic without a GPU and tests/test_gpu_register.py can hold the device loop against it.
#include <cstring>
#include <vector>

#include "../mvus_amd/csrc/ba_register_math.h"

using namespace mvus;

namespace {

// one camera's problem, as the library holds it on the device
struct HostReg {
  int calib, undist, rs_free, sync_free, rs_bounds, P;
  long long M;
  const double *frame, *u_raw, *v_raw;
  double H;
  const double *K4, *d5;
  SplineView sp;
  const double* x;            // the full parameter vector: the control points are read from it
  LossSpec loss;
  uint32_t held;
  std::vector<double> u_obs, v_obs;
};

void undistort_fixed(HostReg& r) {      // k_undistort_fixed / the plain copy of HipBackend::init
  r.u_obs.assign(r.u_raw, r.u_raw + r.M); r.v_obs.assign(r.v_raw, r.v_raw + r.M);
  if (r.calib || !r.undist) return;
  for (long long i = 0; i < r.M; ++i) {
    double xn, yn;
    undistort5<false>((r.u_raw[i] - r.K4[2]) / r.K4[0], (r.v_raw[i] - r.K4[3]) / r.K4[1], r.d5, xn, yn, nullptr, nullptr);
    r.u_obs[i] = r.K4[0] * xn + r.K4[2]; r.v_obs[i] = r.K4[1] * yn + r.K4[3];
  }
}

// the evaluation at v: lin = triangle | g | twice the cost | visible, rows added in detection order (x row, then y row); rows_out (may
// be NULL): the 2 M scaled rows [n + 1] for the caller
template <bool CALIB>
void linearize(const HostReg& r, const double* v, double* lin, double* rows_out, long long* inliers, double thres) {
  constexpr int N = 3 + (CALIB ? 15 : 6), NT = N * (N + 1) / 2;
  CamState cam;
  reg_load_cam_state(v, CALIB, r.K4, r.d5, r.H, cam);
  for (int e = 0; e < NT + N + 2; ++e) lin[e] = 0.0;
  if (inliers) *inliers = 0;
  for (long long i = 0; i < r.M; ++i) {
    RegSink<N> sink;
    for (int k = 0; k < N; ++k) { sink.jx[k] = 0.0; sink.jy[k] = 0.0; }
    const double uo = CALIB ? 0.0 : r.u_obs[i], vo = CALIB ? 0.0 : r.v_obs[i], ur = CALIB ? r.u_raw[i] : 0.0;
    const ObsResult o = eval_observation_to<CALIB, true>(cam, r.sp, r.x, r.undist != 0, r.rs_free != 0, r.sync_free != 0, r.frame[i], ur, r.v_raw[i], uo, vo, sink);
    double row[2][N + 1];
    double fx = o.ex, fy = o.ey, sx = 1.0, sy = 1.0;
    if (o.ctrl >= 0) {
      lin[NT + N + 1] += 1.0;
      if (inliers && thres > 0 && std::sqrt(o.ex * o.ex + o.ey * o.ey) < thres) ++*inliers;
      if (r.loss.kind != 0) {
        lin[NT + N] += loss_rho(r.loss, o.ex) + loss_rho(r.loss, o.ey);
        sx = loss_scale_row(r.loss, fx); sy = loss_scale_row(r.loss, fy);
      } else lin[NT + N] += o.ex * o.ex + o.ey * o.ey;
    }
    for (int k = 0; k < N; ++k) { row[0][k] = sx * sink.jx[k]; row[1][k] = sy * sink.jy[k]; }
    row[0][N] = fx; row[1][N] = fy;
    for (int q = 0; q < 2; ++q) {
      for (int j = 0; j < N; ++j) {
        for (int a = 0; a <= j; ++a) lin[reg_tri_index(a, j)] += row[q][a] * row[q][j];
        lin[NT + j] += row[q][j] * row[q][N];
      }
      if (rows_out) std::memcpy(rows_out + (2 * i + q) * (N + 1), row[q], sizeof(double) * (N + 1));
    }
  }
}

void linearize_any(const HostReg& r, const double* v, double* lin, double* rows_out, long long* inliers, double thres) {
  if (r.calib) linearize<true>(r, v, lin, rows_out, inliers, thres);
  else linearize<false>(r, v, lin, rows_out, inliers, thres);
}

HostReg make(const int32_t* flags, long long M, const double* frame, const double* u_raw, const double* v_raw, double H, const double* K4,
             const double* d5, int S, const double* interval, const int32_t* knot_off, const int32_t* ctrl_off, const int32_t* xoff,
             const double* knots, const double* x, int loss_kind, double f_scale, uint32_t held) {
  HostReg r{};
  r.calib = flags[0]; r.undist = flags[1]; r.rs_free = flags[2]; r.sync_free = flags[3]; r.rs_bounds = flags[4];
  r.P = r.calib ? 15 : 6;
  r.M = M; r.frame = frame; r.u_raw = u_raw; r.v_raw = v_raw; r.H = H; r.K4 = K4; r.d5 = d5;
  r.sp = SplineView{};
  r.sp.S = S; r.sp.istart = interval; r.sp.iend = interval + S; r.sp.knots = knots; r.sp.knot_off = knot_off; r.sp.ctrl_off = ctrl_off; r.sp.xoff = xoff;
  r.x = x; r.loss = LossSpec{loss_kind, f_scale}; r.held = held;
  undistort_fixed(r);
  return r;
}

}  // namespace

extern "C" {

int regcheck_tri_index(int i, int j) { return reg_tri_index(i, j); }
void regcheck_tri_entry(int e, int* i, int* j) { reg_tri_entry(e, *i, *j); }

// (H + lambda D) p = -g with H full symmetric [n * n]; returns reg_damped_solve's code (p untouched on failure)
int regcheck_solve(int n, const double* H, const double* g, double lambda, double* p) {
  double Hp[kRegMaxTri], L[kRegMaxTri];
  for (int j = 0; j < n; ++j) for (int i = 0; i <= j; ++i) Hp[reg_tri_index(i, j)] = H[i * n + j];
  return reg_damped_solve(n, Hp, g, lambda, 0u, L, p);
}

// reg_decide on a state given field by field: dstate = [lambda, nu, cost, trial(4)], istate = [nfev, status, done];
// dopts = [ftol, xtol, gtol, lambda0, lambda_min].  Returns the accept flag.
int regcheck_decide(double* dstate, int32_t* istate, int32_t max_nfev, const double* dopts, double cost_new) {
  RegState s{};
  s.lambda = dstate[0]; s.nu = dstate[1]; s.cost = dstate[2];
  for (int k = 0; k < 4; ++k) s.trial[k] = dstate[3 + k];
  s.nfev = istate[0]; s.status = istate[1]; s.done = istate[2];
  const RegOpts o{max_nfev, 0, dopts[0], dopts[1], dopts[2], dopts[3], dopts[4], 0.0};
  const int accept = reg_decide(s, o, cost_new);
  dstate[0] = s.lambda; dstate[1] = s.nu; dstate[2] = s.cost;
  istate[0] = s.nfev; istate[1] = s.status; istate[2] = s.done;
  return accept;
}

// reg_round on a state given field by field: dstate = [lambda, nu, cost, cost0, trial(4)], istate = [nfev, status, done];
// dopts = [ftol, xtol, gtol, lambda0, lambda_min]; lin = packed triangle | g | twice the cost | visible of the evaluation that has just
// run; x, xt [n], Hp [reg_tri(n)] packed, g [n] in and out.
void regcheck_round(int n, int first, int last, int32_t max_nfev, const double* dopts, uint32_t held, int boxed, int nfree, const double* lin,
                    double* dstate, int32_t* istate, double* x, double* xt, double* Hp, double* g) {
  RegState s{};
  s.lambda = dstate[0]; s.nu = dstate[1]; s.cost = dstate[2]; s.cost0 = dstate[3];
  for (int k = 0; k < 4; ++k) s.trial[k] = dstate[4 + k];
  s.nfev = istate[0]; s.status = istate[1]; s.done = istate[2];
  const RegOpts o{max_nfev, 0, dopts[0], dopts[1], dopts[2], dopts[3], dopts[4], 0.0};
  double L[kRegMaxTri], p[kRegMaxN];
  reg_round(n, first != 0, last != 0, o, held, boxed != 0, nfree, lin, s, x, xt, Hp, g, L, p);
  dstate[0] = s.lambda; dstate[1] = s.nu; dstate[2] = s.cost; dstate[3] = s.cost0;
  for (int k = 0; k < 4; ++k) dstate[4 + k] = s.trial[k];
  istate[0] = s.nfev; istate[1] = s.status; istate[2] = s.done;
}

// the argument checks of the two entry points (C, P of the handle); msg[160]
int regcheck_args(int C, int P, int32_t B, const int32_t* cam, const double* start, int32_t max_nfev, double ftol, double xtol, double gtol, char* msg) {
  if (reg_check_scalars("register_cameras", B, max_nfev, ftol, xtol, gtol, msg, 160)) return 1;
  return reg_check_batch("register_cameras", C, P, B, cam, start, msg, 160);
}

// the first evaluation of one problem at v[3 + P]: H full symmetric with the held entries taken out, g, cost, visible; rows_out (may be
// NULL) the 2 M scaled rows [3 + P + 1], residual last
void regcheck_linearize(const int32_t* flags, long long M, const double* frame, const double* u_raw, const double* v_raw, double H, const double* K4,
                        const double* d5, int S, const double* interval, const int32_t* knot_off, const int32_t* ctrl_off, const int32_t* xoff,
                        const double* knots, const double* x, int loss_kind, double f_scale, uint32_t held, const double* v,
                        double* H_out, double* g_out, double* cost_out, long long* visible_out, double* rows_out) {
  const HostReg r = make(flags, M, frame, u_raw, v_raw, H, K4, d5, S, interval, knot_off, ctrl_off, xoff, knots, x, loss_kind, f_scale, held);
  const int n = 3 + r.P, nt = reg_tri(n);
  double lin[kRegPartial];
  linearize_any(r, v, lin, rows_out, nullptr, 0.0);
  reg_apply_held(n, held, lin, lin + nt);
  for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) H_out[i * n + j] = lin[reg_tri_index(i, j)];
  for (int k = 0; k < n; ++k) g_out[k] = lin[nt + k];
  *cost_out = 0.5 * lin[nt + n];
  *visible_out = (long long)lin[nt + n + 1];
}

// the whole registration of one problem: the device's schedule, one round after another.  dopts = [ftol, xtol, gtol, lambda0, lambda_min,
// inlier_thres]; iout = [nfev, status]; dout = [cost, cost0]; cout = [visible, inliers].  tau_range[2] (may be NULL): the smallest and
// largest time stamp of a detection over every point evaluated.
void regcheck_solve_problem(const int32_t* flags, long long M, const double* frame, const double* u_raw, const double* v_raw, double H, const double* K4,
                            const double* d5, int S, const double* interval, const int32_t* knot_off, const int32_t* ctrl_off, const int32_t* xoff,
                            const double* knots, const double* x, int loss_kind, double f_scale, uint32_t held, const double* start,
                            int32_t max_nfev, const double* dopts, double* v_out, double* dout, int32_t* iout, long long* cout, double* tau_range) {
  const HostReg r = make(flags, M, frame, u_raw, v_raw, H, K4, d5, S, interval, knot_off, ctrl_off, xoff, knots, x, loss_kind, f_scale, held);
  const int n = 3 + r.P;
  const RegOpts o{max_nfev, 0, dopts[0], dopts[1], dopts[2], dopts[3], dopts[4] >= 0 ? dopts[4] : 0.0, dopts[5]};
  const bool boxed = r.rs_bounds && !((held >> 2) & 1u);
  int nfree = 0;
  for (int k = 0; k < n; ++k) {
    const bool off = (k < 2 && !r.sync_free) || (k == 2 && !r.rs_free);
    if (!((held >> k) & 1u) && !off) ++nfree;
  }
  double xc[kRegMaxN], xt[kRegMaxN], Hp[kRegMaxTri], g[kRegMaxN], L[kRegMaxTri], p[kRegMaxN], lin[kRegPartial];
  for (int k = 0; k < n; ++k) { xc[k] = start[k]; xt[k] = start[k]; g[k] = 0.0; }
  for (int e = 0; e < kRegMaxTri; ++e) Hp[e] = 0.0;
  RegState s{};
  auto track = [&](const double* v) {
    if (!tau_range) return;
    for (long long i = 0; i < M; ++i) {
      const double tau = v[0] * (frame[i] + v[2] * v_raw[i] / H) + v[1];
      if (tau < tau_range[0]) tau_range[0] = tau;
      if (tau > tau_range[1]) tau_range[1] = tau;
    }
  };
  linearize_any(r, xt, lin, nullptr, nullptr, 0.0); track(xt);
  for (int k = 1; k < max_nfev; ++k) {
    reg_round(n, k == 1, false, o, held, boxed, nfree, lin, s, xc, xt, Hp, g, L, p);
    if (!s.done) { linearize_any(r, xt, lin, nullptr, nullptr, 0.0); track(xt); }
  }
  reg_round(n, max_nfev == 1, true, o, held, boxed, nfree, lin, s, xc, xt, Hp, g, L, p);
  long long inl = 0;
  linearize_any(r, xc, lin, nullptr, &inl, o.inlier_thres);
  for (int k = 0; k < n; ++k) v_out[k] = xc[k];
  dout[0] = s.cost; dout[1] = s.cost0;
  iout[0] = s.nfev; iout[1] = s.status;
  cout[0] = (long long)lin[reg_tri(n) + n + 1]; cout[1] = inl;
}

}  // extern "C"
