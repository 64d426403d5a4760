/* mvus_ba.h -- C ABI of libmvusba.so, the MI355X (gfx950) bundle-adjustment core.
 *
 * The reference (CenekAlbl/mvus) has no FFI on this path: the boundary is the Python call
 *
 *     res = least_squares(fn, model, jac_sparsity=A, tr_solver='lsmr', xtol=1e-12,
 *                         max_nfev=max_iter, verbose=0, bounds=bounds_rs)
 *                                   (multiviewunsynch/reconstruction/common.py:670)
 *
 * inside Scene.BA (common.py:441-697) with fn = error_BA (common.py:448-487) and A = jac_BA()
 * (common.py:490-610), plus Scene.remove_outliers (common.py:700-717).  The entry points below are
 * what a ctypes binding placed at that call site needs; each one cites the reference code it
 * replaces.  INTEGRATION.md shows the binding.
 *
 * Conventions
 *   - every function returns 0 on success or a negative MVUS_E_* code; nothing throws across the ABI;
 *     mvus_last_error() gives the message of the last failure on the handle (or, with NULL, of the
 *     last failed mvus_ba_create on this thread);
 *   - all `const double*` / `double*` arguments are HOST pointers unless the name ends in `_dev`;
 *     the caller owns every buffer it passes; the handle owns all device memory;
 *   - the parameter vector x has the reference layout (common.py:615-650):
 *       [alpha(C) beta(C) rs(C) cam_0(P) .. cam_{C-1}(P) spline_0: cx(n_0) cy(n_0) cz(n_0) spline_1 ..]
 *     P = 6 (rvec,t) or 15 (fx,fy,cx,cy,rvec,t,k1,k2,p1,p2,k3) when opt_calib (common.py:1113-1124);
 *   - the residual vector f has the reference row order (common.py:476-485): per camera
 *     [|ex|(M_c) |ey|(M_c)], then the motion-regulariser rows (T);
 *   - one handle per (host thread, GPU, stream); calls on one handle must not overlap.
 *   - there is NO CPU fallback: without a HIP device mvus_ba_create fails with MVUS_E_HIP.
 */
#ifndef MVUS_BA_H
#define MVUS_BA_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MVUS_OK 0
#define MVUS_E_INVALID (-1)  /* bad argument / inconsistent problem description */
#define MVUS_E_HIP (-2)      /* HIP runtime error (no device, allocation, launch) */
#define MVUS_E_NUMERIC (-3)  /* non-finite residuals at x0, x0 outside bounds (scipy raises ValueError) */
#define MVUS_E_COMM (-4)     /* the all-reduce callback reported a failure */
#define MVUS_E_UNSUPPORTED (-5)  /* the problem is outside what this solver handles (MVUS_SOLVER_LM_SCHUR: motion rows that couple control
                                 * points more than 16 apart, or more than 6 apart on a time shard): the other solver has no such limit */

#define MVUS_E_RESHARD (-6)  /* time shard (mvus_ba_set_time_shard): at the point the solver has reached, a detection or motion row touches
                              * control points outside this rank's slice +- halo (the time stamps drifted since the cuts were made).
                              * mvus_ba_solve then RETURNS that point in x (and nfev / cost so far in res): the caller re-cuts there
                              * and continues (mvus_amd.dist.solve_time_sharded).  Raised on every rank of the job together.
                              * The reference re-evaluates visibility at every call: common.py:317, tools/util.py:90-116 */

#define MVUS_MOTION_F 0  /* constant-force prior       common.py:984-998 */
#define MVUS_MOTION_KE 1 /* constant-kinetic-energy    common.py:976-981 */

/* Jacobian used by mvus_ba_solve */
#define MVUS_JAC_ANALYTIC 0 /* full analytic block-sparse Jacobian */
#define MVUS_JAC_PATTERN 1  /* analytic, masked to the reference sparsity pattern jac_BA builds at x0
                               (3 nearest knots per row, common.py:559-563,573-585) */
#define MVUS_JAC_FD 2       /* scipy's own estimate: sparse 2-point forward differences over that pattern, columns
                               perturbed group-wise (scipy/optimize/_numdiff.py:628-700), one residual launch per
                               group.  Needs mvus_ba_set_fd_groups. */

/* Solver used by mvus_ba_solve */
#define MVUS_SOLVER_TRF_LSMR 0 /* restatement of scipy trf + lsmr (the reference's optimiser), J kept as operator */
#define MVUS_SOLVER_LM_SCHUR 1 /* Levenberg-Marquardt on device-assembled normal equations: spline block eliminated
                                  by a partitioned band Cholesky + cyclic reduction, Schur complement on the fp64
                                  matrix cores, reduced camera system by block Gauss-Jordan; all vectors stay on the
                                  device, one 7-scalar read-back per iteration.  The damping (and its growth factor)
                                  is carried from one mvus_ba_solve on a handle to the next. */

typedef struct mvus_ba mvus_ba; /* opaque */

/* The Scene state Scene.BA closes over (common.py:441-697), cameras in sequence[:numCam] order. */
typedef struct mvus_problem {
  int32_t num_cam;       /* C = numCam */
  int32_t opt_calib;     /* settings['opt_calib']      common.py:621 */
  int32_t undist_points; /* settings['undist_points']  common.py:126 */
  int32_t rs_free;       /* `rs` argument of Scene.BA: rolling-shutter column in the pattern, common.py:518 */
  int32_t rs_bounds;     /* `rs_bounds`: 0 <= rs <= 1   common.py:655-662 */
  int32_t motion_reg;    /* `motion_reg`                common.py:483-485 */
  int32_t motion_type;   /* MVUS_MOTION_*  settings['motion_type'] common.py:416-420 */
  int32_t opt_sync;      /* settings['opt_sync'] (absent = 1): 0 freezes alpha and beta -- their columns leave the
                            pattern and every Jacobian, common.py:512-515 */
  double motion_weight;  /* `motion_weights`            common.py:413 */
  const int64_t* det_offsets; /* [C+1] detections of camera c are [det_offsets[c], det_offsets[c+1]) */
  const double* frame;        /* [M] detections[c][0]  (np.loadtxt usecols=(2,0,1), common.py:1190) */
  const double* u_raw;        /* [M] detections[c][1] */
  const double* v_raw;        /* [M] detections[c][2] */
  const double* img_height;   /* [C] cameras[c].resolution[1]  common.py:125 */
  const double* K;            /* [C*4] fx fy cx cy, used when !opt_calib */
  const double* dist;         /* [C*5] k1 k2 p1 p2 k3, used when !opt_calib */
  int32_t num_splines;        /* S = spline['int'].shape[1] */
  const double* interval;     /* [2*S] row-major spline['int']: S starts then S ends */
  const int64_t* knot_offsets; /* [S+1] */
  const double* knots;        /* concatenated spline['tck'][s][0] */
  int32_t device;             /* HIP device ordinal */
  void* stream;               /* hipStream_t to run on, or NULL for a stream owned by the handle */
} mvus_problem;

typedef struct mvus_solve_opts {
  int32_t solver;    /* MVUS_SOLVER_* */
  int32_t jac_mode;  /* MVUS_JAC_* */
  int32_t max_nfev;  /* max_iter of Scene.BA (10)           common.py:441,670 */
  double ftol;       /* 1e-8  scipy default                  */
  double xtol;       /* 1e-12 as passed at common.py:670     */
  double gtol;       /* 1e-8  scipy default                  */
  double lsmr_atol;  /* 1e-6  scipy lsmr default             */
  double lsmr_btol;  /* 1e-6                                 */
  double lsmr_conlim; /* 1e8                                 */
  int32_t lsmr_maxiter; /* 0 -> min(m, n)                    */
  int32_t verbose;
  double lm_lambda_min; /* MVUS_SOLVER_LM_SCHUR: floor of the Marquardt damping (3e-3; 0 = none).  Directions the data does
                           not determine (a control point seen by one camera: depth along its rays; rs against beta when the
                           image row hardly varies) have curvature << lambda * diag(H) and stay where they are instead of
                           following the noise -- the effect the reference gets from LSMR's truncated solves (common.py:670).
                           Problems whose motion rows reach over more than six control points (knots less than a frame apart: more
                           control points than detections) use at least 0.3 */
  double lm_trust_radius; /* MVUS_SOLVER_LM_SCHUR: the reference's trust region on top of the damping.  scipy's TRF (common.py:670,
                           x_scale = 1) bounds the Euclidean length of a step by Delta: Delta_0 = |x0|, Delta = 0.25 |step| after a
                           step whose actual / predicted reduction is below 0.25, Delta *= 2 after one above 0.75 that reached the
                           bound (scipy/optimize/_lsq/common.py update_tr_radius).  Here a damped step longer than Delta is cut back
                           to Delta along its direction and the damping is raised in proportion for the next solve.
                           0: Delta_0 = |x0| as scipy; > 0: this Delta_0; < 0: no trust region (damping only, rounds 2-4) */
} mvus_solve_opts;

/* scipy.optimize.OptimizeResult fields Scene.BA returns (common.py:670,697) */
typedef struct mvus_result {
  double cost;        /* 0.5*|f|^2 */
  double optimality;  /* |g|_inf (scaled by the Coleman-Li vector when bounded); LM_SCHUR stopped by max_nfev: at its last
                         linearisation point (the final accepted point is not re-linearised) */
  int32_t nfev, njev;
  int32_t status;     /* 0 max_nfev, 1 gtol, 2 ftol, 3 xtol, 4 ftol&xtol (scipy codes) */
  int32_t lin_iters;  /* total LSMR iterations / Cholesky solves */
  double solve_ms;    /* wall time of the call */
  double initial_cost;
} mvus_result;

/* sum-all-reduce of `count` doubles at device address `buf_dev`, issued on `stream`; returns 0 on success.
 * Called by the solver once per normal-equation assembly / J^T u product when observations are sharded. */
typedef int (*mvus_allreduce_fn)(void* user, void* buf_dev, size_t count, void* stream);

/* Always start from mvus_default_opts: a zero-filled mvus_solve_opts is NOT the default (lm_trust_radius = 0 means "scipy's
 * Delta_0", i.e. ON; the defaults are listed in INTEGRATION.md). */
void mvus_default_opts(mvus_solve_opts* opts);

/* Layout check for bindings in other languages (ctypes / cgo / JNI stubs that restate the structs): writes sizeof(mvus_solve_opts),
 * sizeof(mvus_result), sizeof(mvus_problem) as this library was compiled (any pointer may be NULL) and returns MVUS_ABI_VERSION.  A
 * binding asserts these against its own struct definitions at load time -- mvus_solve_opts has grown over the rounds (lm_lambda_min,
 * lm_trust_radius) and a stale stub would otherwise hand the library a short buffer.  The version is raised whenever a struct or an
 * EXISTING prototype of this header changes; an entry point that is only added (mvus_ba_set_frozen, mvus_ba_num_frozen, mvus_ba_covariance, mvus_ba_set_position_priors, mvus_ba_detection_covariance, mvus_ba_set_landmarks, mvus_triangulate_cov, mvus_spline_fit_open_w, mvus_spline_smooth_w, mvus_spline_fit_normal_w, mvus_spline_fit_residual_w) does not raise
 * it -- a binding that needs one finds it missing at load time.  Stateless, no device is touched.  No reference counterpart (the reference has no FFI). */
#define MVUS_ABI_VERSION 8
int32_t mvus_abi_sizes(int32_t* solve_opts_size, int32_t* result_size, int32_t* problem_size);

/* Copies the problem to the GPU, undistorts observations once when calibration is fixed
 * (detection_to_global, common.py:126).  */
int mvus_ba_create(const mvus_problem* p, mvus_ba** out);
void mvus_ba_destroy(mvus_ba* h);
const char* mvus_last_error(const mvus_ba* h);

int64_t mvus_ba_num_params(const mvus_ba* h);      /* n = 3C + C*P + 3*sum(n_s)            common.py:652 */
int64_t mvus_ba_num_residuals(const mvus_ba* h);   /* m = 2M + T                                          */
int64_t mvus_ba_num_motion_rows(const mvus_ba* h); /* T = len(spline_to_traj()[0]) when motion_reg else 0 */
int32_t mvus_ba_num_slots(const mvus_ba* h);       /* NS = 3 + P + 12 Jacobian slots per residual row     */

/* error_BA(x): f[m]  (common.py:448-487) */
int mvus_ba_residual(mvus_ba* h, const double* x, double* f);

/* Residual plus block-sparse Jacobian of the 2M detection rows (analytic; replaces the 2-point finite
 * differences scipy takes over jac_BA's pattern).  Outputs (any may be NULL):
 *   f[m];  J[2*NS*M]: J[(a*NS + k)*M + i] = d|e_a(i)| / d slot k, a = 0 (x) / 1 (y), observation i in
 *   camera-segmented order; slots: 0 alpha, 1 beta, 2 rs, 3..3+P camera params, 3+P+3q+d control point
 *   ctrl[i]+q coordinate d;  ctrl[M]: global index of the first active control point, -1 if not visible. */
int mvus_ba_residual_jacobian(mvus_ba* h, const double* x, int32_t jac_mode, double* f, double* J, int32_t* ctrl);

/* Motion-regulariser rows and their Jacobian: mf[T], mJ[36*T] (mJ[k*T + j], k = 12*sample + 3*q + d for the
 * samples j-1, j, j+1), mctrl[3*T] first control point of each of the three samples (-1 = unused). */
int mvus_ba_motion_rows(mvus_ba* h, const double* x, int32_t jac_mode, double* mf, double* mJ, int32_t* mctrl);

/* Fix the reference sparsity pattern at x0 (jac_BA + compute_visibility, common.py:427-438,490-610), computed on the
 * GPU.  pat[M]: per detection row a PATTERN CODE  p | (mask << 25)  -- p = global index of the lowest in-pattern
 * control point, bit k of the 4-bit mask set when control point p+k is in the pattern (three bits set) -- or -1 for
 * an all-zero row.  The nearest-three rule of common.py:559-563 gives three consecutive points (mask 0x7).  In rows
 * where exactly one of two control points with the SAME centre knot (t[2:-2] repeats the interval start and end) is
 * among the three nearest, which twin np.argsort returns depends on numpy's sort kernel (scalar / AVX2 / AVX512
 * builds differ): the reference's pattern is implementation defined there.  Those rows get the canonical choice and
 * bit 30 (MVUS_PAT_TIE) set in pat_out. */
#define MVUS_PAT_SHIFT 25
#define MVUS_PAT_TIE (1 << 30)
int mvus_ba_set_pattern(mvus_ba* h, const double* x0, int32_t* pat_out);

/* The pattern codes of the T motion rows (common.py:573-585; parameter independent, canonical unless uploaded). */
int mvus_ba_motion_pattern(mvus_ba* h, int32_t* motion_pat_out);

/* Supply the pattern instead: the matrix A the reference passes as jac_sparsity at common.py:670 is an INPUT of the
 * call this library replaces.  pat[M] / motion_pat[T] (NULL = keep) are pattern codes as above (bit 30 ignored); every
 * point of a code must belong to one spline.  Stays in force -- MVUS_JAC_PATTERN solves do not recompute it -- until
 * the next mvus_ba_set_pattern or mvus_ba_remove_outliers.  Column groups for MVUS_JAC_FD must be set afterwards. */
int mvus_ba_upload_pattern(mvus_ba* h, const int32_t* pat, const int32_t* motion_pat);

/* MVUS_SOLVER_LM_SCHUR.  The normal equations of the analytic Jacobian are assembled window-major (ba_assemble_win.hip.h): every
 * entry has one writer and one order of additions, no floating-point atomics -- a solve gives the same bits on every run, on one
 * rank and on every rank of a sharded run (the sums over the ranks are the collective's).  This call is kept for the ABI and
 * changes nothing (round 3 had an opt-in deterministic mode beside an atomic default).  No counterpart in the reference (scipy is
 * deterministic; the LM solver keeps that property). */
int mvus_ba_set_deterministic(mvus_ba* h, int32_t on);
/* *fell_back = 1 when the handle's LAST assembly went through the detection-major kernel, which adds with fp64 atomics (last-bit
 * differences from run to run): a camera whose frames are not in non-decreasing order, more than 256 cameras, or normal equations
 * formed from a stored Jacobian that is not the analytic one (pattern-masked, finite differences).  0 otherwise. */
int mvus_ba_deterministic_fallback(mvus_ba* h, int32_t* fell_back);

/* Column groups for MVUS_JAC_FD: groups[n] in [0, num_groups), two columns share a group only if no row of the
 * reference pattern contains both (scipy.optimize._numdiff.group_columns on jac_BA's matrix). */
int mvus_ba_set_fd_groups(mvus_ba* h, const int32_t* groups, int32_t num_groups);

/* scipy.optimize._numdiff.group_columns(A, order) -- what least_squares runs on jac_sparsity (the reference passes
 * jac_BA's matrix, common.py:665-670) -- on the HOST, from the pattern's entries instead of a scipy.sparse matrix:
 * entries (rows[k], cols[k]), k < nnz, of an m x n pattern in any order, duplicates allowed; order[n] = the column
 * permutation (scipy: numpy.random.RandomState(0).permutation(n)); groups[n] out.  Same greedy pass as scipy's
 * group_sparse over the permuted columns, hence the same groups.  Returns the number of groups, or a negative MVUS_E_*.
 * Stateless; no device is touched. */
int32_t mvus_group_columns(int64_t m, int64_t n, int64_t nnz, const int64_t* rows, const int64_t* cols, const int64_t* order, int32_t* groups);

/* The same grouping straight from the pattern CODES of a problem (pat[M] as mvus_ba_set_pattern / mvus_ba_upload_pattern use them,
 * motion_pat[T] or NULL without motion rows): the entries of jac_BA's matrix (common.py:559-610 -- per detection row alpha, beta
 * [, rs], the camera's parameters and the three nearest control points' coordinates; per motion row its control points) are
 * generated here instead of being handed over as two nnz-long arrays.  Host only; p as for mvus_ba_create. */
int32_t mvus_fd_groups(const mvus_problem* p, const int32_t* pat, const int32_t* motion_pat, const int64_t* order, int32_t* groups);

/* y[m] = J v (v[n]);  z[n] = J^T u (u[m]) with the Jacobian currently held by the handle
 * (after mvus_ba_residual_jacobian / inside solve).  Test and integration hooks for the operator. */
int mvus_ba_jv(mvus_ba* h, const double* v, double* y);
int mvus_ba_jtu(mvus_ba* h, const double* u, double* z);

/* Gauss-Newton normal equations of the current Jacobian: dense copies for inspection.
 *   g[n] = J^T f;  JtJ_cam[C*B*B] camera diagonal blocks, B = 3+P (row-major);
 *   band: block-banded spline part, band[((g*W + w)*3 + a)*3 + b] = (J^T J)[3g+a, 3(g+w)+b], w < W;
 *   cross[C*B*3N]: cross[(c*B + k)*3N + 3g + d].  Any output may be NULL; *W_out receives W. */
int mvus_ba_normal_equations(mvus_ba* h, double* g, double* JtJ_cam, double* band, double* cross, int32_t* W_out);

/* One damped Gauss-Newton step of MVUS_SOLVER_LM_SCHUR with the Jacobian and residual currently held:
 * p[n] = -(J^T J + lambda D)^-1 J^T f, D = diag(J^T J) (1 where 0).  Inspection hook for the whole solve chain
 * (assembly, band solver, Schur complement, reduced system); no trial evaluation, no bounds.  No reference counterpart. */
int mvus_ba_lm_step(mvus_ba* h, double lambda, double* p_out);

/* The linear solve of MVUS_SOLVER_TRF_LSMR on its own: LSMR (Fong & Saunders, scipy.sparse.linalg.lsmr) on
 *   A = [J diag(D); diag(E)],  right-hand side [b; 0],  min |A x - [b; 0]|^2 + damp^2 |x|^2,  x started from 0,
 * with the Jacobian currently held (after mvus_ba_residual_jacobian).  b[m]; D[n], E[n] or NULL (D = 1, no extra rows): the column scaling
 * and the extra diagonal rows of scipy's trf_bounds; atol, btol, conlim as scipy's (0: that test never stops the run); maxiter <= 0:
 * min(rows of A, n).  Inspection hook for the solver's loop -- the device-resident iteration, and whatever MVUS_LSMR_HOST,
 * MVUS_LSMR_BOUNDED_HOST (read when the handle was created) and MVUS_LSMR_ONE_PASS (read at every run) select.  With a frozen mask in
 * force the frozen columns of J are zero, as inside a solve, and x[k] = 0.0 there.  No reference counterpart.
 *   x_out[n];  *itn_out iterations run;  *istop_out scipy's istop (7: maxiter);  norms_out[4] = normr, normar, normA, condA at return
 *   (itn_out, istop_out, norms_out may be NULL).
 * Changes no state of the handle: the held Jacobian, residual and point, the damping history and what a later mvus_ba_solve returns stay.
 * MVUS_E_INVALID: b or x_out NULL, damp < 0 or NaN, no Jacobian held.  MVUS_E_UNSUPPORTED: a sharded handle (set_allreduce / set_rccl /
 * set_time_shard). */
int mvus_ba_lsmr(mvus_ba* h, const double* b, const double* D, const double* E, double damp, double atol, double btol, double conlim,
                 int64_t maxiter, double* x_out, int32_t* itn_out, int32_t* istop_out, double* norms_out);

/* Robust loss: least_squares(..., loss=, f_scale=) of common.py:670 (the reference passes neither: linear, 1.0).  With z = (f_i / f_scale)^2
 * for EVERY row of f (motion rows included, as scipy does with error_BA):
 *   MVUS_LOSS_LINEAR rho = z | SOFT_L1 2 (sqrt(1 + z) - 1) | HUBER z if z <= 1 else 2 sqrt(z) - 1 | CAUCHY log(1 + z) | ARCTAN atan(z)
 *   cost = 0.5 f_scale^2 sum rho(z_i)  (mvus_result cost, initial_cost, the gain ratio of every trial);
 *   linearisation = scipy's scale_for_robust_loss_function: J_i <- s_i J_i, f_i <- rho' f_i / s_i, s_i = sqrt(max(rho' + 2 rho'' z, 2.22e-16)),
 *   i.e. g = J^T (rho' f), H = J^T diag(s^2) J, damping diag(H) of that H; optimality = |g|_inf of that g.
 * In force for every later mvus_ba_solve / mvus_ba_normal_equations / mvus_ba_lm_step on the handle until set again; everything about
 * error_BA itself (residual, Jacobian, J v, J^T u, motion rows, outlier masks, f_out of a solve) stays raw.  Setting a loss drops what
 * an earlier LM solve carried over (cost, normal equations) and, when the loss changes, the damping history.
 * MVUS_E_INVALID: unknown loss, f_scale not finite or <= 0.  With a loss other than linear mvus_ba_solve returns MVUS_E_UNSUPPORTED for
 * MVUS_SOLVER_TRF_LSMR, for a Jacobian mode other than MVUS_JAC_ANALYTIC and on sharded handles -- it never solves the linear problem
 * instead. */
#define MVUS_LOSS_LINEAR 0
#define MVUS_LOSS_SOFT_L1 1
#define MVUS_LOSS_HUBER 2
#define MVUS_LOSS_CAUCHY 3
#define MVUS_LOSS_ARCTAN 4
int mvus_ba_set_loss(mvus_ba* h, int32_t loss, double f_scale);
/* 0.5 f_scale^2 sum rho((f_i / f_scale)^2) at x under the loss in force; weights_out[m] (may be NULL) = rho'(z_i), the weight each row
 * has in the gradient (1 = inlier, -> 0 = ignored), in the row order of f.  One rank only. */
int mvus_ba_robust_cost(mvus_ba* h, const double* x, double* cost_out, double* weights_out);

/* Hold chosen camera-side unknowns constant: frozen[k] = 1 keeps x[k] where it is, k over the head of x in its own order -- alpha(C),
 * beta(C), rs(C), then the P parameters of every camera -- so count must be C * (3 + P); control points are not freezable.  frozen == NULL
 * or count == 0 clears the mask, and a mask of zeros is no mask.  The reference can only switch whole groups off for every camera
 * (opt_sync, the `rs` argument, opt_calib: common.py:512-518, 621); this is the per-parameter form: a hardware-synchronised pair (alpha, beta),
 * a surveyed camera (pose), trusted intrinsics beside cameras that run opt_calib, or the gauge -- the first camera's pose and one translation
 * component of the second take the seven degrees of freedom of the similarity away (Scene settings ba_gauge / ba_freeze).
 * State of the handle, as the loss is: in force for every later mvus_ba_solve / mvus_ba_normal_equations / mvus_ba_lm_step until set again, kept
 * over mvus_ba_remove_outliers; everything about error_BA itself (residual, mvus_ba_residual_jacobian, J v, J^T u, motion rows, outlier masks)
 * stays raw.  With a mask the frozen columns of J are zero: in the normal equations g[k] = 0 and row and column k of H are zero except
 * H[k][k] = 1 (so D[k] = 1 and lambda = 0 stays solvable), the step has p[k] = 0 and x[k] comes back from a solve with the bits it went in
 * with -- both solvers, every Jacobian mode; under rs_bounds a held rs has no box in either solver (on a bound or outside [0, 1] it stays as given).  Setting or clearing drops what an earlier LM solve
 * carried over (cost, normal equations, the speculative linearisation) and, when the mask changes, the damping history: after clearing, a
 * solve is a fresh handle's bit for bit.  A handle without a mask runs exactly the kernels it ran before this entry point existed.
 * MVUS_E_INVALID: count is neither 0 nor C * (3 + P), a value other than 0 or 1.  MVUS_E_UNSUPPORTED ("sharded" in the message): a non-empty
 * mask on a sharded handle (set_allreduce / set_rccl / set_time_shard), here or -- when the route is installed afterwards -- from the calls
 * above: never solved unmasked.  mvus_ba_num_frozen: the number of held unknowns (0 = no mask). */
int mvus_ba_set_frozen(mvus_ba* h, const uint8_t* frozen, int64_t count);
int64_t mvus_ba_num_frozen(const mvus_ba* h);

/* Position priors on the trajectory (ba_prior.hip.h; no reference counterpart: the reference compares a GPS / RTK log with the result
 * afterwards, analysis/compare_gt.py).  Prior k is a surveyed position p_k at time t_k with weights w_k = 1 / sigma_k per axis; it adds
 * the three rows  r = w_k (.) (S(t_k) - p_k)  to the least-squares problem, S the cubic spline of the unknowns.  t_k is on the spline's
 * own timeline (the reference camera's frame clock) and is a constant, not an unknown.  A weight of 0 leaves that axis out.  Three
 * priors that are not collinear fix the seven freedoms of the similarity gauge: the solution, and its covariance, are then in the
 * surveyed frame and in its unit, with no anchor.
 *   t[K], P[3K] = x(K) y(K) z(K), w[3K] in the same layout, in any order (the library sorts by (t, input order)); K = 0 or a NULL array
 *   clears the priors.  A prior is ACTIVE when start <= t_k <= end for some interval of the spline, both ends closed (at t_k = end the
 *   basis is the right-end value, as splev gives it); the others contribute nothing and are only counted.
 * State of the handle, as the loss and the frozen mask are: in force for every later mvus_ba_solve (MVUS_SOLVER_LM_SCHUR, every Jacobian
 * mode) / mvus_ba_normal_equations / mvus_ba_lm_step / mvus_ba_covariance until set again, kept over mvus_ba_remove_outliers.  There
 *   cost and initial_cost of mvus_result += 0.5 sum r^2;  g and the band of the normal equations gain  h_a w^2 (S - p)  and
 *   h_a h_b diag(w^2)  on the four control points of the prior's knot span (h its four B-spline weights); the camera blocks, the camera
 *   gradient and the cross block are untouched and the band is not widened;  the covariance's dof counts one row per active (prior, axis)
 *   with w > 0.
 * The rows are plain L2: a robust loss in force reweights detection and motion rows only.  Everything about error_BA itself (residual,
 * Jacobian, J v, J^T u, motion rows, outlier masks, mvus_ba_robust_cost, f_out of a solve: 2M + T rows) stays raw.  Setting or clearing
 * drops what an earlier LM solve carried over (cost, normal equations, the speculative linearisation) as mvus_ba_set_loss does, and leaves
 * the damping history alone; a handle without active priors runs exactly the kernels it ran before this entry point existed.
 * MVUS_E_INVALID: K < 0 or K > 2^28, a non-finite t, P or w, a negative weight.  MVUS_E_UNSUPPORTED: priors on a sharded handle ("sharded" in the
 * message; set_allreduce / set_rccl / set_time_shard, here or -- when the route is installed afterwards -- from the calls above), and
 * mvus_ba_solve with MVUS_SOLVER_TRF_LSMR while a prior is active ("TRF_LSMR" in the message): never solved with the priors dropped.
 * Not offered: a time offset of the position log as an unknown, full 3 x 3 prior covariances.
 * mvus_ba_num_position_priors: K as set; *active_out (may be NULL) the active ones.
 * mvus_ba_position_prior_cost: 0.5 sum r^2 at x and, when r_out is not NULL, r[3K] in the CALLER's order and layout, NaN for inactive
 * priors (inspection hook; one rank).  x is evaluated in a buffer of its own: the held Jacobian, its point, f and the blocks of the last
 * mvus_ba_normal_equations stay as they are. */
int mvus_ba_set_position_priors(mvus_ba* h, int64_t K, const double* t, const double* P, const double* w);
int64_t mvus_ba_num_position_priors(const mvus_ba* h, int64_t* active_out);
int mvus_ba_position_prior_cost(mvus_ba* h, const double* x, double* cost_out, double* r_out);

/* Surveyed landmarks (ba_landmark.hip.h; no reference counterpart): L constant world points X_l -- ground control points -- and K
 * observations (camera c_k, landmark l_k, raw pixel (u_k, v_k), weights (wu_k, wv_k) = 1 / sigma in pixels, 0: that axis is unknown).
 * Observation k adds the two rows  r_k = w_k (.) (pi_c(X_l) - obs_k), signed, predicted minus observed, where pi_c and obs are what a
 * detection row does with the spline point replaced by X_l: rotate, translate, divide, apply K; under fixed calibration with
 * undist_points the observed pixel is undistorted once at set time, under opt_calib inside the row with the unknown K and d.  The rows
 * have the P camera columns of a detection row (P = 6: rvec, t; P = 15: fx, fy, cx, cy, rvec, t, k1, k2, p1, p2, k3) and no others: no
 * alpha / beta / rs, no control points, no visibility test (a landmark has no time), no cheirality test.  Three landmarks that are not
 * collinear, seen by the cameras, fix the seven freedoms of the similarity gauge, the scale included.
 *   X[3L] = x(L) y(L) z(L); cam[K], point[K]; uv[2K] = u(K) v(K); w[2K] in the same layout, in any order (the library sorts by
 *   (camera, landmark, input order)); K = 0 or a NULL array clears.
 * State of the handle, as the loss, the frozen mask and the position priors are: in force for every later mvus_ba_solve
 * (MVUS_SOLVER_LM_SCHUR, every Jacobian mode) / mvus_ba_normal_equations / mvus_ba_lm_step / mvus_ba_covariance /
 * mvus_ba_detection_covariance until set again, kept over mvus_ba_remove_outliers.  There
 *   cost and initial_cost of mvus_result += 0.5 sum r^2;  camera block c gains sum J^T J on its P x P part and the camera gradient
 *   sum J^T r on its P entries (J = d r / d camera parameters, weighted), in front of the freeze pass: held parameters stay held.  The
 *   sync slots of the block, the cross block, the band, the spline gradient and other cameras' blocks are untouched.  The covariance's
 *   dof counts one row per (observation, axis) with w > 0.
 * The rows are plain L2: a robust loss in force reweights detection and motion rows only.  Everything about error_BA itself stays raw
 * (2M + T rows), as do mvus_ba_robust_cost and mvus_ba_position_prior_cost.  Setting or clearing drops what an earlier LM solve carried
 * over, as mvus_ba_set_loss does, and leaves the damping history alone; a handle without a weighted observation runs exactly the
 * kernels it ran before this entry point existed.  The sums are formed by one writer per entry in sorted order: the same bits on every
 * run, and for every order of the observations as long as no (camera, landmark) pair occurs twice.
 * MVUS_E_INVALID, before the device is touched: L or K < 0, K > 2^24, a camera index outside [0, C), a landmark index outside [0, L), a
 * non-finite X, uv or w, a negative weight.  MVUS_E_UNSUPPORTED: landmarks on a sharded handle ("sharded" in the message, here or --
 * when the route is installed afterwards -- from the calls above); mvus_ba_solve with MVUS_SOLVER_TRF_LSMR while a weighted observation
 * is set ("TRF_LSMR" in the message); mvus_ba_register_cameras / mvus_ba_register_linearize while observations are set ("landmark" in the
 * message: their per-camera problems would drop rows that involve exactly that camera).
 * Not offered: landmarks as unknowns, full 2 x 2 weights, landmarks inside the register problems, MVUS_SOLVER_TRF_LSMR, sharded handles.
 * mvus_ba_num_landmark_observations: K as set; *rows_out (may be NULL) the rows with w > 0.
 * mvus_ba_landmark_cost: 0.5 sum r^2 at x and, when r_out is not NULL, r[2K] = ru(K) rv(K) in the CALLER's order.
 * mvus_ba_landmark_rows: r as above and J_out[K][2][P] = d r / d (camera parameters of c_k), weighted, in the caller's order (either may
 * be NULL).  Both are inspection hooks on one rank: x is evaluated in a buffer of its own, the held Jacobian, its point, f and the blocks
 * of the last mvus_ba_normal_equations stay as they are. */
int mvus_ba_set_landmarks(mvus_ba* h, int64_t L, const double* X, int64_t K, const int32_t* cam, const int32_t* point, const double* uv, const double* w);
int64_t mvus_ba_num_landmark_observations(const mvus_ba* h, int64_t* rows_out);
int mvus_ba_landmark_cost(mvus_ba* h, const double* x, double* cost_out, double* r_out);
int mvus_ba_landmark_rows(mvus_ba* h, const double* x, double* r_out, double* J_out);

/* Covariance of the estimate at x (ba_cov.hip.h; no reference counterpart: scipy's least_squares returns none either).  With the loss and the
 * frozen mask in force, H is the matrix mvus_ba_normal_equations exports at x -- J^T J, or scipy's J^T diag(s^2) J under a robust loss (the
 * usual Gauss-Newton approximation then), the motion rows included as the prior they are.  An unknown is ESTIMATED when it is not frozen and
 * its diagonal entry of H is non-zero (not: rs without rolling shutter, a control-point coordinate no row touches);
 *   Sigma = sigma^2 (H restricted to the estimated unknowns)^-1, rows and columns of the others exactly 0.
 * sigma2 > 0: the caller's variance factor; otherwise the a-posteriori one, 2 cost / (m_act - n_est) -- cost the (robust) cost at x, m_act the
 * rows of f with a non-empty Jacobian row (every motion row, both rows of every detection with a span), n_est the estimated unknowns
 * (MVUS_E_INVALID when m_act <= n_est).  Outputs (any may be NULL):
 *   cov_cam[CB * CB], CB = C * (3 + P): the camera-side block, in the order of the head of x -- alpha(C), beta(C), rs(C), then P per camera
 *     (the order of mvus_ba_set_frozen);
 *   cov_band[N][4][3][3]: blocks (p, p + w), w = 0..3, of the control points' block in control-point order (p = index over all splines,
 *     coordinates x, y, z inside a block), zero where p + w >= N -- what the covariance of any point of the trajectory needs
 *     (mvus_spline_cov_eval); camera-trajectory cross-covariances are not returned;
 *   estimated[n] in the order of x;  *sigma2_out the factor used;  *dof_out = m_act - n_est.
 * H is singular while the similarity gauge is free: a pivot p_k <= 1e-10 H_kk of either factorisation (spline block, reduced camera system)
 * returns MVUS_E_NUMERIC with a message that names the unknown -- fix the gauge with mvus_ba_set_frozen (settings ba_gauge: "anchor" /
 * ba_freeze).  Below that bound fewer than about six digits of a variance survive fp64.  MVUS_E_UNSUPPORTED: a sharded handle ("sharded" in
 * the message), more than 1152 camera-side unknowns, a band wider than 16 control points.  Computed on the device only (no CPU fallback).
 * The call drops what an LM solve carried over (cost, blocks, the speculative linearisation) exactly as mvus_ba_set_loss does and leaves the
 * damping history alone: a later solve returns the bits it would have returned without the call.  Like mvus_ba_residual_jacobian it leaves
 * the analytic Jacobian of x held. */
int mvus_ba_covariance(mvus_ba* h, const double* x, double sigma2, double* cov_cam, double* cov_band, uint8_t* estimated,
                       double* sigma2_out, int64_t* dof_out);
/* Measurement hook: milliseconds (HIP events) of the stages of the LAST mvus_ba_covariance on the handle and their names, the first `count`
 * of them; returns the number of stages, or MVUS_E_INVALID before the first call. */
int32_t mvus_ba_covariance_stage_ms(mvus_ba* h, double* ms_out, const char** names_out, int32_t count);

/* The covariance carried back to the image plane (ba_detcov.hip.h): per detection the covariance of its fitted value and its studentised
 * residual, at x, with the loss, the frozen mask and the position priors in force.  Sigma is EXACTLY the matrix mvus_ba_covariance defines.
 * For detection i of camera c with a knot span, J_i = the two rows of the analytic Jacobian (raw: the loss does not scale them; frozen
 * columns contribute nothing, Sigma is zero there), Pi_i = J_i Sigma J_i^T -- which needs the camera-trajectory cross-covariance the
 * library keeps to itself.  Outputs (any may be NULL), detections in camera-segmented order as for mvus_ba_residual_jacobian:
 *   e_out[2M] = u(M) v(M): the SIGNED residual in pixels, predicted minus observed; |e| is bit for bit the two rows of f of the detection;
 *   pcov_out[3M] = uu(M) uv(M) vv(M): P = D Pi_i D, D = diag(sign e_u, sign e_v) -- the covariance of the fitted detection in image axes
 *     (its 1-sigma ellipse).  With opt_calib and undist_points the observed point is undistorted with the unknown intrinsics and so
 *     depends on x too: P is then the covariance of the fitted part of the residual in the undistorted frame, not of a bare projection;
 *   t2_out[M] = r^T (sigma^2 I - Pi_i)^-1 r, r = |e|: the squared studentised residual (independent of the signs), NaN when
 *     sigma^2 I - Pi_i is not positive definite.  chi^2 with 2 degrees of freedom under the linear loss only; under a robust loss it is
 *     the Gauss-Newton approximation described above.
 * A detection without a span: NaN in pcov_out and t2_out, 0 in e_out.
 * cov_cam, cov_band, estimated, sigma2_out, dof_out: exactly what mvus_ba_covariance returns for the same arguments (one run of the chain
 * serves both).  Refusals and side effects are those of mvus_ba_covariance, the messages prefixed "detection_covariance:".  The first call
 * allocates one more buffer of 3N x CB doubles (T = Z Sigma_cc); MVUS_E_HIP when that fails. */
int mvus_ba_detection_covariance(mvus_ba* h, const double* x, double sigma2, double* e_out, double* pcov_out, double* t2_out, double* cov_cam,
                                 double* cov_band, uint8_t* estimated, double* sigma2_out, int64_t* dof_out);
/* Measurement hook: milliseconds (HIP events) of the detection pass of the LAST mvus_ba_detection_covariance on the handle; MVUS_E_INVALID
 * before the first such call. */
int32_t mvus_ba_detection_covariance_ms(mvus_ba* h, double* ms_out);

/* The least_squares call of Scene.BA (common.py:670) -- x is read and overwritten with res.x.
 * lb/ub come from opts of the problem (rs_bounds).  f_out[m] may be NULL.  x, res and f_out are complete on return.  MVUS_SOLVER_LM_SCHUR
 * with f_out == NULL may return while device work for the NEXT call is still running on the handle's stream (the linearisation at the
 * returned point, enqueued before the accept / reject decision was known); every later call on the handle is ordered behind it, and a
 * solve that continues from the returned x reuses it together with f(x) and the cost instead of evaluating them again.
 * Termination tests, nfev/njev counting and status codes follow scipy for both solvers (max_nfev = the reference's
 * max_iter); MVUS_SOLVER_LM_SCHUR does not re-linearise the accepted point when max_nfev stops it. */
int mvus_ba_solve(mvus_ba* h, double* x, const mvus_solve_opts* opts, mvus_result* res, double* f_out);

/* Register cameras against a HELD trajectory: a batch of B small, independent least-squares problems, each solved by Levenberg-Marquardt
 * entirely on the device (one read-back at the end of the call).  Problem b is (camera cam[b] of the handle, start vector start[b]): its
 * 3 + P unknowns are that camera's alpha, beta, rs and P parameters -- the order of one camera's entries in mvus_ba_set_frozen -- and the
 * control points are those of x[n], constants.  It minimises 0.5 sum rho over the camera's 2 M_c detection rows only (motion rows and
 * position priors do not involve a camera): visibility is evaluated at every point, switched-off groups (opt_sync = 0, rs_free = 0) have
 * zero columns, the handle's frozen mask restricted to the camera holds further entries (g_k = 0, row and column zero, H_kk = 1; the value
 * returns with the bits it went in with), the handle's loss (mvus_ba_set_loss) is in force with scipy's row scaling as in the LM + Schur
 * assembly, and under rs_bounds the trial point is projected onto 0 <= rs <= 1 (a held rs has no box).  The LM rules are those of
 * MVUS_SOLVER_LM_SCHUR per problem: D = diag(H) (1 where 0), (H + lambda D) p = -g by Cholesky, lambda_0 = max(lambda0 > 0 ? lambda0 : 1e-4,
 * lambda_min), Nielsen's update on a gain, lambda *= nu, nu *= 2 on none, a failed factorisation (x 10) or a non-finite trial cost (x nu)
 * raises lambda up to 1e12, no trust region; termination, nfev and status 0 - 4 follow scipy's check_termination, |x| in the xtol test being
 * the norm of the problem's own 3 + P vector.  Status -1: the problem was never started (non-finite cost at the start, or fewer rows with a
 * Jacobian -- two per visible detection -- than free unknowns).
 *   start[B * (3 + P)]: alpha, beta, rs, then the P parameters of each problem; NULL = every problem starts from x's entries of its camera.
 * Outputs (any may be NULL): cam_out[B * (3 + P)] the result of each problem; cost_out / cost0_out[B] the (robust) cost at the result and at
 * the start; nfev_out, status_out[B]; visible_out[B] detections with a span at the result; inliers_out[B] visible detections with
 * sqrt(ex^2 + ey^2) < inlier_thres at the result (the score of remove_outliers; it cannot be raised by sliding the camera out of the
 * trajectory's time range, as the cost can be lowered), not computed (0) when inlier_thres <= 0.
 * A problem's result has the same bits alone, anywhere in any batch, and from run to run.  Both calls work in buffers of their own: the
 * held Jacobian, what an LM solve carried over, the damping history and the blocks of mvus_ba_normal_equations stay as they are -- a later
 * mvus_ba_solve returns the bits it would have returned without the call.
 * MVUS_E_INVALID before the device is touched: B < 0, B > 4096, a camera index outside [0, C), a non-finite start, max_nfev < 1, a negative
 * tolerance (B == 0 is MVUS_OK and does nothing).  MVUS_E_NUMERIC: an rs start outside [0, 1] under rs_bounds unless held, as mvus_ba_solve
 * treats x0.  MVUS_E_UNSUPPORTED on a sharded handle ("sharded" in the message).  No CPU fallback.  No reference counterpart. */
int mvus_ba_register_cameras(mvus_ba* h, const double* x, int32_t B, const int32_t* cam, const double* start,
                             int32_t max_nfev, double ftol, double xtol, double gtol, double lambda0, double lambda_min, double inlier_thres,
                             double* cam_out, double* cost_out, double* cost0_out, int32_t* nfev_out, int32_t* status_out,
                             int64_t* visible_out, int64_t* inliers_out);
/* Inspection hook of the above (like mvus_ba_lsmr): the normal equations of each problem at its start point exactly as the first iteration
 * of the solver forms them, by the same kernels -- H_out[B][(3 + P)^2] full symmetric (held entries: row and column zero, H_kk = 1;
 * switched-off ones: zero), g_out[B][3 + P], cost_out[B] the (robust) cost and visible_out[B] at the start points.  Arguments, errors and
 * what it leaves alone as above. */
int mvus_ba_register_linearize(mvus_ba* h, const double* x, int32_t B, const int32_t* cam, const double* start,
                               double* H_out, double* g_out, double* cost_out, int64_t* visible_out);

/* Scene.remove_outliers (common.py:700-717): keep[i] = sqrt(ex^2 + ey^2) < thres, camera-segmented order. */
int mvus_ba_outlier_mask(mvus_ba* h, const double* x, double thres, uint8_t* keep);

/* Scene.remove_outliers applied to the handle itself (common.py:709-714: `detections[i] = detections[i][:, error<thres]`):
 * evaluates the mask at x, compacts the device-resident detection arrays in place (order kept) and rebuilds the launch
 * tables, so the next mvus_ba_solve -- the second BA of main.py:59 -- runs on the inliers without a new handle or any
 * re-upload.  keep_out[M_old] (may be NULL) receives the mask, det_offsets_out[C+1] the new camera offsets.
 * On a sharded handle every rank filters its own detections (all ranks must call it: the global row count is re-summed). */
int mvus_ba_remove_outliers(mvus_ba* h, const double* x, double thres, uint8_t* keep_out, int64_t* det_offsets_out);

/* Multi-GPU: observations sharded across ranks, this handle holds one shard.  `is_root` ranks add the
 * replicated terms (motion rows, damping) exactly once. */
int mvus_ba_set_allreduce(mvus_ba* h, mvus_allreduce_fn fn, void* user, int32_t is_root);

/* The same sums by RCCL called from the library itself (no host language in the iteration): every collective is one
 * ncclAllReduce(double, sum, in place) on the handle's stream.  One rank obtains an id with mvus_rccl_unique_id (128 bytes, RCCL's
 * ncclUniqueId) and hands it to the others by any means (a torch.distributed / MPI broadcast, a file); every rank then calls
 * mvus_ba_set_rccl, which joins the communicator (ncclCommInitRank: collective, blocks until all `world` ranks have called) on the
 * handle's device.  librccl.so.1 is opened at run time (the copy the process already holds -- e.g. PyTorch's -- else the loader's):
 * the library has no link-time dependency on it and MVUS_E_COMM reports its absence.  Replaces a callback set earlier; is_root as
 * above.  The sums of a given topology are RCCL's: the same bits on every run.  SURVEY 8e's collective; no reference counterpart. */
/* mvus_rccl_available: MVUS_OK when librccl.so.1 can be opened and its entry points resolved in this process, else MVUS_E_COMM (message:
 * mvus_last_error(NULL)).  It touches no device and no communicator: a job asks it on EVERY rank and exchanges the answers before any
 * rank calls mvus_ba_set_rccl -- ncclCommInitRank is itself a blocking collective, and a rank that cannot open RCCL would otherwise
 * leave the others waiting inside it (mvus_amd/dist.py::agree_on_rccl). */
int mvus_rccl_available(void);
int mvus_rccl_unique_id(uint8_t id_out[128]);
int mvus_ba_set_rccl(mvus_ba* h, const uint8_t id[128], int32_t rank, int32_t world, int32_t is_root);
/* Measurement hook: `reps` back-to-back sums of `count` doubles (a scratch buffer) through the route installed on the handle (the
 * callback or RCCL) between two hipEvents; average milliseconds per collective. */
int mvus_ba_time_allreduce(mvus_ba* h, int64_t count, int32_t reps, double* avg_ms);

/* Time sharding for the LM/Schur solver ("shard by time range"): this handle was created with the
 * detections of ONE time slice and owns the spline control points [ctrl_cuts[rank], ctrl_cuts[rank+1]) (global
 * control-point indices over all splines, ctrl_cuts[0] = 0, ctrl_cuts[world] = N; every rank passes the same array).
 * Each rank then assembles and factorises only its slice of the spline blocks; the cross block never leaves its GPU.
 * Per LM iteration the all-reduce callback (mvus_ba_set_allreduce, required) sums: the camera blocks + the blocks of the
 * control points within `halo` of a cut (rows of both neighbours land there), the separator system of the band solver,
 * the Schur complement contributions, the step, diag(H) and g -- a few MB in all, instead of the whole cross block.
 * A detection whose four control points leave [own range -+ halo) (time-stamp drift larger than the halo) makes the
 * next solve fail with MVUS_E_HIP and a message saying so.  Motion rows are evaluated by the rank owning their first
 * control point (is_root of mvus_ba_set_allreduce is ignored).  Call before mvus_ba_set_allreduce.  world = 1 turns
 * it off.  No reference counterpart (the reference is single-process). */
int mvus_ba_set_time_shard(mvus_ba* h, int32_t rank, int32_t world, const int32_t* ctrl_cuts, int32_t halo);

/* Measurement hook for bench.py: runs `launches` back-to-back launches of one kernel on the handle's
 * stream between two hipEvents and returns the average duration in milliseconds.
 *   which: 0 residual (with a loss other than linear in force: the whole cost evaluation of a robust LM trial -- residual kernel with
 *   the robust partial sums, motion rows and the final sum), 1 residual+Jacobian with the outputs ROTATING over >= 3 buffer sets (>= 1 GiB in rotation, so no
 *   launch writes into lines its predecessor left in the 256 MiB Infinity Cache), 2 J v, 3 J^T u, 4 normal-equation
 *   assembly from the materialised Jacobian, 5 residual+Jacobian re-launched into one buffer set (cache-resident variant,
 *   for comparison), 6 the fused Jacobian + normal-equation assembly of the LM path (no Jacobian in memory), 7 the landmarks' cost kernel,
 *   8 the landmarks' normal-equation kernel (7, 8: MVUS_E_INVALID without a weighted landmark observation) */
int mvus_ba_time_kernel(mvus_ba* h, int32_t which, int32_t launches, double* avg_ms);

/* Upload x to the handle without evaluating anything (used with mvus_ba_time_kernel). */
int mvus_ba_set_x(mvus_ba* h, const double* x);

/* Two-view linear triangulation, epipolar.triangulate_matlab (reconstruction/epipolar.py:497-510) as called by
 * Scene.triangulate (common.py:783): for each of N point pairs the right singular vector of the smallest singular value
 * of the 4x4 matrix built from the two projections, divided by its last component.  x1, x2: [2*N] (u(N) then v(N)) pixel
 * coordinates in camera 1 / 2; P1, P2: [12] row-major 3x4 projection matrices; X: [4*N] rows x, y, z, 1.
 * err1 / err2 (NULL = skip): [N] reprojection distances of X in the two cameras (epipolar.reprojection_error of
 * Camera.projectPoint, common.py:786-787), the quantity Scene.triangulate thresholds.  Stateless: no handle; errors of
 * this call are reported by mvus_last_error(NULL).  No CPU fallback. */
int mvus_triangulate(int32_t device, int64_t N, const double* x1, const double* x2, const double* P1, const double* P2,
                     double* X, double* err1, double* err2);

/* mvus_triangulate with the covariance of every point.  Arguments, layouts and the bits of X, err1, err2 as there (the same Jacobi SVD, one
 * lane per pair, in k_triangulate_cov).  cov[6*N], component-major xx(N) xy(N) xz(N) yy(N) yz(N) zz(N): the Gauss-Newton covariance
 * (A^T A)^-1 of the point at the returned X, A the four rows (P_c[r,:3] - x_r P_c[2,:3]) / (z_c sigma_c), r = 0, 1, c = 1, 2, with (x_0, x_1)
 * the reprojection of X in camera c, z_c its third homogeneous component and sigma_c the pixel noise (1-sigma, isotropic) of camera c; the
 * 3x3 inverse by Cholesky in registers.  To first order this is the covariance of the point of least reprojection error; the linear
 * triangulation is close to that point, not equal to it (tests/test_gpu_triangulate_cov.py measures how close).  All six entries of a pair are
 * NaN when a Cholesky pivot is at most 1e-14 of its diagonal entry (no parallax), X is not finite, or z_c <= 0 in either camera.
 * Not offered: a full 2x2 pixel covariance per detection, and the covariance of anything but the point (the cameras are taken as exact).
 * MVUS_E_INVALID, before the device is touched: sigma1 or sigma2 not finite or <= 0; cov == NULL (mvus_triangulate is that call); what
 * mvus_triangulate refuses.  Stateless; no CPU fallback.  No reference counterpart. */
int mvus_triangulate_cov(int32_t device, int64_t N, const double* x1, const double* x2, const double* P1, const double* P2, double sigma1, double sigma2,
                         double* X, double* cov, double* err1, double* err2);

/* Scene.spline_to_traj (common.py:273-301): evaluate the S trajectory splines at nt timestamps.  interval: [2*S] row-major
 * spline['int'] (starts then ends); knot_offsets [S+1] / knots: concatenated spline['tck'][s][0]; coefs: concatenated
 * spline['tck'][s][1] (cx(n_s) cy(n_s) cz(n_s) per spline).  which[nt] receives the interval each timestamp belongs to
 * (start <= t <= end, closed like common.py:292) or -1; X[3*nt] (x(nt) y(nt) z(nt)) the point, 0 where which = -1.
 * Same recurrence as scipy.interpolate.splev (FITPACK splev.f / fpbspl.f).  Stateless; no CPU fallback. */
int mvus_spline_eval(int32_t device, int32_t S, const double* interval, const int64_t* knot_offsets, const double* knots,
                     const double* coefs, int64_t nt, const double* t, double* X, int32_t* which);

/* Covariance of trajectory samples from mvus_ba_covariance's cov_band[N][4][3][3] (N = all control points, the splines one behind the other as
 * in x): for each of the nt timestamps  Cov X(t) = sum_{a,b} h_a(t) h_b(t) Sigma(p + a, p + b)  over the four control points p .. p + 3 of its
 * knot span, h the basis values mvus_spline_eval uses.  cov[nt * 9]: a row-major 3 x 3 per sample, NaN where which = -1 (outside every
 * interval, closed like mvus_spline_eval).  Arguments as mvus_spline_eval.  One lane per sample; stateless; no CPU fallback. */
int mvus_spline_cov_eval(int32_t device, int32_t S, const double* interval, const int64_t* knot_offsets, const double* knots,
                         const double* cov_band, int64_t nt, const double* t, double* cov, int32_t* which);

/* Kinematics of the trajectory (arguments, checks and `which` as mvus_spline_eval; one lane per sample; stateless; no CPU fallback).
 *
 * mvus_spline_eval_der: X and its first nder derivatives in the spline parameter (nder = 0, 1 or 2, else MVUS_E_INVALID).
 * D[(nder + 1) * 3 * nt], order-major and inside an order x(nt) y(nt) z(nt) as X of mvus_spline_eval, whose bits the order-0 block has;
 * 0 where which = -1.  All orders come from one span search and one run of the FITPACK recurrence (splder.f / fpader.f for the second).
 * On a knot the derivatives are those from the right, at the last knot of a spline those from the left, as scipy's splev(der=). */
int mvus_spline_eval_der(int32_t device, int32_t S, const double* interval, const int64_t* knot_offsets, const double* knots,
                         const double* coefs, int64_t nt, const double* t, int32_t nder, double* D, int32_t* which);

/* Covariance of the state (X, X', .., D^nder X) of each sample from cov_band[N][4][3][3] (as mvus_spline_cov_eval): with Dn = 3 (nder + 1),
 * component 3 i + r = coordinate r of derivative i,  Cov(D^i X, D^j X) = sum_{a,b} h^(i)_a h^(j)_b Sigma(p + a, p + b).  cov[nt * Dn * Dn],
 * a row-major Dn x Dn per sample, symmetric to the bit, NaN where which = -1.  nder as above. */
int mvus_spline_kin_cov_eval(int32_t device, int32_t S, const double* interval, const int64_t* knot_offsets, const double* knots,
                             const double* cov_band, int64_t nt, const double* t, int32_t nder, double* cov, int32_t* which);

/* Distance flown: dist[nt] = the length of the curve from the start of the sample's interval to the sample (exactly 0 at the start, and
 * where which = -1); total[S] (may be NULL) = the length of each interval.  Every knot span is integrated by an 8-point Gauss-Legendre rule
 * (|X'| is not a polynomial: the rule degrades where the speed passes through zero inside a span), the spans are summed in their order
 * without atomics: the same bits on every run, and total[s] is dist at the interval's end to the bit. */
int mvus_spline_length(int32_t device, int32_t S, const double* interval, const int64_t* knot_offsets, const double* knots,
                       const double* coefs, int64_t nt, const double* t, double* dist, int32_t* which, double* total);

/* Least-squares cubic spline on a FIXED knot vector (num_knots = n + 4, first/last four equal): coefs[3*n] (cx cy cz)
 * minimising sum_i |X(t_i) - X_i|^2 over the m data points t[m], X[3*m] (x(m) y(m) z(m)), t inside [knots[3], knots[n]].
 * The coefficient refit of Scene.traj_to_spline (common.py:224-270) once FITPACK's adaptive search has placed the knots (that
 * search stays on the host); equals scipy.interpolate.make_lsq_spline.  MVUS_E_NUMERIC when the data do not
 * determine every coefficient (Schoenberg-Whitney violated: m < n, a coefficient without data, a pivot of the normal equations
 * below 1e-12 of its diagonal entry). */
int mvus_spline_lsq(int32_t device, int32_t num_knots, const double* knots, int64_t m, const double* t, const double* X, double* coefs);

/* The smoothing-spline fit inside Scene.traj_to_spline (common.py:247, :267): scipy.interpolate.splprep(X, u=u, s=s, k=3), i.e.
 * FITPACK parcur / fppara with iopt = 0, unit weights, ub = u[0], ue = u[m-1], nest = m + 6.  u[m] strictly increasing, X[3*m]
 * (x(m) y(m) z(m)), s > 0.  Outputs: *n_out knots in t_out (room for m + 6), the n - 4 coefficients of dimension d at
 * c_out[d * (m + 6) + j] (room for 3 * (m + 6)), *fp_out = the weighted residual sum of squares, *ier_out = FITPACK's ier
 * (0 smoothing spline, -1 interpolating spline, -2 least-squares polynomial, 1..3 its warnings).  FITPACK's knot search
 * (fpknot), root finding (fprati) and discontinuity jumps (fpdisc) are followed line by line; the least-squares problems are
 * solved through banded normal equations on the device instead of row-wise Givens rotations -- same knots, coefficients to
 * ~1e-9 relative on the fixtures (tests/test_traj_to_spline.py), and O(m + n) per pass where FITPACK's smoothing iteration is
 * O(n^2).  The smooth_factor loop around it (common.py:241-262) is mvus_amd.spline.traj_fit.  Stateless; no CPU fallback. */
int mvus_spline_smooth(int32_t device, int64_t m, const double* u, const double* X, double s, int32_t* n_out, double* t_out, double* c_out,
                       double* fp_out, int32_t* ier_out);

/* The same fit as a session: the samples are checked and uploaded once, the work arrays stay allocated, and every call of
 * mvus_spline_fit_smooth is one splprep(X, u=u, s=s, k=3) on them -- Scene.traj_to_spline's smooth_factor loop
 * (common.py:241-262) calls splprep about a dozen times on the same part with s doubled or divided by 1.5.  Same results
 * as mvus_spline_smooth (which is open + smooth + close).  t_out[m + 6], c_out[3][m + 6] as there. */
typedef struct mvus_spline_fit mvus_spline_fit;
int mvus_spline_fit_open(int32_t device, int64_t m, const double* u, const double* X, mvus_spline_fit** out);
int mvus_spline_fit_smooth(mvus_spline_fit* fit, double s, int32_t* n_out, double* t_out, double* c_out, double* fp_out, int32_t* ier_out);
void mvus_spline_fit_close(mvus_spline_fit* fit);

/* The same fit with splprep's w: scipy.interpolate.splprep(X, w=w, u=u, s=s, k=3), one weight per sample (the reference never passes
 * one; Scene.traj_to_spline does when settings['traj_weights'] is set, with w ~ 1 / sigma of the triangulated point).  fppara reads w in two
 * places and so does the fit: the row of sample i in the least-squares system is w_i h with right-hand side w_i X_i (k_fit_blocks_w), and its
 * residual is |w_i (s(u_i) - X_i)|^2 (k_fit_residual_w), which is what the knot search, *fp_out and the comparison with s see.  The knot search
 * itself, fpdisc, fprati, the penalty and both band solvers are those of the unweighted fit; so is the double-double escalation, with two
 * additions for weighted fits: double-double from the pass on with more than half as many coefficients as samples (2 ncoef > m), and in
 * those passes *fp of a least-squares pass from its factorisation (|w x|^2 - |y|^2, as fppara forms it) instead of from coefficients
 * rounded to fp64.  Such a pass solves its system in one chain of ncoef rows, 4.8 us a row: 1.6 ms at 340 coefficients, 17 ms at 3 600;
 * fits of oversampled trajectories (a few hundred knots for 1e5 samples) never get there and keep the partitioned solver.  w[m] finite and
 * strictly positive (scipy's condition), else MVUS_E_INVALID.  w == NULL: the unweighted session / fit, bit for bit, on the unweighted
 * kernels.  mvus_spline_fit_smooth and mvus_spline_fit_close serve both kinds of session.
 * Not offered: a 3x3 weight per sample (FITPACK's w is one scalar per sample), and weights in the fallback for parts of fewer than four
 * samples (mvus_amd.spline.linear_fit_as_cubic, a host restatement). */
int mvus_spline_fit_open_w(int32_t device, int64_t m, const double* u, const double* X, const double* w, mvus_spline_fit** out);
int mvus_spline_smooth_w(int32_t device, int64_t m, const double* u, const double* X, const double* w, double s, int32_t* n_out, double* t_out,
                         double* c_out, double* fp_out, int32_t* ier_out);

/* The banded solvers of that fit on a system handed in: inspection hooks for k_band_solve, k_band_solve_parts and k_band_diag_sum
 * (spline_fit.hip.h), as mvus_ba_lm_step is for the Schur chain.  No reference counterpart.
 *   G5[5*n], BtB[5*n]: the kernels' lower-band layout, M(j, j - w) at 5 j + w, w = 0..4; entries with j - w < 0 must be 0.
 *   rhs[3*n], c_out[3*n]: column d at d * n + j.
 *   G5_lo, BtB_lo, rhs_lo: NULL, or the low words of the operands; read only when precise != 0, where the kernels run in
 *   double-double on dd(hi, lo).  precise == 0: fp64 on the high words.
 *   hb == 3: solves G5 x = rhs as a least-squares pass does (G5's w = 4 column is not read); BtB, BtB_lo must be NULL.
 *   hb == 4: solves (G5 + pinv^2 BtB) x = rhs as a smoothing pass does, through the same combine kernel.
 *   parts == -1: one chain (k_band_solve).  parts == 0: the fit's own rule (from 192 rows on: about sqrt(n / 2.5) interiors,
 *   k_band_solve_parts).  parts >= 2: exactly that many interiors.  *P_out = the number of interiors used (1: one chain).
 *   stats_out[4] = what the kernel leaves in out[0..3]: [0] the sum of diag(L) (NaN from the partitioned kernel, which does not form
 *   it), [1] NaN, [2], [3] the smallest and largest Cholesky pivot (square roots) in the kernel's own elimination order.
 *   *fail_out = 1 when a pivot fell below 1e-12 (fp64) / 1e-24 (double-double) of its diagonal entry and was floored.
 * The work arrays are sized by the fit's own rule for exactly n coefficients.  MVUS_E_INVALID, before any launch: n < 4, hb not 3 or 4, a NULL pointer
 * other than the _lo ones, BtB with hb == 3, no BtB or a non-finite pinv with hb == 4, parts < -1 or 1, parts > 256 or an interior
 * shorter than 2 hb rows ((n - (parts - 1) hb) / parts < 2 hb).  Stateless; no CPU fallback. */
int mvus_spline_band_solve(int32_t device, int32_t n, int32_t hb, int32_t precise, int32_t parts, const double* G5, const double* G5_lo,
                           const double* BtB, const double* BtB_lo, double pinv, const double* rhs, const double* rhs_lo, double* c_out,
                           double* stats_out, int32_t* fail_out, int32_t* P_out);
/* out[0] = the sum of diag(L) of G5 = L L^T (hb = 3) in the natural order, by k_band_diag_sum: fppara's initial p after a partitioned
 * pass.  Arguments as above.  MVUS_E_INVALID: n < 4, G5 or out NULL. */
int mvus_spline_band_diag_sum(int32_t device, int32_t n, int32_t precise, const double* G5, const double* G5_lo, double* out);

/* The passes of that fit before and after its banded solve, on samples, knots and coefficients handed in: inspection hooks for k_fit_basis,
 * k_fit_first, k_fit_blocks, k_fit_slice_sum, k_fit_band, k_fit_penalty, k_fit_residual, k_fit_total_partial / k_fit_total and k_fit_fpint /
 * k_fit_fpint_final (spline_fit.hip.h), with the fit's own launches and work-array sizes for exactly these n knots.  No reference
 * counterpart.  u[m], X[3*m] as in mvus_spline_smooth; t[n] a cubic knot vector on them; ncoef = n - 4 coefficients, nspan = n - 7 spans.
 *   slices == 0: a span's samples are cut into the fit's own number of slices (fit_slices(nspan)); slices >= 1: exactly that many.
 *   precise, parts, the _lo words, stats_out[4] and *fail_out: as in mvus_spline_band_solve (hb = 3).
 * mvus_spline_fit_normal, one least-squares pass: span_out[m] (the span of every sample, 0-based), q_out[4*m] (its four B-splines),
 *   first_out[nspan + 1] (the first sample of every span, first[nspan] = m), G5_out / G5_lo_out[5*ncoef] and rhs_out / rhs_lo_out[3*ncoef]
 *   (the normal equations as the solver reads them; the _lo outputs may be NULL), c_out[3*ncoef] (their solution).
 * mvus_spline_fit_penalty: BtB_out / BtB_lo_out[5*ncoef] = B^T B of the n8 x ncoef jump matrix b[5*n8] (fpdisc's layout: row it holds
 *   columns it .. it + 4), by k_fit_penalty alone.
 * mvus_spline_fit_residual: term_out[m] = |s(u_i) - X_i|^2 for the coefficients c[3*ncoef], *fp_out their total, fpint_out[nspan] the
 *   per-span sums with FITPACK's half / half rule for the sample that opens a span.
 * MVUS_E_INVALID, before any launch: a NULL pointer other than the _lo ones; m <= 3; u not strictly increasing; a non-finite input;
 * n < 8 or n > m + 4; boundary knots other than u[0] / u[m-1] four times each; interior knots not strictly increasing inside
 * (u[0], u[m-1]); a span without a sample; slices < 0, > 256, nspan (slices - 1) > 1536 or nspan slices > 2048 (what the fit's slice
 * arrays hold); parts as in mvus_spline_band_solve; for the penalty, n8 < 1 or n8 > ncoef - 4.  Stateless; no CPU fallback. */
int mvus_spline_fit_normal(int32_t device, int64_t m, const double* u, const double* X, int32_t n, const double* t, int32_t precise, int32_t slices,
                           int32_t parts, int32_t* span_out, double* q_out, int64_t* first_out, double* G5_out, double* G5_lo_out, double* rhs_out,
                           double* rhs_lo_out, double* c_out, double* stats_out, int32_t* fail_out);
int mvus_spline_fit_penalty(int32_t device, int32_t ncoef, int32_t n8, const double* b, int32_t precise, double* BtB_out, double* BtB_lo_out);
int mvus_spline_fit_residual(int32_t device, int64_t m, const double* u, const double* X, int32_t n, const double* t, const double* c, int32_t slices,
                             double* term_out, double* fp_out, double* fpint_out);
/* The same two passes of a weighted fit (mvus_spline_fit_open_w), w[m] after X: the normal equations of the rows w_i h with right-hand sides
 * w_i X_i (k_fit_blocks_w; q_out stays the unweighted basis, as FITPACK stores it), and term_out[m] = |w_i (s(u_i) - X_i)|^2 (k_fit_residual_w).
 * w == NULL: the calls above, bit for bit.  MVUS_E_INVALID also for a weight that is not finite or not > 0. */
int mvus_spline_fit_normal_w(int32_t device, int64_t m, const double* u, const double* X, const double* w, int32_t n, const double* t, int32_t precise,
                             int32_t slices, int32_t parts, int32_t* span_out, double* q_out, int64_t* first_out, double* G5_out, double* G5_lo_out,
                             double* rhs_out, double* rhs_lo_out, double* c_out, double* stats_out, int32_t* fail_out);
int mvus_spline_fit_residual_w(int32_t device, int64_t m, const double* u, const double* X, const double* w, int32_t n, const double* t, const double* c,
                               int32_t slices, double* term_out, double* fp_out, double* fpint_out);

/* Scene.get_camera_pose's cv2.solvePnPRansac(objectPoints, imagePoints, K, d, reprojectionError=error) (common.py:744; OpenCV is
 * a third-party dependency absent from this image: parity unpinned, see pnp.hip.h).  X[3*N] object points (x(N) y(N) z(N)),
 * uv[2*N] raw pixels (u(N) v(N)), K = fx fy cx cy, d = k1 k2 p1 p2 k3.  `iterations` hypotheses (OpenCV's iterationsCount,
 * default 100) from six sampled points each (counter-based sampling from `seed`: deterministic), scored by the number of points
 * with reprojection error <= reproj_error pixels; the best pose is refined on its inliers by damped Gauss-Newton on the pixel
 * reprojection error (OpenCV's SOLVEPNP_ITERATIVE refinement minimises the same quantity).  Outputs: rvec[3], tvec[3]
 * (cv2.Rodrigues convention), inliers[N] (1 = inlier of the best hypothesis; may be NULL), *n_inliers.
 * MVUS_E_NUMERIC when no hypothesis is supported by six points.  Stateless; no CPU fallback. */
int mvus_pnp_ransac(int32_t device, int64_t N, const double* X, const double* uv, const double* K, const double* d, double reproj_error,
                    int32_t iterations, uint64_t seed, double* rvec, double* tvec, uint8_t* inliers, int64_t* n_inliers);

/* cv2.findFundamentalMat(p1, p2, FM_RANSAC, thresh) (Scene.init_traj, common.py:193; synchronization.sync_bf, once per candidate
 * time shift) for P independent problems in one call (epipolar.hip.h; OpenCV is absent from this image: parity unpinned).
 * Problem p holds the pairs offsets[p] .. offsets[p+1]-1 of x1[2*Ntot], x2[2*Ntot] (u(Ntot) then v(Ntot); Ntot = offsets[P]),
 * at least 8 of them.  `iterations` 7-point hypotheses per problem (OpenCV 4: at most 1000 at confidence 0.99; all are
 * evaluated), drawn from `seed` by a counter-based sampler that depends only on (seed, hypothesis, problem size): a batched call
 * and single calls give the same bits.  Score: pairs whose larger squared point-to-epipolar-line distance is <= thresh^2; the
 * best model (ties: the lowest index) is refitted by the normalised 8-point algorithm on its inliers and the refit kept when it
 * has at least as many inliers.  Outputs: F_out[9*P] (row-major, unit Frobenius norm, F[2][2] >= 0), mask[Ntot] (1 = inlier),
 * n_inliers[P] (may be NULL).  MVUS_E_INVALID: fewer than 8 pairs in a problem, non-finite input, thresh <= 0, iterations outside
 * 1..65536.  MVUS_E_NUMERIC: a problem has no valid 7-point model.  Stateless; no CPU fallback. */
int mvus_fundamental_ransac(int32_t device, int32_t P, const int64_t* offsets, const double* x1, const double* x2, double thresh,
                            int32_t iterations, uint64_t seed, double* F_out, uint8_t* mask, int32_t* n_inliers);

/* cv2.correctMatches(F, p1, p2) (Scene.init_traj, common.py:206): the Hartley-Sturm optimal correction of N pairs under F[9]
 * (row-major), x1[2*N], x2[2*N] -> x1c[2*N], x2c[2*N] in the same layout.  A pair with a non-finite coordinate comes back as
 * NaN; no other pair does.  MVUS_E_INVALID: F not finite or zero.  Stateless; no CPU fallback. */
int mvus_correct_matches(int32_t device, int64_t N, const double* F, const double* x1, const double* x2, double* x1c, double* x2c);

/* epipolar.triangulate_from_E (epipolar.py:568-588) on normalised coordinates x1n[2*N], x2n[2*N] (K^-1 x, u(N) then v(N)):
 * E[9] (row-major) decomposed into the four (R, t) of compute_Rt_from_E, each scored by sum(d1 > 0) + sum(d2 > 0) over the
 * pairs triangulated with P1 = [I|0]; the first candidate to exceed the running maximum wins.  Outputs: P2_out[12] = [R|t]
 * row-major, X_out[4*N] (x(N) y(N) z(N) w(N), w = 1) triangulated with it.  MVUS_E_INVALID: N < 1 or non-finite input.
 * MVUS_E_NUMERIC: no candidate puts any point in front of a camera.  Stateless; no CPU fallback. */
int mvus_pose_from_essential(int32_t device, int64_t N, const double* E, const double* x1n, const double* x2n, double* P2_out, double* X_out);

/* The iterative time-shift search of Albl et al. as the reference runs it (synchronization.py:13-130, "sync_method": "iter") for one
 * camera pair (sync_iter.hip.h; synchronization.sync_iter_gpu drives it).  The session is opaque.  open uploads, once: both cameras'
 * interpolating cubic splines in FITPACK form (n coefficients per coordinate, knots[n + 4], coef = x[n] then y[n]; camera 1 on its
 * timeline t / alpha, camera 2 on its OWN unshifted timeline), camera 2's contiguous intervals as K [start, end) pairs
 * (util.find_intervals), camera 1's detections detect1[3 * N1] (t(N1) x(N1) y(N1), t ascending) and camera 2's timestamps t2[N2].
 * `shift` below is the current estimate of beta: camera 2's samples lie at t2 + shift on camera 1's timeline.
 *
 * round: both signs of d in one sequence of launches with one synchronisation.  Per sign H hypotheses of nine samples drawn below
 * min(N1, N2) - 2 |d| by a counter-based sampler (seed, round, sign, hypothesis): the finite real eigenvalues beta of the pencil
 * A1 + beta A2 (up to six), per beta the normalised 8-point fundamental matrix of (s1, s2 + beta ds) and the model (F, beta d),
 * scored over all of camera 1's detections: tau = t1 - shift + beta d, overlap when start <= tau < end for an interval, inlier when
 * the squared Sampson error (epipolar.py:258-265, pixels) of (detection, S2(tau)) is < threshold.  ratio = inliers / overlap; the
 * highest wins with strict >, in (hypothesis, slot) order, from 0; overlap 0 is skipped.  out[8]: for +d then -d the winner's
 * -beta d (the reference's -result[-1]), its ratio, inliers, overlap (zeros without a winner).
 * models (an inspection hook, like mvus_ba_lm_step): one sign -- d carries it -- with explicit sample indices idx[9 * H] into t2;
 * betas[6 * H] ascending per hypothesis, valid[6 * H], F[9 * 6 * H] (row-major, unit norm, F[2][2] >= 0, x2^T F x1 = 0; zeros for
 * an empty slot) and counts[2 * 6 * H] (inliers, overlap per model).  A hypothesis with a repeated timestamp, a non-finite sample
 * or a degenerate one has no valid slot.
 * score: counts[2 * M] of M models handed in, models[11 * M] = F (9), beta d, valid flag; a model that is not finite counts 0, 0.
 * MVUS_E_INVALID: bad arguments, fewer than nine samples to draw from (nothing is launched), an index outside t2.  No CPU
 * fallback. */
typedef struct mvus_sync_iter mvus_sync_iter;
int mvus_sync_iter_open(int32_t device, int32_t n1, const double* knots1, const double* coef1, int32_t n2, const double* knots2, const double* coef2,
                        int32_t K, const double* intervals2, int64_t N1, const double* detect1, int64_t N2, const double* t2, mvus_sync_iter** out);
void mvus_sync_iter_close(mvus_sync_iter* session);
int mvus_sync_iter_round(mvus_sync_iter* session, double shift, int32_t d, int32_t H, double threshold, uint64_t seed, int32_t round, double* out);
int mvus_sync_iter_models(mvus_sync_iter* session, double shift, int32_t d, int32_t H, const int64_t* idx, double threshold, double* betas,
                          uint8_t* valid, double* F, int32_t* counts);
int mvus_sync_iter_score(mvus_sync_iter* session, double shift, int64_t M, const double* models, double threshold, int32_t* counts);

#ifdef __cplusplus
}
#endif
#endif /* MVUS_BA_H */
