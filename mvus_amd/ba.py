"""Python face of the C ABI (include/mvus_ba.h): one ``BAHandle`` per BA problem, GPU and stream.

``BAHandle.solve`` stands where the reference calls ``scipy.optimize.least_squares``
(``reconstruction/common.py:670``); ``residual`` is ``error_BA`` (``common.py:448-487``);
``outlier_mask`` is the test of ``Scene.remove_outliers`` (``common.py:709-713``).
Everything is computed by libmvusba.so on the GPU; there is no CPU fallback.
"""
import ctypes
import sys
from types import SimpleNamespace

import numpy as np

from . import _lib
from ._lib import JAC_ANALYTIC, JAC_FD, JAC_PATTERN, SOLVER_LM_SCHUR, SOLVER_TRF_LSMR  # noqa: F401 (re-exported)
from ._lib import LOSS_ARCTAN, LOSS_CAUCHY, LOSS_HUBER, LOSS_LINEAR, LOSS_NAMES, LOSS_SOFT_L1  # noqa: F401 (re-exported)


def loss_code(loss):
    """'linear' | 'soft_l1' | 'huber' | 'cauchy' | 'arctan' (scipy's names) or an integer MVUS_LOSS_* code -> the code.  An unknown
    NAME raises ValueError here; an unknown integer is left to the library (MVUS_E_INVALID)."""
    if isinstance(loss, str):
        if loss not in LOSS_NAMES:
            raise ValueError('unknown loss %r: one of %s' % (loss, ', '.join(sorted(LOSS_NAMES))))
        return LOSS_NAMES[loss]
    return int(loss)


def _weights(sigma, rows, K, what):
    """sigma as a scalar, per axis (rows,) or per axis and element (rows, K) -> contiguous (rows, K) weights 1 / sigma, 0 for an infinite sigma."""
    s = np.asarray(sigma, dtype=np.float64)
    if s.ndim == 1 and s.shape == (rows,):
        s = s[:, None]
    elif s.ndim not in (0, 2) or (s.ndim == 2 and s.shape != (rows, K)):
        raise ValueError('%s: sigma has shape %s, expected a scalar, (%d,) or (%d, %d)' % (what, s.shape, rows, rows, K))
    s = np.broadcast_to(s, (rows, K))
    if np.any(np.isnan(s)) or np.any(s <= 0):
        raise ValueError('%s: sigma must be positive (np.inf leaves an axis out)' % what)
    with np.errstate(divide='ignore'):
        return np.ascontiguousarray(np.where(np.isinf(s), 0.0, 1.0 / s))


def position_prior_arrays(t, P, sigma):
    """(t (K,), P (3, K), sigma scalar | (3,) | (3, K)) -> contiguous float64 (t, P, w) with w = 1 / sigma (0 for an infinite sigma).
    Shapes, NaN and non-positive sigma raise ValueError here; the library checks the numbers again."""
    t = np.ascontiguousarray(t, dtype=np.float64).ravel()
    P = np.ascontiguousarray(P, dtype=np.float64)
    if P.shape != (3, t.size):
        raise ValueError('position priors: P has shape %s, expected (3, %d)' % (P.shape, t.size))
    return t, P, _weights(sigma, 3, t.size, 'position priors')


def landmark_arrays(X, cam, point, uv, sigma):
    """(X (3, L), cam (K,), point (K,), uv (2, K), sigma scalar | (2,) | (2, K)) -> contiguous (X, cam int32, point int32, uv, w) with
    w = 1 / sigma (0 for an infinite sigma).  Shapes, NaN and non-positive sigma raise ValueError here; the library checks the numbers
    and the index ranges again."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    if X.ndim != 2 or X.shape[0] != 3:
        raise ValueError('landmarks: X has shape %s, expected (3, L)' % (X.shape,))
    cam = np.ascontiguousarray(np.asarray(cam).ravel(), dtype=np.int32)
    point = np.ascontiguousarray(np.asarray(point).ravel(), dtype=np.int32)
    K = cam.size
    uv = np.ascontiguousarray(uv, dtype=np.float64)
    if point.size != K or uv.shape != (2, K):
        raise ValueError('landmarks: cam (%d,), point (%d,) and uv %s do not describe the same K observations' % (K, point.size, uv.shape))
    return X, cam, point, uv, _weights(sigma, 2, K, 'landmarks')


class UnsupportedBySolver(RuntimeError):
    """MVUS_E_UNSUPPORTED: the problem is outside what the chosen solver handles (see include/mvus_ba.h); the other solver has no such limit."""


class ReshardNeeded(RuntimeError):
    """MVUS_E_RESHARD: on a time shard the time stamps have drifted until a row reaches control points outside the slice.  ``x`` is the
    point the solver had reached, ``nfev`` the evaluations it used: re-cut there and continue (mvus_amd.dist.solve_time_sharded)."""
    x = None
    nfev = 0


_ERRORS = {_lib.MVUS_E_INVALID: ValueError, _lib.MVUS_E_NUMERIC: ValueError, _lib.MVUS_E_HIP: RuntimeError,
           _lib.MVUS_E_COMM: RuntimeError, _lib.MVUS_E_UNSUPPORTED: UnsupportedBySolver}


class _Result(SimpleNamespace):
    """OptimizeResult-like; ``active_mask`` (all zeros: the rs box is handled by projection) is built on first use."""

    @property
    def active_mask(self):
        return np.zeros(self.x.shape[0])


class BAHandle:
    # in force on the handle: what set_loss / set_frozen / set_position_priors / set_landmarks last sent and the library accepted
    loss, _frozen, _position_priors, _landmarks = (LOSS_LINEAR, 1.0), None, None, None
    _KEEP = object()                   # configure: "leave this as it is" (None already means "clear")

    def __init__(self, prob, device=0, stream=None):
        self.lib = _lib.load()
        self.prob = prob
        self._struct, self._keep = _lib.make_problem_struct(prob, device=device, stream=stream)
        h = ctypes.c_void_p()
        rc = self.lib.mvus_ba_create(ctypes.byref(self._struct), ctypes.byref(h))
        if rc != 0:
            raise _ERRORS.get(rc, RuntimeError)('mvus_ba_create: ' + self.lib.mvus_last_error(None).decode())
        self.h = h
        self.n = int(self.lib.mvus_ba_num_params(h))
        self.m = int(self.lib.mvus_ba_num_residuals(h))
        self.T = int(self.lib.mvus_ba_num_motion_rows(h))
        self.NS = int(self.lib.mvus_ba_num_slots(h))
        self.M = prob.M
        self._cb = None

    def close(self):
        if getattr(self, 'h', None):
            self.lib.mvus_ba_destroy(self.h)
            self.h = None

    def __del__(self):
        # not while the interpreter shuts down: modules (and torch's own HIP state) are torn down in no particular order then, and
        # a handle that dies with the process needs no hipFree -- one GPU-suite run in eleven ended with a fatal signal after its
        # summary line before this guard
        if sys is None or sys.is_finalizing():       # (module globals are already gone late in the shutdown)
            return
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, rc, what):
        if rc != 0:
            raise _ERRORS.get(rc, RuntimeError)('%s: %s' % (what, self.lib.mvus_last_error(self.h).decode()))

    @staticmethod
    def _x(x, n):
        x = np.ascontiguousarray(x, dtype=np.float64)
        if x.shape != (n,):
            raise ValueError('x has shape %s, expected (%d,)' % (x.shape, n))
        return x

    def residual(self, x):
        x = self._x(x, self.n)
        f = np.empty(self.m)
        self._check(self.lib.mvus_ba_residual(self.h, _lib.dptr(x), _lib.dptr(f)), 'mvus_ba_residual')
        return f

    def residual_jacobian(self, x, jac_mode=JAC_ANALYTIC):
        """f[m], J[2, NS, M] (slot layout of include/mvus_ba.h), ctrl[M]."""
        x = self._x(x, self.n)
        f = np.empty(self.m)
        J = np.empty((2, self.NS, self.M))
        ctrl = np.empty(self.M, dtype=np.int32)
        self._check(self.lib.mvus_ba_residual_jacobian(self.h, _lib.dptr(x), jac_mode, _lib.dptr(f), _lib.dptr(J),
                                                       ctrl.ctypes.data_as(_lib.c_int32_p)), 'mvus_ba_residual_jacobian')
        return f, J, ctrl

    def motion_rows(self, x, jac_mode=JAC_ANALYTIC):
        x = self._x(x, self.n)
        mf = np.zeros(self.T)
        mJ = np.zeros((36, self.T))
        mctrl = np.full((3, self.T), -1, dtype=np.int32)
        self._check(self.lib.mvus_ba_motion_rows(self.h, _lib.dptr(x), jac_mode, _lib.dptr(mf), _lib.dptr(mJ),
                                                 mctrl.ctypes.data_as(_lib.c_int32_p)), 'mvus_ba_motion_rows')
        return mf, mJ, mctrl

    def set_pattern(self, x0, download=True):
        """Canonical pattern codes of the detection rows at x0, computed on the GPU (tie rows carry ``_lib.PAT_TIE``);
        ``download=False`` leaves them on the device only."""
        x0 = self._x(x0, self.n)
        pat = np.empty(self.M, dtype=np.int32) if download else None
        self._check(self.lib.mvus_ba_set_pattern(self.h, _lib.dptr(x0), pat.ctypes.data_as(_lib.c_int32_p) if download else None), 'mvus_ba_set_pattern')
        self._pattern_fixed = False      # (a pattern computed on the device is re-computed at the x0 of every JAC_PATTERN solve)
        return pat

    def motion_pattern(self):
        mp = np.empty(self.T, dtype=np.int32)
        self._check(self.lib.mvus_ba_motion_pattern(self.h, mp.ctypes.data_as(_lib.c_int32_p)), 'mvus_ba_motion_pattern')
        return mp

    def upload_pattern(self, pat, motion_pat=None):
        """Supply the pattern (codes of include/mvus_ba.h) instead of the GPU's canonical one -- the reference's matrix is
        an input of the call this library replaces (common.py:670)."""
        pat = np.ascontiguousarray(pat, dtype=np.int32)
        if pat.shape != (self.M,):
            raise ValueError('pat has shape %s, expected (%d,)' % (pat.shape, self.M))
        mp = None
        if motion_pat is not None and self.T:
            mp = np.ascontiguousarray(motion_pat, dtype=np.int32)
            if mp.shape != (self.T,):
                raise ValueError('motion_pat has shape %s, expected (%d,)' % (mp.shape, self.T))
        self._check(self.lib.mvus_ba_upload_pattern(self.h, pat.ctypes.data_as(_lib.c_int32_p),
                                                    mp.ctypes.data_as(_lib.c_int32_p) if mp is not None else None), 'mvus_ba_upload_pattern')
        self._pattern_fixed = True       # an uploaded pattern stays in force over every solve that follows (mvus_ba_solve keeps it)

    def set_deterministic(self, on=True):
        """Kept for the ABI: the LM + Schur assembly is window-major (one writer and one order per entry, no atomics) -- the same
        bits on every run whatever is set here."""
        self._check(self.lib.mvus_ba_set_deterministic(self.h, 1 if on else 0), 'mvus_ba_set_deterministic')

    def deterministic_fallback(self):
        """True when the last assembly went through the detection-major kernel with fp64 atomics (frames of a camera out of order,
        or normal equations formed from a stored non-analytic Jacobian): correct, not bit-reproducible."""
        v = ctypes.c_int32(0)
        self._check(self.lib.mvus_ba_deterministic_fallback(self.h, ctypes.byref(v)), 'mvus_ba_deterministic_fallback')
        return bool(v.value)

    def set_fd_groups(self, groups, num_groups):
        groups = np.ascontiguousarray(groups, dtype=np.int32)
        if groups.shape != (self.n,):
            raise ValueError('groups has shape %s, expected (%d,)' % (groups.shape, self.n))
        self._check(self.lib.mvus_ba_set_fd_groups(self.h, groups.ctypes.data_as(_lib.c_int32_p), int(num_groups)),
                    'mvus_ba_set_fd_groups')

    def prepare_pattern(self, x0, ties='numpy', matrix=None):
        """The reference pattern at x0 in force on the handle: canonical codes from the GPU, the twin rows decided
        by ``ties`` ('numpy': like np.argsort of this process, what the reference would build here; 'canonical': the
        library's choice), or -- ``matrix`` -- the codes a given reference matrix implies.  Returns (pat, motion_pat)."""
        from . import pattern
        if matrix is not None:
            pat, mpat = pattern.codes_from_matrix(self.prob, matrix)
        else:
            pat, mpat = pattern.resolve_ties(self.prob, x0, self.set_pattern(x0), self.motion_pattern() if self.T else None, how=ties)
        self.upload_pattern(pat, mpat if self.T else None)
        return pat, (mpat if self.T else None)

    def prepare_fd(self, x0, ties='numpy', matrix=None):
        """Set-up for JAC_FD at x0: the reference pattern (see prepare_pattern), scipy's column grouping on the host."""
        from . import pattern
        pat, mpat = self.prepare_pattern(x0, ties, matrix)
        groups, ng = pattern.fd_groups(self.prob, pat, mpat)
        self.set_fd_groups(groups, ng)
        return ng

    def jv(self, v):
        v = self._x(v, self.n)
        y = np.empty(self.m)
        self._check(self.lib.mvus_ba_jv(self.h, _lib.dptr(v), _lib.dptr(y)), 'mvus_ba_jv')
        return y

    def jtu(self, u):
        u = self._x(u, self.m)
        z = np.empty(self.n)
        self._check(self.lib.mvus_ba_jtu(self.h, _lib.dptr(u), _lib.dptr(z)), 'mvus_ba_jtu')
        return z

    def normal_equations(self):
        """g[n], JtJ_cam[C,B,B], band[N,W,3,3], cross[C,B,3N] of the Jacobian currently held."""
        C, B, N = self.prob.C, 3 + self.prob.P, int(self.prob.n_coef.sum())
        W = ctypes.c_int32(0)
        self._check(self.lib.mvus_ba_normal_equations(self.h, None, None, None, None, ctypes.byref(W)), 'mvus_ba_normal_equations')
        g = np.empty(self.n)
        cam = np.empty((C, B, B))
        band = np.empty((N, W.value, 3, 3))
        cross = np.empty((C, B, 3 * N))
        self._check(self.lib.mvus_ba_normal_equations(self.h, _lib.dptr(g), _lib.dptr(cam), _lib.dptr(band), _lib.dptr(cross),
                                                      ctypes.byref(W)), 'mvus_ba_normal_equations')
        return g, cam, band, cross

    def lm_step(self, lam):
        """p = -(J^T J + lam diag(J^T J))^-1 J^T f for the Jacobian / residual currently held (after residual_jacobian)."""
        p = np.empty(self.n)
        self._check(self.lib.mvus_ba_lm_step(self.h, float(lam), _lib.dptr(p)), 'mvus_ba_lm_step')
        return p

    def lsmr(self, b, D=None, E=None, damp=0.0, atol=1e-6, btol=1e-6, conlim=1e8, maxiter=0):
        """LSMR on A = [J diag(D); diag(E)] with right-hand side [b; 0] for the Jacobian currently held (after residual_jacobian): the linear
        solve of the TRF + LSMR solver on its own (mvus_ba_lsmr), by the loop the handle's switches select.  Returns a namespace
        (x, itn, istop, normr, normar, normA, condA).  Changes nothing a later solve sees."""
        b = self._x(b, self.m)
        D = self._x(D, self.n) if D is not None else None
        E = self._x(E, self.n) if E is not None else None
        x = np.empty(self.n)
        itn, istop = ctypes.c_int32(0), ctypes.c_int32(0)
        norms = np.zeros(4)
        self._check(self.lib.mvus_ba_lsmr(self.h, _lib.dptr(b), _lib.dptr(D) if D is not None else None, _lib.dptr(E) if E is not None else None,
                                          float(damp), float(atol), float(btol), float(conlim), int(maxiter), _lib.dptr(x),
                                          ctypes.byref(itn), ctypes.byref(istop), _lib.dptr(norms)), 'mvus_ba_lsmr')
        return SimpleNamespace(x=x, itn=itn.value, istop=istop.value, normr=norms[0], normar=norms[1], normA=norms[2], condA=norms[3])

    def set_loss(self, loss, f_scale=1.0):
        """least_squares(loss=, f_scale=): the robust loss of every later solve / normal_equations / lm_step on the handle (LM + Schur,
        analytic Jacobian, one rank).  residual, residual_jacobian, jv, jtu and the outlier masks stay those of error_BA."""
        code = loss_code(loss)
        self._check(self.lib.mvus_ba_set_loss(self.h, code, float(f_scale)), 'mvus_ba_set_loss')
        self.loss = (code, float(f_scale))

    def set_frozen(self, mask):
        """Hold camera-side unknowns constant (mvus_ba_set_frozen): ``mask[k]`` true keeps ``x[k]`` where it is, k over the head of x in
        pack_x order -- alpha(C), beta(C), rs(C), then P parameters per camera -- so ``mask`` has C * (3 + P) entries.  ``None`` (or an
        empty mask) clears it.  In force for every later solve / normal_equations / lm_step on the handle, kept over remove_outliers;
        residual, residual_jacobian, jv, jtu and the outlier masks stay those of error_BA."""
        if mask is None or np.size(mask) == 0:
            self._check(self.lib.mvus_ba_set_frozen(self.h, None, 0), 'mvus_ba_set_frozen')
            self._frozen = None
            return
        m = np.asarray(mask)
        if m.dtype != np.bool_ and m.dtype != np.uint8:
            if not np.all((m == 0) | (m == 1)):
                raise ValueError('set_frozen: the mask holds values other than 0 and 1')
        m = np.ascontiguousarray(m, dtype=np.uint8).ravel()
        self._check(self.lib.mvus_ba_set_frozen(self.h, m.ctypes.data_as(_lib.c_uint8_p), m.size), 'mvus_ba_set_frozen')
        self._frozen = m.astype(bool) if m.any() else None

    @property
    def frozen(self):
        """The mask in force (bool[C * (3 + P)], a copy), or None without one."""
        if int(self.lib.mvus_ba_num_frozen(self.h)) == 0:
            return None
        return self._frozen.copy()

    @property
    def num_frozen(self):
        return int(self.lib.mvus_ba_num_frozen(self.h))

    def set_position_priors(self, t, P, sigma):
        """Surveyed positions as observations (mvus_ba_set_position_priors): ``t`` (K,) on the spline's timeline, ``P`` (3, K), ``sigma`` the
        1-sigma of a position as a scalar, per axis (3,) or per prior and axis (3, K); ``np.inf`` leaves that axis out (weight 0).  Each
        prior adds the rows (S(t_k) - p_k) / sigma to every later LM solve / normal_equations / lm_step / covariance on the handle, kept
        over remove_outliers.  ``t = None`` (or K = 0) clears them.  Priors outside every interval of the spline are inactive."""
        if t is None or np.size(t) == 0:
            self._check(self.lib.mvus_ba_set_position_priors(self.h, 0, None, None, None), 'mvus_ba_set_position_priors')
            self._position_priors = None
            return
        tc, Pc, w = position_prior_arrays(t, P, sigma)
        self._check(self.lib.mvus_ba_set_position_priors(self.h, tc.size, _lib.dptr(tc), _lib.dptr(Pc), _lib.dptr(w)), 'mvus_ba_set_position_priors')
        self._position_priors = tuple(np.array(a, dtype=np.float64) for a in (t, P, sigma))

    position_priors = property(lambda self: self._position_priors, doc='(t, P, sigma) as last sent (copies), or None without priors')

    @property
    def num_position_priors(self):
        return int(self.lib.mvus_ba_num_position_priors(self.h, None))

    @property
    def num_active_position_priors(self):
        a = ctypes.c_int64(0)
        self.lib.mvus_ba_num_position_priors(self.h, ctypes.byref(a))
        return int(a.value)

    def position_prior_cost(self, x, rows=False):
        """0.5 sum r^2 of the position priors at x; with ``rows`` also r (3, K) in the order the priors were given, NaN for inactive ones."""
        x = self._x(x, self.n)
        cost = ctypes.c_double(0.0)
        r = np.empty((3, self.num_position_priors)) if rows else None
        self._check(self.lib.mvus_ba_position_prior_cost(self.h, _lib.dptr(x), ctypes.byref(cost), _lib.dptr(r) if rows else None),
                    'mvus_ba_position_prior_cost')
        return (cost.value, r) if rows else cost.value

    def set_landmarks(self, X, cam, point, uv, sigma):
        """Surveyed static points as observations (mvus_ba_set_landmarks): ``X`` (3, L) world points, observation k = camera ``cam[k]``
        (index on this handle) sees landmark ``point[k]`` at the raw pixel ``uv[:, k]``; ``sigma`` its 1-sigma in pixels as a scalar, per
        axis (2,) or per axis and observation (2, K); ``np.inf`` leaves that axis out (weight 0).  Each observation adds the rows
        (pi_c(X_l) - obs) / sigma to every later LM solve / normal_equations / lm_step / covariance on the handle, kept over
        remove_outliers.  ``X = None`` (or K = 0) clears them."""
        if X is None or cam is None or np.size(cam) == 0:
            self._check(self.lib.mvus_ba_set_landmarks(self.h, 0, None, 0, None, None, None, None), 'mvus_ba_set_landmarks')
            self._landmarks = None
            return
        Xc, camc, pointc, uvc, w = landmark_arrays(X, cam, point, uv, sigma)
        self._check(self.lib.mvus_ba_set_landmarks(self.h, Xc.shape[1], _lib.dptr(Xc), camc.size, camc.ctypes.data_as(_lib.c_int32_p),
                                                   pointc.ctypes.data_as(_lib.c_int32_p), _lib.dptr(uvc), _lib.dptr(w)), 'mvus_ba_set_landmarks')
        self._landmarks = tuple(np.array(a) for a in (X, cam, point, uv, sigma))

    landmarks = property(lambda self: self._landmarks, doc='(X, cam, point, uv, sigma) as last sent (copies), or None without landmarks')

    def configure(self, loss=_KEEP, frozen=_KEEP, position_priors=_KEEP, landmarks=_KEEP):
        """Make the state of the handle what is given -- ``loss`` (code, f_scale), ``frozen`` a mask, ``position_priors`` / ``landmarks`` the arguments of
        their ``set_*``; None clears the last three; what is not given is left alone.  A ``set_*`` is called only where the state differs: a
        redundant one would drop what the last LM solve carried over, a changed one resets the damping."""
        if loss is not self._KEEP and tuple(loss) != self.loss:
            self.set_loss(*loss)
        cur = self.frozen                      # (no mask and an all-false mask are the same state)
        if frozen is not self._KEEP and (np.any(frozen) if cur is None else frozen is None or not np.array_equal(frozen, cur)):
            self.set_frozen(frozen)
        for new, cur, setter in ((position_priors, self._position_priors, self.set_position_priors), (landmarks, self._landmarks, self.set_landmarks)):
            if new is None and cur is not None:
                setter(*[None] * len(cur))
            elif new is not None and new is not self._KEEP and not (cur is not None and all(np.array_equal(a, b) for a, b in zip(cur, new))):
                setter(*new)                   # (array_equal: the element counts first, then every number)

    @property
    def num_landmark_observations(self):
        return int(self.lib.mvus_ba_num_landmark_observations(self.h, None))

    @property
    def num_landmark_rows(self):
        a = ctypes.c_int64(0)
        self.lib.mvus_ba_num_landmark_observations(self.h, ctypes.byref(a))
        return int(a.value)

    def landmark_cost(self, x, rows=False):
        """0.5 sum r^2 of the landmark rows at x; with ``rows`` also r (2, K) in the order the observations were given."""
        x = self._x(x, self.n)
        cost = ctypes.c_double(0.0)
        r = np.zeros((2, self.num_landmark_observations)) if rows else None
        self._check(self.lib.mvus_ba_landmark_cost(self.h, _lib.dptr(x), ctypes.byref(cost), _lib.dptr(r) if rows else None), 'mvus_ba_landmark_cost')
        return (cost.value, r) if rows else cost.value

    def landmark_rows(self, x):
        """(r (2, K), J (K, 2, P)): the weighted landmark rows at x and their derivatives w.r.t. the P parameters of each row's camera."""
        x = self._x(x, self.n)
        K = self.num_landmark_observations
        r = np.zeros((2, K))
        J = np.zeros((K, 2, self.prob.P))
        self._check(self.lib.mvus_ba_landmark_rows(self.h, _lib.dptr(x), _lib.dptr(r), _lib.dptr(J)), 'mvus_ba_landmark_rows')
        return r, J

    def robust_cost(self, x, weights=False):
        """0.5 f_scale^2 sum rho((f_i / f_scale)^2) at x under the loss in force; with ``weights`` also rho' of every row of f
        (1 = inlier, -> 0 = ignored): (cost, w[m])."""
        x = self._x(x, self.n)
        cost = ctypes.c_double(0.0)
        w = np.empty(self.m) if weights else None
        self._check(self.lib.mvus_ba_robust_cost(self.h, _lib.dptr(x), ctypes.byref(cost), _lib.dptr(w) if weights else None),
                    'mvus_ba_robust_cost')
        return (cost.value, w) if weights else cost.value

    def covariance(self, x, sigma2=None):
        """Covariance of the estimate at x (mvus_ba_covariance) under the loss and the frozen mask in force: a namespace with
        ``cam`` [CB, CB] in the order of the head of x (alpha(C), beta(C), rs(C), P per camera), ``band`` [N, 4, 3, 3] (blocks (p, p + w) of
        the control points, control-point order), ``estimated`` bool[n] in the order of x, ``sigma2`` (the caller's when given and > 0, else
        2 cost / dof) and ``dof``.  Rows and columns of unknowns that are not estimated are exactly 0.  A free gauge raises ValueError
        (MVUS_E_NUMERIC) with "gauge" in the message."""
        x = self._x(x, self.n)
        CB, N = self.prob.C * (3 + self.prob.P), int(self.prob.n_coef.sum())
        cam = np.empty((CB, CB))
        band = np.empty((N, 4, 3, 3))
        est = np.empty(self.n, dtype=np.uint8)
        s2, dof = ctypes.c_double(0.0), ctypes.c_int64(0)
        self._check(self.lib.mvus_ba_covariance(self.h, _lib.dptr(x), 0.0 if sigma2 is None else float(sigma2), _lib.dptr(cam), _lib.dptr(band),
                                                est.ctypes.data_as(_lib.c_uint8_p), ctypes.byref(s2), ctypes.byref(dof)), 'mvus_ba_covariance')
        return SimpleNamespace(cam=cam, band=band, estimated=est.astype(bool), sigma2=s2.value, dof=int(dof.value))

    def covariance_stage_ms(self):
        """[(stage name, milliseconds)] of the last ``covariance`` call on the handle (HIP events)."""
        ms = (ctypes.c_double * 16)()
        names = (ctypes.c_char_p * 16)()
        k = self.lib.mvus_ba_covariance_stage_ms(self.h, ms, names, 16)
        self._check(min(k, 0), 'mvus_ba_covariance_stage_ms')
        return [(names[i].decode(), ms[i]) for i in range(k)]

    def detection_covariance(self, x, sigma2=None):
        """The covariance at x carried back to the image plane (mvus_ba_detection_covariance): the namespace of ``covariance`` -- the same
        bits, one run of the chain -- plus, per detection in camera-segmented order (M = all detections),
        ``e`` [2, M] the signed residual (u, v) in pixels, predicted minus observed (``abs(e)`` is the detection's two rows of ``residual``),
        ``cov`` [3, M] = (P_uu, P_uv, P_vv) of P = J_i Sigma J_i^T in image axes (the 1-sigma ellipse of the fitted detection; with
        ``opt_calib`` and ``undist_points`` the observed point moves with the intrinsics too, and P is the covariance of the fitted part of
        the residual in the undistorted frame), and ``t2`` [M] = r^T (sigma2 I - P)^-1 r, the squared studentised residual (chi^2 with 2
        degrees of freedom under the linear loss; NaN when sigma2 I - P is not positive definite).  A detection without a knot span has NaN
        in ``cov`` and ``t2`` and 0 in ``e``.  Refusals as for ``covariance``."""
        x = self._x(x, self.n)
        CB, N, M = self.prob.C * (3 + self.prob.P), int(self.prob.n_coef.sum()), int(self.M)
        cam = np.empty((CB, CB))
        band = np.empty((N, 4, 3, 3))
        est = np.empty(self.n, dtype=np.uint8)
        e, pc, t2 = np.zeros((2, M)), np.full((3, M), np.nan), np.full(M, np.nan)
        s2, dof = ctypes.c_double(0.0), ctypes.c_int64(0)
        self._check(self.lib.mvus_ba_detection_covariance(self.h, _lib.dptr(x), 0.0 if sigma2 is None else float(sigma2), _lib.dptr(e), _lib.dptr(pc),
                                                          _lib.dptr(t2), _lib.dptr(cam), _lib.dptr(band), est.ctypes.data_as(_lib.c_uint8_p),
                                                          ctypes.byref(s2), ctypes.byref(dof)), 'mvus_ba_detection_covariance')
        return SimpleNamespace(e=e, cov=pc, t2=t2, cam=cam, band=band, estimated=est.astype(bool), sigma2=s2.value, dof=int(dof.value))

    def detection_covariance_ms(self):
        """Milliseconds (HIP events) of the detection pass of the last ``detection_covariance`` call on the handle."""
        ms = ctypes.c_double(0.0)
        self._check(self.lib.mvus_ba_detection_covariance_ms(self.h, ctypes.byref(ms)), 'mvus_ba_detection_covariance_ms')
        return ms.value

    def solve(self, x0, solver=SOLVER_TRF_LSMR, jac_mode=JAC_PATTERN, max_nfev=10, opts=None, return_fun=True,
              ties='numpy', matrix=None, prepared=False):
        """The least_squares call of Scene.BA.  Returns an OptimizeResult-like namespace
        (x, cost, fun, nfev, njev, status, optimality, ...).  ``ties`` / ``matrix``: how the reference pattern of the
        JAC_PATTERN / JAC_FD modes is fixed at x0 (see prepare_pattern); ``prepared``: the pattern (and column groups) UPLOADED by an
        earlier prepare_pattern / prepare_fd stay in force (a run of steps with ONE pattern, as least_squares keeps its
        jac_sparsity) -- a pattern that only exists on the device (set_pattern) would be recomputed at every call's x0, so that is
        refused here."""
        x = np.array(self._x(x0, self.n))
        o = opts if opts is not None else _lib.default_opts(solver, jac_mode, max_nfev)
        if prepared and o.jac_mode in (JAC_FD, JAC_PATTERN):
            if not getattr(self, '_pattern_fixed', False):
                raise ValueError('solve(prepared=True): call prepare_pattern / prepare_fd (or upload_pattern) first')
        elif o.jac_mode == JAC_FD:
            self.prepare_fd(x, ties, matrix)
        elif o.jac_mode == JAC_PATTERN and (matrix is not None or ties != 'canonical'):
            self.prepare_pattern(x, ties, matrix)
        elif o.jac_mode == JAC_PATTERN:
            self.set_pattern(x, download=False)      # canonical codes stay on the GPU: no host round trip (clears an uploaded pattern)
        res = _lib.MvusResult()
        f = np.empty(self.m) if return_fun else None
        rc = self.lib.mvus_ba_solve(self.h, _lib.dptr(x), ctypes.byref(o), ctypes.byref(res), _lib.dptr(f) if return_fun else None)
        if rc == _lib.MVUS_E_RESHARD:
            e = ReshardNeeded('mvus_ba_solve: %s' % self.lib.mvus_last_error(self.h).decode())
            e.x, e.nfev, e.cost, e.initial_cost = x, int(res.nfev), float(res.cost), float(res.initial_cost)
            raise e
        self._check(rc, 'mvus_ba_solve')
        return _Result(x=x, cost=res.cost, fun=f, nfev=res.nfev, njev=res.njev, status=res.status,
                       optimality=res.optimality, lin_iters=res.lin_iters, solve_ms=res.solve_ms,
                       initial_cost=res.initial_cost, success=res.status > 0, grad=None, jac=None)

    def _register_args(self, x, cams, start):
        x = self._x(x, self.n)
        cams = np.ascontiguousarray(np.atleast_1d(cams), dtype=np.int32).ravel()
        B, nb = cams.size, 3 + self.prob.P
        if start is not None:
            start = np.ascontiguousarray(start, dtype=np.float64).reshape(-1, nb) if np.size(start) else np.empty((0, nb))
            if start.shape != (B, nb):
                raise ValueError('start has shape %s, expected (%d, %d)' % (start.shape, B, nb))
        return x, cams, start, B, nb

    def register_cameras(self, x, cams, start=None, max_nfev=50, ftol=1e-8, xtol=1e-12, gtol=1e-8, lambda0=0, lambda_min=0, inlier_thres=0):
        """Register cameras against the trajectory of ``x``, which stays as it is (mvus_ba_register_cameras): problem b adjusts camera
        ``cams[b]``'s alpha, beta, rs and P parameters from ``start[b]`` (3 + P values in that order; ``None``: the camera's entries of x)
        over its own detection rows, by Levenberg-Marquardt on the device, all problems in one call.  The handle's loss and frozen mask
        are in force.  Returns a namespace of arrays: ``params`` (B, 3 + P), ``cost``, ``initial_cost``, ``nfev``, ``status`` (scipy's 0 - 4,
        -1 = never started), ``visible`` and ``inliers`` (detections with a span / with an error below ``inlier_thres`` at the result).
        Changes nothing a later solve sees."""
        x, cams, start, B, nb = self._register_args(x, cams, start)
        params, cost, cost0 = np.zeros((B, nb)), np.zeros(B), np.zeros(B)
        nfev, status = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
        vis, inl = np.zeros(B, dtype=np.int64), np.zeros(B, dtype=np.int64)
        i32, i64 = (lambda a: a.ctypes.data_as(_lib.c_int32_p)), (lambda a: a.ctypes.data_as(_lib.c_int64_p))
        self._check(self.lib.mvus_ba_register_cameras(
            self.h, _lib.dptr(x), B, i32(cams), _lib.dptr(start) if start is not None else None, int(max_nfev), float(ftol), float(xtol),
            float(gtol), float(lambda0), float(lambda_min), float(inlier_thres), _lib.dptr(params), _lib.dptr(cost), _lib.dptr(cost0),
            i32(nfev), i32(status), i64(vis), i64(inl)), 'mvus_ba_register_cameras')
        return SimpleNamespace(params=params, cost=cost, initial_cost=cost0, nfev=nfev, status=status, visible=vis, inliers=inl)

    def register_linearize(self, x, cams, start=None):
        """(H (B, 3 + P, 3 + P), g (B, 3 + P), cost (B,), visible (B,)) of the registration problems at their start points, exactly as the
        first iteration of ``register_cameras`` forms them (mvus_ba_register_linearize)."""
        x, cams, start, B, nb = self._register_args(x, cams, start)
        H, g, cost = np.zeros((B, nb, nb)), np.zeros((B, nb)), np.zeros(B)
        vis = np.zeros(B, dtype=np.int64)
        self._check(self.lib.mvus_ba_register_linearize(
            self.h, _lib.dptr(x), B, cams.ctypes.data_as(_lib.c_int32_p), _lib.dptr(start) if start is not None else None,
            _lib.dptr(H), _lib.dptr(g), _lib.dptr(cost), vis.ctypes.data_as(_lib.c_int64_p)), 'mvus_ba_register_linearize')
        return H, g, cost, vis

    def outlier_mask(self, x, thres):
        """Per-detection ``error < thres`` (camera-segmented order), dtype bool."""
        x = self._x(x, self.n)
        keep = np.empty(self.M, dtype=np.uint8)
        self._check(self.lib.mvus_ba_outlier_mask(self.h, _lib.dptr(x), float(thres), keep.ctypes.data_as(_lib.c_uint8_p)),
                    'mvus_ba_outlier_mask')
        return keep.astype(bool)

    def remove_outliers(self, x, thres):
        """Scene.remove_outliers on the handle itself: the device-resident detections are filtered in place and the
        handle (and ``self.prob``) describe the inliers afterwards.  Returns the keep mask over the old detections."""
        x = self._x(x, self.n)
        keep = np.empty(self.M, dtype=np.uint8)
        off = np.zeros(self.prob.C + 1, dtype=np.int64)
        self._check(self.lib.mvus_ba_remove_outliers(self.h, _lib.dptr(x), float(thres), keep.ctypes.data_as(_lib.c_uint8_p),
                                                     off.ctypes.data_as(_lib.c_int64_p)), 'mvus_ba_remove_outliers')
        keep = keep.astype(bool)
        import dataclasses
        self.prob = dataclasses.replace(self.prob, det_offsets=off, frame=self.prob.frame[keep], u_raw=self.prob.u_raw[keep],
                                        v_raw=self.prob.v_raw[keep])
        self.M = self.prob.M
        self.m = int(self.lib.mvus_ba_num_residuals(self.h))
        assert self.m == self.prob.n_residuals
        return keep

    def set_x(self, x):
        x = self._x(x, self.n)
        self._check(self.lib.mvus_ba_set_x(self.h, _lib.dptr(x)), 'mvus_ba_set_x')

    def time_kernel(self, which, launches=20):
        """Average duration (ms) of ``launches`` back-to-back launches, HIP events on the handle's stream."""
        ms = ctypes.c_double(0.0)
        self._check(self.lib.mvus_ba_time_kernel(self.h, which, launches, ctypes.byref(ms)), 'mvus_ba_time_kernel')
        return ms.value

    def set_time_shard(self, rank, world, cuts, halo=8):
        """This handle holds time slice ``rank`` of ``world`` (BAProblem.shard_time): the LM/Schur solver keeps only the
        spline blocks of control points cuts[rank]..cuts[rank+1] (+- halo).  Call before set_allreduce."""
        cuts = np.ascontiguousarray(cuts, dtype=np.int32)
        assert cuts.size == world + 1
        self._check(self.lib.mvus_ba_set_time_shard(self.h, int(rank), int(world), cuts.ctypes.data_as(_lib.c_int32_p), int(halo)),
                    'mvus_ba_set_time_shard')

    def set_allreduce(self, fn, is_root=True):
        """fn(buf_dev_ptr:int, count:int, stream:int) -> None sums ``count`` doubles in place across ranks."""
        if fn is None:
            self._cb = _lib.ALLREDUCE_FN(0)
        else:
            def tramp(user, buf, count, stream):
                try:
                    fn(int(buf), int(count), int(stream or 0))
                    return 0
                except Exception:      # never let an exception cross the C boundary
                    import traceback
                    traceback.print_exc()
                    return 1
            self._cb = _lib.ALLREDUCE_FN(tramp)
        self._check(self.lib.mvus_ba_set_allreduce(self.h, self._cb, None, int(bool(is_root))), 'mvus_ba_set_allreduce')


    def set_rccl(self, unique_id, rank, world, is_root=True):
        """The sums over the ranks by RCCL called from the library (ncclAllReduce on the handle's stream; no Python in the iteration).
        ``unique_id``: the 128 bytes of _lib.rccl_unique_id() of ONE rank; collective -- returns once all ``world`` ranks have joined."""
        buf = (ctypes.c_uint8 * 128).from_buffer_copy(bytes(unique_id))
        self._cb = None
        self._check(self.lib.mvus_ba_set_rccl(self.h, buf, int(rank), int(world), int(bool(is_root))), 'mvus_ba_set_rccl')

    def time_allreduce(self, count, reps=50):
        """Average milliseconds per sum of ``count`` doubles through the installed route (callback or RCCL), HIP events on the handle's stream."""
        ms = ctypes.c_double(0.0)
        self._check(self.lib.mvus_ba_time_allreduce(self.h, int(count), int(reps), ctypes.byref(ms)), 'mvus_ba_time_allreduce')
        return ms.value


# kernel ids of mvus_ba_time_kernel
KERNEL_RESIDUAL, KERNEL_RESIDUAL_JACOBIAN, KERNEL_JV, KERNEL_JTU, KERNEL_ASSEMBLY, KERNEL_RESIDUAL_JACOBIAN_ONE_BUFFER, KERNEL_FUSED_ASSEMBLY = 0, 1, 2, 3, 4, 5, 6
