"""Spline maintenance either side of BA on the GPU, through the C ABI:

``evaluate``   = the evaluation inside ``Scene.spline_to_traj`` (reference common.py:273-301; scipy ``splev``)
``evaluate_der`` / ``kin_cov_evaluate`` / ``path_length`` = kinematics of the same samples: X, X', X'' (scipy ``splev(der=)``), the
                 covariance of that state from the control points' band, the distance flown (``mvus_spline_eval_der``,
                 ``mvus_spline_kin_cov_eval``, ``mvus_spline_length``)
``lsq_fit``    = least-squares coefficients on a fixed knot vector (the refit step of ``traj_to_spline`` once the knots are
                 placed; scipy ``make_lsq_spline``)
``smooth_fit``  = ``scipy.interpolate.splprep(X, u=t, s=s, k=3)``: FITPACK's adaptive knot placement and smoothing-parameter search
                 with the sample passes and banded solves on the GPU (``mvus_spline_smooth``)
``traj_fit``    = the reference's smooth_factor loop around it (common.py:241-262): one interval of ``Scene.traj_to_spline``
No CPU fallback: without libmvusba.so / a GPU these raise."""
import ctypes

import numpy as np

from . import _lib


def _err(lib, rc, what):
    raise (ValueError if rc in (_lib.MVUS_E_INVALID, _lib.MVUS_E_NUMERIC) else RuntimeError)('%s: %s' % (what, lib.mvus_last_error(None).decode()))


def evaluate(tck, interval, t, device=0):
    """Points of the splines ``tck`` (list of [knots, [cx, cy, cz], 3]) at timestamps ``t`` (1-D).  Returns (X[3, len(t)],
    which[len(t)]): ``which`` is the interval each timestamp lies in (start <= t <= end) or -1, X is 0 where -1."""
    lib = _lib.load()
    interval = np.ascontiguousarray(np.asarray(interval, dtype=np.float64))
    S = interval.shape[1]
    knots = [np.asarray(k[0], dtype=np.float64) for k in tck]
    koff = np.concatenate(([0], np.cumsum([k.size for k in knots]))).astype(np.int64)
    coefs = np.concatenate([np.ravel(np.asarray(k[1], dtype=np.float64)) for k in tck])
    kn = np.ascontiguousarray(np.concatenate(knots))
    t = np.ascontiguousarray(t, dtype=np.float64)
    if t.ndim != 1:
        raise ValueError('Input timestamps must be a 1D array')
    X = np.zeros((3, t.size))
    which = np.full(t.size, -1, dtype=np.int32)
    rc = lib.mvus_spline_eval(int(device), int(S), _lib.dptr(interval), koff.ctypes.data_as(_lib.c_int64_p), _lib.dptr(kn), _lib.dptr(coefs),
                              t.size, _lib.dptr(t), _lib.dptr(X), which.ctypes.data_as(_lib.c_int32_p))
    if rc != 0:
        _err(lib, rc, 'mvus_spline_eval')
    return X, which


def cov_evaluate(tck, interval, band, t, device=0):
    """Covariance of the spline points at timestamps ``t`` from ``band`` [N, 4, 3, 3] -- the control points' band of
    ``BAHandle.covariance`` (N = all control points, the splines one behind the other): ``mvus_spline_cov_eval``.  Returns
    (cov[len(t), 3, 3], which[len(t)]); NaN where which = -1 (outside every interval)."""
    lib = _lib.load()
    interval = np.ascontiguousarray(np.asarray(interval, dtype=np.float64))
    S = interval.shape[1]
    knots = [np.asarray(k[0], dtype=np.float64) for k in tck]
    koff = np.concatenate(([0], np.cumsum([k.size for k in knots]))).astype(np.int64)
    kn = np.ascontiguousarray(np.concatenate(knots))
    band = np.ascontiguousarray(band, dtype=np.float64)
    if band.shape != (int(koff[-1]) - 4 * S, 4, 3, 3):
        raise ValueError('band has shape %s, expected (%d, 4, 3, 3)' % (band.shape, int(koff[-1]) - 4 * S))
    t = np.ascontiguousarray(t, dtype=np.float64)
    if t.ndim != 1:
        raise ValueError('Input timestamps must be a 1D array')
    cov = np.full((t.size, 3, 3), np.nan)
    which = np.full(t.size, -1, dtype=np.int32)
    rc = lib.mvus_spline_cov_eval(int(device), int(S), _lib.dptr(interval), koff.ctypes.data_as(_lib.c_int64_p), _lib.dptr(kn), _lib.dptr(band),
                                  t.size, _lib.dptr(t), _lib.dptr(cov), which.ctypes.data_as(_lib.c_int32_p))
    if rc != 0:
        _err(lib, rc, 'mvus_spline_cov_eval')
    return cov, which


def _spline_args(tck, interval, t):
    """(interval, S, knot offsets, knots, t) as the stateless spline calls take them"""
    interval = np.ascontiguousarray(np.asarray(interval, dtype=np.float64))
    knots = [np.asarray(k[0], dtype=np.float64) for k in tck]
    koff = np.concatenate(([0], np.cumsum([k.size for k in knots]))).astype(np.int64)
    kn = np.ascontiguousarray(np.concatenate(knots))
    t = np.ascontiguousarray(t, dtype=np.float64)
    if t.ndim != 1:
        raise ValueError('Input timestamps must be a 1D array')
    return interval, interval.shape[1], koff, kn, t


def evaluate_der(tck, interval, t, nder=2, device=0):
    """The points of ``evaluate`` with their first ``nder`` (0, 1 or 2) derivatives in the spline parameter: (D[nder + 1, 3, len(t)],
    which[len(t)]), D[0] = ``evaluate``'s X to the bit, D[1] = X', D[2] = X''; 0 where which = -1.  ``mvus_spline_eval_der``."""
    lib = _lib.load()
    interval, S, koff, kn, t = _spline_args(tck, interval, t)
    coefs = np.concatenate([np.ravel(np.asarray(k[1], dtype=np.float64)) for k in tck])
    D = np.zeros((max(int(nder), 0) + 1, 3, t.size))
    which = np.full(t.size, -1, dtype=np.int32)
    rc = lib.mvus_spline_eval_der(int(device), int(S), _lib.dptr(interval), koff.ctypes.data_as(_lib.c_int64_p), _lib.dptr(kn), _lib.dptr(coefs),
                                  t.size, _lib.dptr(t), int(nder), _lib.dptr(D), which.ctypes.data_as(_lib.c_int32_p))
    if rc != 0:
        _err(lib, rc, 'mvus_spline_eval_der')
    return D, which


def kin_cov_evaluate(tck, interval, band, t, nder=2, device=0):
    """Covariance of the state (X, X', .., D^nder X) at timestamps ``t`` from ``band`` [N, 4, 3, 3] (as ``cov_evaluate``):
    (cov[len(t), D, D], which[len(t)]) with D = 3 (nder + 1), component 3 i + r = coordinate r of derivative i; exactly symmetric; NaN
    where which = -1.  ``mvus_spline_kin_cov_eval``."""
    lib = _lib.load()
    interval, S, koff, kn, t = _spline_args(tck, interval, t)
    band = np.ascontiguousarray(band, dtype=np.float64)
    if band.shape != (int(koff[-1]) - 4 * S, 4, 3, 3):
        raise ValueError('band has shape %s, expected (%d, 4, 3, 3)' % (band.shape, int(koff[-1]) - 4 * S))
    D = 3 * (max(int(nder), 0) + 1)
    cov = np.full((t.size, D, D), np.nan)
    which = np.full(t.size, -1, dtype=np.int32)
    rc = lib.mvus_spline_kin_cov_eval(int(device), int(S), _lib.dptr(interval), koff.ctypes.data_as(_lib.c_int64_p), _lib.dptr(kn), _lib.dptr(band),
                                      t.size, _lib.dptr(t), int(nder), _lib.dptr(cov), which.ctypes.data_as(_lib.c_int32_p))
    if rc != 0:
        _err(lib, rc, 'mvus_spline_kin_cov_eval')
    return cov, which


def path_length(tck, interval, t, device=0):
    """Distance flown: (dist[len(t)], which[len(t)], total[S]) -- ``dist`` the length of the curve from the start of the timestamp's interval
    to the timestamp (0 where which = -1), ``total`` the length of each interval.  ``mvus_spline_length``."""
    lib = _lib.load()
    interval, S, koff, kn, t = _spline_args(tck, interval, t)
    coefs = np.concatenate([np.ravel(np.asarray(k[1], dtype=np.float64)) for k in tck])
    dist = np.zeros(t.size)
    which = np.full(t.size, -1, dtype=np.int32)
    total = np.zeros(S)
    rc = lib.mvus_spline_length(int(device), int(S), _lib.dptr(interval), koff.ctypes.data_as(_lib.c_int64_p), _lib.dptr(kn), _lib.dptr(coefs),
                                t.size, _lib.dptr(t), _lib.dptr(dist), which.ctypes.data_as(_lib.c_int32_p), _lib.dptr(total))
    if rc != 0:
        _err(lib, rc, 'mvus_spline_length')
    return dist, which, total


def lsq_fit(knots, t, X, device=0):
    """Coefficients [cx, cy, cz] of the least-squares cubic spline with knot vector ``knots`` through the points X[3, m] at t[m]."""
    lib = _lib.load()
    knots = np.ascontiguousarray(knots, dtype=np.float64)
    t = np.ascontiguousarray(t, dtype=np.float64)
    X = np.ascontiguousarray(np.asarray(X, dtype=np.float64))
    if X.shape != (3, t.size):
        raise ValueError('X must be 3 x len(t)')
    n = knots.size - 4
    c = np.empty((3, max(n, 1)))
    rc = lib.mvus_spline_lsq(int(device), int(knots.size), _lib.dptr(knots), t.size, _lib.dptr(t), _lib.dptr(X), _lib.dptr(c))
    if rc != 0:
        _err(lib, rc, 'mvus_spline_lsq')
    return [c[0].copy(), c[1].copy(), c[2].copy()]


def _weights(w, m):
    """splprep's ``w`` as the library takes it: a contiguous float64[m] (its values are checked there: finite and > 0)"""
    w = np.ascontiguousarray(w, dtype=np.float64)
    if w.shape != (m,):
        raise ValueError('w has shape %s, expected (%d,): one weight per sample' % (w.shape, m))
    return w


def smooth_fit(t, X, s, device=0, full_output=False, w=None):
    """``scipy.interpolate.splprep(X, w=w, u=t, s=s, k=3)[0]``: the tck ``[knots, [cx, cy, cz], 3]`` of the smoothing cubic spline
    through X[3, m] at the strictly increasing timestamps t[m].  ``full_output``: also (fp, ier) as FITPACK reports them.
    ``w``: None (unit weights, the reference's call), or one finite positive weight per sample, 1 / sigma of the sample up to a common
    factor (``mvus_spline_smooth_w``); ``fp`` is then the weighted residual sum that ``s`` is compared with."""
    lib = _lib.load()
    t = np.ascontiguousarray(t, dtype=np.float64)
    X = np.ascontiguousarray(np.asarray(X, dtype=np.float64))
    if t.ndim != 1 or X.shape != (3, t.size):
        raise ValueError('X must be 3 x len(t)')
    nest = t.size + 6
    n = ctypes.c_int32(0)
    ier = ctypes.c_int32(0)
    fp = ctypes.c_double(0.0)
    knots = np.zeros(nest)
    c = np.zeros((3, nest))
    if w is None:
        rc = lib.mvus_spline_smooth(int(device), t.size, _lib.dptr(t), _lib.dptr(X), float(s), ctypes.byref(n), _lib.dptr(knots), _lib.dptr(c),
                                    ctypes.byref(fp), ctypes.byref(ier))
    else:
        w = _weights(w, t.size)
        rc = lib.mvus_spline_smooth_w(int(device), t.size, _lib.dptr(t), _lib.dptr(X), _lib.dptr(w), float(s), ctypes.byref(n), _lib.dptr(knots),
                                      _lib.dptr(c), ctypes.byref(fp), ctypes.byref(ier))
    if rc != 0:
        _err(lib, rc, 'mvus_spline_smooth' if w is None else 'mvus_spline_smooth_w')
    nk = n.value
    tck = [knots[:nk].copy(), [c[d, :nk - 4].copy() for d in range(3)], 3]
    return (tck, fp.value, ier.value) if full_output else tck


class SmoothFit:
    """``smooth_fit`` for several smoothing factors on ONE set of samples: the samples are checked and uploaded once and the
    device work arrays are kept (``mvus_spline_fit_open`` / ``_smooth`` / ``_close``) -- what ``traj_fit``'s loop needs.  ``w`` as in
    ``smooth_fit`` (``mvus_spline_fit_open_w``): the weights belong to the session.

        with SmoothFit(t, X) as fit:
            tck = fit(s)
    """

    def __init__(self, t, X, device=0, w=None):
        self.lib = _lib.load()
        t = np.ascontiguousarray(t, dtype=np.float64)
        X = np.ascontiguousarray(np.asarray(X, dtype=np.float64))
        if t.ndim != 1 or X.shape != (3, t.size):
            raise ValueError('X must be 3 x len(t)')
        self.m = t.size
        self.h = ctypes.c_void_p()
        if w is None:
            rc = self.lib.mvus_spline_fit_open(int(device), t.size, _lib.dptr(t), _lib.dptr(X), ctypes.byref(self.h))
        else:
            w = _weights(w, t.size)
            rc = self.lib.mvus_spline_fit_open_w(int(device), t.size, _lib.dptr(t), _lib.dptr(X), _lib.dptr(w), ctypes.byref(self.h))
        if rc != 0:
            self.h = None
            _err(self.lib, rc, 'mvus_spline_fit_open' if w is None else 'mvus_spline_fit_open_w')
        nest = self.m + 6
        self._knots = np.zeros(nest)
        self._c = np.zeros((3, nest))

    def __call__(self, s, full_output=False):
        if not self.h:
            raise ValueError('the fit session is closed')
        n = ctypes.c_int32(0)
        ier = ctypes.c_int32(0)
        fp = ctypes.c_double(0.0)
        rc = self.lib.mvus_spline_fit_smooth(self.h, float(s), ctypes.byref(n), _lib.dptr(self._knots), _lib.dptr(self._c), ctypes.byref(fp), ctypes.byref(ier))
        if rc != 0:
            _err(self.lib, rc, 'mvus_spline_fit_smooth')
        nk = n.value
        tck = [self._knots[:nk].copy(), [self._c[d, :nk - 4].copy() for d in range(3)], 3]
        return (tck, fp.value, ier.value) if full_output else tck

    def close(self):
        if getattr(self, 'h', None):
            self.lib.mvus_spline_fit_close(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:                                               # (at interpreter shutdown even `import sys` can fail)
            import sys
            if sys.is_finalizing():
                return
            self.close()
        except Exception:
            pass


def _band_operand(a, lo, shape, name):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if a.shape != shape:
        raise ValueError('%s has shape %s, expected %s' % (name, a.shape, shape))
    if lo is not None:
        lo = np.ascontiguousarray(lo, dtype=np.float64)
        if lo.shape != shape:
            raise ValueError('%s_lo has shape %s, expected %s' % (name, lo.shape, shape))
    return a, lo


def band_solve(G5, rhs, hb, BtB=None, pinv=0.0, precise=False, parts=0, G5_lo=None, BtB_lo=None, rhs_lo=None, device=0):
    """The fit's banded solvers on a system handed in (``mvus_spline_band_solve``, an inspection hook): G5[n, 5] (and BtB[n, 5] with
    ``hb`` = 4) in the kernels' lower-band layout, ``M(j, j - w)`` at ``[j, w]``; rhs[3, n].  Solves G5 (hb = 3) or G5 + pinv^2 BtB
    (hb = 4) in fp64, or in double-double on (hi, ``_lo``) when ``precise``; ``parts`` = -1 one chain, 0 the fit's own rule, >= 2 that
    many interiors.  Returns a namespace: c[3, n], stats[4] (the kernel's out[0..3]), fail, P (interiors used)."""
    from types import SimpleNamespace
    lib = _lib.load()
    G5 = np.ascontiguousarray(G5, dtype=np.float64)
    n = G5.shape[0] if G5.ndim == 2 else -1
    G5, G5_lo = _band_operand(G5, G5_lo, (n, 5), 'G5')
    rhs, rhs_lo = _band_operand(rhs, rhs_lo, (3, n), 'rhs')
    if BtB is not None:
        BtB, BtB_lo = _band_operand(BtB, BtB_lo, (n, 5), 'BtB')
    elif BtB_lo is not None:
        raise ValueError('BtB_lo without BtB')
    p = lambda a: _lib.dptr(a) if a is not None else None    # noqa: E731
    c = np.zeros((3, max(n, 1)))
    stats = np.zeros(4)
    fail, P = ctypes.c_int32(0), ctypes.c_int32(0)
    rc = lib.mvus_spline_band_solve(int(device), int(n), int(hb), int(bool(precise)), int(parts), p(G5), p(G5_lo), p(BtB), p(BtB_lo), float(pinv),
                                    p(rhs), p(rhs_lo), _lib.dptr(c), _lib.dptr(stats), ctypes.byref(fail), ctypes.byref(P))
    if rc != 0:
        _err(lib, rc, 'mvus_spline_band_solve')
    return SimpleNamespace(c=c, stats=stats, fail=fail.value, P=P.value)


def band_diag_sum(G5, precise=False, G5_lo=None, device=0):
    """Sum of diag(L) of G5 = L L^T (half-bandwidth 3) in the natural order, by the kernel that gives the smoothing iteration its initial
    p after a partitioned pass (``mvus_spline_band_diag_sum``, an inspection hook).  G5[n, 5] as in ``band_solve``."""
    lib = _lib.load()
    G5 = np.ascontiguousarray(G5, dtype=np.float64)
    n = G5.shape[0] if G5.ndim == 2 else -1
    G5, G5_lo = _band_operand(G5, G5_lo, (n, 5), 'G5')
    out = np.zeros(1)
    rc = lib.mvus_spline_band_diag_sum(int(device), int(n), int(bool(precise)), _lib.dptr(G5), _lib.dptr(G5_lo) if G5_lo is not None else None, _lib.dptr(out))
    if rc != 0:
        _err(lib, rc, 'mvus_spline_band_diag_sum')
    return float(out[0])


def _fit_samples(u, X, t):
    u = np.ascontiguousarray(u, dtype=np.float64)
    X = np.ascontiguousarray(X, dtype=np.float64)
    t = np.ascontiguousarray(t, dtype=np.float64)
    if u.ndim != 1 or t.ndim != 1 or X.shape != (3, u.size):
        raise ValueError('u[m], X[3, m] and a 1-D knot vector expected')
    return u, X, t


def fit_normal(u, X, t, precise=False, slices=0, parts=0, device=0, w=None):
    """One least-squares pass of the smoothing fit on the knots ``t`` (``mvus_spline_fit_normal``, an inspection hook): k_fit_basis,
    k_fit_first, then the fit's own assembly and banded solve, in fp64 or (``precise``) double-double.  ``slices`` = 0: the fit's
    rule, >= 1: that many slices per span; ``parts`` as in ``band_solve``.  Returns a namespace: span[m], q[m, 4], first[nspan + 1],
    G5 / G5_lo[ncoef, 5], rhs / rhs_lo[3, ncoef], c[3, ncoef], stats[4], fail.  ``w``: the pass of a weighted fit
    (``mvus_spline_fit_normal_w``): the normal equations of the rows w_i h, right-hand sides w_i X_i; q stays the unweighted basis."""
    from types import SimpleNamespace
    lib = _lib.load()
    u, X, t = _fit_samples(u, X, t)
    m, n = u.size, t.size
    nc, ns = max(n - 4, 1), max(n - 7, 1)
    span, q, first = np.zeros(m, np.int32), np.zeros((m, 4)), np.zeros(ns + 1, np.int64)
    G5, G5_lo, rhs, rhs_lo, c, stats = np.zeros((nc, 5)), np.zeros((nc, 5)), np.zeros((3, nc)), np.zeros((3, nc)), np.zeros((3, nc)), np.zeros(4)
    fail = ctypes.c_int32(0)
    tail = (n, _lib.dptr(t), int(bool(precise)), int(slices), int(parts), span.ctypes.data_as(_lib.c_int32_p), _lib.dptr(q), first.ctypes.data_as(_lib.c_int64_p),
            _lib.dptr(G5), _lib.dptr(G5_lo), _lib.dptr(rhs), _lib.dptr(rhs_lo), _lib.dptr(c), _lib.dptr(stats), ctypes.byref(fail))
    if w is None:
        rc = lib.mvus_spline_fit_normal(int(device), m, _lib.dptr(u), _lib.dptr(X), *tail)
    else:
        w = _weights(w, m)
        rc = lib.mvus_spline_fit_normal_w(int(device), m, _lib.dptr(u), _lib.dptr(X), _lib.dptr(w), *tail)
    if rc != 0:
        _err(lib, rc, 'mvus_spline_fit_normal' if w is None else 'mvus_spline_fit_normal_w')
    return SimpleNamespace(span=span, q=q, first=first, G5=G5, G5_lo=G5_lo, rhs=rhs, rhs_lo=rhs_lo, c=c, stats=stats, fail=fail.value)


def fit_penalty(b, ncoef, precise=False, device=0):
    """B^T B of the jump matrix ``b[n8, 5]`` (fpdisc's layout) over ``ncoef`` coefficients by k_fit_penalty alone
    (``mvus_spline_fit_penalty``, an inspection hook).  Returns (BtB[ncoef, 5], BtB_lo[ncoef, 5]) in ``band_solve``'s layout."""
    lib = _lib.load()
    b = np.ascontiguousarray(b, dtype=np.float64)
    if b.ndim != 2 or b.shape[1] != 5:
        raise ValueError('b[n8, 5] expected')
    nc = max(int(ncoef), 1)
    BtB, BtB_lo = np.zeros((nc, 5)), np.zeros((nc, 5))
    rc = lib.mvus_spline_fit_penalty(int(device), int(ncoef), b.shape[0], _lib.dptr(b), int(bool(precise)), _lib.dptr(BtB), _lib.dptr(BtB_lo))
    if rc != 0:
        _err(lib, rc, 'mvus_spline_fit_penalty')
    return BtB, BtB_lo


def fit_residual(u, X, t, c, slices=0, device=0, w=None):
    """The residual pass of the smoothing fit for coefficients ``c[3, ncoef]`` on the knots ``t`` (``mvus_spline_fit_residual``, an
    inspection hook): returns a namespace with term[m] (squared residual per sample), fp (their total) and fpint[nspan] (per span,
    the sample that opens a span shared half / half with the span before).  ``w``: the pass of a weighted fit
    (``mvus_spline_fit_residual_w``): term[i] = |w_i (s(u_i) - X_i)|^2."""
    from types import SimpleNamespace
    lib = _lib.load()
    u, X, t = _fit_samples(u, X, t)
    m, n = u.size, t.size
    c = np.ascontiguousarray(c, dtype=np.float64)
    if c.shape != (3, n - 4):
        raise ValueError('c has shape %s, expected (3, %d)' % (c.shape, n - 4))
    term, fp, fpint = np.zeros(m), np.zeros(1), np.zeros(max(n - 7, 1))
    tail = (n, _lib.dptr(t), _lib.dptr(c), int(slices), _lib.dptr(term), _lib.dptr(fp), _lib.dptr(fpint))
    if w is None:
        rc = lib.mvus_spline_fit_residual(int(device), m, _lib.dptr(u), _lib.dptr(X), *tail)
    else:
        w = _weights(w, m)
        rc = lib.mvus_spline_fit_residual_w(int(device), m, _lib.dptr(u), _lib.dptr(X), _lib.dptr(w), *tail)
    if rc != 0:
        _err(lib, rc, 'mvus_spline_fit_residual' if w is None else 'mvus_spline_fit_residual_w')
    return SimpleNamespace(term=term, fp=float(fp[0]), fpint=fpint)


def _fprati(p1, f1, p2, f2, p3, f3):
    """FITPACK fprati: the zero of the rational interpolant r(p) = (u p + v) / (p + w) through three points (p3 < 0: p3 = inf)."""
    if p3 > 0.0:
        h1, h2, h3 = f1 * (f2 - f3), f2 * (f3 - f1), f3 * (f1 - f2)
        p = -(p1 * p2 * h3 + p2 * p3 * h1 + p3 * p1 * h2) / (p1 * h1 + p2 * h2 + p3 * h3)
    else:
        p = (p1 * (f1 - f3) * f2 - p2 * (f2 - f3) * f1) / ((f1 - f2) * f3)
    if f2 < 0.0:
        p3, f3 = p2, f2
    else:
        p1, f1 = p2, f2
    return p, p1, f1, p3, f3


def linear_fit_as_cubic(part, s):
    """The reference's fallback for a part with fewer than four samples (common.py:266-267): ``splprep(k=3)`` raises there
    (it needs m > k) and the bare ``except`` calls ``splprep(X, u=t, s=s, k=1)`` instead.  Through ``find_intervals`` only
    m = 3 can occur (two gaps < 5 spanning >= 5 time units).  This is FITPACK's ``fppara`` for k = 1 written out for that
    size (scipy 1.15.3, third party -- not under /root/reference; same flow, tolerances and iteration as the k = 3 case the
    GPU runs): the least-squares line if its squared residual is below s; otherwise one knot at the middle sample, and
    -- the interpolating polyline then has residual 0 < s -- the smoothing spline between the two with residual s, its
    parameter p found by fppara's own rational iteration (same starting value, brackets and stopping rule, so the same p).
    With the three linear B-splines being 1 at their own sample the observation matrix is the identity, which makes every
    step closed form: c(p) = x - b (b.x) / (p^2 + b.b), b = the derivative-jump row of ``fpdisc``.

    The kernels of this library evaluate CUBIC splines only, so the piecewise-linear curve is returned degree-elevated: the
    same curve, point for point, as a cubic tck (knots [a x4, b x4], or [a x4, u2 x3, b x4] for the bent one).  Documented
    divergence: ``tck[2]`` is 3 where the reference stores 1, and the knot / coefficient arrays differ accordingly; every
    evaluation (spline_to_traj, the BA residual) gives the reference's values.

    Unweighted: a weighted ``traj_fit`` fits such a part at unit weights too (three samples, a host restatement of the k = 1 case)."""
    part = np.asarray(part, dtype=np.float64)
    m = part.shape[1]
    u, X = part[0], part[1:]
    if m < 2:
        raise ValueError('traj_to_spline: a trajectory part with a single sample cannot be fitted (the reference raises too: splprep needs m > k)')
    a, b = u[0], u[-1]
    if m == 2:                                                        # nmax == nmin: the interpolating segment
        P, breaks = [X[:, 0], X[:, 1]], [a, b]
    elif m == 3:
        tol, maxit = 0.001, 20
        acc = tol * s
        lam = (u - a) / (b - a)
        A = np.column_stack((1.0 - lam, lam))
        c, *_ = np.linalg.lstsq(A, X.T, rcond=None)                  # (2, 3): values of the least-squares line at a and b
        fp0 = float(np.sum((A @ c - X.T) ** 2))
        if abs(fp0 - s) < acc or fp0 < s:                              # fppara: |fp - s| < acc, or fp < s with no interior knot (ier = -2)
            P, breaks = [c[0], c[1]], [a, b]
        else:
            fac = 2.0 / (b - a)                                        # fpdisc, k = 1, knots [a, a, u2, b, b]
            bj = np.array([1.0 / ((u[1] - a) * fac), (b - a) / ((u[1] - a) * (u[1] - b) * fac), 1.0 / ((b - u[1]) * fac)])
            bb, w = float(bj @ bj), X @ bj
            W = float(w @ w)
            F = lambda p: bb * W / (p * p + bb) ** 2                   # noqa: E731  residual of the smoothing spline with parameter p
            p1, f1, p3, f3 = 0.0, fp0 - s, -1.0, -s
            p = 1.0                                                    # nk1 / sum of the triangle's diagonal (three ones)
            ich1 = ich3 = 0
            for iteration in range(1, maxit + 1):
                f2 = F(p) - s
                if abs(f2) < acc or iteration == maxit:
                    break
                p2 = p
                if ich3 == 0:
                    if f2 - f3 <= acc:                                 # the initial choice of p is too large
                        p3, f3 = p2, f2
                        p = p * 0.04
                        if p <= p1:
                            p = p1 * 0.9 + p2 * 0.1
                        continue
                    if f2 < 0.0:
                        ich3 = 1
                if ich1 == 0:
                    if f1 - f2 <= acc:                                 # the initial choice of p is too small
                        p1, f1 = p2, f2
                        p = p / 0.04
                        if p3 >= 0.0 and p >= p3:
                            p = p2 * 0.1 + p3 * 0.9
                        continue
                    if f2 > 0.0:
                        ich1 = 1
                if f2 >= f1 or f2 <= f3:
                    break                                              # (fppara: ier = 2, keeps the current spline)
                p, p1, f1, p3, f3 = _fprati(p1, f1, p2, f2, p3, f3)
            Cp = X - np.outer(w, bj) / (p * p + bb)
            P, breaks = [Cp[:, 0], Cp[:, 1], Cp[:, 2]], [a, u[1], b]
    else:
        raise ValueError('linear_fit_as_cubic is the fallback for parts with fewer than four samples')
    knots = [breaks[0]] * 4
    coefs = [P[0]]
    for j in range(1, len(P)):
        d = P[j] - P[j - 1]
        coefs += [P[j - 1] + d / 3.0, P[j - 1] + 2.0 * d / 3.0, P[j]]
        knots += [breaks[j]] * (3 if j < len(P) - 1 else 4)
    C = np.array(coefs).T
    return [np.array(knots, dtype=np.float64), [C[0].copy(), C[1].copy(), C[2].copy()], 3]


def traj_fit(part, smooth_factor, device=0, w=None):
    """One interval of ``Scene.traj_to_spline`` (reference common.py:236-262): ``part`` = [t; x; y; z] (4, m).  The smoothing
    factor starts at 1e-6 * duration and is divided by 1.5 / doubled until duration / #coefficients lies between the two
    ``smooth_factor`` bounds (or the fit is down to 4 coefficients and still too dense).  Returns the tck.  ``w``: one weight per
    sample as in ``smooth_fit``; only their ratios matter here, since the loop rescales s until the knot density fits.  A part of
    fewer than four samples is fitted without them (``linear_fit_as_cubic``)."""
    lo, hi = min(smooth_factor), max(smooth_factor)
    part = np.ascontiguousarray(part, dtype=np.float64)     # once, not in each of the dozen fits below (a column slice of the trajectory is strided)
    measure = part[0, -1] - part[0, 0]
    s = (1e-3) ** 2 * measure
    if part.shape[1] < 4:                        # splprep(k=3) raises -> the reference's k=1 fallback (common.py:266-267)
        return linear_fit_as_cubic(part, s)
    prev, direction = 0, 0
    with SmoothFit(part[0], part[1:], device=device, w=w) as fit:       # one upload for the dozen fits of the loop
        while True:
            tck = fit(s)
            n = len(tck[0]) - 4
            if n == prev and n == 4 and direction == 2:
                break
            prev = n
            if measure / n > hi:
                s, direction = s / 1.5, 1
            elif measure / n < lo:
                s, direction = s * 2, 2
            else:
                break
    return tck
