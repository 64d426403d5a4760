"""Build/load the TEST-ONLY host build of the iterative time-shift search's lane routines (tests/sync_iter_hostcheck.cpp), the way
detcov_hostcheck_util does it for the per-detection covariance."""
import ctypes
import os
import subprocess

import numpy as np

from mvus_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, 'sync_iter_hostcheck.cpp')
DEPS = [SRC] + [os.path.join(ROOT, 'mvus_amd', 'csrc', f) for f in ('sync_iter_math.h', 'epipolar.hip.h', 'pnp.hip.h', 'ba_math.h')]
SO = os.path.join(HERE, 'libsynciter_check.so')               # (next to its source; *.so is ignored by git)

_cached = None


def load():
    global _cached
    if _cached is not None:
        return _cached
    if (not os.path.exists(SO)) or os.path.getmtime(SO) < max(os.path.getmtime(d) for d in DEPS):
        tmp = '%s.%d.tmp' % (SO, os.getpid())                 # (built aside and renamed: two test processes may get here together)
        subprocess.check_call(['g++', '-O2', '-std=c++17', '-ffp-contract=off', '-shared', '-fPIC', '-o', tmp, SRC])
        os.replace(tmp, SO)
    lib = ctypes.CDLL(SO)
    d, ll = _lib.c_double_p, ctypes.c_longlong
    lib.sicheck_sample9.restype = None
    lib.sicheck_sample9.argtypes = [ctypes.c_uint64, ctypes.c_int, ctypes.c_int, ctypes.c_int, ll, ctypes.POINTER(ll)]
    lib.sicheck_betas.restype = ctypes.c_int
    lib.sicheck_betas.argtypes = [d, d, d, d]
    lib.sicheck_eig6.restype = ctypes.c_int
    lib.sicheck_eig6.argtypes = [d, d]
    lib.sicheck_fundamental.restype = ctypes.c_int
    lib.sicheck_fundamental.argtypes = [d, d, d]
    lib.sicheck_spline.restype = None
    lib.sicheck_spline.argtypes = [d, d, ctypes.c_int, ll, d, d]
    lib.sicheck_span.restype = ctypes.c_int
    lib.sicheck_span.argtypes = [d, ctypes.c_int, ctypes.c_double, ctypes.c_int]
    lib.sicheck_sampson.restype = ctypes.c_double
    lib.sicheck_sampson.argtypes = [d] + [ctypes.c_double] * 4
    lib.sicheck_in_intervals.restype = ctypes.c_int
    lib.sicheck_in_intervals.argtypes = [d, ctypes.c_int, ctypes.c_double]
    _cached = lib
    return lib


def _c(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def sample9(seed, rnd, sign, h, n):
    idx = (ctypes.c_longlong * 9)()
    load().sicheck_sample9(int(seed), int(rnd), int(sign), int(h), int(n), idx)
    return list(idx)


def betas(s1, s2, ds):
    """s1, s2, ds: 2 x 9 -> the ascending finite real beta of the pencil."""
    s1, s2, ds = _c(s1), _c(s2), _c(ds)
    out = np.zeros(6)
    n = load().sicheck_betas(_lib.dptr(s1), _lib.dptr(s2), _lib.dptr(ds), _lib.dptr(out))
    return out[:n]


def eig6(a):
    """The real eigenvalues of a 6 x 6 matrix, ascending (None: the QR iteration did not converge)."""
    a = _c(a)
    assert a.shape == (6, 6)
    out = np.zeros(6)
    n = load().sicheck_eig6(_lib.dptr(a), _lib.dptr(out))
    return None if n < 0 else np.sort(out[:n])


def fundamental(x1, x2):
    x1, x2 = _c(x1), _c(x2)
    F = np.zeros(9)
    ok = load().sicheck_fundamental(_lib.dptr(x1), _lib.dptr(x2), _lib.dptr(F))
    return F.reshape(3, 3) if ok else None


def spline(tck, u):
    t, c = _c(tck[0]), _c(np.vstack(tck[1]))
    u = _c(np.atleast_1d(u))
    out = np.empty((2, u.size))
    load().sicheck_spline(_lib.dptr(t), _lib.dptr(c), c.shape[1], u.size, _lib.dptr(u), _lib.dptr(out))
    return out


def span(t, n, u, guess):
    return load().sicheck_span(_lib.dptr(_c(t)), int(n), float(u), int(guess))


def sampson(F, u1, v1, u2, v2):
    return load().sicheck_sampson(_lib.dptr(_c(F).reshape(9)), float(u1), float(v1), float(u2), float(v2))


def in_intervals(intervals, tau):
    """intervals 2 x K (find_intervals' layout): start <= tau < end for one of them."""
    iv = _c(np.asarray(intervals, dtype=np.float64).T)
    return bool(load().sicheck_in_intervals(_lib.dptr(iv), iv.shape[0], float(tau)))
