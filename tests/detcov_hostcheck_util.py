"""Build/load the TEST-ONLY host build of the per-detection covariance's row routines (tests/detcov_hostcheck.cpp), the way
priors_hostcheck_util does it for the position priors."""
import ctypes
import os
import subprocess

import numpy as np

from mvus_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, 'detcov_hostcheck.cpp')
DEPS = [SRC] + [os.path.join(ROOT, 'mvus_amd', 'csrc', f) for f in ('ba_detcov_math.h', 'ba_math.h')]
SO = os.path.join(HERE, 'libdetcovcheck.so')                   # (next to its source; *.so is ignored by git)

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
    d = _lib.c_double_p
    lib.detcheck_row.restype = ctypes.c_int
    lib.detcheck_row.argtypes = [ctypes.c_int, d, d, d, d, d, ctypes.c_longlong, d, ctypes.c_longlong, d, d, d]
    lib.detcheck_image_axes.restype = None
    lib.detcheck_image_axes.argtypes = [d, ctypes.c_double, ctypes.c_double, d]
    lib.detcheck_t2.restype = ctypes.c_double
    lib.detcheck_t2.argtypes = [d, ctypes.c_double, ctypes.c_double, ctypes.c_double]
    _cached = lib
    return lib


def row(a, b, Scc, T, band):
    """detcov_row: a [2, B], b [2, 12], Scc [B, >= B] (rows may be longer: the leading dimension is its row length), T [12, >= B],
    band [4, 4, 3, 3] (blocks (p + a, p + a + w) of four consecutive control points) -> (pi [3], terms [3, 3])."""
    lib = load()
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    Scc, T = np.ascontiguousarray(Scc, dtype=np.float64), np.ascontiguousarray(T, dtype=np.float64)
    band = np.ascontiguousarray(band, dtype=np.float64)
    assert b.shape == (2, 12) and T.shape[0] == 12 and band.shape == (4, 4, 3, 3)
    pi, terms = np.empty(3), np.empty((3, 3))
    rc = lib.detcheck_row(a.shape[1], _lib.dptr(a[0]), _lib.dptr(a[1]), _lib.dptr(b[0]), _lib.dptr(b[1]), _lib.dptr(Scc), Scc.shape[1],
                          _lib.dptr(T), T.shape[1], _lib.dptr(band), _lib.dptr(pi), _lib.dptr(terms))
    assert rc == 0, 'detcheck_row: B = %d is not built' % a.shape[1]
    return pi, terms


def image_axes(pi, su, sv):
    p = np.empty(3)
    load().detcheck_image_axes(_lib.dptr(np.ascontiguousarray(pi, dtype=np.float64)), float(su), float(sv), _lib.dptr(p))
    return p


def t2(pi, sigma2, ru, rv):
    return float(load().detcheck_t2(_lib.dptr(np.ascontiguousarray(pi, dtype=np.float64)), float(sigma2), float(ru), float(rv)))
