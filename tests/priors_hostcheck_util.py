"""Build/load the TEST-ONLY host build of the position priors' row routines (tests/priors_hostcheck.cpp), the way hostcheck_util.load
does it for the rest of the device math."""
import ctypes
import os
import subprocess

import numpy as np

from mvus_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, 'priors_hostcheck.cpp')
DEPS = [SRC] + [os.path.join(ROOT, 'mvus_amd', 'csrc', f) for f in ('ba_prior_math.h', 'ba_math.h')]
SO = os.path.join(HERE, 'libpriorscheck.so')                   # (next to its source; *.so is ignored by git)

_cached = None


def load():
    global _cached
    if _cached is not None:
        return _cached
    if (not os.path.exists(SO)) or os.path.getmtime(SO) < max(os.path.getmtime(d) for d in DEPS):
        tmp = '%s.%d.tmp' % (SO, os.getpid())                 # (built aside and renamed: two test processes may get here together)
        subprocess.check_call(['g++', '-O2', '-std=c++17', '-shared', '-fPIC', '-o', tmp, SRC])
        os.replace(tmp, SO)
    lib = ctypes.CDLL(SO)
    lib.priorcheck_setup.restype = None
    lib.priorcheck_setup.argtypes = [ctypes.c_int, _lib.c_double_p, _lib.c_int32_p, _lib.c_int32_p, _lib.c_double_p, ctypes.c_longlong,
                                     _lib.c_double_p, _lib.c_int32_p, _lib.c_double_p]
    lib.priorcheck_diff.restype = None
    lib.priorcheck_diff.argtypes = [_lib.c_double_p, _lib.c_int32_p, _lib.c_int32_p, _lib.c_double_p, _lib.c_double_p, _lib.c_double_p]
    _cached = lib
    return lib


def setup_rows(prob, t):
    """(ctrl[K], h[K, 4]) of k_prior_setup's row routine for the splines of BAProblem ``prob`` at the times ``t``."""
    lib = load()
    t = np.ascontiguousarray(t, dtype=np.float64)
    interval = np.ascontiguousarray(prob.interval, dtype=np.float64)
    koff = np.ascontiguousarray(prob.knot_offsets, dtype=np.int32)
    coff = np.ascontiguousarray(prob.ctrl_offsets, dtype=np.int32)
    knots = np.ascontiguousarray(prob.knots, dtype=np.float64)
    ctrl = np.empty(t.size, dtype=np.int32)
    h = np.empty((t.size, 4))
    i32 = lambda a: a.ctypes.data_as(_lib.c_int32_p)
    lib.priorcheck_setup(prob.S, _lib.dptr(interval), i32(koff), i32(coff), _lib.dptr(knots), t.size, _lib.dptr(t), i32(ctrl), _lib.dptr(h))
    return ctrl, h
