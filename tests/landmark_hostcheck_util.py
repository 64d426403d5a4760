"""Build/load the TEST-ONLY host build of the landmark row routine (tests/landmark_hostcheck.cpp), the way priors_hostcheck_util.load
does it for the position priors."""
import ctypes
import os
import subprocess

import numpy as np

from mvus_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, 'landmark_hostcheck.cpp')
DEPS = [SRC] + [os.path.join(ROOT, 'mvus_amd', 'csrc', f) for f in ('ba_landmark_math.h', 'ba_math.h')]
SO = os.path.join(HERE, 'liblandmarkcheck.so')                  # (next to its source; *.so is ignored by git)

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
    lib.landmarkcheck_row.restype = None
    lib.landmarkcheck_row.argtypes = [ctypes.c_int, ctypes.c_int] + [_lib.c_double_p] * 8
    lib.landmarkcheck_entries.argtypes = [ctypes.c_int]
    lib.landmarkcheck_entry.restype = None
    lib.landmarkcheck_entry.argtypes = [ctypes.c_int, ctypes.c_int, _lib.c_int32_p, _lib.c_int32_p]
    _cached = lib
    return lib


def row(calib, undist, K4, d5, params, X, uv, w):
    """(r[2], J[2, P]) of the host build of landmark_row"""
    lib = load()
    a = [np.ascontiguousarray(v, dtype=np.float64) for v in (K4, d5, params, X, uv, w)]
    P = 15 if calib else 6
    r, J = np.zeros(2), np.zeros((2, P))
    lib.landmarkcheck_row(int(calib), int(undist), *[_lib.dptr(v) for v in a], _lib.dptr(r), _lib.dptr(J))
    return r, J


def entries(P):
    lib = load()
    out = []
    a, b = ctypes.c_int32(0), ctypes.c_int32(0)
    for e in range(lib.landmarkcheck_entries(P)):
        lib.landmarkcheck_entry(P, e, ctypes.byref(a), ctypes.byref(b))
        out.append((a.value, b.value))
    return out
