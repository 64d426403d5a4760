"""The C-ABI library builds, loads, and exports every symbol include/mvus_ba.h declares (no GPU needed)."""
import ctypes
import os
import re

import pytest

from mvus_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as ge
    ge.build()
    return _lib.load()


def test_header_and_binding_agree(lib):
    hdr = open(os.path.join(ROOT, 'include', 'mvus_ba.h')).read()
    declared = set(re.findall(r'\b(mvus_[a-z_0-9]+)\s*\(', hdr)) - {'mvus_allreduce_fn'}
    bound = {name for name, _, _ in _lib.API}
    assert declared == bound, (declared ^ bound)
    for name in declared:
        assert hasattr(lib, name)


def test_struct_sizes_match_header(lib):
    # natural alignment of the C structs (see include/mvus_ba.h)
    assert ctypes.sizeof(_lib.MvusSolveOpts) == 88
    assert ctypes.sizeof(_lib.MvusResult) == 48
    assert ctypes.sizeof(_lib.MvusProblem) == 144


def test_default_opts_are_scipy_defaults(lib):
    o = _lib.MvusSolveOpts()
    lib.mvus_default_opts(ctypes.byref(o))
    assert (o.max_nfev, o.ftol, o.xtol, o.gtol) == (10, 1e-8, 1e-12, 1e-8)
    assert (o.lsmr_atol, o.lsmr_btol, o.lsmr_conlim) == (1e-6, 1e-6, 1e8)


def test_invalid_problem_is_rejected_before_touching_the_gpu(lib):
    from golden_util import load_case
    from mvus_amd import problem as mp
    scene, _ = load_case('c1_pinhole_2cam')
    prob, _ = mp.problem_from_scene(scene)
    prob.interval = prob.interval[::-1].copy()
    s, keep = _lib.make_problem_struct(prob)
    h = ctypes.c_void_p()
    rc = lib.mvus_ba_create(ctypes.byref(s), ctypes.byref(h))
    assert rc == _lib.MVUS_E_INVALID and not h
    assert b'interval' in lib.mvus_last_error(None)


def test_no_gpu_means_error_not_fallback(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip('a GPU is present')
    from golden_util import load_case
    from mvus_amd import problem as mp
    scene, _ = load_case('c1_pinhole_2cam')
    prob, _ = mp.problem_from_scene(scene)
    s, keep = _lib.make_problem_struct(prob)
    h = ctypes.c_void_p()
    rc = lib.mvus_ba_create(ctypes.byref(s), ctypes.byref(h))
    assert rc == _lib.MVUS_E_HIP and not h


def test_bad_arguments_in_every_unit_reach_the_one_error_string(lib):
    """The library is three translation units with ONE thread-local string behind mvus_last_error(NULL): a failure in the spline
    unit, in the two-view unit and in the BA unit each leaves that function's own message there, whichever failed last."""
    import numpy as np
    z = np.zeros(12)
    rc = lib.mvus_spline_eval(0, 0, _lib.dptr(z), None, _lib.dptr(z), _lib.dptr(z), 0, None, None, None)
    assert rc == _lib.MVUS_E_INVALID
    assert lib.mvus_last_error(None) == b'spline_eval: bad arguments'
    rc = lib.mvus_triangulate(0, -1, None, None, _lib.dptr(z), _lib.dptr(z), None, None, None)
    assert rc == _lib.MVUS_E_INVALID
    assert lib.mvus_last_error(None) == b'triangulate: bad arguments'
    rc = lib.mvus_group_columns(1, 0, 0, None, None, None, None)
    assert rc == _lib.MVUS_E_INVALID
    assert lib.mvus_last_error(None) == b'group_columns: bad arguments'
    rc = lib.mvus_spline_eval(0, 0, _lib.dptr(z), None, _lib.dptr(z), _lib.dptr(z), 0, None, None, None)
    assert rc == _lib.MVUS_E_INVALID
    assert lib.mvus_last_error(None) == b'spline_eval: bad arguments'


def test_no_gpu_means_error_in_every_unit(lib):
    """Without a GPU a valid call into the spline unit and into the two-view unit fails with MVUS_E_HIP and says so through
    mvus_last_error(NULL), as mvus_ba_create does (test_no_gpu_means_error_not_fallback)."""
    import numpy as np
    import torch
    if torch.cuda.is_available():
        pytest.skip('a GPU is present')
    interval = np.array([0.0, 1.0])
    koff = np.array([0, 8], np.int64)
    knots = np.array([0.0, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 1.0])
    coefs = np.arange(12, dtype=float)
    t, X, which = np.array([0.5]), np.zeros(3), np.zeros(1, np.int32)
    lib.mvus_triangulate(0, -1, None, None, None, None, None, None, None)          # another message first
    rc = lib.mvus_spline_eval(0, 1, _lib.dptr(interval), koff.ctypes.data_as(_lib.c_int64_p), _lib.dptr(knots), _lib.dptr(coefs), 1,
                              _lib.dptr(t), _lib.dptr(X), which.ctypes.data_as(_lib.c_int32_p))
    assert rc == _lib.MVUS_E_HIP
    assert b'no usable HIP device' in lib.mvus_last_error(None)
    x1, x2, Xh = np.array([0.1, 0.2]), np.array([0.0, 0.2]), np.zeros(4)
    P1 = np.hstack([np.eye(3), np.zeros((3, 1))]).ravel()
    P2 = np.hstack([np.eye(3), np.array([[-1.0], [0.0], [0.0]])]).ravel()
    lib.mvus_spline_eval(0, 0, None, None, None, None, 0, None, None, None)      # another message first
    assert lib.mvus_last_error(None) == b'spline_eval: bad arguments'
    rc = lib.mvus_triangulate(0, 1, _lib.dptr(x1), _lib.dptr(x2), _lib.dptr(P1), _lib.dptr(P2), _lib.dptr(Xh), None, None)
    assert rc == _lib.MVUS_E_HIP
    assert b'no usable HIP device' in lib.mvus_last_error(None)
