"""The weighted trajectory fit without a GPU: the new entry points are declared, bound and exported, the ABI version stays, what they
refuse is refused before a device is touched, and the host side of settings['traj_weights'] (the weights from the sigmas, the settings'
checks, the pickle's keys)."""
import ctypes
import os
import pickle
import re

import numpy as np
import pytest

from mvus_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('mvus_triangulate_cov', 'mvus_spline_fit_open_w', 'mvus_spline_smooth_w', 'mvus_spline_fit_normal_w', 'mvus_spline_fit_residual_w')


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as ge
    ge.build()
    return _lib.load()


def _prototype(hdr, name):
    m = re.search(r'\bint\s+%s\s*\(([^;]*)\);' % name, hdr)
    assert m, name + ' is not declared in include/mvus_ba.h'
    return [re.sub(r'\s+', ' ', a).strip() for a in m.group(1).split(',')]


def test_new_entry_points_are_declared_bound_and_exported(lib):
    hdr = open(os.path.join(ROOT, 'include', 'mvus_ba.h')).read()
    assert re.search(r'#define\s+MVUS_ABI_VERSION\s+8\b', hdr) and _lib.ABI_VERSION == 8
    assert lib.mvus_abi_sizes(None, None, None) == 8
    api = {name: (res, args) for name, res, args in _lib.API}
    ctype_of = {'int32_t': ctypes.c_int32, 'int64_t': ctypes.c_int64, 'double': ctypes.c_double, 'const double*': _lib.c_double_p, 'double*': _lib.c_double_p,
                'int32_t*': _lib.c_int32_p, 'int64_t*': _lib.c_int64_p, 'mvus_spline_fit**': ctypes.POINTER(ctypes.c_void_p)}
    for name in NEW:
        assert hasattr(lib, name) and api[name][0] is ctypes.c_int
        args = _prototype(hdr, name)
        types = [a.rsplit(' ', 1)[0] for a in args]
        assert [ctype_of[t] for t in types] == list(api[name][1]), name
        assert name in hdr.split('#define MVUS_ABI_VERSION')[0].rsplit('/*', 1)[1], name + ' is not in the list of added entry points'
    # a weighted call is the unweighted one with `const double* w` after X
    for plain in ('mvus_spline_fit_open', 'mvus_spline_smooth', 'mvus_spline_fit_normal', 'mvus_spline_fit_residual'):
        a, b = _prototype(hdr, plain), _prototype(hdr, plain + '_w')
        i = a.index('const double* X') + 1
        assert b == a[:i] + ['const double* w'] + a[i:]
    a, b = _prototype(hdr, 'mvus_triangulate'), _prototype(hdr, 'mvus_triangulate_cov')
    assert b == a[:6] + ['double sigma1', 'double sigma2', 'double* X', 'double* cov'] + a[7:]


def test_refusals_come_before_the_device(lib):
    """a bad weight, a bad sigma and cov == NULL are MVUS_E_INVALID with their own message whether or not a GPU is there"""
    m = 12
    u, X = np.arange(m, dtype=np.float64), np.zeros((3, m))
    n, fp, ier = ctypes.c_int32(0), ctypes.c_double(0.0), ctypes.c_int32(0)
    t, c = np.zeros(m + 6), np.zeros((3, m + 6))
    for bad in (0.0, -2.0, np.nan, np.inf):
        w = np.ones(m)
        w[5] = bad
        rc = lib.mvus_spline_smooth_w(0, m, _lib.dptr(u), _lib.dptr(X), _lib.dptr(w), 1.0, ctypes.byref(n), _lib.dptr(t), _lib.dptr(c), ctypes.byref(fp), ctypes.byref(ier))
        assert rc == _lib.MVUS_E_INVALID and b'weights must be finite and strictly positive' in lib.mvus_last_error(None)
        h = ctypes.c_void_p()
        rc = lib.mvus_spline_fit_open_w(0, m, _lib.dptr(u), _lib.dptr(X), _lib.dptr(w), ctypes.byref(h))
        assert rc == _lib.MVUS_E_INVALID and not h and b'weights' in lib.mvus_last_error(None)
    w = np.ones(m)
    for s in (0.0, -1.0, np.nan):
        rc = lib.mvus_spline_smooth_w(0, m, _lib.dptr(u), _lib.dptr(X), _lib.dptr(w), s, ctypes.byref(n), _lib.dptr(t), _lib.dptr(c), ctypes.byref(fp), ctypes.byref(ier))
        assert rc == _lib.MVUS_E_INVALID and b's > 0' in lib.mvus_last_error(None)
    x1, x2, P, Xh, cov = np.zeros((2, 3)), np.zeros((2, 3)), np.zeros(12), np.zeros((4, 3)), np.zeros((6, 3))
    for s1, s2 in ((0.0, 1.0), (1.0, -1.0), (np.nan, 1.0), (1.0, np.inf)):
        rc = lib.mvus_triangulate_cov(0, 3, _lib.dptr(x1), _lib.dptr(x2), _lib.dptr(P), _lib.dptr(P), s1, s2, _lib.dptr(Xh), _lib.dptr(cov), None, None)
        assert rc == _lib.MVUS_E_INVALID and b'sigma1 and sigma2 must be finite and > 0' in lib.mvus_last_error(None)
    rc = lib.mvus_triangulate_cov(0, 3, _lib.dptr(x1), _lib.dptr(x2), _lib.dptr(P), _lib.dptr(P), 1.0, 1.0, _lib.dptr(Xh), None, None, None)
    assert rc == _lib.MVUS_E_INVALID and b'cov is NULL' in lib.mvus_last_error(None)


def test_python_wrappers_check_the_length_of_w_before_the_library():
    from mvus_amd import spline
    u, X = np.arange(10.0), np.zeros((3, 10))
    for w in (np.ones(9), np.ones(11), np.ones((10, 1))):
        with pytest.raises(ValueError, match='one weight per sample'):
            spline._weights(w, u.size)
    assert spline._weights([1] * 10, 10).dtype == np.float64
    import inspect
    for fn in (spline.smooth_fit, spline.SmoothFit.__init__, spline.fit_normal, spline.fit_residual, spline.traj_fit):
        assert inspect.signature(fn).parameters['w'].default is None
    assert 'w' not in inspect.signature(spline.linear_fit_as_cubic).parameters and 'nweighted' in spline.linear_fit_as_cubic.__doc__


def test_weights_from_sigma_and_the_settings():
    from mvus_amd.reconstruction.common import Scene
    sig = np.array([0.04, 0.02, np.nan, 0.08, 400.0, 0.02, -1.0, np.inf])
    w = Scene.weights_from_sigma(sig, 1e-3)
    np.testing.assert_array_equal(w, [0.5, 1.0, 1e-3, 0.25, 1e-3, 1.0, 1e-3, 1e-3])
    np.testing.assert_array_equal(Scene.weights_from_sigma([np.nan, np.nan], 0.01), [0.01, 0.01])
    cov = np.stack([np.diag([1.0, 4.0, 7.0]), np.full((3, 3), np.nan)])
    np.testing.assert_array_equal(Scene.sigma_from_cov(cov), [2.0, np.nan])
    s = Scene()
    s.numCam = 3
    s.settings = {}
    assert s.traj_weights() is None
    s.settings = {'traj_weights': None}
    assert s.traj_weights() is None
    s.settings = {'traj_weights': 'triangulation'}
    mode, px, floor = s.traj_weights()
    assert mode == 'triangulation' and list(px) == [1.0, 1.0, 1.0] and floor == 1e-3
    s.settings.update(traj_sigma_px=[0.5, 1.0, 2.0], traj_weight_floor=0.01)
    assert list(s.traj_weights()[1]) == [0.5, 1.0, 2.0] and s.traj_weights()[2] == 0.01
    for bad in (dict(traj_weights='full'), dict(traj_sigma_px=[1.0, 2.0]), dict(traj_sigma_px=0.0), dict(traj_sigma_px=[1.0, np.nan, 1.0]), dict(traj_weight_floor=0.0),
                dict(traj_weight_floor=2.0)):
        s.settings = dict({'traj_weights': 'triangulation'}, **bad)
        with pytest.raises(ValueError, match='traj_'):
            s.traj_weights()


def test_pickle_carries_traj_sigma_only_when_set():
    from mvus_amd.reconstruction.common import Scene
    s = Scene()
    assert s.traj_sigma is None and 'traj_sigma' not in s.__getstate__()
    back = pickle.loads(pickle.dumps(s))
    assert back.traj_sigma is None
    s.traj_sigma = np.array([0.1, np.nan])
    assert np.array_equal(pickle.loads(pickle.dumps(s)).traj_sigma, s.traj_sigma, equal_nan=True)
    # a similarity scales the sigmas with the trajectory
    s.traj = np.vstack((np.arange(2.0), np.ones((3, 2))))
    s.spline = {'tck': [], 'int': []}
    s.apply_similarity(2.0, np.eye(3), np.zeros(3))
    np.testing.assert_array_equal(s.traj_sigma, [0.2, np.nan])
