"""Robust losses (mvus_ba_set_loss), the part that needs no GPU: the scipy wrapper every GPU check of tests/test_gpu_robust_loss.py
leans on is pinned against the closed forms of the five losses; the settings of Scene.BA are validated before any library call; the
binding's constants are the header's."""
import os
import re

import numpy as np
import pytest

import robust_reference as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rows(seed=3, m=400, n=7):
    """Residuals from far inside to far outside f_scale, with the rows the fixtures have: exact zeros (detections outside every
    interval) and, for f_scale = 3, rows exactly ON the huber knee z = 1."""
    rng = np.random.default_rng(seed)
    f = np.concatenate([rng.standard_normal(m) * 2.0, rng.standard_normal(40) * 60.0, np.zeros(9), [3.0, -3.0, 3.0]])
    J = rng.standard_normal((f.size, n))
    J[-12:-3] = 0.0                        # zero rows of the Jacobian go with zero residuals
    return f, J


@pytest.mark.parametrize('f_scale', [1.0, 3.0, 0.37])
@pytest.mark.parametrize('loss', rr.LOSSES)
def test_scipy_wrapper_equals_closed_forms(loss, f_scale):
    f, J = _rows()
    cost, grad, Js = rr.scipy_at(f, J, loss, f_scale)
    s, d1 = rr.closed_scale(f, loss, f_scale)
    assert abs(cost - rr.closed_cost(f, loss, f_scale)) <= 4e-15 * cost
    g_ref = J.T @ (d1 * f)
    assert np.max(np.abs(grad - g_ref)) <= 4e-15 * np.sum(np.abs(J) * np.abs(d1 * f)[:, None], axis=0).max()
    # huber beyond the knee: rho' + 2 rho'' z is zero analytically; computed, it is rounding noise of a few EPS rho' around zero and the
    # scale is the square root of max(that, EPS) -- defined in size only (<= a few sqrt(EPS): nothing next to the rows with s ~ 1)
    flat = (loss == 'huber') & (np.abs(f) > f_scale)
    assert np.max(np.abs(Js - s[:, None] * J)[~flat]) <= 4e-15 * np.abs(J).max()
    if flat.any():
        assert np.all(np.abs(Js[flat]) <= np.sqrt(8 * rr.EPS) * np.abs(J[flat])) and np.all(np.abs(Js[flat]) >= np.sqrt(rr.EPS) * np.abs(J[flat]))
    if loss == 'huber' and f_scale == 3.0:
        assert np.array_equal(d1[-3:], np.ones(3)) and np.array_equal(s[-3:], np.ones(3))       # z = 1: still the quadratic branch
        assert np.all(s[np.abs(f) > 3.0] == np.sqrt(rr.EPS))                                   # beyond: rho' + 2 rho'' z = 0
    if loss != 'linear':
        assert np.all(d1[f == 0] == 1.0) and np.all(s[f == 0] == 1.0)


@pytest.mark.parametrize('loss', rr.ROBUST)
def test_wrapper_hands_scipy_a_fresh_jacobian_every_call(loss):
    """scipy scales a dense Jacobian in place: a wrapper that returned the caller's array would answer differently the second time."""
    f, J = _rows(seed=5)
    J0 = J.copy()
    first = rr.scipy_at(f, J, loss, 3.0)
    again = rr.scipy_at(f, J, loss, 3.0)
    assert np.array_equal(J, J0)
    for a, b in zip(first, again):
        assert np.array_equal(a, b)
    assert rr.scipy_cost(f, loss, 3.0) == first[0]


def test_binding_constants_are_the_headers():
    from mvus_amd import _lib, ba
    hdr = open(os.path.join(ROOT, 'include', 'mvus_ba.h')).read()
    defs = {k: int(v) for k, v in re.findall(r'#define\s+MVUS_LOSS_([A-Z_0-9]+)\s+(\d+)', hdr)}
    assert defs == {'LINEAR': 0, 'SOFT_L1': 1, 'HUBER': 2, 'CAUCHY': 3, 'ARCTAN': 4}
    for name, code in defs.items():
        assert getattr(_lib, 'LOSS_' + name) == code and _lib.LOSS_NAMES[name.lower()] == code
    assert int(re.search(r'#define\s+MVUS_ABI_VERSION\s+(\d+)', hdr).group(1)) == _lib.ABI_VERSION == 8
    assert ba.loss_code('huber') == 2 and ba.loss_code(3) == 3
    with pytest.raises(ValueError, match='tukey'):
        ba.loss_code('tukey')


def _scene(**settings):
    from golden_util import load_case
    from test_gpu_scene import build_scene
    scene, g = load_case('rs_F_2int_3cam')
    s = build_scene(scene)
    s.settings.update(settings)
    return s, scene.settings


@pytest.mark.parametrize('settings,key', [
    (dict(ba_solver='lm', ba_loss='tukey'), 'ba_loss'),
    (dict(ba_solver='lm', ba_loss=2), 'ba_loss'),
    (dict(ba_solver='lm', ba_loss='huber', ba_f_scale=0.0), 'ba_f_scale'),
    (dict(ba_solver='lm', ba_loss='huber', ba_f_scale=-1.5), 'ba_f_scale'),
    (dict(ba_solver='lm', ba_loss='huber', ba_f_scale=float('nan')), 'ba_f_scale'),
    (dict(ba_solver='lm', ba_loss='huber', ba_f_scale='3'), 'ba_f_scale'),
    (dict(ba_solver='trf', ba_loss='huber'), 'ba_loss'),
    (dict(ba_loss='cauchy', ba_f_scale=3.0), 'ba_loss'),                       # (ba_solver absent = 'trf')
    (dict(ba_solver='lm', ba_jacobian='pattern', ba_loss='huber'), 'ba_loss'),
])
def test_bad_loss_settings_raise_before_any_library_call(settings, key, monkeypatch):
    from mvus_amd.reconstruction import common
    s, st = _scene(**settings)

    def no_handle(self, prob):
        raise AssertionError('Scene.BA reached the library with bad settings')
    monkeypatch.setattr(common.Scene, '_handle', no_handle)
    with pytest.raises(ValueError, match=key):
        s.ba_mode()
    with pytest.raises(ValueError, match=key):
        s.BA(s.numCam, rs=st['rolling_shutter'], motion_reg=st['motion_reg'], motion_weights=st['motion_weights'], rs_bounds=st['rs_bounds'])


def test_reference_settings_mean_linear():
    """A reference config.json has neither key: linear, 1.0 -- and the solver choice is what it was."""
    from mvus_amd import ba
    s, _ = _scene()
    assert 'ba_loss' not in s.settings and 'ba_f_scale' not in s.settings
    assert s.ba_loss() == (ba.LOSS_LINEAR, 1.0)
    assert s.ba_mode() == (ba.SOLVER_TRF_LSMR, ba.JAC_FD)
    s.settings.update(ba_solver='lm', ba_loss='huber', ba_f_scale=3)
    assert s.ba_loss() == (ba.LOSS_HUBER, 3.0)
    assert s.ba_mode() == (ba.SOLVER_LM_SCHUR, ba.JAC_ANALYTIC)
    s.settings.update(ba_solver='trf', ba_loss='linear', ba_f_scale=2.0)      # linear with TRF stays allowed
    assert s.ba_loss() == (ba.LOSS_LINEAR, 2.0)
