"""Position priors on the trajectory, the parts that need no GPU: the set-up row routine of ba_prior_math.h (host build, against scipy's
design matrix), Scene.apply_similarity / align_to_position_priors against the oracle's residual, and the validation of the settings and of
the prior file before any GPU call."""
import json

import numpy as np
import pytest
from scipy.interpolate import BSpline

import priors_hostcheck_util as phc
import priors_reference as pref
from frozen_util import build_scene, packed
from golden_util import CASES, load_case
from mvus_amd import problem as mp
from mvus_amd.reconstruction import common
from mvus_amd.synth import rodrigues

EPS = np.finfo(np.float64).eps
FIXTURES = ['c1_pinhole_2cam', 'rs_F_2int_3cam']


def _edge_times(prob):
    """Every interior knot exactly, both ends of every interval exactly, a time between two intervals (or before the first), times outside
    all of them, repeated times, and a few hundred ordinary ones."""
    rng = np.random.default_rng(11)
    t = []
    for s in range(prob.S):
        kn = prob.knots[int(prob.knot_offsets[s]):int(prob.knot_offsets[s + 1])]
        t += list(kn[4:-4]) + [prob.interval[0, s], prob.interval[1, s]]
        t += list(rng.uniform(prob.interval[0, s], prob.interval[1, s], 150))
        t += [np.nextafter(prob.interval[1, s], -np.inf), np.nextafter(prob.interval[0, s], np.inf), kn[5], kn[5], 0.5 * (kn[6] + kn[7])] * 2
    gap = 0.5 * (prob.interval[1, 0] + prob.interval[0, 1]) if prob.S > 1 else prob.interval[0, 0] - 1.0
    t += [gap, prob.interval[0, 0] - 7.5, prob.interval[1, -1] + 0.25, np.nextafter(prob.interval[1, -1], np.inf),
          np.nextafter(prob.interval[0, 0], -np.inf)]
    return np.array(t, dtype=np.float64)


@pytest.mark.parametrize('name', FIXTURES)
def test_setup_row_routine_against_scipy_design_matrix(name):
    """1. The span (an integer: equal), the four weights (16 eps: a cubic basis value is at most nine dependent roundings) and the partition
    of unity (4 eps) of prior_setup_row on the fixture's knots, against scipy.interpolate.BSpline.design_matrix."""
    scene, _ = load_case(name)
    prob, _ = mp.problem_from_scene(scene)
    t = _edge_times(prob)
    ctrl, h = phc.setup_rows(prob, t)
    ctrl_ref, h_ref = pref.design(prob, t)
    inside = np.any((t[None, :] >= prob.interval[0][:, None]) & (t[None, :] <= prob.interval[1][:, None]), axis=0)
    assert np.array_equal(ctrl_ref >= 0, inside) and (~inside).sum() >= 5 and inside.sum() > 200
    assert np.array_equal(ctrl, ctrl_ref)
    assert not h[~inside].any()
    err = np.abs(h[inside] - h_ref[inside]).max()
    unity = np.abs(h[inside].sum(axis=1) - 1.0).max()
    print('%s: %d times, max |h - h_scipy| = %.3g (%.2f eps), max |sum h - 1| = %.3g (%.2f eps)' % (name, t.size, err, err / EPS, unity, unity / EPS))
    assert err <= 16 * EPS
    assert unity <= 4 * EPS
    # the right end of an interval is the last span with the right-end basis: all the weight on the last control point (the recurrence divides and multiplies by one knot difference: to rounding)
    for s in range(prob.S):
        k = int(np.nonzero(t == prob.interval[1, s])[0][0])
        assert ctrl[k] == prob.ctrl_offsets[s + 1] - 4 and np.abs(h[k] - [0.0, 0.0, 0.0, 1.0]).max() <= 4 * EPS
        k = int(np.nonzero(t == prob.interval[0, s])[0][0])
        assert ctrl[k] == prob.ctrl_offsets[s] and np.abs(h[k] - [1.0, 0.0, 0.0, 0.0]).max() <= 4 * EPS


def test_row_residual_matches_numpy():
    """prior_diff (what k_prior_cost and k_prior_ne evaluate per row) against the design-matrix product: 8 eps of the sum of |terms|."""
    scene, g = load_case('rs_F_2int_3cam')
    prob, x0 = mp.problem_from_scene(scene)
    lib = phc.load()
    t = _edge_times(prob)
    ctrl, h = phc.setup_rows(prob, t)
    col = pref.ctrl_columns(prob)
    rng = np.random.default_rng(2)
    from mvus_amd import _lib
    i32 = lambda a: a.ctypes.data_as(_lib.c_int32_p)
    x = np.ascontiguousarray(x0)
    for k in np.nonzero(ctrl >= 0)[0][::7]:
        x0i = np.ascontiguousarray(col[ctrl[k]:ctrl[k] + 4, 0], dtype=np.int32)
        st = np.ascontiguousarray(col[ctrl[k]:ctrl[k] + 4, 1] - col[ctrl[k]:ctrl[k] + 4, 0], dtype=np.int32)
        p = rng.standard_normal(3)
        diff = np.empty(3)
        hk = np.ascontiguousarray(h[k])
        lib.priorcheck_diff(_lib.dptr(x), i32(x0i), i32(st), _lib.dptr(hk), _lib.dptr(p), _lib.dptr(diff))
        pts = x[col[ctrl[k]:ctrl[k] + 4]]                  # [4, 3]
        ref = hk @ pts - p
        bar = 8 * EPS * (np.abs(hk) @ np.abs(pts) + np.abs(p))
        assert np.all(np.abs(diff - ref) <= bar)


def _similarity():
    rvec = np.array([0.3, -0.2, 0.17])
    rvec *= 0.4 / np.linalg.norm(rvec)
    T = np.array([3.0, -4.0, 0.0])
    return 1.7, rodrigues(rvec), T


@pytest.mark.parametrize('name', CASES)
def test_apply_similarity_keeps_every_image(name):
    """2. Scene.apply_similarity (s = 1.7, |rvec| = 0.4, |T| = 5): the oracle's detection residuals before and after agree to 1e-9 px, the
    project's residual-parity bar; alpha, beta, rs and the calibration are untouched."""
    from oracle import ba_oracle as orc
    scene, _ = load_case(name)
    oprob, _ = orc.problem_from_scene(scene, motion_reg=False)
    s = build_scene(scene, motion_reg=False)
    cams = list(range(scene.num_cam))
    prob, x0 = packed(s, cams)
    f0 = orc.residual(oprob, x0)
    sc, R, T = _similarity()
    assert abs(np.linalg.norm(T) - 5.0) < 1e-12
    before = [(c.K.copy(), c.d.copy()) for c in s.cameras]
    ctrl0 = [np.vstack(t[1]) for t in s.spline['tck']]
    s.apply_similarity(sc, R, T)
    x1 = s._pack(prob, cams)
    f1 = orc.residual(oprob, x1)
    assert f0.size == 2 * prob.M and np.abs(f0).max() > 0
    err = np.abs(f1 - f0).max()
    print('%s: max |f_after - f_before| = %.3g px' % (name, err))
    assert err <= 1e-9
    C = scene.num_cam
    assert np.array_equal(x1[:3 * C], x0[:3 * C])
    for c, (K, d) in zip(s.cameras, before):
        assert np.array_equal(c.K, K) and np.array_equal(c.d, d)
        assert np.allclose(c.P, c.K @ np.hstack((c.R, c.t.reshape(3, 1))), rtol=0, atol=0)
    for t, c0 in zip(s.spline['tck'], ctrl0):
        np.testing.assert_allclose(np.vstack(t[1]), sc * (R @ c0) + T[:, None], rtol=0, atol=1e-12 * np.abs(c0).max() * sc)


@pytest.mark.parametrize('name', FIXTURES)
def test_align_to_position_priors_recovers_a_known_similarity(name):
    """2. Priors generated as a known similarity of the spline's own points: (s, R, T) comes back to 1e-10, the rms is at most 1e-9 of the
    scene's size, and the scene has moved onto the priors.  Inactive priors (outside every interval) do not count."""
    scene, _ = load_case(name)
    s = build_scene(scene, motion_reg=False)
    prob, x0 = packed(s, list(range(scene.num_cam)))
    size = pref.scene_size(prob, x0)
    lo, hi = prob.interval[0, 0], prob.interval[1, -1]
    t_in = np.concatenate([np.linspace(prob.interval[0, k], prob.interval[1, k], 9) for k in range(prob.S)])
    X = pref.curve(prob, x0, t_in)
    sc, R, T = _similarity()
    P = sc * (R @ X) + T[:, None]
    t = np.concatenate((t_in, [hi + 5.0, lo - 1.0]))
    P = np.hstack((P, [[1e3, -1e3]] * 3))                     # two inactive rows that would wreck the fit if they were used
    s.position_priors = np.vstack((t, P, np.full((3, t.size), 0.01 * size)))
    s2, R2, T2, rms = s.align_to_position_priors()
    print('%s: |s - s0| = %.3g, |R - R0| = %.3g, |T - T0| = %.3g, rms / size = %.3g' % (name, abs(s2 - sc), np.abs(R2 - R).max(), np.abs(T2 - T).max(), rms / size))
    assert abs(s2 - sc) <= 1e-10 and np.abs(R2 - R).max() <= 1e-10 and np.abs(T2 - T).max() <= 1e-10 * max(1.0, np.abs(T).max())
    assert rms <= 1e-9 * size
    x1 = s._pack(prob, list(range(scene.num_cam)))
    np.testing.assert_allclose(pref.curve(prob, x1, t_in), P[:, :t_in.size], rtol=0, atol=1e-9 * size)


def test_align_needs_three_priors_that_are_not_collinear():
    scene, _ = load_case('c1_pinhole_2cam')
    s = build_scene(scene, motion_reg=False)
    prob, x0 = packed(s, [0, 1])
    lo, hi = prob.interval[0, 0], prob.interval[1, 0]
    sig = np.ones((3, 1))
    with pytest.raises(ValueError, match='at least 3'):
        s.align_to_position_priors()                                                      # none at all
    t = np.array([lo + 10.0, hi - 10.0])
    s.position_priors = np.vstack((t, pref.curve(prob, x0, t), np.repeat(sig, 2, axis=1)))
    with pytest.raises(ValueError, match='at least 3'):
        s.align_to_position_priors()                                                      # two
    t = np.array([lo + 10.0, hi - 10.0, lo + 20.0, hi + 50.0])                            # three active ones on a line + one inactive off it
    P = np.array([1.0, 2.0, 3.0])[:, None] + np.array([0.5, -1.0, 2.0])[:, None] * np.array([0.0, 1.0, 2.5, 0.0])[None, :]
    P[:, 3] = [7.0, -3.0, 1.0]
    s.position_priors = np.vstack((t, P, np.repeat(sig, 4, axis=1)))
    x_before = s._pack(prob, [0, 1])
    with pytest.raises(ValueError, match='collinear'):
        s.align_to_position_priors()
    assert np.array_equal(s._pack(prob, [0, 1]), x_before)                                 # a refused alignment moves nothing


def test_settings_are_validated_before_any_gpu_call(monkeypatch):
    """3. ba_position_priors with a solver other than 'lm', a flag that is no bool and a malformed Scene.position_priors raise ValueError
    from ba_mode -- which Scene.BA consults before it creates a handle."""
    scene, _ = load_case('c1_pinhole_2cam')
    monkeypatch.setattr(common.Scene, '_handle', lambda self, prob: pytest.fail('a GPU handle was created'))
    ok = np.vstack((np.array([[5.0, 6.0, 7.0]]), np.zeros((3, 3)), np.ones((3, 3))))
    for settings, pp in [(dict(ba_position_priors=True), ok),
                         (dict(ba_position_priors=True, ba_solver='trf'), ok),
                         (dict(ba_position_priors=1, ba_solver='lm'), ok),
                         (dict(ba_position_priors='yes', ba_solver='lm'), ok),
                         (dict(ba_position_priors=True, ba_solver='lm'), ok[:6]),
                         (dict(ba_position_priors=True, ba_solver='lm'), np.where(np.arange(7)[:, None] == 5, -1.0, ok)),
                         (dict(ba_position_priors=True, ba_solver='lm'), np.where(np.arange(7)[:, None] == 2, np.nan, ok))]:
        s = build_scene(scene, **settings)
        s.position_priors = pp
        with pytest.raises(ValueError, match='position'):
            s.BA(2, max_iter=3)
    s = build_scene(scene, ba_solver='lm', ba_position_priors=True)       # valid: an infinite sigma is an axis left out
    s.position_priors = np.where(np.arange(7)[:, None] == 6, np.inf, ok)
    t, P, sg = s.ba_position_priors()
    assert t.shape == (3,) and P.shape == (3, 3) and np.all(np.isinf(sg[2]))
    s = build_scene(scene, ba_solver='trf')                               # the flag off: the priors are ignored, whatever the solver
    s.position_priors = ok
    assert s.ba_position_priors() is None


def test_sigma_forms_of_the_binding():
    from mvus_amd.ba import position_prior_arrays
    t, P = np.array([1.0, 2.0]), np.arange(6.0).reshape(3, 2)
    for sigma, w in [(0.5, np.full((3, 2), 2.0)), ([1.0, 2.0, np.inf], np.array([[1.0, 1.0], [0.5, 0.5], [0.0, 0.0]])),
                     (np.array([[1.0, 4.0], [2.0, 2.0], [np.inf, 0.25]]), np.array([[1.0, 0.25], [0.5, 0.5], [0.0, 4.0]]))]:
        assert np.array_equal(position_prior_arrays(t, P, sigma)[2], w)
    for bad in (0.0, -1.0, np.nan, [1.0, 2.0], np.ones((2, 3))):
        with pytest.raises(ValueError):
            position_prior_arrays(t, P, bad)
    with pytest.raises(ValueError):
        position_prior_arrays(t, P.T, 1.0)


def _write_config(tmp_path, prior_lines, settings=None, sigma=None):
    det = tmp_path / 'det0.txt'
    det.write_text('100.0 200.0 1\n101.0 201.0 2\n')
    cam = tmp_path / 'cam0.json'
    cam.write_text(json.dumps({'K-matrix': np.eye(3).tolist(), 'distCoeff': [0, 0, 0, 0], 'fps': 30, 'resolution': [1920, 1080]}))
    pri = tmp_path / 'priors.txt'
    pri.write_text(prior_lines)
    st = dict(num_detections=100, ref_cam=0, camera_sequence=[0, 1], rolling_shutter=False, init_rs=0)
    st.update(settings or {})
    opt = {'path_position_priors': str(pri)}
    if sigma is not None:
        opt['position_prior_sigma'] = sigma
    cfg = {'necessary inputs': {'path_detections': [str(det), str(det)], 'path_cameras': [str(cam), str(cam)], 'corresponding_frames': [0, 0]},
           'optional inputs': opt, 'settings': st}
    path = tmp_path / 'config.json'
    path.write_text(json.dumps(cfg))
    return str(path)


def test_prior_file_is_read_and_validated_by_create_scene(tmp_path):
    """3. create_scene: columns t x y z [sigma_x sigma_y sigma_z]; a malformed file, a missing sigma and the flag with another solver raise
    there -- long before any GPU call."""
    lm = dict(ba_solver='lm', ba_position_priors=True)
    flight = common.create_scene(_write_config(tmp_path, '# t x y z sx sy sz\n1.5 1 2 3 0.1 0.1 0.2\n2.5 4 5 6 0.1 0.1 inf\n', lm))
    assert np.array_equal(flight.position_priors, np.array([[1.5, 2.5], [1, 4], [2, 5], [3, 6], [0.1, 0.1], [0.1, 0.1], [0.2, np.inf]]))
    flight = common.create_scene(_write_config(tmp_path, '1.5 1 2 3\n2.5 4 5 6\n', lm, sigma=0.05))
    assert np.array_equal(flight.position_priors[4:], np.full((3, 2), 0.05))
    flight = common.create_scene(_write_config(tmp_path, '1.5 1 2 3\n', lm, sigma=[0.1, 0.2, 0.3]))
    assert np.array_equal(flight.position_priors[4:, 0], [0.1, 0.2, 0.3])
    for text, sigma in [('1.5 1 2 3\n', None), ('1.5 1 2\n', 0.1), ('1.5 1 2 3 0.1\n', 0.1), ('1.5 1 2 3 0.1 0.1 -0.1\n', None),
                        ('1.5 1 nan 3 0.1 0.1 0.1\n', None), ('1.5 1 2 3 0.1 0.1 0.1\n2.5 1 2\n', None), ('1.5 one 2 3\n', 0.1),
                        ('1.5 1 2 3\n', [0.1, 0.2])]:
        with pytest.raises(ValueError, match='position'):
            common.create_scene(_write_config(tmp_path, text, lm, sigma=sigma))
    with pytest.raises(ValueError, match="'lm'"):
        common.create_scene(_write_config(tmp_path, '1.5 1 2 3 0.1 0.1 0.1\n', dict(ba_solver='trf', ba_position_priors=True)))
    common.create_scene(_write_config(tmp_path, '1.5 1 2 3 0.1 0.1 0.1\n', dict(ba_solver='trf')))      # the flag off: read, not used
