"""Surveyed landmarks, the parts that need no GPU: the row routine of ba_landmark_math.h (host build, against the 50-digit restatement of
tests/landmark_reference.py), the entry map of k_landmark_ne's second phase, sigma broadcasting, the two text files, the validation of the
settings before any GPU call and Scene.align_to_landmarks on noise-free marks."""
import mpmath
import numpy as np
import pytest

import landmark_hostcheck_util as lhc
import landmark_reference as lref
from frozen_util import build_scene, packed
from golden_util import load_case
from mvus_amd import ba as mba
from mvus_amd import problem as mp
from mvus_amd.reconstruction import common
from mvus_amd.synth import rodrigues

# What a plain-fp64 evaluation of the reference's own text (mpmath.workprec(53), as tests/golden/make_golden_mp_jacobian.py measures the
# floor of the detection rows) loses against its 50-digit values, relative to the largest entry of the slot group in the row, worst over
# the cases of landmark_reference.host_cases with an ordinary rotation angle (|rvec| >= 0.1) or none at all: measured 8.22e-16 on the CPU
# (P15_raw_c0_rbig_border).  The cases with 0 < |rvec| <= 1.01e-2 are left out of the MEASUREMENT, as that generator leaves them out: the
# dual-number text divides by theta and loses 1e-9 at |rvec| = 2e-9, which says nothing about a sound fp64 evaluation.  Every case is HELD
# to the bar.  test_floor_constant_is_the_measured_one measures it again.
FLOOR_53 = 8.3e-16
BAR = lref.TOL_FACTOR * FLOOR_53


@pytest.fixture(scope='module')
def cases():
    scene, _ = load_case('dist_fixed_2cam')
    prob, _ = mp.problem_from_scene(scene)
    fixed = [(np.asarray(prob.K[c], dtype=np.float64), np.asarray(prob.dist[c], dtype=np.float64)) for c in range(prob.C)]
    assert any(np.any(d != 0) for _, d in fixed)
    out = []
    for case in lref.host_cases(fixed):
        with mpmath.workdps(lref.DPS):
            r50, J50 = lref.row_mp(*case[1:])
        out.append((case, r50, J50))
    return out


def test_cases_cover_the_edges(cases):
    names = [c[0][0] for c in cases]
    for part in ('P6_raw', 'P6_ud_c1', 'P15_raw', 'P15_ud', '_r0_', '_rlo_', '_rhi_', '_rtiny_', '_border', '_centre', 'zero_u', 'w0_axis'):
        assert any(part in n for n in names), part
    for (name, calib, undist, K4, d5, params, X, uv, w), r50, J50 in cases:
        th = np.linalg.norm(params[4:7] if calib else params[0:3])
        if '_rlo_' in name:
            assert 0 < th < 1e-2
        if '_rhi_' in name:
            assert 1e-2 <= th < 1.1e-2
        if 'zero_u' in name:
            assert r50[0] == 0.0 and r50[1] != 0.0


def test_host_rows_against_50_digits(cases):
    """1. r within the project's residual bar (1e-9 px, times the weight) and every derivative within 8 x the fp64 floor of its slot group."""
    worst, worst_name, worst_r = 0.0, None, 0.0
    for (name, *args), r50, J50 in cases:
        r, J = lhc.row(*args)
        w = args[-1]
        assert np.all(np.abs(r - r50) <= lref.RESIDUAL_ATOL * np.maximum(w, 1.0)), (name, r, r50)
        ratio = lref.group_ratio(J, J50)
        if ratio > worst:
            worst, worst_name = ratio, name
        worst_r = max(worst_r, float(np.abs(r - r50).max()))
        assert ratio <= BAR, (name, ratio, BAR)
        if 'zero_u' in name:
            assert r[0] == 0.0
        if 'w0_axis' in name:
            assert r[0] == 0.0 and not J[0].any() and J[1].any()
    print('host landmark rows: worst derivative %.3g of its slot group (%s), bar %.3g; worst residual %.3g px' % (worst, worst_name, BAR, worst_r))


def test_floor_constant_is_the_measured_one(cases):
    floor = 0.0
    for (name, calib, undist, K4, d5, params, X, uv, w), r50, J50 in cases:
        th = np.linalg.norm(params[4:7] if calib else params[0:3])
        if 0 < th < 0.1:
            continue
        with mpmath.workprec(53):
            _, J53 = lref.row_mp(calib, undist, K4, d5, params, X, uv, w)
        floor = max(floor, lref.group_ratio(J53, J50))
    print('53-bit floor of the landmark rows: %.3g (constant %.3g)' % (floor, FLOOR_53))
    assert 0.5 * FLOOR_53 <= floor <= FLOOR_53


@pytest.mark.parametrize('P', [6, 15])
def test_entry_map_covers_the_augmented_triangle_once(P):
    ent = lhc.entries(P)
    assert len(ent) == P * (P + 3) // 2 <= 256
    want = {(a, b) for a in range(P) for b in range(a, P + 1)}
    assert set(ent) == want and len(set(ent)) == len(ent)


def test_sigma_broadcasting_and_inf():
    X = np.zeros((3, 4))
    cam, point = [0, 1, 1], [0, 3, 2]
    uv = np.arange(6.0).reshape(2, 3)
    for sigma, want in ((2.0, np.full((2, 3), 0.5)), ([2.0, 4.0], np.array([[0.5] * 3, [0.25] * 3])),
                        (np.array([[1.0, np.inf, 2.0], [np.inf, np.inf, 4.0]]), np.array([[1.0, 0.0, 0.5], [0.0, 0.0, 0.25]]))):
        Xo, c, p, u, w = mba.landmark_arrays(X, cam, point, uv, sigma)
        assert np.array_equal(w, want) and w.flags['C_CONTIGUOUS'] and c.dtype == np.int32 and p.dtype == np.int32
    for bad in (0.0, -1.0, np.nan, [1.0, 2.0, 3.0], np.ones((3, 3))):
        with pytest.raises(ValueError):
            mba.landmark_arrays(X, cam, point, uv, bad)
    with pytest.raises(ValueError):
        mba.landmark_arrays(np.zeros((4, 3)), cam, point, uv, 1.0)
    with pytest.raises(ValueError):
        mba.landmark_arrays(X, cam, point[:2], uv, 1.0)


def test_files_are_parsed_and_checked(tmp_path):
    pts, obs = tmp_path / 'marks.txt', tmp_path / 'clicks.txt'
    pts.write_text('# id x y z\n7 1.0 2.0 3.0\n3 -1.0 0.5 4.0\n11 0 0 1\n')
    obs.write_text('# camera id u v\n0 3 100.5 200.25\n1 7 300 400\n1 11 5 6\n')
    X, ob = common.load_landmarks(str(pts), str(obs), default_sigma=[0.5, 2.0])
    assert np.array_equal(X, np.array([[1.0, -1.0, 0.0], [2.0, 0.5, 0.0], [3.0, 4.0, 1.0]]))
    assert np.array_equal(ob, np.array([[0, 1, 1], [1, 0, 2], [100.5, 300, 5], [200.25, 400, 6], [0.5] * 3, [2.0] * 3]))
    with pytest.raises(ValueError, match='landmark_sigma'):
        common.load_landmarks(str(pts), str(obs))
    obs.write_text('0 3 100.5 200.25 1.0 inf\n1 8 300 400 1 1\n')
    with pytest.raises(ValueError, match=r'ids \[8\]'):
        common.load_landmarks(str(pts), str(obs))
    obs.write_text('0 3 100.5 200.25 1.0 inf\n')
    X, ob = common.load_landmarks(str(pts), str(obs))
    assert ob.shape == (6, 1) and np.isinf(ob[5, 0])
    obs.write_text('0 3 100.5 200.25 1.0\n')
    with pytest.raises(ValueError, match='columns'):
        common.load_landmarks(str(pts), str(obs))
    pts.write_text('7 1 2 3\n7 1 2 4\n')
    with pytest.raises(ValueError, match='each once'):
        common.load_landmarks(str(pts), str(obs))


def _scene_with_marks(name='c1_pinhole_2cam', L=6, **settings):
    scene, _ = load_case(name)
    s = build_scene(scene, motion_reg=False, **settings)
    cams = list(range(scene.num_cam))
    prob, x0 = packed(s, cams)
    X = lref.landmarks_in_front(prob, x0, L)
    cam = np.repeat(cams, L)
    point = np.tile(np.arange(L), len(cams))
    uv = np.array([lref.project_np(prob, x0, int(c), X[:, int(l)])[0] for c, l in zip(cam, point)]).T
    s.landmarks = X
    s.landmark_observations = np.vstack((cam, point, uv, np.ones((2, cam.size))))
    return s, prob, x0, cams


def test_align_to_landmarks_recovers_a_known_similarity():
    """Noise-free clicks of six marks through the scene's own cameras, the scene then moved away by the inverse of a known similarity:
    (s, R, T) comes back to 1e-10, the bar of align_to_position_priors, and the cameras are back where they were."""
    s, prob, x0, cams = _scene_with_marks()
    assert not s.settings['undist_points'] or not any(np.any(c.d) for c in s.cameras)
    rvec = np.array([0.3, -0.2, 0.17]) * 0.4 / np.linalg.norm([0.3, -0.2, 0.17])
    sc, R, T = 1.7, rodrigues(rvec), np.array([3.0, -4.0, 0.0])
    s.apply_similarity(1.0 / sc, R.T, -(R.T @ T) / sc)               # the inverse: X -> R^T (X - T) / sc
    s2, R2, T2, rms = s.align_to_landmarks()
    size = float(np.abs(s.landmarks).max())
    print('|s - s0| = %.3g, |R - R0| = %.3g, |T - T0| = %.3g, rms / size = %.3g' % (abs(s2 - sc), np.abs(R2 - R).max(), np.abs(T2 - T).max(), rms / size))
    assert abs(s2 - sc) <= 1e-10 and np.abs(R2 - R).max() <= 1e-10 and np.abs(T2 - T).max() <= 1e-10 * max(1.0, np.abs(T).max())
    assert rms <= 1e-9 * size
    np.testing.assert_allclose(s._pack(prob, cams), x0, rtol=0, atol=1e-9 * max(1.0, np.abs(x0[3 * prob.C:]).max()))


def test_align_needs_three_landmarks_that_are_not_collinear():
    s, prob, x0, cams = _scene_with_marks()
    X, ob = s.landmarks.copy(), s.landmark_observations.copy()
    s.landmarks = None
    with pytest.raises(ValueError, match='at least 3'):
        s.align_to_landmarks()
    s.landmarks, s.landmark_observations = X, ob[:, ob[1] < 2]                      # two marks
    with pytest.raises(ValueError, match='at least 3'):
        s.align_to_landmarks()
    s.landmark_observations = ob[:, (ob[1] < 2) | (ob[0] == 0)]                     # the others seen by one camera only
    with pytest.raises(ValueError, match='at least 3'):
        s.align_to_landmarks()
    line = X[:, [0]] + (X[:, [1]] - X[:, [0]]) * np.array([0.0, 1.0, 0.4, 0.7])[None, :]
    cam, point = np.repeat(cams, 4), np.tile(np.arange(4), len(cams))
    uv = np.array([lref.project_np(prob, x0, int(c), line[:, int(l)])[0] for c, l in zip(cam, point)]).T
    s.landmarks, s.landmark_observations = line, np.vstack((cam, point, uv, np.ones((2, cam.size))))
    before = s._pack(prob, cams)
    with pytest.raises(ValueError, match='collinear'):
        s.align_to_landmarks()
    assert np.array_equal(s._pack(prob, cams), before)                              # a refused alignment moves nothing


def test_settings_are_validated_before_any_gpu_call(monkeypatch):
    """ba_landmarks with a solver other than 'lm', a flag that is no bool and malformed arrays raise ValueError from ba_mode, which Scene.BA
    consults before it creates a handle; observations of cameras outside the BA's set are left out and the ids mapped."""
    s, prob, x0, cams = _scene_with_marks(ba_solver='lm', ba_landmarks=True)
    monkeypatch.setattr(common.Scene, '_resident_handle', lambda *a, **k: pytest.fail('a handle was created'))
    lm = s.ba_landmarks(cams)
    assert lm[1].size == 12 and lm[1].dtype == np.int32
    lm = s.ba_landmarks([1])
    assert lm[1].size == 6 and not lm[1].any()                                       # camera id 1 is index 0 of that BA
    assert s.ba_landmarks([5]) is None
    s.settings['ba_solver'] = 'trf'
    with pytest.raises(ValueError, match="'lm'"):
        s.ba_mode()
    with pytest.raises(ValueError, match="'lm'"):
        s.BA(2)
    s.settings['ba_solver'] = 'lm'
    s.settings['ba_landmarks'] = 'yes'
    with pytest.raises(ValueError, match='true or false'):
        s.ba_mode()
    s.settings['ba_landmarks'] = True
    good = s.landmark_observations.copy()
    for row, val in ((1, 6.0), (1, 0.5), (0, -1.0), (2, np.nan), (4, 0.0), (5, -2.0)):
        bad = good.copy()
        bad[row, 3] = val
        s.landmark_observations = bad
        with pytest.raises(ValueError):
            s.ba_mode()
    s.landmark_observations = good
    with pytest.raises(mba.UnsupportedBySolver, match='ba_landmarks'):
        s.register_camera(1)
    held, s.landmark_observations = s.landmark_observations, None        # the flag alone refuses nothing: the call goes on to its own checks
    with pytest.raises(ValueError, match='unknown name'):
        s.register_camera(1, hold=('nonsense',))
    s.landmark_observations = held
    s.settings['ba_landmarks'] = False
    assert s.ba_landmarks(cams) is None


def test_gpu_floor_constants_are_the_measured_ones():
    """The per-fixture and per-set fp64 floors written into tests/test_gpu_landmarks.py (FLOOR_53), measured again on the CPU on the very
    rows that test compares: each constant is at least the measured loss and at most 10 % above it, so a change of the sets or of a
    constant shows here."""
    import test_gpu_landmarks as tg
    measured = {}
    for name in tg.FIXTURES:
        _, _, prob, x, sets = tg._case(name)
        for sname, (X, cam, point, uv, w) in sets.items():
            pick, _, J50 = tg._reference_rows(name, sname)
            with mpmath.workprec(53):
                _, J53 = lref.rows_mp(prob, x, X, cam[pick], point[pick], uv[:, pick], w[:, pick], dps=None)
            key = sname if sname in tg.FLOOR_53 else name
            measured[key] = max(measured.get(key, 0.0), lref.group_ratio(J53, J50))
    print('53-bit floors of the GPU test\'s rows:', {k: '%.3g' % v for k, v in measured.items()})
    assert set(measured) == set(tg.FLOOR_53)
    for key, v in measured.items():
        assert v <= tg.FLOOR_53[key] <= 1.1 * v, (key, v, tg.FLOOR_53[key])
