"""Surveyed landmarks in the LM + Schur BA, on the GPU (mvus_ba_set_landmarks / mvus_ba_num_landmark_observations / mvus_ba_landmark_cost /
mvus_ba_landmark_rows; Scene settings ba_landmarks).

The reference of the rows is the 50-digit restatement of tests/landmark_reference.py; of the blocks, numpy sums of the device's own rows;
of the step, LAPACK on the exported blocks (tests/lm_reference.py); of the detection cost, the oracle."""
import functools

import numpy as np
import pytest

import landmark_reference as lref
from golden_util import load_case
from lm_reference import lapack_lm_step
from mvus_amd import _lib
from mvus_amd import problem as mp
from test_gpu_position_priors import _dense_system, _refined_solve, _route

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
FIXTURES = ['c1_pinhole_2cam', 'calib_KE_bounds_3cam', 'dist_fixed_2cam']
LM = dict(solver=_lib.SOLVER_LM_SCHUR, jac_mode=_lib.JAC_ANALYTIC)
# The bar of the rows is the rule of tests/test_landmarks_host.py on THIS file's rows: 8 x what a plain-fp64 evaluation of the reference's
# own text (mpmath.workprec(53)) loses against its 50-digit values on the compared rows, relative to the largest entry of the slot group
# in the row.  Measured on the CPU per fixture over its four small sets, and per large set of c1_pinhole_2cam (whose cameras sit at
# |rvec| = 2.07: the v row's rvec group has entries of 7.7 formed from products of 340, and the more landmarks, the worse the worst one):
# c1_pinhole_2cam 1.37e-15, e_256 3.28e-15, f_257 6.18e-15, g_1030 1.41e-14 (observation 777); calib_KE_bounds_3cam 7.30e-16;
# dist_fixed_2cam 1.16e-15.
FLOOR_53 = {'c1_pinhole_2cam': 1.4e-15, 'e_256': 3.3e-15, 'f_257': 6.2e-15, 'g_1030': 1.42e-14, 'calib_KE_bounds_3cam': 7.4e-16, 'dist_fixed_2cam': 1.2e-15}


def _obs(prob, x, X, cam, point, seed=9):
    cam, point = np.asarray(cam, dtype=np.int32), np.asarray(point, dtype=np.int32)
    uv, w = lref.observations(prob, x, X, cam, point, seed=seed)
    return X, cam, point, uv, w


def _sets(prob, x, big):
    """{name: (X, cam, point, uv, w)}: (a) K = 1; (b) a camera without rows; (c) one landmark seen by every camera; (d) a w = 0 axis, a
    w = 0 pair and a duplicated (camera, landmark); with ``big`` (the 2-camera fixture) (e) exactly 256 rows on one camera, (f) 257,
    (g) 1030 = four full rounds + 6, no multiple of 4."""
    C = prob.C
    X = lref.landmarks_in_front(prob, x, 5)
    sets = {'a_one': _obs(prob, x, X, [0], [0]),
            'b_idle_camera': _obs(prob, x, X, np.repeat(np.arange(1, C), 5), np.tile(np.arange(5), C - 1)),
            'c_one_mark': _obs(prob, x, X, np.arange(C), np.full(C, 2))}
    d = list(_obs(prob, x, X, [0, 0, C - 1, C - 1, C - 1], [0, 1, 1, 1, 3]))
    d[4][0, 0] = 0.0
    d[4][:, 1] = 0.0
    sets['d_weights_dup'] = tuple(d)
    if big:
        for name, n in (('e_256', 256), ('f_257', 257), ('g_1030', 1030)):
            Xn = lref.landmarks_in_front(prob, x, n, seed=n)
            rng = np.random.default_rng(n)
            order = rng.permutation(n + 3)
            cam = np.concatenate((np.zeros(n, dtype=np.int32), np.ones(3, dtype=np.int32)))[order]
            point = np.concatenate((np.arange(n), [0, 1, 2]))[order]
            sets[name] = _obs(prob, x, Xn, cam, point, seed=n)
    return sets


@functools.lru_cache(maxsize=None)
def _case(name, motion_reg=None):
    scene, g = load_case(name)
    over = {} if motion_reg is None else dict(motion_reg=motion_reg)
    prob, _ = mp.problem_from_scene(scene, **over)
    x = np.array(g['x0'] + g['delta'])
    return scene, g, prob, x, _sets(prob, x, name == 'c1_pinhole_2cam')


@functools.lru_cache(maxsize=None)
def _reference_rows(name, sname):
    """the 50-digit rows of one set, computed once and shared"""
    _, _, prob, x, sets = _case(name)
    X, cam, point, uv, w = sets[sname]
    if cam.size > 40:                        # the large sets: every 7th observation (the row routine is the same for all of them)
        pick = np.arange(0, cam.size, 7)
    else:
        pick = np.arange(cam.size)
    r, J = lref.rows_mp(prob, x, X, cam[pick], point[pick], uv[:, pick], w[:, pick])
    return pick, r, J


def _set(h, X, cam, point, uv, w):
    """The observations with their weights as given (the binding's sigma form would round 1 / (1 / w))."""
    X, uv, w = (np.ascontiguousarray(a, dtype=np.float64) for a in (X, uv, w))
    cam, point = (np.ascontiguousarray(a, dtype=np.int32) for a in (cam, point))
    i32 = lambda a: a.ctypes.data_as(_lib.c_int32_p)
    h._check(h.lib.mvus_ba_set_landmarks(h.h, X.shape[1], _lib.dptr(X), cam.size, i32(cam), i32(point), _lib.dptr(uv), _lib.dptr(w)), 'mvus_ba_set_landmarks')


def _clear(h):
    h.set_landmarks(None, None, None, None, None)


@pytest.mark.parametrize('name', FIXTURES)
def test_rows_against_50_digits(name):
    """1. landmark_rows against the 50-digit reference: r to the residual bar, every derivative to 8 x the fp64 floor of its slot group
    (FLOOR_53 above); landmark_cost's r = landmark_rows' r bit for bit; rows of a weightless axis are exactly 0."""
    from mvus_amd.ba import BAHandle
    _, _, prob, x, sets = _case(name)
    with BAHandle(prob) as h:
        for sname, lset in sets.items():
            _set(h, *lset)
            w = lset[4]
            assert h.num_landmark_observations == lset[1].size and h.num_landmark_rows == int((w > 0).sum())
            r, J = h.landmark_rows(x)
            cost, rc = h.landmark_cost(x, rows=True)
            assert np.array_equal(r, rc)
            assert J.shape == (lset[1].size, 2, prob.P)
            pick, r50, J50 = _reference_rows(name, sname)
            err = np.abs(r[:, pick] - r50)
            ratio = lref.group_ratio(J[pick], J50)
            bar = lref.TOL_FACTOR * FLOOR_53.get(sname, FLOOR_53[name])
            print('%s %s: K = %d, rows max |r - r50| = %.3g px, derivatives %.3g of the slot group (bar %.3g)' % (name, sname, lset[1].size, err.max(), ratio, bar))
            assert np.all(err <= lref.RESIDUAL_ATOL * np.maximum(w[:, pick], 1.0))
            assert ratio <= bar
            assert not r[w == 0].any() and not J[(w == 0).T].any()
            assert np.abs(r[w > 0]).min() > 0


def _check_contribution(prob, lset, ne0, ne1, r, J, what):
    """ne1 - ne0 against the sums of the device's own rows: everything the landmarks do not touch bit for bit, touched entries to
    (n_rows + 8) eps sum |terms| + eps |entry without landmarks|, n_rows the scalar rows of the camera."""
    X, cam, point, uv, w = lset
    g0, A0, band0, cross0 = ne0
    g1, A1, band1, cross1 = ne1
    C, P = prob.C, prob.P
    head = C * (3 + P)
    assert np.array_equal(band1, band0) and np.array_equal(cross1, cross0) and np.array_equal(g1[head:], g0[head:]), what
    assert np.array_equal(g1[:3 * C], g0[:3 * C]), what
    assert np.array_equal(A1[:, :3, :], A0[:, :3, :]) and np.array_equal(A1[:, :, :3], A0[:, :, :3]), what
    dA, dg, aA, ag, n = lref.contribution(prob, cam, r, J)
    worst = 0.0
    for c in range(C):
        gc0, gc1 = g0[3 * C + c * P:3 * C + (c + 1) * P], g1[3 * C + c * P:3 * C + (c + 1) * P]
        if n[c] == 0:
            assert np.array_equal(A1[c], A0[c]) and np.array_equal(gc1, gc0), what
            continue
        eA = np.abs((A1[c, 3:, 3:] - A0[c, 3:, 3:]) - dA[c])
        bA = (2 * n[c] + 8) * EPS * aA[c] + EPS * np.abs(A0[c, 3:, 3:])
        eg = np.abs((gc1 - gc0) - dg[c])
        bg = (2 * n[c] + 8) * EPS * ag[c] + EPS * np.abs(gc0)
        assert np.array_equal(A1[c], A1[c].T) or not np.array_equal(A0[c], A0[c].T), what
        worst = max(worst, float((eA[bA > 0] / bA[bA > 0]).max()), float((eg[bg > 0] / bg[bg > 0]).max()))
        assert np.all(eA <= bA) and np.all(eg <= bg), (what, c)
        assert np.abs(dA[c]).max() > 0
    print('%s: max err / bar = %.3g (up to %d observations on one camera)' % (what, worst, n.max()))


@pytest.mark.parametrize('loss', ['linear', 'huber'])
@pytest.mark.parametrize('route', ['window-major', 'detection-major'])
@pytest.mark.parametrize('name', FIXTURES)
def test_normal_equations_gain_the_landmarks_contribution(name, route, loss, monkeypatch):
    """2. (blocks with landmarks) - (blocks without) = sum J^T J / sum J^T r of the device's own rows; the band, the spline gradient, the
    cross block, the sync slots of every camera block and the blocks of cameras without rows keep their bits; a repeat, and set (c)
    passed in another order, give identical bits window-major (to 1e-12 of the largest entry behind the detection-major kernel when its
    atomics moved the blocks without landmarks); a loss in force does not reach the landmark rows."""
    from mvus_amd.ba import BAHandle
    _, _, prob, x, sets = _case(name)
    _route(monkeypatch, route)
    with BAHandle(prob) as h:
        if loss != 'linear':
            h.set_loss(loss, 1.5)
        h.residual_jacobian(x, _lib.JAC_ANALYTIC)
        for sname, lset in sets.items():
            _clear(h)
            ne0 = h.normal_equations()
            assert h.deterministic_fallback() == (route == 'detection-major')
            _set(h, *lset)
            ne1 = h.normal_equations()
            r, J = h.landmark_rows(x)                    # (an inspection hook: the held blocks stay)
            what = '%s %s %s %s' % (name, route, loss, sname)
            _check_contribution(prob, lset, ne0, ne1, r, J, what)
            for a, b in zip(ne1, h.normal_equations()):
                assert np.array_equal(a, b)
            again = [lset]
            if sname == 'c_one_mark':
                o = np.arange(lset[1].size)[::-1]
                again.append((lset[0], lset[1][o], lset[2][o], lset[3][:, o], lset[4][:, o]))
            if sname == 'g_1030':
                o = np.random.default_rng(1).permutation(lset[1].size)
                again.append((lset[0], lset[1][o], lset[2][o], lset[3][:, o], lset[4][:, o]))
            for ls2 in again:
                _clear(h)
                ne0b = h.normal_equations()                              # a new assembly
                _set(h, *ls2)
                ne1b = h.normal_equations()                              # ... and a new launch of k_landmark_ne on it
                same_raw = all(np.array_equal(a, b) for a, b in zip(ne0, ne0b))
                assert same_raw or route == 'detection-major'
                for a, b in zip(ne1, ne1b):
                    if same_raw:
                        assert np.array_equal(a, b), what
                    else:
                        np.testing.assert_allclose(b, a, rtol=0, atol=1e-12 * np.abs(a).max())
        f, _, _ = h.residual_jacobian(x, _lib.JAC_ANALYTIC)      # error_BA itself stays raw
        assert f.size == prob.n_residuals


@pytest.mark.parametrize('name', FIXTURES)
def test_costs(name):
    """3. landmark_cost = 0.5 sum r^2 of its own rows to (2K + 8) eps relative; initial_cost of a solve with landmarks - without = the
    landmark cost within 1e-12 of the total; numpy's rows agree to the residual bar; the raw cost does not see the landmarks."""
    from mvus_amd.ba import BAHandle
    _, _, prob, x, sets = _case(name)
    with BAHandle(prob) as h:
        assert h.landmark_cost(x) == 0.0 and h.num_landmark_observations == 0
        base = h.solve(x, max_nfev=1, **LM).initial_cost
        for sname, lset in sets.items():
            _set(h, *lset)
            K = lset[1].size
            cost, r = h.landmark_cost(x, rows=True)
            own = 0.5 * float(np.sum(r ** 2))
            print('%s %s: cost %.17g, |cost - 0.5 sum r^2| / cost = %.3g (bar %.3g)' % (name, sname, cost, abs(cost - own) / own, (2 * K + 8) * EPS))
            assert cost > 0 and abs(cost - own) <= (2 * K + 8) * EPS * own
            assert np.abs(r - lref.rows_np(prob, x, *lset)).max() <= lref.RESIDUAL_ATOL * max(1.0, lset[4].max())
            with_l = h.solve(x, max_nfev=1, **LM)
            assert with_l.fun.size == prob.n_residuals                   # f stays error_BA's: 2M + T rows
            assert abs((with_l.initial_cost - base) - cost) <= 1e-12 * with_l.initial_cost, (with_l.initial_cost, base, cost)
            assert h.robust_cost(x) == base
        _clear(h)
        assert h.solve(x, max_nfev=1, **LM).initial_cost == base


@pytest.mark.parametrize('route', ['window-major', 'detection-major'])
@pytest.mark.parametrize('name', FIXTURES)
def test_frozen_parameters_stay_held(name, route, monkeypatch):
    """4. A mask that holds the pose of camera 0, which has landmark rows: rows and columns of the held unknowns are the freeze pass's
    (zero, H_kk = 1, g_k = 0); after a solve the held entries of x have the bits they went in with."""
    from mvus_amd.ba import BAHandle
    _, g, prob, x, sets = _case(name)
    _route(monkeypatch, route)
    C, P = prob.C, prob.P
    o = 4 if prob.opt_calib else 0
    mask = np.zeros(C * (3 + P), dtype=bool)
    held = 3 * C + np.arange(o, o + 6)                         # rvec, t of camera 0 in x
    mask[held] = True
    lset = sets['c_one_mark']
    with BAHandle(prob) as h:
        h.set_frozen(mask)
        _set(h, *lset)
        h.residual_jacobian(x, _lib.JAC_ANALYTIC)
        gg, A, band, cross = h.normal_equations()
        for k in range(o, o + 6):
            e = np.zeros(3 + P)
            e[3 + k] = 1.0
            assert np.array_equal(A[0, 3 + k], e) and np.array_equal(A[0, :, 3 + k], e) and gg[3 * C + k] == 0.0
        assert not cross.reshape(C, 3 + P, -1)[0, 3 + o:3 + o + 6].any()
        free = [k for k in range(P) if not o <= k < o + 6]
        if free:
            assert np.abs(A[0][np.ix_([3 + k for k in free], [3 + k for k in free])]).max() > 0
        assert np.abs(A[1, 3:, 3:]).max() > 0
        x0 = np.array(g['x0'])
        res = h.solve(x0, max_nfev=8, **LM)
        assert np.array_equal(res.x[held], x0[held]) and not np.array_equal(res.x, x0)


@pytest.mark.parametrize('route', ['window-major', 'detection-major'])
@pytest.mark.parametrize('name', FIXTURES)
def test_landmarks_on_top_of_frozen_blocks(name, route, monkeypatch):
    """4. mask -> normal_equations -> set_landmarks -> normal_equations / lm_step: the landmarks' pass goes on top of blocks that carry the
    freeze pass already (no new assembly), and the freeze pass runs again behind it -- rows and columns of the held unknowns are the
    freeze pass's, the step of every held unknown is exactly 0, the free part of the block has gained the landmarks' contribution, and the
    blocks equal those of a fresh assembly with both in force (bit for bit window-major)."""
    from mvus_amd.ba import BAHandle
    _, g, prob, x, sets = _case(name)
    _route(monkeypatch, route)
    C, P = prob.C, prob.P
    o = 4 if prob.opt_calib else 0
    mask = np.zeros(C * (3 + P), dtype=bool)
    held = 3 * C + np.arange(o, o + 3)                          # rvec of camera 0: its translation (and K, d) stay free
    mask[held] = True
    if not prob.rs_free:
        mask[2 * C:3 * C] = True                                # (rs is no unknown there: zero columns)
    lset = sets['c_one_mark']
    with BAHandle(prob) as h:
        h.set_frozen(mask)
        h.residual_jacobian(x, _lib.JAC_ANALYTIC)
        ne0 = h.normal_equations()
        _set(h, *lset)                                          # keeps the blocks: the pass goes on top
        gg, A, band, cross = h.normal_equations()
        for k in range(o, o + 3):
            e = np.zeros(3 + P)
            e[3 + k] = 1.0
            assert np.array_equal(A[0, 3 + k], e) and np.array_equal(A[0, :, 3 + k], e) and gg[3 * C + k] == 0.0
        assert not cross.reshape(C, 3 + P, -1)[0, 3 + o:3 + o + 3].any()
        free = [3 + k for k in range(P) if not o <= k < o + 3]
        assert np.abs(A[0][np.ix_(free, free)] - ne0[1][0][np.ix_(free, free)]).max() > 0      # the landmarks are in
        assert np.array_equal(band, ne0[2]) and np.array_equal(cross, ne0[3])
        p = h.lm_step(0.5)
        assert not p[np.nonzero(mask)[0]].any() and np.abs(p).max() > 0      # (the mask is over the head of x, in x's order)
        p_ref = lapack_lm_step(prob, gg, A, band, cross, 0.5)
        assert np.abs(p - p_ref).max() <= 1e-6 * np.abs(p_ref).max()
        h.residual_jacobian(x, _lib.JAC_ANALYTIC)               # a fresh assembly with mask and landmarks in force
        fresh = h.normal_equations()
        for a, b in zip((gg, A, band, cross), fresh):
            if route == 'window-major':
                assert np.array_equal(a, b)
            else:
                np.testing.assert_allclose(b, a, rtol=0, atol=1e-12 * np.abs(a).max())


@pytest.mark.parametrize('route', ['window-major', 'detection-major'])
@pytest.mark.parametrize('name', FIXTURES)
def test_lm_step_against_lapack(name, route, monkeypatch):
    """5. mvus_ba_lm_step with landmarks against LAPACK on the exported blocks at lambda = 0.5 and 1e-3: 1e-6 of the largest entry."""
    from mvus_amd.ba import BAHandle
    _, _, prob, x, sets = _case(name)
    _route(monkeypatch, route)
    with BAHandle(prob) as h:
        for sname in ('c_one_mark', 'd_weights_dup') + (('g_1030',) if 'g_1030' in sets else ()):
            _set(h, *sets[sname])
            h.residual_jacobian(x, _lib.JAC_ANALYTIC)
            g, A, band, cross = h.normal_equations()
            for lam in (0.5, 1e-3):
                p = h.lm_step(lam)
                p_ref = lapack_lm_step(prob, g, A, band, cross, lam)
                err = np.abs(p - p_ref).max() / np.abs(p_ref).max()
                print('%s %s %s lambda %g: |p - p_lapack|_max / |p_lapack|_max = %.3g' % (name, route, sname, lam, err))
                assert err <= 1e-6


def _gauge_set(prob, x):
    X = lref.landmarks_in_front(prob, x, 3, seed=17)
    sv = np.linalg.svd(X - X.mean(axis=1, keepdims=True), compute_uv=False)
    assert sv[1] > 0.1 * sv[0]                                # not collinear
    return _obs(prob, x, X, np.repeat(np.arange(prob.C), 3), np.tile(np.arange(3), prob.C), seed=17)


def test_landmarks_fix_the_gauge():
    """6. c1_pinhole_2cam, free gauge, no motion regulariser, three non-collinear landmarks seen by both cameras: the undamped step is
    solvable (without landmarks the system is singular) and agrees with LAPACK to 8 x LAPACK's own distance from a long-double-refined
    solve; the covariance is accepted with the gauge free, and refused again after clearing; dof is up by the rows with w > 0 and
    sigma^2 = 2 cost / dof with the landmark term in the cost.  As in the priors' test, the two rs entries -- no unknowns of this fixture,
    their columns are zero -- are held by a mask: that is no gauge freedom."""
    from mvus_amd.ba import BAHandle
    _, g, prob, x, _ = _case('c1_pinhole_2cam', False)
    assert prob.num_motion_rows == 0 and not prob.rs_free
    mask = np.zeros(prob.C * (3 + prob.P), dtype=bool)
    mask[2 * prob.C:3 * prob.C] = True
    lset = list(_gauge_set(prob, x))
    lset[4] = lset[4].copy()
    lset[4][1, 4] = 0.0                                           # one axis unknown: 11 rows
    with BAHandle(prob) as h:
        h.set_frozen(mask)
        h.residual_jacobian(x, _lib.JAC_ANALYTIC)
        H0, _ = _dense_system(prob, h.normal_equations())
        ev0 = np.linalg.eigvalsh(H0 / np.sqrt(np.outer(np.diag(H0), np.diag(H0))))
        assert abs(ev0[0]) < 1e-12                                     # the free gauge: numerically singular without landmarks
        _set(h, *lset)
        assert h.num_landmark_rows == 11
        h.residual_jacobian(x, _lib.JAC_ANALYTIC)
        ne = h.normal_equations()
        p = h.lm_step(0.0)                                             # raises MVUS_E_NUMERIC when the solve is not ok
        assert np.all(np.isfinite(p))
        H, gg = _dense_system(prob, ne)
        d = np.diag(H)
        assert np.all(d > 0)
        p_lapack = -np.linalg.solve(H, gg)
        p_exact = -_refined_solve(H, gg)
        scale = np.abs(p_exact).max()
        e_lapack = np.abs(p_lapack - p_exact).max() / scale
        e_pair = np.abs(p - p_lapack).max() / scale
        ev = np.linalg.eigvalsh(H / np.sqrt(np.outer(d, d)))
        print('lambda 0, three landmarks: GPU vs refined %.3g, LAPACK vs refined %.3g, GPU vs LAPACK %.3g; smallest scaled eigenvalue %.3g'
              % (np.abs(p - p_exact).max() / scale, e_lapack, e_pair, ev[0]))
        assert ev[0] > 1e-10
        assert e_pair <= 8 * max(e_lapack, 1e-12)
    xs = np.array(g['ba10_x'])
    lset = list(_gauge_set(prob, xs))
    lset[4] = lset[4].copy()
    lset[4][1, 4] = 0.0
    with BAHandle(prob) as h:
        _set(h, *lset)
        cv = h.covariance(xs)
        total = h.robust_cost(xs) + h.landmark_cost(xs)
        assert h.landmark_cost(xs) > 0 and abs(cv.sigma2 - 2.0 * total / cv.dof) <= 1e-12 * cv.sigma2
        m_act = 2 * int((h.residual_jacobian(xs, _lib.JAC_ANALYTIC)[2] >= 0).sum())
        assert cv.dof == m_act + 11 - int(cv.estimated.sum())
        _clear(h)
        with pytest.raises(ValueError, match='gauge'):
            h.covariance(xs)


def test_solve_with_landmarks():
    """7. LM, 50 evaluations, from the fixture's start with twelve clicks of six marks placed at its BA result: the total cost falls;
    res.cost = oracle detection cost + numpy landmark cost at the returned x (1e-9 relative); solve -> set -> clear -> solve = solve ->
    solve bit for bit; the landmarks survive remove_outliers."""
    from mvus_amd.ba import BAHandle
    from oracle import ba_oracle as orc
    scene, g, prob, _, _ = _case('c1_pinhole_2cam')
    oprob, _ = orc.problem_from_scene(scene)
    x0, xs = np.array(g['x0']), np.array(g['ba10_x'])
    X = lref.landmarks_in_front(prob, xs, 6, seed=5)
    lset = _obs(prob, xs, X, np.repeat([0, 1], 6), np.tile(np.arange(6), 2), seed=5)
    with BAHandle(prob) as h:
        _set(h, *lset)
        res = h.solve(x0, max_nfev=50, **LM)
        fo = orc.residual(oprob, res.x)
        lc = lref.cost_np(prob, res.x, *lset)
        ref = 0.5 * float(fo @ fo) + lc
        print('solve with 12 clicks: cost %.10g -> %.10g in %d evaluations; oracle + numpy %.10g (rel %.3g); landmark part %.6g'
              % (res.initial_cost, res.cost, res.nfev, ref, abs(res.cost - ref) / ref, lc))
        assert res.cost < res.initial_cost
        assert abs(res.cost - ref) <= 1e-9 * ref
        assert res.fun.size == prob.n_residuals and np.abs(res.fun - fo).max() <= 1e-9
        keep = h.remove_outliers(res.x, float(scene.settings['thres_outlier']))
        assert h.num_landmark_observations == 12 and h.num_landmark_rows == 24
        h.residual_jacobian(res.x, _lib.JAC_ANALYTIC)
        ne1 = h.normal_equations()
        r, J = h.landmark_rows(res.x)
        _clear(h)
        h.residual_jacobian(res.x, _lib.JAC_ANALYTIC)
        ne0 = h.normal_equations()
        _check_contribution(h.prob, lset, ne0, ne1, r, J, 'after remove_outliers (%d of %d kept)' % (keep.sum(), keep.size))
    with BAHandle(prob) as h:
        a1 = h.solve(x0, max_nfev=6, return_fun=False, **LM)
        a2 = h.solve(a1.x, max_nfev=6, **LM)
    with BAHandle(prob) as h:
        b1 = h.solve(x0, max_nfev=6, return_fun=False, **LM)
        _set(h, *lset)
        _clear(h)
        b2 = h.solve(b1.x, max_nfev=6, **LM)
    assert np.array_equal(a1.x, b1.x)
    assert np.array_equal(a2.x, b2.x) and a2.cost == b2.cost and a2.nfev == b2.nfev and np.array_equal(a2.fun, b2.fun)


def test_refusals(monkeypatch):
    """8. Every MVUS_E_INVALID before the device is touched; TRF ('TRF_LSMR'); sharded handles in both orders ('sharded');
    register_cameras / register_linearize ('landmark'); LM in the other Jacobian modes takes them."""
    from mvus_amd.ba import BAHandle, UnsupportedBySolver
    _, g, prob, x, sets = _case('rs_F_2int_3cam')
    lset = sets['c_one_mark']
    X, cam, point, uv, w = lset
    x0 = np.array(g['x0'])
    noop = lambda buf, count, stream: None
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32).ctypes.data_as(_lib.c_int32_p)
    with BAHandle(prob) as h:
        _set(h, *lset)

        def call(L, XX, K, cc, pp, uu, ww):
            return h.lib.mvus_ba_set_landmarks(h.h, L, _lib.dptr(np.ascontiguousarray(XX, dtype=np.float64)), K, i32(cc), i32(pp),
                                               _lib.dptr(np.ascontiguousarray(uu, dtype=np.float64)), _lib.dptr(np.ascontiguousarray(ww, dtype=np.float64)))
        L, K = X.shape[1], cam.size
        bad_cam, bad_pt, neg_pt = cam.copy(), point.copy(), point.copy()
        bad_cam[1], bad_pt[0], neg_pt[2] = prob.C, L, -1
        nanX, infuv, nanw, negw = X.copy(), uv.copy(), w.copy(), w.copy()
        nanX[1, 2], infuv[0, 1], nanw[1, 0], negw[0, 2] = np.nan, np.inf, np.nan, -1.0
        for args in [(-1, X, K, cam, point, uv, w), (L, X, -1, cam, point, uv, w), (L, X, (1 << 24) + 1, cam, point, uv, w),
                     (L, X, K, bad_cam, point, uv, w), (L, X, K, -1 - cam, point, uv, w), (L, X, K, cam, bad_pt, uv, w), (L, X, K, cam, neg_pt, uv, w),
                     (L, nanX, K, cam, point, uv, w), (L, X, K, cam, point, infuv, w), (L, X, K, cam, point, uv, nanw), (L, X, K, cam, point, uv, negw),
                     (L, X, K, cam, point, uv, np.full_like(w, np.inf))]:
            assert call(*args) == _lib.MVUS_E_INVALID
            assert b'set_landmarks' in h.lib.mvus_last_error(h.h)
        assert h.num_landmark_observations == K and h.num_landmark_rows == 2 * K      # a refused set leaves the handle as it was
        for jac in (_lib.JAC_ANALYTIC, _lib.JAC_PATTERN):
            with pytest.raises(UnsupportedBySolver, match='TRF_LSMR'):
                h.solve(x0, solver=_lib.SOLVER_TRF_LSMR, jac_mode=jac, max_nfev=3, ties='canonical')
        with pytest.raises(UnsupportedBySolver, match='landmark'):
            h.register_cameras(x, [0])
        with pytest.raises(UnsupportedBySolver, match='landmark'):
            h.register_linearize(x, [1])
        for jac in (_lib.JAC_PATTERN, _lib.JAC_FD):               # LM takes the landmarks in every Jacobian mode: the pass is behind the assembly
            r = h.solve(x0, solver=_lib.SOLVER_LM_SCHUR, jac_mode=jac, max_nfev=10)
            assert abs(r.initial_cost - (0.5 * float(np.sum(h.residual(x0) ** 2)) + h.landmark_cost(x0))) <= 1e-12 * r.initial_cost
        _clear(h)
        assert h.register_linearize(x, [1])[0].shape == (1, 3 + prob.P, 3 + prob.P)     # cleared: served again
    with BAHandle(prob) as h:                                           # the route first
        h.set_allreduce(noop)
        with pytest.raises(UnsupportedBySolver, match='sharded'):
            _set(h, *lset)
        assert h.num_landmark_observations == 0
        _clear(h)                                                       # nothing to refuse
    with BAHandle(prob) as h:                                           # the landmarks first: never solved without them
        _set(h, *lset)
        h.set_allreduce(noop)
        with pytest.raises(UnsupportedBySolver, match='sharded'):
            h.solve(x0, max_nfev=3, **LM)
        h.residual_jacobian(x0, _lib.JAC_ANALYTIC)
        with pytest.raises(UnsupportedBySolver, match='sharded'):
            h.normal_equations()
        with pytest.raises(UnsupportedBySolver, match='sharded'):
            h.lm_step(0.1)
        with pytest.raises(UnsupportedBySolver, match='sharded'):
            h.landmark_cost(x0)
    N = int(prob.n_coef.sum())
    with BAHandle(prob) as h:                                           # a time shard, both orders
        h.set_time_shard(0, 2, [0, N // 2, N])
        with pytest.raises(UnsupportedBySolver, match='sharded'):
            _set(h, *lset)
    with BAHandle(prob) as h:
        _set(h, *lset)
        h.set_time_shard(0, 2, [0, N // 2, N])
        with pytest.raises(UnsupportedBySolver, match='sharded'):
            h.solve(x0, max_nfev=3, **LM)


def test_scene_ba_refuses_the_trf_hand_over_with_landmarks(monkeypatch):
    """8. Where the wide-band policy of Scene.BA would hand the problem to TRF + LSMR, landmarks raise UnsupportedBySolver instead of being
    dropped; with ba_lm_wide_band = 'lm' the same BA runs and carries them."""
    from frozen_util import ba_kwargs, build_scene
    from mvus_amd.ba import UnsupportedBySolver
    from mvus_amd.reconstruction import common
    scene, _, prob, x, sets = _case('c1_pinhole_2cam')
    X, cam, point, uv, w = sets['c_one_mark']
    monkeypatch.setattr(common.Scene, '_motion_band_width', staticmethod(lambda prob: 8))      # what knots less than a frame apart give
    s = build_scene(scene, ba_solver='lm', ba_landmarks=True)
    s.landmarks = X
    s.landmark_observations = np.vstack((cam, point, uv, 1.0 / w))
    with pytest.raises(UnsupportedBySolver, match='ba_landmarks'):
        s.BA(2, max_iter=3, **ba_kwargs(s.settings))
    s.settings['ba_lm_wide_band'] = 'lm'
    res = s.BA(2, max_iter=3, **ba_kwargs(s.settings))
    assert res.solver_used == 'lm' and res.num_landmark_observations == 2


def _synthetic():
    from mvus_amd import bspline, synth
    sc = synth.make_scene(3, 9000, seed=31)
    tr = sc.truth

    def true_curve(tau):
        Xc = np.full((3, tau.size), np.nan)
        for tck in tr['tck']:
            m = (tau >= tck[0][0]) & (tau <= tck[0][-1])
            if m.any():
                Xc[:, m] = bspline.evaluate(tck[0], np.array(tck[1]), tau[m])
        return Xc
    # six marks at known world positions around the flight, clicked in every camera: projections through the TRUE cameras + N(0, 0.5 px)
    rng = np.random.default_rng(31)
    lo, hi = sc.interval[0, 0], sc.interval[1, -1]
    tau = np.linspace(lo + 5, hi - 5, 400)
    Xc = true_curve(tau)
    Xc = Xc[:, np.all(np.isfinite(Xc), axis=0)]
    span = Xc.max(axis=1) - Xc.min(axis=1)
    X = Xc[:, np.linspace(0, Xc.shape[1] - 1, 6).astype(int)] + 0.15 * span.max() * rng.uniform(-1, 1, (3, 6))
    ob = []
    for c, cam in enumerate(tr['cameras']):
        assert not np.any(cam['d'])
        Xcam = cam['R'] @ X + np.ravel(cam['t'])[:, None]
        assert np.all(Xcam[2] > 0)
        u = cam['K'][0, 0] * Xcam[0] / Xcam[2] + cam['K'][0, 2] + 0.5 * rng.standard_normal(6)
        v = cam['K'][1, 1] * Xcam[1] / Xcam[2] + cam['K'][1, 2] + 0.5 * rng.standard_normal(6)
        ob.append(np.vstack((np.full(6, c), np.arange(6), u, v, np.full((2, 6), 0.5))))
    return sc, true_curve, X, np.hstack(ob)


def test_scene_ba_end_to_end_in_the_surveyed_frame():
    """9. Synthetic scene (3 cameras, 9000 detections), the truth moved by a known similarity; six landmarks clicked in every camera with
    N(0, 0.5 px).  align_to_landmarks, then Scene.BA (lm, ba_landmarks): the trajectory rms against the truth with NO alignment afterwards
    is at most 2 x the same BA without landmarks followed by the best similarity onto the truth, and the scale is within 1 % of 1."""
    from mvus_amd.analysis.compare_gt import similarity_from_points
    from mvus_amd.reconstruction import common
    from mvus_amd.synth import rodrigues
    sc, true_curve, X, ob = _synthetic()
    tr = sc.truth

    def scene(**settings):
        s = common.Scene()
        s.numCam = 3
        s.settings = dict(sc.settings)
        s.settings.update(ba_solver='lm', **settings)
        for c in tr['cameras']:
            cam = common.Camera(K=c['K'].copy(), d=c['d'].copy(), R=c['R'].copy(), t=c['t'].copy(), fps=c['fps'], resolution=list(c['resolution']))
            cam.compose()
            s.addCamera(cam)
        for det in sc.detections:
            s.addDetection(det.copy())
        s.alpha, s.beta, s.rs = np.array(tr['alpha'], float), np.array(tr['beta'], float), np.array(tr['rs'], float)
        s.sequence = [0, 1, 2]
        s.spline = {'tck': [[np.array(t[0]), [np.array(c) for c in t[1]], 3] for t in tr['tck']], 'int': sc.interval.copy()}
        s.apply_similarity(1.3, rodrigues(np.array([0.2, -0.3, 0.1])), np.array([4.0, -2.0, 1.0]))     # the reconstruction's own arbitrary frame
        s.detection_to_global()
        return s
    st = sc.settings
    kw = dict(rs=st['rolling_shutter'], motion_reg=st['motion_reg'], motion_weights=st['motion_weights'], rs_bounds=st['rs_bounds'])
    ts = np.arange(np.ceil(sc.interval[0, 0]), np.floor(sc.interval[1, -1]), 1.0)
    Xt = true_curve(ts)
    ok = np.all(np.isfinite(Xt), axis=0)
    s0 = scene()
    s0.BA(3, max_iter=30, **kw)
    traj0 = s0.spline_to_traj(t=ts[ok])
    M = similarity_from_points(traj0[1:], Xt[:, ok])
    rms0 = float(np.sqrt(np.mean(np.sum((M[:3, :3] @ traj0[1:] + M[:3, 3:] - Xt[:, ok]) ** 2, axis=0))))
    s1 = scene(ba_landmarks=True)
    s1.landmarks, s1.landmark_observations = X, ob
    scale, R, T, rms_fit = s1.align_to_landmarks()
    res = s1.BA(3, max_iter=30, **kw)
    assert res.num_landmark_observations == 18 and res.solver_used == 'lm'
    traj1 = s1.spline_to_traj(t=ts[ok])
    rms1 = float(np.sqrt(np.mean(np.sum((traj1[1:] - Xt[:, ok]) ** 2, axis=0))))
    M1 = similarity_from_points(traj1[1:], Xt[:, ok])
    scale1 = float(np.cbrt(np.linalg.det(M1[:3, :3])))
    print('end to end: rms against the truth with landmarks, NO alignment: %.4g m; without landmarks after the best similarity: %.4g m; bar %.4g m; '
          'scale to the truth %.6f (alignment scale %.5f = 1 / 1.3 expected, fit rms %.3g m)' % (rms1, rms0, 2 * rms0, scale1, scale, rms_fit))
    assert rms1 <= 2 * rms0
    assert abs(scale1 - 1.0) <= 0.01


def test_reconstruct_from_config_with_landmark_files(tmp_path):
    """9. The pipeline from files (tests/test_gpu_init_pipeline.py's inputs plus the two landmark files): the output is in the surveyed
    frame -- scale within 1 % of the truth with no alignment -- and ba_covariance accepts the free gauge."""
    import json
    from mvus_amd import pipeline
    from mvus_amd.analysis.compare_gt import similarity_from_points
    from test_gpu_init_pipeline import _write_inputs
    sc, true_curve, X, ob = _synthetic()
    tr = sc.truth
    path = _write_inputs(tmp_path, sc, -tr['beta'] / tr['alpha'], True)
    cfg = json.loads(path.read_text())
    ids = 100 + 7 * np.arange(6)
    np.savetxt(tmp_path / 'marks.txt', np.column_stack((ids, X.T)), fmt='%.18e')
    np.savetxt(tmp_path / 'clicks.txt', np.column_stack((ob[0], ids[ob[1].astype(int)], ob[2], ob[3])), fmt='%.18e')
    cfg['optional inputs'] = {'path_landmarks': str(tmp_path / 'marks.txt'), 'path_landmark_observations': str(tmp_path / 'clicks.txt'), 'landmark_sigma': 0.5}
    cfg['settings'].update(ba_solver='lm', ba_covariance=True, ba_landmarks=True)
    path.write_text(json.dumps(cfg))
    flight, timer = pipeline.reconstruct_from_config(str(path), output=False)
    assert 'align_to_landmarks' in [r[0] for r in timer.rows]
    ts = np.arange(np.ceil(flight.spline['int'][0, 0]), np.floor(flight.spline['int'][1, -1]), 1.0)
    traj = flight.spline_to_traj(t=ts)
    Xt = true_curve(traj[0])
    ok = np.all(np.isfinite(Xt), axis=0)
    M = similarity_from_points(traj[1:, ok], Xt[:, ok])
    raw = float(np.sqrt(np.mean(np.sum((traj[1:, ok] - Xt[:, ok]) ** 2, axis=0))))
    fit = float(np.sqrt(np.mean(np.sum((M[:3, :3] @ traj[1:, ok] + M[:3, 3:] - Xt[:, ok]) ** 2, axis=0))))
    scale = float(np.cbrt(np.linalg.det(M[:3, :3])))
    print('pipeline with landmark files: %.4g m against the truth with no alignment, %.4g m after the best similarity, scale %.5f' % (raw, fit, scale))
    assert abs(scale - 1.0) <= 0.01
    assert flight.landmark_observations.shape == (6, 18) and flight.settings['ba_landmarks'] is True
    assert flight.covariance['dof'] > 0 and np.all(np.isfinite(flight.covariance['pos_std'][1:-1]))
