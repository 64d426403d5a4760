"""scipy's robust losses in the LM + Schur bundle adjustment (mvus_ba_set_loss / mvus_ba_robust_cost; settings ba_loss, ba_f_scale).

The reference for every number is scipy through its public API (tests/robust_reference.py): least_squares(loss=, f_scale=, max_nfev=1)
at a fixed x gives the robust cost, the gradient J^T (rho' f) and the scaled Jacobian diag(s) J; the dense J is the host build's
(HostHandle.dense_jacobian), the raw residuals are the library's own and the oracle's.  Tolerances are those of the linear tests of
tests/test_gpu_schur.py, unchanged."""
import functools

import numpy as np
import pytest

from oracle import ba_oracle as orc
from golden_util import CASES, ground_truth_x, load_case
from lm_reference import lapack_lm_step
from mvus_amd import _lib
from mvus_amd import problem as mp
import robust_reference as rr

pytestmark = pytest.mark.gpu

F_SCALE = 3.0
LM = dict(solver=_lib.SOLVER_LM_SCHUR, jac_mode=_lib.JAC_ANALYTIC)


def internal_index(prob):
    """x index of every unknown in the solver's internal order: camera blocks (alpha, beta, rs, params), then 3 * ctrl + xyz."""
    C, P = prob.C, prob.P
    cam = [[c, C + c, 2 * C + c] + list(range(3 * C + c * P, 3 * C + (c + 1) * P)) for c in range(C)]
    spl = []
    for s, n in enumerate(prob.n_coef):
        for j in range(int(n)):
            spl += [int(prob.spline_x_offsets[s]) + d * int(n) + j for d in range(3)]
    return np.array(cam), np.array(spl)


@functools.lru_cache(maxsize=None)
def _case(name):
    scene, g = load_case(name)
    prob, _ = mp.problem_from_scene(scene)
    oprob, _ = orc.problem_from_scene(scene)
    return scene, g, prob, oprob


@functools.lru_cache(maxsize=None)
def _dense(key):
    """f, J (dense, host build) at the test point of a golden case or of the mid-size scene."""
    from hostcheck_util import HostHandle
    prob, x = _problem(key)
    return HostHandle(prob).dense_jacobian(x, _lib.JAC_ANALYTIC)


@functools.lru_cache(maxsize=None)
def _problem(key):
    if isinstance(key, str):
        _, g, prob, _ = _case(key)
        return prob, g['x0'] + g['delta']
    from mvus_amd import synth
    if key[0] == 'wide':          # knots closer than a frame (test_wide_band_knots_closer_than_a_frame): the band is wider than six control points
        sc = synth.make_scene(3, 420, seed=61, rolling_shutter=True, knot_spacing=key[1], motion_reg=True, motion_type='F', motion_weights=40.0)
        return mp.problem_from_scene(sc)
    sc = synth.make_scene(6, 9000, seed=61, rolling_shutter=True, num_knots=150, opt_calib=key[1], motion_reg=True, motion_type='F',
                          motion_weights=10.0)
    return mp.problem_from_scene(sc)


def _blocks(prob, H):
    """The solver's blocks cut out of a dense H (x order): camera blocks, band (with the check that nothing lies outside it when a
    width is given), cross block."""
    cam_idx, spl_idx = internal_index(prob)
    Hs = H[np.ix_(spl_idx, spl_idx)]
    E = H[np.ix_(cam_idx.ravel(), spl_idx)]
    A = np.stack([H[np.ix_(cam_idx[c], cam_idx[c])] for c in range(prob.C)])
    return A, Hs, E


def _check_normal_equations(prob, ne, grad, H):
    gg, A, band, cross = ne
    A_ref, Hs, E = _blocks(prob, H)
    scale = np.abs(H).max()
    np.testing.assert_allclose(gg, grad, rtol=0, atol=1e-11 * np.abs(grad).max())
    np.testing.assert_allclose(A, A_ref, rtol=0, atol=1e-12 * scale)
    N, W = band.shape[0], band.shape[1]
    covered = np.zeros_like(Hs, dtype=bool)
    for gi in range(N):
        for w in range(W):
            if gi + w < N:
                np.testing.assert_allclose(band[gi, w], Hs[3 * gi:3 * gi + 3, 3 * (gi + w):3 * (gi + w) + 3], rtol=0, atol=1e-12 * scale)
                covered[3 * gi:3 * gi + 3, 3 * (gi + w):3 * (gi + w) + 3] = True
                covered[3 * (gi + w):3 * (gi + w) + 3, 3 * gi:3 * gi + 3] = True
    assert not Hs[~covered].any()                                   # nothing outside the band
    np.testing.assert_allclose(cross.reshape(E.shape), E, rtol=0, atol=1e-12 * scale)


def _band_from_dense(Hs, N, W):
    band = np.zeros((N, W, 3, 3))
    for gi in range(N):
        for w in range(W):
            if gi + w < N:
                band[gi, w] = Hs[3 * gi:3 * gi + 3, 3 * (gi + w):3 * (gi + w) + 3]
    return band


def _at_fixed_x(key, loss, monkeypatch):
    """Items 1 - 4 of the issue at one point: robust cost and weights, the robust normal equations on both assembly routes, that they
    are not the linear ones, and the damped step."""
    from mvus_amd.ba import BAHandle
    prob, x = _problem(key)
    f_host, D = _dense(key)
    with BAHandle(prob) as h:
        f = h.residual(x)
        h.residual_jacobian(x, _lib.JAC_ANALYTIC)
        ne_lin = h.normal_equations()
        h.set_loss(loss, F_SCALE)
        # 1. cost and weights against scipy fed the library's own raw residuals
        cost, w = h.robust_cost(x, weights=True)
        ref_cost = rr.scipy_cost(f, loss, F_SCALE)
        print('%s %s: robust cost %.17g (scipy %.17g, rel %.3g), rows beyond f_scale %.1f %%'
              % (key, loss, cost, ref_cost, abs(cost - ref_cost) / ref_cost, 100.0 * np.mean(np.abs(f) > F_SCALE)))
        np.testing.assert_allclose(cost, ref_cost, rtol=1e-12)
        np.testing.assert_allclose(w, rr.weights(f, loss, F_SCALE), rtol=0, atol=1e-14)
        assert np.array_equal(h.residual(x), f)                                          # error_BA stays raw
        if isinstance(key, str):
            np.testing.assert_allclose(cost, rr.scipy_cost(orc.residual(_case(key)[3], x), loss, F_SCALE), rtol=1e-9)
        # 2. the robust normal equations: window-major route
        _, grad, Js = rr.scipy_at(f_host, D, loss, F_SCALE)
        H = Js.T @ Js
        monkeypatch.delenv('MVUS_NE_FROM_J', raising=False)
        fj, J, _ = h.residual_jacobian(x, _lib.JAC_ANALYTIC)
        np.testing.assert_allclose(fj, f, rtol=0, atol=1e-9)                             # raw, whatever loss is set (the Jacobian kernel's own rounding)
        ne = h.normal_equations()
        assert not h.deterministic_fallback()
        _check_normal_equations(prob, ne, grad, H)
        # 3. not vacuous: these are not the linear blocks
        H_lin = D.T @ D
        assert np.abs(H - H_lin).max() > 1e-3 * np.abs(H_lin).max()
        assert max(np.abs(a - b).max() for a, b in zip(ne[1:], ne_lin[1:])) > 1e-3 * max(np.abs(b).max() for b in ne_lin[1:])
        # 4. the damped step of the whole solve chain against LAPACK fed the reference's robust blocks
        A_ref, Hs, E = _blocks(prob, H)
        band_ref = _band_from_dense(Hs, ne[2].shape[0], ne[2].shape[1])
        for lam in (1e-3, 1.0):
            p_ref = lapack_lm_step(prob, grad, A_ref, band_ref, E.reshape(prob.C, -1, E.shape[1]), lam)
            p = h.lm_step(lam)
            np.testing.assert_allclose(p, p_ref, rtol=0, atol=1e-7 * np.abs(p_ref).max())
    # 2. again, from the stored Jacobian blocks (detection-major kernel)
    monkeypatch.setenv('MVUS_NE_FROM_J', '1')
    with BAHandle(prob) as h:
        h.set_loss(loss, F_SCALE)
        h.residual_jacobian(x, _lib.JAC_ANALYTIC)
        ne_j = h.normal_equations()
        assert h.deterministic_fallback()
        _check_normal_equations(prob, ne_j, grad, H)
    monkeypatch.delenv('MVUS_NE_FROM_J', raising=False)


@pytest.mark.parametrize('loss', rr.ROBUST)
@pytest.mark.parametrize('name', CASES)
def test_cost_weights_normal_equations_and_step_at_fixed_x(name, loss, monkeypatch):
    monkeypatch.delenv('MVUS_WIN', raising=False)
    _at_fixed_x(name, loss, monkeypatch)


@pytest.mark.parametrize('calib', [False, True])
@pytest.mark.parametrize('win', [None, '4', '9'])
def test_huber_mid_size_every_window_length(calib, win, monkeypatch):
    """The scene of test_window_major_assembly_against_dense_host_jtj_mid_size: several 64-detection batches per window and camera,
    B = 9 and B = 18, motion rows, 2 % outliers."""
    if win is None:
        monkeypatch.delenv('MVUS_WIN', raising=False)
    else:
        monkeypatch.setenv('MVUS_WIN', win)
    monkeypatch.delenv('MVUS_ASM_ATOMIC', raising=False)
    _at_fixed_x(('mid', calib), 'huber', monkeypatch)


def _repeat_bits(prob, x_solve, x_ne, loss):
    """5. Three fresh handles: one (cost, x) of a six-evaluation solve, one set of bits of the robust normal equations."""
    from mvus_amd.ba import BAHandle
    sols, nes = [], []
    for _ in range(3):
        with BAHandle(prob) as h:
            h.set_loss(loss, F_SCALE)
            r = h.solve(x_solve, max_nfev=6, **LM)
            assert not h.deterministic_fallback()
            sols.append((r.cost, r.x.copy(), r.nfev, r.status))
        with BAHandle(prob) as h:
            h.set_loss(loss, F_SCALE)
            h.residual_jacobian(x_ne, _lib.JAC_ANALYTIC)
            nes.append(h.normal_equations())
            assert not h.deterministic_fallback()
    for cost, x, nfev, status in sols[1:]:
        assert cost == sols[0][0] and np.array_equal(x, sols[0][1]) and (nfev, status) == sols[0][2:]
    for ne in nes[1:]:
        for a, b in zip(nes[0], ne):
            assert np.array_equal(a, b)


@pytest.mark.parametrize('loss', rr.ROBUST)
@pytest.mark.parametrize('name', CASES)
def test_robust_solves_and_assemblies_repeat_bit_for_bit(name, loss, monkeypatch):
    monkeypatch.delenv('MVUS_WIN', raising=False)
    _, g, prob, _ = _case(name)
    _repeat_bits(prob, g['x0'], g['x0'] + g['delta'], loss)


@pytest.mark.parametrize('calib', [False, True])
@pytest.mark.parametrize('win', [None, '4', '9'])
def test_huber_mid_size_repeats_bit_for_bit(calib, win, monkeypatch):
    """5. on the scene with several 64-detection batches per window and several windows per camera: where a broken one-writer property
    would show."""
    if win is None:
        monkeypatch.delenv('MVUS_WIN', raising=False)
    else:
        monkeypatch.setenv('MVUS_WIN', win)
    prob, x0 = _problem(('mid', calib))
    _repeat_bits(prob, x0, x0, 'huber')


def test_wide_band_motion_rows_at_fixed_x(monkeypatch):
    """Items 1 - 4 where the motion rows couple more than six control points (k_det_motion_wide, general band solver)."""
    monkeypatch.delenv('MVUS_WIN', raising=False)
    from mvus_amd.ba import BAHandle
    prob, x0 = _problem(('wide', 0.45))
    with BAHandle(prob) as h:
        h.residual_jacobian(x0, _lib.JAC_ANALYTIC)
        assert h.normal_equations()[2].shape[1] > 6
    _at_fixed_x(('wide', 0.45), 'huber', monkeypatch)


@pytest.mark.parametrize('name', CASES)
def test_fused_detection_major_fallback_solves_the_same_robust_problem(name, monkeypatch):
    """MVUS_ASM_ATOMIC=1 sends the fused linearisation of a solve through the detection-major kernel (what unsorted frames or more
    than 256 cameras do): the same optimisation as the window-major one, to the bar test_window_assembly_matches_and_repeats sets
    for the linear system (1e-9 of the cost: fp64 atomics, another order of additions).  Twelve evaluations: on rs_F_2int_3cam the first five trials
    are rejected while the damping grows."""
    from mvus_amd.ba import BAHandle
    _, g, prob, oprob = _case(name)
    monkeypatch.delenv('MVUS_ASM_ATOMIC', raising=False)
    with BAHandle(prob) as h:
        h.set_loss('huber', F_SCALE)
        r_w = h.solve(g['x0'], max_nfev=12, **LM)
        assert not h.deterministic_fallback()
    monkeypatch.setenv('MVUS_ASM_ATOMIC', '1')
    with BAHandle(prob) as h:
        h.set_loss('huber', F_SCALE)
        r_a = h.solve(g['x0'], max_nfev=12, **LM)
        assert h.deterministic_fallback()
    monkeypatch.delenv('MVUS_ASM_ATOMIC', raising=False)
    print('%s: window-major %.12g, detection-major %.12g (initial %.12g)' % (name, r_w.cost, r_a.cost, r_w.initial_cost))
    assert r_w.cost < r_w.initial_cost and r_a.nfev == r_w.nfev
    assert abs(r_w.cost - r_a.cost) <= 1e-9 * r_w.cost
    np.testing.assert_allclose(r_a.cost, rr.scipy_cost(orc.residual(oprob, r_a.x), 'huber', F_SCALE), rtol=1e-9)


@pytest.mark.parametrize('name', CASES)
def test_linear_is_untouched(name):
    """6. set_loss('linear', 1.0) -- and huber set, then linear again -- solves bit for bit like a handle that never heard of losses."""
    from mvus_amd.ba import BAHandle
    _, g, prob, _ = _case(name)

    def run(prepare):
        with BAHandle(prob) as h:
            prepare(h)
            r = h.solve(g['x0'], max_nfev=10, **LM)
            return r.cost, r.initial_cost, r.x.copy(), r.nfev, r.njev, r.status

    def back_to_linear(h):
        h.set_loss('huber', F_SCALE)
        h.set_loss('linear', 1.0)
    base = run(lambda h: None)
    for other in (run(lambda h: h.set_loss('linear', 1.0)), run(back_to_linear), run(lambda h: h.set_loss(_lib.LOSS_LINEAR, 1.0))):
        assert other[:2] == base[:2] and np.array_equal(other[2], base[2]) and other[3:] == base[3:]


@pytest.mark.parametrize('name', CASES)
def test_set_loss_drops_what_a_linear_solve_carried_over(name):
    """7. Solve linear, set huber, solve from the returned x: the same bits as a fresh handle with huber set solving from that x (the
    carried cost and normal equations were the linear problem's)."""
    from mvus_amd.ba import BAHandle
    _, g, prob, _ = _case(name)
    with BAHandle(prob) as h:
        r0 = h.solve(g['x0'], max_nfev=6, return_fun=False, **LM)
        h.set_loss('huber', F_SCALE)
        r1 = h.solve(r0.x, max_nfev=6, **LM)
    with BAHandle(prob) as h:
        h.set_loss('huber', F_SCALE)
        r2 = h.solve(r0.x, max_nfev=6, **LM)
    assert r1.initial_cost == r2.initial_cost and r1.initial_cost < r0.cost            # huber's cost of that point, not the linear one
    assert (r1.cost, r1.nfev, r1.njev, r1.status) == (r2.cost, r2.nfev, r2.njev, r2.status)
    assert np.array_equal(r1.x, r2.x) and np.array_equal(r1.fun, r2.fun)


def test_refusals():
    """8. What the loss does not reach refuses by name; bad arguments are MVUS_E_INVALID."""
    from mvus_amd.ba import BAHandle, UnsupportedBySolver
    _, g, prob, _ = _case('rs_F_2int_3cam')
    x0 = g['x0']
    with BAHandle(prob) as h:
        for bad in ((99, 1.0), (-1, 1.0), (_lib.LOSS_HUBER, 0.0), (_lib.LOSS_HUBER, -2.0), (_lib.LOSS_HUBER, float('nan')),
                    (_lib.LOSS_HUBER, float('inf'))):
            assert h.lib.mvus_ba_set_loss(h.h, bad[0], bad[1]) == _lib.MVUS_E_INVALID, bad
            with pytest.raises(ValueError):
                h.set_loss(*bad)
        assert h.loss == (_lib.LOSS_LINEAR, 1.0)
        h.set_loss('huber', F_SCALE)
        with pytest.raises(UnsupportedBySolver, match='TRF_LSMR'):                        # (a)
            h.solve(x0, solver=_lib.SOLVER_TRF_LSMR, jac_mode=_lib.JAC_ANALYTIC, max_nfev=3)
        with pytest.raises(UnsupportedBySolver, match='TRF_LSMR'):
            h.solve(x0, solver=_lib.SOLVER_TRF_LSMR, jac_mode=_lib.JAC_PATTERN, max_nfev=3)
        for mode in (_lib.JAC_PATTERN, _lib.JAC_FD):                                      # (b)
            with pytest.raises(UnsupportedBySolver, match='MVUS_JAC_ANALYTIC'):
                h.solve(x0, solver=_lib.SOLVER_LM_SCHUR, jac_mode=mode, max_nfev=3)
        o = _lib.default_opts(_lib.SOLVER_TRF_LSMR, _lib.JAC_ANALYTIC, 3)
        res = _lib.MvusResult()
        x = np.array(x0)
        assert h.lib.mvus_ba_solve(h.h, _lib.dptr(x), o, res, None) == _lib.MVUS_E_UNSUPPORTED
        assert np.array_equal(x, x0)
        r = h.solve(x0, max_nfev=10, **LM)                                                # the supported combination still solves
        assert r.cost < r.initial_cost
        h.set_loss('linear')
        assert h.solve(x0, solver=_lib.SOLVER_TRF_LSMR, jac_mode=_lib.JAC_PATTERN, max_nfev=3).nfev >= 1
    with BAHandle(prob) as h:                                                             # (c) an all-reduce route
        h.set_loss('cauchy', F_SCALE)
        h.set_allreduce(lambda buf, count, stream: None)
        with pytest.raises(UnsupportedBySolver, match='sharded'):
            h.solve(x0, max_nfev=3, **LM)
        with pytest.raises(UnsupportedBySolver, match='sharded'):
            h.robust_cost(x0)
    with BAHandle(prob) as h:                                                             # (c) a time shard
        N = int(prob.n_coef.sum())
        h.set_time_shard(0, 2, [0, N // 2, N])
        h.set_loss('huber', F_SCALE)
        with pytest.raises(UnsupportedBySolver, match='sharded'):
            h.solve(x0, max_nfev=3, **LM)
    with BAHandle(prob) as h:                                                             # (c) the library's own RCCL communicator
        from mvus_amd.dist import join_rccl
        ok, why = join_rccl(h, 0, 1)
        assert ok, why
        h.set_loss('huber', F_SCALE)
        with pytest.raises(UnsupportedBySolver, match='sharded'):
            h.solve(x0, max_nfev=3, **LM)


def test_scene_refuses_the_fallback_that_would_drop_the_loss():
    """8. Knots closer than a frame: the wide-band policy hands the problem to TRF -- with a loss set Scene.BA raises instead and the
    Scene keeps its state."""
    from mvus_amd import synth
    from mvus_amd.ba import UnsupportedBySolver
    from test_gpu_scene import build_scene
    sc = synth.make_scene(3, 420, seed=61, rolling_shutter=True, knot_spacing=0.45, motion_reg=True, motion_type='F', motion_weights=40.0)
    s = build_scene(sc)
    s.settings.update(ba_solver='lm', ba_loss='huber', ba_f_scale=F_SCALE)
    before = (s.alpha.copy(), s.beta.copy(), s.rs.copy(), [np.array(c) for c in s.spline['tck'][0][1]], s.cameras[1].R.copy(), s.cameras[1].t.copy())
    kw = dict(rs=True, motion_reg=True, motion_weights=40.0)
    with pytest.raises(UnsupportedBySolver, match='ba_loss'):
        s.BA(s.numCam, **kw)
    after = (s.alpha, s.beta, s.rs, s.spline['tck'][0][1], s.cameras[1].R, s.cameras[1].t)
    for a, b in zip(before[:3] + before[4:], after[:3] + after[4:]):
        assert np.array_equal(a, b)
    for a, b in zip(before[3], after[3]):
        assert np.array_equal(a, b)
    s.settings.update(ba_loss='linear')                      # the linear problem still takes the announced fallback
    res = s.BA(s.numCam, **kw)
    assert res.solver_used.startswith('trf (fallback')


def _robust_cost_oracle(oprob, x, loss, f_scale):
    return rr.scipy_cost(orc.residual(oprob, x), loss, f_scale)


@pytest.mark.parametrize('loss', ['huber', 'cauchy'])
@pytest.mark.parametrize('name', CASES)
def test_robust_solve_cost_is_the_oracles_and_not_worse_than_scipy(name, loss):
    """9, 10. From the fixture's x0, outliers in, 40 evaluations: the reported costs are scipy's formula on the oracle's residuals, and
    the final cost is not above what the reference's own call reaches with the same loss in its 10 evaluations."""
    from scipy.optimize import least_squares
    from mvus_amd.ba import BAHandle
    _, g, prob, oprob = _case(name)
    x0 = g['x0']
    with BAHandle(prob) as h:
        h.set_loss(loss, F_SCALE)
        r = h.solve(x0, max_nfev=40, **LM)
        f_raw = h.residual(r.x)
    assert np.array_equal(r.fun, f_raw)                                                   # f_out is the raw error_BA(x)
    np.testing.assert_allclose(r.cost, _robust_cost_oracle(oprob, r.x, loss, F_SCALE), rtol=1e-9)
    np.testing.assert_allclose(r.initial_cost, _robust_cost_oracle(oprob, x0, loss, F_SCALE), rtol=1e-9)
    ref = least_squares(lambda x: orc.residual(oprob, x), np.asarray(x0, float), jac_sparsity=orc.jac_pattern(oprob, x0), tr_solver='lsmr',
                        xtol=1e-12, max_nfev=10, bounds=orc.bounds(oprob), loss=loss, f_scale=F_SCALE)
    print('%s %s: cost %.8g after %d evaluations (initial %.8g), scipy trf/lsmr 10 evaluations %.8g, ratio %.4f'
          % (name, loss, r.cost, r.nfev, r.initial_cost, ref.cost, r.cost / ref.cost))
    assert r.cost <= ref.cost
    if prob.rs_bounds:
        rs = r.x[2 * prob.C:3 * prob.C]
        assert np.all((rs >= 0) & (rs <= 1))


# scipy's own figures (exact trust-region steps, analytic Jacobian, 40 evaluations): trajectory RMS distance to the truth [m] with
# huber, f_scale 1.5 -- below these a linear run says nothing about the loss (the issue's table)
SCIPY_HUBER_1P5 = {'c1_pinhole_2cam': 1.468, 'rs_F_2int_3cam': 0.019, 'calib_KE_bounds_3cam': 0.912, 'dist_fixed_2cam': 0.221}


def test_huber_ends_closer_to_the_truth_than_linear():
    """11. First BA, outliers in, no outlier removal: the trajectory after huber (f_scale 1.5) is closer to the generator's ground
    truth than after the plain sum of squares.  Direction only.  A fixture on which the damped linear run already ends closer than
    scipy's HUBER figure is not counted (the damping floor holds weakly determined directions in place); at most one of the four."""
    import gauge
    from mvus_amd.ba import BAHandle
    skipped, rows = [], []
    for name in CASES:
        _, g, prob, oprob = _case(name)
        truth = ground_truth_x(oprob, name)
        out = {}
        for loss, fs in (('linear', 1.0), ('huber', 1.5)):
            with BAHandle(prob) as h:
                h.set_loss(loss, fs)
                r = h.solve(g['x0'], max_nfev=40, return_fun=False, **LM)
            out[loss] = float(gauge.compare(oprob, truth, r.x)['traj_rms'])
        rows.append((name, out['linear'], out['huber']))
        print('%s: traj_rms linear %.4f m, huber(1.5) %.4f m, ratio %.2f (scipy huber %.3f m)'
              % (name, out['linear'], out['huber'], out['linear'] / out['huber'], SCIPY_HUBER_1P5[name]))
        if out['linear'] < SCIPY_HUBER_1P5[name]:
            skipped.append(name)
            continue
    for name, lin, hub in rows:
        if name not in skipped:
            assert hub < lin, (name, lin, hub)
    assert len(skipped) <= 1, skipped


def test_scene_ba_with_huber_equals_the_handle_and_downweights_the_outliers():
    """12. Scene.BA with ba_loss / ba_f_scale: the handle-level solve bit for bit, the Scene updated as by a linear BA; at the result
    every detection the fixture's outlier mask rejects has weight < 0.5 (the smaller rho' of its two rows) and no kept one has."""
    from mvus_amd.ba import BAHandle
    from test_gpu_scene import build_scene
    name = 'rs_F_2int_3cam'
    scene, g, prob, oprob = _case(name)
    st = scene.settings
    s = build_scene(scene)
    s.settings.update(ba_solver='lm', ba_loss='huber', ba_f_scale=F_SCALE)
    assert s._motion_band_width(prob) <= 6                       # the wide-band policy does not step in
    kw = dict(rs=st['rolling_shutter'], motion_reg=st['motion_reg'], motion_weights=st['motion_weights'], rs_bounds=st['rs_bounds'])
    cams = list(s.sequence[:s.numCam])
    prob = s._ba_problem(cams, **kw)                             # the problem and the start Scene.BA itself packs (x0 of the fixture to rounding)
    x_start = s._pack(prob, cams)
    np.testing.assert_allclose(x_start, g['x0'], rtol=0, atol=1e-9)
    res = s.BA(s.numCam, max_iter=40, **kw)
    assert res.solver_used == 'lm' and s._ba_handle.loss == (_lib.LOSS_HUBER, F_SCALE)
    with BAHandle(prob) as h:
        h.set_loss('huber', F_SCALE)
        r = h.solve(x_start, max_nfev=40, **LM)
        cost, w = h.robust_cost(r.x, weights=True)
    assert res.cost == r.cost and np.array_equal(res.x, r.x) and (res.nfev, res.status) == (r.nfev, r.status)
    np.testing.assert_allclose(cost, r.cost, rtol=1e-12)
    alpha, beta, rs_new, cams, coefs = mp.unpack_x(prob, r.x)
    assert np.array_equal(s.alpha, alpha) and np.array_equal(s.beta, beta) and np.array_equal(s.rs, rs_new)
    for k in range(prob.C):
        assert np.array_equal(s.cameras[k].R, cams[k]['R']) and np.array_equal(s.cameras[k].t, cams[k]['t'])
    for i, c in enumerate(coefs):
        assert np.array_equal(np.asarray(s.spline['tck'][i][1]), np.asarray(c))
    assert s.global_traj.shape[0] == 7
    keep = g['outlier_keep'].astype(bool)
    off = g['det_offsets']
    wd = np.empty(prob.M)
    for c in range(prob.C):
        a, b = int(off[c]), int(off[c + 1])
        wd[a:b] = np.minimum(w[2 * a:2 * a + (b - a)], w[2 * a + (b - a):2 * b])
    print('%s: %d of %d rejected detections have weight < 0.5, %d of %d kept ones' %
          (name, int((wd[~keep] < 0.5).sum()), int((~keep).sum()), int((wd[keep] < 0.5).sum()), int(keep.sum())))
    assert np.all(wd[~keep] < 0.5)
    assert not np.any(wd[keep] < 0.5)
