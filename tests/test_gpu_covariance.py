"""mvus_ba_covariance / mvus_spline_cov_eval / Scene.ba_covariance on the GPU.

Reference: the dense H built from the blocks the handle itself exports (normal_equations), restricted to the estimated unknowns and
inverted by numpy with a long-double refinement (test_covariance_host.refined_inverse).  Errors are relative to sqrt(Sigma_ii Sigma_jj).
Bar per matrix: 8 x the loss of LAPACK's own fp64 inverse against that reference on that matrix (recomputed here), floor 1e-12 -- 8 x is
the project's margin for a different order of summation.  Every test prints its measured worst case beside the bar.

Measured on an MI355X, worst / bar: c1_pinhole_2cam 8.2e-10 / 3.1e-8, rs_F_2int_3cam 4.4e-12 / 1.2e-10, dist_fixed_2cam
7.8e-11 / 2.1e-10, calib_KE_wellposed_5cam 2.0e-9 / 1.8e-8, rs_F_2int_3cam with huber(1.5) and an extra ba_freeze 2.0e-12 / 2.7e-12, 20 cameras
9.1e-11 / 5.9e-10, wide band (W = 7) 3.8e-11 / 1.8e-10, N = 46 1.2e-10 / 2.0e-10; standard deviations against the host Jacobian 2.1e-12 (bar 1e-5)."""
import functools

import numpy as np
import pytest

from golden_util import load_case
from frozen_util import ba_kwargs, build_scene
from test_covariance_host import bar_for, host_cov_samples
from mvus_amd import _lib
from mvus_amd import problem as mp

pytestmark = pytest.mark.gpu

CHAIN_CASES = ['c1_pinhole_2cam', 'rs_F_2int_3cam', 'dist_fixed_2cam', 'calib_KE_wellposed_5cam']
ALL_CASES = CHAIN_CASES + ['calib_KE_bounds_3cam']


def internal_index(prob):
    """x index of every unknown in the solver's internal order: camera blocks (alpha, beta, rs, params), then 3 * ctrl + xyz."""
    C, P = prob.C, prob.P
    cam = [[c, C + c, 2 * C + c] + list(range(3 * C + c * P, 3 * C + (c + 1) * P)) for c in range(C)]
    spl = []
    for s, n in enumerate(prob.n_coef):
        for j in range(int(n)):
            spl += [int(prob.spline_x_offsets[s]) + d * int(n) + j for d in range(3)]
    return np.array(cam).ravel(), np.array(spl)


def dense_h(prob, ne):
    """H in the order of x from the exported blocks (g, cam[C, B, B], band[N, W, 3, 3], cross[C, B, 3N])."""
    _, A, band, cross = ne
    C, B, N, W = prob.C, 3 + prob.P, band.shape[0], band.shape[1]
    CB, n = C * B, C * B + 3 * N
    Hi = np.zeros((n, n))
    for c in range(C):
        Hi[c * B:(c + 1) * B, c * B:(c + 1) * B] = A[c]
        Hi[c * B:(c + 1) * B, CB:] = cross[c]
        Hi[CB:, c * B:(c + 1) * B] = cross[c].T
    for g in range(N):
        for w in range(W):
            if g + w < N:
                Hi[CB + 3 * g:CB + 3 * g + 3, CB + 3 * (g + w):CB + 3 * (g + w) + 3] = band[g, w]
                Hi[CB + 3 * (g + w):CB + 3 * (g + w) + 3, CB + 3 * g:CB + 3 * g + 3] = band[g, w].T
    cam_idx, spl_idx = internal_index(prob)
    order = np.concatenate((cam_idx, spl_idx))                 # internal position -> x index
    H = np.zeros((n, n))
    H[np.ix_(order, order)] = Hi
    return H


def check_against_dense(prob, h, x, cv, mask, label):
    """cov / sigma2 against the refined inverse of the exported H on the estimated unknowns; returns (worst, bar)."""
    h.residual_jacobian(x, _lib.JAC_ANALYTIC)
    H = dense_h(prob, h.normal_equations())
    n, CB = H.shape[0], prob.C * (3 + prob.P)
    frozen = np.zeros(n, dtype=bool)
    if mask is not None:
        frozen[:CB] = mask
    want_est = ~frozen & (np.diag(H) != 0)
    assert np.array_equal(cv.estimated, want_est)
    idx = np.nonzero(want_est)[0]
    ref, bar = bar_for(H[np.ix_(idx, idx)])
    full = np.zeros((n, n), dtype=np.longdouble)
    full[np.ix_(idx, idx)] = ref
    sd = np.sqrt(np.diag(full))
    sd[sd == 0] = 1.0
    # camera block
    cam = cv.cam / cv.sigma2
    un = ~want_est[:CB]
    assert not cv.cam[un].any() and not cv.cam[:, un].any()
    worst = float(np.max(np.abs(cam.astype(np.longdouble) - full[:CB, :CB]) / np.outer(sd[:CB], sd[:CB])))
    # every block of the band
    _, spl_idx = internal_index(prob)
    N = spl_idx.size // 3
    for p in range(N):
        for w in range(4):
            got = cv.band[p, w]
            if p + w >= N:
                assert not got.any()
                continue
            r, c = spl_idx[3 * p:3 * p + 3], spl_idx[3 * (p + w):3 * (p + w) + 3]
            zr, zc = ~want_est[r], ~want_est[c]
            assert not got[zr].any() and not got[:, zc].any()
            e = np.abs((got / cv.sigma2).astype(np.longdouble) - full[np.ix_(r, c)]) / np.outer(sd[r], sd[c])
            worst = max(worst, float(e.max()))
    print('covariance %s: n_est %d, worst %.3e, bar %.3e' % (label, idx.size, worst, bar))
    return worst, bar


@functools.lru_cache(maxsize=None)
def _case(name, gauge='anchor'):
    scene, g = load_case(name)
    prob, _ = mp.problem_from_scene(scene)
    mask = build_scene(scene, ba_gauge=gauge).ba_frozen_mask(range(scene.num_cam)) if gauge == 'anchor' else None
    return scene, g, prob, mask


@pytest.mark.parametrize('name', CHAIN_CASES)
def test_chain_against_dense_inverse(name):
    from mvus_amd.ba import BAHandle
    scene, g, prob, mask = _case(name)
    x0 = np.array(g['x0'])
    with BAHandle(prob) as h:
        h.set_frozen(mask)
        cv = h.covariance(x0)
        assert cv.sigma2 > 0 and cv.dof > 0
        worst, bar = check_against_dense(prob, h, x0, cv, mask, name)
    assert worst <= bar


def test_against_an_independent_jacobian():
    """Standard deviations from the dense Jacobian of the host build (frozen columns zeroed).  Bar 1e-5 relative: the assembly is pinned
    to 1e-12 * scale and the scaled condition number of this fixture is 8e5, so 8e-7 is the worst case; the bar is 12 x that."""
    from hostcheck_util import HostHandle
    from mvus_amd.ba import BAHandle
    scene, g, prob, mask = _case('rs_F_2int_3cam')
    x0 = np.array(g['x0'])
    _, J = HostHandle(prob).dense_jacobian(x0, _lib.JAC_ANALYTIC)
    J = J.copy()
    J[:, np.nonzero(mask)[0]] = 0.0
    H = J.T @ J
    est = np.diag(H) != 0
    idx = np.nonzero(est)[0]
    ref, _ = bar_for(H[np.ix_(idx, idx)])
    sd_ref = np.zeros(H.shape[0])
    sd_ref[idx] = np.sqrt(np.diag(ref)).astype(np.float64)
    with BAHandle(prob) as h:
        h.set_frozen(mask)
        cv = h.covariance(x0, sigma2=1.0)
    assert np.array_equal(cv.estimated, est)
    CB = prob.C * (3 + prob.P)
    _, spl_idx = internal_index(prob)
    sd = np.zeros(H.shape[0])
    sd[:CB] = np.sqrt(np.diag(cv.cam))
    sd[spl_idx] = np.sqrt(np.array([cv.band[p, 0, a, a] for p in range(spl_idx.size // 3) for a in range(3)]))
    worst = float(np.max(np.abs(sd[idx] - sd_ref[idx]) / sd_ref[idx]))
    print('standard deviations against the host Jacobian: worst relative %.3e (bar 1e-5)' % worst)
    assert worst <= 1e-5


def test_loss_and_mask_in_force():
    from mvus_amd.ba import BAHandle
    scene, g, prob, _ = _case('rs_F_2int_3cam')
    mask = build_scene(scene, ba_gauge='anchor', ba_freeze={1: ['alpha', 'rs'], 2: ['beta']}).ba_frozen_mask(range(scene.num_cam))
    x0 = np.array(g['x0'])
    with BAHandle(prob) as h:
        h.set_loss('huber', 1.5)
        h.set_frozen(mask)
        cv = h.covariance(x0)
        worst, bar = check_against_dense(prob, h, x0, cv, mask, 'rs_F_2int_3cam huber(1.5) + ba_freeze')
        cost = h.robust_cost(x0)
        _, _, ctrl = h.residual_jacobian(x0, _lib.JAC_ANALYTIC)
    assert worst <= bar
    m_act = h.T + 2 * int((ctrl >= 0).sum())
    assert cv.dof == m_act - int(cv.estimated.sum())
    assert cv.sigma2 == 2.0 * cost / cv.dof


def test_sigma2():
    from mvus_amd.ba import BAHandle
    scene, g, prob, mask = _case('dist_fixed_2cam')
    x0 = np.array(g['x0'])
    with BAHandle(prob) as h:
        h.set_frozen(mask)
        cv = h.covariance(x0)
        cost = h.robust_cost(x0)
        _, _, ctrl = h.residual_jacobian(x0, _lib.JAC_ANALYTIC)
        m_act = h.T + 2 * int((ctrl >= 0).sum())
        assert cv.dof == m_act - int(cv.estimated.sum())
        assert cv.sigma2 == 2.0 * cost / (m_act - int(cv.estimated.sum()))
        one = h.covariance(x0, sigma2=1.0)
        four = h.covariance(x0, sigma2=4.0)
    assert one.sigma2 == 1.0 and four.sigma2 == 4.0 and one.dof == cv.dof
    assert np.array_equal(four.cam, 4.0 * one.cam) and np.array_equal(four.band, 4.0 * one.band)      # (a power of two: exactly linear)
    assert np.array_equal(cv.cam, cv.sigma2 * one.cam) and np.array_equal(cv.band, cv.sigma2 * one.band)


@pytest.mark.parametrize('name', ALL_CASES)
def test_free_gauge_is_refused(name):
    from mvus_amd.ba import BAHandle
    scene, g, prob, _ = _case(name, 'free')
    with BAHandle(prob) as h:
        with pytest.raises(ValueError, match='gauge'):
            h.covariance(np.array(g['x0']))


def test_ill_posed_but_anchored_is_accepted():
    from mvus_amd.ba import BAHandle
    scene, g, prob, mask = _case('calib_KE_bounds_3cam')
    with BAHandle(prob) as h:
        h.set_frozen(mask)
        cv = h.covariance(np.array(g['x0']))
    assert np.isfinite(cv.cam).all() and np.isfinite(cv.band).all() and (np.diag(cv.cam)[cv.estimated[:cv.cam.shape[0]]] > 0).all()


def test_sharded_handle_is_refused():
    from mvus_amd.ba import BAHandle, UnsupportedBySolver
    scene, g, prob, _ = _case('calib_KE_wellposed_5cam')
    N = int(prob.n_coef.sum())
    with BAHandle(prob) as h:
        h.set_time_shard(0, 2, [0, N // 2, N], halo=8)
        with pytest.raises(UnsupportedBySolver, match='sharded'):
            h.covariance(np.array(g['x0']))


def _synth_case(kind):
    from mvus_amd import synth
    if kind == 'cams20':          # CB = 180: more than one panel of the dense Cholesky, more than 144
        sc = synth.make_scene(20, 6000, seed=71)
    elif kind == 'wide':
        # knots closer than a frame, as tests/test_gpu_schur.py builds its wide bands: the motion rows then couple seven control points.
        # That scene's spline runs on where no camera looks (one scalar prior row per frame for 3.75 unknowns: singular, rightly refused),
        # so the spline is cut back to the stretch every camera sees and refitted on knots of the same spacing
        import dataclasses
        from mvus_amd import bspline
        sc = synth.make_scene(4, 400, seed=61, rolling_shutter=True, knot_spacing=0.8, motion_reg=True, motion_type='F', motion_weights=40.0)
        t = [sc.alpha[i] * sc.detections[i][0] + sc.beta[i] for i in range(sc.num_cam)]
        lo, hi = max(v.min() for v in t) + 2.0, min(v.max() for v in t) - 2.0
        kn = bspline.make_knots(lo, hi, 0.8)
        xs = np.linspace(lo, hi, 8 * kn.size)
        c = bspline.lsq_fit(kn, xs, bspline.evaluate(sc.tck[0][0], np.array(sc.tck[0][1]), xs))
        sc = dataclasses.replace(sc, tck=[[kn, [c[0].copy(), c[1].copy(), c[2].copy()], 3]], interval=np.array([[lo], [hi]]))
    else:                         # N = 46: not a multiple of the 16 control points of a row tile of stage 6
        sc = synth.make_scene(3, 3000, seed=31, rolling_shutter=True, num_knots=43)
    prob, x0 = mp.problem_from_scene(sc)
    s = build_scene(sc, ba_gauge='anchor')
    return prob, x0, s.ba_frozen_mask(range(sc.num_cam))


@pytest.mark.parametrize('kind', ['cams20', 'wide', 'ragged'])
def test_shapes_where_the_kernels_can_go_wrong(kind):
    from mvus_amd.ba import BAHandle
    prob, x0, mask = _synth_case(kind)
    N = int(prob.n_coef.sum())
    with BAHandle(prob) as h:
        h.set_frozen(mask)
        cv = h.covariance(x0)
        h.residual_jacobian(x0, _lib.JAC_ANALYTIC)
        W = h.normal_equations()[2].shape[1]
        worst, bar = check_against_dense(prob, h, x0, cv, mask, '%s (C %d, N %d, W %d)' % (kind, prob.C, N, W))
    if kind == 'cams20':
        assert prob.C * (3 + prob.P) == 180
    if kind == 'wide':
        assert 7 <= W <= 16
    if kind == 'ragged':
        assert N % 16 != 0 and N > 16
    assert worst <= bar


def test_no_side_effect_on_later_solves():
    from mvus_amd.ba import BAHandle
    scene, g, prob, mask = _case('rs_F_2int_3cam')
    x0 = np.array(g['x0'])
    lm = dict(solver=_lib.SOLVER_LM_SCHUR, jac_mode=_lib.JAC_ANALYTIC, max_nfev=4)
    with BAHandle(prob) as h:
        h.set_frozen(mask)
        a1 = h.solve(x0, **lm)
        c1 = h.covariance(a1.x)
        c2 = h.covariance(a1.x)
        a2 = h.solve(a1.x, **lm)
    with BAHandle(prob) as h:
        h.set_frozen(mask)
        b1 = h.solve(x0, **lm)
        b2 = h.solve(b1.x, **lm)
    assert np.array_equal(a1.x, b1.x)
    assert np.array_equal(a2.x, b2.x) and a2.cost == b2.cost and (a2.nfev, a2.status) == (b2.nfev, b2.status)
    assert np.array_equal(c1.cam, c2.cam) and np.array_equal(c1.band, c2.band) and c1.sigma2 == c2.sigma2 and c1.dof == c2.dof


def test_spline_cov_eval_against_the_host_formula():
    from mvus_amd import spline
    scene, g, prob, _ = _case('rs_F_2int_3cam')                 # two intervals: a gap between them
    rng = np.random.default_rng(3)
    N = int(prob.n_coef.sum())
    A = rng.standard_normal((3 * N, 3 * N))
    Sigma = A @ A.T
    band = np.zeros((N, 4, 3, 3))
    for p in range(N):
        for w in range(4):
            if p + w < N:
                band[p, w] = Sigma[3 * p:3 * p + 3, 3 * (p + w):3 * (p + w) + 3]
    iv = scene.interval
    inner = [k for tck in scene.tck for k in tck[0][4:-4:3]]                                  # knots
    ts = np.array(list(iv[0]) + list(iv[1]) + inner + [iv[0, 0] - 1.0, 0.5 * (iv[1, 0] + iv[0, 1]), iv[1, -1] + 2.0]
                  + list(rng.uniform(iv[0, 0], iv[1, -1], 40)))
    cov, which = spline.cov_evaluate(scene.tck, iv, band, ts)
    want = host_cov_samples(scene.tck, iv, band, ts)
    out = which < 0
    assert out.sum() >= 3 and np.isnan(cov[out]).all() and np.isnan(want[out]).all()
    assert not np.isnan(cov[~out]).any()
    scale = np.abs(want[~out]).max(axis=(1, 2), keepdims=True)
    assert np.max(np.abs(cov[~out] - want[~out]) / scale) <= 1e-12


def test_scene_ba_covariance_names_the_handle_numbers():
    scene, g, prob, mask = _case('calib_KE_wellposed_5cam')
    s = build_scene(scene, ba_gauge='anchor', ba_solver='lm')
    cams = list(range(scene.num_cam))
    ts = np.array([float(scene.interval[0, 0]) - 5.0] + list(np.linspace(scene.interval[0, 0], scene.interval[1, -1], 7)))
    out = s.ba_covariance(cams, t=ts, **ba_kwargs(s.settings))
    assert s.covariance is out
    h = s._ba_handle
    x = s._pack(h.prob, cams)
    cv = h.covariance(x)
    C, P = prob.C, prob.P
    assert np.array_equal(out['cam_cov'], cv.cam) and np.array_equal(out['band'], cv.band)
    assert out['sigma2'] == cv.sigma2 and out['dof'] == cv.dof and out['cams'] == cams
    assert out['param_names'] == ['fx', 'fy', 'cx', 'cy', 'r1', 'r2', 'r3', 't1', 't2', 't3', 'k1', 'k2', 'p1', 'p2', 'k3']
    sd = np.sqrt(np.diag(cv.cam))
    for k in cams:
        assert out['cam_std'][k]['alpha'] == sd[k] and out['cam_std'][k]['beta'] == sd[C + k] and out['cam_std'][k]['rs'] == sd[2 * C + k]
        assert out['cam_std'][k]['fx'] == sd[3 * C + k * P] and out['cam_std'][k]['k3'] == sd[3 * C + k * P + 14]
    assert not any(out['cam_std'][0][n] for n in ('r1', 'r2', 'r3', 't1', 't2', 't3'))      # the anchor
    assert np.isnan(out['pos_cov'][0]).all() and np.isnan(out['pos_std'][0]).all()
    want = host_cov_samples(s.spline['tck'], s.spline['int'], cv.band, ts)
    scale = np.abs(want[1:]).max(axis=(1, 2), keepdims=True)
    assert np.max(np.abs(out['pos_cov'][1:] - want[1:]) / scale) <= 1e-12
    assert np.array_equal(out['pos_std'][1:], np.sqrt(np.einsum('tii->ti', out['pos_cov'][1:])))
    import pickle
    back = pickle.loads(pickle.dumps(s))
    assert np.array_equal(back.covariance['cam_cov'], out['cam_cov'])


@pytest.mark.parametrize('enabled', [True, False])
def test_reconstruct_from_config_carries_the_covariance(tmp_path, enabled):
    import json
    import pickle
    from mvus_amd import pipeline, synth
    from test_gpu_init_pipeline import _write_inputs
    # Three cameras and the motion prior: with two, the trajectory the loop ends with has an end control point that one camera alone sees,
    # whose depth nothing determines -- that problem is, rightly, refused (measured: every two-camera variant tried was)
    sc = synth.make_scene(3, 4500, seed=31, perturb=0.3, motion_reg=True, motion_type='F', motion_weights=1e2)
    cf = -sc.truth['beta'] / sc.truth['alpha']
    path = _write_inputs(tmp_path, sc, cf, True)
    cfg = json.loads(path.read_text())
    cfg['settings'].update(ba_solver='lm', ba_gauge='anchor')
    if enabled:
        cfg['settings']['ba_covariance'] = True
    path.write_text(json.dumps(cfg))
    flight, timer = pipeline.reconstruct_from_config(str(path))
    with open(flight.settings['path_output'], 'rb') as fh:
        back = pickle.load(fh)
    if not enabled:
        assert 'covariance' not in vars(back) and 'ba_covariance' not in [r[0] for r in timer.rows]
        return
    cov = back.covariance
    assert 'ba_covariance' in [r[0] for r in timer.rows]
    assert cov['cams'] == list(flight.sequence) and cov['sigma2'] > 0 and cov['dof'] > 0
    assert cov['cam_cov'].shape == (27, 27) and cov['pos_cov'].shape == (flight.traj.shape[1], 3, 3)
    assert np.array_equal(cov['t'], flight.traj[0]) and np.isfinite(cov['pos_std']).all() and (cov['pos_std'] > 0).all()
