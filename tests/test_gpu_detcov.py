"""mvus_ba_detection_covariance / Scene.ba_detection_covariance / the ``ba_detection_covariance`` setting on the GPU.

Reference: sigma^2 x the long-double-refined inverse (test_covariance_host.refined_inverse) of the dense H built from the blocks the handle
itself exports, restricted to the estimated unknowns; J_i from the slots of ``h.residual_jacobian(x)`` scattered into dense rows with the
frozen columns zeroed; the quadratic forms in long double.  Error measure: |P - P_ref| / sqrt(P_ref,uu P_ref,vv).  Bar per case: 8 x the
loss of numpy's own fp64 inverse pushed through the same three-term split (a Scc a^T - (a T^T b^T + transpose) + b G b^T) in fp64, floor
1e-12 -- 8 x is the project's margin for a different order of summation -- and no bar above 1e-5 (bar_of).  t2 is compared with the long-double
r^T (sigma^2 I - Pi_ref)^-1 r, relative, to that bar / (1 - the largest per-axis leverage).  Every test prints its worst case beside the bar.

Signs: the 50-digit fixture (tests/golden/mp_jacobian.npz, rows of tests/mp_observation.py) stores |residual| and the rows
D dr/dx, D = diag(sign r) of the 50-digit (predicted - observed).  u_cal = fx Xc_x / Xc_z + cx, so dr_u / dt_x = fx / Xc_z and
dr_v / dt_y = fy / Xc_z exactly: the sign of those two stored entries times the sign of the depth Xc_z IS the 50-digit sign (the case
'geometry' holds points behind the camera; the depth's sign comes from scipy's splev and the pose in x, _depth).
Those handles get every camera-side unknown frozen and position priors along the spline (the tiny edge problems of the fixture determine
nothing else), which leaves e what it is.

Measured on an MI355X, worst / bar: c1_pinhole_2cam 2.0e-9 / 4.5e-8, rs_F_2int_3cam 1.2e-12 / 1.5e-9, dist_fixed_2cam
2.0e-11 / 1.1e-9, calib_KE_wellposed_5cam 6.1e-10 / 1e-5 (8 x numpy through the split would be 1.1e-3: held at 1e-5), rs_F_2int_3cam with
huber(1.5) and an extra ba_freeze 7.3e-13 / 1.0e-10, a fully frozen camera 2.1e-15 (bar 1e-12), 20 cameras 5.8e-11 / 5.3e-8, wide band (W = 7)
1.1e-11 / 1.1e-9, N = 46 3.6e-11 / 5.4e-9, with a one-detection camera 1.6e-10 / 3.2e-8; t2 worst relative / bar 2.0e-10 / 1.8e-7, 4.8e-14 /
2.3e-9, 9.4e-13 / 2.0e-9, 5.2e-11 / 1.6e-5 (leverage 0.745, 0.337, 0.460, 0.359); trace 240.000000002 and 116.000000000; 2964 signs agree."""
import dataclasses
import functools

import numpy as np
import pytest

from golden_util import load_case
from frozen_util import ba_kwargs, build_scene
from test_covariance_host import bar_for, refined_inverse      # noqa: F401 (bar_for: the chain's own bar, printed beside ours)
from test_gpu_covariance import _synth_case, dense_h, internal_index
from mvus_amd import _lib
from mvus_amd import problem as mp

pytestmark = pytest.mark.gpu

LD = np.longdouble
CASES = ['c1_pinhole_2cam', 'rs_F_2int_3cam', 'dist_fixed_2cam', 'calib_KE_wellposed_5cam']
HARD_BAR = 1e-5                   # the bar of test_gpu_covariance.test_against_an_independent_jacobian: no case may need more


def bar_of(loss):
    """8 x the loss of numpy's fp64 inverse through the split, floor 1e-12, and never above 1e-5: where numpy's own inverse loses more than
    that through the cancelling split (calib_KE_wellposed_5cam: 8 x 1.4e-4) the bar stays at 1e-5."""
    return min(max(8.0 * loss, 1e-12), HARD_BAR)


def _det_cols(prob, c, p, spl_idx):
    """x indices of the B camera slots of camera c and of the twelve coordinates of control points p .. p + 3, in slot order."""
    C, P = prob.C, prob.P
    return np.array([c, C + c, 2 * C + c] + list(range(3 * C + c * P, 3 * C + (c + 1) * P)) + [int(v) for v in spl_idx[3 * p:3 * p + 12]])


def reference(prob, h, x, mask, sigma2):
    """(P_ref [3, M] row frame in long double, loss of numpy's fp64 inverse through the split, n_est, ctrl) for the handle's H at x."""
    _, J, ctrl = h.residual_jacobian(x, _lib.JAC_ANALYTIC)
    H = dense_h(prob, h.normal_equations())
    n, CB, B = H.shape[0], prob.C * (3 + prob.P), 3 + prob.P
    frozen = np.zeros(n, dtype=bool)
    if mask is not None:
        frozen[:CB] = mask
    est = ~frozen & (np.diag(H) != 0)
    idx = np.nonzero(est)[0]
    ref, X0 = refined_inverse(H[np.ix_(idx, idx)])
    full = np.zeros((n, n), dtype=LD)
    full[np.ix_(idx, idx)] = ref
    full64 = np.zeros((n, n))
    full64[np.ix_(idx, idx)] = X0
    _, spl_idx = internal_index(prob)
    cam_of = np.repeat(np.arange(prob.C), np.diff(prob.det_offsets))
    M = ctrl.size
    Pref = np.full((3, M), np.nan, dtype=LD)
    loss = 0.0
    vis = np.nonzero(ctrl >= 0)[0]
    for lo in range(0, vis.size, 2048):                # (batches: the gathered 30 x 30 long-double blocks of 2048 detections are 30 MB)
        ii = vis[lo:lo + 2048]
        cols = np.stack([_det_cols(prob, int(cam_of[i]), int(ctrl[i]), spl_idx) for i in ii])
        Ji = np.transpose(J[:, :, ii], (2, 0, 1)).copy()                     # [n, 2, NS]
        Ji[np.broadcast_to(~est[cols][:, None, :], Ji.shape)] = 0.0           # frozen (and unestimated) columns: Sigma is zero there
        S = full[cols[:, :, None], cols[:, None, :]]
        Jl = Ji.astype(LD)
        Pi = sigma2 * np.einsum('nak,nkl,nbl->nab', Jl, S, Jl)
        Pref[:, ii] = Pi[:, 0, 0], Pi[:, 0, 1], Pi[:, 1, 1]
        S64 = full64[cols[:, :, None], cols[:, None, :]]
        a, b = Ji[:, :, :B], Ji[:, :, B:]
        cross = np.einsum('nak,nkl,nbl->nab', a, S64[:, :B, B:], b)           # (Sigma_cs = -T^T: the minus sign of the split)
        Pn = sigma2 * ((np.einsum('nak,nkl,nbl->nab', a, S64[:, :B, :B], a) + (cross + np.transpose(cross, (0, 2, 1))))
                       + np.einsum('nak,nkl,nbl->nab', b, S64[:, B:, B:], b))
        scale = np.sqrt(Pi[:, 0, 0] * Pi[:, 1, 1])
        err = np.abs(np.stack((Pn[:, 0, 0], Pn[:, 0, 1], Pn[:, 1, 1])).astype(LD) - Pref[:, ii]) / scale
        loss = max(loss, float(np.max(err)))
    return Pref, loss, idx.size, ctrl


def compare(dc, Pref, loss, label):
    """worst |P - P_ref| / sqrt(P_ref,uu P_ref,vv) with P_ref turned into image axes by the signs of e; returns (worst, bar)."""
    vis = ~np.isnan(Pref[0].astype(np.float64))
    su = np.where(dc.e[0] < 0, -1.0, 1.0) * np.where(dc.e[1] < 0, -1.0, 1.0)
    want = Pref.copy()
    want[1] = want[1] * su
    scale = np.sqrt(want[0, vis] * want[2, vis])
    worst = float(np.max(np.abs(dc.cov[:, vis].astype(LD) - want[:, vis]) / scale))
    bar = bar_of(loss)
    print('detection covariance %s: %d detections (%d without a span), worst %.3e, bar %.3e (8 x numpy through the split: %.3e)'
          % (label, vis.size, int((~vis).sum()), worst, bar, 8.0 * loss))
    return worst, bar


def t2_reference(dc, Pref, sigma2):
    """(t2_ref [M] long double, largest per-axis leverage) from the row-frame reference"""
    r = np.abs(dc.e).astype(LD)
    q11, q12, q22 = sigma2 - Pref[0], -Pref[1], sigma2 - Pref[2]
    det = q11 * q22 - q12 * q12
    t2 = (r[0] * r[0] * q22 - 2 * r[0] * r[1] * q12 + r[1] * r[1] * q11) / det
    vis = ~np.isnan(Pref[0].astype(np.float64))
    lev = float(max(np.max(Pref[0, vis]), np.max(Pref[2, vis])) / sigma2)
    return t2, lev


@functools.lru_cache(maxsize=None)
def _case(name):
    scene, g = load_case(name)
    prob, _ = mp.problem_from_scene(scene)
    mask = build_scene(scene, ba_gauge='anchor').ba_frozen_mask(range(scene.num_cam))
    return scene, g, prob, mask


@functools.lru_cache(maxsize=None)
def _solved(name):
    """One handle per golden case at g['x0'] under the anchored gauge: the call's namespace, what covariance() gives, the dense reference."""
    from mvus_amd.ba import BAHandle
    scene, g, prob, mask = _case(name)
    x0 = np.array(g['x0'])
    with BAHandle(prob) as h:
        h.set_frozen(mask)
        before = h.covariance(x0)
        dc = h.detection_covariance(x0)
        again = h.detection_covariance(x0)
        after = h.covariance(x0)
        f = h.residual(x0)
        ms = h.detection_covariance_ms()
        Pref, loss, n_est, ctrl = reference(prob, h, x0, mask, dc.sigma2)
    return dict(prob=prob, x0=x0, dc=dc, again=again, before=before, after=after, f=f, ms=ms, Pref=Pref, loss=loss, n_est=n_est, ctrl=ctrl)


@pytest.mark.parametrize('name', CASES)
def test_against_the_dense_inverse(name):
    s = _solved(name)
    worst, bar = compare(s['dc'], s['Pref'], s['loss'], name)
    assert worst <= bar


@pytest.mark.parametrize('name', CASES)
def test_t2_against_long_double(name):
    s = _solved(name)
    dc = s['dc']
    t2, lev = t2_reference(dc, s['Pref'], dc.sigma2)
    vis = s['ctrl'] >= 0
    assert lev < 1.0
    tol = bar_of(s['loss']) / (1.0 - lev)
    err = np.abs(dc.t2[vis].astype(LD) - t2[vis])
    worst = float(np.max(err / np.maximum(t2[vis], np.finfo(np.float64).tiny)))
    print('t2 %s: largest per-axis leverage %.3f, worst relative %.3e, bar %.3e' % (name, lev, worst, tol))
    assert np.all(err <= tol * t2[vis])


@pytest.mark.parametrize('name', CASES)
def test_residuals_and_detections_without_a_span(name):
    s = _solved(name)
    dc, prob, f, ctrl = s['dc'], s['prob'], s['f'], s['ctrl']
    M = prob.M
    assert dc.e.shape == (2, M) and dc.cov.shape == (3, M) and dc.t2.shape == (M,)
    # |e| is the detection rows of f, bit for bit (f: per camera u(M_c) then v(M_c))
    for c in range(prob.C):
        a, b = int(prob.det_offsets[c]), int(prob.det_offsets[c + 1])
        assert np.array_equal(np.abs(dc.e[0, a:b]), f[2 * a:2 * a + (b - a)])
        assert np.array_equal(np.abs(dc.e[1, a:b]), f[2 * a + (b - a):2 * b])
    out = ctrl < 0
    assert out.sum() >= 1, 'the fixture holds no detection without a span'
    if name == 'rs_F_2int_3cam':
        assert out.sum() == 50 and M == 1866
    assert np.isnan(dc.cov[:, out]).all() and np.isnan(dc.t2[out]).all() and not dc.e[:, out].any()
    assert np.isfinite(dc.cov[:, ~out]).all() and np.isfinite(dc.t2[~out]).all() and np.isfinite(dc.e).all()
    assert (dc.cov[0, ~out] > 0).all() and (dc.cov[2, ~out] > 0).all() and (dc.t2[~out] >= 0).all()
    assert s['ms'] >= 0.0


@pytest.mark.parametrize('name', CASES)
def test_superset_of_covariance_and_repeatable(name):
    s = _solved(name)
    dc, again, before, after = s['dc'], s['again'], s['before'], s['after']
    for cv in (before, after, again):
        assert np.array_equal(dc.cam, cv.cam) and np.array_equal(dc.band, cv.band) and np.array_equal(dc.estimated, cv.estimated)
        assert dc.sigma2 == cv.sigma2 and dc.dof == cv.dof
    assert np.array_equal(dc.e, again.e) and np.array_equal(dc.cov, again.cov, equal_nan=True) and np.array_equal(dc.t2, again.t2, equal_nan=True)


@pytest.mark.parametrize('name', ['c1_pinhole_2cam', 'dist_fixed_2cam'])
def test_trace_identity(name):
    """Linear loss, no motion rows, no priors: sum_i tr Pi_i / sigma^2 = tr(J Sigma J^T) / sigma^2 = tr(H^-1 H) = n_est."""
    s = _solved(name)
    dc, prob = s['dc'], s['prob']
    assert prob.n_residuals == 2 * prob.M                       # no motion rows
    vis = s['ctrl'] >= 0
    tr = float(np.sum((dc.cov[0, vis] + dc.cov[2, vis]).astype(LD)) / dc.sigma2)
    tr_ref = float(np.sum(s['Pref'][0, vis] + s['Pref'][2, vis]) / dc.sigma2)
    bar = abs(tr_ref - s['n_est']) + prob.M * bar_of(s['loss'])
    print('trace identity %s: n_est %d, sum %.9f (reference %.9f), bar %.3e' % (name, s['n_est'], tr, tr_ref, bar))
    assert abs(tr - s['n_est']) <= bar


def _depth(p, x, i, c):
    """Xc_z of detection i of camera c at x, fp64 (its sign only is used): the third row of R X(tau) + t."""
    from scipy.interpolate import splev
    from mvus_amd.synth import rodrigues
    C, P = p.C, p.P
    tau = x[c] * (p.frame[i] + x[2 * C + c] * p.v_raw[i] / p.img_height[c]) + x[C + c]
    s = int(np.nonzero((p.interval[0] <= tau) & (tau < p.interval[1]))[0][0])
    n, xoff = int(p.n_coef[s]), int(p.spline_x_offsets[s])
    knots = p.knots[int(p.knot_offsets[s]):int(p.knot_offsets[s + 1])]
    X = np.array([splev(tau, (knots, x[xoff + d * n:xoff + (d + 1) * n], 3)) for d in range(3)], dtype=np.float64)
    v = x[3 * C + c * P:3 * C + (c + 1) * P]
    o = 4 if p.opt_calib else 0
    return float(rodrigues(v[o:o + 3])[2] @ X + v[o + 5])


def test_signs_against_50_digits():
    import mp_fixture as mf
    from mvus_amd.ba import BAHandle
    cases, _ = mf.load()
    checked = skipped = 0
    for name, case in cases.items():
        p = case.prob
        o = 7 if p.opt_calib else 3                                # slot of rvec; t follows
        ts = np.concatenate([np.linspace(p.interval[0, k], p.interval[1, k], 4 * int(p.n_coef[k]) + 2)[1:-1] for k in range(p.S)])
        with BAHandle(p) as h:
            h.set_frozen(np.ones(p.C * (3 + p.P), dtype=bool))
            h.set_position_priors(ts, np.zeros((3, ts.size)), 1.0)
            dc = h.detection_covariance(case.x, sigma2=1.0)
            f = h.residual(case.x)
        for k, i in enumerate(case.rows):
            c = mf.camera_of(p, i)
            a, b = int(p.det_offsets[c]), int(p.det_offsets[c + 1])
            assert abs(dc.e[0, i]) == f[2 * a + (i - a)] and abs(dc.e[1, i]) == f[2 * a + (b - a) + (i - a)]
            if case.ctrl[k] < 0:
                assert dc.e[0, i] == 0 and dc.e[1, i] == 0 and np.isnan(dc.t2[i])
                continue
            for axis, slot in ((0, o + 3), (1, o + 4)):
                ref = float(case.J[k, axis, slot]) * _depth(p, case.x, int(i), c)
                assert ref != 0.0
                if abs(dc.e[axis, i]) < 1.9e-11:                  # below the restatement's own loss: the sign is not defined
                    skipped += 1
                    continue
                assert np.sign(dc.e[axis, i]) == np.sign(ref), (name, int(i), axis, dc.e[axis, i], ref)
                checked += 1
    print('signs against 50 digits: %d checked over %d cases, %d below 1.9e-11 skipped' % (checked, len(cases), skipped))
    assert checked > 100


def test_loss_and_freeze_in_force():
    from mvus_amd.ba import BAHandle
    scene, g, prob, _ = _case('rs_F_2int_3cam')
    s = build_scene(scene, ba_gauge='anchor', ba_freeze={1: ['alpha', 'rs'], 2: ['beta']})
    mask = s.ba_frozen_mask(range(scene.num_cam))
    x0 = np.array(g['x0'])
    with BAHandle(prob) as h:
        h.set_loss('huber', 1.5)
        h.set_frozen(mask)
        dc = h.detection_covariance(x0)
        cv = h.covariance(x0)
        Pref, loss, _, ctrl = reference(prob, h, x0, mask, dc.sigma2)
        worst, bar = compare(dc, Pref, loss, 'rs_F_2int_3cam huber(1.5) + ba_freeze')
        assert worst <= bar
        assert np.array_equal(dc.cam, cv.cam) and np.array_equal(dc.band, cv.band) and dc.sigma2 == cv.sigma2
        # every unknown of one camera frozen: its detections see the trajectory's covariance only, P = b Sigma_ss b^T
        C, P, B = prob.C, prob.P, 3 + prob.P
        full_mask = np.array(mask, dtype=bool)
        full_mask[[1, C + 1, 2 * C + 1] + list(range(3 * C + P, 3 * C + 2 * P))] = True
        h.set_frozen(full_mask)
        dc = h.detection_covariance(x0)
        _, J, ctrl = h.residual_jacobian(x0, _lib.JAC_ANALYTIC)
    a, b = int(prob.det_offsets[1]), int(prob.det_offsets[2])
    worst, n = 0.0, 0
    for i in range(a, b):
        p = int(ctrl[i])
        if p < 0:
            continue
        G = np.zeros((12, 12), dtype=LD)
        for q in range(4):
            for w in range(4 - q):
                G[3 * q:3 * q + 3, 3 * (q + w):3 * (q + w) + 3] = dc.band[p + q, w]
                G[3 * (q + w):3 * (q + w) + 3, 3 * q:3 * q + 3] = dc.band[p + q, w].T
        bs = J[:, B:, i].astype(LD)
        want = bs @ G @ bs.T
        sgn = (-1.0 if dc.e[0, i] < 0 else 1.0) * (-1.0 if dc.e[1, i] < 0 else 1.0)
        want = np.array([want[0, 0], sgn * want[0, 1], want[1, 1]])
        worst = max(worst, float(np.max(np.abs(dc.cov[:, i] - want)) / np.sqrt(want[0] * want[2])))
        n += 1
    print('fully frozen camera: P = b Sigma_ss b^T over %d detections, worst %.3e (bar 1e-12)' % (n, worst))
    assert n > 100 and worst <= 1e-12                    # (one term, no cancellation: the order of a 12 x 12 form)


def test_sigma2_scales_exactly():
    from mvus_amd.ba import BAHandle
    scene, g, prob, mask = _case('dist_fixed_2cam')
    x0 = np.array(g['x0'])
    with BAHandle(prob) as h:
        h.set_frozen(mask)
        one = h.detection_covariance(x0, sigma2=1.0)
        four = h.detection_covariance(x0, sigma2=4.0)
        post = h.detection_covariance(x0)
    assert one.sigma2 == 1.0 and four.sigma2 == 4.0
    assert np.array_equal(four.cov, 4.0 * one.cov, equal_nan=True)          # (a power of two: exactly linear)
    assert np.array_equal(four.t2, 0.25 * one.t2, equal_nan=True) and np.array_equal(four.e, one.e)
    vis = ~np.isnan(one.t2)
    assert np.max(np.abs(post.cov[:, vis] - post.sigma2 * one.cov[:, vis]) / np.abs(post.cov[:, vis])) <= 1e-14
    assert np.max(np.abs(post.t2[vis] * post.sigma2 - one.t2[vis]) / one.t2[vis]) <= 1e-13


def _with_a_single_detection_camera(prob, mask):
    """The problem with all but one detection of its last camera removed, and every unknown of that camera frozen."""
    C, P = prob.C, prob.P
    off = np.asarray(prob.det_offsets, dtype=np.int64)
    keep = np.ones(prob.M, dtype=bool)
    mid = int((off[C - 1] + off[C]) // 2)
    keep[off[C - 1]:off[C]] = False
    keep[mid] = True
    new_off = off.copy()
    new_off[C] = new_off[C - 1] + 1
    small = dataclasses.replace(prob, det_offsets=new_off, frame=prob.frame[keep], u_raw=prob.u_raw[keep], v_raw=prob.v_raw[keep])
    m = np.array(mask, dtype=bool)
    c = C - 1
    m[[c, C + c, 2 * C + c] + list(range(3 * C + c * P, 3 * C + (c + 1) * P))] = True
    return small, m


@pytest.mark.parametrize('kind', ['cams20', 'wide', 'ragged', 'single'])
def test_shapes_where_the_kernels_can_go_wrong(kind):
    from mvus_amd.ba import BAHandle
    prob, x0, mask = _synth_case('ragged' if kind == 'single' else kind)
    if kind == 'single':
        prob, mask = _with_a_single_detection_camera(prob, mask)
    counts = np.diff(prob.det_offsets)
    with BAHandle(prob) as h:
        h.set_frozen(mask)
        dc = h.detection_covariance(x0)
        cv = h.covariance(x0)
        Pref, loss, _, ctrl = reference(prob, h, x0, mask, dc.sigma2)
        W = h.normal_equations()[2].shape[1]
    worst, bar = compare(dc, Pref, loss, '%s (C %d, N %d, W %d, detections per camera %s)' % (kind, prob.C, int(prob.n_coef.sum()), W, counts[:4]))
    assert np.array_equal(dc.cam, cv.cam) and np.array_equal(dc.band, cv.band)
    assert (counts % 256 != 0).any() and (counts > 256).any()          # a camera with several workgroups, the last one partly filled
    if kind == 'cams20':
        assert prob.C * (3 + prob.P) == 180
    if kind == 'wide':
        assert 7 <= W <= 16
    if kind == 'ragged':
        assert int(prob.n_coef.sum()) % 16 != 0
    if kind == 'single':
        assert counts[-1] == 1 and np.isfinite(dc.cov[:, -1]).all() == (ctrl[-1] >= 0)
    assert worst <= bar


def test_no_side_effect_on_later_solves():
    from mvus_amd.ba import BAHandle
    scene, g, prob, mask = _case('rs_F_2int_3cam')
    x0 = np.array(g['x0'])
    lm = dict(solver=_lib.SOLVER_LM_SCHUR, jac_mode=_lib.JAC_ANALYTIC, max_nfev=4)
    with BAHandle(prob) as h:
        h.set_frozen(mask)
        a1 = h.solve(x0, **lm)
        h.detection_covariance(a1.x)
        h.detection_covariance(a1.x)
        a2 = h.solve(a1.x, **lm)
    with BAHandle(prob) as h:
        h.set_frozen(mask)
        b1 = h.solve(x0, **lm)
        b2 = h.solve(b1.x, **lm)
    assert np.array_equal(a1.x, b1.x)
    assert np.array_equal(a2.x, b2.x) and a2.cost == b2.cost and (a2.nfev, a2.status) == (b2.nfev, b2.status)


def test_refusals():
    from mvus_amd.ba import BAHandle, UnsupportedBySolver
    scene, g, prob, _ = _case('calib_KE_wellposed_5cam')
    x0 = np.array(g['x0'])
    with BAHandle(prob) as h:
        with pytest.raises(ValueError):
            h.detection_covariance_ms()                          # before the first call
        with pytest.raises(ValueError, match='gauge') as ei:
            h.detection_covariance(x0)                           # free gauge
        assert 'detection_covariance: the pivot' in str(ei.value)
    N = int(prob.n_coef.sum())
    with BAHandle(prob) as h:
        h.set_time_shard(0, 2, [0, N // 2, N], halo=8)
        with pytest.raises(UnsupportedBySolver, match='sharded') as ei:
            h.detection_covariance(x0)
        assert 'detection_covariance: ' in str(ei.value)


def test_scene_names_the_handle_numbers():
    scene, g, prob, mask = _case('calib_KE_wellposed_5cam')
    s = build_scene(scene, ba_gauge='anchor', ba_solver='lm')
    cams = list(range(scene.num_cam))
    ts = np.linspace(scene.interval[0, 0], scene.interval[1, -1], 7)
    out = s.ba_detection_covariance(cams, **ba_kwargs(s.settings))
    assert s.detection_covariance is out and 'covariance' not in vars(s)
    h = s._ba_handle
    x = s._pack(h.prob, cams)
    dc = h.detection_covariance(x)
    assert out['cams'] == cams and out['sigma2'] == dc.sigma2 and out['dof'] == dc.dof
    from mvus_amd.reconstruction.common import ellipse_2x2
    for k in cams:
        a, b = int(h.prob.det_offsets[k]), int(h.prob.det_offsets[k + 1])
        d = out['per_cam'][k]
        assert np.array_equal(d['frame'], h.prob.frame[a:b]) and np.array_equal(d['e'], dc.e[:, a:b])
        assert np.array_equal(d['cov'], dc.cov[:, a:b], equal_nan=True) and np.array_equal(d['t2'], dc.t2[a:b], equal_nan=True)
        major, minor, angle = ellipse_2x2(dc.cov[:, a:b])
        assert np.array_equal(d['semi_major'], major, equal_nan=True) and np.array_equal(d['semi_minor'], minor, equal_nan=True)
        assert np.array_equal(d['angle'], angle, equal_nan=True)
        vis = ~np.isnan(d['t2'])
        assert (d['semi_major'][vis] >= d['semi_minor'][vis]).all() and (d['semi_minor'][vis] >= 0).all()
    flags = s.studentised_flags(out)
    assert sorted(flags) == cams and all(flags[k].shape == out['per_cam'][k]['t2'].shape and flags[k].dtype == bool for k in cams)
    assert not any(flags[k][np.isnan(out['per_cam'][k]['t2'])].any() for k in cams)
    # one call serves both: the covariance it stores is the one ba_covariance gives
    both = s.ba_detection_covariance(cams, with_covariance=True, t=ts, **ba_kwargs(s.settings))
    got = s.covariance
    alone = s.ba_covariance(cams, t=ts, **ba_kwargs(s.settings))
    assert all(np.array_equal(got[key], alone[key], equal_nan=True) for key in ('cam_cov', 'band', 'pos_cov', 'pos_std', 't', 'estimated_cam'))
    assert got['sigma2'] == alone['sigma2'] and got['dof'] == alone['dof'] and got['cam_std'] == alone['cam_std']
    assert np.array_equal(both['per_cam'][0]['cov'], out['per_cam'][0]['cov'], equal_nan=True)
    import pickle
    back = pickle.loads(pickle.dumps(s))
    assert np.array_equal(back.detection_covariance['per_cam'][1]['t2'], out['per_cam'][1]['t2'], equal_nan=True)


@functools.lru_cache(maxsize=None)
def _pipeline(tmp, both):
    """reconstruct_from_config with ba_covariance on and ba_detection_covariance on (both) or off: (the pickled Scene, the timer's rows)."""
    import json
    import pathlib
    import pickle
    from mvus_amd import pipeline, synth
    from test_gpu_init_pipeline import _write_inputs
    d = pathlib.Path(tmp) / ('both' if both else 'cov')
    d.mkdir()
    # (the scene of test_gpu_covariance.test_reconstruct_from_config_carries_the_covariance: three cameras and the motion prior)
    sc = synth.make_scene(3, 4500, seed=31, perturb=0.3, motion_reg=True, motion_type='F', motion_weights=1e2)
    cf = -sc.truth['beta'] / sc.truth['alpha']
    path = _write_inputs(d, sc, cf, True)
    cfg = json.loads(path.read_text())
    cfg['settings'].update(ba_solver='lm', ba_gauge='anchor', ba_covariance=True)
    if both:
        cfg['settings']['ba_detection_covariance'] = True
    path.write_text(json.dumps(cfg))
    flight, timer = pipeline.reconstruct_from_config(str(path))
    with open(flight.settings['path_output'], 'rb') as fh:
        return pickle.load(fh), [r[0] for r in timer.rows], list(flight.sequence)


def test_reconstruct_from_config_carries_the_result(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp('detcov'))
    back, rows, seq = _pipeline(tmp, True)
    alone, rows_alone, _ = _pipeline(tmp, False)
    # the key off: nothing of it in the pickle, no stage
    assert 'detection_covariance' not in vars(alone) and 'ba_detection_covariance' not in rows_alone and 'ba_covariance' in rows_alone
    # the key on: the result per camera of the sequence; one call served both
    assert 'ba_detection_covariance' in rows and 'ba_covariance' not in rows
    dc = back.detection_covariance
    assert dc['cams'] == seq and dc['sigma2'] > 0 and dc['dof'] > 0 and sorted(dc['per_cam']) == sorted(seq)
    for k in seq:
        d = dc['per_cam'][k]
        vis = ~np.isnan(d['t2'])
        assert vis.sum() > 100 and d['e'].shape == (2, vis.size) and d['cov'].shape == (3, vis.size) and d['frame'].shape == vis.shape
        assert (d['semi_major'][vis] > 0).all() and (d['t2'][vis] >= 0).all()
    # and the covariance in the pickle is the one ba_covariance alone gives
    for key in ('cam_cov', 'band', 'pos_cov', 'pos_std', 't'):
        assert np.array_equal(back.covariance[key], alone.covariance[key], equal_nan=True), key
    assert back.covariance['sigma2'] == alone.covariance['sigma2'] and back.covariance['dof'] == alone.covariance['dof']
