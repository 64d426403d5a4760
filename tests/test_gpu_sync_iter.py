"""GPU tests of the iterative time-shift search: synchronization.sync_iter_gpu, "sync_method": "iter_gpu" and the hooks
sync_iter_models / sync_iter_score against the numpy / scipy restatement (tests/sync_iter_oracle.py).  Inputs, recorded figures and
bounds: tests/sync_iter_cases.py; where the bounds come from: tests/test_sync_iter_host.py."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import sync_iter_cases as cases                            # noqa: E402
import sync_iter_oracle as so                              # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def session():
    from mvus_amd.reconstruction import synchronization as sy
    p = cases.prep()
    with sy.SyncIterSession(p['d1'], cases.pair()[3]) as S:
        yield S


@pytest.fixture(scope='module')
def device_models(session):
    """sync_iter_models at the oracle's indices, once per step: d -> (betas, valid, F, counts)."""
    from mvus_amd.reconstruction import synchronization as sy
    p = cases.prep()
    return {d: sy.sync_iter_models(session, p['beta_prior'], d, cases.indices(d), cases.THRESHOLD) for d in cases.STEPS}


@pytest.mark.parametrize('d', cases.STEPS)
def test_beta(device_models, d):
    """Test 4: on settled hypotheses the same number of slots, and |beta_gpu - beta_ref| <= c eps kappa."""
    betas, valid, _, _ = device_models[d]
    worst = 0.0
    for h, ref in enumerate(cases.reference(d)):
        n = int(valid[h].sum())
        assert valid[h, :n].all() and not valid[h, n:].any()                   # the valid slots come first
        assert np.all(np.diff(betas[h, :n]) >= 0.0)                            # ascending
        if not ref['settled']:
            continue
        assert n == len(ref['betas']), 'hypothesis %d: %d slots, scipy has %d' % (h, n, len(ref['betas']))
        if n:
            worst = max(worst, float(np.max(np.abs(betas[h, :n] - ref['betas']) / (so.EPS * ref['kappa']))))
    print('d = %d: worst |beta_gpu - beta_scipy| = %.3g eps kappa (bound c = %.3g)' % (d, worst, cases.C_BETA))
    assert worst <= cases.C_BETA


@pytest.mark.parametrize('d', cases.STEPS)
def test_fundamental_matrix(device_models, d):
    """Test 5: with the device's own beta, F (unit norm, F[2, 2] >= 0) against the oracle's 8-point fit at that beta."""
    betas, valid, F, _ = device_models[d]
    worst = 0.0
    for h, ref in enumerate(cases.reference(d)):
        s1, s2, ds = ref['samples']
        for k in np.nonzero(valid[h])[0]:
            assert abs(np.linalg.norm(F[h, k]) - 1.0) <= 1e-12 and F[h, k, 2, 2] >= 0.0
            worst = max(worst, float(np.max(np.abs(F[h, k] - so.fit_F(s1, s2 + betas[h, k] * ds)))))
        assert not F[h][~valid[h]].any()                                       # an empty slot is zeros, never NaN
    print('d = %d: worst |F_gpu - F_oracle| = %.3g (bound %.3g)' % (d, worst, cases.F_BAR))
    assert worst <= cases.F_BAR


@pytest.mark.parametrize('d', cases.STEPS)
def test_score(session, device_models, d):
    """Test 6: sync_iter_score on the device's own models against the oracle's scorer; overlap 0 is reported as such."""
    from mvus_amd.reconstruction import synchronization as sy
    p = cases.prep()
    betas, valid, F, counts = device_models[d]
    Fs, ms = F[valid], betas[valid] * d
    far = np.array([1e6, -1e6, 5000.0])                                        # models moved off camera 2's track: no overlap
    got = sy.sync_iter_score(session, p['beta_prior'], np.concatenate((Fs, Fs[:3])), np.concatenate((ms, far)), cases.THRESHOLD)
    np.testing.assert_array_equal(got[:len(ms)], counts[valid])                # the hook's counts are the scorer's
    np.testing.assert_array_equal(got[len(ms):], np.zeros((3, 2), dtype=np.int32))
    checked = 0
    for k in range(len(ms)):
        if so.settled_model(p, p['beta_prior'], Fs[k], ms[k], cases.THRESHOLD):
            assert tuple(got[k]) == so.score(p, p['beta_prior'], Fs[k], ms[k], cases.THRESHOLD), 'model %d' % k
            checked += 1
    assert checked >= 0.95 * len(ms)


def test_samples_before_the_first_knot(session):
    """Test 7a: d < 0 and samples among camera 2's first detections: S2(t + d) lies before the first knot and must be splev's extension."""
    from mvus_amd.reconstruction import synchronization as sy
    p = cases.prep()
    d, idx = -4, cases.early_indices(-4)
    assert np.all(p['t2'][idx[:, 0]] + d < p['tck2'][0][0])
    betas, valid, F, counts = sy.sync_iter_models(session, p['beta_prior'], d, idx, cases.THRESHOLD)
    rng = np.random.default_rng(5)
    for h in range(len(idx)):
        s1, s2, ds = so.samples(p, p['beta_prior'], d, idx[h])
        A1, A2 = so.pencil(s1, s2, ds)
        if not so.settled_hypothesis(A1, A2, rng):
            continue
        ref = so.pencil_betas(A1, A2)
        n = int(valid[h].sum())
        assert n == len(ref)
        if n:
            assert np.all(np.abs(betas[h, :n] - ref) <= cases.C_BETA * so.EPS * so.kappa(A1, A2, ref))


def test_gap_and_short_interval():
    """Test 7b: camera 2 with two intervals 40 frames apart and a run shorter than 5 frames that must not count; model shifts that
    move samples across the hole."""
    from mvus_amd.reconstruction import synchronization as sy
    d2g, p = cases.gap_case()
    shift = p['beta_prior']
    with sy.SyncIterSession(p['d1'], d2g) as S:
        np.testing.assert_array_equal(S.intervals, p['intervals'])
        n = p['n'] - 2
        idx = np.array([so.sample9(cases.SEED, 0, 0, h, n) for h in range(8)], dtype=np.int64)
        betas, valid, F, _ = sy.sync_iter_models(S, shift, 1, idx, cases.THRESHOLD)
        Fs = F[valid][:6]
        assert len(Fs) == 6
        moves = np.array([0.0, 15.5, -23.25, 39.75, -700.25, 1500.5])
        got = sy.sync_iter_score(S, shift, Fs, moves, cases.THRESHOLD)
        overlaps = set()
        for k in range(6):
            assert so.settled_model(p, shift, Fs[k], moves[k], cases.THRESHOLD)
            assert tuple(got[k]) == so.score(p, shift, Fs[k], moves[k], cases.THRESHOLD)
            overlaps.add(int(got[k, 1]))
        assert len(overlaps) >= 4                                              # the hole moved across the samples
        # the short run counts nowhere: camera 1's first samples land on it, all later ones beyond camera 2's last detection
        only_short = (d2g[0, -3] + 0.25) - (p['d1'][0, 0] - shift)
        tau = p['d1'][0] - shift + only_short
        assert np.sum((tau >= d2g[0, -3]) & (tau < d2g[0, -1])) >= 1 and tau[0] > p['intervals'][1, 1]
        lone = sy.sync_iter_score(S, shift, Fs[:1], np.array([only_short]), cases.THRESHOLD)
        assert tuple(lone[0]) == (0, 0) == so.score(p, shift, Fs[0], only_short, cases.THRESHOLD)


def test_bad_samples_give_no_model_and_leave_the_others(session, device_models):
    """Test 7c: a repeated timestamp and a non-finite one among camera 2's timestamps: zero models for the hypotheses that draw them,
    the same bits as before for the others."""
    from mvus_amd.reconstruction import synchronization as sy
    p = cases.prep()
    d = 1
    idx = cases.indices(d).copy()
    t2 = p['t2'].copy()
    a, b, c = int(idx[0, 0]), int(idx[0, 1]), int(idx[1, 0])
    t2[b] = t2[a]                                                              # hypothesis 0 draws a repeated timestamp
    t2[c] = np.nan                                                             # hypothesis 1 a non-finite one
    touched = np.array([bool({a, b, c} & set(row.tolist())) for row in idx])
    assert touched[0] and touched[1] and (~touched).sum() >= 30
    with sy.SyncIterSession(p['d1'], cases.pair()[3], t2=t2) as S:
        betas, valid, F, counts = sy.sync_iter_models(S, p['beta_prior'], d, idx, cases.THRESHOLD)
    assert not valid[0].any() and not valid[1].any()
    assert not betas[:2].any() and not F[:2].any() and not counts[:2].any()
    assert np.isfinite(betas).all() and np.isfinite(F).all()
    b0, v0, F0, c0 = device_models[d]
    keep = ~touched
    np.testing.assert_array_equal(valid[keep], v0[keep])
    np.testing.assert_array_equal(betas[keep], b0[keep])
    np.testing.assert_array_equal(F[keep], F0[keep])
    np.testing.assert_array_equal(counts[keep], c0[keep])


def test_too_few_samples_is_an_error(session):
    """Test 7d: min(N1, N2) - 2 |d| < 9: an error, nothing is launched."""
    from mvus_amd.reconstruction import synchronization as sy
    p = cases.prep()
    d = (p['n'] - 8) // 2 + 1
    assert p['n'] - 2 * d < 9
    with pytest.raises(ValueError, match='fewer than nine'):
        sy._round(session, p['beta_prior'], d, cases.H, cases.THRESHOLD, cases.SEED, 0)
    with pytest.raises(ValueError, match='outside'):
        sy.sync_iter_models(session, p['beta_prior'], 1, np.full((1, 9), p['t2'].size, dtype=np.int64), cases.THRESHOLD)
    # the session still works
    out = sy._round(session, p['beta_prior'], 1, cases.H, cases.THRESHOLD, cases.SEED, 0)
    assert out[0][3] > 0


def _time_shift_scene(moved):
    from mvus_amd.reconstruction import common
    a = cases.pair(moved)
    sc = a[7]
    s = common.Scene()
    s.numCam = 2
    s.settings = dict(sc.settings)
    for c in sc.truth['cameras']:
        s.addCamera(common.Camera(K=c['K'].copy(), d=c['d'].copy(), fps=c['fps'], resolution=list(c['resolution'])))
    for det in sc.detections:
        s.addDetection(det.copy())
    s.ref_cam = 0
    s.cf = np.array([a[4], a[5]])
    s.settings.update(cf_exact=False, sync_method='iter_gpu', sync_iter={'maxIter': cases.H})
    s.init_alpha()
    return s, a[6]


@pytest.mark.parametrize('moved', cases.MOVES)
def test_time_shift_end_to_end(moved):
    """Test 8: Scene.time_shift with "sync_method": "iter_gpu": beta within twice the oracle's recorded error, never above one frame."""
    s, truth = _time_shift_scene(moved)
    s.time_shift()
    err = float(s.beta[1]) - truth
    print('moved %+g frames: beta %.6f, truth %.6f, error %+.4f frames (oracle %+.4f, bar %.4f)'
          % (moved, s.beta[1], truth, err, cases.ORACLE_BETA_ERROR[moved], cases.beta_bar(moved)))
    assert s.beta[0] == 0.0
    assert abs(err) <= cases.beta_bar(moved)
    np.testing.assert_array_equal(s.beta_after_Fbeta, s.beta)


def test_unknown_method_names_all_three():
    s, _ = _time_shift_scene(20.0)
    s.settings['sync_method'] = 'nope'
    with pytest.raises(ValueError, match='"iter", "bf" or "iter_gpu"'):
        s.time_shift()
    s.settings.update(sync_method='iter_gpu', sync_iter={'maxiter': 5})
    with pytest.raises(ValueError, match='maxiter'):
        s.time_shift()


def test_determinism(session):
    """Test 9: the same bits from two calls; the round at H = 50 is the first 50 hypotheses of H = 200."""
    from mvus_amd.reconstruction import synchronization as sy
    a = cases.pair()
    r1 = sy.sync_iter_gpu(*a[:6], maxIter=cases.H, seed=cases.SEED)
    r2 = sy.sync_iter_gpu(*a[:6], maxIter=cases.H, seed=cases.SEED)
    assert float(r1[0]).hex() == float(r2[0]).hex() and float(r1[1]).hex() == float(r2[1]).hex()
    p = cases.prep()
    shift, d = p['beta_prior'], 2
    small = sy._round(session, shift, d, 50, cases.THRESHOLD, cases.SEED, 3)
    large = sy._round(session, shift, d, 200, cases.THRESHOLD, cases.SEED, 3)
    assert small == sy._round(session, shift, d, 50, cases.THRESHOLD, cases.SEED, 3)
    n = p['n'] - 2 * d
    for sign, dd in ((0, d), (1, -d)):
        idx = np.array([so.sample9(cases.SEED, 3, sign, h, n) for h in range(200)], dtype=np.int64)
        betas, valid, _, counts = sy.sync_iter_models(session, shift, dd, idx, cases.THRESHOLD)
        for H, got in ((50, small[sign]), (200, large[sign])):
            best = (0.0, 0.0, 0, 0)
            for h in range(H):
                for k in range(6):
                    if valid[h, k] and counts[h, k, 1] > 0 and counts[h, k, 0] / counts[h, k, 1] > best[1]:
                        best = (-(betas[h, k] * dd), counts[h, k, 0] / counts[h, k, 1], int(counts[h, k, 0]), int(counts[h, k, 1]))
            assert got == best, (sign, H)
