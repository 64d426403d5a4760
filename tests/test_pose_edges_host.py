"""The premises of tests/test_gpu_pose_edges.py, proved without a GPU on the references (tests/pose_edge_cases.py) and the host
build of the device math (tests/hostcheck): every bar and every cap the GPU tests rely on is checked here first.

* triangulation: the host build of triangulate_pair lies within the bar that the LAPACK route's own deviation from the 50-digit
  SVD sets, at every geometry and size; the optional error outputs do not change a bit of the others; one degenerate lane
  changes no other lane and does not hang;
* PnP: the builder keeps every pixel inside the image and every depth > 1; over all hypotheses of all cases no point lies on the
  threshold; the winner's mask is the ground-truth labelling and holds every heavy point; po.refine repeats from another start
  far below the pose bars, and dropping any single heavy point moves it by at least 100 x those bars -- so a point lost or counted
  twice at a workgroup edge cannot hide behind them;
* least squares on fixed knots: an fp64 solve of the normal equations stays within the bar (the floor governs, with cond(B) <= 10)
  on every knot vector and size, and the ill-conditioned case has the condition number it was built for."""
import numpy as np
import pytest

import pose_edge_cases as pe
from mvus_amd import _lib


# ---- triangulation -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('geometry,N', pe.TRI_CASES)
def test_host_triangulation_within_the_bar_of_the_lapack_route(geometry, N):
    from hostcheck_util import host_triangulate
    p = pe.tri_problem(geometry, N)
    X, e1, e2 = host_triangulate(p['x1'], p['x2'], p['P1'], p['P2'])
    pe.tri_check('host %s N=%d' % (geometry, N), p, X, e1, e2)


def test_host_triangulation_optional_outputs_and_a_degenerate_lane():
    from hostcheck_util import host_triangulate, load
    lib = load()
    p = pe.tri_problem('base1e-4-noisy', 257)
    N = 257
    outs = []
    for want1, want2 in ((True, True), (True, False), (False, True), (False, False)):
        X, e1, e2 = np.zeros((4, N)), np.full(N, -1.0), np.full(N, -1.0)
        lib.hostcheck_triangulate(N, _lib.dptr(p['x1']), _lib.dptr(p['x2']), _lib.dptr(p['P1']), _lib.dptr(p['P2']), _lib.dptr(X),
                                  _lib.dptr(e1) if want1 else None, _lib.dptr(e2) if want2 else None)
        outs.append((X, e1 if want1 else None, e2 if want2 else None))
        assert want1 or np.all(e1 == -1.0)
        assert want2 or np.all(e2 == -1.0)
    for X, e1, e2 in outs[1:]:
        np.testing.assert_array_equal(X, outs[0][0])
        assert e1 is None or np.array_equal(e1, outs[0][1])
        assert e2 is None or np.array_equal(e2, outs[0][2])
    p = pe.tri_problem('wide', 513)
    clean = host_triangulate(p['x1'], p['x2'], p['P1'], p['P2'])
    x1, x2 = pe.tri_with_degenerate_lane(p, 255)
    dirty = host_triangulate(x1, x2, p['P1'], p['P2'])
    keep = np.arange(513) != 255
    for a, b in zip(clean, dirty):
        np.testing.assert_array_equal(a[..., keep], b[..., keep])
    # the same pixel in two identical cameras, every lane: returns (the sweep loop is bounded), whatever the values
    assert host_triangulate(p['x1'], p['x1'], p['P1'], p['P1'])[0].shape == (4, 513)


# ---- PnP -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', range(len(pe.PNP_CASES)))
def test_pnp_builder_keeps_the_camera_on_the_points(k):
    p = pe.pnp_problem(k)
    N, H, noise, outliers, behind, _dist = pe.PNP_CASES[k]
    front = np.ones(N, dtype=bool)
    front[p['behind']] = False
    uv = p['clean_uv']
    assert uv.shape == (2, N) and p['behind'].size == behind
    assert uv[0].min() > 0 and uv[0].max() < pe.WIDTH and uv[1].min() > 0 and uv[1].max() < pe.HEIGHT
    assert p['depth'].min() > 1.0
    good = ~p['bad']
    assert np.all(np.linalg.norm((p['uv'] - uv)[:, good], axis=0) < 6 * noise + 4.3)
    gross = p['bad'] & front
    assert gross.sum() == 0 or np.linalg.norm((p['uv'] - uv)[:, gross], axis=0).min() >= 30.0
    assert outliers == 0 or gross.sum() > 0
    # the moved points really are behind the true camera, 20 units or so
    zc = (p['R'] @ p['X'] + p['t'].reshape(3, 1))[2]
    assert np.all(zc[p['behind']] < -10.0) and np.all(zc[front] > 1.0)
    want = [i for i in sorted({0, 255, 256, 511, 512, N - 1}) if i < N and good[i]] if N >= pe.HEAVY_FROM else []
    assert p['heavy'].tolist() == want and (N < pe.HEAVY_FROM or {0, N - 1} <= set(want))
    print('N %4d: pixels u %.0f..%.0f v %.0f..%.0f, depth >= %.1f, %d gross, %d behind, heavy %s'
          % (N, uv[0].min(), uv[0].max(), uv[1].min(), uv[1].max(), p['depth'].min(), int(gross.sum()), behind, want))


@pytest.mark.parametrize('k', range(len(pe.PNP_CASES)))
def test_pnp_restatement_has_no_boundary_point_and_finds_the_labelling(k):
    p, r = pe.pnp_problem(k), pe.pnp_restatement(k)
    N, H = p['N'], p['H']
    c = r['counts']
    print('N %4d H %3d: %d valid hypotheses, winner %d with %d of %d good points, runner-up %d, boundary points over all hypotheses %d'
          % (N, H, r['valid'], r['best'], c[r['best']], int((~p['bad']).sum()), np.sort(c)[-2] if H > 1 else -1, int(r['near'].sum())))
    assert int(r['near'].sum()) == 0
    assert c[r['best']] >= 6 and c[r['best']] == int(r['mask'].sum())
    np.testing.assert_array_equal(r['mask'], ~p['bad'])
    assert r['mask'][p['heavy']].all() and not r['mask'][p['behind']].any()
    if N == 6:
        assert c[0] == 6


@pytest.mark.parametrize('k', [k for k, c in enumerate(pe.PNP_CASES) if c[0] > 6])
def test_pnp_bars_notice_a_single_heavy_point(k):
    p = pe.pnp_problem(k)
    mask = ~p['bad']
    R, t = pe.pnp_refine(p, mask)
    R2, t2 = pe.pnp_refine(p, mask, start=(pe.po.rodrigues(np.array([0.01, -0.01, 0.005])) @ p['R'], p['t'] + 0.05))
    rep_a, rep_t = pe.angle_deg(R, R2), np.linalg.norm(t - t2) / np.linalg.norm(t)
    shifts = []
    for i in p['heavy']:
        m = mask.copy()
        m[i] = False
        Rd, td = pe.pnp_refine(p, m)
        shifts.append((pe.angle_deg(R, Rd), np.linalg.norm(t - td) / np.linalg.norm(t)))
    sa, st = min([a for a, _ in shifts] or [np.nan]), min([b for _, b in shifts] or [np.nan])
    print('N %4d: po.refine from another start repeats to %.2e deg, %.2e in t; dropping one heavy point moves it by >= %.2e deg (bar %.0e), >= %.2e in t (bar %.0e)'
          % (p['N'], rep_a, rep_t, sa, pe.PNP_ANGLE_BAR, st, pe.PNP_T_BAR))
    assert rep_a <= 0.5 * pe.PNP_ANGLE_BAR and rep_t <= 0.5 * pe.PNP_T_BAR          # the reference resolves the bars it is used for
    if p['N'] >= pe.HEAVY_FROM:
        assert p['heavy'].size >= 2 and sa >= 100 * pe.PNP_ANGLE_BAR and st >= 100 * pe.PNP_T_BAR


def test_pnp_sampler_terminates_at_six_points():
    """N = 6: every hypothesis draws the same six points, in some order"""
    from hostcheck_util import load
    lib = load()
    for h in range(200):
        idx = np.full(6, -1, dtype=np.int64)
        lib.hostcheck_pnp_sample6(pe.PNP_SEED, h, 6, idx.ctypes.data_as(_lib.c_int64_p))
        assert sorted(idx.tolist()) == [0, 1, 2, 3, 4, 5]


# ---- least squares on fixed knots --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', pe.LSQ_KNOTS)
def test_lsq_fp64_normal_equations_within_the_bar(name):
    from scipy import interpolate
    for m in (0,) + pe.LSQ_SIZES:
        p = pe.lsq_problem(name, m)
        knots, t = p['knots'], p['t']
        n = knots.size - 4
        assert t.size == (m or n)
        if m:
            assert set(np.unique(knots)) <= set(t.tolist())                   # every distinct knot is a data site, both ends included
            assert np.all(np.histogram(t, np.unique(knots))[0] >= 3)
        qr = pe.lsq_deviation(interpolate.make_lsq_spline(np.sort(t), p['X'][:, np.argsort(t)].T, knots, k=3).c.T, p['ref'])
        print('%-8s n %2d m %4d: cond(B) %.1f, fp64 normal equations %.2e, make_lsq_spline %.2e, bar %.1e' % (name, n, t.size, p['cond'], p['fp64'], qr, p['bar']))
        assert p['cond'] <= 10.0
        assert pe.LSQ_BAR_FACTOR * p['fp64'] <= pe.LSQ_FLOOR and p['bar'] == pe.LSQ_FLOOR      # the floor governs
        assert qr <= p['bar']


def test_lsq_ill_conditioned_case_is_what_it_claims():
    p = pe.lsq_ill_conditioned()
    t, knots = p['t'], p['knots']
    assert int((t > 0.4).sum()) == 1 and t.size == 64
    print('ill-conditioned: cond(B) %.2e, fp64 normal equations %.2e, bar %.2e, max |c_ref| %.3e' % (p['cond'], p['fp64'], p['bar'], np.abs(p['ref']).max()))
    assert 1e5 <= p['cond'] <= 1e7
    assert p['bar'] == max(pe.LSQ_BAR_FACTOR * p['fp64'], pe.LSQ_FLOOR)


def test_lsq_reference_span_rule_matches_the_device():
    """lsq_span (the reference's span search) against find_span's rule on knots, ends and a double knot"""
    knots = pe.lsq_knots('double')
    assert [pe.lsq_span(knots, x) for x in (0.0, 0.1, 0.2, 0.5, 0.79, 0.8, 1.0)] == [3, 3, 4, 6, 6, 7, 7]
