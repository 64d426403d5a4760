"""The three device paths that hand the BA its starting point, at their workgroup edges and hard geometries
(tests/pose_edge_cases.py has the builders and references, tests/test_pose_edges_host.py proves the premises on the CPU):

* k_triangulate against a 50-digit SVD at N = 1, 255, 256, 257, 513 on a wide and two short baselines, a scaled projection matrix
  and far points; the bar is 8 x the LAPACK route's own deviation from that reference (floors 1e-12, 1e-10 px).  The optional error
  outputs one at a time, and one degenerate lane among 513.
* mvus_pnp_ransac against the restatement of its RANSAC stage from the host build of its device functions (count and mask equal,
  no boundary point), against the ground-truth labelling, and its refined pose against po.refine on the returned mask at the
  bars of tests/test_pnp.py -- which a single heavy point at index 0, 255, 256, 511, 512 or N - 1 overshoots a hundredfold.
* mvus_spline_lsq against normal equations built and solved at 50 digits: n = 4, 5, knot spacings in ratio 1e3, a double knot,
  n = 40; m = n, 255, 256, 257, 2049; one ill-conditioned case; the Schoenberg-Whitney refusals and the closed right end.

Measured on the MI355X (each test prints its own worst case beside its bar): see DESIGN.md, "Pose, triangulation and fixed-knot
fit at their edges"."""
import ctypes

import numpy as np
import pytest

import pose_edge_cases as pe
from mvus_amd import _lib


# ---- triangulation -------------------------------------------------------------------------------------------------------------
def _triangulate(p, x1, x2, want1=True, want2=True):
    """mvus_triangulate through ctypes: (X, err1 or None, err2 or None); an error array that was not asked for is not passed"""
    lib = _lib.load()
    N = x1.shape[1]
    X, e1, e2 = np.zeros((4, N)), np.zeros(N), np.zeros(N)
    rc = lib.mvus_triangulate(0, N, _lib.dptr(np.ascontiguousarray(x1)), _lib.dptr(np.ascontiguousarray(x2)), _lib.dptr(p['P1']), _lib.dptr(p['P2']),
                              _lib.dptr(X), _lib.dptr(e1) if want1 else None, _lib.dptr(e2) if want2 else None)
    assert rc == 0, lib.mvus_last_error(None).decode()
    return X, (e1 if want1 else None), (e2 if want2 else None)


@pytest.mark.gpu
@pytest.mark.parametrize('geometry,N', pe.TRI_CASES)
def test_triangulation_against_the_50_digit_svd(geometry, N):
    from mvus_amd.reconstruction import epipolar as ep
    p = pe.tri_problem(geometry, N)
    X, e1, e2 = ep.triangulate_with_errors(p['x1'], p['x2'], p['P1'], p['P2'])
    assert X.shape == (4, N) and e1.shape == (N,) and e2.shape == (N,)
    pe.tri_check('gpu %s N=%d' % (geometry, N), p, X, e1, e2)


@pytest.mark.gpu
def test_triangulation_optional_error_outputs_one_at_a_time():
    p = pe.tri_problem('base1e-4-noisy', 257)
    both = _triangulate(p, p['x1'], p['x2'], True, True)
    pe.tri_check('gpu ctypes base1e-4-noisy N=257', p, *both)
    for want1, want2 in ((True, False), (False, True), (False, False)):
        X, e1, e2 = _triangulate(p, p['x1'], p['x2'], want1, want2)
        np.testing.assert_array_equal(X, both[0])
        assert (e1 is None) == (not want1) and (e2 is None) == (not want2)
        if want1:
            np.testing.assert_array_equal(e1, both[1])
        if want2:
            np.testing.assert_array_equal(e2, both[2])


@pytest.mark.gpu
def test_triangulation_one_degenerate_lane_among_513():
    p = pe.tri_problem('wide', 513)
    clean = _triangulate(p, p['x1'], p['x2'])
    x1, x2 = pe.tri_with_degenerate_lane(p, 255)
    dirty = _triangulate(p, x1, x2)
    keep = np.arange(513) != 255
    for a, b in zip(clean, dirty):
        np.testing.assert_array_equal(a[..., keep], b[..., keep])
    print('degenerate lane 255: X = %s, err = %.3e, %.3e' % (dirty[0][:, 255], dirty[1][255], dirty[2][255]))


# ---- PnP -------------------------------------------------------------------------------------------------------------------------
def _pnp(p):
    lib = _lib.load()
    N = p['N']
    rvec, tvec, mask, n_in = np.zeros(3), np.zeros(3), np.full(N, 7, dtype=np.uint8), ctypes.c_int64(-1)
    rc = lib.mvus_pnp_ransac(0, N, _lib.dptr(p['X']), _lib.dptr(p['uv']), _lib.dptr(pe.KV), _lib.dptr(p['d']), pe.PNP_THRESHOLD, p['H'], pe.PNP_SEED,
                             _lib.dptr(rvec), _lib.dptr(tvec), mask.ctypes.data_as(_lib.c_uint8_p), ctypes.byref(n_in))
    assert rc == 0, lib.mvus_last_error(None).decode()
    return rvec, tvec, mask, int(n_in.value)


@pytest.mark.gpu
@pytest.mark.parametrize('k', range(len(pe.PNP_CASES)))
def test_pnp_ransac_at_the_edges(k):
    p, r = pe.pnp_problem(k), pe.pnp_restatement(k)
    N, H = p['N'], p['H']
    rvec, tvec, mask8, n_in = _pnp(p)
    assert set(np.unique(mask8).tolist()) <= {0, 1}
    mask = mask8.astype(bool)
    boundary = int(r['near'].sum())
    print('N %4d H %3d: n_inliers gpu %d, restated %d (winner %d of %d valid); boundary points over all hypotheses %d'
          % (N, H, n_in, r['counts'][r['best']], r['best'], r['valid'], boundary))
    assert boundary == 0                                                       # so the count and the mask admit no exception
    assert n_in == int(r['counts'][r['best']])
    np.testing.assert_array_equal(mask, r['mask'])
    np.testing.assert_array_equal(mask, ~p['bad'])
    assert mask[p['heavy']].all() and not mask[p['behind']].any() and n_in == int(mask.sum())
    if N == 6:
        assert n_in == 6
    else:
        Rg = pe.po.rodrigues(rvec)
        Ro, to, _cost = pe.po.refine(pe.K, p['d'], Rg, tvec, p['X'][:, mask], p['uv'][:, mask])
        da, dt = pe.angle_deg(Rg, Ro), np.linalg.norm(tvec - to) / np.linalg.norm(to)
        print('       pose against po.refine on the returned mask: %.2e deg (bar %.0e), |t - t_ref| / |t_ref| %.2e (bar %.0e); against the truth %.3f deg'
              % (da, pe.PNP_ANGLE_BAR, dt, pe.PNP_T_BAR, pe.angle_deg(Rg, p['R'])))
        assert da < pe.PNP_ANGLE_BAR and dt <= pe.PNP_T_BAR
    again = _pnp(p)
    assert np.array_equal(again[0], rvec) and np.array_equal(again[1], tvec) and np.array_equal(again[2], mask8) and again[3] == n_in


# ---- least squares on fixed knots --------------------------------------------------------------------------------------------------
def _lsq_check(label, p):
    from mvus_amd import spline
    c = np.array(spline.lsq_fit(p['knots'], p['t'], p['X']))
    dev = pe.lsq_deviation(c, p['ref'])
    print('%s n %2d m %4d: max |c - c_ref| / max |c_ref| %.2e (fp64 normal equations %.2e, cond(B) %.1e, bar %.1e)'
          % (label, p['knots'].size - 4, p['t'].size, dev, p['fp64'], p['cond'], p['bar']))
    assert c.shape == p['ref'].shape and np.all(np.isfinite(c))
    assert dev <= p['bar'], (label, dev, p['bar'])
    return dev


@pytest.mark.gpu
@pytest.mark.parametrize('name', pe.LSQ_KNOTS)
def test_lsq_fit_against_the_50_digit_solve(name):
    for m in (0,) + pe.LSQ_SIZES:
        _lsq_check(name, pe.lsq_problem(name, m))


@pytest.mark.gpu
def test_lsq_fit_ill_conditioned():
    _lsq_check('one sample under the last coefficient', pe.lsq_ill_conditioned())


@pytest.mark.gpu
def test_lsq_fit_refusals_and_the_closed_right_end():
    from mvus_amd import spline
    rng = np.random.default_rng(11)
    k5, k6 = pe.lsq_knots('n5'), np.concatenate((np.zeros(4), [0.3, 0.6], np.ones(4)))

    def refused(knots, t, what='Schoenberg-Whitney'):
        with pytest.raises(ValueError, match=what):
            spline.lsq_fit(knots, t, pe.lsq_curve(t, rng))
    refused(k5, rng.uniform(0.0, 0.39, 50))                                    # the last span, and with it the last coefficient, has no data
    refused(pe.lsq_knots('n40'), rng.uniform(0.0, 0.5, 300))
    # the middle span has no data and the last has one sample: every coefficient has data, yet the rank is 5 of 6 -- the pivot is
    # rounding residue of either sign
    for m in (6, 255, 2049):
        refused(k6, np.concatenate((rng.uniform(0.0, 0.3, m - 1), [0.8])))
    refused(k5, np.array([0.0, 0.3, 0.6, 1.0]))                                # m < n
    refused(k5, np.array([0.1, 0.2, 0.7, 0.9]))
    refused(pe.lsq_knots('n40'), np.linspace(0.0, 1.0, 39))
    # a sample exactly on knots[n] is accepted, one ulp outside (either end) is refused
    p = pe.lsq_problem('n5', 255)
    assert p['t'].max() == 1.0 and p['t'].min() == 0.0
    t = np.array(p['t'])
    t[np.argmax(t)] = np.nextafter(1.0, 2.0)
    refused(k5, t, 'outside the knot interval')
    t = np.array(p['t'])
    t[np.argmin(t)] = -5e-324
    refused(k5, t, 'outside the knot interval')
