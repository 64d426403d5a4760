"""Two-view geometry of Scene.init_traj / sync_bf (csrc/epipolar.hip.h): cv2.findFundamentalMat(FM_RANSAC), cv2.correctMatches
and epipolar.triangulate_from_E restated on the GPU.  OpenCV is not in this image, so nothing pins the RANSAC output to
OpenCV's; what is checked:

* CPU: the numpy restatement (tests/epipolar_oracle.py) against the reference's own compute_Rt_from_E, triangulate_from_E and
  Sampson_error (tests/golden/epipolar_2cam.npz, tests/golden/make_golden_epipolar.py), its 7-point solver and Hartley-Sturm
  correction against first principles, and the sampler the kernels share with it;
* GPU: F by RANSAC on synthetic pairs with 30 % gross outliers against the true F and the oracle's error, determinism,
  batched == single calls bit for bit, the error paths; correct_matches against the oracle; pose_from_essential against the
  reference's golden output.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import epipolar_oracle as eo                               # noqa: E402
from mvus_amd import _lib                                  # noqa: E402

GOLDEN = os.path.join(HERE, 'golden', 'epipolar_2cam.npz')


def _h(x):
    return np.vstack((x[:2], np.ones(x.shape[1])))


# ---- CPU: the oracle against the reference ----------------------------------------------------------------------------------
def test_oracle_decomposition_matches_reference():
    g = np.load(GOLDEN)
    Rt = eo.rt_from_E(g['E'])
    for a, b in zip(Rt, g['Rt']):
        np.testing.assert_allclose(a, b, rtol=0, atol=1e-12)
    x1n = np.linalg.inv(g['K1']) @ _h(g['x1'])
    x2n = np.linalg.inv(g['K2']) @ _h(g['x2'])
    X, P2 = eo.pose_from_essential(g['E'], x1n[:2], x2n[:2])
    np.testing.assert_array_equal(P2, g['P2'])                 # the same candidate, the same bits
    np.testing.assert_allclose(X, g['X'], rtol=1e-9, atol=0)


def test_oracle_error_against_reference_sampson():
    """OpenCV's error is the larger of the two squared line distances d1, d2; the reference's Sampson error of the same F is
    their harmonic combination 1 / (1/d1 + 1/d2): both built from the same residual and line vectors."""
    g = np.load(GOLDEN)
    d1, d2 = eo.line_distances2(g['F'], g['x1'], g['x2'])
    np.testing.assert_allclose(1.0 / (1.0 / d1 + 1.0 / d2), g['sampson'], rtol=1e-6, atol=1e-300)   # residuals ~1e-4 of terms ~1e3: cancellation
    np.testing.assert_allclose(eo.fm_error(g['F'], g['x1'], g['x2']), np.maximum(d1, d2), rtol=1e-6, atol=1e-300)


def test_oracle_seven_point_recovers_true_F():
    x1, x2, F, _, _ = eo.synthetic_pair(50, sigma=0.0, outliers=0.0, seed=3)
    T1, T2 = eo.hartley_normalisation(x1), eo.hartley_normalisation(x2)
    h1, h2 = (T1 @ _h(x1))[:2], (T2 @ _h(x2))[:2]
    models = [eo.unit(T2.T @ Fn @ T1) for Fn in eo.seven_point(h1[:, :7], h2[:, :7])]
    assert 1 <= len(models) <= 3
    for M in models:
        assert np.max(eo.fm_error(M, x1[:, :7], x2[:, :7])) < 1e-12
    assert min(np.abs(M - F).max() for M in models) < 1e-8


def test_oracle_hartley_sturm_is_optimal():
    x1, x2, F, _, _ = eo.synthetic_pair(40, sigma=2.0, outliers=0.2, seed=5)
    c1, c2 = eo.correct_matches(F, x1, x2)
    r = np.abs(np.sum(_h(c2) * (F @ _h(c1)), axis=0))
    assert r.max() < 1e-10 * np.linalg.norm(F) * 1e3 ** 2
    # no pair on the epipolar pencil is closer: brute force over the pencil of lines through the epipole
    U, _, Vt = np.linalg.svd(F)
    e1 = Vt[-1] / Vt[-1][2]
    for i in range(x1.shape[1]):
        best = np.sum((c1[:, i] - x1[:, i]) ** 2) + np.sum((c2[:, i] - x2[:, i]) ** 2)
        ang = np.linspace(0, np.pi, 20001)
        d = np.vstack((np.cos(ang), np.sin(ang)))
        p = x1[:, i:i + 1] - e1[:2, None]                    # x1 projected onto each line through e1
        q = e1[:2, None] + d * np.sum(d * p, axis=0)
        l2 = F @ np.vstack((q, np.ones(q.shape[1])))
        dist2 = np.sum((q - x1[:, i:i + 1]) ** 2, axis=0) + (l2[0] * x2[0, i] + l2[1] * x2[1, i] + l2[2]) ** 2 / (l2[0] ** 2 + l2[1] ** 2)
        assert best <= dist2.min() * (1 + 1e-6) + 1e-9


def test_sampler_host_restatement():
    for seed, N in ((0, 8), (1, 9), (12345, 2000), (2 ** 40 + 7, 10 ** 6)):
        draws = [eo.sample7(seed, h, N) for h in range(200)]
        for idx in draws:
            assert len(set(idx)) == 7 and all(0 <= i < N for i in idx)
        assert draws == [eo.sample7(seed, h, N) for h in range(200)]
    assert eo.sample7(0, 5, 1000) != eo.sample7(1, 5, 1000) and eo.sample7(0, 5, 1000) != eo.sample7(0, 6, 1000)
    assert eo.sample7(0, 5, 1000) != eo.sample7(0, 5, 1001)


# ---- GPU -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('N', [2000, 20000])
def test_fundamental_ransac(N):
    from mvus_amd.reconstruction import epipolar as ep
    x1, x2, Ft, bad, _ = eo.synthetic_pair(N, sigma=0.5, outliers=0.3, seed=11)
    F, mask = ep.computeFundamentalMat(x1, x2, error=3)
    s = np.linalg.svd(F, compute_uv=False)
    assert s[2] < 1e-10 * s[0]                                           # rank 2
    assert abs(np.linalg.norm(F) - 1.0) < 1e-12
    true_mask = eo.fm_error(Ft, x1, x2) <= 9.0
    agree = np.mean((mask == 1) == true_mask)
    print('N', N, 'inliers', int(mask.sum()), 'true', int(true_mask.sum()), 'agreement', agree)
    assert agree >= 0.99
    res, cnt = ep.fundamental_ransac_batch([(x1, x2)], error=3)
    assert int(cnt[0]) == int(np.count_nonzero(eo.fm_error(F, x1, x2) <= 9.0)) == int(mask.sum())
    np.testing.assert_array_equal(mask, eo.fm_error(F, x1, x2) <= 9.0)
    F2, mask2 = ep.computeFundamentalMat(x1, x2, error=3)
    np.testing.assert_array_equal(F, F2)
    np.testing.assert_array_equal(mask, mask2)
    with pytest.raises(NotImplementedError):
        ep.computeFundamentalMat(x1, x2, method=ep.FM_LMEDS)


@pytest.mark.gpu
def test_fundamental_ransac_batched_equals_single():
    from mvus_amd.reconstruction import epipolar as ep
    pairs = []
    for k in range(20):
        x1, x2, _, _, _ = eo.synthetic_pair(300 + 97 * k, sigma=0.5, outliers=0.3, seed=100 + k)
        pairs.append((x1, x2))
    batch, cnt = ep.fundamental_ransac_batch(pairs, error=3, seed=4)
    for k, (x1, x2) in enumerate(pairs):
        (F, m), = ep.fundamental_ransac_batch([(x1, x2)], error=3, seed=4)[0]
        np.testing.assert_array_equal(batch[k][0], F)
        np.testing.assert_array_equal(batch[k][1], m)
        assert cnt[k] == m.sum()


@pytest.mark.gpu
def test_fundamental_ransac_errors():
    from mvus_amd.reconstruction import epipolar as ep
    x1, x2, _, _, _ = eo.synthetic_pair(100, seed=2)
    with pytest.raises(ValueError, match='at least 8'):
        ep.computeFundamentalMat(x1[:, :7], x2[:, :7])
    bad = x1.copy()
    bad[0, 3] = np.nan
    with pytest.raises(ValueError, match='non-finite'):
        ep.computeFundamentalMat(bad, x2)
    with pytest.raises(ValueError):
        ep.computeFundamentalMat(x1, x2, error=0)
    same = np.tile(np.array([[500.0], [400.0]]), (1, 100))             # one view all at one pixel: no 7-point model
    with pytest.raises(RuntimeError, match='no valid 7-point model'):
        ep.computeFundamentalMat(same, x2)


@pytest.mark.gpu
def test_correct_matches_against_oracle():
    from mvus_amd.reconstruction import epipolar as ep
    x1, x2, F, bad, _ = eo.synthetic_pair(400, sigma=1.0, outliers=0.3, seed=21)
    x1[1, 7] = np.inf
    c1, c2 = ep.correct_matches(F, x1, x2)
    o1, o2 = eo.correct_matches(F, x1, x2)
    np.testing.assert_array_equal(np.isnan(c1), np.isnan(o1))
    assert np.isnan(c1[:, 7]).all() and np.isnan(c2[:, 7]).all() and np.isfinite(np.delete(c1, 7, axis=1)).all()
    fin = np.isfinite(o1[0])
    d = np.hypot(*(c1 - o1)) + np.hypot(*(c2 - o2))
    # inliers: a well-conditioned minimum, the same point to 1e-8 px
    assert d[fin & ~bad].max() <= 1e-8, d[fin & ~bad].max()
    # gross outliers: the minimum can be flat (near a double root of g, where the root is known to ~sqrt(eps) only); the same
    # cost to 1e-7 relative (measured: 8e-9)
    cost = lambda a, b: np.sum((a - x1) ** 2, axis=0) + np.sum((b - x2) ** 2, axis=0)
    np.testing.assert_allclose(cost(c1, c2)[fin], cost(o1, o2)[fin], rtol=1e-7)
    T1, T2 = eo.hartley_normalisation(x1[:, fin]), eo.hartley_normalisation(x2[:, fin])
    Fn = np.linalg.inv(T2).T @ F @ np.linalg.inv(T1)
    Fn /= np.linalg.norm(Fn)
    r = np.abs(np.sum((T2 @ _h(c2[:, fin])) * (Fn @ (T1 @ _h(c1[:, fin]))), axis=0))
    assert r.max() < 1e-10


@pytest.mark.gpu
def test_pose_from_essential_reproduces_reference():
    from mvus_amd.reconstruction import epipolar as ep
    g = np.load(GOLDEN)
    X, P2 = ep.triangulate_from_E(g['E'], g['K1'], g['K2'], _h(g['x1']), _h(g['x2']))
    np.testing.assert_allclose(P2, g['P2'], rtol=0, atol=1e-12)
    np.testing.assert_allclose(X, g['X'], rtol=1e-9, atol=0)
    for a, b in zip(ep.compute_Rt_from_E(g['E']), g['Rt']):
        np.testing.assert_allclose(a, b, rtol=0, atol=1e-12)
    lib = _lib.load()
    rc = lib.mvus_pose_from_essential(0, 0, _lib.dptr(np.zeros(9)), None, None, None, None)
    assert rc == _lib.MVUS_E_INVALID


def test_remaining_out_of_scope_methods_say_so():
    from mvus_amd.reconstruction import common, synchronization
    s = common.Scene()
    with pytest.raises(NotImplementedError):
        s.plot_reprojection()
    with pytest.raises(NotImplementedError, match='sync_iter'):
        synchronization.sync_iter(30.0, 30.0, None, None, 0, 0)
    assert common.Scene.init_traj is not common.Scene._out_of_scope


def test_init_traj_needs_two_cameras():
    from mvus_amd.reconstruction import common
    s = common.Scene()
    s.numCam = 1
    s.addCamera(common.Camera(K=np.eye(3), d=np.zeros(5), fps=30.0, resolution=[1920, 1080]))
    s.addDetection(np.zeros((3, 10)))
    with pytest.raises(NotImplementedError, match='at least two cameras'):
        s.init_traj()
