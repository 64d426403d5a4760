"""mvus_triangulate_cov (k_triangulate_cov of mvus_amd/csrc/triangulate.hip.h) behind reconstruction.epipolar.triangulate_with_cov:
the points and reprojection distances are mvus_triangulate's to the bit, the covariance is the Gauss-Newton (A^T A)^-1 at the returned
point (against the same expression in np.longdouble), it describes the scatter of the triangulated points (Monte-Carlo), degenerate
pairs get NaN without touching their neighbours, and bad arguments are refused.

The camera pair: K = fx = fy = 1500, centre (960, 540); both cameras look at X0 = (3, 40, 25) (z along the view, x = (0, 0, 1) x z
normalised, y = z x x); camera 1 at the origin, camera 2 at (b, 0, 0.5) with baselines b = 30, 5 and 1 m -- the point is 47 m away.
Every test prints measured / bar (run with -s)."""
import numpy as np
import pytest

X0 = np.array([3.0, 40.0, 25.0])
K = np.array([[1500.0, 0.0, 960.0], [0.0, 1500.0, 540.0], [0.0, 0.0, 1.0]])
BASELINES = (30.0, 5.0, 1.0)
PX = 0.7


def _look_at(C, target=X0):
    z = (target - C) / np.linalg.norm(target - C)
    x = np.cross([0.0, 0.0, 1.0], z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.vstack((x, y, z))
    return K @ np.hstack((R, (-R @ C)[:, None]))


def _pair(b):
    return _look_at(np.zeros(3)), _look_at(np.array([b, 0.0, 0.5]))


def _project(P, X):
    h = P @ np.vstack((X, np.ones((1, X.shape[1]))))
    return h[:2] / h[2]


def _noisy_points(b, N, seed, spread=2.0):
    """N points around X0 seen by the pair with 0.7 px of noise: (x1, x2, P1, P2)"""
    rng = np.random.default_rng(seed)
    P1, P2 = _pair(b)
    X = X0[:, None] + spread * rng.standard_normal((3, N))
    return _project(P1, X) + PX * rng.standard_normal((2, N)), _project(P2, X) + PX * rng.standard_normal((2, N)), P1, P2


def _cov_longdouble(P1, P2, X, s1, s2):
    """(A^T A)^-1 at X in np.longdouble, and cond(A^T A): A's four rows (P[r, :3] - x_r P[2, :3]) / (z sigma)"""
    L = np.longdouble
    rows = []
    Xh = np.append(X.astype(L), L(1))
    for P, s in ((P1, s1), (P2, s2)):
        P = P.astype(L)
        h = P @ Xh
        for r in range(2):
            rows.append((P[r, :3] - h[r] / h[2] * P[2, :3]) / (h[2] * L(s)))
    A = np.array(rows, dtype=L)
    M = A.T @ A
    # inverse by the adjugate, in long double throughout
    c = np.empty((3, 3), dtype=L)
    for i in range(3):
        for j in range(3):
            a, b_ = [k for k in range(3) if k != i], [k for k in range(3) if k != j]
            c[j, i] = (-1) ** (i + j) * (M[a[0], b_[0]] * M[a[1], b_[1]] - M[a[0], b_[1]] * M[a[1], b_[0]])
    det = M[0, 0] * c[0, 0] + M[0, 1] * c[1, 0] + M[0, 2] * c[2, 0]
    return c / det, float(np.linalg.cond(M.astype(np.float64)))


@pytest.mark.gpu
@pytest.mark.parametrize('N', [1, 63, 64, 65, 257])
def test_gpu_triangulate_cov_points_are_mvus_triangulates(N):
    """1a: X, err1, err2 bit for bit, at wavefront and workgroup edges; cov symmetric to the bit"""
    from mvus_amd.reconstruction import epipolar as ep
    for b in BASELINES:
        x1, x2, P1, P2 = _noisy_points(b, N, seed=N)
        X, e1, e2 = ep.triangulate_with_errors(x1, x2, P1, P2)
        Xc, cov, d1, d2 = ep.triangulate_with_cov(x1, x2, P1, P2, sigma1=PX, sigma2=PX)
        assert np.array_equal(X, Xc) and np.array_equal(e1, d1) and np.array_equal(e2, d2)
        assert cov.shape == (N, 3, 3) and np.array_equal(cov, cov.transpose(0, 2, 1)) and np.all(np.isfinite(cov))


@pytest.mark.gpu
@pytest.mark.parametrize('b', BASELINES)
def test_gpu_triangulate_cov_is_the_formula(b):
    """1b: against the same expression in np.longdouble at the returned X: 64 eps cond(A^T A) max|cov| per pair"""
    from mvus_amd.reconstruction import epipolar as ep
    x1, x2, P1, P2 = _noisy_points(b, 257, seed=7)
    s1, s2 = 0.7, 1.3
    X, cov, _, _ = ep.triangulate_with_cov(x1, x2, P1, P2, sigma1=s1, sigma2=s2)
    worst, conds = 0.0, []
    for i in range(X.shape[1]):
        ref, cond = _cov_longdouble(P1, P2, X[:3, i], s1, s2)
        bar = 64 * 2.0 ** -53 * cond * float(np.abs(ref).max())
        worst = max(worst, float(np.abs(cov[i].astype(np.longdouble) - ref).max()) / bar)
        conds.append(cond)
    print('\nbaseline %4.0f m  cond(A^T A) %.0f..%.0f  sigma %.3g m  measured / bar %.3g'
          % (b, min(conds), max(conds), float(np.sqrt(np.trace(cov, axis1=1, axis2=2) / 3).mean()), worst))
    assert worst <= 1


@pytest.mark.gpu
@pytest.mark.parametrize('b', BASELINES)
def test_gpu_triangulate_cov_monte_carlo(b):
    """1c: 20 000 noisy copies of one pair in one call: trace of the sample covariance of the points over the mean trace of cov within
    [0.9, 1.1] (the statistical 5-sigma of a variance from 20 000 samples is 5 %)"""
    from mvus_amd.reconstruction import epipolar as ep
    N = 20000
    rng = np.random.default_rng(0)
    P1, P2 = _pair(b)
    u1, u2 = _project(P1, X0[:, None]), _project(P2, X0[:, None])
    x1 = u1 + PX * rng.standard_normal((2, N))
    x2 = u2 + PX * rng.standard_normal((2, N))
    X, cov, _, _ = ep.triangulate_with_cov(x1, x2, P1, P2, sigma1=PX, sigma2=PX)
    assert np.all(np.isfinite(cov))
    sample = float(np.trace(np.cov(X[:3])))
    model = float(np.trace(cov, axis1=1, axis2=2).mean())
    print('\nbaseline %4.0f m  1-sigma %.4g m  sample trace / mean trace(cov) = %.4f  (bar 0.9 .. 1.1)' % (b, np.sqrt(model / 3), sample / model))
    assert 0.9 <= sample / model <= 1.1


@pytest.mark.gpu
def test_gpu_triangulate_cov_degenerate_pairs():
    """1d: identical cameras, or a point behind a camera: NaN in all six entries; the neighbours of such a pair in the same call keep
    their bits"""
    from mvus_amd.reconstruction import epipolar as ep
    x1, x2, P1, P2 = _noisy_points(5.0, 130, seed=3)
    _, cov_same, _, _ = ep.triangulate_with_cov(x1, x1, P1, P1)
    assert np.all(np.isnan(cov_same))
    X, cov, d1, d2 = ep.triangulate_with_cov(x1, x2, P1, P2)
    behind = (-X0)[:, None]                                    # behind both cameras: projects to finite pixels, triangulates back to itself
    y1, y2 = x1.copy(), x2.copy()
    for i in (0, 64, 129):
        y1[:, i], y2[:, i] = _project(P1, behind)[:, 0], _project(P2, behind)[:, 0]
    Xb, covb, b1, b2 = ep.triangulate_with_cov(y1, y2, P1, P2)
    bad = np.zeros(130, dtype=bool)
    bad[[0, 64, 129]] = True
    np.testing.assert_allclose(Xb[:3, bad], np.repeat(behind, 3, axis=1), rtol=1e-6)
    assert np.all(np.isnan(covb[bad])) and np.all(np.isfinite(covb[~bad]))
    assert np.array_equal(covb[~bad], cov[~bad]) and np.array_equal(Xb[:, ~bad], X[:, ~bad])
    assert np.array_equal(b1[~bad], d1[~bad]) and np.array_equal(b2[~bad], d2[~bad])


@pytest.mark.gpu
def test_gpu_triangulate_cov_refusals():
    """1e: sigma <= 0 (or not finite) and cov == NULL are MVUS_E_INVALID with a message; the next legal call is intact"""
    from mvus_amd import _lib
    from mvus_amd.reconstruction import epipolar as ep
    x1, x2, P1, P2 = _noisy_points(5.0, 10, seed=1)
    good = ep.triangulate_with_cov(x1, x2, P1, P2)
    for kw in (dict(sigma1=0.0), dict(sigma2=-1.0), dict(sigma1=np.nan), dict(sigma2=np.inf)):
        with pytest.raises(ValueError, match='sigma'):
            ep.triangulate_with_cov(x1, x2, P1, P2, **kw)
    lib = _lib.load()
    a, b = np.ascontiguousarray(x1), np.ascontiguousarray(x2)
    X = np.zeros((4, 10))
    rc = lib.mvus_triangulate_cov(0, 10, _lib.dptr(a), _lib.dptr(b), _lib.dptr(np.ascontiguousarray(P1)), _lib.dptr(np.ascontiguousarray(P2)), 1.0, 1.0,
                                  _lib.dptr(X), None, None, None)
    assert rc == _lib.MVUS_E_INVALID and b'cov is NULL' in lib.mvus_last_error(None)
    again = ep.triangulate_with_cov(x1, x2, P1, P2)
    assert all(np.array_equal(p, q) for p, q in zip(good, again))
