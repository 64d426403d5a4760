"""Case builders and references for the edge tests of the three device paths that hand the BA its starting point:
k_triangulate (csrc/triangulate.hip.h), mvus_pnp_ransac (csrc/pnp.hip.h, twoview_api.hip) and mvus_spline_lsq (k_lsq_accumulate,
k_lsq_solve in csrc/spline_ops.hip.h).  Importable without a GPU: tests/test_pose_edges_host.py proves every premise on the
references and the host build alone, tests/test_gpu_pose_edges.py holds the kernels to the same bars.

* triangulation: per point the right singular vector of the smallest singular value of the 4x4 matrix in the header of
  triangulate.hip.h, by ``mpmath.svd_r`` at 50 digits on the fp64 inputs converted exactly; the bar comes from the deviation of
  the LAPACK route (oracle/triangulate_oracle.triangulate_matlab) from that reference, never from the kernel;
* PnP: a builder that keeps the camera looking at the points (every pixel inside the image: the distortion model stays
  invertible over them), and a restatement of the RANSAC stage from the host build of the device math -- sampler, undistortion,
  six-point pose, squared pixel error -- with the driver's centring, scaling and first-maximum rule;
* least squares on fixed knots: B by the de Boor-Cox recurrence and the normal equations by ``mpmath.lu_solve`` at 50 digits.

Every input is seeded; every reference is computed once per process and handed out read-only."""
import functools
import os
import sys

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
from mvus_amd import _lib                                  # noqa: E402
from oracle import pnp_oracle as po                        # noqa: E402
from oracle import triangulate_oracle as tri               # noqa: E402

DPS = 50
K = np.array([[1100.0, 0.0, 960.0], [0.0, 1080.0, 540.0], [0.0, 0.0, 1.0]])
KV = np.array([1100.0, 1080.0, 960.0, 540.0])
WIDTH, HEIGHT = 1920.0, 1080.0


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def angle_deg(Ra, Rb):
    return np.degrees(np.arccos(np.clip((np.trace(Ra.T @ Rb) - 1) / 2, -1, 1)))


# ---- triangulation -------------------------------------------------------------------------------------------------------------
# geometry: baseline, pixel noise, factor on P2, factor on the depth
TRI_GEOMETRIES = {'wide': (5.0, 0.5, 1.0, 1.0), 'base1e-2': (1e-2, 0.5, 1.0, 1.0), 'base1e-4': (1e-4, 0.0, 1.0, 1.0),
                  'base1e-4-noisy': (1e-4, 0.5, 1.0, 1.0), 'Pscaled': (5.0, 0.5, 1e3, 1.0), 'far': (5.0, 0.1, 1.0, 1e4)}
# every geometry at two sizes, every size of 1, 255, 256, 257, 513 at least once
TRI_CASES = [('wide', 1), ('wide', 513), ('base1e-2', 255), ('base1e-2', 257), ('base1e-4', 1), ('base1e-4', 256),
             ('base1e-4-noisy', 255), ('base1e-4-noisy', 257), ('Pscaled', 256), ('Pscaled', 513), ('far', 255), ('far', 513)]
TRI_X_FLOOR = 1e-12        # relative to |X_ref|
TRI_ERR_FLOOR = 1e-10      # px: pixels are ~1e3, so a few hundred ulp
TRI_BAR_FACTOR = 8.0       # times the LAPACK route's own deviation from the 50-digit reference, worst over the case


def _camera(centre, rvec):
    R = po.rodrigues(rvec)
    return K @ np.hstack((R, (-R @ centre).reshape(3, 1)))


def tri_inputs(geometry, N):
    """(P1, P2, x1[2, N], x2[2, N]) of a seeded camera pair: K = (1100, 1080, 960, 540), points x, y in +-5, z in 20..40."""
    base, noise, scale, depth = TRI_GEOMETRIES[geometry]
    rng = np.random.default_rng(1000 * sorted(TRI_GEOMETRIES).index(geometry) + N)
    X = np.vstack((rng.uniform(-5, 5, (2, N)), rng.uniform(20, 40, (1, N)) * depth, np.ones((1, N))))
    P1 = _camera(np.zeros(3), np.array([0.01, 0.02, 0.0]))
    P2 = _camera(np.array([base, 0.1 * base, 0.0]), np.array([0.0, -0.03, 0.01])) * scale
    x1 = P1 @ X
    x1 = x1[:2] / x1[2] + rng.normal(0, noise, (2, N))
    x2 = P2 @ X
    x2 = x2[:2] / x2[2] + rng.normal(0, noise, (2, N))
    return P1, P2, np.ascontiguousarray(x1), np.ascontiguousarray(x2)


def tri_reference_indices(N):
    """every point up to N = 257; above: the workgroup edges, the last point and 32 random ones"""
    if N <= 257:
        return np.arange(N)
    edges = {i for i in (0, 255, 256, 511, 512, N - 1) if i < N}
    extra = np.random.default_rng(N).choice(N, 32, replace=False)
    return np.array(sorted(edges | set(int(i) for i in extra)))


def tri_reference(P1, P2, x1, x2, idx):
    """X[4, len(idx)] and the two reprojection distances of the 50-digit point, all at 50 digits and rounded once."""
    X, e1, e2 = np.zeros((4, idx.size)), np.zeros(idx.size), np.zeros(idx.size)
    with mp.workdps(DPS):
        Pm = [[[mp.mpf(float(P[r, j])) for j in range(4)] for r in range(3)] for P in (P1, P2)]
        for k, i in enumerate(idx):
            px = [(mp.mpf(float(x1[0, i])), mp.mpf(float(x1[1, i]))), (mp.mpf(float(x2[0, i])), mp.mpf(float(x2[1, i])))]
            A = mp.matrix(4, 4)
            for c in range(2):
                for j in range(4):
                    A[2 * c, j] = px[c][0] * Pm[c][2][j] - Pm[c][0][j]
                    A[2 * c + 1, j] = px[c][1] * Pm[c][2][j] - Pm[c][1][j]
            _U, S, V = mp.svd_r(A)
            q = min(range(4), key=lambda r: S[r])
            v = [V[q, j] / V[q, 3] for j in range(4)]
            X[:, k] = [float(a) for a in v]
            for c, out in ((0, e1), (1, e2)):
                h = [sum(Pm[c][r][j] * v[j] for j in range(4)) for r in range(3)]
                out[k] = float(mp.sqrt((px[c][0] - h[0] / h[2]) ** 2 + (px[c][1] - h[1] / h[2]) ** 2))
    return X, e1, e2


def tri_x_deviation(X, ref, idx):
    """worst |X - X_ref| / |X_ref| over the reference points"""
    return float(np.max(np.linalg.norm(X[:3, idx] - ref[:3], axis=0) / np.linalg.norm(ref[:3], axis=0)))


@functools.lru_cache(maxsize=None)
def tri_problem(geometry, N):
    """The inputs, the 50-digit reference at ``idx``, the LAPACK route's deviation from it and the bars that deviation sets."""
    P1, P2, x1, x2 = tri_inputs(geometry, N)
    idx = tri_reference_indices(N)
    X_ref, e1_ref, e2_ref = tri_reference(P1, P2, x1, x2, idx)
    L = tri.triangulate_matlab(x1, x2, P1, P2)
    lapack_x = tri_x_deviation(L, X_ref, idx)
    lapack_e = max(float(np.max(np.abs(tri.reprojection_error(x, tri.project(P, L[:-1]))[idx] - e)))
                   for x, P, e in ((x1, P1, e1_ref), (x2, P2, e2_ref)))
    _frozen(P1, P2, x1, x2, idx, X_ref, e1_ref, e2_ref)
    return dict(P1=P1, P2=P2, x1=x1, x2=x2, idx=idx, X_ref=X_ref, e1_ref=e1_ref, e2_ref=e2_ref, lapack_x=lapack_x, lapack_e=lapack_e,
                bar_x=max(TRI_BAR_FACTOR * lapack_x, TRI_X_FLOOR), bar_e=max(TRI_BAR_FACTOR * lapack_e, TRI_ERR_FLOOR))


def tri_check(name, p, X, e1, e2):
    """Print the measured worst cases beside their bars and assert them; returns (x deviation, error deviation)."""
    dx = tri_x_deviation(X, p['X_ref'], p['idx'])
    de = max(float(np.max(np.abs(e1[p['idx']] - p['e1_ref']))), float(np.max(np.abs(e2[p['idx']] - p['e2_ref']))))
    print('%s: |X - X_ref| / |X_ref| %.3e (LAPACK route %.3e, bar %.3e); reprojection distance %.3e px (LAPACK route %.3e, bar %.3e)'
          % (name, dx, p['lapack_x'], p['bar_x'], de, p['lapack_e'], p['bar_e']))
    np.testing.assert_array_equal(X[3], 1.0)
    assert dx <= p['bar_x'], (name, dx, p['bar_x'])
    assert de <= p['bar_e'], (name, de, p['bar_e'])
    return dx, de


def tri_with_degenerate_lane(p, at=255):
    """(x1, x2) of ``p`` with one degenerate pair at index ``at``.  The two cameras are arguments of the whole call, so a single lane
    cannot have P2 = P1; what a single lane can have is the pair of epipoles -- both rays run along the baseline, the 4x4 matrix has
    rank 2 and no point is defined, which is the same degeneracy."""
    def centre(P):
        return -np.linalg.solve(P[:, :3], P[:, 3])
    x1, x2 = p['x1'].copy(), p['x2'].copy()
    e1 = p['P1'] @ np.append(centre(p['P2']), 1.0)
    e2 = p['P2'] @ np.append(centre(p['P1']), 1.0)
    x1[:, at], x2[:, at] = e1[:2] / e1[2], e2[:2] / e2[2]
    return x1, x2


# ---- PnP -------------------------------------------------------------------------------------------------------------------------
D0 = (0.0, 0.0, 0.0, 0.0, 0.0)
D1 = (-0.12, 0.03, 1e-3, -5e-4, 0.0)
D2 = (0.2, -0.1, 0.0, 0.0, 0.05)
# N, iterations, noise px, outlier share, points behind the camera, distortion
PNP_CASES = [(6, 1, 0.2, 0.0, 0, D0), (7, 63, 0.2, 0.0, 0, D1), (64, 64, 0.5, 0.2, 3, D1), (255, 65, 0.5, 0.1, 0, D2),
             (256, 100, 0.5, 0.3, 5, D1), (257, 1, 0.5, 0.0, 0, D1), (513, 100, 0.5, 0.2, 4, D2), (2049, 64, 0.5, 0.1, 0, D1)]
PNP_BUILD_SEEDS = [300, 400, 302, 401, 402, 403, 404, 405]        # of the builder, case by case
PNP_SEED, PNP_THRESHOLD = 3, 8.0                 # of the sampler; pixels
PNP_ANGLE_BAR, PNP_T_BAR = 1e-6, 1e-7            # degrees; relative to |t_ref|: the bars of tests/test_pnp.py
PNP_BOUNDARY = 1e-9                              # a squared error within this (relative) of thr^2 may fall either way
HEAVY_FROM = 64
HEAVY_SHIFT = np.array([[3.0], [-3.0]])          # 4.2 px: inside the 8 px threshold, yet each such point pulls the minimiser visibly


@functools.lru_cache(maxsize=None)
def pnp_problem(k):
    """Case k of PNP_CASES: dict(X[3, N], uv[2, N], d, R, t, bad[N], heavy, behind, clean_uv, depth).  Like test_pnp._problem, but
    the camera is aimed at the centroid of the points (a rotation of N(0, 0.03) rad on top), so every pixel is inside the image."""
    N, H, noise, outliers, behind, dist = PNP_CASES[k]
    rng = np.random.default_rng(PNP_BUILD_SEEDS[k])
    s = np.linspace(0.0, 600.0, N)
    X = np.vstack((10 * np.sin(s / 80), 10 * np.cos(s / 95), 30 + 3 * np.sin(s / 50))) + rng.normal(0, 0.05, (3, N))
    centre = np.array([3.0, -2.0, -15.0]) + rng.normal(0, 2.0, 3)
    z = X.mean(axis=1) - centre
    z /= np.linalg.norm(z)
    x = np.cross(np.array([0.1, 1.0, 0.0]), z)
    x /= np.linalg.norm(x)
    R = po.rodrigues(rng.normal(0, 0.03, 3)) @ np.vstack((x, np.cross(z, x), z))
    t = -R @ centre
    d = np.array(dist)
    clean_uv, depth = po.project(K, d, R, t, X)
    uv = clean_uv + rng.normal(0, noise, clean_uv.shape)
    bad = np.zeros(N, dtype=bool)
    if outliers:
        bad = rng.random(N) < outliers
        bad[[0, N - 1]] = False
        nb = int(bad.sum())
        uv[:, bad] += rng.uniform(30, 200, (2, nb)) * rng.choice([-1, 1], (2, nb))          # >= 30 px off
    behind_idx = np.zeros(0, dtype=np.int64)
    if behind:
        behind_idx = np.flatnonzero(~bad)[3:3 + behind]
        X[:, behind_idx] = (centre - 20 * z).reshape(3, 1) + rng.normal(0, 1, (3, behind_idx.size))
        bad[behind_idx] = True
    # no heavy points below N = 64: no 256-stride ends there, and among seven points two residuals of 4.2 px bias po.refine (scipy's
    # forward-difference Jacobian) by 1.4e-4 degrees, far above the bar it is the reference for; without them it repeats to 1e-8
    heavy = np.array([i for i in sorted({0, 255, 256, 511, 512, N - 1}) if i < N and not bad[i]] if N >= HEAVY_FROM else [], dtype=np.int64)
    uv[:, heavy] += HEAVY_SHIFT
    X, uv = np.ascontiguousarray(X), np.ascontiguousarray(uv)
    _frozen(X, uv, d, R, t, bad, heavy, behind_idx, clean_uv, depth)
    return dict(N=N, H=H, X=X, uv=uv, d=d, R=R, t=t, bad=bad, heavy=heavy, behind=behind_idx, clean_uv=clean_uv, depth=depth)


@functools.lru_cache(maxsize=None)
def pnp_restatement(k):
    """The RANSAC stage of mvus_pnp_ransac from the host build of its device functions: per hypothesis the inlier count and the
    number of boundary points, the winner (first maximum) and its mask."""
    from hostcheck_util import load
    lib = load()
    p = pnp_problem(k)
    N, H, X, uv = p['N'], p['H'], p['X'], p['uv']
    m = X.mean(axis=1, keepdims=True)
    sigma = np.sqrt(((X - m) ** 2).sum() / (3.0 * N))
    Xc = np.ascontiguousarray((X - m) / sigma)
    Kd = np.concatenate((KV, p['d']))
    xn = np.zeros((2, N))
    lib.hostcheck_undistort5(N, _lib.dptr(uv), _lib.dptr(Kd), _lib.dptr(xn))
    thr2 = PNP_THRESHOLD ** 2
    counts, near = np.zeros(H, dtype=np.int64), np.zeros(H, dtype=np.int64)
    errs = {}
    for h in range(H):
        idx = np.zeros(6, dtype=np.int64)
        lib.hostcheck_pnp_sample6(PNP_SEED, h, N, idx.ctypes.data_as(_lib.c_int64_p))
        assert len(set(idx.tolist())) == 6 and idx.min() >= 0 and idx.max() < N
        Rh, th = np.zeros(9), np.zeros(3)
        if not lib.hostcheck_pnp_dlt6(_lib.dptr(np.ascontiguousarray(Xc[:, idx].T)), _lib.dptr(np.ascontiguousarray(xn[:, idx].T)), _lib.dptr(Rh), _lib.dptr(th)):
            continue
        e2 = np.zeros(N)
        lib.hostcheck_pnp_sqerr(N, _lib.dptr(Xc), _lib.dptr(uv), _lib.dptr(Kd), _lib.dptr(Rh), _lib.dptr(th), _lib.dptr(e2))
        counts[h] = int(((e2 >= 0.0) & (e2 <= thr2)).sum())
        near[h] = int(((e2 >= 0.0) & (np.abs(e2 - thr2) <= PNP_BOUNDARY * thr2)).sum())
        errs[h] = e2
    best = int(np.argmax(counts))                                                             # ties: the first hypothesis
    mask = (errs[best] >= 0.0) & (errs[best] <= thr2) if best in errs else np.zeros(N, dtype=bool)
    _frozen(counts, near, mask)
    return dict(counts=counts, near=near, best=best, mask=mask, valid=len(errs))


def pnp_refine(p, mask, start=None):
    """po.refine (scipy Levenberg-Marquardt) on the flagged points, from the true pose or from ``start`` = (R, t)"""
    R0, t0 = (p['R'], p['t']) if start is None else start
    R, t, _cost = po.refine(K, p['d'], R0, t0, p['X'][:, mask], p['uv'][:, mask])
    return R, t


# ---- least squares on fixed knots --------------------------------------------------------------------------------------------------
LSQ_FLOOR, LSQ_BAR_FACTOR = 1e-12, 8.0
LSQ_SIZES = (255, 256, 257, 2049)                # and m = n (interpolation at the Greville sites)


def lsq_knots(name):
    """knot vectors on [0, 1]"""
    inner = {'n4': [], 'n5': [0.4], 'ratio1e3': [0.25, 0.25025, 0.2505, 0.5, 0.75], 'double': [0.2, 0.5, 0.5, 0.8],
             'n40': np.sort(np.random.default_rng(40).uniform(0, 1, 36))}[name]
    return np.concatenate((np.zeros(4), np.asarray(inner, dtype=np.float64), np.ones(4)))


LSQ_KNOTS = ('n4', 'n5', 'ratio1e3', 'double', 'n40')


def lsq_curve(t, rng, noise=0.02):
    """the trajectory of test_traj_to_spline._trajectory with its parameter rescaled to [0, 1] (u = 400 t)"""
    u = 400.0 * t
    return np.vstack((10 * np.sin(u / 80), 10 * np.cos(u / 95), 30 + 3 * np.sin(u / 50))) + rng.normal(0, noise, (3, t.size))


def lsq_sites(knots, m, rng):
    """m = n: the Greville sites.  Otherwise every distinct knot (both ends included), three random sites per span, the rest random."""
    n = knots.size - 4
    if m == n:
        return np.array([knots[j + 1:j + 4].sum() / 3 for j in range(n)])
    uk = np.unique(knots)
    sites = np.concatenate([uk] + [rng.uniform(a, b, 3) for a, b in zip(uk[:-1], uk[1:])])
    assert sites.size <= m
    t = np.concatenate((sites, rng.uniform(0, 1, m - sites.size)))
    return rng.permutation(t)                     # unsorted: neighbouring lanes hit different rows of the normal equations


def _basis_mp(km, l, x):
    """de Boor-Cox: the four cubic B-splines that are non-zero on span l, at 50 digits"""
    h = [mp.mpf(1)]
    for j in range(1, 4):
        hh = h[:]
        h = [mp.mpf(0)] * (j + 1)
        for i in range(j):
            li, lj = l + 1 + i, l + 1 + i - j
            f = hh[i] / (km[li] - km[lj])
            h[i] += f * (km[li] - x)
            h[i + 1] = f * (x - km[lj])
    return h


def lsq_span(knots, x):
    """l in [3, n - 1] with knots[l] <= x < knots[l + 1], the last span closed on the right"""
    n = knots.size - 4
    l = 3
    while l < n - 1 and x >= knots[l + 1]:
        l += 1
    return l


def lsq_reference(knots, t, X):
    """c[3, n] of the least-squares spline: normal equations built and solved at 50 digits, rounded once"""
    n = knots.size - 4
    with mp.workdps(DPS):
        km = [mp.mpf(float(v)) for v in knots]
        G, R = mp.zeros(n, n), mp.zeros(n, 3)
        for i, x in enumerate(t):
            l = lsq_span(knots, x)
            h = _basis_mp(km, l, mp.mpf(float(x)))
            for a in range(4):
                for b in range(4):
                    G[l - 3 + a, l - 3 + b] += h[a] * h[b]
                for d in range(3):
                    R[l - 3 + a, d] += h[a] * mp.mpf(float(X[d, i]))
        cols = [mp.lu_solve(G, R[:, d]) for d in range(3)]
        return np.array([[float(cols[d][j]) for j in range(n)] for d in range(3)])


def lsq_deviation(c, ref):
    return float(np.abs(np.asarray(c) - ref).max() / np.abs(ref).max())


def _lsq_finish(knots, t, X):
    from scipy import interpolate
    ref = lsq_reference(knots, t, X)
    B = interpolate.BSpline.design_matrix(t, knots, 3).toarray()
    fp64 = lsq_deviation(np.linalg.solve(B.T @ B, B.T @ X.T).T, ref)
    _frozen(knots, t, X, ref)
    return dict(knots=knots, t=t, X=X, ref=ref, fp64=fp64, cond=float(np.linalg.cond(B)), bar=max(LSQ_BAR_FACTOR * fp64, LSQ_FLOOR))


@functools.lru_cache(maxsize=None)
def lsq_problem(name, m):
    """knots, sites t[m], data X[3, m], the 50-digit coefficients, the deviation of an fp64 solve of the normal equations from them
    and the bar it sets.  m = 0 stands for m = n."""
    knots = lsq_knots(name)
    n = knots.size - 4
    m = m or n
    rng = np.random.default_rng(7000 + 10 * LSQ_KNOTS.index(name) + m)
    t = lsq_sites(knots, m, rng)
    return _lsq_finish(knots, t, lsq_curve(t, rng))


@functools.lru_cache(maxsize=None)
def lsq_ill_conditioned():
    """n = 5 (interior knot 0.4): the last coefficient's B-spline lives on (0.4, 1] alone, and one sample at 0.406 is all that supports
    it -- B_4(0.406) = (0.006 / 0.6)^3 = 1e-6, so cond(B) ~ 1e6.  63 more samples lie in [0, 0.4]."""
    knots = lsq_knots('n5')
    rng = np.random.default_rng(7999)
    t = rng.permutation(np.concatenate(([0.0, 0.4, 0.406], rng.uniform(0, 0.4, 61))))
    return _lsq_finish(knots, t, lsq_curve(t, rng))
