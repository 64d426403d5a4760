"""Host build of the two-view device functions of csrc/epipolar.hip.h (tests/hostcheck, g++) against high-precision references
(mpmath at 60 digits): the cubic of the 7-point solver and the 7-point model sets, and the pair error the GPU RANSAC and its
numpy restatement (tests/epipolar_oracle.py) must share bit for bit.  (The Hartley-Sturm correction is not yet pinned to an
mpmath reference here.)

Every bar below is a measured worst case times a stated margin; the measurement is in the comment next to it."""
import os
import sys

import mpmath as mp
import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import epipolar_oracle as eo                               # noqa: E402
import hostcheck_util                                      # noqa: E402
from mvus_amd import _lib                                  # noqa: E402

DPS = 60


@pytest.fixture(scope='module')
def lib():
    return hostcheck_util.load()


# ---- fm_cubic_roots ----------------------------------------------------------------------------------------------------------
def cubic_roots(lib, c):
    c = np.ascontiguousarray(c, dtype=np.float64)
    r = np.zeros(3)
    n = lib.hostcheck_fm_cubic_roots(_lib.dptr(c), _lib.dptr(r))
    return np.sort(r[:n])


def ref_roots(c):
    """All complex roots of the polynomial with the exact (double) coefficients c (highest first), leading zeros dropped."""
    with mp.workdps(DPS):
        cs = [mp.mpf(float(v)) for v in c]
        while cs and cs[0] == 0:
            cs.pop(0)
        if len(cs) < 2:
            return []
        return [mp.mpc(z) for z in mp.polyroots(cs, maxsteps=400, extraprec=400)]


def coeffs_from_roots(roots, lead=1.0):
    """Coefficients (highest first, rounded to double) of lead * prod (x - r); roots given as mpmath-readable numbers."""
    with mp.workdps(DPS):
        p = [mp.mpf(lead)]
        for r in roots:
            r = mp.mpf(r)
            p = [a - r * b for a, b in zip(p + [0], [0] + p)]
        return np.array([float(v) for v in p])


# The rule, for the kernel and the oracle alike.  Reference roots z (of the double coefficients, 60 digits), scale s = max(1, |z|):
# * a real root at more than 1e-6 s from every other root comes back to ISO s;
# * a root in a cluster (another root within 1e-6 s: a (near-)double pair or a triple root, real or a complex pair with an imaginary
#   part below 1e-6 s) is a root of an ill-conditioned cluster, known to ~sqrt(eps) only: some returned root lies within
#   CLUSTER s + (the distance to its partner);
# * every returned root lies within that same bound of some reference root.
ISO = 1e-9           # the issue's 1e-9 relative.  Measured worst: 1.4e-15 s on well-separated roots (margin ~1e6), but 0.32 of
                     # this bound on isolated roots only 1e-5 apart (test_cubic_near_double_roots): a margin of ~3 there
CLUSTER = 1e-7       # measured worst 0.58 of the whole bound (gap 1e-6), 2.5e-8 s at gaps <= 1e-8 (~sqrt(eps)): a margin of 1.7 - 4


def _bounds(z_all):
    out = []
    for i, z in enumerate(z_all):
        s = max(1.0, float(abs(z)))
        near = min([float(abs(z - w)) for j, w in enumerate(z_all) if j != i] or [np.inf])
        if near <= 1e-6 * s:
            out.append((z, CLUSTER * s + near, True))
        elif abs(z.imag) <= 1e-30 * s:
            out.append((z, ISO * s, False))
    return out


def check_roots(got, z_all):
    """Returns the worst (distance / bound) over both directions; asserts the rule above."""
    bounds = _bounds(z_all)
    worst = 0.0
    for z, b, clustered in bounds:
        d = min([float(abs(mp.mpc(x) - z)) for x in got] or [np.inf])
        assert d <= b, ('missing root', z, got, d, b)
        worst = max(worst, d / b)
    for x in got:
        d = min([(float(abs(mp.mpc(x) - z)) / b) for z, b, _ in bounds] or [np.inf])
        assert d <= 1.0, ('spurious root', x, z_all)
        worst = max(worst, d)
    return worst


def test_cubic_three_real_roots_wide_range(lib):
    rng = np.random.default_rng(1)
    worst = 0.0
    cases = [(1e-4, 1.0, 1e4), (-3.0, 0.5, 7.0), (-1e3, 1e-3, 2.0), (1e-6, 2e-6, 1.0), (-5e5, 3.0, 4e5)]
    cases += [tuple(rng.uniform(-1, 1, 3) * 10.0 ** rng.uniform(-4, 4, 3)) for _ in range(200)]
    for roots in cases:
        for lead in (1.0, -3.5e-3, 2.0e5):
            c = coeffs_from_roots(roots, lead)
            z = ref_roots(c)
            got = cubic_roots(lib, c)
            worst = max(worst, check_roots(got, z))
    print('three real roots: worst distance / bound', worst)


def test_cubic_one_real_root_and_complex_pair(lib):
    rng = np.random.default_rng(2)
    for _ in range(200):
        r = rng.uniform(-10, 10)
        m, y = rng.uniform(-10, 10), 10.0 ** rng.uniform(-3, 1)
        with mp.workdps(DPS):
            p = [1, -2 * mp.mpf(m), mp.mpf(m) ** 2 + mp.mpf(y) ** 2]            # x^2 - 2 m x + m^2 + y^2
            c = np.array([float(v) for v in (p[0], p[1] - r * p[0], p[2] - r * p[1], -r * p[2])])
        z = ref_roots(c)
        got = cubic_roots(lib, c)
        check_roots(got, z)
        assert len(got) == 1                                     # the pair's imaginary part is >= 1e-3: not a double root


def test_cubic_exact_double_root(lib):
    """(l - 1)^2 (l - 2) = l^3 - 4 l^2 + 5 l - 2: the double root at 1 must come back."""
    for c in ([1.0, -4.0, 5.0, -2.0], [-2.0, 8.0, -10.0, 4.0], [1.0, -5.0, 8.0, -4.0], [1.0, 0.0, -3.0, 2.0], [1.0, 0.0, -3.0, -2.0]):
        got = cubic_roots(lib, c)
        z = ref_roots(c)
        check_roots(got, z)
        assert len(got) == 2, (c, got)
    np.testing.assert_allclose(cubic_roots(lib, [1.0, -4.0, 5.0, -2.0]), [1.0, 2.0], rtol=0, atol=1e-8)


@pytest.mark.parametrize('gap', [1e-3, 1e-4, 1e-5, 1e-6, 1e-7, 1e-8, 1e-9, 1e-10])
def test_cubic_near_double_roots(lib, gap):
    """Roots r, r + gap, s: either both close roots or their cluster come back; never only the distant root."""
    rng = np.random.default_rng(int(-np.log10(gap)))
    worst = 0.0
    for _ in range(300):
        r, s = rng.uniform(-3, 3), rng.uniform(-3, 3)
        if abs(r - s) < 0.3:
            continue
        d = gap * rng.uniform(1.0, 10.0)
        c = coeffs_from_roots([r, mp.mpf(r) + mp.mpf(d), s], rng.choice([1.0, -0.7, 13.0]))
        got = cubic_roots(lib, c)
        worst = max(worst, check_roots(got, ref_roots(c)))
    print('gap', gap, 'worst distance / bound', worst)


def test_cubic_triple_root(lib):
    for r in (1.0, -2.5, 0.0, 3e3):
        c = coeffs_from_roots([r, r, r])
        got = cubic_roots(lib, c)
        assert len(got) >= 1
        # a triple root is known to eps^(1/3) ~ 6e-6 of the scale only
        np.testing.assert_allclose(got, r, rtol=0, atol=1e-4 * max(1.0, abs(r)))


def test_cubic_leading_coefficient_cutoff(lib):
    """|c3| <= 1e-12 max|c|: the cubic term is ignored (the quadratic's roots); just above it, all three roots."""
    for q in ([1.0, -3.0, 2.0], [2.0, 1.0, -6.0], [1.0, -2.0, 1.0 - 1e-6]):
        mx = max(abs(v) for v in q)
        below = [0.99e-12 * mx] + q
        got = cubic_roots(lib, below)
        check_roots(got, ref_roots(q))                         # the roots of c2 l^2 + c1 l + c0
        check_roots(got, [z for z in ref_roots(below) if abs(z) < 1e6])
        above = [1.01e-12 * mx] + q
        got = cubic_roots(lib, above)
        assert len(got) == 3
        check_roots(got, ref_roots(above))
    # the quadratic branch returns both roots: c0 / q is the second one
    got = cubic_roots(lib, [0.0, 1.0, -3.0, 2.0])
    np.testing.assert_allclose(got, [1.0, 2.0], rtol=1e-15)
    got = cubic_roots(lib, [0.0, 0.0, 2.0, -3.0])
    np.testing.assert_allclose(got, [1.5], rtol=1e-15)
    assert len(cubic_roots(lib, [0.0, 1.0, 0.0, 1.0])) == 0


def test_cubic_zero_constant_and_zero_polynomial(lib):
    got = cubic_roots(lib, [1e-300, 1e-300, -1e-300, 1e-300])         # tiny coefficients: one real root, not a false pair
    assert len(got) == 1
    check_roots(got, ref_roots([1e-300, 1e-300, -1e-300, 1e-300]))
    for c in ([1.0, -3.0, 2.0, 0.0], [2.0, 0.5, -7.0, 0.0], [1.0, 0.0, 1.0, 0.0]):
        got = cubic_roots(lib, c)
        check_roots(got, ref_roots(c))
        assert np.min(np.abs(got)) == 0.0
    assert len(cubic_roots(lib, [0.0, 0.0, 0.0, 0.0])) == 0


def test_oracle_seven_point_root_rule_matches_kernel(lib):
    """epipolar_oracle.cubic_roots states the same rule: the same number of roots as the kernel, the same values."""
    rng = np.random.default_rng(7)
    cases = [[1.0, -4.0, 5.0, -2.0], [1.0, -3.0, 3.0, -1.0], [0.0, 1.0, -3.0, 2.0], [1.0, -3.0, 2.0, 0.0]]
    for gap in (1e-3, 1e-6, 1e-7, 1e-8, 1e-9, 1e-10):
        for _ in range(50):
            r, s = rng.uniform(-3, 3), rng.uniform(-3, 3)
            cases.append(list(coeffs_from_roots([r, mp.mpf(r) + mp.mpf(gap), s])))
    for c in cases:
        k = cubic_roots(lib, c)
        o = np.sort(eo.cubic_roots(*c))
        assert len(k) == len(o), (c, k, o)
        np.testing.assert_allclose(k, o, rtol=1e-15, atol=0)          # measured: equal bits (libm cbrt, acos, cos may differ by an ulp)


# ---- fm_error ----------------------------------------------------------------------------------------------------------------
def test_fm_error_bitwise_equals_oracle(lib):
    """The GPU RANSAC counts equal the restatement's only if the pair error is the same bits: same expression, same order, no
    fused multiply-add.  Pairs include ones moved onto the threshold's boundary (error == thresh^2 to the last bits)."""
    x1, x2, F, _, _ = eo.synthetic_pair(3000, sigma=2.0, outliers=0.3, seed=9)
    x1 = np.ascontiguousarray(x1)
    x2 = np.ascontiguousarray(x2)
    # boundary pairs: x2 moved along the normal of its epipolar line so that its distance is exactly 3 px (to rounding)
    l = F @ np.vstack((x1[:, :500], np.ones(500)))
    n = l[:2] / np.hypot(l[0], l[1])
    x2[:, :500] -= n * ((np.sum(l[:2] * x2[:, :500], axis=0) + l[2]) / np.hypot(l[0], l[1]) - 3.0)
    Fc = np.ascontiguousarray(F.reshape(9))
    e = np.zeros(x1.shape[1])
    lib.hostcheck_fm_error(x1.shape[1], _lib.dptr(Fc), _lib.dptr(x1), _lib.dptr(x2), _lib.dptr(e))
    np.testing.assert_array_equal(e, eo.fm_error(F, x1, x2))
    near = np.abs(e[:500] - 9.0) <= 1e-6 * 9.0
    assert near.sum() >= 100 and (e[:500] <= 9.0).any() and (e[:500] > 9.0).any()


# ---- fm_seven_point ----------------------------------------------------------------------------------------------------------
def seven_point_host(lib, xs):
    xs = np.ascontiguousarray(xs, dtype=np.float64)
    Fs = np.zeros((3, 9))
    n = lib.hostcheck_fm_seven_point(_lib.dptr(xs), _lib.dptr(Fs))
    return [Fs[k].reshape(3, 3) for k in range(n)]


def _canon(F):
    F = np.asarray(F, dtype=np.float64) / np.linalg.norm(F)
    return F if F.flat[np.argmax(np.abs(F))] > 0 else -F


def seven_point_reference(xs):
    """The 7-point model set of the double sample xs (7 x 4) at 60 digits: the 2-D null space of the 7 x 9 system by
    Gauss-Jordan with partial pivoting, the cubics det(N1 + mu N2) and det(mu N1 + N2) interpolated exactly at mu = 0, 1, -1, 2,
    their roots in |mu| <= 1 by polyroots (every model of the pencil is one of them, none at infinity).  A complex pair with |Im| <= 1e-6 is a
    (near-)double root of the rounded sample and stands for one model at its real part (the cubic rule of the kernel).
    Returns [] for a sample of rank < 7."""
    with mp.workdps(DPS):
        A = [[mp.mpf(float(v)) for v in (u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, 1.0)] for u1, v1, u2, v2 in xs]
        amax = max(abs(v) for row in A for v in row)
        piv = []
        r = 0
        for col in range(9):
            if r == 7:
                break
            p = max(range(r, 7), key=lambda i: abs(A[i][col]))
            if abs(A[p][col]) <= mp.mpf(10) ** -40 * amax:
                continue
            A[r], A[p] = A[p], A[r]
            pv = A[r][col]
            A[r] = [v / pv for v in A[r]]
            for i in range(7):
                if i != r and A[i][col] != 0:
                    f = A[i][col]
                    A[i] = [a - f * b for a, b in zip(A[i], A[r])]
            piv.append(col)
            r += 1
        if r < 7:
            return []
        free = [c for c in range(9) if c not in piv]
        N = []
        for fc in free:
            v = [mp.mpf(0)] * 9
            v[fc] = mp.mpf(1)
            for i, pc in enumerate(piv):
                v[pc] = -A[i][fc]
            N.append([v[0:3], v[3:6], v[6:9]])

        # every model is N1 + mu N2 or mu N1 + N2 with |mu| <= 1: the roots of both cubics inside the unit disc
        models = []
        for P, Q in ((N[0], N[1]), (N[1], N[0])):
            def pencil(mu):
                return mp.matrix([[P[i][j] + mu * Q[i][j] for j in range(3)] for i in range(3)])
            dv = [mp.det(pencil(mp.mpf(m))) for m in (0, 1, -1, 2)]
            c0 = dv[0]
            c2 = (dv[1] + dv[2]) / 2 - c0
            s = (dv[1] - dv[2]) / 2
            c3 = (dv[3] - 4 * c2 - c0 - 2 * s) / 6
            c1 = s - c3
            cs = [c3, c2, c1, c0]
            while cs and abs(cs[0]) <= mp.mpf(10) ** -40 * max(abs(v) for v in cs):
                cs = cs[1:]
            for z in (mp.polyroots(cs, maxsteps=400, extraprec=400) if len(cs) > 1 else []):
                z = mp.mpc(z)
                if abs(z) <= 1 + 1e-9 and (abs(z.imag) <= mp.mpf(10) ** -25 or (abs(z.imag) <= 1e-6 and z.imag > 0)):
                    M = np.array([[float(P[i][j] + z.real * Q[i][j]) for j in range(3)] for i in range(3)])
                    if all(np.abs(_canon(M) - G).max() > 1e-12 for G in models):
                        models.append(_canon(M))
        return models


def compare_model_sets(got, ref):
    """Largest distance (unit norm, sign fixed) from each model of one set to the nearest of the other, both ways."""
    got = [_canon(F) for F in got]
    assert len(got) > 0 and len(ref) > 0
    d1 = max(min(np.abs(F - G).max() for G in ref) for F in got)
    d2 = max(min(np.abs(F - G).max() for G in got) for F in ref)
    return max(d1, d2)


def _normalised_sample(x1, x2, idx):
    T1, T2 = eo.hartley_normalisation(x1), eo.hartley_normalisation(x2)
    h1 = (T1 @ np.vstack((x1, np.ones(x1.shape[1]))))[:2, idx]
    h2 = (T2 @ np.vstack((x2, np.ones(x2.shape[1]))))[:2, idx]
    return np.ascontiguousarray(np.vstack((h1, h2)).T)


SEVEN_TOL = 1e-8     # the issue's bar; measured worst 1.5e-14 (generic and collinear samples): a margin of ~7e5
SEVEN_TOL_DOUBLE = 1e-7   # a double root split by rounding the sample to double, known to ~sqrt(eps): measured 1.2e-8, margin 9


def test_seven_point_generic_and_collinear_against_mpmath(lib):
    x1, x2, _, _, _ = eo.synthetic_pair(400, sigma=0.5, outliers=0.3, seed=13)
    rng = np.random.default_rng(13)
    worst = 0.0
    for k in range(40):
        idx = rng.choice(400, 7, replace=False)
        xs = _normalised_sample(x1, x2, idx)
        if k % 4 == 3:                                           # three points collinear in view 1
            xs[2, :2] = xs[0, :2] + 0.37 * (xs[1, :2] - xs[0, :2])
            xs[3, :2] = xs[0, :2] - 1.21 * (xs[1, :2] - xs[0, :2])
        got, ref = seven_point_host(lib, xs), seven_point_reference(xs)
        assert len(got) == len(ref), (k, len(got), len(ref))
        worst = max(worst, compare_model_sets(got, ref))
    print('seven point: worst model difference', worst)
    assert worst <= SEVEN_TOL


def test_seven_point_rank_deficient_sample_has_no_model(lib):
    x1, x2, _, _, _ = eo.synthetic_pair(50, sigma=0.5, outliers=0.0, seed=14)
    xs = _normalised_sample(x1, x2, [0, 1, 2, 3, 4, 5, 6])
    xs[4] = xs[1]                                                # two identical pairs: rank 6
    assert seven_point_reference(xs) == []
    assert seven_point_host(lib, xs) == []
    assert eo.seven_point(xs[:, :2].T, xs[:, 2:].T) == []


def test_seven_point_double_root_sample(lib):
    """A sample whose exact cubic has a double root: the pencil F1 + mu F2 is tangent to det = 0 at F1 (rank 2, e2^T F2 e1 = 0),
    and x2 = (F1 x1) x (F2 x1) lies on both lines.  The kernel must return the double root's model."""
    rng = np.random.default_rng(15)
    worst = 0.0
    for trial in range(10):
        U, _, Vt = np.linalg.svd(rng.normal(size=(3, 3)))
        F1 = U @ np.diag([1.0, rng.uniform(0.3, 1.0), 0.0]) @ Vt
        e1, e2 = Vt[2], U[:, 2]
        F2 = rng.normal(size=(3, 3))
        F2 -= (e2 @ F2 @ e1) * np.outer(e2, e1)
        rows = []
        while len(rows) < 7:
            p = np.array([rng.uniform(-1.2, 1.2), rng.uniform(-1.2, 1.2), 1.0])
            q = np.cross(F1 @ p, F2 @ p)
            if abs(q[2]) > 0.3 and np.all(np.abs(q[:2] / q[2]) < 3):
                rows.append([p[0], p[1], q[0] / q[2], q[1] / q[2]])
        xs = np.ascontiguousarray(rows)
        got, ref = seven_point_host(lib, xs), seven_point_reference(xs)
        # F1 itself is the double root of the sample BEFORE rounding to double: measured 1.7e-7 away, a bar of 1e-6 (margin 6)
        assert min(np.abs(_canon(F) - _canon(F1)).max() for F in got) <= 1e-6, trial
        worst = max(worst, compare_model_sets(got, ref))
    print('seven point, double root: worst model difference', worst)
    assert worst <= SEVEN_TOL_DOUBLE
