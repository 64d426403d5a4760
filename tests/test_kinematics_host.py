"""Kinematics of the trajectory splines on the host (mvus_amd/csrc/spline_kin_math.h through tests/hostcheck/kin_hostcheck.cpp), the bindings of the
three calls, the ``ba_kinematics`` setting and the unit conversion of ``Scene.kinematics``.  No GPU.

Bars.  Derivatives: the error of a sample is taken relative to sum_a |B_a^(v)(t)| |c_a| (what the sum can lose to cancellation), the reference is de
Boor's recurrence restated here in np.longdouble, the bar 8 x the same error of scipy.interpolate.splev(der=v) on the same samples with a floor of
1e-12 -- the project's margin for another order of summation, and its floor.  State covariance: entries relative to sqrt(C_ii C_jj) against a dense
long-double B Sigma B^T, bar 8 x the loss of the fp64 einsum of the same product, floor 1e-12.  Length: scipy.integrate.quad of |splev'|
(epsrel 1e-13, the knots as break points), bar 1e-12 relative."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from mvus_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, 'hostcheck', 'kin_hostcheck.cpp')
DEPS = [SRC] + [os.path.join(ROOT, 'mvus_amd', 'csrc', f) for f in ('spline_kin_math.h', 'ba_math.h')]
SO = os.path.join(HERE, 'hostcheck', 'libkincheck.so')
_cached = None


def load_kincheck():
    """g++ build of kin_hostcheck.cpp (rebuilt when a source is newer), loaded once."""
    global _cached
    if _cached is not None:
        return _cached
    if (not os.path.exists(SO)) or os.path.getmtime(SO) < max(os.path.getmtime(d) for d in DEPS):
        subprocess.check_call(['g++', '-O2', '-std=c++17', '-ffp-contract=off', '-shared', '-fPIC', '-o', SO, SRC])
    lib = ctypes.CDLL(SO)
    dp = _lib.c_double_p
    lib.kincheck_basis.argtypes = [dp, ctypes.c_double, dp, dp, dp]
    lib.kincheck_basis_ref.argtypes = [dp, ctypes.c_double, dp, dp]
    lib.kincheck_eval_der.argtypes = [dp, ctypes.c_int, dp, ctypes.c_longlong, dp, ctypes.c_int, dp]
    lib.kincheck_state_cov.argtypes = [ctypes.c_int, dp, dp, dp]
    lib.kincheck_speed_std.argtypes = [dp, dp, ctypes.c_int]
    lib.kincheck_speed_std.restype = ctypes.c_double
    lib.kincheck_path_length.argtypes = [dp, ctypes.c_int, dp, ctypes.c_double, ctypes.c_double, ctypes.c_longlong, dp, dp]
    lib.kincheck_path_length.restype = ctypes.c_double
    _cached = lib
    return lib


# ---- references ---------------------------------------------------------------------------------------------------------------------
def span_of(knots, x):
    """find_span: l in [3, n - 1] with t[l] <= x < t[l + 1], clamped"""
    n = len(knots) - 4
    return int(np.clip(np.searchsorted(knots, x, side='right') - 1, 3, n - 1))


def deboor_ld(knots, l, x, nu):
    """B^(nu)_{l-3+a, 3}(x), a = 0..3, on span l by the Cox - de Boor recurrence and its derivative formula, in np.longdouble"""
    t = np.asarray(knots, dtype=np.longdouble)
    x = np.longdouble(x)
    zero = np.longdouble(0)

    def B(i, k, d):
        if k == 0:
            return np.longdouble(1) if (i == l and d == 0) else zero
        den1, den2 = t[i + k] - t[i], t[i + k + 1] - t[i + 1]
        if d == 0:
            a = (x - t[i]) / den1 * B(i, k - 1, 0) if den1 > 0 else zero
            b = (t[i + k + 1] - x) / den2 * B(i + 1, k - 1, 0) if den2 > 0 else zero
            return a + b
        a = B(i, k - 1, d - 1) / den1 if den1 > 0 else zero
        b = B(i + 1, k - 1, d - 1) / den2 if den2 > 0 else zero
        return np.longdouble(k) * (a - b)
    return np.array([B(l - 3 + a, 3, nu) for a in range(4)], dtype=np.longdouble)


def der_reference(knots, coefs, xs, nu):
    """(values[3, m] in long double, scale[3, m] = sum_a |B_a^(nu)| |c_a|)"""
    c = np.asarray(coefs, dtype=np.longdouble)
    val = np.zeros((3, len(xs)), dtype=np.longdouble)
    sc = np.zeros((3, len(xs)), dtype=np.longdouble)
    for i, x in enumerate(xs):
        l = span_of(knots, x)
        b = deboor_ld(knots, l, x, nu)
        val[:, i] = c[:, l - 3:l + 1] @ b
        sc[:, i] = np.abs(c[:, l - 3:l + 1]) @ np.abs(b)
    return val, sc


def der_bar(knots, coefs, xs, nu):
    """(reference, scale, bar): 8 x the error of scipy's splev(der=nu) on these samples, floor 1e-12"""
    from scipy.interpolate import splev
    ref, sc = der_reference(knots, coefs, xs, nu)
    sp = np.array(splev(xs, (np.asarray(knots), [np.asarray(c) for c in coefs], 3), der=nu))
    loss = float(np.max(np.abs(sp.astype(np.longdouble) - ref) / sc))
    return ref, sc, max(8.0 * loss, 1e-12)


def host_eval_der(knots, coefs, xs, nder=2):
    lib = load_kincheck()
    k = np.ascontiguousarray(knots, dtype=np.float64)
    c = np.ascontiguousarray(np.asarray(coefs, dtype=np.float64))
    x = np.ascontiguousarray(xs, dtype=np.float64)
    D = np.full((nder + 1, 3, x.size), np.nan)
    lib.kincheck_eval_der(_lib.dptr(k), k.size - 4, _lib.dptr(c), x.size, _lib.dptr(x), nder, _lib.dptr(D))
    return D


def host_basis(knots, x):
    """(h, dh, ddh) of spline_kin_math.h and (h, dh) of bspline_basis_w<true> on the span of x"""
    lib = load_kincheck()
    l = span_of(knots, x)
    tt = np.ascontiguousarray(np.asarray(knots, dtype=np.float64)[l - 2:l + 4])
    h, dh, ddh, h0, dh0 = (np.full(4, np.nan) for _ in range(5))
    lib.kincheck_basis(_lib.dptr(tt), float(x), _lib.dptr(h), _lib.dptr(dh), _lib.dptr(ddh))
    lib.kincheck_basis_ref(_lib.dptr(tt), float(x), _lib.dptr(h0), _lib.dptr(dh0))
    return h, dh, ddh, h0, dh0


def golden_splines():
    g = np.load(os.path.join(HERE, 'golden', 'traj_spline.npz'))
    return [(g['knots_%d' % i], g['coefs_%d' % i]) for i in range(int(g['n_int']))], g['interval'], g['t_query']


def spline_cases():
    """name -> (knots, coefs[3, n], samples): the issue's list"""
    rng = np.random.default_rng(17)
    out = {}
    for i, (k, c) in enumerate(golden_splines()[0]):
        inner = k[4:-4]
        out['golden_%d' % i] = (k, c, np.concatenate(([k[3]], inner, [k[-4]], rng.uniform(k[3], k[-4], 60))))
    k = np.array([0.0, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 1.0])
    out['single_span'] = (k, rng.standard_normal((3, 4)), np.concatenate(([0.0, 1.0], rng.uniform(0, 1, 20))))
    k = np.array([0.0, 0.0, 0.0, 0.0, 0.4, 1.0, 1.0, 1.0, 1.0])
    out['n5'] = (k, rng.standard_normal((3, 5)), np.concatenate(([0.0, 0.4, 1.0], rng.uniform(0, 1, 20))))
    steps = np.array([1.0, 1e-3, 1.0, 1e-3, 1e-3, 1.0, 1.0, 1e-3])              # spacings in ratio 1e3
    inner = np.cumsum(steps)
    k = np.concatenate((np.zeros(4), inner[:-1], np.full(4, inner[-1])))
    out['ratio_1e3'] = (k, rng.standard_normal((3, k.size - 4)), np.concatenate(([0.0], inner, rng.uniform(0, inner[-1], 40), inner[:-1] + 5e-4)))
    return out


CASES = spline_cases()


# ---- basis ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(CASES))
def test_values_and_first_derivatives_are_the_ba_basis_to_the_bit(name):
    knots, _, xs = CASES[name]
    for x in xs:
        h, dh, ddh, h0, dh0 = host_basis(knots, x)
        assert np.array_equal(h, h0) and np.array_equal(dh, dh0)
        assert np.isfinite(ddh).all()


@pytest.mark.parametrize('nu', [0, 1, 2])
@pytest.mark.parametrize('name', sorted(CASES))
def test_derivatives_against_long_double_de_boor(name, nu):
    knots, coefs, xs = CASES[name]
    ref, sc, bar = der_bar(knots, coefs, xs, nu)
    D = host_eval_der(knots, coefs, xs)
    worst = float(np.max(np.abs(D[nu].astype(np.longdouble) - ref) / sc))
    print('derivative %d on %s: worst %.3e, bar %.3e' % (nu, name, worst, bar))
    assert worst <= bar


def test_knot_conventions():
    """On an interior knot the derivatives come from the right, on the last knot from the left (splev(der=) does the same); the second
    derivative of a cubic spline is continuous, so both sides agree there to rounding, the third is not -- the span taken shows in ddh's slope."""
    from scipy.interpolate import splev
    knots, coefs, _ = CASES['n5']
    tck = (knots, list(coefs), 3)
    D = host_eval_der(knots, coefs, np.array([0.4, 1.0, 0.0]))
    for nu in (1, 2):
        want = np.array(splev(np.array([0.4, 1.0, 0.0]), tck, der=nu))
        assert np.allclose(D[nu], want, rtol=1e-12, atol=1e-12 * np.abs(coefs).max())
    eps = 1e-6
    right = (host_eval_der(knots, coefs, np.array([0.4 + eps]))[2] - D[2][:, :1]) / eps      # third derivative right of the knot
    third = np.array(splev(np.array([0.4 + eps / 2]), tck, der=3))
    assert np.allclose(right, third, rtol=1e-5)


# ---- state covariance -----------------------------------------------------------------------------------------------------------------
def random_spd_band(n, BW, seed):
    """SPD with half bandwidth BW: G^T G of a random upper-banded G plus a small ridge (the construction of test_covariance_host.random_spd_band)"""
    rng = np.random.default_rng(seed)
    G = np.triu(rng.standard_normal((n, n)))
    G[np.triu_indices(n, BW + 1)] = 0.0
    G[np.arange(n), np.arange(n)] += 0.5
    return G.T @ G + 1e-3 * np.eye(n)


def band_of(Sigma, N):
    band = np.zeros((N, 4, 3, 3))
    for p in range(N):
        for w in range(4):
            if p + w < N:
                band[p, w] = Sigma[3 * p:3 * p + 3, 3 * (p + w):3 * (p + w) + 3]
    return band


def state_matrix(H, p, N, dtype):
    """B[9, 3N]: row 3 i + r has H[i][a] at column 3 (p + a) + r"""
    B = np.zeros((9, 3 * N), dtype=dtype)
    for i in range(3):
        for a in range(4):
            for r in range(3):
                B[3 * i + r, 3 * (p + a) + r] = H[i][a]
    return B


def state_cov_reference(H, p, Sigma):
    """(long-double B Sigma B^T, bar) for one sample: 8 x the loss of the fp64 einsum of the same product, floor 1e-12"""
    N = Sigma.shape[0] // 3
    Bl = state_matrix(H, p, N, np.longdouble)
    ref = Bl @ Sigma.astype(np.longdouble) @ Bl.T
    B = state_matrix(H, p, N, np.float64)
    got64 = np.einsum('ik,kl,jl->ij', B, Sigma, B)
    sd = np.sqrt(np.diag(ref))
    loss = float(np.max(np.abs(got64.astype(np.longdouble) - ref) / np.outer(sd, sd)))
    return ref, max(8.0 * loss, 1e-12)


def host_state_cov(H, bp, nder=2):
    lib = load_kincheck()
    D = 3 * (nder + 1)
    out = np.full((D, D), np.nan)
    Hc = np.ascontiguousarray(np.asarray(H, dtype=np.float64))
    b = np.ascontiguousarray(bp, dtype=np.float64)
    lib.kincheck_state_cov(nder, _lib.dptr(Hc), _lib.dptr(b), _lib.dptr(out))
    return out


def test_state_covariance_against_dense_long_double():
    knots, _, xs = CASES['ratio_1e3']
    N = knots.size - 4
    Sigma = random_spd_band(3 * N, 11, seed=23)
    assert not np.triu(Sigma, 12).any()
    band = np.concatenate((band_of(Sigma, N), np.zeros((4, 4, 3, 3))))          # (room behind the last control point)
    worst_all = 0.0
    for x in xs:
        l = span_of(knots, x)
        h, dh, ddh, _, _ = host_basis(knots, x)
        H = [h, dh, ddh]
        ref, bar = state_cov_reference(H, l - 3, Sigma)
        got = host_state_cov(H, band[l - 3:l + 1].ravel())
        sd = np.sqrt(np.diag(ref))
        worst = float(np.max(np.abs(got.astype(np.longdouble) - ref) / np.outer(sd, sd)))
        worst_all = max(worst_all, worst / bar)
        assert worst <= bar, (x, worst, bar)
        assert np.array_equal(got, got.T)
        assert np.linalg.eigvalsh(got).min() >= -bar * np.trace(got)
        for nder in (0, 1):                                                     # the smaller states are the leading blocks
            D = 3 * (nder + 1)
            assert np.array_equal(host_state_cov(H, band[l - 3:l + 1].ravel(), nder), got[:D, :D])
    print('state covariance: worst / bar %.3f' % worst_all)


def test_state_covariance_of_unit_sigma():
    """Sigma = I: Cov(X') = sum_a dh_a^2 I, to the bit (the products are summed in the order of a)"""
    knots, _, xs = CASES['golden_0']
    band = np.zeros((4, 4, 3, 3))
    band[:, 0] = np.eye(3)
    for x in xs[:20]:
        h, dh, ddh, _, _ = host_basis(knots, x)
        got = host_state_cov([h, dh, ddh], band.ravel())
        acc = 0.0
        for a in range(4):
            acc += dh[a] * dh[a] * 1.0
        assert np.array_equal(got[3:6, 3:6], acc * np.eye(3))


def test_speed_std():
    lib = load_kincheck()
    rng = np.random.default_rng(3)
    A = rng.standard_normal((9, 9))
    C = np.ascontiguousarray(A @ A.T)
    v = np.array([0.3, -2.0, 1.1])
    got = lib.kincheck_speed_std(_lib.dptr(v), ctypes.cast(C.ctypes.data + 8 * (3 * 9 + 3), _lib.c_double_p), 9)      # the block inside the 9 x 9
    u = v / np.linalg.norm(v)
    assert abs(got - np.sqrt(u @ C[3:6, 3:6] @ u)) <= 1e-14 * got
    z = np.zeros(3)
    assert np.isnan(lib.kincheck_speed_std(_lib.dptr(z), _lib.dptr(np.ascontiguousarray(C[3:6, 3:6])), 3))


# ---- length ---------------------------------------------------------------------------------------------------------------------------
def quad_length(knots, coefs, a, b):
    """int_a^b |X'| by scipy.integrate.quad, the knots inside (a, b) as break points"""
    from scipy.integrate import quad
    from scipy.interpolate import splev
    tck = (np.asarray(knots), [np.asarray(c) for c in coefs], 3)
    if not b > a:
        return 0.0
    pts = [k for k in np.unique(knots) if a < k < b]
    val, _ = quad(lambda x: float(np.linalg.norm(splev(x, tck, der=1))), a, b, points=pts or None, epsabs=0.0, epsrel=1e-13, limit=50 * (len(pts) + 2))
    return val


def host_path_length(knots, coefs, lo, hi, xs):
    lib = load_kincheck()
    k = np.ascontiguousarray(knots, dtype=np.float64)
    c = np.ascontiguousarray(np.asarray(coefs, dtype=np.float64))
    x = np.ascontiguousarray(xs, dtype=np.float64)
    dist = np.full(x.size, np.nan)
    total = lib.kincheck_path_length(_lib.dptr(k), k.size - 4, _lib.dptr(c), float(lo), float(hi), x.size, _lib.dptr(x), _lib.dptr(dist))
    return dist, total


def quad_dist(knots, coefs, lo, hi, xs):
    """(dist at xs, total) of [lo, hi] from quad: every knot span integrated once and summed in order, then the part of each sample's own span"""
    ks = np.unique(np.concatenate(([lo], [k for k in knots if lo < k < hi], [hi])))
    full = np.array([quad_length(knots, coefs, a, b) for a, b in zip(ks[:-1], ks[1:])])
    before = np.concatenate(([0.0], np.cumsum(full)))
    out = np.zeros(len(xs))
    for i, x in enumerate(xs):
        j = int(np.clip(np.searchsorted(ks, x, side='right') - 1, 0, ks.size - 2))
        out[i] = before[j] + quad_length(knots, coefs, ks[j], min(x, hi))
    return out, float(before[-1])


def rel_len_err(got, want):
    """max |got - want| / want over the entries with want > 0 (the others must be exactly 0)"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert not got[want == 0].any()
    pos = want > 0
    return float(np.max(np.abs(got[pos] - want[pos]) / want[pos])) if pos.any() else 0.0


@pytest.mark.parametrize('i', [0, 1])
def test_length_against_quad_on_the_golden_splines(i):
    splines, interval, tq = golden_splines()
    knots, coefs = splines[i]
    lo, hi = interval[0, i], interval[1, i]
    xs = np.concatenate(([lo, hi], knots[4:-4:7], tq[(tq > lo) & (tq < hi)]))
    dist, total = host_path_length(knots, coefs, lo, hi, xs)
    want, want_total = quad_dist(knots, coefs, lo, hi, xs)
    assert abs(want_total - quad_length(knots, coefs, lo, hi)) <= 1e-12 * want_total          # (the span-wise reference against one quad over all)
    worst = max(rel_len_err(dist, want), abs(total - want_total) / want_total)
    print('length of golden spline %d: %.12g, %d samples, worst relative error %.3e (bar 1e-12)' % (i, total, xs.size, worst))
    assert worst <= 1e-12
    assert dist[0] == 0.0 and dist[1] == total


def test_length_of_a_straight_line_at_constant_speed():
    knots = np.concatenate((np.full(4, 2.0), [2.5, 4.0, 4.25, 7.0], np.full(4, 9.0)))
    n = knots.size - 4
    grev = np.array([knots[j + 1:j + 4].sum() / 3.0 for j in range(n)])
    P0, V = np.array([1.0, -2.0, 30.0]), np.array([0.3, 0.4, 1.2])                 # |V| = 1.3
    coefs = P0[:, None] + V[:, None] * grev[None, :]
    xs = np.array([2.0, 3.1, 4.0, 6.5, 9.0])
    dist, total = host_path_length(knots, coefs, 2.0, 9.0, xs)
    speed = float(np.sqrt(V @ V))
    for x, d in zip(list(xs) + [9.0], list(dist) + [total]):
        want = speed * (x - 2.0)
        assert abs(d - want) <= 8 * np.spacing(want), (x, d, want)


def test_length_inside_a_narrower_interval():
    """The interval may be narrower than the knots: only the part inside counts, and the start of the interval is exactly 0"""
    splines, _, _ = golden_splines()
    knots, coefs = splines[0]
    lo, hi = knots[3] + 12.3, knots[-4] - 7.7
    dist, total = host_path_length(knots, coefs, lo, hi, np.array([lo, 0.5 * (lo + hi), hi]))
    assert dist[0] == 0.0 and dist[2] == total
    assert abs(total - quad_length(knots, coefs, lo, hi)) <= 1e-12 * total
    assert abs(dist[1] - quad_length(knots, coefs, lo, 0.5 * (lo + hi))) <= 1e-12 * dist[1]


# ---- bindings and settings --------------------------------------------------------------------------------------------------------------
NAMES = ('mvus_spline_eval_der', 'mvus_spline_kin_cov_eval', 'mvus_spline_length')


def test_the_three_calls_are_bound_declared_and_exported():
    import __graft_entry__ as ge
    ge.build()
    bound = [a[0] for a in _lib.API]
    header = open(os.path.join(ROOT, 'include', 'mvus_ba.h')).read()
    lib = _lib.load()
    for name in NAMES:
        assert name in bound and ('int %s(int32_t device, int32_t S,' % name) in header and hasattr(lib, name)
    z = np.zeros(12)
    assert lib.mvus_spline_eval_der(0, 0, _lib.dptr(z), None, _lib.dptr(z), _lib.dptr(z), 0, None, 2, None, None) == _lib.MVUS_E_INVALID
    assert lib.mvus_last_error(None) == b'spline_eval_der: bad arguments'
    koff = np.array([0, 8], np.int64)
    which = np.zeros(1, np.int32)
    for nder in (3, -1):                                       # refused before any device call
        rc = lib.mvus_spline_eval_der(0, 1, _lib.dptr(z), koff.ctypes.data_as(_lib.c_int64_p), _lib.dptr(z), _lib.dptr(z), 1, _lib.dptr(z), nder, _lib.dptr(z),
                                      which.ctypes.data_as(_lib.c_int32_p))
        assert rc == _lib.MVUS_E_INVALID and b'nder' in lib.mvus_last_error(None)


@pytest.mark.parametrize('bad', [1, 0, 'true', None, 1.0])
def test_ba_kinematics_setting_must_be_a_bool(bad):
    from mvus_amd.reconstruction import common
    s = common.Scene()
    s.settings = {'opt_calib': False, 'ba_kinematics': bad}
    with pytest.raises(ValueError, match='ba_kinematics'):
        s.ba_kinematics_enabled()
    with pytest.raises(ValueError, match='ba_kinematics'):
        s.ba_mode()


def test_ba_kinematics_setting_default_and_values():
    from mvus_amd.reconstruction import common
    s = common.Scene()
    s.settings = {'opt_calib': False}
    assert s.ba_kinematics_enabled() is False
    s.settings['ba_kinematics'] = True
    assert s.ba_kinematics_enabled() is True
    s.settings['ba_kinematics'] = False
    assert s.ba_kinematics_enabled() is False


def test_scene_kinematics_units(monkeypatch):
    """fps 30 against fps 1 with the three spline calls replaced by fixed arrays: velocity x 30, acceleration x 900, the covariance blocks
    by the matching products, distances untouched and continued over the intervals"""
    from mvus_amd import spline
    from mvus_amd.reconstruction import common
    rng = np.random.default_rng(8)
    nt = 6
    which = np.array([0, 0, -1, 1, 1, -1], dtype=np.int32)
    D = rng.standard_normal((3, 3, nt))
    D[:, :, which < 0] = 0.0
    A = rng.standard_normal((nt, 9, 9))
    cov = A @ A.transpose(0, 2, 1)
    cov[which < 0] = np.nan
    dist = np.array([0.0, 2.5, 0.0, 0.0, 1.5, 0.0])
    total = np.array([4.0, 3.0])
    seen = {}
    monkeypatch.setattr(spline, 'evaluate_der', lambda tck, iv, t, nder=2, device=0: (D.copy(), which.copy()))
    monkeypatch.setattr(spline, 'path_length', lambda tck, iv, t, device=0: (dist.copy(), which.copy(), total.copy()))

    def fake_cov(tck, iv, band, t, nder=2, device=0):
        seen['band'] = band
        return cov.copy(), which.copy()
    monkeypatch.setattr(spline, 'kin_cov_evaluate', fake_cov)
    s = common.Scene()
    s.settings = {'opt_calib': False}
    s.addCamera(common.Camera(fps=30.0))
    s.spline = {'tck': [], 'int': np.zeros((2, 2))}
    s.traj = np.vstack((np.arange(nt, dtype=float), np.zeros((3, nt))))
    band = np.zeros((5, 4, 3, 3))
    assert 'kinematics' not in vars(s)
    per_s = s.kinematics(cov={'band': band})
    assert vars(s)['kinematics'] is per_s and seen['band'].shape == band.shape and per_s['fps'] == 30.0
    per_f = common.Scene.kinematics(s, fps=1, cov=band)
    assert set(per_s) == {'t', 'which', 'fps', 'pos', 'vel', 'acc', 'speed', 'dist', 'length', 'state_cov', 'vel_std', 'acc_std', 'speed_std'}
    assert set(common.Scene.kinematics(s, fps=1)) == set(per_s) - {'state_cov', 'vel_std', 'acc_std', 'speed_std'}
    inn = which >= 0
    assert np.array_equal(per_f['pos'], D[0]) and np.array_equal(per_f['vel'], D[1]) and np.array_equal(per_f['acc'], D[2])
    assert np.array_equal(per_s['pos'], D[0]) and np.array_equal(per_s['vel'], 30.0 * D[1]) and np.array_equal(per_s['acc'], 900.0 * D[2])
    assert np.allclose(per_s['speed'], 30.0 * per_f['speed'], rtol=1e-15) and np.array_equal(per_f['speed'], np.sqrt((D[1] ** 2).sum(axis=0)))
    assert np.array_equal(per_f['state_cov'][inn], cov[inn])
    unit = np.repeat([1.0, 30.0, 900.0], 3)
    assert np.array_equal(per_s['state_cov'][inn], cov[inn] * np.outer(unit, unit))
    assert np.allclose(per_s['vel_std'][inn], 30.0 * per_f['vel_std'][inn], rtol=1e-15)
    assert np.allclose(per_s['acc_std'][inn], 900.0 * per_f['acc_std'][inn], rtol=1e-15)
    assert np.allclose(per_s['speed_std'][inn], 30.0 * per_f['speed_std'][inn], rtol=1e-14)
    assert np.array_equal(per_f['vel_std'][inn], np.sqrt(np.einsum('tii->ti', cov[inn])[:, 3:6]))
    assert np.isnan(per_s['speed_std'][~inn]).all() and np.isnan(per_s['vel_std'][~inn]).all()
    for out in (per_s, per_f):
        assert np.array_equal(out['dist'], [0.0, 2.5, 0.0, 4.0, 5.5, 0.0]) and np.array_equal(out['length'], total)
        assert np.array_equal(out['t'], s.traj[0]) and np.array_equal(out['which'], which)
