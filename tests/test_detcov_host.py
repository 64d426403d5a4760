"""Row routines of the per-detection covariance on the host (mvus_amd/csrc/ba_detcov_math.h through tests/detcov_hostcheck.cpp, the
source k_detcov compiles), the ellipse and chi^2 closed forms of ``Scene.ba_detection_covariance`` / ``studentised_flags``, the
``ba_detection_covariance`` setting and the two entry points' declarations.  No GPU.

Bar of the row routine: Pi = J_i Sigma J_i^T is compared with the dense form in long double, relative to sqrt(Pi_uu Pi_vv); the bar is
8 x the loss of the same three-term split formed by numpy from the same fp64 blocks -- 8 x being the project's margin for a different
order of summation -- with a floor of 1e-12.  The split cancels, which is why the bar is taken in the split and not from eps."""
import os

import numpy as np
import pytest

import detcov_hostcheck_util as dh
from test_covariance_host import band_blocks_of, refined_inverse
from mvus_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble


def _problem(CB, B, N, seed):
    """A problem of the BA's own shape: rows that touch one camera's B slots and four consecutive control points, each made orthogonal
    to one direction g inside its own support, H = G^T G + a small ridge, and its long-double inverse.  g is then a weakly determined
    direction that mixes cameras and trajectory, as the anchored gauge of a BA is: Sigma is dominated by g g^T / ridge, every term of
    the split carries it and J_i Sigma J_i^T, with J_i a row pair of G, does not -- the three terms cancel by four to five digits."""
    rng = np.random.default_rng(seed)
    n = CB + 3 * N
    g = rng.standard_normal(n)
    rows = []
    G = np.zeros((6 * n, n))
    for i in range(G.shape[0]):
        c, p = int(rng.integers(CB // B)), int(rng.integers(N - 3))
        sup = np.r_[c * B:(c + 1) * B, CB + 3 * p:CB + 3 * p + 12]
        v = rng.standard_normal(sup.size)
        G[i, sup] = v - (v @ g[sup]) / (g[sup] @ g[sup]) * g[sup]
        rows.append((c, p))
    H = G.T @ G
    Sigma, _ = refined_inverse(H + 1e-5 * np.mean(np.diag(H)) * np.eye(n))
    return rng, G, rows, Sigma


def _rel(P, ref):
    ref = np.asarray(ref, dtype=LD)
    return float(np.max(np.abs(np.asarray(P, dtype=LD) - ref) / np.sqrt(ref[0] * ref[2])))


@pytest.mark.parametrize('CB,B', [(9, 9), (36, 9), (36, 18), (180, 9), (180, 18)])
def test_row_routine_against_dense_long_double(CB, B):
    N = 9
    rng, Grows, rows, Sigma = _problem(CB, B, N, 100 * CB + B)
    S64 = Sigma.astype(np.float64)
    Scc_full, T_full, G_full = S64[:CB, :CB], -S64[CB:, :CB], S64[CB:, CB:]         # Sigma_sc = -T
    band = band_blocks_of(G_full, 3 * N)
    worst = bar = 0.0
    cancel = 0.0
    for _ in range(12):
        i, k = (int(q) for q in rng.integers(len(rows), size=2))
        while rows[k] != rows[i]:                                                   # two rows of one camera and one span: a detection
            k = (k + 1) % len(rows)
        c, p = rows[i]
        a, b = Grows[[i, k], c * B:(c + 1) * B].copy(), Grows[[i, k], CB + 3 * p:CB + 3 * p + 12].copy()
        J = np.zeros((2, CB + 3 * N))
        J[:, c * B:(c + 1) * B] = a
        J[:, CB + 3 * p:CB + 3 * p + 12] = b
        dense = J.astype(LD) @ Sigma @ J.astype(LD).T
        ref = np.array([dense[0, 0], dense[0, 1], dense[1, 1]])
        # the blocks the kernel reads, with their own leading dimensions: Sigma_cc[c, c] inside its CB-wide rows, the slice of T likewise
        Scc = Scc_full[c * B:(c + 1) * B, c * B:]
        T = T_full[3 * p:3 * p + 12, c * B:]
        pi, terms = dh.row(a, b, Scc, T, band[p:p + 4])
        # numpy's own three terms from the same fp64 blocks
        Sb, Tb, Gb = Scc[:, :B], T[:, :B], G_full[3 * p:3 * p + 12, 3 * p:3 * p + 12]
        x = a @ Tb.T @ b.T
        t1, t2, t3 = a @ Sb @ a.T, x + x.T, b @ Gb @ b.T
        mine = (t1 - t2) + t3
        loss = _rel([mine[0, 0], mine[0, 1], mine[1, 1]], ref)
        err = _rel(pi, ref)
        worst, bar = max(worst, err), max(bar, loss)
        cancel = max(cancel, float((abs(t1[0, 0]) + abs(t2[0, 0]) + abs(t3[0, 0])) / abs(mine[0, 0])))
        for k, t in enumerate((t1, t2, t3)):                                        # each term is the one the formula names
            want = np.array([t[0, 0], t[0, 1], t[1, 1]])
            assert np.max(np.abs(terms[k] - want)) <= 1e-12 * max(np.max(np.abs(want)), 1e-300)
    bar = max(8.0 * bar, 1e-12)
    print('detcov_row CB %d B %d: worst %.3e, bar %.3e, cancellation up to %.1e' % (CB, B, worst, bar, cancel))
    assert worst <= bar and cancel > 1e3


def test_t2_guard_and_value():
    rng = np.random.default_rng(5)
    for _ in range(20):
        A = rng.standard_normal((2, 2))
        Pi = 0.3 * (A @ A.T) / np.trace(A @ A.T)                                    # eigenvalues below sigma2 = 0.5
        r = np.abs(rng.standard_normal(2))
        want = float(r @ np.linalg.solve(0.5 * np.eye(2) - Pi, r))
        got = dh.t2([Pi[0, 0], Pi[0, 1], Pi[1, 1]], 0.5, r[0], r[1])
        assert abs(got - want) <= 1e-12 * abs(want)
    assert np.isnan(dh.t2([1.0, 0.0, 0.5], 1.0, 1.0, 1.0))                          # singular: q11 = 0
    assert np.isnan(dh.t2([0.5, 0.0, 1.0], 1.0, 1.0, 1.0))                          # singular: q22 = 0
    assert np.isnan(dh.t2([0.5, 0.5, 0.5], 1.0, 1.0, 1.0))                          # singular: det = 0
    assert np.isnan(dh.t2([0.5, 0.8, 0.5], 1.0, 1.0, 1.0))                          # indefinite
    assert np.isnan(dh.t2([2.0, 0.0, 2.0], 1.0, 1.0, 1.0))                          # negative definite: det > 0, q11 < 0
    assert np.isnan(dh.t2([np.nan, 0.0, 0.1], 1.0, 1.0, 1.0))
    assert dh.t2([0.0, 0.0, 0.0], 2.0, 3.0, 4.0) == 12.5                            # no leverage: |r|^2 / sigma2


def test_sign_convention_is_D_Pi_D():
    Pi = np.array([[2.0, 0.7], [0.7, 1.5]])
    for su in (1.0, -1.0):
        for sv in (1.0, -1.0):
            D = np.diag([su, sv])
            want = D @ Pi @ D
            got = dh.image_axes([2.0, 0.7, 1.5], su, sv)
            assert np.array_equal(got, [want[0, 0], want[0, 1], want[1, 1]])


def test_ellipse_closed_form_against_eigh():
    from mvus_amd.reconstruction.common import ellipse_2x2
    rng = np.random.default_rng(9)
    A = rng.standard_normal((200, 2, 2))
    P = A @ np.transpose(A, (0, 2, 1))
    P[0] = np.diag([4.0, 1.0]); P[1] = np.diag([1.0, 4.0]); P[2] = np.array([[1.0, 1.0], [1.0, 1.0]])      # axis-aligned, rank one
    major, minor, angle = ellipse_2x2(np.array([P[:, 0, 0], P[:, 0, 1], P[:, 1, 1]]))
    w, v = np.linalg.eigh(P)
    assert np.max(np.abs(major - np.sqrt(w[:, 1])) / np.sqrt(w[:, 1])) <= 1e-12
    assert np.max(np.abs(minor - np.sqrt(np.maximum(w[:, 0], 0.0)))) <= 1e-7 * np.max(major)      # (sqrt of a cancelled difference near rank one)
    d = np.stack((np.cos(angle), np.sin(angle)), axis=1)
    assert np.max(np.abs(np.abs(np.einsum('ni,ni->n', d, v[:, :, 1])) - 1.0)) <= 1e-12            # the major axis, up to its sign
    assert angle[0] == 0.0 and abs(angle[1]) == np.pi / 2 and abs(angle[2] - np.pi / 4) <= 1e-15 and minor[2] == 0.0
    assert np.all((angle > -np.pi / 2 - 1e-15) & (angle <= np.pi / 2))
    nan = ellipse_2x2(np.full((3, 2), np.nan))
    assert all(np.isnan(q).all() for q in nan)


def test_chi2_threshold_and_flags():
    from mvus_amd.reconstruction.common import Scene, chi2_2_quantile
    thr = chi2_2_quantile(0.999)
    assert abs(thr - 13.815510557964274) <= 1e-13 and abs((1.0 - np.exp(-0.5 * thr)) - 0.999) <= 1e-15
    assert chi2_2_quantile(0.0) == 0.0
    for bad in (1.0, -0.1, 1.5):
        with pytest.raises(ValueError):
            chi2_2_quantile(bad)
    t2 = np.array([0.0, thr, np.nextafter(thr, np.inf), 50.0, np.nan, np.inf])
    result = {'per_cam': {3: {'t2': t2.copy()}, 7: {'t2': np.array([np.nan])}}}
    flags = Scene.studentised_flags(result)
    assert list(flags) == [3, 7] and flags[3].dtype == bool
    assert flags[3].tolist() == [False, False, True, True, False, True] and flags[7].tolist() == [False]
    assert np.array_equal(result['per_cam'][3]['t2'], t2, equal_nan=True)          # it only flags
    assert Scene.studentised_flags(result, p=0.5)[3].tolist() == [False, True, True, True, False, True]


@pytest.mark.parametrize('bad', [1, 0, 'true', None, 1.0])
def test_setting_must_be_a_bool(bad):
    from mvus_amd.reconstruction import common
    s = common.Scene()
    s.settings = {'opt_calib': False, 'ba_detection_covariance': bad}
    with pytest.raises(ValueError, match='ba_detection_covariance'):
        s.ba_detection_covariance_enabled()
    with pytest.raises(ValueError, match='ba_detection_covariance'):
        s.ba_mode()


def test_setting_default_and_values():
    from mvus_amd.reconstruction import common
    s = common.Scene()
    s.settings = {'opt_calib': False}
    assert s.ba_detection_covariance_enabled() is False
    s.settings['ba_detection_covariance'] = True
    assert s.ba_detection_covariance_enabled() is True
    s.settings['ba_detection_covariance'] = False
    assert s.ba_detection_covariance_enabled() is False


def test_the_two_entry_points_are_declared_bound_and_exported():
    import __graft_entry__ as ge
    ge.build()
    header = open(os.path.join(ROOT, 'include', 'mvus_ba.h')).read()
    bound = {a[0]: a for a in _lib.API}
    lib = _lib.load()
    assert 'int mvus_ba_detection_covariance(mvus_ba* h, const double* x, double sigma2, double* e_out, double* pcov_out, double* t2_out, double* cov_cam,' in header
    assert 'int32_t mvus_ba_detection_covariance_ms(mvus_ba* h, double* ms_out);' in header
    for name in ('mvus_ba_detection_covariance', 'mvus_ba_detection_covariance_ms'):
        assert name in bound and hasattr(lib, name)
    assert len(bound['mvus_ba_detection_covariance'][2]) == 11 and len(bound['mvus_ba_detection_covariance_ms'][2]) == 2
    assert '#define MVUS_ABI_VERSION 8' in header and lib.mvus_abi_sizes(None, None, None) == 8
    # no handle: refused, nothing touched
    assert lib.mvus_ba_detection_covariance(None, None, 0.0, None, None, None, None, None, None, None, None) == _lib.MVUS_E_INVALID
    assert lib.mvus_ba_detection_covariance_ms(None, None) == _lib.MVUS_E_INVALID
