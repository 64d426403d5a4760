"""Row routines of the covariance chain on the host (mvus_amd/csrc/ba_cov_math.h through tests/hostcheck/cov_hostcheck.cpp), the sample
formula of mvus_spline_cov_eval and the ``ba_covariance`` setting.  No GPU.

Bars: a result is compared with a long-double-refined inverse X <- X + X (I - H X) (four sweeps in np.longdouble from numpy's own
inverse), relative to sqrt(Sigma_ii Sigma_jj); the bar is 8 x the loss of numpy.linalg.inv (LAPACK, fp64) against that same reference on
that same matrix -- 8 x being the project's margin for a different order of summation -- with a floor of 1e-12."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from mvus_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, 'hostcheck', 'cov_hostcheck.cpp')
DEPS = [SRC] + [os.path.join(ROOT, 'mvus_amd', 'csrc', f) for f in ('ba_cov_math.h', 'ba_math.h')]
SO = os.path.join(HERE, 'hostcheck', 'libcovcheck.so')
_cached = None


def load_covcheck():
    """g++ build of cov_hostcheck.cpp (rebuilt when a source is newer), loaded once."""
    global _cached
    if _cached is not None:
        return _cached
    if (not os.path.exists(SO)) or os.path.getmtime(SO) < max(os.path.getmtime(d) for d in DEPS):
        subprocess.check_call(['g++', '-O2', '-std=c++17', '-ffp-contract=off', '-shared', '-fPIC', '-o', SO, SRC])
    lib = ctypes.CDLL(SO)
    dp = _lib.c_double_p
    lib.covcheck_selinv.argtypes = [ctypes.c_int, ctypes.c_int, dp, dp]
    lib.covcheck_band_pivots.argtypes = [ctypes.c_int, ctypes.c_int, dp, dp]
    lib.covcheck_dense_inverse.argtypes = [ctypes.c_int, dp, dp, dp]
    lib.covcheck_sample.argtypes = [dp, dp, dp]
    _cached = lib
    return lib


def refined_inverse(H, sweeps=4):
    """numpy's inverse refined in long double: X <- X + X (I - H X).  Returns (refined as float64-rounded long double array, numpy's own)."""
    X0 = np.linalg.inv(H)
    Hl, X = H.astype(np.longdouble), X0.astype(np.longdouble)
    eye = np.eye(H.shape[0], dtype=np.longdouble)
    for _ in range(sweeps):
        X = X + X @ (eye - Hl @ X)
    return X, X0


def rel_err(A, ref, sd=None, mask=None):
    """max |A - ref| / sqrt(ref_ii ref_jj) over the entries of ``mask`` (default: all)."""
    ref = np.asarray(ref, dtype=np.longdouble)
    if sd is None:
        sd = np.sqrt(np.diag(ref))
    e = np.abs(np.asarray(A, dtype=np.longdouble) - ref) / np.outer(sd, sd)
    return float(np.max(e if mask is None else e[mask]))


def bar_for(H):
    """(reference inverse, bar) for matrix H: 8 x LAPACK's own loss, floor 1e-12."""
    ref, X0 = refined_inverse(H)
    return ref, max(8.0 * rel_err(X0, ref), 1e-12)


def band_blocks_of(full, n):
    """[ceil(n / 3)][4][3][3] blocks (p, p + w) of a dense n x n matrix, zero outside it."""
    N = (n + 2) // 3
    pad = np.zeros((3 * N + 9, 3 * N + 9), dtype=full.dtype)
    pad[:n, :n] = full
    out = np.zeros((N, 4, 3, 3), dtype=full.dtype)
    for p in range(N):
        for w in range(4):
            out[p, w] = pad[3 * p:3 * p + 3, 3 * (p + w):3 * (p + w) + 3]
    return out


def band_mask(n):
    """entries (i, j) of an n x n matrix that lie in the blocks (p, p + w), w <= 3, or their transposes"""
    i, j = np.indices((n, n))
    return np.abs(i // 3 - j // 3) <= 3


def random_spd_band(n, BW, seed):
    """SPD with half bandwidth BW: G^T G of a random upper-banded G plus a small ridge -- conditioned like a spline block (1e3 .. 1e5)."""
    rng = np.random.default_rng(seed)
    G = np.triu(rng.standard_normal((n, n)))
    G[np.triu_indices(n, BW + 1)] = 0.0
    G[np.arange(n), np.arange(n)] += 0.5
    return G.T @ G + 1e-3 * np.eye(n)


def pack_factor(L, BW):
    n = L.shape[0]
    Lb = np.zeros((n, BW + 1))
    for j in range(BW + 1):
        Lb[j:, j] = np.diagonal(L, -j)
    return Lb


@pytest.mark.parametrize('n', [40, 41])
@pytest.mark.parametrize('BW', [11, 17, 47])
def test_selected_inverse_of_a_band(n, BW):
    lib = load_covcheck()
    BWe = min(BW, n - 1)
    H = random_spd_band(n, BWe, seed=100 * n + BW)
    assert not np.triu(H, BWe + 1).any()
    ref, bar = bar_for(H)
    Lb = np.ascontiguousarray(pack_factor(np.linalg.cholesky(H), BW))
    out = np.full(((n + 2) // 3, 4, 3, 3), np.nan)
    lib.covcheck_selinv(n, BW, _lib.dptr(Lb), _lib.dptr(out))
    want = band_blocks_of(ref, n)
    sd = np.sqrt(np.concatenate((np.diag(ref), np.ones(12, dtype=np.longdouble))))
    N = (n + 2) // 3
    worst = 0.0
    for p in range(N):
        for w in range(4):
            sc = np.outer(sd[3 * p:3 * p + 3], sd[3 * (p + w):3 * (p + w) + 3])
            worst = max(worst, float(np.max(np.abs(out[p, w].astype(np.longdouble) - want[p, w]) / sc)))
    print('selected inverse n=%d BW=%d: worst %.3e, bar %.3e' % (n, BW, worst, bar))
    assert worst <= bar
    # outside the matrix the blocks are exactly zero, and the diagonal blocks are symmetric to the bit
    assert all(not out[p, w].any() for p in range(N) for w in range(4) if 3 * (p + w) >= n)
    assert all(np.array_equal(out[p, 0], out[p, 0].T) for p in range(N))
    hs = np.ascontiguousarray(np.diag(H).copy())
    assert lib.covcheck_band_pivots(n, BW, _lib.dptr(Lb), _lib.dptr(hs)) == -1


@pytest.mark.parametrize('n', [18, 27, 90, 180])
def test_dense_spd_inverse(n):
    lib = load_covcheck()
    rng = np.random.default_rng(n)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    H = (Q * np.logspace(0, -5, n)) @ Q.T                      # condition 1e5, like a reduced camera system
    H = 0.5 * (H + H.T)
    d = np.exp(rng.uniform(-3, 3, n))                          # raw, unscaled blocks: diagonal entries over six decades
    H = H * np.outer(d, d)
    ref, bar = bar_for(H)
    S = np.ascontiguousarray(np.tril(H) + np.triu(np.full((n, n), np.nan), 1))      # (the upper triangle is never read)
    X = np.full((n, n), np.nan)
    hc = np.ascontiguousarray(np.diag(H).copy())
    assert lib.covcheck_dense_inverse(n, _lib.dptr(S), _lib.dptr(hc), _lib.dptr(X)) == -1
    got = np.tril(X) + np.tril(X, -1).T                        # what k_cov_expand takes
    worst = rel_err(got, ref)
    print('dense inverse n=%d: worst %.3e, bar %.3e' % (n, worst, bar))
    assert worst <= bar


def test_refusal_rule_on_a_singular_matrix():
    """A matrix with a null vector (a free gauge) is refused by the relative pivot test; the same matrix made definite is not."""
    lib = load_covcheck()
    rng = np.random.default_rng(5)
    n = 40
    J = rng.standard_normal((60, n))
    J[:, -1] = J[:, :3] @ np.array([1.0, -2.0, 0.5])           # the last column depends on the first three
    H = J.T @ J
    hc = np.ascontiguousarray(np.diag(H).copy())
    S, X = np.ascontiguousarray(H.copy()), np.empty((n, n))
    assert lib.covcheck_dense_inverse(n, _lib.dptr(S), _lib.dptr(hc), _lib.dptr(X)) == n - 1
    S = np.ascontiguousarray(H + np.diag(1e-6 * np.diag(H)))
    assert lib.covcheck_dense_inverse(n, _lib.dptr(S), _lib.dptr(hc), _lib.dptr(X)) == -1


def test_sample_formula_against_b_sigma_bt():
    """Cov X(t) = sum h_a h_b Sigma(p + a, p + b) from the band equals B Sigma B^T with the basis values of mvus_amd.bspline."""
    from mvus_amd import bspline
    lib = load_covcheck()
    rng = np.random.default_rng(11)
    n = 9                                                      # control points
    knots = np.concatenate((np.zeros(3), np.linspace(0.0, 6.0, n - 2), np.full(3, 6.0)))
    A = rng.standard_normal((3 * n, 3 * n))
    Sigma = A @ A.T                                            # dense covariance in control-point order (x, y, z per point)
    band = np.ascontiguousarray(band_blocks_of(Sigma, 3 * n))
    for t in [0.0, 0.3, 1.0, 2.5, 5.999, 6.0]:
        l = int(np.clip(np.searchsorted(knots, t, side='right') - 1, 3, n - 1))
        h = np.array([bspline.evaluate(knots, np.eye(n)[l - 3 + a][None, :], np.array([t]))[0, 0] for a in range(4)])
        assert abs(h.sum() - 1.0) < 1e-13
        B = np.zeros((3, 3 * n))
        for a in range(4):
            B[:, 3 * (l - 3 + a):3 * (l - 3 + a) + 3] = h[a] * np.eye(3)
        want = B @ Sigma @ B.T
        got = np.empty(9)
        hh = np.ascontiguousarray(h)
        lib.covcheck_sample(_lib.dptr(hh), _lib.dptr(band[l - 3:].ravel().copy()), _lib.dptr(got))
        assert np.max(np.abs(got.reshape(3, 3) - want)) <= 1e-12 * np.max(np.abs(want))


def host_cov_samples(tck, interval, band, ts):
    """mvus_spline_cov_eval on the host: the formula of covcheck_sample with the basis values of mvus_amd.bspline; NaN outside every interval."""
    from mvus_amd import bspline
    lib = load_covcheck()
    band = np.ascontiguousarray(band, dtype=np.float64)
    out = np.full((len(ts), 3, 3), np.nan)
    off = np.concatenate(([0], np.cumsum([len(k[0]) - 4 for k in tck])))
    for i, t in enumerate(ts):
        for s in range(interval.shape[1]):
            if interval[0, s] <= t <= interval[1, s]:
                kn = np.asarray(tck[s][0], dtype=np.float64)
                n = kn.size - 4
                l = int(np.clip(np.searchsorted(kn, t, side='right') - 1, 3, n - 1))
                h = np.ascontiguousarray([bspline.evaluate(kn, np.eye(n)[l - 3 + a][None, :], np.array([t]))[0, 0] for a in range(4)])
                got = np.empty(9)
                lib.covcheck_sample(_lib.dptr(h), _lib.dptr(band[off[s] + l - 3:off[s] + l + 1].ravel().copy()), _lib.dptr(got))
                out[i] = got.reshape(3, 3)
    return out


@pytest.mark.parametrize('bad', [1, 0, 'true', None, 1.0])
def test_ba_covariance_setting_must_be_a_bool(bad):
    from mvus_amd.reconstruction import common
    s = common.Scene()
    s.settings = {'opt_calib': False, 'ba_covariance': bad}
    with pytest.raises(ValueError, match='ba_covariance'):
        s.ba_covariance_enabled()
    with pytest.raises(ValueError, match='ba_covariance'):
        s.ba_mode()


def test_ba_covariance_setting_default_and_values():
    from mvus_amd.reconstruction import common
    s = common.Scene()
    s.settings = {'opt_calib': False}
    assert s.ba_covariance_enabled() is False
    s.settings['ba_covariance'] = True
    assert s.ba_covariance_enabled() is True
    s.settings['ba_covariance'] = False
    assert s.ba_covariance_enabled() is False


def test_abi_declares_the_covariance_entry_points():
    names = [a[0] for a in _lib.API]
    assert 'mvus_ba_covariance' in names and 'mvus_spline_cov_eval' in names
    header = open(os.path.join(ROOT, 'include', 'mvus_ba.h')).read()
    assert 'int mvus_ba_covariance(mvus_ba* h, const double* x, double sigma2,' in header
