"""CPU tests of the iterative time-shift search (csrc/sync_iter_math.h, tests/sync_iter_oracle.py): the lane routines in their host
build (g++, next to tests/sync_iter_hostcheck.cpp) against the oracle, the conditions the GPU tests put on their inputs, the figures
their bounds come from, and the oracle's own full search.  No GPU."""
import os
import sys

import numpy as np
import pytest
from scipy import interpolate

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import sync_iter_cases as cases                            # noqa: E402
import sync_iter_hostcheck_util as hc                      # noqa: E402
import sync_iter_oracle as so                              # noqa: E402


def test_sampler_equals_the_python_sampler():
    for seed, rnd, sign, n in ((0, 0, 0, 1600), (0, 3, 1, 1590), (12345678901234567, 17, 1, 9), (7, 0, 0, 10)):
        for h in (0, 1, 49, 199):
            idx = hc.sample9(seed, rnd, sign, h, n)
            assert idx == so.sample9(seed, rnd, sign, h, n)
            assert len(set(idx)) == 9 and 0 <= min(idx) and max(idx) < n
    # the draw depends on every argument
    assert len({tuple(hc.sample9(*a)) for a in ((0, 0, 0, 0, 1600), (1, 0, 0, 0, 1600), (0, 1, 0, 0, 1600), (0, 0, 1, 0, 1600), (0, 0, 0, 1, 1600))}) == 5


def test_spline_matches_splev_inside_and_beyond_the_knots():
    p = cases.prep()
    t2 = p['t2']
    u = np.concatenate((t2[:5] - 4.0, t2[:5] - 0.5, t2[::97] + 0.37, t2[-5:] + 3.0, [t2[0], t2[-1]]))
    ref = np.asarray(interpolate.splev(u, p['tck2']))            # ext = 0: the end polynomials extended
    got = hc.spline(p['tck2'], u)
    # both run FITPACK's recurrence with one rounding per operation: the same bits where scipy's build does not fuse operations (as
    # measured here); the bound allows a build that does -- a few ulp of the pixel coordinates (~1e3), amplified by the extension
    print('max |spline - splev| = %.3g' % np.max(np.abs(got - ref)))
    assert np.max(np.abs(got - ref)) <= 1e-9
    knots, n = np.asarray(p['tck2'][0]), len(p['tck2'][1][0])
    for x in np.concatenate((u, knots[3:n + 1][::53], [knots[3] - 10.0, knots[n] + 10.0, np.nan])):
        assert hc.span(knots, n, x, 1) == hc.span(knots, n, x, 0)


@pytest.mark.parametrize('d', cases.STEPS)
def test_pencil_eigenvalues_and_F_on_the_host(d):
    """si_pencil_betas against scipy's QZ to c eps kappa, si_fundamental9 against the oracle's fit to 8 x the oracle's own loss."""
    worst_b, worst_f = 0.0, 0.0
    for ref in cases.reference(d):
        s1, s2, ds = ref['samples']
        got = hc.betas(s1, s2, ds)
        if ref['settled']:
            assert len(got) == len(ref['betas'])
            if len(got):
                worst_b = max(worst_b, float(np.max(np.abs(got - ref['betas']) / (so.EPS * ref['kappa']))))
        for b in got:
            F = hc.fundamental(s1, s2 + b * ds)
            assert F is not None and abs(np.linalg.norm(F) - 1.0) < 1e-12 and F[2, 2] >= 0.0
            worst_f = max(worst_f, float(np.max(np.abs(F - so.fit_F(s1, s2 + b * ds)))))
    print('d = %d: worst |beta - beta_scipy| = %.3g eps kappa (bound %.3g), worst |F - F_oracle| = %.3g (bound %.3g)'
          % (d, worst_b, cases.C_BETA, worst_f, cases.F_BAR))
    assert worst_b <= cases.C_BETA
    assert worst_f <= cases.F_BAR


def test_sampson_error_and_interval_test():
    p = cases.prep()
    ref = cases.reference(1)[0]
    s1, s2, ds = ref['samples']
    F = so.fit_F(s1, s2 + ref['betas'][0] * ds)
    x1, x2 = p['d1'][1:3, 100:140], np.asarray(interpolate.splev(p['t2'][90:130] + 0.3, p['tck2']))
    want = so.sampson(F, x1, x2)
    got = np.array([hc.sampson(F, x1[0, k], x1[1, k], x2[0, k], x2[1, k]) for k in range(x1.shape[1])])
    assert np.all(np.abs(got - want) <= 1e-12 * np.abs(want))
    iv = np.array([[10.0, 60.0], [20.0, 65.5]])                     # [10, 20) and [60, 65.5)
    for tau, inside in ((10.0, True), (20.0, False), (19.999, True), (9.999, False), (40.0, False), (60.0, True), (65.5, False), (np.nan, False)):
        assert hc.in_intervals(iv, tau) == inside


def test_degenerate_samples_give_no_model():
    s1, s2, ds = (x.copy() for x in cases.reference(1)[0]['samples'])
    a, b, c = s1.copy(), s2.copy(), ds.copy()
    a[:, 1], b[:, 1], c[:, 1] = a[:, 0], b[:, 0], c[:, 0]         # a repeated sample: two equal rows
    assert len(hc.betas(a, b, c)) == 0
    a = s1.copy()
    a[0, 4] = np.nan
    assert len(hc.betas(a, s2, ds)) == 0
    a = s1.copy()
    a[1] = 2.0 * a[0] + 5.0                                        # collinear s1
    assert len(hc.betas(a, s2, ds)) == 0
    assert hc.fundamental(np.ones((2, 9)), s2) is None             # coinciding points
    x = s2.copy()
    x[1, 3] = np.inf
    assert hc.fundamental(s1, x) is None


def test_real_eigenvalues_of_a_matrix():
    rng = np.random.default_rng(3)
    for _ in range(100):
        A = rng.normal(size=(6, 6))
        w = np.linalg.eigvals(A)
        ref = np.sort(w.real[w.imag == 0.0])
        got = hc.eig6(A)
        assert got is not None and len(got) == len(ref)
        if len(ref):
            assert np.max(np.abs(got - ref)) <= 1e-10


def test_inputs_are_settled():
    """Conditions (a) and (b) on the test's hypotheses and models, on the oracle alone: at least 95 % settled."""
    p = cases.prep()
    nh = ns = nm = nms = 0
    for d in cases.STEPS:
        for ref in cases.reference(d):
            nh += 1
            ns += bool(ref['settled'])
            s1, s2, ds = ref['samples']
            for b in ref['betas']:
                nm += 1
                nms += bool(so.settled_model(p, p['beta_prior'], so.fit_F(s1, s2 + b * ds), b * d, cases.THRESHOLD))
    print('settled hypotheses %d / %d, settled models %d / %d' % (ns, nh, nms, nm))
    assert ns >= 0.95 * nh and nms >= 0.95 * nm


def test_scipy_loss_against_50_digit_roots():
    """Where C_BETA comes from: scipy's eigenvalues against the roots of det(A1 + beta A2) in 50-digit arithmetic, in eps kappa.  A part of
    the hypotheses (the recorded figure is the maximum over all of them)."""
    import mpmath as mp
    mp.mp.dps = 50
    worst = 0.0
    for d in cases.STEPS:
        for ref in cases.reference(d)[:6]:
            M1, M2 = mp.matrix(ref['A1'].tolist()), mp.matrix(ref['A2'].tolist())
            for b, k in zip(ref['betas'], ref['kappa']):
                r = mp.findroot(lambda x: mp.det(M1 + x * M2), mp.mpf(float(b)), tol=1e-40, maxsteps=60)
                worst = max(worst, float(abs(r - b)) / (so.EPS * k))
    print('scipy loses up to %.3g eps kappa on these (recorded maximum over all: %.4g)' % (worst, cases.SCIPY_LOSS))
    assert 0.0 < worst <= cases.SCIPY_LOSS


@pytest.mark.parametrize('moved', cases.MOVES)
def test_oracle_full_search(moved):
    """The oracle's search with the library's sampler; its error against the true beta is what ORACLE_BETA_ERROR records and what the
    GPU's end-to-end bar is twice of."""
    a = cases.pair(moved)
    beta, ratio = so.sync_iter(*a[:6], maxIter=cases.H, seed=cases.SEED)
    err = float(beta) - a[6]
    print('moved %+g frames: beta %.6f, truth %.6f, error %+.4f frames, inlier ratio %.4f' % (moved, beta, a[6], err, ratio))
    assert abs(err - cases.ORACLE_BETA_ERROR[moved]) <= 5e-4
    assert abs(err) <= 1.0 and ratio > 0.9


def test_gap_case_has_two_intervals():
    d2g, p = cases.gap_case()
    iv = p['intervals']
    assert iv.shape == (2, 2)
    assert iv[0, 1] - iv[1, 0] >= 40.0 - 1e-9                       # the hole between them
    assert d2g[0, -1] > iv[1, 1]                                    # the short run at the end is no interval
