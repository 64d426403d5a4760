"""The yardsticks of tests/test_gpu_lsmr.py, checked without a GPU: the numpy LSMR of tests/lsmr_reference.py against scipy and against
50-digit arithmetic, the layouts of tests/lsmr_layouts.py against the branches they exist for, and the deviation of the host build of
Lsmr::run (hostcheck_lsmr: the solver's own code over the plain C++ backend) from the longdouble reference -- dev_host(layout, k), the
figure the GPU bars are multiples of."""
import numpy as np
import pytest
from scipy.sparse.linalg import lsmr as scipy_lsmr

import lsmr_layouts as L
import lsmr_reference as ref


def test_longdouble_is_wider_than_double():
    """The reference format has at least 63 mantissa bits (x87 extended: 63 + the explicit leading bit)."""
    assert np.finfo(np.longdouble).nmant >= 63


@pytest.mark.parametrize('damp', [0.0, L.DAMP])
def test_reference_in_fp64_reproduces_scipy(damp):
    """x and the norm estimates of scipy.sparse.linalg.lsmr(A, b, damp, atol=0, btol=0, conlim=0, maxiter=k), k = 1..4, on `plain` and on
    the scaled operator [J D; E] of `scaled`.  Same algorithm, same format; the statements differ in order (scipy updates in place), so
    the bar is a few roundings of the recurrence: 1e-12 relative (the restatement of ba_solver.h sits at 1e-15 after three iterations,
    test_solver_host.py)."""
    for name in ('plain', 'scaled'):
        hc = L.host_case(name)
        A64 = np.asarray(hc.A, dtype=np.float64)
        b = np.concatenate((hc.rhs['f'], np.zeros(A64.shape[0] - hc.h.m)))
        recs = ref.lsmr_iterates(A64, hc.rhs['f'], damp, max(L.KS), np.float64)
        for k in L.KS:
            x, istop, itn, normr, normar, normA, condA, normx = scipy_lsmr(A64, b, damp=damp, atol=0, btol=0, conlim=0, maxiter=k)[:8]
            r = recs[k - 1]
            assert (itn, istop) == (k, 7)
            assert np.linalg.norm(r.x - x) <= 1e-12 * np.linalg.norm(x)
            for got, want in ((r.normr, normr), (r.normar, normar), (r.normA, normA), (r.condA, condA), (r.normx, normx)):
                assert abs(got - want) <= 1e-12 * abs(want)


def test_longdouble_stands_in_for_50_digits():
    """On `plain` the longdouble reference agrees with the same statements run in mpmath at 50 digits to below 1e-3 of the host build's own
    deviation, k = 1..4: its error is invisible at the scale the GPU bars are set on."""
    import mpmath
    hc = L.host_case('plain')
    with mpmath.workdps(50):
        Amp = ref.dense_operator(hc.Jref, None, None, 'mp')
        mp_recs = ref.lsmr_iterates(Amp, hc.rhs['f'], 0.0, max(L.KS), 'mp')
        ld = L.reference('plain', 'f')
        for k in L.KS:
            xm = mp_recs[k - 1].x
            d = np.array([mpmath.mpf(float(a)) + mpmath.mpf(float(a - np.longdouble(float(a)))) - m for a, m in zip(ld[k - 1].x, xm)], dtype=object)
            err = float(mpmath.sqrt(d @ d) / mpmath.sqrt(xm @ xm))
            host = L.dev_host('plain', 'f', k)[0]
            print('k=%d  |x_longdouble - x_50digits| / |x| = %.3g   dev_host = %.3g' % (k, err, host))
            assert err < 1e-3 * host


def test_dev_host_table_and_branches(capsys):
    """dev_host(layout, k) for every layout, right-hand side and k = 1..4, printed; every layout reaches the branches it exists for (checked
    in L.host_case), the host build runs exactly k iterations, and its deviation is that of a correct fp64 implementation (far below
    1e-6 -- a wrong operator is O(1) at k = 1)."""
    lines = ['%-13s %-5s %s' % ('layout', 'b', '   '.join('k=%d x / norms' % k for k in L.KS))]
    for name in L.NAMES:
        hc = L.host_case(name)
        assert hc.lay.needs <= L.branches(hc.lay.prob, hc.ctrl, hc.h.T)[0]
        for bkey in ('f', 'rand'):
            devs = [L.dev_host(name, bkey, k) for k in L.KS]
            lines.append('%-13s %-5s %s' % (name, bkey, '   '.join('%.2e / %.2e' % d for d in devs)))
            assert all(0 < d[0] < 1e-6 for d in devs), (name, bkey, devs)
    devs = [L.dev_host('plain', 'f', k, L.DAMP) for k in L.KS]
    lines.append('%-13s %-5s %s' % ('plain damp', 'f', '   '.join('%.2e / %.2e' % d for d in devs)))
    with capsys.disabled():
        print('\ndev_host = |x_host - x_longdouble| / |x_longdouble| and the largest relative deviation of (normr, normar, normA, condA)')
        print('\n'.join(lines))


def test_frozen_entries_of_the_host_build_are_exact_zeros():
    hc = L.host_case('frozen')
    idx = np.nonzero(hc.lay.frozen)[0]
    for k in L.KS:
        x = L.host_run('frozen', hc.rhs['f'], k).x
        assert not x[idx].any() and np.abs(x).max() > 0


def test_stopping_case_premise():
    """The run of the stopping test ends inside the first batch of eight, not on its boundary, and the deciding quantity is at least a
    factor 2 away from its threshold at that iteration and at the one before; the host build ends at the same iteration."""
    sc = L.stopping_case()
    print('stops at itn %d with istop %d, margin %.3g' % (sc.itn, sc.istop, sc.margin))
    assert sc.itn % 8 != 0 and 1 < sc.itn < 8
    assert sc.margin >= 2
    got = L.host_run('plain', sc.b, 0, **L.STOP_TOL)
    assert (got.itn, got.istop) == (sc.itn, sc.istop)
