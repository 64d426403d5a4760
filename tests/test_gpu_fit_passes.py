"""The passes of the smoothing fit around its band solvers -- k_fit_basis, k_fit_first, k_fit_blocks<T, NT>, k_fit_slice_sum<T>,
k_fit_band<T>, k_fit_penalty<T>, k_fit_residual, k_fit_total_partial / k_fit_total, k_fit_fpint / k_fit_fpint_final
(mvus_amd/csrc/spline_fit_passes.hip.h) -- on their own, through mvus_spline_fit_normal / _penalty / _residual, each against an exact
(rational) reference of exactly what it was given (tests/fit_reference.py: the cases, the chain lengths k and where they come from;
tests/test_fit_passes_host.py asserts the premises of the cases).  fp64 (NT = 256) and double-double (NT = 64) throughout.

Bars, with eps = 2^-53 and unit = eps (fp64) or 2^-100 (double-double):
  span, first: equal to the reference as integers, and first[span[i]] <= i < first[span[i] + 1] for every sample;
  q: relative error <= gamma_15 per entry against de Boor at 50 digits (5 roundings a level); exact zeros are zeros;
  G5, rhs (hi + lo taken exactly) against the exact accumulation of the DEVICE's q: |error| <= k unit sum |terms| per entry, k that
      entry's chain length; |lo| <= 2^-52 |hi|; G5[.][4] = 0;
  c: bit for bit what mvus_spline_band_solve returns for the G5 / rhs read back (same precise, parts);
  BtB: the same bar with k = 6;
  term against the exact value from the device's q: sum_d (2 |r_d| delta_d + delta_d^2) + gamma_4 term, delta_d = gamma_5 (sum |c q| + |x_d|);
  fp against the exact sum of the device's term: relative (chain + 1) eps;  fpint against both statements of the per-span rule on the
      device's term: relative (chain + 3) eps; production and explicit slice counts within the sum of their bars of each other.
Every test prints measured / bar (run with -s)."""
import functools
import math
from fractions import Fraction

import numpy as np
import pytest

import fit_reference as fr

F = Fraction


def _call(fn, what, *a, **kw):
    try:
        return fn(*a, **kw)
    except RuntimeError as e:                              # a HIP error: nothing more is launched on a device that may have faulted
        pytest.exit('%s on %s' % (e, what), returncode=3)


def _normal(name, slices, parts, precise):
    from mvus_amd import spline
    k = fr.build(name)
    return _call(spline.fit_normal, '%s slices=%d parts=%d precise=%d' % (name, slices, parts, precise), k.u, k.X, k.t, precise=precise, slices=slices, parts=parts)


def _residual(name, c, slices):
    from mvus_amd import spline
    k = fr.build(name)
    return _call(spline.fit_residual, '%s residual slices=%d' % (name, slices), k.u, k.X, k.t, c, slices=slices)


def _same_normal(a, b):
    return all(np.array_equal(getattr(a, f), getattr(b, f), equal_nan=True) for f in ('span', 'q', 'first', 'G5', 'G5_lo', 'rhs', 'rhs_lo', 'c', 'stats')) and a.fail == b.fail


def _same_residual(a, b):
    return np.array_equal(a.term, b.term) and a.fp == b.fp and np.array_equal(a.fpint, b.fpint)


@functools.lru_cache(maxsize=None)
def _device_basis(name):
    """the device's own span / q / first of a case (the same in every configuration: asserted where they are compared)"""
    got = _normal(name, 0, 0, False)
    return got.span.copy(), got.q.copy(), got.first.copy()


@functools.lru_cache(maxsize=None)
def _blocks(name):
    k = fr.build(name)
    return fr.exact_blocks(_device_basis(name)[1], k.X, k.first)


@functools.lru_cache(maxsize=None)
def _basis50(name):
    k = fr.build(name)
    return fr.basis50(k.u, k.t, k.span)


def _ratio(hi, lo, value, sum_abs, kk, unit):
    err = abs(F(float(hi)) + F(float(lo)) - value)
    if sum_abs == 0:
        return 0.0 if err == 0 else math.inf
    return float(err / (kk * F(unit) * sum_abs))


def _slices(k, s):
    return s if s else fr.fit_slices(k.nspan)


NORMAL = [(c.name, precise) for c in fr.normal_cases() for precise in (False, True)]


@pytest.mark.gpu
@pytest.mark.parametrize('name,precise', NORMAL, ids=['%s-%s' % (n, 'dd' if p else 'fp64') for n, p in NORMAL])
def test_gpu_fit_normal(name, precise):
    from mvus_amd import spline
    k = fr.build(name)
    NT, unit = (64, fr.U100) if precise else (256, fr.EPS)
    i = np.arange(k.u.size)
    for slices, parts in k.case.configs:
        got = _normal(name, slices, parts, precise)
        assert _same_normal(got, _normal(name, slices, parts, precise)), 'a repeated call is not bit-identical'
        # integers
        assert np.array_equal(got.span, k.span) and np.array_equal(got.first, k.first)
        assert np.all(got.first[got.span] <= i) and np.all(i < got.first[got.span + 1])
        # the basis
        qerr, zeros_ok = fr.basis_errors(got.q, _basis50(name))
        assert zeros_ok, 'an exact zero of the basis is not a zero (or the other way round)'
        span, q, first = _device_basis(name)
        assert np.array_equal(got.q, q) and np.array_equal(got.span, span) and np.array_equal(got.first, first)
        # the normal equations from the device's q
        G5, rhs = fr.exact_normal(q, k.X, k.first, _slices(k, slices), NT, blocks=_blocks(name))
        worst_g = max(_ratio(got.G5[j, w], got.G5_lo[j, w], *G5[j][w], unit) for j in range(k.ncoef) for w in range(4))
        worst_r = max(_ratio(got.rhs[d, j], got.rhs_lo[d, j], *rhs[d][j], unit) for j in range(k.ncoef) for d in range(3))
        kmax = max(G5[j][0][2] for j in range(k.ncoef))
        print('\n%-22s %-4s slices %-3d parts %-2d  q %.3g  G5 %.3g  rhs %.3g  (k <= %d)  pivots %.2e..%.2e fail %d'
              % (name, 'dd' if precise else 'fp64', _slices(k, slices), parts, qerr / fr.basis_bar(), worst_g, worst_r, kmax, got.stats[2], got.stats[3], got.fail))
        assert qerr <= fr.basis_bar()
        assert worst_g <= 1 and worst_r <= 1
        assert np.all(got.G5[:, 4] == 0) and np.all(got.G5_lo[:, 4] == 0)
        assert np.all(np.abs(got.G5_lo) <= 2.0 ** -52 * np.abs(got.G5)) and np.all(np.abs(got.rhs_lo) <= 2.0 ** -52 * np.abs(got.rhs))
        if not precise:
            assert not got.G5_lo.any() and not got.rhs_lo.any()
        # the solve: k_fit_band's own scatter feeds the same kernels as the band-solve hook's
        ref = _call(spline.band_solve, name, got.G5, got.rhs, 3, precise=precise, parts=parts, G5_lo=got.G5_lo, rhs_lo=got.rhs_lo)
        assert np.array_equal(got.c, ref.c) and np.array_equal(got.stats, ref.stats, equal_nan=True) and got.fail == ref.fail
        assert np.all(np.isfinite(got.c))
        if name == 'interp-m300':
            assert ref.P == (1 if parts == -1 else (2 if parts == 2 else 10))


@functools.lru_cache(maxsize=None)
def _coefficients(name):
    k = fr.build(name)
    sets = dict(fr.coefficient_sets(k.ncoef, 11))
    sets['lsq'] = _normal(name, 0, 0, True).c.copy()          # (double-double: the interpolation limit is ill conditioned in fp64)
    return sets


def _check_sums(name, got, slices, line):
    """fp and fpint of a residual call against the exact sums of ITS term"""
    k = fr.build(name)
    tf = [F(float(v)) for v in got.term]
    total = sum(tf)
    m = k.u.size
    fp_bar = (fr.total_chain(m) + 1) * fr.EPS
    fp_err = float(abs(F(got.fp) - total) / total) if total else float(got.fp != 0)
    closed = fr.fpint_closed(tf, k.first)
    assert closed == fr.fpint_fppara(tf, k.u, k.t)
    chain = fr.fpint_chain(k.first, _slices(k, slices))
    worst = 0.0
    for sp in range(k.nspan):
        if closed[sp] == 0:
            assert got.fpint[sp] == 0
            continue
        worst = max(worst, float(abs(F(float(got.fpint[sp])) - closed[sp]) / closed[sp]) / ((chain[sp] + 3) * fr.EPS))
    line.append('fp %.3g fpint %.3g' % (fp_err / fp_bar, worst))
    return fp_err / fp_bar, worst, closed, chain


RESIDUAL = [c.name for c in fr.normal_cases()]


@pytest.mark.gpu
@pytest.mark.parametrize('name', RESIDUAL)
def test_gpu_fit_residual(name):
    k = fr.build(name)
    span, q, first = _device_basis(name)
    slice_counts = sorted({s for s, _ in k.case.configs})
    for cname, c in _coefficients(name).items():
        terms, bars = fr.exact_term(q, c, k.X, span)
        by_slices = {}
        for slices in slice_counts:
            got = _residual(name, c, slices)
            assert _same_residual(got, _residual(name, c, slices)), 'a repeated call is not bit-identical'
            err = np.array([float(abs(F(float(g)) - e)) for g, e in zip(got.term, terms)])
            ok = bars > 0
            assert np.all(err[~ok] == 0)
            worst_t = float((err[ok] / bars[ok]).max()) if ok.any() else 0.0
            line = ['%-22s c=%-6s slices %-3d term %.3g' % (name, cname, _slices(k, slices), worst_t)]
            fp_r, fpint_r, closed, chain = _check_sums(name, got, slices, line)
            print('\n' + '  '.join(line))
            assert worst_t <= 1 and fp_r <= 1 and fpint_r <= 1
            by_slices[slices] = (got, chain)
        base, chain0 = by_slices[0]
        for slices, (got, chain) in by_slices.items():       # (term does not depend on the slices: same bits)
            assert np.array_equal(got.term, base.term) and got.fp == base.fp
            for sp in range(k.nspan):
                assert abs(got.fpint[sp] - base.fpint[sp]) <= (chain[sp] + chain0[sp] + 6) * fr.EPS * max(got.fpint[sp], base.fpint[sp])


@pytest.mark.gpu
@pytest.mark.parametrize('name', [c.name for c in fr.total_cases()])
def test_gpu_fit_total_switch(name):
    """m = 8192: one stage; m = 8193: two stages with 5 partial sums -- fp and fpint against the exact sums of the device's term"""
    k = fr.build(name)
    assert fr.total_parts(k.u.size) == (4 if k.u.size == 8192 else 5) and (k.u.size > fr.TOTAL_ONE_STAGE) == (name == 'total-m8193')
    for cname, c in fr.coefficient_sets(k.ncoef, 11).items():
        got = _residual(name, c, 0)
        assert _same_residual(got, _residual(name, c, 0))
        line = ['%-22s c=%-6s' % (name, cname)]
        fp_r, fpint_r, _, _ = _check_sums(name, got, 0, line)
        print('\n' + '  '.join(line))
        assert fp_r <= 1 and fpint_r <= 1


@pytest.mark.gpu
def test_gpu_fit_total_capped_partials():
    """m = 2 100 000: ceil(m / 2048) = 1026 partial sums capped at 1024, so the grid-stride loop of k_fit_total_partial takes a ninth
    round in its first workgroups (2048 values a workgroup below the cap: eight); one span in 256 slices.  fp and fpint[0] against math.fsum of the device's term."""
    from mvus_amd import spline
    m = fr.BIG_M
    u, X = fr.samples(m, 4)
    t = fr.knots(u, [])
    c = fr.coefficient_sets(4, 12)['random']
    got = _call(spline.fit_residual, 'm=%d' % m, u, X, t, c)
    total = math.fsum(got.term)
    assert total > 0 and np.all(got.term >= 0)
    fp_bar = (fr.total_chain(m) + 1) * fr.EPS
    chain = fr.fpint_chain(np.array([0, m]), 256)[0]
    fp_err, sp_err = abs(got.fp - total) / total, abs(got.fpint[0] - total) / total
    print('\nm=%d  partials %d  fp %.3g  fpint %.3g  (chains %d, %d; fsum %.17g, fp %.17g, fpint %.17g)'
          % (m, fr.total_parts(m), fp_err / fp_bar, sp_err / ((chain + 3) * fr.EPS), fr.total_chain(m), chain, total, got.fp, got.fpint[0]))
    assert fp_err <= fp_bar and sp_err <= (chain + 3) * fr.EPS
    # term itself at a few samples, against the plain formula in numpy (gamma_5-sized errors of numbers of size 100)
    idx = np.array([0, 1, 2047, 2048, 524287, 524288, m - 2, m - 1])
    from scipy.interpolate import BSpline
    r = np.stack([BSpline(t, c[d], 3)(u[idx]) for d in range(3)]) - X[:, idx]
    np.testing.assert_allclose(got.term[idx], (r * r).sum(axis=0), rtol=1e-12)


PENALTY = [(name, precise) for name, _, _ in fr.penalty_cases() for precise in (False, True)]


@pytest.mark.gpu
@pytest.mark.parametrize('name,precise', PENALTY, ids=['%s-%s' % (n, 'dd' if p else 'fp64') for n, p in PENALTY])
def test_gpu_fit_penalty(name, precise):
    from mvus_amd import spline
    _, ncoef, b = next(c for c in fr.penalty_cases() if c[0] == name)
    unit = fr.U100 if precise else fr.EPS
    BtB, lo = _call(spline.fit_penalty, name, b, ncoef, precise=precise)
    again = spline.fit_penalty(b, ncoef, precise=precise)
    assert np.array_equal(BtB, again[0]) and np.array_equal(lo, again[1])
    ex = fr.exact_btb(b, ncoef)
    worst = max(_ratio(BtB[j, w], lo[j, w], ex[j][w][0], ex[j][w][1], 6, unit) for j in range(ncoef) for w in range(5))
    print('\n%-16s %-4s ncoef %-3d  BtB %.3g' % (name, 'dd' if precise else 'fp64', ncoef, worst))
    assert worst <= 1
    assert np.all(np.abs(lo) <= 2.0 ** -52 * np.abs(BtB)) and (precise or not lo.any())
    for j in range(min(4, ncoef)):
        assert not BtB[j, j + 1:].any() and not lo[j, j + 1:].any()
    assert not BtB[b.shape[0] + 4:].any()                    # columns no row of b reaches


@pytest.mark.gpu
@pytest.mark.parametrize('name,slices,parts', [('interp-m300', 0, 0), ('one-m600', 7, 0), ('edge-nspan511', 0, 0)])
def test_gpu_fit_normal_does_not_see_stale_work_arrays(name, slices, parts):
    """double-double, then fp64 on the same sizes (the allocator hands the same blocks out again), then back: each returns its own bits"""
    first = {p: _normal(name, slices, parts, p) for p in (True, False)}
    for p in (True, False, False, True):
        assert _same_normal(_normal(name, slices, parts, p), first[p])
    assert not np.array_equal(first[True].G5_lo, first[False].G5_lo)


@pytest.mark.gpu
def test_gpu_fit_passes_refusals():
    """what the entry points refuse (tests/test_fit_passes_host.py has the full list, without a device) is refused on a machine with a GPU
    too, raises ValueError through the wrapper, and leaves the next legal call intact"""
    from mvus_amd import spline
    k = fr.build('two-left1')
    good = _normal('two-left1', 1, 0, False)
    a = np.nextafter(k.u[5], np.inf)
    for t in (fr.knots(k.u, [a, np.nextafter(a, np.inf)]), fr.knots(k.u, [k.u[7], k.u[6]]), k.t[1:], fr.knots(k.u, [k.u[0]])):
        with pytest.raises(ValueError):
            spline.fit_normal(k.u, k.X, t)
        with pytest.raises(ValueError):
            spline.fit_residual(k.u, k.X, t, np.zeros((3, t.size - 4)))
    for kw in (dict(slices=257), dict(slices=-1), dict(parts=2), dict(parts=1)):
        with pytest.raises(ValueError):
            spline.fit_normal(k.u, k.X, k.t, **kw)
    with pytest.raises(ValueError):
        spline.fit_normal(k.u[::-1].copy(), k.X, k.t)
    with pytest.raises(ValueError):
        spline.fit_penalty(np.ones((7, 5)), 10)
    assert _same_normal(_normal('two-left1', 1, 0, False), good)
