"""The weighted smoothing fit -- splprep's ``w`` through mvus_spline_smooth_w / mvus_spline_fit_open_w and the two kernels that read the
weights, k_fit_blocks_w<T, NT> and k_fit_residual_w (mvus_amd/csrc/spline_fit_weighted.hip.h):

  1. the weighted fit is FITPACK's: scipy's ``splprep(w=...)`` is the reference (oracle/fitpack_oracle.py is unit-weight) -- identical
     knots and ier, fp to 1e-8 max(fp, s), coefficients within max(1e-8, 8 x spread), ``spread`` the largest change of scipy's OWN weighted
     coefficients under five relative perturbations of X of 1e-13 (how well the problem determines them; never taken from the GPU);
  2. a session is the one-shot call, and w = None / w = 1 are today's fit, bit for bit;
  3. the two passes against exact (rational) sums of what they were given, on the cases and at every slice / partition configuration of
     tests/fit_reference.py: for power-of-two weights w h and w x are exact, so the bars of tests/test_gpu_fit_passes.py apply unchanged
     to the scaled operands; for general weights every term carries two more roundings (one per scaled factor): k + 2 in each bar;
  4. a heteroscedastic trajectory (30 % of the samples with sigma = 0.5, the rest 0.02): scipy's knots, and at least five times closer to
     the true curve than the unweighted fit (scipy gets a factor of 19);
  5. what is refused.
Every test prints measured / bar (run with -s)."""
import functools
import math
from fractions import Fraction

import numpy as np
import pytest
from scipy import interpolate

import fit_reference as fr

F = Fraction
COEF_ATOL = 1e-8


# ---- the trajectories and smoothing factors of tests/test_traj_to_spline.py (restated) ------------------------------------------------------
def _trajectory(seed, m, noise=0.02, speed=1.0):
    rng = np.random.default_rng(seed)
    u = np.cumsum(rng.uniform(0.5, 1.5, m))
    X = np.vstack([10 * np.sin(u / 80 * speed), 10 * np.cos(u / 95), 30 + 3 * np.sin(u / 50)]) + rng.normal(0, noise, (3, m))
    return u, X


CASES = [(0, 120, ('rel', 1e-6)), (1, 90, ('rel', 1e-4)), (2, 150, ('abs', 0.05)), (3, 200, ('abs', 1.0)), (4, 80, ('abs', 50.0)), (5, 60, ('abs', 5e3)),
         (6, 349, ('rel', 1e-6)), (7, 276, ('abs', 0.05)), (8, 5000, ('abs', 1.0))]
KINDS = ('pow2', 'uniform')


def _s_of(u, spec):
    return spec[1] * (u[-1] - u[0]) if spec[0] == 'rel' else spec[1]


def _case_weights(seed, m):
    return {'pow2': 2.0 ** np.random.default_rng(1000 + seed).integers(-3, 2, m), 'uniform': np.random.default_rng(1000 + seed).uniform(0.2, 3.0, m)}


def _scipy_fit(u, X, w, s):
    (tck, _u), fp, ier, _msg = interpolate.splprep(X, w=w, u=u, s=s, k=3, full_output=1)
    return tck, fp, ier


def _spread(u, X, w, s, tck0, seed):
    """largest change of scipy's coefficients over five fits of X (1 + 1e-13 r), r uniform in [-1, 1]; the knots must not move"""
    rng = np.random.default_rng(2000 + seed)
    worst = 0.0
    for _ in range(5):
        tck, _, _ = _scipy_fit(u, X * (1.0 + 1e-13 * rng.uniform(-1.0, 1.0, X.shape)), w, s)
        assert np.array_equal(tck[0], tck0[0]), 'the premise of the case: the knot choice has margin'
        worst = max(worst, float(np.abs(np.asarray(tck[1]) - np.asarray(tck0[1])).max()))
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('seed,m,spec', CASES)
def test_gpu_weighted_fit_is_fitpacks(seed, m, spec, kind):
    """Measured on an MI355X: worst coefficients / bar 0.0070, worst fp / bar 0.081 (seed 6, powers of two: 339 knots for 349 samples;
    3.68 while f_p of its last least-squares pass was summed from coefficients of size 1e13 rounded to fp64)."""
    from mvus_amd import spline
    u, X = _trajectory(seed, m, speed=1 + seed % 7)
    s = _s_of(u, spec)
    w = _case_weights(seed, m)[kind]
    tck0, fp0, ier0 = _scipy_fit(u, X, w, s)
    bar = max(COEF_ATOL, 8 * _spread(u, X, w, s, tck0, seed))
    tck, fp, ier = spline.smooth_fit(u, X, s, full_output=True, w=w)
    np.testing.assert_array_equal(tck[0], tck0[0])
    err = float(np.abs(np.asarray(tck[1]) - np.asarray(tck0[1])).max())
    print('\nseed %d m %-4d %-7s knots %-4d ier %2d  coefficients %.3g / %.3g = %.3g  fp %.3g'
          % (seed, m, kind, len(tck0[0]), ier0, err, bar, err / bar, abs(fp - fp0) / (1e-8 * max(fp0, s))))
    assert ier == ier0 and tck[2] == 3
    assert abs(fp - fp0) <= 1e-8 * max(fp0, s)
    assert err <= bar


@pytest.mark.gpu
def test_gpu_weighted_session_is_the_one_shot_fit_and_none_is_todays_fit():
    from mvus_amd import spline
    u, X = _trajectory(12, 3000, speed=3)
    w = np.random.default_rng(5).uniform(0.2, 3.0, u.size)

    def same(a, b):
        return np.array_equal(a[0][0], b[0][0]) and np.array_equal(np.asarray(a[0][1]), np.asarray(b[0][1])) and a[1:] == b[1:]

    with spline.SmoothFit(u, X, w=w) as fit:
        for s in (20.0, 2.5, 400.0):                       # knot counts up and down: the work arrays grow, are reused, hold stale data
            assert same(fit(s, full_output=True), spline.smooth_fit(u, X, s, full_output=True, w=w))
    plain = spline.smooth_fit(u, X, 20.0, full_output=True)
    assert same(spline.smooth_fit(u, X, 20.0, full_output=True, w=None), plain)
    assert same(spline.smooth_fit(u, X, 20.0, full_output=True, w=np.ones(u.size)), plain)      # 1.0 * h is exact
    with spline.SmoothFit(u, X, w=None) as fit:
        assert same(fit(20.0, full_output=True), plain)
    assert not same(spline.smooth_fit(u, X, 20.0, full_output=True, w=w), plain)


# ---- 3: the passes against exact sums ----------------------------------------------------------------------------------------------------
def _call(fn, what, *a, **kw):
    try:
        return fn(*a, **kw)
    except RuntimeError as e:                              # a HIP error: nothing more is launched on a device that may have faulted
        pytest.exit('%s on %s' % (e, what), returncode=3)


@functools.lru_cache(maxsize=None)
def _pass_weights(name, kind):
    k = fr.build(name)
    rng = np.random.default_rng(3000 + k.u.size)
    return 2.0 ** rng.integers(-3, 2, k.u.size) if kind == 'pow2' else rng.uniform(0.2, 3.0, k.u.size)


@functools.lru_cache(maxsize=None)
def _device_basis(name):
    from mvus_amd import spline
    k = fr.build(name)
    got = _call(spline.fit_normal, name, k.u, k.X, k.t)
    return got.span.copy(), got.q.copy(), got.first.copy()


@functools.lru_cache(maxsize=None)
def _weighted_blocks(name, kind):
    """fr.exact_blocks for the rows w h, right-hand sides w x: on the scaled doubles where the scaling is exact, else with the products
    Fraction(w) Fraction(h), Fraction(w) Fraction(x) taken exactly"""
    k = fr.build(name)
    q, w = _device_basis(name)[1], _pass_weights(name, kind)
    if kind == 'pow2':
        return fr.exact_blocks(q * w[:, None], k.X * w, k.first)
    blocks = []
    for sp in range(len(k.first) - 1):
        s, sa = [F(0)] * fr.K_FIT_BLK, [F(0)] * fr.K_FIT_BLK
        for i in range(int(k.first[sp]), int(k.first[sp + 1])):
            wi = F(float(w[i]))
            h, x = [wi * F(float(v)) for v in q[i]], [wi * F(float(v)) for v in k.X[:, i]]
            for a in range(4):
                for b in range(a + 1):
                    p = h[a] * h[b]
                    s[a * (a + 1) // 2 + b] += p
                    sa[a * (a + 1) // 2 + b] += abs(p)
                for d in range(3):
                    p = h[a] * x[d]
                    s[10 + 3 * a + d] += p
                    sa[10 + 3 * a + d] += abs(p)
        blocks.append((s, sa))
    return blocks


def _ratio(hi, lo, value, sum_abs, kk, unit):
    err = abs(F(float(hi)) + F(float(lo)) - value)
    if sum_abs == 0:
        return 0.0 if err == 0 else math.inf
    return float(err / (kk * F(unit) * sum_abs))


def _slices(k, s):
    return s if s else fr.fit_slices(k.nspan)


NORMAL = [(c.name, precise, kind) for c in fr.normal_cases() for precise in (False, True) for kind in KINDS]


@pytest.mark.gpu
@pytest.mark.parametrize('name,precise,kind', NORMAL, ids=['%s-%s-%s' % (n, 'dd' if p else 'fp64', kd) for n, p, kd in NORMAL])
def test_gpu_weighted_fit_normal(name, precise, kind):
    from mvus_amd import spline
    k = fr.build(name)
    w = _pass_weights(name, kind)
    NT, unit = (64, fr.U100) if precise else (256, fr.EPS)
    extra = 0 if kind == 'pow2' else 2
    span, q, first = _device_basis(name)
    for slices, parts in k.case.configs:
        what = '%s %s slices=%d parts=%d precise=%d' % (name, kind, slices, parts, precise)
        got = _call(spline.fit_normal, what, k.u, k.X, k.t, precise=precise, slices=slices, parts=parts, w=w)
        again = _call(spline.fit_normal, what, k.u, k.X, k.t, precise=precise, slices=slices, parts=parts, w=w)
        assert all(np.array_equal(getattr(got, f), getattr(again, f), equal_nan=True) for f in ('G5', 'G5_lo', 'rhs', 'rhs_lo', 'c', 'stats')), 'a repeated call is not bit-identical'
        assert np.array_equal(got.q, q) and np.array_equal(got.span, span) and np.array_equal(got.first, first)      # q stays unweighted
        G5, rhs = fr.exact_normal(q, k.X, k.first, _slices(k, slices), NT, blocks=_weighted_blocks(name, kind))
        worst_g = max(_ratio(got.G5[j, v], got.G5_lo[j, v], G5[j][v][0], G5[j][v][1], G5[j][v][2] + extra, unit) for j in range(k.ncoef) for v in range(4))
        worst_r = max(_ratio(got.rhs[d, j], got.rhs_lo[d, j], rhs[d][j][0], rhs[d][j][1], rhs[d][j][2] + extra, unit) for j in range(k.ncoef) for d in range(3))
        print('\n%-22s %-4s %-7s slices %-3d parts %-2d  G5 %.3g  rhs %.3g  (k + %d)' % (name, 'dd' if precise else 'fp64', kind, _slices(k, slices), parts, worst_g, worst_r, extra))
        assert worst_g <= 1 and worst_r <= 1
        assert np.all(got.G5[:, 4] == 0) and np.all(got.G5_lo[:, 4] == 0)
        assert np.all(np.abs(got.G5_lo) <= 2.0 ** -52 * np.abs(got.G5)) and np.all(np.abs(got.rhs_lo) <= 2.0 ** -52 * np.abs(got.rhs))
        if not precise:
            assert not got.G5_lo.any() and not got.rhs_lo.any()
        ref = _call(spline.band_solve, what, got.G5, got.rhs, 3, precise=precise, parts=parts, G5_lo=got.G5_lo, rhs_lo=got.rhs_lo)
        assert np.array_equal(got.c, ref.c) and np.array_equal(got.stats, ref.stats, equal_nan=True) and got.fail == ref.fail
    # w = None and w = 1 are the unweighted pass, bit for bit
    slices, parts = k.case.configs[0]
    plain = _call(spline.fit_normal, name, k.u, k.X, k.t, precise=precise, slices=slices, parts=parts)
    for ww in (None, np.ones(k.u.size)):
        one = _call(spline.fit_normal, name, k.u, k.X, k.t, precise=precise, slices=slices, parts=parts, w=ww)
        assert all(np.array_equal(getattr(one, f), getattr(plain, f), equal_nan=True) for f in ('q', 'G5', 'G5_lo', 'rhs', 'rhs_lo', 'c', 'stats'))


def _exact_weighted_term(q, c, X, w, span, extra):
    """fr.exact_term for term[i] = sum_d (w_i (sum_a c q - x_d))^2 with w taken exactly, and its bar with `extra` more roundings in every
    chain: delta_d = gamma_(5 + extra) |w| (sum |c q| + |x_d|), sum_d (2 |w r_d| delta_d + delta_d^2) + gamma_(4 + extra) term"""
    cf = [[F(float(v)) for v in c[d]] for d in range(3)]
    ga, gb = fr.gamma(5 + extra), fr.gamma(4 + extra)
    terms, bars = [], []
    for i in range(q.shape[0]):
        h, sp, wi = [F(float(v)) for v in q[i]], int(span[i]), F(float(w[i]))
        tot, bar = F(0), 0.0
        for d in range(3):
            prods = [cf[d][sp + a] * h[a] for a in range(4)]
            x = F(float(X[d, i]))
            r = wi * (sum(prods) - x)
            delta = ga * float(wi * (sum(abs(p) for p in prods) + abs(x)))
            bar += 2 * abs(float(r)) * delta + delta * delta
            tot += r * r
        terms.append(tot)
        bars.append(bar + gb * float(tot))
    return terms, np.array(bars)


RESIDUAL = [(c.name, kind) for c in fr.normal_cases() for kind in KINDS]


@pytest.mark.gpu
@pytest.mark.parametrize('name,kind', RESIDUAL, ids=['%s-%s' % r for r in RESIDUAL])
def test_gpu_weighted_fit_residual(name, kind):
    from mvus_amd import spline
    k = fr.build(name)
    w = _pass_weights(name, kind)
    span, q, first = _device_basis(name)
    sets = {'random': fr.coefficient_sets(k.ncoef, 11)['random'],
            'lsq': _call(spline.fit_normal, name, k.u, k.X, k.t, precise=True, w=w).c.copy()}      # (double-double: the interpolation limit is ill conditioned in fp64)
    for cname, c in sets.items():
        if kind == 'pow2':                                   # w (fac - x) = sum c (w q) - w x exactly: the unweighted bar on the scaled operands
            terms, bars = fr.exact_term(q * w[:, None], c, k.X * w, span)
        else:
            terms, bars = _exact_weighted_term(q, c, k.X, w, span, 2)
        base = None
        for slices in sorted({s for s, _ in k.case.configs}):
            what = '%s %s residual slices=%d' % (name, kind, slices)
            got = _call(spline.fit_residual, what, k.u, k.X, k.t, c, slices=slices, w=w)
            again = _call(spline.fit_residual, what, k.u, k.X, k.t, c, slices=slices, w=w)
            assert np.array_equal(got.term, again.term) and got.fp == again.fp and np.array_equal(got.fpint, again.fpint)
            err = np.array([float(abs(F(float(g)) - e)) for g, e in zip(got.term, terms)])
            ok = bars > 0
            assert np.all(err[~ok] == 0)
            worst_t = float((err[ok] / bars[ok]).max()) if ok.any() else 0.0
            # fp and fpint: the unweighted kernels on the weighted term, against the exact sums of that term
            tf = [F(float(v)) for v in got.term]
            total = sum(tf)
            fp_r = (float(abs(F(got.fp) - total) / total) if total else float(got.fp != 0)) / ((fr.total_chain(k.u.size) + 1) * fr.EPS)
            closed, chain = fr.fpint_closed(tf, k.first), fr.fpint_chain(k.first, _slices(k, slices))
            fpint_r = max([float(abs(F(float(got.fpint[sp])) - closed[sp]) / closed[sp]) / ((chain[sp] + 3) * fr.EPS) for sp in range(k.nspan) if closed[sp] != 0] or [0.0])
            print('\n%-22s %-7s c=%-6s slices %-3d term %.3g  fp %.3g  fpint %.3g' % (name, kind, cname, _slices(k, slices), worst_t, fp_r, fpint_r))
            assert worst_t <= 1 and fp_r <= 1 and fpint_r <= 1
            if base is None:
                base = got
            assert np.array_equal(got.term, base.term) and got.fp == base.fp      # (term does not depend on the slices)
    plain = _call(spline.fit_residual, name, k.u, k.X, k.t, sets['random'])
    for ww in (None, np.ones(k.u.size)):
        one = _call(spline.fit_residual, name, k.u, k.X, k.t, sets['random'], w=ww)
        assert np.array_equal(one.term, plain.term) and one.fp == plain.fp and np.array_equal(one.fpint, plain.fpint)


# ---- 4: the heteroscedastic trajectory ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_weighted_fit_heteroscedastic_trajectory():
    from mvus_amd import spline
    rng = np.random.default_rng(42)
    m = 400
    u = np.cumsum(rng.uniform(0.5, 1.5, m))
    T = np.vstack([10 * np.sin(u / 80), 10 * np.cos(u / 95), 30 + 3 * np.sin(u / 50)])      # the true curve
    sig = np.where(rng.uniform(size=m) < 0.3, 0.5, 0.02)
    X = T + rng.normal(size=(3, m)) * sig
    rms = {}
    for label, w in (('unweighted', None), ('weighted', 0.02 / sig)):
        s = 3 * float(np.sum(((1.0 if w is None else w) * sig) ** 2))      # the expected weighted residual sum
        tck = spline.smooth_fit(u, X, s, w=w)
        Y = np.asarray(interpolate.splev(u, tck))
        rms[label] = float(np.sqrt(np.mean(np.sum((Y - T) ** 2, axis=0))))
        if w is not None:
            tck0, fp0, ier0 = _scipy_fit(u, X, w, s)
            bar = max(COEF_ATOL, 8 * _spread(u, X, w, s, tck0, 42))
            err = float(np.abs(np.asarray(tck[1]) - np.asarray(tck0[1])).max())
            Y0 = np.asarray(interpolate.splev(u, tck0))
            print('\nweighted: %d knots, coefficients %.3g / %.3g = %.3g; scipy rms %.4g' % (len(tck0[0]), err, bar, err / bar, np.sqrt(np.mean(np.sum((Y0 - T) ** 2, axis=0)))))
            np.testing.assert_array_equal(tck[0], tck0[0])
            assert len(tck0[0]) == 16 and err <= bar
    print('rms distance to the true curve: unweighted %.4g, weighted %.4g, ratio %.3g (bar: > 5)' % (rms['unweighted'], rms['weighted'], rms['unweighted'] / rms['weighted']))
    assert rms['weighted'] < rms['unweighted'] / 5


# ---- 5: refusals ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_weighted_fit_refusals():
    from mvus_amd import _lib, spline
    u, X = _trajectory(0, 50)
    w = np.ones(50)
    good = spline.smooth_fit(u, X, 1.0, w=w)
    k = fr.build('two-left1')
    for bad in (0.0, -1.0, np.nan, np.inf):
        wb = w.copy()
        wb[17] = bad
        for call in (lambda: spline.smooth_fit(u, X, 1.0, w=wb), lambda: spline.SmoothFit(u, X, w=wb),
                     lambda: spline.fit_normal(k.u, k.X, k.t, w=wb[:k.u.size]), lambda: spline.fit_residual(k.u, k.X, k.t, np.zeros((3, k.ncoef)), w=wb[:k.u.size])):
            with pytest.raises(ValueError, match='weights must be finite and strictly positive'):
                call()
            assert _lib.load().mvus_last_error(None)
    for wl in (w[:-1], np.ones(51), np.ones((50, 1))):
        with pytest.raises(ValueError, match='one weight per sample'):
            spline.smooth_fit(u, X, 1.0, w=wl)
        with pytest.raises(ValueError, match='one weight per sample'):
            spline.SmoothFit(u, X, w=wl)
    for s in (0.0, -1.0):
        with pytest.raises(ValueError, match='s > 0'):
            spline.smooth_fit(u, X, s, w=w)
        with spline.SmoothFit(u, X, w=w) as fit:
            with pytest.raises(ValueError, match='s > 0'):
                fit(s)
    again = spline.smooth_fit(u, X, 1.0, w=w)
    assert np.array_equal(again[0], good[0]) and np.array_equal(np.asarray(again[1]), np.asarray(good[1]))
