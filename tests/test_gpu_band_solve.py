"""The spline fit's band solvers -- k_band_solve, k_band_solve_parts, k_band_diag_sum (mvus_amd/csrc/spline_band_solve*.hip.h), HB = 3 and 4, fp64
and double-double -- on their own, through mvus_spline_band_solve / mvus_spline_band_diag_sum, against a banded Cholesky solve at 50
digits (tests/band_reference.py: the systems, their families A .. E and the genuine pair 'G', and the list of shapes; their premises
are asserted by tests/test_band_solve_host.py).

Bars, with eps = 2^-53 and k = 3 (2 hb + 1) + 1 (22 for hb = 3, 28 for hb = 4):
  backward error, fp64, every family:  |b - M c|_inf / (|M|_inf |c|_inf + |b|_inf) <= k eps, evaluated at 50 digits (Higham's gamma_k for
      a Cholesky solve whose factor rows hold at most 2 hb + 1 entries; LAPACK's dpbsv sits at 0.03 .. 0.2 eps on these systems);
  forward error, fp64, A and B:  max |c - c_ref| / max |c_ref| per column <= 2 kappa_inf k eps (the same theorem);
  forward error, double-double, A .. C, E and G:  <= 4 eps per column (unit roundoff 2^-100 and kappa <= 1e12 leave 1e-17 for the solve:
      what remains is the rounding of the result to double); a double-double path degraded to fp64 lands at 1e-7 on family C;
  forward error, double-double, D (n <= 200, kappa_inf at 50 digits):  <= 2 kappa_inf k 2^-100;
  out[2], out[3] (smallest / largest pivot) on A and B: relative 2 kappa_inf k eps against the diagonal of the factor in the kernel's
      own elimination order (natural for one chain, interiors-then-separators for the partitioned kernel); out[0] the same plus
      (n + 2) eps for its fp64 running sum;
  the fit's decision fail || !(out[3] <= 1e4 out[2]) is false on A and B and true on C, D and E; fail_out is 1 exactly on D in fp64
      and on E in both precisions; every output is finite.
Every test prints measured / bar (run with -s)."""
import numpy as np
import pytest

import band_reference as br

U100 = 2.0 ** -100


def _solve(key, parts, precise):
    from mvus_amd import spline
    s = br.system(key)
    try:
        return spline.band_solve(s.G5, s.rhs, s.hb, BtB=s.BtB, pinv=s.pinv, precise=precise, parts=parts, G5_lo=s.G5_lo, BtB_lo=s.BtB_lo, rhs_lo=s.rhs_lo)
    except RuntimeError as e:                              # a HIP error: nothing more is launched on a device that may have faulted
        pytest.exit('%s on %s' % (e, br.case_id(key, parts, precise)), returncode=3)


def _same(a, b):
    return (np.array_equal(a.c, b.c) and np.array_equal(a.stats, b.stats, equal_nan=True) and a.fail == b.fail and a.P == b.P)


def _ill(r):
    return bool(r.fail != 0 or not (r.stats[3] <= 1e4 * r.stats[2]))


SOLVES = [(key, parts, precise) for key, parts in br.solve_cases() for precise in (False, True)]


@pytest.mark.gpu
@pytest.mark.parametrize('key,parts,precise', SOLVES, ids=[br.case_id(*c) for c in SOLVES])
def test_gpu_band_solve(key, parts, precise):
    fam, n, hb = key[0], br.system(key).n, key[2]
    k = br.kbar(hb)
    got = _solve(key, parts, precise)
    assert _same(got, _solve(key, parts, precise)), 'a repeated call is not bit-identical'
    P = 1 if parts == -1 else (parts if parts >= 2 else br.parts_rule(n, hb))
    assert got.P == P
    if (n, parts) == (192, 0):
        assert got.P == 8
    if (n, parts) == (191, 0):
        assert got.P == 1
    chain = P == 1
    assert np.all(np.isfinite(got.c)) and np.isfinite(got.stats[2]) and np.isfinite(got.stats[3]) and got.stats[2] > 0
    assert np.isnan(got.stats[1]) and (np.isfinite(got.stats[0]) if chain else np.isnan(got.stats[0]))
    ref = br.reference(key, precise)
    line = ['%-26s P=%-3d' % (br.case_id(key, parts, precise), P)]
    checks = []

    def hold(name, measured, bar):
        line.append('%s %.3g' % (name, measured / bar))
        checks.append((name, measured, bar))

    if not precise:
        hold('bwd', br.backward_error(ref, got.c), k * br.EPS)
        if fam in 'AB':
            hold('fwd', br.forward_error(ref, got.c), 2 * br.kappa_inf(key) * k * br.EPS)
        elif ref.spd:
            line.append('(fwd %.2e)' % br.forward_error(ref, got.c))
    else:
        if fam in 'ABCEG':                                 # (E: family A less one unknown, the same reasoning)
            hold('fwd', br.forward_error(ref, got.c), 4 * br.EPS)
        elif fam == 'D' and n <= 200:
            hold('fwd', br.forward_error(ref, got.c), 2 * br.kappa_inf_mp(ref) * k * U100)
        else:
            line.append('(fwd %.2e)' % br.forward_error(ref, got.c))
    if fam in 'AB':
        bar = 2 * br.kappa_inf(key) * k * br.EPS
        diag = ref.diag if chain else br.permuted_diag(key, P)
        hold('min', abs(got.stats[2] / diag.min() - 1), bar)
        hold('max', abs(got.stats[3] / diag.max() - 1), bar)
        if chain:
            hold('sum', abs(got.stats[0] / ref.diag_sum - 1), bar + (n + 2) * br.EPS)
    line.append('pivots %.2e..%.2e fail %d' % (got.stats[2], got.stats[3], got.fail))
    print('\n' + '  '.join(line))
    for name, measured, bar in checks:
        assert measured <= bar, '%s: %.3e against %.3e' % (name, measured, bar)
    if fam in 'AB':
        assert not _ill(got)
    if fam in 'CDE':
        assert _ill(got)
    assert got.fail == int(fam == 'E' or (fam == 'D' and not precise))


DIAGS = [(key, precise) for key in br.diag_cases() for precise in (False, True)]


@pytest.mark.gpu
@pytest.mark.parametrize('key,precise', DIAGS, ids=[br.case_id(k, None, p) for k, p in DIAGS])
def test_gpu_band_diag_sum(key, precise):
    """k_band_diag_sum<3, T> against the 50-digit sum of diag(L), and against out[0] of k_band_solve<3, T> on the same system (the two
    differ in their arithmetic -- reciprocal pivots here, divisions there -- so they agree to the bar, not to the bit).  In
    double-double the factor is exact to 1e-17 at any kappa of the list and the bar is the running sum's (n + 2) eps plus the
    rounding of each diagonal entry, eps."""
    from mvus_amd import spline
    s = br.system(key)
    fam, n = key[0], s.n
    ref = br.reference(key, precise)
    got = spline.band_diag_sum(s.G5, precise=precise, G5_lo=s.G5_lo)
    assert got == spline.band_diag_sum(s.G5, precise=precise, G5_lo=s.G5_lo)
    chain = _solve(key, -1, precise).stats[0]
    if precise:
        bar = (n + 3) * br.EPS
    elif fam in 'ABG':
        bar = 2 * br.kappa_inf(key) * br.kbar(3) * br.EPS + (n + 2) * br.EPS
    else:
        bar = None
    err, agree = abs(got / ref.diag_sum - 1), abs(got / chain - 1)
    print('\n%-22s sum %.15g  ' % (br.case_id(key, None, precise), got)
          + ('measured / bar %.3g, against k_band_solve %.3g' % (err / bar, agree / (2 * bar)) if bar else '(error %.2e, against k_band_solve %.2e)' % (err, agree)))
    assert np.isfinite(got) and got > 0
    if bar:
        assert err <= bar and agree <= 2 * bar


@pytest.mark.gpu
@pytest.mark.parametrize('key,parts', [(('A', 700, 3), 0), (('A', 700, 4), 0), (('C', br.SUBSET_N, 4), 65), (('A', 191, 3), -1)], ids=lambda v: str(v).replace(' ', ''))
def test_gpu_band_solve_does_not_see_stale_work_arrays(key, parts):
    """double-double, then fp64 on the same sizes (the allocator hands the same blocks out again, now holding the other precision's
    factor), then double-double again: the same bits; and the same the other way round"""
    first = {p: _solve(key, parts, p) for p in (True, False)}
    for p in (True, False, False, True):
        assert _same(_solve(key, parts, p), first[p])


@pytest.mark.gpu
def test_gpu_band_solve_refusals():
    """what the entry points refuse (tests/test_band_solve_host.py has the full list, without a device) is refused on a machine with a
    GPU too, raises ValueError through the wrapper, and leaves the next legal call intact"""
    from mvus_amd import spline
    s = br.system(('A', 65, 3))
    good = _solve(('A', 65, 3), 2, False)
    for kw in (dict(hb=2), dict(hb=3, parts=8), dict(hb=3, parts=257), dict(hb=3, BtB=s.G5), dict(hb=4), dict(hb=3, parts=1)):
        with pytest.raises(ValueError):
            spline.band_solve(s.G5, s.rhs, **kw)
    with pytest.raises(ValueError):
        spline.band_solve(s.G5[:3], s.rhs[:, :3], 3)
    with pytest.raises(ValueError):
        spline.band_diag_sum(s.G5[:3])
    assert br.parts_fixed(65, 3, 7) is not None and br.parts_fixed(65, 3, 8) is None
    assert _same(_solve(('A', 65, 3), 2, False), good)
