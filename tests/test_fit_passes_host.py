"""What tests/test_gpu_fit_passes.py rests on, checked without a GPU: the capacities of the fit's sliced passes and of its two-stage
total (fit_slices, kFitSliceBlocks, kFitBlk, fit_total_parts of mvus_amd/csrc/spline_fit_passes.hip.h through the host build), the reference
of tests/fit_reference.py against scipy and oracle/fitpack_oracle.py, the premises of every case, and what the entry points refuse."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest

import fit_reference as fr
from hostcheck_util import load
from mvus_amd import _lib


def _constants():
    out = np.zeros(4, np.int64)
    load().hostcheck_fit_constants(out.ctypes.data_as(_lib.c_int64_p))
    return tuple(int(v) for v in out)


# ---- capacities ---------------------------------------------------------------------------------------------------------------------
def test_constants_are_the_restated_ones():
    assert _constants() == (fr.K_FIT_BLK, fr.K_SLICE_BLOCKS, fr.TOTAL_ONE_STAGE, fr.TOTAL_PARTS)
    lib = load()
    for nspan in range(1, 4097):
        assert lib.hostcheck_fit_slices(nspan) == fr.fit_slices(nspan)
    assert fr.fit_slices(1) == 256 and fr.fit_slices(511) == 3 and fr.fit_slices(512) == 1


def test_capacities_of_the_production_rule():
    """nspan = 1 .. 4096: at most 256 slices; the blocks beyond slice 0 stay below kFitSliceBlocks; the partial sums fit fp_part
    (512 + kFitSliceBlocks); the blocks written to SB fit kFitBlk (nest + kFitSliceBlocks) for the smallest nest that can hold nspan
    spans (nest = nspan + 7 knots; the fit's capacity is at least n + 16)."""
    lib = load()
    blk, extra, _, _ = _constants()
    for nspan in range(1, 4097):
        s = lib.hostcheck_fit_slices(nspan)
        assert 1 <= s <= 256
        assert nspan * (s - 1) < extra
        # fp_part holds nspan s partial sums, written by k_fit_fpint only when s > 1 (with one slice it writes fpint itself): the bound
        # holds for every nspan that is sliced and, as a number, up to nspan = 2048
        assert s == 1 or nspan * s <= 512 + extra
        assert (nspan * s <= 512 + extra) == (nspan <= 2048)
        assert (s > 1) == (nspan < 512)
        assert blk * nspan * s <= blk * (nspan + 7 + extra)
        assert lib.hostcheck_fit_slices_legal(nspan, s)         # the rule is one of the explicit counts the entry points accept


def test_capacities_of_explicit_slice_counts():
    """every (nspan, slices) the entry points accept: the same bounds (non-strict: an explicit count may fill the arrays), and the
    acceptance rule is the restated one"""
    lib = load()
    blk, extra, _, _ = _constants()
    accepted = 0
    for nspan in list(range(1, 2100)) + [4096, 100000]:
        for s in range(0, 259):
            ok = bool(lib.hostcheck_fit_slices_legal(nspan, s))
            assert ok == fr.slices_legal(nspan, s), (nspan, s)
            if ok:
                accepted += 1
                assert s <= 256 and nspan * (s - 1) <= extra
                assert s == 1 or nspan * s <= 512 + extra        # (one slice writes no partial sums)
                assert blk * nspan * s <= blk * (nspan + 7 + extra)
    assert accepted > 10000
    for c in fr.normal_cases() + fr.total_cases():
        k = fr.build(c.name)
        for s, _ in c.configs:
            assert s == 0 or fr.slices_legal(k.nspan, s), (c.name, s)


def test_two_stage_total_fits_its_partials():
    lib = load()
    _, _, one, parts = _constants()
    ms = list(range(1, 70000, 7)) + [2048 * k + d for k in (4, 5, 1023, 1024, 1025, 1026) for d in (-1, 0, 1)] + [2 ** e + d for e in range(13, 31) for d in (-1, 0, 1) if 2 ** e + d <= 2 ** 30]
    for m in ms:
        p = lib.hostcheck_fit_total_parts(m)
        assert p == fr.total_parts(m) and 1 <= p <= parts
        assert p * 2048 >= min(m, parts * 2048)                # below the cap every workgroup reads at most 2048 values
    assert fr.total_parts(8193) == 5 and fr.total_parts(fr.BIG_M) == 1024 and -(-fr.BIG_M // 2048) == 1026
    assert one == 8192


# ---- the reference against independent code -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['one-m65', 'two-left1', 'interp-m12', 'off-mid', 'off-above', 'off-below', 'off-last', 'edge-ncoef255'])
def test_exact_normal_equations_against_scipy_design_matrix(name):
    """A^T A and A^T X accumulated exactly from the 50-digit basis (rounded to double: 1 more rounding) against
    scipy.interpolate.BSpline.design_matrix multiplied in numpy, within the fp64 rounding of the latter"""
    from scipy.interpolate import BSpline
    k = fr.build(name)
    q = np.array([[float(v) for v in h] for h in fr.basis50(k.u, k.t)])
    G5, rhs = fr.exact_normal(q, k.X, k.first, 1, 256)
    A = BSpline.design_matrix(k.u, k.t, 3).toarray()
    rows = np.arange(k.u.size)
    for a in range(4):                                         # scipy's basis is this one to its own rounding
        np.testing.assert_allclose(A[rows, k.span + a], q[:, a], rtol=40 * fr.EPS, atol=1e-300)
    AtA, AtX = A.T @ A, A.T @ k.X.T
    assert np.count_nonzero(A) <= 4 * k.u.size
    nmax = 4 * max(int(v) for v in np.diff(k.first)) + 100     # terms of a dot product of numpy, and 2 x 40 for the entries of A
    for j in range(k.ncoef):
        for w in range(4):
            if j - w >= 0:
                v, sa, _ = G5[j][w]
                assert abs(AtA[j, j - w] - float(v)) <= nmax * fr.EPS * float(sa) + 1e-300
            else:
                assert G5[j][w][0] == 0
        assert G5[j][4][0] == 0
        for d in range(3):
            v, sa, _ = rhs[d][j]
            assert abs(AtX[j, d] - float(v)) <= nmax * fr.EPS * float(sa)


def test_exact_btb_against_the_oracle_b_in_numpy():
    for name, ncoef, b in fr.penalty_cases():
        B = np.zeros((b.shape[0], ncoef))
        for it in range(b.shape[0]):
            B[it, it:it + 5] = b[it]
        full = B.T @ B
        ex = fr.exact_btb(b, ncoef)
        for j in range(ncoef):
            for w in range(5):
                v, sa = ex[j][w]
                if j - w >= 0:
                    assert abs(full[j, j - w] - float(v)) <= 8 * fr.EPS * float(sa), (name, j, w)
                else:
                    assert v == 0
    names = [n for n, _, _ in fr.penalty_cases()]
    assert {'fpdisc-n8=%d' % k for k in (1, 2, 3, 4, 5, 6, 251, 252, 253)} <= set(names) and 'random-spread' in names


ALL = [c.name for c in fr.normal_cases() + fr.total_cases()]


@pytest.mark.parametrize('name', ALL)
def test_premises_and_the_two_statements_of_the_span_residual(name):
    """u strictly increasing; no empty span; the spans that hold one sample are the ones the case names; span and first agree; on a
    seeded non-negative `term` the closed rule and fppara's loop give the same rationals, and their sum is the sum of term"""
    k = fr.build(name)
    c = k.case
    assert np.all(np.diff(k.u) > 0) and np.all(np.isfinite(k.X))
    counts = np.diff(k.first)
    assert counts.min() >= 1, 'an empty span'
    assert tuple(np.flatnonzero(counts == 1)) == c.single
    assert not load().hostcheck_fit_samples_knots_wrong(k.u.size, _lib.dptr(k.u), k.n, _lib.dptr(k.t))
    i = np.arange(k.u.size)
    assert np.all(k.first[k.span] <= i) and np.all(i < k.first[k.span + 1])
    assert np.array_equal(np.repeat(np.arange(k.nspan), counts), k.span)
    term = np.random.default_rng(3).uniform(0, 4, k.u.size) ** 3
    a, b = fr.fpint_closed(term, k.first), fr.fpint_fppara(term, k.u, k.t)
    assert a == b
    assert sum(a) == sum(Fraction(float(v)) for v in term)


def test_where_the_samples_sit_against_the_knots():
    """which samples sit on, one ulp below and one ulp above a knot in the off-sample cases, and where the span rules put them"""
    k = fr.build('off-above')
    assert k.t[5] == np.nextafter(k.u[20], np.inf) and k.span[20] == 1 and k.span[21] == 2 and k.first[2] == 21
    assert k.span[10] == 1 and k.first[1] == 10 and k.span[9] == 0                     # a sample on a knot opens its span
    k = fr.build('off-below')
    assert k.t[5] == np.nextafter(k.u[20], -np.inf) and k.span[20] == 2 and k.span[19] == 1 and k.first[2] == 20
    k = fr.build('off-last')
    assert k.t[6] == np.nextafter(k.u[-2], -np.inf) and k.span[-2] == 3 and k.span[-3] == 2 and k.first[3] == 48 and k.span[-1] == 3
    k = fr.build('off-mid')
    assert not np.isin(k.t[4:-4], k.u).any()
    for name in ALL:                                            # the last sample sits on t[n - 4] and belongs to the last span
        k = fr.build(name)
        assert k.u[-1] == k.t[k.n - 4] and k.span[-1] == k.nspan - 1
        on = np.isin(k.u, k.t[4:-4])
        assert np.array_equal(np.flatnonzero(on), k.first[1:-1][np.isin(k.first[1:-1], np.flatnonzero(on))])
    k = fr.build('interp-m300')
    assert k.ncoef == 300 and k.nspan == 297 and fr.fit_slices(k.nspan) == 4
    assert fr.build('edge-nspan511').nspan == 511 and fr.build('edge-nspan512').nspan == 512
    assert fr.build('three-1-2-2997').first.tolist() == [0, 1, 3, 3000]


def test_stride_loops_and_slices_of_the_one_span_case():
    """m = 600 in 1, 2, 3, 7 slices: per = 600, 300, 200, 86 samples a workgroup, 3 / 2 / 1 / 1 passes of the stride loop at NT = 256 and
    10 / 5 / 4 / 2 at NT = 64, the last slice ragged for 7"""
    per = [-(-600 // s) for s in (1, 2, 3, 7)]
    assert per == [600, 300, 200, 86]
    assert [-(-p // 256) for p in per] == [3, 2, 1, 1] and [-(-p // 64) for p in per] == [10, 5, 4, 2]
    assert 600 - 6 * 86 == 84
    assert fr.block_chain(600, 7, 64) == 2 + 6 + 6 and fr.block_chain(600, 1, 256) == 3 + 8


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_before_any_launch():
    """MVUS_E_INVALID without a device (number 99 exists nowhere): every refusal of include/mvus_ba.h; a legal call gets as far as the
    device"""
    import __graft_entry__ as ge
    ge.build()
    lib = _lib.load()
    d = _lib.dptr
    m = 20
    u0, X0 = fr.samples(m, 5)
    t0 = fr.knots(u0, [u0[5], u0[11]])
    n0 = t0.size
    big = 64
    span, q, first = np.zeros(big, np.int32), np.zeros(4 * big), np.zeros(big, np.int64)
    G, Gl, r, rl, c, st = np.zeros(5 * big), np.zeros(5 * big), np.zeros(3 * big), np.zeros(3 * big), np.zeros(3 * big), np.zeros(4)
    term, fp, fpint = np.zeros(big), np.zeros(1), np.zeros(big)
    fail = ctypes.c_int32(0)

    def normal(u=u0, X=X0, t=t0, m=None, n=None, slices=0, parts=0, c_out=c):
        u, X, t = (np.ascontiguousarray(a, dtype=np.float64) if a is not None else None for a in (u, X, t))
        return lib.mvus_spline_fit_normal(99, u.size if m is None else m, d(u) if u is not None else None, d(X) if X is not None else None,
                                          t.size if n is None else n, d(t) if t is not None else None, 0, slices, parts,
                                          span.ctypes.data_as(_lib.c_int32_p), d(q), first.ctypes.data_as(_lib.c_int64_p), d(G), d(Gl), d(r), d(rl),
                                          d(c_out) if c_out is not None else None, d(st), ctypes.byref(fail))

    def residual(u=u0, X=X0, t=t0, m=None, n=None, slices=0, cc=c):
        u, X, t = (np.ascontiguousarray(a, dtype=np.float64) for a in (u, X, t))
        return lib.mvus_spline_fit_residual(99, u.size if m is None else m, d(u), d(X), t.size if n is None else n, d(t), d(cc) if cc is not None else None,
                                            slices, d(term), d(fp), d(fpint))

    def alter(a, i, v):
        a = np.array(a, dtype=np.float64)
        a.flat[i] = v
        return a

    bad = [dict(m=3), dict(u=alter(u0, 7, u0[6])), dict(u=alter(u0, 7, u0[5])), dict(u=alter(u0, 3, np.nan)), dict(X=alter(X0, 30, np.inf)),
           dict(X=alter(X0, 59, np.nan)), dict(t=t0[1:-1], n=7), dict(n=7), dict(t=alter(t0, 2, t0[0] - 1)), dict(t=alter(t0, 3, np.nextafter(t0[3], 1e9))),
           dict(t=alter(t0, n0 - 4, np.nextafter(t0[-1], 0))), dict(t=alter(t0, 5, t0[4])), dict(t=alter(t0, 4, t0[3])), dict(t=alter(t0, 5, t0[-1])),
           dict(t=alter(t0, 4, np.nan)), dict(t=fr.knots(u0, [np.nextafter(u0[5], np.inf), np.nextafter(np.nextafter(u0[5], np.inf), np.inf)])), dict(t=fr.knots(u0, [(u0[5] + u0[6]) / 2, (u0[5] + 3 * u0[6]) / 4])),
           dict(t=fr.knots(u0, u0[1:-1])), dict(slices=-1), dict(slices=257)]
    for kw in bad:
        assert normal(**kw) == _lib.MVUS_E_INVALID, kw
        assert b'spline_fit_normal' in lib.mvus_last_error(None)
        assert residual(**kw) == _lib.MVUS_E_INVALID, kw
        assert b'spline_fit_residual' in lib.mvus_last_error(None)
    for kw in (dict(parts=1), dict(parts=-2), dict(parts=2), dict(parts=257), dict(c_out=None)):        # 6 coefficients: no legal partition
        assert normal(**kw) == _lib.MVUS_E_INVALID, kw
    assert residual(cc=None) == _lib.MVUS_E_INVALID and residual(cc=alter(c, 2, np.nan)) == _lib.MVUS_E_INVALID
    # spans x slices: 1537 spans admit one slice only; 1024 spans two (2048 partial sums) but 1025 spans do not
    for nspan, s, ok in ((1537, 2, False), (1536, 2, False), (1025, 2, False), (1024, 2, True), (3, 256, True), (6, 256, True), (7, 256, False), (7, 220, True), (7, 221, False)):
        assert fr.slices_legal(nspan, s) == ok
    ul, Xl = fr.samples(2200, 6)
    tl = fr.knots(ul, ul[2:2 * 1025:2])
    assert tl.size - 7 == 1025 and residual(u=ul, X=Xl, t=tl, slices=2, cc=np.zeros(3 * (tl.size - 4))) == _lib.MVUS_E_INVALID
    b, B, Bl = np.ones(5 * 10), np.zeros(5 * big), np.zeros(5 * big)
    for args in ((4, 1, d(b)), (10, 0, d(b)), (10, 7, d(b)), (10, 6, None), (10, 6, d(alter(b, 3, np.nan)))):
        assert lib.mvus_spline_fit_penalty(99, args[0], args[1], args[2], 0, d(B), d(Bl)) == _lib.MVUS_E_INVALID
        assert b'spline_fit_penalty' in lib.mvus_last_error(None)
    assert lib.mvus_spline_fit_penalty(99, 10, 6, d(b), 0, None, None) == _lib.MVUS_E_INVALID
    # legal calls reach the device
    assert normal() == _lib.MVUS_E_HIP and normal(slices=256, parts=-1) == _lib.MVUS_E_HIP and residual(slices=3) == _lib.MVUS_E_HIP
    assert lib.mvus_spline_fit_penalty(99, 10, 6, d(b), 1, d(B), None) == _lib.MVUS_E_HIP
