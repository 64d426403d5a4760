"""What tests/test_gpu_band_solve.py rests on, checked without a GPU: the premises of every system it hands to the band solvers (from
the 50-digit factor: these are conditions, not measurements), the reference against LAPACK, and the invariants of the partition
(band_parts / band_parts_fixed of mvus_amd/csrc/spline_band_parts.h through the host build) for every n the fit can reach in the tests."""
import ctypes

import numpy as np
import pytest

import band_reference as br
from hostcheck_util import load
from mvus_amd import _lib

i32p = lambda a: a.ctypes.data_as(_lib.c_int32_p)          # noqa: E731


def _lib_parts(n, hb, P, min_rows=192):
    out = np.zeros(3, np.int32)
    return tuple(int(v) for v in out) if load().hostcheck_band_parts(n, hb, P, min_rows, i32p(out)) else None


# ---- the partition ------------------------------------------------------------------------------------------------------------------
def test_partition_restatement_is_the_library_rule():
    """band_reference.parts_fixed / parts_rule (what the GPU test sizes its shapes with) against band_parts_fixed / band_parts"""
    for hb in (3, 4):
        for n in list(range(4, 260)) + [699, 700, 701, 2301, 3323, 4000, 163840, 200000]:
            got = _lib_parts(n, hb, 0)
            P = br.parts_rule(n, hb)
            assert got[0] == P, (n, hb)
            if P > 1:
                assert got[1:] == br.parts_fixed(n, hb, P)
            for Pe in (2, 3, 5, 63, 64, 65, 128, 129, 256, 257):
                mine, lib = br.parts_fixed(n, hb, Pe), _lib_parts(n, hb, Pe)
                assert (lib is None) == (mine is None), (n, hb, Pe)
                if mine is not None:
                    assert lib == (Pe,) + mine
    assert _lib_parts(192, 3, 0)[0] == 8 and _lib_parts(192, 4, 0)[0] == 8 and _lib_parts(191, 3, 0)[0] == 1


def test_partition_invariants_for_every_n_and_every_legal_P():
    """n = 16 .. 4000, both HB, the production rule and every legal explicit P: locate() walks interior 0, separator 0, interior 1, .. in
    order and agrees with first() / length() (a bijection of the rows onto interior and separator rows); the partition ends at row n;
    every interior has at least 2 HB rows; the largest at() of every transposed array stays below K (n + kBandPartsMax), the size
    FitWork::alloc gives it.  at() itself is the running count over (i, k, p) -- injective -- walked in full for n <= 400 and every 37th n."""
    lib = load()
    counts = np.zeros(6, np.int64)
    looked = 0
    for n in range(16, 4001):
        for hb in (3, 4):
            lib.hostcheck_band_parts_sweep(n, hb, 192, int(n <= 400 or n % 37 == 0), counts.ctypes.data_as(_lib.c_int64_p))
            legal = sum(br.parts_fixed(n, hb, P) is not None for P in range(2, 257)) + (br.parts_rule(n, hb) > 1)
            assert counts[0] == legal, (n, hb)
            assert not counts[1:].any(), (n, hb, counts)
            looked += int(counts[0])
    assert looked > 1_000_000


@pytest.mark.parametrize('hb', (3, 4))
def test_partition_layout_of_the_gpu_shapes(hb):
    """The same invariants once more for the shapes the GPU test uses, from the raw first / length / locate / at values in numpy, and the
    property each shape is on the list for."""
    lib = load()
    for n, parts, what in br.parts_shapes(hb):
        P = parts if parts else br.parts_rule(n, hb)
        if P == 1:
            assert n == 191
            continue
        ln, rem = br.parts_fixed(n, hb, P)
        first, length, lp, li = (np.zeros(k, np.int32) for k in (P, P, n, n))
        lib.hostcheck_band_layout(n, hb, P, ln, rem, i32p(first), i32p(length), i32p(lp), i32p(li))
        assert first[0] == 0 and np.array_equal(first[1:], (first + length + hb)[:-1]) and first[-1] + length[-1] == n
        assert length.min() >= 2 * hb and set(length) <= {ln, ln + 1} and (length == ln + 1).sum() == rem
        j = np.arange(n)
        assert np.array_equal(first[lp] + li, j) and np.all(np.diff(lp) >= 0) and np.all(li < length[lp] + hb) and np.all(li[lp == P - 1] < length[-1])
        order = br.parts_order(n, hb, P)
        assert np.array_equal(np.sort(order), j) and np.array_equal(order[:length.sum()], j[li < length[lp]])
        for K in (hb + 1, 3, hb):
            pp, ii, kk = np.meshgrid(np.arange(P), np.arange(length.max()), np.arange(K), indexing='ij')
            keep = ii < length[pp]
            pp, ii, kk = (np.ascontiguousarray(a[keep], dtype=np.int32) for a in (pp, ii, kk))
            at = np.zeros(pp.size, np.int64)
            lib.hostcheck_band_at(hb, P, ln, rem, K, pp.size, i32p(pp), i32p(ii), i32p(kk), at.ctypes.data_as(_lib.c_int64_p))
            assert np.unique(at).size == at.size and at.min() >= 0 and at.max() < K * (n + 256)
        if 'shortest' in what:
            assert br.parts_fixed(n - 1, hb, P) is None
        if 'interiors of' in what and 'rows' in what:
            assert length.max() == int(what.split()[2])
        if 'rem=' in what and 'P=5' in what:
            assert rem == int(what.split('=')[-1])
        if '2hb+1' in what:
            assert rem == P - 1 and length.max() == 2 * hb + 1
        elif '2hb' in what:
            assert rem == 0 and ln == 2 * hb
        if what == 'rule, first partitioned':
            assert P == 8
    assert br.parts_rule(191, hb) == 1 and br.parts_fixed(257 * 2 * hb + 256 * hb, hb, 257) is None


def test_every_kernel_meets_every_precision_and_bandwidth():
    """the case list runs k_band_solve and k_band_solve_parts with HB = 3 and 4, and the RB = 8 / RB = 2 batches over interiors shorter
    and longer than one batch, in both precisions (each case runs in fp64 and in double-double)"""
    cases = br.solve_cases()
    for hb in (3, 4):
        assert any(k[2] == hb and parts == -1 for k, parts in cases) and any(k[2] == hb and parts >= 2 for k, parts in cases)
        for fam in 'ABCDEG':
            got = {parts for k, parts in cases if k[0] == fam and k[2] == hb}
            assert {-1, 2, 3} <= got and any(p >= 65 for p in got), (fam, hb)
    assert len(cases) == len(set(cases))
    for key, parts in cases:                                # every explicit partition on the list is one the entry point accepts
        n = br.genuine_operands().n if key[0] == 'G' else key[1]
        assert parts < 2 or br.parts_fixed(n, key[2], parts) is not None, (key, parts)
    print('\n%d band-solve cases x 2 precisions, %d diag-sum cases x 2, %d systems' % (len(cases), len(br.diag_cases()), len(br.all_keys())))


# ---- the systems ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('key', br.all_keys(), ids=lambda k: br.case_id(k))
def test_premises_of_the_system(key):
    """From the 50-digit natural-order factor.  A - C: every exact pivot / diagonal entry is above 1e-11, a decade above the fp64
    pivot_floor; D: at least one is below 1e-13 (a decade under it) and all are above 1e-23 (a decade above the double-double floor).
    max / min of diag(L) is below 1e3 on A and B and above 0.9e5 on C: the fit's switch at 1e4 is no coin toss."""
    fam = key[0]
    s = br.system(key)
    refs = [br.reference(key, True)] + ([br.reference(key, False)] if fam != 'D' else [])
    for r in refs:
        assert r.spd
        if fam in 'ABCEG':
            assert r.ratio_min > 1e-11
        if fam in 'ABE':
            assert r.diag_max / r.diag_min < 1e3
            if fam != 'E':
                assert np.allclose(r.diag, s.L0_diag, rtol=1e-12, atol=0)     # Cholesky is unique: L0 is the factor
        if fam == 'C':
            assert r.diag_max / r.diag_min > 0.9e5
        if fam == 'D':
            assert 1e-23 < r.ratio_min < 1e-13
        if fam == 'G':
            assert r.diag_max / r.diag_min < 1e3
    if fam == 'E':
        assert np.all(s.G5[s.zeroed] == 0) and np.all(s.rhs[:, s.zeroed] == 0) and np.all(refs[0].c64[:, s.zeroed] == 0)
    # the low words are low words: hi + lo does not round away from hi
    assert np.all(s.G5 + s.G5_lo == s.G5) and np.all(s.rhs + s.rhs_lo == s.rhs)
    assert np.all(s.G5[:, 4] == 0) or s.hb == 4 and fam == 'G'
    for j in range(min(s.hb, s.n)):                         # nothing outside the matrix
        assert np.all(s.G5[j, j + 1:] == 0) and (s.BtB is None or np.all(s.BtB[j, j + 1:] == 0))


@pytest.mark.parametrize('key', [k for k in br.all_keys() if k[0] == 'C' and k[2] in (3, 4)], ids=lambda k: br.case_id(k))
def test_family_C_keeps_its_pivots_in_the_partitioned_order_too(key):
    """fail_out must stay 0 on family C in every elimination order the GPU test runs: the pivots of the permuted matrix (fp64 dense
    Cholesky; at these ratios good to 1e-5) over their diagonal entries stay above 1e-11 as well."""
    M = br.dense(key)
    for parts in sorted({p for k, p in br.solve_cases() if k == key and p >= 2}):
        order = br.parts_order(key[1], key[2], parts)
        d = br.permuted_diag(key, parts)
        assert (d * d / M.diagonal()[order]).min() > 1e-11, parts


@pytest.mark.parametrize('key', [k for k in br.all_keys() if k[0] == 'A' and k[1] in (8, 65, 191, 700)], ids=lambda k: br.case_id(k))
def test_reference_agrees_with_lapack(key):
    """the 50-digit solve of the fp64 system against scipy.linalg.solveh_banded (dpbsv), to that routine's own accuracy 2 kappa k eps"""
    from scipy.linalg import solveh_banded
    s, r = br.system(key), br.reference(key, False)
    band = s.G5 if s.BtB is None else s.G5 + s.pinv ** 2 * s.BtB
    ab = np.zeros((s.hb + 1, s.n))
    for w in range(s.hb + 1):
        ab[w, :s.n - w] = band[w:, w]                       # LAPACK's lower form: M(j + w, j) at [w, j]
    x = solveh_banded(ab, s.rhs.T, lower=True).T
    bar = 2 * br.kappa_inf(key) * br.kbar(s.hb) * br.EPS
    assert br.forward_error(r, x) <= bar
    assert br.backward_error(r, x) <= br.kbar(s.hb) * br.EPS
    assert br.backward_error(r, r.c64) <= br.EPS and br.forward_error(r, r.c64) <= br.EPS       # the reference rounded to double
    if s.n <= 65:
        assert abs(br.kappa_inf_mp(r) / br.kappa_inf(key) - 1) < 1e-8
        d = br.permuted_diag(key, 2) if br.parts_fixed(s.n, s.hb, 2) else None
        if d is not None:                                  # block elimination is the Cholesky of the permuted matrix: same determinant
            assert abs(np.log(d).sum() - np.log(r.diag).sum()) < 1e-10


def test_jump_matrix_restatement_is_the_library_fpdisc():
    g = br.genuine_operands()
    b = np.zeros_like(g.b)
    load().hostcheck_fpdisc(g.t.size, _lib.dptr(g.t), _lib.dptr(b))
    np.testing.assert_array_equal(b, g.b)
    # and B^T B is what its name says
    B = np.zeros((g.b.shape[0], g.n))
    for it in range(g.b.shape[0]):
        B[it, it:it + 5] = g.b[it]
    full = B.T @ B
    for w in range(5):
        np.testing.assert_allclose(g.BtB[w:, w], np.diagonal(full, -w), rtol=1e-13, atol=1e-13 * np.abs(full).max())


def test_entry_points_refuse_before_any_launch():
    """MVUS_E_INVALID without a device: n < 4, hb not 3 or 4, an illegal explicit partition, NULL pointers, BtB with hb = 3."""
    import __graft_entry__ as ge
    ge.build()
    lib = _lib.load()
    n = 40
    G, r, c, st = np.zeros((n, 5)), np.zeros((3, n)), np.zeros((3, n)), np.zeros(4)
    fail, P = ctypes.c_int32(0), ctypes.c_int32(0)
    d = _lib.dptr

    def call(n=n, hb=3, parts=-1, G5=d(G), BtB=None, rhs=d(r), c_out=d(c), stats=d(st), fail_out=ctypes.byref(fail), P_out=ctypes.byref(P), pinv=0.5):
        return lib.mvus_spline_band_solve(99, n, hb, 0, parts, G5, None, BtB, None, pinv, rhs, None, c_out, stats,
                                          ctypes.cast(fail_out, _lib.c_int32_p) if fail_out else None, ctypes.cast(P_out, _lib.c_int32_p) if P_out else None)

    bad = [dict(n=3), dict(n=0), dict(hb=2), dict(hb=5), dict(BtB=d(G)), dict(hb=4), dict(hb=4, BtB=d(G), pinv=float('nan')), dict(parts=1), dict(parts=-2),
           dict(parts=257), dict(parts=5), dict(hb=4, BtB=d(G), parts=4), dict(G5=None), dict(rhs=None), dict(c_out=None), dict(stats=None),
           dict(fail_out=None), dict(P_out=None)]
    for kw in bad:
        assert call(**kw) == _lib.MVUS_E_INVALID, kw
        assert b'spline_band_solve' in lib.mvus_last_error(None)
    assert br.parts_fixed(n, 3, 4) is not None and br.parts_fixed(n, 3, 5) is None and br.parts_fixed(n, 4, 4) is None
    out = np.zeros(1)
    for args in ((3, 0, d(G), None, d(out)), (n, 0, None, None, d(out)), (n, 1, d(G), None, None)):
        assert lib.mvus_spline_band_diag_sum(99, *args) == _lib.MVUS_E_INVALID
        assert b'spline_band_diag_sum' in lib.mvus_last_error(None)
    # a legal call gets as far as the device (number 99 does not exist anywhere): nothing above was refused for the wrong reason
    assert call(parts=4) == _lib.MVUS_E_HIP and call(hb=4, BtB=d(G), parts=3) == _lib.MVUS_E_HIP
    assert lib.mvus_spline_band_diag_sum(99, n, 0, d(G), None, d(out)) == _lib.MVUS_E_HIP
