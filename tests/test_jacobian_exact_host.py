"""The BA residual and analytic Jacobian of mvus_amd/csrc/ba_math.h (host build, tests/hostcheck) against 50-digit arithmetic.

The reference is tests/golden/mp_jacobian.npz: rows of tests/mp_observation.py (mpmath, forward-mode dual numbers, written from the
reference's semantics and sharing no code with ba_math.h or the oracle) at the edges listed in tests/golden/make_golden_mp_jacobian.py.
No row of a case is skipped; ctrl and visibility must be equal as integers; residuals meet RESIDUAL_ATOL = 1e-9 px; every Jacobian
entry meets  |J - J_ref| <= TOL max |J_ref|  over the entry's slot group of its own row (sync / intrinsics / rvec / t / distortion /
spline), not over a whole column.

    floor  1.905e-11   worst such ratio of the restatement itself at mpmath precision 53 against itself at 50 digits, over the cases
                       with |rvec| >= 0.1 (set by knots_nonuniform: sum_q c_q B'_q(tau) on knots 0.01 apart cancels ~5 digits)
    TOL    1.524e-10   8 x floor, the same for every case, small rotation angles included
    host build, measured worst:  Jacobian 4.9e-12 (sync_off; 1.1e-12 on knots_nonuniform), motion rows 1.9e-13, residual 1.1e-10 px
                       (geometry: pixels of ~1e3 at depth 0.1), rotation sweep 5.7e-15.  With W formed as
                       R (v v^T + (R^T - I)[v]x) / |v|^2 at every angle: 3.9e-9 at |rvec| = 1e-8 (25 x TOL), 6.3e-11 at 1e-6,
                       3.9e-11 at 1e-10 -- the cancellation the series branch of `rodrigues` removes.
"""
import numpy as np
import pytest

import mp_fixture as mf
from mvus_amd import _lib

FLOOR_RECORDED = 1.905e-11      # the fixture's floor, to three digits up: the test below keeps the file and this text together
SUBSET = ('rot_1e-8', 'rot_1', 'knots_nonuniform', 'dist_reset', 'motion_F')      # re-generated bit for bit when mpmath is there


@pytest.fixture(scope='module')
def fixture():
    cases, floor = mf.load()
    assert floor <= FLOOR_RECORDED * (1 + 1e-3) and floor >= FLOOR_RECORDED * (1 - 1e-3)
    return cases, mf.TOL_FACTOR * floor


@pytest.fixture(scope='module')
def hostlib():
    import hostcheck_util
    return hostcheck_util.load()


def case_names():
    with np.load(mf.PATH) as z:
        return [str(n) for n in z['names']]


def check_rows(case, ex, ey, ctrl, J, tol, what):
    """ex, ey, ctrl [R], J [R, 2, NS] of the case's rows against the reference; returns the measured worsts."""
    assert np.array_equal(ctrl, case.ctrl), (what, case.name, np.nonzero(ctrl != case.ctrl)[0])
    vis = case.ctrl >= 0
    assert not ex[~vis].any() and not ey[~vis].any() and not J[~vis].any(), (what, case.name)
    res = max(np.max(np.abs(ex - case.ex)), np.max(np.abs(ey - case.ey)))
    ratio = mf.group_ratio(J, case.J, case.prob.P, per_row=True)
    print('%-6s %-18s residual %.2e px   Jacobian %.2e of the group maximum (row %d)'
          % (what, case.name, res, ratio.max(), case.rows[np.unravel_index(ratio.argmax(), ratio.shape)[0]]))
    assert res <= mf.RESIDUAL_ATOL, (what, case.name, res)
    assert ratio.max() <= tol, (what, case.name, ratio.max(), tol, np.unravel_index(ratio.argmax(), ratio.shape))
    return res, float(ratio.max())


def rows_from_dense(case, f, Jd):
    """ex, ey, ctrl, J[R, 2, NS] of the case's rows out of a dense Jacobian; ctrl is read off the support of the row: the reference's
    first control point when the row's non-zeros lie in its slot columns, -2 when something sits outside them."""
    p = case.prob
    NS = 3 + p.P + 12
    R = case.rows.size
    ex, ey, ctrl, J = np.zeros(R), np.zeros(R), np.full(R, -1, dtype=np.int32), np.zeros((R, 2, NS))
    for k, i in enumerate(case.rows):
        c = mf.camera_of(p, i)
        a, b = int(p.det_offsets[c]), int(p.det_offsets[c + 1])
        rx, ry = 2 * a + (i - a), 2 * a + (b - a) + (i - a)
        ex[k], ey[k] = f[rx], f[ry]
        if not (Jd[rx].any() or Jd[ry].any() or f[rx] or f[ry]):
            continue
        g = int(case.ctrl[k])
        if g < 0:
            ctrl[k] = -2
            continue
        cols = mf.slot_columns(p, c, g)
        rest = np.ones(p.n_params, dtype=bool)
        rest[cols] = False
        ctrl[k] = g if not (Jd[rx, rest].any() or Jd[ry, rest].any()) else -2
        J[k, 0], J[k, 1] = Jd[rx, cols], Jd[ry, cols]
    return ex, ey, ctrl, J


@pytest.mark.parametrize('name', case_names())
def test_host_rows_against_50_digits(fixture, hostlib, name):
    from hostcheck_util import HostHandle
    from test_device_math_host import host_eval
    cases, tol = fixture
    case = cases[name]
    p = case.prob
    # the problem as the library holds it (interval records + span look-up table: locate_span's fast path and its re-search)
    h = HostHandle(p)
    f, Jd = h.dense_jacobian(case.x, _lib.JAC_ANALYTIC)
    check_rows(case, *rows_from_dense(case, f, Jd), tol, 'handle')
    if case.has_motion:
        T = case.mf.size
        assert h.T == T
        mres = np.max(np.abs(f[2 * p.M:] - case.mf))
        ref = mf.motion_dense(case, case.mJ, case.mcidx)
        mr = mf.motion_ratio(Jd[2 * p.M:], ref)
        print('motion %-18s residual %.2e   Jacobian %.2e of the row maximum' % (name, mres, mr))
        assert np.array_equal(f[2 * p.M:] == 0, case.mf == 0)                 # zero rows at the part borders
        assert np.array_equal(Jd[2 * p.M:].any(axis=1), case.mcidx[:, 0] >= 0)
        assert mres <= mf.RESIDUAL_ATOL * max(1.0, p.motion_weight) and mr <= tol, (name, mres, mr)
    h.close()
    # the bare row function (binary searches, no tables); it has no switch for opt_sync
    if p.opt_sync:
        ex, ey, ctrl, J = host_eval(hostlib, p, case.x)
        check_rows(case, ex[case.rows], ey[case.rows], ctrl[case.rows], J[case.rows], tol, 'eval')


@pytest.mark.parametrize('name', ['full_p6', 'full_p15'])
def test_host_normal_equations_against_exact_sums(fixture, name):
    """numpy's J^T J and J^T f of the host build's rows against the sums formed in mpmath; the bar is 8 x the error numpy makes on the
    reference's own rows (mp_fixture.normal_floor)."""
    from hostcheck_util import HostHandle
    cases, _ = fixture
    case = cases[name]
    floor_h, floor_g = mf.normal_floor(case)
    h = HostHandle(case.prob)
    f, Jd = h.dense_jacobian(case.x, _lib.JAC_ANALYTIC)
    h.close()
    eh, eg = mf.normal_ratio(Jd.T @ Jd, Jd.T @ f, case.H, case.g)
    print('%s: H %.2e (floor %.2e)  g %.2e (floor %.2e)' % (name, eh, floor_h, eg, floor_g))
    assert eh <= mf.TOL_FACTOR * floor_h and eg <= mf.TOL_FACTOR * floor_g


def test_rodrigues_small_angle_sweep(fixture):
    """|rvec| swept across the series branch of `rodrigues` and its seam: every magnitude meets the one TOL.  (With W formed as
    R (v v^T + (R^T - I)[v]x) / |v|^2 at every angle the sweep peaks at 3.7e-9, at |rvec| = 1e-8; now 5.7e-15.)"""
    mpmath = pytest.importorskip('mpmath')
    import mp_observation as mo
    from hostcheck_util import HostHandle
    cases, tol = fixture
    case = cases['rot_1']
    p = case.prob
    o = 3 * p.C + 4
    rows = [int(r) for r in case.rows[case.rows < p.det_offsets[1]][[2, 9, 15]]]
    axis = np.array([0.6, -0.48, 0.64])
    seam = 1e-2                                  # kRodriguesSeries of ba_math.h
    mags = np.concatenate((10.0 ** np.linspace(-13, -0.5, 51), seam * (1 + np.array([-1e-3, -1e-9, 0, 1e-9, 1e-3]))))
    h = HostHandle(p)
    worst = (0.0, 0.0)
    for m in np.sort(mags):
        x = case.x.copy()
        x[o:o + 3] = m * axis
        f, Jd = h.dense_jacobian(x, _lib.JAC_ANALYTIC)
        for i in rows:
            with mpmath.workdps(mo.DPS):
                r = mo.detection_row(p, x, i)
            assert r['ctrl'] >= 0
            cols = mf.slot_columns(p, 0, r['ctrl'])
            a, b = int(p.det_offsets[0]), int(p.det_offsets[1])
            J = np.stack((Jd[2 * a + (i - a), cols], Jd[2 * a + (b - a) + (i - a), cols]))
            Jref = np.array([[float(v) for v in r['jx']], [float(v) for v in r['jy']]])
            ratio = mf.group_ratio(J, Jref, p.P)
            worst = max(worst, (ratio, m))
            assert abs(f[2 * a + (i - a)] - float(r['ex'])) <= mf.RESIDUAL_ATOL
    h.close()
    print('sweep: worst %.2e of the group maximum at |rvec| = %.3e (TOL %.2e)' % (worst + (tol,)))
    assert worst[0] <= tol, worst


def test_generator_reproduces_the_fixture_and_its_floor():
    """A fresh run of the generator on a fixed subset: the inputs it builds are the file's (integers exactly, floating-point inputs to
    1e-9 -- they pass through numpy's sin / cos and LAPACK, whose last bits depend on the CPU), the reference arrays computed afresh from
    the file's inputs are the file's bit for bit, and the 53-bit floor measured now is not above the recorded one."""
    pytest.importorskip('mpmath')
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
    import make_golden_mp_jacobian as gen
    assert tuple(gen.SUBSET) == SUBSET
    with np.load(mf.PATH) as z:
        stored = {k: z[k] for k in z.files}
    cases, recorded = mf.load(names=SUBSET)
    floor = 0.0
    for name in SUBSET:
        built = gen.build(name)
        for k, v in gen.pack(name, built, {}).items():
            v = np.asarray(v)
            assert v.shape == stored[k].shape and v.dtype == stored[k].dtype, k
            if v.dtype.kind == 'f':
                assert np.allclose(v, stored[k], rtol=1e-9, atol=1e-9), k
            else:
                assert np.array_equal(v, stored[k]), k
        c = cases[name]
        case = dict(prob=c.prob, x=c.x, rows=c.rows, in_floor=c.in_floor, full=c.full)
        fresh = gen.pack(name, case, gen.reference(case))
        assert set(fresh) == {k for k in stored if k.startswith(name + '/')}
        for k, v in fresh.items():
            assert np.array_equal(np.asarray(v), stored[k]) and np.asarray(v).dtype == stored[k].dtype, k
        if c.in_floor:
            floor = max(floor, float(fresh[name + '/floor']))
    assert floor <= recorded * 1.0
    assert floor == recorded                      # (the subset holds the case that sets the floor)
