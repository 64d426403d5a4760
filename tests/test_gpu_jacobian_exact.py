"""The kernels' BA residual, analytic Jacobian, motion rows and normal equations against 50-digit arithmetic.

Reads only tests/golden/mp_jacobian.npz (see tests/test_jacobian_exact_host.py for the reference, the cases and the bars: residuals
RESIDUAL_ATOL = 1e-9 px, Jacobian entries TOL = 8 x the fixture's 53-bit floor = 1.52e-10 of the largest reference entry of the
entry's slot group in its own row; ctrl, visibility and cidx equal as integers; no row of a case skipped).  A row the library reports
with ctrl = -1 is a row of zeros by the ABI (its Jacobian storage is not written), so its block is not read here.

The normal equations of the two complete scenes (H put together from the camera blocks, the band and the cross block as
test_gpu_rcs._dense_step does) are compared with the sums formed in mpmath: entries of H relative to sqrt(H_ii H_jj), g relative to
max |g|, the bar 8 x what numpy's own fp64 sums over the reference's rows lose (mp_fixture.normal_floor), for the default window-major
assembly and for the detection-major one (MVUS_NE_FROM_J=1).  Everything is evaluated twice and must give the same bits, except the
detection-major assembly, which adds with fp64 atomics in no fixed order.

Every test prints its measured worsts before it asserts (-s).  On an MI355X: Jacobian 2.8e-12 (sync_off; 9.2e-13 on knots_nonuniform),
motion rows 1.5e-13, residual 1.1e-10 px (geometry), H 9.5e-15 against a bar of 1.12e-14 (full_p15, both assemblies; 1.5e-15 against
1.68e-14 on full_p6), g 2.6e-12 against 1.58e-11.
"""
import numpy as np
import pytest

import mp_fixture as mf
from mvus_amd import _lib

pytestmark = pytest.mark.gpu


def case_names():
    with np.load(mf.PATH) as z:
        return [str(n) for n in z['names']]


@pytest.fixture(scope='module')
def fixture():
    cases, floor = mf.load()
    return cases, mf.TOL_FACTOR * floor


def reference_order(prob, f, rows):
    """ex, ey of the given detections out of a residual vector in the reference's order (per camera: x rows, then y rows)"""
    ex, ey = np.zeros(rows.size), np.zeros(rows.size)
    for k, i in enumerate(rows):
        c = mf.camera_of(prob, i)
        a, b = int(prob.det_offsets[c]), int(prob.det_offsets[c + 1])
        ex[k], ey[k] = f[2 * a + (i - a)], f[2 * a + (b - a) + (i - a)]
    return ex, ey


def evaluate(case):
    from mvus_amd.ba import BAHandle
    p = case.prob
    with BAHandle(p) as h:
        f0 = h.residual(case.x)
        f, J, ctrl = h.residual_jacobian(case.x, _lib.JAC_ANALYTIC)
        motion = h.motion_rows(case.x, _lib.JAC_ANALYTIC) if case.has_motion else None
    return f0, f, J, ctrl, motion


@pytest.mark.parametrize('name', case_names())
def test_gpu_rows_against_50_digits(fixture, name):
    cases, tol = fixture
    case = cases[name]
    p, rows = case.prob, case.rows
    f0, f, J, ctrl, motion = evaluate(case)
    again = evaluate(case)
    vis = case.ctrl >= 0
    assert np.array_equal(ctrl[rows], case.ctrl), (name, rows[ctrl[rows] != case.ctrl])
    worst_res = 0.0
    for fv in (f0, f):
        ex, ey = reference_order(p, fv, rows)
        assert not ex[~vis].any() and not ey[~vis].any(), name
        worst_res = max(worst_res, np.max(np.abs(ex - case.ex)), np.max(np.abs(ey - case.ey)))
    Jr = np.ascontiguousarray(np.transpose(J[:, :, rows], (2, 0, 1)))           # [R, 2, NS]
    Jr[~vis] = 0.0
    ratio = mf.group_ratio(Jr, case.J, p.P, per_row=True)
    print('%-18s residual %.2e px   Jacobian %.2e of the group maximum (row %d)'
          % (name, worst_res, ratio.max(), rows[np.unravel_index(ratio.argmax(), ratio.shape)[0]]))
    assert worst_res <= mf.RESIDUAL_ATOL, (name, worst_res)
    assert ratio.max() <= tol, (name, ratio.max(), tol, np.unravel_index(ratio.argmax(), ratio.shape))
    if case.has_motion:
        mfv, mJ, mctrl = motion
        assert np.array_equal(mctrl.T, case.mcidx), name
        assert np.array_equal(mfv == 0, case.mf == 0)                            # zero rows at the part borders
        assert np.array_equal(f[2 * p.M:], mfv) and np.array_equal(f0[2 * p.M:], mfv)
        mres, mr = np.max(np.abs(mfv - case.mf)), mf.motion_ratio(np.ascontiguousarray(mJ.T), case.mJ)
        print('%-18s motion residual %.2e   Jacobian %.2e of the row maximum' % (name, mres, mr))
        assert mres <= mf.RESIDUAL_ATOL * max(1.0, p.motion_weight) and mr <= tol, (name, mres, mr)
    # twice in a row: the same bits
    assert np.array_equal(f0, again[0]) and np.array_equal(f, again[1]) and np.array_equal(ctrl, again[3])
    live = ctrl >= 0
    assert np.array_equal(J[:, :, live], again[2][:, :, live])
    if case.has_motion:
        assert all(np.array_equal(a, b) for a, b in zip(motion, again[4]))


def dense_normal_equations(prob, ne):
    from test_gpu_schur import internal_index
    g, A, band, cross = ne
    n, C, B, W = prob.n_params, prob.C, 3 + prob.P, band.shape[1]
    N = int(prob.n_coef.sum())
    cam_idx, spl_idx = internal_index(prob)
    H = np.zeros((n, n))
    for c in range(C):
        H[np.ix_(cam_idx[c], cam_idx[c])] = A[c]
    E = cross.reshape(C * B, 3 * N)
    ci = cam_idx.ravel()
    H[np.ix_(ci, spl_idx)] = E
    H[np.ix_(spl_idx, ci)] = E.T
    for w in range(W):
        for gi in range(N - w):
            ri, cj = spl_idx[3 * gi:3 * gi + 3], spl_idx[3 * (gi + w):3 * (gi + w) + 3]
            H[np.ix_(ri, cj)] = band[gi, w]
            if w > 0:
                H[np.ix_(cj, ri)] = band[gi, w].T
    return H, g


@pytest.mark.parametrize('from_j', [False, True], ids=['window_major', 'detection_major'])
@pytest.mark.parametrize('name', ['full_p6', 'full_p15'])
def test_gpu_normal_equations_against_exact_sums(fixture, name, from_j, monkeypatch):
    from mvus_amd.ba import BAHandle
    cases, _ = fixture
    case = cases[name]
    if from_j:
        monkeypatch.setenv('MVUS_NE_FROM_J', '1')
    else:
        monkeypatch.delenv('MVUS_NE_FROM_J', raising=False)
    runs = []
    for _ in range(2):
        with BAHandle(case.prob) as h:
            h.residual_jacobian(case.x, _lib.JAC_ANALYTIC)
            runs.append(h.normal_equations())
            assert h.deterministic_fallback() == from_j
    floor_h, floor_g = mf.normal_floor(case)
    H, g = dense_normal_equations(case.prob, runs[0])
    eh, eg = mf.normal_ratio(H, g, case.H, case.g)
    print('%s %s: H %.2e (floor %.2e, bar %.2e)  g %.2e (floor %.2e, bar %.2e)'
          % (name, 'detection-major' if from_j else 'window-major', eh, floor_h, 8 * floor_h, eg, floor_g, 8 * floor_g))
    assert eh <= mf.TOL_FACTOR * floor_h, (name, eh, floor_h)
    assert eg <= mf.TOL_FACTOR * floor_g, (name, eg, floor_g)
    if not from_j:
        assert all(np.array_equal(a, b) for a, b in zip(runs[0], runs[1]))         # the same bits, run to run
