"""One handle walked through the calls that allocate, regrow and free what it owns -- the pinned partial sums and trial mirrors of an LM
solve, the priors' buffers, the ping-pong detection arrays and temporaries of remove_outliers, the rotation sets and events of the timing
hooks -- and through its own destruction, eight times over.

Every comparison is bit for bit against a FRESH handle brought to the same state, at the same x, and only through calls that carry no
state from earlier calls: residual, robust_cost, position_prior_cost, outlier_mask.  Solves run in between and are not compared.
rs_F_2int_3cam: the smallest golden scene with motion rows."""
import ctypes
import functools

import numpy as np
import pytest

import priors_reference as pref
from golden_util import load_case
from mvus_amd import _lib
from mvus_amd import problem as mp

pytestmark = pytest.mark.gpu

NAME = 'rs_F_2int_3cam'
LM = dict(solver=_lib.SOLVER_LM_SCHUR, jac_mode=_lib.JAC_ANALYTIC, return_fun=False)


@functools.lru_cache(maxsize=None)
def _case():
    """The problem, the point every comparison is made at, the reference's point after its first BA, and two prior sets whose K differ by
    more than a workgroup of k_prior_cost (3 priors: one block of partial sums; 300: two)."""
    scene, g = load_case(NAME)
    prob, _ = mp.problem_from_scene(scene)
    x = np.array(g['x0'] + g['delta'])
    sets = pref.prior_sets(prob, x)
    lo, hi = float(prob.interval[0, 0]), float(prob.interval[1, 0])
    t = lo + (hi - lo) * (np.arange(300) + 0.5) / 300.0
    sigma = 0.01 * pref.scene_size(prob, x)
    P = pref.curve(prob, x, t) + sigma * np.random.default_rng(11).standard_normal((3, t.size))
    big = (t, P, np.full((3, t.size), 1.0 / sigma))
    return prob, x, np.array(g['ba10_x']), float(g['thres_outlier']), g['outlier_keep'], sets['three'], big


def _handle(prob):
    from mvus_amd.ba import BAHandle
    return BAHandle(prob)


def _set(h, pset):
    t, P, w = (np.ascontiguousarray(a, dtype=np.float64) for a in pset)
    h._check(h.lib.mvus_ba_set_position_priors(h.h, t.size, _lib.dptr(t), _lib.dptr(P), _lib.dptr(w)), 'mvus_ba_set_position_priors')


def _same_costs(h, fresh, x, with_priors):
    assert h.robust_cost(x) == fresh.robust_cost(x)
    wa, wb = h.robust_cost(x, weights=True), fresh.robust_cost(x, weights=True)
    assert wa[0] == wb[0] and np.array_equal(wa[1], wb[1])
    if with_priors:
        ca, cb = h.position_prior_cost(x, rows=True), fresh.position_prior_cost(x, rows=True)
        assert ca[0] == cb[0] and ca[0] > 0.0 and np.array_equal(ca[1], cb[1], equal_nan=True)
    else:
        assert h.position_prior_cost(x) == 0.0
    assert np.array_equal(h.residual(x), fresh.residual(x))


def test_priors_set_regrown_and_cleared_behind_solves():
    """1. solve, set priors (K = 3), solve -- the host-summed partials gain the priors' block -- costs; another K (300: one block more),
    solve, costs; clear, solve, costs.  Each time against a fresh handle that only had the same priors set."""
    prob, x, _, _, _, three, big = _case()
    with _handle(prob) as h:
        assert h.T > 0
        xs = h.solve(x, max_nfev=4, **LM).x
        for pset in (three, big):
            _set(h, pset)
            assert h.num_position_priors == pset[0].size and h.num_active_position_priors == pset[0].size
            h.solve(x, max_nfev=3, **LM)
            with _handle(prob) as fresh:
                _set(fresh, pset)
                for at in (x, xs):
                    _same_costs(h, fresh, at, True)
        h.set_position_priors(None, None, None)
        assert h.num_position_priors == 0
        h.solve(xs, max_nfev=2, **LM)
        with _handle(prob) as fresh:
            for at in (x, xs):
                _same_costs(h, fresh, at, False)


def test_remove_outliers_twice_then_mask_and_residual():
    """2. the detection arrays change sets twice; the mask and the residual of what is left are those of a handle built from the filtered
    detections (which never ran remove_outliers)."""
    prob, _, x10, thres, keep_ref, _, _ = _case()
    with _handle(prob) as h:
        h.solve(x10, max_nfev=2, **LM)
        keep1 = h.remove_outliers(x10, thres)
        assert np.array_equal(keep1.astype(np.uint8), keep_ref)
        for thres2 in thres * 0.5 ** np.arange(1, 12):          # the first threshold that takes some of what is left, and not all
            mask = h.outlier_mask(x10, thres2)
            if 0 < mask.sum() < mask.size:
                break
        else:
            pytest.fail('no threshold splits the remaining detections')
        keep2 = h.remove_outliers(x10, thres2)
        print('%s: %d detections, %d left at %g px, %d at %g px' % (NAME, prob.M, keep1.sum(), thres, keep2.sum(), thres2))
        assert np.array_equal(keep2, mask) and keep2.size == keep1.sum() and keep2.sum() == h.M
        with _handle(h.prob) as fresh:
            assert fresh.m == h.m
            assert np.array_equal(h.outlier_mask(x10, 0.5 * thres2), fresh.outlier_mask(x10, 0.5 * thres2))
            assert np.array_equal(h.residual(x10), fresh.residual(x10))
            h.solve(x10, max_nfev=3, **LM)                       # (the Schur workspace is rebuilt on the filtered problem)
            assert np.array_equal(h.residual(x10), fresh.residual(x10))


def test_refused_and_served_timing_calls_leave_the_handle_alone():
    """3. mvus_ba_time_kernel with an unknown kernel returns its error code; the residual after it, and after the hooks that take
    rotation sets and events of their own, is unchanged."""
    prob, x, _, _, _, _, _ = _case()
    with _handle(prob) as h, _handle(prob) as fresh:
        f0 = h.residual(x)
        ms = ctypes.c_double(-1.0)
        assert h.lib.mvus_ba_time_kernel(h.h, 99, 1, ctypes.byref(ms)) == _lib.MVUS_E_INVALID
        assert ms.value == -1.0 and h.lib.mvus_last_error(h.h).decode() == 'bad arguments'
        assert np.array_equal(h.residual(x), f0)
        for which in (0, 1, 5):
            assert h.time_kernel(which, launches=2) > 0.0
        assert h.lib.mvus_ba_time_kernel(h.h, 99, 1, ctypes.byref(ms)) == _lib.MVUS_E_INVALID
        assert np.array_equal(h.residual(x), f0) and np.array_equal(fresh.residual(x), f0)


def test_eight_handles_in_turn():
    """4. created, solved once, destroyed, eight times: the last one's residual is the first one's."""
    prob, x, _, _, _, _, _ = _case()
    first = None
    for k in range(8):
        with _handle(prob) as h:
            h.solve(x, max_nfev=2, **LM)
            f = h.residual(x)
        if first is None:
            first = f
    assert np.array_equal(f, first)
