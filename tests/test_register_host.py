"""Registering a camera against a held trajectory, the parts that need no GPU: the damped Cholesky solve of ba_register_math.h against a
50-digit solve, its `decide` function against a restatement written here, the whole host loop against scipy's least_squares, and the
bindings, argument checks and settings."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import register_cases as rc
import register_hostcheck_util as ru
from frozen_util import build_scene
from golden_util import load_case
from mvus_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. damped Cholesky solve -----------------------------------------------------------------------------------------------------
def _spd(n, kind, rng):
    """(H, g, lambda) of one test system: H = J^T J style, symmetric."""
    if kind == 'well':
        J = rng.normal(size=(4 * n, n))
        return J.T @ J, rng.normal(size=n), 1e-3
    Q, _ = np.linalg.qr(rng.normal(size=(n, n)))
    if kind == 'cond1e10':                                       # Jacobi-scaled condition about 1e10, columns of very different size on top
        A = Q @ np.diag(np.logspace(0, -10, n)) @ Q.T
        A = 0.5 * (A + A.T)
        s = 10.0 ** rng.uniform(-3, 3, n)
        return A * np.outer(s, s), rng.normal(size=n) * s, 1e-13
    J = rng.normal(size=(4 * n, n))
    H, g = J.T @ J, rng.normal(size=n)
    k = n // 2
    H[k, :] = 0.0
    H[:, k] = 0.0
    if kind == 'frozen':                                         # a held entry: row and column zero, H_kk = 1, g_k = 0
        H[k, k], g[k] = 1.0, 0.0
    else:                                                        # 'zero_diag': a switched-off entry, H_kk = 0 -> D_k = 1
        g[k] = 0.5
    return H, g, 1e-3


@pytest.mark.parametrize('n', [9, 18])
@pytest.mark.parametrize('kind', ['well', 'cond1e10', 'frozen', 'zero_diag'])
def test_damped_cholesky_against_50_digits(n, kind):
    """1. (H + lambda D) p = -g by reg_damped_solve against mpmath at 50 digits; bar: 8 x the error of numpy.linalg.solve in fp64 on the
    same system, both measured as |dp_k| sqrt(D_k) relative to max_k |p_k| sqrt(D_k)."""
    H, g, lam = _spd(n, kind, np.random.default_rng(100 * n + len(kind)))
    D = np.where(np.diag(H) > 0, np.diag(H), 1.0)
    code, p = ru.damped_solve(H, g, lam)
    assert code == 0
    ref = ru.mp_damped_solve(H, g, lam)
    err = ru.scaled_error(p, ref, D)
    err_np = ru.scaled_error(np.linalg.solve(H + lam * np.diag(D), -g), ref, D)
    print('n=%d %s: cholesky %.3e numpy %.3e' % (n, kind, err, err_np))
    assert err <= 8.0 * err_np
    if kind == 'frozen':
        assert p[n // 2] == 0.0


@pytest.mark.parametrize('n', [9, 18])
def test_indefinite_matrix_returns_the_failure_code(n):
    rng = np.random.default_rng(n)
    Q, _ = np.linalg.qr(rng.normal(size=(n, n)))
    ev = np.linspace(1.0, 2.0, n)
    ev[n // 3] = -0.5
    H = Q @ np.diag(ev) @ Q.T
    H = 0.5 * (H + H.T)
    code, p = ru.damped_solve(H, rng.normal(size=n), 1e-3)
    assert code == 1 and np.all(np.isnan(p))                    # the failure code, not numbers
    code, p = ru.damped_solve(np.zeros((n, n)), np.ones(n), 0.0)      # H = 0 without damping: a zero pivot
    assert code == 1


def test_packed_triangle_indexing():
    lib = ru.load()
    seen = {}
    for j in range(18):
        for i in range(j + 1):
            e = lib.regcheck_tri_index(i, j)
            assert e == lib.regcheck_tri_index(j, i) and e not in seen
            seen[e] = (i, j)
            a, b = ctypes.c_int(), ctypes.c_int()
            lib.regcheck_tri_entry(e, ctypes.byref(a), ctypes.byref(b))
            assert (a.value, b.value) == (i, j)
    assert sorted(seen) == list(range(171))


# ---- 2. decide ----------------------------------------------------------------------------------------------------------------------
def _decide_py(lam, nu, cost, trial, nfev, max_nfev, ftol, xtol, lambda_min, cost_new):
    """The rules of lm_schur for one evaluated trial, restated: returns (accept, lam, nu, cost, nfev, status, done)."""
    gp, pDp, s2, x2 = trial
    nfev += 1
    accept, status, done = False, 0, False
    if not math.isfinite(cost_new):
        lam = lam * nu
        nu = nu * 2.0
        if lam > 1e12:
            status, done = 0, True
    else:
        predicted = 0.5 * (lam * pDp - gp)
        actual = cost - cost_new
        ratio = actual / predicted if predicted > 0 else (1.0 if actual > 0 else 0.0)
        f_ok = actual < ftol * cost and ratio > 0.25
        x_ok = math.sqrt(s2) < xtol * (xtol + math.sqrt(x2))
        term = 4 if (f_ok and x_ok) else 2 if f_ok else 3 if x_ok else -1
        if actual > 0:
            t = 2.0 * ratio - 1.0
            lam = lam * max(1.0 / 3.0, 1.0 - t * t * t)
            lam = max(lam, lambda_min)
            nu = 2.0
            cost = cost_new
            accept = True
        else:
            lam = lam * nu
            nu = nu * 2.0
        if term != -1:
            status, done = term, True
    if not done and nfev >= max_nfev:
        status, done = 0, True
    return accept, lam, nu, cost, nfev, status, done


# (lam, nu, cost, trial = [g.step, step^T D step, |step|^2, |x|^2], nfev, max_nfev, ftol, xtol, lambda_min, cost_new)
DECIDE_CASES = {
    'accept': (1e-3, 2.0, 100.0, [-20.0, 5.0, 1.0, 50.0], 3, 50, 1e-8, 1e-12, 0.0, 91.0),
    'accept_poor_ratio': (1e-3, 4.0, 100.0, [-20.0, 5.0, 1.0, 50.0], 3, 50, 1e-8, 1e-12, 0.0, 99.0),
    'reject': (1e-3, 2.0, 100.0, [-20.0, 5.0, 1.0, 50.0], 3, 50, 1e-8, 1e-12, 0.0, 104.0),
    'reject_again': (4e-3, 8.0, 100.0, [-20.0, 5.0, 1.0, 50.0], 7, 50, 1e-8, 1e-12, 0.0, 100.0),
    'nonfinite_inf': (1e-3, 2.0, 100.0, [-20.0, 5.0, 1.0, 50.0], 3, 50, 1e-8, 1e-12, 0.0, float('inf')),
    'nonfinite_nan': (1e-3, 4.0, 100.0, [-20.0, 5.0, 1.0, 50.0], 3, 50, 1e-8, 1e-12, 0.0, float('nan')),
    'status2_ftol': (1e-3, 2.0, 100.0, [-2e-7, 1e-8, 1e-9, 50.0], 3, 50, 1e-8, 1e-12, 0.0, 100.0 - 0.9e-7),
    'status3_xtol': (1e-3, 2.0, 100.0, [-20.0, 5.0, 1e-30, 50.0], 3, 50, 1e-8, 1e-12, 0.0, 91.0),
    'status3_xtol_on_a_rejected_step': (1e-3, 2.0, 100.0, [-20.0, 5.0, 1e-30, 50.0], 3, 50, 1e-8, 1e-12, 0.0, 101.0),
    'status4_both': (1e-3, 2.0, 100.0, [-2e-7, 1e-8, 1e-30, 50.0], 3, 50, 1e-8, 1e-12, 0.0, 100.0 - 0.9e-7),
    'max_nfev_on_accept': (1e-3, 2.0, 100.0, [-20.0, 5.0, 1.0, 50.0], 49, 50, 1e-8, 1e-12, 0.0, 91.0),
    'max_nfev_on_reject': (1e-3, 2.0, 100.0, [-20.0, 5.0, 1.0, 50.0], 49, 50, 1e-8, 1e-12, 0.0, 104.0),
    'lambda_over_1e12': (0.9e12, 2.0, 100.0, [-20.0, 5.0, 1.0, 50.0], 3, 50, 1e-8, 1e-12, 0.0, float('inf')),
    'lambda_floor': (4e-3, 2.0, 100.0, [-20.0, 5.0, 1.0, 50.0], 3, 50, 1e-8, 1e-12, 3e-3, 90.002),
    'predicted_not_positive': (1e-3, 2.0, 100.0, [20.0, 5.0, 1.0, 50.0], 3, 50, 1e-8, 1e-12, 0.0, 99.0),
}


@pytest.mark.parametrize('name', sorted(DECIDE_CASES))
def test_decide_against_the_restatement(name):
    """2. Integers and booleans equal; lambda, nu and the cost bit-equal (a handful of fp64 operations in a fixed order)."""
    lam, nu, cost, trial, nfev, max_nfev, ftol, xtol, lmin, cost_new = DECIDE_CASES[name]
    want = _decide_py(lam, nu, cost, trial, nfev, max_nfev, ftol, xtol, lmin, cost_new)
    got = ru.decide(lam, nu, cost, trial, nfev, max_nfev, ftol, xtol, 1e-8, lmin, cost_new)
    assert (got.accept, got.nfev, got.status, got.done) == (want[0], want[4], want[5], want[6])
    assert got.lam.tobytes() == np.float64(want[1]).tobytes() and got.nu.tobytes() == np.float64(want[2]).tobytes()
    assert got.cost.tobytes() == np.float64(want[3]).tobytes()


def test_decide_cases_cover_what_they_name():
    """The table above reaches, in the LIBRARY's function, every outcome it is there for."""
    def lib_out(v):
        lam, nu, cost, trial, nfev, max_nfev, ftol, xtol, lmin, cost_new = v
        r = ru.decide(lam, nu, cost, trial, nfev, max_nfev, ftol, xtol, 1e-8, lmin, cost_new)
        return r.accept, r.lam, r.nu, r.cost, r.nfev, r.status, r.done
    out = {k: lib_out(v) for k, v in DECIDE_CASES.items()}
    assert out['accept'][0] and not out['accept'][6] and out['accept'][1] < 1e-3
    assert not out['reject'][0] and out['reject'][1] == 2e-3 and out['reject'][2] == 4.0
    assert not out['nonfinite_inf'][0] and not out['nonfinite_inf'][6] and out['nonfinite_nan'][1] == 4e-3
    assert [out[k][5] for k in ('status2_ftol', 'status3_xtol', 'status3_xtol_on_a_rejected_step', 'status4_both')] == [2, 3, 3, 4]
    assert all(out[k][6] for k in ('status2_ftol', 'status3_xtol', 'status3_xtol_on_a_rejected_step', 'status4_both'))
    assert out['max_nfev_on_accept'][5:] == (0, True) and out['max_nfev_on_accept'][0] and out['max_nfev_on_reject'][5:] == (0, True)
    assert out['lambda_over_1e12'][5:] == (0, True) and out['lambda_over_1e12'][1] > 1e12
    assert out['lambda_floor'][0] and out['lambda_floor'][1] == 3e-3
    assert out['predicted_not_positive'][0]


# ---- 2b. the whole round: gradient test, blocked rs, solve with retries -------------------------------------------------------------------
def _damp(h):
    return h if h > 0 else 1.0


def _solve_py(n, H, g, lam, skip):
    """reg_damped_solve restated operation by operation (Python floats are IEEE doubles; the host build has no fused multiply-add): the
    upper factor column by column, then the two triangular solves.  None on a pivot that is not positive."""
    U = [[0.0] * n for _ in range(n)]
    for j in range(n):
        for i in range(j + 1):
            s = H[i][j]
            if i in skip or j in skip:
                s = 1.0 if i == j else 0.0
            if i == j:
                s += lam * _damp(s)
            for k in range(i):
                s -= U[k][i] * U[k][j]
            if i == j:
                if not s > 0:
                    return None
                U[j][j] = math.sqrt(s)
            else:
                U[i][j] = s / U[i][i]
    p = [0.0] * n
    for i in range(n):
        s = 0.0 if i in skip else -g[i]
        for k in range(i):
            s -= U[k][i] * p[k]
        p[i] = s / U[i][i]
    for i in range(n - 1, -1, -1):
        s = p[i]
        for k in range(i + 1, n):
            s -= U[i][k] * p[k]
        p[i] = s / U[i][i]
    return p


def _blocked(x, g, boxed):
    return boxed and ((x[2] <= 0.0 and g[2] > 0) or (x[2] >= 1.0 and g[2] < 0))


def _round_py(n, first, last, max_nfev, ftol, xtol, gtol, lambda0, lambda_min, held, boxed, nfree, lin_H, lin_g, lin_cost2, lin_vis, st, x, xt, H, g):
    """reg_round restated: the rules of lm_schur between two evaluations of one problem."""
    st = dict(st, trial=list(st['trial']))
    x, xt, g = list(map(float, x)), list(map(float, xt)), list(map(float, g))
    H = [list(map(float, r)) for r in H]
    if not first and st['done']:
        return st, x, xt, H, g
    cost_new = 0.5 * lin_cost2
    if first:
        st = dict(lam=max(lambda0 if lambda0 > 0 else 1e-4, lambda_min), nu=2.0, cost=cost_new, cost0=cost_new, trial=[0.0] * 4, nfev=1, status=0, done=False)
        if not math.isfinite(cost_new) or 2 * lin_vis < nfree:
            st['status'], st['done'] = -1, True
        adopt = True
    else:
        adopt, st['lam'], st['nu'], st['cost'], st['nfev'], status, done = _decide_py(st['lam'], st['nu'], st['cost'], st['trial'], st['nfev'], max_nfev,
                                                                                         ftol, xtol, lambda_min, cost_new)
        if done:
            st['status'], st['done'] = status, True
    if adopt:
        x = list(xt)
        g = [0.0 if k in held else float(lin_g[k]) for k in range(n)]
        H = [[(1.0 if i == j else 0.0) if (i in held or j in held) else float(lin_H[i][j]) for j in range(n)] for i in range(n)]
    if st['done']:
        return st, x, xt, H, g
    gnorm = max([0.0] + [abs(g[i]) for i in range(n) if not (i == 2 and _blocked(x, g, boxed))])
    if gnorm < gtol:
        st['status'], st['done'] = 1, True
        return st, x, xt, H, g
    if st['nfev'] >= max_nfev:
        st['status'], st['done'] = 0, True
        return st, x, xt, H, g
    if last:
        return st, x, xt, H, g
    skip = {2} if _blocked(x, g, boxed) else set()
    while not st['done']:
        p = _solve_py(n, H, g, st['lam'], skip)
        if p is not None:
            bad = not all(math.isfinite(v) for v in p)
            gp = pDp = s2 = x2 = 0.0
            new = []
            for i in range(n):
                xn = x[i] if bad else (min(max(x[i] + p[i], 0.0), 1.0) if (boxed and i == 2) else x[i] + p[i])
                step = xn - x[i]
                new.append(xn)
                gp += g[i] * step
                pDp += step * _damp(H[i][i]) * step
                s2 += step * step
                x2 += x[i] * x[i]
            xt = new
            st['trial'] = [float('nan') if bad else gp, pDp, s2, x2]
            if math.isfinite(st['trial'][0]) and math.isfinite(st['trial'][1]):
                break
        st['lam'] = st['lam'] * 10.0
        if st['lam'] > 1e12:
            st['status'], st['done'] = 0, True
    return st, x, xt, H, g


def _round_cases():
    """name -> arguments of a round (n = 9, rs is entry 2).  H0 = a well-conditioned J^T J."""
    rng = np.random.default_rng(2)
    n = 9
    J = rng.normal(size=(40, n))
    H0, g0 = J.T @ J, rng.normal(size=n) * 5.0
    x0 = rng.normal(size=n)
    x0[2] = 0.4
    opts = dict(max_nfev=50, ftol=1e-8, xtol=1e-12, gtol=1e-8, lambda0=0.0, lambda_min=0.0)
    fresh = dict(lam=0.0, nu=0.0, cost=0.0, cost0=0.0, trial=[0.0] * 4, nfev=0, status=0, done=False)
    running = dict(lam=1e-3, nu=2.0, cost=100.0, cost0=120.0, trial=[-20.0, 5.0, 1.0, 50.0], nfev=3, status=0, done=False)
    z, Z = np.zeros(n), np.zeros((n, n))

    def first(H=H0, g=g0, x=x0, held=(), boxed=False, nfree=8, cost2=200.0, vis=30, last=False, **kw):
        return dict(dict(opts, **kw), n=n, first=True, last=last, held=set(held), boxed=boxed, nfree=nfree, lin_H=H, lin_g=g, lin_cost2=cost2,
                    lin_vis=vis, st=fresh, x=x, xt=x, H=Z, g=z)

    tiny = g0 * 1e-10
    at_lo, at_hi = x0.copy(), x0.copy()
    at_lo[2], at_hi[2] = 0.0, 1.0
    g_out_lo, g_in_lo = tiny.copy(), tiny.copy()
    g_out_lo[2], g_in_lo[2] = 7.0, -7.0                    # at rs = 0: g > 0 pushes below the bound (blocked), g < 0 pushes inward (counts)
    g_out_hi = tiny.copy()
    g_out_hi[2] = -7.0
    indef = H0.copy()
    indef[0, 0], indef[1, 1], indef[0, 1], indef[1, 0] = 1.0, 1.0, 3.0, 3.0
    indef[0, 2:] = indef[2:, 0] = indef[1, 2:] = indef[2:, 1] = 0.0          # the block [[1, 3], [3, 1]]: positive definite only for lambda > 2
    hopeless = H0.copy()
    hopeless[4, 4] = -1e13                                # D_44 = 1: no lambda up to 1e12 makes the pivot positive
    big = g0.copy()
    big[5] = float('inf')                                 # a step that is not finite at any damping
    return {
        'first_round_solves': first(),
        'status1_free_gradient_below_gtol': first(g=tiny),
        'status1_with_a_blocked_rs_at_0': first(g=g_out_lo, x=at_lo, boxed=True),
        'status1_with_a_blocked_rs_at_1': first(g=g_out_hi, x=at_hi, boxed=True),
        'rs_on_its_bound_pushing_inward_counts': first(g=g_in_lo, x=at_lo, boxed=True),
        'rs_gradient_counts_without_a_box': first(g=g_out_lo, x=at_lo, boxed=False),
        'blocked_rs_leaves_the_solve': first(g=np.where(np.arange(n) == 2, 7.0, g0), x=at_lo, boxed=True),
        'held_entries_leave_the_system': first(held=(1, 6), nfree=6),
        'a_held_gradient_does_not_count': first(g=np.where(np.arange(n) == 6, 3.0, tiny), held=(6,), nfree=7),
        'indefinite_raises_lambda_by_tens': first(H=indef),
        'indefinite_to_status0_past_1e12': first(H=hopeless),
        'nonfinite_step_to_status0_past_1e12': first(g=big),
        'max_nfev_1': first(max_nfev=1, last=True),
        'max_nfev_1_converged': first(max_nfev=1, last=True, g=tiny),
        'never_started_too_few_rows': first(vis=3),
        'never_started_nonfinite_cost': first(cost2=float('nan')),
        'accepted_trial_is_adopted_and_solved': dict(opts, n=n, first=False, last=False, held=set(), boxed=False, nfree=8, lin_H=H0 * 1.1, lin_g=g0 * 0.5,
                                                     lin_cost2=182.0, lin_vis=30, st=running, x=x0, xt=x0 + 0.1, H=H0, g=g0),
        'rejected_trial_keeps_the_linearisation': dict(opts, n=n, first=False, last=False, held=set(), boxed=False, nfree=8, lin_H=H0 * 1.1, lin_g=g0 * 0.5,
                                                       lin_cost2=208.0, lin_vis=30, st=running, x=x0, xt=x0 + 0.1, H=H0, g=g0),
        'accepted_then_status1': dict(opts, n=n, first=False, last=False, held=set(), boxed=False, nfree=8, lin_H=H0, lin_g=tiny, lin_cost2=182.0,
                                      lin_vis=30, st=running, x=x0, xt=x0 + 0.1, H=H0, g=g0),
        'last_round_only_decides': dict(opts, n=n, first=False, last=True, held=set(), boxed=False, nfree=8, lin_H=H0 * 1.1, lin_g=g0 * 0.5,
                                        lin_cost2=182.0, lin_vis=30, st=running, x=x0, xt=x0 + 0.1, H=H0, g=g0),
        'a_finished_problem_is_left_alone': dict(opts, n=n, first=False, last=False, held=set(), boxed=False, nfree=8, lin_H=H0 * 1.1, lin_g=g0 * 0.5,
                                                 lin_cost2=182.0, lin_vis=30, st=dict(running, status=2, done=True), x=x0, xt=x0 + 0.1, H=H0, g=g0),
    }


ROUND_CASES = _round_cases()
# what each case is there for: (status, done) after the round, and lambda where it says something
ROUND_EXPECT = {
    'first_round_solves': (0, False, 1e-4), 'status1_free_gradient_below_gtol': (1, True, 1e-4), 'status1_with_a_blocked_rs_at_0': (1, True, 1e-4),
    'status1_with_a_blocked_rs_at_1': (1, True, 1e-4), 'rs_on_its_bound_pushing_inward_counts': (0, False, 1e-4),
    'rs_gradient_counts_without_a_box': (0, False, 1e-4), 'blocked_rs_leaves_the_solve': (0, False, 1e-4), 'held_entries_leave_the_system': (0, False, 1e-4),
    'a_held_gradient_does_not_count': (1, True, 1e-4), 'indefinite_raises_lambda_by_tens': (0, False, None), 'indefinite_to_status0_past_1e12': (0, True, None),
    'nonfinite_step_to_status0_past_1e12': (0, True, None), 'max_nfev_1': (0, True, 1e-4), 'max_nfev_1_converged': (1, True, 1e-4),
    'never_started_too_few_rows': (-1, True, 1e-4), 'never_started_nonfinite_cost': (-1, True, 1e-4), 'accepted_trial_is_adopted_and_solved': (0, False, None),
    'rejected_trial_keeps_the_linearisation': (0, False, 2e-3), 'accepted_then_status1': (1, True, None), 'last_round_only_decides': (0, False, None),
    'a_finished_problem_is_left_alone': (2, True, 1e-3),
}


@pytest.mark.parametrize('name', sorted(ROUND_CASES))
def test_round_against_the_restatement(name):
    """2. reg_round -- what the device runs per problem between two evaluations -- against the restatement above: status 1 on the
    projected gradient (a blocked rs and held entries not counting), the blocked rs leaving the solve, a failed factorisation and a
    non-finite step raising lambda by tens up to 1e12 and status 0 past it, max_nfev = 1, problems that never start.  Integers and
    booleans equal; lambda, nu, the costs, the trial scalars, x, the trial point, H and g bit-equal."""
    c = dict(ROUND_CASES[name])
    held = c.pop('held')
    want = _round_py(held=held, **c)
    c['lin_visible'] = c.pop('lin_vis')
    c['state'] = c.pop('st')
    got = ru.round_(held=sum(1 << k for k in held), **c)
    bits = lambda v: np.asarray(v, dtype=np.float64).tobytes()
    ws, gs = want[0], got[0]
    assert (gs['nfev'], gs['status'], gs['done']) == (ws['nfev'], ws['status'], ws['done'])
    for k in ('lam', 'nu', 'cost', 'cost0', 'trial'):
        assert bits(gs[k]) == bits(ws[k]), k
    for k, what in enumerate(('x', 'xt', 'H', 'g')):
        assert bits(got[1 + k]) == bits(want[1 + k]), what
    status, done, lam = ROUND_EXPECT[name]
    assert (gs['status'], gs['done']) == (status, done)
    if lam is not None:
        assert gs['lam'] == lam
    n = c['n']
    if name == 'indefinite_raises_lambda_by_tens':
        assert gs['lam'] == 1e-4 * 10.0 * 10.0 * 10.0 * 10.0 * 10.0 and 2.0 < gs['lam'] < 11.0 and gs['nfev'] == 1   # five failures (1e-4 .. 1), then 10 factorises
    if name in ('indefinite_to_status0_past_1e12', 'nonfinite_step_to_status0_past_1e12'):
        assert gs['lam'] > 1e12 and gs['nfev'] == 1
    if name == 'blocked_rs_leaves_the_solve':
        assert got[2][2] == 0.0 and not np.array_equal(got[2], got[1])                              # rs stays on the bound, the others move
    if name == 'rs_gradient_counts_without_a_box':
        assert got[2][2] < 0.0                                                                      # no box: rs follows its gradient below 0
    if name == 'held_entries_leave_the_system':
        assert got[2][1] == got[1][1] and got[2][6] == got[1][6] and got[4][1] == 0.0 and got[3][1, 1] == 1.0 and not got[3][1, 2:].any()
    if name == 'accepted_trial_is_adopted_and_solved':
        assert np.array_equal(got[1], c['xt']) and np.array_equal(got[3], np.asarray(c['lin_H'])) and gs['nfev'] == 4 and gs['cost'] == 91.0
    if name == 'rejected_trial_keeps_the_linearisation':
        assert np.array_equal(got[1], c['x']) and np.array_equal(got[3], np.asarray(c['H'])) and gs['cost'] == 100.0 and gs['nu'] == 4.0
    if name == 'last_round_only_decides':
        assert np.array_equal(got[2], c['xt']) and np.array_equal(got[1], c['xt'])                  # adopted, no new trial
    if name == 'a_finished_problem_is_left_alone':
        assert np.array_equal(got[1], c['x']) and gs['nfev'] == 3


# ---- 3. the host loop against scipy --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(rc.CASES))
def test_host_loop_against_scipy(name):
    """3. Camera 2 of make_scene(4, 4000, perturb=0.0) from its true entries perturbed by 0.5 degrees, 0.3 m and 1 frame: the host loop
    and scipy (trf, x_scale='jac', tolerances 1e-14, Jacobian of the host build) end at the same estimate -- cost within 1e-9 relative,
    every free parameter within 1e-3 sigma.  The camera's detections are cut 25 frames inside the spline's interval (make_scene lets
    every camera see the target up to its very ends), and every point either solver visits keeps them 20 frames inside: asserted.
    The host loop runs with the defaults of BAHandle.register_cameras (ftol 1e-8, xtol 1e-12, gtol 1e-8, 50 evaluations).
    Measured: cost 4.6e-15, 1.3e-14, 2.4e-15 relative; parameters 2.3e-6, 4.0e-6, 9.7e-7 sigma; 4, 5, 4 evaluations against scipy's 5, 11, 5
    (p6, p6_rs_bounds, p15_Kd_held)."""
    c, ref, got = rc.case(name), rc.scipy_reference(name), rc.host_solution(name)
    lo, hi = c.interval[0, 0] + rc.MARGIN, c.interval[1, -1] - rc.MARGIN
    for tr in (ref.tau_range, got.tau_range):
        assert lo <= tr[0] and tr[1] <= hi, (tr, lo, hi)
    assert got.visible == int(c.prob.det_offsets[rc.CAM + 1] - c.prob.det_offsets[rc.CAM])
    assert ref.status >= 1 and got.status >= 1
    d = np.abs(got.params - ref.params)[c.free] / ref.sigma
    print('%s: scipy status %d nfev %d; host status %d nfev %d; cost rel %.3e; max |dp| / sigma %.3e'
          % (name, ref.status, ref.nfev, got.status, got.nfev, abs(got.cost - ref.cost) / ref.cost, d.max()))
    assert abs(got.cost - ref.cost) <= 1e-9 * ref.cost
    assert np.all(d <= 1e-3)
    assert np.array_equal(got.params[~c.free], c.start[~c.free])              # held and switched-off entries: the bits they went in with
    if c.prob.rs_bounds:
        assert 0.0 <= got.params[2] <= 1.0


# ---- 4. bindings, arguments, settings ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as ge
    ge.build()
    return _lib.load()


NAMES = ('mvus_ba_register_cameras', 'mvus_ba_register_linearize')


def test_entry_points_are_declared_bound_and_exported(lib):
    hdr = open(os.path.join(ROOT, 'include', 'mvus_ba.h')).read()
    declared = set(re.findall(r'\b(mvus_[a-z_0-9]+)\s*\(', hdr))
    bound = {name for name, _, _ in _lib.API}
    for name in NAMES:
        assert name in declared and name in bound and hasattr(lib, name)
    assert _lib.ABI_VERSION == 8 and re.search(r'#define MVUS_ABI_VERSION 8\b', hdr)


def _call(lib, B=1, max_nfev=50, ftol=1e-8, xtol=1e-12, gtol=1e-8):
    """mvus_ba_register_cameras without a handle: what can be refused is refused before the handle is looked at."""
    cam = np.zeros(max(B, 1), dtype=np.int32)
    x = np.zeros(4)
    rc_ = lib.mvus_ba_register_cameras(None, _lib.dptr(x), B, cam.ctypes.data_as(_lib.c_int32_p), None, max_nfev, ftol, xtol, gtol, 0.0, 0.0, 0.0,
                                       None, None, None, None, None, None, None)
    return rc_, lib.mvus_last_error(None).decode()


def test_bad_arguments_are_refused_without_a_device(lib):
    """4. Every bad argument: MVUS_E_INVALID with its own message, no device touched (there is no handle at all here; the checks that
    need C and P of a handle are the same functions, called through the host build)."""
    for kw, word in [(dict(B=-1), 'negative'), (dict(B=4097), '4096'), (dict(max_nfev=0), 'max_nfev'), (dict(ftol=-1e-8), 'ftol'),
                     (dict(xtol=-1.0), 'xtol'), (dict(gtol=float('nan')), 'gtol')]:
        code, msg = _call(lib, **kw)
        assert code == _lib.MVUS_E_INVALID and word in msg and msg.startswith('register_cameras:'), (kw, msg)
    assert _call(lib, B=0) == (_lib.MVUS_OK, _call(lib, B=0)[1])             # B = 0: MVUS_OK, nothing done
    code, msg = _call(lib, B=1)
    assert code == _lib.MVUS_E_INVALID and 'NULL handle' in msg
    rcode = lib.mvus_ba_register_linearize(None, None, -3, None, None, None, None, None, None)
    assert rcode == _lib.MVUS_E_INVALID and lib.mvus_last_error(None).decode().startswith('register_linearize: B = -3')
    # a camera index outside [0, C) and a non-finite start, for a handle with C = 4, P = 6
    for cams, start, word in [([0, 4], None, 'cam[1] = 4'), ([-1], None, 'cam[0] = -1'), ([1, 2], np.r_[np.zeros(12), np.inf, np.zeros(5)], 'start[12]'),
                              ([3], np.r_[np.nan, np.zeros(8)], 'start[0]')]:
        code, msg = ru.check_args(4, 6, cams, start)
        assert code == 1 and word in msg, msg
    assert ru.check_args(4, 6, [0, 3], np.zeros(18)) == (0, '')
    assert ru.check_args(4, 6, [], B=0) == (0, '')


def test_settings_are_validated_on_the_host(monkeypatch):
    """4. ba_register is a bool (absent = false), ba_register_beta_search [half_width, step]: anything else raises ValueError naming the
    key, from ba_mode -- before any GPU call."""
    from mvus_amd.reconstruction import common
    scene, _ = load_case('c1_pinhole_2cam')
    monkeypatch.setattr(common.Scene, '_handle', lambda self, prob: pytest.fail('a GPU handle was created'))
    assert build_scene(scene).ba_register_enabled() is False and build_scene(scene).ba_register_beta_search() is None
    assert build_scene(scene, ba_register=True).ba_register_enabled() is True
    assert build_scene(scene, ba_register_beta_search=[10, 0.5]).ba_register_beta_search() == (10.0, 0.5)
    for bad in (1, 'yes', None, [True]):
        s = build_scene(scene, ba_register=bad)
        with pytest.raises(ValueError, match='ba_register'):
            s.ba_mode()
        with pytest.raises(ValueError, match='ba_register'):
            s.BA(2, max_iter=3)
    for bad in (5, [10], [10, 0], [-1, 1], ['a', 1], [10, float('inf')], [True, 1], 'wide'):
        s = build_scene(scene, ba_register_beta_search=bad)
        with pytest.raises(ValueError, match='ba_register_beta_search'):
            s.ba_mode()
    s = build_scene(scene)
    with pytest.raises(ValueError, match='hold'):
        s.register_camera(1, hold=('pose',))
    with pytest.raises(ValueError, match='beta_search'):
        s.register_camera(1, beta_search=(10, 0))


def test_ranking_of_the_starts():
    """Scene.register_rank, the order register_camera prefers its starts in: started ones only; most inliers, then lowest cost, then
    smallest |k|, then the lower index."""
    from mvus_amd.reconstruction.common import Scene
    rank = Scene.register_rank
    ks = np.array([-2, -1, 0, 1, 2])
    assert rank([2, 2, 2, 2, 2], [5, 9, 7, 9, 3], [1.0, 4.0, 0.5, 3.0, 0.1], ks) == [3, 1, 2, 0, 4]            # inliers first, cost breaks the 9 / 9 tie
    assert rank([2, 2, 2, 2, 2], [9, 9, 9, 9, 9], [2.0, 1.0, 1.0, 1.0, 2.0], ks) == [2, 1, 3, 0, 4]            # equal cost: smallest |k|, then the lower index
    assert rank([-1, 2, -1, 0, 4], [99, 1, 99, 2, 2], [0.0, 1.0, 0.0, 5.0, 4.0], ks) == [4, 3, 1]              # never-started entries are out, whatever they score
    assert rank([-1, -1], [3, 3], [1.0, 1.0], [0, 1]) == [] and rank([], [], [], []) == []
    assert rank([0], [0], [np.inf], [0]) == [0]
    assert rank([1, 1], [4, 4], [np.float64(1.0), np.nextafter(1.0, 0.0)], [0, 5]) == [1, 0]                    # one ulp of cost outranks |k|
