"""Position priors on the trajectory in the LM + Schur BA, on the GPU (mvus_ba_set_position_priors / mvus_ba_num_position_priors /
mvus_ba_position_prior_cost; Scene settings ba_position_priors).

The reference of the priors' blocks and costs is numpy on scipy's design matrix (tests/priors_reference.py); of the step, LAPACK on the
exported blocks (tests/lm_reference.py); of the covariance, the long-double-refined inverse of the exported H."""
import ctypes
import functools

import numpy as np
import pytest

import priors_reference as pref
from golden_util import load_case
from lm_reference import lapack_lm_step
from mvus_amd import _lib
from mvus_amd import problem as mp

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
FIXTURES = ['c1_pinhole_2cam', 'rs_F_2int_3cam']
LM = dict(solver=_lib.SOLVER_LM_SCHUR, jac_mode=_lib.JAC_ANALYTIC)


@functools.lru_cache(maxsize=None)
def _case(name, motion_reg=None):
    scene, g = load_case(name)
    over = {} if motion_reg is None else dict(motion_reg=motion_reg)
    prob, x0 = mp.problem_from_scene(scene, **over)
    x = np.array(g['x0'] + g['delta'])
    return scene, g, prob, x, pref.prior_sets(prob, x)


def _set(h, t, P, w):
    """The priors with their weights as given (the binding's sigma form would round 1 / (1 / w))."""
    t, P, w = (np.ascontiguousarray(a, dtype=np.float64) for a in (t, P, w))
    h._check(h.lib.mvus_ba_set_position_priors(h.h, t.size, _lib.dptr(t), _lib.dptr(P), _lib.dptr(w)), 'mvus_ba_set_position_priors')


def _route(monkeypatch, route):
    if route == 'detection-major':
        monkeypatch.setenv('MVUS_NE_FROM_J', '1')
    else:
        monkeypatch.delenv('MVUS_NE_FROM_J', raising=False)


def _check_contribution(prob, x, pset, ne0, ne1, what, r_dev):
    """ne1 - ne0 against numpy: camera side and untouched spline entries bit for bit, touched ones to (n_rows + 8) eps sum |terms| +
    eps |entry without priors|, the terms being the row terms h_a h_b w^2 (band) and h_a w^2 (S - p) (gradient).  For the gradient that
    bar is held against the sum built from the DEVICE's own rows r_dev = w (S - p) (mvus_ba_position_prior_cost, pinned row by row in
    test_costs): that is what k_prior_ne itself does, the products and the ordered sum.  Against scipy's S the comparison carries the
    rounding of S as well -- S - p cancels, with |h_a w^2 (S - p)| as terms the K = 3 set of c1_pinhole_2cam misses by a factor 3.2 --
    so there the terms are the products that are summed, h_a w^2 h_q x_q and h_a w^2 p (priors_reference.contribution)."""
    t, P, w = pset
    g0, A0, band0, cross0 = ne0
    g1, A1, band1, cross1 = ne1
    head = prob.C * (3 + prob.P)
    assert np.array_equal(A1, A0) and np.array_equal(cross1, cross0) and np.array_equal(g1[:head], g0[:head]), what
    dg, dband, ag, aband, ng, nband = pref.contribution(prob, x, t, P, w, band0.shape[1])
    assert np.array_equal(g1[ng == 0], g0[ng == 0]) and np.array_equal(band1[nband == 0], band0[nband == 0]), what
    assert (ng > 0).sum() >= 12 and (nband > 0).sum() >= 30
    eg = np.abs((g1 - g0) - dg)
    bg = (ng + 8) * EPS * ag + EPS * np.abs(g0)
    eb = np.abs((band1 - band0) - dband)
    bb = (nband + 8) * EPS * aband + EPS * np.abs(band0)
    tg, tb = ng > 0, nband > 0
    dg_r, ag_r, ng_r = pref.gradient_from_rows(prob, g0.size, t, w, r_dev)
    assert np.array_equal(ng_r, ng)
    er = np.abs((g1 - g0) - dg_r)
    br = (ng + 8) * EPS * ag_r + EPS * np.abs(g0)
    tr = tg & (br > 0)
    print('%s: gradient max err / bar = %.3g from the device rows, %.3g against scipy S; band max err / bar = %.3g (%d + %d entries, up to %d rows each)'
          % (what, (er[tr] / br[tr]).max(), (eg[tg] / bg[tg]).max(), (eb[tb] / bb[tb]).max(), tg.sum(), tb.sum(), nband.max()))
    assert np.all(er[tg] <= br[tg]), what
    assert np.all(eg[tg] <= bg[tg]), what
    assert np.all(eb[tb] <= bb[tb]), what
    assert np.abs(dg).max() > 0 and np.abs(dband).max() > 0


@pytest.mark.parametrize('loss', ['linear', 'huber'])
@pytest.mark.parametrize('route', ['window-major', 'detection-major'])
@pytest.mark.parametrize('name', FIXTURES)
def test_normal_equations_gain_the_priors_contribution(name, route, loss, monkeypatch):
    """4. (blocks with priors) - (blocks without) = the numpy contribution; A, g_c, the cross block and every spline entry no active row
    touches keep their bits; two calls give identical bits; the shuffled set gives the bits of the same set passed sorted; a loss in
    force does not reach the prior rows.  The repeat and the sorted set each go through a FRESH assembly and a fresh launch of
    k_prior_ne (clear, normal_equations, set, normal_equations).  Window-major every assembly gives the same bits, so the comparison is
    bit for bit always; the detection-major kernel adds with fp64 atomics (include/mvus_ba.h, mvus_ba_deterministic_fallback), so there
    it is bit for bit whenever the blocks WITHOUT priors came out with the bits of the first assembly, and to rounding otherwise."""
    from mvus_amd.ba import BAHandle
    _, _, prob, x, sets = _case(name)
    _route(monkeypatch, route)
    with BAHandle(prob) as h:
        if loss != 'linear':
            h.set_loss(loss, 1.5)
        h.residual_jacobian(x, _lib.JAC_ANALYTIC)
        for sname, pset in sets.items():
            h.set_position_priors(None, None, None)
            ne0 = h.normal_equations()
            assert h.deterministic_fallback() == (route == 'detection-major')
            _set(h, *pset)
            act = int((pref.design(prob, pset[0])[0] >= 0).sum())
            assert h.num_position_priors == pset[0].size and h.num_active_position_priors == act
            ne1 = h.normal_equations()
            r_dev = h.position_prior_cost(x, rows=True)[1]           # (an inspection hook: the held blocks stay)
            what = '%s %s %s %s' % (name, route, loss, sname)
            _check_contribution(prob, x, pset, ne0, ne1, what, r_dev)
            for a, b in zip(ne1, h.normal_equations()):
                assert np.array_equal(a, b)
            again = [pset]
            if sname == 'mixed':
                order = np.argsort(pset[0], kind='stable')
                assert not np.array_equal(order, np.arange(order.size))
                again.append((pset[0][order], pset[1][:, order], pset[2][:, order]))
            for ps2 in again:
                h.set_position_priors(None, None, None)
                ne0b = h.normal_equations()                              # a new assembly
                _set(h, *ps2)
                ne1b = h.normal_equations()                              # ... and a new launch of k_prior_ne on it
                same_raw = all(np.array_equal(a, b) for a, b in zip(ne0, ne0b))
                assert same_raw or route == 'detection-major'
                if not same_raw:
                    print('%s: the second assembly without priors differs in its last bits (atomics)' % what)
                for a, b in zip(ne1, ne1b):
                    if same_raw:
                        assert np.array_equal(a, b), what
                    else:
                        np.testing.assert_allclose(b, a, rtol=0, atol=1e-12 * np.abs(a).max())
        f, J, _ = h.residual_jacobian(x, _lib.JAC_ANALYTIC)      # error_BA itself stays raw
        assert f.size == prob.n_residuals


@pytest.mark.parametrize('name', FIXTURES)
def test_costs(name):
    """5. r row by row to 32 eps |w| (|S| + |p|) in the CALLER's order, NaN for inactive rows, `active` = the host count;
    position_prior_cost = 0.5 sum r_out^2 of the device's own rows to (3K + 8) eps relative (the squares and the reduction tree:
    wave_sum, the wavefronts in order, k_dot_final); against numpy on scipy's S the same (3K + 8) eps plus what the rows' own bar
    leaves in the sum, sum |r| 32 eps |w| (|S| + |p|) -- S - p cancels (the priors sit within a few sigma of the curve), so a relative bar on the cost
    alone would ask more of the sum than its terms can give (measured on one MI355X: |cost - numpy| / cost = 0 - 1.6e-14 over the eight
    cases; (3K + 8) eps alone is 2.4e-15 at K = 1 and 3.8e-15 at K = 3 and is missed at K = 3 on both fixtures, 1.6e-14 and 1.1e-14,
    and at K = 1 on rs_F_2int_3cam, 7.2e-15; the bar used here is 1.2e-12 - 2.4e-12); initial_cost of a solve with priors - without =
    the prior cost within 1e-12 of the total."""
    from mvus_amd.ba import BAHandle
    _, _, prob, x, sets = _case(name)
    with BAHandle(prob) as h:
        assert h.position_prior_cost(x) == 0.0 and h.num_position_priors == 0
        base = h.solve(x, max_nfev=1, **LM).initial_cost
        for sname, (t, P, w) in sets.items():
            _set(h, t, P, w)
            cost_ref, r_ref, ctrl, _, S = pref.rows(prob, x, t, P, w)
            cost, r = h.position_prior_cost(x, rows=True)
            K = t.size
            assert h.num_active_position_priors == int((ctrl >= 0).sum())
            assert np.array_equal(np.isnan(r), np.repeat((ctrl < 0)[None, :], 3, axis=0))
            a = ctrl >= 0
            bar = 32 * EPS * np.abs(w[:, a]) * (np.abs(S[:, a]) + np.abs(P[:, a]))
            err = np.abs(r[:, a] - r_ref[:, a])
            cost_bar = (3 * K + 8) * EPS * cost_ref + float(np.sum(np.abs(r_ref[:, a]) * bar))
            print('%s %s: cost %.17g, |cost - numpy| / cost = %.3g (sum alone %.3g, with the bar of the rows %.3g), rows max err / bar = %.3g'
                  % (name, sname, cost, abs(cost - cost_ref) / cost_ref, (3 * K + 8) * EPS, cost_bar / cost_ref, (err / np.maximum(bar, 1e-300))[bar > 0].max()))
            assert np.all(err <= bar)
            cost_rows = 0.5 * float(np.sum(r[:, a] ** 2))           # the device's own rows: what is left is the 3K squares and their sum
            print('%s %s: |cost - 0.5 sum r_out^2| / cost = %.3g (bar %.3g)' % (name, sname, abs(cost - cost_rows) / cost_rows, (3 * K + 8) * EPS))
            assert abs(cost - cost_rows) <= (3 * K + 8) * EPS * cost_rows
            assert abs(cost - cost_ref) <= cost_bar
            with_p = h.solve(x, max_nfev=1, **LM)
            assert with_p.fun.size == prob.n_residuals                   # f stays error_BA's: 2M + T rows
            assert abs((with_p.initial_cost - base) - cost) <= 1e-12 * with_p.initial_cost, (with_p.initial_cost, base, cost)
            assert h.robust_cost(x) == base                              # the raw cost does not see the priors
        h.set_position_priors(None, None, None)
        assert h.solve(x, max_nfev=1, **LM).initial_cost == base


def _refined_solve(H, b):
    """H^-1 b with three steps of iterative refinement, residuals in long double."""
    Hl, bl = H.astype(np.longdouble), b.astype(np.longdouble)
    y = np.linalg.solve(H, b)
    for _ in range(3):
        r = (bl - Hl @ y.astype(np.longdouble)).astype(np.float64)
        y = (y.astype(np.longdouble) + np.linalg.solve(H, r).astype(np.longdouble)).astype(np.float64)
    return y


def _dense_system(prob, ne):
    """H (n x n, x order) and g from the exported blocks."""
    g, A, band, cross = ne
    C, B, N, W = prob.C, 3 + prob.P, band.shape[0], band.shape[1]
    cam = np.array([[c, C + c, 2 * C + c] + list(range(3 * C + c * prob.P, 3 * C + (c + 1) * prob.P)) for c in range(C)])
    spl = pref.ctrl_columns(prob).ravel()
    H = np.zeros((g.size, g.size))
    for c in range(C):
        H[np.ix_(cam[c], cam[c])] = A[c]
    E = cross.reshape(C * B, 3 * N)
    H[np.ix_(cam.ravel(), spl)] = E
    H[np.ix_(spl, cam.ravel())] = E.T
    for gi in range(N):
        for w in range(W):
            if gi + w < N:
                r, q = spl[3 * gi:3 * gi + 3], spl[3 * (gi + w):3 * (gi + w) + 3]
                H[np.ix_(r, q)] = band[gi, w]
                H[np.ix_(q, r)] = band[gi, w].T
    return H, g


@pytest.mark.parametrize('loss', ['linear', 'huber'])
@pytest.mark.parametrize('route', ['window-major', 'detection-major'])
@pytest.mark.parametrize('name', FIXTURES)
def test_lm_step_against_lapack(name, route, loss, monkeypatch):
    """6. mvus_ba_lm_step with priors against LAPACK on the exported blocks at lambda = 0.5 and 1e-3: 1e-6 of the largest entry -- both
    fixtures, both assembly routes, linear and huber(1.5), the four prior sets."""
    from mvus_amd.ba import BAHandle
    _, _, prob, x, sets = _case(name)
    _route(monkeypatch, route)
    with BAHandle(prob) as h:
        if loss != 'linear':
            h.set_loss(loss, 1.5)
        for sname, pset in sets.items():
            _set(h, *pset)
            h.residual_jacobian(x, _lib.JAC_ANALYTIC)
            g, A, band, cross = h.normal_equations()
            assert h.deterministic_fallback() == (route == 'detection-major')
            for lam in (0.5, 1e-3):
                p = h.lm_step(lam)
                p_ref = lapack_lm_step(prob, g, A, band, cross, lam)
                err = np.abs(p - p_ref).max() / np.abs(p_ref).max()
                print('%s %s %s %s lambda %g: |p - p_lapack|_max / |p_lapack|_max = %.3g' % (name, route, loss, sname, lam, err))
                assert err <= 1e-6


def test_undamped_step_is_solvable_because_of_the_priors():
    """6. lambda = 0 on c1_pinhole_2cam, free gauge, no motion regulariser, K = 3: finite and solve_ok (without the priors the undamped
    system is singular); error against LAPACK held to 8 x LAPACK's own fp64 error against the long-double-refined solve.  A frozen MASK
    IS IN FORCE in this test: rs is no unknown of this fixture -- no rolling shutter, its columns of J are zero, and an undamped system
    cannot have a zero row -- so the two rs entries are held with mvus_ba_set_frozen and the freeze pass runs behind the priors' pass.
    That is not a gauge freedom: the seven freedoms of the similarity stay free, and only the priors remove them."""
    from mvus_amd.ba import BAHandle
    _, _, prob, x, sets = _case('c1_pinhole_2cam', False)
    assert prob.num_motion_rows == 0
    assert not prob.rs_free
    mask = np.zeros(prob.C * (3 + prob.P), dtype=bool)
    mask[2 * prob.C:3 * prob.C] = True
    with BAHandle(prob) as h:
        h.set_frozen(mask)
        h.residual_jacobian(x, _lib.JAC_ANALYTIC)
        H0, _ = _dense_system(prob, h.normal_equations())
        ev0 = np.linalg.eigvalsh(H0 / np.sqrt(np.outer(np.diag(H0), np.diag(H0))))
        assert abs(ev0[0]) < 1e-12                                     # the free gauge: numerically singular without the priors
        _set(h, *sets['three'])
        h.residual_jacobian(x, _lib.JAC_ANALYTIC)
        ne = h.normal_equations()
        p = h.lm_step(0.0)                                             # raises MVUS_E_NUMERIC when the solve is not ok
        assert np.all(np.isfinite(p))
        H, g = _dense_system(prob, ne)
        d = np.diag(H)
        assert np.all(d > 0)
        p_lapack = -np.linalg.solve(H, g)
        p_exact = -_refined_solve(H, g)
        scale = np.abs(p_exact).max()
        e_lapack = np.abs(p_lapack - p_exact).max() / scale
        e_gpu = np.abs(p - p_exact).max() / scale
        e_pair = np.abs(p - p_lapack).max() / scale
        ev = np.linalg.eigvalsh(H / np.sqrt(np.outer(d, d)))
        print('lambda 0, K = 3: GPU vs refined %.3g, LAPACK vs refined %.3g, GPU vs LAPACK %.3g; smallest scaled eigenvalue %.3g'
              % (e_gpu, e_lapack, e_pair, ev[0]))
        assert ev[0] > 1e-8
        assert e_pair <= 8 * max(e_lapack, 1e-12)


@functools.lru_cache(maxsize=None)
def _solve_case():
    """c1_pinhole_2cam: 40 priors on the curve of the fixture's own BA result (ba10_x) + N(0, sigma), sigma = 1 % of the scene's size."""
    scene, g, prob, _, _ = _case('c1_pinhole_2cam')
    xs = np.array(g['ba10_x'])
    rng = np.random.default_rng(40)
    sigma = 0.01 * pref.scene_size(prob, xs)
    lo, hi = prob.interval[0, 0], prob.interval[1, 0]
    t = np.sort(rng.uniform(lo, hi, 40))
    P = pref.curve(prob, xs, t) + sigma * rng.standard_normal((3, 40))
    return scene, g, prob, (t, P, np.full((3, 40), 1.0 / sigma))


def test_solve_with_priors():
    """7. LM, 50 evaluations: res.cost = oracle detection cost + numpy prior cost at the returned x (1e-9 relative); the cost decreases; with
    a loss in force robust_cost + position_prior_cost = res.cost (1e-12: the prior rows are not reweighted); solve -> set -> clear ->
    solve = solve -> solve bit for bit; the priors survive remove_outliers."""
    from mvus_amd.ba import BAHandle
    from oracle import ba_oracle as orc
    scene, g, prob, pset = _solve_case()
    oprob, _ = orc.problem_from_scene(scene)
    x0 = np.array(g['x0'])
    with BAHandle(prob) as h:
        _set(h, *pset)
        res = h.solve(x0, max_nfev=50, **LM)
        fo = orc.residual(oprob, res.x)
        ref = 0.5 * float(fo @ fo) + pref.rows(prob, res.x, *pset)[0]
        print('solve with 40 priors: cost %.10g -> %.10g in %d evaluations; oracle + numpy %.10g (rel %.3g); prior part %.6g'
              % (res.initial_cost, res.cost, res.nfev, ref, abs(res.cost - ref) / ref, pref.rows(prob, res.x, *pset)[0]))
        assert res.cost < res.initial_cost
        assert abs(res.cost - ref) <= 1e-9 * ref
        assert res.fun.size == prob.n_residuals and np.abs(res.fun - fo).max() <= 1e-9      # f stays error_BA's
        h.set_loss('huber', 1.5)
        rl = h.solve(x0, max_nfev=50, **LM)
        assert rl.cost < rl.initial_cost
        assert abs(h.robust_cost(rl.x) + h.position_prior_cost(rl.x) - rl.cost) <= 1e-12 * rl.cost
        h.set_loss('linear')
        # the priors survive remove_outliers, and the normal equations afterwards still carry their contribution
        keep = h.remove_outliers(res.x, float(scene.settings['thres_outlier']))
        assert h.num_position_priors == 40 and h.num_active_position_priors == 40
        h.residual_jacobian(res.x, _lib.JAC_ANALYTIC)
        ne1 = h.normal_equations()
        r_dev = h.position_prior_cost(res.x, rows=True)[1]
        h.set_position_priors(None, None, None)
        h.residual_jacobian(res.x, _lib.JAC_ANALYTIC)
        ne0 = h.normal_equations()
        _check_contribution(h.prob, res.x, pset, ne0, ne1, 'after remove_outliers (%d of %d kept)' % (keep.sum(), keep.size), r_dev)
    with BAHandle(prob) as h:
        a1 = h.solve(x0, max_nfev=6, return_fun=False, **LM)
        a2 = h.solve(a1.x, max_nfev=6, **LM)
    with BAHandle(prob) as h:
        b1 = h.solve(x0, max_nfev=6, return_fun=False, **LM)
        _set(h, *pset)
        h.set_position_priors(None, None, None)
        b2 = h.solve(b1.x, max_nfev=6, **LM)
    assert np.array_equal(a1.x, b1.x)
    assert np.array_equal(a2.x, b2.x) and a2.cost == b2.cost and a2.nfev == b2.nfev and np.array_equal(a2.fun, b2.fun)


def test_refusals():
    """8. TRF with active priors: 'TRF_LSMR'; sharded handles in both orders: 'sharded'; negative or NaN weights, non-finite t or P, K < 0:
    MVUS_E_INVALID; a set with zero active rows solves as no priors, bit for bit."""
    from mvus_amd.ba import BAHandle, UnsupportedBySolver
    _, g, prob, x, sets = _case('rs_F_2int_3cam')
    t, P, w = sets['three']
    x0 = np.array(g['x0'])
    noop = lambda buf, count, stream: None
    with BAHandle(prob) as h:
        _set(h, t, P, w)
        for jac in (_lib.JAC_ANALYTIC, _lib.JAC_PATTERN):
            with pytest.raises(UnsupportedBySolver, match='TRF_LSMR'):
                h.solve(x0, solver=_lib.SOLVER_TRF_LSMR, jac_mode=jac, max_nfev=3, ties='canonical')
        for jac in (_lib.JAC_PATTERN, _lib.JAC_FD):               # LM takes the priors in every Jacobian mode: the pass is behind the assembly
            r = h.solve(x0, solver=_lib.SOLVER_LM_SCHUR, jac_mode=jac, max_nfev=10)      # (the first three trials from x0 are rejected, with or without priors)
            assert r.cost < r.initial_cost
            assert abs(r.initial_cost - (0.5 * float(np.sum(h.residual(x0) ** 2)) + h.position_prior_cost(x0))) <= 1e-12 * r.initial_cost
    with BAHandle(prob) as h:                                           # the route first
        h.set_allreduce(noop)
        with pytest.raises(UnsupportedBySolver, match='sharded'):
            _set(h, t, P, w)
        assert h.num_position_priors == 0
        h.set_position_priors(None, None, None)                         # nothing to refuse
    with BAHandle(prob) as h:                                           # the priors first: never solved without them
        _set(h, t, P, w)
        h.set_allreduce(noop)
        with pytest.raises(UnsupportedBySolver, match='sharded'):
            h.solve(x0, max_nfev=3, **LM)
        h.residual_jacobian(x0, _lib.JAC_ANALYTIC)
        with pytest.raises(UnsupportedBySolver, match='sharded'):
            h.normal_equations()
        with pytest.raises(UnsupportedBySolver, match='sharded'):
            h.lm_step(0.1)
    N = int(prob.n_coef.sum())
    with BAHandle(prob) as h:                                           # a time shard, both orders
        h.set_time_shard(0, 2, [0, N // 2, N])
        with pytest.raises(UnsupportedBySolver, match='sharded'):
            _set(h, t, P, w)
    with BAHandle(prob) as h:
        _set(h, t, P, w)
        h.set_time_shard(0, 2, [0, N // 2, N])
        with pytest.raises(UnsupportedBySolver, match='sharded'):
            h.solve(x0, max_nfev=3, **LM)
    with BAHandle(prob) as h:
        call = lambda K, tt, PP, ww: h.lib.mvus_ba_set_position_priors(h.h, K, _lib.dptr(np.ascontiguousarray(tt)), _lib.dptr(np.ascontiguousarray(PP)),
                                                                      _lib.dptr(np.ascontiguousarray(ww)))
        _set(h, t, P, w)
        for bad_t, bad_P, bad_w in [(t, P, np.where(np.arange(3)[None, :] == 1, -w, w)), (t, P, np.where(np.arange(3)[:, None] == 2, np.nan, w)),
                                    (t, P, np.full_like(w, np.inf)), (np.array([t[0], np.nan, t[2]]), P, w), (t, np.where(P == P[1, 1], np.inf, P), w)]:
            assert call(3, bad_t, bad_P, bad_w) == _lib.MVUS_E_INVALID
            assert b'set_position_priors' in h.lib.mvus_last_error(h.h)
        assert call(-1, t, P, w) == _lib.MVUS_E_INVALID
        assert h.num_position_priors == 3 and h.num_active_position_priors == 3      # a refused set leaves the handle as it was
    with BAHandle(prob) as h:
        plain = h.solve(x0, max_nfev=8, **LM)
    with BAHandle(prob) as h:                                           # zero active rows: between the intervals and outside them
        gap = 0.5 * (prob.interval[1, 0] + prob.interval[0, 1])
        tt = np.array([gap, prob.interval[0, 0] - 1.0, prob.interval[1, -1] + 1.0])
        _set(h, tt, P, w)
        assert h.num_position_priors == 3 and h.num_active_position_priors == 0
        cost, r = h.position_prior_cost(x0, rows=True)
        assert cost == 0.0 and np.all(np.isnan(r))
        idle = h.solve(x0, max_nfev=8, **LM)
    assert np.array_equal(idle.x, plain.x) and idle.cost == plain.cost and idle.nfev == plain.nfev and np.array_equal(idle.fun, plain.fun)


def test_covariance_with_a_free_gauge():
    """9. c1_pinhole_2cam, free gauge, no motion regulariser: K = 3 priors make the covariance acceptable (the same handle without them is
    refused); Sigma against the long-double-refined inverse of the exported H at 8 x LAPACK's loss (floor 1e-12); dof rises by the
    number of active (prior, axis) pairs with w > 0."""
    from mvus_amd.ba import BAHandle
    _, g, prob, _, _ = _case('c1_pinhole_2cam', False)
    x = np.array(g['ba10_x'])
    t, P, w = (a.copy() for a in pref.prior_sets(prob, x)['three'])
    w[2, 1] = 0.0                                                    # one axis unknown: 8 rows, still three non-collinear points
    with BAHandle(prob) as h:
        _set(h, t, P, w)
        cv = h.covariance(x)
        total = h.robust_cost(x) + h.position_prior_cost(x)              # the a-posteriori factor takes the cost WITH the prior term
        assert h.position_prior_cost(x) > 0 and abs(cv.sigma2 - 2.0 * total / cv.dof) <= 1e-12 * cv.sigma2
        h.residual_jacobian(x, _lib.JAC_ANALYTIC)
        H, _ = _dense_system(prob, h.normal_equations())
        est = cv.estimated
        m_act = 2 * int((h.residual_jacobian(x, _lib.JAC_ANALYTIC)[2] >= 0).sum())
        assert cv.dof == m_act + 8 - int(est.sum())
        He = H[np.ix_(est, est)]
        n = He.shape[0]
        inv_lapack = np.linalg.inv(He)
        inv_exact = np.column_stack([_refined_solve(He, e) for e in np.eye(n)])
        scale = np.abs(inv_exact).max()
        loss = np.abs(inv_lapack - inv_exact).max() / scale
        cols = pref.ctrl_columns(prob)
        pos = {c: i for i, c in enumerate(np.nonzero(est)[0])}
        head = prob.C * (3 + prob.P)
        ch = [i for i in range(head) if est[i]]
        err = np.abs(cv.cam[np.ix_(ch, ch)] - cv.sigma2 * inv_exact[np.ix_([pos[i] for i in ch], [pos[i] for i in ch])]).max()
        for p in range(cols.shape[0]):
            for wv in range(min(4, cols.shape[0] - p)):
                ia, ib = [pos[c] for c in cols[p]], [pos[c] for c in cols[p + wv]]
                err = max(err, np.abs(cv.band[p, wv] - cv.sigma2 * inv_exact[np.ix_(ia, ib)]).max())
        err /= cv.sigma2 * scale
        ev = np.linalg.eigvalsh(He / np.sqrt(np.outer(np.diag(He), np.diag(He))))
        print('covariance with 3 priors, free gauge: max |Sigma - exact| / max = %.3g, LAPACK loss %.3g, smallest scaled eigenvalue %.3g, dof %d'
              % (err, loss, ev[0], cv.dof))
        assert err <= 8 * max(loss, 1e-12)
        h.set_position_priors(None, None, None)
        with pytest.raises(ValueError, match='gauge'):
            h.covariance(x)


def test_scene_ba_end_to_end_in_the_surveyed_frame():
    """10. Synthetic scene (3 cameras, 9000 detections): the truth's cameras and spline moved by a similarity, 30 priors = the true curve +
    N(0, 0.02 m).  align_to_position_priors, then Scene.BA (lm) with the priors: the trajectory rms against the truth with NO alignment
    afterwards is at most 2 x (the same BA without priors followed by the best similarity to the truth) + 3 sigma / sqrt(K), and the
    recovered scale is within 1 % of 1."""
    from mvus_amd import bspline, synth
    from mvus_amd.analysis.compare_gt import similarity_from_points
    from mvus_amd.reconstruction import common
    from mvus_amd.synth import rodrigues
    sc = synth.make_scene(3, 9000, seed=31)
    tr = sc.truth
    sigma, K = 0.02, 30
    rng = np.random.default_rng(31)

    def true_curve(tau):
        X = np.full((3, tau.size), np.nan)
        for tck in tr['tck']:
            m = (tau >= tck[0][0]) & (tau <= tck[0][-1])
            if m.any():
                X[:, m] = bspline.evaluate(tck[0], np.array(tck[1]), tau[m])
        return X

    def scene(**settings):
        s = common.Scene()
        s.numCam = 3
        s.settings = dict(sc.settings)
        s.settings.update(ba_solver='lm', **settings)
        for c in tr['cameras']:
            cam = common.Camera(K=c['K'].copy(), d=c['d'].copy(), R=c['R'].copy(), t=c['t'].copy(), fps=c['fps'], resolution=list(c['resolution']))
            cam.compose()
            s.addCamera(cam)
        for det in sc.detections:
            s.addDetection(det.copy())
        s.alpha, s.beta, s.rs = np.array(tr['alpha'], float), np.array(tr['beta'], float), np.array(tr['rs'], float)
        s.sequence = [0, 1, 2]
        s.spline = {'tck': [[np.array(t[0]), [np.array(c) for c in t[1]], 3] for t in tr['tck']], 'int': sc.interval.copy()}
        rv = np.array([0.2, -0.3, 0.1])
        s.apply_similarity(1.3, rodrigues(rv), np.array([4.0, -2.0, 1.0]))     # the reconstruction's own arbitrary frame
        s.detection_to_global()
        return s
    st = sc.settings
    kw = dict(rs=st['rolling_shutter'], motion_reg=st['motion_reg'], motion_weights=st['motion_weights'], rs_bounds=st['rs_bounds'])
    lo, hi = sc.interval[0, 0], sc.interval[1, -1]
    ts = np.arange(np.ceil(lo), np.floor(hi), 1.0)
    Xt = true_curve(ts)
    ok = np.all(np.isfinite(Xt), axis=0)
    # the yardstick: the same BA without priors, then the best similarity onto the truth
    s0 = scene()
    s0.BA(3, max_iter=30, **kw)
    traj0 = s0.spline_to_traj(t=ts[ok])
    M = similarity_from_points(traj0[1:], Xt[:, ok])
    rms0 = float(np.sqrt(np.mean(np.sum((M[:3, :3] @ traj0[1:] + M[:3, 3:] - Xt[:, ok]) ** 2, axis=0))))
    # with priors
    tp = np.sort(rng.uniform(lo, hi, K))
    tp = tp[np.all(np.isfinite(true_curve(tp)), axis=0)]
    Pp = true_curve(tp) + sigma * rng.standard_normal((3, tp.size))
    s1 = scene(ba_position_priors=True)
    s1.position_priors = np.vstack((tp, Pp, np.full((3, tp.size), sigma)))
    scale, R, T, rms_fit = s1.align_to_position_priors()
    res = s1.BA(3, max_iter=30, **kw)
    assert res.num_position_priors == tp.size and res.num_active_position_priors == tp.size and res.solver_used == 'lm'
    traj1 = s1.spline_to_traj(t=ts[ok])
    rms1 = float(np.sqrt(np.mean(np.sum((traj1[1:] - Xt[:, ok]) ** 2, axis=0))))
    M1 = similarity_from_points(traj1[1:], Xt[:, ok])
    scale1 = float(np.cbrt(np.linalg.det(M1[:3, :3])))
    bar = 2 * rms0 + 3 * sigma / np.sqrt(tp.size)
    print('end to end: rms against the truth with priors, NO alignment: %.4g m; without priors after the best similarity: %.4g m; bar %.4g m; '
          'scale to the truth %.6f (alignment scale %.4f, fit rms %.3g m)' % (rms1, rms0, bar, scale1, scale, rms_fit))
    assert rms1 <= bar
    assert abs(scale1 - 1.0) <= 0.01


def test_reconstruct_from_config_with_a_position_log(tmp_path):
    """The pipeline from files (tests/test_gpu_init_pipeline.py's inputs, 3 cameras x 9000 detections, exact corresponding frames, 'lm') with
    a position log of 30 lines = the true curve + N(0, 0.02 m): the loop runs as always (its result lives in the arbitrary frame of the
    two-view initialisation), then align_to_position_priors and one BA with the priors.  The trajectory against the truth with NO
    alignment afterwards is held to the bar of the end-to-end test above -- 2 x (the run without the log, after the best similarity onto
    the truth) + 3 sigma / sqrt(K) -- the scale to 1 %, and the covariance is accepted with the gauge left free.  Measured on one MI355X:
    0.331 m with the log against 0.349 m (31 m and a scale of 97.8 before any alignment) without."""
    import json
    from mvus_amd import bspline, pipeline, synth
    from mvus_amd.analysis.compare_gt import similarity_from_points
    from test_gpu_init_pipeline import _write_inputs
    sc = synth.make_scene(3, 9000, seed=31)
    tr = sc.truth

    def true_curve(tau):
        X = np.full((3, tau.size), np.nan)
        for tck in tr['tck']:
            m = (tau >= tck[0][0]) & (tau <= tck[0][-1])
            if m.any():
                X[:, m] = bspline.evaluate(tck[0], np.array(tck[1]), tau[m])
        return X
    rng = np.random.default_rng(7)
    sigma, K = 0.02, 30
    tp = np.sort(rng.uniform(sc.interval[0, 0] + 20, sc.interval[1, -1] - 20, K))
    Pp = true_curve(tp) + sigma * rng.standard_normal((3, K))
    out = {}
    for priors in (False, True):
        path = _write_inputs(tmp_path, sc, -tr['beta'] / tr['alpha'], True)
        cfg = json.loads(path.read_text())
        cfg['settings'].update(ba_solver='lm', ba_covariance=priors)
        if priors:
            np.savetxt(tmp_path / 'priors.txt', np.column_stack((tp, Pp.T)), fmt='%.18e')
            cfg['optional inputs'] = {'path_position_priors': str(tmp_path / 'priors.txt'), 'position_prior_sigma': sigma}
            cfg['settings']['ba_position_priors'] = True
        path.write_text(json.dumps(cfg))
        flight, timer = pipeline.reconstruct_from_config(str(path), output=False)
        assert ('align_to_position_priors' in [r[0] for r in timer.rows]) == priors
        ts = np.arange(np.ceil(flight.spline['int'][0, 0]), np.floor(flight.spline['int'][1, -1]), 1.0)
        traj = flight.spline_to_traj(t=ts)
        Xt = true_curve(traj[0])
        ok = np.all(np.isfinite(Xt), axis=0)
        M = similarity_from_points(traj[1:, ok], Xt[:, ok])
        out[priors] = dict(raw=float(np.sqrt(np.mean(np.sum((traj[1:, ok] - Xt[:, ok]) ** 2, axis=0)))),
                           fit=float(np.sqrt(np.mean(np.sum((M[:3, :3] @ traj[1:, ok] + M[:3, 3:] - Xt[:, ok]) ** 2, axis=0)))),
                           scale=float(np.cbrt(np.linalg.det(M[:3, :3]))))
    bar = 2 * out[False]['fit'] + 3 * sigma / np.sqrt(K)
    print('pipeline: with the log %.4g m (no alignment; scale %.5f); without %.4g m before, %.4g m after the best similarity (scale %.4g); bar %.4g m'
          % (out[True]['raw'], out[True]['scale'], out[False]['raw'], out[False]['fit'], out[False]['scale'], bar))
    assert out[True]['raw'] <= bar
    assert abs(out[True]['scale'] - 1.0) <= 0.01
    assert flight.position_priors.shape == (7, K) and flight.covariance['dof'] > 0 and np.all(np.isfinite(flight.covariance['pos_std'][1:-1]))


def test_scene_ba_refuses_the_trf_hand_over_with_priors(monkeypatch):
    """Where the wide-band policy of Scene.BA would hand the problem to TRF + LSMR, active priors raise UnsupportedBySolver (as a loss
    does) instead of being dropped; with ba_lm_wide_band = 'lm' the same BA runs."""
    from frozen_util import ba_kwargs, build_scene
    from mvus_amd.ba import UnsupportedBySolver
    from mvus_amd.reconstruction import common
    scene, _, prob, x, sets = _case('c1_pinhole_2cam')
    t, P, w = sets['three']
    monkeypatch.setattr(common.Scene, '_motion_band_width', staticmethod(lambda prob: 8))      # what knots less than a frame apart give
    s = build_scene(scene, ba_solver='lm', ba_position_priors=True)
    s.position_priors = np.vstack((t, P, 1.0 / w))
    with pytest.raises(UnsupportedBySolver, match='ba_position_priors'):
        s.BA(2, max_iter=3, **ba_kwargs(s.settings))
    s.settings['ba_lm_wide_band'] = 'lm'
    res = s.BA(2, max_iter=3, **ba_kwargs(s.settings))
    assert res.solver_used == 'lm' and res.num_active_position_priors == 3
