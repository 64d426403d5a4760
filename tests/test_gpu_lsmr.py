"""The LSMR loop of the default solver (TRF + LSMR) on the GPU, through mvus_ba_lsmr / BAHandle.lsmr, against the longdouble LSMR of
tests/lsmr_reference.py on the dense Jacobian of the host build -- at the layouts of tests/lsmr_layouts.py, which steer k_jtu_partial,
k_jvjtu, k_jtu_index, k_jtu_first and k_jtu_reduce into each of their branches.

Three forms of the loop: the device-resident two-pass loop (the default), the host-driven loop (MVUS_LSMR_HOST, read when a handle is
created) and the one-pass form (MVUS_LSMR_ONE_PASS, read at every run).

The accuracy bar is 8 x dev_host(layout, k): dev_host is the deviation of the HOST build of the same Lsmr::run (plain C++ backend, fp64)
from the reference after the same k iterations, computed here, never from the GPU; 8 is the project's allowance for another summation
order (the factor the triangulation bar gives LAPACK).  k stops at 4: the recurrence amplifies rounding about tenfold every one or two
iterations (test_solver_host.py), and a wrong branch is an O(1) error at k = 1.  The norm estimates (normr, normar, normA, condA) are
functions of the same alpha and beta: their bar is 8 x the larger of dev_host and the host build's own deviation in those four.

Figures measured on an MI355X: DESIGN.md section 16."""
import numpy as np
import pytest

import lsmr_layouts as L
import lsmr_reference as ref
from mvus_amd import _lib

pytestmark = pytest.mark.gpu

FACTOR = 8.0
SWITCHES = ('MVUS_LSMR_HOST', 'MVUS_LSMR_BOUNDED_HOST', 'MVUS_LSMR_ONE_PASS', 'MVUS_LSMR_TRACE')
FORMS = {'device': None, 'host_loop': 'MVUS_LSMR_HOST', 'one_pass': 'MVUS_LSMR_ONE_PASS'}
EXACT = dict(atol=0.0, btol=0.0, conlim=0.0)
NORMS = ref.NORMS
STOP_NORMS = ('normA', 'condA')      # at a converged stop normr and normar are rounding noise themselves: no relative deviation to speak of


def _handle(monkeypatch, lay, switch=None):
    """a handle created with ``switch`` set (and the other LSMR switches unset), the mask of the layout in force and the analytic Jacobian
    of x0 held; MVUS_LSMR_ONE_PASS stays set for the runs that follow (it is read at every run)"""
    from mvus_amd.ba import BAHandle
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    if switch:
        monkeypatch.setenv(switch, '1')
    h = BAHandle(lay.prob)
    if lay.frozen is not None:
        h.set_frozen(lay.frozen)
    _, _, ctrl = h.residual_jacobian(lay.x0, _lib.JAC_ANALYTIC)
    L.check_branches(lay, ctrl, h.T)
    if switch and switch != 'MVUS_LSMR_ONE_PASS':
        monkeypatch.delenv(switch)                       # (read at creation: later handles of the test are not affected)
    return h


def _run(h, lay, b, k, damp=0.0, **tol):
    return h.lsmr(b, lay.D, lay.E, damp=damp, maxiter=k, **(tol or EXACT))


def _same_bits(a, b):
    return (a.itn, a.istop) == (b.itn, b.istop) and np.array_equal(a.x, b.x) and all(getattr(a, k) == getattr(b, k) for k in NORMS)


def _own_operator(h, lay, hc):
    """A = [J diag(D); diag(E)] in longdouble from the Jacobian the GPU itself holds (its slot arrays scattered in numpy).  It is the host
    build's Jacobian up to the rounding of its entries -- asserted: a wrong scatter would be O(1)."""
    _, J, ctrl = h.residual_jacobian(lay.x0, _lib.JAC_ANALYTIC)
    _, mJ, mctrl = h.motion_rows(lay.x0, _lib.JAC_ANALYTIC)
    Jown = L.dense_from_slots(lay.prob, J, ctrl, mJ, mctrl, lay.frozen)
    assert np.linalg.norm(Jown - hc.Jref) <= 1e-9 * np.linalg.norm(hc.Jref)
    return ref.dense_operator(Jown, lay.D, lay.E, np.longdouble), float(np.linalg.norm(Jown - hc.Jref) / np.linalg.norm(hc.Jref))


def _accuracy(h, lay, name, form, bkeys, damp=0.0):
    """Every (b, k), two references:
      host-J: the longdouble LSMR on the HOST build's dense Jacobian.  |x - x_ref| / |x_ref| <= 8 dev_host(layout, k).
      own-J:  the same LSMR on the Jacobian the GPU holds.  The GPU evaluates its own Jacobian, whose entries differ from the host build's in
              their last bits (|dJ|_F / |J|_F is 1e-15 .. 1e-14, printed), and the host-J figure is mostly that difference, not the loop's
              arithmetic; dev_host contains none of it, the host build and the reference sharing one Jacobian.
              Against its own Jacobian the loop is held to the same multiples: x to 8 dev_host, the four norm estimates to
              8 max(dev_host, the host build's own deviation in them) -- like against like.
    The figures are printed, then the misses are asserted together."""
    hc = L.host_case(name)
    Aown, dj = _own_operator(h, lay, hc)
    print('lsmr-dJ  %-12s %-9s |J_gpu - J_host|_F / |J_host|_F = %.3e' % (name, form, dj))
    misses = []
    for bkey in bkeys:
        own = ref.lsmr_iterates(Aown, hc.rhs[bkey], damp, max(L.KS), np.longdouble)
        for k in L.KS:
            r, o = L.reference(name, bkey, damp)[k - 1], own[k - 1]
            dx_host, dn_host = L.dev_host(name, bkey, k, damp)
            got = _run(h, lay, hc.rhs[bkey], k, damp)
            dx, dxo, dno = ref.rel_dev(got.x, r.x), ref.rel_dev(got.x, o.x), ref.norms_dev(got, o)
            bar_x, bar_n = FACTOR * dx_host, FACTOR * max(dx_host, dn_host)
            print('lsmr-dev %-12s %-9s b=%-4s damp=%-4g k=%d  dev_host %.3e  host-J: x %.3e (%.2f dev_host)  own-J: x %.3e (%.2f dev_host) norms %.3e (bar %.3e)'
                  % (name, form, bkey, damp, k, dx_host, dx, dx / dx_host, dxo, dxo / dx_host, dno, bar_n))
            if (got.itn, got.istop) != (k, 7):
                misses.append((bkey, k, 'itn, istop', got.itn, got.istop))
            if not dx <= bar_x:
                misses.append((bkey, k, 'x against the host-J reference', dx, bar_x))
            if not dxo <= bar_x:
                misses.append((bkey, k, 'x against the own-J reference', dxo, bar_x))
            if not dno <= bar_n:
                misses.append((bkey, k, 'norms against the own-J reference', dno, bar_n))
            if lay.frozen is not None and got.x[np.nonzero(lay.frozen)[0]].any():
                misses.append((bkey, k, 'frozen entries of x are not exactly 0.0'))
    assert not misses, misses


@pytest.mark.parametrize('form', list(FORMS))
@pytest.mark.parametrize('name', L.NAMES)
def test_iterates_match_the_longdouble_reference(monkeypatch, name, form):
    """k = 1..4 iterations, b = the residual and a seeded random b: |x - x_ref| / |x_ref| <= 8 dev_host(layout, k), the norm estimates,
    (itn, istop) = (k, 7); `frozen`: the frozen entries of x are exactly 0.0.  `wide` is held to the same bar (its atomics are one more
    summation order)."""
    lay = L.build(name)
    with _handle(monkeypatch, lay, FORMS[form]) as h:
        _accuracy(h, lay, name, form, ('f', 'rand'))


@pytest.mark.parametrize('form', list(FORMS))
def test_damped_iterates_match_the_reference(monkeypatch, form):
    """damp > 0 (the unbounded trust-region problem's regularisation) on `plain`"""
    lay = L.build('plain')
    with _handle(monkeypatch, lay, FORMS[form]) as h:
        _accuracy(h, lay, 'plain', form, ('f',), damp=L.DAMP)


@pytest.mark.parametrize('name', [n for n in L.NAMES if n != 'wide'])
def test_twelve_iterations_bit_for_bit(monkeypatch, name):
    """12 iterations cross the batch boundary at 8.  The device-resident loop gives the bits of the host-driven loop (x, itn, istop, the
    norms) -- on `scaled` also those of MVUS_LSMR_BOUNDED_HOST -- and each form gives the same bits on a second run of the same handle (the
    index built at the first launch of a run, the J^T u accumulator the consumer clears) and leaves the held Jacobian as it was."""
    lay = L.build(name)
    hc = L.host_case(name)
    u = np.random.default_rng(5).normal(size=hc.h.m)
    runs = {}
    with _handle(monkeypatch, lay) as h:
        z0 = h.jtu(u)
        for bkey, b in hc.rhs.items():
            runs['device', bkey] = _run(h, lay, b, 12)
            assert _same_bits(_run(h, lay, b, 12), runs['device', bkey]), ('device, second run', bkey)
        monkeypatch.setenv('MVUS_LSMR_ONE_PASS', '1')
        for bkey, b in hc.rhs.items():
            one = _run(h, lay, b, 12)
            assert _same_bits(_run(h, lay, b, 12), one), ('one_pass, second run', bkey)
            assert (one.itn, one.istop) == (12, 7)
        monkeypatch.delenv('MVUS_LSMR_ONE_PASS')
        for bkey, b in hc.rhs.items():                                   # and the two-pass loop after the one-pass loop, same handle
            assert _same_bits(_run(h, lay, b, 12), runs['device', bkey]), ('device after one_pass', bkey)
        assert np.array_equal(h.jtu(u), z0)
    others = ['MVUS_LSMR_HOST'] + (['MVUS_LSMR_BOUNDED_HOST'] if name == 'scaled' else [])
    for switch in others:
        with _handle(monkeypatch, lay, switch) as h:
            for bkey, b in hc.rhs.items():
                got = _run(h, lay, b, 12)
                assert (got.itn, got.istop) == (12, 7)
                assert _same_bits(got, runs['device', bkey]), (switch, bkey, ref.rel_dev(got.x, runs['device', bkey].x.astype(np.longdouble)))
                assert _same_bits(_run(h, lay, b, 12), got), (switch, 'second run', bkey)


# LM + Schur assembles detection-major (fp64 atomics) when a camera's frames are out of order: no bits to compare on those layouts
SOLVERS = {'trf': ([n for n in L.NAMES if n != 'wide'], _lib.SOLVER_TRF_LSMR),
           'lm': (['plain', 'calib', 'many_cameras', 'frozen'], _lib.SOLVER_LM_SCHUR)}


@pytest.mark.parametrize('solver,name', [(s, n) for s in SOLVERS for n in SOLVERS[s][0]])
def test_a_solve_after_the_call_is_the_solve_before_it(monkeypatch, solver, name):
    """mvus_ba_lsmr changes no solver state: a 3-evaluation solve on a handle that ran it (both forms) returns the bits of the same solve on
    a handle that did not."""
    lay = L.build(name)
    hc = L.host_case(name)
    out = []
    for call in (False, True):
        with _handle(monkeypatch, lay) as h:
            if call:
                _run(h, lay, hc.rhs['f'], 3)
                monkeypatch.setenv('MVUS_LSMR_ONE_PASS', '1')
                _run(h, lay, hc.rhs['rand'], 3)
                monkeypatch.delenv('MVUS_LSMR_ONE_PASS')
            out.append(h.solve(lay.x0, solver=SOLVERS[solver][1], jac_mode=_lib.JAC_ANALYTIC, max_nfev=3))
    a, b = out
    assert np.array_equal(a.x, b.x) and a.cost == b.cost and (a.nfev, a.njev, a.status) == (b.nfev, b.njev, b.status)
    assert np.array_equal(a.fun, b.fun)


def test_stopping_inside_a_batch(monkeypatch):
    """`plain`, default tolerances (1e-6, 1e-6, 1e8), a b for which the reference stops at iteration 5 -- inside the first batch of 8 -- with
    its deciding quantity a factor >= 2 from the threshold there and one iteration earlier (asserted in test_lsmr_host.py and here).  Every
    form returns that itn and istop and the reference's x at that iteration, to 8 x the host build's deviation at that iteration (normA and
    condA the same way; normr and normar are at rounding level there, and what they decide -- istop -- is asserted itself); the
    device-resident loop, whose launches 6..8 are no-ops, returns the bits of the host-driven loop, which stops launching."""
    lay = L.build('plain')
    sc = L.stopping_case()
    assert sc.itn % 8 != 0 and 1 < sc.itn < 8 and sc.margin >= 2
    host = L.host_run('plain', sc.b, 0, **L.STOP_TOL)
    assert (host.itn, host.istop) == (sc.itn, sc.istop)
    dx_host, dn_host = ref.rel_dev(host.x, sc.ref.x), ref.norms_dev(host, sc.ref, STOP_NORMS)
    got = {}
    for form, switch in FORMS.items():
        with _handle(monkeypatch, lay, switch) as h:
            got[form] = r = _run(h, lay, sc.b, 0, **L.STOP_TOL)
            again = _run(h, lay, sc.b, 0, **L.STOP_TOL)
        dx, dn = ref.rel_dev(r.x, sc.ref.x), ref.norms_dev(r, sc.ref, STOP_NORMS)
        print('lsmr-stop %-9s itn %d istop %d  x %.3e (bar %.3e)  normA, condA %.3e (bar %.3e)'
              % (form, r.itn, r.istop, dx, FACTOR * dx_host, dn, FACTOR * max(dx_host, dn_host)))
        assert (r.itn, r.istop) == (sc.itn, sc.istop)
        assert dx <= FACTOR * dx_host and dn <= FACTOR * max(dx_host, dn_host)
        assert _same_bits(again, r)
    assert _same_bits(got['device'], got['host_loop'])


def test_refusals(monkeypatch):
    """No Jacobian held: MVUS_E_INVALID, as mvus_ba_jtu; a sharded handle (all-reduce route or time shard): MVUS_E_UNSUPPORTED; bad
    arguments: MVUS_E_INVALID."""
    from mvus_amd.ba import BAHandle, UnsupportedBySolver
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    lay = L.build('plain')
    b = L.host_case('plain').rhs['f']
    with BAHandle(lay.prob) as h:
        with pytest.raises(ValueError, match='no Jacobian held'):
            h.lsmr(b, maxiter=1)
        h.residual_jacobian(lay.x0, _lib.JAC_ANALYTIC)
        assert h.lsmr(b, maxiter=1, **EXACT).itn == 1
        with pytest.raises(ValueError, match='bad arguments'):
            h.lsmr(b, damp=-1.0, maxiter=1)
        x = np.zeros(h.n)
        assert h.lib.mvus_ba_lsmr(h.h, None, None, None, 0.0, 0.0, 0.0, 0.0, 1, _lib.dptr(x), None, None, None) == _lib.MVUS_E_INVALID
        assert h.lib.mvus_ba_lsmr(h.h, _lib.dptr(b), None, None, 0.0, 0.0, 0.0, 0.0, 1, None, None, None, None) == _lib.MVUS_E_INVALID
        assert h.lib.mvus_ba_lsmr(h.h, _lib.dptr(b), None, None, 0.0, 0.0, 0.0, 0.0, 1, _lib.dptr(x), None, None, None) == 0      # the outputs beside x are optional
    with BAHandle(lay.prob) as h:
        h.residual_jacobian(lay.x0, _lib.JAC_ANALYTIC)
        h.set_allreduce(lambda buf, count, stream: None)
        with pytest.raises(UnsupportedBySolver, match='sharded'):
            h.lsmr(b, maxiter=1)
    N = int(lay.prob.n_coef.sum())
    with BAHandle(lay.prob) as h:
        h.set_time_shard(0, 2, [0, N // 2, N])          # (drops the held Jacobian: the refusal comes first)
        with pytest.raises(UnsupportedBySolver, match='sharded'):
            h.lsmr(b, maxiter=1)
