"""The damped step of the whole HipSchur chain (mvus_ba_lm_step), held to its backward error on the Jacobi-scaled system the device itself
exported (tests/schur_reference.py), on every route a switch of mvus_amd/csrc/ba_switches.h selects through the solve.

The older tests compare the step with an fp64 solve at 1e-7 ... 1e-8 of max |p|: one max-norm over angles, pixels and metres, against a
reference that is itself only fp64.  A step wrong in the sixth digit passes that (tests/test_schur_reference_host.py shows it).  Here:

  1. eta <= 64 * max(eta_ref, 1e-15), eta_ref that of lapack_lm_step on the same blocks (lm_reference.eta_bound; a route with a factor of
     its own is listed in lm_reference.ROUTE_FACTOR with its reason, and in DESIGN.md section 4.10);
  2. eta <= 1e-11 on every case, whatever the factor;
  3. where n <= 1000: forward_scaled(p, p*) <= 2 kappa (bound of 1), p* the long-double-refined solve;
  4. every route's step agrees with the default route's to forward_scaled <= 2 kappa (bound of 1).

Every case prints eta, eta_cam, eta_spline and eta_ref: the table of DESIGN.md section 4.10 is that output."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

import schur_reference as sr
from lm_reference import SOLVE_ROUTES, backward_error, route_factor
from mvus_amd import _lib
from mvus_amd import problem as mp

pytestmark = pytest.mark.gpu

LAMS = (1e-4, 1e-3, 0.7)
KAPPA_MAX_N = 2000            # kappa (one dense inverse per scene and lambda) also for scenes D and K, n = 1296 and 1956: assertion 4 needs it on every route

# every switch that changes the solve route: cleared before each handle
SWITCHES = ('MVUS_RCS', 'MVUS_RCS_TRSM', 'MVUS_RCS_SPIN_LIMIT', 'MVUS_SEP_SEQUENTIAL', 'MVUS_BCR_FUSED', 'MVUS_PART_BACK', 'MVUS_DIRECT_RHS',
            'MVUS_NO_OVERLAP', 'MVUS_PART_LEN', 'MVUS_GEMM_SLABS', 'MVUS_DEBUG')

ROUTES = SOLVE_ROUTES
_CAMERA = ['rcs_gj', 'rcs_trsm_launch']
_BAND = ['part_back', 'rhs_copy', 'no_overlap']
# Each switch on the scenes where it changes what runs: reach() below states the condition for every route and every case asserts it.
SCENE_ROUTES = {
    'A': [],                                           # P = 6, one to two interiors, no level chain
    # P = 15, B = 18; 90 camera unknowns: interiors of 16 by default, and ONE super-panel -- no rows below it, MVUS_RCS_TRSM has nothing to move
    'B': ['rcs_gj'] + _BAND + ['part_len_32'],
    'C': _CAMERA,                                      # 153 camera unknowns: one block row below the first super-panel of 144
    # 297 camera unknowns: three super-panels; more than 128, so interiors of 32 by default and its 27 control points are ONE interior --
    # MVUS_PART_BACK and MVUS_DIRECT_RHS act on separators only (HipSchur::plan_separators), so they run together with MVUS_PART_LEN=16;
    # 81 rows are six row sets: the slab plan is one slab by itself
    'G': _CAMERA + ['no_overlap', 'part_len_16', 'part_len_16_part_back', 'part_len_16_rhs_copy', 'slabs_3', 'slabs_8'],
    # 423 control points: 22 separators by default (one wide level), 12 / 46 with interiors of 32 / 6; 20 slabs by the plan
    'D': ['sep_sequential'] + _BAND + ['part_len_32', 'slabs_1', 'slabs_3', 'slabs_8', 'part_len_6', 'part_len_6_sequential'],
    'E': [],                                           # wide band: k_band_chol_generic / k_band_solve_generic
    'F': ['sep_sequential'],                           # two splines: two chains
    'H': [],                                           # a camera without detections: zero block, D falls back to 1
    # 643 control points: 71 separators with interiors of 6 -- TWO wide levels of the cyclic reduction, the fewest at which they run in one
    # launch (k_sep_bcr_levels) and MVUS_BCR_FUSED=0 changes anything (HipSchur::bcr_fused_levels)
    'K': ['part_len_6', 'part_len_6_bcr_per_level', 'part_len_6_sequential'],
}
SCENE_LAMS = {'H': (1e-3, 0.7)}
CASES = [(s, r) for s, routes in SCENE_ROUTES.items() for r in ['default'] + routes]


@functools.lru_cache(maxsize=None)
def scene(name):
    """(prob, x) of a scene of the table."""
    from mvus_amd import synth
    if name == 'F':
        from golden_util import load_case
        sc, g = load_case('rs_F_2int_3cam')
        prob, _ = mp.problem_from_scene(sc)
        return prob, g['x0'] + g['delta']
    make = functools.partial(synth.make_scene, rolling_shutter=True)
    if name in ('A', 'H'):
        sc = make(3, 1200, seed=103, num_knots=40)
        if name == 'H':
            sc.detections[2] = sc.detections[2][:, :0]
    elif name == 'B':
        sc = make(5, 1400, seed=105, num_knots=64, opt_calib=True)
    elif name == 'C':
        sc = make(17, 1420, seed=117, num_knots=24)
    elif name == 'G':
        sc = make(33, 2380, seed=133, num_knots=24)
    elif name == 'D':
        sc = make(3, 3000, seed=31, num_knots=420)
    elif name == 'K':
        sc = make(3, 4500, seed=71, num_knots=640)
    elif name == 'E':
        sc = make(3, 420, seed=61, knot_spacing=0.3, motion_reg=True, motion_type='KE', motion_weights=40.0)
    return mp.problem_from_scene(sc)


def partition(n, sctrl, length, part_l=32):
    """mvus::partition_chain (ba_partition.h) for an open chain of n control points: the first control point of every separator."""
    length = max(2 * sctrl, min(length, part_l))
    g, seps = 0, []
    while g < n:
        g = min(g + length, n)
        if g < n:
            e2 = min(g + sctrl, n)
            if n - e2 < 1:
                g = n                                   # tail too short for another interior: merged
            else:
                seps.append(g)
                g = e2
    return seps


def separators(n, sctrl, length):
    return len(partition(n, sctrl, length))


def wide_levels(m, tail=16):
    """Levels of the separators' cyclic reduction with more than kBcrTailNs = 16 survivors (HipSchur::bcr_fused_levels): they run in ONE
    launch where there are two to four of them."""
    h, n = 1, 0
    while h <= m and m // (2 * h) > tail:
        h, n = 2 * h, n + 1
    return n


def plan_slabs(CB, rows, cus, forced=0):
    """mvus::gemm_plan_slabs (ba_gemm_plan.h)."""
    if forced > 0:
        return forced
    nbk = (CB + 47) // 48
    tiles, slots, nsets = nbk * (nbk + 1) // 2, max(8, 2 * cus), max(1, (rows + 15) // 16)
    nslab, best, s_ = 1, 1e300, 1
    while s_ <= 128 and 4 * s_ <= nsets:
        per_wave, on_xcd = (nsets + 4 * s_ - 1) // (4 * s_), tiles * ((s_ + 7) // 8)
        cost = float((on_xcd + slots // 8 - 1) // (slots // 8)) * (per_wave + 1.5) + 0.002 * s_
        if cost < best * 0.995:
            best, nslab = cost, s_
        s_ += 1
    return nslab


def reach(route, CB, N, W, cus):
    """What must hold of a scene for the route to run anything the default route does not (read off HipSchur's constructor and solve):
    a list of (condition, what it is).  Every case asserts its own."""
    env = ROUTES[route]
    wide, sctrl = W > 6, W - 1
    own = 16 if CB <= 128 else 32                                                  # HipSchur::plan_partition
    length = int(env.get('MVUS_PART_LEN', own))
    m = 0 if wide else separators(N, sctrl, length)
    out = []
    if 'MVUS_RCS_TRSM' in env:
        out.append(((CB + 15) // 16 > 9, 'block rows below the first super-panel of nine'))
    if 'MVUS_PART_LEN' in env:
        out.append((not wide and partition(N, sctrl, length) != partition(N, sctrl, own), 'another partition than the default length gives'))
    if 'MVUS_SEP_SEQUENTIAL' in env or 'MVUS_PART_BACK' in env or 'MVUS_DIRECT_RHS' in env:
        out.append((m > 0, 'a separator'))
    if 'MVUS_NO_OVERLAP' in env:
        out.append((not wide, 'the partitioned band solver'))
    if 'MVUS_BCR_FUSED' in env:
        out.append((2 <= wide_levels(m) <= 4, 'two to four wide reduction levels: 68 to 543 separators'))
    if 'MVUS_GEMM_SLABS' in env:
        out.append((plan_slabs(CB, 3 * N, cus) != int(env['MVUS_GEMM_SLABS']), 'a slab count the plan does not choose itself'))
    if env.get('MVUS_PART_LEN') == '6':
        out.append((m > 16, 'more than 16 separators: several reduction levels'))
    return out


def run(name, env, monkeypatch):
    """One handle on the route `env`: the blocks it exported and its step for every lambda of the scene."""
    from mvus_amd.ba import BAHandle
    prob, x = scene(name)
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    try:
        with BAHandle(prob) as h:
            h.residual_jacobian(x, _lib.JAC_ANALYTIC)
            blocks = h.normal_equations()
            steps = {lam: h.lm_step(lam) for lam in SCENE_LAMS.get(name, LAMS)}
    finally:
        for k in env:
            monkeypatch.delenv(k)
    return SimpleNamespace(blocks=blocks, steps=steps)


_default_runs = {}
_references = {}


def default_run(name, monkeypatch):
    if name not in _default_runs:
        _default_runs[name] = run(name, {}, monkeypatch)
    return _default_runs[name]


def reference(name, lam, blocks):
    """kappa and the refined solve p* of the system a handle exported: computed once per (scene, lambda) and shared while the routes
    export the same bits (the assembly does not depend on the solve route), computed again for blocks that differ."""
    prob, _ = scene(name)
    key = (name, lam)
    ref = _references.get(key)
    if ref is None or not all(np.array_equal(a, b) for a, b in zip(ref.blocks, blocks)):
        n = prob.n_params
        ref = _references[key] = SimpleNamespace(
            blocks=blocks, kappa=sr.kappa(prob, *blocks, lam, limit=KAPPA_MAX_N) if n <= KAPPA_MAX_N else None,
            p_star=sr.refined(prob, *blocks, lam) if n <= sr.DENSE_MAX else None)
    return ref


def test_the_scenes_reach_what_the_table_says():
    sizes = {name: (scene(name)[0].C * (3 + scene(name)[0].P), int(scene(name)[0].n_coef.sum()), scene(name)[0].n_params) for name in SCENE_ROUTES}
    print(sizes)
    assert scene('A')[0].P == 6 and scene('B')[0].P == 15
    assert sizes['C'][0] == 153 and sizes['G'][0] == 297 and sizes['B'][0] <= 128 < sizes['C'][0]
    # up to 128 camera unknowns the interiors are 16 control points long, 32 beyond (HipSchur::plan_partition)
    assert 1 <= separators(sizes['A'][1], 3, 16) <= 2
    assert separators(sizes['G'][1], 3, 32) == 0 < separators(sizes['G'][1], 3, 16) and separators(sizes['B'][1], 3, 32) > 0
    assert separators(sizes['D'][1], 3, 6) > separators(sizes['D'][1], 3, 16) > 16 > separators(sizes['D'][1], 3, 32) >= 6
    assert wide_levels(separators(sizes['D'][1], 3, 6)) == 1 and wide_levels(separators(sizes['K'][1], 3, 6)) == 2
    assert [wide_levels(m) for m in (33, 34, 67, 68, 543, 544)] == [0, 1, 1, 2, 4, 5]
    assert len(scene('F')[0].n_coef) == 2
    assert all(sizes[name][2] <= sr.DENSE_MAX for name in 'ABCGFH') and all(sr.DENSE_MAX < sizes[name][2] <= KAPPA_MAX_N for name in 'DK')


@pytest.mark.parametrize('name,route', CASES, ids=['%s-%s' % c for c in CASES])
def test_backward_error_of_the_step(name, route, monkeypatch):
    prob, _ = scene(name)
    base = default_run(name, monkeypatch)
    cur = base if route == 'default' else run(name, ROUTES[route], monkeypatch)
    g, A, band, cross = cur.blocks
    N, W = band.shape[0], band.shape[1]
    if name == 'E':
        assert W > 6, 'the band is not wide: the generic kernels did not run'
    if name == 'H':
        assert not A[2].any() and A[0].any(), 'camera 2 was meant to have a zero block'
    import torch
    for ok, what in reach(route, A.shape[0] * A.shape[1], N, W, torch.cuda.get_device_properties(0).multi_processor_count):
        assert ok, 'scene %s does not reach what %s changes: it needs %s' % (name, route, what)
    factor = route_factor(route)
    failures = []
    for lam, p in cur.steps.items():
        ref = reference(name, lam, cur.blocks)
        e, e_ref, bound = backward_error(prob, g, A, band, cross, lam, p, '%s %s' % (name, route), factor)
        if not (np.isfinite(p).all() and e.eta <= bound):
            failures.append('lambda %g: eta %.3g (cam %.3g, spline %.3g) > %.3g; eta_ref %.3g' % (lam, e.eta, e.cam, e.spline, bound, e_ref.eta))
        if ref.p_star is not None:
            fwd = sr.forward_scaled(prob, g, A, band, cross, lam, p, ref.p_star)
            print('    forward_scaled against the refined solve %.3g, 2 kappa bound = %.3g (kappa %.3g)' % (fwd, 2 * ref.kappa * bound, ref.kappa))
            if not fwd <= 2 * ref.kappa * bound:
                failures.append('lambda %g: forward error %.3g > 2 kappa bound = %.3g' % (lam, fwd, 2 * ref.kappa * bound))
        if cur is not base:
            apart = sr.forward_scaled(prob, g, A, band, cross, lam, p, base.steps[lam])
            print('    forward_scaled against the default route %.3g' % apart)
            if not apart <= 2 * ref.kappa * bound:
                failures.append('lambda %g: %.3g from the default route > 2 kappa bound = %.3g' % (lam, apart, 2 * ref.kappa * bound))
    assert not failures, failures
