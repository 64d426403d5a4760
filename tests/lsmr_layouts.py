"""Seeded BA problems that steer the J^T u / LSMR kernels (k_jtu_partial, k_jvjtu, k_jtu_index, k_jtu_first, k_jtu_reduce) into each of
their branches, for tests/test_lsmr_host.py and tests/test_gpu_lsmr.py.  All are synth.make_scene scenes with rolling shutter, motion rows
and the analytic Jacobian, kept as small as the branch allows.

A CHUNK is 256 consecutive detections of a camera (one workgroup of the kernels).  ``branches(prob, ctrl, T)`` says, from the span array
``ctrl`` of a Jacobian (first control point per detection, -1 = not visible: BAHandle.residual_jacobian / HostHandle.spans), which branches
the kernels take on it, by the kernels' own rules; every layout names the branches it exists for in ``needs`` and both test files assert
them, so a layout that stops reaching its branch fails instead of passing."""
import functools
from types import SimpleNamespace

import numpy as np

from mvus_amd import problem as mp
from mvus_amd import synth

CHUNK = 256        # kThreads: detections per chunk
JT_WIN = 144       # kJtWin: control points per chunk window of the J^T u gather


def xcd_grid(tiles):
    """workgroups launched for ``tiles`` chunks (xcd_grid of ba_dev_problem.h): whole runs on all eight XCDs"""
    run = min(64, max(1, (tiles + 7) // 8))
    per = 8 * run
    return (tiles + per - 1) // per * per


def branches(prob, ctrl, T):
    """(set of branch names, dict of measured figures) for the span array ``ctrl``"""
    ctrl = np.asarray(ctrl)
    found, slack_max, ext_max, n_chunks = set(), 0, 0, 0
    for c in range(prob.C):
        a, b = int(prob.det_offsets[c]), int(prob.det_offsets[c + 1])
        if b - a == CHUNK:
            found.add('camera_of_256')
        carry = None
        for s in range(a, b, CHUNK):
            n_chunks += 1
            g = ctrl[s:min(s + CHUNK, b)]
            if g.size == 1:
                found.add('tail_of_1')
            tid = np.nonzero(g >= 0)[0]
            if tid.size == 0:
                found.add('invisible_chunk')             # zg0 = 0x7fffffff: pass 2 skips the chunk
                continue
            if tid.size < g.size:
                found.add('invisible_rows')              # rows without a span inside a chunk that has some
            vis = g[tid]
            g0 = int(vis.min())
            if int(vis.max()) - g0 + 3 >= JT_WIN:
                found.add('wide')                        # wide_s: atomics, the chunk leaves the index
                continue
            ext_max = max(ext_max, int(vis.max()) - g0 + 4)
            spans = np.unique(vis)
            lo = np.array([tid[vis == v].min() for v in spans])
            hi = np.array([tid[vis == v].max() + 1 for v in spans])
            if np.any(lo[1:] < hi[:-1]):
                found.add('interleaved')                 # bad_s: every detection in index order
            carry = g0 if carry is None else max(carry, g0)
            slack_max = max(slack_max, carry - g0)       # bounds[0]: how far a chunk starts below the running maximum
    if slack_max > 0:
        found.add('walk')
    if prob.C > 64:
        found.add('cameras_past_lane_63')
    if xcd_grid(n_chunks) != n_chunks:
        found.add('padded_tiles')
    if T > 0:
        found.add('motion_rows')
    off = prob.ctrl_offsets
    if prob.S >= 2 and all(np.any((ctrl >= off[s]) & (ctrl < off[s + 1])) for s in range(prob.S)):
        found.add('two_intervals')
    return found, dict(slack=slack_max, ext=ext_max, n_chunks=n_chunks, grid=xcd_grid(n_chunks))


def _scene(num_cam, total_obs, seed, **kw):
    args = dict(seed=seed, rolling_shutter=True, motion_reg=True, motion_type='F', num_intervals=2, outlier_frac=0.0)
    args.update(kw)
    return synth.make_scene(num_cam, total_obs, **args)


def _plain(**kw):
    return _scene(3, 900, 11, num_knots=24, **kw)


def _edges():
    sc = _plain()
    d = sc.detections
    assert d[0].shape[1] >= 256 and d[1].shape[1] >= 257 and d[2].shape[1] >= 300
    d[0] = d[0][:, :256].copy()
    d[1] = d[1][:, :257].copy()
    d[2] = d[2].copy()
    d[2][0, :256] -= 1e5                      # the first chunk of camera 2 lies before every interval
    return sc


def _interleaved():
    sc = _scene(3, 3000, 12, knot_spacing=15.0)
    rng = np.random.default_rng(120)
    d0 = sc.detections[0]
    perm = np.concatenate([a + rng.permutation(min(16, d0.shape[1] - a)) for a in range(0, d0.shape[1], 16)])
    sc.detections[0] = d0[:, perm].copy()
    d1 = sc.detections[1]
    blocks = [np.arange(a, min(a + 64, d1.shape[1])) for a in range(0, d1.shape[1], 64)]
    sc.detections[1] = d1[:, np.concatenate([blocks[i] for i in rng.permutation(len(blocks))])].copy()      # a permutation of the whole camera, 64 at a time
    return sc


def _wide():
    sc = _scene(3, 1800, 13, num_knots=400, num_intervals=1)
    sc.detections[1] = sc.detections[1][:, ::9].copy()
    return sc


def _many_cameras():
    sc = _scene(70, 2500, 14, num_knots=24)
    total = sum(d.shape[1] for d in sc.detections)
    step = max(1, int(round(total / 2500.0)))
    sc.detections = [d[:, (c % step)::step].copy() for c, d in enumerate(sc.detections)]
    return sc


def _frozen_mask(prob):
    C, P = prob.C, prob.P
    mask = np.zeros(C * (3 + P), dtype=np.uint8)
    mask[[0, C, 2 * C + 1]] = 1                       # alpha and beta of camera 0, rs of camera 1
    mask[3 * C + 2 * P:3 * C + 3 * P] = 1             # the pose of camera 2
    return mask


# name -> (scene builder, branches the layout exists for)
LAYOUTS = {
    'plain': (_plain, {'motion_rows', 'two_intervals', 'padded_tiles'}),
    'calib': (lambda: _plain(distortion=True, opt_calib=True), {'motion_rows', 'two_intervals'}),
    'edges': (_edges, {'camera_of_256', 'tail_of_1', 'invisible_chunk', 'invisible_rows', 'motion_rows'}),
    'interleaved': (_interleaved, {'interleaved', 'walk', 'motion_rows'}),
    'wide': (_wide, {'wide', 'motion_rows'}),
    'many_cameras': (_many_cameras, {'cameras_past_lane_63', 'padded_tiles', 'motion_rows'}),
    # variants of `plain`: the bounded problem's scaling, and a frozen mask (no new branch)
    'scaled': (_plain, {'motion_rows'}),
    'frozen': (_plain, {'motion_rows'}),
}
NAMES = list(LAYOUTS)
MIN_SLACK = 8      # `interleaved`: a chunk starts at least this many control points below the running maximum ("far below")


@functools.lru_cache(maxsize=None)
def build(name):
    """prob, x0, the scaling (D, E) and the frozen mask (None where the layout has none), the branches it must reach"""
    make, needs = LAYOUTS[name]
    prob, x0 = mp.problem_from_scene(make())
    n = prob.n_params
    D = E = frozen = None
    if name == 'scaled':
        rng = np.random.default_rng(150)
        D = rng.uniform(0.1, 1.0, n)
        E = rng.uniform(0.0, 1.0, n)
        E[rng.choice(n, n // 5, replace=False)] = 0.0
    if name == 'frozen':
        frozen = _frozen_mask(prob)
    return SimpleNamespace(name=name, prob=prob, x0=x0, D=D, E=E, frozen=frozen, needs=set(needs),
                           NS=30 if prob.opt_calib else 21)


def check_branches(lay, ctrl, T):
    """assert that ``ctrl`` reaches what the layout exists for; returns the measured figures"""
    found, fig = branches(lay.prob, ctrl, T)
    assert lay.needs <= found, '%s no longer reaches %s (reaches %s, %s)' % (lay.name, sorted(lay.needs - found), sorted(found), fig)
    if lay.name == 'interleaved':
        assert fig['slack'] >= MIN_SLACK, fig
    if lay.name == 'many_cameras':
        assert fig['n_chunks'] % 8 != 0 and fig['grid'] > fig['n_chunks'], fig
    if lay.name == 'wide':
        assert 'interleaved' not in lay.needs
    return fig


def random_rhs(lay, m):
    """the seeded random right-hand side of the tests"""
    return np.random.default_rng(1000 + NAMES.index(lay.name)).normal(size=m)


# ---- what both test files compute once per layout: the host build's Jacobian, the longdouble reference and the host build's deviation ----
KS = (1, 2, 3, 4)
DAMP = 0.37        # the damp > 0 of the tests (plain only), of the order of the columns' norms


@functools.lru_cache(maxsize=None)
def host_case(name):
    """The layout on the plain C++ backend: f(x0), the dense analytic Jacobian (frozen columns zeroed for `frozen`), its span array, the
    right-hand sides {'f': residual, 'rand': seeded random} and A = [J diag(D); diag(E)] in longdouble."""
    import lsmr_reference as ref
    from hostcheck_util import HostHandle
    from mvus_amd import _lib
    lay = build(name)
    h = HostHandle(lay.prob)
    f, J = h.dense_jacobian(lay.x0, _lib.JAC_ANALYTIC)
    ctrl = h.spans()
    fig = check_branches(lay, ctrl, h.T)
    Jref = J.copy()
    if lay.frozen is not None:
        Jref[:, np.nonzero(lay.frozen)[0]] = 0.0
    A = ref.dense_operator(Jref, lay.D, lay.E, np.longdouble)
    return SimpleNamespace(lay=lay, h=h, f=f, J=J, Jref=Jref, ctrl=ctrl, fig=fig, A=A, rhs={'f': f, 'rand': random_rhs(lay, h.m)})


@functools.lru_cache(maxsize=None)
def reference(name, bkey, damp=0.0, k=max(KS)):
    """records of the longdouble reference after each of k iterations (lsmr_reference.lsmr_iterates), tolerances 0"""
    import lsmr_reference as ref
    hc = host_case(name)
    return ref.lsmr_iterates(hc.A, hc.rhs[bkey], damp, k, np.longdouble)


def host_run(name, b, k, damp=0.0, **tol):
    hc = host_case(name)
    tol = tol or dict(atol=0.0, btol=0.0, conlim=0.0)
    return hc.h.lsmr(b, hc.lay.D, hc.lay.E, damp=damp, maxiter=k, frozen=hc.lay.frozen, **tol)


@functools.lru_cache(maxsize=None)
def dev_host(name, bkey, k, damp=0.0):
    """(dev_host(layout, k) = |x_host - x_ref|_2 / |x_ref|_2, the same for the four norm estimates) of the host build after exactly k
    iterations on right-hand side ``bkey``"""
    import lsmr_reference as ref
    r = reference(name, bkey, damp)[k - 1]
    got = host_run(name, host_case(name).rhs[bkey], k, damp)
    assert (got.itn, got.istop) == (k, 7)
    return ref.rel_dev(got.x, r.x), ref.norms_dev(got, r)


def dense_from_slots(prob, J, ctrl, mJ, mctrl, frozen=None):
    """The (m, n) matrix of a Jacobian in the slot layout of include/mvus_ba.h -- J[2, NS, M] and ctrl[M] of BAHandle.residual_jacobian, mJ[36, T]
    and mctrl[3, T] of BAHandle.motion_rows -- scattered in numpy, with no use of the library's J v or J^T u; frozen columns zeroed."""
    C, P, M = prob.C, prob.P, prob.M
    T = mJ.shape[1]
    A = np.zeros((2 * M + T, prob.n_params))
    coff, xoff, ncoef = prob.ctrl_offsets, prob.spline_x_offsets, prob.n_coef

    def spline_cols(g):
        s = int(np.searchsorted(coff, g, side='right') - 1)
        return [int(xoff[s]) + d * int(ncoef[s]) + (g - int(coff[s])) + q for q in range(4) for d in range(3)]

    for c in range(C):
        a, b = int(prob.det_offsets[c]), int(prob.det_offsets[c + 1])
        cam_cols = [c, C + c, 2 * C + c] + list(range(3 * C + c * P, 3 * C + (c + 1) * P))
        for i in range(a, b):
            g = int(ctrl[i])
            if g < 0:
                continue
            cols = cam_cols + spline_cols(g)
            A[2 * a + (i - a), cols] = J[0, :, i]
            A[2 * a + (b - a) + (i - a), cols] = J[1, :, i]
    for j in range(T):
        for k in range(3):
            g = int(mctrl[k, j])
            if g >= 0:
                A[2 * M + j, spline_cols(g)] += mJ[12 * k:12 * k + 12, j]
    if frozen is not None:
        A[:, np.nonzero(frozen)[0]] = 0.0
    return A


# ---- a run that stops by itself inside the first batch of 8 -----------------------------------------------------------------------------
STOP_SEED = 3
STOP_TOL = dict(atol=1e-6, btol=1e-6, conlim=1e8)      # scipy's (and mvus_solve_opts') defaults


@functools.lru_cache(maxsize=None)
def stopping_case():
    """On `plain`: a right-hand side in the span of five of the eight dominant left singular vectors of J, so the bidiagonalisation ends after
    five steps and the residual test (istop = 1) fires there (the dominant ones: what rounding leaves of the other directions then decays
    from step to step instead of growing like a power iteration).  Returns b, the reference's records (run past the stop), the iteration and istop at which a run
    with STOP_TOL ends, and ``margin``: the smallest factor by which a stopping test's quantity misses its threshold at that iteration and
    at the one before (the premise the tests assert: >= 2)."""
    import lsmr_reference as ref
    hc = host_case('plain')
    rng = np.random.default_rng(STOP_SEED)
    U, s, _ = np.linalg.svd(hc.J, full_matrices=False)
    pick = np.sort(rng.choice(8, 5, replace=False))
    b = U[:, pick] @ rng.uniform(0.5, 1.5, 5)
    recs = ref.lsmr_iterates(hc.A, b, 0.0, 7, np.longdouble, **STOP_TOL)
    stop = next(r for r in recs if r.istop != 0)
    # every test that could decide: (quantity, threshold) -- it fires when quantity <= threshold
    def tests(r):
        return {1: (r.test1, r.rtol), 2: (r.test2, r.atol), 3: (r.test3, r.ctol)}
    margin = np.inf
    if stop.itn > 1:
        for q, t in tests(recs[stop.itn - 2]).values():      # the iteration before: nothing fires, by a factor
            margin = min(margin, float(q / t))
    t = tests(stop)
    margin = min(margin, float(t[stop.istop][1] / t[stop.istop][0]))      # the deciding test fires by a factor ...
    for i in range(1, stop.istop):                                         # ... and none that outranks it is near firing
        margin = min(margin, float(t[i][0] / t[i][1]))
    return SimpleNamespace(b=b, recs=recs, itn=stop.itn, istop=stop.istop, margin=margin, ref=stop)
