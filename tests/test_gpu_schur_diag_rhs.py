"""k_schur_gemm carries the right-hand-side column inside its diagonal tiles (three accumulators above the diagonal of a 48x48 tile on the
block diagonal, ba_gemm_plan.h): the damped step against a dense solve of the exported normal equations, by the method and the bar of
test_gpu_schur.py::test_schur_product_slab_plans, at the shapes where such a tile can go wrong."""
import numpy as np
import pytest

from mvus_amd import _lib
from mvus_amd import problem as mp

pytestmark = pytest.mark.gpu

LAM = 0.05
# name -> (cameras, detections asked for, scene keywords, CB): every scene on <= 10 k detections, 3N no multiple of 16
SHAPES = {
    # one ragged diagonal tile and nothing else; 28 control points: ONE interior, no separator range, six row sets in all
    'cb18': (2, 1500, dict(seed=71, num_knots=25), 18),
    # the same with the calibration free (B = 18): still one tile, its second 16-row piece partly live, its third dead
    'cb36_calib': (2, 2500, dict(seed=72, num_knots=90, distortion=True, opt_calib=True), 36),
    # CB a multiple of 48: three full diagonal tiles
    'cb144': (16, 7000, dict(seed=73, num_knots=120), 144),
    # ragged at the 48 and at the 16 level: the last diagonal tile has 9 live columns, its rhs rows are partly clamped;
    # 174 control points: several interiors, so the rhs fragment is also taken from the separators' compact array (Xs)
    'cb153_sep': (17, 7000, dict(seed=74, num_knots=171), 153),
}
_cache = {}


def internal_index(prob):
    """x index of every unknown in the solver's internal order: camera blocks (alpha,beta,rs,params), then 3*ctrl+xyz."""
    C, P = prob.C, prob.P
    cam = [[c, C + c, 2 * C + c] + list(range(3 * C + c * P, 3 * C + (c + 1) * P)) for c in range(C)]
    spl = []
    for s, n in enumerate(prob.n_coef):
        for j in range(int(n)):
            spl += [int(prob.spline_x_offsets[s]) + d * int(n) + j for d in range(3)]
    return np.array(cam), np.array(spl)


def dense_step(prob, g, A, band, cross, lam):
    """-(H + lam diag(H))^-1 g of the exported blocks, by numpy.linalg.solve"""
    cam_idx, spl_idx = internal_index(prob)
    N = int(prob.n_coef.sum())
    n, C, B, W = prob.n_params, prob.C, 3 + prob.P, band.shape[1]
    H = np.zeros((n, n))
    for c in range(C):
        H[np.ix_(cam_idx[c], cam_idx[c])] = A[c]
    E = cross.reshape(C * B, 3 * N)
    H[np.ix_(cam_idx.ravel(), spl_idx)] = E
    H[np.ix_(spl_idx, cam_idx.ravel())] = E.T
    for w in range(W):
        for gi in range(N - w):
            ri, cj = spl_idx[3 * gi:3 * gi + 3], spl_idx[3 * (gi + w):3 * (gi + w) + 3]
            H[np.ix_(ri, cj)] = band[gi, w]
            H[np.ix_(cj, ri)] = band[gi, w].T
    d = np.diag(H).copy()
    return np.linalg.solve(H + lam * np.diag(np.where(d > 0, d, 1.0)), -g)


def shape(name):
    """(prob, x0, p_ref) of a shape: the scene and its dense reference are made once (the exported blocks do not depend on the route)"""
    if name not in _cache:
        from mvus_amd import synth
        from mvus_amd.ba import BAHandle
        cams, obs, kw, CB = SHAPES[name]
        sc = synth.make_scene(cams, obs, rolling_shutter=True, **kw)
        prob, x0 = mp.problem_from_scene(sc)
        assert prob.C * (3 + prob.P) == CB and prob.M <= 10000
        assert (3 * int(prob.n_coef.sum())) % 16 != 0
        with BAHandle(prob) as h:
            h.residual_jacobian(x0, _lib.JAC_ANALYTIC)
            g, A, band, cross = h.normal_equations()
        p_ref = dense_step(prob, g, A, band, cross, LAM)
        p_ref.setflags(write=False)
        _cache[name] = (prob, x0, p_ref)
    return _cache[name]


@pytest.mark.parametrize('route', ['ldlt', 'gj'])
@pytest.mark.parametrize('slabs', [None, 1, 3, 11, 24])
@pytest.mark.parametrize('name', list(SHAPES))
def test_step_with_rhs_in_the_diagonal_tiles(name, slabs, route, monkeypatch):
    """Planned and forced slab counts (one; fewer than the XCDs; no multiple of eight; 24 -- at cb18 more wavefronts than row sets), both
    routes of the reduced camera system (the Gauss-Jordan route reads both triangles, mirrored at 16-column granularity): relative
    max error of the step against the dense solve below 1e-8."""
    from mvus_amd.ba import BAHandle
    if slabs is None:
        monkeypatch.delenv('MVUS_GEMM_SLABS', raising=False)
    else:
        monkeypatch.setenv('MVUS_GEMM_SLABS', str(slabs))
    if route == 'gj':
        monkeypatch.setenv('MVUS_RCS', 'gj')
    else:
        monkeypatch.delenv('MVUS_RCS', raising=False)
    prob, x0, p_ref = shape(name)
    with BAHandle(prob) as h:
        h.residual_jacobian(x0, _lib.JAC_ANALYTIC)
        p = h.lm_step(LAM)
    err = float(np.abs(p - p_ref).max() / np.abs(p_ref).max())
    print('%s slabs %s route %s: relative max error %.3g' % (name, slabs, route, err))
    assert err < 1e-8


def test_step_on_two_time_shards(monkeypatch):
    """Two time shards on one device (host threads and an in-process sum, as in test_gpu_dist.py): each rank's diagonal tiles carry its part
    of the rhs column, k_sum_slabs adds the slabs and the ranks' sums meet in the reduced system; the step of both ranks against the
    dense solve of the unsharded equations, same bar."""
    import threading
    import torch
    from mvus_amd.ba import BAHandle
    from mvus_amd.dist import _DeviceDoubles
    monkeypatch.delenv('MVUS_GEMM_SLABS', raising=False)
    monkeypatch.delenv('MVUS_RCS', raising=False)
    prob, x0, p_ref = shape('cb153_sep')
    world = 2
    barrier = threading.Barrier(world)
    bufs, total, steps, errors = [None] * world, [None], [None] * world, []

    def make_cb(rank):
        def cb(ptr, count, stream):
            t = torch.as_tensor(_DeviceDoubles(ptr, count), device='cuda:0')
            torch.cuda.synchronize()
            bufs[rank] = t
            barrier.wait(60)
            if rank == 0:
                # (entries of the partial sums that no tile writes and nothing reads may hold anything: they are summed like the others)
                total[0] = bufs[0] + bufs[1]
                torch.cuda.synchronize()
            barrier.wait(60)
            t.copy_(total[0])
            torch.cuda.synchronize()
            barrier.wait(60)
        return cb

    def run(rank):
        try:
            shard, keep, cuts = prob.shard_time(rank, world, x0)
            h = BAHandle(shard, device=0)
            h.set_time_shard(rank, world, cuts)
            h.set_allreduce(make_cb(rank), is_root=(rank == 0))
            h.residual_jacobian(x0, _lib.JAC_ANALYTIC)
            steps[rank] = h.lm_step(LAM)
            h.close()
        except Exception as e:                      # pragma: no cover
            errors.append(e)
            barrier.abort()

    threads = [threading.Thread(target=run, args=(r,), daemon=True) for r in range(world)]      # daemon: a failure must not hang the exit
    [t.start() for t in threads]
    [t.join(120) for t in threads]
    assert not errors, errors
    for p in steps:
        err = float(np.abs(p - p_ref).max() / np.abs(p_ref).max())
        print('time shards: relative max error %.3g' % err)
        assert err < 1e-8
