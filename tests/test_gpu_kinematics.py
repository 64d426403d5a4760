"""mvus_spline_eval_der / mvus_spline_kin_cov_eval / mvus_spline_length / Scene.kinematics on the GPU.

References and bars are those of tests/test_kinematics_host.py: derivatives against de Boor's recurrence in np.longdouble, relative to
sum_a |B_a^(v)| |c_a|, bar max(8 x scipy's splev(der=v), 1e-12); state covariance against a dense long-double B Sigma B^T, relative to
sqrt(C_ii C_jj), bar max(8 x the fp64 einsum's loss, 1e-12); lengths against scipy.integrate.quad, 1e-12 relative.  Every test prints its
measured worst case beside the bar.

Spline sets: one span (n = 4), n = 5, three splines with gaps between their intervals (n = 4, 9 on knot spacings in ratio 1e3 with an interval
narrower than its knots, 12), and the golden trajectory at its own t_query.  Sample counts 1, 255, 256, 257 (the workgroup is 256 lanes); the
samples sit on interval starts and ends, on interior knots, in a gap, before the first interval and after the last, the rest random.

Measured on an MI355X: derivatives 5.0e-16 against long-double de Boor and 5.4e-16 against the host build (bar 1e-12), state
covariance at most 1.2e-3 of its bar, lengths 3.9e-16 against the host build and 4.7e-16 against quad on the golden trajectory (bar 1e-12)."""
import functools

import numpy as np
import pytest

import test_kinematics_host as kh
from mvus_amd import _lib

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def spline_set(name):
    """(tck, interval[2, S], special samples)"""
    rng = np.random.default_rng(29)
    if name == 'golden':
        splines, interval, tq = kh.golden_splines()
        return [[k, [c[0], c[1], c[2]], 3] for k, c in splines], interval, tq
    if name == 'n4':
        k, c, _ = kh.CASES['single_span']
        return [[k, list(c), 3]], np.array([[0.0], [1.0]]), np.array([0.0, 1.0, 0.5, -0.1, 1.1])
    if name == 'n5':
        k, c, _ = kh.CASES['n5']
        return [[k, list(c), 3]], np.array([[0.0], [1.0]]), np.array([0.0, 1.0, 0.4, -1.0, 2.0])
    assert name == 's3'
    k0, c0, _ = kh.CASES['single_span']
    k1, c1, _ = kh.CASES['ratio_1e3']
    k1 = k1 + 2.0                                                               # knots 2 .. 6.004, interval 2.5 .. 5.5 inside them
    inner = np.sort(rng.uniform(9.0, 20.0, 8))
    k2 = np.concatenate((np.full(4, 9.0), inner, np.full(4, 20.0)))
    c2 = rng.standard_normal((3, 12)) * 5.0
    tck = [[k0, list(c0), 3], [k1, list(c1), 3], [k2, list(c2), 3]]
    interval = np.array([[0.0, 2.5, 9.0], [1.0, 5.5, 20.0]])
    special = np.concatenate((interval[0], interval[1], k1[4:-4][(k1[4:-4] > 2.5) & (k1[4:-4] < 5.5)], inner, [1.7, 8.0, -3.0, 20.5, 2.2, 5.8]))
    return tck, interval, special


def samples(name, nt):
    tck, interval, special = spline_set(name)
    if name == 'golden':
        return special
    rng = np.random.default_rng(1000 + nt)
    lo, hi = interval[0, 0] - 0.5, interval[1, -1] + 0.5
    ts = np.concatenate((special, rng.uniform(lo, hi, max(nt - special.size, 0))))[:nt]
    if nt == 1:
        ts = np.array([interval[1, -1]])                                        # the last knot of the last spline: the left derivative
    return ts


SHAPES = [('n4', 1), ('n4', 255), ('n5', 256), ('n5', 257), ('s3', 1), ('s3', 255), ('s3', 256), ('s3', 257), ('golden', 300)]


@pytest.mark.parametrize('name,nt', SHAPES)
def test_eval_der(name, nt):
    from mvus_amd import spline
    tck, interval, _ = spline_set(name)
    ts = samples(name, nt)
    X, w0 = spline.evaluate(tck, interval, ts)
    D, which = spline.evaluate_der(tck, interval, ts)
    assert D.shape == (3, 3, ts.size) and np.array_equal(which, w0)
    assert np.array_equal(D[0], X)                                             # the bits of mvus_spline_eval
    out = which < 0
    assert not D[:, :, out].any()
    if name != 'golden' and nt > 1:
        assert out.sum() >= 2 and (~out).sum() >= 2
    for nder in (0, 1):                                                         # fewer orders: the leading blocks, bit for bit
        Dn, wn = spline.evaluate_der(tck, interval, ts, nder=nder)
        assert Dn.shape == (nder + 1, 3, ts.size) and np.array_equal(Dn, D[:nder + 1]) and np.array_equal(wn, which)
    for s in range(interval.shape[1]):
        m = which == s
        if not m.any():
            continue
        knots, coefs = tck[s][0], np.array(tck[s][1])
        host = kh.host_eval_der(knots, coefs, ts[m])
        for nu in (1, 2):
            ref, sc, bar = kh.der_bar(knots, coefs, ts[m], nu)
            worst = float(np.max(np.abs(D[nu][:, m].astype(np.longdouble) - ref) / sc))
            vs_host = float(np.max(np.abs(D[nu][:, m] - host[nu]) / sc.astype(np.float64)))
            print('eval_der %s nt=%d spline %d order %d: worst %.3e (against the host build %.3e), bar %.3e' % (name, nt, s, nu, worst, vs_host, bar))
            assert worst <= bar and vs_host <= bar


@pytest.mark.parametrize('nder', [3, -1])
def test_eval_der_refuses_other_orders(nder):
    from mvus_amd import spline
    tck, interval, _ = spline_set('n5')
    with pytest.raises(ValueError, match='nder'):
        spline.evaluate_der(tck, interval, np.array([0.5]), nder=nder)
    lib = _lib.load()
    z, koff, which = np.zeros(12), np.array([0, 8], np.int64), np.zeros(1, np.int32)
    rc = lib.mvus_spline_kin_cov_eval(0, 1, _lib.dptr(z), koff.ctypes.data_as(_lib.c_int64_p), _lib.dptr(z), _lib.dptr(z), 1, _lib.dptr(z), nder, _lib.dptr(z),
                                      which.ctypes.data_as(_lib.c_int32_p))
    assert rc == _lib.MVUS_E_INVALID and b'nder' in lib.mvus_last_error(None)


@functools.lru_cache(maxsize=None)
def sigma_of(name):
    """(dense SPD Sigma over all control points of the set, its band, first control point of each spline)"""
    tck, _, _ = spline_set(name)
    off = np.concatenate(([0], np.cumsum([len(k[0]) - 4 for k in tck])))
    N = int(off[-1])
    Sigma = kh.random_spd_band(3 * N, 11, seed=7 + N)
    return Sigma, kh.band_of(Sigma, N), off


@pytest.mark.parametrize('name,nt', SHAPES)
def test_kin_cov_evaluate(name, nt):
    from mvus_amd import spline
    tck, interval, _ = spline_set(name)
    ts = samples(name, nt)
    Sigma, band, off = sigma_of(name)
    cov, which = spline.kin_cov_evaluate(tck, interval, band, ts)
    pos, w0 = spline.cov_evaluate(tck, interval, band, ts)
    assert cov.shape == (ts.size, 9, 9) and np.array_equal(which, w0) and np.array_equal(which, spline.evaluate(tck, interval, ts)[1])
    out = which < 0
    assert np.isnan(cov[out]).all() and not np.isnan(cov[~out]).any()
    assert np.array_equal(cov, cov.transpose(0, 2, 1), equal_nan=True)         # symmetric to the bit
    N = Sigma.shape[0] // 3
    worst_all, pos_all = 0.0, 0.0
    for i in np.nonzero(~out)[0]:
        s = which[i]
        knots = tck[s][0]
        l = kh.span_of(knots, ts[i])
        h, dh, ddh, _, _ = kh.host_basis(knots, ts[i])
        p = int(off[s]) + l - 3
        ref, bar = kh.state_cov_reference([h, dh, ddh], p, Sigma)
        sd = np.sqrt(np.diag(ref))
        worst = float(np.max(np.abs(cov[i].astype(np.longdouble) - ref) / np.outer(sd, sd)))
        ppos = float(np.max(np.abs(cov[i, :3, :3] - pos[i]) / np.outer(sd[:3], sd[:3]).astype(np.float64)))
        assert worst <= bar and ppos <= bar, (ts[i], worst, ppos, bar)
        assert np.linalg.eigvalsh(cov[i]).min() >= -bar * np.trace(cov[i])
        worst_all, pos_all = max(worst_all, worst / bar), max(pos_all, ppos / bar)
    print('kin_cov %s nt=%d: worst / bar %.4f, position block against cov_evaluate / bar %.4f' % (name, nt, worst_all, pos_all))
    for nder in (0, 1):                                                         # the smaller states: the leading blocks (another kernel instance: to 1e-12)
        D = 3 * (nder + 1)
        cn, wn = spline.kin_cov_evaluate(tck, interval, band, ts, nder=nder)
        assert cn.shape == (ts.size, D, D) and np.array_equal(wn, which) and np.isnan(cn[out]).all()
        sd = np.sqrt(np.einsum('tii->ti', cov[~out]))[:, :D]
        assert np.max(np.abs(cn[~out] - cov[~out][:, :D, :D]) / (sd[:, :, None] * sd[:, None, :]), initial=0.0) <= 1e-12
        assert np.array_equal(cn, cn.transpose(0, 2, 1), equal_nan=True)


def test_kin_cov_evaluate_refuses_a_band_of_another_size():
    from mvus_amd import spline
    tck, interval, _ = spline_set('s3')
    _, band, _ = sigma_of('s3')
    for bad in (band[:-1], band[:, :3], np.concatenate((band, band[:1]))):
        with pytest.raises(ValueError, match='band'):
            spline.kin_cov_evaluate(tck, interval, bad, np.array([0.5]))


@functools.lru_cache(maxsize=None)
def length_reference(name, nt):
    """(dist, total) of the set: scipy's quad on the golden trajectory; on the other sets -- random coefficients, where the speed comes close to
    zero inside a span and the 8-point rule itself is good to 1e-5 only (DESIGN) -- the host build of the same rule"""
    tck, interval, _ = spline_set(name)
    ts = samples(name, nt)
    dist, total = np.zeros(ts.size), np.zeros(interval.shape[1])
    for s in range(interval.shape[1]):
        lo, hi = interval[0, s], interval[1, s]
        m = (ts >= lo) & (ts <= hi)
        fn = kh.quad_dist if name == 'golden' else kh.host_path_length
        dist[m], total[s] = fn(tck[s][0], np.array(tck[s][1]), lo, hi, ts[m])
    return dist, total


@pytest.mark.parametrize('name,nt', SHAPES)
def test_path_length(name, nt):
    from mvus_amd import spline
    tck, interval, _ = spline_set(name)
    ts = samples(name, nt)
    dist, which, total = spline.path_length(tck, interval, ts)
    assert np.array_equal(which, spline.evaluate(tck, interval, ts)[1]) and total.shape == (interval.shape[1],)
    again = spline.path_length(tck, interval, ts)
    assert all(np.array_equal(a, b) for a, b in zip((dist, which, total), again))                  # the same bits on every run
    assert not dist[which < 0].any() and (dist >= 0).all()
    want, want_total = length_reference(name, nt)
    worst = max(kh.rel_len_err(dist, want), float(np.max(np.abs(total - want_total) / want_total)))
    print('path_length %s nt=%d against %s: totals %s, worst relative error %.3e (bar 1e-12)' % (name, nt, 'quad' if name == 'golden' else 'the host build', total, worst))
    assert worst <= 1e-12
    # interval starts are exactly 0, the ends carry the total to the bit, and the distance never falls inside an interval
    ends = np.concatenate((interval[0], interval[1]))
    d2, w2, t2 = spline.path_length(tck, interval, ends)
    S = interval.shape[1]
    assert np.array_equal(w2, np.concatenate((np.arange(S), np.arange(S)))) and np.array_equal(t2, total)
    assert not d2[:S].any() and np.array_equal(d2[S:], total)
    for s in range(S):
        m = which == s
        order = np.argsort(ts[m], kind='stable')
        assert (np.diff(dist[m][order]) >= 0).all()


def test_path_length_of_a_straight_line():
    from mvus_amd import spline
    knots = np.concatenate((np.full(4, 2.0), [2.5, 4.0, 4.25, 7.0], np.full(4, 9.0)))
    grev = np.array([knots[j + 1:j + 4].sum() / 3.0 for j in range(knots.size - 4)])
    P0, V = np.array([1.0, -2.0, 30.0]), np.array([0.3, 0.4, 1.2])
    coefs = P0[:, None] + V[:, None] * grev[None, :]
    xs = np.array([2.0, 3.1, 4.0, 6.5, 9.0])
    dist, which, total = spline.path_length([[knots, list(coefs), 3]], np.array([[2.0], [9.0]]), xs)
    want = 1.3 * (xs - 2.0)
    assert dist[0] == 0.0 and total[0] == dist[-1]
    assert (np.abs(dist - want) <= 8 * np.spacing(want)).all(), (dist, want)


# ---- Scene ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scene_after_ba():
    """rs_F_2int_3cam (two intervals) after an LM bundle adjustment with the anchor gauge, its trajectory resampled, and its covariance"""
    from golden_util import load_case
    from frozen_util import ba_kwargs, build_scene
    scene, _ = load_case('rs_F_2int_3cam')
    s = build_scene(scene, ba_solver='lm', ba_gauge='anchor')
    res = s.BA(s.numCam, max_iter=10, **ba_kwargs(s.settings))
    assert res.solver_used == 'lm'
    s.spline_to_traj()
    cams = list(s.sequence[:s.numCam])
    cv = s.ba_covariance(cams, **ba_kwargs(s.settings))
    return s, cv


KEYS = {'t', 'which', 'fps', 'pos', 'vel', 'acc', 'speed', 'dist', 'length'}
COV_KEYS = {'state_cov', 'vel_std', 'acc_std', 'speed_std'}


def test_scene_kinematics():
    from mvus_amd import spline
    from mvus_amd.reconstruction.common import Scene
    s, cv = scene_after_ba()
    S = s.spline['int'].shape[1]
    assert S == 2
    fps = float(s.cameras[s.ref_cam].fps)
    vars(s).pop('kinematics', None)
    kin = s.kinematics(cov=cv)
    assert vars(s)['kinematics'] is kin and set(kin) == KEYS | COV_KEYS and kin['fps'] == fps
    nt = s.traj.shape[1]
    assert np.array_equal(kin['t'], s.traj[0]) and (kin['which'] >= 0).all()
    for key, shape in dict(pos=(3, nt), vel=(3, nt), acc=(3, nt), speed=(nt,), dist=(nt,), length=(S,), which=(nt,), state_cov=(nt, 9, 9), vel_std=(nt, 3),
                           acc_std=(nt, 3), speed_std=(nt,)).items():
        assert kin[key].shape == shape, key
    assert np.array_equal(kin['pos'], s.traj[1:])
    for key in ('vel_std', 'acc_std', 'speed_std'):
        assert np.isfinite(kin[key]).all() and (kin[key] > 0).all(), key
    assert np.array_equal(kin['speed'], np.sqrt(np.sum(kin['vel'] ** 2, axis=0)))
    u = kin['vel'] / kin['speed']
    want = np.sqrt(np.einsum('it,tij,jt->t', u, kin['state_cov'][:, 3:6, 3:6], u))
    assert np.allclose(kin['speed_std'], want, rtol=1e-13, atol=0)
    assert np.array_equal(kin['vel_std'], np.sqrt(np.einsum('tii->ti', kin['state_cov'])[:, 3:6]))
    raw, _ = spline.kin_cov_evaluate(s.spline['tck'], s.spline['int'], cv['band'], s.traj[0])
    assert np.array_equal(kin['state_cov'][:, :3, :3], raw[:, :3, :3])                    # positions carry no unit
    # the distance runs on over the intervals: an interval starts where the one before it ended
    first = kin['which'] == 0
    assert np.array_equal(kin['length'], spline.path_length(s.spline['tck'], s.spline['int'], s.traj[0])[2])
    assert kin['dist'][first].max() <= kin['length'][0] <= kin['dist'][~first].min() and kin['dist'][~first].max() <= kin['length'].sum()
    assert (np.diff(kin['dist']) >= 0).all()
    # fps: per-frame units with fps = 1, the stored dict replaced by the latest call; without cov the 1-sigma keys are absent
    per_frame = Scene.kinematics(s, fps=1, cov=cv['band'])
    assert vars(s)['kinematics'] is per_frame and per_frame['fps'] == 1.0
    assert np.array_equal(kin['vel'], fps * per_frame['vel']) and np.array_equal(kin['acc'], fps ** 2 * per_frame['acc'])
    assert np.array_equal(kin['pos'], per_frame['pos']) and np.array_equal(kin['dist'], per_frame['dist'])
    unit = np.repeat([1.0, fps, fps ** 2], 3)
    assert np.array_equal(kin['state_cov'], per_frame['state_cov'] * np.outer(unit, unit))
    assert np.allclose(kin['vel_std'], fps * per_frame['vel_std'], rtol=1e-15) and np.allclose(kin['acc_std'], fps ** 2 * per_frame['acc_std'], rtol=1e-15)
    assert np.allclose(kin['speed_std'], fps * per_frame['speed_std'], rtol=1e-13)
    D, _ = spline.evaluate_der(s.spline['tck'], s.spline['int'], s.traj[0])
    assert np.array_equal(per_frame['vel'], D[1]) and np.array_equal(per_frame['acc'], D[2])
    ts = np.array([s.spline['int'][0, 0] - 3.0, s.spline['int'][0, 0], s.spline['int'][1, -1]])
    bare = Scene.kinematics(s, t=ts)
    assert set(bare) == KEYS and bare['which'][0] == -1 and not bare['vel'][:, 0].any() and bare['dist'][0] == 0.0 and bare['dist'][1] == 0.0
    assert bare['dist'][2] == kin['length'][0] + kin['length'][1]
    import pickle
    back = pickle.loads(pickle.dumps(s))
    assert set(back.kinematics) == KEYS
    # a band of another trajectory
    with pytest.raises(ValueError, match='band'):
        Scene.kinematics(s, cov=cv['band'][:-1])
    stale = dict(cv, band=np.concatenate((cv['band'], cv['band'][:2])))
    with pytest.raises(ValueError, match='band'):
        Scene.kinematics(s, cov=stale)


@pytest.mark.parametrize('enabled', [True, False])
def test_reconstruct_from_config_carries_the_kinematics(tmp_path, enabled):
    import json
    import pickle
    from mvus_amd import pipeline, synth
    from test_gpu_init_pipeline import _write_inputs
    sc = synth.make_scene(3, 4500, seed=31, perturb=0.3, motion_reg=True, motion_type='F', motion_weights=1e2)      # (the scene of the covariance test of this name)
    cf = -sc.truth['beta'] / sc.truth['alpha']
    path = _write_inputs(tmp_path, sc, cf, True)
    cfg = json.loads(path.read_text())
    cfg['settings'].update(ba_solver='lm', ba_gauge='anchor')
    if enabled:
        cfg['settings'].update(ba_covariance=True, ba_kinematics=True)
    path.write_text(json.dumps(cfg))
    flight, timer = pipeline.reconstruct_from_config(str(path))
    with open(flight.settings['path_output'], 'rb') as fh:
        back = pickle.load(fh)
    stages = [r[0] for r in timer.rows]
    if not enabled:
        assert 'kinematics' not in vars(back) and 'kinematics' not in stages
        return
    assert stages.index('kinematics') > stages.index('ba_covariance')
    kin = vars(back)['kinematics']
    nt = flight.traj.shape[1]
    assert set(kin) == KEYS | COV_KEYS and np.array_equal(kin['t'], flight.traj[0]) and np.array_equal(kin['pos'], flight.traj[1:])
    assert kin['fps'] == flight.cameras[flight.ref_cam].fps and kin['state_cov'].shape == (nt, 9, 9)
    assert np.isfinite(kin['speed_std']).all() and (kin['speed_std'] > 0).all() and (kin['speed'] > 0).all()
    assert np.isfinite(kin['vel_std']).all() and (kin['vel_std'] > 0).all() and (np.diff(kin['dist']) >= 0).all()
