"""Starting a reconstruction on the GPU: Scene.init_traj (reference common.py:178-221), Scene.time_shift with the brute-force
synchronisation search (common.py:1004-1040, synchronization.sync_bf) and the whole of main.py from files on disk
(pipeline.reconstruct_from_config).  Before these existed every one of them raised NotImplementedError.

The accuracy bars of init_traj are set from the numpy restatement (tests/epipolar_oracle.py) run on the same data on the CPU --
the oracle clears each of them by at least 2x there -- not from GPU runs."""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import epipolar_oracle as eo                               # noqa: E402

# init_traj on init_scene(): the oracle measured 6.2 deg / 0.82 deg / 1.19 m (points on one trajectory constrain F weakly; BA refines)
ROT_BAR_DEG, DIR_BAR_DEG, TRAJ_RMS_BAR_M = 15.0, 2.0, 3.0


def init_scene(num_cam=3, total_obs=9000, seed=31, **kw):
    """A Scene straight after detection_to_global with exact time shifts and no poses, and the generator's SynthScene."""
    from mvus_amd import synth
    from mvus_amd.reconstruction import common
    sc = synth.make_scene(num_cam, total_obs, seed=seed, **kw)
    s = common.Scene()
    s.numCam = num_cam
    s.settings = dict(sc.settings)
    for c in sc.truth['cameras']:
        s.addCamera(common.Camera(K=c['K'].copy(), d=c['d'].copy(), fps=c['fps'], resolution=list(c['resolution'])))
    for det in sc.detections:
        s.addDetection(det.copy())
    s.alpha, s.beta, s.rs = sc.truth['alpha'].copy(), sc.truth['beta'].copy(), sc.truth['rs'].copy()
    s.find_order, s.ref_cam = True, 0
    s.detection_to_global()
    return s, sc


def _true_curve(sc, tau):
    from mvus_amd import bspline
    X = np.full((3, tau.size), np.nan)
    for tck in sc.truth['tck']:
        m = (tau >= tck[0][0]) & (tau < tck[0][-1])
        if m.any():
            X[:, m] = bspline.evaluate(tck[0], np.array(tck[1]), tau[m])
    return X


def _angle_deg(R):
    return float(np.degrees(np.arccos(np.clip(0.5 * (np.trace(R) - 1.0), -1.0, 1.0))))


def pose_errors(sc, t1, t2, R_rel, t_rel, traj):
    """(relative rotation error deg, translation direction error deg, trajectory rms after the best similarity, m)."""
    from mvus_amd.analysis.compare_gt import similarity_from_points
    c1, c2 = sc.truth['cameras'][t1], sc.truth['cameras'][t2]
    R_true = c2['R'] @ c1['R'].T
    t_true = c2['t'] - R_true @ c1['t']
    rot = _angle_deg(R_true.T @ R_rel)
    cosd = np.dot(t_true, t_rel) / np.linalg.norm(t_true) / np.linalg.norm(t_rel)
    direction = float(np.degrees(np.arccos(np.clip(cosd, -1.0, 1.0))))
    Xt = _true_curve(sc, traj[0])
    ok = np.isfinite(Xt[0])
    M = similarity_from_points(traj[1:, ok], Xt[:, ok])
    d = np.sqrt(((Xt[:, ok] - (M[:3, :3] @ traj[1:, ok] + M[:3, 3:4])) ** 2).sum(axis=0))
    return rot, direction, float(np.sqrt(np.mean(d ** 2)))


def oracle_init(s, sc, error=10):
    """init_traj's steps with the numpy restatement: (t1, t2, R, t, traj)."""
    from mvus_amd.tools import util
    n = s.numCam
    best, pair = 0, None
    for i in range(n - 1):
        for j in range(i + 1, n):
            x, _ = util.match_overlap(s.detections_global[i], s.detections_global[j])
            if x.shape[1] / s.cameras[i].fps > best:
                best, pair = x.shape[1] / s.cameras[i].fps, (i, j)
    t1, t2 = pair
    if s.cameras[t1].fps > s.cameras[t2].fps:
        d1, d2 = util.match_overlap(s.detections_global[t1], s.detections_global[t2])
    else:
        d2, d1 = util.match_overlap(s.detections_global[t2], s.detections_global[t1])
    F, _, _ = eo.fundamental_ransac(d1[1:], d2[1:], error)
    K1, K2 = s.cameras[t1].K, s.cameras[t2].K
    E = K2.T @ F @ K1
    m1, m2 = eo.correct_matches(F, d1[1:], d2[1:])
    keep = np.isfinite(m1[0])
    x1n = (np.linalg.inv(K1) @ np.vstack((m1[:, keep], np.ones(keep.sum()))))[:2]
    x2n = (np.linalg.inv(K2) @ np.vstack((m2[:, keep], np.ones(keep.sum()))))[:2]
    X, P2 = eo.pose_from_essential(E, x1n, x2n)
    return t1, t2, P2[:, :3], P2[:, 3], np.vstack((d1[0][keep], X[:3]))


def test_oracle_clears_the_init_bars():
    """CPU: where the bars of test_init_traj come from."""
    s, sc = init_scene()
    t1, t2, R, t, traj = oracle_init(s, sc)
    rot, direction, rms = pose_errors(sc, t1, t2, R, t, traj)
    print('oracle: rot %.4f deg, direction %.4f deg, traj rms %.4f m' % (rot, direction, rms))
    assert rot <= ROT_BAR_DEG / 2 and direction <= DIR_BAR_DEG / 2 and rms <= TRAJ_RMS_BAR_M / 2


@pytest.mark.gpu
def test_init_traj():
    from mvus_amd.tools import util
    s, sc = init_scene()
    s.init_traj(error=10)
    t1, t2 = s.sequence
    # the pair with the most overlap (select_most_overlap(init=True))
    best, pair = 0, None
    for i in range(s.numCam - 1):
        for j in range(i + 1, s.numCam):
            x, _ = util.match_overlap(s.detections_global[i], s.detections_global[j])
            if x.shape[1] / s.cameras[i].fps > best:
                best, pair = x.shape[1] / s.cameras[i].fps, [i, j]
    assert [t1, t2] == pair
    K1 = s.cameras[t1].K
    np.testing.assert_allclose(s.cameras[t1].P, K1 @ np.hstack((np.eye(3), np.zeros((3, 1)))), rtol=0, atol=1e-9)
    if s.cameras[t1].fps > s.cameras[t2].fps:
        d1, _ = util.match_overlap(s.detections_global[t1], s.detections_global[t2])
    else:
        _, d1 = util.match_overlap(s.detections_global[t2], s.detections_global[t1])
    assert s.traj.shape[0] == 4 and s.traj.shape[1] == d1.shape[1]          # inlier_only=False keeps every pair; none is NaN
    np.testing.assert_array_equal(s.traj[0], d1[0])
    R_rel = s.cameras[t2].R @ s.cameras[t1].R.T
    t_rel = s.cameras[t2].t - R_rel @ s.cameras[t1].t
    rot, direction, rms = pose_errors(sc, t1, t2, R_rel, t_rel, s.traj)
    print('gpu: rot %.4f deg, direction %.4f deg, traj rms %.4f m' % (rot, direction, rms))
    assert rot < ROT_BAR_DEG and direction < DIR_BAR_DEG and rms < TRAJ_RMS_BAR_M


def _perturbed_cf(sc, rng):
    """Corresponding frames that the truth would make exact (cf[0] = 0), camera j's moved by 2-7 s."""
    tr = sc.truth
    cf = -tr['beta'] / tr['alpha']
    for j in range(1, len(cf)):
        cf[j] += rng.choice([-1, 1]) * rng.uniform(2.0, 7.0) * sc.cameras[j]['fps']
    return cf


@pytest.mark.gpu
def test_time_shift_brute_force(monkeypatch):
    from mvus_amd.reconstruction import epipolar as ep
    s, sc = init_scene(num_cam=4, total_obs=12000, seed=32)
    s.cf = _perturbed_cf(sc, np.random.default_rng(5))
    s.settings.update(cf_exact=False, sync_method='bf')
    s.init_alpha()
    calls = []
    real = ep.fundamental_ransac_batch

    def counting(pairs, *a, **k):
        pairs = list(pairs)
        calls.append(len(pairs))
        return real(pairs, *a, **k)
    monkeypatch.setattr(ep, 'fundamental_ransac_batch', counting)
    s.time_shift()
    assert len(calls) == 2 * (s.numCam - 1)                   # one batched call per stage and camera
    assert all(n >= 15 for n in calls)                          # ~20 candidates each
    tr = sc.truth
    # The search's resolution is the fine grid step (fps2 / 20 frames, times alpha); on this scene the inlier count peaks within
    # 0.7 - 2.1 frames of the truth against a 1.5-frame step, so the bar is two steps: far below the 2 - 7 s
    # the corresponding frames were moved by
    for j in range(s.numCam):
        step = sc.cameras[j]['fps'] / 20 * tr['alpha'][j]
        print('camera', j, 'beta', s.beta[j], 'truth', tr['beta'][j], 'step', step)
        assert abs(s.beta[j] - tr['beta'][j]) <= 2 * step + 1e-9
    np.testing.assert_array_equal(s.beta_after_Fbeta, s.beta)
    s.settings['sync_method'] = 'iter'
    with pytest.raises(NotImplementedError, match='sync_iter'):
        s.time_shift()


def _write_inputs(tmp_path, sc, cf, cf_exact):
    dets, cams = [], []
    for i in range(sc.num_cam):
        d = sc.detections[i]
        p = tmp_path / ('cam%d.txt' % i)
        np.savetxt(p, np.column_stack((d[1], d[2], d[0])), fmt='%.18e')
        dets.append(str(p))
        c = sc.cameras[i]
        q = tmp_path / ('cam%d.json' % i)
        q.write_text(json.dumps({'comment': 'synthetic', 'K-matrix': c['K'].tolist(), 'distCoeff': c['d'].tolist()[:4],
                                 'fps': c['fps'], 'resolution': [int(c['resolution'][0]), int(c['resolution'][1])]}))
        cams.append(str(q))
    st = sc.settings
    cfg = {'comments': 'tests/test_gpu_init_pipeline.py',
           'necessary inputs': {'path_detections': dets, 'path_cameras': cams, 'corresponding_frames': [float(v) for v in cf]},
           'optional inputs': {},
           'settings': {'num_detections': 1000000, 'opt_calib': False, 'cf_exact': cf_exact, 'sync_method': 'bf', 'undist_points': True,
                        'rolling_shutter': st['rolling_shutter'], 'init_rs': 0.5, 'rs_bounds': False, 'motion_prior': False,
                        'motion_reg': st['motion_reg'], 'motion_weights': st['motion_weights'], 'motion_type': st['motion_type'],
                        'cut_detection_second': 0, 'camera_sequence': [], 'ref_cam': 0, 'thres_Fmatix': 10, 'thres_PnP': 8,
                        'thres_outlier': 10, 'thres_triangulation': 20, 'smooth_factor': [10, 20], 'sampling_rate': 0.02,
                        'path_output': str(tmp_path / ('flight_%s.pkl' % cf_exact))}}
    path = tmp_path / ('config_%s.json' % cf_exact)
    path.write_text(json.dumps(cfg))
    return path


@pytest.mark.gpu
def test_reconstruct_from_config(tmp_path):
    """main.py end to end from files -- detections, calibrations and a config, no pose and no trajectory -- with exact
    corresponding frames.  Bars of test_gpu_pipeline.py::test_incremental_loop_seven_cameras where this run meets them (mean
    reprojection error, camera centres and orientations, gross outliers kept); that test starts from perturbed TRUE poses, this
    one from an initialisation by E (6 deg off on this scene, see test_init_traj): measured trajectory rms 1.53 m and 92.5 % of
    the clean detections kept, so those two bars are 2.0 m and 90 % here.  The scale of the gauge is free."""
    import pickle
    from mvus_amd import pipeline, synth
    kw = dict(synth.BASELINE_CONFIGS[1])
    kw.pop('seed'); kw.pop('num_cam'); kw.pop('total_obs'); kw.pop('num_intervals', None)
    kw['motion_weights'] = 1e2
    sc = synth.make_scene(7, 60_000, seed=2, perturb=0.3, **kw)
    cf = -sc.truth['beta'] / sc.truth['alpha']
    path = _write_inputs(tmp_path, sc, cf, True)
    flight, timer = pipeline.reconstruct_from_config(str(path))
    stages = [r[0] for r in timer.rows]
    for name in ('create_scene', 'time_shift', 'init_traj', 'traj_to_spline', 'BA', 'get_camera_pose', 'spline_to_traj'):
        assert name in stages
    assert sorted(flight.sequence) == list(range(7)) and all(c.P is not None for c in flight.cameras)
    ev = pipeline.evaluate_against_truth(flight, sc)
    print('mean err', np.round(ev['mean_err'], 3), 'traj rms %.3f' % ev['traj_rms'], 'centres', np.round(ev['centre_err'], 3),
          'rot', np.round(ev['rot_err_deg'], 3), 'kept/clean/dirty', list(zip(ev['kept'], ev['clean'], ev['kept_dirty'])),
          'seconds', {k: round(v, 2) for k, v in timer.totals().items()})
    assert max(ev['mean_err']) < 1.3
    for kept, clean, dirty in zip(ev['kept'], ev['clean'], ev['kept_dirty']):
        assert kept >= 0.90 * clean
        assert dirty <= 0.02 * kept + 5
    assert ev['traj_rms'] < 2.0 and max(ev['centre_err']) < 2.5 and max(ev['rot_err_deg']) < 2.5
    with open(flight.settings['path_output'], 'rb') as fh:
        back = pickle.load(fh)
    np.testing.assert_array_equal(back.cameras[3].P, flight.cameras[3].P)
