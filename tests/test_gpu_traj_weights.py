"""settings['traj_weights'] = 'triangulation' on the Scene: init_traj and triangulate keep the 1-sigma of every triangulated point in
Scene.traj_sigma (reconstruction.epipolar.triangulate_with_cov), traj_to_spline turns it into splprep's w, spline_to_traj clears it; without
the setting every method does what it did.  Small synthetic scenes of three cameras, a few hundred detections each."""
import pickle

import numpy as np
import pytest

ON = {'traj_weights': 'triangulation', 'traj_sigma_px': [0.5, 0.7, 0.9], 'traj_weight_floor': 1e-3}


def _init_scene(settings, total_obs=1500, seed=31):
    """a Scene straight after detection_to_global with exact time shifts and no poses (as tests/test_gpu_init_pipeline.py builds it)"""
    from mvus_amd import synth
    from mvus_amd.reconstruction import common
    sc = synth.make_scene(3, total_obs, seed=seed)
    s = common.Scene()
    s.numCam = 3
    s.settings = dict(sc.settings)
    s.settings.update(settings)
    for c in sc.truth['cameras']:
        s.addCamera(common.Camera(K=c['K'].copy(), d=c['d'].copy(), fps=c['fps'], resolution=list(c['resolution'])))
    for det in sc.detections:
        s.addDetection(det.copy())
    s.alpha, s.beta, s.rs = sc.truth['alpha'].copy(), sc.truth['beta'].copy(), sc.truth['rs'].copy()
    s.find_order, s.ref_cam = True, 0
    s.detection_to_global()
    return s


def _staged_scene(settings):
    """cameras 0 and 1 with poses and a spline over the FIRST HALF of their common time range, camera 2 with the generator's pose: its
    detections outside the spline pair with both other cameras at the same timestamps"""
    from mvus_amd import pipeline
    s, sc = pipeline.staged_scene(num_cam=3, total_obs=1500, seed=2, windows=[(0.0, 1.0), (0.0, 1.0), (0.0, 1.0)], settings=settings)
    lo, hi = s.traj[0, 0], s.traj[0, -1]
    s.traj = s.traj[:, s.traj[0] <= 0.5 * (lo + hi)]
    s.traj_to_spline(smooth_factor=s.settings['smooth_factor'])
    cam, c = s.cameras[2], sc.cameras[2]
    cam.R, cam.t = c['R'].copy(), c['t'].copy()
    cam.compose()
    return s


def _same_tck(a, b):
    return len(a) == len(b) and all(np.array_equal(x[0], y[0]) and np.array_equal(np.asarray(x[1]), np.asarray(y[1])) for x, y in zip(a, b))


@pytest.mark.gpu
def test_gpu_traj_weights_init_traj_and_the_fit():
    from mvus_amd import spline
    from mvus_amd.reconstruction import common
    from mvus_amd.tools import util
    s = _init_scene(ON)
    s.init_traj(error=10)
    assert s.traj_sigma is not None and s.traj_sigma.shape == (s.traj.shape[1],)
    fin = np.isfinite(s.traj_sigma)
    assert fin.sum() > 0.9 * fin.size and np.all(s.traj_sigma[fin] > 0)
    print('\ninit_traj: %d samples, sigma %.3g .. %.3g (median %.3g), %d NaN' % (fin.size, s.traj_sigma[fin].min(), s.traj_sigma[fin].max(), np.median(s.traj_sigma[fin]), (~fin).sum()))
    # the same points as without the setting
    s0 = _init_scene({})
    s0.init_traj(error=10)
    assert np.array_equal(s0.traj, s.traj) and s0.traj_sigma is None
    # traj_to_spline = traj_fit with w = max(sigma_min / sigma, floor) of the interval, by hand
    order = np.argsort(s.traj[0], kind='stable')              # (init_traj's samples come in the order of the matches)
    s.traj, s.traj_sigma = s.traj[:, order], s.traj_sigma[order]
    keep = np.concatenate(([True], np.diff(s.traj[0]) > 0))
    s.traj, s.traj_sigma = s.traj[:, keep], s.traj_sigma[keep]
    sf = s.settings['smooth_factor']
    sp = s.traj_to_spline(smooth_factor=sf)
    interval, idx = util.find_intervals(s.traj[0], idx=True)
    by_hand = []
    for i in range(interval.shape[1]):
        sig = s.traj_sigma[idx[0, i]:idx[1, i] + 1]
        ok = np.isfinite(sig) & (sig > 0)
        w = np.full(sig.size, 1e-3)
        w[ok] = np.maximum(sig[ok].min() / sig[ok], 1e-3)
        assert np.array_equal(w, common.Scene.weights_from_sigma(sig, 1e-3)) and w.max() == 1.0
        by_hand.append(spline.traj_fit(s.traj[:, idx[0, i]:idx[1, i] + 1], sf, w=w))
    assert _same_tck(sp['tck'], by_hand)
    unweighted = [spline.traj_fit(s.traj[:, idx[0, i]:idx[1, i] + 1], sf) for i in range(interval.shape[1])]
    assert not _same_tck(sp['tck'], unweighted)
    # the pickle carries traj_sigma while it is set; a rebuild of traj from the spline clears it
    assert 'traj_sigma' in s.__getstate__() and np.array_equal(pickle.loads(pickle.dumps(s)).traj_sigma, s.traj_sigma, equal_nan=True)
    s.spline_to_traj(sampling_rate=1)
    assert s.traj_sigma is None and 'traj_sigma' not in s.__getstate__()
    assert pickle.loads(pickle.dumps(s)).traj_sigma is None


@pytest.mark.gpu
def test_gpu_traj_weights_triangulate_keeps_the_smaller_sigma():
    from mvus_amd.reconstruction import common, epipolar as ep
    from mvus_amd.tools import util
    s = _staged_scene(ON)
    covered = s.spline['int'].copy()
    thres, sf, rate = s.settings['thres_triangulation'], s.settings['smooth_factor'], s.settings['sampling_rate']
    # every candidate by hand: camera 2's detections outside the spline against cameras 0 and 1
    s.detection_to_global(2)
    mine = s.detections_global[2]
    mine = mine[:, ~np.asarray(util.sampling(mine, covered)[1], dtype=bool)]
    per_cam = {}
    for other in (0, 1):
        s.detection_to_global(other)
        a, b = util.match_overlap(mine, s.detections_global[other])
        Xh, cov, d1, d2 = ep.triangulate_with_cov(a[1:], b[1:], s.cameras[2].P, s.cameras[other].P, sigma1=ON['traj_sigma_px'][2], sigma2=ON['traj_sigma_px'][other])
        sig = common.Scene.sigma_from_cov(cov)
        ok = (d1 < thres) & (d2 < thres)
        per_cam[other] = (a[0, ok], np.where(np.isfinite(sig[ok]), sig[ok], np.inf), Xh[:3, ok])
    # the camera with the smaller sigmas goes SECOND in the list: "whichever comes first" would keep the other one's points
    order = [0, 1] if np.median(per_cam[1][1]) < np.median(per_cam[0][1]) else [1, 0]
    cand = {}
    for other in order:
        for t, sg, x in zip(per_cam[other][0], per_cam[other][1], per_cam[other][2].T):
            cand.setdefault(float(t), []).append((sg, x))
    X_new = s.triangulate(2, order, thres=thres, factor_t2s=sf, factor_s2t=rate, refit=False)
    assert X_new.shape[1] == sum(len(v) for v in cand.values())
    assert s.traj_sigma.shape == (s.traj.shape[1],) and np.all(np.diff(s.traj[0]) > 0)
    twice = [t for t, v in cand.items() if len(v) == 2 and v[0][0] != v[1][0]]
    assert len(twice) > 20, 'the premise: both other cameras see the uncovered part'
    second_wins = 0
    col = {float(t): j for j, t in enumerate(s.traj[0])}
    for t, v in cand.items():
        best = min(range(len(v)), key=lambda k: (v[k][0], k))          # the smaller sigma, the first on a tie
        j = col[t]
        assert np.array_equal(s.traj[1:, j], v[best][1])
        assert s.traj_sigma[j] == v[best][0] or (np.isnan(s.traj_sigma[j]) and v[best][0] == np.inf)
        second_wins += best == 1
    assert 0 < second_wins, 'the rule is not "the first": some points of the second camera must win'
    new = np.isin(s.traj[0], list(cand))
    finite = [v[0] for vs in cand.values() for v in vs if np.isfinite(v[0])]
    assert np.all(s.traj_sigma[~new] == min(finite))                 # the samples of the spline: the smallest sigma among the new points
    fin = np.isfinite(s.traj_sigma)
    assert np.all(s.traj_sigma[fin] > 0)
    print('\ntriangulate: %d new points at %d timestamps (%d seen twice, %d won by the second camera), sigma %.3g .. %.3g'
          % (X_new.shape[1], len(cand), len(twice), second_wins, min(finite), max(finite)))
    # the refit is the weighted one, and the next rebuild of traj clears the sigmas
    sp = s.traj_to_spline(smooth_factor=sf)
    from mvus_amd import spline
    interval, idx = util.find_intervals(s.traj[0], idx=True)
    by_hand = [spline.traj_fit(s.traj[:, idx[0, i]:idx[1, i] + 1], sf, w=common.Scene.weights_from_sigma(s.traj_sigma[idx[0, i]:idx[1, i] + 1], 1e-3))
               for i in range(interval.shape[1])]
    assert _same_tck(sp['tck'], by_hand)
    s.spline_to_traj(sampling_rate=1)
    assert s.traj_sigma is None


@pytest.mark.gpu
def test_gpu_traj_weights_absent_is_todays_scene():
    """without the setting (absent, or None): traj, the spline and the pickle keys are what a scene without it gives; with it the
    triangulated points themselves are the same bits (triangulate_with_cov), only the choice among duplicates and the fit differ"""
    runs = {}
    probe = _staged_scene(ON)
    probe.triangulate(2, [0, 1], thres=probe.settings['thres_triangulation'], factor_t2s=probe.settings['smooth_factor'], factor_s2t=probe.settings['sampling_rate'], refit=False)
    first_only = _staged_scene({})
    first_only.triangulate(2, [0, 1], thres=probe.settings['thres_triangulation'], factor_t2s=probe.settings['smooth_factor'], factor_s2t=probe.settings['sampling_rate'], refit=False)
    cams = [1, 0] if np.array_equal(probe.traj, first_only.traj) else [0, 1]      # the order in which "the first" is not always "the smaller sigma"
    for label, st in (('absent', {}), ('none', {'traj_weights': None}), ('on', ON)):
        s = _staged_scene(st)
        X_new = s.triangulate(2, cams, thres=s.settings['thres_triangulation'], factor_t2s=s.settings['smooth_factor'], factor_s2t=s.settings['sampling_rate'])
        runs[label] = (s, X_new)
    a, n, on = runs['absent'][0], runs['none'][0], runs['on'][0]
    assert np.array_equal(a.traj, n.traj) and _same_tck(a.spline['tck'], n.spline['tck']) and np.array_equal(a.spline['int'], n.spline['int'])
    assert a.traj_sigma is None and n.traj_sigma is None
    assert sorted(a.__getstate__()) == sorted(n.__getstate__()) and 'traj_sigma' not in a.__getstate__()
    assert set(pickle.loads(pickle.dumps(a)).__dict__) == set(a.__getstate__()) | {'traj_sigma'}      # (the attribute itself is back after loading: None)
    assert np.array_equal(runs['absent'][1], runs['on'][1])          # the same candidates, bit for bit
    assert on.traj_sigma is not None and np.array_equal(a.traj[0], on.traj[0]) and not np.array_equal(a.traj, on.traj)
    assert not _same_tck(a.spline['tck'], on.spline['tck'])
    with pytest.raises(ValueError, match='traj_weights'):
        _staged_scene({'traj_weights': 'covariance'}).traj_weights()
