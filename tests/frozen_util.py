"""Shared by tests/test_frozen_host.py and tests/test_gpu_frozen.py: a drop-in Scene from a golden case, the similarity transform of a
scene, and the mask's indices into the solver's internal order.  Host only."""
import numpy as np

from mvus_amd.reconstruction import common
from mvus_amd.synth import rodrigues


def build_scene(scene, **settings):
    """mvus_amd.reconstruction.common.Scene with the state of a golden case (tests/golden_util.load_case) and extra settings."""
    s = common.Scene()
    s.numCam = scene.num_cam
    s.settings = dict(scene.settings)
    s.settings.update(settings)
    for cam in scene.cameras:
        c = common.Camera(K=cam['K'].copy(), d=cam['d'].copy(), R=cam['R'].copy(), t=cam['t'].copy(), fps=cam['fps'],
                          resolution=list(cam['resolution']))
        c.compose()
        s.addCamera(c)
    for det in scene.detections:
        s.addDetection(det.copy())
    s.alpha, s.beta, s.rs = scene.alpha.copy(), scene.beta.copy(), scene.rs.copy()
    s.sequence = list(range(scene.num_cam))
    s.spline = {'tck': [[t.copy(), [c.copy() for c in cs], 3] for t, cs, _ in scene.tck], 'int': scene.interval.copy()}
    s.detection_to_global()
    return s


def ba_kwargs(st):
    return dict(rs=st['rolling_shutter'], motion_reg=st['motion_reg'], motion_weights=st['motion_weights'], rs_bounds=st['rs_bounds'])


def packed(s, cams):
    st = s.settings
    prob = s._ba_problem(cams, **ba_kwargs(st))
    return prob, s._pack(prob, cams)


def apply_similarity(s, scale, rvec, T):
    """X -> scale * R X + T applied to the world of Scene ``s`` in place: control points move with it, every camera keeps its image
    (R_c -> R_c R^T, t_c -> scale t_c - R_c R^T T); alpha, beta, rs and the calibration do not change."""
    R = rodrigues(np.asarray(rvec, dtype=np.float64))
    T = np.asarray(T, dtype=np.float64)
    for c in s.cameras:
        Rn = np.asarray(c.R) @ R.T
        c.t = scale * np.ravel(c.t) - Rn @ T
        c.R = Rn
        c.compose()
    for tck in s.spline['tck']:
        X = scale * (R @ np.vstack(tck[1])) + T[:, None]
        tck[1] = [X[0].copy(), X[1].copy(), X[2].copy()]


def internal_of_mask(mask, C, P):
    """(camera, slot) of every set entry of a pack_x-order mask: slot 0 alpha, 1 beta, 2 rs, 3 + j camera parameter j."""
    out = []
    for k in np.nonzero(mask)[0]:
        out.append((int(k % C), int(k // C)) if k < 3 * C else (int((k - 3 * C) // P), 3 + int((k - 3 * C) % P)))
    return out
