"""``Scene`` / ``Camera`` / ``create_scene`` with the reference's names, attributes and config surface
(reference ``multiviewunsynch/reconstruction/common.py``), with the bundle-adjustment hot path --
``Scene.BA`` (common.py:441-697), ``Scene.remove_outliers`` (:700-717), ``Scene.error_cam`` (:304-359) --
running on the GPU through libmvusba.so.  There is no CPU fallback for those three.

Kept from the reference: the ``Scene`` attribute set that ends up in the output pickle (README "Output"),
method names and signatures, the ``config.json`` schema (``create_scene``), the parameter-vector layout and the
side effects of ``BA`` on ``alpha/beta/rs/cameras/spline/detections_global``.

Also on the GPU: ``Scene.init_traj`` (two-view initialisation: fundamental matrix by RANSAC, optimal correction, pose from
E), ``Scene.time_shift`` with ``cf_exact: false`` and ``sync_method: 'bf'`` (synchronization.sync_bf), ``get_camera_pose`` (PnP +
RANSAC) and ``Scene.triangulate`` (per-point SVD).  Out of scope: ``sync_iter``, plotting, and the dead ``motion_prior=True``
branch -- those raise ``NotImplementedError``.  The optional ``settings`` keys this package adds (``ba_*``; a reference ``config.json``
has none of them) are listed, documented and validated in ``ba_settings.py``.
"""
import json

import numpy as np

from ..tools import util
from .. import problem as _problem
from ..synth import rodrigues as _rodrigues, rotation_to_rvec as _rotation_to_rvec
from . import ba_settings as _settings
from .surveyed import check_landmarks, check_position_priors, load_landmarks, load_position_priors, umeyama_similarity, _undistort_normalised  # noqa: F401


def _undistort_normalized(points, K, d):
    """cv2.undistortPoints(src, K, d): 5 fixed-point iterations of the 5-coefficient model (host copy of
    ``undistort5`` in csrc/ba_math.h; used outside the BA loop only)."""
    k1, k2, p1, p2, k3 = [float(v) for v in np.asarray(d, dtype=np.float64).reshape(-1)[:5]]
    x0 = (points[0] - K[0, 2]) / K[0, 0]
    y0 = (points[1] - K[1, 2]) / K[1, 1]
    x, y = x0.copy(), y0.copy()
    reset = np.zeros(np.shape(x), dtype=bool)        # OpenCV >= 4.1.1: a negative 1/(1 + k1 r^2 + ...) puts the point back at its start for good
    for _ in range(5):
        r2 = x * x + y * y
        with np.errstate(divide='ignore', invalid='ignore'):
            icd = 1.0 / (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2)
        reset = reset | (icd < 0)
        dx = 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
        dy = p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
        x, y = np.where(reset, x0, (x0 - dx) * icd), np.where(reset, y0, (y0 - dy) * icd)
    return np.vstack((x, y))


# Floor of the LM damping that mvus_amd.pipeline.incremental_reconstruction sets (settings['ba_lambda_min']) when the loop runs with
# ba_solver = 'lm' and the caller gave none.  The staged BAs of the loop -- two or three cameras, similarity gauge free, a motion
# regulariser that is not scale invariant -- slope towards a smaller scene; a nearly undamped Newton step (the library's floor, 3e-3,
# chosen for single large BAs) follows that slope where the reference's ten truncated LSMR solves barely move.  Eleven seeds of the
# loop: with 0.3 every seed ends 0.21 - 0.43 m from the truth (the reference's algorithm: 0.23 - 0.51 m), with 3e-3 one seed in
# three ends metres away (profiles/round4/r04_loop_lm_damping_floors.txt).  A single Scene.BA keeps the library's floor: with 0.3 its last
# steps get short enough for xtol to end a 200-evaluation solve above the minimum (dist_fixed_2cam: cost 252.9 against 238.0).
LOOP_LM_LAMBDA_MIN = 0.3


class Camera:
    """K, R, t, d, P container (reference common.py:1040-1168)."""

    def __init__(self, **kwargs):
        self.P = kwargs.get('P')
        self.K = kwargs.get('K')
        self.R = kwargs.get('R')
        self.t = kwargs.get('t')
        self.d = kwargs.get('d')
        self.c = kwargs.get('c')
        self.fps = kwargs.get('fps')
        self.resolution = kwargs.get('resolution')

    def projectPoint(self, X):
        assert self.P is not None, 'The projection matrix P has not been calculated yet'
        if X.shape[0] == 3:
            X = util.homogeneous(X)
        x = self.P @ X
        return x / x[2]

    def compose(self):
        self.P = self.K @ np.hstack((self.R, np.asarray(self.t, dtype=np.float64).reshape(3, 1)))

    def decompose(self):
        M = self.P[:, :3]
        Rinv, Kinv = np.linalg.qr(np.linalg.inv(M))
        R, K = np.linalg.inv(Rinv), np.linalg.inv(Kinv)
        T = np.diag(np.sign(np.diag(K)))
        if np.linalg.det(T) < 0:
            T[1, 1] *= -1
        self.K, self.R = K @ T, T @ R
        self.t = np.linalg.inv(self.K) @ self.P[:, 3]
        self.K = self.K / self.K[-1, -1]
        return self.K, self.R, self.t

    def center(self):
        if self.c is None:
            self.decompose()
            self.c = -self.R.T @ self.t
        return self.c

    def P2vector(self, calib=False):
        r = _rotation_to_rvec(self.R)
        if calib:
            return np.concatenate(([self.K[0, 0], self.K[1, 1], self.K[0, 2], self.K[1, 2]], r, self.t, self.d))
        return np.concatenate((r, self.t))

    def vector2P(self, vector, calib=False):
        vector = np.asarray(vector, dtype=np.float64)
        if calib:
            self.K = np.diag((1.0, 1.0, 1.0))
            self.K[0, 0], self.K[1, 1] = vector[0], vector[1]
            self.K[:2, -1] = vector[2:4]
            self.R = _rodrigues(vector[4:7])
            self.t = vector[7:10].copy()
            self.d = vector[10:].copy()
        else:
            self.R = _rodrigues(vector[:3])
            self.t = vector[3:6].copy()
        self.compose()
        return self.P

    def undist_point(self, points):
        assert points.shape[0] == 2, 'Input must be a 2D array'
        return (self.K @ util.homogeneous(_undistort_normalized(points, self.K, self.d)))[:2]

    def info(self):
        for name in ('P', 'K', 'R', 't'):
            print('\n %s:' % name)
            print(getattr(self, name))


def ellipse_2x2(cov):
    """(semi_major, semi_minor, angle) of the 1-sigma ellipses of the symmetric 2 x 2 matrices cov = (uu, uv, vv), shape [3, ...]: the
    closed form  lambda = (uu + vv) / 2 +- sqrt(((uu - vv) / 2)^2 + uv^2),  angle = atan2(2 uv, uu - vv) / 2  of the major axis from the
    first axis towards the second, in (-pi / 2, pi / 2].  A negative small eigenvalue (rounding) gives semi_minor 0; NaN stays NaN."""
    uu, uv, vv = (np.asarray(v, dtype=np.float64) for v in cov)
    mean, half = 0.5 * (uu + vv), 0.5 * (uu - vv)
    rad = np.hypot(half, uv)
    with np.errstate(invalid='ignore'):
        major = np.sqrt(np.maximum(mean + rad, 0.0))
        minor = np.sqrt(np.maximum(mean - rad, 0.0))
    return major, minor, 0.5 * np.arctan2(2.0 * uv, uu - vv)


def chi2_2_quantile(p):
    """The p quantile of chi^2 with 2 degrees of freedom, -2 ln(1 - p) (its distribution function is 1 - exp(-x / 2))."""
    p = float(p)
    if not 0.0 <= p < 1.0:
        raise ValueError('chi2_2_quantile: p must lie in [0, 1), not %r' % (p,))
    return -2.0 * float(np.log1p(-p))


class Scene:
    """Everything known about the scene (reference common.py:22-61)."""

    def __init__(self):
        self.numCam = 0
        self.cameras = []
        self.detections = []
        self.detections_raw = []
        self.detections_global = []
        self.alpha = []
        self.beta = []
        self.beta_after_Fbeta = []
        self.cf = []
        self.traj = []
        self.traj_len = []
        self.sequence = []
        self.visible = []
        self.settings = []
        self.gt = []
        self.out = {}
        self.spline = {'tck': [], 'int': []}
        self.rs = []
        self.ref_cam = 0
        self.find_order = True
        self._ba_handle = None      # GPU handle kept between BA -> remove_outliers -> BA (main.py:49-62)
        self._ba_key = None
        self.landmarks = None          # (3, L) surveyed static points, or None (settings['ba_landmarks'])
        self.landmark_observations = None      # (6, K): camera id, landmark, u, v, sigma_u, sigma_v
        self.position_priors = None    # (7, K): t, x, y, z, sigma_x, sigma_y, sigma_z of surveyed positions, or None (settings['ba_position_priors'])
        self.traj_sigma = None         # 1-sigma (sqrt(trace(cov) / 3)) of every column of traj, or None (settings['traj_weights'])

    def __getstate__(self):         # the output pickle (main.py:93) carries data only
        state = dict(self.__dict__)
        state['_ba_handle'] = None
        state['_ba_key'] = None
        if state.get('traj_sigma') is None:      # (carried only when set: without settings['traj_weights'] the pickle has the keys it had)
            state.pop('traj_sigma', None)
        return state

    def __setstate__(self, state):
        self.__dict__.update(state)
        self.__dict__.setdefault('traj_sigma', None)

    # ---- bookkeeping --------------------------------------------------------------------------
    def addCamera(self, *camera):
        for c in camera:
            assert type(c) is Camera, 'camera is not an instance of Camera'
            self.cameras.append(c)

    def addDetection(self, *detection):
        for d in detection:
            assert d.shape[0] == 3, 'Detection must in form of (x,y,frameId)*N'
            self.detections.append(d)

    def init_alpha(self, *prior):
        if len(prior):
            assert len(prior) == self.numCam, 'Number of input must be the same as the number of cameras'
            self.alpha = prior
        else:
            fps_ref = self.cameras[self.ref_cam].fps
            self.alpha = np.array([fps_ref / self.cameras[i].fps for i in range(self.numCam)], dtype=np.float64)

    def time_shift(self, iter=False):
        assert len(self.cf) == self.numCam, 'The number of frame indices should equal to the number of cameras'
        if self.settings['cf_exact']:
            self.beta = self.cf[self.ref_cam] - self.alpha * self.cf
            print('The given corresponding frames are directly exploited as temporal synchronization\n')
        else:
            # common.py:1016-1040: the brute-force search of synchronization.sync_bf against the reference camera, each of its
            # two stages one batched RANSAC call on the GPU
            from . import synchronization as sync
            method = self.settings.get('sync_method')
            if method == 'iter':
                sync_fun = sync.sync_iter
            elif method == 'bf':
                sync_fun = sync.sync_bf
            elif method == 'iter_gpu':
                # the reference's sync_iter on the GPU; settings['sync_iter'] may override its search parameters
                import functools
                over = dict(self.settings.get('sync_iter') or {})
                unknown = set(over) - {'maxIter', 'threshold', 'step', 'p_min', 'p_max', 'seed'}
                if unknown:
                    raise ValueError('settings["sync_iter"]: unknown key(s) %s' % sorted(unknown))
                sync_fun = functools.partial(sync.sync_iter_gpu, **over)
            else:
                raise ValueError('Synchronization method must be "iter", "bf" or "iter_gpu"')
            device = int(self.settings.get('device', 0))
            print('Computing temporal synchronization...\n')
            beta = np.zeros(self.numCam)
            i = self.ref_cam
            for j in range(self.numCam):
                if j != i:
                    beta[j], _ = sync_fun(self.cameras[i].fps, self.cameras[j].fps, self.detections[i], self.detections[j],
                                          self.cf[i], self.cf[j], device=device)
                print('Status: {} from {} cam finished'.format(j + 1, self.numCam))
            self.beta = beta
            self.beta_after_Fbeta = beta.copy()

    def detection_to_global(self, *cam, motion_prior=False):
        """Frame indices -> global timeline, and the observed pixel (common.py:105-127)."""
        assert len(self.alpha) == self.numCam and len(self.beta) == self.numCam, 'The Number of alpha and beta is wrong'
        if motion_prior:
            raise NotImplementedError('motion_prior branch is dead in the reference pipeline')
        if len(cam):
            cams = cam if isinstance(cam[0], (int, np.integer)) else cam[0]
        else:
            cams = range(self.numCam)
            self.detections_global = [[] for _ in cams]
        for i in cams:
            det = self.detections[i]
            ts = self.alpha[i] * (det[0] + self.rs[i] * det[2] / self.cameras[i].resolution[1]) + self.beta[i]
            obs = self.cameras[i].undist_point(det[1:]) if self.settings['undist_points'] else det[1:]
            self.detections_global[i] = np.vstack((ts, obs))

    def cut_detection(self, second=1):
        if not second:
            return
        for i in range(self.numCam):
            det = self.detections[i]
            interval = util.find_intervals(det[0])
            cut = int(self.cameras[i].fps * second)
            keep = interval[:, interval[1] - interval[0] > cut * 2]
            keep[0] += cut
            keep[1] -= cut
            assert (keep[1] - keep[0] >= 0).all()
            self.detections[i], _ = util.sampling(det, keep)

    # ---- spline <-> trajectory: evaluation on the GPU, FITPACK's adaptive knot search on the host ----
    def traj_to_spline(self, smooth_factor):
        """One smoothing cubic spline per contiguous part of ``self.traj`` (reference common.py:224-270): FITPACK's ``splprep``
        inside the reference's knot-density loop, with the sample passes and banded solves on the GPU
        (``mvus_amd.spline.traj_fit`` -> ``mvus_spline_smooth``; no host fallback)."""
        from .. import spline as _spline
        assert len(smooth_factor) == 2, 'Smoothness should be defined by two parameters (min, max)'
        interval, idx = util.find_intervals(self.traj[0], idx=True)
        device = self._device()
        sigma = getattr(self, 'traj_sigma', None)
        # traj_sigma counts only while it is aligned with traj: code that cuts or reorders self.traj by hand (s.traj = s.traj[:, mask]) and
        # does not cut traj_sigma with it gets the unweighted fit, said aloud -- sigmas of other samples would be worse than none
        if sigma is not None and len(sigma) != self.traj.shape[1]:
            print('traj_to_spline: traj_sigma has %d entries for %d samples -- fitting without weights' % (len(sigma), self.traj.shape[1]))
        if sigma is not None and len(sigma) == self.traj.shape[1]:
            # settings['traj_weights']: splprep's w from the 1-sigma of every sample, interval by interval (only the ratios inside a fit matter)
            floor = self.traj_weights()[2]
            tck = [_spline.traj_fit(self.traj[:, idx[0, i]:idx[1, i] + 1], smooth_factor, device=device,
                                    w=self.weights_from_sigma(sigma[idx[0, i]:idx[1, i] + 1], floor)) for i in range(interval.shape[1])]
        else:
            tck = [_spline.traj_fit(self.traj[:, idx[0, i]:idx[1, i] + 1], smooth_factor, device=device) for i in range(interval.shape[1])]
        self.spline['tck'], self.spline['int'] = tck, interval
        return self.spline

    def traj_weights(self):
        """``settings['traj_weights']``: None (absent: every method does what the reference does), or (mode, sigma_px, floor) with mode
        'triangulation' -- ``init_traj`` and ``triangulate`` then keep the 1-sigma of every triangulated point in ``traj_sigma``
        (``triangulate_with_cov`` with ``settings['traj_sigma_px']`` pixels of noise: a scalar or one value per camera, default 1) and
        ``traj_to_spline`` fits with w = max(sigma_min / sigma, ``settings['traj_weight_floor']``) (default 1e-3)."""
        return _settings.traj_weights(_settings.as_dict(self.settings), self.numCam)

    @staticmethod
    def weights_from_sigma(sigma, floor=1e-3):
        """splprep's w of one trajectory part from the 1-sigma of its samples: max(sigma_min / sigma, floor), the floor where sigma is NaN
        (a pair without parallax); sigma_min over the finite, positive values of the part."""
        sigma = np.asarray(sigma, dtype=np.float64)
        ok = np.isfinite(sigma) & (sigma > 0)
        w = np.full(sigma.shape, float(floor))
        if ok.any():
            w[ok] = np.maximum(sigma[ok].min() / sigma[ok], floor)
        return w

    @staticmethod
    def sigma_from_cov(cov):
        """sqrt(trace(cov) / 3) of (N, 3, 3) covariances: the 1-sigma of an isotropic point with the same total variance (NaN stays NaN)"""
        return np.sqrt(np.trace(np.asarray(cov, dtype=np.float64), axis1=1, axis2=2) / 3.0)

    def spline_to_traj(self, sampling_rate=1, t=None):
        """Discrete 3D points of the splines (common.py:273-301): sampled at a constant rate or at the given timestamps,
        kept where they lie inside an interval (closed ends), interval by interval.  The evaluation runs on the GPU
        (``mvus_spline_eval``, the FITPACK recurrence of the BA kernels) instead of scipy's splev."""
        from .. import spline as _spline
        tck, interval = self.spline['tck'], self.spline['int']
        if t is not None:
            assert len(t.shape) == 1, 'Input timestamps must be a 1D array'
            ts = np.asarray(t, dtype=np.float64)
        else:
            ts = np.arange(interval[0, 0], interval[1, -1], sampling_rate)
        X, which = _spline.evaluate(tck, interval, ts, device=self._device())
        parts = [np.empty([4, 0])]
        for i in range(interval.shape[1]):                       # the reference's order: interval by interval
            m = which == i
            if m.any():
                parts.append(np.vstack((ts[m], X[:, m])))
        self.traj = np.hstack(parts)
        self.traj_sigma = None                                   # samples of the spline: no triangulation behind them
        assert (self.traj[0, 1:] >= self.traj[0, :-1]).all()
        return self.traj

    def all_detect_to_traj(self, *cam):
        """Attributes the reference refreshes while regularising (common.py:887-947); they do not enter the
        residual, so they are computed once after BA instead of on every evaluation."""
        cams = list(cam[0]) if len(cam) else list(range(self.numCam))
        self.detection_to_global(cams)
        ts = np.concatenate([self.detections_global[i][0] for i in cams])
        frames = np.concatenate([self.detections[i][0] for i in cams])
        ids = np.concatenate([np.full(self.detections[i].shape[1], float(i)) for i in cams])
        self.frame_id_all = frames
        self.global_time_stamps_all = ts
        self.spline_to_traj(t=np.sort(ts))
        self.global_detections = np.vstack((ids, frames, ts))
        ordered = self.global_detections[:, np.argsort(ts)]
        ordered = ordered[:, np.isin(ordered[2], self.traj[0])]
        self.global_traj = np.vstack((np.arange(ordered.shape[1]), ordered, self.traj[1:]))
        assert (self.global_traj[3][1:] >= self.global_traj[3][:-1]).all(), 'timestamps are not in ascending order'

    # ---- the hot path --------------------------------------------------------------------------
    def _ba_problem(self, cams, rs=False, motion_reg=False, motion_weights=1, rs_bounds=False):
        st = self.settings
        return _problem.problem_from_arrays(
            [self.detections[i] for i in cams], [self.cameras[i] for i in cams], self.spline['tck'], self.spline['int'],
            opt_calib=st['opt_calib'], undist_points=st['undist_points'], rs=rs, rs_bounds=rs_bounds,
            motion_reg=motion_reg, motion_type=st.get('motion_type', 'F'), motion_weights=motion_weights,
            opt_sync=st.get('opt_sync', True))                      # absent -> alpha, beta free (common.py:512-515)

    def _pack(self, prob, cams):
        return _problem.pack_x(prob, np.asarray(self.alpha)[cams], np.asarray(self.beta)[cams], np.asarray(self.rs)[cams],
                               [self.cameras[i] for i in cams], self.spline['tck'])

    def _device(self):
        return int(_settings.as_dict(self.settings).get('device', 0))

    def _handle(self, prob):
        from ..ba import BAHandle          # raises if libmvusba.so is missing: no CPU fallback
        return BAHandle(prob, device=self._device())

    @staticmethod
    def _same_problem(a, b):
        if (a.num_cam, a.opt_calib, a.undist_points, a.rs_free, a.rs_bounds, a.motion_reg, a.motion_type, a.motion_weight, a.opt_sync) != \
           (b.num_cam, b.opt_calib, b.undist_points, b.rs_free, b.rs_bounds, b.motion_reg, b.motion_type, b.motion_weight, b.opt_sync):
            return False
        pairs = [(a.det_offsets, b.det_offsets), (a.frame, b.frame), (a.u_raw, b.u_raw), (a.v_raw, b.v_raw),
                 (a.img_height, b.img_height), (a.interval, b.interval), (a.knot_offsets, b.knot_offsets), (a.knots, b.knots)]
        if not a.opt_calib:                      # with opt_calib K and d are parameters (in x), not problem data
            pairs += [(a.K, b.K), (a.dist, b.dist)]
        return all(x.shape == y.shape and np.array_equal(x, y) for x, y in pairs)

    def _resident_handle(self, prob, cams):
        """The handle of the previous BA over the same cameras if its (device-resident) problem is still this one."""
        h = self._ba_handle
        if h is not None and h.h and self._ba_key == tuple(cams) and self._same_problem(h.prob, prob):
            return h
        if h is not None:
            h.close()
        self._ba_handle, self._ba_key = self._handle(prob), tuple(cams)
        return self._ba_handle

    def _configured_handle(self, prob, cams):
        """``_resident_handle`` with the loss, the held parameters, the position priors and the landmarks of the settings in force (sent only where they differ)."""
        h = self._resident_handle(prob, cams)
        h.configure(loss=self.ba_loss(), frozen=self.ba_frozen_mask(cams), position_priors=self.ba_position_priors(), landmarks=self.ba_landmarks(cams))
        return h

    def _resident_for(self, cams):
        """The handle left by the last BA if it still describes the CURRENT scene state of its cameras (detections, knots,
        intervals, fixed calibration, flags) and covers ``cams``; else None.  x is packed from the current state."""
        h = self._ba_handle
        if h is None or not h.h or self._ba_key is None or not set(cams) <= set(self._ba_key):
            return None
        key = list(self._ba_key)
        if any(self.detections[i].shape[1] != int(h.prob.det_offsets[k + 1] - h.prob.det_offsets[k]) for k, i in enumerate(key)):
            return None
        now = self._ba_problem(key, rs=h.prob.rs_free, motion_reg=h.prob.motion_reg, motion_weights=h.prob.motion_weight,
                               rs_bounds=h.prob.rs_bounds)
        return h if self._same_problem(h.prob, now) else None

    def error_cam(self, cam_id, mode='dist', motion_prior=False, norm=False):
        """Reprojection errors of one camera (common.py:304-359), evaluated by the HIP residual kernel: on the handle the
        last BA left resident when it still describes the scene, else on a temporary residual-only handle."""
        if motion_prior or norm:
            raise NotImplementedError('motion_prior / norm variants are not on the BA hot path')
        self.detection_to_global(cam_id)
        h = self._resident_for([cam_id])
        if h is not None:
            key = list(self._ba_key)
            k = key.index(cam_id)
            a, b = int(h.prob.det_offsets[k]), int(h.prob.det_offsets[k + 1])
            f = h.residual(self._pack(h.prob, key))[2 * a:2 * b]
        else:
            prob = self._ba_problem([cam_id])
            with self._handle(prob) as tmp:
                f = tmp.residual(self._pack(prob, [cam_id]))
        M = self.detections[cam_id].shape[1]
        ex, ey = f[:M], f[M:2 * M]
        if mode == 'each':
            return np.concatenate((ex, ey))
        _, ids = util.sampling(self.detections_global[cam_id], self.spline['int'], belong=True)
        order = np.concatenate([np.nonzero(ids == s + 1)[0] for s in range(self.spline['int'].shape[1])]).astype(int)
        if mode == 'dist':
            return np.sqrt(ex[order] ** 2 + ey[order] ** 2)
        if mode == 'xy_1D':
            return np.concatenate((ex[order], ey[order]))
        if mode == 'xy_2D':
            return np.vstack((ex[order], ey[order]))
        raise ValueError('unknown mode %r' % (mode,))

    def compute_visibility(self):
        self.visible = []
        self.detection_to_global()
        for cam_id in range(self.numCam):
            _, vis = util.sampling(self.detections_global[cam_id], self.spline['int'], belong=True)
            self.visible.append(vis)

    @staticmethod
    def _motion_band_width(prob):
        """Control points a motion row couples (common.py:959-1001: samples j-1, j, j+1, four control points each), i.e. the block
        band width W of the spline part of J^T J; 4 without the regulariser."""
        if not prob.motion_reg:
            return 4
        ts, sid = prob.motion_sample_times()
        coff = prob.ctrl_offsets
        first = np.empty(ts.size, dtype=np.int64)
        for s in range(prob.S):
            t = prob.knots[int(prob.knot_offsets[s]):int(prob.knot_offsets[s + 1])]
            sel = sid == s
            first[sel] = coff[s] + np.clip(np.searchsorted(t, ts[sel], side='right') - 1, 3, t.size - 5) - 3
        W = 4
        step = 2 if prob.motion_type == 0 else 1            # 'F' rows use three samples, 'KE' two
        for d in range(1, step + 1):
            same = sid[d:] == sid[:-d]
            if same.any():
                W = max(W, int(np.max(np.abs(first[d:] - first[:-d])[same])) + 4)
        return W

    def BA(self, numCam, max_iter=10, rs=False, motion_prior=False, motion_reg=False, motion_weights=1, norm=False,
           rs_bounds=False, jac_sparsity=None):
        """Bundle adjustment over ``self.sequence[:numCam]`` (common.py:441-697): same arguments, same side effects,
        the optimisation itself runs in ``mvus_ba_solve`` on the GPU.  ``jac_sparsity`` (not in the reference's signature):
        the matrix ``jac_BA`` would return, for callers that have it -- the parity modes then use exactly that pattern
        instead of rebuilding it on the GPU (the reference hands the same matrix to ``least_squares``, common.py:670)."""
        if motion_prior:
            raise NotImplementedError('motion_prior=True is dead code in the reference pipeline (SURVEY.md section 2)')
        from .. import ba as _ba
        cams = list(self.sequence[:numCam])
        self.alpha, self.beta, self.rs = (np.asarray(v, dtype=np.float64) for v in (self.alpha, self.beta, self.rs))
        prob = self._ba_problem(cams, rs=rs, motion_reg=motion_reg, motion_weights=motion_weights, rs_bounds=rs_bounds)
        model = self._pack(prob, cams)
        print('Number of BA parameters is {}'.format(len(model)))
        print('Doing BA with {} cameras...\n'.format(numCam))
        st = self.settings
        solver, jac_mode = self.ba_mode()
        h = self._configured_handle(prob, cams)    # stays resident for remove_outliers and the next BA
        opts = _settings.solve_options(st, solver, jac_mode, max_iter)
        try:
            if solver == _ba.SOLVER_LM_SCHUR and st.get('ba_lm_wide_band', 'trf') != 'lm' and self._motion_band_width(prob) > 6:
                # POLICY, not a limit of the library (it solves bands of up to sixteen control points, tests/test_gpu_schur.py): knots less
                # than a frame apart mean more control points than detections -- what traj_to_spline returns after a dense triangulate
                # inside the incremental loop -- and there an exact Newton-type step follows the regulariser-only directions: three
                # seeds of the loop end 2.6 - 8 m from the truth with LM on those problems, 0.2 - 0.35 m with the truncated solver
                # (profiles/round4/r04_loop_lm_wide_band.txt).  settings['ba_lm_wide_band'] = 'lm' keeps LM (damping floor 0.3).
                raise _ba.UnsupportedBySolver("settings['ba_lm_wide_band'] = 'trf': the motion rows reach over more than six control points (knots less than a frame apart)")
            res = h.solve(model, opts=opts, ties=st.get('ba_pattern_ties', 'numpy'), matrix=jac_sparsity)
            res.solver_used = 'lm' if solver == _ba.SOLVER_LM_SCHUR else 'trf'
        except _ba.UnsupportedBySolver as e:
            # the other solver has no robust loss, no position priors and no landmarks: handing the problem over would silently solve without them
            for on, key, what, off in ((h.loss[0] != _ba.LOSS_LINEAR, "ba_loss'] = %r" % (st.get('ba_loss'),), 'loss', "ba_loss: 'linear'"),
                                       (h.num_active_position_priors, "ba_position_priors']", 'priors', 'ba_position_priors: false'),
                                       (h.num_landmark_rows, "ba_landmarks']", 'landmarks', 'ba_landmarks: false')):
                if on:
                    raise _ba.UnsupportedBySolver("settings['%s needs the LM solver, which does not take this problem (%s); the fallback to ba_solver=trf "
                                                  "would drop the %s -- set ba_lm_wide_band: 'lm' or %s" % (key, e, what, off)) from e
            # LM + Schur keeps the spline block as a band of at most sixteen 3x3 blocks (MVUS_E_UNSUPPORTED beyond; FITPACK knots far
            # below one frame apart make the motion rows reach further).  The other GPU solver has no such limit: same analytic
            # Jacobian, TRF + LSMR instead of the normal equations.  Said aloud and recorded in the result, not silently.
            print('BA: %s -- solving this problem with ba_solver=trf (analytic Jacobian) instead' % e)
            opts = _ba._lib.default_opts(_ba.SOLVER_TRF_LSMR, _ba.JAC_ANALYTIC, max_iter)
            res = h.solve(model, opts=opts, ties='canonical')
            res.solver_used = 'trf (fallback from lm: %s)' % e
        res.num_frozen = h.num_frozen
        res.num_position_priors = h.num_position_priors
        res.num_active_position_priors = h.num_active_position_priors
        res.num_landmark_observations = h.num_landmark_observations
        alpha, beta, rs_new, cam_states, coefs = _problem.unpack_x(prob, res.x)
        self.alpha[cams], self.beta[cams], self.rs[cams] = alpha, beta, rs_new
        for k, i in enumerate(cams):
            c = self.cameras[i]
            if st['opt_calib']:
                c.K, c.d = cam_states[k]['K'], cam_states[k]['d']
            c.R, c.t = cam_states[k]['R'], cam_states[k]['t']
            c.compose()
        for s, c in enumerate(coefs):
            self.spline['tck'][s][1] = c
        self.detection_to_global()
        if motion_reg:
            self.all_detect_to_traj(cams)
            self.spline_to_traj()
        return res

    def ba_mode(self):
        """(solver, Jacobian mode) that ``BA`` runs with the current settings.  Without any ``ba_*`` key -- a reference
        config.json -- that is the reference's own algorithm: TRF + LSMR over grouped 2-point differences."""
        st = _settings.as_dict(self.settings)
        _settings.validate(st)               # every ba_* key of the table: a bad one raises before any GPU call
        self.ba_position_priors()            # (and the arrays they switch on: Scene.position_priors,
        self.ba_landmarks()                  # Scene.landmarks / Scene.landmark_observations)
        return _settings.solver_and_jacobian(st)

    def ba_landmarks(self, cams=None):
        """(X (3, L), cam (K,), point (K,), uv (2, K), sigma (2, K)) when settings['ba_landmarks'] is true and the scene holds landmarks and
        observations, else None.  Validated on the host, before any GPU call: the flag is a bool, the arrays are finite with positive sigmas
        (inf = that axis unknown) and landmark indices inside [0, L), and the solver must be 'lm'.  ``cams``: the BA's camera set --
        observations of other cameras are left out and the camera id becomes the index in ``cams`` (None: ids as they are)."""
        if not _settings.needs_lm(_settings.as_dict(self.settings), 'ba_landmarks', 'landmarks'):
            return None
        X, ob = getattr(self, 'landmarks', None), getattr(self, 'landmark_observations', None)
        if X is None or ob is None:
            return None
        X, ob = check_landmarks(X, ob, 'Scene.landmarks')
        cam = ob[0].astype(np.int64)
        if cams is not None:
            index = {int(c): k for k, c in enumerate(cams)}
            keep = np.array([int(c) in index for c in cam], dtype=bool)
            ob, cam = ob[:, keep], np.array([index[int(c)] for c in cam[keep]], dtype=np.int64)
        if ob.shape[1] == 0:
            return None
        return X.copy(), cam.astype(np.int32), ob[1].astype(np.int32), ob[2:4].copy(), ob[4:6].copy()

    def triangulate_landmarks(self):
        """(ids, Y (3, len(ids))): every landmark seen by at least two cameras that have a pose, triangulated from the current cameras by a
        multi-view DLT on the host (undistorted, normalised image points; L is tens).  Whatever the settings say."""
        X, ob = getattr(self, 'landmarks', None), getattr(self, 'landmark_observations', None)
        if X is None or ob is None:
            return np.empty(0, dtype=np.int64), np.empty((3, 0))
        X, ob = check_landmarks(X, ob, 'Scene.landmarks')
        undist = bool(_settings.as_dict(self.settings).get('undist_points', False))
        ids, Y = [], []
        for l in range(X.shape[1]):
            rows, seen = [], set()
            for k in np.nonzero(ob[1].astype(np.int64) == l)[0]:
                c = int(ob[0, k])
                if not 0 <= c < len(self.cameras):
                    continue
                cam = self.cameras[c]
                if getattr(cam, 'R', None) is None or getattr(cam, 't', None) is None or cam.K is None:
                    continue
                K = np.asarray(cam.K, dtype=np.float64)
                xn, yn = (ob[2, k] - K[0, 2]) / K[0, 0], (ob[3, k] - K[1, 2]) / K[1, 1]
                if undist and cam.d is not None:
                    xn, yn = _undistort_normalised(xn, yn, np.ravel(np.asarray(cam.d, dtype=np.float64)))
                Pm = np.hstack((np.asarray(cam.R, dtype=np.float64), np.ravel(np.asarray(cam.t, dtype=np.float64))[:, None]))
                rows += [xn * Pm[2] - Pm[0], yn * Pm[2] - Pm[1]]
                seen.add(c)
            if len(seen) < 2:
                continue
            A = np.array(rows)
            A /= np.linalg.norm(A, axis=1, keepdims=True)
            v = np.linalg.svd(A)[2][-1]
            if v[3] == 0:
                continue
            ids.append(l)
            Y.append(v[:3] / v[3])
        return np.array(ids, dtype=np.int64), (np.array(Y).T if Y else np.empty((3, 0)))

    def align_to_landmarks(self):
        """The similarity (Umeyama) that takes the landmarks as the current cameras triangulate them (``triangulate_landmarks``) onto their
        surveyed positions, applied to the scene (``apply_similarity``); returns (s, R, T, rms).  Needs at least three such landmarks that
        are not collinear -- the rule of ``align_to_position_priors`` -- else ValueError."""
        ids, Y = self.triangulate_landmarks()
        if ids.size < 3:
            raise ValueError('align_to_landmarks: %d landmarks seen by at least two placed cameras, at least 3 are needed' % ids.size)
        Xs = np.asarray(self.landmarks, dtype=np.float64)[:, ids]
        sv = np.linalg.svd(Xs - Xs.mean(axis=1, keepdims=True), compute_uv=False)
        if not sv[1] > 1e-6 * sv[0]:
            raise ValueError('align_to_landmarks: the landmarks are collinear (singular values %s): the similarity is not determined' % (sv,))
        s, R, T = umeyama_similarity(Y, Xs)
        rms = float(np.sqrt(np.mean(np.sum((s * (R @ Y) + T[:, None] - Xs) ** 2, axis=0))))
        self.apply_similarity(s, R, T)
        return s, R, T, rms

    def ba_position_priors(self):
        """(t (K,), P (3, K), sigma (3, K)) when settings['ba_position_priors'] is true and ``self.position_priors`` holds priors, else
        None.  Validated on the host, before any GPU call: the flag is a bool, the array is (7, K) of finite t, x, y, z and positive
        sigmas (inf = that axis unknown), and the solver must be 'lm'."""
        if not _settings.needs_lm(_settings.as_dict(self.settings), 'ba_position_priors', 'position priors'):
            return None
        pp = getattr(self, 'position_priors', None)
        if pp is None:
            return None
        pp = check_position_priors(pp, 'Scene.position_priors')
        return pp[0].copy(), pp[1:4].copy(), pp[4:7].copy()

    def _active_position_priors(self):
        """(t, P) of the priors whose time lies in an interval of the spline (closed ends), whatever the settings say."""
        pp = getattr(self, 'position_priors', None)
        if pp is None:
            return np.empty(0), np.empty((3, 0))
        pp = check_position_priors(pp, 'Scene.position_priors')
        iv = np.asarray(self.spline['int'], dtype=np.float64)
        act = np.any((pp[0][None, :] >= iv[0][:, None]) & (pp[0][None, :] <= iv[1][:, None]), axis=0) if iv.size else np.zeros(pp.shape[1], bool)
        return pp[0, act], pp[1:4, act]

    def apply_similarity(self, s, R, T):
        """Move the whole reconstruction by the similarity X -> s R X + T of the world: the control points of every spline move with it and
        every camera keeps its image (R_c -> R_c R^T, t_c -> s t_c - R_c R^T T: the projection of the moved point is the old one, up to the
        homogeneous factor s).  alpha, beta, rs, K and d are untouched; ``traj``, when present, moves too."""
        s = float(s)
        R = np.asarray(R, dtype=np.float64).reshape(3, 3)
        T = np.asarray(T, dtype=np.float64).reshape(3)
        if not (np.isfinite(s) and s > 0 and np.all(np.isfinite(R)) and np.all(np.isfinite(T))):
            raise ValueError('apply_similarity: s must be finite and positive, R and T finite')
        for tck in self.spline['tck']:
            c = np.asarray(tck[1], dtype=np.float64)              # [cx, cy, cz]
            moved = s * (R @ c) + T[:, None]
            tck[1] = [moved[0].copy(), moved[1].copy(), moved[2].copy()]
        for c in self.cameras:
            if getattr(c, 'R', None) is None or getattr(c, 't', None) is None:
                continue
            Rc = np.asarray(c.R, dtype=np.float64)
            tc = np.ravel(np.asarray(c.t, dtype=np.float64))
            Rn = Rc @ R.T
            c.R, c.t = Rn, s * tc - Rn @ T
            if c.c is not None:
                c.c = s * (R @ np.ravel(np.asarray(c.c, dtype=np.float64))) + T
            if c.K is not None:
                c.compose()
        if isinstance(self.traj, np.ndarray) and self.traj.ndim == 2 and self.traj.shape[0] == 4 and self.traj.shape[1]:
            self.traj = np.vstack((self.traj[0], s * (R @ self.traj[1:]) + T[:, None]))
            if getattr(self, 'traj_sigma', None) is not None:
                self.traj_sigma = s * np.asarray(self.traj_sigma)

    def align_to_position_priors(self):
        """The similarity (Umeyama) that takes the spline at the active priors' times onto their positions, applied to the scene
        (``apply_similarity``); returns (s, R, T, rms) with rms the residual of the fit.  Needs at least three active priors that are not
        collinear -- the second singular value of the centred positions above 1e-6 of the first -- else ValueError."""
        from scipy.interpolate import splev
        t, P = self._active_position_priors()
        if t.size < 3:
            raise ValueError('align_to_position_priors: %d active position priors, at least 3 are needed' % t.size)
        sv = np.linalg.svd(P - P.mean(axis=1, keepdims=True), compute_uv=False)
        if not sv[1] > 1e-6 * sv[0]:
            raise ValueError('align_to_position_priors: the active position priors are collinear (singular values %s): the similarity is not determined' % (sv,))
        iv = np.asarray(self.spline['int'], dtype=np.float64)
        X = np.empty((3, t.size))
        for i in range(iv.shape[1]):
            m = (t >= iv[0, i]) & (t <= iv[1, i])
            if m.any():
                X[:, m] = np.asarray(splev(t[m], self.spline['tck'][i]))
        s, R, T = umeyama_similarity(X, P)
        rms = float(np.sqrt(np.mean(np.sum((s * (R @ X) + T[:, None] - P) ** 2, axis=0))))
        self.apply_similarity(s, R, T)
        return s, R, T, rms

    def ba_covariance_enabled(self):
        """settings['ba_covariance'] validated (a bool; absent = False): host only."""
        return _settings.flag(_settings.as_dict(self.settings), 'ba_covariance')

    def ba_kinematics_enabled(self):
        """settings['ba_kinematics'] validated (a bool; absent = False): host only."""
        return _settings.flag(_settings.as_dict(self.settings), 'ba_kinematics')

    def ba_detection_covariance_enabled(self):
        """settings['ba_detection_covariance'] validated (a bool; absent = False): host only."""
        return _settings.flag(_settings.as_dict(self.settings), 'ba_detection_covariance')

    def ba_register_enabled(self):
        """settings['ba_register'] validated (a bool; absent = False): host only.  True: the incremental loop calls ``register_camera`` on every new camera."""
        return _settings.flag(_settings.as_dict(self.settings), 'ba_register')

    def ba_register_beta_search(self):
        """settings['ba_register_beta_search'] validated: absent / None -> None, else (half_width, step) in frames, finite, half_width >= 0, step > 0.  Host only."""
        return _settings.register_beta_search(_settings.as_dict(self.settings))

    @staticmethod
    def register_rank(status, inliers, cost, ks):
        """The order in which ``register_camera`` prefers the starts of one call: the ones that started (status >= 0) only; most inliers
        first, then the lowest cost, then the smallest |k| (the start nearest the camera's own beta), then the lower index.  A list of
        indices, empty when no problem started.  Host only."""
        started = [b for b in range(len(status)) if int(status[b]) >= 0]
        return sorted(started, key=lambda b: (-int(inliers[b]), float(cost[b]), abs(int(ks[b])), b))

    def register_camera(self, cam_id, beta_search=None, hold=('K', 'd'), rs=False, rs_bounds=False, thres=None, max_nfev=50, keep_start=True):
        """Adjust ONE camera -- alpha, beta, rs and its pose (and K, d under ``opt_calib``) -- against the trajectory as it stands
        (``mvus_ba_register_cameras``): ``self.spline`` and every other camera are left alone.  The camera needs a pose (``get_camera_pose``).
        ``hold``: names of ``ba_freeze`` (alpha beta rs R t K d; K, d only exist under ``opt_calib``) kept where they are.
        ``beta_search = (half_width, step)`` in frames: the starts ``beta + k step``, ``|k step| <= half_width``, all solved in ONE call;
        the winner has the most inliers at ``thres`` (default ``settings['thres_outlier']``), then the lowest cost, then the smallest
        ``|k|``.  ``Scene.ba_loss()`` is in force.  Writes alpha, beta, rs, R, t (K, d when free) back and returns the namespace of
        ``BAHandle.register_cameras`` plus ``chosen`` (the winning index) and ``starts``.
        ``keep_start`` (default on; off = the winner is always written back): the camera as it came in is scored the same way (one more
        evaluation: ``start_inliers``), and a winner with FEWER inliers at ``thres`` than that is NOT written back -- ``kept_start`` says
        so, and the call prints it.  The camera's detections have not been through ``remove_outliers``: least squares under the linear
        loss gives way to gross outliers that PnP + RANSAC ignored (a robust ``ba_loss`` is the remedy, and then the winner is kept)."""
        cam_id = int(cam_id)
        st = _settings.as_dict(self.settings)
        if self.ba_landmarks() is not None:          # (the setting is on AND the scene holds landmarks and clicks)
            from .. import ba as _ba
            raise _ba.UnsupportedBySolver("register_camera: settings['ba_landmarks'] is on -- the per-camera problem holds no landmark rows and "
                                          "would drop exactly the ones that involve this camera")
        calib = bool(st.get('opt_calib', False))
        hold = tuple(hold) if hold is not None else ()
        for name in hold:
            if not isinstance(name, str) or name not in self.FREEZE_NAMES:
                raise ValueError('register_camera: unknown name %r in hold (one of %s)' % (name, list(self.FREEZE_NAMES)))
        if beta_search is not None:
            if len(beta_search) != 2 or not (np.isfinite(beta_search[0]) and np.isfinite(beta_search[1]) and beta_search[0] >= 0 and beta_search[1] > 0):
                raise ValueError('register_camera: beta_search must be (half_width, step) in frames with half_width >= 0 and step > 0, not %r' % (beta_search,))
        cam = self.cameras[cam_id]
        if getattr(cam, 'R', None) is None or getattr(cam, 't', None) is None:
            raise ValueError('register_camera: camera %d has no pose yet (get_camera_pose first)' % cam_id)
        if not getattr(self, 'spline', None) or not self.spline.get('tck'):
            raise ValueError('register_camera: the scene has no trajectory spline')
        loss = self.ba_loss()
        self.alpha, self.beta, self.rs = (np.asarray(v, dtype=np.float64) for v in (self.alpha, self.beta, self.rs))
        prob = self._ba_problem([cam_id], rs=rs, rs_bounds=rs_bounds)
        x = self._pack(prob, [cam_id])
        lay = _problem.HeadLayout(calib)
        mask = np.zeros(lay.size, dtype=bool)
        for name in hold:                            # (K, d without opt_calib are not in x: held by construction)
            mask[lay.indices(0, name)] = True
        start = x[:lay.size].copy()[None, :]
        if beta_search is not None:
            kmax = int(np.floor(beta_search[0] / beta_search[1] + 1e-9))
            ks = np.arange(-kmax, kmax + 1)
            start = np.repeat(start, ks.size, axis=0)
            start[:, 1] += ks * float(beta_search[1])
        else:
            ks = np.zeros(1, dtype=np.int64)
        thres = float(st.get('thres_outlier', 0) if thres is None else thres)
        with self._handle(prob) as h:
            h.configure(loss=loss, frozen=mask)
            res = h.register_cameras(x, np.zeros(start.shape[0], dtype=np.int32), start=start, max_nfev=max_nfev, inlier_thres=thres)
            # the camera as it came in, scored the same way (one evaluation, nothing moves)
            came = h.register_cameras(x, [0], max_nfev=1, inlier_thres=thres) if (keep_start and thres > 0) else None
        order = self.register_rank(res.status, res.inliers, res.cost, ks)
        if not order:
            raise ValueError('register_camera: camera %d has too few detections on the trajectory for its %d free parameters' % (cam_id, int((~mask).sum())))
        best = int(order[0])
        res.chosen, res.starts = best, start
        # The camera's detections have not been through remove_outliers yet.  Under the linear loss a few gross outliers can pull the
        # least-squares estimate away from what PnP + RANSAC found (the rms falls, the typical error rises): a result that explains FEWER
        # detections within ``thres`` than the camera did as it came in is not written back.
        res.start_inliers = int(came.inliers[0]) if came is not None else None
        res.kept_start = bool(came is not None and res.start_inliers > int(res.inliers[best]))
        if res.kept_start:
            print('register_camera: camera %d keeps the state it came in with (%d inliers at %g px; the registered one has %d)'
                  % (cam_id, res.start_inliers, thres, int(res.inliers[best])))
            return res
        xb = x.copy()
        xb[:lay.size] = res.params[best]
        alpha, beta, rs_new, cam_states, _ = _problem.unpack_x(prob, xb)
        self.alpha[cam_id], self.beta[cam_id], self.rs[cam_id] = alpha[0], beta[0], rs_new[0]
        for name in ('K', 'd') if calib else ():     # (a held part keeps the object it has: no round trip through x)
            if name not in hold:
                setattr(cam, name, cam_states[0][name])
        for name in ('R', 't'):
            if name not in hold:
                setattr(cam, name, cam_states[0][name])
        cam.compose()
        self.detection_to_global(cam_id)
        return res

    def kinematics(self, t=None, fps=None, cov=None):
        """Velocity, acceleration, speed and distance flown along the trajectory splines at timestamps ``t`` (default: the stamps of
        ``spline_to_traj``, ``self.traj[0]``), differentiated on the spline itself (``mvus_spline_eval_der``, ``mvus_spline_length``) instead
        of differencing samples.  The spline parameter runs in frames of the reference camera; ``fps`` (default: that camera's) converts to
        per-second values: velocity x fps, acceleration x fps^2, covariance blocks by the matching products; ``fps=1`` keeps per-frame units.
        ``cov``: the dict ``ba_covariance`` returned, or its band [N, 4, 3, 3] -- then the 1-sigma of each (``mvus_spline_kin_cov_eval``); a
        band that does not fit the current splines raises ValueError.  Stores and returns a data-only dict:
          t, which (interval of each stamp, -1 outside: zeros / NaN there), fps,
          pos [3, nt], vel [3, nt], acc [3, nt], speed [nt] = |vel|,
          dist [nt] distance flown, continued over the intervals in order (an interval starts at the length of those before it; the gaps
          count nothing), length [S] of each interval,
          with ``cov``: state_cov [nt, 9, 9] of (pos, vel, acc), vel_std [nt, 3], acc_std [nt, 3], speed_std [nt] = sqrt(u^T Cov(vel) u),
          u = vel / speed (NaN where the speed is 0).
        The variance of ``dist`` needs covariances between control points further apart than the band holds; it is not given.
        The dict is stored as ``self.kinematics`` -- on the instance it takes this method's place, so a later evaluation of the same Scene
        goes through the class: ``Scene.kinematics(scene, ...)``."""
        from .. import spline as _spline
        tck, interval = self.spline['tck'], self.spline['int']
        ts = np.asarray(self.traj[0] if t is None else t, dtype=np.float64)
        fps = float(self.cameras[self.ref_cam].fps if fps is None else fps)
        device = self._device()
        D, which = _spline.evaluate_der(tck, interval, ts, nder=2, device=device)
        dist, _, length = _spline.path_length(tck, interval, ts, device=device)
        before = np.concatenate(([0.0], np.cumsum(length)[:-1]))
        dist = np.where(which >= 0, dist + before[np.maximum(which, 0)], 0.0)
        vel, acc = D[1] * fps, D[2] * fps ** 2
        out = {'t': ts.copy(), 'which': which, 'fps': fps, 'pos': D[0].copy(), 'vel': vel, 'acc': acc, 'speed': np.sqrt(np.sum(vel * vel, axis=0)),
               'dist': dist, 'length': length}
        if cov is not None:
            band = np.asarray(cov['band'] if isinstance(cov, dict) else cov, dtype=np.float64)
            state_cov, _ = _spline.kin_cov_evaluate(tck, interval, band, ts, nder=2, device=device)          # (checks the band's shape)
            unit = np.repeat([1.0, fps, fps ** 2], 3)
            state_cov = state_cov * np.outer(unit, unit)
            with np.errstate(invalid='ignore', divide='ignore'):
                sd = np.sqrt(np.einsum('tii->ti', state_cov))
                u = vel / out['speed']
                speed_std = np.sqrt(np.einsum('it,tij,jt->t', u, state_cov[:, 3:6, 3:6], u))
            out.update(state_cov=state_cov, vel_std=sd[:, 3:6].copy(), acc_std=sd[:, 6:9].copy(), speed_std=speed_std)
        self.kinematics = out
        return out

    def ba_param_names(self):
        """Names of the P parameters of one camera in x (Camera.P2vector order)."""
        return _problem.HeadLayout(self.settings['opt_calib']).names

    def ba_covariance(self, cams, t=None, sigma2=None, rs=False, motion_reg=False, motion_weights=1, rs_bounds=False):
        """Covariance of the BA estimate over the cameras ``cams`` at the scene's current state (``mvus_ba_covariance``): built on the
        handle the last BA left resident when it still describes that problem (else a new one), with the loss and the frozen mask of the
        settings.  The gauge must be fixed (``ba_gauge: 'anchor'`` / ``ba_freeze``), else ValueError.  ``t``: timestamps of the position
        covariance (default: the stamps of ``spline_to_traj``, ``self.traj[0]``); ``sigma2``: the variance factor (default: a posteriori).
        Stores and returns a data-only dict:
          cams, param_names, sigma2, dof,
          cam_cov [CB, CB] in the order of the head of x (alpha(C), beta(C), rs(C), P per camera), estimated_cam bool[CB],
          cam_std {camera: {'alpha', 'beta', 'rs', <parameter names>}: standard deviation},
          band [N, 4, 3, 3] blocks (p, p + w) of the control points' covariance,
          t, pos_cov [len(t), 3, 3], pos_std [len(t), 3] (1-sigma per axis; NaN outside every interval)."""
        cams = list(cams)
        h, prob, x = self._covariance_handle(cams, rs, motion_reg, motion_weights, rs_bounds)
        return self._store_covariance(h.covariance(x, sigma2=sigma2), cams, prob, t)

    def _covariance_handle(self, cams, rs, motion_reg, motion_weights, rs_bounds):
        """(handle, problem, x) of the covariance calls: the handle the last BA left resident when it still describes the problem over
        ``cams`` (else a new one), with the loss, the frozen mask and the position priors of the settings in force."""
        self.alpha, self.beta, self.rs = (np.asarray(v, dtype=np.float64) for v in (self.alpha, self.beta, self.rs))
        prob = self._ba_problem(cams, rs=rs, motion_reg=motion_reg, motion_weights=motion_weights, rs_bounds=rs_bounds)
        x = self._pack(prob, cams)
        self.ba_mode()                             # validates the ba_* settings
        return self._configured_handle(prob, cams), prob, x

    def _store_covariance(self, cv, cams, prob, t):
        """``self.covariance`` from the namespace of ``BAHandle.covariance`` / ``detection_covariance`` (the dict ``ba_covariance`` documents)."""
        from .. import spline as _spline
        lay = _problem.HeadLayout(prob.opt_calib, len(cams))
        sd = np.sqrt(np.diag(cv.cam))
        cam_std = {int(cam): {name: float(sd[lay.index(k, name)]) for name in list(lay.HEAD) + lay.names} for k, cam in enumerate(cams)}
        ts = np.asarray(self.traj[0] if t is None else t, dtype=np.float64)
        pos_cov, _ = _spline.cov_evaluate(self.spline['tck'], self.spline['int'], cv.band, ts, device=self._device())
        with np.errstate(invalid='ignore'):
            pos_std = np.sqrt(np.einsum('tii->ti', pos_cov))
        self.covariance = {'cams': [int(c) for c in cams], 'param_names': lay.names, 'sigma2': float(cv.sigma2), 'dof': int(cv.dof),
                           'cam_cov': cv.cam, 'estimated_cam': cv.estimated[:lay.size].copy(), 'cam_std': cam_std, 'band': cv.band,
                           't': ts.copy(), 'pos_cov': pos_cov, 'pos_std': pos_std}
        return self.covariance

    def ba_detection_covariance(self, cams, sigma2=None, rs=False, motion_reg=False, motion_weights=1, rs_bounds=False, with_covariance=False, t=None):
        """The covariance of the BA estimate over ``cams`` carried back to the image plane (``mvus_ba_detection_covariance``), at the
        scene's current state and built as ``ba_covariance`` is (resident handle, loss, frozen mask and priors of the settings; the gauge
        must be fixed).  Stores (``self.detection_covariance``) and returns a data-only dict:
          cams, sigma2, dof,
          per_cam {camera id: {frame [M_c], e [2, M_c] signed residual (u, v) in px, predicted minus observed,
                               cov [3, M_c] = (P_uu, P_uv, P_vv) of the fitted detection in image axes, t2 [M_c] squared studentised residual,
                               semi_major, semi_minor [M_c] 1-sigma half axes in px, angle [M_c] of the major axis from +u towards +v (rad)}}
        in the order of the camera's detections in the BA problem.  Detections outside every interval of the spline have NaN in cov, t2 and
        the ellipse, 0 in e.  With ``opt_calib`` and ``undist_points`` the observed point is undistorted with the unknown intrinsics: cov is
        then the covariance of the fitted part of the residual in the undistorted frame, not of a bare projection.  t2 is chi^2 with 2
        degrees of freedom under the linear loss only (a robust loss: the Gauss-Newton approximation).
        ``with_covariance``: the same call also stores ``self.covariance`` exactly as ``ba_covariance(cams, t=t, ...)`` would -- one run of
        the chain serves both."""
        cams = list(cams)
        h, prob, x = self._covariance_handle(cams, rs, motion_reg, motion_weights, rs_bounds)
        dc = h.detection_covariance(x, sigma2=sigma2)
        if with_covariance:
            self._store_covariance(dc, cams, prob, t)
        off = np.asarray(prob.det_offsets, dtype=np.int64)
        per_cam = {}
        for k, cam in enumerate(cams):
            seg = slice(int(off[k]), int(off[k + 1]))
            cov = dc.cov[:, seg].copy()
            major, minor, angle = ellipse_2x2(cov)
            per_cam[int(cam)] = {'frame': np.array(prob.frame[seg], dtype=np.float64), 'e': dc.e[:, seg].copy(), 'cov': cov, 't2': dc.t2[seg].copy(),
                                 'semi_major': major, 'semi_minor': minor, 'angle': angle}
        self.detection_covariance = {'cams': [int(c) for c in cams], 'sigma2': float(dc.sigma2), 'dof': int(dc.dof), 'per_cam': per_cam}
        return self.detection_covariance

    @staticmethod
    def studentised_flags(result, p=0.999):
        """{camera id: bool [M_c]} of the detections whose squared studentised residual exceeds the chi^2 quantile with 2 degrees of freedom,
        ``t2 > -2 ln(1 - p)``; NaN is never flagged.  ``result``: the dict ``ba_detection_covariance`` returned.  It only flags: nothing is
        cut (``remove_outliers`` stays the fixed-threshold test it is)."""
        thr = chi2_2_quantile(p)
        with np.errstate(invalid='ignore'):
            return {cam: np.asarray(d['t2']) > thr for cam, d in result['per_cam'].items()}

    FREEZE_NAMES = _settings.FREEZE_NAMES
    FREEZE_NAMES = ('alpha', 'beta', 'rs', 'R', 't', 'K', 'd')

    def ba_freeze(self):
        """({camera index: names}, gauge) of settings['ba_freeze'] / settings['ba_gauge'], validated: host only, raises ValueError before
        any GPU call.  Without the keys: ({}, 'free') -- the reference's problem."""
        return _settings.freeze(_settings.as_dict(self.settings))

    def ba_frozen_mask(self, cams):
        """bool[C * (3 + P)] over the camera-side head of x (pack_x order: alpha(C), beta(C), rs(C), P parameters per camera) for a BA over
        ``cams``: what settings['ba_freeze'] names, plus -- settings['ba_gauge'] = 'anchor' -- the trivial gauge: the six pose parameters of
        cams[0] and component k = argmax |R_1 (C_0 - C_1)| of the translation of cams[1].  That vector is d t_1 / d s of a scaling of the
        scene about the first camera's centre C_0 (t_1 = -R_1 C_1, C_1 -> C_0 + s (C_1 - C_0)): with the first pose held the similarity has
        only that scaling left, and holding a component it moves removes it.  Pure host function; no GPU call."""
        freeze, gauge = self.ba_freeze()
        cams = list(cams)
        C = len(cams)
        lay = _problem.HeadLayout(bool(_settings.as_dict(self.settings).get('opt_calib', False)), C)
        mask = np.zeros(lay.size, dtype=bool)
        for k, cam in enumerate(cams):
            for name in freeze.get(int(cam), ()):
                mask[lay.indices(k, name)] = True
        if gauge == 'anchor' and C >= 1:
            mask[lay.indices(0, 'R') + lay.indices(0, 't')] = True
            if C >= 2:
                c0, c1 = self.cameras[cams[0]], self.cameras[cams[1]]
                R0, R1 = np.asarray(c0.R, dtype=np.float64), np.asarray(c1.R, dtype=np.float64)
                centre0 = -R0.T @ np.ravel(np.asarray(c0.t, dtype=np.float64))
                centre1 = -R1.T @ np.ravel(np.asarray(c1.t, dtype=np.float64))
                comp = int(np.argmax(np.abs(R1 @ (centre0 - centre1))))
                mask[lay.indices(1, 't')[comp]] = True
        return mask

    def ba_loss(self):
        """(MVUS_LOSS_* code, f_scale) of settings['ba_loss'] / settings['ba_f_scale']: the ``loss`` and ``f_scale`` arguments of scipy's least_squares, which
        the reference never passes ('linear', 1.0 -- also the defaults here).  A loss other than 'linear' needs ``ba_solver: 'lm'`` with the analytic Jacobian."""
        return _settings.loss(_settings.as_dict(self.settings))

    def remove_outliers(self, cams, thres=30, verbose=False):
        """Drop detections whose reprojection error is >= thres (common.py:700-717); the mask is computed by
        ``mvus_ba_outlier_mask``."""
        if not thres:
            return
        cams = list(cams)
        self.detection_to_global(cams)
        # in place on the GPU only if the resident handle is over exactly these cameras AND still describes the current
        # scene (detections, knots, intervals, fixed K/d, undist_points): the reference always evaluates current state
        h = self._resident_for(cams) if self._ba_key == tuple(cams) else None
        if h is not None:
            # the detections of the last BA are still on the GPU: filter them there (mvus_ba_remove_outliers)
            prob_old = h.prob
            x = self._pack(prob_old, cams)
            f = h.residual(x) if verbose else None
            keep = h.remove_outliers(x, thres)
            prob = prob_old
        else:
            prob = self._ba_problem(cams)
            with self._handle(prob) as tmp:
                x = self._pack(prob, cams)
                keep = tmp.outlier_mask(x, thres)
                f = tmp.residual(x) if verbose else None
        for k, i in enumerate(cams):
            a, b = int(prob.det_offsets[k]), int(prob.det_offsets[k + 1])
            if verbose:
                ex, ey = f[2 * a:2 * a + (b - a)], f[2 * a + (b - a):2 * b]
                print('{} out of {} detections are removed for camera {}'.format(int((~keep[a:b]).sum()),
                                                                                  int(((ex != 0) | (ey != 0)).sum()), i))
            self.detections[i] = self.detections[i][:, keep[a:b]]
            self.detection_to_global(i)

    def triangulate(self, cam_id, cams, factor_t2s, factor_s2t=0.02, thres=0, refit=True, verbose=0):
        """Triangulate the detections of camera ``cam_id`` that lie outside the existing spline against the (already
        processed) cameras ``cams`` and append them to the trajectory (common.py:754-815).  Same steps as the reference;
        the per-point linear triangulation and both reprojection distances come from one GPU kernel
        (``mvus_triangulate``) instead of a Python loop of 4x4 SVDs."""
        from . import epipolar as ep
        new_cam = self.cameras[cam_id]
        assert new_cam.P is not None, 'The camera pose must be computed first'
        covered = self.spline['int']
        device = self._device()
        self.detection_to_global(cam_id)
        mine = self.detections_global[cam_id]
        mine = mine[:, ~np.asarray(util.sampling(mine, covered)[1], dtype=bool)]      # only what the spline does not cover yet

        def against(other):
            """[t; X] of this camera's uncovered detections paired in time with camera ``other`` (one GPU launch per pair of cameras)."""
            self.detection_to_global(other)
            try:
                a, b = util.match_overlap(mine, self.detections_global[other])
            except Exception:                       # no temporal overlap with this camera (the reference's bare except)
                return None
            if weighted is None:
                Xh, d_new, d_other = ep.triangulate_with_errors(a[1:], b[1:], new_cam.P, self.cameras[other].P, device=device)
                sig = None
            else:                                   # the same points and distances, with the 1-sigma of every point
                Xh, cov, d_new, d_other = ep.triangulate_with_cov(a[1:], b[1:], new_cam.P, self.cameras[other].P, sigma1=weighted[1][cam_id],
                                                                   sigma2=weighted[1][other], device=device)
                sig = self.sigma_from_cov(cov)
            pts = np.vstack((a[0], Xh[:3]))
            if thres:
                ok = (d_new < thres) & (d_other < thres)
                if verbose:
                    print('{} out of {} points are triangulated'.format(sum(ok), len(d_new)))
                pts = pts[:, ok]
                sig = sig if sig is None else sig[ok]
            if verbose:
                print('{} points are triangulated into the 3D spline'.format(pts.shape[1]))
            return pts, sig

        weighted = self.traj_weights()
        found = [r for r in map(against, cams) if r is not None]
        X_new = np.hstack([np.empty([4, 0])] + [pts for pts, _ in found])
        assert not np.any(util.sampling(X_new, covered)[1]), 'Points should not be triangulated into the existing part of the 3D spline'
        self.spline_to_traj(sampling_rate=factor_s2t)
        merged = np.hstack((self.traj, X_new))
        if weighted is None:
            self.traj = merged[:, np.unique(merged[0], return_index=True)[1]]      # time ordered, one sample per timestamp (the first)
        else:
            # the samples of the spline come out of a BA: as good as the best raw pair; of several points at one timestamp the one with the
            # smallest sigma stays (NaN last, then the first) where the reference keeps whichever comes first
            sig_new = np.concatenate([np.empty(0)] + [sig for _, sig in found])
            good = sig_new[np.isfinite(sig_new) & (sig_new > 0)]
            sigma = np.concatenate((np.full(self.traj.shape[1], good.min() if good.size else 1.0), sig_new))
            key = np.where(np.isfinite(sigma) & (sigma > 0), sigma, np.inf)
            order = np.lexsort((np.arange(key.size), key, merged[0]))
            first = order[np.unique(merged[0][order], return_index=True)[1]]
            self.traj, self.traj_sigma = merged[:, first], sigma[first]
        if refit:
            self.traj_to_spline(smooth_factor=factor_t2s)
        return X_new

    def get_camera_pose(self, cam_id, error=8, verbose=0):
        """Absolute pose of camera ``cam_id`` from the trajectory (reference common.py:719-750): the spline points at the
        camera's detection timestamps (GPU: ``mvus_spline_eval``) against the raw detections, PnP + RANSAC on the GPU
        (``mvus_pnp_ransac`` in place of ``cv2.solvePnPRansac``, reprojectionError = ``error``); sets R, t, P of the camera."""
        from .. import spline as _spline
        from .pnp import solve_pnp_ransac
        tck, interval = self.spline['tck'], self.spline['int']
        device = self._device()
        self.detection_to_global(cam_id)
        det = self.detections_global[cam_id]
        _, idx = util.sampling(det, interval, belong=True)
        detect, point_3D = np.empty([3, 0]), np.empty([3, 0])
        for i in range(interval.shape[1]):                       # the reference's order: interval by interval
            part = det[:, idx == i + 1]
            if part.size:
                X, which = _spline.evaluate([tck[i]], interval[:, i:i + 1], part[0], device=device)
                detect = np.hstack((detect, part))
                point_3D = np.hstack((point_3D, X))
        N = point_3D.shape[1]
        cam = self.cameras[cam_id]
        retval, rvec, tvec, inliers = solve_pnp_ransac(point_3D.T, detect[1:].T, cam.K, cam.d, reprojectionError=error, device=device)
        if not retval:
            raise ValueError('get_camera_pose: no pose is supported by six trajectory points within %g px' % error)
        cam.R = _rodrigues(np.ravel(rvec))
        cam.t = np.ravel(tvec)
        cam.compose()
        if verbose:
            print('{} out of {} points are inliers for PnP'.format(inliers.shape[0], N))

    def select_most_overlap(self, init=False):
        """The initial pair of cameras or the next camera with the largest temporal overlap (reference common.py:851-884): host
        bookkeeping over the detection timestamps; the resampled trajectory of the second branch comes from the GPU."""
        if not self.find_order:
            return
        self.detection_to_global()
        overlap_max = 0
        if init:
            init_pair = None
            for i in range(self.numCam - 1):
                for j in range(i + 1, self.numCam):
                    x, _ = util.match_overlap(self.detections_global[i], self.detections_global[j])
                    overlap = x.shape[1] / self.cameras[i].fps
                    if overlap > overlap_max:
                        overlap_max, init_pair = overlap, [i, j]
            self.sequence = init_pair
        else:
            traj = self.spline_to_traj()
            next_cam = None
            for i in [c for c in range(self.numCam) if self.cameras[c].P is None]:
                interval = util.find_intervals(self.detections_global[i][0])
                overlap = util.sampling(traj[0], interval)
                overlap = overlap[0] if isinstance(overlap, tuple) else overlap
                if len(overlap) > overlap_max:
                    overlap_max, next_cam = len(overlap), i
            self.sequence.append(next_cam)

    # ---- outside the hot path -----------------------------------------------------------------------
    def _out_of_scope(self, *a, **k):
        raise NotImplementedError('outside the BA hot path this package accelerates (SURVEY.md section 2); '
                                  'use the reference implementation for initialisation / synchronisation search')

    plot_reprojection = _out_of_scope

    def init_traj(self, error=10, inlier_only=False):
        """The first two cameras and the first trajectory (reference common.py:178-221): the pair with the most overlap, F by
        RANSAC on their matched detections (``mvus_fundamental_ransac``), E = K2^T F K1, the optimal correction of the pairs
        (``mvus_correct_matches``), the pose of the second camera and the points from E (``mvus_pose_from_essential``).  With
        ``inlier_only=False`` every pair is kept, as in the reference.  A scene with fewer than two cameras has no pair to start
        from: single-view reconstruction is not implemented (the reference fails there with a TypeError on ``sequence``)."""
        from . import epipolar as ep
        if len(self.cameras) < 2 or self.numCam < 2:
            raise NotImplementedError('init_traj: two-view initialisation needs at least two cameras with detections (this scene has '
                                      '%d); single-view reconstruction is not implemented' % min(len(self.cameras), self.numCam))
        device = self._device()
        self.select_most_overlap(init=True)
        t1, t2 = self.sequence[0], self.sequence[1]
        K1, K2 = self.cameras[t1].K, self.cameras[t2].K
        if self.cameras[t1].fps > self.cameras[t2].fps:          # the denser camera first in match_overlap
            d1, d2 = util.match_overlap(self.detections_global[t1], self.detections_global[t2])
        else:
            d2, d1 = util.match_overlap(self.detections_global[t2], self.detections_global[t1])
        F, inlier = ep.computeFundamentalMat(d1[1:], d2[1:], error=error, device=device)
        E = K2.T @ F @ K1
        if not inlier_only:
            inlier = np.ones(len(inlier))
        keep = inlier == 1
        m1, m2 = ep.correct_matches(F, d1[1:, keep], d2[1:, keep], device=device)
        x1, x2 = util.homogeneous(m1), util.homogeneous(m2)
        mask = np.logical_not(np.isnan(x1[0]))
        x1, x2 = x1[:, mask], x2[:, mask]
        X, P = ep.triangulate_from_E(E, K1, K2, x1, x2, device=device)
        self.traj = np.vstack((d1[0][keep][mask], X[:-1]))
        self.traj_sigma = None
        self.cameras[t1].P = K1 @ np.hstack((np.eye(3), np.zeros((3, 1))))
        self.cameras[t2].P = K2 @ P
        weighted = self.traj_weights()
        if weighted is not None:                  # the 1-sigma of every point, from the corrected matches and the two P just set
            _, cov, _, _ = ep.triangulate_with_cov(x1[:2], x2[:2], self.cameras[t1].P, self.cameras[t2].P, sigma1=weighted[1][t1], sigma2=weighted[1][t2],
                                                   device=device)
            self.traj_sigma = self.sigma_from_cov(cov)
        self.cameras[t1].decompose()
        self.cameras[t2].decompose()

    def error_motion(self, cams, mode='dist', norm=False, motion_weights=0, motion_reg=False, motion_prior=False):
        """The motion-regularisation rows of the BA residual (reference common.py:362-424 with ``motion_reg=True``): one value
        per sample of ``spline_to_traj()`` (unit steps of the reference camera's frame clock), 'F' or 'KE' by
        ``settings['motion_type']``, zero at the first/last samples of an interval.  Evaluated by ``k_motion`` on the GPU (the
        rows ``error_BA`` appends, common.py:462-467).  ``motion_prior=True`` is the reference's dead branch."""
        if motion_prior:
            raise NotImplementedError('motion_prior=True is dead code in the reference pipeline (SURVEY.md section 2)')
        if not motion_reg:
            raise ValueError('error_motion: motion_reg=True is the only live mode (the reference returns an unbound name otherwise)')
        cams = [int(cams)] if isinstance(cams, (int, np.integer)) else list(cams)
        self.detection_to_global(cams)
        self.spline_to_traj()
        prob = self._ba_problem(cams[:1], motion_reg=True, motion_weights=motion_weights)
        with self._handle(prob) as tmp:
            f = tmp.residual(self._pack(prob, cams[:1]))
        out = f[2 * prob.M:]
        assert out.size == self.traj.shape[1], 'motion rows and trajectory samples do not correspond'
        return out


def create_scene(path_input):
    """Build a Scene from the reference's JSON config (common.py:1171-1230): sections
    'necessary inputs', 'optional inputs', 'settings'."""
    with open(path_input, 'r') as fh:
        config = json.load(fh)
    flight = Scene()
    flight.settings = config['settings']
    paths = config['necessary inputs']['path_detections']
    flight.numCam = len(paths)
    for p in paths:
        det = np.loadtxt(p, usecols=(2, 0, 1))[:flight.settings['num_detections']].T
        flight.addDetection(det)
    for p in config['necessary inputs']['path_cameras']:
        try:
            with open(p, 'r') as fh:
                cam = json.load(fh)
        except Exception:
            raise Exception('Wrong input of camera')
        d = list(cam['distCoeff'])
        if len(d) == 4:
            d.append(0)
        flight.addCamera(Camera(K=np.asarray(cam['K-matrix'], dtype=np.float64), d=np.asarray(d, dtype=np.float64),
                                fps=cam['fps'], resolution=cam['resolution']))
    flight.ref_cam = config['settings']['ref_cam']
    flight.sequence = config['settings']['camera_sequence']
    flight.find_order = False if len(flight.sequence) else True
    flight.cf = np.asarray(config['necessary inputs']['corresponding_frames'], dtype=np.float64)
    init_rs = config['settings']['init_rs'] if config['settings']['rolling_shutter'] else 0
    if isinstance(init_rs, list):
        assert len(init_rs) == flight.numCam, 'the number of initial rolling shutter values must equal the number of cameras'
        flight.rs = np.asarray(init_rs, dtype=np.float64)
    else:
        flight.rs = np.full(flight.numCam, float(init_rs))
    if 'optional inputs' in config and 'ground_truth' in config['optional inputs']:
        flight.gt = config['optional inputs']['ground_truth']
    opt = config.get('optional inputs', {})
    if opt.get('path_position_priors'):
        # surveyed positions (GPS / RTK log): t x y z [sigma_x sigma_y sigma_z] per line, t on the reference camera's frame clock
        flight.position_priors = load_position_priors(opt['path_position_priors'], opt.get('position_prior_sigma'))
    flight.ba_position_priors()              # (settings['ba_position_priors'] validated here, before any GPU work)
    if opt.get('path_landmarks') and opt.get('path_landmark_observations'):
        # surveyed static points: id x y z per line, and their clicks: camera id u v [sigma_u sigma_v] per line
        flight.landmarks, flight.landmark_observations = load_landmarks(opt['path_landmarks'], opt['path_landmark_observations'], opt.get('landmark_sigma'))
    flight.ba_landmarks()                    # (settings['ba_landmarks'] likewise)
    flight.traj_weights()                    # (settings['traj_weights'], ['traj_sigma_px'], ['traj_weight_floor'] likewise)
    print('Input data are loaded successfully, a scene is created.\n')
    return flight
