"""Temporal synchronisation search of the reference's ``reconstruction/synchronization.py``: ``sync_bf`` (synchronization.py:133-178),
the brute-force search that ``Scene.time_shift`` runs when the corresponding frames are not exact (``cf_exact: false``,
``sync_method: 'bf'``).  Every candidate time shift is scored by the inliers of a RANSAC fundamental matrix over the detections
the two cameras share at that shift; the reference runs one ``cv2.findFundamentalMat`` per candidate, here each of the two stages
(20 coarse, 20 fine candidates) is ONE batched call of ``mvus_fundamental_ransac`` (epipolar.fundamental_ransac_batch).
``sync_iter_gpu`` (``sync_method: 'iter_gpu'``) is the reference's iterative search ``sync_iter`` (synchronization.py:13-130, Albl et al.): a
generalised eigenproblem per sample of nine detections, every shift it yields scored against all detections of the other camera; the
hypotheses, the fundamental matrices and the models x samples scoring run on the GPU (csrc/sync_iter.hip.h) through one
``mvus_sync_iter_round`` per round, the preprocessing, the two interpolating splines and the outer loop on the host.  The reference's own
name ``sync_iter`` / ``sync_method: 'iter'`` is still refused (tests/test_epipolar.py and tests/test_gpu_init_pipeline.py hold that)."""
import ctypes

import numpy as np

from .. import _lib
from ..tools import util
from . import epipolar as ep


def sync_iter(*args, **kwargs):
    raise NotImplementedError('sync_iter (synchronization.py:9-130) is not implemented; use sync_method "bf"')


def _candidate_pairs(detect1_temp, detect2, betas):
    """match_overlap pairs of every shifted candidate; None where the candidate has fewer than 8 common samples (the reference's
    cv2 call would raise there; such a shift cannot win)."""
    out = []
    for beta in betas:
        detect2_temp = np.vstack((detect2[0] + beta, detect2[1:]))
        try:
            pts1, pts2 = util.match_overlap(detect1_temp, detect2_temp)
        except Exception:
            out.append(None)
            continue
        out.append((pts1[1:], pts2[1:]) if pts1.shape[1] >= 8 else None)
    return out


def _search(detect1_temp, detect2, betas, thres=8, device=0):
    """The reference's inner ``search``: the shift with the most RANSAC inliers (strict >, starting from 0)."""
    pairs = _candidate_pairs(detect1_temp, detect2, betas)
    live = [k for k, p in enumerate(pairs) if p is not None]
    counts = np.zeros(len(betas), dtype=np.int64)
    if live:
        res, _ = ep.fundamental_ransac_batch([pairs[k] for k in live], error=thres, device=device)
        for k, (_, mask) in zip(live, res):
            counts[k] = int(mask.sum())
    max_inlier, beta_est = 0, 0
    for beta, inlier in zip(betas, counts):
        if inlier > max_inlier:
            max_inlier, beta_est = int(inlier), beta
    return beta_est, max_inlier


def sync_bf(fps1, fps2, detect1, detect2, frame1, frame2, r=10, device=0):
    """synchronization.py:133-178: time shift of camera 2 against camera 1 by a two-stage grid search within +-r seconds of the
    prior given by the corresponding frames ``frame1``, ``frame2``; detect1, detect2 are raw detections (frame, x, y).  Returns
    (beta, overlap in seconds) like the reference: beta in camera-1 frames."""
    alpha = fps1 / fps2
    detect1_temp = np.vstack((detect1[0] / alpha, detect1[1:]))
    beta_prior = frame1 / alpha - frame2
    beta_coarse = np.arange(beta_prior - r * fps2, beta_prior + r * fps2, fps2)
    beta_est, _ = _search(detect1_temp, detect2, beta_coarse, device=device)
    beta_fine = np.arange(beta_est - fps2 / 2, beta_est + fps2 / 2, fps2 / 20)
    beta_est, num_inlier = _search(detect1_temp, detect2, beta_fine, device=device)
    return beta_est * alpha, num_inlier / fps1


class SyncIterSession:
    """One camera pair on the device (``mvus_sync_iter_open``): camera 1's detections ``d1`` (t, x, y with t already divided by alpha) and
    its interpolating spline, camera 2's raw detections ``d2`` (frame, x, y), its spline on its own unshifted timeline and its contiguous
    intervals (``util.find_intervals``, gap 5).  ``t2`` overrides the timestamps the samples are drawn from (tests).  A context manager."""

    def __init__(self, d1, d2, t2=None, intervals=None, device=0):
        from scipy import interpolate
        self._h = ctypes.c_void_p()
        self._lib = _lib.load()
        d1 = np.ascontiguousarray(np.asarray(d1, dtype=np.float64)[:3])
        d2 = np.asarray(d2, dtype=np.float64)[:3]
        tck1, _ = interpolate.splprep(d1[1:], u=d1[0], s=0, k=3)
        tck2, _ = interpolate.splprep(d2[1:], u=d2[0], s=0, k=3)
        self.tck1, self.tck2 = tck1, tck2
        k1, c1 = np.ascontiguousarray(tck1[0], dtype=np.float64), np.ascontiguousarray(np.vstack(tck1[1]), dtype=np.float64)
        k2, c2 = np.ascontiguousarray(tck2[0], dtype=np.float64), np.ascontiguousarray(np.vstack(tck2[1]), dtype=np.float64)
        iv = util.find_intervals(d2[0]) if intervals is None else np.asarray(intervals, dtype=np.float64)
        self.intervals = iv
        ivp = np.ascontiguousarray(iv.T, dtype=np.float64)                      # [start, end) pairs
        self.t2 = np.ascontiguousarray(d2[0] if t2 is None else t2, dtype=np.float64)
        self.d1 = d1
        self.num_sample = min(d1.shape[1], self.t2.size)
        rc = self._lib.mvus_sync_iter_open(int(device), c1.shape[1], _lib.dptr(k1), _lib.dptr(c1), c2.shape[1], _lib.dptr(k2), _lib.dptr(c2),
                                           ivp.shape[0], _lib.dptr(ivp), d1.shape[1], _lib.dptr(d1), self.t2.size, _lib.dptr(self.t2),
                                           ctypes.byref(self._h))
        if rc != 0:
            self._h = ctypes.c_void_p()
            ep._raise(self._lib, rc, 'mvus_sync_iter_open')

    def close(self):
        if self._h:
            self._lib.mvus_sync_iter_close(self._h)
            self._h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        self.close()


def _round(session, shift, d, H, threshold, seed, rnd):
    """Both of the reference's ``ransac(d)`` / ``ransac(-d)`` calls of one round: [(beta_temp, ratio, inliers, overlap)] * 2."""
    out = np.zeros(8)
    rc = session._lib.mvus_sync_iter_round(session._h, float(shift), int(d), int(H), float(threshold), int(seed), int(rnd), _lib.dptr(out))
    if rc != 0:
        ep._raise(session._lib, rc, 'mvus_sync_iter_round')
    return [(out[0], out[1], int(out[2]), int(out[3])), (out[4], out[5], int(out[6]), int(out[7]))]


def sync_iter_models(session, shift, d, idx, threshold=10):
    """The inspection hook ``mvus_sync_iter_models``: hypotheses with the explicit sample indices ``idx`` (H x 9, into camera 2's
    timestamps) and the signed step ``d``.  Returns (betas H x 6, valid H x 6 bool, F H x 6 x 3 x 3, counts H x 6 x 2 [inliers, overlap])."""
    idx = np.ascontiguousarray(idx, dtype=np.int64)
    if idx.ndim != 2 or idx.shape[1] != 9:
        raise ValueError('idx must be H x 9')
    H = idx.shape[0]
    betas, valid = np.zeros((H, 6)), np.zeros((H, 6), dtype=np.uint8)
    F, counts = np.zeros((H, 6, 3, 3)), np.zeros((H, 6, 2), dtype=np.int32)
    rc = session._lib.mvus_sync_iter_models(session._h, float(shift), int(d), H, idx.ctypes.data_as(_lib.c_int64_p), float(threshold), _lib.dptr(betas),
                                            valid.ctypes.data_as(_lib.c_uint8_p), _lib.dptr(F), counts.ctypes.data_as(_lib.c_int32_p))
    if rc != 0:
        ep._raise(session._lib, rc, 'mvus_sync_iter_models')
    return betas, valid.astype(bool), F, counts


def sync_iter_score(session, shift, F, mshift, threshold=10):
    """``mvus_sync_iter_score``: (inliers, overlap) per model (F[m] 3 x 3, mshift[m] = beta d) at the current ``shift``: M x 2."""
    F = np.asarray(F, dtype=np.float64).reshape(-1, 9)
    mshift = np.asarray(mshift, dtype=np.float64).reshape(-1)
    if F.shape[0] != mshift.size:
        raise ValueError('one shift per model')
    models = np.ascontiguousarray(np.hstack((F, mshift[:, None], np.ones((F.shape[0], 1)))))
    counts = np.zeros((F.shape[0], 2), dtype=np.int32)
    rc = session._lib.mvus_sync_iter_score(session._h, float(shift), F.shape[0], _lib.dptr(models), float(threshold), counts.ctypes.data_as(_lib.c_int32_p))
    if rc != 0:
        ep._raise(session._lib, rc, 'mvus_sync_iter_score')
    return counts


def sync_iter_gpu(fps1, fps2, detect1, detect2, frame1, frame2, maxIter=200, threshold=10, step=10, p_min=0, p_max=6, verbose=False, seed=0,
                  device=0):
    """synchronization.py:13-130 (``sync_iter``): the time shift of camera 2 against camera 1 by the iterative algorithm of Albl et al.,
    "On the two-view geometry of unsynchronized cameras" (CVPR 2017), from the prior given by the corresponding frames.  Returns
    (beta, inlier ratio) like the reference.  The samples come from the library's counter-based sampler (``seed``), not from
    ``np.random.choice``: the same call gives the same bits."""
    # pre-processing (synchronization.py:85-92); camera 2's spline stays on its own timeline, the device carries beta as a shift
    alpha = fps1 / fps2
    beta_prior = frame1 / alpha - frame2
    detect1 = np.asarray(detect1, dtype=np.float64)
    d1 = np.vstack((detect1[0] / alpha, detect1[1:3]))
    with SyncIterSession(d1, detect2, device=device) as session:
        # the iterative algorithm (synchronization.py:95-130), branch for branch
        skip, maxInlier, k = 0, 0, 0
        d, p, beta = 2 ** p_min, p_min, beta_prior
        rnd = 0
        while k < step:
            (beta1, Inlier1, _, _), (beta2, Inlier2, _, _) = _round(session, beta, d, maxIter, threshold, seed, rnd)
            rnd += 1
            beta_temp = beta1 if Inlier1 >= Inlier2 else beta2
            Inlier = Inlier1 if Inlier1 >= Inlier2 else Inlier2
            if verbose:
                print('d:{}, beta:{:.3f}, maxInlier:{}, Inlier:{}'.format(d, (beta + beta_temp) * alpha, maxInlier, Inlier))
            if skip > p_max:
                break
            elif Inlier < maxInlier:
                if p < p_max:
                    p += 1
                else:
                    p = 0
                d = 2 ** p
                skip += 1
            else:
                beta += beta_temp
                maxInlier = Inlier
                skip = 0
                k += 1
    return beta * alpha, maxInlier
