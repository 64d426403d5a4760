"""Temporal synchronisation search of the reference's ``reconstruction/synchronization.py``: ``sync_bf`` (synchronization.py:133-178),
the brute-force search that ``Scene.time_shift`` runs when the corresponding frames are not exact (``cf_exact: false``,
``sync_method: 'bf'``).  Every candidate time shift is scored by the inliers of a RANSAC fundamental matrix over the detections
the two cameras share at that shift; the reference runs one ``cv2.findFundamentalMat`` per candidate, here each of the two stages
(20 coarse, 20 fine candidates) is ONE batched call of ``mvus_fundamental_ransac`` (epipolar.fundamental_ransac_batch).
``sync_iter`` (a generalised eigenproblem per sample) is not implemented."""
import numpy as np

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
