"""Two-view geometry of the reference's ``reconstruction/epipolar.py`` on the GPU, with the reference's names and signatures:

* ``triangulate_matlab`` (epipolar.py:497-510), called per camera pair by ``Scene.triangulate`` (common.py:783) -- there a
  Python loop with one 4x4 ``np.linalg.svd`` per point, here one lane per point in ``k_triangulate``
  (csrc/triangulate.hip.h, one-sided Jacobi SVD) through ``mvus_triangulate``; ``triangulate_with_cov`` adds the covariance of
  every point (``k_triangulate_cov`` through ``mvus_triangulate_cov``; no reference counterpart);
* ``computeFundamentalMat`` (epipolar.py:92-118, ``cv2.findFundamentalMat(FM_RANSAC)``) and its batched form
  ``fundamental_ransac_batch`` (one call for many independent point sets: ``synchronization.sync_bf``), through
  ``mvus_fundamental_ransac``;
* ``correct_matches`` (the ``cv2.correctMatches`` call of ``Scene.init_traj``, Hartley-Sturm) through ``mvus_correct_matches``;
* ``compute_Rt_from_E`` (epipolar.py:513-539) and ``triangulate_from_E`` (epipolar.py:568-588, the four candidates scored in one
  launch) through ``mvus_pose_from_essential``.

OpenCV is absent from this image, so the RANSAC output is not pinned to OpenCV's (csrc/epipolar.hip.h states the contract that
is restated).  FM_LMEDS and FM_8POINT are not implemented.  No CPU fallback."""
import ctypes

import numpy as np

from .. import _lib


def _call(x1, x2, P1, P2, errors, device):
    lib = _lib.load()
    x1 = np.ascontiguousarray(np.asarray(x1, dtype=np.float64)[:2])
    x2 = np.ascontiguousarray(np.asarray(x2, dtype=np.float64)[:2])
    if x1.shape != x2.shape or x1.ndim != 2:
        raise ValueError('x1 and x2 must both be (2 or 3) x N')
    P1 = np.ascontiguousarray(P1, dtype=np.float64)
    P2 = np.ascontiguousarray(P2, dtype=np.float64)
    if P1.shape != (3, 4) or P2.shape != (3, 4):
        raise ValueError('P1 and P2 must be 3 x 4')
    N = x1.shape[1]
    X = np.empty((4, N))
    e1 = np.empty(N) if errors else None
    e2 = np.empty(N) if errors else None
    rc = lib.mvus_triangulate(int(device), N, _lib.dptr(x1), _lib.dptr(x2), _lib.dptr(P1), _lib.dptr(P2), _lib.dptr(X),
                              _lib.dptr(e1) if errors else None, _lib.dptr(e2) if errors else None)
    if rc != 0:
        raise (ValueError if rc == _lib.MVUS_E_INVALID else RuntimeError)('mvus_triangulate: ' + lib.mvus_last_error(None).decode())
    return X, e1, e2


def triangulate_matlab(x1, x2, P1, P2, device=0):
    """x1, x2: (2 or 3) x N pixel coordinates (a homogeneous third row is ignored, like the reference only reads rows 0
    and 1); returns 4 x N homogeneous points with last row 1 (epipolar.py:497-510)."""
    return _call(x1, x2, P1, P2, False, device)[0]


def triangulate_with_errors(x1, x2, P1, P2, device=0):
    """triangulate_matlab plus the reprojection distances in both cameras (what Scene.triangulate thresholds,
    common.py:786-789), computed in the same kernel."""
    return _call(x1, x2, P1, P2, True, device)


def triangulate_with_cov(x1, x2, P1, P2, sigma1=1.0, sigma2=1.0, device=0):
    """triangulate_with_errors plus the covariance of every point (``mvus_triangulate_cov``, the same kernel work and the same bits of
    X, d1, d2): returns (Xh 4 x N, cov N x 3 x 3, d1, d2).  ``cov`` is the Gauss-Newton covariance (A^T A)^-1 of the point at Xh for
    isotropic pixel noise ``sigma1`` / ``sigma2`` (1-sigma, px) in the two cameras, symmetric to the bit; NaN for a pair without
    parallax, with a non-finite point or a point behind a camera.  No reference counterpart."""
    lib = _lib.load()
    x1 = np.ascontiguousarray(np.asarray(x1, dtype=np.float64)[:2])
    x2 = np.ascontiguousarray(np.asarray(x2, dtype=np.float64)[:2])
    if x1.shape != x2.shape or x1.ndim != 2:
        raise ValueError('x1 and x2 must both be (2 or 3) x N')
    P1 = np.ascontiguousarray(P1, dtype=np.float64)
    P2 = np.ascontiguousarray(P2, dtype=np.float64)
    if P1.shape != (3, 4) or P2.shape != (3, 4):
        raise ValueError('P1 and P2 must be 3 x 4')
    N = x1.shape[1]
    X, c6, e1, e2 = np.empty((4, N)), np.empty((6, N)), np.empty(N), np.empty(N)
    rc = lib.mvus_triangulate_cov(int(device), N, _lib.dptr(x1), _lib.dptr(x2), _lib.dptr(P1), _lib.dptr(P2), float(sigma1), float(sigma2),
                                  _lib.dptr(X), _lib.dptr(c6), _lib.dptr(e1), _lib.dptr(e2))
    if rc != 0:
        raise (ValueError if rc == _lib.MVUS_E_INVALID else RuntimeError)('mvus_triangulate_cov: ' + lib.mvus_last_error(None).decode())
    cov = c6[[0, 1, 2, 1, 3, 4, 2, 4, 5]].T.reshape(N, 3, 3)      # xx xy xz / xy yy yz / xz yz zz: both halves from the same six values
    return X, np.ascontiguousarray(cov), e1, e2


def reprojection_error(x, x_p):
    """epipolar.py:639."""
    return np.sqrt((x[0] - x_p[0]) ** 2 + (x[1] - x_p[1]) ** 2)


FM_RANSAC, FM_LMEDS, FM_8POINT = 8, 4, 2          # OpenCV's values
RANSAC_ITERATIONS = 1000                           # OpenCV 4's default maxIters of findFundamentalMat


def _raise(lib, rc, name):
    raise (ValueError if rc == _lib.MVUS_E_INVALID else RuntimeError)('%s: %s' % (name, lib.mvus_last_error(None).decode()))


def _rows2(x, name):
    x = np.asarray(x, dtype=np.float64)
    if x.ndim != 2 or x.shape[0] < 2:
        raise ValueError('%s must be (2 or 3) x N' % name)
    return x[:2]


def fundamental_ransac_batch(pairs, error=3, seed=0, iterations=RANSAC_ITERATIONS, device=0):
    """``cv2.findFundamentalMat(p1, p2, FM_RANSAC, error)`` for every (pts1, pts2) of ``pairs`` -- each (2 or 3) x N_p pixels,
    N_p >= 8 -- in ONE library call (all problems in the same launches).  Returns a list of (F 3x3, mask uint8[N_p]) and the
    inlier counts.  The samples of problem p depend only on (seed, hypothesis, N_p): the result of a problem does not depend on
    what else is in the batch."""
    lib = _lib.load()
    pairs = list(pairs)
    if not pairs:
        return [], np.zeros(0, dtype=np.int32)
    x1s, x2s, offs = [], [], [0]
    for a, b in pairs:
        a, b = _rows2(a, 'pts1'), _rows2(b, 'pts2')
        if a.shape != b.shape:
            raise ValueError('pts1 and pts2 differ in shape')
        x1s.append(a)
        x2s.append(b)
        offs.append(offs[-1] + a.shape[1])
    x1 = np.ascontiguousarray(np.hstack(x1s))
    x2 = np.ascontiguousarray(np.hstack(x2s))
    offs = np.asarray(offs, dtype=np.int64)
    P = len(pairs)
    F = np.zeros((P, 9))
    mask = np.zeros(max(int(offs[-1]), 1), dtype=np.uint8)
    cnt = np.zeros(P, dtype=np.int32)
    rc = lib.mvus_fundamental_ransac(int(device), P, offs.ctypes.data_as(_lib.c_int64_p), _lib.dptr(x1), _lib.dptr(x2), float(error),
                                     int(iterations), int(seed), _lib.dptr(F), mask.ctypes.data_as(_lib.c_uint8_p),
                                     cnt.ctypes.data_as(_lib.c_int32_p))
    if rc != 0:
        _raise(lib, rc, 'mvus_fundamental_ransac')
    return [(F[p].reshape(3, 3), mask[offs[p]:offs[p + 1]].copy()) for p in range(P)], cnt


def computeFundamentalMat(pts1, pts2, method=FM_RANSAC, error=3, inliers=True, seed=0, device=0):
    """epipolar.py:92-118: F (3x3) and, with ``inliers``, the inlier mask (uint8[N]) of ``cv2.findFundamentalMat(pts1.T,
    pts2.T, method, error)``; pts1, pts2 (2 or 3) x N pixels."""
    if method != FM_RANSAC:
        raise NotImplementedError('computeFundamentalMat: only FM_RANSAC is restated on the GPU (FM_LMEDS and FM_8POINT are not used '
                                  'by the reference pipeline)')
    (F, mask), = fundamental_ransac_batch([(pts1, pts2)], error=error, seed=seed, device=device)[0]
    return (F, mask) if inliers else F


def correct_matches(F, x1, x2, device=0):
    """``cv2.correctMatches(F, pts1, pts2)`` (Hartley-Sturm optimal correction) of (2 or 3) x N pixel pairs: the corrected
    x1, x2 as 2 x N.  A pair with a non-finite coordinate comes back as NaN (Scene.init_traj masks those)."""
    lib = _lib.load()
    x1 = np.ascontiguousarray(_rows2(x1, 'x1'))
    x2 = np.ascontiguousarray(_rows2(x2, 'x2'))
    if x1.shape != x2.shape:
        raise ValueError('x1 and x2 differ in shape')
    F = np.ascontiguousarray(np.asarray(F, dtype=np.float64).reshape(9))
    N = x1.shape[1]
    o1, o2 = np.empty((2, N)), np.empty((2, N))
    rc = lib.mvus_correct_matches(int(device), N, _lib.dptr(F), _lib.dptr(x1), _lib.dptr(x2), _lib.dptr(o1), _lib.dptr(o2))
    if rc != 0:
        _raise(lib, rc, 'mvus_correct_matches')
    return o1, o2


def compute_Rt_from_E(E):
    """epipolar.py:513-539: the four [R|t] (3x4) for P1 = [I|0], in the reference's order -- (R1, t), (R1, -t), (R2, t), (R2, -t)
    with R1 = U W V^T, R2 = U W^T V^T (each times its determinant), t = U[:, 2], V^T negated when det(U V^T) < 0."""
    U, _, Vt = np.linalg.svd(np.asarray(E, dtype=np.float64))
    if np.linalg.det(U @ Vt) < 0:
        Vt = -Vt
    W = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    rots = [U @ W @ Vt, U @ W.T @ Vt]
    rots = [R * np.linalg.det(R) for R in rots]
    t = U[:, 2].reshape(3, 1)
    return [np.hstack((R, s * t)) for R in rots for s in (1.0, -1.0)]


def triangulate_from_E(E, K1, K2, x1, x2, device=0):
    """epipolar.py:568-588: x1, x2 homogeneous 3 x N pixels; normalised by K^-1, the four candidates of compute_Rt_from_E scored by
    the points in front of both cameras (one launch), the first to exceed the running maximum triangulated.  Returns
    (X 4 x N with last row 1, P2 = [R|t])."""
    lib = _lib.load()
    x1n = np.linalg.inv(K1) @ np.asarray(x1, dtype=np.float64)
    x2n = np.linalg.inv(K2) @ np.asarray(x2, dtype=np.float64)
    x1n = np.ascontiguousarray(x1n[:2] / x1n[2])
    x2n = np.ascontiguousarray(x2n[:2] / x2n[2])
    E = np.ascontiguousarray(np.asarray(E, dtype=np.float64).reshape(9))
    N = x1n.shape[1]
    X = np.empty((4, N))
    P2 = np.empty((3, 4))
    rc = lib.mvus_pose_from_essential(int(device), N, _lib.dptr(E), _lib.dptr(x1n), _lib.dptr(x2n), _lib.dptr(P2), _lib.dptr(X))
    if rc != 0:
        _raise(lib, rc, 'mvus_pose_from_essential')
    return X, P2
