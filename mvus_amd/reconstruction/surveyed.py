"""Surveyed landmarks, clicks and position priors read from text files and checked; the similarity onto them.  Host only, no ``Scene`` (``common`` serves these names too)."""
import numpy as np


def umeyama_similarity(X, Y):
    """(s, R, T) minimising sum |s R X_i + T - Y_i|^2 over similarities (Umeyama 1991), X and Y (3, k) with k >= 3: R a proper rotation."""
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    mx, my = X.mean(axis=1, keepdims=True), Y.mean(axis=1, keepdims=True)
    a, b = X - mx, Y - my
    U, D, Vt = np.linalg.svd(b @ a.T / X.shape[1])
    S = np.ones(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        S[2] = -1.0
    R = U @ np.diag(S) @ Vt
    s = float(np.sum(D * S) / (np.sum(a * a) / X.shape[1]))
    T = (my - s * (R @ mx)).ravel()
    return s, R, T


def _undistort_normalised(x0, y0, d):
    """cv2.undistortPoints on normalised coordinates (five fixed-point iterations), host side"""
    k1, k2, p1, p2, k3 = (list(d) + [0.0] * 5)[:5]
    x, y = x0, y0
    for _ in range(5):
        r2 = x * x + y * y
        ic = 1.0 / (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2)
        if ic < 0:
            return x0, y0
        dx = 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
        dy = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
        x, y = (x0 - dx) * ic, (y0 - dy) * ic
    return x, y


def check_landmarks(X, ob, what='landmarks'):
    """((3, L) landmarks, (6, K) observations: camera id, landmark, u, v, sigma_u, sigma_v), validated: finite positions and pixels, whole
    non-negative camera ids, landmark indices inside [0, L), sigmas positive (inf allowed)."""
    X, ob = np.asarray(X, dtype=np.float64), np.asarray(ob, dtype=np.float64)
    if X.ndim != 2 or X.shape[0] != 3:
        raise ValueError('%s must be a (3, L) array, not shape %s' % (what, X.shape))
    if ob.ndim != 2 or ob.shape[0] != 6:
        raise ValueError('%s: the observations must be a (6, K) array of camera, landmark, u, v, sigma_u, sigma_v, not shape %s' % (what, ob.shape))
    if not np.all(np.isfinite(X)) or not np.all(np.isfinite(ob[:4])):
        raise ValueError('%s: a position, an index or a pixel is not finite' % what)
    if np.any(ob[:2] != np.floor(ob[:2])) or np.any(ob[0] < 0) or np.any(ob[1] < 0) or np.any(ob[1] >= X.shape[1]):
        raise ValueError('%s: camera ids must be whole and >= 0, landmark indices whole and inside [0, %d)' % (what, X.shape[1]))
    if np.any(np.isnan(ob[4:])) or np.any(ob[4:] <= 0):
        raise ValueError('%s: sigma must be positive (inf leaves an axis out)' % what)
    return X, ob


def load_landmarks(path_points, path_observations, default_sigma=None):
    """Two text files (``#`` comments): ``id x y z`` per landmark and ``camera id u v [sigma_u sigma_v]`` per click -> ((3, L), (6, K)) with the
    ids replaced by the landmark's position in the first file.  Clicks without sigma columns take ``default_sigma`` (a positive number, or
    two of them)."""
    try:
        a = np.loadtxt(path_points, dtype=np.float64, ndmin=2)
        b = np.loadtxt(path_observations, dtype=np.float64, ndmin=2)
    except ValueError as e:
        raise ValueError('landmarks %s / %s: %s' % (path_points, path_observations, e)) from None
    if a.shape[0] and a.shape[1] != 4:
        raise ValueError('landmarks %s: %d columns, expected id x y z' % (path_points, a.shape[1]))
    a = a.reshape(-1, 4)
    ids = a[:, 0]
    if np.any(ids != np.floor(ids)) or np.unique(ids).size != ids.size:
        raise ValueError('landmarks %s: ids must be whole numbers, each once' % path_points)
    if b.shape[0] == 0:
        return a[:, 1:4].T.copy(), np.empty((6, 0))
    if b.shape[1] == 4:
        if default_sigma is None:
            raise ValueError("landmark observations %s: columns camera id u v only -- give sigma_u sigma_v columns or 'landmark_sigma'" % path_observations)
        sg = np.asarray(default_sigma, dtype=np.float64)
        if sg.shape not in ((), (2,)) or isinstance(default_sigma, bool):
            raise ValueError("'landmark_sigma' must be a positive number or two of them, not %r" % (default_sigma,))
        b = np.hstack((b, np.broadcast_to(sg, (b.shape[0], 2))))
    elif b.shape[1] != 6:
        raise ValueError('landmark observations %s: %d columns, expected camera id u v [sigma_u sigma_v]' % (path_observations, b.shape[1]))
    where = {int(i): k for k, i in enumerate(ids)}
    unknown = [int(i) for i in b[:, 1] if i != np.floor(i) or int(i) not in where]
    if unknown:
        raise ValueError('landmark observations %s: ids %s are not in %s' % (path_observations, sorted(set(unknown)), path_points))
    ob = b.T.copy()
    ob[1] = [where[int(i)] for i in b[:, 1]]
    return check_landmarks(a[:, 1:4].T.copy(), ob, 'landmarks %s' % path_points)


def check_position_priors(pp, what='position priors'):
    """A (7, K) float array of t, x, y, z, sigma_x, sigma_y, sigma_z, validated: finite t and positions, sigmas positive (inf allowed)."""
    pp = np.asarray(pp, dtype=np.float64)
    if pp.ndim != 2 or pp.shape[0] != 7:
        raise ValueError('%s must be a (7, K) array of t, x, y, z, sigma_x, sigma_y, sigma_z, not shape %s' % (what, pp.shape))
    if not np.all(np.isfinite(pp[:4])):
        raise ValueError('%s: a time or a position is not finite' % what)
    if np.any(np.isnan(pp[4:])) or np.any(pp[4:] <= 0):
        raise ValueError('%s: sigma must be positive (inf leaves an axis out)' % what)
    return pp


def load_position_priors(path, default_sigma=None):
    """A text file with the columns t x y z [sigma_x sigma_y sigma_z] (one prior per line, ``#`` comments) -> (7, K).  Files without the sigma
    columns take ``default_sigma`` (a positive number, or three of them)."""
    try:
        a = np.loadtxt(path, dtype=np.float64, ndmin=2)
    except ValueError as e:
        raise ValueError('position priors %s: %s' % (path, e)) from None
    if a.shape[0] == 0:
        return np.empty((7, 0))
    if a.shape[1] == 4:
        if default_sigma is None:
            raise ValueError("position priors %s: columns t x y z only -- give sigma_x sigma_y sigma_z columns or 'position_prior_sigma'" % path)
        sg = np.asarray(default_sigma, dtype=np.float64)
        if sg.shape not in ((), (3,)) or isinstance(default_sigma, bool):
            raise ValueError("'position_prior_sigma' must be a positive number or three of them, not %r" % (default_sigma,))
        a = np.hstack((a, np.broadcast_to(sg, (a.shape[0], 3))))
    elif a.shape[1] != 7:
        raise ValueError('position priors %s: %d columns, expected t x y z [sigma_x sigma_y sigma_z]' % (path, a.shape[1]))
    return check_position_priors(a.T.copy(), 'position priors %s' % path)
