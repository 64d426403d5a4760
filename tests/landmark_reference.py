"""References for the landmark rows (mvus_ba_set_landmarks): one row pair and its P derivatives in mpmath, built from the pieces of
tests/mp_observation.py (Dual, rodrigues, undistort_points) -- the detection row's camera part with the spline point replaced by a
constant X -- at mpmath's CURRENT precision (50 digits for the reference, ``mpmath.workprec(53)`` for a plain-fp64 evaluation of this
text); a vectorised numpy restatement for costs and sums; the edge cases of the host test and the observation sets of the GPU test.
Shares no code with mvus_amd/csrc/ba_landmark_math.h.  Host only."""
import mpmath
import numpy as np
from mpmath import mpf

from mp_observation import DPS, Dual, rodrigues, seeded, undistort_points

EPS = np.finfo(np.float64).eps
TOL_FACTOR = 8.0
RESIDUAL_ATOL = 1e-9       # px, the project's residual bar
GROUPS_P6 = dict(rvec=(0, 3), t=(3, 6))
GROUPS_P15 = dict(intrinsics=(0, 4), rvec=(4, 7), t=(7, 10), distortion=(10, 15))


def groups(P):
    return GROUPS_P15 if P == 15 else GROUPS_P6


def group_ratio(J, Jref):
    """worst |J - Jref| / max |Jref| over the entry's slot group of ONE row and axis; J, Jref [..., P].  An entry of a group that is all
    zero in the reference must be zero."""
    worst = 0.0
    for lo, hi in groups(Jref.shape[-1]).values():
        scale = np.max(np.abs(Jref[..., lo:hi]), axis=-1, keepdims=True)
        diff = np.abs(J[..., lo:hi] - Jref[..., lo:hi])
        ok = scale > 0
        r = np.where(ok, diff / np.where(ok, scale, 1.0), np.where(diff > 0, np.inf, 0.0))
        worst = max(worst, float(r.max()))
    return worst


def row_mp(calib, undist, K4, d5, params, X, uv, w):
    """(r[2], J[2][P]) of one observation as float64 arrays, evaluated at the current mpmath precision.  ``params``: the camera's P
    parameters in x's order; K4 / d5: the fixed calibration (ignored under calib)."""
    P = 15 if calib else 6
    if calib:
        fx, fy, cx, cy = (seeded(params[k], k) for k in range(4))
        rvec = [seeded(params[4 + k], 4 + k) for k in range(3)]
        tvec = [seeded(params[7 + k], 7 + k) for k in range(3)]
        dist = [seeded(params[10 + k], 10 + k) for k in range(5)]
    else:
        fx, fy, cx, cy = (seeded(K4[k]) for k in range(4))
        rvec = [seeded(params[k], k) for k in range(3)]
        tvec = [seeded(params[3 + k], 3 + k) for k in range(3)]
        dist = [seeded(d5[k]) for k in range(5)]
    Xw = [mpf(float(v)) for v in X]
    u_raw, v_raw = mpf(float(uv[0])), mpf(float(uv[1]))
    R = rodrigues(rvec)
    Xc = [R[r][0] * Xw[0] + R[r][1] * Xw[1] + R[r][2] * Xw[2] + tvec[r] for r in range(3)]
    hom = [fx * Xc[0] + cx * Xc[2], fy * Xc[1] + cy * Xc[2], Xc[2]]
    u_cal, v_cal = hom[0] / hom[2], hom[1] / hom[2]
    if undist:
        xn, yn, _ = undistort_points((u_raw - cx) / fx, (v_raw - cy) / fy, *dist)
        u_obs, v_obs = fx * xn + cx, fy * yn + cy
        if not calib:                                              # undistorted once, with the fixed calibration: a constant
            u_obs, v_obs = Dual(u_obs.v), Dual(v_obs.v)
    else:
        u_obs, v_obs = Dual(u_raw), Dual(v_raw)
    res = [u_cal - u_obs, v_cal - v_obs]
    r, J = np.zeros(2), np.zeros((2, P))
    for a in range(2):
        wa = mpf(float(w[a]))
        r[a] = float(wa * res[a].v)
        for k in range(P):
            J[a, k] = float(wa * res[a].d.get(k, mpf(0)))
    return r, J


def rows_mp(prob, x, X, cam, point, uv, w, dps=DPS):
    """(r (2, K), J (K, 2, P)) of an observation set on BAProblem ``prob`` at x, at ``dps`` digits (None: the current precision)."""
    K, P, C = len(cam), prob.P, prob.C
    r, J = np.zeros((2, K)), np.zeros((K, 2, P))
    ctx = mpmath.workdps(dps) if dps else mpmath.workprec(mpmath.mp.prec)
    with ctx:
        for k in range(K):
            c = int(cam[k])
            rk, Jk = row_mp(prob.opt_calib, prob.undist_points, prob.K[c], prob.dist[c], x[3 * C + c * P:3 * C + (c + 1) * P],
                            X[:, int(point[k])], uv[:, k], w[:, k])
            r[:, k], J[k] = rk, Jk
    return r, J


def rodrigues_np(r):
    th = np.linalg.norm(r)
    if th < EPS:
        return np.eye(3)
    k = r / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.cos(th) * np.eye(3) + (1 - np.cos(th)) * np.outer(k, k) + np.sin(th) * Kx


def undistort_np(x0, y0, d):
    k1, k2, p1, p2, k3 = d
    x, y = x0, y0
    for _ in range(5):
        r2 = x * x + y * y
        ic = 1.0 / (1 + ((k3 * r2 + k2) * r2 + k1) * r2)
        if ic < 0:
            return x0, y0
        dx = 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
        dy = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
        x, y = (x0 - dx) * ic, (y0 - dy) * ic
    return x, y


def camera_np(prob, x, c):
    """(K4, d5, R, t) of camera c at x"""
    C, P = prob.C, prob.P
    v = x[3 * C + c * P:3 * C + (c + 1) * P]
    if prob.opt_calib:
        return v[0:4], v[10:15], rodrigues_np(v[4:7]), v[7:10]
    return np.asarray(prob.K[c], dtype=np.float64), np.asarray(prob.dist[c], dtype=np.float64), rodrigues_np(v[0:3]), v[3:6]


def project_np(prob, x, c, Xw):
    K4, _, R, t = camera_np(prob, x, c)
    Xc = R @ Xw + t
    return np.array([K4[0] * Xc[0] / Xc[2] + K4[2], K4[1] * Xc[1] / Xc[2] + K4[3]]), Xc[2]


def rows_np(prob, x, X, cam, point, uv, w):
    """r (2, K) in plain numpy fp64"""
    K = len(cam)
    r = np.zeros((2, K))
    for k in range(K):
        c = int(cam[k])
        K4, d5, _, _ = camera_np(prob, x, c)
        pred, _ = project_np(prob, x, c, X[:, int(point[k])])
        obs = np.array(uv[:, k], dtype=np.float64)
        if prob.undist_points:
            xn, yn = undistort_np((obs[0] - K4[2]) / K4[0], (obs[1] - K4[3]) / K4[1], d5)
            obs = np.array([K4[0] * xn + K4[2], K4[1] * yn + K4[3]])
        r[:, k] = w[:, k] * (pred - obs)
    return r


def cost_np(prob, x, X, cam, point, uv, w):
    return 0.5 * float(np.sum(rows_np(prob, x, X, cam, point, uv, w) ** 2))


def contribution(prob, cam, r, J):
    """(dA [C, P, P], dgc [C, P], bA, bg): sum J^T J and sum J^T r per camera of the given rows, and per entry the sum of |terms| and the
    number of rows -- what the derived bound of the normal-equation test needs."""
    C, P = prob.C, prob.P
    dA, dg = np.zeros((C, P, P)), np.zeros((C, P))
    aA, ag = np.zeros((C, P, P)), np.zeros((C, P))
    n = np.zeros(C, dtype=np.int64)
    for k in range(len(cam)):
        c = int(cam[k])
        n[c] += 1
        for a in range(2):
            dA[c] += np.outer(J[k, a], J[k, a])
            aA[c] += np.abs(np.outer(J[k, a], J[k, a]))
            dg[c] += J[k, a] * r[a, k]
            ag[c] += np.abs(J[k, a] * r[a, k])
    return dA, dg, aA, ag, n


# ---- the host test's edge cases ------------------------------------------------------------------------------------
K_PIN = np.array([1400.0, 1410.0, 960.0, 540.0])
D_FIX = np.array([-0.12, 0.05, 1.5e-3, -8e-4, 0.01])       # replaced by the dist_fixed_2cam cameras where the fixture is at hand


def host_cases(fixed=None):
    """[(name, calib, undist, K4, d5, params[P], X, uv, w)]: P = 6 and 15, undist on and off, fixed calibration with distortion (``fixed``:
    [(K4, d5)] of the dist_fixed_2cam cameras), |rvec| = 0, either side of kRodriguesSeries = 1e-2 and ordinary, a point near the image
    border and one near the principal point, a residual that is exactly 0 on one axis, a weightless axis."""
    rng = np.random.default_rng(23)
    fixed = fixed or [(K_PIN, D_FIX)]
    rvecs = {'r0': np.zeros(3), 'rlo': np.array([0.3, -0.5, 0.8]) * 9.9e-3 / np.linalg.norm([0.3, -0.5, 0.8]),
             'rhi': np.array([0.3, -0.5, 0.8]) * 1.01e-2 / np.linalg.norm([0.3, -0.5, 0.8]), 'rtiny': np.array([1e-9, -2e-9, 5e-10]),
             'rord': np.array([0.31, -0.22, 0.17]), 'rbig': np.array([1.2, 0.9, -1.6])}
    cases = []
    for calib in (False, True):
        for undist in (False, True):
            for ci, (K4, d5) in enumerate(fixed if not calib else [(K_PIN, D_FIX)]):
                for rn, rv in rvecs.items():
                    R = rodrigues_np(rv)
                    t = np.array([0.4, -0.3, 6.0])
                    for pn, pix in (('border', np.array([25.0, 1050.0])), ('centre', K4[2:4] + np.array([0.75, -0.5])), ('mid', np.array([1300.0, 300.0]))):
                        z = 5.0 + 3.0 * rng.random()
                        Xc = np.array([(pix[0] - K4[2]) / K4[0] * z, (pix[1] - K4[3]) / K4[1] * z, z])
                        X = R.T @ (Xc - t)
                        uv = pix + rng.uniform(-4, 4, 2)
                        w = np.array([1.0 / 0.7, 1.0 / 1.3])
                        params = np.concatenate([K4, rv, t, d5]) if calib else np.concatenate([rv, t])
                        cases.append(('%s_%s_c%d_%s_%s' % ('P15' if calib else 'P6', 'ud' if undist else 'raw', ci, rn, pn), calib, undist, K4, d5, params, X, uv, w))
    # a residual that is exactly 0 on one axis: a point on the x = 0 plane of a camera without rotation, observed at u = cx (undist off)
    for calib in (False, True):
        rv, t = np.zeros(3), np.array([0.0, 0.0, 5.0])
        params = np.concatenate([K_PIN, rv, t, D_FIX]) if calib else np.concatenate([rv, t])
        cases.append(('%s_zero_u' % ('P15' if calib else 'P6'), calib, False, K_PIN, D_FIX, params, np.array([0.0, 0.3, 0.0]), np.array([K_PIN[2], 700.0]), np.array([2.0, 0.5])))
        cases.append(('%s_w0_axis' % ('P15' if calib else 'P6'), calib, True, K_PIN, D_FIX, params, np.array([0.2, 0.3, 0.1]), np.array([1000.0, 650.0]), np.array([0.0, 0.5])))
    return cases


# ---- the GPU test's landmarks and observation sets ------------------------------------------------------------------
def landmarks_in_front(prob, x, L, seed=3, spread=0.25):
    """L world points in front of every camera at x: around the point the cameras' axes come closest to, scaled by its depth."""
    rng = np.random.default_rng(seed)
    cams = [camera_np(prob, x, c) for c in range(prob.C)]
    # least-squares meeting point of the optical axes
    A, b = np.zeros((3, 3)), np.zeros(3)
    for _, _, R, t in cams:
        o, d = -R.T @ t, R.T @ np.array([0.0, 0.0, 1.0])
        Pm = np.eye(3) - np.outer(d, d)
        A += Pm
        b += Pm @ o
    centre = np.linalg.lstsq(A, b, rcond=None)[0]
    depth = min((R @ centre + t)[2] for _, _, R, t in cams)
    if depth <= 0:                                                  # axes that diverge: a point in front of camera 0, pushed until all see it
        _, _, R, t = cams[0]
        centre, depth = R.T @ (np.array([0.0, 0.0, 10.0]) - t), 10.0
    X = centre[:, None] + spread * abs(depth) * rng.uniform(-1, 1, (3, L))
    for _, _, R, t in cams:
        assert np.all((R @ X + t[:, None])[2] > 0), 'a landmark behind a camera'
    return X


def observations(prob, x, X, cam, point, seed=9, sigma=(0.8, 1.1), offset=3.0):
    """(uv (2, K), w (2, K)): projections at x plus a fixed pseudo-random offset of a few pixels.  Under undist_points the offset is put on
    the undistorted pixel's raw counterpart only approximately (the raw pixel IS the projection + offset): r is a few pixels either way."""
    rng = np.random.default_rng(seed)
    K = len(cam)
    uv = np.zeros((2, K))
    for k in range(K):
        uv[:, k] = project_np(prob, x, int(cam[k]), X[:, int(point[k])])[0]
    uv += rng.uniform(-offset, offset, (2, K))
    w = np.broadcast_to(1.0 / np.asarray(sigma, dtype=np.float64)[:, None], (2, K)).copy()
    return uv, w
