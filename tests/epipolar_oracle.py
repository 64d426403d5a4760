"""numpy restatement of the two-view geometry of csrc/epipolar.hip.h, for the tests (CPU and GPU) and tools/time_init.py.

Independent of the kernels' own formulation where it can be: the 7-point null space from np.linalg.svd (the kernels use
Gauss-Jordan elimination), the cubic and the degree-6 Hartley-Sturm polynomial solved by np.roots (companion-matrix
eigenvalues; the kernels use closed forms and Aberth iteration), E decomposed by np.linalg.svd.  What must agree exactly is
restated exactly: the counter-based sampler and the error of a pair (same expression, same order, no fused operations)."""
import numpy as np

M64 = (1 << 64) - 1


def _mix(z):
    """splitmix64 finaliser (pnp_mix in csrc/pnp.hip.h)."""
    z = (z + 0x9e3779b97f4a7c15) & M64
    z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & M64
    z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & M64
    return z ^ (z >> 31)


def sample7(seed, h, N):
    """fm_sample7: the seven distinct indices of hypothesis h among N pairs."""
    ctr = (seed * 0x100000001b3 + h * 1000003 + 0x5851f42d4c957f2d) & M64
    idx = []
    while len(idx) < 7:
        ctr = _mix(ctr)
        c = ctr % N
        if c not in idx:
            idx.append(c)
    return idx


def fm_error(F, x1, x2):
    """OpenCV's error of F on pairs x1, x2 (2 x N pixels): max of the two squared point-to-epipolar-line distances."""
    F = np.asarray(F, dtype=np.float64).reshape(9)
    u1, v1, u2, v2 = x1[0], x1[1], x2[0], x2[1]
    a = F[0] * u1 + F[1] * v1 + F[2]
    b = F[3] * u1 + F[4] * v1 + F[5]
    c = F[6] * u1 + F[7] * v1 + F[8]
    with np.errstate(divide='ignore', invalid='ignore'):
        s2 = 1.0 / (a * a + b * b)
    d2 = u2 * a + v2 * b + c
    a = F[0] * u2 + F[3] * v2 + F[6]
    b = F[1] * u2 + F[4] * v2 + F[7]
    c = F[2] * u2 + F[5] * v2 + F[8]
    with np.errstate(divide='ignore', invalid='ignore'):
        s1 = 1.0 / (a * a + b * b)
    d1 = u1 * a + v1 * b + c
    e1, e2 = d1 * d1 * s1, d2 * d2 * s2
    return np.where(e1 > e2, e1, e2)


def line_distances2(F, x1, x2):
    """The two squared point-to-epipolar-line distances (d1: x1 to F^T x2, d2: x2 to F x1) whose maximum is fm_error."""
    F = np.asarray(F, dtype=np.float64).reshape(3, 3)
    h1, h2 = np.vstack((x1[:2], np.ones(x1.shape[1]))), np.vstack((x2[:2], np.ones(x2.shape[1])))
    l2, l1 = F @ h1, F.T @ h2
    r = np.sum(h2 * l2, axis=0)
    return r * r / (l1[0] ** 2 + l1[1] ** 2), r * r / (l2[0] ** 2 + l2[1] ** 2)


def hartley_normalisation(x):
    c = x.mean(axis=1)
    md = np.mean(np.sqrt(((x - c[:, None]) ** 2).sum(axis=0)))
    s = np.sqrt(2.0) / md
    return np.array([[s, 0, -s * c[0]], [0, s, -s * c[1]], [0, 0, 1.0]])


def _rows(x1, x2):
    u1, v1, u2, v2 = x1[0], x1[1], x2[0], x2[1]
    return np.stack((u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, np.ones_like(u1)), axis=1)


def seven_point(x1n, x2n):
    """The 7-point algorithm on 7 normalised pairs: the models (3x3, unnormalised scale) for the real roots of the cubic."""
    A = _rows(x1n, x2n)
    _, _, Vt = np.linalg.svd(A)
    F1, F2 = Vt[-2].reshape(3, 3), Vt[-1].reshape(3, 3)
    d = [np.linalg.det(l * F1 + (1 - l) * F2) for l in (0.0, 1.0, -1.0, 2.0)]
    c0 = d[0]
    c2 = 0.5 * (d[1] + d[2]) - c0
    s = 0.5 * (d[1] - d[2])
    c3 = (d[3] - 4 * c2 - c0 - 2 * s) / 6.0
    c1 = s - c3
    out = []
    for r in np.roots([c3, c2, c1, c0]):
        if abs(r.imag) <= 1e-9 * max(1.0, abs(r.real)):
            l = r.real
            out.append(l * F1 + (1 - l) * F2)
    return out


def unit(F):
    F = F / np.linalg.norm(F)
    return -F if F[2, 2] < 0 else F


def eight_point(x1, x2, T1, T2):
    """Normalised 8-point fit (smallest right singular vector, rank 2 by SVD), denormalised, unit norm."""
    A = _rows((T1 @ np.vstack((x1, np.ones(x1.shape[1]))))[:2], (T2 @ np.vstack((x2, np.ones(x2.shape[1]))))[:2])
    _, _, Vt = np.linalg.svd(A)
    Fn = Vt[-1].reshape(3, 3)
    U, S, Vt = np.linalg.svd(Fn)
    Fn = U @ np.diag([S[0], S[1], 0.0]) @ Vt
    return unit(T2.T @ Fn @ T1)


def fundamental_ransac(x1, x2, thresh, iterations=1000, seed=0):
    """The kernels' RANSAC in numpy: every hypothesis, scored by fm_error <= thresh^2, best count (lowest index on ties),
    8-point refit kept when it keeps at least as many inliers.  Returns (F, mask, count)."""
    x1 = np.asarray(x1, dtype=np.float64)[:2]
    x2 = np.asarray(x2, dtype=np.float64)[:2]
    N = x1.shape[1]
    T1, T2 = hartley_normalisation(x1), hartley_normalisation(x2)
    h1 = (T1 @ np.vstack((x1, np.ones(N))))[:2]
    h2 = (T2 @ np.vstack((x2, np.ones(N))))[:2]
    thr2 = thresh * thresh
    best, best_cnt = None, -1
    for h in range(iterations):
        idx = sample7(seed, h, N)
        for Fn in seven_point(h1[:, idx], h2[:, idx]):
            F = unit(T2.T @ Fn @ T1)
            cnt = int(np.count_nonzero(fm_error(F, x1, x2) <= thr2))
            if cnt > best_cnt:
                best, best_cnt = F, cnt
    mask = fm_error(best, x1, x2) <= thr2
    Fr = eight_point(x1[:, mask], x2[:, mask], T1, T2)
    mr = fm_error(Fr, x1, x2) <= thr2
    if mr.sum() >= best_cnt:
        return Fr, mr, int(mr.sum())
    return best, mask, best_cnt


# ---- Hartley-Sturm (H&Z Algorithm 12.1) ----------------------------------------------------------------------------------------
def _epipoles(F):
    U, _, Vt = np.linalg.svd(F)
    return Vt[-1], U[:, -1]


def correct_matches(F, x1, x2):
    """cv2.correctMatches(F, p1, p2): x1, x2 2 x N pixels -> corrected 2 x N; np.roots for the degree-6 polynomial,
    each root's real part polished by Newton steps, the cost also at t = 0 and t = infinity."""
    F = np.asarray(F, dtype=np.float64).reshape(3, 3)
    F = F / np.linalg.norm(F)
    e1, e2 = _epipoles(F)
    N = x1.shape[1]
    o1, o2 = np.full((2, N), np.nan), np.full((2, N), np.nan)
    for i in range(N):
        x, y, xp, yp = x1[0, i], x1[1, i], x2[0, i], x2[1, i]
        if not np.all(np.isfinite([x, y, xp, yp])):
            continue
        Ti = np.array([[1, 0, x], [0, 1, y], [0, 0, 1.0]])
        Tpi = np.array([[1, 0, xp], [0, 1, yp], [0, 0, 1.0]])
        G = Tpi.T @ F @ Ti
        ea = np.linalg.inv(Ti) @ e1
        eb = np.linalg.inv(Tpi) @ e2
        ea, eb = ea / np.hypot(ea[0], ea[1]), eb / np.hypot(eb[0], eb[1])
        R = np.array([[ea[0], ea[1], 0], [-ea[1], ea[0], 0], [0, 0, 1.0]])
        Rp = np.array([[eb[0], eb[1], 0], [-eb[1], eb[0], 0], [0, 0, 1.0]])
        G = Rp @ G @ R.T
        f, fp = ea[2], eb[2]
        a, b, c, d = G[1, 1], G[1, 2], G[2, 1], G[2, 2]
        P = np.polynomial.polynomial
        q = P.polyadd(P.polymul([b, a], [b, a]), fp * fp * P.polymul([d, c], [d, c]))
        g = P.polysub(P.polymul([0, 1], P.polymul(q, q)),
                      (a * d - b * c) * P.polymul(P.polymul([1, 0, f * f], [1, 0, f * f]), P.polymul([b, a], [d, c])))
        g = np.trim_zeros(np.asarray(g) / np.max(np.abs(g)), 'b')
        cost = lambda t: t * t / (1 + f * f * t * t) + (c * t + d) ** 2 / ((a * t + b) ** 2 + fp * fp * (c * t + d) ** 2)
        cands = [0.0]
        for r in np.roots(g[::-1]):
            t = r.real
            for _ in range(4):
                p, dp = P.polyval(t, g), P.polyval(t, P.polyder(g))
                if dp == 0:
                    break
                tn = t - p / dp
                if not np.isfinite(tn) or abs(P.polyval(tn, g)) > abs(p):
                    break
                t = tn
            cands.append(t)
        costs = [cost(t) for t in cands]
        k = int(np.argmin(costs))
        if f != 0 and 1 / (f * f) + c * c / (a * a + fp * fp * c * c) < costs[k]:
            l, lp = np.array([f, 0, -1.0]), np.array([-fp * c, a, c])
        else:
            t = cands[k]
            l, lp = np.array([t * f, 1, -t]), np.array([-fp * (c * t + d), a * t + b, c * t + d])
        p1 = np.array([-l[0] * l[2], -l[1] * l[2], l[0] ** 2 + l[1] ** 2])
        p2 = np.array([-lp[0] * lp[2], -lp[1] * lp[2], lp[0] ** 2 + lp[1] ** 2])
        p1 = Ti @ R.T @ p1
        p2 = Tpi @ Rp.T @ p2
        o1[:, i] = p1[:2] / p1[2]
        o2[:, i] = p2[:2] / p2[2]
    return o1, o2


# ---- E -> (R, t), cheirality -----------------------------------------------------------------------------------------------------
def rt_from_E(E):
    """The four [R|t] candidates in compute_Rt_from_E's order and sign convention."""
    U, _, Vt = np.linalg.svd(E)
    if np.linalg.det(U @ Vt) < 0:
        Vt = -Vt
    W = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1.0]])
    Ra, Rb = U @ W @ Vt, U @ W.T @ Vt
    Ra, Rb = Ra * np.linalg.det(Ra), Rb * np.linalg.det(Rb)
    t = U[:, 2:3]
    return [np.hstack((Ra, t)), np.hstack((Ra, -t)), np.hstack((Rb, t)), np.hstack((Rb, -t))]


def triangulate_dlt(x1, x2, P1, P2):
    """Linear triangulation (smallest right singular vector of the 4x4 system), last row 1; x 2 x N."""
    A = np.stack((x1[0][:, None] * P1[2] - P1[0], x1[1][:, None] * P1[2] - P1[1],
                  x2[0][:, None] * P2[2] - P2[0], x2[1][:, None] * P2[2] - P2[1]), axis=1)
    _, _, Vt = np.linalg.svd(A)
    X = Vt[:, -1, :].T
    return X / X[3]


def pose_from_essential(E, x1n, x2n):
    """triangulate_from_E on normalised coordinates: (X 4 x N, P2 3 x 4)."""
    P1 = np.hstack((np.eye(3), np.zeros((3, 1))))
    best, P2 = 0, None
    for cand in rt_from_E(E):
        X = triangulate_dlt(x1n, x2n, P1, cand)
        n = int(np.sum(X[2] > 0) + np.sum((cand @ X)[2] > 0))
        if n > best:
            best, P2 = n, cand
    return triangulate_dlt(x1n, x2n, P1, P2), P2


# ---- synthetic two-view data -------------------------------------------------------------------------------------------------
def synthetic_pair(N, sigma=0.5, outliers=0.3, seed=0):
    """Two cameras of mvus_amd.synth's ring (K, R, t of make_scene) looking at N random 3-D points near the trajectory's
    centroid: x1, x2 (2 x N pixels, Gaussian noise sigma, a fraction of gross outliers), the true F and the outlier flags."""
    from mvus_amd import synth
    sc = synth.make_scene(2, 200, seed=seed + 100, perturb=0.0)
    rng = np.random.default_rng(seed)
    tr = sc.truth['cameras']
    X = np.array([0.0, 0.0, 30.0])[:, None] + rng.uniform(-12, 12, (3, N))
    xs = []
    for c in tr:
        Xc = c['R'] @ X + c['t'][:, None]
        x = (c['K'] @ (Xc / Xc[2]))[:2] + rng.normal(0, sigma, (2, N))
        xs.append(x)
    bad = rng.uniform(size=N) < outliers
    xs[1][:, bad] = np.vstack((rng.uniform(0, 1920, bad.sum()), rng.uniform(0, 1080, bad.sum())))
    K1, K2 = tr[0]['K'], tr[1]['K']
    R = tr[1]['R'] @ tr[0]['R'].T
    t = tr[1]['t'] - R @ tr[0]['t']
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    F = unit(np.linalg.inv(K2).T @ tx @ R @ np.linalg.inv(K1))
    return xs[0], xs[1], F, bad, (K1, K2, R, t)
