"""numpy restatement of the two-view geometry of csrc/epipolar.hip.h, for the tests (CPU and GPU) and tools/time_init.py.

Independent of the kernels' own formulation where it can be: the 7-point null space from np.linalg.svd (the kernels use
Gauss-Jordan elimination), the degree-6 Hartley-Sturm polynomial solved by np.roots (companion-matrix eigenvalues; the kernels
use Aberth iteration), E decomposed by np.linalg.svd.  What must agree exactly is restated exactly: the counter-based sampler,
the error of a pair (same expression, same order, no fused operations) and the 7-point cubic's root rule (cubic_roots)."""
import math

import numpy as np

EPS = float(np.finfo(np.float64).eps)
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


def _cubic_polish(c, r):
    f = lambda x: ((c[0] * x + c[1]) * x + c[2]) * x + c[3]
    out = []
    for x in r:
        for _ in range(2):
            fx, df = f(x), (3.0 * c[0] * x + 2.0 * c[1]) * x + c[2]
            if df == 0.0:
                break
            xn = x - fx / df
            if not math.isfinite(xn) or not abs(f(xn)) <= abs(fx):
                break
            x = xn
        out.append(x)
    return out


def _quadratic_roots(q2, q1, q0):
    e = math.frexp(max(abs(q2), abs(q1), abs(q0)))[1] - 1            # ilogb
    q2, q1, q0 = math.ldexp(q2, -e), math.ldexp(q1, -e), math.ldexp(q0, -e)
    disc, tol = q1 * q1 - 4.0 * q2 * q0, 16.0 * EPS * (q1 * q1 + 4.0 * abs(q2 * q0))
    if disc < -tol:
        return []
    if disc <= tol:
        return [-0.5 * q1 / q2]
    q = -0.5 * (q1 + (math.sqrt(disc) if q1 >= 0.0 else -math.sqrt(disc)))
    return [q / q2] if q == 0.0 else [q / q2, q0 / q]


def cubic_roots(c3, c2, c1, c0, delta=0.0):
    """fm_cubic_roots' rule: the real roots of c3 l^3 + c2 l^2 + c1 l + c0 -- the quadratic below the 1e-12 cutoff, else the
    largest closed-form root, the cubic deflated by it and the quadratic's roots, a discriminant within 16 eps of its terms being
    a double root returned once.  The closed form is the kernel's: np.roots has no such rule (it gives an exact double root an
    imaginary part of ~1e-8 and keeps or drops near-double pairs by its own rounding)."""
    c3, c2, c1, c0 = float(c3), float(c2), float(c1), float(c0)
    c = (c3, c2, c1, c0)
    mx = max(abs(c3), abs(c2), abs(c1), abs(c0))
    if not mx > 0.0:
        return []
    if abs(c3) <= 1e-12 * mx:
        if abs(c2) <= 1e-12 * mx:
            return [] if abs(c1) <= 1e-12 * mx else _cubic_polish(c, [-c0 / c1])
        return _cubic_polish(c, _quadratic_roots(c2, c1, c0))
    a, b, cc = c2 / c3, c1 / c3, c0 / c3
    Q, R = (a * a - 3.0 * b) / 9.0, (2.0 * a * a * a - 9.0 * a * b + 27.0 * cc) / 54.0
    Q3 = Q * Q * Q
    if R * R < Q3:
        th, sq = math.acos(min(1.0, max(-1.0, R / math.sqrt(Q3)))), -2.0 * math.sqrt(Q)
        t = [sq * math.cos(th / 3.0) - a / 3.0, sq * math.cos((th + 2.0 * math.pi) / 3.0) - a / 3.0,
             sq * math.cos((th - 2.0 * math.pi) / 3.0) - a / 3.0]
        x0 = t[0]
        for v in t[1:]:
            if abs(v) > abs(x0):
                x0 = v
    else:
        A = float(np.cbrt(abs(R) + math.sqrt(R * R - Q3)))
        if R > 0.0:
            A = -A
        B = Q / A if A != 0.0 else 0.0
        x0 = A + B - a / 3.0
    x0, = _cubic_polish(c, [x0])
    if x0 != 0.0 and abs(x0) * x0 * x0 * abs(c3) >= abs(c0):
        q0 = -c0 / x0
        q1 = (q0 - c1) / x0
    else:
        q1 = c2 + c3 * x0
        q0 = c1 + q1 * x0
    r = _quadratic_roots(c3, q1, q0)
    if not r and delta > 0.0:
        xm = -0.5 * (q1 / c3)
        ax = abs(xm)
        if abs(((c3 * xm + c2) * xm + c1) * xm + c0) <= delta * (((ax + 1.0) * ax + 1.0) * ax + 1.0):
            r = [xm]
    return [x0] + _cubic_polish(c, r)


def seven_point(x1n, x2n):
    """The 7-point algorithm on 7 normalised pairs: the models (3x3, unnormalised scale) for the real roots of the cubic."""
    A = _rows(x1n, x2n)
    _, S, Vt = np.linalg.svd(A)
    # rank < 7 (duplicated pairs): no model.  The kernel's test is a Gauss-Jordan pivot (best > 1e-10 max|A|), not a singular
    # value: the two agree on rank-deficient samples and can differ only on samples within ~1e-10 of rank 6
    if not S[6] > 1e-10 * S[0]:
        return []
    F1, F2 = Vt[-2].reshape(3, 3), Vt[-1].reshape(3, 3)
    Ms = [l * F1 + (1 - l) * F2 for l in (0.0, 1.0, -1.0, 2.0)]
    d = [np.linalg.det(M) for M in Ms]
    A_ = [np.abs(M).reshape(9) for M in Ms]
    pmax = max(a[0] * (a[4] * a[8] + a[5] * a[7]) + a[1] * (a[3] * a[8] + a[5] * a[6]) + a[2] * (a[3] * a[7] + a[4] * a[6]) for a in A_)
    c0 = d[0]
    c2 = 0.5 * (d[1] + d[2]) - c0
    s = 0.5 * (d[1] - d[2])
    c3 = (d[3] - 4 * c2 - c0 - 2 * s) / 6.0
    c1 = s - c3
    return [l * F1 + (1 - l) * F2 for l in cubic_roots(c3, c2, c1, c0, 128.0 * EPS * pmax)]


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


# ---- edge-case builders (tests/test_epipolar_host.py, tests/test_gpu_epipolar_edges.py) ------------------------------------------
def ransac_case(N, kind, seed):
    """x1, x2 (2 x N pixels) of one RANSAC edge case: 'outliers' (30 % gross outliers), 'clean' (noise-free: every exact model
    ties and the lowest index wins), 'offset' (both views moved by thousands of px), 'dup' (every fifth pair a copy of its
    neighbour: samples with duplicated points, degenerate 7-point systems)."""
    if kind == 'outliers':
        x1, x2, _, _, _ = synthetic_pair(N, sigma=0.5, outliers=0.3, seed=seed)
    elif kind == 'clean':
        x1, x2, _, _, _ = synthetic_pair(N, sigma=0.0, outliers=0.0, seed=seed)
    elif kind == 'offset':
        x1, x2, _, _, _ = synthetic_pair(N, sigma=0.5, outliers=0.1, seed=seed)
        x1 = x1 + np.array([[4000.0], [-2500.0]])
        x2 = x2 + np.array([[-3000.0], [6000.0]])
    else:
        x1, x2, _, _, _ = synthetic_pair(N, sigma=0.5, outliers=0.2, seed=seed)
        m = x1[:, 1::5].shape[1]
        x1[:, 1::5] = x1[:, 0::5][:, :m]
        x2[:, 1::5] = x2[:, 0::5][:, :m]
    return np.ascontiguousarray(x1), np.ascontiguousarray(x2)


def random_rotation(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def skew(t):
    return np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])


def scene_for_candidate(P2, N, rng):
    """N noise-free normalised pairs (x1, x2: 2 x N) and their points X (3 x N) in front of P1 = [I|0] and of P2 = [R|t]:
    drawn from a ball around the two centres and kept where both depths are clearly positive."""
    X = np.zeros((3, 0))
    C2 = -P2[:, :3].T @ P2[:, 3]
    r = 20.0 * max(1.0, float(np.linalg.norm(C2)))
    for _ in range(100):
        Y = rng.uniform(-r, r, (3, 8 * N + 64))
        d2 = P2[2, :3] @ Y + P2[2, 3]
        ok = (Y[2] > 0.05 * np.linalg.norm(Y, axis=0)) & (d2 > 0.05 * np.linalg.norm(Y - C2[:, None], axis=0))
        X = np.hstack((X, Y[:, ok]))
        if X.shape[1] >= N:
            break
    assert X.shape[1] >= N, 'no points in front of both cameras'
    X = X[:, :N]
    y = P2[:, :3] @ X + P2[:, 3:4]
    return X[:2] / X[2], y[:2] / y[2], X


def cheirality_counts(E, x1n, x2n):
    """The four counts sum(d1 > 0) + sum(d2 > 0) of pose_from_essential, in rt_from_E's order."""
    P1 = np.hstack((np.eye(3), np.zeros((3, 1))))
    out = []
    for cand in rt_from_E(E):
        X = triangulate_dlt(x1n, x2n, P1, cand)
        out.append(int(np.sum(X[2] > 0) + np.sum((cand @ X)[2] > 0)))
    return out


def translation_F(K, t):
    """F of two cameras K [I|0], K [I|t] (pure translation): K^-T [t]_x K^-1, unit norm."""
    Ki = np.linalg.inv(K)
    return unit(Ki.T @ skew(t) @ Ki)


def epipoles(F):
    """(e1, e2): F e1 = 0, e2^T F = 0, unit vectors (SVD)."""
    return _epipoles(np.asarray(F, dtype=np.float64).reshape(3, 3))


def hs_infinity_case(f1, f2, a, d, x1, x2, angle1=0.0, angle2=0.0):
    """F, e1, e2 of a pair (x1, x2 pixels) whose Hartley-Sturm minimum is exactly at t = infinity: H&Z's canonical G with
    b = c = 0 (the cost t^2 / (1 + f1^2 t^2) + d^2 / (a^2 t^2 + f2^2 d^2) falls monotonically in t^2 when f1 > f2), moved to
    the points and rotated by the given angles."""
    G = np.array([[f1 * f2 * d, 0.0, -f2 * d], [0.0, a, 0.0], [-f1 * d, 0.0, d]])

    def frame(x, ang):
        T = np.array([[1.0, 0.0, -x[0]], [0.0, 1.0, -x[1]], [0.0, 0.0, 1.0]])
        R = np.array([[np.cos(ang), np.sin(ang), 0.0], [-np.sin(ang), np.cos(ang), 0.0], [0.0, 0.0, 1.0]])
        return R @ T
    M1, M2 = frame(x1, angle1), frame(x2, angle2)
    F = M2.T @ G @ M1
    e1 = np.linalg.solve(M1, np.array([1.0, 0.0, f1]))
    e2 = np.linalg.solve(M2, np.array([1.0, 0.0, f2]))
    return F, e1 / np.linalg.norm(e1), e2 / np.linalg.norm(e2)
