"""High-precision restatement of one bundle-adjustment row, written with mpmath from the reference's semantics
(multiviewunsynch/reconstruction/common.py, tools/util.py, FITPACK splev, cv2.Rodrigues, cv2.undistortPoints):

    detection row   tau = alpha (frame + rs v_raw / H) + beta ; start <= tau < end ; t[l] <= tau < t[l+1] (clamped) ;
                    Cox-de Boor ; cv2.Rodrigues ; x = K [R t] X, x /= x[2] ; observed = K undistortPoints(raw) ;
                    |x_cal - x_obs| per axis
    motion row      Scene.error_motion(motion_reg=True) + motion_prior ('F', 'KE', eps = 1e-20)

Derivatives are forward-mode dual numbers carried through the same text, one tangent per slot of the row layout
(alpha, beta, rs, the P camera parameters, 12 spline slots), so they are the derivatives of the unrolled five undistortion
iterations.  The sign of the signed residual is applied at the end.  Every function works at mpmath's CURRENT precision:
50 digits (``with mpmath.workdps(50)``) for the reference, ``mpmath.workprec(53)`` for a plain-fp64 evaluation of this text.
It shares no code with mvus_amd/csrc/ba_math.h or oracle/ba_oracle.py.
"""
import mpmath
import numpy as np
from mpmath import mpf

from mp_fixture import camera_of, control_columns, slot_columns

DPS = 50
DBL_EPSILON = 2.220446049250313e-16


class Dual:
    """value + sparse tangent {slot: derivative}"""
    __slots__ = ('v', 'd')

    def __init__(self, v, d=None):
        self.v = v if isinstance(v, mpf) else mpf(v)
        self.d = d if d is not None else {}

    @staticmethod
    def lift(a):
        return a if isinstance(a, Dual) else Dual(a)

    def __neg__(self):
        return Dual(-self.v, {k: -t for k, t in self.d.items()})

    def __add__(self, o):
        o = Dual.lift(o)
        d = dict(self.d)
        for k, t in o.d.items():
            d[k] = d[k] + t if k in d else t
        return Dual(self.v + o.v, d)
    __radd__ = __add__

    def __sub__(self, o):
        return self + (-Dual.lift(o))

    def __rsub__(self, o):
        return Dual.lift(o) + (-self)

    def __mul__(self, o):
        o = Dual.lift(o)
        d = {k: t * o.v for k, t in self.d.items()}
        for k, t in o.d.items():
            d[k] = d[k] + self.v * t if k in d else self.v * t
        return Dual(self.v * o.v, d)
    __rmul__ = __mul__

    def __truediv__(self, o):
        o = Dual.lift(o)
        q = self.v / o.v
        d = {k: t / o.v for k, t in self.d.items()}
        for k, t in o.d.items():
            d[k] = d[k] - q * t / o.v if k in d else -q * t / o.v
        return Dual(q, d)

    def __rtruediv__(self, o):
        return Dual.lift(o) / self

    def chain(self, value, slope):
        return Dual(value, {k: slope * t for k, t in self.d.items()})


def dsqrt(a):
    r = mpmath.sqrt(a.v)
    return a.chain(r, 1 / (2 * r))


def dsin(a):
    return a.chain(mpmath.sin(a.v), mpmath.cos(a.v))


def dcos(a):
    return a.chain(mpmath.cos(a.v), -mpmath.sin(a.v))


def seeded(value, slot=None):
    return Dual(mpf(float(value)), {slot: mpf(1)} if slot is not None else {})


def rodrigues(r):
    """cv2.Rodrigues, vector -> matrix: theta = |r|; theta < DBL_EPSILON gives the identity (whose derivative is the three
    generators); otherwise R = cos I + (1 - cos) k k^T + sin [k]x with k = r / theta."""
    th2 = r[0] * r[0] + r[1] * r[1] + r[2] * r[2]
    if mpmath.sqrt(th2.v) < DBL_EPSILON:
        z = Dual(0)
        gen = [[z, -r[2], r[1]], [r[2], z, -r[0]], [-r[1], r[0], z]]
        return [[Dual(mpf(1 if i == j else 0), dict(gen[i][j].d)) for j in range(3)] for i in range(3)]
    th = dsqrt(th2)
    c, s = dcos(th), dsin(th)
    k = [ri / th for ri in r]
    cross = [[Dual(0), -k[2], k[1]], [k[2], Dual(0), -k[0]], [-k[1], k[0], Dual(0)]]
    return [[(c if i == j else Dual(0)) + (1 - c) * k[i] * k[j] + s * cross[i][j] for j in range(3)] for i in range(3)]


def fitpack_span(t, tau):
    """splev.f: l with t[l] <= tau < t[l+1], searched upwards from the first span and clamped to the last one (0-based l in [3, n-1],
    n coefficients)."""
    n = len(t) - 4
    l = 3
    while l < n - 1 and tau >= t[l + 1]:
        l += 1
    return l


def basis_on_span(t, l, x):
    """The four cubic B-splines B_{l-3..l,3} at x, for x treated as a member of span l: the Cox-de Boor recurrence
    B_{i,p} = (x - t_i) / (t_{i+p} - t_i) B_{i,p-1} + (t_{i+p+1} - x) / (t_{i+p+1} - t_{i+1}) B_{i+1,p-1}, 0/0 = 0, degree by degree."""
    B = {l: Dual(1)}                                   # degree 0: indicator of span l
    for p in range(1, 4):
        Bn = {}
        for i in range(l - p, l + 1):
            acc = Dual(0)
            if i in B and t[i + p] != t[i]:
                acc = acc + (x - t[i]) / (t[i + p] - t[i]) * B[i]
            if (i + 1) in B and t[i + p + 1] != t[i + 1]:
                acc = acc + (t[i + p + 1] - x) / (t[i + p + 1] - t[i + 1]) * B[i + 1]
            Bn[i] = acc
        B = Bn
    return [B[l - 3 + q] for q in range(4)]


def undistort_points(x0, y0, k1, k2, p1, p2, k3):
    """cv2.undistortPoints on normalised coordinates, no termination criteria: five fixed-point iterations; OpenCV >= 4.1.1 leaves the
    point at its start and stops when 1 / (1 + k1 r^2 + k2 r^4 + k3 r^6) is negative.  Returns x, y and the smallest |1 + k1 r^2 + ..|
    met (the caller's guard against a branch decided by rounding)."""
    x, y = x0, y0
    guard = None
    for _ in range(5):
        r2 = x * x + y * y
        den = 1 + ((k3 * r2 + k2) * r2 + k1) * r2
        guard = abs(den.v) if guard is None else min(guard, abs(den.v))
        icdist = 1 / den
        if icdist.v < 0:
            x, y = x0, y0
            break
        dx = 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
        dy = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
        x = (x0 - dx) * icdist
        y = (y0 - dy) * icdist
    return x, y, guard


def detection_row(prob, x, i):
    """Row pair of detection i (camera-segmented index): dict(ex, ey, ctrl, jx[NS], jy[NS], guard) in mpf.
    guard: the undistortion's smallest |denominator|; tau: the exact time stamp."""
    C, P = prob.C, prob.P
    NS = 3 + P + 12
    c = camera_of(prob, i)
    sync = bool(getattr(prob, 'opt_sync', True))
    alpha = seeded(x[c], 0 if sync else None)
    beta = seeded(x[C + c], 1 if sync else None)
    rs = seeded(x[2 * C + c], 2 if prob.rs_free else None)
    v = x[3 * C + c * P:3 * C + (c + 1) * P]
    if prob.opt_calib:
        fx, fy, cx, cy = (seeded(v[k], 3 + k) for k in range(4))
        rvec = [seeded(v[4 + k], 7 + k) for k in range(3)]
        tvec = [seeded(v[7 + k], 10 + k) for k in range(3)]
        dist = [seeded(v[10 + k], 13 + k) for k in range(5)]
    else:
        fx, fy, cx, cy = (seeded(prob.K[c][k]) for k in range(4))
        rvec = [seeded(v[k], 3 + k) for k in range(3)]
        tvec = [seeded(v[3 + k], 6 + k) for k in range(3)]
        dist = [seeded(prob.dist[c][k]) for k in range(5)]
    frame, u_raw, v_raw = (mpf(float(a[i])) for a in (prob.frame, prob.u_raw, prob.v_raw))
    H = mpf(float(prob.img_height[c]))
    tau = alpha * (frame + rs * v_raw / H) + beta
    zero = dict(ex=mpf(0), ey=mpf(0), ctrl=-1, jx=[mpf(0)] * NS, jy=[mpf(0)] * NS, guard=mpf(1), tau=tau.v)
    s = -1
    guard = mpf(1)
    for k in range(prob.S):
        if mpf(float(prob.interval[0, k])) <= tau.v < mpf(float(prob.interval[1, k])):
            s = k
    if s < 0:
        return zero
    koff = [int(o) for o in prob.knot_offsets]
    t = [mpf(float(q)) for q in prob.knots[koff[s]:koff[s + 1]]]
    n = len(t) - 4
    l = fitpack_span(t, tau.v)
    xoff = int(prob.spline_x_offsets[s])
    base = 3 + P
    X = [Dual(0), Dual(0), Dual(0)]
    Bq = basis_on_span(t, l, tau)
    for q in range(4):
        for d in range(3):
            X[d] = X[d] + Bq[q] * seeded(x[xoff + d * n + (l - 3 + q)], base + 3 * q + d)
    R = rodrigues(rvec)
    Xc = [R[r][0] * X[0] + R[r][1] * X[1] + R[r][2] * X[2] + tvec[r] for r in range(3)]
    # x = K [R t] X ; x /= x[2]
    hom = [fx * Xc[0] + cx * Xc[2], fy * Xc[1] + cy * Xc[2], Xc[2]]
    u_cal, v_cal = hom[0] / hom[2], hom[1] / hom[2]
    if prob.undist_points:
        xn, yn, g = undistort_points((u_raw - cx) / fx, (v_raw - cy) / fy, *dist)
        guard = min(guard, g)
        u_obs, v_obs = fx * xn + cx, fy * yn + cy
        if not prob.opt_calib:                                     # undistorted once, with the fixed calibration: a constant
            u_obs, v_obs = Dual(u_obs.v), Dual(v_obs.v)
    else:
        u_obs, v_obs = Dual(u_raw), Dual(v_raw)
    ru, rv = u_cal - u_obs, v_cal - v_obs
    su, sv = (-1 if ru.v < 0 else 1), (-1 if rv.v < 0 else 1)
    return dict(ex=abs(ru.v), ey=abs(rv.v), ctrl=int(prob.ctrl_offsets[s]) + l - 3,
                jx=[su * ru.d.get(k, mpf(0)) for k in range(NS)], jy=[sv * rv.d.get(k, mpf(0)) for k in range(NS)],
                guard=guard, tau=tau.v)


def motion_samples(prob):
    """Scene.spline_to_traj(): timestamps np.arange(int[0,0], int[1,-1], 1), kept per interval where start <= t <= end (closed),
    and util.sampling(belong=True): the interval each one is a half-open member of (-1: none).  Returns ts, spline, part."""
    iv = np.asarray(prob.interval, dtype=np.float64)
    grid = np.arange(iv[0, 0], iv[1, -1], 1)
    ts, spl, part = [], [], []
    for s in range(iv.shape[1]):
        for tt in grid[np.logical_and(grid >= iv[0, s], grid <= iv[1, s])]:
            ts.append(float(tt))
            spl.append(s)
            mem = [k for k in range(iv.shape[1]) if iv[0, k] <= tt < iv[1, k]]
            part.append(mem[0] if mem else -1)
    return ts, spl, part


def _sample_point(prob, x, s, tt):
    """splev of spline s at tt with the four active control points seeded 3 q + d; also their first global index."""
    koff = [int(o) for o in prob.knot_offsets]
    t = [mpf(float(q)) for q in prob.knots[koff[s]:koff[s + 1]]]
    n = len(t) - 4
    tau = mpf(tt)
    l = fitpack_span(t, tau)
    xoff = int(prob.spline_x_offsets[s])
    Bq = basis_on_span(t, l, Dual(tau))
    X = [Dual(0), Dual(0), Dual(0)]
    for q in range(4):
        for d in range(3):
            X[d] = X[d] + Bq[q] * seeded(x[xoff + d * n + (l - 3 + q)], 3 * q + d)
    return X, int(prob.ctrl_offsets[s]) + l - 3


def _shift(a, off):
    return Dual(a.v, {k + off: t for k, t in a.d.items()})


def motion_rows(prob, x):
    """Every row of the motion block (unmasked): list of dict(f, j36[36], cidx[3], guard); entry 12 k + 3 q + d of j36 is the derivative
    w.r.t. coordinate d of control point q of sample j-1+k.  guard: smallest |r_d| of the row's three signed terms."""
    eps = mpf('1e-20')
    w = mpf(float(prob.motion_weight))
    ts, spl, part = motion_samples(prob)
    T = len(ts)
    pts = [_sample_point(prob, x, spl[j], ts[j]) for j in range(T)]
    rows = [dict(f=mpf(0), j36=[mpf(0)] * 36, cidx=[-1, -1, -1], guard=mpf(1)) for _ in range(T)]
    ke = prob.motion_type == 1
    for s in range(prob.S):
        mem = [j for j in range(T) if part[j] == s]                # traj[:, idx == s + 1]
        if not mem:
            continue
        targets = mem[1:] if ke else mem[1:-1]
        for pos, j in enumerate(targets, start=1):
            terms = []
            if ke:
                a, b = mem[pos - 1], mem[pos]
                dt = mpf(ts[b]) - mpf(ts[a])
                for d in range(3):
                    vel = (_shift(pts[b][0][d], 12) - pts[a][0][d]) / (dt + eps)
                    terms.append(w * 0.5 * (vel * vel * dt))
                cidx = [pts[a][1], pts[b][1], -1]
            else:
                a, b, e = mem[pos - 1], mem[pos], mem[pos + 1]
                dt1 = mpf(ts[b]) - mpf(ts[a])
                dt2 = mpf(ts[e]) - mpf(ts[b])
                dt3 = dt1 + dt2
                for d in range(3):
                    mid = _shift(pts[b][0][d], 12)
                    v1 = (mid - pts[a][0][d]) / (dt1 + eps)
                    v2 = (_shift(pts[e][0][d], 24) - mid) / (dt2 + eps)
                    accel = (v2 - v1) / (dt3 + eps)
                    terms.append(w * (accel * dt3))
                cidx = [pts[a][1], pts[b][1], pts[e][1]]
            j36 = [mpf(0)] * 36
            f = mpf(0)
            for r in terms:
                sg = -1 if r.v < 0 else 1
                f += abs(r.v)
                for k, tk in r.d.items():
                    j36[k] = j36[k] + sg * tk
            rows[j] = dict(f=f, j36=j36, cidx=cidx, guard=min(abs(r.v) for r in terms))
    return rows


def normal_equations(prob, det_rows, mot_rows):
    """g = J^T f and H = J^T J summed in mpmath over the given rows (det_rows: {i: detection_row}, mot_rows: motion_rows)."""
    n = prob.n_params
    g = [mpf(0)] * n
    H = {}
    def add(cols, jac, f):
        nz = [(col, v) for col, v in zip(cols, jac) if v != 0]
        for ca, va in nz:
            g[ca] += va * f
            for cb, vb in nz:
                H[(ca, cb)] = H.get((ca, cb), mpf(0)) + va * vb
    for i, r in det_rows.items():
        if r['ctrl'] < 0:
            continue
        cols = slot_columns(prob, camera_of(prob, i), r['ctrl'])
        add(cols, r['jx'], r['ex'])
        add(cols, r['jy'], r['ey'])
    for r in mot_rows:
        cols, jac = [], []
        for k in range(3):
            if r['cidx'][k] >= 0:
                cols += control_columns(prob, r['cidx'][k])
                jac += r['j36'][12 * k:12 * k + 12]
        # samples of one row share control points: their entries fall on the same column and add up
        merged = {}
        for col, v in zip(cols, jac):
            merged[col] = merged.get(col, mpf(0)) + v
        add(list(merged.keys()), list(merged.values()), r['f'])
    Hd = np.zeros((n, n))
    for (a, b), v in H.items():
        Hd[a, b] = float(v)
    return np.array([float(v) for v in g]), Hd
