"""Shared by tests/test_position_priors_host.py and tests/test_gpu_position_priors.py: the numpy reference of the position priors
(mvus_ba_set_position_priors) built on scipy.interpolate.BSpline.design_matrix, and the prior sets of the tests.  Host only.

A prior (t, p, w) adds the rows r = w (.) (S(t) - p); with h the four B-spline weights of its knot span on control points q .. q + 3
  cost += 0.5 sum r^2,   g[q + a] += h_a w^2 (S - p),   band block (q + a, q + b), a <= b, += h_a h_b diag(w^2)."""
import numpy as np
from scipy.interpolate import BSpline

EPS = np.finfo(np.float64).eps


def design(prob, t):
    """(ctrl[K], h[K, 4]) from scipy: ctrl = global index of the first control point of the knot span, -1 where t lies in no interval
    [start, end] (both ends closed); h = the four basis values of the span (design_matrix stores exactly k + 1 entries per row)."""
    t = np.asarray(t, dtype=np.float64)
    ctrl = np.full(t.size, -1, dtype=np.int64)
    h = np.zeros((t.size, 4))
    coff = prob.ctrl_offsets
    for s in range(prob.S):
        kn = prob.knots[int(prob.knot_offsets[s]):int(prob.knot_offsets[s + 1])]
        m = (t >= prob.interval[0, s]) & (t <= prob.interval[1, s])
        if not m.any():
            continue
        D = BSpline.design_matrix(t[m], kn, 3).tocsr()
        assert np.all(np.diff(D.indptr) == 4)
        ctrl[m] = coff[s] + D.indices[::4]
        h[m] = D.data.reshape(-1, 4)
    return ctrl, h


def ctrl_columns(prob):
    """col[g, d]: index in x of coordinate d of global control point g."""
    cols = []
    for s, n in enumerate(prob.n_coef):
        base = int(prob.spline_x_offsets[s])
        cols.append(base + np.arange(int(n))[:, None] + int(n) * np.arange(3)[None, :])
    return np.vstack(cols)


def rows(prob, x, t, P, w):
    """(cost, r[3, K] with NaN for inactive priors, ctrl, h, S[3, K])."""
    ctrl, h = design(prob, t)
    col = ctrl_columns(prob)
    K = np.size(t)
    S = np.full((3, K), np.nan)
    for k in np.nonzero(ctrl >= 0)[0]:
        S[:, k] = h[k] @ x[col[ctrl[k]:ctrl[k] + 4]]
    r = w * (S - P)
    return 0.5 * float(np.nansum(r * r)), r, ctrl, h, S


def contribution(prob, x, t, P, w, W):
    """What the priors add to the exported normal equations at x: dg[n], dband[N, W, 3, 3], and for the error bars of every entry the
    sum of |terms| (ag, aband) and the number of rows added into it (ng[n], nband[N, W, 3, 3]).  The terms of a gradient entry are the
    products that are actually summed, h_a w^2 h_q x_q (q = 0..3) and h_a w^2 p: S - p cancels (a prior sits within a few sigma of the
    curve), so the rounding of S, a few eps |S|, is what the entry inherits -- the same (|S| + |p|) the rows' own bar carries."""
    _, r, ctrl, h, S = rows(prob, x, t, P, w)
    col = ctrl_columns(prob)
    N = col.shape[0]
    dg, ag, ng = np.zeros(x.size), np.zeros(x.size), np.zeros(x.size, dtype=np.int64)
    dband, aband, nband = np.zeros((N, W, 3, 3)), np.zeros((N, W, 3, 3)), np.zeros((N, W, 3, 3), dtype=np.int64)
    order = np.argsort(t, kind='stable')                   # the library adds in (t, input order)
    for k in order:
        if ctrl[k] < 0:
            continue
        w2 = w[:, k] ** 2
        diff = S[:, k] - P[:, k]
        mag = np.abs(h[k]) @ np.abs(x[col[ctrl[k]:ctrl[k] + 4]]) + np.abs(P[:, k])
        for a in range(4):
            for d in range(3):
                term = h[k, a] * (w2[d] * diff[d])
                c = col[ctrl[k] + a, d]
                dg[c] += term
                ag[c] += abs(h[k, a]) * w2[d] * mag[d]
                ng[c] += 1
            for b in range(a, 4):
                for d in range(3):
                    term = h[k, a] * h[k, b] * w2[d]
                    dband[ctrl[k] + a, b - a, d, d] += term
                    aband[ctrl[k] + a, b - a, d, d] += abs(term)
                    nband[ctrl[k] + a, b - a, d, d] += 1
    return dg, dband, ag, aband, ng, nband


def gradient_from_rows(prob, n, t, w, r):
    """The priors' gradient from given rows r = w (S - p) (3, K; NaN = inactive): dg[n] = sum h_a w r over the rows in (t, input order),
    the sum of |terms| and the number of rows per entry.  With the DEVICE's rows (mvus_ba_position_prior_cost) the cancellation in S - p
    is out of the comparison, and what is left is what k_prior_ne itself does: the products and the ordered sum."""
    ctrl, h = design(prob, t)
    col = ctrl_columns(prob)
    dg, ag, ng = np.zeros(n), np.zeros(n), np.zeros(n, dtype=np.int64)
    for k in np.argsort(t, kind='stable'):
        if ctrl[k] < 0:
            continue
        for a in range(4):
            for d in range(3):
                term = h[k, a] * (w[d, k] * r[d, k])
                c = col[ctrl[k] + a, d]
                dg[c] += term
                ag[c] += abs(term)
                ng[c] += 1
    return dg, ag, ng


def scene_size(prob, x):
    """Largest extent of the control points along an axis: the unit the tests' sigmas are given in."""
    c = x[ctrl_columns(prob)]
    return float(np.max(c.max(axis=0) - c.min(axis=0)))


def curve(prob, x, t):
    """S(t) (3, K) of the splines in x at times inside the intervals."""
    return rows(prob, x, t, np.zeros((3, np.size(t))), np.ones((3, np.size(t))))[4]


def prior_sets(prob, x, seed=5):
    """The prior sets of the tests, {name: (t, P, w)}: positions are the curve of x plus N(0, sigma) noise, sigma = 1 % of the scene.
      one      K = 1
      three    K = 3
      span70   70 priors inside ONE knot span (the 64-row batch of a wavefront wraps)
      mixed    both exact ends of every interval, two rows outside every interval (between two intervals where there are two), one row
               with w_z = 0, two equal times -- in shuffled order."""
    rng = np.random.default_rng(seed)
    sigma = 0.01 * scene_size(prob, x)
    lo, hi = float(prob.interval[0, 0]), float(prob.interval[1, 0])

    def make(t, w=None):
        t = np.asarray(t, dtype=np.float64)
        act = design(prob, t)[0] >= 0
        P = np.zeros((3, t.size))
        P[:, act] = curve(prob, x, t[act])
        P += sigma * rng.standard_normal(P.shape)
        if w is None:
            w = np.full((3, t.size), 1.0 / sigma)
        return t, P, w
    kn = prob.knots[int(prob.knot_offsets[0]):int(prob.knot_offsets[1])]
    j = 3 + (kn.size - 8) // 2                               # an interior knot span of the first spline
    sets = {'one': make([lo + 0.37 * (hi - lo)]),
            'three': make(lo + np.array([0.11, 0.52, 0.93]) * (hi - lo)),
            'span70': make(kn[j] + (kn[j + 1] - kn[j]) * (np.arange(70) + 0.5) / 70.0)}
    ends = list(prob.interval[0]) + list(prob.interval[1])
    outside = [float(prob.interval[1, 0]) + 0.5 * (float(prob.interval[0, 1]) - float(prob.interval[1, 0])) if prob.S > 1 else lo - 3.0,
               float(prob.interval[1, -1]) + 2.5]
    tw = lo + 0.613 * (hi - lo)
    t = np.array(ends + outside + [tw, tw, lo + 0.3 * (hi - lo), lo + 0.31 * (hi - lo)])
    w = np.full((3, t.size), 1.0 / sigma)
    w[2, -1] = 0.0
    w[0, -2] = 0.5 / sigma
    t, P, w = make(t, w)
    perm = rng.permutation(t.size)
    sets['mixed'] = (t[perm], P[:, perm], w[:, perm])
    return sets
