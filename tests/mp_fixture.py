"""Reader of tests/golden/mp_jacobian.npz (the 50-digit reference of tests/golden/make_golden_mp_jacobian.py) and the bars shared by
tests/test_jacobian_exact_host.py and tests/test_gpu_jacobian_exact.py.  Needs numpy only."""
import os

import numpy as np

from mvus_amd import problem as mp

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'mp_jacobian.npz')
PROBLEM_FIELDS = ('det_offsets', 'frame', 'u_raw', 'v_raw', 'img_height', 'K', 'dist', 'interval', 'knot_offsets', 'knots')
FLAG_FIELDS = ('num_cam', 'opt_calib', 'undist_points', 'rs_free', 'rs_bounds', 'motion_reg', 'motion_type', 'opt_sync')
GROUPS_P6 = dict(sync=(0, 3), rvec=(3, 6), t=(6, 9), spline=(9, 21))
GROUPS_P15 = dict(sync=(0, 3), intrinsics=(3, 7), rvec=(7, 10), t=(10, 13), distortion=(13, 18), spline=(18, 30))

RESIDUAL_ATOL = 1e-9       # px: the project's own residual bar (README, "What 'parity' means here")
TOL_FACTOR = 8.0           # a different but sound evaluation order may lose a few more bits than the restatement, not orders of magnitude


def groups(P):
    return GROUPS_P15 if P == 15 else GROUPS_P6


def _ratio(diff, scale):
    ok = scale > 0
    return np.where(ok, diff / np.where(ok, scale, 1.0), np.where(diff > 0, np.inf, 0.0))


def group_ratio(J, Jref, P, per_row=False):
    """worst |J - Jref| / max |Jref| over the entry's slot group (sync / intrinsics / rvec / t / distortion / spline of ONE row and axis);
    J, Jref: [..., NS].  An entry of a group that is all zero in the reference must be zero."""
    worst = np.zeros(Jref.shape[:-1])
    for lo, hi in groups(P).values():
        scale = np.max(np.abs(Jref[..., lo:hi]), axis=-1, keepdims=True)
        r = _ratio(np.abs(J[..., lo:hi] - Jref[..., lo:hi]), scale)
        worst = np.maximum(worst, r.max(axis=-1))
    return worst if per_row else (float(worst.max()) if worst.size else 0.0)


def motion_ratio(mJ, mJref):
    """the same for motion rows: one group, the row's entries"""
    scale = np.max(np.abs(mJref), axis=-1, keepdims=True)
    r = _ratio(np.abs(mJ - mJref), scale)
    return float(r.max()) if r.size else 0.0


class Case:
    pass


def load(names=None):
    """{name: Case} with .prob (BAProblem), .x, .rows and the reference arrays of the file; plus the recorded floor."""
    out = {}
    with np.load(PATH) as z:
        floor = float(z['floor'])
        for name in [str(n) for n in z['names']]:
            if names is not None and name not in names:
                continue
            get = lambda k: z[name + '/' + k]
            fl = dict(zip(FLAG_FIELDS, (int(v) for v in get('flags'))))
            arr = {k: get(k) for k in PROBLEM_FIELDS}
            c = Case()
            c.name = name
            c.prob = mp.BAProblem(num_cam=fl['num_cam'], opt_calib=bool(fl['opt_calib']), undist_points=bool(fl['undist_points']),
                                  rs_free=bool(fl['rs_free']), rs_bounds=bool(fl['rs_bounds']), motion_reg=bool(fl['motion_reg']),
                                  motion_type=fl['motion_type'], motion_weight=float(get('motion_weight')), opt_sync=bool(fl['opt_sync']),
                                  **arr)
            c.x, c.rows, c.in_floor, c.floor = get('x'), get('rows'), bool(get('in_floor')), float(get('floor'))
            c.ex, c.ey, c.ctrl, c.J = get('ex'), get('ey'), get('ctrl'), get('J')
            c.has_motion = (name + '/mf') in z.files
            if c.has_motion:
                c.mf, c.mJ, c.mcidx = get('mf'), get('mJ'), get('mcidx')
            c.full = (name + '/H') in z.files
            if c.full:
                c.g, c.H = get('g'), get('H')
                c.ex53, c.ey53, c.mf53 = get('ex53'), get('ey53'), get('mf53')
            out[name] = c
    return out, floor


def camera_of(prob, i):
    return int(np.searchsorted(np.asarray(prob.det_offsets), i, side='right') - 1)


def control_columns(prob, ctrl):
    coff = np.asarray(prob.ctrl_offsets)
    s = int(np.searchsorted(coff, ctrl, side='right') - 1)
    n = int(prob.n_coef[s])
    j = int(ctrl) - int(coff[s])
    return [int(prob.spline_x_offsets[s]) + d * n + j + q for q in range(4) for d in range(3)]


def slot_columns(prob, c, ctrl):
    C, P = prob.C, prob.P
    return [c, C + c, 2 * C + c] + list(range(3 * C + c * P, 3 * C + (c + 1) * P)) + control_columns(prob, ctrl)


def dense_reference(case, plain=False):
    """f_ref[m], J_ref[m, n] of a case whose rows are ALL rows (the complete scenes), in the reference's row order; plain: f is the one
    the restatement gives at 53 bits."""
    p = case.prob
    ex, ey, mf_ = (case.ex53, case.ey53, case.mf53) if plain else (case.ex, case.ey, case.mf)
    assert case.rows.size == p.M
    f, J = np.zeros(p.n_residuals), np.zeros((p.n_residuals, p.n_params))
    for k, i in enumerate(case.rows):
        if case.ctrl[k] < 0:
            continue
        c = camera_of(p, i)
        a, b = int(p.det_offsets[c]), int(p.det_offsets[c + 1])
        cols = slot_columns(p, c, case.ctrl[k])
        rx, ry = 2 * a + (i - a), 2 * a + (b - a) + (i - a)
        f[rx], f[ry] = ex[k], ey[k]
        J[rx, cols], J[ry, cols] = case.J[k, 0], case.J[k, 1]
    if case.has_motion:
        J[2 * p.M:] = motion_dense(case, case.mJ, case.mcidx)
        f[2 * p.M:] = mf_
    return f, J


def motion_dense(case, mJ, mcidx):
    """36-entry motion rows scattered (added: the samples of one row share control points) into [T, n]"""
    p = case.prob
    out = np.zeros((mJ.shape[0], p.n_params))
    for j in range(mJ.shape[0]):
        for k in range(3):
            if mcidx[j, k] >= 0:
                np.add.at(out[j], control_columns(p, mcidx[j, k]), mJ[j, 12 * k:12 * k + 12])
    return out


def normal_floor(case):
    """What fp64 can do for H = J^T J and g = J^T f: numpy's own sums over the reference's rows (rounded to double) against the sums
    formed in mpmath; for g with the residuals of the 53-bit evaluation, since a residual is a difference of two pixels of ~1e3 whose
    roundings (~1e-13 px) no double-precision evaluation avoids."""
    f53, J_ref = dense_reference(case, plain=True)
    return normal_ratio(J_ref.T @ J_ref, J_ref.T @ f53, case.H, case.g)


def normal_ratio(H, g, Href, gref):
    """worst |H - Href| / sqrt(Href_ii Href_jj) and |g - gref| / max |gref|"""
    d = np.sqrt(np.abs(np.diag(Href)))
    scale = np.outer(d, d)
    return float(_ratio(np.abs(H - Href), scale).max()), float(np.max(np.abs(g - gref)) / np.max(np.abs(gref)))
