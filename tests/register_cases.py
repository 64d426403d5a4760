"""The registration problems that tests/test_register_host.py solves with the host loop and scipy, and that tests/test_gpu_register.py
solves again on the device: scenes from synth.make_scene(4, 4000, perturb=0.0), camera 2 started from its true entries perturbed by
0.5 degrees in rvec, 0.3 m in t and 1 frame in beta.  The scipy reference of a case is computed once per process."""
import functools
from types import SimpleNamespace

import numpy as np

import register_hostcheck_util as ru
from mvus_amd import problem as mp
from mvus_amd import synth

CAM = 2
MARGIN = 20.0          # frames every detection must keep from the ends of the spline's interval at every point visited
TRIM = 25.0            # the camera's detections are cut this far inside the interval at the true time stamps
CASES = {
    'p6': dict(seed=11),
    'p6_rs_bounds': dict(seed=12, rolling_shutter=True, rs_bounds=True),
    'p15_Kd_held': dict(seed=13, opt_calib=True),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """A namespace: prob, x (the truth), start (3 + P), held (bool[3 + P]), free (bool[3 + P]: neither held nor switched off)."""
    kw = dict(CASES[name])
    sc = synth.make_scene(4, 4000, perturb=0.0, **kw)
    # make_scene lets every camera see the target up to the very ends of the interval; the comparison needs a visibility that does
    # not change between the points two different solvers visit
    d = sc.detections[CAM]
    tau = sc.truth['alpha'][CAM] * (d[0] + sc.truth['rs'][CAM] * d[2] / 1080.0) + sc.truth['beta'][CAM]
    sc.detections[CAM] = d[:, (tau >= sc.interval[0, 0] + TRIM) & (tau <= sc.interval[1, -1] - TRIM)]
    prob, x = mp.problem_from_scene(sc)
    P = prob.P
    truth = ru.camera_vector(prob, x, CAM)
    start = truth.copy()
    o = 3 + (4 if prob.opt_calib else 0)                       # first entry of rvec
    start[1] += 1.0
    start[o:o + 3] += np.deg2rad(0.5) * np.array([1.0, -1.0, 1.0]) / np.sqrt(3.0)
    start[o + 3:o + 6] += 0.3 * np.array([1.0, 1.0, -1.0]) / np.sqrt(3.0)
    held = np.zeros(3 + P, dtype=bool)
    if prob.opt_calib:
        held[3:7] = True
        held[13:18] = True
    free = ~held
    if not prob.rs_free:
        free[2] = False
    return SimpleNamespace(name=name, scene=sc, prob=prob, x=x, truth=truth, start=start, held=held, free=free, interval=sc.interval.copy())


def sigma_at(c, v):
    """1-sigma of the free entries at the camera vector v: s^2 (J^T J)^-1 with s^2 = 2 cost / (rows - free unknowns)."""
    _, _, cost, vis, R = ru.linearize(c.prob, c.x, CAM, v, held=ru.held_bits(c.held), rows=True)
    n = 3 + c.prob.P
    J = R[:, :n][:, c.free]
    s2 = 2.0 * cost / (2 * vis - int(c.free.sum()))
    return np.sqrt(np.diag(s2 * np.linalg.inv(J.T @ J)))


@functools.lru_cache(maxsize=None)
def scipy_reference(name):
    """scipy.optimize.least_squares (trf, x_scale='jac', every tolerance 1e-14) on the rows of the host build: a namespace with params
    (3 + P), cost, status, sigma (free entries) and tau_range over every point scipy evaluated."""
    from scipy.optimize import least_squares
    c = case(name)
    n = 3 + c.prob.P
    d0, d1 = int(c.prob.det_offsets[CAM]), int(c.prob.det_offsets[CAM + 1])
    frame, vraw, Himg = c.prob.frame[d0:d1], c.prob.v_raw[d0:d1], c.prob.img_height[CAM]
    tr = [np.inf, -np.inf]
    memo = {}

    def rows(vf):
        key = vf.tobytes()
        if key not in memo:
            v = c.start.copy()
            v[c.free] = vf
            tau = v[0] * (frame + v[2] * vraw / Himg) + v[1]
            tr[0], tr[1] = min(tr[0], tau.min()), max(tr[1], tau.max())
            memo.clear()
            memo[key] = ru.linearize(c.prob, c.x, CAM, v, held=ru.held_bits(c.held), rows=True)[4]
        return memo[key]

    lb, ub = np.full(n, -np.inf), np.full(n, np.inf)
    if c.prob.rs_bounds:
        lb[2], ub[2] = 0.0, 1.0
    res = least_squares(lambda vf: rows(vf)[:, n].copy(), c.start[c.free], jac=lambda vf: rows(vf)[:, :n][:, c.free].copy(), method='trf',
                        x_scale='jac', ftol=1e-14, xtol=1e-14, gtol=1e-14, bounds=(lb[c.free], ub[c.free]), max_nfev=400)
    v = c.start.copy()
    v[c.free] = res.x
    return SimpleNamespace(params=v, cost=float(res.cost), status=int(res.status), nfev=int(res.nfev), sigma=sigma_at(c, v), tau_range=np.array(tr))


HOST_OPTS = dict(max_nfev=50, ftol=1e-8, xtol=1e-12, gtol=1e-8)      # the defaults of BAHandle.register_cameras: the loop stops on a
                                                                     # step whose gain is far above rounding, so host and device stop alike


@functools.lru_cache(maxsize=None)
def host_solution(name):
    c = case(name)
    return ru.solve_problem(c.prob, c.x, CAM, c.start, held=ru.held_bits(c.held), **HOST_OPTS)
