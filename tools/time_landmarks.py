#!/usr/bin/env python3
"""Times of the landmark passes on the GPU at bench.py's configs[2] (32 cameras, 500k observations, 5000 knots), 20 landmarks seen by
every camera (640 observations) and again with 4096 observations per camera:

    set          BAHandle.set_landmarks (sort, uploads, k_landmark_setup when the calibration is fixed), wall clock
    cost_kernel  k_landmark_cost alone          } between two HIP events on the handle's stream, back-to-back launches
    ne_kernel    k_landmark_ne alone            } (mvus_ba_time_kernel, which = 7 / 8)
    step         one LM iteration of a solve with the landmarks in force and without them: (t(max_nfev = 12) - t(max_nfev = 2)) / 10,
                 tolerances at 0 so that every call runs its budget

    python tools/time_landmarks.py [--config 2] [--reps 5] [--json out.json]

Per-launch times of the three kernels come from a separate profiler run:

    rocprofv3 --kernel-trace --stats -d OUT -o run -- python tools/time_landmarks.py --reps 1
"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def clock(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3


def landmark_set(prob, x, per_camera, seed=1):
    """``per_camera`` landmarks around the trajectory's centroid, every one seen by every camera at its projection + U(-3, 3) px"""
    from mvus_amd import problem as mp
    rng = np.random.default_rng(seed)
    _, _, _, cams, coefs = mp.unpack_x(prob, x)
    ctrl = np.hstack([np.vstack(c) for c in coefs])
    centre, spread = ctrl.mean(axis=1), ctrl.std(axis=1).max()
    X = centre[:, None] + spread * rng.uniform(-1, 1, (3, per_camera))
    cam = np.repeat(np.arange(prob.C), per_camera)
    point = np.tile(np.arange(per_camera), prob.C)
    uv = np.zeros((2, cam.size))
    for c in range(prob.C):
        K = cams[c]['K'] if prob.opt_calib else np.array([[prob.K[c][0], 0, prob.K[c][2]], [0, prob.K[c][1], prob.K[c][3]], [0, 0, 1.0]])
        Xc = cams[c]['R'] @ X + np.ravel(cams[c]['t'])[:, None]
        uv[0, cam == c] = K[0, 0] * Xc[0] / Xc[2] + K[0, 2]
        uv[1, cam == c] = K[1, 1] * Xc[1] / Xc[2] + K[1, 2]
    uv += rng.uniform(-3, 3, uv.shape)
    return X, cam, point, uv


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', type=int, default=2)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--json')
    a = ap.parse_args()
    from mvus_amd import _lib
    from mvus_amd import problem as mp
    from mvus_amd import synth
    from mvus_amd.ba import BAHandle
    sc = synth.baseline_scene(a.config)
    prob, x = mp.problem_from_scene(sc)
    row = dict(config=a.config, cameras=int(prob.C), observations=int(prob.M), P=int(prob.P))
    lm = dict(solver=_lib.SOLVER_LM_SCHUR, jac_mode=_lib.JAC_ANALYTIC)

    def step_ms(h):
        def run(nfev):
            opts = _lib.default_opts(lm['solver'], lm['jac_mode'], nfev)
            opts.ftol = opts.xtol = opts.gtol = 0.0
            return clock(lambda: h.solve(x, opts=opts, return_fun=False), a.reps)
        return (run(12) - run(2)) / 10.0
    with BAHandle(prob) as h:
        h.solve(x, max_nfev=3, return_fun=False, **lm)                      # warm-up: code objects, work buffers
        row['step_ms_without'] = step_ms(h)
        for per in (20, 4096):
            X, cam, point, uv = landmark_set(prob, x, per)
            tag = 'K%d' % cam.size
            h.set_landmarks(X, cam, point, uv, 1.0)
            row[tag + '_set_ms'] = clock(lambda: h.set_landmarks(X, cam, point, uv, 1.0), a.reps)
            h.set_x(x)
            row[tag + '_cost_kernel_us'] = 1e3 * h.time_kernel(7, launches=50)
            row[tag + '_ne_kernel_us'] = 1e3 * h.time_kernel(8, launches=50)
            row[tag + '_landmark_cost'] = h.landmark_cost(x)
            row[tag + '_step_ms'] = step_ms(h)
        h.set_landmarks(None, None, None, None, None)
        row['step_ms_without_again'] = step_ms(h)
    print(json.dumps(row))
    if a.json:
        with open(a.json, 'w') as fh:
            json.dump(row, fh, indent=1)


if __name__ == '__main__':
    main()
