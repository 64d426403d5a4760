#!/usr/bin/env python3
"""Wall-clock of BAHandle.register_cameras on the GPU at the camera size of bench.py's configs[2] (32 cameras, 500k observations: about
15.6k detections per camera, 5000 knots): one camera registered against the held trajectory

    B = 1            one start
    B = 41           one camera x 41 beta starts (a beta search of +-20 frames, step 1) in ONE call
    41 x (B = 1)     the same 41 starts as single calls

Every call returns after its one read-back, so the clock needs no extra synchronisation.  Stages: the schedule is fixed, so with every
tolerance at 0 a call runs exactly max_nfev evaluations, and two budgets give the cost of one round (decode + linearise + decide/solve)
and of the fixed part (uploads, first evaluation, counts, read-back); `converged` is the call as a user makes it (default tolerances).

    python tools/time_register.py [--config 2] [--camera 1] [--reps 5] [--json out.json]

Per-kernel times come from a separate profiler run:

    rocprofv3 --kernel-trace --stats -d OUT -o run -- python tools/time_register.py --reps 1
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', type=int, default=2)
    ap.add_argument('--camera', type=int, default=1)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--json')
    a = ap.parse_args()
    from mvus_amd import problem as mp
    from mvus_amd import synth
    from mvus_amd.ba import BAHandle
    sc = synth.baseline_scene(a.config)
    prob, x = mp.problem_from_scene(sc)
    C, P, cam = prob.C, prob.P, a.camera
    v = np.concatenate(([x[cam], x[C + cam], x[2 * C + cam]], x[3 * C + cam * P:3 * C + (cam + 1) * P]))
    starts = np.repeat(v[None], 41, axis=0)
    starts[:, 1] += np.arange(-20, 21)
    cams41 = np.full(41, cam, dtype=np.int32)
    row = dict(config=a.config, camera=cam, detections=int(prob.det_offsets[cam + 1] - prob.det_offsets[cam]), cameras=C, observations=int(prob.M))
    zero = dict(ftol=0.0, xtol=0.0, gtol=0.0)
    with BAHandle(prob) as h:
        h.register_cameras(x, cams41, start=starts)                       # warm-up: code objects, work buffers
        h.register_cameras(x, [cam], start=starts[20:21])
        for name, cams, st in (('B1', [cam], starts[20:21]), ('B41', cams41, starts)):
            res = h.register_cameras(x, cams, start=st)
            row[name + '_converged_ms'] = clock(lambda: h.register_cameras(x, cams, start=st), a.reps)
            row[name + '_nfev_max'] = int(res.nfev.max())
            t10 = clock(lambda: h.register_cameras(x, cams, start=st, max_nfev=10, **zero), a.reps)
            t50 = clock(lambda: h.register_cameras(x, cams, start=st, max_nfev=50, **zero), a.reps)
            row[name + '_round_ms'] = (t50 - t10) / 40.0
            row[name + '_fixed_ms'] = t10 - 9.0 * row[name + '_round_ms']
            row[name + '_50_rounds_ms'] = t50
            row[name + '_linearize_ms'] = clock(lambda: h.register_linearize(x, cams, start=st), a.reps)
        row['41_single_calls_converged_ms'] = clock(lambda: [h.register_cameras(x, [cam], start=starts[k:k + 1]) for k in range(41)], a.reps)
    print(json.dumps(row))
    if a.json:
        with open(a.json, 'w') as fh:
            json.dump(row, fh, indent=1)


if __name__ == '__main__':
    main()
