#!/usr/bin/env python3
"""Wall-clock of the two-view initialisation for one camera pair: Scene.init_traj and synchronization.sync_bf on the GPU
(warm-up done, a device synchronise inside the clock: every library call returns after its stream has drained), and, for
context, the numpy restatement of the same steps (tests/epipolar_oracle.py) on one CPU core.

    python tools/time_init.py [--scenes small,large] [--reps 3] [--no-oracle] [--json out.json]

small = synth.BASELINE_CONFIGS[1]-sized (7 cameras, 100k observations); large = a 2M-observation scene of the same shape
(its generator needs well over 200 GB of host memory at that knot spacing: not run so far).
Per-kernel times of k_fm_score (and the models x points it evaluates per second) come from a separate profiler run:

    rocprofv3 --kernel-trace --stats -d OUT -o run -- python tools/time_init.py --scenes small --reps 1 --no-oracle
"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
os.environ.setdefault('OMP_NUM_THREADS', '1')

import numpy as np  # noqa: E402


def build(total_obs):
    from mvus_amd import synth
    from mvus_amd.reconstruction import common
    kw = dict(synth.BASELINE_CONFIGS[1])
    kw.pop('total_obs')
    sc = synth.make_scene(total_obs=total_obs, **kw)
    s = common.Scene()
    s.numCam = sc.num_cam
    s.settings = dict(sc.settings)
    for c in sc.truth['cameras']:
        s.addCamera(common.Camera(K=c['K'].copy(), d=c['d'].copy(), fps=c['fps'], resolution=list(c['resolution'])))
    for det in sc.detections:
        s.addDetection(det.copy())
    s.alpha, s.beta, s.rs = sc.truth['alpha'].copy(), sc.truth['beta'].copy(), sc.truth['rs'].copy()
    s.find_order, s.ref_cam = True, 0
    s.detection_to_global()
    return s, sc


def clock(fn, reps):
    import torch
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), [round(t, 4) for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--scenes', default='small')
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--no-oracle', action='store_true')
    ap.add_argument('--json')
    a = ap.parse_args()
    from mvus_amd.reconstruction import synchronization as sync
    from mvus_amd.tools import util
    import epipolar_oracle as eo
    sizes = {'small': 100_000, 'large': 2_000_000}
    out = []
    for name in a.scenes.split(','):
        s, sc = build(sizes[name])
        cf = -sc.truth['beta'] / sc.truth['alpha']
        cf[1] += 3.0 * sc.cameras[1]['fps']
        run_init = lambda: s.init_traj(error=10)
        run_sync = lambda: sync.sync_bf(s.cameras[0].fps, s.cameras[1].fps, s.detections[0], s.detections[1], cf[0], cf[1])
        run_init(); run_sync()                                   # warm-up: library load, code objects, allocator
        t1, t2 = s.sequence
        if s.cameras[t1].fps > s.cameras[t2].fps:
            d1, d2 = util.match_overlap(s.detections_global[t1], s.detections_global[t2])
        else:
            d2, d1 = util.match_overlap(s.detections_global[t2], s.detections_global[t1])
        row = dict(scene=name, observations=int(sc.num_obs), pair=[int(t1), int(t2)], pairs=int(d1.shape[1]))
        row['init_traj_s'], row['init_traj_reps'] = clock(run_init, a.reps)
        row['sync_bf_s'], row['sync_bf_reps'] = clock(run_sync, a.reps)
        if not a.no_oracle:
            t0 = time.perf_counter()
            F, _, _ = eo.fundamental_ransac(d1[1:], d2[1:], 10)
            row['oracle_fundamental_ransac_s'] = time.perf_counter() - t0
            n = min(d1.shape[1], 2000)
            t0 = time.perf_counter()
            eo.correct_matches(F, d1[1:, :n], d2[1:, :n])
            row['oracle_correct_matches_s_per_1k'] = (time.perf_counter() - t0) / n * 1000
        print(json.dumps(row))
        out.append(row)
    if a.json:
        with open(a.json, 'w') as fh:
            json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
