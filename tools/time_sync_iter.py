#!/usr/bin/env python3
"""Wall-clock of the iterative time-shift search for one camera pair at the synth.BASELINE_CONFIGS[1] size (7 cameras, 100k
observations: about 14 000 detections per camera), against the numpy / scipy restatement (tests/sync_iter_oracle.py) on one CPU core.

    python tools/time_sync_iter.py [--reps 5] [--H 200] [--oracle-h 10] [--no-oracle] [--json out.json]

Stages (every library call returns after its stream has drained, so the clock needs no further synchronisation):
  open      the two host splines (scipy splprep), find_intervals and the upload: once per camera pair
  round     mvus_sync_iter_round: both signs, 2 x H hypotheses, up to 12 H models, every model against every detection, selection
  models    mvus_sync_iter_models: one sign of the same with all per-model outputs read back
  score     mvus_sync_iter_score: 6 H models handed in, scored against every detection (upload + the scoring kernel + read-back)
  search    synchronization.sync_iter_gpu from start to finish (open included)
The oracle runs ONE round with --oracle-h hypotheses per sign; its time per hypothesis is what a round of H costs it.
Per-kernel times come from a separate profiler run:

    rocprofv3 --kernel-trace --stats -d OUT -o run -- python tools/time_sync_iter.py --reps 1 --no-oracle
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


def clock(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--H', type=int, default=200)
    ap.add_argument('--oracle-h', type=int, default=10)
    ap.add_argument('--moved', type=float, default=20.0)
    ap.add_argument('--no-oracle', action='store_true')
    ap.add_argument('--json')
    a = ap.parse_args()
    from mvus_amd import synth
    from mvus_amd.reconstruction import synchronization as sync
    import sync_iter_oracle as so
    sc = synth.baseline_scene(1)
    tr = sc.truth
    cf = -np.asarray(tr['beta'], dtype=np.float64) / np.asarray(tr['alpha'], dtype=np.float64)
    cf[1] += a.moved
    fps1, fps2 = sc.cameras[0]['fps'], sc.cameras[1]['fps']
    det1, det2 = np.asarray(sc.detections[0], dtype=np.float64), np.asarray(sc.detections[1], dtype=np.float64)
    prep = so.prepare(fps1, fps2, det1, det2, cf[0], cf[1])
    shift, H, thr = prep['beta_prior'], a.H, 10.0
    row = dict(detections=[int(det1.shape[1]), int(det2.shape[1])], H=H, moved=a.moved)
    sync.SyncIterSession(prep['d1'], det2).close()                 # warm-up: library load, code objects
    row['open_s'] = clock(lambda: sync.SyncIterSession(prep['d1'], det2).close(), a.reps)
    with sync.SyncIterSession(prep['d1'], det2) as S:
        sync._round(S, shift, 1, H, thr, 0, 0)
        row['round_s'] = clock(lambda: sync._round(S, shift, 1, H, thr, 0, 0), a.reps)
        n = prep['n'] - 2
        idx = np.array([so.sample9(0, 0, 0, h, n) for h in range(H)], dtype=np.int64)
        betas, valid, F, counts = sync.sync_iter_models(S, shift, 1, idx, thr)
        row['models_s'] = clock(lambda: sync.sync_iter_models(S, shift, 1, idx, thr), a.reps)
        Fs, ms = F.reshape(-1, 3, 3), (betas * 1.0).reshape(-1)
        Fs[~valid.reshape(-1)] = np.eye(3)                         # every slot scored: 6 H models x N1 detections
        sync.sync_iter_score(S, shift, Fs, ms, thr)
        row['score_s'] = clock(lambda: sync.sync_iter_score(S, shift, Fs, ms, thr), a.reps)
        row['score_models'] = int(Fs.shape[0])
        row['score_evaluations_per_s'] = Fs.shape[0] * det1.shape[1] / row['score_s']
        row['valid_models_per_sign'] = int(valid.sum())
    run = lambda: sync.sync_iter_gpu(fps1, fps2, det1, det2, cf[0], cf[1], maxIter=H)
    beta, ratio = run()
    row['search_s'] = clock(run, max(1, a.reps // 2))
    row['beta_error_frames'] = float(beta - tr['beta'][1])
    row['inlier_ratio'] = float(ratio)
    if not a.no_oracle:
        t0 = time.perf_counter()
        so.round_(prep, shift, 1, a.oracle_h, thr, 0, 0)
        row['oracle_round_s_per_hypothesis'] = (time.perf_counter() - t0) / (2 * a.oracle_h)
        row['oracle_round_s_at_H'] = row['oracle_round_s_per_hypothesis'] * 2 * H
    print(json.dumps(row))
    if a.json:
        with open(a.json, 'w') as fh:
            json.dump(row, fh, indent=1)


if __name__ == '__main__':
    main()
