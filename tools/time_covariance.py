#!/usr/bin/env python
"""Time of mvus_ba_covariance per stage (HIP events inside the library: mvus_ba_covariance_stage_ms) at the benchmark
configurations configs[1] and configs[2] of mvus_amd.synth.BASELINE_CONFIGS, gauge anchored.

    python tools/time_covariance.py [--configs 1 2] [--repeats 3] [--out profiles/covariance_stage_times.txt]

The first call on a handle allocates the chain's buffers; the times printed are those of the LAST of ``repeats`` calls."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def anchor_mask(prob, x0):
    """The trivial gauge over the head of x: the pose of camera 0 and the largest translation component of camera 1 (a component the
    scaling about the first camera moves, as Scene.ba_frozen_mask chooses it from the cameras' centres)."""
    import numpy as np
    C, P = prob.C, prob.P
    mask = np.zeros(C * (3 + P), dtype=bool)
    pose0 = 4 if P == 15 else 0
    mask[3 * C + pose0:3 * C + pose0 + 6] = True
    t1 = x0[3 * C + P + pose0 + 3:3 * C + P + pose0 + 6]
    mask[3 * C + P + pose0 + 3 + int(np.argmax(np.abs(t1)))] = True
    return mask


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument('--configs', type=int, nargs='+', default=[1, 2])
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args(argv)
    from mvus_amd import problem as mp, synth
    from mvus_amd.ba import BAHandle
    lines = []
    for k in a.configs:
        sc = synth.baseline_scene(k)
        prob, x0 = mp.problem_from_scene(sc)
        N = int(prob.n_coef.sum())
        with BAHandle(prob) as h:
            h.set_frozen(anchor_mask(prob, x0))
            note = ''
            for _ in range(max(a.repeats, 1)):
                t0 = time.perf_counter()
                try:
                    cv = h.covariance(x0)
                    note = 'dof %d, sigma2 %.6g' % (cv.dof, cv.sigma2)
                except ValueError as e:          # refused (the whole chain has run all the same: its times stand)
                    note = 'REFUSED: %s' % e
                wall = (time.perf_counter() - t0) * 1e3
            stages = h.covariance_stage_ms()
        lines.append('configs[%d]: C %d, CB %d, N %d (3N = %d), M %d, %s' % (k, prob.C, prob.C * (3 + prob.P), N, 3 * N, prob.M, note))
        for name, ms in stages:
            lines.append('  %-28s %10.3f ms' % (name, ms))
        lines.append('  %-28s %10.3f ms   (wall time of the call %.3f ms, read-back included)' % ('all stages', sum(ms for _, ms in stages), wall))
    text = '\n'.join(lines)
    print(text)
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write(text + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
