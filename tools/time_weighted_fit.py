#!/usr/bin/env python
"""Wall time of the weighted smoothing fit beside the unweighted one, and of triangulate_with_cov beside triangulate_with_errors.

    python tools/time_weighted_fit.py [--samples 5000 560000] [--pairs 22020] [--repeats 5] [--unweighted-only] [--out FILE]

Per sample count: a trajectory (the curve of tests/test_traj_to_spline.py; the long one 50x oversampled, as the trajectories traj_to_spline
fits) with noise of sigma = 2e-5 on 70 % of the samples and 1e-4 on the rest, w = 2e-5 / sigma -- samples of a spline out of a BA next to
a few raw points: traj_fit starts at s = 1e-6 x duration, and noise above that drives its loop through fits close to interpolation.
Timed are one fit inside an open SmoothFit session at s = the expected weighted residual sum (the work arrays warm), and the whole of traj_fit (open, the smooth_factor loop,
close).  The weighted fit reads m more doubles in two kernels per pass; the knot sets differ, so the number of passes does too -- the line
says how many knots each fit ended on.  ``--unweighted-only`` times only what a checkout without the weighted fit has.
Every figure is the median of ``repeats`` calls after one warm-up call."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median_ms(fn, repeats):
    import numpy as np
    fn()
    ts = []
    for _ in range(max(repeats, 1)):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def trajectory(m, seed=0):
    import numpy as np
    rng = np.random.default_rng(seed)
    rate = 1.0 if m <= 20000 else 0.02                     # the long one: samples every 0.02 frames
    u = np.cumsum(rng.uniform(0.5, 1.5, m)) * rate
    sig = np.where(rng.uniform(size=m) < 0.3, 1e-4, 2e-5)
    X = np.vstack([10 * np.sin(u / 80), 10 * np.cos(u / 95), 30 + 3 * np.sin(u / 50)]) + rng.normal(size=(3, m)) * sig
    return u, X, sig


def camera_pair(baseline=5.0):
    import numpy as np
    K = np.array([[1500.0, 0.0, 960.0], [0.0, 1500.0, 540.0], [0.0, 0.0, 1.0]])
    target = np.array([3.0, 40.0, 25.0])

    def look_at(C):
        z = (target - C) / np.linalg.norm(target - C)
        x = np.cross([0.0, 0.0, 1.0], z)
        x /= np.linalg.norm(x)
        R = np.vstack((x, np.cross(z, x), z))
        return K @ np.hstack((R, (-R @ C)[:, None]))
    return look_at(np.zeros(3)), look_at(np.array([baseline, 0.0, 0.5])), target


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument('--samples', type=int, nargs='+', default=[5000, 560000])
    ap.add_argument('--pairs', type=int, default=22020)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--unweighted-only', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args(argv)
    import numpy as np
    from mvus_amd import spline
    from mvus_amd.reconstruction import epipolar as ep
    lines = []

    def say(line):
        lines.append(line)
        print(line, flush=True)
        if a.out:
            with open(a.out, 'w') as fh:
                fh.write('\n'.join(lines) + '\n')
    for m in a.samples:
        try:
            u, X, sig = trajectory(m)
        except MemoryError:
            say('%d samples: not enough host memory' % m)
            continue
        part = np.vstack((u, X))
        kinds = [('unweighted', None)] + ([] if a.unweighted_only else [('weighted', 2e-5 / sig)])
        say('%d samples' % m)
        for label, w in kinds:
            kw = {} if w is None else {'w': w}
            s = 3 * float(np.sum(((1.0 if w is None else w) * sig) ** 2))
            with spline.SmoothFit(u, X, **kw) as fit:
                knots = len(fit(s)[0])
                one = median_ms(lambda: fit(s), a.repeats)
            loop_knots = len(spline.traj_fit(part, [10, 20], **kw)[0])
            loop = median_ms(lambda: spline.traj_fit(part, [10, 20], **kw), a.repeats)
            say('  %-10s one fit in a session (s = %.4g, %d knots) %9.3f ms    traj_fit, smooth_factor [10, 20] (%d knots) %9.3f ms'
                % (label, s, knots, one, loop_knots, loop))
    P1, P2, target = camera_pair()
    rng = np.random.default_rng(1)
    Xw = np.vstack((target[:, None] + 2.0 * rng.standard_normal((3, a.pairs)), np.ones((1, a.pairs))))
    x1, x2 = P1 @ Xw, P2 @ Xw
    x1, x2 = x1[:2] / x1[2] + 0.7 * rng.standard_normal((2, a.pairs)), x2[:2] / x2[2] + 0.7 * rng.standard_normal((2, a.pairs))
    say('%d pairs' % a.pairs)
    say('  %-24s %9.3f ms' % ('triangulate_with_errors', median_ms(lambda: ep.triangulate_with_errors(x1, x2, P1, P2), a.repeats)))
    if not a.unweighted_only:
        say('  %-24s %9.3f ms' % ('triangulate_with_cov', median_ms(lambda: ep.triangulate_with_cov(x1, x2, P1, P2, 0.7, 0.7), a.repeats)))
    return 0


if __name__ == '__main__':
    sys.exit(main())
