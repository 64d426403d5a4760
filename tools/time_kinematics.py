#!/usr/bin/env python
"""Wall time of the three kinematics calls (mvus_spline_eval_der, mvus_spline_kin_cov_eval, mvus_spline_length: upload, kernels and read-back
of one stateless call) on the golden trajectory (tests/golden/traj_spline.npz, two splines) at 1e5 and 2e6 samples, beside
scipy.interpolate.splev(der=0, 1, 2) on one core for the same samples.

    python tools/time_kinematics.py [--samples 100000 2000000] [--repeats 3] [--out profiles/kinematics_times.txt]

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


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument('--samples', type=int, nargs='+', default=[100000, 2000000])
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args(argv)
    import numpy as np
    from scipy.interpolate import splev
    from mvus_amd import spline
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'traj_spline.npz'))
    S = int(g['n_int'])
    tck = [[g['knots_%d' % i], list(g['coefs_%d' % i]), 3] for i in range(S)]
    interval = g['interval']
    N = sum(len(k[0]) - 4 for k in tck)
    rng = np.random.default_rng(0)
    A = rng.standard_normal((N, 4, 3, 3))
    band = A + A.transpose(0, 1, 3, 2)                       # (any numbers do: the time does not depend on them)
    lines = ['golden trajectory: %d splines, %d control points' % (S, N)]
    for nt in a.samples:
        ts = np.sort(rng.uniform(interval[0, 0], interval[1, -1], nt))
        inside = [ts[(ts >= interval[0, s]) & (ts <= interval[1, s])] for s in range(S)]

        def scipy_all():
            for s in range(S):
                for der in (0, 1, 2):
                    splev(inside[s], (tck[s][0], tck[s][1], 3), der=der)
        rows = [('mvus_spline_eval_der (nder 2)', median_ms(lambda: spline.evaluate_der(tck, interval, ts), a.repeats)),
                ('mvus_spline_kin_cov_eval (nder 2)', median_ms(lambda: spline.kin_cov_evaluate(tck, interval, band, ts), a.repeats)),
                ('mvus_spline_length', median_ms(lambda: spline.path_length(tck, interval, ts), a.repeats)),
                ('scipy splev(der=0, 1, 2), one core', median_ms(scipy_all, a.repeats))]
        lines.append('%d samples (%d inside an interval)' % (nt, sum(v.size for v in inside)))
        for name, ms in rows:
            lines.append('  %-38s %10.3f ms' % (name, ms))
    text = '\n'.join(lines)
    print(text)
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write(text + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
