#!/usr/bin/env python
"""Time of mvus_ba_detection_covariance: the eight stages of the covariance chain (mvus_ba_covariance_stage_ms, stage 6 now storing T), the
detection pass (mvus_ba_detection_covariance_ms, HIP events inside the library), the bytes that pass must move and what share of the HBM
peak that is -- at the benchmark configurations configs[1] and configs[2] of mvus_amd.synth.BASELINE_CONFIGS, gauge anchored.  For the
comparison the stages of plain mvus_ba_covariance on the same handle are printed beside them (stage 6 without the store).

    python tools/time_detection_covariance.py [--configs 1 2] [--repeats 3] [--out profiles/detection_covariance_times.txt]

Bytes of the pass, from the shapes: per detection its 2 NS Jacobian slots read and 2 + 3 + 1 doubles written (2 NS + 6 doubles), plus what
the detections share -- per distinct (camera, span) the 12 x B slice of T, per distinct span the ten 3 x 3 band blocks, per camera its
B x B block of Sigma_cc.  Share of peak = those bytes / 8.0 TB/s (the HBM3E figure of the MI355X) / the pass's time: the pass is bound by
bytes, not by its 2 (B^2 + 12 B + 144) multiply-adds per detection.  The first call on a handle allocates the buffers; the times printed
are those of the LAST of ``repeats`` calls."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

HBM_PEAK = 8.0e12        # bytes / s


def pass_bytes(prob, ctrl):
    """(bytes per detection stream, bytes of the shared slices) of the detection pass from the problem's shapes and the spans."""
    import numpy as np
    B, NS = 3 + prob.P, 3 + prob.P + 12
    cam = np.repeat(np.arange(prob.C), np.diff(prob.det_offsets))
    vis = ctrl >= 0
    pairs = np.unique(np.stack((cam[vis], ctrl[vis])), axis=1).shape[1]
    spans = np.unique(ctrl[vis]).size
    stream = 8 * (2 * NS + 6) * int(prob.M)
    shared = 8 * (12 * B * pairs + 90 * spans + B * B * prob.C)
    return stream, shared


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument('--configs', type=int, nargs='+', default=[1, 2])
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args(argv)
    from mvus_amd import _lib, problem as mp, synth
    from mvus_amd.ba import BAHandle
    from time_covariance import anchor_mask
    lines = []
    for k in a.configs:
        sc = synth.baseline_scene(k)
        prob, x0 = mp.problem_from_scene(sc)
        N = int(prob.n_coef.sum())
        with BAHandle(prob) as h:
            h.set_frozen(anchor_mask(prob, x0))
            note, plain, stages, det_ms, wall = '', [], [], None, 0.0
            for _ in range(max(a.repeats, 1)):
                try:
                    h.covariance(x0)
                except ValueError:
                    pass
                plain = h.covariance_stage_ms()
                t0 = time.perf_counter()
                try:
                    dc = h.detection_covariance(x0)
                    note = 'dof %d, sigma2 %.6g' % (dc.dof, dc.sigma2)
                except ValueError as e:          # refused (the whole chain has run all the same: its times stand)
                    note = 'REFUSED: %s' % e
                wall = (time.perf_counter() - t0) * 1e3
                stages = h.covariance_stage_ms()
                det_ms = h.detection_covariance_ms()
            _, _, ctrl = h.residual_jacobian(x0, _lib.JAC_ANALYTIC)
        stream, shared = pass_bytes(prob, ctrl)
        lines.append('configs[%d]: C %d, CB %d, N %d (3N = %d), M %d, %s' % (k, prob.C, prob.C * (3 + prob.P), N, 3 * N, prob.M, note))
        for (name, ms), (_, ms0) in zip(stages, plain):
            lines.append('  %-28s %10.3f ms   (plain covariance() %10.3f ms)' % (name, ms, ms0))
        lines.append('  %-28s %10.3f ms   (plain covariance() %10.3f ms; wall time of the call %.3f ms, read-back included)'
                     % ('all stages', sum(ms for _, ms in stages), sum(ms for _, ms in plain), wall))
        s6, s6p = stages[5][1], plain[5][1]
        lines.append('  stage 6 with T stored / without: %.3f' % (s6 / s6p if s6p > 0 else float('nan')))
        lines.append('  %-28s %10.3f ms' % ('detection pass', det_ms))
        total = stream + shared
        lines.append('  bytes of the pass: %d per-detection + %d shared = %.3f MB; at %.1f TB/s that is %.3f us = %.2f %% of the pass (bound: bytes)'
                     % (stream, shared, total / 1e6, HBM_PEAK / 1e12, total / HBM_PEAK * 1e6, 100.0 * (total / HBM_PEAK) / (det_ms * 1e-3) if det_ms else float('nan')))
    text = '\n'.join(lines)
    print(text)
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write(text + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
