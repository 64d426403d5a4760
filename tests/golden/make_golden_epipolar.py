#!/usr/bin/env python3
"""Golden vectors for the two-view initialisation (Scene.init_traj), produced by the REAL reference on a seeded synthetic pair:

  * ``epipolar.compute_Rt_from_E`` (reconstruction/epipolar.py:513-539): the four [R|t] candidates of the true E;
  * ``epipolar.triangulate_from_E`` (epipolar.py:568-588): the chosen P2 and the triangulated points;
  * ``epipolar.Sampson_error`` (epipolar.py:258-265) of the true F on the pairs.

The pairs are two cameras of this repo's generator (tests/epipolar_oracle.synthetic_pair, 300 pairs, sigma 0.5 px, no
outliers).  Run in the build container only (needs the reference checkout):  python tests/golden/make_golden_epipolar.py
Stores data only (the inputs and the reference's outputs) in tests/golden/epipolar_2cam.npz."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import import_reference   # noqa: E402


def main():
    import epipolar_oracle as eo
    import_reference()
    from reconstruction import epipolar as ep
    x1, x2, F, _, (K1, K2, R, t) = eo.synthetic_pair(300, sigma=0.5, outliers=0.0, seed=7)
    E = K2.T @ F @ K1
    h1, h2 = np.vstack((x1, np.ones(x1.shape[1]))), np.vstack((x2, np.ones(x2.shape[1])))
    Rt = ep.compute_Rt_from_E(E)
    X, P2 = ep.triangulate_from_E(E, K1, K2, h1, h2)
    out = dict(x1=x1, x2=x2, F=F, E=E, K1=K1, K2=K2, R_true=R, t_true=t, Rt=np.stack(Rt), X=X, P2=P2,
               sampson=ep.Sampson_error(h1, h2, F))
    path = os.path.join(HERE, 'epipolar_2cam.npz')
    np.savez_compressed(path, **out)
    print('P2 =\n%s\nwrote %s (%.1f KiB)' % (P2, path, os.path.getsize(path) / 1024))


if __name__ == '__main__':
    main()
