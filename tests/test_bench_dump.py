"""bench.py --dump-outputs on the host: what is written, in which dtype, and the seeded sample above the size limit."""
import os
import sys
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402


def _result(n):
    return SimpleNamespace(x=np.linspace(-1.0, 1.0, n), cost=12.5, initial_cost=13.0, optimality=0.25, nfev=2, njev=2, status=1)


def test_dump_writes_the_result_as_float64(tmp_path):
    res = _result(1000)
    bench.dump_outputs(str(tmp_path), res)
    names = sorted(f[:-4] for f in os.listdir(str(tmp_path)))
    assert names == ['cost', 'initial_cost', 'nfev', 'njev', 'optimality', 'status', 'x']
    x = np.load(str(tmp_path / 'x.npy'))
    assert x.dtype == np.float64 and np.array_equal(x, res.x)
    for name in names[:-1]:
        a = np.load(str(tmp_path / (name + '.npy')))
        assert a.dtype == np.float64 and a.shape == (1,) and a[0] == getattr(res, name)


def test_dump_samples_above_the_limit_the_same_way_every_time(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, 'DUMP_LIMIT_BYTES', 4096)
    res = _result(10000)
    for d in ('a', 'b'):
        bench.dump_outputs(str(tmp_path / d), res)
    total = sum(os.path.getsize(str(tmp_path / 'a' / f)) for f in os.listdir(str(tmp_path / 'a')))
    assert total <= 4096 + 8 * 128                    # (plus one .npy header per file)
    xa, ia = np.load(str(tmp_path / 'a' / 'x.npy')), np.load(str(tmp_path / 'a' / 'x_sample_idx.npy'))
    assert np.array_equal(xa, res.x[ia.astype(np.int64)])
    assert np.array_equal(xa, np.load(str(tmp_path / 'b' / 'x.npy')))
    assert np.array_equal(ia, np.load(str(tmp_path / 'b' / 'x_sample_idx.npy')))
