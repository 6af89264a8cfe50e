"""bench.py's host-side pieces that need no device: the --dump-outputs writer and the --steps check."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bytes(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def test_dump_outputs_writes_float64_arrays_whole_when_they_fit(tmp_path):
    import bench
    rng = np.random.RandomState(0)
    vj, vk = rng.rand(1, 10), rng.rand(1, 4, 4).astype(np.float32)
    bench._dump_outputs(str(tmp_path), [('vj_tril', vj), ('vk', vk)])
    assert sorted(os.listdir(tmp_path)) == ['vj_tril.npy', 'vk.npy']
    a, b = np.load(tmp_path / 'vj_tril.npy'), np.load(tmp_path / 'vk.npy')
    assert a.dtype == b.dtype == np.float64 and np.array_equal(a, vj) and np.array_equal(b, vk)


def test_dump_outputs_samples_larger_outputs_the_same_way_every_run(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, 'DUMP_BYTES', 1 << 20)
    vj, vk = np.arange(60000.0).reshape(1, -1), -np.arange(250000.0).reshape(1, 500, 500)      # 2.48 MB together
    for d in ('a', 'b'):
        bench._dump_outputs(str(tmp_path / d), [('vj_tril', vj), ('vk', vk)])
    assert sorted(os.listdir(tmp_path / 'a')) == ['vj_tril_sample.npy', 'vk_sample.npy']
    assert _bytes(tmp_path / 'a') <= 1 << 20
    for f in ('vj_tril_sample.npy', 'vk_sample.npy'):
        s = np.load(tmp_path / 'a' / f)
        assert np.array_equal(s, np.load(tmp_path / 'b' / f)) and s.dtype == np.float64 and s.size > 0
        assert len(np.unique(s)) == s.size                      # distinct elements, each taken from the array as it is
    assert set(np.load(tmp_path / 'a' / 'vk_sample.npy')) <= set(vk.ravel())


def test_bench_refuses_zero_steps():
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--steps', '0'], capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and '--steps' in p.stderr
