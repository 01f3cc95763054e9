"""bench.py's --dump-outputs writer and its argument checks, without a GPU."""
import os
import subprocess
import sys

import numpy as np
import torch

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_writes_float32_and_a_fixed_sample_of_large_arrays(tmp_path, monkeypatch):
    small = torch.arange(6, dtype=torch.float16).reshape(2, 3)
    big = torch.arange(1000, dtype=torch.float32)
    monkeypatch.setattr(bench, 'DUMP_MAX_ELEMS', 100)
    bench.dump_outputs(str(tmp_path / 'a'), small=small, big=big)
    bench.dump_outputs(str(tmp_path / 'b'), big=big)
    s = np.load(str(tmp_path / 'a' / 'small.npy'))
    assert s.dtype == np.float32 and np.array_equal(s, small.float().numpy())
    a, b = np.load(str(tmp_path / 'a' / 'big.npy')), np.load(str(tmp_path / 'b' / 'big.npy'))
    assert a.dtype == np.float32 and a.shape == (100,)
    assert np.array_equal(a, b)                      # the same elements in every run
    assert np.all(np.diff(a) > 0)                    # distinct elements, in their original order


def test_dump_budget_holds_the_whole_flagship_output():
    assert 16 * 3 * 512 * 512 <= bench.DUMP_MAX_ELEMS and bench.DUMP_MAX_ELEMS * 4 <= 64e6


def test_bad_arguments_are_refused_before_any_gpu_work(tmp_path):
    for flags in (['--steps', '0'], ['--mode', 'train', '--dump-outputs', str(tmp_path / 'x')]):
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py')] + flags, cwd=ROOT,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 2 and 'error' in r.stderr, (flags, r.stderr[-2000:])
    assert not os.path.exists(str(tmp_path / 'x'))
