"""CPU-only: bench.py's command line and its --dump-outputs writer (the step itself needs the MI355X)."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location('bench_for_test', os.path.join(ROOT, 'bench.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_steps_must_be_positive():
    """--steps sets the number of timed steps; zero would divide ms_per_step by zero, so it is refused before any GPU call."""
    for args in (['--steps', '0'], ['--warmup', '-1']):
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py')] + args, capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and '--steps must be >= 1' in r.stderr, (args, r.returncode, r.stderr[-400:])


def test_dump_outputs_writes_float32_sample(tmp_path):
    """dump_outputs: float32 .npy files, the full loss / loss parts / moving statistics, the weight and gradient arenas at the
    same seeded positions on every call, at most 64 MB in all."""
    bench = _bench()
    n = bench.DUMP_SAMPLE + 12345

    class Plan:
        loss4 = torch.tensor([1.0, 2.0, 3.0, 4.0])

    class Model:
        arena_floats = n
        params = torch.arange(n, dtype=torch.float32)
        grads = -torch.arange(n, dtype=torch.float32)
        moving = torch.ones(300)

        def _plan(self, batch, training):
            assert (batch, training) == (bench.BATCH, True)
            return Plan

    outs = []
    for d in (tmp_path / 'a', tmp_path / 'b'):
        bench.dump_outputs(str(d), Model(), torch.tensor(7.5))
        outs.append({f[:-4]: np.load(str(d / f)) for f in sorted(os.listdir(str(d)))})
        assert sum(os.path.getsize(str(d / f)) for f in os.listdir(str(d))) <= 64 << 20
    a, b = outs
    assert sorted(a) == ['grads_sample', 'loss', 'loss_parts', 'moving_stats', 'weights_sample']
    assert all(v.dtype == np.float32 for v in a.values())
    assert float(a['loss']) == 7.5 and a['loss_parts'].tolist() == [1, 2, 3, 4] and a['moving_stats'].shape == (300,)
    w = a['weights_sample']
    assert w.shape == (bench.DUMP_SAMPLE,) and np.all(np.diff(w) > 0) and w[-1] < n      # distinct positions, ascending
    assert np.array_equal(a['grads_sample'], -w)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
