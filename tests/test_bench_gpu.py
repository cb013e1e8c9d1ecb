"""bench.py's plain run: --steps timed steps, the headline fields of the result line, nothing of --full, and
--dump-outputs writing the last timed step's outputs from identical inputs on every run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(out_dir, steps=3, warmup=2):
  env = dict(os.environ)
  for k in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_PORT', 'MMT_BENCH_BACKEND'):
    env.pop(k, None)
  r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', str(steps), '--warmup',
                      str(warmup), '--dump-outputs', str(out_dir)],
                     env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
  assert r.returncode == 0, r.stderr[-2000:]
  return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_bench_plain_run_and_dumped_outputs(tmp_path):
  a = _bench(tmp_path / 'a')
  for k in ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step'):
    assert k in a, k
  assert a['steps'] == 3 and a['warmup'] == 2 and a['ms_per_step'] > 0
  assert abs(a['value'] - 32 * 1e3 / a['ms_per_step']) < 1e-6 * a['value']  # pairs/s of the same timed steps
  assert a['dense'] is None and 'cpu_baseline' not in a and 'roofline' not in a and a['config']['full'] is False
  files = sorted(os.listdir(tmp_path / 'a'))
  assert files == ['loss.npy', 'weights.npy']
  assert sum(os.path.getsize(tmp_path / 'a' / f) for f in files) <= 64 * 1024 * 1024
  loss = np.load(tmp_path / 'a' / 'loss.npy')
  w = np.load(tmp_path / 'a' / 'weights.npy')
  assert loss.dtype == np.float64 and loss.shape == (1,) and loss[0] == a['final_loss']
  assert w.dtype == np.float32 and w.ndim == 1 and w.size > 0 and np.isfinite(w).all()
  # the same arguments: the same inputs, so the same outputs up to the order of floating-point reductions (Adam at lr 5e-5
  # moves a weight by at most ~lr per step, 5 steps here)
  b = _bench(tmp_path / 'b')
  lb, wb = np.load(tmp_path / 'b' / 'loss.npy'), np.load(tmp_path / 'b' / 'weights.npy')
  assert abs(lb[0] - loss[0]) <= 1e-3 * abs(loss[0]), (lb[0], loss[0])
  assert wb.shape == w.shape and np.abs(wb - w).max() <= 5 * 5e-5 * 2, np.abs(wb - w).max()
