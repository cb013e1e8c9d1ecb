"""The host side of VideoIndex.ranks / metric.retrieval_metrics_indexed without a GPU: the video-to-text renumbering,
the rank restatement the GPU tests use (pinned to the golden t2v_cols / v2t_cols and metrics), the argument errors that
need no device, and the new exports."""
import ctypes
import json

import numpy as np
import pytest
import torch

from tests.fixtures import load_npz


def brute_counts(scores, target):
  """(#{j : s_j > s_t}, #{j : s_j == s_t}) over one row of scores; the tie-averaged 0-based rank of model/metric.py:90-121
  is greater + (equal - 1) / 2."""
  return int((scores > scores[target]).sum()), int((scores == scores[target]).sum())


def brute_rank(scores, target):
  greater, equal = brute_counts(scores, target)
  return greater + (equal - 1) / 2


def restated_v2t_targets(query_masks):
  """Caption (b, c) -> its position among the unmasked captions in row order b*C + c, -1 where masked: spelled as a loop."""
  qm = np.asarray(query_masks)
  out = np.full(qm.shape, -1, np.int64)
  n = 0
  for b in range(qm.shape[0]):
    for c in range(qm.shape[1]):
      if qm[b, c]:
        out[b, c] = n
        n += 1
  return out


def test_v2t_renumbering_matches_its_restatement():
  from mmt_amd.metric import v2t_targets
  qm = load_npz('trainer_valid')['query_masks']
  assert qm.shape == (24, 3) and int((qm != 0).sum()) == 55
  emptied = qm.copy()
  emptied[4] = 0      # a video with no real caption at all
  emptied[23] = 0     # ... and the last one
  for masks in (qm, emptied, np.ones_like(qm), np.zeros_like(qm)):
    valid, targets = v2t_targets(masks, 24, 3)
    assert valid.dtype == bool and np.array_equal(valid, masks.reshape(-1) != 0)
    assert targets.dtype == np.int64 and np.array_equal(targets, restated_v2t_targets(masks))
    # a torch mask and a flat one mean the same
    assert np.array_equal(v2t_targets(torch.from_numpy(masks), 24, 3)[1], targets)
    assert np.array_equal(v2t_targets(masks.reshape(-1), 24, 3)[1], targets)
  valid, targets = v2t_targets(None, 5, 2)
  assert valid.all() and np.array_equal(targets, np.arange(10).reshape(5, 2))
  assert (v2t_targets(emptied, 24, 3)[1][4] == -1).all()
  with pytest.raises(ValueError):
    v2t_targets(qm, 24, 2)


def test_brute_force_ranks_of_the_golden_sims_reproduce_the_golden_cols_and_metrics():
  """greater + (equal - 1) / 2 handles ties as the reference's t2v_cols / v2t_cols do, and cols2metrics on those ranks gives
  the recorded metrics: the restatement the GPU tests bracket with is the reference's."""
  from mmt_amd.metric import cols2metrics, v2t_targets
  g = load_npz('trainer_valid')
  sims, qm = g['sims'].astype(np.float64), g['query_masks']
  caps = qm.shape[1]
  valid, targets = v2t_targets(qm, *qm.shape)
  t2v = np.array([brute_rank(sims[r], r // caps) for r in np.flatnonzero(valid)])
  gallery = sims[valid]  # the unmasked captions only
  v2t = np.array([min(brute_rank(gallery[:, b], t) for t in targets[b] if t >= 0) for b in range(qm.shape[0])])
  assert np.array_equal(t2v, g['t2v_cols']) and np.array_equal(v2t, g['v2t_cols'])
  tied = np.array([0.5, 0.25, 0.5, 0.5, -0.0, 0.0])
  assert [brute_rank(tied, t) for t in range(6)] == [1.0, 3.0, 1.0, 1.0, 4.5, 4.5]
  want = json.loads(str(g['metrics']))
  for name, cols in (('t2v_metrics', t2v), ('v2t_metrics', v2t)):
    got = cols2metrics(cols, cols.size)
    assert set(got) == set(want[name])
    for key, value in want[name].items():
      assert got[key] == pytest.approx(value, rel=1e-6), (name, key)


def _hollow_index(num_items, dtype=torch.float32):
  """A VideoIndex with its bookkeeping and no storage: the argument checks come before anything reads it."""
  from mmt_amd.search import VideoIndex
  index = VideoIndex.__new__(VideoIndex)
  index.capacity, index.num_experts, index.dim, index.num_items = 8, 2, 8, num_items
  index.device, index.dtype = torch.device('cuda', 0), dtype
  return index


def test_argument_errors_are_raised_without_a_device():
  q, qw = torch.zeros(3, 2, 8), torch.zeros(3, 2)
  for method in ('rank_counts', 'ranks'):
    with pytest.raises(ValueError, match='holds no items'):
      getattr(_hollow_index(0), method)(q, qw, torch.zeros(3, dtype=torch.int64))
    call = getattr(_hollow_index(5), method)
    with pytest.raises(ValueError, match='int64'):
      call(q, qw, torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ValueError, match='int64'):
      call(q, qw, [0, 1, 2])
    with pytest.raises(ValueError, match='index device'):
      call(q, qw, torch.zeros(3, dtype=torch.int64))  # host targets for a device index
  index = _hollow_index(5)
  index.device = torch.device('cpu')  # lets the shape checks be reached with host tensors
  for bad in (torch.zeros((), dtype=torch.int64), torch.zeros(3, 2, 2, dtype=torch.int64), torch.zeros(3, 0, dtype=torch.int64)):
    with pytest.raises(ValueError, match='targets'):
      index.rank_counts(q, qw, bad)
  with pytest.raises(ValueError, match='CUDA tensor'):
    index.rank_counts(q, qw, torch.zeros(3, dtype=torch.int64))  # the queries themselves are host tensors
  from mmt_amd.metric import retrieval_metrics_indexed
  with pytest.raises(ValueError, match='no caption'):
    retrieval_metrics_indexed(torch.zeros(2, 2, 8), torch.zeros(2, 2, 1, 8), torch.zeros(2, 2), torch.zeros(2, 1, 2),
                              query_masks=np.zeros((2, 1)))


def test_rank_exports_gate_their_arguments_on_the_host():
  """mmt_rank_workspace_ints is pure host code (the gates of mmt_search_rank: tests/test_search_abi_cpu.py)."""
  from mmt_amd import _lib
  handle = ctypes.CDLL(_lib.LIB_PATH)
  f = handle.mmt_rank_workspace_ints
  f.restype = ctypes.c_int64
  assert f(64, 4096 * 512, 1) == 64 * (1 + 2 * 512)                 # full-size chunks
  assert f(63, 127, 3) == 63 * 3 * (1 + 2 * 1)                      # one tile
  assert f(257, 4097, 32) == 257 * 32 * (1 + 2 * 33)                # 128-column chunks while the chip is not full
  for bad in ((0, 5, 1), (5, 0, 1), (5, 5, 0), (5, 5, 33)):
    assert f(*bad) == -1


