"""The host side of querybank hubness normalisation (search.VideoIndex.hub_norm and norm=; mmt_search_col_lse,
mmt_search_topk_norm, mmt_search_thresholds_norm, mmt_search_count_norm, their bf16 forms and
mmt_col_lse_workspace_floats) without a GPU: the header and the ctypes table agree, the argument gates, the errors that
need no device, and the numpy restatements the GPU tests hold the kernels to -- the fp32 blockwise log-sum-exp, the
multiply-then-subtract correction, a stable top-k and brute-force counts -- pinned on hand-made cases."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests.test_index_ranks_cpu import _hollow_index
from tests.test_index_subset_cpu import brute_topk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ('mmt_col_lse_workspace_floats',)  # the scans with a norm: tests/test_search_abi_cpu.py
F32 = np.float32


def blockwise_lse32(scores, beta):
  """The recipe of mmt_search_col_lse restated in numpy float32: scores fp32 [NB, NV] (bank x items), beta ->
  lse fp32 [NV].  x = fl(beta * score); per 64-row block m = max x, p = sum exp(x - m) over its rows in ascending order;
  the blocks folded in ascending order, M' = max(M, m), S' = S exp(M - M') + p exp(m - M'); lse = M + log S.  (numpy's
  exp and log are not the device's, so this pins the recipe, not the device's last bit.)"""
  x = (F32(beta) * np.asarray(scores, F32)).astype(F32)
  big_m = big_s = None
  for i in range(0, x.shape[0], 64):
    blk = x[i:i + 64]
    m = blk.max(0)
    p = np.zeros(x.shape[1], F32)
    for row in blk:
      p = (p + np.exp((row - m).astype(F32)).astype(F32)).astype(F32)
    if big_m is None:
      big_m, big_s = m, p
    else:
      new = np.maximum(big_m, m)
      big_s = ((big_s * np.exp((big_m - new).astype(F32)).astype(F32)).astype(F32) +
               (p * np.exp((m - new).astype(F32)).astype(F32)).astype(F32)).astype(F32)
      big_m = new
  return (big_m + np.log(big_s).astype(F32)).astype(F32)


def corrected32(scores, lse, beta):
  """score' = fl(fl(beta * score) - lse[item]) in float32: scores fp32 [NQ, NV], lse fp32 [NV] -> fp32 [NQ, NV].  Two
  roundings, not an fma."""
  prod = (F32(beta) * np.asarray(scores, F32)).astype(F32)
  return (prod - np.asarray(lse, F32)[None, :]).astype(F32)


def stable_topk(scores, allowed, exclude, k):
  """search(k, subset, exclude) on a given fp32 score matrix: (scores fp32 [nq, k'], indices int64 [nq, k']), descending,
  equal scores (-0 == +0) by ascending item, then (-inf, -1); a returned score keeps its bits."""
  scores = np.asarray(scores, F32)
  s, idx = brute_topk(scores.astype(np.float64), allowed, exclude, k)
  out = np.full(idx.shape, -np.inf, F32)
  rows, cols = np.nonzero(idx >= 0)
  out[rows, cols] = scores[rows, idx[rows, cols]]
  return out, idx


def brute_counts(scores, targets, allowed=None):
  """rank_counts on a given fp32 score matrix: scores [nq, nv], targets int64 [nq, T] (-1 = none), allowed None or bool
  [nv] -> (greater, equal) int32 [nq, T]: the allowed items scoring above / equal to the target's score, plain float
  compares; 0 / 0 for -1."""
  scores = np.asarray(scores, F32)
  nq, t = targets.shape
  greater, equal = np.zeros((nq, t), np.int32), np.zeros((nq, t), np.int32)
  for r in range(nq):
    row = scores[r] if allowed is None else scores[r][allowed]
    for j in range(t):
      if targets[r, j] >= 0:
        thr = scores[r, targets[r, j]]
        greater[r, j], equal[r, j] = (row > thr).sum(), (row == thr).sum()
  return greater, equal


def lse64(scores, beta):
  x = np.float64(F32(beta)) * np.asarray(scores, np.float64)
  m = x.max(0)
  return m + np.log(np.exp(x - m).sum(0))


def lse_bound(scores, beta):
  """2^-23 * (NB + |ref| + max_b |beta * score| + 16) per item: the bound of the GPU test, derived there."""
  x = np.float64(F32(beta)) * np.asarray(scores, np.float64)
  return 2.0 ** -23 * (x.shape[0] + np.abs(lse64(scores, beta)) + np.abs(x).max(0) + 16)


def _bits(x):
  return np.ascontiguousarray(x, F32).view(np.int32)


def test_blockwise_lse_on_hand_made_cases():
  one = F32([[0.3, -2.0, 0.0]])
  for beta in (1.0, 20.0, 100.0):                       # one bank row: lse = fl(beta * score), exactly
    assert np.array_equal(_bits(blockwise_lse32(one, beta)), _bits(F32(beta) * one[0]))
  twice = np.repeat(one, 2, 0)                          # two equal rows: x + log 2
  assert np.array_equal(blockwise_lse32(twice, 1.0), (one[0] + np.log(F32(2))).astype(F32))
  far = F32([[0.0, 1.0], [-200.0, 1.0 - 200.0]])        # a dominated row adds nothing in fp32
  assert np.array_equal(_bits(blockwise_lse32(far, 1.0)), _bits(F32([0.0, 1.0])))
  zeros = np.zeros((65, 2), F32)                        # 64 + 1 rows: two blocks, log 65
  got = blockwise_lse32(zeros, 7.0)
  assert np.abs(got - np.log(65.0)).max() <= 2.0 ** -22
  # the order of the blocks is part of the recipe: a big late block rescales the early sum
  late = np.concatenate([np.zeros((64, 1), F32), np.full((3, 1), 5.0, F32)])
  assert abs(float(blockwise_lse32(late, 2.0)[0]) - float(lse64(late, 2.0)[0])) <= float(lse_bound(late, 2.0)[0])
  rng = np.random.default_rng(0)
  for nb in (1, 63, 65, 300, 1000):
    for beta in (1.0, 20.0, 100.0):
      s = rng.standard_normal((nb, 50)).astype(F32)
      err = np.abs(blockwise_lse32(s, beta).astype(np.float64) - lse64(s, beta))
      assert (err <= lse_bound(s, beta)).all(), (nb, beta, (err / lse_bound(s, beta)).max())


def test_correction_is_a_multiply_then_a_subtract():
  # beta * s = 3 * (1 + 2^-23) needs 25 bits: rounded to 3 + 2^-21 (ties to even) before the subtract; an fma would keep
  # the exact product and give 3 * 2^-23 against the rounded 2^-21
  s = F32([[1.0 + 2.0 ** -23]])
  got = corrected32(s, F32([3.0]), 3.0)
  assert got.dtype == F32 and got.shape == (1, 1)
  assert float(got[0, 0]) == 2.0 ** -21 and float(got[0, 0]) != 3 * 2.0 ** -23
  m = corrected32(F32([[0.5, 1.0], [2.0, -1.0]]), F32([1.0, -1.0]), 2.0)
  assert m.tolist() == [[0.0, 3.0], [3.0, -1.0]]


def test_stable_topk_and_brute_counts_on_hand_made_cases():
  scores = F32([[0.5, 0.25, 0.5, 0.5, -0.0, 0.0]])
  every = np.ones(6, bool)
  s, i = stable_topk(scores, every, None, 10)
  assert i.tolist() == [[0, 2, 3, 1, 4, 5]]
  assert _bits(s)[0, 4:].tolist() == _bits(F32([-0.0, 0.0])).tolist()     # a tie in item order, each with its own sign bit
  s, i = stable_topk(scores, np.array([True, True, False, True, True, True]), np.array([[0, 3, 1, 4]]), 5)
  assert i.tolist() == [[5, -1, -1, -1, -1]] and np.isneginf(s[0, 1:]).all() and s.dtype == F32
  tg = np.array([[0, 1, 4, -1]])
  greater, equal = brute_counts(scores, tg)
  assert greater.tolist() == [[0, 3, 4, 0]] and equal.tolist() == [[3, 1, 2, 0]]
  greater, equal = brute_counts(scores, tg, np.array([False, True, True, False, False, True]))
  assert greater.tolist() == [[0, 1, 2, 0]] and equal.tolist() == [[1, 1, 1, 0]]   # target 0 is outside: it counts item 2


def test_signatures_of_the_new_exports_agree_with_the_header():
  from mmt_amd import _lib
  src = open(os.path.join(ROOT, 'include', 'mmt_hip.h')).read()
  handle = ctypes.CDLL(_lib.LIB_PATH)
  for name in NEW_EXPORTS:
    m = re.search(r'\b(int|int64_t) %s\(([^;]*?)\);' % name, src)
    assert m, name + ' is not declared in mmt_hip.h'
    params = [p.strip() for p in m.group(2).replace('\n', ' ').split(',')]
    res, args = _lib.SIGNATURES[name]
    assert res is (ctypes.c_int if m.group(1) == 'int' else ctypes.c_int64) and len(args) == len(params), name
    for p, a in zip(params, args):
      assert (a is ctypes.c_void_p) == ('*' in p) and (a is ctypes.c_int) == (p.startswith('int ')), (name, p)
      assert (a is ctypes.c_float) == (p.startswith('float ') and '*' not in p), (name, p)
    assert hasattr(handle, name)
  assert handle.mmt_abi_version() == 6


def test_new_exports_gate_their_arguments_on_the_host():
  """Every refusal below returns before any launch: MMT_ERR_ARG = -1, MMT_ERR_ALIGN = -2."""
  from mmt_amd import _lib
  handle = ctypes.CDLL(_lib.LIB_PATH)
  fns = {}
  for name in NEW_EXPORTS:
    fns[name] = getattr(handle, name)
    fns[name].restype, fns[name].argtypes = _lib.SIGNATURES[name]
  size = fns['mmt_col_lse_workspace_floats']
  assert size(1, 1) == 2 and size(64, 10) == 20 and size(65, 10) == 40 and size(4096, 262144) == 2 * 64 * 262144
  assert size(0, 5) == -1 and size(5, 0) == -1


def _hollow_norm(num_items, device, hubs=None):
  from mmt_amd.search import HubNorm
  norm = HubNorm.__new__(HubNorm)
  norm.num_items, norm.device, norm.beta, norm.bank_size, norm.hubs, norm.lse = num_items, torch.device(device), 1.0, 1, hubs, None
  return norm


def test_argument_errors_are_raised_without_a_device():
  q, qw = torch.zeros(3, 2, 8), torch.zeros(3, 2)
  tg = torch.zeros(3, dtype=torch.int64)
  thr = torch.zeros(3)
  index = _hollow_index(5)
  for bad in (20, True, None, '1', 0.0, -1.0, float('inf'), float('nan'), np.float32(2.0)):
    with pytest.raises(ValueError, match='beta'):
      index.hub_norm(q, qw, bad)
  with pytest.raises(ValueError, match='dynamic'):
    index.hub_norm(q, qw, 1.0, dynamic=1)
  with pytest.raises(ValueError, match='holds no items'):
    _hollow_index(0).hub_norm(q, qw, 1.0)
  with pytest.raises(ValueError, match='CUDA tensor'):      # the checks above come before the bank is touched
    index.hub_norm(q, qw, 1.0)
  calls = (lambda **kw: index.search(q, qw, **kw), lambda **kw: index.rank_counts(q, qw, tg, **kw),
           lambda **kw: index.ranks(q, qw, tg, **kw), lambda **kw: index.target_scores(q, qw, tg, **kw),
           lambda **kw: index.threshold_counts(q, qw, thr, **kw))
  index.device = torch.device('cpu')  # lets the checks of targets and thresholds pass with host tensors
  for call in calls:
    with pytest.raises(ValueError, match='VideoIndex.hub_norm'):
      call(norm=torch.zeros(5))
    with pytest.raises(ValueError, match='built for 4 items'):   # a norm is tied to the index size and device
      call(norm=_hollow_norm(4, 'cpu'))
    with pytest.raises(ValueError, match='the norm is on'):
      call(norm=_hollow_norm(5, 'cuda:0'))
    with pytest.raises(ValueError, match='dynamic'):
      call(norm=_hollow_norm(5, 'cpu'), dynamic=1)
    with pytest.raises(ValueError, match='dynamic=True needs'):  # the rule needs the hubs
      call(norm=_hollow_norm(5, 'cpu'), dynamic=True)
    with pytest.raises(ValueError, match='dynamic=True needs'):
      call(dynamic=True)
    with pytest.raises(ValueError, match='CUDA tensor'):         # a fitting norm: on to the queries
      call(norm=_hollow_norm(5, 'cpu'))
  from mmt_amd.search import ShardedVideoIndex
  with pytest.raises(ValueError, match='beta'):
    ShardedVideoIndex.hub_norm(index, q, qw, 2)
  with pytest.raises(ValueError, match='ShardedVideoIndex.hub_norm'):
    ShardedVideoIndex._norm(index, _hollow_norm(5, 'cpu'), 'search')


def test_indexed_metrics_reject_a_bank_without_beta():
  from mmt_amd.metric import retrieval_metrics_indexed
  args = (torch.zeros(4, 2, 8), torch.zeros(4, 2, 1, 8), torch.zeros(4, 2), torch.zeros(4, 1, 2))
  bank = (torch.zeros(3, 2, 8), torch.zeros(3, 2))
  for kwargs in ({'text_bank': bank}, {'video_bank': bank}, {'text_bank': bank, 'video_bank': bank}):
    with pytest.raises(ValueError, match='needs beta'):
      retrieval_metrics_indexed(*args, **kwargs)
  with pytest.raises(ValueError, match='pair'):
    retrieval_metrics_indexed(*args, text_bank=bank[0], beta=20.0)
