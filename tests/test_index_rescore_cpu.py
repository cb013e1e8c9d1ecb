"""The host side of VideoIndex.rescore (mmt_search_rescore and its bf16 / fp8 forms) without a GPU: the definition the GPU
tests hold the kernels to, the select pass of search_rescore.hip restated on key integers against it, the header and the
ctypes table, the argument gates of the entry points and the argument errors of the calls."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests.test_index_groups_cpu import _hollow_index, _hollow_sharded, _item, _key, best_first

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = {'mmt_rescore_workspace_keys': 2}  # mmt_search_rescore itself: tests/test_search_abi_cpu.py
INF = float('inf')


def brute_rescore(scores_row, candidates_row, k):
  """The definition, for one query: scores_row[j] is the score of candidates_row[j] (any value where the candidate is
  negative) -> (scores float32 [k], items int64 [k]): the distinct non-negative candidates, best first under `search`'s
  order -- score descending with -0.0 tied to +0.0, equal scores by ascending item -- the best k of them, then (-inf, -1).
  A score keeps its bits but for a -0.0, which `search` returns as +0.0."""
  scores_row, cand = np.asarray(scores_row, np.float32), np.asarray(candidates_row, np.int64)
  items, first = np.unique(cand[cand >= 0], return_index=True)        # ascending items: a stable sort keeps them so on ties
  mine = scores_row[cand >= 0][first]
  order = best_first(mine)[:k]
  scores, out = np.full(k, -INF, np.float32), np.full(k, -1, np.int64)
  scores[:order.size], out[:order.size] = mine[order] + np.float32(0.0), items[order]
  return scores, out


def padded_rescore(scores, candidates, k):
  """brute_rescore row by row -> (scores [NQ, k] float32, items [NQ, k] int64)."""
  rows = [brute_rescore(s, c, k) for s, c in zip(scores, candidates)]
  return np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])


def _score(key):
  """tk_score of search_topk.h: the score bits back from a key's upper half."""
  u = key >> 32
  u = (u & 0x7fffffff) if u & 0x80000000 else (~u & 0xffffffff)
  return np.uint32(u).view(np.float32)


def select_pass(scores_row, candidates_row, k):
  """rescore_select_kernel restated: the keys of the pairs (0 for none), padded with 0 to a power of two, sorted
  descending, a key equal to its predecessor dropped, the first k survivors decoded, (-inf, -1) after them."""
  keys = [_key(s, c) if c >= 0 else 0 for s, c in zip(scores_row, candidates_row)]
  p = 1
  while p < len(keys):
    p <<= 1
  keys = sorted(keys + [0] * (p - len(keys)), reverse=True)
  survivors = [x for i, x in enumerate(keys) if x and (i == 0 or x != keys[i - 1])][:k]
  scores, out = np.full(k, -INF, np.float32), np.full(k, -1, np.int64)
  for j, x in enumerate(survivors):
    scores[j], out[j] = _score(x), _item(x)
  return scores, out


def _same(a, b):
  return np.array_equal(a[1], b[1]) and np.array_equal(a[0].view(np.int32), b[0].view(np.int32))


def _crafted_rows():
  """(name, scores of the pairs, candidates): a repeated item carries the same score every time it is listed."""
  f = np.float32
  yield 'all none', f([0, 0, 0, 0]), [-1, -1, -1, -1]
  yield 'one candidate', f([0.25]), [7]
  yield 'one among none', f([9, 0.25, 9]), [-1, 7, -1]
  yield 'one item repeated', f([0.5] * 6), [3] * 6
  yield 'equal scores', f([1, 1, 1, 2, 1]), [9, 2, 5, 4, 0]
  yield 'signed zeros', f([-0.0, 0.0, -0.0, 0.0, -1e-45, 1e-45]), [5, 3, 1, 8, 0, 2]
  yield 'infinities', f([-INF, INF, 0, -INF]), [1, 2, 3, 0]
  gen = np.random.default_rng(0)
  for c in (1, 3, 129, 1024):
    table = np.round(gen.standard_normal(300), 1).astype(np.float32)          # a score per item, many ties
    table[gen.integers(0, 300, 20)] = -0.0
    cand = gen.integers(-1, 300 if c > 3 else 4, c)
    yield 'C = %d' % c, table[np.maximum(cand, 0)], cand
  cand = np.arange(1024)[::-1].copy()                                           # every candidate distinct: C = 1 024 survivors
  yield 'distinct', gen.standard_normal(1024).astype(np.float32), cand


@pytest.mark.parametrize('name,scores,cand', list(_crafted_rows()), ids=lambda v: v if isinstance(v, str) else None)
def test_select_pass_restated_gives_the_definition(name, scores, cand):
  distinct = len({c for c in cand if c >= 0})
  ks = sorted({1, 2, max(1, distinct - 1), max(1, distinct), min(128, distinct + 1), min(128, len(cand)), 128})
  for k in ks:
    want, got = brute_rescore(scores, cand, k), select_pass(scores, cand, k)
    assert _same(want, got), (name, k)
    have = min(k, distinct)
    assert (want[1][:have] >= 0).all() and (want[1][have:] == -1).all() and np.isneginf(want[0][have:]).all()
    assert len(set(want[1][:have].tolist())) == have                            # each item once


def test_definition_on_rows_worked_by_hand():
  f = np.float32
  s, i = brute_rescore(f([1, 1, 1, 2, 1]), [9, 2, 5, 4, 0], 4)
  assert i.tolist() == [4, 0, 2, 5] and s.tolist() == [2, 1, 1, 1]             # equal scores: ascending item wins
  s, i = brute_rescore(f([-0.0, 0.0, -0.0, 0.0, -1e-45, 1e-45]), [5, 3, 1, 8, 0, 2], 6)
  assert i.tolist() == [2, 1, 3, 5, 8, 0]                                      # -0 ties with +0
  assert not np.signbit(s[1:5]).any() and (s[1:5] == 0).all()                  # and comes back as +0
  s, i = brute_rescore(f([0.5] * 6), [3] * 6, 3)
  assert i.tolist() == [3, -1, -1] and s[0] == 0.5 and np.isneginf(s[1:]).all()
  s, i = brute_rescore(f([0, 0]), [-1, -1], 2)
  assert i.tolist() == [-1, -1] and np.isneginf(s).all()
  # the order of a query's candidates does not matter
  gen = np.random.default_rng(1)
  table = np.round(gen.standard_normal(50), 1).astype(np.float32)
  cand = gen.integers(-1, 50, 200)
  perm = gen.permutation(200)
  assert _same(brute_rescore(table[np.maximum(cand, 0)], cand, 20), brute_rescore(table[np.maximum(cand, 0)][perm], cand[perm], 20))


def test_signatures_of_the_new_exports_agree_with_the_header():
  from mmt_amd import _lib
  src = open(os.path.join(ROOT, 'include', 'mmt_hip.h')).read()
  handle = ctypes.CDLL(_lib.LIB_PATH)
  for name, arity in NEW_EXPORTS.items():
    m = re.search(r'\b(int|int64_t) %s\(([^;]*?)\);' % name, src)
    assert m, name + ' is not declared in mmt_hip.h'
    params = [p.strip() for p in m.group(2).replace('\n', ' ').split(',')]
    res, args = _lib.SIGNATURES[name]
    assert res is (ctypes.c_int if m.group(1) == 'int' else ctypes.c_int64), name
    assert len(args) == len(params) == arity, name
    for p, a in zip(params, args):
      assert (a is ctypes.c_void_p) == ('*' in p) and (a is ctypes.c_int) == (p.startswith('int ')), (name, p)
    assert hasattr(handle, name)
  assert 'search_rescore.hip' in src
  assert handle.mmt_abi_version() == 6


def test_new_exports_gate_their_arguments_on_the_host():
  """Every refusal below returns before any launch: MMT_ERR_ARG = -1, MMT_ERR_ALIGN = -2."""
  from mmt_amd import _lib
  handle = ctypes.CDLL(_lib.LIB_PATH)
  fns = {}
  for name in NEW_EXPORTS:
    fns[name] = getattr(handle, name)
    fns[name].restype, fns[name].argtypes = _lib.SIGNATURES[name]
  size = fns['mmt_rescore_workspace_keys']
  assert size(1, 1) == 1 and size(130, 1000) == 130000 and size(4096, 1024) == 4096 * 1024
  for bad in ((0, 1), (-1, 1), (1, 0), (1, 1025), (1, -1)):
    assert size(*bad) == -1, bad


@pytest.mark.parametrize('hollow', [_hollow_index, _hollow_sharded], ids=['VideoIndex', 'ShardedVideoIndex'])
def test_argument_errors_are_raised_without_a_device(hollow):
  from mmt_amd import search
  from mmt_amd.search import ShardedVideoIndex, VideoIndex
  assert search.MAX_C == 1024
  q, qw = torch.zeros(3, 2, 8), torch.zeros(3, 2)
  cand = torch.zeros(3, 4, dtype=torch.int64)
  index = hollow(5)
  for bad in ([[0, 1]], np.zeros((3, 4), np.int64), None, cand.to(torch.int32), cand.double(), cand > 0):
    with pytest.raises(ValueError, match='candidates must be an int64 tensor'):
      index.rescore(q, qw, bad)
  with pytest.raises(ValueError, match='index device'):
    index.rescore(q, qw, cand)                                     # host candidates for a device index
  index.device = torch.device('cpu')                               # lets the later checks be reached with host tensors
  for bad in (cand[:, 0], cand.reshape(3, 2, 2), torch.zeros(3, 0, dtype=torch.int64), torch.zeros(3, 1025, dtype=torch.int64),
              torch.tensor(3)):
    with pytest.raises(ValueError, match=r'candidates \[NQ, 1 <= C <= 1024\] expected'):
      index.rescore(q, qw, bad)
  for bad in (0, 129, -1, 2.0, True, 'all'):
    with pytest.raises(ValueError, match=r'k must be None or an int in 1\.\.128'):
      index.rescore(q, qw, cand, k=bad)
  with pytest.raises(ValueError, match='holds no items'):
    empty = hollow(0)
    empty.device = torch.device('cpu')
    empty.rescore(q, qw, cand)
  with pytest.raises(ValueError, match='CUDA tensor'):
    index.rescore(q, qw, cand)                                     # the queries themselves are host tensors
  # search_refined: k, shortlist and the coarse index before anything is scored
  coarse = hollow(5)
  for bad in (0, 129, True, None):
    with pytest.raises(ValueError, match=r'search_refined: k must be an int in 1\.\.128'):
      index.search_refined(q, qw, coarse, k=bad)
    with pytest.raises(ValueError, match=r'shortlist must be an int in 1\.\.128'):
      index.search_refined(q, qw, coarse, shortlist=bad)
  for bad in (None, 'fp8', cand):
    with pytest.raises(ValueError, match='coarse must be a VideoIndex or ShardedVideoIndex'):
      index.search_refined(q, qw, bad)
  for field in ('num_items', 'num_experts', 'dim'):
    other = hollow(5)
    setattr(other, field, getattr(other, field) + 1)
    with pytest.raises(ValueError, match=r'the coarse index holds \(num_items, num_experts, dim\)'):
      index.search_refined(q, qw, other)
  with pytest.raises(ValueError, match='the coarse index is on cuda:0, this one on cpu'):
    index.search_refined(q, qw, coarse)
  # neither normalisation nor pooling are part of the call; both classes have one surface
  for extra in ('norm', 'pooling', 'item_pooling', 'subset'):
    with pytest.raises(TypeError):
      index.rescore(q, qw, cand, **{extra: None})
  for method in ('rescore', 'search_refined'):
    assert getattr(ShardedVideoIndex, method) is getattr(VideoIndex, method)
  assert list(inspect.signature(VideoIndex.rescore).parameters) == ['self', 'embds', 'weights', 'candidates', 'k']
  assert list(inspect.signature(VideoIndex.search_refined).parameters) == [
      'self', 'embds', 'weights', 'coarse', 'k', 'shortlist', 'subset', 'exclude']
  refined = inspect.signature(VideoIndex.search_refined).parameters
  assert refined['k'].default == 10 and refined['shortlist'].default == search.MAX_K == 128
