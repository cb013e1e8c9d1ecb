"""The host side of the diversified search (VideoIndex.pair_scores, diversify, search_diverse; mmt_search_pair_scores and
mmt_search_mmr) without a GPU: the selection rule of mmr_kernel (search_diverse.hip) restated in numpy fp32 -- the
definition the GPU tests hold the kernel to, bit for bit -- and checked on a case worked by hand, the header and the ctypes
table, the argument gates of the two entry points and the argument errors of the three calls."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests.test_index_groups_cpu import _hollow_index, _hollow_sharded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = {'mmt_search_pair_scores': 12, 'mmt_search_mmr': 12}
INF = float('inf')


def _order(v):
  """tk_key of search_topk.h over (value, position) for values float32 [n] at positions 0 .. n - 1 -> uint64 [n], larger is
  better: the value descending with -0 as +0, equal values by ascending position."""
  u = np.ascontiguousarray(v, np.float32).view(np.uint32).copy()
  u[(u & 0x7fffffff) == 0] = 0
  u = np.where(u & 0x80000000, ~u, u | np.uint32(0x80000000))
  return (u.astype(np.uint64) << np.uint64(32)) | (~np.arange(u.shape[0], dtype=np.uint32)).astype(np.uint64)


def brute_mmr(rel, items, sims, k, a, b):
  """The selection rule for one row, in fp32: rel float32 [C] and items int64 [C], the row's distinct candidates in
  `search`'s order padded with (-inf, -1); sims float32 [C, C] their Gram; a, b the two weights -> (scores float32 [k],
  indices int64 [k], values float32 [k]).  With n the number of items >= 0: slot 0 is position 0 with value fl(a * rel[0]);
  for slot t >= 1 every unselected position p has pen_p, the largest sims[p, s] over the selected s (the first as it is,
  then replaced where larger: a plain compare), v_p = fl(fl(a * rel[p]) - fl(b * pen_p)), and the position with the
  largest v_p is selected, -0 tied with +0, equal values to the lowest p.  Slots from min(k, n) on hold (-inf, -1, -inf)."""
  rel, items, sims = np.asarray(rel, np.float32), np.asarray(items, np.int64), np.asarray(sims, np.float32)
  a, b = np.float32(a), np.float32(b)
  scores, index, values = np.full(k, -INF, np.float32), np.full(k, -1, np.int64), np.full(k, -INF, np.float32)
  n = int((items >= 0).sum())
  if n == 0:
    return scores, index, values
  with np.errstate(all='ignore'):
    ar = (a * rel[:n]).astype(np.float32)
    scores[0], index[0], values[0] = rel[0], items[0], ar[0]
    unselected, last, pen = np.arange(n) > 0, 0, None
    for t in range(1, min(k, n)):
      x = sims[last, :n]
      pen = x.copy() if pen is None else np.where(x > pen, x, pen)
      v = (ar - (b * pen).astype(np.float32)).astype(np.float32)
      last = int(np.argmax(np.where(unselected, _order(v), np.uint64(0))))   # the key of a position is never 0
      unselected[last] = False
      scores[t], index[t], values[t] = rel[last], items[last], v[last]
  return scores, index, values


def padded_mmr(rel, items, sims, k, a, b):
  """brute_mmr row by row -> (scores [R, k], indices [R, k], values [R, k])."""
  rows = [brute_mmr(r, i, s, k, a, b) for r, i, s in zip(rel, items, sims)]
  return tuple(np.stack([row[j] for row in rows]) for j in range(3))


def weights_of(lam):
  """(a, b) of a call with this lam: float32(lam), float32(1.0 - lam) with the subtraction in double."""
  return np.float32(lam), np.float32(1.0 - lam)


def test_the_rule_on_a_case_worked_by_hand():
  # A and A' are copies (sim 1), B is unlike both (sim 0)
  rel, items = np.float32([0.9, 0.9, 0.6]), np.int64([10, 11, 20])
  sims = np.float32([[1, 1, 0], [1, 1, 0], [0, 0, 1]])
  s, i, v = brute_mmr(rel, items, sims, 3, *weights_of(0.5))
  assert i.tolist() == [10, 20, 11]                       # B's 0.3 - 0 beats A' at 0.45 - 0.5
  assert s.tolist() == [np.float32(0.9), np.float32(0.6), np.float32(0.9)]
  half = np.float32(0.5)
  assert v.tolist() == [half * rel[0], half * rel[2] - np.float32(0.0), half * rel[1] - half]
  s, i, v = brute_mmr(rel, items, sims, 3, *weights_of(1.0))
  assert i.tolist() == [10, 11, 20] and np.array_equal(s, rel) and np.array_equal(v, rel)   # lam = 1: relevance alone
  s, i, v = brute_mmr(rel, items, sims, 2, *weights_of(0.5))
  assert i.tolist() == [10, 20] and s.shape == (2,)
  # lam = 0: after the most relevant item, the least similar; equal values go to the lower position
  s, i, v = brute_mmr(np.float32([3, 2, 1, 0.5]), np.int64([5, 6, 7, 8]), np.float32(
      [[1, .5, .25, .25], [.5, 1, .9, .1], [.25, .9, 1, .2], [.25, .1, .2, 1]]), 4, *weights_of(0.0))
  assert i.tolist() == [5, 7, 8, 6] and v.tolist() == [0.0, -0.25, -0.25, np.float32(-0.9)]
  # a padded row, a row without candidates, and -0 tied with +0 (position 1 before position 2)
  s, i, v = brute_mmr(np.float32([1, 1, -INF, -INF]), np.int64([4, 9, -1, -1]), np.zeros((4, 4), np.float32), 4, *weights_of(0.5))
  assert i.tolist() == [4, 9, -1, -1] and np.isneginf(s[2:]).all() and np.isneginf(v[2:]).all() and s[1] == 1
  s, i, v = brute_mmr(np.float32([-INF] * 3), np.int64([-1] * 3), np.full((3, 3), np.nan, np.float32), 2, *weights_of(0.5))
  assert i.tolist() == [-1, -1] and np.isneginf(s).all() and np.isneginf(v).all()
  s, i, v = brute_mmr(np.float32([1, -0.0, 0.0]), np.int64([1, 2, 3]), np.float32([[1, 0, 0], [0, 1, 0], [0, 0, 1]]), 3,
                      np.float32(1), np.float32(1))
  assert i.tolist() == [1, 2, 3] and np.signbit(v[1]) and not np.signbit(v[2]) and v[1] == v[2] == 0
  keys = _order(np.float32([0.25, -0.0, 0.0, 0.5, 0.5, -1, -INF, INF])).tolist()
  assert keys[7] > keys[3] > keys[4] > keys[0] > keys[1] > keys[2] > keys[5] > keys[6] > 0
  assert keys[1] >> 32 == keys[2] >> 32 and keys[3] >> 32 == keys[4] >> 32
  assert weights_of(0.3) == (np.float32(0.3), np.float32(0.7)) and weights_of(1.0) == (1.0, 0.0)


def _functions():
  from mmt_amd import _lib
  handle = ctypes.CDLL(_lib.LIB_PATH)
  fns = {}
  for name in NEW_EXPORTS:
    fns[name] = getattr(handle, name)
    fns[name].restype, fns[name].argtypes = _lib.SIGNATURES[name]
  return handle, fns


def test_signatures_of_the_new_exports_agree_with_the_header():
  from mmt_amd import _lib, search
  src = open(os.path.join(ROOT, 'include', 'mmt_hip.h')).read()
  handle, _ = _functions()
  for name, arity in NEW_EXPORTS.items():
    m = re.search(r'\bint %s\(([^;]*?)\);' % name, src)
    assert m, name + ' is not declared in mmt_hip.h'
    params = [p.strip() for p in m.group(1).replace('\n', ' ').split(',')]
    res, args = _lib.SIGNATURES[name]
    assert res is ctypes.c_int and len(args) == len(params) == arity, name
    for p, a in zip(params, args):
      assert (a is ctypes.c_void_p) == ('*' in p), (name, p)
      assert (a is ctypes.c_int) == p.startswith('int '), (name, p)
      assert (a is ctypes.c_float) == p.startswith('float '), (name, p)
    assert hasattr(handle, name)
  assert 'search_diverse.hip' in src
  assert int(re.search(r'#define MMT_SEARCH_MAX_DC (\d+)', src).group(1)) == search.MAX_DC == 128
  assert handle.mmt_abi_version() == 6


def test_new_exports_gate_their_arguments_on_the_host():
  """Every refusal below returns before any launch: MMT_ERR_ARG = -1, MMT_ERR_ALIGN = -2.  A knock-out of
  mmt_search_pair_scores is made with g off its boundary as well, so a gate that has gone missing shows as -2."""
  _, fns = _functions()
  buf = (ctypes.c_char * 256)()
  P = ctypes.addressof(buf) + -ctypes.addressof(buf) % 16       # 16-byte aligned, never dereferenced
  pair, mmr = fns['mmt_search_pair_scores'], fns['mmt_search_mmr']
  names = ['g', 'gw', 'gscale', 'storage', 'NV', 'M', 'd', 'items', 'R', 'C', 'sims', 'stream']
  for storage, mult in ((0, 4), (1, 8), (2, 16)):
    good = dict(g=P, gw=P, gscale=P if storage == 2 else None, storage=storage, NV=5, M=2, d=32, items=P, R=3, C=7, sims=P,
                stream=None)

    def call(**changes):
      return pair(*[dict(good, **changes)[n] for n in names])
    for off in (4, 8):
      assert call(g=P + off) == -2, storage                      # everything else in order: only the alignment is refused
    for C in (1, 128):
      assert call(g=P + 8, C=C) == -2, (storage, C)
    bad = [dict(gw=None), dict(items=None), dict(sims=None), dict(gscale=None if storage == 2 else P), dict(storage=3),
           dict(storage=-1), dict(C=0), dict(C=-1), dict(C=129), dict(R=0), dict(R=-1), dict(NV=0), dict(NV=-1), dict(M=0),
           dict(M=17), dict(d=0), dict(d=-16), dict(d=32 + mult // 2)]
    for changes in bad:
      assert call(**dict(dict(g=P + 8), **changes)) == -1, (storage, changes)
    assert call(g=None) == -1, storage
  assert pair(P + 8, P, None, 1, 5, 2, 4, P, 3, 7, P, None) == -1  # an fp32 width on a bf16 index
  assert pair(P + 8, P, P, 2, 5, 2, 8, P, 3, 7, P, None) == -1     # a bf16 width on an fp8 index
  names = ['items', 'rel', 'sims', 'R', 'C', 'k', 'a', 'b', 'scores', 'index', 'values', 'stream']
  good = dict(items=P, rel=P, sims=P, R=3, C=7, k=7, a=0.5, b=0.5, scores=P, index=P, values=P, stream=None)
  for changes in [dict(items=None), dict(rel=None), dict(sims=None), dict(scores=None), dict(index=None), dict(values=None),
                  dict(R=0), dict(R=-1), dict(C=0), dict(C=129, k=1), dict(k=0), dict(k=-1), dict(k=8), dict(C=128, k=129)]:
    assert mmr(*[dict(good, **changes)[n] for n in names]) == -1, changes


@pytest.mark.parametrize('hollow', [_hollow_index, _hollow_sharded], ids=['VideoIndex', 'ShardedVideoIndex'])
def test_argument_errors_are_raised_without_a_device(hollow):
  from mmt_amd import search
  from mmt_amd.search import ShardedVideoIndex, VideoIndex
  assert search.MAX_DC == 128
  q, qw = torch.zeros(3, 2, 8), torch.zeros(3, 2)
  cand = torch.zeros(3, 4, dtype=torch.int64)
  index = hollow(5)
  calls = {'pair_scores': lambda c, **kw: index.pair_scores(c, **kw), 'diversify': lambda c, **kw: index.diversify(q, qw, c, **kw)}
  for name, call in calls.items():
    for bad in ([[0, 1]], np.zeros((3, 4), np.int64), None, cand.to(torch.int32), cand.double(), cand > 0):
      with pytest.raises(ValueError, match=name + ': candidates must be an int64 tensor'):
        call(bad)
    with pytest.raises(ValueError, match='index device'):
      call(cand)                                                   # host candidates for a device index
  index.device = torch.device('cpu')                               # lets the later checks be reached with host tensors
  for name, call in calls.items():
    for bad in (cand[:, 0], cand.reshape(3, 2, 2), torch.zeros(3, 0, dtype=torch.int64), torch.zeros(3, 129, dtype=torch.int64),
                torch.tensor(3)):
      with pytest.raises(ValueError, match=name + r': candidates \[R, 1 <= C <= 128\] expected'):
        call(bad)
    with pytest.raises(ValueError, match=name + ': the index holds no items'):
      empty = hollow(0)
      empty.device = torch.device('cpu')
      empty.pair_scores(cand) if name == 'pair_scores' else empty.diversify(q, qw, cand)
  for bad in (cand[:2], torch.cat([cand, cand[:1]])):
    with pytest.raises(ValueError, match='diversify: 3 queries but candidates'):
      index.diversify(q, qw, bad)
  with pytest.raises(ValueError, match='diversify: 6 queries but candidates'):
    index.diversify(torch.zeros(2, 2, 3, 8), torch.zeros(2, 3, 2), cand)     # the text layout: rows b * C + c
  for method, args in (('diversify', (q, qw, cand)), ('search_diverse', (q, qw))):
    fn = getattr(index, method)
    for bad in (0, 129, -1, 2.0, True, None, 'all'):
      with pytest.raises(ValueError, match=method + r': k must be an int in 1\.\.128'):
        fn(*args, k=bad)
    for bad in (-0.1, 1.5, float('nan'), INF, -INF, True, None, 'half', np.float32(2)):
      with pytest.raises(ValueError, match=method + ': lam must be a number with 0 <= lam <= 1'):
        fn(*args, lam=bad)
    for option in ('norm', 'pooling', 'item_pooling', 'grouping', 'after', 'dynamic'):
      with pytest.raises(ValueError, match='%s: %s= is out of scope' % (method, option)):
        fn(*args, **{option: None})
    with pytest.raises(TypeError, match='unexpected keyword'):
      fn(*args, shortlists=3)
  with pytest.raises(ValueError, match='CUDA tensor'):
    index.diversify(q, qw, cand)                                   # the queries themselves are host tensors
  # search_diverse: shortlist and the coarse index before anything is scored
  coarse = hollow(5)
  for bad in (0, 129, True, None):
    with pytest.raises(ValueError, match=r'search_diverse: shortlist must be an int in 1\.\.128'):
      index.search_diverse(q, qw, shortlist=bad)
  for bad in ('fp8', cand):
    with pytest.raises(ValueError, match='search_diverse: coarse must be a VideoIndex or ShardedVideoIndex'):
      index.search_diverse(q, qw, coarse=bad)
  for field in ('num_items', 'num_experts', 'dim'):
    other = hollow(5)
    setattr(other, field, getattr(other, field) + 1)
    with pytest.raises(ValueError, match=r'the coarse index holds \(num_items, num_experts, dim\)'):
      index.search_diverse(q, qw, coarse=other)
  with pytest.raises(ValueError, match='the coarse index is on cuda:0, this one on cpu'):
    index.search_diverse(q, qw, coarse=coarse)
  with pytest.raises(ValueError, match='search_diverse: the index holds no items'):
    hollow(0).search_diverse(q, qw)
  for method in ('pair_scores', 'diversify', 'search_diverse'):
    assert getattr(ShardedVideoIndex, method) is getattr(VideoIndex, method)
  assert list(inspect.signature(VideoIndex.pair_scores).parameters) == ['self', 'candidates']
  assert list(inspect.signature(VideoIndex.diversify).parameters) == ['self', 'embds', 'weights', 'candidates', 'k', 'lam', 'unsupported']
  assert list(inspect.signature(VideoIndex.search_diverse).parameters) == [
      'self', 'embds', 'weights', 'k', 'lam', 'shortlist', 'subset', 'exclude', 'coarse', 'unsupported']
  defaults = inspect.signature(VideoIndex.search_diverse).parameters
  assert defaults['k'].default == 10 and defaults['lam'].default == 0.5 and defaults['shortlist'].default == search.MAX_K == 128
  assert VideoIndex._list_batches(70, 128) == [(0, 70)] and VideoIndex._list_batches(0, 5) == []
  assert VideoIndex._list_batches(2000, 128) == [(0, 768), (768, 1536), (1536, 2000)]      # 768 * 64 KiB = 48 MiB
