"""The host side of cursor paging (VideoIndex.search(after=), search_deep; mmt_search_topk_after and its kin) without a GPU:
the definition the GPU tests hold the kernels to, the bound arithmetic of search_topk.h restated on plain integers and
held to it -- on one index and cut into shards --, the header and the ctypes table, the argument gates of the entry points
and the argument errors of the calls."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests.test_index_groups_cpu import _hollow_index, _hollow_sharded, _key, best_first

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = {'mmt_search_after_keys': 5}  # the scan that takes the bounds: tests/test_search_abi_cpu.py
INF = float('inf')
NO_CURSOR, EXHAUSTED = (INF, -1), (-INF, -1)


def admitted(scores_row, a_score, a_item):
  """The definition of a cursor row, for one query: bool per item -- is it a candidate after the position?  a_item >= 0:
  the items scoring below a_score, and at a_score (-0.0 == +0.0: a plain float compare) those numbered above a_item.
  (+inf, -1): every item.  (-inf, -1): none."""
  s = np.asarray(scores_row, np.float32)
  if a_item < 0:
    assert np.isinf(a_score)
    return np.full(s.shape, a_score > 0)
  a = np.float32(a_score)
  return (s < a) | ((s == a) & (np.arange(s.size) > a_item))


def complete_list(scores_row, allowed=None):
  """Every candidate of one query, best first under `search`'s order -> (scores float32, items int64).  A score keeps its
  bits but for a -0.0, which `search` returns as +0.0."""
  s = np.asarray(scores_row, np.float32)
  order = best_first(s)
  if allowed is not None:
    order = order[np.asarray(allowed, bool)[order]]
  return s[order] + np.float32(0.0), order


def slice_after(scores_row, a_score, a_item, k, allowed=None):
  """search(after=) for one query by the definition: the first k of the complete list of the candidates that are admitted,
  padded with (-inf, -1) -> (scores float32 [k], items int64 [k])."""
  keep = admitted(scores_row, a_score, a_item)
  if allowed is not None:
    keep = keep & np.asarray(allowed, bool)
  s, i = complete_list(scores_row, keep)
  scores, items = np.full(k, -INF, np.float32), np.full(k, -1, np.int64)
  n = min(k, i.size)
  scores[:n], items[:n] = s[:n], i[:n]
  return scores, items


def bound(a_score, first):
  """mmt_search_after_keys on plain integers: the uint64 bound of a cursor row.  first >= 0 is the lowest item number still
  admitted at the cursor's score; first < 0 selects a sentinel by the sign of the score."""
  if first < 0:
    return 2 ** 64 - 1 if a_score > 0 else 0
  return _key(a_score, first) + 1


def _scores_with_everything():
  """A row of 40 scores: ties, both zeros, the denormals around them, both infinities."""
  f = np.float32
  base = [0.5, 0.5, -0.0, 0.0, 1e-45, -1e-45, INF, -INF, 0.25, 0.5, -0.5, 0.0, -0.0, INF, -INF, 3.0, -3.0, 0.25]
  gen = np.random.default_rng(3)
  return f(base + list(np.round(gen.standard_normal(40 - len(base)), 1)))


CURSOR_SCORES = [0.5, 0.25, 0.0, -0.0, 1e-45, -1e-45, INF, -INF, 0.3, -0.5, 3.0, 3.5, -3.5, 0.1]


def test_definition_on_rows_worked_by_hand():
  s = np.float32([1, 1, 2, 1, -0.0, 0.0, 1])
  assert complete_list(s)[1].tolist() == [2, 0, 1, 3, 6, 4, 5]
  assert slice_after(s, 1.0, 1, 3)[1].tolist() == [3, 6, 4]                   # behind (1, item 1): the later items at 1
  assert slice_after(s, 1.0, 6, 3)[1].tolist() == [4, 5, -1]                  # the last of the tie: only the zeros are left
  assert slice_after(s, 1.5, 0, 2)[1].tolist() == [0, 1]                      # no item scores 1.5: everything below it
  assert slice_after(s, 1.0, 2, 9)[1].tolist() == [3, 6, 4, 5] + [-1] * 5     # item 2 does not score 1: an arbitrary number
  assert slice_after(s, 0.0, 4, 2)[1].tolist() == [5, -1]                     # -0 ties with +0
  assert slice_after(s, -0.0, 4, 2)[1].tolist() == [5, -1]                    # ... in the cursor too
  zeros = slice_after(s, 1.0, 6, 3)[0]
  assert zeros[:2].tolist() == [0, 0] and not np.signbit(zeros[:2]).any() and np.isneginf(zeros[2])
  assert slice_after(s, *NO_CURSOR, 3)[1].tolist() == [2, 0, 1]
  assert slice_after(s, *EXHAUSTED, 3)[1].tolist() == [-1, -1, -1]
  assert slice_after(s, 1.0, 0, 3, allowed=[1, 0, 1, 0, 1, 1, 1])[1].tolist() == [6, 4, 5]   # a subset on top
  # pages: each continues from the last column of the one before, and together they are the complete list
  want = complete_list(s)
  pages, cursor = [], NO_CURSOR
  for _ in range(4):
    page = slice_after(s, *cursor, 2)
    pages.append(page)
    cursor = (page[0][-1], page[1][-1])
  got = np.concatenate([p[1] for p in pages])
  assert got[:7].tolist() == want[1].tolist() and got[7] == -1 and cursor == EXHAUSTED


def test_a_key_below_the_bound_is_an_item_after_the_position():
  """tk_key(a, first) + 1 with first = item + 1 admits exactly the items of the definition; first = 0 admits every item
  at the cursor's score and first = count none of them; the two sentinels admit everything and nothing."""
  s = _scores_with_everything()
  n = s.size
  keys = [_key(v, g) for g, v in enumerate(s)]
  assert all(0 < x < 2 ** 64 - 1 for x in keys)                                 # no key is a sentinel
  for a in CURSOR_SCORES:
    for item in list(range(n)) + [2 ** 31 - 2]:
      b = bound(a, item + 1)
      assert b == _key(a, item)                                                 # the low word of a key is ~item
      assert 0 < b < 2 ** 64 - 1
      if item < n:
        assert [x < b for x in keys] == admitted(s, a, item).tolist(), (a, item)
    below, at = s < np.float32(a), s == np.float32(a)
    assert [x < bound(a, 0) for x in keys] == (below | at).tolist(), a        # first = 0: the carry into the score word
    assert [x < bound(a, n) for x in keys] == below.tolist(), a               # first = count
  assert [x < bound(*NO_CURSOR) for x in keys] == [True] * n
  assert [x < bound(*EXHAUSTED) for x in keys] == [False] * n
  assert bound(-0.0, 5) == bound(0.0, 5)
  assert bound(INF, 0) == (0xff800000 + 1) << 32 and bound(-INF, 0) < bound(-3.5, 0) < bound(-0.0, 0) < bound(INF, 0)


@pytest.mark.parametrize('tables', [
    [[0, 1, 2, 3, 4], [5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19], list(range(20, 40))],     # contiguous
    [list(range(0, 40, 3)), list(range(1, 40, 3)), list(range(2, 40, 3))],                                 # interleaved
    [list(range(0, 25)), list(range(25, 40)), []],                                                         # one empty
], ids=['contiguous', 'interleaved', 'one_empty'])
def test_the_bound_restated_per_shard_admits_the_same_items(tables):
  """first_s = searchsorted(ids_s, cursor item, right=True) -- the count of the shard's items numbered at or below the
  cursor's -- reproduces the global tie rule in local numbers, including 0 and the shard's item count."""
  s = _scores_with_everything()
  seen = set()
  for a in CURSOR_SCORES:
    for item in range(s.size):
      want = admitted(s, a, item)
      got = np.zeros(s.size, bool)
      for ids in tables:
        ids = np.asarray(ids, np.int64)
        first = int(np.searchsorted(ids, item, side='right'))
        seen.add((first == 0, first == ids.size))
        b = bound(a, first)
        for local, g in enumerate(ids):
          got[g] = _key(s[g], local) < b
      assert got.tolist() == want.tolist(), (a, item)
    for sentinel in (NO_CURSOR, EXHAUSTED):                                      # a sentinel is the same on every shard
      assert bound(*sentinel) in (0, 2 ** 64 - 1)
  assert (True, False) in seen and (False, True) in seen


def test_limits_checks_the_cursor_values_and_gives_first():
  from mmt_amd import search
  f, i = (lambda v: torch.tensor(v, dtype=torch.float32)), (lambda v: torch.tensor(v, dtype=torch.int64))
  ex, cur = search._limits(None, (f([0.5, INF, -INF, -0.0, INF]), i([3, -1, -1, 0, 9])), 5, 10)
  assert ex is None and cur[1].tolist() == [4, -1, -1, 1, 10] and cur[1].dtype is torch.int64
  assert cur[0].tolist() == [0.5, INF, -INF, -0.0, INF] and cur[0].dtype is torch.float32
  assert search._limits(None, None, 5, 10) == (None, None)
  for scores, items, text in (([0.5, float('nan')], [3, 3], 'after must not be NaN'),
                              ([float('nan'), INF], [-1, -1], 'after must not be NaN'),
                              ([0.5, 0.5], [3, -1], r'-1 in after goes with a score of \+inf'),
                              ([0.5, 0.0], [3, -1], r'-1 in after goes with'),
                              ([0.5, 0.5], [3, 10], r'items of after must lie in -1 \.\. 9, got 3 \.\. 10'),
                              ([0.5, -INF], [3, -2], r'items of after must lie in -1 \.\. 9, got -2 \.\. 3')):
    with pytest.raises(ValueError, match=text):
      search._limits(None, (f(scores), i(items)), 2, 10)
  with pytest.raises(ValueError, match='2 queries but after holds 3 rows'):
    search._limits(None, (f([1, 1, 1]), i([0, 0, 0])), 2, 10)
  # together with the exclusions: both are checked, the exclusions' message as it always was
  ex, cur = search._limits(i([[0, -1], [9, 2]]), (f([0.5, INF]), i([3, -1])), 2, 10)
  assert ex.tolist() == [[0, -1], [9, 2]] and cur[1].tolist() == [4, -1]
  with pytest.raises(ValueError, match=r'exclude must lie in -1 \.\. 9, got -1 \.\. 10'):
    search._limits(i([[0, -1], [10, 2]]), (f([0.5, INF]), i([3, -1])), 2, 10)
  with pytest.raises(ValueError, match='after must not be NaN'):
    search._limits(i([[0, -1], [9, 2]]), (f([0.5, float('nan')]), i([3, -1])), 2, 10)
  assert search._limits(i([1, 2]), None, 2, 10)[0].tolist() == [[1], [2]]        # exclusions alone, [NQ] -> [NQ, 1]


def _params(src, name):
  m = re.search(r'\b(int|int64_t) %s\(([^;]*?)\);' % name, src)
  assert m, name + ' is not declared in mmt_hip.h'
  return m.group(1), [p.strip() for p in m.group(2).replace('\n', ' ').split(',')]


def test_signatures_of_the_new_exports_agree_with_the_header():
  from mmt_amd import _lib
  src = open(os.path.join(ROOT, 'include', 'mmt_hip.h')).read()
  handle = ctypes.CDLL(_lib.LIB_PATH)
  for name, arity in NEW_EXPORTS.items():
    res, params = _params(src, name)
    restype, args = _lib.SIGNATURES[name]
    assert res == 'int' and restype is ctypes.c_int, name
    assert len(args) == len(params) == arity, name
    for p, a in zip(params, args):
      assert (a is ctypes.c_void_p) == ('*' in p) and (a is ctypes.c_int) == (p.startswith('int ')) and \
          (a is ctypes.c_float) == (p.startswith('float ')), (name, p)
    assert hasattr(handle, name)
  assert _params(src, 'mmt_search_after_keys')[1] == ['const float* scores', 'const int64_t* first', 'int NQ', 'uint64_t* keys',
                                                      'void* stream']
  assert handle.mmt_abi_version() == 6


def test_new_exports_gate_their_arguments_on_the_host():
  """Every refusal below returns before any launch: MMT_ERR_ARG = -1, MMT_ERR_ALIGN = -2."""
  from mmt_amd import _lib
  handle = ctypes.CDLL(_lib.LIB_PATH)
  fns = {}
  for name in NEW_EXPORTS:
    fns[name] = getattr(handle, name)
    fns[name].restype, fns[name].argtypes = _lib.SIGNATURES[name]
  buf = (ctypes.c_char * 256)()
  base = ctypes.addressof(buf)
  base += -base % 16
  p = ctypes.c_void_p(base)
  keys = fns['mmt_search_after_keys']
  for args in ((None, p, 1, p, None), (p, None, 1, p, None), (p, p, 1, None, None), (p, p, 0, p, None), (p, p, -1, p, None)):
    assert keys(*args) == -1, args


@pytest.mark.parametrize('hollow', [_hollow_index, _hollow_sharded], ids=['VideoIndex', 'ShardedVideoIndex'])
def test_argument_errors_are_raised_without_a_device(hollow):
  from mmt_amd import search
  from mmt_amd.search import ShardedVideoIndex, VideoIndex
  q, qw = torch.zeros(3, 2, 8), torch.zeros(3, 2)
  a_s, a_i = torch.full((3,), INF), torch.full((3,), -1, dtype=torch.int64)
  index = hollow(5)
  for bad in (a_s, [a_s], (a_s, a_i, a_i), 'next', 7, (a_s, None), (a_s.double(), a_i), (a_s, a_i.to(torch.int32)),
              (a_i, a_s), (a_s.numpy(), a_i.numpy())):
    with pytest.raises(ValueError, match=r'after must be None or a pair \(scores float32 \[NQ\], items int64 \[NQ\]\)'):
      index.search(q, qw, after=bad)
  with pytest.raises(ValueError, match='after must be on the index device cuda:0, got cpu'):
    index.search(q, qw, after=(a_s, a_i))                          # a host cursor for a device index
  index.device = torch.device('cpu')                               # lets the later checks be reached with host tensors
  for bad in ((a_s[:, None], a_i[:, None]), (a_s, a_i[:2]), (a_s[0], a_i[0]), (a_s.reshape(3, 1), a_i)):
    with pytest.raises(ValueError, match=r'after \(scores \[NQ\], items \[NQ\]\) expected'):
      index.search(q, qw, after=bad)
  for extra in ('pooling', 'item_pooling'):                        # refused by name before either is looked at
    with pytest.raises(ValueError, match='after= does not combine with pooling= or item_pooling='):
      index.search(q, qw, after=(a_s, a_i), **{extra: object()})
  with pytest.raises(ValueError, match='CUDA tensor'):
    index.search(q, qw, after=(a_s, a_i))                          # the cursor passed: the queries are host tensors
  for bad in (0, -1, 2.0, True, None, '300'):
    with pytest.raises(ValueError, match='search_deep: depth must be an int >= 1'):
      index.search_deep(q, qw, bad)
  for bad in (0, 129, -1, 64.0, True, None):
    with pytest.raises(ValueError, match=r'search_deep: page must be an int in 1\.\.128'):
      index.search_deep(q, qw, 300, page=bad)
  with pytest.raises(ValueError, match='holds no items'):
    hollow(0).search_deep(q, qw, 300)
  with pytest.raises(ValueError, match='CUDA tensor'):
    index.search_deep(q, qw, 300, page=7)
  # one surface on both classes; the cursor is the last argument of `search` and no part of the grouped search
  for method in ('search', 'search_deep'):
    assert getattr(ShardedVideoIndex, method) is getattr(VideoIndex, method)
  assert list(inspect.signature(VideoIndex.search).parameters) == [
      'self', 'embds', 'weights', 'k', 'subset', 'exclude', 'norm', 'dynamic', 'pooling', 'item_pooling', 'after']
  assert inspect.signature(VideoIndex.search).parameters['after'].default is None
  deep = inspect.signature(VideoIndex.search_deep).parameters
  assert list(deep) == ['self', 'embds', 'weights', 'depth', 'page', 'subset', 'exclude', 'norm', 'dynamic']
  assert deep['page'].default == search.DEEP_PAGE == 64 and search.MAX_K == 128     # the default page is a measured choice
  for method in ('search_groups', 'search_refined', 'rescore'):
    assert 'after' not in inspect.signature(getattr(VideoIndex, method)).parameters
  with pytest.raises(TypeError):
    index.search_groups(q, qw, None, after=(a_s, a_i))


def test_the_dynamic_rule_decides_without_the_cursor_and_falls_back_with_it():
  from mmt_amd.search import _Scan
  cursor = (torch.zeros(2), torch.zeros(2, dtype=torch.int64))
  scan = _Scan(subset='s', ex='e', norm='n', after=cursor)
  plain, decide, moved = scan.plain(), scan.uncursored(), scan.at(None)
  assert (plain.subset, plain.ex, plain.norm, plain.after) == ('s', 'e', None, cursor)
  assert (decide.subset, decide.ex, decide.norm, decide.after) == ('s', 'e', None, None)
  assert (moved.subset, moved.ex, moved.norm, moved.after) == ('s', 'e', 'n', None)
  assert _Scan().after is None and _Scan().plain().after is None
