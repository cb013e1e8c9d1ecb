"""The host side of VideoIndex.search_groups (mmt_search_topk_groups, its bf16 form and mmt_search_merge_group_lists) without a
GPU: the brute-force definition the GPU tests hold the kernels to, the list algorithm of search_group.hip restated in numpy
against it, the header and the ctypes table, the argument gates and the argument errors of the calls."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ('mmt_search_merge_group_lists',)  # the grouped scan: tests/test_search_abi_cpu.py
INF = float('inf')


def best_first(scores):
  """Item numbers by `search`'s order along the last axis: score descending with -0.0 tied to +0.0, equal scores by ascending
  item (a stable sort of the negated scores)."""
  return np.argsort(-(np.asarray(scores).astype(np.float64) + 0.0), axis=-1, kind='stable').astype(np.int64)


def brute_groups(scores_row, group_ids, k, allowed=None, order=None):
  """The definition, for one query: (scores float32, groups int64, items int64), each of length min(k, groups that have an
  allowed member).  Per group the member with the largest key under `search`'s order -- score descending with -0.0 tied
  to +0.0, equal scores by ascending item -- among the `allowed` items (bool [NV], None = all); the groups sorted by
  their representatives under the same order.  A score keeps the bits it has in scores_row.  `order`: best_first of the row,
  where the caller has it already."""
  scores_row = np.asarray(scores_row)
  group_ids = np.asarray(group_ids).astype(np.int64)
  items = best_first(scores_row) if order is None else order                       # best first
  if allowed is not None:
    items = items[np.asarray(allowed, bool)[items]]
  _, first = np.unique(group_ids[items], return_index=True)                         # a group's first = its representative
  reps = items[np.sort(first)][:k]
  return scores_row[reps], group_ids[reps], reps


def padded_groups(matrix, group_ids, k, allowed=None, order=None):
  """brute_groups row by row -> (scores [NQ, k] float32, groups [NQ, k] int64, items [NQ, k] int64), the slots without a
  group holding (-inf, -1, -1).  `order`: best_first of the matrix, computed here unless given."""
  nq = matrix.shape[0]
  order = best_first(matrix) if order is None else order
  scores = np.full((nq, k), -INF, np.float32)
  groups = np.full((nq, k), -1, np.int64)
  items = np.full((nq, k), -1, np.int64)
  for r in range(nq):
    s, g, i = brute_groups(matrix[r], group_ids, k, allowed, order[r])
    scores[r, :s.size], groups[r, :s.size], items[r, :s.size] = s, g, i
  return scores, groups, items


# ---- the list algorithm of search_group.hip, restated ---------------------------------------------------------------------

def _key(score, item):
  """tk_key of search_topk.h as a Python int: order-preserving score bits above, ~item below; 0 is "no candidate"."""
  u = int(np.float32(score).view(np.uint32))
  if not u & 0x7fffffff:
    u = 0
  u = (~u & 0xffffffff) if u & 0x80000000 else (u | 0x80000000)
  return (u << 32) | (~int(item) & 0xffffffff)


def _item(key):
  return ~key & 0xffffffff


def _compact(c, k, gids):
  """gk_compact: drops every candidate for which the list holds a larger key of the same group, sorts the survivors and
  keeps the best k -> (the row, the number of survivors)."""
  best = {}
  for x in c:
    g = gids[_item(x)]
    best[g] = max(best.get(g, 0), x)
  survivors = sorted((x for x in c if best[gids[_item(x)]] == x), reverse=True)
  return survivors[:k], len(survivors)


def _chunk_list(row, gids, k, g_begin, g_end, allowed, stats):
  """One (query, chunk) of group_scan_kernel: 64 columns per push, capacity k + 64, the threshold rule, the flush."""
  c, thr = [], 0
  for g0 in range(g_begin, g_end, 64):
    if len(c) > k:
      c, survivors = _compact(c, k, gids)
      stats['compactions'] += 1
      if survivors >= k:
        assert c[k - 1] >= thr                 # the threshold only rises
        thr = c[k - 1]
      else:
        assert thr == 0                        # fewer than k distinct groups: c[k - 1] would be a stale slot
    for g in range(g0, min(g0 + 64, g_end)):
      if allowed is None or allowed[g]:
        key = _key(row[g], g)
        if key > thr:
          c.append(key)
    assert len(c) <= k + 64
    stats['peak'] = max(stats['peak'], len(c))
  if c:
    c, _ = _compact(c, k, gids)
  return c + [0] * (k - len(c))


def _merge(lists, k, gids):
  """gm_select: the heads popped in descending key order, a key whose group is out already dropped."""
  out, taken = [], set()
  heads = [0] * len(lists)
  while len(out) < k:
    best = max(range(len(lists)), key=lambda c: lists[c][heads[c]] if heads[c] < k else 0)
    key = lists[best][heads[best]] if heads[best] < k else 0
    if not key:
      break
    heads[best] += 1
    if gids[_item(key)] not in taken:
      taken.add(gids[_item(key)])
      out.append(key)
  return out


def list_algorithm(row, gids, k, chunk, allowed=None, stats=None):
  stats = stats if stats is not None else {'compactions': 0, 'peak': 0}
  nv = len(row)
  lists = [_chunk_list(row, gids, k, g, min(nv, g + chunk), allowed, stats) for g in range(0, nv, chunk)]
  items = np.array([_item(x) for x in _merge(lists, k, gids)], np.int64)
  return row[items], np.asarray(gids, np.int64)[items], items


def test_brute_groups_on_hand_made_rows():
  #                 0     1     2    3    4     5     6    7
  row = np.float32([0.5, -0.0, 0.25, 0.0, 0.5, -1.0, 0.75, 0.0])
  gids = np.int64([7, 3, 7, 9, 11, 3, 3, 40])
  s, g, i = brute_groups(row, gids, 10)                                     # k above the group count: every group, once
  assert i.tolist() == [6, 0, 4, 3, 7] and g.tolist() == [3, 7, 11, 9, 40]  # 0.5 ties between groups 7 and 11: item order
  assert i.dtype == g.dtype == np.int64 and s.dtype == np.float32
  assert np.array_equal(s.view(np.int32), row[i].view(np.int32))
  assert brute_groups(row, gids, 2)[2].tolist() == [6, 0]
  assert brute_groups(row, gids, 1)[1].tolist() == [3]
  allowed = np.array([1, 1, 1, 1, 1, 1, 0, 1], bool)                         # group 3 loses its best member
  s, g, i = brute_groups(row, gids, 10, allowed)
  assert i.tolist() == [0, 4, 1, 3, 7]                  # ... and is represented by item 1, -0.0, tied with the +0.0 of 3 and 7
  assert np.signbit(s).tolist() == [False, False, True, False, False]
  tie_inside = brute_groups(np.float32([1, 2, 2, 2]), np.int64([5, 6, 6, 5]), 5)     # a tie inside a group and across two
  assert tie_inside[2].tolist() == [1, 3] and tie_inside[1].tolist() == [6, 5]
  allowed = np.array([1, 0, 1, 1, 1, 0, 0, 1], bool)                         # group 3 wholly disallowed
  s, g, i = brute_groups(row, gids, 10, allowed)
  assert g.tolist() == [7, 11, 9, 40] and i.tolist() == [0, 4, 3, 7]
  ps, pg, pi = padded_groups(row[None], gids, 5, allowed)
  assert pg.tolist() == [[7, 11, 9, 40, -1]] and pi.tolist() == [[0, 4, 3, 7, -1]] and ps[0, 4] == -INF


def _groupings(rng, nv, k, chunk):
  every = np.arange(nv)
  flood = 7 * every + 3
  flood[chunk:chunk + min(nv - chunk, k + 64 + 9)] = 1                        # more than k + 64 members inside one chunk
  spread = 11 * every + 5
  spread[::chunk] = 2                                                         # one group with a member in every chunk
  return {'singletons': 7 * every + 3, 'one': np.full(nv, 12), 'runs': every // 5, 'strided': every % 37, 'flood': flood,
          'spread': spread, 'random': rng.integers(0, max(1, nv // 3), nv) * 3}


@pytest.mark.parametrize('nv,chunk,k', [(1, 128, 1), (130, 128, 1), (300, 128, 3), (700, 256, 10), (520, 256, 128),
                                        (400, 128, 40)])
def test_list_algorithm_equals_the_definition(nv, chunk, k):
  """Scores from a handful of values, both zeros among them, so ties abound; every grouping; no subset, a random half and a
  subset that removes each group's best member."""
  rng = np.random.default_rng(nv + k)
  values = np.float32([-1.5, -0.0, 0.0, 0.25, 0.5, 0.75, 1.0, 3.0])
  stats = {'compactions': 0, 'peak': 0}
  for name, gids in _groupings(rng, nv, k, chunk).items():
    n_groups = np.unique(gids).size
    for trial in range(3):
      row = rng.choice(values, nv) if trial else rng.standard_normal(nv).astype(np.float32)
      if name == 'flood' and trial == 2:
        row = np.sort(row)                      # ascending: every member of the flood group beats the ones before it
      best = np.zeros(nv, bool)
      best[brute_groups(row, gids, nv)[2]] = True
      for allowed in (None, rng.random(nv) < 0.5, ~best):
        if allowed is not None and not allowed.any():
          continue
        want = brute_groups(row, gids, k, allowed)
        got = list_algorithm(row, gids, k, chunk, allowed, stats)
        assert want[2].size == min(k, np.unique(gids[allowed]).size if allowed is not None else n_groups)
        assert np.array_equal(got[2], want[2]) and np.array_equal(got[1], want[1]), (name, trial)
        assert np.array_equal(got[0].view(np.int32), want[0].view(np.int32)), (name, trial)
  if nv > k + 64:
    assert stats['compactions'] > 0 and stats['peak'] > k


def test_signatures_of_the_new_exports_agree_with_the_header():
  from mmt_amd import _lib
  src = open(os.path.join(ROOT, 'include', 'mmt_hip.h')).read()
  handle = ctypes.CDLL(_lib.LIB_PATH)
  arity = {'mmt_search_merge_group_lists': 12}
  for name in NEW_EXPORTS:
    m = re.search(r'\b(int|int64_t) %s\(([^;]*?)\);' % name, src)
    assert m, name + ' is not declared in mmt_hip.h'
    params = [p.strip() for p in m.group(2).replace('\n', ' ').split(',')]
    res, args = _lib.SIGNATURES[name]
    assert res is (ctypes.c_int if m.group(1) == 'int' else ctypes.c_int64), name
    assert len(args) == len(params) == arity[name], name
    for p, a in zip(params, args):
      assert (a is ctypes.c_void_p) == ('*' in p) and (a is ctypes.c_int) == (p.startswith('int ')), (name, p)
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
  buf = (ctypes.c_char * 256)()
  base = ctypes.addressof(buf)
  base += -base % 16
  p = ctypes.c_void_p(base)
  merge = fns['mmt_search_merge_group_lists']   # scores groups index ids S NQ kin kout out_scores out_groups out_items stream
  good = [p, p, p, p, 1, 1, 1, 1, p, p, p, None]
  for missing in (0, 1, 2, 3, 8, 9, 10):
    args = list(good)
    args[missing] = None
    assert merge(*args) == -1, missing
  for at, value in ((4, 0), (4, 33), (5, 0), (6, 0), (6, 129), (7, 0), (7, 129)):   # S NQ kin kout
    args = list(good)
    args[at] = value
    assert merge(*args) == -1, (at, value)


def _hollow_index(num_items, dtype=torch.float32):
  """A VideoIndex with its bookkeeping and no storage: the argument checks come before anything reads it."""
  from mmt_amd.search import VideoIndex
  index = VideoIndex.__new__(VideoIndex)
  index.capacity, index.num_experts, index.dim, index.num_items = 8, 2, 8, num_items
  index.device, index.dtype = torch.device('cuda', 0), dtype
  return index


def _hollow_sharded(num_items):
  from mmt_amd.search import ShardedVideoIndex
  sharded = ShardedVideoIndex.__new__(ShardedVideoIndex)
  sharded.num_items, sharded.num_experts, sharded.dim, sharded.device = num_items, 2, 8, torch.device('cuda', 0)
  sharded.shards = []
  return sharded


@pytest.mark.parametrize('hollow', [_hollow_index, _hollow_sharded], ids=['VideoIndex', 'ShardedVideoIndex'])
def test_argument_errors_are_raised_without_a_device(hollow):
  from mmt_amd.search import IndexGrouping, IndexSubset, ShardedGrouping, ShardedVideoIndex, VideoIndex
  cls = 'VideoIndex' if hollow is _hollow_index else 'ShardedVideoIndex'
  kind = IndexGrouping if hollow is _hollow_index else ShardedGrouping
  q, qw = torch.zeros(3, 2, 8), torch.zeros(3, 2)
  ids = torch.tensor([4, 4, 9, 0, 2 ** 31 - 2])
  with pytest.raises(ValueError, match='holds no items'):
    hollow(0).grouping(ids)
  index = hollow(5)
  for bad in ([4, 4, 9, 0, 1], np.int64([4, 4, 9, 0, 1]), None, ids.to(torch.int32), ids.double(), ids > 3):
    with pytest.raises(ValueError, match='group_ids must be an int64 tensor'):
      index.grouping(bad)
  with pytest.raises(ValueError, match='index device'):
    index.grouping(ids)                                         # host ids for a device index
  index.device = torch.device('cpu')                            # lets the value checks be reached with host tensors
  for bad in (ids[:4], torch.zeros(6, dtype=torch.int64), ids.reshape(5, 1), ids.reshape(1, 5), torch.tensor(3)):
    with pytest.raises(ValueError, match=r'group_ids of shape \(5,\) expected'):
      index.grouping(bad)
  for bad, text in ((torch.tensor([0, 1, -1, 2, 3]), r'-1 \.\. 3'), (torch.tensor([0, 1, 2 ** 31 - 1, 2, 3]), '2147483647'),
                    (torch.tensor([0, 1, 2 ** 40, 2, 3]), str(2 ** 40))):
    with pytest.raises(ValueError, match=r'must lie in 0 \.\. 2147483646, got.*' + text):
      index.grouping(bad)
  grp = index.grouping(ids)                                      # nothing of the build needs the device
  assert isinstance(grp, kind) and grp.num_groups == 4 and grp.num_items == 5 and grp.device == index.device
  assert grp.ids.dtype == torch.int32 and grp.ids.tolist() == ids.tolist()
  # search_groups: k, the grouping, the subset, then the queries
  for bad in (0, 129, -1, 2.0, True, None):
    with pytest.raises(ValueError, match=r'k must be an int in 1\.\.128'):
      index.search_groups(q, qw, grp, k=bad)
  for foreign in (ids, None, 'runs', IndexGrouping(grp.ids, 4) if kind is ShardedGrouping else ShardedGrouping([], grp.ids, 4)):
    with pytest.raises(ValueError, match='grouping must come from %s.grouping' % cls):
      index.search_groups(q, qw, foreign)
  index.num_items = 6                                            # a further add: the grouping is stale
  with pytest.raises(ValueError, match='the grouping was built for 5 items, the index holds 6'):
    index.search_groups(q, qw, grp)
  index.num_items = 5
  with pytest.raises(ValueError, match='subset must come from %s.subset' % cls):
    index.search_groups(q, qw, grp, subset=torch.ones(5, dtype=torch.bool))
  if kind is IndexGrouping:
    stale = IndexSubset.__new__(IndexSubset)
    stale.num_items, stale.device = 4, index.device
    with pytest.raises(ValueError, match='the subset was built for 4 items, the index holds 5'):
      index.search_groups(q, qw, grp, subset=stale)
  with pytest.raises(ValueError, match='CUDA tensor'):
    index.search_groups(q, qw, grp)                              # the queries themselves are host tensors
  with pytest.raises(ValueError, match='holds no items'):
    hollow(0).search_groups(q, qw, grp)
  # neither exclusions nor normalisation are part of the call
  for extra in ('exclude', 'norm', 'dynamic'):
    with pytest.raises(TypeError):
      index.search_groups(q, qw, grp, **{extra: None})
  # both classes have one surface
  for method in ('grouping', 'search_groups'):
    assert (inspect.signature(getattr(ShardedVideoIndex, method)).parameters.keys() ==
            inspect.signature(getattr(VideoIndex, method)).parameters.keys())
  assert list(inspect.signature(VideoIndex.search_groups).parameters) == ['self', 'embds', 'weights', 'grouping', 'k', 'subset']
  assert inspect.signature(VideoIndex.search_groups).parameters['k'].default == 10
