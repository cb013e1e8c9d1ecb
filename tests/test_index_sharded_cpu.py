"""The host side of the sharded index (search.ShardedVideoIndex; mmt_search_thresholds, mmt_search_count, their bf16 forms,
mmt_count_workspace_ints and mmt_search_merge_lists) without a GPU: the header and the ctypes table agree, the argument
gates, the placement rule as a pure function, and the merge restated in numpy -- the answer the GPU tests hold the kernel
to."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ('mmt_count_workspace_ints', 'mmt_search_merge_lists')  # the two scans: tests/test_search_abi_cpu.py


def merge_reference(scores, index, ids, kout):
  """The expected answer of mmt_search_merge_lists, restated: scores fp32 / index int64 [S, NQ, kin] (index -1 = empty
  slot), ids a list of S int64 local -> global tables -> (scores fp32 [NQ, kout], index int64 [NQ, kout]): per query the
  candidates of all lists by descending score (-0.0 and +0.0 compare equal), equal scores by ascending global item, cut to
  kout, then (-inf, -1).  A score keeps its bits."""
  scores, index = np.asarray(scores, np.float32), np.asarray(index, np.int64)
  n_lists, nq, _ = scores.shape
  out_s = np.full((nq, kout), -np.inf, np.float32)
  out_i = np.full((nq, kout), -1, np.int64)
  for q in range(nq):
    cand = [(scores[s, q, j], int(ids[s][index[s, q, j]])) for s in range(n_lists) for j in np.flatnonzero(index[s, q] >= 0)]
    if cand:
      sc = np.array([c[0] for c in cand], np.float32)
      gid = np.array([c[1] for c in cand], np.int64)
      order = np.lexsort((gid, -sc.astype(np.float64)))[:kout]   # -(-0.0) == -(+0.0): a tie, broken by the item number
      out_s[q, :order.size], out_i[q, :order.size] = sc[order], gid[order]
  return out_s, out_i


def _bits(x):
  return np.ascontiguousarray(x, np.float32).view(np.int32)


def test_merge_reference_on_hand_made_lists():
  inf = np.inf
  ids = [np.array([1, 4, 6]), np.array([0, 2, 3, 5]), np.array([7])]
  # [query][list][slot]: query 0 has ties across lists with interleaving item numbers, query 1 -0.0 against +0.0 and
  # short lists, query 2 nothing at all
  scores = np.float32([[[0.5, 0.5, 0.25], [0.5, 0.5, 0.5], [0.75, -inf, -inf]],
                       [[0.0, -1.0, -inf], [-0.0, -0.0, -inf], [-inf, -inf, -inf]],
                       [[-inf, -inf, -inf], [-inf, -inf, -inf], [-inf, -inf, -inf]]]).transpose(1, 0, 2)
  index = np.int64([[[0, 2, 1], [0, 1, 3], [0, -1, -1]],
                    [[1, 0, -1], [1, 3, -1], [-1, -1, -1]],
                    [[-1, -1, -1], [-1, -1, -1], [-1, -1, -1]]]).transpose(1, 0, 2)
  s, i = merge_reference(scores, index, ids, 8)
  assert i.tolist() == [[7, 0, 1, 2, 5, 6, 4, -1], [2, 4, 5, 1, -1, -1, -1, -1], [-1] * 8]
  assert s[0].tolist() == [0.75, 0.5, 0.5, 0.5, 0.5, 0.5, 0.25, -inf]
  # items 2 (-0.0), 4 (+0.0), 5 (-0.0): one tie, in item order, every score with its own sign bit
  assert _bits(s[1, :3]).tolist() == _bits(np.float32([-0.0, 0.0, -0.0])).tolist() and s[1, 3] == -1.0
  assert np.isneginf(s[1, 4:]).all() and np.isneginf(s[2]).all()
  # a cut is a prefix; kout may exceed the candidates and S * kin
  for kout in (1, 3, 7):
    s2, i2 = merge_reference(scores, index, ids, kout)
    assert np.array_equal(i2, i[:, :kout]) and np.array_equal(_bits(s2), _bits(s[:, :kout]))
  s2, i2 = merge_reference(scores, index, ids, 20)
  assert np.array_equal(i2[:, :8], i) and (i2[:, 8:] == -1).all() and np.isneginf(s2[:, 8:]).all()
  # one list: the list itself, in global numbers
  s1, i1 = merge_reference(scores[:1], index[:1], ids[:1], 3)
  assert i1.tolist() == [[1, 6, 4], [4, 1, -1], [-1, -1, -1]]


def test_placement_rule():
  from mmt_amd.search import place
  assert place([234, 234, 234], [0, 0, 0], 300) == [(0, 234), (1, 66)]        # spills only when the shard is full
  assert place([234, 234, 234], [234, 66, 0], 129) == [(2, 129)]              # the fewest items
  assert place([234, 234, 234], [234, 66, 129], 271) == [(1, 168), (2, 103)]
  assert place([5, 5], [3, 3], 1) == [(0, 1)]                                 # a tie: the lowest number
  assert place([5, 5], [5, 0], 5) == [(1, 5)]
  assert place([2, 2, 2], [0, 0, 0], 6) == [(0, 2), (1, 2), (2, 2)]           # the contiguous near-equal cut
  assert place([1, 1, 0], [0, 0, 0], 2) == [(0, 1), (1, 1)]                   # a shard without rows is never chosen
  assert place([4, 4], [1, 2], 0) == []
  fills = [4, 3]
  with pytest.raises(ValueError, match='do not fit'):
    place([4, 4], fills, 2)
  assert fills == [4, 3]
  assert place([4, 4], fills, 1) == [(1, 1)] and fills == [4, 3]             # pure: the arguments are not changed
  # a full shard that holds the fewest items is passed over
  assert place([1, 8], [1, 5], 2) == [(1, 2)]


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
  size = fns['mmt_count_workspace_ints']
  assert size(64, 4096 * 512, 1) == 64 * 2 * 512                     # full-size chunks
  assert size(63, 127, 3) == 63 * 3 * 2                              # one tile
  assert size(257, 4097, 32) == 257 * 32 * 2 * 33                    # 128-column chunks while the chip is not full
  rank_size = handle.mmt_rank_workspace_ints
  rank_size.restype = ctypes.c_int64
  for shape in ((64, 4096 * 512, 1), (257, 4097, 32), (1, 1, 1)):    # the rank workspace less its thresholds
    assert size(*shape) == rank_size(*shape) - shape[0] * shape[2]
  for bad in ((0, 5, 1), (5, 0, 1), (5, 5, 0), (5, 5, 33)):
    assert size(*bad) == -1
  buf = (ctypes.c_char * 256)()
  base = ctypes.addressof(buf)
  base += -base % 16
  p = ctypes.c_void_p(base)
  merge = fns['mmt_search_merge_lists']       # scores index ids S NQ kin kout out_scores out_index stream
  assert merge(p, p, p, 0, 1, 1, 1, p, p, None) == -1                # S = 0
  assert merge(p, p, p, 33, 1, 1, 1, p, p, None) == -1
  assert merge(p, p, p, 1, 0, 1, 1, p, p, None) == -1                # NQ = 0
  assert merge(p, p, p, 1, 1, 0, 1, p, p, None) == -1                # kin
  assert merge(p, p, p, 1, 1, 129, 1, p, p, None) == -1
  assert merge(p, p, p, 1, 1, 1, 0, p, p, None) == -1                # kout
  assert merge(p, p, p, 1, 1, 1, 129, p, p, None) == -1
  for missing in (0, 1, 2, 7, 8):
    args = [p, p, p, 1, 1, 1, 1, p, p, None]
    args[missing] = None
    assert merge(*args) == -1, missing
