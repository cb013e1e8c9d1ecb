"""The host side of the subset-restricted scans (VideoIndex.subset, search(subset=, exclude=), rank_counts(subset=),
metric.retrieval_metrics_indexed(video_subset=)) without a GPU: the bitmap layout, the restatements the GPU tests compare
against, the argument gates of the five new exports and the errors that need no device."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests.test_index_ranks_cpu import _hollow_index

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ('mmt_search_subset_pack',)  # the scans that take the words: tests/test_search_abi_cpu.py


def pack_reference(mask):
  """bool [n] -> uint32 words, spelled as a loop: bit i & 31 of word i >> 5 is item i; 4 words per 128 items (one scan
  tile = 16 bytes), the padding zero."""
  mask = np.asarray(mask, dtype=bool)
  words = [0] * (4 * -(-mask.size // 128))
  for i in np.flatnonzero(mask):
    words[i >> 5] |= 1 << (int(i) & 31)
  return np.array(words, dtype=np.uint32)


def brute_topk(scores, allowed, exclude, k):
  """The expected answer of search(k, subset, exclude), restated: scores [nq, nv] fp64, allowed bool [nv], exclude None or
  int [nq, E] (-1 = none) -> (scores [nq, k'], indices [nq, k']) with k' = min(k, allowed.sum()): per query the allowed,
  unexcluded items by descending score, equal scores by ascending item number (a stable argsort), then (-inf, -1)."""
  nq, nv = scores.shape
  kout = min(k, int(allowed.sum()))
  s = np.full((nq, kout), -np.inf)
  idx = np.full((nq, kout), -1, np.int64)
  for r in range(nq):
    ok = allowed.copy()
    if exclude is not None:
      ok[exclude[r][exclude[r] >= 0]] = False
    items = np.flatnonzero(ok)
    best = items[np.argsort(-scores[r, items], kind='stable')[:kout]]
    s[r, :best.size] = scores[r, best]
    idx[r, :best.size] = best
  return s, idx


def test_pack_reference_is_little_endian_packbits_padded_to_16_bytes():
  rng = np.random.default_rng(0)
  for n in (1, 31, 32, 33, 127, 128, 129, 255, 256, 4097):
    for mask in (rng.random(n) < 0.5, np.ones(n, bool), np.zeros(n, bool), np.arange(n) == n - 1):
      packed = np.packbits(mask, bitorder='little')
      padded = np.zeros(-(-packed.size // 16) * 16, np.uint8)
      padded[:packed.size] = packed
      want = padded.view('<u4')
      got = pack_reference(mask)
      assert got.dtype == np.uint32 and got.size % 4 == 0 and got.size == 4 * -(-n // 128)
      assert np.array_equal(got, want), n
      assert sum(bin(int(w)).count('1') for w in got) == int(mask.sum())  # nothing set past n


def test_brute_topk_orders_ties_by_item_number_and_pads():
  scores = np.array([[0.5, 0.25, 0.5, 0.5, -0.0, 0.0]])
  allowed = np.array([True, True, False, True, True, True])
  s, i = brute_topk(scores, allowed, None, 10)
  assert i.tolist() == [[0, 3, 1, 4, 5]] and s.tolist() == [[0.5, 0.5, 0.25, 0.0, 0.0]]
  s, i = brute_topk(scores, allowed, np.array([[0, -1, 0, 2]]), 4)
  assert i.tolist() == [[3, 1, 4, 5]]
  s, i = brute_topk(scores, allowed, np.array([[0, 3, 1, 4]]), 5)
  assert i.tolist() == [[5, -1, -1, -1, -1]] and s[0, 0] == 0 and np.isneginf(s[0, 1:]).all()


def test_signatures_of_the_new_exports_agree_with_the_header():
  from mmt_amd import _lib
  src = open(os.path.join(ROOT, 'include', 'mmt_hip.h')).read()
  handle = ctypes.CDLL(_lib.LIB_PATH)
  for name in NEW_EXPORTS:
    m = re.search(r'\bint %s\(([^;]*?)\);' % name, src)
    assert m, name + ' is not declared in mmt_hip.h'
    params = [p.strip() for p in m.group(1).replace('\n', ' ').split(',')]
    res, args = _lib.SIGNATURES[name]
    assert res is ctypes.c_int and len(args) == len(params), name
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
  p, off4, off8 = ctypes.c_void_p(base), ctypes.c_void_p(base + 4), ctypes.c_void_p(base + 8)
  pack = fns['mmt_search_subset_pack']
  assert pack(None, 5, p, None) == -1 and pack(p, 5, None, None) == -1
  assert pack(p, 0, p, None) == -1 and pack(p, -3, p, None) == -1
  assert pack(p, 5, off4, None) == -2 and pack(p, 5, off8, None) == -2


def _hollow_subset(num_items, device):
  from mmt_amd.search import IndexSubset
  sub = IndexSubset.__new__(IndexSubset)
  sub.num_items, sub.device, sub.count = num_items, torch.device(device), 1
  return sub


def test_argument_errors_are_raised_without_a_device():
  from mmt_amd import search
  assert search.MAX_E == 32
  q, qw = torch.zeros(3, 2, 8), torch.zeros(3, 2)
  tg = torch.zeros(3, dtype=torch.int64)
  index = _hollow_index(5)
  with pytest.raises(ValueError, match='holds no items'):
    _hollow_index(0).subset(torch.ones(5, dtype=torch.bool))
  for bad in ([0, 1], np.ones(5, bool), torch.ones(5), torch.ones(5, dtype=torch.int32)):
    with pytest.raises(ValueError, match='bool or int64'):
      index.subset(bad)
  with pytest.raises(ValueError, match='index device'):
    index.subset(torch.ones(5, dtype=torch.bool))          # a host mask for a device index
  host = _hollow_index(5)
  host.device = torch.device('cpu')  # lets the value checks be reached with host tensors
  with pytest.raises(ValueError, match='shape'):
    host.subset(torch.ones(6, dtype=torch.bool))
  for bad in ([-1, 2], [0, 5]):
    with pytest.raises(ValueError, match='0 .. 4'):
      host.subset(torch.tensor(bad))
  with pytest.raises(ValueError, match='no item'):
    host.subset(torch.zeros(5, dtype=torch.bool))
  with pytest.raises(ValueError, match='no item'):
    host.subset(torch.zeros(0, dtype=torch.int64))
  # a subset is tied to the index size and device it was built for
  for call in (lambda s: host.search(q, qw, subset=s), lambda s: host.rank_counts(q, qw, tg, subset=s),
               lambda s: host.ranks(q, qw, tg, subset=s)):
    with pytest.raises(ValueError, match='VideoIndex.subset'):
      call(torch.ones(5, dtype=torch.bool))
    with pytest.raises(ValueError, match='built for 4 items'):
      call(_hollow_subset(4, 'cpu'))
    with pytest.raises(ValueError, match='the subset is on'):
      call(_hollow_subset(5, 'cuda:0'))
  with pytest.raises(ValueError, match='index device'):     # targets are still checked first
    index.rank_counts(q, qw, tg, subset=_hollow_subset(4, 'cuda:0'))
  # exclusions
  for bad in ([0, 1, 2], torch.zeros(3, dtype=torch.int32), torch.zeros(3, 2)):
    with pytest.raises(ValueError, match='int64'):
      index.search(q, qw, exclude=bad)
  for bad in (torch.zeros((), dtype=torch.int64), torch.zeros(3, 0, dtype=torch.int64), torch.zeros(3, 33, dtype=torch.int64),
              torch.zeros(3, 2, 2, dtype=torch.int64)):
    with pytest.raises(ValueError, match='exclude'):
      index.search(q, qw, exclude=bad)
  with pytest.raises(ValueError, match='index device'):
    index.search(q, qw, exclude=torch.zeros(3, 32, dtype=torch.int64))
  with pytest.raises(ValueError, match='CUDA tensor'):      # the checks above come before the queries are touched
    host.search(q, qw, exclude=torch.zeros(3, 32, dtype=torch.int64))
  from mmt_amd.metric import retrieval_metrics_indexed
  args = (torch.zeros(4, 2, 8), torch.zeros(4, 2, 1, 8), torch.zeros(4, 2), torch.zeros(4, 1, 2))
  with pytest.raises(ValueError, match='video_subset'):
    retrieval_metrics_indexed(*args, video_subset=np.ones(5, bool))
  for bad in (np.array([0, 4]), np.array([-1]), np.array([0.5])):
    with pytest.raises(ValueError, match='video_subset'):
      retrieval_metrics_indexed(*args, video_subset=bad)
  with pytest.raises(ValueError, match='video_subset leaves no caption'):
    retrieval_metrics_indexed(*args, query_masks=np.array([[1], [0], [1], [1]]), video_subset=torch.tensor([1]))
  with pytest.raises(ValueError, match='video_subset leaves no caption'):
    retrieval_metrics_indexed(*args, video_subset=np.zeros(4, bool))
