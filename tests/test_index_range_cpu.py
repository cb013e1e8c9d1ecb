"""The host side of VideoIndex.range_search (mmt_range_workspace_ints, mmt_search_range_count, mmt_search_range_fill and
their bf16 forms) without a GPU: the brute-force restatement the GPU tests hold the kernels to, the two-pass offsets
arithmetic restated in numpy, the header and the ctypes table, the argument gates and the argument errors of the call."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ('mmt_range_workspace_ints',)  # the two passes: tests/test_search_abi_cpu.py
TILE, ROWS = 128, 64  # gallery columns per score tile, query rows per block


def brute_range(scores_row, thr, allowed=None, order='index'):
  """The hits of one query: (item numbers int64, their scores with their own bits) of the items with score >= thr (a plain
  compare: NaN hits nothing, -inf everything) among the `allowed` ones (bool [NV], None = all).  order='index': ascending
  item; order='score': descending score, -0.0 tied with +0.0, equal scores by ascending item."""
  scores_row = np.asarray(scores_row)
  hit = scores_row >= thr
  if allowed is not None:
    hit &= np.asarray(allowed, bool)
  items = np.flatnonzero(hit).astype(np.int64)
  if order == 'score':
    items = items[np.lexsort((items, -(scores_row[items].astype(np.float64) + 0.0)))]
  else:
    assert order == 'index'
  return items, scores_row[items]


def two_pass_positions(hit, chunk):
  """The arithmetic of the two passes, restated: hit bool [NQ, NV] -> (offsets int64 [NQ + 1], pos int64 [NQ, NV], the slot
  of every hit, -1 elsewhere).  Count pass: hits per (query, chunk).  Offsets: per row the exclusive prefix of the chunk
  counts, and the exclusive prefix of the row totals.  Fill pass, per (row, chunk): walking the chunk's 128-column tiles, a
  hit at lane l of 64-column half h goes to offsets[q] + prefix[q][chunk] + (hits of the row in the chunk's earlier tiles)
  + (hits in lower columns of the tile) = popcount of the half's ballot below l, plus the first half's popcount for h = 1.
  Positions are clamped against the row's next chunk, as in the kernel."""
  nq, nv = hit.shape
  n_chunks = -(-nv // chunk)
  counts = np.zeros((nq, n_chunks), np.int64)
  for c in range(n_chunks):
    counts[:, c] = hit[:, c * chunk:(c + 1) * chunk].sum(1)
  prefix = np.cumsum(counts, 1) - counts
  offsets = np.concatenate([[0], np.cumsum(counts.sum(1))]).astype(np.int64)
  pos = np.full((nq, nv), -1, np.int64)
  for q in range(nq):
    for c in range(n_chunks):
      base = offsets[q] + prefix[q, c]
      cap = (offsets[q] + prefix[q, c + 1] if c + 1 < n_chunks else offsets[q + 1]) - base
      seen = 0
      for g0 in range(c * chunk, min(nv, (c + 1) * chunk), TILE):
        halves = [np.zeros(64, bool), np.zeros(64, bool)]
        for h in range(2):
          live = hit[q, g0 + 64 * h:min(nv, g0 + 64 * h + 64, (c + 1) * chunk)]
          halves[h][:live.size] = live
        n0 = int(halves[0].sum())
        for h in range(2):
          for lane in np.flatnonzero(halves[h]):
            p = seen + h * n0 + int(halves[h][:lane].sum())
            if p < cap:
              pos[q, g0 + 64 * h + lane] = base + p
        seen += n0 + int(halves[1].sum())
  return offsets, pos


def test_brute_range_on_hand_made_rows():
  row = np.float32([0.5, -0.0, 0.25, 0.0, 0.5, -1.0, 0.0])
  items, scores = brute_range(row, 0.0)
  assert items.tolist() == [0, 1, 2, 3, 4, 6] and items.dtype == np.int64       # -0.0 >= 0.0
  assert np.array_equal(scores.view(np.int32), row[items].view(np.int32))
  items, scores = brute_range(row, 0.0, order='score')
  assert items.tolist() == [0, 4, 2, 1, 3, 6]                                    # the zeros are one tie, in item order
  assert np.signbit(scores).tolist() == [False, False, False, True, False, False]   # ... and each keeps its own sign
  assert brute_range(row, 0.5)[0].tolist() == [0, 4]                             # a threshold on an attained value
  assert brute_range(row, np.float32(0.5000001))[0].size == 0
  assert brute_range(row, np.float32('nan'))[0].size == 0
  assert brute_range(row, np.float32('inf'))[0].size == 0
  assert brute_range(row, -np.inf)[0].tolist() == list(range(7))
  allowed = np.array([0, 1, 1, 0, 1, 1, 0], bool)
  assert brute_range(row, 0.0, allowed)[0].tolist() == [1, 2, 4]
  assert brute_range(row, -np.inf, allowed, 'score')[0].tolist() == [4, 2, 1, 5]


@pytest.mark.parametrize('nq,nv,chunk,density', [(3, 1, 128, 1.0), (5, 127, 128, 0.3), (7, 300, 128, 0.5), (4, 1000, 256, 0.05),
                                                 (6, 1160, 256, 0.9), (2, 4097, 4096, 0.01)])
def test_two_pass_offsets_arithmetic_reproduces_ascending_order(nq, nv, chunk, density):
  """Random hit masks with empty chunks, an empty row, a full row and a ragged last tile (nv is no multiple of 128; 1160 =
  4 chunks of 256 and one of 136: a whole tile and 8 columns): the slots are exactly 0 .. total - 1, each taken once, and
  reading them in slot order gives every row by ascending item."""
  rng = np.random.default_rng(nq * 1000 + nv)
  hit = rng.random((nq, nv)) < density
  hit[0] = False                                    # a row without a hit
  hit[nq - 1] = True                                # a row that hits everything
  if nv > chunk:
    hit[1, chunk:2 * chunk] = False                 # an empty chunk in the middle of a row
    hit[1, nv - 1] = True                           # ... whose last (ragged) tile has a hit
  offsets, pos = two_pass_positions(hit, chunk)
  total = int(hit.sum())
  assert offsets[-1] == total and np.array_equal(np.diff(offsets), hit.sum(1))
  assert np.array_equal(pos >= 0, hit)
  assert np.array_equal(np.sort(pos[hit]), np.arange(total))
  items = np.empty(total, np.int64)
  rows = np.empty(total, np.int64)
  qs, gs = np.nonzero(hit)
  items[pos[qs, gs]], rows[pos[qs, gs]] = gs, qs
  for q in range(nq):
    mine = slice(offsets[q], offsets[q + 1])
    assert (rows[mine] == q).all() and np.array_equal(items[mine], np.flatnonzero(hit[q]))


def test_signatures_of_the_new_exports_agree_with_the_header():
  from mmt_amd import _lib
  src = open(os.path.join(ROOT, 'include', 'mmt_hip.h')).read()
  handle = ctypes.CDLL(_lib.LIB_PATH)
  arity = {'mmt_range_workspace_ints': 2}
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
  for name in NEW_EXPORTS + ('mmt_count_workspace_ints',):
    fns[name] = getattr(handle, name)
    fns[name].restype, fns[name].argtypes = _lib.SIGNATURES[name]
  size = fns['mmt_range_workspace_ints']
  assert size(64, 4096 * 512) == 64 * 512                            # full-size chunks
  assert size(63, 127) == 63                                         # one tile
  assert size(257, 4097) == 257 * 33                                 # 128-column chunks while the chip is not full
  assert size(513, 14600) == 513 * 58                                # 256-column chunks: 9 query tiles x 58 >= 512 blocks
  for shape in ((64, 4096 * 512), (257, 4097), (513, 14600), (1, 1)):   # the chunk rule of the count kernels, one slot each
    assert 2 * size(*shape) == fns['mmt_count_workspace_ints'](*shape, 1)
  for bad in ((0, 5), (5, 0), (-1, 5)):
    assert size(*bad) == -1


def _hollow_index(num_items, dtype=torch.float32):
  """A VideoIndex with its bookkeeping and no storage: the argument checks come before anything reads it."""
  from mmt_amd.search import VideoIndex
  index = VideoIndex.__new__(VideoIndex)
  index.capacity, index.num_experts, index.dim, index.num_items = 8, 2, 8, num_items
  index.device, index.dtype = torch.device('cuda', 0), dtype
  return index


def test_argument_errors_are_raised_without_a_device():
  from mmt_amd.search import IndexSubset, ShardedVideoIndex, VideoIndex
  q, qw = torch.zeros(3, 2, 8), torch.zeros(3, 2)
  with pytest.raises(ValueError, match='holds no items'):
    _hollow_index(0).range_search(q, qw, 0.5)
  index = _hollow_index(5)
  with pytest.raises(ValueError, match="order must be 'index' or 'score'"):
    index.range_search(q, qw, 0.5, order='rank')
  for bad in (-1, 2.0, True, None):
    with pytest.raises(ValueError, match='max_hits'):
      index.range_search(q, qw, 0.5, max_hits=bad)
  for bad in ('0.5', None, True, [0.5] * 3, np.float32([0.5] * 3)):
    with pytest.raises(ValueError, match='threshold must be a float or a float32 tensor'):
      index.range_search(q, qw, bad)
  with pytest.raises(ValueError, match='float32 tensor'):
    index.range_search(q, qw, torch.zeros(3, dtype=torch.float64))
  with pytest.raises(ValueError, match='index device'):
    index.range_search(q, qw, torch.zeros(3))                 # host thresholds for a device index
  with pytest.raises(ValueError, match='subset must come from VideoIndex.subset'):
    index.range_search(q, qw, 0.5, subset=torch.ones(5, dtype=torch.bool))
  stale = IndexSubset.__new__(IndexSubset)
  stale.num_items, stale.device = 4, index.device
  with pytest.raises(ValueError, match='built for 4 items, the index holds 5'):
    index.range_search(q, qw, 0.5, subset=stale)
  with pytest.raises(ValueError, match='CUDA tensor'):
    index.range_search(q, qw, 0.5)                            # the queries themselves are host tensors
  index.device = torch.device('cpu')                          # lets the shape checks be reached with host tensors
  for bad in (torch.zeros(()), torch.zeros(3, 1)):
    with pytest.raises(ValueError, match=r'threshold \[NQ\] expected'):
      index.range_search(q, qw, bad)
  # neither normalisation nor exclusions are part of the call
  for extra in ('norm', 'exclude', 'dynamic'):
    with pytest.raises(TypeError):
      index.range_search(q, qw, 0.5, **{extra: None})
  # the sharded index has the same surface and the same checks
  import inspect
  assert (inspect.signature(ShardedVideoIndex.range_search).parameters.keys() ==
          inspect.signature(VideoIndex.range_search).parameters.keys())
  assert inspect.signature(VideoIndex.range_search).parameters['max_hits'].default == 1 << 27
  sharded = ShardedVideoIndex.__new__(ShardedVideoIndex)
  sharded.num_items, sharded.num_experts, sharded.dim, sharded.device = 0, 2, 8, torch.device('cuda', 0)
  with pytest.raises(ValueError, match='holds no items'):
    sharded.range_search(q, qw, 0.5)
  sharded.num_items = 5
  with pytest.raises(ValueError, match='order'):
    sharded.range_search(q, qw, 0.5, order='rank')
  with pytest.raises(ValueError, match='subset must come from ShardedVideoIndex.subset'):
    sharded.range_search(q, qw, 0.5, subset=stale)


def test_csr_helpers_order_rows_as_search_does():
  """order='score' is host composition over the CSR: restated by brute_range on a hand-made CSR with ties and both zeros."""
  from mmt_amd.search import _csr_rows, _range_result
  rows = [np.float32([0.5, -0.0, 0.25, 0.0, 0.5, -1.0, 0.0]), np.float32([]), np.float32([1.0, 2.0, 2.0, -0.0, 0.0])]
  items = [np.int64([3, 4, 9, 10, 11, 40, 41]), np.int64([]), np.int64([0, 5, 6, 7, 8])]
  offsets = torch.tensor([0, 7, 7, 12])
  assert _csr_rows(offsets).tolist() == [0] * 7 + [2] * 5
  idx, sc = torch.from_numpy(np.concatenate(items)), torch.from_numpy(np.concatenate(rows))
  same = _range_result(offsets, idx, sc, 'index')
  assert same.indices is idx and same.scores is sc and same.counts.tolist() == [7, 0, 5]
  res = _range_result(offsets, idx, sc, 'score')
  assert torch.equal(res.offsets, offsets)
  for r in range(3):
    lo, hi = int(offsets[r]), int(offsets[r + 1])
    want_pos, want_s = brute_range(rows[r], -np.inf, order='score')
    assert res.indices[lo:hi].tolist() == items[r][want_pos].tolist()
    assert np.array_equal(res.scores[lo:hi].numpy().view(np.int32), want_s.view(np.int32))
