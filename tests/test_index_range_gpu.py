"""VideoIndex.range_search / ShardedVideoIndex.range_search (mmt_search_range_count, mmt_search_range_fill and their bf16
forms): every item scoring at or above a per-query threshold, as a CSR, without the N_query x N_video matrix.

  1. lattice inputs, where fp32, bf16 and fp64 agree bit for bit and ties abound: hits and scores equal the fp64 brute
     force exactly, for thresholds on attained values, between values, at -inf, +inf and NaN;
  2. random inputs: equal to numpy >= on the device's own score matrix (target_scores over every item), bit for bit;
  3. consistent with threshold_counts and with search(k = 10);  4. subsets;  5. max_hits;  6. query batching;
  7. sharded equals monolithic;  8. no buffer that grows with NQ * NV."""
import functools

import numpy as np
import pytest
import torch

from tests.test_index_range_cpu import brute_range
from tests.test_index_ranks_gpu import _dev, _lattice, _random
from tests.test_index_sharded_gpu import _spilling, _whole
from tests.test_search_gpu import _cuda, _ref_sims

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
DTYPES = [torch.float32, torch.bfloat16]
INF, NAN = float('inf'), float('nan')

# (nq, nv, M, d): across the query block (64), the tile (128), 128-column chunks and several of them; the last has 256-item
# chunks, two tiles per block, and a last chunk of 8 items
LATTICE = [(1, 1, 1, 8), (63, 127, 7, 8), (65, 129, 2, 8), (130, 8193, 3, 64), (513, 14600, 1, 8)]
RANDOM = [(1, 1), (63, 127), (65, 129), (130, 4097)]   # (nq, nv) with M = 7, d = 16


def _expect(matrix, thr, allowed=None, order='index'):
  """brute_range row by row -> the CSR (offsets, indices, scores) as numpy arrays."""
  thr = np.broadcast_to(np.asarray(thr, np.float32), matrix.shape[:1])
  rows = [brute_range(matrix[r], thr[r], allowed, order) for r in range(matrix.shape[0])]
  offsets = np.concatenate([[0], np.cumsum([i.size for i, _ in rows])]).astype(np.int64)
  return (offsets, np.concatenate([i for i, _ in rows]).astype(np.int64),
          np.concatenate([s for _, s in rows]).astype(np.float32))


def _assert_result(res, want, what=None):
  offsets, indices, scores = want
  nq, total = offsets.size - 1, int(offsets[-1])
  for x, dtype, shape in ((res.offsets, torch.int64, (nq + 1,)), (res.indices, torch.int64, (total,)),
                          (res.scores, torch.float32, (total,)), (res.counts, torch.int64, (nq,))):
    assert x.dtype == dtype and tuple(x.shape) == shape and x.device == DEV, what
  got_i, got_s = res.indices.cpu().numpy(), res.scores.cpu().numpy()
  print('%s: %d hits, %d wrong items, %d wrong score bits' % (
      what, total, (got_i != indices).sum(), (got_s.view(np.int32) != scores.view(np.int32)).sum()))
  assert np.array_equal(res.offsets.cpu().numpy(), offsets), what
  assert np.array_equal(res.counts.cpu().numpy(), np.diff(offsets)), what
  assert np.array_equal(got_i, indices), what
  assert np.array_equal(got_s.view(np.int32), scores.view(np.int32)), what


def _equal(a, b):
  return (torch.equal(a.offsets, b.offsets) and torch.equal(a.indices, b.indices) and a.scores.shape == b.scores.shape and
          torch.equal(a.scores.view(torch.int32), b.scores.view(torch.int32)) and torch.equal(a.counts, b.counts))


# ---- 1. lattice inputs ------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _lattice_case(case):
  """The lattice of tests/test_index_ranks_gpu.py at T = 1 and its fp64 scores, which are float32 values bit for bit."""
  q, qw, g, gw = _lattice(*LATTICE[case], 1)[:4]
  ref = _ref_sims(q, qw, g, gw)
  ref32 = ref.astype(np.float32)
  assert np.array_equal(ref, ref32)
  ref32.setflags(write=False)
  return q, qw, g, gw, ref32


def _lattice_thresholds(ref):
  """name -> float32 [nq]: on attained values (>= against ties), between two neighbouring values, and the special ones."""
  nq, nv = ref.shape
  rng = np.random.default_rng(nq + nv)
  srt = np.sort(ref, 1)
  at = rng.integers(0, nv, nq)
  attained = srt[np.arange(nq), at].copy()
  attained[::5] = srt[::5, -1]                                # the row's best score: its ties and nothing else
  between = np.empty(nq, np.float32)
  for r in range(nq):
    distinct = np.unique(ref[r])
    j = rng.integers(0, distinct.size)
    between[r] = (distinct[j] + distinct[j - 1]) / 2 if j else distinct[0] - 0.25
    assert not (ref[r] == between[r]).any()
  special = np.float32([-INF, INF, NAN, 0.0, -0.0])[np.arange(nq) % 5]
  return {'attained': attained.astype(np.float32), 'between': between, 'special': special}


@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16'])
@pytest.mark.parametrize('case', range(len(LATTICE)), ids=['x'.join(map(str, s)) for s in LATTICE])
def test_hits_are_exact_on_lattice_inputs(case, dtype):
  from mmt_amd import _lib
  from mmt_amd.search import VideoIndex
  nq, nv, m, d = LATTICE[case]
  q, qw, g, gw, ref = _lattice_case(case)
  if case == len(LATTICE) - 1:
    # 9 query tiles x 58 chunks of 256 items >= 512 blocks: every block walks two tiles and carries its row counters
    # across them, and the last chunk holds 8 items
    assert _lib.lib().mmt_range_workspace_ints(nq, nv) == nq * 58 and nv - 57 * 256 == 8
  if case % 2 and nv > 1:
    # filled in two pieces with room to spare: the unused rows (never written) must not hit, not even at -inf
    index = VideoIndex.empty(nv + 200, m, d, DEV, dtype=dtype)
    index.add(_dev(g[:nv // 3]), _dev(gw[:nv // 3]))
    index.add(_dev(g[nv // 3:]), _dev(gw[nv // 3:]))
    assert index.num_items == nv < index.capacity
  else:
    index = VideoIndex(_dev(g), _dev(gw), dtype=dtype)
  qd, qwd = _dev(q), _dev(qw)
  for name, thr in _lattice_thresholds(ref).items():
    res = index.range_search(qd, qwd, _dev(thr))
    _assert_result(res, _expect(ref, thr), name)
  special = res.counts.cpu().numpy()                           # 'special' is the last: -inf, +inf, NaN, 0.0, -0.0 by row
  assert (special[0::5] == nv).all() and not special[1::5].any() and not special[2::5].any()
  # a Python float is every row's threshold; the rows without query weight score 0 everywhere: one tie of nv items
  _assert_result(index.range_search(qd, qwd, 0.0), _expect(ref, 0.0), 'float 0.0')
  _assert_result(index.range_search(qd, qwd, -0.0, order='score'), _expect(ref, 0.0, order='score'), 'float -0.0 by score')
  if nq > 1:
    assert int(index.range_search(qd, qwd, 0.0).counts[nq // 3]) == nv
  # no queries: offsets [0] and empty outputs
  none = index.range_search(qd[:0], qwd[:0], 0.0)
  assert none.offsets.tolist() == [0] and none.indices.shape == none.scores.shape == none.counts.shape == (0,)
  assert none.indices.dtype == torch.int64 and none.scores.dtype == torch.float32 and none.offsets.device == DEV
  none = index.range_search(qd[:0], qwd[:0], _dev(np.zeros(0, np.float32)), order='score')
  assert none.offsets.tolist() == [0] and none.indices.numel() == 0


# ---- 2. random inputs against the device's own scores ----------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _random_case(nq, nv, dtype):
  """A random index, its queries and its own score matrix: target_scores with every item as a target returns the scan's
  scores.  Per-query thresholds on attained values, row 0 at -inf and row 1 above its best score."""
  from mmt_amd.search import VideoIndex
  q, qw, g, gw = _random(nq, nv, 7, 16, nq + 3 * nv)
  index = VideoIndex(g, gw, dtype=dtype)
  every = torch.arange(nv, device=DEV).repeat(nq, 1)
  matrix = index.target_scores(q, qw, every).cpu().numpy()
  assert matrix.shape == (nq, nv) and not np.isnan(matrix).any()
  rng = np.random.default_rng(nq + nv)
  thr = np.sort(matrix, 1)[np.arange(nq), rng.integers(0, nv, nq)].astype(np.float32)
  thr[0] = -INF
  if nq > 1:
    thr[1] = np.nextafter(matrix[1].max(), np.float32(INF))
  matrix.setflags(write=False)
  thr.setflags(write=False)
  return index, q, qw, matrix, thr


@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16'])
@pytest.mark.parametrize('nq,nv', RANDOM)
def test_hits_equal_numpy_on_the_scores_of_the_scan(nq, nv, dtype):
  index, q, qw, matrix, thr = _random_case(nq, nv, dtype)
  res = index.range_search(q, qw, _dev(thr))
  _assert_result(res, _expect(matrix, thr), 'index order')
  counts = res.counts.cpu().numpy()
  assert counts[0] == nv and res.indices[:nv].tolist() == list(range(nv))     # -inf: every item, ascending
  assert nq == 1 or counts[1] == 0
  _assert_result(index.range_search(q, qw, _dev(thr), order='score'), _expect(matrix, thr, order='score'), 'score order')
  assert _equal(index.range_search(q, qw, _dev(thr)), res)                     # bit-reproducible
  # the text layout of `search`: (B, M, C, d) / (B, C, M) are rows b * C + c
  if nq % 5 == 0:
    q4 = q.reshape(nq // 5, 5, 7, 16).permute(0, 2, 1, 3).contiguous()
    assert _equal(index.range_search(q4, qw.reshape(nq // 5, 5, 7), _dev(thr)), res)


# ---- 3. consistency with what exists ----------------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16'])
@pytest.mark.parametrize('nq,nv', RANDOM)
def test_consistent_with_threshold_counts_and_search(nq, nv, dtype):
  index, q, qw, matrix, thr = _random_case(nq, nv, dtype)
  res = index.range_search(q, qw, _dev(thr))
  greater, equal = index.threshold_counts(q, qw, _dev(thr))
  assert torch.equal(res.counts, greater.long() + equal.long())
  k = min(10, nv)
  top_s, top_i = index.search(q, qw, k=k)
  res = index.range_search(q, qw, top_s[:, -1].contiguous(), order='score')
  assert bool((res.counts >= k).all())
  head = res.offsets[:-1, None] + torch.arange(k, device=DEV)
  assert torch.equal(res.indices[head], top_i)
  assert torch.equal(res.scores[head].view(torch.int32), top_s.contiguous().view(torch.int32))


# ---- 4. subsets -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16'])
def test_subsets_on_random_inputs(dtype):
  """130 x 4097: chunks of one 128-item tile.  The result is that of numpy restricted to the mask."""
  nq, nv = RANDOM[-1]
  index, q, qw, matrix, thr = _random_case(nq, nv, dtype)
  every = np.arange(nv)
  masks = {'random_half': np.random.default_rng(4).random(nv) < 0.5, 'without_tiles_1_to_4': (every < 128) | (every >= 640),
           'one_item': every == 777, 'last_item': every == nv - 1}
  for name, mask in masks.items():
    sub = index.subset(_cuda(mask))
    for order in ('index', 'score'):
      res = index.range_search(q, qw, _dev(thr), subset=sub, order=order)
      _assert_result(res, _expect(matrix, thr, mask, order), (name, order))
    assert int(res.counts[0]) == int(mask.sum())              # the row at -inf: every allowed item
    greater, equal = index.threshold_counts(q, qw, _dev(thr), subset=sub)
    assert torch.equal(res.counts, greater.long() + equal.long())
  ids = index.subset(_cuda(np.flatnonzero(masks['random_half']).astype(np.int64)))     # the same set as item numbers
  _assert_result(index.range_search(q, qw, _dev(thr), subset=ids), _expect(matrix, thr, masks['random_half']), 'ids')


@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16'])
def test_a_subset_that_empties_tiles_and_a_whole_chunk(dtype):
  """513 x 14600, 256-item chunks of two tiles: the mask drops chunk 1 (items 256 .. 511) whole, the second tile of chunk 4
  and the first of chunk 6, and a random half of the rest -- blocks that skip both tiles, either tile, or none."""
  from mmt_amd.search import VideoIndex
  case = len(LATTICE) - 1
  nq, nv, m, d = LATTICE[case]
  q, qw, g, gw, ref = _lattice_case(case)
  every = np.arange(nv)
  mask = np.random.default_rng(9).random(nv) < 0.5
  mask[(every >= 256) & (every < 512)] = False
  mask[(every >= 4 * 256 + 128) & (every < 5 * 256)] = False
  mask[(every >= 6 * 256) & (every < 6 * 256 + 128)] = False
  index = VideoIndex(_dev(g), _dev(gw), dtype=dtype)
  sub = index.subset(_cuda(mask))
  for name, thr in _lattice_thresholds(ref).items():
    _assert_result(index.range_search(_dev(q), _dev(qw), _dev(thr), subset=sub), _expect(ref, thr, mask), name)
  stale = VideoIndex.empty(nv + 1, m, d, DEV, dtype=dtype)
  stale.add(_dev(g), _dev(gw))
  old = stale.subset(_cuda(mask))
  stale.add(_dev(g[:1]), _dev(gw[:1]))
  with pytest.raises(ValueError, match='built for %d items, the index holds %d' % (nv, nv + 1)):
    stale.range_search(_dev(q), _dev(qw), 0.0, subset=old)


# ---- 5. max_hits ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16'])
def test_max_hits_is_held_before_the_outputs_exist(dtype):
  """Every item of every row hits: 130 * 4097 = 532 610 hits, 6.1 MiB of outputs against some 80 KiB of operands and
  workspace.  One hit above the cap is refused with less than the indices alone (8 bytes per hit) ever allocated."""
  nq, nv = RANDOM[-1]
  index, q, qw, matrix, thr = _random_case(nq, nv, dtype)
  total = nq * nv
  torch.cuda.synchronize()
  base = torch.cuda.memory_allocated()
  torch.cuda.reset_peak_memory_stats()
  with pytest.raises(ValueError, match='%d hits exceed max_hits = %d' % (total, total - 1)):
    index.range_search(q, qw, -INF, max_hits=total - 1)
  torch.cuda.synchronize()
  growth = torch.cuda.max_memory_allocated() - base
  print('allocator peak growth of the refused call %.1f KiB, outputs %.1f KiB' % (growth / 1024, total * 12 / 1024))
  assert growth < 8 * total, growth
  res = index.range_search(q, qw, -INF, max_hits=total)      # exactly at the cap
  assert int(res.offsets[-1]) == total and torch.equal(res.indices, torch.arange(nv, device=DEV).repeat(nq))
  assert np.array_equal(res.scores.cpu().numpy().view(np.int32), matrix.reshape(-1).view(np.int32))
  with pytest.raises(ValueError, match='exceed max_hits = 0'):
    index.range_search(q, qw, _dev(thr), max_hits=0)
  assert index.range_search(q, qw, INF, max_hits=0).indices.numel() == 0


# ---- 6. query batching ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16'])
def test_query_batches_do_not_change_the_result(dtype, monkeypatch):
  from mmt_amd import search
  nq, nv = RANDOM[-1]
  index, q, qw, matrix, thr = _random_case(nq, nv, dtype)
  mask = np.arange(nv) % 3 != 1
  sub = index.subset(_cuda(mask))
  whole = {(s, o): index.range_search(q, qw, _dev(thr), subset=sub if s else None, order=o)
           for s in (False, True) for o in ('index', 'score')}
  assert len(index._batches(nq, 1)) == 1
  monkeypatch.setattr(search, '_BATCH_BYTES', 1)
  assert index._batches(nq, 1) == [(0, 64), (64, 128), (128, 130)]
  for (s, o), want in whole.items():
    assert _equal(index.range_search(q, qw, _dev(thr), subset=sub if s else None, order=o), want), (s, o)
  # the cap is held against the total of the whole call, not of a batch
  total = int(whole[(False, 'index')].offsets[-1])
  with pytest.raises(ValueError, match='%d hits exceed' % total):
    index.range_search(q, qw, _dev(thr), max_hits=total - 1)
  assert _equal(index.range_search(q, qw, _dev(thr), max_hits=total), whole[(False, 'index')])


# ---- 7. sharded -------------------------------------------------------------------------------------------------------

def _five_with_an_empty_shard(g, gw, dtype):
  from mmt_amd.search import ShardedVideoIndex
  index = ShardedVideoIndex.empty(1000, g.shape[1], g.shape[2], [DEV] * 5, dtype=dtype)
  assert index.add(g, gw) == (0, 700)                         # one chunk that spills three times; the last shard stays empty
  assert index.shard_sizes == [200, 200, 200, 100, 0]
  return index


@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16'])
@pytest.mark.parametrize('build', [_whole(1), _spilling, _five_with_an_empty_shard], ids=['1', '3_spilling', '5_one_empty'])
def test_sharded_equals_monolithic_bit_for_bit(build, dtype):
  from mmt_amd.search import VideoIndex
  nq, nv, m, d = 65, 700, 3, 8
  q, qw, g, gw = _random(nq, nv, m, d, nq + nv + m + d)
  for twin in (nv // 2, nv - 1):                              # copies of item 0 on other shards: ties across shards
    g[twin], gw[twin] = g[0], gw[0]
  qw[nq // 2] = 0                                             # every score 0: one tie over all shards
  mono = VideoIndex(g, gw, dtype=dtype)
  shard = build(g, gw, dtype)
  assert shard.num_items == nv
  matrix = mono.target_scores(q, qw, torch.arange(nv, device=DEV).repeat(nq, 1))
  thr = matrix.sort(1).values[torch.arange(nq, device=DEV), torch.arange(nq, device=DEV) * 7 % nv].contiguous()
  thr[0], thr[1], thr[2] = -INF, INF, NAN
  thr[3] = matrix[3, 0]                                       # item 0 and its twins on other shards
  every = torch.arange(nv, device=DEV)
  masks = {None: None, 'every_other': every % 2 == 1, 'one_item': every == nv // 2}
  if len(shard.shards) > 1:
    masks['without_shard_0'] = shard._shard_of[:nv] != 0     # a shard without an allowed item
  for name, mask in masks.items():
    sub_m, sub_s = (None, None) if mask is None else (mono.subset(mask), shard.subset(mask))
    for order in ('index', 'score'):
      for t in (thr, 0.0):
        want = mono.range_search(q, qw, t, subset=sub_m, order=order)
        got = shard.range_search(q, qw, t, subset=sub_s, order=order)
        assert got.indices.device == got.scores.device == got.offsets.device == DEV
        assert _equal(got, want), (name, order)
  total = int(mono.range_search(q, qw, thr).offsets[-1])
  with pytest.raises(ValueError, match='%d hits exceed max_hits = %d' % (total, total - 1)):
    shard.range_search(q, qw, thr, max_hits=total - 1)       # the cap is held against the sum over the shards
  assert _equal(shard.range_search(q, qw, thr, max_hits=total), mono.range_search(q, qw, thr))
  none = shard.range_search(q[:0], qw[:0], 0.0)
  assert none.offsets.tolist() == [0] and none.indices.numel() == 0 and none.scores.dtype == torch.float32
  assert shard.range_search(q, qw, INF).indices.numel() == 0
  old = shard.subset(every % 2 == 1)
  if shard.num_items < shard.capacity:
    shard.add(g[:1], gw[:1])
    with pytest.raises(ValueError, match='built for %d items' % nv):
      shard.range_search(q, qw, 0.0, subset=old)


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason='needs two GPUs')
@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16'])
def test_two_devices_equal_one(dtype):
  from mmt_amd.search import ShardedVideoIndex, VideoIndex
  nq, nv, m, d = 65, 700, 3, 8
  q, qw, g, gw = _random(nq, nv, m, d, nq + nv + m + d)
  g[nv - 1], gw[nv - 1] = g[0], gw[0]
  mono = VideoIndex(g, gw, dtype=dtype)
  index = ShardedVideoIndex.empty(700, m, d, ['cuda:0', 'cuda:1'], dtype=dtype)
  for a, b in ((0, 300), (300, 429), (429, 700)):
    index.add(g[a:b], gw[a:b])
  thr = mono.search(q, qw, k=20)[0][:, -1].contiguous()
  mask = torch.arange(nv, device=DEV) % 2 == 1
  for sub_m, sub_s in ((None, None), (mono.subset(mask), index.subset(mask))):
    for order in ('index', 'score'):
      got = index.range_search(q, qw, thr, subset=sub_s, order=order)
      assert got.indices.device == DEV and _equal(got, mono.range_search(q, qw, thr, subset=sub_m, order=order))
  with pytest.raises(ValueError, match='must be on the index device'):
    index.range_search(q, qw, thr.to(torch.device('cuda', 1)))


# ---- 8. memory --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16'])
def test_range_search_allocates_no_quadratic_buffer(dtype):
  """256 x 65 536, M = 1, d = 8, about 4 hits per row.  What the call may hold at its peak: the outputs (12 bytes per hit,
  offsets, counts), the per-row totals of the count pass, the thresholds, one batch's folded queries (32 bytes per row in
  either dtype) and its workspace (mmt_range_workspace_ints int32), plus the allocator's rounding of each of these (at
  most 512 bytes for each of fewer than 16 tensors): some 150 KiB, where the score matrix would be 64 MiB."""
  from mmt_amd import _lib
  from mmt_amd.search import VideoIndex
  nq, nv, m, d = 256, 65536, 1, 8
  gen = torch.Generator(device=DEV).manual_seed(8)
  index = VideoIndex(torch.rand(nv, m, d, device=DEV, generator=gen) - 0.5, torch.rand(nv, m, device=DEV, generator=gen) + 0.5,
                     dtype=dtype)
  q = torch.rand(nq, m, d, device=DEV, generator=gen) - 0.5
  qw = torch.rand(nq, m, device=DEV, generator=gen) + 0.5
  thr = index.search(q, qw, k=4)[0][:, -1].contiguous()
  assert len(index._batches(nq, 1)) == 1
  torch.cuda.synchronize()
  base = torch.cuda.memory_allocated()
  torch.cuda.reset_peak_memory_stats()
  res = index.range_search(q, qw, thr)
  torch.cuda.synchronize()
  growth = torch.cuda.max_memory_allocated() - base
  total = int(res.offsets[-1])
  bound = (12 * total + 8 * (nq + 1) + 8 * nq) + 8 * nq + 4 * nq + 32 * nq + 4 * _lib.lib().mmt_range_workspace_ints(nq, nv) + 16 * 512
  print('hits %d, allocator peak growth %.1f KiB, bound %.1f KiB, matrix %.1f KiB' % (
      total, growth / 1024, bound / 1024, nq * nv * 4 / 1024))
  assert 4 * nq <= total < 8 * nq
  assert growth <= bound < nq * nv * 4 // 256, (growth, bound)
  top_s, top_i = index.search(q, qw, k=4)
  by_score = index.range_search(q, qw, thr, order='score')
  head = by_score.offsets[:-1, None] + torch.arange(4, device=DEV)
  assert torch.equal(by_score.indices[head], top_i)
