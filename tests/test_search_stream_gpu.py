"""index.schedule = 'stream': the streaming schedule of `search`'s plain top-k scan (mmt_search_topk_stream).

THE CONTRACT is bit identity with the tile schedule: every case here makes the same call twice on the same index, with its
schedule set to 'stream' and as it was made, and compares the indices with torch.equal and the scores as int32 -- at every edge of the
new kernel's geometry (its 32-row query tile, its 128-item wave tile, its 512-item sweep and chunk, a slab of K that is
partial or whole), for the three storages, with subset, exclusions and cursor, on one index and on shards.  One shape per
storage is also held against fp64 of the definition, within the 1e-5 of the sweeps of tests/test_search_gpu.py,
tests/test_search_bf16_gpu.py and tests/test_search_fp8_gpu.py: two schedules that agree could still agree on a wrong
value.  Every test fails on a build without the schedule: there an index has no such property, assigning it sets a plain
attribute that nothing reads, and the first thing every test here does is to check what the property does with a value
it must refuse."""
import contextlib
import functools

import numpy as np
import pytest
import torch

from tests.test_search_bf16_cpu import sweep_data
from tests.test_search_gpu import _assert_topk, _cuda, _ref_sims

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
DTYPES = {'fp32': torch.float32, 'bf16': torch.bfloat16, 'fp8': torch.float8_e4m3fn}
# (M, d): K = M * d off and on the slab (32 fp32 values, 64 bf16 values or fp8 codes), below one slab and above
SHAPES = {'fp32': [(1, 4), (3, 12), (7, 40)], 'bf16': [(1, 8), (3, 24), (2, 64), (5, 104)],
          'fp8': [(1, 16), (3, 48), (16, 16)]}
NQS = [1, 2, 31, 32, 33, 65]
STORES = list(DTYPES)


def _data(nq, nv, m, d, seed):
  """Random positive weights, some experts zeroed per item and per query, one query row (where there are two) and one item
  (where there are three) without any weight -- the 1e-5 denominator -- and every tenth item an exact copy of another, so
  that equal scores have to come out by ascending index."""
  rng = np.random.default_rng([seed, nq, nv, m, d])
  q = ((rng.random((nq, m, d), dtype=np.float32) * 2 - 1) / np.float32(np.sqrt(d)))
  g = ((rng.random((nv, m, d), dtype=np.float32) * 2 - 1) / np.float32(np.sqrt(d)))
  qw = rng.uniform(0.1, 1, (nq, m)).astype(np.float32)
  gw = rng.uniform(0.1, 1, (nv, m)).astype(np.float32)
  if m > 1:
    qw[rng.random((nq, m)) < 0.2] = 0
    gw[rng.random((nv, m)) < 0.2] = 0
  if nq >= 2:
    qw[nq // 2] = 0
  if nv >= 3:
    gw[nv // 3] = 0
  dup = np.arange(9, nv, 10)                                     # ascending: a copy of a copy is still a copy
  g[dup], gw[dup] = g[dup - 7], gw[dup - 7]
  return _cuda(q), _cuda(qw), _cuda(g), _cuda(gw)


def _index(store, g, gw):
  from mmt_amd.search import VideoIndex
  return VideoIndex(g, gw, dtype=DTYPES[store])


def _same(a, b):
  return len(a) == len(b) and all(
      x.dtype == y.dtype and x.shape == y.shape and
      torch.equal(x.view(torch.int32) if x.dtype is torch.float32 else x, y.view(torch.int32) if y.dtype is torch.float32 else y)
      for x, y in zip(a, b))


@contextlib.contextmanager
def _scheduled(index, schedule):
  """The index with that schedule, and afterwards with the one it had (the option tests share their indexes)."""
  with pytest.raises(ValueError, match='schedule must be'):   # a build without the property would take anything
    index.schedule = 'no such schedule'
  before = index.schedule
  index.schedule = schedule
  assert index.schedule == schedule
  try:
    yield index
  finally:
    index.schedule = before


def _both(index, q, qw, **args):
  """The call with the streaming schedule and without; asserts the contract and returns the (tile) result."""
  assert index.schedule is None
  tile = index.search(q, qw, **args)
  with _scheduled(index, 'tile'):
    assert _same(index.search(q, qw, **args), tile)
  with _scheduled(index, 'stream'):
    stream = index.search(q, qw, **args)
  bad = int((stream[1] != tile[1]).sum()), int((stream[0].view(torch.int32) != tile[0].view(torch.int32)).sum())
  print('%s k=%d: %d index, %d score-bit mismatches of %d' % (sorted(set(args) - {'k'}), args['k'], bad[0], bad[1],
                                                              tile[1].numel()))
  assert _same(stream, tile), (bad, args.keys())
  return tile


def _first_nv_with(nq, chunks):
  """The smallest NV whose workspace has `chunks` chunk lists per query, by bisection (the count is monotone in NV)."""
  from mmt_amd import _lib
  keys = _lib.lib().mmt_topk_stream_workspace_keys
  lo, hi = 1, 1 << 22
  assert keys(nq, lo, 1) // nq < chunks <= keys(nq, hi, 1) // nq
  while hi - lo > 1:
    mid = (lo + hi) // 2
    lo, hi = (lo, mid) if keys(nq, mid, 1) // nq >= chunks else (mid, hi)
  return hi


@pytest.mark.parametrize('store', STORES)
def test_plain_search_at_every_gallery_size(store):
  """NV at the edges of the wave tile, the sweep and the chunk rule -- the sizes where the workspace function first reports
  two and three chunks for the NQ in use, and one item either side -- each with another NQ and another K, and k = 1, 10,
  128 and a k above NV."""
  n = 0
  for nq in (1, 33):
    edges = [_first_nv_with(nq, c) + o for c in (2, 3) for o in (-1, 0, 1)]
    for nv in sorted(set(([1, 31, 32, 33, 127, 129, 513, 1000] if nq == 1 else []) + edges)):
      m, d = SHAPES[store][n % len(SHAPES[store])]
      nq_here = nq if nv in edges else NQS[n % len(NQS)]   # the edges were found for this NQ
      n += 1
      q, qw, g, gw = _data(nq_here, nv, m, d, 1)
      index = _index(store, g, gw)
      for k in (1, 10, 128, min(128, nv + 5)):
        s, i = _both(index, q, qw, k=k)
        assert s.shape == (nq_here, min(k, nv))


@pytest.mark.parametrize('store', STORES)
def test_every_query_count_and_every_row_width(store):
  for nq in NQS:
    for m, d in SHAPES[store]:
      q, qw, g, gw = _data(nq, 1000, m, d, 2)
      _both(_index(store, g, gw), q, qw, k=10)


# Blocks that take SEVERAL sweeps: a chunk is more than one 512-item sweep only when there are more sweeps than
# max(512 / ceil(NQ / 32), ceil(sweeps / 8)) -- beyond 262 144 items for up to 32 queries, beyond 87 040 for 65.  Then the
# query buffers, the thresholds and the candidate lists are carried from one sweep to the next, tk_push compacts across
# sweeps, chunks are uneven (some one sweep, some two), and a subset can empty a whole sweep in the middle of a chunk, or
# a whole chunk.  (NQ, NV): one query just past the threshold (514 and 515 sweeps in 512 chunks), 65 queries past theirs
# (172 sweeps in 170 chunks), and 513 queries over 62 140 items: 122 sweeps in 30 chunks, four or five sweeps a block.
DEEP = [(1, 512 * 512 + 513), (1, 512 * 512 + 1025), (65, 512 * 170 + 513), (513, 62140)]


def _chunks(nq, nv):
  """The chunks of the streaming scan as ranges of sweeps: the rule of the workspace function, restated."""
  from mmt_amd import _lib
  n = _lib.lib().mmt_topk_stream_workspace_keys(nq, nv, 1) // nq
  sweeps = -(-nv // 512)
  assert n == min(sweeps, max(512 // -(-nq // 32), -(-sweeps // 8)))
  return [(c * sweeps // n, (c + 1) * sweeps // n) for c in range(n)]


@pytest.mark.parametrize('nq,nv', DEEP, ids=['%dx%d' % s for s in DEEP])
@pytest.mark.parametrize('store', STORES)
def test_blocks_of_several_sweeps(store, nq, nv):
  m, d = SHAPES[store][0]
  q, qw, g, gw = _data(nq, nv, m, d, 8)
  index = _index(store, g, gw)
  chunks = _chunks(nq, nv)
  deep = [c for c, (lo, hi) in enumerate(chunks) if hi - lo >= 2]
  assert deep and len({hi - lo for lo, hi in chunks}) >= 2       # several sweeps somewhere, and uneven chunks
  for k in (1, 10, 128):
    page = _both(index, q, qw, k=k)
  # a subset that empties a sweep in the middle (or at the head) of a multi-sweep chunk, the whole of another such chunk
  # where there is one, and all of the gallery's first chunk where that is a single sweep; dense elsewhere
  allowed = torch.rand(nv, device=DEV, generator=torch.Generator(device=DEV).manual_seed(9)) < 0.6
  lo, hi = chunks[deep[0]]
  hole = lo + 1 if hi - lo >= 3 else lo
  allowed[512 * hole:512 * (hole + 1)] = False
  lo, hi = chunks[deep[-1]]
  if len(deep) > 1:
    allowed[512 * lo:512 * hi] = False
  if 0 not in deep:
    allowed[512 * chunks[0][0]:512 * chunks[0][1]] = False
  sub = index.subset(allowed)
  for k in (10, 128):
    _both(index, q, qw, k=k, subset=sub)
  # everything at once, the cursor in the middle of the k = 128 list, the exclusions right behind it
  ex = page[1][:, 40:72:4].contiguous()
  after = (page[0][:, 30].contiguous(), page[1][:, 30].contiguous())
  _both(index, q, qw, k=10, exclude=ex, after=after)
  _both(index, q, qw, k=128, subset=sub, exclude=ex, after=after)
  # a sparse subset: a handful of items, most sweeps and most chunks empty
  few = torch.tensor([0, 511, 512 * (hole + 1), 512 * chunks[deep[-1]][0] + 7, nv - 1], device=DEV)
  _both(index, q, qw, k=10, subset=index.subset(few))


@functools.lru_cache(maxsize=None)
def _case(store):
  """One gallery of three chunks and eleven 128-item tiles, 33 queries: shared by the option tests."""
  m, d = SHAPES[store][1]
  q, qw, g, gw = _data(33, 1300, m, d, 3)
  return q, qw, _index(store, g, gw)


def _subsets(index):
  nv = index.num_items
  gen = torch.Generator(device=DEV).manual_seed(5)
  # sparse: the tiles at 128 .. 639 and 768 .. 1151 hold no allowed item, and the sweep at 512 .. 1023 only one
  sparse = torch.tensor([3, 9, 2, 127, 640, 700, 1152, 1299], device=DEV)
  dense = torch.rand(nv, device=DEV, generator=gen) < 0.7
  return {'sparse': index.subset(sparse), 'dense': index.subset(dense)}


@pytest.mark.parametrize('store', STORES)
def test_subsets(store):
  q, qw, index = _case(store)
  for name, sub in _subsets(index).items():
    for k in (1, 10, 128):
      s, i = _both(index, q, qw, k=k, subset=sub)
      assert s.shape == (33, min(k, sub.count)), name


@pytest.mark.parametrize('store', STORES)
def test_exclusions(store):
  q, qw, index = _case(store)
  top = index.search(q, qw, k=32)[1]
  for e in (1, 32):
    ex = top[:, :e].clone()
    ex[::3, -1] = -1                                             # none
    s, i = _both(index, q, qw, k=10, exclude=ex)
    assert not (i[:, :, None] == ex[:, None, :]).any()
  _both(index, q, qw, k=128, exclude=top)


@pytest.mark.parametrize('store', STORES)
def test_pages_two_and_three(store):
  q, qw, index = _case(store)
  page = _both(index, q, qw, k=10)
  whole = index.search(q, qw, k=30)
  for n in (1, 2):
    page = _both(index, q, qw, k=10, after=(page[0][:, -1].contiguous(), page[1][:, -1].contiguous()))
    assert _same(page, tuple(t[:, 10 * n:10 * n + 10] for t in whole))
  # a row without a cursor, an exhausted one
  a_s, a_i = page[0][:, -1].clone(), page[1][:, -1].clone()
  a_s[0], a_i[0], a_s[1], a_i[1] = float('inf'), -1, float('-inf'), -1
  s, i = _both(index, q, qw, k=10, after=(a_s, a_i))
  assert (i[1] == -1).all() and _same((s[0], i[0]), (whole[0][0, :10], whole[1][0, :10]))


@pytest.mark.parametrize('store', STORES)
def test_subset_exclusions_and_cursor_together(store):
  q, qw, index = _case(store)
  sub = _subsets(index)['dense']
  first = index.search(q, qw, k=40, subset=sub)
  ex = first[1][:, 12:44:2][:, :8].contiguous()                  # bars part of the next page
  after = (first[0][:, 9].contiguous(), first[1][:, 9].contiguous())
  for k in (10, 128):
    _both(index, q, qw, k=k, subset=sub, exclude=ex, after=after)


def test_search_refined_takes_the_coarse_index_schedule():
  m, d = 3, 48
  q, qw, g, gw = _data(5, 1300, m, d, 4)
  coarse = _index('fp8', g, gw)
  for store in ('fp32', 'bf16'):
    fine = _index(store, g, gw)
    sub = coarse.subset(torch.arange(1300, device=DEV) % 3 != 1)
    for args in ({}, {'subset': sub, 'exclude': torch.arange(5, device=DEV) * 3}):
      want = fine.search_refined(q, qw, coarse, k=10, shortlist=64, **args)
      for schedule in ('stream', 'tile'):
        with _scheduled(coarse, schedule):
          assert _same(fine.search_refined(q, qw, coarse, k=10, shortlist=64, **args), want), schedule


@pytest.mark.parametrize('store', STORES)
def test_a_row_searched_alone_is_its_row_of_the_batch(store):
  q, qw, index = _case(store)
  with _scheduled(index, 'stream'):
    batch = index.search(q, qw, k=10)
    for r in (0, 16, 31, 32):
      alone = index.search(q[r:r + 1], qw[r:r + 1], k=10)
      assert _same(alone, tuple(t[r:r + 1] for t in batch)), r


@pytest.mark.parametrize('store', STORES)
def test_three_shards_one_of_them_empty_equal_one_index(store):
  from mmt_amd.search import ShardedVideoIndex
  m, d = SHAPES[store][1]
  q, qw, g, gw = _data(33, 1300, m, d, 3)
  one = _case(store)[2]
  three = ShardedVideoIndex.empty(2400, m, d, [DEV] * 3, dtype=DTYPES[store])
  three.add(g, gw)
  assert three.shard_sizes == [800, 500, 0]
  mask = torch.rand(1300, device=DEV, generator=torch.Generator(device=DEV).manual_seed(6)) < 0.5
  top = one.search(q, qw, k=4)[1]
  for k in (1, 10, 128):
    want = one.search(q, qw, k=k)
    assert _same(_both(three, q, qw, k=k), want), k
  after = (want[0][:, 5].contiguous(), want[1][:, 5].contiguous())
  want = one.search(q, qw, k=10, subset=one.subset(mask), exclude=top, after=after)
  assert _same(_both(three, q, qw, k=10, subset=three.subset(mask), exclude=top, after=after), want)


@functools.lru_cache(maxsize=None)
def _anchor_data():
  return sweep_data(33, 1300, 3, 48, 10)   # read by every storage's test, written by none


@pytest.mark.parametrize('store', STORES)
def test_streamed_scores_against_fp64_of_the_definition(store):
  """The independent anchor: fp64 of the storage's own definition (the dequantised stored rows as the gallery, the gate
  weights in the denominator only), as the sweeps of the three storages hold the tile schedule to it."""
  q, qw, g, gw = _anchor_data()
  nq, nv, m, d, k = 33, 1300, 3, 48, 10
  idx = _index(store, _cuda(g), _cuda(gw))
  with _scheduled(idx, 'stream'):
    s, i = idx.search(_cuda(q), _cuda(qw), k=k)
  if store == 'fp32':
    ref = _ref_sims(q, qw, g, gw)
  else:
    deq = idx.folded[:nv].cpu().float()
    if store == 'fp8':
      deq = deq * idx.scales[:nv].cpu()[:, None]
    one = np.ones((nv, m))
    den1 = np.asarray(qw, np.float64) @ one.T
    den1[den1 == 0] = 1e-5
    den = np.asarray(qw, np.float64) @ np.asarray(gw, np.float64).T
    den[den == 0] = 1e-5
    ref = _ref_sims(q, qw, deq.numpy().reshape(nv, m, d), one) * den1 / den
  got = np.take_along_axis(ref, i.cpu().numpy(), 1)
  print('%s: max |score - fp64| on the returned items = %.3g' % (store, np.abs(s.cpu().numpy() - got).max()))
  _assert_topk(ref, i.cpu().numpy(), s.cpu().numpy(), k, 1e-5, 1e-5)
  assert np.array_equal(i[nq // 2].cpu().numpy(), np.arange(k))   # the query without weights: every score 0, by index


def test_refusals_come_before_anything_is_scored(monkeypatch):
  from mmt_amd import search
  from mmt_amd.search import ShardedVideoIndex
  q, qw, g, gw = _data(4, 256, 2, 8, 7)
  one = _index('fp32', g, gw)
  three = ShardedVideoIndex(g[:252], gw[:252], [DEV] * 3)   # 84 items a shard: whole sets of two
  cases = []
  for index in (one, three):
    norm = index.hub_norm(q, qw, 20.0)
    dyn = index.hub_norm(q, qw, 20.0, dynamic=True)
    cases += [(index, dict(norm=norm), 'norm='), (index, dict(norm=dyn, dynamic=True), 'norm='),
              (index, dict(dynamic=False), 'dynamic='), (index, dict(pooling=index.pooling(2, 2)), 'pooling='),
              (index, dict(item_pooling=index.item_pooling(2)), 'item_pooling=')]
  fp8 = _index('fp8', torch.cat([g, g], 2), gw)
  # nothing is prepared, launched or allocated from here on
  monkeypatch.setattr(search._lib, 'lib', lambda: pytest.fail('a launch was prepared'))
  monkeypatch.setattr(search, '_lists', lambda *a, **kw: pytest.fail('an output was allocated'))
  monkeypatch.setattr(search, '_fold', lambda *a, **kw: pytest.fail('the queries were folded'))
  for index, args, name in cases:
    with _scheduled(index, 'stream'):
      with pytest.raises(ValueError, match="schedule 'stream' does not combine with %s" % name):
        index.search(q, qw, k=3, **args)
  for index in (one, three, fp8):
    assert index.schedule is None
    for bad in ('streaming', 'Stream', '', 0, True, b'stream', ['stream']):
      with pytest.raises(ValueError, match='schedule must be'):
        index.schedule = bad
      assert index.schedule is None                              # the index keeps what it had
    for good in ('tile', 'stream', None):
      index.schedule = good
      assert index.schedule == good


def test_the_other_searches_keep_the_tile_schedule(monkeypatch):
  """`search_diverse`, `search_deep` and `search_groups` on an index set to 'stream' never reach the streaming entry, and
  answer what they answer on an index that was never set."""
  from mmt_amd import search
  q, qw, g, gw = _data(5, 1300, 3, 48, 4)
  index, coarse = _index('bf16', g, gw), _index('fp8', g, gw)
  grouping = index.grouping(torch.arange(1300, device=DEV) // 4)
  calls = {'diverse': lambda: index.search_diverse(q, qw, k=5, shortlist=32),
           'diverse, coarse': lambda: index.search_diverse(q, qw, k=5, shortlist=32, coarse=coarse),
           'deep': lambda: index.search_deep(q, qw, 40, page=16),
           'groups': lambda: index.search_groups(q, qw, grouping, k=5)}
  want = {name: call() for name, call in calls.items()}
  real = search._lib.lib()

  class NoStream:
    def __getattr__(self, name):
      if name == 'mmt_search_topk_stream':
        pytest.fail('the streaming entry was reached')
      return getattr(real, name)
  with _scheduled(index, 'stream'), _scheduled(coarse, 'stream'):
    monkeypatch.setattr(search._lib, 'lib', lambda: NoStream())
    for name, call in calls.items():
      assert _same(call(), want[name]), name
