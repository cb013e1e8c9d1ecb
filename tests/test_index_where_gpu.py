"""Per-query attribute filters on the GPU: where= on `search` (both schedules), `search_deep`, `rank_counts`, `ranks`,
`threshold_counts` and `range_search`, on fp32, bf16 and fp8 indexes and on both index classes (mmt_search_topk_where and
its four kin).  Every claim is one of bit identity.  The expected value is always the PLAIN call on the same
index, post-filtered in numpy by `tag_pass`: the complete ordered list of every row is plain
range_search(-inf, order='score') -- `search`'s order with `search`'s score bits, however deep -- and a filtered list is
what is left of it, in order, padded with (-inf, -1); counts are taken over the same scores by item.  Results are
compared with torch.equal on the indices and on the int32 views of the scores.  M = 2, d = 16: what every storage accepts.

Shapes (NQ, NV): (1, 1) the smallest case; (63, 127) one short of a block and a tile; (65, 129) a second block with one
row, a second tile with one column; (33, 300) the streaming schedule's 32-row blocks, three tiles; (257, 26 500) by
tk_chunk's rule a 256-column chunk, two tiles per block (asserted through mmt_topk_workspace_keys): a running list or a
counter carried wrongly across tiles, a skipped first or second tile.  At NV = 1 no row can have both a passing and a
failing item, so (1, 1) takes the two cases that need none (all-zero masks, nobody passes) and the others start at
(63, 127)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
FP8 = torch.float8_e4m3fn
DTYPES = [torch.float32, torch.bfloat16, FP8]
IDS = ['fp32', 'bf16', 'fp8']
M, D = 2, 16
SHAPES = [(1, 1), (63, 127), (65, 129), (33, 300), (257, 26500)]
SHAPE_IDS = ['%dx%d' % s for s in SHAPES]
KS = (1, 10, 128)
INF = float('inf')
B0, B31, B32, B63 = (np.uint64(1) << np.uint64(b) for b in (0, 31, 32, 63))
LAST, LONE, NOBODY = (np.uint64(1) << np.uint64(b) for b in (40, 41, 42))   # the last item; one or two lone items; no item
CASES = ['zero', 'nobody', 'last', 'tile', 'wave', 'all_of', 'none_of', 'any_of', 'all_three']
_cache = {}


def _data(shape):
  """The gallery and the queries of a shape; items 5 .. 8 are copies of item 5 where there are that many (ties)."""
  if ('data', shape) not in _cache:
    nq, nv = shape
    gen = torch.Generator(device=DEV).manual_seed(1000 * nq + nv)
    g, gw = torch.randn(nv, M, D, device=DEV, generator=gen), torch.rand(nv, M, device=DEV, generator=gen)
    q, qw = torch.randn(nq, M, D, device=DEV, generator=gen), torch.rand(nq, M, device=DEV, generator=gen)
    if nv > 9:
      g[5:9], gw[5:9] = g[5], gw[5]
    _cache['data', shape] = g, gw, q, qw
  return _cache['data', shape]


def _index(dtype, shape):
  from mmt_amd.search import VideoIndex
  if ('index', dtype, shape) not in _cache:
    g, gw, _, _ = _data(shape)
    _cache['index', dtype, shape] = VideoIndex(g, gw, dtype=dtype)
  return _cache['index', dtype, shape]


def _tags(shape):
  """uint64 [NV]: bits 0, 31, 32 and 63 at random, a 4-bit field in bits 8 .. 11, bit 40 on the last item only, bit 41 on
  item 205 (or the last, if that comes first: the one column of a second tile at NV = 129) and on item 261 -- at
  NV = 26 500 the second tile of block 0 and the first tile of block 1 -- and bit 42 nowhere."""
  if ('tags', shape) not in _cache:
    nv = shape[1]
    rng = np.random.default_rng(nv)
    t = np.zeros(nv, np.uint64)
    for bit in (B0, B31, B32, B63):
      t |= np.where(rng.random(nv) < 0.5, bit, np.uint64(0))
    t |= rng.integers(0, 16, nv).astype(np.uint64) << np.uint64(8)
    t[nv - 1] |= LAST
    t[min(nv - 1, 205)] |= LONE
    if nv > 261:
      t[261] |= LONE
    _cache['tags', shape] = t
  return _cache['tags', shape]


def _tagging(dtype, shape):
  if ('tagging', dtype, shape) not in _cache:
    tags = torch.from_numpy(_tags(shape).view(np.int64)).to(DEV)
    _cache['tagging', dtype, shape] = _index(dtype, shape).tagging(tags)
  return _cache['tagging', dtype, shape]


def _masks(case, shape):
  """uint64 [NQ, 3] = (all_of, none_of, any_of) per row."""
  nq = shape[0]
  m = np.zeros((nq, 3), np.uint64)
  r = np.arange(nq)
  if case == 'nobody':
    m[:, 0] = NOBODY
  elif case == 'last':
    m[:, 0] = LAST
  elif case == 'tile':       # one row has a candidate, in one tile; no other row has any
    m[:, 0] = NOBODY
    m[nq // 2, 0] = LONE
  elif case == 'wave':       # rows 15 and 16 of every block differ: the boundary between two waves of the selection
    m[:, 0] = np.where(r % 64 < 16, B0, np.uint64(0))
    m[:, 1] = np.where(r % 64 < 16, np.uint64(0), B0)
  elif case == 'all_of':
    m[:, 0] = np.array([B0, B31, B32, B63, B0 | B63, B31 | B32], np.uint64)[r % 6]
  elif case == 'none_of':
    m[:, 1] = np.array([B63, B32, B31, B0, B31 | B63, B0 | B32], np.uint64)[r % 6]
  elif case == 'any_of':
    m[:, 2] = np.array([B63, B0 | B31, B32, B32 | B63, B31, B0], np.uint64)[r % 6]
  elif case == 'all_three':
    m[:, 0] = np.array([B0, B63, B32, B31], np.uint64)[r % 4]
    m[:, 1] = np.array([B31, B32, B63, B0], np.uint64)[r % 4]
    m[:, 2] = np.array([B32 | B63, B0 | B31, B0 | (np.uint64(3) << np.uint64(8)), B63 | B32], np.uint64)[r % 4]
  else:
    assert case == 'zero'
  return m


def _filter(dtype, shape, case, tagging=None):
  cols = [torch.from_numpy(np.ascontiguousarray(c).view(np.int64)).to(DEV) for c in _masks(case, shape).T]
  return (tagging or _tagging(dtype, shape)).where(all_of=cols[0], none_of=cols[1], any_of=cols[2])


def _passes(case, shape):
  """tag_pass of the case: bool [NQ, NV] -- with the assertion every case but the first two owes: some row has both a
  passing and a failing item, for a case that filters nothing tests nothing."""
  from mmt_amd.search import tag_pass
  if ('pass', case, shape) not in _cache:
    p = tag_pass(_tags(shape), _masks(case, shape))
    assert p.shape == shape
    if case == 'zero':
      assert p.all()
    elif case == 'nobody':
      assert not p.any()
    else:
      assert (p.any(1) & (~p).any(1)).any(), (case, shape)
    _cache['pass', case, shape] = p
  return _cache['pass', case, shape]


def _reference(dtype, shape):
  """The plain index's complete ordered list of every row, computed once: (scores [NQ, NV] float32, items [NQ, NV] int64)
  in `search`'s order from range_search(-inf, order='score'), and the same scores by item, [NQ, NV].  numpy, on the host."""
  if ('ref', dtype, shape) not in _cache:
    nq, nv = shape
    _, _, q, qw = _data(shape)
    res = _index(dtype, shape).range_search(q, qw, -INF, order='score')
    assert res.counts.tolist() == [nv] * nq
    s, i = res.scores.cpu().numpy().reshape(nq, nv), res.indices.cpu().numpy().reshape(nq, nv)
    by_item = np.empty_like(s)
    np.put_along_axis(by_item, i, s, 1)
    _cache['ref', dtype, shape] = s, i, by_item
  return _cache['ref', dtype, shape]


def _expect(dtype, shape, allowed, width):
  """What is left of the complete lists where `allowed` (bool [NQ, NV], by item) holds, in order, the first `width` of
  it, padded with (-inf, -1) -> (scores, items) on the device."""
  s, i, _ = _reference(dtype, shape)
  keep = np.take_along_axis(allowed, i, 1)
  pos = np.cumsum(keep, 1) - 1
  r, c = np.nonzero(keep & (pos < width))
  out_s, out_i = np.full((shape[0], width), -INF, np.float32), np.full((shape[0], width), -1, np.int64)
  out_s[r, pos[r, c]], out_i[r, pos[r, c]] = s[r, c], i[r, c]
  return torch.from_numpy(out_s).to(DEV), torch.from_numpy(out_i).to(DEV)


def _same(a, b):
  return all(x.dtype == y.dtype and x.shape == y.shape and
             torch.equal(x.view(torch.int32) if x.dtype is torch.float32 else x, y.view(torch.int32) if y.dtype is torch.float32 else y)
             for x, y in zip(a, b))


def test_the_largest_shape_has_two_tiles_per_block():
  from mmt_amd import _lib
  assert _lib.lib().mmt_topk_workspace_keys(257, 26500, 1) == 257 * -(-26500 // 256)   # tk_chunk: 256-column chunks


@pytest.mark.parametrize('shape', SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_filtered_search_is_the_plain_list_post_filtered(dtype, shape):
  """Every filter case, k = 1, 10 and 128, on the tile schedule and on the streaming one: the expected list at the widest
  k is computed once per case, the best k of a row are the first k of it."""
  from mmt_amd.search import VideoIndex
  nq, nv = shape
  _, _, q, qw = _data(shape)
  index = _index(dtype, shape)
  stream = VideoIndex.__new__(VideoIndex)            # the same stored tensors on the other schedule
  stream.__dict__.update(index.__dict__)
  stream.schedule = 'stream'
  for case in CASES if nv > 1 else CASES[:2]:
    flt, allowed = _filter(dtype, shape, case), _passes(case, shape)
    want = _expect(dtype, shape, allowed, min(128, nv))
    for k in KS:
      w = min(k, nv)
      got = index.search(q, qw, k=k, where=flt)
      assert got[0].shape == got[1].shape == (nq, w) and got[0].dtype is torch.float32 and got[1].dtype is torch.int64
      assert _same(got, (want[0][:, :w], want[1][:, :w])), (case, k)
      assert _same(stream.search(q, qw, k=k, where=flt), got), (case, k, 'stream')
      if case == 'zero':                                               # equals plain search, with no vacant slot
        assert _same(got, index.search(q, qw, k=k)) and (got[1] >= 0).all(), k
      if case == 'nobody':                                             # every slot vacant
        assert (got[1] == -1).all() and torch.isneginf(got[0]).all(), k
      if case == 'last':
        assert (got[1][:, 0] == nv - 1).all() and (got[1][:, 1:] == -1).all(), k
  # ints broadcast to every row: the same answer as the masks written out
  if nv > 1:
    word = int(B63 | B0)
    flt = _tagging(dtype, shape).where(none_of=word)
    rows = torch.full((nq,), word - (1 << 64), device=DEV, dtype=torch.int64)
    assert _same(index.search(q, qw, k=10, where=flt), index.search(q, qw, k=10, where=_tagging(dtype, shape).where(none_of=rows)))


@pytest.mark.parametrize('shape', [(65, 129), (33, 300)], ids=['65x129', '33x300'])
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_the_filter_is_anded_with_subset_exclude_and_after(dtype, shape):
  nq, nv = shape
  _, _, q, qw = _data(shape)
  index = _index(dtype, shape)
  for case in ('all_three', 'wave', 'tile'):
    flt, passes = _filter(dtype, shape, case), _passes(case, shape)
    # subset: every third item and the lone ones; the width is min(k, subset.count)
    in_subset = (np.arange(nv) % 3 == 0) | ((_tags(shape) & LONE) != 0)
    subset = index.subset(torch.from_numpy(in_subset).to(DEV))
    # exclude: per row its best passing item, an item that does not pass, an item outside the subset, -1
    best = _expect(dtype, shape, passes, 1)[1][:, 0]
    exclude = torch.stack([best, torch.full_like(best, nv - 2), torch.full_like(best, 1), torch.full_like(best, -1)], 1)
    barred = np.zeros(shape, bool)
    ex = exclude.cpu().numpy()
    for j in range(ex.shape[1]):
      rows = np.nonzero(ex[:, j] >= 0)[0]
      barred[rows, ex[rows, j]] = True
    for k in KS:
      w = min(k, subset.count)
      assert _same(index.search(q, qw, k=k, where=flt, subset=subset), _expect(dtype, shape, passes & in_subset, w)), (case, k)
      assert _same(index.search(q, qw, k=k, where=flt, exclude=exclude),
                   _expect(dtype, shape, passes & ~barred, min(k, nv))), (case, k)
      assert _same(index.search(q, qw, k=k, where=flt, subset=subset, exclude=exclude),
                   _expect(dtype, shape, passes & in_subset & ~barred, w)), (case, k)
    # after: page 2 continues page 1; search_deep: the concatenated pages are the whole filtered list, then vacant slots
    whole = _expect(dtype, shape, passes & ~barred, nv)
    page1 = index.search(q, qw, k=10, where=flt, exclude=exclude)
    page2 = index.search(q, qw, k=10, where=flt, exclude=exclude, after=(page1[0][:, -1], page1[1][:, -1]))
    assert _same(page1, (whole[0][:, :10], whole[1][:, :10])) and _same(page2, (whole[0][:, 10:20], whole[1][:, 10:20])), case
    for page in (64, 37):
      assert _same(index.search_deep(q, qw, depth=nv, page=page, where=flt, exclude=exclude), whole), (case, page)
    left = (passes & ~barred).sum(1)
    assert (whole[1].cpu().numpy() >= 0).sum(1).tolist() == left.tolist() and left.max() < nv   # they do end in vacant slots
    deep = index.search_deep(q, qw, depth=nv, where=flt, subset=subset)
    assert _same(deep, _expect(dtype, shape, passes & in_subset, subset.count)), case


def _targets(passes):
  """int64 [NQ, 3]: the row's first passing item, its first failing item (-1 where there is none), and -1."""
  first = lambda mask: np.where(mask.any(1), mask.argmax(1), -1)
  return np.stack([first(passes), first(~passes), np.full(passes.shape[0], -1)], 1).astype(np.int64)


def _counts(by_item, passes, thr):
  """(greater, equal) int32 [NQ, T] over the passing items of every row, against thr float32 [NQ, T] (NaN counts nothing)."""
  with np.errstate(invalid='ignore'):
    greater = (passes[:, None, :] & (by_item[:, None, :] > thr[:, :, None])).sum(2)
    equal = (passes[:, None, :] & (by_item[:, None, :] == thr[:, :, None])).sum(2)
  return greater.astype(np.int32), equal.astype(np.int32)


@pytest.mark.parametrize('shape', SHAPES[1:], ids=SHAPE_IDS[1:])
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_filtered_counts_are_counts_over_the_filtered_rows(dtype, shape):
  nq, nv = shape
  _, _, q, qw = _data(shape)
  index = _index(dtype, shape)
  by_item = _reference(dtype, shape)[2]
  in_subset = np.arange(nv) % 2 == 0
  subset = index.subset(torch.from_numpy(in_subset).to(DEV))
  for case in ('all_three', 'tile', 'nobody', 'zero'):
    flt, passes = _filter(dtype, shape, case), _passes(case, shape)
    tg = _targets(passes)
    if case == 'all_three':
      assert (tg[:, 0] >= 0).any() and (tg[:, 1] >= 0).any()           # a target that passes, a target that does not
    thr = np.where(tg >= 0, np.take_along_axis(by_item, tg.clip(0), 1), np.float32('nan')).astype(np.float32)
    targets = torch.from_numpy(tg).to(DEV)
    for allowed, kwargs in ((passes, {}), (passes & in_subset, {'subset': subset})):
      greater, equal = (torch.from_numpy(c).to(DEV) for c in _counts(by_item, allowed, thr))
      got = index.rank_counts(q, qw, targets, where=flt, **kwargs)
      assert got[0].dtype is torch.int32 and torch.equal(got[0], greater) and torch.equal(got[1], equal), (case, sorted(kwargs))
      # a passing target counts itself, one that does not pass does not, a target of -1 counts nothing
      hit = np.take_along_axis(allowed, tg.clip(0), 1) & (tg >= 0)
      assert ((got[1].cpu().numpy() >= 1) == hit).all() or case == 'zero', case
      assert not got[0][:, 2].any() and not got[1][:, 2].any()
      thresholds = torch.from_numpy(thr).to(DEV)
      assert all(torch.equal(a, b) for a, b in zip(index.threshold_counts(q, qw, thresholds, where=flt, **kwargs), (greater, equal)))
      ranks = index.ranks(q, qw, targets, where=flt, **kwargs)
      want = torch.where(torch.from_numpy(hit).to(DEV), greater.double() + (equal.double() - 1) / 2,
                         torch.full(tg.shape, INF, device=DEV, dtype=torch.float64))
      assert torch.equal(ranks, want), (case, sorted(kwargs))
  # one column of targets, as a vector
  flt, passes = _filter(dtype, shape, 'all_of'), _passes('all_of', shape)
  tg = _targets(passes)[:, 0]
  thr = np.where(tg >= 0, by_item[np.arange(nq), tg.clip(0)], np.float32('nan')).astype(np.float32)[:, None]
  greater, equal = _counts(by_item, passes, thr)
  got = index.rank_counts(q, qw, torch.from_numpy(tg).to(DEV), where=flt)
  assert got[0].shape == (nq,) and got[0].cpu().numpy().tolist() == greater[:, 0].tolist()
  assert got[1].cpu().numpy().tolist() == equal[:, 0].tolist()


@pytest.mark.parametrize('shape', SHAPES[1:], ids=SHAPE_IDS[1:])
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_filtered_range_search_is_the_filtered_plain_csr(dtype, shape):
  nq, nv = shape
  _, _, q, qw = _data(shape)
  index = _index(dtype, shape)
  s, i, by_item = _reference(dtype, shape)
  thr = np.median(by_item, 1).astype(np.float32)                       # about half of a row's items, one threshold per row
  thr[0] = -INF
  if nq > 2:
    thr[1], thr[2] = INF, np.float32('nan')
  threshold = torch.from_numpy(thr).to(DEV)
  in_subset = np.arange(nv) % 2 == 1
  subset = index.subset(torch.from_numpy(in_subset).to(DEV))
  for case in ('all_three', 'tile', 'wave', 'nobody', 'zero'):
    flt, passes = _filter(dtype, shape, case), _passes(case, shape)
    for allowed, kwargs in ((passes, {}), (passes & in_subset, {'subset': subset})):
      with np.errstate(invalid='ignore'):
        hits = allowed & (by_item >= thr[:, None])
      offsets = np.concatenate([[0], np.cumsum(hits.sum(1))]).astype(np.int64)
      got = index.range_search(q, qw, threshold, where=flt, **kwargs)
      r, c = np.nonzero(hits)                                          # by row, then by ascending item
      assert got.offsets.cpu().numpy().tolist() == offsets.tolist(), (case, sorted(kwargs))
      assert got.indices.cpu().numpy().tolist() == c.tolist(), (case, sorted(kwargs))
      assert np.array_equal(got.scores.cpu().numpy().view(np.int32), by_item[r, c].view(np.int32)), (case, sorted(kwargs))
      got = index.range_search(q, qw, threshold, order='score', where=flt, **kwargs)
      keep = np.take_along_axis(hits, i, 1)                            # the complete lists are in `search`'s order already
      r, c = np.nonzero(keep)
      assert got.offsets.cpu().numpy().tolist() == offsets.tolist(), (case, sorted(kwargs))
      assert got.indices.cpu().numpy().tolist() == i[r, c].tolist(), (case, sorted(kwargs))
      assert np.array_equal(got.scores.cpu().numpy().view(np.int32), s[r, c].view(np.int32)), (case, sorted(kwargs))
    if case == 'zero':
      plain = index.range_search(q, qw, threshold)
      got = index.range_search(q, qw, threshold, where=flt)
      assert torch.equal(got.offsets, plain.offsets) and torch.equal(got.indices, plain.indices)


def _sharded(dtype, shape):
  """The shape's gallery on three shards of unequal sizes, all on device 0: global numbers in insertion order."""
  from mmt_amd.search import ShardedVideoIndex
  if ('sharded', dtype, shape) not in _cache:
    nv = shape[1]
    g, gw, _, _ = _data(shape)
    index = ShardedVideoIndex.empty(3 * nv, M, D, [DEV] * 3, dtype=dtype)
    cuts = [0, nv // 6, nv // 6 + nv // 2, nv]
    for lo, hi in zip(cuts[:-1], cuts[1:]):
      index.add(g[lo:hi], gw[lo:hi])
    assert len(set(index.shard_sizes)) == 3 and sum(index.shard_sizes) == nv
    _cache['sharded', dtype, shape] = index
  return _cache['sharded', dtype, shape]


@pytest.mark.parametrize('shape', [(65, 129), (33, 300)], ids=['65x129', '33x300'])
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_sharded_index_is_bit_identical(dtype, shape):
  from mmt_amd.search import ShardedTagging
  nq, nv = shape
  _, _, q, qw = _data(shape)
  one, many = _index(dtype, shape), _sharded(dtype, shape)
  tags = torch.from_numpy(_tags(shape).view(np.int64)).to(DEV)
  tagging = many.tagging(tags)
  assert isinstance(tagging, ShardedTagging) and tagging.num_items == nv and torch.equal(tagging.tags, tags)
  assert [p.num_items for p in tagging.parts] == many.shard_sizes
  for s, part in enumerate(tagging.parts):
    assert torch.equal(part.tags, tags[many.shards[s].ids[:part.num_items]])
  in_subset = np.arange(nv) % 3 != 1
  mask = torch.from_numpy(in_subset).to(DEV)
  exclude = torch.stack([torch.arange(nq, device=DEV) % nv, torch.full((nq,), -1, device=DEV)], 1)
  threshold = torch.from_numpy(np.median(_reference(dtype, shape)[2], 1).astype(np.float32)).to(DEV)
  for case in ('all_three', 'tile', 'wave', 'nobody'):
    a, b = _filter(dtype, shape, case), _filter(dtype, shape, case, tagging)
    targets = torch.from_numpy(_targets(_passes(case, shape))).to(DEV)
    for schedule in (None, 'stream'):
      many.schedule = schedule
      for k in KS:
        assert _same(many.search(q, qw, k=k, where=b), one.search(q, qw, k=k, where=a)), (case, k, schedule)
        assert _same(many.search(q, qw, k=k, where=b, subset=many.subset(mask), exclude=exclude),
                     one.search(q, qw, k=k, where=a, subset=one.subset(mask), exclude=exclude)), (case, k, schedule)
    many.schedule = None
    assert _same(many.search_deep(q, qw, depth=nv, where=b), one.search_deep(q, qw, depth=nv, where=a)), case
    for kwargs_many, kwargs_one in (({}, {}), ({'subset': many.subset(mask)}, {'subset': one.subset(mask)})):
      assert _same(many.rank_counts(q, qw, targets, where=b, **kwargs_many), one.rank_counts(q, qw, targets, where=a, **kwargs_one)), case
      assert torch.equal(many.ranks(q, qw, targets, where=b, **kwargs_many), one.ranks(q, qw, targets, where=a, **kwargs_one)), case
      for order in ('index', 'score'):
        x = many.range_search(q, qw, threshold, order=order, where=b, **kwargs_many)
        y = one.range_search(q, qw, threshold, order=order, where=a, **kwargs_one)
        assert torch.equal(x.offsets, y.offsets) and torch.equal(x.indices, y.indices), (case, order)
        assert torch.equal(x.scores.view(torch.int32), y.scores.view(torch.int32)), (case, order)


def test_search_refined_filters_the_coarse_stage():
  shape = (33, 300)
  _, _, q, qw = _data(shape)
  fine, coarse = _index(torch.float32, shape), _index(FP8, shape)
  flt = _filter(FP8, shape, 'all_three')
  _, shortlisted = coarse.search(q, qw, k=64, where=flt)
  assert _same(fine.search_refined(q, qw, coarse, k=10, shortlist=64, where=flt), fine.rescore(q, qw, shortlisted, 10))
  with pytest.raises(ValueError, match='the tagging was built for 129 items, the index holds 300'):
    fine.search_refined(q, qw, coarse, k=10, shortlist=64, where=_filter(FP8, (65, 129), 'all_three'))   # checked by `coarse`


def test_refusals_are_raised_by_name_before_anything_is_scored():
  from mmt_amd.search import VideoIndex
  shape = (33, 300)
  nq, nv = shape
  g, gw, q, qw = _data(shape)
  index, tagging = _index(torch.float32, shape), _tagging(torch.float32, shape)
  flt = tagging.where(all_of=1)
  targets = torch.zeros(nq, device=DEV, dtype=torch.int64)
  norm = index.hub_norm(q, qw, 10.0)
  options = {'norm': norm, 'pooling': index.pooling(1, nq), 'item_pooling': index.item_pooling(1)}
  for name, value in options.items():
    for call in (lambda **kw: index.search(q, qw, **kw), lambda **kw: index.rank_counts(q, qw, targets, **kw),
                 lambda **kw: index.ranks(q, qw, targets, **kw),
                 lambda **kw: index.threshold_counts(q, qw, torch.zeros(nq, device=DEV), **kw)):
      with pytest.raises(ValueError, match='where= does not combine with %s=' % name):
        call(where=flt, **{name: value})
  with pytest.raises(ValueError, match='where= does not combine with norm='):
    index.search_deep(q, qw, depth=200, where=flt, norm=norm)
  # a filter of another row count, of another tagging, of an index that has grown
  rows = tagging.where(all_of=torch.zeros(nq + 1, device=DEV, dtype=torch.int64))
  for call in (lambda w: index.search(q, qw, where=w), lambda w: index.rank_counts(q, qw, targets, where=w),
               lambda w: index.range_search(q, qw, 0.0, where=w), lambda w: index.search_deep(q, qw, depth=200, where=w)):
    with pytest.raises(ValueError, match='%d query rows but the where= filter holds %d rows' % (nq, nq + 1)):
      call(rows)
    with pytest.raises(ValueError, match='where must come from the where'):
      call(torch.zeros(nq, 3, device=DEV, dtype=torch.int64))
  grown = VideoIndex.empty(nv + 1, M, D, DEV)
  grown.add(g, gw)
  old = grown.tagging(tagging.tags).where()
  assert grown.search(q, qw, k=1, where=old)[1].shape == (nq, 1)
  nbytes = grown.nbytes
  grown.add(g[:1], gw[:1])
  assert grown.nbytes == nbytes                                        # the index's own storage does not change
  with pytest.raises(ValueError, match='the tagging was built for %d items, the index holds %d' % (nv, nv + 1)):
    grown.search(q, qw, k=1, where=old)
  with pytest.raises(ValueError, match='the tagging was built for %d items' % nv):
    grown.range_search(q, qw, 0.0, where=flt)
  # the calls that take no filter
  grouping = index.grouping(torch.arange(nv, device=DEV))
  cand = torch.zeros(nq, 4, device=DEV, dtype=torch.int64)
  for who, call in (('search_groups', lambda: index.search_groups(q, qw, grouping, where=flt)),
                    ('rescore', lambda: index.rescore(q, qw, cand, where=flt)),
                    ('reverse_search', lambda: index.reverse_search(q, qw, where=flt)),
                    ('neighbours', lambda: index.neighbours(where=flt)),
                    ('neighbour_range', lambda: index.neighbour_range(0.5, where=flt)),
                    ('duplicate_groups', lambda: index.duplicate_groups(0.5, where=flt)),
                    ('query_lse', lambda: index.query_lse(q, qw, 10.0, where=flt))):
    with pytest.raises(ValueError, match='%s: where= is out of scope' % who):
      call()
  index.schedule = 'stream'
  try:
    with pytest.raises(ValueError, match="does not combine with norm="):
      index.search(q, qw, where=flt, norm=norm)
  finally:
    index.schedule = None
