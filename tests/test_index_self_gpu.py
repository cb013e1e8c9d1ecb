"""The gallery self-join on the GPU: VideoIndex.neighbours (mmt_search_self_topk), neighbour_range
(mmt_search_self_range_count, mmt_search_self_range_fill) and duplicate_groups, on all three storage dtypes and both index
classes.  The reference is the device's own `pair_scores`: the full 300 x 300 matrix S of gallery A, built once per dtype
from 64-item blocks, and every claim against it is a claim of bit identity, compared with torch.equal on the indices and
on the int32 views of the floats -- the lists against tests.test_index_self_cpu.brute_neighbours / brute_range fed S.  The
score itself is held to the fp64 value of its definition on the stored values within the bound test_index_diverse_gpu
derives.  Gallery A is that module's: rows 100 .. 139 and 250 .. 259 exact copies of row 100 (50-way ties beyond k = 10),
item 7 with all-zero weights; M = 3, d = 64, 300 items = three 128-column tiles, the last with 44 live columns, one tile
per chunk, so the merge runs."""
import pytest
import torch

from tests.test_index_diverse_gpu import DEV, DTYPES, FP8, IDS, NV, _bits, _data, _definition, _index, _sharded
from tests.test_index_self_cpu import brute_neighbours, brute_range

pytestmark = pytest.mark.gpu
INF = float('inf')
COPIES = list(range(100, 140)) + list(range(250, 260))
_cache = {}


def _matrix(dtype):
  """S float32 [300, 300] on the host: S[g, h] = pair_scores' sim(g, h) on the index of this dtype, from 64-item blocks:
  one 128-wide list per pair of blocks (block i, then block j, padded with -1), whose [0:64, 64:128] corner is S[i, j]."""
  if dtype not in _cache:
    index = _index(dtype)
    blocks = [torch.arange(b, min(NV, b + 64), device=DEV) for b in range(0, NV, 64)]
    lists = torch.full((len(blocks) ** 2, 128), -1, device=DEV, dtype=torch.int64)
    for i, bi in enumerate(blocks):
      for j, bj in enumerate(blocks):
        lists[i * len(blocks) + j, :bi.numel()] = bi
        lists[i * len(blocks) + j, 64:64 + bj.numel()] = bj
    sims = index.pair_scores(lists)
    s = torch.empty(NV, NV, device=DEV, dtype=torch.float32)
    for i, bi in enumerate(blocks):
      for j, bj in enumerate(blocks):
        s[bi[0]:bi[-1] + 1, bj[0]:bj[-1] + 1] = sims[i * len(blocks) + j, :bi.numel(), 64:64 + bj.numel()]
    assert not torch.isnan(s).any()
    _cache[dtype] = s.cpu()
    assert _cache[dtype].dtype is torch.float32 and _cache[dtype].shape == (NV, NV)
  return _cache[dtype]


def _rows(r):
  """The rows of a join of R rows: every item in order for 300; else drawn with repeats and in no order, item 100 (a
  copy) and item 7 (zero weights) among them when there is room."""
  if r == NV:
    return None
  gen = torch.Generator().manual_seed(r)
  items = torch.randint(0, NV, (r,), generator=gen)
  if r >= 4:
    items[1], items[2], items[3] = 100, 7, items[0]
  return items


def _same(got, want):
  assert len(got) == len(want)
  for x, y in zip(got, want):
    assert x.dtype == y.dtype and tuple(x.shape) == tuple(y.shape), (x.dtype, y.dtype, x.shape, y.shape)
    assert torch.equal(_bits(x.cpu()), _bits(y.cpu()))


@pytest.mark.parametrize('r', [1, 65, NV])   # 65: one live row in the second row block
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_neighbours_have_the_bits_and_the_order_of_pair_scores(dtype, r):
  index, s, items = _index(dtype), _matrix(dtype), _rows(r)
  own = torch.arange(NV) if items is None else items
  for k in (1, 10, 128):
    got = index.neighbours(k=k, items=None if items is None else items.to(DEV))
    assert got[0].device == DEV and got[0].shape == (r, k)
    want = brute_neighbours(s[own], own, k)
    _same(got, want)
  scores, indices = got
  assert (indices != own.to(DEV)[:, None]).all()                       # the self pair is left out by number
  copy = torch.isin(own, torch.tensor(COPIES))
  if copy.any():   # ... not by score: the other 49 exact copies lead a copy's list, ascending, with the diagonal's bits
    lead = indices[copy.to(DEV)][:, :49].cpu()
    assert all(row.tolist() == [c for c in COPIES if c != g] for row, g in zip(lead, own[copy].tolist()))
    assert torch.equal(_bits(scores[copy.to(DEV)][:, :49].cpu()), _bits(s[100, 100].expand(int(copy.sum()), 49).contiguous()))


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_a_subset_restricts_the_candidates_and_changes_no_bit(dtype):
  index, s = _index(dtype), _matrix(dtype)
  allowed = torch.zeros(NV, dtype=torch.bool)
  allowed[0:128:3] = True                       # a ragged tile; tile 1 (128 .. 255) is empty and skipped
  allowed[[256, 257, 259, 298, 299]] = True     # and a few of the last tile's 44, copies among them
  subset = index.subset(allowed.to(DEV))
  for items in (None, _rows(65)):
    own = torch.arange(NV) if items is None else items
    for k in (10, 128):
      got = index.neighbours(k=k, items=None if items is None else items.to(DEV), subset=subset)
      _same(got, brute_neighbours(s[own], own, k, allowed))
      assert allowed[got[1].cpu().clamp(min=0)].all() and (got[1][:, int(allowed.sum()):] == -1).all()
  lone = index.subset(torch.tensor([100], device=DEV))                 # row 100's only candidate is itself: an empty list
  scores, indices = index.neighbours(k=3, items=torch.tensor([100, 101], device=DEV), subset=lone)
  assert indices.tolist() == [[-1, -1, -1], [100, -1, -1]] and scores[0].tolist() == [-INF] * 3


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_scores_are_the_definition_on_the_stored_values(dtype):
  """Against the fp64 value of sim on the values read back from the index, within gamma_K sum |f_g f_h| / |den| +
  2^-22 |value| with K = 192 (test_index_diverse_gpu._definition: derived, not tuned)."""
  value, tol = _definition(dtype)
  scores, indices = _index(dtype).neighbours(k=128)
  got, at = scores.cpu().double().numpy(), indices.cpu().numpy()
  rows = torch.arange(NV).numpy()[:, None].repeat(128, 1)
  err = abs(got - value[rows, at])
  print('%s: max |error| %.3g, max error / bound %.3g over %d pairs' % (
      dtype, err.max(), (err / tol[rows, at].clip(1e-300)).max(), err.size))
  assert (at >= 0).all() and (err <= tol[rows, at]).all()


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_a_small_index_pads_its_lists(dtype):
  """5 items, M = 1, d = 16: K is shorter than one slab (the fp8 minimum width); k = 10 gives 4 neighbours, then (-inf, -1)."""
  from mmt_amd.search import VideoIndex
  gen = torch.Generator(device=DEV).manual_seed(5)
  g, gw = torch.randn(5, 1, 16, device=DEV, generator=gen), torch.rand(5, 1, device=DEV, generator=gen)
  index = VideoIndex(g, gw, dtype=dtype)
  s = index.pair_scores(torch.arange(5, device=DEV)[None])[0].cpu()
  got = index.neighbours(k=10)
  _same(got, brute_neighbours(s, torch.arange(5), 10))
  assert (got[1][:, :4] >= 0).all() and (got[1][:, 4:] == -1).all() and (got[0][:, 4:] == -INF).all()
  hits = index.neighbour_range(-INF)
  assert hits.offsets.tolist() == [0, 4, 8, 12, 16, 20]
  _same((hits.offsets, hits.indices, hits.scores), brute_range(s, torch.arange(5), torch.full((5,), -INF)))


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_row_batching_and_a_second_run_change_no_bit(dtype, monkeypatch):
  from mmt_amd import search
  index, items = _index(dtype), _rows(200).to(DEV)
  thr = torch.full((200,), float(_matrix(dtype)[3, 4]), device=DEV)
  first = index.neighbours(k=10, items=items)
  hits = index.neighbour_range(thr, items=items)
  monkeypatch.setattr(search, '_BATCH_BYTES', 1)                        # 64 rows per launch
  assert index._row_batches(200, 0) == [(0, 64), (64, 128), (128, 192), (192, 200)]
  for _ in range(2):
    _same(index.neighbours(k=10, items=items), first)
    again = index.neighbour_range(thr, items=items)
    _same((again.offsets, again.indices, again.scores), (hits.offsets, hits.indices, hits.scores))


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_a_ragged_last_slab_of_the_stored_row_loops(dtype):
  """Several slabs, then a partial one, in the K loops over two stored rows: 130 items (two column tiles, the second with
  2 live columns; three row blocks, the last with 2 rows), M = 7, d = 16, so K = 112 = 3.5 fp32 slabs = 1.75 16-bit slabs.
  Item 7 has all-zero weights (the 1e-5 denominator), item 129 is an exact copy of item 3 (another tile, another row block).
  pair_scores over 128-wide lists of 64-item blocks is held to the fp64 definition on the stored values within
  gamma_K sum |f_g f_h| / |den| + 2^-22 |value|, gamma_K = K u / (1 - K u) with K = 112 and u = 2^-24: the worst case of
  an fp32 sum of K exact products in any order, plus the scale multiply and the division (test_index_diverse_gpu.
  _definition's formula: derived, not tuned).  neighbours and neighbour_range (threshold: the matrix's median, one of its
  own values) have that matrix's bits and order."""
  import numpy as np
  from mmt_amd.search import VideoIndex
  nv, m, d = 130, 7, 16
  gamma = m * d * 2.0 ** -24 / (1 - m * d * 2.0 ** -24)
  gen = torch.Generator(device=DEV).manual_seed(nv)
  g, gw = torch.randn(nv, m, d, device=DEV, generator=gen), torch.rand(nv, m, device=DEV, generator=gen)
  g[129], gw[129] = g[3], gw[3]
  gw[7] = 0
  index = VideoIndex(g, gw, dtype=dtype)
  blocks = [torch.arange(b, min(nv, b + 64), device=DEV) for b in range(0, nv, 64)]
  lists = torch.full((len(blocks) ** 2, 128), -1, device=DEV, dtype=torch.int64)
  for i, bi in enumerate(blocks):
    for j, bj in enumerate(blocks):
      lists[i * len(blocks) + j, :bi.numel()] = bi
      lists[i * len(blocks) + j, 64:64 + bj.numel()] = bj
  sims = index.pair_scores(lists)
  s = torch.empty(nv, nv, device=DEV, dtype=torch.float32)
  for i, bi in enumerate(blocks):
    for j, bj in enumerate(blocks):
      s[bi[0]:bi[-1] + 1, bj[0]:bj[-1] + 1] = sims[i * len(blocks) + j, :bi.numel(), 64:64 + bj.numel()]
  s = s.cpu()
  assert not torch.isnan(s).any()
  f = index.folded[:nv].cpu().float().double().numpy()
  if index.scales is not None:
    f = f * index.scales[:nv].cpu().double().numpy()[:, None]
  w = index.weights[:nv].cpu().double().numpy()
  den = w @ w.T
  den[den == 0] = float(np.float32(1e-5))
  value = (f @ f.T) / den
  tol = gamma * (np.abs(f) @ np.abs(f).T) / np.abs(den) + 2.0 ** -22 * np.abs(value)
  err = np.abs(s.double().numpy() - value)
  print('%s: max |error| %.3g, max error / bound %.3g over %d pairs' % (dtype, err.max(), (err / tol.clip(1e-300)).max(),
                                                                        err.size))
  assert f.shape == (nv, m * d) and (err <= tol).all()
  assert torch.equal(_bits(s[3]), _bits(s[129])) and torch.equal(_bits(s[:, 3].contiguous()), _bits(s[:, 129].contiguous()))
  own = torch.arange(nv)
  _same(index.neighbours(k=128), brute_neighbours(s, own, 128))
  thr = float(s.median())
  hits = index.neighbour_range(thr)
  _same((hits.offsets, hits.indices, hits.scores), brute_range(s, own, torch.full((nv,), thr)))
  assert 0 < int(hits.offsets[-1]) < nv * (nv - 1)


def _thresholds(s, own):
  """One threshold per row, taken from S itself -- the row's sim to item (7 row + 3) % 300, which must then be hit unless
  it is the row's own item -- with rows 10 .. 19 at -inf (every item but the row's own) and 20 .. 29 at NaN (nothing)."""
  target = (7 * torch.arange(own.shape[0]) + 3) % NV
  thr = s[own, target].clone()
  thr[10:20], thr[20:30] = -INF, float('nan')
  return thr, target


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_neighbour_range_is_the_brute_force_on_pair_scores(dtype):
  index, s = _index(dtype), _matrix(dtype)
  for items in (None, _rows(65)):
    own = torch.arange(NV) if items is None else items
    thr, target = _thresholds(s, own)
    want = brute_range(s[own], own, thr)
    dev_items = None if items is None else items.to(DEV)
    hits = index.neighbour_range(thr.to(DEV), items=dev_items)
    _same((hits.offsets, hits.indices, hits.scores), want)
    assert torch.equal(hits.counts, hits.offsets[1:] - hits.offsets[:-1]) and hits.indices.device == DEV
    counts = hits.counts.cpu()
    assert (counts[10:20] == NV - 1).all() and (counts[20:30] == 0).all()
    for row in (0, 5, 40, 64):   # exact equality hits
      if target[row] != own[row]:
        assert int(target[row]) in hits.indices[hits.offsets[row]:hits.offsets[row + 1]].tolist()
    # order='score' is `search`'s order: a row's first k entries are its `neighbours`
    by_score = index.neighbour_range(thr.to(DEV), items=dev_items, order='score')
    assert torch.equal(by_score.offsets, hits.offsets)
    scores, indices = index.neighbours(k=10, items=dev_items)
    for row in (0, 10, 15, 64):
      lo, n = int(by_score.offsets[row]), min(10, int(counts[row]))
      assert torch.equal(by_score.indices[lo:lo + n], indices[row, :n])
      assert torch.equal(_bits(by_score.scores[lo:lo + n] + 0.0), _bits(scores[row, :n]))
    total = int(hits.offsets[-1])
    with pytest.raises(ValueError, match='neighbour_range: %d hits exceed max_hits = %d' % (total, total - 1)):
      index.neighbour_range(thr.to(DEV), items=dev_items, max_hits=total - 1)
    assert index.neighbour_range(thr.to(DEV), items=dev_items, max_hits=total).indices.shape[0] == total
  plain = index.neighbour_range(float(s[0, 3]))                        # a Python float: one threshold for every row
  _same((plain.offsets, plain.indices, plain.scores), brute_range(s, torch.arange(NV), torch.full((NV,), float(s[0, 3]))))
  none = index.neighbour_range(float('nan'), items=torch.zeros(0, dtype=torch.int64, device=DEV))
  assert none.offsets.tolist() == [0] and none.indices.shape == (0,)


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_source_joins_another_index_against_this_one(dtype):
  """An index holding rows 90 .. 109 of gallery A, joined against A: `neighbours(items=arange(90, 110))` with the self
  pair put back."""
  from mmt_amd.search import VideoIndex
  g, gw, _, _ = _data()
  index, s = _index(dtype), _matrix(dtype)
  batch = VideoIndex(g[90:110], gw[90:110], dtype=dtype)
  none = torch.full((20,), -1)
  _same(index.neighbours(k=10, source=batch), brute_neighbours(s[90:110], none, 10))
  pick = torch.tensor([19, 0, 10, 10])                                  # `items` numbers the source
  _same(index.neighbours(k=128, source=batch, items=pick.to(DEV)), brute_neighbours(s[90 + pick], none[:4], 128))
  own = index.neighbours(k=10, items=torch.arange(90, 110, device=DEV))
  joined = index.neighbours(k=11, source=batch)
  for row in range(20):   # the row's own item, back in its place in the order, and then the same list
    keep = joined[1][row] != 90 + row
    assert int(keep.sum()) == 10 or 90 + row in COPIES                  # (a copy's own item may tie beyond slot 11)
    if int(keep.sum()) == 10:
      assert torch.equal(joined[1][row][keep], own[1][row]) and torch.equal(_bits(joined[0][row][keep]), _bits(own[0][row]))
  thr = torch.full((20,), float(s[100, 100]))
  hits = index.neighbour_range(thr.to(DEV), source=batch)
  _same((hits.offsets, hits.indices, hits.scores), brute_range(s[90:110], none, thr))
  assert hits.counts[10:].tolist() == [50] * 10                         # rows 100 .. 109: all fifty copies, themselves included


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_a_sharded_index_is_bit_identical(dtype, monkeypatch):
  from mmt_amd import search
  mono, shards, s = _index(dtype), _sharded(dtype), _matrix(dtype)
  allowed = torch.zeros(NV, dtype=torch.bool)
  allowed[0:128:3], allowed[[256, 257, 259, 298, 299]] = True, True
  for items in (None, _rows(65)):
    own = torch.arange(NV) if items is None else items
    dev_items = None if items is None else items.to(DEV)
    thr = _thresholds(s, own)[0].to(DEV)
    for subset in (None, allowed):
      sub = (None, None) if subset is None else (mono.subset(subset.to(DEV)), shards.subset(subset.to(DEV)))
      for k in (10, 128):
        got = shards.neighbours(k=k, items=dev_items, subset=sub[1])
        assert got[0].device == DEV
        _same(got, mono.neighbours(k=k, items=dev_items, subset=sub[0]))
      for order in ('index', 'score'):
        a = shards.neighbour_range(thr, items=dev_items, subset=sub[1], order=order)
        b = mono.neighbour_range(thr, items=dev_items, subset=sub[0], order=order)
        _same((a.offsets, a.indices, a.scores), (b.offsets, b.indices, b.scores))
  _same(shards.neighbours(k=10), brute_neighbours(s, torch.arange(NV), 10))
  level = float(s[100, 101])
  labels = shards.duplicate_groups(level)
  assert labels.device == DEV and torch.equal(labels, mono.duplicate_groups(level))
  with pytest.raises(ValueError, match='neighbour_range: .* hits exceed max_hits = 5'):
    shards.neighbour_range(-INF, max_hits=5)
  monkeypatch.setattr(search, '_BATCH_BYTES', 1)                        # 64-row staging blocks
  assert shards._stage_batches(130) == [(0, 64), (64, 128), (128, 130)]
  _same(shards.neighbours(k=10), mono.neighbours(k=10))
  a, b = shards.neighbour_range(level), mono.neighbour_range(level)
  _same((a.offsets, a.indices, a.scores), (b.offsets, b.indices, b.scores))


def _chain(dtype, sharded):
  """Gallery B, exactly representable in every storage: M = 1, d = 16, weights 1.  Items 0 .. 6: 1.0 at positions i and
  i + 1, so sim(i, i + 1) = 1 and sim(i, i + 2) = 0: a chain that needs several propagation rounds.  Item 7: 1.0 at 10
  and 12, isolated.  Item 8: a copy of item 3."""
  from mmt_amd.search import ShardedVideoIndex, VideoIndex
  g = torch.zeros(9, 1, 16, device=DEV)
  for i in range(7):
    g[i, 0, i] = g[i, 0, i + 1] = 1.0
  g[7, 0, 10] = g[7, 0, 12] = 1.0
  g[8] = g[3]
  gw = torch.ones(9, 1, device=DEV)
  return ShardedVideoIndex(g, gw, [DEV] * 3, dtype=dtype) if sharded else VideoIndex(g, gw, dtype=dtype)


@pytest.mark.parametrize('sharded', [False, True], ids=['VideoIndex', 'ShardedVideoIndex'])
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_duplicate_groups_of_a_chain(dtype, sharded):
  index = _chain(dtype, sharded)
  scores, indices = index.neighbours(k=3, items=torch.tensor([3, 7], device=DEV))
  assert indices.tolist() == [[8, 2, 4], [0, 1, 2]] and scores.tolist() == [[2.0, 1.0, 1.0], [0.0, 0.0, 0.0]]
  labels = index.duplicate_groups(1.0)
  assert labels.dtype is torch.int64 and labels.device == DEV and labels.tolist() == [0, 0, 0, 0, 0, 0, 0, 7, 0]
  assert index.duplicate_groups(2.0).tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 3]      # only the exact copy
  assert index.duplicate_groups(2.5).tolist() == list(range(9))
  part = index.subset(torch.tensor([0, 1, 5, 6, 7], device=DEV))
  assert index.duplicate_groups(1.0, subset=part).tolist() == [0, 0, 2, 3, 4, 5, 5, 7, 8]
  with pytest.raises(ValueError, match='duplicate_groups: 18 hits exceed max_hits = 17'):
    index.duplicate_groups(1.0, max_hits=17)                           # 6 + 3 edges, hit from both ends
  assert index.duplicate_groups(1.0, max_hits=18).tolist() == labels.tolist()


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_duplicate_groups_feed_search_groups(dtype):
  """On gallery A with the threshold S[100, 101] the 50 copies carry label 100; the labels go unchanged into `grouping`,
  and `search_groups` returns the copies' group once where plain `search` returns ten copies.  (`search_groups` is not
  available on a float8_e4m3fn index: there the labels and the grouping are checked.)"""
  index, s = _index(dtype), _matrix(dtype)
  g, gw, _, _ = _data()
  labels = index.duplicate_groups(float(s[100, 101]))
  assert labels.shape == (NV,) and labels[COPIES].tolist() == [100] * 50 and int((labels == 100).sum()) == 50
  rest = torch.ones(NV, dtype=torch.bool)
  rest[COPIES] = False
  assert torch.equal(labels.cpu()[rest], torch.arange(NV)[rest])        # nothing else is that alike
  grouping = index.grouping(labels)
  assert grouping.num_groups == NV - 49 and grouping.num_items == NV
  if dtype == FP8:
    return
  q, qw = g[100:101], gw[100:101]
  _, plain = index.search(q, qw, k=10)
  assert plain[0].tolist() == COPIES[:10]
  scores, groups, items = index.search_groups(q, qw, grouping, k=10)
  assert groups[0, 0] == 100 and items[0, 0] == 100 and int((groups[0] == 100).sum()) == 1
  assert not torch.isin(items[0, 1:].cpu(), torch.tensor(COPIES)).any()
