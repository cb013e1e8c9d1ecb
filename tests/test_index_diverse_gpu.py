"""The diversified search on the GPU: VideoIndex.pair_scores (mmt_search_pair_scores), diversify (mmt_search_mmr on top of
`rescore`) and search_diverse, on all three storage dtypes and both index classes.  The item-item score is held to the fp64
value of its definition on the stored values, within the worst-case bound of an fp32 sum of exact products; everything
else is a claim of bit identity, compared with torch.equal on the indices and on the int32 views of the floats: the
selection against tests.test_index_diverse_cpu.brute_mmr fed the device's own relevances and Gram."""
import numpy as np
import pytest
import torch

from tests.test_index_diverse_cpu import padded_mmr, weights_of

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
FP8 = torch.float8_e4m3fn
DTYPES = [torch.float32, torch.bfloat16, FP8]
IDS = ['fp32', 'bf16', 'fp8']
M, D, NV, NQ = 3, 64, 300, 70
WIDTHS = [1, 2, 33, 127, 128]   # 33: a second 32-row fragment with one live row; 127 / 128: all four waves, one short
LAMS = [0.0, 0.3, 0.7, 1.0]
ZERO_ITEM, ZERO_QUERY, ALL_NONE = 7, 5, 64   # an item with all-zero weights; an all-zero query; a row of -1 (row 0 of tile 2)
K_SUM = M * D                                # 192 products per pair
GAMMA = K_SUM * 2.0 ** -24 / (1 - K_SUM * 2.0 ** -24)
_cache = {}


def _data():
  """The gallery (300 items, rows 100 .. 139 and 250 .. 259 exact copies of row 100: equal relevances, and sim equal to the
  diagonal's; item 7 with all-zero weights: the 1e-5 denominator) and 70 queries, row 5 all zero."""
  if 'data' not in _cache:
    gen = torch.Generator(device=DEV).manual_seed(300)
    g, gw = torch.randn(NV, M, D, device=DEV, generator=gen), torch.rand(NV, M, device=DEV, generator=gen)
    q, qw = torch.randn(NQ, M, D, device=DEV, generator=gen), torch.rand(NQ, M, device=DEV, generator=gen)
    for lo, hi in ((100, 140), (250, 260)):
      g[lo:hi], gw[lo:hi] = g[100], gw[100]
    gw[ZERO_ITEM] = 0
    q[ZERO_QUERY] = 0
    _cache['data'] = g, gw, q, qw
  return _cache['data']


def _index(dtype):
  from mmt_amd.search import VideoIndex
  if dtype not in _cache:
    g, gw, _, _ = _data()
    _cache[dtype] = VideoIndex(g, gw, dtype=dtype)
  return _cache[dtype]


def _sharded(dtype):
  from mmt_amd.search import ShardedVideoIndex
  if ('sharded', dtype) not in _cache:
    g, gw, _, _ = _data()
    _cache['sharded', dtype] = ShardedVideoIndex(g, gw, [DEV] * 3, dtype=dtype)
    assert _cache['sharded', dtype].shard_sizes == [100, 100, 100]      # the copies of row 100 lie on two shards
  return _cache['sharded', dtype]


def _candidates(c):
  """int64 [70, C], drawn with replacement -- half of them from around the copies -- about a fifth of them -1; row 64 all
  -1, and the zero-weight item leads row 3."""
  if ('cand', c) not in _cache:
    gen = torch.Generator(device=DEV).manual_seed(c)
    near = torch.cat([torch.arange(90, 150, device=DEV), torch.arange(245, 265, device=DEV)])
    cand = torch.where(torch.rand(NQ, c, device=DEV, generator=gen) < 0.5,
                       near[torch.randint(0, near.numel(), (NQ, c), device=DEV, generator=gen)],
                       torch.randint(0, NV, (NQ, c), device=DEV, generator=gen))
    cand[torch.rand(NQ, c, device=DEV, generator=gen) < 0.2] = -1
    cand[ALL_NONE], cand[3, 0] = -1, ZERO_ITEM
    _cache['cand', c] = cand
  return _cache['cand', c]


def _definition(dtype):
  """sim of every pair of stored items in fp64, on the values read back from the index, and its tolerance: the worst-case
  bound of an fp32 sum of K exact products in any order, gamma_K * sum_k |f_g[k] f_h[k]| / |den|, plus 2^-22 * |value| for
  the scale multiply and the division.  Derived, not measured.  -> (value [NV, NV], tolerance [NV, NV]), float64."""
  if ('def', dtype) not in _cache:
    index = _index(dtype)
    f = index.folded[:NV].cpu().float().double().numpy()
    if index.scales is not None:
      f = f * index.scales[:NV].cpu().double().numpy()[:, None]
    w = index.weights[:NV].cpu().double().numpy()
    den = w @ w.T
    den[den == 0] = float(np.float32(1e-5))
    value = (f @ f.T) / den
    _cache['def', dtype] = value, GAMMA * (np.abs(f) @ np.abs(f).T) / np.abs(den) + 2.0 ** -22 * np.abs(value)
  return _cache['def', dtype]


def _bits(x):
  return x.view(torch.int32) if x.dtype is torch.float32 else x


def _same(a, b):
  return all(x.dtype == y.dtype and x.shape == y.shape and torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _permuted(sims, perm):
  c = perm.shape[1]
  return sims.gather(1, perm[:, :, None].expand(-1, -1, c)).gather(2, perm[:, None, :].expand(-1, c, -1))


@pytest.mark.parametrize('c', WIDTHS)
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_pair_scores_are_the_definition_on_the_stored_values(dtype, c):
  index, cand, (value, tol) = _index(dtype), _candidates(c), _definition(dtype)
  sims = index.pair_scores(cand)
  assert sims.dtype is torch.float32 and sims.shape == (NQ, c, c) and sims.device == DEV
  got, cd = sims.cpu().double().numpy(), cand.cpu().numpy()
  live = cd >= 0
  both, at = live[:, :, None] & live[:, None, :], np.maximum(cd, 0)
  want, allowed = value[at[:, :, None], at[:, None, :]], tol[at[:, :, None], at[:, None, :]]
  err = np.abs(got - want)[both]
  print('%s C = %d: max |error| %.3g, max error / tolerance %.3g over %d pairs' % (
      dtype, c, err.max(), (err / np.maximum(allowed[both], 1e-300)).max(), err.size))
  assert (err <= allowed[both]).all()
  assert np.isnan(got[~both]).all() and not np.isnan(got[both]).any() and np.isnan(got[ALL_NONE]).all()
  assert (got[3, 0][live[3]] == 0).all()                                    # the zero-weight item: 0 / 1e-5
  assert torch.equal(_bits(sims), _bits(sims.transpose(1, 2).contiguous()))  # sim(g, h) and sim(h, g): the same bits
  copies = torch.isin(cand, torch.cat([torch.arange(100, 140, device=DEV), torch.arange(250, 260, device=DEV)]))
  among = sims[copies[:, :, None] & copies[:, None, :]]
  diagonal = index.pair_scores(torch.tensor([[100]], device=DEV)).reshape(())
  assert among.numel() > 0 or c == 1
  assert torch.equal(_bits(among), _bits(diagonal.expand_as(among)))         # a copy is as like the original as itself
  # a pair's bits depend on nothing but the pair: not on its place, the rest of the list, the rows beside it
  gen = torch.Generator(device=DEV).manual_seed(c + 1)
  perm = torch.argsort(torch.rand(NQ, c, device=DEV, generator=gen), 1)
  assert torch.equal(_bits(index.pair_scores(torch.gather(cand, 1, perm))), _bits(_permuted(sims, perm)))
  for nq in (1, 65):
    assert torch.equal(_bits(index.pair_scores(cand[:nq])), _bits(sims[:nq]))
  if c > 1:
    assert torch.equal(_bits(index.pair_scores(cand[:, :c // 2])), _bits(sims[:, :c // 2, :c // 2]))
  assert torch.equal(_bits(index.pair_scores(cand)), _bits(sims))            # and again


def _staged(dtype, c):
  """The device's own first stage for all 70 rows, once: rescore(k=None) -- the distinct candidates in `search`'s order with
  `search`'s bits -- and the pair scores of that list, on the device and as numpy."""
  if ('staged', dtype, c) not in _cache:
    _, _, q, qw = _data()
    index = _index(dtype)
    rel, items = index.rescore(q, qw, _candidates(c))
    sims = index.pair_scores(items)
    _cache['staged', dtype, c] = (rel, items, sims), tuple(t.cpu().numpy() for t in (rel, items, sims))
  return _cache['staged', dtype, c]


def _restated(dtype, c, lam):
  """brute_mmr at the widest k = C for all rows, once per lam: greedy, so the selection at a smaller k is its first slots."""
  if ('mmr', dtype, c, lam) not in _cache:
    _, (rel, items, sims) = _staged(dtype, c)
    _cache['mmr', dtype, c, lam] = tuple(torch.from_numpy(t).to(DEV) for t in padded_mmr(rel, items, sims, c, *weights_of(lam)))
  return _cache['mmr', dtype, c, lam]


@pytest.mark.parametrize('c', WIDTHS)
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_diversify_is_the_rule_restated_in_numpy_bit_for_bit(dtype, c):
  _, _, q, qw = _data()
  index, cand = _index(dtype), _candidates(c)
  (rel, items, _), _ = _staged(dtype, c)
  assert rel.shape == items.shape == (NQ, c)
  for lam in LAMS:
    want = _restated(dtype, c, lam)
    assert (want[1][ALL_NONE] == -1).all() and torch.isneginf(want[2][ALL_NONE]).all()
    for nq, ks in ((NQ, (1, 10, c)), (65, (10,)), (1, (10,))):    # a second tile of rows with one live row; one row
      for k in ks:
        kp = min(k, c)
        got = index.diversify(q[:nq], qw[:nq], cand[:nq], k=k, lam=lam)
        assert [t.dtype for t in got] == [torch.float32, torch.int64, torch.float32]
        assert all(t.shape == (nq, kp) and t.device == DEV for t in got)
        assert torch.equal(got[1], want[1][:nq, :kp]), (lam, nq, k)
        assert torch.equal(_bits(got[0]), _bits(want[0][:nq, :kp])), (lam, nq, k)
        assert torch.equal(_bits(got[2]), _bits(want[2][:nq, :kp])), (lam, nq, k)
  if c >= 33:   # the penalty does something: at lam = 0.3 some row's list is not the list by relevance
    assert not torch.equal(_restated(dtype, c, 0.3)[1], items)


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_lam_one_is_rescore(dtype):
  _, _, q, qw = _data()
  index = _index(dtype)
  for c in WIDTHS:
    cand = _candidates(c)
    for k in (1, 10, c):
      scores, indices, values = index.diversify(q, qw, cand, k=k, lam=1.0)
      assert _same((scores, indices), index.rescore(q, qw, cand, k=min(k, 128))), (c, k)
      assert torch.equal(_bits(values), _bits(scores)), (c, k)
  assert _same(index.diversify(q, qw, _candidates(33), k=10, lam=1), index.diversify(q, qw, _candidates(33), k=10, lam=1.0))


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_neither_the_order_of_the_candidates_nor_the_row_batches_change_the_result(dtype, monkeypatch):
  from mmt_amd import search
  _, _, q, qw = _data()
  index = _index(dtype)
  for c in (2, 33, 128):
    cand = _candidates(c)
    want = index.diversify(q, qw, cand, k=10, lam=0.3)
    assert _same(index.diversify(q, qw, cand, k=10, lam=0.3), want), c       # two runs
    gen = torch.Generator(device=DEV).manual_seed(c + 2)
    perm = torch.argsort(torch.rand(NQ, c, device=DEV, generator=gen), 1)
    assert _same(index.diversify(q, qw, torch.gather(cand, 1, perm), k=10, lam=0.3), want), c
    assert _same(index.diversify(q, qw, cand.flip(1), k=10, lam=0.3), want), c
    sims = index.pair_scores(cand)
    with monkeypatch.context() as patch:
      assert index._list_batches(NQ, c) == [(0, NQ)]
      patch.setattr(search, '_BATCH_BYTES', 1)
      assert index._list_batches(NQ, c) == [(r, r + 1) for r in range(NQ)]
      assert _same(index.diversify(q, qw, cand, k=10, lam=0.3), want), c
      assert torch.equal(_bits(index.pair_scores(cand)), _bits(sims)), c


def _copies_gallery(dtype):
  """A, its copy A' and B, unlike both: sim(A, A') = 1 and sim(., B) = 0 exactly, on every dtype; the query likes A and A'
  equally (0.9) and B less (0.6).  Items 3 .. 7 are unlike everything and irrelevant."""
  from mmt_amd.search import VideoIndex
  g = torch.zeros(8, 1, 16, device=DEV)
  g[0, 0, 0], g[1, 0, 0], g[2, 0, 1] = 1, 1, 1
  for j in range(3, 8):
    g[j, 0, j] = 1
  q = torch.zeros(1, 1, 16, device=DEV)
  q[0, 0, 0], q[0, 0, 1] = 0.9, 0.6
  ones = torch.ones(8, 1, device=DEV)
  return VideoIndex(g, ones, dtype=dtype), q, ones[:1]


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_the_copies_gallery_worked_by_hand(dtype):
  index, q, qw = _copies_gallery(dtype)
  cand = torch.tensor([[2, 1, 0]], device=DEV)
  sims = index.pair_scores(torch.tensor([[0, 1, 2]], device=DEV))
  assert sims.tolist() == [[[1, 1, 0], [1, 1, 0], [0, 0, 1]]]
  scores, indices, values = index.diversify(q, qw, cand, k=3, lam=0.5)
  assert indices.tolist() == [[0, 2, 1]]                           # A, then B: 0.3 - 0 beats A' at 0.45 - 0.5
  rel = index.rescore(q, qw, cand)[0]
  assert torch.equal(_bits(scores), _bits(rel[:, [0, 2, 1]])) and values[0, 1] > values[0, 2] and values[0, 2] < 0
  scores, indices, values = index.diversify(q, qw, cand, k=3, lam=1.0)
  assert indices.tolist() == [[0, 1, 2]] and torch.equal(_bits(scores), _bits(rel)) and torch.equal(_bits(values), _bits(rel))
  three = index.subset(torch.tensor([0, 1, 2], device=DEV))
  assert index.search_diverse(q, qw, k=3, lam=0.5, subset=three)[1].tolist() == [[0, 2, 1]]
  assert index.search_diverse(q, qw, k=3, lam=1.0)[1].tolist() == [[0, 1, 2]]
  assert index.search_diverse(q, qw, k=2, lam=0.5, shortlist=3)[1].tolist() == [[0, 2]]
  # over the whole gallery an item unlike everything (0 - 0) comes before the copy (0.45 - 0.5)
  assert index.search_diverse(q, qw, k=4, lam=0.5)[1].tolist() == [[0, 2, 3, 4]]


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_search_diverse_is_the_search_then_diversify(dtype):
  _, _, q, qw = _data()
  index = _index(dtype)
  for k, shortlist, lam in ((10, 128, 0.5), (10, 50, 0.3), (40, 20, 0.7), (1, 1, 0.0)):
    want = index.diversify(q, qw, index.search(q, qw, k=shortlist)[1], k=k, lam=lam)
    got = index.search_diverse(q, qw, k=k, lam=lam, shortlist=shortlist)
    assert got[0].shape == (NQ, min(k, shortlist)) and _same(got, want), (k, shortlist)
  assert _same(index.search_diverse(q, qw), index.diversify(q, qw, index.search(q, qw, k=128)[1], k=10, lam=0.5))
  sub = index.subset(torch.arange(NV, device=DEV) % 3 != 1)
  few = index.subset(torch.tensor([3, 100, 101, 250], device=DEV))       # fewer allowed items than k: the list is 4 wide
  ex = torch.stack([torch.arange(NQ, device=DEV), torch.full((NQ,), -1, device=DEV)], 1)
  for kwargs in ({'subset': sub}, {'exclude': ex}, {'subset': sub, 'exclude': ex}, {'subset': few}, {'subset': few, 'exclude': ex}):
    shortlisted = index.search(q, qw, k=30, **kwargs)[1]
    got = index.search_diverse(q, qw, k=10, lam=0.3, shortlist=30, **kwargs)
    assert got[0].shape == (NQ, min(10, shortlisted.shape[1])), list(kwargs)
    assert _same(got, index.diversify(q, qw, shortlisted, k=10, lam=0.3)), list(kwargs)
  lost = index.search_diverse(q, qw, k=10, lam=0.3, shortlist=30, subset=few, exclude=ex)
  assert (lost[1][3] == -1).sum() == 1 and torch.isneginf(lost[2][3, -1])   # query 3 lost item 3: a vacant slot stays vacant
  if dtype is torch.float32:                                               # an fp8 index of the same items proposes
    coarse = _index(FP8)
    want = index.diversify(q, qw, coarse.search(q, qw, k=64)[1], k=10, lam=0.3)
    assert _same(index.search_diverse(q, qw, k=10, lam=0.3, shortlist=64, coarse=coarse), want)
    csub = coarse.subset(torch.arange(NV, device=DEV) % 3 != 1)
    want = index.diversify(q, qw, coarse.search(q, qw, k=64, subset=csub, exclude=ex)[1], k=10, lam=0.3)
    assert _same(index.search_diverse(q, qw, k=10, lam=0.3, shortlist=64, subset=csub, exclude=ex, coarse=coarse), want)
    assert not torch.equal(want[0], coarse.diversify(q, qw, coarse.search(q, qw, k=64, subset=csub, exclude=ex)[1], k=10, lam=0.3)[0])


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_sharded_equals_the_single_index_bit_for_bit(dtype):
  _, _, q, qw = _data()
  mono, shards = _index(dtype), _sharded(dtype)
  for c in (1, 33, 128):
    cand = _candidates(c)
    got = shards.pair_scores(cand)
    assert got.device == DEV and torch.equal(_bits(got), _bits(mono.pair_scores(cand))), c
    for nq, k, lam in ((NQ, 10, 0.3), (65, c, 0.7), (1, 1, 0.0)):
      got = shards.diversify(q[:nq], qw[:nq], cand[:nq], k=k, lam=lam)
      assert got[0].device == DEV and _same(got, mono.diversify(q[:nq], qw[:nq], cand[:nq], k=k, lam=lam)), (c, nq, k)
  assert _same(shards.search_diverse(q, qw, k=10, lam=0.3, shortlist=40), mono.search_diverse(q, qw, k=10, lam=0.3, shortlist=40))
  coarse = _sharded(FP8)
  assert _same(shards.search_diverse(q, qw, k=10, lam=0.3, shortlist=40, coarse=coarse),
               mono.search_diverse(q, qw, k=10, lam=0.3, shortlist=40, coarse=_index(FP8)))
  none = torch.full((2, 5), -1, device=DEV)
  assert torch.isnan(shards.pair_scores(none)).all() and torch.isnan(mono.pair_scores(none)).all()


@pytest.mark.parametrize('sharded', [False, True], ids=['VideoIndex', 'ShardedVideoIndex'])
def test_argument_errors_leave_the_index_usable(sharded):
  from mmt_amd.search import ShardedVideoIndex, VideoIndex
  _, _, q, qw = _data()
  index = _sharded(torch.float32) if sharded else _index(torch.float32)
  cand = _candidates(33)
  want = _index(torch.float32).diversify(q, qw, cand, k=10, lam=0.3)
  low, high = cand.clone(), cand.clone()
  low[69, 32], high[0, 0] = -2, NV
  for bad, text in ((cand.to(torch.int32), 'int64 tensor'), (cand.cpu(), 'index device'), (cand[:, 0], 'expected'),
                    (torch.cat([cand, cand[:1]]), '70 queries but candidates'),
                    (torch.zeros(NQ, 129, dtype=torch.int64, device=DEV), 'expected'),
                    (high, r'must lie in -1 \.\. 299, got -1 \.\. 300'), (low, r'must lie in -1 \.\. 299, got -2 \.\. ')):
    with pytest.raises(ValueError, match='diversify: .*' + text):
      index.diversify(q, qw, bad, k=10, lam=0.3)
    assert _same(index.diversify(q, qw, cand, k=10, lam=0.3), want)
  for bad in (high, low):
    with pytest.raises(ValueError, match='pair_scores: candidates must lie in'):
      index.pair_scores(bad)
  with pytest.raises(ValueError, match='lam must be'):
    index.diversify(q, qw, cand, lam=1.5)
  with pytest.raises(ValueError, match='norm= is out of scope'):
    index.search_diverse(q, qw, norm=None)
  empty = ShardedVideoIndex.empty(10, M, D, [DEV] * 2) if sharded else VideoIndex.empty(10, M, D, DEV)
  for call in (lambda: empty.diversify(q, qw, cand), lambda: empty.pair_scores(cand), lambda: empty.search_diverse(q, qw)):
    with pytest.raises(ValueError, match='holds no items'):
      call()
  got = index.diversify(q[:0], qw[:0], cand[:0], k=10)                    # no queries: empty lists
  assert all(t.shape == (0, 10) for t in got) and [t.dtype for t in got] == [torch.float32, torch.int64, torch.float32]
  assert index.pair_scores(cand[:0]).shape == (0, 33, 33)
  assert _same(index.diversify(q, qw, cand, k=10, lam=0.3), want)
