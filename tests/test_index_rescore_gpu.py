"""VideoIndex.rescore (mmt_search_rescore and its bf16 / fp8 forms) and search_refined on the GPU.  Every claim is one of
bit identity: per query the distinct non-negative candidates, ranked under `search`'s order, with the score bits
`target_scores` -- the threshold pass the call generalises -- gives the pair on the same index.  The reference is that
call for the bits and tests.test_index_rescore_cpu.brute_rescore for the list; results are compared with torch.equal on
the indices and on the int32 views of the scores."""
import numpy as np
import pytest
import torch

from tests.test_index_rescore_cpu import padded_rescore

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
FP8 = torch.float8_e4m3fn
DTYPES = [torch.float32, torch.bfloat16, FP8]
IDS = ['fp32', 'bf16', 'fp8']
M, D, NV, NQ = 3, 64, 777, 130
WIDTHS = [1, 3, 32, 33, 128, 129, 1000, 1024]   # 3: a query's pairs straddle a 128-pair tile; 33: past MAX_T; 129, 1000: no powers of two
ALL_NONE, ONE_ITEM = 64, 5                      # rows of every candidate list: all -1 (the one live row of the second query
                                                # tile at NQ = 65), and one item C times
_cache = {}


def _data():
  """The gallery (777 items, rows 100 .. 139 and 500 .. 519 exact copies of row 100: ties, also across shards) and 130
  queries, row 7 all zero."""
  if 'data' not in _cache:
    gen = torch.Generator(device=DEV).manual_seed(777)
    g, gw = torch.randn(NV, M, D, device=DEV, generator=gen), torch.rand(NV, M, device=DEV, generator=gen)
    q, qw = torch.randn(NQ, M, D, device=DEV, generator=gen), torch.rand(NQ, M, device=DEV, generator=gen)
    for lo, hi in ((100, 140), (500, 520)):
      g[lo:hi], gw[lo:hi] = g[100], gw[100]
    q[7] = 0
    _cache['data'] = g, gw, q, qw
  return _cache['data']


def _index(dtype):
  from mmt_amd.search import VideoIndex
  if dtype not in _cache:
    g, gw, _, _ = _data()
    _cache[dtype] = VideoIndex(g, gw, dtype=dtype)
  return _cache[dtype]


def _candidates(c):
  """int64 [130, C], drawn with replacement -- half of them from around the tied rows -- about a fifth of them -1."""
  if ('cand', c) not in _cache:
    gen = torch.Generator(device=DEV).manual_seed(c)
    near = torch.cat([torch.arange(90, 150, device=DEV), torch.arange(495, 525, device=DEV)])
    cand = torch.where(torch.rand(NQ, c, device=DEV, generator=gen) < 0.5,
                       near[torch.randint(0, near.numel(), (NQ, c), device=DEV, generator=gen)],
                       torch.randint(0, NV, (NQ, c), device=DEV, generator=gen))
    cand[torch.rand(NQ, c, device=DEV, generator=gen) < 0.2] = -1
    cand[ALL_NONE], cand[ONE_ITEM] = -1, 123
    _cache['cand', c] = cand
  return _cache['cand', c]


def _reference(dtype, c):
  """The definition at the widest k' = min(C, 128) for all 130 rows, computed once: the bits of `target_scores`, the list of
  brute_rescore.  The best k of a row are the first k of its best 128."""
  if ('ref', dtype, c) not in _cache:
    _, _, q, qw = _data()
    cand = _candidates(c)
    bits = _index(dtype).target_scores(q, qw, cand)
    s, i = padded_rescore(bits.cpu().numpy(), cand.cpu().numpy(), min(c, 128))
    _cache['ref', dtype, c] = torch.from_numpy(s).to(DEV), torch.from_numpy(i).to(DEV)
  return _cache['ref', dtype, c]


def _same(a, b):
  return all(x.dtype == y.dtype and x.shape == y.shape and
             torch.equal(x.view(torch.int32) if x.dtype is torch.float32 else x, y.view(torch.int32) if y.dtype is torch.float32 else y)
             for x, y in zip(a, b))


@pytest.mark.parametrize('c', WIDTHS)
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_rescore_is_the_definition_on_the_bits_of_target_scores(dtype, c):
  _, _, q, qw = _data()
  index, cand, (ws, wi) = _index(dtype), _candidates(c), _reference(dtype, c)
  assert (wi[ALL_NONE] == -1).all() and wi[ONE_ITEM].tolist() == [123] + [-1] * (min(c, 128) - 1)
  for nq in (1, 65, 130):       # a second query tile with one live row, a third with two
    for k in (None, 1, 10, 128):
      kp = min(c, 128 if k is None else k)
      s, i = index.rescore(q[:nq], qw[:nq], cand[:nq], k=k)
      assert s.dtype is torch.float32 and i.dtype is torch.int64 and s.shape == i.shape == (nq, kp) and s.device == DEV
      assert torch.equal(i, wi[:nq, :kp]), (nq, k)
      assert torch.equal(s.view(torch.int32), ws[:nq, :kp].view(torch.int32)), (nq, k)
  assert _same(index.rescore(q, qw, cand, k=10), index.rescore(q, qw, cand, k=10))      # and again


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_a_row_is_the_search_of_its_candidates_as_a_subset(dtype):
  _, _, q, qw = _data()
  index, cand = _index(dtype), _candidates(129)
  s, i = index.rescore(q, qw, cand, k=128)
  for r in (0, 7, ONE_ITEM):
    mine = cand[r][cand[r] >= 0]
    distinct = int(torch.unique(mine).numel())
    ss, si = index.search(q[r:r + 1], qw[r:r + 1], k=128, subset=index.subset(mine))
    assert ss.shape == (1, distinct) and distinct < 128
    assert torch.equal(i[r, :distinct], si[0]) and torch.equal(s[r, :distinct].view(torch.int32), ss[0].view(torch.int32))
    assert (i[r, distinct:] == -1).all() and torch.isneginf(s[r, distinct:]).all()


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_neither_the_order_of_the_candidates_nor_the_row_batches_change_the_result(dtype, monkeypatch):
  from mmt_amd import search
  _, _, q, qw = _data()
  index = _index(dtype)
  for c in (3, 129, 1024):
    cand = _candidates(c)
    want = index.rescore(q, qw, cand)
    gen = torch.Generator(device=DEV).manual_seed(c + 1)
    perm = torch.argsort(torch.rand(NQ, c, device=DEV, generator=gen), 1)
    assert _same(index.rescore(q, qw, torch.gather(cand, 1, perm)), want), c
    assert _same(index.rescore(q, qw, cand.flip(1)), want), c
    with monkeypatch.context() as patch:
      assert len(index._row_batches(NQ, 8 * c)) == 1
      patch.setattr(search, '_BATCH_BYTES', 1)
      assert index._row_batches(NQ, 8 * c) == [(0, 64), (64, 128), (128, 130)]
      assert _same(index.rescore(q, qw, cand), want), c


def _three_shards(g, gw, dtype):
  from mmt_amd.search import ShardedVideoIndex
  index = ShardedVideoIndex(g, gw, [DEV] * 3, dtype=dtype)
  assert index.shard_sizes == [259, 259, 259]
  return index


def _three_shards_one_empty(g, gw, dtype):
  from mmt_amd.search import ShardedVideoIndex
  index = ShardedVideoIndex.empty(1200, M, D, [DEV] * 3, dtype=dtype)
  assert index.add(g, gw) == (0, NV)
  assert index.shard_sizes == [400, 377, 0]      # one piece that spills once; the last shard stays empty
  return index


@pytest.mark.parametrize('build', [_three_shards, _three_shards_one_empty], ids=['3', '3_one_empty'])
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_sharded_equals_the_single_index_bit_for_bit(dtype, build):
  g, gw, q, qw = _data()
  mono, shards = _index(dtype), build(g, gw, dtype)
  assert shards.num_items == NV
  for c in (1, 3, 129, 1024):
    cand = _candidates(c)
    for nq, k in ((130, None), (65, 10), (1, 1)):
      got = shards.rescore(q[:nq], qw[:nq], cand[:nq], k=k)
      assert got[0].device == DEV and _same(got, mono.rescore(q[:nq], qw[:nq], cand[:nq], k=k)), (c, nq, k)
  fine = shards.search_refined(q, qw, _index(FP8), k=10, shortlist=64)
  assert _same(fine, mono.search_refined(q, qw, _index(FP8), k=10, shortlist=64))


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_the_list_of_search_comes_back_as_it_is(dtype):
  """The same index: the scan's bits come back through the gather, in the scan's order."""
  _, _, q, qw = _data()
  index = _index(dtype)
  want = index.search(q, qw, k=128)
  assert _same(index.rescore(q, qw, want[1]), want)
  assert _same(index.rescore(q, qw, want[1].flip(1), k=10), (want[0][:, :10], want[1][:, :10]))


@pytest.mark.parametrize('dtype', DTYPES[:2], ids=IDS[:2])
def test_search_refined_is_the_coarse_search_then_rescore(dtype):
  from mmt_amd.search import VideoIndex
  g, gw, q, qw = _data()
  fine, coarse = _index(dtype), _index(FP8)
  for k, shortlist in ((10, 128), (10, 50), (40, 20), (1, 1)):
    want = fine.rescore(q, qw, coarse.search(q, qw, k=shortlist)[1], k)
    got = fine.search_refined(q, qw, coarse, k=k, shortlist=shortlist)
    assert got[0].shape == (NQ, min(k, shortlist)) and _same(got, want), (k, shortlist)
  assert _same(fine.search_refined(q, qw, coarse), fine.rescore(q, qw, coarse.search(q, qw, k=128)[1], 10))
  sub = coarse.subset(torch.arange(NV, device=DEV) % 3 != 1)
  few = coarse.subset(torch.tensor([3, 100, 101, 700], device=DEV))       # fewer allowed items than k: the list is 4 wide
  ex = torch.stack([torch.arange(NQ, device=DEV), torch.full((NQ,), -1, device=DEV)], 1)
  for kwargs in ({'subset': sub}, {'exclude': ex}, {'subset': sub, 'exclude': ex}, {'subset': few}, {'subset': few, 'exclude': ex}):
    shortlisted = coarse.search(q, qw, k=30, **kwargs)[1]
    got = fine.search_refined(q, qw, coarse, k=10, shortlist=30, **kwargs)
    assert got[0].shape == (NQ, min(10, shortlisted.shape[1])) and _same(got, fine.rescore(q, qw, shortlisted, 10)), list(kwargs)
  assert (fine.search_refined(q, qw, coarse, k=10, shortlist=30, subset=few, exclude=ex)[1][3] == torch.tensor(
      [-1], device=DEV)).sum() == 1                                      # query 3 lost item 3: a vacant slot stays vacant
  # a coarse index that cannot hold the same items, before anything is scored
  for other in (VideoIndex(g[:NV - 1], gw[:NV - 1], dtype=FP8), VideoIndex(g[:, :, :32], gw, dtype=FP8),
                VideoIndex(g[:, :2], gw[:, :2], dtype=FP8)):
    with pytest.raises(ValueError, match='the coarse index holds'):
      fine.search_refined(q, qw, other)
  elsewhere = VideoIndex(g[:8], gw[:8], dtype=FP8)
  elsewhere.num_items, elsewhere.device = NV, torch.device('cuda', 1)    # only its label is looked at: the check comes first
  with pytest.raises(ValueError, match='the coarse index is on cuda:1'):
    fine.search_refined(q, qw, elsewhere)
  for bad in (0, 129):
    with pytest.raises(ValueError, match='shortlist must be an int'):
      fine.search_refined(q, qw, coarse, shortlist=bad)
  with pytest.raises(ValueError, match='subset must come from'):
    fine.search_refined(q, qw, coarse, subset=torch.ones(NV, dtype=torch.bool, device=DEV))


@pytest.mark.parametrize('sharded', [False, True], ids=['VideoIndex', 'ShardedVideoIndex'])
def test_argument_errors_leave_the_index_usable(sharded):
  from mmt_amd.search import ShardedVideoIndex, VideoIndex
  g, gw, q, qw = _data()
  index = ShardedVideoIndex(g, gw, [DEV] * 2) if sharded else _index(torch.float32)
  cand = _candidates(32)
  want = _index(torch.float32).rescore(q, qw, cand, k=10)
  low, high = cand.clone(), cand.clone()
  low[129, 31], high[0, 0] = -2, NV
  for bad, text in ((cand.to(torch.int32), 'int64 tensor'), (cand.cpu(), 'index device'), (cand[:, 0], 'expected'),
                    (torch.cat([cand, cand[:1]]), '130 queries but candidates'),
                    (torch.zeros(NQ, 1025, dtype=torch.int64, device=DEV), 'expected'),
                    (high, r'must lie in -1 \.\. 776, got -1 \.\. 777'), (low, r'must lie in -1 \.\. 776, got -2 \.\. ')):
    with pytest.raises(ValueError, match=text):
      index.rescore(q, qw, bad)
    assert _same(index.rescore(q, qw, cand, k=10), want)
  for bad in (0, 129, True):
    with pytest.raises(ValueError, match='k must be None or an int'):
      index.rescore(q, qw, cand, k=bad)
  empty = ShardedVideoIndex.empty(10, M, D, [DEV] * 2) if sharded else VideoIndex.empty(10, M, D, DEV)
  with pytest.raises(ValueError, match='holds no items'):
    empty.rescore(q, qw, cand)
  s, i = index.rescore(q[:0], qw[:0], cand[:0], k=10)                    # no queries: empty lists
  assert s.shape == i.shape == (0, 10) and s.dtype is torch.float32 and i.dtype is torch.int64
  assert _same(index.rescore(q, qw, cand, k=10), want)
