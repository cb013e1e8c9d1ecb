"""search.ShardedVideoIndex -- one gallery held as several VideoIndex shards -- and what it is built from
(mmt_search_merge_lists, VideoIndex.target_scores / threshold_counts over mmt_search_thresholds / mmt_search_count,
metric.retrieval_metrics_indexed(devices=)).  On one GPU the shards repeat cuda:0.

  1. the merge kernel alone against its numpy restatement (tests/test_index_sharded_cpu.py), indices and score bits;
  2. sharded equals monolithic, bit for bit: search, rank_counts and ranks, with subsets and exclusions, on shapes where a
     chunk spills, a shard holds one item, a shard crosses the 4096 edge and a shard is empty;
  3. lattice inputs against the fp64 brute force, exactly; 4. target_scores has the bits search returns and
     threshold_counts fed with it gives rank_counts; 5. the indexed metrics do not change with devices=;
  6. no buffer that grows with NQ * NV; 7. the error paths; 8. two devices, where there are two."""
import numpy as np
import pytest
import torch

from tests.test_index_ranks_gpu import _dev, _lattice, _random
from tests.test_index_sharded_cpu import merge_reference
from tests.test_index_subset_cpu import brute_topk
from tests.test_index_subset_gpu import LATTICE, _lattice_scores, _lattice_topk
from tests.test_search_gpu import _cuda

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
DTYPES = [torch.float32, torch.bfloat16]
INF = float('inf')


def _bits(x):
  return x.contiguous().view(torch.int32)


def _same(a, b):
  """Two (float32, int64) search results or two (int32, int32) count pairs: equal shapes, indices and bits."""
  return all(x.shape == y.shape and x.dtype == y.dtype and x.device == y.device for x, y in zip(a, b)) and all(
      torch.equal(_bits(x) if x.dtype == torch.float32 else x, _bits(y) if y.dtype == torch.float32 else y)
      for x, y in zip(a, b))


# ---- 1. the merge kernel ----------------------------------------------------------------------------------------------

def _merge(scores, index, tables, kout):
  from mmt_amd import _lib, ops
  n_lists, nq, kin = scores.shape
  scores_d, index_d = _cuda(scores), _cuda(index)
  tables_d = [_cuda(t) for t in tables]
  ids = torch.tensor([t.data_ptr() for t in tables_d], dtype=torch.int64).to(DEV)
  out_s = torch.full((nq, kout), 7.0, device=DEV, dtype=torch.float32)   # every slot must be written
  out_i = torch.full((nq, kout), -7, device=DEV, dtype=torch.int64)
  _lib.check(_lib.lib().mmt_search_merge_lists(ops._p(scores_d), ops._p(index_d), ops._p(ids), n_lists, nq, kin, kout,
                                               ops._p(out_s), ops._p(out_i), ops._stream()), 'mmt_search_merge_lists')
  torch.cuda.synchronize()
  return out_s.cpu().numpy(), out_i.cpu().numpy()


def _lists(rng, n_lists, nq, kin):
  """Random lists obeying the kernel's precondition: the global items are dealt to the shards at random (so the tables
  interleave), every list is a random handful of its shard's items with scores from a small set (many ties across lists,
  -0.0 and +0.0 among them), best first under (score descending, item ascending), the empty slots last.  Some lists are
  short, some empty, one query has nothing at all."""
  owner = rng.integers(0, n_lists, 40 * n_lists + 150)
  owner[:n_lists] = np.arange(n_lists)                    # no shard without items
  tables = [np.flatnonzero(owner == s).astype(np.int64) for s in range(n_lists)]
  values = np.float32([-INF, -1.5, -0.0, 0.0, 0.25, 0.25, 1.0, 3.0e38])
  scores = np.full((n_lists, nq, kin), -INF, np.float32)
  index = np.full((n_lists, nq, kin), -1, np.int64)
  for q in range(nq):
    if q == nq // 2 and nq > 1:
      continue                                            # a row with no candidate at all
    for s in range(n_lists):
      have = int(rng.choice([0, min(kin, tables[s].size), rng.integers(0, min(kin, tables[s].size) + 1)]))
      local = np.sort(rng.choice(tables[s].size, have, replace=False))
      sc = rng.choice(values, have)
      order = np.lexsort((local, -sc.astype(np.float64)))
      scores[s, q, :have], index[s, q, :have] = sc[order], local[order]
  return scores, index, tables


@pytest.mark.parametrize('nq', [1, 65])
@pytest.mark.parametrize('n_lists', [1, 2, 3, 32])
def test_merge_kernel_equals_its_restatement(n_lists, nq):
  rng = np.random.default_rng(100 * n_lists + nq)
  for kin in (1, 10, 128):
    scores, index, tables = _lists(rng, n_lists, nq, kin)
    for kout in (1, 10, 128):                             # kout > S * kin among them
      want_s, want_i = merge_reference(scores, index, tables, kout)
      got_s, got_i = _merge(scores, index, tables, kout)
      bad = (got_i != want_i).sum(), (got_s.view(np.int32) != want_s.view(np.int32)).sum()
      print('S=%d nq=%d kin=%d kout=%d: %d index, %d score-bit mismatches of %d' % (n_lists, nq, kin, kout, bad[0], bad[1],
                                                                                  want_i.size))
      assert np.array_equal(got_i, want_i), (kin, kout)
      assert np.array_equal(got_s.view(np.int32), want_s.view(np.int32)), (kin, kout)


def test_merge_kernel_on_full_lists_at_the_largest_footprint():
  """S = 32 lists of kin = 128 with every slot live (the lists above are short at that size: their shards hold about 45
  items): the whole 32 KiB of keys takes part in every binary search.  Few distinct scores, so most of the order is
  decided by global item numbers that interleave over the shards."""
  n_lists, nq, kin = 32, 3, 128
  rng = np.random.default_rng(7)
  owner = rng.permutation(np.arange(n_lists * 160) % n_lists)   # 160 items per shard, dealt at random
  tables = [np.flatnonzero(owner == s).astype(np.int64) for s in range(n_lists)]
  values = np.float32([-1.5, -0.0, 0.0, 0.25, 1.0, 3.0e38])
  scores = np.empty((n_lists, nq, kin), np.float32)
  index = np.empty((n_lists, nq, kin), np.int64)
  for q in range(nq):
    for s in range(n_lists):
      local = np.sort(rng.choice(160, kin, replace=False))
      sc = rng.choice(values, kin)
      order = np.lexsort((local, -sc.astype(np.float64)))
      scores[s, q], index[s, q] = sc[order], local[order]
  assert (index >= 0).all()
  for kout in (1, 10, 128):
    want_s, want_i = merge_reference(scores, index, tables, kout)
    got_s, got_i = _merge(scores, index, tables, kout)
    assert (want_i >= 0).all()
    assert np.array_equal(got_i, want_i), kout
    assert np.array_equal(got_s.view(np.int32), want_s.view(np.int32)), kout


def test_merge_kernel_keeps_the_sign_of_zero_and_orders_ties_by_global_item():
  """The hand-made lists of the CPU test: ties across lists whose items interleave, -0.0 beside +0.0, an empty row."""
  tables = [np.array([1, 4, 6]), np.array([0, 2, 3, 5]), np.array([7])]
  scores = np.float32([[[0.5, 0.5, 0.25], [0.5, 0.5, 0.5], [0.75, -INF, -INF]],
                       [[0.0, -1.0, -INF], [-0.0, -0.0, -INF], [-INF, -INF, -INF]],
                       [[-INF, -INF, -INF], [-INF, -INF, -INF], [-INF, -INF, -INF]]]).transpose(1, 0, 2)
  index = np.int64([[[0, 2, 1], [0, 1, 3], [0, -1, -1]],
                    [[1, 0, -1], [1, 3, -1], [-1, -1, -1]],
                    [[-1, -1, -1], [-1, -1, -1], [-1, -1, -1]]]).transpose(1, 0, 2)
  s, i = _merge(scores, index, tables, 8)
  assert i.tolist() == [[7, 0, 1, 2, 5, 6, 4, -1], [2, 4, 5, 1, -1, -1, -1, -1], [-1] * 8]
  assert s.view(np.int32)[1, :3].tolist() == np.float32([-0.0, 0.0, -0.0]).view(np.int32).tolist()
  want_s, want_i = merge_reference(scores, index, tables, 8)
  assert np.array_equal(i, want_i) and np.array_equal(s.view(np.int32), want_s.view(np.int32))


# ---- 2. sharded equals monolithic -------------------------------------------------------------------------------------

def _spilling(g, gw, dtype):
  from mmt_amd.search import ShardedVideoIndex
  index = ShardedVideoIndex.empty(700, g.shape[1], g.shape[2], [DEV] * 3, dtype=dtype)
  assert [sh.capacity for sh in index.shards] == [234] * 3
  assert index.add(g[:300], gw[:300]) == (0, 300)          # fills shard 0, the rest spills to shard 1
  assert index.shard_sizes == [234, 66, 0]
  assert index.add(g[300:429], gw[300:429]) == (300, 429)  # the emptiest shard
  assert index.add(g[429:], gw[429:]) == (429, 700)        # fills shard 1, the rest spills to shard 2
  assert index.shard_sizes == [234, 234, 232]
  return index


def _whole(n_shards):
  def build(g, gw, dtype):
    from mmt_amd.search import ShardedVideoIndex
    index = ShardedVideoIndex(g, gw, [DEV] * n_shards, dtype=dtype)
    nv = g.shape[0]
    assert index.shard_sizes == [nv // n_shards + (i < nv % n_shards) for i in range(n_shards)]
    return index
  return build


def _past_the_chunk_edge(g, gw, dtype):
  from mmt_amd.search import ShardedVideoIndex
  index = ShardedVideoIndex.empty(8400, g.shape[1], g.shape[2], ['cuda:0', 'cuda:0'], dtype=dtype)
  index.add(g[:4150], gw[:4150])                           # shard 0 alone: past item 4096 in its own numbers too
  index.add(g[4150:], gw[4150:])
  assert index.shard_sizes == [4150, 50]
  return index


# (nq, nv, M, d), how the sharded index is built
SHAPES = [((65, 700, 3, 8), _spilling), ((1, 3, 1, 8), _whole(3)), ((130, 4200, 2, 64), _past_the_chunk_edge),
          ((5, 2, 2, 8), _whole(3))]


def _masks(index):
  """name -> bool [nv] on the device, the empty ones dropped."""
  nv = index.num_items
  every = torch.arange(nv, device=DEV)
  out = {'every_other': every % 2 == 1, 'one_item': every == nv // 2, 'without_shard_0': index._shard_of[:nv] != 0,
         'without_tile_1': (every < 128) | (every >= 256)}
  return {n: m for n, m in out.items() if bool(m.any()) and (n == 'one_item' or not bool(m.all()))}


@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16'])
@pytest.mark.parametrize('shape,build', SHAPES, ids=['x'.join(map(str, s)) for s, _ in SHAPES])
def test_sharded_equals_monolithic_bit_for_bit(shape, build, dtype):
  """Not to be loosened: score(q, g) does not depend on where item g is stored (search_scan.h), so a mismatch here is a
  finding about the scoring tile, not noise."""
  from mmt_amd.search import VideoIndex
  nq, nv, m, d = shape
  q, qw, g, gw = _random(nq, nv, m, d, nq + nv + m + d)
  for twin in (nv // 2, nv - 1):                            # copies of item 0 on other shards: ties across shards
    g[twin], gw[twin] = g[0], gw[0]
  if nq > 2:
    qw[nq // 2] = 0                                          # every score 0: one tie over all shards
  mono = VideoIndex(g, gw, dtype=dtype)
  shard = build(g, gw, dtype)
  assert (shard.num_items, shard.dtype, shard.device, shard.devices[0]) == (nv, dtype, DEV, DEV)
  owners = shard._shard_of[:nv].cpu().numpy()
  assert len(set(owners[[0, nv // 2, nv - 1]].tolist())) > 1 or nv < 3
  for s, sh in enumerate(shard.shards):                      # the tables are increasing and partition the items
    assert np.array_equal(sh.ids[:sh.num_items].cpu().numpy(), np.flatnonzero(owners == s))
  subsets = {None: (None, None)}
  for name, mask in _masks(shard).items():
    subsets[name] = (mono.subset(mask), shard.subset(mask))
    assert subsets[name][1].count == subsets[name][0].count == int(mask.sum()) and subsets[name][1].num_items == nv
  top = mono.search(q, qw, k=min(nv, 32))[1]
  barred = torch.cat([top, top.new_full((nq, 32 - top.shape[1]), -1)], 1)   # the 32 best; every item where nv <= 32
  excludes = {None: None, 'E1': top[:, 0].contiguous(), 'E32': barred}
  for name, (sub_m, sub_s) in subsets.items():
    for ex_name, ex in excludes.items():
      for k in (1, 10, 128):
        want = mono.search(q, qw, k=k, subset=sub_m, exclude=ex)
        got = shard.search(q, qw, k=k, subset=sub_s, exclude=ex)
        assert _same(got, want), (name, ex_name, k)
  if 'one_item' in subsets:                                  # every candidate of every query barred
    only = torch.full((nq, 1), nv // 2, device=DEV, dtype=torch.int64)
    got = shard.search(q, qw, k=10, subset=subsets['one_item'][1], exclude=only)
    assert _same(got, mono.search(q, qw, k=10, subset=subsets['one_item'][0], exclude=only))
    assert got[0].shape == (nq, 1) and bool((got[1] == -1).all()) and bool(torch.isneginf(got[0]).all())
  crossing = 0
  for t in (1, 3, 33):
    tg = torch.randint(-1, nv, (nq, t), device=DEV, generator=torch.Generator(device=DEV).manual_seed(t))
    tg[0, 0] = 0                                             # an item with twins elsewhere
    if t > 1:
      tg[:, 1] = nv - 1
      tg[nq - 1, 0] = -1
    for name, (sub_m, sub_s) in subsets.items():
      want = mono.rank_counts(q, qw, tg, subset=sub_m)
      got = shard.rank_counts(q, qw, tg, subset=sub_s)
      assert _same(got, want), (name, t)
      assert torch.equal(shard.ranks(q, qw, tg, subset=sub_s), mono.ranks(q, qw, tg, subset=sub_m)), (name, t)
      if name is None:
        crossing += int((got[1] > 1).sum())
    one = shard.ranks(q, qw, tg[:, 0].contiguous())
    assert one.shape == (nq,) and torch.equal(one, mono.ranks(q, qw, tg[:, 0].contiguous()))
  assert crossing > 0 or nv < 3                              # ties that span shards were counted


# ---- 3. lattice inputs against the fp64 brute force -------------------------------------------------------------------

@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16'])
@pytest.mark.parametrize('case', [2, 3], ids=['x'.join(map(str, LATTICE[c])) for c in (2, 3)])
def test_three_shards_are_exact_on_lattice_inputs(case, dtype):
  from mmt_amd.search import ShardedVideoIndex
  nq, nv, m, d, t = LATTICE[case]
  assert LATTICE[case] in ((65, 129, 2, 8, 3), (130, 8193, 3, 64, 33))
  q, qw, g, gw, tg, greater, equal = _lattice(*LATTICE[case])
  index = ShardedVideoIndex(_dev(g), _dev(gw), [DEV] * 3, dtype=dtype)
  q, qw = _dev(q), _dev(qw)
  want_s, want_i = _lattice_topk(case, 'all')
  for k in (1, 10, 128):
    s, i = index.search(q, qw, k=k)
    assert np.array_equal(i.cpu().numpy(), want_i[:, :k]) and np.array_equal(s.cpu().numpy(), want_s[:, :k]), k
  got_g, got_e = (x.cpu().numpy() for x in index.rank_counts(q, qw, _dev(tg)))
  print('mismatches: greater %d, equal %d of %d' % ((got_g != greater).sum(), (got_e != equal).sum(), tg.size))
  assert np.array_equal(got_g, greater) and np.array_equal(got_e, equal)
  ranks = index.ranks(q, qw, _dev(tg)).cpu().numpy()
  assert np.array_equal(ranks, np.where(tg >= 0, greater + (equal - 1) / 2, INF))
  # a subset and exclusions against the brute force as well
  mask = np.arange(nv) % 2 == 1
  ex = want_i[:, :3].copy()
  want = brute_topk(_lattice_scores(case), mask, ex, 10)
  s, i = index.search(q, qw, k=10, subset=index.subset(_cuda(mask)), exclude=_cuda(ex))
  assert np.array_equal(i.cpu().numpy(), want[1]) and np.array_equal(s.cpu().numpy(), want[0])


# ---- 4. the two halves of rank_counts ---------------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16'])
@pytest.mark.parametrize('nq,nv,m,d', [(65, 100, 3, 8), (130, 77, 7, 64), (5, 1, 1, 8)])
def test_target_scores_have_the_bits_search_returns(nq, nv, m, d, dtype):
  from mmt_amd.search import VideoIndex
  q, qw, g, gw = _random(nq, nv, m, d, nq + nv + m + d)
  qw[nq // 2] = 0
  index = VideoIndex(g, gw, dtype=dtype)
  s, i = index.search(q, qw, k=128)                          # nv <= 128: every score of the scan
  by_item = torch.empty_like(s).scatter_(1, i, s)            # by_item[q, g] = score(q, g)
  rng = np.random.default_rng(nv)
  tg = _cuda(np.concatenate([np.arange(nv)[None].repeat(nq, 0)[:, :40], rng.integers(-1, nv, (nq, 3))], 1))   # T up to 43
  got = index.target_scores(q, qw, tg)
  assert got.shape == tg.shape and got.dtype == torch.float32 and got.device == DEV
  none = tg < 0
  assert bool(torch.isnan(got[none]).all()) and not bool(torch.isnan(got[~none]).any())
  want = by_item.gather(1, tg.clamp(min=0))
  assert torch.equal(_bits(got)[~none], _bits(want)[~none])
  one = index.target_scores(q, qw, tg[:, 0].contiguous())
  assert one.shape == (nq,) and torch.equal(_bits(one), _bits(got[:, 0]))
  want_counts = index.rank_counts(q, qw, tg)
  assert _same(index.threshold_counts(q, qw, got), want_counts)
  assert not bool(want_counts[0][none].any()) and not bool(want_counts[1][none].any())
  sub = index.subset(torch.arange(nv, device=DEV) % 2 == 0)
  assert _same(index.threshold_counts(q, qw, got, subset=sub), index.rank_counts(q, qw, tg, subset=sub))
  assert _same(index.threshold_counts(q, qw, got[:, 0].contiguous()), index.rank_counts(q, qw, tg[:, 0].contiguous()))
  # any value is a threshold: +inf has nothing above it, -inf everything that is not -inf itself
  ends = torch.tensor([[INF, -INF]], device=DEV).repeat(nq, 1)
  greater, equal = index.threshold_counts(q, qw, ends)
  assert bool((greater[:, 0] == 0).all()) and bool((greater[:, 1] == nv).all()) and not bool(equal.any())
  with pytest.raises(ValueError, match='targets must lie'):
    index.target_scores(q, qw, torch.full((nq,), nv, device=DEV, dtype=torch.int64))
  with pytest.raises(ValueError, match='float32'):
    index.threshold_counts(q, qw, tg)


# ---- 5. the indexed metrics -------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16'])
def test_indexed_metrics_do_not_change_with_devices(dtype):
  from mmt_amd.metric import retrieval_metrics_indexed
  b, c, m, d = 70, 3, 2, 8
  txt, tw, vid, vw = (np.array(x) for x in _lattice(b * c, b, m, d, 1)[:4])   # the shape of the existing indexed-metrics test
  text4 = np.ascontiguousarray(txt.reshape(b, c, m, d).transpose(0, 2, 1, 3))
  tw3 = tw.reshape(b, c, m)
  rng = np.random.default_rng(5)
  qm = (rng.random((b, c)) < 0.6).astype(np.float32)
  qm[:, 0] = 1
  qm[[4, 69]] = 0
  cut = rng.random(b) < 0.4
  cut[[0, 4, 64, 65]] = True
  for kwargs in ({}, {'query_masks': qm}, {'video_subset': cut}, {'query_masks': qm, 'video_subset': cut}):
    want = retrieval_metrics_indexed(vid, text4, vw, tw3, dtype=dtype, **kwargs)
    got = retrieval_metrics_indexed(vid, text4, vw, tw3, dtype=dtype, devices=[DEV, 'cuda:0', DEV], **kwargs)
    assert set(got) == set(want) == {'t2v_metrics', 'v2t_metrics'}
    for name in want:
      assert set(got[name]) == set(want[name])
      assert np.array_equal(got[name]['cols'], want[name]['cols']), (name, sorted(kwargs))
      for key in want[name]:
        if key != 'cols':
          assert got[name][key] == want[name][key], (name, key)


# ---- 6. memory --------------------------------------------------------------------------------------------------------

def test_sharded_scans_allocate_no_quadratic_buffer():
  """The bound of tests/test_index_subset_gpu.py: the matrix alone would be 1 GiB."""
  from mmt_amd.search import ShardedVideoIndex
  nq, nv, m, d = 2048, 131072, 7, 512
  gen = torch.Generator(device=DEV).manual_seed(5)
  index = ShardedVideoIndex.empty(nv, m, d, [DEV] * 4)
  for at in range(0, nv, 16384):
    index.add(torch.rand(16384, m, d, device=DEV, generator=gen) - 0.5, torch.rand(16384, m, device=DEV, generator=gen))
  assert index.shard_sizes == [nv // 4] * 4 and index.num_items == index.capacity == nv
  q = torch.rand(nq, m, d, device=DEV, generator=gen) - 0.5
  qw = torch.rand(nq, m, device=DEV, generator=gen)
  tg = torch.randint(0, nv, (nq,), device=DEV, generator=gen)
  allowed = torch.rand(nv, device=DEV, generator=gen) < 0.5
  torch.cuda.synchronize()
  base = torch.cuda.memory_allocated()
  torch.cuda.reset_peak_memory_stats()
  sub = index.subset(allowed)
  s, i = index.search(q, qw, k=10, subset=sub, exclude=tg)
  ranks = index.ranks(q, qw, tg, subset=sub)
  torch.cuda.synchronize()
  growth = torch.cuda.max_memory_allocated() - base
  print('allocator peak growth %.1f MiB' % (growth / 2 ** 20))
  assert growth < 64 << 20, growth
  assert sub.count == int(allowed.sum())
  assert bool(allowed[i].all()) and not bool((i == tg[:, None]).any()) and bool((s[:, 1:] <= s[:, :-1]).all())
  assert bool(((ranks >= 0) & (ranks < sub.count))[allowed[tg]].all()) and bool(torch.isinf(ranks[~allowed[tg]]).all())
  again = index.search(q, qw, k=10, subset=sub, exclude=tg)
  assert torch.equal(s, again[0]) and torch.equal(i, again[1]) and torch.equal(ranks, index.ranks(q, qw, tg, subset=sub))


# ---- 7. errors --------------------------------------------------------------------------------------------------------

def test_error_paths():
  from mmt_amd.search import ShardedVideoIndex, VideoIndex
  q, qw, g, gw = _random(3, 10, 2, 8, 1)
  for bad in (['cpu'], [DEV, 'cpu'], [], [DEV] * 33, DEV):
    with pytest.raises(ValueError, match='devices'):
      ShardedVideoIndex(g, gw, bad)
    with pytest.raises(ValueError, match='devices'):
      ShardedVideoIndex.empty(10, 2, 8, bad)
  with pytest.raises(ValueError, match='dtype'):
    ShardedVideoIndex(g, gw, [DEV], dtype=torch.float16)
  index = ShardedVideoIndex.empty(12, 2, 8, [DEV] * 3)
  with pytest.raises(ValueError, match='holds no items'):
    index.search(q, qw)
  index.add(g, gw)
  tg = torch.zeros(3, device=DEV, dtype=torch.int64)
  for call in (lambda: index.search(q.cpu(), qw.cpu()), lambda: index.rank_counts(q.cpu(), qw.cpu(), tg)):
    with pytest.raises(ValueError, match='CUDA tensor'):    # queries off the primary
      call()
  with pytest.raises(ValueError, match='index device'):
    index.rank_counts(q, qw, tg.cpu())
  with pytest.raises(ValueError, match='index device'):
    index.search(q, qw, exclude=tg.cpu())
  with pytest.raises(ValueError, match='index device'):
    index.subset(torch.ones(10, dtype=torch.bool))
  with pytest.raises(ValueError, match='k must be'):
    index.search(q, qw, k=129)
  for bad in (-2, 10):
    with pytest.raises(ValueError, match='exclude must lie'):
      index.search(q, qw, exclude=torch.full((3,), bad, device=DEV, dtype=torch.int64))
    with pytest.raises(ValueError, match='targets must lie'):
      index.ranks(q, qw, torch.full((3,), bad, device=DEV, dtype=torch.int64))
  with pytest.raises(ValueError, match='ShardedVideoIndex.subset'):   # a single index's subset is not this one's
    index.search(q, qw, subset=VideoIndex(g, gw).subset(torch.ones(10, device=DEV, dtype=torch.bool)))
  # an add that does not fit changes nothing
  before = index.shard_sizes
  assert before == [4, 4, 2] and index.capacity == 12
  want = index.search(q, qw, k=10)
  with pytest.raises(ValueError, match='do not fit'):
    index.add(g[:3], gw[:3])
  assert index.num_items == 10 and index.shard_sizes == before and _same(index.search(q, qw, k=10), want)
  # a subset from before an add is refused
  old = index.subset(torch.ones(10, device=DEV, dtype=torch.bool))
  assert index.add(g[:2], gw[:2]) == (10, 12) and index.shard_sizes == [4, 4, 4]
  for call in (lambda: index.search(q, qw, subset=old), lambda: index.rank_counts(q, qw, tg, subset=old),
               lambda: index.ranks(q, qw, tg, subset=old)):
    with pytest.raises(ValueError, match='built for 10 items'):
      call()
  assert index.nbytes > 12 * 2 * 8 * 4


# ---- 8. two devices ---------------------------------------------------------------------------------------------------

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
  assert [sh.index.folded.device.index for sh in index.shards] == [0, 1] and index.shard_sizes == [350, 350]
  assert all(sh.ids.device == DEV for sh in index.shards)  # the tables the merge kernel follows are all on the primary
  tg = torch.randint(-1, nv, (nq, 3), device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))
  tg[0, 0] = 0
  mask = torch.arange(nv, device=DEV) % 2 == 1
  for sub_m, sub_s in ((None, None), (mono.subset(mask), index.subset(mask))):
    for k in (1, 10, 128):
      got = index.search(q, qw, k=k, subset=sub_s, exclude=tg[:, 0].contiguous())
      assert got[0].device == DEV and _same(got, mono.search(q, qw, k=k, subset=sub_m, exclude=tg[:, 0].contiguous()))
    assert _same(index.rank_counts(q, qw, tg, subset=sub_s), mono.rank_counts(q, qw, tg, subset=sub_m))
    assert torch.equal(index.ranks(q, qw, tg, subset=sub_s), mono.ranks(q, qw, tg, subset=sub_m))
  # queries, targets and exclusions are given on the primary: another CUDA device is refused like the host
  other = torch.device('cuda', 1)
  for call in (lambda: index.search(q.to(other), qw.to(other)), lambda: index.rank_counts(q.to(other), qw.to(other), tg),
               lambda: index.rank_counts(q, qw, tg.to(other)), lambda: index.search(q, qw, exclude=tg[:, 0].to(other))):
    with pytest.raises(ValueError, match='must be on the index device'):
      call()
