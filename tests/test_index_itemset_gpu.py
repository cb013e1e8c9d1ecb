"""Item-set pooling of VideoIndex / ShardedVideoIndex (item_pooling= of search, rank_counts, ranks, target_scores and
threshold_counts; mmt_search_topk_itemsets, mmt_search_thresholds_itemsets, mmt_search_count_itemsets and their bf16
forms): the STORED items are sets of C consecutive items and every scan answers per set, on the mean or the max of the
set's scores.  The definition is tests/test_index_pooled_cpu.py::brute_pooled applied to the transposed score matrix.

  1. lattice inputs with power-of-two weights, where fp32, bf16 and fp64 agree bit for bit and ties abound: score bits,
     set numbers and counts equal brute force on the fp64 pooled matrix, for both modes;
  2. random inputs and arbitrary weights: equal to brute_pooled of the scan's own score matrix (target_scores over every
     item, unpooled), bit for bit -- an fma or a reordered sum shows here;
  3. consistent with the plain scans (sets of one), the text layout, subsets of sets, query batches;
  4. sharded equals monolithic;  5. the reference's 'avg' similarities of the golden file and the 'avg' metrics;
  6. no buffer that grows with NQ * num_items."""
import functools

import numpy as np
import pytest
import torch

from tests.fixtures import load_npz
from tests.test_index_groups_cpu import best_first
from tests.test_index_pooled_cpu import brute_pooled
from tests.test_index_pooled_gpu import _assert_counts, _assert_search, _bits, _counts, _mask_rows, _same
from tests.test_index_ranks_gpu import _dev, _lattice, _random
from tests.test_index_sharded_gpu import _spilling, _whole
from tests.test_search_gpu import _cuda, _ref_sims

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
DTYPES = [torch.float32, torch.bfloat16]
MODES = ['mean', 'max']
F32 = np.float32
KS = (1, 10, 128)

# (NQ, C, NT, M, d): the smallest shape; a second query block and tiles of 64 sets with a partial last tile; 16 sets per
# tile and 33 one-tile chunks; one set per tile; 3 query blocks x many one-tile chunks: the score tile reused after pooling
LATTICE = [(1, 1, 1, 1, 8), (65, 2, 129, 2, 8), (9, 8, 513, 3, 8), (3, 128, 5, 1, 8), (130, 4, 3650, 1, 8)]
RANDOM_C = (3, 5, 20, 33, 64, 65, 128)      # SG = 42, 25, 6, 3, 2, 1, 1 sets per tile
NQ, M, D = 70, 7, 16


def _random_nt(c):
  sg = 128 // c
  return [nt for nt in (sg - 1, sg, sg + 1, 4 * sg + 1) if nt >= 1]


def _set_targets(rng, nq, nt, c, t=3):
  """Random target sets with the edges planted: set 0, the last set, both sides of a tile edge (SG - 1, SG), a repeat and a
  -1."""
  sg = 128 // c
  tg = rng.integers(0, nt, (nq, t))
  for i, s in enumerate([0, nt - 1] + [e for e in (sg - 1, sg) if e < nt]):
    tg[i % nq, (i // nq) % t] = s
  tg[nq // 2, 1] = tg[nq // 2, 0]
  tg[nq - 1, t - 1] = -1
  return tg.astype(np.int64)


def _pooled(matrix, c, iw, mode):
  """matrix [NQ, NT * C] (query q's scores) -> [NQ, NT]: the definition, brute_pooled on the transposed matrix."""
  out = np.ascontiguousarray(brute_pooled(np.ascontiguousarray(matrix.T), c, iw, mode).T)
  out.setflags(write=False)
  return out


# ---- 1. lattice inputs ------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _lattice_case(case):
  """The lattice of tests/test_index_ranks_gpu.py with NT * C items, weights 1 / C (a power of two) with about a quarter
  of the items zeroed, and per mode the fp64 pooled matrix -- a float32 value bit for bit, equal to the definition on the
  float32 scores -- its order, targets and their counts."""
  nq, c, nt, m, d = LATTICE[case]
  q, qw, g, gw = _lattice(nq, nt * c, m, d, 1)[:4]
  ref = _ref_sims(q, qw, g, gw)
  assert np.array_equal(ref, ref.astype(F32))
  rng = np.random.default_rng(100 + case)
  iw = _mask_rows(rng, nt, c, F32(1) / F32(c)) if nt > 1 else np.full(c, F32(1) / F32(c), F32)
  assert set(np.unique(iw)) <= {F32(0), F32(1) / F32(c)} and (iw.reshape(nt, c) != 0).any(1).all()
  tg = _set_targets(rng, nq, nt, c) if nt > 1 else np.zeros((1, 1), np.int64)
  cols, w = ref.reshape(nq, nt, c), iw.reshape(nt, c).astype(np.float64)
  by_mode = {}
  for mode in MODES:
    exact = (w[None] * cols).sum(2) if mode == 'mean' else np.where((w != 0)[None], cols, -np.inf).max(2)   # fp64
    pooled = _pooled(ref.astype(F32), c, iw, mode)
    assert np.array_equal(exact, exact.astype(F32)) and np.array_equal(exact.astype(F32), pooled)          # exact in float32
    by_mode[mode] = (pooled, best_first(pooled), _counts(pooled, tg))
  return q, qw, g, gw, iw, tg, by_mode


@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16'])
@pytest.mark.parametrize('case', range(len(LATTICE)), ids=['x'.join(map(str, s)) for s in LATTICE])
def test_item_pooled_scans_are_exact_on_lattice_inputs(case, dtype):
  from mmt_amd import _lib
  from mmt_amd.search import ItemPooling, VideoIndex
  nq, c, nt, m, d = LATTICE[case]
  nv = nt * c
  q, qw, g, gw, iw, tg, by_mode = _lattice_case(case)
  if case == len(LATTICE) - 1:
    # 3 query blocks x 115 chunks: more than one chunk per block, each of one tile of 32 sets, the last of 2
    assert _lib.lib().mmt_topk_itemsets_workspace_keys(nq, nt, c, 10) == nq * 115 * 10 and nt - 114 * 32 == 2
  if case % 2 and nv > 1:
    index = VideoIndex.empty(nv + 200, m, d, DEV, dtype=dtype)      # two pieces and spare capacity
    index.add(_dev(g[:nv // 3]), _dev(gw[:nv // 3]))
    index.add(_dev(g[nv // 3:]), _dev(gw[nv // 3:]))
    assert index.num_items == nv < index.capacity
  else:
    index = VideoIndex(_dev(g), _dev(gw), dtype=dtype)
  qd, qwd, tgd = _dev(q), _dev(qw), _dev(tg)
  for mode in MODES:
    ip = index.item_pooling(c, _dev(iw), mode=mode)
    assert isinstance(ip, ItemPooling) and (ip.set_size, ip.num_sets, ip.num_items, ip.mode) == (c, nt, nv, mode)
    assert ip.device == DEV and np.array_equal(ip.weights.cpu().numpy(), iw)
    pooled, order, counts = by_mode[mode]
    for k in KS:
      _assert_search(index.search(qd, qwd, k=k, item_pooling=ip), pooled, order, k, (mode, k))
    _assert_counts(index.rank_counts(qd, qwd, tgd, item_pooling=ip), counts, mode)
    assert (counts[1][tg >= 0] >= 1).all()                          # a target counts itself
    ranks = index.ranks(qd, qwd, tgd, item_pooling=ip)
    assert ranks.dtype == torch.float64 and np.array_equal(
        ranks.cpu().numpy(), np.where(tg >= 0, counts[0] + (counts[1] - 1) / 2, np.inf))
    one = index.rank_counts(qd, qwd, tgd[:, 0].contiguous(), item_pooling=ip)    # a 1-D target list keeps its shape
    _assert_counts(one, (counts[0][:, 0], counts[1][:, 0]), (mode, '1-D'))
  none = index.search(qd[:0], qwd[:0], k=10, item_pooling=ip)        # no queries: empty outputs, no launch
  assert [tuple(x.shape) for x in none] == [(0, min(10, nt))] * 2
  if index.num_items + c <= index.capacity:                          # it describes the items of its moment
    index.add(_dev(g[:c]), _dev(gw[:c]))
    with pytest.raises(ValueError, match='the item pooling was built for %d items, the index holds %d' % (nv, nv + c)):
      index.search(qd, qwd, k=1, item_pooling=ip)


# ---- 2. random inputs against the scan's own scores ------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _random_case(c, nt, dtype, nq=NQ):
  """A random index of NT * C items, NQ queries, arbitrary item weights (negative ones, zeros) and the scan's own score
  matrix: target_scores with every item as a target, unpooled."""
  from mmt_amd.search import VideoIndex
  nv = nt * c
  q, qw, g, gw = _random(nq, nv, M, D, 7 * c + nt)
  index = VideoIndex(g, gw, dtype=dtype)
  matrix = index.target_scores(q, qw, torch.arange(nv, device=DEV).repeat(nq, 1)).cpu().numpy()
  assert matrix.shape == (nq, nv) and not np.isnan(matrix).any()
  matrix.setflags(write=False)
  rng = np.random.default_rng(c + nt)
  w = rng.standard_normal((nt, c)).astype(F32) * F32(3)
  iw = _mask_rows(rng, nt, c, w) if nt > 1 else np.where(np.arange(c) % 4 == 1, F32(0), w.reshape(-1))
  if c > 1:
    assert (iw < 0).any() and (iw == 0).any()
  assert np.isfinite(iw).all() and (iw.reshape(nt, c) != 0).any(1).all()
  return index, q, qw, matrix, iw, _set_targets(rng, nq, nt, c) if nt > 1 else np.zeros((nq, 1), np.int64)


@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16'])
@pytest.mark.parametrize('c,nt', [(c, nt) for c in RANDOM_C for nt in _random_nt(c)])
def test_item_pooled_scans_equal_the_definition_on_the_scores_of_the_scan(c, nt, dtype):
  index, q, qw, matrix, iw, tg = _random_case(c, nt, dtype)
  every = torch.arange(nt, device=DEV).repeat(NQ, 1)
  for mode in MODES:
    ip = index.item_pooling(c, _cuda(iw).reshape(nt, c), mode=mode)
    pooled = _pooled(matrix, c, iw, mode)
    order = best_first(pooled)
    got = index.target_scores(q, qw, every, item_pooling=ip)         # the pooled bits as they are, -0 included
    assert got.dtype == torch.float32 and tuple(got.shape) == (NQ, nt)
    print('%s: target_scores wrong bits %d of %d' % (mode, (_bits(got) != _bits(pooled)).sum(), pooled.size))
    assert np.array_equal(_bits(got), _bits(pooled)), mode
    for k in KS:
      _assert_search(index.search(q, qw, k=k, item_pooling=ip), pooled, order, k, (mode, k))
    counts = index.rank_counts(q, qw, _cuda(tg), item_pooling=ip)
    _assert_counts(counts, _counts(pooled, tg), mode)
    assert (counts[1].cpu().numpy()[tg >= 0] >= 1).all()
    thr = _cuda(np.take_along_axis(pooled, np.maximum(tg, 0), 1))
    _assert_counts(index.threshold_counts(q, qw, thr, item_pooling=ip), _counts(pooled, np.maximum(tg, 0)), (mode, 'thr'))
    assert _same(index.search(q, qw, k=10, item_pooling=ip), index.search(q, qw, k=10, item_pooling=ip))   # bit-reproducible
    assert _same(index.rank_counts(q, qw, _cuda(tg), item_pooling=ip), counts)


# ---- 3. consistency ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16'])
def test_sets_of_one_item_with_unit_weights_are_the_plain_scans(dtype):
  from mmt_amd.search import VideoIndex
  nq, nv = 130, 4097
  q, qw, g, gw = _random(nq, nv, M, D, 5)
  index = VideoIndex(g, gw, dtype=dtype)
  tg = _cuda(_set_targets(np.random.default_rng(3), nq, nv, 1))
  for mode in MODES:
    ip = index.item_pooling(1, torch.ones(nv, device=DEV), mode=mode)
    for k in KS:
      assert _same(index.search(q, qw, k=k, item_pooling=ip), index.search(q, qw, k=k)), (mode, k)
    assert _same(index.rank_counts(q, qw, tg, item_pooling=ip), index.rank_counts(q, qw, tg)), mode
    assert _same((index.target_scores(q, qw, tg, item_pooling=ip),), (index.target_scores(q, qw, tg),)), mode
  assert _same(index.search(q, qw, k=10, item_pooling=index.item_pooling(1)), index.search(q, qw, k=10))   # the default: 1 / 1


@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16'])
def test_the_text_layout_queries_work(dtype):
  c, nt = 5, 26
  index, q, qw, matrix, iw, tg = _random_case(c, nt, dtype)
  b, cq = NQ // 7, 7
  q4 = q.reshape(b, cq, M, D).permute(0, 2, 1, 3).contiguous()       # (B, M, C, d) / (B, C, M): rows b * C + c
  for mode in MODES:
    ip = index.item_pooling(c, _cuda(iw), mode=mode)
    assert _same(index.search(q4, qw.reshape(b, cq, M), k=10, item_pooling=ip), index.search(q, qw, k=10, item_pooling=ip))
    assert _same(index.rank_counts(q4, qw.reshape(b, cq, M), _cuda(tg), item_pooling=ip),
                 index.rank_counts(q, qw, _cuda(tg), item_pooling=ip))


@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16'])
def test_subsets_of_sets_equal_brute_force_on_the_allowed_sets(dtype):
  """70 queries x 425 sets of 3: tiles of 42 sets, so a tile's first set is no multiple of 32 and its mask bits come from
  an unaligned window of the bitmap.  A random half; one set; a contiguous range that empties whole tiles (they are
  skipped before their K loop); a range that starts mid-word (set 45: bit 13); the last set alone (the bitmap's last word,
  and the window of the last tile reaches past it)."""
  from mmt_amd.search import IndexSubset
  c, nt = 3, 425
  index, q, qw, matrix, iw, tg = _random_case(c, nt, dtype)
  every = np.arange(nt)
  masks = {'random_half': np.random.default_rng(4).random(nt) < 0.5, 'one_set': every == 100,
           'sets_90_to_299': (every >= 90) & (every < 300), 'sets_45_to_60': (every >= 45) & (every <= 60),
           'last_set': every == nt - 1}
  for mode in MODES:
    ip = index.item_pooling(c, _cuda(iw), mode=mode)
    pooled = _pooled(matrix, c, iw, mode)
    for name, mask in masks.items():
      sub = ip.subset(_cuda(mask))
      assert isinstance(sub, IndexSubset) and sub.num_items == nt and sub.count == mask.sum()
      allowed = np.flatnonzero(mask)
      inside = pooled[:, allowed]
      order = allowed[best_first(inside)]                              # ties by ascending ORIGINAL set number
      for k in (10, 128):
        scores, indices = index.search(q, qw, k=k, item_pooling=ip, subset=sub)
        kout = min(k, allowed.size)
        assert tuple(indices.shape) == (NQ, kout), (mode, name, k)
        assert np.array_equal(indices.cpu().numpy(), order[:, :kout]), (mode, name, k)
        assert np.array_equal(_bits(scores), _bits(np.take_along_axis(pooled, order[:, :kout], 1) + F32(0))), (mode, name, k)
      thr = np.take_along_axis(pooled, np.maximum(tg, 0), 1)
      want_g = np.where(tg >= 0, (inside[:, None, :] > thr[:, :, None]).sum(2), 0).astype(np.int32)
      want_e = np.where(tg >= 0, (inside[:, None, :] == thr[:, :, None]).sum(2), 0).astype(np.int32)
      assert (tg >= 0).any() and (~mask[np.maximum(tg, 0)] & (tg >= 0)).any()    # targets outside the subset: not counted
      _assert_counts(index.rank_counts(q, qw, _cuda(tg), item_pooling=ip, subset=sub), (want_g, want_e), (mode, name))
      ranks = index.ranks(q, qw, _cuda(tg), item_pooling=ip, subset=sub).cpu().numpy()
      assert np.array_equal(np.isinf(ranks), (tg < 0) | ~mask[np.maximum(tg, 0)])
    sub = ip.subset(torch.tensor([7, 300, 7], device=DEV))              # set numbers, with a duplicate
    assert sub.count == 2 and index.search(q, qw, k=5, item_pooling=ip, subset=sub)[1].sort(1).values.tolist() == [[7, 300]] * NQ
  with pytest.raises(ValueError, match='the subset was built for %d sets, the item pooling has %d' % (nt * c, nt)):
    index.search(q, qw, item_pooling=ip, subset=index.subset(torch.ones(nt * c, device=DEV, dtype=torch.bool)))


@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16'])
@pytest.mark.parametrize('c', [3, 20, 128])
def test_query_batches_do_not_change_the_result(c, dtype, monkeypatch):
  from mmt_amd import search
  nt = 4 * (128 // c) + 1
  index, q, qw, matrix, iw, tg = _random_case(c, nt, dtype)
  ip = index.item_pooling(c, _cuda(iw))
  whole = (index.search(q, qw, k=10, item_pooling=ip), index.rank_counts(q, qw, _cuda(tg), item_pooling=ip),
           (index.target_scores(q, qw, _cuda(tg), item_pooling=ip),))
  assert len(index._row_batches(NQ, 0)) == 1
  monkeypatch.setattr(search, '_BATCH_BYTES', 1)                      # one query block per batch
  assert index._row_batches(NQ, 0) == [(0, 64), (64, NQ)]
  assert _same(index.search(q, qw, k=10, item_pooling=ip), whole[0])
  assert _same(index.rank_counts(q, qw, _cuda(tg), item_pooling=ip), whole[1])
  assert _same((index.target_scores(q, qw, _cuda(tg), item_pooling=ip),), whole[2])


# ---- 4. sharded -------------------------------------------------------------------------------------------------------

def _spilling_whole_sets(g, gw, dtype):
  """700 items = 140 sets of 5 on three shards of 235 rows (47 sets), added in pieces of whole sets, two of which spill."""
  from mmt_amd.search import ShardedVideoIndex
  index = ShardedVideoIndex.empty(705, g.shape[1], g.shape[2], [DEV] * 3, dtype=dtype)
  assert [sh.capacity for sh in index.shards] == [235] * 3
  assert index.add(g[:300], gw[:300]) == (0, 300)          # fills shard 0, 13 sets spill to shard 1
  assert index.shard_sizes == [235, 65, 0]
  assert index.add(g[300:400], gw[300:400]) == (300, 400)  # the emptiest shard
  assert index.add(g[400:], gw[400:]) == (400, 700)        # fills shard 1, the rest spills to shard 2
  assert index.shard_sizes == [235, 235, 230]
  return index


@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16'])
@pytest.mark.parametrize('build', [_whole(1), _spilling_whole_sets], ids=['1', '3_spilling'])
def test_sharded_equals_monolithic_bit_for_bit(build, dtype):
  from mmt_amd.search import ShardedItemPooling, VideoIndex
  nq, c, nt, m, d = 13, 5, 140, 3, 8
  nv = nt * c
  q, qw, g, gw = _random(nq, nv, m, d, nq + c + nv)
  for twin in (60, nt - 1):                                   # copies of set 0 on other shards: ties across shards
    g[twin * c:twin * c + c], gw[twin * c:twin * c + c] = g[:c], gw[:c]
  qw[3] = 0                                                   # query 3: every score 0, one tie over all shards
  rng = np.random.default_rng(11)
  iw = _mask_rows(rng, nt, c, rng.standard_normal((nt, c)).astype(F32))
  iw.reshape(nt, c)[[60, nt - 1]] = iw.reshape(nt, c)[0]
  iw, tg = _cuda(iw), _cuda(_set_targets(rng, nq, nt, c))
  mono = VideoIndex(g, gw, dtype=dtype)
  shard = build(g, gw, dtype)
  assert shard.num_items == nv
  every = torch.arange(nt, device=DEV)
  masks = {None: None, 'every_other': every % 2 == 1, 'one_set': every == 60}
  if len(shard.shards) > 1:
    masks['without_shard_0'] = shard._shard_of[:nv:c] != 0    # a shard without an allowed set
  for mode in MODES:
    ip_m, ip_s = mono.item_pooling(c, iw, mode=mode), shard.item_pooling(c, iw, mode=mode)
    assert isinstance(ip_s, ShardedItemPooling) and torch.equal(ip_s.weights, ip_m.weights)
    assert (ip_s.set_size, ip_s.num_sets, ip_s.num_items, ip_s.mode, ip_s.device) == (c, nt, nv, mode, DEV)
    assert sorted(torch.cat([t for t in ip_s.tables if t is not None]).tolist()) == list(range(nt))
    for name, mask in masks.items():
      sub_m, sub_s = (None, None) if mask is None else (ip_m.subset(mask), ip_s.subset(mask))
      for k in KS:
        got = shard.search(q, qw, k=k, item_pooling=ip_s, subset=sub_s)
        assert all(x.device == DEV for x in got)
        assert _same(got, mono.search(q, qw, k=k, item_pooling=ip_m, subset=sub_m)), (mode, name, k)
      assert _same(shard.rank_counts(q, qw, tg, item_pooling=ip_s, subset=sub_s),
                   mono.rank_counts(q, qw, tg, item_pooling=ip_m, subset=sub_m)), (mode, name)
      assert torch.equal(shard.ranks(q, qw, tg, item_pooling=ip_s, subset=sub_s),
                         mono.ranks(q, qw, tg, item_pooling=ip_m, subset=sub_m)), (mode, name)
  first = mono.search(q, qw, k=3, item_pooling=ip_m)[1][3].tolist()
  assert first == [0, 1, 2]                                   # the all-zero query: ties by ascending set number


def test_a_layout_that_splits_a_set_across_shards_is_refused():
  q, qw, g, gw = _random(1, 700, 3, 8, 1)
  shard = _spilling(g, gw, torch.float32)                    # pieces of 234, 66, 129, ...: the set at items 428, 429 is split
  with pytest.raises(ValueError, match='item_pooling: a set of 2 items is split across shards'):
    shard.item_pooling(2)
  assert shard.item_pooling(1).num_sets == 700
  three = _whole(3)(g[:696], gw[:696], torch.float32)        # 232 items per shard: sets of 8 are whole, sets of 3 are not
  with pytest.raises(ValueError, match='split across shards'):
    three.item_pooling(3)
  assert three.item_pooling(8).num_sets == 87


# ---- 5. golden --------------------------------------------------------------------------------------------------------

def test_item_pooled_mean_gives_the_avg_similarities_of_the_reference():
  """tests/golden/sim_loss_metric.npz: 5 videos (one with all-zero weights: the 1e-5 denominator), 5 x 3 captions.  A
  caption index in row order b * C + c with item_pooling(3), queried with the videos, gives sims_avg transposed.
  Tolerance 1e-5, the one tests/test_index_pooled_gpu.py and tests/test_cenet_gpu.py grant on this file."""
  from mmt_amd.search import VideoIndex
  g = load_npz('sim_loss_metric')
  avg = g['sims_avg']
  b, c, m = g['sim_in_tw'].shape
  d = g['sim_in_txt'].shape[3]
  assert (g['sim_in_vw'] == 0).all(1).any()
  txt = _cuda(g['sim_in_txt']).permute(0, 2, 1, 3).reshape(b * c, m, d).contiguous()
  index = VideoIndex(txt, _cuda(g['sim_in_tw']).reshape(b * c, m), dtype=torch.float32)
  ip = index.item_pooling(c)
  vid, vw = _cuda(g['sim_in_vid']), _cuda(g['sim_in_vw'])
  every = torch.arange(b, device=DEV).repeat(b, 1)
  thr = index.target_scores(vid, vw, every, item_pooling=ip).cpu().numpy()
  scores, indices = index.search(vid, vw, k=5, item_pooling=ip)
  scores, indices = scores.cpu().numpy(), indices.cpu().numpy()
  print('target_scores max err %.3g' % np.abs(thr - avg.T).max())
  assert thr.shape == scores.shape == indices.shape == (5, 5) and np.abs(thr - avg.T).max() < 1e-5
  assert (np.sort(indices, 1) == np.arange(5)).all() and (np.diff(scores, axis=1) <= 0).all()
  assert np.array_equal(_bits(np.take_along_axis(thr, indices, 1) + F32(0)), _bits(scores))


def _assert_avg_metrics(got, sims_avg):
  from mmt_amd.metric import t2v_metrics, v2t_metrics
  want = {'t2v_metrics': t2v_metrics(sims_avg), 'v2t_metrics': v2t_metrics(sims_avg)}
  for half in want:
    assert set(got[half]) == set(want[half]), half
    print(half, got[half]['cols'], want[half]['cols'])
    assert np.array_equal(got[half]['cols'], want[half]['cols']), half
    for key in want[half]:
      if key != 'cols':
        assert got[half][key] == want[half][key], (half, key)


def test_avg_metrics_of_the_golden_file_without_the_matrix():
  """The ranks of sims_avg cannot be reordered by the 1e-5 of the scores: every row of sims_avg has gaps >= 0.04, every
  column of a weighted video gaps >= 0.009, and the zero-weight video scores exactly 0 everywhere (asserted below)."""
  from mmt_amd.metric import retrieval_metrics_indexed
  g = load_npz('sim_loss_metric')
  avg = g['sims_avg']
  zero = (g['sim_in_vw'] == 0).all(1)
  assert np.diff(np.sort(avg, 1), axis=1).min() >= 0.04 and (avg[:, zero] == 0).all()
  assert np.diff(np.sort(avg[:, ~zero], 0), axis=0).min() >= 0.009
  got = retrieval_metrics_indexed(g['sim_in_vid'], g['sim_in_txt'], g['sim_in_vw'], g['sim_in_tw'], caption_mode='avg')
  _assert_avg_metrics(got, avg)


@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16'])
def test_avg_metrics_on_a_lattice_eval_set(dtype):
  """37 videos x 4 captions on the lattice, where the mean of the captions' similarities is exact in float32 and ties
  abound: all videos, a cut of them, and both indexes sharded over two shards."""
  from mmt_amd.metric import retrieval_metrics_indexed
  b, c, m, d = 37, 4, 3, 8
  txt, tw, vid, vw = (np.array(x) for x in _lattice(b * c, b, m, d, 1)[:4])   # caption rows b * C + c; copies: writable
  indep = _ref_sims(txt, tw, vid, vw)                               # [B * C, B]
  avg = indep.reshape(b, c, b).mean(1)
  assert np.array_equal(avg, avg.astype(F32))
  txt4 = np.ascontiguousarray(txt.reshape(b, c, m, d).transpose(0, 2, 1, 3))
  args = (vid, txt4, vw, tw.reshape(b, c, m))
  _assert_avg_metrics(retrieval_metrics_indexed(*args, dtype=dtype, caption_mode='avg'), avg.astype(F32))
  _assert_avg_metrics(retrieval_metrics_indexed(*args, dtype=dtype, caption_mode='avg', devices=[0, 0]), avg.astype(F32))
  cut = np.random.default_rng(5).random(b) < 0.6
  for devices in (None, [0, 0]):
    got = retrieval_metrics_indexed(*args, dtype=dtype, caption_mode='avg', video_subset=cut, devices=devices)
    _assert_avg_metrics(got, np.ascontiguousarray(avg[cut][:, cut]).astype(F32))
  indep_metrics = retrieval_metrics_indexed(*args, dtype=dtype)     # 'indep' is untouched: one rank per caption
  assert indep_metrics['t2v_metrics']['cols'].shape == (b * c,)


# ---- 6. memory --------------------------------------------------------------------------------------------------------

def test_item_pooled_search_allocates_no_quadratic_buffer():
  """64 queries x 65 536 sets of 4, M = 1, d = 8, bf16, k = 10.  What the calls hold at their peak: the outputs, the folded
  queries, the chunk lists and the chunk counters, within 3 MiB, where the score matrix would be 64 MiB."""
  from mmt_amd import _lib
  from mmt_amd.search import VideoIndex
  nq, c, nt, m, d, k = 64, 4, 65536, 1, 8, 10
  nv = nt * c
  gen = torch.Generator(device=DEV).manual_seed(8)
  index = VideoIndex(torch.rand(nv, m, d, device=DEV, generator=gen) - 0.5, torch.rand(nv, m, device=DEV, generator=gen) + 0.5,
                     dtype=torch.bfloat16)
  q = torch.rand(nq, m, d, device=DEV, generator=gen) - 0.5
  qw = torch.rand(nq, m, device=DEV, generator=gen) + 0.5
  ip = index.item_pooling(c)
  tg = torch.arange(nq, device=DEV) * 1000
  torch.cuda.synchronize()
  base = torch.cuda.memory_allocated()
  torch.cuda.reset_peak_memory_stats()
  scores, indices = index.search(q, qw, k=k, item_pooling=ip)
  greater, equal = index.rank_counts(q, qw, tg, item_pooling=ip)
  torch.cuda.synchronize()
  growth = torch.cuda.max_memory_allocated() - base
  lists = 8 * _lib.lib().mmt_topk_itemsets_workspace_keys(nq, nt, c, k)
  counters = 4 * _lib.lib().mmt_count_itemsets_workspace_ints(nq, nt, c, 1)
  print('allocator peak growth %.1f KiB, chunk lists %.1f KiB, counters %.1f KiB, matrix %.1f KiB' % (
      growth / 1024, lists / 1024, counters / 1024, nq * nv * 4 / 1024))
  assert lists + counters + 12 * nq * k + 32 * nq <= 3 << 20
  assert growth < nq * nv * 4 // 4, growth
  # and the answers agree with each other: target set t of query q is beaten by `greater` sets, so it is in the list iff < k
  thr = index.target_scores(q, qw, tg, item_pooling=ip)
  inside = (indices == tg[:, None]).any(1)
  assert torch.equal(inside, greater < k) and bool((equal >= 1).all())
  assert bool((scores[:, -1] >= thr)[~inside].all())
