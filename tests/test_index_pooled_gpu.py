"""Query-set pooling of VideoIndex / ShardedVideoIndex (pooling= of search, rank_counts, ranks, target_scores and
threshold_counts; mmt_search_topk_pooled, mmt_search_thresholds_pooled, mmt_search_count_pooled and their bf16 forms): the
queries are sets of C rows and every scan answers per set, on the mean or the max of the set's scores.

  1. lattice inputs with power-of-two weights, where fp32, bf16 and fp64 agree bit for bit and ties abound: score bits,
     indices and counts equal brute force on the fp64 pooled matrix, for both modes;
  2. random inputs and arbitrary weights: equal to brute_pooled of the scan's own score matrix (target_scores over every
     item, unpooled), bit for bit -- an fma or a reordered sum shows here;
  3. consistent with the plain scans (sets of one), the text layout, subsets, query batches;  4. sharded equals monolithic;
  5. the reference's 'avg' similarities of the golden file;  6. no buffer that grows with NQ * NV."""
import functools

import numpy as np
import pytest
import torch

from tests.fixtures import load_npz
from tests.test_index_groups_cpu import best_first
from tests.test_index_pooled_cpu import brute_pooled
from tests.test_index_ranks_gpu import _dev, _lattice, _random
from tests.test_index_sharded_gpu import _spilling, _whole
from tests.test_search_gpu import _cuda, _ref_sims

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
DTYPES = [torch.float32, torch.bfloat16]
MODES = ['mean', 'max']
F32 = np.float32
KS = (1, 10, 128)

# (NS, C, NV, M, d): one row; a second block holding one set (32 sets per block); 8 sets per block and 33 one-tile chunks;
# one set per block; 9 blocks of 16 sets x 58 chunks of 256 items: two tiles per block, the score tile reused after pooling
LATTICE = [(1, 1, 1, 1, 8), (33, 2, 129, 2, 8), (9, 8, 4097, 3, 8), (3, 64, 257, 1, 8), (130, 4, 14600, 1, 8)]
# C -> NS of the random cases: blocks of 21, 12, 3, 1 and 1 sets (rows 63, 60, 60, 33 and 64 of 64 in use) and a partial
# last block everywhere but at one set per block
RANDOM_SETS = {3: 45, 5: 14, 20: 4, 33: 2, 64: 3}
RANDOM_NV = (127, 129, 4097)
M, D = 7, 16


def _bits(x):
  x = x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
  return np.ascontiguousarray(x, F32).view(np.int32)


def _mask_rows(rng, ns, c, w):
  """Row weights [ns * c]: w with about a quarter of the rows zeroed, every set keeping a row; where there is room, set 0
  loses its first row and the last set keeps only its last."""
  w = np.array(np.broadcast_to(w, (ns, c)), F32)
  if c > 1:
    keep = rng.random((ns, c)) >= 0.25
    keep[np.arange(ns), rng.integers(0, c, ns)] = True
    keep[0, 0], keep[0, 1] = False, True
    keep[ns - 1] = False
    keep[ns - 1, c - 1] = True
    w[~keep] = 0
  return w.reshape(-1)


def _counts(pooled, tg):
  """(greater, equal) int32 of tg's shape: the items of row s above / equal to pooled[s, tg[s, t]]; 0 / 0 for -1."""
  thr = np.take_along_axis(pooled, np.maximum(tg, 0), 1)
  greater = (pooled[:, None, :] > thr[:, :, None]).sum(2)
  equal = (pooled[:, None, :] == thr[:, :, None]).sum(2)
  return np.where(tg >= 0, greater, 0).astype(np.int32), np.where(tg >= 0, equal, 0).astype(np.int32)


def _targets(rng, ns, nv, t=3):
  """Random targets with the edges planted: item 0, the last item, both sides of a tile edge, a repeat and a -1."""
  tg = rng.integers(0, nv, (ns, t))
  for i, item in enumerate([0, nv - 1] + [e for e in (127, 128) if e < nv]):
    tg[i % ns, (i // ns) % t] = item
  tg[ns // 2, 1] = tg[ns // 2, 0]
  tg[ns - 1, t - 1] = -1
  return tg.astype(np.int64)


def _assert_search(got, pooled, order, k, what):
  """search's (scores, indices) against the pooled matrix: indices = its first k by best_first, the scores its bits there
  with -0 as +0."""
  scores, indices = got
  kout = min(k, pooled.shape[1])
  assert scores.dtype == torch.float32 and indices.dtype == torch.int64 and scores.device == DEV, what
  assert tuple(scores.shape) == tuple(indices.shape) == (pooled.shape[0], kout), what
  want_i = order[:, :kout]
  want_s = np.take_along_axis(pooled, want_i, 1) + F32(0)
  wrong = ((indices.cpu().numpy() != want_i).sum(), (_bits(scores) != _bits(want_s)).sum())
  print('%s: %d slots, wrong indices %d, score bits %d' % (what, want_i.size, *wrong))
  assert np.array_equal(indices.cpu().numpy(), want_i), what
  assert np.array_equal(_bits(scores), _bits(want_s)), what


def _assert_counts(got, want, what):
  for g, w, name in zip(got, want, ('greater', 'equal')):
    assert g.dtype == torch.int32 and tuple(g.shape) == w.shape and g.device == DEV, what
    print('%s: %s mismatches %d of %d' % (what, name, (g.cpu().numpy() != w).sum(), w.size))
    assert np.array_equal(g.cpu().numpy(), w), (what, name)


def _same(a, b):
  return all(x.shape == y.shape and torch.equal(x.contiguous().view(torch.int32) if x.dtype == torch.float32 else x,
                                                y.contiguous().view(torch.int32) if y.dtype == torch.float32 else y)
             for x, y in zip(a, b))


# ---- 1. lattice inputs ------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _lattice_case(case):
  """The lattice of tests/test_index_ranks_gpu.py with NS * C query rows, weights 1 / C (a power of two) with rows masked,
  and per mode the fp64 pooled matrix -- a float32 value bit for bit, equal to brute_pooled of the float32 scores -- its
  order, targets and their counts."""
  ns, c, nv, m, d = LATTICE[case]
  q, qw, g, gw = _lattice(ns * c, nv, m, d, 1)[:4]
  ref = _ref_sims(q, qw, g, gw)
  assert np.array_equal(ref, ref.astype(F32))
  rng = np.random.default_rng(case)
  rw = _mask_rows(rng, ns, c, F32(1) / F32(c))
  assert set(np.unique(rw)) <= {F32(0), F32(1) / F32(c)} and (rw.reshape(ns, c) != 0).any(1).all()
  tg = _targets(rng, ns, nv) if nv > 1 else np.zeros((1, 1), np.int64)
  rows, w = ref.reshape(ns, c, nv), rw.reshape(ns, c).astype(np.float64)
  part = (w != 0)[:, :, None]
  by_mode = {}
  for mode in MODES:
    exact = (w[:, :, None] * rows).sum(1) if mode == 'mean' else np.where(part, rows, -np.inf).max(1)   # fp64
    pooled = brute_pooled(ref.astype(F32), c, rw, mode)
    assert np.array_equal(exact, exact.astype(F32)) and np.array_equal(exact.astype(F32), pooled)        # exact in float32
    pooled.setflags(write=False)
    by_mode[mode] = (pooled, best_first(pooled), _counts(pooled, tg))
  return q, qw, g, gw, rw, tg, by_mode


@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16'])
@pytest.mark.parametrize('case', range(len(LATTICE)), ids=['x'.join(map(str, s)) for s in LATTICE])
def test_pooled_scans_are_exact_on_lattice_inputs(case, dtype):
  from mmt_amd import _lib
  from mmt_amd.search import QueryPooling, VideoIndex
  ns, c, nv, m, d = LATTICE[case]
  q, qw, g, gw, rw, tg, by_mode = _lattice_case(case)
  if case == len(LATTICE) - 1:
    # 9 query blocks x 58 chunks of 256 items >= 512 blocks: every block walks two tiles, pooling the second in the LDS the
    # first was pooled in, and carries its lists across them
    assert _lib.lib().mmt_topk_pooled_workspace_keys(ns, c, nv, 10) == ns * 58 * 10 and nv - 57 * 256 == 8
    assert -(-ns // (64 // c)) * 58 >= 512
  if case % 2 and nv > 1:
    index = VideoIndex.empty(nv + 200, m, d, DEV, dtype=dtype)      # two pieces and spare capacity
    index.add(_dev(g[:nv // 3]), _dev(gw[:nv // 3]))
    index.add(_dev(g[nv // 3:]), _dev(gw[nv // 3:]))
    assert index.num_items == nv < index.capacity
  else:
    index = VideoIndex(_dev(g), _dev(gw), dtype=dtype)
  qd, qwd, tgd = _dev(q), _dev(qw), _dev(tg)
  for mode in MODES:
    pool = index.pooling(c, ns, _dev(rw), mode=mode)
    assert isinstance(pool, QueryPooling) and (pool.set_size, pool.num_sets, pool.num_rows, pool.mode) == (c, ns, ns * c, mode)
    assert pool.device == DEV and np.array_equal(pool.weights.cpu().numpy(), rw)
    pooled, order, counts = by_mode[mode]
    for k in KS:
      _assert_search(index.search(qd, qwd, k=k, pooling=pool), pooled, order, k, (mode, k))
    _assert_counts(index.rank_counts(qd, qwd, tgd, pooling=pool), counts, mode)
    assert (counts[1][tg >= 0] >= 1).all()                          # a target counts itself
    ranks = index.ranks(qd, qwd, tgd, pooling=pool)
    assert ranks.dtype == torch.float64 and np.array_equal(
        ranks.cpu().numpy(), np.where(tg >= 0, counts[0] + (counts[1] - 1) / 2, np.inf))
    one = index.rank_counts(qd, qwd, tgd[:, 0].contiguous(), pooling=pool)       # a 1-D target list keeps its shape
    _assert_counts(one, (counts[0][:, 0], counts[1][:, 0]), (mode, '1-D'))
  none = index.search(qd[:0], qwd[:0], k=10, pooling=index.pooling(c, 0))          # no sets: empty outputs, no launch
  assert [tuple(x.shape) for x in none] == [(0, min(10, nv))] * 2
  if index.num_items < index.capacity:                              # a pooling does not describe the items: valid after `add`
    index.add(_dev(g[:1]), _dev(gw[:1]))
    again = index.search(qd, qwd, k=1, pooling=pool)
    assert tuple(again[1].shape) == (ns, 1) and bool((again[1] <= nv).all())


# ---- 2. random inputs against the scan's own scores ------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _random_case(c, nv, dtype):
  """A random index, NS * C queries, arbitrary row weights (negative ones, zeros) and the scan's own score matrix:
  target_scores with every item as a target, unpooled."""
  from mmt_amd.search import VideoIndex
  ns = RANDOM_SETS[c]
  q, qw, g, gw = _random(ns * c, nv, M, D, 7 * c + nv)
  index = VideoIndex(g, gw, dtype=dtype)
  matrix = index.target_scores(q, qw, torch.arange(nv, device=DEV).repeat(ns * c, 1)).cpu().numpy()
  assert matrix.shape == (ns * c, nv) and not np.isnan(matrix).any()
  matrix.setflags(write=False)
  rng = np.random.default_rng(c + nv)
  rw = _mask_rows(rng, ns, c, rng.standard_normal((ns, c)).astype(F32) * F32(3))
  assert (rw < 0).any() and (rw == 0).any() and np.isfinite(rw).all()
  return index, q, qw, matrix, rw, _targets(rng, ns, nv)


@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16'])
@pytest.mark.parametrize('nv', RANDOM_NV)
@pytest.mark.parametrize('c', sorted(RANDOM_SETS))
def test_pooled_scans_equal_the_definition_on_the_scores_of_the_scan(c, nv, dtype):
  index, q, qw, matrix, rw, tg = _random_case(c, nv, dtype)
  ns = RANDOM_SETS[c]
  every = torch.arange(nv, device=DEV).repeat(ns, 1)
  for mode in MODES:
    pool = index.pooling(c, ns, _cuda(rw).reshape(ns, c), mode=mode)
    pooled = brute_pooled(matrix, c, rw, mode)
    order = best_first(pooled)
    got = index.target_scores(q, qw, every, pooling=pool)            # the pooled bits as they are, -0 included
    assert got.dtype == torch.float32 and tuple(got.shape) == (ns, nv)
    print('%s: target_scores wrong bits %d of %d' % (mode, (_bits(got) != _bits(pooled)).sum(), pooled.size))
    assert np.array_equal(_bits(got), _bits(pooled)), mode
    for k in KS:
      _assert_search(index.search(q, qw, k=k, pooling=pool), pooled, order, k, (mode, k))
    counts = index.rank_counts(q, qw, _cuda(tg), pooling=pool)
    _assert_counts(counts, _counts(pooled, tg), mode)
    assert (counts[1].cpu().numpy()[tg >= 0] >= 1).all()
    thr = _cuda(np.take_along_axis(pooled, np.maximum(tg, 0), 1))
    _assert_counts(index.threshold_counts(q, qw, thr, pooling=pool), _counts(pooled, np.maximum(tg, 0)), (mode, 'thr'))
    assert _same(index.search(q, qw, k=10, pooling=pool), index.search(q, qw, k=10, pooling=pool))   # bit-reproducible
    assert _same(index.rank_counts(q, qw, _cuda(tg), pooling=pool), counts)


# ---- 3. consistency ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16'])
def test_sets_of_one_row_with_unit_weights_are_the_plain_scans(dtype):
  from mmt_amd.search import VideoIndex
  nq, nv = 130, 4097
  q, qw, g, gw = _random(nq, nv, M, D, 5)
  index = VideoIndex(g, gw, dtype=dtype)
  tg = _cuda(_targets(np.random.default_rng(3), nq, nv))
  for mode in MODES:
    pool = index.pooling(1, nq, torch.ones(nq, device=DEV), mode=mode)
    for k in KS:
      assert _same(index.search(q, qw, k=k, pooling=pool), index.search(q, qw, k=k)), (mode, k)
    assert _same(index.rank_counts(q, qw, tg, pooling=pool), index.rank_counts(q, qw, tg)), mode
    assert _same((index.target_scores(q, qw, tg, pooling=pool),), (index.target_scores(q, qw, tg),)), mode
  assert _same(index.search(q, qw, k=10, pooling=index.pooling(1, nq)), index.search(q, qw, k=10))   # the default: 1 / 1


@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16'])
def test_the_text_layout_is_sets_of_its_captions(dtype):
  c, nv = 5, 129
  index, q, qw, matrix, rw, tg = _random_case(c, nv, dtype)
  b = RANDOM_SETS[c]
  q4 = q.reshape(b, c, M, D).permute(0, 2, 1, 3).contiguous()        # (B, M, C, d) / (B, C, M): rows b * C + c
  for mode in MODES:
    pool = index.pooling(c, b, _cuda(rw), mode=mode)
    assert _same(index.search(q4, qw.reshape(b, c, M), k=10, pooling=pool), index.search(q, qw, k=10, pooling=pool))
    assert _same(index.rank_counts(q4, qw.reshape(b, c, M), _cuda(tg), pooling=pool),
                 index.rank_counts(q, qw, _cuda(tg), pooling=pool))
  with pytest.raises(ValueError, match=r'%d queries but the pooling has %d rows' % (b * c, (b + 1) * c)):
    index.search(q, qw, pooling=index.pooling(c, b + 1))


@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16'])
def test_subsets_equal_brute_force_on_the_allowed_items(dtype):
  """45 sets of 3 x 4097 items, chunks of one tile: a random half, one item, and a contiguous range that empties every
  other tile (they are skipped before their K loop)."""
  c, nv = 3, 4097
  index, q, qw, matrix, rw, tg = _random_case(c, nv, dtype)
  ns = RANDOM_SETS[c]
  every = np.arange(nv)
  masks = {'random_half': np.random.default_rng(4).random(nv) < 0.5, 'one_item': every == 300,
           'items_200_to_449': (every >= 200) & (every < 450)}
  for mode in MODES:
    pool = index.pooling(c, ns, _cuda(rw), mode=mode)
    pooled = brute_pooled(matrix, c, rw, mode)
    for name, mask in masks.items():
      sub = index.subset(_cuda(mask))
      allowed = np.flatnonzero(mask)
      inside = pooled[:, allowed]
      order = allowed[best_first(inside)]                              # ties by ascending ORIGINAL item number
      for k in (10, 128):
        scores, indices = index.search(q, qw, k=k, pooling=pool, subset=sub)
        kout = min(k, allowed.size)
        assert tuple(indices.shape) == (ns, kout), (mode, name, k)
        assert np.array_equal(indices.cpu().numpy(), order[:, :kout]), (mode, name, k)
        assert np.array_equal(_bits(scores), _bits(np.take_along_axis(pooled, order[:, :kout], 1) + F32(0))), (mode, name, k)
      thr = np.take_along_axis(pooled, np.maximum(tg, 0), 1)
      want_g = np.where(tg >= 0, (inside[:, None, :] > thr[:, :, None]).sum(2), 0).astype(np.int32)
      want_e = np.where(tg >= 0, (inside[:, None, :] == thr[:, :, None]).sum(2), 0).astype(np.int32)
      _assert_counts(index.rank_counts(q, qw, _cuda(tg), pooling=pool, subset=sub), (want_g, want_e), (mode, name))


@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16'])
@pytest.mark.parametrize('c', [3, 20, 64])
def test_query_batches_do_not_change_the_result(c, dtype, monkeypatch):
  from mmt_amd import search
  nv = 129
  index, q, qw, matrix, rw, tg = _random_case(c, nv, dtype)
  ns = RANDOM_SETS[c]
  pool = index.pooling(c, ns, _cuda(rw))
  whole = (index.search(q, qw, k=10, pooling=pool), index.rank_counts(q, qw, _cuda(tg), pooling=pool),
           (index.target_scores(q, qw, _cuda(tg), pooling=pool),))
  assert len(index._row_batches(ns * c, 0, pool)) == 1
  monkeypatch.setattr(search, '_BATCH_BYTES', 1)                      # one block of whole sets per batch
  batches = index._row_batches(ns * c, 0, pool)
  block = 64 // c * c
  assert batches == [(r0, min(ns * c, r0 + block)) for r0 in range(0, ns * c, block)] and len(batches) > 1
  assert _same(index.search(q, qw, k=10, pooling=pool), whole[0])
  assert _same(index.rank_counts(q, qw, _cuda(tg), pooling=pool), whole[1])
  assert _same((index.target_scores(q, qw, _cuda(tg), pooling=pool),), whole[2])


# ---- 4. sharded -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16'])
@pytest.mark.parametrize('build', [_whole(1), _spilling], ids=['1', '3_spilling'])
def test_sharded_equals_monolithic_bit_for_bit(build, dtype):
  from mmt_amd.search import VideoIndex
  ns, c, nv, m, d = 13, 5, 700, 3, 8
  q, qw, g, gw = _random(ns * c, nv, m, d, ns + c + nv)
  for twin in (nv // 2, nv - 1):                              # copies of item 0 on other shards: ties across shards
    g[twin], gw[twin] = g[0], gw[0]
  qw[3 * c:4 * c] = 0                                         # set 3: every score 0, one tie over all shards
  rng = np.random.default_rng(11)
  rw = _cuda(_mask_rows(rng, ns, c, rng.standard_normal((ns, c)).astype(F32)))
  tg = _cuda(_targets(rng, ns, nv))
  mono = VideoIndex(g, gw, dtype=dtype)
  shard = build(g, gw, dtype)
  assert shard.num_items == nv
  every = torch.arange(nv, device=DEV)
  masks = {None: None, 'every_other': every % 2 == 1, 'one_item': every == nv // 2}
  if len(shard.shards) > 1:
    masks['without_shard_0'] = shard._shard_of[:nv] != 0     # a shard without an allowed item
  for mode in MODES:
    pool_m, pool_s = mono.pooling(c, ns, rw, mode=mode), shard.pooling(c, ns, rw, mode=mode)
    assert type(pool_s) is type(pool_m) and torch.equal(pool_s.weights, pool_m.weights)
    for name, mask in masks.items():
      sub_m, sub_s = (None, None) if mask is None else (mono.subset(mask), shard.subset(mask))
      for k in KS:
        got = shard.search(q, qw, k=k, pooling=pool_s, subset=sub_s)
        assert all(x.device == DEV for x in got)
        assert _same(got, mono.search(q, qw, k=k, pooling=pool_m, subset=sub_m)), (mode, name, k)
      assert _same(shard.rank_counts(q, qw, tg, pooling=pool_s, subset=sub_s),
                   mono.rank_counts(q, qw, tg, pooling=pool_m, subset=sub_m)), (mode, name)
      assert torch.equal(shard.ranks(q, qw, tg, pooling=pool_s, subset=sub_s),
                         mono.ranks(q, qw, tg, pooling=pool_m, subset=sub_m)), (mode, name)


# ---- 5. golden --------------------------------------------------------------------------------------------------------

def test_pooled_mean_gives_the_avg_similarities_of_the_reference():
  """tests/golden/sim_loss_metric.npz: 5 videos (one with all-zero weights: the 1e-5 denominator), 5 x 3 captions in the
  text layout.  Tolerance 1e-5, the one tests/test_cenet_gpu.py grants the matrix path on this file."""
  from mmt_amd.search import VideoIndex
  g = load_npz('sim_loss_metric')
  avg = g['sims_avg']
  b, c = g['sim_in_tw'].shape[:2]
  assert (g['sim_in_vw'] == 0).all(1).any()
  index = VideoIndex(_cuda(g['sim_in_vid']), _cuda(g['sim_in_vw']), dtype=torch.float32)
  txt, tw = _cuda(g['sim_in_txt']), _cuda(g['sim_in_tw'])
  pool = index.pooling(c, b)
  scores, indices = index.search(txt, tw, k=5, pooling=pool)
  scores, indices = scores.cpu().numpy(), indices.cpu().numpy()
  assert scores.shape == indices.shape == avg.shape == (5, 5)
  assert (np.sort(indices, 1) == np.arange(5)).all() and (np.diff(scores, axis=1) <= 0).all()
  err = np.abs(scores - np.take_along_axis(avg, indices, 1)).max()
  every = torch.arange(5, device=DEV).repeat(b, 1)
  thr = index.target_scores(txt, tw, every, pooling=pool).cpu().numpy()
  print('search max err %.3g, target_scores max err %.3g' % (err, np.abs(thr - avg).max()))
  assert err < 1e-5 and np.abs(thr - avg).max() < 1e-5
  assert np.array_equal(_bits(np.take_along_axis(thr, indices, 1) + F32(0)), _bits(scores))


# ---- 6. memory --------------------------------------------------------------------------------------------------------

def test_pooled_search_allocates_no_quadratic_buffer():
  """16 sets of 4 x 262 144 items, M = 1, d = 8, bf16, k = 10.  What the calls hold at their peak: the outputs, the folded
  queries, the chunk lists and the chunk counters, far below 3 MiB, where the score matrix would be 64 MiB."""
  from mmt_amd import _lib
  from mmt_amd.search import VideoIndex
  ns, c, nv, m, d, k = 16, 4, 262144, 1, 8, 10
  nq = ns * c
  gen = torch.Generator(device=DEV).manual_seed(8)
  index = VideoIndex(torch.rand(nv, m, d, device=DEV, generator=gen) - 0.5, torch.rand(nv, m, device=DEV, generator=gen) + 0.5,
                     dtype=torch.bfloat16)
  q = torch.rand(nq, m, d, device=DEV, generator=gen) - 0.5
  qw = torch.rand(nq, m, device=DEV, generator=gen) + 0.5
  pool = index.pooling(c, ns)
  tg = torch.arange(ns, device=DEV) * 1000
  torch.cuda.synchronize()
  base = torch.cuda.memory_allocated()
  torch.cuda.reset_peak_memory_stats()
  scores, indices = index.search(q, qw, k=k, pooling=pool)
  greater, equal = index.rank_counts(q, qw, tg, pooling=pool)
  torch.cuda.synchronize()
  growth = torch.cuda.max_memory_allocated() - base
  lists = 8 * _lib.lib().mmt_topk_pooled_workspace_keys(ns, c, nv, k)
  counters = 4 * _lib.lib().mmt_count_pooled_workspace_ints(ns, c, nv, 1)
  print('allocator peak growth %.1f KiB, chunk lists %.1f KiB, counters %.1f KiB, matrix %.1f KiB' % (
      growth / 1024, lists / 1024, counters / 1024, nq * nv * 4 / 1024))
  assert lists + counters + 12 * ns * k + 32 * nq <= 3 << 20
  assert growth < nq * nv * 4 // 4, growth
  # and the answers agree with each other: target t of set s is beaten by `greater` items, so it is in the list iff < k
  thr = index.target_scores(q, qw, tg, pooling=pool)
  inside = (indices == tg[:, None]).any(1)
  assert torch.equal(inside, greater < k) and bool((equal >= 1).all())
  assert bool((scores[:, -1] >= thr)[~inside].all())
