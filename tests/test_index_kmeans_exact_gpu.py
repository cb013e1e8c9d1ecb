"""The exact k-means update on the GPU (sum_scale, cell_sums_exact, cell_centroids(exact=True), train_cells(exact=True),
assign_cells on VideoIndex and ShardedVideoIndex; mmt_search_absmax, mmt_search_cell_sums_exact,
mmt_search_cell_centroids_exact).  The integer sums are compared with search.cell_sums_exact_ref bit for bit on the
fixture of test_index_kmeans_gpu.py, at the rounding edges of a term and over fp8 scales sixty binades apart; the fp32
values they give with the stated bound against fp64 and, on exact data, with the fp32 accumulator bit for bit; a
ShardedVideoIndex with the single index bit for bit, through the trainer, the assignment and the probed search."""
import math

import numpy as np
import pytest
import torch

from tests.test_index_kmeans_gpu import (CELLS, CONFIGS, DEV, EMPTY, FP8, IDS, MAIN, MAIN_IDS, PLANTED, U, ZERO_EXPERT,
                                         _bits, _cells, _configs, _data, _index, _labels, _labels_of, _planted,
                                         _planted_index, _same, _stored, _sums)

pytestmark = pytest.mark.gpu
_cache = {}


def _exact(kind, config):
  """cell_sums_exact of the fixture, once: (the ExactCellSums, its tensors on the host, the numpy restatement)."""
  from mmt_amd import search
  if (kind, config) not in _cache:
    index, cells = _index(kind, config), _cells(kind, config)
    got = index.cell_sums_exact(cells)
    weights = index.weights[:index.num_items]
    scale = search.sum_scale_ref(_stored(index), weights)
    ref = search.cell_sums_exact_ref(_stored(index), weights, cells.offsets, cells.items, scale)
    _cache[kind, config] = got, tuple(t.cpu().numpy() for t in (got.sums, got.wsums, got.counts)), scale, ref
  return _cache[kind, config]


def _host_sums(index, cells_of, got):
  """An ExactCellSums against the numpy restatement on the index's own stored rows: scale, integers, counts and the way
  back to fp32, all bit for bit."""
  from mmt_amd import search
  n = index.num_items
  scale = search.sum_scale_ref(_stored(index), index.weights[:n])
  assert got.scale == scale == index.sum_scale()
  ref = search.cell_sums_exact_ref(_stored(index), index.weights[:n], cells_of.offsets, cells_of.items, scale)
  assert got.sums.dtype is got.wsums.dtype is got.counts.dtype is torch.int64
  for mine, want in zip((got.sums, got.wsums, got.counts), ref):
    assert np.array_equal(mine.cpu().numpy(), want)
  fsums, fwsums, counts = got.float()
  assert np.array_equal(_bits(fsums.cpu().numpy()), _bits(search.exact_sums_float(ref[0], scale.exponent, scale.bits)))
  assert np.array_equal(_bits(fwsums.cpu().numpy()), _bits(search.exact_sums_float(ref[1], scale.wexponent, scale.bits)))
  assert torch.equal(counts, got.counts)
  return scale, ref


def _sums_of(index, labels, num_cells):
  cells = index.cells(torch.from_numpy(labels).to(DEV), num_cells)
  return cells, index.cell_sums_exact(cells)


# ------------------------------------------------------------------------------------------------------------ sums

@pytest.mark.parametrize('kind', ['exact', 'random'])
@pytest.mark.parametrize('config', CONFIGS, ids=IDS)
def test_sums_and_scale_equal_the_numpy_references(config, kind):
  from mmt_amd import search
  dtype, m, d = _configs()[config]
  index, cells = _index(kind, config), _cells(kind, config)
  got, (sums, wsums, counts), scale, ref = _exact(kind, config)
  assert type(got) is search.ExactCellSums and got.device == DEV
  assert got.scale == scale and index.sum_scale() == scale and index.sum_scale() is index.sum_scale()
  assert scale.bits == search.lse_bits(index.num_items) and scale.num_items == index.num_items
  assert sums.dtype == wsums.dtype == counts.dtype == np.int64 and sums.shape == (CELLS, m * d) and wsums.shape == (CELLS, m)
  assert np.array_equal(sums, ref[0]) and np.array_equal(wsums, ref[1]) and np.array_equal(counts, ref[2])
  assert counts[EMPTY] == 0 and not sums[EMPTY].any() and not wsums[EMPTY].any() and sums[1:].any(1).all()
  fsums, fwsums, fcounts = got.float()
  assert fsums.dtype is fwsums.dtype is torch.float32 and fcounts.dtype is torch.int64
  assert np.array_equal(_bits(fsums.cpu().numpy()), _bits(search.exact_sums_float(ref[0], scale.exponent, scale.bits)))
  assert np.array_equal(_bits(fwsums.cpu().numpy()), _bits(search.exact_sums_float(ref[1], scale.wexponent, scale.bits)))
  assert np.array_equal(fcounts.cpu().numpy(), counts)
  assert _same((index.cell_sums_exact(cells, scale=index.sum_scale()).sums,), (got.sums,))       # and a second call
  if kind == 'exact':   # every term and every fp32 partial sum is exact: the two accumulators agree in every bit
    (want, wwant, _), _ = _sums('exact', config)
    assert np.array_equal(_bits(fsums.cpu().numpy()), _bits(want)) and np.array_equal(_bits(fwsums.cpu().numpy()), _bits(wwant))
    assert _same(index.cell_centroids(cells, exact=True), index.cell_centroids(cells))


@pytest.mark.parametrize('config', CONFIGS, ids=IDS)
def test_exact_sums_and_centroids_against_fp64(config):
  """The fp32 values of the sums within n_c 2^(E - B - 1) + ulp32 / 2 of the fp64 sums of the stored rows (math.fsum: the
  correctly rounded sum, half an ulp64 more); the centroids from the device's own fp32 sums within the bound
  test_index_kmeans_gpu.py holds the float path's centroids to."""
  dtype, m, d = _configs()[config]
  index, cells = _index('random', config), _cells('random', config)
  got, (_, _, counts), scale, _ = _exact('random', config)
  fsums = got.float()[0].cpu().numpy()
  ids, rows = _labels(), _stored(index).astype(np.float64)
  worst = 0.0
  for c in range(CELLS):
    want = np.array([math.fsum(col) for col in rows[ids == c].T]) if counts[c] else np.zeros(m * d)
    bound = counts[c] * 2.0 ** (scale.exponent - scale.bits - 1) + np.spacing(np.abs(fsums[c])).astype(np.float64) / 2
    bound = bound + np.spacing(np.abs(want)) / 2
    err = np.abs(fsums[c].astype(np.float64) - want)
    worst = max(worst, float((err / bound).max()))
    assert (err <= bound).all(), c
  print('max error / bound = %.3f' % worst)
  embds, weights = index.cell_centroids(cells, exact=True)
  assert embds.dtype is weights.dtype is torch.float32 and tuple(embds.shape) == (CELLS, m, d) and tuple(weights.shape) == (CELLS, m)
  e, w = embds.cpu().numpy(), weights.cpu().numpy()
  assert np.isfinite(e).all() and np.isfinite(w).all()
  s64 = fsums.astype(np.float64).reshape(CELLS, m, d)
  norm = np.sqrt((s64 * s64).sum(2, keepdims=True))
  want = np.divide(s64, norm, out=np.zeros_like(s64), where=norm > 0)
  err = np.abs(e - want)
  print('max relative error / bound = %.3f' % float((err / np.maximum((d + 4) * U * np.abs(want), 1e-300)).max()))
  assert (err <= (d + 4) * U * np.abs(want)).all()
  live = counts > 0
  fw = got.float()[1].cpu().numpy()
  assert np.array_equal(_bits(w[live]), _bits(fw[live] / counts[live, None].astype(np.float32)))
  assert not e[ZERO_EXPERT, 1].any() and w[ZERO_EXPERT, 1] == 0 and e[ZERO_EXPERT, 0].any()
  assert not e[EMPTY].any() and not w[EMPTY].any()
  # an empty cell's rows in a prefilled out= are untouched, the others are what they were without it
  out = (torch.full((CELLS, m, d), 7.0, device=DEV), torch.full((CELLS, m), 7.0, device=DEV))
  back = index.cell_centroids(cells, out=out, exact=True, scale=index.sum_scale())
  assert back[0] is out[0] and back[1] is out[1]
  assert bool((out[0][EMPTY] == 7).all()) and bool((out[1][EMPTY] == 7).all())
  assert _same((out[0][1:], out[1][1:]), (embds[1:], weights[1:]))


def test_a_term_rounds_to_nearest_even_at_its_edges():
  """An fp32 index of 16 items, so B = 58, whose largest value is exactly 1.0, so E = 0 and the unit is 2^-58: members of
  half a unit (a tie, to 0), three halves (a tie, to 2), a subnormal, -0.0; and a cell whose members cancel in expert 1."""
  from mmt_amd import search
  from mmt_amd.search import VideoIndex
  n, m, d = 16, 2, 8
  bits = search.lse_bits(n)
  assert bits == 58
  half = np.float32(2.0 ** -(bits + 1))
  g = np.zeros((n, m, d), np.float32)
  gw = np.ones((n, m), np.float32)
  g[0, 0, 0] = 1.0
  g[1, 0, :6] = [half, -half, 3 * half, -3 * half, 2.0 ** -149, -0.0]
  g[2, 0, :6] = [half, -half, 3 * half, -3 * half, -2.0 ** -149, -0.0]
  g[3, 0, :6] = [2 * half, 0.75 * 2 * half, 5 * half, -5 * half, 0.5, -1.0]
  g[1:4, 1, :] = np.float32(0.25)
  rng = np.random.RandomState(4)
  g[4:10, 0] = rng.standard_normal((6, d)).astype(np.float32) / 4
  g[4:7, 1] = rng.standard_normal((3, d)).astype(np.float32) / 4
  g[7:10, 1] = -g[4:7, 1]                                           # expert 1 of cell 2 cancels exactly
  gw[4:10, 1] = 0.5
  gw[7, 0] = 0.0
  g[10:, :, :] = (rng.randint(-8, 9, size=(6, m, d)) / 8).astype(np.float32)
  labels = np.array([0] + [1] * 3 + [2] * 6 + [3] * 4 + [-1] * 2, np.int64)
  index = VideoIndex(torch.from_numpy(g).to(DEV), torch.from_numpy(gw).to(DEV))
  assert np.array_equal(_bits(_stored(index)), _bits((gw[:, :, None] * g).reshape(n, -1)))   # stored as given, -0.0 too
  cells, got = _sums_of(index, labels, 5)
  scale, ref = _host_sums(index, cells, got)
  assert (scale.exponent, scale.wexponent, scale.bits) == (0, 0, bits)
  sums = got.sums.cpu().numpy()
  assert sums[0, 0] == 2 ** bits and not sums[0, 1:].any()
  assert sums[1, :6].tolist() == [0 + 0 + 1, 0 + 0 + 1, 2 + 2 + 2, -2 - 2 - 2, 2 ** (bits - 1), -2 ** bits]   # 0.75 units -> 1; 2.5 units -> 2
  assert not sums[2, d:].any() and sums[2, :d].any() and not sums[4].any()
  assert got.wsums.cpu().numpy()[2].tolist() == [5 * 2 ** bits, 3 * 2 ** bits]
  embds, weights = index.cell_centroids(cells, exact=True)
  assert not embds[2, 1].any() and embds[2, 0].any() and float(weights[2, 1]) == 0.5
  assert bool(torch.isfinite(embds).all()) and not embds[4].any()


def test_fp8_rows_sixty_binades_apart():
  """fp8 rows whose magnitudes span 2^-40 .. 2^20: under E of the largest the small rows' terms round to 0 or to small
  integers, and the code x scale product has to be formed exactly as `cell_sums` forms it."""
  from mmt_amd import search
  from mmt_amd.search import VideoIndex
  n, m, d = 200, 2, 16
  rng = np.random.RandomState(6)
  power = rng.randint(-40, 21, size=n)
  power[:4] = [20, -40, -34, -33]
  g = (rng.standard_normal((n, m, d)) * 2.0 ** power[:, None, None]).astype(np.float32)
  gw = np.ones((n, m), np.float32)
  labels = rng.randint(-1, 6, size=n).astype(np.int64)
  index = VideoIndex(torch.from_numpy(g).to(DEV), torch.from_numpy(gw).to(DEV), dtype=FP8)
  cells, got = _sums_of(index, labels, 7)
  scale, ref = _host_sums(index, cells, got)
  assert 20 <= scale.exponent <= 24 and scale.bits == 54
  stored = _stored(index)
  unit = 2.0 ** (scale.exponent - scale.bits)
  small = np.abs(stored).max(1) < unit / 2
  tiny = (np.abs(stored).max(1) >= unit / 2) & (np.abs(stored).max(1) < 64 * unit)
  print('%d rows below half a unit, %d rows of a few units' % (small.sum(), tiny.sum()))
  assert small.sum() >= 5 and tiny.sum() >= 5 and (labels[small] >= 0).any() and (labels[tiny] >= 0).any()
  embds, weights = index.cell_centroids(cells, exact=True)
  assert bool(torch.isfinite(embds).all()) and int(got.counts[6]) == 0 and not embds[6].any()


@pytest.mark.parametrize('config', MAIN, ids=MAIN_IDS)
def test_the_sums_depend_on_the_items_as_a_set(config):
  """The same items inserted in a random permutation, the labels permuted alike: identical integers, identical scale,
  identical centroids cell by cell."""
  from mmt_amd.search import VideoIndex
  dtype, m, d = _configs()[config]
  index, cells = _index('random', config), _cells('random', config)
  got, _, scale, _ = _exact('random', config)
  g, gw = _data('random', m, d)
  perm = np.random.RandomState(11).permutation(len(g))
  other = VideoIndex(torch.from_numpy(g[perm]).to(DEV), torch.from_numpy(gw[perm]).to(DEV), dtype=dtype)
  other_cells = other.cells(torch.from_numpy(_labels()[perm]).to(DEV), CELLS)
  again = other.cell_sums_exact(other_cells)
  assert again.scale == scale and again.scale is not got.scale
  assert _same((again.sums, again.wsums, again.counts), (got.sums, got.wsums, got.counts))
  assert _same(other.cell_centroids(other_cells, exact=True), index.cell_centroids(cells, exact=True))


# -------------------------------------------------------------------------------------------------------- sharding

def _placements(g, gw, labels, dtype):
  """(name, sharded index, the single index over the same items in the same order, their labels), all shards on one
  device: contiguous ranges; uneven `add` chunks, so that the shards interleave; one small `add` that leaves two shards
  empty."""
  from mmt_amd.search import ShardedVideoIndex, VideoIndex
  n, m, d = g.shape
  tg, tgw = torch.from_numpy(g).to(DEV), torch.from_numpy(gw).to(DEV)
  single = VideoIndex(tg, tgw, dtype=dtype)
  yield 'contiguous', ShardedVideoIndex(tg, tgw, [DEV] * 3, dtype=dtype), single, labels
  chunks = ShardedVideoIndex.empty(n, m, d, [DEV] * 3, dtype=dtype)
  at = 0
  for size in (100, 7, 333, 50, 1, 260, n):
    chunks.add(tg[at:at + size], tgw[at:at + size])
    at = min(n, at + size)
    if at == n:
      break
  assert chunks.num_items == n and min(chunks.shard_sizes) > 0
  order = torch.cat([sh.ids[:sh.num_items] for sh in chunks.shards])
  assert not bool((order[1:] > order[:-1]).all())                    # the shards do interleave
  yield 'chunks', chunks, single, labels
  few = 300
  lonely = ShardedVideoIndex.empty(3 * n, m, d, [DEV] * 3, dtype=dtype)
  lonely.add(tg[:few], tgw[:few])
  assert lonely.shard_sizes == [few, 0, 0]
  yield 'two shards empty', lonely, VideoIndex(tg[:few], tgw[:few], dtype=dtype), labels[:few]


@pytest.mark.parametrize('config', MAIN, ids=MAIN_IDS)
def test_a_sharded_index_gives_the_single_index_bit_for_bit(config):
  from mmt_amd.search import ExactCellSums, ShardedCells
  dtype, m, d = _configs()[config]
  g, gw = _data('random', m, d)
  for name, sharded, single, labels in _placements(g, gw, _labels(), dtype):
    ids = torch.from_numpy(labels).to(DEV)
    cells, want_cells = sharded.cells(ids, CELLS), single.cells(ids, CELLS)
    assert type(cells) is ShardedCells
    assert sharded.sum_scale() == single.sum_scale(), name
    got, want = sharded.cell_sums_exact(cells), single.cell_sums_exact(want_cells)
    assert type(got) is ExactCellSums and got.device == DEV
    assert _same((got.sums, got.wsums, got.counts), (want.sums, want.wsums, want.counts)), name
    assert _same(got.float(), want.float()), name
    centroids = single.cell_centroids(want_cells, exact=True)
    assert _same(sharded.cell_centroids(cells, exact=True), centroids), name
    out = (torch.full((CELLS, m, d), 7.0, device=DEV), torch.full((CELLS, m), 7.0, device=DEV))
    want_out = (out[0].clone(), out[1].clone())
    back = sharded.cell_centroids(cells, out=out, exact=True, scale=sharded.sum_scale())
    assert back[0] is out[0] and back[1] is out[1]
    assert _same(out, single.cell_centroids(want_cells, out=want_out, exact=True)), name
    assert bool((out[0][EMPTY] == 7).all()) and bool((out[1][EMPTY] == 7).all())


def _trained(dtype, name, **how):
  """(single index, sharded index with interleaved shards, single quantiser, sharded quantiser) on the planted clusters;
  `name` names the arguments in the cache."""
  from mmt_amd.search import ShardedVideoIndex
  key = ('trained', dtype, name)
  if key not in _cache:
    g, gw, _, _ = _planted()
    single = _planted_index(dtype)
    if ('sharded', dtype) not in _cache:
      tg, tgw = torch.from_numpy(g).to(DEV), torch.from_numpy(gw).to(DEV)
      sharded = ShardedVideoIndex.empty(len(g), 3, 64, [DEV] * 3, dtype=dtype)
      at = 0
      for size in (100, 7, 333, 50, 1, 260, len(g)):
        sharded.add(tg[at:at + size], tgw[at:at + size])
        at = min(len(g), at + size)
        if at == len(g):
          break
      _cache['sharded', dtype] = sharded
    sharded = _cache['sharded', dtype]
    _cache[key] = single, sharded, single.train_cells(PLANTED, exact=True, **how), sharded.train_cells(PLANTED, exact=True, **how)
  return _cache[key]


def _same_quantiser(a, b):
  return (a.iterations == b.iterations and a.exact is b.exact is True and a.scale == b.scale and
          _same((a.embds, a.weights, a.objective, a.moved), (b.embds, b.weights, b.objective, b.moved)) and
          _same((a.centroids.folded, a.centroids.weights), (b.centroids.folded, b.centroids.weights)))


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16, FP8], ids=MAIN_IDS)
def test_the_sharded_trainer_is_the_single_trainer_bit_for_bit(dtype):
  from mmt_amd.search import CellQuantiser, VideoIndex
  single, sharded, q, sq = _trained(dtype, 'seeded', iters=8, seed=0)
  assert type(sq) is CellQuantiser and type(sq.centroids) is VideoIndex and sq.centroids.device == DEV
  assert (sq.centroids.num_items, sq.centroids.dtype, sq.num_cells) == (PLANTED, dtype, PLANTED)
  assert _same_quantiser(q, sq)
  print('objective', q.objective.cpu().numpy(), 'moved', q.moved.cpu().numpy())
  assert float(q.objective[-1]) >= float(q.objective[0]) and int(q.moved[-1]) == 0 and q.iterations <= 8
  assert q.objective.dtype is torch.float32 and q.moved.dtype is torch.int64
  # a second run repeats itself
  assert _same_quantiser(sq, sharded.train_cells(PLANTED, iters=8, seed=0, exact=True))
  assert _same_quantiser(q, single.train_cells(PLANTED, iters=8, seed=0, exact=True))
  # the labels
  assert np.array_equal(_labels_of(sharded.assign_cells(sq)), _labels_of(single.assign_cells(q)))


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16, FP8], ids=MAIN_IDS)
def test_one_exact_iteration_recovers_planted_clusters_with_init_and_with_a_sample(dtype):
  """The standard test_index_kmeans_gpu.py applies to the float trainer: from the first item of each cluster, one
  iteration's centroids assign every item to its planted cluster (in fp64 the gap is above 0.1)."""
  _, _, planted, init = _planted()
  start = torch.from_numpy(init).to(DEV)
  single, sharded, q, sq = _trained(dtype, 'one iteration', iters=1, init=start)
  assert _same_quantiser(q, sq) and q.iterations == 1
  assert np.array_equal(_labels_of(single.assign_cells(q)), planted)
  assert np.array_equal(_labels_of(sharded.assign_cells(sq)), planted)
  # a training sample: every second item and the starts; order and repeats do not matter
  sample = torch.unique(torch.cat([torch.arange(0, len(planted), 2, device=DEV), start]))
  half = single.train_cells(PLANTED, iters=2, init=start, items=sample, exact=True)
  shalf = sharded.train_cells(PLANTED, iters=2, init=start, items=sample.flip(0).repeat(2), exact=True)
  assert _same_quantiser(half, shalf) and int(half.moved[0]) <= sample.shape[0]
  assert not _same((half.embds,), (q.embds,))


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16, FP8], ids=MAIN_IDS)
def test_assignment_and_probed_search_on_trained_cells(dtype):
  from mmt_amd.search import IndexCells, ShardedCells
  g = _planted()[0]
  single, sharded, q, sq = _trained(dtype, 'seeded', iters=8, seed=0)
  floaty = single.train_cells(PLANTED, iters=2, seed=0)
  assert floaty.exact is False and floaty.scale is None
  for quantiser in (q, sq, floaty):
    want = quantiser.assign(single)
    mine, cells = single.assign_cells(quantiser), sharded.assign_cells(quantiser)
    assert type(mine) is IndexCells and type(cells) is ShardedCells and mine.quantiser is cells.quantiser is quantiser
    assert _same((cells.offsets, cells.items), (want.offsets, want.items))
    assert _same((mine.offsets, mine.items), (want.offsets, want.items))
    assert np.array_equal(np.sort(cells.items.cpu().numpy()), np.arange(single.num_items))
  gen = torch.Generator(device=DEV).manual_seed(9)
  queries, weights = torch.randn(130, 3, 64, device=DEV, generator=gen), torch.rand(130, 3, device=DEV, generator=gen)
  queries[:40] = torch.from_numpy(g[100:140]).to(DEV)
  cells, want = sharded.assign_cells(sq), single.assign_cells(q)
  assert torch.equal(cells.probes(queries, weights, 4), want.probes(queries, weights, 4))
  got = sharded.search_cells(queries, weights, cells, nprobe=4, k=10)
  assert _same(got, single.search_cells(queries, weights, want, nprobe=4, k=10))
  assert _same(sharded.search_cells(queries, weights, cells, nprobe=PLANTED, k=10), single.search(queries, weights, k=10))


def test_refusals_leave_both_indexes_usable():
  from mmt_amd import search
  from mmt_amd.search import ShardedVideoIndex, SumScale, VideoIndex
  g, gw, planted, init = _planted()
  tg, tgw = torch.from_numpy(g).to(DEV), torch.from_numpy(gw).to(DEV)
  n = 1000
  single = VideoIndex.empty(len(g), 3, 64, DEV)
  sharded = ShardedVideoIndex.empty(len(g), 3, 64, [DEV] * 2)
  gen = torch.Generator(device=DEV).manual_seed(2)
  queries, weights = torch.randn(9, 3, 64, device=DEV, generator=gen), torch.rand(9, 3, device=DEV, generator=gen)
  other = VideoIndex(tg[:n], tgw[:n])
  for index in (single, sharded):
    index.add(tg[:n], tgw[:n])
    cells = index.cells(torch.from_numpy(planted[:n]).to(DEV), PLANTED)
    scale = index.sum_scale()
    quantiser = index.train_cells(PLANTED, iters=1, init=torch.from_numpy(init).to(DEV), exact=True)
    assert quantiser.scale == scale
    kept = index.cell_sums_exact(cells)
    with pytest.raises(ValueError, match='cell_sums_exact: the scale belongs to another index'):
      index.cell_sums_exact(cells, scale=other.sum_scale())
    index.add(tg[n:], tgw[n:])                                       # cells, scale and quantiser cells are stale now
    want = index.search(queries, weights, k=5)
    assert index.sum_scale() is not scale and index.sum_scale().num_items == len(g)
    fresh = index.cells(torch.from_numpy(planted).to(DEV), PLANTED)
    for who, call in (('cell_sums_exact', lambda **kw: index.cell_sums_exact(fresh, **kw)),
                      ('cell_centroids', lambda **kw: index.cell_centroids(fresh, exact=True, **kw))):
      with pytest.raises(ValueError, match='%s: the scale was built for %d items, the index holds %d' % (who, n, len(g))):
        call(scale=scale)
      with pytest.raises(ValueError, match='%s: scale must be a SumScale' % who):
        call(scale=kept)
    with pytest.raises(ValueError, match='cell_sums_exact: the cells were built for %d items' % n):
      index.cell_sums_exact(cells)
    with pytest.raises(ValueError, match='cell_centroids: the cells were built for %d items' % n):
      index.cell_centroids(cells, exact=True)
    for bad in (1, None):
      with pytest.raises(ValueError, match='exact must be a bool'):
        index.cell_centroids(fresh, exact=bad)
    with pytest.raises(ValueError, match='cell_centroids: scale= goes with exact=True'):
      index.cell_centroids(fresh, scale=index.sum_scale())
    # a scale made by hand for this many items, wide enough, is taken; it gives other integers and the same kind of result
    wide = SumScale(index.sum_scale().exponent + 3, index.sum_scale().wexponent, search.lse_bits(len(g)), len(g))
    assert _same((index.cell_sums_exact(fresh, scale=wide).counts,), (fresh.sizes,))
    assert _same(index.search(queries, weights, k=5), want)
  with pytest.raises(ValueError, match='cells must come from'):
    single.cell_sums_exact(sharded.cells(torch.from_numpy(planted).to(DEV), PLANTED))
  ids = torch.from_numpy(planted).to(DEV)
  for who, args in (('train_cells', (PLANTED,)), ('cell_sums', (sharded.cells(ids, PLANTED),)),
                    ('cell_centroids', (sharded.cells(ids, PLANTED),))):
    with pytest.raises(ValueError, match='%s: not available on a ShardedVideoIndex' % who):
      getattr(sharded, who)(*args)
  with pytest.raises(ValueError, match='assign: not available on a ShardedVideoIndex'):
    single.train_cells(PLANTED, iters=1, exact=True).assign(sharded)
  assert _same(sharded.search(queries, weights, k=5), single.search(queries, weights, k=5))
