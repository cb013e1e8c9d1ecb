"""The k-means cells on the GPU (VideoIndex.cell_sums, cell_centroids, train_cells, CellQuantiser; mmt_search_cell_sums,
mmt_search_cell_centroids).  The sums are compared with search.cell_sums_ref bit for bit and with fp64 -- equal on exact
data, within the bound of a sequential sum on random data; the centroids with fp64 from the device's own sums; the
trainer with the public pieces called by hand, with its own second run, and on planted clusters whose separation the test
measures in fp64 first."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
FP8 = torch.float8_e4m3fn
U = 2.0 ** -24
_cache = {}


def _configs():
  """(dtype, M, d): (3, 64) on the three dtypes, (2, 16) on fp8, (7, 32) on fp32, and M = 7 with the least d that takes
  M * d across the kernel's column slab, on the three dtypes."""
  from mmt_amd import search
  d = (search.SUM_SLAB // 7 // 16 + 1) * 16
  assert 7 * d > search.SUM_SLAB > 7 * (d - 16) and (7 * d) % search.SUM_SLAB
  return [(torch.float32, 3, 64), (torch.bfloat16, 3, 64), (FP8, 3, 64), (FP8, 2, 16), (torch.float32, 7, 32),
          (torch.float32, 7, d), (torch.bfloat16, 7, d), (FP8, 7, d)]


CONFIGS = range(8)
IDS = ['fp32-3x64', 'bf16-3x64', 'fp8-3x64', 'fp8-2x16', 'fp32-7x32', 'fp32-slab', 'bf16-slab', 'fp8-slab']
MAIN, MAIN_IDS = range(3), IDS[:3]
EMPTY, ONE, ZERO_EXPERT = 0, 1, 2     # cells: no item; one item; every member without expert 1
CELLS = 12


def _labels():
  """int64 [NV] on the host: cell 0 empty, cell 1 one item, cells 2 .. 5 of SUM_PIECE - 1, SUM_PIECE, SUM_PIECE + 1 and
  2 SUM_PIECE + 1 items, cells 6 .. 11 of 20 .. 50 items and 40 items in no cell, interleaved at random: about 1 500."""
  from mmt_amd import search
  if 'labels' not in _cache:
    rng = np.random.RandomState(25)
    p = search.SUM_PIECE
    sizes = [0, 1, p - 1, p, p + 1, 2 * p + 1] + list(rng.randint(20, 51, size=CELLS - 6))
    ids = np.concatenate([np.full(n, c) for c, n in enumerate(sizes)] + [np.full(40, -1)]).astype(np.int64)
    rng.shuffle(ids)
    _cache['labels'] = ids
  return _cache['labels']


def _data(kind, m, d):
  """The gallery on the host, float32.  'exact': G in k / 8 with |k| <= 8 and weights in {0, 1/4, 1/2} -- the folded
  values are exact in fp32, bf16 and e4m3 and every partial sum of them is exact in fp32.  'random': rows of about unit
  length, weights uniform in [0, 1) with a tenth of them 0.  In both the members of cell ZERO_EXPERT have weight 0 for
  expert 1 and the item of cell ONE has every weight above 0."""
  if (kind, m, d) not in _cache:
    ids = _labels()
    rng = np.random.RandomState(1000 * m + d)
    nv = ids.shape[0]
    if kind == 'exact':
      g = (rng.randint(-8, 9, size=(nv, m, d)) / 8).astype(np.float32)
      gw = (rng.randint(0, 3, size=(nv, m)) / 4).astype(np.float32)
      gw[ids == ONE] = 0.5
    else:
      g = (rng.standard_normal((nv, m, d)) / np.sqrt(d)).astype(np.float32)
      gw = (rng.random_sample((nv, m)) * (rng.random_sample((nv, m)) > 0.1)).astype(np.float32)
      gw[ids == ONE] = rng.random_sample(m).astype(np.float32) * 0.5 + 0.25
    gw[ids == ZERO_EXPERT, 1] = 0
    _cache[kind, m, d] = g, gw
  return _cache[kind, m, d]


def _index(kind, config):
  from mmt_amd.search import VideoIndex
  dtype, m, d = _configs()[config]
  if ('index', kind, config) not in _cache:
    g, gw = _data(kind, m, d)
    _cache['index', kind, config] = VideoIndex(torch.from_numpy(g).to(DEV), torch.from_numpy(gw).to(DEV), dtype=dtype)
  return _cache['index', kind, config]


def _stored(index):
  """The stored rows of an index dequantised, on the host: float32 [num_items, M * d], exact."""
  n = index.num_items
  rows = index.folded[:n].to(torch.float32)
  if index.scales is not None:
    rows = rows * index.scales[:n, None]
  return rows.cpu().numpy()


def _cells(kind, config):
  if ('cells', kind, config) not in _cache:
    _cache['cells', kind, config] = _index(kind, config).cells(torch.from_numpy(_labels()).to(DEV), CELLS)
  return _cache['cells', kind, config]


def _sums(kind, config):
  """cell_sums of the fixture, once, on the host, and the numpy restatement of it."""
  from mmt_amd import search
  if ('sums', kind, config) not in _cache:
    index, cells = _index(kind, config), _cells(kind, config)
    got = tuple(t.cpu().numpy() for t in index.cell_sums(cells))
    ref = search.cell_sums_ref(_stored(index), index.weights[:index.num_items], cells.offsets, cells.items)
    _cache['sums', kind, config] = got, ref
  return _cache['sums', kind, config]


def _bits(x):
  return np.ascontiguousarray(x).view(np.int32)


def _same(a, b):
  return all(x.dtype == y.dtype and x.shape == y.shape and
             torch.equal(x.view(torch.int32) if x.dtype is torch.float32 else x, y.view(torch.int32) if y.dtype is torch.float32 else y)
             for x, y in zip(a, b))


def _labels_of(cells):
  """int64 [num_items] on the host: the cell of every item, -1 = in none; every item at most once."""
  items = cells.items.cpu().numpy()
  assert len(np.unique(items)) == len(items)
  ids = np.full(cells.num_items, -1, np.int64)
  ids[items] = np.repeat(np.arange(cells.num_cells), cells.sizes.cpu().numpy())
  return ids


# ------------------------------------------------------------------------------------------------------------ sums

@pytest.mark.parametrize('config', CONFIGS, ids=IDS)
def test_sums_of_exact_data_equal_the_fp64_sums(config):
  index = _index('exact', config)
  (sums, wsums, counts), ref = _sums('exact', config)
  ids, rows, weights = _labels(), _stored(index).astype(np.float64), index.weights[:index.num_items].cpu().numpy().astype(np.float64)
  g, gw = _data('exact', *_configs()[config][1:])
  assert np.array_equal(rows, (gw[:, :, None].astype(np.float64) * g).reshape(len(ids), -1))   # stored without rounding
  assert sums.dtype == wsums.dtype == np.float32 and counts.dtype == np.int64
  for c in range(CELLS):
    assert np.array_equal(sums[c], rows[ids == c].sum(0)), c
    assert np.array_equal(wsums[c], weights[ids == c].sum(0)), c
    assert counts[c] == (ids == c).sum()
  assert counts[EMPTY] == 0 and not sums[EMPTY].any() and not wsums[EMPTY].any() and counts[ONE] == 1
  assert np.array_equal(_bits(sums), _bits(ref[0])) and np.array_equal(_bits(wsums), _bits(ref[1]))
  assert np.array_equal(counts, ref[2])


@pytest.mark.parametrize('config', CONFIGS, ids=IDS)
def test_sums_of_random_data_have_the_stated_order_and_its_bound(config):
  """Bit-equal to the numpy restatement; and within the bound of a sequential fp32 sum in that order: an element goes
  through at most min(n, SUM_PIECE) adds inside its piece and `pieces` adds across them."""
  from mmt_amd import search
  index = _index('random', config)
  (sums, wsums, counts), ref = _sums('random', config)
  assert np.array_equal(_bits(sums), _bits(ref[0])) and np.array_equal(_bits(wsums), _bits(ref[1]))
  assert np.array_equal(counts, ref[2])
  ids, rows = _labels(), _stored(index).astype(np.float64)
  for c in range(CELLS):
    n = int((ids == c).sum())
    pieces = -(-n // search.SUM_PIECE)
    bound = (min(n, search.SUM_PIECE) + pieces) * U * np.abs(rows[ids == c]).sum(0)
    err = np.abs(sums[c] - rows[ids == c].sum(0))
    print('cell %d: n = %d, max error / bound = %.3f' % (c, n, float((err / np.maximum(bound, 1e-300)).max()) if n else 0.0))
    assert (err <= bound).all(), c
  assert sums[1:].any(1).all()


# ------------------------------------------------------------------------------------------------------- centroids

@pytest.mark.parametrize('kind', ['exact', 'random'])
@pytest.mark.parametrize('config', CONFIGS, ids=IDS)
def test_centroids_against_fp64_from_the_devices_own_sums(config, kind):
  dtype, m, d = _configs()[config]
  index, cells = _index(kind, config), _cells(kind, config)
  (sums, wsums, counts), _ = _sums(kind, config)
  embds, weights = index.cell_centroids(cells)
  assert embds.dtype is weights.dtype is torch.float32 and tuple(embds.shape) == (CELLS, m, d) and tuple(weights.shape) == (CELLS, m)
  e, w = embds.cpu().numpy(), weights.cpu().numpy()
  assert np.isfinite(e).all() and np.isfinite(w).all()
  s64 = sums.astype(np.float64).reshape(CELLS, m, d)
  norm = np.sqrt((s64 * s64).sum(2, keepdims=True))
  want = np.divide(s64, norm, out=np.zeros_like(s64), where=norm > 0)
  err = np.abs(e - want)
  print('max relative error / bound = %.3f' % float((err / np.maximum((d + 4) * U * np.abs(want), 1e-300)).max()))
  assert (err <= (d + 4) * U * np.abs(want)).all()
  live = counts > 0
  assert np.array_equal(_bits(w[live]), _bits(wsums[live] / counts[live, None].astype(np.float32)))
  # a zero S[m]: a zero row with weight 0, and no NaN; an empty cell: zeros, as the buffers were made
  assert not sums.reshape(CELLS, m, d)[ZERO_EXPERT, 1].any() and not e[ZERO_EXPERT, 1].any() and w[ZERO_EXPERT, 1] == 0
  assert e[ZERO_EXPERT, 0].any() and not e[EMPTY].any() and not w[EMPTY].any()
  # an empty cell's rows in a prefilled out= are untouched, the others are what they were without it
  out = (torch.full((CELLS, m, d), 7.0, device=DEV), torch.full((CELLS, m), 7.0, device=DEV))
  back = index.cell_centroids(cells, out=out)
  assert back[0] is out[0] and back[1] is out[1]
  assert bool((out[0][EMPTY] == 7).all()) and bool((out[1][EMPTY] == 7).all())
  assert _same((out[0][1:], out[1][1:]), (embds[1:], weights[1:]))


@pytest.mark.parametrize('config', [0, 4, 5], ids=['fp32-3x64', 'fp32-7x32', 'fp32-slab'])
def test_the_centroid_of_a_one_item_cell_is_the_item(config):
  """On fp32: the item's unfolded row, normalised, within the centroid bound (the fold's one rounding per element is well
  inside it), and its weights exactly."""
  dtype, m, d = _configs()[config]
  index, cells = _index('random', config), _cells('random', config)
  g, gw = _data('random', m, d)
  item = int(np.flatnonzero(_labels() == ONE)[0])
  embds, weights = index.cell_centroids(cells)
  g64 = g[item].astype(np.float64)
  want = g64 / np.sqrt((g64 * g64).sum(1, keepdims=True))
  assert (np.abs(embds[ONE].cpu().numpy() - want) <= (d + 4) * U * np.abs(want)).all()
  assert np.array_equal(_bits(weights[ONE].cpu().numpy()), _bits(gw[item]))


# ------------------------------------------------------------------------------------------------------ invariance

@pytest.mark.parametrize('config', [0, 1, 2, 7], ids=['fp32-3x64', 'bf16-3x64', 'fp8-3x64', 'fp8-slab'])
def test_a_cells_sums_depend_on_its_member_list_alone(config):
  from mmt_amd.search import VideoIndex
  dtype, m, d = _configs()[config]
  index = _index('random', config)
  (sums, wsums, counts), _ = _sums('random', config)
  ids = _labels()
  keep = (3, 5, 9)
  # the other cells relabelled, and more cells
  rng = np.random.RandomState(7)
  other = np.where(np.isin(ids, keep), ids, rng.choice([-1, 0, 1, 2, 4, 6, 7, 8, 10, 11, 12, 17], size=ids.shape))
  got = [t.cpu().numpy() for t in index.cell_sums(index.cells(torch.from_numpy(other).to(DEV), CELLS + 7))]
  assert got[0].shape == (CELLS + 7, m * d)
  for c in keep:
    assert np.array_equal(_bits(got[0][c]), _bits(sums[c])) and np.array_equal(_bits(got[1][c]), _bits(wsums[c])), c
    assert got[2][c] == counts[c]
  grown = [t.cpu().numpy() for t in index.cell_sums(index.cells(torch.from_numpy(ids).to(DEV), CELLS + 300))]
  assert np.array_equal(_bits(grown[0][:CELLS]), _bits(sums)) and not grown[0][CELLS:].any() and not grown[2][CELLS:].any()
  # items added behind, in a rebuilt index
  g, gw = (torch.from_numpy(x).to(DEV) for x in _data('random', m, d))
  rebuilt = VideoIndex.empty(len(ids) + 300, m, d, DEV, dtype=dtype)
  rebuilt.add(g, gw)
  rebuilt.add(g[:300].flip(0), gw[:300].flip(0))
  more = np.concatenate([ids, rng.choice([-1, 0, 1, 2, 4, 6], size=300)])
  got = [t.cpu().numpy() for t in rebuilt.cell_sums(rebuilt.cells(torch.from_numpy(more).to(DEV), CELLS))]
  for c in keep:
    assert np.array_equal(_bits(got[0][c]), _bits(sums[c])) and np.array_equal(_bits(got[1][c]), _bits(wsums[c])), c
  # and a second call
  assert _same(index.cell_sums(_cells('random', config)), index.cell_sums(_cells('random', config)))


# --------------------------------------------------------------------------------------------------------- trainer

@pytest.mark.parametrize('config', MAIN, ids=MAIN_IDS)
def test_the_trainer_is_its_public_pieces_and_deterministic(config):
  from mmt_amd.search import CellQuantiser, IndexCells, VideoIndex
  dtype, m, d = _configs()[config]
  index = _index('random', config)
  n, c = index.num_items, 20
  init = torch.from_numpy(np.random.RandomState(3).permutation(n)[:c].astype(np.int64)).to(DEV)
  q = index.train_cells(c, iters=3, init=init)
  assert type(q) is CellQuantiser and q.num_cells == c and 1 <= q.iterations <= 3
  assert type(q.centroids) is VideoIndex and (q.centroids.num_items, q.centroids.dtype) == (c, dtype)
  assert tuple(q.embds.shape) == (c, m, d) and tuple(q.weights.shape) == (c, m)
  assert q.objective.device == q.moved.device == DEV and q.objective.shape == q.moved.shape == (q.iterations,)
  cells = q.assign(index)
  assert type(cells) is IndexCells and cells.quantiser is q and cells.num_cells == c
  labels = _labels_of(cells)
  assert np.array_equal(labels, q.centroids.neighbours(k=1, source=index)[1][:, 0].cpu().numpy())
  assert np.array_equal(np.sort(cells.items.cpu().numpy()), np.arange(n))            # every item in exactly one cell
  again = index.train_cells(c, iters=3, init=init)
  assert _same((q.embds, q.weights, q.objective, q.moved), (again.embds, again.weights, again.objective, again.moved))
  assert np.array_equal(_labels_of(again.assign(index)), labels)
  assert _same((q.centroids.folded, q.centroids.weights), (again.centroids.folded, again.centroids.weights))
  # one iteration by hand: singleton cells -> cell_centroids -> neighbours -> cells -> cell_centroids
  ids = torch.full((n,), -1, dtype=torch.int64, device=DEV)
  ids[init] = torch.arange(c, device=DEV)
  e0, w0 = index.cell_centroids(index.cells(ids, c))
  s, best = VideoIndex(e0, w0, dtype=dtype).neighbours(k=1, source=index)
  assert int(torch.bincount(best[:, 0], minlength=c).min()) > 0                       # no cell to re-seed here
  e1, w1 = index.cell_centroids(index.cells(best[:, 0].contiguous(), c), out=(e0.clone(), w0.clone()))
  one = index.train_cells(c, iters=1, init=init)
  assert one.iterations == 1 and _same((one.embds, one.weights), (e1, w1))
  assert _same((one.objective, one.moved), (s.mean().reshape(1), (best[:, 0] != ids).sum().reshape(1)))
  # a training sample: the items outside it take no part
  sample = torch.arange(0, n, 2, device=DEV)
  half = index.train_cells(c, iters=2, init=sample[:c], items=sample)
  ids.fill_(-1)
  ids[sample[:c]] = torch.arange(c, device=DEV)
  s, _ = VideoIndex(*index.cell_centroids(index.cells(ids, c)), dtype=dtype).neighbours(k=1, source=index, items=sample)
  assert _same((half.objective[:1],), (s.mean().reshape(1),)) and int(half.moved[0]) <= sample.shape[0]
  mixed = index.train_cells(c, iters=2, init=sample[:c], items=sample.flip(0).repeat(2))   # order and repeats do not matter
  assert _same((half.embds, half.weights, half.objective, half.moved), (mixed.embds, mixed.weights, mixed.objective, mixed.moved))


# ------------------------------------------------------------------------------------------------- planted clusters

PLANTED = 12


def _planted(noise=0.5, seed=0, m=3, d=64, nv=1500):
  """12 unit centres per expert; item = centre + noise * (unit-variance noise / sqrt(d)), renormalised; weights uniform in
  [0.2, 1] with 15 % of the modalities missing (an item that would lose all three keeps its first).  -> (G float32
  [nv, m, d], gw float32 [nv, m], the planted labels int64 [nv], init: the first item of each cluster)."""
  if ('planted', noise, seed) not in _cache:
    rng = np.random.RandomState(100 + seed)
    centres = rng.standard_normal((PLANTED, m, d))
    centres /= np.linalg.norm(centres, axis=2, keepdims=True)
    labels = rng.randint(0, PLANTED, size=nv)
    labels[:PLANTED] = np.arange(PLANTED)
    g = centres[labels] + noise * rng.standard_normal((nv, m, d)) / np.sqrt(d)
    g /= np.linalg.norm(g, axis=2, keepdims=True)
    gw = rng.uniform(0.2, 1.0, size=(nv, m))
    missing = rng.random_sample((nv, m)) < 0.15
    missing[missing.all(1), 0] = False
    gw[missing] = 0
    init = np.array([np.flatnonzero(labels == c)[0] for c in range(PLANTED)], np.int64)
    _cache['planted', noise, seed] = g.astype(np.float32), gw.astype(np.float32), labels.astype(np.int64), init
  return _cache['planted', noise, seed]


def _sims64(g, gw, ce, cw):
  """The score of every item under every centroid in fp64: sum_m gw gw_c <G, G_c> / sum_m gw gw_c (0 -> 1e-5)."""
  num = np.einsum('nm,cm,nmd,cmd->nc', gw, cw, g, ce)
  den = gw @ cw.T
  return num / np.where(den == 0, 1e-5, den)


def _centroids64(g, gw, labels, c, previous=None):
  ce, cw = (np.zeros((c,) + g.shape[1:]), np.zeros((c, g.shape[1]))) if previous is None else (previous[0].copy(), previous[1].copy())
  for k in range(c):
    if (labels == k).any():
      s = (gw[labels == k, :, None] * g[labels == k]).sum(0)
      norm = np.linalg.norm(s, axis=1, keepdims=True)
      ce[k] = np.divide(s, norm, out=np.zeros_like(s), where=norm > 0)
      cw[k] = gw[labels == k].mean(0)
  return ce, cw


def _planted_index(dtype, **kw):
  from mmt_amd.search import VideoIndex
  g, gw, _, _ = _planted(**kw)
  key = ('planted index', dtype, tuple(sorted(kw.items())))
  if key not in _cache:
    _cache[key] = VideoIndex(torch.from_numpy(g).to(DEV), torch.from_numpy(gw).to(DEV), dtype=dtype)
  return _cache[key]


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16, FP8], ids=MAIN_IDS)
def test_one_iteration_recovers_planted_clusters(dtype):
  """The fixture decides the outcome, not the kernel: in fp64 the second assignment equals the planted labels with a gap
  between the best and the second centroid above 0.1, far above the rounding of any stored dtype."""
  g, gw, planted, init = _planted()
  g64, gw64 = g.astype(np.float64), gw.astype(np.float64)
  first = np.argmax(_sims64(g64, gw64, *_centroids64(g64, gw64, np.where(np.isin(np.arange(len(planted)), init), planted, -1),
                                                       PLANTED)), 1)
  sims = np.sort(_sims64(g64, gw64, *_centroids64(g64, gw64, first, PLANTED)), 1)
  second = np.argmax(_sims64(g64, gw64, *_centroids64(g64, gw64, first, PLANTED)), 1)
  gap = float((sims[:, -1] - sims[:, -2]).min())
  print('fp64: %d items off after the first assignment, smallest gap of the second %.3f' % ((first != planted).sum(), gap))
  assert np.array_equal(second, planted) and gap > 0.1
  index = _planted_index(dtype)
  q = index.train_cells(PLANTED, iters=1, init=torch.from_numpy(init).to(DEV))
  assert np.array_equal(_labels_of(q.assign(index)), planted)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16, FP8], ids=MAIN_IDS)
def test_the_objective_rises_and_the_labels_settle(dtype):
  index = _planted_index(dtype)
  q = index.train_cells(PLANTED, iters=8, seed=0)
  objective, moved = q.objective.cpu().numpy(), q.moved.cpu().numpy()
  print('objective', objective, 'moved', moved)
  assert objective[-1] >= objective[0]
  assert moved[-1] == 0 and q.iterations <= 8
  assert q.objective.dtype is torch.float32 and q.moved.dtype is torch.int64


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16, FP8], ids=MAIN_IDS)
def test_an_empty_cell_is_reseeded_with_the_lowest_scoring_item(dtype):
  """init[11] is an exact copy of init[0]: every tie goes to the lower cell, so cell 11 is empty after the first
  assignment and takes the item with the lowest score, as search.reseed_ref says."""
  from mmt_amd import search
  from mmt_amd.search import VideoIndex
  g, gw, planted, init = (x.copy() for x in _planted())
  g[init[11]], gw[init[11]] = g[init[0]], gw[init[0]]
  index = VideoIndex(torch.from_numpy(g).to(DEV), torch.from_numpy(gw).to(DEV), dtype=dtype)
  n, start = len(planted), torch.from_numpy(init).to(DEV)
  ids = torch.full((n,), -1, dtype=torch.int64, device=DEV)
  ids[start] = torch.arange(PLANTED, device=DEV)
  e0, w0 = index.cell_centroids(index.cells(ids, PLANTED))
  assert _same((e0[11], w0[11]), (e0[0], w0[0]))
  s, best = VideoIndex(e0, w0, dtype=dtype).neighbours(k=1, source=index)
  labels, scores = best[:, 0].cpu().numpy(), s[:, 0].cpu().numpy()
  assert (labels != 11).all() and np.bincount(labels, minlength=PLANTED)[:11].min() > 0
  want = search.reseed_ref(labels, scores, np.arange(n), PLANTED)
  worst = int(np.argsort(scores, kind='stable')[0])
  assert want[worst] == 11 and (want != labels).sum() == 1
  e1, w1 = index.cell_centroids(index.cells(torch.from_numpy(want).to(DEV), PLANTED), out=(e0.clone(), w0.clone()))
  one = index.train_cells(PLANTED, iters=1, init=start)
  assert _same((one.embds, one.weights), (e1, w1))
  assert int(one.moved[0]) == int((want != ids.cpu().numpy()).sum())
  done = index.train_cells(PLANTED, iters=8, init=start)
  assert int(done.assign(index).sizes.min()) > 0


# ------------------------------------------------------------------------------------------------------ end to end

@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16, FP8], ids=MAIN_IDS)
def test_search_cells_through_a_trained_quantiser(dtype):
  g, gw, planted, init = _planted()
  index = _planted_index(dtype)
  quantiser = index.train_cells(PLANTED, iters=2, init=torch.from_numpy(init).to(DEV))
  cells = quantiser.assign(index)
  gen = torch.Generator(device=DEV).manual_seed(9)
  q, qw = torch.randn(130, 3, 64, device=DEV, generator=gen), torch.rand(130, 3, device=DEV, generator=gen)
  q[:40] = torch.from_numpy(g[100:140]).to(DEV)
  assert _same(index.search_cells(q, qw, cells, nprobe=PLANTED, k=10), index.search(q, qw, k=10))
  assert _same(index.search_cells(q, qw, cells, nprobe=64, k=10), index.search(q, qw, k=10))
  probes = cells.probes(q, qw, 1)
  assert tuple(probes.shape) == (130, 1) and torch.equal(probes, quantiser.probes(q, qw, 1))
  assert torch.equal(probes, quantiser.centroids.search(q, qw, k=1)[1])
  got = index.search_cells(q, qw, cells, nprobe=1, k=10)
  assert _same(got, index.search_probed(q, qw, cells, probes, k=10))
  for c in range(PLANTED):
    rows = torch.nonzero(probes[:, 0] == c)[:, 0]
    if rows.numel():
      members = cells.items[int(cells.offsets[c]):int(cells.offsets[c + 1])]
      want = index.search(q[rows], qw[rows], k=10, subset=index.subset(members))
      assert _same((got[0][rows], got[1][rows]), want), c
  # plain cells keep refusing, in the words they had
  plain = index.cells(torch.from_numpy(planted).to(DEV), PLANTED)
  with pytest.raises(ValueError, match='probes: these cells were not made from centres; take the probes from a coarse index of your own'):
    index.search_cells(q, qw, plain, nprobe=2)


def test_refusals_by_name_leave_the_index_usable():
  from mmt_amd.search import ShardedVideoIndex, VideoIndex
  g, gw, planted, init = _planted()
  index = _planted_index(torch.float32)
  cells = index.cells(torch.from_numpy(planted).to(DEV), PLANTED)
  want = index.cell_sums(cells)
  quantiser = index.train_cells(PLANTED, iters=1, init=torch.from_numpy(init).to(DEV))
  for name in ('subset', 'where', 'norm', 'pooling', 'item_pooling'):
    for who, call in (('train_cells', lambda **kw: index.train_cells(PLANTED, **kw)),
                      ('cell_sums', lambda **kw: index.cell_sums(cells, **kw)),
                      ('cell_centroids', lambda **kw: index.cell_centroids(cells, **kw)),
                      ('assign', lambda **kw: quantiser.assign(index, **kw))):
      with pytest.raises(ValueError, match='%s: %s= is out of scope' % (who, name)):
        call(**{name: None})
  shards = ShardedVideoIndex(torch.from_numpy(g).to(DEV), torch.from_numpy(gw).to(DEV), [DEV] * 2)
  sharded_cells = shards.cells(torch.from_numpy(planted).to(DEV), PLANTED)
  for who, args in (('train_cells', (PLANTED,)), ('cell_sums', (sharded_cells,)), ('cell_centroids', (sharded_cells,))):
    with pytest.raises(ValueError, match='%s: not available on a ShardedVideoIndex' % who):
      getattr(shards, who)(*args)
  with pytest.raises(ValueError, match='assign: not available on a ShardedVideoIndex'):
    quantiser.assign(shards)
  with pytest.raises(ValueError, match='cells must come from'):
    index.cell_sums(sharded_cells)
  other = VideoIndex(torch.from_numpy(g[:500]).to(DEV), torch.from_numpy(gw[:500]).to(DEV), dtype=torch.bfloat16)
  with pytest.raises(ValueError, match='cells must come from'):
    other.cell_centroids(cells)
  with pytest.raises(ValueError, match='neighbours: the source holds'):
    quantiser.assign(other)                                                     # another dtype than the centroids'
  with pytest.raises(ValueError, match='train_cells: the items of init must be distinct'):
    index.train_cells(2, init=torch.tensor([5, 5], device=DEV))
  assert _same(index.cell_sums(cells), want)
