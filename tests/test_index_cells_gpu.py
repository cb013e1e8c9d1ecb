"""The cell-probed search on the GPU (VideoIndex.cells, search_probed, cells_from_centres, search_cells;
mmt_search_topk_cells).  Every claim is one of bit identity.  The oracle does not touch the new kernel:
index.search_deep(q, qw, depth=num_items) gives every row's complete ordered list with the score bits; filtered in numpy
by membership in the row's probed cells, cut at k and padded with (-inf, -1) it is the expected result.  Scores are compared
as bit patterns, indices exactly."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
FP8 = torch.float8_e4m3fn
CONFIGS = [(torch.float32, 3, 64), (torch.bfloat16, 3, 64), (FP8, 3, 64), (FP8, 2, 16), (torch.float32, 7, 32)]
IDS = ['fp32-3x64', 'bf16-3x64', 'fp8-3x64', 'fp8-2x16', 'fp32-7x32']
MAIN, MAIN_IDS = CONFIGS[:3], IDS[:3]
NQ, CELLS = 130, 40
EMPTY, ONE, C127, C128, C129, BIG, TIES_A, TIES_B = 0, 1, 2, 3, 4, 5, 6, 7
NO_PROBE, ONE_ITEM, ONLY_EMPTY, TIED = 100, 101, 102, 70    # rows: all -1; cell ONE alone; the empty cell alone; = the copied item
_cache = {}


def _labels():
  """int64 [NV]: cell 0 empty, cell 1 one item, cells 2 .. 4 of 127 / 128 / 129 items, cell 5 one item over the piece
  bound, cells 6 .. 39 of 20 .. 90 items, 50 items in no cell -- randomly interleaved.  -> (labels, the 12 copies: 6 of
  them in cell 6, 3 in cell 7, 3 in cell 5)."""
  from mmt_amd import search
  if 'labels' not in _cache:
    rng = np.random.RandomState(40)
    sizes = [0, 1, 127, 128, 129, search.CELL_PIECE + 1] + list(rng.randint(20, 91, size=CELLS - 6))
    ids = np.concatenate([np.full(n, c) for c, n in enumerate(sizes)] + [np.full(50, -1)]).astype(np.int64)
    rng.shuffle(ids)
    copies = np.concatenate([np.flatnonzero(ids == TIES_A)[:6], np.flatnonzero(ids == TIES_B)[:3], np.flatnonzero(ids == BIG)[-3:]])
    _cache['labels'] = ids, copies
  return _cache['labels']


def _data(m, d):
  """The gallery and 130 queries; the 12 `copies` are exact copies of one item, row TIED of the queries is that item (the
  copies lead its list), row 7 is all zero."""
  if ('data', m, d) not in _cache:
    ids, copies = _labels()
    nv = ids.shape[0]
    gen = torch.Generator(device=DEV).manual_seed(1000 * m + d)
    g, gw = torch.randn(nv, m, d, device=DEV, generator=gen), torch.rand(nv, m, device=DEV, generator=gen)
    q, qw = torch.randn(NQ, m, d, device=DEV, generator=gen), torch.rand(NQ, m, device=DEV, generator=gen)
    at = torch.from_numpy(copies).to(DEV)
    g[at], gw[at] = 3 * g[at[0]], gw[at[0]].clone()                  # long rows: the copies lead the list of row TIED
    q[TIED], qw[TIED] = g[at[0]], gw[at[0]]
    q[7] = 0
    _cache['data', m, d] = g, gw, q, qw
  return _cache['data', m, d]


def _index(config):
  from mmt_amd.search import VideoIndex
  if ('index', config) not in _cache:
    g, gw, _, _ = _data(*config[1:])
    _cache['index', config] = VideoIndex(g, gw, dtype=config[0])
  return _cache['index', config]


def _cells(config):
  if ('cells', config) not in _cache:
    _cache['cells', config] = _index(config).cells(torch.from_numpy(_labels()[0]).to(DEV), CELLS)
  return _cache['cells', config]


def _probes(width):
  """int64 [130, P] on the host.  P = 1: row r probes cell r % 40.  P = 5, 64: cell C127 is probed by exactly rows 0 .. 63,
  C128 by rows 0 .. 64, C129 by every row, twice; the other columns are drawn from -1, numbers out of range and the other
  cells (at P = 64 most cells repeat in a row); the columns of a row are shuffled; row TIED probes the cells of the
  copies.  At P = 1 and 5 rows NO_PROBE, ONE_ITEM and ONLY_EMPTY are what their names say (so C129 has 127 rows there and
  all 130 at P = 64)."""
  if ('probes', width) not in _cache:
    rng = np.random.RandomState(width)
    if width == 1:
      p = (np.arange(NQ) % CELLS).reshape(NQ, 1).astype(np.int64)
    else:
      others = [c for c in range(CELLS) if c not in (C127, C128, C129)] + [-1, -1, -1, CELLS, CELLS + 9, -5]
      p = rng.choice(others, size=(NQ, width)).astype(np.int64)
      p[:, 0] = p[:, 3] = C129
      p[:64, 1] = C127
      p[:65, 2] = C128
      p[TIED, :5] = [C129, TIES_A, TIES_B, BIG, TIES_A]
      for r in range(NQ):
        rng.shuffle(p[r])
    if width < 64:
      p[NO_PROBE], p[ONLY_EMPTY] = -1, EMPTY
      p[ONE_ITEM], p[ONE_ITEM, 0] = -1, ONE
    _cache['probes', width] = p
  return _cache['probes', width]


def _deep(config):
  """Every row's complete ordered list on this index, once: (score bits int32 [NQ, NV], items int64 [NQ, NV]) on the host."""
  if ('deep', config) not in _cache:
    _, _, q, qw = _data(*config[1:])
    index = _index(config)
    s, i = index.search_deep(q, qw, depth=index.num_items)
    assert i.shape == (NQ, index.num_items)
    _cache['deep', config] = s.view(torch.int32).cpu().numpy(), i.cpu().numpy()
  return _cache['deep', config]


def _allowed(probes, ids=None):
  """bool [rows, NV]: the item is in one of the row's probed cells."""
  ids = _labels()[0] if ids is None else ids
  wanted = np.zeros((probes.shape[0], CELLS + 1), bool)
  ok = (probes >= 0) & (probes < CELLS)
  np.logical_or.at(wanted, (np.nonzero(ok)[0], probes[ok]), True)
  return wanted[:, np.where(ids >= 0, ids, CELLS)]


def _expected(config, probes, k, ids=None):
  """The deep list filtered by the probed cells, the first k, padded -> (bits int32 [rows, k], items int64 [rows, k])."""
  bits, items = _deep(config)
  rows = probes.shape[0]
  keep = np.take_along_axis(_allowed(probes, ids), items[:rows], 1)
  want_b = np.full((rows, k), np.float32(-np.inf).view(np.int32), np.int32)
  want_i = np.full((rows, k), -1, np.int64)
  for r in range(rows):
    at = np.flatnonzero(keep[r])[:k]
    want_b[r, :len(at)], want_i[r, :len(at)] = bits[r, at], items[r, at]
  return want_b, want_i


def _check(got, want, what):
  s, i = got
  assert s.dtype is torch.float32 and i.dtype is torch.int64 and s.device == DEV and tuple(s.shape) == tuple(i.shape) == want[1].shape
  assert np.array_equal(i.cpu().numpy(), want[1]), what
  assert np.array_equal(s.view(torch.int32).cpu().numpy(), want[0]), what


def _same(a, b):
  return all(x.dtype == y.dtype and x.shape == y.shape and
             torch.equal(x.view(torch.int32) if x.dtype is torch.float32 else x, y.view(torch.int32) if y.dtype is torch.float32 else y)
             for x, y in zip(a, b))


def test_the_cells_are_the_csr_of_the_labels():
  from mmt_amd import search
  ids, copies = _labels()
  assert 3000 <= ids.shape[0] <= 6000
  cells = _cells(CONFIGS[0])
  offsets, items = search.cell_lists(ids, CELLS)
  assert cells.num_cells == CELLS and cells.num_items == ids.shape[0] and cells.device == DEV and cells.centres is None
  assert cells.offsets.dtype == cells.items.dtype == cells.sizes.dtype == torch.int64
  assert cells.offsets.cpu().tolist() == offsets.tolist() and cells.items.cpu().tolist() == items.tolist()
  sizes = cells.sizes.cpu().tolist()
  assert sizes == np.diff(offsets).tolist() and sizes[:6] == [0, 1, 127, 128, 129, search.CELL_PIECE + 1]
  assert cells.max_pieces == 2
  assert len(set(ids[copies])) == 3                                   # the copies lie in three cells
  # the labels are interleaved: no cell's items are consecutive, so the indirection matters
  assert all(np.diff(items[offsets[c]:offsets[c + 1]]).max() > 1 for c in range(2, CELLS))


@pytest.mark.parametrize('width', [1, 5, 64])
@pytest.mark.parametrize('config', CONFIGS, ids=IDS)
def test_probed_is_the_deep_list_filtered_by_the_probed_cells(config, width):
  from mmt_amd import search
  assert search.MAX_PROBES == 64
  _, _, q, qw = _data(*config[1:])
  index, cells, probes = _index(config), _cells(config), _probes(width)
  dev_probes = torch.from_numpy(probes).to(DEV)
  if width > 1:
    counts = [sum(c in row for row in probes.tolist()) for c in (C127, C128, C129)]
    assert counts == [64, 65, 130 if width == 64 else 127]
  for nq in (1, 63, 65, 130):
    for k in (1, 10, 128):
      got = index.search_probed(q[:nq], qw[:nq], cells, dev_probes[:nq], k=k)
      _check(got, _expected(config, probes[:nq], k), (nq, k))
  got = index.search_probed(q, qw, cells, dev_probes, k=10)
  assert _same(got, index.search_probed(q, qw, cells, dev_probes, k=10))        # and again
  s, i = (t.cpu() for t in got)
  if width < 64:
    assert (i[NO_PROBE] == -1).all() and torch.isneginf(s[NO_PROBE]).all() and (i[ONLY_EMPTY] == -1).all()
    one = int(np.flatnonzero(_labels()[0] == ONE)[0])
    assert i[ONE_ITEM].tolist() == [one] + [-1] * 9 and torch.isneginf(s[ONE_ITEM, 1:]).all()   # k beyond the candidates
  if width > 1:                                                                # equal scores across cells: by item number
    copies = np.sort(_labels()[1])
    assert i[TIED].tolist()[:10] == copies[:10].tolist() and len(set(s[TIED, :10].view(torch.int32).tolist())) == 1


@pytest.mark.parametrize('config', MAIN, ids=MAIN_IDS)
def test_rows_with_a_small_union_equal_rescore_on_that_union(config):
  _, _, q, qw = _data(*config[1:])
  index, cells, probes = _index(config), _cells(config), _probes(5)
  allowed = _allowed(probes)
  rows = [r for r in range(NQ) if 0 < allowed[r].sum() <= 1024]
  assert ONE_ITEM in rows and len(rows) >= 1
  cand = np.full((len(rows), 1024), -1, np.int64)
  for j, r in enumerate(rows):
    mine = np.flatnonzero(allowed[r])
    cand[j, :len(mine)] = mine[::-1]
  at = torch.tensor(rows, device=DEV)
  for k in (1, 10, 128):
    got = index.search_probed(q[at], qw[at], cells, torch.from_numpy(probes[rows]).to(DEV), k=k)
    assert _same(got, index.rescore(q[at], qw[at], torch.from_numpy(cand).to(DEV), k=k)), k


@pytest.mark.parametrize('config', MAIN, ids=MAIN_IDS)
def test_neither_the_order_of_the_probes_nor_the_other_rows_nor_the_row_batches_change_the_result(config, monkeypatch):
  from mmt_amd import search
  _, _, q, qw = _data(*config[1:])
  index, cells = _index(config), _cells(config)
  for width in (5, 64):
    probes = torch.from_numpy(_probes(width)).to(DEV)
    want = index.search_probed(q, qw, cells, probes, k=10)
    gen = torch.Generator(device=DEV).manual_seed(width)
    perm = torch.argsort(torch.rand(NQ, width, device=DEV, generator=gen), 1)
    assert _same(index.search_probed(q, qw, cells, torch.gather(probes, 1, perm), k=10), want), width
    assert _same(index.search_probed(q, qw, cells, probes.flip(1), k=10), want), width
    rows = torch.tensor([TIED, 77, 0, 129, ONE_ITEM], device=DEV)              # other neighbours, another place in the call
    got = index.search_probed(q[rows], qw[rows], cells, probes[rows], k=10)
    assert _same(got, tuple(t[rows] for t in want)), width
    with monkeypatch.context() as patch:
      extra = 8 * 10 * width * cells.max_pieces
      assert len(index._row_batches(NQ, extra)) == 1
      patch.setattr(search, '_BATCH_BYTES', 1)
      assert index._row_batches(NQ, extra) == [(0, 64), (64, 128), (128, 130)]
      assert _same(index.search_probed(q, qw, cells, probes, k=10), want), width
  # the CENet text layout (B, M, C, d) / (B, C, M) gives the rows b * C + c
  m, d = config[1:]
  q4, qw4 = q.reshape(65, 2, m, d).permute(0, 2, 1, 3).contiguous(), qw.reshape(65, 2, m)
  assert _same(index.search_probed(q4, qw4, cells, probes, k=10), want)


@pytest.mark.parametrize('config', MAIN, ids=MAIN_IDS)
def test_three_shards_on_one_device_equal_the_single_index(config):
  from mmt_amd.search import ShardedCells, ShardedVideoIndex
  g, gw, q, qw = _data(*config[1:])
  ids = torch.from_numpy(_labels()[0]).to(DEV)
  mono, mono_cells = _index(config), _cells(config)
  shards = ShardedVideoIndex(g, gw, [DEV] * 3, dtype=config[0])
  cells = shards.cells(ids, CELLS)
  assert type(cells) is ShardedCells and len(cells.parts) == 3 and cells.num_items == mono.num_items
  assert torch.equal(cells.offsets, mono_cells.offsets) and torch.equal(cells.items, mono_cells.items)
  assert sum(int(p.sizes[BIG]) for p in cells.parts) == int(mono_cells.sizes[BIG])
  for width in (1, 5, 64):
    probes = torch.from_numpy(_probes(width)).to(DEV)
    for nq, k in ((130, 10), (65, 128), (1, 1)):
      got = shards.search_probed(q[:nq], qw[:nq], cells, probes[:nq], k=k)
      assert got[0].device == DEV and _same(got, mono.search_probed(q[:nq], qw[:nq], mono_cells, probes[:nq], k=k)), (width, nq, k)
  centres = torch.arange(7, mono.num_items, 150, device=DEV)
  a, b = shards.cells_from_centres(centres), mono.cells_from_centres(centres)
  assert torch.equal(a.offsets, b.offsets) and torch.equal(a.items, b.items) and torch.equal(a.centres, b.centres)
  assert torch.equal(a.probes(q, qw, 4), b.probes(q, qw, 4))
  assert _same(shards.search_cells(q, qw, a, nprobe=4, k=10), mono.search_cells(q, qw, b, nprobe=4, k=10))
  with pytest.raises(ValueError, match='cells must come from'):
    shards.search_probed(q, qw, mono_cells, probes)
  with pytest.raises(ValueError, match='cells must come from'):
    mono.search_probed(q, qw, cells, probes)


@pytest.mark.parametrize('config', MAIN, ids=MAIN_IDS)
def test_cells_from_centres_probes_and_search_cells(config):
  from mmt_amd import search
  _, _, q, qw = _data(*config[1:])
  index = _index(config)
  nv = index.num_items
  centres = torch.from_numpy(np.random.RandomState(5).permutation(nv)[:33].astype(np.int64)).to(DEV)
  cells = index.cells_from_centres(centres)
  assert cells.num_cells == 33 and torch.equal(cells.centres, centres) and int(cells.offsets[-1]) == nv
  # the numpy restatement, from `neighbours`: an item's best centre other than itself; a centre keeps its own cell
  _, best = index.neighbours(k=1, subset=index.subset(centres))
  best, host = best[:, 0].cpu().numpy(), centres.cpu().numpy()
  cell_of = {int(c): j for j, c in enumerate(host)}
  ids = np.array([cell_of[g] if g in cell_of else cell_of[int(best[g])] for g in range(nv)], np.int64)
  offsets, items = search.cell_lists(ids, 33)
  assert cells.offsets.cpu().tolist() == offsets.tolist() and cells.items.cpu().tolist() == items.tolist()
  # probes: `search` over the centres, item numbers -> cell numbers, a vacant slot -1
  for nprobe in (1, 8, 64):
    probes = cells.probes(q, qw, nprobe)
    _, found = index.search(q, qw, k=nprobe, subset=index.subset(centres))
    want = np.array([[cell_of[int(g)] if g >= 0 else -1 for g in row] for row in found.cpu().numpy()], np.int64)
    assert probes.dtype is torch.int64 and probes.device == DEV and probes.cpu().numpy().tolist() == want.tolist()
    assert probes.shape == (NQ, min(nprobe, 33))
    got = index.search_cells(q, qw, cells, nprobe=nprobe, k=10)
    assert _same(got, index.search_probed(q, qw, cells, probes, k=10))
  # every cell probed: the exact search
  assert _same(index.search_cells(q, qw, cells, nprobe=64, k=10), index.search(q, qw, k=10))
  with pytest.raises(ValueError, match='not made from centres'):
    _cells(config).probes(q, qw, 4)


@pytest.mark.parametrize('config', CONFIGS, ids=IDS)
def test_with_every_cell_probed_it_is_plain_search(config):
  _, _, q, qw = _data(*config[1:])
  index = _index(config)
  ids = torch.from_numpy(_labels()[0]).to(DEV)
  cells = index.cells(torch.where(ids < 0, torch.full_like(ids, EMPTY), ids))       # every item in a cell
  probes = torch.arange(CELLS, device=DEV).flip(0).repeat(NQ, 1)
  for k in (1, 10, 128):
    assert _same(index.search_probed(q, qw, cells, probes, k=k), index.search(q, qw, k=k)), k


@pytest.mark.parametrize('config', MAIN, ids=MAIN_IDS)
def test_search_is_what_it_was(config):
  """`search` before and after the feature has run on the same index, and against the deep list's head."""
  from mmt_amd.search import VideoIndex
  g, gw, q, qw = _data(*config[1:])
  fresh = VideoIndex(g, gw, dtype=config[0])
  before = fresh.search(q, qw, k=10)
  cells = fresh.cells(torch.from_numpy(_labels()[0]).to(DEV), CELLS)
  fresh.search_probed(q, qw, cells, torch.from_numpy(_probes(64)).to(DEV), k=128)
  after = fresh.search(q, qw, k=10)
  bits, items = _deep(config)
  assert _same(before, after)
  assert np.array_equal(after[1].cpu().numpy(), items[:, :10])
  assert np.array_equal(after[0].view(torch.int32).cpu().numpy(), bits[:, :10])


def test_refusals_leave_the_index_usable():
  from mmt_amd import search
  from mmt_amd.search import VideoIndex
  config = CONFIGS[0]
  g, gw, q, qw = _data(*config[1:])
  index, cells = _index(config), _cells(config)
  probes = torch.from_numpy(_probes(5)).to(DEV)
  want = index.search_probed(q, qw, cells, probes, k=10)
  for name in ('subset', 'exclude', 'after', 'where', 'norm', 'dynamic', 'pooling', 'item_pooling', 'grouping'):
    with pytest.raises(ValueError, match='search_probed: %s= ' % name):
      index.search_probed(q, qw, cells, probes, **{name: None})
  other = VideoIndex(g[:500], gw[:500])
  with pytest.raises(ValueError, match='cells must come from'):
    other.search_probed(q, qw, cells, probes)
  grown = VideoIndex.empty(600, config[1], config[2], DEV)
  grown.add(g[:500], gw[:500])
  old = grown.cells(torch.zeros(500, dtype=torch.int64, device=DEV))
  grown.search_probed(q, qw, old, probes)
  grown.add(g[500:510], gw[500:510])
  with pytest.raises(ValueError, match='the cells were built for 500 items, the index holds 510'):
    grown.search_probed(q, qw, old, probes)
  for bad, why in ((probes.to(torch.int32), 'must be an int64 tensor'), (probes.cpu(), 'must be on the index device'),
                   (probes[:, :0], r'probes \[NQ, 1 <= P <= 64\] expected'),
                   (probes.repeat(1, 13), r'probes \[NQ, 1 <= P <= 64\] expected'), (probes[:7], '130 queries but probes')):
    with pytest.raises(ValueError, match=why):
      index.search_probed(q, qw, cells, bad)
  with pytest.raises(ValueError, match=r'k must be an int in 1\.\.128'):
    index.search_probed(q, qw, cells, probes, k=search.MAX_K + 1)
  index.schedule = 'stream'                                                   # no effect on this call
  try:
    assert _same(index.search_probed(q, qw, cells, probes, k=10), want)
  finally:
    index.schedule = None
  assert _same(index.search_probed(q, qw, cells, probes, k=10), want)
