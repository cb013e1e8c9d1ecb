"""The host side of the k-means cells (VideoIndex.cell_sums, cell_centroids, train_cells; mmt_search_cell_sums,
mmt_search_cell_centroids) without a GPU: the numpy restatements of the summation order and of the re-seeding rule --
search.cell_sums_ref and search.reseed_ref, and the torch forms the calls run on the device, here on host tensors --
against brute-force loops; the header and the ctypes table; the argument gates of the entry points and the argument
errors of the calls."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests.test_index_groups_cpu import _hollow_index, _hollow_sharded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = {'mmt_cell_sums_workspace_floats': 3, 'mmt_search_cell_sums': 13, 'mmt_search_cell_centroids': 13}


def _labels(piece, seed=0):
  """Cell 0 empty, cell 1 one item, cells of piece - 1, piece, piece + 1 and 2 * piece + 1 items, and 9 items in no cell,
  interleaved at random."""
  sizes = [0, 1, piece - 1, piece, piece + 1, 2 * piece + 1]
  ids = np.concatenate([np.full(n, c) for c, n in enumerate(sizes)] + [np.full(9, -1)]).astype(np.int64)
  np.random.RandomState(seed).shuffle(ids)
  return ids, len(sizes)


def test_cell_sums_ref_is_the_sum_of_the_members_on_exact_data():
  """Multiples of 1/8 below 2^10 in magnitude: every partial sum is exact in fp32, so the stated order must give the fp64
  sums of brute-force loops over the labels."""
  from mmt_amd import search
  assert search.SUM_PIECE == 256 and search.SUM_SLAB == 1024
  piece = 5
  ids, num_cells = _labels(piece)
  rng = np.random.RandomState(1)
  rows = (rng.randint(-8, 9, size=(len(ids), 12)) / 8).astype(np.float32)
  weights = (rng.randint(0, 3, size=(len(ids), 3)) / 4).astype(np.float32)
  offsets, items = search.cell_lists(ids, num_cells)
  sums, wsums, counts = search.cell_sums_ref(rows, weights, offsets, items, piece)
  assert sums.dtype == wsums.dtype == np.float32 and counts.dtype == np.int64
  want, wwant, n = np.zeros((num_cells, 12)), np.zeros((num_cells, 3)), np.zeros(num_cells, np.int64)
  for g, c in enumerate(ids):
    if c >= 0:
      want[c] += rows[g]
      wwant[c] += weights[g]
      n[c] += 1
  assert np.array_equal(sums, want) and np.array_equal(wsums, wwant) and counts.tolist() == n.tolist()
  assert n[0] == 0 and not sums[0].any() and n[1] == 1 and np.array_equal(sums[1], rows[np.flatnonzero(ids == 1)[0]])
  # torch tensors are taken as well
  again = search.cell_sums_ref(torch.from_numpy(rows), torch.from_numpy(weights), torch.from_numpy(offsets),
                               torch.from_numpy(items), piece)
  assert all(np.array_equal(a, b) for a, b in zip((sums, wsums, counts), again))


def test_cell_sums_ref_adds_in_the_stated_order():
  """Random fp32 data, where the order shows: scalar loops -- piece by piece, position by position, each from +0."""
  from mmt_amd import search
  piece = 4
  ids, num_cells = _labels(piece, seed=3)
  rng = np.random.RandomState(2)
  rows = (rng.standard_normal((len(ids), 3)) * 10.0 ** rng.randint(-3, 4, size=(len(ids), 1))).astype(np.float32)
  weights = rng.random_sample((len(ids), 2)).astype(np.float32)
  offsets, items = search.cell_lists(ids, num_cells)
  sums, wsums, _ = search.cell_sums_ref(rows, weights, offsets, items, piece)
  for table, got in ((rows, sums), (weights, wsums)):
    for c in range(num_cells):
      members = [g for g in range(len(ids)) if ids[g] == c]
      for col in range(table.shape[1]):
        total = np.float32(0)
        for first in range(0, len(members), piece):
          part = np.float32(0)
          for g in members[first:first + piece]:
            part = np.float32(part + table[g, col])
          total = np.float32(total + part)
        assert got[c, col] == total, (c, col)
  # the cut is part of the order: (2^24 + 1) + (1 - 2^24) = 1 in pieces of two, ((2^24 + 1) + 1) - 2^24 = 0 in one piece
  column = np.array([[2.0 ** 24], [1], [1], [-2.0 ** 24]], np.float32)
  one_cell = (column, np.ones((4, 1), np.float32), np.array([0, 4]), np.arange(4))
  assert search.cell_sums_ref(*one_cell, 2)[0].tolist() == [[1.0]] and search.cell_sums_ref(*one_cell, 4)[0].tolist() == [[0.0]]


def _brute_pieces(offsets, piece):
  work, start = [], [0]
  for c in range(len(offsets) - 1):
    for first in range(offsets[c], offsets[c + 1], piece):
      work.append((c, first, min(first + piece, offsets[c + 1])))
    start.append(len(work))
  return work, start


@pytest.mark.parametrize('piece', [5, 256])
def test_sum_plan_on_host_tensors(piece):
  from mmt_amd import search
  ids, num_cells = _labels(piece)
  offsets, items = search.cell_lists(ids, num_cells)
  want, start = _brute_pieces(offsets.tolist(), piece)
  n_work = -(-len(items) // piece) + num_cells                     # the bound the host knows
  assert len(want) <= n_work
  work, piece_start = search._sum_plan(torch.from_numpy(offsets), n_work, piece)
  assert work.dtype == piece_start.dtype == torch.int32 and tuple(work.shape) == (n_work, 3)
  assert work[:len(want)].tolist() == [list(w) for w in want] and not work[len(want):].any()
  assert piece_start.tolist() == start
  assert ((work[:, 2] - work[:, 1]) <= piece).all()
  tight = search._sum_plan(torch.from_numpy(offsets), len(want), piece)[0]
  assert tight.tolist() == [list(w) for w in want]
  none = search._sum_plan(torch.zeros(4, dtype=torch.int64), 3, piece)
  assert not none[0].any() and none[1].tolist() == [0, 0, 0, 0]


def _brute_reseed(ids, scores, items, num_cells):
  ids = list(ids)
  empty = [c for c in range(num_cells) if not any(ids[g] == c for g in items)]
  taken = []
  for c in empty:
    best = None
    for i, g in enumerate(items):                                  # ascending item numbers: a tie stays with the first
      if g not in taken and (best is None or scores[i] < scores[best]):
        best = i
    taken.append(items[best])
    ids[items[best]] = c
  return ids


def test_reseed_rule_against_brute_force():
  from mmt_amd import search
  items = np.array([0, 1, 3, 4, 5, 7, 8, 9])
  ids = np.full(10, -1, np.int64)
  ids[items] = [2, 2, 0, 2, 5, 5, 0, 2]                            # cells 1, 3 and 4 empty
  cases = {
      'distinct': [0.9, 0.1, 0.5, 0.3, 0.8, 0.2, 0.7, 0.6],
      'two tied lowest': [0.9, 0.1, 0.5, 0.1, 0.8, 0.1, 0.7, 0.6],
      'all tied': [0.5] * 8,
  }
  for name, scores in cases.items():
    scores = np.array(scores, np.float32)
    got = search.reseed_ref(ids, scores, items, 6)
    assert got.tolist() == _brute_reseed(ids, scores, items.tolist(), 6), name
    assert (got[[2, 6]] == -1).all()                               # outside the sample: never relabelled
    torch_form = search._reseed(torch.from_numpy(ids), torch.from_numpy(scores), torch.from_numpy(items), 6)
    assert torch_form.tolist() == got.tolist(), name
  tied = search.reseed_ref(ids, np.array(cases['two tied lowest'], np.float32), items, 6)
  assert (tied[1], tied[4], tied[7]) == (1, 3, 4)                  # cells ascending take the tied items ascending
  # no empty cell: nothing changes; a relabelling may empty a one-item cell, which stays empty
  full = np.array([0, 1, 2, 2, 1])
  assert search.reseed_ref(full, np.zeros(5, np.float32), np.arange(5), 3).tolist() == full.tolist()
  assert search._reseed(torch.from_numpy(full), torch.zeros(5), torch.arange(5), 3).tolist() == full.tolist()
  emptied = search.reseed_ref(np.array([0, 1, 1, 1]), np.array([0.1, 0.5, 0.5, 0.5], np.float32), np.arange(4), 3)
  assert emptied.tolist() == [2, 1, 1, 1]


def test_header_and_bindings_agree():
  from mmt_amd import _lib, search
  src = open(os.path.join(ROOT, 'include', 'mmt_hip.h')).read()
  handle = ctypes.CDLL(_lib.LIB_PATH)
  for name, arity in NEW_EXPORTS.items():
    m = re.search(r'\b(int|int64_t) %s\(([^;]*?)\);' % name, src)
    assert m, name + ' is not declared in mmt_hip.h'
    params = [p.strip() for p in m.group(2).replace('\n', ' ').split(',')]
    res, args = _lib.SIGNATURES[name]
    assert res is (ctypes.c_int if m.group(1) == 'int' else ctypes.c_int64), name
    assert len(args) == len(params) == arity, name
    for p, a in zip(params, args):
      assert (a is ctypes.c_void_p) == ('*' in p) and (a is ctypes.c_int) == (p.startswith('int ')), (name, p)
    assert hasattr(handle, name)
  assert 'search_kmeans.hip' in src and os.path.exists(os.path.join(ROOT, 'mmt_amd', 'csrc', 'search_kmeans.hip'))
  assert int(re.search(r'#define MMT_SEARCH_SUM_PIECE (\d+)', src).group(1)) == search.SUM_PIECE
  assert int(re.search(r'#define MMT_SEARCH_SUM_SLAB (\d+)', src).group(1)) == search.SUM_SLAB
  assert handle.mmt_abi_version() == 6
  assert 'sizeof(MmtSearchScan) == 128' in src and ctypes.sizeof(_lib.MmtSearchScan) == 128


_buf = (ctypes.c_char * 256)()
P = ctypes.addressof(_buf) + -ctypes.addressof(_buf) % 16        # 16-byte aligned, never dereferenced: every call is refused


def test_new_exports_gate_their_arguments_on_the_host():
  """Every refusal below returns before any launch: MMT_ERR_ARG = -1, MMT_ERR_ALIGN = -2.  A good call is recognised by the
  alignment refusal that only an otherwise accepted call reaches."""
  from mmt_amd import _lib
  L = _lib.lib()
  size = L.mmt_cell_sums_workspace_floats
  assert size(1, 1, 4) == 5 and size(1030, 7, 512) == 1030 * 7 * 513
  for bad in ((0, 1, 4), (1, 0, 4), (1, 17, 4), (1, 1, 0), (1, 1, 6), (-1, 1, 4)):
    assert size(*bad) == -1, bad

  def sums(store=0, **own):
    a = dict(g=P + 8, gw=P, gscale=P if store == 2 else None, storage=store, NV=1, M=1, d=16, items=P, n_items=1, work=P,
             n_work=1, ws=P)
    a.update(own)
    return L.mmt_search_cell_sums(*a.values(), None)
  for store in (0, 1, 2):
    assert sums(store) == -2                                       # accepted up to the alignment of the stored rows
    assert sums(store, g=P, ws=P + 4) == -2
    for name in ('g', 'gw', 'items', 'work', 'ws'):
      assert sums(store, **{name: None}) == -1, name
    for name, bad in (('NV', 0), ('M', 0), ('M', 17), ('d', 0), ('d', 16 + (4, 8, 16)[store] // 2), ('n_items', 0),
                      ('n_items', -1), ('n_work', 0), ('n_work', -1), ('storage', 3), ('storage', -1), ('d', 1 << 27)):
      assert sums(store, **{name: bad}) == -1, (name, bad)
  assert sums(0, gscale=P) == -1 and sums(1, gscale=P) == -1 and sums(2, gscale=None) == -1

  def centroids(**own):
    a = dict(ws=P + 4, n_work=1, piece_start=P, offsets=P, n_items=1, C=1, M=1, d=4, sums=P, wsums=P, embds=P, weights=P)
    a.update(own)
    return L.mmt_search_cell_centroids(*a.values(), None)
  assert centroids() == -2 and centroids(embds=None, weights=None) == -2
  for name in ('ws', 'piece_start', 'offsets', 'sums', 'wsums', 'embds', 'weights'):   # a centroid needs both outputs
    assert centroids(**{name: None}) == -1, name
  for name, bad in (('n_work', 0), ('n_items', 0), ('C', 0), ('M', 0), ('M', 17), ('d', 0), ('d', 6), ('d', 1 << 27),
                    ('n_work', -1), ('C', -1)):
    assert centroids(**{name: bad}) == -1, (name, bad)


def _hollow_cells(index, num_items=5, sharded=False):
  from mmt_amd.search import IndexCells, ShardedCells
  offsets = torch.tensor([0, 2, 2, num_items])
  items = torch.arange(num_items)
  cells = ShardedCells(index, offsets, items, num_items, []) if sharded else IndexCells(index, offsets, items, num_items)
  cells.device = index.device
  return cells


def test_a_sharded_index_refuses_the_calls_by_name():
  from mmt_amd.search import CellQuantiser
  index = _hollow_sharded(5)
  cells = _hollow_cells(index, sharded=True)
  for who, args in (('train_cells', (2,)), ('cell_sums', (cells,)), ('cell_centroids', (cells,))):
    with pytest.raises(ValueError, match='%s: not available on a ShardedVideoIndex' % who):
      getattr(index, who)(*args)
  quantiser = CellQuantiser.__new__(CellQuantiser)
  with pytest.raises(ValueError, match='assign: not available on a ShardedVideoIndex'):
    quantiser.assign(index)


def test_argument_errors_are_raised_without_a_device():
  from mmt_amd import search
  from mmt_amd.search import CellQuantiser
  index = _hollow_index(5)
  cells = _hollow_cells(index)
  assert cells.quantiser is None
  assert set(search._NOT_TRAINED) == {'subset', 'where', 'norm', 'pooling', 'item_pooling'}
  quantiser = CellQuantiser.__new__(CellQuantiser)
  for name in search._NOT_TRAINED:
    for who, call in (('train_cells', lambda **kw: index.train_cells(2, **kw)),
                      ('cell_sums', lambda **kw: index.cell_sums(cells, **kw)),
                      ('cell_centroids', lambda **kw: index.cell_centroids(cells, **kw)),
                      ('assign', lambda **kw: quantiser.assign(index, **kw))):
      with pytest.raises(ValueError, match='%s: %s= is out of scope' % (who, name)):
        call(**{name: None})
  with pytest.raises(TypeError):
    index.train_cells(2, schedule='stream')
  with pytest.raises(TypeError):
    index.cell_sums(cells, k=3)
  # cells: type, origin, age
  other = _hollow_index(5)
  for who in ('cell_sums', 'cell_centroids'):
    for bad in (None, torch.zeros(3), _hollow_cells(other), _hollow_cells(index, sharded=True)):
      with pytest.raises(ValueError, match=r'%s: cells must come from the cells\(\) or cells_from_centres\(\) of this index' % who):
        getattr(index, who)(bad)
    index.num_items = 6
    with pytest.raises(ValueError, match='%s: the cells were built for 5 items, the index holds 6' % who):
      getattr(index, who)(cells)
    index.num_items = 5
  # out=
  good = (torch.zeros(3, 2, 8), torch.zeros(3, 2))
  for bad in (good[0], (good[0],), (good[0], None), [good[0], 1.0]):
    with pytest.raises(ValueError, match='cell_centroids: out must be a pair of tensors'):
      index.cell_centroids(cells, out=bad)
  with pytest.raises(ValueError, match='cell_centroids: out must hold contiguous float32 tensors'):
    index.cell_centroids(cells, out=good)                          # host tensors for a device index
  index.device = torch.device('cpu')
  for bad in ((good[0].double(), good[1]), (good[0], torch.zeros(3, 3)), (torch.zeros(4, 2, 8), good[1]),
              (torch.zeros(3, 8, 2).transpose(1, 2), good[1])):
    with pytest.raises(ValueError, match='cell_centroids: out must hold contiguous float32 tensors'):
      index.cell_centroids(cells, out=bad)
  index.device = torch.device('cuda', 0)
  # train_cells
  for bad in (0, -1, True, 2.0, None, 2 ** 31):
    with pytest.raises(ValueError, match='train_cells: num_cells must be an int'):
      index.train_cells(bad)
  for bad in (0, -1, True, 2.0, None):
    with pytest.raises(ValueError, match='train_cells: iters must be an int >= 1'):
      index.train_cells(2, iters=bad)
  for bad in (-1, True, 2.0, None, 2 ** 32):
    with pytest.raises(ValueError, match='train_cells: seed must be an int'):
      index.train_cells(2, seed=bad)
  for name in ('init', 'items'):
    for bad in ([0, 1], np.zeros(2, np.int64), torch.zeros(2, dtype=torch.int32), torch.zeros(2)):
      with pytest.raises(ValueError, match='train_cells: %s must be an int64 tensor' % name):
        index.train_cells(2, **{name: bad})
    with pytest.raises(ValueError, match='train_cells: %s must be on the index device' % name):
      index.train_cells(2, **{name: torch.zeros(2, dtype=torch.int64)})
  index.device = torch.device('cpu')                               # lets the later checks be reached with host tensors
  for bad in (torch.zeros(3, dtype=torch.int64), torch.zeros(1, 2, dtype=torch.int64), torch.zeros(0, dtype=torch.int64)):
    with pytest.raises(ValueError, match=r'train_cells: init \[num_cells\] expected'):
      index.train_cells(2, init=bad)
  for bad in (torch.zeros(0, dtype=torch.int64), torch.zeros(2, 2, dtype=torch.int64)):
    with pytest.raises(ValueError, match=r'train_cells: items \[T >= 1\] expected'):
      index.train_cells(2, items=bad)
  with pytest.raises(ValueError, match=r'train_cells: items must lie in 0 \.\. 4, got 0 \.\. 5'):
    index.train_cells(2, items=torch.tensor([0, 5]))
  with pytest.raises(ValueError, match=r'train_cells: init must lie in 0 \.\. 4, got -1 \.\. 3'):
    index.train_cells(2, init=torch.tensor([3, -1]))
  with pytest.raises(ValueError, match='train_cells: 6 cells but 5 training items'):
    index.train_cells(6)
  with pytest.raises(ValueError, match='train_cells: 3 cells but 2 training items'):
    index.train_cells(3, items=torch.tensor([4, 1, 4]))
  with pytest.raises(ValueError, match='train_cells: the items of init must be distinct'):
    index.train_cells(3, init=torch.tensor([1, 2, 1]))
  with pytest.raises(ValueError, match='train_cells: the items of init must belong to the training items'):
    index.train_cells(2, init=torch.tensor([1, 2]), items=torch.tensor([1, 3, 4]))
  with pytest.raises(ValueError, match='train_cells: the index holds no items'):
    _hollow_index(0).train_cells(1)
  # cells with a quantiser answer probes through it; plain cells keep their message
  with pytest.raises(ValueError, match='probes: these cells were not made from centres; take the probes from a coarse index of your own'):
    cells.probes(None, None, 4)
  cells.quantiser = quantiser
  for bad in (0, 65, True, 1.0, None):
    with pytest.raises(ValueError, match=r'probes: nprobe must be an int in 1\.\.64'):
      cells.probes(None, None, bad)
  index.num_items = 6
  with pytest.raises(ValueError, match='the cells were built for 5 items, the index holds 6'):
    cells.probes(None, None, 4)
