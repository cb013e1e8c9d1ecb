"""The host side of the cell-probed search (VideoIndex.cells, search_probed; mmt_search_topk_cells) without a GPU: the CSR
of the cells and the regrouping of the (row, probe) pairs -- search.cell_lists and search.probe_plan, and the torch plan the
calls run on the device, here on host tensors -- against brute force; the header and the ctypes table; the argument gates
of the entry points and the argument errors of the calls."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests.test_index_groups_cpu import _hollow_index, _hollow_sharded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = {'mmt_topk_cells_workspace_keys': 4, 'mmt_search_topk_cells': 15}
PIECE = 2048


def _labels(seed=0):
  """130 rows' worth of cells: cell 0 empty, cell 1 one item, cells 2 .. 4 of 127 / 128 / 129 items, cell 5 one item over
  the piece bound, cells 6 .. 11 random, and 40 items in no cell -- interleaved at random."""
  rng = np.random.RandomState(seed)
  sizes = [0, 1, 127, 128, 129, PIECE + 1] + list(rng.randint(1, 60, size=6))
  ids = np.concatenate([np.full(n, c) for c, n in enumerate(sizes)] + [np.full(40, -1)]).astype(np.int64)
  rng.shuffle(ids)
  return ids, len(sizes)


def _probes(nq, num_cells, seed=1):
  """[nq, 6] probes with -1s, out-of-range numbers, a repeat per row, the empty cell, and cells probed by exactly 0, 64, 65
  and all rows: cell 7 by nobody, cell 2 by rows 0 .. 63, cell 3 by rows 0 .. 64, cell 4 by all."""
  rng = np.random.RandomState(seed)
  p = rng.choice([-1, 0, 1, 5, 6, 8, 9, 10, 11, num_cells, num_cells + 7, -3], size=(nq, 6)).astype(np.int64)
  p[:, 0] = 4
  p[:64, 1] = 2
  p[:65, 2] = 3
  p[:, 3] = p[:, 0]                      # a cell listed twice in every row
  p[min(nq - 1, 100)] = -1               # a row without a probe
  for r in range(nq):
    rng.shuffle(p[r])
  return p


def brute_lists(ids, num_cells):
  return [[g for g in range(len(ids)) if ids[g] == c] for c in range(num_cells)]


def brute_plan(probes, lists, piece):
  """The definition, in loops: per cell the distinct rows that probe it, ascending, in groups of 64; per group the pieces."""
  num_cells = len(lists)
  offsets = np.concatenate([[0], np.cumsum([len(x) for x in lists])])
  slots = {}
  for r, row in enumerate(probes):
    # the slot: the first place of the cell in the row sorted by cell, the probes that name no cell last
    ordered = sorted(int(c) if 0 <= c < num_cells and lists[c] else num_cells for c in row)
    for c in set(ordered) - {num_cells}:
      slots[(c, r)] = ordered.index(c)
  pairs = sorted(slots)
  work = []
  for c in range(num_cells):
    mine = [i for i, (cc, _) in enumerate(pairs) if cc == c]
    for g in range(0, len(mine), 64):
      for pc, first in enumerate(range(0, len(lists[c]), piece)):
        work.append((mine[g], min(64, len(mine) - g), offsets[c] + first, offsets[c] + min(first + piece, len(lists[c])), pc))
  return ([r for _, r in pairs], [slots[p] for p in pairs], np.array(work, dtype=np.int64).reshape(-1, 5))


def test_cell_lists_is_the_csr_of_the_labels():
  from mmt_amd import search
  ids, num_cells = _labels()
  offsets, items = search.cell_lists(ids, num_cells)
  lists = brute_lists(ids, num_cells)
  assert offsets.dtype == items.dtype == np.int64 and offsets.shape == (num_cells + 1,)
  assert offsets[0] == 0 and offsets[-1] == len(items) == (ids >= 0).sum()
  for c in range(num_cells):
    assert items[offsets[c]:offsets[c + 1]].tolist() == lists[c]
  assert not lists[0] and len(lists[1]) == 1 and len(lists[5]) == PIECE + 1
  # the device form of the same, on host tensors
  from mmt_amd.search import _Index
  t_off, t_items = _Index._cell_csr(torch.from_numpy(ids), num_cells)
  assert t_off.tolist() == offsets.tolist() and t_items.tolist() == items.tolist()
  assert search.cell_lists(torch.from_numpy(ids), num_cells)[1].tolist() == items.tolist()
  only_none = search.cell_lists(np.full(5, -1), 3)
  assert only_none[0].tolist() == [0, 0, 0, 0] and only_none[1].shape == (0,)


@pytest.mark.parametrize('nq', [1, 63, 65, 130])
@pytest.mark.parametrize('piece', [PIECE, 100])
def test_probe_plan_against_brute_force(nq, piece):
  from mmt_amd import search
  assert search.CELL_PIECE == PIECE and search.MAX_PROBES == 64
  ids, num_cells = _labels()
  lists = brute_lists(ids, num_cells)
  offsets, _ = search.cell_lists(ids, num_cells)
  probes = _probes(nq, num_cells)
  rows, slots, work = search.probe_plan(probes, offsets, piece)
  want_rows, want_slots, want_work = brute_plan(probes, lists, piece)
  assert rows.dtype == slots.dtype == work.dtype == np.int32
  assert rows.tolist() == want_rows and slots.tolist() == want_slots
  assert work.tolist() == want_work.tolist()
  # what the kernel relies on: a (row, slot) pair has one writer, every kept (row, cell) is covered once per piece
  assert len(set(zip(rows.tolist(), slots.tolist()))) == len(rows) and (slots < probes.shape[1]).all()
  assert ((work[:, 1] >= 1) & (work[:, 1] <= 64) & (work[:, 3] - work[:, 2] >= 1) & (work[:, 3] - work[:, 2] <= piece)).all()
  if nq == 130 and piece == PIECE:
    by_cell = {}
    for first, n, i0, i1, pc in work.tolist():
      by_cell.setdefault(int(np.searchsorted(offsets, i0, side='right')) - 1, []).append((n, pc))
    assert 7 not in by_cell and 0 not in by_cell                   # probed by nobody; empty
    assert by_cell[2] == [(64, 0)] and by_cell[3] == [(64, 0), (1, 0)] and by_cell[4] == [(64, 0), (64, 0), (1, 0)]
    assert [pc for _, pc in by_cell[5]][:2] == [0, 1]               # one item over the bound: two pieces
  # the plan the calls run, on host tensors: the same tables, padded to bounds known without the device
  max_pieces = -(-max(len(x) for x in lists) // piece)
  t_rows, t_slots, t_work = search._probe_plan(torch.from_numpy(probes), torch.from_numpy(offsets), max_pieces, piece)
  n, w = len(rows), len(work)
  assert t_rows.dtype == t_slots.dtype == t_work.dtype == torch.int32
  assert t_rows.shape == t_slots.shape == (probes.size,) and t_work.shape[0] >= w and t_work.shape[1] == 5
  assert t_rows[:n].tolist() == rows.tolist() and t_slots[:n].tolist() == slots.tolist()
  assert t_work[:w].tolist() == work.tolist() and not t_work[w:].any()
  again = search._probe_plan(torch.from_numpy(probes), torch.from_numpy(offsets), max_pieces, piece)
  assert all(torch.equal(a, b) for a, b in zip((t_rows, t_slots, t_work), again))


def test_probe_plan_depends_on_a_rows_probes_as_a_set():
  from mmt_amd import search
  ids, num_cells = _labels()
  offsets, _ = search.cell_lists(ids, num_cells)
  probes = _probes(65, num_cells)
  perm = np.stack([np.random.RandomState(r).permutation(probes.shape[1]) for r in range(65)])
  a, b = search.probe_plan(probes, offsets), search.probe_plan(np.take_along_axis(probes, perm, 1), offsets)
  assert all(np.array_equal(x, y) for x, y in zip(a, b))
  none = search.probe_plan(np.full((3, 2), -1), offsets)
  assert none[0].shape == none[1].shape == (0,) and none[2].shape == (0, 5)
  # the widest row: MAX_PROBES distinct cells in one row keep MAX_PROBES slots
  wide = search.probe_plan(np.arange(64).reshape(1, 64), np.arange(65))
  assert wide[1].tolist() == list(range(64)) and wide[2][:, 1].tolist() == [1] * 64


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
    for p, a in zip(params[1:] if 'MmtSearchScan' in params[0] else params, args[1:] if 'MmtSearchScan' in params[0] else args):
      assert (a is ctypes.c_void_p) == ('*' in p) and (a is ctypes.c_int) == (p.startswith('int ')), (name, p)
    assert hasattr(handle, name)
  params = re.search(r'int mmt_search_topk_cells\(([^;]*?)\);', src).group(1)
  assert params.startswith('const MmtSearchScan* scan') and params.rstrip().endswith('void* stream')
  assert _lib.SIGNATURES['mmt_search_topk_cells'][1][0] is ctypes.POINTER(_lib.MmtSearchScan)
  assert 'search_cells.hip' in src and os.path.exists(os.path.join(ROOT, 'mmt_amd', 'csrc', 'search_cells.hip'))
  assert int(re.search(r'#define MMT_SEARCH_MAX_PROBES (\d+)', src).group(1)) == search.MAX_PROBES == 64
  assert int(re.search(r'#define MMT_SEARCH_CELL_PIECE (\d+)', src).group(1)) == search.CELL_PIECE
  assert handle.mmt_abi_version() == 6
  assert 'sizeof(MmtSearchScan) == 128' in src and ctypes.sizeof(_lib.MmtSearchScan) == 128


_buf = (ctypes.c_char * 256)()
P = ctypes.addressof(_buf) + -ctypes.addressof(_buf) % 16        # 16-byte aligned, never dereferenced: every call is refused


def test_new_exports_gate_their_arguments_on_the_host():
  """Every refusal below returns before any launch: MMT_ERR_ARG = -1, MMT_ERR_ALIGN = -2.  A good call is recognised by the
  alignment refusal that only an otherwise accepted call reaches."""
  from mmt_amd import _lib
  L = _lib.lib()
  size = L.mmt_topk_cells_workspace_keys
  assert size(1, 1, 1, 1) == 1 and size(130, 64, 3, 128) == 130 * 64 * 3 * 128
  for bad in ((0, 1, 1, 1), (1, 0, 1, 1), (1, 65, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0), (1, 1, 1, 129), (1, 64, 1 << 20, 128)):
    assert size(*bad) == -1, bad

  def call(store=0, off=8, desc=None, **own):
    f = dict(q=P + off, q_lo=P if store else None, qw=P, g=P, gw=P, gscale=P if store == 2 else None, storage=store, NQ=1,
             NV=1, M=1, d=16)
    f.update(desc or {})
    a = dict(items=P, n_items=1, work=P, n_work=1, pair_row=P, pair_slot=P, n_pairs=1, P=1, pieces=1, k=1, ws=P, scores=P,
             index=P)
    a.update(own)
    return L.mmt_search_topk_cells(ctypes.byref(_lib.MmtSearchScan(**f)), *a.values(), None)
  for store in (0, 1, 2):
    assert call(store) == -2                                       # accepted up to the alignment of the query rows
    assert call(store, off=0, desc=dict(g=P + 4)) == -2
    for name in ('items', 'work', 'pair_row', 'pair_slot', 'ws', 'scores', 'index'):
      assert call(store, **{name: None}) == -1, name
    for name, bad in (('n_items', 0), ('n_work', 0), ('n_pairs', 0), ('P', 0), ('P', 65), ('pieces', 0), ('k', 0), ('k', 129),
                      ('n_items', -1), ('n_work', -1)):
      assert call(store, **{name: bad}) == -1, (name, bad)
    for field in ('q', 'qw', 'g', 'gw'):
      assert call(store, desc={field: None}) == -1, field
    # none of the descriptor's optional parts
    for part in (dict(subset=P), dict(exclude=P, E=1), dict(after=P), dict(lse=P, beta=1.0), dict(sets=1, set_size=1, set_weights=P),
                 dict(sets=2, set_size=1, set_weights=P)):
      assert call(store, desc=part) == -1, part
    for field, bad in (('NQ', 0), ('NV', 0), ('M', 0), ('M', 17), ('d', 0), ('d', 16 + (4, 8, 16)[store] // 2)):
      assert call(store, desc={field: bad}) == -1, (field, bad)
  assert call(0, desc=dict(q_lo=P)) == -1 and call(1, desc=dict(gscale=P)) == -1 and call(2, desc=dict(gscale=None)) == -1
  assert L.mmt_search_topk_cells(None, *([P, 1] * 2), P, P, 1, 1, 1, 1, P, P, P, None) == -1


def _hollow_cells(index, num_items=5, sharded=False):
  from mmt_amd.search import IndexCells, ShardedCells
  offsets = torch.tensor([0, 2, 2, num_items])
  items = torch.arange(num_items)
  cells = ShardedCells(index, offsets, items, num_items, []) if sharded else IndexCells(index, offsets, items, num_items)
  cells.device = index.device
  return cells


@pytest.mark.parametrize('hollow', [_hollow_index, _hollow_sharded], ids=['VideoIndex', 'ShardedVideoIndex'])
def test_argument_errors_are_raised_without_a_device(hollow):
  from mmt_amd import search
  from mmt_amd.search import ShardedVideoIndex, VideoIndex
  sharded = hollow is _hollow_sharded
  q, qw = torch.zeros(3, 2, 8), torch.zeros(3, 2)
  probes = torch.zeros(3, 4, dtype=torch.int64)
  index = hollow(5)
  cells = _hollow_cells(index, sharded=sharded)
  assert (cells.num_cells, cells.num_items, cells.max_pieces) == (3, 5, 1) and cells.sizes.tolist() == [2, 0, 3]
  assert cells.centres is None
  for name in search._NOT_PROBED:
    with pytest.raises(ValueError, match='search_probed: %s= is out of scope' % name):
      index.search_probed(q, qw, cells, probes, **{name: None})
  assert set(search._NOT_PROBED) == {'subset', 'exclude', 'after', 'where', 'norm', 'dynamic', 'pooling', 'item_pooling',
                                     'grouping'}
  with pytest.raises(TypeError):
    index.search_probed(q, qw, cells, probes, schedule='stream')
  for bad in (0, 129, -1, 2.0, True, None):
    with pytest.raises(ValueError, match=r'search_probed: k must be an int in 1\.\.128'):
      index.search_probed(q, qw, cells, probes, k=bad)
  # cells: type, origin, age
  other = hollow(5)
  for bad in (None, torch.zeros(3), _hollow_cells(other, sharded=sharded), _hollow_cells(index, sharded=not sharded)):
    with pytest.raises(ValueError, match=r'cells must come from the cells\(\) or cells_from_centres\(\) of this index'):
      index.search_probed(q, qw, bad, probes)
  index.num_items = 6                                                  # an `add` since the cells were built
  with pytest.raises(ValueError, match='the cells were built for 5 items, the index holds 6'):
    index.search_probed(q, qw, cells, probes)
  with pytest.raises(ValueError, match='the cells were built for 5 items, the index holds 6'):
    index.search_cells(q, qw, cells)
  index.num_items = 5
  # probes: dtype, device, width
  for bad in ([[0, 1]], np.zeros((3, 4), np.int64), None, probes.to(torch.int32), probes.double(), probes > 0):
    with pytest.raises(ValueError, match='probes must be an int64 tensor'):
      index.search_probed(q, qw, cells, bad)
  with pytest.raises(ValueError, match='probes must be on the index device'):
    index.search_probed(q, qw, cells, probes)                          # host probes for a device index
  index.device = torch.device('cpu')                                   # lets the later checks be reached with host tensors
  for bad in (probes[:, 0], probes.reshape(3, 2, 2), torch.zeros(3, 0, dtype=torch.int64),
              torch.zeros(3, 65, dtype=torch.int64)):
    with pytest.raises(ValueError, match=r'probes \[NQ, 1 <= P <= 64\] expected'):
      index.search_probed(q, qw, cells, bad)
  with pytest.raises(ValueError, match='CUDA tensor'):
    index.search_probed(q, qw, cells, probes)                          # the queries themselves are host tensors
  # cells(): labels
  for bad in ([0, 1], np.zeros(5, np.int64), torch.zeros(5, dtype=torch.int32)):
    with pytest.raises(ValueError, match='cells: cell_ids must be an int64 tensor'):
      index.cells(bad)
  with pytest.raises(ValueError, match=r'cells: cell_ids of shape \(5,\) expected'):
    index.cells(torch.zeros(6, dtype=torch.int64))
  with pytest.raises(ValueError, match='cells: cell_ids must be on the index device'):
    index.cells(torch.zeros(5, dtype=torch.int64, device='meta'))
  for bad in (0, -1, True, 2.0, 2 ** 31):
    with pytest.raises(ValueError, match='cells: num_cells must be None or an int'):
      index.cells(torch.zeros(5, dtype=torch.int64), bad)
  with pytest.raises(ValueError, match=r'cells: cell_ids must lie in -1 \.\. 2, got -2 \.\. 1'):
    index.cells(torch.tensor([0, 1, -2, 0, 1]), 3)
  with pytest.raises(ValueError, match=r'cells: cell_ids must lie in -1 \.\. 2, got 0 \.\. 3'):
    index.cells(torch.tensor([0, 1, 3, 0, 1]), 3)
  with pytest.raises(ValueError, match='holds no items'):
    empty = hollow(0)
    empty.device = torch.device('cpu')
    empty.cells(torch.zeros(0, dtype=torch.int64))
  if not sharded:                                                      # a single index builds its cells from host labels here
    made = index.cells(torch.tensor([2, -1, 0, 2, 0]))
    assert made.num_cells == 3 and made.offsets.tolist() == [0, 2, 2, 4] and made.items.tolist() == [2, 4, 0, 3]
    assert made.sizes.tolist() == [2, 0, 2] and made.num_items == 5 and made.device == index.device
    assert index.cells(torch.tensor([2, -1, 0, 2, 0]), 6).num_cells == 6
  # probes() and centres
  with pytest.raises(ValueError, match='probes: these cells were not made from centres'):
    cells.probes(q, qw, 4)
  cells.centres = torch.tensor([0, 1, 2])
  for bad in (0, 65, True, 1.0, None):
    with pytest.raises(ValueError, match=r'probes: nprobe must be an int in 1\.\.64'):
      cells.probes(q, qw, bad)
  for bad in ([0], torch.zeros(2, dtype=torch.int32)):
    with pytest.raises(ValueError, match='cells_from_centres: centres must be an int64 tensor'):
      index.cells_from_centres(bad)
  for bad in (torch.zeros(0, dtype=torch.int64), torch.zeros(2, 2, dtype=torch.int64)):
    with pytest.raises(ValueError, match=r'cells_from_centres: centres \[C >= 1\] expected'):
      index.cells_from_centres(bad)
  with pytest.raises(ValueError, match=r'cells_from_centres: centres must lie in 0 \.\. 4, got 0 \.\. 5'):
    index.cells_from_centres(torch.tensor([0, 5]))
  with pytest.raises(ValueError, match='the centres must be distinct'):
    index.cells_from_centres(torch.tensor([0, 3, 0]))
  for method in ('search_probed', 'search_cells', 'cells_from_centres'):
    assert getattr(ShardedVideoIndex, method) is getattr(VideoIndex, method)
  assert ShardedVideoIndex.cells is not VideoIndex.cells
