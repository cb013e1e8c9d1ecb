"""The host side of the exact k-means update (sum_scale, cell_sums_exact, cell_centroids(exact=True), train_cells(exact=
True), assign_cells on VideoIndex and ShardedVideoIndex; mmt_search_absmax, mmt_search_cell_sums_exact,
mmt_search_cell_centroids_exact) without a GPU: the numpy restatements of the definition -- search.sum_scale_ref,
search.cell_sums_exact_ref, search.exact_sums_float -- against permutations, splits, fp64 and the fp32 order on exact
data; the header and the ctypes table; the argument gates of the entry points and the argument errors of the calls."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from tests.test_index_groups_cpu import _hollow_index, _hollow_sharded
from tests.test_index_kmeans_cpu import P, _hollow_cells, _labels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = {'mmt_search_absmax': 10, 'mmt_cell_sums_exact_workspace_bytes': 3, 'mmt_search_cell_sums_exact': 20,
               'mmt_search_cell_centroids_exact': 15}


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
  assert int(re.search(r'#define MMT_SEARCH_SUM_MAX_EXPONENT (\d+)', src).group(1)) == search.MAX_SUM_EXPONENT == 160
  assert handle.mmt_abi_version() == 6
  assert 'sizeof(MmtSearchScan) == 128' in src and ctypes.sizeof(_lib.MmtSearchScan) == 128


def test_new_exports_gate_their_arguments_on_the_host():
  """Every refusal below returns before any launch: MMT_ERR_ARG = -1, MMT_ERR_ALIGN = -2.  A good call is recognised by the
  alignment refusal that only an otherwise accepted call reaches; the finish entry, which has no alignment rule, is never
  given a good call."""
  from mmt_amd import _lib
  L = _lib.lib()
  size = L.mmt_cell_sums_exact_workspace_bytes
  assert size(1, 1, 4) == 40 and size(1030, 7, 512) == 1030 * 7 * 513 * 8
  for bad in ((0, 1, 4), (1, 0, 4), (1, 17, 4), (1, 1, 0), (1, 1, 6), (-1, 1, 4)):
    assert size(*bad) == -1, bad

  def absmax(store=0, **own):
    a = dict(g=P + 8, gw=P, gscale=P if store == 2 else None, storage=store, NV=1, M=1, d=16, out=P, n_blocks=1)
    a.update(own)
    return L.mmt_search_absmax(*a.values(), None)

  def sums(store=0, **own):
    a = dict(g=P + 8, gw=P, gscale=P if store == 2 else None, storage=store, NV=1, M=1, d=16, items=P, n_items=1, work=P,
             n_work=1, piece_start=P, C=1, bits=61, exponent=0, wexponent=0, ws=P, sums=P, wsums=P)
    a.update(own)
    return L.mmt_search_cell_sums_exact(*a.values(), None)

  shapes = lambda store: (('NV', 0), ('M', 0), ('M', 17), ('d', 0), ('d', 16 + (4, 8, 16)[store] // 2), ('storage', 3),
                          ('storage', -1), ('d', 1 << 27))
  for store in (0, 1, 2):
    assert absmax(store) == -2                                     # accepted up to the alignment of the stored rows
    for name in ('g', 'gw', 'out'):
      assert absmax(store, **{name: None}) == -1, name
    for name, bad in shapes(store) + (('n_blocks', 0), ('n_blocks', -1), ('n_blocks', 65536)):
      assert absmax(store, **{name: bad}) == -1, (name, bad)
    assert sums(store) == -2
    assert sums(store, g=P, ws=P + 8) == -2
    assert sums(store, bits=1, exponent=160, wexponent=-160) == -2
    for name in ('g', 'gw', 'items', 'work', 'piece_start', 'ws', 'sums', 'wsums'):
      assert sums(store, **{name: None}) == -1, name
    for name, bad in shapes(store) + (('n_items', 0), ('n_items', -1), ('n_work', 0), ('n_work', -1), ('C', 0), ('C', -1),
                                      ('bits', 0), ('bits', 62), ('bits', -1), ('exponent', 161), ('exponent', -161),
                                      ('wexponent', 161), ('wexponent', -161)):
      assert sums(store, **{name: bad}) == -1, (name, bad)
  assert absmax(0, gscale=P) == -1 and absmax(1, gscale=P) == -1 and absmax(2, gscale=None) == -1
  assert sums(0, gscale=P) == -1 and sums(1, gscale=P) == -1 and sums(2, gscale=None) == -1

  def centroids(**own):
    a = dict(sums=P, wsums=P, offsets=P, n_items=1, C=1, M=1, d=4, bits=61, exponent=0, wexponent=0, fsums=P, fwsums=P,
             embds=P, weights=P)
    a.update(own)
    return L.mmt_search_cell_centroids_exact(*a.values(), None)
  for name in ('sums', 'wsums', 'offsets', 'fsums', 'fwsums', 'embds', 'weights'):   # a centroid needs both outputs
    assert centroids(**{name: None}) == -1, name
  for name, bad in (('n_items', 0), ('C', 0), ('C', -1), ('M', 0), ('M', 17), ('d', 0), ('d', 6), ('d', 1 << 27), ('bits', 0),
                    ('bits', 62), ('exponent', 161), ('exponent', -161), ('wexponent', 161), ('wexponent', -161)):
    assert centroids(**{name: bad}) == -1, (name, bad)


def _random_case(seed=0, n=3000, k=48, m=3, cells=7):
  """Rows with row scales 1, 2^-6 and 2^-20, weights in [0, 1), random labels with some items in no cell."""
  rng = np.random.RandomState(seed)
  rows = (rng.standard_normal((n, k)) * 2.0 ** rng.choice([0, -6, -20], size=(n, 1))).astype(np.float32)
  weights = rng.random_sample((n, m)).astype(np.float32)
  ids = rng.randint(-1, cells, size=n).astype(np.int64)
  return rows, weights, ids, cells


def test_exact_sums_do_not_depend_on_order_or_on_the_split():
  from mmt_amd import search
  rows, weights, ids, c = _random_case()
  scale = search.sum_scale_ref(rows, weights)
  assert scale.bits == search.lse_bits(len(ids)) and scale.num_items == len(ids)
  offsets, items = search.cell_lists(ids, c)
  sums, wsums, counts = search.cell_sums_exact_ref(rows, weights, offsets, items, scale)
  assert sums.dtype == wsums.dtype == counts.dtype == np.int64 and sums.shape == (c, 48) and wsums.shape == (c, 3)
  assert counts.tolist() == np.bincount(ids[ids >= 0], minlength=c).tolist() and sums.any(1).all()
  rng = np.random.RandomState(5)
  for _ in range(3):                                               # every cell's list in a random order
    shuffled = items.copy()
    for ci in range(c):
      rng.shuffle(shuffled[offsets[ci]:offsets[ci + 1]])
    again = search.cell_sums_exact_ref(rows, weights, offsets, shuffled, scale)
    assert all(np.array_equal(a, b) for a, b in zip((sums, wsums, counts), again))
  # the items re-inserted in another order, the labels permuted alike
  perm = rng.permutation(len(ids))
  again = search.cell_sums_exact_ref(rows[perm], weights[perm], *search.cell_lists(ids[perm], c),
                                     search.sum_scale_ref(rows[perm], weights[perm]))
  assert all(np.array_equal(a, b) for a, b in zip((sums, wsums, counts), again))
  # any split into "shards", each with its own rows and item numbers, under the global scale: the results add
  for shards in (2, 3, 5):
    owner = rng.randint(0, shards, size=len(ids))
    owner[:40] = 0                                                 # uneven; shard 1 of 5 may be small
    total, wtotal, n = np.zeros_like(sums), np.zeros_like(wsums), np.zeros_like(counts)
    for s in range(shards):
      mine = np.flatnonzero(owner == s)
      part = search.cell_sums_exact_ref(rows[mine], weights[mine], *search.cell_lists(ids[mine], c), scale)
      total, wtotal, n = total + part[0], wtotal + part[1], n + part[2]
    assert np.array_equal(total, sums) and np.array_equal(wtotal, wsums) and np.array_equal(n, counts)
  # torch tensors are taken as well
  again = search.cell_sums_exact_ref(torch.from_numpy(rows), torch.from_numpy(weights), torch.from_numpy(offsets),
                                     torch.from_numpy(items), scale)
  assert all(np.array_equal(a, b) for a, b in zip((sums, wsums, counts), again))


def test_exact_sums_are_within_the_stated_bound_of_fp64():
  """|S - sum f| <= n_c 2^(E - B - 1) + ulp32(S) / 2 per column: half a unit per term, half an ulp for the one conversion."""
  from mmt_amd import search
  rows, weights, ids, c = _random_case(seed=1)
  scale = search.sum_scale_ref(rows, weights)
  offsets, items = search.cell_lists(ids, c)
  sums, wsums, counts = search.cell_sums_exact_ref(rows, weights, offsets, items, scale)
  for table, got, e in ((rows, sums, scale.exponent), (weights, wsums, scale.wexponent)):
    back = search.exact_sums_float(got, e, scale.bits)
    assert back.dtype == np.float32
    for ci in range(c):
      members = table[ids == ci].astype(np.float64)
      want = np.array([math.fsum(column) for column in members.T])   # the fp64 sum, correctly rounded: half an ulp64 off
      ulp = np.spacing(np.abs(back[ci])).astype(np.float64)
      bound = counts[ci] * 2.0 ** (e - scale.bits - 1) + ulp / 2 + np.spacing(np.abs(want)) / 2
      assert (np.abs(back[ci].astype(np.float64) - want) <= bound).all(), ci


def test_on_exact_data_the_exact_sums_are_the_fp32_sums_bit_for_bit():
  """Values k / 8 and weights in {0, 1/4, 1/2}: every term and every partial fp32 sum is exact, so the two accumulators
  must agree in every bit."""
  from mmt_amd import search
  ids, num_cells = _labels(5)
  rng = np.random.RandomState(1)
  rows = (rng.randint(-8, 9, size=(len(ids), 12)) / 8).astype(np.float32)
  weights = (rng.randint(0, 3, size=(len(ids), 3)) / 4).astype(np.float32)
  offsets, items = search.cell_lists(ids, num_cells)
  scale = search.sum_scale_ref(rows, weights)
  assert (scale.exponent, scale.wexponent) == (0, -1)
  sums, wsums, counts = search.cell_sums_exact_ref(rows, weights, offsets, items, scale)
  want = search.cell_sums_ref(rows, weights, offsets, items, 5)
  got = (search.exact_sums_float(sums, scale.exponent, scale.bits), search.exact_sums_float(wsums, scale.wexponent, scale.bits))
  for a, b in zip(got, want):
    assert a.dtype == np.float32 and np.array_equal(a.view(np.int32), b.view(np.int32))
  assert np.array_equal(counts, want[2])


def test_sum_scale_ref_takes_the_least_exponent():
  from mmt_amd import search
  one = np.zeros((4, 8), np.float32)
  w = np.full((4, 2), 0.25, np.float32)
  assert search.sum_scale_ref(one, np.zeros((4, 2), np.float32)) == search.SumScale(0, 0, search.lse_bits(4), 4)   # all zero
  one[2, 3] = -1.0
  assert search.sum_scale_ref(one, w).exponent == 0 and search.sum_scale_ref(one, w).wexponent == -2
  one[1, 1] = np.nextafter(np.float32(1), np.float32(2))
  assert search.sum_scale_ref(one, w).exponent == 1
  for value, e in ((0.5, -1), (0.75, 0), (3.0, 2), (4.0, 2), (2.0 ** -149, -149), (2.0 ** -126, -126),
                   (float(np.finfo(np.float32).max), 128)):
    assert search.sum_scale_ref(np.full((1, 4), -value, np.float32), w[:1]).exponent == e, value
    assert search.sum_scale_ref(one[:1] * 0, np.full((1, 2), value, np.float32)).wexponent == e, value
  # the largest of the parts' exponents is the exponent of the whole; bits come from the whole's size
  rows, weights, _, _ = _random_case(seed=2)
  whole = search.sum_scale_ref(rows, weights)
  cuts = (0, 40, 1000, 1001, 3000)
  parts = [search.sum_scale_ref(rows[a:b], weights[a:b]) for a, b in zip(cuts, cuts[1:])]
  assert max(p.exponent for p in parts) == whole.exponent and max(p.wexponent for p in parts) == whole.wexponent
  assert whole.bits == search.lse_bits(3000) == 62 - 12
  with pytest.raises(ValueError, match='SumScale: bits must be lse_bits'):
    search.SumScale(0, 0, 61, 3000)
  for bad in (161, -161, True, 1.0):
    with pytest.raises(ValueError, match='SumScale: exponent must be an int'):
      search.SumScale(bad, 0, 50, 3000)


def test_terms_round_to_nearest_even_and_clamp():
  from mmt_amd import search
  n = 4
  bits = search.lse_bits(n)
  unit = 2.0 ** -bits
  values = np.array([[1.0, -1.0, unit / 2, -unit / 2, 3 * unit / 2, -3 * unit / 2, 2.0 ** -149, -0.0, unit, 0.75 * unit,
                      2.0, -8.0]], np.float32)
  scale = search.SumScale(0, 0, bits, n)
  got = search.cell_sums_exact_ref(values, np.zeros((1, 1), np.float32), np.array([0, 1]), np.array([0]), scale)[0][0]
  assert got.tolist() == [2 ** bits, -2 ** bits, 0, 0, 2, -2, 0, 0, 1, 1, 2 ** bits, -2 ** bits]   # the last two: clamped


def test_the_way_back_to_fp32_rounds_once():
  from mmt_amd import search
  cases = {2 ** 53 + 2 ** 29 + 1: 2.0 ** 53 + 2.0 ** 30,           # through fp64 it would be 2^53 first, then a tie down
           2 ** 40 + 2 ** 16: 2.0 ** 40,                           # a tie: to even, down
           2 ** 40 + 3 * 2 ** 16: 2.0 ** 40 + 2.0 ** 18,           # a tie: to even, up
           2 ** 24 + 1: 2.0 ** 24, 2 ** 24 + 3: 2.0 ** 24 + 4, 5: 5.0, 0: 0.0, 2 ** 62: 2.0 ** 62}
  ints = np.array(list(cases) + [-v for v in cases], np.int64)
  want = np.array(list(cases.values()) + [-v for v in cases.values()], np.float32)
  for shift in (0, -61, 7):
    got = search.exact_sums_float(ints, shift + 50, 50)
    assert got.dtype == np.float32 and np.array_equal(got, np.ldexp(want, shift))
  twice = (ints.astype(np.float64)).astype(np.float32)
  assert twice[0] != want[0]                                       # the detour the definition rules out
  assert search.exact_sums_float(torch.from_numpy(ints), 50, 50).tolist() == want.tolist()


def test_argument_errors_are_raised_without_a_device():
  from mmt_amd import search
  from mmt_amd.search import CellQuantiser, SumScale
  index = _hollow_index(5)
  cells = _hollow_cells(index)
  good = SumScale(0, 0, search.lse_bits(5), 5)
  # exact must be a bool; scale= goes with it
  for bad in (1, 0, None, 'yes'):
    with pytest.raises(ValueError, match='cell_centroids: exact must be a bool'):
      index.cell_centroids(cells, exact=bad)
    with pytest.raises(ValueError, match='train_cells: exact must be a bool'):
      index.train_cells(2, exact=bad)
  with pytest.raises(ValueError, match='cell_centroids: scale= goes with exact=True'):
    index.cell_centroids(cells, scale=good)
  # the options refused by name, and unknown ones
  for name in search._NOT_TRAINED:
    with pytest.raises(ValueError, match='cell_sums_exact: %s= is out of scope' % name):
      index.cell_sums_exact(cells, **{name: None})
  with pytest.raises(TypeError):
    index.cell_sums_exact(cells, k=3)
  # cells: type, origin, age
  other = _hollow_index(5)
  for bad in (None, torch.zeros(3), _hollow_cells(other), _hollow_cells(index, sharded=True)):
    with pytest.raises(ValueError, match=r'cell_sums_exact: cells must come from the cells\(\) or cells_from_centres\(\) of this index'):
      index.cell_sums_exact(bad, scale=good)
    with pytest.raises(ValueError, match=r'cell_centroids: cells must come from the cells\(\) or cells_from_centres\(\) of this index'):
      index.cell_centroids(bad, exact=True, scale=good)
  # a scale: type, age, origin
  stale = SumScale(0, 0, search.lse_bits(4), 4)
  foreign = SumScale(0, 0, search.lse_bits(5), 5)
  foreign._index = other
  for who, call in (('cell_sums_exact', lambda s: index.cell_sums_exact(cells, scale=s)),
                    ('cell_centroids', lambda s: index.cell_centroids(cells, exact=True, scale=s))):
    for bad in ((0, 0), 'scale', 1.0):
      with pytest.raises(ValueError, match='%s: scale must be a SumScale' % who):
        call(bad)
    with pytest.raises(ValueError, match='%s: the scale was built for 4 items, the index holds 5' % who):
      call(stale)
    with pytest.raises(ValueError, match='%s: the scale belongs to another index' % who):
      call(foreign)
  index.num_items = 6
  with pytest.raises(ValueError, match='cell_sums_exact: the cells were built for 5 items, the index holds 6'):
    index.cell_sums_exact(cells, scale=good)
  index.num_items = 5
  with pytest.raises(ValueError, match='cell_centroids: out must be a pair of tensors'):
    index.cell_centroids(cells, out=torch.zeros(3, 2, 8), exact=True, scale=good)
  with pytest.raises(ValueError, match='sum_scale: the index holds no items'):
    _hollow_index(0).sum_scale()
  # assign_cells
  quantiser = CellQuantiser.__new__(CellQuantiser)
  for bad in (None, index, 'quantiser'):
    with pytest.raises(ValueError, match='assign_cells: quantiser must be a CellQuantiser'):
      index.assign_cells(bad)
  with pytest.raises(ValueError, match='assign_cells: the index holds no items'):
    _hollow_index(0).assign_cells(quantiser)
  quantiser.centroids = _hollow_index(3, dtype=torch.bfloat16)
  with pytest.raises(ValueError, match=r'assign_cells: the quantiser holds \(dtype, num_experts, dim\)'):
    index.assign_cells(quantiser)
  # a quantiser records how it was trained
  plain = CellQuantiser(_hollow_index(3), None, None, torch.zeros(2), torch.zeros(2))
  assert plain.exact is False and plain.scale is None and plain.iterations == 2 and plain.num_cells == 3


def test_a_sharded_index_takes_the_exact_calls_and_keeps_refusing_the_others():
  from mmt_amd import search
  from mmt_amd.search import CellQuantiser, SumScale
  index = _hollow_sharded(5)
  cells = _hollow_cells(index, sharded=True)
  good = SumScale(0, 0, search.lse_bits(5), 5)
  for who, args in (('train_cells', (2,)), ('cell_sums', (cells,)), ('cell_centroids', (cells,))):
    with pytest.raises(ValueError, match='%s: not available on a ShardedVideoIndex' % who):
      getattr(index, who)(*args)
  for who, args in (('train_cells', (2,)), ('cell_centroids', (cells,))):
    with pytest.raises(ValueError, match='%s: not available on a ShardedVideoIndex.*exact=True' % who):
      getattr(index, who)(*args, exact=False)
    with pytest.raises(ValueError, match='%s: exact must be a bool' % who):
      getattr(index, who)(*args, exact=1)
  with pytest.raises(ValueError, match='cell_sums: not available on a ShardedVideoIndex.*cell_sums_exact'):
    index.cell_sums(cells)
  quantiser = CellQuantiser.__new__(CellQuantiser)
  with pytest.raises(ValueError, match='assign: not available on a ShardedVideoIndex.*assign_cells'):
    quantiser.assign(index)
  # the exact calls reach their own checks
  for name in search._NOT_TRAINED:
    with pytest.raises(ValueError, match='train_cells: %s= is out of scope' % name):
      index.train_cells(2, exact=True, **{name: None})
    with pytest.raises(ValueError, match='cell_centroids: %s= is out of scope' % name):
      index.cell_centroids(cells, exact=True, **{name: None})
  for bad in (0, -1, True, 2.0, None, 2 ** 31):
    with pytest.raises(ValueError, match='train_cells: num_cells must be an int'):
      index.train_cells(bad, exact=True)
  with pytest.raises(ValueError, match='train_cells: iters must be an int >= 1'):
    index.train_cells(2, iters=0, exact=True)
  with pytest.raises(ValueError, match='train_cells: init must be on the index device'):
    index.train_cells(2, init=torch.zeros(2, dtype=torch.int64), exact=True)
  with pytest.raises(ValueError, match='train_cells: the index holds no items'):
    _hollow_sharded(0).train_cells(1, exact=True)
  plain = _hollow_cells(_hollow_index(5))
  for bad in (None, plain, _hollow_cells(_hollow_sharded(5), sharded=True)):
    with pytest.raises(ValueError, match='cell_sums_exact: cells must come from'):
      index.cell_sums_exact(bad, scale=good)
    with pytest.raises(ValueError, match='cell_centroids: cells must come from'):
      index.cell_centroids(bad, exact=True, scale=good)
  with pytest.raises(ValueError, match='cell_sums_exact: the scale was built for 4 items, the index holds 5'):
    index.cell_sums_exact(cells, scale=SumScale(0, 0, search.lse_bits(4), 4))
  with pytest.raises(ValueError, match='cell_centroids: scale must be a SumScale'):
    index.cell_centroids(cells, exact=True, scale=(0, 0))
  with pytest.raises(ValueError, match='assign_cells: quantiser must be a CellQuantiser'):
    index.assign_cells(None)
  with pytest.raises(ValueError, match='sum_scale: the index holds no items'):
    _hollow_sharded(0).sum_scale()
