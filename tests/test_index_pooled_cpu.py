"""The host side of query-set pooling (VideoIndex.pooling and pooling= of the scans; mmt_search_topk_pooled,
mmt_search_thresholds_pooled, mmt_search_count_pooled and their bf16 forms) without a GPU: the definition the GPU tests hold
the kernels to, that definition against the reference's 'avg' similarities, the header and the ctypes table, the argument
gates of the entry points and the argument errors of the calls."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests.fixtures import load_npz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = ('mmt_topk_pooled_workspace_keys', 'mmt_count_pooled_workspace_ints')
F32 = np.float32


def brute_pooled(matrix, C, rw, mode):
  """The definition, in numpy float32: matrix [NS * C, NV] (row r's scores) and row weights rw [NS * C] -> [NS, NV].  Set s
  is rows s * C .. s * C + C - 1; a row with rw == 0 takes no part; over the participating rows in row order
    'mean': v = fl(rw[r0] * s_r0), then v = fl(v + fl(rw[ri] * s_ri))  (numpy rounds every float32 product and sum: no fma)
    'max' : v = s_r0, then v = s_ri where s_ri > v                      (the first of equal values stays)
  A set without a participating row gives 0."""
  assert mode in ('mean', 'max')
  matrix = np.ascontiguousarray(matrix, F32)
  rw = np.ascontiguousarray(rw, F32).reshape(-1)
  nq, nv = matrix.shape
  assert nq % C == 0 and rw.shape == (nq,)
  ns = nq // C
  rows, w = matrix.reshape(ns, C, nv), rw.reshape(ns, C)
  out = np.zeros((ns, nv), F32)
  have = np.zeros(ns, bool)
  for c in range(C):
    part = w[:, c] != 0
    x = rows[:, c]
    if mode == 'mean':
      p = w[:, c:c + 1] * x                      # float32 * float32, rounded
      new = np.where(have[:, None], out + p, p)  # float32 + float32, rounded
    else:
      new = np.where(have[:, None] & ~(x > out), out, x)
    out = np.where(part[:, None], new, out).astype(F32)
    have |= part
  return out


def test_brute_pooled_on_hand_made_rows():
  m = F32([[1, -0.0, 3, 5], [2, 0.0, 3, -7], [4, -0.0, 1, 2], [0.5, 0.5, 0.5, 0.5]])
  one = np.ones(4, F32)
  assert brute_pooled(m, 1, one, 'mean').tolist() == m.tolist() and brute_pooled(m, 1, one, 'max').tolist() == m.tolist()
  mx = brute_pooled(m, 2, one, 'max')
  assert mx.tolist() == [[2, 0, 3, 5], [4, 0.5, 1, 2]] and np.signbit(mx[0, 1])    # -0 then +0: the first of equals stays
  mean = brute_pooled(m, 2, F32([0.5, 0.5, 0.5, 0.5]), 'mean')
  assert mean.tolist() == [[1.5, 0, 3, -1], [2.25, 0.25, 0.75, 1.25]]
  masked = brute_pooled(m, 4, F32([0, 2, 0, -1]), 'mean')                           # rows 0 and 2 take no part
  assert masked.tolist() == [[3.5, -0.5, 5.5, -14.5]]
  assert brute_pooled(m, 4, F32([0, 2, 0, -1]), 'max').tolist() == [[2, 0.5, 3, 0.5]]
  assert brute_pooled(m, 2, F32([0, 0, 1, 0]), 'max').tolist() == [[0, 0, 0, 0], [4, -0.0, 1, 2]]
  # rounded product, then rounded sum, in row order: not an fma and not another order
  a, b = F32(1 + 2.0 ** -12), F32(-(1 + 2.0 ** -11))
  assert np.float64(a) * np.float64(a) + np.float64(b) == 2.0 ** -24              # what an fma of the second step gives
  assert brute_pooled(F32([[a], [1]]), 2, F32([a, b]), 'mean')[0, 0] == 0           # fl(a * a) = 1 + 2^-11: the tie to even
  big = brute_pooled(F32([[1], [2.0 ** -24], [2.0 ** -24]]), 3, one[:3], 'mean')[0, 0]
  assert big == 1 and brute_pooled(F32([[2.0 ** -24], [2.0 ** -24], [1]]), 3, one[:3], 'mean')[0, 0] > 1   # row order


def test_mean_of_the_reference_indep_similarities_is_its_avg_mode():
  """model/model.py:826-831: 'avg' is the mean over a video's captions of the 'indep' similarities.  Tolerance: the 1e-5
  tests/test_oracle_golden.py uses on this file."""
  g = load_npz('sim_loss_metric')
  indep, avg = g['sims_indep'], g['sims_avg']
  b, c = avg.shape[0], indep.shape[0] // avg.shape[0]
  assert indep.shape == (b * c, avg.shape[1]) and c == g['sim_in_tw'].shape[1] == 3
  got = brute_pooled(indep, c, np.full(b * c, F32(1) / F32(c), F32), 'mean')
  assert got.shape == avg.shape and got.dtype == F32
  assert np.abs(got - avg).max() < 1e-5


def _params(src, name):
  m = re.search(r'\b(int|int64_t) %s\(([^;]*?)\);' % name, src)
  assert m, name + ' is not declared in mmt_hip.h'
  return m.group(1), [p.strip() for p in m.group(2).replace('\n', ' ').split(',')]


def test_signatures_of_the_new_exports_agree_with_the_header():
  from mmt_amd import _lib
  src = open(os.path.join(ROOT, 'include', 'mmt_hip.h')).read()
  handle = ctypes.CDLL(_lib.LIB_PATH)
  arity = dict(zip(SIZES, (4, 4)))
  for name in SIZES:
    res_name, params = _params(src, name)
    res, args = _lib.SIGNATURES[name]
    assert res is (ctypes.c_int if res_name == 'int' else ctypes.c_int64), name
    assert (res_name == 'int64_t') == (name in SIZES)
    assert len(args) == len(params) == arity[name], name
    for p, a in zip(params, args):
      assert (a is ctypes.c_void_p) == ('*' in p) and (a is ctypes.c_int) == (p.startswith('int ')), (name, p)
    assert hasattr(handle, name)
  assert handle.mmt_abi_version() == 6
  assert _lib.lib().mmt_abi_version() == 6                  # and every declared symbol binds


def _fns():
  from mmt_amd import _lib
  handle = ctypes.CDLL(_lib.LIB_PATH)
  fns = {}
  for name in SIZES:
    fns[name] = getattr(handle, name)
    fns[name].restype, fns[name].argtypes = _lib.SIGNATURES[name]
  return fns


def test_workspace_sizes_follow_the_query_blocks():
  """A block holds 64 // C sets; the chunk rule of the unpooled scans (4096 columns, halved down to 128 while the launch has
  fewer than 512 blocks) is taken from the number of blocks."""
  from mmt_amd import _lib
  fns = _fns()
  keys, ints = fns['mmt_topk_pooled_workspace_keys'], fns['mmt_count_pooled_workspace_ints']
  plain = _lib.lib().mmt_topk_workspace_keys
  for ns, c, nv, k in ((1, 1, 1, 1), (130, 4, 14600, 10), (3, 64, 257, 128), (9, 8, 4097, 10), (33, 2, 129, 1),
                       (1000, 33, 100000, 7), (70000, 1, 5000, 3)):
    blocks = -(-ns // (64 // c))
    chunk = 4096
    while chunk > 128 and blocks * -(-nv // chunk) < 512:
      chunk //= 2
    assert keys(ns, c, nv, k) == ns * -(-nv // chunk) * k, (ns, c, nv, k)
    assert ints(ns, c, nv, k % 32 + 1) == ns * (k % 32 + 1) * 2 * -(-nv // chunk)
    if c == 1:
      assert keys(ns, c, nv, k) == plain(ns, nv, k)         # sets of one row: the unpooled geometry
  assert keys(130, 4, 14600, 10) == 130 * 58 * 10           # 9 blocks of 16 sets x 58 chunks of 256 columns
  for bad in ((0, 1, 1, 1), (1, 0, 1, 1), (1, 65, 1, 1), (1, -1, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0), (2 ** 26, 64, 1, 1)):
    assert keys(*bad) == -1 and ints(*bad) == -1, bad
  assert keys(1, 1, 1, 129) == -1 and ints(1, 1, 1, 33) == -1


def _hollow_index(num_items, dtype=torch.float32):
  """A VideoIndex with its bookkeeping and no storage: the argument checks come before anything reads it."""
  from mmt_amd.search import VideoIndex
  index = VideoIndex.__new__(VideoIndex)
  index.capacity, index.num_experts, index.dim, index.num_items = 8, 2, 8, num_items
  index.device, index.dtype = torch.device('cuda', 0), dtype
  return index


def _hollow_sharded(num_items):
  from mmt_amd.search import ShardedVideoIndex
  sharded = ShardedVideoIndex.__new__(ShardedVideoIndex)
  sharded.num_items, sharded.num_experts, sharded.dim, sharded.device = num_items, 2, 8, torch.device('cuda', 0)
  sharded.shards = []
  return sharded


@pytest.mark.parametrize('hollow', [_hollow_index, _hollow_sharded], ids=['VideoIndex', 'ShardedVideoIndex'])
def test_argument_errors_are_raised_without_a_device(hollow):
  from mmt_amd.search import MAX_SET, QueryPooling, ShardedVideoIndex, VideoIndex
  assert MAX_SET == 64
  index = hollow(5)
  # the factory: sizes and mode first, then the weights
  for bad in (0, 65, -1):
    with pytest.raises(ValueError, match=r'set_size must lie in 1\.\.64'):
      index.pooling(bad, 2)
  for bad in (2.0, True, None, '3'):
    with pytest.raises(ValueError, match='set_size must be an int'):
      index.pooling(bad, 2)
    with pytest.raises(ValueError, match='num_sets must be an int'):
      index.pooling(2, bad)
  for bad in (-1, 2 ** 31):
    with pytest.raises(ValueError, match='num_sets must be >= 0'):
      index.pooling(2, bad)
  for bad in ('avg', 'sum', None, 0):
    with pytest.raises(ValueError, match="mode must be 'mean' or 'max'"):
      index.pooling(2, 3, mode=bad)
  w = torch.tensor([0.5, 0.5, 0.0, 1.0, -2.0, 0.0])
  for bad in (w.tolist(), w.numpy(), w.double(), w.to(torch.bfloat16), (w * 2).long()):
    with pytest.raises(ValueError, match='row_weights must be a float32 tensor'):
      index.pooling(2, 3, bad)
  with pytest.raises(ValueError, match='index device'):
    index.pooling(2, 3, w)                                       # host weights for a device index
  index.device = torch.device('cpu')                             # lets the value checks be reached with host tensors
  for bad in (w[:5], w.reshape(2, 3), w.reshape(6, 1), torch.zeros(7), torch.tensor(1.0)):
    with pytest.raises(ValueError, match=r'row_weights of shape \(6,\) or \(3, 2\) expected'):
      index.pooling(2, 3, bad)
  for value in (float('nan'), float('inf'), -float('inf')):
    bad = w.clone()
    bad[4] = value
    with pytest.raises(ValueError, match='row_weights must be finite'):
      index.pooling(2, 3, bad)
  with pytest.raises(ValueError, match='every set needs a row'):
    index.pooling(2, 3, torch.tensor([0.5, 0.5, 0.0, -0.0, -2.0, 0.0]))
  pool = index.pooling(2, 3, w, mode='max')                       # nothing of the build needs the device
  assert isinstance(pool, QueryPooling) and (pool.set_size, pool.num_sets, pool.num_rows, pool.mode) == (2, 3, 6, 'max')
  assert pool.device == index.device and pool.weights.dtype == torch.float32 and pool.weights.tolist() == w.tolist()
  assert pool.weights.data_ptr() != w.data_ptr()                  # a copy of its own
  assert index.pooling(2, 3, w.reshape(3, 2)).weights.tolist() == w.tolist()
  default = index.pooling(3, 2)
  assert default.mode == 'mean' and default.weights.tolist() == [float(np.float32(1) / np.float32(3))] * 6
  assert index.pooling(64, 0).num_rows == 0 and index.pooling(1, 4).weights.tolist() == [1.0] * 4
  # the calls: pooling's type, device and combinations, then the queries, then their count
  q, qw = torch.zeros(6, 2, 8), torch.zeros(6, 2)
  tg = torch.zeros(3, dtype=torch.int64)
  thr = torch.zeros(3)
  calls = [('search', lambda **kw: index.search(q, qw, **kw)), ('ranks', lambda **kw: index.rank_counts(q, qw, tg, **kw)),
           ('ranks', lambda **kw: index.ranks(q, qw, tg, **kw))]
  if hollow is _hollow_index:
    calls += [('ranks', lambda **kw: index.target_scores(q, qw, tg, **kw)),
              ('ranks', lambda **kw: index.threshold_counts(q, qw, thr, **kw))]
  for who, call in calls:
    for foreign in (w, 2, 'mean', (2, 3)):
      with pytest.raises(ValueError, match=who + r': pooling must come from pooling\(\)'):
        call(pooling=foreign)
    with pytest.raises(ValueError, match='does not combine with exclude= or norm='):
      call(pooling=pool, norm=object())
    with pytest.raises(ValueError, match='CUDA tensor'):
      call(pooling=pool)                                          # the queries themselves are host tensors
  index.device = torch.device('cuda', 0)
  with pytest.raises(ValueError, match='search: the pooling is on cpu, the index on cuda:0'):
    index.search(q, qw, pooling=pool)
  index.device = torch.device('cpu')
  with pytest.raises(ValueError, match='does not combine with exclude= or norm='):
    index.search(q, qw, pooling=pool, exclude=torch.zeros(6, dtype=torch.int64))
  # the row count is held against the pooling before anything is scored: host "CUDA" queries are refused earlier, so the
  # check is reached through _queries
  index._queries = lambda embds, weights: (embds, weights)
  for who, call in calls:
    with pytest.raises(ValueError, match=who + r': 6 queries but the pooling has 8 rows \(4 sets of 2\)'):
      call(pooling=index.pooling(2, 4))
  for call in (lambda: index.rank_counts(q, qw, torch.zeros(6, dtype=torch.int64), pooling=pool),
               lambda: index.ranks(q, qw, torch.zeros(2, 2, dtype=torch.int64), pooling=pool)):
    with pytest.raises(ValueError, match='ranks: 3 query sets but targets'):
      call()
  if hollow is _hollow_index:
    with pytest.raises(ValueError, match='ranks: 3 query sets but thresholds'):
      index.threshold_counts(q, qw, torch.zeros(6), pooling=pool)
  # search_groups and range_search take no pooling
  for method in ('search_groups', 'range_search'):
    assert 'pooling' not in inspect.signature(getattr(VideoIndex, method)).parameters
    assert 'pooling' not in inspect.signature(getattr(ShardedVideoIndex, method)).parameters
  # both classes have one surface
  for method in ('pooling', 'search', 'rank_counts', 'ranks'):
    assert (inspect.signature(getattr(ShardedVideoIndex, method)).parameters.keys() ==
            inspect.signature(getattr(VideoIndex, method)).parameters.keys())
    if method != 'pooling':
      assert inspect.signature(getattr(VideoIndex, method)).parameters['pooling'].default is None
  assert list(inspect.signature(VideoIndex.pooling).parameters) == ['self', 'set_size', 'num_sets', 'row_weights', 'mode']
  assert inspect.signature(VideoIndex.pooling).parameters['mode'].default == 'mean'
  for method in ('target_scores', 'threshold_counts'):
    assert inspect.signature(getattr(VideoIndex, method)).parameters['pooling'].default is None


def test_row_batches_are_cut_at_whole_blocks_of_whole_sets():
  from mmt_amd import search
  index = _hollow_index(5000)
  index.num_experts, index.dim = 7, 512
  per_row = 7 * 512 * 4
  for c in (1, 3, 5, 20, 33, 64):
    block = 64 // c * c
    pool = search.QueryPooling(c, 4000, torch.zeros(4000 * c), 'mean')
    batches = index._row_batches(pool.num_rows, 8 * 10 * 2, pool)
    assert batches[0][0] == 0 and batches[-1][1] == pool.num_rows and len(batches) > 1
    assert all(a[1] == b[0] for a, b in zip(batches, batches[1:]))
    assert all(r0 % block == 0 and (r1 - r0) % c == 0 for r0, r1 in batches)
    assert all((r1 - r0) % block == 0 for r0, r1 in batches[:-1])
    assert all((r1 - r0) * per_row <= search._BATCH_BYTES for r0, r1 in batches)
  assert index._row_batches(200, 0) == [(0, 200)] and index._row_batches(200, 0, None) == [(0, 200)]
