"""The host side of reverse search and CSLS normalisation (search.VideoIndex.reverse_search and csls_norm;
mmt_search_col_topk and mmt_col_topk_workspace_keys) without a GPU: the numpy restatement of the CSLS term r[g] the GPU
tests hold the kernel to, its derived bound against fp64, the header and the ctypes table, the gates of the new entry --
every one refused on the host, before any launch -- and the Python errors that need no device."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests.test_index_ranks_cpu import _hollow_index

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ('mmt_col_topk_workspace_keys', 'mmt_search_col_topk')
F32 = np.float32
MAX_RK = 32


def csls_r32(lists):
  """The recipe of mmt_search_col_topk's mean restated in numpy float32: lists fp32 [n, k'] (an item's k' best scores in
  list order) -> r fp32 [n]: v = s_0, v = fl(v + s_i) for i = 1 .. k' - 1, r = fl(v * float32(1 / k')).  No fma, no division
  on the device, so this is the device's value bit for bit."""
  lists = np.asarray(lists, F32)
  v = lists[:, 0].copy()
  for i in range(1, lists.shape[1]):
    v = (v + lists[:, i]).astype(F32)
  return (v * F32(1.0 / lists.shape[1])).astype(F32)


def csls_bound(lists):
  """2^-23 (k' + 1) mean|s_i| + 2^-149 per item: the bound of |r - fp64 mean|.  Derived, with u = 2^-24: a sequential sum of
  k' terms is off by at most (k' - 1) u sum|s_i| to first order; the weight float32(1 / k') is off by u / k' and the product
  is rounded once, each at most u |sum| / k' <= u mean|s_i|: together (k' + 1) u mean|s_i|.  The factor 2 (2^-23 for u)
  covers the second-order terms -- (1 + u)^(k' + 1) - 1 <= 2 (k' + 1) u for k' <= 32 by a wide margin -- and 2^-149 a
  product that lands in the subnormal range."""
  a = np.abs(np.asarray(lists, np.float64))
  return 2.0 ** -23 * (a.shape[1] + 1) * a.mean(1) + 2.0 ** -149


def _bits(x):
  return np.ascontiguousarray(x, F32).view(np.int32)


def test_restatement_on_hand_made_cases():
  assert csls_r32(F32([[0.3]])).tolist() == [float(F32(0.3))]                    # k' = 1: the score itself, times 1
  assert csls_r32(F32([[1.0, 3.0]])).tolist() == [2.0]
  assert csls_r32(F32([[0.0, -0.0, 0.0]])).tolist() == [0.0]
  # the chain is sequential: (2^24 + 1) rounds to 2^24 at every step, a pairwise sum of the ones would keep them
  row = F32([[2.0 ** 24, 1.0, 1.0, 1.0]])
  assert csls_r32(row).tolist() == [2.0 ** 22]
  assert csls_r32(row[:, ::-1].copy()).tolist() == [float(F32(2.0 ** 24 + 4) * F32(0.25))] != [2.0 ** 22]
  # the weight is float32(1 / k') and the last step a multiply, not a division: fl(5 * fl(1 / 3)) is not fl(5 / 3)
  third = F32(1.0 / 3)
  got = csls_r32(F32([[5.0, 0.0, 0.0]]))
  assert _bits(got)[0] == _bits(F32(5.0) * third) and got[0] != F32(5.0) / F32(3.0)
  out = csls_r32(F32([[1.0, 2.0], [3.0, 5.0]]))
  assert out.dtype == F32 and out.tolist() == [1.5, 4.0]


def test_restatement_stays_within_the_derived_bound_of_the_fp64_mean():
  rng = np.random.default_rng(0)
  worst = 0.0
  for k in range(1, MAX_RK + 1):
    descending = -np.sort(-rng.standard_normal((400, k)), axis=1)                # what a list looks like
    alternating = (rng.random((400, k)) + 0.5) * np.where(np.arange(k) % 2 == 0, 1.0, -1.0)   # cancelling sums
    huge = rng.standard_normal((400, k))
    huge[:, rng.integers(0, k)] *= 2.0 ** 40                                     # one term dwarfs the others
    tiny = rng.standard_normal((400, k)) * 2.0 ** -140                           # the product is subnormal
    equal = np.repeat(rng.standard_normal((400, 1)), k, 1)
    for lists in (descending, alternating, huge, tiny, equal, rng.standard_normal((400, k)) * 1e-3):
      lists = lists.astype(F32)
      err = np.abs(csls_r32(lists).astype(np.float64) - lists.astype(np.float64).mean(1))
      bound = csls_bound(lists)
      assert (err <= bound).all(), (k, float((err / bound).max()))
      worst = max(worst, float((err / bound).max()))
  print('restatement err / bound at most %.3f' % worst)
  assert 0 < worst <= 1


def _params(name, src):
  m = re.search(r'\b(int|int64_t) %s\(([^;]*?)\);' % name, src)
  assert m, name + ' is not declared in mmt_hip.h'
  return m.group(1), [p.strip() for p in m.group(2).replace('\n', ' ').split(',')]


def test_signatures_of_the_new_exports_agree_with_the_header():
  from mmt_amd import _lib
  src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'mmt_hip.h')).read(), flags=re.S)
  handle = ctypes.CDLL(_lib.LIB_PATH)
  for name in NEW_EXPORTS:
    restype, params = _params(name, src)
    res, args = _lib.SIGNATURES[name]
    assert res is (ctypes.c_int if restype == 'int' else ctypes.c_int64) and len(args) == len(params), name
    for p, a in zip(params, args):
      pointer = '*' in p
      assert (a is ctypes.c_void_p or a is ctypes.POINTER(_lib.MmtSearchScan)) == pointer, (name, p)
      assert (a is ctypes.c_int) == p.startswith('int '), (name, p)
      assert (a is ctypes.c_float) == (p.startswith('float ') and not pointer), (name, p)
    assert hasattr(handle, name)
  _, params = _params('mmt_search_col_topk', src)
  args = _lib.SIGNATURES['mmt_search_col_topk'][1]
  assert params[0] == 'const MmtSearchScan* scan' and params[-1] == 'void* stream'
  assert args[0] is ctypes.POINTER(_lib.MmtSearchScan) and args[-1] is ctypes.c_void_p
  assert [p.split()[-1].lstrip('*') for p in params[1:-1]] == ['k', 'row0', 'ws', 'state', 'first', 'scores', 'rows', 'mean',
                                                               'mean_weight']
  assert int(re.search(r'#define MMT_SEARCH_MAX_RK (\d+)', src).group(1)) == MAX_RK
  from mmt_amd import search
  assert search.MAX_RK == MAX_RK
  assert handle.mmt_abi_version() == 6 and 'sizeof(MmtSearchScan) == 128' in src   # additive: neither moved


_buf = (ctypes.c_char * 256)()
P = ctypes.addressof(_buf) + -ctypes.addressof(_buf) % 16        # 16-byte aligned, never dereferenced: every call is refused
STORAGES = {'fp32': 0, 'bf16': 1, 'fp8': 2}


def _descriptor(store, **changes):
  """A descriptor the gate accepts: NQ = NV = M = 1, d = 16 (a multiple for every storage), no options."""
  from mmt_amd import _lib
  f = dict(q=P, q_lo=None if store == 'fp32' else P, qw=P, g=P, gw=P, gscale=P if store == 'fp8' else None, subset=None,
           exclude=None, after=None, lse=None, set_weights=None, storage=STORAGES[store], NQ=1, NV=1, M=1, d=16, E=0, beta=0.0,
           sets=0, set_size=0, mode=0)
  f.update(changes)
  return _lib.MmtSearchScan(**f)


def _call(desc, **own):
  from mmt_amd import _lib
  a = dict(k=1, row0=0, ws=P, state=P, first=1, scores=P, rows=P, mean=P, mean_weight=1.0)
  a.update(own)
  return _lib.lib().mmt_search_col_topk(None if desc is None else ctypes.byref(desc), a['k'], a['row0'], a['ws'], a['state'],
                                        a['first'], a['scores'], a['rows'], a['mean'], a['mean_weight'], None)


def test_the_new_entry_gates_its_arguments_on_the_host():
  """Every call below is refused before any launch: MMT_ERR_ARG = -1, MMT_ERR_ALIGN = -2.  A call that passes every
  argument gate is recognised by the alignment refusal only it reaches; a knock-out that must give -1 is made with the query
  rows misaligned as well, so a gate that has gone missing shows as -2, never as a launch."""
  assert _call(None) == -1
  for store in STORAGES:
    off = dict(q=P + 8)
    assert _call(_descriptor(store, **off)) == -2, store                          # an accepted call, stopped at alignment
    for k in (0, -1, 33):
      assert _call(_descriptor(store, **off), k=k) == -1, (store, k)
    assert _call(_descriptor(store, **off), k=32) == -2 and _call(_descriptor(store, **off), k=1) == -2
    assert _call(_descriptor(store, **off), row0=-1) == -1, store
    assert _call(_descriptor(store, NQ=2, **off), row0=2 ** 31 - 2) == -1, store   # the last row number would not fit an int
    assert _call(_descriptor(store, **off), row0=2 ** 31 - 2) == -2, store
    for name in ('ws', 'state'):
      assert _call(_descriptor(store, **off), **{name: None}) == -1, (store, name)
    for name in ('scores', 'rows', 'mean'):                                       # nullable: still accepted
      assert _call(_descriptor(store, **off), **{name: None}) == -2, (store, name)
    required = ['q', 'qw', 'g', 'gw'] + (['q_lo'] if store != 'fp32' else []) + (['gscale'] if store == 'fp8' else [])
    for field in required:
      assert _call(_descriptor(store, **dict(off, **{field: None}))) == -1, (store, field)
    for field, value in (('NQ', 0), ('NV', 0), ('M', 0), ('M', 17), ('d', 0), ('d', 18), ('NQ', -1), ('NV', -1), ('d', -16),
                         ('storage', 3), ('storage', -1), ('sets', 3), ('sets', -1)):
      assert _call(_descriptor(store, **dict(off, **{field: value}))) == -1, (store, field, value)
    # the descriptor takes no options: each part alone is refused
    for part in (dict(subset=P), dict(exclude=P, E=1), dict(E=1), dict(after=P), dict(lse=P, beta=1.0), dict(lse=P),
                 dict(beta=1.0), dict(sets=1, set_size=1, set_weights=P), dict(sets=2, set_size=1, set_weights=P),
                 dict(set_size=1), dict(mode=1), dict(set_weights=P)):
      assert _call(_descriptor(store, **dict(off, **part))) == -1, (store, part)
    # alignment: each of the five alone 4 or 8 bytes off
    for shift in (4, 8):
      for field in ['q', 'g'] + (['q_lo'] if store != 'fp32' else []):
        assert _call(_descriptor(store, **{field: P + shift})) == -2, (store, field, shift)
      for name in ('ws', 'state'):
        assert _call(_descriptor(store), **{name: P + shift}) == -2, (store, name, shift)
  assert _call(_descriptor('fp32', q_lo=P, q=P + 8)) == -1                         # q_lo with fp32
  for store in ('fp32', 'bf16'):
    assert _call(_descriptor(store, gscale=P, q=P + 8)) == -1, store               # gscale without fp8
  assert _call(_descriptor('fp8', d=8, q=P + 8)) == -1                             # a bf16 width, not an fp8 one
  assert _call(_descriptor('bf16', d=4, q=P + 8)) == -1                            # an fp32 width
  assert _call(_descriptor('bf16', d=8, q=P + 8)) == -2 and _call(_descriptor('fp32', d=4, q=P + 8)) == -2


def test_the_workspace_size():
  from mmt_amd import _lib
  size = _lib.lib().mmt_col_topk_workspace_keys
  assert size(1, 1, 1) == 1 and size(64, 10, 3) == 30 and size(65, 10, 3) == 60
  assert size(4096, 262144, 32) == 64 * 262144 * 32
  for bad in ((0, 5, 1), (5, 0, 1), (-1, 5, 1), (5, -1, 1), (5, 5, 0), (5, 5, -1), (5, 5, 33)):
    assert size(*bad) < 0, bad


def test_argument_errors_are_raised_without_a_device():
  from mmt_amd.search import FP8, HubNorm, ShardedHubNorm, ShardedVideoIndex
  q, qw = torch.zeros(3, 2, 8), torch.zeros(3, 2)
  index = _hollow_index(5)
  for bad in (True, False, 0, -1, 33, 10.0, None, '3', np.int64(3)):
    with pytest.raises(ValueError, match='reverse_search: k must be an int in 1..32'):
      index.reverse_search(q, qw, bad)
    with pytest.raises(ValueError, match='csls_norm: k must be an int in 1..32'):
      index.csls_norm(q, qw, bad)
    with pytest.raises(ValueError, match='k must be an int'):
      ShardedVideoIndex.reverse_search(index, q, qw, k=bad)
  with pytest.raises(ValueError, match='dynamic'):
    index.csls_norm(q, qw, 10, dynamic=1)
  for call in (lambda i: i.reverse_search(q, qw), lambda i: i.csls_norm(q, qw)):
    with pytest.raises(ValueError, match='holds no items'):
      call(_hollow_index(0))
    with pytest.raises(ValueError, match='CUDA tensor'):      # the checks above come before the queries are touched
      call(index)
  # csls_norm on an fp8 index names the dtype, before k is looked at; reverse_search is not refused there
  with pytest.raises(ValueError, match='csls_norm.*float8_e4m3fn'):
    _hollow_index(5, FP8).csls_norm(q, qw, 0)
  with pytest.raises(ValueError, match='reverse_search: k'):
    _hollow_index(5, FP8).reverse_search(q, qw, 0)
  with pytest.raises(ValueError, match='CUDA tensor'):
    _hollow_index(5, FP8).reverse_search(q, qw)
  # the new trailing keyword of the norms: positional construction as before, 'softmax' unless said
  lse = torch.zeros(4)
  norm = HubNorm(lse, 20.0, 7)
  assert (norm.kind, norm.k, norm.hubs, norm.beta, norm.bank_size, norm.num_items) == ('softmax', None, None, 20.0, 7, 4)
  norm = HubNorm(lse, 2.0, 7, None, kind='csls', k=10)
  assert (norm.kind, norm.k, norm.beta) == ('csls', 10, 2.0)
  sharded = ShardedHubNorm([None], lse, 20.0, 7, lse > 0)
  assert (sharded.kind, sharded.k) == ('softmax', None) and sharded.hubs is not None
  assert ShardedHubNorm([None], lse, 2.0, 7, kind='csls', k=3).kind == 'csls'


def test_indexed_metrics_check_bank_norm_before_anything_is_built():
  from mmt_amd.metric import retrieval_metrics_indexed
  args = (torch.zeros(4, 2, 8), torch.zeros(4, 2, 1, 8), torch.zeros(4, 2), torch.zeros(4, 1, 2))
  bank = (torch.zeros(3, 2, 8), torch.zeros(3, 2))
  for bad in ('x', None, 'CSLS', 1):
    with pytest.raises(ValueError, match='bank_norm'):
      retrieval_metrics_indexed(*args, text_bank=bank, beta=20.0, bank_norm=bad)
  for kwargs in ({'text_bank': bank}, {'video_bank': bank}, {}):
    with pytest.raises(ValueError, match="'csls' takes no beta"):
      retrieval_metrics_indexed(*args, bank_norm='csls', beta=20.0, **kwargs)
  with pytest.raises(ValueError, match='needs beta'):           # 'softmax' is as before
    retrieval_metrics_indexed(*args, text_bank=bank, bank_norm='softmax')
  with pytest.raises(ValueError, match='pair'):                 # 'csls' without beta goes on to the next check
    retrieval_metrics_indexed(*args, text_bank=bank[0], bank_norm='csls')
