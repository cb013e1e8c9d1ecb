"""The host side of the softmax over the gallery (VideoIndex.query_lse, search_softmax; mmt_search_row_expsum) without a
GPU: the fixed-point position, the rounding of a term and the float64 closing step on cases worked by hand, on CPU tensors;
the brute-force log-sum-exp the GPU tests hold the kernel to; the header, the ctypes table and the library; every gate of
the new entry; the argument errors that need no device."""
import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

from mmt_amd.search import QueryLse, fixed_terms, lse_bits, lse_from_sums
from tests.test_index_groups_cpu import _hollow_index, _hollow_sharded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float('inf')
OWN = ['beta', 'xmax', 'F', 'ws']   # the entry's own arguments between the descriptor and the stream


def brute_row_lse(scores, beta, allowed=None):
  """The definition of `query_lse` with an exact exponential and an exact sum: scores float32 [NQ, N] (numpy: the device's
  own score bits), beta a float, allowed bool [N] or None -> (lse float64 [NQ], xmax float32 [NQ], d float32 [NQ, n] the
  rounded differences x - xmax of the n allowed columns).  x = fl32(float32(beta) * score) and d = fl32(x - xmax) are
  float32 operations, as in the kernel; exp is float64 and a row's sum is math.fsum, the correctly rounded sum, so the
  result does not depend on the order of the columns."""
  scores = np.asarray(scores, dtype=np.float32)
  if allowed is not None:
    scores = scores[:, np.asarray(allowed, dtype=bool)]
  x = np.float32(beta) * scores
  assert x.dtype == np.float32
  xmax = x.max(axis=1)
  d = x - xmax[:, None]
  assert d.dtype == np.float32
  e = np.exp(d.astype(np.float64))
  total = np.array([math.fsum(row) for row in e])
  return xmax.astype(np.float64) + np.log(total), xmax, d


def test_lse_bits():
  want = {1: 61, 2: 61, 3: 60, 2 ** 18: 44, 2 ** 18 + 1: 43, 2 ** 31 - 1: 31}
  for n, f in want.items():
    assert lse_bits(n) == f, n
    assert n * 2 ** f <= 2 ** 62, n                       # n terms of at most 2^F: no overflow, no saturation
    assert f == 62 - math.ceil(math.log2(max(n, 2)))
  assert 2 * (2 ** 18 + 1) * 2 ** 43 > 2 ** 62            # and F is the largest such position but one bit of headroom
  for bad in (0, -1, 2.0, True, None, 2 ** 62):
    with pytest.raises(ValueError, match='lse_bits: num_items must be an int'):
      lse_bits(bad)


def test_fixed_terms_on_cases_worked_by_hand():
  for bits in (61, 44, 31, 20):
    e = torch.tensor([1.0, 0.0, 2.0 ** -(bits + 2), 2.0 ** -(bits + 1), 3 * 2.0 ** -(bits + 1), 2.0 ** -bits, 0.75],
                     dtype=torch.float32)
    t = fixed_terms(e, bits)
    assert t.dtype == torch.int64
    # 1 -> 2^F; 0 and a value below 2^-(F + 1) -> 0; the ties at one half and at three halves go to even: 0 and 2
    assert t.tolist() == [2 ** bits, 0, 0, 0, 2, 1, 3 * 2 ** (bits - 2)], bits
  # below 2^24 the rounding is to nearest: 5.25 -> 5, 5.5 -> 6 (even), 6.5 -> 6 (even), 6.75 -> 7
  e = torch.tensor([5.25, 5.5, 6.5, 6.75], dtype=torch.float32) * 2.0 ** -20
  assert fixed_terms(e, 20).tolist() == [5, 6, 6, 7]
  assert fixed_terms(torch.rand(3, 4), 31).shape == (3, 4)


def test_lse_from_sums_on_cases_worked_by_hand():
  for n in (1, 2, 3, 50, 300, 2 ** 18):
    bits = lse_bits(max(n, 300))
    xmax = torch.tensor([0.0, 3.25, -17.5, 160.0], dtype=torch.float32)
    lse = lse_from_sums(xmax, torch.full((4,), n << bits, dtype=torch.int64), bits)
    assert lse.dtype == torch.float32
    want = (xmax.double() + math.log(n)).float()          # n equal scores: xmax + log n; a single candidate: xmax
    assert torch.equal(lse, want), n
    if n == 1:
      assert torch.equal(lse, xmax)
  # a half-weight second term: log(1.5) above the maximum
  bits = lse_bits(2)
  got = lse_from_sums(torch.tensor([2.0]), torch.tensor([(1 << bits) + (1 << (bits - 1))]), bits)
  assert got.item() == np.float32(2.0 + math.log(1.5))


def test_the_brute_force_is_the_definition_and_ignores_the_column_order():
  gen = np.random.default_rng(12)
  scores = gen.standard_normal((7, 300)).astype(np.float32) * 0.2
  scores[3] = 0.125                                        # n equal scores
  allowed = gen.random(300) < 0.4
  for mask in (None, allowed):
    lse, xmax, d = brute_row_lse(scores, 20.0, mask)
    n = 300 if mask is None else int(mask.sum())
    assert lse.dtype == np.float64 and xmax.dtype == np.float32 and d.shape == (7, n)
    assert (d <= 0).all() and (d.max(axis=1) == 0).all()
    assert lse[3] == 2.5 + math.log(n)
    x = 20.0 * scores.astype(np.float64)[:, slice(None) if mask is None else mask]
    want = np.log(np.exp(x - x.max(1, keepdims=True)).sum(1)) + x.max(1)
    assert np.abs(lse - want).max() < 1e-5                 # float32 x against float64 x: 2^-24 * |x| per term
    for seed in (1, 2):
      perm = np.random.default_rng(seed).permutation(300)
      again = brute_row_lse(scores[:, perm], 20.0, None if mask is None else mask[perm])
      assert np.array_equal(again[0], lse) and np.array_equal(again[1], xmax)
  one = brute_row_lse(scores, 20.0, np.arange(300) == 17)
  assert np.array_equal(one[0], (np.float32(20.0) * scores[:, 17]).astype(np.float64))   # a single candidate: xmax


def test_the_fixed_point_sum_meets_the_definition_on_the_host():
  """The whole chain on CPU tensors with torch's own exp in the kernel's place: within the quantisation bound plus the
  float32 exp's error, and the integer sum does not move under a permutation -- where a float32 sum does."""
  gen = np.random.default_rng(5)
  scores = gen.standard_normal((9, 4000)).astype(np.float32) * 0.1
  lse, xmax, d = brute_row_lse(scores, 20.0)
  bits = lse_bits(4000)
  terms = fixed_terms(torch.exp(torch.from_numpy(d)), bits)
  sums = terms.sum(1)
  assert (sums >= 1 << bits).all() and (sums <= 4000 << bits).all()
  got = lse_from_sums(torch.from_numpy(xmax), sums, bits).double().numpy()
  assert np.abs(got - lse).max() <= 2.0 ** -22 + 2.0 ** -24 * np.abs(lse).max() + 4000 * 2.0 ** -(bits + 1)
  perm = torch.from_numpy(np.random.default_rng(6).permutation(4000))
  assert torch.equal(terms[:, perm].sum(1), sums)
  assert torch.equal(torch.stack([part.sum(1) for part in terms.split(128, dim=1)]).sum(0), sums)   # any chunking


def _function(name):
  from mmt_amd import _lib
  handle = ctypes.CDLL(_lib.LIB_PATH)
  fn = getattr(handle, name)
  fn.restype, fn.argtypes = _lib.SIGNATURES[name]
  return handle, fn


def test_header_bindings_and_library_agree_on_the_new_entry():
  from mmt_amd import _lib
  src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'mmt_hip.h')).read(), flags=re.S)
  handle, _ = _function('mmt_search_row_expsum')
  params = [p.strip() for p in re.search(r'\bint mmt_search_row_expsum\(([^;]*?)\);', src).group(1).replace('\n', ' ').split(',')]
  res, args = _lib.SIGNATURES['mmt_search_row_expsum']
  assert res is ctypes.c_int and len(args) == len(params) == 6
  assert params[0] == 'const MmtSearchScan* scan' and params[-1] == 'void* stream'
  assert args[0] is ctypes.POINTER(_lib.MmtSearchScan) and args[-1] is ctypes.c_void_p
  assert [p.split()[-1].lstrip('*') for p in params[1:-1]] == OWN
  for p, a in zip(params[1:-1], args[1:-1]):
    assert (a is ctypes.c_void_p) == ('*' in p), p
    assert (a is ctypes.c_float) == p.startswith('float '), p
    assert (a is ctypes.c_int) == p.startswith('int '), p
  assert 'const float* xmax' in params and 'int64_t* ws' in params
  size = re.search(r'\bint64_t mmt_row_expsum_workspace_ints64\(([^;]*?)\);', src).group(1)
  assert [p.strip() for p in size.split(',')] == ['int NQ', 'int NV']
  assert _lib.SIGNATURES['mmt_row_expsum_workspace_ints64'] == (ctypes.c_int64, [ctypes.c_int, ctypes.c_int])
  assert hasattr(handle, 'mmt_search_row_expsum') and hasattr(handle, 'mmt_row_expsum_workspace_ints64')
  assert handle.mmt_abi_version() == 6 and '#define MMT_ABI_VERSION 6' in src
  assert os.path.exists(os.path.join(ROOT, 'mmt_amd', 'csrc', 'search_lse.hip'))


def test_workspace_size():
  _, size = _function('mmt_row_expsum_workspace_ints64')
  assert size(300, 300) == 300 * 3                          # one tile per chunk: three chunks
  assert size(4096, 262144) == 4096 * 64                    # full-size chunks of 4096 columns
  assert size(1, 1) == 1
  for bad in ((0, 5), (5, 0), (-3, 5), (5, -1)):
    assert size(*bad) == -1, bad


def _descriptor(P, store, **changes):
  from mmt_amd import _lib
  storage = store
  f = dict(q=P, q_lo=None if storage == 0 else P, qw=P, g=P, gw=P, gscale=P if storage == 2 else None, subset=None,
           exclude=None, after=None, lse=None, set_weights=None, storage=storage, NQ=3, NV=5, M=2, d=32, E=0, beta=0.0,
           sets=0, set_size=0, mode=0)
  f.update(changes)
  return _lib.MmtSearchScan(**f)


def test_the_new_entry_gates_its_arguments_on_the_host():
  """Every refusal below returns before any launch: MMT_ERR_ARG = -1, MMT_ERR_ALIGN = -2.  The pointers are aligned and
  never dereferenced.  A knock-out of an argument gate is made with the query rows off their boundary as well, so a gate
  that has gone missing shows as -2 (or as a launch), never as a pass."""
  _, fn = _function('mmt_search_row_expsum')
  buf = (ctypes.c_char * 256)()
  P = ctypes.addressof(buf) + -ctypes.addressof(buf) % 16
  good = dict(beta=20.0, xmax=P, F=53, ws=P)

  def call(desc, **own):
    return fn(None if desc is None else ctypes.byref(desc), *[dict(good, **own)[n] for n in OWN], None)
  assert call(None) == -1
  for storage, mult in ((0, 4), (1, 8), (2, 16)):
    def arg(own=None, **fields):
      return call(_descriptor(P, storage, **dict(dict(q=P + 8), **fields)), **(own or {}))
    # everything in order, with and without a subset: only the alignment is refused
    for field in ['q', 'g'] + (['q_lo'] if storage else []):
      for off in (4, 8):
        assert call(_descriptor(P, storage, **{field: P + off})) == -2, (storage, field)
        assert call(_descriptor(P, storage, subset=P, **{field: P + off})) == -2, (storage, field)
    assert call(_descriptor(P, storage, subset=P + 4)) == -2 and call(_descriptor(P, storage, subset=P + 8)) == -2
    for f in (0, 31, 61, 62):
      assert arg(dict(F=f)) == -2, (storage, f)
    # each part of the descriptor the entry does not take, alone and beside a subset
    parts = [dict(exclude=P, E=1), dict(E=1), dict(exclude=P), dict(after=P), dict(lse=P, beta=1.0), dict(lse=P),
             dict(beta=1.0), dict(sets=1, set_size=1, set_weights=P), dict(sets=2, set_size=1, set_weights=P),
             dict(set_weights=P), dict(set_size=1), dict(mode=1), dict(sets=3), dict(sets=-1), dict(storage=3),
             dict(storage=-1)]
    for part in parts:
      assert arg(**part) == -1, (storage, part)
      assert arg(subset=P, **part) == -1, (storage, part)
    # the entry's own arguments
    for own in (dict(xmax=None), dict(ws=None), dict(F=-1), dict(F=63), dict(beta=0.0), dict(beta=-1.0), dict(beta=INF),
                dict(beta=float('nan'))):
      assert arg(own) == -1, (storage, own)
    # operands and shapes
    required = ['q', 'qw', 'g', 'gw'] + (['q_lo'] if storage else []) + (['gscale'] if storage == 2 else [])
    for field in required:
      assert call(_descriptor(P, storage, **{field: None, 'g' if field == 'q' else 'q': P + 8})) == -1, (storage, field)
    for field, value in (('NQ', 0), ('NQ', -1), ('NV', 0), ('NV', -1), ('M', 0), ('M', 17), ('d', 0), ('d', -16),
                         ('d', 32 + mult // 2)):
      assert arg(**{field: value}) == -1, (storage, field, value)
    if storage == 0:
      assert arg(q_lo=P) == -1
    if storage != 2:
      assert arg(gscale=P) == -1
  assert call(_descriptor(P, 1, d=4, q=P + 8)) == -1           # an fp32 width on a bf16 index
  assert call(_descriptor(P, 2, d=8, q=P + 8)) == -1           # a bf16 width on an fp8 index


@pytest.mark.parametrize('hollow', [_hollow_index, _hollow_sharded], ids=['VideoIndex', 'ShardedVideoIndex'])
def test_argument_errors_are_raised_without_a_device(hollow):
  from mmt_amd import search
  from mmt_amd.search import ShardedVideoIndex, VideoIndex
  q, qw = torch.zeros(3, 2, 8), torch.zeros(3, 2)
  index = hollow(5)
  calls = {'query_lse': lambda beta=20.0, **kw: index.query_lse(q, qw, beta, **kw),
           'search_softmax': lambda beta=20.0, **kw: index.search_softmax(q, qw, beta=beta, **kw)}
  for name, call in calls.items():
    for option in ('exclude', 'norm', 'pooling', 'item_pooling', 'after', 'grouping'):
      with pytest.raises(ValueError, match='%s: %s= is out of scope' % (name, option)):
        call(**{option: None})
    with pytest.raises(TypeError, match='unexpected keyword'):
      call(betta=3.0)
    for bad in (0.0, -1.0, INF, float('nan'), 20, True, None, '20', torch.tensor(20.0)):
      with pytest.raises(ValueError, match=name + ': beta must be a float with 0 < beta < inf'):
        call(bad)
    with pytest.raises(ValueError, match=name + ': subset must come from'):
      call(subset=torch.zeros(3, dtype=torch.int64))
    with pytest.raises(ValueError, match=name + ': the index holds no items'):
      getattr(hollow(0), name)(q, qw, beta=20.0)
    with pytest.raises(ValueError, match='must be a CUDA tensor'):
      call()                                                   # host queries: the last check before the device
  for bad in (0, 129, -1, 2.0, True, None):
    with pytest.raises(ValueError, match=r'search_softmax: k must be an int in 1\.\.128'):
      index.search_softmax(q, qw, k=bad, beta=20.0)
  with pytest.raises(ValueError, match='search_softmax: beta must be a float'):
    index.search_softmax(q, qw)                                # beta has no default worth having
  for method in ('query_lse', 'search_softmax'):
    assert getattr(ShardedVideoIndex, method) is getattr(VideoIndex, method)
  assert list(inspect.signature(VideoIndex.query_lse).parameters) == ['self', 'embds', 'weights', 'beta', 'subset', 'unsupported']
  assert list(inspect.signature(VideoIndex.search_softmax).parameters) == [
      'self', 'embds', 'weights', 'k', 'beta', 'subset', 'unsupported']
  assert inspect.signature(VideoIndex.search_softmax).parameters['k'].default == 10
  assert 'the twelfth question' in search.__doc__.lower()


def test_query_lse_puts_scores_on_the_softmax_scale():
  """QueryLse.log_prob / prob on CPU tensors: plain torch ops, a rounded multiply then a rounded subtract."""
  lse = torch.tensor([1.5, -2.0], dtype=torch.float32)
  ql = QueryLse(lse, 20.0, torch.tensor([0.05, -0.125]), torch.tensor([4, 0]), torch.tensor([3, 5]), 60, 5, 5)
  assert (ql.bits, ql.num_items, ql.count, ql.beta, ql.device) == (60, 5, 5, 20.0, lse.device)
  scores = torch.tensor([[0.05, 0.0123, -INF], [-0.125, -0.3, 0.01]], dtype=torch.float32)
  lp = ql.log_prob(scores)
  want = (np.float32(20.0) * scores.numpy()) - lse.numpy()[:, None]
  assert lp.dtype == torch.float32 and np.array_equal(lp.numpy().view(np.int32), want.astype(np.float32).view(np.int32))
  assert lp[0, 2] == -INF and ql.prob(scores)[0, 2] == 0
  assert torch.equal(ql.prob(scores), torch.exp(lp))
  assert ql.log_prob(scores[:, 0]).shape == (2,) and ql.log_prob(scores.reshape(2, 3, 1)).shape == (2, 3, 1)
  for bad in (scores.double(), scores[:1], [0.5], torch.tensor(0.5)):
    with pytest.raises(ValueError, match='log_prob: scores'):
      ql.log_prob(bad)


def test_info_nce_indexed_refuses_what_it_does_not_support():
  from mmt_amd import metric
  v, t, vw, tw = torch.zeros(4, 2, 16), torch.zeros(4, 2, 1, 16), torch.zeros(4, 2), torch.zeros(4, 1, 2)
  with pytest.raises(ValueError, match='info_nce_indexed: torch.float8_e4m3fn is not supported'):
    metric.info_nce_indexed(v, t, vw, tw, dtype=torch.float8_e4m3fn)
  with pytest.raises(ValueError, match='info_nce_indexed: dtype must be'):
    metric.info_nce_indexed(v, t, vw, tw, dtype=torch.float16)
  for bad in (0.0, -1.0, INF, 1, None):
    with pytest.raises(ValueError, match='info_nce_indexed: scale must be a float'):
      metric.info_nce_indexed(v, t, vw, tw, scale=bad)
  with pytest.raises(ValueError, match='one caption per video'):
    metric.info_nce_indexed(v, torch.zeros(4, 2, 3, 16), vw, torch.zeros(4, 3, 2))
  assert list(inspect.signature(metric.info_nce_indexed).parameters) == [
      'vid_embds', 'text_embds', 'vid_weights', 'text_weights', 'scale', 'dtype']
