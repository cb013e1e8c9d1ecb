"""The per-expert score breakdown (mmt_search_expert_parts; expert_scores, search_explained, pair_expert_scores) without a
GPU: the header, the ctypes table and the exported symbol; every host gate of the entry, one knocked out at a time; the
argument errors of the three calls; and the fp64 definition of tests/expert_parts_ref.py against the reference's own
similarity matrix of the golden fixture."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests.expert_parts_ref import U, expert_parts_ref, fold
from tests.test_index_groups_cpu import _hollow_index, _hollow_sharded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = 'mmt_search_expert_parts'
PARAMS = ['qf', 'qw', 'g', 'gw', 'gscale', 'storage', 'NV', 'M', 'd', 'candidates', 'R', 'C', 'parts', 'mix', 'stream']
STORAGES = {'fp32': (0, 4), 'bf16': (1, 8), 'fp8': (2, 16)}   # tag, the multiple d must be

_buf = (ctypes.c_char * 256)()
P = ctypes.addressof(_buf) + -ctypes.addressof(_buf) % 16     # 16-byte aligned, never dereferenced: every call is refused


def _call(store, **changes):
  """A call every gate accepts -- R = NV = M = C = 1, d = 16 (a multiple for every storage) -- with `changes`."""
  from mmt_amd import _lib
  args = dict(qf=P, qw=P, g=P, gw=P, gscale=P if store == 'fp8' else None, storage=STORAGES[store][0], NV=1, M=1, d=16,
              candidates=P, R=1, C=1, parts=P, mix=P, stream=None)
  args.update(changes)
  return _lib.lib().mmt_search_expert_parts(*(args[name] for name in PARAMS))


def test_header_bindings_and_symbol_agree():
  from mmt_amd import _lib
  src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'mmt_hip.h')).read(), flags=re.S)
  m = re.search(r'\bint %s\(([^;]*?)\);' % NAME, src)
  assert m, NAME + ' is not declared in mmt_hip.h'
  params = [p.strip() for p in m.group(1).replace('\n', ' ').split(',')]
  assert [p.split()[-1].lstrip('*') for p in params] == PARAMS
  res, args = _lib.SIGNATURES[NAME]
  assert res is ctypes.c_int and len(args) == len(params) == 15
  for p, a in zip(params, args):
    assert (a is ctypes.c_void_p) == ('*' in p) and (a is ctypes.c_int) == p.startswith('int '), p
  assert params[0] == 'const float* qf' and params[2] == 'const void* g' and params[9] == 'const int64_t* candidates'
  assert int(re.search(r'#define MMT_SEARCH_MAX_C (\d+)', src).group(1)) == 1024
  handle = ctypes.CDLL(_lib.LIB_PATH)
  assert hasattr(handle, NAME)
  assert handle.mmt_abi_version() == 6                         # additive: the ABI version stays


@pytest.mark.parametrize('store', list(STORAGES))
def test_every_gate_of_the_entry(store):
  """One thing knocked out of a good call at a time.  A knock-out that returns MMT_ERR_ARG (-1) is made with qf misaligned as
  well, so a gate that has gone missing shows as MMT_ERR_ALIGN (-2), never as a launch; -2 itself is returned only for an
  otherwise good call."""
  mult = STORAGES[store][1]

  def arg(**changes):
    return _call(store, **dict(dict(qf=P + 8), **changes))
  assert arg() == -2                                           # the good call, misaligned: every gate before it passed
  for name in ('qf', 'qw', 'g', 'gw', 'candidates', 'parts', 'mix'):
    assert arg(**{name: None}) == -1, name
  for tag in (3, -1, 7):
    assert arg(storage=tag) == -1, tag
  assert arg(gscale=None if store == 'fp8' else P) == -1       # missing on fp8, given on the other two: never ignored
  for m in (0, -1, 17):
    assert arg(M=m) == -1, m
  assert arg(M=16) == -2
  for d in (0, -16, 16 + mult // 2, mult // 2):
    assert arg(d=d) == -1, d
  assert arg(d=mult) == -2 and arg(d=3 * mult) == -2
  if store == 'fp8':
    assert arg(d=8) == -1                                      # a bf16 width, not an fp8 one
  if store == 'bf16':
    assert arg(d=4) == -1                                      # an fp32 width
  for field in ('NV', 'R'):
    for bad in (0, -1):
      assert arg(**{field: bad}) == -1, (field, bad)
  for c in (0, -1, 1025):
    assert arg(C=c) == -1, c
  assert arg(C=1024) == -2
  # a grid that would overflow: one block per row and 64 candidates of it
  assert arg(R=2 ** 27, C=1024) == -1 and arg(R=2 ** 31 - 1, C=65) == -1
  assert arg(R=2 ** 27 - 1, C=1024) == -2 and arg(R=2 ** 31 - 1, C=64) == -2
  # alignment: the gates passed, qf or g alone 4 or 8 bytes off
  for field in ('qf', 'g'):
    for off in (4, 8):
      assert _call(store, **{field: P + off}) == -2, (field, off)


@pytest.mark.parametrize('hollow', [_hollow_index, _hollow_sharded], ids=['VideoIndex', 'ShardedVideoIndex'])
def test_argument_errors_are_raised_without_a_device(hollow):
  from mmt_amd.search import ExpertScores, ShardedVideoIndex, VideoIndex
  q, qw = torch.zeros(3, 2, 8), torch.zeros(3, 2)
  cand, items = torch.zeros(3, 4, dtype=torch.int64), torch.zeros(3, dtype=torch.int64)
  calls = {'expert_scores': lambda index, c: index.expert_scores(q, qw, c),
           'pair_expert_scores': lambda index, c: index.pair_expert_scores(items, c)}
  for who, call in calls.items():
    index = hollow(5)
    for bad in ([[0, 1]], np.zeros((3, 4), np.int64), None, cand.to(torch.int32), cand.double(), cand > 0):
      with pytest.raises(ValueError, match='%s: candidates must be an int64 tensor' % who):
        call(index, bad)
    with pytest.raises(ValueError, match='%s: candidates must be on the index device' % who):
      call(index, cand)                                          # host candidates for a device index
    index.device = torch.device('cpu')                           # lets the later checks be reached with host tensors
    for bad in (cand[:, 0], cand.reshape(3, 2, 2), torch.zeros(3, 0, dtype=torch.int64),
                torch.zeros(3, 1025, dtype=torch.int64), torch.tensor(3)):
      with pytest.raises(ValueError, match=r'%s: candidates \[NQ, 1 <= C <= 1024\] expected' % who):
        call(index, bad)
    empty = hollow(0)
    empty.device = torch.device('cpu')
    with pytest.raises(ValueError, match='%s: the index holds no items' % who):
      call(empty, cand)
  index = hollow(5)
  index.device = torch.device('cpu')
  with pytest.raises(ValueError, match='CUDA tensor'):
    index.expert_scores(q, qw, cand)                             # the queries themselves are host tensors
  for bad in ([0, 1, 2], None, items.to(torch.int32), items.double()):
    with pytest.raises(ValueError, match='pair_expert_scores: items must be an int64 tensor'):
      index.pair_expert_scores(bad, cand)
  with pytest.raises(ValueError, match=r'pair_expert_scores: items \[R\] expected'):
    index.pair_expert_scores(cand, cand)
  with pytest.raises(ValueError, match='pair_expert_scores: 2 items but candidates'):
    index.pair_expert_scores(items[:2], cand)
  for lo in (torch.tensor([0, -1, 4]), torch.tensor([0, 5, 4])):
    with pytest.raises(ValueError, match=r'pair_expert_scores: items must lie in 0 \.\. 4'):
      index.pair_expert_scores(lo, cand)
  for bad in (-2, 5):
    with pytest.raises(ValueError, match=r'pair_expert_scores: candidates must lie in -1 \.\. 4'):
      index.pair_expert_scores(items, torch.full((3, 4), bad, dtype=torch.int64))
  es = index.pair_expert_scores(items[:0], cand[:0])             # no rows: empty results, nothing is launched
  assert isinstance(es, ExpertScores) and es.parts.shape == es.mix.shape == es.expert_sims.shape == (0, 4, 2)
  assert es.parts.dtype is es.mix.dtype is torch.float32
  # search_explained: the options that are out of scope by name, before anything is searched
  for name in ('norm', 'dynamic', 'pooling', 'item_pooling'):
    with pytest.raises(ValueError, match='search_explained: %s= is out of scope' % name):
      index.search_explained(q, qw, **{name: None})
  with pytest.raises(TypeError, match="unexpected keyword argument 'grouping'"):
    index.search_explained(q, qw, grouping=None)
  for extra in ('norm', 'pooling', 'subset', 'k'):
    with pytest.raises(TypeError):
      index.expert_scores(q, qw, cand, **{extra: None})
  for method in ('expert_scores', 'search_explained', 'pair_expert_scores'):
    assert getattr(ShardedVideoIndex, method) is getattr(VideoIndex, method)   # one surface, on _Index
  assert list(inspect.signature(VideoIndex.expert_scores).parameters) == ['self', 'embds', 'weights', 'candidates']
  assert list(inspect.signature(VideoIndex.pair_expert_scores).parameters) == ['self', 'items', 'candidates']
  assert list(inspect.signature(VideoIndex.search_explained).parameters) == [
      'self', 'embds', 'weights', 'k', 'subset', 'exclude', 'after', 'where', 'unsupported']
  assert inspect.signature(VideoIndex.search_explained).parameters['k'].default == 10


def test_the_parts_sum_to_the_reference_similarity_of_the_golden_fixture():
  """The text layout of tests/golden/sim_loss_metric.npz: 15 captions x 5 videos, M = 3, d = 16, one video whose weights are
  all 0.  sum_m part_m (fp64, on the fp32 folds) against the reference's own sims_indep: both are fp32-input evaluations
  of one quantity, the reference's in fp32 -- M d products and sums, two M-term weight sums, a division and a few
  roundings of the weights' normalisation -- so within (M d + 2 M + 8) * 2^-24 * sum_m <|qf_m|, |f_m|> / |den|."""
  g = np.load(os.path.join(ROOT, 'tests', 'golden', 'sim_loss_metric.npz'))
  vid, txt, vw, tw = (g[k] for k in ('sim_in_vid', 'sim_in_txt', 'sim_in_vw', 'sim_in_tw'))
  b, m, c, d = txt.shape
  assert (b, m, c, d) == (5, 3, 3, 16) and vid.shape == (5, m, d) and g['sims_indep'].shape == (b * c, 5)
  q, qw = txt.transpose(0, 2, 1, 3).reshape(b * c, m, d), tw.reshape(b * c, m)      # rows b * C + c
  cand = np.tile(np.arange(5), (b * c, 1))
  parts, mix, bound = expert_parts_ref(fold(q, qw), qw, fold(vid, vw), vw, cand, m, d)
  assert parts.shape == mix.shape == bound.shape == (15, 5, 3) and np.isfinite(parts).all()
  tol = (m * d + 2 * m + 8) * U * bound.sum(-1) / ((d + m + 4) * U)               # the bound's own <|qf|, |f|> / |den|
  err = np.abs(parts.sum(-1) - g['sims_indep'].astype(np.float64))
  assert (err <= tol).all(), (err / np.maximum(tol, 1e-300)).max()
  zero = (vw == 0).all(1)
  assert zero.sum() == 1                                          # 15 pairs with den = 0 -> 1e-5
  assert (parts[:, zero] == 0).all() and (mix[:, zero] == 0).all() and (g['sims_indep'][:, zero] == 0).all()
  live = ~zero
  assert np.abs(mix[:, live].sum(-1) - 1).max() < 1e-12           # the gate's shares sum to 1
  none = expert_parts_ref(fold(q, qw), qw, fold(vid, vw), vw, np.full((15, 2), -1), m, d)
  assert all(np.isnan(t).all() for t in none)


@pytest.mark.parametrize('m', [1, 7, 16])
@pytest.mark.parametrize('d', [4, 64, 512, 2048])
def test_the_bound_holds_for_a_sequential_fp32_evaluation(m, d):
  """What the bound is deduced for, shown once on the CPU: the definition evaluated in fp32 -- sequential sums without fma,
  numpy's cumulative sum -- stays within it."""
  rng = np.random.default_rng(100 * m + d)
  q, g = rng.standard_normal((4, m, d)).astype(np.float32), rng.standard_normal((6, m, d)).astype(np.float32)
  qw, gw = rng.random((4, m)).astype(np.float32), rng.random((6, m)).astype(np.float32)
  gw[2] = 0
  qf, f, cand = fold(q, qw), fold(g, gw), np.tile(np.arange(6), (4, 1))
  parts, mix, bound = expert_parts_ref(qf, qw, f, gw, cand, m, d)
  prod = qf.reshape(4, 1, m, d) * f.reshape(1, 6, m, d)
  dots = np.cumsum(prod, -1, dtype=np.float32)[..., -1]
  gate = (qw[:, None, :] * gw[None]).astype(np.float32)
  den = np.cumsum(gate, -1, dtype=np.float32)[..., -1:]
  den = np.where(den == 0, np.float32(1e-5), den)
  assert (np.abs((dots / den).astype(np.float64) - parts) <= bound).all()
  assert (np.abs((gate / den).astype(np.float64) - mix) <= (m + 3) * U).all()
