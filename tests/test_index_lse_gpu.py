"""The softmax over the gallery on the GPU: VideoIndex.query_lse and search_softmax (mmt_search_row_expsum), on all three
storage dtypes and both index classes, and metric.info_nce_indexed.  Two kinds of claim.  Bit identity, compared with
torch.equal on the integers and on the int32 views of the floats: the sums and the lse do not depend on the run, the row
batching, the order of the items, the shard or whether the candidates are a subset of a larger index.  And the definition:
every pair's score bits are read back from the device (`target_scores` with all 300 items as targets), fed to
tests.test_index_lse_cpu.brute_row_lse in float64, and the lse is held to it within the bound `_bound` derives (DESIGN
9.19), with no violation.  Gallery A is that of test_index_self_gpu: M = 3, d = 64, 300 items = three 128-column tiles,
the last with 44 live columns, one tile per chunk, so the chunk reduction runs; rows 100 .. 139 and 250 .. 259 are exact
copies of row 100 and item 7 has all-zero weights.  beta = 20; the queries are scaled so that beta * score spreads over a
few units -- a softmax with many live terms, not one."""
import math

import numpy as np
import pytest
import torch

from tests.test_index_diverse_gpu import DEV, DTYPES, FP8, IDS, M, D, NV, _bits, _data, _index, _sharded
from tests.test_index_lse_cpu import brute_row_lse

pytestmark = pytest.mark.gpu
INF = float('inf')
BETA = 20.0
NQS = [1, 65, 130]   # 65: one live row in the second row block; 130: three row blocks
BITS = 53            # 62 - ceil(log2(300))
# the compiled expf (the build's flags): v_exp_f32(fl(d * fl32(log2 e))), and for d below about -87.3 the same at d + 64
# times a constant.  Relative error of a term, first order: the rounded product moves the exponent by 2^-24 |d log2 e|, the
# constant fl32(log2 e) is 2^-26.2 off, both times ln 2 -> (2^-24 + 2^-26) |d|; v_exp_f32 itself is good to one ulp
# (the CDNA ISA's statement), 2^-23 relative.
C1, C2 = 2.0 ** -24 + 2.0 ** -26, 2.0 ** -23
_cache = {}


def _queries():
  """130 queries (M = 3, d = 64) scaled by 1 / 64, so that 20 * score has a standard deviation of a few units; row 5 is
  all zero: every score 0, the sum is exactly 300 * 2^F."""
  if 'q' not in _cache:
    gen = torch.Generator(device=DEV).manual_seed(1220)
    q = torch.randn(NQS[-1], M, D, device=DEV, generator=gen) / 64
    qw = torch.rand(NQS[-1], M, device=DEV, generator=gen)
    q[5] = 0
    _cache['q'] = q, qw
  return _cache['q']


def _lse(dtype):
  """index.query_lse of all 130 queries, once per dtype."""
  if ('lse', dtype) not in _cache:
    _cache['lse', dtype] = _index(dtype).query_lse(*_queries(), BETA)
  return _cache['lse', dtype]


def _scores(dtype):
  """Every pair's score bits, from the device itself: float32 numpy [130, 300]."""
  if ('scores', dtype) not in _cache:
    q, qw = _queries()
    targets = torch.arange(NV, device=DEV).expand(q.shape[0], NV).contiguous()
    _cache['scores', dtype] = _index(dtype).target_scores(q, qw, targets).cpu().numpy()
  return _cache['scores', dtype]


def _bound(lse, xmax, d, num_items, bits):
  """The derived bound on |lse - brute lse| per row: lse float64 [NQ], xmax float32 [NQ] and d float32
  [NQ, n] from brute_row_lse.  Four terms.  (1) the compiled expf: term g is off by at most (C1 |d_g| + C2) relative
  (below d = -87 the term is under 2^-125 and is charged whole), so the sum by the e-weighted mean of that.  (2) the
  rounding of a term to an integer: half a unit each, num_items * 2^-(bits + 1) relative to a sum of at least 2^bits.
  Both move log T by -log1p(-r).  (3) the final rounding to float32, 2^-24 of the value.  (4) float64 log and the two
  float64 adds on values below 128: 2^-45 covers an ulp of each."""
  d = d.astype(np.float64)
  e = np.exp(d)
  rel = np.where(d >= -87.0, C1 * np.abs(d) + C2, 1.0)
  r = (e * rel).sum(1) / e.sum(1) + num_items * 2.0 ** -(bits + 1)
  moved = -np.log1p(-r) + 2.0 ** -45
  return moved + 2.0 ** -24 * (np.abs(lse) + moved)


def _same(a, b):
  assert a.dtype == b.dtype and tuple(a.shape) == tuple(b.shape), (a.dtype, b.dtype, a.shape, b.shape)
  assert torch.equal(_bits(a.cpu()), _bits(b.cpu()))


def _same_lse(got, want, rows=slice(None), items=True):
  _same(got.sums, want.sums[rows])
  _same(got.lse, want.lse[rows])
  _same(got.top_scores, want.top_scores[rows])
  if items:
    _same(got.top_items, want.top_items[rows])


@pytest.mark.parametrize('nq', NQS)
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_top1_fields_and_independence_of_run_and_batching(dtype, nq, monkeypatch):
  from mmt_amd import search
  index, (q, qw) = _index(dtype), _queries()
  got = index.query_lse(q[:nq], qw[:nq], BETA)
  assert (got.bits, got.num_items, got.count, got.beta, got.device) == (BITS, NV, NV, BETA, DEV)
  assert got.bits == search.lse_bits(NV)
  for t, kind in ((got.lse, torch.float32), (got.sums, torch.int64), (got.top_scores, torch.float32), (got.top_items, torch.int64)):
    assert t.dtype is kind and t.shape == (nq,) and t.device == DEV
  scores, indices = index.search(q[:nq], qw[:nq], k=1)
  _same(got.top_scores, scores[:, 0])
  _same(got.top_items, indices[:, 0])
  assert (got.sums >= 1 << BITS).all() and (got.sums <= NV << BITS).all()     # the top-1 term is 2^F; no term is more
  _same_lse(index.query_lse(q[:nq], qw[:nq], BETA), got)                      # a second run
  _same_lse(got, _lse(dtype), slice(0, nq))                                   # a row does not see the other rows
  _same(got.lse, search.lse_from_sums(got.top_scores * BETA, got.sums, BITS))
  monkeypatch.setattr(search, '_BATCH_BYTES', 1)                              # one 64-row block per batch
  _same_lse(index.query_lse(q[:nq], qw[:nq], BETA), got)
  if nq > 5:
    assert got.sums[5] == NV << BITS and got.top_scores[5] == 0               # the all-zero query: 300 equal terms
    assert got.lse[5].item() == np.float32(math.log(NV))


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_the_order_of_the_items_and_the_shards_change_no_bit(dtype):
  from mmt_amd.search import VideoIndex
  (g, gw, _, _), (q, qw), want = _data(), _queries(), _lse(dtype)
  flipped = VideoIndex(g.flip(0).contiguous(), gw.flip(0).contiguous(), dtype=dtype).query_lse(q, qw, BETA)
  _same_lse(flipped, want, items=False)                                       # ties: the copies' numbers differ
  assert torch.equal(_bits(flipped.top_scores), _bits(want.top_scores))
  sharded = _sharded(dtype)
  got = sharded.query_lse(q, qw, BETA)
  assert (got.bits, got.num_items, got.count, got.device) == (BITS, NV, NV, DEV)
  _same_lse(got, want)
  _same_lse(sharded.query_lse(q[:65], qw[:65], BETA), want, slice(0, 65))


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_a_subset_is_the_index_of_its_items(dtype):
  """The integer sum of a subset is that of an index holding the allowed items alone.  F comes from the WHOLE index's item
  count, so the public call on the smaller index is bit-equal where the two counts give one F (the 280-item subset, ragged
  in every tile: 9 bits both); for the 48-item subset with an empty tile (6 bits against 9) the smaller index is asked for
  its sums at the larger one's F, the call a shard gets, and everything else of the result follows from the sums."""
  from mmt_amd.search import VideoIndex, _Scan, lse_bits, lse_from_sums
  (g, gw, _, _), (q, qw), index = _data(), _queries(), _index(dtype)
  wide = torch.ones(NV, dtype=torch.bool)
  wide[3::15] = False                           # 280 allowed: every tile ragged, none empty
  assert int(wide.sum()) == 280 and lse_bits(280) == BITS
  narrow = torch.zeros(NV, dtype=torch.bool)
  narrow[0:128:3] = True                        # a ragged tile; tile 1 (128 .. 255) is empty and skipped
  narrow[[256, 257, 259, 298, 299]] = True      # and a few of the last tile's 44, copies among them
  for allowed in (wide, narrow):
    n = int(allowed.sum())
    for nq in (65, 130):
      got = index.query_lse(q[:nq], qw[:nq], BETA, subset=index.subset(allowed.to(DEV)))
      assert (got.count, got.num_items, got.bits) == (n, NV, BITS)
      scores, indices = index.search(q[:nq], qw[:nq], k=1, subset=index.subset(allowed.to(DEV)))
      _same(got.top_scores, scores[:, 0])
      _same(got.top_items, indices[:, 0])
      alone = VideoIndex(g[allowed.to(DEV)], gw[allowed.to(DEV)], dtype=dtype)
      if lse_bits(n) == BITS:
        _same_lse(alone.query_lse(q[:nq], qw[:nq], BETA), got, items=False)
      top = alone.search(q[:nq], qw[:nq], k=1)[0][:, 0]
      _same(top, got.top_scores)
      sums = alone._row_expsum(q[:nq], qw[:nq], BETA, top * BETA, BITS, _Scan())
      _same(sums, got.sums)
      _same(lse_from_sums(top * BETA, sums, BITS), got.lse)
    # and on the sharded index, whose shards each hold a part of the subset
    sharded = _sharded(dtype)
    _same_lse(sharded.query_lse(q, qw, BETA, subset=sharded.subset(allowed.to(DEV))),
              index.query_lse(q, qw, BETA, subset=index.subset(allowed.to(DEV))))


@pytest.mark.parametrize('n', [1, 50, 300])
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_a_gallery_of_copies_sums_to_n_terms_of_one(dtype, n):
  from mmt_amd.search import VideoIndex, lse_bits
  (g, gw, _, _), (q, qw) = _data(), _queries()
  got = VideoIndex(g[100:101].expand(n, M, D).contiguous(), gw[100:101].expand(n, M).contiguous(), dtype=dtype).query_lse(
      q[:65], qw[:65], BETA)
  bits = lse_bits(n)
  assert got.bits == bits and (got.sums == n << bits).all()
  xmax = (got.top_scores * BETA).double()
  _same(got.lse, (xmax + math.log(n)).float())
  assert (got.top_items == 0).all()


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_a_small_index_works(dtype):
  """5 items, M = 1, d = 16: K is shorter than one slab (the fp8 minimum width)."""
  from mmt_amd.search import VideoIndex, lse_bits
  gen = torch.Generator(device=DEV).manual_seed(5)
  g, gw = torch.randn(5, 1, 16, device=DEV, generator=gen), torch.rand(5, 1, device=DEV, generator=gen)
  q, qw = torch.randn(3, 1, 16, device=DEV, generator=gen) / 16, torch.rand(3, 1, device=DEV, generator=gen)
  index = VideoIndex(g, gw, dtype=dtype)
  got = index.query_lse(q, qw, BETA)
  assert got.bits == lse_bits(5) == 59 and got.count == 5
  scores = index.target_scores(q, qw, torch.arange(5, device=DEV).expand(3, 5).contiguous())
  want, xmax, d = brute_row_lse(scores.cpu().numpy(), BETA)
  assert np.array_equal(xmax, (got.top_scores * BETA).cpu().numpy())
  err = np.abs(got.lse.cpu().double().numpy() - want)
  assert (err <= _bound(want, xmax, d, 5, 59)).all(), err
  p = got.prob(scores).double().sum(1).cpu().numpy()
  assert np.abs(p - 1).max() <= 5 * _bound(want, xmax, d, 5, 59).max()


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_search_softmax_is_search_with_the_log_probabilities(dtype):
  index, (q, qw), lse = _index(dtype), _queries(), _lse(dtype)
  for k in (1, 10, 128):
    scores, indices, log_probs = index.search_softmax(q, qw, k=k, beta=BETA)
    want = index.search(q, qw, k=k)
    _same(scores, want[0])
    _same(indices, want[1])
    _same(log_probs, lse.log_prob(want[0]))
    assert log_probs.shape == (q.shape[0], k) and (log_probs <= 2.0 ** -20).all()
  allowed = torch.zeros(NV, dtype=torch.bool)
  allowed[0:128:3] = True
  allowed[[256, 257, 259, 298, 299]] = True
  subset = index.subset(allowed.to(DEV))
  scores, indices, log_probs = index.search_softmax(q, qw, k=128, beta=BETA, subset=subset)
  want = index.search(q, qw, k=128, subset=subset)
  assert scores.shape == (q.shape[0], 48)
  _same(scores, want[0])
  _same(indices, want[1])
  _same(log_probs, index.query_lse(q, qw, BETA, subset=subset).log_prob(want[0]))
  sharded = _sharded(dtype)
  for a, b in zip(sharded.search_softmax(q, qw, k=10, beta=BETA), index.search_softmax(q, qw, k=10, beta=BETA)):
    _same(a, b)


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_lse_is_the_definition_on_the_devices_own_scores(dtype):
  """Against brute_row_lse in float64 on the score bits the device itself gives every pair, within `_bound`, with no
  violation; and the probabilities of a row's 300 items sum to 1 within 300 times that bound."""
  scores, got = _scores(dtype), _lse(dtype)
  want, xmax, d = brute_row_lse(scores, BETA)
  assert np.array_equal(xmax.view(np.int32), (got.top_scores * BETA).cpu().numpy().view(np.int32))
  tol = _bound(want, xmax, d, NV, BITS)
  err = np.abs(got.lse.cpu().double().numpy() - want)
  live = (np.exp(d.astype(np.float64)) > 2.0 ** -24).sum(1)
  print('%s: max |lse error| %.3g, max error / bound %.3g over %d rows; terms above 2^-24 per row: median %d, max %d' % (
      dtype, err.max(), (err / tol).max(), err.size, np.median(live), live.max()))
  assert (err <= tol).all(), (err / tol).max()
  p = got.prob(torch.from_numpy(scores).to(DEV))
  assert p.shape == (scores.shape[0], NV) and (p >= 0).all() and (p <= 1 + 2.0 ** -20).all()
  off = np.abs(p.double().sum(1).cpu().numpy() - 1)
  print('%s: max |sum of probabilities - 1| %.3g, against 300 x bound %.3g' % (dtype, off.max(), (off / (NV * tol)).max()))
  assert (off <= NV * tol).all()
  # the subset's definition: the same scores, the allowed columns only
  allowed = torch.rand(NV, generator=torch.Generator().manual_seed(3)) < 0.4
  index, (q, qw) = _index(dtype), _queries()
  sub = index.query_lse(q, qw, BETA, subset=index.subset(allowed.to(DEV)))
  want, xmax, d = brute_row_lse(scores, BETA, allowed.numpy())
  err = np.abs(sub.lse.cpu().double().numpy() - want)
  assert (err <= _bound(want, xmax, d, NV, BITS)).all()


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
def test_info_nce_indexed_is_the_cross_entropy_of_the_matrix(dtype):
  """300 pairs, one caption per video, against torch.nn.functional.cross_entropy in float64 on scale * sims in both
  directions: fp32 on metric.eval_similarity's matrix, bf16 on the bf16 index's own scores.  Tolerance: 4 * scale * 1e-5,
  the project's score tolerance between two GEMM orders through the two log-sum-exps and the diagonal, plus the lse bound."""
  from mmt_amd import metric
  from mmt_amd.search import VideoIndex
  g, gw, _, _ = _data()
  gen = torch.Generator(device=DEV).manual_seed(81)
  t = (0.3 * g + torch.randn(NV, M, D, device=DEV, generator=gen)) / 64        # a caption leaning towards its video
  tw = torch.rand(NV, M, device=DEV, generator=gen)
  scale = 20.0
  got = metric.info_nce_indexed(g, t[:, :, None, :], gw, tw[:, None, :], scale=scale, dtype=dtype)
  assert set(got) == {'loss', 't2v', 'v2t'} and all(isinstance(v, float) for v in got.values())
  if dtype is torch.float32:
    sims = metric.eval_similarity(g, t[:, :, None, :], gw, tw[:, None, :])
  else:
    sims = VideoIndex(g, gw, dtype=dtype).target_scores(t, tw, torch.arange(NV, device=DEV).expand(NV, NV).contiguous())
  x = scale * sims.double()
  target = torch.arange(NV, device=DEV)
  t2v = torch.nn.functional.cross_entropy(x, target).item()
  v2t = torch.nn.functional.cross_entropy(x.t().contiguous(), target).item()
  want, xmax, d = brute_row_lse(sims.cpu().numpy(), scale)
  tol = 4 * scale * 1e-5 + _bound(want, xmax, d, NV, BITS).max()
  print('%s: t2v %.6f (matrix %.6f), v2t %.6f (matrix %.6f), tolerance %.3g' % (dtype, got['t2v'], t2v, got['v2t'], v2t, tol))
  assert abs(got['t2v'] - t2v) <= tol and abs(got['v2t'] - v2t) <= tol
  assert abs(got['loss'] - (t2v + v2t)) <= 2 * tol and got['loss'] == got['t2v'] + got['v2t']
  same = metric.info_nce_indexed(g, t, gw, tw, scale=scale, dtype=dtype)       # the (B, M, d) / (B, M) layout
  assert same == got


def test_errors():
  from mmt_amd import metric
  from mmt_amd.search import VideoIndex
  index, (q, qw) = _index(torch.float32), _queries()
  for name, call in (('query_lse', lambda **kw: index.query_lse(q, qw, BETA, **kw)),
                     ('search_softmax', lambda **kw: index.search_softmax(q, qw, beta=BETA, **kw))):
    for option in ('exclude', 'norm', 'pooling', 'item_pooling', 'after', 'grouping'):
      with pytest.raises(ValueError, match='%s: %s= is out of scope' % (name, option)):
        call(**{option: None})
  for bad in (0.0, INF, float('nan'), torch.tensor(20.0, device=DEV), 20):
    with pytest.raises(ValueError, match='query_lse: beta must be a float with 0 < beta < inf'):
      index.query_lse(q, qw, bad)
    with pytest.raises(ValueError, match='search_softmax: beta must be a float with 0 < beta < inf'):
      index.search_softmax(q, qw, beta=bad)
  empty = VideoIndex.empty(8, M, D, DEV)
  with pytest.raises(ValueError, match='query_lse: the index holds no items'):
    empty.query_lse(q, qw, BETA)
  with pytest.raises(ValueError, match='search_softmax: the index holds no items'):
    empty.search_softmax(q, qw, beta=BETA)
  with pytest.raises(ValueError, match='query_lse: the subset was built for'):
    index.query_lse(q, qw, BETA, subset=VideoIndex(_data()[0][:10], _data()[1][:10]).subset(torch.arange(5, device=DEV)))
  g, gw, _, _ = _data()
  with pytest.raises(ValueError, match='info_nce_indexed: torch.float8_e4m3fn is not supported'):
    metric.info_nce_indexed(g, q[:1].expand(NV, M, D), gw, qw[:1].expand(NV, M), dtype=FP8)
  none = index.query_lse(q[:0], qw[:0], BETA)                                  # no queries: empty fields, no launch
  assert none.lse.shape == (0,) and none.sums.shape == (0,) and none.top_items.shape == (0,)
