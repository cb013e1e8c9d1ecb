"""Querybank hubness normalisation on the device: VideoIndex.hub_norm, norm= on search / rank_counts / ranks /
target_scores / threshold_counts, the dynamic rule, ShardedVideoIndex and metric.retrieval_metrics_indexed(text_bank=,
video_bank=, beta=).

The truth of every test is built from the device's own plain scores: target_scores with targets arange(NV) gives
score(q, g) bit for bit, so nothing here depends on the summation order of the scoring GEMM.  From that matrix the
expected lse is the fp64 log-sum-exp (test 1), and everything downstream is exact: score' = corrected32(scores, norm.lse)
in numpy float32, a stable top-k and brute-force counts on it (tests/test_index_norm_cpu.py), compared bit for bit."""
import numpy as np
import pytest
import torch

from tests.test_index_norm_cpu import (F32, blockwise_lse32, brute_counts, corrected32, lse64, lse_bound, stable_topk)
from tests.test_search_gpu import _golden

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
DTYPES = [torch.float32, torch.bfloat16]
IDS = ['fp32', 'bf16']
INF = float('inf')
SHAPES = [(1, 1), (63, 127), (65, 129), (130, 4097)]   # (nq, nv): one item, under / over one tile, over one 4096 chunk
M, D, NB = 3, 8, 70


def _cuda(x):
  return torch.as_tensor(x).to(DEV)


def _bits(x):
  x = x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
  return np.ascontiguousarray(x, F32).view(np.int32)


def _scores(index, q, qw):
  """score(q, g) for every stored item, with the bits the scan computes: fp32 numpy [nq, num_items]."""
  tg = torch.arange(index.num_items, device=DEV).repeat(q.shape[0], 1)
  return index.target_scores(q, qw, tg).cpu().numpy()


def _hubby(nq, nv, nb, seed, m=M, d=D, share=0.6):
  """Queries, a gallery and a bank that share a direction c (unit per expert; queries and bank `share` c + noise, items
  0.2 c + noise), and one gallery item (nv // 2) that is 3 c: a clear hub -- the plain top-1 of most queries and bank rows
  (of all of them at share = 2).  Row 1 of the bank and item 1 have all-zero weights."""
  gen = torch.Generator(device=DEV).manual_seed(seed)
  c = torch.randn(1, m, d, device=DEV, generator=gen)
  c = c / c.norm(dim=2, keepdim=True)

  def rows(n, share):
    return share * c + 0.5 * torch.randn(n, m, d, device=DEV, generator=gen), 0.25 + torch.rand(n, m, device=DEV, generator=gen)
  q, qw = rows(nq, share)
  g, gw = rows(nv, 0.2)
  b, bw = rows(nb, share)
  g[nv // 2] = 3 * c[0]
  if nb > 1:
    bw[1] = 0
  if nv > 2:
    gw[1] = 0
  return q, qw, g, gw, b, bw


_CACHE = {}


def _case(nq, nv, dtype):
  """One index, its queries, a norm (beta = 20) and the expected matrices per (shape, dtype), computed once and shared by
  the search and the rank tests: plain scores S and S' = corrected32(S, norm.lse)."""
  key = (nq, nv, dtype)
  if key not in _CACHE:
    from mmt_amd.search import VideoIndex
    q, qw, g, gw, b, bw = _hubby(nq, nv, NB, nq + nv)
    index = VideoIndex(g, gw, dtype=dtype)
    norm = index.hub_norm(b, bw, 20.0)
    plain = _scores(index, q, qw)
    fixed = corrected32(plain, norm.lse.cpu().numpy(), 20.0)
    for a in (plain, fixed):
      a.setflags(write=False)
    _CACHE[key] = (index, q, qw, norm, plain, fixed)
  return _CACHE[key]


# ---- 1. lse against fp64 ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('nb,m,d', [(1, 3, 8), (63, 3, 8), (65, 3, 8), (300, 3, 8), (65, 16, 64)])
def test_lse_against_fp64(nb, m, d, dtype):
  """|lse - ref| <= 2^-23 (NB + |ref| + X + 16), ref the fp64 log-sum-exp of float64(float32(beta)) * score over the device's
  own scores, X = max_b |beta * score|.  Derived, with u = 2^-24 the unit roundoff, not measured:
    - x = fl(beta * score) is off by <= u X, and log-sum-exp moves by at most the largest move of an argument: u X;
    - t = x - m is rounded (<= u |t|) and exp carries about 2 ulp plus, where it is computed as exp2(t log2 e), u |t| more:
      relative error (4 + 2 |t|) u of a term whose share of the sum is at most exp(-|t|); |t| exp(-|t|) <= 1 / e, so all
      terms together move log S by <= (4 + 2 NB / e) u;
    - the sequential sum of a block (<= 63 adds) and the folds (3 roundings and two exps of ~4u each per block, NB / 64
      blocks) have relative error <= (NB + 11 NB / 64) u in S, the same absolute error in log S;
    - log carries about 2 ulp of |log S| <= log NB, and M + log S is rounded once: <= (4 log NB + |ref|) u.
  Sum: u (X + |ref| + 1.91 NB + 4 log NB + 4) <= 2 u (NB + |ref| + X + 16) for NB <= 1000.  With one bank row lse is
  fl(beta * score) itself and the error u X is within 2x of the bound's X term: the tightest case.  The numpy restatement
  of the recipe stays within the bound for NB up to 1000 (tests/test_index_norm_cpu.py); on the MI355X the kernels came to at
  most 0.35 of it on these cases, the restatement on the same scores to the same figure."""
  from mmt_amd.search import HubNorm, VideoIndex
  nv = 130
  q, qw, g, gw, b, bw = _hubby(1, nv, nb, 7 * nb + m, m, d)
  index = VideoIndex(g, gw, dtype=dtype)
  bank = _scores(index, b, bw)
  if nb > 1:
    assert not bank[1].any()                                  # the bank row without weights scores 0 everywhere
  assert not bank[:, 1].any()
  for beta in (1.0, 20.0, 100.0):
    norm = index.hub_norm(b, bw, beta)
    assert isinstance(norm, HubNorm) and (norm.beta, norm.bank_size, norm.num_items, norm.device) == (beta, nb, nv, DEV)
    assert norm.hubs is None and norm.lse.shape == (nv,) and norm.lse.dtype == torch.float32 and norm.lse.device == DEV
    got = norm.lse.cpu().numpy().astype(np.float64)
    ref, bound = lse64(bank, beta), lse_bound(bank, beta)
    err = np.abs(got - ref)
    print('nb=%d m=%d d=%d beta=%g: max err %.3e, max err / bound %.3f, restatement err / bound %.3f' % (
        nb, m, d, beta, err.max(), (err / bound).max(), (np.abs(blockwise_lse32(bank, beta) - ref) / bound).max()))
    assert np.isfinite(got).all() and (err <= bound).all(), (beta, (err / bound).max())
    assert abs(got[1] - np.log(nb)) <= bound[1]               # the item without weights: every x is 0
    # the 4-D text layout of the bank is the same bank
    if beta == 20.0 and nb % 5 == 0:
      b4 = b.reshape(nb // 5, 5, m, d).permute(0, 2, 1, 3).contiguous()
      assert np.array_equal(_bits(index.hub_norm(b4, bw.reshape(nb // 5, 5, m), beta).lse), _bits(norm.lse))


# ---- 2. lse is local to the item --------------------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_lse_depends_on_the_item_the_bank_and_beta_only(dtype, monkeypatch):
  from mmt_amd import search
  from mmt_amd.search import ShardedVideoIndex, VideoIndex
  nv, m, d, nb = 8193, 2, 8, 130
  q, qw, g, gw, b, bw = _hubby(1, nv, nb, 11, m, d)
  big = VideoIndex.empty(9000, m, d, DEV, dtype=dtype)        # spare capacity, filled in two pieces
  big.add(g[:5000], gw[:5000])
  big.add(g[5000:], gw[5000:])
  want = big.hub_norm(b, bw, 20.0).lse
  assert want.shape == (nv,)
  rng = np.random.default_rng(3)
  edges = [0, 127, 128, 4095, 4096, 8192]
  sample = np.concatenate([edges, rng.choice(np.setdiff1d(np.arange(nv), edges), 194, replace=False)])
  sample = _cuda(rng.permutation(sample))                     # 200 items in another order, at other positions, another NV
  assert sample.numel() == 200 and sample.unique().numel() == 200
  small = VideoIndex(g[sample], gw[sample], dtype=dtype)
  assert np.array_equal(_bits(small.hub_norm(b, bw, 20.0).lse), _bits(want[sample]))
  shards = ShardedVideoIndex(g, gw, [DEV] * 3, dtype=dtype)
  sharded = shards.hub_norm(b, bw, 20.0)
  assert sharded.lse.device == DEV and np.array_equal(_bits(sharded.lse), _bits(want))
  for s, sh in enumerate(shards.shards):
    assert np.array_equal(_bits(sharded.parts[s].lse), _bits(want[sh.ids[:sh.num_items]]))
  # the bank in batches of 64 and of 128 rows (the default takes it in one): the same blocks folded in the same order
  per_row = m * d * 4 + -(-nv // 8)
  for rows in (64, 128):
    monkeypatch.setattr(search, '_BATCH_BYTES', rows * per_row)
    assert np.array_equal(_bits(big.hub_norm(b, bw, 20.0).lse), _bits(want)), rows
  monkeypatch.undo()
  assert not np.array_equal(_bits(big.hub_norm(b, bw, 19.0).lse), _bits(want))   # beta is not ignored


# ---- 3. search --------------------------------------------------------------------------------------------------------

def _masks(nv, rng):
  """A subset that empties whole 128-item tiles and thins the others; for a small gallery 20 items at most."""
  items = np.arange(nv)
  allowed = ((items // 128) % 2 == 0) & (rng.random(nv) < 0.5)
  if nv <= 129:
    allowed &= items % 6 == 0
  allowed[nv // 2] = True                                      # the hub stays a candidate
  return allowed


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('nq,nv', SHAPES, ids=['%dx%d' % s for s in SHAPES])
def test_normalised_search_is_exact(nq, nv, dtype):
  index, q, qw, norm, plain, fixed = _case(nq, nv, dtype)
  every = np.ones(nv, bool)
  assert not np.array_equal(_bits(fixed), _bits(plain))
  moved = 0
  for k in (1, 10, 128):
    want_s, want_i = stable_topk(fixed, every, None, k)
    s, i = index.search(q, qw, k=k, norm=norm)
    assert s.shape == i.shape == (nq, min(k, nv)) and s.dtype == torch.float32 and i.dtype == torch.int64
    bad = (i.cpu().numpy() != want_i).sum(), (_bits(s) != _bits(want_s)).sum()
    print('k=%d: %d index, %d score-bit mismatches of %d' % (k, bad[0], bad[1], want_i.size))
    assert np.array_equal(i.cpu().numpy(), want_i) and np.array_equal(_bits(s), _bits(want_s)), k
    # an ignored norm cannot pass: the hub is demoted in some query's list
    plain_i = index.search(q, qw, k=k)[1].cpu().numpy()
    hub = nv // 2
    moved += int(((plain_i == hub).argmax(1) != (want_i == hub).argmax(1)).sum() + ((plain_i == hub).any(1) != (want_i == hub).any(1)).sum())
  assert moved > 0 or nv == 1
  # a subset that empties whole tiles, with exclusions; some queries run out of candidates: (-inf, -1)
  rng = np.random.default_rng(nv)
  allowed = _masks(nv, rng)
  sub = index.subset(_cuda(allowed))
  best = stable_topk(fixed, allowed, None, 5)[1]
  ex = np.concatenate([best, rng.integers(-1, nv, (nq, 3))], 1)
  padded = 0
  for k in (1, 10, 128):
    want_s, want_i = stable_topk(fixed, allowed, ex, k)
    s, i = index.search(q, qw, k=k, subset=sub, exclude=_cuda(ex), norm=norm)
    assert np.array_equal(i.cpu().numpy(), want_i) and np.array_equal(_bits(s), _bits(want_s)), k
    padded += int((want_i < 0).sum())
    want_s, want_i = stable_topk(fixed, every, ex[:, :1], k)    # exclusions alone: E = 1, no subset
    s, i = index.search(q, qw, k=k, exclude=_cuda(ex[:, 0].copy()), norm=norm)
    assert np.array_equal(i.cpu().numpy(), want_i) and np.array_equal(_bits(s), _bits(want_s)), k
  assert padded > 0 or nv > 129
  want_s, want_i = stable_topk(fixed, allowed, None, 10)        # a subset alone
  s, i = index.search(q, qw, k=10, subset=sub, norm=norm)
  assert np.array_equal(i.cpu().numpy(), want_i) and np.array_equal(_bits(s), _bits(want_s))


# ---- 4. rank_counts / ranks -------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('nq,nv', SHAPES, ids=['%dx%d' % s for s in SHAPES])
def test_normalised_rank_counts_are_exact(nq, nv, dtype):
  index, q, qw, norm, plain, fixed = _case(nq, nv, dtype)
  rng = np.random.default_rng(nq)
  allowed = _masks(nv, rng)
  sub = index.subset(_cuda(allowed))
  for t in (1, 3, 33):
    tg = rng.integers(0, nv, (nq, t))
    tg[:, 0] = nv // 2                                          # the hub
    if t > 1:
      tg[rng.random((nq, t)) < 0.2] = -1
      tg[0, 1] = -1
    tg_d = _cuda(tg)
    greater, equal = brute_counts(fixed, tg)
    got_g, got_e = index.rank_counts(q, qw, tg_d, norm=norm)
    assert got_g.shape == got_e.shape == (nq, t) and got_g.dtype == torch.int32
    print('T=%d: mismatches greater %d, equal %d of %d' % (t, (got_g.cpu().numpy() != greater).sum(),
                                                           (got_e.cpu().numpy() != equal).sum(), tg.size))
    assert np.array_equal(got_g.cpu().numpy(), greater) and np.array_equal(got_e.cpu().numpy(), equal), t
    assert (equal[tg >= 0] >= 1).all() and not equal[tg < 0].any() and not greater[tg < 0].any()
    thr = index.target_scores(q, qw, tg_d, norm=norm)           # the target's score' has the bits of the matrix
    want_thr = np.take_along_axis(fixed, np.maximum(tg, 0), 1)
    assert np.array_equal(_bits(thr)[tg >= 0], _bits(want_thr)[tg >= 0]) and bool(torch.isnan(thr[tg_d < 0]).all())
    halves = index.threshold_counts(q, qw, thr, norm=norm)
    assert torch.equal(halves[0], got_g) and torch.equal(halves[1], got_e)
    ranks = index.ranks(q, qw, tg_d, norm=norm)
    assert ranks.dtype == torch.float64
    assert np.array_equal(ranks.cpu().numpy(), np.where(tg >= 0, greater + (equal - 1) / 2, INF))
    # a subset: only its items count; a target outside it is scored as before and does not count itself
    greater, equal = brute_counts(fixed, tg, allowed)
    got_g, got_e = index.rank_counts(q, qw, tg_d, subset=sub, norm=norm)
    assert np.array_equal(got_g.cpu().numpy(), greater) and np.array_equal(got_e.cpu().numpy(), equal), t
    inside = (tg >= 0) & allowed[np.maximum(tg, 0)]
    ranks = index.ranks(q, qw, tg_d, subset=sub, norm=norm).cpu().numpy()
    assert np.array_equal(ranks, np.where(inside, greater + (equal - 1) / 2, INF))
  one = index.ranks(q, qw, _cuda(tg[:, 0].copy()), norm=norm)   # a 1-D target list keeps its shape
  assert one.shape == (nq,)
  if nv > 1:                                                    # an ignored norm cannot pass: the hub's rank moves
    hub = _cuda(np.full(nq, nv // 2))
    assert not torch.equal(index.ranks(q, qw, hub, norm=norm), index.ranks(q, qw, hub))


# ---- 5. the dynamic rule ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_dynamic_normalises_only_the_queries_whose_top1_is_a_hub(dtype):
  from mmt_amd.search import VideoIndex
  nq, nv = 65, 129
  q, qw, g, gw, b, bw = _hubby(nq, nv, NB, 77, share=2.0)      # the hub scores about 6, no other item above 2
  hub, c = nv // 2, g[nv // 2:nv // 2 + 1] / 3
  p = g[3:3 + nq - nq // 2]
  q[nq // 2:] = 4 * (p - (p * c).sum(2, keepdim=True) * c)      # the second half: orthogonal to c, so the hub scores ~0
  qw[nq // 2:] = gw[3:3 + nq - nq // 2]
  bw[1] = 0.5                                                   # a bank row without weights would make item 0 a hub
  index = VideoIndex(g, gw, dtype=dtype)
  norm = index.hub_norm(b, bw, 20.0, dynamic=True)
  static = index.hub_norm(b, bw, 20.0)
  hubs = norm.hubs
  assert hubs.shape == (nv,) and hubs.dtype == torch.bool and hubs.device == DEV
  assert np.array_equal(_bits(norm.lse), _bits(static.lse)) and static.hubs is None
  top1_bank = index.search(b, bw, k=1)[1][:, 0]
  assert torch.equal(hubs, torch.zeros(nv, device=DEV, dtype=torch.bool).index_fill_(0, top1_bank, True))
  assert bool(hubs.any()) and not bool(hubs.all()) and hubs.nonzero()[:, 0].tolist() == [hub]
  sub = index.subset(torch.arange(nv, device=DEV) % 3 != 2)
  assert hub % 3 != 2
  best2 = index.search(q, qw, k=2)[1]
  ex = torch.where(torch.arange(nq, device=DEV) % 2 == 0, best2[:, 0], best2[:, 1]).contiguous()   # even queries lose
  # their plain best, and with it (first half) the hub as their top-1; odd queries lose their second best
  tg = torch.randint(-1, nv, (nq, 3), device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
  for kwargs in ({}, {'subset': sub}, {'exclude': ex}, {'subset': sub, 'exclude': ex}):
    use = hubs[index.search(q, qw, k=1, **kwargs)[1][:, 0]]     # the rule, from the public results
    assert 0 < int(use.sum()) < nq, kwargs
    if not kwargs:
      assert bool(use[:nq // 2].all()) and not bool(use[nq // 2:].any())
    plain = index.search(q, qw, k=10, **kwargs)
    fixed = index.search(q, qw, k=10, norm=static, **kwargs)
    assert not torch.equal(plain[1][use], fixed[1][use])
    for got in (index.search(q, qw, k=10, norm=norm, **kwargs), index.search(q, qw, k=10, norm=norm, dynamic=True, **kwargs)):
      for x, a, p in zip(got, fixed, plain):
        assert np.array_equal(_bits(x[use]) if x.dtype == torch.float32 else x[use].cpu().numpy(),
                              _bits(a[use]) if a.dtype == torch.float32 else a[use].cpu().numpy())
        assert np.array_equal(_bits(x[~use]) if x.dtype == torch.float32 else x[~use].cpu().numpy(),
                              _bits(p[~use]) if p.dtype == torch.float32 else p[~use].cpu().numpy())
    off = index.search(q, qw, k=10, norm=norm, dynamic=False, **kwargs)   # the override: every query normalised
    assert torch.equal(off[1], fixed[1]) and np.array_equal(_bits(off[0]), _bits(fixed[0]))
    if 'exclude' in kwargs:
      continue
    plain = index.rank_counts(q, qw, tg, **kwargs)
    fixed = index.rank_counts(q, qw, tg, norm=static, **kwargs)
    got = index.rank_counts(q, qw, tg, norm=norm, **kwargs)
    for x, a, p in zip(got, fixed, plain):
      assert torch.equal(x[use], a[use]) and torch.equal(x[~use], p[~use])
    assert not torch.equal(fixed[0], plain[0])
    off = index.rank_counts(q, qw, tg, norm=norm, dynamic=False, **kwargs)
    assert torch.equal(off[0], fixed[0]) and torch.equal(off[1], fixed[1])
    ranks = index.ranks(q, qw, tg, norm=norm, **kwargs)
    want = torch.where(use[:, None], index.ranks(q, qw, tg, norm=static, **kwargs), index.ranks(q, qw, tg, **kwargs))
    assert torch.equal(ranks, want)
  with pytest.raises(ValueError, match='dynamic=True needs'):
    index.search(q, qw, norm=static, dynamic=True)


# ---- 6. sharded -------------------------------------------------------------------------------------------------------

def _same(a, b):
  return all(x.shape == y.shape and x.dtype == y.dtype and x.device == y.device and
             (np.array_equal(_bits(x), _bits(y)) if x.dtype == torch.float32 else torch.equal(x, y)) for x, y in zip(a, b))


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('n_shards,pieces', [(1, None), (3, None), (3, (300, 129, 271)), (5, (1, 2, 650, 47))],
                         ids=['1', '3', '3-adds', '5-adds'])
def test_sharded_equals_the_single_index_bit_for_bit(n_shards, pieces, dtype):
  from mmt_amd.search import ShardedHubNorm, ShardedVideoIndex, VideoIndex
  nq, nv = 65, 700
  q, qw, g, gw, b, bw = _hubby(nq, nv, NB, 5)
  g[nv - 1], gw[nv - 1] = g[0], gw[0]                           # a tie across shards
  mono = VideoIndex(g, gw, dtype=dtype)
  if pieces is None:
    shard = ShardedVideoIndex(g, gw, [DEV] * n_shards, dtype=dtype)
  else:
    shard = ShardedVideoIndex.empty(nv, M, D, [DEV] * n_shards, dtype=dtype)
    at = 0
    for n in pieces:
      shard.add(g[at:at + n], gw[at:at + n])
      at += n
    assert at == nv
  assert shard.num_items == nv and len(shard.shards) == n_shards
  mask = torch.arange(nv, device=DEV) % 3 != 0
  subsets = ((None, None), (mono.subset(mask), shard.subset(mask)))
  tg = torch.randint(-1, nv, (nq, 3), device=DEV, generator=torch.Generator(device=DEV).manual_seed(2))
  tg[0, 0] = 0
  ex = mono.search(q, qw, k=1)[1][:, 0].contiguous()
  for dynamic in (False, True):
    norm_m = mono.hub_norm(b, bw, 20.0, dynamic=dynamic)
    norm_s = shard.hub_norm(b, bw, 20.0, dynamic=dynamic)
    assert isinstance(norm_s, ShardedHubNorm) and (norm_s.beta, norm_s.bank_size, norm_s.num_items, norm_s.device) == (20.0, NB, nv, DEV)
    assert np.array_equal(_bits(norm_s.lse), _bits(norm_m.lse))
    assert (norm_s.hubs is None) == (not dynamic) and (not dynamic or torch.equal(norm_s.hubs, norm_m.hubs))
    for sub_m, sub_s in subsets:
      for k in (1, 10, 128):
        want = mono.search(q, qw, k=k, subset=sub_m, norm=norm_m)
        assert _same(shard.search(q, qw, k=k, subset=sub_s, norm=norm_s), want), (dynamic, k)
      assert not torch.equal(want[1], mono.search(q, qw, k=128, subset=sub_m)[1])
      assert _same(shard.search(q, qw, k=10, subset=sub_s, exclude=ex, norm=norm_s),
                   mono.search(q, qw, k=10, subset=sub_m, exclude=ex, norm=norm_m))
      want = mono.rank_counts(q, qw, tg, subset=sub_m, norm=norm_m)
      assert _same(shard.rank_counts(q, qw, tg, subset=sub_s, norm=norm_s), want), dynamic
      assert torch.equal(shard.ranks(q, qw, tg, subset=sub_s, norm=norm_s), mono.ranks(q, qw, tg, subset=sub_m, norm=norm_m))
    if dynamic:
      assert _same(shard.search(q, qw, k=10, norm=norm_s, dynamic=False), mono.search(q, qw, k=10, norm=norm_m, dynamic=False))
  with pytest.raises(ValueError, match='ShardedVideoIndex.hub_norm'):
    shard.search(q, qw, norm=norm_m)
  with pytest.raises(ValueError, match='VideoIndex.hub_norm'):
    mono.search(q, qw, norm=norm_s)


def test_a_norm_is_refused_after_a_further_add_and_on_another_index():
  from mmt_amd.search import ShardedVideoIndex, VideoIndex
  q, qw, g, gw, b, bw = _hubby(3, 10, 4, 1)
  tg = torch.zeros(3, device=DEV, dtype=torch.int64)
  for index in (VideoIndex.empty(12, M, D, DEV), ShardedVideoIndex.empty(12, M, D, [DEV] * 2)):
    with pytest.raises(ValueError, match='holds no items'):
      index.hub_norm(b, bw, 1.0)
    index.add(g, gw)
    with pytest.raises(ValueError, match='no queries'):
      index.hub_norm(b[:0], bw[:0], 1.0)
    old = index.hub_norm(b, bw, 1.0, dynamic=True)
    index.search(q, qw, norm=old)
    index.add(g[:2], gw[:2])
    for call in (lambda: index.search(q, qw, norm=old), lambda: index.rank_counts(q, qw, tg, norm=old),
                 lambda: index.ranks(q, qw, tg, norm=old)):
      with pytest.raises(ValueError, match='built for 10 items'):
        call()


# ---- 7. metrics -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_indexed_metrics_with_banks_on_the_golden_eval_set(dtype):
  """tests/golden/trainer_valid.npz (24 videos, 72 captions, 55 unmasked) with all captions as the text bank and all videos
  as the video bank, beta = 20: the metrics equal cols2metrics of brute-force ranks on the corrected matrices."""
  from mmt_amd.metric import cols2metrics, retrieval_metrics_indexed, v2t_targets
  from mmt_amd.search import VideoIndex
  g, vid, vw, txt, tw = _golden()
  qm = g['query_masks']
  b, caps = qm.shape
  m = vid.shape[1]
  text4 = txt.reshape(b, caps, m, -1).transpose(0, 2, 1, 3)                     # (B, M, C, d)
  tw3 = g['text_weights']
  valid, targets = v2t_targets(qm, b, caps)
  rows = np.flatnonzero(valid)
  vid_d, vw_d = _cuda(vid).float(), _cuda(vw).float().reshape(b, m)
  txt_d, tw_d = _cuda(txt).float().reshape(b * caps, m, -1), _cuda(tw).float().reshape(b * caps, m)
  real, real_w = txt_d[_cuda(rows)].contiguous(), tw_d[_cuda(rows)].contiguous()

  def brute(index, q, qw, bank, tg):
    scores = _scores(index, q, qw)
    if bank is not None:
      scores = corrected32(scores, index.hub_norm(bank[0], bank[1], 20.0).lse.cpu().numpy(), 20.0)
    greater, equal = brute_counts(scores, tg)
    return np.where(tg >= 0, greater + (equal - 1) / 2, INF)

  def expected(text_bank, video_bank):
    t2v = brute(VideoIndex(vid_d, vw_d, dtype=dtype), real, real_w, text_bank, (rows // caps)[:, None])[:, 0]
    v2t = brute(VideoIndex(real, real_w, dtype=dtype), vid_d, vw_d, video_bank, targets).min(1)
    return {'t2v_metrics': dict(cols2metrics(t2v, t2v.size), cols=t2v), 'v2t_metrics': dict(cols2metrics(v2t, v2t.size), cols=v2t)}

  def check(got, want):
    assert set(got) == set(want) == {'t2v_metrics', 'v2t_metrics'}
    for name in want:
      assert set(got[name]) == set(want[name])
      assert np.array_equal(got[name]['cols'], want[name]['cols']), name
      for key in want[name]:
        if key != 'cols':
          assert got[name][key] == want[name][key], (name, key)

  banks = {'text_bank': (text4, tw3), 'video_bank': (vid, vw)}                  # numpy, the text bank in the 4-D layout
  dev_banks = {'text_bank': (txt_d, tw_d), 'video_bank': (vid_d, vw_d)}
  plain = retrieval_metrics_indexed(vid, text4, vw, tw3, query_masks=qm, dtype=dtype)
  check(plain, expected(None, None))
  check(retrieval_metrics_indexed(vid, text4, vw, tw3, query_masks=qm, dtype=dtype, text_bank=None, video_bank=None, beta=None), plain)
  both = retrieval_metrics_indexed(vid, text4, vw, tw3, query_masks=qm, dtype=dtype, beta=20.0, **banks)
  check(both, expected(dev_banks['text_bank'], dev_banks['video_bank']))
  assert not np.array_equal(both['t2v_metrics']['cols'], plain['t2v_metrics']['cols'])
  only_text = retrieval_metrics_indexed(vid, text4, vw, tw3, query_masks=qm, dtype=dtype, beta=20.0, text_bank=banks['text_bank'])
  check(only_text, expected(dev_banks['text_bank'], None))
  sharded = retrieval_metrics_indexed(vid, text4, vw, tw3, query_masks=qm, dtype=dtype, beta=20.0, devices=[DEV] * 3, **banks)
  check(sharded, both)
  cut = np.arange(b) % 3 != 1                                                   # with a cut of the videos it still runs
  out = retrieval_metrics_indexed(vid, text4, vw, tw3, query_masks=qm, dtype=dtype, beta=20.0, video_subset=cut, **banks)
  assert out['t2v_metrics']['cols'].size == int((valid & np.repeat(cut, caps)).sum())


# ---- 8. memory --------------------------------------------------------------------------------------------------------

def test_normalised_scans_allocate_no_quadratic_buffer():
  """A 2048-row bank and 2048 queries over 131072 items: either matrix alone would be 1 GiB.  Budget, linear in the
  gallery: the scans' batches stay within search._BATCH_BYTES = 48 MiB (the folded bank batch and its (m, p) pairs; the
  folded query batch and its chunk lists) and the normaliser adds 12 bytes per item (the (M, S) state and lse) plus, for
  the dynamic rule, 1 byte per item of hubs and a second result: 64 MiB + 16 bytes per item."""
  from mmt_amd.search import VideoIndex
  nq, nv, m, d = 2048, 131072, 7, 512
  gen = torch.Generator(device=DEV).manual_seed(5)
  index = VideoIndex.empty(nv, m, d, DEV)
  for at in range(0, nv, 16384):
    index.add(torch.rand(16384, m, d, device=DEV, generator=gen) - 0.5, torch.rand(16384, m, device=DEV, generator=gen))
  q = torch.rand(nq, m, d, device=DEV, generator=gen) - 0.5
  qw = torch.rand(nq, m, device=DEV, generator=gen)
  tg = torch.randint(0, nv, (nq,), device=DEV, generator=gen)
  torch.cuda.synchronize()
  base = torch.cuda.memory_allocated()
  torch.cuda.reset_peak_memory_stats()
  norm = index.hub_norm(q, qw, 20.0, dynamic=True)
  s, i = index.search(q, qw, k=10, norm=norm)
  ranks = index.ranks(q, qw, tg, norm=norm, dynamic=False)
  torch.cuda.synchronize()
  growth = torch.cuda.max_memory_allocated() - base
  print('allocator peak growth %.1f MiB' % (growth / 2 ** 20))
  assert growth < (64 << 20) + 16 * nv, growth
  assert norm.lse.shape == (nv,) and bool(torch.isfinite(norm.lse).all()) and bool(norm.hubs.any())
  assert bool((s[:, 1:] <= s[:, :-1]).all()) and bool(((ranks >= 0) & (ranks < nv)).all())
  again = index.hub_norm(q, qw, 20.0)
  assert np.array_equal(_bits(again.lse), _bits(norm.lse))
  assert torch.equal(index.ranks(q, qw, tg, norm=again), ranks)
