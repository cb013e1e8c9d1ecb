"""The per-expert score breakdown on the GPU (mmt_search_expert_parts; expert_scores, search_explained,
pair_expert_scores).  Four kinds of claim: bit identity with numpy's single fp32 division on operands whose sums are
exact; the fp64 definition of tests/expert_parts_ref.py within its derived bound; consistency of the summed parts with
the scores `rescore` and `pair_scores` give the pair; and invariance, bit for bit, of a pair's values under everything
that is not the pair -- its place, its neighbours, C, NQ, the row batching, the query layout, the operand order of a
stored pair, the shard."""
import numpy as np
import pytest
import torch

from tests.expert_parts_ref import U, expert_parts_ref

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
FP8 = torch.float8_e4m3fn
DTYPES = [torch.float32, torch.bfloat16, FP8]
IDS = ['fp32', 'bf16', 'fp8']
MULT = {torch.float32: 4, torch.bfloat16: 8, FP8: 16}
NV = 300
_cache = {}


def _same(a, b):
  """Bit for bit, NaN included."""
  return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _same_scores(a, b):
  return _same(a.parts, b.parts) and _same(a.mix, b.mix)


def _stored(index):
  """The dequantised stored rows of an index as float32 [num_items, M d] on the host: exact on every dtype."""
  n = index.num_items
  rows = index.folded[:n].cpu().float()
  return (rows if index.scales is None else rows * index.scales[:n].cpu()[:, None]).numpy()


def _folded(q, qw):
  """The fp32 fold of the queries as the library forms it: the kernel's own input."""
  from mmt_amd import search
  return search._fold(q, qw).cpu().numpy()


# ---------------------------------------------------------------------------------------------------------- exact

def _exact_shapes(dtype):
  """(M, d): the smallest at which the kernel can still go wrong -- one expert and sixteen at the least d, a d that is no
  multiple of a wave's stride of 16-byte groups nor of anything else (a ragged tail inside every expert), M = 7 with
  d = 64, and a folded row past the LDS budget of 48 KiB (the kernel's other path: the row through the caches)."""
  least = MULT[dtype]
  return [(1, least), (16, least), (3, {4: 20, 8: 24, 16: 48}[least]), (7, 64), (16, 784)]


def _exact_data(dtype, m, d):
  """Q, G from +-{1 .. 8}, weights from {0.5, 1, 2}: exact in bf16 and e4m3, every dot exact in fp32 in any order, the
  denominators exact.  -> the index, the queries, and the exact per-expert dots and gates of ALL 65 x 300 pairs (fp64)."""
  key = ('exact', dtype, m, d)
  if key not in _cache:
    from mmt_amd.search import VideoIndex
    gen = torch.Generator(device=DEV).manual_seed(1000 * m + d)
    ints = lambda *s: (torch.randint(1, 9, s, device=DEV, generator=gen) * (2 * torch.randint(0, 2, s, device=DEV, generator=gen) - 1)).float()
    pick = lambda *s: torch.tensor([0.5, 1.0, 2.0], device=DEV)[torch.randint(0, 3, s, device=DEV, generator=gen)]
    g, gw, q, qw = ints(NV, m, d), pick(NV, m), ints(65, m, d), pick(65, m)
    dots = torch.einsum('qmj,gmj->qgm', (qw[:, :, None] * q).double(), (gw[:, :, None] * g).double())
    gate = qw.double()[:, None, :] * gw.double()[None]
    assert float(dots.abs().max()) < 2 ** 22
    _cache[key] = VideoIndex(g, gw, dtype=dtype), q, qw, dots.cpu().numpy(), gate.cpu().numpy()
  return _cache[key]


def _exact_candidates(c):
  """int64 [65, C]: random with replacement, a seventh of them -1; row 0 opens with item 0, row 1 with item NV - 1, row 2 is
  all -1; with C >= 3 row 0 is (0, 0, NV - 1, ...): a repeat and both ends in one row, behind them a -1 where C > 3."""
  gen = torch.Generator(device=DEV).manual_seed(c)
  cand = torch.randint(0, NV, (65, c), device=DEV, generator=gen)
  cand[torch.rand(65, c, device=DEV, generator=gen) < 1 / 7] = -1
  cand[0, 0], cand[1, 0], cand[2] = 0, NV - 1, -1
  if c >= 3:
    cand[0, 1], cand[0, 2] = 0, NV - 1
  if c > 3:
    cand[0, 3] = -1
  return cand


@pytest.mark.parametrize('shape', range(5), ids=['M1', 'M16', 'ragged', 'M7', 'past-lds'])
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_parts_and_mix_are_numpys_division_of_the_exact_sums(dtype, shape):
  """Catches a dropped or doubled element, an expert boundary off by one load, a tail handled wrong, a scale misplaced."""
  from mmt_amd.search import ExpertScores
  m, d = _exact_shapes(dtype)[shape]
  index, q, qw, dots, gate = _exact_data(dtype, m, d)
  den = gate.sum(-1, keepdims=True)
  assert (den > 0).all() and (den == den.astype(np.float32)).all() and (dots == dots.astype(np.float32)).all()
  want_parts = dots.astype(np.float32) / den.astype(np.float32)          # ONE float32 division of exact operands
  want_mix = gate.astype(np.float32) / den.astype(np.float32)
  for c in (1, 3, 128, 1024):
    cand = _exact_candidates(c)
    host = cand.cpu().numpy()
    rows, none = np.arange(65)[:, None], host < 0
    wp, wm = want_parts[rows, np.where(none, 0, host)], want_mix[rows, np.where(none, 0, host)]
    wp[none], wm[none] = np.nan, np.nan
    assert none[2].all() and (host[0, 0], host[1, 0]) == (0, NV - 1)
    for nq in (1, 65):
      es = index.expert_scores(q[:nq], qw[:nq], cand[:nq])
      assert isinstance(es, ExpertScores) and es.parts.shape == es.mix.shape == (nq, c, m) and es.parts.device == DEV
      assert es.parts.dtype is es.mix.dtype is torch.float32
      gp, gm = es.parts.cpu().numpy(), es.mix.cpu().numpy()
      assert (np.isnan(gp) == none[:nq, :, None]).all() and (np.isnan(gm) == none[:nq, :, None]).all(), (c, nq)
      live = ~none[:nq]
      assert (gp[live].view(np.int32) == wp[:nq][live].view(np.int32)).all(), (c, nq)
      assert (gm[live].view(np.int32) == wm[:nq][live].view(np.int32)).all(), (c, nq)
  assert _same(es.expert_sims, es.parts / es.mix)


# ----------------------------------------------------------------------------------------------------------- fp64

def _random_data(dtype, m, d, nq, nv):
  """Random normal rows, non-negative weights a fifth of them exactly 0, item 3 and query 1 with all-zero weights."""
  key = ('random', dtype, m, d, nq, nv)
  if key not in _cache:
    from mmt_amd.search import VideoIndex
    gen = torch.Generator(device=DEV).manual_seed(7 * m + d + nq)
    g, q = torch.randn(nv, m, d, device=DEV, generator=gen), torch.randn(nq, m, d, device=DEV, generator=gen)
    gw, qw = torch.rand(nv, m, device=DEV, generator=gen), torch.rand(nq, m, device=DEV, generator=gen)
    gw[torch.rand(nv, m, device=DEV, generator=gen) < 0.2] = 0
    qw[torch.rand(nq, m, device=DEV, generator=gen) < 0.2] = 0
    gw[3], qw[1] = 0, 0
    gw[0, 0], qw[0, 0] = 1.0, 1.0
    _cache[key] = VideoIndex(g, gw, dtype=dtype), g, gw, q, qw
  return _cache[key]


@pytest.mark.parametrize('m,d,nq,c,nv', [(3, 48, 5, 40, 50), (7, 512, 8, 32, 256)], ids=['small', 'realistic'])
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_every_part_is_within_the_derived_bound_of_the_fp64_definition(dtype, m, d, nq, c, nv):
  index, _, gw, q, qw = _random_data(dtype, m, d, nq, nv)
  gen = torch.Generator(device=DEV).manual_seed(c)
  cand = torch.randint(-1, nv, (nq, c), device=DEV, generator=gen)
  cand[0, :3] = torch.tensor([3, -1, 3], device=DEV)                       # the item without weights, a none, a repeat
  es = index.expert_scores(q, qw, cand)
  parts, mix, bound = expert_parts_ref(_folded(q, qw), qw.cpu().numpy(), _stored(index), gw.cpu().numpy(),
                                       cand.cpu().numpy(), m, d)
  gp, gm = es.parts.cpu().numpy().astype(np.float64), es.mix.cpu().numpy().astype(np.float64)
  none = cand.cpu().numpy() < 0
  assert (np.isnan(gp) == none[:, :, None]).all() and (np.isnan(gm) == none[:, :, None]).all()
  live = ~none
  err, tol = np.abs(gp - parts)[live], bound[live]
  print('parts: largest error / bound %.3f' % (err / np.maximum(tol, 1e-300)).max())
  print('mix: largest error %.3g against %.3g' % (np.abs(gm - mix)[live].max(), (m + 3) * U))
  assert (err <= tol).all()
  assert (np.abs(gm - mix)[live] <= (m + 3) * U).all()
  zero = (cand == 3).cpu().numpy()                                         # den = 0 -> 1e-5: every part and share is 0
  assert zero.any() and (gp[zero] == 0).all() and (gm[zero] == 0).all() and (gp[1][live[1]] == 0).all()


# ---------------------------------------------------------------------------------------------------- consistency

@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_the_parts_sum_to_the_scores_of_rescore_and_of_pair_scores(dtype):
  m, d, nq, nv = 7, 512, 8, 256
  index, _, gw, q, qw = _random_data(dtype, m, d, nq, nv)
  gen = torch.Generator(device=DEV).manual_seed(5)
  cand = torch.stack([torch.randperm(nv, device=DEV, generator=gen)[:40] for _ in range(nq)])
  cand[:, 7] = -1
  scores, items = index.rescore(q, qw, cand)                               # [8, 40], best first, the -1 as (-inf, -1)
  es = index.expert_scores(q, qw, items)
  host, stored, w = items.cpu().numpy(), _stored(index), gw.cpu().numpy()
  _, _, bound = expert_parts_ref(_folded(q, qw), qw.cpu().numpy(), stored, w, host, m, d)
  live = host >= 0
  assert live.sum() == 8 * 39 and torch.isnan(es.parts[~torch.from_numpy(live).to(DEV)]).all()
  err = np.abs(es.parts.cpu().numpy().astype(np.float64).sum(-1) - scores.cpu().numpy())[live]
  assert (err <= bound.sum(-1)[live] + 1e-5).all(), err.max()              # the summed bound + rescore's documented 1e-5
  # stored items in the queries' place: the Gram row of `pair_scores`
  lists = cand[:, :16].clone()
  lists[:, 7] = lists[:, 0]                                                # a repeat: the self pair again
  lists[0, 3] = -1
  sims = index.pair_scores(lists)                                          # [8, 16, 16]
  heads = lists[:, 0].contiguous()
  pes = index.pair_expert_scores(heads, lists)
  _, _, bound = expert_parts_ref(stored[heads.cpu().numpy()], w[heads.cpu().numpy()], stored, w, lists.cpu().numpy(), m, d)
  live = lists.cpu().numpy() >= 0
  err = np.abs(pes.parts.cpu().numpy().astype(np.float64).sum(-1) - sims[:, 0].cpu().numpy())[live]
  assert (err <= bound.sum(-1)[live] + 1e-5).all(), err.max()
  assert torch.isnan(pes.parts[0, 3]).all() and torch.isnan(pes.mix[0, 3]).all()


# ----------------------------------------------------------------------------------------------------- invariance

@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_the_values_of_a_pair_depend_on_the_pair_alone(dtype, monkeypatch):
  from mmt_amd import search
  m, d, nq, nv, c = 3, 48, 130, 50, 37
  index, _, _, q, qw = _random_data(dtype, m, d, nq, nv)
  gen = torch.Generator(device=DEV).manual_seed(11)
  cand = torch.randint(-1, nv, (nq, c), device=DEV, generator=gen)
  base = index.expert_scores(q, qw, cand)
  perm = torch.randperm(c, device=DEV, generator=gen)                      # another place in its list
  moved = index.expert_scores(q, qw, cand[:, perm])
  assert _same(moved.parts, base.parts[:, perm]) and _same(moved.mix, base.mix[:, perm])
  others = torch.randint(-1, nv, (nq, c), device=DEV, generator=gen)       # other neighbours
  others[:, 5] = cand[:, 5]
  beside = index.expert_scores(q, qw, others)
  assert _same(beside.parts[:, 5], base.parts[:, 5]) and _same(beside.mix[:, 5], base.mix[:, 5])
  alone = index.expert_scores(q, qw, cand[:, 5:6].contiguous())            # C = 1
  assert _same(alone.parts[:, 0], base.parts[:, 5]) and _same(alone.mix[:, 0], base.mix[:, 5])
  one = index.expert_scores(q[77:78], qw[77:78], cand[77:78])              # NQ = 1
  assert _same(one.parts[0], base.parts[77]) and _same(one.mix[0], base.mix[77])
  wide = torch.cat([cand] * 28, 1)[:, :1024].contiguous()                  # C = 1024: another block geometry
  spread = index.expert_scores(q, qw, wide)
  assert _same(spread.parts[:, 999], base.parts[:, 999 % c]) and _same(spread.mix[:, 999], base.mix[:, 999 % c])
  b, caps = 26, 5                                                          # the text layout (B, M, C, d) / (B, C, M)
  text = index.expert_scores(q.reshape(b, caps, m, d).permute(0, 2, 1, 3).contiguous(), qw.reshape(b, caps, m), cand)
  assert _same_scores(text, base)
  monkeypatch.setattr(search, '_BATCH_BYTES', 1)                           # 64-row batches: 64 + 64 + 2 rows
  assert index._row_batches(nq, 8 * c * m) == [(0, 64), (64, 128), (128, 130)]
  assert _same_scores(index.expert_scores(q, qw, cand), base)
  # stored pairs: (g, h) has the bits of (h, g), the self pair and the item without weights included
  a = torch.randint(0, nv, (200,), device=DEV, generator=gen)
  h = torch.randint(0, nv, (200,), device=DEV, generator=gen)
  a[:3], h[:3] = torch.tensor([3, 7, 3], device=DEV), torch.tensor([9, 7, 3], device=DEV)
  ah, ha = index.pair_expert_scores(a, h[:, None].contiguous()), index.pair_expert_scores(h, a[:, None].contiguous())
  assert _same_scores(ah, ha) and not torch.isnan(ah.parts).any()


# ----------------------------------------------------------------------------------------------- search_explained

@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_search_explained_is_search_and_the_breakdown_of_its_list(dtype):
  from mmt_amd.search import VideoIndex
  m, d, nq, nv = 3, 48, 5, 50
  index, g, gw, q, qw = _random_data(dtype, m, d, nq, nv)
  sub = index.subset(torch.arange(0, nv, 2, device=DEV))
  ex = torch.full((nq, 2), -1, device=DEV, dtype=torch.int64)
  ex[:, 0] = torch.arange(nq, device=DEV) * 2
  tags = torch.arange(nv, device=DEV, dtype=torch.int64) % 4
  flt = index.tagging(tags).where(none_of=2)
  few = index.subset(torch.tensor([4, 8, 12, 16, 20, 24], device=DEV))
  barred = torch.tensor([[4, 8, 12]] + [[-1, -1, -1]] * (nq - 1), device=DEV)
  streamed = VideoIndex(g, gw, dtype=dtype)
  streamed.schedule = 'stream'
  cases = [(index, {}), (index, dict(subset=sub)), (index, dict(exclude=ex)), (index, dict(where=flt)),
           (index, dict(subset=sub, exclude=ex, where=flt)), (index, dict(subset=few, exclude=barred)), (streamed, {}),
           (streamed, dict(exclude=ex))]
  for which, options in cases:
    scores, items, es = which.search_explained(q, qw, k=10, **options)
    ws, wi = which.search(q, qw, k=10, **options)
    assert _same(scores, ws) and torch.equal(items, wi), options
    assert _same_scores(es, index.expert_scores(q, qw, wi)), options
    vacant = items < 0
    assert torch.isnan(es.parts[vacant]).all() and not torch.isnan(es.parts[~vacant]).any(), options
  assert items.shape == (nq, 10)
  scores, items, es = index.search_explained(q, qw, k=10, subset=few, exclude=barred)
  assert items.shape == (nq, 6) and (items[0, 3:] == -1).all() and (items[0, :3] >= 0).all() and (items[1:] >= 0).all()
  assert torch.isnan(es.parts[0, 3:]).all() and torch.isnan(es.mix[0, 3:]).all()
  after = (scores[:, 1].contiguous(), items[:, 1].contiguous())            # the next page, explained
  s2, i2, e2 = index.search_explained(q, qw, k=2, subset=few, exclude=barred, after=after)
  assert torch.equal(i2, items[:, 2:4]) and _same(e2.parts, es.parts[:, 2:4])


# -------------------------------------------------------------------------------------------------------- sharded

@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_a_sharded_index_gives_the_bits_of_one_index(dtype):
  from mmt_amd.search import ShardedVideoIndex
  m, d, nq, nv = 3, 48, 130, 50
  index, g, gw, q, qw = _random_data(dtype, m, d, nq, nv)
  sharded = ShardedVideoIndex.empty(60, m, d, [DEV] * 3, dtype=dtype)     # 20 rows per shard
  for lo, hi in ((0, 15), (15, 35), (35, 50)):                              # shard 0 keeps 15 of 20, then 1, then 2
    sharded.add(g[lo:hi], gw[lo:hi])
  assert sharded.shard_sizes[0] < 20 and all(sharded.shard_sizes) and sum(sharded.shard_sizes) == nv
  gen = torch.Generator(device=DEV).manual_seed(13)
  cand = torch.randint(-1, nv, (nq, 24), device=DEV, generator=gen)
  cand[0, :4] = torch.tensor([0, 20, 49, -1], device=DEV)
  owners = sharded._shard_of[cand[0].clamp(min=0)]
  assert set(owners.tolist()) == {0, 1, 2}                                  # every shard in one row
  assert _same_scores(sharded.expert_scores(q, qw, cand), index.expert_scores(q, qw, cand))
  one = index.search_explained(q[:9], qw[:9], k=10)
  many = sharded.search_explained(q[:9], qw[:9], k=10)
  assert _same(many[0], one[0]) and torch.equal(many[1], one[1]) and _same_scores(many[2], one[2])
  items = torch.randint(0, nv, (nq,), device=DEV, generator=gen)
  assert _same_scores(sharded.pair_expert_scores(items, cand), index.pair_expert_scores(items, cand))
