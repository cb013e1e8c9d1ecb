"""VideoIndex.rank_counts / ranks (mmt_search_rank, mmt_search_rank_bf16) and metric.retrieval_metrics_indexed: for every
query and target item, how many stored items score above the target and how many score exactly equal to it -- the exact
tie-averaged rank of model/metric.py:90-121, 153-243 without the N_query x N_video matrix.

  1. lattice inputs, where fp32, bf16 and fp64 agree bit for bit: the counts equal the fp64 brute force everywhere;
  2. random inputs: the counts equal those taken from the scores search() returns (the threshold pass computes the very
     bits of the scan), and a target is in the top k exactly when fewer than k items beat it;
  3. random inputs against fp64: every count inside the bracket the kernels' stated accuracy (1e-5) allows;
  4. the golden eval set: retrieval_metrics_indexed inside the brackets of the reference's own sims;
  5. no buffer that grows with NQ * NV."""
import functools

import numpy as np
import pytest
import torch

from tests.fixtures import load_npz
from tests.test_index_ranks_cpu import brute_counts
from tests.test_search_gpu import _cuda, _golden, _ref_sims

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
DTYPES = [torch.float32, torch.bfloat16]
INF = float('inf')


def _dev(x):
  return torch.tensor(x, device=DEV)  # a copy: the cached arrays stay read-only


# (nq, nv, M, d, T): across the query block (64), the tile (128), 128-column chunks and several of them, the T slice (32)
LATTICE = [(1, 1, 1, 8, 1), (63, 127, 7, 8, 1), (65, 129, 2, 8, 3), (257, 4097, 16, 8, 2), (130, 8193, 3, 64, 33),
           (63, 70001, 1, 512, 1)]


def _targets(rng, nq, nv, t):
  """Random targets with the edges planted: item 0, the last item, both sides of a tile / chunk edge (128) and of a
  full-size chunk edge (4096), a repeated target within a row, and -1s."""
  tg = rng.integers(0, nv, (nq, t))
  planted = [0, nv - 1] + [e for e in (127, 128, 4095, 4096) if e < nv]
  for i, item in enumerate(planted):
    tg[i % nq, (i // nq) % t] = item
  if t > 1:
    tg[nq // 2, 1] = tg[nq // 2, 0]        # the same target twice in a row
    tg[nq - 1, 0] = -1
    tg[0, t - 1] = -1
  if nq > 7:
    tg[7] = -1                               # a query with no target at all
  return tg.astype(np.int64)


@functools.lru_cache(maxsize=None)
def _lattice(nq, nv, m, d, t):
  """Inputs on which every fold, product, sum and the division by a power-of-two denominator is exact in fp32 and in bf16,
  in any order (embeddings k/8 with |k| <= 4, one power-of-two weight per item, 0/1 query weights with 1, 2 or 4 ones; the
  bf16 query's lo half is zero): the fp64 brute-force counts are the answer bit for bit, with many ties."""
  rng = np.random.default_rng(nq + 3 * nv + 5 * m + 7 * d + 11 * t)
  q = rng.integers(-4, 5, (nq, m, d)).astype(np.float32) / 8
  g = rng.integers(-4, 5, (nv, m, d)).astype(np.float32) / 8
  gw = np.repeat(rng.choice(np.float32([0.5, 1, 2]), (nv, 1)), m, 1)
  qw = np.zeros((nq, m), np.float32)
  for r in range(nq):
    ones = rng.choice([c for c in (1, 2, 4) if c <= m])
    qw[r, rng.choice(m, ones, replace=False)] = 1
  if nq > 1:
    qw[nq // 3] = 0                          # denominator 1e-5, numerator 0: every score 0, one tie of nv items
  ref = _ref_sims(q, qw, g, gw)
  assert np.array_equal(ref, ref.astype(np.float32))
  tg = _targets(rng, nq, nv, t)
  greater, equal = np.zeros((2, nq, t), np.int32)
  for r in range(nq):
    for c in range(t):
      if tg[r, c] >= 0:
        greater[r, c], equal[r, c] = brute_counts(ref[r], tg[r, c])
  for a in (q, qw, g, gw, tg, greater, equal):
    a.setflags(write=False)
  return q, qw, g, gw, tg, greater, equal


@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16'])
@pytest.mark.parametrize('case', range(len(LATTICE)), ids=['x'.join(map(str, s)) for s in LATTICE])
def test_counts_are_exact_on_lattice_inputs(case, dtype):
  from mmt_amd.search import VideoIndex
  nq, nv, m, d, t = LATTICE[case]
  q, qw, g, gw, tg, greater, equal = _lattice(*LATTICE[case])
  if case % 2 and nv > 1:
    # filled in two pieces with room to spare: the unused rows (never written) must not count
    index = VideoIndex.empty(nv + 200, m, d, DEV, dtype=dtype)
    index.add(_dev(g[:nv // 3]), _dev(gw[:nv // 3]))
    index.add(_dev(g[nv // 3:]), _dev(gw[nv // 3:]))
    assert index.num_items == nv < index.capacity
  else:
    index = VideoIndex(_dev(g), _dev(gw), dtype=dtype)
  got_g, got_e = index.rank_counts(_dev(q), _dev(qw), _dev(tg))
  assert got_g.dtype == got_e.dtype == torch.int32 and got_g.shape == got_e.shape == (nq, t) and got_g.device == DEV
  got_g, got_e = got_g.cpu().numpy(), got_e.cpu().numpy()
  print('mismatches: greater %d, equal %d of %d' % ((got_g != greater).sum(), (got_e != equal).sum(), tg.size))
  assert np.array_equal(got_g, greater) and np.array_equal(got_e, equal)
  assert (got_e[tg >= 0] >= 1).all() and not got_g[tg < 0].any() and not got_e[tg < 0].any()
  ranks = index.ranks(_dev(q), _dev(qw), _dev(tg))
  assert ranks.dtype == torch.float64 and ranks.shape == (nq, t)
  want = np.where(tg >= 0, greater + (equal - 1) / 2, INF)
  assert np.array_equal(ranks.cpu().numpy(), want)
  # a 1-D target list is the T = 1 case and keeps its shape
  one = index.ranks(_dev(q), _dev(qw), _dev(tg[:, 0].copy()))
  assert one.shape == (nq,) and np.array_equal(one.cpu().numpy(), want[:, 0])


def _random(nq, nv, m, d, seed):
  gen = torch.Generator(device=DEV).manual_seed(seed)
  g, gw = torch.randn(nv, m, d, device=DEV, generator=gen), torch.rand(nv, m, device=DEV, generator=gen)
  q, qw = torch.randn(nq, m, d, device=DEV, generator=gen), torch.rand(nq, m, device=DEV, generator=gen)
  return q, qw, g, gw


@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16'])
@pytest.mark.parametrize('nq,nv,m,d', [(70, 128, 16, 512), (65, 100, 3, 8), (5, 1, 1, 8), (130, 77, 7, 64)])
def test_counts_equal_those_of_the_scores_search_returns(nq, nv, m, d, dtype):
  """nv <= 128: search(k = 128) returns every score of the scan.  The threshold pass scores the target in another tile
  column than the scan does; were its bits different, an item would not compare equal to itself."""
  from mmt_amd.search import VideoIndex
  q, qw, g, gw = _random(nq, nv, m, d, nq + nv + m + d)
  qw[nq // 2] = 0
  index = VideoIndex(g, gw, dtype=dtype)
  s, i = index.search(q, qw, k=128)
  by_item = torch.empty_like(s).scatter_(1, i, s).cpu().numpy()   # by_item[q, g] = score(q, g)
  rng = np.random.default_rng(nv)
  tg = np.concatenate([np.arange(nv)[None].repeat(nq, 0)[:, :40], rng.integers(-1, nv, (nq, 3))], 1)  # T up to 43: two slices
  got_g, got_e = (x.cpu().numpy() for x in index.rank_counts(q, qw, _cuda(tg)))
  want_g, want_e = np.zeros_like(got_g), np.zeros_like(got_e)
  for r in range(nq):
    for c in range(tg.shape[1]):
      if tg[r, c] >= 0:
        want_g[r, c], want_e[r, c] = brute_counts(by_item[r], tg[r, c])
  print('mismatches: greater %d, equal %d of %d; equal == 0 on %d real targets' % (
      (got_g != want_g).sum(), (got_e != want_e).sum(), tg.size, (got_e[tg >= 0] == 0).sum()))
  assert np.array_equal(got_g, want_g) and np.array_equal(got_e, want_e)
  assert (got_e[nq // 2][tg[nq // 2] >= 0] == nv).all()


@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16'])
def test_a_target_is_in_the_top_k_exactly_when_fewer_than_k_items_beat_it(dtype):
  from mmt_amd.search import VideoIndex
  nq, nv, m, d, k = 70, 5000, 3, 64, 17
  q, qw, g, gw = _random(nq, nv, m, d, 21)
  index = VideoIndex(g, gw, dtype=dtype)
  s, i = index.search(q, qw, k=k)
  rng = np.random.default_rng(2)
  tg = torch.cat([i[:, [0, 5, k - 1]], _cuda(rng.integers(0, nv, (nq, 4)))], 1)   # three from the list, four anywhere
  got_g, got_e = (x.cpu().numpy() for x in index.rank_counts(q, qw, tg))
  s, i, tg = s.cpu().numpy(), i.cpu().numpy(), tg.cpu().numpy()
  listed = 0
  for r in range(nq):
    for c in range(tg.shape[1]):
      at = np.flatnonzero(i[r] == tg[r, c])
      if at.size:
        listed += 1
        assert got_g[r, c] < k
        if (s[r] == s[r, at[0]]).sum() == 1:  # no other returned score equals the target's: its place is its count
          assert got_g[r, c] == at[0], (r, c)
      else:  # at least k items are ahead of it: all of them score above it or equal to it
        assert got_g[r, c] + got_e[r, c] - 1 >= k, (r, c)
        if got_e[r, c] == 1:
          assert got_g[r, c] >= k
  assert listed >= 3 * nq


def _brackets(ref, err, tg):
  """ref [nq, nv] fp64 scores, err (scalar or [nq, nv]) the distance a computed score may lie from ref -> lo, hi [nq, T]:
  the items certainly above the target, and those possibly above or level with it (the target itself excluded)."""
  err = np.broadcast_to(err, ref.shape)
  lo, hi = np.zeros((2,) + tg.shape, np.int64)
  for r in range(tg.shape[0]):
    for c in range(tg.shape[1]):
      t = tg[r, c]
      if t >= 0:
        lo[r, c] = (ref[r] - err[r] > ref[r, t] + err[r, t]).sum()
        hi[r, c] = (ref[r] + err[r] >= ref[r, t] - err[r, t]).sum() - 1
  return lo, hi


def _assert_bracketed(got_g, got_e, lo, hi, tg):
  real = tg >= 0
  print('pairs %d, exact brackets %d, widest %d' % (real.sum(), (real & (lo == hi)).sum(), (hi - lo)[real].max(initial=0)))
  assert (lo[real] <= got_g[real]).all() and ((got_g + got_e - 1)[real] <= hi[real]).all()
  assert (got_e[real] >= 1).all()
  alone = real & (lo == hi)  # no other item within reach of the target
  assert (got_g[alone] == lo[alone]).all() and (got_e[alone] == 1).all()
  assert not got_g[~real].any() and not got_e[~real].any()


# the shapes of test_search_gpu.test_random_sweep_against_fp64 with nv >= 4095
SWEEP = [(257, 4095, 7, 4), (63, 4097, 1, 512), (257, 4097, 16, 4), (1, 70001, 1, 512), (257, 70001, 1, 4), (63, 70001, 16, 4),
         (257, 4095, 7, 512)]


@pytest.mark.parametrize('nq,nv,m,d', SWEEP)
def test_random_sweep_against_fp64(nq, nv, m, d):
  """tol = 1e-5, the search kernels' stated accuracy against fp64: with s the fp64 scores, lo = #(s_j > s_t + 2 tol) and
  hi = #(s_j >= s_t - 2 tol) - 1 bracket the counts, lo <= greater and greater + equal - 1 <= hi; where no other item lies
  within 2 tol of the target, greater == lo and equal == 1.  No pair is skipped.  The bf16 index is bracketed the same way
  by the fp64 scores of its own definition (the stored, rounded fold), where d allows one (d % 8 == 0)."""
  from mmt_amd.search import VideoIndex
  rng = np.random.default_rng(nq * 7 + nv + m * 13 + d)
  q = (rng.random((nq, m, d), dtype=np.float32) * 2 - 1) / np.float32(np.sqrt(d))
  g = (rng.random((nv, m, d), dtype=np.float32) * 2 - 1) / np.float32(np.sqrt(d))
  qw = rng.uniform(0.1, 1, (nq, m)).astype(np.float32)
  gw = rng.uniform(0.1, 1, (nv, m)).astype(np.float32)
  qw[nq // 2] = 0   # every score 0: one tie of nv items
  gw[nv // 3] = 0   # one column 0
  tg = rng.integers(0, nv, (nq, 2)).astype(np.int64)
  tg[0, 0] = nv // 3
  tg[nq - 1, 1] = -1
  for dtype in DTYPES if d % 8 == 0 else DTYPES[:1]:
    index = VideoIndex(_cuda(g), _cuda(gw), dtype=dtype)
    if dtype is torch.float32:
      ref = _ref_sims(q, qw, g, gw)
    else:  # fp64 of the bf16 definition, as tests/test_search_bf16_gpu.py: the dequantised stored fold, weights in the denominator
      deq = index.folded[:nv].to(torch.float32).cpu().numpy().reshape(nv, m, d)
      one = np.ones((nv, m))
      den1 = np.asarray(qw, np.float64) @ one.T
      den1[den1 == 0] = 1e-5
      den = np.asarray(qw, np.float64) @ np.asarray(gw, np.float64).T
      den[den == 0] = 1e-5
      ref = _ref_sims(q, qw, deq, one) * den1 / den
    got_g, got_e = (x.cpu().numpy() for x in index.rank_counts(_cuda(q), _cuda(qw), _cuda(tg)))
    lo, hi = _brackets(ref, 1e-5, tg)
    _assert_bracketed(got_g, got_e, lo, hi, tg)
    assert got_e[nq // 2, 0] == nv and got_g[nq // 2, 0] == 0


@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16'])
def test_indexed_metrics_on_the_golden_eval_set(dtype):
  """tests/golden/trainer_valid.npz: 24 videos, 72 captions, 55 unmasked.  Every rank lies inside the bracket its row of
  the fixture's sims allows -- scores within 2e-5 of them for the fp32 index; for the bf16 index within
  2^-8 * sum_m qw gw <|Q_m|, |G_m|> / sum_m qw gw more (search.py's bound on a score's move against the fp32 index) -- and
  every metric between its values on the all-lo and all-hi rank vectors.  The fixture's closest pair is 3e-6 apart, so the
  recorded metrics themselves are not demanded."""
  from mmt_amd.metric import cols2metrics, retrieval_metrics, retrieval_metrics_indexed, v2t_targets
  g, vid, vw, txt, tw = _golden()
  qm = g['query_masks']
  b, caps = qm.shape
  text4 = txt.reshape(b, caps, vid.shape[1], -1).transpose(0, 2, 1, 3)           # (B, M, C, d)
  out = retrieval_metrics_indexed(vid, text4, vw, g['text_weights'], query_masks=qm, dtype=dtype)
  want = retrieval_metrics(vid, text4, vw, g['text_weights'], query_masks=qm)
  assert set(out) == set(want) and all(set(out[k]) == set(want[k]) for k in want)
  sims = g['sims'].astype(np.float64)
  err = np.full(sims.shape, 2e-5)
  if dtype is torch.bfloat16:
    err += 2.0 ** -8 * _ref_sims(np.abs(txt), tw, np.abs(vid), vw)
  valid, targets = v2t_targets(qm, b, caps)
  rows = np.flatnonzero(valid)
  lo, hi = _brackets(sims[rows], err[rows], (rows // caps)[:, None])
  cols = out['t2v_metrics']['cols']
  assert cols.shape == (55,) and (lo[:, 0] <= cols).all() and (cols <= hi[:, 0]).all()
  assert (lo[:, 0] <= g['t2v_cols']).all() and (g['t2v_cols'] <= hi[:, 0]).all()
  bounds = {'t2v_metrics': (lo[:, 0], hi[:, 0])}
  # video to text: the gallery is the 55 unmasked captions, a video's rank the best among its own
  lo, hi = _brackets(sims[rows].T, err[rows].T, targets)
  lo, hi = (np.where(targets >= 0, x, np.iinfo(np.int64).max).min(1) for x in (lo, hi))
  cols = out['v2t_metrics']['cols']
  assert cols.shape == (24,) and (lo <= cols).all() and (cols <= hi).all()
  assert (lo <= g['v2t_cols']).all() and (g['v2t_cols'] <= hi).all()
  bounds['v2t_metrics'] = (lo, hi)
  for name, (lo, hi) in bounds.items():
    m_lo, m_hi = cols2metrics(lo, lo.size), cols2metrics(hi, hi.size)
    print(name, {k: (m_lo[k], out[name][k], m_hi[k]) for k in m_lo})
    for k in m_lo:
      assert min(m_lo[k], m_hi[k]) <= out[name][k] <= max(m_lo[k], m_hi[k]), (name, k)


def test_ranks_allocate_no_quadratic_buffer():
  """The bound of test_search_gpu.test_search_allocates_no_quadratic_buffer: the matrix alone would be 1 GiB."""
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
  ranks = index.ranks(q, qw, tg)
  torch.cuda.synchronize()
  growth = torch.cuda.max_memory_allocated() - base
  print('allocator peak growth %.1f MiB' % (growth / 2 ** 20))
  assert growth < 64 << 20, growth
  again = index.ranks(q, qw, tg)
  assert torch.equal(ranks, again)
  assert ranks.shape == (nq,) and bool((ranks >= 0).all()) and bool((ranks < nv).all())
  counts = index.rank_counts(q, qw, tg), index.rank_counts(q, qw, tg)
  assert torch.equal(counts[0][0], counts[1][0]) and torch.equal(counts[0][1], counts[1][1])
