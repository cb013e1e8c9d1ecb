"""VideoIndex.subset and the masked scans behind search(subset=, exclude=), rank_counts(subset=), ranks(subset=)
(mmt_search_subset_pack, mmt_search_topk_ex, mmt_search_rank_ex and their bf16 forms), and
metric.retrieval_metrics_indexed(video_subset=):

  1. lattice inputs, where fp32, bf16 and fp64 agree bit for bit: the top k' over the allowed items equals the fp64 brute
     force in score and index, for every kind of subset (whole tiles skipped, one item, across a chunk edge, ...);
  2. random inputs, nv <= 128: equal to plain search(k = 128) with the disallowed entries dropped, bit for bit;
  3. random inputs against fp64 at nv = 4097 / 8193 within the kernels' stated 1e-5;
  4. exclusions; 5. an all-ones subset equals no subset; 6. rank counts over the allowed items;
  7. the metrics of a cut equal those of the gathered arrays; 8. no buffer that grows with NQ * NV."""
import functools

import numpy as np
import pytest
import torch

from tests.test_index_ranks_cpu import brute_counts
from tests.test_index_ranks_gpu import _dev, _lattice, _random
from tests.test_index_subset_cpu import brute_topk, pack_reference
from tests.test_search_gpu import _cuda, _ref_sims

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
DTYPES = [torch.float32, torch.bfloat16]
INF = float('inf')

# (nq, nv, M, d, T): the first five shapes of tests/test_index_ranks_gpu.py (their lattices are shared with that file)
LATTICE = [(1, 1, 1, 8, 1), (63, 127, 7, 8, 1), (65, 129, 2, 8, 3), (130, 8193, 3, 64, 33), (257, 4097, 16, 8, 2)]
IDS = ['x'.join(map(str, s)) for s in LATTICE]


def _subsets(nv):
  """name -> bool [nv], the empty ones dropped."""
  every = np.arange(nv)
  rng = np.random.default_rng(nv)
  tenth = rng.random(nv) < 0.1
  tenth[rng.integers(nv)] = True
  out = {'all': every >= 0, 'first': every == 0, 'last': every == nv - 1, 'every_other': every % 2 == 1,
         'without_tile_1': (every < 128) | (every >= 256), 'only_tile_1': (every >= 128) & (every < 256),
         'across_chunk_edge': (every >= 4000) & (every < 4200), 'random_tenth': tenth}
  return {n: m for n, m in out.items() if m.any()}


@functools.lru_cache(maxsize=None)
def _lattice_scores(case):
  q, qw, g, gw = _lattice(*LATTICE[case])[:4]
  ref = _ref_sims(q, qw, g, gw)
  ref.setflags(write=False)
  return ref


@functools.lru_cache(maxsize=None)
def _lattice_topk(case, name):
  """The brute-force top 128 of the allowed items: the lists for smaller k are its prefixes."""
  s, i = brute_topk(_lattice_scores(case), _subsets(LATTICE[case][1])[name], None, 128)
  s.setflags(write=False)
  i.setflags(write=False)
  return s, i


def _index(case, dtype, split):
  from mmt_amd.search import VideoIndex
  nq, nv, m, d, t = LATTICE[case]
  g, gw = _lattice(*LATTICE[case])[2:4]
  if split and nv > 1:
    # filled in two pieces with room to spare: neither the unused rows (never written) nor the padding bits may appear
    index = VideoIndex.empty(nv + 200, m, d, DEV, dtype=dtype)
    index.add(_dev(g[:nv // 3]), _dev(gw[:nv // 3]))
    index.add(_dev(g[nv // 3:]), _dev(gw[nv // 3:]))
    assert index.num_items == nv < index.capacity
    return index
  return VideoIndex(_dev(g), _dev(gw), dtype=dtype)


def _make_subset(index, mask, as_ids):
  if not as_ids:
    return index.subset(_cuda(mask))
  ids = np.flatnonzero(mask)
  ids = np.random.default_rng(ids.size).permutation(np.concatenate([ids, ids[:3]]))   # any order, duplicates
  return index.subset(_cuda(ids.astype(np.int64)))


@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16'])
@pytest.mark.parametrize('case', range(len(LATTICE)), ids=IDS)
def test_search_is_exact_on_lattice_inputs(case, dtype):
  nq, nv, m, d, t = LATTICE[case]
  q, qw = _lattice(*LATTICE[case])[:2]
  q, qw = _dev(q), _dev(qw)
  index = _index(case, dtype, split=case % 2 == 0)
  for n, (name, mask) in enumerate(_subsets(nv).items()):
    sub = _make_subset(index, mask, as_ids=n % 2 == 1)
    assert sub.count == mask.sum() and sub.num_items == nv and sub.words.device == DEV
    assert sub.words.dtype == torch.uint32 and sub.words.data_ptr() % 16 == 0
    assert np.array_equal(sub.words.cpu().numpy(), pack_reference(mask)), name
    want_s, want_i = _lattice_topk(case, name)
    for k in (1, 10, 128):
      s, i = index.search(q, qw, k=k, subset=sub)
      kout = min(k, int(mask.sum()))
      assert s.shape == i.shape == (nq, kout) and s.dtype == torch.float32 and i.dtype == torch.int64
      s, i = s.cpu().numpy(), i.cpu().numpy()
      bad = (i != want_i[:, :kout]).sum(), (s != want_s[:, :kout]).sum()
      print('%s k=%d: %d index, %d score mismatches of %d' % (name, k, bad[0], bad[1], i.size))
      assert np.array_equal(i, want_i[:, :kout]) and np.array_equal(s, want_s[:, :kout]), (name, k)


def _bits(x):
  return np.ascontiguousarray(x, np.float32).view(np.int32)


@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16'])
@pytest.mark.parametrize('nq,nv,m,d', [(70, 128, 16, 512), (65, 100, 3, 8), (130, 77, 7, 64)])
def test_masked_search_equals_the_plain_list_with_the_disallowed_dropped(nq, nv, m, d, dtype):
  """nv <= 128: plain search(k = 128) returns every item, in order.  The masked search must return that list less the
  disallowed entries, cut to k' -- the very same score bits, since the mask acts at selection only."""
  from mmt_amd.search import VideoIndex
  q, qw, g, gw = _random(nq, nv, m, d, nq + nv + m + d)
  qw[nq // 2] = 0
  index = VideoIndex(g, gw, dtype=dtype)
  s_all, i_all = (x.cpu().numpy() for x in index.search(q, qw, k=128))
  rng = np.random.default_rng(nv)
  mask = rng.random(nv) < 0.6
  ex = rng.integers(-1, nv, (nq, 3)).astype(np.int64)
  ex[:, 0] = i_all[:, 0]                       # the best item of every query
  ex[3] = -1
  for sub_mask, exclude in ((mask, None), (None, ex), (mask, ex)):
    sub = None if sub_mask is None else index.subset(_cuda(sub_mask))
    allowed = np.ones(nv, bool) if sub_mask is None else sub_mask
    for k in (1, 10, 128):
      s, i = index.search(q, qw, k=k, subset=sub, exclude=None if exclude is None else _cuda(exclude))
      kout = min(k, int(allowed.sum()))
      want_s = np.full((nq, kout), -INF, np.float32)
      want_i = np.full((nq, kout), -1, np.int64)
      for r in range(nq):
        keep = allowed[i_all[r]]
        if exclude is not None:
          keep &= ~np.isin(i_all[r], exclude[r])
        n = min(kout, int(keep.sum()))
        want_s[r, :n], want_i[r, :n] = s_all[r][keep][:n], i_all[r][keep][:n]
      assert s.shape == i.shape == (nq, kout)
      assert np.array_equal(i.cpu().numpy(), want_i) and np.array_equal(_bits(s.cpu().numpy()), _bits(want_s)), k


@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16'])
@pytest.mark.parametrize('nq,nv,m,d', [(70, 4097, 3, 64), (130, 8193, 2, 32)])
def test_random_inputs_against_fp64(nq, nv, m, d, dtype):
  """The kernels' stated accuracy against fp64 is 1e-5 per score, so an item left out may beat the last returned one by
  at most 2e-5 in fp64.  The bf16 index is held against the fp64 scores of its own definition (the stored, rounded fold),
  as tests/test_index_ranks_gpu.py does."""
  from mmt_amd.search import VideoIndex
  rng = np.random.default_rng(nq * 7 + nv + m * 13 + d)
  q = (rng.random((nq, m, d), dtype=np.float32) * 2 - 1) / np.float32(np.sqrt(d))
  g = (rng.random((nv, m, d), dtype=np.float32) * 2 - 1) / np.float32(np.sqrt(d))
  qw = rng.uniform(0.1, 1, (nq, m)).astype(np.float32)
  gw = rng.uniform(0.1, 1, (nv, m)).astype(np.float32)
  index = VideoIndex(_cuda(g), _cuda(gw), dtype=dtype)
  if dtype is torch.float32:
    ref = _ref_sims(q, qw, g, gw)
  else:
    deq = index.folded[:nv].to(torch.float32).cpu().numpy().reshape(nv, m, d)
    one = np.ones((nv, m))
    ref = _ref_sims(q, qw, deq, one) * (np.asarray(qw, np.float64) @ one.T) / (np.asarray(qw, np.float64) @ np.asarray(gw, np.float64).T)
  mask = rng.random(nv) < 0.5
  mask[128:256] = False                        # one tile skipped
  best = np.argsort(-np.where(mask, ref, -INF), axis=1, kind='stable')
  ex = np.stack([best[:, 0], best[:, 2], rng.integers(-1, nv, nq)], 1).astype(np.int64)   # the top-1 among them
  k = 10
  s, i = index.search(_cuda(q), _cuda(qw), k=k, subset=index.subset(_cuda(mask)), exclude=_cuda(ex))
  s, i = s.cpu().numpy(), i.cpu().numpy()
  assert s.shape == (nq, k) and (i >= 0).all()
  worst = 0.0
  for r in range(nq):
    ok = mask.copy()
    ok[ex[r][ex[r] >= 0]] = False
    assert ok[i[r]].all() and len(set(i[r].tolist())) == k, r
    assert np.all(np.diff(s[r]) <= 0), r
    assert np.abs(s[r] - ref[r, i[r]]).max() <= 1e-5, r
    ok[i[r]] = False
    worst = max(worst, ref[r, ok].max() - ref[r, i[r, -1]])
  print('largest fp64 lead of an item left out over the last returned: %.3g' % worst)
  assert worst <= 2e-5


@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16'])
@pytest.mark.parametrize('case', [2, 4], ids=[IDS[2], IDS[4]])
def test_exclusions(case, dtype, monkeypatch):
  nq, nv, m, d, t = LATTICE[case]
  q, qw = _lattice(*LATTICE[case])[:2]
  q, qw = _dev(q), _dev(qw)
  ref = _lattice_scores(case)
  index = _index(case, dtype, split=True)
  rng = np.random.default_rng(case)
  top = _lattice_topk(case, 'all')[1]           # [nq, 128] best items of every query, no restriction
  every_other = _subsets(nv)['every_other']
  sub = index.subset(_cuda(every_other))
  for e in (1, 3, 32):
    ex = np.stack([rng.permutation(top[r, :40])[:e] for r in range(nq)]).astype(np.int64)   # items that matter
    ex[:, 0] = top[:, 0]                        # the top-1 ...
    if e > 1:
      ex[:, 1] = np.where(np.arange(nq) % 2, ex[:, 0], -1)   # ... a duplicate of it, or none
      ex[:, e - 1] = 2 * rng.integers(0, nv // 2, nq)        # an even item: outside the every-other subset
    ex[nq // 2] = -1                            # a row that bars nothing
    for mask, s_arg in ((np.ones(nv, bool), None), (every_other, sub)):
      want_s, want_i = brute_topk(ref, mask, ex, 128)   # the lists for smaller k are its prefixes
      for k in (1, 10, 128):
        s, i = index.search(q, qw, k=k, subset=s_arg, exclude=_cuda(ex))
        kout = min(k, int(mask.sum()))
        assert s.shape == i.shape == (nq, kout)
        assert np.array_equal(i.cpu().numpy(), want_i[:, :kout]) and np.array_equal(s.cpu().numpy(), want_s[:, :kout]), (e, k)
  # a 1-D list is E = 1 and bars the best item: the answer is the plain list from its second entry on
  s, i = index.search(q, qw, k=10, exclude=_cuda(top[:, 0].copy()))
  s0, i0 = index.search(q, qw, k=11)
  assert torch.equal(i, i0[:, 1:]) and torch.equal(s, s0[:, 1:])
  # five items allowed, three of them barred, k = 10: two results, then (-inf, -1)
  five = np.array([0, 5, 127, 128, nv - 3])
  ex = np.tile(five[2:], (nq, 1)).astype(np.int64)
  s, i = index.search(q, qw, k=10, subset=index.subset(_cuda(five.astype(np.int64))), exclude=_cuda(ex))
  assert s.shape == (nq, 5)
  want_s, want_i = brute_topk(ref, np.isin(np.arange(nv), five), ex, 10)
  assert np.array_equal(i.cpu().numpy(), want_i) and np.array_equal(s.cpu().numpy(), want_s)
  assert (want_i[:, 2:] == -1).all() and (want_i[:, :2] >= 0).all() and np.isneginf(want_s[:, 2:]).all()
  # E = 33 and values out of range are refused before anything is launched
  from mmt_amd import search
  monkeypatch.setattr(search._lib, 'lib', lambda: pytest.fail('a launch was prepared'))
  with pytest.raises(ValueError, match='exclude'):
    index.search(q, qw, k=10, exclude=torch.zeros(nq, 33, device=DEV, dtype=torch.int64))
  for bad in (-2, nv):
    with pytest.raises(ValueError, match='exclude must lie'):
      index.search(q, qw, k=10, exclude=torch.full((nq, 2), bad, device=DEV, dtype=torch.int64))
  with pytest.raises(ValueError, match='queries but exclude'):
    index.search(q, qw, k=10, exclude=torch.zeros(nq + 1, 2, device=DEV, dtype=torch.int64))


@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16'])
def test_an_all_ones_subset_equals_no_subset(dtype):
  from mmt_amd.search import VideoIndex
  nq, nv, m, d = 130, 8193, 3, 64
  q, qw, g, gw = _random(nq, nv, m, d, 77)
  index = VideoIndex(g, gw, dtype=dtype)
  sub = index.subset(torch.ones(nv, device=DEV, dtype=torch.bool))
  assert sub.count == nv
  for k in (1, 10, 128):
    a, b = index.search(q, qw, k=k), index.search(q, qw, k=k, subset=sub)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
  tg = torch.randint(-1, nv, (nq, 5), device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
  a, b = index.rank_counts(q, qw, tg), index.rank_counts(q, qw, tg, subset=sub)
  assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
  assert torch.equal(index.ranks(q, qw, tg), index.ranks(q, qw, tg, subset=sub))
  # a subset built before a further add no longer fits the index
  grown = VideoIndex.empty(nv + 1, m, d, DEV, dtype=dtype)
  grown.add(g, gw)
  old = grown.subset(torch.ones(nv, device=DEV, dtype=torch.bool))
  grown.add(g[:1], gw[:1])
  with pytest.raises(ValueError, match='built for'):
    grown.search(q, qw, subset=old)


@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16'])
@pytest.mark.parametrize('case', range(len(LATTICE)), ids=IDS)
def test_rank_counts_are_exact_on_lattice_inputs(case, dtype):
  nq, nv, m, d, t = LATTICE[case]
  q, qw, g, gw, tg = _lattice(*LATTICE[case])[:5]   # targets planted at tile and chunk edges; T = 33 crosses the slice
  ref = _lattice_scores(case)
  index = _index(case, dtype, split=case % 2 == 1)
  q, qw, tg_d = _dev(q), _dev(qw), _dev(tg)
  outside = 0
  for name, mask in _subsets(nv).items():
    sub = index.subset(_cuda(mask))
    got_g, got_e = (x.cpu().numpy() for x in index.rank_counts(q, qw, tg_d, subset=sub))
    assert got_g.shape == got_e.shape == (nq, t) and got_g.dtype == np.int32
    want_g, want_e = np.zeros((2, nq, t), np.int32)
    for r in range(nq):
      row = ref[r, mask]
      for c in range(t):
        if tg[r, c] >= 0:   # brute_counts over the allowed items; the target's own score stays its threshold
          want_g[r, c], want_e[r, c] = int((row > ref[r, tg[r, c]]).sum()), int((row == ref[r, tg[r, c]]).sum())
    print('%s: mismatches greater %d, equal %d of %d' % (name, (got_g != want_g).sum(), (got_e != want_e).sum(), tg.size))
    assert np.array_equal(got_g, want_g) and np.array_equal(got_e, want_e), name
    inside = (tg >= 0) & mask[np.maximum(tg, 0)]
    assert (got_e[inside] >= 1).all()
    if name == 'all':
      for r in range(0, nq, 7):
        assert (got_g[r, 0], got_e[r, 0]) == (brute_counts(ref[r], tg[r, 0]) if tg[r, 0] >= 0 else (0, 0))
    ranks = index.ranks(q, qw, tg_d, subset=sub).cpu().numpy()
    assert np.array_equal(ranks, np.where(inside, want_g + (want_e - 1) / 2, INF)), name
    outside += int(((tg >= 0) & ~inside).sum())
    one = index.ranks(q, qw, _dev(tg[:, 0].copy()), subset=sub)
    assert one.shape == (nq,) and np.array_equal(one.cpu().numpy(), ranks[:, 0])
  assert outside > 0 or nv == 1   # targets outside the subset were met: counted against, not counted, rank +inf


@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16'])
def test_metrics_of_a_cut_equal_those_of_the_gathered_arrays(dtype):
  from mmt_amd.metric import retrieval_metrics_indexed
  b, c, m, d = 70, 3, 2, 8
  txt, tw, vid, vw = (np.array(x) for x in _lattice(b * c, b, m, d, 1)[:4])   # copies: the cached arrays stay read-only
  text4 = np.ascontiguousarray(txt.reshape(b, c, m, d).transpose(0, 2, 1, 3))   # (B, M, C, d), rows b*C + c
  tw3 = tw.reshape(b, c, m)
  rng = np.random.default_rng(5)
  qm = (rng.random((b, c)) < 0.6).astype(np.float32)   # padded captions
  qm[:, 0] = 1
  qm[[4, 69]] = 0                                      # videos without a real caption, one of them in the cut
  cut = rng.random(b) < 0.4
  cut[[0, 4, 64, 65]] = True
  cut[69] = False
  ids = np.flatnonzero(cut)
  want = retrieval_metrics_indexed(vid[ids], text4[ids], vw[ids], tw3[ids], query_masks=qm[ids], dtype=dtype)
  shuffled = np.random.default_rng(6).permutation(np.concatenate([ids, ids[:2]]))
  for video_subset in (cut, torch.from_numpy(cut), ids, torch.from_numpy(shuffled).to(DEV)):
    got = retrieval_metrics_indexed(vid, text4, vw, tw3, query_masks=qm, dtype=dtype, video_subset=video_subset)
    assert set(got) == set(want) == {'t2v_metrics', 'v2t_metrics'}
    for name in want:
      assert set(got[name]) == set(want[name])
      assert np.array_equal(got[name]['cols'], want[name]['cols']), name
      for key in want[name]:
        if key != 'cols':
          assert got[name][key] == want[name][key], (name, key)
  assert want['t2v_metrics']['cols'].shape == (int(qm[ids].sum()),) and want['v2t_metrics']['cols'].shape == (ids.size,)
  assert np.isinf(want['v2t_metrics']['cols']).sum() == 1   # video 4
  # no cut: today's path
  whole = retrieval_metrics_indexed(vid, text4, vw, tw3, query_masks=qm, dtype=dtype)
  every = retrieval_metrics_indexed(vid, text4, vw, tw3, query_masks=qm, dtype=dtype, video_subset=np.ones(b, bool))
  for name in whole:
    assert np.array_equal(whole[name]['cols'], every[name]['cols'])


def test_masked_scans_allocate_no_quadratic_buffer():
  """The bound of tests/test_index_ranks_gpu.py: the matrix alone would be 1 GiB."""
  from mmt_amd.search import VideoIndex
  nq, nv, m, d = 2048, 131072, 7, 512
  gen = torch.Generator(device=DEV).manual_seed(5)
  index = VideoIndex.empty(nv, m, d, DEV)
  for at in range(0, nv, 16384):
    index.add(torch.rand(16384, m, d, device=DEV, generator=gen) - 0.5, torch.rand(16384, m, device=DEV, generator=gen))
  q = torch.rand(nq, m, d, device=DEV, generator=gen) - 0.5
  qw = torch.rand(nq, m, device=DEV, generator=gen)
  tg = torch.randint(0, nv, (nq,), device=DEV, generator=gen)
  allowed = torch.rand(nv, device=DEV, generator=gen) < 0.5
  torch.cuda.synchronize()
  base = torch.cuda.memory_allocated()
  torch.cuda.reset_peak_memory_stats()
  sub = index.subset(allowed)
  s, i = index.search(q, qw, k=10, subset=sub, exclude=tg)
  ranks = index.ranks(q, qw, tg, subset=sub)
  torch.cuda.synchronize()
  growth = torch.cuda.max_memory_allocated() - base
  print('allocator peak growth %.1f MiB' % (growth / 2 ** 20))
  assert growth < 64 << 20, growth
  assert sub.words.numel() == nv // 32 and sub.count == int(allowed.sum())
  assert bool(allowed[i].all()) and not bool((i == tg[:, None]).any()) and bool((s[:, 1:] <= s[:, :-1]).all())
  assert bool(((ranks >= 0) & (ranks < sub.count))[allowed[tg]].all()) and bool(torch.isinf(ranks[~allowed[tg]]).all())
  again = index.search(q, qw, k=10, subset=sub, exclude=tg)
  assert torch.equal(s, again[0]) and torch.equal(i, again[1]) and torch.equal(ranks, index.ranks(q, qw, tg, subset=sub))
