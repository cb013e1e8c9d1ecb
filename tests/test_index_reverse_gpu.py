"""Reverse search and CSLS normalisation on the device: VideoIndex.reverse_search, VideoIndex.csls_norm, norm=<csls> on
search / rank_counts / target_scores, the dynamic rule, ShardedVideoIndex and
metric.retrieval_metrics_indexed(bank_norm='csls').

The truth of every test is built from the device's own plain scores, as in tests/test_index_norm_gpu.py: target_scores
with targets arange(NV) gives S[q, g] = score(q, g) bit for bit.  Everything expected is exact numpy on S: the reverse lists
are a stable top-k of S.T, r[g] is the float32 chain of tests/test_index_reverse_cpu.py on those lists, and downstream
score' = corrected32(S, r, 2.0).  A returned score comes out of a key, which holds -0 as +0: where the expected score is a
zero the sign is not compared here -- the tie test compares the bits with what `search` returns for the pair instead."""
import numpy as np
import pytest
import torch

from tests.test_index_norm_cpu import F32, brute_counts, corrected32, stable_topk
from tests.test_index_norm_gpu import _bits, _cuda, _hubby, _masks, _same, _scores
from tests.test_index_reverse_cpu import csls_bound, csls_r32
from tests.test_search_gpu import _golden

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
FP8 = torch.float8_e4m3fn
DTYPES3 = [torch.float32, torch.bfloat16, FP8]
IDS3 = ['fp32', 'bf16', 'fp8']
DTYPES = DTYPES3[:2]
IDS = IDS3[:2]
INF = float('inf')
SHAPES = [(1, 1), (63, 127), (65, 129), (130, 4097)]   # (nq, nv): one pair, under / over one tile and block, over one chunk
M, D, NB = 3, 16, 70
KS = (1, 10, 32)


def _reverse(scores, k):
  """The expected reverse lists of a score matrix [nq, nv]: (scores fp32 [nv, k'], rows int64 [nv, k']), k' = min(k, nq)."""
  return stable_topk(scores.T, np.ones(scores.shape[0], bool), None, k)


def _equal_scores(got, want):
  """Bit for bit, but for the sign of a zero (module docstring)."""
  got, want = _bits(got), _bits(want)
  return got.shape == want.shape and bool(((got == want) | (((got | want) & 0x7fffffff) == 0)).all())


def _check_lists(got, scores, k):
  want_s, want_r = _reverse(scores, k)
  s, r = got
  nq, nv = scores.shape
  assert s.shape == r.shape == (nv, min(k, nq)) and s.dtype == torch.float32 and r.dtype == torch.int64
  assert s.device == r.device == DEV
  bad = (r.cpu().numpy() != want_r).sum(), (_bits(s) != _bits(want_s)).sum()
  print('k=%d: %d row, %d score-bit mismatches of %d' % (k, bad[0], bad[1], want_r.size))
  assert np.array_equal(r.cpu().numpy(), want_r) and _equal_scores(s, want_s), k


def _data(nq, nv, seed, m=M, d=D):
  gen = torch.Generator(device=DEV).manual_seed(seed)
  q = torch.randn(nq, m, d, device=DEV, generator=gen)
  qw = 0.25 + torch.rand(nq, m, device=DEV, generator=gen)
  g = torch.randn(nv, m, d, device=DEV, generator=gen)
  gw = 0.25 + torch.rand(nv, m, device=DEV, generator=gen)
  return q, qw, g, gw


# ---- 1. the lists, bit for bit ----------------------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', DTYPES3, ids=IDS3)
@pytest.mark.parametrize('nq,nv', SHAPES, ids=['%dx%d' % s for s in SHAPES])
def test_reverse_lists_are_exact(nq, nv, dtype):
  from mmt_amd.search import VideoIndex
  q, qw, g, gw = _data(nq, nv, 3 * nq + nv)
  index = VideoIndex(g, gw, dtype=dtype)
  scores = _scores(index, q, qw)
  for k in KS:
    _check_lists(index.reverse_search(q, qw, k=k), scores, k)
  s, r = index.reverse_search(q, qw)                            # the default is k = 10
  assert s.shape == (nv, min(10, nq))


@pytest.mark.parametrize('dtype', DTYPES3, ids=IDS3)
def test_reverse_lists_are_exact_at_sixteen_experts(dtype):
  from mmt_amd.search import VideoIndex
  q, qw, g, gw = _data(70, 131, 9, 16, 64)
  index = VideoIndex(g, gw, dtype=dtype)
  scores = _scores(index, q, qw)
  for k in (10, 32):
    _check_lists(index.reverse_search(q, qw, k=k), scores, k)


# ---- 2. ties ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', DTYPES3, ids=IDS3)
def test_ties_go_by_ascending_row_and_scores_have_the_bits_of_search(dtype):
  from mmt_amd.search import VideoIndex
  nq, nv = 70, 130
  q, qw, g, gw = _data(nq, nv, 21)
  q[3], qw[3] = 2 * g[10], gw[10]                               # row 3 pulls hard on item 10 ...
  for twin in (5, 69):                                          # ... and so do its copies, one of them in the next block
    q[twin], qw[twin] = q[3], qw[3]
  gw[1] = 0                                                     # an item without weights: every score on it is 0
  qw[7] = 0                                                     # a row without weights: it scores 0 on every item
  index = VideoIndex(g, gw, dtype=dtype)
  scores = _scores(index, q, qw)
  assert not scores[:, 1].any() and not scores[7].any()
  assert _bits(scores[3]).tolist() == _bits(scores[5]).tolist() == _bits(scores[69]).tolist()   # identical rows, identical bits
  above = (scores > 0).sum(0)                                   # an item on which 1 .. 31 rows score positive and the others
  mixed = int(np.flatnonzero((above >= 1) & (above <= 31))[0])  # negative: row 7, at 0, ranks between them, inside the list
  assert mixed not in (1, 10) and (scores[:, mixed] < 0).sum() == nq - 1 - above[mixed]
  for k in KS:
    got = index.reverse_search(q, qw, k=k)
    _check_lists(got, scores, k)
    s, r = got[0].cpu().numpy(), got[1].cpu().numpy()
    assert r[1].tolist() == list(range(k)) and not s[1].any()   # the all-zero item: rows 0 .. k' - 1
    assert r[10, :min(k, 3)].tolist() == [3, 5, 69][:k]         # equal scores by ascending row
    # a score has the bits `search` returns for the pair: per item, search(subset = that item, k = 1) scores every row on it
    for item in (1, 10, mixed, nv - 1):
      pair = index.search(q, qw, k=1, subset=index.subset(_cuda(np.array([item]))))[0][:, 0].cpu().numpy()
      assert np.array_equal(_bits(s[item]), _bits(pair[r[item]])), (k, item)
  want_r = _reverse(scores, 32)[1]
  assert want_r[mixed].tolist().index(7) == above[mixed]        # the zero row sits between the positive and the negative


# ---- 3. a list depends on its item and the query rows only ------------------------------------------------------------

@pytest.mark.parametrize('dtype', DTYPES3, ids=IDS3)
def test_lists_do_not_depend_on_the_batching_or_the_layout(dtype, monkeypatch):
  from mmt_amd import search
  from mmt_amd.search import VideoIndex
  nq, nv = 300, 130
  q, qw, g, gw = _data(nq, nv, 33)
  index = VideoIndex(g, gw, dtype=dtype)
  scores = _scores(index, q, qw)
  for k in (10, 32):
    want = index.reverse_search(q, qw, k=k)                     # the default takes the rows in one batch
    _check_lists(want, scores, k)
    want_r = index.csls_norm(q, qw, k=k).lse if dtype != FP8 else None
    per_row = M * D * 4 + -(-8 * k * nv // 64)                  # the folded row and its share of the block's lists
    for rows in (64, 128):
      monkeypatch.setattr(search, '_BATCH_BYTES', rows * per_row)
      assert index._row_batches(nq, -(-8 * k * nv // 64))[0] == (0, rows)
      assert _same(index.reverse_search(q, qw, k=k), want), (k, rows)
      if want_r is not None:
        assert np.array_equal(_bits(index.csls_norm(q, qw, k=k).lse), _bits(want_r)), (k, rows)
    monkeypatch.undo()
  # the 4-D text layout numbers its rows b * C + c
  q4 = q.reshape(nq // 5, 5, M, D).permute(0, 2, 1, 3).contiguous()
  assert _same(index.reverse_search(q4, qw.reshape(nq // 5, 5, M), k=10), index.reverse_search(q, qw, k=10))


@pytest.mark.parametrize('dtype', DTYPES3, ids=IDS3)
def test_lists_do_not_depend_on_the_position_or_the_index_size(dtype):
  from mmt_amd.search import VideoIndex
  nq, nv, m = 130, 8193, 2
  q, qw, g, gw = _data(nq, nv, 41, m, D)
  big = VideoIndex.empty(9000, m, D, DEV, dtype=dtype)          # spare capacity, filled in two pieces
  big.add(g[:5000], gw[:5000])
  big.add(g[5000:], gw[5000:])
  want = big.reverse_search(q, qw, k=10)
  rng = np.random.default_rng(3)
  edges = [0, 127, 128, 4095, 4096, 8192]
  sample = np.concatenate([edges, rng.choice(np.setdiff1d(np.arange(nv), edges), 194, replace=False)])
  sample = _cuda(rng.permutation(sample))                       # 200 items in another order, at other positions, another NV
  small = VideoIndex(g[sample], gw[sample], dtype=dtype)
  got = small.reverse_search(q, qw, k=10)
  _check_lists(got, _scores(small, q, qw), 10)
  assert _same(got, tuple(t[sample] for t in want))


# ---- 4. sharded ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', DTYPES3, ids=IDS3)
@pytest.mark.parametrize('n_shards,pieces', [(1, None), (3, (300, 129, 271)), (5, (1, 2, 650, 47))], ids=['1', '3-adds', '5-adds'])
def test_sharded_equals_the_single_index_bit_for_bit(n_shards, pieces, dtype):
  from mmt_amd.search import ShardedHubNorm, ShardedVideoIndex, VideoIndex
  nq, nv = 65, 700
  q, qw, g, gw, b, bw = _hubby(nq, nv, NB, 5, M, D)
  g[nv - 1], gw[nv - 1] = g[0], gw[0]
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
  for k in KS:
    want = mono.reverse_search(q, qw, k=k)
    assert _same(shard.reverse_search(q, qw, k=k), want), k
  _check_lists(want, _scores(mono, q, qw), 32)
  if dtype == FP8:
    with pytest.raises(ValueError, match='float8_e4m3fn'):
      shard.csls_norm(b, bw)
    return
  for dynamic in (False, True):
    norm_m = mono.csls_norm(b, bw, k=10, dynamic=dynamic)
    norm_s = shard.csls_norm(b, bw, k=10, dynamic=dynamic)
    assert isinstance(norm_s, ShardedHubNorm)
    assert (norm_s.beta, norm_s.bank_size, norm_s.num_items, norm_s.device, norm_s.kind, norm_s.k) == (2.0, NB, nv, DEV, 'csls', 10)
    assert np.array_equal(_bits(norm_s.lse), _bits(norm_m.lse))
    assert (norm_s.hubs is None) == (not dynamic) and (not dynamic or torch.equal(norm_s.hubs, norm_m.hubs))
    for s, sh in enumerate(shard.shards):
      if sh.num_items:
        assert np.array_equal(_bits(norm_s.parts[s].lse), _bits(norm_m.lse[sh.ids[:sh.num_items]]))
        assert (norm_s.parts[s].kind, norm_s.parts[s].k, norm_s.parts[s].beta) == ('csls', 10, 2.0)
    assert _same(shard.search(q, qw, k=10, norm=norm_s), mono.search(q, qw, k=10, norm=norm_m)), dynamic
  with pytest.raises(ValueError, match='ShardedVideoIndex.hub_norm'):
    shard.search(q, qw, norm=norm_m)


# ---- 5. csls_norm -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('nb', [1, 63, 65, 300])
def test_csls_term_is_the_mean_of_the_reverse_list(nb, dtype):
  """.lse is bit-equal to the float32 chain on the device's own reverse lists, and within 2^-23 (k' + 1) mean|s_i| + 2^-149
  of the fp64 mean of the k' largest entries of the item's column of S (derived in tests/test_index_reverse_cpu.py)."""
  from mmt_amd.search import HubNorm, VideoIndex
  nv = 130
  q, qw, g, gw, b, bw = _hubby(1, nv, nb, 7 * nb, M, D)
  index = VideoIndex(g, gw, dtype=dtype)
  bank = _scores(index, b, bw)
  top1 = index.search(b, bw, k=1)[1][:, 0]
  for k in KS:
    norm = index.csls_norm(b, bw, k=k)
    assert isinstance(norm, HubNorm)
    assert (norm.beta, norm.kind, norm.k, norm.bank_size, norm.num_items, norm.device) == (2.0, 'csls', k, nb, nv, DEV)
    assert norm.hubs is None and norm.lse.shape == (nv,) and norm.lse.dtype == torch.float32 and norm.lse.device == DEV
    lists = index.reverse_search(b, bw, k=k)[0].cpu().numpy()
    assert np.array_equal(_bits(norm.lse), _bits(csls_r32(lists))), k
    best = -np.sort(-bank.T.astype(np.float64), axis=1)[:, :min(k, nb)]
    err = np.abs(norm.lse.cpu().numpy().astype(np.float64) - best.mean(1))
    bound = csls_bound(best)
    print('nb=%d k=%d: max err %.3e, max err / bound %.3f' % (nb, k, err.max(), (err / bound).max()))
    assert (err <= bound).all(), (k, (err / bound).max())
    dyn = index.csls_norm(b, bw, k=k, dynamic=True)
    assert np.array_equal(_bits(dyn.lse), _bits(norm.lse)) and (dyn.kind, dyn.k) == ('csls', k)
    assert torch.equal(dyn.hubs, torch.zeros(nv, device=DEV, dtype=torch.bool).index_fill_(0, top1, True))
  if nb % 5 == 0:                                               # the 4-D text layout of the bank is the same bank
    b4 = b.reshape(nb // 5, 5, M, D).permute(0, 2, 1, 3).contiguous()
    assert np.array_equal(_bits(index.csls_norm(b4, bw.reshape(nb // 5, 5, M), k=32).lse), _bits(norm.lse))


def test_csls_norm_is_refused_on_an_fp8_index_and_checks_in_order():
  from mmt_amd.search import VideoIndex
  q, qw, g, gw = _data(4, 10, 1)
  with pytest.raises(ValueError, match='float8_e4m3fn'):
    VideoIndex(g, gw, dtype=FP8).csls_norm(q, qw)
  for index in (VideoIndex.empty(12, M, D, DEV), VideoIndex.empty(12, M, D, DEV, dtype=FP8)):
    with pytest.raises(ValueError, match='holds no items'):
      index.reverse_search(q, qw)
    index.add(g, gw)
    with pytest.raises(ValueError, match='NQ >= 1'):
      index.reverse_search(q[:0], qw[:0])
  with pytest.raises(ValueError, match='no queries'):
    VideoIndex(g, gw).csls_norm(q[:0], qw[:0])


# ---- 6. downstream under norm=csls --------------------------------------------------------------------------------------

_CACHE = {}


def _case(nq, nv, dtype):
  """One index, its queries, a CSLS norm (k = 10 over a bank of 70) and the expected matrices per (shape, dtype), computed
  once and shared: plain scores S and S' = corrected32(S, r, 2.0)."""
  key = (nq, nv, dtype)
  if key not in _CACHE:
    from mmt_amd.search import VideoIndex
    q, qw, g, gw, b, bw = _hubby(nq, nv, NB, nq + nv, M, D)
    index = VideoIndex(g, gw, dtype=dtype)
    norm = index.csls_norm(b, bw, k=10)
    plain = _scores(index, q, qw)
    fixed = corrected32(plain, norm.lse.cpu().numpy(), 2.0)
    for a in (plain, fixed):
      a.setflags(write=False)
    _CACHE[key] = (index, q, qw, norm, plain, fixed)
  return _CACHE[key]


def _same_lists(got, want_s, want_i):
  return np.array_equal(got[1].cpu().numpy(), want_i) and np.array_equal(_bits(got[0]), _bits(want_s))


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('nq,nv', SHAPES[2:], ids=['%dx%d' % s for s in SHAPES[2:]])
def test_scans_under_a_csls_norm_are_exact(nq, nv, dtype):
  index, q, qw, norm, plain, fixed = _case(nq, nv, dtype)
  every = np.ones(nv, bool)
  assert not np.array_equal(_bits(fixed), _bits(plain))
  assert not np.array_equal(stable_topk(fixed, every, None, 10)[1], stable_topk(plain, every, None, 10)[1])   # not ignored
  rng = np.random.default_rng(nv)
  allowed = _masks(nv, rng)                                     # empties whole 128-item tiles
  sub = index.subset(_cuda(allowed))
  ex = np.concatenate([stable_topk(fixed, allowed, None, 5)[1], rng.integers(-1, nv, (nq, 3))], 1)
  for k in (1, 10, 128):
    assert _same_lists(index.search(q, qw, k=k, norm=norm), *stable_topk(fixed, every, None, k)), k
    assert _same_lists(index.search(q, qw, k=k, subset=sub, norm=norm), *stable_topk(fixed, allowed, None, k)), k
    assert _same_lists(index.search(q, qw, k=k, subset=sub, exclude=_cuda(ex), norm=norm), *stable_topk(fixed, allowed, ex, k)), k
  want_s, want_i = stable_topk(fixed, every, None, 20)          # one after= page: columns 10 .. 19 of the list
  first = index.search(q, qw, k=10, norm=norm)
  page = index.search(q, qw, k=10, norm=norm, after=(first[0][:, -1].contiguous(), first[1][:, -1].contiguous()))
  assert _same_lists(page, want_s[:, 10:], want_i[:, 10:])
  for t in (1, 3):
    tg = rng.integers(0, nv, (nq, t))
    tg[:, 0] = nv // 2
    if t > 1:
      tg[rng.random((nq, t)) < 0.2] = -1
    tg_d = _cuda(tg)
    greater, equal = brute_counts(fixed, tg)
    got_g, got_e = index.rank_counts(q, qw, tg_d, norm=norm)
    assert np.array_equal(got_g.cpu().numpy(), greater) and np.array_equal(got_e.cpu().numpy(), equal), t
    greater, equal = brute_counts(fixed, tg, allowed)
    got_g, got_e = index.rank_counts(q, qw, tg_d, subset=sub, norm=norm)
    assert np.array_equal(got_g.cpu().numpy(), greater) and np.array_equal(got_e.cpu().numpy(), equal), t
    thr = index.target_scores(q, qw, tg_d, norm=norm)
    want_thr = np.take_along_axis(fixed, np.maximum(tg, 0), 1)
    assert np.array_equal(_bits(thr)[tg >= 0], _bits(want_thr)[tg >= 0]) and bool(torch.isnan(thr[tg_d < 0]).all())


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_dynamic_rule_row_by_row_under_a_csls_norm(dtype):
  from mmt_amd.search import VideoIndex
  nq, nv = 65, 129
  q, qw, g, gw, b, bw = _hubby(nq, nv, NB, 77, M, D, share=2.0)
  hub, c = nv // 2, g[nv // 2:nv // 2 + 1] / 3
  p = g[3:3 + nq - nq // 2]
  q[nq // 2:] = 4 * (p - (p * c).sum(2, keepdim=True) * c)      # the second half: orthogonal to c, the hub is not their top-1
  qw[nq // 2:] = gw[3:3 + nq - nq // 2]
  bw[1] = 0.5
  index = VideoIndex(g, gw, dtype=dtype)
  norm = index.csls_norm(b, bw, k=10, dynamic=True)
  static = index.csls_norm(b, bw, k=10)
  hubs = norm.hubs.cpu().numpy()
  assert hubs[hub] and not hubs.all() and static.hubs is None
  assert np.array_equal(_bits(norm.lse), _bits(static.lse))
  scores = _scores(index, q, qw)
  fixed = corrected32(scores, static.lse.cpu().numpy(), 2.0)
  every = np.ones(nv, bool)
  use = hubs[stable_topk(scores, every, None, 1)[1][:, 0]]      # the rule, from the plain matrix
  assert 0 < use.sum() < nq
  want_s, want_i = stable_topk(scores, every, None, 10)
  fix_s, fix_i = stable_topk(fixed, every, None, 10)
  want_s[use], want_i[use] = fix_s[use], fix_i[use]
  assert not np.array_equal(fix_i[use], stable_topk(scores, every, None, 10)[1][use])
  for kwargs in ({}, {'dynamic': True}):
    assert _same_lists(index.search(q, qw, k=10, norm=norm, **kwargs), want_s, want_i), kwargs
  assert _same_lists(index.search(q, qw, k=10, norm=norm, dynamic=False), fix_s, fix_i)
  tg = np.random.default_rng(1).integers(0, nv, (nq, 3))
  greater, equal = brute_counts(scores, tg)
  fix_g, fix_e = brute_counts(fixed, tg)
  greater[use], equal[use] = fix_g[use], fix_e[use]
  got_g, got_e = index.rank_counts(q, qw, _cuda(tg), norm=norm)
  assert np.array_equal(got_g.cpu().numpy(), greater) and np.array_equal(got_e.cpu().numpy(), equal)


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_indexed_metrics_with_csls_banks_on_the_golden_eval_set(dtype):
  """tests/golden/trainer_valid.npz with all captions as the text bank and all videos as the video bank, CSLS with
  bank_k = 10: the metrics equal cols2metrics of brute-force ranks on the corrected matrices."""
  from mmt_amd.metric import cols2metrics, retrieval_metrics_indexed, v2t_targets
  from mmt_amd.search import VideoIndex
  g, vid, vw, txt, tw = _golden()
  qm = g['query_masks']
  b, caps = qm.shape
  m = vid.shape[1]
  text4 = txt.reshape(b, caps, m, -1).transpose(0, 2, 1, 3)
  tw3 = g['text_weights']
  valid, targets = v2t_targets(qm, b, caps)
  rows = np.flatnonzero(valid)
  vid_d, vw_d = _cuda(vid).float(), _cuda(vw).float().reshape(b, m)
  txt_d, tw_d = _cuda(txt).float().reshape(b * caps, m, -1), _cuda(tw).float().reshape(b * caps, m)
  real, real_w = txt_d[_cuda(rows)].contiguous(), tw_d[_cuda(rows)].contiguous()

  def brute(index, q, qw, bank, tg):
    scores = _scores(index, q, qw)
    if bank is not None:
      scores = corrected32(scores, index.csls_norm(bank[0], bank[1], k=10).lse.cpu().numpy(), 2.0)
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

  banks = {'text_bank': (text4, tw3), 'video_bank': (vid, vw)}
  dev_banks = {'text_bank': (txt_d, tw_d), 'video_bank': (vid_d, vw_d)}
  plain = retrieval_metrics_indexed(vid, text4, vw, tw3, query_masks=qm, dtype=dtype)
  both = retrieval_metrics_indexed(vid, text4, vw, tw3, query_masks=qm, dtype=dtype, bank_norm='csls', bank_k=10, **banks)
  check(both, expected(dev_banks['text_bank'], dev_banks['video_bank']))
  assert not np.array_equal(both['t2v_metrics']['cols'], plain['t2v_metrics']['cols'])
  only_text = retrieval_metrics_indexed(vid, text4, vw, tw3, query_masks=qm, dtype=dtype, bank_norm='csls', text_bank=banks['text_bank'])
  check(only_text, expected(dev_banks['text_bank'], None))
  sharded = retrieval_metrics_indexed(vid, text4, vw, tw3, query_masks=qm, dtype=dtype, bank_norm='csls', devices=[DEV] * 3, **banks)
  check(sharded, both)


# ---- 7. memory ----------------------------------------------------------------------------------------------------------

def test_reverse_search_allocates_no_quadratic_buffer():
  """4096 rows against 8193 items: the score matrix would be 128 MiB.  Budget: the batch (its folded rows and its blocks'
  partial lists) within search._BATCH_BYTES = 48 MiB, plus 20 k bytes per item (the carried state 8 k, the outputs 12 k),
  plus 1 MiB of slack for the second folded batch that lives while the first is released and the allocator's rounding.  At
  k = 32 the rows go in three batches."""
  from mmt_amd import search
  from mmt_amd.search import VideoIndex
  nq, nv = 4096, 8193
  q, qw, g, gw = _data(nq, nv, 5)
  index = VideoIndex(g, gw)
  for k in (10, 32):
    assert len(index._row_batches(nq, -(-8 * k * nv // 64))) == (1 if k == 10 else 3)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    s, r = index.reverse_search(q, qw, k=k)
    torch.cuda.synchronize()
    growth = torch.cuda.max_memory_allocated() - base
    print('k=%d: allocator peak growth %.1f MiB' % (k, growth / 2 ** 20))
    assert growth < search._BATCH_BYTES + 20 * k * nv + (1 << 20) < nq * nv * 4, (k, growth)
    assert bool((s[:, 1:] <= s[:, :-1]).all()) and bool(((r >= 0) & (r < nq)).all())
    for item in (0, 4096, nv - 1):                              # spot checks against the plain search of one item
      pair = index.search(q, qw, k=1, subset=index.subset(_cuda(np.array([item]))))[0][:, 0]
      want = torch.sort(pair, descending=True, stable=True)
      assert torch.equal(r[item], want.indices[:k]) and torch.equal(s[item], want.values[:k]), (k, item)
