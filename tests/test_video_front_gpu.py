"""The video / text token front end (assemble.hip, video_front.h, and the copy of plan + cast that rides in the text heads'
launches, texthead2.hip) called directly through the C ABI and compared with plain references:

  plan, text plan : every output EXACT against tests/video_front_ref.py (itself checked against the oracle's dense token
                    assembly on the CPU, tests/test_video_front_ref_cpu.py)
  cast            : bit for bit against torch's fp32 -> bf16 conversion (round to nearest even on both sides)
  scatter fwd/bwd : float64 F.normalize (eps 1e-12) and its autograd, with an error bound DERIVED from the kernel's
                    operation count (see _fwd_bound / _bwd_bound), never tuned to what the kernel gives
  riders          : bit for bit against the stand-alone launches

Every output buffer is prefilled with a sentinel, so a write outside the documented live region shows."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import video_front_ref as R

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
ERR_ARG = -1
I_SENT = -77        # int32 outputs (rows are >= 0, dropped slots -1)
F_SENT = 123.5      # fp32 outputs
H_SENT = 0x5A5A     # bf16 outputs, as bits
U = 2.0 ** -24      # fp32 unit roundoff
EPS = 1e-12
PLAN_OUT = ('counts', 'cu_seqlens', 'n_rows', 'slot', 'row_index', 'type_ids', 'pos_ids', 'mask_bias', 'agg_row')
SRC_OUT = ('src_row', 'src_cnt', 'xsrc')
SLACK = 8           # guard elements behind every plan output: must keep the sentinel


def _L():
  from mmt_amd import _lib
  return _lib.lib()


def _stream():
  from mmt_amd import ops
  return ops._stream()


def _dev(a):
  return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _ptr(t):
  return None if t is None else t.data_ptr()


class _Experts:
  """Host arrays, their device copies and the MmtExpertIO table of one minibatch."""

  def __init__(self, ind, t, type_idx=None):
    from mmt_amd._lib import MmtExpertIO
    self.M = len(ind)
    self.B, self.T = ind[0].shape
    self.S = 1 + self.M * (self.T + 1)
    self.ind_h, self.t_h = ind, t
    self.type_idx = type_idx or [3 * e + 1 for e in range(self.M)]
    self.ind, self.t = [_dev(a) for a in ind], [_dev(a) for a in t]
    self.io = (MmtExpertIO * max(self.M, 17))()
    self.keep = []
    for e in range(self.M):
      self.io[e].ind, self.io[e].t, self.io[e].type_idx = self.ind[e].data_ptr(), self.t[e].data_ptr(), self.type_idx[e]

  def reference(self, pack, max_pos=R.MAX_POS):
    return R.video_plan_reference(self.ind_h, self.t_h, self.type_idx, max_pos, pack)


def _make(B, M, T, pattern, seed=0):
  return _Experts(R.make_ind(B, M, T, pattern, seed), R.make_times(B, M, T, R.MAX_POS, seed))


def _plan_bufs(B, M, T):
  n = B * (1 + M * (T + 1))
  size = dict(counts=B, cu_seqlens=B + 1, n_rows=1, slot=n, row_index=n, type_ids=n, pos_ids=n, agg_row=B * M, src_row=n,
              src_cnt=M, xsrc=M * B * T)
  bufs = {k: torch.full((v + SLACK,), I_SENT, dtype=torch.int32, device=DEV) for k, v in size.items()}  # + guard words
  bufs['mask_bias'] = torch.full((n + SLACK,), F_SENT, dtype=torch.float32, device=DEV)
  return bufs


def _src(bufs, null=None):
  from mmt_amd._lib import MmtVideoSrc
  s = MmtVideoSrc()
  for k in SRC_OUT:
    setattr(s, k, None if k == null else bufs[k].data_ptr())
  return s


def _plan(x, pack, bufs, seed=None, null=None, M=None, B=None, T=None, max_pos=R.MAX_POS):
  src = _src(bufs, null)
  args = [None if k == null else bufs[k].data_ptr() for k in PLAN_OUT]
  rc = _L().mmt_video_plan(x.io, x.M if M is None else M, x.B if B is None else B, x.T if T is None else T, pack, max_pos,
                           *args, _ptr(seed), None if null == 'src' else ctypes.byref(src), _stream())
  torch.cuda.synchronize()
  return rc


def _check_plan(bufs, ref, tag, fresh=True):
  """Live region exact; with `fresh` (buffers prefilled with the sentinel) nothing outside it was written."""
  B, M, T = ref['B'], ref['M'], ref['T']
  h = {k: v.cpu().numpy() for k, v in bufs.items()}
  n = ref['n_rows']

  def eq(name, got, want):
    assert np.array_equal(got, want), '%s: %s differs at %s' % (tag, name, np.flatnonzero(np.ravel(got != want))[:8])

  for k, v in h.items():
    eq('guard words behind ' + k, v[-SLACK:], np.full(SLACK, F_SENT if k == 'mask_bias' else I_SENT, v.dtype))
    h[k] = v[:-SLACK]
  eq('n_rows', h['n_rows'], [n])
  for k in ('counts', 'cu_seqlens', 'slot', 'agg_row', 'src_cnt'):
    eq(k, h[k], ref[k])
  for k in ('row_index', 'type_ids', 'pos_ids', 'src_row', 'mask_bias'):
    assert h[k].dtype == ref[k].dtype
    eq(k, h[k][:n], ref[k])
    if fresh:
      eq(k + ' past n_rows', h[k][n:], np.full(len(h[k]) - n, F_SENT if k == 'mask_bias' else I_SENT, h[k].dtype))
  xs = h['xsrc'].reshape(M, B * T)
  for e in range(M):
    k = int(ref['src_cnt'][e]) - B
    eq('xsrc[%d]' % e, xs[e, :k], ref['xsrc'][e])
    if fresh:
      eq('xsrc[%d] past src_cnt' % e, xs[e, k:], np.full(B * T - k, I_SENT, np.int32))


# ---- 1. token plan ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('pack', [1, 0])
@pytest.mark.parametrize('B,M,T', R.PLAN_SHAPES)
def test_video_plan_exact(B, M, T, pack):
  """mmt_video_plan, every output exact, on every validity pattern.  Paths by shape: (5,7,30) scan pass 1 only (S = 218),
  M > 4; (2,3,100) scan passes 1-2 (S = 304) and T > 64 lane loops; (2,16,40) scan passes 1-3 (S = 657), M = 16 > 4 with
  S > 256, the wave-per-expert loop wrapping four times; (70,2,3) B > 64 in the prefix count over earlier samples.
  pack = 1 also checks the host-side CENet.count_live_rows against the device n_rows."""
  from mmt_amd.model import CENet
  for pattern in R.PATTERNS:
    x = _make(B, M, T, pattern, seed=B + M)
    bufs = _plan_bufs(B, M, T)
    assert _plan(x, pack, bufs) == 0
    ref = x.reference(pack)
    _check_plan(bufs, ref, '%s pack=%d' % (pattern, pack))
    if pack:
      assert CENet.count_live_rows({e: torch.from_numpy(a) for e, a in enumerate(x.ind_h)}) == int(bufs['n_rows'][0].item())
    else:
      assert int(bufs['n_rows'][0].item()) == B * x.S
    if pattern == 'zeros':  # CLS + AGG rows only, every AGG masked
      mb = bufs['mask_bias'].cpu().numpy()[:ref['n_rows']]
      s = ref['row_index'] % x.S
      assert np.all(mb[(s > 0) & ((s - 1) % (T + 1) == 0)] == np.float32(-10000.0))
      if pack:
        assert ref['n_rows'] == B * (1 + M)


def test_video_plan_times():
  """features_t: negative -> 0, 2.7 -> 2 (truncation after the clamp), exactly max_pos, above it and 1e9 -> max_pos."""
  ind = [np.ones((2, 6), np.float32)]
  t = [np.asarray([[-1.0, 2.7, 32.0, 32.5, 40.0, 1e9], [-1e9, 0.999, 31.999, 5.0, -0.0, 33.0]], np.float32)]
  x = _Experts(ind, t)
  bufs = _plan_bufs(2, 1, 6)
  assert _plan(x, 1, bufs, max_pos=32) == 0
  assert bufs['pos_ids'][:16].cpu().tolist() == [0, 0, 0, 2, 32, 32, 32, 32, 0, 0, 0, 0, 31, 5, 0, 32]
  _check_plan(bufs, x.reference(1, 32), 'times')


@pytest.mark.parametrize('pack', [1, 0])
@pytest.mark.parametrize('B,M,T', [(3, 2, 5), (2, 3, 100)])
def test_video_plan_reuse(B, M, T, pack):
  """The same output buffers after a fuller batch: nothing stale in the live region (scan passes 1-2 at (2,3,100))."""
  bufs = _plan_bufs(B, M, T)
  full = _make(B, M, T, 'ones')
  assert _plan(full, pack, bufs) == 0
  _check_plan(bufs, full.reference(pack), 'first')
  for pattern in ('holes', 'first_empty', 'zeros'):
    sparse = _make(B, M, T, pattern, seed=7)
    assert _plan(sparse, pack, bufs) == 0
    _check_plan(bufs, sparse.reference(pack), 'reuse ' + pattern, fresh=False)


def test_video_plan_seed_bump():
  """seed_bump moves by exactly 1 per call, whatever B is; NULL is accepted (every other plan test passes it)."""
  seed = torch.tensor([41], dtype=torch.int32, device=DEV)
  for i, (B, M, T) in enumerate([(1, 1, 1), (3, 2, 5), (70, 2, 3)]):
    x = _make(B, M, T, 'holes')
    assert _plan(x, i % 2, _plan_bufs(B, M, T), seed=seed) == 0
    assert seed.item() == 42 + i
  assert _plan(x, 1, _plan_bufs(B, M, T), seed=None) == 0
  assert seed.item() == 44


def test_video_plan_argument_errors():
  B, M, T = 3, 2, 5
  x = _make(B, M, T, 'holes')
  big = _make(B, 17, T, 'ones')
  bufs = _plan_bufs(B, 17, T)
  seed = torch.tensor([5], dtype=torch.int32, device=DEV)
  before = {k: v.clone() for k, v in bufs.items()}
  assert _plan(x, 1, bufs, seed, M=0) == ERR_ARG
  assert _plan(big, 1, bufs, seed) == ERR_ARG          # M = 17 > MMT_MAX_EXPERTS
  assert _plan(x, 1, bufs, seed, T=0) == ERR_ARG
  assert _plan(x, 1, bufs, seed, B=0) == ERR_ARG
  assert _plan(x, 1, bufs, seed, max_pos=-1) == ERR_ARG
  for null in PLAN_OUT + SRC_OUT + ('src',):
    assert _plan(x, 1, bufs, seed, null=null) == ERR_ARG, null
  for field in ('ind', 't'):
    y = _make(B, M, T, 'holes')
    setattr(y.io[1], field, None)
    assert _plan(y, 1, bufs, seed) == ERR_ARG, field
  assert seed.item() == 5
  for k, v in bufs.items():
    assert torch.equal(v, before[k]), k
  assert _plan(x, 1, bufs, seed) == 0  # the same arguments, unbroken, are accepted
  assert seed.item() == 6


# ---- 2. cast -----------------------------------------------------------------------------------------------------------
def _planted():
  """+-0, +-inf, fp32 values exactly halfway between two bf16 neighbours (even and odd lower neighbour, both signs, two
  binades), 3.39e38 (just above the largest bf16, still rounds to it) and 3.4e38 (past the halfway point: rounds to inf)."""
  bits = np.asarray([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000,
                     0x40008000, 0x40018000, 0x7F7E8000, 0x7F7F8000], np.uint32).view(np.float32)
  return np.concatenate([bits, np.asarray([3.39e38, -3.39e38, 3.4e38, -3.4e38], np.float32)])


def _features(B, T, D, rng):
  feat = (rng.standard_normal((B, T, D)) * 10.0 ** rng.uniform(-3, 3, size=(B, T, 1))).astype(np.float32)
  mp = (rng.standard_normal((B, D)) * 3.0).astype(np.float32)
  sp = _planted()
  for a in (feat.reshape(-1), mp.reshape(-1)):
    reps = 3 if a.size >= 4 * len(sp) else 1
    for _ in range(reps):
      k = min(len(sp), a.size)
      a[rng.permutation(a.size)[:k]] = rng.permutation(sp)[:k]
  assert not np.isnan(feat).any() and not np.isnan(mp).any()
  return feat, mp


def _bind_cast(x, widths, rng, extra_rows=3):
  """Features, max-pooled rows and sentinel-filled X of every expert, bound into the expert table."""
  B, T = x.B, x.T
  x.feat_h, x.mp_h, x.xbuf, x.widths = [], [], [], widths
  for e, (D, Dpad) in enumerate(widths):
    feat, mp = _features(B, T, D, rng)
    fd, md = _dev(feat), _dev(mp)
    xb = torch.full((B * (T + 1) + extra_rows, Dpad), H_SENT, dtype=torch.int16, device=DEV)
    x.keep += [fd, md]
    x.feat_h.append(feat), x.mp_h.append(mp), x.xbuf.append(xb)
    io = x.io[e]
    io.feat, io.maxpool, io.x, io.D, io.Dpad, io.rows_pad = fd.data_ptr(), md.data_ptr(), xb.data_ptr(), D, Dpad, B * (T + 1)


def _cast(x, bufs):
  src = _src(bufs)
  rc = _L().mmt_video_cast(x.io, x.M, x.B, x.T, ctypes.byref(src), _stream())
  torch.cuda.synchronize()
  return rc


def _check_cast(x, ref, tag):
  B, T = x.B, x.T
  for e, (D, Dpad) in enumerate(x.widths):
    rows = torch.cat([torch.from_numpy(x.mp_h[e]), torch.from_numpy(x.feat_h[e]).reshape(B * T, D)[ref['xsrc'][e].astype(np.int64)]])
    cnt = int(ref['src_cnt'][e])
    assert rows.shape[0] == cnt
    want = torch.full((x.xbuf[e].shape[0], Dpad), H_SENT, dtype=torch.int16)
    want[:cnt] = 0
    want[:cnt, :D] = rows.to(torch.bfloat16).view(torch.int16)
    got = x.xbuf[e].cpu()
    bad = (got != want).nonzero()
    assert bad.numel() == 0, '%s: expert %d (D %d, Dpad %d): %d elements differ, first (row, col) %s' % (
        tag, e, D, Dpad, bad.shape[0], bad[0].tolist())


CAST_WIDTHS = [(1, 4), (6, 8), (130, 256), (128, 128), (300, 384), (2208, 2304)]


@pytest.mark.parametrize('pattern,pack', [('ones', 1), ('holes', 1), ('first_empty', 1), ('zeros', 1), ('holes', 0)])
def test_video_cast_bit_exact(pattern, pack):
  """mmt_video_cast with six widths as the experts of one call: the scalar branch (D % 4 != 0: 1, 6, 130), no pad (128),
  the vector branch with a pad tail that starts on a vector boundary (300 -> 384) and a wide expert (2208 -> 2304).
  'holes' / 'first_empty' / 'zeros' are the sparse plans (src_cnt well below B * (T + 1)); rows at and past src_cnt keep
  the sentinel, pad columns of live rows are zero."""
  B, T = 3, 5
  rng = np.random.RandomState(11)
  x = _make(B, len(CAST_WIDTHS), T, pattern, seed=2)
  _bind_cast(x, CAST_WIDTHS, rng)
  bufs = _plan_bufs(B, x.M, T)
  assert _plan(x, pack, bufs) == 0
  ref = x.reference(pack)
  _check_plan(bufs, ref, 'plan')
  assert _cast(x, bufs) == 0
  _check_cast(x, ref, '%s pack=%d' % (pattern, pack))


def test_video_cast_second_grid_pass():
  """B = 8, T = 64, one expert of (2208, 2304): 520 rows x 576 quads = 299 520 > the 262 144 quads one pass of the
  256 x 256-thread grid covers four at a time, so the cast's 4 * stride loop runs a second, partial pass."""
  B, T = 8, 64
  x = _make(B, 1, T, 'ones')
  _bind_cast(x, [(2208, 2304)], np.random.RandomState(12))
  bufs = _plan_bufs(B, 1, T)
  assert _plan(x, 1, bufs) == 0
  _check_plan(bufs, x.reference(1), 'plan')  # the row maps are verified before the cast dereferences them
  assert _cast(x, bufs) == 0
  _check_cast(x, x.reference(1), 'second pass')


def test_video_cast_argument_errors():
  B, T = 3, 5
  x = _make(B, 2, T, 'ones')
  _bind_cast(x, [(6, 8), (128, 128)], np.random.RandomState(13))
  bufs = _plan_bufs(B, 2, T)
  assert _plan(x, 1, bufs) == 0
  _check_plan(bufs, x.reference(1), 'plan')
  x.io[1].Dpad = 130
  assert _cast(x, bufs) == ERR_ARG
  x.io[1].Dpad = 128
  x.io[0].rows_pad = B * (T + 1) - 1
  assert _cast(x, bufs) == ERR_ARG
  for xb in x.xbuf:
    assert bool((xb == H_SENT).all())
  x.io[0].rows_pad = B * (T + 1)
  assert _cast(x, bufs) == 0
  _check_cast(x, x.reference(1), 'after errors')


# ---- 3 / 4. scatter ------------------------------------------------------------------------------------------------------
ZERO_ROW, TINY_ROW = 0, 1  # compact source rows of expert 0 (the AGG inputs of samples 0 and 1: always live)


def _bind_scatter(x, d, n_part0, rng):
  """y and y_part[0..] of every expert: positive fractions of an intended sum, so sum_k |part_k| ~ |y|.  Expert e has
  (n_part0 + e) % 3 extra parts.  Expert 0: source row 0 all zeros, source row 1 of norm 1e-13."""
  rows_pad = x.B * (x.T + 1)
  x.parts, x.dy, x.n_part = [], [], []
  for e in range(x.M):
    n_part = (n_part0 + e) % 3
    ysum = rng.standard_normal((rows_pad, d)) * 10.0 ** rng.uniform(-2, 2, size=(rows_pad, 1))
    if e == 0:
      ysum[ZERO_ROW] = 0.0
      ysum[TINY_ROW] *= 1e-13 / np.linalg.norm(ysum[TINY_ROW])
    frac = rng.uniform(0.2, 1.0, size=(n_part + 1, rows_pad, d))
    parts = [_dev(np.concatenate([frac[k] / frac.sum(0) * ysum, np.full((2, d), F_SENT)]).astype(np.float32))
             for k in range(n_part + 1)]  # + two guard rows
    dy = torch.full((rows_pad + 2, d), H_SENT, dtype=torch.int16, device=DEV)
    io = x.io[e]
    io.y, io.dy, io.n_part, io.rows_pad = parts[0].data_ptr(), dy.data_ptr(), n_part, rows_pad
    for k in range(n_part):
      io.y_part[k] = parts[1 + k].data_ptr()
    x.parts.append(parts), x.dy.append(dy), x.n_part.append(n_part)


def _gathered(x, ref):
  """Per live token row, float64: the summed source row y, a = sum_k |part_k|, (expert, source row, n_part); CLS: zeros."""
  n, d = ref['n_rows'], x.parts[0][0].shape[1]
  Y = [torch.stack([p.cpu().double() for p in ps]).sum(0) for ps in x.parts]
  A = [torch.stack([p.cpu().double().abs() for p in ps]).sum(0) for ps in x.parts]
  y, a = torch.zeros(n, d, dtype=torch.float64), torch.zeros(n, d, dtype=torch.float64)
  where = []
  for i in range(n):
    s = int(ref['row_index'][i]) % x.S
    if s == 0:
      where.append(None)
      continue
    e, r = (s - 1) // (x.T + 1), int(ref['src_row'][i])
    y[i], a[i] = Y[e][r], A[e][r]
    where.append((e, r, x.n_part[e]))
  return y, a, where


def _fwd_bound(y, a, yhat):
  """got_i = y_i * (1 / max(sqrt(sum_j y_j^2), eps)) with y the fp32 sum of up to three parts, a_i = sum_k |part_k,i|.
  Up to two fp32 adds per element put y_i off by <= 2u a_i.  The sum of squares is a chain of at most 16 sequential plus
  6 tree additions of products of such inputs, which puts the norm off by <= (2 + 1/2 + 22/2) u ||a||^2 / ||y|| to first
  order; then a correctly rounded sqrtf (u/2), a divide (u) and a multiply (u).  Altogether
  |got_i - yhat_i| <= (2 a_i + (16 ||a||_2^2 / ||y||_2^2) |y_i|) u / ||y||_2, which, with ||a|| >= ||y|| and rounded up
  to one constant, is the bound asserted: 32 u (a_i + |yhat_i| ||a||_2) / ||y||_2 (parts built as positive fractions keep
  ||a|| ~ ||y||, i.e. about 64 u |yhat_i|).  Below eps the divisor is the constant 1e-12 and the norm's error does not
  enter, so max(||y||_2, eps) in its place only tightens the expression (and keeps it finite for the all-zero row, where
  it is 0: exact)."""
  nrm = y.norm(dim=-1, keepdim=True).clamp_min(EPS)
  return 32.0 * U * (a + yhat.abs() * a.norm(dim=-1, keepdim=True)) / nrm


def _bwd_bound(y, g, yhat, want, n_part):
  """bf16 rounding of the result (2^-8 relative, twice the half-ulp) + the fp32 arithmetic of (g - yhat (yhat . g)) / |y|
  with y the sum of 1 + n_part parts: 64 u (1 + n_part) (|g_i| + |yhat_i| sum_j |g_j yhat_j|) / ||y||_2."""
  nrm = y.norm(dim=-1, keepdim=True).clamp_min(EPS)
  return 2.0 ** -8 * want.abs() + 64.0 * U * (1.0 + n_part) * (g.abs() + yhat.abs() * (g * yhat).abs().sum(-1, keepdim=True)) / nrm


def _worst(err, bound):
  ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float('inf')),
                                                                            torch.zeros_like(err)))
  return ratio.max().item()


def _rows(x):
  return x.B * x.S


def _scatter_case(d, n_part0, pack):
  B, M, T = 3, 2, 5
  x = _make(B, M, T, 'holes', seed=3)
  _bind_scatter(x, d, n_part0, np.random.RandomState(100 * d + 10 * n_part0 + pack))
  bufs = _plan_bufs(B, M, T)
  assert _plan(x, pack, bufs) == 0
  ref = x.reference(pack)
  _check_plan(bufs, ref, 'plan')
  return x, bufs, ref


@pytest.mark.parametrize('n_part', [0, 1, 2])
@pytest.mark.parametrize('d', [256, 512, 768, 1024])
def test_video_scatter_forward(d, n_part):
  """mmt_video_scatter on a packed and a dense plan: d = 256 / 512 / 768 (three of the four chunks) / 1024, n_part 0, 1
  and 2 (expert 0 has n_part, expert 1 (n_part + 1) % 3).  CLS rows exactly zero; the all-zero source row gives exactly
  zero and the row of norm 1e-13 gives y / 1e-12 (the eps branch of the normalise); rows at and past n_rows keep the
  sentinel.  The assertion message carries the worst error / bound of the case."""
  for pack in (1, 0):
    x, bufs, ref = _scatter_case(d, n_part, pack)
    n = ref['n_rows']
    feats = torch.full((_rows(x) + 2, d), F_SENT, dtype=torch.float32, device=DEV)
    src = _src(bufs)
    rc = _L().mmt_video_scatter(x.io, x.M, x.B, x.T, d, _ptr(bufs['n_rows']), _ptr(bufs['row_index']), ctypes.byref(src),
                                _ptr(feats), _stream())
    torch.cuda.synchronize()
    assert rc == 0
    got = feats.cpu().double()
    assert bool((got[n:] == F_SENT).all()), 'rows at and past n_rows were written'
    y, a, where = _gathered(x, ref)
    yhat = F.normalize(y, dim=-1, eps=EPS)
    cls = torch.tensor([w is None for w in where])
    zero = torch.tensor([w is not None and w[:2] == (0, ZERO_ROW) for w in where])
    tiny = torch.tensor([w is not None and w[:2] == (0, TINY_ROW) for w in where])
    assert cls.sum() == x.B and zero.sum() == 1 and tiny.sum() == 1
    assert bool((got[:n][cls] == 0).all()) and bool((got[:n][zero] == 0).all())
    assert torch.allclose(yhat[tiny], y[tiny] / EPS, rtol=1e-12, atol=0) and 0.09 < yhat[tiny].norm().item() < 0.11
    # the eps branch on the device output itself: y / 1e-12 up to two adds (2u a_i), the fp32 image of 1e-12, the divide
    # and the multiply (u |y_i| each) -- (2 a_i + 3 |y_i|) u / eps, rounded up to 4u (a_i + |y_i|) / eps
    eps_err = (got[:n][tiny] - y[tiny] / EPS).abs()
    assert bool((eps_err <= 4.0 * U * (a[tiny] + y[tiny].abs()) / EPS).all()), \
        'norm-1e-13 row is not y / 1e-12: %.3e' % eps_err.max()
    err, bound = (got[:n] - yhat).abs(), _fwd_bound(y, a, yhat)
    ratio = _worst(err, bound)
    print('scatter fwd d=%d n_part=%d pack=%d: worst error / bound = %.4f' % (d, n_part, pack, ratio))
    assert ratio <= 1.0, 'd=%d n_part=%d pack=%d: worst error / bound = %.4f' % (d, n_part, pack, ratio)


@pytest.mark.parametrize('n_part', [0, 1, 2])
@pytest.mark.parametrize('d', [256, 512, 768, 1024])
def test_video_scatter_backward(d, n_part):
  """mmt_video_scatter_bwd against float64 autograd through F.normalize of the summed parts, same cases as the forward
  (d = 768 and 1024, n_part 1 and 2 included).  The all-zero and the norm-1e-13 source row take the eps branch
  (nrm <= 1e-12): g / 1e-12.  'dY needs no zero fill': dy is prefilled with a sentinel bit pattern, none may remain in
  rows [0, src_cnt[e]) and every row past that still holds it.  The worst error / bound is dominated by the first term
  of the bound: bf16 rounding reaches 2^-8 relative at the bottom of a binade, so a ratio just under 1 is expected."""
  for pack in (1, 0):
    x, bufs, ref = _scatter_case(d, n_part, pack)
    n = ref['n_rows']
    g32 = torch.randn(_rows(x), d, generator=torch.Generator().manual_seed(d + n_part + pack))
    gdev = g32.to(DEV)
    src = _src(bufs)
    rc = _L().mmt_video_scatter_bwd(x.io, x.M, x.B, x.T, d, _ptr(bufs['n_rows']), _ptr(bufs['row_index']),
                                    ctypes.byref(src), _ptr(gdev), _stream())
    torch.cuda.synchronize()
    assert rc == 0
    y, a, where = _gathered(x, ref)
    g = g32[:n].double()
    leaf = y.clone().requires_grad_(True)
    F.normalize(leaf, dim=-1, eps=EPS).backward(g)
    want = leaf.grad.clone()
    yhat = F.normalize(y, dim=-1, eps=EPS)
    eps_rows = [i for i, w in enumerate(where) if w is not None and w[0] == 0 and w[1] in (ZERO_ROW, TINY_ROW)]
    assert len(eps_rows) == 2
    for i in eps_rows:  # the reference itself takes the eps branch there
      assert torch.allclose(want[i], g[i] / EPS, rtol=1e-12, atol=0)
      want[i] = g[i] / EPS
    got = torch.zeros_like(want)
    n_parts = torch.zeros(n, 1, dtype=torch.float64)
    dy = [t.cpu() for t in x.dy]
    seen = [set() for _ in range(x.M)]
    for i, w in enumerate(where):
      if w is None:
        want[i] = 0  # CLS: no source row
        continue
      e, r, n_parts[i, 0] = w
      got[i] = dy[e][r].view(torch.bfloat16).double()
      seen[e].add(r)
    for e in range(x.M):
      cnt = int(ref['src_cnt'][e])
      assert seen[e] == set(range(cnt)), 'every live source row belongs to exactly one live token'
      assert not bool((dy[e][:cnt] == H_SENT).any()), 'expert %d: sentinel left in a live dY row' % e
      assert bool((dy[e][cnt:] == H_SENT).all()), 'expert %d: a dY row past src_cnt was written' % e
    for i in eps_rows:  # the eps branch on the device output itself: bf16(g * (1 / 1e-12f)), i.e. g / 1e-12 up to the
      # bf16 rounding (2^-8) and the fp32 image of 1e-12, the divide and the multiply (3u, rounded up to 4u)
      w = g[i] / EPS
      assert bool(((got[i] - w).abs() <= (2.0 ** -8 + 4.0 * U) * w.abs()).all()), 'eps row %d is not g / 1e-12' % i
    err, bound = (got - want).abs(), _bwd_bound(y, g, yhat, want, n_parts)
    ratio = _worst(err, bound)
    print('scatter bwd d=%d n_part=%d pack=%d: worst error / bound = %.4f' % (d, n_part, pack, ratio))
    assert ratio <= 1.0, 'd=%d n_part=%d pack=%d: worst error / bound = %.4f' % (d, n_part, pack, ratio)


@pytest.mark.parametrize('d', [128, 384, 1280])
def test_video_scatter_rejects_width(d):
  x, bufs, ref = _scatter_case(256, 0, 1)
  feats = torch.full((_rows(x), 1280), F_SENT, dtype=torch.float32, device=DEV)
  src = _src(bufs)
  L = _L()
  assert L.mmt_video_scatter(x.io, x.M, x.B, x.T, d, _ptr(bufs['n_rows']), _ptr(bufs['row_index']), ctypes.byref(src),
                             _ptr(feats), _stream()) == ERR_ARG
  assert L.mmt_video_scatter_bwd(x.io, x.M, x.B, x.T, d, _ptr(bufs['n_rows']), _ptr(bufs['row_index']), ctypes.byref(src),
                                 _ptr(feats), _stream()) == ERR_ARG
  torch.cuda.synchronize()
  assert bool((feats == F_SENT).all()) and all(bool((t == H_SENT).all()) for t in x.dy)


# ---- 5. plan and cast riding in the text heads' launches -----------------------------------------------------------------
def _heads_params(M, d, K, seed):
  g = torch.Generator().manual_seed(seed)
  r = lambda *s, sc=1.0: (torch.randn(*s, generator=g) * sc).to(DEV)
  return [dict(w1=r(d, K, sc=K ** -0.5), b1=r(d, sc=0.1), w2=r(d, d, sc=d ** -0.5), b2=r(d, sc=0.1),
               bn_gamma=1.0 + r(d, sc=0.1), bn_beta=r(d, sc=0.1), moe_w=r(1, K, sc=K ** -0.5), moe_b=r(1, sc=0.1),
               running_mean=r(d, sc=0.1), running_var=(1.0 + 0.3 * torch.rand(d, generator=g)).to(DEV)) for _ in range(M)]


def _run_heads(P, text, C, front=None):
  """Forward of the small text-heads path (training, BatchNorm); front: MmtVideoFront to carry, or None."""
  from mmt_amd._lib import MmtTextHeads, MmtTextHeadsOpts
  L = _L()
  N, K = text.shape
  M, d = len(P), P[0]['w1'].shape[0]
  assert L.mmt_text_heads_fast(N, M, d, K)
  h = MmtTextHeads()
  run = [dict(running_mean=p['running_mean'].clone(), running_var=p['running_var'].clone()) for p in P]
  for m, p in enumerate(P):
    for k in ('w1', 'b1', 'w2', 'b2', 'bn_gamma', 'bn_beta', 'moe_w', 'moe_b'):
      getattr(h, k)[m] = p[k].data_ptr()
    h.running_mean[m], h.running_var[m] = run[m]['running_mean'].data_ptr(), run[m]['running_var'].data_ptr()
  out = dict(ws=torch.zeros(L.mmt_text_heads_workspace_floats(N, M, d), device=DEV),
             embds=torch.zeros(N // C, M, C, d, device=DEV), tw=torch.zeros(N // C, C, M, device=DEV),
             nbt=torch.full((M,), 5, dtype=torch.long, device=DEV))
  o = MmtTextHeadsOpts()
  o.num_batches_tracked = out['nbt'].data_ptr()
  if front is not None:
    o.video_front = ctypes.addressof(front)
  rc = L.mmt_text_heads_fwd(ctypes.byref(h), _ptr(text), None, N, C, M, d, K, 1, 1, _ptr(out['ws']), _ptr(out['embds']),
                            _ptr(out['tw']), ctypes.byref(o), _stream())
  torch.cuda.synchronize()
  assert rc == 0
  for m in range(M):
    out['running_mean%d' % m], out['running_var%d' % m] = run[m]['running_mean'], run[m]['running_var']
  return out


@pytest.mark.parametrize('do_cast', [1, 0])
def test_front_riding_in_text_heads_launches(do_cast):
  """th_fwd1_plan_kernel / th_fwd2_cast_kernel / th_fwd3_cast_kernel (texthead2.hip) on (B, M, T) = (2, 3, 100) with the
  widths (6, 8), (300, 384), (128, 128): scan passes 1-2, the cast's scalar branch, its pad tail and its split between two
  launches in one run.  Plan outputs and X bit for bit those of the stand-alone mmt_video_plan + mmt_video_cast on
  separate buffers; the text heads' outputs bit for bit those of the call without video_front; the seed word moves by
  exactly 1.  do_cast = 0: X stays untouched."""
  from mmt_amd._lib import MmtVideoFront
  B, M, T = 2, 3, 100
  widths = [(6, 8), (300, 384), (128, 128)]
  ind, t = R.make_ind(B, M, T, 'holes', seed=5), R.make_times(B, M, T, R.MAX_POS, seed=5)
  alone, ride = _Experts(ind, t), _Experts(ind, t)
  _bind_cast(alone, widths, np.random.RandomState(21))
  _bind_cast(ride, widths, np.random.RandomState(21))
  ref = alone.reference(1)
  # stand-alone
  bufs_a, seed_a = _plan_bufs(B, M, T), torch.tensor([9], dtype=torch.int32, device=DEV)
  assert _plan(alone, 1, bufs_a, seed=seed_a) == 0
  _check_plan(bufs_a, ref, 'stand-alone')
  if do_cast:
    assert _cast(alone, bufs_a) == 0
    _check_cast(alone, ref, 'stand-alone')
  # riding
  N, C, Mt, d, K = 8, 1, 2, 256, 768
  P = _heads_params(Mt, d, K, seed=31)
  text = torch.randn(N, K, generator=torch.Generator().manual_seed(32)).to(DEV)
  bufs_r, seed_r = _plan_bufs(B, M, T), torch.tensor([9], dtype=torch.int32, device=DEV)
  src = _src(bufs_r)
  f = MmtVideoFront()
  f.experts = ctypes.addressof(ride.io)
  f.M, f.B, f.T, f.pack, f.max_pos, f.do_cast = M, B, T, 1, R.MAX_POS, do_cast
  for k in PLAN_OUT:
    setattr(f, 'n_rows_dev' if k == 'n_rows' else k, bufs_r[k].data_ptr())
  f.seed_bump = seed_r.data_ptr()
  f.src = ctypes.addressof(src)
  with_front = _run_heads(P, text, C, f)
  plain = _run_heads(P, text, C, None)
  assert seed_a.item() == 10 and seed_r.item() == 10
  for k in bufs_a:
    assert torch.equal(bufs_a[k], bufs_r[k]), 'plan output %s differs from the stand-alone launch' % k
  for e in range(M):
    assert torch.equal(alone.xbuf[e], ride.xbuf[e]), 'X of expert %d differs from the stand-alone cast' % e
    if not do_cast:
      assert bool((ride.xbuf[e] == H_SENT).all())
  bits = lambda v: v.view(torch.int32) if v.dtype == torch.float32 else v
  for k in plain:
    if k != 'ws':  # the workspace is scratch between the launches, not an output
      assert torch.equal(bits(plain[k]), bits(with_front[k])), 'text heads: %s changes when the front rides along' % k
  assert plain['nbt'].tolist() == [6] * Mt and float(plain['embds'].abs().sum()) > 0


# ---- 6. text plan -------------------------------------------------------------------------------------------------------
TEXT_OUT = ('counts', 'cu_seqlens', 'n_rows', 'ids', 'types', 'pos', 'row_index', 'cls_rows')


def _text_bufs(B, W):
  size = dict(counts=B, cu_seqlens=B + 1, n_rows=1, ids=B * W + 3, types=B * W + 3, pos=B * W + 3, row_index=B * W + 3, cls_rows=B)
  return {k: torch.full((v,), I_SENT, dtype=torch.int32, device=DEV) for k, v in size.items()}


def _text_plan(inp, bufs, B, W, null=None):
  ins = [None if (k == null or inp[k] is None) else inp[k].data_ptr() for k in ('ids', 'types', 'pos', 'mask')]
  rc = _L().mmt_text_plan(*ins, B, W, *[bufs[k].data_ptr() for k in TEXT_OUT], _stream())
  torch.cuda.synchronize()
  return rc


def _masks(B, W, rng):
  lens = rng.randint(1, W + 1, size=B)
  prefix = (np.arange(W)[None, :] < lens[:, None]).astype(np.int64)
  interior = prefix * (rng.rand(B, W) < 0.7)
  interior[0, 0] = 0  # token 0 masked out: kept all the same
  other = interior * rng.choice([5, -1, 1, 1 << 40], size=(B, W))
  return dict(prefix=prefix, interior=interior.astype(np.int64), ones=np.ones((B, W), np.int64),
              zeros=np.zeros((B, W), np.int64), other_values=other.astype(np.int64))


@pytest.mark.parametrize('B,W', [(1, 1), (3, 20), (4, 256), (2, 257), (2, 600)])
def test_text_plan_exact(B, W):
  """mmt_text_plan, every output exact: W = 256 exactly one pass of text_pack_kernel, W = 257 one element into the second
  pass (W > 256), W = 600 three passes with a carry.  Masks: prefix, interior zeros, all ones, all zero (token 0 still
  kept, cls_rows points at it), values other than 1.  token_type_ids / position_ids given and NULL."""
  rng = np.random.RandomState(W)
  ids = rng.randint(0, 30522, size=(B, W)).astype(np.int64)
  ids[0, 0], ids[-1, -1] = 30521, 30521
  types = rng.randint(0, 2, size=(B, W)).astype(np.int64)
  pos = rng.randint(0, 512, size=(B, W)).astype(np.int64)
  for name, mask in _masks(B, W, rng).items():
    for with_tp in (True, False):
      tag = '%s %s' % (name, 'given' if with_tp else 'NULL')
      inp = dict(ids=_dev(ids), types=_dev(types) if with_tp else None, pos=_dev(pos) if with_tp else None, mask=_dev(mask))
      bufs = _text_bufs(B, W)
      assert _text_plan(inp, bufs, B, W) == 0
      ref = R.text_plan_reference(ids, types if with_tp else None, pos if with_tp else None, mask)
      h = {k: v.cpu().numpy() for k, v in bufs.items()}
      n = ref['n_rows']
      assert h['n_rows'][0] == n, tag
      for k in ('counts', 'cu_seqlens', 'cls_rows'):
        assert np.array_equal(h[k], ref[k]), '%s: %s' % (tag, k)
      for k in ('ids', 'types', 'pos', 'row_index'):
        assert np.array_equal(h[k][:n], ref[k]), '%s: %s' % (tag, k)
        assert np.all(h[k][n:] == I_SENT), '%s: %s written past n_rows' % (tag, k)
      if name == 'zeros':
        assert n == B and np.array_equal(h['row_index'][:n], np.arange(B) * W) and np.array_equal(h['cls_rows'], np.arange(B))


def test_text_plan_argument_errors():
  B, W = 3, 20
  rng = np.random.RandomState(1)
  z = lambda: _dev(rng.randint(0, 2, size=(B, W)).astype(np.int64))
  inp = dict(ids=z(), types=z(), pos=z(), mask=z())
  bufs = _text_bufs(B, W)
  before = {k: v.clone() for k, v in bufs.items()}
  for null in ('ids', 'mask'):
    assert _text_plan(inp, bufs, B, W, null=null) == ERR_ARG, null
  for k in TEXT_OUT:
    outs = [None if o == k else bufs[o].data_ptr() for o in TEXT_OUT]
    assert _L().mmt_text_plan(*[inp[i].data_ptr() for i in ('ids', 'types', 'pos', 'mask')], B, W, *outs, _stream()) == ERR_ARG, k
  assert _text_plan(inp, bufs, 0, W) == ERR_ARG
  assert _text_plan(inp, bufs, B, 0) == ERR_ARG
  torch.cuda.synchronize()
  for k, v in bufs.items():
    assert torch.equal(v, before[k]), k
  assert _text_plan(inp, bufs, B, W) == 0
