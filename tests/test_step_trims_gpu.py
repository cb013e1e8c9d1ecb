"""The four one-round launches of the training step whose exposed latency was trimmed, each against an fp64 reference
computed from the inputs exactly as the kernel sees them (bf16-rounded where the kernel reads bf16):

  1. mmt_wgrad_grouped with blocks of different lengths in one launch (a row-split item + a compact item): the
     longest-first block order must not change a single result;
  2. the phased 128x64 GEMM tile (18) whose epilogue operands are requested ahead of its last K-steps: K / 64 below, at and
     above the hoist distance, dead rows, the dropout mask;
  3. the small-batch text-head backward (th_bwd2 / th_bwd3 fetch their dy-independent operands ahead of the barriers);
  4. fused Adam (its streaming cache policy was measured: see elementwise.hip): every bit of p, m, v and both shadows.

Tolerances: an fp32 dot product of n terms, in any summation order, is within n * 2^-24 * sum|a||b| of the exact one
(Higham, Accuracy and Stability, 3.5: gamma_n = n u / (1 - n u), u = 2^-24); the tests use n * 2^-23 * sum|a||b|, twice
that, which also covers the two or three fp32 additions of an epilogue (bias, residual), each bounded by u times a
magnitude that sum|a||b| + |bias| + |res| dominates.  A bf16 output (8 significand bits) adds its rounding: at most
half an ulp, 2^-8 |value|."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
U23 = 2.0 ** -23


def _rand(shape, scale, seed, dtype=torch.float32):
  g = torch.Generator().manual_seed(seed)
  return (torch.randn(*shape, generator=g) * scale).to(dtype).to(DEV)


def _within(name, got, ref, tol):
  err = (got.double() - ref).abs()
  bad = err > tol
  assert not bool(bad.any()), '%s: %d elements off, worst err %.3e against tol %.3e' % (
      name, int(bad.sum()), float(err[bad].max()), float(tol[bad].min()))


# ---- 1. grouped weight gradients: a row-split item next to a compact one ------------------------------------------------
ROWS1, LIVE1, COMPACT1 = 256, 193, 65  # 193 = 3 units of 64 rows + 1 ragged row; 65 = 1 unit + 1 row


@pytest.fixture(scope='module')
def wgrad_case():
  a0, b0 = _rand((ROWS1, 128), 1.0, 1, torch.bfloat16), _rand((ROWS1, 128), 0.5, 2, torch.bfloat16)
  a1, b1 = _rand((128, 128), 1.0, 3, torch.bfloat16), _rand((128, 128), 0.5, 4, torch.bfloat16)
  a0[LIVE1:] = float('nan'); b0[LIVE1:] = float('nan')        # rows past the device row count must not be read into a sum
  a1[COMPACT1:] = float('nan'); b1[COMPACT1:] = float('nan')
  A0, B0, A1, B1 = a0[:LIVE1].double(), b0[:LIVE1].double(), a1[:COMPACT1].double(), b1[:COMPACT1].double()
  ref = dict(w0=A0.t() @ B0, w0_tol=LIVE1 * U23 * (A0.abs().t() @ B0.abs()), b0=A0.sum(0), b0_tol=LIVE1 * U23 * A0.abs().sum(0),
             w1=A1.t() @ B1, w1_tol=COMPACT1 * U23 * (A1.abs().t() @ B1.abs()), b1=A1.sum(0),
             b1_tol=COMPACT1 * U23 * A1.abs().sum(0))
  return (a0, b0, a1, b1), ref


def _run_wgrad(ops_in, splits):
  from mmt_amd import _lib, ops
  from mmt_amd._lib import MmtWgradGroup, check
  a0, b0, a1, b1 = ops_in
  out0, bias0 = torch.full((128, 128), 7.0, device=DEV), torch.full((128,), 7.0, device=DEV)
  out1, bias1 = torch.full((128, 128), 7.0, device=DEV), torch.full((128,), 7.0, device=DEV)
  slab, bslab = torch.full((splits, 128, 128), 7.0, device=DEV), torch.full((splits, 128), 7.0, device=DEV)
  nr = torch.tensor([LIVE1], device=DEV, dtype=torch.int32)
  g = MmtWgradGroup()
  g.count, g.rows, g.n_rows_dev = 2, ROWS1, nr.data_ptr()
  it = g.item[0]
  it.A, it.B, it.out, it.bias_out = a0.data_ptr(), b0.data_ptr(), out0.data_ptr(), bias0.data_ptr()
  it.lda, it.ldb, it.N, it.K2 = 128, 128, 128, 128
  if splits > 1:
    it.splits, it.slab, it.bias_slab = splits, slab.data_ptr(), bslab.data_ptr()
  it = g.item[1]
  it.A, it.B, it.out, it.bias_out = a1.data_ptr(), b1.data_ptr(), out1.data_ptr(), bias1.data_ptr()
  it.lda, it.ldb, it.N, it.K2, it.reserved = 128, 128, 128, 128, COMPACT1
  check(_lib.lib().mmt_wgrad_grouped(ctypes.byref(g), ops._stream()), 'mmt_wgrad_grouped')
  torch.cuda.synchronize()
  if splits > 1:  # the caller sums the slabs; here in fp64, so the sum adds no error of its own
    return slab.clone(), bslab.clone(), out1, bias1
  return out0[None].clone(), bias0[None].clone(), out1, bias1


@pytest.mark.parametrize('splits', [1, 2, 3, 4])
def test_wgrad_grouped_mixed_block_lengths(wgrad_case, splits):
  """One 128x128 item over 193 live rows of 256 (n_rows_dev), cut `splits` ways (3 -> per-split units 2, 2, 0: an empty
  slab), next to a compact item of reserved = 65 rows: results and bias sums against fp64, and two runs bit for bit."""
  ops_in, ref = wgrad_case
  slab, bslab, out1, bias1 = _run_wgrad(ops_in, splits)
  _within('split item', slab.double().sum(0), ref['w0'], ref['w0_tol'])
  _within('split bias', bslab.double().sum(0), ref['b0'], ref['b0_tol'])
  _within('compact item', out1, ref['w1'], ref['w1_tol'])
  _within('compact bias', bias1, ref['b1'], ref['b1_tol'])
  again = _run_wgrad(ops_in, splits)
  for x, y in zip((slab, bslab, out1, bias1), again):
    assert torch.equal(x, y)


def test_wgrad_grouped_listed_multi_tile():
  """A 256 x 384 item (6 tiles, patches of 2 x 3) cut 4 ways = 24 blocks of one unit next to a compact 128 x 256 item (2
  blocks of two units): the launch takes the longest-first order, the compact item moves to the front, and the remap
  inside the split item is a real permutation (24 blocks, 3 per XCD).  Every tile, slab and bias sum against fp64."""
  from mmt_amd import _lib, ops
  from mmt_amd._lib import MmtWgradGroup, check
  splits = 4
  a0, b0 = _rand((ROWS1, 256), 1.0, 5, torch.bfloat16), _rand((ROWS1, 384), 0.5, 6, torch.bfloat16)
  a1, b1 = _rand((128, 128), 1.0, 7, torch.bfloat16), _rand((128, 256), 0.5, 8, torch.bfloat16)
  a0[LIVE1:] = float('nan'); b0[LIVE1:] = float('nan'); a1[COMPACT1:] = float('nan'); b1[COMPACT1:] = float('nan')
  slab, bslab = torch.full((splits, 256, 384), 7.0, device=DEV), torch.full((splits, 256), 7.0, device=DEV)
  out0, bias0 = torch.full((256, 384), 7.0, device=DEV), torch.full((256,), 7.0, device=DEV)
  out1, bias1 = torch.full((128, 256), 7.0, device=DEV), torch.full((128,), 7.0, device=DEV)
  nr = torch.tensor([LIVE1], device=DEV, dtype=torch.int32)
  g = MmtWgradGroup()
  g.count, g.rows, g.n_rows_dev = 2, ROWS1, nr.data_ptr()
  it = g.item[0]
  it.A, it.B, it.out, it.bias_out = a0.data_ptr(), b0.data_ptr(), out0.data_ptr(), bias0.data_ptr()
  it.lda, it.ldb, it.N, it.K2, it.splits, it.slab, it.bias_slab = 256, 384, 256, 384, splits, slab.data_ptr(), bslab.data_ptr()
  it = g.item[1]
  it.A, it.B, it.out, it.bias_out = a1.data_ptr(), b1.data_ptr(), out1.data_ptr(), bias1.data_ptr()
  it.lda, it.ldb, it.N, it.K2, it.reserved = 128, 256, 128, 256, COMPACT1
  check(_lib.lib().mmt_wgrad_grouped(ctypes.byref(g), ops._stream()), 'mmt_wgrad_grouped')
  torch.cuda.synchronize()
  A0, B0, A1, B1 = a0[:LIVE1].double(), b0[:LIVE1].double(), a1[:COMPACT1].double(), b1[:COMPACT1].double()
  # split s of the 4 units covers rows [64 s, 64 s + 64): every slab on its own, then their sum
  for sp in range(splits):
    lo, hi = 64 * sp, min(64 * sp + 64, LIVE1)
    _within('slab %d' % sp, slab[sp], A0[lo:hi].t() @ B0[lo:hi], (hi - lo) * U23 * (A0[lo:hi].abs().t() @ B0[lo:hi].abs()))
    _within('bias slab %d' % sp, bslab[sp], A0[lo:hi].sum(0), (hi - lo) * U23 * A0[lo:hi].abs().sum(0))
  _within('compact item', out1, A1.t() @ B1, COMPACT1 * U23 * (A1.abs().t() @ B1.abs()))
  _within('compact bias', bias1, A1.sum(0), COMPACT1 * U23 * A1.abs().sum(0))
  assert bool((out0 == 7.0).all()) and bool((bias0 == 7.0).all())  # a split item writes its slabs only


# ---- 2. tile 18 (phased 128x64): epilogue operands requested before the K loop ends ------------------------------------
ALLOC2, LIVE2 = 256, 129


@pytest.mark.parametrize('N,K', [(64, 64), (64, 128), (64, 320), (128, 64), (128, 128), (128, 320)])
def test_phased_tile_epilogues(N, K):
  """K / 64 = 1, 2 (below the hoist distance of 3 K-steps) and 5; 129 live rows of 256 allocated: the second tile row has
  one live row, rows past it keep their sentinel."""
  from mmt_amd import ops
  from tests import dropout_ref as D
  a, b = _rand((ALLOC2, K), 1.0, 10 + K, torch.bfloat16), _rand((N, K), 0.3, 11 + N, torch.bfloat16)
  a[LIVE2:] = float('nan')
  bias, res = _rand((N,), 0.5, 12), _rand((ALLOC2, N), 1.0, 13)
  A, B = a[:LIVE2].double(), b.double()
  acc = A @ B.t()
  tol = K * U23 * (A.abs() @ B.abs().t() + bias.double().abs()[None] + res[:LIVE2].double().abs())
  nr = torch.tensor([LIVE2], device=DEV, dtype=torch.int32)
  kw = dict(m=LIVE2, n_rows_dev=nr, tile=18)

  def run(epi, dtype=torch.float32, **more):
    out = torch.full((ALLOC2, N), 9.0, device=DEV, dtype=dtype)
    ops.gemm_nt(a, b, out, epi, **kw, **more)
    torch.cuda.synchronize()
    assert bool((out[LIVE2:] == 9.0).all()), epi + ': dead rows were written'
    return out[:LIVE2]

  # ADD_F32
  _within('ADD_F32', run('ADD_F32', res=res), acc + res[:LIVE2].double(), tol)
  # BIAS_DROP_RES without dropout
  want = acc + bias.double()[None] + res[:LIVE2].double()
  _within('BIAS_DROP_RES p=0', run('BIAS_DROP_RES', bias=bias, res=res), want, tol)
  # BIAS_DROP_RES, p = 0.1, original row numbers + device seed: mask = the documented hash
  orow = torch.arange(ALLOC2, dtype=torch.int32, device=DEV) * 3 + 5
  seed = torch.tensor([77], dtype=torch.int32, device=DEV)
  thr, scale = ops.dropout_params(0.1)
  drop = dict(row_index=orow, drop_key=0x51f3, drop_p=0.1, seed_dev=seed)
  keep = torch.from_numpy(D.keep_rows(D.eff_key(0x51f3, 77), orow[:LIVE2].cpu().numpy(), N, thr)).to(DEV)
  dropped = run('BIAS_DROP_RES', bias=bias, res=torch.zeros_like(res), **drop) == 0.0  # over a zero residual: 0.0f exactly
  assert torch.equal(dropped, ~keep), 'dropout mask differs from the hash in %d places' % int((dropped == keep).sum())
  got = run('BIAS_DROP_RES', bias=bias, res=res, **drop)
  want = torch.where(keep, (acc + bias.double()[None]) * float(np.float32(scale)), torch.zeros_like(acc)) + res[:LIVE2].double()
  _within('BIAS_DROP_RES p=0.1', got, want, tol * float(np.float32(scale)) + U23 * want.abs())
  # BF16 with row dots: out to the fp32 bound + half a bf16 ulp; the dots against the bf16 numbers the kernel stored (64 terms each)
  src = _rand((ALLOC2, N), 1.0, 14, torch.bfloat16)
  dots = torch.full((ALLOC2, N // 64), 9.0, device=DEV)
  got = run('BF16', torch.bfloat16, dot_src=src, dot_out=dots)
  t32 = K * U23 * (A.abs() @ B.abs().t())
  _within('BF16', got, acc, t32 + 2.0 ** -8 * (acc.abs() + t32))
  g64, s64 = got.double().view(LIVE2, N // 64, 64), src[:LIVE2].double().view(LIVE2, N // 64, 64)
  _within('row dots', dots[:LIVE2], (g64 * s64).sum(-1), 64 * U23 * (g64 * s64).abs().sum(-1))
  assert bool((dots[LIVE2:] == 9.0).all())


@pytest.mark.parametrize('N,K', [(64, 64), (128, 128), (64, 320)])
def test_phased_tile_packed_rows(N, K):
  """The packed configuration of the step: M = the 384 allocated rows, n_rows_dev = 129 below it, NaN in every dead row
  of the A operand, the residual and the dot partner.  The hoisted residual / aux / row-index loads then touch dead rows
  INSIDE the matrix.  The kernel works on live tile ROWS (128 rows): rows 129..255 share a tile row with live row 128 and
  are computed from their (NaN) inputs, as they always were -- stores are guarded by M, not by the row count -- so what
  must hold is that no NaN reaches a live row, that the dead tile row 256..383 keeps its sentinel, and that the row dots
  (guarded by the row count) are written for live rows only."""
  from mmt_amd import ops
  alloc = 384
  a, b = _rand((alloc, K), 1.0, 40 + K, torch.bfloat16), _rand((N, K), 0.3, 41 + N, torch.bfloat16)
  bias, res = _rand((N,), 0.5, 42), _rand((alloc, N), 1.0, 43)
  src = _rand((alloc, N), 1.0, 44, torch.bfloat16)
  a[LIVE2:] = float('nan'); res[LIVE2:] = float('nan'); src[LIVE2:] = float('nan')
  A, B = a[:LIVE2].double(), b.double()
  acc = A @ B.t()
  t32 = K * U23 * (A.abs() @ B.abs().t())
  tol = t32 + K * U23 * (bias.double().abs()[None] + res[:LIVE2].double().abs())
  nr = torch.tensor([LIVE2], device=DEV, dtype=torch.int32)
  orow = torch.arange(alloc, dtype=torch.int32, device=DEV)

  def run(epi, dtype=torch.float32, **more):
    out = torch.full((alloc, N), 9.0, device=DEV, dtype=dtype)
    ops.gemm_nt(a, b, out, epi, n_rows_dev=nr, tile=18, live_rows=LIVE2, **more)
    torch.cuda.synchronize()
    assert bool((out[256:] == 9.0).all()), epi + ': the dead tile row was written'
    return out[:LIVE2]

  _within('ADD_F32', run('ADD_F32', res=res), acc + res[:LIVE2].double(), tol)
  _within('BIAS_DROP_RES', run('BIAS_DROP_RES', bias=bias, res=res, row_index=orow),
          acc + bias.double()[None] + res[:LIVE2].double(), tol)
  dots = torch.full((alloc, N // 64), 9.0, device=DEV)
  got = run('BF16', torch.bfloat16, dot_src=src, dot_out=dots)
  _within('BF16', got, acc, t32 + 2.0 ** -8 * (acc.abs() + t32))
  g64, s64 = got.double().view(LIVE2, N // 64, 64), src[:LIVE2].double().view(LIVE2, N // 64, 64)
  _within('row dots', dots[:LIVE2], (g64 * s64).sum(-1), 64 * U23 * (g64 * s64).abs().sum(-1))
  assert bool((dots[LIVE2:] == 9.0).all()), 'row dots of dead rows were written'


# ---- 3. text-head backward, small batches -------------------------------------------------------------------------------
@pytest.mark.parametrize('N', [1, 31, 32])
@pytest.mark.parametrize('M,d,K', [(1, 32, 32), (1, 32, 768), (1, 512, 32), (1, 512, 768), (7, 32, 32), (7, 32, 768),
                                   (7, 512, 32), (7, 512, 768)])
def test_text_heads_bwd_small(N, M, d, K):
  """The weight-gradient tiles of th_bwd2 / th_bwd3 (g_w2 = dx1^T y, g_w1 = dy^T text, g_b1 = column sums of dy) against
  fp64 products of the very fp32 operands the kernels read (dy, dx1 and y from the workspace): contraction over N rows,
  tolerance N * 2^-23 * sum|a||b|.  Every other gradient against fp64 autograd of the module, at the tolerance
  tests/test_text_heads_gpu.py states for the same chain (2e-5 + 2e-4 max|ref|): those kernels are unchanged."""
  from mmt_amd import _lib, ops
  from mmt_amd._lib import MmtTextHeads, MmtTextHeadsOpts, check
  from tests.test_text_heads_gpu import _close, _params, _reference
  L = _lib.lib()
  assert L.mmt_text_heads_fast(N, M, d, K) == 1
  C = 1
  training = int(N > 1)  # (batch statistics of one row do not exist: N = 1 runs on the running statistics)
  P = _params(M, d, K, seed=N + d + K)
  g = torch.Generator().manual_seed(5)
  text = torch.randn(N, K, generator=g).to(DEV)
  de, dtw = torch.randn(N, M, C, d, generator=g).to(DEV), torch.randn(N, C, M, generator=g).to(DEV)
  Pr = [{k: v.double().clone().requires_grad_(not k.startswith('running')) for k, v in p.items()} for p in P]
  tr = text.double().clone().requires_grad_(True)
  e_ref, tw_ref, _ = _reference(Pr, tr, tr, C, True, bool(training))
  ((e_ref * de.double()).sum() + (tw_ref * dtw.double()).sum()).backward()

  h = MmtTextHeads()
  G = [{k: torch.full_like(v, 7.0) for k, v in p.items() if not k.startswith('running')} for p in P]
  run = [dict(running_mean=p['running_mean'].clone(), running_var=p['running_var'].clone()) for p in P]
  w1_all = torch.cat([p['w1'] for p in P], 0).contiguous()
  for m, p in enumerate(P):
    for k in ('b1', 'w2', 'b2', 'bn_gamma', 'bn_beta', 'moe_w', 'moe_b'):
      getattr(h, k)[m] = p[k].data_ptr()
      getattr(h, 'g_' + k)[m] = G[m][k].data_ptr()
    h.w1[m] = w1_all[m * d:(m + 1) * d].data_ptr()
    h.g_w1[m] = G[m]['w1'].data_ptr()
    h.running_mean[m] = run[m]['running_mean'].data_ptr()
    h.running_var[m] = run[m]['running_var'].data_ptr()
  ws = torch.zeros(L.mmt_text_heads_workspace_floats(N, M, d), device=DEV)
  embds, tw = torch.zeros(N, M, C, d, device=DEV), torch.zeros(N, C, M, device=DEV)
  o = MmtTextHeadsOpts()
  check(L.mmt_text_heads_fwd(ctypes.byref(h), ops._p(text), None, N, C, M, d, K, 1, training, ops._p(ws), ops._p(embds), ops._p(tw),
                             ctypes.byref(o), ops._stream()), 'fwd')
  dtext = torch.full_like(text, 7.0)
  check(L.mmt_text_heads_bwd(ctypes.byref(h), ops._p(text), None, ops._p(w1_all), N, C, M, d, K, 1, training, ops._p(ws), ops._p(de),
                             ops._p(tw), ops._p(dtw), ops._p(dtext), None, ctypes.byref(o), ops._stream()), 'bwd')
  torch.cuda.synchronize()
  # workspace layout (texthead2.hip th_layout): y | x1 | mean | rstd | dyg (= dy after the backward) | dz (= dx1) | ...
  nmd, md = N * M * d, M * d
  y = ws[:nmd].view(N, M, d).double()
  dy = ws[2 * nmd + 2 * md:3 * nmd + 2 * md].view(N, M, d).double()
  dx1 = ws[3 * nmd + 2 * md:4 * nmd + 2 * md].view(N, M, d).double()
  t64 = text.double()
  for m in range(M):
    _within('g_w1[%d]' % m, G[m]['w1'], dy[:, m].t() @ t64, N * U23 * (dy[:, m].abs().t() @ t64.abs()))
    _within('g_b1[%d]' % m, G[m]['b1'], dy[:, m].sum(0), N * U23 * dy[:, m].abs().sum(0))
    _within('g_w2[%d]' % m, G[m]['w2'], dx1[:, m].t() @ y[:, m], N * U23 * (dx1[:, m].abs().t() @ y[:, m].abs()))
    for k in ('w1', 'b1', 'w2', 'b2', 'moe_w', 'moe_b', 'bn_gamma', 'bn_beta'):
      _close('g_%s[%d]' % (k, m), G[m][k].double(), Pr[m][k].grad, 2e-5, 2e-4)
  _close('dtext', dtext.double(), tr.grad, 2e-5, 2e-4)


# ---- 4. fused Adam ------------------------------------------------------------------------------------------------------
def test_fused_adam_matches_the_plain_kernel_bit_for_bit():
  """A 65 x 68 shadowed matrix (ragged 64x64 tiles both ways, row-major and transposed shadow) + a plain span of 4100
  elements (one full 4096-element unit + 4), two steps: p, m and v bit for bit what mmt_adam_step -- the plain kernel,
  same adam_update4 formula, default-policy accesses -- leaves on a copy, within test_optim_gpu.py's tolerance of
  torch.optim.Adam, and both shadows equal to the bf16 rounding of the updated master."""
  from mmt_amd import _lib, ops
  from mmt_amd._lib import MmtAdamSeg, check
  L = _lib.lib()
  rows, cols, span = 65, 68, 4100
  n = rows * cols + span
  p0, hyper = _rand((n,), 0.3, 20), (1e-2, 0.9, 0.999, 1e-8, 0.01)
  pf, mf, vf = p0.clone(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
  pp, mp, vp = p0.clone(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
  ref = torch.nn.Parameter(p0.clone())
  topt = torch.optim.Adam([ref], lr=hyper[0], betas=hyper[1:3], eps=hyper[3], weight_decay=hyper[4])
  dst = torch.full((rows, cols), 9.0, device=DEV, dtype=torch.bfloat16)
  dst_t = torch.full((cols, 72), 9.0, device=DEV, dtype=torch.bfloat16)
  segs = (MmtAdamSeg * 2)()
  segs[0].offset, segs[0].count, segs[0].dst, segs[0].dst_t = 0, rows * cols, dst.data_ptr(), dst_t.data_ptr()
  segs[0].rows, segs[0].cols, segs[0].dst_ld, segs[0].dst_t_ld = rows, cols, cols, 72
  segs[1].offset, segs[1].count = rows * cols, span
  segs_dev = torch.frombuffer(bytearray(bytes(segs)), dtype=torch.uint8).clone().to(DEV)
  step_store = torch.zeros(2, dtype=torch.int32, device=DEV)
  step_plain = torch.zeros(1, dtype=torch.int32, device=DEV)
  for step in range(2):
    g = _rand((n,), 0.1, 30 + step)
    check(L.mmt_adam_step_fused(ops._p(pf), ops._p(g), ops._p(mf), ops._p(vf), segs, ops._p(segs_dev), 2, *hyper,
                                ops._p(step_store), None, 1, ops._stream()), 'mmt_adam_step_fused')
    step_plain.add_(1)
    check(L.mmt_adam_step(ops._p(pp), ops._p(g), ops._p(mp), ops._p(vp), n, *hyper, ops._p(step_plain), None, ops._stream()),
          'mmt_adam_step')
    ref.grad = g.clone()
    topt.step()
    torch.cuda.synchronize()
    assert step_store.tolist() == [step + 1, 0]
    assert torch.equal(pf, pp) and torch.equal(mf, mp) and torch.equal(vf, vp), 'step %d' % step
    w16 = pf[:rows * cols].view(rows, cols).to(torch.bfloat16)
    assert torch.equal(dst, w16), 'row-major shadow'
    assert torch.equal(dst_t[:, :rows], w16.t()), 'transposed shadow'
    assert bool((dst_t[:, rows:] == 9.0).all()), 'transposed shadow: columns past the matrix were written'
  assert torch.allclose(pf, ref.detach(), rtol=2e-5, atol=2e-6), (pf - ref.detach()).abs().max().item()
