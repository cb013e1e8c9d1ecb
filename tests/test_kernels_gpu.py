"""GPU unit tests: every HIP kernel against a plain PyTorch fp32 reference of the same op."""
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu


def _dev():
  return torch.device('cuda:0')


def _rand(shape, scale=1.0, seed=0, dtype=torch.float32):
  g = torch.Generator(device='cpu').manual_seed(seed)
  return (torch.randn(*shape, generator=g) * scale).to(dtype).to(_dev())


def _close(name, got, want, atol, rtol):
  got, want = got.float(), want.float()
  err = (got - want).abs()
  tol = atol + rtol * want.abs()
  bad = err > tol
  if bad.any():
    idx = bad.nonzero()[:8].tolist()
    raise AssertionError('%s: %d/%d mismatches, max err %.4g (ref max %.4g); first bad idx %s; got %s want %s'
                         % (name, int(bad.sum()), bad.numel(), err.max().item(), want.abs().max().item(), idx,
                            got[bad][:4].tolist(), want[bad][:4].tolist()))


def _gelu(x):
  return x * 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0)))


@pytest.mark.parametrize('M,N,K,tile', [(256, 64, 64, 2), (384, 192, 128, 2), (256, 128, 64, 1),
                                        (512, 384, 256, 1), (7168, 1536, 512, 0), (7168, 512, 3072, 0)])
def test_gemm_nt_plain_and_bias(M, N, K, tile):
  from mmt_amd import ops
  a = _rand((M, K), seed=1, dtype=torch.bfloat16)
  b = _rand((N, K), 0.1, seed=2, dtype=torch.bfloat16)
  bias = _rand((N,), seed=3)
  ref = a.float() @ b.float().t()
  out = torch.zeros(M, N, device=_dev(), dtype=torch.bfloat16)
  ops.gemm_nt(a, b, out, 'BF16', tile=tile)
  _close('BF16', out, ref, 2e-2, 1e-2)
  o32 = torch.zeros(M, N, device=_dev(), dtype=torch.float32)
  ops.gemm_nt(a, b, o32, 'F32', tile=tile)
  _close('F32', o32, ref, 1e-3, 1e-4)
  ops.gemm_nt(a, b, o32, 'BIAS_F32', bias=bias, tile=tile)
  _close('BIAS_F32', o32, ref + bias, 1e-3, 1e-4)
  ops.gemm_nt(a, b, out, 'BIAS_BF16', bias=bias, tile=tile)
  _close('BIAS_BF16', out, ref + bias, 2e-2, 1e-2)


@pytest.mark.parametrize('tile', [1, 2])
def test_gemm_nt_fused_epilogues(tile):
  from mmt_amd import ops
  M, N, K = 384, 256, 192
  a = _rand((M, K), seed=4, dtype=torch.bfloat16)
  b = _rand((N, K), 0.1, seed=5, dtype=torch.bfloat16)
  bias = _rand((N,), seed=6)
  res = _rand((M, N), seed=7)
  ref = a.float() @ b.float().t()
  # bias + GELU (two outputs)
  pre = torch.zeros(M, N, device=_dev(), dtype=torch.bfloat16)
  act = torch.zeros_like(pre)
  ops.gemm_nt(a, b, pre, 'BIAS_GELU', bias=bias, out2=act, tile=tile)
  _close('gelu.pre', pre, ref + bias, 2e-2, 1e-2)
  _close('gelu.act', act, _gelu(pre.float()), 1e-2, 1e-2)
  # bias + residual (dropout off)
  z = torch.zeros(M, N, device=_dev(), dtype=torch.float32)
  ops.gemm_nt(a, b, z, 'BIAS_DROP_RES', bias=bias, res=res, tile=tile)
  _close('drop_res(p=0)', z, ref + bias + res, 1e-3, 1e-4)
  # dropout on: every element is either res or res + (acc+bias)/(1-p); keep rate ~ 0.9; deterministic
  ops.gemm_nt(a, b, z, 'BIAS_DROP_RES', bias=bias, res=res, drop_key=1234, drop_p=0.1, tile=tile)
  thr, sc = ops.dropout_params(0.1)
  kept = (z - res - (ref + bias) * sc).abs() < 1e-3 + 1e-4 * (ref + bias).abs() * sc
  dropped = (z - res).abs() < 1e-6
  assert bool((kept | dropped).all())
  rate = kept.float().mean().item()
  assert 0.88 < rate < 0.92, rate
  z2 = torch.zeros_like(z)
  ops.gemm_nt(a, b, z2, 'BIAS_DROP_RES', bias=bias, res=res, drop_key=1234, drop_p=0.1, tile=3 - tile)
  assert torch.equal(z == res, z2 == res)  # mask depends only on (key, element), not on the tiling
  # add fp32
  ops.gemm_nt(a, b, z, 'ADD_F32', res=res, tile=tile)
  _close('add_f32', z, ref + res, 1e-3, 1e-4)
  # dGELU + column sums
  aux = _rand((M, N), seed=8, dtype=torch.bfloat16)
  out = torch.zeros(M, N, device=_dev(), dtype=torch.bfloat16)
  colsum = torch.zeros((M + 127) // 128, N, device=_dev(), dtype=torch.float32)
  ops.gemm_nt(a, b, out, 'DGELU', aux=aux, colsum=colsum, tile=tile)
  x = aux.float().requires_grad_(True)
  _gelu(x).backward(ref)
  _close('dgelu', out, x.grad, 3e-2, 1.5e-2)
  _close('dgelu.colsum', colsum.sum(0), out.float().sum(0), 1e-2, 1e-4)


# The product library holds the tiles the dispatcher selects on its own: 13 / 14 / 18 (gemm2.hip), 21 (gemm3.hip), 24 / 25
# (gemm5.hip: 128x128 / 128x64).  The tiles that were measured and lost are gone from the source.
_PRODUCT_TILES = [13, 14, 18, 24, 25]


@pytest.mark.parametrize('tile', _PRODUCT_TILES)
@pytest.mark.parametrize('M,N,K', [(300, 256, 128), (777, 512, 192), (7168, 1536, 512), (3583, 512, 3072), (640, 512, 64)])
def test_gemm_nt_wide_tiles(tile, M, N, K):
  """gemm2.hip (128x128 / 128x64 tiles, 32x32x16 MFMA, LDS-staged epilogue) and gemm5.hip (tiles 24 / 25: persistent,
  wave-specialised 128x128 / 128x64): every epilogue."""
  _wide_tile_case(tile, M, N, K)


@pytest.mark.parametrize('tile', [24, 25])
@pytest.mark.parametrize('M,N,K,live', [(6976, 512, 3072, 3639), (6976, 512, 3072, 1), (7168, 1536, 512, 3001), (2048, 512, 256, 2048),
                                        (6976, 512, 3072, 6976)])
def test_persistent_gemm_on_packed_rows(tile, M, N, K, live):
  """gemm5.hip under token packing: the live row count is on the device, the grid is sized for the allocated rows.  Fewer live
  tiles than blocks (the last, partial round is spread over the eight XCDs), several tiles per block plus a partial round,
  one live row, every row live.  Tile rows past the live ones are not written; results agree with the 128x64 tile's."""
  from mmt_amd import ops
  R = ops.pad_rows(M)
  a = _rand((R, K), seed=61, dtype=torch.bfloat16)
  b = _rand((N, K), 0.05, seed=62, dtype=torch.bfloat16)
  bias, res = _rand((N,), seed=63), _rand((R, N), seed=64)
  nrd = torch.tensor([live], device=_dev(), dtype=torch.int32)
  edge = min(R, (live + 127) // 128 * 128)
  ref = a[:live].float() @ b.float().t()
  for epi, kw, dt in (('BIAS_DROP_RES', dict(bias=bias, res=res, drop_key=99, drop_p=0.1), torch.float32),
                      ('ADD_F32', dict(res=res), torch.float32), ('BF16', {}, torch.bfloat16)):
    got = torch.full((R, N), 7.0, device=_dev(), dtype=dt)
    want = torch.full((R, N), 7.0, device=_dev(), dtype=dt)
    ops.gemm_nt(a, b, got, epi, m=M, n_rows_dev=nrd, tile=tile, **kw)
    ops.gemm_nt(a, b, want, epi, m=M, n_rows_dev=nrd, tile=13, **kw)
    if dt == torch.float32:  # same K order and dropout mask; the epilogues may contract their fp32 arithmetic differently
      _close(epi + ' vs the 128x64 tile', got[:live], want[:live], 1e-5, 1e-5)
    else:
      _close(epi + ' vs the 128x64 tile', got[:live], want[:live], 1e-2, 1e-2)
    assert bool((got[edge:] == 7.0).all()), epi
    if epi == 'ADD_F32':
      _close('add_f32 vs fp32 reference', got[:live], ref + res[:live], 2e-3, 2e-4)


def test_a_removed_tile_id_is_an_argument_error():
  """A tile id that no kernel answers to (the removed lab tiles among them) is an argument error, not a silent fallback."""
  from mmt_amd import ops
  a = _rand((256, 64), seed=1, dtype=torch.bfloat16)
  b = _rand((128, 64), seed=2, dtype=torch.bfloat16)
  out = torch.zeros(256, 128, device=_dev(), dtype=torch.bfloat16)
  for tile in (3, 4, 5, 7, 10, 11, 12, 15, 16, 17, 19, 20, 22, 23):
    with pytest.raises(RuntimeError):
      ops.gemm_nt(a, b, out, 'BF16', tile=tile)


@pytest.mark.parametrize('tile', [15, 16, 17])
@pytest.mark.parametrize('M,N,K', [(300, 384, 128), (777, 576, 192), (3583, 3072, 512), (7168, 1536, 512)])
def test_gemm_nt_192_wide_tiles(tile, M, N, K):
  """The tiles with 192 output columns (256x192 / 128x192) are gone: on the shapes they served (N a multiple of 192), asking
  for one is an argument error for every epilogue family, raised before any launch -- the output is not touched."""
  from mmt_amd import ops
  R = ops.pad_rows(M)
  a = _rand((R, K), seed=21, dtype=torch.bfloat16)
  b = _rand((N, K), 0.1, seed=22, dtype=torch.bfloat16)
  bias, res = _rand((N,), seed=23), _rand((R, N), seed=24)
  for epi, kw, dt in (('BF16', {}, torch.bfloat16), ('BIAS_BF16', dict(bias=bias), torch.bfloat16),
                      ('BIAS_DROP_RES', dict(bias=bias, res=res), torch.float32), ('ADD_F32', dict(res=res), torch.float32)):
    out = torch.full((R, N), 7.0, device=_dev(), dtype=dt)
    with pytest.raises(RuntimeError):
      ops.gemm_nt(a, b, out, epi, m=M, tile=tile, **kw)
    assert bool((out == 7.0).all()), epi


@pytest.mark.parametrize('M,N,K', [(300, 256, 64), (777, 512, 128), (640, 256, 192), (3583, 3072, 512), (7168, 1536, 512),
                                   (2100, 1024, 1024)])
def test_gemm_nt_256x256_eight_phase_tile(M, N, K):
  """gemm3.hip (tile 21): 256x256 tiles, 8 waves in two groups a barrier apart, four phases per K-tile, LDS-DMA ring that
  is never drained; K-tile counts 1, 2, 3, 8, 16 exercise the prologue / tail wait counts.  Every epilogue."""
  _wide_tile_case(21, M, N, K)


def _wide_tile_case(tile, M, N, K):
  from mmt_amd import ops
  R = ops.pad_rows(M)
  a = _rand((R, K), seed=21, dtype=torch.bfloat16)
  b = _rand((N, K), 0.1, seed=22, dtype=torch.bfloat16)
  bias, res = _rand((N,), seed=23), _rand((R, N), seed=24)
  ref = a[:M].float() @ b.float().t()
  pre = torch.full((R, N), 7.0, device=_dev(), dtype=torch.bfloat16)
  act = torch.zeros_like(pre)
  ops.gemm_nt(a, b, pre, 'BIAS_GELU', m=M, bias=bias, out2=act, tile=tile)
  _close('gelu.pre', pre[:M], ref + bias, 2e-2, 1e-2)
  _close('gelu.act', act[:M], _gelu(pre[:M].float()), 1e-2, 1e-2)
  assert bool((pre[M:] == 7.0).all())  # rows beyond M are never written
  z = torch.zeros(R, N, device=_dev(), dtype=torch.float32)
  ops.gemm_nt(a, b, z, 'BIAS_DROP_RES', m=M, bias=bias, res=res, tile=tile)
  _close('drop_res(p=0)', z[:M], ref + bias + res[:M], 1e-3, 1e-4)
  z1 = torch.zeros_like(z)
  ops.gemm_nt(a, b, z, 'BIAS_DROP_RES', m=M, bias=bias, res=res, drop_key=77, drop_p=0.1, tile=tile)
  ops.gemm_nt(a, b, z1, 'BIAS_DROP_RES', m=M, bias=bias, res=res, drop_key=77, drop_p=0.1, tile=2)
  _close('dropout mask identical across tile shapes', z[:M], z1[:M], 1e-3, 1e-4)
  ops.gemm_nt(a, b, z, 'ADD_F32', m=M, res=res, tile=tile)
  _close('add_f32', z[:M], ref + res[:M], 1e-3, 1e-4)
  ops.gemm_nt(a, b, z, 'BIAS_F32', m=M, bias=bias, tile=tile)
  _close('bias_f32', z[:M], ref + bias, 1e-3, 1e-4)
  ops.gemm_nt(a, b, pre, 'BF16', m=M, tile=tile)
  _close('bf16', pre[:M], ref, 2e-2, 1e-2)
  aux = _rand((R, N), seed=25, dtype=torch.bfloat16)
  live = torch.tensor([M - 37], device=_dev(), dtype=torch.int32)
  colsum = torch.zeros((M + 127) // 128, N, device=_dev(), dtype=torch.float32)
  ops.gemm_nt(a, b, pre, 'DGELU', m=M, aux=aux, colsum=colsum, n_rows_dev=live, tile=tile)
  x = aux[:M].float().requires_grad_(True)
  _gelu(x).sum().backward()
  _close('dgelu', pre[:M - 37], (ref * x.grad)[:M - 37], 3e-2, 1.5e-2)
  _close('dgelu.colsum (live rows only)', colsum.sum(0), pre[:M - 37].float().sum(0), 2e-2, 2e-4)


@pytest.mark.parametrize('batch,M,N,K,trans', [(3, 6, 256, 768, False), (7, 32, 512, 512, False), (2, 300, 130, 6, True),
                                               (1, 33, 96, 1000, True)])
def test_sgemm_batched(batch, M, N, K, trans):
  """fp32 MFMA batched GEMM with generic strides (text heads): C = beta*C + A.B^T + bias."""
  from mmt_amd import ops
  As, Bs, Cs, refs, biases = [], [], [], [], []
  for i in range(batch):
    if trans:  # contraction index is the slow one (weight-gradient form)
      a, b = _rand((K, M), seed=30 + i), _rand((K, N), seed=40 + i)
      A, B = a.t(), b.t()
    else:
      a, b = _rand((M, K), seed=30 + i), _rand((N, K), seed=40 + i)
      A, B = a, b
    bias = _rand((N,), seed=50 + i)
    c = _rand((M, N), seed=60 + i)
    refs.append(0.5 * c.double() + A.double() @ B.double().t() + bias.double())
    As.append(a); Bs.append(b); Cs.append(c); biases.append(bias)
  if trans:
    ops.sgemm_batched(As, Bs, Cs, M, N, K, 1, M, 1, N, N, biases, beta=0.5)
  else:
    ops.sgemm_batched(As, Bs, Cs, M, N, K, K, 1, K, 1, N, biases, beta=0.5)
  for c, r in zip(Cs, refs):
    _close('sgemm', c, r.float(), 1e-4 * math.sqrt(K), 1e-5)


def test_gemm_nt_live_rows_and_colsum_mask():
  from mmt_amd import ops
  M, N, K = 512, 128, 64
  a = _rand((M, K), seed=9, dtype=torch.bfloat16)
  b = _rand((N, K), 0.1, seed=10, dtype=torch.bfloat16)
  aux = _rand((M, N), seed=11, dtype=torch.bfloat16)
  live = torch.tensor([200], device=_dev(), dtype=torch.int32)
  out = torch.full((M, N), 7.0, device=_dev(), dtype=torch.bfloat16)
  colsum = torch.zeros(4, N, device=_dev(), dtype=torch.float32)
  ops.gemm_nt(a, b, out, 'DGELU', aux=aux, colsum=colsum, n_rows_dev=live, tile=2)
  assert bool((out[256:] == 7.0).all())  # tiles beyond the live row count exit early
  _close('colsum live', colsum.sum(0), out[:200].float().sum(0), 1e-2, 1e-4)


@pytest.mark.parametrize('rows,N,K2,splits,live', [(256, 128, 128, 1, None), (448, 256, 128, 3, None),
                                                   (512, 128, 384, 4, 333), (7168, 512, 1536, 8, 6976)])
def test_gemm_tn_weight_gradient(rows, N, K2, splits, live):
  from mmt_amd import ops
  a = _rand((rows, N), seed=12, dtype=torch.bfloat16)
  b = _rand((rows, K2), 0.1, seed=13, dtype=torch.bfloat16)
  n = rows if live is None else live
  nr = None if live is None else torch.tensor([live], device=_dev(), dtype=torch.int32)
  if live is not None:  # garbage (incl. NaN) beyond the live rows must not leak in
    a[live:] = float('nan')
    b[live:] = float('nan')
  ref = a[:n].float().t() @ b[:n].float()
  got = ops.gemm_tn(a, b, splits=splits, n_rows_dev=nr)
  _close('tn', got, ref, 2e-3 * math.sqrt(n / 256.0), 2e-4)
  acc = torch.ones_like(got)
  ops.gemm_tn(a, b, splits=splits, n_rows_dev=nr, out=acc, accumulate=True)
  _close('tn accumulate', acc, ref + 1.0, 2e-3 * math.sqrt(n / 256.0), 2e-4)


def test_gemm_nt_grouped():
  """Seven ReduceDim-shaped GEMMs (different K) + bias in one launch."""
  from mmt_amd import ops
  M, R, N = 992, 1024, 512
  items, refs = [], []
  for i, K in enumerate([512, 384, 2048, 1024, 2304, 384, 128]):
    a = _rand((R, K), seed=90 + i, dtype=torch.bfloat16)
    b = _rand((N, K), 0.05, seed=100 + i, dtype=torch.bfloat16)
    bias = _rand((N,), seed=110 + i)
    out = torch.full((R, N), 3.0, device=_dev())
    items.append((a, b, out, bias))
    refs.append(a[:M].float() @ b.float().t() + bias)
  ops.gemm_nt_grouped(items, m=M)
  for (a, b, out, bias), r in zip(items, refs):
    _close('grouped gemm', out[:M], r, 2e-3, 2e-4)
    assert bool((out[M:] == 3.0).all())


@pytest.mark.parametrize('live', [None, 333])
def test_wgrad_grouped(live):
  """One launch for several dW = dY^T X (+ bias gradient = column sums of dY), incl. an un-padded output."""
  from mmt_amd import ops
  rows = 512
  shapes = [(256, 128, 128, 128), (128, 384, 128, 300), (384, 128, 384, 128)]  # (N, K2, N_out, K2_out)
  items, refs = [], []
  for i, (N, K2, n_out, k_out) in enumerate(shapes):
    a = _rand((rows, N), seed=70 + i, dtype=torch.bfloat16)
    b = _rand((rows, K2), 0.1, seed=80 + i, dtype=torch.bfloat16)
    if live is not None:  # garbage beyond the live rows must not leak in
      a[live:] = float('nan')
      b[live:] = float('nan')
    n = rows if live is None else live
    out = torch.full((n_out, k_out), 5.0, device=_dev())
    bias = torch.full((n_out,), 5.0, device=_dev()) if i != 2 else None
    items.append((a, b, out, bias))
    refs.append(((a[:n].float().t() @ b[:n].float())[:n_out, :k_out], a[:n].float().sum(0)[:n_out]))
  nr = None if live is None else torch.tensor([live], device=_dev(), dtype=torch.int32)
  ops.wgrad_grouped(items, rows, n_rows_dev=nr)
  for (a, b, out, bias), (rw, rb) in zip(items, refs):
    _close('wgrad', out, rw, 4e-3, 2e-4)
    if bias is not None:
      _close('bias grad', bias, rb, 1e-3, 1e-5)


@pytest.mark.parametrize('live', [None, 561, 64])
def test_wgrad_grouped_short_contraction(live):
  """A text-tower layer's weight gradients (432 tiles of 128x128 over <= 1024 rows: nine 64-row units, 1.7 tiles per CU)
  against torch -- full and ragged live rows, bias gradients, garbage beyond the live rows.  (r06 tried a one-group lock-step
  kernel at two blocks per CU for this shape: 39.4 us per launch against the phased kernel's 28.3, tower step 4.28 vs 4.16 ms;
  reverted, profiles/r06_experiments.txt.)"""
  from mmt_amd import ops
  rows, d, inter = 960, 768, 3072
  shapes = [(3 * d, d), (d, d), (inter, d), (d, inter)]  # (N, K2): dWqkv, dWo, dW1, dW2
  items, refs = [], []
  n = rows if live is None else live
  for i, (N, K2) in enumerate(shapes):
    a = _rand((1024, N), seed=170 + i, dtype=torch.bfloat16)
    b = _rand((1024, K2), 0.1, seed=180 + i, dtype=torch.bfloat16)
    a[n:] = float('nan')
    b[n:] = float('nan')
    out, bias = torch.full((N, K2), 5.0, device=_dev()), torch.full((N,), 5.0, device=_dev())
    items.append((a, b, out, bias))
    refs.append((a[:n].float().t() @ b[:n].float(), a[:n].float().sum(0)))
  nr = torch.tensor([n], device=_dev(), dtype=torch.int32)
  ops.wgrad_grouped(items, rows, n_rows_dev=nr)
  for (a, b, out, bias), (rw, rb) in zip(items, refs):
    _close('wgrad short', out, rw, 6e-3, 3e-4)
    _close('bias grad short', bias, rb, 2e-3, 1e-5)


@pytest.mark.parametrize('d', [256, 512, 1024])
def test_layernorm_fwd_bwd(d):
  from mmt_amd import ops
  R, rows = 256, 203
  z = _rand((R, d), 2.0, seed=14) + 0.5
  gamma = 1.0 + 0.1 * _rand((d,), seed=15)
  beta = 0.1 * _rand((d,), seed=16)
  h32, h16, mean, rstd = ops.ln_fwd(z, gamma, beta, 1e-12, rows=rows)
  zr = z[:rows].clone().requires_grad_(True)
  gr, br = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
  ref = torch.nn.functional.layer_norm(zr, (d,), gr, br, 1e-12)
  _close('ln.h32', h32[:rows], ref, 1e-5, 1e-5)
  _close('ln.h16', h16[:rows], ref, 2e-2, 1e-2)
  assert bool((h32[rows:] == 0).all())
  dout = _rand((R, d), seed=17)
  ref.backward(dout[:rows])
  dz, dy, dg, db, dbias = ops.ln_bwd(dout, z, mean, rstd, gamma, rows=rows)
  _close('ln.dz', dz[:rows], zr.grad, 2e-5, 1e-4)
  _close('ln.dy', dy[:rows], zr.grad, 2e-2, 1e-2)
  _close('ln.dgamma', dg, gr.grad, 1e-3, 1e-4)
  _close('ln.dbeta', db, br.grad, 1e-3, 1e-4)
  _close('ln.dbias', dbias, dy[:rows].float().sum(0), 1e-3, 1e-4)
  # dropout-before-LN mode: dy = mask * dz / (1-p), same mask as the GEMM epilogue would have drawn
  dz2, dy2, _, _, _ = ops.ln_bwd(dout, z, mean, rstd, gamma, rows=rows, drop_mode=1, drop_key=77, drop_p=0.1)
  assert torch.equal(dz2, dz)
  thr, sc = ops.dropout_params(0.1)
  kept = dy2[:rows].float() != 0
  _close('ln.dy drop', dy2[:rows].float(), dz[:rows] * sc * kept, 2e-2, 1e-2)
  assert 0.87 < kept.float().mean().item() < 0.93


def test_embedding_layernorm_fwd_bwd():
  from mmt_amd import ops
  R, rows, d = 256, 218, 512
  feats = _rand((R, d), seed=18)
  g = torch.Generator().manual_seed(19)
  tids = torch.randint(0, 19, (R,), generator=g).int().to(_dev())
  pids = torch.randint(0, 32, (R,), generator=g).int().to(_dev())
  temb, pemb = _rand((19, d), 0.05, seed=20), _rand((32, d), 0.05, seed=21)
  gamma = 1.0 + 0.1 * _rand((d,), seed=22)
  beta = 0.1 * _rand((d,), seed=23)
  z, h32, h16, mean, rstd = ops.embed_ln_fwd(feats, tids, pids, temb, pemb, gamma, beta, 1e-12, rows=rows)
  zr = (feats + temb[tids.long()] + pemb[pids.long()])[:rows]
  _close('emb.z', z[:rows], zr, 1e-6, 1e-6)
  _close('emb.h32', h32[:rows], torch.nn.functional.layer_norm(zr, (d,), gamma, beta, 1e-12), 1e-5, 1e-5)
  z2, h2, _, _, _ = ops.embed_ln_fwd(feats, tids, None, temb, None, gamma, beta, 1e-12, rows=rows)
  _close('emb.nopos', z2[:rows], (feats + temb[tids.long()])[:rows], 1e-6, 1e-6)
  # table gradient: segmented sum
  gsum = ops.table_grad(feats, tids, 19, rows=rows)
  ref = torch.zeros(19, d, device=_dev()).index_add_(0, tids[:rows].long(), feats[:rows])
  _close('table_grad', gsum, ref, 1e-4, 1e-5)
  # dropout-after-LN (mode 2): forward mask and backward mask agree
  _, hd, _, _, _ = ops.embed_ln_fwd(feats, tids, pids, temb, pemb, gamma, beta, 1e-12, rows=rows, drop_key=5,
                                    drop_p=0.1)
  keep = hd[:rows] != 0
  thr, sc = ops.dropout_params(0.1)
  _close('emb.drop', hd[:rows], h32[:rows] * sc * keep, 1e-5, 1e-5)
  dout = _rand((R, d), seed=24)
  dz_d, _, _, _, _ = ops.ln_bwd(dout, z, mean, rstd, gamma, rows=rows, drop_mode=2, drop_key=5, drop_p=0.1,
                                want_dy=False)
  dz_ref, _, _, _, _ = ops.ln_bwd(dout * keep_pad(keep, R) * sc, z, mean, rstd, gamma, rows=rows, want_dy=False)
  _close('emb.bwd mask', dz_d[:rows], dz_ref[:rows], 1e-5, 1e-5)


def keep_pad(keep, R):
  out = torch.zeros(R, keep.shape[1], device=keep.device)
  out[:keep.shape[0]] = keep.float()
  return out


def _attn_ref(qkv, bias, B, S, H, scale, cu=None, mask=None, sc=1.0):
  """fp32 reference of bert.py:141-168 on the bf16-rounded inputs; returns ctx [rows, d]."""
  d = qkv.shape[1] // 3
  dh = d // H
  out = torch.zeros(qkv.shape[0], d, device=qkv.device)
  for b in range(B):
    o, n = (b * S, S) if cu is None else (int(cu[b]), int(cu[b + 1] - cu[b]))
    x = qkv[o:o + n]
    q, k, v = (x[:, i * d:(i + 1) * d].reshape(n, H, dh).transpose(0, 1) for i in range(3))
    s = q @ k.transpose(1, 2) * scale + bias[o:o + n][None, None, :]
    p = torch.softmax(s, -1)
    if mask is not None:
      p = p * mask[b, :, :n, :n] * sc
    out[o:o + n] = (p @ v).transpose(0, 1).reshape(n, d)
  return out


@pytest.mark.parametrize('B,S,H,DH', [(2, 16, 2, 128), (3, 37, 2, 128), (2, 70, 4, 128), (2, 218, 4, 128), (1, 300, 2, 128),
                                      (3, 30, 12, 64), (2, 37, 4, 64), (2, 150, 8, 64)])
def test_attention_fwd_bwd_dense(B, S, H, DH):
  """DH = 128: every published video-BERT config; DH = 64: BERT-base (the text tower, 12 heads x 64)."""
  from mmt_amd import ops
  d = H * DH
  rows = B * S
  R = ops.pad_rows(rows)
  qkv = _rand((R, 3 * d), 1.0, seed=25, dtype=torch.bfloat16)
  g = torch.Generator().manual_seed(26)
  valid = (torch.rand(R, generator=g) > 0.3)
  valid[::S] = True
  bias = ((~valid).float() * -10000.0).to(_dev())
  scale = 1.0 / math.sqrt(float(DH))
  ctx, lse = ops.attn_fwd(qkv, bias, B, S, H, scale)
  x = qkv[:rows].float().requires_grad_(True)
  ref = _attn_ref(x, bias, B, S, H, scale)
  _close('attn.ctx', ctx[:rows], ref, 2e-2, 2e-2)
  dctx = _rand((R, d), seed=27, dtype=torch.bfloat16)
  ref.backward(dctx[:rows].float())
  dqkv = ops.attn_bwd(qkv, bias, ctx, lse, dctx, B, S, H, scale)
  for i, nm in enumerate('QKV'):
    _close('attn.d' + nm, dqkv[:rows, i * d:(i + 1) * d], x.grad[:, i * d:(i + 1) * d], 4e-2, 4e-2)


@pytest.mark.parametrize('DH', [128, 64])
def test_attention_dropout_replay_and_varlen(DH):
  from mmt_amd import ops
  B, S, H = 3, 50, 2
  d = H * DH
  scale = 1.0 / math.sqrt(float(DH))
  rows = B * S
  R = ops.pad_rows(rows)
  qkv = _rand((R, 3 * d), 1.0, seed=28, dtype=torch.bfloat16)
  bias = torch.zeros(R, device=_dev())
  bias[5:9] = -10000.0
  # dropout: export the mask the kernel draws and replay it through the reference
  mask = ops.attn_dropout_mask(B, H, S, 99, 0.1).float()
  assert 0.88 < mask.mean().item() < 0.92
  thr, sc = ops.dropout_params(0.1)
  ctx, lse = ops.attn_fwd(qkv, bias, B, S, H, scale, drop_key=99, drop_p=0.1)
  x = qkv[:rows].float().requires_grad_(True)
  ref = _attn_ref(x, bias, B, S, H, scale, mask=mask, sc=sc)
  _close('attn.drop ctx', ctx[:rows], ref, 2e-2, 2e-2)
  dctx = _rand((R, d), seed=29, dtype=torch.bfloat16)
  ref.backward(dctx[:rows].float())
  dqkv = ops.attn_bwd(qkv, bias, ctx, lse, dctx, B, S, H, scale, drop_key=99, drop_p=0.1)
  _close('attn.drop dqkv', dqkv[:rows], x.grad, 4e-2, 4e-2)
  # variable-length packing: three samples of 11, 50, 30 rows
  cu = torch.tensor([0, 11, 61, 91], dtype=torch.int32, device=_dev())
  ctx2, lse2 = ops.attn_fwd(qkv, bias, 3, 50, H, scale, cu_seqlens=cu)
  x2 = qkv[:91].float().requires_grad_(True)
  ref2 = _attn_ref(x2, bias, 3, 50, H, scale, cu=cu.cpu())
  _close('attn.varlen ctx', ctx2[:91], ref2, 2e-2, 2e-2)
  ref2.backward(dctx[:91].float())
  dqkv2 = ops.attn_bwd(qkv, bias, ctx2, lse2, dctx, 3, 50, H, scale, cu_seqlens=cu)
  _close('attn.varlen dqkv', dqkv2[:91], x2.grad, 4e-2, 4e-2)


@pytest.mark.parametrize('M,N,K,epi', [(224, 512, 3072, 'BIAS_DROP_RES'), (224, 512, 512, 'BF16'), (200, 1024, 6144, 'ADD_F32'),
                                       (77, 256, 192, 'F32')])
def test_gemm_nt_splitk(M, N, K, epi):
  """Skinny split-K GEMM (last-layer read-out rows): same results as the fused-epilogue GEMM, incl. the dropout mask."""
  from mmt_amd import ops
  R = ops.pad_rows(M)
  a = _rand((R, K), seed=120, dtype=torch.bfloat16)
  b = _rand((N, K), 0.05, seed=121, dtype=torch.bfloat16)
  bias, res = _rand((N,), seed=122), _rand((R, N), seed=123)
  rowidx = torch.arange(R, device=_dev(), dtype=torch.int32) * 3 + 5
  f32 = epi != 'BF16'
  want = torch.zeros(R, N, device=_dev(), dtype=torch.float32 if f32 else torch.bfloat16)
  got = torch.full((R, N), 9.0, device=_dev(), dtype=want.dtype)
  kw = dict(bias=bias, res=res, row_index=rowidx, drop_key=55, drop_p=0.1 if epi == 'BIAS_DROP_RES' else 0.0)
  ops.gemm_nt(a, b, want, epi, m=M, tile=2, **kw)
  ops.gemm_nt_splitk(a, b, got, epi, m=M, **kw)
  _close('splitk', got[:M], want[:M], 2e-2 if not f32 else 2e-3, 1e-2 if not f32 else 2e-4)
  assert bool((got[M:] == 9.0).all())


def test_wgrad_grouped_item_splits_and_row_override():
  """Per-item row override (compact operands) and per-item split-K slabs summed by mmt_col_reduce_multi."""
  import ctypes
  from mmt_amd import _lib, ops
  from mmt_amd._lib import MmtColReduceJob, MmtWgradGroup, check
  rows, live = 1024, 900
  a0, b0 = _rand((rows, 256), seed=130, dtype=torch.bfloat16), _rand((rows, 128), 0.1, seed=131, dtype=torch.bfloat16)
  a1, b1 = _rand((256, 128), seed=132, dtype=torch.bfloat16), _rand((256, 384), 0.1, seed=133, dtype=torch.bfloat16)
  a0[live:] = float('nan'); b0[live:] = float('nan')
  a1[200:] = float('nan'); b1[200:] = float('nan')
  out0, bias0 = torch.zeros(256, 128, device=_dev()), torch.zeros(256, device=_dev())
  out1, bias1 = torch.zeros(128, 384, device=_dev()), torch.zeros(128, device=_dev())
  splits = 4
  slab, bslab = torch.zeros(splits, 256, 128, device=_dev()), torch.zeros(splits, 256, device=_dev())
  nr = torch.tensor([live], device=_dev(), dtype=torch.int32)
  g = MmtWgradGroup()
  g.count, g.rows, g.n_rows_dev = 2, rows, nr.data_ptr()
  it = g.item[0]
  it.A, it.B, it.out, it.bias_out = a0.data_ptr(), b0.data_ptr(), out0.data_ptr(), bias0.data_ptr()
  it.lda, it.ldb, it.N, it.K2, it.splits, it.slab, it.bias_slab = 256, 128, 256, 128, splits, slab.data_ptr(), bslab.data_ptr()
  it = g.item[1]
  it.A, it.B, it.out, it.bias_out = a1.data_ptr(), b1.data_ptr(), out1.data_ptr(), bias1.data_ptr()
  it.lda, it.ldb, it.N, it.K2, it.reserved = 128, 384, 128, 384, 200
  check(_lib.lib().mmt_wgrad_grouped(ctypes.byref(g), ops._stream()), 'mmt_wgrad_grouped')
  jobs = (MmtColReduceJob * 2)()
  for j, (p, o, dd) in enumerate(((slab, out0, 256 * 128), (bslab, bias0, 256))):
    jobs[j].partials, jobs[j].nblocks, jobs[j].nvec, jobs[j].nout, jobs[j].d = p.data_ptr(), splits, 1, 1, dd
    jobs[j].out[0] = o.data_ptr()
  check(_lib.lib().mmt_col_reduce_multi(jobs, 2, ops._stream()), 'mmt_col_reduce_multi')
  _close('split item', out0, a0[:live].float().t() @ b0[:live].float(), 6e-3, 2e-4)
  _close('split bias', bias0, a0[:live].float().sum(0), 2e-3, 1e-5)
  _close('row-override item', out1, a1[:200].float().t() @ b1[:200].float(), 4e-3, 2e-4)
  _close('row-override bias', bias1, a1[:200].float().sum(0), 1e-3, 1e-5)


@pytest.mark.parametrize('M,N,K,tile', [(300, 512, 1536, 0), (777, 3072, 512, 14), (777, 3072, 512, 13), (1500, 1536, 768, 0),
                                        (130, 768, 2304, 0), (1100, 512, 3072, 0)])
def test_gemm_nn_input_gradient_form(M, N, K, tile):
  """C = A . W with W row-major [K, N] (a weight as stored, no transposed copy): every epilogue the backward uses."""
  from mmt_amd import ops
  R = ops.pad_rows(M)
  a = _rand((R, K), seed=140, dtype=torch.bfloat16)
  w = _rand((K, N), 0.05, seed=141, dtype=torch.bfloat16)
  ref = a[:M].float() @ w.float()
  out16 = torch.zeros(R, N, device=_dev(), dtype=torch.bfloat16)
  ops.gemm_nn(a, w, out16, 'BF16', m=M, tile=tile)
  _close('nn.bf16', out16[:M].float(), ref, 2e-2, 2e-2)
  out32 = torch.zeros(R, N, device=_dev())
  ops.gemm_nn(a, w, out32, 'F32', m=M, tile=tile)
  _close('nn.f32', out32[:M], ref, 2e-3, 2e-3)
  res = _rand((R, N), seed=142)
  ops.gemm_nn(a, w, out32, 'ADD_F32', m=M, res=res, tile=tile)
  _close('nn.add', out32[:M], ref + res[:M], 2e-3, 2e-3)
  aux = _rand((R, N), seed=143, dtype=torch.bfloat16)
  ops.gemm_nn(a, w, out16, 'DGELU', m=M, aux=aux, tile=tile)
  x = aux[:M].float().requires_grad_(True)
  (x * 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0)))).sum().backward()
  _close('nn.dgelu', out16[:M].float(), ref * x.grad, 3e-2, 3e-2)
  # live-row count on the device (token packing): rows past it are left untouched
  nr = torch.tensor([M // 2], device=_dev(), dtype=torch.int32)
  out32.fill_(7.0)
  ops.gemm_nn(a, w, out32, 'F32', m=M, n_rows_dev=nr, tile=tile)
  _close('nn.live', out32[:M // 2], ref[:M // 2], 2e-3, 2e-3)
  assert (out32[(M // 2 + 127) // 128 * 128:M] == 7.0).all()
  # split-K variant
  ops.gemm_nt_splitk(a, w, out32, 'ADD_F32', m=M, res=res, splits=3, b_kn=True)
  _close('nn.splitk', out32[:M], ref + res[:M], 2e-3, 2e-3)


def test_standalone_dropout_keep_rate_and_backward_mask():
  """mmt_dropout_f32 (the text MoE-logit dropout): keep rate p, survivors scaled by 1/(1-p), the backward re-draws the
  SAME mask from the saved key although the per-step seed has advanced in between, and a new seed gives a new mask."""
  from mmt_amd import ops
  from mmt_amd.model import _MoeDropoutFn
  _, sc = ops.dropout_params(0.1)  # 1 / (1 - p) for the 16-bit threshold actually used
  x = _rand((64, 768), seed=150).requires_grad_(True)
  seed = torch.tensor([1234], dtype=torch.int32, device=_dev())
  y = _MoeDropoutFn.apply(x, 0.1, seed)
  keep = y != 0
  assert 0.88 < keep.float().mean().item() < 0.92
  _close('dropout.scale', y[keep], (x * sc)[keep].detach(), 1e-6, 1e-6)
  seed.add_(1)  # the encoder advances the seed between forward and backward
  g = _rand((64, 768), seed=151)
  y.backward(g)
  _close('dropout.bwd', x.grad, g * keep * sc, 1e-6, 1e-6)
  y2 = _MoeDropoutFn.apply(x.detach(), 0.1, seed)
  assert ((y2 != 0) != keep).float().mean().item() > 0.05


@pytest.mark.parametrize('rows,d,v0,v1,live', [(3583, 512, 19, 32, None), (700, 256, 19, 32, 333), (900, 1024, 40, 64, 801),
                                                (257, 512, 19, 0, None), (2300, 512, 19, 102, 2101), (500, 256, 128, 65, None)])
def test_table_grad_pair_on_matrix_cores(rows, d, v0, v1, live):
  """Embedding-table gradients (token types + temporal positions, model/bert.py:87-105 backward) as one-hot products on the
  fp32 MFMA, both tables in one launch: against index_add_ in fp64."""
  from mmt_amd import _lib, ops
  from mmt_amd._lib import check
  L = _lib.lib()
  R = ops.pad_rows(rows)
  g = _rand((R, d), seed=61)
  gen = torch.Generator().manual_seed(62)
  ids0 = torch.randint(0, v0, (R,), generator=gen, dtype=torch.int32).to(_dev())
  ids1 = torch.randint(0, max(v1, 1), (R,), generator=gen, dtype=torch.int32).to(_dev()) if v1 else None
  nr = torch.tensor([live], device=_dev(), dtype=torch.int32) if live else None
  chunks = L.mmt_table_grad_chunks()
  s0 = torch.full((chunks, v0, d), 7.0, device=_dev())
  s1 = torch.full((chunks, v1, d), 7.0, device=_dev()) if v1 else None
  check(L.mmt_table_grad_partials_pair(ops._p(g), ops._p(ids0), v0, ops._p(s0), ops._p(ids1), v1, ops._p(s1), rows, d,
                                       ops._p(nr), ops._stream()), 'pair')
  n = live if live else rows
  for ids, v, s in ((ids0, v0, s0), (ids1, v1, s1)):
    if ids is None:
      continue
    want = torch.zeros(v, d, device=_dev(), dtype=torch.float64).index_add_(0, ids[:n].long(), g[:n].double())
    _close('table', s.sum(0), want.float(), 1e-4, 1e-5)


@pytest.mark.parametrize('DH', [128, 64])
def test_attention_dropout_is_keyed_on_original_positions(DH):
  """Token packing must not change which attention probabilities are dropped: the packed run (rows compacted, row_index
  = b*S + original position) draws exactly the mask of the dense run on the same tokens -- forward and backward."""
  from mmt_amd import ops
  B, S, H = 3, 70, 2
  d, scale = H * DH, 1.0 / math.sqrt(DH)
  rows = B * S
  R = ops.pad_rows(rows)
  qkv = _rand((R, 3 * d), 1.0, seed=71, dtype=torch.bfloat16)
  dctx = _rand((R, d), seed=72, dtype=torch.bfloat16)
  gen = torch.Generator().manual_seed(73)
  keep = torch.rand(B, S, generator=gen) > 0.4
  keep[:, 0] = True
  keep[1, 1::2] = False  # parity changes inside a sample: consecutive packed keys are NOT consecutive originally
  bias = torch.zeros(R, device=_dev())
  bias[:rows] = (~keep).reshape(-1).float().to(_dev()) * -10000.0
  ctx_d, lse_d = ops.attn_fwd(qkv, bias, B, S, H, scale, drop_key=31, drop_p=0.2)
  dq_d = ops.attn_bwd(qkv, bias, ctx_d, lse_d, dctx, B, S, H, scale, drop_key=31, drop_p=0.2)
  idx = keep.reshape(-1).nonzero().reshape(-1).to(_dev())          # dense rows that survive, in order
  n = idx.numel()
  qkv_p, dctx_p = torch.zeros_like(qkv), torch.zeros_like(dctx)
  qkv_p[:n], dctx_p[:n] = qkv[idx], dctx[idx]
  cu = torch.zeros(B + 1, dtype=torch.int32)
  cu[1:] = keep.sum(1).cumsum(0).int()
  cu = cu.to(_dev())
  row_index = torch.zeros(R, dtype=torch.int32, device=_dev())
  row_index[:n] = idx.int()
  bias_p = torch.zeros(R, device=_dev())
  ctx_p, lse_p = ops.attn_fwd(qkv_p, bias_p, B, S, H, scale, cu_seqlens=cu, drop_key=31, drop_p=0.2, row_index=row_index)
  dq_p = ops.attn_bwd(qkv_p, bias_p, ctx_p, lse_p, dctx_p, B, S, H, scale, cu_seqlens=cu, drop_key=31, drop_p=0.2,
                      row_index=row_index)
  # kept queries see the same keys with the same mask; (dense) padded keys carry exp(-10000) = 0
  _close('ctx', ctx_p[:n], ctx_d[idx], 2e-2, 1e-2)
  # dQ of kept rows, dK/dV of kept rows: the dense backward also lets the PADDED queries push gradient into the kept keys
  # (the engine never reads a padded query's output, here dctx of those rows is simply zeroed for the comparison)
  dctx_z = dctx.clone()
  dctx_z[:rows][~keep.reshape(-1).to(_dev())] = 0
  dq_dz = ops.attn_bwd(qkv, bias, ctx_d, lse_d, dctx_z, B, S, H, scale, drop_key=31, drop_p=0.2)
  _close('dqkv', dq_p[:n], dq_dz[idx], 4e-2, 2e-2)


@pytest.mark.gpu
@pytest.mark.parametrize('rows,cols,pad', [(128, 128, 0), (384, 1152, 0), (1024, 256, 64)])
def test_transpose_bf16_is_exact(rows, cols, pad):
  """mmt_transpose_bf16 (K-contiguous operands for the row block's backward NT GEMMs): a permutation of bf16 bit patterns,
  with leading dimensions wider than the matrices (elements outside stay untouched)."""
  from mmt_amd import _lib, ops
  from mmt_amd._lib import check
  src = _rand((rows, cols + pad), seed=31, dtype=torch.bfloat16)
  dst = torch.full((cols, rows + pad), 3.0, device=_dev(), dtype=torch.bfloat16)
  check(_lib.lib().mmt_transpose_bf16(ops._p(src), cols + pad, rows, cols, ops._p(dst), rows + pad, ops._stream()), 'transpose')
  assert torch.equal(dst[:, :rows], src[:, :cols].t())
  if pad:
    assert bool((dst[:, rows:] == 3.0).all())
  assert _lib.lib().mmt_transpose_bf16(ops._p(src), cols + pad, rows - 1, cols, ops._p(dst), rows + pad, ops._stream()) != 0


@pytest.mark.gpu
@pytest.mark.parametrize('DH,B,H,S', [(128, 8, 4, 218), (64, 16, 12, 30), (128, 6, 4, 400)])
def test_attention_backward_block_schedule_changes_nothing(DH, B, H, S):
  """mmt_attn_schedule (attn_sched.h): the backward's blocks in longest-first order, every block of a (sample, head) on one
  XCD, empty slots at the end.  The work list must name every live (role, tile, sample, head) exactly once -- checked
  directly -- and the scheduled backward must produce the bits of the unscheduled one (packed batch with dropout)."""
  from mmt_amd import _lib, ops
  from mmt_amd._lib import check
  d = H * DH
  scale = 1.0 / math.sqrt(float(DH))
  g = torch.Generator(device='cpu').manual_seed(40 + B)
  lens = torch.randint(1, S + 1, (B,), generator=g)
  lens[0], lens[1] = S, 1
  cu = torch.zeros(B + 1, dtype=torch.int32)
  cu[1:] = torch.cumsum(lens, 0)
  rows = int(cu[-1])
  R = ops.pad_rows(rows)
  cu_d = cu.to(_dev())
  L = _lib.lib()
  tiles = (S + 63) // 64
  work = torch.full((L.mmt_attn_schedule_words(B, S, H),), 7, device=_dev(), dtype=torch.int32)
  check(L.mmt_attn_schedule(ops._p(cu_d), B, S, H, ops._p(work), ops._stream()), 'mmt_attn_schedule')
  w = work.view(-1, 4).cpu()
  assert w.shape[0] == 2 * tiles * B * H
  live = w[w[:, 0] >= 0]
  want = set()
  for b in range(B):
    for h in range(H):
      for role in range(2):
        for t in range((int(lens[b]) + 63) // 64):
          want.add((b, h, role, t))
  got = [(int(r[0]), int(r[1]) & 0xff, (int(r[1]) >> 8) & 1, int(r[1]) >> 16) for r in live]
  assert len(got) == len(set(got)) and set(got) == want
  for r in live:
    assert int(r[2]) == int(cu[int(r[0])]) and int(r[3]) == int(lens[int(r[0])])
  pos = torch.nonzero(w[:, 0] >= 0).flatten()
  for i, r in zip(pos.tolist(), live):                     # XCD of a block = its index mod 8 = (sample, head) pair mod 8
    assert i % 8 == (int(r[0]) * H + (int(r[1]) & 0xff)) % 8
  for x in range(8):                                       # per XCD: iterations descending, dK/dV before dQ inside a count
    seq = [(-((int(lens[int(r[0])]) + 63) // 64), (int(r[1]) >> 8) & 1) for i, r in zip(pos.tolist(), live) if i % 8 == x]
    assert seq == sorted(seq)
    dead = [i for i in range(x, w.shape[0], 8) if w[i, 0] < 0]
    assert not dead or min(dead) > max([i for i in pos.tolist() if i % 8 == x] + [-1])
  qkv = _rand((R, 3 * d), 1.0, seed=41, dtype=torch.bfloat16)
  bias = torch.zeros(R, device=_dev())
  bias[3:5] = -10000.0
  ridx = torch.zeros(R, dtype=torch.int32)
  for b in range(B):
    ridx[int(cu[b]):int(cu[b + 1])] = b * S + torch.arange(int(lens[b]), dtype=torch.int32)
  ridx = ridx.to(_dev())
  ctx, lse = ops.attn_fwd(qkv, bias, B, S, H, scale, cu_seqlens=cu_d, drop_key=5, drop_p=0.1, row_index=ridx)
  dctx = _rand((R, d), seed=42, dtype=torch.bfloat16)
  a = ops.attn_bwd(qkv, bias, ctx, lse, dctx, B, S, H, scale, cu_seqlens=cu_d, drop_key=5, drop_p=0.1, row_index=ridx)
  b_ = ops.attn_bwd(qkv, bias, ctx, lse, dctx, B, S, H, scale, cu_seqlens=cu_d, drop_key=5, drop_p=0.1, row_index=ridx,
                    scheduled=True)
  assert torch.equal(a, b_)
  assert a[:rows].float().abs().sum().item() > 0


@pytest.mark.gpu
@pytest.mark.parametrize('rows,live,per_item', [(2304, None, False), (2304, 2129, False), (2304, 65, False), (4096, 3000, True)])
def test_wgrad_grouped_256x256_tiles(rows, live, per_item):
  """wgrad3.hip: the four weight gradients of a d = 1024 layer (256 tiles of 256 x 256) in one launch -- eight-phase schedule
  on k-major operands, transpose reads, buffer loads whose descriptor ends at the live row count (rows past it must read as
  ZERO: they hold NaN here), bias gradients from the A fragments on the VALU.  Against torch fp32 on the bf16 operands."""
  from mmt_amd import ops
  d, inter = 1024, 6144
  shapes = [(inter, d), (d, inter), (3 * d, d), (d, d)]  # (N, K2) of dW1, dW2, dWqkv, dWo
  n = rows if live is None else live
  counts = [n, max(1, n - 70), max(1, n - 200), n] if per_item else [n] * 4
  items, refs = [], []
  for q, (N, K2) in enumerate(shapes):
    a = _rand((rows, N), 0.5, seed=50 + q, dtype=torch.bfloat16)
    b = _rand((rows, K2), 0.5, seed=60 + q, dtype=torch.bfloat16)
    refs.append((a[:counts[q]].float().t() @ b[:counts[q]].float(), a[:counts[q]].float().sum(0)))
    a[counts[q]:] = float('nan')
    b[counts[q]:] = float('nan')
    out = torch.full((N, K2), 3.0, device=_dev())
    bias = torch.full((N,), 3.0, device=_dev()) if q != 2 else None
    items.append((a, b, out, bias))
  nrd = torch.tensor([n], device=_dev(), dtype=torch.int32) if live is not None and not per_item else None
  ird = torch.tensor(counts, device=_dev(), dtype=torch.int32) if per_item else None
  ops.wgrad_grouped(items, rows, n_rows_dev=nrd, item_rows_dev=ird)
  for q, ((a, b, out, bias), (want, wb)) in enumerate(zip(items, refs)):
    scale = want.abs().max().item()
    assert torch.isfinite(out).all(), q
    assert (out - want).abs().max().item() <= 2e-3 * scale + 1e-3, (q, (out - want).abs().max().item(), scale)
    if bias is not None:
      assert (bias - wb).abs().max().item() <= 1e-3 * wb.abs().max().item() + 1e-3, q
