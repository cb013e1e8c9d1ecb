"""Keeps the references of tests/test_engine_paths_gpu.py honest on a machine without a GPU: tests/engine_paths_ref.py
against torch.nn.functional.layer_norm, scaled_dot_product_attention and autograd in float64, against tests/dropout_ref.py
for the masks, and against hand-worked cases of the split-K slab geometry."""
import math

import numpy as np
import pytest
import torch

from tests import dropout_ref as D
from tests import engine_paths_ref as R


def _rand(shape, seed, scale=1.0):
  return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale).numpy()


@pytest.mark.parametrize('M,K,req,splits,per', [(56, 512, 0, 8, 1), (200, 3072, 0, 16, 3), (200, 1536, 4, 4, 6), (56, 448, 4, 4, 2),
                                                (56, 320, 4, 3, 2), (56, 64, 0, 1, 1), (56, 2048, 0, 16, 2), (300, 1152, 16, 9, 2)])
def test_splitk_geometry(M, K, req, splits, per):
  """Hand-worked cases: 448 = 7 steps in 4 slabs of 2 (the last one short), 320 = 5 steps -> 3 slabs although 4 were asked
  for, 1152 = 18 steps at 16 requested -> 9 slabs of 2.  The chunks tile [0, K) without a gap."""
  sp, p, stride = R.splitk_geometry(M, 256, K, req)
  assert (sp, p) == (splits, per)
  assert stride == (M + 127) // 128 * 128 * 256
  assert (sp - 1) * p * 64 < K <= sp * p * 64


def test_slab_products_add_up_to_the_product():
  a = torch.from_numpy(_rand((70, 448), 1)).to(torch.bfloat16)
  b = torch.from_numpy(_rand((64, 448), 2)).to(torch.bfloat16)
  prod, mag, kl = R.slab_products(a, b, 56, 2, 4)
  assert kl.tolist() == [128, 128, 128, 64]
  np.testing.assert_allclose(prod.sum(0), a[:56].double().numpy() @ b.double().numpy().T, rtol=0, atol=1e-12)
  assert (mag >= np.abs(prod) - 1e-12).all()


@pytest.mark.parametrize('d,splits,p', [(256, 1, 0.0), (768, 4, 0.1), (1024, 16, 0.5)])
def test_splitk_ln_fwd_reference(d, splits, p):
  """z against the sentence of the header written out with torch, LayerNorm against torch.nn.functional.layer_norm (fp64)."""
  rows, eps = 37, 1e-12
  slabs, bias, res = _rand((splits, rows, d), 3), _rand((d,), 4), _rand((rows, d), 5)
  gamma, beta = 1.0 + 0.1 * _rand((d,), 6), 0.1 * _rand((d,), 7)
  thr = D.thr16_of(p)
  scale = 1.0 / (1.0 - thr / 65536.0)
  orow = np.arange(rows) * 5 + 3
  keep = R.ln_site_keep(0x1234, 77, orow, d, thr) if thr else None
  out = R.splitk_ln_fwd(slabs, bias, res, keep, scale, gamma, beta, eps)
  t = torch.from_numpy
  pre = t(slabs).sum(0) + t(bias)
  z = (pre * scale * t(keep) if thr else pre) + t(res)
  np.testing.assert_allclose(out['z'], z.numpy(), rtol=0, atol=1e-13)
  h = torch.nn.functional.layer_norm(z, (d,), t(gamma), t(beta), eps)
  np.testing.assert_allclose(out['h'], h.numpy(), rtol=1e-12, atol=1e-12)
  np.testing.assert_allclose(out['mean'], z.mean(1).numpy(), rtol=0, atol=1e-13)
  np.testing.assert_allclose(out['rstd'], (1.0 / torch.sqrt(z.var(1, unbiased=False) + eps)).numpy(), rtol=1e-12)
  assert (out['mag'] >= np.abs(out['z']) - 1e-12).all()
  if thr:
    dropped = ~keep
    assert np.array_equal(out['z'][dropped], res[dropped])  # a dropped element is exactly the residual
    assert abs(keep.mean() - (1.0 - p)) < 0.03


def test_ln_site_mask_is_the_row_major_element_index():
  """element index orow * d + col, key hashed with the seed: the same bits as keep_flat on the written-out index, also for
  row numbers whose element index passes 2^32."""
  d, thr = 512, D.thr16_of(0.5)
  orow = np.array([0, 1, 7, (1 << 25) + 3], dtype=np.int64)
  idx = orow[:, None].astype(np.uint64) * np.uint64(d) + np.arange(d, dtype=np.uint64)[None, :]
  assert int(idx.max()) > 1 << 32
  for seed in (None, 0x9cd41a55):
    assert np.array_equal(R.ln_site_keep(0xa5a51234, seed, orow, d, thr), D.keep_flat(D.eff_key(0xa5a51234, seed), idx, thr))
  assert not np.array_equal(R.ln_site_keep(1, None, orow, d, thr), R.ln_site_keep(1, 5, orow, d, thr))


@pytest.mark.parametrize('d,splits,with_res', [(256, 1, False), (512, 4, True), (1024, 16, True)])
def test_ln_bwd_slabs_reference_against_autograd(d, splits, with_res):
  rows, eps = 29, 1e-12
  slabs = _rand((splits, rows, d), 8, 1.0 / math.sqrt(splits + 1))
  res = _rand((rows, d), 9, 1.0 / math.sqrt(splits + 1)) if with_res else None
  z, gamma = _rand((rows, d), 10, 2.0) + 0.5, 1.0 + 0.1 * _rand((d,), 11)
  dout, dz, dgamma, dbeta = R.ln_bwd_slabs(slabs, res, z, gamma, eps)
  zt = torch.from_numpy(z).requires_grad_(True)
  gt = torch.from_numpy(gamma).requires_grad_(True)
  bt = torch.zeros(d, dtype=torch.float64, requires_grad=True)
  want_dout = torch.from_numpy(slabs).sum(0) + (torch.from_numpy(res) if with_res else 0.0)
  torch.nn.functional.layer_norm(zt, (d,), gt, bt, eps).backward(want_dout)
  np.testing.assert_allclose(dout, want_dout.numpy(), rtol=0, atol=1e-13)
  np.testing.assert_allclose(dz, zt.grad.numpy(), rtol=1e-10, atol=1e-12)
  np.testing.assert_allclose(dgamma, gt.grad.numpy(), rtol=1e-10, atol=1e-12)
  np.testing.assert_allclose(dbeta, bt.grad.numpy(), rtol=1e-10, atol=1e-12)


def test_row_dots_are_the_per_head_delta():
  x, y = _rand((9, 256), 12), _rand((9, 256), 13)
  dots, mags = R.row_dots(x, y)
  assert dots.shape == (9, 4)
  np.testing.assert_allclose(dots[:, 1], (x[:, 64:128] * y[:, 64:128]).sum(1), rtol=0, atol=1e-13)
  np.testing.assert_allclose(dots.reshape(9, 2, 2).sum(2), (x * y).reshape(9, 2, 128).sum(2), rtol=0, atol=1e-12)  # DH = 128
  assert (mags >= np.abs(dots)).all()


@pytest.mark.parametrize('packed', [False, True])
def test_attention_rows_reference(packed):
  """Against torch's scaled_dot_product_attention per sample (no dropout), and with a mask against the written-out formula;
  the mask is taken at ORIGINAL positions: the packed run on the kept tokens of a dense batch equals the dense run on them."""
  B, S, H, DH, nq = 3, 20, 2, 8, 3
  d, scale = H * DH, 1.0 / math.sqrt(DH)
  qkv = torch.from_numpy(_rand((B * S, 3 * d), 14))
  g = torch.Generator().manual_seed(15)
  valid = torch.rand(B, S, generator=g) > 0.4
  valid[:, 0] = True
  keep = D.attn_mask(99, B, H, S, D.thr16_of(0.25))
  if not packed:
    bias = (~valid).reshape(-1).double() * -10000.0
    qsel = np.concatenate([b * S + np.array([S - 1, 0, 7]) for b in range(B)])
    ctx, lse = R.attention_rows(qkv, bias, B, S, H, scale, qsel, nq)
    for b in range(B):
      x = qkv[b * S:(b + 1) * S]
      q, k, v = (x[:, i * d:(i + 1) * d].reshape(S, H, DH).transpose(0, 1) for i in range(3))
      want = torch.nn.functional.scaled_dot_product_attention(q, k, v, attn_mask=bias[b * S:(b + 1) * S][None, None, :].expand(H, S, S),
                                                              scale=scale).transpose(0, 1).reshape(S, d)
      np.testing.assert_allclose(ctx[b * nq:(b + 1) * nq].numpy(), want[[S - 1, 0, 7]].numpy(), rtol=1e-10, atol=1e-12)
      s = q @ k.transpose(1, 2) * scale + bias[b * S:(b + 1) * S]
      np.testing.assert_allclose(lse[b * nq:(b + 1) * nq].numpy(), torch.logsumexp(s, -1).t()[[S - 1, 0, 7]].numpy(), rtol=1e-12)
    return
  # packed: only the valid tokens are rows; dense reference: the same tokens with the others masked out as keys
  idx = valid.reshape(-1).nonzero().reshape(-1)
  cu = np.concatenate([[0], valid.sum(1).cumsum(0).numpy()])
  qsel_p = np.concatenate([[cu[b + 1] - 1, cu[b], cu[b] + 1] for b in range(B)])  # last live row, first row, one more
  ctx_p, _ = R.attention_rows(qkv[idx], torch.zeros(len(idx), dtype=torch.float64), B, S, H, scale, qsel_p, nq, cu=cu, keep=keep,
                              drop_scale=1.0 / 0.75, row_index=idx.numpy())
  ctx_d, _ = R.attention_rows(qkv, (~valid).reshape(-1).double() * -10000.0, B, S, H, scale, idx.numpy()[qsel_p], nq, keep=keep,
                              drop_scale=1.0 / 0.75)
  np.testing.assert_allclose(ctx_p.numpy(), ctx_d.numpy(), rtol=1e-10, atol=1e-12)
  # and the dense masked run against the formula written out for one (sample, head, query)
  b, h, qi = 1, 1, int(idx.numpy()[qsel_p][nq] - S)
  x = qkv[S:2 * S]
  s = (x[qi, h * DH:(h + 1) * DH] @ x[:, d + h * DH:d + (h + 1) * DH].t()) * scale + (~valid[1]).double() * -10000.0
  p = torch.softmax(s, -1) * torch.from_numpy(keep[b, h, qi]).double() / 0.75
  np.testing.assert_allclose(ctx_d[nq, h * DH:(h + 1) * DH].numpy(), (p @ x[:, 2 * d + h * DH:2 * d + (h + 1) * DH]).numpy(),
                             rtol=1e-10, atol=1e-12)


def test_reduce_slabs_reference():
  ws = _rand((4 * 24 + 5,), 16)
  s, mag = R.reduce_slabs(ws, 4, 24)
  np.testing.assert_allclose(s, ws[:24] + ws[24:48] + ws[48:72] + ws[72:96], rtol=0, atol=1e-13)
  assert (mag >= np.abs(s)).all()
