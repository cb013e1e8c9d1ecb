"""fp64 host references of the kernel paths that only the encoder engine reaches (tests/test_engine_paths_gpu.py), written
from the comments of include/mmt_hip.h and the formulas of model/bert.py -- not from any kernel's output.  numpy and CPU torch
(float64).  Their own checks: tests/test_engine_paths_ref_cpu.py.

Every reference returns, next to the value, the sum of the magnitudes of the terms that enter it where a test derives its
bound from the arithmetic: an fp32 sum of n terms in ANY order is within (n - 1) 2^-24 sum |terms| of the exact sum to first
order, and the tests allow n 2^-24 sum |terms|.
"""
import numpy as np
import torch

from tests import dropout_ref as D

U32 = 2.0**-24  # unit roundoff of fp32
BK = 64         # K-step of the GEMM kernels


def f64(t):
  """torch tensor (any float type, any device) -> float64 numpy."""
  return t.detach().double().cpu().numpy()


# ---- split-K slabs -----------------------------------------------------------------------------------------------------

def splitk_geometry(M, N, K, requested):
  """(splits, K-steps per slab, slab stride in floats): `requested` slabs (<= 0: as many as there are K-steps) capped at 16
  and at the K-steps, the steps dealt out evenly rounded up, and the slab count recomputed from that -- so it can come out
  below the request.  A slab holds round_up(M, 128) rows of N floats."""
  ksteps = K // BK
  sp = 16 if requested <= 0 else requested
  sp = min(sp, ksteps, 16)
  per = -(-ksteps // sp)
  return -(-ksteps // per), per, (M + 127) // 128 * 128 * N


def slab_products(a, b, M, per, splits):
  """a [>= M, K], b [N, K] (bf16 torch): per slab s the fp64 product over its K chunk [s per 64, min(K, (s + 1) per 64)), the
  sum of |a_k| |b_k| over the chunk and the chunk length.  -> (prod [splits, M, N], mag [splits, M, N], kl [splits])."""
  a64, b64 = f64(a)[:M], f64(b)
  K = a64.shape[1]
  prod, mag, kl = [], [], []
  for s in range(splits):
    k0, k1 = s * per * BK, min(K, (s + 1) * per * BK)
    prod.append(a64[:, k0:k1] @ b64[:, k0:k1].T)
    mag.append(np.abs(a64[:, k0:k1]) @ np.abs(b64[:, k0:k1]).T)
    kl.append(k1 - k0)
  return np.stack(prod), np.stack(mag), np.array(kl)


# ---- LayerNorm with the slab sum folded in ------------------------------------------------------------------------------

def ln_site_keep(site_key, seed, orow, d, thr16):
  """Keep mask [len(orow), d] of a LayerNorm-site dropout: element index orow * d + col under eff_key(site key, seed)."""
  return D.keep_rows(D.eff_key(site_key, seed), np.asarray(orow, dtype=np.int64), d, thr16)


def layer_norm(z, gamma, beta, eps):
  """(h, mean, rstd) of a row-wise LayerNorm, biased variance (bert.py:188,236)."""
  mean = z.mean(1)
  var = ((z - mean[:, None])**2).mean(1)
  rstd = 1.0 / np.sqrt(var + eps)
  return (z - mean[:, None]) * rstd[:, None] * gamma[None, :] + beta[None, :], mean, rstd


def splitk_ln_fwd(slabs, bias, res, keep, scale, gamma, beta, eps):
  """z = dropout(sum_s slab_s + bias) + res, h = LN(z)  (bert.py:185-189 / 233-237).  slabs [splits, rows, d], res [rows, d]
  (already gathered), keep bool [rows, d] or None, scale = 1 / (1 - p).  -> dict(pre, z, h, mean, rstd, mag) with pre the
  sum in front of the dropout and mag = scale (sum_s |slab_s| + |bias|) + |res|, the magnitudes entering a kept z."""
  pre = slabs.sum(0) + bias[None, :]
  mag = scale * (np.abs(slabs).sum(0) + np.abs(bias)[None, :]) + np.abs(res)
  y = pre * scale
  if keep is not None:
    y = np.where(keep, y, 0.0)
  z = y + res
  h, mean, rstd = layer_norm(z, gamma, beta, eps)
  return dict(pre=pre, z=z, h=h, mean=mean, rstd=rstd, mag=mag)


def ln_bwd(dout, z, gamma, eps):
  """Backward of h = LN(z) gamma + beta for the incoming gradient dout: (dz, dgamma, dbeta).
  xh = (z - mean) rstd, g = dout gamma, dz = rstd (g - mean_c g - xh mean_c (g xh))."""
  _, mean, rstd = layer_norm(z, np.ones_like(gamma), np.zeros_like(gamma), eps)
  xh = (z - mean[:, None]) * rstd[:, None]
  g = dout * gamma[None, :]
  dz = rstd[:, None] * (g - g.mean(1)[:, None] - xh * (g * xh).mean(1)[:, None])
  return dz, (dout * xh).sum(0), dout.sum(0)


def ln_bwd_slabs(slabs, res, z, gamma, eps):
  """mmt_ln_bwd_slabs: the same with dout = sum_s slab_s + res (res may be None)."""
  dout = slabs.sum(0)
  if res is not None:
    dout = dout + res
  return (dout,) + ln_bwd(dout, z, gamma, eps)


# ---- row dots / delta ---------------------------------------------------------------------------------------------------

def row_dots(x, y):
  """x, y [rows, n] float64, n % 64 == 0 -> (dots [rows, n / 64], mags [rows, n / 64]): sum and sum of magnitudes of x y over
  each group of 64 columns (MmtEpilogue.dot_out; the attention backward's delta of head h is its DH / 64 groups)."""
  p = x * y
  rows, n = p.shape
  return p.reshape(rows, n // 64, 64).sum(2), np.abs(p).reshape(rows, n // 64, 64).sum(2)


# ---- attention ----------------------------------------------------------------------------------------------------------

def attention_rows(qkv, mask_bias, B, S, H, scale, qsel, nq, cu=None, keep=None, drop_scale=1.0, row_index=None):
  """Attention of bert.py:141-168 over ALL keys of a sample, evaluated at the queries qsel [B * nq] (rows of qkv) only.
  qkv float64 torch [rows, 3 d] (may require grad); mask_bias [rows] float64 additive key mask; sample b owns rows
  cu[b] .. cu[b + 1] (None: b S .. (b + 1) S).  keep: bool [B, H, S, S] dropout mask at ORIGINAL (query, key) positions;
  row_index [rows] maps a row to b S + its original position (None: the row's own position in its sample).
  -> (ctx [B * nq, d], lse [B * nq, H]) float64 torch."""
  d = qkv.shape[1] // 3
  dh = d // H
  ctx, lse = [], []
  for b in range(B):
    o, n = (b * S, S) if cu is None else (int(cu[b]), int(cu[b + 1]) - int(cu[b]))
    rows = torch.as_tensor(np.asarray(qsel[b * nq:(b + 1) * nq], dtype=np.int64))
    pos = (np.arange(o, o + n) - o) if row_index is None else (np.asarray(row_index[o:o + n], dtype=np.int64) - b * S)
    qpos = pos[rows.numpy() - o]
    q = qkv[rows, :d].reshape(nq, H, dh).transpose(0, 1)
    k = qkv[o:o + n, d:2 * d].reshape(n, H, dh).transpose(0, 1)
    v = qkv[o:o + n, 2 * d:].reshape(n, H, dh).transpose(0, 1)
    s = q @ k.transpose(1, 2) * scale + mask_bias[o:o + n][None, None, :]
    lse.append(torch.logsumexp(s, -1).transpose(0, 1))
    p = torch.softmax(s, -1)
    if keep is not None:
      m = torch.from_numpy(np.ascontiguousarray(keep[b][:, qpos][:, :, pos])).double()
      p = p * m * drop_scale
    ctx.append((p @ v).transpose(0, 1).reshape(nq, d))
  return torch.cat(ctx), torch.cat(lse)


# ---- slab sums ----------------------------------------------------------------------------------------------------------

def reduce_slabs(ws, splits, count):
  """ws: float64 [>= splits * count] -> (sum over the slabs [count], sum of magnitudes [count])."""
  s = ws[:splits * count].reshape(splits, count)
  return s.sum(0), np.abs(s).sum(0)
