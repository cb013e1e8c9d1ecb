"""The per-expert breakdown of a score (mmt_search_expert_parts; VideoIndex.expert_scores) in numpy float64: the
definition the kernel is held to, evaluated on the kernel's own fp32 inputs, with the bound derived for it.

Inputs are what the kernel reads, taken as given: qf, the fp32 fold of the queries (fl(qw[m] * Q[m][j])), and f, the
dequantised stored rows (float32: the row; bfloat16: the row widened; float8_e4m3fn: code * scale -- all exact in fp32, and
the scale a power of two, so dividing on the codes and scaling afterwards is the same real number).  For expert m,

    den  = sum_m qw[m] * gw[m]                       (0 -> 1e-5)
    dot_m  = sum_{j < d} qf[m d + j] * f[m d + j]
    part_m = dot_m / den
    mix_m  = qw[m] * gw[m] / den

The kernel forms dot_m as d fp32 products summed in SOME fixed order, with or without fma; for any order the error of
such a sum is at most d * u * <|qf_m|, |f_m|> to first order (u = 2^-24).  Weights are non-negative, so the M-term
denominator does not cancel and carries a relative error of at most M * u; the division adds u, the fp8 scale multiply
is exact short of underflow and is allowed another u, and two more cover the second-order terms:

    |part_m - exact| <= (d + M + 4) * 2^-24 * <|qf_m|, |f_m|> / |den|

mix_m is one rounded product over the same denominator and a division: within (M + 3) * 2^-24 relative, and mix_m <= 1.
"""
import numpy as np

U = 2.0 ** -24


def fold(x, w):
  """fl(w[n][m] * x[n][m][j]) in fp32 -> [n, M * d]: the bits of mmt_search_fold."""
  x, w = np.asarray(x, np.float32), np.asarray(w, np.float32)
  return (w[:, :, None] * x).astype(np.float32).reshape(x.shape[0], -1)


def expert_parts_ref(qf, qw, f, gw, candidates, m, d):
  """qf float32 [R, M d], qw float32 [R, M], f float32 [NV, M d] (dequantised stored rows), gw float32 [NV, M], candidates
  int [R, C] (-1 = none) -> (parts, mix, bound) float64 [R, C, M]: the definition, and the bound on |part - parts| above.
  NaN in all three where the candidate is none."""
  qf, f = np.asarray(qf, np.float64).reshape(-1, m, d), np.asarray(f, np.float64).reshape(-1, m, d)
  qw, gw, cand = np.asarray(qw, np.float64), np.asarray(gw, np.float64), np.asarray(candidates, np.int64)
  none = cand < 0
  at = np.where(none, 0, cand)
  fg, wg = f[at], gw[at]                                     # [R, C, M, d], [R, C, M]
  gate = qw[:, None, :] * wg                                 # [R, C, M]
  den = gate.sum(-1, keepdims=True)
  den = np.where(den == 0, np.float64(np.float32(1e-5)), den)
  dots = np.einsum('rmj,rcmj->rcm', qf, fg)
  mags = np.einsum('rmj,rcmj->rcm', np.abs(qf), np.abs(fg))
  parts, mix, bound = dots / den, gate / den, (d + m + 4) * U * mags / np.abs(den)
  for out in (parts, mix, bound):
    out[none] = np.nan
  return parts, mix, bound
