"""fp64 host reference of the text heads (texthead.hip: any shape; texthead2.hip: N <= 32 rows), stage by stage, with the bound
of every stage.  Written from include/mmt_hip.h ("text heads") and the formulas of model/model.py -- GatedEmbeddingUnit
(:683-702), ContextGating with BatchNorm1d (:736-750), compute_weights_from_emb with the L1 normalise (:262-283, 618),
F.normalize -- not from any kernel's output.  numpy, float64.  Its own checks: tests/test_text_heads_ref_cpu.py; the kernels
against it: tests/test_text_heads_bounds_gpu.py.

STAGES.  Each stage takes the DEVICE's values of the stage before it (read back from the workspace, whose float layout
mmt_text_heads_workspace_floats documents: y | x1 | mean | rstd | dyg | dz | dlogit | ...; after the backward dz holds dx1 and
dyg holds dy), so a bound is local to one stage and nothing is amplified through rstd or 1 / |o|:

  1  y = text W1^T + b1, laid out [N, M, d]                 5  tw = softmax_m(moe_in moe_w^T + moe_b), L1-normalised, (B, C, M)
  2  x1 = y W2^T + b2                                       6  dx1: normalise, gate and BatchNorm backward; g_bn_gamma, g_bn_beta,
  3  mean, rstd over the N rows of x1 (training: biased        g_b2 = sum_n dx1, g_w2 = dx1^T y
     variance, eps 1e-5; eval: the running statistics)      7  dy = gate-path gradient + dx1 W2; g_b1, g_w1 = dy^T text, dtext
  4  e = normalize(y sigmoid(BN(x1))), (B, M, C, d)         8  dlogit = tw (dtw - <tw, dtw>); g_moe_w, g_moe_b, MoE input gradient

Training also updates the running statistics: 0.9 old + 0.1 new with the UNBIASED variance, and for N = 1 the biased one (0):
both kernel files say so in their code (N > 1 ? q / (N - 1) : var).  PyTorch refuses BatchNorm1d training on one row; this is
the project's own rule for that shape.

BOUNDS.  The convention of tests/engine_paths_ref.py: an fp32 sum of n terms in ANY order is allowed n 2^-24 sum |terms| -- the
contractions with their length (K, d, N or M d) plus one for the bias or the accumulate term.  An elementwise stage gets the
first-order sum of the roundings of its own operations, propagated through the stage (1 - sg, for one, carries an ABSOLUTE
error of one unit roundoff plus the error of sg, which matters where the gate saturates).  One part cannot be derived: the
accuracy of what the library's build (-ffast-math) approximates -- the exponential (__expf: the hardware's exp2 of a rounded
product, whose rounding IS derived: |x| 2^-24 relative), division, reciprocal and square root.  Each evaluation of one of these
is allowed FN_ULPS units in the last place (2^-23 relative) of its result.  A bound is therefore a pair (base, fn): base + FN_ULPS
2^-23 fn, fn the first-order sensitivity of the stage to one unit of relative error in each such evaluation.

FN_ULPS was measured on an MI355X against these stage references over every case of tests/test_text_heads_bounds_gpu.py.  Two
figures per elementwise stage, the sums (stages 1, 2, the g_* and dtext) holding no such evaluation:
  excess    the largest (error - base) / (2^-23 fn): what the derived roundings leave unexplained;
  charged   the largest error / (2^-23 fn), the element's WHOLE error charged to the functions, over the elements where one ulp
            per evaluation outweighs the derived roundings (2^-23 fn >= base) -- elsewhere the figure would be about the sums.
Worst values measured (ulps per evaluation; "-": the stage has no element where the functions outweigh the roundings):

  stage                                 excess   charged
  3  rstd, eval (square root, 1 / x)    0.000    0.433   (small path 0.433, general path 0.212)
  3  mean, rstd, running_var, training  0.000    0.177   (N = 1; - at every other N)
  4  text_embds                         0.000    0.477   (d = 4 without BatchNorm; - at every other shape)
  5  text_weights                       0.000    -
  6  dx1, g_bn_gamma, g_bn_beta         0.000    -
  7  dy (its gate-path part)            0.000    -

So the exponential is nowhere visible by itself: where it enters, the derived part of the bound (the convention's n 2^-24 sum
|terms| of the sums next to it) is the larger, and covered every error measured.  FN_ULPS = 4 x the worst figure (0.477), rounded
up to a power of two = 2; the margin is for the few thousand points at which the cases sample each function.
"""
import numpy as np

from tests import dropout_ref as D

U32 = 2.0**-24      # unit roundoff of fp32
ULP = 2.0**-23      # one unit in the last place, relative (at most)
FN_ULPS = 2.0       # allowance per evaluation of an approximated function, see above
TINY = 2.0**-126    # smallest normal fp32: what a result may lose to underflow
EPS_BN = 1e-5
EPS_NORM = 1e-12


# ---- bounds: pairs (base, fn) stacked on a leading axis, linear in the allowance --------------------------------------------

def lin(base, fn=None):
  base = np.asarray(base, dtype=np.float64)
  return np.stack([base, np.zeros_like(base) if fn is None else np.broadcast_to(np.asarray(fn, dtype=np.float64), base.shape)])


def FN(like):
  """One approximated evaluation: relative error 0 (base) + 1 (fn)."""
  like = np.asarray(like, dtype=np.float64)
  return np.stack([np.zeros_like(like), np.ones_like(like)])


def bsum(b, axis):
  return b.sum(axis + 1 if axis >= 0 else axis)


def bound(b, allowance=None):
  return b[0] + (FN_ULPS if allowance is None else allowance) * ULP * b[1]


class R(dict):
  """A stage result: val, bnd (a pair) and, for a sum, mag = sum |terms|."""
  __getattr__ = dict.__getitem__


def sum_bound(mag, n):
  return lin(n * U32 * np.asarray(mag, dtype=np.float64))


# ---- values: the formulas, in the dtype of their inputs (float64: the reference; float32: a stand-in for a kernel) -------------

def _bmm_nt(a, W):
  """a [N, M, c], W [M, j, c] -> [N, M, j]: per expert a W^T"""
  return np.matmul(a.transpose(1, 0, 2), W.transpose(0, 2, 1)).transpose(1, 0, 2)


def _bmm_nn(a, W):
  """a [N, M, c], W [M, c, j] -> [N, M, j]: per expert a W"""
  return np.matmul(a.transpose(1, 0, 2), W).transpose(1, 0, 2)


def v_fc1(text, W1, b1):
  """text [N, K], W1 [M, d, K], b1 [M, d] -> y [N, M, d]"""
  M, d, K = W1.shape
  return (text @ W1.reshape(M * d, K).T).reshape(-1, M, d) + b1[None]


def v_fc2(y, W2, b2):
  """y [N, M, d], W2 [M, d, d] -> x1 [N, M, d]"""
  return _bmm_nt(y, W2) + b2[None]


def v_batch_stats(x1, unbiased_norm=False, no_eps=False, drop_last_row=False):
  """-> mean, rstd [M, d] (biased variance), unbiased variance for the running update (N = 1: the biased one)."""
  N = x1.shape[0]
  t = x1.dtype.type
  s = (x1[:-1] if drop_last_row else x1).sum(0)
  mean = s / t(N)
  q = ((x1 - mean[None])**2).sum(0)
  var = q / t(N - 1 if unbiased_norm else N)
  rstd = t(1) / np.sqrt(var + (t(0) if no_eps else t(EPS_BN)))
  return mean, rstd, (q / t(N - 1) if N > 1 else q / t(N))


def v_running_rstd(rv, no_eps=False):
  t = rv.dtype.type
  return t(1) / np.sqrt(rv + (t(0) if no_eps else t(EPS_BN)))


def v_running_update(old, new):
  t = old.dtype.type
  return t(0.9) * old + t(0.1) * new


def v_gate(y, x1, mean, rstd, gamma, beta, use_bn):
  """-> z, sg, o [N, M, d]"""
  t = y.dtype.type
  z = (x1 - mean[None]) * rstd[None] * gamma[None] + beta[None] if use_bn else x1
  sg = t(1) / (t(1) + np.exp(-z))
  return z, sg, y * sg


def to_bmcd(e, C, wrong_order=False):
  """[N, M, d] -> (B, M, C, d) (wrong_order: (B, C, M, d))"""
  N, M, d = e.shape
  e = e.reshape(N // C, C, M, d)
  return np.ascontiguousarray(e).reshape(N // C, M, C, d) if wrong_order else np.ascontiguousarray(e.transpose(0, 2, 1, 3))


def from_bmcd(e, C):
  """(B, M, C, d) -> [N, M, d]"""
  B, M, _, d = e.shape
  return np.ascontiguousarray(e.transpose(0, 2, 1, 3)).reshape(B * C, M, d)


def v_embed(y, x1, mean, rstd, gamma, beta, use_bn):
  """-> e [N, M, d] = o / max(|o|, 1e-12)"""
  t = y.dtype.type
  o = v_gate(y, x1, mean, rstd, gamma, beta, use_bn)[2]
  nrm = np.sqrt((o * o).sum(-1, keepdims=True))
  return o / np.maximum(nrm, t(EPS_NORM))


def v_moe(x, moe_w, moe_b, drop_expert=False, no_l1=False):
  """x [N, K], moe_w [M, K], moe_b [M] -> tw [N, M]"""
  t = x.dtype.type
  l = x @ moe_w.T + moe_b[None]
  if drop_expert:
    l = l[:, :-1]
  e = np.exp(l - l.max(1, keepdims=True))
  p = e / e.sum(1, keepdims=True)
  if drop_expert:
    p = np.concatenate([p, np.zeros_like(p[:, :1])], 1)
  return p if no_l1 else p / np.maximum(np.abs(p).sum(1, keepdims=True), t(EPS_NORM))


def v_gate_bwd(de, y, x1, mean, rstd, gamma, beta, use_bn, training, no_proj=False, no_inv_n=False):
  """de [N, M, d] -> dyg (gate-path gradient wrt y), dz (wrt the gate's input), dx1, g_bn_gamma, g_bn_beta ([M, d] or None)"""
  t = y.dtype.type
  N = y.shape[0]
  z, sg, o = v_gate(y, x1, mean, rstd, gamma, beta, use_bn)
  nrm = np.sqrt((o * o).sum(-1, keepdims=True))
  inv = t(1) / np.maximum(nrm, t(EPS_NORM))
  proj = np.where(nrm > t(EPS_NORM), (de * o).sum(-1, keepdims=True) * inv * inv, t(0))
  if no_proj:
    proj = proj * t(0)
  dox = (de - o * proj) * inv
  dyg = dox * sg
  dz = dox * y * sg * (t(1) - sg)
  if not use_bn:
    return dyg, dz, dz, None, None
  xh = (x1 - mean[None]) * rstd[None]
  s1, s2 = dz.sum(0), (dz * xh).sum(0)
  gr = (gamma * rstd)[None]
  if training:
    n = t(1) if no_inv_n else t(N)
    dx1 = gr * (dz - s1[None] / n - xh * s2[None] / n)
  else:
    dx1 = gr * dz
  return dyg, dz, dx1, s2, s1


def v_dy(dyg, dx1, W2):
  """dy[n, m, j] = dyg + sum_c dx1[n, m, c] W2[m, c, j]"""
  return dyg + _bmm_nn(dx1, W2)


def v_wgrad(a, b):
  """a [N, M, i], b [N, M, c] or [N, c] -> [M, i, c]: sum over the rows"""
  N, M, i = a.shape
  if b.ndim == 3:
    return np.matmul(a.transpose(1, 2, 0), b.transpose(1, 0, 2))
  return (a.reshape(N, M * i).T @ b).reshape(M, i, -1)


def v_dtext(dy, W1):
  N, M, d = dy.shape
  return dy.reshape(N, M * d) @ W1.reshape(M * d, -1)


def v_dlogit(tw, dtw):
  return tw * (dtw - (tw * dtw).sum(1, keepdims=True))


def moe_mask(key, seed, N, K, thr16, scale):
  """The on-the-fly dropout of the MoE input as a float64 factor [N, K]: keep(eff_key(key, seed), n K + k) * scale."""
  idx = np.arange(N, dtype=np.uint64)[:, None] * np.uint64(K) + np.arange(K, dtype=np.uint64)[None, :]
  return D.keep_flat(D.eff_key(key, seed), idx, thr16).astype(np.float64) * float(np.float32(scale))


# ---- stages: fp64 value + bound ----------------------------------------------------------------------------------------------

def s_fc1(text, W1, b1):
  mag = v_fc1(np.abs(text), np.abs(W1), np.abs(b1))
  return R(val=v_fc1(text, W1, b1), mag=mag, bnd=sum_bound(mag, text.shape[1] + 1))


def s_fc2(y, W2, b2):
  mag = v_fc2(np.abs(y), np.abs(W2), np.abs(b2))
  return R(val=v_fc2(y, W2, b2), mag=mag, bnd=sum_bound(mag, y.shape[2] + 1))


def s_batch_stats(x1):
  """Stage 3, training.  mean = (sum x) / N: the sum's bound, the division (one approximated evaluation and a product).
  q = sum (x - mean)^2 with the error of mean in every term; var + eps; rstd = 1 / sqrt: two evaluations."""
  N = x1.shape[0]
  mean, rstd, varu = v_batch_stats(x1)
  am = np.abs(mean)
  dmean = lin(N * U32 * np.abs(x1).sum(0) / N + U32 * am) + FN(am) * am
  dev = x1 - mean[None]
  ddev = dmean[:, None] + lin(U32 * np.abs(dev))
  q = (dev * dev).sum(0)
  dq = bsum(2.0 * np.abs(dev) * ddev, 0) + lin((N + 1) * U32 * q)
  var = q / N
  dvar = dq / N + (lin(U32 * var) + FN(var) * var)
  ve = var + EPS_BN
  dve = dvar + lin(U32 * ve + U32 * EPS_BN)
  drstd = rstd * (dve / (2.0 * ve) + lin(2.0 * U32 * np.ones_like(ve)) + 2.0 * FN(ve))
  n1 = max(N - 1, 1)
  dvaru = dq / n1 + (lin(U32 * varu) + FN(varu) * varu)
  return R(mean=mean, dmean=dmean, rstd=rstd, drstd=drstd, varu=varu, dvaru=dvaru)


def s_running_rstd(rv):
  """Stage 3, eval: 1 / sqrt(rv + eps).  The sum's rounding (and the rounded constant) halved by the root, two evaluations --
  nothing else, so this is where the device's square root and reciprocal can be measured."""
  rstd = v_running_rstd(rv)
  return R(val=rstd, bnd=rstd * (lin(0.5 * U32 * (1.0 + EPS_BN / (rv + EPS_BN))) + 2.0 * FN(rv)))


def s_running_update(old, new, dnew=None):
  """0.9 old + 0.1 new: two rounded constants (the general path forms 1 - 0.1f), two products, one sum: 4 roundings."""
  val = v_running_update(old, new)
  bnd = lin(4.0 * U32 * (np.abs(0.9 * old) + np.abs(0.1 * new)))
  return R(val=val, bnd=bnd if dnew is None else bnd + 0.1 * dnew)


def _gate_err(y, x1, mean, rstd, gamma, beta, use_bn):
  """z, sg, o with the absolute error bounds of sg and o as a kernel forms them from the same fp32 inputs.
  z = (x1 - mean) rstd gamma + beta: four roundings (a fused multiply-add only removes one).  exp(-z): relative |dz| from its
  argument, |z| 2^-24 from the rounded product in front of exp2, one evaluation.  1 + e: one rounding; 1 / (.): one evaluation.
  d sg / sg = (1 - sg) d e / e."""
  z, sg, o = v_gate(y, x1, mean, rstd, gamma, beta, use_bn)
  if use_bn:
    t = (x1 - mean[None]) * rstd[None] * gamma[None]
    dz = lin(U32 * (3.0 * np.abs(t) + np.abs(z)))
  else:
    dz = lin(np.zeros_like(z))
  rho = (1.0 - sg) * (dz + lin(U32 * np.abs(z)) + FN(z)) + lin(U32 * np.ones_like(z)) + FN(z)
  dsg = sg * rho
  do = np.abs(o) * (rho + lin(U32 * np.ones_like(z)))
  return z, sg, o, dsg, do


def _norm_err(o, do):
  """ss = sum o^2 over d terms, inv = 1 / max(sqrt(ss), 1e-12): -> ss, inv, relative error bound of inv (two evaluations)."""
  d = o.shape[-1]
  ss = (o * o).sum(-1, keepdims=True)
  dss = bsum(2.0 * np.abs(o) * do, -1)[..., None] + lin((d + 1) * U32 * ss)
  safe = np.maximum(ss, TINY)
  rinv = dss / (2.0 * safe) + lin(2.0 * U32 * np.ones_like(ss)) + 2.0 * FN(ss)
  return ss, 1.0 / np.maximum(np.sqrt(ss), EPS_NORM), rinv


def s_embed(y, x1, mean, rstd, gamma, beta, use_bn):
  """Stage 4 in [N, M, d] order (to_bmcd gives the output's).  Also min_norm, the smallest |o| of a row."""
  z, sg, o, dsg, do = _gate_err(y, x1, mean, rstd, gamma, beta, use_bn)
  ss, inv, rinv = _norm_err(o, do)
  e = o * inv
  return R(val=e, bnd=do * inv + np.abs(e) * (rinv + lin(U32 * np.ones_like(e))), min_norm=float(np.sqrt(ss).min()))


def s_moe(x, moe_w, moe_b, extra=0):
  """Stage 5.  The logits are sums of K + 1 terms (+ extra roundings per term: the dropout's scale).  The maximum that the device
  subtracts is a shift that the softmax does not see, so its error does not enter; l - max: one rounding; exp: its argument's
  error, the rounded product, one evaluation; sum over M; e / sum: one evaluation and a product; the L1 sum and division the
  same again.  Relative errors of a sum of positive terms: the weighted mean of the terms' + M 2^-24.  TINY: underflow."""
  M, K = moe_w.shape
  l = x @ moe_w.T + moe_b[None]
  dl = sum_bound(np.abs(x) @ np.abs(moe_w).T + np.abs(moe_b)[None], K + 1 + extra)
  a = l - l.max(1, keepdims=True)
  one = np.ones_like(a)
  rho_e = dl + lin(2.0 * U32 * np.abs(a)) + FN(a)
  e = np.exp(a)
  S = e.sum(1, keepdims=True)
  rho_S = bsum(e * rho_e, 1)[..., None] / S + lin(M * U32 * np.ones_like(S))
  p = e / S
  rho_p = rho_e + rho_S + FN(a) + lin(U32 * one)
  l1 = p.sum(1, keepdims=True)
  rho_l1 = bsum(p * rho_p, 1)[..., None] / l1 + lin(M * U32 * np.ones_like(S))
  tw = p / l1
  return R(val=tw, bnd=tw * (rho_p + rho_l1 + FN(a) + lin(U32 * one)) + lin(TINY * one))


def s_gate_bwd(de, y, x1, mean, rstd, gamma, beta, use_bn, training):
  """Stage 6 and the gate-path part of stage 7, from de [N, M, d] and the forward buffers.  A kernel may re-form sg and o (the
  general path) or re-read its forward's (the small path): both carry the errors of _gate_err.  First order throughout."""
  N, M, d = y.shape
  z, sg, o, dsg, do = _gate_err(y, x1, mean, rstd, gamma, beta, use_bn)
  ss, inv, rinv = _norm_err(o, do)
  live = np.sqrt(ss) > EPS_NORM
  u1 = lambda v: lin(U32 * np.abs(v))
  dot = (de * o).sum(-1, keepdims=True)
  ddot = bsum(np.abs(de) * do, -1)[..., None] + lin((d + 1) * U32 * np.abs(de * o).sum(-1, keepdims=True))
  proj = np.where(live, dot * inv * inv, 0.0)
  dproj = ddot * inv * inv + np.abs(proj) * (2.0 * rinv + lin(2.0 * U32 * np.ones_like(ss)))
  op = o * proj
  dop = do * np.abs(proj) + np.abs(o) * dproj + u1(op)
  diff = de - op
  dox = diff * inv
  ddox = (dop + u1(diff)) * inv + np.abs(dox) * (rinv + lin(U32 * np.ones_like(ss)))
  dyg = dox * sg
  ddyg = ddox * sg + np.abs(dox) * dsg + u1(dyg)
  oms = 1.0 - sg
  doms = dsg + lin(U32 * np.ones_like(sg))           # 1 - sg: the error of sg and one ABSOLUTE unit roundoff
  dz = dox * y * sg * oms
  ddz = ddox * np.abs(y * sg * oms) + np.abs(dox * y) * (dsg * oms + sg * doms) + 3.0 * u1(dz)
  out = R(dyg=dyg, ddyg=ddyg, dz=dz, ddz=ddz)
  if not use_bn:
    out.update(dx1=dz, ddx1=ddz, g_gamma=None, g_beta=None)
    return out
  xh = (x1 - mean[None]) * rstd[None]
  dxh = lin(2.0 * U32 * np.abs(xh))
  s1, s2 = dz.sum(0), (dz * xh).sum(0)
  ds1 = bsum(ddz, 0) + lin(N * U32 * np.abs(dz).sum(0))
  ds2 = bsum(ddz * np.abs(xh) + np.abs(dz) * dxh + u1(dz * xh), 0) + lin(N * U32 * np.abs(dz * xh).sum(0))
  gr = (gamma * rstd)[None]
  if training:  # s / N: one evaluation and a product each
    m1, m2 = s1[None] / N, xh * s2[None] / N
    dm1 = (ds1 + np.abs(s1) * (FN(s1) + lin(U32 * np.ones_like(s1))))[:, None] / N
    dm2 = (dxh * np.abs(s2)[None] + np.abs(xh) * ds2[:, None] + np.abs(xh * s2[None]) * (FN(xh) + lin(2.0 * U32 * np.ones_like(xh)))) / N
    inner = dz - m1 - m2
    dinner = ddz + dm1 + dm2 + lin(2.0 * U32 * (np.abs(dz) + np.abs(m1) + np.abs(m2)))
    dx1 = gr * inner
  else:
    dx1, dinner = gr * dz, ddz
  out.update(dx1=dx1, ddx1=np.abs(gr) * dinner + 3.0 * u1(dx1), g_gamma=s2, dg_gamma=ds2, g_beta=s1, dg_beta=ds1)
  return out


def s_colsum(v):
  """sum over the N rows of v [N, ...]"""
  return R(val=v.sum(0), bnd=sum_bound(np.abs(v).sum(0), v.shape[0]))


def s_wgrad(a, b):
  return R(val=v_wgrad(a, b), bnd=sum_bound(v_wgrad(np.abs(a), np.abs(b)), a.shape[0]))


def s_dy(dyg, ddyg, dx1, W2):
  """Stage 7: the contraction over d plus the accumulate term, which carries its own elementwise error."""
  mag = v_dy(np.abs(dyg), np.abs(dx1), np.abs(W2))
  return R(val=v_dy(dyg, dx1, W2), bnd=ddyg + sum_bound(mag, dx1.shape[2] + 1))


def s_dtext(dy, W1, moe_term=None):
  """dy [N, M d] . W1_all, plus (no dtext_moe) the MoE input gradient added in: its own bound and one more rounding."""
  val, mag = v_dtext(dy, W1), v_dtext(np.abs(dy), np.abs(W1))
  bnd = sum_bound(mag, dy.shape[1] * dy.shape[2])
  if moe_term is not None:
    val = val + moe_term.val
    bnd = bnd + moe_term.bnd + lin(U32 * (mag + np.abs(moe_term.val)))
  return R(val=val, bnd=bnd)


def s_dlogit(tw, dtw):
  M = tw.shape[1]
  dot = (tw * dtw).sum(1, keepdims=True)
  val = tw * (dtw - dot)
  ddot = (M + 1) * U32 * np.abs(tw * dtw).sum(1, keepdims=True)
  return R(val=val, bnd=lin(np.abs(tw) * (ddot + U32 * np.abs(dtw - dot)) + U32 * np.abs(val)))


def s_moe_wgrad(dlogit, ddlogit, x):
  """g_moe_w [M, K] = dlogit^T x, g_moe_b [M] = sum_n dlogit, over the N rows.  Two kernels may have written ws.dlogit (the small
  path forms it once per launch that needs it, with another order of its M-term dot): the one read back and the one the sums
  used are both within the stage's bound of its value, so they differ by at most twice that."""
  N = x.shape[0]
  slack = 2.0 * bound(ddlogit, 0.0)
  w = R(val=dlogit.T @ x, bnd=lin(N * U32 * (np.abs(dlogit).T @ np.abs(x)) + slack.T @ np.abs(x)))
  b = R(val=dlogit.sum(0), bnd=lin(N * U32 * np.abs(dlogit).sum(0) + slack.sum(0)))
  return w, b


def s_moe_dinput(dlogit, moe_w, mask=None):
  """sum_m dlogit[n, m] moe_w[m, k], times the dropout's factor where there is one (two more roundings)."""
  M = moe_w.shape[0]
  val, mag = dlogit @ moe_w, np.abs(dlogit) @ np.abs(moe_w)
  if mask is not None:
    val, mag = val * mask, mag * mask
  return R(val=val, bnd=sum_bound(mag, M + (2 if mask is not None else 0)))


# ---- cases, a stand-in for the kernels, and the check of a set of buffers against the stages -----------------------------------

def form(text_moe=False, dtext=True, dtext_moe=False, moe=True, drop_p=0.0, g_null=()):
  """An argument form.  g_null: (parameter name, expert) pairs whose g_* pointer is NULL, or 'all'."""
  return dict(text_moe=text_moe, dtext=dtext, dtext_moe=dtext_moe, moe=moe, drop_p=drop_p, g_null=g_null)


PARAMS = ('w1', 'b1', 'w2', 'b2', 'bn_gamma', 'bn_beta', 'moe_w', 'moe_b')


def wants(fm, name, m):
  return fm['g_null'] != 'all' and (name, m) not in fm['g_null']


def make_case(N, C, M, d, K, use_bn, training, seed=0, logit_spread=0.0, zero_row=None):
  """Seeded host inputs as float32 (what the device is given).  Weights scaled by fan-in, running_var in [1, 1.3].  logit_spread:
  moe_w scaled so that a row's logits spread over about that much (0: fan-in scale).  zero_row: that text row and every b1 zero."""
  g = np.random.default_rng(1000 * seed + N + 7 * d + K)
  r = lambda *s, sc=1.0: (g.standard_normal(s) * sc).astype(np.float32)
  c = dict(N=N, C=C, M=M, d=d, K=K, use_bn=int(use_bn), training=int(training))
  c.update(text=r(N, K), text_moe=r(N, K), W1=r(M, d, K, sc=K**-0.5), b1=r(M, d, sc=0.1), W2=r(M, d, d, sc=d**-0.5),
           b2=r(M, d, sc=0.1), gamma=(1.0 + r(M, d, sc=0.1)).astype(np.float32), beta=r(M, d, sc=0.1),
           moe_w=r(M, K, sc=K**-0.5 * (logit_spread / 4.0 if logit_spread else 1.0)), moe_b=r(M, sc=0.1),
           rm=r(M, d, sc=0.1), rv=(1.0 + 0.3 * g.random((M, d))).astype(np.float32),
           de=r(N // C, M, C, d), dtw=r(N, M), drop_key=0x1234, seed_fwd=77)
  if zero_row is not None:
    c['text'][zero_row] = 0.0
    c['b1'][:] = 0.0
  return c


def moe_input(c, fm, dtype=np.float64):
  """(input of the MoE branch, its dropout factor or None)"""
  if fm['text_moe']:
    return c['text_moe'].astype(dtype), None
  if fm['drop_p'] > 0:
    thr = D.thr16_of(fm['drop_p'])
    mask = moe_mask(c['drop_key'], c['seed_fwd'], c['N'], c['K'], thr, 1.0 / (1.0 - thr / 65536.0))
    return (c['text'].astype(np.float64) * mask).astype(dtype), mask
  return c['text'].astype(dtype), None


def simulate(c, fm, dtype=np.float64, wrong=None):
  """Every buffer the two calls leave behind, each stage evaluated in `dtype` on the stage before's own output: with float64 the
  chained reference, with float32 a stand-in for a kernel.  wrong: one of WRONG, that stage done wrongly."""
  f = lambda k: c[k].astype(dtype)
  C, use_bn, training = c['C'], c['use_bn'], c['training']
  text = f('text')
  b = {}
  if wrong == 'contraction_short' and c['K'] > 8:
    b['y'] = v_fc1(text[:, :-8], f('W1')[:, :, :-8], f('b1'))
  else:
    b['y'] = v_fc1(text, f('W1'), f('b1'))
  b['x1'] = v_fc2(b['y'], f('W2'), f('b2'))
  b['rm'], b['rv'] = f('rm'), f('rv')
  if use_bn and training:
    b['mean'], b['rstd'], varu = v_batch_stats(b['x1'], unbiased_norm=wrong == 'unbiased_norm', no_eps=wrong == 'no_eps',
                                               drop_last_row=wrong == 'bn_sum_short')
    b['rm'], b['rv'] = v_running_update(b['rm'], b['mean']), v_running_update(b['rv'], varu)
  elif use_bn:
    b['mean'], b['rstd'] = f('rm'), v_running_rstd(f('rv'), no_eps=wrong == 'no_eps')
  else:
    b['mean'] = b['rstd'] = None
  st = (b['y'], b['x1'], b['mean'], b['rstd'], f('gamma'), f('beta'), use_bn)
  b['e'] = to_bmcd(v_embed(*st), C, wrong_order=wrong == 'bcmd_order')
  x, mask = moe_input(c, fm, dtype)
  if fm['moe']:
    b['tw'] = v_moe(x, f('moe_w'), f('moe_b'), drop_expert=wrong == 'softmax_short', no_l1=wrong == 'no_l1')
  # backward
  dyg, _, b['dx1'], gg, gb = v_gate_bwd(from_bmcd(f('de'), C), *st, training, no_proj=wrong == 'no_proj',
                                        no_inv_n=wrong == 'no_inv_n')
  if use_bn:
    b['g_bn_gamma'], b['g_bn_beta'] = gg, gb
  b['g_b2'] = b['dx1'].sum(0)
  if wrong == 'contraction_short' and c['K'] <= 8:
    b['g_w2'] = v_wgrad(b['dx1'][:-8], b['y'][:-8])
  else:
    b['g_w2'] = v_wgrad(b['dx1'], b['y'])
  b['dy'] = v_dy(dyg, b['dx1'], f('W2'))
  b['g_b1'] = b['dy'].sum(0)
  b['g_w1'] = v_wgrad(b['dy'], text)
  if fm['dtext']:
    b['dtext'] = v_dtext(b['dy'], f('W1'))
  if fm['moe']:
    b['dlogit'] = v_dlogit(b['tw'], f('dtw'))
    b['g_moe_w'], b['g_moe_b'] = b['dlogit'].T @ x, b['dlogit'].sum(0)
    din = b['dlogit'] @ f('moe_w')
    if mask is not None:
      din = din * mask.astype(dtype)
    if fm['dtext_moe'] and wrong != 'moe_to_dtext':
      b['dtext_moe'] = din
    else:
      if fm['dtext_moe']:
        b['dtext_moe'] = np.zeros_like(din)
      if fm['dtext']:
        b['dtext'] = b['dtext'] + din
  for name in PARAMS:
    k = 'g_' + name
    if k in b:
      b[k] = [b[k][m] if wants(fm, name, m) else None for m in range(c['M'])]
  return b


# wrong version -> does it apply to (case, form)?  One of them cannot be told from the right one: see no_l1.
WRONG = {
    'bn_sum_short': lambda c, fm: c['use_bn'] and c['training'] and c['N'] > 1,      # last text row left out of a column sum
    'contraction_short': lambda c, fm: c['K'] > 8 or c['N'] > 8,                      # last 8 values of a contraction dropped
    'unbiased_norm': lambda c, fm: c['use_bn'] and c['training'] and c['N'] > 1,     # unbiased variance in the normalisation
    'no_eps': lambda c, fm: bool(c['use_bn']),
    'no_proj': lambda c, fm: True,                                                    # projection term of the normalise backward
    'no_inv_n': lambda c, fm: c['use_bn'] and c['training'] and c['N'] > 1,          # 1 / N of the BatchNorm backward
    'bcmd_order': lambda c, fm: c['C'] > 1 and c['M'] > 1,                            # (B, C, M, d) written
    'softmax_short': lambda c, fm: fm['moe'] and c['M'] > 1,                          # one expert left out of the softmax
    'moe_to_dtext': lambda c, fm: fm['moe'] and fm['dtext_moe'] and fm['dtext'],     # MoE input gradient in the wrong buffer
    # the L1 normalise of a softmax over the same axis divides by a sum that IS one: leaving it out changes the last bit at
    # most, and no bound can tell (model.py:270/280 take the softmax over the experts, :618 normalises over the experts)
    'no_l1': lambda c, fm: False,
}

FN_STAGES = {'mean': 3, 'rstd': 3, 'running_var': 3, 'e': 4, 'tw': 5, 'dx1': 6, 'g_bn_gamma': 6, 'g_bn_beta': 6, 'dy': 7}


def verify(c, fm, b, backward=True):
  """b: the buffers of a device (or of simulate) -> {name: (|b - stage reference| , bound pair)}, every stage fed with b's own
  previous-stage values.  Lists of per-expert gradients are checked expert by expert where they are given."""
  f = lambda k: np.asarray(b[k], dtype=np.float64)
  p = lambda k: c[k].astype(np.float64)
  C, M, use_bn, training = c['C'], c['M'], c['use_bn'], c['training']
  out = {}

  def put(name, got, r_val, r_bnd):
    out[name] = (np.abs(np.asarray(got, dtype=np.float64) - r_val), r_bnd)

  def put_g(name, r_val, r_bnd):
    for m in range(M):
      if b['g_' + name][m] is not None:
        put('g_%s[%d]' % (name, m), b['g_' + name][m], r_val[m], r_bnd[:, m])

  r = s_fc1(p('text'), p('W1'), p('b1'))
  put('y', b['y'], r.val, r.bnd)
  r = s_fc2(f('y'), p('W2'), p('b2'))
  put('x1', b['x1'], r.val, r.bnd)
  mean = rstd = None
  if use_bn:
    mean, rstd = f('mean'), f('rstd')
    if training:
      r = s_batch_stats(f('x1'))
      put('mean', mean, r.mean, r.dmean)
      put('rstd', rstd, r.rstd, r.drstd)
      u = s_running_update(p('rm'), mean)
      put('running_mean', b['rm'], u.val, u.bnd)
      u = s_running_update(p('rv'), r.varu, r.dvaru)
      put('running_var', b['rv'], u.val, u.bnd)
    else:
      put('mean', mean, p('rm'), lin(np.zeros_like(mean)))
      r = s_running_rstd(p('rv'))
      put('rstd', rstd, r.val, r.bnd)
  if not (use_bn and training):
    put('running_mean', b['rm'], p('rm'), lin(np.zeros_like(p('rm'))))
    put('running_var', b['rv'], p('rv'), lin(np.zeros_like(p('rv'))))
  st = (f('y'), f('x1'), mean, rstd, p('gamma'), p('beta'), use_bn)
  r = s_embed(*st)
  put('e', b['e'], to_bmcd(r.val, C), np.stack([to_bmcd(r.bnd[0], C), to_bmcd(r.bnd[1], C)]))
  x, mask = moe_input(c, fm)
  if fm['moe']:
    r = s_moe(x, p('moe_w'), p('moe_b'), extra=1 if mask is not None else 0)
    put('tw', b['tw'], r.val, r.bnd)
  if not backward:
    return out
  r = s_gate_bwd(from_bmcd(p('de'), C), *st, training)
  put('dx1', b['dx1'], r.dx1, r.ddx1)
  if use_bn:
    put_g('bn_gamma', r.g_gamma, r.dg_gamma)
    put_g('bn_beta', r.g_beta, r.dg_beta)
  dx1 = f('dx1')
  q = s_colsum(dx1)
  put_g('b2', q.val, q.bnd)
  q = s_wgrad(dx1, f('y'))
  put_g('w2', q.val, q.bnd)
  q = s_dy(r.dyg, r.ddyg, dx1, p('W2'))
  put('dy', b['dy'], q.val, q.bnd)
  dy = f('dy')
  q = s_colsum(dy)
  put_g('b1', q.val, q.bnd)
  q = s_wgrad(dy, p('text'))
  put_g('w1', q.val, q.bnd)
  din = None
  if fm['moe']:
    q = s_dlogit(f('tw'), p('dtw'))
    put('dlogit', b['dlogit'], q.val, q.bnd)
    dl = f('dlogit')
    gw, gb = s_moe_wgrad(dl, q.bnd, x)
    put_g('moe_w', gw.val, gw.bnd)
    put_g('moe_b', gb.val[:, None], gb.bnd[:, :, None])
    din = s_moe_dinput(dl, p('moe_w'), mask)
    if fm['dtext_moe']:
      put('dtext_moe', b['dtext_moe'], din.val, din.bnd)
      din = None
  if fm['dtext']:
    q = s_dtext(dy, p('W1'), din)
    put('dtext', b['dtext'], q.val, q.bnd)
  return out


def worst(res, allowance=None):
  """{name: (worst error / bound, measured function error in ulps per evaluation)}.  The second figure charges an element's
  WHOLE error to the approximated functions, error / (2^-23 fn), over the elements where one ulp per evaluation outweighs the
  derived roundings (2^-23 fn >= base), so that the figure is about the functions; nan where a stage has no such element."""
  o = {}
  for name, (err, bnd) in res.items():
    tot = bound(bnd, allowance)
    with np.errstate(divide='ignore', invalid='ignore'):
      ratio = np.where(tot > 0, err / tot, np.where(err > 0, np.inf, 0.0))
      dom = (bnd[1] > 0) & (ULP * bnd[1] >= bnd[0]) & np.isfinite(err)
      ulps = np.where(dom, err / (ULP * bnd[1]), 0.0)
    o[name] = (float(ratio.max()), float(ulps.max()) if dom.any() else float('nan'))
  return o


def failures(res, allowance=None):
  return sorted(name for name, (ratio, _) in worst(res, allowance).items() if not ratio <= 1.0)


# ---- the cases of the GPU test (and of the CPU checks of the bounds): (N, C, M, d, K, use_bn, training, logit spread) ----------

SMALL_CASES = [
    (1, 1, 1, 32, 32, 0, 1, 0),        # smallest accepted shape; 12 of 16 waves idle in both split-K slices
    (1, 1, 3, 32, 64, 1, 1, 0),        # N = 1 with batch statistics (variance 0); N M % 4 != 0
    (2, 2, 16, 64, 64, 1, 1, 0),       # M at its maximum; one batch item with C = 2: the (B, M, C, d) order is visible
    (17, 1, 5, 544, 544, 1, 1, 40),    # k_slice 40: last working wave has 24 values, two idle; ct = 17; 85 rows
    (31, 1, 3, 96, 992, 1, 0, 0),      # last tile row dead; d no multiple of 64; wave 15's K slice short; eval statistics
    (9, 3, 7, 512, 768, 0, 1, 0),      # the 'gem' form on the wide shape
    (32, 4, 2, 1024, 1024, 1, 1, 0),   # every limit at once
]
GENERAL_CASES = [
    (33, 3, 3, 32, 32, 1, 1, 80),      # first N past the gate
    (8, 2, 2, 36, 50, 1, 1, 0),        # small N off the shape gate; row stride 50: scalar loads and K tails
    (130, 1, 2, 40, 130, 1, 0, 0),     # weight-gradient contraction over N >= 128 with a short last slice; eval
    (520, 8, 16, 4, 4, 0, 1, 0),       # N M = 8320 > 8192: the capped grid loops; d at its minimum
    (40, 1, 3, 1024, 1100, 1, 1, 0),   # d at its maximum, K past 1024
]
FORM_SHAPES = {'small': (17, 1, 5, 544, 544, 1, 1, 40), 'general': (8, 2, 2, 36, 50, 1, 1, 0)}
FORMS = {
    'a': form(),
    'b': form(text_moe=True, dtext_moe=True),
    'c': form(text_moe=True),
    'd_a': form(dtext=False),
    'd_b': form(text_moe=True, dtext=False, dtext_moe=True),
    'e': form(moe=False),
    'f': form(drop_p=0.1, dtext_moe=True),          # small path only
    'g': form(g_null='all'),
    'h': form(g_null=tuple((name, 1) for name in PARAMS)),
}


def case_of(spec, **kw):
  N, C, M, d, K, use_bn, training, spread = spec
  return make_case(N, C, M, d, K, use_bn, training, logit_spread=float(spread), **kw)
