"""fp64 reference of the fused attention (mmt_amd/csrc/attention.hip), a first-order model of the kernels' rounding error,
inputs whose tile-edge rows are loud, and the mutants that show what the bound can see.  numpy and CPU torch only; its own
checks are tests/test_attention_ref_cpu.py, the kernels are judged with it in tests/test_attention_bounds_gpu.py.

Reference.  Per sample and head, with s = q k^T scale + key bias:
  P = softmax(s)   A = P o keep drop_scale   ctx = A v   dA = dO v^T   delta = rowsum(dO o ctx)
  dS = P o (keep drop_scale dA - delta)   dQ = scale dS k   dK = scale dS^T q   dV = A^T dO
lse and ctx of the full reference come from engine_paths_ref.attention_rows; everything else is written out here.

Error model (first order).  u = 2^-9 is HALF the unit roundoff of pack_bf2's round-to-nearest-even bf16 (8 significant bits:
a relative error between 0 and 2^-8, 2^-9 at the top of a binade): the model charges every bf16 rounding at half its worst
case, and FACTOR x the model below is the first-order worst case itself.  Read from attention.hip:
the inputs are exact bf16; scores and dA accumulate in fp32 on the MFMA; A and dS are rounded to bf16 by pack8 before the
second MFMA; the softmax row sum l_run is summed from the unrounded fp32 exponentials; delta is formed from the kernel's OWN
bf16 ctx (attn_delta_kernel); every output is rounded once to bf16 (store_block16).
  ctx      u (A |V|) + u |ctx|
  dV       u (A^T |dO|) + u |dV|
  E_delta  sum_d |dO[q, d]| (u (A |V|)[q, d] + u |ctx[q, d]|)          the error delta inherits from ctx
  E_dS     u |dS| + P o E_delta
  dQ       scale (E_dS |K|) + u |dQ|
  dK       scale (E_dS^T |Q|) + u |dK|
  lse      2^-23 (C_X max_k |x| + C_SUM n_tiles + C_LOG + |lse|),  x = s scale log2(e) over the unmasked keys
The ASSERTED bound is FACTOR = 2 times the model, for every output alike, and it is the only free number.  For the bf16
outputs it lifts u to the unit roundoff; second-order terms and the fp32 accumulation (2^-24 per addition) are left to the
fact that the worst cases of the many roundings in a sum do not coincide (tests/test_attention_ref_cpu.py: the emulated
rounding uses at most 0.82 of the bound); for lse, whose model counts worst cases already, it is room for the MFMA's fp32
accumulation of the scores.  Where reference and bound are both exactly 0 (dK / dV of a masked key)
`within` leaves no room: the kernel's value must be exactly 0.
"""
import functools
import math

import numpy as np
import torch

from tests import dropout_ref as D
from tests import engine_paths_ref as R

U16 = 2.0**-9    # half the unit roundoff of bf16 (module docstring)
ULP32 = 2.0**-23  # one ulp of an fp32 number in [1, 2): two unit roundoffs
FACTOR = 2.0     # asserted bound = FACTOR x the first-order model (module docstring)
LOG2E = math.log2(math.e)
SITE_KEY = 0xa5a51234  # dropout site key of the attention calls (top bit set: an unsigned word)
MASKED = -10000.0

# lse = (m_run + log2f(l_run)) LN2 is all fp32.  With x_k = s_k scale log2(e) the kernel's exponent of key k, the exact
# function of the COMPUTED x is y = log2 sum_k 2^x_k, and |dy| <= max_k |dx_k| (the weights dy / dx_k = P_k sum to one).
# Counting unit roundoffs (2^-24, half of ULP32) and converting to natural log (times ln 2 = 0.69):
#  C_X (relative to max_k |x| over the unmasked keys): c1 = scale * LOG2E carries the fp32 rounding of `scale` (1), of the
#    constant (<1) and of the product (1); s * c1 + bias is one rounding (an fma, or a product and the exact addition of a
#    live key's bias 0) (1); x - m_new is one rounding of a number below 2 max |x| (2); the arguments m_run - m_new of the
#    tile rescales add up to m_final - m_first <= 2 max |x|, one rounding each (2).  8 roundoffs = 4 ULP32, times ln 2 = 2.8;
#    the 0.03 |lse| that the last line below leaves over is at most 0.03 (max |x| ln 2 + ln n): C_X = 3.
#    (The fp32 accumulation of the exact bf16 products inside the MFMA is not charged here: it is left to FACTOR.)
#  C_SUM (per 64-key tile, relative to l, which enters lse as dl / l): the rescale of what was summed before:
#    alpha = v_exp_f32 (1 ulp = 2 roundoffs), l_run * alpha (1), + psum (1): 4 roundoffs: C_SUM = 2.
#  C_LOG (once): every exponential is v_exp_f32 (2 roundoffs) and goes through the 15 in-lane additions and the two
#    cross-lane additions of its tile's psum (17, worst case): 19 roundoffs = 9.5 ULP32; log2f is good to 1 ulp of
#    log2 l, in natural log ln l <= ln 512 = 6.3 ULP32 (lse_model refuses longer samples): C_LOG = 16.
#  |lse|: m_run + log2f(l_run) (1) and the product with LN2 (1; the constant itself is off by 0.05 roundoffs): 1.03 ULP32.
C_X, C_SUM, C_LOG = 3, 2, 16


def edges(n):
  """Edge positions of a sample of n rows: first, last, and both sides of every 64-row tile boundary inside it."""
  return sorted({0, n - 1} | {e for t in range(64, n, 64) for e in (t - 1, t)})


def bf16(x):
  """float64 numpy -> nearest bf16, back as float64."""
  return torch.from_numpy(np.ascontiguousarray(x)).to(torch.bfloat16).double().numpy()


def _heads(x, H):
  """[n, H DH] -> [H, n, DH]"""
  n, d = x.shape
  return x.reshape(n, H, d // H).transpose(1, 0, 2)


def _rows(x):
  """[H, n, DH] -> [n, H DH]"""
  H, n, dh = x.shape
  return x.transpose(1, 0, 2).reshape(n, H * dh)


# ---- the cases -----------------------------------------------------------------------------------------------------------

DENSE_S = (1, 16, 17, 63, 64, 65, 127, 128, 129, 192, 193, 257)
VARLEN = {193: (1, 64, 129, 193), 130: (63, 65, 128)}  # S: the lengths of the packed samples


def _cases():
  c = {}
  for S in DENSE_S:
    c['dense-S%d' % S] = dict(S=S, B=2, p=0.0)
  for S in (64, 65, 193):
    c['dense-S%d-p0.1' % S] = dict(S=S, B=2, p=0.1)
  for S, lens in VARLEN.items():
    for p in (0.0, 0.1):
      c['varlen-S%d%s' % (S, '-p0.1' if p else '')] = dict(S=S, B=len(lens), lens=lens, p=p)
  c['packed-S130-p0.1'] = dict(S=130, B=3, lens=VARLEN[130], p=0.1, packed=True)
  for nq in (64, 65):
    c['rows-S129-nq%d' % nq] = dict(S=129, B=2, p=0.0, nq=nq)
  return c


CASES = _cases()  # (the scheduled backward runs 'varlen-S193-p0.1': B H = 8)
DHS = (128, 64)
H = 2


@functools.lru_cache(maxsize=None)
def problem(case, DH, amp2=3.0, dgain=8.0):
  """Inputs of a case: unit-variance Gaussians (fixed seed); amp c[h] added to every Q row and to the K rows at the edge
  positions, amp = sqrt(amp2 / scale), so that an edge key scores about amp2 above an ordinary one; the dctx rows at the
  edge positions times dgain; all rounded to bf16.  Ordinary keys are masked with probability 0.3, edge keys never (row 0 is
  an edge: every sample keeps a live key).  packed: row_index scatters the packed rows over sorted original positions;
  nq: qsel = the edge rows and random others per sample, unsorted, and dctx is compact [B nq, d]."""
  P = dict(CASES[case])
  S, B, p = P['S'], P['B'], P['p']
  d, scale = H * DH, 1.0 / math.sqrt(DH)
  lens = P.get('lens', (S,) * B)
  cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
  rows = int(cu[-1])
  g = torch.Generator().manual_seed(7000 + 13 * sorted(CASES).index(case) + DH)
  qkv = torch.randn(rows, 3 * d, generator=g, dtype=torch.float64)
  dctx = torch.randn(rows, d, generator=g, dtype=torch.float64)
  c = torch.randn(H, DH, generator=g, dtype=torch.float64)
  c = (c / c.norm(dim=-1, keepdim=True) * math.sqrt(amp2 / scale)).reshape(1, d)
  valid = torch.rand(rows, generator=g) > 0.3
  edge_rows = np.concatenate([cu[b] + np.array(edges(lens[b])) for b in range(B)])
  qkv[:, :d] += c
  qkv[edge_rows, d:2 * d] += c
  dctx[edge_rows] *= dgain
  valid[edge_rows] = True
  row_index = None
  if P.get('packed'):
    row_index = np.concatenate([np.sort(torch.randperm(S, generator=g)[:lens[b]].numpy()) + b * S for b in range(B)]).astype(np.int64)
  qsel, nq = None, P.get('nq')
  if nq:
    sel = []
    for b in range(B):
      e = np.array(edges(lens[b]))
      rest = np.setdiff1d(np.arange(lens[b]), e)
      more = rest[torch.randperm(len(rest), generator=g)[:nq - len(e)].numpy()]
      both = np.concatenate([e, more])
      sel.append(cu[b] + both[torch.randperm(nq, generator=g).numpy()])
    qsel = np.concatenate(sel)
    dctx = dctx[qsel]
  thr, drop_scale = D.thr16_of(p), 1.0
  keep = None
  if thr:
    drop_scale = 1.0 / (1.0 - thr / 65536.0)
    keep = D.attn_mask(D.eff_key(SITE_KEY, None), B, H, S, thr)
  P.update(case=case, DH=DH, H=H, d=d, scale=scale, lens=lens, cu=cu, rows=rows, varlen='lens' in CASES[case],
           qkv=qkv.to(torch.bfloat16), dctx=dctx.to(torch.bfloat16), bias=(~valid).double() * MASKED, row_index=row_index,
           qsel=qsel, nq=nq, thr=thr, drop_scale=drop_scale, keep=keep)
  return P


def _sample_inputs(P, b):
  """(q [H, nq, DH], k, v [H, n, DH], dO [H, nq, DH], bias [n], keep [H, nq, n] or None, local query positions) of sample b."""
  o, n, d, S = int(P['cu'][b]), P['lens'][b], P['d'], P['S']
  x = P['qkv'][o:o + n].double().numpy()
  if P['nq']:
    ql = P['qsel'][b * P['nq']:(b + 1) * P['nq']] - o
    do = P['dctx'][b * P['nq']:(b + 1) * P['nq']].double().numpy()
  else:
    ql = np.arange(n)
    do = P['dctx'][o:o + n].double().numpy()
  keep = None
  if P['keep'] is not None:
    pos = np.arange(n) if P['row_index'] is None else P['row_index'][o:o + n] - b * S
    keep = P['keep'][b][:, pos[ql]][:, :, pos]
  return (_heads(x[ql, :d], H), _heads(x[:, d:2 * d], H), _heads(x[:, 2 * d:], H), _heads(do, H), P['bias'][o:o + n].numpy(),
          keep, ql)


def attention_sample(q, k, v, do, bias, scale, keep, drop_scale, lse=None, no_key=None, no_query=None, rounded=False):
  """One sample in float64 (module docstring); all heads at once.  lse: take the softmax's normaliser from the caller.
  no_key / no_query: the mutants -- the sample without that key (its score is -inf) or with that query's contributions to
  dK and dV removed.  rounded: the kernels' bf16 rounding points (A, ctx, delta from that ctx, dS, the outputs), everything
  else exact.  -> dict of lse [H, nq], P / A / dA / dS [H, nq, n], ctx / dQ [H, nq, DH], dK / dV [H, n, DH]."""
  rd = bf16 if rounded else (lambda t: t)
  s = q @ k.transpose(0, 2, 1) * scale + bias[None, None, :]
  if no_key is not None:
    s[:, :, no_key] = -np.inf
  if lse is None:
    m = s.max(-1)
    lse = m + np.log(np.exp(s - m[..., None]).sum(-1))
  P = np.exp(s - lse[..., None])
  kd = drop_scale if keep is None else keep * drop_scale
  A = rd(P * kd)
  ctx = rd(A @ v)
  dA = do @ v.transpose(0, 2, 1)
  delta = (do * ctx).sum(-1)
  dS = rd(P * (kd * dA - delta[..., None]))
  dQ = rd(scale * (dS @ k))
  Ak, dSk = A, dS
  if no_query is not None:
    Ak, dSk = A.copy(), dS.copy()
    Ak[:, no_query], dSk[:, no_query] = 0.0, 0.0
  dK = rd(scale * (dSk.transpose(0, 2, 1) @ q))
  dV = rd(Ak.transpose(0, 2, 1) @ do)
  return dict(lse=lse, P=P, A=A, dA=dA, dS=dS, ctx=ctx, dQ=dQ, dK=dK, dV=dV)


def lse_model(q, k, bias, scale, lse):
  """First-order error of the fp32 lse [H, nq] (constants: top of the file), before FACTOR."""
  n = k.shape[1]
  assert n <= 512, 'C_LOG counts ln l <= ln 512'
  x = np.abs(q @ k.transpose(0, 2, 1))[:, :, bias == 0].max(-1) * scale * LOG2E
  return ULP32 * (C_X * x + C_SUM * ((n + 63) // 64) + C_LOG + np.abs(lse))


def bounds_sample(r, q, k, v, do, bias, scale):
  """FACTOR x the first-order model for every output of one sample (r = attention_sample's dict)."""
  av = r['A'] @ np.abs(v)
  ctx = U16 * av + U16 * np.abs(r['ctx'])
  e_delta = (np.abs(do) * ctx).sum(-1)
  e_ds = U16 * np.abs(r['dS']) + r['P'] * e_delta[..., None]
  m = dict(ctx=ctx, dV=U16 * (r['A'].transpose(0, 2, 1) @ np.abs(do)) + U16 * np.abs(r['dV']),
           dQ=scale * (e_ds @ np.abs(k)) + U16 * np.abs(r['dQ']),
           dK=scale * (e_ds.transpose(0, 2, 1) @ np.abs(q)) + U16 * np.abs(r['dK']),
           lse=lse_model(q, k, bias, scale, r['lse']))
  return {name: FACTOR * t for name, t in m.items()}


OUTPUTS = ('lse', 'ctx', 'dQ', 'dK', 'dV')


def _flat(name, t):
  return t.T if name == 'lse' else _rows(t)  # lse [H, nq] -> [nq, H]


@functools.lru_cache(maxsize=None)
def reference(case, DH, amp2=3.0, dgain=8.0):
  """-> dict(P=problem, samples=[per sample: inputs, attention_sample's dict, bounds], ref / bound = {output: [rows, .]}).
  ctx / lse / dQ have one row per query (compact for the rows-only cases), dK / dV one per key row."""
  P = problem(case, DH, amp2, dgain)
  x64, b64 = P['qkv'].double(), P['bias']
  samples = []
  for b in range(P['B']):
    o, n = int(P['cu'][b]), P['lens'][b]
    inp = _sample_inputs(P, b)
    q, k, v, do, bias, keep, ql = inp
    ri = None if P['row_index'] is None else P['row_index'] - b * P['S']
    ctx, lse = R.attention_rows(x64, b64, 1, P['S'], H, P['scale'], o + ql, len(ql), cu=[o, o + n],
                                keep=None if P['keep'] is None else P['keep'][b:b + 1], drop_scale=P['drop_scale'], row_index=ri)
    r = attention_sample(q, k, v, do, bias, P['scale'], keep, P['drop_scale'], lse=lse.numpy().T)
    r['ctx_av'] = r['ctx']  # (tests/test_attention_ref_cpu.py: A v is attention_rows' ctx)
    r['ctx'] = _heads(ctx.numpy(), H)
    samples.append(dict(inp=inp, r=r, bound=bounds_sample(r, q, k, v, do, bias, P['scale']), n=n, o=o))
  cat = lambda key: {name: np.concatenate([_flat(name, s[key][name]) for s in samples]) for name in OUTPUTS}
  return dict(P=P, samples=samples, ref=cat('r'), bound=cat('bound'))


def mutant(ref, b, e, kind):
  """Sample b of the reference evaluated without key e (kind 'key': ctx, lse, dQ change) or without query e ('query': dK,
  dV change).  -> {output: [rows of the sample, .]}"""
  P, s = ref['P'], ref['samples'][b]
  q, k, v, do, bias, keep, _ = s['inp']
  r = attention_sample(q, k, v, do, bias, P['scale'], keep, P['drop_scale'], **{'no_' + kind: e})
  return {name: _flat(name, r[name]) for name in (('lse', 'ctx', 'dQ') if kind == 'key' else ('dK', 'dV'))}


def emulate(ref):
  """The kernels' bf16 rounding points applied to the fp64 formulas, and lse evaluated the kernel's way in fp32 numpy (64-key
  tiles, running maximum, exp2).  -> {output: [rows, .]}"""
  P, out = ref['P'], []
  for s in ref['samples']:
    q, k, v, do, bias, keep, _ = s['inp']
    r = attention_sample(q, k, v, do, bias, P['scale'], keep, P['drop_scale'], rounded=True)
    f = np.float32
    c1 = f(f(P['scale']) * f(LOG2E))
    x = (q @ k.transpose(0, 2, 1)).astype(f) * c1 + (bias.astype(f) * f(LOG2E))[None, None, :]
    m, l = np.full(x.shape[:2], -1e30, dtype=f), np.zeros(x.shape[:2], dtype=f)
    for t in range(0, x.shape[2], 64):
      mn = np.maximum(m, x[:, :, t:t + 64].max(-1))
      l = l * np.exp2(m - mn) + np.exp2(x[:, :, t:t + 64] - mn[..., None]).sum(-1, dtype=f)
      m = mn
    r['lse'] = ((m + np.log2(l)) * f(math.log(2.0))).astype(np.float64)
    out.append(r)
  return {name: np.concatenate([_flat(name, r[name]) for r in out]) for name in OUTPUTS}


def judge(name, got, want, bound):
  """-> (largest |got - want| / bound, '' or what is wrong): |got - want| <= bound elementwise, and an element whose bound is
  0 must be equal.  Prints the figure."""
  got, want, bound = (np.asarray(t, dtype=np.float64) for t in (got, want, bound))
  assert got.shape == want.shape == bound.shape, '%s: shapes %s %s %s' % (name, got.shape, want.shape, bound.shape)
  if not np.isfinite(got).all():
    return np.inf, '%s: Inf or NaN in the output' % name
  err = np.abs(got - want)
  pos = bound > 0
  used = float((err[pos] / bound[pos]).max()) if pos.any() else 0.0
  print('%s: error / bound %.3f (largest error %.3g)' % (name, used, float(err.max()) if err.size else 0.0))
  bad = err > bound
  if not bad.any():
    return used, ''
  return used, '%s: %d of %d beyond the bound (up to %.3g of it, %d where the bound is 0); first at %s' % (
      name, int(bad.sum()), bad.size, used, int((bad & ~pos).sum()), np.argwhere(bad)[:6].tolist())


def within(name, got, want, bound):
  used, wrong = judge(name, got, want, bound)
  assert not wrong, wrong
  return used
