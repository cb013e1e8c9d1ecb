"""fp64 restatement of the row-sharded similarity + max-margin loss (mmt_amd/large_sim.py, the first half of largesim.hip),
written from oracle/mmt_oracle.py (cross_view_rows, max_margin_rows, max_margin_ranking_loss) and the header comments of
largesim.hip.  Plain torch on the CPU in float64; nothing of mmt_amd is imported.  A row block is b text rows (global rows
r0 .. r0 + b) against all n videos with M experts; the kernels take the raw fp32 numerators of the similarity GEMM, so every
input here is fp32 data and every hinge decision of a correct kernel is determined wherever |h| exceeds `band`.

tests/test_large_sim_ref_cpu.py proves this file (against the oracle, and that the inputs leave nothing in band) without a GPU;
tests/test_large_sim_mm_gpu.py judges the kernels with it."""
import functools

import numpy as np
import torch

U = 2.0 ** -24      # unit round-off of fp32
CPB = 8192          # columns per block of the sweeps (largesim.hip LS_CPB): the granularity of loss_part and gs_part
MARGIN = float(np.float32(0.05))

# (b, n, r0, M): the smallest shapes that reach each edge of the sweeps
CASES = [
    (4, 4, 0, 1),            # one thread holds the whole block; every row on the checked path; b < TR
    (43, 2560, 256, 7),      # a partial last row tile at TR = 16 and TR = 8
    (21, 9220, 8185, 12),    # M > 8 (TR 8 / 4); two column blocks, last chunk of 4 columns; odd r0; diagonal crosses column 8192
    (19, 1028, 1009, 8),     # M = 8 | 9: the template boundary; r0 + b == n; diagonal crosses column 1024
    (19, 1028, 1009, 9),
    (37, 2052, 1003, 16),    # M = MMT_MAX_EXPERTS; diagonal crosses column 1024; three row tiles at TR = 16
]


def ncb(n):
  return (n + CPB - 1) // CPB


def inv_norm32(n, fix_norm=True):
  """1 / norm as the fp32 value the C ABI receives."""
  return float(np.float32(1.0 / (2.0 * n * (n - 1) if fix_norm else 2.0 * n * n)))


def den_of(tw, vw):
  """(den [b, n] with 1e-5 where the weights give 0 (model.py:816), the mask of those elements), fp64."""
  den = tw.double() @ vw.double().t()
  zero = den == 0
  return torch.where(zero, torch.full_like(den, 1e-5), den), zero


@functools.lru_cache(maxsize=None)
def inputs(case, seed=5):
  """dict(raw [b, n], tw [b, M], vw [n, M], diag [n]) in fp32 + margin: a zero-weight video (column 5) and a zero-weight text
  (row 2); where den == 0 the numerators are scaled by 1e-5, so that the 1e-5 branch yields similarities of ordinary size.
  The softmax is taken in fp64 and rounded once, so that the bits do not depend on the host's vector exp."""
  b, n, r0, M = case
  g = torch.Generator().manual_seed(seed)
  raw = torch.randn(b, n, generator=g) * 0.05
  tw = torch.softmax(torch.randn(b, M, generator=g).double(), -1).float()
  vw = torch.softmax(torch.randn(n, M, generator=g).double(), -1).float()
  if n > 5:
    vw[5] = 0.0
  if b > 2:
    tw[2] = 0.0
  diag = torch.randn(n, generator=g) * 0.05
  _, zero = den_of(tw, vw)
  raw = torch.where(zero, raw * 1e-5, raw)
  return dict(b=b, n=n, r0=r0, M=M, raw=raw, tw=tw, vw=vw, diag=diag, margin=MARGIN)


def similarities(raw, tw, vw):
  den, _ = den_of(tw, vw)
  return raw.double() / den


def hinges(s, diag, r0, margin):
  """(h1 = margin - s_rr + s_rc: the row's hinge, h2 = margin - s_cc + s_rc: the column's, off: the off-diagonal mask)."""
  b, n = s.shape
  d = diag.double()
  h1 = margin - d[r0:r0 + b][:, None] + s
  h2 = margin - d[None, :] + s
  off = torch.ones(b, n, dtype=torch.bool)
  off[torch.arange(b), r0 + torch.arange(b)] = False
  return h1, h2, off


def band(h, ms_or_md, s, M):
  """|fp32 hinge - fp64 hinge| of a correct kernel, doubled: den is an fma chain of M non-negative terms (M u relative), the
  reciprocal 1 ulp (2 u) and the multiply u -> (M + 3) u |s|; margin - diag rounds once (u |ms|) and the final add once (u |h|,
  to first order).  A decision can differ from the fp64 one only where |h| <= band."""
  return 2.0 * U * (ms_or_md.abs() + (M + 3) * s.abs() + h.abs())


def bands(x, s=None):
  """(band of h1, band of h2, h1, h2, off) of an input dict (s: the similarities, if they do not come from x['raw'])."""
  s = similarities(x['raw'], x['tw'], x['vw']) if s is None else s
  b, r0, M = x['b'], x['r0'], x['M']
  h1, h2, off = hinges(s, x['diag'], r0, x['margin'])
  d = x['diag'].double()
  ms = (x['margin'] - d[r0:r0 + b])[:, None].expand_as(s)
  md = (x['margin'] - d)[None, :].expand_as(s)
  return band(h1, ms, s, M), band(h2, md, s, M), h1, h2, off


def _blocks(x):
  """[b, n] -> [b, ncb]: sums over each block of CPB columns."""
  b, n = x.shape
  pad = ncb(n) * CPB - n
  return torch.nn.functional.pad(x, (0, pad)).view(b, ncb(n), CPB).sum(-1)


def counts(s, diag, r0, margin):
  """(rowcnt [b], colcnt [n]: this block's share of every column's count, loss_part [b, ncb]: the UN-normalised hinge sums per
  row and block of 8192 columns).  The diagonal element carries no hinge."""
  h1, h2, off = hinges(s, diag, r0, margin)
  p1, p2 = (h1 > 0) & off, (h2 > 0) & off
  part = _blocks(torch.where(p1, h1, torch.zeros_like(h1)) + torch.where(p2, h2, torch.zeros_like(h2)))
  return p1.sum(1), p2.sum(0), part


def loss_part_tol(x, s=None):
  """Bound of |kernel loss_part - counts(...)[2]| [b, ncb]: the active hinges' bands + 72 u sum |h| (a thread adds two hinges for
  each of its 4 columns of a block's 8 chunks: 64 additions; then 6 butterfly steps and 2 adds across the 4 waves)."""
  b1, b2, h1, h2, off = bands(x, s)
  p1, p2 = (h1 > 0) & off, (h2 > 0) & off
  z = torch.zeros_like(h1)
  return _blocks(torch.where(p1, b1, z) + torch.where(p2, b2, z)) + 72 * U * _blocks(torch.where(p1, h1, z) + torch.where(p2, h2, z))


def grad(s, den, diag, r0, margin, rowcnt, colcnt_total, inv_norm):
  """G' = g / den [b, n]: g = ((h1 > 0) + (h2 > 0)) inv_norm off the diagonal, -(rowcnt[t] + colcnt_total[r0 + t]) inv_norm on it."""
  b = s.shape[0]
  h1, h2, off = hinges(s, diag, r0, margin)
  g = ((h1 > 0).double() + (h2 > 0).double()) * inv_norm
  t = torch.arange(b)
  g[t, r0 + t] = -(rowcnt.double() + colcnt_total.double()[r0:r0 + b]) * inv_norm
  return g / den


def gs_terms(G16, s, vw, zero):
  """[b, n, M]: G' S vw[v][m]; an element on the 1e-5 branch carries no normaliser gradient."""
  e = torch.where(zero, torch.zeros_like(s), G16.double() * s)
  return e[:, :, None] * vw.double()[None, :, :]


def gs_from(G16, s, vw, zero):
  """gs_part [b, ncb, M]: the sum of gs_terms over each block's columns."""
  b, n = s.shape
  t = gs_terms(G16, s, vw, zero)
  return torch.stack([t[:, c:c + CPB].sum(1) for c in range(0, n, CPB)], 1)


def gs_tol(G16, s, vw, zero, M):
  """(44 + M + 4) u sum |terms|: 32 elements per thread, 8 reduction adds and the products; the kernel's own fp32 similarity."""
  t = gs_terms(G16, s, vw, zero).abs()
  n = s.shape[1]
  return (44 + M + 4) * U * torch.stack([t[:, c:c + CPB].sum(1) for c in range(0, n, CPB)], 1)


TIE = (19, 1028, 1009, 4)
TIE_MARGIN = 2.0 ** -4
TIE_ZERO_COLS, TIE_ZERO_ROW = (5, 1020), 2


@functools.lru_cache(maxsize=None)
def tie_case():
  """A dyadic block on which every fp32 operation of the sweeps is exact: the weights are one-hot on expert 0 (den == 1.0,
  its reciprocal 1.0), except two videos on expert 1 and one text on expert 2 (den == 0; their numerators are 0, as the fold
  produces, so s == 0 exactly there); raw and diag are multiples of 2^-6 in [-0.5, 0.5], margin = 2^-4.  About 8 % of the
  elements are set to h1 == 0 and another 8 % to h2 == 0 exactly: `>=` for `>` changes hundreds of counts.  Hinge sums stay
  below 2^12 in units of 2^-6, exact in fp32 in any order."""
  b, n, r0, M = TIE
  g = torch.Generator().manual_seed(17)
  q = lambda *shape, lim: torch.randint(-lim, lim + 1, shape, generator=g).float() / 64.0
  raw = q(b, n, lim=32)
  diag = q(n, lim=24)                                   # (so that diag - margin stays within [-0.5, 0.5])
  pick = torch.rand(b, n, generator=g)
  raw = torch.where(pick < 0.08, (diag[r0:r0 + b] - TIE_MARGIN)[:, None].expand(b, n), raw)                    # h1 == 0
  raw = torch.where((pick >= 0.08) & (pick < 0.16), (diag - TIE_MARGIN)[None, :].expand(b, n), raw)            # h2 == 0
  tw, vw = torch.zeros(b, M), torch.zeros(n, M)
  tw[:, 0], vw[:, 0] = 1.0, 1.0
  for c in TIE_ZERO_COLS:
    vw[c, 0], vw[c, 1] = 0.0, 1.0
  tw[TIE_ZERO_ROW, 0], tw[TIE_ZERO_ROW, 2] = 0.0, 1.0
  _, zero = den_of(tw, vw)
  raw = torch.where(zero, torch.zeros_like(raw), raw)
  return dict(b=b, n=n, r0=r0, M=M, raw=raw, tw=tw, vw=vw, diag=diag, margin=TIE_MARGIN)


def problem(name):
  """Inputs by parametrisation id: 'tie' or the index of a case."""
  return tie_case() if name == 'tie' else inputs(CASES[int(name)])


NAMES = [str(i) for i in range(len(CASES))] + ['tie']


@functools.lru_cache(maxsize=None)
def reference(name, extra_seed=23):
  """Everything the GPU tests compare with, computed once per case and left unchanged: s, den, zero, the counts, their bounds,
  colcnt_total = the block's own counts + a seeded vector in [0, 50] standing for the other ranks', and G'."""
  x = problem(name)
  b, n, r0, M = x['b'], x['n'], x['r0'], x['M']
  den, zero = den_of(x['tw'], x['vw'])
  s = x['raw'].double() / den
  rowcnt, colcnt, part = counts(s, x['diag'], r0, x['margin'])
  b1, b2, h1, h2, off = bands(x, s)
  in_band = int((((h1.abs() <= b1) | (h2.abs() <= b2)) & off).sum())
  others = torch.randint(0, 51, (n,), generator=torch.Generator().manual_seed(extra_seed))
  total = colcnt + others
  inv = inv_norm32(n)
  return dict(x, s=s, den=den, zero=zero, rowcnt=rowcnt, colcnt=colcnt, loss_part=part, loss_tol=loss_part_tol(x, s), h1=h1, h2=h2,
              off=off, in_band=in_band, colcnt_total=total, inv_norm=inv,
              G=grad(s, den, x['diag'], r0, x['margin'], rowcnt, total, inv))


# ---- the host path (RowBlock) at the smallest shapes it accepts -------------------------------------------------------------
HOST_SHAPES = [dict(b=128, n=256, r0=128, M=3, d=128), dict(b=43, n=384, r0=300, M=9, d=128)]
HOST_ZERO_VIDEO, HOST_ZERO_TEXT = 5, 2  # (global video 5; block-local text 2)


@functools.lru_cache(maxsize=None)
def host_inputs(i):
  """CPU-generated, normalised inputs as in test_row_sharded_similarity_and_maxmargin, with video weights that vary, one
  zero-weight video and one zero-weight text of the block.  Texts exist for all n rows (the other ranks'): they give the global
  diagonal.  Every embedding also carries a signed share of one common direction per expert: the similarities then spread
  over +-0.5 instead of +-1/sqrt(d), which thins the hinges near 0 -- the block's similarities come from a bf16 GEMM, so the
  decisions within its error bound of 0 are the ones no reference can settle, and they have to be few (at most 0.1 %)."""
  sh = HOST_SHAPES[i]
  b, n, r0, m, d = sh['b'], sh['n'], sh['r0'], sh['M'], sh['d']
  rs = np.random.RandomState(7)
  f32 = lambda a: torch.from_numpy(a.astype(np.float32))
  nrm = lambda a: torch.nn.functional.normalize(a, dim=-1)
  vid0, txt0 = f32(rs.randn(n, m, d)), f32(rs.randn(n, m, d))
  tw = torch.softmax(torch.from_numpy(rs.randn(n, m)).double(), -1).float()
  vw = torch.softmax(torch.from_numpy(rs.randn(n, m)).double(), -1).float()
  u, av, at = f32(rs.randn(m, d)), f32(rs.randn(n, 1, 1)), f32(rs.randn(n, 1, 1))
  vid = nrm(vid0 + 0.7 * av * u)
  txt = nrm(txt0 + 0.5 * vid + 0.7 * at * u)
  vw[HOST_ZERO_VIDEO] = 0.0
  tw[r0 + HOST_ZERO_TEXT] = 0.0
  return dict(sh, vid=vid, txt=txt, tw=tw, vw=vw, margin=MARGIN)


def fold(x, w):
  """[R, M, d] x [R, M] -> the bf16 GEMM operand [R, M*d] (mmt_ls_fold_bf16)."""
  return (x * w[..., None]).to(torch.bfloat16).reshape(x.shape[0], -1)


def gemm_bound(a16, b16, K):
  """fp32 accumulation of K products in any order: K 2^-23 sum |a b| (two roundings per accumulation)."""
  return K * 2.0 * U * (a16.double().abs() @ b16.double().abs().t())


@functools.lru_cache(maxsize=None)
def host_reference(i):
  """fp64 raw numerators of the folded bf16 operands of host shape i, their GEMM bound, and the global diagonal (fp32)."""
  x = host_inputs(i)
  b, n, r0 = x['b'], x['n'], x['r0']
  t16, v16 = fold(x['txt'], x['tw']), fold(x['vid'], x['vw'])
  raw_all = t16.double() @ v16.double().t()                            # [n, n]: every rank's rows
  den_all, _ = den_of(x['tw'], x['vw'])
  diag = (raw_all / den_all).diagonal().float()
  sl = slice(r0, r0 + b)
  K = x['M'] * x['d']
  return dict(x, t16=t16[sl], v16=v16, raw=raw_all[sl], raw_bound=gemm_bound(t16[sl], v16, K), diag=diag, tw_blk=x['tw'][sl],
              txt_blk=x['txt'][sl])


def host_block(i, raw, diag):
  """An input dict of the section-1 form for host shape i on the raw numerators `raw` [b, n] and the diagonal `diag` [n]."""
  x = host_inputs(i)
  sl = slice(x['r0'], x['r0'] + x['b'])
  return dict(b=x['b'], n=x['n'], r0=x['r0'], M=x['M'], raw=raw, tw=x['tw'][sl], vw=x['vw'], diag=diag, margin=x['margin'])
