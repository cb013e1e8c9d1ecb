"""The two functions of the fused epilogues whose correct output is exactly defined, against independent host references:

* the counter-based dropout masks of every site with a wrapper, bit for bit against tests/dropout_ref.py (written from the
  formulas in mmt_common.h / attention.hip; its own properties: tests/test_dropout_ref_cpu.py);
* GELU and dGELU of the fused GEMM epilogues over EVERY bf16 argument against fp64, with a bound derived from the kernel's
  arithmetic (table tiles) -- the absolute term of the scalar tiles 1 / 2 is the one measured figure, see SCALAR_*_UNITS.

GEMM tiles: 13 / 14 / 18 (gemm2.hip), 21 (gemm3.hip), 24 / 25 (gemm5.hip), 1 / 2 (gemm.hip), 0 = the dispatcher's choice.
gemm5.hip takes K >= 128 only (at K = 64 tiles 24 / 25 are routed to 14 / 13, and the 64-wide tile 25 has no GELU epilogue
at any K), so the cases that are there for gemm5.hip's own epilogue and its own copy of the table load run at K = 128 in
addition to K = 64.
"""
import functools
import math

import numpy as np
import pytest
import torch

from tests import dropout_ref as D

pytestmark = pytest.mark.gpu

TABLE_TILES = [13, 14, 18, 21, 24, 25, 0]
SCALAR_TILES = [1, 2]
SITE_KEY = 0xa5a51234    # (top bit set: the key is an unsigned word)
SEED = 0x9cd41a55        # (seed + 0x632be5ab wraps past 2^32)


def _dev():
  return torch.device('cuda:0')


def _seed_dev(seeded):
  return torch.tensor([SEED - (1 << 32)], dtype=torch.int32, device=_dev()) if seeded else None


def _randn(shape, seed, scale=1.0):
  g = torch.Generator(device='cpu').manual_seed(seed)
  return torch.randn(*shape, generator=g) * scale


def _away_from_zero(shape, seed):
  """sign * (1 + |N(0, 1)|): no element is anywhere near 0, so 'dropped' is exactly 'output == 0'."""
  x = _randn(shape, seed)
  return torch.where(x < 0, x - 1.0, x + 1.0)


def _row_numbers(kind, n):
  """Original row numbers of n packed rows: none, small ones, and ones whose element index passes 2^34 (the high word of the
  64-bit pair index is live without a large tensor)."""
  r = np.arange(n, dtype=np.int64)
  if kind == 'none':
    return r, None
  orow = r * 3 + 5 if kind == 'small' else (1 << 25) + r * 7 + 1
  return orow, torch.from_numpy(orow.astype(np.int32)).to(_dev())


def _same_mask(name, got, want):
  got, want = np.asarray(got, dtype=bool), np.asarray(want, dtype=bool)
  assert got.shape == want.shape, (name, got.shape, want.shape)
  bad = got != want
  if bad.any():
    raise AssertionError('%s: %d of %d mask elements differ from the reference hash (keep rate got %.4f, reference %.4f); '
                         'first at %s' % (name, int(bad.sum()), bad.size, got.mean(), want.mean(), np.argwhere(bad)[:6].tolist()))


def _close_np(name, got, want, atol, rtol):
  got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
  err = np.abs(got - want)
  bad = err > atol + rtol * np.abs(want)
  if bad.any():
    raise AssertionError('%s: %d of %d beyond atol %g rtol %g, max err %.4g; first at %s'
                         % (name, int(bad.sum()), bad.size, atol, rtol, err.max(), np.argwhere(bad)[:6].tolist()))


# ---- dropout, GEMM sites ---------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _gemm_problem(M, N, K):
  """Operands and the fp64 value of a b^T + bias; |bias| >= 1 and a b^T ~ N(0, 0.1^2) at every K: no kept element is near
  zero."""
  from mmt_amd import ops
  R = ops.pad_rows(M)
  a = _randn((R, K), 201).to(torch.bfloat16)
  b = _randn((N, K), 202, 0.1 / math.sqrt(K)).to(torch.bfloat16)
  bias = _away_from_zero((N,), 203)
  want = (a[:M].double() @ b.double().t() + bias.double()).numpy()
  assert np.abs(want).min() > 0.25  # (of this file's own construction)
  return a.to(_dev()), b.to(_dev()), bias.to(_dev()), torch.zeros(R, N, device=_dev()), want


def _gemm_dropout_case(run, M, N, K, p, seeded):
  """run(a, b, out, **kw) is the GEMM under test.  res = 0: the output is 0 where the element was dropped and
  (a b^T + bias) / (1 - p) where it was kept."""
  from mmt_amd import ops
  a, b, bias, res, want = _gemm_problem(M, N, K)
  thr, sc = ops.dropout_params(p)
  assert thr == D.thr16_of(p)
  key = D.eff_key(SITE_KEY, SEED if seeded else None)
  for kind in ('none', 'small', 'large'):
    orow, row_index = _row_numbers(kind, a.shape[0])
    out = torch.full_like(res, 7.0)
    run(a, b, out, m=M, bias=bias, res=res, row_index=row_index, drop_key=SITE_KEY, drop_p=p, seed_dev=_seed_dev(seeded))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[M:] == 7.0).all(), 'rows past M were written'
    name = 'row numbers: %s' % kind
    _same_mask(name, got[:M] != 0, D.keep_rows(key, orow[:M], N, thr))  # element index orow * N + col
    kept = got[:M] != 0
    _close_np(name + ', kept values', got[:M][kept], (want * sc)[kept], 1e-3, 1e-4)


@pytest.mark.parametrize('seeded', [False, True])
@pytest.mark.parametrize('p', [0.1, 0.5])
@pytest.mark.parametrize('tile,K', [(t, 64) for t in SCALAR_TILES + TABLE_TILES] + [(24, 128), (25, 128)])
def test_gemm_nt_dropout_mask_is_the_documented_hash(tile, K, p, seeded):
  """BIAS_DROP_RES of every GEMM tile, 300 rows (two full 128-row tiles and a partial one) x 512 columns: the mask is
  keep_flat(eff_key(key, seed), orow * N + col) for every element."""
  from mmt_amd import ops
  _gemm_dropout_case(lambda a, b, out, **kw: ops.gemm_nt(a, b, out, 'BIAS_DROP_RES', tile=tile, **kw), 300, 512, K, p, seeded)


@pytest.mark.parametrize('seeded', [False, True])
@pytest.mark.parametrize('p', [0.1, 0.5])
def test_gemm_nt_splitk_dropout_mask_is_the_documented_hash(p, seeded):
  """The split-K epilogue kernel draws the same function (77 x 256 x 192)."""
  from mmt_amd import ops
  _gemm_dropout_case(lambda a, b, out, **kw: ops.gemm_nt_splitk(a, b, out, 'BIAS_DROP_RES', **kw), 77, 256, 192, p, seeded)


# ---- dropout, LayerNorm sites ----------------------------------------------------------------------------------------

@pytest.mark.parametrize('seeded', [False, True])
@pytest.mark.parametrize('p', [0.1, 0.5])
@pytest.mark.parametrize('d', [256, 1024])
def test_layernorm_sites_dropout_mask_is_the_documented_hash(d, p, seeded):
  """Dropout after the embedding LayerNorm (mmt_embed_ln_fwd), its replay in the backward (drop_mode 2) and the dropout in
  front of a LayerNorm replayed on dy (drop_mode 1): element index orow * d + col.  d = 256 / 1024: one / four 256-column
  chunks per lane; 203 live rows of 256."""
  from mmt_amd import ops
  R, rows = 256, 203
  feats = _randn((R, d), 211).to(_dev())
  g = torch.Generator().manual_seed(212)
  tids = torch.randint(0, 19, (R,), generator=g).int().to(_dev())
  temb = _randn((19, d), 213, 0.05).to(_dev())
  gamma = (1.0 + 0.1 * _randn((d,), 214)).to(_dev())
  beta = (0.1 * _randn((d,), 215)).to(_dev())
  dout = _away_from_zero((R, d), 216).to(_dev())  # |dout| >= 1: one wrong mask element of mode 2 moves dz by O(0.1)
  thr, sc = ops.dropout_params(p)
  key = D.eff_key(SITE_KEY, SEED if seeded else None)
  z, h32, _, mean, rstd = ops.embed_ln_fwd(feats, tids, None, temb, None, gamma, beta, 1e-12, rows=rows)
  dz, _, _, _, _ = ops.ln_bwd(dout, z, mean, rstd, gamma, rows=rows)
  for kind in ('none', 'small', 'large'):
    orow, row_index = _row_numbers(kind, R)
    want = D.keep_rows(key, orow[:rows], d, thr)
    kw = dict(drop_key=SITE_KEY, drop_p=p, row_index=row_index, seed_dev=_seed_dev(seeded))
    name = 'd %d, row numbers: %s' % (d, kind)
    # forward: the mask is where the dropped-out LayerNorm output is non-zero (as test_embedding_layernorm_fwd_bwd recovers it)
    _, hd, _, _, _ = ops.embed_ln_fwd(feats, tids, None, temb, None, gamma, beta, 1e-12, rows=rows, **kw)
    _same_mask('embed_ln_fwd, ' + name, (hd[:rows] != 0).cpu().numpy(), want)
    wmask = torch.from_numpy(want).to(_dev())
    _close_np('embed_ln_fwd kept values, ' + name, hd[:rows].cpu().numpy(), (h32[:rows] * sc * wmask).cpu().numpy(), 1e-5, 1e-5)
    # drop_mode 1: dy = mask * dz / (1 - p) (as test_layernorm_fwd_bwd recovers it)
    dz1, dy1, _, _, _ = ops.ln_bwd(dout, z, mean, rstd, gamma, rows=rows, drop_mode=1, **kw)
    assert torch.equal(dz1, dz)
    _same_mask('ln_bwd mode 1, ' + name, (dy1[:rows].float() != 0).cpu().numpy(), want)
    _close_np('ln_bwd mode 1 kept values, ' + name, dy1[:rows].float().cpu().numpy(), (dz[:rows] * sc * wmask).cpu().numpy(), 2e-2, 1e-2)
    # drop_mode 2: the incoming gradient is masked -- the same as handing the masked gradient to mode 0
    dz2, _, _, _, _ = ops.ln_bwd(dout, z, mean, rstd, gamma, rows=rows, drop_mode=2, want_dy=False, **kw)
    masked = torch.zeros_like(dout)
    masked[:rows] = dout[:rows] * wmask * sc
    dz2_want, _, _, _, _ = ops.ln_bwd(masked, z, mean, rstd, gamma, rows=rows, want_dy=False)
    _close_np('ln_bwd mode 2, ' + name, dz2[:rows].cpu().numpy(), dz2_want[:rows].cpu().numpy(), 1e-5, 1e-5)


# ---- dropout, stand-alone and attention ------------------------------------------------------------------------------

@pytest.mark.parametrize('seeded', [False, True])
@pytest.mark.parametrize('p', [0.1, 0.5])
def test_standalone_dropout_mask_is_the_documented_hash(p, seeded):
  """mmt_dropout_f32 through _MoeDropoutFn (site key _MoeDropoutFn.SITE_KEY, as model.py passes it): element index = the flat
  element number of the 64 x 768 input; and with a saved key (the backward's path) the key is used as it is."""
  import ctypes
  from mmt_amd import _lib, ops
  from mmt_amd.model import _MoeDropoutFn
  thr, sc = ops.dropout_params(p)
  x = _away_from_zero((64, 768), 221).to(_dev())
  idx = np.arange(x.numel(), dtype=np.uint64).reshape(64, 768)
  y = _MoeDropoutFn.apply(x, p, _seed_dev(seeded)).cpu().numpy()
  want = D.keep_flat(D.eff_key(_MoeDropoutFn.SITE_KEY, SEED if seeded else None), idx, thr)
  _same_mask('forward', y != 0, want)
  _close_np('kept values', y, x.cpu().numpy() * np.float32(sc) * want, 1e-6, 1e-6)
  saved = torch.tensor([0x0badc0de], dtype=torch.int32, device=_dev())
  y2 = torch.empty_like(x)
  _lib.check(_lib.lib().mmt_dropout_f32(ops._p(x), ops._p(y2), x.numel(), _MoeDropoutFn.SITE_KEY, thr, ctypes.c_float(sc),
                                        ops._p(_seed_dev(seeded)), None, ops._p(saved), ops._stream()), 'mmt_dropout_f32')
  _same_mask('saved key', y2.cpu().numpy() != 0, D.keep_flat(0x0badc0de, idx, thr))


@pytest.mark.parametrize('seeded', [False, True])
@pytest.mark.parametrize('p', [0.1, 0.5])
@pytest.mark.parametrize('B,H,S', [(3, 2, 50), (2, 4, 37), (1, 12, 30), (2, 4, 218)])
def test_attention_dropout_mask_is_the_documented_hash(B, H, S, p, seeded):
  """mmt_attn_dropout_mask (which the replay tests of test_kernels_gpu.py tie the forward and backward kernels to) against
  attn_mask; every S here has S % 4 != 0, so the row stride S4 of the row key is not S."""
  from mmt_amd import ops
  assert S % 4
  got = ops.attn_dropout_mask(B, H, S, SITE_KEY, p, seed_dev=_seed_dev(seeded)).cpu().numpy()
  _same_mask('attention', got != 0, D.attn_mask(D.eff_key(SITE_KEY, SEED if seeded else None), B, H, S, D.thr16_of(p)))


# ---- GELU / dGELU over every bf16 argument ---------------------------------------------------------------------------
#
# Reference: fp64 on the bf16 argument x.  Forward x Phi(x), Phi(x) = erfc(-x / sqrt 2) / 2; backward Phi(x) + x phi(x).
# Bound (table tiles), from the code and not from any output: |got - ref| <= 1 bf16 ulp of ref + a.  The ulp is half an ulp
# for a correctly rounded result plus half an ulp for the fp32 intermediate that is rounded; a is the fp32 rounding of a
# table entry near 1 (2^-24), which the sign fix 1 - t of a negative argument turns from a relative into an absolute error:
# a = |x| 2^-24 forward (the entry is multiplied by x), a = 2^-24 backward.  Against a shifted table -- which the bound alone
# lets through where neighbouring entries are within an ulp -- at least 99 % of the live arguments must give exactly
# bf16(ref).  A CPU emulation of the kernel arithmetic (fp32 table of gelu_lut.h, fp32 sign fix and product, round to
# nearest even to bf16):                 cases over the bound        bit-equal to bf16(ref)
#                            forward          0 of 65026                   99.59 %
#                            backward         0 of 65026                   99.71 %
#
# Scalar tiles 1 / 2 (gemm.hip: fp32 erff / __expf, no table): the same one-ulp term; the absolute term cannot be derived from
# this project's code (it is the error of the device math library where 1 + erf cancels), so it is twice the largest excess
# over the one-ulp term measured on an MI355X against the fp64 reference, in the units of a above:
#                            forward          measured 0.232 |x| 2^-24   -> SCALAR_FWD_UNITS = 0.464
#                            backward         measured 0.324 2^-24       -> SCALAR_BWD_UNITS = 0.648
# (both tiles give the same figures; an allowance above |x| 2^-20, 16 units, would have been a finding, not a tolerance).  No
# bit-equality floor for these tiles (measured: 99.70 % / 99.72 %).  On the table tiles the MI355X gives the emulation's
# figures to the digit: largest excess 0.484 / 0.970 units, 99.59 % / 99.71 % bit-equal.
TABLE_UNITS = 1.0
SCALAR_FWD_UNITS = 0.464
SCALAR_BWD_UNITS = 0.648
BIT_EQUAL_FLOOR = 0.99


def _patterns():
  """All 65536 bf16 bit patterns with Inf / NaN (exponent 255) and subnormals (exponent 0, mantissa != 0) replaced by zero:
  65026 distinct live patterns (+0 and -0 among them)."""
  pat = np.arange(65536, dtype=np.uint16)
  e, m = (pat >> 7) & 0xff, pat & 0x7f
  pat[(e == 255) | ((e == 0) & (m != 0))] = 0
  return pat


def _bf16_tensor(bits):
  return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).view(torch.bfloat16).to(_dev())


def _bits_of(t):
  return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _f64_of_bits(bits):
  with np.errstate(invalid='ignore'):  # (NaN patterns, where the full pattern range is converted)
    return (bits.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def _ulp_bf16(v):
  """Spacing of the bf16 numbers at |v| (8 significant bits; the subnormal spacing 2^-133 below 2^-126)."""
  _, e = np.frexp(np.abs(v))  # |v| = m 2^e, m in [0.5, 1)
  e = np.where(v == 0, -126, np.maximum(e - 1, -126))
  return np.ldexp(1.0, e - 7)


def _round_to_bf16(v):
  """fp64 -> nearest bf16 (ties to even), as fp64."""
  u = _ulp_bf16(v)
  return np.rint(v / u) * u


@functools.lru_cache(maxsize=None)
def _gelu_ref():
  """(x, x Phi(x), Phi(x) + x phi(x)) in fp64, indexed by the bf16 bit pattern of x (live patterns only)."""
  live = np.unique(_patterns())
  assert live.size == 65026
  x = _f64_of_bits(np.arange(65536, dtype=np.uint16))
  cdf = np.full(65536, np.nan)
  cdf[live] = [0.5 * math.erfc(-v / math.sqrt(2.0)) for v in x[live]]
  pdf = np.full(65536, np.nan)
  pdf[live] = np.exp(-0.5 * x[live] * x[live]) / math.sqrt(2.0 * math.pi)
  return x, x * cdf, cdf + x * pdf


def _check_activation(name, got_bits, arg_bits, backward, units, floor):
  """got = the kernel's bf16 result for the argument with bits arg_bits (same shape).  Prints the figures, then asserts
  |got - ref| <= ulp_bf16(ref) + units * (|x| 2^-24 forward / 2^-24 backward) everywhere and, where a floor is given, that
  at least that share of the live patterns gives bf16(ref) exactly at every one of its copies."""
  x_all, fwd, bwd = _gelu_ref()
  x, ref = x_all[arg_bits], (bwd if backward else fwd)[arg_bits]
  assert not np.isnan(ref).any()
  got = _f64_of_bits(got_bits)
  assert np.isfinite(got).all(), '%s: Inf or NaN in the output' % name
  unit =np.full_like(x, 2.0**-24) if backward else np.abs(x) * 2.0**-24
  excess = np.abs(got - ref) - _ulp_bf16(ref)
  over = excess > units * unit
  pos = unit > 0
  worst = float((excess[pos] / unit[pos]).max())
  exact = got == _round_to_bf16(ref)  # (as values: +0 and -0 are the same result)
  per_pattern = np.ones(65536, dtype=bool)
  np.logical_and.at(per_pattern, arg_bits.reshape(-1), exact.reshape(-1))
  live = np.unique(arg_bits)
  share = float(per_pattern[live].mean())
  print('%s: %d of %d over the bound, largest excess over one ulp %.3f units, bit-equal %.2f %% of %d patterns'
        % (name, int(over.sum()), over.size, worst, 100.0 * share, live.size))
  if over.any():
    i = np.argwhere(over)[:6]
    raise AssertionError('%s: %d of %d results beyond 1 ulp + %g units (largest excess %.3f units); first at %s: x = %s got %s ref %s'
                         % (name, int(over.sum()), over.size, units, worst, i.tolist(), x[over][:6].tolist(), got[over][:6].tolist(),
                            ref[over][:6].tolist()))
  if floor is not None:
    assert share >= floor, '%s: only %.2f %% of the patterns are bit-equal to bf16(ref)' % (name, 100.0 * share)
  return worst, share


def _is_scalar_tile(tile, epi, M, N, K, colsum):
  """Tiles 1 / 2 evaluate erff, every other tile reads the table; tile 0 is whatever the dispatcher picks for the problem."""
  from mmt_amd import _lib
  if tile == 0:
    tile = _lib.lib().mmt_gemm_select_tile(_lib.EPI[epi], M, N, K, 0, 0, int(colsum), 0, 0)
  return tile in (1, 2)


_GELU_CASES = [(t, 64) for t in TABLE_TILES + SCALAR_TILES] + [(24, 128)]


@pytest.mark.parametrize('tile,K', _GELU_CASES)
def test_gelu_epilogue_over_every_bf16_argument(tile, K):
  """BIAS_GELU.  B [1024, K] holds the patterns in its first 64 columns, row m of A [256, K] is one-hot at m % 64 and the
  bias is 0: pre[m, n] = B[n, m % 64] exactly, four copies of every pattern at different tile rows.  Bound: 1 bf16 ulp of
  the fp64 reference + |x| 2^-24 (derivation above); the CPU emulation of the table arithmetic has 0 of 65026 patterns over
  it and 99.59 % bit-equal to bf16(ref), asserted >= 99 %.  Tiles 1 / 2: 1 ulp + 0.464 |x| 2^-24, twice the measured 0.232."""
  from mmt_amd import ops
  M, N = 256, 1024
  pat = _patterns()
  bbits = np.zeros((N, K), dtype=np.uint16)
  bbits[:, :64] = pat.reshape(N, 64)
  a = torch.zeros(M, K)
  a[torch.arange(M), torch.arange(M) % 64] = 1.0
  pre = torch.full((M, N), 7.0, device=_dev(), dtype=torch.bfloat16)
  act = torch.full((M, N), 7.0, device=_dev(), dtype=torch.bfloat16)
  ops.gemm_nt(a.to(torch.bfloat16).to(_dev()), _bf16_tensor(bbits), pre, 'BIAS_GELU', bias=torch.zeros(N, device=_dev()), out2=act,
              tile=tile)
  torch.cuda.synchronize()
  planted = bbits[:, np.arange(M) % 64].T
  stored = _bits_of(pre)
  zero = lambda b: np.where(b == 0x8000, 0, b)  # +0 and -0 count as equal
  assert np.array_equal(zero(stored), zero(planted)), 'the stored pre-activation is not the planted pattern'
  assert np.array_equal(np.unique(zero(stored)), np.unique(zero(pat)))  # every live pattern is there
  scalar = _is_scalar_tile(tile, 'BIAS_GELU', M, N, K, False)
  _check_activation('gelu tile %d K %d' % (tile, K), _bits_of(act), stored, False, SCALAR_FWD_UNITS if scalar else TABLE_UNITS,
                    None if scalar else BIT_EQUAL_FLOOR)


def _dgelu_aux():
  """[256, 1024] patterns: four copies of all 65536, each shifted by 257 elements against the one before, so that a
  pattern meets different rows, columns and positions inside the 4-element groups of the sweep."""
  pat = _patterns()
  return np.concatenate([np.roll(pat, 257 * c).reshape(64, 1024) for c in range(4)], axis=0)


def _check_colsum(name, colsum, out_bits):
  """colsum.sum(0) against the fp64 column sums of the stored output: 255 fp32 additions per column, each rounding a partial
  sum of at most sum |out|: the difference is at most 256 * 2^-24 * sum |out|."""
  out = _f64_of_bits(out_bits)
  got = colsum.double().sum(0).cpu().numpy()
  err = np.abs(got - out.sum(0))
  tol = 256 * 2.0**-24 * np.abs(out).sum(0)
  print('%s: colsum error at most %.3g of its bound' % (name, float((err / tol).max())))
  assert (err <= tol).all(), '%s: colsum off by up to %.3g of the bound' % (name, float((err / tol).max()))


@pytest.mark.parametrize('tile,K,with_colsum', [(t, k, True) for t, k in _GELU_CASES] + [(0, 64, False)])
def test_dgelu_epilogue_over_every_bf16_argument(tile, K, with_colsum):
  """DGELU of gemm_nt.  aux holds the patterns, A[:, 0] = B[:, 0] = 1 and the rest is zero: the accumulator is exactly 1 and
  the output is dGELU(aux) rounded to bf16.  (Tile 0 with colsum is the scalar tile 2 at this size: it also runs without.)
  Bound: 1 bf16 ulp of the fp64 reference + 2^-24 (derivation above); the CPU emulation has 0 of 65026 patterns over it and
  99.71 % bit-equal to bf16(ref), asserted >= 99 %.  Tiles 1 / 2: 1 ulp + 0.648 2^-24, twice the measured 0.324."""
  from mmt_amd import ops
  M, N = 256, 1024
  aux_bits = _dgelu_aux()
  a = torch.zeros(M, K, dtype=torch.bfloat16, device=_dev())
  b = torch.zeros(N, K, dtype=torch.bfloat16, device=_dev())
  a[:, 0] = 1.0
  b[:, 0] = 1.0
  out = torch.full((M, N), 7.0, device=_dev(), dtype=torch.bfloat16)
  colsum = torch.zeros((M + 127) // 128, N, device=_dev()) if with_colsum else None
  ops.gemm_nt(a, b, out, 'DGELU', aux=_bf16_tensor(aux_bits), colsum=colsum, tile=tile)
  torch.cuda.synchronize()
  scalar = _is_scalar_tile(tile, 'DGELU', M, N, K, with_colsum)
  name = 'dgelu tile %d K %d%s' % (tile, K, '' if with_colsum else ' no colsum')
  _check_activation(name, _bits_of(out), aux_bits, True, SCALAR_BWD_UNITS if scalar else TABLE_UNITS, None if scalar else BIT_EQUAL_FLOOR)
  if with_colsum:
    _check_colsum(name, colsum, _bits_of(out))


@pytest.mark.parametrize('tile', [0, 13, 14])
def test_dgelu_epilogue_of_gemm_nn_over_every_bf16_argument(tile):
  """The same sweep through the input-gradient form (w [64, 1024] row-major, a[:, 0] = w[0, :] = 1)."""
  from mmt_amd import ops
  M, N, K = 256, 1024, 64
  aux_bits = _dgelu_aux()
  a = torch.zeros(M, K, dtype=torch.bfloat16, device=_dev())
  w = torch.zeros(K, N, dtype=torch.bfloat16, device=_dev())
  a[:, 0] = 1.0
  w[0, :] = 1.0
  out = torch.full((M, N), 7.0, device=_dev(), dtype=torch.bfloat16)
  ops.gemm_nn(a, w, out, 'DGELU', aux=_bf16_tensor(aux_bits), tile=tile)
  torch.cuda.synchronize()
  _check_activation('dgelu nn tile %d' % tile, _bits_of(out), aux_bits, True, TABLE_UNITS, BIT_EQUAL_FLOOR)
