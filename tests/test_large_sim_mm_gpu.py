"""The row-sharded max-margin kernels (the first half of largesim.hip) through the C ABI against the fp64 restatement of
tests/large_sim_ref.py, at the tile edges of its CASES and on its tie case, in all three forms of the sweeps; then the host
path (mmt_amd.large_sim.RowBlock, ShardedSimLoss) at the smallest shapes it accepts.  The kernels take the raw fp32 numerators
as an input, so the hinge decisions are exactly checkable (tests/test_large_sim_ref_cpu.py proves that no hinge of a case lies
where fp32 and fp64 may differ) and everything else gets a bound derived from the arithmetic; every test prints its worst
error-to-bound ratio."""
import functools

import pytest
import torch

from tests import large_sim_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
U = R.U
MMT_ERR_ARG = -1
S_NAN, G_NAN = 0x7fc00abc, 0x7fc5   # NaN sentinels of the pad columns and pad rows (fp32 / bf16 bit patterns)
PAD_S, PAD_G, PAD_ROWS = 12, 8, 2   # ld = n + 12, ldg = n + 8, two rows below row b
# (form, vw_t given): a = mmt_ls_finish, mmt_ls_counts, mmt_ls_grad | b = finish 1, raw 0 | c = finish 2, raw 1
FORMS = [('a', False), ('b', False), ('b', True), ('c', False), ('c', True)]


def _lib():
  from mmt_amd import _lib, ops
  return _lib.lib(), ops._p, ops._stream(), _lib.check


def _padded(x, pad_cols, pattern, int_dtype):
  """[b, n] -> a device buffer [b + 2, n + pad_cols] of x's dtype whose pad columns and pad rows hold the sentinel."""
  b, n = x.shape
  buf = torch.full((b + PAD_ROWS, n + pad_cols), pattern, dtype=int_dtype, device=DEV).view(x.dtype)
  buf[:b, :n] = x.to(DEV)
  return buf


def _pads_intact(buf, b, n, pattern, int_dtype):
  i = buf.view(int_dtype)
  return bool((i[:b, n:] == pattern).all()) and bool((i[b:] == pattern).all())


def _same_bits(a, b):
  return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _half_ulp_bf16(x):
  """Half the spacing of bf16 (8 significand bits) at |x|: 2^(floor(log2 |x|) - 8), between 2^-9 |x| and 2^-8 |x|."""
  e = torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -126)))
  return torch.where(x == 0, torch.zeros_like(x), torch.exp2(e - 8.0))


def _g_bound(G, M):
  """|G16 - G'|: half a bf16 ulp of G' plus the fp32 error of the quotient ((M + 5) u: den, reciprocal, multiply, and the
  rounding of g).  The half ulp is taken at G' itself: 2^-9 |G'| is its value at the top of a binade only (bf16 keeps 8
  significand bits, so a correctly rounded value is off by up to 2^-8 relative at the bottom)."""
  return _half_ulp_bf16(G) + (M + 5) * U * G.abs()


@functools.lru_cache(maxsize=None)
def _run(name, form, vwt):
  """One pass of a form over a case: counts (twice, on fresh buffers), then the gradient.  Everything comes back on the CPU."""
  L, p, st, check = _lib()
  x = R.reference(name)
  b, n, r0, M, margin = x['b'], x['n'], x['r0'], x['M'], x['margin']
  ld, ldg, ncb = n + PAD_S, n + PAD_G, R.ncb(n)
  assert L.mmt_ls_col_blocks(n) == ncb
  tw, vw, diag = x['tw'].to(DEV), x['vw'].to(DEV), x['diag'].to(DEV)
  vw_t = vw.t().contiguous() if vwt else None
  out = dict(pads=True)

  def counts():
    S = _padded(x['raw'], PAD_S, S_NAN, torch.int32)
    rowcnt = torch.zeros(b, device=DEV, dtype=torch.int32)
    colcnt = torch.zeros(n, device=DEV, dtype=torch.int32)
    part = torch.full((b, ncb), float('nan'), device=DEV)
    if form == 'a':
      check(L.mmt_ls_finish(p(S), ld, p(tw), p(vw), b, n, M, st), 'mmt_ls_finish')
      out['pads'] &= _pads_intact(S, b, n, S_NAN, torch.int32)
      out['S_finished'] = S[:b, :n].cpu()
      check(L.mmt_ls_counts(p(S), ld, p(diag), b, n, r0, margin, p(rowcnt), p(colcnt), p(part), st), 'mmt_ls_counts')
    else:
      check(L.mmt_ls_counts_ex(p(S), ld, p(diag), p(tw), p(vw), p(vw_t), M, 1 if form == 'b' else 2, b, n, r0, margin, p(rowcnt),
                               p(colcnt), p(part), st), 'mmt_ls_counts_ex')
    out['pads'] &= _pads_intact(S, b, n, S_NAN, torch.int32)
    return S, rowcnt.cpu(), colcnt.cpu(), part.cpu()

  S, out['rowcnt'], out['colcnt'], out['part'] = counts()
  out['S_counts'] = S[:b, :n].cpu()
  out['again'] = counts()[1:]
  rowcnt = x['rowcnt'].to(device=DEV, dtype=torch.int32)
  total = x['colcnt_total'].to(device=DEV, dtype=torch.int32)
  G16 = _padded(torch.full((b, n), float('nan'), dtype=torch.bfloat16), PAD_G, G_NAN, torch.int16)
  gs = torch.full((b, ncb, M), float('nan'), device=DEV)
  if form == 'a':
    check(L.mmt_ls_grad(p(S), ld, p(diag), p(tw), p(vw), p(rowcnt), p(total), b, n, M, r0, margin, x['inv_norm'], p(G16), ldg, p(gs),
                        st), 'mmt_ls_grad')
  else:
    check(L.mmt_ls_grad_ex(p(S), ld, p(diag), p(tw), p(vw), p(vw_t), p(rowcnt), p(total), b, n, M, r0, margin, x['inv_norm'], p(G16),
                           ldg, p(gs), 1 if form == 'c' else 0, st), 'mmt_ls_grad_ex')
  torch.cuda.synchronize()
  out['pads'] &= _pads_intact(S, b, n, S_NAN, torch.int32) and _pads_intact(G16, b, n, G_NAN, torch.int16)
  out['S_grad'] = S[:b, :n].cpu()
  out['G16'], out['gs'] = G16[:b, :n].cpu(), gs.cpu()
  return out


@pytest.mark.parametrize('name', R.NAMES)
def test_finish_and_diag_match_fp64(name):
  """mmt_ls_finish: |S - s| <= (M + 4) u |s| + 1e-37 element by element (den an fma chain of M non-negative terms, a reciprocal
  within 1 ulp, one multiply; the den == 0 elements included).  mmt_ls_diag on the RAW block: bit-equal to the diagonal of the
  finished block (the promise at ls_quot) and within the same bound; r0 + b > n and r0 < 0 are refused."""
  L, p, st, check = _lib()
  x = R.reference(name)
  b, n, r0, M = x['b'], x['n'], x['r0'], x['M']
  got = _run(name, 'a', False)['S_finished'].double()
  tol = (M + 4) * U * x['s'].abs() + 1e-37
  err = (got - x['s']).abs()
  assert bool(x['zero'].any()) and torch.isfinite(got).all()
  t = torch.arange(b)
  S = _padded(x['raw'], PAD_S, S_NAN, torch.int32)
  tw, vw = x['tw'].to(DEV), x['vw'].to(DEV)
  dl = torch.full((b + 1,), float('nan'), device=DEV)
  check(L.mmt_ls_diag(p(S), n + PAD_S, p(tw), p(vw), b, n, M, r0, p(dl), st), 'mmt_ls_diag')
  dl = dl.cpu()
  print('finish %s: worst |S - s| / bound %.3f; diag %.3f' % (name, (err / tol).max().item(),
                                                            ((dl[:b].double() - x['s'][t, r0 + t]).abs() / tol[t, r0 + t]).max().item()))
  assert bool((err <= tol).all())
  assert _same_bits(dl[:b], got.float()[t, r0 + t]) and bool(torch.isnan(dl[b]))
  assert bool(((dl[:b].double() - x['s'][t, r0 + t]).abs() <= tol[t, r0 + t]).all())
  assert _same_bits(S[:b, :n].cpu(), x['raw']) and _pads_intact(S, b, n, S_NAN, torch.int32)
  assert L.mmt_ls_diag(p(S), n + PAD_S, p(tw), p(vw), b, n, M, n - b + 1, p(dl), st) == MMT_ERR_ARG
  assert L.mmt_ls_diag(p(S), n + PAD_S, p(tw), p(vw), b, n, M, -1, p(dl), st) == MMT_ERR_ARG


@pytest.mark.parametrize('form,vwt', FORMS)
@pytest.mark.parametrize('name', R.NAMES)
def test_counts_are_exact_and_loss_partials_within_bound(name, form, vwt):
  """rowcnt and colcnt equal the fp64 reference's exactly (no hinge of a case is in band; on the tie case every operation is
  exact).  loss_part[t, cb] within the active hinges' bands + 72 u sum |h| (64 thread-local additions, 6 butterfly steps, 2
  adds across the waves); bit-equal to the exact sums on the tie case; identical on a second run.  S: unchanged by finish 0 and
  2, the mmt_ls_finish result after finish 1; the pad columns and rows bitwise untouched."""
  x, o = R.reference(name), _run(name, form, vwt)
  if name != 'tie':
    assert x['in_band'] == 0
  assert o['pads']
  assert torch.equal(o['rowcnt'].long(), x['rowcnt']), (o['rowcnt'].long() - x['rowcnt']).abs().max().item()
  assert torch.equal(o['colcnt'].long(), x['colcnt']), (o['colcnt'].long() - x['colcnt']).abs().max().item()
  err = (o['part'].double() - x['loss_part']).abs()
  print('counts %s %s vwt=%d: worst |loss_part - ref| / bound %.3f' % (name, form, vwt, (err / x['loss_tol'].clamp_min(1e-300)).max().item()))
  assert torch.isfinite(o['part']).all() and bool((err <= x['loss_tol']).all())
  if name == 'tie':
    assert torch.equal(o['part'].double(), x['loss_part'])
  finished = _run(name, 'a', False)['S_finished']
  assert _same_bits(o['S_counts'], x['raw'] if form == 'c' else finished)
  assert _same_bits(o['S_grad'], o['S_counts'])
  again = o['again']
  assert torch.equal(again[0], o['rowcnt']) and torch.equal(again[1], o['colcnt']) and _same_bits(again[2], o['part'])


@pytest.mark.parametrize('form,vwt', FORMS)
@pytest.mark.parametrize('name', R.NAMES)
def test_gradient_operand_and_gs_partials_within_bound(name, form, vwt):
  """G16 off the diagonal: bits exactly +0 where both hinges are inactive, elsewhere within half a bf16 ulp + (M + 5) u |G'| of
  G' = g / den (see _g_bound: the half ulp is 2^-9 |G'| at the top of a binade and 2^-8 |G'| at its bottom); the diagonal
  against -(rowcnt + colcnt_total) inv_norm / den with colcnt_total = own counts + a random vector (a kernel that ignored the
  argument, or indexed it without r0, shows), negative where the counts are positive.  gs_part against the fp64 sum over the
  kernel's OWN G16: (44 + M + 4) u sum |G16 s vw| (32 elements per thread, 8 reduction adds, the products; the fp32 similarity).
  Tie case: G16 bit-equal to bf16(fp32(g)) wherever den == 1 (where den == 0 the quotient g / 1e-5 is not exact: the bound)."""
  x, o = R.reference(name), _run(name, form, vwt)
  b, n, r0, M = x['b'], x['n'], x['r0'], x['M']
  assert o['pads']
  G, got = x['G'], o['G16'].double()
  t = torch.arange(b)
  idle = ~(x['h1'] > 0) & ~(x['h2'] > 0) & x['off']
  assert int(idle.sum()) > 0 and bool((o['G16'].view(torch.int16)[idle] == 0).all())
  assert bool((G[idle] == 0).all()) and bool((G[~idle & x['off']] > 0).all())
  tol = _g_bound(G, M)
  err = (got - G).abs()
  print('grad %s %s vwt=%d: worst |G16 - G\'| / bound %.3f (diagonal %.3f)' % (
      name, form, vwt, (err / tol.clamp_min(1e-300))[~idle].max().item(), (err / tol)[t, r0 + t].max().item()))
  assert torch.isfinite(got).all() and bool((err <= tol).all())
  cnt = x['rowcnt'] + x['colcnt_total'][r0:r0 + b]
  assert bool((cnt > 0).all()) and bool((got[t, r0 + t] < 0).all())
  if name == 'tie':
    g32 = (G * x['den']).float()                     # k * inv_norm, |k| < 2^24: one rounding, as the kernel's single multiply
    one = x['den'] == 1.0
    assert torch.equal(o['G16'].view(torch.int16)[one], g32.to(torch.bfloat16).view(torch.int16)[one])
  want = R.gs_from(o['G16'], x['s'], x['vw'], x['zero'])
  gtol = R.gs_tol(o['G16'], x['s'], x['vw'], x['zero'], M)
  gerr = (o['gs'].double() - want).abs()
  print('grad %s %s vwt=%d: worst |gs - ref| / bound %.3f' % (name, form, vwt, (gerr / gtol.clamp_min(1e-300)).max().item()))
  assert torch.isfinite(o['gs']).all() and bool((gerr <= gtol).all())
  assert bool((o['gs'][x['zero'].all(1)] == 0).all())   # the zero-weight text: nothing flows into its mixture weights


@pytest.mark.parametrize('name', R.NAMES)
def test_forms_agree_bit_for_bit(name):
  ref = _run(name, 'a', False)
  for form, vwt in FORMS[1:]:
    o = _run(name, form, vwt)
    assert torch.equal(o['rowcnt'], ref['rowcnt']) and torch.equal(o['colcnt'], ref['colcnt']), (form, vwt)
    assert torch.equal(o['G16'].view(torch.int16), ref['G16'].view(torch.int16)), (form, vwt)


@pytest.mark.parametrize('R_,Rpad,M,d', [(1, 1, 1, 4), (43, 128, 7, 260), (5, 5, 16, 1024)])
def test_fold_bf16_is_the_rounded_product(R_, Rpad, M, d):
  L, p, st, check = _lib()
  g = torch.Generator().manual_seed(9)
  x = torch.randn(R_, M, d, generator=g)
  w = torch.softmax(torch.randn(R_, M, generator=g), -1)
  w[R_ // 2, 0] = 0.0
  out = torch.full((Rpad + 1, M * d), G_NAN, dtype=torch.int16, device=DEV).view(torch.bfloat16)
  xd, wd = x.to(DEV), w.to(DEV)
  check(L.mmt_ls_fold_bf16(p(xd), p(wd), R_, Rpad, M, d, p(out), st), 'mmt_ls_fold_bf16')
  got = out.cpu().view(torch.int16)
  assert torch.equal(got[:R_], R.fold(x, w).view(torch.int16))
  assert bool((got[R_:Rpad] == 0).all()) and bool((got[Rpad] == G_NAN).all())
  assert L.mmt_ls_fold_bf16(p(xd), p(wd), R_, Rpad, M, 6, p(out), st) == MMT_ERR_ARG


@pytest.mark.parametrize('pad', [0, 8])
@pytest.mark.parametrize('d', [4, 260, 1024])
def test_unfold_is_the_weighted_copy_and_the_dot(d, pad):
  """dx bit-equal to fp32(P w); dw within (d / 64 + 8) u sum |P x| + u |gsub| of fp64 (a lane adds at most d / 64 products, then
  6 butterfly steps and the subtraction); gsub = None subtracts nothing; with dx or dw None the other is unchanged, bit for bit."""
  L, p, st, check = _lib()
  R_, M = 5, 3
  ldp = M * d + pad
  g = torch.Generator().manual_seed(13)
  P = torch.randn(R_, ldp, generator=g)
  x = torch.randn(R_, M, d, generator=g)
  w = torch.softmax(torch.randn(R_, M, generator=g), -1)
  gsub = torch.randn(R_, M, generator=g)
  Pd, xd, wd, gd = P.to(DEV), x.to(DEV), w.to(DEV), gsub.to(DEV)

  def run(sub, want_dx, want_dw):
    dx = torch.full((R_ + 1, M, d), float('nan'), device=DEV)
    dw = torch.full((R_ + 1, M), float('nan'), device=DEV)
    check(L.mmt_ls_unfold(p(Pd), ldp, p(xd), p(wd), p(gd) if sub else None, R_, M, d, p(dx) if want_dx else None,
                          p(dw) if want_dw else None, st), 'mmt_ls_unfold')
    return dx.cpu(), dw.cpu()
  dx, dw = run(True, True, True)
  Pv = P[:, :M * d].reshape(R_, M, d)
  assert _same_bits(dx[:R_], Pv * w[..., None]) and bool(torch.isnan(dx[R_]).all()) and bool(torch.isnan(dw[R_]).all())
  dot = (Pv.double() * x.double()).sum(-1)
  tol = (d / 64.0 + 8.0) * U * (Pv.double() * x.double()).abs().sum(-1)
  err = (dw[:R_].double() - (dot - gsub.double())).abs()
  print('unfold d=%d ldp=%d: worst |dw - ref| / bound %.3f' % (d, ldp, (err / (tol + U * gsub.abs().double())).max().item()))
  assert bool((err <= tol + U * gsub.abs().double()).all())
  _, dw0 = run(False, True, True)
  assert bool(((dw0[:R_].double() - dot).abs() <= tol).all())
  dx1, dw1 = run(True, False, True)
  assert bool(torch.isnan(dx1).all()) and _same_bits(dw1[:R_], dw[:R_]) and bool(torch.isnan(dw1[R_]).all())
  dx2, dw2 = run(True, True, False)
  assert bool(torch.isnan(dw2).all()) and _same_bits(dx2[:R_], dx[:R_]) and bool(torch.isnan(dx2[R_]).all())


# ---- the host path: RowBlock and ShardedSimLoss at the smallest shapes they accept ---------------------------------------------

@functools.lru_cache(maxsize=None)
def _host(i):
  """RowBlock on host shape i: the phases up to the counts, then mmt_ls_grad_ex called directly (colcnt_total = the block's
  counts + the other ranks' stand-in) and _backward_tail / phase_video_grad on its outputs.  Everything on the CPU."""
  from mmt_amd.large_sim import RowBlock
  L, p, st, check = _lib()
  h = R.host_reference(i)
  b, n, r0, m = h['b'], h['n'], h['r0'], h['M']
  blk = RowBlock(h['txt_blk'].to(DEV), h['tw_blk'].to(DEV), h['vid'].to(DEV), h['vw'].to(DEV), r0, h['margin'])
  diag_local = blk.phase_similarity().cpu()
  raw = blk.S[:b].cpu().clone()
  diag = h['diag'].clone()
  diag[r0:r0 + b] = diag_local                         # (the all-gather: the other ranks' entries come from the reference)
  colcnt, loss = blk.phase_counts(diag.to(DEV))
  out = dict(t16=blk.t16.cpu(), v16=blk.v16.cpu(), raw=raw, raw_after=blk.S[:b].cpu(), diag_local=diag_local, diag=diag,
             rowcnt=blk.rowcnt.cpu().long(), colcnt=colcnt.cpu().long(), loss=loss.item(), norm=blk.norm)
  others = torch.randint(0, 51, (n,), generator=torch.Generator().manual_seed(29))
  total = out['colcnt'] + others
  total_dev = total.to(device=DEV, dtype=torch.int32)
  bp = blk.t16.shape[0]
  g16 = torch.empty(bp, n, device=DEV, dtype=torch.bfloat16)
  g16[b:].zero_()
  gs_part = torch.full((b, L.mmt_ls_col_blocks(n), m), float('nan'), device=DEV)
  check(L.mmt_ls_grad_ex(p(blk.S), blk.ld, p(blk.diag_all), p(blk.tw), p(blk.vw_all), p(blk.vw_t), p(blk.rowcnt),
                         p(total_dev), b, n, m, r0, blk.margin, 1.0 / blk.norm, p(g16), n, p(gs_part), 1, st),
        'mmt_ls_grad_ex')
  dtxt, dtw, q = blk._backward_tail(g16, gs_part)
  sl = slice(r0, r0 + b)
  dvid = blk.phase_video_grad(q[sl], h['vid'][sl].to(DEV), h['vw'][sl].to(DEV))
  out.update(total=total, g16=g16.cpu(), gs_part=gs_part.cpu(), dtxt=dtxt.cpu(), dtw=dtw.cpu(), q=q.cpu(), dvid=dvid.cpu())
  return out


@pytest.mark.parametrize('i', range(len(R.HOST_SHAPES)))
def test_host_operands_similarity_counts_and_loss(i):
  """In order: t16 / v16 bit-equal to the torch restatement of the fold; the raw S within K 2^-23 sum |t v| (K = M d: two
  roundings per accumulation in any order) of the fp64 product of those operands; diag_local, rowcnt, colcnt and the loss
  against the reference evaluated on the block's OWN raw S read back -- a count may differ by the in-band elements of its row
  or column, which must be at most 0.1 % of the block."""
  h, o = R.host_reference(i), _host(i)
  b, n, r0, M = h['b'], h['n'], h['r0'], h['M']
  assert torch.equal(o['t16'][:b].view(torch.int16), h['t16'].view(torch.int16)) and bool((o['t16'][b:].view(torch.int16) == 0).all())
  assert torch.equal(o['v16'].view(torch.int16), h['v16'].view(torch.int16))
  err = (o['raw'].double() - h['raw']).abs()
  print('host %d: worst |raw S - fp64| / bound %.3f' % (i, (err / h['raw_bound'].clamp_min(1e-300)).max().item()))
  assert bool((err <= h['raw_bound']).all())
  assert _same_bits(o['raw_after'], o['raw'])          # (keep_similarity=False: the block keeps the numerators)
  x = R.host_block(i, o['raw'], o['diag'])
  den, zero = R.den_of(x['tw'], x['vw'])
  s = o['raw'].double() / den
  t = torch.arange(b)
  dtol = (M + 4) * U * s[t, r0 + t].abs() + 1e-37
  assert bool(((o['diag_local'].double() - s[t, r0 + t]).abs() <= dtol).all())
  b1, b2, h1, h2, off = R.bands(x, s)
  in1, in2 = (h1.abs() <= b1) & off, (h2.abs() <= b2) & off
  assert int((in1 | in2).sum()) <= 1e-3 * b * n
  rowcnt, colcnt, part = R.counts(s, o['diag'], r0, x['margin'])
  assert bool(((o['rowcnt'] - rowcnt).abs() <= in1.sum(1)).all()) and bool(((o['colcnt'] - colcnt).abs() <= in2.sum(0)).all())
  assert int(rowcnt.sum()) > 0 and int(colcnt.sum()) > 0
  # the loss: the partials' bound, an in-band hinge counted or not (|h| <= band), b + 2 roundings of the host's sums and division
  z = torch.zeros_like(h1)
  tol = (R.loss_part_tol(x, s).sum() + torch.where(in1, b1, z).sum() + torch.where(in2, b2, z).sum() + (b + 2) * U * part.sum()) / o['norm']
  want = part.sum() / o['norm']
  print('host %d: in band %d, |loss - ref| / bound %.3f' % (i, int((in1 | in2).sum()), abs(o['loss'] - want.item()) / tol.item()))
  assert abs(o['loss'] - want.item()) <= tol.item()


@pytest.mark.parametrize('i', range(len(R.HOST_SHAPES)))
def test_host_backward_tail_matches_fp64_products(i):
  """G16 from mmt_ls_grad_ex on the block, then _backward_tail and phase_video_grad.  P = G' V' and Q = G'^T T' are judged through
  their outputs against fp64 products of the read-back bf16 operands with the accumulation bound K 2^-23 sum |a b| (K = n for
  P, bp for Q); dtxt = tw P, dtw = <T, P> - gs and dvid = vw Q follow with the unfold bounds.  A reference that loses one column
  of G16 is outside the dtxt bound."""
  h, o = R.host_reference(i), _host(i)
  b, n, r0, M, d = h['b'], h['n'], h['r0'], h['M'], h['d']
  bp = o['t16'].shape[0]
  x = R.host_block(i, o['raw'], o['diag'])
  den, zero = R.den_of(x['tw'], x['vw'])
  s = o['raw'].double() / den
  b1, b2, h1, h2, off = R.bands(x, s)
  settled = ~(((h1.abs() <= b1) | (h2.abs() <= b2)) & off)
  G = R.grad(s, den, o['diag'], r0, x['margin'], o['rowcnt'], o['total'], 1.0 / o['norm'])
  g16 = o['g16'][:b]
  assert bool((o['g16'][b:].view(torch.int16) == 0).all())
  gerr, gtol = (g16.double() - G).abs(), _g_bound(G, M) + 2.0 * U * G.abs()   # (+ inv_norm passed as a rounded fp32)
  print('host %d: worst |G16 - G\'| / bound %.3f' % (i, (gerr / gtol.clamp_min(1e-300))[settled & (G != 0)].max().item()))
  assert bool((gerr <= gtol)[settled].all())
  ga, v16, t16 = g16.double(), o['v16'].double(), o['t16'].double()
  tw, txt = x['tw'].double(), h['txt_blk'].double()
  # P and dtxt
  P = (ga @ v16).view(b, M, d)
  Pb = (n * 2.0 * U * (ga.abs() @ v16.abs())).view(b, M, d)
  want = tw[..., None] * P
  tol = tw[..., None] * Pb * (1 + U) + U * want.abs()
  err = (o['dtxt'].double() - want).abs()
  print('host %d: worst |dtxt - ref| / bound %.3f' % (i, (err / tol.clamp_min(1e-300)).max().item()))
  assert bool((err <= tol).all())
  c = 7                                                # one lost column of G16 (a video with weights) moves dtxt out of the bound
  lost = ga.clone()
  lost[:, c] = 0.0
  moved = (tw[..., None] * (lost @ v16).view(b, M, d) - want).abs()
  assert bool((moved > 2.0 * tol).any()) and float((moved > 2.0 * tol).double().mean()) > 0.25
  # dtw = <T, P> - gs
  gs = R.gs_from(g16, s, x['vw'], zero).sum(1)
  gs_tol = R.gs_tol(g16, s, x['vw'], zero, M).sum(1)
  gerr = (o['gs_part'].double().sum(1) - gs).abs()
  assert bool((gerr <= gs_tol).all())
  want = (txt * P).sum(-1) - gs
  tol = ((txt.abs() * Pb).sum(-1) + (d / 64.0 + 8.0) * U * (txt * P).abs().sum(-1)) * (1 + 64 * U) + U * gs.abs() + gs_tol
  err = (o['dtw'].double() - want).abs()
  print('host %d: worst |dtw - ref| / bound %.3f, |gs - ref| / bound %.3f' % (i, (err / tol.clamp_min(1e-300)).max().item(),
                                                                             (gerr / gs_tol.clamp_min(1e-300)).max().item()))
  assert bool((err <= tol).all())
  # Q (K = the zero-padded local rows) and dvid of the block's own videos
  Q = ga.t() @ t16[:b]
  Qb = bp * 2.0 * U * (ga.abs().t() @ t16[:b].abs())
  err = (o['q'].double() - Q).abs()
  print('host %d: worst |Q - ref| / bound %.3f' % (i, (err / Qb.clamp_min(1e-300)).max().item()))
  assert bool((err <= Qb).all())
  sl = slice(r0, r0 + b)
  vw = h['vw'][sl]
  assert _same_bits(o['dvid'], o['q'][sl].view(b, M, d) * vw[..., None])
  want = vw.double()[..., None] * Q[sl].view(b, M, d)
  tol = vw.double()[..., None] * Qb[sl].view(b, M, d) * (1 + U) + U * want.abs()
  assert bool(((o['dvid'].double() - want).abs() <= tol).all())


@pytest.mark.parametrize('margin', [0.05, -0.01])
def test_sharded_sim_loss_without_fixed_norm(margin):
  """ShardedSimLoss(margin, fix_norm=False) without a process group (one row block, n = 256) against
  oracle.max_margin_ranking_loss on the fp64 similarity, 2e-3 relative as test_row_sharded_similarity_and_maxmargin; and the
  constant 2 n max(margin, 0) / norm on its own: without it the loss is the fix_norm=True loss times (n - 1) / n."""
  from mmt_amd.large_sim import ShardedSimLoss
  from oracle import mmt_oracle as O
  x = R.host_inputs(0)
  n = x['n']
  vid, txt, tw, vw = x['vid'], x['txt'], x['tw'], x['vw']
  sims = O.cross_view_inner_product(vid.double(), txt.double()[:, :, None, :], vw.double(), tw.double()[:, None, :], 'avg')
  want = O.max_margin_ranking_loss(sims, margin, False).item()
  run = lambda fix: ShardedSimLoss(margin, fix)(vid.to(DEV), txt.to(DEV)[:, :, None, :], vw.to(DEV), tw.to(DEV)[:, None, :]).item()
  free, fixed = run(False), run(True)
  print('ShardedSimLoss margin %g: fix_norm=False %.8f (oracle %.8f), fix_norm=True %.8f' % (margin, free, want, fixed))
  assert want > 0 and abs(free - want) <= 2e-3 * abs(want) + 1e-6
  const = 2.0 * n * max(margin, 0.0) / (2.0 * n * n)
  assert abs((free - const) - fixed * (n - 1) / n) <= 1e-6 * abs(fixed)
