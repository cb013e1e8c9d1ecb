"""The kernels and epilogue paths that only the encoder engine (bert_engine.hip) launches, each on its own against the fp64
references of tests/engine_paths_ref.py: the split-K slab producer, the two LayerNorm kernels that sum the slabs themselves,
the row-dot epilogue of the dO GEMM and the attention backward that consumes it, the rows-only attention of the last layer,
and the two small tail-layer kernels.

Bounds.  "n 2^-24 sum |terms|" is the first-order bound of an fp32 sum of n terms in any order (nothing measured); every
other tolerance is the one tests/test_kernels_gpu.py already uses for the same quantity (test_layernorm_fwd_bwd,
test_attention_fwd_bwd_dense, test_gemm_nt_wide_tiles).  Dropout masks are compared bit for bit with tests/dropout_ref.py.
Buffers are allocated larger than what a call may touch and pre-filled: outputs with a sentinel that must survive, inputs
with NaN where no live row may read them.
"""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

from tests import dropout_ref as D
from tests import engine_paths_ref as R
from tests import test_epilogue_exact_gpu as E

pytestmark = pytest.mark.gpu

U32 = R.U32
NAN = float('nan')
EPS = 1e-12
ROW_KINDS = ('none', 'small', 'large')
_close_np, _same_mask = E._close_np, E._same_mask


def _dev():
  return torch.device('cuda:0')


def _randn(shape, seed, scale=1.0):
  return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _i32(x):
  return torch.as_tensor(np.asarray(x), dtype=torch.int32).to(_dev())


def _within(name, got, want, bound):
  """|got - want| <= bound elementwise (fp64 numpy); prints the largest share of the bound that is used."""
  got, want, bound = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64), np.asarray(bound, dtype=np.float64)
  assert np.isfinite(got).all(), '%s: Inf or NaN in the output' % name
  err = np.abs(got - want)
  pos = bound > 0
  used = float((err[pos] / bound[pos]).max()) if pos.any() else 0.0
  print('%s: largest error %.3g, %.3g of its bound' % (name, float(err.max()) if err.size else 0.0, used))
  bad = err > bound
  assert not bad.any(), '%s: %d of %d beyond the bound (up to %.3g of it); first at %s' % (
      name, int(bad.sum()), bad.size, used, np.argwhere(bad)[:6].tolist())


def _keep_rate(name, keep, p):
  assert abs(float(np.mean(keep)) - (1.0 - p)) <= 0.03, '%s: keep rate %.4f of the reference' % (name, float(np.mean(keep)))


def _raises_arg_error(fn):
  with pytest.raises(RuntimeError, match=r'failed with code -1$'):
    fn()


# ---- A. the slab producer -------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _slab_operands(M, N, K):
  from mmt_amd import ops
  a = _randn((ops.pad_rows(M), K), 301).to(torch.bfloat16)
  b = _randn((N, K), 302, 0.05).to(torch.bfloat16)
  return a, b, a.to(_dev()), b.to(_dev())


def _run_slabs(M, N, K, req, n_rows_dev=None):
  from mmt_amd import ops
  a, b, a_d, b_d = _slab_operands(M, N, K)
  splits, stride = ops.splitk_geometry(M, N, K, req)
  want_splits, per, want_stride = R.splitk_geometry(M, N, K, req)
  assert (splits, stride) == (want_splits, want_stride) and stride == (M + 127) // 128 * 128 * N
  ws = torch.full((16 * stride,), NAN, device=_dev())
  ops.gemm_nt_splitk(a_d, b_d, None, 'F32', m=M, splits=req, no_epilogue=True, ws=ws, n_rows_dev=n_rows_dev)
  torch.cuda.synchronize()
  return a, b, splits, per, ws.cpu().numpy().astype(np.float64).reshape(16, stride // N, N)


@pytest.mark.parametrize('M,N,K,req', [(56, 256, 512, 0), (200, 512, 3072, 0), (200, 256, 1536, 4), (56, 256, 448, 4),
                                       (56, 256, 320, 4)])
def test_splitk_slabs_are_the_chunk_products(M, N, K, req):
  """gemm_nt_splitk(no_epilogue=True), wide = 0, as the engine calls it.  K = 448: the last chunk is one K-step short;
  K = 320: three slabs although four were asked for.  Slab s alone against the fp64 product over its chunk of kl columns,
  bound kl 2^-24 sum |a_k| |b_k|.  The workspace starts as NaN: the code GUARANTEES that rows >= M of every slab and the
  slabs >= splits are never written (the tile epilogue stores rows < M only, the grid has `splits` K-slices), so they must
  still be NaN -- the consumers (mmt_splitk_ln_fwd, mmt_ln_bwd_slabs) never read them either, which their own tests show."""
  a, b, splits, per, ws = _run_slabs(M, N, K, req)
  prod, mag, kl = R.slab_products(a, b, M, per, splits)
  assert kl.sum() == K
  for s in range(splits):
    _within('slab %d of %d (kl %d)' % (s, splits, kl[s]), ws[s, :M], prod[s], kl[s] * U32 * mag[s])
  assert np.isnan(ws[:splits, M:]).all(), 'rows >= M of a slab were written'
  assert np.isnan(ws[splits:]).all(), 'a slab >= splits was written'


def test_splitk_slabs_on_a_packed_batch():
  """n_rows_dev = 70 at M = 200: the row tile at 128 is past the live rows and exits -- rows >= 128 stay untouched; rows < 70
  are the chunk products."""
  M, N, K, req, live = 200, 256, 1536, 4, 70
  a, b, splits, per, ws = _run_slabs(M, N, K, req, n_rows_dev=_i32([live]))
  prod, mag, kl = R.slab_products(a, b, M, per, splits)
  for s in range(splits):
    _within('slab %d' % s, ws[s, :live], prod[s, :live], kl[s] * U32 * mag[s, :live])
  assert np.isnan(ws[:, 128:]).all() and np.isnan(ws[splits:]).all()


# ---- B. mmt_splitk_ln_fwd(_ex) --------------------------------------------------------------------------------------------

LN_FWD_SHAPES = [(256, 1, 1), (512, 2, 56), (768, 4, 203), (1024, 16, 203), (256, 8, 56)]  # (d, splits, rows)
RES_ROWS = 320  # rows of the larger residual buffer of the tail's attention-out site


def _ln_fwd_problem(d, splits, rows, cap, seed):
  """Synthetic slabs at the geometry's stride for `cap` launched rows of which `rows` are live: sum_s slab_s + bias =
  +-(1.01 + |N(0, 1)|) 1.01 (never within 1 of zero), slab 0 solved for in fp64; residual in [0, 4] (its mean of 2 keeps the
  row mean of z away from zero: the 1e-5 relative bound on `mean` is then a bound on rounding, not on cancellation).  16
  slabs are allocated; the unused ones and the rows past the live ones are NaN."""
  stride = (cap + 127) // 128 * 128 * d
  target = E._away_from_zero((rows, d), seed).double() * 1.01
  bias = _randn((d,), seed + 1)
  slabs = torch.full((16, stride // d, d), NAN)
  slabs[1:splits, :rows] = _randn((max(splits - 1, 0), rows, d), seed + 2)
  slabs[0, :rows] = (target - bias.double() - slabs[1:splits, :rows].double().sum(0)).float()
  res = torch.rand(rows, d, generator=torch.Generator().manual_seed(seed + 3)) * 4.0
  gamma, beta = 1.0 + 0.1 * _randn((d,), seed + 4), 0.1 * _randn((d,), seed + 5)
  return dict(d=d, splits=splits, rows=rows, cap=cap, stride=stride, slabs=slabs, bias=bias, res=res, gamma=gamma, beta=beta)


def _ln_fwd_run_and_check(name, P, pointers, orow_of_kind, res_buf, res_rows_np):
  """One pointer configuration over dropout off and p in {0.1, 0.5} x seeded / unseeded x row numbers none / small / large.
  pointers(kind) -> keyword arguments of ops.splitk_ln_fwd for that kind of row numbers (res / res_rows / rowidx / row_index
  / rowidx_out / n_rows_dev / want_h16); orow_of_kind(kind) -> the RNG row of every live row; res_buf: the residual buffer
  handed to the kernel (NaN outside the rows it may read), res_rows_np: the rows of it the live rows read."""
  from mmt_amd import ops
  d, splits, rows, cap = P['d'], P['splits'], P['rows'], P['cap']
  dev = _dev()
  slabs_d, bias_d, gamma_d, beta_d = (P[k].to(dev) for k in ('slabs', 'bias', 'gamma', 'beta'))
  res_d = res_buf.to(dev)
  slabs64, bias64, res64 = R.f64(P['slabs'][:splits, :rows]), R.f64(P['bias']), R.f64(P['res'])
  gamma64, beta64 = R.f64(P['gamma']), R.f64(P['beta'])
  assert np.array_equal(R.f64(res_buf)[res_rows_np], res64)
  alloc = cap + 5
  for p, seeded, kind in [(0.0, False, 'none'), (0.0, False, 'large')] + [(p, s, k) for p in (0.1, 0.5) for s in (False, True)
                                                                           for k in ROW_KINDS]:
    kw = pointers(kind)
    want_h16 = kw.pop('want_h16', True)
    thr, scale = ops.dropout_params(p)
    assert thr == D.thr16_of(p)
    orow = orow_of_kind(kind)
    keep = R.ln_site_keep(E.SITE_KEY, E.SEED if seeded else None, orow, d, thr) if thr else None
    ref = R.splitk_ln_fwd(slabs64, bias64, res64, keep, scale, gamma64, beta64, EPS)
    assert np.abs(ref['pre']).min() >= 1.0 and np.abs(res64).max() <= 4.0  # (of this file's own construction)
    z = torch.full((alloc, d), 7.0, device=dev)
    h32 = torch.full((alloc, d), 7.0, device=dev)
    h16 = torch.full((alloc, d), 7.0, device=dev, dtype=torch.bfloat16) if want_h16 else None
    mean, rstd = torch.full((alloc,), 7.0, device=dev), torch.full((alloc,), 7.0, device=dev)
    ops.splitk_ln_fwd(slabs_d, splits, P['stride'], bias_d, res_d, gamma_d, beta_d, EPS, z, h32, h16, mean, rstd, cap,
                      drop_key=E.SITE_KEY, drop_p=p, seed_dev=E._seed_dev(seeded), **kw)
    torch.cuda.synchronize()
    tag = '%s, p %g, %s, row numbers %s' % (name, p, 'seeded' if seeded else 'unseeded', kind)
    zg = R.f64(z)
    for nm, t in (('z', z), ('h32', h32), ('h16', h16), ('mean', mean), ('rstd', rstd)):
      if t is not None:
        assert bool((t[rows:] == 7.0).all()), '%s: %s was written past the live rows' % (tag, nm)
    if kw.get('rowidx_out') is not None:
      got_idx = kw['rowidx_out'].cpu().numpy()
      assert np.array_equal(got_idx[:rows], orow), '%s: rowidx_out' % tag
      assert (got_idx[rows:] == -7).all(), '%s: rowidx_out was written past the live rows' % tag
    bound = (splits + 3) * U32 * ref['mag']
    if thr:
      # (+-0.03 is six standard deviations of the rate only from ~10^4 elements on: a case with fewer has the reference
      # evaluated on the 64 row numbers that follow its own as well)
      more = orow if keep.size >= 16384 else np.concatenate([orow, orow[-1] + 1 + np.arange(64)])
      _keep_rate(tag, R.ln_site_keep(E.SITE_KEY, E.SEED if seeded else None, more, d, thr), p)
      _same_mask(tag, zg[:rows] != res64, keep)  # a dropped element is exactly z == res
      _within(tag + ', kept z', zg[:rows][keep], ref['z'][keep], bound[keep])
      assert np.array_equal(zg[:rows][~keep], res64[~keep])
    else:
      _within(tag + ', z', zg[:rows], ref['z'], bound)
    _close_np(tag + ', mean', R.f64(mean)[:rows], ref['mean'], 0.0, 1e-5)
    _close_np(tag + ', rstd', R.f64(rstd)[:rows], ref['rstd'], 0.0, 1e-5)
    _close_np(tag + ', h32', R.f64(h32)[:rows], ref['h'], 1e-5, 1e-5)
    if want_h16:
      _close_np(tag + ', h16', R.f64(h16)[:rows], ref['h'], 2e-2, 1e-2)


@pytest.mark.parametrize('d,splits,rows', LN_FWD_SHAPES)
def test_splitk_ln_fwd_tail_attention_out_site(d, splits, rows):
  """mmt_splitk_ln_fwd as the compact last layer's attention-output site calls it: the residual is gathered through
  res_rows from a larger buffer (distinct unsorted rows, row 0 and the last row among them; every other row of it is NaN),
  rowidx = NULL, the RNG row is row_index[res_rows[i]] -- or res_rows[i] without a row_index -- and is written to
  rowidx_out."""
  P = _ln_fwd_problem(d, splits, rows, rows, 310)
  g = torch.Generator().manual_seed(311)
  pick = torch.randperm(RES_ROWS - 2, generator=g)[:max(rows - 2, 0)].numpy() + 1
  res_rows = np.concatenate([[RES_ROWS - 1], pick, [0]])[:rows] if rows > 1 else np.array([RES_ROWS - 1])
  if rows > 2:
    assert 0 in res_rows and RES_ROWS - 1 in res_rows and len(set(res_rows.tolist())) == rows and (np.diff(res_rows) < 0).any()
  res_buf = torch.full((RES_ROWS, d), NAN)
  res_buf[torch.from_numpy(res_rows).long()] = P['res']
  tables = {k: E._row_numbers(k, RES_ROWS) for k in ROW_KINDS}

  def pointers(kind):
    return dict(res_rows=_i32(res_rows), row_index=tables[kind][1], rowidx_out=torch.full((rows + 5,), -7, dtype=torch.int32, device=_dev()))

  _ln_fwd_run_and_check('tail attention-out', P, pointers, lambda kind: tables[kind][0][res_rows], res_buf, res_rows)


@pytest.mark.parametrize('d,splits,rows', LN_FWD_SHAPES)
def test_splitk_ln_fwd_tail_ffn_out_site(d, splits, rows):
  """... as the tail's FFN-output site calls it: res_rows = NULL, the RNG rows given as rowidx (what the attention-out site
  wrote), row_index = NULL, h16 = NULL.  ('none': no rowidx either -- the RNG row is the row.)"""
  P = _ln_fwd_problem(d, splits, rows, rows, 320)
  res_buf = torch.full((rows + 3, d), NAN)
  res_buf[:rows] = P['res']
  tables = {k: E._row_numbers(k, rows) for k in ROW_KINDS}
  _ln_fwd_run_and_check('tail FFN-out', P, lambda kind: dict(rowidx=tables[kind][1], want_h16=False), lambda kind: tables[kind][0],
                        res_buf, np.arange(rows))


@pytest.mark.parametrize('d,splits,cap,live', [(256, 1, 1, 1), (512, 2, 56, 56), (768, 4, 203, 203), (1024, 16, 256, 203),
                                               (256, 8, 56, 1), (512, 4, 256, 203), (1024, 16, 203, 1)])
def test_splitk_ln_fwd_full_layer_packed(d, splits, cap, live):
  """mmt_splitk_ln_fwd_ex as a full layer of a packed batch calls it: rowidx = NULL, row_index given, n_rows_dev = live
  rows of `cap` launched ones (all of them, 1, 203 of 256); h32 and h16 both written.  Slabs, residual and row_index of the
  rows that are not live are NaN / garbage and nothing past the live rows is written."""
  P = _ln_fwd_problem(d, splits, live, cap, 330)
  res_buf = torch.full((cap + 3, d), NAN)
  res_buf[:live] = P['res']
  tables = {k: E._row_numbers(k, cap) for k in ROW_KINDS}
  n_rows_dev = _i32([live])
  _ln_fwd_run_and_check('full layer, %d of %d live' % (live, cap), P,
                        lambda kind: dict(row_index=tables[kind][1], n_rows_dev=n_rows_dev), lambda kind: tables[kind][0][:live],
                        res_buf, np.arange(live))


# ---- C. mmt_ln_bwd_slabs(_ex) ---------------------------------------------------------------------------------------------

def _ln_bwd_problem(d, splits, cap, live, seed):
  """slabs and residual gradient scaled by 1 / sqrt(splits + 1): the summed gradient has unit variance, as the dout of
  test_layernorm_fwd_bwd, whose tolerances are used.  Everything of the rows that are not live, and the unused slabs, is
  NaN."""
  stride = (cap + 127) // 128 * 128 * d
  sc = 1.0 / math.sqrt(splits + 1)
  slabs = torch.full((16, stride // d, d), NAN)
  slabs[:splits, :live] = _randn((splits, live, d), seed, sc)
  res = torch.full((cap, d), NAN)
  res[:live] = _randn((live, d), seed + 1, sc)
  z = torch.full((cap, d), NAN)
  z[:live] = _randn((live, d), seed + 2, 2.0) + 0.5
  gamma = 1.0 + 0.1 * _randn((d,), seed + 3)
  _, mean64, rstd64 = R.layer_norm(R.f64(z[:live]), np.ones(d), np.zeros(d), EPS)
  mean, rstd = torch.full((cap,), NAN), torch.full((cap,), NAN)
  mean[:live], rstd[:live] = torch.from_numpy(mean64).float(), torch.from_numpy(rstd64).float()
  return dict(d=d, splits=splits, cap=cap, live=live, stride=stride, slabs=slabs, res=res, z=z, gamma=gamma, mean=mean, rstd=rstd)


def _ln_bwd_run(P, dev_in, with_res=True, alias=False, **kw):
  """-> (dz, dy, partials, [dgamma, dbeta, dbias]) of one ops.ln_bwd_slabs call on sentinel-filled outputs; alias: dz is the
  buffer the residual gradient is read from, as in the engine."""
  from mmt_amd import _lib, ops
  d, cap, live = P['d'], P['cap'], P['live']
  rpb = _lib.lib().mmt_ln_bwd_rows_per_block(cap)
  nblk = (cap + rpb - 1) // rpb
  res = dev_in['res'].clone() if alias else (dev_in['res'] if with_res else None)
  dz = res if alias else torch.full((cap + 5, d), 7.0, device=_dev())
  dy = torch.full((cap + 5, d), 7.0, device=_dev(), dtype=torch.bfloat16)
  partials = torch.full((nblk + 1, 3, d), NAN, device=_dev())
  partials[nblk] = 7.0
  n_rows_dev = _i32([live]) if live != cap else None
  ops.ln_bwd_slabs(dev_in['slabs'], P['splits'], P['stride'], res, dev_in['z'], dev_in['mean'], dev_in['rstd'], dev_in['gamma'], dz, dy,
                   partials, cap, n_rows_dev=n_rows_dev, **kw)
  sums = ops.col_reduce(partials, nblk, 3, d)
  torch.cuda.synchronize()
  assert bool((partials[nblk] == 7.0).all()), 'partials were written past the last block'
  first_dead = (live + rpb - 1) // rpb  # blocks from here on hold no live row: their sums are exactly zero
  assert bool((partials[first_dead:nblk] == 0).all()), 'a block past the live rows contributes to the column sums'
  return dz, dy, partials[:nblk], sums


LN_BWD_SHAPES = [(256, 1, 56, 56), (512, 2, 203, 203), (768, 4, 56, 1), (1024, 16, 256, 203), (256, 4, 2061, 2061),
                 (512, 16, 203, 1), (1024, 2, 56, 56)]  # (d, splits, rows launched, live rows)


@pytest.mark.parametrize('d,splits,cap,live', LN_BWD_SHAPES)
def test_ln_bwd_slabs_against_fp64(d, splits, cap, live):
  """dz, dy, dgamma, dbeta, dbias of mmt_ln_bwd_slabs(_ex) against the fp64 LayerNorm backward of dout = sum_s slab_s + res,
  tolerances of test_layernorm_fwd_bwd; dbias is the column sum of the bf16 dy that was stored.  2061 rows: the
  two-rows-per-wave instantiation (16 rows per block, a partial last block).  Aliased dz / res as the engine runs it: bit
  equal to the out-of-place run.  Sentinels past the live rows hold, NaN in rows that are not live changes nothing."""
  P = _ln_bwd_problem(d, splits, cap, live, 340)
  dev_in = {k: P[k].to(_dev()) for k in ('slabs', 'res', 'z', 'gamma', 'mean', 'rstd')}
  dz, dy, partials, (dg, db, dbias) = _ln_bwd_run(P, dev_in)
  _, rdz, rdg, rdb = R.ln_bwd_slabs(R.f64(P['slabs'][:splits, :live]), R.f64(P['res'][:live]), R.f64(P['z'][:live]), R.f64(P['gamma']), EPS)
  assert bool((dz[live:] == 7.0).all()) and bool((dy[live:] == 7.0).all()), 'written past the live rows'
  _close_np('dz', R.f64(dz)[:live], rdz, 2e-5, 1e-4)
  _close_np('dy', R.f64(dy)[:live], rdz, 2e-2, 1e-2)
  _close_np('dgamma', R.f64(dg), rdg, 1e-3, 1e-4)
  _close_np('dbeta', R.f64(db), rdb, 1e-3, 1e-4)
  _close_np('dbias', R.f64(dbias), R.f64(dy)[:live].sum(0), 1e-3, 1e-4)
  dz2, dy2, partials2, _ = _ln_bwd_run(P, dev_in, alias=True)
  assert torch.equal(dz2[:live], dz[:live]) and torch.equal(dy2[:live], dy[:live]) and torch.equal(partials2, partials)
  assert bool(torch.isnan(dz2[live:]).all()), 'the aliased buffer was written past the live rows'


@pytest.mark.parametrize('seeded', [False, True])
@pytest.mark.parametrize('p', [0.1, 0.5])
@pytest.mark.parametrize('d,splits,cap,live', [(256, 2, 56, 56), (1024, 16, 256, 203), (256, 4, 2061, 2061)])
def test_ln_bwd_slabs_dropout_mask_is_the_documented_hash(d, splits, cap, live, p, seeded):
  """drop_mode 1: dy != 0 is keep_rows(eff_key, orow, d, thr) bit for bit for row numbers none / small / large, kept values
  are dz scale within the dy tolerance, and dz does not depend on the dropout."""
  from mmt_amd import ops
  P = _ln_bwd_problem(d, splits, cap, live, 350)
  dev_in = {k: P[k].to(_dev()) for k in ('slabs', 'res', 'z', 'gamma', 'mean', 'rstd')}
  dz0, _, _, _ = _ln_bwd_run(P, dev_in)
  _, rdz, _, _ = R.ln_bwd_slabs(R.f64(P['slabs'][:splits, :live]), R.f64(P['res'][:live]), R.f64(P['z'][:live]), R.f64(P['gamma']), EPS)
  thr, scale = ops.dropout_params(p)
  for kind in ROW_KINDS:
    orow, row_index = E._row_numbers(kind, cap)
    keep = R.ln_site_keep(E.SITE_KEY, E.SEED if seeded else None, orow[:live], d, thr)
    _keep_rate(kind, keep, p)
    dz, dy, _, (_, _, dbias) = _ln_bwd_run(P, dev_in, drop_mode=1, row_index=row_index, drop_key=E.SITE_KEY, drop_p=p,
                                           seed_dev=E._seed_dev(seeded))
    assert torch.equal(dz, dz0)
    assert bool((dy[live:] == 7.0).all())
    got = R.f64(dy)[:live]
    _same_mask('row numbers %s' % kind, got != 0, keep)
    _close_np('kept dy, row numbers %s' % kind, got[keep], (rdz * scale)[keep], 2e-2, 1e-2)
    _close_np('dbias, row numbers %s' % kind, R.f64(dbias), got.sum(0), 1e-3, 1e-4)


@pytest.mark.parametrize('d,cap,live', [(256, 56, 56), (768, 256, 203), (256, 2061, 2061)])
def test_ln_bwd_slabs_of_one_slab_is_ln_bwd(d, cap, live):
  """splits = 1, res = NULL: dz, dy and the partials are bit equal to mmt_ln_bwd on dout = slab 0 (adding zeros is exact)."""
  from mmt_amd import _lib, ops
  P = _ln_bwd_problem(d, 1, cap, live, 360)
  dev_in = {k: P[k].to(_dev()) for k in ('slabs', 'res', 'z', 'gamma', 'mean', 'rstd')}
  dz, dy, partials, _ = _ln_bwd_run(P, dev_in, with_res=False)
  dz1, dy1 = torch.full_like(dz, 7.0), torch.full_like(dy, 7.0)
  partials1 = torch.full_like(partials, NAN)
  n_rows_dev = _i32([live]) if live != cap else None
  p = ops._p
  _lib.check(_lib.lib().mmt_ln_bwd(p(dev_in['slabs']), p(dev_in['z']), p(dev_in['mean']), p(dev_in['rstd']), p(dev_in['gamma']), p(dz1), p(dy1),
                                   p(partials1), cap, d, 0, p(n_rows_dev), None, 0, 0, ctypes.c_float(1.0), None, ops._stream()), 'mmt_ln_bwd')
  torch.cuda.synchronize()
  assert torch.equal(dz, dz1) and torch.equal(dy, dy1) and torch.equal(partials, partials1)
  assert bool(torch.isfinite(dz[:live]).all())


# ---- D. the row-dot epilogue and its consumer -----------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _dot_problem(M, N, K):
  from mmt_amd import ops
  R_ = ops.pad_rows(M)
  a = _randn((R_, K), 401).to(torch.bfloat16)
  b = _randn((N, K), 402, 1.0 / math.sqrt(K)).to(torch.bfloat16)
  wide = _randn((R_, N + 64), 403).to(torch.bfloat16)  # dot_src = its columns 64 .. N + 64: lddot = N + 64
  return a, b, wide, (a[:M].double() @ b.double().t()).numpy()


def _check_row_dots(name, run, M, N, K, live=None, wide_src=True):
  """run(a, b, out, dot_src, dot_out) is the GEMM under test.  out against the fp64 product (2e-2 + 1e-2 |ref|);
  dot_out[row, g] against the fp64 sum over group g of float(out as STORED) float(dot_src), bound 64 2^-24 sum |terms|;
  rows >= M, or >= the live rows, keep the sentinel."""
  a, b, wide, want = _dot_problem(M, N, K)
  src = wide[:, 64:] if wide_src else wide[:, 64:].contiguous()
  wide_d = wide.to(_dev())
  src_d = wide_d[:, 64:] if wide_src else src.to(_dev())
  assert (src_d.stride(0) != N) == wide_src
  out = torch.full((a.shape[0], N), 7.0, device=_dev(), dtype=torch.bfloat16)
  dot = torch.full((a.shape[0], N // 64), 7.0, device=_dev())
  run(a.to(_dev()), b.to(_dev()), out, src_d, dot)
  torch.cuda.synchronize()
  n = M if live is None else live
  _close_np(name + ' out', R.f64(out)[:n], want[:n], 2e-2, 1e-2)
  dots, mags = R.row_dots(R.f64(out)[:n], R.f64(src)[:n])
  _within(name + ' dot_out', R.f64(dot)[:n], dots, 64 * U32 * mags)
  assert bool((dot[n:] == 7.0).all()), '%s: dot_out was written at or past row %d' % (name, n)
  assert bool((out[M:] == 7.0).all())


DOT_TILES = [13, 14, 18, 21, 24, 0, 1, 2]  # (1 / 2 have no row dots of their own: select_tile runs them as tile 13)


@pytest.mark.parametrize('tile', DOT_TILES)
def test_gemm_nt_row_dots(tile):
  """MmtEpilogue.dot_src / lddot / dot_out of every tile that can be selected with dot_out set: 13 / 14 / 18 (gemm2.hip), 21
  (gemm3.hip), 24 (gemm5.hip), the dispatcher's choice, and the forced ids 1 / 2, which the policy turns into 13.  300 rows
  (two 128-row tiles and a partial one) with a contiguous dot_src; 1100 rows of which 777 are live with dot_src a column
  slice of a wider buffer (lddot != N)."""
  from mmt_amd import ops
  _check_row_dots('tile %d, 300 x 256 x 128' % tile,
                  lambda a, b, out, src, dot: ops.gemm_nt(a, b, out, 'BF16', m=300, tile=tile, dot_src=src, dot_out=dot), 300, 256, 128,
                  wide_src=False)
  live = _i32([777])
  _check_row_dots('tile %d, 1100 x 512 x 128, 777 live' % tile,
                  lambda a, b, out, src, dot: ops.gemm_nt(a, b, out, 'BF16', m=1100, tile=tile, dot_src=src, dot_out=dot, n_rows_dev=live,
                                                          live_rows=777), 1100, 512, 128, live=777)


def test_gemm_nt_row_dots_argument_errors():
  """Tile 25 (gemm5.hip's 64-wide tile) has no row dots and says so; dot_out without dot_src is an error on every path."""
  from mmt_amd import ops
  a, b, wide, _ = _dot_problem(300, 256, 128)
  a, b, src = a.to(_dev()), b.to(_dev()), wide[:, 64:320].contiguous().to(_dev())
  out = torch.zeros(a.shape[0], 256, device=_dev(), dtype=torch.bfloat16)
  dot = torch.zeros(a.shape[0], 4, device=_dev())
  _raises_arg_error(lambda: ops.gemm_nt(a, b, out, 'BF16', m=300, tile=25, dot_src=src, dot_out=dot))
  ops.gemm_nt(a, b, out, 'BF16', m=300, tile=25)  # (the tile itself takes the shape)
  _raises_arg_error(lambda: ops.gemm_nt(a, b, out, 'BF16', m=300, dot_out=dot))
  _raises_arg_error(lambda: ops.gemm_nt_splitk(a, b, out, 'BF16', m=300, dot_out=dot))
  _raises_arg_error(lambda: ops.gemm_nt_splitk(a, b, torch.zeros(a.shape[0], 256, device=_dev()), 'F32', m=300, dot_src=src, dot_out=dot))
  torch.cuda.synchronize()


def test_gemm_nt_splitk_row_dots():
  """The split-K epilogue's row dots at 200 x 1024 x 1024 (the engine's d > 512 branch), dot_src a column slice."""
  from mmt_amd import ops
  _check_row_dots('split-K', lambda a, b, out, src, dot: ops.gemm_nt_splitk(a, b, out, 'BF16', m=200, dot_src=src, dot_out=dot),
                  200, 1024, 1024)


@functools.lru_cache(maxsize=None)
def _attn_dense_problem(B, S, H, DH):
  """Inputs of test_attention_fwd_bwd_dense and the fp64 autograd reference (R.attention_rows at every query)."""
  from mmt_amd import ops
  d, rows = H * DH, B * S
  Rp = ops.pad_rows(rows)
  qkv = _randn((Rp, 3 * d), 411).to(torch.bfloat16)
  dctx = _randn((Rp, d), 412).to(torch.bfloat16)
  valid = torch.rand(Rp, generator=torch.Generator().manual_seed(413)) > 0.3
  valid[::S] = True
  bias = (~valid).float() * -10000.0
  x = qkv[:rows].double().requires_grad_(True)
  ctx, _ = R.attention_rows(x, bias.double(), B, S, H, 1.0 / math.sqrt(DH), np.arange(rows), S)
  (ctx * dctx[:rows].double()).sum().backward()
  return qkv, dctx, bias, ctx.detach().numpy(), x.grad.numpy()


@pytest.mark.parametrize('B,S,H,DH', [(2, 70, 4, 128), (3, 30, 12, 64)])
def test_attention_backward_takes_delta_from_the_caller(B, S, H, DH):
  """mmt_attn_bwd_ex(delta_ready = 1): delta[row, g] = sum over the 64 columns of group g of dctx ctx (head h owns DH / 64
  groups), formed on the host in fp64 from the kernel's own bf16 ctx and rounded to fp32.  dqkv against the fp64 autograd
  reference at test_attention_fwd_bwd_dense's tolerances; the delta buffer is bit-identical afterwards (it was read, not
  recomputed).  delta_ready = 0 leaves behind a delta within 64 2^-24 sum |terms| of the host's.  A delta that is 4 too
  large everywhere must move dQ: the buffer is what the kernel uses."""
  from mmt_amd import ops
  d, rows, scale = H * DH, B * S, 1.0 / math.sqrt(DH)
  qkv, dctx, bias, rctx, rgrad = _attn_dense_problem(B, S, H, DH)
  qkv_d, dctx_d, bias_d = qkv.to(_dev()), dctx.to(_dev()), bias.to(_dev())
  ctx, lse = ops.attn_fwd(qkv_d, bias_d, B, S, H, scale)
  _close_np('ctx', R.f64(ctx)[:rows], rctx, 2e-2, 2e-2)
  dots, mags = R.row_dots(R.f64(dctx)[:rows], R.f64(ctx)[:rows])
  delta = torch.full((qkv.shape[0], d // 64), NAN, device=_dev())  # (rows past B S are never read)
  delta[:rows] = torch.from_numpy(dots).float().to(_dev())
  before = delta.clone()
  dqkv = ops.attn_bwd(qkv_d, bias_d, ctx, lse, dctx_d, B, S, H, scale, delta=delta, delta_ready=1)
  torch.cuda.synchronize()
  assert torch.equal(delta[:rows], before[:rows]) and bool(torch.isnan(delta[rows:]).all())
  for i, nm in enumerate('QKV'):
    _close_np('delta_ready = 1, d' + nm, R.f64(dqkv)[:rows, i * d:(i + 1) * d], rgrad[:, i * d:(i + 1) * d], 4e-2, 4e-2)
  left = torch.full_like(delta, 7.0)
  dqkv0 = ops.attn_bwd(qkv_d, bias_d, ctx, lse, dctx_d, B, S, H, scale, delta=left, delta_ready=0)
  torch.cuda.synchronize()
  _within('delta left behind', R.f64(left)[:rows], dots, 64 * U32 * mags)
  assert bool((left[rows:] == 7.0).all())
  for i, nm in enumerate('QKV'):
    _close_np('delta_ready = 0, d' + nm, R.f64(dqkv0)[:rows, i * d:(i + 1) * d], rgrad[:, i * d:(i + 1) * d], 4e-2, 4e-2)
  off = ops.attn_bwd(qkv_d, bias_d, ctx, lse, dctx_d, B, S, H, scale, delta=before + 4.0, delta_ready=1)
  assert float((off[:rows, :d].float() - dqkv[:rows, :d].float()).abs().max()) > 0.05


# ---- E. rows-only attention -----------------------------------------------------------------------------------------------

CU = [0, 11, 61, 91]  # packed samples of 11, 50, 30 rows (S = 50)


def _rows_problem(DH, S, packed, nq, seed):
  """(B, S, H) = (3, S, 2).  packed: cu_seqlens = CU and a row_index that maps the packed rows to scattered original
  positions (sample 1 keeps all 50).  Masked keys in every sample.  qsel: nq distinct unsorted rows per sample, its first
  row and its last live row among them."""
  from mmt_amd import ops
  B, H = 3, 2
  d = H * DH
  Rp = ops.pad_rows(B * S)
  g = torch.Generator().manual_seed(seed)
  qkv = _randn((Rp, 3 * d), seed + 1).to(torch.bfloat16)
  cu = np.array(CU) if packed else np.arange(B + 1) * S
  live = int(cu[-1])
  bias = torch.zeros(Rp)
  row_index = None
  if packed:
    pos = [np.sort(torch.randperm(S, generator=g)[:int(cu[b + 1] - cu[b])].numpy()) + b * S for b in range(B)]
    row_index = np.zeros(Rp, dtype=np.int64)
    row_index[:live] = np.concatenate(pos)
  qsel = []
  for b in range(B):
    n = int(cu[b + 1] - cu[b])
    bias[cu[b] + 2:cu[b] + 5] = -10000.0
    inner = torch.randperm(n - 2, generator=g)[:max(nq - 2, 0)].numpy() + 1
    rows = np.concatenate([[n - 1], inner, [0]]) if nq > 1 else np.array([n - 1 if b % 2 else 0])
    assert len(rows) == nq and len(set(rows.tolist())) == nq
    qsel.append(cu[b] + rows)
  return dict(B=B, S=S, H=H, DH=DH, d=d, qkv=qkv, bias=bias, cu=cu if packed else None, live=live, row_index=row_index,
              qsel=np.concatenate(qsel), nq=nq, scale=1.0 / math.sqrt(DH))


def _rows_forward(P, p, alloc_extra=3):
  from mmt_amd import ops
  B, S, H, d, nq = P['B'], P['S'], P['H'], P['d'], P['nq']
  n = B * nq
  ctx = torch.full((n + alloc_extra, d), 7.0, device=_dev(), dtype=torch.bfloat16)
  lse = torch.full((n + alloc_extra, H), 7.0, device=_dev())
  ops.attn_fwd_rows(P['qkv'].to(_dev()), P['bias'].to(_dev()), _i32(P['qsel']), nq, ctx, lse, B, S, H, P['scale'],
                    cu_seqlens=None if P['cu'] is None else _i32(P['cu']), drop_key=E.SITE_KEY, drop_p=p,
                    row_index=None if P['row_index'] is None else _i32(P['row_index']))
  torch.cuda.synchronize()
  assert bool((ctx[n:] == 7.0).all()) and bool((lse[n:] == 7.0).all()), 'the compact buffers were written past B nq rows'
  return ctx, lse


def _rows_reference(P, p, dctx):
  """fp64: ctx / lse at the selected queries and, through autograd of sum(ctx[sel] dctx), the gradient of qkv."""
  from mmt_amd import ops
  thr, sc = ops.dropout_params(p)
  keep = D.attn_mask(D.eff_key(E.SITE_KEY, None), P['B'], P['H'], P['S'], thr) if thr else None
  if keep is not None:
    _keep_rate('attention mask', keep, p)
  x = P['qkv'][:P['live']].double().requires_grad_(True)
  ctx, lse = R.attention_rows(x, P['bias'].double(), P['B'], P['S'], P['H'], P['scale'], P['qsel'], P['nq'], cu=P['cu'], keep=keep,
                              drop_scale=sc, row_index=P['row_index'])
  (ctx * dctx.double()).sum().backward()
  return ctx.detach().numpy(), lse.detach().numpy(), x.grad.numpy()


@pytest.mark.parametrize('p', [0.0, 0.1])
@pytest.mark.parametrize('nq', [1, 7])
@pytest.mark.parametrize('packed', [False, True])
@pytest.mark.parametrize('DH', [128, 64])
def test_attention_rows_fwd_bwd(DH, packed, nq, p):
  """mmt_attn_fwd_rows / mmt_attn_bwd_rows(_ex) against fp64 attention over all keys evaluated at the selected queries;
  dropout mask from dropout_ref.attn_mask at ORIGINAL (query, key) positions; tolerances of test_attention_fwd_bwd_dense
  (wrong rows or RNG coordinates move the results by O(1)).  The whole dqkv starts as a sentinel: afterwards the Q section
  of the non-selected live rows is exactly zero (the kernel clears it itself), the selected rows hold dQ, K and V sections
  of every live row match, rows past the live ones are untouched.  delta_ready = 0 (both entry points) and 1."""
  from mmt_amd import ops
  P = _rows_problem(DH, 50, packed, nq, 500 + DH + nq)
  B, S, H, d, live, n = P['B'], P['S'], P['H'], P['d'], P['live'], P['B'] * nq
  dctx = _randn((n + 3, d), 520).to(torch.bfloat16)
  rctx, rlse, rgrad = _rows_reference(P, p, dctx[:n])
  ctx, lse = _rows_forward(P, p)
  _close_np('ctx', R.f64(ctx)[:n], rctx, 2e-2, 2e-2)
  _close_np('lse', R.f64(lse)[:n], rlse, 2e-2, 2e-2)
  sel = np.zeros(live, dtype=bool)
  sel[P['qsel']] = True
  dots, _ = R.row_dots(R.f64(dctx)[:n], R.f64(ctx)[:n])
  args = (P['qkv'].to(_dev()), P['bias'].to(_dev()), _i32(P['qsel']), nq, ctx, lse, dctx.to(_dev()))
  kw = dict(cu_seqlens=None if P['cu'] is None else _i32(P['cu']), drop_key=E.SITE_KEY, drop_p=p,
            row_index=None if P['row_index'] is None else _i32(P['row_index']))
  for ready in (None, 0, 1):
    dqkv = torch.full((P['qkv'].shape[0], 3 * d), 7.0, device=_dev(), dtype=torch.bfloat16)
    delta = torch.full((n + 3, d // 64), 7.0, device=_dev())
    if ready:
      delta[:n] = torch.from_numpy(dots).float().to(_dev())
    before = delta.clone()
    ops.attn_bwd_rows(*args, dqkv, delta, B, S, H, P['scale'], delta_ready=ready, **kw)
    torch.cuda.synchronize()
    tag = 'delta_ready %s' % ready
    got = R.f64(dqkv)
    assert bool((delta[n:] == 7.0).all()) and (not ready or torch.equal(delta, before)), tag
    assert (got[live:] == 7.0).all(), '%s: dqkv was written past the live rows' % tag
    assert (got[:live, :d][~sel] == 0).all(), '%s: the Q section of a non-selected row is not zero' % tag
    _close_np(tag + ', dQ of the selected rows', got[:live, :d][sel], rgrad[:, :d][sel], 4e-2, 4e-2)
    assert np.abs(rgrad[:, :d][~sel]).max() == 0
    _close_np(tag + ', dK', got[:live, d:2 * d], rgrad[:, d:2 * d], 4e-2, 4e-2)
    _close_np(tag + ', dV', got[:live, 2 * d:], rgrad[:, 2 * d:], 4e-2, 4e-2)


@pytest.mark.parametrize('DH', [128, 64])
def test_attention_rows_fwd_on_the_eight_wave_kernel(DH):
  """nq = 70 at S = 100: more than 64 queries per sample run on the 8-wave forward kernel (dense, p = 0.1)."""
  P = _rows_problem(DH, 100, False, 70, 540 + DH)
  n = P['B'] * 70
  rctx, rlse, _ = _rows_reference(P, 0.1, torch.zeros(n, P['d']))
  ctx, lse = _rows_forward(P, 0.1)
  _close_np('ctx', R.f64(ctx)[:n], rctx, 2e-2, 2e-2)
  _close_np('lse', R.f64(lse)[:n], rlse, 2e-2, 2e-2)


def test_attention_rows_bwd_rejects_more_than_64_queries():
  """nq = 65 would start a second dQ block per (sample, head) that races with the first one's clear of the Q section: an
  argument error on both backward entry points, before anything is launched (the buffers stay as they are); nq = 64 runs."""
  from mmt_amd import ops
  P = _rows_problem(128, 100, False, 65, 560)
  d, n = P['d'], P['B'] * 65
  qkv, bias = P['qkv'].to(_dev()), P['bias'].to(_dev())
  ctx = torch.zeros(n, d, device=_dev(), dtype=torch.bfloat16)
  lse = torch.zeros(n, P['H'], device=_dev())
  dqkv = torch.full((qkv.shape[0], 3 * d), 7.0, device=_dev(), dtype=torch.bfloat16)
  delta = torch.full((n, d // 64), 7.0, device=_dev())
  for ready in (None, 0, 1):
    _raises_arg_error(lambda: ops.attn_bwd_rows(qkv, bias, _i32(P['qsel']), 65, ctx, lse, ctx, dqkv, delta, P['B'], P['S'], P['H'],
                                                P['scale'], delta_ready=ready))
  torch.cuda.synchronize()
  assert bool((dqkv == 7.0).all()) and bool((delta == 7.0).all())
  P64 = _rows_problem(128, 100, False, 64, 561)
  ops.attn_bwd_rows(qkv, bias, _i32(P64['qsel']), 64, ctx, lse, ctx, dqkv, delta, P['B'], P['S'], P['H'], P['scale'])
  torch.cuda.synchronize()


# ---- F. the two small tail-layer kernels ----------------------------------------------------------------------------------

@pytest.mark.parametrize('n,d,R_', [(1, 256, 9), (21, 768, 300), (203, 1024, 256)])
def test_rows_scatter_accumulate(n, d, R_):
  """mmt_rows_scatter(accumulate = 1) with distinct rows: every element gets ONE fp32 add, which is exact -- bit equal to
  index_add_; the other rows are unchanged."""
  from mmt_amd import ops
  g = torch.Generator().manual_seed(601)
  rows = torch.randperm(R_, generator=g)[:n]
  src, dst = _randn((n + 2, d), 602).to(_dev()), _randn((R_, d), 603).to(_dev())
  want = dst.clone().index_add_(0, rows.to(_dev()), src[:n])
  untouched = torch.ones(R_, dtype=torch.bool)
  untouched[rows] = False
  before = dst.clone()
  ops.rows_scatter(src, _i32(rows.numpy()), dst, accumulate=True)
  torch.cuda.synchronize()
  assert torch.equal(dst, want)
  assert torch.equal(dst[untouched.to(_dev())], before[untouched.to(_dev())])
  assert not torch.equal(dst, before)


@pytest.mark.parametrize('count_a,count_b', [(3 * 256 * 256, 3 * 256), (4 * 2048 * 256 + 1024, 3 * 256)])
def test_reduce_slabs_pair(count_a, count_b):
  """out = the sum of 4 slabs, both sets in one launch, bound (splits - 1) 2^-24 sum |terms|.  The second case has more than
  2048 blocks x 256 threads x 4 floats: the grid-stride loop takes a second sweep.  Nothing past `count` is written."""
  from mmt_amd import ops
  splits = 4
  ws_a, ws_b = _randn((splits * count_a,), 611).to(_dev()), _randn((splits * count_b,), 612).to(_dev())
  out_a, out_b = torch.full((count_a + 4,), 7.0, device=_dev()), torch.full((count_b + 4,), 7.0, device=_dev())
  ops.reduce_slabs_pair(ws_a, count_a, out_a, ws_b, count_b, out_b, splits)
  torch.cuda.synchronize()
  for nm, ws, out, count in (('a', ws_a, out_a, count_a), ('b', ws_b, out_b, count_b)):
    want, mag = R.reduce_slabs(R.f64(ws), splits, count)
    _within('set ' + nm, R.f64(out)[:count], want, (splits - 1) * U32 * mag)
    assert bool((out[count:] == 7.0).all())


def test_reduce_slabs_pair_rejects_counts_that_are_no_multiple_of_4():
  from mmt_amd import ops
  ws, out = torch.zeros(4 * 64, device=_dev()), torch.full((64,), 7.0, device=_dev())
  for ca, cb in ((62, 64), (64, 62), (63, 61)):
    _raises_arg_error(lambda: ops.reduce_slabs_pair(ws, ca, out, ws, cb, out, 4))
  torch.cuda.synchronize()
  assert bool((out == 7.0).all())
