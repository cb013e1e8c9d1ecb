"""Row-sharded InfoNCE (model/loss.py:68-81 on a row block; mmt_amd/large_sim.py, largesim.hip: mmt_ls_nce_stats /
mmt_ls_nce_grad): the two kernels against fp64 through the C ABI, the phases on simulated ranks and the nn.Module on a real
process group against autograd through the oracle on the full matrix."""
import functools
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

# (b, n, r0, M): a partial last row tile with the diagonal inside the block | several row tiles and row groups, the M > 8
# kernels, more than one column block of either pass (4096 and 8192 columns) and a ragged last chunk of 4 columns
SHAPES = [(43, 2560, 256, 7), (300, 9220, 8900, 12)]
# (multiplier of the raw numerators, scale): the reference's logits | logits of several hundred (exp overflows fp32)
RANGES = {'unit': (1.0, 1.0), 'huge': (200.0, 2.0)}
ZERO_COL = 5  # a video with all-zero weights: den == 0 -> 1e-5 (model.py:816); its numerators are 0, as the fold produces


@functools.lru_cache(maxsize=None)
def _block(b, n, r0, m, rng):
  """The raw block, its weights, and the fp64 references; computed once and shared (nothing below writes to them)."""
  from mmt_amd import _lib, ops
  from mmt_amd._lib import check
  L = _lib.lib()
  mult, scale = RANGES[rng]
  g = torch.Generator(device=DEV).manual_seed(5)
  raw = torch.randn(b, n, device=DEV, generator=g) * (0.05 * mult)
  tw = torch.softmax(torch.randn(b, m, device=DEV, generator=g), -1)
  vw = torch.softmax(torch.randn(n, m, device=DEV, generator=g), -1)
  vw[ZERO_COL] = 0.0
  raw[:, ZERO_COL] = 0.0
  S = raw.clone()  # the fp32 similarities: the same bits the kernels divide to (largesim.hip ls_quot)
  check(L.mmt_ls_finish(ops._p(S), n, ops._p(tw), ops._p(vw), b, n, m, ops._stream()), 'finish')
  z64 = scale * S.double()
  z32 = (scale * S)
  row_ref, col_ref = torch.logsumexp(z64, 1), torch.logsumexp(z64, 0)
  # the yardstick: fp32 torch.logsumexp's own error on the same rows and columns
  e_row = (torch.logsumexp(z32, 1).double() - row_ref).abs().max().item()
  e_col = (torch.logsumexp(z32, 0).double() - col_ref).abs().max().item()
  return dict(raw=raw, tw=tw, vw=vw, vw_t=vw.t().contiguous(), S=S, z64=z64, scale=scale, row_ref=row_ref, col_ref=col_ref,
              e_row=e_row, e_col=e_col)


def _ulp32(x64):
  a = x64.abs().float()
  return (torch.nextafter(a, torch.full_like(a, float('inf'))) - a).double()


@pytest.mark.parametrize('use_vwt', [True, False])
@pytest.mark.parametrize('rng', ['unit', 'huge'])
@pytest.mark.parametrize('b,n,r0,m', SHAPES)
def test_nce_stats_kernel_matches_fp64_logsumexp(b, n, r0, m, rng, use_vwt):
  """mmt_ls_nce_stats: row and column logsumexp of scale * S from the kernel's (max, sum-exp) partials against fp64
  torch.logsumexp, within 4 x the error of fp32 torch.logsumexp on the same data (another summation order) + one fp32 ulp of
  the result; S untouched; two runs bit-identical."""
  from mmt_amd import _lib, ops
  from mmt_amd._lib import check
  from mmt_amd.large_sim import RowBlock
  L = _lib.lib()
  x = _block(b, n, r0, m, rng)
  S = x['raw'].clone()
  ncb, nrg = L.mmt_ls_nce_col_blocks(n), L.mmt_ls_nce_row_groups(b)
  assert ncb == -(-n // 4096) and nrg == -(-b // 128)
  # the column workspace at the workload's own size: at most 1/16 of the row block's bytes
  assert L.mmt_ls_nce_row_groups(8192) * 2 * 65536 * 4 * 16 <= 8192 * 65536 * 4

  def run():
    rp = torch.full((2, b, ncb), float('nan'), device=DEV)
    cp = torch.full((nrg, 2, n), float('nan'), device=DEV)
    check(L.mmt_ls_nce_stats(ops._p(S), n, ops._p(x['tw']), ops._p(x['vw']), ops._p(x['vw_t']) if use_vwt else None, b, n, m, r0,
                             x['scale'], ops._p(rp), ops._p(cp), ops._stream()), 'nce_stats')
    return rp, cp
  rp, cp = run()
  assert torch.equal(S, x['raw'])                                  # the row block is never rewritten
  assert torch.isfinite(rp).all() and torch.isfinite(cp).all()     # (every partial written, none overflowed)
  top, sm = RowBlock.nce_merge(rp[0], rp[1], 1)
  row = (top + torch.log(sm)).float().double()
  top, sm = RowBlock.nce_merge(cp[:, 0], cp[:, 1], 0)
  col = RowBlock.nce_col_lse(torch.stack([top, sm]).float()[None]).double()
  for name, got, ref, e32 in (('row', row, x['row_ref'], x['e_row']), ('col', col, x['col_ref'], x['e_col'])):
    err = (got - ref).abs()
    tol = 4.0 * e32 + _ulp32(ref)
    print('nce_stats %s b=%d n=%d M=%d %s vwt=%d: kernel err %.3e, fp32 logsumexp err %.3e, min tol %.3e'
          % (name, b, n, m, rng, use_vwt, err.max().item(), e32, tol.min().item()))
    assert (err <= tol).all(), (name, err.max().item(), e32)
  rp2, cp2 = run()
  assert torch.equal(rp, rp2) and torch.equal(cp, cp2)


@pytest.mark.parametrize('use_vwt', [True, False])
@pytest.mark.parametrize('rng', ['unit', 'huge'])
@pytest.mark.parametrize('b,n,r0,m', SHAPES)
def test_nce_grad_kernel_matches_fp64(b, n, r0, m, rng, use_vwt):
  """mmt_ls_nce_grad: G' = bf16(g / den) against fp64 (bf16 rounds to 2^-9 relative; 2^-8 allowed), the diagonal's -2 scale / n
  term explicitly, and the gs partial sums against the fp64 sum over the kernel's own rounded G'."""
  from mmt_amd import _lib, ops
  from mmt_amd._lib import check
  L = _lib.lib()
  x = _block(b, n, r0, m, rng)
  S = x['raw'].clone()
  scale, z64 = x['scale'], x['z64']
  row_lse, col_lse = x['row_ref'].float(), x['col_ref'].float()   # (the block stands for the whole matrix's rows here)
  ncb = L.mmt_ls_col_blocks(n)
  g16 = torch.full((b, n), float('nan'), device=DEV, dtype=torch.bfloat16)
  gs = torch.full((b, ncb, m), float('nan'), device=DEV)
  check(L.mmt_ls_nce_grad(ops._p(S), n, ops._p(x['tw']), ops._p(x['vw']), ops._p(x['vw_t']) if use_vwt else None, ops._p(row_lse),
                          ops._p(col_lse), b, n, m, r0, scale, 1.0 / n, ops._p(g16), n, ops._p(gs), ops._stream()), 'nce_grad')
  assert torch.equal(S, x['raw'])
  den = x['tw'].double() @ x['vw'].double().t()
  zero = den == 0
  assert bool(zero[:, ZERO_COL].all()) and int(zero.sum()) == b
  den = torch.where(zero, torch.full_like(den, 1e-5), den)
  g = torch.exp(z64 - row_lse.double()[:, None]) + torch.exp(z64 - col_lse.double()[None, :])
  t = torch.arange(b, device=DEV)
  g[t, r0 + t] -= 2.0
  want = g * (scale / n) / den
  got = g16.double()
  excess = ((got - want).abs() - (2.0 ** -8 * want.abs() + 1e-12)).max().item()
  print('nce_grad b=%d n=%d M=%d %s vwt=%d: max (|dG| - bound) %.3e' % (b, n, m, rng, use_vwt, excess))
  assert excess <= 0.0
  dg, dw = got[t, r0 + t], want[t, r0 + t]
  if rng == 'unit':
    assert bool((dw < 0).all())                                     # (the -2 dominates: the check below is about that term)
  assert ((dg - dw).abs() <= 2.0 ** -8 * dw.abs() + 1e-12).all()
  # gs = sum_v G' S vw over the kernel's own G', nothing from the 1e-5 column
  keep = (~zero).double()
  keep[:, ZERO_COL] = 0.0
  gs_want = (got * x['S'].double() * keep) @ x['vw'].double()
  gs_got = gs.sum(1).double()
  assert torch.isfinite(gs).all()
  assert (gs_got - gs_want).abs().max().item() <= 1e-5 * gs_want.abs().max().item()


# ---- the phases on simulated ranks ---------------------------------------------------------------------------------

def _inputs():
  rs = np.random.RandomState(7)
  n, m, d = 512, 3, 128
  vid = torch.nn.functional.normalize(torch.from_numpy(rs.randn(n, m, d).astype(np.float32)), dim=-1)
  txt = torch.nn.functional.normalize(torch.from_numpy(rs.randn(n, m, d).astype(np.float32)) + 0.5 * vid, dim=-1)
  tw = torch.softmax(torch.from_numpy(rs.randn(n, m).astype(np.float32)), -1)
  vw = torch.full((n, m), 1.0 / m)
  return vid, txt, tw, vw


@functools.lru_cache(maxsize=None)
def _oracle(scale):
  from oracle import mmt_oracle as O
  vid, txt, tw, vw = _inputs()
  leaves = [x.clone().requires_grad_(True) for x in (vid, txt, tw)]
  sims = O.cross_view_inner_product(leaves[0], leaves[1][:, :, None, :], vw, leaves[2][:, None, :], 'avg')
  loss = O.info_nce_loss(scale * sims)
  loss.backward()
  return dict(sims=sims.detach(), loss=loss.item(), dvid=leaves[0].grad, dtxt=leaves[1].grad, dtw=leaves[2].grad)


def _phases(world, scale):
  """The phases of RowBlock with the collectives done by hand."""
  from mmt_amd.large_sim import RowBlock
  vid, txt, tw, vw = _inputs()
  n = vid.shape[0]
  b = n // world
  blocks = [RowBlock(txt[r * b:(r + 1) * b].to(DEV), tw[r * b:(r + 1) * b].to(DEV), vid.to(DEV), vw.to(DEV), r * b, 0.0)
            for r in range(world)]
  diag = torch.cat([blk.phase_similarity() for blk in blocks])                     # (each rank keeps its own part)
  stats = [blk.phase_nce_stats(scale) for blk in blocks]
  col_lse = RowBlock.nce_col_lse(torch.stack([s[0] for s in stats]))               # all-gather + combine in rank order
  loss = sum(blk.phase_nce_loss(col_lse) for blk in blocks)                        # all-reduce
  outs = [blk.phase_nce_backward(col_lse) for blk in blocks]
  q = sum(o[2] for o in outs)                                                      # reduce-scatter
  dvid = torch.cat([blocks[r].phase_video_grad(q[r * b:(r + 1) * b], vid[r * b:(r + 1) * b].to(DEV), vw[r * b:(r + 1) * b].to(DEV))
                    for r in range(world)]).cpu()
  return dict(diag=diag.cpu(), S=torch.cat([blk.similarity() for blk in blocks]).cpu(), loss=loss.item(), dvid=dvid,
              dtxt=torch.cat([o[0] for o in outs]).cpu(), dtw=torch.cat([o[1] for o in outs]).cpu(),
              col_lse=col_lse.cpu(), row_lse=torch.cat([s[1] for s in stats]).cpu())


@functools.lru_cache(maxsize=None)
def _phases_cached(world, scale):
  return _phases(world, scale)


def _cos(a, b):
  a, b = a.double().reshape(-1), b.double().reshape(-1)
  return float(a @ b / (a.norm() * b.norm()))


def _check_against_oracle(got, ref, scale, tag):
  e_s = (got['S'] - ref['sims']).abs().max().item()
  assert e_s < 2e-3                                                               # bf16 operands
  # each cross-entropy term is 1-Lipschitz in the sup norm through its logsumexp and through the diagonal
  assert abs(got['loss'] - ref['loss']) <= 4.0 * scale * e_s + 1e-6, (got['loss'], ref['loss'], e_s)
  for nm in ('dvid', 'dtxt', 'dtw'):
    cos, ratio = _cos(got[nm], ref[nm]), got[nm].norm().item() / ref[nm].norm().item()
    print('%s %s: cos %.6f, norm ratio %.5f' % (tag, nm, cos, ratio))
    assert cos > 0.995 and abs(ratio - 1.0) < 0.03, (nm, cos, ratio)
  return e_s


@pytest.mark.parametrize('world', [1, 2, 4])
def test_row_sharded_infonce_matches_oracle(world):
  """n = 512 pairs over `world` simulated ranks at the reference's scale = 1 against autograd through
  oracle.cross_view_inner_product + oracle.info_nce_loss on the full matrix."""
  got, ref = _phases_cached(world, 1.0), _oracle(1.0)
  assert (got['diag'] - ref['sims'].diagonal()).abs().max() < 2e-3
  e_s = _check_against_oracle(got, ref, 1.0, 'world %d' % world)
  print('world %d: e_S %.3e, |loss - ref| %.3e' % (world, e_s, abs(got['loss'] - ref['loss'])))


def test_row_sharded_infonce_at_scale_100_is_finite_and_consistent():
  """A learned temperature of 1/100: logits of +-100, exp(z) overflows fp32 -- only the max subtraction keeps it finite."""
  ref = _oracle(100.0)
  runs = [_phases_cached(w, 100.0) for w in (1, 2, 4)]
  for r in runs:
    assert all(torch.isfinite(r[k]).all() for k in ('dvid', 'dtxt', 'dtw', 'col_lse', 'row_lse')) and np.isfinite(r['loss'])
    e_s = (r['S'] - ref['sims']).abs().max().item()
    bound = 4.0 * 100.0 * e_s + 1e-6
    assert abs(r['loss'] - ref['loss']) <= bound, (r['loss'], ref['loss'], bound)
    assert abs(r['loss'] - runs[0]['loss']) <= bound


def test_sharded_infonce_module_is_one_row_block_without_a_process_group():
  from mmt_amd.large_sim import ShardedInfoNceLoss
  vid, txt, tw, vw = _inputs()
  want = _phases_cached(1, 1.0)

  def run():
    lv = [x.clone().to(DEV).requires_grad_(True) for x in (vid, txt, tw)]
    loss = ShardedInfoNceLoss()(lv[0], lv[1][:, :, None, :], vw.to(DEV), lv[2][:, None, :])
    loss.backward()
    return [loss.detach().cpu()] + [x.grad.cpu() for x in lv]
  a, b = run(), run()
  assert abs(a[0].item() - want['loss']) < 1e-6
  for got, nm in zip(a[1:], ('dvid', 'dtxt', 'dtw')):
    assert (got - want[nm]).abs().max() < 1e-6, nm
  assert all(torch.equal(x, y) for x, y in zip(a, b))                             # a second invocation is bit-identical
  again = _phases(1, 1.0)
  assert all(torch.equal(again[k], want[k]) for k in ('dvid', 'dtxt', 'dtw', 'col_lse', 'row_lse')) and again['loss'] == want['loss']
  with pytest.raises(NotImplementedError):
    ShardedInfoNceLoss()(vid.to(DEV), txt.to(DEV), vw.to(DEV).requires_grad_(True), tw.to(DEV))


# ---- a real process group ----------------------------------------------------------------------------------------------

def _free_port():
  s = socket.socket()
  s.bind(('127.0.0.1', 0))
  p = s.getsockname()[1]
  s.close()
  return p


def _nce_worker(rank, world, port, out):
  os.environ['MASTER_ADDR'] = '127.0.0.1'
  os.environ['MASTER_PORT'] = str(port)
  torch.cuda.set_device(0)
  dist.init_process_group('gloo', rank=rank, world_size=world)
  from mmt_amd.large_sim import ShardedInfoNceLoss
  vid, txt, tw, vw = _inputs()
  b = vid.shape[0] // world
  sl = slice(rank * b, (rank + 1) * b)
  lv = [x[sl].clone().cuda().requires_grad_(True) for x in (vid, txt, tw)]
  loss = ShardedInfoNceLoss(1.0)(lv[0], lv[1][:, :, None, :], vw[sl].cuda(), lv[2][:, None, :])
  loss.backward()
  torch.save(dict(loss=float(loss.item()), dvid=lv[0].grad.cpu(), dtxt=lv[1].grad.cpu(), dtw=lv[2].grad.cpu()),
             '%s.%d' % (out, rank))
  dist.barrier()
  dist.destroy_process_group()


def test_sharded_infonce_with_a_real_process_group_matches_oracle(tmp_path):
  """Two gloo ranks sharing this GPU: the all-gathers, the all-gather of the column statistics, the all-reduce of the loss
  and the reduce-scatter of the video gradients are real."""
  out = str(tmp_path / 'nce')
  mp.spawn(_nce_worker, args=(2, _free_port(), out), nprocs=2, join=True)
  r = [torch.load(out + '.%d' % i) for i in range(2)]
  assert abs(r[0]['loss'] - r[1]['loss']) <= 1e-7
  ref = _oracle(1.0)
  got = dict(S=_phases_cached(2, 1.0)['S'], loss=r[0]['loss'], dvid=torch.cat([x['dvid'] for x in r]),
             dtxt=torch.cat([x['dtxt'] for x in r]), dtw=torch.cat([x['dtw'] for x in r]))
  _check_against_oracle(got, ref, 1.0, 'gloo x2')
