"""Proves tests/large_sim_ref.py before tests/test_large_sim_mm_gpu.py judges a kernel with it, on a machine without a GPU: the
restatement is the oracle's loss, counts and gradient; the inputs of every case leave no hinge inside the band in which fp32
and fp64 may decide differently (so the GPU tests demand exact counts); the tie case is exactly representable and ties where
it says; and one lost hinge, or one lost column of gs, lies outside the GPU tests' tolerances."""
import pytest
import torch

from oracle import mmt_oracle as O
from tests import large_sim_ref as R


def _square(n=24, M=3, seed=3):
  g = torch.Generator().manual_seed(seed)
  raw = torch.randn(n, n, generator=g) * 0.05
  tw = torch.softmax(torch.randn(n, M, generator=g), -1)
  vw = torch.softmax(torch.randn(n, M, generator=g), -1)
  vw[5], tw[2] = 0.0, 0.0
  return raw, tw, vw


@pytest.mark.parametrize('margin', [0.05, -0.01])
@pytest.mark.parametrize('fix_norm', [True, False])
@pytest.mark.parametrize('bs', [24, 12, 8])
def test_reference_is_the_oracle(bs, fix_norm, margin):
  """n = 24, M = 3 split into row blocks of bs rows: loss, counts and gradient against oracle.max_margin_ranking_loss (fp64
  autograd) on the whole matrix and oracle.max_margin_rows on each block."""
  raw, tw, vw = _square()
  n = raw.shape[0]
  den, zero = R.den_of(tw, vw)
  assert int(zero.sum()) == 2 * n - 1
  s = R.similarities(raw, tw, vw).requires_grad_(True)
  loss = O.max_margin_ranking_loss(s, margin, fix_norm)
  loss.backward()
  norm = 2.0 * n * (n - 1) if fix_norm else 2.0 * n * n
  want, s = s.grad, s.detach()
  diag = s.diagonal().clone()
  blocks = [R.counts(s[r0:r0 + bs], diag, r0, margin) for r0 in range(0, n, bs)]
  total = sum(float(p.sum()) for _, _, p in blocks) / norm
  if not fix_norm:
    total += 2.0 * n * max(margin, 0.0) / norm       # (the diagonal's two constant hinges: ShardedSimLoss adds them on the host)
  assert abs(total - loss.item()) <= 1e-12
  colcnt = sum(c for _, c, _ in blocks)
  for k, r0 in enumerate(range(0, n, bs)):
    rows = torch.arange(r0, r0 + bs)
    G = R.grad(s[rows], den[rows], diag, r0, margin, blocks[k][0], colcnt, 1.0 / norm)
    assert (G * den[rows] - want[rows]).abs().max().item() <= 1e-15
    if fix_norm:
      # (the rows' own column hinges are part of max_margin_rows' count only through col_hinge_counts)
      _, g, rowcnt = O.max_margin_rows(s[rows], rows, diag, margin, n, colcnt[rows])
      assert torch.equal(rowcnt, blocks[k][0])
      assert (G * den[rows] - g).abs().max().item() <= 1e-15


def test_case_list_is_the_issue_s():
  assert R.CASES == [(4, 4, 0, 1), (43, 2560, 256, 7), (21, 9220, 8185, 12), (19, 1028, 1009, 8), (19, 1028, 1009, 9), (37, 2052, 1003, 16)]
  assert R.MARGIN == float(torch.tensor(0.05, dtype=torch.float32))
  assert R.ncb(8192) == 1 and R.ncb(9220) == 2


@pytest.mark.parametrize('name', R.NAMES[:-1])
def test_no_hinge_is_in_band(name):
  """The condition the exact counts of the GPU tests rest on, and that both branches of every decision are exercised.  The
  4 x 4 case has 12 off-diagonal elements, M = 1 and den == 1 (or 1e-5 on raw * 1e-5): h = 0.05 + N(0, 2 * 0.05^2) is positive
  with probability 0.76, so the 30 % .. 70 % window of the other cases (where s = raw / den is about M times larger and
  dominates the margin) does not apply to it -- 9 and 10 of its 12 hinges are active; it must show both outcomes."""
  r = R.reference(name)
  assert r['in_band'] == 0
  off = r['off']
  n_off = int(off.sum())
  assert n_off == r['b'] * r['n'] - r['b']
  a1, a2 = int(((r['h1'] > 0) & off).sum()), int(((r['h2'] > 0) & off).sum())
  print('case %s: active %.3f / %.3f of %d, den == 0 at %d' % (name, a1 / n_off, a2 / n_off, n_off, int(r['zero'].sum())))
  if n_off >= 1000:
    assert 0.3 <= a1 / n_off <= 0.7 and 0.3 <= a2 / n_off <= 0.7
  else:
    assert 2 <= a1 <= n_off - 2 and 2 <= a2 <= n_off - 2
  nz = int(r['zero'].sum())
  assert nz > 0
  if r['n'] > 5:
    assert nz == r['b'] + r['n'] - 1                   # text 2 and video 5
    assert bool((r['s'].abs()[r['zero']] > 1e-4).any())  # the 1e-5 branch gives similarities of ordinary size
  assert bool(r['rowcnt'].max() > 0) and bool(r['colcnt'].max() > 0)


def test_tie_case_is_exact_and_ties():
  r = R.reference('tie')
  off, n_off = r['off'], int(r['off'].sum())
  assert (r['b'], r['n'], r['r0'], r['M']) == (19, 1028, 1009, 4) and r['margin'] == 2.0 ** -4
  assert int(((r['h1'] == 0) & off).sum()) >= 0.05 * n_off and int(((r['h2'] == 0) & off).sum()) >= 0.05 * n_off
  assert int(r['zero'].sum()) == 2 * r['b'] + r['n'] - 2
  assert bool(((r['den'] == 1.0) | r['zero']).all()) and bool((r['raw'][r['zero']] == 0).all())
  for k in ('raw', 'diag'):
    assert torch.equal(r[k] * 64.0, (r[k] * 64.0).round()) and r[k].abs().max().item() <= 0.5
  for k in ('s', 'h1', 'h2', 'loss_part'):             # every value the kernels form is an fp32 number
    assert torch.equal(r[k].float().double(), r[k]), k
    assert torch.equal(r[k] * 64.0, (r[k] * 64.0).round()), k
  assert r['loss_part'].abs().max().item() < 2.0 ** 12   # < 2^24 units of 2^-6: partial sums in any order are exact too
  # `>=` for `>` would count every tie
  assert int(((r['h1'] >= 0) & off).sum()) - int(r['rowcnt'].sum()) > 500


@pytest.mark.parametrize('name', R.NAMES)
def test_one_lost_hinge_or_column_is_outside_the_tolerances(name):
  """For every (row, column block): dropping the median active hinge moves loss_part by more than its tolerance; for every
  (row, column block, expert): dropping the median non-zero term moves gs by more than its tolerance."""
  r = R.reference(name)
  b, n = r['b'], r['n']
  z = torch.full_like(r['h1'], float('nan'))
  act = torch.cat([torch.where((r['h1'] > 0) & r['off'], r['h1'], z), torch.where((r['h2'] > 0) & r['off'], r['h2'], z)], 0)  # [2b, n]
  G16 = r['G'].to(torch.bfloat16)
  terms = R.gs_terms(G16, r['s'], r['vw'], r['zero']).abs()
  terms = torch.where(terms > 0, terms, torch.full_like(terms, float('nan')))
  tol_gs = R.gs_tol(G16, r['s'], r['vw'], r['zero'], r['M'])
  seen = 0
  for cb in range(R.ncb(n)):
    sl = slice(cb * R.CPB, min(n, (cb + 1) * R.CPB))
    a = act[:, sl]
    med = torch.nanmedian(torch.cat([a[:b], a[b:]], 1), 1).values       # per row, both kinds of hinge pooled
    ok = torch.isnan(med) | (med > r['loss_tol'][:, cb])
    assert bool(ok.all()), (name, cb, med, r['loss_tol'][:, cb])
    seen += int((~torch.isnan(med)).sum())
    # a kernel that loses column v is outside the bound if some (row, expert) sees v's term above twice the tolerance (the
    # kernel's own error may take up one): every column, but those whose den is 0 in every row and contribute nothing
    loud = (terms[:, sl] > 2.0 * tol_gs[:, cb][:, None, :]).any(2).any(0)
    silent = r['zero'][:, sl].all(0)
    assert bool((loud | silent).all()), (name, cb, int((~(loud | silent)).sum()))
    assert int(silent.sum()) <= 2
    # ... and for (row, expert) pairs one by one: the median non-zero term is above the tolerance in 99 % of them (one pair of
    # the 9220-column case's second block, where the diagonal's term is 5000 times an ordinary one, sits at 0.93)
    medg = torch.nanmedian(terms[:, sl], 1).values                      # [b, M]
    okg = (medg > tol_gs[:, cb])[~torch.isnan(medg)]
    assert okg.double().mean().item() >= 0.99, (name, cb, okg.double().mean().item())
  assert seen >= min(b, 3)


@pytest.mark.parametrize('i', range(len(R.HOST_SHAPES)))
def test_host_shapes_leave_few_hinges_near_zero(i):
  """The host-path test reads the similarities back from a bf16 GEMM on the GPU, so its band cannot be emptied in advance: a
  count may differ by the in-band elements of its row or column.  Here, for the fp64 product of the bf16 operands with the band
  widened by the GEMM bound / den: at most 0.1 % of the block."""
  h = R.host_reference(i)
  assert (h['b'], h['n'], h['r0'], h['M'], h['d']) in ((128, 256, 128, 3, 128), (43, 384, 300, 9, 128))
  x = R.host_block(i, h['raw'], h['diag'])
  den, zero = R.den_of(x['tw'], x['vw'])
  assert int(zero.sum()) == h['b'] + h['n'] - 1 and bool((h['raw'][zero] == 0).all())
  s = h['raw'] / den
  b1, b2, h1, h2, off = R.bands(x, s)
  w = h['raw_bound'] / den
  near = int((((h1.abs() <= b1 + w) | (h2.abs() <= b2 + w)) & off).sum())
  a1, a2 = ((h1 > 0) & off).double().mean().item(), ((h2 > 0) & off).double().mean().item()
  print('host shape %d: %d of %d near 0, active %.3f / %.3f' % (i, near, int(off.sum()), a1, a2))
  assert near <= 1e-3 * h['b'] * h['n']
  assert 0.3 <= a1 <= 0.7 and 0.3 <= a2 <= 0.7
