"""Proves the harness of tests/test_attention_bounds_gpu.py before it judges a kernel, on a machine without a GPU, for every
case of that file: the fp64 reference of tests/attention_ref.py is the autograd gradient of engine_paths_ref.attention_rows;
an emulation of the kernels' rounding points lies INSIDE the bound (the bound does not reject correct arithmetic); and every
tile-edge mutant -- the same attention with one edge key, or one edge query, lost -- lies OUTSIDE it at the stated shares
(an in-bound kernel error cannot hide a lost row).  The shares are conditions on the inputs, not measurements: a case that
misses one gets louder inputs (attention_ref.problem's amp2 / dgain), never a smaller share or a smaller bound."""
import numpy as np
import pytest
import torch

from tests import attention_ref as A
from tests import engine_paths_ref as R

ALL = [(c, DH) for c in A.CASES for DH in A.DHS]
SHARE = dict(ctx=0.05, dV=0.05, dQ=0.01, dK=0.01)  # least share of elements a mutant moves by more than 2 x the bound
LSE_MOVES = 10.0                                   # ... and every lse entry by more than this many bounds


def _outputs(P):
  return ('lse', 'ctx') if P['nq'] else A.OUTPUTS  # (the rows-only cases judge the forward only)


def test_case_list_is_the_issue_s():
  assert A.DENSE_S == (1, 16, 17, 63, 64, 65, 127, 128, 129, 192, 193, 257)
  assert A.problem('varlen-S193', 64)['cu'].tolist() == [0, 1, 65, 194, 387]
  assert A.problem('varlen-S130', 64)['cu'].tolist() == [0, 63, 128, 256]
  assert A.edges(1) == [0] and A.edges(64) == [0, 63] and A.edges(65) == [0, 63, 64]
  assert A.edges(193) == [0, 63, 64, 127, 128, 191, 192] and A.edges(257) == [0, 63, 64, 127, 128, 191, 192, 255, 256]
  P = A.problem('rows-S129-nq65', 128)
  for b in range(2):
    sel = P['qsel'][b * 65:(b + 1) * 65] - b * 129
    assert len(set(sel.tolist())) == 65 and set(A.edges(129)) <= set(sel.tolist()) and (np.diff(sel) < 0).any()


@pytest.mark.parametrize('case,DH', ALL)
def test_inputs_are_as_described(case, DH):
  """Edge keys are live and score about +3 above an ordinary key; ordinary keys are masked here and there; the values are
  bf16; the packed case's positions are scattered."""
  P = A.problem(case, DH)
  d, qkv = P['d'], P['qkv'].double().numpy()
  gaps = []
  for b in range(P['B']):
    o, n = int(P['cu'][b]), P['lens'][b]
    e = np.array(A.edges(n))
    assert (P['bias'][o + e] == 0).all()
    s = A._heads(qkv[o:o + n, :d], A.H) @ A._heads(qkv[o:o + n, d:2 * d], A.H).transpose(0, 2, 1) * P['scale']
    rest = np.setdiff1d(np.arange(n), e)
    if len(rest) > 8:
      gaps.append(s[:, :, e].mean() - s[:, :, rest].mean())
  if gaps:
    assert 2.0 < np.mean(gaps) < 4.0, gaps
  if P['S'] > 16:
    assert (P['bias'] == A.MASKED).any()
  if P['row_index'] is not None:
    assert (np.diff(P['row_index'][:P['lens'][0]]) > 1).any()


@pytest.mark.parametrize('case,DH', [('dense-S17', 128), ('dense-S65-p0.1', 64), ('varlen-S193-p0.1', 128), ('packed-S130-p0.1', 64),
                                     ('rows-S129-nq65', 128)])
def test_reference_is_the_autograd_gradient(case, DH):
  """dQ, dK, dV written out in attention_ref against autograd of sum(ctx dctx) through engine_paths_ref.attention_rows (one
  call per sample: its query count is per call); A v against its ctx."""
  ref = A.reference(case, DH)
  P = ref['P']
  x = P['qkv'].double().requires_grad_(True)
  for b, s in enumerate(ref['samples']):
    o, n, ql = s['o'], s['n'], s['inp'][6]
    ri = None if P['row_index'] is None else P['row_index'] - b * P['S']
    ctx, _ = R.attention_rows(x, P['bias'], 1, P['S'], A.H, P['scale'], o + ql, len(ql), cu=[o, o + n],
                              keep=None if P['keep'] is None else P['keep'][b:b + 1], drop_scale=P['drop_scale'], row_index=ri)
    (ctx * torch.from_numpy(A._rows(s['inp'][3]))).sum().backward()
    np.testing.assert_allclose(A._rows(s['r']['ctx_av']), ctx.detach().numpy(), rtol=1e-10, atol=1e-12)
  g, d = x.grad.numpy(), P['d']
  dq = np.zeros((P['rows'], d))
  qrows = np.concatenate([s['o'] + s['inp'][6] for s in ref['samples']])
  dq[qrows] = ref['ref']['dQ']
  np.testing.assert_allclose(dq, g[:, :d], rtol=1e-9, atol=1e-11)
  np.testing.assert_allclose(ref['ref']['dK'], g[:, d:2 * d], rtol=1e-9, atol=1e-11)
  np.testing.assert_allclose(ref['ref']['dV'], g[:, 2 * d:], rtol=1e-9, atol=1e-11)


@pytest.mark.parametrize('case,DH', ALL)
def test_rounding_emulation_lies_inside_the_bound(case, DH):
  """A, ctx, dS and the outputs rounded to bf16 where the kernels round them, delta taken from the rounded ctx, lse evaluated
  in fp32 over 64-key tiles: inside the bound for every output, exactly 0 where the bound is 0."""
  ref = A.reference(case, DH)
  em = A.emulate(ref)
  for name in _outputs(ref['P']):
    A.within('%s DH %d, emulated %s' % (case, DH, name), em[name], ref['ref'][name], ref['bound'][name])


@pytest.mark.parametrize('case,DH', ALL)
def test_every_edge_mutant_lies_outside_the_bound(case, DH):
  """Every edge position e of every sample: without key e at least 5 % of ctx and 1 % of dQ move by more than 2 x the bound
  and EVERY lse entry by more than 10 x its bound; without query e at least 5 % of dV and 1 % of dK do, counted over the
  live keys.  A sample of one row has no mutant: nothing is left of it without its only key, and its dS is 0."""
  ref = A.reference(case, DH)
  P = ref['P']
  low = dict(dict.fromkeys(SHARE, 1.0), lse=np.inf)  # the smallest share / lse move over the mutants of this case
  for b, s in enumerate(ref['samples']):
    if s['n'] == 1:
      continue
    live = s['inp'][4] == 0
    for e in A.edges(s['n']):
      for kind in ('key',) if P['nq'] else ('key', 'query'):
        mut = A.mutant(ref, b, e, kind)
        for name, got in mut.items():
          moved = np.abs(got - A._flat(name, s['r'][name])) / np.maximum(A._flat(name, s['bound'][name]), 1e-300)
          if name == 'lse':
            low['lse'] = min(low['lse'], float(moved.min()))
            assert moved.min() > LSE_MOVES, 'sample %d without key %d: an lse entry moves by %.3g bounds only' % (b, e, moved.min())
            continue
          if name in ('dK', 'dV'):
            moved = moved[live]
          share = float((moved > 2.0).mean())
          low[name] = min(low[name], share)
          assert share >= SHARE[name], 'sample %d without %s %d: only %.3f of %s moves by more than 2 x the bound' % (b, kind, e, share, name)
  print('%s DH %d: ' % (case, DH) + ', '.join('%s %.3g' % kv for kv in low.items()))


def test_the_old_tolerance_does_not_see_a_lost_key():
  """Why this harness exists.  Inputs of the existing tests' kind (plain unit-variance rows: amp2 = 0, dgain = 1), S = 193:
  ctx without the LAST key, or any other edge key, moves by 5e-3 to 7e-3 on average; more than 90 % of its elements (93 to
  97 %) lie inside 2e-2 + 2e-2 |want|, the tolerance of test_attention_fwd_bwd_dense, and for more than a third of the
  queries (36 to 68 %) the whole ctx row does: a key lost to such a query alone, or read as garbage of ordinary size, passes
  the old tolerance.  (Not every element lies inside: a key lost to ALL queries of a sample would fail the old test in
  the few per cent of elements where it carries much of the softmax.)  The bound of this harness sees the loss in far more
  than 5 % of the elements and in more queries' rows than the old tolerance -- on these quiet inputs; the loud edge rows
  of attention_ref.problem are what makes it see every edge key from every query (the lse condition above)."""
  for DH in A.DHS:
    ref = A.reference('dense-S193', DH, 0.0, 1.0)
    for b, s in enumerate(ref['samples']):
      want, bound = A._rows(s['r']['ctx']), A._rows(s['bound']['ctx'])
      for e in A.edges(193):
        moved = np.abs(A.mutant(ref, b, e, 'key')['ctx'] - want)
        inside = moved <= 2e-2 + 2e-2 * np.abs(want)
        assert moved.mean() < 1e-2 and inside.mean() > 0.9 and inside.all(1).mean() > 1.0 / 3.0, (DH, b, e)
        seen = moved > 2.0 * bound
        assert seen.mean() >= 0.05 and seen.any(1).mean() > (~inside).any(1).mean(), (DH, b, e)
