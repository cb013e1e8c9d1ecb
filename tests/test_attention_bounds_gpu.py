"""The attention kernels (mmt_amd/csrc/attention.hip) against the fp64 reference and the DERIVED elementwise bound of
tests/attention_ref.py, at the lengths where their tiling can go wrong: one key, lengths around every 64-key tile boundary
(the 4-wave forward up to 64 queries, the 8-wave one from 65), three, four and five key tiles (the in-loop prefetch, its
first stage reuse), full and ragged last tiles, with and without dropout, packed samples (cu_seqlens, row_index), the
scheduled backward and the rows-only forward.  tests/test_attention_ref_cpu.py shows, for every case here, that correct
arithmetic lies inside the bound and that one lost tile-edge key or query lies outside it.

Every case: lse, ctx, dQ, dK, dV elementwise within the bound (exactly 0 where reference and bound are 0), and the rows past
the live ones of ctx, lse, dqkv and delta still hold the sentinel they were filled with.  Input rows past the live ones are
NaN: nothing may read them.  Each case prints its largest error / bound per output."""
import numpy as np
import pytest
import torch

from tests import attention_ref as A

pytestmark = pytest.mark.gpu

NAN = float('nan')
SENT = 7.0
PAD = 3  # rows allocated past the live ones
WORST = {}


@pytest.fixture(scope='module', autouse=True)
def _report():
  yield
  print('\nlargest error / bound over all cases: ' + ', '.join('%s %.3f' % (n, WORST[n]) for n in A.OUTPUTS if n in WORST))


def _dev():
  return torch.device('cuda:0')


def _padded(t, fill, dtype):
  out = torch.full((t.shape[0] + PAD,) + tuple(t.shape[1:]), fill, dtype=dtype)
  out[:t.shape[0]] = t.to(dtype)
  return out.to(_dev())


def _i32(x):
  return None if x is None else torch.as_tensor(np.asarray(x), dtype=torch.int32).to(_dev())


def _run(case, DH, scheduled=False):
  """-> (reference, {output: what the kernels wrote for the live rows}); asserts the sentinels."""
  from mmt_amd import _lib, ops
  L, p = _lib.lib(), ops._p
  ref = A.reference(case, DH)
  P = ref['P']
  B, S, H, d, rows, nq = P['B'], P['S'], P['H'], P['d'], P['rows'], P['nq']
  nqr = B * nq if nq else rows  # rows of ctx / lse / dctx
  qkv, bias, dctx = _padded(P['qkv'], NAN, torch.bfloat16), _padded(P['bias'], NAN, torch.float32), _padded(P['dctx'], NAN, torch.bfloat16)
  ctx = torch.full((nqr + PAD, d), SENT, device=_dev(), dtype=torch.bfloat16)
  lse = torch.full((nqr + PAD, H), SENT, device=_dev())
  cu = _i32(P['cu']) if P['varlen'] else None
  ri = None if P['row_index'] is None else _i32(np.concatenate([P['row_index'], np.zeros(PAD, dtype=np.int64)]))
  drop = (A.SITE_KEY, P['thr'], P['drop_scale'], None, p(ri), ops._stream())
  qsel = _i32(P['qsel'])
  if nq:
    _lib.check(L.mmt_attn_fwd_rows(p(qkv), p(cu), p(bias), p(qsel), nq, p(ctx), p(lse), B, S, H, d, P['scale'], *drop),
               'mmt_attn_fwd_rows')
  else:
    _lib.check(L.mmt_attn_fwd(p(qkv), p(cu), p(bias), p(ctx), p(lse), B, S, H, d, P['scale'], *drop), 'mmt_attn_fwd')
  torch.cuda.synchronize()
  assert bool((ctx[nqr:] == SENT).all()) and bool((lse[nqr:] == SENT).all()), 'ctx / lse were written past the live rows'
  got = dict(lse=lse[:nqr].double().cpu().numpy(), ctx=ctx[:nqr].double().cpu().numpy())
  if nq:
    return ref, got
  if P['thr'] == 0:
    for s in ref['samples']:
      if s['n'] == 1:  # a softmax over one key: ctx IS the bf16 v
        assert torch.equal(ctx[s['o']], qkv[s['o'], 2 * d:]), 'ctx of a one-key sample is not its v'
  dqkv = torch.full((rows + PAD, 3 * d), SENT, device=_dev(), dtype=torch.bfloat16)
  delta = torch.full((rows + PAD, d // 64), SENT, device=_dev())
  head = (p(qkv), p(cu), p(bias), p(ctx), p(lse), p(dctx), p(dqkv), p(delta))
  if scheduled:
    work = torch.empty(L.mmt_attn_schedule_words(B, S, H), device=_dev(), dtype=torch.int32)
    _lib.check(L.mmt_attn_schedule(p(cu), B, S, H, p(work), ops._stream()), 'mmt_attn_schedule')
    _lib.check(L.mmt_attn_bwd_ex(*head, 0, B, S, H, d, P['scale'], *drop[:5], p(work), ops._stream()), 'mmt_attn_bwd_ex')
  else:
    _lib.check(L.mmt_attn_bwd(*head, B, S, H, d, P['scale'], *drop), 'mmt_attn_bwd')
  torch.cuda.synchronize()
  assert bool((dqkv[rows:] == SENT).all()) and bool((delta[rows:] == SENT).all()), 'dqkv / delta were written past the live rows'
  g = dqkv[:rows].double().cpu().numpy()
  got.update(dQ=g[:, :d], dK=g[:, d:2 * d], dV=g[:, 2 * d:])
  return ref, got


def _check(case, DH, scheduled=False):
  ref, got = _run(case, DH, scheduled)
  wrong = []
  for name, t in got.items():
    used, msg = A.judge('%s%s DH %d, %s' % (case, ' scheduled' if scheduled else '', DH, name), t, ref['ref'][name], ref['bound'][name])
    WORST[name] = max(WORST.get(name, 0.0), used)
    if msg:
      wrong.append(msg)
  assert not wrong, '\n'.join(wrong)


@pytest.mark.parametrize('DH', A.DHS)
@pytest.mark.parametrize('case', list(A.CASES))
def test_attention_within_the_derived_bound(case, DH):
  """Dense at p = 0 and 0.1, cu_seqlens (lengths 1 / 64 / 129 / 193 and 63 / 65 / 128) at p = 0 and 0.1, packed rows with a
  row_index (the mask is keyed on the ORIGINAL positions), and mmt_attn_fwd_rows with 64 and 65 queries per sample (the
  4-wave and the 8-wave forward; the edge rows are among the queries)."""
  _check(case, DH)


@pytest.mark.parametrize('DH', A.DHS)
def test_scheduled_backward_within_the_derived_bound(DH):
  """mmt_attn_bwd_ex with the work list of mmt_attn_schedule (B H = 8, lengths 1 / 64 / 129 / 193, p = 0.1): against the
  same bound as the unscheduled launch, not against that launch."""
  _check('varlen-S193-p0.1', DH, scheduled=True)
