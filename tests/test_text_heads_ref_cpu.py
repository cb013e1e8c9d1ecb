"""Keeps tests/text_heads_ref.py honest without a GPU: the chained fp64 stages against torch.autograd in float64, every bound
against a float32 evaluation of its stage (not too tight) and against wrong versions of the stages (not too loose), over the
cases and argument forms that tests/test_text_heads_bounds_gpu.py runs on the device."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import dropout_ref as D
from tests import text_heads_ref as T

ALL_CASES = T.SMALL_CASES + T.GENERAL_CASES
FORM_RUNS = [(path, name) for path in ('small', 'general') for name in T.FORMS if not (path == 'general' and name == 'f')]


def _autograd(c, fm):
  """The same model with torch.autograd in float64 -> (e, tw, grads per expert, dtext, dtext_moe, running stats)."""
  t = lambda k: torch.from_numpy(c[k].astype(np.float64))
  N, C, M, use_bn, training = c['N'], c['C'], c['M'], c['use_bn'], c['training']
  P = {k: t(k).requires_grad_(True) for k in ('W1', 'b1', 'W2', 'b2', 'gamma', 'beta', 'moe_w', 'moe_b')}
  text = t('text').requires_grad_(True)
  x_np, mask = T.moe_input(c, fm)
  if fm['text_moe']:
    moe_in = t('text_moe').requires_grad_(True)
    leaf = moe_in
  elif mask is not None:
    leaf = text.clone().detach().requires_grad_(True)     # the branch's own view of text, to see its gradient alone
    moe_in = leaf * torch.from_numpy(mask)
  else:
    leaf = text.clone().detach().requires_grad_(True)
    moe_in = leaf
  rm, rv = t('rm').clone(), t('rv').clone()
  embs = []
  for m in range(M):
    y = F.linear(text, P['W1'][m], P['b1'][m])
    x1 = F.linear(y, P['W2'][m], P['b2'][m])
    if use_bn:
      if training and N == 1:  # PyTorch refuses one row: batch statistics by hand, variance 0, the project's rule for the update
        z = (x1 - x1.mean(0)) / torch.sqrt(torch.zeros(()) + 1e-5) * P['gamma'][m] + P['beta'][m]
        rm[m], rv[m] = 0.9 * rm[m] + 0.1 * x1.detach().mean(0), 0.9 * rv[m]
      else:
        a, b = rm[m].clone(), rv[m].clone()
        z = F.batch_norm(x1, a, b, P['gamma'][m], P['beta'][m], bool(training), 0.1, 1e-5)
        rm[m], rv[m] = a, b
    else:
      z = x1
    embs.append(F.normalize(F.glu(torch.cat([y, z], -1), -1), dim=-1))
  e = torch.stack(embs, 1).view(N // C, C, M, -1).permute(0, 2, 1, 3)
  loss = (e * t('de')).sum()
  tw = None
  if fm['moe']:
    tw = F.normalize(F.softmax(F.linear(moe_in, P['moe_w'], P['moe_b']), dim=1), p=1, dim=-1)
    loss = loss + (tw * t('dtw')).sum()
  loss.backward()
  g = lambda v: None if v.grad is None else v.grad.numpy()
  return dict(e=e.detach().numpy(), tw=None if tw is None else tw.detach().numpy(), grads={k: g(v) for k, v in P.items()},
              dtext=g(text), dmoe=g(leaf), rm=rm.numpy(), rv=rv.numpy())


@pytest.mark.parametrize('spec,fname', [
    ((6, 2, 3, 8, 12, 1, 1, 0), 'a'),      # BatchNorm, training, C > 1
    ((6, 2, 3, 8, 12, 1, 0, 0), 'b'),      # eval statistics, a separate text_moe with its own gradient
    ((6, 3, 2, 8, 12, 0, 1, 20), 'c'),     # no BatchNorm, separate text_moe whose gradient joins dtext
    ((5, 1, 4, 12, 16, 1, 1, 0), 'f'),     # a host-computed dropout mask
    ((1, 1, 3, 8, 12, 1, 1, 0), 'a'),      # one row with batch statistics
    ((4, 1, 2, 8, 12, 1, 1, 0), 'e'),      # no MoE work
])
def test_chained_stages_match_autograd(spec, fname):
  c, fm = T.case_of(spec), T.FORMS[fname]
  b, a = T.simulate(c, fm), _autograd(c, fm)
  close = lambda x, y, what: np.testing.assert_allclose(x, y, rtol=1e-10, atol=1e-12, err_msg=what)
  close(b['e'], a['e'], 'text_embds')
  close(b['rm'], a['rm'], 'running_mean')
  close(b['rv'], a['rv'], 'running_var')
  names = dict(w1='W1', b1='b1', w2='W2', b2='b2', bn_gamma='gamma', bn_beta='beta', moe_w='moe_w', moe_b='moe_b')
  for k, ak in names.items():
    if 'g_' + k not in b:
      assert a['grads'][ak] is None or not np.any(a['grads'][ak]), k
      continue
    for m in range(c['M']):
      close(np.asarray(b['g_' + k][m]), a['grads'][ak][m], 'g_%s[%d]' % (k, m))
  if fm['moe']:
    close(b['tw'], a['tw'], 'text_weights')
  want = a['dtext']
  if fm['moe'] and fm['dtext_moe']:
    close(b['dtext_moe'], a['dmoe'], 'dtext_moe')
  elif fm['moe']:
    want = want + a['dmoe']
  close(b['dtext'], want, 'dtext')


def test_no_batch_norm_gradient_for_gem():
  c = T.case_of((4, 2, 2, 8, 12, 0, 1, 0))
  b = T.simulate(c, T.FORMS['a'])
  assert 'g_bn_gamma' not in b and 'g_bn_beta' not in b and b['mean'] is None
  assert np.array_equal(b['rm'], c['rm'].astype(np.float64)) and np.array_equal(b['rv'], c['rv'].astype(np.float64))


@pytest.mark.parametrize('spec', ALL_CASES + [T.FORM_SHAPES['small'], T.FORM_SHAPES['general']])
def test_no_small_row_norm_in_the_reference(spec):
  c = T.case_of(spec)
  b = T.simulate(c, T.FORMS['a'])
  p = lambda k: c[k].astype(np.float64)
  r = T.s_embed(b['y'], b['x1'], b['mean'], b['rstd'], p('gamma'), p('beta'), c['use_bn'])
  assert r.min_norm >= 1e-3
  if spec[7]:  # the logits of a row spread over several tens: the subtraction of the maximum matters
    logits = p('text') @ p('moe_w').T + p('moe_b')
    assert np.median(logits.max(1) - logits.min(1)) > 20.0


def _runs():
  for spec in ALL_CASES:
    yield spec, 'a'
  for path, name in FORM_RUNS:
    if name != 'a':
      yield T.FORM_SHAPES[path], name


@pytest.mark.parametrize('spec,fname', list(_runs()))
def test_float32_stages_pass_every_bound(spec, fname):
  """A float32 numpy evaluation of each stage stands in for a kernel: it must sit inside every bound at the committed allowance
  (numpy's own exp, division and square root are correctly rounded, so this says nothing about the allowance's size)."""
  c, fm = T.case_of(spec), T.FORMS[fname]
  res = T.verify(c, fm, T.simulate(c, fm, np.float32))
  assert T.failures(res) == [], {k: v for k, v in T.worst(res).items() if not v[0] <= 1.0}


# where a wrong version shows: the outputs of the stage it sits in
SHOWS_IN = {
    'bn_sum_short': ('mean',), 'contraction_short': ('y', 'g_w2'), 'unbiased_norm': ('rstd',), 'no_eps': ('rstd',),
    'no_proj': ('dx1', 'dy'), 'no_inv_n': ('dx1',), 'bcmd_order': ('e',), 'softmax_short': ('tw',),
    'moe_to_dtext': ('dtext', 'dtext_moe'),
}


@pytest.mark.parametrize('wrong', sorted(SHOWS_IN))
def test_wrong_stage_exceeds_its_bound_on_every_case(wrong):
  """Each wrong version of a stage, evaluated in float64 (no rounding of its own to hide behind), leaves the bound on at least one
  element of EVERY case and form it applies to -- so the allowance has not been inflated past usefulness."""
  applied = 0
  for spec, fname in _runs():
    c, fm = T.case_of(spec), T.FORMS[fname]
    if not T.WRONG[wrong](c, fm):
      continue
    applied += 1
    with np.errstate(all='ignore'):  # (no eps with a zero variance: infinities, which are outside every bound as well)
      bad = T.failures(T.verify(c, fm, T.simulate(c, fm, np.float64, wrong=wrong)))
    assert any(b.split('[')[0] in SHOWS_IN[wrong] for b in bad), (wrong, spec, fname, bad)
  assert applied >= 3


def test_l1_normalise_after_a_softmax_is_the_identity():
  """The one wrong version that no bound can catch: model.py takes the softmax over the experts and then L1-normalises over the
  experts, i.e. divides by a sum that is one.  Recorded here so that the list of wrong versions is complete."""
  assert not any(T.WRONG['no_l1'](T.case_of(s), T.FORMS['a']) for s in ALL_CASES)
  c, fm = T.case_of(T.FORM_SHAPES['small']), T.FORMS['a']
  a, b = T.simulate(c, fm)['tw'], T.simulate(c, fm, wrong='no_l1')['tw']
  assert np.abs(a - b).max() <= 4 * 2.0**-53


def test_right_stages_in_float64_are_inside_every_bound():
  c, fm = T.case_of(T.FORM_SHAPES['general']), T.FORMS['b']
  assert T.failures(T.verify(c, fm, T.simulate(c, fm)), allowance=0.0) == []


def test_host_dropout_mask_is_dropout_refs_keep_at_n_k():
  """Fixed expectation: the MoE input dropout keeps element (n, k) iff dropout_ref keeps the flat index n K + k under
  eff_key(site key, seed), and scales it by 1 / (1 - thr / 65536)."""
  N, K, key, seed = 5, 96, 0x1234, 77
  thr = D.thr16_of(0.1)
  assert thr == 6554
  scale = 1.0 / (1.0 - thr / 65536.0)
  mask = T.moe_mask(key, seed, N, K, thr, scale)
  ek = D.eff_key(key, seed)
  for n in range(N):
    for k in range(K):
      keep = bool(D.keep_flat(ek, np.uint64(n * K + k), thr))
      assert mask[n, k] == (float(np.float32(scale)) if keep else 0.0)
  kept = mask != 0
  assert 0.8 < kept.mean() < 0.97
  assert int(ek) == EXPECTED_KEY and int(kept.sum()) == EXPECTED_KEPT and np.flatnonzero(~kept)[:6].tolist() == EXPECTED_DROPPED


EXPECTED_KEY, EXPECTED_KEPT, EXPECTED_DROPPED = 2742821781, 427, [6, 36, 39, 49, 51, 55]
