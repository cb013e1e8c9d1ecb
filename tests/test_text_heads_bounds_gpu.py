"""Text heads through the C ABI (mmt_text_heads_fwd / mmt_text_heads_bwd), on both kernel paths -- texthead2.hip for N <= 32 rows
with d, K multiples of 32 up to 1024, texthead.hip for everything else -- against the fp64 stage references and bounds of
tests/text_heads_ref.py.  Every stage is fed with the device's own previous-stage values, read back from the workspace.  Every
case also checks: the running statistics, that ws / every output / every gradient is written completely and nothing beside it
(NaN sentinels, guard regions, ws allocated at exactly mmt_text_heads_workspace_floats), and that a second run on fresh buffers
gives the same bits.  Then the argument forms of mmt_amd/model.py (separate text_moe, null dtext / text_weights / g_*), and
the refusals.  Every test prints its worst error-to-bound ratio per stage."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import dropout_ref as D
from tests import text_heads_ref as T

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
SENT = 0x7fc0beef   # a NaN that no arithmetic produces
GUARD = 64          # floats in front of and behind every buffer the kernels write (256 bytes: keeps the payload aligned)
ERR_ARG = -1


class Guarded:
  """n floats between two guard regions, all prefilled with the sentinel."""

  def __init__(self, n):
    self.n = int(n)
    self.raw = torch.full((self.n + 2 * GUARD,), SENT, dtype=torch.int32, device=DEV)

  @property
  def ptr(self):
    return self.raw.data_ptr() + 4 * GUARD

  def bits(self):
    return self.raw[GUARD:GUARD + self.n].cpu().numpy().copy()

  def f32(self):
    return self.bits().view(np.float32)

  def guards_intact(self):
    return bool((self.raw[:GUARD] == SENT).all()) and bool((self.raw[GUARD + self.n:] == SENT).all())

  def untouched(self):
    return bool((self.raw == SENT).all())


def _dev(a):
  return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class Heads:
  """One set of device buffers for a case and an argument form, and the two calls."""

  def __init__(self, c, fm, nbt=False):
    from mmt_amd import _lib
    self.L, self.c, self.fm = _lib.lib(), c, fm
    N, M, d, K = c['N'], c['M'], c['d'], c['K']
    self.fast = bool(self.L.mmt_text_heads_fast(N, M, d, K))
    self.inp = {k: _dev(c[k]) for k in ('text', 'text_moe', 'W1', 'b1', 'W2', 'b2', 'gamma', 'beta', 'moe_w', 'moe_b', 'de', 'dtw')}
    self.rm, self.rv = _dev(c['rm']), _dev(c['rv'])
    self.h = _lib.MmtTextHeads()
    self.G = {}
    sizes = dict(w1=d * K, b1=d, w2=d * d, b2=d, bn_gamma=d, bn_beta=d, moe_w=K, moe_b=1)
    src = dict(w1='W1', b1='b1', w2='W2', b2='b2', bn_gamma='gamma', bn_beta='beta', moe_w='moe_w', moe_b='moe_b')
    for m in range(min(M, 16)):
      for name in T.PARAMS:
        bn, moe = name.startswith('bn_'), name.startswith('moe_')
        if (bn and not c['use_bn']) or (moe and not fm['moe']):
          continue
        getattr(self.h, name)[m] = self.inp[src[name]][m].data_ptr()
        if T.wants(fm, name, m):
          self.G[name, m] = Guarded(sizes[name])
          getattr(self.h, 'g_' + name)[m] = self.G[name, m].ptr
      self.h.running_mean[m], self.h.running_var[m] = self.rm[m].data_ptr(), self.rv[m].data_ptr()
    self.ws_floats = int(self.L.mmt_text_heads_workspace_floats(N, M, d))
    self.ws = Guarded(self.ws_floats)
    self.e = Guarded(N * M * d)
    self.tw = Guarded(N * M) if fm['moe'] else None
    self.dtext = Guarded(N * K) if fm['dtext'] else None
    self.dmoe = Guarded(N * K) if (fm['dtext_moe'] and fm['moe']) else None
    self.o = _lib.MmtTextHeadsOpts()
    self.seed = torch.tensor([c['seed_fwd']], dtype=torch.int32, device=DEV)
    self.key = torch.zeros(1, dtype=torch.int32, device=DEV)
    self.nbt = torch.full((M,), 5, dtype=torch.long, device=DEV) if nbt else None
    if fm['drop_p'] > 0:
      from mmt_amd import ops
      self.o.moe_drop_key = c['drop_key']
      self.o.moe_drop_thr16, self.o.moe_drop_scale = ops.dropout_params(fm['drop_p'])
      self.o.seed_dev, self.o.key_dev = self.seed.data_ptr(), self.key.data_ptr()
    if nbt:
      self.o.num_batches_tracked = self.nbt.data_ptr()

  def _p(self, g):
    return None if g is None else ctypes.c_void_p(g.ptr)

  def fwd(self, C=None, text_weights=True):
    from mmt_amd import ops
    c = self.c
    rc = self.L.mmt_text_heads_fwd(ctypes.byref(self.h), ops._p(self.inp['text']),
                                   ops._p(self.inp['text_moe']) if self.fm['text_moe'] else None, c['N'], C or c['C'], c['M'],
                                   c['d'], c['K'], c['use_bn'], c['training'], self._p(self.ws), self._p(self.e),
                                   self._p(self.tw) if text_weights else None, ctypes.byref(self.o), ops._stream())
    torch.cuda.synchronize()
    return rc

  def bwd(self, C=None, w1_all=True):
    from mmt_amd import ops
    c, moe = self.c, self.fm['moe']
    rc = self.L.mmt_text_heads_bwd(ctypes.byref(self.h), ops._p(self.inp['text']),
                                   ops._p(self.inp['text_moe']) if self.fm['text_moe'] else None,
                                   ops._p(self.inp['W1']) if w1_all else None, c['N'], C or c['C'], c['M'], c['d'], c['K'],
                                   c['use_bn'], c['training'], self._p(self.ws), ops._p(self.inp['de']),
                                   self._p(self.tw) if moe else None, ops._p(self.inp['dtw']) if moe else None,
                                   self._p(self.dtext), self._p(self.dmoe), ctypes.byref(self.o), ops._stream())
    torch.cuda.synchronize()
    return rc

  def ws_regions(self):
    c = self.c
    nmd, md = c['N'] * c['M'] * c['d'], c['M'] * c['d']
    return dict(y=(0, nmd), x1=(nmd, nmd), mean=(2 * nmd, md), rstd=(2 * nmd + md, md), dy=(2 * nmd + 2 * md, nmd),
                dx1=(3 * nmd + 2 * md, nmd), dlogit=(4 * nmd + 2 * md, c['N'] * c['M']))

  def read_forward(self, b):
    c = self.c
    N, C, M, d = c['N'], c['C'], c['M'], c['d']
    ws, reg = self.ws.f32(), self.ws_regions()
    cut = lambda k, *shape: ws[reg[k][0]:reg[k][0] + reg[k][1]].reshape(*shape).copy()
    b['y'], b['x1'] = cut('y', N, M, d), cut('x1', N, M, d)
    b['mean'], b['rstd'] = (cut('mean', M, d), cut('rstd', M, d)) if c['use_bn'] else (None, None)
    b['e'] = self.e.f32().reshape(N // C, M, C, d)
    if self.tw is not None:
      b['tw'] = self.tw.f32().reshape(N, M)
    b['rm'], b['rv'] = self.rm.cpu().numpy(), self.rv.cpu().numpy()
    return b

  def read_backward(self, b):
    c, fm = self.c, self.fm
    N, M, d, K = c['N'], c['M'], c['d'], c['K']
    ws, reg = self.ws.f32(), self.ws_regions()
    cut = lambda k, *shape: ws[reg[k][0]:reg[k][0] + reg[k][1]].reshape(*shape).copy()
    b['dx1'], b['dy'] = cut('dx1', N, M, d), cut('dy', N, M, d)
    if fm['moe']:
      b['dlogit'] = cut('dlogit', N, M)
    shapes = dict(w1=(d, K), b1=(d,), w2=(d, d), b2=(d,), bn_gamma=(d,), bn_beta=(d,), moe_w=(K,), moe_b=(1,))
    for name in T.PARAMS:
      if (name.startswith('bn_') and not c['use_bn']) or (name.startswith('moe_') and not fm['moe']):
        continue
      b['g_' + name] = [self.G[name, m].f32().reshape(shapes[name]) if (name, m) in self.G else None for m in range(M)]
    if self.dtext is not None:
      b['dtext'] = self.dtext.f32().reshape(N, K)
    if self.dmoe is not None:
      b['dtext_moe'] = self.dmoe.f32().reshape(N, K)
    return b

  def written(self):
    """Every region that the two calls have to write completely (name, int32 bits)."""
    c, fm = self.c, self.fm
    ws, reg = self.ws.bits(), self.ws_regions()
    names = ['y', 'x1', 'dy', 'dx1'] + (['mean', 'rstd'] if c['use_bn'] else []) + (['dlogit'] if fm['moe'] else [])
    out = [('ws.' + k, ws[reg[k][0]:reg[k][0] + reg[k][1]]) for k in names]
    out += [('text_embds', self.e.bits())] + [('g_%s[%d]' % k, g.bits()) for k, g in sorted(self.G.items())]
    for name, g in (('text_weights', self.tw), ('dtext', self.dtext), ('dtext_moe', self.dmoe)):
      if g is not None:
        out.append((name, g.bits()))
    out += [('running_mean', self.rm.cpu().numpy().view(np.int32)), ('running_var', self.rv.cpu().numpy().view(np.int32))]
    return out

  def guarded(self):
    return [self.ws, self.e] + [g for g in (self.tw, self.dtext, self.dmoe) if g is not None] + list(self.G.values())


def _run(c, fm, nbt=False):
  """Both calls on fresh buffers -> (Heads, buffers as numpy)."""
  hd = Heads(c, fm, nbt=nbt)
  assert hd.fwd() == 0
  b = hd.read_forward({})
  if fm['drop_p'] > 0:
    hd.seed.fill_(c['seed_fwd'] + 1)   # the seed has moved on by the time of the backward: the mask comes from *key_dev
  assert hd.bwd() == 0
  return hd, hd.read_backward(b)


def _report(tag, res):
  w = T.worst(res)
  groups = {}
  for name, (ratio, ulps) in w.items():
    g = groups.setdefault(name.split('[')[0], [0.0, float('nan')])
    g[0], g[1] = max(g[0], ratio), np.fmax(g[1], ulps)
  print('%s: worst error / bound  %s' % (tag, '  '.join('%s %.3f' % (k, v[0]) for k, v in groups.items())))
  print('%s: function error measured (ulps per evaluation)  %s' % (
      tag, '  '.join('stage%d:%s %.3f' % (T.FN_STAGES[k], k, v[1]) for k, v in groups.items() if k in T.FN_STAGES)))
  return T.failures(res)


def _complete(hd):
  for name, bits in hd.written():
    assert not (bits == np.int32(SENT)).any(), '%s: %d elements not written' % (name, int((bits == np.int32(SENT)).sum()))
    assert not np.isnan(bits.view(np.float32)).any(), name
  assert all(g.guards_intact() for g in hd.guarded())


def _same_bits(hd1, hd2, only=None):
  w1, w2 = dict(hd1.written()), dict(hd2.written())
  names = [n for n in w1 if n in w2 and (only is None or only(n))]
  assert names and (only is not None or sorted(w1) == sorted(w2))
  for n in names:
    assert np.array_equal(w1[n], w2[n]), n


def _check_case(spec, fast):
  N, C, M, d, K = spec[:5]
  from mmt_amd import _lib
  assert _lib.lib().mmt_text_heads_fast(N, M, d, K) == int(fast)
  c, fm = T.case_of(spec), T.FORMS['a']
  hd, b = _run(c, fm, nbt=fast)
  _complete(hd)
  bad = _report('%s %s' % ('small' if fast else 'general', spec[:7]), T.verify(c, fm, b))
  assert bad == []
  if fast:
    assert hd.nbt.tolist() == [5 + int(c['use_bn'] and c['training'])] * M
  hd2, _ = _run(c, fm, nbt=fast)
  _same_bits(hd, hd2)


@pytest.mark.parametrize('spec', T.SMALL_CASES, ids=lambda s: '-'.join(map(str, s[:7])))
def test_small_path_stage_by_stage(spec):
  _check_case(spec, True)


@pytest.mark.parametrize('spec', T.GENERAL_CASES, ids=lambda s: '-'.join(map(str, s[:7])))
def test_general_path_stage_by_stage(spec):
  _check_case(spec, False)


@functools.lru_cache(maxsize=None)
def _form_run(path, fname):
  c, fm = T.case_of(T.FORM_SHAPES[path]), T.FORMS[fname]
  return (c, fm) + _run(c, fm)


def _is_param_grad(name):
  return name.startswith('g_')


FORM_RUNS = [(p, f) for p in ('small', 'general') for f in T.FORMS if not (p == 'general' and f == 'f')]


@pytest.mark.parametrize('path,fname', FORM_RUNS)
def test_argument_forms(path, fname):
  """(a) text_moe NULL; (b) a separate text_moe with its dtext_moe; (c) a separate text_moe without: the MoE term joins dtext;
  (d) dtext NULL; (e) no MoE work at all; (f) on-the-fly dropout; (g) every g_* NULL; (h) the g_* of one expert NULL."""
  from mmt_amd import _lib
  spec = T.FORM_SHAPES[path]
  assert _lib.lib().mmt_text_heads_fast(spec[0], spec[2], spec[3], spec[4]) == int(path == 'small')
  c, fm, hd, b = _form_run(path, fname)
  _complete(hd)
  assert _report('%s form %s' % (path, fname), T.verify(c, fm, b)) == []
  if fname == 'd_a':   # nothing to write for dtext; every parameter gradient as with it
    _same_bits(_form_run(path, 'a')[2], hd, only=_is_param_grad)
  if fname == 'd_b':
    _same_bits(_form_run(path, 'b')[2], hd, only=lambda n: _is_param_grad(n) or n == 'dtext_moe')
  if fname == 'e':
    lo, n = hd.ws_regions()['dlogit']
    if path == 'general':
      assert (hd.ws.bits()[lo:lo + n] == np.int32(SENT)).all()
  if fname == 'f':
    assert (int(hd.key.item()) & 0xffffffff) == int(D.eff_key(c['drop_key'], c['seed_fwd']))
    assert int(hd.seed.item()) == c['seed_fwd'] + 1
  if fname == 'g':
    assert hd.G == {}
    assert np.array_equal(hd.dtext.bits(), _form_run(path, 'a')[2].dtext.bits())
  if fname == 'h':
    ha = _form_run(path, 'a')[2]
    assert sorted(hd.G) == sorted(k for k in ha.G if k[1] != 1) and len(hd.G) == len(ha.G) - len(T.PARAMS)
    for k, g in hd.G.items():
      assert np.array_equal(g.bits(), ha.G[k].bits()), k
    assert np.array_equal(hd.dtext.bits(), ha.dtext.bits())


@pytest.mark.parametrize('use_bn,training', [(1, 1), (1, 0), (0, 1)])
def test_num_batches_tracked_counts_training_forwards_with_bn(use_bn, training):
  c = T.make_case(2, 1, 2, 32, 32, use_bn, training)
  hd = Heads(c, T.FORMS['a'], nbt=True)
  assert hd.fast
  assert hd.fwd() == 0 and hd.fwd() == 0
  assert hd.nbt.tolist() == [5 + 2 * int(use_bn and training)] * 2


def test_zero_row_is_clamped_not_divided():
  """A text row of zeros with every b1 zero: o = 0, |o| = 0 < 1e-12, so that row of text_embds is exactly zero, and nothing
  anywhere is NaN (forward only, small path)."""
  c, fm = T.make_case(5, 1, 3, 64, 64, 1, 1, zero_row=2), T.FORMS['a']
  hd = Heads(c, fm)
  assert hd.fast and hd.fwd() == 0
  b = hd.read_forward({})
  assert (b['e'][2].view(np.int32) & 0x7fffffff == 0).all()
  for k in ('y', 'x1', 'mean', 'rstd', 'e', 'tw', 'rm', 'rv'):
    assert np.isfinite(b[k]).all(), k
  assert not (hd.e.bits() == np.int32(SENT)).any() and all(g.guards_intact() for g in hd.guarded())
  assert _report('zero row', T.verify(c, fm, b, backward=False)) == []


# ---- refusals: the stated code, and nothing written ---------------------------------------------------------------------------

def _refused(hd, rc):
  assert rc == ERR_ARG
  assert all(g.untouched() for g in hd.guarded())
  assert np.array_equal(hd.rm.cpu().numpy(), hd.c['rm']) and np.array_equal(hd.rv.cpu().numpy(), hd.c['rv'])


SMALL, GENERAL = (4, 2, 2, 32, 32, 1, 1), (4, 2, 2, 36, 40, 1, 1)


@pytest.mark.parametrize('shape', [SMALL, GENERAL])
def test_refuses_rows_not_a_multiple_of_captions(shape):
  hd = Heads(T.make_case(*shape), T.FORMS['a'])
  _refused(hd, hd.fwd(C=3))
  _refused(hd, hd.bwd(C=3))


@pytest.mark.parametrize('d', [34, 1028])
def test_refuses_unsupported_width(d):
  hd = Heads(T.make_case(2, 1, 1, d, 32, 1, 1), T.FORMS['a'])
  assert not hd.fast
  _refused(hd, hd.fwd())
  _refused(hd, hd.bwd())


def test_refuses_more_than_16_experts():
  hd = Heads(T.make_case(2, 1, 17, 32, 32, 1, 1), T.FORMS['a'])
  _refused(hd, hd.fwd())
  _refused(hd, hd.bwd())


@pytest.mark.parametrize('shape', [SMALL, GENERAL])
def test_refuses_text_weights_without_a_moe_weight(shape):
  hd = Heads(T.make_case(*shape), T.FORMS['a'])
  hd.h.moe_w[1] = None
  _refused(hd, hd.fwd())


def test_general_path_refuses_the_small_paths_extras():
  from mmt_amd import _lib
  c = T.make_case(*GENERAL)
  hd = Heads(c, T.FORMS['f'])                  # on-the-fly dropout
  assert not hd.fast
  _refused(hd, hd.fwd())
  _refused(hd, hd.bwd())
  hd = Heads(c, T.FORMS['a'], nbt=True)        # num_batches_tracked
  _refused(hd, hd.fwd())
  assert hd.nbt.tolist() == [5, 5]
  hd = Heads(c, T.FORMS['a'])                  # video_front
  vf = _lib.MmtVideoFront()
  hd.o.video_front = ctypes.addressof(vf)
  _refused(hd, hd.fwd())


def test_small_path_refuses_dropout_gradient_without_its_buffer():
  """On-the-fly dropout, a dtext and no dtext_moe: the masked gradient has nowhere to go."""
  hd = Heads(T.make_case(*SMALL), T.form(drop_p=0.1))
  assert hd.fast and hd.dmoe is None
  _refused(hd, hd.bwd())


def test_small_path_refuses_dtext_without_w1_all():
  hd = Heads(T.make_case(*SMALL), T.FORMS['a'])
  assert hd.fast
  _refused(hd, hd.bwd(w1_all=False))
