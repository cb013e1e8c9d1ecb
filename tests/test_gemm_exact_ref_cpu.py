"""Proves the harness of tests/test_gemm_exact_gpu.py on a machine without a GPU, for every case of that file: the operands meet
the exactness conditions (tests/gemm_exact_ref.py: integers, below 2^24 in fp32, at most 256 where a bf16 is stored), the
expected outputs equal a plain int64 numpy product (the small cases; the two large ones are tied to it through the same
functions), and every mutant -- a K-step dropped, counted twice, replaced by the step before it, or taken from the previous row
tile's rows -- changes at least 90 % of the elements of every affected 128 x 64 output tile.  The 90 % is a condition on the
operands: a seed that misses it is replaced, the share is never lowered.  K-step counts and the ring each is there for: the
docstring of tests/gemm_exact_ref.py.

Part b's shape comes from the device; here it is formed for 256 CUs (8259 x 1024 / 512 x <= 576) and its conditions for other
CU counts as well."""
import numpy as np
import pytest
import torch

from tests import gemm_exact_ref as G

SHARE = 0.90


def _i64(t):
  return t.double().numpy().astype(np.int64)


def _mutants_change(name, a, b, ksteps, kinds=G.MUTATIONS):
  """a [n, K], b [N, K] float32 CPU tensors: every mutant of every K-step changes >= SHARE of every affected 128 x 64 tile.
  Prints and returns the largest share of a tile that a mutant left unchanged."""
  worst = 0.0
  for s in range(ksteps):
    for kind in kinds:
      delta, first = G.mutation_delta(a, b, s, kind)
      if delta is None:
        continue
      share = G.least_changed_share(delta, first)
      worst = max(worst, 1.0 - share)
      assert share >= SHARE, '%s: %s of K-step %d changes only %.1f %% of a tile' % (name, kind, s, 100.0 * share)
  print('%s: a mutant leaves at most %.2f %% of a 128 x 64 tile unchanged' % (name, 100.0 * worst))
  return worst


def _expected_is_the_int64_product(C, keep):
  """Every epilogue's expected output of case C against numpy int64 arithmetic written out here."""
  n, M = C['live'], C['M']
  a, b = _i64(C['a'][:n]), _i64(C['b'])
  acc = a @ (b if C['nn'] else b.T)
  bias, res, aux, src = _i64(C['bias']), _i64(C['res'][:n]), _i64(C['aux'][:n]), _i64(C['dot_src'][:n])
  acc64 = G.product(C)
  assert np.array_equal(_i64(acc64), acc)
  eq = lambda epi, key, want, **kw: np.testing.assert_array_equal(_i64(G.expected(epi, C, acc64, **kw)[key]), want)
  eq('F32', 'out', acc)
  eq('BF16', 'out', acc)
  eq('BIAS_F32', 'out', acc + bias)
  eq('BIAS_BF16', 'out', acc + bias)
  eq('BIAS_GELU', 'out', acc + bias)
  eq('ADD_F32', 'out', acc + res)
  eq('BIAS_DROP_RES', 'out', acc + bias + res)
  eq('BIAS_DROP_RES', 'out', res + np.where(keep[:n], 2 * (acc + bias), 0), keep=torch.from_numpy(keep[:n]))
  eq('BF16', 'dot_out', (acc * src).reshape(n, -1, 64).sum(2), dot=True)
  out = np.where(aux > 0, acc, 0)
  eq('DGELU', 'out', out)
  cs = np.zeros(((M + 127) // 128, acc.shape[1]), dtype=np.int64)
  for r in range(n):
    cs[r // 128] += out[r]
  eq('DGELU', 'colsum', cs)


def test_operands_are_the_issue_s_and_the_poison_is_in_place():
  P = G.operands(G.SWEEP_M, G.SWEEP_N)
  for key, vals in (('a', range(-2, 3)), ('b', (-1, 0, 1)), ('bias', range(-3, 4)), ('res', range(-8, 9)), ('aux', (-16, 16)),
                    ('dot_src', (-1, 0, 1))):
    assert sorted(set(P[key].double().unique().tolist())) == [float(v) for v in vals], key
  assert P['R'] == 512 and P['a'].shape == (512, G.KMAX) and P['b'].shape == (G.SWEEP_N, G.KMAX)
  C = G.take(P, 3, live=G.SWEEP_LIVE)
  assert C['a'].shape == (512, 192) and C['a'].is_contiguous() and torch.equal(C['a'][:263], P['a'][:263, :192])
  assert bool((C['a'][263:] == G.POISON_A).all()) and bool((C['res'][263:] == G.POISON_RES).all()) and bool((C['aux'][263:] == 16).all())
  assert torch.equal(G.take(P, 3, nn=True)['b'], P['b'][:, :192].t()) and bool((P['a'].abs() <= 2).all())  # (the clean ones stay clean)
  thr, scale = 32768, 2.0
  assert (G.DROP_THR16, G.DROP_SCALE) == (int(round(G.DROP_P * 65536.0)), 1.0 / (1.0 - thr / 65536.0)) == (thr, scale)
  keep = G.keep_mask(300, 256)
  assert abs(float(keep.mean()) - 0.5) < 0.01


def test_the_activation_rule_knows_its_values():
  """gelu_table: x Phi(x) at the integers, rounded to bf16; act_errors accepts the reference and its bf16 neighbours in the
  middle, pre itself and 0 past the clamp, and nothing else."""
  ref, ulp = G.gelu_table()
  assert ref[7] == 0.0 and ref[8] == 0.83984375 and ref[9] == 1.953125 and ref[14] == 7.0  # 0.8413, 1.9545, 7 (1 - 1.3e-12)
  assert abs(ref[6] + 0.1587) < 1e-3 and -1e-11 < ref[0] < 0
  pre = torch.arange(-12, 13, dtype=torch.float64)
  want = torch.where(pre >= 8, pre, torch.zeros_like(pre))
  idx = (pre.clamp(-7, 7) + 7).long()
  good = torch.where(pre.abs() < 8, torch.from_numpy(ref)[idx], want)
  clamp, mid = G.act_errors(pre, good)
  assert not clamp.any() and not mid.any()
  clamp, mid = G.act_errors(pre, good + torch.from_numpy(ulp)[idx] * (pre.abs() < 8))
  assert not clamp.any() and not mid.any()
  clamp, mid = G.act_errors(pre, good + 2.0 * torch.from_numpy(ulp)[idx])
  assert bool(clamp[pre.abs() >= 8].all()) and bool(mid[pre.abs() < 8].all())
  lines = G.act_figures(pre, good + 2.0 * torch.from_numpy(ulp)[idx]).split('\n')
  assert len(lines) == 15 and all(line.endswith('off by 2 ulp') for line in lines) and lines[0].startswith('pre -7: act [')


def test_differences_sees_one_element():
  want = torch.arange(12, dtype=torch.float64).reshape(3, 4)
  got = want.to(torch.bfloat16)
  assert G.differences('x', got, want) == '' and G.differences('x', -0.0 * want, 0.0 * want) == ''
  got[2, 1] += 1
  assert G.differences('x', got, want) == 'x: 1 of 12 differ; first at [[2, 1]]: got [10.0] want [9.0]'
  bad = want.clone()
  bad[0, 0] = float('nan')
  assert G.differences('x', bad, want).startswith('x: 1 of 12 differ; first at [[0, 0]]')
  with pytest.raises(AssertionError):
    G.same('x', got, want)
  with pytest.raises(AssertionError):
    G.differences('x', got[:2], want)


@pytest.mark.parametrize('kt', G.KSTEPS)
def test_sweep_and_nn_cases(kt):
  """Part a (every tile shares the operands of its K-step count) and part c (the same product with b as [K, N])."""
  P = G.operands(G.SWEEP_M, G.SWEEP_N)
  keep = G.keep_mask(P['R'], G.SWEEP_N)
  for live, nn in ((None, False), (G.SWEEP_LIVE, False), (100, False), (None, True), (129, True)):
    _expected_is_the_int64_product(G.take(P, kt, live=live, nn=nn), keep)
  C = G.take(P, kt)
  _mutants_change('sweep kt %d' % kt, C['a'][:C['live']].float(), C['b'].float(), kt)


def test_forced_tiles_run_as_documented():
  assert [G.runs_as(24, 1, e) for e in G.ALL_EPIS] == [14] * 8 and [G.runs_as(25, 1, e) for e in G.ALL_EPIS] == [13] * 8
  assert G.runs_as(24, 2, 'BIAS_GELU') == 24 and G.runs_as(25, 2, 'BIAS_GELU') == 13 and G.runs_as(25, 2, 'DGELU') == 13
  assert G.runs_as(25, 2, 'BF16') == 25 and G.runs_as(25, 2, 'BF16', dot=True) is None
  assert G.runs_as(1, 3, 'BF16', dot=True) == 13 and G.runs_as(2, 3, 'BF16') == 2 and G.runs_as(24, 5, 'BF16', dot=True) == 24
  assert G.sweep_id(24, 1) == 'tile24-as-14-kt1' and G.sweep_id(25, 1) == 'tile25-as-13-kt1' and G.sweep_id(25, 9) == 'tile25-kt9'


def test_grouped_cases():
  """Part d: seven items of 1..7 K-steps, each with its own operands and live count."""
  assert len(G.GROUPED_KSTEPS) == len(G.GROUPED_LIVES) == 7 and set(G.GROUPED_LIVES) == {1, 128, 129, 300}
  worst = 0.0
  for i, (kt, live) in enumerate(zip(G.GROUPED_KSTEPS, G.GROUPED_LIVES)):
    C = G.take(G.operands(G.GROUPED_M, G.GROUPED_N, seed=10 + i), kt, live=live)
    acc = G.product(C)
    want = _i64(C['a'][:live]) @ _i64(C['b']).T
    np.testing.assert_array_equal(_i64(G.expected('F32', C, acc)['out']), want)
    np.testing.assert_array_equal(_i64(G.expected('BIAS_F32', C, acc)['out']), want + _i64(C['bias']))
    full = G.take(G.operands(G.GROUPED_M, G.GROUPED_N, seed=10 + i), kt)
    worst = max(worst, _mutants_change('grouped item %d' % i, full['a'][:300].float(), full['b'].float(), kt))
  assert worst <= 1.0 - SHARE


@pytest.mark.parametrize('rows', G.TN_ROWS)
def test_weight_gradient_cases(rows):
  """Part e, gemm_tn: out = a^T b over `rows` rows in units of 64.  The mutants are taken over the FULL units (a ragged unit of
  one row is an outer product: 47 % of it is zero whatever the seed; the rows before it are what the 90 % speaks of)."""
  a, b = G.wgrad_operands(576, G.TN_N, G.TN_K2, 0)
  want, wb = G.wgrad_expected(a, b, rows)
  np.testing.assert_array_equal(_i64(want), _i64(a[:rows]).T @ _i64(b[:rows]))
  np.testing.assert_array_equal(_i64(wb), _i64(a[:rows]).sum(0))
  G.check_exact('tn', want + 5.0, False)
  full = rows // 64
  if full:
    _mutants_change('tn rows %d' % rows, a[:full * 64].float().t().contiguous(), b[:full * 64].float().t().contiguous(), full,
                    kinds=('drop', 'twice', 'stale_step'))


@pytest.mark.parametrize('mpc', [256, 304, 64, 32, 260])
def test_stream_geometry(mpc):
  for tile in (24, 25):
    g = G.stream_geometry(tile, mpc)
    assert g['tiles'] > 2 * g['cus'] and g['cus'] % 8 == 0 and g['M'] == 128 * g['T'] - 61 and g['lives'][2] == 1
    assert g['lives'][1] < g['M']
  if mpc == 256:
    assert (g['M'], G.stream_geometry(24, 256)['N'], G.stream_geometry(25, 256)['N']) == (8259, 1024, 512)
    assert G.stream_geometry(24, 256)['lives'] == (1987, 6083, 1)


@pytest.mark.parametrize('tile', [24, 25])
def test_stream_cases(tile):
  """Part b at 256 CUs: the exactness conditions of every epilogue at every K-step count and live count, through the same
  functions the small cases tie to int64 numpy; the mutants on the full problem."""
  g = G.stream_geometry(tile, 256)
  P = G.operands(g['M'], g['N'], seed=tile)
  keep = torch.from_numpy(G.keep_mask(g['M'], g['N']))
  worst = 0.0
  for kt in G.STREAM_TILES[tile]['ksteps']:
    C = G.take(P, kt)
    acc = G.product(C)
    for epi in G.STREAM_TILES[tile]['epis']:
      G.expected(epi, C, acc, keep=keep if epi == 'BIAS_DROP_RES' else None)
    for live in g['lives']:  # (the live rows' outputs are the first rows of the full problem's; the column sums are not)
      if 'DGELU' in G.STREAM_TILES[tile]['epis']:
        Cl = G.take(P, kt, live=live)
        cs = G.expected('DGELU', Cl, acc[:live])['colsum']
        assert cs.shape == (g['T'], g['N']) and bool((cs[-(-live // 128):] == 0).all())
    worst = max(worst, _mutants_change('stream tile %d kt %d' % (tile, kt), C['a'][:g['M']].float(), C['b'].float(), kt))
  assert worst <= 1.0 - SHARE


def test_wgrad3_cases():
  """Part e, wgrad3.hip: four items of (3072, 1024) over 2176 rows = 192 tiles of 256 x 256; entries are bounded by 2 n (asserted
  in wgrad_expected); one item's reference against int64 numpy at a ragged count, and the mutants of its first full units."""
  assert sum((N // 256) * (K2 // 256) for N, K2 in G.WGRAD3_ITEMS) == 192 and G.WGRAD3_ROWS >= 2048 and G.WGRAD3_ROWS % 64 == 0
  assert max(G.WGRAD3_LIVES) == G.WGRAD3_ROWS and len(set(G.WGRAD3_ITEM_LIVES)) == 4
  a, b = G.wgrad_operands(G.WGRAD3_ROWS, 3072, 1024, 0)
  want, wb = G.wgrad_expected(a, b, 129)
  np.testing.assert_array_equal(_i64(want), _i64(a[:129]).T @ _i64(b[:129]))
  np.testing.assert_array_equal(_i64(wb), _i64(a[:129]).sum(0))
  _mutants_change('wgrad3 item 0', a[:192].float().t().contiguous(), b[:192].float().t().contiguous(), 3,
                  kinds=('drop', 'twice', 'stale_step'))
