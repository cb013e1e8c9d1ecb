"""The GEMM family bit for bit: gemm.hip (tiles 1 / 2, gemm_tn), gemm2.hip (13 / 14 / 18, the NN form, the grouped launch),
gemm3.hip (21), gemm5.hip (24 / 25) and wgrad3.hip on the small-integer operands of tests/gemm_exact_ref.py, whose fp64 product
is the expected output exactly -- every comparison here is at ZERO tolerance, but for the one stated rule on the BIAS_GELU
activation of arguments below 8 in magnitude (test_gelu_activation_*).  tests/test_gemm_exact_ref_cpu.py proves the
harness: the exactness conditions, the expected outputs against int64 numpy, and that a lost, doubled or stale K-step changes
at least 90 % of every affected 128 x 64 tile.

K-step counts 1..9 and the ring depth each is there for are listed in the docstring of tests/gemm_exact_ref.py (2 deep: gemm.hip,
tile 14; 3 deep: tile 13, NN, grouped; 4 deep: tiles 18 and 24; 5 deep: tile 25; gemm3.hip: two buffers, half-tiles requested two
K-tiles ahead).  Part b is the part no other test reaches: tiles 24 / 25 are persistent, a block that owns several tiles
carries its ring slot from tile to tile, and with more than 2 x CUs tiles and K-step counts that are no multiple of the depth a
block's second and third tile start in slots other than 0 while each consumer group both sits a tile out and resumes.

Outputs are pre-filled with a sentinel that must survive in the rows at and past M and, under n_rows_dev, at and past
round_up(live, 128).  Input rows past the live ones hold finite poison (NT / NN) or NaN (weight gradients).

What a forced tile id runs (gemm_exact_ref.runs_as, pinned by tests that were here before): tiles 24 / 25 at K = 64 run as 14 /
13; tile 25 has no GELU table and no column sums and runs BIAS_GELU / DGELU as 13; tiles 1 / 2 run row dots as 13.  The one
refusal is row dots on tile 25: an argument error that leaves the outputs untouched.
"""
import functools

import numpy as np
import pytest
import torch

from tests import gemm_exact_ref as G

pytestmark = pytest.mark.gpu

S = G.SENTINEL
NAN = float('nan')


def _dev():
  return torch.device('cuda:0')


def _i32(x):
  return torch.as_tensor(np.asarray(x), dtype=torch.int32).to(_dev())


@functools.lru_cache(maxsize=None)
def _operands(M, N, seed=0):
  """The clean operands on the device (shared by every case of the shape, never modified: G.take copies)."""
  return {k: v.to(_dev()) if torch.is_tensor(v) else v for k, v in G.operands(M, N, seed).items()}


@functools.lru_cache(maxsize=None)
def _keep(rows, N):
  return torch.from_numpy(G.keep_mask(rows, N)).to(_dev())


def _untouched(errors, name, t, first_row):
  bad = t[first_row:] != S
  if bool(bad.any()):
    errors.append('%s: %d elements at or past row %d were written; first at %s' % (
        name, int(bad.sum()), first_row, (bad.nonzero()[:6] + torch.tensor([first_row, 0], device=t.device)).tolist()))


def _run(errors, name, C, acc, epi, tile, packed=False, dot=False, p=0.0, colsum=True, act=None, row_tile=128):
  """One launch of epilogue `epi` on case C (acc = its fp64 product) and every exact comparison it allows; what differs is
  appended to `errors`.  packed: the live count goes in through n_rows_dev.  act: None (pre only), 'clamp' (act where |pre| >=
  8) or 'mid' (the one-ulp rule where |pre| < 8).  row_tile: rows of the kernel's tile (the rows of a live tile past the live
  count may be written)."""
  from mmt_amd import ops
  M, N, R, live, nn = C['M'], C['N'], C['R'], C['live'], C['nn']
  assert packed or live == M
  edge = min(M, -(-live // row_tile) * row_tile)
  f32 = epi in G.F32_EPIS
  out = torch.full((R, N), S, device=_dev(), dtype=torch.float32 if f32 else torch.bfloat16)
  kw, keep = {}, None
  if epi in ('ADD_F32', 'BIAS_DROP_RES'):
    kw['res'] = C['res']
  if epi == 'DGELU':
    kw['aux'] = C['aux']
  if not nn:
    if epi.startswith('BIAS'):
      kw['bias'] = C['bias']
    if epi == 'BIAS_GELU':
      kw['out2'] = torch.full((R, N), S, device=_dev(), dtype=torch.bfloat16)
    if epi == 'BIAS_DROP_RES' and p:
      assert ops.dropout_params(p) == (G.DROP_THR16, G.DROP_SCALE)
      kw.update(drop_key=G.DROP_KEY, drop_p=p)
      keep = _keep(R, N)[:live]
    if epi == 'DGELU' and colsum:
      kw['colsum'] = torch.full(((M + 127) // 128, N), S, device=_dev())
    if dot:
      kw.update(dot_src=C['dot_src'], dot_out=torch.full((R, N // 64), S, device=_dev()))
  nrd = _i32([live]) if packed else None
  (ops.gemm_nn if nn else ops.gemm_nt)(C['a'], C['b'], out, epi, m=M, n_rows_dev=nrd, tile=tile, **kw)
  e = G.expected(epi, C, acc, keep=keep, dot=dot)
  errors.append(G.differences(name, out[:live], e['out']))
  _untouched(errors, name, out, edge)
  if 'colsum' in kw:
    errors.append(G.differences(name + ' colsum', kw['colsum'], e['colsum']))
  if dot:
    errors.append(G.differences(name + ' dot_out', kw['dot_out'][:live], e['dot_out']))
    _untouched(errors, name + ' dot_out', kw['dot_out'], live)
  if epi == 'BIAS_GELU':
    _untouched(errors, name + ' act', kw['out2'], edge)
    if act:
      clamp, mid = G.act_errors(out[:live].double(), kw['out2'][:live].double())
      bad = clamp if act == 'clamp' else mid
      if act == 'mid':
        print('%s\n%s' % (name, G.act_figures(out[:live].double(), kw['out2'][:live].double())))
      if bool(bad.any()):
        errors.append('%s act (%s): %d of %d break the rule; first at %s: pre %s act %s' % (
            name, act, int(bad.sum()), bad.numel(), bad.nonzero()[:6].tolist(), out[:live][bad][:6].tolist(), kw['out2'][:live][bad][:6].tolist()))
  while '' in errors:
    errors.remove('')


def _report(errors):
  assert not errors, '%d findings:\n%s' % (len(errors), '\n'.join(errors))


def _raises_arg_error(fn):
  with pytest.raises(RuntimeError, match=r'failed with code -1$'):
    fn()


# ---- a. K-step sweep ------------------------------------------------------------------------------------------------------

_SWEEP = [(t, kt) for t in G.SWEEP_TILES for kt in G.KSTEPS]


@pytest.mark.parametrize('tile,kt', _SWEEP, ids=[G.sweep_id(t, kt) for t, kt in _SWEEP])
def test_k_step_sweep(tile, kt):
  """300 x 256 (two full row tiles and one of 44 rows; on tile 21 one of 256 and one of 44) over 1..9 K-steps, every epilogue:
  the fp32 family, dropout at p = 0.5 against the documented hash, the bf16 stores, row dots, BIAS_GELU's pre-activation (and
  its activation past the table's clamp), DGELU with column sums over all rows, over 263 live ones, and over 100 (the column
  sums of the row tiles without a live row are 0; tile 21's one live tile is 256 rows)."""
  from mmt_amd import ops
  P = _operands(G.SWEEP_M, G.SWEEP_N)
  C = G.take(P, kt)
  acc = G.product(C)
  name = G.sweep_id(tile, kt) + ' %s'
  errors = []
  for epi in G.ALL_EPIS:
    _run(errors, name % epi, C, acc, epi, tile, act=None if tile in (1, 2) else 'clamp')
  _run(errors, name % 'BIAS_DROP_RES p = 0.5', C, acc, 'BIAS_DROP_RES', tile, p=G.DROP_P)
  if G.runs_as(tile, kt, 'BF16', dot=True) is None:
    out = torch.full((C['R'], C['N']), S, device=_dev(), dtype=torch.bfloat16)
    dots = torch.full((C['R'], C['N'] // 64), S, device=_dev())
    _raises_arg_error(lambda: ops.gemm_nt(C['a'], C['b'], out, 'BF16', m=C['M'], tile=tile, dot_src=C['dot_src'], dot_out=dots))
    torch.cuda.synchronize()
    _untouched(errors, name % 'refused row dots: out', out, 0)
    _untouched(errors, name % 'refused row dots: dot_out', dots, 0)
  else:
    _run(errors, name % 'BF16 + row dots', C, acc, 'BF16', tile, dot=True)
  Cl = G.take(P, kt, live=G.SWEEP_LIVE)
  _run(errors, name % 'DGELU, 263 live rows', Cl, acc[:G.SWEEP_LIVE], 'DGELU', tile, packed=True)
  _run(errors, name % 'DGELU, 100 live rows', G.take(P, kt, live=100), acc[:100], 'DGELU', tile, packed=True, row_tile=256 if tile == 21 else 128)
  _report(errors)


@pytest.mark.parametrize('tile', G.TABLE_TILES + (25,))
def test_gelu_activation_in_the_sweep(tile):
  """BIAS_GELU's activation where |pre| < 8, at every K-step count of the sweep, on the tiles that read the GELU table (25 runs
  it as 13): within one bf16 ulp of the fp64 x Phi(x) rounded to bf16 -- the table entry is the double value rounded to fp32,
  then come one fp32 multiply and one rounding to bf16, and double rounding moves a result to an adjacent bf16 at most.

  gelu_lut (gemm_epi.h) meets it because its table holds the lower tail Phi(-|x|): a negative argument takes x fp32(Phi(-|x|)),
  one table rounding and one multiply.  (With a table of Phi(|x|) and the sign fix 1 - t the table's rounding became an
  absolute error behind the subtraction: pre = -5, -6, -7 came out 8, 203 and 158 ulp off -- -1.4901161e-06, -0, -0 against
  -1.4305115e-06, -5.9080776e-09, -8.9812602e-12 -- which is what this test found and the change of the table fixed.)"""
  P = _operands(G.SWEEP_M, G.SWEEP_N)
  errors = []
  for kt in G.KSTEPS:
    C = G.take(P, kt)
    _run(errors, 'tile %d, %d K-steps: BIAS_GELU' % (tile, kt), C, G.product(C), 'BIAS_GELU', tile, act='mid')
  _report(errors)


# ---- b. the persistent stream across tiles ----------------------------------------------------------------------------------

def _stream(tile):
  g = G.stream_geometry(tile, torch.cuda.get_device_properties(0).multi_processor_count)
  assert g['tiles'] > 2 * g['cus'], g  # some blocks own three tiles: each consumer group both skips a tile and resumes
  return g, _operands(g['M'], g['N'], seed=tile)


_STREAM = [(t, kt) for t in (24, 25) for kt in G.STREAM_TILES[t]['ksteps']]


@pytest.mark.parametrize('tile,kt', _STREAM, ids=['tile%d-kt%d' % c for c in _STREAM])
def test_persistent_stream_across_tiles(tile, kt):
  """gemm5.hip with more than 2 x CUs tiles (on 256 CUs: 8259 x 1024 / 512, 520 tiles): F32, BIAS_DROP_RES at p = 0.5, BF16 and,
  on tile 24, BIAS_GELU's pre-activation and DGELU with column sums -- on all rows, and with n_rows_dev at a count that leaves
  fewer live tiles than blocks, one between CUs and 2 x CUs live tiles, and one live row (column sums of dead tiles are 0)."""
  g, P = _stream(tile)
  full = None
  errors = []
  for live in (None,) + g['lives']:
    C = G.take(P, kt, live=live)
    if full is None:
      full = G.product(C)
    acc = full[:C['live']]
    name = 'tile %d, %d K-steps, %s: ' % (tile, kt, 'all rows' if live is None else '%d live rows' % live)
    for epi in G.STREAM_TILES[tile]['epis']:
      _run(errors, name + epi, C, acc, epi, tile, packed=live is not None, p=G.DROP_P if epi == 'BIAS_DROP_RES' else 0.0, act='clamp')
  _report(errors)


def test_gelu_activation_in_the_persistent_stream():
  """The one-ulp rule of test_gelu_activation_in_the_sweep on tile 24's stream, every K-step count of part b."""
  g, P = _stream(24)
  errors = []
  for kt in G.STREAM_TILES[24]['ksteps']:
    C = G.take(P, kt)
    _run(errors, 'tile 24, %d K-steps: BIAS_GELU' % kt, C, G.product(C), 'BIAS_GELU', 24, act='mid')
  _report(errors)


# ---- c. NN form -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('kt', G.KSTEPS)
@pytest.mark.parametrize('tile', G.NN_TILES)
def test_nn_form(tile, kt):
  """ops.gemm_nn (b as [K, N]) on the sweep's problem: BF16, F32, ADD_F32, DGELU; F32 again with 129 live rows of 300."""
  P = _operands(G.SWEEP_M, G.SWEEP_N)
  C = G.take(P, kt, nn=True)
  acc = G.product(C)
  errors = []
  for epi in G.NN_EPIS:
    _run(errors, 'nn tile %d, %d K-steps: %s' % (tile, kt, epi), C, acc, epi, tile)
  _run(errors, 'nn tile %d, %d K-steps: F32, 129 live rows' % (tile, kt), G.take(P, kt, live=129, nn=True), acc[:129], 'F32', tile, packed=True)
  _report(errors)


# ---- d. grouped NT ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('packed', [False, True])
def test_grouped_nt(packed):
  """ops.gemm_nt_grouped: seven items of 1..7 K-steps in one launch, 300 x 128 each, BIAS_F32 and F32; packed: per-item
  n_rows_dev of 300, 1, 128, 129, 300, 129, 128."""
  from mmt_amd import ops
  M, N = G.GROUPED_M, G.GROUPED_N
  lives = G.GROUPED_LIVES if packed else (M,) * 7
  cases = [G.take(_operands(M, N, seed=10 + i), kt, live=live) for i, (kt, live) in enumerate(zip(G.GROUPED_KSTEPS, lives))]
  errors = []
  for epi in ('BIAS_F32', 'F32'):
    outs = [torch.full((C['R'], N), S, device=_dev()) for C in cases]
    ops.gemm_nt_grouped([(C['a'], C['b'], o, C['bias'] if epi == 'BIAS_F32' else None) for C, o in zip(cases, outs)], m=M, epilogue=epi,
                        n_rows_dev=_i32(lives) if packed else None)
    for i, (C, o) in enumerate(zip(cases, outs)):
      name = 'grouped %s item %d (%d K-steps, %d live rows)' % (epi, i, C['kt'], C['live'])
      errors.append(G.differences(name, o[:C['live']], G.expected(epi, C, G.product(C))['out']))
      _untouched(errors, name, o, min(M, -(-C['live'] // 128) * 128))
  _report([e for e in errors if e])


# ---- e. weight gradients ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('rows', G.TN_ROWS)
def test_gemm_tn(rows):
  """ops.gemm_tn at 128 x 128 over 1..9 units of 64 rows, full and with one row in the last unit; splits 1 / 3 / 4 (more
  slabs than units included); the count as an argument and on the device; accumulation onto an integer.  Rows past the count
  hold NaN."""
  from mmt_amd import ops
  alloc = -(-rows // 64) * 64
  a, b = (t[:alloc].to(_dev()) for t in G.wgrad_operands(576, G.TN_N, G.TN_K2, 0))
  want, _ = G.wgrad_expected(a, b, rows)
  a[rows:], b[rows:] = NAN, NAN
  errors = []
  for splits in G.TN_SPLITS:
    name = 'tn %d rows, %d splits' % (rows, splits)
    errors.append(G.differences(name + ', count on the device', ops.gemm_tn(a, b, rows=alloc, splits=splits, n_rows_dev=_i32([rows])), want))
    errors.append(G.differences(name + ', count as an argument', ops.gemm_tn(a, b, rows=rows, splits=splits), want))
    onto = torch.full((G.TN_N, G.TN_K2), 5.0, device=_dev())
    ops.gemm_tn(a, b, rows=rows, splits=splits, out=onto, accumulate=True)
    errors.append(G.differences(name + ', accumulated onto 5', onto, want + 5.0))
  _report([e for e in errors if e])


@functools.lru_cache(maxsize=None)
def _wgrad3_operands():
  return [tuple(t.to(_dev()) for t in G.wgrad_operands(G.WGRAD3_ROWS, N, K2, q)) for q, (N, K2) in enumerate(G.WGRAD3_ITEMS)]


@pytest.mark.parametrize('live', G.WGRAD3_LIVES + ('per item',))
def test_wgrad3(live):
  """wgrad3.hip through ops.wgrad_grouped: four items of (3072, 1024) over 2176 rows (192 tiles of 256 x 256, the smallest group
  routed there); 1, 64, 129, 2049 and all rows live through n_rows_dev, and one launch with four different counts in
  item_rows_dev.  Rows past the live count hold NaN: the buffer descriptor must make them read as zero.  Weight gradients and
  bias gradients are exact integers."""
  from mmt_amd import ops
  rows = G.WGRAD3_ROWS
  counts = G.WGRAD3_ITEM_LIVES if live == 'per item' else (live,) * 4
  items, wants = [], []
  for q, ((a, b), n) in enumerate(zip(_wgrad3_operands(), counts)):
    wants.append(G.wgrad_expected(a, b, n))
    a, b = a.clone(), b.clone()
    a[n:], b[n:] = NAN, NAN
    items.append((a, b, torch.full((a.shape[1], b.shape[1]), S, device=_dev()), torch.full((a.shape[1],), S, device=_dev()) if q != 2 else None))
  if live == 'per item':
    ops.wgrad_grouped(items, rows, item_rows_dev=_i32(counts))
  else:
    ops.wgrad_grouped(items, rows, n_rows_dev=_i32([live]) if live != rows else None)
  errors = []
  for q, ((a, b, out, bias), (want, wb)) in enumerate(zip(items, wants)):
    errors.append(G.differences('wgrad3 item %d, %d live rows' % (q, counts[q]), out, want))
    if bias is not None:
      errors.append(G.differences('wgrad3 item %d, %d live rows: bias gradient' % (q, counts[q]), bias, wb))
  _report([e for e in errors if e])
