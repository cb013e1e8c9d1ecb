"""Exact expected outputs of the GEMM family (gemm.hip, gemm2.hip, gemm3.hip, gemm5.hip, wgrad3.hip) on small-integer bf16
operands, the case lists of tests/test_gemm_exact_gpu.py, and the mutants that show what bit equality can see.  Host only
(numpy and CPU torch; the functions that form expected outputs are plain torch and also run on device tensors).  Its own checks
are tests/test_gemm_exact_ref_cpu.py.

Why integers.  a in {-2..2} and b in {-1, 0, 1} are exact bf16 numbers; every product and every partial sum of a contraction
is an integer far below 2^24, so ANY order of fp32 accumulation gives the same bits, and the fp64 product is the expected
output itself -- no tolerance.  bias in {-3..3}, res in {-8..8} and dot_src in {-1, 0, 1} keep the epilogues' arithmetic on
integers; aux is +16 or -16, where the dGELU table clamps (gelu_lut.h: magnitudes of 8 and more take the last entry, error
none), so dGELU(aux) is exactly 1 or 0.  `check_exact` asserts the two conditions this rests on for every case: |value| <= 256
wherever a bf16 is stored (bf16 holds every integer up to 256), and every fp32 quantity, the sums of magnitudes behind a
column sum or a row dot included, below 2^24.  A lost, doubled or stale K-step, a wrong ring slot, a row that leaks in from
the padding or a column sum in the wrong row moves an integer by at least 1.

Poison.  Rows past the problem's rows (M, or the live count under n_rows_dev) hold finite poison -- a = 32, res = 2^20,
aux = +16 (dGELU = 1: the row counts in full if it leaks into a column sum) -- in the NT / NN forms, and NaN in the weight
gradients, whose contract is that such rows read as zero.

K-step counts and the ring each is there for (a K-step is 64 deep; `first wrap` = the count at which the ring's slot index
returns to 0 inside one tile, so that a second tile starts in a slot other than 0 unless the count is a multiple of the depth):
  1        prologue = tail, no steady state (gemm5.hip refuses it: tiles 24 / 25 run as 14 / 13)
  2        gemm.hip's two-deep ring wraps; gemm3.hip's two buffers are both used; gemm2.hip's tile 14 (two deep) wraps
  3        wrap + 1 of the two-deep rings; first wrap of tile 13's three-deep ring and of the grouped kernel's
  4        first wrap of gemm5.hip's four-deep ring (tile 24) and of tile 18's four-deep ring; wrap + 1 of depth three
  5        first wrap of gemm5.hip's five-deep ring (tile 25); wrap + 1 of depth four; d = 320 on tile 24
  6        second wrap of depth three, wrap + 1 of depth five; tile 18's two groups take three steps each
  7        wrap + 1 of the second wrap of depth three; an odd count for tile 18's alternating groups and gemm3.hip's half-tiles
  8        second wrap of depth four (the only count the shipped hidden size 512 gives)
  9        wrap + 1 of that; d = 576 on tile 24; 9 = 2 x 4 + 1 = 5 + 4: a persistent block's second tile starts in slot 1 (tile
           24) / slot 4 (tile 25), its third in slot 2 / 3
In the persistent stream (part b) a block's tile i starts in ring slot (i KT) mod RING: KT = 2, 3, 5, 6, 7, 9 give tile 24 the
start slots (0, 2, 0), (0, 3, 2), (0, 1, 2), (0, 2, 0), (0, 3, 2), (0, 1, 2) over a block's three tiles, and KT = 2, 3, 4, 5, 6, 7, 9
give tile 25 (five deep) (0, 2, 4), (0, 3, 1), (0, 4, 3), (0, 0, 0), (0, 1, 2), (0, 2, 4), (0, 4, 3).
"""
import functools
import math

import numpy as np
import torch

from tests import dropout_ref as D

BK = 64
ROW_ALIGN = 256          # mmt_amd.ops.ROW_ALIGN: activation buffers are allocated in multiples of it
KMAX = 9 * BK            # operands are generated once at 9 K-steps; a case of KT steps takes the first KT
SENTINEL = 7.0           # outputs are pre-filled with it; it must survive where a kernel may not write
POISON_A, POISON_RES, POISON_AUX = 32.0, 2.0**20, 16.0
DROP_KEY = 0xa5a51234    # dropout site key of the BIAS_DROP_RES cases (top bit set: an unsigned word)
DROP_P, DROP_THR16, DROP_SCALE = 0.5, 32768, 2.0


def pad_rows(n):
  return (n + ROW_ALIGN - 1) // ROW_ALIGN * ROW_ALIGN


def _ints(shape, lo, hi, seed):
  return torch.randint(lo, hi + 1, shape, generator=torch.Generator().manual_seed(seed))


@functools.lru_cache(maxsize=None)
def operands(M, N, seed=0, K=KMAX):
  """Clean operands of an M x N problem over K (fixed seed): a [pad_rows(M), K], b [N, K], aux, dot_src [pad_rows(M), N] bf16;
  bias [N], res [pad_rows(M), N] fp32.  `take` cuts a case out of them and poisons the rows past its live count."""
  R = pad_rows(M)
  s = 1000 * seed
  return dict(M=M, N=N, K=K, R=R,
              a=_ints((R, K), -2, 2, s + 1).to(torch.bfloat16), b=_ints((N, K), -1, 1, s + 2).to(torch.bfloat16),
              bias=_ints((N,), -3, 3, s + 3).float(), res=_ints((R, N), -8, 8, s + 4).float(),
              aux=(_ints((R, N), 0, 1, s + 5) * 32 - 16).to(torch.bfloat16), dot_src=_ints((R, N), -1, 1, s + 6).to(torch.bfloat16))


def take(P, kt, live=None, nn=False):
  """The case of kt K-steps (the first kt 64 columns of a and b, contiguous) with the rows at and past `live` (default M)
  poisoned.  nn: b as [K, N].  Works on CPU and on device tensors; the clean operands are not modified."""
  n, K = P['M'] if live is None else live, kt * BK
  cut = lambda t: t.clone(memory_format=torch.contiguous_format)  # (a copy also where the slice is the whole tensor)
  a = cut(P['a'][:, :K])
  b = cut(P['b'][:, :K].t() if nn else P['b'][:, :K])
  res, aux = P['res'].clone(), P['aux'].clone()
  a[n:], res[n:], aux[n:] = POISON_A, POISON_RES, POISON_AUX
  return dict(P, a=a, b=b, res=res, aux=aux, K=K, kt=kt, live=n, nn=nn)


def product(C):
  """fp64 a b^T over the live rows of a case: exact for these integers in any summation order."""
  b = C['b'].double()
  return C['a'][:C['live']].double() @ (b if C['nn'] else b.t())


# ---- expected outputs ---------------------------------------------------------------------------------------------------

def colsums(out, M):
  """out [n, N]: the live rows of a DGELU output.  -> [ceil(M / 128), N]: per 128-row tile the column sums over its live rows;
  a tile without a live row is 0."""
  T, (n, N) = (M + 127) // 128, out.shape
  full = torch.zeros(T * 128, N, dtype=out.dtype, device=out.device)
  full[:n] = out
  return full.reshape(T, 128, N).sum(1)


def row_dots(out, dot_src):
  """-> [n, N / 64]: sum of out dot_src over each group of 64 columns (MmtEpilogue.dot_out)."""
  n, N = out.shape
  return (out * dot_src).reshape(n, N // 64, 64).sum(2)


def expected(epi, C, acc, keep=None, dot=False):
  """Expected outputs of epilogue `epi` over the live rows of case C, from acc = product(C), in fp64: dict of out (BIAS_GELU: the
  pre-activation; its activation is judged by act_errors) and, by epilogue, dot_out / colsum.  keep: bool [live, N] dropout
  mask, or None for p = 0.  Every entry and every intermediate fp32 quantity is asserted to meet the exactness conditions (check_exact)."""
  n, N = acc.shape
  f = lambda t: t[:n].double() if t.dim() == 2 else t.double()
  bias, res, aux, src = f(C['bias']), f(C['res']), f(C['aux']), f(C['dot_src'])
  e = {}
  if epi in ('F32', 'BF16'):
    e['out'] = acc
    if dot:
      e['dot_out'] = row_dots(acc, src)
      check_exact('dot_out', row_dots(acc.abs(), src.abs()), False)
  elif epi in ('BIAS_F32', 'BIAS_BF16', 'BIAS_GELU'):
    e['out'] = acc + bias
  elif epi == 'ADD_F32':
    e['out'] = acc + res
    check_exact('acc', acc, False)
  elif epi == 'BIAS_DROP_RES':
    y = acc + bias
    check_exact('acc + bias', y * DROP_SCALE, False)
    e['out'] = res + (y if keep is None else torch.where(keep, y * DROP_SCALE, torch.zeros_like(y)))
  elif epi == 'DGELU':
    e['out'] = torch.where(aux > 0, acc, torch.zeros_like(acc))
    e['colsum'] = colsums(e['out'], C['M'])
    check_exact('colsum', colsums(e['out'].abs(), C['M']), False)
  else:
    raise ValueError(epi)
  check_exact(epi, e['out'], epi in ('BF16', 'BIAS_BF16', 'BIAS_GELU', 'DGELU'))
  return e


def check_exact(name, t, stored_bf16):
  """The exactness conditions (module docstring) of one expected quantity: integers, below 2^24, and at most 256 in magnitude
  where a bf16 is stored."""
  m = float(t.abs().max()) if t.numel() else 0.0
  assert bool((t == t.round()).all()), '%s: not integers' % name
  assert m < 2.0**24, '%s: magnitude %g is not exact in fp32' % (name, m)
  assert not stored_bf16 or m <= 256.0, '%s: magnitude %g is not exact in bf16' % (name, m)


@functools.lru_cache(maxsize=None)
def keep_mask(rows, N):
  """bool [rows, N] numpy: the BIAS_DROP_RES mask at p = 0.5 without a row index or a device seed (element orow N + col)."""
  return D.keep_rows(D.eff_key(DROP_KEY), np.arange(rows, dtype=np.int64), N, DROP_THR16)


# ---- the activation of BIAS_GELU on integer pre-activations ----------------------------------------------------------------

def _ulp_bf16(v):
  _, e = np.frexp(np.abs(v))
  return np.ldexp(1.0, np.where(v == 0, -126, np.maximum(e - 1, -126)) - 7)


@functools.lru_cache(maxsize=None)
def gelu_table():
  """(ref, ulp) fp64 numpy [15], indexed by pre + 7 for the integers pre = -7 .. 7: x Phi(x) in fp64 rounded to the nearest
  bf16, and the bf16 spacing at that number."""
  x = np.arange(-7, 8, dtype=np.float64)
  g = np.array([v * 0.5 * math.erfc(-v / math.sqrt(2.0)) for v in x])
  u = _ulp_bf16(g)
  ref = np.rint(g / u) * u
  return ref, _ulp_bf16(ref)


def act_errors(pre, act):
  """pre, act fp64 tensors of one shape (pre integers).  -> (clamp, mid): bool tensors of the elements that break the rule
  `act = pre where pre >= 8, 0 where pre <= -8` and the rule `|act - bf16(x Phi(x))| <= one bf16 ulp where |pre| < 8`."""
  ref, ulp = (torch.from_numpy(t).to(pre.device) for t in gelu_table())
  mid = pre.abs() < 8
  idx = (pre.clamp(-7, 7) + 7).long()
  bad_mid = mid & ~((act - ref[idx]).abs() <= ulp[idx])
  want = torch.where(pre >= 8, pre, torch.zeros_like(pre))
  return ~mid & (act != want), bad_mid


def act_figures(pre, act):
  """One line per integer pre = -7 .. 7 that occurs: the activations the kernel returned for it, the reference, and the largest
  distance between them in bf16 ulps of the reference (the rule allows 1)."""
  ref, ulp = gelu_table()
  lines = []
  for v in range(-7, 8):
    got = act[pre == v].unique().tolist()
    if got:
      lines.append('pre %2d: act %s, reference %.9g, off by %.3g ulp' % (
          v, got, ref[v + 7], max(abs(g - ref[v + 7]) for g in got) / ulp[v + 7]))
  return '\n'.join(lines)


# ---- judging ------------------------------------------------------------------------------------------------------------

def differences(name, got, want):
  """'' if got == want everywhere (as values: -0 is 0), else how many elements differ, the first few indices and values."""
  assert got.shape == want.shape, '%s: shapes %s %s' % (name, tuple(got.shape), tuple(want.shape))
  bad = ~(got.double() == want.double())  # (a NaN in the output differs)
  count = int(bad.sum())
  if not count:
    return ''
  idx = bad.nonzero()[:6]
  return '%s: %d of %d differ; first at %s: got %s want %s' % (
      name, count, bad.numel(), idx.tolist(), got[bad][:6].tolist(), want[bad][:6].tolist())


def same(name, got, want):
  wrong = differences(name, got, want)
  assert not wrong, wrong


# ---- the mutants ----------------------------------------------------------------------------------------------------------

MUTATIONS = ('drop', 'twice', 'stale_step', 'stale_tile')


def mutation_delta(a, b, s, kind, row_tile=128):
  """a [n, K], b [N, K] float CPU tensors (the live rows of a contraction written as a b^T).  -> (delta [n, N], first affected
  row): what the mutant adds to the product when K-step s is dropped, counted twice, replaced by step s - 1 (a stale ring
  slot) or taken from the same step of the previous row tile's A rows (a stale tile in a persistent stream; rows of the first
  tile are not affected).  None where the mutant does not exist (stale_step at s = 0, stale_tile with one row tile)."""
  k = slice(s * BK, (s + 1) * BK)
  a_s, b_s = a[:, k], b[:, k]
  if kind == 'drop':
    return -(a_s @ b_s.t()), 0
  if kind == 'twice':
    return a_s @ b_s.t(), 0
  if kind == 'stale_step':
    if s == 0:
      return None, 0
    p = slice((s - 1) * BK, s * BK)
    return a[:, p] @ b[:, p].t() - a_s @ b_s.t(), 0
  if kind == 'stale_tile':
    if a.shape[0] <= row_tile:
      return None, 0
    d = torch.zeros(a.shape[0], b.shape[0], dtype=a.dtype)
    d[row_tile:] = (a_s[:-row_tile] - a_s[row_tile:]) @ b_s.t()
    return d, row_tile
  raise ValueError(kind)


def least_changed_share(delta, first_row=0, th=128, tw=64):
  """Smallest share of changed (non-zero) elements over the th x tw output tiles from first_row on; a ragged last tile counts
  with the elements it has."""
  n, N = delta.shape
  least = 1.0
  for r in range(first_row, n, th):
    blk = (delta[r:r + th] != 0).float()
    least = min(least, float(blk.reshape(blk.shape[0], N // tw, tw).mean(dim=(0, 2)).min()))
  return least


# ---- the cases ------------------------------------------------------------------------------------------------------------

SWEEP_M, SWEEP_N, SWEEP_LIVE = 300, 256, 263  # (263 live rows of 300: the DGELU column sums' live-row mask, three live tiles)
SWEEP_TILES = (1, 2, 13, 14, 18, 21, 24, 25)
KSTEPS = tuple(range(1, 10))
F32_EPIS = ('F32', 'BIAS_F32', 'ADD_F32', 'BIAS_DROP_RES')
ALL_EPIS = F32_EPIS + ('BF16', 'BIAS_BF16', 'BIAS_GELU', 'DGELU')
TABLE_TILES = (13, 14, 18, 21, 24)  # GELU by table; tiles 1 / 2 evaluate erff (test_epilogue_exact_gpu.py's subject)


def runs_as(tile, kt, epi, dot=False):
  """The kernel a forced tile id documents to run: gemm5.hip needs two K-steps (24 -> 14, 25 -> 13 at K = 64); its 64-wide tile
  has no GELU table and no column sums (25 -> 13 for BIAS_GELU / DGELU: mmt_gemm2_dispatch, tests/test_kernels_gpu.py's
  test_gemm_nt_wide_tiles); tiles 1 / 2 have no row dots (-> 13: select_tile, test_engine_paths_gpu.py's test_gemm_nt_row_dots).
  None: the call is refused with an argument error (row dots on tile 25)."""
  if tile == 25 and dot:
    return None
  if tile == 24 and kt == 1:
    return 14
  if tile == 25 and (kt == 1 or epi in ('BIAS_GELU', 'DGELU')):
    return 13
  if tile in (1, 2) and dot:
    return 13
  return tile


def sweep_id(tile, kt):
  return 'tile%d%s-kt%d' % (tile, '-as-%d' % runs_as(tile, kt, 'F32') if runs_as(tile, kt, 'F32') != tile else '', kt)


STREAM_TILES = {24: dict(N=1024, ksteps=(2, 3, 5, 6, 7, 9), epis=('F32', 'BIAS_DROP_RES', 'BF16', 'BIAS_GELU', 'DGELU')),
                25: dict(N=512, ksteps=(2, 3, 4, 5, 6, 7, 9), epis=('F32', 'BIAS_DROP_RES', 'BF16'))}


def stream_geometry(tile, multi_processor_count):
  """Part b's shape on a device of that many CUs, as launch5 sizes its grid: cus blocks (a multiple of 8), eight column tiles,
  T = 2 cus / 8 + 1 row tiles of which the last holds 67 rows -- more than 2 cus tiles, so some blocks own three.  lives: one
  live count that leaves fewer live tiles than blocks, one between cus and 2 cus live tiles, and one live row."""
  cus = multi_processor_count & ~7 if multi_processor_count > 8 else 8
  assert cus >= 32, 'the three live counts need at least 32 CUs'
  N = STREAM_TILES[tile]['N']
  tiles_n = N // (128 if tile == 24 else 64)
  T = 2 * cus // 8 + 1
  M = 128 * T - 61
  lives = (128 * (cus // 16) - 61, 128 * (3 * cus // 16) - 61, 1)
  g = dict(cus=cus, N=N, tiles_n=tiles_n, T=T, M=M, tiles=T * tiles_n, lives=lives)
  assert tiles_n == 8 and g['tiles'] > 2 * cus
  assert -(-lives[0] // 128) * tiles_n < cus < -(-lives[1] // 128) * tiles_n < 2 * cus
  return g


NN_TILES = (0, 13, 14)
NN_EPIS = ('BF16', 'F32', 'ADD_F32', 'DGELU')

GROUPED_M, GROUPED_N = 300, 128
GROUPED_KSTEPS = (1, 2, 3, 4, 5, 6, 7)
GROUPED_LIVES = (300, 1, 128, 129, 300, 129, 128)  # per-item n_rows_dev

TN_N = TN_K2 = 128
TN_ROWS = tuple(r for u in range(1, 10) for r in (64 * u - 63, 64 * u))
TN_SPLITS = (1, 3, 4)

WGRAD3_ROWS, WGRAD3_ITEMS = 2176, ((3072, 1024),) * 4  # 4 x 48 = 192 tiles of 256 x 256 at 2176 rows: wgrad3.hip's smallest group
WGRAD3_LIVES = (1, 64, 129, 2049, 2176)
WGRAD3_ITEM_LIVES = (2049, 64, 2176, 129)


@functools.lru_cache(maxsize=None)
def wgrad_operands(rows, N, K2, seed):
  """a [rows, N] in {-2..2}, b [rows, K2] in {-1, 0, 1}, bf16: out = a^T b over the live rows, bias gradient = column sums of a."""
  return _ints((rows, N), -2, 2, 5000 + 10 * seed).to(torch.bfloat16), _ints((rows, K2), -1, 1, 5001 + 10 * seed).to(torch.bfloat16)


def wgrad_expected(a, b, n):
  """(a[:n]^T b[:n], column sums of a[:n]) in fp64; |entries| <= 2 n and n are far below 2^24 for every n used here."""
  assert 2 * n < 2**24
  a64, b64 = a[:n].double(), b[:n].double()
  return a64.t() @ b64, a64.sum(0)
