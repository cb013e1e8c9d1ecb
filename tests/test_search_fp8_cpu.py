"""The fp8-stored VideoIndex without a GPU: the reference quantiser the GPU tests compare the stored bits with, the dtype
gate (checked before any tensor is looked at) and the tolerance argument of its contract.  With f = fold_fp32(G, gw)[g]
an fp8 index keeps, per item,
    scale[g] = 2^e, the smallest power of two with max_k |f[k]| / 2^e <= 448 (e in -120 .. 120; an all-zero row: 1),
    stored[g] = e4m3fn_rne(f / scale[g]),
and the score is defined on the stored value,
    score(q, g) = fl(fl(acc * scale[g]) / den),  acc = <fold_fp32(Q, qw)[q], dequant(stored[g])>,  den = sum_m qw gw (0 -> 1e-5),
with acc on the bf16 matrix cores: hi = bf16(qf), lo = bf16(qf - hi), fp32 accumulation.  An emulation of exactly that
stays within the 1e-5 the fp32 and bf16 searches are tested to, and within
    (2^-4 <|qf|, |f|> + 2^-10 scale[g] sum_k |qf[k]|) / |den| + 1e-5
of the float32 index's score."""
import ctypes
import os
import re

import pytest
import torch

from tests.test_search_bf16_cpu import sweep_data

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP8 = torch.float8_e4m3fn
SWEEP = [(1, 1, 1, 16, 1), (2, 7, 7, 16, 10), (63, 7, 16, 512, 128), (257, 4095, 7, 16, 10), (63, 4097, 1, 512, 128),
         (257, 4097, 16, 16, 1), (65, 300, 3, 48, 10), (257, 70001, 1, 16, 128), (63, 70001, 16, 16, 10),
         (257, 4095, 7, 512, 1)]
NEW_EXPORTS = {'mmt_search_fold_fp8': 8}  # the scans over fp8 storage: tests/test_search_abi_cpu.py


def fp8_quantise_ref(f):
  """f fp32 [n, K] (any device), finite -> (stored float8_e4m3fn [n, K], scale fp32 [n]) by the rule of the module
  docstring: amax = mant * 2^ex with mant in [0.5, 1) (torch.frexp); e = ex - 9 if mant <= 0.875 else ex - 8, since
  448 = 0.875 * 2^9; the division by 2^e is exact and torch's cast is round-to-nearest-even, subnormals included."""
  amax = f.abs().amax(1)
  mant, ex = torch.frexp(amax)
  e = torch.where(mant <= 0.875, ex - 9, ex - 8).clamp(-120, 120)
  e = torch.where(amax == 0, torch.zeros_like(e), e)
  scale = torch.ldexp(torch.ones_like(amax), e)
  return torch.ldexp(f, -e[:, None]).to(FP8), scale


def _finite_codes():
  codes = torch.arange(256, dtype=torch.uint8)
  vals = codes.view(FP8).to(torch.float32)
  keep = torch.isfinite(vals)
  return codes[keep], vals[keep]


def test_every_finite_e4m3_code_is_a_bf16_value():
  codes, vals = _finite_codes()
  assert len(codes) == 254
  assert torch.equal(vals.to(torch.bfloat16).to(torch.float32), vals)
  assert torch.equal(vals.to(FP8).view(torch.uint8), codes)
  assert vals.abs().max().item() == 448.0


def test_the_reference_cast_rounds_to_nearest_even_with_subnormals():
  """The cast behind fp8_quantise_ref against a restatement in exact arithmetic: the nearest of the 127 non-negative
  values, the one with the even code on a tie -- at every midpoint between neighbours, one fp32 ulp either side of it, and
  both signs."""
  codes, vals = _finite_codes()
  pos = vals[:127].double()                   # codes 0x00 .. 0x7E: 0 .. 448, ascending
  assert torch.all(pos[1:] > pos[:-1])
  mid = ((pos[1:] + pos[:-1]) / 2).float()    # exact in fp32
  assert torch.equal(mid.double(), (pos[1:] + pos[:-1]) / 2)
  inf = torch.full_like(mid, float('inf'))
  probe = torch.cat([mid, torch.nextafter(mid, inf), torch.nextafter(mid, -inf), vals[:127]])
  probe = torch.cat([probe, -probe])
  got = probe.to(FP8).view(torch.uint8)
  dist = (probe.abs().double()[:, None] - pos[None, :]).abs()
  best = dist.min(1).values
  want = torch.empty(len(probe), dtype=torch.uint8)
  for i in range(len(probe)):
    near = torch.nonzero(dist[i] == best[i])[:, 0]
    code = int(near[0]) if len(near) == 1 else int(near[near % 2 == 0][0])
    want[i] = code | (0x80 if torch.signbit(probe[i]) else 0)
  assert torch.equal(got, want)


def test_reference_quantiser_scale_rule():
  gen = torch.Generator().manual_seed(0)
  f = torch.randn(2000, 48, generator=gen) * torch.exp(torch.randn(2000, 1, generator=gen) * 8)
  f[7] = 0
  f[8, 0], f[9, 0], f[10, 0], f[11, 0] = 448.0, 448.0 * 2 ** -20, 0.875 * (1 + 2 ** -23) * 2 ** 5, 1e-45
  f[8, 1:], f[9, 1:], f[10, 1:], f[11, 1:] = 1.0, 0.0, 0.0, 0.0
  stored, scale = fp8_quantise_ref(f)
  amax = f.abs().amax(1)
  ratio = amax.double() / scale.double()
  live = amax > 0
  live[11] = False                               # the clamp at 2^-120: below the window
  assert torch.all((ratio[live] > 224) & (ratio[live] <= 448))
  assert scale[7].item() == 1.0 and not stored[7].view(torch.uint8).any()
  assert scale[8].item() == 1.0 and scale[9].item() == 2.0 ** -20 and scale[10].item() == 2.0 ** -3
  assert scale[11].item() == 2.0 ** -120
  assert torch.equal(torch.log2(scale).round().exp2(), scale)                      # powers of two
  deq = stored.to(torch.float32)
  assert torch.isfinite(deq).all()
  # per element: within half a unit in the last place for normal values, half the subnormal spacing below
  err = (deq.double() * scale.double()[:, None] - f.double()).abs()
  assert torch.all(err <= torch.maximum(f.abs().double() * 2.0 ** -4, scale.double()[:, None] * 2.0 ** -10))


def test_dtype_is_validated_before_any_tensor():
  from mmt_amd.search import ShardedVideoIndex, VideoIndex
  with pytest.raises(ValueError, match='bfloat16'):
    VideoIndex(torch.zeros(4, 2, 16), torch.zeros(4, 2), dtype=torch.float8_e5m2)
  with pytest.raises(ValueError, match='float32'):
    VideoIndex.empty(8, 2, 16, 'cpu', dtype=torch.float8_e4m3fnuz)
  # d = 8 is a bf16 width, not an fp8 one: refused by name before the device or the tensors are looked at
  with pytest.raises(ValueError, match='d % 16'):
    VideoIndex.empty(8, 2, 8, 'cpu', dtype=FP8)
  with pytest.raises(ValueError, match='d % 16'):
    VideoIndex(torch.zeros(4, 2, 8), torch.zeros(4, 2), dtype=FP8)
  with pytest.raises(ValueError, match='d % 16'):
    ShardedVideoIndex.empty(8, 2, 24, ['cpu'], dtype=FP8)
  with pytest.raises(ValueError, match='d % 16'):
    ShardedVideoIndex(torch.zeros(4, 2, 8), torch.zeros(4, 2), ['cpu'], dtype=FP8)
  # an accepted dtype and width go on to the device check
  with pytest.raises(ValueError, match='CUDA'):
    VideoIndex.empty(8, 2, 16, 'cpu', dtype=FP8)


@pytest.mark.parametrize('nq,nv,m,d,k', SWEEP)
def test_kernel_arithmetic_emulation_against_fp64_and_the_fp32_index(nq, nv, m, d, k):
  q, qw, g, gw = (torch.from_numpy(x) for x in sweep_data(nq, nv, m, d, k))
  qf = (qw[:, :, None] * q).reshape(nq, -1)                              # fp32 fold
  f = (gw[:, :, None] * g).reshape(nv, -1)
  stored, scale = fp8_quantise_ref(f)
  deq = stored.to(torch.float32)
  assert torch.equal(deq.to(torch.bfloat16).to(torch.float32), deq)      # the widening to bf16 is exact
  hi = qf.to(torch.bfloat16)
  lo = (qf - hi.to(torch.float32)).to(torch.bfloat16)
  acc = hi.to(torch.float32) @ deq.T + lo.to(torch.float32) @ deq.T      # bf16 x bf16 products, fp32 accumulation
  den = qw @ gw.T
  den[den == 0] = 1e-5
  got = ((acc * scale[None, :]) / den).double()
  den64 = qw.double() @ gw.double().T
  den64[den64 == 0] = 1e-5
  want = (qf.double() @ (deq.double() * scale.double()[:, None]).T) / den64
  err = (got - want).abs().max().item()
  print('max |emulation - fp64 of the definition| = %.3g' % err)
  assert err <= 1e-5
  # against the float32 index: only the gallery rounding differs
  full = (qf.double() @ f.double().T) / den64
  bound = (2.0 ** -4 * (qf.abs().double() @ f.abs().double().T) +
           2.0 ** -10 * scale.double()[None, :] * qf.abs().double().sum(1)[:, None]) / den64.abs() + 1e-5
  over = int(((got - full).abs() > bound).sum())
  print('max |fp8 - fp32| / bound = %.3g' % ((got - full).abs() / bound).max().item())
  assert over == 0


def test_new_exports_are_declared_in_the_header_as_the_loader_has_them():
  from mmt_amd import _lib
  src = open(os.path.join(ROOT, 'include', 'mmt_hip.h')).read()
  for name, arity in NEW_EXPORTS.items():
    m = re.search(r'\bint %s\(([^;]*?)\);' % name, src)
    assert m, name + ' is not declared in mmt_hip.h'
    params = [p.strip() for p in m.group(1).replace('\n', ' ').split(',')]
    res, args = _lib.SIGNATURES[name]
    assert res is ctypes.c_int and len(args) == len(params) == arity, name
    for p, a in zip(params, args):
      assert (a is ctypes.c_void_p) == ('*' in p) and (a is ctypes.c_int) == (p.startswith('int ')), (name, p)
  assert 'search_fp8.hip' in src
