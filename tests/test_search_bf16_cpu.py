"""The bf16-stored VideoIndex without a GPU: the dtype gate (checked before any tensor is looked at) and the tolerance
argument of its contract.  The score of a bf16 index is defined on the stored value,
    score(q, g) = <fold_fp32(Q, qw)[q], dequant(bf16(fold_fp32(G, gw)[g]))> / sum_m qw gw     (0 -> 1e-5),
and the kernel realises the fp32 query as hi = bf16(qf), lo = bf16(qf - hi) with fp32 accumulation.  An emulation of
exactly that stays within the 1e-5 the fp32 search is tested to, on the shapes the GPU sweep uses."""
import numpy as np
import pytest
import torch

SWEEP = [(1, 1, 1, 8, 1), (1, 7, 7, 8, 10), (63, 7, 16, 512, 128), (257, 4095, 7, 8, 10), (63, 4097, 1, 512, 128),
         (257, 4097, 16, 8, 1), (1, 70001, 1, 512, 10), (257, 70001, 1, 8, 128), (63, 70001, 16, 8, 10),
         (257, 4095, 7, 512, 1)]


def sweep_data(nq, nv, m, d, k):
  """The data of tests/test_search_gpu.py::test_random_sweep_against_fp64."""
  rng = np.random.default_rng(nq * 7 + nv + m * 13 + d + k)
  q = (rng.random((nq, m, d), dtype=np.float32) * 2 - 1) / np.float32(np.sqrt(d))
  g = (rng.random((nv, m, d), dtype=np.float32) * 2 - 1) / np.float32(np.sqrt(d))
  qw = rng.uniform(0.1, 1, (nq, m)).astype(np.float32)
  gw = rng.uniform(0.1, 1, (nv, m)).astype(np.float32)
  qw[nq // 2] = 0   # denominator 1e-5 on the query side: every score 0
  gw[nv // 3] = 0   # ... and on the gallery side: one column 0
  return q, qw, g, gw


def test_dtype_is_validated_before_any_tensor():
  from mmt_amd.search import VideoIndex
  with pytest.raises(ValueError, match='bfloat16'):
    VideoIndex(torch.zeros(4, 2, 8), torch.zeros(4, 2), dtype=torch.float16)
  with pytest.raises(ValueError, match='bfloat16'):
    VideoIndex.empty(8, 2, 8, 'cpu', dtype=torch.int8)
  with pytest.raises(ValueError, match='float32'):
    VideoIndex.empty(8, 2, 8, 'cpu', dtype=None)


@pytest.mark.parametrize('nq,nv,m,d,k', SWEEP)
def test_split_query_emulation_is_within_1e5_of_the_fp64_definition(nq, nv, m, d, k):
  q, qw, g, gw = (torch.from_numpy(x) for x in sweep_data(nq, nv, m, d, k))
  qf = (qw[:, :, None] * q).reshape(nq, -1)                              # fp32 fold
  stored = (gw[:, :, None] * g).reshape(nv, -1).to(torch.bfloat16)       # rounded once, nearest-even
  deq = stored.to(torch.float32)
  hi = qf.to(torch.bfloat16)
  lo = (qf - hi.to(torch.float32)).to(torch.bfloat16)
  assert torch.equal(hi.to(torch.float32) + (qf - hi.to(torch.float32)), qf)   # the subtraction is exact
  num = hi.to(torch.float32) @ deq.T + lo.to(torch.float32) @ deq.T      # bf16 x bf16 products, fp32 accumulation
  den = qw @ gw.T
  den[den == 0] = 1e-5
  got = (num / den).double()
  den64 = qw.double() @ gw.double().T
  den64[den64 == 0] = 1e-5
  want = (qf.double() @ deq.double().T) / den64
  err = (got - want).abs().max().item()
  print('max |emulation - fp64| = %.3g' % err)
  assert err <= 1e-5
