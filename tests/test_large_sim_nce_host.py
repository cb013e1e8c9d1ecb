"""Host-side gating of the row-sharded InfoNCE path (no GPU): the C exports refuse bad arguments before any launch
(largesim.hip: mmt_ls_nce_stats / mmt_ls_nce_grad) and ShardedInfoNceLoss refuses what ShardedSimLoss refuses."""
import ctypes

import pytest
import torch

ERR_ARG, ERR_ALIGN = -1, -2  # include/mmt_hip.h
P = ctypes.c_void_p(0x10000)  # a non-null, 16-byte aligned address that is never dereferenced: every call below fails first


def _stats(L, S=P, ld=64, tw=P, vw=P, vwt=None, b=8, n=64, M=7, r0=0, scale=1.0, rp=P, cp=P):
  return L.mmt_ls_nce_stats(S, ld, tw, vw, vwt, b, n, M, r0, scale, rp, cp, None)


def _grad(L, S=P, ld=64, tw=P, vw=P, vwt=None, rl=P, cl=P, b=8, n=64, M=7, r0=0, scale=1.0, inv_n=1.0 / 64, g16=P, ldg=64, gs=P):
  return L.mmt_ls_nce_grad(S, ld, tw, vw, vwt, rl, cl, b, n, M, r0, scale, inv_n, g16, ldg, gs, None)


def test_nce_exports_reject_bad_arguments_before_any_launch():
  from mmt_amd import _lib
  L = _lib.lib()
  for f in (_stats, _grad):
    for bad in (dict(S=None), dict(tw=None), dict(vw=None), dict(r0=57), dict(r0=-1), dict(M=17), dict(M=0), dict(b=0),
                dict(scale=0.0), dict(scale=-1.0), dict(scale=float('inf')), dict(scale=float('nan'))):
      assert f(L, **bad) == ERR_ARG, (f.__name__, bad)
    for bad in (dict(n=62, ld=62, ldg=62) if f is _grad else dict(n=62, ld=62), dict(ld=66), dict(S=ctypes.c_void_p(0x10004)),
                dict(vwt=ctypes.c_void_p(0x10004))):
      assert f(L, **bad) == ERR_ALIGN, (f.__name__, bad)
  for bad in (dict(rp=None), dict(cp=None)):
    assert _stats(L, **bad) == ERR_ARG, bad
  assert _stats(L, cp=ctypes.c_void_p(0x10004)) == ERR_ALIGN
  for bad in (dict(rl=None), dict(cl=None), dict(g16=None), dict(gs=None), dict(inv_n=0.0), dict(ldg=60)):
    assert _grad(L, **bad) == ERR_ARG, bad
  for bad in (dict(ldg=66), dict(cl=ctypes.c_void_p(0x10004)), dict(g16=ctypes.c_void_p(0x10004))):
    assert _grad(L, **bad) == ERR_ALIGN, bad
  assert L.mmt_ls_nce_col_blocks(0) == ERR_ARG and L.mmt_ls_nce_row_groups(0) == ERR_ARG
  assert L.mmt_ls_nce_col_blocks(4096) == 1 and L.mmt_ls_nce_col_blocks(4100) == 2
  assert L.mmt_ls_nce_row_groups(128) == 1 and L.mmt_ls_nce_row_groups(129) == 2


def test_sharded_infonce_module_refuses_what_the_maxmargin_module_refuses():
  from mmt_amd.large_sim import ShardedInfoNceLoss
  vid, txt, w = torch.zeros(4, 2, 8), torch.zeros(4, 2, 3, 8), torch.full((4, 2), 0.5)
  with pytest.raises(NotImplementedError):  # C = 3 captions per video
    ShardedInfoNceLoss()(vid, txt, w, w)
  with pytest.raises(RuntimeError):         # CPU tensors: no fallback
    ShardedInfoNceLoss()(vid, txt[:, :, :1], w, w)
  for bad in (0.0, -1.0, float('inf'), float('nan')):
    with pytest.raises(ValueError):
      ShardedInfoNceLoss(scale=bad)
