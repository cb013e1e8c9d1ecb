"""Host reference of the counter-based dropout masks, written from the comments and formulas of mmt_common.h (mix32,
rng_pair, keep_elem / keep4, eff_key) and attention.hip (attn_rowkey, attn_keymix, attn_keep_mixed) -- not from any kernel's
output.  numpy, uint64 arithmetic masked to 32 bits, so that every wrap-around of the device's 32-bit unsigned arithmetic is
written out here.

A mask is an integer function of (site key, device seed, ORIGINAL element index):

  site                                   element index
  GEMM BIAS_DROP_RES and split-K         orow * N + col
  LayerNorm sites                        orow * d + col
  stand-alone dropout                    the flat element number
  attention probabilities                (b * H + h, query position, key position), see attn_mask

orow = row_index[row] where a row index is given (token packing), else the row itself.
"""
import numpy as np

M32 = np.uint64(0xffffffff)


def _u64(x):
  return np.asarray(x).astype(np.uint64)


def _mul32(x, c):
  """(x * c) mod 2^32 for x < 2^32, c < 2^32 (the 64-bit product wraps at most harmlessly: only the low word is kept)."""
  with np.errstate(over='ignore'):
    return (_u64(x) * np.uint64(c)) & M32


def mix32(x):
  x = _u64(x) & M32
  x = x ^ (x >> np.uint64(16))
  x = _mul32(x, 0x7feb352d)
  x = x ^ (x >> np.uint64(15))
  x = _mul32(x, 0x846ca68b)
  x = x ^ (x >> np.uint64(16))
  return x


def eff_key(key, seed=None):
  """The stream key of a site: the site key itself without a device seed, else a hash of both."""
  key = _u64(key) & M32
  if seed is None:
    return key
  return mix32(key ^ mix32((_u64(seed) + np.uint64(0x632be5ab)) & M32))


def rng_pair(key, pair_idx):
  """One 32-bit hash per PAIR of elements; pair_idx is a 64-bit number, both words enter."""
  pair_idx = _u64(pair_idx)
  hi, lo = pair_idx >> np.uint64(32), pair_idx & M32
  return mix32(mix32((_u64(key) & M32) ^ _mul32(hi, 0x9e3779b9)) ^ lo)


def uniform16_flat(key, idx):
  """The 16-bit uniform of element idx: low half of the pair's hash for an even idx, high half for an odd one."""
  idx = _u64(idx)
  r = rng_pair(key, idx >> np.uint64(1))
  return np.where((idx & np.uint64(1)) != 0, r >> np.uint64(16), r & np.uint64(0xffff))


def keep_flat(key, idx, thr16):
  """bool array: element idx (any shape, values < 2^64) is kept iff its uniform is >= thr16."""
  return uniform16_flat(key, idx) >= np.uint64(thr16)


def keep_rows(key, orow, ncols, thr16):
  """[len(orow), ncols] mask of a row-major site: element index orow * ncols + col."""
  idx = _u64(orow)[:, None] * np.uint64(ncols) + np.arange(ncols, dtype=np.uint64)[None, :]
  return keep_flat(key, idx, thr16)


def attn_uniform16(key, B, H, S):
  """[B, H, S, S] 16-bit uniforms of the attention-probability dropout (query on axis 2, key on axis 3)."""
  S4 = (S + 3) & ~3
  bh = np.arange(B * H, dtype=np.uint64)[:, None]
  q = np.arange(S, dtype=np.uint64)[None, :]
  rowkey = mix32((_u64(key) & M32) ^ _mul32((bh * np.uint64(S4) + q) & M32, 0x9e3779b9))          # [BH, S]
  keymix = mix32((_mul32(np.arange(S, dtype=np.uint64), 0x85ebca6b) + np.uint64(0x1b873593)) & M32)  # [S]
  x24 = (rowkey[:, :, None] ^ keymix[None, None, :]) & np.uint64(0xffffff)
  u = _mul32(x24, 0x9e3779) >> np.uint64(16)
  return u.reshape(B, H, S, S)


def attn_mask(key, B, H, S, thr16):
  return attn_uniform16(key, B, H, S) >= np.uint64(thr16)


def thr16_of(p):
  """round(p * 65536): the keep probability is quantised to 1/65536 (0 = dropout off)."""
  return max(int(round(float(p) * 65536.0)), 0)
