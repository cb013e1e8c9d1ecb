"""Properties of the host dropout reference (tests/dropout_ref.py) that tests/test_epilogue_exact_gpu.py compares the kernels
with bit for bit: the vectorised uint64 arithmetic against plain Python integers, the structure the header documents (two
elements per hash, every coordinate enters the mask), and that the function it defines is usable as a dropout mask at all
(keep rate, no correlation between neighbours).  Runs without a GPU."""
import numpy as np
import pytest

from tests import dropout_ref as D

P = 0.1
THR = D.thr16_of(P)
ATTN_SHAPE = (3, 4, 218)
ATTN_KEYS = (99, 31, 5, 1234)
FLAT_SHAPE = (384, 256)
FLAT_KEYS = (1234, 77)


def _mix32_int(x):
  x &= 0xffffffff
  x ^= x >> 16
  x = x * 0x7feb352d % 2**32
  x ^= x >> 15
  x = x * 0x846ca68b % 2**32
  x ^= x >> 16
  return x


def _keep_flat_int(key, idx, thr16):
  pair = idx >> 1
  hi, lo = pair >> 32, pair & 0xffffffff
  r = _mix32_int(_mix32_int(key ^ (hi * 0x9e3779b9 % 2**32)) ^ lo)
  return ((r >> 16) if idx & 1 else (r & 0xffff)) >= thr16


def _attn_keep_int(key, H, S, b, h, q, k, thr16):
  S4 = (S + 3) & ~3
  rowkey = _mix32_int(key ^ (((b * H + h) * S4 + q) * 0x9e3779b9 % 2**32))
  keymix = _mix32_int((k * 0x85ebca6b + 0x1b873593) % 2**32)
  return ((((rowkey ^ keymix) & 0xffffff) * 0x9e3779 % 2**32) >> 16) >= thr16


def test_vectorised_arithmetic_matches_plain_integers():
  """Every 32-bit wrap-around of the numpy code against Python's unbounded integers: words with the top bit set, indices
  with a live high word, and the largest 64-bit index."""
  words = [0, 1, 0x7fffffff, 0x80000000, 0xffffffff, 0x9e3779b9, 0xdeadbeef, 1234, 0x7e57d0a1]
  assert D.mix32(np.array(words)).tolist() == [_mix32_int(w) for w in words]
  assert D.mix32(np.array([0])).tolist() == [0] and _mix32_int(1) != 1
  for key in (0, 77, 0xffffffff, 0x7e57d0a1):
    for seed in (0, 1, 1234, 0x9cd41a55, 0xffffffff):
      want = _mix32_int(key ^ _mix32_int((seed + 0x632be5ab) % 2**32))
      assert int(D.eff_key(key, seed)) == want
    assert int(D.eff_key(key)) == key
  idx = [0, 1, 2, 3, 510, 511, 2**32 - 1, 2**32, 2**33 - 2, 2**33 + 1, 2**34 + 7, (2**25 + 770) * 512 + 509, 2**40 + 12345,
         2**63 + 5, 2**64 - 1]
  for key in (0, 1234, 0xffffffff):
    for thr in (1, THR, 32768, 65535):
      assert D.keep_flat(key, np.array(idx, dtype=np.uint64), thr).tolist() == [_keep_flat_int(key, i, thr) for i in idx]
  B, H, S = 2, 3, 37
  m = D.attn_mask(0xdeadbeef, B, H, S, 32768)
  assert m.shape == (B, H, S, S)
  for b, h, q, k in [(0, 0, 0, 0), (1, 2, 36, 36), (1, 0, 5, 17), (0, 2, 36, 0), (1, 1, 0, 36)]:
    assert bool(m[b, h, q, k]) == _attn_keep_int(0xdeadbeef, H, S, b, h, q, k, 32768)


def test_threshold_is_the_quantised_probability():
  assert D.thr16_of(0.0) == 0 and D.thr16_of(0.1) == 6554 and D.thr16_of(0.5) == 32768
  u = D.uniform16_flat(5, np.arange(4096, dtype=np.uint64))
  assert int(u.max()) < 65536
  for thr in (1, 6554, 32768):
    assert np.array_equal(D.keep_flat(5, np.arange(4096, dtype=np.uint64), thr), u >= thr)
  assert D.keep_flat(5, np.arange(4096, dtype=np.uint64), 0).all()  # thr16 = 0 keeps everything


def test_elements_2j_and_2j_plus_1_share_one_hash():
  for base in (0, 2**33, 2**40 + 2):
    j = np.arange(2048, dtype=np.uint64) + np.uint64(base // 2)
    r = D.rng_pair(1234, j)
    assert np.array_equal(D.uniform16_flat(1234, 2 * j), r & np.uint64(0xffff))
    assert np.array_equal(D.uniform16_flat(1234, 2 * j + np.uint64(1)), r >> np.uint64(16))
  # ... and a row-major site is nothing but the flat index
  orow = np.array([0, 5, 2**25 + 3], dtype=np.uint64)
  want = np.stack([D.keep_flat(9, r * np.uint64(512) + np.arange(512, dtype=np.uint64), THR) for r in orow])
  assert np.array_equal(D.keep_rows(9, orow, 512, THR), want)


def _differs(a, b):
  """Two independent masks of keep rate 1 - p differ in 2 p (1 - p) = 18 % of their elements; 'different' asks for half of
  that, 'the same function' would give 0."""
  return float(np.mean(a != b)) > P * (1 - P)


def test_every_coordinate_changes_the_mask():
  idx = np.arange(1 << 14, dtype=np.uint64)
  base = D.keep_flat(D.eff_key(1234, 7), idx, THR)
  assert _differs(base, D.keep_flat(D.eff_key(1234, 8), idx, THR))      # seed
  assert _differs(base, D.keep_flat(D.eff_key(1235, 7), idx, THR))      # site key
  assert _differs(base, D.keep_flat(D.eff_key(1234), idx, THR))         # seed or no seed
  rows = D.keep_rows(1234, np.arange(64), 256, THR)
  assert _differs(rows[:-1], rows[1:])                                  # row
  assert _differs(rows, D.keep_rows(1234, np.arange(64) * 3 + 5, 256, THR))  # original row number, not the packed one
  B, H, S = 2, 4, 50
  m = D.attn_mask(99, B, H, S, THR)
  assert _differs(m, D.attn_mask(98, B, H, S, THR))                      # key
  assert _differs(m, D.attn_mask(D.eff_key(99, 3), B, H, S, THR))        # seed
  assert _differs(m[:, :-1], m[:, 1:])                                   # head
  assert _differs(m[:-1], m[1:])                                         # sample
  assert _differs(m[:, :, :-1], m[:, :, 1:])                             # query row
  assert _differs(m[..., :-1], m[..., 1:])                               # key column


def test_the_high_word_of_the_index_is_live():
  """An index above 2^33 (pair index above 2^32) draws another value than the same index with its high word cleared."""
  lo = np.arange(1 << 14, dtype=np.uint64)
  for hi in (2**33, 2**34, 2**34 + 2**33, 2**40):
    assert _differs(D.keep_flat(1234, lo + np.uint64(hi), THR), D.keep_flat(1234, lo, THR))
  assert _differs(D.keep_flat(1234, lo + np.uint64(2**34), THR), D.keep_flat(1234, lo + np.uint64(2**33), THR))
  # the row numbers of the GPU test: orow * 512 passes 2^34
  big = D.keep_rows(1234, np.arange(64) + 2**25, 512, THR)
  assert _differs(big, D.keep_rows(1234, np.arange(64), 512, THR))


def _zscore(mask):
  q = 1.0 - THR / 65536.0
  n = mask.size
  return (float(mask.sum()) - n * q) / np.sqrt(n * q * (1.0 - q))


def _corr(a, b):
  """Normalised correlation of two equally shaped masks around the nominal keep rate."""
  q = 1.0 - THR / 65536.0
  return float(np.mean((a.astype(np.float64) - q) * (b.astype(np.float64) - q)) / (q * (1.0 - q)))


@pytest.mark.parametrize('key', ATTN_KEYS)
def test_attention_mask_rate_and_neighbour_correlation(key):
  """p = 0.1, B, H, S = 3, 4, 218.  Observed on this reference: |z| <= 1.81 for the overall keep rate and |c| <= 0.0086 for
  neighbours along key, query and head, over the four keys.  Asserted: |z| < 4, |c| < 0.02 (a hash that ties neighbours
  together, such as one that drops a coordinate, gives c = 1).  Per-row z-scores are not asserted: over 2616 rows the
  reference's own largest is 4.6."""
  m = D.attn_mask(key, *ATTN_SHAPE, THR)
  assert abs(_zscore(m)) < 4
  assert abs(_corr(m[..., :-1], m[..., 1:])) < 0.02      # along the key
  assert abs(_corr(m[:, :, :-1], m[:, :, 1:])) < 0.02    # along the query
  assert abs(_corr(m[:, :-1], m[:, 1:])) < 0.02          # along the head


@pytest.mark.parametrize('key', FLAT_KEYS)
def test_flat_mask_rate_and_neighbour_correlation(key):
  """p = 0.1, 384 x 256 elements; same bounds as the attention mask, neighbours along column and row."""
  m = D.keep_rows(key, np.arange(FLAT_SHAPE[0]), FLAT_SHAPE[1], THR)
  assert abs(_zscore(m)) < 4
  assert abs(_corr(m[:, :-1], m[:, 1:])) < 0.02
  assert abs(_corr(m[:-1], m[1:])) < 0.02
