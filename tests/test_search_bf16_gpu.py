"""VideoIndex with a bf16-stored gallery (mmt_search_fold_bf16 / mmt_search_fold_split_bf16 / mmt_search_topk_bf16) and the
chunked build (VideoIndex.empty + add) for both storage dtypes.  The contract: the index stores bf16(gw (.) G), the fp32
fold rounded once to nearest-even, and

    score(q, g) = <fold_fp32(Q, qw)[q], dequant(stored[g])> / sum_m qw[q][m] gw[g][m]          (0 -> 1e-5)

is computed to the fp32 search's own tolerance (1e-5 against fp64 of this definition: the query is not rounded to 8 bits).
Against the float32 index only the gallery rounding differs, bounded by bf16's unit roundoff:
    |score_bf16 - score_fp32| <= 2^-8 * sum_m qw gw <|Q_m|, |G_m|> / sum_m qw gw  (+ 1e-5)."""
import numpy as np
import pytest
import torch

from tests.test_search_bf16_cpu import SWEEP, sweep_data
from tests.test_search_gpu import _assert_topk, _cuda, _golden, _ref_sims

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
BF16 = torch.bfloat16


def _bits(x):
  return x.view(torch.int16 if x.dtype is BF16 else torch.int32)


def _random(nv, nq, m, d, seed):
  gen = torch.Generator(device=DEV).manual_seed(seed)
  g, gw = torch.randn(nv, m, d, device=DEV, generator=gen), torch.rand(nv, m, device=DEV, generator=gen)
  q, qw = torch.randn(nq, m, d, device=DEV, generator=gen), torch.rand(nq, m, device=DEV, generator=gen)
  return g, gw, q, qw


def test_stored_bits_are_the_fp32_fold_cast_once():
  from mmt_amd.search import VideoIndex
  g, gw, _, _ = _random(1000, 1, 3, 40, 1)
  gw[17] = 0  # a zero-weight row: signed zeros
  gw[5, 1] = 1.0  # exact ties between two bf16 neighbours: to the even one, both signs
  g[5, 1, :8] = torch.tensor([1.00390625, 1.01171875, -1.00390625, -1.01171875, 65504.0, 0.0, 1.00390626, 1.0117187], device=DEV)
  idx = VideoIndex(g, gw, dtype=BF16)
  n = idx.num_items
  want = (gw[:, :, None] * g).reshape(n, -1).to(BF16)
  assert idx.folded.dtype is BF16 and idx.folded.shape == (1000, 120)
  assert torch.equal(_bits(idx.folded[:n]), _bits(want))
  assert torch.equal(idx.weights[:n], gw)


@pytest.mark.parametrize('nq,nv,m,d,k', SWEEP)
def test_random_sweep_against_fp64_of_the_definition(nq, nv, m, d, k):
  from mmt_amd.search import VideoIndex
  q, qw, g, gw = sweep_data(nq, nv, m, d, k)
  idx = VideoIndex(_cuda(g), _cuda(gw), dtype=BF16)
  s, i = idx.search(_cuda(q), _cuda(qw), k=k)
  # fp64 of the definition: _ref_sims with the dequantised stored fold as the gallery and gw = 1 inside the numerator
  deq = idx.folded[:nv].to(torch.float32).cpu().numpy().reshape(nv, m, d)
  one = np.ones((nv, m))
  den1 = np.asarray(qw, np.float64) @ one.T
  den1[den1 == 0] = 1e-5
  den = np.asarray(qw, np.float64) @ np.asarray(gw, np.float64).T
  den[den == 0] = 1e-5
  ref = _ref_sims(q, qw, deq, one) * den1 / den
  got = np.take_along_axis(ref, i.cpu().numpy(), 1)
  print('max |score - fp64| on the returned items = %.3g' % np.abs(s.cpu().numpy() - got).max())
  _assert_topk(ref, i.cpu().numpy(), s.cpu().numpy(), k, 1e-5, 1e-5)
  assert np.array_equal(i[nq // 2].cpu().numpy(), np.arange(min(k, nv)))


def _abs_bound(q, qw, g, gw):
  """sum_m qw gw <|Q_m|, |G_m|> / sum_m qw gw in fp64: what one relative gallery rounding of 2^-8 can move a score by."""
  return _ref_sims(np.abs(q), qw, np.abs(g), gw)


@pytest.mark.parametrize('direction,want_rows', [('text_to_video', {1: 26, 3: 5}), ('video_to_text', {1: 12, 3: 4})])
def test_against_the_fp32_index_on_the_golden_embeddings(direction, want_rows):
  """Every returned score is within 2^-8 * bound + 1e-5 of the fp64 full-precision score of its item (k = 1, 3, 10), and
  where the fp32 reference's k-th and (k+1)-th scores are further apart than twice that (the row's largest bound over the
  gallery) the returned index set equals the fp32 index's.  The rows that qualify depend on the fixture and fp64 only:
  26 of 72 and 5 of 72 (text to video), 12 of 24 and 4 of 24 (video to text, the gallery being all 72 caption rows of the
  fixture, padding included) at k = 1 and 3 (at k = 5 the same rule leaves 2 and 0 rows, not run).  The 24-video
  fixture is packed too tightly for k = 10 to say anything about the order, so there only the score bound is checked."""
  from mmt_amd.search import VideoIndex
  _, vid, vw, txt, tw = _golden()
  q, qw, g, gw = (txt, tw, vid, vw) if direction == 'text_to_video' else (vid, vw, txt, tw)
  ref = _ref_sims(q, qw, g, gw)
  tol = 2.0 ** -8 * _abs_bound(q, qw, g, gw) + 1e-5
  i32 = VideoIndex(_cuda(g), _cuda(gw))
  i16 = VideoIndex(_cuda(g), _cuda(gw), dtype=BF16)
  for k in (1, 3, 10):
    s, i = i16.search(_cuda(q), _cuda(qw), k=k)
    s, i = s.cpu().numpy(), i.cpu().numpy()
    err = np.abs(s - np.take_along_axis(ref, i, 1))
    lim = np.take_along_axis(tol, i, 1)
    print(direction, k, 'max err / bound = %.3g' % (err / lim).max())
    assert np.all(err <= lim), (direction, k)
    if k not in want_rows:
      continue
    best = -np.sort(-ref, axis=1)
    rows = np.nonzero(best[:, k - 1] - best[:, k] > 2 * tol.max(1))[0]
    assert len(rows) == want_rows[k], (direction, k, len(rows))
    f = i32.search(_cuda(q), _cuda(qw), k=k)[1].cpu().numpy()
    for r in rows:
      assert set(i[r].tolist()) == set(f[r].tolist()), (direction, k, r)


@pytest.mark.parametrize('dtype', [torch.float32, BF16])
def test_incremental_build_equals_one_shot_build(dtype):
  from mmt_amd.search import VideoIndex
  nv = 6000
  g, gw, q, qw = _random(nv, 300, 3, 64, 11)
  whole = VideoIndex(g, gw, dtype=dtype)
  idx = VideoIndex.empty(nv, 3, 64, DEV, dtype=dtype)
  assert (idx.num_items, idx.capacity, idx.dtype) == (0, nv, dtype) and idx.nbytes == whole.nbytes
  at = 0
  for n in (1, 63, 4097, nv - 4161):
    assert idx.add(g[at:at + n], gw[at:at + n]) == (at, at + n)
    at += n
    assert idx.num_items == at
  assert torch.equal(_bits(idx.folded), _bits(whole.folded))
  assert torch.equal(idx.weights, whole.weights)
  a, b = idx.search(q, qw, k=17), whole.search(q, qw, k=17)
  assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
  before = idx.folded.clone()
  with pytest.raises(ValueError):
    idx.add(g[:1], gw[:1])                         # full
  assert idx.num_items == nv and torch.equal(_bits(before), _bits(idx.folded))
  # a partly filled index searches only what it holds
  part = VideoIndex.empty(nv, 3, 64, DEV, dtype=dtype)
  part.folded.fill_(100.0)                         # rows past num_items must never be scored
  part.add(g[:777], gw[:777])
  with pytest.raises(ValueError):
    part.add(g[:nv - 776], gw[:nv - 776])          # one too many: refused as a whole
  assert part.num_items == 777
  a, b = part.search(q, qw, k=17), VideoIndex(g[:777], gw[:777], dtype=dtype).search(q, qw, k=17)
  assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_chunked_bf16_build_never_holds_the_fp32_gallery():
  from mmt_amd.search import VideoIndex
  nq, nv, m, d, k, chunk = 2048, 131072, 7, 512, 10, 8192
  gen = torch.Generator(device=DEV).manual_seed(5)
  torch.cuda.synchronize()
  torch.cuda.empty_cache()
  base = torch.cuda.memory_allocated()
  torch.cuda.reset_peak_memory_stats()
  idx = VideoIndex.empty(nv, m, d, DEV, dtype=BF16)
  for at in range(0, nv, chunk):
    g = torch.rand(chunk, m, d, device=DEV, generator=gen).sub_(0.5)
    gw = torch.rand(chunk, m, device=DEV, generator=gen)
    assert idx.add(g, gw) == (at, at + chunk)
    del g, gw
  torch.cuda.synchronize()
  growth = torch.cuda.max_memory_allocated() - base
  assert idx.nbytes == nv * m * d * 2 + nv * m * 4
  assert growth < idx.nbytes + 2 * chunk * m * d * 4 + (16 << 20), (growth, idx.nbytes)
  q = torch.rand(nq, m, d, device=DEV, generator=gen) - 0.5
  qw = torch.rand(nq, m, device=DEV, generator=gen)
  torch.cuda.synchronize()
  base = torch.cuda.memory_allocated()
  torch.cuda.reset_peak_memory_stats()
  s, i = idx.search(q, qw, k=k)
  torch.cuda.synchronize()
  growth = torch.cuda.max_memory_allocated() - base
  assert growth < 64 << 20, growth
  assert s.shape == (nq, k) and int(i.min()) >= 0 and int(i.max()) < nv


def test_deterministic_and_argument_errors():
  from mmt_amd.search import VideoIndex
  g, gw, q, qw = _random(5000, 300, 3, 64, 9)
  index = VideoIndex(g, gw, dtype=BF16)
  a, b = index.search(q, qw, k=17), index.search(q, qw, k=17)
  assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
  with pytest.raises(ValueError):
    VideoIndex(g[:, :, :4], gw, dtype=BF16)        # d = 4: bf16 rows are not 16 bytes
  with pytest.raises(ValueError):
    VideoIndex.empty(10, 3, 4, DEV, dtype=BF16)
  for bad in (0, 129):
    with pytest.raises(ValueError):
      index.search(q, qw, k=bad)
  with pytest.raises(ValueError):
    index.search(q.cpu(), qw.cpu())                # wrong device
  with pytest.raises(ValueError):
    index.search(q[:, :2], qw[:, :2])              # M mismatch
  with pytest.raises(ValueError):
    index.search(q[:, :, :32], qw)                 # d mismatch
  empty = VideoIndex.empty(10, 3, 64, DEV, dtype=BF16)
  with pytest.raises(ValueError):
    empty.search(q, qw)                            # nothing stored
  with pytest.raises(ValueError):
    empty.add(g[:4].cpu(), gw[:4].cpu())           # wrong device
  with pytest.raises(ValueError):
    empty.add(g[:4, :2], gw[:4, :2])               # M mismatch
  with pytest.raises(ValueError):
    empty.add(g[:4], gw[:3])                       # weights do not match
  with pytest.raises(ValueError):
    VideoIndex.empty(10, 3, 64, 'cpu', dtype=BF16)
  assert empty.num_items == 0


def test_float32_default_is_untouched():
  from mmt_amd.search import VideoIndex
  g, gw, q, qw = _random(5000, 300, 3, 64, 9)
  a, b = VideoIndex(g, gw), VideoIndex(g, gw, dtype=torch.float32)
  assert a.folded.dtype is torch.float32 and b.folded.dtype is torch.float32 and a.dtype is torch.float32
  assert torch.equal(a.folded, (gw[:, :, None] * g).reshape(5000, -1)) and torch.equal(a.folded, b.folded)
  ra, rb = a.search(q, qw, k=10), b.search(q, qw, k=10)
  assert torch.equal(ra[0], rb[0]) and torch.equal(ra[1], rb[1])
  assert a.nbytes == 5000 * 3 * 64 * 4 + 5000 * 3 * 4
