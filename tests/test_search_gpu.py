"""Top-k retrieval on the device: `metric.compress_predictions` (drop-in for utils/util.py:38-68) and `search.VideoIndex`
(fused fp32-MFMA scoring + selection, never the N_query x N_video matrix).  The expected top k is the reference restated
with a stable sort: np.argsort(-sims[valid], axis=1, kind='stable')[:, :topk]."""
import numpy as np
import pytest
import torch

from tests.fixtures import load_npz
from tests.test_search_cpu import restated_compress_predictions

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
MODS = ('s3d', 'vggish')


def _golden():
  g = load_npz('trainer_valid')
  vid = np.stack([g['vid_embds/' + m] for m in MODS], 1)                  # (24, M, d)
  txt = np.stack([g['text_embds/' + m] for m in MODS], 1)                 # (72, M, d), rows b*C + c
  return g, vid, g['vid_weights'], txt, g['text_weights'].reshape(txt.shape[0], len(MODS))


def _cuda(x):
  return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _ref_sims(q, qw, g, gw):
  """score(q, g) in fp64 (model/model.py:789-837, 'indep')."""
  q, qw, g, gw = (np.asarray(x, np.float64) for x in (q, qw, g, gw))
  num = np.zeros((q.shape[0], g.shape[0]))
  for m in range(q.shape[1]):
    num += (qw[:, m:m + 1] * q[:, m]) @ (gw[:, m:m + 1] * g[:, m]).T
  den = qw @ gw.T
  den[den == 0] = 1e-5
  return num / den


def _assert_topk(ref, idx, scores, k, tol, score_tol):
  """Tolerance-aware: the j-th returned item's reference score equals the j-th best reference score within tol, no item
  repeats, returned scores sit within score_tol of the reference and never increase; where the j-th best is separated from
  its neighbours by more than tol the index is exact."""
  kout = min(k, ref.shape[1])
  assert idx.shape == (ref.shape[0], kout) and idx.dtype == np.int64
  want = np.argsort(-ref, axis=1, kind='stable')[:, :kout + 1]
  for r in range(ref.shape[0]):
    best = ref[r, want[r]]
    got = ref[r, idx[r]]
    assert len(set(idx[r].tolist())) == kout, r
    assert np.all(np.abs(got - best[:kout]) <= tol), (r, got, best)
    if scores is not None:
      assert np.all(np.abs(scores[r] - got) <= score_tol), (r, scores[r], got)
      assert np.all(np.diff(scores[r]) <= 0), r
    for j in range(kout):
      gaps = [abs(best[j] - best[i]) for i in (j - 1, j + 1) if 0 <= i < len(best)]
      if all(gp > tol for gp in gaps):
        assert idx[r, j] == want[r, j], (r, j)


def test_compress_predictions_golden_matrix_exact():
  from mmt_amd.metric import compress_predictions
  g = load_npz('trainer_valid')
  sims, qm = g['sims'], g['query_masks']
  for topk in (1, 5, 10, 24, 30):
    want = restated_compress_predictions(qm, sims, topk)
    for s in (sims, _cuda(sims)):
      got = compress_predictions(qm, s, topk=topk)
      assert isinstance(got, np.ndarray) and got.dtype == np.int64
      assert got.shape == (55, min(topk, 24))
      assert np.array_equal(got, want), topk


def test_equal_scores_come_out_by_ascending_index():
  from mmt_amd.metric import compress_predictions
  rows = np.array([[0.5] * 9,
                   [0.1, 0.3, 0.3, 0.2, 0.3, 0.1, 0.3, 0.0, 0.3],
                   [-1.0, 2.0, -1.0, 2.0, -1.0, 2.0, -1.0, -1.0, 2.0]], np.float32)
  sims = np.repeat(rows, 3, axis=0)  # (9 queries, 9 videos): one caption per video
  qm = np.ones((9, 1), np.float32)
  for topk in (1, 4, 9):
    got = compress_predictions(qm, sims, topk=topk)
    assert np.array_equal(got, restated_compress_predictions(qm, sims, topk)), topk
  assert np.array_equal(compress_predictions(qm, sims, topk=9)[0], np.arange(9))
  # the same through the fused search: an all-zero query weight gives the score 0 everywhere (denominator 1e-5)
  from mmt_amd.search import VideoIndex
  gen = torch.Generator().manual_seed(3)
  index = VideoIndex(torch.rand(300, 2, 8, generator=gen).to(DEV), torch.rand(300, 2, generator=gen).to(DEV))
  s, i = index.search(torch.rand(2, 2, 8, generator=gen).to(DEV), torch.zeros(2, 2, device=DEV), k=128)
  assert torch.equal(i.cpu(), torch.arange(128).repeat(2, 1)) and not s.any()


def test_video_index_on_the_golden_embeddings():
  from mmt_amd.search import VideoIndex
  g, vid, vw, txt, tw = _golden()
  valid = g['query_masks'].reshape(-1).astype(bool)
  index = VideoIndex(_cuda(vid), _cuda(vw))
  for k in (1, 5, 10, 24, 128):
    s, i = index.search(_cuda(txt), _cuda(tw), k=k)
    s, i = s.cpu().numpy()[valid], i.cpu().numpy()[valid]
    ref = g['sims'][valid].astype(np.float64)
    assert np.abs(s - np.take_along_axis(ref, i, 1)).max() < 1e-5
    _assert_topk(ref, i, s, k, 2e-5, 1e-5)
    if k == 10:
      # the CENet text layout (B, M, C, d) / (B, C, M) gives the same rows b*C + c
      t4 = _cuda(txt.reshape(24, 3, 2, -1).transpose(0, 2, 1, 3))
      s4, i4 = index.search(t4, _cuda(g['text_weights']), k=k)
      assert torch.equal(i4.cpu()[torch.from_numpy(valid)], torch.from_numpy(i))


def test_role_swap_video_to_text():
  from mmt_amd.search import VideoIndex
  g, vid, vw, txt, tw = _golden()
  valid = g['query_masks'].reshape(-1).astype(bool)
  index = VideoIndex(_cuda(txt[valid]), _cuda(tw[valid]))
  ref = g['sims'][valid].T.astype(np.float64)  # (24 videos, 55 captions)
  for k in (1, 10, 55):
    s, i = index.search(_cuda(vid), _cuda(vw), k=k)
    _assert_topk(ref, i.cpu().numpy(), s.cpu().numpy(), k, 2e-5, 1e-5)


@pytest.mark.parametrize('nq,nv,m,d,k', [
    (1, 1, 1, 4, 1), (1, 7, 7, 4, 10), (63, 7, 16, 512, 128), (257, 4095, 7, 4, 10), (63, 4097, 1, 512, 128),
    (257, 4097, 16, 4, 1), (1, 70001, 1, 512, 10), (257, 70001, 1, 4, 128), (63, 70001, 16, 4, 10),
    (257, 4095, 7, 512, 1)])
def test_random_sweep_against_fp64(nq, nv, m, d, k):
  from mmt_amd.search import VideoIndex
  rng = np.random.default_rng(nq * 7 + nv + m * 13 + d + k)
  q = (rng.random((nq, m, d), dtype=np.float32) * 2 - 1) / np.float32(np.sqrt(d))
  g = (rng.random((nv, m, d), dtype=np.float32) * 2 - 1) / np.float32(np.sqrt(d))
  qw = rng.uniform(0.1, 1, (nq, m)).astype(np.float32)
  gw = rng.uniform(0.1, 1, (nv, m)).astype(np.float32)
  qw[nq // 2] = 0   # denominator 1e-5 on the query side: every score 0
  gw[nv // 3] = 0   # ... and on the gallery side: one column 0
  s, i = VideoIndex(_cuda(g), _cuda(gw)).search(_cuda(q), _cuda(qw), k=k)
  ref = _ref_sims(q, qw, g, gw)
  _assert_topk(ref, i.cpu().numpy(), s.cpu().numpy(), k, 1e-5, 1e-5)
  assert np.array_equal(i[nq // 2].cpu().numpy(), np.arange(min(k, nv)))


def test_search_allocates_no_quadratic_buffer():
  from mmt_amd.search import VideoIndex
  nq, nv, m, d, k = 2048, 131072, 7, 512, 10
  gen = torch.Generator(device=DEV).manual_seed(5)
  g = torch.rand(nv, m, d, device=DEV, generator=gen) - 0.5
  gw = torch.rand(nv, m, device=DEV, generator=gen)
  q = torch.rand(nq, m, d, device=DEV, generator=gen) - 0.5
  qw = torch.rand(nq, m, device=DEV, generator=gen)
  index = VideoIndex(g, gw)
  torch.cuda.synchronize()
  base = torch.cuda.memory_allocated()
  torch.cuda.reset_peak_memory_stats()
  s, i = index.search(q, qw, k=k)
  torch.cuda.synchronize()
  growth = torch.cuda.max_memory_allocated() - base
  assert growth < 64 << 20, growth  # the matrix alone would be 1 GiB
  # the materialised path on sampled rows: the kernels of eval_similarity (mmt_sims_eval) and of compress_predictions
  # (mmt_rows_topk); the public functions want NQ = NV * captions, which this gallery shape is not
  del index
  from mmt_amd import _lib, ops
  L = _lib.lib()
  rows = torch.arange(0, nq, 97, device=DEV)
  nt = len(rows)
  qs, qws = q[rows].contiguous(), qw[rows].contiguous()
  ws = torch.empty(L.mmt_sims_eval_workspace_floats(nt, nv, m, d), device=DEV)
  sims = torch.empty(nt, nv, device=DEV)
  assert L.mmt_sims_eval(ops._p(qs), ops._p(g), ops._p(qws), ops._p(gw), nt, nv, m, d, ops._p(ws), ops._p(sims),
                         ops._stream()) == 0
  tk = torch.empty(L.mmt_topk_workspace_keys(nt, nv, k), device=DEV, dtype=torch.int64)
  mi = torch.empty(nt, k, device=DEV, dtype=torch.int64)
  assert L.mmt_rows_topk(ops._p(sims), nv, None, nt, nv, k, ops._p(tk), None, ops._p(mi), ops._stream()) == 0
  ref = sims.double().cpu().numpy()
  _assert_topk(ref, mi.cpu().numpy(), None, k, 0.0, 0.0)  # the row select is exact on the matrix it is given
  _assert_topk(ref, i[rows].cpu().numpy(), s[rows].cpu().numpy(), k, 2e-5, 2e-5)


def test_deterministic_and_argument_errors():
  from mmt_amd.search import VideoIndex
  gen = torch.Generator(device=DEV).manual_seed(9)
  g, gw = torch.randn(5000, 3, 64, device=DEV, generator=gen), torch.rand(5000, 3, device=DEV, generator=gen)
  q, qw = torch.randn(300, 3, 64, device=DEV, generator=gen), torch.rand(300, 3, device=DEV, generator=gen)
  index = VideoIndex(g, gw)
  a, b = index.search(q, qw, k=17), index.search(q, qw, k=17)
  assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
  for bad in (0, 129):
    with pytest.raises(ValueError):
      index.search(q, qw, k=bad)
  with pytest.raises(ValueError):
    index.search(q[:, :2], qw[:, :2])           # M mismatch
  with pytest.raises(ValueError):
    index.search(q[:, :, :32], qw)              # d mismatch
  with pytest.raises(ValueError):
    index.search(q.cpu(), qw.cpu())             # CPU tensors
  with pytest.raises(ValueError):
    VideoIndex(g.cpu(), gw.cpu())
