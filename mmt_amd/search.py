"""Text-to-video search over a gallery held on the MI355X: the k best videos per query without the N_query x N_video
similarity matrix.

    index = VideoIndex(vid_embds, vid_weights)          # (NV, M, d), (NV, M) CUDA tensors; folded once
    scores, indices = index.search(text_embds, text_weights, k=10)

The score is the 'indep' similarity of model/model.py:789-837 (the matrix `metric.eval_similarity` builds):
    score(q, g) = sum_m qw[q][m] gw[g][m] <Q_m[q], G_m[g]> / sum_m qw[q][m] gw[g][m]     (0 -> 1e-5)
It is symmetric, so video-to-text search is an index of captions queried with videos.  Each query gets min(k, NV)
(score, index) pairs, best first, equal scores by ascending gallery index.  One launch scores 64-query x 4096-video
blocks on the fp32 matrix cores and keeps a running top-k per query; a second merges the chunk lists (mmt_search_topk).
Results are bit-reproducible.
"""
import torch

from . import _lib, ops
from ._lib import check

MAX_K = 128
_BATCH_BYTES = 48 << 20  # folded queries + chunk lists per launch


def _cuda_f32(x, name):
  if not torch.is_tensor(x) or not x.is_cuda:
    raise ValueError('%s must be a CUDA tensor' % name)
  return x.to(torch.float32).contiguous()


def _fold(x, w):
  n, m, d = x.shape
  out = torch.empty(n, m * d, device=x.device, dtype=torch.float32)
  check(_lib.lib().mmt_search_fold(ops._p(x), ops._p(w), n, m, d, ops._p(out), ops._stream()), 'mmt_search_fold')
  return out


class VideoIndex:
  """A gallery of NV items with M expert embeddings of width d (d % 4 == 0, M <= 16), weighted per item and expert."""

  def __init__(self, embds, weights):
    g = _cuda_f32(embds, 'embds')
    gw = _cuda_f32(weights, 'weights')
    if g.dim() != 3 or gw.shape != g.shape[:2]:
      raise ValueError('VideoIndex expects embds (NV, M, d) and weights (NV, M), got %s and %s' % (
          tuple(g.shape), tuple(gw.shape)))
    nv, m, d = g.shape
    if nv < 1 or not 1 <= m <= 16 or d < 4 or d % 4:
      raise ValueError('VideoIndex: need NV >= 1, 1 <= M <= 16 and d % 4 == 0, got %s' % (tuple(g.shape),))
    self.num_items, self.num_experts, self.dim = nv, m, d
    self.device = g.device
    with torch.cuda.device(self.device):
      self.folded = _fold(g, gw)  # gw (.) G: [NV, M*d]
    self.weights = gw

  def _queries(self, embds, weights):
    q = _cuda_f32(embds, 'embds')
    qw = _cuda_f32(weights, 'weights')
    m, d = self.num_experts, self.dim
    if q.dim() == 4:  # CENet text layout (B, M, C, d) / (B, C, M) -> rows b*C + c, as metric.eval_similarity
      b, qm, c, qd = q.shape
      if (qm, qd) != (m, d) or tuple(qw.shape) != (b, c, m):
        raise ValueError('search: text embds (B, %d, C, %d) with weights (B, C, %d) expected, got %s and %s' % (
            m, d, m, tuple(q.shape), tuple(qw.shape)))
      q = q.permute(0, 2, 1, 3).reshape(b * c, m, d).contiguous()
      qw = qw.reshape(b * c, m).contiguous()
    elif q.dim() != 3 or tuple(q.shape[1:]) != (m, d) or tuple(qw.shape) != (q.shape[0], m):
      raise ValueError('search: embds (NQ, %d, %d) with weights (NQ, %d) expected, got %s and %s' % (
          m, d, m, tuple(q.shape), tuple(qw.shape)))
    if q.device != self.device or qw.device != self.device:
      raise ValueError('search: queries must be on the index device %s' % self.device)
    return q, qw

  def search(self, embds, weights, k=10):
    """Queries (NQ, M, d) / (NQ, M), or the text layout (B, M, C, d) / (B, C, M) -> (scores [NQ, k'] float32,
    indices [NQ, k'] int64) on the device, k' = min(k, NV), best first."""
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= MAX_K:
      raise ValueError('search: k must be an int in 1..%d, got %r' % (MAX_K, k))
    q, qw = self._queries(embds, weights)
    nq, nv, m, d = q.shape[0], self.num_items, self.num_experts, self.dim
    kout = min(k, nv)
    scores = torch.empty(nq, kout, device=self.device, dtype=torch.float32)
    indices = torch.empty(nq, kout, device=self.device, dtype=torch.int64)
    if nq == 0:
      return scores, indices
    L = _lib.lib()
    with torch.cuda.device(self.device):
      per_row = m * d * 4 + 8 * k * -(-nv // 4096)  # folded row + its chunk lists at full-size chunks
      batch = max(64, (_BATCH_BYTES // per_row) // 64 * 64)
      for r0 in range(0, nq, batch):
        r1 = min(nq, r0 + batch)
        qf = _fold(q[r0:r1], qw[r0:r1])
        ws = torch.empty(L.mmt_topk_workspace_keys(r1 - r0, nv, k), device=self.device, dtype=torch.int64)
        check(L.mmt_search_topk(ops._p(qf), ops._p(qw[r0:r1]), ops._p(self.folded), ops._p(self.weights), r1 - r0, nv, m,
                                d, k, ops._p(ws), ops._p(scores[r0:r1]), ops._p(indices[r0:r1]), ops._stream()),
              'mmt_search_topk')
    return scores, indices
