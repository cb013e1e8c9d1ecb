"""Drop-in for the reference's `model/metric.py` retrieval metrics, computed on the MI355X.

`t2v_metrics(sims, query_masks=None)` / `v2t_metrics(sims, query_masks=None)` keep the reference signatures and
result keys (model/metric.py:26-150, 153-243, 246-258) but rank on the device: `sims` may be a CUDA tensor (it then
never leaves HBM -- only the n rank values are copied to the host) or a numpy array (uploaded once).
`retrieval_metrics(...)` goes one step further and also builds the N_text x N_video similarity on the device from
the gathered embeddings (the reference does both on the CPU: trainer/trainer.py:396-447).  SURVEY.md section 8f.1.
`retrieval_metrics_indexed(...)` gives the same metrics from exact rank counts over a search.VideoIndex, without the
matrix: for eval sets whose N_text x N_video similarity does not fit; caption_mode='avg' gives the reference's merged-caption
evaluation the same way (query-set pooling for text-to-video, item-set pooling for video-to-text).
`info_nce_indexed(...)` evaluates the reference's InfoNceLoss (model/loss.py:68-81) over a whole evaluation set the same
way: the row log-sum-exps from VideoIndex.query_lse, the column ones from hub_norm, the diagonal from target_scores.
"""
import numpy as np
import torch

from . import _lib, ops
from ._lib import check


def _as_cuda_f32(x):
  if not torch.is_tensor(x):
    x = torch.from_numpy(np.ascontiguousarray(x))
  if not torch.cuda.is_available():
    raise RuntimeError('mmt_amd.metric needs a GPU (no CPU fallback)')
  return x.to(device='cuda', dtype=torch.float32).contiguous()


def retrieval_ranks(sims, query_masks=None):
  """sims [NQ = NV*cpv, NV] (rows = text queries) -> (t2v 0-based ranks [NQ], v2t best rank per video [NV]),
  tie-averaged like the reference; both float32 CUDA tensors."""
  sims = _as_cuda_f32(sims)
  nq, nv = sims.shape
  qm = None
  if query_masks is not None:
    qm = torch.as_tensor(np.asarray(query_masks.cpu() if torch.is_tensor(query_masks) else query_masks)).reshape(-1)
    qm = (qm != 0).to(device=sims.device, dtype=torch.uint8).contiguous()
    assert qm.numel() == nq
  t2v = torch.empty(nq, device=sims.device, dtype=torch.float32)
  v2t = torch.empty(nv, device=sims.device, dtype=torch.float32)
  scratch = torch.empty(nq, device=sims.device, dtype=torch.float32)
  check(_lib.lib().mmt_retrieval_ranks(ops._p(sims), ops._p(qm), nq, nv, ops._p(t2v), ops._p(v2t), ops._p(scratch),
                                       ops._stream()), 'mmt_retrieval_ranks')
  return t2v, v2t, qm


def cols2metrics(cols, num_queries):
  """model/metric.py:246-258 (same keys; numpy on the O(n) rank vector)."""
  cols = np.asarray(cols, dtype=np.float64)
  metrics = {}
  metrics['R1'] = 100 * float(np.sum(cols == 0)) / num_queries
  metrics['R5'] = 100 * float(np.sum(cols < 5)) / num_queries
  metrics['R10'] = 100 * float(np.sum(cols < 10)) / num_queries
  metrics['R50'] = 100 * float(np.sum(cols < 50)) / num_queries
  metrics['MedR'] = float(np.median(cols) + 1)
  metrics['MeanR'] = float(np.mean(cols) + 1)
  stats = np.array([metrics[x] for x in ('R1', 'R5', 'R10')])
  metrics['geometric_mean_R1-R5-R10'] = float(np.exp(np.mean(np.log(stats)))) if (stats > 0).all() else 0.0
  return metrics


def t2v_metrics(sims, query_masks=None):
  """Text-to-video retrieval metrics; sims: (N_text, N_video), text rows grouped per video."""
  t2v, _, qm = retrieval_ranks(sims, query_masks)
  cols = t2v.cpu().numpy()
  if qm is not None:
    cols = cols[qm.cpu().numpy().astype(bool)]
  out = cols2metrics(cols, cols.size)
  out['cols'] = cols
  return out


def v2t_metrics(sims, query_masks=None):
  """Video-to-text retrieval metrics (best rank among a video's own captions)."""
  _, v2t, _ = retrieval_ranks(sims, query_masks)
  cols = v2t.cpu().numpy()
  out = cols2metrics(cols, cols.size)
  out['cols'] = cols
  return out


def eval_similarity(vid_embds, text_embds, vid_weights, text_weights):
  """(B,M,d), (B,M,C,d), (B,M), (B,C,M) -> sims (B*C, B) on the device ('indep' caption mode, model.py:826-836)."""
  vid = _as_cuda_f32(vid_embds)
  txt4 = _as_cuda_f32(text_embds)
  b, m, d = vid.shape
  c = txt4.shape[2]
  txt = txt4.permute(0, 2, 1, 3).reshape(b * c, m, d).contiguous()
  tw = _as_cuda_f32(text_weights).reshape(b * c, m).contiguous()
  vw = _as_cuda_f32(vid_weights).reshape(b, m).contiguous()
  L = _lib.lib()
  ws = torch.empty(L.mmt_sims_eval_workspace_floats(b * c, b, m, d), device=vid.device, dtype=torch.float32)
  sims = torch.empty(b * c, b, device=vid.device, dtype=torch.float32)
  check(L.mmt_sims_eval(ops._p(txt), ops._p(vid), ops._p(tw), ops._p(vw), b * c, b, m, d, ops._p(ws), ops._p(sims),
                        ops._stream()), 'mmt_sims_eval')
  return sims


def retrieval_metrics(vid_embds, text_embds, vid_weights, text_weights, query_masks=None):
  """Embeddings of the whole eval set -> {'t2v_metrics': {...}, 'v2t_metrics': {...}} without an n^2 host copy."""
  sims = eval_similarity(vid_embds, text_embds, vid_weights, text_weights)
  return {'t2v_metrics': t2v_metrics(sims, query_masks), 'v2t_metrics': v2t_metrics(sims, query_masks)}


def v2t_targets(query_masks, num_videos, captions_per_video):
  """query_masks (None = every caption real; else anything of num_videos * captions_per_video entries, nonzero = real)
  -> (valid bool [B*C], targets int64 [B, C]): targets[b, c] is the position of caption (b, c) in the gallery of the real
  captions only (rows b*C + c with valid set, in order), -1 where it is masked.  Pure numpy: the renumbering behind
  retrieval_metrics_indexed's video-to-text half."""
  n = num_videos * captions_per_video
  if query_masks is None:
    valid = np.ones(n, dtype=bool)
  else:
    qm = np.asarray(query_masks.cpu() if torch.is_tensor(query_masks) else query_masks).reshape(-1)
    if qm.size != n:
      raise ValueError('query_masks has %d entries, %d videos x %d captions expected' % (qm.size, num_videos, captions_per_video))
    valid = qm != 0
  targets = np.where(valid, np.cumsum(valid) - 1, -1).astype(np.int64)
  return valid, targets.reshape(num_videos, captions_per_video)


def retrieval_metrics_indexed(vid_embds, text_embds, vid_weights, text_weights, query_masks=None, dtype=torch.float32,
                              video_subset=None, devices=None, text_bank=None, video_bank=None, beta=None,
                              caption_mode='indep', bank_norm='softmax', bank_k=10):
  """`retrieval_metrics` (same arguments, same result dict and keys) without the N_text x N_video matrix: the rank of every
  ground truth comes from search.VideoIndex.ranks, so no buffer grows with N_text * N_video.  t2v: an index of the videos
  queried with the real captions, the target of caption row b*C + c being video b.  v2t: an index of the real captions
  queried with the videos, each video's targets its own captions (`v2t_targets`), the best of their ranks kept (+inf for a
  video without a real caption, as mmt_retrieval_ranks).  dtype: the index storage, torch.float32 or torch.bfloat16.
  video_subset (bool [B], or int64 video numbers in any order): the metrics of one cut of the set -- what this function
  gives on the arrays gathered to the cut's videos in ascending order -- from the SAME two indexes over all videos and
  all real captions (VideoIndex.subset): t2v queries are the real captions of the cut's videos and rank among the cut's
  videos; v2t queries are the cut's videos and rank among the real captions of the cut.
  devices (a list of CUDA devices): both indexes are search.ShardedVideoIndex over those devices, the arrays and the
  ranking on devices[0]; the result is the same, bit for bit.
  text_bank / video_bank ((embds, weights) pairs in either query layout of VideoIndex.search) with beta (a float > 0):
  querybank hubness normalisation (VideoIndex.hub_norm) -- a bank of text queries re-scores the t2v ranking over the video
  index, a bank of videos the v2t ranking over the caption index; either may be given alone.
  bank_norm: 'softmax' (that, the default) or 'csls': the banks build VideoIndex.csls_norm(k=bank_k) instead -- CSLS, the
  mean of each item's bank_k best bank scores in the same norm slot with beta = 2 -- and beta, which it has no use for,
  must be None.
  caption_mode: 'indep' (every caption a query of its own, as above) or 'avg' (the reference's
  merge_caption_similiarities = 'avg', model/model.py:826-831: a video's C captions answer as one, on the mean of their
  similarities) -- then the result is what t2v_metrics / v2t_metrics give on the B x B matrix of those means.  t2v: the
  video index is queried with the captions under VideoIndex.pooling(C, B), the target of set b being video b.  v2t: an
  index of all B * C captions in row order b*C + c carries VideoIndex.item_pooling(C) with the default weights (the
  reference's mean includes every caption) and is queried with the videos, the target of video b being set b.
  video_subset and devices work as above (the sharded caption index is filled so that every set stays whole on one
  shard); query_masks, text_bank and video_bank with 'avg' raise ValueError: the reference gives masked captions no
  meaning in this mode, and pooling does not combine with a norm."""
  from .search import ShardedVideoIndex, VideoIndex
  if caption_mode not in ('indep', 'avg'):
    raise ValueError("retrieval_metrics_indexed: caption_mode must be 'indep' or 'avg', got %r" % (caption_mode,))
  if caption_mode == 'avg' and (query_masks is not None or text_bank is not None or video_bank is not None):
    raise ValueError("retrieval_metrics_indexed: caption_mode='avg' does not combine with query_masks, text_bank or video_bank")
  if bank_norm not in ('softmax', 'csls'):
    raise ValueError("retrieval_metrics_indexed: bank_norm must be 'softmax' or 'csls', got %r" % (bank_norm,))
  if bank_norm == 'csls' and beta is not None:
    raise ValueError("retrieval_metrics_indexed: bank_norm='csls' takes no beta (it is 2 by definition), got %r" % (beta,))
  if bank_norm == 'softmax' and (text_bank is not None or video_bank is not None) and beta is None:
    raise ValueError('retrieval_metrics_indexed: a bank needs beta')
  for bank in (text_bank, video_bank):
    if bank is not None and not (isinstance(bank, (tuple, list)) and len(bank) == 2):
      raise ValueError('retrieval_metrics_indexed: a bank is an (embds, weights) pair')
  if devices is None:
    make_index = VideoIndex
  else:
    devices = [torch.device(dev) for dev in devices]

    def make_index(embds, weights, dtype):
      return ShardedVideoIndex(embds, weights, devices, dtype=dtype)
  b, m, d = vid_embds.shape
  c = text_embds.shape[2]
  valid, targets = v2t_targets(query_masks, b, c)
  cut = None
  if video_subset is not None:
    vs = np.asarray(video_subset.cpu() if torch.is_tensor(video_subset) else video_subset)
    if vs.dtype == bool:
      if vs.shape != (b,):
        raise ValueError('retrieval_metrics_indexed: a bool video_subset of shape (%d,) expected, got %s' % (b, vs.shape))
      cut = vs
    else:
      if vs.dtype.kind not in 'iu' or vs.size and (vs.min() < 0 or vs.max() >= b):
        raise ValueError('retrieval_metrics_indexed: video_subset must be a bool mask or video numbers in 0 .. %d' % (b - 1))
      cut = np.zeros(b, dtype=bool)
      cut[vs.reshape(-1)] = True
    if not (valid & np.repeat(cut, c)).any():
      raise ValueError('retrieval_metrics_indexed: video_subset leaves no caption to rank')
  if not valid.any():
    raise ValueError('retrieval_metrics_indexed: query_masks leaves no caption to rank')
  vid = _as_cuda_f32(vid_embds)
  txt4 = _as_cuda_f32(text_embds)
  vw = _as_cuda_f32(vid_weights).reshape(b, m).contiguous()
  tw = _as_cuda_f32(text_weights).reshape(b * c, m)
  if devices is not None:
    vid, txt4, vw, tw = (x.to(devices[0]) for x in (vid, txt4, vw, tw))

  def normaliser(index, bank):
    if bank is None:
      return None
    bank = tuple(_as_cuda_f32(x).to(vid.device) for x in bank)
    return index.csls_norm(*bank, k=bank_k) if bank_norm == 'csls' else index.hub_norm(*bank, beta)
  if caption_mode == 'avg':
    return _metrics_avg(make_index, devices, vid, vw, txt4.permute(0, 2, 1, 3).reshape(b * c, m, d).contiguous(),
                        tw.contiguous(), c, cut, dtype)
  rows = torch.from_numpy(np.flatnonzero(valid)).to(vid.device)
  txt = txt4.permute(0, 2, 1, 3).reshape(b * c, m, d)[rows].contiguous()      # the real captions, rows b*C + c in order
  tw = tw[rows].contiguous()
  if cut is not None:
    dev = vid.device
    cut_d = torch.from_numpy(cut).to(dev)
    mine = cut_d[rows // c]                                                     # real captions of the cut's videos
    videos = make_index(vid, vw, dtype=dtype)
    cols = videos.ranks(txt[mine], tw[mine], (rows // c)[mine], subset=videos.subset(cut_d),
                        norm=normaliser(videos, text_bank)).cpu().numpy()
    out = {'t2v_metrics': dict(cols2metrics(cols, cols.size), cols=cols)}
    captions = make_index(txt, tw, dtype=dtype)
    ranks = captions.ranks(vid[cut_d], vw[cut_d], torch.from_numpy(targets).to(dev)[cut_d], subset=captions.subset(mine),
                           norm=normaliser(captions, video_bank))
    cols = ranks.min(dim=1).values.cpu().numpy()
    out['v2t_metrics'] = dict(cols2metrics(cols, cols.size), cols=cols)
    return out
  videos = make_index(vid, vw, dtype=dtype)
  cols = videos.ranks(txt, tw, rows // c, norm=normaliser(videos, text_bank)).cpu().numpy()
  del videos
  out = {'t2v_metrics': dict(cols2metrics(cols, cols.size), cols=cols)}
  captions = make_index(txt, tw, dtype=dtype)
  ranks = captions.ranks(vid, vw, torch.from_numpy(targets).to(vid.device), norm=normaliser(captions, video_bank))
  cols = ranks.min(dim=1).values.cpu().numpy()
  out['v2t_metrics'] = dict(cols2metrics(cols, cols.size), cols=cols)
  return out


def _metrics_avg(make_index, devices, vid, vw, txt, tw, c, cut, dtype):
  """`retrieval_metrics_indexed` in 'avg' mode behind its checks: vid (B, M, d) / vw (B, M), txt (B*C, M, d) / tw (B*C, M)
  in row order b*C + c, all on one device; cut None or a bool numpy mask [B]."""
  from .search import ShardedVideoIndex
  b, m, d = vid.shape
  dev = vid.device
  if cut is None:
    mine = torch.arange(b, device=dev)
  else:
    mine = torch.from_numpy(np.flatnonzero(cut)).to(dev)
  cut_d = None if cut is None else torch.from_numpy(cut).to(dev)
  nb = mine.shape[0]
  videos = make_index(vid, vw, dtype=dtype)
  sets = txt.view(b, c, m, d)[mine].reshape(nb * c, m, d)
  cols = videos.ranks(sets, tw.view(b, c, m)[mine].reshape(nb * c, m), mine, pooling=videos.pooling(c, nb),
                      subset=None if cut is None else videos.subset(cut_d)).cpu().numpy()
  del videos
  out = {'t2v_metrics': dict(cols2metrics(cols, cols.size), cols=cols)}
  if devices is None:
    captions = make_index(txt, tw, dtype=dtype)
  else:  # every shard's capacity a multiple of C, filled in pieces of whole sets that fit one shard: the sets stay whole
    per_shard = -(-b // len(devices)) * c
    captions = ShardedVideoIndex.empty(per_shard * len(devices), m, d, devices, dtype=dtype)
    for r0 in range(0, b * c, per_shard):
      captions.add(txt[r0:r0 + per_shard], tw[r0:r0 + per_shard])
  ip = captions.item_pooling(c)
  cols = captions.ranks(vid[mine], vw[mine], mine, item_pooling=ip,
                        subset=None if cut is None else ip.subset(cut_d)).cpu().numpy()
  out['v2t_metrics'] = dict(cols2metrics(cols, cols.size), cols=cols)
  return out


def info_nce_indexed(vid_embds, text_embds, vid_weights, text_weights, scale=1.0, dtype=torch.float32):
  """The reference's InfoNceLoss (model/loss.py:68-81: cross entropy of the rows plus cross entropy of the columns, each a
  mean, targets on the diagonal) on scale * sims over a whole evaluation set with ONE caption per video -- vid (B, M, d) /
  (B, M), text (B, M, 1, d) / (B, 1, M) or (B, M, d) / (B, M) -- without the B x B matrix, from three scans of one
  search.VideoIndex of the videos queried with the captions:
      rows     : query_lse(captions, beta=scale).lse[i] = log sum_j exp(scale * sims[i, j])
      columns  : hub_norm(bank=captions, beta=scale).lse[j] = log sum_i exp(scale * sims[i, j])
      diagonal : target_scores(captions, i -> video i)
  -> {'loss': t2v + v2t, 't2v': mean_i(rows[i] - scale * sims[i, i]), 'v2t': mean_j(columns[j] - scale * sims[j, j])} as
  Python floats, the differences and the means taken in float64.  scale: a Python float, 0 < scale < inf.  dtype: the
  index storage, torch.float32 or torch.bfloat16 (the loss is then that of the bfloat16 index's own scores);
  torch.float8_e4m3fn is refused, because `hub_norm` is."""
  from .search import FP8, VideoIndex
  if isinstance(scale, bool) or not isinstance(scale, float) or not 0 < scale < float('inf'):
    raise ValueError('info_nce_indexed: scale must be a float with 0 < scale < inf, got %r' % (scale,))
  if dtype == FP8:
    raise ValueError('info_nce_indexed: %s is not supported: hub_norm is not available on such an index' % (dtype,))
  if dtype not in (torch.float32, torch.bfloat16):
    raise ValueError('info_nce_indexed: dtype must be torch.float32 or torch.bfloat16, got %r' % (dtype,))
  if len(vid_embds.shape) != 3:
    raise ValueError('info_nce_indexed: vid_embds (B, M, d) expected, got %s' % (tuple(vid_embds.shape),))
  b, m, d = vid_embds.shape
  if tuple(text_embds.shape) not in ((b, m, 1, d), (b, m, d)):
    raise ValueError('info_nce_indexed: one caption per video, text_embds (%d, %d, 1, %d) expected, got %s' % (
        b, m, d, tuple(text_embds.shape)))
  vid = _as_cuda_f32(vid_embds)
  vw = _as_cuda_f32(vid_weights).reshape(b, m).contiguous()
  txt = _as_cuda_f32(text_embds).reshape(b, m, d)
  tw = _as_cuda_f32(text_weights).reshape(b, m).contiguous()
  videos = VideoIndex(vid, vw, dtype=dtype)
  rows = videos.query_lse(txt, tw, scale).lse.double()
  cols = videos.hub_norm(txt, tw, scale).lse.double()
  diag = videos.target_scores(txt, tw, torch.arange(b, device=vid.device)).double() * scale
  t2v, v2t = float((rows - diag).mean()), float((cols - diag).mean())
  return {'loss': t2v + v2t, 't2v': t2v, 'v2t': v2t}


def compress_predictions(query_masks, sims, topk=10):
  """Drop-in for utils/util.py:38-68 (trainer/trainer.py:411-437, sets == 'final_eval'): the masked query rows are dropped
  and each remaining row of `sims` keeps the indices of its `topk` highest columns, best first -> numpy int64
  [n_valid, min(topk, N_video)].  The selection runs on the device (mmt_rows_topk): a numpy `sims` is uploaded once, a
  CUDA tensor never leaves HBM; only the index rows come back.  Equal scores come out by ascending column index (a stable
  argsort); the reference's quicksort argsort leaves their order unspecified, the one place the two can differ."""
  qm = np.asarray(query_masks.cpu() if torch.is_tensor(query_masks) else query_masks)
  assert qm.ndim == 2, 'Expected query_masks to be a matrix'
  query_num_videos, query_max_per_video = qm.shape
  sims_queries, sims_num_videos = tuple(sims.shape)
  msg = (f'Expected sims and query masks to represent the same number of videos '
         f'(found {sims_num_videos} v {query_num_videos}')
  assert query_num_videos == sims_num_videos, msg
  msg = (f'Expected sims and query masks to represent the same number of queries '
         f'(found {sims_queries} v {query_num_videos * query_max_per_video}')
  assert query_max_per_video * query_num_videos == sims_queries, msg
  kout = min(int(topk), sims_num_videos)
  if kout < 1 or kout > 128:
    raise ValueError('compress_predictions: topk must give 1..128 columns, got topk=%r for %d videos' % (topk, sims_num_videos))
  rows = np.flatnonzero(qm.reshape(-1).astype(bool)).astype(np.int32)
  if rows.size == 0:
    return np.zeros((0, kout), dtype=np.int64)
  sims = _as_cuda_f32(sims)
  dev = sims.device
  rows_d = torch.from_numpy(rows).to(dev)
  L = _lib.lib()
  ws = torch.empty(L.mmt_topk_workspace_keys(rows.size, sims_num_videos, kout), device=dev, dtype=torch.int64)
  index = torch.empty(rows.size, kout, device=dev, dtype=torch.int64)
  check(L.mmt_rows_topk(ops._p(sims), sims.stride(0), ops._p(rows_d), rows.size, sims_num_videos, kout, ops._p(ws), None,
                        ops._p(index), ops._stream()), 'mmt_rows_topk')
  return index.cpu().numpy()
