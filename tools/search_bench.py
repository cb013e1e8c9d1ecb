"""Top-k text-to-video search: fused score + select (search.VideoIndex.search) against the materialised path (the
N_query x N_video similarity of metric.eval_similarity, then the device compress_predictions), M = 7, d = 512, k = 10.

  S1  1 000 x 1 000      MSRVTT 1k-A size
  S2  4 917 x 4 917      ActivityNet val1 size
  S3  4 096 x 262 144    gallery search

Times with device events after warm-up, over >= --min-seconds of work per point; reports peak allocator growth,
FLOP/s from 2 NQ NV M d and the fraction of the 157.3 TF fp32 matrix peak.  At S1 / S2 (one caption per video) the
materialised path is the public eval_similarity + compress_predictions; at S3 (NQ != NV * captions, which those
functions require) it is their kernels, mmt_sims_eval + mmt_rows_topk.
   python tools/search_bench.py [--shapes S1,S2,S3] [--out profiles/search_bench.json] [--min-seconds 0.5]

--gallery-dtype bfloat16 times the bf16-stored index instead; --gallery-dtype both times the two indexes side by side on
the same data (--runs timed runs each, interleaved; median and spread = max - min) and reports per shape the index bytes,
peak memory, TF (2 NQ NV M d counted once: the hi / lo query split is overhead, not work) and the share of rows whose
index lists agree.  The bf16 index is built in chunks (VideoIndex.empty + add).

--ranks times the exact rank of one ground-truth item per query (VideoIndex.ranks, T = 1) on both indexes, beside
search(k = 1) and search(k = 10) on the same index -- the same scan with the top-k epilogue, the yardstick -- and beside
the materialised path (mmt_sims_eval + mmt_retrieval_ranks: the N_query x N_video matrix, then its ranking) where that
path applies (it wants NQ = NV x captions, so S1 and S2).  --runs rounds, every variant once per round, interleaved;
median and spread.  Default output profiles/search_ranks_bench.json.

--subset FRACTION and / or --exclude E time the masked search (VideoIndex.search(subset=, exclude=)) beside the unmasked
one on the same index (--gallery-dtype, both = the two indexes): an all-ones subset (the cost of the predicate), a
contiguous FRACTION of the items (whole tiles skipped: the time should follow the fraction), a random FRACTION (no tile
skips: as all-ones), and E exclusions per query without a subset (the query's own item and E - 1 random ones).  --runs
rounds, every variant once per round, interleaved; median and spread.  Default output profiles/search_subset_bench.json.

--shards N times search.ShardedVideoIndex with N shards in place of the single index of the default mode: the shards go to
the visible devices in turn (cuda:0, cuda:1, ..., again from cuda:0 when there are fewer devices than shards), queries
and results on cuda:0.  On one device the difference to the plain run is the cost of the merge launch, the staged lists
and of scanning N shorter galleries; with --skip-materialised only the index is timed.

--norm BETA times querybank hubness normalisation (VideoIndex.hub_norm, search(norm=)) with the queries as the bank, per
index dtype (--gallery-dtype, both = the two indexes): the lse pass over the bank (hub_norm: mmt_search_col_lse), the
normalised search and the plain search of the same build, which is also the plain scan of the same bank.  --runs rounds,
every variant once per round, interleaved; median and spread, and the two costs as ratios: normalised over plain search,
lse pass over plain scan.  --baseline-json FILE... records beside them the plain search of another build (default-mode
outputs of its own search_bench, --skip-materialised, run in the same session) and --same-build-json FILE... such runs
of this build, taken alternately with them.  The result goes under the key "norm" of
--out (default profiles/search_bench.json), whose other content is kept.

--reverse K times the reverse search (VideoIndex.reverse_search: for every stored item the K best query rows, 1 <= K <= 32)
and the CSLS normaliser on top of it (VideoIndex.csls_norm) with the queries as the rows / the bank, per index dtype
(--gallery-dtype, both = the two indexes): reverse_search(k = K), reverse_search(k = 32) and csls_norm(k = K), beside the
lse pass of hub_norm over the same bank on the same index -- the same scan with the cheapest column pass, existing code,
the yardstick -- and the plain search(k = 10).  --runs rounds, every variant once per round, interleaved; median and
spread, and each cost as a ratio over the lse pass.  The result goes under the key "reverse" of --out (default
profiles/search_bench.json), whose other content is kept.

--range HITS times the range search (VideoIndex.range_search: every item at or above a per-query threshold, two scans) per
index dtype (--gallery-dtype, both = the two indexes).  The thresholds are the HITS-th best score of each query (the last
score of search(k = HITS), 1 <= HITS <= 128), so every query has at least HITS hits.  Beside it, on the same index:
threshold_counts against the same thresholds (T = 1: one scan, the yardstick -- a range search should cost about two) and
search(k = 10).  --runs rounds, every variant once per round, interleaved; median and spread.  --counts-only times the
two yardsticks alone: it calls nothing a build without range_search lacks, so the same file run inside a checkout of the
parent commit gives the parent's numbers, and --baseline-json FILE... records such results beside this build's.  Default
output profiles/search_range_bench.json.

--groups SIZE times the grouped search (VideoIndex.search_groups, k = 10: the k best groups, each with its best item) per
index dtype (--gallery-dtype, both = the two indexes) with the items in groups of SIZE: contiguous groups (item i in group
i // SIZE: a clip gallery stored video by video) and the same groups with the item order shuffled (members anywhere: every
chunk list can hold any group, so the merge de-duplicates), beside the plain search(k = 10) of the same index -- the same
scan with the plain running list, the yardstick.  --runs rounds, every variant once per round, interleaved; median and
spread.  Default output profiles/search_groups_bench.json.

--pooled C times the pooled search (VideoIndex.search(pooling=), k = 10, mean with weights 1 / C and max) per index dtype
(--gallery-dtype, both = the two indexes) with the first NQ // C * C query rows as sets of C, beside the plain search(k = 10)
of the same rows on the same index -- the same scan without the pool step and with C times the selection rows, the
yardstick.  At S1 and S2 the materialised path is timed too: the NQ x NV matrix (mmt_sims_eval, the kernel of
eval_similarity, which itself wants NQ = NV x captions), its mean over the sets in torch, then mmt_rows_topk.  --runs
rounds, every variant once per round, interleaved; median and spread.  Default output profiles/search_pooled_bench.json.

--item-pooled C times the item-pooled search (VideoIndex.search(item_pooling=), k = 10, mean with weights 1 / C and max)
per index dtype (--gallery-dtype, both = the two indexes) with the first NV // C * C stored items as sets of C, beside the
plain search(k = 10) over the same stored items on the same index -- the same scan without the pool step, the yardstick.
What the code predicts is the plain scan's time, times 128 / (128 // C * C) for the idle tile columns, plus the pool step;
the prediction's factor is reported beside the measured ratio.  --runs rounds, every variant once per round, interleaved;
median and spread.  Default output profiles/search_itemset_bench.json.

--fp8 times the fp8-stored index (dtype=torch.float8_e4m3fn) against the bf16-stored one over 262 144 items built in chunks
from the same data: search(k = 10) with 64 queries (one query tile per gallery chunk: the gallery streams from HBM) and with
4 096 (the chunk's query tiles share it in L2), and `add` of 8 192 items into a preallocated index.  --runs rounds, every
variant once per round, interleaved; median and spread; the share of rows whose index lists agree.  Default output
profiles/search_fp8_bench.json.

--rescore times the second stage of a two-stage search over 262 144 items: 4 096 queries, 128 candidates each from the fp8
index's search(k = 128), k = 10, on a bf16 and on a float32 index of the same items -- `rescore`, the composition it
replaces (`target_scores` of the candidates, then `search`'s order as two stable torch sorts) and the index's own full
search(k = 10) for scale; the coarse search(k = 128) is timed beside them.  --runs rounds, every variant once per round,
interleaved; median and spread; the share of rows on which `rescore` and the composition agree bit for bit and on which
`search_refined` returns the fine index's own top 10.  Default output profiles/search_rescore_bench.json.

--after times cursor paging over 262 144 items with 4 096 queries on a bf16 and an fp8 index of the same items: page 2 at
k = 10 (search(after=) from the last column of page 1) beside the plain search(k = 10) of the same build, the plain search at
k = 32, 64 and 128 (how the cost of a page grows with its width) and search_deep(depth = 256) at page = 32, 64 and 128.
--runs rounds, every variant once per round, interleaved; median and spread; whether page 2 and the deep lists are the
slices of the plain k = 128 list they must be.  Default output profiles/search_after_bench.json.

--diverse times the stages of `search_diverse` over 262 144 items with 4 096 queries, shortlist 128, k = 10, on a float32, a
bf16 and an fp8 index: search(k = 128) alone, `rescore`, the Gram launches (mmt_search_pair_scores, in diversify's row
batches), the selection launch (mmt_search_mmr), the whole call, and the torch route to the Gram (index_select of the
shortlist rows + torch.bmm, in row batches under the same _BATCH_BYTES budget); the Gram launch's share of the fp32 or bf16
matrix peak.  --runs rounds, every variant once per round, interleaved; median and spread.  Joins --out (default
profiles/search_bench.json) under 'diverse'.

--neighbours times the gallery self-join over 262 144 items with 4 096 row items, k = 10, on a float32, a bf16 and an fp8
index: `neighbours`, search(k = 10) of 4 096 query rows on the same index (the same tile count), that search with one
exclusion per query (the masked selection and prefilled outputs the join runs with), the torch route
(dequantised rows @ chunk.T with the denominators and topk over chunks under the same _BATCH_BYTES budget) and
`neighbour_range` at per-row thresholds that give 16 hits per row; one full self-join (items=None) per storage as a single
run.  --runs rounds, every variant once per round, interleaved; median and spread.  Joins --out (default
profiles/search_bench.json) under 'neighbours'.

--lse times the softmax over 262 144 items (beta = 20) at NQ = 64 and 4 096 on a float32, a bf16 and an fp8 index: the sum
pass alone (mmt_search_row_expsum with xmax given) and `query_lse` whole, beside search(k = 1) and search(k = 10) on the same
index, and on float32 the route through the matrix (the similarity kernel + torch.logsumexp) with its peak memory.  --runs
rounds, every variant once per round, interleaved; median and spread.  Default output profiles/search_lse_bench.json.

--stream times `search` on an index whose schedule is 'stream' against the same index with 'tile' -- the same build's tile kernels, whose code this
schedule leaves as it was -- with k = 10 over 262 144 items at NQ = 1, 8, 32 and 64 on a float32, a bf16 and an fp8 index:
--runs rounds, the two schedules interleaved, on device events; median and spread, the index bytes over the time (TB/s),
the device time of the scan and the merge kernel separately (one profiled call), at NQ = 1 the wall time of a call with its
synchronisation, and whether the two results are the same bits.  Default output profiles/search_stream_bench.json.

--where times the per-query attribute filter (search(where=)) at 4 096 queries x 262 144 items, k = 10, on a float32, a bf16
and an fp8 index, every pair of variants alternated in one process, --runs rounds on device events; median and spread:
(a) all-zero masks against plain `search` -- the cost of the predicate -- with search(exclude=) at E = 32 beside them;
(b) 16 distinct predicates interleaved over the rows, each passing about 1/16 of randomly placed items, against the route
without where=: 16 subset= searches over gathered row groups, bitmap builds included; (c) one predicate shared by all rows
that passes one contiguous sixteenth of the gallery against subset= of the same items -- the tile skip; (d) one query on
the streaming schedule (bf16, fp8) with and without a predicate.  Default output profiles/search_where_bench.json.

--cells times the cell-probed search (search_probed) over 262 144 items drawn from 1 024 planted clusters (a unit centre plus
unit noise per expert: an inverted file on isotropic data says nothing), k = 10, with 1 024 cells from randomly sampled
centres (cells_from_centres), at NQ = 1, 64 and 4 096 and nprobe = 1, 4, 16 and 64 on a float32, a bf16 and an fp8 index:
`search_probed` against `search` on the same index and, where every row's probed union fits 1 024 items, against `rescore`
on that union; --runs rounds on device events, every variant once per round, interleaved; median and spread.  Beside the
times: the 64 x 128 tile K loops each route executes (the probed scan's from search.probe_plan), whose ratio is the derived
expectation; the regrouping alone (the torch plan), timed on its own; recall@10 of `search_cells` against `search`, per
nprobe -- a property of the quantiser, reported and never a test.  Default output profiles/search_cells_bench.json.

--kmeans times the k-means cells on the data of --cells (262 144 x 7 x 512 from 1 024 planted clusters, 1 024 cells) on a
float32, a bf16 and an fp8 index: (a) the update step, cell_centroids (mmt_search_cell_sums + mmt_search_cell_centroids)
over the cells of the sampled centres, in ms and as a fraction of the HBM peak from the bytes of the labelled rows, their
weights and scales; (b) the same update from the public tensors -- the stored rows dequantised in chunks of 8 192 and
summed with index_add_, whose atomics make two runs differ -- with the peak memory of both; (c) one Lloyd iteration split
into its assignment (the centroid index and neighbours(k=1, source=index)) and its update (cells + cell_centroids);
--runs rounds on device events, every variant once per round, interleaved; median and spread.  (d) train_cells(1 024,
iters=10) once on a host clock, its objective and moved, and recall@10 of search_cells against search at nprobe 1, 4, 16
and 64 with its cells beside the cells of the sampled centres on the same data and queries -- reported, never a test.
Default output profiles/search_kmeans_bench.json.

--kmeans-exact times the exact (integer-sum) k-means update on the data of --kmeans, in one process and interleaved rounds:
the sum_scale pass; cell_centroids with and without exact=True; one Lloyd iteration (assignment, cells, update) each way;
the exact update and iteration on a 4-shard ShardedVideoIndex on the same device; and it checks once that a permuted
re-insertion of the stored rows gives bit-identical exact centroids.  Default output
profiles/search_kmeans_exact_bench.json."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mmt_amd import _lib, metric, ops  # noqa: E402
from mmt_amd.search import ShardedVideoIndex, VideoIndex  # noqa: E402

SHAPES = {'S1': (1000, 1000), 'S2': (4917, 4917), 'S3': (4096, 262144)}
PEAK = 157.3e12
M, D, K = 7, 512, 10


def materialised_kernels(q, qw, g, gw, k):
  nq, nv = q.shape[0], g.shape[0]
  L = _lib.lib()
  ws = torch.empty(L.mmt_sims_eval_workspace_floats(nq, nv, M, D), device=q.device)
  sims = torch.empty(nq, nv, device=q.device)
  _lib.check(L.mmt_sims_eval(ops._p(q), ops._p(g), ops._p(qw), ops._p(gw), nq, nv, M, D, ops._p(ws), ops._p(sims),
                             ops._stream()), 'mmt_sims_eval')
  del ws
  tk = torch.empty(L.mmt_topk_workspace_keys(nq, nv, k), device=q.device, dtype=torch.int64)
  idx = torch.empty(nq, k, device=q.device, dtype=torch.int64)
  _lib.check(L.mmt_rows_topk(ops._p(sims), nv, None, nq, nv, k, ops._p(tk), None, ops._p(idx), ops._stream()),
             'mmt_rows_topk')
  return idx.cpu().numpy()


def materialised_public(q, qw, g, gw, k):
  nv = g.shape[0]
  sims = metric.eval_similarity(g, q.unsqueeze(2), gw, qw.unsqueeze(1))
  return metric.compress_predictions(np.ones((nv, 1), np.float32), sims, topk=k)


def timed(fn, min_seconds):
  fn()
  torch.cuda.synchronize()
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  e0.record()
  fn()
  e1.record()
  torch.cuda.synchronize()
  once = e0.elapsed_time(e1) / 1e3
  iters = max(3, math.ceil(min_seconds / max(once, 1e-6)))
  base = torch.cuda.memory_allocated()
  torch.cuda.reset_peak_memory_stats()
  e0.record()
  for _ in range(iters):
    out = fn()
  e1.record()
  torch.cuda.synchronize()
  return e0.elapsed_time(e1) / 1e3 / iters, iters, torch.cuda.max_memory_allocated() - base, out


def both_dtypes(q, qw, g, gw, flop, a):
  """fp32 and bf16 indexes over the same gallery, timed alternately so drift hits both alike."""
  nv = g.shape[0]
  idx = {'float32': VideoIndex(g, gw)}
  idx['bfloat16'] = VideoIndex.empty(nv, M, D, g.device, dtype=torch.bfloat16)
  for at in range(0, nv, 8192):
    idx['bfloat16'].add(g[at:at + 8192], gw[at:at + 8192])
  ts = {n: [] for n in idx}
  mem = {n: 0 for n in idx}
  out = {}
  for _ in range(a.runs):
    for n in idx:
      t, _, m, out[n] = timed(lambda: idx[n].search(q, qw, k=K), a.min_seconds)
      ts[n].append(t)
      mem[n] = max(mem[n], m)
  row = {}
  for n in idx:
    med = float(np.median(ts[n]))
    row[n] = dict(seconds_median=med, seconds_spread=max(ts[n]) - min(ts[n]), seconds_runs=ts[n], tflops=flop / med / 1e12,
                  index_bytes=idx[n].nbytes, peak_mem_growth_bytes=mem[n])
  row['bf16_speedup'] = row['float32']['seconds_median'] / row['bfloat16']['seconds_median']
  row['margin_seconds'] = max(row['float32']['seconds_spread'], row['bfloat16']['seconds_spread'])
  row['bf16_faster_beyond_margin'] = bool(row['float32']['seconds_median'] - row['bfloat16']['seconds_median'] >
                                          row['margin_seconds'])
  row['bf16_not_slower_beyond_margin'] = bool(row['bfloat16']['seconds_median'] - row['float32']['seconds_median'] <=
                                              row['margin_seconds'])
  row['index_rows_identical'] = float((out['float32'][1] == out['bfloat16'][1]).all(1).float().mean())
  return row


def materialised_ranks(q, qw, g, gw):
  """The eval path of metric.retrieval_metrics: the whole similarity matrix, then the rank of the diagonal."""
  nq, nv = q.shape[0], g.shape[0]
  L = _lib.lib()
  ws = torch.empty(L.mmt_sims_eval_workspace_floats(nq, nv, M, D), device=q.device)
  sims = torch.empty(nq, nv, device=q.device)
  _lib.check(L.mmt_sims_eval(ops._p(q), ops._p(g), ops._p(qw), ops._p(gw), nq, nv, M, D, ops._p(ws), ops._p(sims),
                             ops._stream()), 'mmt_sims_eval')
  del ws
  t2v, v2t, scratch = (torch.empty(n, device=q.device) for n in (nq, nv, nq))
  _lib.check(L.mmt_retrieval_ranks(ops._p(sims), None, nq, nv, ops._p(t2v), ops._p(v2t), ops._p(scratch), ops._stream()),
             'mmt_retrieval_ranks')
  return t2v


def ranks_mode(q, qw, g, gw, flop, a):
  """ranks() with one target per query against search(k = 1), search(k = 10) and the materialised ranking, per index."""
  nq, nv = q.shape[0], g.shape[0]
  tg = torch.arange(nq, device=q.device) % nv   # the item each query was drawn around (main)
  idx = {'float32': VideoIndex(g, gw)}
  idx['bfloat16'] = VideoIndex.empty(nv, M, D, g.device, dtype=torch.bfloat16)
  for at in range(0, nv, 8192):
    idx['bfloat16'].add(g[at:at + 8192], gw[at:at + 8192])
  fns = {}
  for n in idx:
    fns[n + '/ranks'] = lambda n=n: idx[n].ranks(q, qw, tg)
    fns[n + '/search_k1'] = lambda n=n: idx[n].search(q, qw, k=1)
    fns[n + '/search_k10'] = lambda n=n: idx[n].search(q, qw, k=K)
  if nq % nv == 0:
    fns['materialised/ranks'] = lambda: materialised_ranks(q, qw, g, gw)
  ts = {n: [] for n in fns}
  mem = {n: 0 for n in fns}
  out = {}
  for _ in range(a.runs):
    for n, fn in fns.items():
      t, _, m, out[n] = timed(fn, a.min_seconds)
      ts[n].append(t)
      mem[n] = max(mem[n], m)
  row = {}
  for n in fns:
    med = float(np.median(ts[n]))
    row[n] = dict(seconds_median=med, seconds_spread=max(ts[n]) - min(ts[n]), seconds_runs=ts[n], tflops=flop / med / 1e12,
                  peak_mem_growth_bytes=mem[n])
  if 'materialised/ranks' not in fns:
    row['materialised/ranks'] = 'not applicable: mmt_retrieval_ranks wants NQ = NV x captions'
  for n in idx:
    r, k1, k10 = (row['%s/%s' % (n, v)] for v in ('ranks', 'search_k1', 'search_k10'))
    margin = max(r['seconds_spread'], k1['seconds_spread'], k10['seconds_spread'])
    ranks = out[n + '/ranks']
    row[n + '/summary'] = dict(
        ranks_over_search_k1=r['seconds_median'] / k1['seconds_median'],
        ranks_over_search_k10=r['seconds_median'] / k10['seconds_median'], margin_seconds=margin,
        ranks_within_margin_of_search_k1=bool(r['seconds_median'] - k1['seconds_median'] <= margin),
        ranks_slower_than_search_k10_beyond_margin=bool(r['seconds_median'] - k10['seconds_median'] > margin),
        # R@1 two ways: rank 0 from ranks(), and the first item of search(k = 1) being the target (they can differ on ties)
        r_at_1_from_ranks=float((ranks == 0).double().mean()),
        r_at_1_from_search=float((out[n + '/search_k1'][1][:, 0] == tg).double().mean()),
        median_rank=float(ranks.median()), mean_rank=float(ranks.mean()))
    if 'materialised/ranks' in fns:
      row[n + '/summary']['ranks_equal_materialised'] = float((ranks == out['materialised/ranks'].double()).double().mean())
  return row


def subset_mode(q, qw, g, gw, flop, a):
  """Masked search against the unmasked one, per index dtype."""
  nq, nv = q.shape[0], g.shape[0]
  dtypes = ('float32', 'bfloat16') if a.gallery_dtype == 'both' else (a.gallery_dtype,)
  gen = torch.Generator(device=q.device).manual_seed(1)
  fns = {}
  for n in dtypes:
    index = VideoIndex.empty(nv, M, D, g.device, dtype=getattr(torch, n))
    for at in range(0, nv, 8192):
      index.add(g[at:at + 8192], gw[at:at + 8192])
    fns[n + '/unmasked'] = lambda index=index: index.search(q, qw, k=K)
    if a.subset is not None:
      count = max(1, int(round(a.subset * nv)))
      subs = {'all_ones': torch.ones(nv, device=q.device, dtype=torch.bool),
              'contiguous': torch.arange(nv, device=q.device) < count,
              'random': torch.rand(nv, device=q.device, generator=gen) < a.subset}
      for name, mask in subs.items():
        sub = index.subset(mask)
        fns['%s/subset_%s' % (n, name)] = lambda index=index, sub=sub: index.search(q, qw, k=K, subset=sub)
    if a.exclude:
      ex = torch.randint(0, nv, (nq, a.exclude), device=q.device, generator=gen)
      ex[:, 0] = torch.arange(nq, device=q.device) % nv   # the item each query was drawn around (main)
      fns['%s/exclude_%d' % (n, a.exclude)] = lambda index=index, ex=ex: index.search(q, qw, k=K, exclude=ex)
  ts = {n: [] for n in fns}
  for _ in range(a.runs):
    for n, fn in fns.items():
      ts[n].append(timed(fn, a.min_seconds)[0])
  row = {}
  for n in fns:
    med = float(np.median(ts[n]))
    base = float(np.median(ts[n.split('/')[0] + '/unmasked']))
    row[n] = dict(seconds_median=med, seconds_min=min(ts[n]), seconds_max=max(ts[n]), seconds_runs=ts[n],
                  over_unmasked=med / base, tflops_of_the_full_scan=flop / med / 1e12)
  return row


def norm_mode(q, qw, g, gw, flop, a):
  """hub_norm (the lse pass), search(norm=) and the plain search, per index dtype; the bank is the queries."""
  nv = g.shape[0]
  dtypes = ('float32', 'bfloat16') if a.gallery_dtype == 'both' else (a.gallery_dtype,)
  fns = {}
  for n in dtypes:
    index = VideoIndex.empty(nv, M, D, g.device, dtype=getattr(torch, n))
    for at in range(0, nv, 8192):
      index.add(g[at:at + 8192], gw[at:at + 8192])
    norm = index.hub_norm(q, qw, a.norm)
    fns[n + '/search'] = lambda index=index: index.search(q, qw, k=K)
    fns[n + '/search_norm'] = lambda index=index, norm=norm: index.search(q, qw, k=K, norm=norm)
    fns[n + '/col_lse'] = lambda index=index: index.hub_norm(q, qw, a.norm)
  ts = {n: [] for n in fns}
  mem = {n: 0 for n in fns}
  out = {}
  for _ in range(a.runs):
    for n, fn in fns.items():
      t, _, m, out[n] = timed(fn, a.min_seconds)
      ts[n].append(t)
      mem[n] = max(mem[n], m)
  row = {'beta': a.norm, 'bank_rows': q.shape[0]}
  for n in fns:
    med = float(np.median(ts[n]))
    row[n] = dict(seconds_median=med, seconds_spread=max(ts[n]) - min(ts[n]), seconds_runs=ts[n], tflops=flop / med / 1e12,
                  peak_mem_growth_bytes=mem[n])
  for n in dtypes:
    plain = row[n + '/search']['seconds_median']
    moved = (out[n + '/search'][1] != out[n + '/search_norm'][1]).any(1).float().mean()
    row[n + '/summary'] = dict(search_norm_over_search=row[n + '/search_norm']['seconds_median'] / plain,
                               col_lse_over_search=row[n + '/col_lse']['seconds_median'] / plain,
                               rows_reordered_by_the_norm=float(moved))
  return row


def reverse_mode(q, qw, g, gw, flop, a):
  """reverse_search at k = --reverse and k = 32, csls_norm, the lse pass of hub_norm (the yardstick) and the plain search,
  per index dtype; the rows and the bank are the queries."""
  nv = g.shape[0]
  dtypes = ('float32', 'bfloat16') if a.gallery_dtype == 'both' else (a.gallery_dtype,)
  names = ('col_lse', 'reverse_k%d' % a.reverse, 'reverse_k32', 'csls_norm_k%d' % a.reverse, 'search')
  fns = {}
  for n in dtypes:
    index = VideoIndex.empty(nv, M, D, g.device, dtype=getattr(torch, n))
    for at in range(0, nv, 8192):
      index.add(g[at:at + 8192], gw[at:at + 8192])
    calls = (lambda index=index: index.hub_norm(q, qw, 20.0), lambda index=index: index.reverse_search(q, qw, k=a.reverse),
             lambda index=index: index.reverse_search(q, qw, k=32), lambda index=index: index.csls_norm(q, qw, k=a.reverse),
             lambda index=index: index.search(q, qw, k=K))
    fns.update({n + '/' + name: call for name, call in zip(names, calls)})
  ts = {n: [] for n in fns}
  mem = {n: 0 for n in fns}
  for _ in range(a.runs):
    for n, fn in fns.items():
      t, _, m, _ = timed(fn, a.min_seconds)
      ts[n].append(t)
      mem[n] = max(mem[n], m)
  row = {'k': a.reverse, 'rows': q.shape[0]}
  for n in fns:
    med = float(np.median(ts[n]))
    row[n] = dict(seconds_median=med, seconds_spread=max(ts[n]) - min(ts[n]), seconds_runs=ts[n], tflops=flop / med / 1e12,
                  peak_mem_growth_bytes=mem[n])
  for n in dtypes:
    lse = row[n + '/col_lse']['seconds_median']
    row[n + '/summary'] = {name + '_over_col_lse': row[n + '/' + name]['seconds_median'] / lse for name in names[1:]}
  return row


def range_mode(q, qw, g, gw, flop, a):
  """range_search against threshold_counts (T = 1, one scan) and search(k = 10), per index dtype."""
  nv = g.shape[0]
  dtypes = ('float32', 'bfloat16') if a.gallery_dtype == 'both' else (a.gallery_dtype,)
  hits = min(a.range, nv)
  fns = {}
  for n in dtypes:
    index = VideoIndex.empty(nv, M, D, g.device, dtype=getattr(torch, n))
    for at in range(0, nv, 8192):
      index.add(g[at:at + 8192], gw[at:at + 8192])
    thr = index.search(q, qw, k=hits)[0][:, -1].contiguous()
    if not a.counts_only:
      fns[n + '/range_search'] = lambda index=index, thr=thr: index.range_search(q, qw, thr)
    fns[n + '/threshold_counts'] = lambda index=index, thr=thr: index.threshold_counts(q, qw, thr)
    fns[n + '/search_k10'] = lambda index=index: index.search(q, qw, k=K)
  ts = {n: [] for n in fns}
  mem = {n: 0 for n in fns}
  out = {}
  for _ in range(a.runs):
    for n, fn in fns.items():
      t, _, m, out[n] = timed(fn, a.min_seconds)
      ts[n].append(t)
      mem[n] = max(mem[n], m)
  row = {'hits_per_query_at_least': hits}
  for n in fns:
    med = float(np.median(ts[n]))
    row[n] = dict(seconds_median=med, seconds_spread=max(ts[n]) - min(ts[n]), seconds_runs=ts[n],
                  tflops_of_one_scan=flop / med / 1e12, peak_mem_growth_bytes=mem[n])
  if not a.counts_only:
    for n in dtypes:
      r, c, s10 = (row['%s/%s' % (n, v)] for v in ('range_search', 'threshold_counts', 'search_k10'))
      res, (greater, equal) = out[n + '/range_search'], out[n + '/threshold_counts']
      spread = max(r['seconds_spread'], 2 * c['seconds_spread'])
      row[n + '/summary'] = dict(
          total_hits=int(res.offsets[-1]), counts_agree=bool(torch.equal(res.counts, greater.long() + equal.long())),
          range_over_threshold_counts=r['seconds_median'] / c['seconds_median'],
          range_over_search_k10=r['seconds_median'] / s10['seconds_median'],
          seconds_above_two_scans=r['seconds_median'] - 2 * c['seconds_median'], spread_seconds=spread,
          above_two_scans_beyond_spread=bool(r['seconds_median'] - 2 * c['seconds_median'] > spread))
  return row


def groups_mode(q, qw, g, gw, flop, a):
  """search_groups with contiguous and with shuffled groups of a.groups items against search(k = 10), per index dtype."""
  nv = g.shape[0]
  dtypes = ('float32', 'bfloat16') if a.gallery_dtype == 'both' else (a.gallery_dtype,)
  gen = torch.Generator(device=q.device).manual_seed(2)
  every = torch.arange(nv, device=q.device)
  ids = {'contiguous': every // a.groups, 'shuffled': (every // a.groups)[torch.randperm(nv, device=q.device, generator=gen)]}
  fns = {}
  for n in dtypes:
    index = VideoIndex.empty(nv, M, D, g.device, dtype=getattr(torch, n))
    for at in range(0, nv, 8192):
      index.add(g[at:at + 8192], gw[at:at + 8192])
    for name, gids in ids.items():
      grp = index.grouping(gids)
      fns['%s/search_groups_%s' % (n, name)] = lambda index=index, grp=grp: index.search_groups(q, qw, grp, k=K)
    fns[n + '/search_k10'] = lambda index=index: index.search(q, qw, k=K)
  ts = {n: [] for n in fns}
  mem = {n: 0 for n in fns}
  out = {}
  for _ in range(a.runs):
    for n, fn in fns.items():
      t, _, m, out[n] = timed(fn, a.min_seconds)
      ts[n].append(t)
      mem[n] = max(mem[n], m)
  row = {'group_size': a.groups, 'num_groups': -(-nv // a.groups)}
  for n in fns:
    med = float(np.median(ts[n]))
    row[n] = dict(seconds_median=med, seconds_spread=max(ts[n]) - min(ts[n]), seconds_runs=ts[n],
                  tflops_of_the_scan=flop / med / 1e12, peak_mem_growth_bytes=mem[n])
  for n in dtypes:
    plain = row[n + '/search_k10']
    summary = {}
    for name in ids:
      r = row['%s/search_groups_%s' % (n, name)]
      scores, groups, items = out['%s/search_groups_%s' % (n, name)]
      spread = max(r['seconds_spread'], plain['seconds_spread'])
      summary[name] = dict(
          over_search_k10=r['seconds_median'] / plain['seconds_median'], spread_seconds=spread,
          slower_than_search_k10_beyond_spread=bool(r['seconds_median'] - plain['seconds_median'] > spread),
          # the best group is the group of the best item, and every row holds K distinct groups
          top_group_is_that_of_the_top_item=bool(torch.equal(items[:, 0], out[n + '/search_k10'][1][:, 0])),
          rows_with_distinct_groups=float((groups.sort(1).values.diff(dim=1) != 0).all(1).float().mean()),
          groups_are_those_of_the_items=bool(torch.equal(groups, ids[name][items])))
    row[n + '/summary'] = summary
  return row


def materialised_pooled(q, qw, g, gw, c, k):
  """The matrix path of the 'avg' caption mode: every row's scores, their mean over the sets of c rows, then the top k."""
  nq, nv = q.shape[0], g.shape[0]
  L = _lib.lib()
  ws = torch.empty(L.mmt_sims_eval_workspace_floats(nq, nv, M, D), device=q.device)
  sims = torch.empty(nq, nv, device=q.device)
  _lib.check(L.mmt_sims_eval(ops._p(q), ops._p(g), ops._p(qw), ops._p(gw), nq, nv, M, D, ops._p(ws), ops._p(sims),
                             ops._stream()), 'mmt_sims_eval')
  del ws
  avg = sims.view(nq // c, c, nv).mean(1)
  del sims
  tk = torch.empty(L.mmt_topk_workspace_keys(nq // c, nv, k), device=q.device, dtype=torch.int64)
  scores = torch.empty(nq // c, k, device=q.device)
  idx = torch.empty(nq // c, k, device=q.device, dtype=torch.int64)
  _lib.check(L.mmt_rows_topk(ops._p(avg), nv, None, nq // c, nv, k, ops._p(tk), ops._p(scores), ops._p(idx), ops._stream()),
             'mmt_rows_topk')
  return scores, idx


def pooled_mode(q, qw, g, gw, flop, a):
  """search(pooling=) in both modes against the plain search of the same rows, per index dtype; at up to 25 M scores the
  materialised mean as well."""
  nv, c = g.shape[0], a.pooled
  ns = q.shape[0] // c
  q, qw = q[:ns * c].contiguous(), qw[:ns * c].contiguous()
  flop = 2.0 * ns * c * nv * M * D   # the rows in use
  dtypes = ('float32', 'bfloat16') if a.gallery_dtype == 'both' else (a.gallery_dtype,)
  fns = {}
  for n in dtypes:
    index = VideoIndex.empty(nv, M, D, g.device, dtype=getattr(torch, n))
    for at in range(0, nv, 8192):
      index.add(g[at:at + 8192], gw[at:at + 8192])
    for mode in ('mean', 'max'):
      pool = index.pooling(c, ns, mode=mode)
      fns['%s/search_pooled_%s' % (n, mode)] = lambda index=index, pool=pool: index.search(q, qw, k=K, pooling=pool)
    fns[n + '/search_k10'] = lambda index=index: index.search(q, qw, k=K)
  if ns * c * nv <= 25e6:
    fns['materialised_mean'] = lambda: materialised_pooled(q, qw, g, gw, c, K)
  ts = {n: [] for n in fns}
  mem = {n: 0 for n in fns}
  out = {}
  for _ in range(a.runs):
    for n, fn in fns.items():
      t, _, m, out[n] = timed(fn, a.min_seconds)
      ts[n].append(t)
      mem[n] = max(mem[n], m)
  row = {'set_size': c, 'num_sets': ns, 'rows': ns * c, 'flop': flop}
  for n in fns:
    med = float(np.median(ts[n]))
    row[n] = dict(seconds_median=med, seconds_spread=max(ts[n]) - min(ts[n]), seconds_runs=ts[n],
                  tflops_of_the_scan=flop / med / 1e12, peak_mem_growth_bytes=mem[n])
  for n in dtypes:
    plain = row[n + '/search_k10']
    summary = {}
    for mode in ('mean', 'max'):
      r = row['%s/search_pooled_%s' % (n, mode)]
      spread = max(r['seconds_spread'], plain['seconds_spread'])
      summary[mode] = dict(over_search_k10=r['seconds_median'] / plain['seconds_median'], spread_seconds=spread,
                           slower_than_search_k10_beyond_spread=bool(r['seconds_median'] - plain['seconds_median'] > spread))
    # the best item of a set under max is the best item of one of its rows
    top = out[n + '/search_k10'][1][:, 0].view(ns, c)
    summary['max']['top_item_is_a_row_top_item'] = bool((top == out[n + '/search_pooled_max'][1][:, :1]).any(1).all())
    if 'materialised_mean' in row:
      mat = row['materialised_mean']
      summary['mean']['materialised_over_pooled'] = mat['seconds_median'] / row[n + '/search_pooled_mean']['seconds_median']
      summary['mean']['memory_over_materialised'] = (row[n + '/search_pooled_mean']['peak_mem_growth_bytes'] /
                                                     max(1, mat['peak_mem_growth_bytes']))
      if n == 'float32':
        summary['mean']['rows_identical_to_materialised'] = float(
            (out['materialised_mean'][1] == out[n + '/search_pooled_mean'][1]).all(1).float().mean())
        summary['mean']['max_score_difference_to_materialised'] = float(
            (out['materialised_mean'][0] - out[n + '/search_pooled_mean'][0]).abs().max())
    row[n + '/summary'] = summary
  return row


def item_pooled_mode(q, qw, g, gw, flop, a):
  """search(item_pooling=) in both modes against the plain search over the same stored items, per index dtype."""
  c = a.item_pooled
  nt = g.shape[0] // c
  nv = nt * c
  flop = 2.0 * q.shape[0] * nv * M * D   # the items in use
  dtypes = ('float32', 'bfloat16') if a.gallery_dtype == 'both' else (a.gallery_dtype,)
  fns = {}
  for n in dtypes:
    index = VideoIndex.empty(nv, M, D, g.device, dtype=getattr(torch, n))
    for at in range(0, nv, 8192):
      index.add(g[at:min(nv, at + 8192)], gw[at:min(nv, at + 8192)])
    for mode in ('mean', 'max'):
      ip = index.item_pooling(c, mode=mode)
      fns['%s/search_item_pooled_%s' % (n, mode)] = lambda index=index, ip=ip: index.search(q, qw, k=K, item_pooling=ip)
    fns[n + '/search_k10'] = lambda index=index: index.search(q, qw, k=K)
  ts = {n: [] for n in fns}
  mem = {n: 0 for n in fns}
  out = {}
  for _ in range(a.runs):
    for n, fn in fns.items():
      t, _, m, out[n] = timed(fn, a.min_seconds)
      ts[n].append(t)
      mem[n] = max(mem[n], m)
  idle = 128.0 / (128 // c * c)
  row = {'set_size': c, 'num_sets': nt, 'items': nv, 'flop': flop, 'idle_column_factor': idle}
  for n in fns:
    med = float(np.median(ts[n]))
    row[n] = dict(seconds_median=med, seconds_spread=max(ts[n]) - min(ts[n]), seconds_runs=ts[n],
                  tflops_of_the_scan=flop / med / 1e12, peak_mem_growth_bytes=mem[n])
  for n in dtypes:
    plain = row[n + '/search_k10']
    summary = {}
    for mode in ('mean', 'max'):
      r = row['%s/search_item_pooled_%s' % (n, mode)]
      spread = max(r['seconds_spread'], plain['seconds_spread'])
      summary[mode] = dict(over_search_k10=r['seconds_median'] / plain['seconds_median'], spread_seconds=spread,
                           predicted_without_the_pool_step=idle,
                           beyond_prediction_by_more_than_spread=bool(
                               r['seconds_median'] - idle * plain['seconds_median'] > spread))
    # the best set under max is the set of the best item
    summary['max']['top_set_is_that_of_the_top_item'] = bool(
        torch.equal(out[n + '/search_item_pooled_max'][1][:, 0], out[n + '/search_k10'][1][:, 0] // c))
    row[n + '/summary'] = summary
  return row


def fp8_mode(a, dev):
  """The fp8-stored index against the bf16-stored one: search(k = 10) at NQ = 64 (the gallery streams from HBM) and
  NQ = 4096 (L2 serves it) over NV = 262 144 items, and `add` of 8 192 items into a preallocated index."""
  nv, chunk = SHAPES['S3'][1], 8192
  gen = torch.Generator(device=dev).manual_seed(0)
  nrm = lambda x: torch.nn.functional.normalize(x, dim=-1)
  dtypes = {'bfloat16': torch.bfloat16, 'float8_e4m3fn': torch.float8_e4m3fn}
  idx = {n: VideoIndex.empty(nv, M, D, dev, dtype=t) for n, t in dtypes.items()}
  small = {n: VideoIndex.empty(chunk, M, D, dev, dtype=t) for n, t in dtypes.items()}
  for at in range(0, nv, chunk):
    g = nrm(torch.randn(chunk, M, D, device=dev, generator=gen))
    gw = torch.softmax(torch.randn(chunk, M, device=dev, generator=gen), -1)
    for index in idx.values():
      index.add(g, gw)
  q = nrm(torch.randn(4096, M, D, device=dev, generator=gen) + 0.3 * g[torch.arange(4096, device=dev) % chunk])
  qw = torch.softmax(torch.randn(4096, M, device=dev, generator=gen), -1)

  def add(index):
    index.num_items = 0
    return index.add(g, gw)

  fns = {}
  for n in dtypes:
    fns[n + '/search_nq64'] = lambda n=n: idx[n].search(q[:64], qw[:64], k=K)
    fns[n + '/search_nq4096'] = lambda n=n: idx[n].search(q, qw, k=K)
    fns[n + '/add_8192'] = lambda n=n: add(small[n])
  ts = {n: [] for n in fns}
  out = {}
  for _ in range(a.runs):
    for n, fn in fns.items():
      t, _, _, out[n] = timed(fn, a.min_seconds)
      ts[n].append(t)
  row = {'NV': nv, 'index_bytes': {n: idx[n].nbytes for n in idx}}
  for n in fns:
    med = float(np.median(ts[n]))
    row[n] = dict(seconds_median=med, seconds_spread=max(ts[n]) - min(ts[n]), seconds_runs=ts[n])
  for what, rows in (('search_nq64', 64), ('search_nq4096', 4096), ('add_8192', 0)):
    b, f = row['bfloat16/' + what], row['float8_e4m3fn/' + what]
    row[what + '/summary'] = dict(bf16_over_fp8=b['seconds_median'] / f['seconds_median'],
                                  spread_seconds=max(b['seconds_spread'], f['seconds_spread']))
    if rows:
      row[what + '/summary'].update(
          gallery_gbytes_per_second_fp8=nv * M * D / f['seconds_median'] / 1e9,
          gallery_gbytes_per_second_bf16=2 * nv * M * D / b['seconds_median'] / 1e9,
          rows_identical=float((out['bfloat16/' + what][1] == out['float8_e4m3fn/' + what][1]).all(1).float().mean()))
  return row


def kernel_times(fn):
  """Device time of every kernel of one call of fn, by kernel name (torch.profiler), in seconds."""
  from torch.profiler import ProfilerActivity, profile
  fn()
  torch.cuda.synchronize()
  with profile(activities=[ProfilerActivity.CUDA]) as prof:
    fn()
    torch.cuda.synchronize()
  out = {}
  for ev in prof.events():
    if ev.device_type.name != 'CPU' and 'Memcpy' not in ev.name and 'Memset' not in ev.name:
      out[ev.name] = out.get(ev.name, 0.0) + ev.device_time_total / 1e6
  return out


def stream_mode(a, dev):
  """`search` with index.schedule = 'stream' against 'tile' in one session: k = 10 over NV = 262 144 items at NQ = 1, 8, 32 and
  64 on a float32, a bf16 and an fp8 index of the same gallery."""
  import time
  nv, chunk = SHAPES['S3'][1], 8192
  gen = torch.Generator(device=dev).manual_seed(0)
  nrm = lambda x: torch.nn.functional.normalize(x, dim=-1)
  dtypes = {'float32': torch.float32, 'bfloat16': torch.bfloat16, 'float8_e4m3fn': torch.float8_e4m3fn}
  idx = {n: VideoIndex.empty(nv, M, D, dev, dtype=t) for n, t in dtypes.items()}
  for at in range(0, nv, chunk):
    g = nrm(torch.randn(chunk, M, D, device=dev, generator=gen))
    gw = torch.softmax(torch.randn(chunk, M, device=dev, generator=gen), -1)
    for index in idx.values():
      index.add(g, gw)
  q = nrm(torch.randn(64, M, D, device=dev, generator=gen) + 0.3 * g[:64])
  qw = torch.softmax(torch.randn(64, M, device=dev, generator=gen), -1)
  row = {'NV': nv, 'index_bytes': {n: idx[n].nbytes for n in idx}, 'cells': {}}
  for n in dtypes:
    for nq in (1, 8, 32, 64):
      def call(n, nq, sched):
        idx[n].schedule = sched          # a property of the index; a plain assignment, no device work
        return idx[n].search(q[:nq], qw[:nq], k=K)
      fns = {sched: (lambda n=n, nq=nq, sched=sched: call(n, nq, sched)) for sched in ('tile', 'stream')}
      ts, out = {sched: [] for sched in fns}, {}
      for _ in range(a.runs):          # interleaved: drift hits both alike
        for sched, fn in fns.items():
          t, _, _, out[sched] = timed(fn, a.min_seconds)
          ts[sched].append(t)
      cell = {'bit_identical': bool(torch.equal(out['tile'][1], out['stream'][1]) and
                                    torch.equal(out['tile'][0].view(torch.int32), out['stream'][0].view(torch.int32)))}
      for sched, fn in fns.items():
        med = float(np.median(ts[sched]))
        cell[sched] = dict(seconds_median=med, seconds_spread=max(ts[sched]) - min(ts[sched]), seconds_runs=ts[sched],
                           gallery_tbytes_per_second=idx[n].nbytes / med / 1e12)
        try:
          cell[sched]['kernel_seconds'] = kernel_times(fn)
        except Exception as e:  # the profiler is an instrument: a build without it still gives the timings above
          cell[sched]['kernel_seconds'] = 'unavailable: %s' % type(e).__name__
        if nq == 1:                    # a served query: the host's share is part of it
          torch.cuda.synchronize()
          t0 = time.perf_counter()
          for _ in range(50):
            fn()
            torch.cuda.synchronize()
          cell[sched]['wall_seconds_per_call'] = (time.perf_counter() - t0) / 50
      t, st = cell['tile'], cell['stream']
      cell['summary'] = dict(tile_over_stream=t['seconds_median'] / st['seconds_median'],
                             spreads_combined=t['seconds_spread'] + st['seconds_spread'],
                             stream_wins=t['seconds_median'] - st['seconds_median'] > t['seconds_spread'] + st['seconds_spread'])
      row['cells']['%s/nq%d' % (n, nq)] = cell
      print('%s nq=%d: tile %.3f ms, stream %.3f ms (%.2f TB/s), identical %s' % (
          n, nq, 1e3 * t['seconds_median'], 1e3 * st['seconds_median'], st['gallery_tbytes_per_second'], cell['bit_identical']),
          file=sys.stderr)
  return row


def where_mode(a, dev):
  """search(where=) at NQ = 4 096 over NV = 262 144 items, k = 10, on all three storages (module docstring, --where)."""
  nq, nv, chunk, preds = 4096, SHAPES['S3'][1], 8192, 16
  gen = torch.Generator(device=dev).manual_seed(0)
  nrm = lambda x: torch.nn.functional.normalize(x, dim=-1)
  dtypes = {'float32': torch.float32, 'bfloat16': torch.bfloat16, 'float8_e4m3fn': torch.float8_e4m3fn}
  idx = {n: VideoIndex.empty(nv, M, D, dev, dtype=t) for n, t in dtypes.items()}
  for at in range(0, nv, chunk):
    g = nrm(torch.randn(chunk, M, D, device=dev, generator=gen))
    gw = torch.softmax(torch.randn(chunk, M, device=dev, generator=gen), -1)
    for index in idx.values():
      index.add(g, gw)
  q = nrm(torch.randn(nq, M, D, device=dev, generator=gen) + 0.3 * g[torch.arange(nq, device=dev) % chunk])
  qw = torch.softmax(torch.randn(nq, M, device=dev, generator=gen), -1)
  # bits 0 .. 15: one category per item, at random; bit 16: one contiguous sixteenth of the gallery
  category = torch.randint(0, preds, (nv,), device=dev, generator=gen)
  block = torch.zeros(nv, device=dev, dtype=torch.bool)
  block[nv // 2:nv // 2 + nv // 16] = True
  tags = (torch.ones(nv, device=dev, dtype=torch.int64) << category) | (block.long() << 16)
  per_row = torch.ones(nq, device=dev, dtype=torch.int64) << (torch.arange(nq, device=dev) % preds)
  groups = [torch.arange(c, nq, preds, device=dev) for c in range(preds)]
  exclude = torch.randint(0, nv, (nq, 32), device=dev, generator=gen)
  row = {'NQ': nq, 'NV': nv, 'index_bytes': {n: idx[n].nbytes for n in idx}}

  def by_subsets(index):   # the route without where=: per distinct predicate a bitmap, a gather of its rows, a whole scan
    scores = torch.empty(nq, K, device=dev)
    items = torch.empty(nq, K, device=dev, dtype=torch.int64)
    for c, rows in enumerate(groups):
      scores[rows], items[rows] = index.search(q[rows], qw[rows], k=K, subset=index.subset(category == c))
    return scores, items

  same = lambda x, y: bool(torch.equal(x[1], y[1]) and torch.equal(x[0].view(torch.int32), y[0].view(torch.int32)))
  for n, index in idx.items():
    tg = index.tagging(tags)
    zero, mixed, shared = tg.where(), tg.where(all_of=per_row), tg.where(all_of=1 << 16)
    subset = index.subset(block)
    pairs = {
        'a_predicate_cost': {'plain': lambda: index.search(q, qw, k=K), 'where_zero': lambda: index.search(q, qw, k=K, where=zero),
                             'exclude_32': lambda: index.search(q, qw, k=K, exclude=exclude)},
        'b_16_predicates': {'where': lambda: index.search(q, qw, k=K, where=mixed), 'subsets_16': lambda: by_subsets(index)},
        'c_shared_sixteenth': {'where': lambda: index.search(q, qw, k=K, where=shared),
                               'subset': lambda: index.search(q, qw, k=K, subset=subset)},
    }
    if n != 'float32':
      def one(sched, flt):
        index.schedule = sched
        try:
          return index.search(q[:1], qw[:1], k=K, where=flt)
        finally:
          index.schedule = None
      sixteenth = tg.where(all_of=1)
      pairs['d_stream_one_query'] = {'plain': lambda: one('stream', None), 'where': lambda: one('stream', sixteenth),
                                     'where_zero': lambda: one('stream', zero)}
    for what, fns in pairs.items():
      ts, out = {v: [] for v in fns}, {}
      for _ in range(a.runs):          # alternated: drift hits the variants alike
        for v, fn in fns.items():
          t, _, _, out[v] = timed(fn, a.min_seconds)
          ts[v].append(t)
      cell = {v: dict(seconds_median=float(np.median(ts[v])), seconds_spread=max(ts[v]) - min(ts[v]), seconds_runs=ts[v])
              for v in fns}
      first, second = list(fns)[:2]
      cell['summary'] = dict(
          ratio='%s / %s' % (second, first), value=cell[second]['seconds_median'] / cell[first]['seconds_median'],
          difference_seconds=cell[second]['seconds_median'] - cell[first]['seconds_median'],
          spreads_combined=cell[first]['seconds_spread'] + cell[second]['seconds_spread'])
      if what != 'd_stream_one_query':
        cell['summary']['same_bits'] = same(out[first], out[second])
      else:
        cell['summary']['zero_masks_same_bits_as_plain'] = same(out['plain'], out['where_zero'])
      row['%s/%s' % (n, what)] = cell
      print('%s %s: %s' % (n, what, ', '.join('%s %.3f ms (+- %.3f)' % (v, 1e3 * cell[v]['seconds_median'],
                                                                        1e3 * cell[v]['seconds_spread']) for v in fns)),
            file=sys.stderr)
  return row


def clustered_gallery(dev, nv, ncells, nq_all, chunk=8192, shards=0):
  """The data of --cells and --kmeans, from seed 0: nv items drawn from ncells planted clusters (a unit centre plus unit
  noise per expert, renormalised; softmax weights) on a float32, a bf16 and an fp8 index, nq_all queries that are noisy
  copies of stored items, and ncells randomly sampled centre items -> (indexes by dtype name, q, qw, centres).  shards > 0:
  the same chunks also go into a ShardedVideoIndex of that many shards on dev per dtype, returned as a fifth element."""
  gen = torch.Generator(device=dev).manual_seed(0)
  nrm = lambda x: torch.nn.functional.normalize(x, dim=-1)
  noise = lambda n: torch.randn(n, M, D, device=dev, generator=gen) / math.sqrt(D)
  planted = nrm(torch.randn(ncells, M, D, device=dev, generator=gen))
  dtypes = {'float32': torch.float32, 'bfloat16': torch.bfloat16, 'float8_e4m3fn': torch.float8_e4m3fn}
  idx = {n: VideoIndex.empty(nv, M, D, dev, dtype=t) for n, t in dtypes.items()}
  sharded = {n: ShardedVideoIndex.empty(nv, M, D, [dev] * shards, dtype=t) for n, t in dtypes.items()} if shards else {}
  source = torch.randint(0, nv, (nq_all,), device=dev, generator=gen)       # a query is a noisy copy of a stored item
  q = torch.empty(nq_all, M, D, device=dev)
  for at in range(0, nv, chunk):
    g = nrm(planted[torch.randint(0, ncells, (chunk,), device=dev, generator=gen)] + noise(chunk))
    gw = torch.softmax(torch.randn(chunk, M, device=dev, generator=gen), -1)
    for index in list(idx.values()) + list(sharded.values()):
      index.add(g, gw)
    mine = (source >= at) & (source < at + chunk)
    q[mine] = g[source[mine] - at]
  q = nrm(q + noise(nq_all))
  qw = torch.softmax(torch.randn(nq_all, M, device=dev, generator=gen), -1)
  centres = torch.randperm(nv, device=dev, generator=gen)[:ncells]
  return (idx, q, qw, centres, sharded) if shards else (idx, q, qw, centres)


HBM_PEAK = 8.0e12  # bytes/s, HBM3E specification


def kmeans_mode(a, dev):
  """The k-means update, one Lloyd iteration and the recall of trained cells (module docstring, --kmeans)."""
  import time
  from mmt_amd import search
  nv, ncells, nq_all, chunk = SHAPES['S3'][1], 1024, 4096, 8192
  idx, q, qw, centres = clustered_gallery(dev, nv, ncells, nq_all)
  row = {'NV': nv, 'num_cells': ncells, 'sum_piece': search.SUM_PIECE, 'sum_slab': search.SUM_SLAB,
         'hbm_peak_bytes_per_second': HBM_PEAK, 'index_bytes': {n: idx[n].nbytes for n in idx},
         'not_measured': ['kernel times from a profiler trace: the update is timed as one call on device events',
                          'a training sample smaller than the gallery (items=)', 'num_cells other than 1 024']}

  def recall(index, cells, exact):
    out = {}
    for p in (1, 4, 16, 64):
      got = index.search_cells(q, qw, cells, nprobe=p, k=K)[1]
      out['nprobe%d' % p] = float(((got.unsqueeze(2) == exact.unsqueeze(1)).any(2).float().sum(1) / K).mean())
    return out

  for n, index in idx.items():
    sampled = index.cells_from_centres(centres)
    ids = torch.empty(nv, device=dev, dtype=torch.int64)
    ids[sampled.items] = torch.repeat_interleave(torch.arange(ncells, device=dev), sampled.sizes)
    labelled = int(sampled.items.shape[0])
    row_bytes = labelled * (M * D * index.folded.element_size() + M * 4 + (4 if index.scales is not None else 0))
    out = (torch.zeros(ncells, M, D, device=dev), torch.zeros(ncells, M, device=dev))

    def update_torch():
      sums, wsums = torch.zeros(ncells, M * D, device=dev), torch.zeros(ncells, M, device=dev)
      for at in range(0, nv, chunk):
        rows = index.folded[at:at + chunk].to(torch.float32)
        if index.scales is not None:
          rows = rows * index.scales[at:at + chunk, None]
        sums.index_add_(0, ids[at:at + chunk], rows)
        wsums.index_add_(0, ids[at:at + chunk], index.weights[at:at + chunk])
      counts = torch.bincount(ids, minlength=ncells).clamp(min=1)
      return torch.nn.functional.normalize(sums.view(ncells, M, D), dim=-1), wsums / counts[:, None]

    def assignment():
      return VideoIndex(out[0], out[1], dtype=index.dtype).neighbours(k=1, source=index)

    fns = {'update': lambda: index.cell_centroids(sampled, out=out), 'update_torch_index_add': update_torch,
           'assignment': assignment, 'cells_build': lambda: index.cells(ids, ncells),
           'cells_build_and_update': lambda: index.cell_centroids(index.cells(ids, ncells), out=out)}
    ts, peaks, res = {v: [] for v in fns}, {v: 0 for v in fns}, {}
    for _ in range(a.runs):            # interleaved: drift hits the variants alike
      for v, fn in fns.items():
        t, _, peak, res[v] = timed(fn, a.min_seconds)
        ts[v].append(t)
        peaks[v] = max(peaks[v], peak)
    cell = {v: dict(seconds_median=float(np.median(ts[v])), seconds_spread=max(ts[v]) - min(ts[v]), seconds_runs=ts[v],
                    peak_mem_growth_bytes=int(peaks[v])) for v in fns}
    up, ref = cell['update'], cell['update_torch_index_add']
    up.update(bytes_read=row_bytes, bytes_per_second=row_bytes / up['seconds_median'],
              fraction_of_hbm_peak=row_bytes / up['seconds_median'] / HBM_PEAK)
    again = index.cell_centroids(sampled)
    diff = (res['update_torch_index_add'][0] - again[0]).abs().max()
    cell['summary'] = dict(
        torch_over_update_seconds=ref['seconds_median'] / up['seconds_median'],
        torch_over_update_peak_bytes=ref['peak_mem_growth_bytes'] / max(1, up['peak_mem_growth_bytes']),
        iteration_seconds=cell['assignment']['seconds_median'] + cell['cells_build_and_update']['seconds_median'],
        update_share_of_iteration=cell['cells_build_and_update']['seconds_median'] /
        (cell['assignment']['seconds_median'] + cell['cells_build_and_update']['seconds_median']),
        update_is_bit_identical_across_calls=bool(torch.equal(again[0].view(torch.int32), res['update'][0].view(torch.int32))),
        max_abs_difference_to_the_torch_route=float(diff))
    row[n + '/times'] = cell
    exact = index.search(q, qw, k=K)[1]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    quantiser = index.train_cells(ncells, iters=10)
    trained = quantiser.assign(index)
    torch.cuda.synchronize()
    sizes = trained.sizes.cpu().numpy()
    row[n + '/train_cells'] = dict(seconds_host_clock=time.perf_counter() - t0, iterations=quantiser.iterations,
                                   objective=quantiser.objective.cpu().tolist(), moved=quantiser.moved.cpu().tolist(),
                                   size_min=int(sizes.min()), size_median=float(np.median(sizes)), size_max=int(sizes.max()))
    row[n + '/recall_at_10'] = {'trained': recall(index, trained, exact), 'sampled_centres': recall(index, sampled, exact)}
    print('%s: update %.3f ms (%.0f%% of HBM peak), torch %.3f ms, assignment %.3f ms; recall trained %s sampled %s' % (
        n, 1e3 * up['seconds_median'], 100 * up['fraction_of_hbm_peak'], 1e3 * ref['seconds_median'],
        1e3 * cell['assignment']['seconds_median'], row[n + '/recall_at_10']['trained'],
        row[n + '/recall_at_10']['sampled_centres']), file=sys.stderr)
  return row


def kmeans_exact_mode(a, dev):
  """The exact k-means update against the float update (module docstring, --kmeans-exact)."""
  from mmt_amd import search
  nv, ncells, shards = SHAPES['S3'][1], 1024, 4
  idx, _, _, centres, sharded_idx = clustered_gallery(dev, nv, ncells, 64, shards=shards)
  row = {'NV': nv, 'num_cells': ncells, 'shards': shards, 'sum_piece': search.SUM_PIECE, 'sum_slab': search.SUM_SLAB,
         'hbm_peak_bytes_per_second': HBM_PEAK,
         'not_measured': ['kernel times from a profiler trace: every variant is timed as calls on device events',
                          'shards on more than one physical device', 'num_cells other than 1 024',
                          'a training sample smaller than the gallery (items=)']}
  same = lambda x, y: bool(all(torch.equal(u.view(torch.int32), v.view(torch.int32)) for u, v in zip(x, y)))
  pair = lambda: (torch.zeros(ncells, M, D, device=dev), torch.zeros(ncells, M, device=dev))
  for n, index in idx.items():
    sharded = sharded_idx[n]
    sampled = index.cells_from_centres(centres)
    ids = torch.empty(nv, device=dev, dtype=torch.int64)
    ids[sampled.items] = torch.repeat_interleave(torch.arange(ncells, device=dev), sampled.sizes)
    scells = sharded.cells(ids, ncells)
    labelled = int(sampled.items.shape[0])
    row_bytes = labelled * (M * D * index.folded.element_size() + M * 4 + (4 if index.scales is not None else 0))
    start, out, tmp = index.cell_centroids(sampled, exact=True), pair(), pair()

    def forget(ix):
      ix._sum_scale = None
      return ix.sum_scale()

    def iteration(ix, how):
      if ix is index:
        _, best = VideoIndex(start[0], start[1], dtype=index.dtype).neighbours(k=1, source=index)
      else:
        _, best = ix._assign(start[0], start[1], None)
      return ix.cell_centroids(ix.cells(best[:, 0].contiguous(), ncells), out=tmp, **how)

    fns = {'sum_scale': lambda: forget(index),
           'update_float': lambda: index.cell_centroids(sampled, out=out),
           'update_exact': lambda: index.cell_centroids(sampled, out=out, exact=True),
           'iteration_float': lambda: iteration(index, {}),
           'iteration_exact': lambda: iteration(index, {'exact': True}),
           'sharded_sum_scale': lambda: forget(sharded),
           'sharded_update_exact': lambda: sharded.cell_centroids(scells, out=out, exact=True),
           'sharded_iteration_exact': lambda: iteration(sharded, {'exact': True})}
    ts, peaks = {v: [] for v in fns}, {v: 0 for v in fns}
    for _ in range(a.runs):            # interleaved: drift hits the variants alike
      for v, fn in fns.items():
        t, _, peak, _ = timed(fn, a.min_seconds)
        ts[v].append(t)
        peaks[v] = max(peaks[v], peak)
    cell = {v: dict(seconds_median=float(np.median(ts[v])), seconds_spread=max(ts[v]) - min(ts[v]), seconds_runs=ts[v],
                    peak_mem_growth_bytes=int(peaks[v])) for v in fns}
    for v in ('update_float', 'update_exact', 'sharded_update_exact'):
      cell[v].update(bytes_read=row_bytes, bytes_per_second=row_bytes / cell[v]['seconds_median'],
                     fraction_of_hbm_peak=row_bytes / cell[v]['seconds_median'] / HBM_PEAK)
    med = lambda v: cell[v]['seconds_median']
    # a permuted re-insertion, once: the stored rows moved as they are, the labels alike
    perm = torch.randperm(nv, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    again = VideoIndex.empty(nv, M, D, dev, dtype=index.dtype)
    again.folded.view(torch.uint8).copy_(index.folded.view(torch.uint8)[perm])
    again.weights.copy_(index.weights[perm])
    if index.scales is not None:
      again.scales.copy_(index.scales[perm])
    again.num_items = nv
    moved = again.cell_centroids(again.cells(ids[perm], ncells), exact=True)
    moved_float = again.cell_centroids(again.cells(ids[perm], ncells))
    del again
    cell['summary'] = dict(
        scale=repr(index.sum_scale()),
        exact_over_float_update_seconds=med('update_exact') / med('update_float'),
        exact_over_float_iteration_seconds=med('iteration_exact') / med('iteration_float'),
        iteration_spreads_combined=cell['iteration_exact']['seconds_spread'] + cell['iteration_float']['seconds_spread'],
        sharded_over_single_exact_update_seconds=med('sharded_update_exact') / med('update_exact'),
        sharded_over_single_exact_iteration_seconds=med('sharded_iteration_exact') / med('iteration_exact'),
        sum_scale_share_of_exact_iteration=med('sum_scale') / med('iteration_exact'),
        sharded_centroids_same_bits_as_single=same(sharded.cell_centroids(scells, exact=True), start),
        sharded_scale_equals_single=sharded.sum_scale() == index.sum_scale(),
        permuted_reinsertion_same_bits_exact=same(moved, start),
        permuted_reinsertion_same_bits_float=same(moved_float, index.cell_centroids(sampled)),
        max_abs_difference_exact_to_float_centroids=float((start[0] - index.cell_centroids(sampled)[0]).abs().max()))
    row[n + '/times'] = cell
    print('%s: sum_scale %.3f ms; update float %.3f ms, exact %.3f ms (%.2f TB/s); iteration float %.3f ms, exact %.3f ms '
          '(x %.3f); %d shards: update %.3f ms, iteration %.3f ms; permuted same bits: %s' % (
              n, 1e3 * med('sum_scale'), 1e3 * med('update_float'), 1e3 * med('update_exact'),
              cell['update_exact']['bytes_per_second'] / 1e12, 1e3 * med('iteration_float'), 1e3 * med('iteration_exact'),
              cell['summary']['exact_over_float_iteration_seconds'], shards, 1e3 * med('sharded_update_exact'),
              1e3 * med('sharded_iteration_exact'), cell['summary']['permuted_reinsertion_same_bits_exact']), file=sys.stderr)
  return row


def cells_mode(a, dev):
  """search_probed against search and rescore on planted clusters (module docstring, --cells)."""
  from mmt_amd import search
  nv, ncells, nq_all = SHAPES['S3'][1], 1024, 4096
  idx, q, qw, centres = clustered_gallery(dev, nv, ncells, nq_all)
  row = {'NV': nv, 'num_cells': ncells, 'cell_piece': search.CELL_PIECE, 'index_bytes': {n: idx[n].nbytes for n in idx}}
  same = lambda x, y: bool(torch.equal(x[1], y[1]) and torch.equal(x[0].view(torch.int32), y[0].view(torch.int32)))
  for n, index in idx.items():
    cells = index.cells_from_centres(centres)
    sizes = cells.sizes.cpu().numpy()
    offsets, items = cells.offsets.cpu().numpy(), cells.items.cpu().numpy()
    row[n + '/cells'] = dict(size_min=int(sizes.min()), size_median=float(np.median(sizes)), size_max=int(sizes.max()),
                             max_pieces=cells.max_pieces)
    exact = index.search(q, qw, k=K)[1]
    probes = {p: cells.probes(q, qw, p) for p in (1, 4, 16, 64)}
    for p, pr in probes.items():                                            # recall@10 at 4 096 queries
      got = index.search_probed(q, qw, cells, pr, k=K)[1]
      hit = (got.unsqueeze(2) == exact.unsqueeze(1)).any(2).float().sum(1) / K
      row['%s/recall_at_10/nprobe%d' % (n, p)] = float(hit.mean())
    for nq in (1, 64, nq_all):
      qq, ww = q[:nq], qw[:nq]
      fns = {'search': lambda: index.search(qq, ww, k=K)}
      tiles = {'search': -(-nq // 64) * -(-nv // 128)}
      notes = {}
      for p, pr in probes.items():
        mine = pr[:nq].contiguous()
        fns['probed_%d' % p] = lambda mine=mine: index.search_probed(qq, ww, cells, mine, k=K)
        fns['plan_%d' % p] = lambda mine=mine: search._probe_plan(mine, cells.offsets, cells.max_pieces)
        host = mine.cpu().numpy()
        work = search.probe_plan(host, offsets)[2]
        tiles['probed_%d' % p] = int((-(-(work[:, 3] - work[:, 2]) // 128)).sum())
        union = [np.concatenate([items[offsets[c]:offsets[c + 1]] for c in np.unique(r[r >= 0])] or [items[:0]]) for r in host]
        widest = max(len(u) for u in union)
        if widest <= search.MAX_C:                                          # the route a caller has today for such rows
          cand = np.full((nq, widest), -1, np.int64)
          for r, u in enumerate(union):
            cand[r, :len(u)] = u
          cand = torch.from_numpy(cand).to(dev)
          fns['rescore_%d' % p] = lambda cand=cand: index.rescore(qq, ww, cand, k=K)
          tiles['rescore_%d' % p] = -(-nq // 64) * -(-64 * widest // 128)
          notes['rescore_%d' % p] = 'C = %d' % widest
        else:
          notes['rescore_%d' % p] = 'not run: the widest probed union holds %d items' % widest
      ts, out = {v: [] for v in fns}, {}
      for _ in range(a.runs):          # interleaved: drift hits the variants alike
        for v, fn in fns.items():
          t, _, _, out[v] = timed(fn, a.min_seconds)
          ts[v].append(t)
      cell = {v: dict(seconds_median=float(np.median(ts[v])), seconds_spread=max(ts[v]) - min(ts[v]), seconds_runs=ts[v])
              for v in fns}
      for v, t in tiles.items():
        cell[v]['tile_k_loops'] = t
      base = cell['search']
      summary = {'notes': notes}
      for p in probes:
        c = cell['probed_%d' % p]
        s = dict(search_over_probed_seconds=base['seconds_median'] / c['seconds_median'],
                 search_over_probed_tiles=base['tile_k_loops'] / max(1, c['tile_k_loops']),
                 plan_share_of_probed=cell['plan_%d' % p]['seconds_median'] / c['seconds_median'],
                 spreads_combined=base['seconds_spread'] + c['seconds_spread'],
                 probed_faster_beyond_spread=bool(base['seconds_median'] - c['seconds_median'] >
                                                  base['seconds_spread'] + c['seconds_spread']))
        if 'rescore_%d' % p in cell:
          r = cell['rescore_%d' % p]
          padded = tuple(torch.cat([t, torch.full((nq, K - t.shape[1]), v, device=dev, dtype=t.dtype)], 1) if t.shape[1] < K else t
                         for t, v in zip(out['rescore_%d' % p], (float('-inf'), -1)))
          s.update(rescore_over_probed_seconds=r['seconds_median'] / c['seconds_median'],
                   rescore_over_probed_tiles=r['tile_k_loops'] / max(1, c['tile_k_loops']),
                   same_bits_as_rescore=same(out['probed_%d' % p], padded))
        summary['nprobe%d' % p] = s
      cell['summary'] = summary
      row['%s/nq%d' % (n, nq)] = cell
      print('%s nq=%d: search %.3f ms; %s' % (n, nq, 1e3 * base['seconds_median'], ', '.join(
          'nprobe %d: %.3f ms (plan %.3f), tiles %d' % (p, 1e3 * cell['probed_%d' % p]['seconds_median'],
                                                        1e3 * cell['plan_%d' % p]['seconds_median'],
                                                        cell['probed_%d' % p]['tile_k_loops']) for p in probes)), file=sys.stderr)
  return row


def composed_rescore(index, q, qw, cand, k):
  """What `rescore` replaces, from the public calls: `target_scores` of the candidates (MAX_T columns per launch), then
  `search`'s order in torch -- two stable sorts, by item and then by descending score with -0 as +0 and none last.
  Candidates that repeat would need a de-duplication on top; a list from `search` has none."""
  s = index.target_scores(q, qw, cand)
  s = torch.where(cand < 0, torch.full_like(s, float('-inf')), s) + 0.0
  by_item = torch.argsort(cand, dim=1, stable=True)
  perm = torch.gather(by_item, 1, torch.argsort(torch.gather(s, 1, by_item), dim=1, descending=True, stable=True))[:, :k]
  return torch.gather(s, 1, perm), torch.gather(cand, 1, perm)


def rescore_mode(a, dev):
  """The second stage of a two-stage search over NV = 262 144 items, NQ = 4 096, C = 128 candidates per query from the fp8
  index's search(k = 128), k = 10, on a bf16 and on a float32 fine index: `rescore`, the composition it replaces
  (composed_rescore) and the fine index's full search(k = 10) for scale."""
  nq, nv = SHAPES['S3']
  chunk, c = 8192, 128
  gen = torch.Generator(device=dev).manual_seed(0)
  nrm = lambda x: torch.nn.functional.normalize(x, dim=-1)
  dtypes = {'bfloat16': torch.bfloat16, 'float32': torch.float32}
  coarse = VideoIndex.empty(nv, M, D, dev, dtype=torch.float8_e4m3fn)
  fine = {n: VideoIndex.empty(nv, M, D, dev, dtype=t) for n, t in dtypes.items()}
  for at in range(0, nv, chunk):
    g = nrm(torch.randn(chunk, M, D, device=dev, generator=gen))
    gw = torch.softmax(torch.randn(chunk, M, device=dev, generator=gen), -1)
    for index in [coarse] + list(fine.values()):
      index.add(g, gw)
  q = nrm(torch.randn(nq, M, D, device=dev, generator=gen) + 0.3 * g[torch.arange(nq, device=dev) % chunk])
  qw = torch.softmax(torch.randn(nq, M, device=dev, generator=gen), -1)
  cand = coarse.search(q, qw, k=c)[1]
  fns = {'float8_e4m3fn/search_k128': lambda: coarse.search(q, qw, k=c)}
  for n in dtypes:
    fns[n + '/rescore'] = lambda n=n: fine[n].rescore(q, qw, cand, k=K)
    fns[n + '/target_scores_torch_sort'] = lambda n=n: composed_rescore(fine[n], q, qw, cand, K)
    fns[n + '/search_k10'] = lambda n=n: fine[n].search(q, qw, k=K)
  ts = {n: [] for n in fns}
  out = {}
  for _ in range(a.runs):
    for n, fn in fns.items():
      t, _, _, out[n] = timed(fn, a.min_seconds)
      ts[n].append(t)
  row = {'NQ': nq, 'NV': nv, 'C': c}
  for n in fns:
    row[n] = dict(seconds_median=float(np.median(ts[n])), seconds_spread=max(ts[n]) - min(ts[n]), seconds_runs=ts[n])
  same = lambda x, y: float(((x[1] == y[1]) & (x[0].view(torch.int32) == y[0].view(torch.int32))).all(1).float().mean())
  for n in dtypes:
    r, b, s = (row[n + '/' + what] for what in ('rescore', 'target_scores_torch_sort', 'search_k10'))
    refined = fine[n].search_refined(q, qw, coarse, k=K, shortlist=c)
    row[n + '/summary'] = dict(
        composition_over_rescore=b['seconds_median'] / r['seconds_median'],
        search_over_rescore=s['seconds_median'] / r['seconds_median'],
        spread_seconds=max(r['seconds_spread'], b['seconds_spread']),
        rows_identical_to_composition=same(out[n + '/rescore'], out[n + '/target_scores_torch_sort']),
        refined_rows_with_the_fine_top10=float((refined[1] == out[n + '/search_k10'][1]).all(1).float().mean()))
  return row


def after_mode(a, dev):
  """Cursor paging over NV = 262 144 items, NQ = 4 096, on a bf16 and an fp8 index: page 2 at k = 10 against the plain
  search(k = 10), the plain search at k = 32 / 64 / 128, and search_deep(256) at page 32 / 64 / 128."""
  nq, nv = SHAPES['S3']
  chunk, depth = 8192, 256
  gen = torch.Generator(device=dev).manual_seed(0)
  nrm = lambda x: torch.nn.functional.normalize(x, dim=-1)
  dtypes = {'bfloat16': torch.bfloat16, 'float8_e4m3fn': torch.float8_e4m3fn}
  idx = {n: VideoIndex.empty(nv, M, D, dev, dtype=t) for n, t in dtypes.items()}
  for at in range(0, nv, chunk):
    g = nrm(torch.randn(chunk, M, D, device=dev, generator=gen))
    gw = torch.softmax(torch.randn(chunk, M, device=dev, generator=gen), -1)
    for index in idx.values():
      index.add(g, gw)
  q = nrm(torch.randn(nq, M, D, device=dev, generator=gen) + 0.3 * g[torch.arange(nq, device=dev) % chunk])
  qw = torch.softmax(torch.randn(nq, M, device=dev, generator=gen), -1)
  fns, cursor = {}, {}
  for n in dtypes:
    page1 = idx[n].search(q, qw, k=K)
    cursor[n] = (page1[0][:, -1].contiguous(), page1[1][:, -1].contiguous())
    fns[n + '/search_k10'] = lambda n=n: idx[n].search(q, qw, k=K)
    fns[n + '/page2_k10'] = lambda n=n: idx[n].search(q, qw, k=K, after=cursor[n])
    for k in (32, 64, 128):
      fns[n + '/search_k%d' % k] = lambda n=n, k=k: idx[n].search(q, qw, k=k)
    for page in (32, 64, 128):
      fns[n + '/deep256_page%d' % page] = lambda n=n, page=page: idx[n].search_deep(q, qw, depth, page=page)
  ts = {n: [] for n in fns}
  out = {}
  for r in range(a.runs):
    for n, fn in fns.items():
      t, _, _, out[n] = timed(fn, a.min_seconds)
      ts[n].append(t)
    print('round %d of %d' % (r + 1, a.runs), file=sys.stderr, flush=True)
  row = {'NQ': nq, 'NV': nv, 'depth': depth}
  for n in fns:
    row[n] = dict(seconds_median=float(np.median(ts[n])), seconds_spread=max(ts[n]) - min(ts[n]), seconds_runs=ts[n])
  same = lambda x, y: float(((x[1] == y[1]) & (x[0].view(torch.int32) == y[0].view(torch.int32))).all(1).float().mean())
  for n in dtypes:
    top = out[n + '/search_k128']
    deep = idx[n].search_deep(q, qw, 128, page=32)
    plain, page2 = row[n + '/search_k10'], row[n + '/page2_k10']
    row[n + '/summary'] = dict(
        page2_over_plain=page2['seconds_median'] / plain['seconds_median'],
        spread_seconds=max(plain['seconds_spread'], page2['seconds_spread']),
        page2_rows_identical_to_the_k128_list=same(out[n + '/page2_k10'], (top[0][:, K:2 * K], top[1][:, K:2 * K])),
        deep128_rows_identical_to_the_k128_list=same(deep, top),
        deep256_rows_identical_across_pages=min(same(out[n + '/deep256_page32'], out[n + '/deep256_page%d' % p])
                                                 for p in (64, 128)),
        seconds_per_page_column={'k%d' % k: row[n + '/search_k%d' % k]['seconds_median'] / k for k in (10, 32, 64, 128)})
  return row


PEAK_BF16 = 2.5e15  # dense bf16 matrix peak


def torch_gram(index, items, budget):
  """The torch route to the Gram of `pair_scores`: index_select of the shortlist rows, widened to a dtype torch.bmm takes
  (an fp8 row to bf16, exactly), one batched matmul, the same for the weights, and the division -- in row batches whose
  gathered operand stays within `budget` bytes.  -> float32 [R, C, C]."""
  r, c = items.shape
  wide = torch.float32 if index.dtype is torch.float32 else torch.bfloat16
  kk = index.folded.shape[1]
  rows = max(1, budget // (c * kk * (4 if wide is torch.float32 else 2)))
  out = torch.empty(r, c, c, device=items.device, dtype=torch.float32)
  stored = index.folded.view(torch.uint8)
  for r0 in range(0, r, rows):
    at = items[r0:r0 + rows].clamp(min=0).reshape(-1)
    f = stored.index_select(0, at).view(index.dtype).to(wide).view(-1, c, kk)
    w = index.weights.index_select(0, at).view(-1, c, index.num_experts)
    num = torch.bmm(f, f.transpose(1, 2)).float()
    if index.scales is not None:
      s = index.scales.index_select(0, at).view(-1, c)
      num = num * (s[:, :, None] * s[:, None, :])
    den = torch.bmm(w, w.transpose(1, 2))
    out[r0:r0 + rows] = num / torch.where(den == 0, torch.full_like(den, 1e-5), den)
  return out


def diverse_mode(a, dev):
  """The stages of `search_diverse` over NV = 262 144 items, NQ = 4 096, shortlist C = 128, k = 10, per storage dtype:
  search(k = 128) alone, `rescore` of that list, the Gram launches (mmt_search_pair_scores in diversify's row batches), the
  selection launch (mmt_search_mmr) and the torch route to the same Gram under the same byte budget."""
  from mmt_amd import search
  nq, nv = SHAPES['S3']
  chunk, c = 8192, 128
  gen = torch.Generator(device=dev).manual_seed(0)
  nrm = lambda x: torch.nn.functional.normalize(x, dim=-1)
  dtypes = {'float32': torch.float32, 'bfloat16': torch.bfloat16, 'float8_e4m3fn': torch.float8_e4m3fn}
  idx = {n: VideoIndex.empty(nv, M, D, dev, dtype=t) for n, t in dtypes.items()}
  for at in range(0, nv, chunk):
    g = nrm(torch.randn(chunk, M, D, device=dev, generator=gen))
    gw = torch.softmax(torch.randn(chunk, M, device=dev, generator=gen), -1)
    for index in idx.values():
      index.add(g, gw)
  q = nrm(torch.randn(nq, M, D, device=dev, generator=gen) + 0.3 * g[torch.arange(nq, device=dev) % chunk])
  qw = torch.softmax(torch.randn(nq, M, device=dev, generator=gen), -1)
  L = _lib.lib()

  def gram(index, items):
    for r0, r1 in index._list_batches(nq, c):
      sims = torch.empty(r1 - r0, c, c, device=dev, dtype=torch.float32)
      index._pair_scores(items[r0:r1], sims)
    return sims

  def mmr(rel, items, sims):
    outs = (torch.empty(nq, K, device=dev), torch.empty(nq, K, device=dev, dtype=torch.int64), torch.empty(nq, K, device=dev))
    _lib.check(L.mmt_search_mmr(ops._p(items), ops._p(rel), ops._p(sims), nq, c, K, 0.5, 0.5, *[ops._p(o) for o in outs],
                                ops._stream()), 'mmt_search_mmr')
    return outs

  fns, kept = {}, {}
  for n, index in idx.items():
    cand = index.search(q, qw, k=c)[1]
    rel, items = index.rescore(q, qw, cand)
    kept[n] = (rel, items, index.pair_scores(items))
    fns[n + '/search_k128'] = lambda index=index: index.search(q, qw, k=c)
    fns[n + '/rescore'] = lambda index=index, cand=cand: index.rescore(q, qw, cand)
    fns[n + '/gram'] = lambda index=index, items=items: gram(index, items)
    fns[n + '/mmr'] = lambda n=n: mmr(*kept[n])
    fns[n + '/gram_torch'] = lambda index=index, items=items: torch_gram(index, items, search._BATCH_BYTES)
    fns[n + '/search_diverse'] = lambda index=index: index.search_diverse(q, qw, k=K, lam=0.5, shortlist=c)
  ts = {n: [] for n in fns}
  for r in range(a.runs):
    for n, fn in fns.items():
      t, _, _, _ = timed(fn, a.min_seconds)
      ts[n].append(t)
    print('round %d of %d' % (r + 1, a.runs), file=sys.stderr, flush=True)
  flop = 2.0 * nq * c * c * M * D
  row = {'NQ': nq, 'NV': nv, 'C': c, 'gram_flop': flop, 'torch_gather_bytes_fp32': nq * c * M * D * 4}
  for n in fns:
    row[n] = dict(seconds_median=float(np.median(ts[n])), seconds_spread=max(ts[n]) - min(ts[n]), seconds_runs=ts[n])
  for n, index in idx.items():
    ours, theirs = row[n + '/gram'], row[n + '/gram_torch']
    peak = PEAK if n == 'float32' else PEAK_BF16
    ref = torch_gram(index, kept[n][1], search._BATCH_BYTES)
    live = ~torch.isnan(kept[n][2])
    row[n + '/summary'] = dict(
        torch_over_gram=theirs['seconds_median'] / ours['seconds_median'],
        spread_seconds=max(ours['seconds_spread'], theirs['seconds_spread']),
        gram_tflops=flop / ours['seconds_median'] / 1e12, gram_fraction_of_matrix_peak=flop / ours['seconds_median'] / peak,
        matrix_peak_flops=peak,
        max_abs_difference_to_torch=float((kept[n][2] - ref)[live].abs().max()),
        stages_over_search_k128={s: row[n + '/' + s]['seconds_median'] / row[n + '/search_k128']['seconds_median']
                                 for s in ('rescore', 'gram', 'mmr')})
  return row


def torch_neighbours(index, items, k, budget):
  """The torch route to `neighbours`: the rows dequantised to a dtype torch.matmul takes (an fp8 row to bf16, exactly, with
  its scale applied to the product), f_rows @ f_chunk.T with the denominators, the self pair masked by number, and topk
  over chunks of columns whose [R, chunk] fp32 scores stay within `budget` bytes, merged by a running topk.  ->
  (scores float32 [R, k], indices int64 [R, k])."""
  wide = torch.float32 if index.dtype is torch.float32 else torch.bfloat16
  r, nv, dev = items.shape[0], index.num_items, items.device
  f_rows, w_rows = index.folded.index_select(0, items).to(wide), index.weights.index_select(0, items)
  s_rows = None if index.scales is None else index.scales.index_select(0, items)
  cols = max(1, budget // (4 * r))
  best_s = torch.full((r, k), float('-inf'), device=dev)
  best_i = torch.full((r, k), -1, device=dev, dtype=torch.int64)
  for c0 in range(0, nv, cols):
    c1 = min(nv, c0 + cols)
    num = (f_rows @ index.folded[c0:c1].to(wide).T).float()
    if s_rows is not None:
      num = num * (s_rows[:, None] * index.scales[c0:c1][None, :])
    den = w_rows @ index.weights[c0:c1].T
    sims = num / torch.where(den == 0, torch.full_like(den, 1e-5), den)
    sims.masked_fill_(torch.arange(c0, c1, device=dev)[None, :] == items[:, None], float('-inf'))
    s, i = sims.topk(min(k, c1 - c0), dim=1)
    s, i = torch.cat([best_s, s], 1), torch.cat([best_i, i + c0], 1)
    best_s, at = s.topk(k, dim=1)
    best_i = i.gather(1, at)
  return best_s, best_i


def neighbours_mode(a, dev):
  """The gallery self-join over NV = 262 144 items with R = 4 096 row items, k = 10, per storage dtype: `neighbours`, beside
  search(k = 10) of 4 096 query rows on the same index (the same tile count; on bf16 and fp8 it issues two MFMAs per fragment
  where the join issues one) and the torch route under the same byte budget; `neighbour_range` at per-row thresholds that
  give 16 hits per row; and one full self-join (items=None), a single run."""
  from mmt_amd import search
  nq, nv = SHAPES['S3']
  chunk, hits = 8192, 16
  gen = torch.Generator(device=dev).manual_seed(0)
  nrm = lambda x: torch.nn.functional.normalize(x, dim=-1)
  dtypes = {'float32': torch.float32, 'bfloat16': torch.bfloat16, 'float8_e4m3fn': torch.float8_e4m3fn}
  idx = {n: VideoIndex.empty(nv, M, D, dev, dtype=t) for n, t in dtypes.items()}
  for at in range(0, nv, chunk):
    g = nrm(torch.randn(chunk, M, D, device=dev, generator=gen))
    gw = torch.softmax(torch.randn(chunk, M, device=dev, generator=gen), -1)
    for index in idx.values():
      index.add(g, gw)
  q = nrm(torch.randn(nq, M, D, device=dev, generator=gen) + 0.3 * g[torch.arange(nq, device=dev) % chunk])
  qw = torch.softmax(torch.randn(nq, M, device=dev, generator=gen), -1)
  items = torch.arange(nq, device=dev) * (nv // nq)       # 4 096 rows spread over the gallery
  fns, thr = {}, {}
  for n, index in idx.items():
    thr[n] = index.neighbours(k=hits, items=items)[0][:, hits - 1].contiguous()   # the 16th best sim of every row
    fns[n + '/neighbours'] = lambda index=index: index.neighbours(k=K, items=items)
    fns[n + '/search_k10'] = lambda index=index: index.search(q, qw, k=K)
    # the same search with one exclusion per query: the masked selection and prefilled outputs the join runs with
    fns[n + '/search_k10_exclude1'] = lambda index=index: index.search(q, qw, k=K, exclude=items[:, None])
    fns[n + '/neighbours_torch'] = lambda index=index: torch_neighbours(index, items, K, search._BATCH_BYTES)
    fns[n + '/neighbour_range'] = lambda index=index, n=n: index.neighbour_range(thr[n], items=items)
  ts = {n: [] for n in fns}
  for r in range(a.runs):
    for n, fn in fns.items():
      t, _, _, _ = timed(fn, a.min_seconds)
      ts[n].append(t)
    print('round %d of %d' % (r + 1, a.runs), file=sys.stderr, flush=True)
  flop = 2.0 * nq * nv * M * D
  row = {'R': nq, 'NQ': nq, 'NV': nv, 'flop': flop, 'range_hits_per_row': hits}
  for n in fns:
    row[n] = dict(seconds_median=float(np.median(ts[n])), seconds_spread=max(ts[n]) - min(ts[n]), seconds_runs=ts[n])
  for n, index in idx.items():
    ours, scan, theirs = row[n + '/neighbours'], row[n + '/search_k10'], row[n + '/neighbours_torch']
    peak = PEAK if n == 'float32' else PEAK_BF16
    mine, ref = index.neighbours(k=K, items=items), torch_neighbours(index, items, K, search._BATCH_BYTES)
    ranged = index.neighbour_range(thr[n], items=items)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    full = index.neighbours(k=K)
    e1.record()
    torch.cuda.synchronize()
    row[n + '/summary'] = dict(
        neighbours_over_search=ours['seconds_median'] / scan['seconds_median'],
        spread_seconds_of_the_two=max(ours['seconds_spread'], scan['seconds_spread']),
        torch_over_neighbours=theirs['seconds_median'] / ours['seconds_median'],
        neighbours_tflops=flop / ours['seconds_median'] / 1e12,
        neighbours_fraction_of_matrix_peak=flop / ours['seconds_median'] / peak, matrix_peak_flops=peak,
        top1_agreement_with_torch=float((mine[1][:, 0] == ref[1][:, 0]).float().mean()),
        max_abs_score_difference_to_torch=float((mine[0] - ref[0]).abs().max()),
        range_hits_total=int(ranged.offsets[-1]),
        full_self_join_seconds_single_run=e0.elapsed_time(e1) / 1e3,
        full_self_join_rows_equal_the_batch=bool(torch.equal(full[1][items], mine[1])))
    del full
  return row


def materialised_lse(q, qw, g, gw, beta):
  """The route through the matrix: the kernel behind metric.eval_similarity (which wants NQ = NV * C) on NQ x NV, scaled in
  place, then torch.logsumexp along the rows."""
  nq, nv = q.shape[0], g.shape[0]
  L = _lib.lib()
  ws = torch.empty(L.mmt_sims_eval_workspace_floats(nq, nv, M, D), device=q.device)
  sims = torch.empty(nq, nv, device=q.device)
  _lib.check(L.mmt_sims_eval(ops._p(q), ops._p(g), ops._p(qw), ops._p(gw), nq, nv, M, D, ops._p(ws), ops._p(sims),
                             ops._stream()), 'mmt_sims_eval')
  del ws
  return torch.logsumexp(sims.mul_(beta), 1)


def lse_mode(a, dev):
  """The softmax over NV = 262 144 items, beta = 20, at NQ = 64 and 4 096, per storage dtype: the sum pass alone
  (mmt_search_row_expsum with xmax given), `query_lse` whole (top-1 scan + sum pass + the float64 closing step), beside
  search(k = 1) and search(k = 10) on the same index in the same session; on float32 also the materialised route,
  metric.eval_similarity + torch.logsumexp over the NQ x NV matrix, with its peak memory."""
  from mmt_amd.search import _Scan, lse_bits
  nv, chunk, beta = SHAPES['S3'][1], 8192, 20.0
  gen = torch.Generator(device=dev).manual_seed(0)
  nrm = lambda x: torch.nn.functional.normalize(x, dim=-1)
  dtypes = {'float32': torch.float32, 'bfloat16': torch.bfloat16, 'float8_e4m3fn': torch.float8_e4m3fn}
  idx = {n: VideoIndex.empty(nv, M, D, dev, dtype=t) for n, t in dtypes.items()}
  g_all, gw_all = [], []
  for at in range(0, nv, chunk):
    g = nrm(torch.randn(chunk, M, D, device=dev, generator=gen))
    gw = torch.softmax(torch.randn(chunk, M, device=dev, generator=gen), -1)
    for index in idx.values():
      index.add(g, gw)
    g_all.append(g)
    gw_all.append(gw)
  g_all, gw_all = torch.cat(g_all), torch.cat(gw_all)
  bits = lse_bits(nv)
  row = {'NV': nv, 'beta': beta, 'bits': bits}
  for nq in (64, 4096):
    q = nrm(torch.randn(nq, M, D, device=dev, generator=gen) + 0.3 * g[torch.arange(nq, device=dev) % chunk])
    qw = torch.softmax(torch.randn(nq, M, device=dev, generator=gen), -1)
    fns, peaks = {}, {}
    for n, index in idx.items():
      xmax = index.search(q, qw, k=1)[0][:, 0] * beta
      fns[n + '/sum_pass'] = lambda index=index, xmax=xmax: index._row_expsum(q, qw, beta, xmax, bits, _Scan())
      fns[n + '/query_lse'] = lambda index=index: index.query_lse(q, qw, beta).lse
      fns[n + '/search_k1'] = lambda index=index: index.search(q, qw, k=1)
      fns[n + '/search_k10'] = lambda index=index: index.search(q, qw, k=K)
    if not a.skip_materialised:
      fns['float32/materialised_logsumexp'] = lambda: materialised_lse(q, qw, g_all, gw_all, beta)
    ts = {n: [] for n in fns}
    for r in range(a.runs):
      for n, fn in fns.items():
        t, _, peak, _ = timed(fn, a.min_seconds)
        ts[n].append(t)
        peaks[n] = max(peaks.get(n, 0), peak)
      print('NQ %d: round %d of %d' % (nq, r + 1, a.runs), file=sys.stderr, flush=True)
    res = {'NQ': nq, 'flop': 2.0 * nq * nv * M * D}
    for n in fns:
      res[n] = dict(seconds_median=float(np.median(ts[n])), seconds_spread=max(ts[n]) - min(ts[n]), seconds_runs=ts[n],
                    peak_bytes=int(peaks[n]))
    for n, index in idx.items():
      s, whole, k1, k10 = (res[n + '/' + v]['seconds_median'] for v in ('sum_pass', 'query_lse', 'search_k1', 'search_k10'))
      summary = dict(sum_pass_over_search_k1=s / k1, sum_pass_over_search_k10=s / k10, query_lse_over_search_k1=whole / k1,
                     spread_seconds_of_the_three=max(res[n + '/' + v]['seconds_spread'] for v in ('sum_pass', 'search_k1', 'search_k10')),
                     sum_pass_tflops=res['flop'] / s / 1e12)
      if n == 'float32' and not a.skip_materialised:
        mat = res['float32/materialised_logsumexp']
        lse, ref = index.query_lse(q, qw, beta).lse, fns['float32/materialised_logsumexp']()
        summary.update(materialised_over_query_lse=mat['seconds_median'] / whole, materialised_peak_bytes=mat['peak_bytes'],
                       query_lse_peak_bytes=res[n + '/query_lse']['peak_bytes'],
                       max_abs_difference_to_materialised=float((lse - ref).abs().max()))
        del ref
      res[n + '/summary'] = summary
    row['NQ%d' % nq] = res
  return row


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--lse', action='store_true', help='time the softmax over 262 144 items (beta = 20) at NQ = 64 and 4 096 on '
                  'a float32, a bf16 and an fp8 index: the sum pass alone and query_lse whole against search(k = 1) and '
                  'search(k = 10), and on float32 eval_similarity + torch.logsumexp with its peak memory (no other mode flag)')
  ap.add_argument('--neighbours', action='store_true', help='time the gallery self-join (R = 4 096 rows, k = 10) on a float32, '
                  'a bf16 and an fp8 index of 262 144 items against search(k = 10) of 4 096 queries and the torch route, '
                  'neighbour_range at 16 hits per row, and one full self-join (no other mode flag)')
  ap.add_argument('--diverse', action='store_true', help='time the stages of search_diverse (shortlist 128, k = 10) on a '
                  'float32, a bf16 and an fp8 index of 262 144 items: search(k = 128), rescore, the Gram launches, the '
                  'selection launch and the torch route to the Gram (no other mode flag)')
  ap.add_argument('--after', action='store_true', help='time cursor paging on a bf16 and an fp8 index of 262 144 items: page 2 '
                  'at k = 10 against search(k = 10), the plain search at k = 32 / 64 / 128 and search_deep(256) at page '
                  '32 / 64 / 128 (no other mode flag)')
  ap.add_argument('--rescore', action='store_true', help='time rescore (C = 128 candidates from the fp8 index, k = 10) on a '
                  'bf16 and a float32 index of 262 144 items against target_scores + a torch sort and the full '
                  'search(k = 10) (no other mode flag)')
  ap.add_argument('--fp8', action='store_true', help='time the fp8-stored index against the bf16-stored one: search(k = 10) '
                  'at NQ = 64 and 4096 over 262 144 items, and add of 8 192 items (no other mode flag)')
  ap.add_argument('--stream', action='store_true', help="time search with index.schedule = 'stream' against 'tile' (k = 10) at "
                  'NQ = 1, 8, 32, 64 on a float32, a bf16 and an fp8 index of 262 144 items; no other mode')
  ap.add_argument('--where', action='store_true', help='time search(where=) at 4 096 x 262 144, k = 10, on a float32, a bf16 and '
                  'an fp8 index: zero masks against plain search, 16 predicates against 16 subset searches, a shared '
                  'contiguous predicate against the same subset, one streamed query with and without a predicate')
  ap.add_argument('--cells', action='store_true', help='time search_probed at 1, 64 and 4 096 queries x 262 144 clustered items '
                  'in 1 024 cells, nprobe = 1, 4, 16, 64, k = 10, on a float32, a bf16 and an fp8 index, against search and '
                  'rescore; tile counts and recall@10 beside the times')
  ap.add_argument('--kmeans', action='store_true', help='time the k-means update (cell_centroids) at 262 144 clustered items '
                  'in 1 024 cells on a float32, a bf16 and an fp8 index against dequantise + index_add_, one Lloyd iteration '
                  'split into assignment and update, and recall@10 of search_cells with train_cells(1 024, iters=10)')
  ap.add_argument('--kmeans-exact', action='store_true', help='time the exact k-means update (cell_centroids(exact=True)) '
                  'against the float update on the data of --kmeans: sum_scale, the update, one Lloyd iteration each way, '
                  'the same on a 4-shard ShardedVideoIndex on one device, and a permuted re-insertion checked once')
  ap.add_argument('--shapes', default='S1,S2,S3')
  ap.add_argument('--out', default=None)
  ap.add_argument('--min-seconds', type=float, default=0.5)
  ap.add_argument('--skip-materialised', action='store_true', help='fused path only (kernel-trace runs)')
  ap.add_argument('--gallery-dtype', choices=('float32', 'bfloat16', 'both'), default='float32')
  ap.add_argument('--runs', type=int, default=5, help='timed runs per index with --gallery-dtype both')
  ap.add_argument('--ranks', action='store_true', help='time VideoIndex.ranks (T = 1) against search(k = 1) and the '
                  'materialised ranking, both gallery dtypes')
  ap.add_argument('--subset', type=float, default=None, metavar='FRACTION', help='time search(subset=) with an all-ones, '
                  'a contiguous and a random subset of this fraction of the items against the unmasked search')
  ap.add_argument('--exclude', type=int, default=0, metavar='E', help='time search(exclude=) with E (1..32) exclusions per '
                  'query against the unmasked search')
  ap.add_argument('--shards', type=int, default=0, metavar='N', help='time a ShardedVideoIndex of N (1..32) shards over '
                  'the visible devices, cycling, in place of the single index (default mode only)')
  ap.add_argument('--norm', type=float, default=None, metavar='BETA', help='time hub_norm (the lse pass, bank = the queries) '
                  'and search(norm=) against the plain search')
  ap.add_argument('--reverse', type=int, default=0, metavar='K', help='time reverse_search (k = K and k = 32) and csls_norm '
                  '(k = K), rows and bank = the queries, against the lse pass of hub_norm and search(k = 10)')
  ap.add_argument('--range', type=int, default=0, metavar='HITS', help='time range_search with per-query thresholds at the '
                  'HITS-th best score (1..128) against threshold_counts (T = 1) and search(k = 10)')
  ap.add_argument('--counts-only', action='store_true', help='with --range: the two yardsticks alone (runs on a build '
                  'without range_search)')
  ap.add_argument('--groups', type=int, default=0, metavar='SIZE', help='time search_groups(k = 10) with contiguous and with '
                  'shuffled groups of SIZE items against search(k = 10)')
  ap.add_argument('--pooled', type=int, default=0, metavar='C', help='time search(pooling=) with sets of C (1..64) rows, mean '
                  'and max, against search(k = 10) of the same rows and, at S1 / S2, the materialised mean')
  ap.add_argument('--item-pooled', type=int, default=0, metavar='C', help='time search(item_pooling=) with stored sets of C '
                  '(1..128) items, mean and max, against search(k = 10) over the same items')
  ap.add_argument('--baseline-json', nargs='+', default=[], help='with --norm: default-mode results of another build; '
                  'with --range: --range --counts-only results of another build')
  ap.add_argument('--same-build-json', nargs='+', default=[], help='with --norm: default-mode results of this build')
  a = ap.parse_args()
  masked = a.subset is not None or a.exclude > 0
  if a.subset is not None and not 0 < a.subset <= 1:
    raise SystemExit('--subset wants a fraction in (0, 1]')
  if not 0 <= a.exclude <= 32:
    raise SystemExit('--exclude wants 0..32')
  if not 0 <= a.shards <= 32 or a.shards and (masked or a.ranks or a.gallery_dtype == 'both'):
    raise SystemExit('--shards wants 1..32 and the default mode (no --ranks, --subset, --exclude, --gallery-dtype both)')
  if a.norm is not None and (masked or a.ranks or a.shards or not 0 < a.norm < math.inf):
    raise SystemExit('--norm wants 0 < BETA < inf and no --ranks, --subset, --exclude, --shards')
  if not 0 <= a.reverse <= 32 or a.reverse and (masked or a.ranks or a.shards or a.norm is not None or a.range or a.groups or
                                                a.pooled or a.item_pooled):
    raise SystemExit('--reverse wants K in 1..32 and no other mode')
  if a.reverse and a.out is None:
    a.out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'search_bench.json')
  if not 0 <= a.range <= 128 or a.range and (masked or a.ranks or a.shards or a.norm is not None):
    raise SystemExit('--range wants 1..128 and no --ranks, --subset, --exclude, --shards, --norm')
  if a.groups < 0 or a.groups and (masked or a.ranks or a.shards or a.norm is not None or a.range):
    raise SystemExit('--groups wants SIZE >= 1 and no --ranks, --subset, --exclude, --shards, --norm, --range')
  if a.groups and a.out is None:
    a.out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'search_groups_bench.json')
  if not 0 <= a.pooled <= 64 or a.pooled and (masked or a.ranks or a.shards or a.norm is not None or a.range or a.groups):
    raise SystemExit('--pooled wants C in 1..64 and no --ranks, --subset, --exclude, --shards, --norm, --range, --groups')
  if a.pooled and a.out is None:
    a.out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'search_pooled_bench.json')
  if not 0 <= a.item_pooled <= 128 or a.item_pooled and (masked or a.ranks or a.shards or a.norm is not None or a.range or
                                                         a.groups or a.pooled):
    raise SystemExit('--item-pooled wants C in 1..128 and no --ranks, --subset, --exclude, --shards, --norm, --range, '
                     '--groups, --pooled')
  if a.item_pooled and a.out is None:
    a.out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'search_itemset_bench.json')
  if a.lse and (masked or a.ranks or a.shards or a.norm is not None or a.reverse or a.range or a.groups or a.pooled or
                a.item_pooled or a.neighbours or a.diverse or a.after or a.rescore or a.fp8):
    raise SystemExit('--lse wants no other mode')
  if a.counts_only and not a.range:
    raise SystemExit('--counts-only goes with --range')
  if a.range and a.out is None and not a.counts_only:
    a.out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'search_range_bench.json')
  if a.norm is not None and a.out is None:
    a.out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'search_bench.json')
  if masked and a.out is None:
    a.out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'search_subset_bench.json')
  if a.ranks and a.out is None:
    a.out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'search_ranks_bench.json')
  if not torch.cuda.is_available():
    raise SystemExit('search_bench needs the GPU')
  dev = torch.device('cuda', 0)
  if a.kmeans_exact:
    res = {'M': M, 'd': D, 'device': torch.cuda.get_device_name(0), 'mode': 'kmeans-exact', 'runs': a.runs,
           'min_seconds': a.min_seconds}
    res.update(kmeans_exact_mode(a, dev))
    out = a.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
                                'search_kmeans_exact_bench.json')
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'w') as f:
      json.dump(res, f, indent=1)
    print(json.dumps(res))
    return
  if a.kmeans:
    res = {'M': M, 'd': D, 'k': K, 'device': torch.cuda.get_device_name(0), 'mode': 'kmeans', 'runs': a.runs,
           'min_seconds': a.min_seconds}
    res.update(kmeans_mode(a, dev))
    out = a.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
                                'search_kmeans_bench.json')
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'w') as f:
      json.dump(res, f, indent=1)
    print(json.dumps(res))
    return
  if a.cells:
    res = {'M': M, 'd': D, 'k': K, 'device': torch.cuda.get_device_name(0), 'mode': 'cells', 'runs': a.runs,
           'min_seconds': a.min_seconds}
    res.update(cells_mode(a, dev))
    out = a.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
                                'search_cells_bench.json')
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'w') as f:
      json.dump(res, f, indent=1)
    print(json.dumps(res))
    return
  if a.where:
    res = {'M': M, 'd': D, 'k': K, 'device': torch.cuda.get_device_name(0), 'mode': 'where', 'runs': a.runs,
           'min_seconds': a.min_seconds}
    res.update(where_mode(a, dev))
    out = a.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
                                'search_where_bench.json')
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'w') as f:
      json.dump(res, f, indent=1)
    print(json.dumps(res))
    return
  if a.lse:
    res = {'M': M, 'd': D, 'k': K, 'device': torch.cuda.get_device_name(0), 'mode': 'lse', 'runs': a.runs,
           'min_seconds': a.min_seconds}
    res.update(lse_mode(a, dev))
    out = a.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
                                'search_lse_bench.json')
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'w') as f:
      json.dump(res, f, indent=1)
    print(json.dumps(res))
    return
  if a.neighbours:
    res = {'M': M, 'd': D, 'k': K, 'device': torch.cuda.get_device_name(0), 'mode': 'neighbours', 'runs': a.runs,
           'min_seconds': a.min_seconds}
    res.update(neighbours_mode(a, dev))
    out = a.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'search_bench.json')
    kept = {}
    if os.path.exists(out):  # joins the results of that file, as --diverse does
      with open(out) as f:
        kept = json.load(f)
    kept['neighbours'] = res
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'w') as f:
      json.dump(kept, f, indent=1)
    print(json.dumps(res))
    return
  if a.diverse:
    res = {'M': M, 'd': D, 'k': K, 'device': torch.cuda.get_device_name(0), 'mode': 'diverse', 'runs': a.runs,
           'min_seconds': a.min_seconds}
    res.update(diverse_mode(a, dev))
    out = a.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'search_bench.json')
    kept = {}
    if os.path.exists(out):  # joins the default-mode results of that file, as --norm and --reverse do
      with open(out) as f:
        kept = json.load(f)
    kept['diverse'] = res
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'w') as f:
      json.dump(kept, f, indent=1)
    print(json.dumps(res))
    return
  if a.after:
    res = {'M': M, 'd': D, 'k': K, 'device': torch.cuda.get_device_name(0), 'mode': 'after', 'runs': a.runs,
           'min_seconds': a.min_seconds}
    res.update(after_mode(a, dev))
    out = a.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
                                'search_after_bench.json')
    with open(out, 'w') as f:
      json.dump(res, f, indent=1)
    print(json.dumps(res))
    return
  if a.rescore:
    res = {'M': M, 'd': D, 'k': K, 'device': torch.cuda.get_device_name(0), 'mode': 'rescore', 'runs': a.runs,
           'min_seconds': a.min_seconds}
    res.update(rescore_mode(a, dev))
    out = a.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
                                'search_rescore_bench.json')
    with open(out, 'w') as f:
      json.dump(res, f, indent=1)
    print(json.dumps(res))
    return
  if a.stream:
    res = {'M': M, 'd': D, 'k': K, 'device': torch.cuda.get_device_name(0), 'mode': 'stream', 'runs': a.runs,
           'min_seconds': a.min_seconds}
    res.update(stream_mode(a, dev))
    out = a.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
                                'search_stream_bench.json')
    with open(out, 'w') as f:
      json.dump(res, f, indent=1)
    print(json.dumps(res))
    return
  if a.fp8:
    res = {'M': M, 'd': D, 'k': K, 'device': torch.cuda.get_device_name(0), 'mode': 'fp8', 'runs': a.runs,
           'min_seconds': a.min_seconds}
    res.update(fp8_mode(a, dev))
    out = a.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
                                'search_fp8_bench.json')
    with open(out, 'w') as f:
      json.dump(res, f, indent=1)
    print(json.dumps(res))
    return
  res = {'M': M, 'd': D, 'k': K, 'peak_fp32_matrix_flops': PEAK, 'device': torch.cuda.get_device_name(0), 'shapes': {}}
  if a.gallery_dtype != 'float32':  # the default invocation keeps its JSON layout
    res['gallery_dtype'] = a.gallery_dtype
  if a.ranks:
    res.update(mode='ranks', T=1, runs=a.runs, min_seconds=a.min_seconds)
  if a.norm is not None:
    res.update(mode='norm', gallery_dtype=a.gallery_dtype, runs=a.runs, min_seconds=a.min_seconds)
    for key, files in (('baseline_plain_search', a.baseline_json), ('same_build_plain_search', a.same_build_json)):
      runs = {}
      for path in files:
        with open(path) as f:
          for name, row in json.load(f)['shapes'].items():
            runs.setdefault(name, []).append(row['fused']['seconds'])
      if runs:
        res[key] = {name: dict(seconds_runs=v, seconds_median=float(np.median(v)), seconds_spread=max(v) - min(v))
                    for name, v in runs.items()}
  if a.reverse:
    res.update(mode='reverse', gallery_dtype=a.gallery_dtype, runs=a.runs, min_seconds=a.min_seconds)
  if a.range:
    res.update(mode='range', hits=a.range, counts_only=a.counts_only, gallery_dtype=a.gallery_dtype, runs=a.runs,
               min_seconds=a.min_seconds)
    if a.baseline_json:
      res['baseline'] = []
      for path in a.baseline_json:
        with open(path) as f:
          other = json.load(f)
        res['baseline'].append({name: {n: v for n, v in row.items() if isinstance(v, dict) and 'seconds_median' in v}
                                for name, row in other['shapes'].items()})
  if a.groups:
    res.update(mode='groups', group_size=a.groups, gallery_dtype=a.gallery_dtype, runs=a.runs, min_seconds=a.min_seconds)
  if a.pooled:
    res.update(mode='pooled', set_size=a.pooled, gallery_dtype=a.gallery_dtype, runs=a.runs, min_seconds=a.min_seconds)
  if a.item_pooled:
    res.update(mode='item_pooled', set_size=a.item_pooled, gallery_dtype=a.gallery_dtype, runs=a.runs,
               min_seconds=a.min_seconds)
  if masked:
    res.update(mode='subset', subset_fraction=a.subset, exclude=a.exclude, runs=a.runs, min_seconds=a.min_seconds)
  for name in a.shapes.split(','):
    nq, nv = SHAPES[name]
    gen = torch.Generator(device=dev).manual_seed(0)
    nrm = lambda x: torch.nn.functional.normalize(x, dim=-1)
    g = nrm(torch.randn(nv, M, D, device=dev, generator=gen))
    gw = torch.softmax(torch.randn(nv, M, device=dev, generator=gen), -1)
    q = nrm(torch.randn(nq, M, D, device=dev, generator=gen) + 0.3 * g[torch.arange(nq, device=dev) % nv])
    qw = torch.softmax(torch.randn(nq, M, device=dev, generator=gen), -1)
    flop = 2.0 * nq * nv * M * D
    row = {'NQ': nq, 'NV': nv, 'flop': flop}
    if (masked or a.ranks or a.norm is not None or a.range or a.groups or a.pooled or a.item_pooled or a.reverse or
        a.gallery_dtype == 'both'):
      mode = (reverse_mode if a.reverse else norm_mode if a.norm is not None else range_mode if a.range else groups_mode if a.groups else
              pooled_mode if a.pooled else item_pooled_mode if a.item_pooled else
              subset_mode if masked else ranks_mode if a.ranks else both_dtypes)
      row.update(mode(q, qw, g, gw, flop, a))
      res['shapes'][name] = row
      print(name, json.dumps(row), flush=True)
      del g, gw, q, qw
      torch.cuda.empty_cache()
      continue
    if a.shards:
      devices = [torch.device('cuda', i % torch.cuda.device_count()) for i in range(a.shards)]
      index = ShardedVideoIndex.empty(nv, M, D, devices, dtype=getattr(torch, a.gallery_dtype))
      for at in range(0, nv, 8192):
        index.add(g[at:at + 8192], gw[at:at + 8192])
      row.update(shards=a.shards, devices=[str(dev) for dev in devices], shard_sizes=index.shard_sizes)
    else:
      index = VideoIndex(g, gw, dtype=getattr(torch, a.gallery_dtype))
    t, it, mem, (s, i) = timed(lambda: index.search(q, qw, k=K), a.min_seconds)
    row['fused'] = dict(seconds=t, iters=it, peak_mem_growth_bytes=mem, tflops=flop / t / 1e12,
                        fraction_of_peak=flop / t / PEAK)
    fused_idx = i.cpu().numpy()
    del index
    if not a.skip_materialised:
      fn = materialised_public if nq == nv else materialised_kernels
      t, it, mem, idx = timed(lambda: fn(q, qw, g, gw, K), a.min_seconds)
      row['materialised'] = dict(path='eval_similarity + compress_predictions' if nq == nv else
                                 'mmt_sims_eval + mmt_rows_topk', seconds=t, iters=it, peak_mem_growth_bytes=mem,
                                 tflops=flop / t / 1e12, fraction_of_peak=flop / t / PEAK)
      row['fused_speedup'] = row['materialised']['seconds'] / row['fused']['seconds']
      row['memory_ratio'] = row['fused']['peak_mem_growth_bytes'] / max(1, row['materialised']['peak_mem_growth_bytes'])
      row['rows_identical'] = float((fused_idx == idx).all(1).mean())
    res['shapes'][name] = row
    print(name, json.dumps(row), flush=True)
    del g, gw, q, qw
    torch.cuda.empty_cache()
  if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    if (a.norm is not None or a.reverse) and os.path.exists(a.out):  # joins the default-mode results of that file
      with open(a.out) as f:
        kept = json.load(f)
      kept['reverse' if a.reverse else 'norm'] = res
      res = kept
    with open(a.out, 'w') as f:
      json.dump(res, f, indent=1)
  print(json.dumps(res))


if __name__ == '__main__':
  main()
