"""Where the time of an item-pooled search goes when its tiles are no whole number of rounds of blocks: plain search(k = 10)
over --items stored items beside search(item_pooling=) with sets of --set-size over --sets sets, 4 096 queries, M = 7,
d = 512, both gallery dtypes, on prefixes of one seeded gallery.  Every variant once per round, interleaved, --runs rounds
(search_bench.timed: device events after warm-up); median and spread = max - min.  Each result is named by its tiles and
chunks, which is what the comparison is about: at 4 096 queries a chunk is 32 tiles and a launch is 64 blocks per chunk,
512 blocks run at a time (two per CU), so 64 chunks are 8 full rounds and 68 - 72 chunks need a ninth.
   python tools/search_itemset_rounds.py --items 262144,245760 --sets 12288 --out profiles/search_itemset_rounds.json
   python tools/search_itemset_rounds.py --items 276480 --sets 13107,13824 --out profiles/search_itemset_rounds2.json"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from search_bench import D, K, M, timed  # noqa: E402
from mmt_amd.search import VideoIndex  # noqa: E402

NQ = 4096


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--items', default='262144', help='item counts of the plain searches')
  ap.add_argument('--sets', default='12288', help='set counts of the item-pooled searches')
  ap.add_argument('--set-size', type=int, default=20)
  ap.add_argument('--runs', type=int, default=3)
  ap.add_argument('--min-seconds', type=float, default=0.5)
  ap.add_argument('--out', default=None)
  a = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit('search_itemset_rounds needs the GPU')
  dev = torch.device('cuda', 0)
  c = a.set_size
  items = [int(x) for x in a.items.split(',')]
  sets = [int(x) for x in a.sets.split(',')]
  nv = max(items + [nt * c for nt in sets])
  gen = torch.Generator(device=dev).manual_seed(0)
  nrm = lambda x: torch.nn.functional.normalize(x, dim=-1)
  g = nrm(torch.randn(nv, M, D, device=dev, generator=gen))
  gw = torch.softmax(torch.randn(nv, M, device=dev, generator=gen), -1)
  q = nrm(torch.randn(NQ, M, D, device=dev, generator=gen))
  qw = torch.softmax(torch.randn(NQ, M, device=dev, generator=gen), -1)

  def build(n, dtype):
    index = VideoIndex.empty(n, M, D, dev, dtype=getattr(torch, dtype))
    for at in range(0, n, 8192):
      index.add(g[at:min(n, at + 8192)], gw[at:min(n, at + 8192)])
    return index
  fns = {}
  for dtype in ('float32', 'bfloat16'):
    for n in items:
      tiles = -(-n // 128)
      fns['%s/plain_%d_items_%d_tiles_%d_chunks' % (dtype, n, tiles, -(-tiles // 32))] = (
          lambda index=build(n, dtype): index.search(q, qw, k=K))
    for nt in sets:
      index = build(nt * c, dtype)
      tiles = -(-nt // (128 // c))
      fns['%s/item_pooled_c%d_%d_sets_%d_tiles_%d_chunks' % (dtype, c, nt, tiles, -(-tiles // 32))] = (
          lambda index=index, ip=index.item_pooling(c): index.search(q, qw, k=K, item_pooling=ip))
  ts = {n: [] for n in fns}
  for _ in range(a.runs):
    for n, fn in fns.items():
      ts[n].append(timed(fn, a.min_seconds)[0])
  res = {n: dict(seconds_median=float(np.median(v)), seconds_spread=max(v) - min(v), seconds_runs=v) for n, v in ts.items()}
  for n, r in res.items():
    print('%-60s %.3f ms (spread %.3f)' % (n, r['seconds_median'] * 1e3, r['seconds_spread'] * 1e3))
  if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
      json.dump(res, f, indent=1)


if __name__ == '__main__':
  main()
