"""The per-expert score breakdown (search.VideoIndex.expert_scores, mmt_search_expert_parts) at shortlist scale: 4 096
rows x 128 candidates on a gallery of 262 144 items x 7 experts x 512, per storage dtype.

  kernel            mmt_search_expert_parts alone, on rows folded beforehand: one launch for all R x C pairs
  expert_scores     the public call: the fp32 fold and the row batches included
  search            search(k = 10), the yardstick of the next line
  search_explained  search_explained(k = 10): the same search, then the breakdown of its 10 hits
  torch             the route the call replaces, chunked so that it fits: index_select of the hit rows, dequantise to fp32,
                    einsum('rmd,rcmd->rcm'), the gate and the division in torch ops

The candidates are uniformly random items (seeded), every pair another stored row: the gather at its worst, nothing
shared inside a list.  Times are device events after a warm-up, over >= --min-seconds of work per point, the median of
--runs rounds with every variant once per round; spread = max - min.  Bytes are what the algorithm needs, from the shapes:
R C K sizeof(storage) gathered + R C M 12 of weights and outputs + R K 4 of folded rows; the roof is that over the HBM
rate of MI355X (8.0 TB/s spec, 6.29 TB/s measured for a streaming copy).
   python tools/explain_bench.py [--gallery-dtype float32,bfloat16,float8_e4m3fn] [--out profiles/search_explain_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mmt_amd import _lib, ops, search  # noqa: E402

HBM_SPEC, HBM_COPY = 8.0e12, 6.29e12
DTYPES = {'float32': torch.float32, 'bfloat16': torch.bfloat16, 'float8_e4m3fn': torch.float8_e4m3fn}


def timed(fn, min_seconds):
  """Milliseconds per call: device events around enough calls for min_seconds, after one warm-up call."""
  fn()
  torch.cuda.synchronize()
  start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  calls, total = 0, 0.0
  while total < min_seconds * 1e3:
    n = max(1, calls)
    start.record()
    for _ in range(n):
      fn()
    stop.record()
    stop.synchronize()
    total += start.elapsed_time(stop)
    calls += n
  return total / calls


def torch_route(index, q, qw, cand, chunk):
  """parts [R, C, M] by torch ops, `chunk` rows at a time: the gathered operand of a chunk is chunk * C * K * 4 bytes."""
  m, d = index.num_experts, index.dim
  qf = (qw[:, :, None] * q)
  out = torch.empty(cand.shape + (m,), device=q.device, dtype=torch.float32)
  for r0 in range(0, q.shape[0], chunk):
    c = cand[r0:r0 + chunk]
    rows = index.folded.view(torch.uint8).index_select(0, c.reshape(-1)).view(index.dtype).to(torch.float32)
    if index.scales is not None:
      rows = rows * index.scales.index_select(0, c.reshape(-1))[:, None]
    dots = torch.einsum('rmd,rcmd->rcm', qf[r0:r0 + chunk], rows.view(c.shape[0], c.shape[1], m, d))
    den = torch.einsum('rm,rcm->rc', qw[r0:r0 + chunk], index.weights[c])
    out[r0:r0 + chunk] = dots / torch.where(den == 0, torch.full_like(den, 1e-5), den)[:, :, None]
  return out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--gallery-dtype', default='float32,bfloat16,float8_e4m3fn')
  ap.add_argument('--rows', type=int, default=4096)
  ap.add_argument('--candidates', type=int, default=128)
  ap.add_argument('--items', type=int, default=262144)
  ap.add_argument('--experts', type=int, default=7)
  ap.add_argument('--dim', type=int, default=512)
  ap.add_argument('--runs', type=int, default=5)
  ap.add_argument('--min-seconds', type=float, default=0.3)
  ap.add_argument('--torch-chunk', type=int, default=64)
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'search_explain_bench.json'))
  args = ap.parse_args()
  assert torch.cuda.is_available(), 'explain_bench needs the GPU: there is no CPU path to time'
  dev = torch.device('cuda', 0)
  r, c, nv, m, d = args.rows, args.candidates, args.items, args.experts, args.dim
  k = m * d
  gen = torch.Generator(device=dev).manual_seed(2024)
  q, qw = torch.randn(r, m, d, device=dev, generator=gen), torch.rand(r, m, device=dev, generator=gen)
  cand = torch.randint(0, nv, (r, c), device=dev, generator=gen)
  L = _lib.lib()
  results = dict(rows=r, candidates=c, items=nv, experts=m, dim=d, runs=args.runs, min_seconds=args.min_seconds, dtypes={})
  for name in args.gallery_dtype.split(','):
    dtype = DTYPES[name]
    index = search.VideoIndex.empty(nv, m, d, dev, dtype=dtype)
    fill = torch.Generator(device=dev).manual_seed(7)
    for lo in range(0, nv, 16384):
      n = min(16384, nv - lo)
      index.add(torch.randn(n, m, d, device=dev, generator=fill), torch.rand(n, m, device=dev, generator=fill))
    qf = search._fold(q, qw)
    parts, mix = (torch.empty(r, c, m, device=dev, dtype=torch.float32) for _ in range(2))

    def kernel():
      search.check(L.mmt_search_expert_parts(ops._p(qf), ops._p(qw), ops._p(index.folded), ops._p(index.weights),
                                             ops._p(index.scales), search._STORAGE[dtype], nv, m, d, ops._p(cand), r, c,
                                             ops._p(parts), ops._p(mix), ops._stream()), 'mmt_search_expert_parts')
    variants = {'kernel': kernel,
                'expert_scores': lambda: index.expert_scores(q, qw, cand),
                'search': lambda: index.search(q, qw, k=10),
                'search_explained': lambda: index.search_explained(q, qw, k=10),
                'torch': lambda: torch_route(index, q, qw, cand, args.torch_chunk)}
    got = index.expert_scores(q[:64], qw[:64], cand[:64]).parts
    want = torch_route(index, q[:64], qw[:64], cand[:64], args.torch_chunk)
    agree = float((got - want).abs().max())
    times = {v: [] for v in variants}
    for _ in range(args.runs):
      for v, fn in variants.items():
        times[v].append(timed(fn, args.min_seconds))
    elt = torch.empty(0, dtype=dtype).element_size()
    nbytes = r * c * k * elt + r * c * m * 12 + r * k * 4
    ms = statistics.median(times['kernel'])
    entry = dict(bytes=nbytes, gathered_bytes=r * c * k * elt, max_abs_diff_to_torch=agree,
                 kernel_tb_per_s=nbytes / (ms * 1e-3) / 1e12, share_of_hbm_spec=nbytes / HBM_SPEC / (ms * 1e-3),
                 share_of_hbm_copy=nbytes / HBM_COPY / (ms * 1e-3),
                 ms={v: dict(median=statistics.median(t), spread=max(t) - min(t)) for v, t in times.items()})
    results['dtypes'][name] = entry
    print(name, json.dumps(entry))
    del index, parts, mix, qf
    torch.cuda.empty_cache()
  os.makedirs(os.path.dirname(args.out), exist_ok=True)
  with open(args.out, 'w') as f:
    json.dump(results, f, indent=1)
  print('wrote', args.out)


if __name__ == '__main__':
  main()
