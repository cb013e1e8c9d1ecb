// Exact top-k over per-query shortlists (search.py: VideoIndex.rescore): "the k best among THESE items", the second stage
// of a two-stage search -- a wide, cheap list from an fp8 index, a range search or another model, re-ranked on the index
// that holds the items at full precision.  candidates int64 [NQ][C], 1 <= C <= 1024, -1 (or anything outside 0 .. NV - 1)
// = none, any order, an item may repeat.  Per query the best min(k, C) DISTINCT candidates under the one order of the
// search kernels (tk_key: score descending, -0 tied with +0, equal scores by ascending item), then (-inf, -1).  It
// replaces what a caller had to build from mmt_search_thresholds (at most 32 targets per launch, unsorted scores, NaN for
// none) and a host-side sort with a tie rule and de-duplication of its own.  Two launches, one call:
//   rescore_score_kernel<BF16, .>: the threshold pass of rank_kernel (search_rank.hip) for any C.  Block = a 64-query tile
//                                  x 128 consecutive (query, candidate) pairs of it: tile column c of block (qt, j) holds
//                                  the gallery row of pair p = 128 j + c, i.e. of query p / C, candidate p % C, through the
//                                  `grow` functor of tk_tile (search_scan.h), so the score has the bits every scan gives the
//                                  pair; only the entry on the pair's own query row is kept, and it goes to the workspace
//                                  [NQ][C] as tk_key(score, item), 0 for none.  A block past the tile's live pairs (a last
//                                  query tile with fewer than 64 rows) leaves before its K loop.  This computes 64 rows to
//                                  keep one: per tile it reads the 128 gallery rows a scan tile reads, and there are
//                                  NQ * C / 128 tiles against NQ * NV / 8192 of the full scan.
//   rescore_select_kernel        : one block per query.  The C keys, padded with 0 to a power of two P, are sorted
//                                  descending in LDS (bitonic, P / 2 comparators per step, 8 KiB at C = 1024).  A repeated
//                                  item has the same score bits and the same index, hence the same key: duplicates are
//                                  adjacent and a key equal to its predecessor is dropped.  Wave 0 walks the sorted list 64
//                                  keys at a time, places the survivors with a ballot and stops at min(k, C) of them; the
//                                  slots left over get (-inf, -1).  The score written is decoded from the key as the top-k
//                                  merge does (tk_score: a -0 comes back as +0).
// No atomics, every workspace and output slot has one writer: bit-reproducible, and independent of the order of a query's
// candidates (the sort sees a multiset of keys).  LDS: the score pass has the threshold pass's footprint (score tile /
// slab union + 4 KiB query weights + 512 B of rows: under the 64 KiB default, so no limit is raised); the select pass 8 P.
#include "search_topk.h"

#define RS_MAXC 1024

struct RsArgs {
  const void* q;              // fp32: Q' [NQ][K]; bf16: hi(Q')
  const void* q_lo;           // bf16: lo(Q')
  const float* qw;            // [NQ][M]
  const void* g;              // [NV][K] fp32, bf16 bits or e4m3fn codes
  const float* gw;            // [NV][M]
  const int64_t* candidates;  // [NQ][C]
  uint64_t* keys;             // [NQ][C] workspace
  int NQ, NV, M, K, C, n_qt;
  static constexpr TkMask kMask = TK_MASK_NONE;
  static constexpr bool kNorm = false;
};

struct RsFp8Args : RsArgs {
  const float* gscale;        // [NV]
  static constexpr bool kFp8 = true;
};

template <bool BF16, class Args>
__global__ __launch_bounds__(256) void rescore_score_kernel(Args a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int kUnion = BF16 ? TKB_UNION_BYTES : TK_UNION_BYTES;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, h = lane >> 5, wq = wave >> 1, wg = wave & 1;
  const int C = a.C;
  float* sS = (float*)smem;                            // [TK_Q][TK_SLD]  scores (after the K loop)
  float* sQw = (float*)(smem + kUnion);                // [TK_Q][MMT_MAX_EXPERTS]
  int* sRow = (int*)(sQw + TK_Q * MMT_MAX_EXPERTS);    // [TK_G] gallery row of the tile's columns
  const int q0 = (blockIdx.x % a.n_qt) * TK_Q, p0 = (blockIdx.x / a.n_qt) * TK_G;
  const int pairs = min(a.NQ - q0, TK_Q) * C;          // live (query, candidate) pairs of this query tile (<= 65536)
  if (p0 >= pairs) return;                             // block-uniform, before any barrier
  tk_load_qw(sQw, a.qw, a.NQ, a.M, q0, tid);
  if (tid < TK_G) {
    const int64_t cd = p0 + tid < pairs ? a.candidates[(int64_t)q0 * C + p0 + tid] : -1;
    sRow[tid] = (cd >= 0 && cd < a.NV) ? (int)cd : -1;
  }
  __syncthreads();
  tk_tile<BF16, false>(a, smem, sS, sQw, q0, [=](int r) { return sRow[r]; }, tid, wq, wg, l31, h);
  if (tid < TK_G && p0 + tid < pairs) {
    const int item = sRow[tid];
    a.keys[(int64_t)q0 * C + p0 + tid] = item >= 0 ? tk_key(sS[((p0 + tid) / C) * TK_SLD + tid], item) : 0ull;
  }
}

// One block of 64 .. 256 threads per query: keys [NQ][C] -> scores / index [NQ][kp], kp = min(k, C) <= 128.  P = C rounded
// up to a power of two, dynamic LDS 8 P bytes.
__global__ __launch_bounds__(256) void rescore_select_kernel(const uint64_t* __restrict__ keys, int C, int P, int kp,
                                                             float* __restrict__ scores, int64_t* __restrict__ index) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint64_t* sK = (uint64_t*)smem;  // [P]
  const int tid = threadIdx.x, nt = blockDim.x, q = blockIdx.x;
  for (int i = tid; i < P; i += nt) sK[i] = i < C ? keys[(int64_t)q * C + i] : 0ull;
  for (int size = 2; size <= P; size <<= 1)
    for (int stride = size >> 1; stride; stride >>= 1) {
      __syncthreads();
      for (int t = tid; t < (P >> 1); t += nt) {
        const int lo = ((t & ~(stride - 1)) << 1) | (t & (stride - 1)), hi = lo + stride;
        const uint64_t x = sK[lo], y = sK[hi];
        if ((x < y) == !(lo & size)) {  // descending where bit `size` of the position is clear
          sK[lo] = y;
          sK[hi] = x;
        }
      }
    }
  __syncthreads();
  if (tid >= 64) return;
  int n = 0;  // survivors placed so far: wave-uniform
  for (int base = 0; base < P && n < kp; base += 64) {
    const int i = base + tid;
    const uint64_t key = i < P ? sK[i] : 0ull;
    const bool keep = key && (i == 0 || key != sK[i - 1]);
    const uint64_t mask = __ballot(keep);
    const int pos = n + __popcll(mask & ((1ull << tid) - 1ull));
    if (keep && pos < kp) {
      scores[(int64_t)q * kp + pos] = tk_score(key);
      index[(int64_t)q * kp + pos] = tk_index(key);
    }
    n += __popcll(mask);
  }
  for (int j = n + tid; j < kp; j += 64) {
    scores[(int64_t)q * kp + j] = -__builtin_inff();
    index[(int64_t)q * kp + j] = -1;
  }
}

namespace {
bool rs_sizes_ok(int NQ, int C) {
  // the score pass's grid: ceil(NQ / 64) query tiles x ceil(64 C / 128) pair tiles
  return NQ > 0 && C >= 1 && C <= RS_MAXC && ((int64_t)((NQ + TK_Q - 1) / TK_Q)) * ((TK_Q * C + TK_G - 1) / TK_G) < (1ll << 31);
}

template <bool BF16, class Args>
int rs_rescore(const MmtSearchScan& s, const int64_t* candidates, int C, int k, uint64_t* ws, float* scores, int64_t* index,
               void* stream) {
  constexpr bool FP8 = TkFp8<Args>::value;
  if (!tk_scan_operands<BF16, FP8>(s) || !candidates || !ws || !scores || !index || !rs_sizes_ok(s.NQ, C) || k < 1 ||
      k > TK_MAXK || !tk_shape_ok(s.NQ, s.NV, s.M, s.d, BF16, FP8))
    return MMT_ERR_ARG;
  if (!tk_scan_aligned(s)) return MMT_ERR_ALIGN;  // (no subset here: the gate of the entry refused one)
  Args a = {};
  a.q = s.q; a.q_lo = s.q_lo; a.qw = s.qw; a.g = s.g; a.gw = s.gw; a.candidates = candidates; a.keys = ws;
  if constexpr (FP8) a.gscale = s.gscale;
  a.NQ = s.NQ; a.NV = s.NV; a.M = s.M; a.K = s.M * s.d; a.C = C; a.n_qt = (s.NQ + TK_Q - 1) / TK_Q;
  const hipStream_t st = (hipStream_t)stream;
  const int n_pt = (TK_Q * C + TK_G - 1) / TK_G;  // pair tiles per query tile
  hipLaunchKernelGGL((rescore_score_kernel<BF16, Args>), dim3(a.n_qt * n_pt), dim3(256), tk_base_lds<BF16>() + TK_G * 4, st, a);
  if (const int rc = (int)hipGetLastError()) return rc;
  int P = 1;
  while (P < C) P <<= 1;
  const int threads = P / 2 < 64 ? 64 : P / 2 > 256 ? 256 : P / 2;
  hipLaunchKernelGGL(rescore_select_kernel, dim3(s.NQ), dim3(threads), (size_t)P * 8, st, ws, C, P, k < C ? k : C, scores,
                     index);
  return (int)hipGetLastError();
}
}  // namespace

extern "C" int64_t mmt_rescore_workspace_keys(int NQ, int C) {
  if (!rs_sizes_ok(NQ, C)) return MMT_ERR_ARG;
  return (int64_t)NQ * C;
}

extern "C" int mmt_search_rescore(const MmtSearchScan* scan, const int64_t* candidates, int C, int k, uint64_t* ws,
                                  float* scores, int64_t* index, void* stream) {
  if (const int rc = tk_scan_gate(scan, SC_FP8)) return rc;
  switch (scan->storage) {
    case MMT_SEARCH_FP32: return rs_rescore<false, RsArgs>(*scan, candidates, C, k, ws, scores, index, stream);
    case MMT_SEARCH_BF16: return rs_rescore<true, RsArgs>(*scan, candidates, C, k, ws, scores, index, stream);
    default: return rs_rescore<true, RsFp8Args>(*scan, candidates, C, k, ws, scores, index, stream);
  }
}
