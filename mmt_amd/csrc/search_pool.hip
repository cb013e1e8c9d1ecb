// Query-set pooling without the N_query x N_gallery matrix: the queries are NS sets of C consecutive rows (the captions of a
// video, the clips of a query video, a caption and its paraphrases) and every scan answers per SET, on the pooled score
//   mean: v(s, g) = fl(rw[r0] * score(r0, g)), then v = fl(v + fl(rw[ri] * score(ri, g)))   (reference: model/model.py:826-831,
//                                                                 merge_caption_similiarities = 'avg', is rw = 1 / C)
//   max : v(s, g) = score(r0, g), then v = score(ri, g) where score(ri, g) > v
// over the rows r0 < r1 < ... of set s whose weight rw[r] is not 0 (tk_tile_pool of search_scan.h has the order and why it
// may work in place).  The score is not linear in the query -- its denominator depends on the pair -- so the rows cannot
// be merged before the scan: the pooling is a step on the score tile.
//
// A block takes SB = 64 / C whole sets: query rows q0 = block * SB * C and the SB * C rows behind it; the remaining rows
// of the 64-row tile are scored and never read (C = 33 .. 64: one set per block, up to half the tile idle).  Per 128-column
// tile: tk_tile (the scan's own scores, bit for bit), tk_tile_pool, then the step of the unpooled kernel over `sets_live`
// rows in place of `rows_live`:
//   pool_topk_kernel<BF16>       : tk_tile_select<true> and tk_flush of search_topk.h -- the running top-k of search.hip, one
//                                  list per set; workspace [NS][n_chunks][k], merged by tk_merge_launch (search.hip).
//   pool_rank_kernel<BF16, true> : thresholds.  Tile column c of block (qt, j) holds the gallery row of pair p = 128 j + c of
//                                  the block's (set, target) pairs; the column is scored on ALL rows of the block, pooled,
//                                  and the entry on the pair's own set, row p / T, is kept.  Same tile, same pool step, so
//                                  the threshold has the bits the count pass computes for that (set, item).
//   pool_rank_kernel<BF16, false>: counts, the count step of rank_kernel (tk_tile_count, tk_count_flush) over the pooled
//                                  rows; (greater, equal) per (set, target, chunk), summed by rk_reduce_launch.
// The subset bitmap is a pointer that may be null, as in the masked kernels: a tile without an allowed item is skipped
// before its K loop.  The chunk rule is tk_chunk's, taken from the number of query BLOCKS (ceil(NS / SB)), which is what
// fills the chip.  A pooled value depends on the set's rows, their weights and the item only: score bits do not depend on
// the tile row, the pool order is the row order, so neither the set's place in its block nor the launch geometry enters.
// No atomics, one writer per slot: bit-reproducible.
//
// LDS: the unpooled kernel's layout plus the row weights (256 bytes), the candidate lists for SB rows instead of 64:
// union + 4 KiB query weights + 256 + 768 + SB * (k + 64) * 8 (top-k); + 128 * 4 (thresholds); + SB * T * 12 (counts).
#include <climits>

#include "search_topk.h"

#define PL_MAXC TK_Q   // MAX_SET: one 64-row query block holds whole sets
#define PL_MAXT 32

struct PlArgs {
  const void* q;            // fp32: Q' [NS * C][K]; bf16: hi(Q')
  const void* q_lo;         // bf16: lo(Q')
  const float* qw;          // [NS * C][M]
  const void* g;            // [NV][K] fp32 or bf16 bits
  const float* gw;          // [NV][M]
  const float* rw;          // [NS * C] row weights, 0 = the row takes no part
  const uint32_t* subset;   // top-k, count: bit g & 31 of word g >> 5 allows item g (nullable = all; 16-byte aligned)
  uint64_t* ws;             // top-k: [NS][n_chunks][k]
  const int64_t* targets;   // thresholds: [NS][T]
  float* thr;               // [NS][T]
  int32_t* cnt;             // count: [NS][T][n_chunks][2]
  int NQ, NV, M, K, NS, C, SB, mode, k, T, chunk, n_qt, n_chunks;
};

// Row weights of the block's rows -> sRw [TK_Q], zero past the block's live rows (so an idle row never takes part).
__device__ __forceinline__ void pl_load_rw(float* sRw, const float* rw, int q0, int rows_live, int tid) {
  if (tid < TK_Q) sRw[tid] = tid < rows_live ? rw[q0 + tid] : 0.f;
}

// One block of the pooled top-k scan: SB sets x one gallery chunk -> the chunk's sorted k best per set in the workspace.
template <bool BF16>
__global__ __launch_bounds__(256) void pool_topk_kernel(PlArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int kUnion = BF16 ? TKB_UNION_BYTES : TK_UNION_BYTES;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int bid = xcd_remap(blockIdx.x, gridDim.x);  // gallery-chunk-major: an XCD's blocks share their chunk in L2
  const int chunk = bid / a.n_qt, s0 = (bid % a.n_qt) * a.SB, q0 = s0 * a.C;
  const int sets_live = min(a.NS - s0, a.SB);
  const int g_begin = chunk * a.chunk, g_end = min(a.NV, g_begin + a.chunk);
  const int cap = a.k + 64;
  uint64_t* ws = a.ws + chunk * (int64_t)a.k;
  const int64_t ws_row = (int64_t)a.n_chunks * a.k;

  float* sS = (float*)smem;                                   // [TK_Q][TK_SLD]  scores, then pooled rows 0 .. sets_live - 1
  float* sQw = (float*)(smem + kUnion);                       // [TK_Q][MMT_MAX_EXPERTS]
  float* sRw = sQw + TK_Q * MMT_MAX_EXPERTS;                  // [TK_Q] row weights
  int* sN = (int*)(sRw + TK_Q);                               // [TK_Q] candidates held
  uint64_t* sT = (uint64_t*)(sN + TK_Q);                      // [TK_Q] thresholds
  uint64_t* sC = sT + TK_Q;                                   // [SB][cap] candidates
  const int l31 = lane & 31, h = lane >> 5, wq = wave >> 1, wg = wave & 1;
  if (tid < TK_Q) { sN[tid] = 0; sT[tid] = 0; }
  tk_load_qw(sQw, a.qw, a.NQ, a.M, q0, tid);
  pl_load_rw(sRw, a.rw, q0, sets_live * a.C, tid);
  for (int g0 = g_begin; g0 < g_end; g0 += TK_G) {
    uint64_t m0 = ~0ull, m1 = ~0ull;
    if (a.subset && !tk_tile_mask(a.subset, g0, m0, m1)) continue;  // block-uniform: nothing of this tile is allowed
    tk_tile<BF16, false>(a, smem, sS, sQw, q0, [=](int r) { return g0 + r < g_end ? g0 + r : -1; }, tid, wq, wg, l31, h);
    tk_tile_pool(sS, sRw, a.C, sets_live, a.mode, tid);
    __syncthreads();
    tk_tile_select<true>(sS, sC, sN, sT, a.k, sets_live, g0, g_end, wave, lane, m0, m1, nullptr, 0);
  }
  __syncthreads();
  for (int rr = 0; rr < TK_Q / 4; ++rr) {
    const int row = wave * (TK_Q / 4) + rr;
    if (row >= sets_live) break;
    tk_flush(sC + row * cap, sN[row], a.k, lane, ws + (s0 + row) * ws_row);
  }
}

// The pooled threshold pass (THR) or count pass of one block.
template <bool BF16, bool THR>
__global__ __launch_bounds__(256) void pool_rank_kernel(PlArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int kUnion = BF16 ? TKB_UNION_BYTES : TK_UNION_BYTES;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, h = lane >> 5, wq = wave >> 1, wg = wave & 1;
  const int T = a.T;
  float* sS = (float*)smem;                       // [TK_Q][TK_SLD]  scores, then pooled rows
  float* sQw = (float*)(smem + kUnion);           // [TK_Q][MMT_MAX_EXPERTS]
  float* sRw = sQw + TK_Q * MMT_MAX_EXPERTS;      // [TK_Q] row weights
  if constexpr (THR) {
    int* sRow = (int*)(sRw + TK_Q);               // [TK_G] gallery row of the tile's columns
    const int s0 = (blockIdx.x % a.n_qt) * a.SB, q0 = s0 * a.C, p0 = (blockIdx.x / a.n_qt) * TK_G;
    const int sets_live = min(a.NS - s0, a.SB);
    const int pairs = sets_live * T;              // live (set, target) pairs of this block (<= 64 * 32)
    tk_load_qw(sQw, a.qw, a.NQ, a.M, q0, tid);
    pl_load_rw(sRw, a.rw, q0, sets_live * a.C, tid);
    if (tid < TK_G) {
      const int64_t tg = p0 + tid < pairs ? a.targets[(int64_t)s0 * T + p0 + tid] : -1;
      sRow[tid] = (tg >= 0 && tg < a.NV) ? (int)tg : -1;
    }
    __syncthreads();
    tk_tile<BF16, false>(a, smem, sS, sQw, q0, [=](int r) { return sRow[r]; }, tid, wq, wg, l31, h);
    tk_tile_pool(sS, sRw, a.C, sets_live, a.mode, tid);
    __syncthreads();
    if (tid < TK_G && p0 + tid < pairs)
      a.thr[(int64_t)s0 * T + p0 + tid] = sRow[tid] >= 0 ? sS[((p0 + tid) / T) * TK_SLD + tid] : __builtin_nanf("");
  } else {
    float* sThr = sRw + TK_Q;                     // [SB][T]
    int* sCnt = (int*)(sThr + a.SB * T);          // [SB][T][2]
    const int bid = xcd_remap(blockIdx.x, gridDim.x);  // gallery-chunk-major: an XCD's blocks share their chunk in L2
    const int chunk = bid / a.n_qt, s0 = (bid % a.n_qt) * a.SB, q0 = s0 * a.C;
    const int sets_live = min(a.NS - s0, a.SB);
    const int g_begin = chunk * a.chunk, g_end = min(a.NV, g_begin + a.chunk);
    tk_load_qw(sQw, a.qw, a.NQ, a.M, q0, tid);
    pl_load_rw(sRw, a.rw, q0, sets_live * a.C, tid);
    for (int i = tid; i < a.SB * T; i += 256) {
      sThr[i] = i < sets_live * T ? a.thr[(int64_t)s0 * T + i] : 0.f;
      sCnt[2 * i] = 0;
      sCnt[2 * i + 1] = 0;
    }
    __syncthreads();  // every tile may be skipped: the counters are read below all the same
    for (int g0 = g_begin; g0 < g_end; g0 += TK_G) {
      uint64_t m0 = ~0ull, m1 = ~0ull;
      if (a.subset && !tk_tile_mask(a.subset, g0, m0, m1)) continue;  // block-uniform
      tk_tile<BF16, false>(a, smem, sS, sQw, q0, [=](int r) { return g0 + r < g_end ? g0 + r : -1; }, tid, wq, wg, l31, h);
      tk_tile_pool(sS, sRw, a.C, sets_live, a.mode, tid);
      __syncthreads();
      // wave w owns pooled rows 16w .. 16w + 15 for the whole block, so its counters need no barrier
      const bool live0 = g0 + lane < g_end && ((m0 >> lane) & 1ull);
      const bool live1 = g0 + 64 + lane < g_end && ((m1 >> lane) & 1ull);
      tk_tile_count(sS, sThr, sCnt, T, sets_live, live0, live1, wave, lane);
    }
    tk_count_flush(sCnt, a.cnt, T, sets_live, s0, a.n_chunks, chunk, wave, lane);
  }
}

namespace {
bool pl_sets_ok(int NS, int C, int mode) {
  return NS > 0 && C >= 1 && C <= PL_MAXC && (int64_t)NS * C <= INT_MAX && (mode == TK_POOL_MEAN || mode == TK_POOL_MAX);
}

// Query blocks of a pooled scan: SB = 64 / C sets each.
int pl_blocks(int NS, int C) {
  const int sb = TK_Q / C;
  return (NS + sb - 1) / sb;
}

// The chunk rule of the unpooled scans, taken from the number of query blocks.
int pl_chunk(int NS, int C, int NV) {
  const int64_t rows = (int64_t)pl_blocks(NS, C) * TK_Q;
  return tk_chunk(rows > INT_MAX ? INT_MAX : (int)rows, NV);
}

int pl_n_chunks(int NS, int C, int NV) {
  const int chunk = pl_chunk(NS, C, NV);
  return (NV + chunk - 1) / chunk;
}

template <bool BF16>
constexpr size_t pl_base_lds() { return tk_base_lds<BF16>() + TK_Q * 4; }
size_t pl_topk_lds(int sb, int k) { return TK_Q * (4 + 8) + (size_t)sb * (k + 64) * 8; }
size_t pl_count_lds(int sb, int T) { return (size_t)sb * T * 12; }

// The gate and the fill every entry point shares: 0, or the error code.  `own`: the entry's own pointers are all there.
// `subset`: the descriptor's, or null for a pass that has none.  The descriptor's NQ rows are NS = NQ / C whole sets.
template <bool BF16>
int pl_fill(PlArgs& a, const MmtSearchScan& s, const uint32_t* subset, bool own) {
  const int C = s.set_size, NS = C >= 1 ? s.NQ / C : 0;
  if (!tk_scan_operands<BF16>(s) || !s.set_weights || !own || !pl_sets_ok(NS, C, s.mode) || s.NQ != NS * C ||
      !tk_shape_ok(s.NQ, s.NV, s.M, s.d, BF16))
    return MMT_ERR_ARG;
  if (((uintptr_t)s.q | (uintptr_t)s.q_lo | (uintptr_t)s.g | (uintptr_t)subset) & 15) return MMT_ERR_ALIGN;
  a.q = s.q; a.q_lo = s.q_lo; a.qw = s.qw; a.g = s.g; a.gw = s.gw; a.rw = s.set_weights; a.subset = subset;
  a.NQ = s.NQ; a.NV = s.NV; a.M = s.M; a.K = s.M * s.d; a.NS = NS; a.C = C; a.SB = TK_Q / C; a.mode = s.mode;
  a.chunk = pl_chunk(NS, C, s.NV);
  a.n_qt = pl_blocks(NS, C);
  a.n_chunks = (s.NV + a.chunk - 1) / a.chunk;
  return 0;
}

// The k = 128 footprint of the top-k kernels at C = 1 is over the 64 KiB default.
void pl_topk_lds_limits() {
  static bool done[64] = {};
  tk_lds_limits(done, {{(const void*)pool_topk_kernel<false>, pl_base_lds<false>() + pl_topk_lds(TK_Q, TK_MAXK)},
                       {(const void*)pool_topk_kernel<true>, pl_base_lds<true>() + pl_topk_lds(TK_Q, TK_MAXK)}});
}

// The count kernels' T = 32 footprint at C = 1 passes the 64 KiB default.
template <bool BF16>
void pl_count_lds_limits() {
  static bool done[64] = {};
  tk_lds_limits(done, {{(const void*)pool_rank_kernel<BF16, false>, pl_base_lds<BF16>() + pl_count_lds(TK_Q, PL_MAXT)}});
}

template <bool BF16>
int pl_topk_body(const MmtSearchScan& s, int k, uint64_t* ws, float* scores, int64_t* index, void* stream) {
  PlArgs a = {};
  if (k < 1 || k > TK_MAXK) return MMT_ERR_ARG;
  if (const int rc = pl_fill<BF16>(a, s, s.subset, ws && index)) return rc;
  a.ws = ws; a.k = k;
  pl_topk_lds_limits();
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL((pool_topk_kernel<BF16>), dim3(a.n_qt * a.n_chunks), dim3(256),
                     pl_base_lds<BF16>() + pl_topk_lds(a.SB, k), st, a);
  return tk_merge_launch(ws, a.NS, a.n_chunks, k, k < s.NV ? k : s.NV, scores, index, st);
}

template <bool BF16>
int pl_thresholds_body(const MmtSearchScan& s, const int64_t* targets, int T, float* thr, void* stream) {
  PlArgs a = {};
  if (T < 1 || T > PL_MAXT) return MMT_ERR_ARG;
  if (const int rc = pl_fill<BF16>(a, s, nullptr, targets && thr)) return rc;
  a.targets = targets; a.thr = thr; a.T = T;
  const int n_pt = (a.SB * T + TK_G - 1) / TK_G;  // threshold tiles per query block
  hipLaunchKernelGGL((pool_rank_kernel<BF16, true>), dim3(a.n_qt * n_pt), dim3(256), pl_base_lds<BF16>() + TK_G * 4,
                     (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

// workspace (int32 units): (greater, equal) [NS][T][n_chunks][2]
template <bool BF16>
int pl_count_body(const MmtSearchScan& s, const float* thr, int T, int32_t* ws, int32_t* greater, int32_t* equal,
                  void* stream) {
  PlArgs a = {};
  if (T < 1 || T > PL_MAXT) return MMT_ERR_ARG;
  if (const int rc = pl_fill<BF16>(a, s, s.subset, thr && ws && greater && equal)) return rc;
  a.thr = const_cast<float*>(thr); a.cnt = ws; a.T = T;
  pl_count_lds_limits<BF16>();
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL((pool_rank_kernel<BF16, false>), dim3(a.n_qt * a.n_chunks), dim3(256),
                     pl_base_lds<BF16>() + pl_count_lds(a.SB, T), st, a);
  return rk_reduce_launch(a.cnt, (int64_t)a.NS * T, a.n_chunks, greater, equal, st);
}
}  // namespace

extern "C" int64_t mmt_topk_pooled_workspace_keys(int NS, int C, int NV, int k) {
  if (!pl_sets_ok(NS, C, TK_POOL_MEAN) || NV <= 0 || k < 1 || k > TK_MAXK) return MMT_ERR_ARG;
  return (int64_t)NS * pl_n_chunks(NS, C, NV) * k;
}

extern "C" int64_t mmt_count_pooled_workspace_ints(int NS, int C, int NV, int T) {
  if (!pl_sets_ok(NS, C, TK_POOL_MEAN) || NV <= 0 || T < 1 || T > PL_MAXT) return MMT_ERR_ARG;
  return (int64_t)NS * T * 2 * (int64_t)pl_n_chunks(NS, C, NV);
}

// The query-set halves of mmt_search_topk, mmt_search_thresholds and mmt_search_count (search.hip, search_rank.hip: the
// descriptor has passed their gate, so the storage is fp32 or bf16).
int pl_topk(const MmtSearchScan& s, int k, uint64_t* ws, float* scores, int64_t* index, void* stream) {
  return s.storage == MMT_SEARCH_FP32 ? pl_topk_body<false>(s, k, ws, scores, index, stream)
                                      : pl_topk_body<true>(s, k, ws, scores, index, stream);
}

int pl_thresholds(const MmtSearchScan& s, const int64_t* targets, int T, float* thr, void* stream) {
  return s.storage == MMT_SEARCH_FP32 ? pl_thresholds_body<false>(s, targets, T, thr, stream)
                                      : pl_thresholds_body<true>(s, targets, T, thr, stream);
}

int pl_count(const MmtSearchScan& s, const float* thr, int T, int32_t* ws, int32_t* greater, int32_t* equal, void* stream) {
  return s.storage == MMT_SEARCH_FP32 ? pl_count_body<false>(s, thr, T, ws, greater, equal, stream)
                                      : pl_count_body<true>(s, thr, T, ws, greater, equal, stream);
}
