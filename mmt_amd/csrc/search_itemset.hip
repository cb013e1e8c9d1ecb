// Item-set pooling without the N_query x N_item matrix: the STORED items are NT sets of C consecutive items (the captions
// of a video in a caption index, the clips of a video in a clip gallery) and every scan answers per SET, on the pooled
// score
//   mean: v(q, t) = fl(iw[g0] * score(q, g0)), then v = fl(v + fl(iw[gi] * score(q, gi)))   (reference: model/model.py:826-831
//                                                     on the gallery axis -- video-to-text in 'avg' mode -- is iw = 1 / C)
//   max : v(q, t) = score(q, g0), then v = score(q, gi) where score(q, gi) > v
// over the items g0 < g1 < ... of set t whose weight iw[g] is not 0 (tk_tile_pool_items of search_scan.h has the order and
// why it may work in place).  The score's denominator depends on the pair, so the C items of a set cannot be merged when
// the index is built, and per-item top-k lists cannot be merged into set means: the pooling is a step on the score tile,
// search_pool.hip's along the other axis.
//
// A tile takes SG = 128 / C whole sets: with t0 its first set, its columns are items t0 * C .. (t0 + SG) * C - 1 and the
// remaining 128 - SG * C columns hold nothing (grow = -1: zero-filled, never read; C = 20 idles 8, C = 65 .. 128 puts one set
// in a tile).  Tiles advance by SG * C items, so a tile's first item is no multiple of 128.  A chunk is a whole number of
// tiles: tk_chunk's rule on 128 * ceil(NT / SG) virtual columns.  Per tile: tk_tile (the scan's own scores, bit for bit),
// tk_tile_pool_items, a barrier, then the step of the unpooled kernel over the tile's first `sets` columns, whose "item
// numbers" are the set numbers t0 + s:
//   iset_topk_kernel<BF16>       : tk_tile_select<true> and tk_flush of search_topk.h; workspace [NQ][n_chunks][k], merged by
//                                  tk_merge_launch (search.hip).
//   iset_rank_kernel<BF16, true> : thresholds.  A (query, target set) pair needs the C columns of its set, so a threshold
//                                  tile holds SG pairs: columns s * C .. s * C + C - 1 of block (qt, j) are the items of the
//                                  target of pair p = SG j + s of the block's (row, target) pairs.  The tile is scored on ALL
//                                  rows of the block and pooled by the same step in the same order; the entry on the pair's
//                                  own row, p / T, is kept: the threshold has the bits the count pass computes.
//   iset_rank_kernel<BF16, false>: counts, tk_tile_count and tk_count_flush over the pooled columns; (greater, equal) per
//                                  (query, target, chunk), summed by rk_reduce_launch.
// The subset bitmap is over SET numbers (nullable, as in the masked kernels); a tile's sets start at t0, any number, so
// its mask bits come through tk_tile_mask_window.  A tile without an allowed set is skipped before its K loop.  The item
// weights of a tile are staged in LDS (sIw, 512 bytes) before the tile's K loop, whose barriers publish them; they are
// next written after the barrier that follows the pool step.  A pooled value depends on the query row, the set's items and
// their weights only: score bits do not depend on the tile column, the pool order is the item order, so neither the
// set's place in its tile nor the launch geometry enters.  No atomics, one writer per slot: bit-reproducible.
//
// LDS: the unpooled kernel's layout plus the tile's item weights: union + 4 KiB query weights + 512 + 768 + 64 (k + 64) 8
// (top-k); + 128 * 4 (thresholds); + 64 * T * 12 (counts).
#include <climits>

#include "search_topk.h"

#define IS_MAXC TK_G   // MAX_ITEM_SET: one 128-column tile holds whole sets
#define IS_MAXT 32

struct IsArgs {
  const void* q;            // fp32: Q' [NQ][K]; bf16: hi(Q')
  const void* q_lo;         // bf16: lo(Q')
  const float* qw;          // [NQ][M]
  const void* g;            // [NT * C][K] fp32 or bf16 bits
  const float* gw;          // [NT * C][M]
  const float* iw;          // [NT * C] item weights, 0 = the item takes no part
  const uint32_t* subset;   // top-k, count: bit t & 31 of word t >> 5 allows SET t (nullable = all; 16-byte aligned)
  uint64_t* ws;             // top-k: [NQ][n_chunks][k]
  const int64_t* targets;   // thresholds: [NQ][T] set numbers
  float* thr;               // [NQ][T]
  int32_t* cnt;             // count: [NQ][T][n_chunks][2]
  int NQ, NT, M, K, C, SG, mode, k, T, n_tiles, tpc, n_qt, n_chunks, n_words;
};

// The tile at set t0 with `sets` live sets: its item weights -> sIw [TK_G], zero past the live columns.
__device__ __forceinline__ void is_load_iw(float* sIw, const float* iw, int i0, int cols, int tid) {
  if (tid < TK_G) sIw[tid] = tid < cols ? iw[i0 + tid] : 0.f;
}

// One block of the item-set top-k scan: 64 queries x one chunk of tiles -> the chunk's sorted k best sets per query.
template <bool BF16>
__global__ __launch_bounds__(256) void iset_topk_kernel(IsArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int kUnion = BF16 ? TKB_UNION_BYTES : TK_UNION_BYTES;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int bid = xcd_remap(blockIdx.x, gridDim.x);  // gallery-chunk-major: an XCD's blocks share their chunk in L2
  const int chunk = bid / a.n_qt, q0 = (bid % a.n_qt) * TK_Q;
  const int rows_live = min(a.NQ - q0, TK_Q);
  const int tile_begin = chunk * a.tpc, tile_end = min(a.n_tiles, tile_begin + a.tpc);
  const int cap = a.k + 64;
  uint64_t* ws = a.ws + chunk * (int64_t)a.k;
  const int64_t ws_row = (int64_t)a.n_chunks * a.k;

  float* sS = (float*)smem;                                   // [TK_Q][TK_SLD]  scores, then pooled columns 0 .. sets - 1
  float* sQw = (float*)(smem + kUnion);                       // [TK_Q][MMT_MAX_EXPERTS]
  float* sIw = sQw + TK_Q * MMT_MAX_EXPERTS;                  // [TK_G] item weights of the tile
  int* sN = (int*)(sIw + TK_G);                               // [TK_Q] candidates held
  uint64_t* sT = (uint64_t*)(sN + TK_Q);                      // [TK_Q] thresholds
  uint64_t* sC = sT + TK_Q;                                   // [TK_Q][cap] candidates
  const int l31 = lane & 31, h = lane >> 5, wq = wave >> 1, wg = wave & 1;
  if (tid < TK_Q) { sN[tid] = 0; sT[tid] = 0; }
  tk_load_qw(sQw, a.qw, a.NQ, a.M, q0, tid);
  for (int tile = tile_begin; tile < tile_end; ++tile) {
    const int t0 = tile * a.SG, sets = min(a.NT - t0, a.SG), cols = sets * a.C, i0 = t0 * a.C;
    uint64_t m0 = ~0ull, m1 = ~0ull;
    if (a.subset && !tk_tile_mask_window(a.subset, a.n_words, t0, sets, m0, m1)) continue;  // block-uniform
    is_load_iw(sIw, a.iw, i0, cols, tid);
    tk_tile<BF16, false>(a, smem, sS, sQw, q0, [=](int r) { return r < cols ? i0 + r : -1; }, tid, wq, wg, l31, h);
    tk_tile_pool_items(sS, sIw, a.C, sets, a.mode, tid);
    __syncthreads();
    tk_tile_select<true>(sS, sC, sN, sT, a.k, rows_live, t0, t0 + sets, wave, lane, m0, m1, nullptr, 0);
  }
  __syncthreads();
  for (int rr = 0; rr < TK_Q / 4; ++rr) {
    const int row = wave * (TK_Q / 4) + rr;
    if (row >= rows_live) break;
    tk_flush(sC + row * cap, sN[row], a.k, lane, ws + (q0 + row) * ws_row);
  }
}

// The item-set threshold pass (THR) or count pass of one block.
template <bool BF16, bool THR>
__global__ __launch_bounds__(256) void iset_rank_kernel(IsArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int kUnion = BF16 ? TKB_UNION_BYTES : TK_UNION_BYTES;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, h = lane >> 5, wq = wave >> 1, wg = wave & 1;
  const int T = a.T;
  float* sS = (float*)smem;                       // [TK_Q][TK_SLD]  scores, then pooled columns
  float* sQw = (float*)(smem + kUnion);           // [TK_Q][MMT_MAX_EXPERTS]
  float* sIw = sQw + TK_Q * MMT_MAX_EXPERTS;      // [TK_G] item weights of the tile
  if constexpr (THR) {
    int* sRow = (int*)(sIw + TK_G);               // [TK_G] item of the tile's columns
    const int q0 = (blockIdx.x % a.n_qt) * TK_Q, p0 = (blockIdx.x / a.n_qt) * a.SG;
    const int pairs = min(a.NQ - q0, TK_Q) * T;   // live (row, target) pairs of this block (<= 64 * 32)
    if (p0 >= pairs) return;                      // block-uniform: the last query block has fewer pairs
    tk_load_qw(sQw, a.qw, a.NQ, a.M, q0, tid);
    if (tid < TK_G) {
      const int s = tid / a.C, c = tid - s * a.C;
      int item = -1;
      if (s < a.SG && p0 + s < pairs) {
        const int64_t tg = a.targets[(int64_t)q0 * T + p0 + s];
        if (tg >= 0 && tg < a.NT) item = (int)tg * a.C + c;
      }
      sRow[tid] = item;
      sIw[tid] = item >= 0 ? a.iw[item] : 0.f;
    }
    __syncthreads();
    tk_tile<BF16, false>(a, smem, sS, sQw, q0, [=](int r) { return sRow[r]; }, tid, wq, wg, l31, h);
    tk_tile_pool_items(sS, sIw, a.C, a.SG, a.mode, tid);
    __syncthreads();
    if (tid < a.SG && p0 + tid < pairs)
      a.thr[(int64_t)q0 * T + p0 + tid] = sRow[tid * a.C] >= 0 ? sS[((p0 + tid) / T) * TK_SLD + tid] : __builtin_nanf("");
  } else {
    float* sThr = sIw + TK_G;                     // [TK_Q][T]
    int* sCnt = (int*)(sThr + TK_Q * T);          // [TK_Q][T][2]
    const int bid = xcd_remap(blockIdx.x, gridDim.x);  // gallery-chunk-major: an XCD's blocks share their chunk in L2
    const int chunk = bid / a.n_qt, q0 = (bid % a.n_qt) * TK_Q;
    const int rows_live = min(a.NQ - q0, TK_Q);
    const int tile_begin = chunk * a.tpc, tile_end = min(a.n_tiles, tile_begin + a.tpc);
    tk_load_qw(sQw, a.qw, a.NQ, a.M, q0, tid);
    for (int i = tid; i < TK_Q * T; i += 256) {
      sThr[i] = i < rows_live * T ? a.thr[(int64_t)q0 * T + i] : 0.f;
      sCnt[2 * i] = 0;
      sCnt[2 * i + 1] = 0;
    }
    __syncthreads();  // every tile may be skipped: the counters are read below all the same
    for (int tile = tile_begin; tile < tile_end; ++tile) {
      const int t0 = tile * a.SG, sets = min(a.NT - t0, a.SG), cols = sets * a.C, i0 = t0 * a.C;
      uint64_t m0 = ~0ull, m1 = ~0ull;
      if (a.subset && !tk_tile_mask_window(a.subset, a.n_words, t0, sets, m0, m1)) continue;  // block-uniform
      is_load_iw(sIw, a.iw, i0, cols, tid);
      tk_tile<BF16, false>(a, smem, sS, sQw, q0, [=](int r) { return r < cols ? i0 + r : -1; }, tid, wq, wg, l31, h);
      tk_tile_pool_items(sS, sIw, a.C, sets, a.mode, tid);
      __syncthreads();
      // wave w owns rows 16w .. 16w + 15 for the whole block, so its counters need no barrier
      const bool live0 = lane < sets && ((m0 >> lane) & 1ull);
      const bool live1 = 64 + lane < sets && ((m1 >> lane) & 1ull);
      tk_tile_count(sS, sThr, sCnt, T, rows_live, live0, live1, wave, lane);
    }
    tk_count_flush(sCnt, a.cnt, T, rows_live, q0, a.n_chunks, chunk, wave, lane);
  }
}

namespace {
bool is_sets_ok(int NT, int C, int mode) {
  return NT > 0 && C >= 1 && C <= IS_MAXC && (int64_t)NT * C <= INT_MAX && (mode == TK_POOL_MEAN || mode == TK_POOL_MAX);
}

// Tiles of an item-set scan: SG = 128 / C sets each.
int is_tiles(int NT, int C) {
  const int sg = TK_G / C;
  return (NT + sg - 1) / sg;
}

// The chunk rule of the unpooled scans on the tiles' 128 * n_tiles virtual columns -> tiles per chunk.
int is_tiles_per_chunk(int NQ, int NT, int C) {
  const int64_t cols = (int64_t)is_tiles(NT, C) * TK_G;
  return tk_chunk(NQ, cols > INT_MAX - TK_CHUNK ? INT_MAX - TK_CHUNK : (int)cols) / TK_G;
}

int is_n_chunks(int NQ, int NT, int C) {
  const int tpc = is_tiles_per_chunk(NQ, NT, C);
  return (is_tiles(NT, C) + tpc - 1) / tpc;
}

template <bool BF16>
constexpr size_t is_base_lds() { return tk_base_lds<BF16>() + TK_G * 4; }
size_t is_topk_lds(int k) { return TK_Q * (4 + 8) + (size_t)TK_Q * (k + 64) * 8; }
size_t is_count_lds(int T) { return (size_t)TK_Q * T * 12; }

// The gate and the fill every entry point shares: 0, or the error code.  `own`: the entry's own pointers are all there.
// `subset`: the descriptor's, or null for a pass that has none.  The descriptor's NV items are NT = NV / C whole sets.
template <bool BF16>
int is_fill(IsArgs& a, const MmtSearchScan& s, const uint32_t* subset, bool own) {
  const int C = s.set_size, NT = C >= 1 ? s.NV / C : 0;
  if (!tk_scan_operands<BF16>(s) || !s.set_weights || !own || !is_sets_ok(NT, C, s.mode) || s.NV != NT * C ||
      !tk_shape_ok(s.NQ, s.NV, s.M, s.d, BF16))
    return MMT_ERR_ARG;
  if (((uintptr_t)s.q | (uintptr_t)s.q_lo | (uintptr_t)s.g | (uintptr_t)subset) & 15) return MMT_ERR_ALIGN;
  a.q = s.q; a.q_lo = s.q_lo; a.qw = s.qw; a.g = s.g; a.gw = s.gw; a.iw = s.set_weights; a.subset = subset;
  a.NQ = s.NQ; a.NT = NT; a.M = s.M; a.K = s.M * s.d; a.C = C; a.SG = TK_G / C; a.mode = s.mode;
  a.n_tiles = is_tiles(NT, C);
  a.tpc = is_tiles_per_chunk(s.NQ, NT, C);
  a.n_qt = (s.NQ + TK_Q - 1) / TK_Q;
  a.n_chunks = (a.n_tiles + a.tpc - 1) / a.tpc;
  a.n_words = 4 * ((NT + 127) / 128);
  return 0;
}

// The k = 128 footprint of the top-k kernels is over the 64 KiB default.
void is_topk_lds_limits() {
  static bool done[64] = {};
  tk_lds_limits(done, {{(const void*)iset_topk_kernel<false>, is_base_lds<false>() + is_topk_lds(TK_MAXK)},
                       {(const void*)iset_topk_kernel<true>, is_base_lds<true>() + is_topk_lds(TK_MAXK)}});
}

// The count kernels' T = 32 footprint passes the 64 KiB default.
template <bool BF16>
void is_count_lds_limits() {
  static bool done[64] = {};
  tk_lds_limits(done, {{(const void*)iset_rank_kernel<BF16, false>, is_base_lds<BF16>() + is_count_lds(IS_MAXT)}});
}

template <bool BF16>
int is_topk_body(const MmtSearchScan& s, int k, uint64_t* ws, float* scores, int64_t* index, void* stream) {
  IsArgs a = {};
  if (k < 1 || k > TK_MAXK) return MMT_ERR_ARG;
  if (const int rc = is_fill<BF16>(a, s, s.subset, ws && index)) return rc;
  a.ws = ws; a.k = k;
  is_topk_lds_limits();
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL((iset_topk_kernel<BF16>), dim3(a.n_qt * a.n_chunks), dim3(256), is_base_lds<BF16>() + is_topk_lds(k), st,
                     a);
  return tk_merge_launch(ws, s.NQ, a.n_chunks, k, k < a.NT ? k : a.NT, scores, index, st);
}

template <bool BF16>
int is_thresholds_body(const MmtSearchScan& s, const int64_t* targets, int T, float* thr, void* stream) {
  IsArgs a = {};
  if (T < 1 || T > IS_MAXT) return MMT_ERR_ARG;
  if (const int rc = is_fill<BF16>(a, s, nullptr, targets && thr)) return rc;
  a.targets = targets; a.thr = thr; a.T = T;
  const int n_pt = (TK_Q * T + a.SG - 1) / a.SG;  // threshold tiles per query block
  hipLaunchKernelGGL((iset_rank_kernel<BF16, true>), dim3(a.n_qt * n_pt), dim3(256), is_base_lds<BF16>() + TK_G * 4,
                     (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

// workspace (int32 units): (greater, equal) [NQ][T][n_chunks][2]
template <bool BF16>
int is_count_body(const MmtSearchScan& s, const float* thr, int T, int32_t* ws, int32_t* greater, int32_t* equal,
                  void* stream) {
  IsArgs a = {};
  if (T < 1 || T > IS_MAXT) return MMT_ERR_ARG;
  if (const int rc = is_fill<BF16>(a, s, s.subset, thr && ws && greater && equal)) return rc;
  a.thr = const_cast<float*>(thr); a.cnt = ws; a.T = T;
  is_count_lds_limits<BF16>();
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL((iset_rank_kernel<BF16, false>), dim3(a.n_qt * a.n_chunks), dim3(256),
                     is_base_lds<BF16>() + is_count_lds(T), st, a);
  return rk_reduce_launch(a.cnt, (int64_t)s.NQ * T, a.n_chunks, greater, equal, st);
}
}  // namespace

extern "C" int64_t mmt_topk_itemsets_workspace_keys(int NQ, int NT, int C, int k) {
  if (NQ <= 0 || !is_sets_ok(NT, C, TK_POOL_MEAN) || k < 1 || k > TK_MAXK) return MMT_ERR_ARG;
  return (int64_t)NQ * is_n_chunks(NQ, NT, C) * k;
}

extern "C" int64_t mmt_count_itemsets_workspace_ints(int NQ, int NT, int C, int T) {
  if (NQ <= 0 || !is_sets_ok(NT, C, TK_POOL_MEAN) || T < 1 || T > IS_MAXT) return MMT_ERR_ARG;
  return (int64_t)NQ * T * 2 * (int64_t)is_n_chunks(NQ, NT, C);
}

// The item-set halves of mmt_search_topk, mmt_search_thresholds and mmt_search_count (search.hip, search_rank.hip: the
// descriptor has passed their gate, so the storage is fp32 or bf16).
int is_topk(const MmtSearchScan& s, int k, uint64_t* ws, float* scores, int64_t* index, void* stream) {
  return s.storage == MMT_SEARCH_FP32 ? is_topk_body<false>(s, k, ws, scores, index, stream)
                                      : is_topk_body<true>(s, k, ws, scores, index, stream);
}

int is_thresholds(const MmtSearchScan& s, const int64_t* targets, int T, float* thr, void* stream) {
  return s.storage == MMT_SEARCH_FP32 ? is_thresholds_body<false>(s, targets, T, thr, stream)
                                      : is_thresholds_body<true>(s, targets, T, thr, stream);
}

int is_count(const MmtSearchScan& s, const float* thr, int T, int32_t* ws, int32_t* greater, int32_t* equal, void* stream) {
  return s.storage == MMT_SEARCH_FP32 ? is_count_body<false>(s, thr, T, ws, greater, equal, stream)
                                      : is_count_body<true>(s, thr, T, ws, greater, equal, stream);
}
