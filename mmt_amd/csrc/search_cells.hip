// Cell-probed search (search.py: VideoIndex.cells, search_probed): the inverted file.  The gallery is partitioned into
// cells, every query row names a few of them (its probes), and the answer is the k best items of those cells -- for that
// row search(subset = the probed cells' items), bit for bit.  What is approximate is the choice of cells, the caller's.
//
// The stored rows are not moved: `items` holds the item numbers cell after cell (a cell's items ascending, cell c at
// offsets[c] .. offsets[c + 1]: search.py IndexCells) and the kernel reads the gallery through it.  The host regroups the
// call's (row, probe) pairs (search.py: _probe_plan, on the device with torch sorts and prefix sums; probe_plan is its numpy
// restatement): invalid, empty and repeated cells dropped, the pairs ordered by (cell, row), each cell's pairs cut into row
// groups of at most 64, each cell's items into pieces of at most CL_PIECE.  A work item is (row group, piece):
//   work [n_work][CL_WORK] int32 = (first pair, rows, first position in `items`, end position, piece); rows = 0: none
//   pair_row / pair_slot [n_pairs] int32: the query row of a pair and its probe slot, a number below P unique in the row
// n_work is an upper bound the host knows without waiting for the device; the entries past the call's real count hold
// rows = 0 and their blocks leave at once.
//   cells_scan_kernel<BF16, .>: one block per work item.  Its <= 64 query rows are read through a row table in LDS (rows past
//                               the group: -1, zero-filled), their weights through the same table; the 128 columns of a tile
//                               through `items`.  tk_scan with both row functors, then tk_tile_scores, composed as tk_tile
//                               composes them (search_scan.h) -- the bf16 hi / lo query pair, the fp8 widening and scale
//                               included -- so a pair has the score bits every scan gives it.  Selection is the running top-k
//                               of search_topk.h (tk_push) with the key's index taken from the item table.  Each row flushes
//                               its sorted k keys into a slot of its own, ws [row][probe slot][piece][k].
//   topk_merge_kernel         : the chunk merge of search.hip over the P * pieces lists of a row (tk_merge_launch).  It has
//                               no cap on the number of lists: past 64 KiB of keys per row it reads them from memory.
// The workspace is zeroed first (a list nobody writes is empty) and the outputs are filled with (-inf, -1): the merge writes
// the slots that have a candidate.  Items of different cells are different items, so every key of a row is distinct and the
// merge by rank applies the one order -- score descending, -0 tied with +0, equal scores by ascending ITEM NUMBER -- across
// cells as within them; the result depends on a row's probes as a set, not on their order, the other rows, or how pairs fell
// into groups.  No atomics; every slot has one writer.  A work item or a pair the tables do not back (a number outside its
// range) is dropped on the device and never dereferenced.
//
// LDS: slab / score-tile union + 4 KiB query weights + row and slot tables (2 x 256 B) + two item tables (2 x 512 B: the
// next tile's items are loaded during the K loop of the current one and written between its two closing barriers) + counts,
// thresholds and candidates of the running top-k.  k = 128 passes the 64 KiB default: cl_lds_limits.
#include <type_traits>

#include "search_topk.h"

#define CL_PIECE MMT_SEARCH_CELL_PIECE  // items of a cell one block walks (16 tiles): a larger cell is cut into pieces
#define CL_MAXP MMT_SEARCH_MAX_PROBES   // probes per query row
#define CL_WORK 5                       // int32 words per work item

struct ClArgs {
  const void* q;              // fp32: Q' [NQ][K]; bf16: hi(Q')
  const void* q_lo;           // bf16: lo(Q')
  const float* qw;            // [NQ][M]
  const void* g;              // [NV][K] fp32, bf16 bits or e4m3fn codes
  const float* gw;            // [NV][M]
  const int64_t* items;       // [n_items] item numbers, cell after cell
  const int32_t* work;        // [n_work][CL_WORK]
  const int32_t* pair_row;    // [n_pairs]
  const int32_t* pair_slot;   // [n_pairs]
  uint64_t* ws;               // [NQ][P][pieces][k]
  int NQ, NV, M, K, k, P, pieces, n_items, n_pairs;
};

struct ClFp8Args : ClArgs {
  const float* gscale;        // [NV]
  static constexpr bool kFp8 = true;
};

// tk_tile_select (search_topk.h) with the item of a column taken from the tile's item table (-1 = no item) in place of
// g0 + col: wave w owns rows 16w .. 16w + 15, lane l offers columns l and 64 + l.
__device__ __forceinline__ void cl_tile_select(const float* sS, uint64_t* sC, int* sN, uint64_t* sT, int k, int rows_live,
                                               const int* sItem, int wave, int lane) {
  const int cap = k + 64;
  const int i0 = sItem[lane], i1 = sItem[64 + lane];
  for (int rr = 0; rr < TK_Q / 4; ++rr) {
    const int row = wave * (TK_Q / 4) + rr;
    if (row >= rows_live) break;
    int n = sN[row];
    uint64_t thr = sT[row];
    tk_push(sC + row * cap, n, thr, k, i0 >= 0 ? tk_key(sS[row * TK_SLD + lane], i0) : 0ull, lane);
    tk_push(sC + row * cap, n, thr, k, i1 >= 0 ? tk_key(sS[row * TK_SLD + 64 + lane], i1) : 0ull, lane);
    if (lane == 0) { sN[row] = n; sT[row] = thr; }
  }
}

template <bool BF16, class Args>
__global__ __launch_bounds__(256) void cells_scan_kernel(Args a) {
  constexpr bool FP8 = TkFp8<Args>::value;
  static_assert(!FP8 || BF16, "an fp8 gallery is scanned with the bf16 query pair");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int kUnion = BF16 ? TKB_UNION_BYTES : TK_UNION_BYTES;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, h = lane >> 5, wq = wave >> 1, wg = wave & 1;
  const int32_t* w = a.work + (int64_t)blockIdx.x * CL_WORK;
  const int p0 = w[0], rows = w[1], i0 = w[2], i1 = w[3], piece = w[4];
  // block-uniform, before any barrier: a slot of the grid's upper bound past the call's work items (rows = 0), or a work
  // item the tables do not back
  if (rows < 1 || rows > TK_Q || p0 < 0 || p0 > a.n_pairs - rows || i0 < 0 || i1 > a.n_items || i0 >= i1 ||
      i1 - i0 > CL_PIECE || piece < 0 || piece >= a.pieces)
    return;
  const int cap = a.k + 64;

  float* sS = (float*)smem;                                   // [TK_Q][TK_SLD]  scores (after the K loop)
  float* sQw = (float*)(smem + kUnion);                       // [TK_Q][MMT_MAX_EXPERTS]
  int* sRow = (int*)(sQw + TK_Q * MMT_MAX_EXPERTS);           // [TK_Q] query row of the block's rows, -1 = none
  int* sSlot = sRow + TK_Q;                                   // [TK_Q] their probe slots
  int* sItem = sSlot + TK_Q;                                  // [2][TK_G] items of the current and the next tile, -1 = none
  int* sN = sItem + 2 * TK_G;                                 // [TK_Q] candidates held
  uint64_t* sT = (uint64_t*)(sN + TK_Q);                      // [TK_Q] thresholds
  uint64_t* sC = sT + TK_Q;                                   // [TK_Q][cap] candidates

  const int64_t* items = a.items;
  const int NV = a.NV;
  const auto item_at = [=](int i) {  // position i of the item table -> the item, -1 past the piece or outside 0 .. NV - 1
    if (i >= i1) return -1;
    const int64_t v = items[i];
    return v >= 0 && v < NV ? (int)v : -1;
  };
  if (tid < TK_Q) {
    int r = -1, s = 0;
    if (tid < rows) {
      r = a.pair_row[p0 + tid];
      s = a.pair_slot[p0 + tid];
      if (r < 0 || r >= a.NQ || s < 0 || s >= a.P) r = -1;
    }
    sRow[tid] = r;
    sSlot[tid] = s;
    sN[tid] = 0;
    sT[tid] = 0;
  }
  if (tid < TK_G) sItem[tid] = item_at(i0 + tid);
  __syncthreads();
  for (int i = tid; i < TK_Q * MMT_MAX_EXPERTS; i += 256) {  // the rows' weights through the row table, zero past rows / M
    const int r = sRow[i / MMT_MAX_EXPERTS], m = i % MMT_MAX_EXPERTS;
    sQw[i] = (r >= 0 && m < a.M) ? a.qw[(int64_t)r * a.M + m] : 0.f;   // read behind the barriers of tk_scan
  }
  const auto arow = [=](int r) { return sRow[r]; };
  int t = 0;
  for (int g0 = i0; g0 < i1; g0 += TK_G, t ^= 1) {
    const int* it = sItem + t * TK_G;
    const auto grow = [=](int c) { return it[c]; };
    // the next tile's items: in flight during this tile's K loop
    const int nxt = (tid < TK_G && g0 + TK_G < i1) ? item_at(g0 + TK_G + tid) : -1;
    f32x16 acc[2];
    if constexpr (BF16)  // the query as two bf16 planes, hi then lo: tk_tile's composition
      tk_scan(acc, smem, {(const bf16_t*)a.q, (const bf16_t*)a.q_lo}, arow,
              (const std::conditional_t<FP8, uint8_t, bf16_t>*)a.g, grow, a.K, tid, wq, wg, l31, h);
    else
      tk_scan(acc, smem, {(const float*)a.q}, arow, (const float*)a.g, grow, a.K, tid, wq, wg, l31, h);
    __syncthreads();  // the slabs become the score tile
    // Between the K loop's barriers and the one below: the table the tile BEFORE this one used -- its last readers, that
    // tile's selection, are behind this tile's K loop -- becomes the next tile's, whose first readers are behind the barrier
    // below.
    if (tid < TK_G) sItem[(t ^ 1) * TK_G + tid] = nxt;
    if constexpr (FP8)
      tk_tile_scores<true>(acc, sS, sQw, a.gw, a.M, grow, wq, wg, l31, h, a.gscale);
    else
      tk_tile_scores(acc, sS, sQw, a.gw, a.M, grow, wq, wg, l31, h);
    __syncthreads();
    cl_tile_select(sS, sC, sN, sT, a.k, rows, it, wave, lane);
  }
  __syncthreads();
  for (int rr = 0; rr < TK_Q / 4; ++rr) {
    const int row = wave * (TK_Q / 4) + rr;
    if (row >= rows) break;
    const int q = sRow[row];
    if (q < 0) continue;  // wave-uniform
    tk_flush(sC + row * cap, sN[row], a.k, lane, a.ws + (((int64_t)q * a.P + sSlot[row]) * a.pieces + piece) * a.k);
  }
}

// (-inf, -1) into every output slot: the merge writes the slots that have a candidate.
__global__ __launch_bounds__(256) void cells_vacant_kernel(float* __restrict__ scores, int64_t* __restrict__ index, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  scores[i] = -__builtin_inff();
  index[i] = -1;
}

namespace {
// a row's lists: P * pieces * k keys, counted as int by the merge
bool cl_sizes_ok(int NQ, int P, int pieces, int k) {
  return NQ > 0 && P >= 1 && P <= CL_MAXP && pieces >= 1 && k >= 1 && k <= TK_MAXK && (int64_t)P * pieces * k < (1ll << 31);
}

// LDS behind the slab / score-tile union: query weights, row and slot tables, two item tables, counts, thresholds, candidates
constexpr size_t cl_state_lds(int k) {
  return TK_QW_BYTES + 2 * TK_Q * 4 + 2 * TK_G * 4 + TK_Q * (4 + 8) + (size_t)TK_Q * (k + 64) * 8;
}
static_assert(TKB_UNION_BYTES + cl_state_lds(TK_MAXK) <= 160 * 1024 && TK_UNION_BYTES + cl_state_lds(TK_MAXK) <= 160 * 1024,
              "the k = 128 footprint fits the 160 KiB of a CU");

// The k = 128 footprint is over the 64 KiB default.
void cl_lds_limits() {
  static bool done[64] = {};
  const size_t f32 = TK_UNION_BYTES + cl_state_lds(TK_MAXK), bf16 = TKB_UNION_BYTES + cl_state_lds(TK_MAXK);
  tk_lds_limits(done, {{(const void*)cells_scan_kernel<false, ClArgs>, f32},
                       {(const void*)cells_scan_kernel<true, ClArgs>, bf16},
                       {(const void*)cells_scan_kernel<true, ClFp8Args>, bf16}});
}

template <bool BF16, class Args>
int cl_search(const MmtSearchScan& s, const int64_t* items, int n_items, const int32_t* work, int n_work,
              const int32_t* pair_row, const int32_t* pair_slot, int n_pairs, int P, int pieces, int k, uint64_t* ws,
              float* scores, int64_t* index, void* stream) {
  constexpr bool FP8 = TkFp8<Args>::value;
  if (!tk_scan_operands<BF16, FP8>(s) || !items || !work || !pair_row || !pair_slot || !ws || !scores || !index ||
      n_items < 1 || n_work < 1 || n_pairs < 1 || !cl_sizes_ok(s.NQ, P, pieces, k) ||
      !tk_shape_ok(s.NQ, s.NV, s.M, s.d, BF16, FP8))
    return MMT_ERR_ARG;
  if (!tk_scan_aligned(s)) return MMT_ERR_ALIGN;  // (no subset here: the gate of the entry refused one)
  Args a = {};
  a.q = s.q; a.q_lo = s.q_lo; a.qw = s.qw; a.g = s.g; a.gw = s.gw;
  if constexpr (FP8) a.gscale = s.gscale;
  a.items = items; a.work = work; a.pair_row = pair_row; a.pair_slot = pair_slot; a.ws = ws;
  a.NQ = s.NQ; a.NV = s.NV; a.M = s.M; a.K = s.M * s.d; a.k = k; a.P = P; a.pieces = pieces;
  a.n_items = n_items; a.n_pairs = n_pairs;
  const hipStream_t st = (hipStream_t)stream;
  const int lists = P * pieces;
  if (const int rc = (int)hipMemsetAsync(ws, 0, (size_t)s.NQ * lists * k * 8, st)) return rc;
  const int64_t slots = (int64_t)s.NQ * k;
  hipLaunchKernelGGL(cells_vacant_kernel, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, st, scores, index, slots);
  cl_lds_limits();
  const size_t lds = (BF16 ? TKB_UNION_BYTES : TK_UNION_BYTES) + cl_state_lds(k);
  hipLaunchKernelGGL((cells_scan_kernel<BF16, Args>), dim3(n_work), dim3(256), lds, st, a);
  if (const int rc = (int)hipGetLastError()) return rc;
  return tk_merge_launch(ws, s.NQ, lists, k, k, scores, index, st);
}
}  // namespace

extern "C" int64_t mmt_topk_cells_workspace_keys(int NQ, int P, int pieces, int k) {
  if (!cl_sizes_ok(NQ, P, pieces, k)) return MMT_ERR_ARG;
  return (int64_t)NQ * P * pieces * k;
}

extern "C" int mmt_search_topk_cells(const MmtSearchScan* scan, const int64_t* items, int n_items, const int32_t* work,
                                     int n_work, const int32_t* pair_row, const int32_t* pair_slot, int n_pairs, int P,
                                     int pieces, int k, uint64_t* ws, float* scores, int64_t* index, void* stream) {
  if (const int rc = tk_scan_gate(scan, SC_FP8)) return rc;
  switch (scan->storage) {
    case MMT_SEARCH_FP32:
      return cl_search<false, ClArgs>(*scan, items, n_items, work, n_work, pair_row, pair_slot, n_pairs, P, pieces, k, ws,
                                      scores, index, stream);
    case MMT_SEARCH_BF16:
      return cl_search<true, ClArgs>(*scan, items, n_items, work, n_work, pair_row, pair_slot, n_pairs, P, pieces, k, ws,
                                     scores, index, stream);
    default:
      return cl_search<true, ClFp8Args>(*scan, items, n_items, work, n_work, pair_row, pair_slot, n_pairs, P, pieces, k, ws,
                                        scores, index, stream);
  }
}
