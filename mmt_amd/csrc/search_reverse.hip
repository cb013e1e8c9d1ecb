// Reverse search: for every stored ITEM the k best query rows (search.py: reverse_search, and csls_norm, whose per-item
// term is the mean of that list).  The one reduction of the scans that runs per item over all queries and keeps more than
// a number: a running top-k per item over a stream of query rows, 1 <= k <= MMT_SEARCH_MAX_RK = 32.  Nothing here forms a
// query x gallery matrix.
//
//   key(q, g)  = tk_key(score(q, g), q)      the search's key with the global ROW number in the index field: score
//                                            descending, -0 tied with +0, equal scores by ascending query row
//   list[g]    = the k largest keys of item g over all query rows, descending
//   mean[g]    = fl(fl(.. fl(s_0 + s_1) .. + s_{k'-1}) * w)     s_i = list[g]'s scores in list order, k' = min(k, rows),
//                                            w = float32(1 / k') from the caller: rounded adds, one rounded multiply, no
//                                            fma and no division, so numpy float32 restates it bit for bit
//
// with score the value of the plain scan, bit for bit: the kernel scores its tile with the K loops and the epilogue of
// search_scan.h (tk_tile<., false>) and the query rows as the QUERY operand, on all three storages (an fp8 gallery through
// an argument block that says kFp8 and carries gscale, as the other scans).
//
//   col_topk_kernel<BF16, Args> : col_lse_kernel's geometry (block = 64 query rows x one gallery chunk, tk_geometry, the
//                                 XCD remap) with the column pass replaced: per 64 x 128 score tile in LDS a wave takes
//                                 32 columns, four at a time; lane r reads row r's four scores with one 16-byte read,
//                                 turns them into keys (0 for a row past the batch's end), parks the keys in 2 KiB of
//                                 LDS of the wave's own and rank-sorts each column's 64 keys directly -- rank = the number
//                                 of keys above mine, 64 broadcast reads and 64-bit compares -- so lane r writes its key
//                                 to slot rank of part[query block][item][k] when rank < k; slots past the live rows get
//                                 0.  One writer per slot, no atomics, no per-thread list.
//   col_topk_fold_kernel        : one wave per item: the carried list in state [NV][k] (ignored when `first`) and this
//                                 batch's n_qt partial lists stream 64 keys at a time through tk_push into k + 64 <= 96
//                                 keys of LDS; the best k go back to state and, when asked, out as scores / rows / mean.
//
// Schedule: "queries in batches" (DESIGN 9.5, 9.16): the rows stream through in batches of whole 64-row blocks, a launch
// fills the chip whatever the gallery size, and the partial lists are bounded by the caller's batch.
//
// Why the result depends on the item, the query rows and k only: keys of distinct rows are distinct (the row number is
// part of the key) and a score does not depend on NV, the item's position, the chunk or the shard, so "the k largest keys
// of a union of rows" is one well-defined set however the rows were cut into blocks and batches; every step here (the
// block's rank sort, tk_push / tk_compact of the fold) returns exactly the k largest of what it is given, and the k
// largest of a union are among the k largest of its parts.  The mean is a fixed chain over that list in list order.
//
// The column read: 64 lanes reading one column of sS at the row pitch TK_SLD = 132 floats would meet on 16 banks
// ((4 r + c) mod 64: 4-way).  Reading four columns as one ds_read_b128 avoids it (a 16-lane group of that instruction
// covers rows whose 16-byte slots 4 r mod 64 are all distinct), but it would not matter either way: a tile's column pass
// issues 32 such reads per wave against 64 broadcast reads and compares per COLUMN in the rank loop right behind them,
// and against K = M d multiply-adds per score in the K loop before.
#include "search_topk.h"

#define CT_MAXK MMT_SEARCH_MAX_RK
#define CT_U 4                                   // columns a wave ranks at a time
#define CT_KEYS_BYTES (4 * CT_U * 64 * 8)        // the waves' parked keys

struct CtArgs {
  const void* q;        // fp32: Q' [NQ][K]; bf16 / fp8: hi(Q')
  const void* q_lo;     // bf16 / fp8: lo(Q')
  const float* qw;      // [NQ][M]
  const void* g;        // [NV][K] in the storage's form
  const float* gw;      // [NV][M]
  int NQ, NV, M, K, chunk, n_qt, n_chunks;
  int k, row0;          // list length; global number of the batch's first row
};

struct CtFp8Args : CtArgs {
  const float* gscale;  // [NV]
  static constexpr bool kFp8 = true;
};

// The column pass of one score tile: part -> this query block's lists [NV][k]; row_base = the global number of tile row 0.
__device__ __forceinline__ void ct_tile_cols(const float* sS, uint64_t* sK, uint64_t* __restrict__ part, int k, int rows_live,
                                             int row_base, int g0, int g_end, int wave, int lane) {
  const bool live = lane < rows_live;
  for (int cc = 0; cc < TK_G / 4; cc += CT_U) {
    const int c = wave * (TK_G / 4) + cc;
    if (g0 + c >= g_end) break;  // wave-uniform
    const f32x4 s = *(const f32x4*)(sS + lane * TK_SLD + c);
    uint64_t key[CT_U];
    int rk[CT_U];
#pragma unroll
    for (int u = 0; u < CT_U; ++u) {
      key[u] = live ? tk_key(s[u], row_base + lane) : 0ull;
      sK[u * 64 + lane] = key[u];
      rk[u] = 0;
    }
    __builtin_amdgcn_wave_barrier();  // one wave: LDS ops stay in order
    // all 64 slots, eight at a time so that the broadcast reads of a group are in flight together (a dead row's 0 is
    // above nothing)
#pragma unroll 8
    for (int j = 0; j < TK_Q; ++j) {
#pragma unroll
      for (int u = 0; u < CT_U; ++u) rk[u] += sK[u * 64 + j] > key[u];
    }
    __builtin_amdgcn_wave_barrier();  // the reads above precede the next group's keys
#pragma unroll
    for (int u = 0; u < CT_U; ++u) {
      const int g = g0 + c + u;
      if (g < g_end) {
        uint64_t* dst = part + (int64_t)g * k;
        if (live && rk[u] < k) dst[rk[u]] = key[u];
        if (lane < k && lane >= rows_live) dst[lane] = 0ull;
      }
    }
  }
}

template <bool BF16, class Args>
__global__ __launch_bounds__(256) void col_topk_kernel(Args a, uint64_t* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int kUnion = BF16 ? TKB_UNION_BYTES : TK_UNION_BYTES;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, h = lane >> 5, wq = wave >> 1, wg = wave & 1;
  const int bid = xcd_remap(blockIdx.x, gridDim.x);  // gallery-chunk-major, as the top-k kernel
  const int chunk = bid / a.n_qt, qt = bid % a.n_qt, q0 = qt * TK_Q;
  const int g_begin = chunk * a.chunk, g_end = min(a.NV, g_begin + a.chunk);
  const int rows_live = min(a.NQ - q0, TK_Q);
  float* sS = (float*)smem;                       // [TK_Q][TK_SLD]  scores (after the K loop)
  float* sQw = (float*)(smem + kUnion);           // [TK_Q][MMT_MAX_EXPERTS]
  uint64_t* sK = (uint64_t*)(smem + kUnion + TK_QW_BYTES) + wave * (CT_U * 64);   // [CT_U][64] keys of the wave's columns
  uint64_t* mine = part + (int64_t)qt * a.NV * a.k;
  tk_load_qw(sQw, a.qw, a.NQ, a.M, q0, tid);
  for (int g0 = g_begin; g0 < g_end; g0 += TK_G) {
    tk_tile<BF16, false>(a, smem, sS, sQw, q0, [=](int r) { return g0 + r < g_end ? g0 + r : -1; }, tid, wq, wg, l31, h);
    ct_tile_cols(sS, sK, mine, a.k, rows_live, a.row0 + q0, g0, g_end, wave, lane);
  }
}

// state: [NV][k] keys, descending, 0 = empty.  first: the state is not read.  One wave per item.
__global__ __launch_bounds__(256) void col_topk_fold_kernel(const uint64_t* __restrict__ part, int n_blocks, int NV, int k,
                                                            uint64_t* __restrict__ state, int first,
                                                            float* __restrict__ scores, int64_t* __restrict__ rows,
                                                            float* __restrict__ mean, float mean_weight) {
  __shared__ uint64_t sC[4][CT_MAXK + 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = blockIdx.x * 4 + wave;
  if (g >= NV) return;  // wave-uniform; no block barrier below
  uint64_t* c = sC[wave];
  int n = 0;
  uint64_t thr = 0ull;  // an empty slot's 0 is never taken
  if (!first) tk_push(c, n, thr, k, lane < k ? state[(int64_t)g * k + lane] : 0ull, lane);
  const int total = n_blocks * k;
  for (int t = 0; t < total; t += 64) {
    const int i = t + lane;
    uint64_t key = 0ull;
    if (i < total) key = part[((int64_t)(i / k) * NV + g) * k + i % k];
    tk_push(c, n, thr, k, key, lane);
  }
  tk_flush(c, n, k, lane, state + (int64_t)g * k);
  const int have = n < k ? n : k;
  if (lane < k) {
    const uint64_t key = lane < have ? c[lane] : 0ull;
    if (scores) scores[(int64_t)g * k + lane] = lane < have ? tk_score(key) : -INFINITY;
    if (rows) rows[(int64_t)g * k + lane] = lane < have ? (int64_t)tk_index(key) : -1;
  }
  if (mean && lane == 0) {
    float v = have ? tk_score(c[0]) : 0.f;
    for (int i = 1; i < have; ++i) v = tk_add_rn(v, tk_score(c[i]));
    mean[g] = tk_mul_rn(v, mean_weight);
  }
}

namespace {
inline bool ct_sizes_ok(int NB, int NV, int k) { return NB > 0 && NV > 0 && k >= 1 && k <= CT_MAXK; }

template <bool BF16, class Args>
int ct_col_topk(const MmtSearchScan& s, int k, int row0, uint64_t* ws, uint64_t* state, int first, float* scores,
                int64_t* rows, float* mean, float mean_weight, void* stream) {
  constexpr bool FP8 = TkFp8<Args>::value;
  if (!tk_scan_operands<BF16, FP8>(s) || !ws || !state || !tk_shape_ok(s.NQ, s.NV, s.M, s.d, BF16, FP8) ||
      !ct_sizes_ok(s.NQ, s.NV, k) || row0 < 0 || (int64_t)row0 + s.NQ > INT32_MAX)
    return MMT_ERR_ARG;
  if (!tk_scan_aligned(s) || (((uintptr_t)ws | (uintptr_t)state) & 15)) return MMT_ERR_ALIGN;
  Args a = {};
  a.q = s.q; a.q_lo = s.q_lo; a.qw = s.qw; a.g = s.g; a.gw = s.gw;
  if constexpr (FP8) a.gscale = s.gscale;
  a.NQ = s.NQ; a.NV = s.NV; a.M = s.M; a.K = s.M * s.d; a.k = k; a.row0 = row0;
  tk_geometry(a);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL((col_topk_kernel<BF16, Args>), dim3(a.n_qt * a.n_chunks), dim3(256), tk_base_lds<BF16>() + CT_KEYS_BYTES,
                     st, a, ws);
  hipLaunchKernelGGL(col_topk_fold_kernel, dim3((s.NV + 3) / 4), dim3(256), 0, st, (const uint64_t*)ws, a.n_qt, s.NV, k, state,
                     first, scores, rows, mean, mean_weight);
  return (int)hipGetLastError();
}
}  // namespace

extern "C" int64_t mmt_col_topk_workspace_keys(int NB, int NV, int k) {
  if (!ct_sizes_ok(NB, NV, k)) return MMT_ERR_ARG;
  return (int64_t)((NB + TK_Q - 1) / TK_Q) * NV * k;
}

// The descriptor takes no options: all three storages, no other part.
extern "C" int mmt_search_col_topk(const MmtSearchScan* scan, int k, int row0, uint64_t* ws, uint64_t* state, int first,
                                   float* scores, int64_t* rows, float* mean, float mean_weight, void* stream) {
  if (const int rc = tk_scan_gate(scan, SC_FP8)) return rc;
  switch (scan->storage) {
    case MMT_SEARCH_FP32:
      return ct_col_topk<false, CtArgs>(*scan, k, row0, ws, state, first, scores, rows, mean, mean_weight, stream);
    case MMT_SEARCH_BF16:
      return ct_col_topk<true, CtArgs>(*scan, k, row0, ws, state, first, scores, rows, mean, mean_weight, stream);
    default:
      return ct_col_topk<true, CtFp8Args>(*scan, k, row0, ws, state, first, scores, rows, mean, mean_weight, stream);
  }
}
