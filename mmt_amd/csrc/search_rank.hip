// Exact retrieval ranks without the N_query x N_gallery matrix (reference: model/metric.py:90-121 t2v_metrics,
// 153-243 v2t_metrics -- the tie-averaged rank of the ground truth in a row of sims).
//
// For a query q and a target item t the rank is  #{g : score(q, g) > score(q, t)} + (#{g : score(q, g) == score(q, t)} - 1) / 2.
// The two counts come from the scan the top-k search does (search_scan.h: same tile, same gated denominator, same chunk
// rule) with a counter per (query, target) in place of a running top-k list.  Three launches, T <= 32 targets per query:
//   rank_kernel<BF16, true, .>: thresholds.  thr[q][t] = score(q, targets[q][t]) from the SAME scoring tile with a
//                               gallery-row indirection: block = 64 queries x 128 (query, target) pairs, tile column c of
//                               block (qt, j) holds the gallery row of pair p = 128 j + c, i.e. of query p / T, target
//                               p % T; only the entry on that query's own row is kept.  The K order of an MFMA output
//                               element does not depend on its column, the denominator is the same code on the same
//                               operands, so an item compares equal to itself in the count pass (checked by the tests
//                               against search(k = 128), which returns the scan's own scores).  A target outside 0 .. NV - 1
//                               (-1 = none) is never dereferenced; its threshold is NaN, which counts nothing.
//   rank_kernel<BF16, false, .>: counts.  Block = 64 queries x one gallery chunk, as the top-k kernel.  Per 64 x 128 score
//                               tile in LDS a wave takes its 16 rows; per row, lane t holds threshold t, the wave
//                               broadcasts one threshold at a time and counts `score > thr` / `score == thr` over the live
//                               columns with two ballots each (plain float compares: -0 == +0, NaN counts for nothing);
//                               lane t keeps the sums of threshold t in LDS.  (greater, equal) per (query, target, chunk)
//                               go to the workspace.
//   rank_reduce_kernel        : sums the chunks, in chunk order.
// No atomics, integer sums only, every slot has one writer: bit-reproducible.  LDS at T = 32: score tile / slab union +
// 4 KiB query weights + 24 KiB thresholds and counters, against the 97 KiB of candidate lists of the top-k kernel at
// k = 128; registers: the top-k kernel's K loop plus four counters.
//
// rank_kernel<BF16, false, RkMaskedArgs> is the masked count pass (mmt_search_rank [subset]): only items whose bit is set in a packed
// bitmap (search_subset.hip) are counted -- the live-column predicate ANDed with the tile's 128 bits, one block-uniform
// 16-byte load per tile, and a tile without a set bit skipped before its K loop.  Thresholds and the reduce are the
// unmasked ones, so a target outside the subset is still scored; it just does not count itself.
//
// mmt_search_thresholds / mmt_search_count (and their bf16 forms) launch the threshold pass alone and the count pass +
// reduce against given thresholds: the same instantiations with the same argument blocks.  A gallery cut into shards
// scores a target where it is stored and counts it on every shard (search.py: ShardedVideoIndex); the int32 counts add.
//
// rank_kernel<BF16, THR, NmRankArgs> (mmt_search_thresholds [lse] / mmt_search_count [lse]) is the same pair of passes on
// the querybank-normalised score' (search_norm.hip): the tile is rewritten by tk_tile_norm before it is read, the subset
// of the count pass is a pointer that may be null.  rank_kernel is ONE body, generic over its argument block, which says
// how the subset and the normalisation enter (kMask, kNorm: search_scan.h); the blocks stay separate types because a
// field appended to RkArgs moves the hidden kernel arguments behind it and changes the unmasked code
// (profiles/search_subset_kernel_identity.txt).
#include <type_traits>

#include "search_scan.h"

#define RK_MAXT 32

struct RkArgs {
  const void* q;           // fp32: Q' [NQ][K]; bf16: hi(Q')
  const void* q_lo;        // bf16: lo(Q')
  const float* qw;         // [NQ][M]
  const void* g;           // [NV][K] fp32 or bf16 bits
  const float* gw;         // [NV][M]
  const int64_t* targets;  // [NQ][T]
  float* thr;              // [NQ][T]
  int32_t* cnt;            // [NQ][T][n_chunks][2]
  int NQ, NV, M, K, T, chunk, n_qt, n_chunks;
  static constexpr TkMask kMask = TK_MASK_NONE;
  static constexpr bool kNorm = false;
};

// The masked count pass takes an argument type of its own, so the unmasked kernels keep their argument block (and with
// it their code) byte for byte.
struct RkMaskedArgs : RkArgs {
  const uint32_t* subset;  // bit g & 31 of word g >> 5 allows item g (16-byte aligned)
  static constexpr TkMask kMask = TK_MASK_SET;
};

// A gallery stored in fp8 (search_fp8.hip): e4m3fn codes behind g, one power-of-two scale per item; the block says so in
// kFp8 (search_scan.h: TkFp8).
struct RkFp8Args : RkArgs {
  const float* gscale;     // [NV]
  static constexpr bool kFp8 = true;
};

struct RkFp8MaskedArgs : RkFp8Args {  // as RkMaskedArgs
  const uint32_t* subset;
  static constexpr TkMask kMask = TK_MASK_SET;
};

// The filtered count pass (mmt_search_count_where): the masked blocks with a tag word per item and three masks per query
// row behind them (search_scan.h: tk_tag_pass); the subset may be null here.  An item is counted for a row only if its
// tags pass the row's masks; thresholds come from the unfiltered threshold pass, so a target is scored whether or not it
// passes and counts itself only if it does.
struct RkWhereArgs : RkMaskedArgs {
  const uint64_t* tags;    // [NV]
  const uint64_t* where;   // [NQ][3]: all_of, none_of, any_of
  static constexpr TkMask kMask = TK_MASK_NULLABLE;
  static constexpr bool kWhere = true;
};

struct RkFp8WhereArgs : RkFp8MaskedArgs {  // as RkWhereArgs
  const uint64_t* tags;
  const uint64_t* where;
  static constexpr TkMask kMask = TK_MASK_NULLABLE;
  static constexpr bool kWhere = true;
};

// The unmasked block of a masked one: what the threshold pass and a count pass without a subset are launched with.
template <class Args>
using RkPlain = std::conditional_t<TkFp8<Args>::value, RkFp8Args, RkArgs>;

struct NmRankArgs : NmArgs {
  const int64_t* targets;   // THR: [NQ][T]
  float* thr;               // [NQ][T]
  int32_t* cnt;             // count: [NQ][T][n_chunks][2]
  const uint32_t* subset;   // count: nullable = all
  int T;
};

// The threshold pass (THR) or the count pass of one block, on the plain score or (Args::kNorm) on score'; Args = RkArgs,
// RkMaskedArgs, their fp8 forms or NmRankArgs.
template <bool BF16, bool THR, class Args>
__global__ __launch_bounds__(256) void rank_kernel(Args a) {
  constexpr TkMask MASK = Args::kMask;
  constexpr bool NORM = Args::kNorm;
  constexpr bool WHERE = TkWhere<Args>::value;
  static_assert(!WHERE || (!THR && !NORM && MASK == TK_MASK_NULLABLE), "the filter belongs to the plain count pass");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int kUnion = BF16 ? TKB_UNION_BYTES : TK_UNION_BYTES;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, h = lane >> 5, wq = wave >> 1, wg = wave & 1;
  const int T = a.T;
  float* sS = (float*)smem;                       // [TK_Q][TK_SLD]  scores (after the K loop)
  float* sQw = (float*)(smem + kUnion);           // [TK_Q][MMT_MAX_EXPERTS]
  if constexpr (THR) {
    int* sRow = (int*)(sQw + TK_Q * MMT_MAX_EXPERTS);  // [TK_G] gallery row of the tile's columns
    const int q0 = (blockIdx.x % a.n_qt) * TK_Q, p0 = (blockIdx.x / a.n_qt) * TK_G;
    const int64_t pairs = ((int64_t)min(a.NQ - q0, TK_Q)) * T;  // live (query, target) pairs of this query tile
    tk_load_qw(sQw, a.qw, a.NQ, a.M, q0, tid);
    if (tid < TK_G) {
      const int64_t tg = p0 + tid < pairs ? a.targets[(int64_t)q0 * T + p0 + tid] : -1;
      sRow[tid] = (tg >= 0 && tg < a.NV) ? (int)tg : -1;
    }
    __syncthreads();
    tk_tile<BF16, NORM>(a, smem, sS, sQw, q0, [=](int r) { return sRow[r]; }, tid, wq, wg, l31, h);
    if (tid < TK_G && p0 + tid < pairs)
      a.thr[(int64_t)q0 * T + p0 + tid] = sRow[tid] >= 0 ? sS[((p0 + tid) / T) * TK_SLD + tid] : __builtin_nanf("");
  } else {
    float* sThr = sQw + TK_Q * MMT_MAX_EXPERTS;   // [TK_Q][T]
    int* sCnt = (int*)(sThr + TK_Q * T);          // [TK_Q][T][2]
    const int bid = xcd_remap(blockIdx.x, gridDim.x);  // gallery-chunk-major: an XCD's blocks share their chunk in L2
    const int chunk = bid / a.n_qt, q0 = (bid % a.n_qt) * TK_Q;
    const int g_begin = chunk * a.chunk, g_end = min(a.NV, g_begin + a.chunk);
    const int rows_live = min(a.NQ - q0, TK_Q);
    tk_load_qw(sQw, a.qw, a.NQ, a.M, q0, tid);
    for (int i = tid; i < TK_Q * T; i += 256) {
      sThr[i] = i < rows_live * T ? a.thr[(int64_t)q0 * T + i] : 0.f;
      sCnt[2 * i] = 0;
      sCnt[2 * i + 1] = 0;
    }
    uint64_t* sW = nullptr;  // filtered: [TK_Q][3] masks behind the counters (TK_Q * T * 12 bytes: 8-byte aligned)
    TkWhereGate gate;        // what the rows' masks share, the tags a tile ahead
    TkTagStream stream;
    if constexpr (WHERE) {
      sW = (uint64_t*)(sCnt + 2 * TK_Q * T);
      tk_load_where<TK_Q>(sW, a.where, a.NQ, q0, tid);
      gate.template init<TK_Q>(a.where, a.NQ, q0, lane);
      stream.init(a.tags, g_begin, g_end, lane);
    }
    if constexpr (MASK != TK_MASK_NONE) __syncthreads();  // every tile may be skipped: the counters are read below all the same
    for (int g0 = g_begin; g0 < g_end; g0 += TK_G) {
      uint64_t m0 = ~0ull, m1 = ~0ull, t0 = 0, t1 = 0;
      if constexpr (WHERE) stream.next(a.tags, g0, g_end, lane, t0, t1);  // before any skip: the next tile's are asked for
      if constexpr (MASK != TK_MASK_NONE)
        if ((MASK == TK_MASK_SET || a.subset) && !tk_tile_mask(a.subset, g0, m0, m1)) continue;  // block-uniform
      if constexpr (WHERE) {
        if (!tk_tile_where_any<TK_Q>(gate, sW, rows_live, t0, t1, g0 + lane < g_end && ((m0 >> lane) & 1ull),
                                     g0 + 64 + lane < g_end && ((m1 >> lane) & 1ull), wave))
          continue;  // block-uniform: no live row has an item to count in this tile
      }
      tk_tile<BF16, NORM>(a, smem, sS, sQw, q0, [=](int r) { return g0 + r < g_end ? g0 + r : -1; }, tid, wq, wg, l31, h);
      // wave w owns rows 16w .. 16w + 15 for the whole block, so its counters need no barrier
      const bool live0 = g0 + lane < g_end && (MASK == TK_MASK_NONE || ((m0 >> lane) & 1ull));
      const bool live1 = g0 + 64 + lane < g_end && (MASK == TK_MASK_NONE || ((m1 >> lane) & 1ull));
      if constexpr (WHERE) {
        if (gate.uniform)  // block-uniform: one predicate for all rows is one more term of the shared liveness
          tk_tile_count(sS, sThr, sCnt, T, rows_live, live0 && gate.common(t0), live1 && gate.common(t1), wave, lane);
        else
          tk_tile_count<true>(sS, sThr, sCnt, T, rows_live, live0, live1, wave, lane, sW, t0, t1);
      } else {
        tk_tile_count(sS, sThr, sCnt, T, rows_live, live0, live1, wave, lane);
      }
    }
    tk_count_flush(sCnt, a.cnt, T, rows_live, q0, a.n_chunks, chunk, wave, lane);
  }
}

// One thread per (query, target): the chunk counts summed in chunk order.
__global__ __launch_bounds__(256) void rank_reduce_kernel(const int32_t* __restrict__ cnt, int64_t n, int n_chunks,
                                                          int32_t* __restrict__ greater, int32_t* __restrict__ equal) {
  const int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x;
  if (i >= n) return;
  int g = 0, e = 0;
  for (int c = 0; c < n_chunks; ++c) {
    g += cnt[(i * n_chunks + c) * 2];
    e += cnt[(i * n_chunks + c) * 2 + 1];
  }
  greater[i] = g;
  equal[i] = e;
}

// The chunk reduce behind every count entry point (declared in search_scan.h: search_pool.hip sums the counters of its
// sets with it): cnt [n][n_chunks][2] -> greater [n], equal [n].
int rk_reduce_launch(const int32_t* cnt, int64_t n, int n_chunks, int32_t* greater, int32_t* equal, hipStream_t s) {
  hipLaunchKernelGGL(rank_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, cnt, n, n_chunks, greater, equal);
  return (int)hipGetLastError();
}

namespace {
bool rk_args_ok(int NQ, int NV, int T) { return NQ > 0 && NV > 0 && T >= 1 && T <= RK_MAXT; }

// The gate and the fill every entry point shares (Args = RkMaskedArgs, RkFp8MaskedArgs or NmRankArgs): 0, or the error
// code.  `own`: the entry's own pointers are all there.  `subset`: the descriptor's, or null for a pass that has none.
template <bool BF16, class Args>
int rk_fill(Args& a, const MmtSearchScan& s, int T, const uint32_t* subset, bool own) {
  constexpr bool FP8 = TkFp8<Args>::value;
  if constexpr (TkWhere<Args>::value) own = own && a.tags && a.where;  // set by the caller before the fill
  if (!tk_scan_operands<BF16, FP8, Args::kNorm>(s) || !own || !rk_args_ok(s.NQ, s.NV, T) ||
      !tk_shape_ok(s.NQ, s.NV, s.M, s.d, BF16, FP8))
    return MMT_ERR_ARG;
  if (((uintptr_t)s.q | (uintptr_t)s.q_lo | (uintptr_t)s.g | (uintptr_t)subset) & 15) return MMT_ERR_ALIGN;
  a.q = s.q; a.q_lo = s.q_lo; a.qw = s.qw; a.g = s.g; a.gw = s.gw; a.subset = subset;
  if constexpr (FP8) a.gscale = s.gscale;
  if constexpr (Args::kNorm) { a.beta = s.beta; a.lse = s.lse; }
  a.NQ = s.NQ; a.NV = s.NV; a.M = s.M; a.K = s.M * s.d; a.T = T;
  tk_geometry(a);
  return 0;
}

template <bool BF16, class Args>
void rk_launch_thresholds(const Args& a, hipStream_t s) {
  const int n_pt = (TK_Q * a.T + TK_G - 1) / TK_G;  // threshold tiles per query tile
  const dim3 grid(a.n_qt * n_pt);
  using Plain = std::conditional_t<Args::kNorm, Args, RkPlain<Args>>;  // the threshold pass has no subset
  hipLaunchKernelGGL((rank_kernel<BF16, true, Plain>), grid, dim3(256), tk_base_lds<BF16>() + TK_G * 4, s, (Plain)a);
}

// The count kernels' T = 32 footprint reaches the 64 KiB default limit (bf16: exactly).
template <bool BF16, bool FP8>
void rk_lds_limits() {
  static bool done[64] = {};
  constexpr size_t bytes = tk_base_lds<BF16>() + (size_t)TK_Q * RK_MAXT * 12;
  if constexpr (FP8)
    tk_lds_limits(done, {{(const void*)rank_kernel<BF16, false, RkFp8Args>, bytes},
                         {(const void*)rank_kernel<BF16, false, RkFp8MaskedArgs>, bytes}});
  else
    tk_lds_limits(done, {{(const void*)rank_kernel<BF16, false, RkArgs>, bytes},
                         {(const void*)rank_kernel<BF16, false, RkMaskedArgs>, bytes},
                         {(const void*)rank_kernel<BF16, false, NmRankArgs>, bytes}});
}

// The filtered count pass and the reduce: always the filtered instantiation, its masks behind the counters.
template <bool BF16, class Args>
int rk_count_where(const MmtSearchScan& s, const uint64_t* tags, const uint64_t* where, const float* thr, int T, int32_t* ws,
                   int32_t* greater, int32_t* equal, void* stream) {
  static bool done[64] = {};
  Args a = {};
  a.tags = tags; a.where = where;
  if (const int rc = rk_fill<BF16>(a, s, T, s.subset, thr && ws && greater && equal)) return rc;
  a.thr = const_cast<float*>(thr); a.cnt = ws;
  tk_lds_limits(done, {{(const void*)rank_kernel<BF16, false, Args>,
                        tk_base_lds<BF16>() + (size_t)TK_Q * RK_MAXT * 12 + TK_WHERE_BYTES(TK_Q)}});
  hipLaunchKernelGGL((rank_kernel<BF16, false, Args>), dim3(a.n_qt * a.n_chunks), dim3(256),
                     tk_base_lds<BF16>() + (size_t)TK_Q * a.T * 12 + TK_WHERE_BYTES(TK_Q), (hipStream_t)stream, a);
  return rk_reduce_launch(a.cnt, (int64_t)a.NQ * a.T, a.n_chunks, greater, equal, (hipStream_t)stream);
}

// The count pass and the reduce.
template <bool BF16, class Args>
int rk_launch_count(const Args& a, int32_t* greater, int32_t* equal, hipStream_t s) {
  rk_lds_limits<BF16, TkFp8<Args>::value>();
  const dim3 grid(a.n_qt * a.n_chunks);
  const size_t lds = tk_base_lds<BF16>() + (size_t)TK_Q * a.T * 12;
  if (Args::kNorm || a.subset)
    hipLaunchKernelGGL((rank_kernel<BF16, false, Args>), grid, dim3(256), lds, s, a);
  else if constexpr (!Args::kNorm)  // constexpr only so that the slice to RkArgs is not instantiated for NmRankArgs
    hipLaunchKernelGGL((rank_kernel<BF16, false, RkPlain<Args>>), grid, dim3(256), lds, s, (RkPlain<Args>)a);
  return rk_reduce_launch(a.cnt, (int64_t)a.NQ * a.T, a.n_chunks, greater, equal, s);
}

// workspace (int32 units): thresholds [NQ][T] fp32, then (greater, equal) [NQ][T][n_chunks][2]
// (Args = RkMaskedArgs or RkFp8MaskedArgs)
template <bool BF16, class Args>
int rk_rank(const MmtSearchScan& s, const int64_t* targets, int T, int32_t* ws, int32_t* greater, int32_t* equal,
            void* stream) {
  Args a = {};
  if (const int rc = rk_fill<BF16>(a, s, T, s.subset, targets && ws && greater && equal)) return rc;
  a.targets = targets; a.thr = (float*)ws; a.cnt = ws + (int64_t)s.NQ * T;
  rk_launch_thresholds<BF16>(a, (hipStream_t)stream);
  return rk_launch_count<BF16>(a, greater, equal, (hipStream_t)stream);
}

// The two halves on their own (a gallery cut into shards scores a target on the shard that holds it and counts it on every
// shard: search.py, ShardedVideoIndex), plain (Args = RkMaskedArgs, RkFp8MaskedArgs) or normalised (NmRankArgs): the same
// kernels, launched as above.
template <bool BF16, class Args>
int rk_thresholds(const MmtSearchScan& s, const int64_t* targets, int T, float* thr, void* stream) {
  Args a = {};
  if (const int rc = rk_fill<BF16>(a, s, T, nullptr, targets && thr)) return rc;
  a.targets = targets; a.thr = thr;
  rk_launch_thresholds<BF16>(a, (hipStream_t)stream);
  return (int)hipGetLastError();
}

// workspace (int32 units): (greater, equal) [NQ][T][n_chunks][2]
template <bool BF16, class Args>
int rk_count(const MmtSearchScan& s, const float* thr, int T, int32_t* ws, int32_t* greater, int32_t* equal, void* stream) {
  Args a = {};
  if (const int rc = rk_fill<BF16>(a, s, T, s.subset, thr && ws && greater && equal)) return rc;
  a.thr = const_cast<float*>(thr); a.cnt = ws;
  return rk_launch_count<BF16>(a, greater, equal, (hipStream_t)stream);
}
}  // namespace

extern "C" int64_t mmt_rank_workspace_ints(int NQ, int NV, int T) {
  if (!rk_args_ok(NQ, NV, T)) return MMT_ERR_ARG;
  return (int64_t)NQ * T * (1 + 2 * (int64_t)tk_n_chunks(NQ, NV));
}

extern "C" int64_t mmt_count_workspace_ints(int NQ, int NV, int T) {
  if (!rk_args_ok(NQ, NV, T)) return MMT_ERR_ARG;
  return (int64_t)NQ * T * 2 * (int64_t)tk_n_chunks(NQ, NV);
}

// (storage, norm, sets) -> the body and its argument block, for each of the three entries.
extern "C" int mmt_search_rank(const MmtSearchScan* scan, const int64_t* targets, int T, int32_t* ws, int32_t* greater,
                               int32_t* equal, void* stream) {
  if (const int rc = tk_scan_gate(scan, SC_SUBSET | SC_FP8)) return rc;
  switch (scan->storage) {
    case MMT_SEARCH_FP32: return rk_rank<false, RkMaskedArgs>(*scan, targets, T, ws, greater, equal, stream);
    case MMT_SEARCH_BF16: return rk_rank<true, RkMaskedArgs>(*scan, targets, T, ws, greater, equal, stream);
    default: return rk_rank<true, RkFp8MaskedArgs>(*scan, targets, T, ws, greater, equal, stream);
  }
}

extern "C" int mmt_search_thresholds(const MmtSearchScan* scan, const int64_t* targets, int T, float* thr, void* stream) {
  if (const int rc = tk_scan_gate(scan, SC_NORM | SC_QSETS | SC_ISETS | SC_FP8)) return rc;
  const MmtSearchScan& s = *scan;
  const unsigned p = tk_scan_parts(s);
  if (p & SC_QSETS) return pl_thresholds(s, targets, T, thr, stream);
  if (p & SC_ISETS) return is_thresholds(s, targets, T, thr, stream);
  if (p & SC_FP8) return rk_thresholds<true, RkFp8MaskedArgs>(s, targets, T, thr, stream);
  if (s.storage == MMT_SEARCH_FP32)
    return p & SC_NORM ? rk_thresholds<false, NmRankArgs>(s, targets, T, thr, stream)
                       : rk_thresholds<false, RkMaskedArgs>(s, targets, T, thr, stream);
  return p & SC_NORM ? rk_thresholds<true, NmRankArgs>(s, targets, T, thr, stream)
                     : rk_thresholds<true, RkMaskedArgs>(s, targets, T, thr, stream);
}

extern "C" int mmt_search_count(const MmtSearchScan* scan, const float* thr, int T, int32_t* ws, int32_t* greater,
                                int32_t* equal, void* stream) {
  if (const int rc = tk_scan_gate(scan, SC_SUBSET | SC_NORM | SC_QSETS | SC_ISETS | SC_FP8)) return rc;
  const MmtSearchScan& s = *scan;
  const unsigned p = tk_scan_parts(s);
  if (p & SC_QSETS) return pl_count(s, thr, T, ws, greater, equal, stream);
  if (p & SC_ISETS) return is_count(s, thr, T, ws, greater, equal, stream);
  if (p & SC_FP8) return rk_count<true, RkFp8MaskedArgs>(s, thr, T, ws, greater, equal, stream);
  if (s.storage == MMT_SEARCH_FP32)
    return p & SC_NORM ? rk_count<false, NmRankArgs>(s, thr, T, ws, greater, equal, stream)
                       : rk_count<false, RkMaskedArgs>(s, thr, T, ws, greater, equal, stream);
  return p & SC_NORM ? rk_count<true, NmRankArgs>(s, thr, T, ws, greater, equal, stream)
                     : rk_count<true, RkMaskedArgs>(s, thr, T, ws, greater, equal, stream);
}

// The filtered count pass (subset; fp32, bf16, fp8): mmt_search_count against given thresholds with the per-query
// attribute filter; workspace and outputs are mmt_search_count's.
extern "C" int mmt_search_count_where(const MmtSearchScan* scan, const uint64_t* tags, const uint64_t* where, const float* thr,
                                      int T, int32_t* ws, int32_t* greater, int32_t* equal, void* stream) {
  if (const int rc = tk_scan_gate(scan, SC_SUBSET | SC_FP8)) return rc;
  switch (scan->storage) {
    case MMT_SEARCH_FP32: return rk_count_where<false, RkWhereArgs>(*scan, tags, where, thr, T, ws, greater, equal, stream);
    case MMT_SEARCH_BF16: return rk_count_where<true, RkWhereArgs>(*scan, tags, where, thr, T, ws, greater, equal, stream);
    default: return rk_count_where<true, RkFp8WhereArgs>(*scan, tags, where, thr, T, ws, greater, equal, stream);
  }
}
