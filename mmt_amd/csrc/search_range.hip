// Range search without the N_query x N_gallery matrix: every item g with score(q, g) >= thr[q], however many there are,
// as a CSR over the queries (offsets, item numbers, scores).  Near-duplicate joins, all captions that match a video, all
// negatives inside a margin, any list deeper than the top-k kernels' k <= 128.
//
// The scan is the one of the count kernels (search_rank.hip): block = 64 queries x one gallery chunk (tk_geometry), blocks
// ordered by xcd_remap, tk_tile of search_scan.h leaves a 64 x 128 score tile in LDS (tk_tile_mask gates it) and a wave
// takes its 16 rows.  It runs twice over the same operands, with a host-side sum between the passes:
//   range_kernel<BF16, false, MASKED> : counts.  Per row and tile two ballots of `live && score >= thr[row]` (the two
//                               64-column halves; a plain float compare: a NaN threshold hits nothing, -inf every live
//                               item); the popcounts add up in a register of the lane that holds the row (lane l < 16 of
//                               wave w holds row 16 w + l for the whole block: no LDS, no barrier).  One int32 per (query,
//                               chunk) goes to the workspace [NQ][n_chunks].
//   range_offsets_kernel      : one thread per query turns the row's chunk counts into their exclusive prefix in place, in
//                               chunk order, and writes the row total as int64.  The host sums the rows (torch cumsum)
//                               into offsets [NQ + 1] and learns the grand total before anything of that size exists.
//   range_kernel<BF16, true, MASKED>  : fill.  The same scan and predicate, so the same hits.  A hit at lane l of half h
//                               of row q goes to  offsets[q] + prefix[q][chunk] + (hits of the row in the block's earlier
//                               tiles) + (hits in lower columns of this tile): popcount of the ballot below the lane, plus
//                               the first half's popcount for the second half.  It writes the item number (int64) and
//                               the tile's own score bits.  A block whose 64 rows have no hit in its chunk (the prefix
//                               says so) returns before its first K loop.
// No atomics and one writer per slot: bit-reproducible, every row ascending by item number by construction.  Both passes
// compute the same bits from the same code, so the counts agree; all the same a fill position is clamped against the
// start of the row's next chunk (the next prefix, or the next row's offset), so a disagreement would show as a wrong
// answer inside the row's own slots and never as a stray write.
// MASKED: only items whose bit is set in the packed bitmap (search_subset.hip) are hits; a tile without a set bit is
// skipped before its K loop, as in rank_kernel<., false, true>.
#include <type_traits>

#include "search_scan.h"

struct RgArgs {
  const void* q;           // fp32: Q' [NQ][K]; bf16: hi(Q')
  const void* q_lo;        // bf16: lo(Q')
  const float* qw;         // [NQ][M]
  const void* g;           // [NV][K] fp32 or bf16 bits
  const float* gw;         // [NV][M]
  const float* thr;        // [NQ]
  int32_t* ws;             // [NQ][n_chunks]: the count pass writes hit counts, the offsets kernel their prefix
  const int64_t* offsets;  // fill: [NQ + 1]
  int64_t* indices;        // fill: [offsets[NQ]]
  float* scores;           // fill: [offsets[NQ]]
  int NQ, NV, M, K, chunk, n_qt, n_chunks;
};

// The masked passes take an argument type of their own, as RkMaskedArgs: the unmasked kernels keep their argument block.
struct RgMaskedArgs : RgArgs {
  const uint32_t* subset;  // bit g & 31 of word g >> 5 allows item g (16-byte aligned)
};

// A gallery stored in fp8 (search_fp8.hip): e4m3fn codes behind g, one power-of-two scale per item; the block says so in
// kFp8 (search_scan.h: TkFp8).
struct RgFp8Args : RgArgs {
  const float* gscale;     // [NV]
  static constexpr bool kFp8 = true;
};

struct RgFp8MaskedArgs : RgFp8Args {  // as RgMaskedArgs
  const uint32_t* subset;
};

// The filtered passes (mmt_search_range_count_where, mmt_search_range_fill_where): the masked blocks with a tag word per
// item and three masks per query row behind them (search_scan.h: tk_tag_pass); the subset may be null here.  Both passes
// apply the same term, so they see the same hits.
struct RgWhereArgs : RgMaskedArgs {
  const uint64_t* tags;    // [NV]
  const uint64_t* where;   // [NQ][3]: all_of, none_of, any_of
  static constexpr bool kWhere = true;
};

struct RgFp8WhereArgs : RgFp8MaskedArgs {  // as RgWhereArgs
  const uint64_t* tags;
  const uint64_t* where;
  static constexpr bool kWhere = true;
};

// The unmasked block of a masked one.
template <class Args>
using RgPlain = std::conditional_t<TkFp8<Args>::value, RgFp8Args, RgArgs>;

// Args: RgArgs / RgMaskedArgs unless given (the fp8 blocks).
template <bool BF16, bool FILL, bool MASKED, class Args = std::conditional_t<MASKED, RgMaskedArgs, RgArgs>>
__global__ __launch_bounds__(256) void range_kernel(Args a) {
  constexpr bool WHERE = TkWhere<Args>::value;
  static_assert(!WHERE || MASKED, "the filtered blocks extend the masked ones");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int kUnion = BF16 ? TKB_UNION_BYTES : TK_UNION_BYTES;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, h = lane >> 5, wq = wave >> 1, wg = wave & 1;
  float* sS = (float*)smem;              // [TK_Q][TK_SLD]  scores (after the K loop)
  float* sQw = (float*)(smem + kUnion);  // [TK_Q][MMT_MAX_EXPERTS]
  const int bid = xcd_remap(blockIdx.x, gridDim.x);  // gallery-chunk-major: an XCD's blocks share their chunk in L2
  const int chunk = bid / a.n_qt, q0 = (bid % a.n_qt) * TK_Q;
  const int g_begin = chunk * a.chunk, g_end = min(a.NV, g_begin + a.chunk);
  const int rows_live = min(a.NQ - q0, TK_Q);
  TkRange<FILL, false> rg;  // the rows' thresholds, hits so far and, for the fill, slots of this chunk
  if (!rg.init(a.thr, nullptr, a.ws, a.offsets, q0, rows_live, chunk, a.n_chunks, g_end - g_begin, wave, lane))
    return;  // block-uniform: no row of this block has a hit in this chunk
  tk_load_qw(sQw, a.qw, a.NQ, a.M, q0, tid);  // read after the barriers of the first K loop
  uint64_t* sW = nullptr;                     // filtered: [TK_Q][3] masks behind the query weights
  TkWhereGate gate;                           // what the rows' masks share, the tags a tile ahead
  TkTagStream stream;
  if constexpr (WHERE) {
    sW = (uint64_t*)(sQw + TK_Q * MMT_MAX_EXPERTS);
    tk_load_where<TK_Q>(sW, a.where, a.NQ, q0, tid);
    gate.template init<TK_Q>(a.where, a.NQ, q0, lane);
    stream.init(a.tags, g_begin, g_end, lane);
    __syncthreads();  // read by the gate of the first tile
  }
  for (int g0 = g_begin; g0 < g_end; g0 += TK_G) {
    uint64_t m0 = ~0ull, m1 = ~0ull, t0 = 0, t1 = 0;
    if constexpr (WHERE) stream.next(a.tags, g0, g_end, lane, t0, t1);  // before any skip: the next tile's are asked for
    if constexpr (WHERE) {
      if (a.subset && !tk_tile_mask(a.subset, g0, m0, m1)) continue;  // block-uniform; a null subset allows every item
    } else if constexpr (MASKED) {
      if (!tk_tile_mask(a.subset, g0, m0, m1)) continue;  // block-uniform: nothing of this tile can hit
    }
    if constexpr (WHERE) {
      if (!tk_tile_where_any<TK_Q>(gate, sW, rows_live, t0, t1, g0 + lane < g_end && ((m0 >> lane) & 1ull),
                                   g0 + 64 + lane < g_end && ((m1 >> lane) & 1ull), wave))
        continue;  // block-uniform: no live row has a candidate in this tile
    }
    tk_tile<BF16, false>(a, smem, sS, sQw, q0, [=](int r) { return g0 + r < g_end ? g0 + r : -1; }, tid, wq, wg, l31, h);
    const bool live0 = g0 + lane < g_end && (!MASKED || ((m0 >> lane) & 1ull));
    const bool live1 = g0 + 64 + lane < g_end && (!MASKED || ((m1 >> lane) & 1ull));
    if constexpr (WHERE) {
      if (gate.uniform)  // block-uniform: one predicate for all rows is one more term of the shared liveness
        rg.tile(sS, g0, live0 && gate.common(t0), live1 && gate.common(t1), rows_live, a.indices, a.scores, wave, lane);
      else
        rg.template tile<true>(sS, g0, live0, live1, rows_live, a.indices, a.scores, wave, lane, sW, t0, t1);
    } else {
      rg.tile(sS, g0, live0, live1, rows_live, a.indices, a.scores, wave, lane);
    }
  }
  if constexpr (!FILL) rg.flush(a.ws, a.n_chunks, chunk);
}

// One thread per query: the chunk counts become their exclusive prefix, in chunk order; the row total as int64.
__global__ __launch_bounds__(256) void range_offsets_kernel(int32_t* __restrict__ ws, int NQ, int n_chunks,
                                                            int64_t* __restrict__ row_counts) {
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= NQ) return;
  int32_t* row = ws + (int64_t)q * n_chunks;
  int run = 0;
  for (int c = 0; c < n_chunks; ++c) {
    const int n = row[c];
    row[c] = run;
    run += n;
  }
  row_counts[q] = run;
}

int rg_offsets_launch(int32_t* ws, int R, int n_chunks, int64_t* row_counts, hipStream_t s) {
  hipLaunchKernelGGL(range_offsets_kernel, dim3((R + 255) / 256), dim3(256), 0, s, ws, R, n_chunks, row_counts);
  return (int)hipGetLastError();
}

namespace {
// The gate and the fill of the two entry points (Args = RgMaskedArgs or RgFp8MaskedArgs): 0, or the error code.  `own`:
// the entry's other pointers are all there.
template <bool BF16, class Args>
int rg_fill(Args& a, const MmtSearchScan& s, const float* thr, const int32_t* ws, bool own) {
  constexpr bool FP8 = TkFp8<Args>::value;
  if constexpr (TkWhere<Args>::value) own = own && a.tags && a.where;  // set by the caller before the fill
  if (!tk_scan_operands<BF16, FP8>(s) || !thr || !ws || !own || !tk_shape_ok(s.NQ, s.NV, s.M, s.d, BF16, FP8))
    return MMT_ERR_ARG;
  if (!tk_scan_aligned(s)) return MMT_ERR_ALIGN;
  a.q = s.q; a.q_lo = s.q_lo; a.qw = s.qw; a.g = s.g; a.gw = s.gw; a.thr = thr; a.ws = const_cast<int32_t*>(ws);
  a.subset = s.subset;
  if constexpr (FP8) a.gscale = s.gscale;
  a.NQ = s.NQ; a.NV = s.NV; a.M = s.M; a.K = s.M * s.d;
  tk_geometry(a);
  return 0;
}

template <bool BF16, bool FILL, class Args>
void rg_launch(const Args& a, hipStream_t s) {
  if constexpr (TkWhere<Args>::value)  // always the filtered instantiation, its masks behind the query weights
    hipLaunchKernelGGL((range_kernel<BF16, FILL, true, Args>), dim3(a.n_qt * a.n_chunks), dim3(256),
                       tk_base_lds<BF16>() + TK_WHERE_BYTES(TK_Q), s, a);
  else if (a.subset)
    hipLaunchKernelGGL((range_kernel<BF16, FILL, true, Args>), dim3(a.n_qt * a.n_chunks), dim3(256), tk_base_lds<BF16>(), s,
                       a);
  else
    hipLaunchKernelGGL((range_kernel<BF16, FILL, false, RgPlain<Args>>), dim3(a.n_qt * a.n_chunks), dim3(256),
                       tk_base_lds<BF16>(), s, (RgPlain<Args>)a);
}

// tags, where: the filtered blocks' (Args = Rg*WhereArgs), null for the others.
template <bool BF16, class Args>
int rg_count_tagged(const MmtSearchScan& s, const float* thr, int32_t* ws, int64_t* row_counts, void* stream,
                    const uint64_t* tags, const uint64_t* where) {
  Args a = {};
  if constexpr (TkWhere<Args>::value) { a.tags = tags; a.where = where; }
  if (const int rc = rg_fill<BF16>(a, s, thr, ws, row_counts != nullptr)) return rc;
  rg_launch<BF16, false>(a, (hipStream_t)stream);
  return rg_offsets_launch(ws, s.NQ, a.n_chunks, row_counts, (hipStream_t)stream);
}

template <bool BF16, class Args>
int rg_count(const MmtSearchScan& s, const float* thr, int32_t* ws, int64_t* row_counts, void* stream) {
  return rg_count_tagged<BF16, Args>(s, thr, ws, row_counts, stream, nullptr, nullptr);
}

template <bool BF16, class Args>
int rg_fill_hits_tagged(const MmtSearchScan& s, const float* thr, const int32_t* ws, const int64_t* offsets, int64_t* indices,
                        float* scores, void* stream, const uint64_t* tags, const uint64_t* where) {
  Args a = {};
  if constexpr (TkWhere<Args>::value) { a.tags = tags; a.where = where; }
  if (const int rc = rg_fill<BF16>(a, s, thr, ws, offsets && indices && scores)) return rc;
  a.offsets = offsets; a.indices = indices; a.scores = scores;
  rg_launch<BF16, true>(a, (hipStream_t)stream);
  return (int)hipGetLastError();
}

template <bool BF16, class Args>
int rg_fill_hits(const MmtSearchScan& s, const float* thr, const int32_t* ws, const int64_t* offsets, int64_t* indices,
                 float* scores, void* stream) {
  return rg_fill_hits_tagged<BF16, Args>(s, thr, ws, offsets, indices, scores, stream, nullptr, nullptr);
}
}  // namespace

extern "C" int64_t mmt_range_workspace_ints(int NQ, int NV) {
  return tk_range_workspace_ints(NQ, NV);
}

// storage -> the body and its argument block.  The fp8 pair is named last: the kernels lie in the code object in the order
// of their first use here, and that order stays what it has been (profiles/search_abi_kernel_identity.txt).
namespace {
struct RgBodies {
  int (*count[3])(const MmtSearchScan&, const float*, int32_t*, int64_t*, void*);
  int (*fill[3])(const MmtSearchScan&, const float*, const int32_t*, const int64_t*, int64_t*, float*, void*);
};
const RgBodies kRgBodies = [] {
  RgBodies b = {};
  b.count[MMT_SEARCH_FP32] = rg_count<false, RgMaskedArgs>;
  b.count[MMT_SEARCH_BF16] = rg_count<true, RgMaskedArgs>;
  b.fill[MMT_SEARCH_FP32] = rg_fill_hits<false, RgMaskedArgs>;
  b.fill[MMT_SEARCH_BF16] = rg_fill_hits<true, RgMaskedArgs>;
  b.count[MMT_SEARCH_FP8] = rg_count<true, RgFp8MaskedArgs>;
  b.fill[MMT_SEARCH_FP8] = rg_fill_hits<true, RgFp8MaskedArgs>;
  return b;
}();
}  // namespace

extern "C" int mmt_search_range_count(const MmtSearchScan* scan, const float* thr, int32_t* ws, int64_t* row_counts,
                                      void* stream) {
  if (const int rc = tk_scan_gate(scan, SC_SUBSET | SC_FP8)) return rc;
  return kRgBodies.count[scan->storage](*scan, thr, ws, row_counts, stream);
}

extern "C" int mmt_search_range_fill(const MmtSearchScan* scan, const float* thr, const int32_t* ws, const int64_t* offsets,
                                     int64_t* indices, float* scores, void* stream) {
  if (const int rc = tk_scan_gate(scan, SC_SUBSET | SC_FP8)) return rc;
  return kRgBodies.fill[scan->storage](*scan, thr, ws, offsets, indices, scores, stream);
}

// The filtered passes (subset; fp32, bf16, fp8): workspace, outputs and the offsets kernel are the unfiltered entries'.
extern "C" int mmt_search_range_count_where(const MmtSearchScan* scan, const uint64_t* tags, const uint64_t* where,
                                            const float* thr, int32_t* ws, int64_t* row_counts, void* stream) {
  if (const int rc = tk_scan_gate(scan, SC_SUBSET | SC_FP8)) return rc;
  switch (scan->storage) {
    case MMT_SEARCH_FP32: return rg_count_tagged<false, RgWhereArgs>(*scan, thr, ws, row_counts, stream, tags, where);
    case MMT_SEARCH_BF16: return rg_count_tagged<true, RgWhereArgs>(*scan, thr, ws, row_counts, stream, tags, where);
    default: return rg_count_tagged<true, RgFp8WhereArgs>(*scan, thr, ws, row_counts, stream, tags, where);
  }
}

extern "C" int mmt_search_range_fill_where(const MmtSearchScan* scan, const uint64_t* tags, const uint64_t* where,
                                           const float* thr, const int32_t* ws, const int64_t* offsets, int64_t* indices,
                                           float* scores, void* stream) {
  if (const int rc = tk_scan_gate(scan, SC_SUBSET | SC_FP8)) return rc;
  switch (scan->storage) {
    case MMT_SEARCH_FP32:
      return rg_fill_hits_tagged<false, RgWhereArgs>(*scan, thr, ws, offsets, indices, scores, stream, tags, where);
    case MMT_SEARCH_BF16:
      return rg_fill_hits_tagged<true, RgWhereArgs>(*scan, thr, ws, offsets, indices, scores, stream, tags, where);
    default: return rg_fill_hits_tagged<true, RgFp8WhereArgs>(*scan, thr, ws, offsets, indices, scores, stream, tags, where);
  }
}
