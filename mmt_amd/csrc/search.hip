// Top-k retrieval without the N_query x N_gallery matrix (reference: utils/util.py:38-68 compress_predictions,
// trainer/trainer.py:411-437, utils/visualizer.py:74-92; similarity of model/model.py:789-837 in 'indep' mode).
//
//   score(q, g) = sum_m qw[q][m] gw[g][m] <Q_m[q], G_m[g]> / sum_m qw[q][m] gw[g][m]     (0 -> 1e-5)
//
// Both operands arrive folded (Q' = qw * Q, G' = gw * G: mmt_search_fold), so the numerator is ONE fp32 GEMM with
// K = M*d on v_mfma_f32_32x32x2_f32, like mmt_sims_eval.  Two launches:
//   topk_scan_kernel         : block = 64 queries x one gallery chunk.  Per 128-column tile the K loop streams
//                              through LDS in 32-wide slabs (register-staged: the next slab's global loads are in flight
//                              during the current slab's MFMAs), the epilogue divides by the gated denominator and the
//                              tile's 64 x 128 scores land in LDS, where each wave keeps a running top-k for its 16 rows
//                              (threshold = k-th best so far; candidates above it are appended, the list is compacted
//                              back to k when full).  The chunk's sorted k best go to the workspace.
//   topk_select_kernel       : the same selection stage reading the scores from a given matrix (compress_predictions).
//   topk_merge_kernel        : per query, the chunk lists merged by rank (each list is sorted: binary search).
// Order: score descending, ties by ascending gallery index (= a stable argsort of -score).  A (score, index) pair is one
// uint64 key -- order-preserving score bits above, ~index below -- so "better" is one unsigned compare and every key is
// distinct; 0 is "no candidate".  No atomics: every output slot has exactly one writer, results are bit-reproducible.
// The key and the running top-k live in search_topk.h; the scoring tile (K loops, score epilogue, querybank rewrite) in
// search_scan.h, shared with the count, range and column-pass kernels (search_rank.hip, search_range.hip, search_norm.hip).
//
// topk_scan_kernel<BF16, Args> is ONE body, generic over its argument block; the block says how the subset bitmap and the
// querybank normalisation enter (kMask, kNorm: search_scan.h):
//   <false, TkArgs>, <false, TkMaskedArgs>       : fp32 gallery, above.
//   <true, TkBf16Args>, <true, TkBf16MaskedArgs> : a gallery stored in bf16 (search_bf16.hip has the fold and the score
//                                      definition): the K loop on v_mfma_f32_32x32x16_bf16 with the fp32 query as a bf16
//                                      hi / lo pair; same block, tile, accumulator layout, epilogue, selection, workspace
//                                      and merge.
//   <true, TkFp8Args>, <true, TkFp8MaskedArgs>   : a gallery stored in fp8 with a scale per item (search_fp8.hip): the
//                                      bf16 kernels with the gallery widened to bf16 on its way into LDS and the scale in
//                                      the epilogue (tk_tile reads kFp8 off the block).
//   <BF16, NmTopkArgs>               : the masked kernels with tk_tile_norm between the score epilogue and the selection:
//                                      ranks by and returns the querybank-normalised score' (search_norm.hip).
//   <., Tk*AfterArgs>, <., NmTopkAfterArgs> : the masked and normalised kernels with a cursor per query row (the paged search,
//                                      mmt_search_topk [after]): the selection also declines every key at or above the row's
//                                      bound (tk_tile_select<true, true>), one more compare on the same score tile.
//   <., Tk*WhereArgs>                : the paged kernels with the per-query attribute filter (mmt_search_topk_where): a tag
//                                      word per item, three masks per row, one more term of the selection's `live` per row
//                                      (tk_tile_select<true, true, TK_Q, true>), and a tile in which no row has a candidate
//                                      skipped before its K loop (tk_tile_where_any).
// The argument blocks stay separate types with their layouts as they are: a field appended to TkArgs moves the hidden
// kernel arguments behind it and changes the unmasked code (profiles/search_subset_kernel_identity.txt).
//
// The masked blocks (mmt_search_topk [subset, exclude] and the normalised calls): the candidates are the items whose bit is set in a
// packed bitmap (search_subset.hip; a null pointer allows every item), less up to TK_MAXE items per query.  A tile's four
// mask words are one block-uniform 16-byte load (tk_tile_mask; g0 is a multiple of 128); a tile with no bit set is skipped
// before its K loop -- no gallery loads, no MFMAs.  The mask acts at selection only (tk_tile_select<true>), on the score
// tile the unmasked kernel computes.  The unmasked instantiations compile to the code they had before the mask existed.
#include <type_traits>

#include "search_topk.h"

struct TkArgs {
  const float* q;       // fused: Q' [NQ][K]        select: sims (row stride ld)
  const float* qw;      // fused: query weights [NQ][M]
  const float* g;       // fused: G' [NV][K]
  const float* gw;      // fused: gallery weights [NV][M]
  const int32_t* rows;  // select: source row of output row r (nullable = identity)
  int64_t ld;
  uint64_t* ws;         // [NQ][n_chunks][k]
  int NQ, NV, M, K, k, chunk, n_qt, n_chunks;
  static constexpr TkMask kMask = TK_MASK_NONE;
  static constexpr bool kNorm = false;
};

// The masked instantiation's arguments: a kernel argument of its own type, so the unmasked kernels keep their argument
// block (and with it their code) byte for byte.
struct TkMaskedArgs : TkArgs {
  const uint32_t* subset;   // bit g & 31 of word g >> 5 allows item g (nullable = all; 16-byte aligned)
  const int64_t* exclude;   // [NQ][E] items barred per query, -1 = none
  int E;
  static constexpr TkMask kMask = TK_MASK_NULLABLE;
};

struct TkBf16Args {
  const bf16_t* q;      // hi(Q') [NQ][K]
  const bf16_t* q_lo;   // lo(Q') [NQ][K]
  const float* qw;      // [NQ][M]
  const bf16_t* g;      // [NV][K]
  const float* gw;      // [NV][M]
  uint64_t* ws;         // [NQ][n_chunks][k]
  int NQ, NV, M, K, k, chunk, n_qt, n_chunks;
  static constexpr TkMask kMask = TK_MASK_NONE;
  static constexpr bool kNorm = false;
};

struct TkBf16MaskedArgs : TkBf16Args {  // as TkMaskedArgs
  const uint32_t* subset;
  const int64_t* exclude;
  int E;
  static constexpr TkMask kMask = TK_MASK_NULLABLE;
};

// A gallery stored in fp8 (search_fp8.hip): e4m3fn codes behind g, one power-of-two scale per item.  The block says so in
// kFp8 (search_scan.h: TkFp8); the bf16 blocks keep their layout.
struct TkFp8Args : TkBf16Args {
  const float* gscale;  // [NV]
  static constexpr bool kFp8 = true;
};

struct TkFp8MaskedArgs : TkFp8Args {  // as TkMaskedArgs
  const uint32_t* subset;
  const int64_t* exclude;
  int E;
  static constexpr TkMask kMask = TK_MASK_NULLABLE;
};

struct NmTopkArgs : NmArgs {
  uint64_t* ws;             // [NQ][n_chunks][k]
  const uint32_t* subset;   // nullable = all
  const int64_t* exclude;   // [NQ][E]
  int k, E;
};

// The paged search (mmt_search_topk [after] and its kin): the masked blocks with one bound per query row behind them, in
// types of their own, so the blocks above keep their layout and their kernels their code.  after[q] is a position in the
// search's order as a key: only keys strictly below it are candidates (tk_tile_select<true, true>).
struct TkAfterArgs : TkMaskedArgs {
  const uint64_t* after;    // [NQ]: 2^64 - 1 = no cursor, 0 = exhausted, tk_key(a, first) + 1 = a position
  static constexpr bool kAfter = true;
};

struct TkBf16AfterArgs : TkBf16MaskedArgs {  // as TkAfterArgs
  const uint64_t* after;
  static constexpr bool kAfter = true;
};

struct TkFp8AfterArgs : TkFp8MaskedArgs {  // as TkAfterArgs
  const uint64_t* after;
  static constexpr bool kAfter = true;
};

struct NmTopkAfterArgs : NmTopkArgs {  // as TkAfterArgs
  const uint64_t* after;
  static constexpr bool kAfter = true;
};

// The filtered search (mmt_search_topk_where): the paged blocks with a tag word per item and three masks per query row
// behind them (search_scan.h: tk_tag_pass), again in types of their own.  One instantiation per storage serves every
// combination of subset, exclusions and cursor: `after` may be null here, and every live row then gets the bound
// 2^64 - 1, which no key reaches.
struct TkWhereArgs : TkAfterArgs {
  const uint64_t* tags;     // [NV]
  const uint64_t* where;    // [NQ][3]: all_of, none_of, any_of
  static constexpr bool kWhere = true;
};

struct TkBf16WhereArgs : TkBf16AfterArgs {  // as TkWhereArgs
  const uint64_t* tags;
  const uint64_t* where;
  static constexpr bool kWhere = true;
};

struct TkFp8WhereArgs : TkFp8AfterArgs {  // as TkWhereArgs
  const uint64_t* tags;
  const uint64_t* where;
  static constexpr bool kWhere = true;
};

// One block of the fused scan: 64 queries x one gallery chunk -> the chunk's sorted k best per query in the workspace.
// Args = TkArgs, TkBf16Args (kMask = TK_MASK_NONE), their masked forms or NmTopkArgs (TK_MASK_NULLABLE: subset bitmap,
// may be null, and per-query exclusions, E = 0 allowed), or one of those with a cursor per row (kAfter).
template <bool BF16, class Args>
__global__ __launch_bounds__(256) void topk_scan_kernel(Args a) {
  constexpr TkMask MASK = Args::kMask;
  constexpr bool NORM = Args::kNorm;
  constexpr bool AFTER = TkAfter<Args>::value;
  static_assert(!AFTER || MASK != TK_MASK_NONE, "the blocks with a cursor extend the masked ones");
  constexpr bool WHERE = TkWhere<Args>::value;
  static_assert(!WHERE || (AFTER && !NORM), "the filtered blocks extend the paged ones of the plain score");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int kUnion = BF16 ? TKB_UNION_BYTES : TK_UNION_BYTES;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int bid = xcd_remap(blockIdx.x, gridDim.x);  // gallery-chunk-major: an XCD's blocks share their chunk in L2
  const int chunk = bid / a.n_qt, q0 = (bid % a.n_qt) * TK_Q;
  const int g_begin = chunk * a.chunk, g_end = min(a.NV, g_begin + a.chunk);
  const int cap = a.k + 64;
  uint64_t* ws = a.ws + chunk * (int64_t)a.k;
  const int64_t ws_row = (int64_t)a.n_chunks * a.k;

  float* sS = (float*)smem;                                   // [TK_Q][TK_SLD]  scores (after the K loop)
  float* sQw = (float*)(smem + kUnion);                       // [TK_Q][MMT_MAX_EXPERTS]
  int* sN = (int*)(smem + kUnion + TK_QW_BYTES);              // [TK_Q] candidates held
  uint64_t* sT = (uint64_t*)(sN + TK_Q);                      // [TK_Q] thresholds
  uint64_t* sC = sT + TK_Q;                                   // [TK_Q][cap] candidates
  const int l31 = lane & 31, h = lane >> 5, wq = wave >> 1, wg = wave & 1;
  if (tid < TK_Q) { sN[tid] = 0; sT[tid] = 0; }
  tk_load_qw(sQw, a.qw, a.NQ, a.M, q0, tid);
  int* sEx = (int*)(sC + TK_Q * cap);                         // masked: [TK_Q][E] exclusions
  if constexpr (MASK != TK_MASK_NONE)
    for (int i = tid; i < TK_Q * a.E; i += 256) sEx[i] = q0 + i / a.E < a.NQ ? (int)a.exclude[(int64_t)q0 * a.E + i] : -1;
  int g_stop = g_end;
  uint64_t* sB = nullptr;                                     // paged: [TK_Q] bounds, behind the exclusions
  if constexpr (AFTER) {
    sB = (uint64_t*)(sEx + TK_Q * a.E);
    uint64_t mine;  // every wave reads the block's 64 bounds
    if constexpr (WHERE) mine = q0 + lane < a.NQ ? (a.after ? a.after[q0 + lane] : ~0ull) : 0ull;  // filtered: a null cursor
    else mine = q0 + lane < a.NQ ? a.after[q0 + lane] : 0ull;
    if (wave == 0) sB[lane] = mine;                                       // read behind the barriers of tk_tile
    // block-uniform (the four waves hold the same 64 values), before any barrier: every row of the block is exhausted --
    // no tile is scored, and the flush below writes the empty lists
    if (!__ballot(mine != 0ull)) g_stop = g_begin;
  }
  uint64_t* sW = nullptr;                                     // filtered: [TK_Q][3] masks, behind the bounds
  TkWhereGate gate;                                           // what the rows' masks share, the tags a tile ahead
  TkTagStream stream;
  if constexpr (WHERE) {
    sW = sB + TK_Q;
    tk_load_where<TK_Q>(sW, a.where, a.NQ, q0, tid);
    gate.template init<TK_Q>(a.where, a.NQ, q0, lane);
    stream.init(a.tags, g_begin, g_end, lane);
    __syncthreads();  // read by the gate of the first tile
  }
  for (int g0 = g_begin; g0 < g_stop; g0 += TK_G) {
    uint64_t t0 = 0, t1 = 0;
    if constexpr (WHERE) stream.next(a.tags, g0, g_end, lane, t0, t1);  // before any skip: the next tile's are asked for
    uint64_t m0 = ~0ull, m1 = ~0ull;
    if constexpr (MASK != TK_MASK_NONE)
      if (a.subset && !tk_tile_mask(a.subset, g0, m0, m1)) continue;  // block-uniform: nothing of this tile is allowed
    if constexpr (WHERE) {
      // block-uniform: no live row has a candidate in this tile (subset and filter; exclusions and cursor play no part)
      if (!tk_tile_where_any<TK_Q>(gate, sW, a.NQ - q0, t0, t1, g0 + lane < g_end && ((m0 >> lane) & 1ull),
                                   g0 + 64 + lane < g_end && ((m1 >> lane) & 1ull), wave))
        continue;
    }
    tk_tile<BF16, NORM>(a, smem, sS, sQw, q0, [=](int r) { return g0 + r < g_end ? g0 + r : -1; }, tid, wq, wg, l31, h);
    if constexpr (WHERE) {
      if (gate.uniform)  // block-uniform: one predicate for all rows is two more mask words, and the paged selection runs
        tk_tile_select<true, true>(sS, sC, sN, sT, a.k, a.NQ - q0, g0, g_end, wave, lane, m0 & __ballot(gate.common(t0)),
                                   m1 & __ballot(gate.common(t1)), sEx, a.E, sB);
      else
        tk_tile_select<true, true, TK_Q, true>(sS, sC, sN, sT, a.k, a.NQ - q0, g0, g_end, wave, lane, m0, m1, sEx, a.E, sB,
                                               sW, t0, t1);
    } else if constexpr (AFTER)
      tk_tile_select<true, true>(sS, sC, sN, sT, a.k, a.NQ - q0, g0, g_end, wave, lane, m0, m1, sEx, a.E, sB);
    else if constexpr (MASK != TK_MASK_NONE)
      tk_tile_select<true>(sS, sC, sN, sT, a.k, a.NQ - q0, g0, g_end, wave, lane, m0, m1, sEx, a.E);
    else
      tk_tile_select(sS, sC, sN, sT, a.k, a.NQ - q0, g0, g_end, wave, lane);
  }
  __syncthreads();
  for (int rr = 0; rr < TK_Q / 4; ++rr) {
    const int row = wave * (TK_Q / 4) + rr, q = q0 + row;
    if (q >= a.NQ) break;
    tk_flush(sC + row * cap, sN[row], a.k, lane, ws + q * ws_row);
  }
}

// The selection stage alone, reading the scores from a given matrix (mmt_rows_topk).
__global__ __launch_bounds__(256) void topk_select_kernel(TkArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int bid = xcd_remap(blockIdx.x, gridDim.x);
  const int chunk = bid / a.n_qt, q0 = (bid % a.n_qt) * TK_Q;
  const int g_begin = chunk * a.chunk, g_end = min(a.NV, g_begin + a.chunk);
  const int cap = a.k + 64;
  uint64_t* ws = a.ws + chunk * (int64_t)a.k;
  const int64_t ws_row = (int64_t)a.n_chunks * a.k;
  uint64_t* cand = (uint64_t*)smem + (int64_t)wave * cap;
  for (int rr = 0; rr < TK_Q / 4; ++rr) {
    const int q = q0 + wave * (TK_Q / 4) + rr;
    if (q >= a.NQ) break;
    const float* row = a.q + (a.rows ? (int64_t)a.rows[q] : (int64_t)q) * a.ld;
    int n = 0;
    uint64_t thr = 0;
    for (int g0 = g_begin; g0 < g_end; g0 += 64) {
      const int g = g0 + lane;
      tk_push(cand, n, thr, a.k, g < g_end ? tk_key(row[g], g) : 0ull, lane);
    }
    tk_flush(cand, n, a.k, lane, ws + q * ws_row);
  }
}

// One block per query: the n_chunks sorted lists of k keys -> the best kout, by rank.  A key at position j of its list
// has rank j + (number of keys above it in every other list); only the first kout of a list can matter.
__global__ __launch_bounds__(256) void topk_merge_kernel(const uint64_t* __restrict__ ws, int n_chunks, int k, int kout,
                                                         int stage, float* __restrict__ scores, int64_t* __restrict__ index) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int q = blockIdx.x, n = n_chunks * k;
  const uint64_t* L = ws + (int64_t)q * n;
  if (stage) {  // the lists fit in LDS
    uint64_t* s = (uint64_t*)smem;
    for (int i = threadIdx.x; i < n; i += 256) s[i] = L[i];
    __syncthreads();
    L = s;
  }
  const int lim = min(k, kout);
  for (int i = threadIdx.x; i < n; i += 256) {
    const int c = i / k, j = i - c * k;
    if (j >= kout) continue;
    const uint64_t key = L[i];
    if (!key) continue;
    int rank = j;
    for (int c2 = 0; c2 < n_chunks && rank < kout; ++c2) {
      if (c2 == c) continue;
      const uint64_t* l = L + (int64_t)c2 * k;
      int lo = 0, hi = lim;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (l[mid] > key) lo = mid + 1;
        else hi = mid;
      }
      rank += lo;
    }
    if (rank < kout) {
      if (scores) scores[(int64_t)q * kout + rank] = tk_score(key);
      index[(int64_t)q * kout + rank] = tk_index(key);
    }
  }
}

// Gallery columns per block: TK_CHUNK, halved (down to one tile) while the launch would not fill the chip.  A smaller
// chunk only happens when n_qt * n_chunks < TK_FILL, so the workspace stays below TK_FILL * TK_Q * k keys then.
int tk_chunk(int NQ, int NV) {
  const int64_t n_qt = (NQ + TK_Q - 1) / TK_Q;
  int chunk = TK_CHUNK;
  while (chunk > TK_G && n_qt * ((NV + chunk - 1) / chunk) < TK_FILL) chunk >>= 1;
  return chunk;
}

// The merge of the chunk lists behind every top-k entry point (declared in search_topk.h: search_pool.hip merges the
// lists of its sets with it).
int tk_merge_launch(const uint64_t* ws, int NQ, int n_chunks, int k, int kout, float* scores, int64_t* index,
                    hipStream_t s) {
  constexpr int kMergeLdsMax = 64 * 1024;
  const int64_t list_bytes = (int64_t)n_chunks * k * 8;
  const int stage = list_bytes <= kMergeLdsMax;
  hipLaunchKernelGGL(topk_merge_kernel, dim3(NQ), dim3(256), stage ? (size_t)list_bytes : 0, s, ws, n_chunks, k, kout,
                     stage, scores, index);
  return (int)hipGetLastError();
}

namespace {
bool tk_args_ok(int NQ, int NV, int k) { return NQ > 0 && NV > 0 && k >= 1 && k <= TK_MAXK; }

// LDS behind the slab / score-tile union: query weights, counts, thresholds, candidates ...
size_t tk_state_lds(int k) { return TK_QW_BYTES + TK_Q * (4 + 8) + (size_t)TK_Q * (k + 64) * 8; }
// ... and behind those, the masked kernels' exclusions [TK_Q][E]
size_t tk_exclude_lds(int E) { return (size_t)TK_Q * E * 4; }
// ... and behind those, the paged kernels' bounds [TK_Q]
constexpr size_t kAfterLds = (size_t)TK_Q * 8;
// ... and behind those, the filtered kernels' masks [TK_Q][3]
constexpr size_t kWhereLds = TK_WHERE_BYTES(TK_Q);
size_t tk_select_lds(int k) { return (size_t)4 * (k + 64) * 8; }

// The k = 128 footprint of the fused kernels is over the 64 KiB default.
void tk_topk_lds_limits() {
  static bool done[64] = {};
  const size_t f32 = TK_UNION_BYTES + tk_state_lds(TK_MAXK), bf16 = TKB_UNION_BYTES + tk_state_lds(TK_MAXK);
  const size_t ex = tk_exclude_lds(TK_MAXE);
  tk_lds_limits(done, {{(const void*)topk_scan_kernel<false, TkArgs>, f32},
                       {(const void*)topk_scan_kernel<false, TkMaskedArgs>, f32 + ex},
                       {(const void*)topk_scan_kernel<true, TkBf16Args>, bf16},
                       {(const void*)topk_scan_kernel<true, TkBf16MaskedArgs>, bf16 + ex},
                       {(const void*)topk_scan_kernel<true, TkFp8Args>, bf16},
                       {(const void*)topk_scan_kernel<true, TkFp8MaskedArgs>, bf16 + ex},
                       {(const void*)topk_scan_kernel<false, NmTopkArgs>, f32 + ex},
                       {(const void*)topk_scan_kernel<true, NmTopkArgs>, bf16 + ex},
                       {(const void*)topk_scan_kernel<false, TkAfterArgs>, f32 + ex + kAfterLds},
                       {(const void*)topk_scan_kernel<true, TkBf16AfterArgs>, bf16 + ex + kAfterLds},
                       {(const void*)topk_scan_kernel<true, TkFp8AfterArgs>, bf16 + ex + kAfterLds},
                       {(const void*)topk_scan_kernel<false, NmTopkAfterArgs>, f32 + ex + kAfterLds},
                       {(const void*)topk_scan_kernel<true, NmTopkAfterArgs>, bf16 + ex + kAfterLds}});
}

void tk_where_lds_limits() {
  static bool done[64] = {};
  const size_t f32 = TK_UNION_BYTES + tk_state_lds(TK_MAXK), bf16 = TKB_UNION_BYTES + tk_state_lds(TK_MAXK);
  const size_t more = tk_exclude_lds(TK_MAXE) + kAfterLds + kWhereLds;
  tk_lds_limits(done, {{(const void*)topk_scan_kernel<false, TkWhereArgs>, f32 + more},
                       {(const void*)topk_scan_kernel<true, TkBf16WhereArgs>, bf16 + more},
                       {(const void*)topk_scan_kernel<true, TkFp8WhereArgs>, bf16 + more}});
}

// The fused search behind mmt_search_topk (Args = TkMaskedArgs, TkBf16MaskedArgs, TkFp8MaskedArgs or NmTopkArgs, or one of
// those with a cursor; the descriptor has passed tk_scan_gate and carries the parts Args stands for): gate, fill, the
// chunk scan and the merge.  Without subset, exclusions, norm and cursor the unmasked instantiation runs.  tags, where: the
// filtered blocks' (mmt_search_topk_where: Args = Tk*WhereArgs, whose one instantiation takes every combination).
template <bool BF16, class Args>
int tk_search(const MmtSearchScan& s, int k, uint64_t* ws, float* scores, int64_t* index, void* stream,
              const uint64_t* tags = nullptr, const uint64_t* where = nullptr) {
  constexpr bool AFTER = TkAfter<Args>::value, FP8 = TkFp8<Args>::value, WHERE = TkWhere<Args>::value;
  if (!tk_scan_operands<BF16, FP8, Args::kNorm>(s) || !ws || !index || !tk_args_ok(s.NQ, s.NV, k) ||
      !tk_shape_ok(s.NQ, s.NV, s.M, s.d, BF16, FP8) || (WHERE && (!tags || !where)))
    return MMT_ERR_ARG;
  if (((uintptr_t)s.q | (uintptr_t)s.q_lo | (uintptr_t)s.g) & 15) return MMT_ERR_ALIGN;
  if (s.E < 0 || s.E > TK_MAXE || (s.E > 0 && !s.exclude)) return MMT_ERR_ARG;
  if ((uintptr_t)s.subset & 15) return MMT_ERR_ALIGN;  // null = every item allowed
  Args a = {};
  a.q = static_cast<decltype(a.q)>(s.q); a.qw = s.qw; a.g = static_cast<decltype(a.g)>(s.g); a.gw = s.gw; a.ws = ws;
  if constexpr (BF16) a.q_lo = static_cast<decltype(a.q_lo)>(s.q_lo);
  if constexpr (FP8) a.gscale = s.gscale;
  if constexpr (Args::kNorm) { a.beta = s.beta; a.lse = s.lse; }
  a.NQ = s.NQ; a.NV = s.NV; a.M = s.M; a.K = s.M * s.d; a.k = k;
  a.subset = s.subset; a.exclude = s.exclude; a.E = s.E;
  if constexpr (AFTER) a.after = s.after;
  if constexpr (WHERE) { a.tags = tags; a.where = where; }
  tk_geometry(a);
  if constexpr (WHERE) tk_where_lds_limits();
  else tk_topk_lds_limits();
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(a.n_qt * a.n_chunks);
  const size_t lds = (BF16 ? TKB_UNION_BYTES : TK_UNION_BYTES) + tk_state_lds(k);
  using Plain = std::conditional_t<FP8, TkFp8Args, std::conditional_t<BF16, TkBf16Args, TkArgs>>;
  if (AFTER || Args::kNorm || s.subset || s.E)
    hipLaunchKernelGGL((topk_scan_kernel<BF16, Args>), grid, dim3(256),
                       lds + tk_exclude_lds(s.E) + (AFTER ? kAfterLds : 0) + (WHERE ? kWhereLds : 0), st, a);
  else if constexpr (!Args::kNorm && !AFTER)  // constexpr only so that the slice to Plain is not instantiated for NmTopkArgs
    hipLaunchKernelGGL((topk_scan_kernel<BF16, Plain>), grid, dim3(256), lds, st, (Plain)a);
  return tk_merge_launch(ws, s.NQ, a.n_chunks, k, k < s.NV ? k : s.NV, scores, index, st);
}
}  // namespace

// The bounds of the paged search from positions: keys[q] = tk_key(scores[q], first[q]) + 1, where first[q] >= 0 is the
// lowest item number still admitted at that score (the low word of a key is ~item, so the + 1 carries into the score word
// exactly when first is 0: "every item at this score"); first[q] < 0 selects a sentinel by the sign of the score, which is
// then infinite: + = no cursor (2^64 - 1, above every key), - = exhausted (0).
__global__ __launch_bounds__(256) void after_keys_kernel(const float* __restrict__ scores, const int64_t* __restrict__ first,
                                                         int NQ, uint64_t* __restrict__ keys) {
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= NQ) return;
  const float s = scores[q];
  const int64_t f = first[q];
  keys[q] = f < 0 ? (s > 0.f ? ~0ull : 0ull) : tk_key(s, (int)f) + 1ull;
}

extern "C" int mmt_search_after_keys(const float* scores, const int64_t* first, int NQ, uint64_t* keys, void* stream) {
  if (!scores || !first || !keys || NQ < 1) return MMT_ERR_ARG;
  hipLaunchKernelGGL(after_keys_kernel, dim3((NQ + 255) / 256), dim3(256), 0, (hipStream_t)stream, scores, first, NQ, keys);
  return (int)hipGetLastError();
}

extern "C" int64_t mmt_topk_workspace_keys(int NQ, int NV, int k) {
  if (!tk_args_ok(NQ, NV, k)) return MMT_ERR_ARG;
  return (int64_t)NQ * tk_n_chunks(NQ, NV) * k;
}

// (storage, norm, cursor, sets) -> the body and its argument block.
extern "C" int mmt_search_topk(const MmtSearchScan* scan, int k, uint64_t* ws, float* scores, int64_t* index,
                               void* stream) {
  if (const int rc = tk_scan_gate(scan, SC_SUBSET | SC_EXCLUDE | SC_AFTER | SC_NORM | SC_QSETS | SC_ISETS | SC_FP8)) return rc;
  const MmtSearchScan& s = *scan;
  const unsigned p = tk_scan_parts(s);
  if (p & SC_QSETS) return pl_topk(s, k, ws, scores, index, stream);
  if (p & SC_ISETS) return is_topk(s, k, ws, scores, index, stream);
  const bool after = p & SC_AFTER;
  if (p & SC_FP8)
    return after ? tk_search<true, TkFp8AfterArgs>(s, k, ws, scores, index, stream)
                 : tk_search<true, TkFp8MaskedArgs>(s, k, ws, scores, index, stream);
  if (s.storage == MMT_SEARCH_BF16) {
    if (p & SC_NORM)
      return after ? tk_search<true, NmTopkAfterArgs>(s, k, ws, scores, index, stream)
                   : tk_search<true, NmTopkArgs>(s, k, ws, scores, index, stream);
    return after ? tk_search<true, TkBf16AfterArgs>(s, k, ws, scores, index, stream)
                 : tk_search<true, TkBf16MaskedArgs>(s, k, ws, scores, index, stream);
  }
  if (p & SC_NORM)
    return after ? tk_search<false, NmTopkAfterArgs>(s, k, ws, scores, index, stream)
                 : tk_search<false, NmTopkArgs>(s, k, ws, scores, index, stream);
  return after ? tk_search<false, TkAfterArgs>(s, k, ws, scores, index, stream)
               : tk_search<false, TkMaskedArgs>(s, k, ws, scores, index, stream);
}

// The filtered search: storage -> the one filtered block of that storage.
extern "C" int mmt_search_topk_where(const MmtSearchScan* scan, const uint64_t* tags, const uint64_t* where, int k,
                                     uint64_t* ws, float* scores, int64_t* index, void* stream) {
  if (const int rc = tk_scan_gate(scan, SC_SUBSET | SC_EXCLUDE | SC_AFTER | SC_FP8)) return rc;
  const MmtSearchScan& s = *scan;
  if (s.storage == MMT_SEARCH_FP8) return tk_search<true, TkFp8WhereArgs>(s, k, ws, scores, index, stream, tags, where);
  if (s.storage == MMT_SEARCH_BF16) return tk_search<true, TkBf16WhereArgs>(s, k, ws, scores, index, stream, tags, where);
  return tk_search<false, TkWhereArgs>(s, k, ws, scores, index, stream, tags, where);
}

extern "C" int mmt_rows_topk(const float* sims, int64_t ld, const int32_t* rows, int NR, int NV, int k, uint64_t* ws,
                             float* scores, int64_t* index, void* stream) {
  if (!sims || !ws || !index || !tk_args_ok(NR, NV, k) || ld < NV) return MMT_ERR_ARG;
  TkArgs a = {};
  a.q = sims; a.ld = ld; a.rows = rows; a.ws = ws;
  a.NQ = NR; a.NV = NV; a.k = k;
  tk_geometry(a);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(topk_select_kernel, dim3(a.n_qt * a.n_chunks), dim3(256), tk_select_lds(k), s, a);
  return tk_merge_launch(ws, NR, a.n_chunks, k, k < NV ? k : NV, scores, index, s);
}
