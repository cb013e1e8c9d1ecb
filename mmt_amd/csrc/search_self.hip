// The gallery self-join (search.py: VideoIndex.neighbours, neighbour_range, duplicate_groups): the stored items searched
// against the stored items, as a streaming scan -- per row item its k best stored items, or every stored item at or above
// a threshold as a CSR -- without the NV x NV matrix.  The quantity is the one of search_diverse.hip,
//   sim(g, h) = <f_g, f_h> / sum_m gw_g[m] gw_h[m]      (0 -> 1e-5)
// f_g the dequantised stored row, and every score here has the bits pair_scores_kernel gives the pair BY CONSTRUCTION: the K
// loop is search_scan.h's tk_scan -- the scans' composition of TkStager, tk_k_loop and tk_step, with the A rows read
// through a row table and ONE plane of the stored element (fp32 rows on v_mfma_f32_32x32x2_f32; bf16 rows, and fp8 codes
// widened exactly in the stager, on one v_mfma_f32_32x32x16_bf16 per fragment, no hi / lo pair), the pieces the Gram of
// search_diverse.hip is made of -- and the epilogue is the one definition of sim, tk_pair_sims.
//
// BOTH operands are stored rows, and they are two operands: the A side (a_rows, a_weights, a_scales: NA rows) read
// through the row indirection items[r] (null = row r), 64 rows of the slab per block; the B side (g, gw, gscale: NV items)
// the chunk's 128 columns per tile.  On one index A = B; a sharded index stages the rows' stored bytes and hands every
// shard that block as A, and `source=` joins another index's items against this one.  self[r] is the B-side item number
// row r must not meet (its own: left out by NUMBER, so an exact copy of it stays in its list), -1 = none.
//   self_kernel<ST, SJ_TOPK> : block = 64 rows x one gallery chunk (tk_geometry, xcd_remap).  Per 128-column tile the
//                              scores land in LDS in the layout tk_tile leaves (sS [TK_Q][TK_SLD]) and tk_tile_select<true>
//                              consumes it unchanged: the row's own item is its single exclusion (E = 1), a subset bitmap
//                              gates tiles and columns (tk_tile_mask).  tk_flush leaves the chunk's sorted k best per row
//                              in the workspace [R][n_chunks][k]; tk_merge_launch merges it.
//   self_kernel<ST, SJ_COUNT>, <ST, SJ_FILL> : the count and the fill pass of a range scan: search_scan.h's range step
//                              TkRange<FILL, true>, range_kernel's with the row's own item to skip (`live && item != self
//                              && score >= thr[row]`); between the passes search_range.hip's offsets kernel
//                              (rg_offsets_launch) turns a row's chunk counts into their exclusive prefix.
// No atomics; every output slot has one writer; results are bit-reproducible.
#include "search_topk.h"

enum { SJ_TOPK = 0, SJ_COUNT = 1, SJ_FILL = 2 };

#define SJ_SLAB_BYTES ((TK_Q + TK_G) * TK_LD * 4)
static_assert(SJ_SLAB_BYTES == (TK_Q + TK_G) * TKB_LD * 2, "the fp32 and the bf16 slabs are the same bytes");
#define SJ_UNION_BYTES (TK_TILE_BYTES > SJ_SLAB_BYTES ? TK_TILE_BYTES : SJ_SLAB_BYTES)
// behind the slab / score-tile union: the rows' weights, their scales, their stored rows
#define SJ_ROWS_BYTES (TK_QW_BYTES + TK_Q * 4 + TK_Q * 4)

struct SjArgs {
  const void* a;           // A side: [NA][K] fp32, bf16 bits or e4m3fn codes
  const float* aw;         // [NA][M]
  const float* ascale;     // fp8: [NA]
  const int64_t* items;    // [R] rows of A (null = row r)
  const int64_t* self;     // [R] B-side item row r skips, -1 = none (null = none)
  const void* g;           // B side: [NV][K]
  const float* gw;         // [NV][M]
  const float* gscale;     // fp8: [NV]
  const uint32_t* subset;  // bit g & 31 of word g >> 5 allows item g (null = all; 16-byte aligned)
  uint64_t* ws;            // top-k: [R][n_chunks][k]
  const float* thr;        // range: [R]
  int32_t* cnt;            // range: [R][n_chunks], counts, then their prefix
  const int64_t* offsets;  // fill: [R + 1]
  int64_t* indices;        // fill
  float* scores;           // fill
  int NA, NQ, NV, M, K, k, chunk, n_qt, n_chunks;  // NQ = R, named as tk_geometry reads it
};

// One 64 x 128 tile of sims in sS [TK_Q][TK_SLD]: tk_scan with the A rows read through the row table -- one plane of
// the stored element, widened if it is fp8 -- and the stored-pair epilogue tk_pair_sims: the rows' weights
// (sAw [TK_Q][MMT_MAX_EXPERTS], zero past M and for no row) and, fp8, scales (sAsc [TK_Q]) from LDS, the column's read per
// lane, once per m for its 16 rows.  Ends fenced.
template <int ST, class GRow>
__device__ __forceinline__ void sj_tile(const SjArgs& a, unsigned char* smem, float* sS, const float* sAw, const float* sAsc,
                                        const int* sRow, GRow grow, int tid, int wq, int wg, int l31, int h) {
  using T = std::conditional_t<ST == MMT_SEARCH_FP32, float, std::conditional_t<ST == MMT_SEARCH_FP8, uint8_t, bf16_t>>;
  f32x16 acc[2];
  tk_scan(acc, smem, {(const T*)a.a}, [=](int r) { return sRow[r]; }, (const T*)a.g, grow, a.K, tid, wq, wg, l31, h);
  __syncthreads();  // the slabs become the score tile
  const int M = a.M;
  const float* gw = a.gw;
  const auto row = [=](int r) { return wq * 32 + (r & 3) + 8 * (r >> 2) + 4 * h; };  // of accumulator element r
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int col = wg * 64 + t * 32 + l31, g = grow(col);
    float sc = 1.f, sim[16];
    if constexpr (ST == MMT_SEARCH_FP8) sc = g >= 0 ? a.gscale[g] : 1.f;
    tk_pair_sims<ST == MMT_SEARCH_FP8>(
        sim, acc[t], M, [=](int r, int m) { return sAw[row(r) * MMT_MAX_EXPERTS + m]; },
        [=](int m) { return g >= 0 ? gw[(int64_t)g * M + m] : 0.f; }, [=](int r) { return sAsc[row(r)]; }, sc);
#pragma unroll
    for (int r = 0; r < 16; ++r) sS[row(r) * TK_SLD + col] = sim[r];
  }
  __syncthreads();
}

template <int ST, int MODE>
__global__ __launch_bounds__(256) void self_kernel(SjArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int kRows = TK_Q / 4;  // rows per wave
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, h = lane >> 5, wq = wave >> 1, wg = wave & 1;
  const int bid = xcd_remap(blockIdx.x, gridDim.x);  // gallery-chunk-major: an XCD's blocks share their chunk in L2
  const int chunk = bid / a.n_qt, q0 = (bid % a.n_qt) * TK_Q;
  const int g_begin = chunk * a.chunk, g_end = min(a.NV, g_begin + a.chunk);
  const int rows_live = min(a.NQ - q0, TK_Q);

  float* sS = (float*)smem;                                  // [TK_Q][TK_SLD]  sims (after the K loop)
  float* sAw = (float*)(smem + SJ_UNION_BYTES);              // [TK_Q][MMT_MAX_EXPERTS]
  float* sAsc = sAw + TK_Q * MMT_MAX_EXPERTS;                // [TK_Q]
  int* sRow = (int*)(sAsc + TK_Q);                           // [TK_Q] stored row of A, -1 = none
  // top-k only, behind those: counts, thresholds, candidates, the rows' own items
  int* sN = sRow + TK_Q;                                     // [TK_Q]
  uint64_t* sT = (uint64_t*)(sN + TK_Q);                     // [TK_Q]
  uint64_t* sC = sT + TK_Q;                                  // [TK_Q][k + 64]
  const int cap = a.k + 64;
  int* sEx = (int*)(sC + (MODE == SJ_TOPK ? TK_Q * cap : 0));  // [TK_Q]

  // range only: the rows' thresholds, own items, hits so far and, for the fill, slots of this chunk
  TkRange<MODE == SJ_FILL, true> rg;
  if constexpr (MODE != SJ_TOPK) {
    if (!rg.init(a.thr, a.self, a.cnt, a.offsets, q0, rows_live, chunk, a.n_chunks, g_end - g_begin, wave, lane))
      return;  // block-uniform: no row of this block has a hit in this chunk
  }

  if (tid < TK_Q) {
    const int r = q0 + tid;
    int64_t v = -1;
    if (r < a.NQ) v = a.items ? a.items[r] : (int64_t)r;
    const int row = (v >= 0 && v < a.NA) ? (int)v : -1;  // outside A: none, never dereferenced
    sRow[tid] = row;
    if constexpr (ST == MMT_SEARCH_FP8) sAsc[tid] = row >= 0 ? a.ascale[row] : 1.f;
    if constexpr (MODE == SJ_TOPK) {
      sN[tid] = 0;
      sT[tid] = 0;
      sEx[tid] = (r < a.NQ && a.self) ? (int)a.self[r] : -1;
    }
  }
  __syncthreads();
  for (int i = tid; i < TK_Q * MMT_MAX_EXPERTS; i += 256) {  // read behind the barriers of the first K loop
    const int row = sRow[i / MMT_MAX_EXPERTS], m = i % MMT_MAX_EXPERTS;
    sAw[i] = (row >= 0 && m < a.M) ? a.aw[(int64_t)row * a.M + m] : 0.f;
  }

  for (int g0 = g_begin; g0 < g_end; g0 += TK_G) {
    uint64_t m0 = ~0ull, m1 = ~0ull;
    if (a.subset && !tk_tile_mask(a.subset, g0, m0, m1)) continue;  // block-uniform: nothing of this tile is allowed
    sj_tile<ST>(a, smem, sS, sAw, sAsc, sRow, [=](int r) { return g0 + r < g_end ? g0 + r : -1; }, tid, wq, wg, l31, h);
    if constexpr (MODE == SJ_TOPK) {
      tk_tile_select<true>(sS, sC, sN, sT, a.k, rows_live, g0, g_end, wave, lane, m0, m1, sEx, 1);
    } else {
      const bool live0 = g0 + lane < g_end && ((m0 >> lane) & 1ull), live1 = g0 + 64 + lane < g_end && ((m1 >> lane) & 1ull);
      rg.tile(sS, g0, live0, live1, rows_live, a.indices, a.scores, wave, lane);
    }
  }
  if constexpr (MODE == SJ_TOPK) {
    __syncthreads();
    uint64_t* ws = a.ws + chunk * (int64_t)a.k;
    const int64_t ws_row = (int64_t)a.n_chunks * a.k;
    for (int rr = 0; rr < kRows; ++rr) {
      const int row = wave * kRows + rr;
      if (row >= rows_live) break;
      tk_flush(sC + row * cap, sN[row], a.k, lane, ws + (q0 + row) * ws_row);
    }
  }
  if constexpr (MODE == SJ_COUNT) rg.flush(a.cnt, a.n_chunks, chunk);
}

namespace {
constexpr size_t kRangeLds = SJ_UNION_BYTES + SJ_ROWS_BYTES;
// ... and behind those, the top-k state: counts, thresholds, candidates, the rows' own items
size_t sj_topk_lds(int k) { return kRangeLds + TK_Q * (4 + 8) + (size_t)TK_Q * (k + 64) * 8 + TK_Q * 4; }

// The k = 128 footprint of the top-k kernels is over the 64 KiB default.
void sj_lds_limits() {
  static bool done[64] = {};
  const size_t most = sj_topk_lds(TK_MAXK);
  tk_lds_limits(done, {{(const void*)self_kernel<MMT_SEARCH_FP32, SJ_TOPK>, most},
                       {(const void*)self_kernel<MMT_SEARCH_BF16, SJ_TOPK>, most},
                       {(const void*)self_kernel<MMT_SEARCH_FP8, SJ_TOPK>, most}});
}

// The gate of the three entries, as mmt_search_pair_scores: 0 with `a` filled, or the error code.  `own`: the entry's
// other pointers are all there.
int sj_gate(SjArgs& a, const void* a_rows, const float* a_weights, const float* a_scales, int NA, const int64_t* items,
            const int64_t* self, int R, const void* g, const float* gw, const float* gscale, int NV, const uint32_t* subset,
            int storage, int M, int d, bool own) {
  const bool fp8 = storage == MMT_SEARCH_FP8;
  if (!a_rows || !a_weights || !g || !gw || !own || (unsigned)storage > MMT_SEARCH_FP8 || fp8 != (gscale != nullptr) ||
      fp8 != (a_scales != nullptr) || NA < 1 || (!items && R > NA) ||
      !tk_shape_ok(R, NV, M, d, storage != MMT_SEARCH_FP32, fp8))
    return MMT_ERR_ARG;
  if (((uintptr_t)a_rows | (uintptr_t)g | (uintptr_t)subset) & 15) return MMT_ERR_ALIGN;
  a = SjArgs{};
  a.a = a_rows; a.aw = a_weights; a.ascale = a_scales; a.items = items; a.self = self;
  a.g = g; a.gw = gw; a.gscale = gscale; a.subset = subset;
  a.NA = NA; a.NQ = R; a.NV = NV; a.M = M; a.K = M * d;
  tk_geometry(a);
  return 0;
}

template <int MODE>
void sj_launch(const SjArgs& a, int storage, size_t lds, hipStream_t st) {
  const dim3 grid(a.n_qt * a.n_chunks);
  switch (storage) {
    case MMT_SEARCH_FP32: hipLaunchKernelGGL((self_kernel<MMT_SEARCH_FP32, MODE>), grid, dim3(256), lds, st, a); break;
    case MMT_SEARCH_BF16: hipLaunchKernelGGL((self_kernel<MMT_SEARCH_BF16, MODE>), grid, dim3(256), lds, st, a); break;
    default: hipLaunchKernelGGL((self_kernel<MMT_SEARCH_FP8, MODE>), grid, dim3(256), lds, st, a); break;
  }
}
}  // namespace

extern "C" int64_t mmt_self_topk_workspace_keys(int R, int NV, int k) {
  if (R < 1 || NV < 1 || k < 1 || k > TK_MAXK) return MMT_ERR_ARG;
  return (int64_t)R * tk_n_chunks(R, NV) * k;
}

extern "C" int64_t mmt_self_range_workspace_ints(int R, int NV) {
  return tk_range_workspace_ints(R, NV);
}

extern "C" int mmt_search_self_topk(const void* a_rows, const float* a_weights, const float* a_scales, int NA,
                                    const int64_t* items, const int64_t* self, int R, const void* g, const float* gw,
                                    const float* gscale, int NV, const uint32_t* subset, int storage, int M, int d, int k,
                                    uint64_t* ws, float* scores, int64_t* index, void* stream) {
  SjArgs a;
  if (k < 1 || k > TK_MAXK) return MMT_ERR_ARG;
  if (const int rc = sj_gate(a, a_rows, a_weights, a_scales, NA, items, self, R, g, gw, gscale, NV, subset, storage, M, d,
                             ws && scores && index))
    return rc;
  a.ws = ws; a.k = k;
  sj_lds_limits();
  const hipStream_t st = (hipStream_t)stream;
  sj_launch<SJ_TOPK>(a, storage, sj_topk_lds(k), st);
  return tk_merge_launch(ws, R, a.n_chunks, k, k, scores, index, st);
}

extern "C" int mmt_search_self_range_count(const void* a_rows, const float* a_weights, const float* a_scales, int NA,
                                           const int64_t* items, const int64_t* self, int R, const void* g, const float* gw,
                                           const float* gscale, int NV, const uint32_t* subset, int storage, int M, int d,
                                           const float* thr, int32_t* ws, int64_t* row_counts, void* stream) {
  SjArgs a;
  if (const int rc = sj_gate(a, a_rows, a_weights, a_scales, NA, items, self, R, g, gw, gscale, NV, subset, storage, M, d,
                             thr && ws && row_counts))
    return rc;
  a.thr = thr; a.cnt = ws;
  const hipStream_t st = (hipStream_t)stream;
  sj_launch<SJ_COUNT>(a, storage, kRangeLds, st);
  return rg_offsets_launch(ws, R, a.n_chunks, row_counts, st);
}

extern "C" int mmt_search_self_range_fill(const void* a_rows, const float* a_weights, const float* a_scales, int NA,
                                          const int64_t* items, const int64_t* self, int R, const void* g, const float* gw,
                                          const float* gscale, int NV, const uint32_t* subset, int storage, int M, int d,
                                          const float* thr, const int32_t* ws, const int64_t* offsets, int64_t* indices,
                                          float* scores, void* stream) {
  SjArgs a;
  if (const int rc = sj_gate(a, a_rows, a_weights, a_scales, NA, items, self, R, g, gw, gscale, NV, subset, storage, M, d,
                             thr && ws && offsets && indices && scores))
    return rc;
  a.thr = thr; a.cnt = const_cast<int32_t*>(ws); a.offsets = offsets; a.indices = indices; a.scores = scores;
  sj_launch<SJ_FILL>(a, storage, kRangeLds, (hipStream_t)stream);
  return (int)hipGetLastError();
}
