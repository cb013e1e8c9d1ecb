// The gallery self-join (search.py: VideoIndex.neighbours, neighbour_range, duplicate_groups): the stored items searched
// against the stored items, as a streaming scan -- per row item its k best stored items, or every stored item at or above
// a threshold as a CSR -- without the NV x NV matrix.  The quantity is the one of search_diverse.hip,
//   sim(g, h) = <f_g, f_h> / sum_m gw_g[m] gw_h[m]      (0 -> 1e-5)
// f_g the dequantised stored row, and every score here has the bits pair_scores_kernel gives the pair: the K loops below
// are written next to dv_gram_f32 / dv_gram_b16 and run their slab and MFMA sequence -- kb ascending in the slab widths
// of search_scan.h, kk ascending, u ascending, ONE accumulator per output, fp32 rows on v_mfma_f32_32x32x2_f32, bf16 rows
// and fp8 codes widened exactly (tk_widen_fp8) on one v_mfma_f32_32x32x16_bf16 per fragment, no hi / lo pair -- and the
// epilogue is that kernel's: den = fma(gw_g[m], gw_h[m], den) for m ascending, fp8: num = fl(acc * fl(scale_g * scale_h))
// (tk_mul_rn), sim = num / den.  search_scan.h, search_topk.h and every other .hip file are only read.
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
//   self_kernel<ST, SJ_COUNT>, <ST, SJ_FILL> : the count and the fill step of range_kernel (search_range.hip) restated:
//                              `live && item != self && score >= thr[row]`, two ballots per row and tile, the popcounts
//                              summed in the lane that holds the row; self_offsets_kernel turns a row's chunk counts into
//                              their exclusive prefix; the fill writes a hit to offsets[r] + prefix + hits before it, the
//                              position clamped against the start of the row's next chunk.
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

// fp32 K loop of one 64 x 128 tile, both operands stored rows: acc = A[sRow[.]] . G[grow(.)]^T.  tk_scan_f32 with the A
// slab read through the row table; the slab and MFMA sequence of dv_gram_f32.  Opens with a barrier, leaves the last
// slab's reads unfenced.
template <class GRow>
__device__ __forceinline__ void sj_scan_f32(f32x16 (&acc)[2], unsigned char* smem, const float* a, const int* sRow,
                                            const float* g, int K, GRow grow, int tid, int wq, int wg, int l31, int h) {
  float* sA = (float*)smem;        // [TK_Q][TK_LD]
  float* sB = sA + TK_Q * TK_LD;   // [TK_G][TK_LD]
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  int ar[2], gr[4];
#pragma unroll
  for (int j = 0; j < 2; ++j) ar[j] = sRow[(tid + 256 * j) >> 3];
#pragma unroll
  for (int j = 0; j < 4; ++j) gr[j] = grow((tid + 256 * j) >> 3);
  f32x4 ra[2], rb[4];
  auto load = [&](int kb) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int c = kb + ((tid + 256 * j) & 7) * 4;
      ra[j] = (ar[j] >= 0 && c < K) ? *(const f32x4*)(a + (int64_t)ar[j] * K + c) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = kb + ((tid + 256 * j) & 7) * 4;
      rb[j] = (gr[j] >= 0 && c < K) ? *(const f32x4*)(g + (int64_t)gr[j] * K + c) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
  };
  load(0);
  for (int kb = 0; kb < K; kb += TK_BK) {
    __syncthreads();  // previous slab (or the previous tile's scores) consumed
#pragma unroll
    for (int j = 0; j < 2; ++j) { const int i = tid + 256 * j; *(f32x4*)(sA + (i >> 3) * TK_LD + (i & 7) * 4) = ra[j]; }
#pragma unroll
    for (int j = 0; j < 4; ++j) { const int i = tid + 256 * j; *(f32x4*)(sB + (i >> 3) * TK_LD + (i & 7) * 4) = rb[j]; }
    __syncthreads();
    if (kb + TK_BK < K) load(kb + TK_BK);
    // 8 contraction values per step; lane half h feeds k = kk + 4h + u to MFMA u (as dv_gram_f32)
#pragma unroll
    for (int kk = 0; kk < TK_BK; kk += 8) {
      const f32x4 av = *(const f32x4*)(sA + (wq * 32 + l31) * TK_LD + kk + 4 * h);
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const f32x4 bv = *(const f32x4*)(sB + (wg * 64 + t * 32 + l31) * TK_LD + kk + 4 * h);
#pragma unroll
        for (int u = 0; u < 4; ++u) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u], bv[u], acc[t], 0, 0, 0);
      }
    }
  }
}

// The same over rows stored in 16 bits or fewer: bf16 as they are, fp8 widened exactly to bf16 on the way into LDS, on
// BOTH sides; one MFMA per fragment (as dv_gram_b16).  A slab: 64 rows x 64 elements = 8 (bf16) or 4 (fp8) sixteen-byte
// loads per row, 2 or 1 per thread; B slab: 128 rows, 4 or 2 per thread.
template <bool FP8, class GRow>
__device__ __forceinline__ void sj_scan_b16(f32x16 (&acc)[2], unsigned char* smem, const void* a, const int* sRow,
                                            const void* g, int K, GRow grow, int tid, int wq, int wg, int l31, int h) {
  constexpr int NA_ = FP8 ? 1 : 2;   // A loads per thread and slab
  constexpr int NB = FP8 ? 2 : 4;    // B loads per thread and slab
  constexpr int SH = FP8 ? 2 : 3;    // log2 of the loads per row and slab
  constexpr int EL = FP8 ? 16 : 8;   // elements per load
  bf16_t* sA = (bf16_t*)smem;           // [TK_Q][TKB_LD]
  bf16_t* sB = sA + TK_Q * TKB_LD;      // [TK_G][TKB_LD]
  const u32x4 zero = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  int ar[NA_], gr[NB];
#pragma unroll
  for (int j = 0; j < NA_; ++j) ar[j] = sRow[(tid + 256 * j) >> SH];
#pragma unroll
  for (int j = 0; j < NB; ++j) gr[j] = grow((tid + 256 * j) >> SH);
  u32x4 ra[NA_], rb[NB];
  auto fetch = [&](const void* base, int row, int c) {
    const int64_t off = (int64_t)row * K + c;
    if (row < 0 || c >= K) return zero;
    if constexpr (FP8)
      return *(const u32x4*)((const uint8_t*)base + off);
    else
      return *(const u32x4*)((const bf16_t*)base + off);
  };
  auto load = [&](int kb) {
#pragma unroll
    for (int j = 0; j < NA_; ++j) ra[j] = fetch(a, ar[j], kb + ((tid + 256 * j) & ((1 << SH) - 1)) * EL);
#pragma unroll
    for (int j = 0; j < NB; ++j) rb[j] = fetch(g, gr[j], kb + ((tid + 256 * j) & ((1 << SH) - 1)) * EL);
  };
  auto stage = [&](bf16_t* slab, int i, const u32x4& v) {
    bf16_t* dst = slab + (i >> SH) * TKB_LD + (i & ((1 << SH) - 1)) * EL;
    if constexpr (FP8) {
      u32x4 lo, hi;
      tk_widen_fp8(v, lo, hi);
      *(u32x4*)dst = lo;
      *(u32x4*)(dst + 8) = hi;
    } else {
      *(u32x4*)dst = v;
    }
  };
  load(0);
  for (int kb = 0; kb < K; kb += TKB_BK) {
    __syncthreads();  // previous slab (or the previous tile's scores) consumed
#pragma unroll
    for (int j = 0; j < NA_; ++j) stage(sA, tid + 256 * j, ra[j]);
#pragma unroll
    for (int j = 0; j < NB; ++j) stage(sB, tid + 256 * j, rb[j]);
    __syncthreads();
    if (kb + TKB_BK < K) load(kb + TKB_BK);
    // 16 contraction values per MFMA; lane half h holds k = kk + 8h .. + 7 of its row (as dv_gram_b16)
#pragma unroll
    for (int kk = 0; kk < TKB_BK; kk += 16) {
      const bf16x8_t av = *(const bf16x8_t*)(sA + (wq * 32 + l31) * TKB_LD + kk + 8 * h);
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const bf16x8_t bv = *(const bf16x8_t*)(sB + (wg * 64 + t * 32 + l31) * TKB_LD + kk + 8 * h);
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, bv, acc[t], 0, 0, 0);
      }
    }
  }
}

// One 64 x 128 tile of sims in sS [TK_Q][TK_SLD]: the K loop and the epilogue of pair_scores_kernel -- the rows' weights
// (sAw [TK_Q][MMT_MAX_EXPERTS], zero past M and for no row) and, fp8, scales (sAsc [TK_Q]) from LDS, the column's read
// per lane.  Ends fenced.
template <int ST, class GRow>
__device__ __forceinline__ void sj_tile(const SjArgs& a, unsigned char* smem, float* sS, const float* sAw, const float* sAsc,
                                        const int* sRow, GRow grow, int tid, int wq, int wg, int l31, int h) {
  f32x16 acc[2];
  if constexpr (ST == MMT_SEARCH_FP32)
    sj_scan_f32(acc, smem, (const float*)a.a, sRow, (const float*)a.g, a.K, grow, tid, wq, wg, l31, h);
  else
    sj_scan_b16<ST == MMT_SEARCH_FP8>(acc, smem, a.a, sRow, a.g, a.K, grow, tid, wq, wg, l31, h);
  __syncthreads();  // the slabs become the score tile
  const int M = a.M;
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int col = wg * 64 + t * 32 + l31, g = grow(col);
    float sc = 1.f;
    if constexpr (ST == MMT_SEARCH_FP8) sc = g >= 0 ? a.gscale[g] : 1.f;
    float den[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) den[r] = 0.f;
    for (int m = 0; m < M; ++m) {
      const float gwm = g >= 0 ? a.gw[(int64_t)g * M + m] : 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r)
        den[r] = __builtin_fmaf(sAw[(wq * 32 + (r & 3) + 8 * (r >> 2) + 4 * h) * MMT_MAX_EXPERTS + m], gwm, den[r]);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = wq * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
      float num = acc[t][r];
      if constexpr (ST == MMT_SEARCH_FP8) num = tk_mul_rn(num, tk_mul_rn(sAsc[row], sc));
      sS[row * TK_SLD + col] = num / (den[r] == 0.f ? 1e-5f : den[r]);
    }
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

  // range only: lane l < 16 of wave w holds the state of row 16 w + l for the whole block (as range_kernel)
  const int my_row = wave * kRows + lane;
  const bool holder = lane < kRows && my_row < rows_live;
  float my_thr = __builtin_nanf("");
  int my_self = -1, my_cnt = 0, my_cap = 0;
  int64_t my_base = 0;
  if constexpr (MODE != SJ_TOPK) {
    if (holder) {
      my_thr = a.thr[q0 + my_row];
      if (a.self) my_self = (int)a.self[q0 + my_row];
    }
  }
  if constexpr (MODE == SJ_FILL) {
    if (holder) {
      const int64_t q = q0 + my_row, off = a.offsets[q];
      const int32_t* pre = a.cnt + q * a.n_chunks + chunk;
      my_base = off + pre[0];
      const int64_t next = chunk + 1 < a.n_chunks ? off + pre[1] : a.offsets[q + 1];
      const int64_t room = next - my_base;  // never beyond the row's next chunk, nor more than the chunk has items
      my_cap = room < 0 ? 0 : room > g_end - g_begin ? g_end - g_begin : (int)room;
    }
    if (!__syncthreads_or(my_cap > 0)) return;  // block-uniform: no row of this block has a hit in this chunk
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
      const int c0 = g0 + lane, c1 = g0 + 64 + lane;
      const bool live0 = c0 < g_end && ((m0 >> lane) & 1ull), live1 = c1 < g_end && ((m1 >> lane) & 1ull);
      for (int rr = 0; rr < kRows; ++rr) {
        const int row = wave * kRows + rr;
        if (row >= rows_live) break;
        const float s0 = sS[row * TK_SLD + lane], s1 = sS[row * TK_SLD + 64 + lane];
        const float thr = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_thr), rr));
        const int own = __builtin_amdgcn_readlane(my_self, rr);  // the self pair goes by item number, not by score
        const bool hit0 = live0 && c0 != own && s0 >= thr, hit1 = live1 && c1 != own && s1 >= thr;
        const uint64_t b0 = __ballot(hit0), b1 = __ballot(hit1);
        const int n0 = __popcll(b0), n1 = __popcll(b1);
        if constexpr (MODE == SJ_FILL) {
          if (b0 | b1) {  // wave-uniform
            const int seen = __builtin_amdgcn_readlane(my_cnt, rr), room = __builtin_amdgcn_readlane(my_cap, rr);
            const int64_t base = (int64_t)(((uint64_t)(unsigned)__builtin_amdgcn_readlane((int)(my_base >> 32), rr) << 32) |
                                           (unsigned)__builtin_amdgcn_readlane((int)my_base, rr));
            const uint64_t below = (1ull << lane) - 1;
            const int p0 = seen + __popcll(b0 & below), p1 = seen + n0 + __popcll(b1 & below);
            if (hit0 && p0 < room) {
              a.indices[base + p0] = c0;
              a.scores[base + p0] = s0;
            }
            if (hit1 && p1 < room) {
              a.indices[base + p1] = c1;
              a.scores[base + p1] = s1;
            }
          }
        }
        if (lane == rr) my_cnt += n0 + n1;
      }
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
  if constexpr (MODE == SJ_COUNT) {
    if (holder) a.cnt[(int64_t)(q0 + my_row) * a.n_chunks + chunk] = my_cnt;
  }
}

// One thread per row: the chunk counts become their exclusive prefix, in chunk order; the row total as int64.
__global__ __launch_bounds__(256) void self_offsets_kernel(int32_t* __restrict__ cnt, int R, int n_chunks,
                                                           int64_t* __restrict__ row_counts) {
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= R) return;
  int32_t* row = cnt + (int64_t)q * n_chunks;
  int run = 0;
  for (int c = 0; c < n_chunks; ++c) {
    const int n = row[c];
    row[c] = run;
    run += n;
  }
  row_counts[q] = run;
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
  if (R < 1 || NV < 1) return MMT_ERR_ARG;
  return (int64_t)R * tk_n_chunks(R, NV);
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
  hipLaunchKernelGGL(self_offsets_kernel, dim3((R + 255) / 256), dim3(256), 0, st, ws, R, a.n_chunks, row_counts);
  return (int)hipGetLastError();
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
