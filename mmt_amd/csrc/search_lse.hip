// Softmax over the gallery without the N_query x N_gallery matrix (search.py: query_lse, search_softmax): the row-wise
// log-partition of softmax(beta * score(q, .)) over a query's candidates, as a sum that is ONE number whatever the
// chunking, the row batching, the launch geometry, the item order or the shard -- an integer sum.  In fp32 unless stated:
//
//   x(q, g) = fl(beta * score(q, g))                          one rounded multiply (tk_mul_rn), as tk_tile_col_stats
//   e(q, g) = expf(x(q, g) - xmax[q])                         xmax[q] = fl(beta * top-1 score of q): the caller's search(k=1)
//   t(q, g) = (int64) rint(ldexpf(e(q, g), F))                F = 62 - ceil(log2(max(num_items, 2))), from the caller
//   T[q]    = sum over the candidates g of t(q, g)            int64, exact: t <= 2^F and num_items <= 2^(62 - F)
//
// with score the value of the plain scan, bit for bit: the tile is tk_tile's (search_scan.h), so the K loops, the gated
// denominator and the fp8 scales are the scans' own.  The host turns T into lse = xmax + log T - F ln 2 in float64.
//
//   row_expsum_kernel<BF16, FP8> : the scan of the count kernels (block = 64 query rows x one gallery chunk, tk_geometry,
//                                  xcd_remap) with the selection replaced by the sum: four threads per row, thread p of a
//                                  row takes columns p, p + 4, .. of every 64 x 128 score tile in LDS (the 132-float row
//                                  pitch puts the 32 (row, p) pairs of a half wave on 32 banks) and adds t of every live,
//                                  allowed column into an int64 register that lives across the chunk's tiles.  At the end
//                                  of the chunk the four partials of a row meet by two lane exchanges -- integers, so in
//                                  any order -- and thread p = 0 writes ws[q][chunk].  With a subset a tile without an
//                                  allowed item is skipped before its K loop (tk_tile_mask) and a chunk without one
//                                  writes 0.
// The caller sums ws over the chunks.  No atomics, one writer per slot.  Rows past NQ, columns past NV and columns whose
// subset bit is clear add nothing; a column that is no candidate may hold any score (e above 1, inf, NaN): its
// exponential is replaced by 0 before it is made an integer (ls_term).
#include "search_scan.h"

template <bool FP8>
struct LsArgs {
  const void* q;           // fp32: Q' [NQ][K]; bf16 / fp8: hi(Q')
  const void* q_lo;        // bf16 / fp8: lo(Q')
  const float* qw;         // [NQ][M]
  const void* g;           // [NV][K] fp32, bf16 bits or e4m3fn codes
  const float* gw;         // [NV][M]
  const float* gscale;     // fp8: [NV]
  const uint32_t* subset;  // bit g & 31 of word g >> 5 allows item g (null = all; 16-byte aligned)
  const float* xmax;       // [NQ]
  int64_t* ws;             // [NQ][n_chunks]
  float beta;
  int F;
  int NQ, NV, M, K, chunk, n_qt, n_chunks;
  static constexpr bool kFp8 = FP8;
};

// The term of one pair: rint(e * 2^F) as an integer.  ldexpf is exact (F >= 0 scales up; a result below one half rounds
// to 0 whether or not a subnormal e was flushed on the way) and e <= 1 gives a value <= 2^F <= 2^62.  A column that is
// no candidate may hold any score (e above 1, inf, NaN), which no int64 holds: its e is replaced by 0 BEFORE the
// conversion, so only values of 0 .. 2^F are ever converted.
__device__ __forceinline__ int64_t ls_term(float score, float beta, float xmax, int F, bool candidate) {
  const float e = candidate ? expf(tk_mul_rn(beta, score) - xmax) : 0.f;
  return (int64_t)rintf(ldexpf(e, F));
}

template <bool BF16, bool FP8>
__global__ __launch_bounds__(256) void row_expsum_kernel(LsArgs<FP8> a) {
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
  // thread (row, p): columns p, p + 4, ..., p + 124 of its row, for the whole block
  const int row = tid >> 2, p = tid & 3;
  const bool mine = row < rows_live;
  const float xmax = mine ? a.xmax[q0 + row] : 0.f;
  const float* srow = sS + row * TK_SLD + p;
  int64_t sum = 0;
  tk_load_qw(sQw, a.qw, a.NQ, a.M, q0, tid);  // read after the barriers of the first K loop
  for (int g0 = g_begin; g0 < g_end; g0 += TK_G) {
    uint64_t m0 = ~0ull, m1 = ~0ull;
    if (a.subset && !tk_tile_mask(a.subset, g0, m0, m1)) continue;  // block-uniform: nothing of this tile is allowed
    tk_tile<BF16, false>(a, smem, sS, sQw, q0, [=](int r) { return g0 + r < g_end ? g0 + r : -1; }, tid, wq, wg, l31, h);
    if (mine) {
      const int left = g_end - g0;  // live columns of the tile: 0 .. left - 1
#pragma unroll 8
      for (int j = 0; j < TK_G / 4; ++j) {
        const int c = p + 4 * j;
        const bool allowed = c < left && (((c < 64 ? m0 : m1) >> (c & 63)) & 1ull);
        sum += ls_term(srow[4 * j], a.beta, xmax, a.F, allowed);
      }
    }
    // the next tile's K loop opens with a barrier: the scores are consumed before the slabs overwrite them
  }
  // the four partials of a row: lanes 4r .. 4r + 3 of one wave
  sum += __shfl_xor((long long)sum, 1);
  sum += __shfl_xor((long long)sum, 2);
  if (mine && p == 0) a.ws[(int64_t)(q0 + row) * a.n_chunks + chunk] = sum;
}

namespace {
template <bool BF16, bool FP8>
int ls_row_expsum(const MmtSearchScan& s, float beta, const float* xmax, int F, int64_t* ws, void* stream) {
  if (!tk_scan_operands<BF16, FP8>(s) || !xmax || !ws || !tk_beta_ok(beta) || F < 0 || F > 62 ||
      !tk_shape_ok(s.NQ, s.NV, s.M, s.d, BF16, FP8))
    return MMT_ERR_ARG;
  if (!tk_scan_aligned(s)) return MMT_ERR_ALIGN;
  LsArgs<FP8> a = {};
  a.q = s.q; a.q_lo = s.q_lo; a.qw = s.qw; a.g = s.g; a.gw = s.gw; a.gscale = s.gscale; a.subset = s.subset;
  a.xmax = xmax; a.ws = ws; a.beta = beta; a.F = F;
  a.NQ = s.NQ; a.NV = s.NV; a.M = s.M; a.K = s.M * s.d;
  tk_geometry(a);
  static bool done[64] = {};
  tk_lds_limits(done, {{(const void*)row_expsum_kernel<BF16, FP8>, tk_base_lds<BF16>()}});
  hipLaunchKernelGGL((row_expsum_kernel<BF16, FP8>), dim3(a.n_qt * a.n_chunks), dim3(256), tk_base_lds<BF16>(),
                     (hipStream_t)stream, a);
  return (int)hipGetLastError();
}
}  // namespace

extern "C" int64_t mmt_row_expsum_workspace_ints64(int NQ, int NV) {
  if (NQ <= 0 || NV <= 0) return MMT_ERR_ARG;
  return (int64_t)NQ * tk_n_chunks(NQ, NV);
}

extern "C" int mmt_search_row_expsum(const MmtSearchScan* scan, float beta, const float* xmax, int F, int64_t* ws,
                                     void* stream) {
  if (const int rc = tk_scan_gate(scan, SC_SUBSET | SC_FP8)) return rc;
  switch (scan->storage) {
    case MMT_SEARCH_FP32: return ls_row_expsum<false, false>(*scan, beta, xmax, F, ws, stream);
    case MMT_SEARCH_BF16: return ls_row_expsum<true, false>(*scan, beta, xmax, F, ws, stream);
    default: return ls_row_expsum<true, true>(*scan, beta, xmax, F, ws, stream);
  }
}
