// Querybank hubness normalisation of the gallery scans (inverted softmax, the static half of QB-Norm: Bogolin et al.,
// CVPR 2022; search.py: VideoIndex.hub_norm and the norm= of search / rank_counts).  For a bank of NB queries and a
// temperature beta > 0, all in fp32,
//
//   x(b, g)      = fl(beta * score(b, g))                      one rounded multiply
//   lse[g]       = log sum_b exp(x(b, g))                      blockwise, below
//   score'(q, g) = fl(fl(beta * score(q, g)) - lse[g])         a rounded multiply, then a rounded subtract: no fma
//
// with score the value of the plain scan, bit for bit: every kernel here scores its tile with the K loops and the epilogue
// of search_scan.h and the bank rows as the QUERY operand.  score' is the log of the inverted-softmax probability, so
// ordering by it is ordering by that probability.  Nothing here forms a bank x gallery or query x gallery matrix.
//
//   col_lse_kernel<BF16>       : the scan of the top-k kernel (block = 64 bank rows x one gallery chunk, same chunk rule,
//                                same XCD remap) with the selection replaced by a column pass: per 64 x 128 score tile in
//                                LDS thread c takes column c and the live rows in ascending order, m = max x,
//                                p = sum exp(x - m) (tk_tile_col_stats), and writes (m, p) to part[bank block][item].
//   col_lse_fold_kernel        : one thread per item: the carried (M, S) of the earlier bank batches (or the first block's
//                                (m, p)) folded with this batch's blocks in ascending order, M' = max(M, m),
//                                S' = S exp(M - M') + p exp(m - M'); (M, S) goes back to the state and, when asked,
//                                lse = M + log S comes out.
//                                Schedule: "bank in batches".  The bank streams through in batches of whole 64-row blocks;
//                                a launch fills the chip whatever the gallery size and the partials are bounded by the
//                                caller's batch.  lse[g] is a function of item g's stored row and weights, the bank in its
//                                row order and beta: (m, p) of a block depends on that block's 64 rows and the item only
//                                (the score does not depend on NV, the position or the chunk; the column pass runs in row
//                                order), and the fold runs over the blocks in ascending order with the same instructions
//                                whether a block is the next of this batch or the first of the next (the state is the
//                                fp32 pair itself).  A batch boundary is a multiple of 64 rows, so the blocks are the same
//                                however the bank is batched.  No atomics, one writer per slot.
// The scans on score' are instantiations of the shared bodies with the rewrite switched on (tk_tile<., true> of
// search_scan.h): topk_scan_kernel<., NmTopkArgs> (search.hip), rank_kernel<., ., NmRankArgs> (search_rank.hip).  NmArgs is
// in search_scan.h.
#include "search_scan.h"

template <bool BF16>
__global__ __launch_bounds__(256) void col_lse_kernel(NmArgs a, float2* __restrict__ part) {
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
  tk_load_qw(sQw, a.qw, a.NQ, a.M, q0, tid);
  for (int g0 = g_begin; g0 < g_end; g0 += TK_G) {
    tk_tile<BF16, false>(a, smem, sS, sQw, q0, [=](int r) { return g0 + r < g_end ? g0 + r : -1; }, tid, wq, wg, l31, h);
    if (tid < TK_G && g0 + tid < g_end) {
      float m, p;
      tk_tile_col_stats(sS, a.beta, rows_live, tid, m, p);
      part[(int64_t)qt * a.NV + g0 + tid] = make_float2(m, p);
    }
  }
}

// state: M [NV] then S [NV].  first: the state is not read, block 0 of `part` starts it.
__global__ __launch_bounds__(256) void col_lse_fold_kernel(const float2* __restrict__ part, int n_blocks, int NV,
                                                           float* __restrict__ state, int first, float* __restrict__ lse) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= NV) return;
  float M, S;
  int i = 0;
  if (first) {
    const float2 v = part[g];
    M = v.x; S = v.y; i = 1;
  } else {
    M = state[g]; S = state[(int64_t)NV + g];
  }
  for (; i < n_blocks; ++i) {
    const float2 v = part[(int64_t)i * NV + g];
    const float Mn = fmaxf(M, v.x);
    S = S * expf(M - Mn) + v.y * expf(v.x - Mn);
    M = Mn;
  }
  state[g] = M;
  state[(int64_t)NV + g] = S;
  if (lse) lse[g] = M + logf(S);
}

namespace {
template <bool BF16>
int nm_col_lse(const MmtSearchScan& s, float beta, float* ws, float* state, int first, float* lse, void* stream) {
  if (!tk_scan_operands<BF16>(s) || !ws || !state || !tk_shape_ok(s.NQ, s.NV, s.M, s.d, BF16) || !tk_beta_ok(beta))
    return MMT_ERR_ARG;
  if (!tk_scan_aligned(s) || ((uintptr_t)ws & 15)) return MMT_ERR_ALIGN;
  NmArgs a = {};
  a.q = s.q; a.q_lo = s.q_lo; a.qw = s.qw; a.g = s.g; a.gw = s.gw; a.beta = beta;
  a.NQ = s.NQ; a.NV = s.NV; a.M = s.M; a.K = s.M * s.d;
  tk_geometry(a);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(col_lse_kernel<BF16>, dim3(a.n_qt * a.n_chunks), dim3(256), tk_base_lds<BF16>(), st, a, (float2*)ws);
  hipLaunchKernelGGL(col_lse_fold_kernel, dim3((s.NV + 255) / 256), dim3(256), 0, st, (const float2*)ws, a.n_qt, s.NV, state,
                     first, lse);
  return (int)hipGetLastError();
}
}  // namespace

extern "C" int64_t mmt_col_lse_workspace_floats(int NB, int NV) {
  if (NB <= 0 || NV <= 0) return MMT_ERR_ARG;
  return 2 * (int64_t)((NB + TK_Q - 1) / TK_Q) * NV;
}

// The descriptor's own lse and beta stay null / 0 (the gate takes no norm): this operation writes the lse.
extern "C" int mmt_search_col_lse(const MmtSearchScan* scan, float beta, float* ws, float* state, int first, float* lse,
                                  void* stream) {
  if (const int rc = tk_scan_gate(scan, 0)) return rc;
  return scan->storage == MMT_SEARCH_FP32 ? nm_col_lse<false>(*scan, beta, ws, state, first, lse, stream)
                                          : nm_col_lse<true>(*scan, beta, ws, state, first, lse, stream);
}
