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
//   topk_norm_kernel<BF16>     : topk_chunk_kernel<true, true> (search.hip) / topk_chunk_bf16_kernel<true> with one more
//                                pass between the score epilogue and the selection: tk_tile_norm rewrites the tile to
//                                score'.  Subset bitmap (nullable), exclusions (E = 0 allowed), keys, ties, workspace and
//                                the merge launch are those of the masked search; the returned scores are score'.
//   rank_norm_kernel<BF16,THR> : the two halves of the rank pass on score': THR = true gives thr[q][t] = score'(q, target)
//                                from the same tile code (NaN for a target outside 0 .. NV - 1), THR = false counts
//                                score' against given thresholds, subset nullable; nm_reduce_kernel sums the chunks.
// The plain kernels are not touched: these are kernels of their own on the shared tile helpers.
#include <cmath>

#include "search_topk.h"

#define NM_MAXT 32

struct NmArgs {
  const void* q;        // fp32: Q' [NQ][K]; bf16: hi(Q')
  const void* q_lo;     // bf16: lo(Q')
  const float* qw;      // [NQ][M]
  const void* g;        // [NV][K] fp32 or bf16 bits
  const float* gw;      // [NV][M]
  const float* lse;     // [NV] (the lse pass: unused)
  float beta;
  int NQ, NV, M, K, chunk, n_qt, n_chunks;
};

struct NmTopkArgs : NmArgs {
  uint64_t* ws;             // [NQ][n_chunks][k]
  const uint32_t* subset;   // nullable = all
  const int64_t* exclude;   // [NQ][E]
  int k, E;
};

struct NmRankArgs : NmArgs {
  const int64_t* targets;   // THR: [NQ][T]
  float* thr;               // [NQ][T]
  int32_t* cnt;             // count: [NQ][T][n_chunks][2]
  const uint32_t* subset;   // count: nullable = all
  int T;
};

// One 64 x 128 tile of plain scores in sS, then (NORM) rewritten to score'.  Ends fenced.
template <bool BF16, bool NORM, class GRow>
__device__ __forceinline__ void nm_tile(const NmArgs& a, unsigned char* smem, float* sS, const float* sQw, int q0, GRow grow,
                                        int tid, int wq, int wg, int l31, int h) {
  f32x16 acc[2];
  if constexpr (BF16)
    tk_scan_bf16(acc, smem, (const bf16_t*)a.q, (const bf16_t*)a.q_lo, (const bf16_t*)a.g, a.NQ, a.K, q0, grow, tid, wq, wg,
                 l31, h);
  else
    tk_scan_f32(acc, smem, (const float*)a.q, (const float*)a.g, a.NQ, a.K, q0, grow, tid, wq, wg, l31, h);
  __syncthreads();  // the slabs become the score tile
  tk_tile_scores(acc, sS, sQw, a.gw, a.M, grow, wq, wg, l31, h);
  __syncthreads();
  if constexpr (NORM) {
    tk_tile_norm(sS, a.lse, a.beta, grow, tid);
    __syncthreads();
  }
}

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
    nm_tile<BF16, false>(a, smem, sS, sQw, q0, [=](int r) { return g0 + r < g_end ? g0 + r : -1; }, tid, wq, wg, l31, h);
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

template <bool BF16>
__global__ __launch_bounds__(256) void topk_norm_kernel(NmTopkArgs a) {
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
  int* sEx = (int*)(sC + TK_Q * cap);                         // [TK_Q][E] exclusions
  const int l31 = lane & 31, h = lane >> 5, wq = wave >> 1, wg = wave & 1;
  if (tid < TK_Q) { sN[tid] = 0; sT[tid] = 0; }
  tk_load_qw(sQw, a.qw, a.NQ, a.M, q0, tid);
  for (int i = tid; i < TK_Q * a.E; i += 256) sEx[i] = q0 + i / a.E < a.NQ ? (int)a.exclude[(int64_t)q0 * a.E + i] : -1;
  for (int g0 = g_begin; g0 < g_end; g0 += TK_G) {
    uint64_t m0 = ~0ull, m1 = ~0ull;
    if (a.subset) {
      const u32x4 w = *(const u32x4*)(a.subset + (g0 >> 5));
      m0 = w[0] | (uint64_t)w[1] << 32;
      m1 = w[2] | (uint64_t)w[3] << 32;
      if (!(m0 | m1)) continue;  // block-uniform: nothing of this tile is allowed
    }
    nm_tile<BF16, true>(a, smem, sS, sQw, q0, [=](int r) { return g0 + r < g_end ? g0 + r : -1; }, tid, wq, wg, l31, h);
    tk_tile_select<true>(sS, sC, sN, sT, a.k, a.NQ - q0, g0, g_end, wave, lane, m0, m1, sEx, a.E);
  }
  __syncthreads();
  for (int rr = 0; rr < TK_Q / 4; ++rr) {
    const int row = wave * (TK_Q / 4) + rr, q = q0 + row;
    if (q >= a.NQ) break;
    tk_flush(sC + row * cap, sN[row], a.k, lane, ws + q * ws_row);
  }
}

template <bool BF16, bool THR>
__global__ __launch_bounds__(256) void rank_norm_kernel(NmRankArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int kUnion = BF16 ? TKB_UNION_BYTES : TK_UNION_BYTES;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, h = lane >> 5, wq = wave >> 1, wg = wave & 1;
  const int T = a.T;
  float* sS = (float*)smem;                       // [TK_Q][TK_SLD]  scores (after the K loop)
  float* sQw = (float*)(smem + kUnion);           // [TK_Q][MMT_MAX_EXPERTS]
  if constexpr (THR) {  // rank_kernel<BF16, true> of search_rank.hip on score'
    int* sRow = (int*)(sQw + TK_Q * MMT_MAX_EXPERTS);  // [TK_G] gallery row of the tile's columns
    const int q0 = (blockIdx.x % a.n_qt) * TK_Q, p0 = (blockIdx.x / a.n_qt) * TK_G;
    const int64_t pairs = ((int64_t)min(a.NQ - q0, TK_Q)) * T;  // live (query, target) pairs of this query tile
    tk_load_qw(sQw, a.qw, a.NQ, a.M, q0, tid);
    if (tid < TK_G) {
      const int64_t tg = p0 + tid < pairs ? a.targets[(int64_t)q0 * T + p0 + tid] : -1;
      sRow[tid] = (tg >= 0 && tg < a.NV) ? (int)tg : -1;
    }
    __syncthreads();
    nm_tile<BF16, true>(a, smem, sS, sQw, q0, [=](int r) { return sRow[r]; }, tid, wq, wg, l31, h);
    if (tid < TK_G && p0 + tid < pairs)
      a.thr[(int64_t)q0 * T + p0 + tid] = sRow[tid] >= 0 ? sS[((p0 + tid) / T) * TK_SLD + tid] : __builtin_nanf("");
  } else {  // rank_kernel<BF16, false, true> on score', the subset nullable
    float* sThr = sQw + TK_Q * MMT_MAX_EXPERTS;   // [TK_Q][T]
    int* sCnt = (int*)(sThr + TK_Q * T);          // [TK_Q][T][2]
    const int bid = xcd_remap(blockIdx.x, gridDim.x);
    const int chunk = bid / a.n_qt, q0 = (bid % a.n_qt) * TK_Q;
    const int g_begin = chunk * a.chunk, g_end = min(a.NV, g_begin + a.chunk);
    const int rows_live = min(a.NQ - q0, TK_Q);
    tk_load_qw(sQw, a.qw, a.NQ, a.M, q0, tid);
    for (int i = tid; i < TK_Q * T; i += 256) {
      sThr[i] = i < rows_live * T ? a.thr[(int64_t)q0 * T + i] : 0.f;
      sCnt[2 * i] = 0;
      sCnt[2 * i + 1] = 0;
    }
    __syncthreads();  // every tile may be skipped: the counters are read below all the same
    for (int g0 = g_begin; g0 < g_end; g0 += TK_G) {
      uint64_t m0 = ~0ull, m1 = ~0ull;
      if (a.subset) {
        const u32x4 w = *(const u32x4*)(a.subset + (g0 >> 5));
        m0 = w[0] | (uint64_t)w[1] << 32;
        m1 = w[2] | (uint64_t)w[3] << 32;
        if (!(m0 | m1)) continue;  // block-uniform: nothing of this tile is counted
      }
      nm_tile<BF16, true>(a, smem, sS, sQw, q0, [=](int r) { return g0 + r < g_end ? g0 + r : -1; }, tid, wq, wg, l31, h);
      // wave w owns rows 16w .. 16w + 15 for the whole block, so its counters need no barrier
      const bool live0 = g0 + lane < g_end && ((m0 >> lane) & 1ull);
      const bool live1 = g0 + 64 + lane < g_end && ((m1 >> lane) & 1ull);
      for (int rr = 0; rr < TK_Q / 4; ++rr) {
        const int row = wave * (TK_Q / 4) + rr;
        if (row >= rows_live) break;
        const float s0 = sS[row * TK_SLD + lane], s1 = sS[row * TK_SLD + 64 + lane];
        const int mine = lane < T ? __float_as_int(sThr[row * T + lane]) : 0;
        int ng = 0, ne = 0;
        for (int t = 0; t < T; ++t) {
          const float thr = __int_as_float(__builtin_amdgcn_readlane(mine, t));
          const int cg = __popcll(__ballot(live0 && s0 > thr)) + __popcll(__ballot(live1 && s1 > thr));
          const int ce = __popcll(__ballot(live0 && s0 == thr)) + __popcll(__ballot(live1 && s1 == thr));
          if (lane == t) { ng = cg; ne = ce; }
        }
        if (lane < T) {
          sCnt[2 * (row * T + lane)] += ng;
          sCnt[2 * (row * T + lane) + 1] += ne;
        }
      }
    }
    for (int rr = 0; rr < TK_Q / 4; ++rr) {
      const int row = wave * (TK_Q / 4) + rr;
      if (row >= rows_live) break;
      if (lane < T) {
        int32_t* dst = a.cnt + (((int64_t)(q0 + row) * T + lane) * a.n_chunks + chunk) * 2;
        dst[0] = sCnt[2 * (row * T + lane)];
        dst[1] = sCnt[2 * (row * T + lane) + 1];
      }
    }
  }
}

// One thread per (query, target): the chunk counts summed in chunk order.
__global__ __launch_bounds__(256) void nm_reduce_kernel(const int32_t* __restrict__ cnt, int64_t n, int n_chunks,
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

namespace {
template <bool BF16>
constexpr size_t nm_base() { return (BF16 ? TKB_UNION_BYTES : TK_UNION_BYTES) + TK_QW_BYTES; }

bool nm_beta_ok(float beta) { return beta > 0.f && std::isfinite(beta); }

bool nm_shape_ok(int NQ, int NV, int M, int d, bool bf16) {
  return NQ > 0 && NV > 0 && M > 0 && M <= MMT_MAX_EXPERTS && d > 0 && !(d & (bf16 ? 7 : 3));
}

void nm_geometry(NmArgs& a) {
  a.chunk = tk_chunk(a.NQ, a.NV);
  a.n_qt = (a.NQ + TK_Q - 1) / TK_Q;
  a.n_chunks = (a.NV + a.chunk - 1) / a.chunk;
}

// Dynamic LDS limits above the 64 KiB default, raised once on every device the kernels are launched on (a function
// attribute belongs to the device that is current when it is set, and a gallery cut into shards launches on several).
template <bool BF16>
void nm_attrs() {
  static bool done[64] = {};
  int dev = -1;
  const bool known = hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 64;  // beyond the table: set every time
  if (known && done[dev]) return;
  constexpr size_t u = BF16 ? TKB_UNION_BYTES : TK_UNION_BYTES;
  (void)hipFuncSetAttribute((const void*)topk_norm_kernel<BF16>, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)(u + tk_state_lds(TK_MAXK) + tk_exclude_lds(TK_MAXE)));
  (void)hipFuncSetAttribute((const void*)rank_norm_kernel<BF16, false>, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)(nm_base<BF16>() + (size_t)TK_Q * NM_MAXT * 12));
  if (known) done[dev] = true;
}

template <bool BF16>
int nm_col_lse(NmArgs a, float* ws, float* state, int first, float* lse, hipStream_t s) {
  nm_geometry(a);
  hipLaunchKernelGGL(col_lse_kernel<BF16>, dim3(a.n_qt * a.n_chunks), dim3(256), nm_base<BF16>(), s, a, (float2*)ws);
  hipLaunchKernelGGL(col_lse_fold_kernel, dim3((a.NV + 255) / 256), dim3(256), 0, s, (const float2*)ws, a.n_qt, a.NV, state,
                     first, lse);
  return (int)hipGetLastError();
}

template <bool BF16>
int nm_topk(NmTopkArgs a, float* scores, int64_t* index, hipStream_t s) {
  nm_attrs<BF16>();
  nm_geometry(a);
  constexpr size_t u = BF16 ? TKB_UNION_BYTES : TK_UNION_BYTES;
  hipLaunchKernelGGL(topk_norm_kernel<BF16>, dim3(a.n_qt * a.n_chunks), dim3(256),
                     u + tk_state_lds(a.k) + tk_exclude_lds(a.E), s, a);
  return tk_merge_launch(a.ws, a.NQ, a.n_chunks, a.k, a.k < a.NV ? a.k : a.NV, scores, index, s);
}

template <bool BF16>
int nm_thresholds(NmRankArgs a, hipStream_t s) {
  nm_geometry(a);
  const int n_pt = (TK_Q * a.T + TK_G - 1) / TK_G;  // threshold tiles per query tile
  hipLaunchKernelGGL((rank_norm_kernel<BF16, true>), dim3(a.n_qt * n_pt), dim3(256), nm_base<BF16>() + TK_G * 4, s, a);
  return (int)hipGetLastError();
}

template <bool BF16>
int nm_count(NmRankArgs a, int32_t* greater, int32_t* equal, hipStream_t s) {
  nm_attrs<BF16>();
  nm_geometry(a);
  hipLaunchKernelGGL((rank_norm_kernel<BF16, false>), dim3(a.n_qt * a.n_chunks), dim3(256),
                     nm_base<BF16>() + (size_t)TK_Q * a.T * 12, s, a);
  const int64_t n = (int64_t)a.NQ * a.T;
  hipLaunchKernelGGL(nm_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a.cnt, n, a.n_chunks, greater,
                     equal);
  return (int)hipGetLastError();
}

void nm_fill(NmArgs& a, const void* q, const void* q_lo, const float* qw, const void* g, const float* gw, int NQ, int NV,
             int M, int d, float beta, const float* lse) {
  a.q = q; a.q_lo = q_lo; a.qw = qw; a.g = g; a.gw = gw; a.lse = lse; a.beta = beta;
  a.NQ = NQ; a.NV = NV; a.M = M; a.K = M * d;
}
}  // namespace

extern "C" int64_t mmt_col_lse_workspace_floats(int NB, int NV) {
  if (NB <= 0 || NV <= 0) return MMT_ERR_ARG;
  return 2 * (int64_t)((NB + TK_Q - 1) / TK_Q) * NV;
}

extern "C" int mmt_search_col_lse(const float* bf, const float* bw, const float* gf, const float* gw, int NB, int NV, int M,
                                  int d, float beta, float* ws, float* state, int first, float* lse, void* stream) {
  if (!bf || !bw || !gf || !gw || !ws || !state || !nm_shape_ok(NB, NV, M, d, false) || !nm_beta_ok(beta)) return MMT_ERR_ARG;
  if (((uintptr_t)bf | (uintptr_t)gf | (uintptr_t)ws) & 15) return MMT_ERR_ALIGN;
  NmArgs a = {};
  nm_fill(a, bf, nullptr, bw, gf, gw, NB, NV, M, d, beta, nullptr);
  return nm_col_lse<false>(a, ws, state, first, lse, (hipStream_t)stream);
}

extern "C" int mmt_search_col_lse_bf16(const uint16_t* b_hi, const uint16_t* b_lo, const float* bw, const uint16_t* gf,
                                       const float* gw, int NB, int NV, int M, int d, float beta, float* ws, float* state,
                                       int first, float* lse, void* stream) {
  if (!b_hi || !b_lo || !bw || !gf || !gw || !ws || !state || !nm_shape_ok(NB, NV, M, d, true) || !nm_beta_ok(beta))
    return MMT_ERR_ARG;
  if (((uintptr_t)b_hi | (uintptr_t)b_lo | (uintptr_t)gf | (uintptr_t)ws) & 15) return MMT_ERR_ALIGN;
  NmArgs a = {};
  nm_fill(a, b_hi, b_lo, bw, gf, gw, NB, NV, M, d, beta, nullptr);
  return nm_col_lse<true>(a, ws, state, first, lse, (hipStream_t)stream);
}

extern "C" int mmt_search_topk_norm(const float* qf, const float* qw, const float* gf, const float* gw, int NQ, int NV, int M,
                                    int d, int k, const uint32_t* subset, const int64_t* exclude, int E, float beta,
                                    const float* lse, uint64_t* ws, float* scores, int64_t* index, void* stream) {
  if (!qf || !qw || !gf || !gw || !lse || !ws || !index || !tk_args_ok(NQ, NV, k) || !nm_shape_ok(NQ, NV, M, d, false) ||
      !nm_beta_ok(beta))
    return MMT_ERR_ARG;
  if (((uintptr_t)qf | (uintptr_t)gf) & 15) return MMT_ERR_ALIGN;
  int rc;
  if (!tk_mask_args_ok(subset, exclude, E, &rc)) return rc;
  NmTopkArgs a = {};
  nm_fill(a, qf, nullptr, qw, gf, gw, NQ, NV, M, d, beta, lse);
  a.ws = ws; a.subset = subset; a.exclude = exclude; a.k = k; a.E = E;
  return nm_topk<false>(a, scores, index, (hipStream_t)stream);
}

extern "C" int mmt_search_topk_bf16_norm(const uint16_t* q_hi, const uint16_t* q_lo, const float* qw, const uint16_t* gf,
                                         const float* gw, int NQ, int NV, int M, int d, int k, const uint32_t* subset,
                                         const int64_t* exclude, int E, float beta, const float* lse, uint64_t* ws,
                                         float* scores, int64_t* index, void* stream) {
  if (!q_hi || !q_lo || !qw || !gf || !gw || !lse || !ws || !index || !tk_args_ok(NQ, NV, k) ||
      !nm_shape_ok(NQ, NV, M, d, true) || !nm_beta_ok(beta))
    return MMT_ERR_ARG;
  if (((uintptr_t)q_hi | (uintptr_t)q_lo | (uintptr_t)gf) & 15) return MMT_ERR_ALIGN;
  int rc;
  if (!tk_mask_args_ok(subset, exclude, E, &rc)) return rc;
  NmTopkArgs a = {};
  nm_fill(a, q_hi, q_lo, qw, gf, gw, NQ, NV, M, d, beta, lse);
  a.ws = ws; a.subset = subset; a.exclude = exclude; a.k = k; a.E = E;
  return nm_topk<true>(a, scores, index, (hipStream_t)stream);
}

extern "C" int mmt_search_thresholds_norm(const float* qf, const float* qw, const float* gf, const float* gw, int NQ, int NV,
                                          int M, int d, const int64_t* targets, int T, float beta, const float* lse,
                                          float* thr, void* stream) {
  if (!qf || !qw || !gf || !gw || !targets || !lse || !thr || T < 1 || T > NM_MAXT || !nm_shape_ok(NQ, NV, M, d, false) ||
      !nm_beta_ok(beta))
    return MMT_ERR_ARG;
  if (((uintptr_t)qf | (uintptr_t)gf) & 15) return MMT_ERR_ALIGN;
  NmRankArgs a = {};
  nm_fill(a, qf, nullptr, qw, gf, gw, NQ, NV, M, d, beta, lse);
  a.targets = targets; a.thr = thr; a.T = T;
  return nm_thresholds<false>(a, (hipStream_t)stream);
}

extern "C" int mmt_search_thresholds_bf16_norm(const uint16_t* q_hi, const uint16_t* q_lo, const float* qw,
                                               const uint16_t* gf, const float* gw, int NQ, int NV, int M, int d,
                                               const int64_t* targets, int T, float beta, const float* lse, float* thr,
                                               void* stream) {
  if (!q_hi || !q_lo || !qw || !gf || !gw || !targets || !lse || !thr || T < 1 || T > NM_MAXT ||
      !nm_shape_ok(NQ, NV, M, d, true) || !nm_beta_ok(beta))
    return MMT_ERR_ARG;
  if (((uintptr_t)q_hi | (uintptr_t)q_lo | (uintptr_t)gf) & 15) return MMT_ERR_ALIGN;
  NmRankArgs a = {};
  nm_fill(a, q_hi, q_lo, qw, gf, gw, NQ, NV, M, d, beta, lse);
  a.targets = targets; a.thr = thr; a.T = T;
  return nm_thresholds<true>(a, (hipStream_t)stream);
}

extern "C" int mmt_search_count_norm(const float* qf, const float* qw, const float* gf, const float* gw, int NQ, int NV,
                                     int M, int d, const float* thr, int T, const uint32_t* subset, float beta,
                                     const float* lse, int32_t* ws, int32_t* greater, int32_t* equal, void* stream) {
  if (!qf || !qw || !gf || !gw || !thr || !lse || !ws || !greater || !equal || T < 1 || T > NM_MAXT ||
      !nm_shape_ok(NQ, NV, M, d, false) || !nm_beta_ok(beta))
    return MMT_ERR_ARG;
  if (((uintptr_t)qf | (uintptr_t)gf | (uintptr_t)subset) & 15) return MMT_ERR_ALIGN;
  NmRankArgs a = {};
  nm_fill(a, qf, nullptr, qw, gf, gw, NQ, NV, M, d, beta, lse);
  a.thr = const_cast<float*>(thr); a.cnt = ws; a.subset = subset; a.T = T;
  return nm_count<false>(a, greater, equal, (hipStream_t)stream);
}

extern "C" int mmt_search_count_bf16_norm(const uint16_t* q_hi, const uint16_t* q_lo, const float* qw, const uint16_t* gf,
                                          const float* gw, int NQ, int NV, int M, int d, const float* thr, int T,
                                          const uint32_t* subset, float beta, const float* lse, int32_t* ws,
                                          int32_t* greater, int32_t* equal, void* stream) {
  if (!q_hi || !q_lo || !qw || !gf || !gw || !thr || !lse || !ws || !greater || !equal || T < 1 || T > NM_MAXT ||
      !nm_shape_ok(NQ, NV, M, d, true) || !nm_beta_ok(beta))
    return MMT_ERR_ARG;
  if (((uintptr_t)q_hi | (uintptr_t)q_lo | (uintptr_t)gf | (uintptr_t)subset) & 15) return MMT_ERR_ALIGN;
  NmRankArgs a = {};
  nm_fill(a, q_hi, q_lo, qw, gf, gw, NQ, NV, M, d, beta, lse);
  a.thr = const_cast<float*>(thr); a.cnt = ws; a.subset = subset; a.T = T;
  return nm_count<true>(a, greater, equal, (hipStream_t)stream);
}
