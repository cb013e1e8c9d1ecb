// Top-k search over a gallery stored in bf16 (search.py: VideoIndex(dtype=torch.bfloat16)).
//
// Only the storage is lossy: the index keeps bf16_rne(gw (.) G) -- the fp32 fold of mmt_search_fold rounded once by a
// plain cast -- and the score is DEFINED on that stored value,
//
//   score(q, g) = < fold_fp32(Q, qw)[q], dequant(stored[g]) > / sum_m qw[q][m] gw[g][m]     (0 -> 1e-5)
//
// The fp32 query runs on the bf16 matrix cores as two terms, hi = bf16(qf) and lo = bf16(qf - hi): bf16 x bf16 products
// are exact in fp32, the accumulator is fp32, and what the split drops is below 2^-16 relative per query element.
//
//   fold_bf16_kernel<false> : x [N][M][d] fp32, w [N][M] -> bf16 [N][M*d], 8 elements (one 16-byte store) per thread
//   fold_bf16_kernel<true>  : the same fold written as the hi / lo pair (queries)
//   topk_chunk_bf16_kernel  : topk_chunk_kernel<true> of search.hip with the K loop on v_mfma_f32_32x32x16_bf16.  Same
//                             block (64 queries x one gallery chunk, 4 waves of 32 rows x 64 columns), same 128-column
//                             tile, same accumulator layout, hence the same epilogue, selection, workspace and merge
//                             (search_topk.h).  Per 64-wide K slab the block stages hi, lo (64 rows each) and the
//                             gallery (128 rows) in LDS; a wave reads each gallery fragment ONCE and feeds it to the hi
//                             and the lo MFMA.  A 64-query tile is below the bf16 ridge for a gallery streamed from
//                             HBM; the blocks of one gallery chunk are consecutive ids on one XCD (xcd_remap), so the
//                             chunk is fetched from HBM once per XCD and served to the other query tiles from L2.
//                             Rows past NQ / NV and the K tail are zero-filled in registers, never read.
//                             <true> is the masked instantiation (mmt_search_topk_bf16_ex): subset bitmap, tile skip
//                             and per-query exclusions exactly as topk_chunk_kernel<true, true> of search.hip.
#include <type_traits>

#include "search_topk.h"

struct TkBf16Args {
  const bf16_t* q_hi;   // [NQ][K]
  const bf16_t* q_lo;   // [NQ][K]
  const float* qw;      // [NQ][M]
  const bf16_t* g;      // [NV][K]
  const float* gw;      // [NV][M]
  uint64_t* ws;         // [NQ][n_chunks][k]
  int NQ, NV, M, K, k, chunk, n_qt, n_chunks;
};

struct TkBf16MaskedArgs : TkBf16Args {  // as TkMaskedArgs of search.hip
  const uint32_t* subset;   // bit g & 31 of word g >> 5 allows item g (nullable = all; 16-byte aligned)
  const int64_t* exclude;   // [NQ][E] items barred per query, -1 = none
  int E;
};

// out[r][m*d + c] = bf16(w[r][m] * x[r][m][c]); SPLIT: hi = bf16(v), lo = bf16(v - hi).  i8 counts groups of 8 elements,
// which never straddle an (r, m) row because d % 8 == 0.
template <bool SPLIT>
__global__ __launch_bounds__(256) void fold_bf16_kernel(const float* __restrict__ x, const float* __restrict__ w, int64_t n8,
                                                        int d, bf16_t* __restrict__ hi, bf16_t* __restrict__ lo) {
  const int d8 = d >> 3;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n8; i += (int64_t)gridDim.x * blockDim.x) {
    const float wv = w[i / d8];  // r*M + m
    const f32x4 v0 = ((const f32x4*)x)[2 * i] * wv, v1 = ((const f32x4*)x)[2 * i + 1] * wv;
    u16x8 h, l;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      h[j] = f2bf(v0[j]);
      h[4 + j] = f2bf(v1[j]);
      if constexpr (SPLIT) {
        l[j] = f2bf(v0[j] - bf2f(h[j]));
        l[4 + j] = f2bf(v1[j] - bf2f(h[4 + j]));
      }
    }
    ((u16x8*)hi)[i] = h;
    if constexpr (SPLIT) ((u16x8*)lo)[i] = l;
  }
}

template <bool MASKED>
__global__ __launch_bounds__(256) void topk_chunk_bf16_kernel(std::conditional_t<MASKED, TkBf16MaskedArgs, TkBf16Args> a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int bid = xcd_remap(blockIdx.x, gridDim.x);  // gallery-chunk-major: an XCD's blocks share their chunk in L2
  const int chunk = bid / a.n_qt, q0 = (bid % a.n_qt) * TK_Q;
  const int g_begin = chunk * a.chunk, g_end = min(a.NV, g_begin + a.chunk);
  const int cap = a.k + 64;
  uint64_t* ws = a.ws + chunk * (int64_t)a.k;
  const int64_t ws_row = (int64_t)a.n_chunks * a.k;

  float* sS = (float*)smem;                                   // [TK_Q][TK_SLD]  scores (after the K loop: tk_scan_bf16)
  float* sQw = (float*)(smem + TKB_UNION_BYTES);              // [TK_Q][MMT_MAX_EXPERTS]
  int* sN = (int*)(smem + TKB_UNION_BYTES + TK_QW_BYTES);     // [TK_Q] candidates held
  uint64_t* sT = (uint64_t*)(sN + TK_Q);                      // [TK_Q] thresholds
  uint64_t* sC = sT + TK_Q;                                   // [TK_Q][cap] candidates
  const int l31 = lane & 31, h = lane >> 5, wq = wave >> 1, wg = wave & 1;
  const int K = a.K, M = a.M;
  if (tid < TK_Q) { sN[tid] = 0; sT[tid] = 0; }
  tk_load_qw(sQw, a.qw, a.NQ, M, q0, tid);
  int* sEx = (int*)(sC + TK_Q * cap);                         // MASKED: [TK_Q][E] exclusions
  if constexpr (MASKED)
    for (int i = tid; i < TK_Q * a.E; i += 256) sEx[i] = q0 + i / a.E < a.NQ ? (int)a.exclude[(int64_t)q0 * a.E + i] : -1;
  for (int g0 = g_begin; g0 < g_end; g0 += TK_G) {
    uint64_t m0 = ~0ull, m1 = ~0ull;
    if constexpr (MASKED) {
      if (a.subset) {
        const u32x4 w = *(const u32x4*)(a.subset + (g0 >> 5));
        m0 = w[0] | (uint64_t)w[1] << 32;
        m1 = w[2] | (uint64_t)w[3] << 32;
        if (!(m0 | m1)) continue;  // block-uniform: nothing of this tile is allowed
      }
    }
    const auto grow = [=](int r) { return g0 + r < g_end ? g0 + r : -1; };
    f32x16 acc[2];
    tk_scan_bf16(acc, smem, a.q_hi, a.q_lo, a.g, a.NQ, K, q0, grow, tid, wq, wg, l31, h);
    __syncthreads();  // the slabs become the score tile
    tk_tile_scores(acc, sS, sQw, a.gw, M, grow, wq, wg, l31, h);
    __syncthreads();
    if constexpr (MASKED)
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

namespace {
size_t tkb_lds(int k) { return TKB_UNION_BYTES + tk_state_lds(k); }

bool fold_args_ok(const void* x, const void* w, int N, int M, int d) {
  return x && w && N > 0 && M > 0 && M <= MMT_MAX_EXPERTS && d > 0 && !(d & 7);
}

int fold_blocks(int64_t n8) { return (int)((n8 + 255) / 256 < 4096 ? (n8 + 255) / 256 : 4096); }
}  // namespace

extern "C" int mmt_search_fold_bf16(const float* x, const float* w, int N, int M, int d, uint16_t* out, void* stream) {
  if (!fold_args_ok(x, w, N, M, d) || !out) return MMT_ERR_ARG;
  if (((uintptr_t)x | (uintptr_t)out) & 15) return MMT_ERR_ALIGN;
  const int64_t n8 = (int64_t)N * M * d / 8;
  hipLaunchKernelGGL(fold_bf16_kernel<false>, dim3(fold_blocks(n8)), dim3(256), 0, (hipStream_t)stream, x, w, n8, d, out,
                     (bf16_t*)nullptr);
  return (int)hipGetLastError();
}

extern "C" int mmt_search_fold_split_bf16(const float* x, const float* w, int N, int M, int d, uint16_t* hi, uint16_t* lo,
                                          void* stream) {
  if (!fold_args_ok(x, w, N, M, d) || !hi || !lo) return MMT_ERR_ARG;
  if (((uintptr_t)x | (uintptr_t)hi | (uintptr_t)lo) & 15) return MMT_ERR_ALIGN;
  const int64_t n8 = (int64_t)N * M * d / 8;
  hipLaunchKernelGGL(fold_bf16_kernel<true>, dim3(fold_blocks(n8)), dim3(256), 0, (hipStream_t)stream, x, w, n8, d, hi, lo);
  return (int)hipGetLastError();
}

extern "C" int mmt_search_topk_bf16_ex(const uint16_t* q_hi, const uint16_t* q_lo, const float* qw, const uint16_t* gf,
                                       const float* gw, int NQ, int NV, int M, int d, int k, const uint32_t* subset,
                                       const int64_t* exclude, int E, uint64_t* ws, float* scores, int64_t* index,
                                       void* stream) {
  if (!q_hi || !q_lo || !qw || !gf || !gw || !ws || !index || !tk_args_ok(NQ, NV, k) || M <= 0 || M > MMT_MAX_EXPERTS ||
      d <= 0 || (d & 7))
    return MMT_ERR_ARG;
  if (((uintptr_t)q_hi | (uintptr_t)q_lo | (uintptr_t)gf) & 15) return MMT_ERR_ALIGN;
  int rc;
  if (!tk_mask_args_ok(subset, exclude, E, &rc)) return rc;
  static const bool attrs = [] {  // allow the k = 128 footprint (over the 64 KiB default)
    (void)hipFuncSetAttribute((const void*)topk_chunk_bf16_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)tkb_lds(TK_MAXK));
    (void)hipFuncSetAttribute((const void*)topk_chunk_bf16_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)(tkb_lds(TK_MAXK) + tk_exclude_lds(TK_MAXE)));
    return true;
  }();
  (void)attrs;
  TkBf16MaskedArgs a = {};
  a.q_hi = q_hi; a.q_lo = q_lo; a.qw = qw; a.g = gf; a.gw = gw; a.ws = ws;
  a.NQ = NQ; a.NV = NV; a.M = M; a.K = M * d; a.k = k;
  a.subset = subset; a.exclude = exclude; a.E = E;
  a.chunk = tk_chunk(NQ, NV);
  a.n_qt = (NQ + TK_Q - 1) / TK_Q;
  a.n_chunks = (NV + a.chunk - 1) / a.chunk;
  hipStream_t s = (hipStream_t)stream;
  if (subset || E)
    hipLaunchKernelGGL(topk_chunk_bf16_kernel<true>, dim3(a.n_qt * a.n_chunks), dim3(256), tkb_lds(k) + tk_exclude_lds(E), s,
                       a);
  else
    hipLaunchKernelGGL(topk_chunk_bf16_kernel<false>, dim3(a.n_qt * a.n_chunks), dim3(256), tkb_lds(k), s, (TkBf16Args)a);
  return tk_merge_launch(ws, NQ, a.n_chunks, k, k < NV ? k : NV, scores, index, s);
}

extern "C" int mmt_search_topk_bf16(const uint16_t* q_hi, const uint16_t* q_lo, const float* qw, const uint16_t* gf,
                                    const float* gw, int NQ, int NV, int M, int d, int k, uint64_t* ws, float* scores,
                                    int64_t* index, void* stream) {
  return mmt_search_topk_bf16_ex(q_hi, q_lo, qw, gf, gw, NQ, NV, M, d, k, nullptr, nullptr, 0, ws, scores, index, stream);
}
