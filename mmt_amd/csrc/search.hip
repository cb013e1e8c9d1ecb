// Top-k retrieval without the N_query x N_gallery matrix (reference: utils/util.py:38-68 compress_predictions,
// trainer/trainer.py:411-437, utils/visualizer.py:74-92; similarity of model/model.py:789-837 in 'indep' mode).
//
//   score(q, g) = sum_m qw[q][m] gw[g][m] <Q_m[q], G_m[g]> / sum_m qw[q][m] gw[g][m]     (0 -> 1e-5)
//
// Both operands arrive folded (Q' = qw * Q, G' = gw * G: mmt_search_fold), so the numerator is ONE fp32 GEMM with
// K = M*d on v_mfma_f32_32x32x2_f32, like mmt_sims_eval.  Two launches:
//   topk_chunk_kernel<true>  : block = 64 queries x one gallery chunk.  Per 128-column tile the K loop streams
//                              through LDS in 32-wide slabs (register-staged: the next slab's global loads are in flight
//                              during the current slab's MFMAs), the epilogue divides by the gated denominator and the
//                              tile's 64 x 128 scores land in LDS, where each wave keeps a running top-k for its 16 rows
//                              (threshold = k-th best so far; candidates above it are appended, the list is compacted
//                              back to k when full).  The chunk's sorted k best go to the workspace.
//   topk_chunk_kernel<false> : the same selection stage reading the scores from a given matrix (compress_predictions).
//   topk_merge_kernel        : per query, the chunk lists merged by rank (each list is sorted: binary search).
// Order: score descending, ties by ascending gallery index (= a stable argsort of -score).  A (score, index) pair is one
// uint64 key -- order-preserving score bits above, ~index below -- so "better" is one unsigned compare and every key is
// distinct; 0 is "no candidate".  No atomics: every output slot has exactly one writer, results are bit-reproducible.
// The key and the running top-k live in search_topk.h, shared with the bf16-gallery kernel (search_bf16.hip); the K loop
// and the score epilogue in search_scan.h, shared with the rank-count kernels as well (search_rank.hip).
//
// topk_chunk_kernel<true, true> is the masked instantiation (mmt_search_topk_ex): the candidates are the items whose bit
// is set in a packed bitmap (search_subset.hip), less up to TK_MAXE items per query.  A tile's four mask words are one
// block-uniform 16-byte load (g0 is a multiple of 128); a tile with no bit set is skipped before its K loop -- no gallery
// loads, no MFMAs.  The mask acts at selection only (tk_tile_select<true>), on the score tile the unmasked kernel
// computes.  The unmasked instantiations compile to the code they had before the mask existed.
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
};

// The masked instantiation's arguments: a kernel argument of its own type, so the unmasked kernels keep their argument
// block (and with it their code) byte for byte.
struct TkMaskedArgs : TkArgs {
  const uint32_t* subset;   // bit g & 31 of word g >> 5 allows item g (nullable = all; 16-byte aligned)
  const int64_t* exclude;   // [NQ][E] items barred per query, -1 = none
  int E;
};

template <bool FUSED, bool MASKED = false>
__global__ __launch_bounds__(256) void topk_chunk_kernel(std::conditional_t<MASKED, TkMaskedArgs, TkArgs> a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int bid = xcd_remap(blockIdx.x, gridDim.x);  // gallery-chunk-major: an XCD's blocks share their chunk in L2
  const int chunk = bid / a.n_qt, q0 = (bid % a.n_qt) * TK_Q;
  const int g_begin = chunk * a.chunk, g_end = min(a.NV, g_begin + a.chunk);
  const int cap = a.k + 64;
  uint64_t* ws = a.ws + chunk * (int64_t)a.k;
  const int64_t ws_row = (int64_t)a.n_chunks * a.k;

  if constexpr (!FUSED) {
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
    return;
  } else {
    float* sS = (float*)smem;                                  // [TK_Q][TK_SLD]  scores (after the K loop: tk_scan_f32)
    float* sQw = (float*)(smem + TK_UNION_BYTES);              // [TK_Q][MMT_MAX_EXPERTS]
    int* sN = (int*)(smem + TK_UNION_BYTES + TK_QW_BYTES);     // [TK_Q] candidates held
    uint64_t* sT = (uint64_t*)(sN + TK_Q);                     // [TK_Q] thresholds
    uint64_t* sC = sT + TK_Q;                                  // [TK_Q][cap] candidates
    const int l31 = lane & 31, h = lane >> 5, wq = wave >> 1, wg = wave & 1;
    const int K = a.K, M = a.M;
    if (tid < TK_Q) { sN[tid] = 0; sT[tid] = 0; }
    tk_load_qw(sQw, a.qw, a.NQ, M, q0, tid);
    int* sEx = (int*)(sC + TK_Q * cap);                        // MASKED: [TK_Q][E] exclusions
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
      tk_scan_f32(acc, smem, a.q, a.g, a.NQ, K, q0, grow, tid, wq, wg, l31, h);
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

bool tk_args_ok(int NQ, int NV, int k) { return NQ > 0 && NV > 0 && k >= 1 && k <= TK_MAXK; }

size_t tk_state_lds(int k) { return TK_QW_BYTES + TK_Q * (4 + 8) + (size_t)TK_Q * (k + 64) * 8; }

size_t tk_exclude_lds(int E) { return (size_t)TK_Q * E * 4; }

bool tk_mask_args_ok(const uint32_t* subset, const int64_t* exclude, int E, int* rc) {
  if (E < 0 || E > TK_MAXE || (E > 0 && !exclude)) { *rc = MMT_ERR_ARG; return false; }
  if ((uintptr_t)subset & 15) { *rc = MMT_ERR_ALIGN; return false; }
  return true;
}

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
size_t tk_fused_lds(int k) { return TK_UNION_BYTES + tk_state_lds(k); }
size_t tk_select_lds(int k) { return (size_t)4 * (k + 64) * 8; }

int tk_launch(const TkMaskedArgs& a, bool fused, int kout, float* scores, int64_t* index, hipStream_t s) {
  static const bool attrs = [] {  // allow the k = 128 footprint (over the 64 KiB default)
    (void)hipFuncSetAttribute((const void*)topk_chunk_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                        (int)tk_fused_lds(TK_MAXK));
    (void)hipFuncSetAttribute((const void*)topk_chunk_kernel<true, true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)(tk_fused_lds(TK_MAXK) + tk_exclude_lds(TK_MAXE)));
    return true;
  }();
  (void)attrs;
  const int blocks = a.n_qt * a.n_chunks;
  if (fused && (a.subset || a.E))
    hipLaunchKernelGGL((topk_chunk_kernel<true, true>), dim3(blocks), dim3(256), tk_fused_lds(a.k) + tk_exclude_lds(a.E), s, a);
  else if (fused)
    hipLaunchKernelGGL(topk_chunk_kernel<true>, dim3(blocks), dim3(256), tk_fused_lds(a.k), s, (TkArgs)a);
  else
    hipLaunchKernelGGL(topk_chunk_kernel<false>, dim3(blocks), dim3(256), tk_select_lds(a.k), s, (TkArgs)a);
  return tk_merge_launch(a.ws, a.NQ, a.n_chunks, a.k, kout, scores, index, s);
}

TkMaskedArgs tk_args(int NQ, int NV, int k, uint64_t* ws) {
  TkMaskedArgs a = {};
  a.NQ = NQ; a.NV = NV; a.k = k; a.ws = ws;
  a.chunk = tk_chunk(NQ, NV);
  a.n_qt = (NQ + TK_Q - 1) / TK_Q;
  a.n_chunks = (NV + a.chunk - 1) / a.chunk;
  return a;
}
}  // namespace

extern "C" int64_t mmt_topk_workspace_keys(int NQ, int NV, int k) {
  if (!tk_args_ok(NQ, NV, k)) return MMT_ERR_ARG;
  const int chunk = tk_chunk(NQ, NV);
  return (int64_t)NQ * ((NV + chunk - 1) / chunk) * k;
}

extern "C" int mmt_search_topk_ex(const float* qf, const float* qw, const float* gf, const float* gw, int NQ, int NV, int M,
                                  int d, int k, const uint32_t* subset, const int64_t* exclude, int E, uint64_t* ws,
                                  float* scores, int64_t* index, void* stream) {
  if (!qf || !qw || !gf || !gw || !ws || !index || !tk_args_ok(NQ, NV, k) || M <= 0 || M > MMT_MAX_EXPERTS || d <= 0 ||
      (d & 3))
    return MMT_ERR_ARG;
  if (((uintptr_t)qf | (uintptr_t)gf) & 15) return MMT_ERR_ALIGN;
  int rc;
  if (!tk_mask_args_ok(subset, exclude, E, &rc)) return rc;
  TkMaskedArgs a = tk_args(NQ, NV, k, ws);
  a.q = qf; a.qw = qw; a.g = gf; a.gw = gw; a.M = M; a.K = M * d;
  a.subset = subset; a.exclude = exclude; a.E = E;
  return tk_launch(a, true, k < NV ? k : NV, scores, index, (hipStream_t)stream);
}

extern "C" int mmt_search_topk(const float* qf, const float* qw, const float* gf, const float* gw, int NQ, int NV, int M,
                               int d, int k, uint64_t* ws, float* scores, int64_t* index, void* stream) {
  return mmt_search_topk_ex(qf, qw, gf, gw, NQ, NV, M, d, k, nullptr, nullptr, 0, ws, scores, index, stream);
}

extern "C" int mmt_rows_topk(const float* sims, int64_t ld, const int32_t* rows, int NR, int NV, int k, uint64_t* ws,
                             float* scores, int64_t* index, void* stream) {
  if (!sims || !ws || !index || !tk_args_ok(NR, NV, k) || ld < NV) return MMT_ERR_ARG;
  TkMaskedArgs a = tk_args(NR, NV, k, ws);
  a.q = sims; a.ld = ld; a.rows = rows;
  return tk_launch(a, false, k < NV ? k : NV, scores, index, (hipStream_t)stream);
}
