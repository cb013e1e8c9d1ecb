// Exact retrieval ranks without the N_query x N_gallery matrix (reference: model/metric.py:90-121 t2v_metrics,
// 153-243 v2t_metrics -- the tie-averaged rank of the ground truth in a row of sims).
//
// For a query q and a target item t the rank is  #{g : score(q, g) > score(q, t)} + (#{g : score(q, g) == score(q, t)} - 1) / 2.
// The two counts come from the scan the top-k search does (search_scan.h: same tile, same gated denominator, same chunk
// rule) with a counter per (query, target) in place of a running top-k list.  Three launches, T <= 32 targets per query:
//   rank_kernel<BF16, true>   : thresholds.  thr[q][t] = score(q, targets[q][t]) from the SAME scoring tile with a
//                               gallery-row indirection: block = 64 queries x 128 (query, target) pairs, tile column c of
//                               block (qt, j) holds the gallery row of pair p = 128 j + c, i.e. of query p / T, target
//                               p % T; only the entry on that query's own row is kept.  The K order of an MFMA output
//                               element does not depend on its column, the denominator is the same code on the same
//                               operands, so an item compares equal to itself in the count pass (checked by the tests
//                               against search(k = 128), which returns the scan's own scores).  A target outside 0 .. NV - 1
//                               (-1 = none) is never dereferenced; its threshold is NaN, which counts nothing.
//   rank_kernel<BF16, false>  : counts.  Block = 64 queries x one gallery chunk, as the top-k kernel.  Per 64 x 128 score
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
// rank_kernel<BF16, false, true> is the masked count pass (mmt_search_rank_ex): only items whose bit is set in a packed
// bitmap (search_subset.hip) are counted -- the live-column predicate ANDed with the tile's 128 bits, one block-uniform
// 16-byte load per tile, and a tile without a set bit skipped before its K loop.  Thresholds and the reduce are the
// unmasked ones, so a target outside the subset is still scored; it just does not count itself.
//
// mmt_search_thresholds / mmt_search_count (and their bf16 forms) launch the threshold pass alone and the count pass +
// reduce against given thresholds: the same instantiations with the same argument blocks.  A gallery cut into shards
// scores a target where it is stored and counts it on every shard (search.py: ShardedVideoIndex); the int32 counts add.
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
};

// The masked count pass takes an argument type of its own, so the unmasked kernels keep their argument block (and with
// it their code) byte for byte.
struct RkMaskedArgs : RkArgs {
  const uint32_t* subset;  // bit g & 31 of word g >> 5 allows item g (16-byte aligned)
};

template <bool BF16, class GRow>
__device__ __forceinline__ void rk_tile(const RkArgs& a, unsigned char* smem, float* sS, const float* sQw, int q0, GRow grow,
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
}

template <bool BF16, bool THR, bool MASKED = false>
__global__ __launch_bounds__(256) void rank_kernel(std::conditional_t<MASKED, RkMaskedArgs, RkArgs> a) {
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
    rk_tile<BF16>(a, smem, sS, sQw, q0, [=](int r) { return sRow[r]; }, tid, wq, wg, l31, h);
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
    if constexpr (MASKED) __syncthreads();  // every tile may be skipped: the counters are read below all the same
    for (int g0 = g_begin; g0 < g_end; g0 += TK_G) {
      uint64_t m0 = ~0ull, m1 = ~0ull;
      if constexpr (MASKED) {
        const u32x4 w = *(const u32x4*)(a.subset + (g0 >> 5));
        m0 = w[0] | (uint64_t)w[1] << 32;
        m1 = w[2] | (uint64_t)w[3] << 32;
        if (!(m0 | m1)) continue;  // block-uniform: nothing of this tile is counted
      }
      rk_tile<BF16>(a, smem, sS, sQw, q0, [=](int r) { return g0 + r < g_end ? g0 + r : -1; }, tid, wq, wg, l31, h);
      // wave w owns rows 16w .. 16w + 15 for the whole block, so its counters need no barrier
      const bool live0 = g0 + lane < g_end && (!MASKED || ((m0 >> lane) & 1ull));
      const bool live1 = g0 + 64 + lane < g_end && (!MASKED || ((m1 >> lane) & 1ull));
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

namespace {
bool rk_args_ok(int NQ, int NV, int T) { return NQ > 0 && NV > 0 && T >= 1 && T <= RK_MAXT; }

int rk_chunks(int NQ, int NV) {
  const int chunk = tk_chunk(NQ, NV);
  return (NV + chunk - 1) / chunk;
}

// The count kernels' dynamic LDS limit, raised once on every device they are launched on (the T = 32 footprint of the bf16
// kernel is exactly the 64 KiB default limit).  A function attribute belongs to the device that is current when it is set,
// and a gallery cut into shards launches these kernels on several.  Two threads meeting here set the same value twice.
template <bool BF16>
void rk_count_attrs() {
  constexpr size_t base = (BF16 ? TKB_UNION_BYTES : TK_UNION_BYTES) + TK_QW_BYTES;
  static bool done[64] = {};
  int dev = -1;
  const bool known = hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 64;  // beyond the table: set every time
  if (known && done[dev]) return;
  (void)hipFuncSetAttribute((const void*)rank_kernel<BF16, false>, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)(base + (size_t)TK_Q * RK_MAXT * 12));
  (void)hipFuncSetAttribute((const void*)rank_kernel<BF16, false, true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)(base + (size_t)TK_Q * RK_MAXT * 12));
  if (known) done[dev] = true;
}

// workspace (int32 units): thresholds [NQ][T] fp32, then (greater, equal) [NQ][T][n_chunks][2]
template <bool BF16>
int rk_launch(RkMaskedArgs a, int32_t* ws, int32_t* greater, int32_t* equal, hipStream_t s) {
  constexpr size_t base = (BF16 ? TKB_UNION_BYTES : TK_UNION_BYTES) + TK_QW_BYTES;
  rk_count_attrs<BF16>();
  a.chunk = tk_chunk(a.NQ, a.NV);
  a.n_qt = (a.NQ + TK_Q - 1) / TK_Q;
  a.n_chunks = (a.NV + a.chunk - 1) / a.chunk;
  a.thr = (float*)ws;
  a.cnt = ws + (int64_t)a.NQ * a.T;
  const int n_pt = (TK_Q * a.T + TK_G - 1) / TK_G;  // threshold tiles per query tile
  hipLaunchKernelGGL((rank_kernel<BF16, true>), dim3(a.n_qt * n_pt), dim3(256), base + TK_G * 4, s, (RkArgs)a);
  if (a.subset)
    hipLaunchKernelGGL((rank_kernel<BF16, false, true>), dim3(a.n_qt * a.n_chunks), dim3(256),
                       base + (size_t)TK_Q * a.T * 12, s, a);
  else
    hipLaunchKernelGGL((rank_kernel<BF16, false>), dim3(a.n_qt * a.n_chunks), dim3(256), base + (size_t)TK_Q * a.T * 12, s,
                       (RkArgs)a);
  const int64_t n = (int64_t)a.NQ * a.T;
  hipLaunchKernelGGL(rank_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a.cnt, n, a.n_chunks, greater,
                     equal);
  return (int)hipGetLastError();
}

// The two halves of rk_launch on their own (a gallery cut into shards scores a target on the shard that holds it and
// counts it on every shard: search.py, ShardedVideoIndex): the same kernels, launched as above.
template <bool BF16>
int rk_launch_thresholds(RkMaskedArgs a, float* thr, hipStream_t s) {
  constexpr size_t base = (BF16 ? TKB_UNION_BYTES : TK_UNION_BYTES) + TK_QW_BYTES;
  a.chunk = tk_chunk(a.NQ, a.NV);
  a.n_qt = (a.NQ + TK_Q - 1) / TK_Q;
  a.n_chunks = (a.NV + a.chunk - 1) / a.chunk;
  a.thr = thr;
  const int n_pt = (TK_Q * a.T + TK_G - 1) / TK_G;
  hipLaunchKernelGGL((rank_kernel<BF16, true>), dim3(a.n_qt * n_pt), dim3(256), base + TK_G * 4, s, (RkArgs)a);
  return (int)hipGetLastError();
}

// workspace (int32 units): (greater, equal) [NQ][T][n_chunks][2]; a.thr is the caller's
template <bool BF16>
int rk_launch_count(RkMaskedArgs a, int32_t* ws, int32_t* greater, int32_t* equal, hipStream_t s) {
  constexpr size_t base = (BF16 ? TKB_UNION_BYTES : TK_UNION_BYTES) + TK_QW_BYTES;
  rk_count_attrs<BF16>();
  a.chunk = tk_chunk(a.NQ, a.NV);
  a.n_qt = (a.NQ + TK_Q - 1) / TK_Q;
  a.n_chunks = (a.NV + a.chunk - 1) / a.chunk;
  a.cnt = ws;
  if (a.subset)
    hipLaunchKernelGGL((rank_kernel<BF16, false, true>), dim3(a.n_qt * a.n_chunks), dim3(256),
                       base + (size_t)TK_Q * a.T * 12, s, a);
  else
    hipLaunchKernelGGL((rank_kernel<BF16, false>), dim3(a.n_qt * a.n_chunks), dim3(256), base + (size_t)TK_Q * a.T * 12, s,
                       (RkArgs)a);
  const int64_t n = (int64_t)a.NQ * a.T;
  hipLaunchKernelGGL(rank_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a.cnt, n, a.n_chunks, greater,
                     equal);
  return (int)hipGetLastError();
}
}  // namespace

extern "C" int64_t mmt_rank_workspace_ints(int NQ, int NV, int T) {
  if (!rk_args_ok(NQ, NV, T)) return MMT_ERR_ARG;
  return (int64_t)NQ * T * (1 + 2 * (int64_t)rk_chunks(NQ, NV));
}

extern "C" int mmt_search_rank_ex(const float* qf, const float* qw, const float* gf, const float* gw, int NQ, int NV, int M,
                                  int d, const int64_t* targets, int T, const uint32_t* subset, int32_t* ws,
                                  int32_t* greater, int32_t* equal, void* stream) {
  if (!qf || !qw || !gf || !gw || !targets || !ws || !greater || !equal || !rk_args_ok(NQ, NV, T) || M <= 0 ||
      M > MMT_MAX_EXPERTS || d <= 0 || (d & 3))
    return MMT_ERR_ARG;
  if (((uintptr_t)qf | (uintptr_t)gf | (uintptr_t)subset) & 15) return MMT_ERR_ALIGN;
  RkMaskedArgs a = {};
  a.q = qf; a.qw = qw; a.g = gf; a.gw = gw; a.targets = targets; a.subset = subset;
  a.NQ = NQ; a.NV = NV; a.M = M; a.K = M * d; a.T = T;
  return rk_launch<false>(a, ws, greater, equal, (hipStream_t)stream);
}

extern "C" int mmt_search_rank(const float* qf, const float* qw, const float* gf, const float* gw, int NQ, int NV, int M,
                               int d, const int64_t* targets, int T, int32_t* ws, int32_t* greater, int32_t* equal,
                               void* stream) {
  return mmt_search_rank_ex(qf, qw, gf, gw, NQ, NV, M, d, targets, T, nullptr, ws, greater, equal, stream);
}

extern "C" int mmt_search_rank_bf16_ex(const uint16_t* q_hi, const uint16_t* q_lo, const float* qw, const uint16_t* gf,
                                       const float* gw, int NQ, int NV, int M, int d, const int64_t* targets, int T,
                                       const uint32_t* subset, int32_t* ws, int32_t* greater, int32_t* equal,
                                       void* stream) {
  if (!q_hi || !q_lo || !qw || !gf || !gw || !targets || !ws || !greater || !equal || !rk_args_ok(NQ, NV, T) || M <= 0 ||
      M > MMT_MAX_EXPERTS || d <= 0 || (d & 7))
    return MMT_ERR_ARG;
  if (((uintptr_t)q_hi | (uintptr_t)q_lo | (uintptr_t)gf | (uintptr_t)subset) & 15) return MMT_ERR_ALIGN;
  RkMaskedArgs a = {};
  a.q = q_hi; a.q_lo = q_lo; a.qw = qw; a.g = gf; a.gw = gw; a.targets = targets; a.subset = subset;
  a.NQ = NQ; a.NV = NV; a.M = M; a.K = M * d; a.T = T;
  return rk_launch<true>(a, ws, greater, equal, (hipStream_t)stream);
}

extern "C" int mmt_search_rank_bf16(const uint16_t* q_hi, const uint16_t* q_lo, const float* qw, const uint16_t* gf,
                                    const float* gw, int NQ, int NV, int M, int d, const int64_t* targets, int T,
                                    int32_t* ws, int32_t* greater, int32_t* equal, void* stream) {
  return mmt_search_rank_bf16_ex(q_hi, q_lo, qw, gf, gw, NQ, NV, M, d, targets, T, nullptr, ws, greater, equal, stream);
}

extern "C" int64_t mmt_count_workspace_ints(int NQ, int NV, int T) {
  if (!rk_args_ok(NQ, NV, T)) return MMT_ERR_ARG;
  return (int64_t)NQ * T * 2 * (int64_t)rk_chunks(NQ, NV);
}

extern "C" int mmt_search_thresholds(const float* qf, const float* qw, const float* gf, const float* gw, int NQ, int NV,
                                     int M, int d, const int64_t* targets, int T, float* thr, void* stream) {
  if (!qf || !qw || !gf || !gw || !targets || !thr || !rk_args_ok(NQ, NV, T) || M <= 0 || M > MMT_MAX_EXPERTS || d <= 0 ||
      (d & 3))
    return MMT_ERR_ARG;
  if (((uintptr_t)qf | (uintptr_t)gf) & 15) return MMT_ERR_ALIGN;
  RkMaskedArgs a = {};
  a.q = qf; a.qw = qw; a.g = gf; a.gw = gw; a.targets = targets;
  a.NQ = NQ; a.NV = NV; a.M = M; a.K = M * d; a.T = T;
  return rk_launch_thresholds<false>(a, thr, (hipStream_t)stream);
}

extern "C" int mmt_search_thresholds_bf16(const uint16_t* q_hi, const uint16_t* q_lo, const float* qw, const uint16_t* gf,
                                          const float* gw, int NQ, int NV, int M, int d, const int64_t* targets, int T,
                                          float* thr, void* stream) {
  if (!q_hi || !q_lo || !qw || !gf || !gw || !targets || !thr || !rk_args_ok(NQ, NV, T) || M <= 0 ||
      M > MMT_MAX_EXPERTS || d <= 0 || (d & 7))
    return MMT_ERR_ARG;
  if (((uintptr_t)q_hi | (uintptr_t)q_lo | (uintptr_t)gf) & 15) return MMT_ERR_ALIGN;
  RkMaskedArgs a = {};
  a.q = q_hi; a.q_lo = q_lo; a.qw = qw; a.g = gf; a.gw = gw; a.targets = targets;
  a.NQ = NQ; a.NV = NV; a.M = M; a.K = M * d; a.T = T;
  return rk_launch_thresholds<true>(a, thr, (hipStream_t)stream);
}

extern "C" int mmt_search_count(const float* qf, const float* qw, const float* gf, const float* gw, int NQ, int NV, int M,
                                int d, const float* thr, int T, const uint32_t* subset, int32_t* ws, int32_t* greater,
                                int32_t* equal, void* stream) {
  if (!qf || !qw || !gf || !gw || !thr || !ws || !greater || !equal || !rk_args_ok(NQ, NV, T) || M <= 0 ||
      M > MMT_MAX_EXPERTS || d <= 0 || (d & 3))
    return MMT_ERR_ARG;
  if (((uintptr_t)qf | (uintptr_t)gf | (uintptr_t)subset) & 15) return MMT_ERR_ALIGN;
  RkMaskedArgs a = {};
  a.q = qf; a.qw = qw; a.g = gf; a.gw = gw; a.thr = const_cast<float*>(thr); a.subset = subset;
  a.NQ = NQ; a.NV = NV; a.M = M; a.K = M * d; a.T = T;
  return rk_launch_count<false>(a, ws, greater, equal, (hipStream_t)stream);
}

extern "C" int mmt_search_count_bf16(const uint16_t* q_hi, const uint16_t* q_lo, const float* qw, const uint16_t* gf,
                                     const float* gw, int NQ, int NV, int M, int d, const float* thr, int T,
                                     const uint32_t* subset, int32_t* ws, int32_t* greater, int32_t* equal, void* stream) {
  if (!q_hi || !q_lo || !qw || !gf || !gw || !thr || !ws || !greater || !equal || !rk_args_ok(NQ, NV, T) || M <= 0 ||
      M > MMT_MAX_EXPERTS || d <= 0 || (d & 7))
    return MMT_ERR_ARG;
  if (((uintptr_t)q_hi | (uintptr_t)q_lo | (uintptr_t)gf | (uintptr_t)subset) & 15) return MMT_ERR_ALIGN;
  RkMaskedArgs a = {};
  a.q = q_hi; a.q_lo = q_lo; a.qw = qw; a.g = gf; a.gw = gw; a.thr = const_cast<float*>(thr); a.subset = subset;
  a.NQ = NQ; a.NV = NV; a.M = M; a.K = M * d; a.T = T;
  return rk_launch_count<true>(a, ws, greater, equal, (hipStream_t)stream);
}
