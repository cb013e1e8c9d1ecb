// The streaming schedule of the plain top-k scan (mmt_search_topk_stream): the search of a handful of queries, where the
// gallery is read once and every byte of it is the cost.  Same answer as topk_scan_kernel (search.hip), bit for bit:
//
//   * a (query, item) accumulator goes through tk_step's instruction sequence -- bf16 / fp8: K ascending in steps of 16,
//     lane half h feeding k = kk + 8h .. + 7, one v_mfma_f32_32x32x16_bf16 per query plane, hi then lo; fp32: K ascending in
//     steps of 8, four v_mfma_f32_32x32x2_f32 u = 0 .. 3 with k = kk + 4h + u -- from zero, in fp32.  An MFMA output depends
//     on its A row, its B column and its accumulator only, so the tiling, the staging and the geometry are free;
//   * a step past K multiplies zeros on both sides (the tile kernel's zero fill): the accumulator keeps its value, -0
//     becoming +0 at most, which the key (tk_key) does anyway;
//   * the epilogue is tk_tile_scores' expression: the same `den += qw[m] * gw[m]` chain over m ascending, 0 -> 1e-5, with an
//     fp8 gallery tk_mul_rn(acc, scale) first, then num / den;
//   * selection and workspace are the tile schedule's (tk_key, tk_push, tk_compact, tk_flush): keys are distinct and their
//     order is total, so neither the order in which candidates are offered nor the number of chunk lists can change a
//     result.  The merge is by rank as well, a rank is unique (topk_stream_merge_kernel).  No atomics; one writer per slot.
//
// What differs is the organisation, around gallery bytes in flight and not around tile reuse (the tile kernel's block
// shares a 128-item slab among 64 query rows through LDS, single-buffered, two barriers per slab):
//   block  = 32 query rows (ONE MFMA row block) x one gallery chunk, 4 waves.  A sweep covers 512 items: wave w owns items
//            G0 + 128 w .. + 127 as T = 4 accumulators of 32 x 32, so every A fragment is used four times.
//   gallery: never in LDS.  A B fragment is exactly one 16-byte load by the lane that consumes it (row g0 + 32 t + l31,
//            element kk + 8h of a bf16 row, kk + 4h of an fp32 row), held in registers ONE WHOLE SLAB ahead: the 16 loads of
//            slab s + 1 are issued into the registers of slab s as the MFMAs free them, 16 KiB per wave always in flight.
//            An fp8 row: one 16-byte load covers two steps of the two lane halves (bytes 32 jj + 16 h ..), and
//            v_permlane32_swap hands each half the 8 codes of its step; the codes are widened exactly (tk_widen_fp8's
//            arithmetic) in registers.  A row past the chunk's end is the last row of the gallery again: its column is
//            never a candidate, and no load is predicated but those of a last, partial slab.
//   queries: the block's 32 rows (fp32, or the bf16 hi / lo pair) go through LDS slab by slab, double-buffered, ONE
//            barrier per slab; register loads survive a __syncthreads(), so the gallery stream is not drained there.
//   scores : after a K sweep the waves take turns: a wave's 32 x 128 scores land in the one score tile [32][TK_SLD], and
//            the block's 32 rows, 8 per wave, are offered to the running top-k (tk_push) -- per-wave lists of 32 rows do
//            not fit at k = 128.  Subset, exclusions and cursor act here and only here, as in tk_tile_select.
//   subset : a 128-item tile without an allowed item is skipped before its loads (its wave idles through the sweep's
//            barriers); a sweep without one is skipped whole.
// The chunk rule (st_geometry) is a pure function of (NQ, NV), monotone in NV.
#include <type_traits>

#include "search_topk.h"

#define ST_Q 32                   // query rows per block
#define ST_T 4                    // 32-column accumulators per wave
#define ST_G (4 * TK_G)           // gallery columns per sweep: a 128-column tile per wave
#define ST_MAX_TILES 8            // sweeps per block at most
#define ST_TILE_BYTES (ST_Q * TK_SLD * 4)
#define ST_QW_BYTES (ST_Q * MMT_MAX_EXPERTS * 4)

struct StArgs {
  const void* q;            // fp32: Q' [NQ][K]; bf16 / fp8: hi(Q')
  const void* q_lo;         // bf16 / fp8: lo(Q')
  const float* qw;          // [NQ][M]
  const void* g;            // [NV][K] fp32, bf16 bits or e4m3fn codes
  const float* gw;          // [NV][M]
  const float* gscale;      // fp8: [NV]
  uint64_t* ws;             // [NQ][n_chunks][k]
  const uint32_t* subset;   // masked: nullable = all
  const int64_t* exclude;   // masked: [NQ][E]
  const uint64_t* after;    // paged: [NQ]
  int NQ, NV, M, K, k, E, tiles, n_qt, n_chunks;
};

// The filtered search on this schedule (mmt_search_topk_stream_where): StArgs with a tag word per item and three masks per
// query row behind it (search_scan.h: tk_tag_pass), in a type of its own, so the kernels above keep their argument block.
// One instantiation per storage, masked and paged: subset, exclude and after may each be absent (a null `after` gives
// every live row the bound 2^64 - 1).  The filter acts in the selection; it skips no sweep.
struct StWhereArgs : StArgs {
  const uint64_t* tags;     // [NV]
  const uint64_t* where;    // [NQ][3]: all_of, none_of, any_of
  static constexpr bool kWhere = true;
};

// What a gallery stored as TG (float, bf16_t = bf16 bits, uint8_t = e4m3fn codes) means for the loop.
template <class TG>
struct StKind {
  static constexpr bool F32 = std::is_same_v<TG, float>, FP8 = std::is_same_v<TG, uint8_t>;
  using TQ = std::conditional_t<F32, float, bf16_t>;   // a query plane
  static constexpr int P = F32 ? 1 : 2;                 // query planes
  using TS = TkStager<TQ, ST_Q, P>;                     // the tile kernel's slabs: width, pitch, one load per thread
  static constexpr int BK = TS::BK, KK = TS::KK, LD = TS::LD;
  using V = std::conditional_t<F32, f32x4, u32x4>;     // one gallery load of a lane
  static constexpr int EL = 16 / (int)sizeof(TG);       // elements per load
  static constexpr int NL = FP8 ? 2 : 4;                // loads per slab and accumulator
  static constexpr int LSTEP = BK / NL;                 // elements between them: both lane halves' shares
  static constexpr int SLAB_BYTES = P * ST_Q * LD * (int)sizeof(TQ);
};

// The query slab stager: TkStager<TQ, ST_Q, P>'s slabs ([P][ST_Q][LD], zero past NQ and past K; one 16-byte load per
// thread and plane) with loads that are never predicated.  A load at a place that does not exist reads the start of the
// plane instead and a select zeroes it on the way into LDS: a branch round a load makes the compiler wait for EVERY load
// in flight at the next use of its result, and that would drain the gallery stream once per slab.
template <class TG>
struct StQueryStager {
  using X = StKind<TG>;
  using TQ = typename X::TQ;
  using V = typename X::V;
  static constexpr int EL = 16 / (int)sizeof(TQ);  // 8 loads cover a slab row in both kinds
  static_assert(X::TS::N == 1 && X::BK == 8 * EL, "one load per thread and plane");
  int64_t off;  // of the thread's row in a plane, < 0 = no such query
  int c0;
  bool in;      // whether the registers hold a place that exists: applied by `store`, a barrier after the load
  V reg[X::P];

  __device__ __forceinline__ void rows(int q0, int NQ, int K, int tid) {
    const int r = q0 + (tid >> 3);
    off = r < NQ ? (int64_t)r * K : -1;
    c0 = (tid & 7) * EL;
  }
  __device__ __forceinline__ void load(const TQ* const (&base)[X::P], int K, int kb) {
    in = off >= 0 && kb + c0 < K;
    const int64_t at = in ? off + kb + c0 : 0;
#pragma unroll
    for (int p = 0; p < X::P; ++p) reg[p] = *(const V*)(base[p] + at);
  }
  __device__ __forceinline__ void store(TQ* slab, int tid) const {
#pragma unroll
    for (int p = 0; p < X::P; ++p) *(V*)(slab + p * ST_Q * X::LD + (tid >> 3) * X::LD + c0) = in ? reg[p] : V{};
  }
};

// 8 e4m3fn codes -> 8 bf16, exactly: tk_widen_fp8's arithmetic on two dwords.
__device__ __forceinline__ bf16x8_t st_widen8(uint32_t w0, uint32_t w1) {
  uint32_t o[4];
  const uint32_t w[2] = {w0, w1};
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], false);  // bytes 0, 1 of dword i
    const f32x2 b = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], true);   // bytes 2, 3
    o[2 * i] = (__float_as_uint(a[0]) >> 16) | (__float_as_uint(a[1]) & 0xffff0000u);
    o[2 * i + 1] = (__float_as_uint(b[0]) >> 16) | (__float_as_uint(b[1]) & 0xffff0000u);
  }
  return __builtin_bit_cast(bf16x8_t, (u32x4{o[0], o[1], o[2], o[3]}));
}

// A lane's gallery row: a pointer that says "global memory" in its type.  The four of them are stepped in a loop; as
// plain pointers they come out of it as flat ones, and a flat load counts as an LDS operation too, so every wait for a
// query fragment would wait for the gallery stream.
template <class TG>
using StRow = const __attribute__((address_space(1))) TG*;

enum StNext { ST_NEXT_NONE, ST_NEXT_FULL, ST_NEXT_PART };

// Load l of the slab at kb for accumulator t -> b; rowp[t] is the lane's row AT that slab, its half's offset included (the
// caller steps the four pointers from slab to slab, so a load's own offset is an immediate).  PART: the slab reaches past
// K, a load at or past K is zeros (K is a whole number of loads).
template <class TG, bool PART>
__device__ __forceinline__ void st_load(typename StKind<TG>::V (&b)[StKind<TG>::NL][ST_T], StRow<TG> (&rowp)[ST_T], int l,
                                        int kb, int K, int h) {
  using X = StKind<TG>;
  using V = typename X::V;
#pragma unroll
  for (int t = 0; t < ST_T; ++t) {
    using GV = const __attribute__((address_space(1))) V*;
    if constexpr (PART) {  // past K: the row's first bytes, then zeros by a select -- no branch round a load (StQueryStager)
      const bool in = kb + l * X::LSTEP + h * X::EL < K;
      const V v = *(GV)(in ? rowp[t] + l * X::LSTEP : rowp[t] - (kb + h * X::EL));
      b[l][t] = in ? v : V{};
    } else {
      b[l][t] = *(GV)(rowp[t] + l * X::LSTEP);
    }
  }
}

// One slab of a wave: the MFMA steps of slab registers b against the query slab sq, and -- NEXT -- the loads of the slab at
// kb_next into every register set as its last MFMA has read it.
template <class TG, int NEXT>
__device__ __forceinline__ void st_slab(f32x16 (&acc)[ST_T], typename StKind<TG>::V (&b)[StKind<TG>::NL][ST_T],
                                        const typename StKind<TG>::TQ* sq, StRow<TG> (&rowp)[ST_T], int kb_next, int K,
                                        int l31, int h) {
  using X = StKind<TG>;
  // fenced for the scheduler: a load hoisted above the MFMAs that read its registers would need a second set of them
  const auto reload = [&](int l) {
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (NEXT == ST_NEXT_FULL) st_load<TG, false>(b, rowp, l, kb_next, K, h);
    if constexpr (NEXT == ST_NEXT_PART) st_load<TG, true>(b, rowp, l, kb_next, K, h);
    __builtin_amdgcn_sched_barrier(0);
  };
  if constexpr (X::F32) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {  // kk = 8 j: lane half h feeds k = kk + 4h + u to MFMA u
      const f32x4 av = *(const f32x4*)(sq + l31 * X::LD + 8 * j + 4 * h);
#pragma unroll
      for (int t = 0; t < ST_T; ++t)
#pragma unroll
        for (int u = 0; u < 4; ++u) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u], b[j][t][u], acc[t], 0, 0, 0);
      reload(j);
    }
  } else if constexpr (!X::FP8) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {  // kk = 16 j: lane half h holds k = kk + 8h .. + 7; hi, then lo
      bf16x8_t av[2];
#pragma unroll
      for (int p = 0; p < 2; ++p) av[p] = *(const bf16x8_t*)(sq + p * ST_Q * X::LD + l31 * X::LD + 16 * j + 8 * h);
#pragma unroll
      for (int t = 0; t < ST_T; ++t)
#pragma unroll
        for (int p = 0; p < 2; ++p)
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av[p], __builtin_bit_cast(bf16x8_t, b[j][t]), acc[t], 0, 0, 0);
      reload(j);
    }
  } else {
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) {  // one load = codes 32 jj + 16 h .. + 15 of the row: steps kk = 32 jj and 32 jj + 16
      bf16x8_t bv[2][ST_T];
#pragma unroll
      for (int t = 0; t < ST_T; ++t) {
        // lanes 32 .. 63 of the first swap with lanes 0 .. 31 of the second: afterwards (x0, x1) holds codes kk + 8h .. + 7
        // of the first step in both halves, (y0, y1) those of the second
        const auto s0 = __builtin_amdgcn_permlane32_swap(b[jj][t][0], b[jj][t][2], false, false);
        const auto s1 = __builtin_amdgcn_permlane32_swap(b[jj][t][1], b[jj][t][3], false, false);
        bv[0][t] = st_widen8(s0[0], s1[0]);
        bv[1][t] = st_widen8(s0[1], s1[1]);
      }
      reload(jj);
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        bf16x8_t av[2];
#pragma unroll
        for (int p = 0; p < 2; ++p)
          av[p] = *(const bf16x8_t*)(sq + p * ST_Q * X::LD + l31 * X::LD + 32 * jj + 16 * e + 8 * h);
#pragma unroll
        for (int t = 0; t < ST_T; ++t)
#pragma unroll
          for (int p = 0; p < 2; ++p) acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av[p], bv[e][t], acc[t], 0, 0, 0);
      }
    }
  }
}

// The K sweep of one wave: K streams slab by slab, the gallery through the registers b, one slab ahead (MINE; a wave whose
// tile is skipped only stages queries and keeps the barriers), the queries through the two LDS buffers sQ, ONE barrier per
// slab: slab s waits in buffer s & 1 while slab s + 1 is written to the other one, which every wave left before the
// barrier, and slab s + 2 is on its way to the stager's registers -- asked for BEFORE the slab's gallery loads, so the wait
// for it leaves those in flight.  The slabs whose successor is a whole slab run in the loop; the successor that reaches
// past K (predicated loads) and the last slab are peeled, so every body is straight-line code.  The previous sweep's reads
// of buffer 0 are behind its epilogue's barriers; this one leaves its last slab's reads unfenced.
template <class TG, bool MINE, class QLoad>
__device__ __forceinline__ void st_sweep(f32x16 (&acc)[ST_T], StQueryStager<TG>& Q, QLoad qload,
                                         typename StKind<TG>::TQ* sQ, StRow<TG> (&rowp)[ST_T], int K, int tid, int l31, int h) {
  using X = StKind<TG>;
  constexpr int kSlab = X::SLAB_BYTES / (int)sizeof(typename X::TQ);
  typename X::V b[X::NL][ST_T];
  // In the order of the loop body -- the query slab's loads, then the gallery slab's: the wait for the query registers at
  // the loop's head is the stricter of what its two ways in need, and it must leave a slab of gallery loads in flight.
  qload(0);
  Q.store(sQ, tid);
  qload(X::BK);
  if constexpr (MINE) {
    if (X::BK <= K) {
#pragma unroll
      for (int l = 0; l < X::NL; ++l) st_load<TG, false>(b, rowp, l, 0, K, h);
    } else {
#pragma unroll
      for (int l = 0; l < X::NL; ++l) st_load<TG, true>(b, rowp, l, 0, K, h);
    }
#pragma unroll
    for (int t = 0; t < ST_T; ++t) rowp[t] += X::BK;
  }
  int kb = 0, buf = 0;
  const auto slab = [&](auto next) {
    constexpr int NEXT = decltype(next)::value;
    __syncthreads();
    if constexpr (NEXT != ST_NEXT_NONE) {
      Q.store(sQ + (buf ^ 1) * kSlab, tid);
      qload(kb + 2 * X::BK);  // unconditional, past K too (zeros, never stored): the loop body has no branch
    }
    if constexpr (MINE) {
      st_slab<TG, NEXT>(acc, b, sQ + buf * kSlab, rowp, kb + X::BK, K, l31, h);
#pragma unroll
      for (int t = 0; t < ST_T; ++t) rowp[t] += X::BK;
    }
    kb += X::BK;
    buf ^= 1;
  };
  while (kb + 2 * X::BK <= K) slab(std::integral_constant<int, ST_NEXT_FULL>{});
  if (kb + X::BK < K) slab(std::integral_constant<int, ST_NEXT_PART>{});
  slab(std::integral_constant<int, ST_NEXT_NONE>{});
}

// Epilogue of a wave's 32 x 128 scores held as four 32x32 MFMA accumulators (lane: column t * 32 + l31, rows
// (r & 3) + 8 (r >> 2) + 4h): tk_tile_scores' arithmetic, expression for expression, into sS [ST_Q][TK_SLD].  A column
// past g_end has no item (g = -1): weights and scale 0, as there.
template <bool SCALE>
__device__ __forceinline__ void st_tile_scores(const f32x16 (&acc)[ST_T], float* sS, const float* sQw, const float* gw, int M,
                                               int g0, int g_end, int l31, int h, const float* gscale) {
#pragma unroll
  for (int t = 0; t < ST_T; ++t) {
    const int col = t * 32 + l31, g = g0 + col < g_end ? g0 + col : -1;
    float sc = 1.f;
    if constexpr (SCALE) sc = g >= 0 ? gscale[g] : 0.f;
    float den[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) den[r] = 0.f;
    for (int m = 0; m < M; ++m) {
      const float gwm = g >= 0 ? gw[(int64_t)g * M + m] : 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) den[r] += sQw[((r & 3) + 8 * (r >> 2) + 4 * h) * MMT_MAX_EXPERTS + m] * gwm;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
      float num = acc[t][r];
      if constexpr (SCALE) num = tk_mul_rn(num, sc);
      sS[row * TK_SLD + col] = num / (den[r] == 0.f ? 1e-5f : den[r]);
    }
  }
}

// One block: 32 queries x one gallery chunk -> the chunk's sorted k best per query in the workspace.
template <class TG, bool MASKED, bool AFTER, class Args = StArgs>
__global__ __launch_bounds__(256, 2) void topk_stream_kernel(Args a) {
  using X = StKind<TG>;
  using TQ = typename X::TQ;
  static_assert(!AFTER || MASKED, "the paged kernels extend the masked ones");
  constexpr bool WHERE = TkWhere<Args>::value;
  static_assert(!WHERE || AFTER, "the filtered kernels extend the paged ones");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, h = lane >> 5;
  const int bid = xcd_remap(blockIdx.x, gridDim.x);  // gallery-chunk-major: the query tiles of a chunk meet in L2
  const int chunk = bid / a.n_qt, q0 = (bid % a.n_qt) * ST_Q;
  // in 64 bits: the end of the last sweep may lie past 2^31 where NV (gated to INT_MAX - ST_G) does not
  const int g_begin = (int)((int64_t)chunk * a.tiles / a.n_chunks * ST_G);
  const int g_end = (int)min((int64_t)a.NV, (int64_t)(chunk + 1) * a.tiles / a.n_chunks * ST_G);
  const int K = a.K, cap = a.k + 64, rows_live = a.NQ - q0;

  TQ* sQ = (TQ*)smem;                                             // [2][P][ST_Q][LD] query slabs
  float* sS = (float*)(smem + 2 * X::SLAB_BYTES);                 // [ST_Q][TK_SLD] scores of one wave's tile
  float* sQw = (float*)((unsigned char*)sS + ST_TILE_BYTES);      // [ST_Q][MMT_MAX_EXPERTS]
  int* sN = (int*)((unsigned char*)sQw + ST_QW_BYTES);            // [ST_Q] candidates held
  uint64_t* sT = (uint64_t*)(sN + ST_Q);                          // [ST_Q] thresholds
  uint64_t* sC = sT + ST_Q;                                       // [ST_Q][cap] candidates
  int* sEx = (int*)(sC + ST_Q * cap);                             // masked: [ST_Q][E] exclusions
  uint64_t* sB = (uint64_t*)(sEx + ST_Q * (MASKED ? a.E : 0));    // paged: [ST_Q] bounds
  if (tid < ST_Q) { sN[tid] = 0; sT[tid] = 0; }
  for (int i = tid; i < ST_Q * MMT_MAX_EXPERTS; i += 256) {
    const int r = i / MMT_MAX_EXPERTS, m = i % MMT_MAX_EXPERTS;
    sQw[i] = (q0 + r < a.NQ && m < a.M) ? a.qw[(int64_t)(q0 + r) * a.M + m] : 0.f;
  }
  if constexpr (MASKED)
    for (int i = tid; i < ST_Q * a.E; i += 256) sEx[i] = q0 + i / a.E < a.NQ ? (int)a.exclude[(int64_t)q0 * a.E + i] : -1;
  if constexpr (WHERE) {
    if (tid < ST_Q) sB[tid] = q0 + tid < a.NQ ? (a.after ? a.after[q0 + tid] : ~0ull) : 0ull;  // filtered: a null cursor
  } else if constexpr (AFTER) {
    if (tid < ST_Q) sB[tid] = q0 + tid < a.NQ ? a.after[q0 + tid] : 0ull;
  }
  uint64_t* sW = nullptr;                                         // filtered: [ST_Q][3] masks, behind the bounds
  if constexpr (WHERE) {
    sW = sB + ST_Q;
    tk_load_where<ST_Q>(sW, a.where, a.NQ, q0, tid);
  }
  // all of the above is read behind the barriers of the first sweep

  StQueryStager<TG> Q;
  Q.rows(q0, a.NQ, K, tid);
  const auto qload = [&](int kb) {
    if constexpr (X::F32) Q.load({(const float*)a.q}, K, kb);
    else Q.load({(const bf16_t*)a.q, (const bf16_t*)a.q_lo}, K, kb);
  };

  for (int G0 = g_begin; G0 < g_end; G0 += ST_G) {
    // the sweep's four tiles: whether they hold an item at all, and their subset words (block-uniform)
    uint64_t m0[4], m1[4];
    bool live[4], any = false;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      m0[w] = m1[w] = ~0ull;
      live[w] = G0 + w * TK_G < g_end;
      if constexpr (MASKED)
        if (live[w] && a.subset) live[w] = tk_tile_mask(a.subset, G0 + w * TK_G, m0[w], m1[w]);
      any = any || live[w];
    }
    if (!any) continue;  // nothing of this sweep is allowed: no loads, no MFMAs, no barrier
    bool mine = false;   // wave-uniform: this wave's tile is scored
#pragma unroll
    for (int w = 0; w < 4; ++w) mine = w == wave ? live[w] : mine;
    const int g0 = G0 + wave * TK_G;

    f32x16 acc[ST_T];
#pragma unroll
    for (int t = 0; t < ST_T; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    StRow<TG> rowp[ST_T];  // the lane's rows, its half's offset included
#pragma unroll
    for (int t = 0; t < ST_T; ++t)
      rowp[t] = (StRow<TG>)(const TG*)a.g + (int64_t)min(g0 + 32 * t + l31, a.NV - 1) * K + h * X::EL;
    if (mine) st_sweep<TG, true>(acc, Q, qload, sQ, rowp, K, tid, l31, h);
    else st_sweep<TG, false>(acc, Q, qload, sQ, rowp, K, tid, l31, h);
    // the waves take turns with the score tile (one copy of the selection code: the loop stays rolled)
#pragma nounroll
    for (int w = 0; w < 4; ++w) {
      bool lw = false;
      uint64_t x0 = 0, x1 = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (i == w) { lw = live[i]; x0 = m0[i]; x1 = m1[i]; }
      if (!lw) continue;  // block-uniform
      uint64_t t0 = 0, t1 = 0;  // filtered: the tags of the lane's two columns, on their way during the epilogue
      if constexpr (WHERE) tk_tile_tags(a.tags, G0 + w * TK_G, g_end, lane, t0, t1);
      if (w == wave) st_tile_scores<X::FP8>(acc, sS, sQw, a.gw, a.M, g0, g_end, l31, h, a.gscale);
      __syncthreads();
      if constexpr (WHERE)
        tk_tile_select<true, true, ST_Q, true>(sS, sC, sN, sT, a.k, rows_live, G0 + w * TK_G, g_end, wave, lane, x0, x1, sEx,
                                               a.E, sB, sW, t0, t1);
      else
        tk_tile_select<MASKED, AFTER, ST_Q>(sS, sC, sN, sT, a.k, rows_live, G0 + w * TK_G, g_end, wave, lane, x0, x1, sEx,
                                    MASKED ? a.E : 0, sB);
      __syncthreads();
    }
  }
  __syncthreads();
  uint64_t* ws = a.ws + chunk * (int64_t)a.k;
  const int64_t ws_row = (int64_t)a.n_chunks * a.k;
  for (int rr = 0; rr < ST_Q / 4; ++rr) {
    const int row = wave * (ST_Q / 4) + rr, q = q0 + row;
    if (q >= a.NQ) break;
    tk_flush(sC + row * cap, sN[row], a.k, lane, ws + q * ws_row);
  }
}

// The merge of this schedule's chunk lists: one block per query, the n_chunks sorted lists of k keys -> the best kout, by
// rank, as topk_merge_kernel -- which a single query leaves with one block that walks every list for every key it cannot
// rule out (measured at 512 lists of 10: about 1.45 ms, up to five times the scan: DESIGN 9.21).  Here the HEADS decide
// first.  A list whose head has kout or more heads above it holds nothing of the best kout (those heads, all above
// everything in it, already fill them); so only the lists whose head ranks below kout among the heads are candidates, at
// most kout of them, and they hold every key of the answer.  A key of a candidate list with fewer than kout keys above it
// in ALL lists has none of them in a list that is no candidate (such a list's head, and the kout heads above that, would
// all be above the key), and a key with kout or more above it has the whole answer above it, inside the candidates: so
// "rank < kout", counted over the candidate lists alone, picks the same keys, and their ranks there are their ranks.  Keys
// are distinct, a rank is unique: the output is topk_merge_kernel's by construction.  Candidates are walked best head
// first, so a key that does not make it is out after a list or two.  sH [n_chunks] heads, sCand [kout] the candidate
// lists by head rank, sL (STAGE: the candidates fit) their first min(k, kout) keys.
__global__ __launch_bounds__(256) void topk_stream_merge_kernel(const uint64_t* __restrict__ ws, int n_chunks, int k, int kout,
                                                                int stage, float* __restrict__ scores,
                                                                int64_t* __restrict__ index) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int q = blockIdx.x, tid = threadIdx.x, lim = min(k, kout);
  const uint64_t* L = ws + (int64_t)q * n_chunks * k;
  uint64_t* sH = (uint64_t*)smem;
  int* sCand = (int*)(sH + n_chunks);
  uint64_t* sL = (uint64_t*)(sCand + ((kout + 1) & ~1));
  for (int c = tid; c < n_chunks; c += 256) sH[c] = L[(int64_t)c * k];
  for (int i = tid; i < kout; i += 256) sCand[i] = -1;
  __syncthreads();
  for (int c = tid; c < n_chunks; c += 256) {
    const uint64_t h = sH[c];
    if (!h) continue;  // an empty list
    int r = 0;
    for (int c2 = 0; c2 < n_chunks; ++c2) r += sH[c2] > h;
    if (r < kout) sCand[r] = c;  // distinct keys: one writer per slot, slots 0 .. nc - 1 without a gap
  }
  __syncthreads();
  int nc = 0;
  while (nc < kout && sCand[nc] >= 0) ++nc;
  if (stage) {
    for (int i = tid; i < nc * lim; i += 256) sL[i] = L[(int64_t)sCand[i / lim] * k + i % lim];
    __syncthreads();
  }
  for (int i = tid; i < nc * lim; i += 256) {
    const int ci = i / lim, j = i - ci * lim;
    const uint64_t key = stage ? sL[i] : L[(int64_t)sCand[ci] * k + j];
    if (!key) continue;
    int rank = j;
    for (int c2 = 0; c2 < nc && rank < kout; ++c2) {
      if (c2 == ci) continue;
      const uint64_t* l = stage ? sL + c2 * lim : L + (int64_t)sCand[c2] * k;
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

namespace {
// The chunk rule: the gallery is `tiles` sweeps of 512 items, cut into n_chunks runs of consecutive sweeps as evenly as
// whole sweeps allow (chunk c = sweeps c * tiles / n_chunks .. (c + 1) * tiles / n_chunks - 1).  n_chunks = one per sweep
// while that stays within two blocks per CU over all query tiles (TK_FILL blocks), beyond that as many as TK_FILL asks
// for, and never fewer than a block per ST_MAX_TILES sweeps: a minimum of non-decreasing functions of NV, so non-decreasing.
void st_geometry(StArgs& a) {
  a.n_qt = (a.NQ + ST_Q - 1) / ST_Q;
  a.tiles = (a.NV + ST_G - 1) / ST_G;
  const int want = TK_FILL / a.n_qt > 1 ? TK_FILL / a.n_qt : 1, deep = (a.tiles + ST_MAX_TILES - 1) / ST_MAX_TILES;
  const int n = want > deep ? want : deep;
  a.n_chunks = a.tiles < n ? a.tiles : n;
}

// NV at most INT_MAX - ST_G: an item number of a sweep's last, partly empty tile is then still an int.
bool st_args_ok(int NQ, int NV, int k) { return NQ > 0 && NV > 0 && NV <= 0x7fffffff - ST_G && k >= 1 && k <= TK_MAXK; }

template <class TG>
size_t st_lds(int k, int E, bool after, bool where = false) {
  return 2 * StKind<TG>::SLAB_BYTES + ST_TILE_BYTES + ST_QW_BYTES + ST_Q * (4 + 8) + (size_t)ST_Q * (k + 64) * 8 +
         (size_t)ST_Q * E * 4 + (after ? ST_Q * 8 : 0) + (where ? TK_WHERE_BYTES(ST_Q) : 0);
}

// The k = 128 footprint is over the 64 KiB default.
void st_lds_limits() {
  static bool done[64] = {};
  const size_t f32 = st_lds<float>(TK_MAXK, TK_MAXE, true), bf16 = st_lds<bf16_t>(TK_MAXK, TK_MAXE, true);
  tk_lds_limits(done, {{(const void*)topk_stream_kernel<float, false, false>, f32},
                       {(const void*)topk_stream_kernel<float, true, false>, f32},
                       {(const void*)topk_stream_kernel<float, true, true>, f32},
                       {(const void*)topk_stream_kernel<bf16_t, false, false>, bf16},
                       {(const void*)topk_stream_kernel<bf16_t, true, false>, bf16},
                       {(const void*)topk_stream_kernel<bf16_t, true, true>, bf16},
                       {(const void*)topk_stream_kernel<uint8_t, false, false>, bf16},
                       {(const void*)topk_stream_kernel<uint8_t, true, false>, bf16},
                       {(const void*)topk_stream_kernel<uint8_t, true, true>, bf16}});
}

void st_where_lds_limits() {
  static bool done[64] = {};
  const size_t f32 = st_lds<float>(TK_MAXK, TK_MAXE, true, true), bf16 = st_lds<bf16_t>(TK_MAXK, TK_MAXE, true, true);
  tk_lds_limits(done, {{(const void*)topk_stream_kernel<float, true, true, StWhereArgs>, f32},
                       {(const void*)topk_stream_kernel<bf16_t, true, true, StWhereArgs>, bf16},
                       {(const void*)topk_stream_kernel<uint8_t, true, true, StWhereArgs>, bf16}});
}

// The merge launch of this path; lists beyond what the heads' LDS holds go to the tile schedule's merge.
int st_merge_launch(const uint64_t* ws, int NQ, int n_chunks, int k, int kout, float* scores, int64_t* index, hipStream_t s) {
  constexpr size_t kLdsMax = 64 * 1024;
  const int lim = k < kout ? k : kout;
  const size_t heads = (size_t)n_chunks * 8 + (size_t)((kout + 1) & ~1) * 4, lists = (size_t)kout * lim * 8;
  if (heads > kLdsMax) return tk_merge_launch(ws, NQ, n_chunks, k, kout, scores, index, s);
  const int stage = heads + lists <= kLdsMax;
  hipLaunchKernelGGL(topk_stream_merge_kernel, dim3(NQ), dim3(256), heads + (stage ? lists : 0), s, ws, n_chunks, k, kout,
                     stage, scores, index);
  return (int)hipGetLastError();
}

// Gate, geometry, the chunk scan and the merge: tk_search's gates in tk_search's order.  Args = StWhereArgs: the filtered
// search, with its tags and masks.
template <class TG, class Args = StArgs>
int st_search(const MmtSearchScan& s, int k, uint64_t* ws, float* scores, int64_t* index, void* stream,
              const uint64_t* tags = nullptr, const uint64_t* where = nullptr) {
  constexpr bool BF16 = !StKind<TG>::F32, FP8 = StKind<TG>::FP8, WHERE = TkWhere<Args>::value;
  if (!tk_scan_operands<BF16, FP8>(s) || !ws || !index || !st_args_ok(s.NQ, s.NV, k) ||
      !tk_shape_ok(s.NQ, s.NV, s.M, s.d, BF16, FP8) || (WHERE && (!tags || !where)))
    return MMT_ERR_ARG;
  if (((uintptr_t)s.q | (uintptr_t)s.q_lo | (uintptr_t)s.g) & 15) return MMT_ERR_ALIGN;
  if (s.E < 0 || s.E > TK_MAXE || (s.E > 0 && !s.exclude)) return MMT_ERR_ARG;
  if ((uintptr_t)s.subset & 15) return MMT_ERR_ALIGN;  // null = every item allowed
  Args a = {};
  a.q = s.q; a.q_lo = s.q_lo; a.qw = s.qw; a.g = s.g; a.gw = s.gw; a.gscale = s.gscale; a.ws = ws;
  a.subset = s.subset; a.exclude = s.exclude; a.after = s.after;
  a.NQ = s.NQ; a.NV = s.NV; a.M = s.M; a.K = s.M * s.d; a.k = k; a.E = s.E;
  st_geometry(a);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(a.n_qt * a.n_chunks);
  if constexpr (WHERE) {
    a.tags = tags; a.where = where;
    st_where_lds_limits();
    hipLaunchKernelGGL((topk_stream_kernel<TG, true, true, Args>), grid, dim3(256), st_lds<TG>(k, s.E, true, true), st, a);
  } else {
    st_lds_limits();
    const bool after = s.after != nullptr, masked = after || s.subset || s.E;
    const size_t lds = st_lds<TG>(k, s.E, after);
    if (after) hipLaunchKernelGGL((topk_stream_kernel<TG, true, true>), grid, dim3(256), lds, st, a);
    else if (masked) hipLaunchKernelGGL((topk_stream_kernel<TG, true, false>), grid, dim3(256), lds, st, a);
    else hipLaunchKernelGGL((topk_stream_kernel<TG, false, false>), grid, dim3(256), lds, st, a);
  }
  return st_merge_launch(ws, s.NQ, a.n_chunks, k, k < s.NV ? k : s.NV, scores, index, st);
}
}  // namespace

extern "C" int64_t mmt_topk_stream_workspace_keys(int NQ, int NV, int k) {
  if (!st_args_ok(NQ, NV, k)) return MMT_ERR_ARG;
  StArgs a = {};
  a.NQ = NQ; a.NV = NV;
  st_geometry(a);
  return (int64_t)NQ * a.n_chunks * k;
}

extern "C" int mmt_search_topk_stream(const MmtSearchScan* scan, int k, uint64_t* ws, float* scores, int64_t* index,
                                      void* stream) {
  if (const int rc = tk_scan_gate(scan, SC_SUBSET | SC_EXCLUDE | SC_AFTER | SC_FP8)) return rc;
  if (scan->storage == MMT_SEARCH_FP8) return st_search<uint8_t>(*scan, k, ws, scores, index, stream);
  if (scan->storage == MMT_SEARCH_BF16) return st_search<bf16_t>(*scan, k, ws, scores, index, stream);
  return st_search<float>(*scan, k, ws, scores, index, stream);
}

// The filtered search on this schedule: mmt_search_topk_where's arguments and answer, mmt_search_topk_stream's workspace.
extern "C" int mmt_search_topk_stream_where(const MmtSearchScan* scan, const uint64_t* tags, const uint64_t* where, int k,
                                            uint64_t* ws, float* scores, int64_t* index, void* stream) {
  if (const int rc = tk_scan_gate(scan, SC_SUBSET | SC_EXCLUDE | SC_AFTER | SC_FP8)) return rc;
  if (scan->storage == MMT_SEARCH_FP8) return st_search<uint8_t, StWhereArgs>(*scan, k, ws, scores, index, stream, tags, where);
  if (scan->storage == MMT_SEARCH_BF16) return st_search<bf16_t, StWhereArgs>(*scan, k, ws, scores, index, stream, tags, where);
  return st_search<float, StWhereArgs>(*scan, k, ws, scores, index, stream, tags, where);
}
