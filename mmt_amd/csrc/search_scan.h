// The scoring tile of the gallery scans, shared by every kernel that scores a (query, item) pair: the top-k kernels
// (search.hip: a running top-k per query), the count / threshold kernels (search_rank.hip: a counter per query and
// target), the range kernels (search_range.hip: every hit) and the querybank column pass (search_norm.hip).  Block shape,
// the K loop (tk_scan: fp32 gallery on v_mfma_f32_32x32x2_f32, bf16 gallery on v_mfma_f32_32x32x16_bf16 -- an fp8 gallery is
// widened to bf16 on its way into LDS and runs the bf16 loop), the gated-denominator epilogue (with an fp8 gallery: the
// item's scale first) and the querybank rewrite are composed in ONE place, tk_tile, so a pair has the same score bits on
// every path by construction.  The K loop is itself a composition -- slab stager, loop with its barriers, MFMA step -- and
// the kernels that score two STORED rows (search_self.hip, search_diverse.hip) are made of the same three pieces and of ONE
// definition of that similarity, tk_pair_sims.  The subset gate of a tile (tk_tile_mask), the chunk rule and launch
// geometry (tk_chunk, tk_geometry), the shape gate and the per-device dynamic-LDS limit (tk_lds_limits) are here once as
// well, and so are the steps that follow a tile on more than one path: the count step (tk_tile_count), the range step
// (TkRange), the query-set pooling (tk_tile_pool) and the item-set pooling (tk_tile_pool_items, with the unaligned subset
// window tk_tile_mask_window).  The per-query attribute filter is here too: the predicate (tk_tag_pass), its staging, its
// tile gate (TkWhereGate, tk_tile_where_any) and the WHERE forms of the count and range steps.
//
// Which row a slab row / tile column holds is a functor `row(r)` on both sides -> row number, or -1 for "none" (zero-filled
// in registers, never read): g0 + r for a scan's gallery side, a table lookup for the rank kernels' threshold pass and the
// stored-row kernels, q0 + r below NQ for a query.
#pragma once
#include <cmath>
#include <initializer_list>
#include <type_traits>

#include "mmt_common.h"
#include "../../include/mmt_hip.h"

typedef __attribute__((ext_vector_type(16))) float f32x16;

#define TK_Q 64                  // query rows per block (4 waves: 2 x 2 of 32 rows x 64 columns)
#define TK_G 128                 // gallery columns per tile
#define TK_SLD (TK_G + 4)        // score tile row pitch
#define TK_CHUNK 4096            // gallery columns per block at full occupancy
#define TK_FILL 512              // blocks wanted per launch before the chunk is allowed to shrink (2 per CU)
#define TK_TILE_BYTES (TK_Q * TK_SLD * 4)
#define TK_QW_BYTES (TK_Q * MMT_MAX_EXPERTS * 4)

#define TK_BK 32                 // fp32 contraction slab
#define TK_LD (TK_BK + 4)        // slab row pitch (floats): conflict-free ds_read_b128 across 16 consecutive rows
#define TK_SLAB_BYTES ((TK_Q + TK_G) * TK_LD * 4)
#define TK_UNION_BYTES (TK_TILE_BYTES > TK_SLAB_BYTES ? TK_TILE_BYTES : TK_SLAB_BYTES)

#define TKB_BK 64                 // bf16 contraction slab (bf16 elements): 128 bytes of a folded row
#define TKB_LD (TKB_BK + 8)       // slab row pitch (bf16): 36 dwords, the fp32 kernel's conflict-free pitch
#define TKB_SLAB_BYTES ((2 * TK_Q + TK_G) * TKB_LD * 2)
#define TKB_UNION_BYTES (TK_TILE_BYTES > TKB_SLAB_BYTES ? TK_TILE_BYTES : TKB_SLAB_BYTES)

// Query weights of the block's rows -> sQw [TK_Q][MMT_MAX_EXPERTS], zero past NQ / M.
__device__ __forceinline__ void tk_load_qw(float* sQw, const float* qw, int NQ, int M, int q0, int tid) {
  for (int i = tid; i < TK_Q * MMT_MAX_EXPERTS; i += 256) {
    const int r = i / MMT_MAX_EXPERTS, m = i % MMT_MAX_EXPERTS;
    sQw[i] = (q0 + r < NQ && m < M) ? qw[(int64_t)(q0 + r) * M + m] : 0.f;
  }
}

// 16 fp8 values (OCP e4m3fn, one 16-byte load) -> 16 bf16 as two 16-byte halves, exactly: every e4m3fn value is a bf16
// value (3 mantissa bits against 7, and the range fits), so the upper half of v_cvt_pk_f32_fp8's fp32 IS the bf16.
__device__ __forceinline__ void tk_widen_fp8(const u32x4& v, u32x4& lo, u32x4& hi) {
  uint32_t o[8];
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8((int)v[w], false);  // bytes 0, 1 of dword w
    const f32x2 b = __builtin_amdgcn_cvt_pk_f32_fp8((int)v[w], true);   // bytes 2, 3
    o[2 * w] = (__float_as_uint(a[0]) >> 16) | (__float_as_uint(a[1]) & 0xffff0000u);
    o[2 * w + 1] = (__float_as_uint(b[0]) >> 16) | (__float_as_uint(b[1]) & 0xffff0000u);
  }
  lo = u32x4{o[0], o[1], o[2], o[3]};
  hi = u32x4{o[4], o[5], o[6], o[7]};
}

// The K loops.  Every contraction over the folded row -- a query against stored rows (tk_scan in tk_tile), stored rows
// against stored rows (tk_scan in search_self.hip, the Gram of search_diverse.hip) -- is a composition of three pieces, so
// the slab sequence (kb ascending) and the MFMA sequence inside a slab (kk ascending; then u ascending for fp32, hi before
// lo for a query's two bf16 planes; ONE accumulator per output) are the same everywhere by construction.
//
// 1. The slab stager: ROWS (64 or 128) rows of one slab, staged through registers it owns, 16 bytes per load.  T is what a
// row is stored as: float (32-wide slabs, pitch TK_LD), bf16_t = bf16 bits, or uint8_t = e4m3fn codes (64-wide slabs of
// bf16, pitch TKB_LD; the codes are widened on their way into LDS, here and nowhere else).  K % EL == 0, so a load is
// inside its row or past its end as a whole.  P planes of the same rows (a query's hi and lo) share one stager, so the
// load predicate and the row offset are formed once for both.
template <class T, int ROWS, int P = 1>
struct TkStager {
  static constexpr bool F32 = std::is_same_v<T, float>, FP8 = std::is_same_v<T, uint8_t>;
  using S = std::conditional_t<F32, float, bf16_t>;   // what the slab holds in LDS
  using V = std::conditional_t<F32, f32x4, u32x4>;    // one load
  static constexpr int BK = F32 ? TK_BK : TKB_BK;     // contraction values per slab
  static constexpr int LD = F32 ? TK_LD : TKB_LD;     // slab row pitch, in S
  static constexpr int KK = F32 ? 8 : 16;             // contraction values per fragment step: lane half h holds kk + KK/2 * h ..
  static constexpr int EL = 16 / sizeof(T);           // elements per load
  static constexpr int SH = FP8 ? 2 : 3;              // log2 of the loads per row and slab
  static constexpr int N = (ROWS << SH) / 256;        // loads per thread and slab
  int at[N];
  V reg[P][N];  // P planes of the same rows (a query's hi and lo), one behind the other in LDS

  template <class Row>
  __device__ __forceinline__ void rows(Row row, int tid) {
#pragma unroll
    for (int j = 0; j < N; ++j) at[j] = row((tid + 256 * j) >> SH);
  }
  // slab kb of the planes base[p] [.][K] -> registers
  __device__ __forceinline__ void load(const T* const (&base)[P], int K, int kb, int tid) {
#pragma unroll
    for (int j = 0; j < N; ++j) {
      const int c = kb + ((tid + 256 * j) & ((1 << SH) - 1)) * EL;
      const bool in = at[j] >= 0 && c < K;
      const int64_t off = (int64_t)at[j] * K + c;
#pragma unroll
      for (int p = 0; p < P; ++p) reg[p][j] = in ? *(const V*)(base[p] + off) : V{};
    }
  }
  // registers -> slabs [P][ROWS][LD]
  __device__ __forceinline__ void store(S* slab, int tid) const {
#pragma unroll
    for (int j = 0; j < N; ++j) {
      const int i = tid + 256 * j, o = (i >> SH) * LD + (i & ((1 << SH) - 1)) * EL;
#pragma unroll
      for (int p = 0; p < P; ++p) {
        S* dst = slab + p * ROWS * LD + o;
        if constexpr (FP8) {
          u32x4 lo, hi;
          tk_widen_fp8(reg[p][j], lo, hi);
          *(u32x4*)dst = lo;
          *(u32x4*)(dst + 8) = hi;
        } else {
          *(V*)dst = reg[p][j];
        }
      }
    }
  }
};

// 2. The loop and its barrier discipline, stated once: K streams through LDS slab by slab, the next slab's global loads
// (`load(kb)`) in flight during the current slab's MFMAs (`step(kk)`, KK contraction values each).  It OPENS with a barrier
// (what shared the slabs' LDS before, the previous tile's scores for one, is consumed) and leaves the last slab's reads
// UNFENCED: the caller syncs before it reuses that LDS.
template <int BK, int KK, class Load, class Store, class Step>
__device__ __forceinline__ void tk_k_loop(int K, Load load, Store store, Step step) {
  load(0);
  for (int kb = 0; kb < K; kb += BK) {
    __syncthreads();
    store();
    __syncthreads();
    if (kb + BK < K) load(kb + BK);
#pragma unroll
    for (int kk = 0; kk < BK; kk += KK) step(kk);
  }
}

// 3. The fragment step of a wave: S x T accumulators of 32 x 32 (acc[s * T + t]) take KK contraction values of slab rows
// ar + 32 s (A) and br + 32 t (B), the lane's own row l31 included in ar / br.  `live(s, t)` is wave-uniform and stays
// outside the arithmetic: a dead output is not multiplied.  fp32 rows: lane half h feeds k = kk + 4h + u to MFMA u.
template <int P, int S, int T, class Live>
__device__ __forceinline__ void tk_step(f32x16* acc, const float* a, int ar, const float* b, int br, int kk, int h, Live live) {
  static_assert(P == 1, "fp32 rows are one plane");
  f32x4 av[S], bv[T];
#pragma unroll
  for (int s = 0; s < S; ++s) av[s] = *(const f32x4*)(a + (ar + s * 32) * TK_LD + kk + 4 * h);
#pragma unroll
  for (int t = 0; t < T; ++t) bv[t] = *(const f32x4*)(b + (br + t * 32) * TK_LD + kk + 4 * h);
#pragma unroll
  for (int s = 0; s < S; ++s)
#pragma unroll
    for (int t = 0; t < T; ++t)
      if (live(s, t)) {
#pragma unroll
        for (int u = 0; u < 4; ++u)
          acc[s * T + t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s][u], bv[t][u], acc[s * T + t], 0, 0, 0);
      }
}

// bf16 slabs: lane half h holds k = kk + 8h .. + 7 of its row, one v_mfma_f32_32x32x16_bf16 per A plane.  The A side is P
// planes [TK_Q][TKB_LD] one behind the other: a query's hi then lo (a B fragment is read once and feeds both), a stored
// row's single plane of exact bf16 values.
template <int P, int S, int T, class Live>
__device__ __forceinline__ void tk_step(f32x16* acc, const bf16_t* a, int ar, const bf16_t* b, int br, int kk, int h, Live live) {
  bf16x8_t av[P][S], bv[T];
#pragma unroll
  for (int p = 0; p < P; ++p)
#pragma unroll
    for (int s = 0; s < S; ++s) av[p][s] = *(const bf16x8_t*)(a + p * TK_Q * TKB_LD + (ar + s * 32) * TKB_LD + kk + 8 * h);
#pragma unroll
  for (int t = 0; t < T; ++t) bv[t] = *(const bf16x8_t*)(b + (br + t * 32) * TKB_LD + kk + 8 * h);
#pragma unroll
  for (int s = 0; s < S; ++s)
#pragma unroll
    for (int t = 0; t < T; ++t)
      if (live(s, t)) {
#pragma unroll
        for (int p = 0; p < P; ++p)
          acc[s * T + t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av[p][s], bv[t], acc[s * T + t], 0, 0, 0);
      }
}

// K loop of one 64 x 128 tile: acc = A[arow(.)] . G[grow(.)]^T, the block's 4 waves as 2 x 2 of 32 rows x 64 columns.
// A is P planes of TA (a[p] [.][K]), G one of TB; smem holds the slabs [P][TK_Q][LD] then [TK_G][LD] (TK_SLAB_BYTES,
// TKB_SLAB_BYTES with two planes).  Barriers: tk_k_loop's.
template <int P, class TA, class TB, class ARow, class GRow>
__device__ __forceinline__ void tk_scan(f32x16 (&acc)[2], unsigned char* smem, const TA* const (&a)[P], ARow arow, const TB* g,
                                        GRow grow, int K, int tid, int wq, int wg, int l31, int h) {
  using SA = TkStager<TA, TK_Q, P>;
  using SB = TkStager<TB, TK_G>;
  using S = typename SB::S;
  static_assert(std::is_same_v<S, typename SA::S>, "both sides are staged into slabs of one kind");
  constexpr int LD = SB::LD;
  S* sA = (S*)smem;
  S* sB = sA + P * TK_Q * LD;
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  SA A;
  SB B;
  A.rows(arow, tid);
  B.rows(grow, tid);
  tk_k_loop<SB::BK, SB::KK>(
      K,
      [&](int kb) {
        A.load(a, K, kb, tid);
        B.load({g}, K, kb, tid);
      },
      [&] {
        A.store(sA, tid);
        B.store(sB, tid);
      },
      [&](int kk) {
        tk_step<P, 1, 2>(acc, sA, wq * 32 + l31, sB, wg * 64 + l31, kk, h, [](int, int) { return true; });
      });
}

// fl(a * b) as an instruction of its own: the optimiser cannot contract it with a following add or subtract into an fma
// (plain `a * b`, and __fmul_rn which is defined as that, may be under -ffast-math).
__device__ __forceinline__ float tk_mul_rn(float a, float b) {
  float r;
  asm("v_mul_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}

// Epilogue of one 64 x 128 tile held as 32x32 MFMA accumulators (lane: column wg*64 + t*32 + l31, rows
// wq*32 + (r&3) + 8*(r>>2) + 4h -- the layout of v_mfma_f32_32x32x2_f32 and v_mfma_f32_32x32x16_bf16 alike): divides by
// the gated denominator and leaves the scores in sS [TK_Q][TK_SLD].  SCALE (an fp8 gallery): the accumulator is first
// multiplied by the item's scale gscale[grow(col)], a power of two, as a rounded multiply of its own (tk_mul_rn):
// score = fl(fl(acc * scale) / den); a column without an item gets the scale 0.
template <bool SCALE = false, class GRow>
__device__ __forceinline__ void tk_tile_scores(const f32x16 (&acc)[2], float* sS, const float* sQw, const float* gw, int M,
                                               GRow grow, int wq, int wg, int l31, int h, const float* gscale = nullptr) {
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int col = wg * 64 + t * 32 + l31, g = grow(col);
    float sc = 1.f;
    if constexpr (SCALE) sc = g >= 0 ? gscale[g] : 0.f;
    float den[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) den[r] = 0.f;
    for (int m = 0; m < M; ++m) {
      const float gwm = g >= 0 ? gw[(int64_t)g * M + m] : 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) den[r] += sQw[(wq * 32 + (r & 3) + 8 * (r >> 2) + 4 * h) * MMT_MAX_EXPERTS + m] * gwm;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = wq * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
      float num = acc[t][r];
      if constexpr (SCALE) num = tk_mul_rn(num, sc);
      sS[row * TK_SLD + col] = num / (den[r] == 0.f ? 1e-5f : den[r]);
    }
  }
}

// Querybank normalisation of one score tile in place (tk_tile<., true> only): sS[r][c] = fl(fl(beta * sS[r][c]) - lse[item
// of column c]) -- a rounded multiply, then a rounded subtract, never an fma, so the value can be restated bit for bit.
// Two threads per column (rows of one parity each); a thread reads its column's lse once per tile.  A column without an
// item (grow = -1) keeps a plain product: it is never selected or counted.  The caller syncs before the tile is read.
template <class GRow>
__device__ __forceinline__ void tk_tile_norm(float* sS, const float* lse, float beta, GRow grow, int tid) {
  const int col = tid & (TK_G - 1), g = grow(col);
  const float l = g >= 0 ? lse[g] : 0.f;
  for (int row = tid >> 7; row < TK_Q; row += 2)
    sS[row * TK_SLD + col] = tk_mul_rn(beta, sS[row * TK_SLD + col]) - l;
}

// fl(a + b) as an instruction of its own, the partner of tk_mul_rn: a sum the optimiser can neither contract with the
// multiply that feeds it nor reassociate.
__device__ __forceinline__ float tk_add_rn(float a, float b) {
  float r;
  asm("v_add_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}

#define TK_POOL_MEAN 0
#define TK_POOL_MAX 1

// Query-set pooling of one score tile in place (search_pool.hip only): the block's query rows are `sets` sets of C
// consecutive rows (sets * C <= TK_Q), sRw [TK_Q] their row weights; a row whose weight is 0 takes no part.  Over the
// participating rows r0 < r1 < ... of set s, in row order:
//   mean: v = fl(rw[r0] * s_r0), then v = fl(v + fl(rw[ri] * s_ri))  -- a rounded multiply, then a rounded add
//   max : v = s_r0, then v = s_ri where s_ri > v                      -- a plain compare: the first of equal values stays
// and v lands in row s of the tile.  ONE thread per column (threads 0 .. TK_G - 1) walks the sets in ascending order: set
// s reads rows s * C .. s * C + C - 1, all >= s, and then writes row s; the rows written before, 0 .. s - 1, are below
// every row it reads, so no thread ever reads a pooled value back and no second buffer is needed.  The caller syncs
// before the tile is read.  A set without a participating row (refused by the host) would give 0.
__device__ __forceinline__ void tk_tile_pool(float* sS, const float* sRw, int C, int sets, int mode, int tid) {
  if (tid >= TK_G) return;
  // `step(v, have, w, x)`: the value after a participating row.  Rows go four at a time: their scores are read whether or
  // not they take part (past the set's end the last row again, with weight 0) and the update is a select, so the four LDS
  // reads are in flight together and the loop has no branch.
  auto walk = [&](auto step) {
    for (int s = 0; s < sets; ++s) {
      const float* col = sS + s * C * TK_SLD + tid;
      const float* wr = sRw + s * C;
      float v = 0.f;
      bool have = false;
      for (int c = 0; c < C; c += 4) {
        float w[4], x[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int cc = min(c + j, C - 1);
          w[j] = wr[cc];
          x[j] = col[cc * TK_SLD];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const bool part = c + j < C && w[j] != 0.f;
          const float nv = step(v, have, w[j], x[j]);
          v = part ? nv : v;
          have = have || part;
        }
      }
      sS[s * TK_SLD + tid] = v;
    }
  };
  if (mode == TK_POOL_MEAN)
    walk([](float v, bool have, float w, float x) {
      const float p = tk_mul_rn(w, x);
      return have ? tk_add_rn(v, p) : p;
    });
  else  // selected as integers: a float select may become v_max_f32, which treats NaN and the zeros differently
    walk([](float v, bool have, float, float x) {
      return __int_as_float(!have || x > v ? __float_as_int(x) : __float_as_int(v));
    });
}

// Item-set pooling of one score tile in place (search_itemset.hip only), tk_tile_pool along the other axis: the tile's
// columns are `sets` sets of C consecutive columns (sets * C <= TK_G), sIw [TK_G] their item weights (16-byte aligned); a
// column whose weight is 0 takes no part.  Over the participating columns g0 < g1 < ... of set s, in column order, the
// value is tk_tile_pool's (mean: a rounded multiply, then a rounded add; max: a plain compare on the integer bits), and it
// lands in column s of the row.  ONE thread per row (threads 0 .. TK_Q - 1: one wave) walks its row left to right: when it
// has consumed n columns it has finished floor(n / C) <= n sets, so every column it has written, 0 .. floor(n / C) - 1, is
// below every column it has yet to read, n .. sets * C - 1: no thread ever reads a pooled value back, rows do not meet, and
// no second buffer is needed.  (A split of one row's sets over several threads would not do: set s reads columns up to
// s * C + C - 1, into the columns a thread with higher sets writes.)  The row is read four columns at a time -- an aligned
// 16-byte read, the whole of which is in registers before the thread writes anything at or beyond its first column: with
// the 132-float row pitch eight rows cover the 32 banks, so the reads are conflict-free where 64 single-column reads of 64
// rows would meet on 8 banks; the `sets` single-column writes of a row do meet there.  The caller syncs before the tile is
// read.  A set without a participating column (refused by the host) would give 0.
__device__ __forceinline__ void tk_tile_pool_items(float* sS, const float* sIw, int C, int sets, int mode, int tid) {
  if (tid >= TK_Q) return;
  float* row = sS + tid * TK_SLD;
  const int cols = sets * C;
  auto walk = [&](auto step) {
    float v = 0.f;
    bool have = false;
    int pos = 0, s = 0;  // wave-uniform: the place inside the set, the set
    for (int c = 0; c < cols; c += 4) {
      const f32x4 x = *(const f32x4*)(row + c), w = *(const f32x4*)(sIw + c);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (c + j >= cols) break;
        const bool part = w[j] != 0.f;
        const float nv = step(v, have, w[j], x[j]);
        v = part ? nv : v;
        have = have || part;
        if (++pos == C) {
          row[s++] = v;
          pos = 0;
          v = 0.f;
          have = false;
        }
      }
    }
  };
  if (mode == TK_POOL_MEAN)
    walk([](float v, bool have, float w, float x) {
      const float p = tk_mul_rn(w, x);
      return have ? tk_add_rn(v, p) : p;
    });
  else  // selected as integers, as in tk_tile_pool
    walk([](float v, bool have, float, float x) {
      return __int_as_float(!have || x > v ? __float_as_int(x) : __float_as_int(v));
    });
}

// The per-query attribute filter (the `_where` entries of mmt_hip.h; search.py: IndexTagging, TagFilter): every stored item
// carries one 64-bit tag word, every query row three 64-bit masks (all_of, none_of, any_of), and item g is a candidate of
// row q iff tk_tag_pass(tags[g], where[q]) -- plain integer operations on bit patterns, bit 63 an ordinary bit; three zero
// masks admit every item.  It is one more term of the column liveness at selection and counting, per ROW where the subset
// and the chunk's end are per column (tk_tile_select, tk_tile_count, TkRange::tile: their WHERE forms), and never touches a
// score.  An argument block says so itself with `static constexpr bool kWhere = true`; a block that says nothing has none,
// and its kernels are the ones they were.
template <class Args, class = void>
struct TkWhere { static constexpr bool value = false; };
template <class Args>
struct TkWhere<Args, std::void_t<decltype(Args::kWhere)>> { static constexpr bool value = Args::kWhere; };

#define TK_WHERE_BYTES(rows) ((rows) * 3 * 8)  // a block's masks in LDS: [rows][3] uint64

__device__ __forceinline__ bool tk_tag_pass(uint64_t t, uint64_t all_of, uint64_t none_of, uint64_t any_of) {
  return (t & all_of) == all_of && (t & none_of) == 0ull && (any_of == 0ull || (t & any_of) != 0ull);
}

// The masks of the block's ROWS query rows -> sW [ROWS][3]; a row past NQ gets zeros (it is never live).  The caller
// syncs before they are read.
template <int ROWS>
__device__ __forceinline__ void tk_load_where(uint64_t* sW, const uint64_t* where, int NQ, int q0, int tid) {
  for (int i = tid; i < ROWS * 3; i += 256) sW[i] = q0 + i / 3 < NQ ? where[(int64_t)q0 * 3 + i] : 0ull;
}

// The tag words of the lane's two columns of the tile at g0 (column `lane` and 64 + `lane`; 0 past g_end, where the
// column is not live anyway): two loads per thread and tile, 1 KiB per wave.
__device__ __forceinline__ void tk_tile_tags(const uint64_t* tags, int g0, int g_end, int lane, uint64_t& t0, uint64_t& t1) {
  t0 = g0 + lane < g_end ? tags[g0 + lane] : 0ull;
  t1 = g0 + 64 + lane < g_end ? tags[g0 + 64 + lane] : 0ull;
}

// The same, one tile ahead: `next` hands out the tags of the tile at g0 and asks for those of the tile behind it, so the
// loads of a tile are in flight during the tile before -- a skipped tile costs no memory round trip of its own.
struct TkTagStream {
  uint64_t n0, n1;
  __device__ __forceinline__ void init(const uint64_t* tags, int g_begin, int g_end, int lane) {
    tk_tile_tags(tags, g_begin, g_end, lane, n0, n1);
  }
  __device__ __forceinline__ void next(const uint64_t* tags, int g0, int g_end, int lane, uint64_t& t0, uint64_t& t1) {
    t0 = n0;
    t1 = n1;
    tk_tile_tags(tags, g0 + TK_G, g_end, lane, n0, n1);
  }
};

__device__ __forceinline__ uint64_t tk_shfl_xor64(uint64_t x, int m) {
  return (uint64_t)(unsigned)__shfl_xor((int)x, m) | (uint64_t)(unsigned)__shfl_xor((int)(x >> 32), m) << 32;
}

// What the masks of a block's live rows have in common, formed once per block by every wave alike (lane l reads row l
// from memory, six butterfly reductions): a_and / n_and = the bits EVERY row demands / bars, y_or = the bits some row's
// any_of names, every_any = every row has an any_of.  An item that lacks a bit of a_and, has a bit of n_and, or -- where
// every row has an any_of -- has no bit of y_or passes NO row: `common` is a necessary condition, and where all rows
// carry the same three masks (uniform: the shared predicate) it is the predicate itself -- a per-COLUMN liveness like the
// subset's, which the kernels then fold into the shared liveness and run the unfiltered step.
struct TkWhereGate {
  uint64_t a_and, n_and, y_or;
  bool every_any, uniform;

  template <int ROWS>
  __device__ __forceinline__ void init(const uint64_t* where, int NQ, int q0, int lane) {
    static_assert(ROWS <= 64, "a lane per row");
    const bool live = lane < ROWS && q0 + lane < NQ;
    const uint64_t* w = where + (int64_t)(q0 + lane) * 3;
    const uint64_t a = live ? w[0] : 0ull, n = live ? w[1] : 0ull, y = live ? w[2] : 0ull;
    uint64_t aa = live ? a : ~0ull, ao = a, na = live ? n : ~0ull, no = n, ya = live ? y : ~0ull, yo = y;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      aa &= tk_shfl_xor64(aa, m); ao |= tk_shfl_xor64(ao, m);
      na &= tk_shfl_xor64(na, m); no |= tk_shfl_xor64(no, m);
      ya &= tk_shfl_xor64(ya, m); yo |= tk_shfl_xor64(yo, m);
    }
    a_and = aa; n_and = na; y_or = yo;
    every_any = __ballot(live && y == 0ull) == 0ull;
    uniform = aa == ao && na == no && ya == yo;
  }
  __device__ __forceinline__ bool common(uint64_t t) const {
    return (t & a_and) == a_and && (t & n_and) == 0ull && (!every_any || (t & y_or) != 0ull);
  }
};

// The filter's gate of a tile, exact and block-uniform: whether ANY (live row, live column) pair of the ROWS x 128 tile
// passes -- live0 / live1 the column liveness every row shares (the chunk's end, the subset's bit).  First the rows'
// common condition: the four waves hold the same 128 tags and the same column liveness, so its ballot is the same in all
// of them and decides without a barrier -- false: no pair passes; true with uniform rows: a pair passes.  Otherwise the
// pairs are spread as the selection spreads them (wave w: rows ROWS / 4 * w ..; lane: columns `lane` and 64 + `lane`), a
// wave stops at its first row with a pass, and one __syncthreads_or joins the four waves.  False: the caller skips the
// tile before its K loop, as it skips a tile without a subset bit.  Every thread of the block must arrive.
template <int ROWS>
__device__ __forceinline__ bool tk_tile_where_any(const TkWhereGate& gate, const uint64_t* sW, int rows_live, uint64_t t0,
                                                  uint64_t t1, bool live0, bool live1, int wave) {
  if (!__ballot((live0 && gate.common(t0)) || (live1 && gate.common(t1)))) return false;
  if (gate.uniform) return true;
  bool any = false;
  for (int rr = 0; rr < ROWS / 4 && !any; ++rr) {
    const int row = wave * (ROWS / 4) + rr;
    if (row >= rows_live) break;
    const uint64_t wa = sW[row * 3], wn = sW[row * 3 + 1], wy = sW[row * 3 + 2];
    any = __ballot((live0 && tk_tag_pass(t0, wa, wn, wy)) || (live1 && tk_tag_pass(t1, wa, wn, wy))) != 0ull;  // wave-uniform
  }
  return __syncthreads_or(any);
}

// The count step of one score tile (the count passes of search_rank.hip and search_pool.hip): wave w owns rows 16w .. 16w + 15
// of the tile for the whole block, so its counters need no barrier.  Per row, lane t holds threshold t of sThr [.][T]; the
// wave broadcasts one threshold at a time and counts `score > thr` / `score == thr` over the live columns (live0: column
// `lane`, live1: column 64 + `lane`) with two ballots each -- plain float compares: -0 == +0, NaN counts for nothing --
// and lane t adds the sums of threshold t to sCnt [.][T][2].  WHERE: the liveness is per row -- the shared one ANDed with
// the row's filter sW [.][3] over the lane's tags t0 / t1 (tk_tile_tags).
template <bool WHERE = false>
__device__ __forceinline__ void tk_tile_count(const float* sS, const float* sThr, int* sCnt, int T, int rows_live, bool live0,
                                              bool live1, int wave, int lane, const uint64_t* sW = nullptr, uint64_t t0 = 0,
                                              uint64_t t1 = 0) {
  for (int rr = 0; rr < TK_Q / 4; ++rr) {
    const int row = wave * (TK_Q / 4) + rr;
    if (row >= rows_live) break;
    const float s0 = sS[row * TK_SLD + lane], s1 = sS[row * TK_SLD + 64 + lane];
    const int mine = lane < T ? __float_as_int(sThr[row * T + lane]) : 0;
    bool l0 = live0, l1 = live1;
    if constexpr (WHERE) {
      const uint64_t wa = sW[row * 3], wn = sW[row * 3 + 1], wy = sW[row * 3 + 2];
      l0 = l0 && tk_tag_pass(t0, wa, wn, wy);
      l1 = l1 && tk_tag_pass(t1, wa, wn, wy);
    }
    int ng = 0, ne = 0;
    for (int t = 0; t < T; ++t) {
      const float thr = __int_as_float(__builtin_amdgcn_readlane(mine, t));
      const int cg = __popcll(__ballot(l0 && s0 > thr)) + __popcll(__ballot(l1 && s1 > thr));
      const int ce = __popcll(__ballot(l0 && s0 == thr)) + __popcll(__ballot(l1 && s1 == thr));
      if (lane == t) { ng = cg; ne = ce; }
    }
    if (lane < T) {
      sCnt[2 * (row * T + lane)] += ng;
      sCnt[2 * (row * T + lane) + 1] += ne;
    }
  }
}

// The block's counters sCnt [.][T][2] -> cnt [.][T][n_chunks][2] at its chunk; row0 = the block's first output row.
__device__ __forceinline__ void tk_count_flush(const int* sCnt, int32_t* cnt, int T, int rows_live, int row0, int n_chunks,
                                               int chunk, int wave, int lane) {
  for (int rr = 0; rr < TK_Q / 4; ++rr) {
    const int row = wave * (TK_Q / 4) + rr;
    if (row >= rows_live) break;
    if (lane < T) {
      int32_t* dst = cnt + (((int64_t)(row0 + row) * T + lane) * n_chunks + chunk) * 2;
      dst[0] = sCnt[2 * (row * T + lane)];
      dst[1] = sCnt[2 * (row * T + lane) + 1];
    }
  }
}

// The range step of one score tile (search_range.hip, search_self.hip), count and fill: lane l < 16 of wave w holds the
// state of row 16 w + l for the whole block -- its threshold, with OWN the one item it never meets (left out by NUMBER, -1 =
// none; without OWN that compare does not exist), its hits so far and, for the fill, where its slots of this chunk begin and
// how many they are -- so there is no LDS and no barrier.  Per row and tile two ballots of `live && score >= thr` (a plain
// float compare: a NaN threshold hits nothing, -inf every live item); the popcounts add up in the holder.  The fill writes a
// hit to base + (hits of the row in the block's earlier tiles) + (hits in lower columns of this tile), clamped against the
// start of the row's next chunk: a disagreement between the passes would show inside the row's own slots, never as a stray
// write.
template <bool FILL, bool OWN>
struct TkRange {
  static constexpr int kRows = TK_Q / 4;  // rows per wave
  bool holder;
  int64_t q, base;
  float thr;
  int own, cnt, cap;

  // ws [.][n_chunks]: the count pass's counts (flush), for the fill their exclusive prefix (the offsets kernel).  False
  // (FILL only, block-uniform): no row of this block has a hit in this chunk of `items` items.
  __device__ __forceinline__ bool init(const float* thrs, const int64_t* self, const int32_t* ws, const int64_t* offsets, int q0,
                                       int rows_live, int chunk, int n_chunks, int items, int wave, int lane) {
    holder = lane < kRows && wave * kRows + lane < rows_live;
    q = q0 + wave * kRows + lane;
    thr = holder ? thrs[q] : __builtin_nanf("");
    own = (OWN && holder && self) ? (int)self[q] : -1;
    cnt = cap = 0;
    base = 0;
    if constexpr (FILL) {
      if (holder) {
        const int64_t off = offsets[q];
        const int32_t* pre = ws + q * n_chunks + chunk;
        base = off + pre[0];
        const int64_t next = chunk + 1 < n_chunks ? off + pre[1] : offsets[q + 1];
        const int64_t room = next - base;  // never beyond the row's next chunk, nor more than the chunk has items
        cap = room < 0 ? 0 : room > items ? items : (int)room;
      }
      return __syncthreads_or(cap > 0);
    }
    return true;
  }

  // live0 / live1: column `lane` / 64 + `lane` of the tile at g0 holds an item that may be hit.  WHERE: by the row's filter
  // sW [.][3] as well, over the lane's tags t0 / t1 (tk_tile_tags) -- the same term in the count and in the fill.
  template <bool WHERE = false>
  __device__ __forceinline__ void tile(const float* sS, int g0, bool live0, bool live1, int rows_live, int64_t* indices,
                                       float* scores, int wave, int lane, const uint64_t* sW = nullptr, uint64_t t0 = 0,
                                       uint64_t t1 = 0) {
    const int c0 = g0 + lane, c1 = g0 + 64 + lane;
#pragma nounroll
    for (int rr = 0; rr < kRows; ++rr) {
      const int row = wave * kRows + rr;
      if (row >= rows_live) break;
      const float s0 = sS[row * TK_SLD + lane], s1 = sS[row * TK_SLD + 64 + lane];
      const float t = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(thr), rr));
      const int o = OWN ? __builtin_amdgcn_readlane(own, rr) : -1;
      bool hit0 = live0 && (!OWN || c0 != o) && s0 >= t, hit1 = live1 && (!OWN || c1 != o) && s1 >= t;
      if constexpr (WHERE) {
        const uint64_t wa = sW[row * 3], wn = sW[row * 3 + 1], wy = sW[row * 3 + 2];
        hit0 = hit0 && tk_tag_pass(t0, wa, wn, wy);
        hit1 = hit1 && tk_tag_pass(t1, wa, wn, wy);
      }
      const uint64_t b0 = __ballot(hit0), b1 = __ballot(hit1);
      const int n0 = __popcll(b0), n1 = __popcll(b1);
      if constexpr (FILL) {
        if (b0 | b1) {  // wave-uniform
          const int seen = __builtin_amdgcn_readlane(cnt, rr), room = __builtin_amdgcn_readlane(cap, rr);
          const int64_t at = (int64_t)(((uint64_t)(unsigned)__builtin_amdgcn_readlane((int)(base >> 32), rr) << 32) |
                                       (unsigned)__builtin_amdgcn_readlane((int)base, rr));
          const uint64_t below = (1ull << lane) - 1;
          const int p0 = seen + __popcll(b0 & below), p1 = seen + n0 + __popcll(b1 & below);
          if (hit0 && p0 < room) {
            indices[at + p0] = c0;
            scores[at + p0] = s0;
          }
          if (hit1 && p1 < room) {
            indices[at + p1] = c1;
            scores[at + p1] = s1;
          }
        }
      }
      if (lane == rr) cnt += n0 + n1;
    }
  }

  __device__ __forceinline__ void flush(int32_t* ws, int n_chunks, int chunk) const {
    if (holder) ws[q * n_chunks + chunk] = cnt;
  }
};

// THE similarity of two STORED items (search_diverse.hip: pair_scores_kernel; search_self.hip: sj_tile), N rows against one
// column:  sim = <f_g, f_h> / sum_m gw_g[m] gw_h[m]  (0 -> 1e-5), the denominator an explicit fma chain over m ascending
// (symmetric in its factors), with fp8 rows the numerator fl(acc * fl(scale_g * scale_h)): the product of two powers of two,
// then one rounded multiply (tk_mul_rn).  acc[r] is row r's contraction, row_w(r, m) / row_scale(r) its weights and scale,
// col_w(m) / col_scale the column's.  Not tk_tile_scores: a query's denominator is another, non-fma expression.
template <bool FP8, int N, class Acc, class RowW, class ColW, class RowS>
__device__ __forceinline__ void tk_pair_sims(float (&sim)[N], const Acc& acc, int M, RowW row_w, ColW col_w, RowS row_scale,
                                             float col_scale) {
  float den[N];
#pragma unroll
  for (int r = 0; r < N; ++r) den[r] = 0.f;
  for (int m = 0; m < M; ++m) {
    const float w = col_w(m);
#pragma unroll
    for (int r = 0; r < N; ++r) den[r] = __builtin_fmaf(row_w(r, m), w, den[r]);
  }
#pragma unroll
  for (int r = 0; r < N; ++r) {
    float num = acc[r];
    if constexpr (FP8) num = tk_mul_rn(num, tk_mul_rn(row_scale(r), col_scale));
    sim[r] = num / (den[r] == 0.f ? 1e-5f : den[r]);
  }
}

// Column statistics of one score tile for the log-sum-exp over a bank of queries (search_norm.hip only): thread c < TK_G
// takes column c and the tile's live rows 0 .. rows_live - 1 in ascending order: x = fl(beta * score), m = max x,
// p = sum exp(x - m).  The order is fixed by the row number alone, so (m, p) is a function of the 64-row bank block, the
// item and beta -- not of the launch geometry.
__device__ __forceinline__ void tk_tile_col_stats(const float* sS, float beta, int rows_live, int col, float& m, float& p) {
  m = tk_mul_rn(beta, sS[col]);
  for (int row = 1; row < rows_live; ++row) m = fmaxf(m, tk_mul_rn(beta, sS[row * TK_SLD + col]));
  p = 0.f;
  for (int row = 0; row < rows_live; ++row) p += expf(tk_mul_rn(beta, sS[row * TK_SLD + col]) - m);
}

// Whether an argument block's gallery is stored in fp8 (e4m3fn codes in g, one fp32 scale per item in gscale): a block
// says so itself with `static constexpr bool kFp8 = true`, as it says kMask and kNorm; a block that says nothing is not.
template <class Args, class = void>
struct TkFp8 { static constexpr bool value = false; };
template <class Args>
struct TkFp8<Args, std::void_t<decltype(Args::kFp8)>> { static constexpr bool value = Args::kFp8; };

// One 64 x 128 tile of scores in sS: the K loop, the gated-denominator epilogue and, with NORM, the querybank rewrite to
// score'.  Ends fenced.  `a` is any of the scans' argument blocks (q, q_lo for BF16, g, gw, NQ, K, M; lse and beta for
// NORM; gscale for an fp8 gallery, which takes the BF16 query operands, LDS footprint and MFMA loop).
template <bool BF16, bool NORM, class Args, class GRow>
__device__ __forceinline__ void tk_tile(const Args& a, unsigned char* smem, float* sS, const float* sQw, int q0, GRow grow,
                                        int tid, int wq, int wg, int l31, int h) {
  constexpr bool FP8 = TkFp8<Args>::value;
  static_assert(!FP8 || BF16, "an fp8 gallery is scanned with the bf16 query pair");
  f32x16 acc[2];
  const int NQ = a.NQ;
  const auto qrow = [=](int r) { return q0 + r < NQ ? q0 + r : -1; };
  if constexpr (BF16)  // the query as two bf16 planes, hi then lo
    tk_scan(acc, smem, {(const bf16_t*)a.q, (const bf16_t*)a.q_lo}, qrow, (const std::conditional_t<FP8, uint8_t, bf16_t>*)a.g,
            grow, a.K, tid, wq, wg, l31, h);
  else
    tk_scan(acc, smem, {(const float*)a.q}, qrow, (const float*)a.g, grow, a.K, tid, wq, wg, l31, h);
  __syncthreads();  // the slabs become the score tile
  if constexpr (FP8)
    tk_tile_scores<true>(acc, sS, sQw, a.gw, a.M, grow, wq, wg, l31, h, a.gscale);
  else
    tk_tile_scores(acc, sS, sQw, a.gw, a.M, grow, wq, wg, l31, h);
  __syncthreads();
  if constexpr (NORM) {
    tk_tile_norm(sS, a.lse, a.beta, grow, tid);
    __syncthreads();
  }
}

// How a subset bitmap (search_subset.hip: bit g & 31 of word g >> 5 allows item g) enters a scan kernel: not at all, as a
// compile-time fact, or as a pointer that may be null (= every item allowed).  An argument block says so itself, in
// kMask, and in kNorm whether its kernels score the querybank-normalised score': the kernels are generic over the block.
enum TkMask { TK_MASK_NONE, TK_MASK_SET, TK_MASK_NULLABLE };

// The subset gate of the tile at g0 (a multiple of 128): its four mask words are one block-uniform 16-byte load; m0 holds
// columns 0 .. 63, m1 columns 64 .. 127.  False = no bit set: the caller skips the tile before its K loop.
__device__ __forceinline__ bool tk_tile_mask(const uint32_t* subset, int g0, uint64_t& m0, uint64_t& m1) {
  const u32x4 w = *(const u32x4*)(subset + (g0 >> 5));
  m0 = w[0] | (uint64_t)w[1] << 32;
  m1 = w[2] | (uint64_t)w[3] << 32;
  return m0 | m1;
}

// The subset gate of a tile whose first column stands for number t0 of the bitmap, t0 any value (search_itemset.hip: a
// tile's sets start wherever the tile before ended): bits t0 .. t0 + n - 1 of the bitmap (n <= 128 live columns) come from
// up to five block-uniform words, funnel-shifted by t0 & 31; a word at or past n_words (the bitmap's length: 4 words per
// 128 numbers) is not read.  m0 / m1 as tk_tile_mask, bits n .. 127 cleared, so false = none of the tile's own columns is
// allowed.
__device__ __forceinline__ bool tk_tile_mask_window(const uint32_t* subset, int n_words, int t0, int n, uint64_t& m0,
                                                    uint64_t& m1) {
  const int w0 = t0 >> 5, sh = t0 & 31;
  uint32_t w[5], o[4];
#pragma unroll
  for (int i = 0; i < 5; ++i) w[i] = w0 + i < n_words ? subset[w0 + i] : 0u;
#pragma unroll
  for (int i = 0; i < 4; ++i) o[i] = (uint32_t)((((uint64_t)w[i + 1] << 32) | w[i]) >> sh);
  m0 = o[0] | (uint64_t)o[1] << 32;
  m1 = o[2] | (uint64_t)o[3] << 32;
  if (n < 64) { m0 &= (1ull << n) - 1ull; m1 = 0; }
  else if (n < 128) m1 &= (1ull << (n - 64)) - 1ull;
  return m0 | m1;
}

// The operands of the querybank scans; the argument blocks of the normalised top-k (search.hip) and rank kernels
// (search_rank.hip) extend it.
struct NmArgs {
  const void* q;        // fp32: Q' [NQ][K]; bf16: hi(Q')
  const void* q_lo;     // bf16: lo(Q')
  const float* qw;      // [NQ][M]
  const void* g;        // [NV][K] fp32 or bf16 bits
  const float* gw;      // [NV][M]
  const float* lse;     // [NV] (the lse pass: unused)
  float beta;
  int NQ, NV, M, K, chunk, n_qt, n_chunks;
  static constexpr TkMask kMask = TK_MASK_NULLABLE;
  static constexpr bool kNorm = true;
};

// Host side.  Gallery columns per block (search.hip): TK_CHUNK halved (down to one tile) while the launch would not fill
// the chip.
int tk_chunk(int NQ, int NV);

// The chunk reduce of the count passes (search_rank.hip): cnt [n][n_chunks][2] summed in chunk order.
int rk_reduce_launch(const int32_t* cnt, int64_t n, int n_chunks, int32_t* greater, int32_t* equal, hipStream_t s);

// The offsets kernel between the count and the fill pass of a range scan (search_range.hip): one thread per row turns
// ws [R][n_chunks] into the row's exclusive prefix in place, in chunk order, and writes the row total as int64.
int rg_offsets_launch(int32_t* ws, int R, int n_chunks, int64_t* row_counts, hipStream_t s);

inline int tk_n_chunks(int NQ, int NV) {
  const int chunk = tk_chunk(NQ, NV);
  return (NV + chunk - 1) / chunk;
}

// int32 words of a range scan's workspace [NQ][n_chunks].
inline int64_t tk_range_workspace_ints(int NQ, int NV) {
  return NQ < 1 || NV < 1 ? (int64_t)MMT_ERR_ARG : (int64_t)NQ * tk_n_chunks(NQ, NV);
}

// The launch geometry of a scan over a.NQ queries and a.NV items: grid = n_qt * n_chunks blocks.
template <class Args>
void tk_geometry(Args& a) {
  a.chunk = tk_chunk(a.NQ, a.NV);
  a.n_qt = (a.NQ + TK_Q - 1) / TK_Q;
  a.n_chunks = (a.NV + a.chunk - 1) / a.chunk;
}

// The shape gate of every scan entry point: folded rows are 16 bytes times a whole number (d % 4 fp32, d % 8 bf16,
// d % 16 fp8).
inline bool tk_shape_ok(int NQ, int NV, int M, int d, bool bf16, bool fp8 = false) {
  return NQ > 0 && NV > 0 && M > 0 && M <= MMT_MAX_EXPERTS && d > 0 && !(d & (fp8 ? 15 : bf16 ? 7 : 3));
}

inline bool tk_beta_ok(float beta) { return beta > 0.f && std::isfinite(beta); }

template <bool BF16>
constexpr size_t tk_base_lds() { return (BF16 ? TKB_UNION_BYTES : TK_UNION_BYTES) + TK_QW_BYTES; }

// Raises the dynamic-LDS limit of kernels whose footprint can pass the 64 KiB default, once on every device they are
// launched on: a function attribute belongs to the device that is current when it is set, and a gallery cut into shards
// launches on several.  `done` is the caller's table (static, zeroed), one per group of kernels.  Two threads meeting here
// set the same values twice.
struct TkLdsLimit { const void* kernel; size_t bytes; };
inline void tk_lds_limits(bool (&done)[64], std::initializer_list<TkLdsLimit> kernels) {
  int dev = -1;
  const bool known = hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 64;  // beyond the table: set every time
  if (known && done[dev]) return;
  for (const TkLdsLimit& k : kernels)
    (void)hipFuncSetAttribute(k.kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)k.bytes);
  if (known) done[dev] = true;
}

// The descriptor of a scan (mmt_hip.h: MmtSearchScan) on the host.  Its optional parts as bits: what an entry point says
// it has kernels for, and what its dispatch to a body's template arguments switches on.
enum : unsigned { SC_SUBSET = 1, SC_EXCLUDE = 2, SC_AFTER = 4, SC_NORM = 8, SC_QSETS = 16, SC_ISETS = 32, SC_FP8 = 64 };

inline unsigned tk_scan_parts(const MmtSearchScan& s) {
  return (s.subset ? SC_SUBSET : 0) | (s.exclude || s.E ? SC_EXCLUDE : 0) | (s.after ? SC_AFTER : 0) |
         (s.lse || s.beta != 0.f ? SC_NORM : 0) | (s.sets == MMT_SEARCH_SETS_QUERY ? SC_QSETS : 0) |
         (s.sets == MMT_SEARCH_SETS_ITEM ? SC_ISETS : 0) | (s.storage == MMT_SEARCH_FP8 ? SC_FP8 : 0);
}

// The gate every scan entry point opens with: 0, or MMT_ERR_ARG for a null descriptor, an unknown tag, a part outside
// `takes` (what the operation has kernels for), a combination no kernel exists for, or a field set whose part is absent.
inline int tk_scan_gate(const MmtSearchScan* s, unsigned takes) {
  if (!s || (unsigned)s->storage > MMT_SEARCH_FP8 || (unsigned)s->sets > MMT_SEARCH_SETS_ITEM) return MMT_ERR_ARG;
  const unsigned p = tk_scan_parts(*s), sets = p & (SC_QSETS | SC_ISETS);
  if (p & ~takes) return MMT_ERR_ARG;
  if ((p & SC_FP8) && (p & SC_NORM || sets)) return MMT_ERR_ARG;
  if (sets && (p & (SC_NORM | SC_EXCLUDE | SC_AFTER))) return MMT_ERR_ARG;
  if ((s->storage == MMT_SEARCH_FP32 && s->q_lo) || (!(p & SC_FP8) && s->gscale)) return MMT_ERR_ARG;
  if (!sets && (s->set_size || s->mode || s->set_weights)) return MMT_ERR_ARG;
  return 0;
}

// The operands a body with these template arguments reads are all there (the norm's beta in range).
template <bool BF16, bool FP8 = false, bool NORM = false>
bool tk_scan_operands(const MmtSearchScan& s) {
  return s.q && (!BF16 || s.q_lo) && s.qw && s.g && s.gw && (!FP8 || s.gscale) && (!NORM || (s.lse && tk_beta_ok(s.beta)));
}

// Query rows, gallery rows and subset words on 16-byte boundaries (null is aligned).
inline bool tk_scan_aligned(const MmtSearchScan& s) {
  return !(((uintptr_t)s.q | (uintptr_t)s.q_lo | (uintptr_t)s.g | (uintptr_t)s.subset) & 15);
}

// The scans of a gallery or of queries in sets (search_pool.hip, search_itemset.hip) behind mmt_search_topk,
// mmt_search_thresholds and mmt_search_count: the descriptor has passed tk_scan_gate and carries that kind of sets.
int pl_topk(const MmtSearchScan& s, int k, uint64_t* ws, float* scores, int64_t* index, void* stream);
int pl_thresholds(const MmtSearchScan& s, const int64_t* targets, int T, float* thr, void* stream);
int pl_count(const MmtSearchScan& s, const float* thr, int T, int32_t* ws, int32_t* greater, int32_t* equal, void* stream);
int is_topk(const MmtSearchScan& s, int k, uint64_t* ws, float* scores, int64_t* index, void* stream);
int is_thresholds(const MmtSearchScan& s, const int64_t* targets, int T, float* thr, void* stream);
int is_count(const MmtSearchScan& s, const float* thr, int T, int32_t* ws, int32_t* greater, int32_t* equal, void* stream);
