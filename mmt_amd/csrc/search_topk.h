// Selection machinery of the top-k search (search.hip; the shard merge of search_shard.hip shares the key): the
// (score, index) key and the per-row running top-k in LDS.  The scoring tile itself (K loops, score epilogue, chunk rule)
// is search_scan.h.  See search.hip for the algorithm.
#pragma once
#include "search_scan.h"

#define TK_MAXK 128
#define TK_MAXE 32  // per-query exclusions of the masked instantiations

__device__ __forceinline__ uint64_t tk_key(float s, int idx) {
  unsigned u = __float_as_uint(s);
  if (!(u & 0x7fffffffu)) u = 0;  // -0 ranks as +0 (numpy compares them equal)
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ((uint64_t)u << 32) | (uint64_t)(~(unsigned)idx);
}
__device__ __forceinline__ float tk_score(uint64_t key) {
  const unsigned u = (unsigned)(key >> 32);
  return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
}
__device__ __forceinline__ int tk_index(uint64_t key) { return (int)~(unsigned)key; }

// Whether an argument block carries a cursor per query row (`after`: uint64 bounds [NQ], tk_tile_select<., true>): a block
// says so itself with `static constexpr bool kAfter = true`, as TkFp8; a block that says nothing does not.
template <class Args, class = void>
struct TkAfter { static constexpr bool value = false; };
template <class Args>
struct TkAfter<Args, std::void_t<decltype(Args::kAfter)>> { static constexpr bool value = Args::kAfter; };

// One wave, one row: rank-sort the n (<= k + 64 <= 192) candidates c[0..n) and keep the best min(n, k) in c[0..) in
// descending order.
__device__ __forceinline__ void tk_compact(uint64_t* c, int n, int k, int lane) {
  uint64_t v[3];
  int rk[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int i = lane + 64 * j;
    v[j] = i < n ? c[i] : 0;
    rk[j] = 0;
  }
  for (int i = 0; i < n; ++i) {
    const uint64_t x = c[i];
#pragma unroll
    for (int j = 0; j < 3; ++j) rk[j] += x > v[j];
  }
  __builtin_amdgcn_wave_barrier();  // every lane's reads above precede any rewrite (one wave: LDS ops stay in order)
#pragma unroll
  for (int j = 0; j < 3; ++j)
    if (lane + 64 * j < n && rk[j] < k) c[rk[j]] = v[j];
  __builtin_amdgcn_wave_barrier();
}

// One wave, one row: offers one key per lane (0 = none).  Keys at or below the threshold (the k-th best so far) cannot
// enter the top k; the others are appended.  Capacity k + 64: the list is compacted first whenever it holds more than k.
// AFTER: keys at or above `bound` (the row's cursor, tk_tile_select) are declined as well.
template <bool AFTER = false>
__device__ __forceinline__ void tk_push(uint64_t* c, int& n, uint64_t& thr, int k, uint64_t key, int lane,
                                        uint64_t bound = ~0ull) {
  if (n > k) {
    tk_compact(c, n, k, lane);
    n = k;
    thr = c[k - 1];
  }
  bool take = key > thr;
  if constexpr (AFTER) take = take && key < bound;
  const uint64_t mask = __ballot(take);
  if (take) c[n + __popcll(mask & ((1ull << lane) - 1ull))] = key;
  n += __popcll(mask);
}

// The chunk's best min(n, k) keys of one row, sorted, padded with 0 to k.
__device__ __forceinline__ void tk_flush(uint64_t* c, int n, int k, int lane, uint64_t* dst) {
  if (n > 0) tk_compact(c, n, k, lane);
  const int have = n < k ? n : k;
  for (int j = lane; j < k; j += 64) dst[j] = j < have ? c[j] : 0ull;
}

// Selection over the score tile: wave w owns rows 16w .. 16w + 15 (ROWS / 4 of them); columns in increasing index order.  MASKED: only the
// columns whose bit is set in m0 (columns 0 .. 63) / m1 (64 .. 127) are candidates, less the row's exclusions sEx[row][E]
// (item numbers, -1 = none; lane e holds exclusion e, and the few that fall into this tile clear their bit).  The score
// tile is the unmasked kernel's, so a returned score has the bits the unmasked search gives that item.  AFTER (the paged
// search: the argument blocks with kAfter): sB [TK_Q] holds one bound per row, a position in the search's order, and only
// keys strictly below it are candidates: 2^64 - 1 = no cursor (no score gives that key), 0 = the row is exhausted, and
// tk_key(a, first) + 1 = everything that scores below a, and at score a the items from number `first` on.  ROWS: the rows of
// the block's score tile, a quarter per wave (TK_Q, or the streaming schedule's 32: search_stream.hip).  WHERE (the
// per-query attribute filter: search_scan.h, tk_tag_pass): sW [ROWS][3] holds the rows' masks and t0 / t1 the tag words of
// the lane's two columns (tk_tile_tags), loaded once per tile outside the row loop; a column is a candidate of a row only
// if its tags pass the row's masks -- one more term of `live`, per row.
template <bool MASKED = false, bool AFTER = false, int ROWS = TK_Q, bool WHERE = false>
__device__ __forceinline__ void tk_tile_select(const float* sS, uint64_t* sC, int* sN, uint64_t* sT, int k, int rows_live,
                                               int g0, int g_end, int wave, int lane, uint64_t m0 = 0, uint64_t m1 = 0,
                                               const int* sEx = nullptr, int E = 0, const uint64_t* sB = nullptr,
                                               const uint64_t* sW = nullptr, uint64_t t0 = 0, uint64_t t1 = 0) {
  const int cap = k + 64;
  for (int rr = 0; rr < ROWS / 4; ++rr) {
    const int row = wave * (ROWS / 4) + rr;
    if (row >= rows_live) break;
    int n = sN[row];
    uint64_t thr = sT[row];
    uint64_t bound = ~0ull;
    if constexpr (AFTER) bound = sB[row];
    uint64_t a0 = m0, a1 = m1;
    uint64_t wa = 0, wn = 0, wy = 0;
    if constexpr (WHERE) { wa = sW[row * 3]; wn = sW[row * 3 + 1]; wy = sW[row * 3 + 2]; }
    if constexpr (MASKED) {
      if (E) {
        const int mine = lane < E ? sEx[row * E + lane] : -1;
        uint64_t hit = __ballot(mine >= g0 && mine < g0 + TK_G);
        while (hit) {  // wave-uniform: one pass per exclusion inside this tile
          const int c = __builtin_amdgcn_readlane(mine, __ffsll((unsigned long long)hit) - 1) - g0;
          hit &= hit - 1;
          if (c < 64) a0 &= ~(1ull << c);
          else a1 &= ~(1ull << (c - 64));
        }
      }
    }
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const int col = half * 64 + lane, g = g0 + col;
      bool live = g < g_end;
      if constexpr (MASKED) live = live && (((half ? a1 : a0) >> lane) & 1ull);
      if constexpr (WHERE) live = live && tk_tag_pass(half ? t1 : t0, wa, wn, wy);
      tk_push<AFTER>(sC + row * cap, n, thr, k, live ? tk_key(sS[row * TK_SLD + col], g) : 0ull, lane, bound);
    }
    if (lane == 0) { sN[row] = n; sT[row] = thr; }
  }
}

// Host side (search.hip): the merge launch over the workspace of a chunk scan -- NQ rows of n_chunks sorted lists of k
// keys -> the best kout per row.
int tk_merge_launch(const uint64_t* ws, int NQ, int n_chunks, int k, int kout, float* scores, int64_t* index, hipStream_t s);
