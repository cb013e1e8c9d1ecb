// Grouped search without the N_query x N_gallery matrix: the k best GROUPS of a gallery whose items carry a group id (the
// clips of a video, the captions of a video), each reported with its best item -- Milvus "grouping search", Qdrant "search
// groups", Elasticsearch field collapsing.  groups[g] (int32, any labelling, ids need not be dense or contiguous) is the
// group of item g.  Per query:
//   representative of a group = its member with the largest key (search_topk.h: score descending, -0 tied with +0, equal
//   scores by ascending item); groups are ranked by their representatives' keys; slot j = the j-th best group, its
//   representative and that item's score (the bits `mmt_search_topk` gives the pair).
// It cannot be composed from the plain top-k: one group's items push other groups' representatives out of a list before
// anybody could remove them, so the de-duplication is inside the running list and again where lists merge.
//
//   group_scan_kernel<BF16> : the block of topk_scan_kernel (search.hip) -- 64 queries x one gallery chunk, tk_tile of
//                             search_scan.h per 128-column tile, the masked tile skip (tk_tile_mask) for a subset -- with a
//                             running list of the best k DISTINCT groups per row.  A key enters if it is above the
//                             threshold, as there.  A compaction (gk_compact) first drops every candidate for which the
//                             list holds a larger key of the same group, then rank-sorts the survivors; the row then holds
//                             min(survivors, k) keys, and the threshold becomes the k-th key only when k survivors exist
//                             (otherwise it stays 0: c[k - 1] would be a stale slot).  The chunk's best distinct groups go
//                             to the workspace of mmt_topk_workspace_keys, sorted and zero-padded.
//   group_merge_kernel      : one wave per query merges the chunk lists: the lists' heads are popped in descending key
//                             order (lane l holds the heads of lists l, l + 64, ...; a wave-wide max picks the next), a
//                             popped key whose group is already in the output is the lesser duplicate and is dropped,
//                             until kout groups are out or the lists' first kout positions are used up.  The remaining
//                             slots get (-inf, -1, -1).
//   group_shard_merge_kernel: the same selection over S shard lists of (score, shard-local item, group), keyed by the GLOBAL
//                             item number (search_shard.hip), so a group with members on several shards is reported once.
//
// Why the threshold is safe.  It is the k-th best of k distinct groups' best keys seen so far.  A key at or below it either
// belongs to one of those k groups -- then the list holds a larger key of its group and it is the lesser duplicate -- or
// it ranks below k other groups; neither can be in the chunk's answer.  Once set it only rises: the k listed groups stay
// in the row, so every later compaction has at least k survivors.
// Why per-chunk lists suffice.  A group in the global top k is in the top k groups of the chunk that holds its
// representative: were it not, that chunk alone would have k groups with a better key than the representative, so k better
// groups overall.  The same holds for a shard, and for the first kout positions of a list in the merges.
// Why popping is the merge.  Popped keys descend, so the first key popped of a group is its best key in all lists, i.e. its
// representative, and the groups come out in rank order.  The flat test "no other list holds a larger key of my group"
// costs a key its rank in group compares (lists are sorted by key, not by group); popping stops after kout groups, at
// most kout * n_lists pops since a list holds a group once.
//
// LDS at k = 128: the candidate list [64][k + 64] keys is 96 KiB beside the score tile, so there is no second array of group
// ids.  A candidate's group is gathered from the int32 table when its row is compacted (at most 3 per lane, held in
// registers, broadcast with readlane in the de-duplication loop).  No atomics, one writer per slot: bit-reproducible.
#include "search_topk.h"

struct GpArgs {
  const void* q;            // fp32: Q' [NQ][K]; bf16: hi(Q')
  const void* q_lo;         // bf16: lo(Q')
  const float* qw;          // [NQ][M]
  const void* g;            // [NV][K] fp32 or bf16 bits
  const float* gw;          // [NV][M]
  const int32_t* groups;    // [NV] group of item g, >= 0
  const uint32_t* subset;   // bit g & 31 of word g >> 5 allows item g (nullable = all; 16-byte aligned)
  uint64_t* ws;             // [NQ][n_chunks][k]
  int NQ, NV, M, K, k, chunk, n_qt, n_chunks;
};

// One wave, one row: of the n (wave-uniform, <= k + 64 <= 192) candidates c[0..n) drop every key for which c holds a larger
// key of the same group, rank-sort the survivors and keep the best min(survivors, k) in c[0..) in descending order.
// Returns the number of survivors (= distinct groups among the candidates).
__device__ __forceinline__ int gk_compact(uint64_t* c, int n, int k, int lane, const int32_t* __restrict__ groups) {
  uint64_t v[3];
  int gid[3], rk[3];
  bool dead[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int i = lane + 64 * j;
    v[j] = i < n ? c[i] : 0;
    gid[j] = i < n ? groups[tk_index(v[j])] : -1;  // -1 matches no candidate's group
    dead[j] = false;
    rk[j] = 0;
  }
#pragma unroll
  for (int j2 = 0; j2 < 3; ++j2) {
    const int m = min(64, n - 64 * j2);
    for (int i = 0; i < m; ++i) {
      const uint64_t x = c[64 * j2 + i];
      const int gx = __builtin_amdgcn_readlane(gid[j2], __builtin_amdgcn_readfirstlane(i));
#pragma unroll
      for (int j = 0; j < 3; ++j) dead[j] |= gx == gid[j] && x > v[j];
    }
  }
  int survivors = n;
#pragma unroll
  for (int j = 0; j < 3; ++j) survivors -= __popcll(__ballot(dead[j]));
  __builtin_amdgcn_wave_barrier();  // every lane's reads above precede the rewrite (one wave: LDS ops stay in order)
#pragma unroll
  for (int j = 0; j < 3; ++j)
    if (dead[j]) {
      c[lane + 64 * j] = 0;
      v[j] = 0;
    }
  __builtin_amdgcn_wave_barrier();
  for (int i = 0; i < n; ++i) {  // a dropped key is 0 by now and outranks nothing
    const uint64_t x = c[i];
#pragma unroll
    for (int j = 0; j < 3; ++j) rk[j] += x > v[j];
  }
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int j = 0; j < 3; ++j)
    if (v[j] && rk[j] < k) c[rk[j]] = v[j];
  __builtin_amdgcn_wave_barrier();
  return survivors;
}

// tk_push with the de-duplicating compaction: n is wave-uniform.  The threshold is the k-th key only when k distinct
// groups are listed.
__device__ __forceinline__ void gk_push(uint64_t* c, int& n, uint64_t& thr, int k, uint64_t key, int lane,
                                        const int32_t* __restrict__ groups) {
  if (n > k) {
    const int survivors = gk_compact(c, n, k, lane, groups);
    n = survivors < k ? survivors : k;
    if (survivors >= k) thr = c[k - 1];
  }
  const bool take = key > thr;
  const uint64_t mask = __ballot(take);
  if (take) c[n + __popcll(mask & ((1ull << lane) - 1ull))] = key;
  n += __popcll(mask);
}

// One block of the grouped scan: 64 queries x one gallery chunk -> per query the chunk's best min(distinct groups, k)
// representatives' keys, sorted, zero-padded to k, in the workspace.
template <bool BF16>
__global__ __launch_bounds__(256) void group_scan_kernel(GpArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int kUnion = BF16 ? TKB_UNION_BYTES : TK_UNION_BYTES;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int bid = xcd_remap(blockIdx.x, gridDim.x);  // gallery-chunk-major: an XCD's blocks share their chunk in L2
  const int chunk = bid / a.n_qt, q0 = (bid % a.n_qt) * TK_Q;
  const int g_begin = chunk * a.chunk, g_end = min(a.NV, g_begin + a.chunk);
  const int k = a.k, cap = k + 64, rows_live = a.NQ - q0;
  uint64_t* ws = a.ws + chunk * (int64_t)k;
  const int64_t ws_row = (int64_t)a.n_chunks * k;

  float* sS = (float*)smem;                                   // [TK_Q][TK_SLD]  scores (after the K loop)
  float* sQw = (float*)(smem + kUnion);                       // [TK_Q][MMT_MAX_EXPERTS]
  int* sN = (int*)(smem + kUnion + TK_QW_BYTES);              // [TK_Q] candidates held
  uint64_t* sT = (uint64_t*)(sN + TK_Q);                      // [TK_Q] thresholds
  uint64_t* sC = sT + TK_Q;                                   // [TK_Q][cap] candidates
  const int l31 = lane & 31, h = lane >> 5, wq = wave >> 1, wg = wave & 1;
  if (tid < TK_Q) { sN[tid] = 0; sT[tid] = 0; }
  tk_load_qw(sQw, a.qw, a.NQ, a.M, q0, tid);
  for (int g0 = g_begin; g0 < g_end; g0 += TK_G) {
    uint64_t m0 = ~0ull, m1 = ~0ull;
    if (a.subset && !tk_tile_mask(a.subset, g0, m0, m1)) continue;  // block-uniform: nothing of this tile is allowed
    tk_tile<BF16, false>(a, smem, sS, sQw, q0, [=](int r) { return g0 + r < g_end ? g0 + r : -1; }, tid, wq, wg, l31, h);
    // selection: wave w owns rows 16w .. 16w + 15; columns in increasing item order
    for (int rr = 0; rr < TK_Q / 4; ++rr) {
      const int row = wave * (TK_Q / 4) + rr;
      if (row >= rows_live) break;
      int n = __builtin_amdgcn_readfirstlane(sN[row]);
      uint64_t thr = sT[row];
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        const int col = half * 64 + lane, g = g0 + col;
        const bool live = g < g_end && (((half ? m1 : m0) >> lane) & 1ull);
        gk_push(sC + row * cap, n, thr, k, live ? tk_key(sS[row * TK_SLD + col], g) : 0ull, lane, a.groups);
      }
      if (lane == 0) { sN[row] = n; sT[row] = thr; }
    }
  }
  __syncthreads();
  for (int rr = 0; rr < TK_Q / 4; ++rr) {
    const int row = wave * (TK_Q / 4) + rr, q = q0 + row;
    if (row >= rows_live) break;
    uint64_t* c = sC + row * cap;
    const int n = __builtin_amdgcn_readfirstlane(sN[row]);
    int have = 0;
    if (n > 0) {  // candidates pushed since the last compaction may repeat a listed group
      const int survivors = gk_compact(c, n, k, lane, a.groups);
      have = survivors < k ? survivors : k;
    }
    uint64_t* dst = ws + q * ws_row;
    for (int j = lane; j < k; j += 64) dst[j] = j < have ? c[j] : 0ull;
  }
}

// The lists of one query as the merges see them: list c's key j is keys[c * stride + j] (descending, distinct groups, 0 =
// none, zeros last); its group is grp[c * stride + j] where grp is given, else table[item of the key].
struct GmLists {
  const uint64_t* keys;
  const int32_t* grp;
  const int32_t* table;
  int stride;
};

template <bool TABLE>
__device__ __forceinline__ int gm_group(const GmLists& L, int c, int j, uint64_t key) {
  if constexpr (TABLE) return L.table[tk_index(key)];
  else return L.grp[c * L.stride + j];
}

__device__ __forceinline__ uint64_t gm_wave_max(uint64_t x) {
#pragma unroll
  for (int s = 32; s; s >>= 1) {
    const uint64_t y = __shfl_xor((unsigned long long)x, s);
    x = y > x ? y : x;
  }
  return ((uint64_t)(unsigned)__builtin_amdgcn_readfirstlane((int)(x >> 32)) << 32) |
         (unsigned)__builtin_amdgcn_readfirstlane((int)x);
}

// The winner's next head: list bc moves one step on, the lane's other lists are searched for their first key below m.
template <bool TABLE>
__device__ __forceinline__ void gm_advance(const GmLists& L, int n_lists, int lim, int lane, uint64_t m, uint64_t& bk, int& bc,
                                           int& bp, int& bg) {
  uint64_t nk = 0;
  int nc = -1, np = 0;
  for (int c = lane; c < n_lists; c += 64) {
    const uint64_t* l = L.keys + c * L.stride;
    int p = bp + 1;
    if (c != bc) {
      int lo = 0, hi = lim;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (l[mid] >= m) lo = mid + 1;
        else hi = mid;
      }
      p = lo;
    }
    const uint64_t key = p < lim ? l[p] : 0ull;
    if (key > nk) { nk = key; nc = c; np = p; }
  }
  bk = nk; bc = nc; bp = np;
  bg = bk ? gm_group<TABLE>(L, bc, bp, bk) : -1;
}

// One wave, one query: pops the heads of n_lists lists (their first lim positions) in descending key order and writes the
// first kout keys whose group is new, then (-inf, -1, -1).  Lane l keeps the best head among lists l, l + 64, ...: its key,
// list, position and group.  The lists carry no cursor: everything above the key popped last has been popped, so the head
// of a list is its first key below that one (one step on for the list just popped, a binary search for the lane's others).
template <bool TABLE>
__device__ __forceinline__ void gm_select(const GmLists& L, int n_lists, int lim, int kout, int lane, float* scores,
                                          int64_t* out_groups, int64_t* out_items) {
  uint64_t bk = 0;
  int bc = -1, bp = 0;
  for (int c = lane; c < n_lists; c += 64) {
    const uint64_t key = L.keys[c * L.stride];
    if (key > bk) { bk = key; bc = c; }
  }
  int bg = bk ? gm_group<TABLE>(L, bc, 0, bk) : -1;
  uint64_t ok[2] = {0, 0};  // lane l holds output slots l and l + 64
  int og[2] = {-1, -1};
  int cnt = 0;
  uint64_t m = gm_wave_max(bk);
  while (m && cnt < kout) {  // m = 0: every list is used up
    const int w = __ffsll((unsigned long long)__ballot(bk == m)) - 1;  // keys are distinct: one lane
    const int g = __builtin_amdgcn_readlane(bg, w);
    const bool fresh = !(__ballot(og[0] == g) | __ballot(og[1] == g));  // wave-uniform; g >= 0 matches no unused slot
    if (fresh && lane == (cnt & 63)) {
      ok[cnt >> 6] = m;
      og[cnt >> 6] = g;
    }
    cnt += fresh;
    if (lane == w) gm_advance<TABLE>(L, n_lists, lim, lane, m, bk, bc, bp, bg);
    m = gm_wave_max(bk);
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int slot = lane + 64 * j;
    const bool has = slot < cnt;
    if (slot < kout) {
      scores[slot] = has ? tk_score(ok[j]) : -__builtin_inff();
      out_groups[slot] = has ? (int64_t)og[j] : (int64_t)-1;
      out_items[slot] = has ? (int64_t)tk_index(ok[j]) : (int64_t)-1;
    }
  }
}

// One wave per query: the n_chunks chunk lists of k keys -> the best kout distinct groups.  stage: the lists' first lim keys
// and their groups fit in LDS; otherwise they are read where they are.
__global__ __launch_bounds__(64) void group_merge_kernel(const uint64_t* __restrict__ ws, const int32_t* __restrict__ groups,
                                                         int n_chunks, int k, int kout, int stage, float* __restrict__ scores,
                                                         int64_t* __restrict__ out_groups, int64_t* __restrict__ out_items) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int q = blockIdx.x, lane = threadIdx.x, lim = min(k, kout);
  const uint64_t* mine = ws + (int64_t)q * n_chunks * k;
  const GmLists L = {mine, nullptr, groups, k};
  if (stage) {
    const int n = n_chunks * lim;
    uint64_t* sK = (uint64_t*)smem;  // [n_chunks][lim]
    int32_t* sG = (int32_t*)(sK + n);
    for (int i = lane; i < n; i += 64) {
      const uint64_t key = mine[(i / lim) * k + i % lim];
      sK[i] = key;
      sG[i] = key ? groups[tk_index(key)] : -1;
    }
    __syncthreads();
    const GmLists S = {sK, sG, nullptr, lim};
    gm_select<false>(S, n_chunks, lim, kout, lane, scores + (int64_t)q * kout, out_groups + (int64_t)q * kout,
                     out_items + (int64_t)q * kout);
    return;
  }
  gm_select<true>(L, n_chunks, lim, kout, lane, scores + (int64_t)q * kout, out_groups + (int64_t)q * kout,
                  out_items + (int64_t)q * kout);
}

#define GS_MAXS 32

struct GsArgs {
  const float* scores;        // [S][NQ][kin]
  const int64_t* groups;      // [S][NQ][kin] group of the entry
  const int64_t* index;       // [S][NQ][kin] shard-local item, -1 = empty slot
  const int64_t* const* ids;  // [S] pointers to tables on this device: local -> global item number (< 2^31)
  float* out_scores;          // [NQ][kout]
  int64_t* out_groups;        // [NQ][kout]
  int64_t* out_items;         // [NQ][kout] global item numbers
  int S, NQ, kin, kout;
};

// One wave per query: the S shard lists become keys of the global item number in LDS (48 KiB at S = 32, kin = 128), then
// the selection of group_merge_kernel.  A shard's table is increasing, so its list is best-first under the global order.
__global__ __launch_bounds__(64) void group_shard_merge_kernel(GsArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int q = blockIdx.x, lane = threadIdx.x, kin = a.kin, n = a.S * kin;
  uint64_t* sK = (uint64_t*)smem;  // [S][kin]
  int32_t* sG = (int32_t*)(sK + n);
  for (int i = lane; i < n; i += 64) {
    const int c = i / kin, j = i - c * kin;
    const int64_t at = ((int64_t)c * a.NQ + q) * kin + j;
    const int64_t local = a.index[at];
    sK[i] = local >= 0 ? tk_key(a.scores[at], (int)a.ids[c][local]) : 0ull;
    sG[i] = local >= 0 ? (int32_t)a.groups[at] : -1;
  }
  __syncthreads();
  const GmLists L = {sK, sG, nullptr, kin};
  gm_select<false>(L, a.S, min(kin, a.kout), a.kout, lane, a.out_scores + (int64_t)q * a.kout,
                   a.out_groups + (int64_t)q * a.kout, a.out_items + (int64_t)q * a.kout);
}

namespace {
// LDS of group_scan_kernel behind the slab / score-tile union: query weights, counts, thresholds, candidates.
size_t gp_state_lds(int k) { return TK_QW_BYTES + TK_Q * (4 + 8) + (size_t)TK_Q * (k + 64) * 8; }

// The k = 128 footprint of the scan is over the 64 KiB default.
void gp_lds_limits() {
  static bool done[64] = {};
  tk_lds_limits(done, {{(const void*)group_scan_kernel<false>, TK_UNION_BYTES + gp_state_lds(TK_MAXK)},
                       {(const void*)group_scan_kernel<true>, TKB_UNION_BYTES + gp_state_lds(TK_MAXK)}});
}

template <bool BF16>
int gp_search(const MmtSearchScan& s, int k, const int32_t* groups, uint64_t* ws, float* scores, int64_t* out_groups,
              int64_t* out_items, void* stream) {
  if (!tk_scan_operands<BF16>(s) || !groups || !ws || !scores || !out_groups || !out_items || k < 1 || k > TK_MAXK ||
      !tk_shape_ok(s.NQ, s.NV, s.M, s.d, BF16))
    return MMT_ERR_ARG;
  if (!tk_scan_aligned(s)) return MMT_ERR_ALIGN;
  GpArgs a = {};
  a.q = s.q; a.q_lo = s.q_lo; a.qw = s.qw; a.g = s.g; a.gw = s.gw; a.groups = groups; a.subset = s.subset; a.ws = ws;
  a.NQ = s.NQ; a.NV = s.NV; a.M = s.M; a.K = s.M * s.d; a.k = k;
  tk_geometry(a);
  gp_lds_limits();
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL((group_scan_kernel<BF16>), dim3(a.n_qt * a.n_chunks), dim3(256),
                     (BF16 ? TKB_UNION_BYTES : TK_UNION_BYTES) + gp_state_lds(k), st, a);
  constexpr int64_t kMergeLdsMax = 64 * 1024;
  const int64_t list_bytes = (int64_t)a.n_chunks * k * 12;
  const int stage = list_bytes <= kMergeLdsMax;
  hipLaunchKernelGGL(group_merge_kernel, dim3(s.NQ), dim3(64), stage ? (size_t)list_bytes : 0, st, ws, groups, a.n_chunks, k,
                     k, stage, scores, out_groups, out_items);
  return (int)hipGetLastError();
}
}  // namespace

extern "C" int mmt_search_topk_groups(const MmtSearchScan* scan, int k, const int32_t* group_ids, uint64_t* ws, float* scores,
                                      int64_t* groups, int64_t* items, void* stream) {
  if (const int rc = tk_scan_gate(scan, SC_SUBSET)) return rc;
  return scan->storage == MMT_SEARCH_FP32 ? gp_search<false>(*scan, k, group_ids, ws, scores, groups, items, stream)
                                          : gp_search<true>(*scan, k, group_ids, ws, scores, groups, items, stream);
}

extern "C" int mmt_search_merge_group_lists(const float* scores, const int64_t* groups, const int64_t* index,
                                            const int64_t* const* ids, int S, int NQ, int kin, int kout, float* out_scores,
                                            int64_t* out_groups, int64_t* out_items, void* stream) {
  if (!scores || !groups || !index || !ids || !out_scores || !out_groups || !out_items || S < 1 || S > GS_MAXS || NQ <= 0 ||
      kin < 1 || kin > TK_MAXK || kout < 1 || kout > TK_MAXK)
    return MMT_ERR_ARG;
  GsArgs a = {scores, groups, index, ids, out_scores, out_groups, out_items, S, NQ, kin, kout};
  hipLaunchKernelGGL(group_shard_merge_kernel, dim3(NQ), dim3(64), (size_t)S * kin * 12, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}
