// The merge behind a gallery cut into shards (search.py: ShardedVideoIndex.search): every shard is an ordinary index with
// item numbers of its own and returns, per query, its best kin (score, local item) pairs; this kernel turns the S lists of
// a query into the best kout of the whole gallery, under the one tie rule of the search kernels -- score descending, equal
// scores by ascending GLOBAL item number (ids[s][local]: shard s's local -> global table).
//
//   shard_merge_kernel : one block per query.  The S x kin candidates become keys in LDS (search_topk.h: tk_key of the
//                        score and the global number; 0 = empty slot, local index -1), 32 KiB at S = 32, kin = 128.  Each
//                        list is best-first under the global order (a shard's table is increasing, so its local tie order
//                        is the global one) with its empty slots last, so a key at position j of its list has rank
//                        j + (keys above it in every other list), each term a binary search -- topk_merge_kernel's scheme.
//                        Distinct items have distinct keys, so every output slot below the candidate count has exactly
//                        one writer; the slots from the count on are written (-inf, -1) by the threads that own them.
// The key only orders: the score written is the input's own bits (so -0.0 stays -0.0 while it ties with +0.0, as tk_key
// ranks them) and the index comes from the table as int64.  No atomics: bit-reproducible.
#include "search_topk.h"

#define SM_MAXS 32

struct SmArgs {
  const float* scores;        // [S][NQ][kin]
  const int64_t* index;       // [S][NQ][kin] shard-local item, -1 = empty slot
  const int64_t* const* ids;  // [S] pointers to tables on this device: local -> global item number (< 2^31); index values
                              //     are trusted to lie below their table's length (mmt_hip.h)
  float* out_scores;          // [NQ][kout]
  int64_t* out_index;         // [NQ][kout]
  int S, NQ, kin, kout;
};

__global__ __launch_bounds__(256) void shard_merge_kernel(SmArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint64_t* sK = (uint64_t*)smem;        // [S][kin] keys
  int* sCnt = (int*)(sK + a.S * a.kin);  // [S] candidates held by list s
  const int q = blockIdx.x, kin = a.kin, n = a.S * kin;
  for (int i = threadIdx.x; i < n; i += 256) {
    const int c = i / kin, j = i - c * kin;
    const int64_t at = ((int64_t)c * a.NQ + q) * kin + j;
    const int64_t local = a.index[at];
    sK[i] = local >= 0 ? tk_key(a.scores[at], (int)a.ids[c][local]) : 0ull;
  }
  __syncthreads();
  if (threadIdx.x < a.S) {  // empty slots come last: the first of them is the list's length
    const uint64_t* l = sK + threadIdx.x * kin;
    int lo = 0, hi = kin;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (l[mid]) lo = mid + 1;
      else hi = mid;
    }
    sCnt[threadIdx.x] = lo;
  }
  __syncthreads();
  int total = 0;
  for (int c = 0; c < a.S; ++c) total += sCnt[c];
  for (int j = total + threadIdx.x; j < a.kout; j += 256) {
    a.out_scores[(int64_t)q * a.kout + j] = -__builtin_inff();
    a.out_index[(int64_t)q * a.kout + j] = -1;
  }
  const int lim = min(kin, a.kout);
  for (int i = threadIdx.x; i < n; i += 256) {
    const int c = i / kin, j = i - c * kin;
    if (j >= a.kout) continue;
    const uint64_t key = sK[i];
    if (!key) continue;
    int rank = j;
    for (int c2 = 0; c2 < a.S && rank < a.kout; ++c2) {
      if (c2 == c) continue;
      const uint64_t* l = sK + c2 * kin;
      int lo = 0, hi = lim;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (l[mid] > key) lo = mid + 1;
        else hi = mid;
      }
      rank += lo;
    }
    if (rank < a.kout) {
      const int64_t at = ((int64_t)c * a.NQ + q) * kin + j;
      a.out_scores[(int64_t)q * a.kout + rank] = a.scores[at];
      a.out_index[(int64_t)q * a.kout + rank] = a.ids[c][a.index[at]];
    }
  }
}

extern "C" int mmt_search_merge_lists(const float* scores, const int64_t* index, const int64_t* const* ids, int S, int NQ,
                                      int kin, int kout, float* out_scores, int64_t* out_index, void* stream) {
  if (!scores || !index || !ids || !out_scores || !out_index || S < 1 || S > SM_MAXS || NQ <= 0 || kin < 1 ||
      kin > TK_MAXK || kout < 1 || kout > TK_MAXK)
    return MMT_ERR_ARG;
  SmArgs a = {scores, index, ids, out_scores, out_index, S, NQ, kin, kout};
  hipLaunchKernelGGL(shard_merge_kernel, dim3(NQ), dim3(256), (size_t)S * kin * 8 + S * 4, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}
