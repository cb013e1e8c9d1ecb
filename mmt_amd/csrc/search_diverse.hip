// Diversified search (search.py: VideoIndex.pair_scores, diversify, search_diverse): max marginal relevance (Carbonell &
// Goldstein, SIGIR 1998) over a per-query shortlist -- repeatedly the candidate most relevant to the query and least similar
// to the ones already picked.  It needs what no scan computes, the similarity of two STORED items to each other:
//   sim(g, h) = <f_g, f_h> / sum_m gw_g[m] gw_h[m]      (0 -> 1e-5)
// with f_g the dequantised stored row (fp32: the row; bf16: widened; fp8: code * gscale[g]) -- the 'indep' similarity with
// item g in the query's place.  Two launches, two additive entries; MmtSearchScan and the ten scans are untouched.
//   pair_scores_kernel<ST>: one block per list of C <= 128 candidates computes its C x C Gram: the two 64 x 128 tiles of
//                           tk_tile's shape at once, as a 2 x 2 grid of waves with 2 x 2 accumulators of 32 x 32 each, BOTH
//                           operands read from ONE gathered slab in LDS (128 rows x 32 fp32 or x 64 bf16: 18 KiB): the
//                           128-row TkStager of search_scan.h inside tk_k_loop, both fragments of tk_step read from it -- the
//                           pieces the scans' K loop and the self-join's are made of.  fp32 rows go to
//                           v_mfma_f32_32x32x2_f32; bf16 rows, and fp8 codes widened exactly in the stager, to
//                           v_mfma_f32_32x32x16_bf16 -- the operands are exact bf16 values, so one MFMA per fragment, no
//                           hi / lo pair.  A fragment wholly past C is neither loaded nor multiplied.
//                           Every product a[k] * b[k] is exact or rounded the same way round, and every output sums its
//                           products in the one order the slab and MFMA sequence fix, so sim(g, h) has the bits of sim(h, g)
//                           and depends on the two rows alone: not on their places in the list, the other candidates, the
//                           row batching, NV or the shard.  Epilogue: tk_pair_sims (search_scan.h), the one definition of
//                           sim: den = fma(gw_g[m], gw_h[m], den) for m ascending, fp8: num = fl(acc * fl(scale_g *
//                           scale_h)), sim = num / den.  A candidate outside
//                           0 .. NV - 1 is "none": checked on the device, never dereferenced, NaN in its row and column.
//   mmr_kernel            : one wave per list.  items / rel are the list in the search's order (what mmt_search_rescore
//                           with k = C returns, padded with (-1, -inf)), sims its Gram.  n = the number of items >= 0, taken
//                           to be the positions 0 .. n - 1.  Slot 0 is position 0 with value fl(a * rel[0]).  For slot
//                           t >= 1 every unselected position p keeps pen_p, the largest sim(p, s) over the selected s (the
//                           first one as it is, then replaced where sim > pen: a plain compare, the first of equals stays),
//                           v_p = fl(fl(a * rel[p]) - fl(b * pen_p)) -- two rounded multiplies (tk_mul_rn) and a rounded
//                           subtract, never an fma -- and the position with the largest tk_key(v_p, p) is selected: the
//                           largest v_p, -0 tied with +0, equal values to the lowest p.  Slot t gets (rel[p], items[p],
//                           v_p); the slots from min(k, n) on (-inf, -1, -inf).  Lane l holds positions l and 64 + l; a
//                           step reads row s of the Gram (two coalesced loads) and reduces 64 keys with shuffles.
// No atomics; every output slot has one writer.  LDS 27.5 KiB static: under the 64 KiB default, so no limit is raised.
#include "search_topk.h"

#define DV_MAXC MMT_SEARCH_MAX_DC
static_assert(DV_MAXC == TK_G, "a list is one 128-column tile");
#define DV_SLAB_BYTES (DV_MAXC * TK_LD * 4)
static_assert(DV_SLAB_BYTES == DV_MAXC * TKB_LD * 2, "the fp32 and the bf16 slab are the same bytes");

struct DvArgs {
  const void* g;          // [NV][K] fp32, bf16 bits or e4m3fn codes
  const float* gw;        // [NV][M]
  const float* gscale;    // fp8: [NV]
  const int64_t* items;   // [R][C]
  float* sims;            // [R][C][C]
  int NV, M, K, C;
};

// acc[s * 2 + t] += slab rows (wr*64 + s*32 ..) . slab rows (wc*64 + t*32 ..)^T over the whole K: the 128-row stager of
// search_scan.h (T = float, bf16_t, or uint8_t for fp8 codes, widened on the way in) with BOTH fragments read from its one
// slab, inside tk_k_loop.  lr[s] && lc[t]: the fragment pair holds a position below C.
template <class T>
__device__ __forceinline__ void dv_gram(f32x16 (&acc)[4], unsigned char* smem, const T* g, int K, const int* sRow,
                                        const bool (&lr)[2], const bool (&lc)[2], int tid, int wr, int wc, int l31, int h) {
  using St = TkStager<T, DV_MAXC>;
  typename St::S* sB = (typename St::S*)smem;  // [DV_MAXC][LD]
  St B;
  B.rows([=](int r) { return sRow[r]; }, tid);
  tk_k_loop<St::BK, St::KK>(
      K, [&](int kb) { B.load({g}, K, kb, tid); }, [&] { B.store(sB, tid); },
      [&](int kk) {
        tk_step<1, 2, 2>(acc, sB, wr * 64 + l31, sB, wc * 64 + l31, kk, h, [&](int s, int t) { return lr[s] && lc[t]; });
      });
}

template <int ST>
__global__ __launch_bounds__(256) void pair_scores_kernel(DvArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[DV_SLAB_BYTES];
  __shared__ float sW[DV_MAXC * MMT_MAX_EXPERTS];  // the candidates' weights, zero for none and past M
  __shared__ float sSc[DV_MAXC];                   // fp8: their scales
  __shared__ int sRow[DV_MAXC];                    // their stored rows, -1 = none
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, h = lane >> 5, wr = wave >> 1, wc = wave & 1;
  const int C = a.C, M = a.M;
  const int64_t list = blockIdx.x;
  if (tid < DV_MAXC) {
    const int64_t v = tid < C ? a.items[list * C + tid] : -1;
    const int g = (v >= 0 && v < a.NV) ? (int)v : -1;
    sRow[tid] = g;
    if constexpr (ST == MMT_SEARCH_FP8) sSc[tid] = g >= 0 ? a.gscale[g] : 1.f;
  }
  __syncthreads();
  for (int i = tid; i < DV_MAXC * MMT_MAX_EXPERTS; i += 256) {
    const int g = sRow[i / MMT_MAX_EXPERTS], m = i % MMT_MAX_EXPERTS;
    sW[i] = (g >= 0 && m < M) ? a.gw[(int64_t)g * M + m] : 0.f;
  }
  // which of the wave's 32-row / 32-column fragments hold a position below C: wave-uniform
  const bool lr[2] = {wr * 64 < C, wr * 64 + 32 < C}, lc[2] = {wc * 64 < C, wc * 64 + 32 < C};
  using T = std::conditional_t<ST == MMT_SEARCH_FP32, float, std::conditional_t<ST == MMT_SEARCH_FP8, uint8_t, bf16_t>>;
  f32x16 acc[4];  // [s][t]
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
  dv_gram(acc, smem, (const T*)a.g, a.K, sRow, lr, lc, tid, wr, wc, l31, h);
  // the K loop's barriers fence sW.  Lane: column wc*64 + t*32 + l31, rows wr*64 + s*32 + (r&3) + 8*(r>>2) + 4h.
  float* out = a.sims + list * C * C;
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int col = wc * 64 + t * 32 + l31;
    if (col >= C) continue;
    const bool col_live = sRow[col] >= 0;
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = wr * 64 + s * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
        if (row >= C) continue;
        const float one[1] = {acc[s * 2 + t][r]};
        float sim[1];
        tk_pair_sims<ST == MMT_SEARCH_FP8>(
            sim, one, M, [&](int, int m) { return sW[row * MMT_MAX_EXPERTS + m]; },
            [&](int m) { return sW[col * MMT_MAX_EXPERTS + m]; }, [&](int) { return sSc[row]; },
            ST == MMT_SEARCH_FP8 ? sSc[col] : 1.f);
        out[row * C + col] = (col_live && sRow[row] >= 0) ? sim[0] : __builtin_nanf("");
      }
  }
}

// fl(a - b) as an instruction of its own, the partner of tk_mul_rn and tk_add_rn.
__device__ __forceinline__ float dv_sub_rn(float a, float b) {
  float r;
  asm("v_sub_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}

// One wave per list: blockDim 64.
__global__ __launch_bounds__(64) void mmr_kernel(const int64_t* __restrict__ items, const float* __restrict__ rel,
                                                 const float* __restrict__ sims, int C, int k, float a, float b,
                                                 float* __restrict__ scores, int64_t* __restrict__ index,
                                                 float* __restrict__ values) {
  const int lane = threadIdx.x;
  const int64_t list = blockIdx.x;
  const float* gram = sims + list * C * C;
  int64_t it[2];
  float ar[2], pen[2] = {0.f, 0.f};
  bool open[2];  // live and not yet selected
  int n = 0;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int p = lane + 64 * j;
    it[j] = p < C ? items[list * C + p] : -1;
    ar[j] = p < C ? rel[list * C + p] : 0.f;
    n += __popcll(__ballot(it[j] >= 0));
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) open[j] = lane + 64 * j < n;
  const int kk = k < n ? k : n;
  float* o_s = scores + list * k;
  int64_t* o_i = index + list * k;
  float* o_v = values + list * k;
  for (int t = kk + lane; t < k; t += 64) {
    o_s[t] = -__builtin_inff();
    o_i[t] = -1;
    o_v[t] = -__builtin_inff();
  }
  if (kk == 0) return;
#pragma unroll
  for (int j = 0; j < 2; ++j) ar[j] = tk_mul_rn(a, ar[j]);  // fl(a * rel[p]); rel itself is read again where it is written
  int sel = 0;  // the position selected last: wave-uniform
  if (lane == 0) {
    o_s[0] = rel[list * C];
    o_i[0] = it[0];
    o_v[0] = ar[0];
    open[0] = false;
  }
  for (int t = 1; t < kk; ++t) {
    uint64_t best = 0ull;
    float v[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int p = lane + 64 * j;
      v[j] = 0.f;
      if (open[j]) {
        const float x = gram[sel * C + p];
        // selected as integers: a float select may become v_max_f32, which treats NaN and the zeros differently
        pen[j] = __int_as_float((t == 1 || x > pen[j]) ? __float_as_int(x) : __float_as_int(pen[j]));
        v[j] = dv_sub_rn(ar[j], tk_mul_rn(b, pen[j]));
        const uint64_t key = tk_key(v[j], p);
        best = key > best ? key : best;
      }
    }
#pragma unroll
    for (int off = 32; off; off >>= 1) {
      const uint64_t other = __shfl_xor(best, off, 64);
      best = other > best ? other : best;
    }
    sel = tk_index(best);  // t < kk <= n: an open position exists, and every key of one is > 0
    if (lane == (sel & 63)) {
      const int j = sel >> 6;
      o_s[t] = rel[list * C + sel];
      o_i[t] = j ? it[1] : it[0];
      o_v[t] = j ? v[1] : v[0];
      if (j) open[1] = false; else open[0] = false;
    }
  }
}

namespace {
template <int ST>
int dv_launch(const DvArgs& a, int R, hipStream_t st) {
  hipLaunchKernelGGL(pair_scores_kernel<ST>, dim3(R), dim3(256), 0, st, a);
  return (int)hipGetLastError();
}
}  // namespace

extern "C" int mmt_search_pair_scores(const void* g, const float* gw, const float* gscale, int storage, int NV, int M, int d,
                                      const int64_t* items, int R, int C, float* sims, void* stream) {
  if (!g || !gw || !items || !sims || (unsigned)storage > MMT_SEARCH_FP8 || (storage == MMT_SEARCH_FP8) != (gscale != nullptr) ||
      C < 1 || C > DV_MAXC || !tk_shape_ok(R, NV, M, d, storage != MMT_SEARCH_FP32, storage == MMT_SEARCH_FP8))
    return MMT_ERR_ARG;
  if ((uintptr_t)g & 15) return MMT_ERR_ALIGN;
  const DvArgs a = {g, gw, gscale, items, sims, NV, M, M * d, C};
  const hipStream_t st = (hipStream_t)stream;
  switch (storage) {
    case MMT_SEARCH_FP32: return dv_launch<MMT_SEARCH_FP32>(a, R, st);
    case MMT_SEARCH_BF16: return dv_launch<MMT_SEARCH_BF16>(a, R, st);
    default: return dv_launch<MMT_SEARCH_FP8>(a, R, st);
  }
}

extern "C" int mmt_search_mmr(const int64_t* items, const float* rel, const float* sims, int R, int C, int k, float a, float b,
                              float* scores, int64_t* index, float* values, void* stream) {
  if (!items || !rel || !sims || !scores || !index || !values || R < 1 || C < 1 || C > DV_MAXC || k < 1 || k > C)
    return MMT_ERR_ARG;
  hipLaunchKernelGGL(mmr_kernel, dim3(R), dim3(64), 0, (hipStream_t)stream, items, rel, sims, C, k, a, b, scores, index, values);
  return (int)hipGetLastError();
}
