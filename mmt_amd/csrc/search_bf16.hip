// A gallery stored in bf16 (search.py: VideoIndex(dtype=torch.bfloat16)): the folds.  The scans over it are the BF16
// instantiations of the shared bodies (search.hip, search_rank.hip, search_range.hip, search_norm.hip).
//
// Only the storage is lossy: the index keeps bf16_rne(gw (.) G) -- the fp32 fold of mmt_search_fold rounded once by a
// plain cast -- and the score is DEFINED on that stored value,
//
//   score(q, g) = < fold_fp32(Q, qw)[q], dequant(stored[g]) > / sum_m qw[q][m] gw[g][m]     (0 -> 1e-5)
//
// The fp32 query runs on the bf16 matrix cores as two terms, hi = bf16(qf) and lo = bf16(qf - hi): bf16 x bf16 products
// are exact in fp32, the accumulator is fp32, and what the split drops is below 2^-16 relative per query element.
// (tk_scan_bf16 of search_scan.h: per 64-wide K slab the block stages hi, lo and the gallery in LDS; a wave reads each
// gallery fragment ONCE and feeds it to the hi and the lo MFMA.  A 64-query tile is below the bf16 ridge for a gallery
// streamed from HBM; the blocks of one gallery chunk are consecutive ids on one XCD (xcd_remap), so the chunk is fetched
// from HBM once per XCD and served to the other query tiles from L2.)
//
//   fold_bf16_kernel<false> : x [N][M][d] fp32, w [N][M] -> bf16 [N][M*d], 8 elements (one 16-byte store) per thread
//   fold_bf16_kernel<true>  : the same fold written as the hi / lo pair (queries)
#include "search_scan.h"

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

namespace {
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
