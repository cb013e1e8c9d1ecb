// A gallery stored in fp8 (search.py: VideoIndex(dtype=torch.float8_e4m3fn)): the fold.  The scans over it are further
// instantiations of the shared bodies (search.hip, search_rank.hip, search_range.hip) with an argument block that says
// kFp8: tk_tile (search_scan.h) then takes tk_scan_fp8 -- the bf16 K loop with the gallery slab loaded at half the bytes
// and widened exactly to bf16 on its way into LDS -- and multiplies by the item's scale in the epilogue.
//
// Only the storage is lossy.  With f = fold_fp32(G, gw)[g], the row mmt_search_fold produces, the index keeps per item
//
//   amax   = max_k |f[k]|
//   scale  = 2^e, the smallest power of two with amax / 2^e <= 448 (the largest e4m3fn value): with amax = mant * 2^ex,
//            mant in [0.5, 1), e = ex - 9 if mant <= 0.875, else ex - 8; e clamped to -120 .. 120; amax == 0 -> scale = 1
//   stored = e4m3fn_rne(f / scale)     OCP e4m3fn, round-to-nearest-even, subnormals included
//
// The division by a power of two is exact and |f / scale| <= 448, so the cast never saturates.  The scale depends on the
// item alone: the stored bytes do not depend on how the gallery was chunked or which shard holds the item.  The inputs are
// taken to be finite: a NaN or Inf in an item is not looked for, gives that item an unspecified scale and NaN codes or
// garbage in its row, and so meaningless (possibly NaN) scores for that item alone.  The score is DEFINED on the stored
// value, as for bf16,
//
//   score(q, g) = fl( fl(acc * scale[g]) / den ),   acc = < fold_fp32(Q, qw)[q], dequant(stored[g]) >,
//   den = sum_m qw[q][m] gw[g][m]     (0 -> 1e-5)
//
// with acc on the bf16 matrix cores as tk_scan_bf16 computes it: hi = bf16(qf), lo = bf16(qf - hi), fp32 accumulation;
// every e4m3fn value is a bf16 value, so nothing is rounded on the way.  The scale multiply is a rounded multiply of its
// own (tk_mul_rn); the scale being a power of two, its place in the expression cannot change the bits short of underflow
// or overflow.  Against the float32 index only the gallery rounding differs:
//
//   |score_fp8 - score_fp32| <= ( 2^-4 * <|qf|, |f|> + 2^-10 * scale[g] * sum_k |qf[k]| ) / |den|  + 1e-5
//
// -- e4m3's unit roundoff for normal values, and half the subnormal spacing 2^-9 * scale below 2^-6 * scale.
//
//   fold_fp8_kernel : x [N][M][d] fp32, w [N][M] -> e4m3fn codes [N][M*d] and scale [N]; one wave per item, two passes over
//                     the row (amax, then the cast), 16 elements = one 16-byte store per lane and step
#include "search_scan.h"

// One wave per row: lane l takes the groups of 16 elements l, l + 64, ... of the row's K = M*d (a group never straddles an
// (r, m) row because d % 16 == 0).  f = fl(w * x) is a rounded multiply of its own in both passes (tk_mul_rn), the fold of
// mmt_search_fold bit for bit.
__global__ __launch_bounds__(256) void fold_fp8_kernel(const float* __restrict__ x, const float* __restrict__ w, int N, int M,
                                                       int d, uint8_t* __restrict__ out, float* __restrict__ scale) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int K = M * d, n16 = K >> 4;
  for (int64_t row = blockIdx.x * 4 + wave; row < N; row += (int64_t)gridDim.x * 4) {
    const f32x4* xr = (const f32x4*)(x + row * K);
    const float* wr = w + row * M;
    float amax = 0.f;
    for (int i = lane; i < n16; i += 64) {
      const float wv = wr[(i << 4) / d];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const f32x4 v = xr[4 * i + j];
#pragma unroll
        for (int u = 0; u < 4; ++u) amax = fmaxf(amax, fabsf(tk_mul_rn(wv, v[u])));
      }
    }
#pragma unroll
    for (int o = 32; o; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o));
    int ex;
    const float mant = frexpf(amax, &ex);
    int e = mant <= 0.875f ? ex - 9 : ex - 8;
    e = e < -120 ? -120 : e > 120 ? 120 : e;
    if (amax == 0.f) e = 0;
    const float inv = ldexpf(1.f, -e);  // exact, and so is every product with it: |f * inv| <= 448
    if (lane == 0) scale[row] = ldexpf(1.f, e);
    for (int i = lane; i < n16; i += 64) {
      const float wv = wr[(i << 4) / d];
      u32x4 o;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const f32x4 v = xr[4 * i + j];
        float p[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) p[u] = tk_mul_rn(tk_mul_rn(wv, v[u]), inv);
        int r = __builtin_amdgcn_cvt_pk_fp8_f32(p[0], p[1], 0, false);  // v_cvt_pk_fp8_f32: e4m3fn, nearest-even
        r = __builtin_amdgcn_cvt_pk_fp8_f32(p[2], p[3], r, true);
        o[j] = (uint32_t)r;
      }
      *(u32x4*)(out + row * K + (i << 4)) = o;
    }
  }
}

extern "C" int mmt_search_fold_fp8(const float* x, const float* w, int N, int M, int d, uint8_t* out, float* scale,
                                   void* stream) {
  if (!x || !w || !out || !scale || N <= 0 || M <= 0 || M > MMT_MAX_EXPERTS || d <= 0 || (d & 15)) return MMT_ERR_ARG;
  if (((uintptr_t)x | (uintptr_t)out) & 15) return MMT_ERR_ALIGN;
  const int blocks = (N + 3) / 4 < 65536 ? (N + 3) / 4 : 65536;
  hipLaunchKernelGGL(fold_fp8_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x, w, N, M, d, out, scale);
  return (int)hipGetLastError();
}
