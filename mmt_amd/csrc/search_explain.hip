// The per-expert breakdown of a score (search.py: expert_scores, search_explained, pair_expert_scores): which expert
// produced a match, and with what share of the gate.  The score every scan ranks by is a gated mixture,
//   score(q, g) = sum_m qw[q][m] gw[g][m] <Q_m[q], G_m[g]> / sum_m qw[q][m] gw[g][m]        (0 -> 1e-5)
// a sum over experts of terms that share ONE denominator, so it decomposes exactly.  With qf = fold_fp32(Q, qw)[q] (the
// row mmt_search_fold produces), f_g the dequantised stored row of item g and den(q, g) = sum_m qw[q][m] gw[g][m]:
//   dot_m  = sum_{j < d} qf[m d + j] * f_g[m d + j]
//   part_m = dot_m / den                 fp8: fl(fl(dot_m * scale[g]) / den) on the codes, the scale where the scans place it
//   mix_m  = fl(qw[q][m] * gw[g][m]) / den
// sum_m part_m is the score on the stored value, sum_m mix_m is 1 (0 where the denominator was 0) and part_m / mix_m is
// <Q_m[q], G_m[g]>, the similarity of the pair under expert m alone.
//
// This is a gather -- R * C stored rows of K * sizeof(storage) bytes, about 2 flops per byte -- so it runs on the vector
// ALUs with 16-byte loads of the stored row, not on the 64 x 128 MFMA tile of mmt_search_rescore, which computes 64 rows to
// keep one.  A block is one row of qf (in LDS while K * 4 bytes fit XP_LDS_BYTES, through the caches otherwise) and `cb`
// consecutive candidates of it; a wave takes XP_PAIRS candidates at a time, so that many stored rows are in flight per
// wave and a group of qf is read once for all of them.
//
// THE ORDER.  Expert by expert, lane l takes the 16-byte groups l, l + 64, ... of the expert's d values (4 fp32, 8 bf16,
// 16 e4m3 codes; d is a multiple of that, so a group never straddles an expert), ONE fp32 accumulator per (pair, expert):
// acc = fma(qf[e], f[e], acc) over the lane's groups ascending and a group's elements ascending, then the butterfly
// acc += shfl_xor(acc, 32), 16, 8, 4, 2, 1 -- an fp32 add commutes, so every lane ends with the same bits -- and lane m
// keeps expert m.  The order is a function of (d, storage) and the element index alone: not of which operand is the row,
// the candidate's place in its list, C, cb, R, the row batching or the launch geometry.  A pair's values therefore depend
// on the pair alone, bit for bit, and with a stored row in qf's place parts(g, h) has the bits of parts(h, g): every
// product commutes and the denominator is an fma chain over m ascending, symmetric in its factors.
//
// The quotients are correctly rounded IEEE divisions (xp_div_rn: under the library's -ffast-math a plain `/` would be a
// multiply by v_rcp_f32), so on operands whose sums are exact numpy restates parts and mix bit for bit.
// No atomics; lane m of one wave is the one writer of slot m of a pair.  A candidate outside 0 .. NV - 1 is "none": its
// slots get NaN and no row is read for it (the loads go to row 0 and are discarded).
#include "search_scan.h"

// fl(a / b), correctly rounded: the IEEE division sequence of the hardware (v_div_scale_f32 brings both operands into
// range, a Newton step on v_rcp_f32 and two residual corrections as fmas, v_div_fmas_f32 undoes the scaling and
// v_div_fixup_f32 places the special cases) -- what the compiler emits for `a / b` without -ffast-math, spelled out because
// under the library's -ffast-math `a / b` is a * v_rcp_f32(b), 1 ulp off.  The fmas are builtins: not contracted, not split.
__device__ __forceinline__ float xp_div_rn(float a, float b) {
  bool vcc;
  const float ds = __builtin_amdgcn_div_scalef(a, b, false, &vcc);  // the denominator, scaled
  const float ns = __builtin_amdgcn_div_scalef(a, b, true, &vcc);   // the numerator, scaled; vcc: the quotient needs rescaling
  float rc = __builtin_amdgcn_rcpf(ds);
  rc = __builtin_fmaf(__builtin_fmaf(-ds, rc, 1.f), rc, rc);
  float qt = tk_mul_rn(ns, rc);
  qt = __builtin_fmaf(__builtin_fmaf(-ds, qt, ns), rc, qt);
  return __builtin_amdgcn_div_fixupf(__builtin_amdgcn_div_fmasf(__builtin_fmaf(-ds, qt, ns), rc, qt, vcc), b, a);
}

#define XP_PAIRS 4               // candidates a wave has in flight
#define XP_CB 64                 // candidates per block at full occupancy
#define XP_CB_MIN 16             // 4 waves x XP_PAIRS: one step of the block
#define XP_FILL 512              // blocks wanted per launch before cb is allowed to shrink (TK_FILL)
#define XP_LDS_BYTES (48 << 10)  // a longer qf row is read through the caches

struct XpArgs {
  const float* qf;            // [R][K] fp32
  const float* qw;            // [R][M]
  const void* g;              // [NV][K] fp32, bf16 bits or e4m3fn codes
  const float* gw;            // [NV][M]
  const float* gscale;        // [NV], fp8 only
  const int64_t* candidates;  // [R][C]
  float* parts;               // [R][C][M]
  float* mix;                 // [R][C][M]
  int NV, M, d, C, cb, n_cb;
};

// One 16-byte group of a stored row, widened exactly to fp32: EL values in element order.
template <int ST>
struct XpGroup;
template <>
struct XpGroup<MMT_SEARCH_FP32> {
  using T = float;
  static constexpr int EL = 4;
  static __device__ __forceinline__ void widen(const u32x4& v, float (&f)[EL]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) f[j] = __uint_as_float(v[j]);
  }
};
template <>
struct XpGroup<MMT_SEARCH_BF16> {
  using T = bf16_t;
  static constexpr int EL = 8;
  static __device__ __forceinline__ void widen(const u32x4& v, float (&f)[EL]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      f[2 * j] = __uint_as_float(v[j] << 16);
      f[2 * j + 1] = __uint_as_float(v[j] & 0xffff0000u);
    }
  }
};
template <>
struct XpGroup<MMT_SEARCH_FP8> {  // v_cvt_pk_f32_fp8, as tk_widen_fp8: every e4m3fn value is an fp32 value
  using T = uint8_t;
  static constexpr int EL = 16;
  static __device__ __forceinline__ void widen(const u32x4& v, float (&f)[EL]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8((int)v[j], false);  // bytes 0, 1 of dword j
      const f32x2 b = __builtin_amdgcn_cvt_pk_f32_fp8((int)v[j], true);   // bytes 2, 3
      f[4 * j] = a[0]; f[4 * j + 1] = a[1]; f[4 * j + 2] = b[0]; f[4 * j + 3] = b[1];
    }
  }
};

template <int ST, bool LDSQ>
__global__ __launch_bounds__(256) void expert_parts_kernel(XpArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  using G = XpGroup<ST>;
  using T = typename G::T;
  constexpr int EL = G::EL;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int M = a.M, d = a.d, K = M * d, C = a.C;
  const int64_t r = blockIdx.x / a.n_cb;
  const int c0 = (blockIdx.x % a.n_cb) * a.cb, c_end = min(C, c0 + a.cb);
  const float* q = a.qf + r * K;
  const float* qw = a.qw + r * M;
  if constexpr (LDSQ) {
    float* sQ = (float*)smem;  // [K]
    for (int i = tid * 4; i < K; i += 1024) *(f32x4*)(sQ + i) = *(const f32x4*)(q + i);
    __syncthreads();
    q = sQ;
  }
  const T* g = (const T*)a.g;
  const int groups = d / EL;  // 16-byte groups per expert
  for (int c = c0 + wave * XP_PAIRS; c < c_end; c += 4 * XP_PAIRS) {  // wave-uniform
    int item[XP_PAIRS];
    const T* row[XP_PAIRS];
#pragma unroll
    for (int p = 0; p < XP_PAIRS; ++p) {
      const int64_t cd = c + p < c_end ? a.candidates[r * C + c + p] : -1;
      item[p] = __builtin_amdgcn_readfirstlane((cd >= 0 && cd < a.NV) ? (int)cd : -1);
      row[p] = g + (int64_t)(item[p] < 0 ? 0 : item[p]) * K;  // none: row 0 is read and discarded, never out of bounds
    }
    float dot[XP_PAIRS];  // lane m: expert m's contraction
#pragma unroll
    for (int p = 0; p < XP_PAIRS; ++p) dot[p] = 0.f;
    bool any = false;  // wave-uniform: a step without an item (a shard's view of another shard's items) reads nothing
#pragma unroll
    for (int p = 0; p < XP_PAIRS; ++p) any = any || item[p] >= 0;
    for (int m = 0; any && m < M; ++m) {
      float acc[XP_PAIRS];
#pragma unroll
      for (int p = 0; p < XP_PAIRS; ++p) acc[p] = 0.f;
      for (int i = lane; i < groups; i += 64) {
        const int e = m * d + i * EL;
        u32x4 v[XP_PAIRS];
#pragma unroll
        for (int p = 0; p < XP_PAIRS; ++p) v[p] = *(const u32x4*)(row[p] + e);
        float qv[EL];
#pragma unroll
        for (int j = 0; j < EL; j += 4) {
          const f32x4 t = *(const f32x4*)(q + e + j);
          qv[j] = t[0]; qv[j + 1] = t[1]; qv[j + 2] = t[2]; qv[j + 3] = t[3];
        }
#pragma unroll
        for (int p = 0; p < XP_PAIRS; ++p) {
          float f[EL];
          G::widen(v[p], f);
#pragma unroll
          for (int j = 0; j < EL; ++j) acc[p] = __builtin_fmaf(qv[j], f[j], acc[p]);
        }
      }
#pragma unroll
      for (int p = 0; p < XP_PAIRS; ++p) {
#pragma unroll
        for (int o = 32; o; o >>= 1) acc[p] = tk_add_rn(acc[p], __shfl_xor(acc[p], o));
        dot[p] = lane == m ? acc[p] : dot[p];
      }
    }
    if (lane < M) {
      const float qwm = qw[lane];
#pragma unroll
      for (int p = 0; p < XP_PAIRS; ++p) {
        if (c + p >= c_end) break;
        const int64_t at = (r * C + c + p) * M + lane;
        if (item[p] < 0) {
          a.parts[at] = a.mix[at] = __builtin_nanf("");
          continue;
        }
        const float* gwi = a.gw + (int64_t)item[p] * M;
        float den = 0.f;
        for (int m = 0; m < M; ++m) den = __builtin_fmaf(qw[m], gwi[m], den);
        den = den == 0.f ? 1e-5f : den;
        float num = dot[p];
        if constexpr (ST == MMT_SEARCH_FP8) num = tk_mul_rn(num, a.gscale[item[p]]);
        a.parts[at] = xp_div_rn(num, den);
        a.mix[at] = xp_div_rn(tk_mul_rn(qwm, gwi[lane]), den);
      }
    }
  }
}

namespace {
// Candidates per block: XP_CB, halved (down to one step of the block) while the launch would not fill the chip.
int xp_cb(int R, int C) {
  int cb = XP_CB;
  while (cb > XP_CB_MIN && (int64_t)R * ((C + cb - 1) / cb) < XP_FILL) cb >>= 1;
  return cb;
}

template <int ST>
int xp_launch(XpArgs a, int R, hipStream_t st) {
  const int K = a.M * a.d, grid = R * a.n_cb;
  if ((size_t)K * 4 <= XP_LDS_BYTES)
    hipLaunchKernelGGL((expert_parts_kernel<ST, true>), dim3(grid), dim3(256), (size_t)K * 4, st, a);
  else
    hipLaunchKernelGGL((expert_parts_kernel<ST, false>), dim3(grid), dim3(256), 0, st, a);
  return (int)hipGetLastError();
}
}  // namespace

extern "C" int mmt_search_expert_parts(const float* qf, const float* qw, const void* g, const float* gw, const float* gscale,
                                       int storage, int NV, int M, int d, const int64_t* candidates, int R, int C,
                                       float* parts, float* mix, void* stream) {
  if (!qf || !qw || !g || !gw || !candidates || !parts || !mix || (unsigned)storage > MMT_SEARCH_FP8 ||
      (storage == MMT_SEARCH_FP8) != (gscale != nullptr) || C < 1 || C > MMT_SEARCH_MAX_C ||
      !tk_shape_ok(R, NV, M, d, storage != MMT_SEARCH_FP32, storage == MMT_SEARCH_FP8))
    return MMT_ERR_ARG;
  const int cb = xp_cb(R, C), n_cb = (C + cb - 1) / cb;
  if ((int64_t)R * n_cb >= (1ll << 31)) return MMT_ERR_ARG;  // the grid: one block per row and cb candidates
  if (((uintptr_t)qf | (uintptr_t)g) & 15) return MMT_ERR_ALIGN;
  const XpArgs a = {qf, qw, g, gw, gscale, candidates, parts, mix, NV, M, d, C, cb, n_cb};
  const hipStream_t st = (hipStream_t)stream;
  switch (storage) {
    case MMT_SEARCH_FP32: return xp_launch<MMT_SEARCH_FP32>(a, R, st);
    case MMT_SEARCH_BF16: return xp_launch<MMT_SEARCH_BF16>(a, R, st);
    default: return xp_launch<MMT_SEARCH_FP8>(a, R, st);
  }
}
