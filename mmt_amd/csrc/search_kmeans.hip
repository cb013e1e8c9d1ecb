// The update step of a k-means over the stored items (search.py: cell_sums, cell_centroids, train_cells).  The assignment
// step of a Lloyd iteration is the self-join with a source -- centroids.neighbours(k=1, source=index), on the matrix cores;
// this file is the other half: per cell the sum of its members' stored rows and weights, and the centroid they make.
// With f_g the dequantised stored row of item g (fp32 as it is, bf16 widened, fp8 code x the item's power-of-two scale --
// all exact), gw_g its weights and L the member list of a cell (its slice of the cells' item table, ascending, n = |L|):
//   S[m] = sum_{g in L} f_g[m]        w[m] = sum_{g in L} gw_g[m]
//   G_c[m] = S[m] / |S[m]|_2  (a zero S[m]: a zero row)        gw_c[m] = w[m] / n
// spherical k-means per expert, weighted by the gate.
//
// This is a gather at well under 1 flop per byte (one add per element read), so it runs on the vector ALUs with 16-byte
// loads of the stored rows through the item table, as expert_parts_kernel does; the bound is HBM, every labelled row read
// once.
//
// THE ORDER.  A cell's list is cut into pieces of at most KM_PIECE consecutive positions.  cell_sums_kernel: one block per
// (piece, slab of KM_SLAB columns); a thread owns the EL columns of its 16-byte group and adds the piece's rows in
// ascending position, one rounded fp32 add each (tk_add_rn: not contracted, not reassociated), starting from +0, KM_ROWS
// rows in flight per lane; it writes one partial row to the workspace [pieces][M d] -- one writer per slot.  The weights
// go the same way into [pieces][M] (the slab-0 block, thread m).  cell_centroids_kernel: one block per cell adds the
// cell's partial rows in ascending piece order, again from +0.  So the sum of a column is a function of the rows'
// positions in their cell's list and of the column: not of the launch geometry, the other cells, num_items or the
// batching (search.cell_sums_ref restates it in numpy).  The squares of an expert's d sums are reduced by one wave: lane l
// takes the elements l, l + 64, ... ascending with one fma each, then the butterfly of expert_parts_kernel -- an order
// that depends on d alone.  The root is v_sqrt_f32 with one Newton correction, the quotients are correctly rounded
// divisions.  No atomics, no scratch.
//
// Everything that comes from the device is range-checked and dropped when outside, never dereferenced: a piece whose
// positions are not inside the item table or that is longer than KM_PIECE is "no work" (its partial row is zero), an
// item number outside 0 .. NV - 1 contributes nothing, a cell whose piece range is not inside the workspace is skipped.
//
// THE EXACT SUMS (search.py: sum_scale, cell_sums_exact, cell_centroids(exact=True); mmt_hip.h states the definition).  The
// same kernels with another accumulator: a value becomes the int64 term rint(f * 2^(B - E)) -- widened to fp64, where the
// scaling by a power of two is exact, rounded to nearest even (v_rndne_f64), clamped to +-2^B, converted -- and the terms
// are added as integers, so a cell's sums are a function of its member SET: not of the order of the list, the cut into
// pieces or the shard that held a row.  cell_sums_join_kernel adds a cell's partial int64 rows; the int64 tensors of
// several shards add with a plain integer add.  cell_centroids_exact_kernel turns them back into fp32 -- one int64 ->
// fp32 conversion, round to nearest even, then a scaling by 2^(E - B) -- and finishes the centroid with the very code of
// cell_centroids_kernel (km_centroid_block): equal fp32 sums give equal centroid bits on both paths.  absmax_kernel is the
// one pass that finds E: per-block maxima of |f| and |gw|, one writer per slot.
#include "search_scan.h"

#define KM_PIECE MMT_SEARCH_SUM_PIECE  // positions of a cell's list one block adds
#define KM_SLAB MMT_SEARCH_SUM_SLAB    // columns of the M d one block takes
#define KM_ROWS 8                      // stored rows a lane has in flight

// fl(a / b), correctly rounded: the IEEE division sequence (see xp_div_rn of search_explain.hip) -- under the library's
// -ffast-math a plain `a / b` is a * v_rcp_f32(b).
__device__ __forceinline__ float km_div_rn(float a, float b) {
  bool vcc;
  const float ds = __builtin_amdgcn_div_scalef(a, b, false, &vcc);
  const float ns = __builtin_amdgcn_div_scalef(a, b, true, &vcc);
  float rc = __builtin_amdgcn_rcpf(ds);
  rc = __builtin_fmaf(__builtin_fmaf(-ds, rc, 1.f), rc, rc);
  float qt = tk_mul_rn(ns, rc);
  qt = __builtin_fmaf(__builtin_fmaf(-ds, qt, ns), rc, qt);
  return __builtin_amdgcn_div_fixupf(__builtin_amdgcn_div_fmasf(__builtin_fmaf(-ds, qt, ns), rc, qt, vcc), b, a);
}

// sqrt(x) for x > 0 in the normal range: v_sqrt_f32 (1 ulp) and one Newton step on the fma residual, within half an ulp
// and a bit.
__device__ __forceinline__ float km_sqrt(float x) {
  const float s = __builtin_amdgcn_sqrtf(x);
  const float r = __builtin_fmaf(-s, s, x);
  return __builtin_fmaf(r, km_div_rn(0.5f, s), s);
}

// The accumulator of a column.  KmFloatAcc: fp32, one rounded add per row -- the stated order.  KmFixedAcc: the int64
// term of the exact sums, rint(f * scale) in fp64 with scale = 2^(B - E), clamped to +-limit = 2^B: f * scale is exact
// (a power of two; where it underflows fp64 the term is 0 either way), the rounding is v_rndne_f64, and |r| <= 2^61
// converts without loss.  The comparisons are written out so that -ffast-math has nothing to reassociate.
struct KmFloatAcc {
  using T = float;
  __device__ __forceinline__ float add(float acc, float f) const { return tk_add_rn(acc, f); }
};
struct KmFixedAcc {
  using T = long long;
  double scale, limit;
  __device__ __forceinline__ long long add(long long acc, float f) const {
    double r = __builtin_rint((double)f * scale);
    r = r > limit ? limit : r;
    r = r < -limit ? -limit : r;
    return acc + (long long)r;
  }
};
typedef long long i64x2 __attribute__((ext_vector_type(2)));

template <class A>
struct KmSumArgs {
  const void* g;         // [NV][K] fp32, bf16 bits or e4m3fn codes
  const float* gw;       // [NV][M]
  const float* gscale;   // [NV], fp8 only
  const int64_t* items;  // [n_items]
  const int32_t* work;   // [n_work][3] = (cell, first position, end position)
  typename A::T* ws;     // [n_work][K]
  typename A::T* wws;    // [n_work][M]
  int NV, M, K, n_items;
  A acc, wacc;           // of the rows, of the weights
};

// One 16-byte group of a stored row, widened exactly to fp32 (the groups of expert_parts_kernel).
template <int ST>
struct KmGroup;
template <>
struct KmGroup<MMT_SEARCH_FP32> {
  using T = float;
  static constexpr int EL = 4;
  static __device__ __forceinline__ void widen(const u32x4& v, float (&f)[EL]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) f[j] = __uint_as_float(v[j]);
  }
};
template <>
struct KmGroup<MMT_SEARCH_BF16> {
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
struct KmGroup<MMT_SEARCH_FP8> {
  using T = uint8_t;
  static constexpr int EL = 16;
  static __device__ __forceinline__ void widen(const u32x4& v, float (&f)[EL]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8((int)v[j], false);
      const f32x2 b = __builtin_amdgcn_cvt_pk_f32_fp8((int)v[j], true);
      f[4 * j] = a[0]; f[4 * j + 1] = a[1]; f[4 * j + 2] = b[0]; f[4 * j + 3] = b[1];
    }
  }
};

// grid (n_work, ceil(K / KM_SLAB)), KM_SLAB / EL threads: thread t owns columns slab * KM_SLAB + t * EL .. + EL - 1.
template <int ST, class A>
__global__ __launch_bounds__(KM_SLAB / KmGroup<ST>::EL) void cell_sums_kernel(KmSumArgs<A> a) {
  using G = KmGroup<ST>;
  using S = typename A::T;
  using T = typename G::T;
  constexpr int EL = G::EL;
  const int tid = threadIdx.x, K = a.K, M = a.M;
  const int64_t piece = blockIdx.x;
  int first = a.work[piece * 3 + 1], end = a.work[piece * 3 + 2];
  if (first < 0 || end > a.n_items || end <= first || end - first > KM_PIECE) first = end = 0;  // no work: a zero row
  const int col = blockIdx.y * KM_SLAB + tid * EL;
  if (col < K) {
    const T* g = (const T*)a.g + col;
    S acc[EL];
#pragma unroll
    for (int j = 0; j < EL; ++j) acc[j] = 0;
    for (int r = first; r < end; r += KM_ROWS) {  // block-uniform
      int64_t item[KM_ROWS];
      u32x4 v[KM_ROWS];
#pragma unroll
      for (int u = 0; u < KM_ROWS; ++u) {
        const int64_t it = r + u < end ? a.items[r + u] : -1;
        item[u] = (it >= 0 && it < a.NV) ? it : -1;
      }
#pragma unroll
      for (int u = 0; u < KM_ROWS; ++u) v[u] = *(const u32x4*)(g + (item[u] < 0 ? 0 : item[u]) * K);  // none: row 0, discarded
#pragma unroll
      for (int u = 0; u < KM_ROWS; ++u) {
        if (item[u] < 0) continue;  // block-uniform
        float f[EL];
        G::widen(v[u], f);
        if constexpr (ST == MMT_SEARCH_FP8) {
          const float sc = a.gscale[item[u]];
#pragma unroll
          for (int j = 0; j < EL; ++j) f[j] = tk_mul_rn(f[j], sc);  // exact: a power of two
        }
#pragma unroll
        for (int j = 0; j < EL; ++j) acc[j] = a.acc.add(acc[j], f[j]);
      }
    }
    S* out = a.ws + piece * K + col;
    if constexpr (std::is_same_v<S, float>) {
#pragma unroll
      for (int j = 0; j < EL; j += 4) *(f32x4*)(out + j) = f32x4{acc[j], acc[j + 1], acc[j + 2], acc[j + 3]};
    } else {
#pragma unroll
      for (int j = 0; j < EL; j += 2) *(i64x2*)(out + j) = i64x2{acc[j], acc[j + 1]};
    }
  }
  if (blockIdx.y == 0 && tid < M) {  // the weights, by the same rule: thread m owns column m
    S acc = 0;
    for (int r = first; r < end; r += KM_ROWS) {
      int64_t item[KM_ROWS];
      float w[KM_ROWS];
#pragma unroll
      for (int u = 0; u < KM_ROWS; ++u) {
        const int64_t it = r + u < end ? a.items[r + u] : -1;
        item[u] = (it >= 0 && it < a.NV) ? it : -1;
      }
#pragma unroll
      for (int u = 0; u < KM_ROWS; ++u) w[u] = a.gw[(item[u] < 0 ? 0 : item[u]) * M + tid];
#pragma unroll
      for (int u = 0; u < KM_ROWS; ++u)
        if (item[u] >= 0) acc = a.wacc.add(acc, w[u]);
    }
    a.wws[piece * M + tid] = acc;
  }
}

// The centroid of one cell from its fp32 sums, by the block of 4 waves that owns the cell: wave w takes the experts w,
// w + 4, ..., lane l the elements l, l + 64, ... of each.  src.sum(column) / src.wsum(m) give the cell's fp32 sums --
// joined from the partial rows, or converted from the exact integers: everything behind them is this one body.
template <class SRC>
__device__ __forceinline__ void km_centroid_block(const SRC& src, int64_t c, int64_t n, bool centroid, float* all_sums,
                                                  float* wsums, float* embds, float* weights, int M, int d) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, K = M * d;
  float* sums = all_sums + c * K;
  for (int m = wave; m < M; m += 4) {  // wave-uniform
    float sq = 0.f;
    for (int j = lane; j < d; j += 64) {
      const float s = src.sum(m * d + j);
      sums[m * d + j] = s;
      sq = __builtin_fmaf(s, s, sq);
    }
    if (!centroid) continue;
#pragma unroll
    for (int o = 32; o; o >>= 1) sq = tk_add_rn(sq, __shfl_xor(sq, o));
    const float norm = sq > 0.f ? km_sqrt(sq) : 0.f;
    float* e = embds + c * K + m * d;
    for (int j = lane; j < d; j += 64) e[j] = norm > 0.f ? km_div_rn(sums[m * d + j], norm) : 0.f;  // its own write, read back
  }
  if (tid < M) {
    const float w = src.wsum(tid);
    wsums[c * M + tid] = w;
    if (centroid) weights[c * M + tid] = km_div_rn(w, (float)n);
  }
}

struct KmCentroidArgs {
  const float* ws;             // [n_work][K]
  const float* wws;            // [n_work][M]
  const int32_t* piece_start;  // [C + 1]: cell c's partial rows are piece_start[c] .. piece_start[c + 1] - 1
  const int64_t* offsets;      // [C + 1]
  float* sums;                 // [C][K]
  float* wsums;                // [C][M]
  float* embds;                // [C][K], in/out, or null
  float* weights;              // [C][M], in/out, or null
  int n_work, n_items, M, d;
};

// The fp32 sums of a cell: its partial rows p0 .. p1 - 1 added in ascending order from +0.
struct KmJoined {
  const float *ws, *wws;
  int p0, p1, K, M;
  __device__ __forceinline__ float sum(int col) const {
    float s = 0.f;
    for (int p = p0; p < p1; ++p) s = tk_add_rn(s, ws[(int64_t)p * K + col]);
    return s;
  }
  __device__ __forceinline__ float wsum(int m) const {
    float w = 0.f;
    for (int p = p0; p < p1; ++p) w = tk_add_rn(w, wws[(int64_t)p * M + m]);
    return w;
  }
};

// One block of 4 waves per cell.
__global__ __launch_bounds__(256) void cell_centroids_kernel(KmCentroidArgs a) {
  const int64_t c = blockIdx.x;
  int p0 = a.piece_start[c], p1 = a.piece_start[c + 1];
  const int64_t o0 = a.offsets[c], o1 = a.offsets[c + 1];
  const bool ok = p0 >= 0 && p1 >= p0 && p1 <= a.n_work && o0 >= 0 && o1 >= o0 && o1 <= a.n_items;
  if (!ok) p0 = p1 = 0;
  const int64_t n = ok ? o1 - o0 : 0;
  const bool centroid = a.embds && n > 0 && p1 > p0;  // an empty cell keeps what the buffers hold
  const KmJoined src = {a.ws, a.wws, p0, p1, a.M * a.d, a.M};
  km_centroid_block(src, c, n, centroid, a.sums, a.wsums, a.embds, a.weights, a.M, a.d);
}

struct KmJoinArgs {
  const long long* ws;         // [n_work][K]
  const long long* wws;        // [n_work][M]
  const int32_t* piece_start;  // [C + 1]
  long long* sums;             // [C][K]
  long long* wsums;            // [C][M]
  int n_work, M, K;
};

// One block per cell: thread t adds the columns t, t + 256, ... of the cell's partial int64 rows, then the weights.  A
// cell whose piece range is not inside the workspace has no pieces: zeros.
__global__ __launch_bounds__(256) void cell_sums_join_kernel(KmJoinArgs a) {
  const int tid = threadIdx.x, K = a.K, M = a.M;
  const int64_t c = blockIdx.x;
  int p0 = a.piece_start[c], p1 = a.piece_start[c + 1];
  if (p0 < 0 || p1 < p0 || p1 > a.n_work) p0 = p1 = 0;
  for (int col = tid; col < K; col += 256) {
    long long s = 0;
    for (int p = p0; p < p1; ++p) s += a.ws[(int64_t)p * K + col];
    a.sums[c * K + col] = s;
  }
  if (tid < M) {
    long long w = 0;
    for (int p = p0; p < p1; ++p) w += a.wws[(int64_t)p * M + tid];
    a.wsums[c * M + tid] = w;
  }
}

struct KmExactCentroidArgs {
  const long long* isums;   // [C][K], possibly the sum of several shards' tensors
  const long long* iwsums;  // [C][M]
  const int64_t* offsets;   // [C + 1]
  float* sums;              // [C][K]
  float* wsums;             // [C][M]
  float* embds;             // [C][K], in/out, or null
  float* weights;           // [C][M], in/out, or null
  int n_items, M, d;
  int shift, wshift;        // E - B, wexponent - B
};

// The fp32 sums of a cell from its exact integers: ONE conversion int64 -> fp32, round to nearest even (never through
// fp64: that rounds twice), then the scaling by a power of two (v_ldexp_f32).
struct KmConverted {
  const long long *isums, *iwsums;
  int shift, wshift;
  __device__ __forceinline__ float sum(int col) const { return __builtin_ldexpf(__ll2float_rn(isums[col]), shift); }
  __device__ __forceinline__ float wsum(int m) const { return __builtin_ldexpf(__ll2float_rn(iwsums[m]), wshift); }
};

__global__ __launch_bounds__(256) void cell_centroids_exact_kernel(KmExactCentroidArgs a) {
  const int64_t c = blockIdx.x;
  const int64_t o0 = a.offsets[c], o1 = a.offsets[c + 1];
  const bool ok = o0 >= 0 && o1 >= o0 && o1 <= a.n_items;
  const int64_t n = ok ? o1 - o0 : 0;
  const bool centroid = a.embds && n > 0;  // an empty cell keeps what the buffers hold
  const KmConverted src = {a.isums + c * a.M * a.d, a.iwsums + c * a.M, a.shift, a.wshift};
  km_centroid_block(src, c, n, centroid, a.sums, a.wsums, a.embds, a.weights, a.M, a.d);
}

struct KmMaxArgs {
  const void* g;        // [NV][K]
  const float* gw;      // [NV][M]
  const float* gscale;  // [NV], fp8 only
  float* out;           // [2][n_blocks]: the blocks' maxima of |f|, then of |gw|
  int64_t groups;       // NV * K / EL 16-byte groups
  int64_t n_weights;    // NV * M
  int K;
};

// grid n_blocks, 256 threads, grid-stride over the 16-byte groups of the stored rows and over the weights.  A group lies
// inside one row (K is a multiple of EL), so on fp8 its largest |code| times the row's scale is its largest |f|: the
// product is exact and the scale positive.  Every block writes its two slots; a maximum does not depend on the order.
template <int ST>
__global__ __launch_bounds__(256) void absmax_kernel(KmMaxArgs a) {
  using G = KmGroup<ST>;
  constexpr int EL = G::EL;
  __shared__ float part[2][4];
  const int tid = threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * 256;
  float mx = 0.f, wmx = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + tid; i < a.groups; i += stride) {
    float f[EL];
    G::widen(((const u32x4*)a.g)[i], f);
    float m = 0.f;
#pragma unroll
    for (int j = 0; j < EL; ++j) m = fmaxf(m, fabsf(f[j]));
    if constexpr (ST == MMT_SEARCH_FP8) m = tk_mul_rn(m, fabsf(a.gscale[i * EL / a.K]));
    mx = fmaxf(mx, m);
  }
  for (int64_t i = (int64_t)blockIdx.x * 256 + tid; i < a.n_weights; i += stride) wmx = fmaxf(wmx, fabsf(a.gw[i]));
#pragma unroll
  for (int o = 32; o; o >>= 1) {
    mx = fmaxf(mx, __shfl_xor(mx, o));
    wmx = fmaxf(wmx, __shfl_xor(wmx, o));
  }
  if ((tid & 63) == 0) {
    part[0][tid >> 6] = mx;
    part[1][tid >> 6] = wmx;
  }
  __syncthreads();
  if (tid < 2)
    a.out[(int64_t)tid * gridDim.x + blockIdx.x] = fmaxf(fmaxf(part[tid][0], part[tid][1]), fmaxf(part[tid][2], part[tid][3]));
}

namespace {
bool km_shape_ok(int storage, int NV, int M, int d) {
  return (unsigned)storage <= MMT_SEARCH_FP8 &&
         tk_shape_ok(1, NV, M, d, storage != MMT_SEARCH_FP32, storage == MMT_SEARCH_FP8);
}

// The operand checks the sum entries share: MMT_ERR_ARG, MMT_ERR_ALIGN or 0.
int km_sums_ok(const void* g, const float* gw, const float* gscale, int storage, int NV, int M, int d, const int64_t* items,
               int n_items, const int32_t* work, int n_work, const void* ws) {
  if (!g || !gw || !items || !work || !ws || !km_shape_ok(storage, NV, M, d) ||
      (storage == MMT_SEARCH_FP8) != (gscale != nullptr) || n_items < 1 || n_work < 1)
    return MMT_ERR_ARG;
  if ((int64_t)M * d >= (1ll << 31) / 16 || (int64_t)M * d > 65535ll * KM_SLAB) return MMT_ERR_ARG;  // the grid, the columns
  if (((uintptr_t)g | (uintptr_t)ws) & 15) return MMT_ERR_ALIGN;
  return 0;
}

bool km_scale_ok(int bits, int exponent, int wexponent) {
  return bits >= 1 && bits <= 61 && exponent >= -MMT_SEARCH_SUM_MAX_EXPONENT && exponent <= MMT_SEARCH_SUM_MAX_EXPONENT &&
         wexponent >= -MMT_SEARCH_SUM_MAX_EXPONENT && wexponent <= MMT_SEARCH_SUM_MAX_EXPONENT;
}

template <int ST, class A>
int km_sums_launch(const KmSumArgs<A>& a, int n_work, hipStream_t st) {
  const dim3 grid((unsigned)n_work, (unsigned)((a.K + KM_SLAB - 1) / KM_SLAB));
  hipLaunchKernelGGL((cell_sums_kernel<ST, A>), grid, dim3(KM_SLAB / KmGroup<ST>::EL), 0, st, a);
  return (int)hipGetLastError();
}

template <class A>
int km_sums_dispatch(int storage, const KmSumArgs<A>& a, int n_work, hipStream_t st) {
  switch (storage) {
    case MMT_SEARCH_FP32: return km_sums_launch<MMT_SEARCH_FP32>(a, n_work, st);
    case MMT_SEARCH_BF16: return km_sums_launch<MMT_SEARCH_BF16>(a, n_work, st);
    default: return km_sums_launch<MMT_SEARCH_FP8>(a, n_work, st);
  }
}

template <int ST>
int km_absmax_launch(const KmMaxArgs& a, int NV, int n_blocks, hipStream_t st) {
  KmMaxArgs b = a;
  b.groups = (int64_t)NV * a.K / KmGroup<ST>::EL;
  hipLaunchKernelGGL((absmax_kernel<ST>), dim3((unsigned)n_blocks), dim3(256), 0, st, b);
  return (int)hipGetLastError();
}
}  // namespace

extern "C" int64_t mmt_cell_sums_workspace_floats(int n_work, int M, int d) {
  if (n_work < 1 || M < 1 || M > MMT_MAX_EXPERTS || d < 1 || (d & 3)) return MMT_ERR_ARG;
  return (int64_t)n_work * M * (d + 1);
}

extern "C" int mmt_search_cell_sums(const void* g, const float* gw, const float* gscale, int storage, int NV, int M, int d,
                                    const int64_t* items, int n_items, const int32_t* work, int n_work, float* ws,
                                    void* stream) {
  if (const int bad = km_sums_ok(g, gw, gscale, storage, NV, M, d, items, n_items, work, n_work, ws)) return bad;
  const int K = M * d;
  const KmSumArgs<KmFloatAcc> a = {g, gw, gscale, items, work, ws, ws + (int64_t)n_work * K, NV, M, K, n_items, {}, {}};
  return km_sums_dispatch(storage, a, n_work, (hipStream_t)stream);
}

extern "C" int mmt_search_cell_centroids(const float* ws, int n_work, const int32_t* piece_start, const int64_t* offsets,
                                         int n_items, int C, int M, int d, float* sums, float* wsums, float* embds,
                                         float* weights, void* stream) {
  if (!ws || !piece_start || !offsets || !sums || !wsums || (embds == nullptr) != (weights == nullptr) || n_work < 1 ||
      n_items < 1 || C < 1 || M < 1 || M > MMT_MAX_EXPERTS || d < 1 || (d & 3) || (int64_t)M * d >= (1ll << 31) / 16)
    return MMT_ERR_ARG;
  if ((uintptr_t)ws & 15) return MMT_ERR_ALIGN;
  const KmCentroidArgs a = {ws, ws + (int64_t)n_work * M * d, piece_start, offsets, sums, wsums, embds, weights, n_work,
                            n_items, M, d};
  hipLaunchKernelGGL(cell_centroids_kernel, dim3((unsigned)C), dim3(256), 0, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

extern "C" int mmt_search_absmax(const void* g, const float* gw, const float* gscale, int storage, int NV, int M, int d,
                                 float* out, int n_blocks, void* stream) {
  if (!g || !gw || !out || !km_shape_ok(storage, NV, M, d) || (storage == MMT_SEARCH_FP8) != (gscale != nullptr) ||
      n_blocks < 1 || n_blocks > 65535 || (int64_t)M * d >= (1ll << 31) / 16)
    return MMT_ERR_ARG;
  if ((uintptr_t)g & 15) return MMT_ERR_ALIGN;
  const KmMaxArgs a = {g, gw, gscale, out, 0, (int64_t)NV * M, M * d};
  const hipStream_t st = (hipStream_t)stream;
  switch (storage) {
    case MMT_SEARCH_FP32: return km_absmax_launch<MMT_SEARCH_FP32>(a, NV, n_blocks, st);
    case MMT_SEARCH_BF16: return km_absmax_launch<MMT_SEARCH_BF16>(a, NV, n_blocks, st);
    default: return km_absmax_launch<MMT_SEARCH_FP8>(a, NV, n_blocks, st);
  }
}

extern "C" int64_t mmt_cell_sums_exact_workspace_bytes(int n_work, int M, int d) {
  if (n_work < 1 || M < 1 || M > MMT_MAX_EXPERTS || d < 1 || (d & 3)) return MMT_ERR_ARG;
  return (int64_t)n_work * M * (d + 1) * 8;
}

extern "C" int mmt_search_cell_sums_exact(const void* g, const float* gw, const float* gscale, int storage, int NV, int M,
                                          int d, const int64_t* items, int n_items, const int32_t* work, int n_work,
                                          const int32_t* piece_start, int C, int bits, int exponent, int wexponent,
                                          int64_t* ws, int64_t* sums, int64_t* wsums, void* stream) {
  if (!piece_start || !sums || !wsums || C < 1 || !km_scale_ok(bits, exponent, wexponent)) return MMT_ERR_ARG;
  if (const int bad = km_sums_ok(g, gw, gscale, storage, NV, M, d, items, n_items, work, n_work, ws)) return bad;
  const int K = M * d;
  const double limit = std::ldexp(1.0, bits);
  long long* w = (long long*)ws;
  const KmSumArgs<KmFixedAcc> a = {g, gw, gscale, items, work, w, w + (int64_t)n_work * K, NV, M, K, n_items,
                                   {std::ldexp(1.0, bits - exponent), limit}, {std::ldexp(1.0, bits - wexponent), limit}};
  const hipStream_t st = (hipStream_t)stream;
  if (const int err = km_sums_dispatch(storage, a, n_work, st)) return err;
  const KmJoinArgs j = {w, w + (int64_t)n_work * K, piece_start, (long long*)sums, (long long*)wsums, n_work, M, K};
  hipLaunchKernelGGL(cell_sums_join_kernel, dim3((unsigned)C), dim3(256), 0, st, j);
  return (int)hipGetLastError();
}

extern "C" int mmt_search_cell_centroids_exact(const int64_t* sums, const int64_t* wsums, const int64_t* offsets,
                                               int n_items, int C, int M, int d, int bits, int exponent, int wexponent,
                                               float* fsums, float* fwsums, float* embds, float* weights, void* stream) {
  if (!sums || !wsums || !offsets || !fsums || !fwsums || (embds == nullptr) != (weights == nullptr) || n_items < 1 ||
      C < 1 || M < 1 || M > MMT_MAX_EXPERTS || d < 1 || (d & 3) || (int64_t)M * d >= (1ll << 31) / 16 ||
      !km_scale_ok(bits, exponent, wexponent))
    return MMT_ERR_ARG;
  const KmExactCentroidArgs a = {(const long long*)sums, (const long long*)wsums, offsets, fsums, fwsums, embds, weights,
                                 n_items, M, d, exponent - bits, wexponent - bits};
  hipLaunchKernelGGL(cell_centroids_exact_kernel, dim3((unsigned)C), dim3(256), 0, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

