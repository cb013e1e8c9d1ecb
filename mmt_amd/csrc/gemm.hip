// bf16 MFMA GEMMs for the MMT hot path (gfx950).
//
//   gemm_nt : C[M,N] = A[M,K] . B[N,K]^T      forward Linear + input-gradient GEMMs, fused epilogues
//   gemm_tn : C[N,K2] = A[rows,N]^T . B[rows,K2]   weight gradients (contraction over tokens)
//
// Structure (both): 256 threads = 4 waves (2x2), 128x{128,64} block tile, BK = 64, double-buffered
// LDS filled by LDS-DMA (global_load_lds_dwordx4, 1 KiB per wave-instruction, no VGPR round trip).
// The LDS image is lane-linear, so the bank-conflict XOR swizzle is applied to the per-lane SOURCE
// address and again on the fragment read (cdna guide 5.4 rule 21).
//   NT: rows are 128 B (8 x 16 B chunks); chunk c of row r lives at chunk c ^ (r & 7); fragments are
//       ds_read_b128.
//   TN: rows are 256 B (16 chunks); chunk c of row r lives at c ^ ((r & 7) << 1); fragments are two
//       ds_read_b64_tr_b16 (hardware 4x16 transpose) because the contraction index is the ROW.
// MFMA operands are swapped (a = B-side fragment) so each lane ends up with 4 consecutive output
// columns of one row: 8/16-byte stores instead of 2-byte scatters.
#include "mmt_common.h"
#include "../../include/mmt_hip.h"

#define BK 64

template <int R>
__device__ __forceinline__ void stage_nt(const bf16_t* __restrict__ G, int64_t ld, int row0, int k0,
                                         bf16_t* lds_tile, int wave, int lane) {
#pragma unroll
  for (int i = 0; i < R / 32; ++i) {
    const int rbase = (wave * (R / 32) + i) * 8;  // 8 rows of 128 B per wave-instruction
    const int r = rbase + (lane >> 3);
    const int c = (lane & 7) ^ (r & 7);
    const bf16_t* src = G + (int64_t)(row0 + r) * ld + k0 + c * 8;
    __builtin_amdgcn_global_load_lds(GLB_PTR(src), LDS_PTR(lds_tile + rbase * BK), 16, 0, 0);
  }
}

template <int BM, int BN, int EPI>
__global__ __launch_bounds__(256, 2) void gemm_nt_kernel(
    const bf16_t* __restrict__ A, int64_t lda, const bf16_t* __restrict__ B, int64_t ldb,
    void* __restrict__ Cout, int64_t ldc, int M, int N, int K, MmtEpilogue epi,
    const int32_t* __restrict__ n_rows_dev) {
  constexpr int MI = BM / 32, NI = BN / 32;  // 16x16 fragments per wave in m / n
  __shared__ __attribute__((aligned(16))) bf16_t smem[2 * (BM + BN) * BK];
  const int tiles_n = N / BN;
  const int nrows = n_rows_dev ? *n_rows_dev : M;
  // variable-length packing: remap over the LIVE tiles only, so that every XCD gets live work (see gemm2.hip)
  const int live_tiles = min((int)gridDim.x, ((min(nrows, M) + BM - 1) / BM) * tiles_n);
  if ((int)blockIdx.x >= live_tiles) {  // dead tile: contributes zeros to the column sums
    if constexpr (EPI == MMT_EPI_DGELU) {
      const int dtm = (int)blockIdx.x / tiles_n, dn0 = ((int)blockIdx.x % tiles_n) * BN;
      if (epi.colsum && threadIdx.x < BN) epi.colsum[(int64_t)dtm * N + dn0 + threadIdx.x] = 0.f;
    }
    return;
  }
  const int id = xcd_remap(blockIdx.x, live_tiles);
  const int tm = id / tiles_n, tn = id % tiles_n;
  const int m0 = tm * BM, n0 = tn * BN;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int li = lane & 15, lg = lane >> 4;

  f32x4 acc[MI][NI];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NI; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  constexpr int STAGE = (BM + BN) * BK;  // elements per pipeline stage: [A tile | B tile]

  const int KT = K / BK;
  stage_nt<BM>(A, lda, m0, 0, smem, wave, lane);
  stage_nt<BN>(B, ldb, n0, 0, smem + BM * BK, wave, lane);
  for (int kt = 0; kt < KT; ++kt) {
    const int cur = kt & 1;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (kt + 1 < KT) {
      stage_nt<BM>(A, lda, m0, (kt + 1) * BK, smem + (cur ^ 1) * STAGE, wave, lane);
      stage_nt<BN>(B, ldb, n0, (kt + 1) * BK, smem + (cur ^ 1) * STAGE + BM * BK, wave, lane);
    }
    const bf16_t* as = smem + cur * STAGE;
    const bf16_t* bs = as + BM * BK;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8_t af[MI], bfr[NI];
      const int c = ks * 4 + lg;
#pragma unroll
      for (int i = 0; i < MI; ++i) {
        const int r = wm * (BM / 2) + i * 16 + li;
        af[i] = *(const bf16x8_t*)(as + r * BK + ((c ^ (r & 7)) << 3));
      }
#pragma unroll
      for (int j = 0; j < NI; ++j) {
        const int r = wn * (BN / 2) + j * 16 + li;
        bfr[j] = *(const bf16x8_t*)(bs + r * BK + ((c ^ (r & 7)) << 3));
      }
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfr[j], af[i], acc[i][j], 0, 0, 0);
    }
  }

  // ---- epilogue: lane (li, lg), reg r holds C[row(i, li)][col(j, lg) + r] ----
  float csum[NI][4];
  if constexpr (EPI == MMT_EPI_DGELU) {
#pragma unroll
    for (int j = 0; j < NI; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) csum[j][r] = 0.f;
  }
#pragma unroll
  for (int i = 0; i < MI; ++i) {
    const int row = m0 + wm * (BM / 2) + i * 16 + li;
    const bool row_ok = row < M;
#pragma unroll
    for (int j = 0; j < NI; ++j) {
      const int col = n0 + wn * (BN / 2) + j * 16 + lg * 4;
      f32x4 v = acc[i][j];
      if constexpr (EPI == MMT_EPI_BIAS_BF16 || EPI == MMT_EPI_BIAS_GELU ||
                    EPI == MMT_EPI_BIAS_DROP_RES || EPI == MMT_EPI_BIAS_F32) {
        const f32x4 b = *(const f32x4*)(epi.bias + col);
        v += b;
      }
      if (!row_ok) continue;
      if constexpr (EPI == MMT_EPI_BF16 || EPI == MMT_EPI_BIAS_BF16) {
        u32x2 o = {pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3])};
        *(u32x2*)((bf16_t*)Cout + (int64_t)row * ldc + col) = o;
      } else if constexpr (EPI == MMT_EPI_BIAS_GELU) {
        u32x2 o = {pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3])};
        *(u32x2*)((bf16_t*)Cout + (int64_t)row * ldc + col) = o;
        // GELU is evaluated on the bf16-rounded pre-activation so that backward (which only has
        // the stored bf16 value) differentiates exactly the function that was applied.
        float p0 = bf2f((bf16_t)(o[0] & 0xffff)), p1 = bf2f((bf16_t)(o[0] >> 16));
        float p2 = bf2f((bf16_t)(o[1] & 0xffff)), p3 = bf2f((bf16_t)(o[1] >> 16));
        u32x2 g = {pack_bf2(gelu_erf_f(p0), gelu_erf_f(p1)), pack_bf2(gelu_erf_f(p2), gelu_erf_f(p3))};
        *(u32x2*)((bf16_t*)epi.out2 + (int64_t)row * epi.ldout2 + col) = g;
      } else if constexpr (EPI == MMT_EPI_BIAS_DROP_RES) {
        if (epi.drop_thr16) {
          const int orow = epi.row_index ? epi.row_index[row] : row;
          bool k[4];
          keep4(eff_key(epi.drop_key, epi.seed_dev), (unsigned long long)orow * (unsigned)N + (unsigned)col, epi.drop_thr16, k);
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] = k[r] ? v[r] * epi.drop_scale : 0.f;
        }
        v += *(const f32x4*)(epi.res + (int64_t)row * epi.ldres + col);
        *(f32x4*)((float*)Cout + (int64_t)row * ldc + col) = v;
      } else if constexpr (EPI == MMT_EPI_DGELU) {
        const u32x2 a = *(const u32x2*)((const bf16_t*)epi.aux + (int64_t)row * epi.ldaux + col);
        v[0] *= gelu_erf_grad_f(bf2f((bf16_t)(a[0] & 0xffff)));
        v[1] *= gelu_erf_grad_f(bf2f((bf16_t)(a[0] >> 16)));
        v[2] *= gelu_erf_grad_f(bf2f((bf16_t)(a[1] & 0xffff)));
        v[3] *= gelu_erf_grad_f(bf2f((bf16_t)(a[1] >> 16)));
        u32x2 o = {pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3])};
        *(u32x2*)((bf16_t*)Cout + (int64_t)row * ldc + col) = o;
        if (row < nrows) {
          csum[j][0] += bf2f((bf16_t)(o[0] & 0xffff)); csum[j][1] += bf2f((bf16_t)(o[0] >> 16));
          csum[j][2] += bf2f((bf16_t)(o[1] & 0xffff)); csum[j][3] += bf2f((bf16_t)(o[1] >> 16));
        }
      } else if constexpr (EPI == MMT_EPI_ADD_F32) {
        v += *(const f32x4*)(epi.res + (int64_t)row * epi.ldres + col);
        *(f32x4*)((float*)Cout + (int64_t)row * ldc + col) = v;
      } else {  // MMT_EPI_F32 / MMT_EPI_BIAS_F32
        *(f32x4*)((float*)Cout + (int64_t)row * ldc + col) = v;
      }
    }
  }
  if constexpr (EPI == MMT_EPI_DGELU) {
    if (epi.colsum) {  // per-row-tile column sums of the bf16 output (-> bias gradient, deterministic)
      __syncthreads();
      float* red = (float*)smem;  // [2][BN]
#pragma unroll
      for (int j = 0; j < NI; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float s = csum[j][r];
          s += __shfl_xor(s, 1, 64); s += __shfl_xor(s, 2, 64);
          s += __shfl_xor(s, 4, 64); s += __shfl_xor(s, 8, 64);
          if (li == 0) red[wm * BN + wn * (BN / 2) + j * 16 + lg * 4 + r] = s;
        }
      __syncthreads();
      if (tid < BN) epi.colsum[(int64_t)tm * N + n0 + tid] = red[tid] + red[BN + tid];
    }
  }
}

// ------------------------------------------------------------------------------------------------
// TN: weight gradient.  Tiles: At[64 rows][128 n], Bt[64 rows][128 k2], both row-major 256-B rows.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void stage_tn(const bf16_t* __restrict__ G, int64_t ld, int row0, int c0,
                                         bf16_t* lds_tile, int wave, int lane) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int rbase = (wave * 4 + i) * 4;  // 4 rows of 256 B per wave-instruction
    const int r = rbase + (lane >> 4);
    const int c = (lane & 15) ^ ((r & 7) << 1);
    const bf16_t* src = G + (int64_t)(row0 + r) * ld + c0 + c * 8;
    __builtin_amdgcn_global_load_lds(GLB_PTR(src), LDS_PTR(lds_tile + rbase * 128), 16, 0, 0);
  }
}

// 8 contraction values for column `col` of a [64][128] tile, k-sub-step ks: lane group g gets rows
// ks*32 + 4g + {0..3} and ks*32 + 16 + 4g + {0..3} (same permutation for both operands).
__device__ __forceinline__ bf16x8_t tr_frag(const bf16_t* tile, int ks, int colbase, int lane) {
  const int t = lane & 15, g = lane >> 4;
  const int col = colbase + 4 * (t & 3);
  const int r0 = ks * 32 + 4 * g + (t >> 2);
  const int r1 = r0 + 16;
  const int ch = col >> 3, w = col & 7;
  const bf16_t* p0 = tile + r0 * 128 + ((ch ^ ((r0 & 7) << 1)) << 3) + w;
  const bf16_t* p1 = tile + r1 * 128 + ((ch ^ ((r1 & 7) << 1)) << 3) + w;
  bf16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) bf16x4_t*)LDS_PTR(p0));
  bf16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) bf16x4_t*)LDS_PTR(p1));
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

__global__ __launch_bounds__(256, 2) void gemm_tn_kernel(
    const bf16_t* __restrict__ A, int64_t lda, const bf16_t* __restrict__ B, int64_t ldb,
    float* __restrict__ ws, int rows, int N, int K2, int splits,
    const int32_t* __restrict__ n_rows_dev) {
  __shared__ __attribute__((aligned(16))) bf16_t smem[2 * 2 * 64 * 128];
  const int tiles_k = K2 / 128, tiles = (N / 128) * tiles_k;
  const int id = xcd_remap(blockIdx.x, gridDim.x);
  const int split = id / tiles, tile = id % tiles;
  const int n0 = (tile / tiles_k) * 128, k0 = (tile % tiles_k) * 128;
  const int nrows = n_rows_dev ? min(*n_rows_dev, rows) : rows;
  const int ktiles = (nrows + 63) / 64;
  const int per = (ktiles + splits - 1) / splits;
  const int kt_begin = split * per, kt_end = min(ktiles, kt_begin + per);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int li = lane & 15, lg = lane >> 4;
  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  constexpr int TSTAGE = 2 * 64 * 128;  // [A tile | B tile] per stage

  if (kt_begin < kt_end) {
    stage_tn(A, lda, kt_begin * 64, n0, smem, wave, lane);
    stage_tn(B, ldb, kt_begin * 64, k0, smem + 64 * 128, wave, lane);
  }
  for (int kt = kt_begin; kt < kt_end; ++kt) {
    const int cur = (kt - kt_begin) & 1;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (kt + 1 < kt_end) {
      stage_tn(A, lda, (kt + 1) * 64, n0, smem + (cur ^ 1) * TSTAGE, wave, lane);
      stage_tn(B, ldb, (kt + 1) * 64, k0, smem + (cur ^ 1) * TSTAGE + 64 * 128, wave, lane);
    }
    bf16_t* at = smem + cur * TSTAGE;
    bf16_t* bt = at + 64 * 128;
    const int live = nrows - kt * 64;  // rows of this tile that exist
    if (live < 64) {                   // ragged tail: zero dead rows of both operands
      for (int e = tid; e < (64 - live) * 32; e += 256) {
        const int r = live + e / 32, q = e % 32;  // 32 x 16-B per pair of row images
        u32x4 z = {0, 0, 0, 0};
        if (q < 16) *(u32x4*)(at + r * 128 + q * 8) = z;
        else *(u32x4*)(bt + r * 128 + (q - 16) * 8) = z;
      }
      __syncthreads();
    }
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8_t af[4], bfr[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) af[i] = tr_frag(at, ks, wm * 64 + i * 16, lane);
#pragma unroll
      for (int j = 0; j < 4; ++j) bfr[j] = tr_frag(bt, ks, wn * 64 + j * 16, lane);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfr[j], af[i], acc[i][j], 0, 0, 0);
    }
  }
  float* out = ws + (int64_t)split * N * K2;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int n = n0 + wm * 64 + i * 16 + li;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int k2 = k0 + wn * 64 + j * 16 + lg * 4;
      *(f32x4*)(out + (int64_t)n * K2 + k2) = acc[i][j];
    }
  }
}

// ------------------------------------------------------------------------------------------------
// Grouped weight gradients: every weight (and bias) gradient of one encoder layer -- or of all ReduceDim
// experts -- in ONE launch.  Each block owns one 128x128 tile of one dW and contracts over ALL live rows, so
// there are no split-K slabs and no reduce kernels; with d=512, I=3072 a layer has exactly
// 48 + 16 + 96 + 96 = 256 tiles = one per CU.  Tiles in the first tile-column also produce the bias gradient
// (column sums of the bf16 dY operand) with one extra MFMA per fragment against an all-ones operand.
// ------------------------------------------------------------------------------------------------
// Transpose reads issued from inline asm.  The compiler cannot tell an LDS-DMA write from the LDS location a transpose
// read touches and drains vmcnt to ZERO in front of every builtin ds_read_tr that follows a global_load_lds -- i.e. it
// waits for the prefetches of later units as well.  Issued this way the reads are invisible to that analysis; the price
// is that their completion has to be waited for by hand (TR_WAIT ties the loaded registers to the s_waitcnt so that no
// consumer can be scheduled above it).
// Both halves of one fragment (rows r0 and r0 + 16 of the same 16-byte chunk: the swizzle repeats every 8 rows, so the
// second read is the first one's address + 16 rows = 4096 bytes, an instruction immediate).
__device__ __forceinline__ void tr_frag_issue(u32x2& lo, u32x2& hi, unsigned addr) {
  asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(lo) : "v"(addr));
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:4096" : "=v"(hi) : "v"(addr));
}
// LDS byte offset (inside a [64][128] bf16 tile) of the first half of the fragment for columns colbase .. colbase + 15,
// k-sub-step ks.  Fragments 16 columns further on are this offset XOR 32 per step (two 16-byte chunks: the chunk index is
// XOR-swizzled, and colbase only sets bits the swizzle leaves alone in a multiple of 64).
__device__ __forceinline__ unsigned tr_frag_offset(int ks, int colbase, int lane) {
  const int t = lane & 15, g = lane >> 4;
  const int col = colbase + 4 * (t & 3);
  const int r0 = ks * 32 + 4 * g + (t >> 2);
  const int ch = col >> 3, w = col & 7;
  return (unsigned)((r0 * 128 + ((ch ^ ((r0 & 7) << 1)) << 3) + w) * 2);
}
#define TR_TIE4(x) "+v"(x[0]), "+v"(x[1]), "+v"(x[2]), "+v"(x[3])
__device__ __forceinline__ bf16x8_t tr_join(const u32x2& lo, const u32x2& hi) {
  const u32x4 v = {lo[0], lo[1], hi[0], hi[1]};
  return __builtin_bit_cast(bf16x8_t, v);
}

#define WGRAD_LISTED (1 << 30)  // MmtWgradItem.reserved2: see wgrad_phased_kernel's block order
#ifdef MMT_GEMM2_INSTR
__device__ long long* g_wgrad_dbg = nullptr;  // instrumented build only: per-block cycle counters
extern "C" int mmt_debug_set_wgrad_buffer(void* p) {
  return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_wgrad_dbg), &p, sizeof(p));
}
#define WTICK(acc) do { const long long tn_ = clock64(); acc += tn_ - tp; tp = tn_; } while (0)
#else
#define WTICK(acc) do {} while (0)
#endif

// ------------------------------------------------------------------------------------------------
// Eight waves per tile, as two groups of four in OPPOSITE phase, with 64 x 128 wave tiles.
//   * The 64-row units of the contraction alternate between the groups: unit u belongs to group u & 1 and lives in stage
//     u & 3 of ONE four-deep ring.  In half-step h, group h & 1 runs the transpose reads + MFMAs of unit h while the other
//     group issues the LDS-DMA loads of unit h + 3 (its own next but one): the ~90 cycles a global_load_lds stalls its wave
//     at issue hide under the other group's MFMAs, loads have two half-steps to land (counted vmcnt: a group waits for
//     its OWN loads), and one workgroup barrier per half-step orders both hazards (unit h has landed; the stage of unit
//     h - 1 is free).
//   * What then bounds a half-step is LDS read bandwidth: ds_read_b64_tr_b16 delivers ~64 B/clk/CU, and four 64 x 64 wave
//     tiles read 64 KiB per unit (measured on r02's lock-step kernel: 1620 cycles per unit against 544 cycles of MFMA).  The
//     four waves of a group therefore split the unit 2 (32-row halves = the two k-sub-steps) x 2 (halves of the tile's
//     128 dW rows): a wave computes 64 x 128 outputs over 32 rows from 4 + 8 fragments (48 KiB per unit, -25 %), at the
//     price of four partial tiles per output (2 groups x 2 row halves) summed through LDS at the end, in a fixed order.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(512) void wgrad_phased_kernel(MmtWgradGroup g) {
  extern __shared__ __attribute__((aligned(16))) unsigned char wg_smem[];
#ifdef MMT_GEMM2_INSTR
  const long long t_entry = clock64();
#endif
  bf16_t* smem = (bf16_t*)wg_smem;  // ring: 4 units x [A 64x128 | B 64x128]
  // Block -> (item, tile, split).  Launches whose blocks all run equally long take ONE XCD-aware remap over the whole grid:
  // an XCD then works on ~32 consecutive tiles of one item.  Launches that mix long and short blocks (row splits, compact
  // items: WGRAD_LISTED, set by the host, which has also sorted the items longest blocks first) keep the item order as the
  // DISPATCH order and remap inside each item instead: workgroups go to the XCDs round-robin, so every XCD starts on its
  // eighth of the long blocks and fills up with short ones as CUs come free.  One remap over the whole grid hands the
  // first XCDs nothing but long blocks, two rounds deep, while the others run out of work (the last layer's launch:
  // 192 blocks of 15 units + 208 of 4 on 256 CUs took what 30 units take).
  const bool listed = (g.item[0].reserved2 & WGRAD_LISTED) != 0;
  const int id = listed ? (int)blockIdx.x : xcd_remap(blockIdx.x, gridDim.x);
  int p = 0;
#pragma unroll 1
  for (int q = 1; q < g.count; ++q)
    if (id >= g.item[q].tile_begin) p = q;
  const MmtWgradItem& it = g.item[p];
  const bf16_t* __restrict__ A = (const bf16_t*)it.A;
  const bf16_t* __restrict__ B = (const bf16_t*)it.B;
  const int64_t lda = it.lda, ldb = it.ldb;
  const int nsplit = it.splits > 1 ? it.splits : 1;
  const int tiles_k = it.K2 / 128;
  // (listed: the item's blocks that share an XCD are those of one residue of the local index -- a contiguous run of its ids)
  const int local = listed ? xcd_remap(id - it.tile_begin, (it.N / 128) * tiles_k * nsplit) : id - it.tile_begin;
  const int tile = local / nsplit, split = local % nsplit;
  // Tile order inside an item: patches of PN x PK tiles (reserved2 = PN << 16 | PK, chosen by the host so that PN * PK is
  // about the 32 consecutive ids one XCD receives): the tiles that share an L2 then share as few distinct operand panels
  // as possible (8 x 4 or 4 x 8 tiles = 12 panels; a row-major run over a 4 x 24 grid = 34).
  int tn, tk;
  {
    const int PN = (it.reserved2 >> 16) & 0xff, PK = it.reserved2 & 0xffff;
    if (PN > 0 && PK > 0) {
      const int per = PN * PK, patches_k = tiles_k / PK;
      const int patch = tile / per, within = tile % per;
      tn = (patch / patches_k) * PN + within / PK;
      tk = (patch % patches_k) * PK + within % PK;
    } else {
      tn = tile / tiles_k;
      tk = tile % tiles_k;
    }
  }
  const int n0 = tn * 128, k0 = tk * 128;
  // item.reserved > 0: this item contracts over exactly that many rows (compact last-layer buffers)
  const int nrows = it.reserved > 0 ? it.reserved
                    : it.n_rows_dev ? min(*it.n_rows_dev, g.rows)
                                    : (g.n_rows_dev ? min(*g.n_rows_dev, g.rows) : g.rows);
  const int units_all = (nrows + 63) / 64;  // 64-row units of the contraction
  // item.splits > 1: the units are divided among `splits` blocks per tile, each writing its own partial slab
  const int per_split = (units_all + nsplit - 1) / nsplit;
  const int u0 = split * per_split;
  const int units = max(0, min(units_all, u0 + per_split) - u0);

  const int tid = threadIdx.x, lane = tid & 63, wave8 = tid >> 6;
  const int kg = wave8 >> 2, wave = wave8 & 3;
  const int wk = wave >> 1, wt = wave & 1;  // row half of the unit (k-sub-step), half of the tile's 128 dW rows
  const int li = lane & 15, lg = lane >> 4;
  const bool want_bias = it.bias_out != nullptr && tk == 0;
  f32x4 acc[4][8], accb[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    accb[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  }
  bf16x8_t ones;
#pragma unroll
  for (int e = 0; e < 8; ++e) ones[e] = (__bf16)1.0f;
  constexpr int GSTAGE = 2 * 64 * 128;  // one unit's [A | B] tiles

  // Source addresses of this lane's 4 + 4 LDS-DMA instructions for unit 0; unit u is 64 u rows further on, a wave-uniform
  // byte offset -- one 64-bit add per instruction in the loop instead of the row x leading-dimension product (the issuing
  // wave's VALU work comes out of the issue slots of the computing wave on the same SIMD).
  const bf16_t *pa[4], *pb[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = (wave * 4 + i) * 4 + (lane >> 4);
    const int c = (lane & 15) ^ ((r & 7) << 1);
    pa[i] = A + (int64_t)(u0 * 64 + r) * lda + n0 + c * 8;
    pb[i] = B + (int64_t)(u0 * 64 + r) * ldb + k0 + c * 8;
  }
  const int64_t astep = 64 * lda, bstep = 64 * ldb;
  auto issue = [&](int u) {  // by the four waves of group u & 1
    if (u < units) {
      bf16_t* base = smem + (u & 3) * GSTAGE;
#pragma unroll
      for (int i = 0; i < 4; ++i)
        __builtin_amdgcn_global_load_lds(GLB_PTR(pa[i] + u * astep), LDS_PTR(base + (wave * 4 + i) * 4 * 128), 16, 0, 0);
#pragma unroll
      for (int i = 0; i < 4; ++i)
        __builtin_amdgcn_global_load_lds(GLB_PTR(pb[i] + u * bstep), LDS_PTR(base + 64 * 128 + (wave * 4 + i) * 4 * 128), 16, 0, 0);
    }
  };
  if (kg == 0) { issue(0); issue(2); } else { issue(1); }
  const unsigned aoff = tr_frag_offset(wk, wt * 64, lane), boff = tr_frag_offset(wk, 0, lane);
#ifdef MMT_GEMM2_INSTR
  long long t_wait = 0, t_bar = 0, t_issue = 0, t_comp = 0, t0 = clock64(), tp = t0;
#endif
  for (int h = 0; h < units; ++h) {
    const bool mine = (h & 1) == kg;
    WTICK(t_comp);  // (loop overhead + the tail of the previous half-step)
    if (mine) {
      // outstanding loads of this wave: unit h and (issued one half-step ago) unit h + 2, eight instructions each
      if (h + 2 < units) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    asm volatile("" ::: "memory");
    WTICK(t_wait);
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    WTICK(t_bar);
    bf16_t* at = smem + (h & 3) * GSTAGE;
    bf16_t* bt = at + 64 * 128;
    const int live = nrows - (u0 + h) * 64;  // rows of unit h that exist (> 0)
    if (live < 64) {  // ragged last unit (block-uniform): its group zeroes the dead rows of both operands
      if (mine) {
        for (int e = wave * 64 + lane; e < (64 - live) * 32; e += 256) {
          const int r = live + e / 32, q = e % 32;
          u32x4 z = {0, 0, 0, 0};
          if (q < 16) *(u32x4*)(at + r * 128 + q * 8) = z;
          else *(u32x4*)(bt + r * 128 + (q - 16) * 8) = z;
        }
      }
      __syncthreads();
    }
    if (!mine) {
      issue(h + 3);
      WTICK(t_issue);
      continue;
    }
    // transpose reads: the 4 A fragments and the first THREE pairs of B fragments go out at once, the fourth after the
    // first pair's MFMAs: an LDS round trip (~150-200 cycles) then hides behind two pairs of MFMAs (in-order returns:
    // "at most N outstanding" = everything issued before the last N reads has landed).  Measured with the MFMAs compiled
    // out: the reads' latency chain alone is 1040 of the 1400 cycles of a compute half-step when only one pair is in flight
    // ahead of the MFMAs.  (r05: the opposite split -- A and
    // the first B pair up front, pairs 1..3 behind the MFMAs of pairs 0 / 1, 12 instead of 20 reads in front of the first
    // MFMA -- measured identical: 46.8-47.0 vs 45.5-46.9 us per launch in the step's eager probes, same step time.)
    // One base address per operand; every fragment's address is that XOR a constant, formed right at the read (the asm
    // barrier keeps the compiler from hoisting 24 loop-invariant addresses into registers the accumulators need).
    u32x2 alo[4], ahi[4], blo[4][2], bhi[4][2];
    unsigned abase = (unsigned)(uintptr_t)LDS_PTR(at) + aoff, bbase = (unsigned)(uintptr_t)LDS_PTR(bt) + boff;
    asm volatile("" : "+v"(abase), "+v"(bbase));
#pragma unroll
    for (int i = 0; i < 4; ++i) tr_frag_issue(alo[i], ahi[i], abase ^ (unsigned)(i << 5));
#pragma unroll
    for (int q = 0; q < 3; ++q)
#pragma unroll
      for (int jj = 0; jj < 2; ++jj) tr_frag_issue(blo[q][jj], bhi[q][jj], bbase ^ (unsigned)((2 * q + jj) << 5));
    bf16x8_t af[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (q == 0) {  // outstanding allowed: pairs 1, 2
        asm volatile("s_waitcnt lgkmcnt(8)" : TR_TIE4(alo), TR_TIE4(ahi), "+v"(blo[0][0]), "+v"(bhi[0][0]), "+v"(blo[0][1]), "+v"(bhi[0][1]));
#pragma unroll
        for (int i = 0; i < 4; ++i) af[i] = tr_join(alo[i], ahi[i]);
      } else if (q == 1) {  // pairs 2, 3
        asm volatile("s_waitcnt lgkmcnt(8)" : "+v"(blo[1][0]), "+v"(bhi[1][0]), "+v"(blo[1][1]), "+v"(bhi[1][1]));
      } else if (q == 2) {  // pair 3
        asm volatile("s_waitcnt lgkmcnt(4)" : "+v"(blo[2][0]), "+v"(bhi[2][0]), "+v"(blo[2][1]), "+v"(bhi[2][1]));
      } else {
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(blo[3][0]), "+v"(bhi[3][0]), "+v"(blo[3][1]), "+v"(bhi[3][1]));
      }
#pragma unroll
      for (int jj = 0; jj < 2; ++jj) {
        const int j = 2 * q + jj;
        const bf16x8_t bfr = tr_join(blo[q][jj], bhi[q][jj]);
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfr, af[i], acc[i][j], 0, 0, 0);
      }
      if (q == 0) {
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) tr_frag_issue(blo[3][jj], bhi[3][jj], bbase ^ (unsigned)((6 + jj) << 5));
        if (want_bias) {
#pragma unroll
          for (int i = 0; i < 4; ++i) accb[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, af[i], accb[i], 0, 0, 0);
        }
      }
      __builtin_amdgcn_sched_barrier(0);  // (or the scheduler sinks this pair's MFMAs below the later waits)
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#ifdef MMT_GEMM2_INSTR
  asm volatile("s_nop 0" ::"v"(acc[0][0][0]), "v"(acc[3][7][3]));
  WTICK(t_comp);
  const long long t_loop_end = clock64();
  if (g_wgrad_dbg && (tid == 0 || tid == 256)) {  // wave 0 of either group
    long long* d = g_wgrad_dbg + ((int64_t)blockIdx.x * 2 + kg) * 8;
    d[0] = t_wait; d[1] = t_bar; d[2] = t_issue; d[3] = t_comp; d[4] = t_loop_end - t0; d[5] = units; d[6] = t0 - t_entry; d[7] = t_entry;
  }
#endif
  // ---- four partial tiles per output (group x row half), summed by two pairwise EXCHANGES through LDS so that all
  // eight waves stay busy and each ends up storing one eighth of the tile:
  //   round 1, (g, k0) <-> (g, k1): the k0 wave keeps dW rows i = 0, 1 of its 64, the k1 wave rows i = 2, 3;
  //   round 2, (0, k) <-> (1, k): the group-0 wave keeps columns j = 0..3, the group-1 wave j = 4..7.
  // Every output is (P00 + P01) + (P10 + P11) (fp32 addition commutes): deterministic, the same order everywhere. ----
  f32x4* xch = (f32x4*)wg_smem;  // round 1: 2 regions x [18][256] f32x4 = 144 KiB; round 2: 2 x [10][256]
  __syncthreads();
  {
    const int pid = (kg * 2 + wt) * 64 + lane;
    f32x4* to_k0 = xch;                 // written by the k1 waves: rows i = 0, 1 (+ their bias sums)
    f32x4* to_k1 = xch + 18 * 256;      // written by the k0 waves: rows i = 2, 3
    if (wk == 0) {
#pragma unroll
      for (int ii = 0; ii < 2; ++ii) {
#pragma unroll
        for (int j = 0; j < 8; ++j) to_k1[(ii * 8 + j) * 256 + pid] = acc[2 + ii][j];
        to_k1[(16 + ii) * 256 + pid] = accb[2 + ii];
      }
    } else {
#pragma unroll
      for (int ii = 0; ii < 2; ++ii) {
#pragma unroll
        for (int j = 0; j < 8; ++j) to_k0[(ii * 8 + j) * 256 + pid] = acc[ii][j];
        to_k0[(16 + ii) * 256 + pid] = accb[ii];
      }
    }
    __syncthreads();
    if (wk == 0) {
#pragma unroll
      for (int ii = 0; ii < 2; ++ii) {
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[ii][j] += to_k0[(ii * 8 + j) * 256 + pid];
        accb[ii] += to_k0[(16 + ii) * 256 + pid];
      }
    } else {
#pragma unroll
      for (int ii = 0; ii < 2; ++ii) {  // (kept in slots 0, 1 from here on: slot ii = row i = 2 + ii)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[ii][j] = acc[2 + ii][j] + to_k1[(ii * 8 + j) * 256 + pid];
        accb[ii] = accb[2 + ii] + to_k1[(16 + ii) * 256 + pid];
      }
    }
  }
  __syncthreads();
  {
    const int pid = (wk * 2 + wt) * 64 + lane;
    f32x4* to_g0 = xch;                 // written by the group-1 waves: columns j = 0..3 (+ bias sums)
    f32x4* to_g1 = xch + 10 * 256;      // written by the group-0 waves: columns j = 4..7
    if (kg == 0) {
#pragma unroll
      for (int ii = 0; ii < 2; ++ii)
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) to_g1[(ii * 4 + jj) * 256 + pid] = acc[ii][4 + jj];
    } else {
#pragma unroll
      for (int ii = 0; ii < 2; ++ii) {
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) to_g0[(ii * 4 + jj) * 256 + pid] = acc[ii][jj];
        to_g0[(8 + ii) * 256 + pid] = accb[ii];
      }
    }
    __syncthreads();
    if (kg == 0) {
#pragma unroll
      for (int ii = 0; ii < 2; ++ii) {
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) acc[ii][jj] += to_g0[(ii * 4 + jj) * 256 + pid];
        accb[ii] += to_g0[(8 + ii) * 256 + pid];
      }
    } else {
#pragma unroll
      for (int ii = 0; ii < 2; ++ii)
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) acc[ii][jj] = acc[ii][4 + jj] + to_g1[(ii * 4 + jj) * 256 + pid];
    }
  }
  // this wave now holds rows i = 2 wk + ii (ii = 0, 1), columns j = 4 kg + jj (jj = 0..3) in acc[ii][jj]
  float* __restrict__ out = nsplit > 1 ? it.slab + (int64_t)split * it.N_out * it.ldo : it.out;
  float* __restrict__ bias_out = nsplit > 1 ? (it.bias_slab ? it.bias_slab + (int64_t)split * it.N_out : nullptr) : it.bias_out;
#pragma unroll
  for (int ii = 0; ii < 2; ++ii) {
    const int n = n0 + wt * 64 + (2 * wk + ii) * 16 + li;
    if (n >= it.N_out) continue;
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
      const int k2 = k0 + (4 * kg + jj) * 16 + lg * 4;
      if (k2 + 3 < it.K2_out && !(it.ldo & 3)) {
        *(f32x4*)(out + (int64_t)n * it.ldo + k2) = acc[ii][jj];
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (k2 + e < it.K2_out) out[(int64_t)n * it.ldo + k2 + e] = acc[ii][jj][e];
      }
    }
    if (want_bias && kg == 0 && lg == 0) bias_out[n] = accb[ii][0];
  }
#ifdef MMT_GEMM2_INSTR
  if (g_wgrad_dbg && tid == 0) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the stores have left the wave
    g_wgrad_dbg[((int64_t)blockIdx.x * 2 + 1) * 8 + 7] = clock64() - t_loop_end;  // epilogue cycles (reduction + stores)
  }
#endif
}

int mmt_wgrad3_launch(const MmtWgradGroup& h, int tiles, hipStream_t s);  // wgrad3.hip

extern "C" int mmt_wgrad_grouped(const MmtWgradGroup* g, void* stream) {
  if (!g || g->count <= 0 || g->count > MMT_WGRAD_MAX || g->rows <= 0) return MMT_ERR_ARG;
  MmtWgradGroup h = *g;
  int tiles = 0;
  // r04: 256 x 256 tiles (wgrad3.hip) when every item is cut into such tiles without remainder, nothing is split over the
  // rows, and the launch has at least 3/4 of a tile per CU over thousands of rows (configs[4]: d = 1024, 256 tiles).
  constexpr int kWgrad3MinRows = 2048, kWgrad3MinTiles = 192;
  {
    int t3 = 0;
    bool ok = h.rows >= kWgrad3MinRows;
    for (int q = 0; q < h.count && ok; ++q) {
      const MmtWgradItem& it = h.item[q];
      ok = it.A && it.B && it.out && it.N > 0 && it.K2 > 0 && it.N % 256 == 0 && it.K2 % 256 == 0 && it.splits <= 1 &&
           !(it.lda % 8) && !(it.ldb % 8) && !((uintptr_t)it.A & 15) && !((uintptr_t)it.B & 15) && !((uintptr_t)it.out & 15) &&
           it.lda >= 256 && it.ldb >= 256;
      t3 += (it.N / 256) * (it.K2 / 256);
    }
    if (ok && t3 >= kWgrad3MinTiles) {
      int tb = 0;
      for (int q = 0; q < h.count; ++q) {
        MmtWgradItem& it = h.item[q];
        if (it.N_out <= 0 || it.N_out > it.N) it.N_out = it.N;
        if (it.K2_out <= 0 || it.K2_out > it.K2) it.K2_out = it.K2;
        if (it.ldo <= 0) it.ldo = it.K2_out;
        it.tile_begin = tb;
        tb += (it.N / 256) * (it.K2 / 256);
      }
      return mmt_wgrad3_launch(h, tb, (hipStream_t)stream);
    }
  }
  // Blocks of different lengths in one launch (an item split over its rows, or contracting over its own row count): the
  // items are launched longest blocks first (a stable sort of the group's copy -- items are independent of each other), a
  // pure function of the group's shape.  The length of a block = 64-row units per split, from the rows the host knows of.
  bool listed = false;
  {
    int len[MMT_WGRAD_MAX];
    for (int q = 0; q < h.count; ++q) {
      const MmtWgradItem& it = h.item[q];
      const int rows_q = it.reserved > 0 ? it.reserved : h.rows, sp = it.splits > 1 ? it.splits : 1;
      len[q] = ((rows_q + 63) / 64 + sp - 1) / sp;
      listed = listed || len[q] != len[0];
    }
    if (listed)
      for (int q = 1; q < h.count; ++q)  // insertion sort, descending, stable
        for (int r = q; r > 0 && len[r] > len[r - 1]; --r) {
          const MmtWgradItem ti = h.item[r]; h.item[r] = h.item[r - 1]; h.item[r - 1] = ti;
          const int tl = len[r]; len[r] = len[r - 1]; len[r - 1] = tl;
        }
  }
  for (int q = 0; q < h.count; ++q) {
    MmtWgradItem& it = h.item[q];
    if (!it.A || !it.B || !it.out || it.N <= 0 || it.K2 <= 0 || it.N % 128 || it.K2 % 128) return MMT_ERR_ARG;
    if ((it.lda % 8) || (it.ldb % 8) || ((uintptr_t)it.A & 15) || ((uintptr_t)it.B & 15) || ((uintptr_t)it.out & 15))
      return MMT_ERR_ALIGN;
    if (it.N_out <= 0 || it.N_out > it.N) it.N_out = it.N;
    if (it.K2_out <= 0 || it.K2_out > it.K2) it.K2_out = it.K2;
    if (it.ldo <= 0) it.ldo = it.K2_out;
    if (it.splits > 1 && (!it.slab || (it.bias_out && !it.bias_slab))) return MMT_ERR_ARG;
    it.tile_begin = tiles;
    tiles += (it.N / 128) * (it.K2 / 128) * (it.splits > 1 ? it.splits : 1);
    // patch shape: PN = largest divisor of the tile rows <= 8, PK = largest divisor of the tile columns <= 32 / PN
    {
      const int tn_all = it.N / 128, tk_all = it.K2 / 128;
      int pn = 1, pk = 1;
      for (int c = 1; c <= 8; ++c)
        if (tn_all % c == 0) pn = c;
      for (int c = 1; c <= 32 / pn; ++c)
        if (tk_all % c == 0) pk = c;
      it.reserved2 = (pn << 16) | pk | (listed ? WGRAD_LISTED : 0);
    }
  }
  constexpr int lds = 36 * 256 * 16;  // a 128 KiB ring of 4 units x (A + B) 64x128 bf16; 144 KiB for the final exchange
  static bool configured = false;
  if (!configured) {
    hipError_t rc = hipFuncSetAttribute((const void*)wgrad_phased_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (rc != hipSuccess) return (int)rc;
    configured = true;
  }
  hipLaunchKernelGGL(wgrad_phased_kernel, dim3(tiles), dim3(512), lds, (hipStream_t)stream, h);
  return (int)hipGetLastError();
}

__global__ void reduce_slabs_kernel(const float* __restrict__ ws, int splits, int64_t count4,
                                    float* __restrict__ out, int accumulate) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < count4;
       i += (int64_t)gridDim.x * blockDim.x) {
    f32x4 s = ((const f32x4*)ws)[i];
    for (int k = 1; k < splits; ++k) s += ((const f32x4*)ws)[k * count4 + i];
    if (accumulate) s += ((const f32x4*)out)[i];
    ((f32x4*)out)[i] = s;
  }
}

// ------------------------------------------------------------------------------------------------
template <int BM, int BN, int EPI>
static int launch_nt(const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc,
                     int M, int N, int K, const MmtEpilogue& e, const int32_t* nr, hipStream_t s) {
  const int grid = ((M + BM - 1) / BM) * (N / BN);
  hipLaunchKernelGGL((gemm_nt_kernel<BM, BN, EPI>), dim3(grid), dim3(256), 0, s, (const bf16_t*)A, lda,
                     (const bf16_t*)B, ldb, C, ldc, M, N, K, e, nr);
  return (int)hipGetLastError();
}

int mmt_gemm2_dispatch(int tile, int epilogue, const void* A, int64_t lda, const void* B, int64_t ldb, void* C,
                       int64_t ldc, int M, int N, int K, const MmtEpilogue& e, const int32_t* nr, hipStream_t s);

// ---- tile policy ---------------------------------------------------------------------------------------------------
// Which kernel runs a GEMM is a pure function of its shape, its epilogue and the number of LIVE rows (token packing: the
// tiles past the live row count exit, so the launch's real size is the live one): no environment variable and no build
// flag enters it.  The live count is on the device; the host's figure is MmtEpilogue.live_rows_hint -- what the collator
// counted before the upload (MmtBertBatch.live_rows_hint) -- and WITHOUT a hint a packed batch is priced at its allocated
// rows (every tile live); no default of this file is tied to a dataset's fill.  mmt_gemm_select_tile exposes the policy to
// tests (tests/test_host_cpu.py asserts the tile of every shipped (shape, live rows) class).

// rows of the problem that hold live tokens, as far as the host knows
static int live_rows_of(int M, bool packed, int hint) {
  if (!packed) return M;
  return hint > 0 && hint < M ? hint : M;
}

// -> tile id: 13 / 14 / 18 (gemm2.hip), 21 (gemm3.hip), 24 / 25 (gemm5.hip), or 1 / 2 = this file's 4-wave 128x128 / 128x64
// kernel.  Measured on MI355X (tools/gemm_lab.py, tools/gemm_instr.py, profiles/r01_gemm_lab.txt):
//   * wide outputs (N >= 1024: QKV, FFN up-projection, dGELU) run best on gemm2's 128x128 tile with 8 waves (wave tile 64x32)
//     at 2 blocks/CU -- from 1024 live tiles on (>= 4 per CU) on the persistent wave-specialised kernel (tile 24: its first
//     K-loop and last epilogue are not overlapped with anything: headline, 696 live tiles: 1.2934 vs 1.2816 ms with it; dense
//     rows, 1320+ tiles: 1.8355 vs 1.8680 ms);
//   * packed N < 1024 GEMMs: the phased 128x64 tile (18; a 96 KiB ring = ONE block per CU) while the live tiles fit one round
//     of 256 CUs, else the 8-wave staggered tile at two blocks per CU (13; tools/splitk_lab.py: 38 vs 49 us at 440 tiles);
//   * long-K narrow GEMMs (FFN down-projection, FFN-up input gradient) on gemm5's 128x128 tiles once those fill a round of
//     the chip (tile 24, >= 200 live tiles: 30 vs 56 us per launch, unpacked step 1.840 -> 1.764 ms);
//   * the 256x256 eight-phase kernel (21) from ~one round of such tiles with K >= 1024 (220 of 256 CUs), or 160 with K >= 3072
//     (at K = 512 prologue and epilogue eat the gain: configs[3] 3.00 -> 3.26 ms with it);
//   * short batches (M <= 1024: the text tower's ~560..960 token rows) and few-row problems: the 128x64 8-wave tile (13);
//   * the dense N = 512 GEMMs stay on this file's 128x64 4-wave tile (both saturate the CU's LDS ingest).
constexpr int kRoundBlocks = 256;       // one block per CU: what "one round" of the chip holds
constexpr int kBigTiles = 220;          // 256x256 tiles from which tile 21 fills the chip, K >= kBigK ...
constexpr int kBigK = 1024;
constexpr int kBigTilesLongK = 160;     // ... or this many with K >= kBigLongK
constexpr int kBigLongK = 3072;
constexpr int kNarrowLongK = 1536;      // "long K" of the narrow GEMMs (tile 24 ...
constexpr int kNarrowLongKTiles = 200;  // ... from this many live 128x128 tiles)
constexpr int kWideLiveTiles = 1024;    // live 128x128 tiles (>= 4 per CU) from which the wide K = hidden GEMMs take tile 24
static int select_tile(int EPI, int M, int N, int K, bool packed, int live_hint, bool colsum, bool dot_out, int reserved) {
  if ((reserved & 0xff) >= 3) return reserved & 0xff;  // forced (tests / tuning)
  const bool dgelu_sums = EPI == MMT_EPI_DGELU && colsum;
  const int live = live_rows_of(M, packed, live_hint);
  const long rt128 = (live + 127) / 128;  // live row tiles of 128
  if (reserved == 0 && N % 256 == 0 && M > 1024) {
    const long t21 = (long)((live + 255) / 256) * (N / 256);
    if ((t21 >= kBigTiles && K >= kBigK) || (t21 >= kBigTilesLongK && K >= kBigLongK)) return 21;
  }
  if (reserved == 0 && M > 1024 && !dgelu_sums) {
    const long t128 = rt128 * (N / 128);
    const bool plain_epi = EPI != MMT_EPI_BIAS_GELU && EPI != MMT_EPI_DGELU && !dot_out;
    if (N < 1024 && N % 128 == 0 && K >= kNarrowLongK && plain_epi && t128 >= kNarrowLongKTiles) return 24;
    if (N < 1024 && packed && rt128 * (N / 64) <= kRoundBlocks) return 18;
    if (N >= 1024 && N % 128 == 0 && K >= 128 && K <= 1024 && t128 >= kWideLiveTiles) return 24;
  }
  if (reserved == 0 && M <= 1024 && !dgelu_sums) return 13;
  if (reserved == 0 && M >= 512) {
    if (N >= 1024 && N % 128 == 0 && !dgelu_sums) return 14;
    if (packed && N % 64 == 0) return 13;
  }
  if (reserved == 0 && M < 512 && N >= 1024 && !dgelu_sums) return 13;  // few rows (the compact last layer): shortest block latency
  if (EPI == MMT_EPI_BF16 && dot_out) return 13;  // the row-dot sums live in gemm2's LDS-staged epilogue only
  return (N % 128 == 0 && reserved == 1) ? 1 : 2;
}

extern "C" int mmt_gemm_select_tile(int epilogue, int M, int N, int K, int packed, int live_rows_hint, int has_colsum,
                                    int has_dot_out, int reserved) {
  if (M <= 0 || N <= 0 || K <= 0 || epilogue < 0 || epilogue > MMT_EPI_BIAS_F32) return MMT_ERR_ARG;
  return select_tile(epilogue, M, N, K, packed != 0, live_rows_hint, has_colsum != 0, has_dot_out != 0, reserved);
}

template <int EPI>
static int dispatch_tile(const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc,
                         int M, int N, int K, const MmtEpilogue& e, const int32_t* nr, hipStream_t s) {
  const int t = select_tile(EPI, M, N, K, nr != nullptr, e.live_rows_hint, e.colsum != nullptr, e.dot_out != nullptr, e.reserved);
  if (t >= 3) return mmt_gemm2_dispatch(t, EPI, A, lda, B, ldb, C, ldc, M, N, K, e, nr, s);
  if (t == 1) return launch_nt<128, 128, EPI>(A, lda, B, ldb, C, ldc, M, N, K, e, nr, s);
  return launch_nt<128, 64, EPI>(A, lda, B, ldb, C, ldc, M, N, K, e, nr, s);
}

extern "C" int mmt_gemm_nt_bf16(const void* A, int64_t lda, const void* B, int64_t ldb, void* C,
                                int64_t ldc, int M, int N, int K, int epilogue, const MmtEpilogue* epi,
                                const int32_t* n_rows_dev, void* stream) {
  if (!A || !B || !C || M <= 0 || N <= 0 || K <= 0) return MMT_ERR_ARG;
  if (K % BK || N % 64) return MMT_ERR_ARG;
  if ((lda % 8) || (ldb % 8) || (ldc % 4) || ((uintptr_t)A & 15) || ((uintptr_t)B & 15) || ((uintptr_t)C & 15))
    return MMT_ERR_ALIGN;
  MmtEpilogue e = {};
  if (epi) e = *epi;
  hipStream_t s = (hipStream_t)stream;
  switch (epilogue) {
    case MMT_EPI_BF16:
      if (e.dot_out && !e.dot_src) return MMT_ERR_ARG;
      return dispatch_tile<MMT_EPI_BF16>(A, lda, B, ldb, C, ldc, M, N, K, e, n_rows_dev, s);
    case MMT_EPI_BIAS_BF16:
      if (!e.bias) return MMT_ERR_ARG;
      return dispatch_tile<MMT_EPI_BIAS_BF16>(A, lda, B, ldb, C, ldc, M, N, K, e, n_rows_dev, s);
    case MMT_EPI_BIAS_GELU:
      if (!e.bias || !e.out2) return MMT_ERR_ARG;
      return dispatch_tile<MMT_EPI_BIAS_GELU>(A, lda, B, ldb, C, ldc, M, N, K, e, n_rows_dev, s);
    case MMT_EPI_BIAS_DROP_RES:
      if (!e.bias || !e.res) return MMT_ERR_ARG;
      return dispatch_tile<MMT_EPI_BIAS_DROP_RES>(A, lda, B, ldb, C, ldc, M, N, K, e, n_rows_dev, s);
    case MMT_EPI_DGELU:
      if (!e.aux) return MMT_ERR_ARG;
      return dispatch_tile<MMT_EPI_DGELU>(A, lda, B, ldb, C, ldc, M, N, K, e, n_rows_dev, s);
    case MMT_EPI_ADD_F32:
      if (!e.res) return MMT_ERR_ARG;
      return dispatch_tile<MMT_EPI_ADD_F32>(A, lda, B, ldb, C, ldc, M, N, K, e, n_rows_dev, s);
    case MMT_EPI_F32: return dispatch_tile<MMT_EPI_F32>(A, lda, B, ldb, C, ldc, M, N, K, e, n_rows_dev, s);
    case MMT_EPI_BIAS_F32:
      if (!e.bias) return MMT_ERR_ARG;
      return dispatch_tile<MMT_EPI_BIAS_F32>(A, lda, B, ldb, C, ldc, M, N, K, e, n_rows_dev, s);
  }
  return MMT_ERR_ARG;
}

extern "C" int mmt_gemm_tn_bf16(const void* A, int64_t lda, const void* B, int64_t ldb, float* ws,
                                int rows, int N, int K2, int splits, const int32_t* n_rows_dev,
                                void* stream) {
  if (!A || !B || !ws || rows <= 0 || N <= 0 || K2 <= 0 || splits <= 0) return MMT_ERR_ARG;
  if (N % 128 || K2 % 128) return MMT_ERR_ARG;
  if ((lda % 8) || (ldb % 8) || ((uintptr_t)A & 15) || ((uintptr_t)B & 15) || ((uintptr_t)ws & 15))
    return MMT_ERR_ALIGN;
  const int grid = (N / 128) * (K2 / 128) * splits;
  hipLaunchKernelGGL(gemm_tn_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)A, lda,
                     (const bf16_t*)B, ldb, ws, rows, N, K2, splits, n_rows_dev);
  return (int)hipGetLastError();
}

// two slab sets (a weight gradient and its bias gradient) in one launch
__global__ void reduce_slabs_pair_kernel(const float* __restrict__ wa, int64_t ca4, float* __restrict__ oa,
                                         const float* __restrict__ wb, int64_t cb4, float* __restrict__ ob, int splits) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < ca4 + cb4; i += (int64_t)gridDim.x * blockDim.x) {
    const bool first = i < ca4;
    const f32x4* ws = (const f32x4*)(first ? wa : wb);
    const int64_t j = first ? i : i - ca4, c4 = first ? ca4 : cb4;
    f32x4 s = ws[j];
    for (int k = 1; k < splits; ++k) s += ws[k * c4 + j];
    ((f32x4*)(first ? oa : ob))[j] = s;
  }
}

extern "C" int mmt_reduce_slabs_pair(const float* ws_a, int64_t count_a, float* out_a, const float* ws_b, int64_t count_b,
                                     float* out_b, int splits, void* stream) {
  if (!ws_a || !out_a || !ws_b || !out_b || splits <= 0 || count_a <= 0 || count_b <= 0 || ((count_a | count_b) & 3))
    return MMT_ERR_ARG;
  const int64_t c4 = (count_a + count_b) / 4;
  const int grid = (int)((c4 + 255) / 256 < 2048 ? (c4 + 255) / 256 : 2048);
  hipLaunchKernelGGL(reduce_slabs_pair_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, ws_a, count_a / 4, out_a, ws_b,
                     count_b / 4, out_b, splits);
  return (int)hipGetLastError();
}

extern "C" int mmt_reduce_slabs(const float* ws, int splits, int64_t count, float* out, int accumulate,
                                void* stream) {
  if (!ws || !out || splits <= 0 || count <= 0 || (count & 3)) return MMT_ERR_ARG;
  const int64_t c4 = count / 4;
  const int grid = (int)((c4 + 255) / 256 < 2048 ? (c4 + 255) / 256 : 2048);
  hipLaunchKernelGGL(reduce_slabs_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, ws, splits, c4,
                     out, accumulate);
  return (int)hipGetLastError();
}
