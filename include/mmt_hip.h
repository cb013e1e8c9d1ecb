/* mmt_hip.h -- C ABI of libmmt_hip.so: the MI355X (gfx950) hot path of MMT.
 *
 * The reference (gabeur/mmt) is pure Python on ATen; it has no FFI layer.  The boundary a
 * maintainer binds is therefore the set of ATen op chains on the hot path;
 * each entry point below names the reference code it replaces (paths relative to the reference
 * root).  Python binds these through ctypes (mmt_amd/_lib.py); INTEGRATION.md shows the stub.
 *
 * Conventions (last row):
 *   - every pointer is a DEVICE pointer owned by the caller (torch-allocated); no ownership moves;
 *   - calls are asynchronous on `stream` (a hipStream_t passed as void*); no hipMalloc, no device
 *     sync, no global mutable state => safe under hipGraph capture;
 *   - return 0 on success, negative MMT_ERR_* on bad arguments, positive hipError_t on launch error;
 *   - bf16 tensors are raw uint16 bit patterns; "ld*" are leading dimensions in ELEMENTS;
 *   - activations are token-major [rows, channels]; row buffers are allocated with the row count
 *     rounded up to MMT_ROW_ALIGN so that GEMM tiles never need row bounds checks;
 *   - `n_rows_dev` (nullable) points at the live row count on the device (variable-length packing
 *     of valid tokens): tiles at or beyond it exit early, reductions over rows stop there;
 *   - dropout is a counter-based RNG keyed by (key, original element index): the backward pass
 *     regenerates masks from the same (key, threshold) instead of storing them.
 */
#ifndef MMT_HIP_H_
#define MMT_HIP_H_
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MMT_ABI_VERSION 6  /* 6: the 54 per-variant scan entries became nine over MmtSearchScan; 5: mmt_gemm_nt_ln_fwd removed (4: MmtEpilogue.rider*, MmtBertBatch.rider*, MmtAdamQueue and the Adam rider exports removed; r06: live_rows_hint; r04: MmtEpilogue.dot_*, mmt_attn_bwd*_ex) */
#define MMT_ROW_ALIGN 256

#define MMT_ERR_ARG (-1)    /* unsupported shape / null pointer */
#define MMT_ERR_ALIGN (-2)  /* pointer or leading dimension not 16-byte aligned */

int mmt_abi_version(void);
const char* mmt_build_info(void);

/* ---- GEMM epilogues ------------------------------------------------------------------------ */
enum {
  MMT_EPI_BF16 = 0,          /* out(bf16) = acc                                                 */
  MMT_EPI_BIAS_BF16 = 1,     /* out(bf16) = acc + bias[n]              bert.py:137-139 Q/K/V     */
  MMT_EPI_BIAS_GELU = 2,     /* out(bf16) = acc + bias; out2(bf16) = gelu_erf(out)  bert.py:217-220 */
  MMT_EPI_BIAS_DROP_RES = 3, /* out(f32) = dropout(acc + bias) + res   bert.py:186-188,234-236 (pre-LN sum) */
  MMT_EPI_DGELU = 4,         /* out(bf16) = acc * gelu_erf'(aux)       backward of bert.py:37-53 */
  MMT_EPI_ADD_F32 = 5,       /* out(f32) = acc + res                   dgrad + residual gradient */
  MMT_EPI_F32 = 6,           /* out(f32) = acc                                                   */
  MMT_EPI_BIAS_F32 = 7       /* out(f32) = acc + bias[n]               model.py:724 ReduceDim.fc */
};

typedef struct MmtEpilogue {
  const float* bias;        /* [N] fp32                                                         */
  const float* res;         /* [M, ldres] fp32 residual / addend                                */
  int64_t ldres;
  void* out2;               /* second bf16 output [M, ldout2] (MMT_EPI_BIAS_GELU)               */
  int64_t ldout2;
  const void* aux;          /* bf16 [M, ldaux] pre-activation (MMT_EPI_DGELU)                   */
  int64_t ldaux;
  float* colsum;            /* nullable: [ceil(M/128), N] per-row-tile column sums of `out`     */
  const int32_t* row_index; /* nullable: row -> original token index (b*S+s) for the RNG        */
  const uint32_t* seed_dev; /* nullable: per-step seed in device memory, hashed into drop_key   */
  uint32_t drop_key;        /* dropout stream key (seed, site, layer mixed by the host)         */
  uint32_t drop_thr16;      /* keep iff u16 >= thr16; 0 disables dropout                        */
  float drop_scale;         /* 1 / (1 - thr16/65536)                                            */
  int32_t reserved;         /* 0 = auto tile; forced tile id (tests/tuning): 1 / 2 = the 4-wave 128x128 / 128x64 kernel
                             * of gemm.hip, 13 / 14 / 18 = gemm2.hip, 21 = gemm3.hip, 24 / 25 = gemm5.hip; any other
                             * id >= 3 is MMT_ERR_ARG                                                    */
  /* MMT_EPI_BF16 only, nullable: dot_out[row, n / 64] = sum over the 64 output columns of group n / 64 of
   * out(bf16)[row, n] * dot_src(bf16)[row, n] -- with out = dO = dA . Wo and dot_src = O (the attention context) these are
   * the "delta" sums of the attention backward (rowsum(dO * O) per head = DH / 64 groups), formed while dO is still in
   * registers instead of by re-reading dO and O (model/bert.py:141-168 backward).  dot_out: fp32 [M, N / 64], rows at or past M or
   * *n_rows_dev are not written.  Every tile forms them but the forced tile 25 (MMT_ERR_ARG); forced
   * tiles 1 / 2 run as tile 13. */
  const void* dot_src;
  int64_t lddot;
  float* dot_out;
  /* r06: with n_rows_dev set, the live row count as the HOST knows it (0 = unknown: the tile choice then prices the problem
   * at all M rows).  Only mmt_gemm_select_tile reads it; the kernels read n_rows_dev. */
  int32_t live_rows_hint;
} MmtEpilogue;

/* C[M,N] = A[M,K] . B[N,K]^T  (both operands K-contiguous bf16, fp32 accumulate on MFMA).
 * Replaces every nn.Linear forward on the path (bert.py:137-139,186,218,234; model.py:724) and,
 * with B = W^T copies, the input-gradient GEMMs of their backward.
 * Requirements: K % 64 == 0, N % 64 == 0, rows allocated to a multiple of 128. */
int mmt_gemm_nt_bf16(const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc,
                     int M, int N, int K, int epilogue, const MmtEpilogue* epi,
                     const int32_t* n_rows_dev, void* stream);

/* The tile mmt_gemm_nt_bf16 runs a problem on (13 / 14 / 18: gemm2.hip, 21: gemm3.hip, 24 / 25: gemm5.hip, 1 / 2: the 4-wave
 * 128x128 / 128x64 kernel of gemm.hip): a pure function of the shape, the epilogue and the live row count the host knows
 * (packed != 0: n_rows_dev given; live_rows_hint as MmtEpilogue.live_rows_hint; has_colsum / has_dot_out: the epilogue's
 * optional outputs; reserved as MmtEpilogue.reserved).  Host-only, no GPU needed (tests/test_host_cpu.py pins the policy). */
int mmt_gemm_select_tile(int epilogue, int M, int N, int K, int packed, int live_rows_hint, int has_colsum, int has_dot_out,
                         int reserved);

/* Split-K form for skinny problems (M up to a few hundred rows, long K): K-slices run as independent blocks writing fp32
 * partial slabs into `ws`, a second kernel sums them in a fixed order and applies the epilogue
 * (MMT_EPI_BF16 / F32 / BIAS_F32 / ADD_F32 / BIAS_DROP_RES).  Same results as mmt_gemm_nt_bf16 up to fp32 summation order. */
int64_t mmt_gemm_nt_splitk_workspace_floats(int M, int N, int K);
int mmt_gemm_nt_splitk(const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc, int M, int N, int K,
                       int epilogue, const MmtEpilogue* epi, float* ws, void* stream);
/* The same with explicit control: splits (<= 0: up to 16), wide != 0: 128x128 tiles (N % 128 == 0), n_rows_dev (nullable):
 * device count of live rows, no_epilogue != 0: only the partial slabs are produced (slab s at ws + s*round_up(M,128)*N,
 * leading dimension N) for a consumer that sums them itself. */
int mmt_gemm_nt_splitk_ex(const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc, int M, int N, int K,
                          int epilogue, const MmtEpilogue* epi, float* ws, int splits, int wide, const int32_t* n_rows_dev,
                          int no_epilogue, void* stream);
/* NN operand form: C[M,N] = A[M,K] . B[K,N] with B row-major [K, N] -- a weight W[out, in] as stored, used for the
 * input gradient dX = dY . W (autograd of every nn.Linear of model/bert.py:146-150,186,218,234) without a transposed
 * copy: the tile is staged as it lies and the MFMA fragments come from ds_read_b64_tr_b16.  Epilogues: MMT_EPI_BF16,
 * MMT_EPI_F32, MMT_EPI_ADD_F32, MMT_EPI_DGELU (no colsum).  Same alignment rules as mmt_gemm_nt_bf16; N % 64 == 0. */
int mmt_gemm_nn_bf16(const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc, int M, int N, int K,
                     int epilogue, const MmtEpilogue* epi, const int32_t* n_rows_dev, void* stream);
int mmt_gemm_nn_splitk_ex(const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc, int M, int N, int K,
                          int epilogue, const MmtEpilogue* epi, float* ws, int splits, int wide, const int32_t* n_rows_dev,
                          int no_epilogue, void* stream);

/* Several independent C_i[M_i,N_i] = A_i . B_i^T (+ bias_i) in ONE launch (epilogue MMT_EPI_BIAS_F32 / MMT_EPI_F32):
 * the per-expert ReduceDim.fc projections of model/model.py:426-437 (seven GEMMs with different K). */
#define MMT_GEMM_GROUP_MAX 16
typedef struct MmtGemmItem {
  const void* A; const void* B; void* C; const float* bias; /* bf16 [M,lda], bf16 [N,ldb], fp32 [M,ldc], fp32 [N] */
  int64_t lda, ldb, ldc;
  int32_t M, N, K, tile_begin;
  const int32_t* n_rows_dev; /* nullable: live rows of this problem on the device (<= M); tiles past them exit */
} MmtGemmItem;
int mmt_gemm_nt_grouped(const MmtGemmItem* items, int n, int epilogue, void* stream);

/* dW[N,K2] (+)= sum_rows A[rows,N]^T . B[rows,K2]   (weight gradients: contraction over tokens).
 * A, B are row-major bf16 [rows, *]; the result is written as fp32 `splits` partial slabs
 * ws[splits][N*K2] which mmt_reduce_slabs sums.  Replaces autograd's weight-gradient mm for every
 * nn.Linear on the path.  N % 128 == 0, K2 % 128 == 0. */
int mmt_gemm_tn_bf16(const void* A, int64_t lda, const void* B, int64_t ldb, float* ws,
                     int rows, int N, int K2, int splits, const int32_t* n_rows_dev, void* stream);
int mmt_reduce_slabs(const float* ws, int splits, int64_t count, float* out, int accumulate,
                     void* stream);
/* the same for a weight-gradient slab set and its bias-gradient slab set in ONE launch (out = sum of `splits` slabs) */
int mmt_reduce_slabs_pair(const float* ws_a, int64_t count_a, float* out_a, const float* ws_b, int64_t count_b,
                          float* out_b, int splits, void* stream);

/* Grouped weight gradients: for every item, out[N_out, K2_out] = sum_rows A[rows,N]^T . B[rows,K2] written
 * directly as fp32 (no split-K slabs), and bias_out[n] = sum_rows A[rows, n] (nullable) -- all items in ONE
 * launch, one 128x128 tile per block.  Replaces autograd's weight AND bias gradients of the four nn.Linear of a
 * BertLayer (bert.py:137-139,186,218,234) resp. of all ReduceDim.fc (model.py:724).  N % 128 == 0, K2 % 128 == 0
 * (operands padded); N_out / K2_out / ldo (0 = N / K2 / K2_out) un-pad the stored result. */
#define MMT_WGRAD_MAX 16
typedef struct MmtWgradItem {
  const void* A;   /* bf16 [rows, lda] : dY                                                          */
  const void* B;   /* bf16 [rows, ldb] : X                                                           */
  float* out;      /* fp32 [N_out, ldo]                                                              */
  float* bias_out; /* fp32 [N_out] or NULL                                                           */
  int64_t lda, ldb, ldo;
  int32_t N, K2, N_out, K2_out, tile_begin;
  int32_t reserved; /* > 0: this item contracts over exactly `reserved` rows (overrides rows / n_rows_dev)     */
  float* slab;      /* splits > 1: partial results [splits][N_out, ldo] (summed by the caller, e.g.            */
  float* bias_slab; /*   mmt_col_reduce_multi) and partial bias gradients [splits][N_out]                       */
  int32_t splits, reserved2; /* reserved2: set by mmt_wgrad_grouped (tile patch shape; bit 30: longest-first launch
                              * order, below), callers leave it 0 */
  const int32_t* n_rows_dev; /* nullable: this item contracts over *n_rows_dev rows (device; overrides the group's) */
} MmtWgradItem;
typedef struct MmtWgradGroup {
  MmtWgradItem item[MMT_WGRAD_MAX];
  const int32_t* n_rows_dev; /* nullable live row count on device                                    */
  int32_t count, rows;
} MmtWgradGroup;
/* A group whose blocks differ in length (an item with splits > 1 or reserved > 0 next to others; lengths from `rows` and
 * `reserved`, the row counts the host knows) is launched longest blocks first, item by item.  Results do not depend on it. */
int mmt_wgrad_grouped(const MmtWgradGroup* g, void* stream);

/* out[i] (+)= sum_s ws[s][i] over a [rows, cols_ws] slab keeping only the first cols_out columns
 * (un-pads the K-padded ReduceDim weight gradients). */
int mmt_reduce_slabs_2d(const float* ws, int splits, int rows, int cols_ws, int cols_out, float* out,
                        int accumulate, void* stream);

/* ---- LayerNorm / embeddings (norm.hip) ---------------------------------------------------------
 * h = LN(z) over the last dim, fp32 statistics.  bert.py:188,236 (BertSelfOutput / BertOutput
 * layer_norm; z is the pre-LN sum written by MMT_EPI_BIAS_DROP_RES).  d % 256 == 0, d <= 1024. */
int mmt_ln_fwd(const float* z, const float* gamma, const float* beta, float eps, float* h32, void* h16,
               float* mean, float* rstd, int rows, int d, const int32_t* n_rows_dev, void* stream);
/* h = dropout(LN(features + type_emb[type_ids] + pos_emb[pos_ids]))   bert.py:87-105.
 * z_save receives the pre-LN sum (needed by backward). pos_ids may be NULL (pos_enc='none'). */
int mmt_embed_ln_fwd(const float* features, const int32_t* type_ids, const int32_t* pos_ids,
                     const float* type_emb, const float* pos_emb, float* z_save, const float* gamma,
                     const float* beta, float eps, float* h32, void* h16, float* mean, float* rstd,
                     int rows, int d, const int32_t* n_rows_dev, const int32_t* row_index,
                     uint32_t drop_key, uint32_t thr16, float drop_scale, const uint32_t* seed_dev,
                     void* stream);
/* the same launch carrying one extra block that writes the attention backward's block order of this batch (sched_work
 * nullable = no rider; arguments as for mmt_attn_schedule with tiles = ceil(S / 64)) */
int mmt_embed_ln_fwd_sched(const float* features, const int32_t* type_ids, const int32_t* pos_ids,
                           const float* type_emb, const float* pos_emb, float* z_save, const float* gamma,
                           const float* beta, float eps, float* h32, void* h16, float* mean, float* rstd,
                           int rows, int d, const int32_t* n_rows_dev, const int32_t* row_index,
                           uint32_t drop_key, uint32_t thr16, float drop_scale, const uint32_t* seed_dev,
                           const int32_t* sched_cu, int sched_B, int sched_H, int sched_tiles, int32_t* sched_work,
                           void* stream);
/* Compact-row variant: LN over `rows` compact rows; fp32 row i goes to h32[dst_rows[i]] (h16 compact, nullable). */
int mmt_ln_fwd_scatter(const float* z, const float* gamma, const float* beta, float eps, float* h32,
                       const int32_t* dst_rows, void* h16, float* mean, float* rstd, int rows, int d, void* stream);
/* dst[i] = src[rows[i]] (+ idx_out[i] = idx_in ? idx_in[rows[i]] : rows[i]) / dst[rows[i]] (+)= src[i]; fp32 rows of d
 * (rows must be distinct for the accumulating scatter). */
int mmt_rows_gather(const float* src, const int32_t* rows, int n, int d, float* dst, const int32_t* idx_in,
                    int32_t* idx_out, void* stream);
int mmt_rows_scatter(const float* src, const int32_t* rows, int n, int d, float* dst, int accumulate, void* stream);
/* Embedding-table gradient written directly (dtable[v] = sum of g[r] over token rows r < min(rows, *n_rows_dev) with
 * ids[r] == v, row order; rows of unused ids are zeroed): for large tables with few ids in use (BERT-base's 512-row
 * position table).  The small video-BERT tables use mmt_table_grad_partials + mmt_col_reduce. */
int mmt_table_grad_direct(const float* g, const int32_t* ids, int rows, int d, int vocab, const int32_t* n_rows_dev,
                          float* dtable, void* stream);
/* Word-embedding gradient of the text tower (HF BertEmbeddings.word_embeddings, reached from model/model.py:371-376):
 * dtable[id] = sum of g[i] over token rows i with ids[i] == id, in row order (deterministic); rows with
 * id == padding_idx or outside [0, vocab) contribute nothing; n_rows_dev (nullable) bounds n on the device.  dtable
 * [vocab, d] must be zero on entry.  The forward
 * lookup is mmt_rows_gather(table, ids, ...). */
int mmt_embedding_grad(const float* g, const int32_t* ids, int n, int d, int vocab, int padding_idx,
                       const int32_t* n_rows_dev, float* dtable, void* stream);
/* Text-side token packing (drops the padded tokens of model/model.py:353-369; valid when only the [CLS] row of the
 * last layer is read, :378-379).  int64 [B, W] inputs (token_type_ids nullable = 0, position_ids nullable = 0..W-1);
 * int32 outputs: counts [B], cu_seqlens [B+1], n_rows_dev [1], ids/types/pos/row_index [>= B*W] (first *n_rows_dev
 * entries written; row_index = dense coordinate b*W + t), cls_rows [B] = first kept row of each sample. */
int mmt_text_plan(const int64_t* input_ids, const int64_t* token_type_ids, const int64_t* position_ids,
                  const int64_t* attention_mask, int B, int W, int32_t* counts, int32_t* cu_seqlens, int32_t* n_rows_dev,
                  int32_t* ids, int32_t* types, int32_t* pos, int32_t* row_index, int32_t* cls_rows, void* stream);
/* The reduction of split-K partial slabs (mmt_gemm_nt_splitk_ex with no_epilogue = 1; geometry from
 * mmt_gemm_splitk_geometry) folded into the LayerNorm pass next to it -- the compact last encoder layer, where a launch
 * costs more than the work it carries:
 *   mmt_splitk_ln_fwd : z = sum_s slab_s + bias -> dropout -> + residual (res[res_rows ? res_rows[i] : i]); h = LN(z)
 *                       (bert.py:185-189 / 233-237).  RNG row coordinate: rowidx[i] if given, else
 *                       row_index[res_rows[i]] (written to rowidx_out for the kernels that follow).
 *   mmt_ln_bwd_slabs  : mmt_ln_bwd with dout = sum_s slab_s + res. */
int mmt_gemm_splitk_geometry(int M, int N, int K, int splits_requested, int* splits, int64_t* slab_stride);
int mmt_splitk_ln_fwd(const float* slabs, int splits, int64_t slab_stride, const float* bias, const float* res,
                      const int32_t* res_rows, const int32_t* rowidx, const int32_t* row_index, int32_t* rowidx_out,
                      uint32_t drop_key, uint32_t thr16, float drop_scale, const uint32_t* seed_dev, float* z_out,
                      const float* gamma, const float* beta, float eps, float* h32, void* h16, float* mean, float* rstd,
                      int rows, int d, void* stream);
int mmt_ln_bwd_slabs(const float* slabs, int splits, int64_t slab_stride, const float* res, const float* z,
                     const float* mean, const float* rstd, const float* gamma, float* dz, void* dy, float* partials,
                     int rows, int d, int drop_mode, const int32_t* row_index, uint32_t drop_key, uint32_t thr16,
                     float drop_scale, const uint32_t* seed_dev, void* stream);
/* the same on a packed batch: n_rows_dev (nullable) = device count of live rows, rows = the capacity launched for */
int mmt_splitk_ln_fwd_ex(const float* slabs, int splits, int64_t slab_stride, const float* bias, const float* res,
                         const int32_t* res_rows, const int32_t* rowidx, const int32_t* row_index, int32_t* rowidx_out,
                         uint32_t drop_key, uint32_t thr16, float drop_scale, const uint32_t* seed_dev, float* z_out,
                         const float* gamma, const float* beta, float eps, float* h32, void* h16, float* mean, float* rstd,
                         int rows, int d, const int32_t* n_rows_dev, void* stream);
int mmt_ln_bwd_slabs_ex(const float* slabs, int splits, int64_t slab_stride, const float* res, const float* z,
                        const float* mean, const float* rstd, const float* gamma, float* dz, void* dy, float* partials,
                        int rows, int d, int drop_mode, const int32_t* n_rows_dev, const int32_t* row_index,
                        uint32_t drop_key, uint32_t thr16, float drop_scale, const uint32_t* seed_dev, void* stream);

/* LayerNorm backward.  drop_mode 0: none; 1: the LN input was dropout(y)+res -> dy(bf16) = mask*dz*scale;
 * 2: dropout followed the LN (embeddings) -> dout is masked first.  `partials` receives
 * [ceil(rows/rpb)][3][d] per-block column sums (dgamma, dbeta, dbias) for mmt_col_reduce. */
int mmt_ln_bwd_rows_per_block(int rows);
int mmt_ln_bwd(const float* dout, const float* z, const float* mean, const float* rstd, const float* gamma,
               float* dz, void* dy, float* partials, int rows, int d, int drop_mode,
               const int32_t* n_rows_dev, const int32_t* row_index, uint32_t drop_key, uint32_t thr16,
               float drop_scale, const uint32_t* seed_dev, void* stream);
/* out_j[c] (+)= sum_b partials[b][j][c], j < nvec <= 4 (NULL outputs are skipped); fixed order. */
int mmt_col_reduce(const float* partials, int nblocks, int nvec, int d, float* out0, float* out1,
                   float* out2, float* out3, int accumulate, void* stream);
/* Batched form: every job j writes out[k][c] = sum_b partials[b][k][c] (k < nout <= nvec) in ONE launch. */
#define MMT_COLRED_MAX 32
typedef struct MmtColReduceJob {
  const float* partials; /* [nblocks][nvec][d]                                                      */
  float* out[4];         /* nout outputs of d floats each (NULL entries are skipped)                */
  int32_t nblocks, nvec, nout, d;
} MmtColReduceJob;
int mmt_col_reduce_multi(const MmtColReduceJob* jobs, int n, void* stream);
/* dtable[v] (+)= sum of g[row] over rows with ids[row] == v: gradient of nn.Embedding (bert.py:78-81)
 * as a deterministic segmented sum (no atomics); scratch = mmt_table_grad_scratch_floats() floats. */
int64_t mmt_table_grad_scratch_floats(int vocab, int d);
int mmt_table_grad(const float* g, const int32_t* ids, int rows, int d, int vocab,
                   const int32_t* n_rows_dev, float* scratch, float* dtable, int accumulate, void* stream);
/* The two halves of mmt_table_grad: chunk partials [mmt_table_grad_chunks()][vocab*d] into `scratch`, to be summed
 * by mmt_col_reduce / mmt_col_reduce_multi (nvec = 1, d = vocab*d). */
int mmt_table_grad_partials(const float* g, const int32_t* ids, int rows, int d, int vocab,
                            const int32_t* n_rows_dev, float* scratch, void* stream);
/* both tables of the video BERT (ids1 nullable) as one-hot x gradient products on the exact-fp32 matrix cores, one launch;
 * same scratch layout as mmt_table_grad_partials ([chunks][vocab][d]); d % 128 == 0, vocabularies of at most 128 rows */
int mmt_table_grad_partials_pair(const float* g, const int32_t* ids0, int vocab0, float* scratch0, const int32_t* ids1,
                                 int vocab1, float* scratch1, int rows, int d, const int32_t* n_rows_dev, void* stream);
int mmt_table_grad_chunks(void);
/* partials[blk][c] = column sums of a bf16 matrix over 32-row blocks (bias gradients). */
int mmt_colsum_bf16(const void* x, int64_t ld, int rows, int cols, const int32_t* n_rows_dev,
                    float* partials, void* stream);

/* ---- fused attention (attention.hip), head dim 128 ----------------------------------------------
 * Replaces bert.py:141-168: softmax(QK^T/sqrt(dh) + mask_bias[key]) -> dropout -> .V, merged heads.
 * qkv bf16 [rows, 3d]; sample b owns rows cu_seqlens[b]..cu_seqlens[b+1] (NULL => b*S..(b+1)*S);
 * mask_bias fp32 [rows] is the additive key mask (0 / -10000, bert.py:395); lse fp32 [rows, H]. */
int mmt_attn_fwd(const void* qkv, const int32_t* cu_seqlens, const float* mask_bias, void* ctx, float* lse,
                 int B, int S, int H, int d, float scale, uint32_t drop_key, uint32_t thr16,
                 float drop_scale, const uint32_t* seed_dev,
                 const int32_t* row_index, void* stream);
/* Backward of the above (autograd of bert.py:141-168): dqkv bf16 [rows, 3d].
 * delta fp32 [rows, d/64]: sums of dctx * ctx over the 64-column groups of a row (delta of head h = its DH/64 groups).
 * mmt_attn_bwd forms them itself (scratch, one extra launch); mmt_attn_bwd_ex(delta_ready = 1) takes them as INPUT --
 * the epilogue of the GEMM that produced dctx writes them (MmtEpilogue.dot_src / dot_out). */
/* work (nullable, packed batches with (B * H) % 8 == 0): the block order of THIS batch, mmt_attn_schedule_words(B, S, H) int32
 * words written by mmt_attn_schedule (or by the engine, riding in its embedding LayerNorm launch): longest blocks first,
 * empty slots at the end of the grid, every block of a (sample, head) on one XCD.  Same results as without. */
int mmt_attn_bwd_ex(const void* qkv, const int32_t* cu_seqlens, const float* mask_bias, const void* ctx,
                    const float* lse, const void* dctx, void* dqkv, float* delta, int delta_ready, int B, int S, int H,
                    int d, float scale, uint32_t drop_key, uint32_t thr16, float drop_scale,
                    const uint32_t* seed_dev, const int32_t* row_index, const int32_t* work, void* stream);
int64_t mmt_attn_schedule_words(int B, int S, int H);
int mmt_attn_schedule(const int32_t* cu_seqlens, int B, int S, int H, int32_t* work, void* stream);
int mmt_attn_bwd(const void* qkv, const int32_t* cu_seqlens, const float* mask_bias, const void* ctx,
                 const float* lse, const void* dctx, void* dqkv, float* delta, int B, int S, int H, int d,
                 float scale, uint32_t drop_key, uint32_t thr16, float drop_scale,
                 const uint32_t* seed_dev,
                 const int32_t* row_index, void* stream);
/* Query-subset attention (last encoder layer: only the rows that are read out need a context vector): queries are the
 * rows qsel[b*nq + i] (distinct rows of sample b); ctx / lse / dctx / delta are compact [B*nq, .] (delta: [B*nq, d/64]);
 * qkv / dqkv keep the full layout.  The backward needs nothing of dqkv on entry: it writes dK / dV of every live row, dQ of
 * the selected rows and zero in the Q section of every other live row.  The backward takes nq <= 64 (MMT_ERR_ARG above that:
 * the kernel that clears the Q section is ordered against one dQ block per (sample, head) only); the forward takes any nq. */
int mmt_attn_fwd_rows(const void* qkv, const int32_t* cu_seqlens, const float* mask_bias, const int32_t* qsel, int nq,
                      void* ctx, float* lse, int B, int S, int H, int d, float scale, uint32_t drop_key, uint32_t thr16,
                      float drop_scale, const uint32_t* seed_dev,
                 const int32_t* row_index, void* stream);
int mmt_attn_bwd_rows_ex(const void* qkv, const int32_t* cu_seqlens, const float* mask_bias, const int32_t* qsel, int nq,
                         const void* ctx, const float* lse, const void* dctx, void* dqkv, float* delta, int delta_ready,
                         int B, int S, int H, int d, float scale, uint32_t drop_key, uint32_t thr16, float drop_scale,
                         const uint32_t* seed_dev, const int32_t* row_index, void* stream);
int mmt_attn_bwd_rows(const void* qkv, const int32_t* cu_seqlens, const float* mask_bias, const int32_t* qsel, int nq,
                      const void* ctx, const float* lse, const void* dctx, void* dqkv, float* delta, int B, int S, int H,
                      int d, float scale, uint32_t drop_key, uint32_t thr16, float drop_scale,
                      const uint32_t* seed_dev,
                 const int32_t* row_index, void* stream);
/* (all four) row_index (nullable): token packing -- row_index[row] = b*S + original position of the token; the
 * attention-probability dropout mask is keyed on ORIGINAL (query, key) positions, so packed and dense runs draw the same
 * mask. */
/* Test helper: the keep-mask mmt_attn_fwd draws, uint8 [B,H,S,S] (dense layout). */
int mmt_attn_dropout_mask(uint8_t* out, int B, int H, int S, uint32_t drop_key, uint32_t thr16,
                          const uint32_t* seed_dev, void* stream);

/* ---- parameter packing / optimizer (elementwise.hip) --------------------------------------------- */
#define MMT_PACK_MAX 24
typedef struct MmtPackItem {
  const float* src;  /* fp32 master [rows, cols]                                                   */
  void* dst;         /* bf16 [rows, dst_ld], columns cols..dst_ld zero-filled                      */
  void* dst_t;       /* nullable bf16 transposed copy [dst_t_rows >= cols, dst_t_ld >= rows]       */
  int32_t rows, cols, dst_ld, dst_t_ld, dst_t_rows, reserved;
} MmtPackItem;
/* bf16 shadows of the fp32 master weights (and W^T copies for the input-gradient GEMMs). */
int mmt_pack_weights(const MmtPackItem* items, int n, void* stream);
/* torch.optim.Adam step (train.py:100) over one flat fp32 buffer; step_dev = 1-based step on device.
 * lr_dev (nullable): device float that overrides `lr` -- the learning-rate schedule (StepLR + warm-up,
 * trainer/trainer.py:150-160, train.py:101-103) then works under HIP-graph replay without re-capturing. */
int mmt_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t count,
                  float lr, float beta1, float beta2, float eps, float weight_decay,
                  const int32_t* step_dev, const float* lr_dev, void* stream);

/* The same optimizer step (train.py:100) that ALSO refreshes the bf16 shadows of the GEMM weights (and their W^T
 * copies), so that no re-packing pass over the weights runs between optimizer and the next forward.  The flat buffer is
 * described as segments in ascending order that tile [0, count): dst == NULL: a plain span of `count` elements;
 * otherwise the fp32 matrix [rows, cols] at `offset` (cols % 4 == 0) whose bf16 copy dst [rows, dst_ld] and optional
 * transpose dst_t [cols, dst_t_ld >= rows, % 8 == 0] are rewritten from the updated values.  segs_host / segs_dev: the
 * same table in host memory (grid layout) and device memory (read by the kernel; it must stay valid under graph replay). */
#define MMT_ADAM_SEG_MAX 160
typedef struct MmtAdamSeg {
  int64_t offset, count;
  void* dst;
  void* dst_t;
  int32_t rows, cols, dst_ld, dst_t_ld;
} MmtAdamSeg;
int mmt_adam_fused_blocks(const MmtAdamSeg* seg);
int mmt_adam_step_fused(float* params, const float* grads, float* exp_avg, float* exp_avg_sq,
                        const MmtAdamSeg* segs_host, const MmtAdamSeg* segs_dev, int n_segs, float lr, float beta1,
                        float beta2, float eps, float weight_decay, int32_t* step_dev, const float* lr_dev,
                        int bump_step, void* stream);
/* bump_step = 0: step_dev[0] is this launch's step number t (bias correction), as mmt_adam_step.
 * bump_step = 1: step_dev is int32[2] = {steps taken so far, 0}; the launch is step step_dev[0] + 1 and stores it.
 * bump_step = 2: the launch is step step_dev[0] + 1 as well but leaves the count alone: one optimizer step issued as
 *   several launches over sub-ranges of the segment table (each as soon as its gradients are final), the last with 1. */

/* ---- video tokens (assemble.hip) -------------------------------------------------------------------
 * model.py:426-437 (ReduceDim per expert) + :485-567 (token assembly), see assemble.hip.
 * mmt_video_plan: seed_bump (nullable) = the per-step dropout seed word of the encoder, incremented by the plan kernel
 * (a training forward needs a fresh seed anyway: one launch less than a separate increment). */
#define MMT_MAX_EXPERTS 16
typedef struct MmtExpertIO {
  const float* feat;     /* [B, T, D] fp32  features[mod]                                        */
  const float* maxpool;  /* [B, D] fp32     features_maxpool[mod]                                */
  const float* ind;      /* [B, T] fp32     features_ind[mod]                                    */
  const float* t;        /* [B, T] fp32     features_t[mod]                                      */
  void* x;               /* bf16 [rows_pad, Dpad] GEMM input, COMPACT rows (see MmtVideoSrc)              */
  float* y;              /* fp32 [rows_pad, d] ReduceDim.fc output (pre-normalisation)           */
  void* dy;              /* bf16 [rows_pad, d] gradient wrt y (backward)                         */
  int32_t D, Dpad, type_idx, rows_pad;
  /* K-split of a wide expert's projection (rgb 2048, scene 2208 ...): y holds the first K chunk's product + bias,
   * y_part[i] the other chunks' partial products (same shape as y); the scatter kernels add them up. */
  const float* y_part[2];
  int32_t n_part, reserved;
} MmtExpertIO;
/* Token plan: slot[b*S+s] -> row (or -1), cu_seqlens[B+1], *n_rows_dev, and per-row row_index (b*S+s),
 * type_ids, pos_ids (clamp(features_t,0,max_pos) model.py:516-520), mask_bias, agg_row[b*M+m].
 * pack=0 keeps all S=1+M*(T+1) slots; pack=1 drops padded FEA tokens (exact, see assemble.hip). */
/* Source-row compaction maps written by mmt_video_plan (device): the ReduceDim projections only see live rows.
 * Compact source matrix of expert e (x / y / dy of MmtExpertIO): rows [0, B) = the max-pooled vectors, rows B + i = the
 * valid feature rows in (sample, time) order. */
typedef struct MmtVideoSrc {
  int32_t* src_row; /* [token rows] compact source row of every live token inside its expert's matrix (-1: CLS) */
  int32_t* src_cnt; /* [M] live source rows per expert = B + valid feature rows                                   */
  int32_t* xsrc;    /* [M, B*T] feature row b*T + t behind compact row B + i                                      */
} MmtVideoSrc;
int mmt_video_plan(const MmtExpertIO* experts, int M, int B, int T, int pack, int max_pos, int32_t* counts,
                   int32_t* cu_seqlens, int32_t* n_rows_dev, int32_t* slot, int32_t* row_index, int32_t* type_ids,
                   int32_t* pos_ids, float* mask_bias, int32_t* agg_row, uint32_t* seed_bump, const MmtVideoSrc* src,
                   void* stream);
int mmt_video_cast(const MmtExpertIO* experts, int M, int B, int T, const MmtVideoSrc* src, void* stream);
int mmt_video_scatter(const MmtExpertIO* experts, int M, int B, int T, int d, const int32_t* n_rows_dev,
                      const int32_t* row_index, const MmtVideoSrc* src, float* features, void* stream);
int mmt_video_scatter_bwd(const MmtExpertIO* experts, int M, int B, int T, int d, const int32_t* n_rows_dev,
                          const int32_t* row_index, const MmtVideoSrc* src, const float* dfeatures, void* stream);

/* ---- read-out, similarity, losses (simloss.hip) --------------------------------------------------- */
/* vid_embds[i] = F.normalize(last_hidden[agg_row[i]]), i < B*M      model.py:583-587,621-625 */
int mmt_readout_fwd(const float* last_hidden, const int32_t* agg_row, int BM, int d, float* vid_embds,
                    float* inv_norm, void* stream);
/* writes the B*M AGG rows of dlast_hidden (all other rows must be zero beforehand) */
int mmt_readout_bwd(const float* vid_embds, const float* inv_norm, const float* dvid_embds,
                    const int32_t* agg_row, int BM, int d, float* dlast_hidden, void* stream);
/* sharded_cross_view_inner_product, model.py:789-837: txt [NT,M,d], vid [NV,M,d], tw [NT,M], vw [NV,M]
 * -> sims [NT,NV] (rows = text); dots = NT*NV*M floats saved for the backward (its layout is private to the pair of
 * calls; mmt_sims_bwd OVERWRITES it).  From 64 rows/columns on (the global batch of a data-parallel step) the per-expert
 * dot products and both embedding gradients run as batched exact-fp32 MFMA GEMMs. */
int mmt_sims_fwd(const float* txt, const float* vid, const float* tw, const float* vw, int NT, int NV, int M,
                 int d, float* sims, float* dots, void* stream);
int mmt_sims_bwd(const float* txt, const float* vid, const float* tw, const float* vw, float* dots,
                 const float* dsims, int NT, int NV, int M, int d, float* dtxt, float* dvid, float* dtw,
                 float* dvw, void* stream);
/* Small batches (n <= mmt_simloss_small_max_n() pairs, one caption per video -- the single-rank training step): the loss
 * (kind 0: MaxMarginRankingLoss(margin, fix_norm), loss.py:38-65; kind 1: InfoNceLoss, :68-81), its gradient wrt the
 * similarity matrix and the whole similarity backward (model.py:789-837) in ONE launch from the sims / dots of
 * mmt_sims_fwd.  dtxt/dvid [n, M, d], dtw/dvw [n, M] (each nullable).  dlast (nullable) + inv_norm [n*M]: also the
 * backward of the read-out normalisation (model.py:621-625): dlast[out_rows ? out_rows[i] : i] for i = v*M + m. */
int mmt_simloss_small_max_n(void);
int mmt_simloss_bwd_small(const float* txt, const float* vid, const float* tw, const float* vw, const float* sims,
                          const float* dots, int n, int M, int d, int kind, float margin, int fix_norm, float* loss,
                          float* dtxt, float* dvid, float* dtw, float* dvw, const float* inv_norm,
                          const int32_t* out_rows, float* dlast, void* stream);

/* MaxMarginRankingLoss.forward (loss.py:38-65): loss scalar + d loss/d sims; partial = n floats scratch. */
int mmt_maxmargin(const float* sims, int n, float margin, int fix_norm, float* partial, float* loss,
                  float* grad, void* stream);
/* InfoNceLoss.forward (loss.py:68-81); scratch = 3n floats. */
int mmt_infonce(const float* sims, int n, float* scratch, float* loss, float* grad, void* stream);

/* ---- evaluation path at scale (retrieval.hip): SURVEY.md 8f.1 ------------------------------------------------
 * Replaces the CPU-side sharded_cross_view_inner_product + numpy ranking of trainer/trainer.py:396-447.
 * mmt_sims_eval: same maths as mmt_sims_fwd but as one exact-fp32 MFMA GEMM over K = M*d (no [NT,NV,M] tensor, no
 * backward); ws = mmt_sims_eval_workspace_floats() floats.  Text rows are b*C + cap (model.py:805,822). */
int64_t mmt_sims_eval_workspace_floats(int NT, int NV, int M, int d);
int mmt_sims_eval(const float* txt, const float* vid, const float* tw, const float* vw, int NT, int NV, int M, int d,
                  float* ws, float* sims, void* stream);
/* Tie-averaged retrieval ranks (0-based, model/metric.py:90-121, 153-243) of sims [NQ = NV*cpv, NV]:
 * t2v_rank[q] for every text query; v2t_rank[i] = best rank among video i's unmasked captions (+inf if none).
 * qmask (nullable) uint8 [NQ]: 1 = real caption (query_masks).  scratch: NQ floats. */
int mmt_retrieval_ranks(const float* sims, const uint8_t* qmask, int NQ, int NV, float* t2v_rank, float* v2t_rank,
                        float* scratch, void* stream);

/* ---- gallery search (search.hip, search_bf16.hip, search_fp8.hip, search_rank.hip, search_subset.hip, search_shard.hip,
 * search_norm.hip, search_range.hip, search_group.hip, search_pool.hip, search_itemset.hip, search_rescore.hip; fold in
 * retrieval.hip) ------------------------------------------------------------------------------------------------
 * score(q, g) = sum_m qw[q][m] gw[g][m] <Q_m[q], G_m[g]> / sum_m qw[q][m] gw[g][m] (0 -> 1e-5), the 'indep' similarity
 * of model/model.py:789-837, computed tile by tile: no scan forms the NQ x NV matrix, none uses atomics, every output
 * slot has one writer, so every result is bit-reproducible.  The ORDER of every list is score descending, -0 tied with
 * +0, equal scores by ascending item number (a stable argsort; the reference's np.argsort leaves exact ties unspecified).
 *
 * Storage.  The index keeps the folded rows gf = gw (.) G [NV][M*d] in one of three forms; a scan is told which by
 * MmtSearchScan.storage:
 *   MMT_SEARCH_FP32: fp32 rows, fp32 query rows qf = fold(Q, qw) (mmt_search_fold), fp32 MFMAs.  d % 4 == 0.
 *   MMT_SEARCH_BF16: bf16(gf), rounded once, round-to-nearest-even.  Only storage is lossy; the score is defined on the
 *     stored value, with the fp32 query carried as q = hi = bf16(qf), q_lo = lo = bf16(qf - hi) (mmt_search_fold_split_bf16;
 *     two bf16 MFMAs per gallery fragment, fp32 accumulation; residual < 2^-16 relative per query element).  Against fp32
 *     storage a score moves by at most 2^-8 * sum_m qw gw <|Q_m|, |G_m|> / sum_m qw gw.  d % 8 == 0.
 *   MMT_SEARCH_FP8: with f the fp32 folded row, scale = 2^e, the smallest power of two with max_k |f[k]| / 2^e <= 448 (e
 *     clamped to -120 .. 120; an all-zero row: 1), and stored = e4m3fn_rne(f / scale): OCP e4m3fn codes, round-to-nearest-
 *     even with subnormals, never saturating (mmt_search_fold_fp8; inputs are taken to be finite).  The score is
 *     fl( fl(acc * gscale[g]) / den ), acc as the bf16 scan computes it from the hi / lo pair (every e4m3fn value is a
 *     bf16 value), the scale multiply rounded on its own.  Against fp32 storage a score moves by at most
 *     ( 2^-4 * <|qf|, |f|> + 2^-10 * scale[g] * sum_k |qf[k]| ) / |den|.  d % 16 == 0.
 * Folded rows are 16-byte aligned in every form.
 *
 * mmt_search_fold: out = w (.) x for x [N][M][d] (d % 4 == 0, 16-byte aligned), w [N][M] -> out [N][M*d].
 * mmt_search_fold_bf16: out = bf16(w (.) x); out may point at a row of a larger preallocated buffer.
 * mmt_search_fold_split_bf16: the query pair hi, lo [N][M*d] in one launch.
 * mmt_search_fold_fp8: out = the codes [N][M*d], scale fp32 [N]; both may point into larger preallocated buffers.
 * mmt_rows_topk: the selection of mmt_search_topk on a given fp32 matrix (row stride ld), rows r = rows[i] for output row
 *   i (nullable: i itself) -- utils/util.py:38-68 compress_predictions (trainer/trainer.py:411-437 'final_eval'; the
 *   visualiser's ranking, utils/visualizer.py:74-92).  Workspace: mmt_topk_workspace_keys. */
int mmt_search_fold(const float* x, const float* w, int N, int M, int d, float* out, void* stream);
int mmt_search_fold_bf16(const float* x, const float* w, int N, int M, int d, uint16_t* out, void* stream);
int mmt_search_fold_split_bf16(const float* x, const float* w, int N, int M, int d, uint16_t* hi, uint16_t* lo,
                               void* stream);
int mmt_search_fold_fp8(const float* x, const float* w, int N, int M, int d, uint8_t* out, float* scale, void* stream);
int mmt_rows_topk(const float* sims, int64_t ld, const int32_t* rows, int NR, int NV, int k, uint64_t* ws, float* scores,
                  int64_t* index, void* stream);

/* One scan, described: everything about it except what the operation itself consumes and produces.  Every mmt_search_*
 * scan below takes one.  A part that is not wanted is null / 0; a part the operation, the storage or another part has no
 * kernel for is REFUSED (MMT_ERR_ARG before any launch), never ignored -- the supported combinations are listed with the
 * entries and in DESIGN 9.15.
 *   q, q_lo, qw : query rows [NQ][M*d] -- fp32: q = qf, q_lo null; bf16 / fp8: the hi / lo pair -- and weights [NQ][M].
 *   g, gw, gscale: stored rows [NV][M*d] in `storage`, weights [NV][M]; gscale fp32 [NV] with fp8 and only then.
 *   subset  : nullable = every item.  uint32 words, bit i & 31 of word i >> 5 = item i allowed; 4 * ceil(NV / 128) words
 *             (one 128-item scan tile = one aligned 16-byte load), bits at or past NV zero, 16-byte aligned
 *             (mmt_search_subset_pack: mask [NV] bytes, nonzero = allowed, -> those words).  A tile with no bit set is
 *             skipped before its K loop.  With item sets the bits number SETS.
 *   exclude, E: per query the E items exclude[q][0 .. E - 1] (int64, -1 .. NV - 1, -1 = none; duplicates and items outside
 *             the subset are fine) are no candidates.  0 <= E <= 32; exclude non-null exactly when E > 0.
 *   after   : nullable = no cursor.  uint64 [NQ] bounds of mmt_search_after_keys: a row's candidates are the items whose
 *             key is strictly below its bound (see there).
 *   lse, beta: nullable / 0 = no norm.  Querybank normalisation: lse fp32 [NV] of mmt_search_col_lse and 0 < beta < inf;
 *             the scan works on score'(q, g) = fl(fl(beta * score(q, g)) - lse[g]).  One of the two without the other is
 *             MMT_ERR_ARG.
 *   sets, set_size, mode, set_weights: MMT_SEARCH_SETS_NONE (the other three 0 / null), or
 *             MMT_SEARCH_SETS_QUERY: the queries are NQ / set_size sets of set_size consecutive rows (1 .. 64), or
 *             MMT_SEARCH_SETS_ITEM : the stored items are NV / set_size sets of set_size consecutive items (1 .. 128);
 *             every scan then answers per SET on the pooled score (below).  set_weights fp32 [NQ] resp. [NV]; mode 0 =
 *             mean, 1 = max.  NQ resp. NV must be a whole number of sets.
 *   NQ, NV, M, d: query rows, stored items, experts (1 .. 16), width per expert (a multiple of 4 / 8 / 16 by storage).
 * Pooled score of a set over its participating members r0 < r1 < ... (weight != 0), in member order, with s(r) the score
 * of the member's pair:  mode 0: v = fl(w[r0] * s(r0)), then v = fl(v + fl(w[ri] * s(ri))) -- a rounded multiply, then a
 * rounded add, never an fma, never reassociated (w = 1 / C: model/model.py:826-831 'avg');  mode 1: v = s(r0), then
 * v = s(ri) where s(ri) > v (a plain compare; the weights are a mask).  Trusted, not checked: weights finite, every set
 * has a member with weight != 0 (a set without one pools to 0). */
#define MMT_SEARCH_FP32 0
#define MMT_SEARCH_BF16 1
#define MMT_SEARCH_FP8 2
#define MMT_SEARCH_SETS_NONE 0
#define MMT_SEARCH_SETS_QUERY 1
#define MMT_SEARCH_SETS_ITEM 2
typedef struct MmtSearchScan {
  const void* q;
  const void* q_lo;
  const float* qw;
  const void* g;
  const float* gw;
  const float* gscale;
  const uint32_t* subset;
  const int64_t* exclude;
  const uint64_t* after;
  const float* lse;
  const float* set_weights;
  int32_t storage;
  int32_t NQ;
  int32_t NV;
  int32_t M;
  int32_t d;
  int32_t E;
  float beta;
  int32_t sets;
  int32_t set_size;
  int32_t mode;
} MmtSearchScan;
#ifdef __cplusplus
static_assert(sizeof(MmtSearchScan) == 128, "MmtSearchScan: 11 pointers, then 10 four-byte fields");
#else
_Static_assert(sizeof(MmtSearchScan) == 128, "MmtSearchScan: 11 pointers, then 10 four-byte fields");
#endif

/* The scans.  Common gates, before any launch: MMT_ERR_ARG -- a null descriptor, an unknown storage or sets tag, a null
 * operand, output or workspace (scores of mmt_search_topk may be null), NQ / NV < 1, M outside 1 .. 16, d < 1 or off the
 * storage's multiple, an unsupported combination; MMT_ERR_ALIGN -- q, q_lo, g or subset off a 16-byte boundary.  "R" is
 * the number of result rows: NQ, with query sets NQ / set_size.  "N" is what indices, targets and subset bits number:
 * the NV items, with item sets the NV / set_size sets.
 * Supported everywhere: fp32 and bf16.  fp8: with subset, exclude and after only (no norm, no sets).  Sets: fp32 and bf16,
 * with subset only (no norm, exclude or after), never both kinds.
 *
 * mmt_search_topk (subset, exclude, after, norm, sets): per result row the best min(k, N) candidates, scores (nullable)
 *   fp32 / index int64 [R][min(k, N)], 1 <= k <= 128.  Fused scoring + selection per gallery chunk, then a merge launch.
 *   Without subset, exclude, after, norm and sets the unmasked kernel runs and every slot is written; otherwise ONLY the
 *   slots that have a candidate are written (the caller prefills).  The score of a returned item has the bits the
 *   unmasked search gives it: masks act at selection only.  With norm the scores are score'.
 * mmt_search_topk_groups (subset): the k best GROUPS of a gallery whose items carry a group id (the clips of a video), each
 *   with its best item.  group_ids int32 [NV], values >= 0 (trusted), any labelling.  Per query the representative of a
 *   group is its best allowed member; groups rank by their representatives.  1 <= k <= 128 (the caller passes min(k,
 *   number of groups)).  Outputs [NQ][k]: scores fp32, groups int64, items int64; slots past the last group hold
 *   (-inf, -1, -1).  Workspace as mmt_search_topk.
 * mmt_search_rank (subset): for every query and each of its T targets (int64 [NQ][T], 1 <= T <= 32)
 *     greater[q][t] = #{allowed g : score(q, g) > score(q, targets[q][t])},  equal[q][t] = #{allowed g : score(q, g) == ...}
 *   as int32 [NQ][T]; the reference's tie-averaged 0-based rank (model/metric.py:90-121, 153-243) is greater +
 *   (equal - 1) / 2.  The threshold is the very value the scan computes for the target (scored whether allowed or not),
 *   plain float compares (-0 == +0, NaN counts for nothing).  A target outside 0 .. NV - 1 (-1 = none) is checked on the
 *   device, never dereferenced, and gets 0 / 0.  = mmt_search_thresholds, then mmt_search_count, in one call.
 * mmt_search_thresholds (norm, sets): the threshold pass alone: thr[r][t] = score (norm: score', sets: pooled score) of
 *   (r, targets[r][t]) as fp32 [R][T] with the bits the other passes compute for the pair, NaN for a target outside
 *   0 .. N - 1.  The same value wherever the item is stored and whatever NV is, so a gallery cut into shards scores a
 *   target on the shard that holds it.
 * mmt_search_count (subset, norm, sets): thr fp32 [R][T] -> greater / equal int32 [R][T] over the allowed candidates
 *   (a NaN threshold counts nothing).  The int32 counts of shards add up to those of one index.
 * mmt_search_range_count, mmt_search_range_fill (subset): every allowed item with score(q, g) >= thr[q] (fp32 [NQ]; NaN
 *   hits nothing, -inf everything), however many, as a CSR.  The count pass writes row_counts int64 [NQ] and leaves ws
 *   holding, per query, the exclusive prefix of its chunk counts; the fill pass of the very same descriptor and thr reads
 *   it, with offsets int64 [NQ + 1] the exclusive prefix of row_counts (offsets[0] may be any base), and writes query q's
 *   hits to indices int64 / scores fp32 [offsets[q], offsets[q + 1]) by ascending item.  A position is clamped against
 *   the start of the row's next chunk, so the pass writes nothing outside [offsets[0], offsets[NQ]).
 * mmt_search_rescore (no options; fp32, bf16, fp8): "the k best among THESE items".  candidates int64 [NQ][C],
 *   1 <= C <= 1024, any order, an item may repeat, a value outside 0 .. NV - 1 is ignored -> scores fp32 / index int64
 *   [NQ][min(k, C)], 1 <= k <= 128: the best distinct candidates in the search's order, then (-inf, -1).  A score has the
 *   bits mmt_search_topk gives the pair, decoded from the key (a -0 comes back as +0).
 * mmt_search_col_lse (no options; fp32, bf16; the descriptor's lse and beta stay null / 0: the operation writes lse): the
 *   inverted softmax over a bank of queries, the static half of QB-Norm (Bogolin et al., CVPR 2022).  The descriptor's
 *   query rows are one batch of the bank; with x(b, g) = fl(beta * score(b, g)), lse[g] = log sum_b exp(x(b, g)), computed
 *   blockwise: every 64-row bank block gives m = max x and p = sum exp(x - m) per item, rows ascending, and the blocks
 *   are folded in ascending order, M' = max(M, m), S' = S exp(M - M') + p exp(m - M'), lse = M + log S -- a function of the
 *   item's stored row and weights, the bank in its row order and beta only.  state fp32 [2][NV] (M, then S): first != 0
 *   starts it, otherwise it is what the previous batch left; every batch but the last holds a multiple of 64 rows.  lse
 *   (nullable) fp32 [NV]: written when given, i.e. with the last batch.  ws 16-byte aligned (else MMT_ERR_ALIGN); beta not
 *   finite or <= 0 is MMT_ERR_ARG.
 *
 * Workspaces (MMT_ERR_ARG if a size is out of range): a gallery chunk is 4096 columns, smaller only when the launch would
 * not fill the chip.  mmt_topk_workspace_keys: uint64, NQ * ceil(NV / chunk) * k (mmt_search_topk, _topk_groups,
 * mmt_rows_topk).  mmt_rank_workspace_ints: int32, NQ * T * (1 + 2 * ceil(NV / chunk)).  mmt_count_workspace_ints: int32,
 * NQ * T * 2 * ceil(NV / chunk).  mmt_range_workspace_ints: int32, NQ * ceil(NV / chunk).  mmt_col_lse_workspace_floats:
 * fp32, 2 * ceil(NB / 64) * NV.  mmt_rescore_workspace_keys: uint64, NQ * C.  With query sets (NS sets of C rows: a block
 * holds 64 / C sets and the chunk rule counts blocks) mmt_topk_pooled_workspace_keys / mmt_count_pooled_workspace_ints;
 * with item sets (NT sets of C items: a 128-column tile holds 128 / C whole sets and a chunk is a whole number of tiles)
 * mmt_topk_itemsets_workspace_keys / mmt_count_itemsets_workspace_ints. */
int64_t mmt_topk_workspace_keys(int NQ, int NV, int k);
int64_t mmt_rank_workspace_ints(int NQ, int NV, int T);
int64_t mmt_count_workspace_ints(int NQ, int NV, int T);
int64_t mmt_range_workspace_ints(int NQ, int NV);
int64_t mmt_col_lse_workspace_floats(int NB, int NV);
int64_t mmt_rescore_workspace_keys(int NQ, int C);
int64_t mmt_topk_pooled_workspace_keys(int NS, int C, int NV, int k);
int64_t mmt_count_pooled_workspace_ints(int NS, int C, int NV, int T);
int64_t mmt_topk_itemsets_workspace_keys(int NQ, int NT, int C, int k);
int64_t mmt_count_itemsets_workspace_ints(int NQ, int NT, int C, int T);
int mmt_search_topk(const MmtSearchScan* scan, int k, uint64_t* ws, float* scores, int64_t* index, void* stream);
int mmt_search_topk_groups(const MmtSearchScan* scan, int k, const int32_t* group_ids, uint64_t* ws, float* scores,
                           int64_t* groups, int64_t* items, void* stream);
int mmt_search_rank(const MmtSearchScan* scan, const int64_t* targets, int T, int32_t* ws, int32_t* greater,
                    int32_t* equal, void* stream);
int mmt_search_thresholds(const MmtSearchScan* scan, const int64_t* targets, int T, float* thr, void* stream);
int mmt_search_count(const MmtSearchScan* scan, const float* thr, int T, int32_t* ws, int32_t* greater, int32_t* equal,
                     void* stream);
int mmt_search_range_count(const MmtSearchScan* scan, const float* thr, int32_t* ws, int64_t* row_counts, void* stream);
int mmt_search_range_fill(const MmtSearchScan* scan, const float* thr, const int32_t* ws, const int64_t* offsets,
                          int64_t* indices, float* scores, void* stream);
int mmt_search_rescore(const MmtSearchScan* scan, const int64_t* candidates, int C, int k, uint64_t* ws, float* scores,
                       int64_t* index, void* stream);
int mmt_search_col_lse(const MmtSearchScan* scan, float beta, float* ws, float* state, int first, float* lse,
                       void* stream);

/* The tenth scan, additive: no existing entry, field or cell changes and mmt_abi_version() stays 6.  It serves
 * search.py's `reverse_search` (the lists) and `csls_norm` (the mean, which takes the place of lse in the norm slot with
 * beta = 2: Cross-domain Similarity Local Scaling, Conneau et al., ICLR 2018).
 * mmt_search_col_topk (no options; fp32, bf16, fp8): the running top-k per ITEM over a stream of query rows -- for every
 *   stored item the k best query rows, 1 <= k <= MMT_SEARCH_MAX_RK.  The descriptor's query rows are one batch; row0 >= 0
 *   is the global number of its first row (row0 + NQ <= 2^31), and every batch but the last holds a multiple of 64 rows.
 *   Every 64-row block gives, per item, its best min(k, live rows) keys -- (score, global row) in the search's key, so
 *   score descending, -0 tied with +0, equal scores by ascending row -- and a fold launch merges them with the carried
 *   lists.  Keys of distinct rows are distinct, so the k best of a union do not depend on the batching, the chunk rule,
 *   NV, the item's position or the shard.  state uint64 [NV][k]: first != 0 starts it, otherwise it is what the previous
 *   batch left.  scores fp32 / rows int64 [NV][k] and mean fp32 [NV], each nullable, are written when given, i.e. with the
 *   last batch: slot j of item g holds its j-th best row and the score with the bits mmt_search_topk gives the pair (a -0
 *   comes back as +0); a slot past the number of rows seen holds (-inf, -1).  mean[g] = fl(fl(.. fl(s_0 + s_1) .. +
 *   s_{k'-1}) * mean_weight) over the item's k' = min(k, rows seen) scores in list order -- rounded adds, then one rounded
 *   multiply, never an fma (the caller passes mean_weight = float32(1 / k')).  ws and state 16-byte aligned (else
 *   MMT_ERR_ALIGN).  mmt_col_topk_workspace_keys: uint64, ceil(NB / 64) * NV * k; MMT_ERR_ARG for a size < 1 or k out of
 *   range. */
#define MMT_SEARCH_MAX_RK 32
int64_t mmt_col_topk_workspace_keys(int NB, int NV, int k);
int mmt_search_col_topk(const MmtSearchScan* scan, int k, int row0, uint64_t* ws, uint64_t* state, int first,
                        float* scores, int64_t* rows, float* mean, float mean_weight, void* stream);

/* Diversified search (search_diverse.hip), additive like the tenth scan: two entries without a descriptor, nothing that
 * exists changes and mmt_abi_version() stays 6.  They serve search.py's `pair_scores`, `diversify` and `search_diverse`:
 * max marginal relevance (Carbonell & Goldstein, SIGIR 1998) over a shortlist.
 * mmt_search_pair_scores (fp32, bf16, fp8): the similarity of STORED items to each other.  g [NV][M * d] in `storage`
 *   (MMT_SEARCH_FP32 / _BF16 / _FP8), gw fp32 [NV][M], gscale fp32 [NV] with fp8 and null otherwise; items int64 [R][C],
 *   1 <= C <= MMT_SEARCH_MAX_DC, a value outside 0 .. NV - 1 is "none": checked on the device, never dereferenced -> sims
 *   fp32 [R][C][C], sims[r][i][j] = sim(items[r][i], items[r][j]), NaN where either is none:
 *     sim(g, h) = <f_g, f_h> / sum_m gw[g][m] gw[h][m]   (0 -> 1e-5),  f_g the dequantised stored row
 *   the score of the scans with item g in the query's place.  fp32 accumulation on the matrix cores (fp32 rows:
 *   v_mfma_f32_32x32x2_f32; bf16 rows and fp8 codes, which are exact bf16 values: one v_mfma_f32_32x32x16_bf16 per fragment);
 *   the denominator is fma(gw[g][m], gw[h][m], den) for m ascending; with fp8 the accumulator is multiplied by
 *   fl(gscale[g] * gscale[h]) -- powers of two -- as one rounded multiply before the division.  sim(g, h) has the bits of
 *   sim(h, g) and is a function of the two stored rows, their weights and scales only: not of their places in the list, the
 *   other candidates, R, NV or the shard.  One block per list; no workspace.  MMT_ERR_ARG: a null g, gw, items or sims, an
 *   unknown storage, gscale given without fp8 or missing with it, C out of range, R / NV < 1, M outside 1 .. 16, d < 1 or
 *   off the storage's multiple; MMT_ERR_ALIGN: g off a 16-byte boundary.
 * mmt_search_mmr: the selection.  items int64 / rel fp32 [R][C]: per row a list of distinct candidates in the search's order
 *   with its relevances, padded with (-1, -inf) -- what mmt_search_rescore with k = C returns; sims fp32 [R][C][C] the Gram of
 *   exactly that list (mmt_search_pair_scores).  With n the number of items >= 0 (taken to be positions 0 .. n - 1), in fp32:
 *   slot 0 is position 0 with value fl(a * rel[0]); for slot t >= 1 every unselected position p has pen_p, the largest
 *   sim(p, s) over the selected s (a plain compare, the first of equals stays) and v_p = fl(fl(a * rel[p]) - fl(b * pen_p)) --
 *   two rounded multiplies and a rounded subtract, never an fma -- and the position with the largest v_p is selected, -0
 *   tied with +0, equal values to the lowest p (the order of the search's key over (v_p, p)).  Slot t of scores fp32 / index
 *   int64 / values fp32 [R][k] holds (rel[p], items[p], v_p); slots from min(k, n) on hold (-inf, -1, -inf).  1 <= k <= C
 *   <= MMT_SEARCH_MAX_DC, R >= 1 and no null pointer, else MMT_ERR_ARG.  One wave per row; no atomics in either entry. */
#define MMT_SEARCH_MAX_DC 128
int mmt_search_pair_scores(const void* g, const float* gw, const float* gscale, int storage, int NV, int M, int d,
                           const int64_t* items, int R, int C, float* sims, void* stream);
int mmt_search_mmr(const int64_t* items, const float* rel, const float* sims, int R, int C, int k, float a, float b,
                   float* scores, int64_t* index, float* values, void* stream);

/* The gallery self-join (search_self.hip), additive like the entries above: three entries and two size functions without
 * a descriptor, nothing that exists changes and mmt_abi_version() stays 6.  They serve search.py's `neighbours`,
 * `neighbour_range` and `duplicate_groups`: the stored items searched against the stored items -- near-duplicate joins over
 * a clip gallery (re-uploads, crops, windows of one video) without the NV x NV matrix.  The quantity is
 * mmt_search_pair_scores' sim(g, h) = <f_g, f_h> / sum_m gw[g][m] gw[h][m] (0 -> 1e-5) on the stored values ('indep'
 * similarity, model/model.py:789-837, with a stored item in the query's place), and every score these entries return has
 * exactly the bits mmt_search_pair_scores gives the pair: the same slab and MFMA sequence along K, one accumulator per
 * output, the same fma chain for the denominator, the same rounded multiplies for the fp8 scales.  It does not depend on
 * the row batching, the launch geometry, NV, the items' positions or the shard.
 * Each entry takes TWO stored operands in one `storage` (MMT_SEARCH_FP32 / _BF16 / _FP8), M and d:
 *   A side, the rows: a_rows [NA][M * d], a_weights fp32 [NA][M], a_scales fp32 [NA] with fp8 and null otherwise; items int64
 *     [R] (nullable = row r of A is row r of the join, then R <= NA), a value outside 0 .. NA - 1 is "none": checked on the
 *     device, never dereferenced; self int64 [R] (nullable = none): the B-side item number row r must not meet, -1 = none
 *     -- the self pair is left out by NUMBER, not by score, so an exact copy of an item stays in its list.
 *   B side, the columns: g [NV][M * d], gw fp32 [NV][M], gscale fp32 [NV] with fp8; subset (nullable = every item): the
 *     packed bitmap of mmt_search_subset_pack, only its items are candidates.
 *   On one index the caller passes A = B and self = items; a gallery cut into shards passes a staged block of the rows
 *   as A to every shard, with self the row's local number there or -1.
 * mmt_search_self_topk: per row the best candidates in the search's order (score descending, -0 tied with +0, equal scores
 *   by ascending item) as scores fp32 / index int64 [R][k], 1 <= k <= 128.  ONLY the slots that have a candidate are
 *   written (the caller prefills (-inf, -1)).  ws uint64 [mmt_self_topk_workspace_keys(R, NV, k)] = R * ceil(NV / chunk) * k.
 * mmt_search_self_range_count, mmt_search_self_range_fill: every candidate with sim >= thr[r] (fp32 [R]; a plain compare:
 *   NaN hits nothing, -inf everything) as a CSR, the two passes of mmt_search_range_count / _fill: the count pass writes
 *   row_counts int64 [R] and leaves ws (int32 [mmt_self_range_workspace_ints(R, NV)] = R * ceil(NV / chunk)) holding per row
 *   the exclusive prefix of its chunk counts; the fill pass of the very same arguments reads it, with offsets int64 [R + 1]
 *   the exclusive prefix of row_counts, and writes row r's hits to indices int64 / scores fp32 [offsets[r], offsets[r + 1])
 *   by ascending item.  A position is clamped against the start of the row's next chunk.
 * MMT_ERR_ARG: a null a_rows, a_weights, g, gw, output or workspace, an unknown storage, a_scales / gscale given without
 *   fp8 or missing with it, NA / R / NV < 1, items null with R > NA, M outside 1 .. 16, d < 1 or off the storage's multiple,
 *   k outside 1 .. 128; MMT_ERR_ALIGN: a_rows, g or subset off a 16-byte boundary.  All refused before any launch.  No
 *   atomics; one writer per slot. */
int64_t mmt_self_topk_workspace_keys(int R, int NV, int k);
int64_t mmt_self_range_workspace_ints(int R, int NV);
int mmt_search_self_topk(const void* a_rows, const float* a_weights, const float* a_scales, int NA, const int64_t* items,
                         const int64_t* self, int R, const void* g, const float* gw, const float* gscale, int NV,
                         const uint32_t* subset, int storage, int M, int d, int k, uint64_t* ws, float* scores,
                         int64_t* index, void* stream);
int mmt_search_self_range_count(const void* a_rows, const float* a_weights, const float* a_scales, int NA,
                                const int64_t* items, const int64_t* self, int R, const void* g, const float* gw,
                                const float* gscale, int NV, const uint32_t* subset, int storage, int M, int d,
                                const float* thr, int32_t* ws, int64_t* row_counts, void* stream);
int mmt_search_self_range_fill(const void* a_rows, const float* a_weights, const float* a_scales, int NA,
                               const int64_t* items, const int64_t* self, int R, const void* g, const float* gw,
                               const float* gscale, int NV, const uint32_t* subset, int storage, int M, int d,
                               const float* thr, const int32_t* ws, const int64_t* offsets, int64_t* indices, float* scores,
                               void* stream);

/* Softmax over the gallery (search_lse.hip), additive: one scan over the descriptor and its size function, nothing that
 * exists changes and mmt_abi_version() stays 6.  It serves search.py's `query_lse` and `search_softmax`: the row-wise
 * log-partition of softmax(beta * score(q, .)) over a query's candidates, as an INTEGER sum, so that the result is one
 * number whatever the chunking, the row batching, the launch geometry, the item order or the shard.
 * mmt_search_row_expsum (subset; fp32, bf16, fp8): per query row, over the allowed items g, in fp32
 *     x = fl(beta * score(q, g)),  e = expf(x - xmax[q]),  t = (int64) rint(ldexpf(e, F)),   ws[q][c] = sum of t over chunk c
 *   score the bits mmt_search_topk gives the pair (the scans' own tile), the multiply rounded on its own, expf the
 *   expression of mmt_search_col_lse's column pass.  xmax fp32 [NQ]: fl(beta * the row's top-1 score among the same
 *   candidates), the caller's mmt_search_topk with k = 1, so that e <= 1 and the top-1 item gives exactly 2^F.  F: the
 *   caller's 62 - ceil(log2(max(N, 2))) for the N items of the WHOLE gallery (all shards), 0 <= F <= 62: every term is at
 *   most 2^F and there are at most 2^(62 - F) of them, so no int64 sum overflows.  ws int64
 *   [mmt_row_expsum_workspace_ints64(NQ, NV)] = [NQ][ceil(NV / chunk)], every slot written (0 for a chunk without an
 *   allowed item); the caller adds a row's slots -- and the shards' -- in any order.  MMT_ERR_ARG: a part of the descriptor
 *   other than subset, a null operand, xmax or ws, beta not finite or <= 0, F outside 0 .. 62, and the common shape gates;
 *   MMT_ERR_ALIGN: q, q_lo, g or subset off a 16-byte boundary.  All refused before any launch.  No atomics; one writer per
 *   slot. */
int64_t mmt_row_expsum_workspace_ints64(int NQ, int NV);
int mmt_search_row_expsum(const MmtSearchScan* scan, float beta, const float* xmax, int F, int64_t* ws, void* stream);

/* The streaming schedule of the plain top-k scan (search_stream.hip), additive: one entry and its size function, nothing
 * that exists changes and mmt_abi_version() stays 6.  It serves search.py's `search` on an index whose schedule is 'stream': the search
 * of a handful of queries (a service answering one caption, or a few), where the gallery is read once and its bytes are
 * the cost -- the same similarity and the same order as mmt_search_topk (reference: utils/util.py:38-68
 * compress_predictions, trainer/trainer.py:411-437, utils/visualizer.py:74-92; similarity of model/model.py:789-837).
 * mmt_search_topk_stream (subset, exclude, after; fp32, bf16, fp8; no norm, no sets: MMT_ERR_ARG): outputs, k, gates and
 *   the rule for which slots are written exactly as mmt_search_topk.  THE CONTRACT: scores and indices are those of
 *   mmt_search_topk for the same descriptor, BIT FOR BIT.  A (query, item) accumulator goes through the same MFMA sequence
 *   (bf16 / fp8: K ascending in steps of 16, lane half h feeding k = kk + 8h .. + 7, one v_mfma_f32_32x32x16_bf16 per query
 *   plane, hi then lo; fp32: K ascending in steps of 8, four v_mfma_f32_32x32x2_f32 with k = kk + 4h + u) and the same
 *   epilogue expression (the `den += qw[m] * gw[m]` chain, 0 -> 1e-5, fp8: the rounded multiply by the scale first, then
 *   num / den); the keys and the running top-k are shared, and the merge of the chunk lists is by rank as well, over the
 *   lists whose heads can reach the answer (a rank is unique, so the output is that merge's).  Only the schedule differs:
 *   a block holds 32 query rows, the gallery goes from memory straight to the registers of the lane that multiplies it, a
 *   slab ahead, and never through LDS.  Meant for NQ <= 32; any NQ is taken, in tiles of 32 rows.
 * mmt_topk_stream_workspace_keys: uint64, NQ * n_chunks * k with n_chunks a function of (NQ, NV) only, non-decreasing in
 *   NV: the 512-item sweeps of the gallery cut into min(sweeps, max(512 / ceil(NQ / 32), ceil(sweeps / 8))) runs.
 *   MMT_ERR_ARG if a size is out of range; for both entries that includes NV > INT_MAX - 512 (a sweep's last tile numbers up
 *   to 511 items past NV, and an item number is an int).  MMT_ERR_ALIGN: q, q_lo, g or subset off a 16-byte boundary.  All refused on
 *   the host before any launch.  No atomics; one writer per slot. */
int64_t mmt_topk_stream_workspace_keys(int NQ, int NV, int k);
int mmt_search_topk_stream(const MmtSearchScan* scan, int k, uint64_t* ws, float* scores, int64_t* index, void* stream);

/* Per-query attribute filters, additive: five entries, nothing that exists changes, MmtSearchScan stays 21 fields / 128
 * bytes and mmt_abi_version() stays 6.  Every stored item carries one 64-bit tag word, tags [NV]; every query row three
 * 64-bit masks, where [NQ][3] = (all_of, none_of, any_of).  Item g is a candidate of row q iff
 *   (tags[g] & all_of) == all_of  and  (tags[g] & none_of) == 0  and  (any_of == 0 or (tags[g] & any_of) != 0)
 * -- plain 64-bit integer operations on bit patterns (bit 63 is an ordinary bit); three zero masks admit every item.  The
 * predicate is ANDed with the descriptor's subset, exclusions and cursor and acts at selection and counting only: a
 * returned score has the bits the unfiltered entry gives the pair.  A 128-item tile in which no (live row, allowed item)
 * pair passes is skipped before its K loop on the tile schedule (an exact, block-uniform test); the streaming schedule
 * filters in the selection alone.  Each entry takes the unfiltered entry's arguments with tags and where right behind the
 * descriptor, and its workspace, outputs, written slots and gates:
 *   mmt_search_topk_where         as mmt_search_topk          (subset, exclude, after; fp32, bf16, fp8)
 *   mmt_search_topk_stream_where  as mmt_search_topk_stream   (subset, exclude, after; fp32, bf16, fp8)
 *   mmt_search_count_where        as mmt_search_count         (subset; fp32, bf16, fp8): thresholds from the unfiltered
 *                                 mmt_search_thresholds, so a target is scored whether or not it passes and counts itself
 *                                 only if it does
 *   mmt_search_range_count_where  as mmt_search_range_count   (subset; fp32, bf16, fp8)
 *   mmt_search_range_fill_where   as mmt_search_range_fill    (subset; fp32, bf16, fp8)
 * MMT_ERR_ARG: a norm, sets, any other part the entry does not take, a null tags or a null where, and the unfiltered
 * entry's own refusals -- all before the alignment check (MMT_ERR_ALIGN: q, q_lo, g or subset off a 16-byte boundary).  All
 * refused on the host before any launch.  No atomics; one writer per slot. */
int mmt_search_topk_where(const MmtSearchScan* scan, const uint64_t* tags, const uint64_t* where, int k, uint64_t* ws,
                          float* scores, int64_t* index, void* stream);
int mmt_search_topk_stream_where(const MmtSearchScan* scan, const uint64_t* tags, const uint64_t* where, int k, uint64_t* ws,
                                 float* scores, int64_t* index, void* stream);
int mmt_search_count_where(const MmtSearchScan* scan, const uint64_t* tags, const uint64_t* where, const float* thr, int T,
                           int32_t* ws, int32_t* greater, int32_t* equal, void* stream);
int mmt_search_range_count_where(const MmtSearchScan* scan, const uint64_t* tags, const uint64_t* where, const float* thr,
                                 int32_t* ws, int64_t* row_counts, void* stream);
int mmt_search_range_fill_where(const MmtSearchScan* scan, const uint64_t* tags, const uint64_t* where, const float* thr,
                                const int32_t* ws, const int64_t* offsets, int64_t* indices, float* scores, void* stream);

/* The per-expert breakdown of a score (search_explain.hip), additive: one entry with plain arguments, nothing that exists
 * changes and mmt_abi_version() stays 6.  It serves search.py's `expert_scores`, `search_explained` and
 * `pair_expert_scores`: which expert produced a match, and with what share of the gate -- the score of the scans is a sum
 * over experts of terms that share one denominator, so it decomposes exactly.
 * mmt_search_expert_parts (fp32, bf16, fp8): qf fp32 [R][M * d], rows ALWAYS in fp32 (mmt_search_fold's; or dequantised
 *   stored rows in a query's place), qw fp32 [R][M]; g [NV][M * d] in `storage` (MMT_SEARCH_FP32 / _BF16 / _FP8), gw fp32
 *   [NV][M], gscale fp32 [NV] with fp8 and null otherwise -- not a descriptor entry: MmtSearchScan's q / q_lo mean the bf16
 *   pair on a bf16 or fp8 gallery.  candidates int64 [R][C], 1 <= C <= MMT_SEARCH_MAX_C, any order, repeats allowed, a
 *   value outside 0 .. NV - 1 is "none": checked on the device, never dereferenced -> parts, mix fp32 [R][C][M], NaN in all
 *   M slots of a none.  With f_g the dequantised stored row and den = fma(qw[m], gw[g][m], den) over m ascending, 0 -> 1e-5:
 *     dot_m  = sum_{j < d} qf[m d + j] * f_g[m d + j]
 *     part_m = dot_m / den                        fp8: fl(fl(dot_m * gscale[g]) / den) on the codes, a rounded multiply
 *     mix_m  = fl(qw[m] * gw[g][m]) / den         both quotients correctly rounded divisions
 *   sum_m part_m is the score of the pair on the stored value, sum_m mix_m is 1 (0 where den was 0), part_m / mix_m the
 *   similarity under expert m alone.  dot_m is one fp32 fma chain per lane -- lane l of a wave takes the 16-byte groups l,
 *   l + 64, ... of the expert's d values, elements ascending -- then a fixed butterfly over the 64 lanes: an order that is a
 *   function of (d, storage) and the element index alone, so a pair's values depend on the pair alone, bit for bit -- not
 *   on its place in the list, the other candidates, C, R or the launch geometry -- and with stored rows as qf the values of
 *   (g, h) have the bits of (h, g).  Within (d + M + 4) * 2^-24 * <|qf_m|, |f_g,m|> / |den| of the fp64 value.  One wave
 *   per pair on the vector ALUs, 16-byte loads of the stored row; no workspace.
 * MMT_ERR_ARG: a null qf, qw, g, gw, candidates, parts or mix, an unknown storage, gscale given without fp8 or missing with
 *   it, C out of range, R / NV < 1, M outside 1 .. 16, d < 1 or off the storage's multiple, R * ceil(C / 16) beyond a grid;
 *   then MMT_ERR_ALIGN: qf or g off a 16-byte boundary.  All refused on the host before any launch.  No atomics; one writer
 *   per slot. */
#define MMT_SEARCH_MAX_C 1024
int mmt_search_expert_parts(const float* qf, const float* qw, const void* g, const float* gw, const float* gscale,
                            int storage, int NV, int M, int d, const int64_t* candidates, int R, int C, float* parts,
                            float* mix, void* stream);

/* Cell-probed search (search_cells.hip), additive: one entry over the descriptor and its size function, nothing that
 * exists changes, MmtSearchScan stays 21 fields / 128 bytes and mmt_abi_version() stays 6.  It serves search.py's `cells`,
 * `search_probed` and `search_cells`: the inverted file.  The stored items are partitioned into cells, every query row names
 * a few cells (its probes) and gets the k best items of their union -- for that row mmt_search_topk with the union as its
 * subset, bit for bit: the same K loop and score epilogue (tk_scan, tk_tile_scores), the same key, running top-k and merge.
 * mmt_search_topk_cells (no options; fp32, bf16, fp8): the cell tables and the call's work list come behind the descriptor.
 *   items int64 [n_items]: the item numbers cell after cell, a cell's items ascending; a value outside 0 .. NV - 1 is
 *     "none": checked on the device, never dereferenced.  The stored rows are read through it and are not moved.
 *   pair_row, pair_slot int32 [n_pairs]: the (row, probe) pairs the call keeps -- invalid, empty and repeated cells dropped --
 *     ordered by (cell, row): the query row of a pair, 0 .. NQ - 1, and its probe slot, 0 .. P - 1, unique within the row.
 *   work int32 [n_work][5] = (first pair, rows, first position in items, end position, piece): one block scores `rows`
 *     (1 .. 64) consecutive pairs of one cell against positions [first, end) of items, at most MMT_SEARCH_CELL_PIECE of
 *     them, piece (0 .. pieces - 1) numbering the cuts of a cell.  rows = 0 is "no work": n_work may be an upper bound
 *     known without waiting for the device, the entries past the real count zero.  An entry outside these ranges is
 *     dropped on the device.
 *   1 <= P <= MMT_SEARCH_MAX_PROBES, pieces >= 1, 1 <= k <= 128.  ws uint64 [mmt_topk_cells_workspace_keys(NQ, P, pieces,
 *     k)] = NQ * P * pieces * k: every (row, slot, piece) has a list of its own, zeroed by the entry, one writer each, and
 *     the merge launch of mmt_search_topk joins a row's P * pieces lists.  scores fp32 / index int64 [NQ][k]: the best k
 *     items of the row's probed cells in the search's order -- score descending, -0 tied with +0, equal scores by
 *     ascending item number, across cells as within them -- then (-inf, -1); every slot is written.
 * MMT_ERR_ARG: any part of the descriptor beyond its operands (subset, exclude, after, norm, sets), a null operand, table,
 *   workspace or output, n_items / n_work / n_pairs < 1, P, pieces or k out of range, P * pieces * k >= 2^31, and the common
 *   shape gates; MMT_ERR_ALIGN: q, q_lo or g off a 16-byte boundary.  All refused on the host before any launch.  No
 *   atomics; one writer per slot. */
#define MMT_SEARCH_MAX_PROBES 64
#define MMT_SEARCH_CELL_PIECE 2048
int64_t mmt_topk_cells_workspace_keys(int NQ, int P, int pieces, int k);
int mmt_search_topk_cells(const MmtSearchScan* scan, const int64_t* items, int n_items, const int32_t* work, int n_work,
                          const int32_t* pair_row, const int32_t* pair_slot, int n_pairs, int P, int pieces, int k,
                          uint64_t* ws, float* scores, int64_t* index, void* stream);

/* The k-means update over the stored items (search_kmeans.hip), additive: three entries, nothing that exists changes,
 * MmtSearchScan stays 21 fields / 128 bytes and mmt_abi_version() stays 6.  They serve search.py's `cell_sums`,
 * `cell_centroids` and `train_cells`.  With f_g the dequantised stored row of item g (fp32 as it is, bf16 widened, fp8 code
 * x the item's scale: exact), gw_g its weights and L a cell's slice of `items` (ascending, n = |L|):
 *   S[m] = sum_{g in L} f_g[m], w[m] = sum_{g in L} gw_g[m]; G_c[m] = S[m] / |S[m]|_2 (zero S[m]: a zero row), gw_c[m] = w[m] / n.
 * mmt_search_cell_sums (fp32, bf16, fp8): the partial sums of the pieces of the cells' lists.
 *   g, gw, gscale, storage, NV, M, d: the stored operand as in mmt_search_expert_parts (gscale exactly when fp8).
 *   items int64 [n_items]: the item numbers cell after cell; a value outside 0 .. NV - 1 contributes nothing: checked on
 *     the device, never dereferenced.
 *   work int32 [n_work][3] = (cell, first position in items, end position): one piece, at most MMT_SEARCH_SUM_PIECE
 *     consecutive positions of one cell.  end <= first, positions outside 0 .. n_items or a longer piece mean "no work"
 *     (a zero partial row): n_work may be an upper bound known without waiting for the device.
 *   ws fp32 [mmt_cell_sums_workspace_floats(n_work, M, d)] = n_work * M * (d + 1): [n_work][M d] partial rows, then
 *     [n_work][M] partial weights.  One block per (piece, slab of MMT_SEARCH_SUM_SLAB columns); a thread owns its columns
 *     and adds the piece's rows in ascending position, one rounded fp32 add each, from +0.  One writer per slot.
 * mmt_search_cell_centroids: one block per cell joins the partial rows piece_start[c] .. piece_start[c + 1] - 1 (int32
 *   [C + 1]) in ascending order from +0 into sums fp32 [C][M d] and wsums [C][M] (always written, zero for a cell without
 *   pieces); n = offsets[c + 1] - offsets[c] (int64 [C + 1]).  embds [C][M][d] / weights [C][M] fp32, both or neither, are
 *   in/out: the centroid of a cell with n > 0 is written, the rows of an empty cell are left as they are.  A cell whose
 *   piece range is not inside 0 .. n_work or whose offsets are not inside 0 .. n_items is treated as empty.
 * The order of every sum is a function of a row's position in its cell's list and of the column alone; two calls are
 * bit-identical.  MMT_ERR_ARG: a null operand, table, workspace or output (embds without weights), gscale on fp32 / bf16 or
 * none on fp8, NV / n_items / n_work / C < 1, M outside 1 .. 16, d not a multiple of 4 (bf16: 8, fp8: 16), M d >= 2^27;
 * MMT_ERR_ALIGN: g or ws off a 16-byte boundary.  All refused on the host before any launch.  No atomics, no scratch. */
#define MMT_SEARCH_SUM_PIECE 256
#define MMT_SEARCH_SUM_SLAB 1024
int64_t mmt_cell_sums_workspace_floats(int n_work, int M, int d);
int mmt_search_cell_sums(const void* g, const float* gw, const float* gscale, int storage, int NV, int M, int d,
                         const int64_t* items, int n_items, const int32_t* work, int n_work, float* ws, void* stream);
int mmt_search_cell_centroids(const float* ws, int n_work, const int32_t* piece_start, const int64_t* offsets, int n_items,
                              int C, int M, int d, float* sums, float* wsums, float* embds, float* weights, void* stream);

/* The exact k-means update (search_kmeans.hip), additive: four entries and a size function, nothing that exists changes,
 * MmtSearchScan stays 21 fields / 128 bytes and mmt_abi_version() stays 6.  They serve search.py's `sum_scale`,
 * `cell_sums_exact`, `cell_centroids(exact=True)` and `train_cells(exact=True)` on both index classes.
 * THE DEFINITION.  f_g[k] is the dequantised stored value of item g, column k, as above; gw_g[m] its weights; the index
 * holds num_items items.  bits B = 62 - ceil(log2(max(num_items, 2))) (the F of mmt_search_row_expsum).  exponent E = the
 * least integer with max |f_g[k]| <= 2^E over the stored rows (0 when all are zero; a maximum of exactly 1.0 gives 0, the
 * next float up 1); wexponent the same over |gw_g[m]|.  term(g, k) = rint(f_g[k] * 2^(B - E)), taken in fp64 where the
 * scaling is exact, rounded to nearest, ties to even, converted to int64; |term| <= 2^B and a cell has at most num_items
 * <= 2^(62 - B) members, so a sum stays within +-2^62; a value beyond 2^E (a stale or foreign scale) is clamped to +-2^B
 * and never wraps.  sums[c][k] = sum over the cell's members of term(g, k) as int64, wsums likewise with wexponent:
 * integer addition is associative, so they are functions of the cell's member SET -- not of the order of its list, the
 * pieces, or how the items are spread over several indexes that share (B, E, wexponent), whose tensors simply add.
 * Back to fp32: S = ldexp(float32(sum), E - B), float32(sum) being ONE int64 -> fp32 conversion, round to nearest even
 * (never through fp64: that rounds twice).  |S - sum f| <= n_c 2^(E - B - 1) + ulp32(S) / 2 per column.  The centroid is
 * mmt_search_cell_centroids' formula on these S and w, by the same device code: equal fp32 sums give equal centroid bits.
 * mmt_search_absmax (fp32, bf16, fp8): one pass over the stored rows and the weights; out fp32 [2][n_blocks]: the maxima
 *   of |f| and of |gw| of block b's grid-stride share at out[b] and out[n_blocks + b], every slot written, one writer per
 *   slot.  The caller joins them with a maximum (order-independent) and derives E and wexponent.  1 <= n_blocks <= 65535.
 * mmt_search_cell_sums_exact: the operands of mmt_search_cell_sums, the piece_start table of mmt_search_cell_centroids,
 *   bits in 1 .. 61 and exponent / wexponent in -MMT_SEARCH_SUM_MAX_EXPONENT .. MMT_SEARCH_SUM_MAX_EXPONENT -> sums int64
 *   [C][M d] and wsums int64 [C][M], always written, zero for a cell without pieces.  ws: int64
 *   [mmt_cell_sums_exact_workspace_bytes(n_work, M, d) / 8], [n_work][M d] partial rows then [n_work][M] partial weights.
 *   One block per (piece, column slab) with int64 accumulators in registers, then one block per cell joins its partial
 *   rows.  The device-side range checks are those of mmt_search_cell_sums.
 * mmt_search_cell_centroids_exact: sums int64 [C][M d] / wsums int64 [C][M] -- of one call, or the integer sum of several
 *   indexes' -- offsets int64 [C + 1] (n = offsets[c + 1] - offsets[c]; outside 0 .. n_items: an empty cell) and the
 *   scale -> fsums fp32 [C][M d], fwsums fp32 [C][M] (always written) and in/out embds / weights, both or neither, as
 *   mmt_search_cell_centroids: the rows of an empty cell are left as they are.  One block per cell.
 * MMT_ERR_ARG: what mmt_search_cell_sums / mmt_search_cell_centroids refuse, a null table or output, C < 1, bits or an
 *   exponent out of range, n_blocks out of range; MMT_ERR_ALIGN: g or ws off a 16-byte boundary.  All refused on the host
 *   before any launch.  No atomics, no scratch. */
#define MMT_SEARCH_SUM_MAX_EXPONENT 160
int mmt_search_absmax(const void* g, const float* gw, const float* gscale, int storage, int NV, int M, int d, float* out,
                      int n_blocks, void* stream);
int64_t mmt_cell_sums_exact_workspace_bytes(int n_work, int M, int d);
int mmt_search_cell_sums_exact(const void* g, const float* gw, const float* gscale, int storage, int NV, int M, int d,
                               const int64_t* items, int n_items, const int32_t* work, int n_work,
                               const int32_t* piece_start, int C, int bits, int exponent, int wexponent, int64_t* ws,
                               int64_t* sums, int64_t* wsums, void* stream);
int mmt_search_cell_centroids_exact(const int64_t* sums, const int64_t* wsums, const int64_t* offsets, int n_items, int C,
                                    int M, int d, int bits, int exponent, int wexponent, float* fsums, float* fwsums,
                                    float* embds, float* weights, void* stream);

/* Beside the scans.
 * mmt_search_subset_pack: mask [NV] bytes (nonzero = allowed) -> the subset words, padding included: one ballot per 64
 *   items, one writer per word.
 * mmt_search_after_keys: cursor paging -- "the k best items that come AFTER a given position in the search's order", page 2
 *   of a result list, and through it sorted lists deeper than k = 128.  The order is the order of the uint64 keys of the
 *   scans, so a position is one key: 2^64 - 1 = no cursor (no score gives that key); 0 = exhausted (no candidate);
 *   key(a, first) + 1 = every item scoring below a, and at score a the items numbered first or higher.  first is the
 *   lowest item number still admitted at the cursor's score: a_item + 1 on one index, and on a shard the count of its
 *   items numbered <= a_item, which may be 0 or the shard's item count -- so the shards' lists merge exactly.  scores fp32
 *   [NQ] (non-NaN), first int64 [NQ] -> keys uint64 [NQ]; first < 0 selects a sentinel by the sign of the (then infinite)
 *   score: + no cursor, - exhausted.  0 <= first < 2^31 otherwise.  MMT_ERR_ARG for a null pointer or NQ < 1.  With norm
 *   the keys compared are those of score'.  A block whose 64 rows are all exhausted scores nothing.
 * mmt_search_merge_lists (search_shard.hip; one gallery cut into shards, each an index with item numbers of its own:
 *   search.py ShardedVideoIndex): per query, S lists of kin (score, shard-local item) pairs -- scores fp32 / index int64
 *   [S][NQ][kin], index -1 = empty slot -- and ids, a device array of S device pointers, ids[s] the int64 local -> global
 *   item table of shard s -> the best kout of them as scores fp32 / index int64 (global) [NQ][kout] in the search's order
 *   by GLOBAL item, slots without a candidate (-inf, -1).  Each list must be best-first with its empty slots last (true
 *   of a shard whose table is increasing).  1 <= S <= 32, 1 <= kin, kout <= 128 (kout may exceed S * kin), else
 *   MMT_ERR_ARG.  A returned score has the bits of the input score.  One block per query, the lists as keys in LDS, rank
 *   by binary search.  Every pointer, the S tables behind ids included, is memory of the device the kernel is launched
 *   on.  Trusted, not checked: every index value is -1 or below the length of its list's table, and every global item
 *   number is below 2^31 (the key holds it as int).
 * mmt_search_merge_group_lists: per query, S lists of kin (score, group, shard-local item) triples -- scores fp32, groups
 *   int64, index int64 [S][NQ][kin], index -1 = empty slot, each list best-first with distinct groups and its empty slots
 *   last -- and ids as above -> the best kout distinct groups over all lists as out_scores fp32 / out_groups int64 /
 *   out_items int64 (global) [NQ][kout], equal scores by ascending GLOBAL item, then (-inf, -1, -1).  Limits, pointers
 *   and trust as mmt_search_merge_lists; a group id is below 2^31. */
int mmt_search_subset_pack(const uint8_t* mask, int NV, uint32_t* words, void* stream);
int mmt_search_after_keys(const float* scores, const int64_t* first, int NQ, uint64_t* keys, void* stream);
int mmt_search_merge_lists(const float* scores, const int64_t* index, const int64_t* const* ids, int S, int NQ, int kin,
                           int kout, float* out_scores, int64_t* out_index, void* stream);
int mmt_search_merge_group_lists(const float* scores, const int64_t* groups, const int64_t* index, const int64_t* const* ids,
                                 int S, int NQ, int kin, int kout, float* out_scores, int64_t* out_groups, int64_t* out_items,
                                 void* stream);

/* ---- row-sharded similarity + max-margin loss for very large global batches (largesim.hip) --------------------
 * BASELINE.json configs[4] / SURVEY.md 8e: rank r owns the text rows r0..r0+b of the n x n similarity; same maths as
 * model.py:789-837 + loss.py:38-65 without the [n,n,M] weight tensor or the 2n^2 index vectors.  The two big GEMMs
 * (S = T'V'^T, P = G'V', Q = G'^T T') run on mmt_gemm_nt_bf16 / mmt_wgrad_grouped; these are the passes in between
 * (host orchestration: mmt_amd/large_sim.py).
 *   mmt_ls_fold_bf16: out16[r, m*d+c] = bf16(w[r,m] x[r,m,c]), rows R..Rpad zero.
 *   mmt_ls_finish   : S[t,v] /= sum_m tw[t,m] vw[v,m] (0 -> 1e-5), in place.
 *   mmt_ls_diag     : diag_local[t] = S[t, r0+t] / den from the RAW numerators (before the division below).
 *   mmt_ls_counts_ex: rowcnt[t] +=, colcnt[c] += (both zeroed by the caller), un-normalised hinge sums per column block
 *                     loss_part[t, cb], cb < mmt_ls_col_blocks(n); finish = 1 also divides the raw numerators (one sweep);
 *                     finish = 2 divides on the fly and leaves S raw (mmt_ls_grad_ex(raw = 1) divides again: the row block
 *                     is never rewritten).
 *   mmt_ls_counts   : the same with finish = 0.
 *   mmt_ls_grad     : G16[t,v] = bf16((dL/dS)/den) from the global counts; gs_part[t,cb,m] = sum over column block cb of
 *                     G' S vw[v,m].  mmt_ls_grad_ex: raw = 1 when S still holds the raw numerators.
 *   vw_t (nullable, mmt_ls_counts_ex / mmt_ls_grad_ex): vw transposed to [M, n] -- coalesced 16-byte loads in the sweeps.
 * n, ld, ldg multiples of 4.
 *   mmt_ls_unfold   : dx[r,m,:] = w[r,m] P[r,m*d:], dw[r,m] = <x[r,m], P[r,m]> - gsub[r,m]. */
int mmt_ls_fold_bf16(const float* x, const float* w, int R, int Rpad, int M, int d, void* out16, void* stream);
/* dst[c, r] = src[r, c], bf16, rows and cols multiples of 128 (ld in elements, multiples of 8): K-contiguous operands for the
 * NT GEMMs of the backward (V'^T, G'^T, T'^T). */
int mmt_transpose_bf16(const void* src, int64_t ld_src, int rows, int cols, void* dst, int64_t ld_dst, void* stream);
int mmt_ls_finish(float* S, int64_t ld, const float* tw, const float* vw, int b, int n, int M, void* stream);
int mmt_ls_col_blocks(int n);
int mmt_ls_diag(const float* S, int64_t ld, const float* tw, const float* vw, int b, int n, int M, int r0, float* diag_local,
                void* stream);
int mmt_ls_counts_ex(float* S, int64_t ld, const float* diag, const float* tw, const float* vw, const float* vw_t, int M, int finish, int b, int n,
                     int r0, float margin, int32_t* rowcnt, int32_t* colcnt, float* loss_part, void* stream);
int mmt_ls_counts(const float* S, int64_t ld, const float* diag, int b, int n, int r0, float margin, int32_t* rowcnt,
                  int32_t* colcnt, float* loss_part, void* stream);
int mmt_ls_grad(const float* S, int64_t ld, const float* diag, const float* tw, const float* vw, const int32_t* rowcnt,
                const int32_t* colcnt_total, int b, int n, int M, int r0, float margin, float inv_norm, void* G16,
                int64_t ldg, float* gs_part, void* stream);
int mmt_ls_grad_ex(const float* S, int64_t ld, const float* diag, const float* tw, const float* vw, const float* vw_t, const int32_t* rowcnt,
                   const int32_t* colcnt_total, int b, int n, int M, int r0, float margin, float inv_norm, void* G16,
                   int64_t ldg, float* gs_part, int raw, void* stream);
int mmt_ls_unfold(const float* P, int64_t ldp, const float* x, const float* w, const float* gsub, int R, int M, int d,
                  float* dx, float* dw, void* stream);

/* ---- row-sharded InfoNCE over the same row block (largesim.hip; model/loss.py:68-81) ---------------------------------
 * loss = CE(z, diag) + CE(z^T, diag), z = scale * S (scale = 1 is the reference), with rank r owning rows r0..r0+b:
 *   loss = (1/n) sum_t (row_lse[t] + col_lse[r0+t] - 2 z[t, r0+t]),  dL/dS = scale/n (exp(z - row_lse[t]) + exp(z - col_lse[v]) - 2 [v == r0+t]).
 * Both passes read the RAW numerators of the similarity GEMM and divide on the fly (S is never written); vw_t as above.
 *   mmt_ls_nce_stats: online-softmax partials, (max, sum of exp relative to that max), planar: plane 0 = max, plane 1 = sum.
 *                     row_part[2, b, ncb]   per local row and column block, ncb = mmt_ls_nce_col_blocks(n);
 *                     col_part[nrg, 2, n]   per column and group of rows,  nrg = mmt_ls_nce_row_groups(b), 16-byte aligned.
 *                     No atomics: the caller combines the partials in a fixed order (and the columns across ranks).
 *   mmt_ls_nce_grad : G16[t,v] = bf16((dL/dS)/den) and gs_part[t,cb,m] in the layout of mmt_ls_grad_ex (cb < mmt_ls_col_blocks(n))
 *                     from row_lse[b] and the GLOBAL col_lse[n] (16-byte aligned); inv_n = 1/n.
 * n, ld, ldg multiples of 4; r0 + b <= n; 1 <= M <= 16; scale finite and > 0. */
int mmt_ls_nce_col_blocks(int n);
int mmt_ls_nce_row_groups(int b);
int mmt_ls_nce_stats(const float* S, int64_t ld, const float* tw, const float* vw, const float* vw_t, int b, int n, int M, int r0,
                     float scale, float* row_part, float* col_part, void* stream);
int mmt_ls_nce_grad(const float* S, int64_t ld, const float* tw, const float* vw, const float* vw_t, const float* row_lse,
                    const float* col_lse, int b, int n, int M, int r0, float scale, float inv_n, void* G16, int64_t ldg,
                    float* gs_part, void* stream);

/* ---- text heads (texthead.hip), fp32 ------------------------------------------------------------------
 * GatedEmbeddingUnit per expert (model.py:683-702, 736-750) + text MoE weights (model.py:262-283,618),
 * batched over the M experts. */
typedef struct MmtSgemm {      /* C_b[i][j] = beta*C_b[i][j] + sum_k A_b[i*sai + k*sak] * B_b[j*sbj + k*sbk] + bias_b[j] */
  const float* A[MMT_MAX_EXPERTS];
  const float* B[MMT_MAX_EXPERTS];
  float* C[MMT_MAX_EXPERTS];
  const float* bias[MMT_MAX_EXPERTS];
  int64_t sai, sak, sbj, sbk, ldc;
  int32_t batch, M, N, K;
  float beta;
  int32_t reserved;
} MmtSgemm;
int mmt_sgemm_batched(const MmtSgemm* g, void* stream);

typedef struct MmtTextHeads {
  const float *w1[MMT_MAX_EXPERTS], *b1[MMT_MAX_EXPERTS];            /* text_GU.<mod>.fc      [d,K],[d]   */
  const float *w2[MMT_MAX_EXPERTS], *b2[MMT_MAX_EXPERTS];            /* text_GU.<mod>.cg.fc   [d,d],[d]   */
  const float *bn_gamma[MMT_MAX_EXPERTS], *bn_beta[MMT_MAX_EXPERTS]; /* cg.batch_norm weight/bias         */
  float *running_mean[MMT_MAX_EXPERTS], *running_var[MMT_MAX_EXPERTS];
  const float *moe_w[MMT_MAX_EXPERTS], *moe_b[MMT_MAX_EXPERTS];      /* moe_fc_txt.<mod>      [1,K],[1]   */
  float *g_w1[MMT_MAX_EXPERTS], *g_b1[MMT_MAX_EXPERTS], *g_w2[MMT_MAX_EXPERTS], *g_b2[MMT_MAX_EXPERTS];
  float *g_bn_gamma[MMT_MAX_EXPERTS], *g_bn_beta[MMT_MAX_EXPERTS], *g_moe_w[MMT_MAX_EXPERTS], *g_moe_b[MMT_MAX_EXPERTS];
} MmtTextHeads;
int64_t mmt_text_heads_workspace_floats(int N, int M, int d);
/* Optional extras of the small-batch path (mmt_text_heads_fast() != 0: N <= 32 caption rows, every training
 * configuration of the reference), all nullable / zero:
 *   moe_drop_*: nn.Dropout in front of the MoE logits (model.py:274) applied on the fly by the kernels that read the
 *     text (pass text_moe = NULL): stream key = hash(moe_drop_key, *seed_dev) at forward time, stored in *key_dev and
 *     re-read from there by the backward (which runs after the seed has moved on);
 *   num_batches_tracked: int64 [M], += 1 per training forward with use_bn (BatchNorm1d bookkeeping, on the device). */
/* The video side's token plan (+ feature cast) riding along as extra blocks of the text heads' first two launches
 * (N <= 32 caption rows, mmt_text_heads_fast): the arguments of mmt_video_plan / mmt_video_cast, which the caller then
 * does NOT call for this forward.  Two dependent launches (13 + 7 us under graph replay) leave the step; results are
 * those of the separate launches bit for bit (the dropout-seed bump moves from the plan to the second launch, i.e. it
 * still follows the text heads' read of the seed and precedes the encoder's). */
typedef struct MmtVideoFront {
  const MmtExpertIO* experts;
  int32_t M, B, T, pack, max_pos, do_cast;  /* do_cast = 0: the features arrive as bf16 (RaggedFeatures) */
  int32_t *counts, *cu_seqlens, *n_rows_dev, *slot, *row_index, *type_ids, *pos_ids;
  float* mask_bias;
  int32_t* agg_row;
  uint32_t* seed_bump;
  const MmtVideoSrc* src;
} MmtVideoFront;
typedef struct MmtTextHeadsOpts {
  uint32_t moe_drop_key, moe_drop_thr16;
  float moe_drop_scale;
  int32_t reserved;
  const uint32_t* seed_dev;
  uint32_t* key_dev;
  int64_t* num_batches_tracked;
  const MmtVideoFront* video_front;  /* nullable; forward only, small path only (MMT_ERR_ARG otherwise) */
} MmtTextHeadsOpts;
int mmt_text_heads_fast(int N, int M, int d, int K);
/* text [N = B*C, K] -> text_embds (B, M, C, d) L2-normalised, text_weights (B, C, M) (NULL: txt_wgh='none').
 * use_bn: txt_pro 'gbn' (1) / 'gem' (0).  training: batch statistics + running-stat update.
 * text_moe (nullable): the copy of text the MoE branch reads (after moe_txt_dropout, model.py:274). */
int mmt_text_heads_fwd(const MmtTextHeads* h, const float* text, const float* text_moe, int N, int C, int M, int d,
                       int K, int use_bn, int training, float* ws, float* text_embds, float* text_weights,
                       const MmtTextHeadsOpts* opts, void* stream);
/* gradients are WRITTEN through the g_* pointers; dtext [N, K] (nullable) receives the gradient for the text
 * tower; w1_all = the M fc.weight matrices contiguous as [M*d, K].  dtext_moe [N, K] (nullable): gradient wrt the MoE
 * branch's input (with the on-the-fly dropout: already masked, i.e. the gradient wrt text through that branch); without
 * it that gradient is added into dtext.  Every g_* pointer is nullable on its own, per expert and per parameter (a frozen
 * parameter): a null one is skipped, on both kernel paths, and every other gradient is what it is with all of them set. */
int mmt_text_heads_bwd(const MmtTextHeads* h, const float* text, const float* text_moe, const float* w1_all, int N,
                       int C, int M, int d, int K, int use_bn, int training, float* ws, const float* dtext_embds,
                       const float* text_weights, const float* dtext_weights, float* dtext, float* dtext_moe,
                       const MmtTextHeadsOpts* opts, void* stream);

/* ---- whole-encoder engine (bert_engine.hip) --------------------------------------------------------
 * One call runs every kernel of model/bert.py BertModel.forward (bert.py:371-414, without the unused
 * pooler) resp. its autograd backward on `stream`.  Pointers in MmtBertLayer/MmtBertModel address the
 * caller's flat parameter / shadow / gradient buffers (mmt_amd/flat.py); `ws` is a caller-allocated
 * workspace of mmt_bert_workspace_bytes() that carries the saved activations from forward to backward. */
typedef struct MmtBertLayer {
  const void *wqkv, *wqkv_t, *wo, *wo_t, *w1, *w1_t, *w2, *w2_t;              /* bf16 shadows            */
  const float *bqkv, *bo, *ln1_g, *ln1_b, *b1, *b2, *ln2_g, *ln2_b;           /* fp32 master             */
  float *g_wqkv, *g_bqkv, *g_wo, *g_bo, *g_ln1_g, *g_ln1_b, *g_w1, *g_b1, *g_w2, *g_b2, *g_ln2_g, *g_ln2_b;
} MmtBertLayer;

typedef struct MmtBertModel {
  int32_t hidden, layers, heads, inter, max_pos, type_vocab;
  float ln_eps, p_hidden, p_attn;
  int32_t reserved;
  const float *pos_emb, *type_emb, *emb_ln_g, *emb_ln_b;
  float *g_pos_emb, *g_type_emb, *g_emb_ln_g, *g_emb_ln_b;
  const MmtBertLayer* layer; /* host array [layers] */
} MmtBertModel;

typedef struct MmtBertBatch {
  const float* features;      /* [rows_alloc, hidden] fp32 token features (bert.py:98 `features`)        */
  const int32_t* type_ids;    /* [rows] token_type_ids                                                  */
  const int32_t* pos_ids;     /* [rows] position_ids, NULL for pos_enc='none'                           */
  const float* mask_bias;     /* [rows] (1 - attention_mask) * -10000   (bert.py:386-395)               */
  const int32_t* cu_seqlens;  /* [batch+1] or NULL (dense: sample b owns rows b*seq..)                  */
  const int32_t* row_index;   /* [rows] row -> b*seq+s (RNG coordinates) or NULL (identity)             */
  const int32_t* n_rows_dev;  /* live row count on device or NULL (= rows)                              */
  const uint32_t* seed_dev;   /* per-step dropout seed on device or NULL                                */
  int32_t rows, rows_alloc, batch, seq;
  /* Optional: the only rows of sequence_output the caller will read (CENet: the AGG token of every expert,
   * model.py:583-587), out_rows[b*n_out_per_sample + i], each sample's in ascending order.  The last layer then runs
   * everything after the K/V projection on those rows only (exact: all of it is row-wise) and returns them COMPACT:
   * out_last[i] = sequence_output[out_rows[i]] for i < batch * n_out_per_sample; `dlast` is read the same way.  The
   * compact mode is taken iff batch * n_out_per_sample <= mmt_bert_tail_capacity(rows_alloc).  NULL = every row. */
  const int32_t* out_rows;
  int32_t n_out_per_sample;
  /* MMT_FORK_* bits: which launches of the BACKWARD leave `stream` for `side_stream` (they are off the critical
   * path of the step: nothing on `stream` reads what they write until the optimizer does).  0 = everything on `stream`. */
  int32_t fork;
  /* second hipStream_t of the caller (nullable = no forking).  The engine orders the two streams with events
   * (mmt_stream_fork), which become graph edges under stream capture: the forked kernels then sit on a parallel branch
   * of the captured step.  Without MMT_FORK_JOIN the work on `side_stream` is still pending when the call returns: the
   * caller joins (mmt_stream_fork(side_stream, stream)) before anything on `stream` consumes a parameter gradient.
   * Under stream CAPTURE, MMT_FORK_WGRAD without MMT_FORK_JOIN is only valid when all layer ranges of one backward are
   * captured into the SAME graph: the "weight gradients of layer l + 2 are done" events a range waits for must have been
   * recorded in the capture that waits (ranges captured as separate graphs pass MMT_FORK_JOIN on every call). */
  void* side_stream;
  /* r06: the live row count as the HOST knows it (the collator counts valid tokens before the upload), 0 = unknown.  Only
   * the tile choice reads it (the kernels read n_rows_dev); without it a packed batch is priced at rows (every tile live). */
  int32_t live_rows_hint;
} MmtBertBatch;

enum {
  MMT_FORK_WGRAD = 1,   /* the grouped weight-gradient launch of every layer (trainer/trainer.py:203: autograd's
                         * mm-backward nodes for the weights, which nothing in the remaining backward depends on)  */
  MMT_FORK_EARLY = 2,   /* ... cut in two launches issued as soon as their operands exist (FFN pair after the
                         * dGELU GEMM, attention pair after the attention backward)                               */
  MMT_FORK_REDUCE = 4,  /* LayerNorm gamma/beta and embedding-table reductions                                    */
  MMT_FORK_JOIN = 8,    /* `stream` waits for `side_stream` before mmt_bert_backward_range returns                */
  /* not a fork bit, same field: a range that ends at layer 0 stops BEFORE the embedding stage (layer 0's parameter
   * gradients are final then: a data-parallel caller starts their reduction); the embedding stage follows as its own
   * call with l_hi = l_lo = -1 */
  MMT_RANGE_LAYERS_ONLY = 16
};

/* `to` waits for everything enqueued on `from` so far (hipEventRecord + hipStreamWaitEvent on an event of an internal
 * ring).  Under stream capture this is the fork (main -> side) resp. join (side -> main) edge of the captured graph. */
int mmt_stream_fork(void* from, void* to);

int64_t mmt_bert_workspace_bytes(const MmtBertModel* m, int rows_alloc);
int mmt_bert_tail_capacity(int rows_alloc);
/* out_last: fp32 [rows_alloc, hidden] last-layer hidden states (sequence_output).  training != 0 enables
 * dropout with p_hidden / p_attn. */
int mmt_bert_forward(const MmtBertModel* m, const MmtBertBatch* b, void* ws, float* out_last, int training,
                     void* stream);
/* dlast: fp32 [rows_alloc, hidden] gradient of sequence_output (overwritten as scratch);
 * dfeatures: fp32 [rows_alloc, hidden] gradient wrt `features`; parameter gradients are WRITTEN (not
 * accumulated) through the g_* pointers. */
int mmt_bert_backward(const MmtBertModel* m, const MmtBertBatch* b, void* ws, float* dlast, float* dfeatures,
                      int training, void* stream);
/* The same backward, layers l_hi .. l_lo only (descending; the embedding stage runs with layer 0), so that a
 * data-parallel caller can start the all-reduce of a finished layer's gradients while the layers below still run
 * (the reference's DataParallel reduces after the whole backward, trainer/trainer.py:185-199).  Calls must cover
 * layers-1 .. 0 in descending order with the same dlast / dfeatures / ws.  l_hi = l_lo = -1: the embedding stage alone
 * (see MMT_RANGE_LAYERS_ONLY). */
int mmt_bert_backward_range(const MmtBertModel* m, const MmtBertBatch* b, void* ws, float* dlast, float* dfeatures,
                            int training, int l_hi, int l_lo, void* stream);

/* Measurement hook (bench.py): arm n pairs of caller-created hipEvent_t; each mmt_bert_forward then
 * records one pair around layer 0's FFN up-projection GEMM launch (the dominant kernel) on its stream.
 * The arrays must stay alive until the events have been read.  Pass NULL/0 to disarm. */
int mmt_probe_arm(void** start_events, void** stop_events, int n);
/* the same per site: 0 = FFN up-projection GEMM, 1 = FFN down-projection GEMM, 2 = grouped weight gradients, 3 / 4 = attention
 * forward / backward (all of layer 0) */
int mmt_probe_arm_site(int site, void** start_events, void** stop_events, int n);
int mmt_probe_count_site(int site);
/* y = dropout(x) (n % 4 == 0, 16-byte aligned) with the counter-based RNG of the engine: nn.Dropout in front of the text
 * MoE logits (model/model.py:274).  Forward: key = hash(drop_key, *seed_dev), stored to key_save (nullable); backward:
 * pass the saved key as key_load (the encoder advances the seed in between) and the gradient as x. */
int mmt_dropout_f32(const float* x, float* y, int64_t n, uint32_t drop_key, uint32_t thr16, float scale,
                    const uint32_t* seed_dev, uint32_t* key_save, const uint32_t* key_load, void* stream);
/* Measurement hook (tools/dispatch_lab.py): `blocks` workgroups of `threads` threads with `lds_bytes` of dynamic LDS, each
 * spinning for `spin` clock ticks -- the workgroup dispatch rate as a function of the workgroup's shape. */
int mmt_debug_dispatch_probe(int blocks, int threads, int lds_bytes, int spin, float* sink, void* stream);
int mmt_probe_count(void);

#ifdef __cplusplus
}
#endif
#endif /* MMT_HIP_H_ */
