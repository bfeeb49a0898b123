/*
 * lthm.h — C ABI of the MI355X (gfx950) LTHM training hot path.
 *
 * Every entry point takes plain device pointers, element counts and a
 * hipStream_t passed as `void*`; nothing in here depends on torch.  All buffers
 * are caller-allocated (the Python host layer uses the torch caching
 * allocator); the library owns no device memory.  Return value: 0 on success,
 * otherwise a hipError_t code (1 = hipErrorInvalidValue for bad arguments).
 * Launches are stream-ordered and never synchronise the host.
 *
 * dtype codes: LTHM_F32 = 0, LTHM_BF16 = 1.
 *
 * Each function cites the reference interface it replaces
 * (paths relative to the reference repository ranjanbalappa-nykaa/recommendations).
 */
#ifndef LTHM_H_
#define LTHM_H_

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LTHM_ABI_VERSION 44 /* bumped on any signature / struct layout change */

#define LTHM_F32 0
#define LTHM_BF16 1
#define LTHM_FP8_E4M3 2 /* OCP e4m3fn (gfx950), GEMM operands only */

/* KShift finalisation modes */
#define LTHM_KSHIFT_SCALE 0      /* x / sqrt(K)               commons/layers.py:170 */
#define LTHM_KSHIFT_NORMALIZE 1  /* F.normalize(x, 2, -1)     commons/layers.py:168 */
#define LTHM_KSHIFT_NONE 2       /* plain sum (FlatEmbedding, K = 1)               */

/* ------------------------------------------------------------------------- */
/* version / capability                                                      */
/* ------------------------------------------------------------------------- */
/* returns LTHM_ABI_VERSION of the built library */
int lthm_abi_version(void);
/* number of gfx950 devices visible (0 on a host without a GPU); never fails */
int lthm_device_count(void);

/* ------------------------------------------------------------------------- */
/* Embedding gather / pool — commons/layers.py                               */
/* ------------------------------------------------------------------------- */

/* KShiftEmbedding.get_row_idx for every (id, c), c = 0..K-1.
 * rows[i*K + c] = row of ids[i] for rotation c.  Replaces commons/layers.py:174-185. */
int lthm_kshift_rows(const int64_t* ids, int64_t n, int64_t P, int32_t K,
                     int64_t* rows, void* stream);

/* KShiftEmbedding.forward (commons/layers.py:152-172) fused: K row indices,
 * in-order fp32 sum of the K table rows, then x / sqrt(K) or F.normalize.
 * W: [P, D] (w_dtype), out: [n, D] (out_dtype), norms: optional [n] f32
 * (pre-normalisation L2 norm, needed by the normalize backward).
 * Row offset `row_base` is added to every row (table-batched storage). */
int lthm_kshift_fwd(const int64_t* ids, int64_t n, const void* W, int32_t w_dtype,
                    int64_t P, int64_t row_base, int32_t D, int32_t K, int32_t mode,
                    void* out, int32_t out_dtype, float* norms, void* stream);

/* Same as lthm_kshift_fwd for F features stored in one table-batched weight:
 * ids [n, F]; feature f uses rows [f*P, (f+1)*P) of W [F*P, D]; out [n, F, D]. */
int lthm_kshift_fwd_multi(const int64_t* ids, int64_t n, int32_t F, const void* W,
                          int32_t w_dtype, int64_t P, int32_t D, int32_t K, int32_t mode,
                          void* out, int32_t out_dtype, float* norms, void* stream);
/* lthm_kshift_fwd_multi writing item (b, f)'s row at out + b * out_ld + f * D (elements): the F x D
 * rows of a sample inside a wider row, e.g. the ranker's MLP input [dense | F tables], built without a
 * concatenation pass (round 6, ABI 42).  out_ld > F * D needs K = 1. */
int lthm_kshift_fwd_multi_ld(const int64_t* ids, int64_t n, int32_t F, const void* W, int32_t w_dtype, int64_t P,
                             int32_t D, int32_t K, int32_t mode, void* out, int32_t out_dtype, int64_t out_ld,
                             float* norms, void* stream);

/* Item-embedding artifact forward (embedding_module_gen.py:32-41 ModelWrapper, consumed
 * at encoder.py:25-29 via torch.jit.load): out[i] = KShift_K(ids[i]; W [P, D], mode)
 * * sigmoid(w2 . QuickGELU(W1 m + b1) + b2) with m = KShift_Km(ids[i]; Wm [Pm, Dm]) / sqrt(Km)
 * (the mask model: KShiftEmbedding(normalize_output=False) -> commons MLP with one
 * hidden layer, W1 [H1, Dm], b1 [H1], w2 [H1], b2 [1]; all f32).  Dm % 4 == 0, Dm <= 16,
 * H1 <= 256, Wm 16-B aligned; W f32 or bf16, out f32 or bf16 [n, D].  Forward only. */
int lthm_item_artifact_fwd(const int64_t* ids, int64_t n, const void* W, int32_t w_dtype, int64_t P, int32_t D,
                           int32_t K, int32_t mode, const float* Wm, int64_t Pm, int32_t Dm, int32_t Km,
                           const float* W1, const float* b1, int32_t H1, const float* w2, const float* b2, void* out,
                           int32_t out_dtype, void* stream);

/* Pool K rows of a gathered buffer W [R, D] given explicit row indices
 * rows [n, K] (< R): same in-order f32 sum and finalisation as lthm_kshift_fwd.
 * The row-sharded item table (C3) pools the rows its all_to_all exchange
 * returned with it, bit-identical to the unsharded gather. */
int lthm_gather_pool(const int64_t* rows, int64_t n, int32_t K, const void* W, int32_t w_dtype, int64_t R, int32_t D,
                     int32_t mode, void* out, int32_t out_dtype, float* norms, void* stream);
/* Backward of lthm_kshift_fwd(_multi) into a dense f32 gradient dW [F*P, D]
 * (accumulated, caller zeroes).  LDS-staged dedup: each workgroup sorts its
 * (row, id) pairs in LDS, reduces duplicate rows wave-segment-wise, and emits
 * one f32 add per unique row.  dY: [n, F, D] (dy_dtype); out/norms are the
 * forward's output and norms (only read for LTHM_KSHIFT_NORMALIZE).
 * F = 1 for the single-table form. */
int lthm_kshift_bwd_dense(const int64_t* ids, int64_t n, int32_t F, const void* dY,
                          int32_t dy_dtype, const void* out, int32_t out_dtype,
                          const float* norms, int64_t P, int32_t D, int32_t K,
                          int32_t mode, float* dW, void* stream);

/* Same, plus the touched-row list for the sparse row-wise optimizers: the first
 * add to a row sets flags[row] (int32 [F*P], caller keeps it zeroed; lthm_sparse_adamw /
 * lthm_sparse_adagrad re-zero the entries of the rows they update, or none with flags = NULL) and appends
 * the row to list (int64 [>= n*F*K]) at atomic index *count (int64, zeroed). */
int lthm_kshift_bwd_sparse(const int64_t* ids, int64_t n, int32_t F, const void* dY,
                           int32_t dy_dtype, const void* out, int32_t out_dtype,
                           const float* norms, int64_t P, int32_t D, int32_t K, int32_t mode,
                           float* dW, int32_t* flags, int64_t* list, int64_t* count, void* stream);
/* The K = 1, plain-output case of lthm_kshift_bwd_sparse (FlatEmbedding / table-batched flat
 * lookups, the C4 ranker: commons/layers.py:56-61's nn.Embedding backward) with the rows of
 * first touch STORED: the item that sets the row's bit writes its row of dW (no prior contents
 * needed: rows are stored, not accumulated), every other item of a touched row is added
 * afterwards with f32 atomics.  flags here is a BITMAP: bit (row & 31) of 32-bit word row >> 5,
 * [>= ceil(F * P / 32)] words, kept zeroed by the caller (the row-wise optimizer clears it whole
 * after its step).  dup_ws: int64 [>= n * F + 1] workspace.  Same dW / list / count result as
 * lthm_kshift_bwd_sparse with K = 1, mode LTHM_KSHIFT_SCALE, up to the f32 summation order of
 * duplicated rows. */
int lthm_kshift_bwd_sparse_first(const int64_t* ids, int64_t n, int32_t F, const void* dY, int32_t dy_dtype,
                                 int64_t P, int32_t D, float* dW, int32_t* flags, int64_t* list, int64_t* count,
                                 int64_t* dup_ws, int64_t dup_cap, void* stream);
/* lthm_kshift_bwd_sparse_first reading item (b, f)'s gradient row at dY + b * dy_ld + f * D
 * (the gradient of the strided lthm_kshift_fwd_multi_ld output, in place in the wider row). */
int lthm_kshift_bwd_sparse_first_ld(const int64_t* ids, int64_t n, int32_t F, const void* dY, int32_t dy_dtype,
                                    int64_t dy_ld, int64_t P, int32_t D, float* dW, int32_t* flags, int64_t* list,
                                    int64_t* count, int64_t* dup_ws, int64_t dup_cap, void* stream);

/* Fused dedup + row-wise Adagrad of a KShift table: lthm_kshift_bwd_sparse followed by
 * lthm_sparse_adagrad_ex in one call, with no gradient row stored.  For the item-embedding
 * generator, whose tables step right after their backward with torch.optim.Adagrad and nothing
 * in between (embedding_module_gen.py:137,151-153 and :97-99,113-115): the pairs (row, item) of
 * every (item, shift) are radix-sorted by row (stable, so a row's pairs stay in item order), each
 * row's gradient -- sum over its pairs of the item's pooled-sum gradient (dy / sqrt(K), dy, or the
 * F.normalize backward, as lthm_kshift_bwd_sparse) -- is summed in that order and the row updated
 * once, unfused f32:  s = s + g * g;  W = W - (clr * g) / (sqrt(s) + eps).  A row with more than
 * 256 pairs is summed in chunks of 256 pairs, the chunk sums in 16 contiguous groups, the group
 * sums in order (oracle/ref.py kshift_adagrad_ref restates the order).  Deterministic.
 * clr = lr / (1 + (step - 1) * lr_decay) (torch.optim.Adagrad; no weight decay).  ids / dY / out /
 * norms as lthm_kshift_bwd_sparse ([n, F] ids, item i of table i % F); W, state_sum [F * P, D] f32.
 * Requires F * P <= 2^32, n * F * K < 2^31, D <= 256, K <= 64; workspace 256-B aligned, >=
 * lthm_kshift_adagrad_ws_bytes(n * F, K, D) bytes (-1: invalid sizes). */
int64_t lthm_kshift_adagrad_ws_bytes(int64_t n_items, int32_t K, int32_t D);
int lthm_kshift_adagrad_fused(const int64_t* ids, int64_t n, int32_t F, const void* dY, int32_t dy_dtype,
                              const void* out, int32_t out_dtype, const float* norms, int64_t P, int32_t D, int32_t K,
                              int32_t mode, float* W, float* state_sum, float clr, float eps, void* workspace,
                              int64_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------- */
/* GEMM: every nn.Linear on the path (commons/transformers/layers.py:240-241,   */
/* :274-276; commons/layers.py:65-81; models/lthm/sequence/ Linears)          */
/* ------------------------------------------------------------------------- */
#define LTHM_ACT_NONE 0
#define LTHM_ACT_GELU 1        /* nn.GELU(approximate='tanh')  transformers/layers.py:275 */
#define LTHM_ACT_QGELU 2       /* QuickGELU x*sigmoid(1.702x)   commons/layers.py:9-11    */
#define LTHM_ACT_GELU_GRAD 3   /* multiply by GELU'(aux)   (backward epilogue)            */
#define LTHM_ACT_QGELU_GRAD 4  /* multiply by QuickGELU'(aux)                             */
#define LTHM_ACT_GELU_D 5      /* GELU, but aux_out receives GELU'(x) (bf16), not x      */
#define LTHM_ACT_MUL_AUX 6     /* multiply by aux (a derivative saved by LTHM_ACT_GELU_D) */

/* C[b] = epi(alpha * A[b] . B[b]), bf16 operands, fp32 accumulation (MFMA).
 *   a_kcontig: A is [M][K] (row stride lda) else A is [K][M] (row stride lda)
 *   b_kcontig: B is [N][K] (row stride ldb) else B is [K][N] (row stride ldb)
 * epilogue, in order: + bias[N]; act (GELU/QGELU store the pre-activation to
 * aux_out, *_GRAD multiply by act'(aux)); + res1; + res2; cast to out_dtype.
 * splits > 1: split-K over `workspace` (splits*batch*M*N f32), then combine. */
typedef struct lthm_gemm_desc {
  const void* A;
  const void* B;
  void* C;
  int64_t M;
  int64_t N;
  int64_t K;
  int64_t lda;
  int64_t ldb;
  int64_t ldc;
  int64_t sA;
  int64_t sB;
  int64_t sC;
  int32_t batch;
  int32_t a_kcontig;
  int32_t b_kcontig;
  int32_t out_dtype;
  float alpha;
  int32_t act;
  const float* bias;
  const void* aux;
  void* aux_out;
  int64_t ldaux;
  const void* res1;
  const void* res2;
  int64_t ldr1;
  int64_t ldr2;
  int32_t res1_dtype;
  int32_t res2_dtype;
  int32_t splits;
  int32_t pad0;
  float* workspace;
  size_t workspace_bytes;
  int32_t ab_dtype;
  int32_t pad1;
  const float* a_scale;
  const float* b_scale;
  int32_t* amax_out; /* optional: atomic max of |C| (as f32 bits) over the stored values */
} lthm_gemm_desc;

/* ab_dtype LTHM_BF16 (0 is read as bf16 too) or LTHM_FP8_E4M3: A [M, K] and B [N, K]
 * both K-contiguous e4m3 bytes (lda / ldb in bytes), per-tensor device scales
 * a_scale / b_scale (C = epi(alpha * a_scale * b_scale * A.B)); batch 1, no split-K,
 * K % 128 == 0 -- the fp8 encoder GEMMs of the C5 config, on
 * v_mfma_scale_f32_16x16x128_f8f6f4 with unit block scales. */
int lthm_gemm(const lthm_gemm_desc* desc, void* stream);

/* The launch plan of lthm_gemm: which kernel a descriptor runs on a device of `cus` compute
 * units, decided on the host from the descriptor's numbers and its pointers' low bits alone
 * (no GPU call, no device memory touched).  lthm_gemm launches from lthm_gemm_plan(desc,
 * the device's CU count); the return value is the one lthm_gemm gives the same descriptor
 * (1 for a refused one, the plan is then undefined). */
#define LTHM_GEMM_KERNEL_NONE (-1)  /* M == 0 or N == 0: nothing is launched */
#define LTHM_GEMM_KERNEL_K128 0     /* gemm_k<KA, KB>: 128 x 128 tiles, any shape / stride, batch, split-K */
#define LTHM_GEMM_KERNEL_PS 1       /* gemm_ps_k<KB, BRES, EPI>: persistent ring kernel, tall bf16 GEMMs */
#define LTHM_GEMM_KERNEL_WG 2       /* gemm_wg_k: 256 x 256 split-K tiles, both operands K-strided */
#define LTHM_GEMM_KERNEL_PP 3       /* gemm_pp_k<false, SPREAD>: 256 x 256 tiles, K-contiguous, K >= 512 */
#define LTHM_GEMM_KERNEL_PS_F8 4    /* gemm_ps_k<true, BRES, EPI, true>: fp8 operands */
#define LTHM_GEMM_KERNEL_PP_F8 5    /* gemm_pp_k<true, false>: fp8 operands, K >= 1,024 */
#define LTHM_GEMM_COMBINE_NONE 0
#define LTHM_GEMM_COMBINE_REDUCE 1   /* splitk_reduce_k  */
#define LTHM_GEMM_COMBINE_REDUCE4 2  /* splitk_reduce4_k */
#define LTHM_GEMM_AMAX_NONE 0
#define LTHM_GEMM_AMAX_KERNEL 1  /* the GEMM kernel's epilogue takes max |C| */
#define LTHM_GEMM_AMAX_AFTER 2   /* lthm_amax over C after the GEMM */
#define LTHM_GEMM_EPI_GENERIC (-1)  /* the runtime epilogue (every kernel but gemm_ps_k) */
#define LTHM_GEMM_EPI_PLAIN 0       /* (+ bias) */
#define LTHM_GEMM_EPI_ACT 1         /* (+ bias), GELU / QGELU / GELU_D, optional aux_out */
#define LTHM_GEMM_EPI_GRAD 2        /* * act'(aux) or * aux, no bias */
#define LTHM_GEMM_EPI_RES1 3        /* (+ bias) + res1 (f32) */
#define LTHM_GEMM_EPI_RES2 4        /* (+ bias) + res1 + res2 (f32) */
typedef struct lthm_gemm_plan_out {
  int32_t kernel;  /* LTHM_GEMM_KERNEL_* */
  int32_t ka;      /* template flags of the kernel (0 where it has no such flag) */
  int32_t kb;
  int32_t bres;
  int32_t epi;     /* LTHM_GEMM_EPI_*: the compiled form for PS / PS_F8, the form the epilogue fits elsewhere */
  int32_t spread;
  int32_t splits;   /* effective split count (1: no split-K) */
  int32_t combine;  /* LTHM_GEMM_COMBINE_* */
  int32_t amax;     /* LTHM_GEMM_AMAX_* */
  int32_t fast_ok;  /* 16-B aligned operands, leading dims and batch strides % 8 == 0 */
  int32_t grid_x;   /* the GEMM kernel's grid and block */
  int32_t grid_y;
  int32_t grid_z;
  int32_t block;
  int32_t tiles_m;  /* in the kernel's own tile (128 or 256 rows / columns) */
  int32_t tiles_n;
  int32_t walkers;  /* PS / PS_F8: row-panel walkers per column tile and XCD */
  int32_t ps_mode;  /* the read-once process settings the plan used: LTHM_GEMM_PS, */
  int32_t pp_mode;  /* LTHM_GEMM_PP, */
  int32_t pp_f8_mode;  /* LTHM_GEMM_PP_F8, */
  int32_t wg_ragged;   /* LTHM_WG_RAGGED */
  int32_t pad0;
  int64_t k_per_split;  /* k range of one split (K when splits == 1) */
} lthm_gemm_plan_out;
int lthm_gemm_plan(const lthm_gemm_desc* desc, int32_t cus, lthm_gemm_plan_out* plan);

/* Per-tensor fp8 quantisation: scale = amax(|x|) / 448 (1 if x == 0),
 * q = e4m3(clamp(x / scale, -448, 448)) round-to-nearest-even.  x: n f32 / bf16
 * (n % 8 == 0, 16-B aligned); q: n bytes; scale: device f32; work: 4-byte scratch. */
int lthm_quantize_fp8(const void* x, int32_t dtype, int64_t n, uint8_t* q, float* scale, int32_t* work,
                      void* stream);
/* The same quantisation with amax(|x|) already reduced by the producer (the f32 bits of
 * the maximum in *amax: lthm_layernorm_fwd_amax, lthm_gemm's amax_out, lthm_amax), so
 * x is read once: the C5 encoder's fused quantisation. */
int lthm_quantize_fp8_amax(const void* x, int32_t dtype, int64_t n, const int32_t* amax, uint8_t* q, float* scale,
                           void* stream);
/* *amax = max(*amax, amax(|x|)) as f32 bits (x: n f32 / bf16, n % 8 == 0, 16-B aligned);
 * the caller zeroes *amax before the first producer. */
int lthm_amax(const void* x, int32_t dtype, int64_t n, int32_t* amax, void* stream);

/* ------------------------------------------------------------------------- */
/* Fused encoder MLP: _MLP.forward, commons/transformers/layers.py:279-284      */
/* (c_fc -> GELU(tanh) -> c_proj, dropout 0) with the [M, HID] hidden kept on   */
/* chip.  x: ln_2 output bf16 [M, D]; W1 = c_fc.weight bf16 [HID, D];           */
/* W2T = c_proj.weight^T bf16 [HID, D]; biases f32 (NULL for bias=False).        */
/* Supported shapes: lthm_mlp_supported(D, HID) (D 128 or 256, HID % 32 == 0).  */
/* ------------------------------------------------------------------------- */
int lthm_mlp_supported(int32_t D, int32_t HID);
/* The launch geometry of one fused-MLP entry point on a device of `cus` compute units, decided
 * on the host from the numbers alone (no GPU call).  The six launchers and
 * lthm_mlp_wgrad_ws_bytes take their geometry from lthm_mlp_plan(entry, M, D, HID, the device's
 * CU count); the return value is nonzero (1) for a shape the entry refuses (the plan is then
 * undefined): D not 128 / 256, HID not a multiple of 32 in 32 .. 8192, M < 0, HID > 4096 for
 * BWD_HIDDEN and BWD_DX, HID % 128 != 0 for WGRAD, or static + dynamic LDS above the 160 KiB a
 * gfx950 workgroup can hold.  lthm_mlp_supported(D, HID) is true where the FWD and the BWD plan
 * both accept. */
#define LTHM_MLP_FWD 0         /* lthm_mlp_fwd:        mlp_fwd_k<D, 8>  */
#define LTHM_MLP_FWD_LN 1      /* lthm_mlp_fwd_ln:     mlp_fwd_k<D, 8>, ln_2 in the prologue */
#define LTHM_MLP_BWD 2         /* lthm_mlp_bwd:        mlp_bwd_k<D, 4, true> */
#define LTHM_MLP_BWD_HIDDEN 3  /* lthm_mlp_bwd_hidden: mlp_bwdp_k<D, 8> */
#define LTHM_MLP_BWD_DX 4      /* lthm_mlp_bwd_dx:     mlp_bwdx_k<D, 4> */
#define LTHM_MLP_WGRAD 5       /* lthm_mlp_wgrad:      mlp_wgrad_k<D, 4, FULL> + mlp_wgrad_fold_k */
#define LTHM_MLP_LDS_MAX 163840 /* bytes of LDS one gfx950 workgroup can hold */
typedef struct lthm_mlp_plan_out {
  int32_t waves;      /* waves per workgroup */
  int32_t tile_rows;  /* token rows per tile: 32 x waves; WGRAD: 32 (the staged token tile) */
  int32_t grid;       /* workgroups of the main kernel (0: M == 0, it is not launched) */
  int32_t max_tiles;  /* the most tiles one workgroup walks (WGRAD: token tiles of the longest slice) */
  int32_t nslice;     /* WGRAD: token slices (partial slabs), 0 elsewhere */
  int32_t ngroup;     /* WGRAD: hidden groups of 32 x waves units, 0 elsewhere */
  int32_t full;       /* WGRAD: 1 when M % 32 == 0 (mlp_wgrad_k<.., true>, no row mask) */
  int32_t pad0;
  int64_t ntiles;     /* tiles of tile_rows rows over all M */
  int64_t ws_bytes;   /* WGRAD: workspace bytes, 0 elsewhere */
  int64_t lds_static;   /* bytes of the kernel's __shared__ arrays */
  int64_t lds_dynamic;  /* bytes of dynamic LDS passed at the launch */
} lthm_mlp_plan_out;
int lthm_mlp_plan(int32_t entry, int64_t M, int32_t D, int32_t HID, int32_t cus, lthm_mlp_plan_out* plan);
/* out f32 [M, D] = res1 [+ res2] + c_proj(GELU(c_fc(x))); res1 / res2 f32 [M, D] or NULL
 * (replaces TransformerBlock's x + mlp(ln_2 x), commons/transformers/layers.py:371). */
int lthm_mlp_fwd(const void* x, int64_t M, int32_t D, int32_t HID, const void* W1, const float* b1,
                 const void* W2T, const float* b2, const float* res1, const float* res2, float* out,
                 void* stream);
/* lthm_mlp_fwd with ln_2 fused into the prologue: the input rows are LayerNorm(x) (x f32 [M, D],
 * ln_w / ln_b f32 [D], eps 1e-5, ln_b NULL for bias=False); h_out (bf16 [M, D]), mean and rstd
 * (f32 [M]) receive the LayerNorm output and statistics for the backward (each may be NULL).
 * Replaces the block's x + mlp(ln_2(x)) (commons/transformers/layers.py:371, :142-149). */
int lthm_mlp_fwd_ln(const float* x, const float* ln_w, const float* ln_b, int64_t M, int32_t D, int32_t HID,
                    const void* W1, const float* b1, const void* W2T, const float* b2, const float* res1,
                    const float* res2, float* out, void* h_out, float* mean, float* rstd, void* stream);
/* The training backward with the hidden RECOMPUTED (never stored by the forward):
 * pre = x W1^T + b1; G = GELU(pre); dP = (dY W2) * GELU'(pre); dX = dP W1.  dY bf16 [M, D]
 * (gradient of the MLP output), dX [M, D] in dx_dtype (LTHM_F32 / LTHM_BF16), G and dP bf16
 * [M, HID]: the operands of dW2 = dY^T G and dW1 = dP^T x (db1 = colsum dP), which the
 * weight-gradient GEMM computes.  Replaces the c_proj / c_fc dgrad pair of
 * commons/transformers/layers.py:279-284's backward. */
int lthm_mlp_bwd(const void* x, const void* dY, int64_t M, int32_t D, int32_t HID, const void* W1, const float* b1,
                 const void* W2T, void* dX, int32_t dx_dtype, void* G, void* dP, void* stream);
/* The same recompute without dX (G and dP only; two waves per SIMD): dX = dP W1 then runs on the
 * GEMM.  HID <= 4096. */
int lthm_mlp_bwd_hidden(const void* x, const void* dY, int64_t M, int32_t D, int32_t HID, const void* W1,
                        const float* b1, const void* W2T, void* G, void* dP, void* stream);
/* The training backward with NO [M, HID] operand in HBM (round 5): two recompute kernels.
 * lthm_mlp_bwd_dx: dX = ((dY W2) * GELU'(x W1^T + b1)) W1 alone (dX in dx_dtype). */
int lthm_mlp_bwd_dx(const void* x, const void* dY, int64_t M, int32_t D, int32_t HID, const void* W1,
                    const float* b1, const void* W2T, void* dX, int32_t dx_dtype, void* stream);
/* lthm_mlp_wgrad: dW1 = dP^T x (f32 [HID, D], c_fc.weight's gradient), dW2 = dY^T G (f32 [D, HID],
 * c_proj.weight's), db1 = colsum dP (f32 [HID], or NULL) with G / dP recomputed per token tile
 * inside the kernel; partial sums per token slice go to the workspace (>= lthm_mlp_wgrad_ws_bytes)
 * and are folded in slice order (deterministic).  HID % 128 == 0.  Replaces the c_fc / c_proj
 * weight-gradient products of commons/transformers/layers.py:279-284's backward. */
int64_t lthm_mlp_wgrad_ws_bytes(int64_t M, int32_t D, int32_t HID);
int lthm_mlp_wgrad(const void* x, const void* dY, int64_t M, int32_t D, int32_t HID, const void* W1,
                   const float* b1, const void* W2T, float* dW1, float* dW2, float* db1, void* workspace,
                   int64_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------- */
/* LayerNorm (commons/transformers/layers.py:142-149, eps 1e-5)               */
/* ------------------------------------------------------------------------- */
/* x f32 [M, D] -> y (y_dtype) [M, D], mean/rstd f32 [M]. b may be NULL (bias=False). */
int lthm_layernorm_fwd(const float* x, int64_t M, int32_t D, const float* w, const float* b,
                       void* y, int32_t y_dtype, float* mean, float* rstd, void* stream);
/* lthm_layernorm_fwd that also folds amax(|y|) (of the stored, rounded y) into *amax
 * (f32 bits, atomic max; the caller zeroes it): the fp8 quantisation's reduction. */
int lthm_layernorm_fwd_amax(const float* x, int64_t M, int32_t D, const float* w, const float* b, void* y,
                            int32_t y_dtype, float* mean, float* rstd, int32_t* amax, void* stream);
/* number of row blocks the backward uses (partials is [2, blocks, D] f32) */
int lthm_layernorm_bwd_blocks(int64_t M);
/* dx = LN'(dy) + res1 + res2 (f32; res may be NULL), optional bf16 copy of dx;
 * partials[0] = per-block dweight sums, partials[1] = per-block dbias sums. */
int lthm_layernorm_bwd(const void* dy, int32_t dy_dtype, const float* x, int64_t M, int32_t D,
                       const float* w, const float* mean, const float* rstd, const float* res1,
                       const float* res2, float* dx, void* dx_bf16, float* partials, void* stream);
/* flags bit 0 (D % 4 == 0): dx (f32) = LN'(dy) + 2 res1 + res2 while dx_bf16 = LN'(dy) + res1 + res2:
 * the double-residual block's ln_2 backward hands ln_1's backward its two residual gradients
 * as one f32 tensor (query_tower.py:135, x + block(x)) */
int lthm_layernorm_bwd_ex(const void* dy, int32_t dy_dtype, const float* x, int64_t M, int32_t D,
                          const float* w, const float* mean, const float* rstd, const float* res1,
                          const float* res2, float* dx, void* dx_bf16, float* partials, int32_t flags, void* stream);
/* The input-gradient GEMM that feeds a LayerNorm backward, fused with it (round 5): dh = dy W
 * (dy [M, K] bf16, wt = W^T [256, K] bf16, K % 64 == 0: the block's c_fc / c_attn dgrad,
 * commons/transformers/layers.py:271-284 and :247-265) and then lthm_layernorm_bwd_ex over
 * dh in f32 (layers.py:142-149): dx = LN'(dh) + res1 + res2 (+ res1 again with flags bit 0),
 * its bf16 copy (dx_bf16 may be null), and per-tile weight / bias gradient partials
 * (partials: f32 [2, lthm_dgrad_layernorm_bwd_tiles(M), 256], rows summed by the caller).
 * D must be 256 (one column tile holds whole rows); 16-B aligned operands. */
int lthm_dgrad_layernorm_bwd_tiles(int64_t M);
/* The block's c_proj forward and ln_2 in one kernel (round 5): x1 = res1 + x W^T + bias
 * (x [M, K] bf16, W [256, K] bf16 = nn.Linear weight, K % 64 == 0; transformers/layers.py:
 * 264 + the residual of :371) written in f32, then lthm_layernorm_fwd of x1 (layers.py:142-149,
 * eps 1e-5): h bf16 [M, 256], mean / rstd [M].  bias / res1 / ln_b may be null. */
int lthm_linear_layernorm_fwd(const void* x, const void* w, const float* bias, const float* res1, int64_t M,
                              int32_t D, int64_t K, const float* ln_w, const float* ln_b, float* x1,
                              void* h, float* mean, float* rstd, void* stream);
int lthm_dgrad_layernorm_bwd(const void* dy, const void* wt, int64_t M, int32_t D, int64_t K,
                             const float* x, const float* w, const float* mean, const float* rstd,
                             const float* res1, const float* res2, float* dx, void* dx_bf16,
                             float* partials, int32_t flags, void* stream);

/* ------------------------------------------------------------------------- */
/* Attention with relative position bias + causal mask                       */
/* (commons/transformers/layers.py:13-61, :202-265)                          */
/* ------------------------------------------------------------------------- */
typedef struct lthm_attn_desc {
  const void* q;
  const void* k;
  const void* v;
  int64_t q_tok_stride;
  int64_t k_tok_stride;
  int64_t v_tok_stride;
  int64_t q_head_stride;
  int64_t k_head_stride;
  int64_t v_head_stride;
  int64_t q_batch_stride;
  int64_t k_batch_stride;
  int64_t v_batch_stride;
  void* out;
  int64_t o_tok_stride;
  int64_t o_head_stride;
  int64_t o_batch_stride;
  const float* table;
  int64_t table_rows;
  float* lse;
  int32_t B;
  int32_t T;
  int32_t H;
  int32_t E;
  int32_t causal;
  int32_t pad0;
  const void* dout;
  void* dq;
  void* dk;
  void* dv;
  float* dtable_part;
  float* delta;
  const float* mask;          /* optional additive mask, f32 [., ., T, T] (NULL: none) */
  int64_t mask_batch_stride;  /* 0 broadcasts one mask over the batch */
  int64_t mask_head_stride;   /* 0 broadcasts over the heads */
  int64_t mask_row_stride;    /* >= T */
  /* packed rows (shared pad prefix, lthm_pad_prefix_*; T > 256, E = 64, no mask): when row_map
   * is set the batch strides are unused and row t of sequence b is row row_map[b * T + t] of
   * q / k / v (and of out / dout / dq through live_map, -1 = not this sequence's row: its dout
   * reads as zero, its out / dq are not written, and query tiles with no live row are skipped).
   * dK / dV of a key in the chain (row < chain_rows) go to dk_chain / dv_chain row
   * b * chain_rows + t (token stride chain_ts, head stride = k / v head stride), the others to
   * dk / dv at their packed row. */
  const int32_t* row_map;
  const int32_t* live_map;
  void* dk_chain;
  void* dv_chain;
  int64_t chain_ts;
  int32_t chain_rows;
  int32_t pad1;
} lthm_attn_desc;

/* bf16 q/k/v/out, f32 table [table_rows, H] (row q-k+T), lse f32 [B, H, T].
 * T <= 256: one workgroup per (batch, head) holds K and V whole in LDS.
 * 256 < T <= 4096 (E = 32/64/128): 64-row workgroups stream K/V windows.
 * mask != NULL: S[b, h, q, k] += mask[b * mask_batch_stride + h * mask_head_stride
 * + q * mask_row_stride + k] (the reference's general additive attn_mask, SDPA :57-58,
 * TransformerBlock.inner_forward :404-408, on top of the causal flag); served by the
 * whole-head VALU kernels, so T <= 256 and K, V, Q, dO of one head fit in LDS
 * (lthm_attn_mask_ok: T <= 149 at E = 128). */
int lthm_attn_fwd(const lthm_attn_desc* desc, void* stream);
/* dq/dk/dv bf16 (same strides as q/k/v); dtable_part f32 [parts, 2T+1, H] with
 * parts = lthm_attn_bwd_parts(B, T) (reduce over the first dim; = B for T <= 256);
 * delta: f32 [B, H, T] workspace, required when T > 256. */
int lthm_attn_bwd(const lthm_attn_desc* desc, void* stream);
int64_t lthm_attn_bwd_parts(int32_t B, int32_t T);
/* 1 when lthm_attn_fwd / lthm_attn_bwd take PACKED rows (row_map set) at this T and E with no
 * mask: the long-T' 32x32x16 kernels serve it (T > 256, E = 64, both LDS images fit, not
 * switched off by the A/B environment switches); 0: the caller unpacks to full sequences. */
int lthm_attn_packed_ok(int32_t T, int32_t E);
/* 1 when lthm_attn_fwd AND lthm_attn_bwd take a general additive mask at this T and E: the
 * whole-head VALU kernels keep K, V, Q and dO of one head in LDS, T (8 E + 72) + 16 bytes of the
 * 160 KiB in the backward, so T <= 256 for E = 16 / 32 / 64 and T <= 149 for E = 128. */
int lthm_attn_mask_ok(int32_t T, int32_t E);

/* ------------------------------------------------------------------------- */
/* LTHM towers (models/lthm/sequence/ encoder, product and query towers)     */
/* ------------------------------------------------------------------------- */
#define LTHM_MAX_CVE 8

/* history flip, right padding -> left padding (encoder.py:52-54, 60-61) */
int lthm_flip_tokens(const int64_t* in, int64_t* out, int64_t B, int32_t T, void* stream);

/* ProductTower.forward (product_tower.py:43-62) with its 6 CosineVectorEmbedding
 * modules (commons/transformers/layers.py:443-471) fused per token. */
typedef struct lthm_ptower_desc {
  const int64_t* ids;
  const void* x;
  int32_t x_dtype;
  int32_t Din;
  int64_t n;
  int32_t Dout;
  int32_t n_mod;
  const float* w_map;
  const float* b_map;
  const float* proj;
  const float* grids;
  const void* tables;
  const void* hist;
  int32_t tab_dtype;
  int32_t proj_total;
  int32_t grid_total;
  int32_t cve_rows;
  int32_t norm_bins;
  float norm_threshold;
  int32_t cve_only;       /* 1: plain CosineVectorEmbedding(s): sum of bags only, one normalisation */
  int32_t emb_dtype;      /* dtype of emb_out: LTHM_F32 or LTHM_BF16 */
  int32_t mod_nproj[8];
  int32_t mod_nbins[8];
  int32_t mod_row_off[8];
  int32_t mod_proj_off[8];
  int32_t mod_grid_off[8];
  void* emb_out;
  uint16_t* rows_out;
  void* xn_out;
  uint8_t* mask_out;
} lthm_ptower_desc;

int lthm_product_tower_fwd(const lthm_ptower_desc* desc, void* stream);

/* Which kernels lthm_product_tower_fwd runs for a descriptor and with what geometry, decided on
 * the host from the descriptor's numbers and from which of its pointers are null (no GPU call,
 * no device memory touched).  lthm_product_tower_fwd launches from this plan.  The return value
 * is nonzero (1) for a descriptor the forward refuses (the plan is then undefined): Din outside
 * 1 .. 256, Dout outside 1 .. 512, more than LTHM_MAX_CVE modules, more than 1024 index slots,
 * Dout no multiple of the per-token kernel's outputs per lane, or the per-token kernel's LDS
 * above 160 KiB (asked of every descriptor, whichever path it takes).  With n == 0 nothing is
 * launched: the plan is all zeros and only the first three ranges are asked.
 *   LTHM_PT_MFMA:  ptower_rows_k<x, DM> (bucket rows, mask, xn) then ptower_emb_mfma_k<x, NF, DMA>
 *                  (bag sums as a one-hot MFMA GEMM, mapper as bf16 hi / lo splits).  Taken when
 *                  the descriptor is a tower (not cve_only) with bf16 tables and bf16 emb_out,
 *                  ids, rows_out and mask_out given, a column slice of 16 / 32 / 64 / 128 / 256,
 *                  1 <= R <= 4096 table rows, Din <= 64 and a multiple of 4, at most 32 bins per
 *                  module, at most 256 projections, and the embedding kernel's LDS within 160 KiB.
 *   LTHM_PT_TOKEN: ptower_fwd_k<x, table, OPL>, a wave per token; everything else. */
#define LTHM_PT_TOKEN 0
#define LTHM_PT_MFMA 1
typedef struct lthm_ptower_plan_out {
  int32_t path;        /* LTHM_PT_MFMA or LTHM_PT_TOKEN */
  int32_t total;       /* index slots per token: all projections + 1 for the histogram row */
  int32_t R;           /* table rows: cve_rows + norm_bins */
  int32_t R32;         /* R rounded up to the 32-row slab */
  int32_t nslab;       /* R32 / 32 */
  int32_t nslice;      /* column slices of Dout (grid.y of the embedding kernel): 2 for Dout 512 */
  int32_t rows_dm;     /* MFMA: ptower_rows_k's DM, 32 or 64; 0 on the per-token path */
  int32_t rows_full;   /* MFMA: 1 when Din == DM, the x rows stage through LDS */
  int32_t nf;          /* MFMA: 16-column fragments of one slice (1, 2, 4, 8, 16); else 0 */
  int32_t dma;         /* MFMA: 1 = 4-deep LDS-DMA slab ring, 0 = register double buffer */
  int32_t opl;         /* outputs per lane of ptower_fwd_k for this Dout (1, 2, 4, 8) */
  int32_t rows_grid;   /* workgroups of ptower_rows_k (256 threads); 0: not launched */
  int32_t emb_grid_x;  /* workgroups of ptower_emb_mfma_k (512 threads): 128-token blocks ... */
  int32_t emb_grid_y;  /* ... by column slices; 0: not launched */
  int32_t tok_grid;    /* workgroups of ptower_fwd_k (256 threads); 0: not launched */
  int32_t pad0;
  int64_t rows_lds_static;  /* bytes of ptower_rows_k's __shared__ arrays (0 when not launched) */
  int64_t emb_lds_dynamic;  /* dynamic LDS of ptower_emb_mfma_k (as computed, also when not taken) */
  int64_t tok_lds_dynamic;  /* dynamic LDS of ptower_fwd_k (as computed, also when not taken) */
} lthm_ptower_plan_out;
int lthm_product_tower_plan(const lthm_ptower_desc* desc, lthm_ptower_plan_out* plan);

/* Row gather (scatter = 0: dst row i = src row idx[i], a zero row where idx[i] < 0) or scatter
 * (scatter = 1: dst row idx[i] = src row i, skipped where idx[i] < 0) of `count` rows of
 * row_bytes (a multiple of 16; 16-B aligned pointers and leading dims).  The product tower's
 * token compaction (models/lthm/sequence/product_tower.py:43-62: a pad token's embedding is
 * masked to zero, so the tower runs on the non-pad tokens only). */
int lthm_rows_move(const void* src, int64_t src_ld_bytes, const int32_t* idx, int64_t count, void* dst,
                   int64_t dst_ld_bytes, int64_t row_bytes, int32_t scatter, void* stream);

/* Shared pad prefix (query_tower.py:99-137 over left-padded histories, encoder.py:52): with causal
 * attention, no dropout and the same position-0 token for every sequence, a pad position's state
 * depends only on its position, so the encoder runs the pad chain (positions 0 .. P) once and
 * each sequence's positions past its pads ("packed" rows: the chain first, then the sequences'
 * valid positions in order).
 *   stats:  npad[b] = leading set bytes of mask row b; stats = {1 if every row is a prefix mask,
 *           sum of T - npad, P = max npad, the first b with npad = P (the chain's owner)}.
 *   maps:   full row f = b Tp + p (Tp = T + 1) -> packed row pof[f] (the chain row p for p <= npad[b]);
 *           pof_x[f] the same but -1 at the pad rows of every sequence except the owner;
 *           fop[r] = the full row of packed row r (chain rows: the owner's).  voff[b] = exclusive
 *           prefix sum of T - npad.
 *   sum:    dst[p] (p <= P, packed chain rows) = sum over b with npad[b] >= p of src[b Tp + p]
 *           (W elements of rows src_ld / dst_ld elements apart, bf16 or f32, W, src_ld, dst_ld
 *           multiples of 8; fixed order); ws of lthm_pad_prefix_ws_bytes bytes. */
int lthm_pad_prefix_stats(const uint8_t* mask, int64_t mask_stride, int32_t B, int32_t T, int32_t* npad,
                          int32_t* stats, void* stream);
int lthm_pad_prefix_maps(const int32_t* npad, const int64_t* voff, int32_t B, int32_t Tp, int32_t P, int32_t owner,
                         int32_t* pof, int32_t* pof_x, int32_t* fop, void* stream);
int64_t lthm_pad_prefix_ws_bytes(int32_t B, int32_t P, int32_t W);
int lthm_pad_prefix_sum(const void* src, int64_t src_ld, int32_t dtype, int32_t W, const int32_t* npad, int32_t B,
                        int32_t Tp, int32_t P, void* dst, int64_t dst_ld, void* ws, int64_t ws_bytes, void* stream);

/* dW[rows[t, i]] += dY[t, :] for all tokens t, slots i < nidx <= 64 (0xffff = skip).
 * LDS-privatised EmbeddingBag / Embedding backward for tables of R < 65535 rows.
 * `workspace` (device, may be NULL) holds per-token-chunk partial sums; with
 * >= 2 * R * D * 4 bytes the tokens are split into chunks that are folded into
 * dW in a fixed order (no global atomics).  dW is accumulated into. */
int lthm_small_table_bwd(const uint16_t* rows, int32_t nidx, const void* dY, int32_t dy_dtype, int64_t ldy,
                         int64_t n, int32_t R, int32_t D, float* dW, void* workspace, int64_t workspace_bytes,
                         void* stream);
/* Same, with the slots grouped into nseg (<= 64) segments: segment s covers slots
 * [seg_slot0[s], +seg_nslot[s]) (nslot <= 64) whose rows all lie in
 * [seg_row0[s], +seg_nrow[s]); segment row ranges are disjoint.  A segment's
 * [nrow, 64] f32 slice is held in LDS, so nrow <= 640 (<= 256 keeps two blocks
 * per CU).  The seg_* arrays are HOST arrays. */
int lthm_segmented_table_bwd(const uint16_t* rows, int32_t nidx, int32_t nseg, const int32_t* seg_slot0,
                             const int32_t* seg_nslot, const int32_t* seg_row0, const int32_t* seg_nrow,
                             const void* dY, int32_t dy_dtype, int64_t ldy, int64_t n, int32_t D, float* dW,
                             void* workspace, int64_t workspace_bytes, void* stream);
/* CosineVectorEmbedding / EmbeddingBag gradient for CVE-structured tables on
 * MFMA: module j covers slots [mod_slot0[j], +mod_nslot[j]) and slot s owns rows
 * [mod_row0[j] + (s - mod_slot0[j]) * mod_rps[j], +mod_rps[j]) (module row ranges
 * disjoint, nmod <= 16, <= 64 tiles of 128 rows).  dY bf16 [n, D] with D in
 * {16, 32, 64, 128, 256} (f32 dY is split into bf16 hi + lo); dW f32 accumulated;
 * workspace as lthm_small_table_bwd.
 * (commons/transformers/layers.py:462-471 backward; product_tower.py:43-62).
 * The mod_* arrays are HOST arrays. */
int lthm_cve_table_bwd(const uint16_t* rows, int32_t nidx, int32_t nmod, const int32_t* mod_slot0,
                       const int32_t* mod_nslot, const int32_t* mod_row0, const int32_t* mod_rps,
                       const void* dY, int32_t dy_dtype, int64_t ldy, int64_t n, int32_t D, float* dW,
                       void* workspace, int64_t workspace_bytes, void* stream);
/* Same one-hot MFMA gradient for a small table of R rows whose nidx <= 8 slots
 * may each reference any row (0xffff = skip): dW[rows[t, i]] += dY[t, :]
 * (nn.Embedding / EmbeddingBag-sum backward: the query tower's action, time,
 * position and pad tables, outcome conditioning).  dY f32 (hi + lo bf16 split)
 * or bf16 [n, D], D in {16, 32, 64, 128, 256}; R <= 8192. */
int lthm_table_bwd_mfma(const uint16_t* rows, int32_t nidx, int32_t R, const void* dY, int32_t dy_dtype,
                        int64_t ldy, int64_t n, int32_t D, float* dW, void* workspace, int64_t workspace_bytes,
                        void* stream);
/* QuantileMapper (commons/transformers/layers.py:477-487) on x [B, F]:
 * out = bucketize(x[:, f], q_f) / (nq + 1) - 0.5; quantiles [shared ? 1 : F, nq]. */
int lthm_quantile_map(const float* x, int64_t B, int32_t F, const float* quantiles, int32_t nq, int32_t shared,
                      float* out, void* stream);

/* Vector-feature layers (commons/transformers/layers.py), f32, all device pointers.
 * rowproj_fwd: z[r, j] = s_r sum_k x[r, k] W[j, k] with W[j, k] at w[j*ldj + k*ldk], x [rows, dim].
 *   mode 0 SimhashVectorIndexer (:426-437): out int64 [rows] = sum_j (z[r, j] > 0) << j, P <= 64;
 *   mode 1 CosineLinear (:517-525) forward with w = normalize(W) [P, dim]:
 *          out f32 [rows, P] = z / max(|x_r|, 1e-12). */
int lthm_rowproj_fwd(const float* x, int64_t rows, int32_t dim, const float* w, int64_t ldj, int64_t ldk, int32_t P,
                     int32_t mode, void* out, void* stream);
/* F.normalize(x, dim=-1) over f32 rows */
int lthm_l2norm_rows(const float* x, int64_t rows, int32_t dim, float* y, void* stream);
/* its backward dx = (g - y (y . g)) / |x| (g / eps when |x| <= eps); exactly one of
 * g [rows, dim] or dz [rows, P] (then g = dz @ w_hat, w_hat [P, dim]: CosineLinear's x
 * side) is given; rinv [rows] (may be NULL) receives 1 / max(|x|, eps). */
int lthm_l2norm_rows_bwd(const float* x, int64_t rows, int32_t dim, const float* g, const float* dz,
                         const float* w_hat, int32_t P, float* dx, float* rinv, void* stream);
/* CosineLinear weight side: dw_hat[j, k] += sum_r dz[r, j] x[r, k] rinv[r] (accumulates). */
int lthm_cosine_wgrad(const float* dz, const float* x, const float* rinv, int64_t rows, int32_t P, int32_t dim,
                      float* dw_hat, void* stream);
/* Gaussian bins of LearnableCosineVectorEmbedding / ProbabilityVectorEmbedding
 * (:558-569, :588-595): z [n] f32 with n = rows * P, element i at projection p = i % P,
 * mean [P, nb] (nb <= 64): out[i, b] = normalize_b(topk_b(exp(-0.5 (z_i - mean[p, b])^2 / sigma2)));
 * top_k 0 = no top-k.  out_dtype LTHM_F32 or LTHM_BF16.  bwd: dz [n] (may be NULL) and
 * dmean [P, nb] (accumulated) from gout [n, nb] (g_dtype F32 / BF16). */
int lthm_gauss_bins_fwd(const float* z, int64_t n, int32_t P, const float* mean, int32_t nb, float sigma2,
                        int32_t top_k, void* out, int32_t out_dtype, void* stream);
int lthm_gauss_bins_bwd(const float* z, int64_t n, int32_t P, const float* mean, int32_t nb, float sigma2,
                        int32_t top_k, const void* gout, int32_t g_dtype, float* dz, float* dmean, void* stream);

/* MoELinear (commons/transformers/layers.py:101-136), the parts around its GEMMs.
 * gate: probs[m, :] = softmax(g) with g = scale * logits[m, :] and, when top_k > 0,
 * g[e] -> -inf where g[e] is below the top_k-th largest (:123-127); E <= 64.
 * gate_bwd: dlogits = scale * p (dp - sum_j p_j dp_j).
 * scale: GH[m, e P + p] = probs[m, e] * H[m, e P + p]   (bf16 in / out).
 * hidden_bwd: dg[m, e] = sum_p dGH H;  dpre = probs[m, e] dGH gelu_tanh'(pre)  (bf16 out). */
int lthm_moe_gate_fwd(const float* logits, int64_t M, int32_t E, float scale, int32_t top_k, float* probs,
                      void* stream);
int lthm_moe_gate_bwd(const float* probs, const float* dprobs, int64_t M, int32_t E, float scale, float* dlogits,
                      void* stream);
int lthm_moe_scale(const void* H, const float* probs, int64_t M, int32_t E, int32_t P, void* GH, void* stream);
int lthm_moe_hidden_bwd(const float* dGH, const void* H, const void* pre, const float* probs, int64_t M, int32_t E,
                        int32_t P, void* dpre, float* dg, void* stream);

/* Binary cross-entropy with logits, mean reduction
 * (F.binary_cross_entropy_with_logits; the ranker's click loss and
 * embedding_module_gen.py:112-116's mask-model loss).
 * fwd: *loss_sum += inv_n * sum_i [max(z,0) - z y + log1p(exp(-|z|))]  (caller zeroes it)
 * bwd: dz_i = (sigmoid(z_i) - y_i) * (*gscale) * inv_n                      */
int lthm_bce_logits_fwd(const float* z, const float* y, int64_t n, float inv_n, float* loss_sum, void* stream);
int lthm_bce_logits_bwd(const float* z, const float* y, int64_t n, const float* gscale, float inv_n, float* dz,
                        void* stream);

/* nn.MSELoss (embedding_module_gen.py:139-150): loss_sum += inv_n * sum (y - x)^2 (zero it
 * first); bwd dy = 2 (y - x) * (*gscale) * inv_n.  y F32 or BF16 (dy the same), x f32. */
int lthm_mse_fwd(const void* y, int32_t y_dtype, const float* x, int64_t n, float inv_n, float* loss_sum, void* stream);
int lthm_mse_bwd(const void* y, int32_t y_dtype, const float* x, int64_t n, const float* gscale, float inv_n, void* dy,
                 void* stream);

/* QueryTower input assembly (query_tower.py:89-111): action + time embeddings,
 * pad substitution, zero/CLS token, reversed position embedding. */
typedef struct lthm_tokens_desc {
  const void* P;
  int32_t p_dtype;
  int32_t d;
  const int64_t* labels;
  const int64_t* ts;
  const uint8_t* mask;
  int64_t B;
  int32_t T_full;
  int32_t trim;
  const float* act;
  const float* hod;
  const float* how;
  const float* dow;
  const float* wpe;
  const float* pad;
  const float* ctx;
  int32_t off_act;
  int32_t off_hod;
  int32_t off_how;
  int32_t off_dow;
  int32_t off_wpe;
  int32_t off_pad;
  int64_t div_hod;
  int64_t mod_hod;
  int64_t div_how;
  int64_t mod_how;
  int64_t div_dow;
  int64_t mod_dow;
  float* x0;
  uint16_t* rows_out;
} lthm_tokens_desc;

int lthm_tokens_fwd(const lthm_tokens_desc* desc, void* stream);
/* dP (bf16 [B, T, d]) = unmasked dx0[:, 1:], dctx (f32 [B, d], may be NULL) = dx0[:, 0] */
int lthm_tokens_bwd(const lthm_tokens_desc* desc, const float* dx0, void* dP, float* dctx, void* stream);
/* out = bf16(x + table[outcome mod n_outcomes]) (query_tower.py:118-122); rows_out [B*(T+1)] */
int lthm_outcome_fwd(const float* x, const int64_t* labels, int64_t B, int32_t T_full, int32_t trim,
                     int64_t future, const float* table, int32_t n_outcomes, int32_t D, void* out,
                     uint16_t* rows, void* stream);

/* Row-sharded KShift lookup routing (C3 item table; commons/layers.py:152-185 row math,
 * SURVEY §8e): global row r on rank r % world at local index r / world.
 * lthm_shard_route: the K rows of n_items ids, deduplicated per workgroup of 2,048 (row, shift)
 * pairs (LDS bitonic sort), laid out owner-major in send_rows [capacity n_items * K];
 * send_counts [world] and owner_base [world + 1] (owner_base[world] = the request total) stay on
 * the device; inv [n_items * K] holds, for every pair, the position of its row's value in the
 * buffer the exchange returns (owner-major, the send order).  Replaces torch.unique / argsort /
 * bincount of the reference-style exchange; workspace: lthm_shard_route_ws_bytes bytes.
 * 1 <= world <= 256 (the per-owner counts live in LDS); larger worlds are refused. */
int64_t lthm_shard_route_ws_bytes(int64_t n_pairs, int32_t world);
int lthm_shard_route(const int64_t* ids, int64_t n_items, int32_t K, int64_t P, int32_t world, int64_t* send_rows,
                     int64_t* send_counts, int64_t* owner_base, int64_t* inv, void* workspace, int64_t ws_bytes,
                     void* stream);
/* out[i] = shard[rows[i] / world] (row_bytes a multiple of 16) for i < min(*count, cap) (count NULL: cap);
 * the owner side of the exchange (and the whole lookup at world 1) */
int lthm_shard_gather(const void* shard, int64_t n_local, int32_t row_bytes, const int64_t* rows,
                      const int64_t* count, int64_t cap, int32_t world, void* out, void* stream);

/* ------------------------------------------------------------------------- */
/* In-batch contrastive loss (models/lthm/sequence/wrapper.py:114-245)        */
/* ------------------------------------------------------------------------- */
/* F.normalize of rows: out bf16 [rows, D], norms f32 [rows] (wrapper.py:118-119).
 * row_mask (may be NULL): rows r with row_mask[(r / mask_group) * mask_stride + r % mask_group]
 * set get a zero output row (the loss zeroes the `in` rows of pad positions, which
 * every logit of them excludes; their norm is still written). */
int lthm_rownorm(const void* x, int32_t x_dtype, int64_t rows, int32_t D, void* out_bf16, float* norms,
                 const uint8_t* row_mask, int64_t mask_group, int64_t mask_stride, void* stream);
/* backward of lthm_rownorm: dx = (g - y (y.g)) / |x|; writes dx_bf16 and/or dx_f32 */
int lthm_rownorm_bwd(const void* x, int32_t x_dtype, const float* norms, const float* g, int64_t rows,
                     int32_t D, void* dx_bf16, float* dx_f32, void* stream);

typedef struct lthm_contrastive_desc {
  const void* out_n;      /* bf16 [B, T+1, n_heads, De] normalised next_token_emb */
  const void* in_n;       /* bf16 [B, T, De] normalised current_token_emb */
  const uint8_t* mask;    /* [B, mask_stride] pad mask (already offset by the trim) */
  int64_t mask_stride;
  int64_t B;
  int32_t T;
  int32_t n_heads;
  int32_t head;
  int32_t De;
  int32_t mb_size;        /* train_mini_batch_size (32) */
  int32_t n_mb;
  int32_t n_max;          /* >= mb_size * T, a multiple of 64, n_max * T < 2^32 (no other limit: val_step
                             runs the whole batch as one mini-batch, wrapper.py:75-80) */
  float tau;              /* softmax_temperature */
  const int32_t* offsets; /* [n_mb, n_heads] lookahead offset per mini-batch and head */
  float* lse;             /* [n_mb, n_max] per-row buffers (this head) */
  float* pos;
  int32_t* cnt;
  int32_t* rank;
  float* diag;            /* forward: positive logit (-inf: pad row / r >= n);
                             backward: scratch for the per-row exp2 shift */
  float* w;               /* row weights, written by the forward, read by the backward */
  const float* gscale;    /* device scalar: upstream gradient of the loss (backward) */
  float* d_out;           /* f32 [B, T+1, n_heads, De]: every row of this head is written (no pre-zeroing) */
  float* d_in;            /* f32 [B, T, De] (accumulated over heads) */
  const float* logq;      /* NULL, or f32 [B, logq_stride]: additive logit correction -beta * logQ(id)
                             of every input token (wrapper.py:131-135, 204-208; zero on the positive) */
  int64_t logq_stride;
  float* logq_col;        /* with logq: [n_mb, n_max] scratch written by the forward, read by the backward */
  const void* y_raw;      /* backward, optional: [B, T+1, n_heads, De] next_token_emb before F.normalize (dtype y_dtype;
                             bf16 only without t_raw) */
  const float* y_norm;    /* with y_raw: f32 [B, T+1, n_heads] its row norms (lthm_rownorm) */
  void* dy;               /* with y_raw: [B, T+1, n_heads, De] (dtype y_dtype) written INSTEAD of d_out: the gradient through
                             F.normalize (wrapper.py:118-119), every row of this head written */
  int32_t heads_run;      /* forward: heads head .. head + heads_run - 1 in one set of launches (0 or 1: one) */
  int64_t head_stride;    /* with heads_run > 1: elements between consecutive heads' lse / pos / cnt / rank /
                             diag / w / logq_col buffers; stats rows advance by n_mb * nstat */
  int32_t y_dtype;        /* LTHM_F32 / LTHM_BF16: dtype of y_raw and dy */
  const void* t_raw;      /* backward, with y_raw / dy: [B, T, De] current_token_emb before F.normalize (dtype t_dtype);
                             then every head runs in ONE call (head 0, heads_run = n_heads) and dIn is summed over
                             the heads on chip: dt is written once, through F.normalize, instead of d_in */
  int32_t t_dtype;
  const float* t_norm;    /* with t_raw: f32 [B, T] its row norms (lthm_rownorm) */
  void* dt;               /* with t_raw: [B, T, De] (dtype t_dtype): d current_token_emb, every row written */
  void* stats_ws;         /* forward: device workspace of lthm_contrastive_ws_bytes(n_mb, n_max, heads_run)
                             bytes (rank histograms + per-block partial sums) */
  int64_t stats_ws_bytes;
  int32_t rows_done;      /* backward: the forward already wrote dy (it was given y_raw / y_norm / dy at the fixed
                             shift: the fused forward + ROWS pass) for a unit upstream gradient; the backward
                             then runs the COLS side only and scales dy by *gscale */
  void* main_ev0;         /* optional hipEvent_t pair recorded on the stream around the call's main pass alone
                             (forward: cl_fr32_k / cl_fwd_k; backward: the cl_bwd32_k columns / rows passes),
                             for live per-kernel timing (bench.py); NULL: not recorded */
  void* main_ev1;
  void* vc_ws;            /* optional, training at the fixed shift (the fused forward + ROWS pass and its rows_done
                             backward): device workspace of lthm_contrastive_vc_ws_bytes bytes, the SAME buffer for the
                             forward and its backward.  The S passes then run over the valid (non-pad) indices of each
                             (mini-batch, head) only -- every logit of a pad row or column is excluded anyway
                             (wrapper.py:175-190).  Requires head 0, heads_run = n_heads, head_stride = n_mb * n_max,
                             mb_size <= 4096.  NULL: the full n x n passes */
  int64_t vc_ws_bytes;
} lthm_contrastive_desc;

/* bytes of lthm_contrastive_desc.vc_ws (-1: invalid sizes) */
int64_t lthm_contrastive_vc_ws_bytes(int64_t B, int32_t T, int32_t n_heads, int32_t mb_size, int32_t n_mb,
                                     int32_t n_max);
/* bytes of lthm_contrastive_desc.stats_ws for one forward launch (-1: invalid sizes) */
int64_t lthm_contrastive_ws_bytes(int32_t n_mb, int32_t n_max, int32_t heads);

/* Forward for one head (or heads_run consecutive heads) over all mini-batches.  stats [n_mb, nstat] f32 per head
 * (nstat >= 8 + nk): {mean CE over the used tokens, used rows (effective batch), mean negatives, min negatives,
 *  mean rank, median rank, offset, used tokens, hit@ks[0..nk)}; a used row whose CE is NaN leaves the mean and
 *  the used tokens (wrapper.py:210-214); loss_scale multiplies the row weights (1 / n_mb).
 * Training at the fixed shift (2 / tau <= 80, no logq) with y_raw / y_norm / dy given (heads 0 .. n_heads - 1,
 * mb_size <= 4096 sequences): one pass per row block computes the forward AND the row side of the backward,
 * writing dy for a unit upstream gradient; the backward is then called with rows_done = 1. */
int lthm_contrastive_fwd(const lthm_contrastive_desc* desc, float* stats, int32_t nstat, const int32_t* ks,
                         int32_t nk, float loss_scale, void* stream);
int lthm_contrastive_bwd(const lthm_contrastive_desc* desc, void* stream);

/* ------------------------------------------------------------------------- */
/* Optimizers and gradient transforms                                        */
/* ------------------------------------------------------------------------- */
/* torch.optim.AdamW step on a flat fp32 tensor (wrapper.py:263-275); optional bf16
 * shadow of the updated parameter; grad_scale multiplies g (clipping). */
int lthm_adamw(float* p, float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
               float eps, float weight_decay, int64_t step, float grad_scale, void* bf16_shadow,
               int32_t zero_grad, void* stream);
/* Multi-tensor form of lthm_adamw (optional bf16 shadows pb, no grad zeroing): `count` tensors given by
 * host arrays of device pointers p/g/m/v and element counts n, all with the same
 * hyper-parameters and step; one launch per 48 tensors (torch.optim.AdamW foreach). */
int lthm_adamw_multi(int32_t count, float** p, float** g, float** m, float** v,
                     const int64_t* n, float lr, float beta1, float beta2, float eps, float weight_decay,
                     int64_t step, float grad_scale, void* stream);
/* torch.optim.Adagrad step (embedding_module_gen.py:97,137) */
int lthm_adagrad(float* p, float* g, float* state_sum, int64_t n, float lr, float lr_decay, float eps,
                 float weight_decay, int64_t step, int32_t zero_grad, void* stream);
/* row-wise (lazy) AdamW / Adagrad over the touched rows of a [R, D] table; each
 * consumed gradient row is re-zeroed and its flag cleared.  max_rows bounds *count. */
int lthm_sparse_adamw(const int64_t* rows, const int64_t* count, int64_t max_rows, int32_t D, float* p,
                      float* g, float* m, float* v, int32_t* flags, float lr, float beta1, float beta2,
                      float eps, float weight_decay, int64_t step, void* bf16_shadow, void* stream);
int lthm_sparse_adagrad(const int64_t* rows, const int64_t* count, int64_t max_rows, int32_t D, float* p,
                        float* g, float* state_sum, int32_t* flags, float lr, float lr_decay, float eps,
                        int64_t step, void* bf16_shadow, void* stream);
/* lthm_sparse_adamw / lthm_sparse_adagrad with keep_grad = 1: the consumed gradient rows are NOT
 * re-zeroed -- for tables whose next backward overwrites a row at its first touch
 * (lthm_kshift_bwd_sparse_first with a touched-row bitmap the caller clears after the step), so the
 * zero store is dead traffic; keep_grad = 0 is the plain entry point.  Round 6 (ABI 41). */
int lthm_sparse_adamw_ex(const int64_t* rows, const int64_t* count, int64_t max_rows, int32_t D, float* p,
                         float* g, float* m, float* v, int32_t* flags, float lr, float beta1, float beta2,
                         float eps, float weight_decay, int64_t step, void* bf16_shadow, int32_t keep_grad,
                         void* stream);
int lthm_sparse_adagrad_ex(const int64_t* rows, const int64_t* count, int64_t max_rows, int32_t D, float* p,
                           float* g, float* state_sum, int32_t* flags, float lr, float lr_decay, float eps,
                           int64_t step, void* bf16_shadow, int32_t keep_grad, void* stream);
/* *out_accum += sum(x^2) */
int lthm_sumsq(const void* x, int32_t dtype, int64_t n, float* out_accum, void* stream);
/* max_norm <= 0: y = x / (sqrt(*sumsq) + add_eps)   (cap_gradients, commons/functional.py:23)
 * max_norm  > 0: y = x * min(1, max_norm / (sqrt(*sumsq) + 1e-6))   (clip_grad_norm_) */
int lthm_scale_by_norm(const void* x, void* y, int32_t dtype, int64_t n, const float* sumsq, float add_eps,
                       float max_norm, void* stream);

/* ------------------------------------------------------------------------- */
/* streaming helpers                                                         */
/* ------------------------------------------------------------------------- */
int lthm_cast(const void* in, int32_t in_dtype, void* out, int32_t out_dtype, int64_t n, void* stream);
/* out[t][i] = bf16(in[t][i]) for count tensors of n[t] f32 elements (host arrays of
 * device pointers): the bf16 GEMM operands of a model's fp32 weights, cast in one
 * launch per 48 tensors at the start of each forward (no cross-step copies to go stale) */
int lthm_cast_multi_bf16(int32_t count, float** in, void** out, const int64_t* n, void* stream);
/* out[c] (+)= sum_r in[r*ld + c], c < cols (f32 out) */
int lthm_colsum(const void* in, int32_t dtype, int64_t rows, int64_t cols, int64_t ld, float* out,
                int32_t accumulate, void* stream);
int lthm_fill_f32(float* p, float value, int64_t n, void* stream);
/* nn.Dropout(p) (commons/transformers/layers.py:253-256, 264, 283; query_tower.py:133).
 * Element i is kept iff (splitmix64(seed + i * 0x9E3779B97F4A7C15) >> 40) / 2^24 >= p,
 * kept values are scaled by 1 / (1 - p); the backward calls the same entry point with
 * the forward's seed.  0 <= p < 1.
 * lthm_dropout:      y = [res1] + [res2] + dropout(x)   (res1 / res2: f32 or NULL)
 * lthm_dropout_rows: x [rows, groups * cols] in place, row r of group g scaled by the
 *                    decision for index g * rows + r (token dropout of q / k / v)
 * lthm_dropout_mask: out[i] = keep decision (uint8), for tests and inspection */
int lthm_dropout(const void* x, int32_t x_dtype, void* y, int32_t y_dtype, int64_t n, float p, uint64_t seed,
                 const float* res1, const float* res2, void* stream);
int lthm_dropout_rows(void* x, int32_t dtype, int64_t rows, int32_t cols, int32_t groups, float p, uint64_t seed,
                      void* stream);
int lthm_dropout_mask(uint8_t* out, int64_t n, float p, uint64_t seed, void* stream);
/* Streaming logQ for the LTHM loss (commons/layers.py:189-237 CascadedStreamingLogQ-
 * CorrectionModule, as wrapper.py:126-136 drives it per mini-batch of mb_size sequences):
 * for mini-batch k in order, train_step on its non-pad ids at batch index batch_idx0 + k,
 * then out[b, t] = -beta * min_m(-log b_m[(id + hash_offsets[m]) mod num_buckets]) for
 * all its ids.  b_tables / a_tables: f32 [n_modules, num_buckets] (the modules' b / a
 * buffers stacked), updated in place, bit-identical to the reference's sequence of
 * train_steps.  ids [B, ids_stride], mask [B, mask_stride] (1 = pad; NULL = no pads), out
 * f32 [B, T] or NULL (update only: the β = 0 case, where the reference trains the
 * estimates but the correction vanishes).  update = 0 skips the train_step (the module's
 * plain forward; beta = -1 then returns min_m -log b).  With update, workspace holds
 * lthm_logq_ws_bytes(B, T, mb_size, n_modules) bytes (a per-call bucket table; every
 * mini-batch's updates run in parallel over buckets).  n_modules * num_buckets < 2^32 - 1. */
int64_t lthm_logq_ws_bytes(int64_t B, int32_t T, int32_t mb_size, int32_t n_modules);
int lthm_logq_stream(const int64_t* ids, int64_t ids_stride, const uint8_t* mask, int64_t mask_stride, int64_t B,
                     int32_t T, int32_t mb_size, float* b_tables, float* a_tables, const int64_t* hash_offsets,
                     int32_t n_modules, int64_t num_buckets, float alpha, int64_t batch_idx0, float beta,
                     int32_t update, float* out, void* workspace, int64_t ws_bytes, void* stream);
/* History-trim statistics of mask [B, T] (uint8, 1 = pad) for query_tower.py:73-86:
 * work[0] = first column holding a non-pad entry (T if none), work[1] = number of
 * all-pad columns; work is a device int32 buffer of T + 2 entries (work[2..] scratch). */
int lthm_trim_stats(const uint8_t* mask, int64_t B, int32_t T, int32_t* work, void* stream);
/* y = act(x) (dy == NULL) or y = dy * act'(x); act = LTHM_ACT_GELU / LTHM_ACT_QGELU */
int lthm_activation(const void* x, const void* dy, void* y, int32_t dtype, int64_t n, int32_t act, void* stream);

/* ------------------------------------------------------------------------- */
/* Full-catalogue top-K retrieval (csrc/retrieve.hip)                        */
/* ------------------------------------------------------------------------- */
/* The two-tower model's use: next_token_emb[:, t, head] is a query, the product tower's
 * prod_emb a candidate (wrapper.py:114-119 normalises both for the loss).  For every query
 * the k catalogue rows with the largest dot product, sorted by (score descending, row
 * ascending), without a [Q, N] score buffer.
 *   items         bf16 [N, 128], row-major, already normalised; 1 <= N < 2^31
 *   q             f32 / bf16 [Q, 128]; with normalize_q each row goes through F.normalize
 *                 (eps 1e-12) first and is rounded to bf16 as lthm_rownorm does
 *   target_row    int32 [Q] or NULL: a catalogue row per query, or -1 (rows outside [0, N)
 *                 count as -1)
 *   scores, rows  f32 / int32 [Q, k], k in 1..128; where N < k the tail is -inf / -1
 *   rank          int32 [Q] (with target_row): #{j != target : s[q, j] > s[q, target]}, the
 *                 strict-greater count of the in-batch hit position; -1 without a target
 *   target_score  f32 [Q] (with target_row): the f32 dot of the two bf16 rows (-inf without)
 *   slab_rows     catalogue rows per block of the scoring kernel: a multiple of 64, or 0 for
 *                 the size the call derives from Q and N
 *   workspace     lthm_retrieve_ws_bytes(Q, N, k, slab_rows) bytes, 16-byte aligned
 * items and q must be 16-byte aligned.  The outputs are a pure function of the inputs. */
typedef struct lthm_retrieve_desc {
  const void* items;
  const void* q;
  const int32_t* target_row;
  float* scores;
  int32_t* rows;
  int32_t* rank;
  float* target_score;
  void* workspace;
  int64_t ws_bytes;
  int64_t Q;
  int64_t N;
  int32_t k;
  int32_t q_dtype;
  int32_t normalize_q;
  int32_t slab_rows;
} lthm_retrieve_desc;
/* workspace bytes of lthm_retrieve_topk, or -1 for sizes it refuses */
int64_t lthm_retrieve_ws_bytes(int64_t Q, int64_t N, int32_t k, int32_t slab_rows);
int lthm_retrieve_topk(const lthm_retrieve_desc* d, void* stream);
/* The same with per-query exclusion: the k best rows a query has not named.
 *   rows   int32 [Q, X], contiguous, 1 <= X <= 1024, each query's entries in any order;
 *          entries < 0 or >= N are ignored (-1 pads a short list), duplicates are allowed
 * An excluded row is scored as -inf: it never appears in scores / rows (where fewer than k rows
 * remain the tail is -inf / -1) and never counts in rank.  Order and tie rule are unchanged, and
 * the outputs do not depend on the order of a list.  The target is never excluded as a target:
 * target_score is the plain f32 dot and rank = #{j != target, j not excluded : s[q, j] >
 * s[q, target]}, also where a query lists its own target.  A query with no valid entry gets
 * exactly what lthm_retrieve_topk returns. */
typedef struct lthm_retrieve_excl {
  const int32_t* rows;
  int64_t X;
} lthm_retrieve_excl;
/* workspace bytes of lthm_retrieve_topk_excl (the plain call's plus the sorted lists), or -1
 * for what lthm_retrieve_ws_bytes refuses and for X outside 1..1024 */
int64_t lthm_retrieve_excl_ws_bytes(int64_t Q, int64_t N, int32_t k, int32_t slab_rows, int64_t X);
/* x == NULL is lthm_retrieve_topk; otherwise d->ws_bytes must cover lthm_retrieve_excl_ws_bytes */
int lthm_retrieve_topk_excl(const lthm_retrieve_desc* d, const lthm_retrieve_excl* x, void* stream);
/* Groups: every user has G queries (1 <= G <= 8, say one per lookahead head) and an item is
 * scored by its best match over them.  In the desc d->q is [U, G, 128] (contiguous) and d->Q = U;
 * scores / rows [U, k], target_row / rank / target_score [U] and x->rows [U, X] are per user.
 *   s_g[u, j]        the f32 score lthm_retrieve_topk gives query (u, g) against row j (the same
 *                    preparation, normalisation and accumulation)
 *   s[u, j]          max_g s_g[u, j], and -inf for a row user u excludes (one list per user, the
 *                    entries under the rules of lthm_retrieve_excl)
 *   scores, rows     the k <= 128 best rows of s[u, :] by (score descending, row ascending), the
 *                    tail -inf / -1 where fewer than k rows remain
 *   target_score[u]  max_g of the plain per-query target dots (-inf where target_row[u] is no
 *                    catalogue row)
 *   rank[u]          #{j != target, j not excluded : s[u, j] > target_score[u]}, or -1 where
 *                    the target is no catalogue row
 * The outputs are a pure function of the inputs and do not depend on the order of a user's
 * queries.  Which query attained a maximum is not reported.  Inputs are finite. */
typedef struct lthm_retrieve_group {
  int32_t G;
} lthm_retrieve_group;
/* workspace bytes of lthm_retrieve_topk_group; X = 0: no exclusion.  At G = 1 the value of
 * lthm_retrieve_ws_bytes (X = 0) or lthm_retrieve_excl_ws_bytes; -1 for what those refuse and
 * for G outside 1..8 */
int64_t lthm_retrieve_group_ws_bytes(int64_t U, int32_t G, int64_t N, int32_t k, int32_t slab_rows, int64_t X);
/* x == NULL: no exclusion.  g == NULL or g->G == 1 is lthm_retrieve_topk_excl(d, x, stream);
 * otherwise d->ws_bytes must cover lthm_retrieve_group_ws_bytes */
int lthm_retrieve_topk_group(const lthm_retrieve_desc* d, const lthm_retrieve_excl* x, const lthm_retrieve_group* g,
                             void* stream);
/* Tag filters: the k best rows among those a query may be shown.
 *   tags    int32 [N]: one word per catalogue row, read as 32 independent bits (bit 31 is an
 *           ordinary bit; only the bit pattern matters)
 *   filter  int32 [Q, 3] (with groups [U, 3], one per user): (all, any, none).  Row j is eligible
 *           for query q iff
 *             (tags[j] & all) == all  &&  (any == 0 || (tags[j] & any) != 0)  &&  (tags[j] & none) == 0
 * An ineligible row is treated exactly as an excluded row: it is scored as -inf, takes no slot
 * and never counts in rank; where fewer than k rows remain the tail is -inf / -1; order and tie
 * rule are unchanged.  The target is never filtered as a target: target_score is the plain dot
 * (with groups the best of the plain dots) and
 *   rank = #{j != target, j eligible, j not excluded : s_j > s_target}.
 * The filter (0, 0, 0) gives the bits of the call without tags; an unsatisfiable filter
 * (all & none != 0) gives an empty list and rank 0 for a valid target.  Filters compose with
 * exclusion and with groups.  The outputs stay a pure function of the inputs.  Both arrays are
 * read with 4-byte loads (4-byte aligned), tags never at or past N. */
typedef struct lthm_retrieve_tags {
  const int32_t* tags;
  const int32_t* filter;
} lthm_retrieve_tags;
/* t == NULL is lthm_retrieve_topk_group(d, x, g, stream); with t both pointers must be non-null.
 * The workspace is the group call's: lthm_retrieve_group_ws_bytes (with g == NULL, G = 1). */
int lthm_retrieve_topk_tags(const lthm_retrieve_desc* d, const lthm_retrieve_excl* x, const lthm_retrieve_group* g,
                            const lthm_retrieve_tags* t, void* stream);
/* Cursors: the k best rows strictly after a position of the total order (score descending, row
 * ascending), for "the next k" and for lists longer than one call returns.
 *   after_score  f32 [Q] (with groups [U], one cursor per user)
 *   after_row    int32 [Q] or [U]; any int32
 * Row j with f32 score s_j (with groups the best over the user's queries; -0 equals +0) is
 * eligible iff
 *             s_j < after_score  ||  (s_j == after_score && j > after_row)
 * A row that is not eligible is treated exactly as an excluded row: it is scored as -inf, takes no
 * slot and never counts in rank; target_score stays the plain dot; where fewer than k eligible
 * rows remain the tail is -inf / -1.  after_score = +inf admits every finite-scored row (the bits
 * of the call without a cursor); -inf or NaN admits none, so the (-inf, -1) tail of an exhausted
 * list is a valid cursor.  after_row = -1 admits the whole tie run at after_score, a value >= N
 * none of it.  A list's last (score, row) as the next call's cursor yields the following k rows
 * of the same order, whatever slab_rows or Q either call used.  Cursors compose with exclusion,
 * groups and tag filters.  Both arrays are read with 4-byte loads. */
typedef struct lthm_retrieve_cursor {
  const float* after_score;
  const int32_t* after_row;
} lthm_retrieve_cursor;
/* c == NULL is lthm_retrieve_topk_tags(d, x, g, t, stream); with c both pointers must be non-null
 * and 4-byte aligned.  The workspace is the group call's: lthm_retrieve_group_ws_bytes. */
int lthm_retrieve_topk_after(const lthm_retrieve_desc* d, const lthm_retrieve_excl* x, const lthm_retrieve_group* g,
                             const lthm_retrieve_tags* t, const lthm_retrieve_cursor* c, void* stream);
/* Score priors: a per-item bias, weighted per query, added to the score inside the kernel.
 *   bias    f32 [N]: one word per catalogue row, every value finite
 *   weight  f32 [Q] (with groups [U], one per user), or NULL for 1 everywhere
 * The score of row j for query q becomes
 *             s_j = fmaf(weight[q], bias[j], dot_j)
 * one f32 fused multiply-add on the f32 score dot_j the calls above give (with groups the best over
 * the user's queries: the prior is added after the maximum).  Everything else sees s_j and only
 * s_j: the order and the tie rule (score descending, row ascending), the scores returned, the
 * cursor test and rank.  A row at -inf (excluded, filtered, behind the cursor) stays at -inf.  The
 * target is biased the same way, target_score = fmaf(weight[q], bias[target], dot_target), which is
 * the value written and the value rank counts against:
 *   rank = #{j != target, j eligible : s_j > target_score};
 * the target is never excluded or filtered as a target.  weight = 0 and an all-zero bias give the
 * rows and ranks of the call without a prior, with equal scores (-0 may come back as +0).  A
 * non-finite weight gives that query an unspecified list and nothing else: weights and biases are
 * only ever values.  Priors compose with exclusion, groups, tag filters and cursors (a cursor is a
 * position in the order of the biased scores), and the outputs stay a pure function of the inputs.
 * Both arrays are read with 4-byte loads (4-byte aligned), bias never at or past N. */
typedef struct lthm_retrieve_bias {
  const float* bias;
  const float* weight;
} lthm_retrieve_bias;
/* b == NULL is lthm_retrieve_topk_after(d, x, g, t, c, stream); with b, bias must be non-null and
 * both pointers 4-byte aligned.  The workspace is the group call's: lthm_retrieve_group_ws_bytes. */
int lthm_retrieve_topk_bias(const lthm_retrieve_desc* d, const lthm_retrieve_excl* x, const lthm_retrieve_group* g,
                            const lthm_retrieve_tags* t, const lthm_retrieve_cursor* c, const lthm_retrieve_bias* b,
                            void* stream);
/* Deep lists: up to 1024 rows per query from one scan of the catalogue (the calls above stop at
 * k = 128).  For 129 <= d->k <= 1024 the four outputs are, bit for bit, what a caller of
 * lthm_retrieve_topk_bias gets who pages: ceil(k / 128) calls, each behind the last (score, row)
 * of the one before, concatenated, with rank and target_score those of the first call (whose
 * cursor is the caller's own).  That is: the k first eligible rows under (score descending, row
 * ascending) on the score of the calls above (the f32 dot, the best over a group, the prior), a row
 * being ineligible (-inf) when it is excluded, fails its tag filter or lies at or before the
 * cursor; -1 / -inf where fewer than k rows are eligible.  x, g, t, c and b compose as above and
 * each may be NULL.  The outputs are a pure function of the inputs (no global atomics; they depend
 * neither on slab_rows nor on Q), and a non-finite weight gives that query an unspecified list and
 * nothing else.
 *   workspace  lthm_retrieve_deep_ws_bytes(Q, G, N, k, slab_rows, X) bytes (X = 0: no list): the
 *              queries, nslab x Q x stride keys of 8 bytes with stride = 2048 (or max(k, slab_rows)
 *              for a slab_rows below 2048), nslab x Q counts and the sorted lists
 * lthm_retrieve_deep_ws_bytes takes k in 1..1024 and returns lthm_retrieve_group_ws_bytes for
 * k <= 128; -1 for what it refuses (k outside 1..1024, G outside 1..8, X outside 0..1024, a
 * slab_rows that is no multiple of 64).  With d->k <= 128, lthm_retrieve_topk_deep is exactly
 * lthm_retrieve_topk_bias(d, x, g, t, c, b, stream). */
int64_t lthm_retrieve_deep_ws_bytes(int64_t U, int32_t G, int64_t N, int32_t k, int32_t slab_rows, int64_t X);
int lthm_retrieve_topk_deep(const lthm_retrieve_desc* d, const lthm_retrieve_excl* x, const lthm_retrieve_group* g,
                            const lthm_retrieve_tags* t, const lthm_retrieve_cursor* c, const lthm_retrieve_bias* b,
                            void* stream);
/* Sharded catalogues: the rows of one catalogue held as S shards (on one device or on many), each
 * scanned on its own, the shards' lists merged.  A row's score is a function of (query, row,
 * prior) alone and ties break by item id, so the list over the union is the merge of the lists.
 *
 * lthm_retrieve_target_score: out[q] = the target_score that lthm_retrieve_topk_bias /
 * lthm_retrieve_topk_deep return for the same inputs, bit for bit (the plain f32 dot of the two
 * bf16 rows, the best over a group of G queries, then fmaf(weight[q], bias[target], .) where bias is
 * non-NULL; weight NULL is 1), from the same kernels, without a scan of the catalogue.  Where
 * target_row[q] is outside [0, N) it writes NaN ("this shard does not hold the target").
 *   q  f32 / bf16 [Q, 128], or [U, G, 128] with G >= 2 and Q = U; target_row int32 [Q]; out f32 [Q]
 *   workspace  lthm_retrieve_target_score_ws_bytes(Q, G) bytes, 16-byte aligned (-1 for Q < 1 or
 *              G outside 1..8) */
int64_t lthm_retrieve_target_score_ws_bytes(int64_t Q, int32_t G);
int lthm_retrieve_target_score(const void* items, int64_t N, const void* q, int32_t q_dtype, int32_t normalize_q,
                               int32_t G, const int32_t* target_row, const float* bias, const float* weight, float* out,
                               int64_t Q, void* workspace, int64_t ws_bytes, void* stream);
/* lthm_retrieve_topk_shard: one entry for k in 1..1024 (lthm_retrieve_topk_deep's dispatch and
 * workspace, lthm_retrieve_deep_ws_bytes).  s == NULL is exactly lthm_retrieve_topk_deep(d, x, g, t,
 * c, b, stream).  With s the target's score comes from the caller:
 *   target_score_in  f32 [Q] ([U] with groups), 4-byte aligned; NaN: the query has no target
 * d->target_score must be NULL and d->rank is required; d->target_row may be NULL or hold -1 where
 * this shard does not hold the target.  Nothing is read from items for the target, and
 *   rank[q] = #{j eligible, j != target_row[q] : s_j > target_score_in[q]},
 * or -1 where target_score_in[q] is NaN.  Eligible is what it is above: not excluded, passing the
 * tag filter, behind the cursor.  scores and rows are those of the call without s. */
typedef struct lthm_retrieve_shard {
  const float* target_score_in;
} lthm_retrieve_shard;
int lthm_retrieve_topk_shard(const lthm_retrieve_desc* d, const lthm_retrieve_excl* x, const lthm_retrieve_group* g,
                             const lthm_retrieve_tags* t, const lthm_retrieve_cursor* c, const lthm_retrieve_bias* b,
                             const lthm_retrieve_shard* s, void* stream);
/* lthm_retrieve_merge_shards: the k first entries of the union of S lists per query.
 *   scores  f32 [S, Q, k], ids int64 [S, Q, k]: list (s, q) sorted by (score descending, id
 *           ascending), its empty slots (-inf, 0) at the end; ids distinct across the lists of one
 *           query; no NaN; -0 equals +0 (it is returned as +0, as the scans return it)
 *   ranks   int32 [S, Q] or NULL
 *   out_scores f32 [Q, k], out_ids int64 [Q, k]: the union's first k in that order, then (-inf, 0)
 *   out_rank   int64 [Q] (with ranks): -1 if any of the query's S entries is -1, else their sum
 * 1 <= S <= 64, 1 <= k <= 1024.  Each entry is placed at its rank in the union (binary searches, no
 * sort and no atomics), so the outputs are a pure function of the inputs.  A pair that occurs in two
 * lists breaks the contract but not the call: both copies are returned, the lower list's first. */
int lthm_retrieve_merge_shards(const float* scores, const int64_t* ids, const int32_t* ranks, int32_t S, int64_t Q,
                               int32_t k, float* out_scores, int64_t* out_ids, int64_t* out_rank, void* stream);
/* Clustered catalogues (an inverted-file index): the catalogue's rows are grouped into L lists and a
 * query scans only the lists its probe row names.
 *   items     bf16 [N, 128], list-major: list c is rows [list_off[c], list_off[c + 1]), its ids ascending
 *   row_ids   int64 [N]: the item id of every row, distinct
 *   list_off  int64 [L + 1], ascending from 0 to N (an offset outside [0, N] is clamped, never followed)
 *   q         f32 / bf16 [Q, 128], prepared exactly as the entries above prepare it
 *   probes    int32 [Q, P], 1 <= P <= 64: the lists of query q; an entry outside [0, L) is ignored
 *             (-1 pads).  A list named twice in one row breaks the contract but not the call: the
 *             duplicate rule of lthm_retrieve_merge_shards applies
 *   x         NULL, or one list of excluded rows per query, in this catalogue's own (clustered) row
 *             numbering, under the rules of lthm_retrieve_topk_excl
 *   out_scores f32 [Q, k], out_ids int64 [Q, k], 1 <= k <= 128: the k first, under (score descending,
 *             id ascending), of the rows that lie in a probed list and are not excluded, then
 *             (-inf, 0).  A score is, bit for bit, the one lthm_retrieve_topk returns for the same
 *             (query, item row), wherever the row sits
 *   workspace lthm_retrieve_ivf_ws_bytes(Q, N, L, P, k, X) bytes (X = 0: no exclusion), 16-byte
 *             aligned; -1 for what the call refuses (Q, N or L outside 1..2^31-1, Q P >= 2^31, P
 *             outside 1..64, k outside 1..128, X outside 0..1024)
 * The call runs the query preparation, a plan (pairs counted and grouped by list on the device), one
 * scan in which each block serves up to 64 (query, probe) pairs of one list, and the merge of every
 * query's P lists, in sequence on `stream`, with no host synchronisation.  The scan's grid is
 * lthm_retrieve_ivf_grid(Q, P, L) = Q P / 64 + min(L, Q P), an upper bound on the tiles there can be;
 * the blocks past the true count exit at once.  The outputs are a pure function of the inputs. */
int64_t lthm_retrieve_ivf_grid(int64_t Q, int32_t P, int64_t L);
int64_t lthm_retrieve_ivf_ws_bytes(int64_t Q, int64_t N, int64_t L, int32_t P, int32_t k, int64_t X);
int lthm_retrieve_ivf_topk(const void* items, int64_t N, const int64_t* row_ids, const int64_t* list_off, int64_t L,
                           const void* q, int32_t q_dtype, int32_t normalize_q, int64_t Q, const int32_t* probes,
                           int32_t P, int32_t k, const lthm_retrieve_excl* x, float* out_scores, int64_t* out_ids,
                           void* workspace, int64_t ws_bytes, void* stream);
/* lthm_retrieve_ivf_topk_filt: lthm_retrieve_ivf_topk with tag filters, a score prior and a cursor per
 * query, each under the rules of the flat entries (lthm_retrieve_topk_tags / _bias / _after) and applied
 * in their order: the prior, then exclusion, the tag filter and the cursor.
 *   t   NULL, or tags int32 [N] in this catalogue's own (clustered) row numbering and filter int32
 *       [Q, 3] = (all, any, none); both non-null, 4-byte aligned; tags is never read at or past the end
 *       of a probed list (<= N).  An ineligible row takes no slot; (0, 0, 0) gives the rows of the call
 *       without tags and an unsatisfiable filter (all & none != 0) an empty list
 *   b   NULL, or bias f32 [N] in the clustered numbering (non-null, every value finite) and weight f32
 *       [Q] or NULL (1 for every query), 4-byte aligned: the score of a row is fmaf(weight[q], bias[row],
 *       dot) in f32, bit for bit the score lthm_retrieve_topk_bias returns for the same (query, item),
 *       and the order, the cursor and the scores written see that value only.  weight = 0 or an all-zero
 *       bias gives the rows of the call without a prior
 *   c   NULL, or a cursor per query: after_score f32 [Q] (4-byte aligned) and after_id int64 [Q] (8-byte
 *       aligned), both non-null.  An item with score s and id i is eligible iff s < after_score[q] or
 *       (s == after_score[q] and i > after_id[q]), in f32: -0 equals +0; +inf gives the rows of the call
 *       without a cursor; -inf or NaN admits nothing, so the (-inf, 0) tail of an exhausted page gives an
 *       empty page.  The cursor holds an id, not a row, since ids ascend with the rows inside a list only:
 *       the call turns it into one cursor row per (query, probed list) by a binary search over that
 *       list's row_ids, so after_id need not be an id of a probed list, nor of the catalogue.  With the
 *       same probes, a page's last (score, id) as the next call's cursor yields the following k items
 * The result is the k first, under (score descending, id ascending), of the rows that lie in a probed
 * list, are not excluded, pass the filter and lie strictly behind the cursor, then (-inf, 0); with
 * every list probed it is the flat entry's result for the same arguments.  t, b and c compose with x
 * and with each other.  With t, b and c all NULL the call is lthm_retrieve_ivf_topk: the same kernels
 * and the same bits.  Every pointer, alignment and range check is made before any launch.
 *   workspace lthm_retrieve_ivf_filt_ws_bytes(Q, N, L, P, k, X, has_cursor) bytes: has_cursor = 0 gives
 *             lthm_retrieve_ivf_ws_bytes(Q, N, L, P, k, X), has_cursor != 0 adds the Q P cursor rows; -1
 *             where that is -1
 * With c the call runs one more kernel ahead of the scan (one thread per pair); nothing else changes:
 * no host synchronisation, the same grid, and the outputs stay a pure function of the inputs. */
typedef struct lthm_retrieve_ivf_cursor {
  const float* after_score;
  const int64_t* after_id;
} lthm_retrieve_ivf_cursor;
int64_t lthm_retrieve_ivf_filt_ws_bytes(int64_t Q, int64_t N, int64_t L, int32_t P, int32_t k, int64_t X,
                                        int32_t has_cursor);
int lthm_retrieve_ivf_topk_filt(const void* items, int64_t N, const int64_t* row_ids, const int64_t* list_off,
                                int64_t L, const void* q, int32_t q_dtype, int32_t normalize_q, int64_t Q,
                                const int32_t* probes, int32_t P, int32_t k, const lthm_retrieve_excl* x,
                                const lthm_retrieve_tags* t, const lthm_retrieve_bias* b,
                                const lthm_retrieve_ivf_cursor* c, float* out_scores, int64_t* out_ids,
                                void* workspace, int64_t ws_bytes, void* stream);
/* lthm_retrieve_ivf_topk_group: lthm_retrieve_ivf_topk_filt, argument for argument, with users in place
 * of queries: user u has G queries (1 <= G <= 8, g->G; lthm_retrieve_group above) and an item is scored
 * by its best match over them, on the lists the user's one probe row names.
 *   q       f32 / bf16 [U, G, 128], contiguous, every row prepared as the entries above prepare it
 *   probes  int32 [U, P], 1 <= P <= 64: one probe row per user
 *   x->rows [U, X], t->filter [U, 3], b->weight [U] (or NULL), c->after_score / after_id [U] and
 *   out_scores f32 [U, k], out_ids int64 [U, k], 1 <= k <= 128: one per user
 *   s_g[u, j]  the f32 score, bit for bit, lthm_retrieve_topk gives query (u, g) against item row j
 *   s[u, j]    max_g s_g[u, j]; then, in the order lthm_retrieve_topk_group composed with _bias, _tags
 *              and _after applies them on the flat path: the prior, s = fmaf(weight[u], bias[j], s)
 *              (added behind the maximum, once); exclusion (a row of x is -inf); the tag filter (a row
 *              that fails it is -inf); the cursor (a row at or before (after_score, after_id) is -inf)
 * The result is, per user, the k first under (score descending, id ascending) of the rows that lie in a
 * probed list, are not excluded, pass the filter and lie strictly behind the cursor, then (-inf, 0).  The
 * maximum is taken inside the scan, ahead of candidate selection, so an item takes ONE slot per user
 * however many of the user's queries it matches, and the outputs do not depend on the order of a
 * user's queries.  With every list probed the result is, bit for bit, what lthm_retrieve_topk_group
 * composed with the same x, t, b and c returns (rows given as ids).  g == NULL or g->G == 1 IS
 * lthm_retrieve_ivf_topk_filt: the same kernels, the same workspace size and the same bits.  Deep lists
 * (k > 128) with groups are refused.  Every pointer, alignment, range and workspace check is made before
 * any launch; the call runs on `stream` without a host synchronisation and the outputs are a pure
 * function of the inputs.
 *   workspace lthm_retrieve_ivf_group_ws_bytes(U, G, N, L, P, k, X, has_cursor) bytes, 16-byte aligned: at
 *             G = 1 lthm_retrieve_ivf_filt_ws_bytes(U, N, L, P, k, X, has_cursor); above, the U G prepared
 *             queries and the larger tile table in place of theirs; -1 for what the call refuses (G outside
 *             1..8, U G >= 2^31, and whatever the _filt size refuses)
 * The scan: a (user, probe) pair takes G adjacent MFMA columns of one row of 16 columns, so a block serves
 * up to T(G) = 4 floor(16 / G) pairs of one list (64, 32, 20, 16, 12, 8, 8, 8 for G = 1..8); the columns
 * left over hold no query and never reach selection.  Its grid is
 * lthm_retrieve_ivf_group_grid(U, G, P, L) = U P / T(G) + min(L, U P), an upper bound on the tiles there
 * can be (sum_c ceil(n_c / T) over the lists' pair counts n_c, sum_c n_c <= U P), as
 * lthm_retrieve_ivf_grid is for G = 1, whose value it has there; the blocks past the true count exit at
 * once.  -1 for U, P or L < 1, U or L >= 2^31, G outside 1..8. */
int64_t lthm_retrieve_ivf_group_grid(int64_t U, int32_t G, int32_t P, int64_t L);
int64_t lthm_retrieve_ivf_group_ws_bytes(int64_t U, int32_t G, int64_t N, int64_t L, int32_t P, int32_t k, int64_t X,
                                         int32_t has_cursor);
int lthm_retrieve_ivf_topk_group(const void* items, int64_t N, const int64_t* row_ids, const int64_t* list_off,
                                 int64_t L, const void* q, int32_t q_dtype, int32_t normalize_q, int64_t U,
                                 const lthm_retrieve_group* g, const int32_t* probes, int32_t P, int32_t k,
                                 const lthm_retrieve_excl* x, const lthm_retrieve_tags* t,
                                 const lthm_retrieve_bias* b, const lthm_retrieve_ivf_cursor* c, float* out_scores,
                                 int64_t* out_ids, void* workspace, int64_t ws_bytes, void* stream);
/* lthm_retrieve_ivf_topk_deep: lthm_retrieve_ivf_topk_filt, argument for argument, with 1 <= k <= 1024:
 * the lists a ranking stage or lthm_retrieve_diversify's pool take, from the probed lists alone.  The
 * contract is lthm_retrieve_ivf_topk_filt's with that k: the k first, under (score descending, id
 * ascending), of the rows that lie in a probed list, are not excluded, pass the filter and lie strictly
 * behind the cursor, then (-inf, 0); every score has the bits lthm_retrieve_topk_deep returns for the
 * same (query, item, weight), and with every list probed the result is that entry's.  A list named
 * twice in a probe row gives both copies.  With k <= 128 the call IS lthm_retrieve_ivf_topk_filt: the
 * same kernels, the same workspace and the same bits.  Above, the scan keeps every (query, probe)
 * pair's candidates in 2,048 key slots of the workspace (16 KiB per pair) instead of LDS and sorts
 * them there; the plan, the grid and the merge are unchanged, nothing synchronises with the host and
 * the outputs stay a pure function of the inputs.  Every pointer, alignment, range and workspace check
 * is made before any launch.  Every other clustered entry keeps refusing k > 128.
 *   workspace lthm_retrieve_ivf_deep_ws_bytes(Q, N, L, P, k, X, has_cursor) bytes, 16-byte aligned:
 *             lthm_retrieve_ivf_filt_ws_bytes(...) for k <= 128; above, that layout at k plus Q P 16 KiB
 *             (a caller with many queries splits them: a query's result does not depend on the
 *             others); -1 for k outside 1..1024 and wherever the _filt size is -1 for another reason */
int64_t lthm_retrieve_ivf_deep_ws_bytes(int64_t Q, int64_t N, int64_t L, int32_t P, int32_t k, int64_t X,
                                        int32_t has_cursor);
int lthm_retrieve_ivf_topk_deep(const void* items, int64_t N, const int64_t* row_ids, const int64_t* list_off,
                                int64_t L, const void* q, int32_t q_dtype, int32_t normalize_q, int64_t Q,
                                const int32_t* probes, int32_t P, int32_t k, const lthm_retrieve_excl* x,
                                const lthm_retrieve_tags* t, const lthm_retrieve_bias* b,
                                const lthm_retrieve_ivf_cursor* c, float* out_scores, int64_t* out_ids,
                                void* workspace, int64_t ws_bytes, void* stream);
/* lthm_retrieve_ivf_topk_shards: S clustered catalogues on one device (1 <= S <= 64), each with tensors,
 * centroids and a number of lists of its own and with ids no other shard holds, answer one batch of
 * queries in one call.  Shard s probes its P_s = min(nprobe, L_s) nearest lists per query (the probe row
 * lthm_retrieve_topk gives over its centroids: ties go to the lower list); sum_s P_s <= 64.  The result
 * is the k first, under (score descending, id ascending), of the rows of all probed lists that are
 * eligible under lthm_retrieve_ivf_topk_deep's rules, then (-inf, 0): bit for bit what S calls of
 * lthm_retrieve_ivf_topk_deep (one per shard, with that shard's probe row) followed by
 * lthm_retrieve_merge_shards return, from one plan, one scan launch and one merge.  1 <= k <= 1024.
 *   shards        host array [S]; items bf16 [N, 128] list-major, row_ids int64 [N], list_off int64
 *                 [L + 1], centroids bf16 [L, 128], tags int32 [N] / bias f32 [N] in the rows' order or
 *                 NULL, all device pointers
 *   exclude_rows  int32 [S, Q, X] (X in 1..1024) or NULL with X = 0: the excluded rows of every query in
 *                 every shard's own numbering, entries outside [0, N_s) ignored
 *   tag_filter    int32 [Q, 3] or NULL; with it every shard must carry tags
 *   use_bias      != 0: every shard must carry a bias, and the score is fmaf(w[q], bias[row], dot) with
 *                 bias_weight f32 [Q] or NULL (1 for every query); 0: the plain dot, bias_weight NULL
 *   c             the (score, id) cursor of every query, or NULL
 *   target_rows   int32 [S, Q], target_score f32 [Q] and out_rank int64 [Q], all three or none: the row
 *                 of every query's target in every shard (-1: not there) and the target's score (from
 *                 lthm_retrieve_target_score on the shard that holds it; NaN: no shard does).  out_rank
 *                 is the number of eligible rows of the probed lists, other than the target's, that score
 *                 strictly above target_score (0 for a NaN score: the caller knows no shard holds it)
 *   workspace     lthm_retrieve_ivf_shards_ws_bytes(shards, S, Q, nprobe, k, X, has_cursor) bytes, 256-byte
 *                 aligned; -1 for sizes the call refuses (sum_s P_s > 64 among them)
 * Every pointer, alignment, range and workspace check is made before any launch; nothing synchronises
 * with the host and the outputs are a pure function of the inputs. */
typedef struct lthm_retrieve_ivf_shard {
  const void* items;
  const int64_t* row_ids;
  const int64_t* list_off;
  const void* centroids;
  const int32_t* tags;
  const float* bias;
  int64_t N;
  int64_t L;
} lthm_retrieve_ivf_shard;
int64_t lthm_retrieve_ivf_shards_ws_bytes(const lthm_retrieve_ivf_shard* shards, int32_t S, int64_t Q, int32_t nprobe,
                                          int32_t k, int64_t X, int32_t has_cursor);
int lthm_retrieve_ivf_topk_shards(const lthm_retrieve_ivf_shard* shards, int32_t S, const void* q, int32_t q_dtype,
                                  int32_t normalize_q, int64_t Q, int32_t nprobe, int32_t k,
                                  const int32_t* exclude_rows, int64_t X, const int32_t* tag_filter, int32_t use_bias,
                                  const float* bias_weight, const lthm_retrieve_ivf_cursor* c,
                                  const int32_t* target_rows, const float* target_score, float* out_scores,
                                  int64_t* out_ids, int64_t* out_rank, void* workspace, int64_t ws_bytes, void* stream);
/* Diversified lists: greedy maximal-marginal-relevance (MMR) selection of k out of a pool of M
 * candidates per query, with an optional cap on the selected items of one group.  The pool is a list
 * any of the calls above returned (lthm_retrieve_topk_deep gives up to 1,024 rows in one scan).
 *   items    bf16 [N, 128], 16-byte aligned: the flat catalogue the pool's rows index
 *   rows     int32 [Q, M], scores f32 [Q, M], 1 <= M <= 1024, in any order.  An entry whose row is
 *            outside [0, N), or whose score is -inf or NaN, is no candidate.  A query's rows are
 *            distinct; a row named twice breaks the contract but not the call: it is two candidates,
 *            the one at the lower pool position first where everything else ties
 *   k        1..128
 *   lam      f32 [Q], in [0, 1], or NULL: 1 for every query
 *   groups   int32 [N] or NULL: one key per catalogue row, 0 = no group (never capped); cap >= 1 is
 *            the most selected items of one non-zero key (ignored without groups)
 * Per query, with S empty and d_i = 0 for every candidate, k times: among the candidates not yet
 * selected whose key is 0 or shared by fewer than cap selected items, select the first under
 * (m descending, row ascending), where
 *   m_i = fmaf(-(1.0f - lam), d_i, lam * s_i)            (f32, exactly these operations)
 * and the order is the one integer order of every list here (-0 equals +0); then d_i = fmaxf(d_i,
 * g_ij) for every candidate, g_ij the f32 dot of the bf16 rows i and j (its summation order is not
 * part of the contract: exact for integer-valued rows, within 128 2^-24 sum|a b| otherwise).  If no
 * candidate is eligible the rest of the list is empty.
 *   out_rows   int32 [Q, k]: the selected rows in selection order, then -1
 *   out_scores f32 [Q, k]: the caller's score of the selected row, its bits unchanged, then -inf
 *   out_obj    f32 [Q, k]: m at the moment of selection, then -inf
 *   workspace  lthm_retrieve_diversify_ws_bytes(Q, M, k) bytes, 16-byte aligned: 0 for every size the
 *              call takes (the candidates' rows live in registers; workspace may then be NULL), -1
 *              for Q outside 1..2^31-1, M outside 1..1024, k outside 1..128
 * With lam = 1 and no groups m_i = s_i, so the result is the first k of the pool under (score
 * descending, row ascending) whatever order the pool came in.  One block per query, no atomics: every
 * output is a pure function of the inputs.  Scores are finite or -inf / NaN (+inf is memory-safe, its
 * objective may be NaN). */
int64_t lthm_retrieve_diversify_ws_bytes(int64_t Q, int64_t M, int32_t k);
int lthm_retrieve_diversify(const void* items, int64_t N, const int32_t* rows, const float* scores, int64_t Q, int32_t M,
                            int32_t k, const float* lam, const int32_t* groups, int32_t cap, int32_t* out_rows,
                            float* out_scores, float* out_obj, void* workspace, int64_t ws_bytes, void* stream);
/* e4m3 catalogues: a cheap approximate scan for a shortlist, then exact scores for the shortlist.
 * Quantiser: a bf16 row x[0..127] with a = max |x_k| becomes 128 OCP e4m3fn codes and one f32
 * scale.  e = 0 for a = 0, otherwise the largest integer with a 2^e <= 448, clamped to [-64, 64];
 * code_k = the round-to-nearest-even, saturating e4m3fn conversion of the (exact) f32 product
 * x_k 2^e; scale = 2^-e; the row stands for code_k scale.  On the CPU this is
 * (x.float() * 2.0**e).to(torch.float8_e4m3fn), and the device equals it bit for bit.  A row with
 * a non-finite element gets unspecified codes.
 *   items  bf16 [N, 128], 16-byte aligned; codes uint8 [N, 128], 16-byte aligned; scale f32 [N] */
int lthm_catalogue_quantize_q8(const void* items, int64_t N, uint8_t* codes, float* scale, void* stream);
/* The shortlist: the M first rows (1 <= M <= 1024) under (s^ descending, row ascending), where
 *   s^[q, j] = acc (scale_q scale_j),  acc = the f32 MFMA accumulation of cq_k c_jk from zero,
 * and (cq, scale_q) is the quantiser applied to the bf16 row that lthm_retrieve_topk forms from q
 * (normalize_q included).  Both multiplies are explicit f32 operations by powers of two.  x may be
 * NULL; otherwise it follows lthm_retrieve_topk_excl's rules (an excluded row scores -inf).  Where
 * fewer than M rows are eligible the tail is -inf / -1.  The outputs are a pure function of the
 * inputs: no global atomics, no dependence on slab_rows (a multiple of 64, or 0), Q or slot order.
 *   workspace  lthm_retrieve_q8_ws_bytes(Q, N, M, slab_rows, X) bytes (X = 0: no list), 16-byte
 *              aligned; -1 for M outside 1..1024, X outside 0..1024, slab_rows that is no multiple
 *              of 64, and Q or N outside 1..2^31-1 */
int64_t lthm_retrieve_q8_ws_bytes(int64_t Q, int64_t N, int32_t M, int32_t slab_rows, int64_t X);
int lthm_retrieve_q8_topk(const uint8_t* codes, const float* scale, int64_t N, const void* q, int32_t q_dtype,
                          int32_t normalize_q, int64_t Q, int32_t M, int32_t slab_rows, const lthm_retrieve_excl* x,
                          float* out_scores, int32_t* out_rows, void* workspace, int64_t ws_bytes, void* stream);
/* Re-scoring: rows int32 [Q, M] (1 <= M <= 1024, any order) names catalogue rows per query.  Every
 * entry in [0, N) gets the score whose f32 bits lthm_retrieve_topk returns for that (query, row);
 * an entry outside [0, N) is no candidate; a row named twice appears twice.  out_scores / out_rows
 * [Q, k], 1 <= k <= M: the k first under (score descending, row ascending), then -inf / -1.
 *   workspace  lthm_retrieve_rescore_ws_bytes(Q, M, k) bytes, 16-byte aligned; -1 for Q outside
 *              1..2^31-1, M outside 1..1024, k outside 1..M */
int64_t lthm_retrieve_rescore_ws_bytes(int64_t Q, int32_t M, int32_t k);
int lthm_retrieve_rescore(const void* items, int64_t N, const void* q, int32_t q_dtype, int32_t normalize_q, int64_t Q,
                          const int32_t* rows, int32_t M, int32_t k, float* out_scores, int32_t* out_rows,
                          void* workspace, int64_t ws_bytes, void* stream);
/* lthm_retrieve_rescore with a prior and an id order: a listed row's score is fmaf(weight[q],
 * bias[row], dot), dot the bits lthm_retrieve_rescore returns, one explicit f32 fma as
 * lthm_retrieve_topk_bias does on its score (weight NULL: 1 for every query).  order_ids int64 [N] or
 * NULL: with it the list comes out under (score descending, order_ids[row] ascending), the order of
 * the clustered calls, whose rows do not ascend with their ids across lists; without it under (score
 * descending, row ascending).  With bias == NULL and order_ids == NULL the call IS
 * lthm_retrieve_rescore: the same kernel body, the same bits.  weight without bias is refused.  The
 * workspace is lthm_retrieve_rescore_ws_bytes(Q, M, k). */
int lthm_retrieve_rescore_bias(const void* items, int64_t N, const void* q, int32_t q_dtype, int32_t normalize_q,
                               int64_t Q, const int32_t* rows, int32_t M, int32_t k, const float* bias,
                               const float* weight, const int64_t* order_ids, float* out_scores, int32_t* out_rows,
                               void* workspace, int64_t ws_bytes, void* stream);
/* Clustered e4m3 catalogues: lthm_retrieve_q8_topk's shortlist from the probed lists alone, with
 * lthm_retrieve_ivf_topk_deep's eligibility.  codes uint8 [N, 128] / scale f32 [N] are
 * lthm_catalogue_quantize_q8 of the list-major rows; row_ids, list_off, probes, x, t and b are
 * lthm_retrieve_ivf_topk_deep's (rows, tags and bias in the clustered numbering).
 *   s^[q, j] = acc (scale_q scale_j), lthm_retrieve_q8_topk's score bit for bit (the same query
 *              preparation and quantiser, the same eight bf16 MFMA steps from zero, two explicit f32
 *              multiplies); with b the ranked score is fmaf(weight[q], bias[j], s^), one explicit fma
 *              under lthm_retrieve_topk_bias' rules (a non-finite weight gives that query an
 *              unspecified list and harms nothing else)
 *   a row is a candidate of query q iff it lies in a list of probes[q, 0..P) (entries outside [0, L)
 *              are ignored, an empty list contributes nothing, a list named twice gives both copies),
 *              is not excluded (x) and passes the query's (all, any, none) filter (t)
 *   out_scores f32 [Q, M] / out_rows int32 [Q, M] (clustered rows), 1 <= M <= 1024: the M first
 *              candidates under (score descending, id ascending), lthm_retrieve_ivf_topk_deep's
 *              total order, then -inf / -1
 * A pure function of the inputs: no output depends on Q, on the order of a probe row, on how lists
 * map to blocks or on slot order (the plan's two integer atomics decide only which block column
 * serves a pair).  Every pointer, alignment, range and workspace check is made before any launch.
 *   workspace  lthm_retrieve_ivf_q8_ws_bytes(Q, N, L, P, M, X) bytes, 16-byte aligned:
 *              lthm_retrieve_ivf_deep_ws_bytes' layout at k = M with the key slots (Q P 16 KiB)
 *              whatever M is, plus the queries' codes and scales (Q 132 B, rounded) and the merged
 *              ids (Q M 8 B); -1 for M outside 1..1024, X outside 0..1024, P outside 1..64, and Q,
 *              N, L or Q P outside 1..2^31-1 */
int64_t lthm_retrieve_ivf_q8_ws_bytes(int64_t Q, int64_t N, int64_t L, int32_t P, int32_t M, int64_t X);
int lthm_retrieve_ivf_q8_topk(const uint8_t* codes, const float* scale, int64_t N, const int64_t* row_ids,
                              const int64_t* list_off, int64_t L, const void* q, int32_t q_dtype,
                              int32_t normalize_q, int64_t Q, const int32_t* probes, int32_t P, int32_t M,
                              const lthm_retrieve_excl* x, const lthm_retrieve_tags* t,
                              const lthm_retrieve_bias* b, float* out_scores, int32_t* out_rows, void* workspace,
                              int64_t ws_bytes, void* stream);
/* Catalogue updates: the list-major catalogue that remains when some old rows are dropped and delta
 * rows are merged in, list by list, every list's ids still ascending (csrc/catalogue_update.hip).  A
 * flat, id-ascending catalogue is the case L = 1.  Nothing is sorted and no output is written through
 * an atomic: every output row is written once, from the one source row that binary searches find, so
 * two calls give the same bytes.
 *   N, M, L       old rows (>= 1), delta rows (>= 0), lists (1..2^30); N + M <= 2^31 - 2
 *   N_out         the rows of the output tensors: (the old rows with dead == 0) + M, which the caller
 *                 reads once from the device; the call writes no row at or beyond it
 *   old_ids       int64 [N]; old_emb bf16 [N, 128], 16-byte aligned; old_tags int32 [N], old_bias f32 [N]
 *                 and old_groups int32 [N], each or NULL: the columns, list-major
 *   old_off       int64 [L + 1]: list c is old rows old_off[c] .. old_off[c + 1], its ids ascending
 *                 (compared as signed int64)
 *   dead          uint8 [N]: != 0 for an old row that is removed or replaced.  The call sums the flag
 *                 itself: live_before[p], the rows before p with dead == 0, int32 [N + 1] in the workspace
 *   delta_*       the M delta rows in (list, id) order, with exactly the optional columns the old rows
 *                 carry; delta_off int64 [L + 1] their lists.  No delta id equals a surviving id of
 *                 its list.  With M = 0 the column pointers may be NULL (delta_off still holds L + 1 zeros)
 *   out_*         the N_out output rows and out_off int64 [L + 1], all written by the call:
 *                 out_off[c] = live_before[old_off[c]] + delta_off[c]
 *   workspace     lthm_catalogue_update_ws_bytes(N, M, L) bytes, 16-byte aligned (live_before, the chunk
 *                 table and the delta rows' destinations); -1 for N, M or L outside the ranges above
 * The output is cut into chunks of LTHM_CATALOGUE_UPDATE_CHUNK rows of one list, listed in a table
 * that is built on the device, so the call reads no list length on the host and nothing synchronises.
 * Pointer, alignment, range and workspace checks are made before any launch; offsets on the device that
 * break the contract give wrong rows, never an access outside the tensors. */
#define LTHM_CATALOGUE_UPDATE_CHUNK 256
typedef struct lthm_catalogue_update_desc {
  int64_t N;
  int64_t M;
  int64_t L;
  int64_t N_out;
  const int64_t* old_ids;
  const void* old_emb;
  const int32_t* old_tags;
  const float* old_bias;
  const int32_t* old_groups;
  const int64_t* old_off;
  const uint8_t* dead;
  const int64_t* delta_ids;
  const void* delta_emb;
  const int32_t* delta_tags;
  const float* delta_bias;
  const int32_t* delta_groups;
  const int64_t* delta_off;
  int64_t* out_ids;
  void* out_emb;
  int32_t* out_tags;
  float* out_bias;
  int32_t* out_groups;
  int64_t* out_off;
  void* workspace;
  int64_t ws_bytes;
} lthm_catalogue_update_desc;
int64_t lthm_catalogue_update_ws_bytes(int64_t N, int64_t M, int64_t L);
int lthm_catalogue_update(const lthm_catalogue_update_desc* d, void* stream);

/* ------------------------------------------------------------------------- */
/* Ranking stage — the plumbing around the ranker's forward (csrc/rank.hip)  */
/* ------------------------------------------------------------------------- */
/* The longest candidate list of the two calls below: the k = 1,024 of the deep retrieval lists. */
#define LTHM_RANK_MAX_LIST 1024
/* lthm_rank_assemble: the ranker's input batch of Q users x M candidates each, in one pass.
 *   out_dense[q M + m] = [ user_dense[q] | item_dense[rows[q, m]] ]   f32   [Q M, Du + Di]
 *   out_cat  [q M + m] = [ user_cat[q]   | item_cat[rows[q, m]]   ]   int64 [Q M, Fu + Fi]
 *   Q, M          users (>= 1) and candidates per user (1..LTHM_RANK_MAX_LIST); Q M <= 2^31 - 1
 *   N             rows of the item matrices (0..2^31 - 1)
 *   Du, Di, Fu, Fi  the widths, each >= 0; Du + Di and Fu + Fi at most 2^20.  A matrix of width 0 is
 *                 not read and its pointer may be NULL
 *   rows          int32 [Q, M]: a row of the item matrices; an index outside [0, N) is a pad: it is
 *                 never followed, and its item columns are written as 0.0 and 0
 * Every output element is written exactly once, by plain stores; the values are copies, bit for bit.
 * Odd widths are not refused: a matrix moves in 16-byte units when both of its widths allow it (Du and
 * Di multiples of 4; Fu and Fi multiples of 2) and its three pointers must then be 16-byte aligned;
 * otherwise it moves element by element and the pointers need the element's alignment (4 / 8 bytes).
 * NULL pointers, negative sizes, M outside its range and misaligned pointers are refused before any
 * launch. */
typedef struct lthm_rank_assemble_desc {
  int64_t Q;
  int64_t M;
  int64_t N;
  int64_t Du;
  int64_t Di;
  int64_t Fu;
  int64_t Fi;
  const float* user_dense;
  const int64_t* user_cat;
  const float* item_dense;
  const int64_t* item_cat;
  const int32_t* rows;
  float* out_dense;
  int64_t* out_cat;
} lthm_rank_assemble_desc;
int lthm_rank_assemble(const lthm_rank_assemble_desc* d, void* stream);
/* lthm_rank_sort: every list of M (logit, row) entries in its total order, the first k of it.
 *   logits f32 [Q, M], rows int32 [Q, M], 1 <= k <= M <= LTHM_RANK_MAX_LIST, 1 <= Q <= 2^31 - 1
 *   out_scores f32 [Q, k], out_rows int32 [Q, k], out_src int32 [Q, k]: the logit as it came in, its
 *   row, and the position m it had in the list
 * An entry is a candidate when its row is >= 0 and its logit is not NaN; -inf and +inf are ordinary
 * values and -0.0 orders as +0.0.  The candidates come in the order (logit descending, row ascending,
 * position ascending), so a row that appears twice keeps both copies in input order; the slots behind
 * the last candidate hold (-inf, -1, -1).  One block per list, the keys in LDS, no workspace and no
 * atomics: the result is a pure function of the inputs. */
int lthm_rank_sort(const float* logits, const int32_t* rows, int64_t Q, int32_t M, int32_t k, float* out_scores,
                   int32_t* out_rows, int32_t* out_src, void* stream);

/* ------------------------------------------------------------------------- */
/* Id ingest — commons/feature_utils.py (host CPU unless noted)              */
/* ------------------------------------------------------------------------- */
/* xxHash32 / xxHash64 of a byte string (python-xxhash intdigest()) */
uint32_t lthm_xxh32(const void* data, int64_t len, uint32_t seed);
uint64_t lthm_xxh64(const void* data, int64_t len, uint64_t seed);
/* hash_string_to_long (feature_utils.py:40-46) over n packed UTF-8 strings
 * bytes[offsets[i] .. offsets[i+1]): out[i] = xxh64(s_i, seed) - 2^63.  With
 * to_lower, ASCII letters are lowered here; strings holding non-ASCII bytes are
 * flagged in needs_unicode_lower[i] (may be NULL) and left for the caller
 * (Python str.lower()).  Returns the number flagged, or -1 on bad arguments. */
int64_t lthm_hash_strings(const uint8_t* bytes, const int64_t* offsets, int64_t n, uint64_t seed, int32_t to_lower,
                          int64_t* out, uint8_t* needs_unicode_lower);
/* hash_string_to_long(str(v), seed) for int64 values v (decimal str(), no lowering) */
int lthm_hash_int64_str(const int64_t* vals, int64_t n, uint64_t seed, int64_t* out);
/* the same on the GPU: device pointers, stream-ordered */
int lthm_hash_int64_str_dev(const int64_t* vals, int64_t n, uint64_t seed, int64_t* out, void* stream);
/* handle_categorical_history_feature / pad_array (feature_utils.py:21-25, 149-183):
 * row r = items[row_offsets[r] .. row_offsets[r+1]) (already hashed), optionally
 * dropping entries equal to history_id[r], capped to `length`, right-padded with
 * `pad` -> out [n_rows, length]. */
int lthm_history_pad(const int64_t* items, const int64_t* row_offsets, int64_t n_rows, const int64_t* history_id,
                     int32_t remove_history_id, int32_t length, int64_t pad, int64_t* out);

#ifdef __cplusplus
}
#endif
#endif /* LTHM_H_ */
