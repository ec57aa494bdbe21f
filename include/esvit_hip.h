/* libesvit_hip.so -- C ABI of the MI355X-native EsViT pre-training hot path.
 *
 * Every entry point replaces a stretch of the reference's PyTorch code (cited per
 * function as reference file:line, paths relative to microsoft/esvit).  Conventions
 * (SURVEY.md 8b):
 *   - all buffers are caller-allocated DEVICE memory passed as raw pointers; the
 *     library never allocates, frees or retains device memory;
 *   - all work is enqueued on the caller's hipStream_t; no internal synchronisation;
 *   - return 0 on success, negative on failure (ESVIT_ERR_*); the message is
 *     available through esvit_last_error(); no C++ exception crosses the ABI;
 *   - `dtype` selects the storage type of *activations* (ESVIT_F32 / ESVIT_BF16);
 *     parameters, the residual stream, statistics and gradients of parameters are
 *     always fp32.
 */
#ifndef ESVIT_HIP_H
#define ESVIT_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default) /* the library is built with -fvisibility=hidden: this header IS the export list */

#define ESVIT_F32 0
#define ESVIT_BF16 1

#define ESVIT_OK 0
#define ESVIT_ERR_ARG (-1)
#define ESVIT_ERR_HIP (-2)
#define ESVIT_ERR_UNSUPPORTED (-3)

typedef void* esvit_stream_t; /* hipStream_t */

/* ---- library ---------------------------------------------------------- */
int esvit_version(void);
const char* esvit_last_error(void);
/* Sizes of caller-allocated scratch / capability questions, one entry point (no device work, no state):
 *   ESVIT_Q_ATTN_FRAG_ELEMS (N)                floats per N x N matrix in MFMA fragment order (4096 for N <= 64), -1 unsupported
 *   ESVIT_Q_ATTN_LSE_ELEMS (N)                 per-(window, head) log-sum-exp floats the forward writes (0 for N <= 64)
 *   ESVIT_Q_ATTN_BWD_PARTS (N, Bw, nH)         leading dimension of dbias_ws of esvit_window_attn_bwd
 *   ESVIT_Q_ATTN_BWD_PAD_ROWS (N, Bw, nH | dtype << 32)  rows of dpad_ws of esvit_window_attn_bwd
 *   ESVIT_Q_LN_BWD_BLOCKS (rows, C)            nblk of the [nblk, 2, C] LayerNorm-backward scratch
 *   ESVIT_Q_COLSUM_BLOCKS (rows)               blocks of the esvit_colsum scratch
 *   ESVIT_Q_COL_REDUCE_BLOCKS (rows)           blocks of the esvit_dwconv3x3_wgrad / esvit_col_sums2 scratch
 *   ESVIT_Q_UPDATE_CHUNK_ELEMS ()              elements per chunk of the fused update's chunk table
 *   ESVIT_Q_MLP_FUSED (dtype, C)               bit 0: esvit_mlp_fused_fwd exists (bf16, C in {96, 128, 192, 256, 384}), bit 1: esvit_mlp_fused_bwd exists (bf16, C in {96, 128, 192, 256})
 *   ESVIT_Q_AUG_MAX_BOX (S)                    largest crop-box side esvit_aug_crops resizes to S x S
 *   ESVIT_Q_JPEG_WORKSPACE (n_blocks, plane_bytes, n_lanes | n_segments << 32)  bytes of the esvit_jpeg_decode workspace
 *   ESVIT_Q_RESIZE_FITS (scale_h, scale_w)     1 if esvit_aug_crops' evaluation mode takes a call whose largest per-axis scales
 *                                              are scale_h, scale_w (units of 1 / ESVIT_RESIZE_SCALE_ONE), else 0
 *   ESVIT_Q_CHUNK_ATTN_WS (nB*nH, L, backward) floats of the scratch the sliding-chunk mode of esvit_window_attn_fwd (backward = 0) /
 *                                              esvit_window_attn_bwd (backward = 1) takes through bias_frag_ws
 *   ESVIT_Q_TOPK_WS (M, N, k)                  BYTES of esvit_gemm_topk::workspace for M test rows scored against N train rows at this k
 *                                              (per-(row, split) candidate lists; grows with M, k and the split count, and no longer
 *                                              with N once the splits saturate), ESVIT_ERR_ARG for k outside 1 .. 256
 *   ESVIT_Q_PROBE_CE_REG_ROW ()                longest row (floats) the class-index mode of esvit_dino_ce_fwd_bwd keeps in registers (one wave
 *                                              per row); longer rows take one workgroup per row and three sweeps
 *   ESVIT_Q_GLOBAL_ATTN_WS (nB*nH, L, backward) floats of the scratch the global mode of esvit_window_attn_fwd (backward = 0: none) /
 *                                              esvit_window_attn_bwd (backward = 1) takes through bias_frag_ws; linear in L
 *   ESVIT_Q_MLP_DW_WS (dtype, C, M)            BYTES of partials_ws of esvit_mlp_fused_bwd's on-chip weight-gradient mode for M rows: one partial of
 *                                              ESVIT_MLP_DW_PARTIAL_FLOATS floats per workgroup of the launch (one per CU, at most one per 64 rows);
 *                                              0 where the mode does not exist (anything but bf16, C = 96)
 * Unknown `what` returns ESVIT_ERR_ARG. */
#define ESVIT_Q_ATTN_FRAG_ELEMS 1
#define ESVIT_Q_ATTN_LSE_ELEMS 2
#define ESVIT_Q_ATTN_BWD_PARTS 3
#define ESVIT_Q_ATTN_BWD_PAD_ROWS 4
#define ESVIT_Q_LN_BWD_BLOCKS 5
#define ESVIT_Q_COLSUM_BLOCKS 6
#define ESVIT_Q_COL_REDUCE_BLOCKS 7
#define ESVIT_Q_UPDATE_CHUNK_ELEMS 8
#define ESVIT_Q_MLP_FUSED 9
#define ESVIT_Q_AUG_MAX_BOX 10
#define ESVIT_Q_JPEG_WORKSPACE 11
#define ESVIT_Q_RESIZE_FITS 12
#define ESVIT_Q_CHUNK_ATTN_WS 13
#define ESVIT_Q_TOPK_WS 14
#define ESVIT_Q_PROBE_CE_REG_ROW 15
#define ESVIT_Q_GLOBAL_ATTN_WS 16
#define ESVIT_Q_MLP_DW_WS 17
#define ESVIT_MLP_DW_PARTIAL_FLOATS 74208 /* dW2 96 x 384 + G 384 x 96 + db1 384 + db2 96 */
/*   ESVIT_Q_ATTN_BWD_FUSED_GRID (dtype, C, windows)  workgroups of one launch of the backward mode of the fused attention branch over `windows`
 *                                              windows (= partials and bias-gradient slabs it writes; one per CU, at most one per window); 0 where
 *                                              the mode does not exist (anything but bf16, C = 96).  Needs no device (then: the size of an MI355X) */
#define ESVIT_Q_ATTN_BWD_FUSED_GRID 18
#define ESVIT_ATTN_BWD_PARTIAL_FLOATS 37440 /* dWqkv 288 x 96 + dWproj 96 x 96 + dbqkv 288 + dbproj 96 + dgamma 96 + dbeta 96 */
/*   ESVIT_Q_PATCH_EMBED_WS (dtype, E, rows)    BYTES of partial records one backward launch of the fused patch embedding (the fused mode of
 *                                              esvit_patch_im2col) writes for `rows` token rows: 51 E floats per workgroup (one per CU, at most
 *                                              one per 128 rows); 0 where the mode does not exist (anything but bf16, E in {96, 128, 192}).
 *                                              Needs no device (then: the size of an MI355X) */
#define ESVIT_Q_PATCH_EMBED_WS 19
/*   ESVIT_Q_DIST_STATS (R, K)                  the row-statistics mode of esvit_dino_ce_fwd_bwd (terms = -1).  R = 0: the slab height, the rows one
 *                                              workgroup owns (32).  R > 0: FLOATS of the buffer the mode takes through `ds` for R rows of K
 *                                              columns: K column sums, one partial of K floats per slab, one record of 4 floats per row and
 *                                              block of 65536 columns: (1 + ceil(R / slab)) K + 4 R ceil(K / 65536) */
#define ESVIT_Q_DIST_STATS 20
/*   ESVIT_Q_ATTN_TAIL_WS (dtype, C, M)         BYTES of the partial records of esvit_layernorm_bwd's qkv-tail mode for M rows: one partial of
 *                                              ESVIT_ATTN_TAIL_PARTIAL_FLOATS floats per workgroup of the launch (one per CU, at most one per
 *                                              64 rows); 0 where the mode does not exist (anything but bf16, C = 96).  Needs no device (then:
 *                                              the size of an MI355X) */
#define ESVIT_Q_ATTN_TAIL_WS 21
#define ESVIT_ATTN_TAIL_PARTIAL_FLOATS 28128 /* dWqkv 288 x 96 + dbqkv 288 + dgamma 96 + dbeta 96 */
int64_t esvit_query(int what, int64_t a, int64_t b, int64_t c);

/* ---- host-side integer index maps (bit-exact vs reference) -------------
 * swin_transformer.py:100-110 (relative_position_index), :40-69 + :286-325
 * (pad -> roll -> window_partition and its inverse), :249-272 (shift mask).  */
/* out[N*N], N = ws*ws */
int esvit_relative_position_index(int ws, int64_t* out);
/* win2tok[nW*N]: source token (i*W+j) for every window slot, -1 for zero-pad slots.
 * tok2win[H*W]: window slot of every real token.
 * region_ids[nW*N] (shift > 0 only): region label of every window slot; mask[w,p,q] = (ids[w,p] == ids[w,q]) ? 0 : -100
 * (what the attention kernels consume: the 49x49 mask is rebuilt in registers instead of being loaded).
 * Any of the three pointers may be NULL. */
int esvit_window_maps(int H, int W, int ws, int shift, int32_t* win2tok, int32_t* tok2win, int32_t* region_ids);
/* mask[nW*N*N] in {0,-100}; returns nW through *n_windows */
int esvit_shift_mask(int H, int W, int ws, int shift, float* mask, int* n_windows);

/* ---- MFMA GEMM family -------------------------------------------------- */
#define ESVIT_EPI_NONE 0
#define ESVIT_EPI_GELU 1     /* out = gelu(acc+bias); aux (if set) receives acc+bias */
#define ESVIT_EPI_GELU_BWD 2 /* out = acc * gelu'(aux) */
#define ESVIT_EPI_QGELU 3     /* QuickGELU (cvt_v4_transformer.py:44-46): out = v*sigmoid(1.702 v), v = acc+bias; aux receives v */
#define ESVIT_EPI_QGELU_BWD 4 /* out = acc * d/dv[v*sigmoid(1.702 v)] at v = aux */

/* The k-nearest-neighbour epilogue of esvit_gemm (esvit_gemm_desc::topk; eval_knn.py:197-210 without the [rows, N_train] similarity
 * block): A = test features [M, K], B = train features [N, K], both fp32 row-major as stored (dtype ESVIT_F32, K % 4 == 0).  Per test
 * row the k largest similarities and the numbers of their train rows come out sorted by ONE total order -- larger similarity first,
 * on equal similarities the smaller train row number first --, so the list for any k' < k is the first k' columns of the list for k,
 * and two launches give the same bits.  Every similarity is accumulated over K in one fixed order (v_mfma_f32_16x16x4_f32) that does
 * not depend on where the train row lies in B: scoring B piece by piece with merge = 1 ends with exactly the lists of the whole.
 *   k          1 .. 256; k <= N unless merge
 *   vals, idx  fp32 / int32 [M, k], row-major
 *   idx_base   added to every row number of this call's B (the position of the piece in the whole train matrix)
 *   merge      1: the incoming contents of vals / idx are a valid sorted list (global row numbers) that takes part
 *   workspace  >= esvit_query(ESVIT_Q_TOPK_WS, M, N, k) bytes, 16-byte aligned; contents need not be initialised
 * C may be NULL -- then nothing of size M x N is written; otherwise the dense fp32 similarities [M, ldc] are stored from the same
 * accumulators the selection saw (tests, small problems).  No other epilogue field combines with it: bias, residual, rowmap, rowscale,
 * aux, split-K, colsum, rowstat, k-strided operands, batch > 1 and alpha != 1 are rejected with ESVIT_ERR_ARG before any device call. */
typedef struct {
    int32_t k;
    int32_t merge;
    float* vals;
    int32_t* idx;
    int64_t idx_base;
    void* workspace;
    int64_t workspace_bytes;
} esvit_gemm_topk;

typedef struct {
    const void* A;
    const void* B;
    void* C;
    int32_t M, N, K;
    int64_t lda, ldb, ldc;
    int32_t a_kstrided; /* 0: A is M x K row-major (K contiguous); 1: A is K x M row-major */
    int32_t b_kstrided; /* 0: B is N x K row-major (K contiguous); 1: B is K x N row-major */
    int32_t batch;      /* >=1; strides in elements */
    int64_t strideA, strideB, strideC;
    const float* bias;     /* [N] or NULL */
    const float* residual; /* fp32, indexed [dst_row*ldr + n] or NULL */
    int64_t ldr;
    const int32_t* rowmap; /* NULL or [rowmap_period]: dst_row = (m/period)*rowmap_tokens + rowmap[m%period]; <0 => row dropped */
    int32_t rowmap_period, rowmap_tokens;
    const float* rowscale; /* NULL or per-sample scale, index dst_row / rows_per_sample */
    int32_t rows_per_sample;
    void* aux; /* activation dtype, ld = ldaux */
    int64_t ldaux;
    int32_t epilogue; /* ESVIT_EPI_* */
    int32_t out_f32;  /* 1: C is fp32, 0: C has the activation dtype */
    int32_t splitk;   /* >1: fp32 partial sums in `partial`, then reduced into C (fp32 with out_f32, else the activation dtype); slice z takes the k-tiles
                       * [z, z + 1) * ceil(k-tiles / splitk) -- trailing slices may be empty; no fused epilogue, dense C (ldc == N), batch == 1 */
    float* partial;   /* workspace >= splitk*M*N floats */
    int32_t accumulate; /* split-K reduce: C += sum (1) or C = sum (0) */
    float alpha;
    float* colsum;         /* optional, fp32 [M]: alpha * row sums of op(A) over K (= bias gradient when A = dY^T); fused via an all-ones B fragment; k-strided A only */
    float* colsum_partial; /* workspace >= splitk*M floats when splitk > 1 */
    int32_t kernel;        /* ESVIT_GEMM_AUTO (0): chosen from the shape; otherwise force one main loop (tests / tuning) */
    /* optional softmax statistics of the OUTPUT rows (the logits of the DINO head, vision_transformer.py:418): for every row and
     * every 64-column block j the pair (m, s) = (max_k z_k, sum_k 2^(z_k - m)) over k in [64 j, 64 j + 64) of
     * z_k = (C[row][k] as stored, i.e. rounded to the activation dtype, - rowstat_center[k]) * rowstat_scale
     * (scale = log2(e) / temperature; center NULL = 0).  rowstat: fp32 [M, N / 64, 2] -- or [M, N / 32, 2], blocks of 32 columns,
     * when the descriptor asks for ESVIT_GEMM_P8 (M and N whole 256-tiles; esvit_gemm_select reports what a descriptor resolves to -- AUTO keeps
     * the 128 x 128 tile for statistics, measured faster inside the step).  Only for the plain bf16 epilogue of a
     * dense forward GEMM with M % 128 == 0 and N % 128 == 0 (rejected otherwise); esvit_rowstat_combine folds the blocks of a row,
     * esvit_dino_ce_fwd_bwd takes them in place of its first pass over the logits (main_esvit.py:728-742). */
    float* rowstat;
    const float* rowstat_center;
    float rowstat_scale;
    /* optional, with rowstat on the 128 x 128 tile only (not ESVIT_GEMM_P8): fp32 [M / 64, N], the sums of the STORED logits over
     * each 64-row wave tile per column -- esvit_partial_reduce folds them into the batch sum the centre update needs
     * (main_esvit.py:752-770) without another pass over the logits. */
    float* colstat;
    /* optional: the fused k-nearest-neighbour selection (see esvit_gemm_topk above); NULL = off, every other call is what it was */
    const esvit_gemm_topk* topk;
} esvit_gemm_desc;

/* main loops of the family (esvit_gemm_desc.kernel; what esvit_gemm_select returns) */
#define ESVIT_GEMM_AUTO 0
#define ESVIT_GEMM_REGSTAGE 1 /* register-staged 128-row tiles: the exact-fp32 mode, and a bf16 fallback */
#define ESVIT_GEMM_DMA4 2     /* bf16, LDS-DMA, 128 x {64,96,128} tiles, 4 waves, two workgroups per CU */
#define ESVIT_GEMM_DMA8 3     /* bf16, LDS-DMA, 256 x 256 tiles, 8 waves, one workgroup per CU: very long reductions */
#define ESVIT_GEMM_DMA4W 4    /* bf16, LDS-DMA, 4 waves, 128 x 192 / 128 x 96 tiles with whole-width wave rows (N % 96 == 0) */
#define ESVIT_GEMM_P8 5       /* bf16, LDS-DMA, 256 x 256 tiles, 8 waves, eight-phase schedule with counted DMA waits (K % 64 == 0, no rowmap; rowstat only over whole 256 x 256 tiles, in 32-column blocks, without colstat) */

/* C = alpha * op(A) op(B) (+ epilogue).  Replaces every nn.Linear / conv-as-GEMM on the
 * path: swin_transformer.py:31-37,127,150,418,531; vision_transformer.py:414-418;
 * and their autograd backward (dgrad: b_kstrided or cached W^T; wgrad: a_kstrided && b_kstrided). */
int esvit_gemm(int dtype, const esvit_gemm_desc* d, esvit_stream_t stream);
/* The main loop esvit_gemm would run for this descriptor (a pure function of it; > 0) with its output tile and the
 * number of workgroups the chip keeps resident at once -- what a caller needs to size split-K (one workgroup per
 * (tile, slice); a launch of more workgroups than resident slots runs in rounds) before it allocates `partial`. */
int esvit_gemm_select(int dtype, const esvit_gemm_desc* d, int* tile_m, int* tile_n, int* resident_slots);

/* ---- fused Swin MLP branch, forward and backward (swin_transformer.py:331 + 31-37) ---
 * y = x + rowscale[row] * ( GELU( LayerNorm(x) W1^T + b1 ) W2^T + b2 ) for the narrow stages (bf16, C in {96, 192}: Swin-T / -S, {128, 256}: Swin-B; C = 384: see below;
 * esvit_query(ESVIT_Q_MLP_FUSED, dtype, C, 0) bit 0 = forward, bit 1 = backward).  The unfused LayerNorm -> fc1 (+GELU) -> fc2
 * (+residual) sequence is bound there by the HBM round trips of the 4C-wide hidden activation (40 B per token-channel forward,
 * 64 B backward).  x, y fp32 [M, C]; W1 [4C, C], W2 [C, 4C] in the activation dtype; gamma, beta, b1, b2 fp32; rowscale fp32 [M]
 * (the DropPath factor of each row) or NULL.
 *
 * esvit_mlp_fused_fwd: one kernel, 8 B per token-channel, NOTHING hidden-sized is written (inference passes and training alike:
 *   the backward below recomputes).  Optional second output (gamma_next != NULL): LayerNorm(y) with the parameters of the
 *   NEXT block's norm1 (swin_transformer.py:283) -- xw_next [M, C] in the activation dtype, mean_next / rstd_next fp32 [M] --
 *   so that block needs no LayerNorm launch.
 * esvit_mlp_fused_bwd: the data-gradient path of the branch in one kernel.  Inputs: x (the branch input), gy = dL/dy fp32,
 *   rowscale_mlp (the forward's rowscale), W1, and the transposed copies W2T = W2^T [4C, C], W1T = W1^T [C, 4C]
 *   (esvit_mlp_fused_weight).  It recomputes LayerNorm(x) and the pre-activation, forms dA = (rowscale gy W2) o GELU'(A) and
 *   dH = dA W1 with the hidden tile in registers, applies the LayerNorm backward and writes
 *     gx      fp32 [M, C]   dL/dx = gy + LN'(dH)                 gx_act  act [M, C]  cast(rowscale_out[row] * gx) (NULL scale = 1)
 *     xhat    act [M, C]    (x - mean) rstd                      a1g     act [M, 4C] GELU(A)          da1  act [M, 4C]  dA
 *   The weight gradients are two esvit_gemm calls: dW2 = (rowscale gy)^T a1g, and G = da1^T xhat, db1 = colsum(da1) followed by
 *   esvit_ln_fold_finish.
 *   Weight gradients on the chip (trailing arguments dW2, G, db1, db2, partials_ws; bf16 and C = 96 only): with all five given the
 *   same call also returns   dW2 fp32 [C, 4C] = (rowscale gy)^T GELU(A),   db2 fp32 [C] = colsum(rowscale gy),
 *   G fp32 [4C, C] = dA^T xhat,   db1 fp32 [4C] = colsum(dA)   (overwritten; G and db1 go on to esvit_ln_fold_finish), accumulated in
 *   registers by persistent workgroups and summed from per-workgroup partials in index order by a second launch of the same call (no
 *   atomics: identical launches give identical bits).  partials_ws: esvit_query(ESVIT_Q_MLP_DW_WS, dtype, C, M) bytes, 16-byte aligned,
 *   contents need not be initialised.  xhat, a1g and da1 are not written in this mode and may be NULL; W1T is not read.  All five
 *   NULL: the mode above, unchanged.  Any other combination, or the five given at another dtype / C: ESVIT_ERR_ARG before any launch.
 * esvit_ln_fold_finish: LayerNorm folded out of a weight gradient.  With LN(x) = xhat o gamma + beta and G = dY^T xhat [J, C],
 *   db = colsum(dY) [J], W the fp32 master [J, C]:  dW = G o gamma + db (x) beta (written over G),
 *   dgamma[c] (+)= sum_j W[j, c] G[j, c],  dbeta[c] (+)= sum_j db[j] W[j, c]   (swin_transformer.py:331 autograd).
 */
int esvit_mlp_fused_fwd(int dtype, const float* x, const float* gamma, const float* beta, float eps, const void* W1,
                        const float* b1, const void* W2, const float* b2, const float* rowscale, int64_t M, int C, float* y,
                        const float* gamma_next, const float* beta_next, void* xw_next, float* mean_next, float* rstd_next,
                        esvit_stream_t stream);
/* The wide stage (C = 384, bf16: stage 2 of Swin-T / -S; esvit_query bit 0): esvit_mlp_fused_fwd is the inference pass (the EMA teacher:
 * x in, y out, 8 B per token-channel; gamma_next must be NULL).  esvit_mlp_fused_fwd_train is the same kernel for a pass whose backward is
 * the unfused sequence (swin_transformer.py:31-37 autograd through esvit_gemm): besides y it writes what that backward reads --
 *   a1 act [M, 4C] the pre-activation LN(x) W1^T + b1,  a1g act [M, 4C] GELU(a1),  h act [M, C] LayerNorm(x),  mean / rstd fp32 [M] --
 * in place of the LayerNorm launch and the two GEMM launches that would produce them.  W1 = ESVIT_MLP_W1_FWD (the plain cast at this width). */
int esvit_mlp_fused_fwd_train(int dtype, const float* x, const float* gamma, const float* beta, float eps, const void* W1, const float* b1,
                              const void* W2, const float* b2, const float* rowscale, int64_t M, int C, float* y, void* a1, void* a1g,
                              void* h, float* mean, float* rstd, esvit_stream_t stream);
int esvit_mlp_fused_bwd(int dtype, const float* x, const float* gy, const float* rowscale_mlp, const float* rowscale_out,
                        const float* gamma, const float* beta, float eps, const void* W1, const void* W2T, const void* W1T,
                        const float* b1, int64_t M, int C, float* gx, void* gx_act, void* xhat, void* a1g, void* da1,
                        esvit_stream_t stream, float* dW2, float* G, float* db1, float* db2, float* partials_ws);
int esvit_ln_fold_finish(float* G, const float* db, const float* W, const float* gamma, const float* beta, int J, int C,
                         float* dgamma, float* dbeta, int accumulate, esvit_stream_t stream);
/* The weight copies the fused kernels stream, produced from the fp32 masters (fc1.weight [4C, C], fc2.weight [C, 4C]); fc2.weight
 * itself is consumed as its plain activation-dtype cast.  esvit_mlp_fused_fwd takes W1 = ESVIT_MLP_W1_FWD; esvit_mlp_fused_bwd
 * takes W1 = ESVIT_MLP_W1_BWD, W2T = ESVIT_MLP_W2T_BWD, W1T = ESVIT_MLP_W1T_BWD (the channel order of a copy follows the kernel
 * generation that consumes it and is private to the library). */
#define ESVIT_MLP_W1_FWD 0
#define ESVIT_MLP_W1_BWD 1
#define ESVIT_MLP_W1T_BWD 2
#define ESVIT_MLP_W2T_BWD 3
int esvit_mlp_fused_weight(int kind, const float* src, void* dst_bf16, int C, esvit_stream_t stream);
/* dst (bf16) = cast(src fp32 [R, S]), transposed to [S, R] if `transpose`, and with perm32 != 0 every aligned 32-block of a dst row
 * reordered so that position 8g + e holds column 4g + e (e < 4) / 16 + 4g + (e - 4): the channel order of the 16-token kernels. */
int esvit_cast_weight(const float* src, void* dst_bf16, int R, int S, int transpose, int perm32, esvit_stream_t stream);

/* ---- normalisation ----------------------------------------------------- */
/* LayerNorm forward over rows of C channels (swin_transformer.py:283,331,417,546,687;
 * eps 1e-6 at :963).  x: fp32 [rows, C] (or gathered, see gather).  y has `dtype`.
 * rowmap (optional): y row = (r/tokens)*period_out + rowmap[r%tokens] (token -> window slot);
 * the caller pre-zeroes y so pad slots stay 0 (swin_transformer.py:286-290).
 * y_f32 (optional) receives an fp32 copy at the un-mapped row. */
int esvit_layernorm_fwd(int dtype, const float* x, const float* gamma, const float* beta, float eps,
                        int64_t rows, int C, void* y, float* y_f32, float* mean, float* rstd,
                        const int32_t* rowmap, int tokens, int period_out, esvit_stream_t stream);
/* LayerNorm backward.  dy (dtype) is read at the mapped row when rowmap is given.
 * dx = g_in (optional fp32 residual gradient) + LN'(dy).  dgamma/dbeta partials are written to ws ([nblk,2,C] floats,
 * nblk = esvit_query(ESVIT_Q_LN_BWD_BLOCKS, rows, C, 0)) and reduced into dgamma/dbeta (fp32, overwritten).
 * dx_act (optional, un-mapped rows only) = rowscale[row / rows_per_sample] * dx: the DropPath-scaled copy the next dgrad / wgrad
 * GEMMs of the backward read (rowscale may be NULL = 1) -- saves one esvit_gather_cast pass.  act_dtype: its dtype -- `dtype`, or
 * ESVIT_BF16 while dy is fp32 (the patch-embedding norm, whose upstream gradient is the fp32 residual-stream gradient).  dx may be NULL
 * when dx_act is given (only the copy is wanted; g_in must then be NULL).
 *
 * qkv-tail mode (period_in == ESVIT_LN_BWD_QKV_TAIL; bf16, C = 96): the tail of a Swin block's attention-branch backward in one
 * persistent kernel and an index-ordered reduce.  dy is then dqkv bf16 [rows, 3C], the gradient of qkv = LayerNorm(x) Wqkv^T + bqkv,
 * and `rowmap` points at an esvit_ln_qkv_tail record instead of a row map (tokens = 0).  The call forms dxw = bf16(dqkv Wqkv) per
 * 64-row tile on the chip, applies the LayerNorm backward to it (dx = g_in + LN'(dxw), dx_act, dgamma, dbeta as above; dx and g_in
 * are required) and accumulates dWqkv = dqkv^T LayerNorm(x) [3C, C] and dbqkv = colsum(dqkv) [3C] beside it, LayerNorm(x) recomputed
 * from x, mean, rstd, gamma and the record's beta with the forward's expression and rounded to bf16 as the forward's output is.  ws:
 * esvit_query(ESVIT_Q_ATTN_TAIL_WS, dtype, C, rows) bytes, 16-byte aligned; workgroup b walks tiles b, b + grid, ... and writes
 * partial b, the reduce sums the partials in index order and OVERWRITES dWqkv, dbqkv, dgamma, dbeta (no atomics: identical launches
 * give identical bits).  Any other dtype or width returns ESVIT_ERR_ARG before any launch. */
#define ESVIT_LN_BWD_QKV_TAIL (-1)
typedef struct esvit_ln_qkv_tail {
    const void* Wqkv;   /* bf16 [3C, C]: the plain cast of qkv.weight, 16-byte aligned */
    const float* beta;  /* fp32 [C] */
    float* dWqkv;       /* fp32 [3C, C] out */
    float* dbqkv;       /* fp32 [3C] out */
} esvit_ln_qkv_tail;
int esvit_layernorm_bwd(int dtype, const void* dy, const float* x, const float* mean, const float* rstd,
                        const float* gamma, const float* g_in, int64_t rows, int C, float* dx,
                        float* dgamma, float* dbeta, float* ws, const int32_t* rowmap, int tokens,
                        int period_in, void* dx_act, int act_dtype, const float* rowscale, int rows_per_sample,
                        esvit_stream_t stream);

/* ---- element-wise / data-movement helpers ------------------------------ */
/* dst[r,:] = cast(scale[r/rows_per_sample] * src[map(r),:]); src fp32 [*, C]; dst dtype [rows, C].
 * rowmap (optional, [period]): src row = (r/period)*tokens + rowmap[r%period]; <0 => zeros.
 * Used for dY staging of the windowed proj backward (swin_transformer.py:315-330 reversed). */
int esvit_gather_cast(int dtype, const float* src, void* dst, int64_t rows, int C, const int32_t* rowmap,
                      int period, int tokens, const float* rowscale, int rows_per_sample,
                      esvit_stream_t stream);
/* plain cast fp32 -> activation dtype (weight caches) */
int esvit_cast_f32_to(int dtype, const float* src, void* dst, int64_t n, esvit_stream_t stream);
/* out[n] (+)= sum_r x[r,n]  (bias gradients).  ws >= esvit_query(ESVIT_Q_COLSUM_BLOCKS, rows, 0, 0)*N floats */
int esvit_colsum(int dtype, const void* x, int64_t rows, int N, int64_t ld, float* out, float* ws,
                 int accumulate, esvit_stream_t stream);

/* PatchEmbed im2col for the 4x4/4 conv (swin_transformer.py:531,544) and the ViT patch embedding
 * (vision_transformer.py:121-139): img fp32 NCHW [nB,3,H,W] -> cols dtype [nB*(H/P)*(W/P), Kpad],
 * rows (image, patch row, patch column), column order (c, ph, pw), zero padded to Kpad.
 * S < 65536: a square image, H = W = S.  Otherwise S carries a rectangle: H = S & 0xffff (rows),
 * W = S >> 16 (columns); a square image in this form gives the same bits as the plain call.
 * ESVIT_ERR_ARG before any launch unless P % 4 == 0, H % P == 0, W % P == 0, H > 0, W > 0,
 * Kpad % 8 == 0 and Kpad >= 3*P*P.
 *
 * FUSED MODE (nB = -G, G = 1 .. ESVIT_PATCH_EMBED_MAX_CROPS; dtype ESVIT_BF16, S = 0, P = 4, Kpad = 48; cols unused): `img` is a HOST
 * esvit_patch_embed whose first G crop records are read -- the Swin patch embedding with PATCH_NORM (swin_transformer.py:531-547),
 * Conv2d(3, E, 4, 4) + LayerNorm(E), E in {96, 128, 192}, straight from the images: no column matrix, projection output or dL/dy is
 * ever written.  The crops of a call own consecutive token rows (crop i + 1 starts where crop i ends; rows are (image, patch row,
 * patch column)), H and W any multiples of 4, at most ESVIT_PATCH_EMBED_MAX_ROWS rows.  Columns keep the (c, ph, pw) order and the
 * bf16 rounding of the plain mode; W is the bf16 [E, 48] weight, everything else fp32.
 *   ESVIT_PATCH_EMBED_FWD     x[row, E] = LayerNorm(cols W^T + bias) * gamma + beta; mean / rstd [row] written unless both are NULL
 *   ESVIT_PATCH_EMBED_BWD     from gx = dL/dx [row, E] and the forward's mean / rstd: one partial record
 *                             [dW E x 48 | dbias E | dgamma E | dbeta E] per workgroup of the launch, written from record first_partial
 *                             of `partials` on; esvit_query(ESVIT_Q_PATCH_EMBED_WS, dtype, E, rows of the call) BYTES per call.  dL/dy
 *                             is rounded to bf16 before it meets the columns, as esvit_layernorm_bwd's activation-dtype output is.
 *                             The images get no gradient.
 *   ESVIT_PATCH_EMBED_REDUCE  (G ignored) the first `first_partial` records of `partials` summed in a fixed order into dW, dbias,
 *                             dgamma, dbeta.  No atomics in either launch: the bits depend on the call's shapes only.
 * ESVIT_ERR_ARG before any device call for anything else (another dtype, E, P; a null or misaligned pointer -- images, W and x 16
 * bytes --; a crop that does not start where the one before it ends). */
#define ESVIT_PATCH_EMBED_MAX_CROPS 16
#define ESVIT_PATCH_EMBED_MAX_ROWS (1 << 30)
#define ESVIT_PATCH_EMBED_FWD 0
#define ESVIT_PATCH_EMBED_BWD 1
#define ESVIT_PATCH_EMBED_REDUCE 2
typedef struct {
    const float* img; /* fp32 [nB, 3, H, W] */
    int32_t nB, H, W;
    int32_t reserved;
    int64_t row0; /* first token row of this crop */
} esvit_patch_crop;
typedef struct {
    int32_t mode, E;
    const void* W;
    const float* bias;
    const float* gamma;
    const float* beta;
    float eps;
    int32_t first_partial;
    float* x;
    float* mean;
    float* rstd;
    const float* gx;
    float* partials;
    float* dW;
    float* dbp;
    float* dgamma;
    float* dbeta;
    esvit_patch_crop crops[ESVIT_PATCH_EMBED_MAX_CROPS];
} esvit_patch_embed;
int esvit_patch_im2col(int dtype, const float* img, void* cols, int nB, int S, int P, int Kpad,
                       esvit_stream_t stream);
/* PatchMerging gather + LayerNorm(4C) (swin_transformer.py:410-417): x fp32 [nB,H,W,C] ->
 * y dtype [nB*(H/2)*(W/2), 4C]; channel blocks [x(2i,2j), x(2i+1,2j), x(2i,2j+1), x(2i+1,2j+1)].  H and W even.
 * PAD MODE: H = true height | ESVIT_MERGE_PAD.  H x W is then the true grid, any sides in [1, 32767] of any parity, and the
 * merged grid is Ho x Wo = (H+1)/2 x (W+1)/2: y, mean and rstd have nB*Ho*Wo rows.  A quadrant whose token (2i+di, 2j+dj) lies
 * outside the grid contributes zeros to the 4C row BEFORE the LayerNorm -- F.pad followed by the concatenation
 * (swin_transformer.py:406-414): the zeros enter the row statistics and those channels come out as (0 - mean)*rstd*gamma + beta.
 * No address is formed for such a quadrant (the load is predicated).  On an even grid the flag changes no bit of the result.
 * ESVIT_ERR_ARG before any launch for a null pointer, a side outside [1, 32767], other bits set in H, C % 4 != 0 or nB < 1. */
#define ESVIT_MERGE_PAD 0x40000000
int esvit_merge_ln_fwd(int dtype, const float* x, const float* gamma, const float* beta, float eps,
                       int nB, int H, int W, int C, void* y, float* mean, float* rstd,
                       esvit_stream_t stream);
/* backward of the above: dy dtype [nB*(H/2)*(W/2), 4C] -> dx fp32 [nB,H,W,C] (overwritten); dgamma / dbeta overwritten, or
 * added to when accumulate != 0 (further resolution groups sharing the parameters).  dx_act (optional, `dtype`, [nB,H,W,C]) =
 * rowscale[token row / rows_per_sample] * dx as in esvit_layernorm_bwd: the MLP-branch operand of the stage's LAST block, whose
 * dL/dy this is.
 * PAD MODE (H = true height | ESVIT_MERGE_PAD, as in the forward): dy, mean, rstd have nB*Ho*Wo rows; dx and dx_act stay
 * [nB,H,W,C] and receive every live token exactly once -- nothing is written for a pad position.  dgamma / dbeta include the pad
 * quadrants' terms (their x-hat is -mean*rstd, not zero).  rowscale is indexed by the live token row (b*H + i)*W + j over
 * rows_per_sample.  accumulate keeps its meaning.  Refusals as in the forward. */
int esvit_merge_ln_bwd(int dtype, const void* dy, const float* x, const float* mean, const float* rstd,
                       const float* gamma, int nB, int H, int W, int C, float* dx, float* dgamma,
                       float* dbeta, float* ws, void* dx_act, const float* rowscale, int rows_per_sample, int accumulate,
                       esvit_stream_t stream);
/* token mean (swin_transformer.py:688-689): x fp32 [nB,T,C] -> out fp32 [nB,C] (+ act copy) */
int esvit_token_mean_fwd(int dtype, const float* x, int nB, int T, int C, float* out, void* out_act,
                         esvit_stream_t stream);
/* dx[b,t,:] = g_tok[b,t,:] (optional) + g_mean[b,:]/T */
int esvit_token_mean_bwd(const float* g_mean, const float* g_tok, int nB, int T, int C, float* dx,
                         esvit_stream_t stream);

/* ---- fused attention branch of a Swin block (swin_transformer.py:283-330 with 120-152) --------------------
 * y = x + rowscale * (proj(window_attention(qkv(LayerNorm(x)))) + b_proj) in ONE kernel for 7x7 windows (N = ws*ws <= 64),
 * head_dim 32, C = 32 nH in {96, 192}, bf16 activations: LayerNorm output, qkv and the attention output stay on the chip
 * (8 B per token-channel through HBM).  x, y fp32 [nB*L, C] token-ordered rows of one resolution group; win2tok / region_ids /
 * rel_table / bias_frag_ws / scale as for esvit_window_attn_fwd (zero-pad slots carry q / k / v = bias, pad query rows are
 * dropped).  Wqkv_p bf16 [3C, C] and Wproj_p bf16 [C, C]: esvit_cast_weight(W, perm32 = 1) of qkv.weight / proj.weight.
 * rowscale fp32 [nB*L] (DropPath factor of every row) or NULL.  Side outputs for a training pass whose backward runs the
 * unfused kernels -- all five or none: xw bf16 [nB*L, C] = LayerNorm(x), qkv bf16 [nB*L, 3C], ao bf16 [nB*L, C] (attention
 * output before the projection), mean / rstd fp32 [nB*L].  The rows of one call must fit 2 GiB buffer ranges.  bwd = NULL: this
 * forward; otherwise the backward mode described below. */
/* Backward mode of the fused attention branch (bf16, C = 96, nH = 3, head_dim 32, 7x7 windows): with bwd != NULL the call is the
 * branch's BACKWARD for the same geometry arguments.  It recomputes the forward per window from x and writes gx = dL/dx; the weight
 * gradients, the LayerNorm gradients and the relative-position-bias gradient are accumulated on the chip: every workgroup writes one
 * partial of ESVIT_ATTN_BWD_PARTIAL_FLOATS floats and one bias-gradient slab [nH][4096] in the frag layout esvit_relpos_bias_bwd
 * folds; a second launch sums the partials in index order (no atomics: identical launches give identical bits).  In this mode
 *   y and the five side outputs must be NULL, bias_frag_ws must already be filled (rel_table = NULL), bproj is not read;
 *   Wqkv_p  = the plain bf16 cast of qkv.weight [3C, C] (esvit_cast_weight, no flags);
 *   Wproj_p = the TRANSPOSED plain bf16 cast of proj.weight [C, C] (esvit_cast_weight, transpose = 1);
 *   rowscale = the branch's DropPath row factors (dy = rowscale * gin), or NULL.
 * Layout (64-bit pointers), offsets in bytes:
 *     0 gin            fp32 [rows, C]  dL/dx1 (required, 16-byte aligned)
 *     8 rowscale_out   fp32 [rows] or NULL: factors of gx_act
 *    16 gx             fp32 [rows, C]  out (required, 16-byte aligned)
 *    24 gx_act         bf16 [rows, C] or NULL: cast(rowscale_out * gx)
 *    32 WqkvT          bf16 [C, 3C]: the transposed plain cast of qkv.weight (required)
 *    40 dWqkv  48 dbqkv  56 dWproj  64 dbproj  72 dgamma  80 dbeta     fp32 outputs (required; written by the call with finish > 0)
 *    88 dbias_ws       fp32 [partials, nH, 4096] (required, 16-byte aligned)
 *    96 partials_ws    fp32 [partials, ESVIT_ATTN_BWD_PARTIAL_FLOATS] (required, 16-byte aligned)
 *   104 first_partial  index of this call's first partial / slab; the call writes esvit_query(ESVIT_Q_ATTN_BWD_FUSED_GRID, ...) of them
 *   108 finish         0: do not reduce yet; n > 0: after this launch sum partials [0, n) into the six outputs (n >= first_partial + this
 *                      call's workgroups), so that the groups of a ragged block stack their partials and reduce once
 *   112 index          int64 [N*N] relative-position index, 120 dtable fp32 [table_rows, nH], 128 table_rows: optional, all or none.  With
 *                      them the finishing call also writes the table's gradient (overwritten) WITHOUT atomics: the slabs [0, n) are
 *                      summed in index order into slab 0, whose sum the table's rows then gather in query order -- identical launches give
 *                      identical bits, which esvit_relpos_bias_bwd (an atomicAdd scatter) does only with ESVIT_RELPOS_ORDERED.  dtable = NULL: the slabs are left for
 *                      esvit_relpos_bias_bwd(dbias_ws, n, ...)
 * Every misuse returns ESVIT_ERR_ARG before any launch. */
typedef struct esvit_attn_bwd_desc {
    const float* gin;
    const float* rowscale_out;
    float* gx;
    void* gx_act;
    const void* WqkvT;
    float* dWqkv;
    float* dbqkv;
    float* dWproj;
    float* dbproj;
    float* dgamma;
    float* dbeta;
    float* dbias_ws;
    float* partials_ws;
    int32_t first_partial;
    int32_t finish;
    const int64_t* index;
    float* dtable;
    int32_t table_rows;
} esvit_attn_bwd_desc;
int esvit_attn_branch_fwd(int dtype, const float* x, const float* gamma, const float* beta, float eps, const void* Wqkv_p,
                          const float* bqkv, const void* Wproj_p, const float* bproj, const int32_t* win2tok, int L,
                          const float* rel_table, int ws, float* bias_frag_ws, const int32_t* region_ids, int nW, int nB, int N,
                          int nH, float scale, const float* rowscale, float* y, void* xw, void* qkv, void* ao, float* mean,
                          float* rstd, esvit_stream_t stream, const esvit_attn_bwd_desc* bwd);

/* ---- window attention (swin_transformer.py:126-152) ---------------------
 * "frag layout" of an NP x NP matrix X[q][key] (NP = 64 for 7x7 windows): the order in which the
 * MFMA accumulators of the transposed score tile hold it,
 *   X_frag[((ki*4 + qj)*64 + lane)*4 + r] = X[q = 16*qj + c][key = 16*ki + 4*g + r], lane = 16*g + c.
 * esvit_query(ESVIT_Q_ATTN_FRAG_ELEMS, N, 0, 0) = floats per matrix in that layout (4096), -1 if N is unsupported. */
/* Token-ordered window attention.  qkv dtype [nB*L, 3C] (columns [3][nH][hd]) -> out dtype [nB*L, C].
 * win2tok int32 [nW*N] (esvit_window_maps): window slot -> token of the image, -1 for a zero-pad slot; this map
 * IS pad -> roll -> window_partition and its inverse (swin_transformer.py:286-325), applied on the fly.
 * qkv_bias fp32 [3C]: the value of q,k,v at a zero-pad slot (LayerNorm output is zero-padded, so qkv = bias there;
 * pad keys/values take part in every softmax exactly as in the reference, pad query rows are dropped).
 * rel_table fp32 [(2ws-1)^2, nH] is the relative_position_bias_table parameter itself (swin_transformer.py:133-136,
 * index in closed form).  bias_frag_ws (required): fp32 scratch [2, nH, ESVIT_Q_ATTN_FRAG_ELEMS(N)] the library fills with
 * the bias in MFMA fragment order (one 16-byte load per lane per score tile instead of table gathers in the kernel).
 * rel_table = NULL: bias_frag_ws already holds that (an earlier forward / backward call with the same table, ws and nH filled
 * it) -- a block's second resolution group and its backward reuse the forward's fill.
 * region_ids int32 [nW*N] (esvit_window_maps) for shifted blocks or NULL.
 * scale: applied to q before the product (swin_transformer.py:130: hd^-0.5; CvT passes dim^-0.5).  N = ws*ws <= 64 with
 * hd in {32, 64} (7x7 Swin windows; 7x7 / 6x6 / 3x3 CvT windows at hd 64), or N = 196 (14x14) with hd = 32.
 * lse fp32 [nB*nW*nH, ESVIT_Q_ATTN_LSE_ELEMS(N)]: per-query log-sum-exp, written for 14x14 windows (the blocked
 * backward needs it), unused (may be NULL) for 7x7.  Without attn_out, the 16-slot query tiles of a window that hold no live
 * token (win2tok < 0 in all 16 slots: the padding of a 96^2 crop's window) are not computed -- their output rows do not exist and
 * their lse entries read 0 (a placeholder: esvit_window_attn_bwd either skips the same tiles or treats them as P = 0, it never exponentiates
 * against that 0).  One image's qkv rows (L * 3C activations) must fit a 2 GiB buffer
 * descriptor.
 * attn_out (optional, fp32 [nB*nW,nH,N,N]) receives the softmax (swin_transformer.py:146,152). 
 * N <= 64: head_dim 32 or 64.  64 < N <= 224: head_dim 32, or 64 in bf16 (whole ViT crops -- one window per image, N < ws * ws
 * allowed, zero table -- and the 14x14 windows of the CvT / Swin configurations at head_dim 64).
 *
 * Bias gradient of the 224-slot kernels (64 < N <= 224).  At head_dim 32 the dQ kernel accumulates it beside dQ.  At head_dim 64 that
 * kernel has no registers left for it and a kernel of its own writes the same slabs (it recomputes S and dP a second time): there, and
 * only there, dbias_ws = NULL is accepted and skips that kernel -- the caller without a table (the ViTs, CvT without REL_POS_EMBED).
 * For every other shape dbias_ws = NULL is ESVIT_ERR_ARG before any launch.
 * ws | ESVIT_ATTN_SPLIT_DBIAS (esvit_window_attn_bwd only, 64 < N <= 224, bf16; ESVIT_ERR_ARG elsewhere): the separate bias-gradient
 * kernel also at head_dim 32 -- the dQ kernel runs unchanged, then the separate kernel writes the slabs.  Not routed by the package: the
 * arrangement "bias gradient out of the dQ kernel", kept available for tests and A/B measurements.
 *
 * Sliding-chunk mode (ws | ESVIT_ATTN_SLIDING_CHUNK; chunk_attn.hip): Vision Longformer's attention (layers/slidingchunk_2d.py
 * mode 0, layers/longformer2d.py) over one token grid per image, fused -- no tensor grows with L^2.  The tokens of an image are
 * [nglo globals | an nx x ny grid, row-major]; a global token sees and is seen by every token, a grid token also sees the tokens of
 * its own and the eight adjacent ws x ws chunks.  The arguments mean, in this mode:
 *   ws           7 | ESVIT_ATTN_SLIDING_CHUNK (other chunk sides: ESVIT_ERR_ARG)
 *   L            tokens per image, nglo + nx * ny;  nW = nx (grid rows),  N = ny (grid columns);  nglo = L - nW * N <= 7
 *   win2tok      int32 [L], the chunk table of that grid: -1 for a global token, else chunk row << 16 | chunk column (the kernels use
 *                the closed form the table spells out, csrc/chunk_geom.h)
 *   bias_frag_ws fp32 scratch of esvit_query(ESVIT_Q_CHUNK_ATTN_WS, nB * nH, L, 0 forward | 1 backward) floats
 *   lse          fp32 [nB, nH, L], written by the forward and read by the backward (required), as fwd_out is
 *   hd           32, 48 or 64;  dtype bf16 only (ESVIT_ERR_ARG otherwise, before any launch: the fp32 parity mode keeps the dense route)
 *   qkv_bias, rel_table, region_ids, attn_out, dbias_ws, dpad_ws: not used, pass NULL
 * Every row of out / dqkv is written; no atomics: two launches give identical bits.
 *
 * Global mode (ws = ESVIT_ATTN_GLOBAL; flash_attn.hip): plain softmax attention of every token of an image over every token
 * of that image (vision_transformer.py:76-83) for crops of ANY length, fused -- online softmax over 64-key blocks, no tensor grows
 * with L^2, nothing is padded in memory.  The arguments mean, in this mode:
 *   ws           ESVIT_ATTN_GLOBAL alone (together with ESVIT_ATTN_SLIDING_CHUNK: ESVIT_ERR_ARG)
 *   L            tokens per image, >= 1;  nW = 1;  N = L
 *   bias_frag_ws fp32 scratch of esvit_query(ESVIT_Q_GLOBAL_ATTN_WS, nB * nH, L, 0 forward | 1 backward) floats (forward: none, may be NULL)
 *   lse          fp32 [nB, nH, L], written by the forward and read by the backward (required), as out / fwd_out is
 *   hd           32 or 64;  dtype bf16 only (ESVIT_ERR_ARG otherwise, before any launch: the fp32 parity mode keeps the batched-GEMM route)
 *   scale        multiplies the fp32 scores (q enters the product as the bf16 it is)
 *   win2tok, qkv_bias, rel_table, region_ids, attn_out, dbias_ws, dpad_ws: not used, pass NULL
 * Every row of out / dqkv is written by exactly one workgroup; no atomics: two launches give identical bits.
 *
 * Statistics of the global mode (ws = ESVIT_ATTN_GLOBAL | ESVIT_ATTN_STATS, esvit_window_attn_fwd only; flash_attn.hip): what an
 * attention analysis reads -- the entropy of every query's softmax row and the probability rows of a few listed queries -- from q and k
 * alone: no v, no out, no tensor that grows with L^2.  Scores and probabilities are fp32 (the scores are not rounded to bf16 before the
 * softmax, as the batched-GEMM route does).  The flag is valid only together with ESVIT_ATTN_GLOBAL: alone, with a window side, in
 * esvit_window_attn_bwd or together with ESVIT_ATTN_SLIDING_CHUNK it is ESVIT_ERR_ARG before any launch.  The arguments mean:
 *   L            tokens per image, >= 1;  N = L;  nW = 1 + nq, nq >= 0 the number of listed queries
 *   win2tok      int32 [nq] on the device: token indices in [0, L) of the listed queries, the same for every image and head; duplicates
 *                allowed; NULL when nq = 0.  The library cannot read the array: the caller checks the range (an index outside it yields
 *                the row of a zero query, nothing is read or written out of bounds)
 *   attn_out     fp32 [nB, nH, 1 + nq, L] (required): row 0 = entropy of every query, H = ln l - sum_k e^(s_k - m) (s_k - m) / l in nats
 *                (m, l: maximum and sum of e^(s_k - m) of the row), accumulated online; rows 1 .. nq = softmax_k(scale q k) over all L keys
 *                for the listed queries, from a normaliser of their own
 *   lse          fp32 [nB, nH, L] or NULL: m + ln l of every query
 *   hd, dtype, scale: as in the global mode
 *   out must be NULL;  qkv_bias, rel_table, region_ids, bias_frag_ws: not used, pass NULL
 * Every element has one writer; no atomics: two launches give identical bits.
 *
 * Statistics of the window softmax (ws | ESVIT_ATTN_WINDOW_STATS, a real window side with the flag OR'd in; esvit_window_attn_fwd only;
 * window_attn.hip / window_attn_big.hip): the Swin counterpart of the mode above.  For every (image, window, head) exactly the
 * softmax the forward computes -- staged scale * q with the forward's rounding, pad slots with q, k = qkv bias, the relative-position
 * bias from rel_table / bias_frag_ws (rel_table = NULL: the fragment is already filled), the additive -100 of region_ids, one softmax
 * over the N slots of the window, pad keys included -- and no v, no P V, no out, no N x N tensor.  The arguments mean:
 *   qkv, qkv_bias, win2tok, L, rel_table, bias_frag_ws, region_ids, nW, nB, nH, hd, scale: as in the forward
 *   N            tokens per window | nq << 16, nq >= 0 the number of listed slots (N <= 224 leaves the upper bits free)
 *   attn_out     fp32 [nB*nW, nH, N] (required): the entropy of every query slot's row, pad query slots included, in window-slot order
 *                (the rows the forward's attn_out would hold), in nats: H = ln l - sum_k e^(s_k - m) (s_k - m) / l, m and l the row's
 *                maximum and sum; 0 log 0 = 0 by construction, the padded MFMA columns beyond N do not enter
 *   out          int32 [nq] on the device: the listed query slots, w * N + i in [0, nW * N), the same for every image and head;
 *                duplicates allowed.  The library cannot read the array: the caller checks the range (an index outside it is skipped,
 *                its row stays unwritten, nothing is read or written out of bounds)
 *   lse          fp32 [nB, nH, nq, N]: the probability row of every listed slot over the N slots of its own window, written by the
 *                workgroup that owns the window (one writer per element)
 *   nq = 0: out and lse must be NULL.  nq > 0: both are required.
 * Instances: every one the probability variant has -- N <= 64 at head_dim 32 / 64 in bf16 and fp32, 64 < N <= 224 at head_dim 32 in both
 * and at head_dim 64 in bf16, N < ws * ws as in the forward; anything else is ESVIT_ERR_ARG before any launch, as is the flag in
 * esvit_window_attn_bwd or together with any of the other three flags.  No atomics: two launches give identical bits.
 *
 * Statistics of the sliding-chunk mode (ws = 7 | ESVIT_ATTN_SLIDING_CHUNK | ESVIT_ATTN_CHUNK_STATS, esvit_window_attn_fwd only; chunk_attn.hip,
 * DESIGN §11): the Vision Longformer counterpart of the two modes above -- for every (image, head) exactly the softmax the sliding-chunk
 * forward computes (a local query over the globals and its 3 x 3 chunks with the forward's staging, scale and exponentials; a global
 * query over all L keys per 512-key range) and no v, no P V, no out, no tensor that grows with L^2.  The flag is valid only together with
 * ESVIT_ATTN_SLIDING_CHUNK: without it, in esvit_window_attn_bwd, or together with ESVIT_ATTN_GLOBAL, ESVIT_ATTN_STATS,
 * ESVIT_ATTN_WINDOW_STATS or ESVIT_ATTN_SPLIT_DBIAS it is ESVIT_ERR_ARG before any launch.  The arguments mean:
 *   qkv, win2tok (the chunk table), L, nW = nx, nB, nH, hd, scale: as in the sliding-chunk forward (bf16, head_dim 32 / 48 / 64, chunk
 *                side 7, nglo = L - nx * ny <= 7);  qkv_bias, rel_table, region_ids: not used, pass NULL
 *   N            ny | nq << 16, nq >= 0 the number of listed queries (ny < 65536: the caller refuses wider grids, nq < 32768)
 *   bias_frag_ws fp32 scratch of esvit_query(ESVIT_Q_CHUNK_ATTN_WS, nB * nH, L, 0) floats, the forward's: that is 528 floats per
 *                (image, head, 512-key range), of which the mode writes 24 -- (max, sum, sum e (s - max)) of the 8 global-row slots
 *   attn_out     fp32 [nB, nH, L] (required): the entropy of every token's softmax row over the keys it sees, in nats, token order
 *                [globals | grid row-major] as the forward's lse: H = ln l - sum_k e^(s_k - m) (s_k - m) / l, m and l the row's maximum and
 *                sum; 0 log 0 = 0 by construction; dead neighbourhood slots and the padded MFMA columns do not enter
 *   out          int32 [nq] on the device: the listed query tokens in [0, L), the same for every image and head; duplicates allowed.
 *                The library cannot read the array: the caller checks the range (an index outside it is skipped, its row stays
 *                unwritten, nothing is read or written out of bounds)
 *   lse          fp32 [nB, nH, nq, L]: the probability row of every listed query over ALL L tokens in token order, from a normaliser
 *                of its own; exactly 0 for every key the query does not see; every element written, by one thread
 *   nq = 0: out and lse must be NULL.  nq > 0: both are required.
 * No atomics: two launches give identical bits.
 */
#define ESVIT_ATTN_SLIDING_CHUNK 0x40000000
#define ESVIT_ATTN_GLOBAL 0x20000000
#define ESVIT_ATTN_STATS 0x08000000
#define ESVIT_ATTN_SPLIT_DBIAS 0x10000000
#define ESVIT_ATTN_WINDOW_STATS 0x04000000
#define ESVIT_ATTN_CHUNK_STATS 0x02000000
int esvit_window_attn_fwd(int dtype, const void* qkv, const float* qkv_bias, const int32_t* win2tok, int L,
                          const float* rel_table, int ws, float* bias_frag_ws, const int32_t* region_ids, int nW, int nB,
                          int N, int nH, int hd, float scale, void* out, float* lse, float* attn_out,
                          esvit_stream_t stream);
/* dout dtype [nB*L, C] -> dqkv dtype [nB*L, 3C] (every row written).  fwd_out / lse: the forward's outputs (needed for
 * 14x14 windows only).  Partials: dbias_ws fp32 [ESVIT_Q_ATTN_BWD_PARTS(N, nB*nW, nH), nH, frag]
 * (relative-position-bias gradient, reduced by esvit_relpos_bias_bwd; every element written by exactly one wave, no atomics; NULL:
 * see "Bias gradient of the 224-slot kernels" above) and dpad_ws fp32
 * [ESVIT_Q_ATTN_BWD_PAD_ROWS(N, nB*nW, nH | dtype << 32), 2C], ZERO-INITIALISED by the caller: sums of the dK / dV rows
 * of zero-pad slots, layout [k|v][nH][hd] -- gradients of qkv_bias[C:3C] (column-sum them into the bias gradient). */
int esvit_window_attn_bwd(int dtype, const void* qkv, const float* qkv_bias, const int32_t* win2tok, int L,
                          const void* dout, const void* fwd_out, const float* lse, const float* rel_table, int ws,
                          float* bias_frag_ws, const int32_t* region_ids, int nW, int nB, int N, int nH, int hd,
                          float scale, void* dqkv, float* dbias_ws, float* dpad_ws, esvit_stream_t stream);
/* dtable fp32 [table_rows, nH] (overwritten, or added to when accumulate != 0: the second resolution group of a ragged
 * multi-crop block) = scatter-add over index of sum_parts dbias_ws.  The scatter is one float atomicAdd per (query, key, head): the
 * same slabs give sums that differ in the last bits from launch to launch, and dbias_ws is left as it was.
 * accumulate | ESVIT_RELPOS_ORDERED (the remaining bits keep their meaning: non-zero adds to dtable): every table element has ONE
 * writer and ONE summation order, for N <= 64 and for 64 < N <= 224 alike, no atomics, no memset, no dependence on the grid's
 * schedule -- identical launches give identical bits.  The order: (1) the slabs [0, parts) are summed per frag-layout element in
 * slab order, s = (((0 + slab_0) + slab_1) + ...), INTO slab 0 of dbias_ws: afterwards slab 0 holds the sum and slabs 1.. are
 * untouched (so the call cannot be repeated on the same slabs unless parts = 1); (2) table row t, head h adds its (query, key)
 * pairs {index[q * N + key] == t} to one accumulator that starts at 0, in ascending (query, key) order; (3) the element is written,
 * or added ONCE to dtable's value.  index may hold anything: a row without pairs gets 0 (or keeps its value), entries outside
 * [0, table_rows) are ignored. */
#define ESVIT_RELPOS_ORDERED 0x100
int esvit_relpos_bias_bwd(float* dbias_ws, int parts, const int64_t* index, int N, int nH,
                          int table_rows, float* dtable, int accumulate, esvit_stream_t stream);

/* ---- DINOHead pieces (vision_transformer.py:414-418) -------------------- */
/* z = x / max(||x||_2, 1e-12) row-wise; x dtype [R, D]; z dtype; inv_norm fp32 [R] */
int esvit_l2norm_fwd(int dtype, const void* x, int64_t R, int D, void* z, float* inv_norm,
                     esvit_stream_t stream);
/* dx = (dz - (dz.z) z) * inv_norm */
int esvit_l2norm_bwd(int dtype, const void* dz, const void* z, const float* inv_norm, int64_t R, int D,
                     void* dx, esvit_stream_t stream);
/* legacy weight_norm(dim=0): w[k,:] = g[k] * v[k,:]/||v[k,:]||; v fp32 [K,D]; g fp32 [K];
 * w, wT in dtype ([K,D] and [D,K], either may be NULL); inv_norm fp32 [K] */
int esvit_weightnorm_fwd(int dtype, const float* v, const float* g, int K, int D, void* w, void* wT,
                         float* inv_norm, esvit_stream_t stream);
/* dv = g*inv*(dw - (dw.vhat) vhat); dg = dw.vhat (dg may be NULL) */
int esvit_weightnorm_bwd(const float* dw, const float* v, const float* g, const float* inv_norm, int K,
                         int D, float* dv, float* dg, esvit_stream_t stream);

/* ---- DINOLoss / DDINOLoss (main_esvit.py:603-770) ----------------------- */
/* per-row stats of the sharpened, centred teacher logits (main_esvit.py:629,694,697):
 * for row r: mx[r] = max_k (t[r,k]-c[k])/temp ; lse[r] = log sum exp(.. - mx) */
int esvit_teacher_row_stats(int dtype, const void* t, const float* center, float inv_temp, int64_t R,
                            int K, float* row_max, float* row_lse, esvit_stream_t stream);
/* region matching (main_esvit.py:735-736), fused argmax (first index on ties) + row assembly for the region loss: sim fp32 [B, S, ld] holds, for image b, the cosine
 * similarities of its S student tokens (all crops, image-major) against the 2*Tt teacher tokens
 * (view 0 then view 1).  For student position s of crop crop_id[s] and teacher view iq:
 *   tmatch[cm_row[b*S+s]*2 + iq] = crop_id[s]==iq ? -1 : iq*B*Tt + b*Tt + argmax_j sim[b,s,iq*Tt+j]
 * cm_row maps the image-major position to the student's crop-major logit row (main_esvit.py:710-715). */
int esvit_region_match(const float* sim, int B, int S, int Tt, int ld, const int32_t* crop_id,
                       const int32_t* cm_row, int32_t* tmatch, esvit_stream_t stream);
/* fused student log-softmax CE + gradient (main_esvit.py:706-746).
 * s dtype [Rs, K] student logits (un-tempered); for student row r the teacher rows it is
 * scored against are tmatch[r*2+0], tmatch[r*2+1] (row index into t, -1 = unused term).
 * row_w[r] = weight of each term of that row (0.5/(n_terms*B) or 0.5/(n_terms*B*Ts), 1/.. for DINOLoss); terms = 2.
 * Mixup targets (DINOLoss, main_esvit.py:639-641): terms = 4, tmatch[r*4+j] and an individual weight term_w[r*4+j] per term
 * (row_w unused): row r's loss is sum_j w_j CE(teacher row j, student row r).  term_w = NULL selects the two-term form.
 * Outputs: row_loss fp32 [Rs] (sum over the row's terms, already weighted), ds dtype [Rs, K]
 * = d loss / d s (includes 1/student_temp).
 * row_order (optional, int32 [Rs], a permutation of the rows): the order in which workgroups take the rows -- the region loss
 * passes the image-major order so that the student rows of one image, which share their <= 98 teacher rows, run together and
 * re-read them from cache instead of HBM.  Results do not depend on it.
 * s_row_max / s_row_lse (optional pair, fp32 [Rs]): statistics of z = s / tau_s already known (esvit_rowstat_combine of the
 * last-layer GEMM's side output): lse(z) = s_row_max + s_row_lse and the kernel's first pass over the row is skipped.
 *
 * terms = 0: CLASS-INDEX cross-entropy (F.cross_entropy on a classifier's logits; the linear-probe sweep, eval_linear.py:262).
 * s fp32 [Rs, K] (dtype ESVIT_F32 only, K % 4 == 0, K >= 4): for G classifiers sharing a batch of B samples the logits [B, G*K] are
 * Rs = B*G such rows.  tmatch int32 [Rs]: the class of each row, in [0, K).  row_w fp32 [Rs]: the gradient scale of the row
 * (1 / (B * world) for a batch mean; may be NULL when ds is).  t, center, t_row_max, t_row_lse, term_w, row_order, s_row_max and
 * s_row_lse must be NULL; the temperatures are ignored.  Outputs: row_loss fp32 [Rs, 2] = (lse(z) - z_t, rank of the target), with
 * rank = #{j : z_j > z_t} + #{j < t : z_j == z_t}, the target's position in the stable descending order -- a count, exact as a float,
 * and "among the top k" is rank < k;  ds fp32 [Rs, K] = row_w[r] (softmax(z)_j - [j == t]).  ds may be s (in place) or NULL (no
 * gradient, s untouched).  A row with a NaN / inf logit or a class outside [0, K) gives loss NaN, rank K and a NaN gradient row, and
 * leaves every other row as it would have been.  No atomics: identical launches give identical bits.  Rows of up to
 * esvit_query(ESVIT_Q_PROBE_CE_REG_ROW) floats are held in registers by one wave; longer rows take a workgroup and three sweeps.
 *
 * terms = -1: DISTRIBUTION STATISTICS of softmax rows (the training-health monitor, esvit_amd/monitor.py; no loss, no gradient).
 * s dtype [Rs, K] (bf16 or fp32, K % 8 == 0, K < 2^24, 16-byte aligned): the rows; center fp32 [K] or NULL (student rows);
 * inv_student_temp > 0: the inverse temperature; s_row_max / s_row_lse fp32 [Rs] (REQUIRED): the rows' statistics
 * row_max = max_k z, row_lse = ln sum_k exp(z - row_max) of z = (s - center) * inv_student_temp, as esvit_teacher_row_stats /
 * esvit_rowstat_combine give them.  t, t_row_max, t_row_lse, tmatch, row_w, term_w and row_order must be NULL; inv_teacher_temp is
 * ignored.  With p = softmax(z):
 *   row_loss fp32 [Rs, 2] = (H(p_r) = row_lse - sum_k p_k (z_k - row_max) in nats, the lowest index of the maximal z as a float);
 *   ds: an fp32 buffer of esvit_query(ESVIT_Q_DIST_STATS, Rs, K) floats, 16-byte aligned, contents need not be initialised: its first K
 *       floats receive psum[k] = sum_r p_rk, the rest is scratch (partials per slab of rows and per block of columns, folded in a fixed order).
 * The rows are read once.  A row whose statistics or logits are NaN / inf gives H = NaN and index -1, and all K column sums are NaN;
 * the row outputs of every other row are what they would have been.  No atomics: identical launches give identical bits. */
int esvit_dino_ce_fwd_bwd(int dtype, const void* s, const void* t, const float* center,
                          const float* t_row_max, const float* t_row_lse, const int32_t* tmatch,
                          const float* row_w, int terms, const float* term_w, float inv_student_temp,
                          float inv_teacher_temp, int64_t Rs, int K, float* row_loss, void* ds, const int32_t* row_order,
                          const float* s_row_max, const float* s_row_lse, esvit_stream_t stream);
/* fold esvit_gemm_desc::rowstat (fp32 [R, nblocks, 2], base-2 block statistics) into natural-log row statistics, the outputs of
 * esvit_teacher_row_stats: row_max[r] = max_k z_k, row_lse[r] = log sum_k exp(z_k - row_max[r]) */
int esvit_rowstat_combine(const float* rowstat, int64_t R, int nblocks, float* row_max, float* row_lse, esvit_stream_t stream);
/* deterministic sum of row_loss -> loss[0] */
int esvit_sum_f32(const float* x, int64_t n, float* out, esvit_stream_t stream);
/* ds *= scale[0] (scale on device: grad_output of the scalar loss) */
int esvit_scale_inplace(int dtype, void* x, int64_t n, const float* scale, esvit_stream_t stream);
/* center EMA (main_esvit.py:651-660, 752-770): c = c*m + (1-m) * colsum / denom */
int esvit_center_ema(float* center, const float* colsum, float momentum, float denom, int K,
                     esvit_stream_t stream);

/* ---- fused update: per-parameter clip + optimizer rule + teacher EMA -------------
 * utils.py:106-115 (clip), the optimizers of main_esvit.py:408-415 as driven by :506-510,574, EMA main_esvit.py:587-590.
 *   ESVIT_RULE_ADAMW  torch.optim.AdamW          (beta1, beta2, eps as named)
 *   ESVIT_RULE_SGD    torch.optim.SGD(momentum)  (beta1 = momentum; beta2, eps unused): mu = momentum mu + (c g + wd p)
 *   ESVIT_RULE_LARS   utils.LARS (utils.py:519-557) (beta1 = momentum, beta2 = eta): mu = momentum mu + q (c g + wd p),
 *                     q = eta |p| / |c g + wd p| for tensors of group 0 (ndim != 1), 1 otherwise;  p -= lr mu
 *   ESVIT_RULE_SGD_MEMBERS  torch.optim.SGD(momentum, dampening 0, no nesterov) for independent MEMBERS (the classifiers of a
 *                     linear-probe sweep) in one launch (beta1 = momentum): mu = momentum mu + (g + wd p), p -= lr mu, with lr and wd
 *                     PER TENSOR from the table's slot 9, bits(lr) | bits(wd) << 32; the lr, wd, clip, beta2, eps, ema_m arguments,
 *                     the group slot, the teacher and the bf16 copies are ignored.  Bits 32.. of the flags slot hold the tensor's
 *                     member id; the non-finite guard is per member and `skipped` is REQUIRED: int32 [members] (see below).
 * (c = the clip factor of the tensor).  Tensor table (device, int64[ntensors*12]):
 *   [p, g, exp_avg (SGD: momentum_buffer, LARS: mu), exp_avg_sq (AdamW only), teacher_p (0 = none), numel,
 *    group (0: weight decay, 1: none), flags (bit0: has gradient; otherwise only the EMA is applied; bits 32..: member id, SGD_MEMBERS),
 *    bits(1-beta1^t) | bits(1-beta2^t) << 32 (AdamW), reserved (SGD_MEMBERS: bits(lr) | bits(wd) << 32),
 *    bf16 copy of p (0 = none), bf16 copy of teacher_p (0 = none)]   -- the copies are refreshed in the same pass
 * chunk table (device, int32[nchunks*2]): [tensor_id, chunk_index], chunk =
 * esvit_query(ESVIT_Q_UPDATE_CHUNK_ELEMS, 0, 0, 0) elements.
 * esvit_grad_sqnorm: stats = 1: sqnorms fp32 [ntensors] = sum g^2;  stats = 3 (LARS): fp32 [ntensors*3] =
 * (sum g^2, sum p^2, sum g p) per tensor.  esvit_fused_clip_update_ema reads the layout its rule needs.  Every chunk adds its
 * partial with a float atomicAdd: the statistic differs in the last bits from launch to launch.
 * stats | ESVIT_SQNORM_ORDERED (stats & 0xff in {1, 3} as above; any other value is ESVIT_ERR_ARG): no atomics and no memset --
 * sqnorms is then fp32 [ntensors * stats + nchunks * stats]: the head has the layout above (esvit_fused_clip_update_ema reads it
 * unchanged), the tail is scratch: chunk-table entry i writes its partial to tail[i * stats ..].  The chunk table must be sorted
 * by (tensor_id, chunk_index), which is how it is built anyway.  Summation order of one statistic: a thread adds its 16 products
 * in address order (four float4 of four), the 256 threads of the chunk are summed by a butterfly over the 64 lanes and then over the
 * four waves in wave order; a second launch (one workgroup per tensor) folds the tensor's partials: thread j of 256 adds the
 * partials j, j + 256, ... in chunk order, then the same butterfly and wave sum.  A chain of at most 16 + 6 + 4 additions in
 * the chunk and min(chunks - 1, ceil(chunks / 256) + 9) in the fold (absent partials enter as exact zeros), whatever the grid's
 * schedule: within the sequential bound (32 + chunks) * 2^-24 relative to the sum of the absolute terms.  A tensor without the
 * has-gradient bit gets 0.  The atomic form adds the same chunk partials in whatever order they arrive and meets the same bound.
 * Element contract (u = 2^-24; tests/update_ref.py counts the roundings behind every K, tests/test_update_gpu.py holds the kernels
 * to it): every output is within K u (sum of the absolute values of the relation's terms) of the relation evaluated exactly from the
 * launch's fp32 inputs, its fp32 scalars and the statistics the launch read, the later relations from the earlier outputs as stored:
 *   AdamW  m' = m + (1 - b1)(c g - m)  K = 7;   v' = b2 v + (1 - b2)(c g)^2  K = 12;
 *          p' = (1 - lr wd) p - (lr / bc1) m' / (sqrt(v') / sqrt(bc2) + eps)  K = 8
 *   SGD    mu' = momentum mu + (c g + wd p)  K = 6;    LARS  mu' = momentum mu + q (c g + wd p)  K = 16;    both  p' = p - lr mu'  K = 2
 *   EMA    t' = ema_m t + (1 - ema_m) p'  K = 2;    bf16 copies: round-to-nearest-even of the stored p' and t', exactly
 * with c = min(1, clip / (sqrt(sum g^2) + 1e-6)) (1 when clip == 0) and q = eta sqrt(sum p^2) / sqrt(c^2 sum g^2 + 2 c wd sum g p +
 * wd^2 sum p^2), 1 for group 1 and where either root is 0, both evaluated exactly from the statistics.  Against the exact sums the
 * statistics' bound B = (32 + chunks) u carries over: c within about B / 2 relative, q within (B (1 + cond) / 2 + 8 u) relative where
 * cond = (c^2 sum g^2 + 2 c wd sum|g p| + wd^2 sum p^2) / |c g + wd p|^2 >= 1.  That is the limit of taking |c g + wd p| from three
 * statistics instead of from the tensor, as the reference does: it cancels when c g ~ -wd p (cond large), and K = 16 of the LARS buffer
 * is counted for a radicand that does not (cond near 1, which is what gradients uncorrelated with their weights give).
 * A tensor without the has-gradient bit keeps p; its teacher and copies are still refreshed.  lr == 0 keeps p bit for bit while the
 * moments move, ema_m == 1 keeps the teacher, ema_m == 0 makes it p'.  g is never written, and nothing is written through a zero slot.
 * Non-finite guard: if ANY statistic is NaN / inf (a non-finite loss poisons every gradient) the update launch is a no-op --
 * student, moments, teacher and weight copies keep their values (the reference exits before its update, main_esvit.py:546-551);
 * `skipped` (device int32, may be NULL) is then incremented by one, so that a host that looks at the loss only now and then can still
 * count the updates that did not happen (a gradient overflow with a finite loss) and correct its step counters.
 * ESVIT_RULE_SGD_MEMBERS narrows the guard to the member: a non-finite statistic of ANY tensor of member m (its weight, its bias)
 * makes the update of m's tensors a no-op and adds one to skipped[m]; every other member is updated as if m were not in the launch.
 * A member whose counter is non-zero stays frozen -- later launches leave it alone and keep counting -- until the caller clears
 * skipped[m].  The statistics are esvit_grad_sqnorm(stats = 1). */
#define ESVIT_RULE_ADAMW 0
#define ESVIT_RULE_SGD 1
#define ESVIT_RULE_LARS 2
#define ESVIT_RULE_SGD_MEMBERS 3
#define ESVIT_SQNORM_ORDERED 0x100
int esvit_grad_sqnorm(const int64_t* tensors, int ntensors, const int32_t* chunks, int nchunks, int stats,
                      float* sqnorms, esvit_stream_t stream);
int esvit_fused_clip_update_ema(int rule, const int64_t* tensors, int ntensors, const int32_t* chunks, int nchunks,
                                const float* sqnorms, float clip, float lr, float wd, float beta1,
                                float beta2, float eps, float ema_m, int32_t* skipped, esvit_stream_t stream);

/* ---- CvT backbone pieces (BASELINE config 5) ------------------------------
 * Token-major NHWC activations.  cvt_v4_transformer.py:349-382 (ConvEmbed), :75-105 (DepthWiseConv2d = dw 3x3 +
 * BatchNorm2d + 1x1), :44-46 (QuickGELU: see ESVIT_EPI_QGELU).
 * esvit_conv_im2col: cols[(b,oy,ox)][(ky*k+kx)*Cin + c] = src(b, oy*stride-pad+ky, ox*stride-pad+kx, c), zero outside
 *   the image and in the tail columns [k*k*Cin, Kpad); src = fp32 NCHW images (nchw=1) or activation-dtype NHWC tokens.
 * esvit_conv_col2im: the adjoint, dsrc fp32 NHWC [nB,H,W,Cin].
 * esvit_dwconv3x3: y[b,y,x,c] = sum_t w[c][t] x[b,y+ky-1,x+kx-1,c] (stride 1, zero pad 1); flip=1 applies the taps
 *   mirrored (the data gradient).  esvit_dwconv3x3_wgrad: dw[c][t]; ws: fp32 [ESVIT_Q_COL_REDUCE_BLOCKS(rows)*9*C].
 * esvit_col_sums2: out[0..C) = sum_r a[r][c], out[C..2C) = sum_r a[r][c]*b[r][c]  (BatchNorm statistics: b = a;
 *   BatchNorm backward: a = dy, b = pre-norm activations); ws: fp32 [ESVIT_Q_COL_REDUCE_BLOCKS(rows)*2*C].
 * esvit_col_affine2: act 0: y = a1[c]*x1 + a2[c]*x2 + a3[c]  (x2 may be null);
 *   act 1: y = GELU(a1[c]*x1 + a3[c]) and act 2: y = x2 * GELU'(a1[c]*x1 + a3[c]) -- BatchNorm1d + GELU of DINOHead(use_bn=True)
 *   (vision_transformer.py:391-402) and its backward, the normalised value rebuilt from the pre-norm activation;
 *   act 3: y = max(a1[c]*x1 + a3[c], 0) and act 4: y = x2 where a1[c]*x1 + a3[c] > 0, else 0 -- BatchNorm2d + ReLU of the
 *   residual stem (cvt_v4_transformer.py:385-430) and its backward.
 * Widths and alignment (refused with ESVIT_ERR_ARG, nothing is launched): esvit_col_sums2 takes any C % 4 == 0; esvit_dwconv3x3
 *   and esvit_dwconv3x3_wgrad take C % 4 == 0 up to 1024, and bf16 with C % 8 == 0 and 16-byte aligned tensors up to 2048.
 *   These three move four channels per load: x, y, dy, a, b must be aligned to 8 bytes in bf16 and 16 in fp32 (ws: 16).
 *   esvit_pad_crop_tokens wants src and dst on 16 bytes.  The BatchNorm variance is sum(d^2)/n - mean^2 in fp32: the relative
 *   error of rstd grows as 8 (1 + (mean/std)^2) 2^-24 (tests/test_conv_gpu.py holds it to that).
 *
 * GROUPED MODE of esvit_pad_crop_tokens, esvit_dwconv3x3, esvit_col_sums2 and esvit_col_affine2 (the ragged multi-crop route of
 *   CvT: the resolution groups of a step differ in their grid, not in C or dtype).  A NEGATIVE batch / row count -G, 1 <= G <= 4,
 *   turns the entry's FIRST pointer argument (src / x / a / x1) into a HOST array of G esvit_grid_group records; ONE launch then
 *   does what the G separate calls on the records would do, bit for bit.  The entry copies the records into the kernel's
 *   argument block: the array may be reused as soon as the call returns, there is no device-side table, allocation or sync.
 *   Fields of a record:   pad_crop_tokens: p0 = src, out = dst, (nB, H, W) the source grid, (Hd, Wd) the destination grid
 *                         dwconv3x3:       p0 = x, out = y, (nB, H, W)
 *                         col_sums2:       p0 = a, p1 = b, rows = nB*H*W
 *                         col_affine2:     p0 = x1, p1 = x2 (or NULL), out = y, a1 / a2 / a3 this group's coefficients, rows = nB*H*W
 *   Every record carries the entry's C and dtype (they must equal the entry's arguments).  Arguments of the entry that a record
 *   replaces (H, W, Hs.., dst / y / b / x2 / a1..a3) are ignored; w, flip, act, ws and the stream are shared.
 *   esvit_col_sums2: out is fp32 [G][2*C]; group g keeps the ESVIT_Q_COL_REDUCE_BLOCKS(rows_g) partition and the reduction order of
 *   the plain call on that group alone; ws: fp32 [sum_g ESVIT_Q_COL_REDUCE_BLOCKS(rows_g) * 2*C], the groups' partials one after the
 *   other.  Grouped esvit_col_sums2 takes C <= 1024; grouped esvit_dwconv3x3 wants all records on the same side of the 16-byte
 *   test that selects its strip kernel.  Everything the plain call refuses is refused per record, before anything is launched. */
typedef struct esvit_grid_group {
    const void* p0;
    const void* p1;
    void* out;
    const float* a1;
    const float* a2;
    const float* a3;
    int32_t nB, H, W;
    int32_t Hd, Wd;
    int32_t C, dtype;
    int32_t reserved; /* 0 */
} esvit_grid_group;
#define ESVIT_MAX_GRID_GROUPS 4
int esvit_conv_im2col(int dtype, const void* src, int nchw, int nB, int H, int W, int Cin, int k, int stride, int pad,
                      int Ho, int Wo, int Kpad, void* cols, esvit_stream_t stream);
int esvit_conv_col2im(int dtype, const void* dcols, int nB, int H, int W, int Cin, int k, int stride, int pad, int Ho,
                      int Wo, int Kpad, float* dsrc, esvit_stream_t stream);
int esvit_dwconv3x3(int dtype, const void* x, const float* w, int flip, int nB, int H, int W, int C, void* y,
                    esvit_stream_t stream);
int esvit_dwconv3x3_wgrad(int dtype, const void* x, const void* dy, int nB, int H, int W, int C, float* dw, float* ws,
                          esvit_stream_t stream);
int esvit_col_sums2(int dtype, const void* a, const void* b, int64_t rows, int C, float* out, float* ws,
                    esvit_stream_t stream);
int esvit_col_affine2(int dtype, const void* x1, const void* x2, int64_t rows, int C, const float* a1, const float* a2,
                      const float* a3, int act, void* y, esvit_stream_t stream);
/* token grid [nB,Hs,Ws,C] -> [nB,Hd,Wd,C]: zero-pad at the bottom / right (F.pad of cvt_v4_transformer.py:173) or crop (:216) */
int esvit_pad_crop_tokens(int dtype, const void* src, int nB, int Hs, int Ws, int Hd, int Wd, int C, void* dst,
                          esvit_stream_t stream);
/* BatchNorm2d coefficient vectors (nn.BatchNorm2d of cvt_v4_transformer.py:95; eps 1e-5, momentum 0.1).
 * fwd:  sums = [sum d | sum d^2] over n positions (already summed over the ranks for SyncBatchNorm) ->
 *       coef fp32 [4*C] = [a | shift | mean | rstd], y = a*d + shift; running_mean / running_var (both or neither) are
 *       updated in place with the unbiased variance.   eval: the same coef from the running statistics.
 * bwd:  esvit_bn_bwd_local: sums = [sum dy | sum dy*d] -> red = [sum dy | sum dy*xhat] (= this rank's d beta | d gamma);
 *       esvit_bn_bwd_coeffs: red summed over the ranks (NULL = eval statistics) -> abc = [A | B | C], d(d) = A*dy + B*d + C. */
int esvit_bn_fwd_coeffs(const float* sums, float n, const float* gamma, const float* beta, float eps, float momentum,
                        float* running_mean, float* running_var, int C, float* coef, esvit_stream_t stream);
int esvit_bn_eval_coeffs(const float* running_mean, const float* running_var, const float* gamma, const float* beta,
                         float eps, int C, float* coef, esvit_stream_t stream);
int esvit_bn_bwd_local(const float* sums, const float* coef, int C, float* red, esvit_stream_t stream);
int esvit_bn_bwd_coeffs(const float* red, float n, const float* gamma, const float* coef, int C, float* abc,
                        esvit_stream_t stream);

/* ---- crop producer ------------------------------------------------------ */
/* DataAugmentationDINO (datasets/build.py:203-261; utils.py:43-75 GaussianBlur / Solarization) for n crops of ONE output size S,
 * given their random draws: img.crop(box).resize((S, S), BICUBIC) -> horizontal flip -> ColorJitter (Brightness / Contrast /
 * Color / hue in the drawn order) -> grayscale -> GaussianBlur -> solarize -> ToTensor -> Normalize(ImageNet mean / std).
 * Bit-exact with Pillow's 8-bit arithmetic (Resample.c, Blend.c, Convert.c, BoxBlur.c) at every stage.
 *   src     uint8, decoded RGB images, HWC, packed back to back (the buffer must be readable up to the next 4-byte boundary
 *           past its last pixel);  images  int64 [n_img, 3] = (byte offset into src, H, W)
 *   params  int32 [n, ESVIT_AUG_PARAM_INTS], one row per crop:
 *           0 image row | 1 top | 2 left | 3 h | 4 w  (crop box, inside the image) | 5 flip
 *           6..9  jitter operations in application order: 0 brightness, 1 contrast, 2 saturation, 3 hue, -1 none
 *           10 brightness | 11 contrast | 12 saturation factor (float bits) | 13 hue shift = uint8(hue_factor * 255)
 *           14 grayscale | 15 box radius + 1 of the blur (0 = no blur) | 16 ww | 17 fw (BoxBlur.c fixed-point weights of the
 *           Gaussian radius) | 18 solarize | 19.. reserved (0)
 *   n       crops in this call, <= 65535;  S  output size, a multiple of 4, <= 280;  max_h, max_w  the largest box of the n crops (sizes the LDS of the resize;
 *           <= esvit_query(ESVIT_Q_AUG_MAX_BOX, S, 0, 0))
 *   planes  uint8 scratch of n * (3 S^2 + 4) bytes: on return its first n * 3 S^2 bytes are the resized, flipped crops
 *           [n, 3, S, S] before the jitter;  out  fp32 [n, 3, S, S] */
#define ESVIT_AUG_PARAM_INTS 24
int esvit_aug_crops(const uint8_t* src, const int64_t* images, const int32_t* params, int n, int S, int max_h, int max_w,
                    uint8_t* planes, float* out, esvit_stream_t stream);

/* Evaluation mode (S | ESVIT_AUG_EVAL, planes = NULL): the transforms of eval_knn.py:48-53 / eval_linear.py:50-61 for n crops
 * of one output size S, bit-exact with Pillow, in one launch and without scratch (the flag without planes == NULL is ESVIT_ERR_ARG):
 * img.crop(box).resize((rw, rh), filter) -> the S x S window at (off_y, off_x) of it -> horizontal flip -> ToTensor -> Normalize.
 * Resize(256, BICUBIC) -> CenterCrop(224) is box = the image, (rh, rw) = the resized size, the window offset the centre crop's;
 * RandomResizedCrop(224) -> RandomHorizontalFlip is box = the drawn box, rh = rw = S, offset 0, BILINEAR.
 *   params  int32 [n, ESVIT_RESIZE_PARAM_INTS], one row per crop:
 *           0 image row | 1 top | 2 left | 3 h | 4 w  (box, inside the image) | 5 flip | 6 rh | 7 rw  (size the box is resized to)
 *           8 off_y | 9 off_x  (window, off + S <= resized size) | 10 filter (ESVIT_FILTER_*) | 11.. reserved (0)
 *   n       <= 65535;  S  <= 4096
 *   max_h, max_w  the largest h / rh and w / rw of the n crops in units of 1 / ESVIT_RESIZE_SCALE_ONE, rounded up (they size the
 *           LDS; ESVIT_ERR_UNSUPPORTED, and no launch, when esvit_query(ESVIT_Q_RESIZE_FITS) says no)
 *   out     fp32 [n, 3, S, S] */
#define ESVIT_AUG_EVAL 0x40000000
#define ESVIT_RESIZE_PARAM_INTS 16
#define ESVIT_RESIZE_SCALE_ONE 65536
#define ESVIT_FILTER_BICUBIC 0
#define ESVIT_FILTER_BILINEAR 1

/* ---- JPEG decoder (the input side of the crop producer) ------------------
 * The reference decodes every file with Image.open(f).convert('RGB') (datasets/build.py ImageFolder, the zip and TSV readers).
 * esvit_jpeg_decode decodes a batch of baseline Huffman JPEGs (SOF0 / SOF1, 8-bit; grayscale or YCbCr 4:4:4 / 4:2:2 / 4:2:0;
 * restart intervals; any size) into the packed HWC RGB images esvit_aug_crops reads, bit-exact with Pillow's default decode.
 * The caller (esvit_amd/jpeg.py) has parsed the headers and laid the batch out; every array below is device memory:
 *   images    int32 [n_images, ESVIT_JPEG_IMG_INTS]: H, W, ncomp (0: not decoded here -- its slot is filled by the caller), hmax,
 *             vmax, MCUs per row, MCU rows, blocks per MCU, restart interval, first segment, segments, first coefficient block,
 *             first plane byte, blocks, plane bytes, status bits to report as they are; from int 16, per component (12 ints):
 *             h, v, quant table, DC table, AC table, block columns, block rows, first block, first plane byte, downsampled width,
 *             downsampled height, 0
 *   segments  int32 [n_segments, ESVIT_JPEG_SEG_INTS]: image, entropy-coded bits, byte offset in `scan`, first MCU, MCUs, first lane,
 *             lanes (= max(1, ceil(bits / ESVIT_JPEG_LANE_BITS)))
 *   lane_seg  int32 [n_lanes]: the segment of every lane (a segment's lanes are consecutive)
 *   huff      int32 [*, ESVIT_JPEG_HUFF_INTS]: 9-bit lookup (length << 8 | symbol), maxcode[18], value offsets[18], symbols[256]
 *   quant     int32 [*, 64] quantisation tables in natural order
 *   scan      uint8: the un-stuffed entropy-coded data of every segment, each 4-byte aligned and followed by >= 8 zero bytes
 *   table     int64 [n_images, 3] (byte offset in `out`, H, W) -- the esvit_aug_crops image table
 *   out       uint8 packed HWC RGB images;  status  int32 [n_images]: the host bits | 1 where the entropy data is corrupt
 * mode: ESVIT_JPEG_PARALLEL (self-synchronising parallel entropy decode, bounded by max_passes sync passes (0: the default, 8; at most 64) and
 * ending in the serial decode of any segment that has not converged) or ESVIT_JPEG_SERIAL (one lane per segment: the reference).
 * workspace: esvit_query(ESVIT_Q_JPEG_WORKSPACE, n_blocks, plane_bytes, n_lanes | n_segments << 32) bytes. */
#define ESVIT_JPEG_IMG_INTS 64
#define ESVIT_JPEG_SEG_INTS 8
#define ESVIT_JPEG_HUFF_INTS 832
#define ESVIT_JPEG_LANE_BITS 4096
#define ESVIT_JPEG_PARALLEL 0
#define ESVIT_JPEG_SERIAL 1
typedef struct {
    int32_t n_images, n_segments, n_lanes, n_blocks;
    int64_t plane_bytes;
    const int32_t* images;
    const int32_t* segments;
    const int32_t* lane_seg;
    const int32_t* huff;
    const int32_t* quant;
    const uint8_t* scan;
    const int64_t* table;
    uint8_t* out;
    int32_t* status;
    int32_t mode;
    int32_t max_passes;
} esvit_jpeg_desc;
int esvit_jpeg_decode(const esvit_jpeg_desc* d, void* workspace, size_t ws_bytes, esvit_stream_t stream);

/* ---- global attention of the monolithic ViT backbones --------------------- */
/* models/vision_transformer.py:67-94 (Attention.forward of deit_tiny / deit_small / vit_base): the score matrix lives in HBM
 * and the products run on esvit_gemm (batch = B * nH); these are the layout changes and the row softmax around them.
 *   esvit_heads_split   x [B * N, parts * nH * hd] token-major (the qkv GEMM output: parts = 3; a gradient of the merged heads:
 *                       parts = 1)  ->  y [parts, B, nH, Np, hd], rows N..Np-1 zero        (:76, reshape + permute)
 *   esvit_heads_merge   the inverse, dropping the pad rows                                   (:83, transpose + reshape)
 *   esvit_softmax_rows_fwd   in place over s [batch, Np, Np]: softmax(scale * s[:, :N, :N]) along the last axis, zero on pad rows
 *                       and columns (Np <= 256)                                              (:79-80)
 *   esvit_softmax_rows_bwd   in place over dp: scale * p o (dp - sum_j p_j dp_j), zero on pad rows and columns */
int esvit_heads_split(int dtype, const void* x, int B, int N, int Np, int nH, int hd, int parts, void* y, esvit_stream_t stream);
int esvit_heads_merge(int dtype, const void* y, int B, int N, int Np, int nH, int hd, int parts, void* x, esvit_stream_t stream);
int esvit_softmax_rows_fwd(int dtype, void* s, int64_t batch, int N, int Np, float scale, esvit_stream_t stream);
int esvit_softmax_rows_bwd(int dtype, const void* p, void* dp, int64_t batch, int N, int Np, float scale, esvit_stream_t stream);
/* Vision Longformer's sliding-chunk attention (models/vision_longformer.py AttnBlock 'longformerhand' -> layers/longformer2d.py:138-262
 * with layers/slidingchunk_2d.py, mode 0, exact 0, rpe off, shared global weights) on the same route: the row softmax restricted to
 * the keys a query may see.  chunk int32 [N]: -1 for a global token, else (chunk row << 16) | chunk column of the token's w x w
 * chunk; a query sees all global tokens and the local tokens of its own and the eight adjacent chunks (the reference's zero-padded
 * and out-of-range positions are exactly the ones that do not exist here); a global query sees every token (longformer2d.py:310-327).
 * Masked entries of P are zero, so the backward needs no mask for correctness.  nglo / chunk_row_tokens (optional, 0 = unknown)
 * describe the token order -- nglo global tokens, then the local tokens chunk row by chunk row, chunk_row_tokens (= w * grid width)
 * per chunk row: the kernels then read only the global columns and the three chunk rows around the query's own (everything else is
 * written as zero unread). */
int esvit_softmax_rows_chunked_fwd(int dtype, void* s, int64_t batch, int N, int Np, float scale, const int32_t* chunk, int nglo,
                                   int chunk_row_tokens, esvit_stream_t stream);
int esvit_softmax_rows_chunked_bwd(int dtype, const void* p, void* dp, int64_t batch, int N, int Np, float scale, const int32_t* chunk,
                                   int nglo, int chunk_row_tokens, esvit_stream_t stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* ESVIT_HIP_H */
