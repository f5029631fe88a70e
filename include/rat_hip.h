/* rat_hip.h — C ABI of librat_hip.so: the MI355X (gfx950) hot path of RAT_m2.
 *
 * The reference (YushenLi807/WWW24-RAT) is pure Python on torch ATen and has no FFI; the drop-in boundary
 * is its FuxiCTR model-plugin API (run_expid.py:75-76 -> fuxictr/pytorch/models/RAT_m2.py).  This header is
 * what a ctypes binding inside that plugin calls instead of the ATen op sequences cited per entry point.
 * All paths below are relative to /root/reference.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer unless the name ends in _host; the caller (PyTorch's allocator)
 *    owns every buffer including workspaces; the library allocates and frees nothing;
 *  - every call is asynchronous on `stream` (a hipStream_t passed as void*), never synchronises the
 *    device, is re-entrant and keeps no global mutable state (forward runs on the Python main thread,
 *    backward on autograd's device thread);
 *  - return value 0 = launched, negative = rejected (message via rat_last_error(), thread-local);
 *  - results are fp32; the default arithmetic of the encoder / head GEMMs is RAT_ARITH_BF16X3 (3-way bf16 split, six of the
 *    nine cross products, fp32 accumulate: fp32-class, not bit-identical to an fp32 FMA chain), RAT_ARITH_F32 selects exact
 *    IEEE fp32 MFMA; everything else (softmax, LayerNorm, GELU, optimizer) is IEEE fp32; ids are int32; token grids are row-major [B][T][S][d]
 *    (sample-in-batch, target||retrieved sample, label||field token, embedding dim).
 */
#ifndef RAT_HIP_H_
#define RAT_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RAT_ABI_VERSION 9
#define RAT_ARITH_F32 0        /* arithmetic selectors of the encoder GEMMs: see rat_attn_fwd_ex */
#define RAT_ARITH_BF16X3 1

int rat_version(void);
const char* rat_last_error(void);

/* One feature field (fuxictr/features.py:46-57 feature_specs entry + its nn.Embedding,
 * fuxictr/pytorch/layers/embedding.py:76-95).  `width` is the table's row length (embedding_dim, or 1 for
 * the LR "wide" tables of fuxictr/pytorch/layers/shallow.py:23-45). */
typedef struct RatField {
    float* table;        /* [vocab][width] weights (forward) or gradient table (backward) */
    int32_t col;         /* first input column (feature_specs[f]["index"]) */
    int32_t ncols;       /* 1 for categorical, max_len for a MaskedSumPooling bag (sequence.py:32-38) */
    int32_t vocab;
    int32_t padding_idx; /* -1 = none; rows with this id receive no gradient (nn.Embedding padding_idx) */
} RatField;

/* ---- K1: token-grid assembly -------------------------------------------------------------------------
 * replaces RAT_m2.forward lines 113-126 (RAT_m2.py): 3x EmbeddingLayer.forward (embedding.py:40-43,
 * 158-178, 138-156), 2x label_embedding_layer, 3x torch.concat.
 * idx [B][T][L] int32, label_ids [B][T] int32 (2 for the target row, the retrieved label otherwise),
 * fields_dev: device array of nfields RatField, label_table [3][d], grid out [B][T][1+nfields][d]. */
int rat_gather_fwd(const int32_t* idx, const int32_t* label_ids, const RatField* fields_dev, int nfields,
                   const float* label_table, float* grid, int B, int T, int L, int d, void* stream);

/* rat_gather_fwd for field sets with MaskedAveragePooling sequence fields: replaces the same lines plus
 * MaskedAveragePooling.forward (sequence.py:24-29, chosen by embedding.py:113-121).  modes_dev: device int32 [nfields],
 * 0 = MaskedSumPooling / categorical, 1 = MaskedAveragePooling; an averaged field's grid row is, per element c,
 * sum_i E[id_i][c] / ((float)#{i : E[id_i][c] != 0} + 1e-16f).  modes_dev = NULL is rat_gather_fwd exactly. */
int rat_gather_fwd_pool(const int32_t* idx, const int32_t* label_ids, const RatField* fields_dev, const int32_t* modes_dev,
                        int nfields, const float* label_table, float* grid, int B, int T, int L, int d, void* stream);

/* backward of MaskedAveragePooling (autograd's DivBackward of sequence.py:27, the count a constant), run before the table-gradient
 * stage (rat_gather_bwd or rat_sparse_reduce_grid): the rows of dgrid [B][T][S][d] of the averaged fields avg_fields_dev
 * (device int32 [navg], field indices) and their target rows of dflat (nullable, [B][nfields*d]) are divided IN PLACE by the
 * forward's per-element denominators, recomputed from fields_dev (the forward's tables, unchanged since the forward). */
int rat_pool_scale_bwd(float* dgrid, float* dflat, const int32_t* idx, const RatField* fields_dev, const int32_t* avg_fields_dev,
                       int navg, int nfields, int B, int T, int L, int d, void* stream);

/* backward of the above (autograd's embedding_dense_backward + cat/stack backward, base_model.py:223).
 * dgrid [B][T][S][d]; dflat (nullable) [B][nfields*d] = gradient of the DNN branch input X_emb.flatten(1)
 * (RAT_m2.py:145-146), added onto the target rows; grad tables are ACCUMULATED into (caller zeroes them);
 * dlabel_table [3][d] is accumulated too. */
int rat_gather_bwd(const float* dgrid, const float* dflat, const int32_t* idx, const int32_t* label_ids,
                   const RatField* grad_fields_dev, int nfields, float* dlabel_table,
                   int B, int T, int L, int d, void* stream);

/* nn.Embedding raises IndexError for an id outside [0, vocab) (embedding.py:158-178 -> F.embedding); the kernels above
 * clamp such ids (and labels outside {0,1,2}) for memory safety only.  rat_check_ids makes the error visible without a
 * per-step host synchronisation: counts[0] += number of feature ids outside their table, counts[1] += number of label ids
 * outside {0,1,2} (device int32[2], caller zeroes it once and reads it at its next synchronisation point). */
int rat_check_ids(const int32_t* idx, const int32_t* label_ids, const RatField* fields_dev, int nfields, int B, int T,
                  int L, int32_t* counts, void* stream);

/* ---- a1 / a2 on the device: inputs_to_device + the label-token rule for a batch that already sits in HBM (ABI v8) --------------
 * base_model.py:125-133, RAT_m2.py:110-118.  X [B][T][L] (x_type: RAT_DTYPE_*, integer-valued) -> idx int32; y [B][T] (fp32 / fp64)
 * -> label_ids int32 (2 in column 0, the retrieved sample's label elsewhere) and y_true fp32 [B] (= y[:, 0]).  One launch. */
#define RAT_DTYPE_I32 0
#define RAT_DTYPE_I64 1
#define RAT_DTYPE_F32 2
#define RAT_DTYPE_F64 3
int rat_batch_prepare(const void* X, int x_type, const void* y, int y_type, int32_t* idx, int32_t* label_ids, float* y_true,
                      int B, int T, int L, void* stream);

/* ---- K0: device-side batch assembly ---------------------------------------------------------------------
 * replaces Dataset.__getitem__ + default_collate + inputs_to_device for retrieval-augmented batches
 * (fuxictr/pytorch/data_generator.py:66-78, 239-241; base_model.py:125-133): the encoded query table
 * data_ids [Q][L] / data_labels [Q], the retrieval pool pool_ids [N][L] / pool_labels [N] and the pre-computed
 * neighbour lists retr_indices [Q][K] (negative = counted from the end of the pool, numpy semantics) are resident
 * in HBM; rows [B] selects the batch.  Outputs are exactly rat_gather_fwd's inputs: idx [B][1+K][L],
 * label_ids [B][1+K] (2 for the target row, the neighbour's label otherwise), plus y_true [B]. */
int rat_batch_assemble(const int32_t* data_ids, const float* data_labels, const int32_t* pool_ids,
                       const float* pool_labels, const int64_t* retr_indices, const int64_t* rows, int32_t* idx,
                       int32_t* label_ids, float* y_true, int64_t Q, int64_t N, int B, int K, int L, void* stream);

/* ---- K2: attention phase of CrossIntraEncoderBlock --------------------------------------------------
 * y = Attention(LayerNorm(x)) + x over groups of L tokens (RAT_m2.py:155-161, 176-202, 222-230).
 * Sequence q in [0, nseq) owns tokens  tok(q, p) = (q / q_div) * hi_stride + (q % q_div) * lo_stride
 * + p * pos_stride, p in [0, L)  (token units; a token is d floats).  Intra-sample attention over the
 * grid: nseq=B*T, L=S, q_div=nseq, lo_stride=S, pos_stride=1.  Cross-sample: nseq=B*S, L=T, q_div=S,
 * hi_stride=T*S, lo_stride=1, pos_stride=S — the reference's reshape/transpose/flatten copy
 * (RAT_m2.py:226-227) becomes this addressing. */
typedef struct RatSeqMap {
    int64_t nseq;
    int32_t L;
    int32_t queries; /* ABI v5 (the padding of v4): 0 or >= L — every position is a query.  0 < queries < L — only the outputs of
                      * positions [0, queries) of each sequence are wanted: the forward may leave the other rows of y / o_save /
                      * lse_save with unspecified (finite) contents, and the backward REQUIRES the dy rows of the other positions
                      * to be zero (their queries contribute nothing; all positions still serve as keys and values, and dx is
                      * complete).  The bf16x3 kernels skip the work; every other kernel computes all positions, which the
                      * contract allows.  Used for the last encoder block, of whose output only x[:, 0][:, 0] is read
                      * (RAT_m2.py:138-140). */
    int64_t q_div, hi_stride, lo_stride, pos_stride;
} RatSeqMap;

typedef struct RatAttnParams {      /* HOST struct of device pointers; state_dict names under          */
    float* ln_g;  /* [d]      encoder.encoder.<i>.<which>_attention.norm.weight                          */
    float* ln_b;  /* [d]      ...norm.bias                                                               */
    float* w_qkv; /* [3*h*dh][d]  ...fn.to_qkv.weight (no bias)                                          */
    float* w_out; /* [d][h*dh]    ...fn.to_out.0.weight, NULL when heads==1 && dim_head==d (Identity)    */
    float* b_out; /* [d]          ...fn.to_out.0.bias                                                    */
    void* planes; /* optional, RAT_ARITH_BF16X3 only: the bf16x3 fragment planes of w_qkv / w_out (rat_attn_planes_bytes bytes,
                   * 16-byte aligned) as written by rat_split_weights_batch from the jobs of rat_attn_split_jobs — valid until
                   * the weights change.  NULL: rat_attn_fwd_ex / rat_attn_bwd_ex derive them themselves (2 - 3 small launches
                   * per call).  Ignored in the struct that receives gradients. */
    const uint64_t* drop_seed_dev; /* ABI v6, optional: DEVICE location of this layer's dropout seed (one of the words rat_dropout_seeds
                   * writes).  When set, rat_attn_fwd_ex / rat_attn_bwd_ex read the seed there and ignore their `dropout_seed` argument:
                   * a training step captured into a hipGraph then draws a new mask on every replay.  NULL: the by-value seed. */
} RatAttnParams;

/* ---- bf16x3 weight planes, once per optimizer step instead of once per call ------------------------------------------------
 * The bf16x3 kernels read every weight matrix as pre-split fragment-major planes.  The planes depend on the
 * weights only, so a training step needs them once: collect the jobs of every layer (rat_attn_split_jobs / rat_ffn_split_jobs
 * fill in what to split where inside that layer's `planes` buffer), run them all in ONE launch (rat_split_weights_batch) and
 * hand the buffers to the forward and backward entry points (RatAttnParams.planes, the `planes` argument of rat_ffn_bwd_res).
 * rat_*_planes_bytes return 0 and rat_*_split_jobs return 0 jobs when no bf16x3 kernel serves the shape. */
typedef struct RatSplitJob {
    const float* w; /* source matrix, row-major with leading dimension ld                                   */
    void* out;      /* fragment planes of B[k][n] = transpose ? w[k*ld + n] : w[n*ld + k], n < N, k < K       */
    int32_t N, K, ld, transpose, perm; /* perm: bit 0 = the k order of stacked accumulator tiles (rat_ffn_split_jobs); bits 8-19 `blk`, bits 20-31
                       * `stride` (ABI v9, 0 = off): the job reads `blk` consecutive ROWS of w out of every `stride` — row i -> (i / blk) * stride +
                       * i % blk — a head group's Q | K | V rows in place (rat_attn_groups_split_jobs) */
    int32_t reserved; /* 0, or n_valid | k_valid << 16: the matrix has only n_valid of the N rows / k_valid of the K columns the planes
                       * cover (0 = all); the rest is written as zeros.  Filled in by rat_*_split_jobs for layers narrower than the
                       * kernels' tiles (embedding_dim 40 / 48 / 56 inside the 64-wide bf16x3 tiles). */
} RatSplitJob;
size_t rat_attn_planes_bytes(int d, int heads, int dim_head);
int rat_attn_split_jobs(const RatAttnParams* w_host, int d, int heads, int dim_head, void* planes, RatSplitJob* jobs_out /* [4] */);
size_t rat_ffn_planes_bytes(int d, int hidden);
int rat_ffn_split_jobs(const float* w1, const float* w2, int d, int hidden, void* planes, RatSplitJob* jobs_out /* [3] */);
int rat_split_weights_batch(const RatSplitJob* jobs_host, int njobs, void* stream);

/* o_save [ntok][h*dh] (attention output before to_out) and lse_save [ntok][h] (log2-domain log-sum-exp of the
 * scaled scores), token-indexed like x, are written when non-NULL (training) and consumed by rat_attn_bwd. */
int rat_attn_fwd(const float* x, float* y, float* o_save, float* lse_save, const RatAttnParams* w_host,
                 const RatSeqMap* map_host, int d, int heads, int dim_head, float ln_eps, void* stream);

size_t rat_attn_bwd_workspace(int d, int heads, int dim_head);
/* dx = dL/dx (overwritten), grads_host->* overwritten with the batch-summed parameter gradients. */
int rat_attn_bwd(const float* x, const float* dy, const float* o_save, const float* lse_save, float* dx,
                 const RatAttnParams* w_host, const RatAttnParams* grads_host, float* workspace,
                 size_t workspace_bytes, const RatSeqMap* map_host, int d, int heads, int dim_head,
                 float ln_eps, void* stream);

/* The same kernels with the three constants of `PreNorm(Attention)(x) + x` exposed — RAT_m3's block (RAT_m3.py:164-243) runs two
 * attentions on the same input and averages them, with heads/2 heads of width 2*dim_head but the softmax scale of dim_head:
 *   y = out_scale * to_out(softmax(Q K^T * softmax_scale) V) + res
 * res: residual source — x (rat_attn_fwd), y itself (accumulate onto the first attention's result), or NULL;
 * softmax_scale <= 0 selects dim_head^-0.5.  Backward: the gradient through the projection is out_scale * dy and
 * dx = add + LayerNorm-backward(...), add = dy (rat_attn_bwd), another tensor laid out like dx (may alias dx), or NULL.
 *
 * arith selects the arithmetic of the projections (the GEMMs; the softmax core is the same fp32 VALU code either way):
 *   RAT_ARITH_F32     v_mfma_f32_16x16x4_f32: exact fp32, bit-identical to a k-ordered fmaf chain (what rat_attn_fwd / _bwd use);
 *   RAT_ARITH_BF16X3  v_mfma_f32_16x16x32_bf16 on operands split EXACTLY into three bf16 chunks, the six cross products of weight
 *                     >= 2^-16, fp32 accumulation: fp32-class accuracy (the dropped terms are <= 2^-23 of each product — one fp32
 *                     rounding; measured against fp64 in tools/probes/bf16x3_probe.hip) at 2.4x the fp32-MFMA rate.  Compiled for
 *                     the north-star geometry (embedding_dim 64, 8 heads x 10); any other shape runs RAT_ARITH_F32 regardless.
 * The forward needs rat_attn_fwd_workspace() bytes of workspace for the pre-split weight fragments under RAT_ARITH_BF16X3
 * (NULL / too small: exact fp32); the backward's rat_attn_bwd_workspace() already covers its own.
 *
 * dropout_p > 0: the nn.Dropout behind the output projection (Attention.to_out = Sequential(Linear, Dropout), RAT_m2.py:186-189):
 *   y = out_scale * Dropout(to_out(...)) + res, mask(token, column) = a counter-based function of (dropout_seed, token * d + column)
 *   — the generator of rat_dropout — so the backward call re-derives it from the same (p, seed) instead of reading a stored mask
 *   (torch's Philox stream cannot be matched bit for bit; parity for p > 0 is statistical).  Ignored without a projection. */
size_t rat_attn_fwd_workspace(int d, int heads, int dim_head);
int rat_attn_fwd_ex(const float* x, const float* res, float* y, float* o_save, float* lse_save, const RatAttnParams* w_host,
                    const RatSeqMap* map_host, int d, int heads, int dim_head, float softmax_scale, float out_scale,
                    float ln_eps, float dropout_p, uint64_t dropout_seed, int arith, float* workspace, size_t workspace_bytes,
                    void* stream);
int rat_attn_bwd_ex(const float* x, const float* dy, const float* add, const float* o_save, const float* lse_save, float* dx,
                    const RatAttnParams* w_host, const RatAttnParams* grads_host, float* workspace, size_t workspace_bytes,
                    const RatSeqMap* map_host, int d, int heads, int dim_head, float softmax_scale, float out_scale,
                    float ln_eps, float dropout_p, uint64_t dropout_seed, int arith, void* stream);

/* ---- wide heads in one forward launch (ABI v9).  heads = G x 8 (16 ... 64), dim_head 10, embedding_dim 64 — BASELINE configs[4], the
 * shipped Tmall config's 32 heads (configs/RAT_m2/tmall_x1_002/model_config.yaml:23) at d = 64.  heads * dim_head is too wide for the
 * fused kernels' LDS tile, but the head groups are independent given LayerNorm(x) (RAT_m2.py:192-202: the heads only meet in to_out),
 * so a caller may run the layer as G launches of rat_attn_fwd_ex on 8 heads each (res = x, then res = y) — or as ONE launch that loads
 * and normalises each 64-row chunk once and loops over the groups inside it, adding bias, Dropout and the residual once:
 *   y = out_scale * Dropout(to_out(concat_g softmax(Q_g K_g^T * scale) V_g)) + res        (bf16x3 arithmetic only)
 * planes: rat_attn_groups_planes_bytes() bytes, 16-byte aligned, filled by rat_split_weights_batch from the 4 G jobs of
 *   rat_attn_groups_split_jobs (they read group g's rows of the Q / K / V blocks of to_qkv.weight and its columns of to_out.weight in
 *   place: no permuted copy of the weights) — valid until the weights change; w_host = the layer's full-width parameters.
 * o_save [G][ntok][80], lse_save [G][ntok][8] (or both NULL): group-major, so that slice g is exactly what rat_attn_bwd_ex takes for
 *   a launch on group g; ntok = tokens of x (the slice stride).
 * rat_attn_groups_planes_bytes returns 0 (and rat_attn_groups_split_jobs 0 jobs) for dimensions this form does not serve.
 *
 * The same for the shipped Tmall geometry itself (embedding_dim <= 16, dim_head 10, 16 ... 64 heads; exact fp32, any `arith`): the weights are
 * addressed in place, `planes` is ignored (NULL), and up to 32 heads the BACKWARD is one launch too (rat_attn_bwd_groups): with one
 * 16-wide column tile the weight-gradient accumulators of four head groups fit the registers that one group needs at embedding_dim 64.
 * Gradients arrive in the layer's full-width layout (grads_host = [3*heads*dim_head][d], [d][heads*dim_head], [d], [d], [d]); dx = add +
 * LayerNorm-backward(...) as rat_attn_bwd_ex; workspace: rat_attn_bwd_groups_workspace() bytes (0: not served).
 * Round 6 (same signatures): at embedding_dim <= 16 the groups may also be 4 heads x dim_head 20 (heads = G x 4; RAT_m3 runs num_heads / 2
 * heads of width 2 * dim_head, RAT_m3.py:181): a group's inner width is 80 either way; lse_save is then [G][ntok][4].
 * rat_attn_groups_supported: bit 0 = rat_attn_fwd_groups serves these dimensions, bit 1 = rat_attn_bwd_groups does. */
int rat_attn_groups_supported(int d, int heads, int dim_head);
size_t rat_attn_bwd_groups_workspace(int d, int heads, int dim_head);
int rat_attn_bwd_groups(const float* x, const float* dy, const float* add, const float* o_save, const float* lse_save, int64_t ntok,
                        float* dx, const RatAttnParams* w_host, const RatAttnParams* grads_host, float* workspace, size_t workspace_bytes,
                        const RatSeqMap* map_host, int d, int heads, int dim_head, float softmax_scale, float out_scale, float ln_eps,
                        float dropout_p, uint64_t dropout_seed, void* stream);
size_t rat_attn_groups_planes_bytes(int d, int heads, int dim_head);
int rat_attn_groups_split_jobs(const RatAttnParams* w_host, int d, int heads, int dim_head, void* planes,
                               RatSplitJob* jobs_out /* [4 * heads / 8] */);   /* slice g of `planes` (rat_attn_groups_planes_bytes() / G each) is also a
                               * valid RatAttnParams.planes for rat_attn_bwd_ex on group g */
int rat_attn_fwd_groups(const float* x, const float* res, float* y, float* o_save, float* lse_save, int64_t ntok,
                        const RatAttnParams* w_host, const void* planes, const RatSeqMap* map_host, int d, int heads, int dim_head,
                        float softmax_scale, float out_scale, float ln_eps, float dropout_p, uint64_t dropout_seed, void* stream);

/* ---- K2d: the attention core alone, for sequences longer than the fused kernel's 64-row tile — RAT_m0 attends jointly over all
 * T*S tokens of a sample (RAT_m0.py:123-127; 231 at the north-star shape).  That variant runs LayerNorm as K2c and the two
 * projections as rat_sgemm; this is softmax(Q K^T * scale) V on the projected rows: qkv [ntok][3*heads*dim_head] (the output of
 * nn.Linear(d, 3I): Q | K | V, head-major), o [ntok][heads*dim_head], lse [ntok][heads] (log2-domain, as rat_attn_fwd saves it);
 * sequence q owns tokens [q*L, (q+1)*L).  softmax_scale <= 0 selects dim_head^-0.5.  dim_head <= 32; one head's K, V (backward:
 * also Q, dO) rows of a sequence must fit LDS (L * dim_head * 16 B <= 160 KB). */
int rat_attn_core_fwd(const float* qkv, float* o, float* lse, int64_t nseq, int L, int heads, int dim_head, float softmax_scale,
                      void* stream);
int rat_attn_core_bwd(const float* qkv, const float* o, const float* lse, const float* dout, float* dqkv, int64_t nseq, int L,
                      int heads, int dim_head, float softmax_scale, void* stream);
/* The same with RatSeqMap addressing (sequences strided through the token grid, e.g. the cross-sample phase) — the composed
 * attention path for dimensions the fused kernels do not serve.  rat_attn_fused_supported tells which path applies: 0 for
 * sequences above 64 tokens or heads*dim_head too wide for the fused LDS tile / weight-gradient accumulators (the shipped
 * Tmall config, configs/RAT_m2/tmall_x1_002/model_config.yaml:23: 32 heads x 10). */
int rat_attn_core_fwd_map(const float* qkv, float* o, float* lse, const RatSeqMap* map_host, int heads, int dim_head,
                          float softmax_scale, void* stream);
int rat_attn_core_bwd_map(const float* qkv, const float* o, const float* lse, const float* dout, float* dqkv,
                          const RatSeqMap* map_host, int heads, int dim_head, float softmax_scale, void* stream);
int rat_attn_fused_supported(int d, int heads, int dim_head, int L);

/* ---- K2 (cont.): FeedForward + residual, y = W2 gelu_erf(W1 x + b1) + b2 + x (RAT_m2.py:163-174, 232) */
int rat_ffn_fwd(const float* x, float* y, const float* w1, const float* b1, const float* w2, const float* b2,
                int64_t ntok, int d, int hidden, void* stream);
size_t rat_ffn_bwd_workspace(int d, int hidden);
int rat_ffn_bwd(const float* x, const float* dy, float* dx, const float* w1, const float* b1, const float* w2,
                const float* b2, float* dw1, float* db1, float* dw2, float* db2, float* workspace,
                size_t workspace_bytes, int64_t ntok, int d, int hidden, void* stream);

/* The same block MLP with the residual taken from a SEPARATE tensor: y = W2 gelu_erf(W1 x + b1) + b2 + res (res == x gives
 * rat_ffn_fwd; res == NULL: no residual).  RAT_m1's PreNorm(FeedForward) (RAT_m1.py:143-161,201,207: ff(norm(x)) + x) is
 * rat_layernorm_fwd followed by this with x = norm(x), res = x.  Backward: add_dy = 1 adds dy to dx (residual from x
 * itself), add_dy = 0 returns only the gradient through the two Linear layers.
 * arith: RAT_ARITH_F32 (what rat_ffn_fwd / rat_ffn_bwd use) or RAT_ARITH_BF16X3 (see rat_attn_fwd_ex; compiled for d = 64,
 * hidden = 128, every other shape runs exact fp32). */
int rat_ffn_fwd_res(const float* x, const float* res, float* y, const float* w1, const float* b1, const float* w2,
                    const float* b2, int64_t ntok, int d, int hidden, int arith, void* stream);
int rat_ffn_bwd_res(const float* x, const float* dy, float* dx, const float* w1, const float* b1, const float* w2,
                    const float* b2, float* dw1, float* db1, float* dw2, float* db2, float* workspace,
                    size_t workspace_bytes, const void* planes /* of rat_ffn_split_jobs, or NULL */, int64_t ntok, int d,
                    int hidden, int add_dy, int arith, void* stream);

/* ABI v7: rat_ffn_bwd_res for an incoming gradient that is zero except on the token rows t = k * dy_period (k = 0, 1, ...): dy_rows
 * [ceil(ntok / dy_period)][d] holds those rows compactly, the zero rows are neither stored nor read.  The last encoder block's case:
 * the head reads one class token per sample (RAT_m2.py:138-140), so d loss / d x is zero on every other token of the [B][T][S] grid and
 * the [ntok][d] zero fill in front of the backward disappears.  Only where rat_ffn_bwd_rows_supported says 1 (the bf16x3
 * weight-stationary kernel: d = 64 or 40 / 48 / 56 with hidden = 2 d, RAT_ARITH_BF16X3); ntok, dy_period < 2^31. */
int rat_ffn_bwd_rows_supported(int d, int hidden, int arith);
int rat_ffn_bwd_res_rows(const float* x, const float* dy_rows, int64_t dy_period, float* dx, const float* w1, const float* b1,
                         const float* w2, const float* b2, float* dw1, float* db1, float* dw2, float* db2, float* workspace,
                         size_t workspace_bytes, const void* planes, int64_t ntok, int d, int hidden, int add_dy, int arith,
                         void* stream);

/* ABI v7 — one reduction launch for a whole backward pass.  rat_attn_bwd* / rat_ffn_bwd* / rat_layernorm_bwd each end with a launch
 * that sums their per-work-group gradient slabs (in `workspace`) into the weight gradients.  Between rat_reduce_defer_begin() and
 * rat_reduce_defer_end(stream, 1) of the SAME host thread those launches are recorded instead and run together at the end (one launch
 * per 80 outputs; same sums in the same order).  Contract: every call in between gets a `workspace` of its own that stays untouched
 * until the end call, and nothing reads the weight gradients before it.  run = 0 drops the record (error unwinding). */
int rat_reduce_defer_begin(void);
int rat_reduce_defer_end(void* stream, int run);

/* ---- K2c: stand-alone nn.LayerNorm(d) (biased variance, affine) over selected token rows — RAT_m1's PreNorm in front of
 * FeedForward and the final `self.norm` of each Transformer (RAT_m1.py:137-141,198,209), of which only token 0 of every
 * sequence is read (RAT_m1.py:125,128).  Row r is read at x + r * x_stride; y is a compact [nrows][d]. */
int rat_layernorm_fwd(const float* x, int64_t x_stride, float* y, const float* gamma, const float* beta, int64_t nrows,
                      int d, float eps, void* stream);
size_t rat_layernorm_bwd_workspace(int64_t nrows, int d);
/* dx row r (at dx + r * dx_stride; rows not addressed are left untouched) = [add row r +] LayerNorm backward of the compact
 * dy [nrows][d]; dgamma / dbeta are OVERWRITTEN with the row sums (fixed-order reduction, no atomics).  `add` (optional)
 * is laid out like dx and may alias it. */
int rat_layernorm_bwd(const float* x, int64_t x_stride, const float* dy, const float* gamma, const float* add, float* dx,
                      int64_t dx_stride, float* dgamma, float* dbeta, float* workspace, size_t workspace_bytes,
                      int64_t nrows, int d, float eps, void* stream);

/* ---- K6: BM25-style top-K retrieval pre-compute — the scoring / top-k / merge core of BM25_topk_retrieval_v4
 * (fuxictr/datasets/data_utils.py:774-1064); without exact-match columns (the shipped dataset configs):
 *   score[b][n] = sum_f (qry_ids[b][f] == db[n][f]) * qry_idf[b][f]   (float64, f ascending)
 *   out_values[b][0:K] = the K largest scores, descending; zero scores are dropped: out_indices = -1, out_values = 0;
 *   out_lens[b] = number of entries kept (data_utils.py:786-818 padded_topk + sort_results).
 * db_ids_field_major is [n_fields][n_db] int32 (the pool's id columns, transposed); qry_ids [n_qry][n_fields] int32; qry_idf
 * [n_qry][n_fields] float64 = log(n_db / count of that id in the pool column), 0 for ids absent from the pool
 * (data_utils.py:873-880,843-847).  Equal scores keep the lower pool index (torch.topk leaves that order unspecified).
 * n_fields <= 32, topk <= 32. */
int rat_bm25_topk(const int32_t* db_ids_field_major, const int32_t* qry_ids, const double* qry_idf, double* out_values,
                  int64_t* out_indices, int64_t* out_lens, int64_t n_db, int64_t n_qry, int n_fields, int topk, void* stream);

/* The same with exact-match columns (`exact_match_col_indices`, data_utils.py:851-866, 932-938): db_groups [n_db] / qry_groups
 * [n_qry] int32 number the distinct values of the exact-match columns (every query group >= 0 — queries whose key the pool
 * does not hold are filtered by the caller, as at data_utils.py:923-924); the id columns passed are the REMAINING ones.
 *   score[b][n] = db_groups[n] == qry_groups[b] ? (BM25 score as above) + 1 : 0 */
int rat_bm25_topk_grouped(const int32_t* db_ids_field_major, const int32_t* db_groups, const int32_t* qry_ids,
                          const double* qry_idf, const int32_t* qry_groups, double* out_values, int64_t* out_indices,
                          int64_t* out_lens, int64_t n_db, int64_t n_qry, int n_fields, int topk, void* stream);

/* ---- K6b: the request path (online scoring; additive in ABI v9) ----------------------------------------------------
 * map_data_to_IDF_v1 (data_utils.py:843-847) for ONE query batch on the device.  ids [n_qry][row_stride] int32 are full encoded rows,
 * cols [n_fields] int32 the columns the retrieval compares; the pool's per-column IDF tables are three flat arrays: table_ids (sorted
 * distinct ids of column 0, then column 1, ...), table_idf (their weights, float64 = log(n_db / count)) and table_offsets
 * [n_fields + 1] int64.  Outputs are exactly rat_bm25_topk's query inputs: qry_ids [n_qry][n_fields] = the gathered columns,
 * qry_idf [n_qry][n_fields] = the id's weight, 0 for ids the pool column does not hold — and, bug-compatible with the reference's
 * np.vectorize (its output dtype comes from the first element): if row 0 OF THIS CALL misses in a column, every weight of that column
 * is truncated toward zero.  n_fields <= 32. */
int rat_bm25_query_prepare(const int32_t* ids, const int32_t* cols, const int32_t* table_ids, const double* table_idf,
                           const int64_t* table_offsets, int32_t* qry_ids, double* qry_idf, int64_t n_qry, int row_stride,
                           int n_fields, void* stream);

/* The same for a batch that holds SEVERAL requests, each of them one query batch of the reference: first_row [n_qry] int64 (device)
 * gives, for batch row q, the batch row that opens q's request, and the dtype rule above looks at THAT row instead of row 0 — so every
 * request gets the weights it would get alone, whoever shares the launch.  first_row[q] is clamped to [0, n_qry) on the device: a
 * corrupt array gives a wrong weight, never an address outside `ids`.  With first_row all zero this is rat_bm25_query_prepare.
 * One launch on `stream`, no allocation, no synchronisation, no atomics: capturable.  (Additive in ABI v9.) */
int rat_bm25_query_prepare_seg(const int32_t* ids, const int64_t* first_row, const int32_t* cols, const int32_t* table_ids,
                               const double* table_idf, const int64_t* table_offsets, int32_t* qry_ids, double* qry_idf, int64_t n_qry,
                               int row_stride, int n_fields, void* stream);

/* rat_bm25_topk's contract (same inputs, same outputs, same tie rule, same limits) for FEW queries: the pool is cut into `splits`
 * contiguous row ranges of ceil(n_db / splits) rows scanned by different work-groups (ranges past the end are empty), each leaves its
 * topk best in `workspace` ([n_qry][splits][topk] float64 scores, then as many int64 indices), and a second launch merges them by
 * (score descending, index ascending).  The scores are the same float64 sums in the same order and that order is total, so the
 * result equals rat_bm25_topk's BIT FOR BIT for every splits >= 1 (<= 4096).  splits = 0: the library chooses from (n_qry, n_db) —
 * when the query tiles alone fill the chip it runs rat_bm25_topk itself and touches no workspace.  workspace_bytes >=
 * rat_bm25_topk_split_workspace(n_qry, topk, splits) (for splits = 0: the most the library may choose for that many queries),
 * 8-byte aligned.  Two launches on `stream`, no allocation, no synchronisation, no floating-point atomics: capturable. */
size_t rat_bm25_topk_split_workspace(int64_t n_qry, int topk, int splits);
int rat_bm25_topk_split(const int32_t* db_ids_field_major, const int32_t* qry_ids, const double* qry_idf, double* out_values,
                        int64_t* out_indices, int64_t* out_lens, void* workspace, size_t workspace_bytes, int64_t n_db,
                        int64_t n_qry, int n_fields, int topk, int splits, void* stream);

/* ---- K6c: a pool that grows in place (online scoring with reserved capacity; additive in ABI v9) -------------------
 * The pool's buffers are allocated for `capacity` rows once — db_ids_field_major [n_fields][capacity], pool_ids [capacity][row_len],
 * pool_labels [capacity] — and the number of rows that count lives in DEVICE memory (n_db_dev, one int64), so that launches captured
 * into a hipGraph before an append serve the grown pool after it: no kernel argument depends on the row count.
 *
 * rat_pool_append: n = *n_db_dev; rows i < n_rows of ids [n_rows][row_len] int32 / labels [n_rows] fp32 (device) are written to
 * pool_ids[n + i][:], pool_labels[n + i] and, transposed, db_ids_field_major[f][n + i] = ids[i][cols[f]] (64 consecutive rows of a
 * column per wave); a one-thread tail launch then sets *n_db_dev = n + n_rows.  Both read n on the device: appends queue back to back
 * without a synchronisation.  n + n_rows > capacity writes nothing and leaves the count (the caller checks beforehand).  pool_ids and
 * pool_labels may both be NULL (an index without the row store; labels is then ignored).  This form never removes a row; the ring
 * form below does. */
int rat_pool_append(const int32_t* ids, const float* labels, const int32_t* cols, int32_t* db_ids_field_major, int32_t* pool_ids,
                    float* pool_labels, int64_t* n_db_dev, int64_t n_rows, int64_t capacity, int row_len, int n_fields, void* stream);
/* rat_bm25_topk_split over the first *n_db_dev rows of a [n_fields][capacity] pool.  splits = 0: rat_bm25_topk_split's rule applied
 * to the CAPACITY (the launch shape never changes); where that rule hands over to rat_bm25_topk, the same scan runs with one range
 * here.  Range r covers rows [r c, min((r + 1) c, n)) with c = ceil(n / splits) of the CURRENT n; rows >= n are never read.  The scan
 * and merge code is rat_bm25_topk_split's, so the result equals rat_bm25_topk over the first n rows bit for bit.  Workspace as there
 * (always needed). */
int rat_bm25_topk_split_dev(const int32_t* db_ids_field_major, const int64_t* n_db_dev, const int32_t* qry_ids, const double* qry_idf,
                            double* out_values, int64_t* out_indices, int64_t* out_lens, void* workspace, size_t workspace_bytes,
                            int64_t capacity, int64_t n_qry, int n_fields, int topk, int splits, void* stream);
/* rat_batch_assemble with the pool's row count N read from *n_pool_dev: a negative neighbour index (the -1 padding of a short list)
 * counts back from the pool's last LIVE row, which moves with every append. */
int rat_batch_assemble_dev(const int32_t* data_ids, const float* data_labels, const int32_t* pool_ids, const float* pool_labels,
                           const int64_t* retr_indices, const int64_t* rows, int32_t* idx, int32_t* label_ids, float* y_true,
                           int64_t Q, const int64_t* n_pool_dev, int B, int K, int L, void* stream);

/* A pool that slides (additive in ABI v9 as well): the same three buffers used as a RING.  The header header_dev is two int64 in device
 * memory, {n, head}: n live rows, head = the physical slot of the oldest.  LOGICAL row i (0 = oldest, n - 1 = newest) lives in slot
 * head + i, minus capacity when that is >= capacity.  Everything a caller sees is logical: the indices the scan returns, the tie rule
 * (score descending, logical index ascending — the older row wins) and the neighbour indices the assembly takes.
 *
 * rat_pool_push: rat_pool_append's work with E = max(0, n + n_rows - capacity): row i of the batch goes to slot head + n + i (wrapped)
 * of all three stores, then a one-thread tail launch sets head = head + E (wrapped), n = n + n_rows - E — the E oldest rows leave.
 * Both launches read the header on the device (pushes queue back to back).  n_rows > capacity writes nothing and leaves the header.
 * rat_pool_evict: a one-thread launch, head = head + n_rows (wrapped), n = n - n_rows; nothing happens for n_rows < 0 or n_rows >= n
 * (the pool never becomes empty).
 * rat_bm25_topk_split_ring: rat_bm25_topk_split_dev over the n live rows in logical order (n clamped to [0, capacity], head to
 * [0, capacity)); ranges are cut over the logical rows, only the address of the id load is physical.  The result equals rat_bm25_topk
 * over a contiguous copy of the live rows, oldest first, bit for bit, for every head.
 * rat_batch_assemble_ring: rat_batch_assemble_dev with logical neighbour indices — a negative one counts back from n first, then the
 * index is mapped to its slot. */
int rat_pool_push(const int32_t* ids, const float* labels, const int32_t* cols, int32_t* db_ids_field_major, int32_t* pool_ids,
                  float* pool_labels, int64_t* header_dev, int64_t n_rows, int64_t capacity, int row_len, int n_fields, void* stream);
int rat_pool_evict(int64_t* header_dev, int64_t n_rows, int64_t capacity, void* stream);
int rat_bm25_topk_split_ring(const int32_t* db_ids_field_major, const int64_t* header_dev, const int32_t* qry_ids, const double* qry_idf,
                             double* out_values, int64_t* out_indices, int64_t* out_lens, void* workspace, size_t workspace_bytes,
                             int64_t capacity, int64_t n_qry, int n_fields, int topk, int splits, void* stream);
int rat_batch_assemble_ring(const int32_t* data_ids, const float* data_labels, const int32_t* pool_ids, const float* pool_labels,
                            const int64_t* retr_indices, const int64_t* rows, int32_t* idx, int32_t* label_ids, float* y_true,
                            int64_t Q, const int64_t* header_dev, int64_t capacity, int B, int K, int L, void* stream);

/* A pool that loses rows (additive in ABI v9 as well): arbitrary rows leave the ring above, the survivors close up IN PLACE and in age
 * order, so that the scan, the merge and the assembly serve the result unchanged.
 *
 * rat_pool_delete: del_dev [n_del] int64 (device) are LOGICAL indices, strictly ascending (the caller sorts and validates them).  Live
 * row j that is not listed ends at logical position j - #{listed rows < j} in all three stores (slot head + position, wrapped); rows
 * older than del_dev[0] are not touched, head does not move, and a one-thread tail launch sets n = n - n_del.  The move is staged through
 * `scratch`, one store after the other in stream order: a launch gathers the survivors of the suffix [del_dev[0], n) in compact order
 * (64 consecutive rows of a column per wave for db_ids_field_major, words for pool_ids, as rat_pool_push addresses them), the next one
 * copies them back — no work-group waits for another.  scratch_bytes >= 4 capacity max(n_fields, row_len) (4 capacity n_fields when
 * pool_ids and pool_labels are NULL — they go together, as for rat_pool_push), 4-byte aligned; it is not read between calls.  All
 * launches read the header on the device: a delete queues behind pushes and evictions without a synchronisation, and the grid depends
 * on the capacity only.  n_del <= 0 launches nothing.  n_del >= n (the pool would become empty) moves nothing and leaves the header.
 * For ANY header or list content nothing outside the buffers is addressed (n is clamped to [0, capacity], head to [0, capacity),
 * del_dev[0] to [0, n]; a source row is always a live one); what the stores then hold is unspecified. */
int rat_pool_delete(int32_t* db_ids_field_major, int32_t* pool_ids, float* pool_labels, int64_t* header_dev, const int64_t* del_dev,
                    void* scratch, size_t scratch_bytes, int64_t n_del, int64_t capacity, int row_len, int n_fields, void* stream);

/* A pool addressed by key (additive in ABI v9 as well): find the live rows that hold given ids, and relabel rows, on the device.
 * Both take the pool in one of the three forms of the scan — pool_form RAT_POOL_HOST: n_rows live rows, given by value (header_dev is
 * not read); RAT_POOL_DEV: n = header_dev[0]; RAT_POOL_RING: {n, head} = header_dev[0 .. 1], logical row i in slot head + i (wrapped).
 * n is clamped to [0, capacity] and head to [0, capacity), as the ring scan clamps them; `capacity` is the number of rows (slots) the
 * store holds (for an immutable pool: its N).
 *
 * rat_pool_find: word (slot, c) of the store is store[slot * row_stride + cols[c] * col_stride] — db_ids_field_major: row_stride 1,
 * col_stride capacity (or N), store_cols n_fields; pool_ids: row_stride row_len, col_stride 1, store_cols row_len.  cols [n_cols] int32
 * (device) are positions inside the store (clamped to [0, store_cols)), keys [n_keys][n_cols] int32 (device) are sorted
 * lexicographically (signed) and distinct — the caller sorts.  Logical row i MATCHES if some key equals it on all n_cols columns.
 * out_count[0] = the number of matching live rows (also when it exceeds max_out); out_idx[0 .. min(total, max_out)) = the first matches
 * in ascending logical order; out_idx[min(total, max_out) .. max_out) = -1, so the list can be handed to rat_pool_set_labels whole.
 * Three launches on the stream — count per range, offsets, ranked store — with no work-group waiting for another.  groups = 0: the
 * number of ranges is chosen from the capacity alone (at most RAT_POOL_FIND_AUTO_GROUPS), so the grid does not depend on the live
 * count and a find queues behind pushes, evictions and deletions; 1 .. 4096 forces that many (a range past the end is empty).
 * workspace: 8 (2 groups + 1) bytes, 8-byte aligned (groups = 0: 8 (2 RAT_POOL_FIND_AUTO_GROUPS + 1) always suffices).  For ANY header
 * and key content nothing outside the store, keys, out_idx[0 .. max_out), out_count and the workspace is addressed.
 *
 * rat_pool_set_labels: pool_labels[slot of logical indices[j]] = labels[j * label_stride] for j < m, one launch; label_stride 1 (a
 * label per index) or 0 (labels[0] for all).  An index < 0 or >= n is skipped on the device.  Distinct indices are the caller's
 * business (two entries for one row: either label stays).  m <= 0 launches nothing. */
#define RAT_POOL_HOST 0
#define RAT_POOL_DEV 1
#define RAT_POOL_RING 2
#define RAT_POOL_FIND_AUTO_GROUPS 1024
int rat_pool_find(const int32_t* store, int64_t row_stride, int64_t col_stride, int store_cols, int pool_form, const int64_t* header_dev,
                  int64_t n_rows, int64_t capacity, const int32_t* cols, int n_cols, const int32_t* keys, int64_t n_keys, int64_t* out_idx,
                  int64_t max_out, int64_t* out_count, void* workspace, size_t workspace_bytes, int groups, void* stream);
int rat_pool_set_labels(float* pool_labels, int pool_form, const int64_t* header_dev, int64_t n_rows, int64_t capacity,
                        const int64_t* indices, const float* labels, int64_t m, int label_stride, void* stream);

/* A pool that looks at itself (additive in ABI v9 as well): score live rows against only the rows OLDER than them — what the
 * reference's <X>-fold retrieval does for a self-pool (fuxictr/pytorch/data_generator.py:115-176).  The pool keeps its rows in age
 * order (logical 0 = the oldest), so the horizon of a row is one number: its own logical index.  Both take the pool in the three
 * forms above (pool_form, header_dev, n_rows, capacity; n clamped to [0, capacity], head to [0, capacity)).
 *
 * rat_pool_gather_rows: out_ids[j][0 .. row_len) and out_labels[j] = ids and label of the logical row indices[j] (int64, device) out
 * of pool_ids [capacity][row_len] / pool_labels [capacity], one launch; an index < 0 or >= n gives a row of zeros and label 0.
 * out_before[j] = indices[j] clamped to [0, n]: the row's horizon, which rat_bm25_topk_split_before consumes — nothing is read back
 * in between.  n_indices <= 0 launches nothing.
 *
 * rat_bm25_topk_split_before: rat_bm25_topk_split's two launches with a horizon per query — query q's candidates are the logical
 * rows i < before_dev[q] (int64 [n_qry], device; clamped to [0, n] on the device: a negative value or 0 gives lens 0, values 0 and
 * indices -1, a value past the end the whole pool; no value gives an address outside the buffers).  db_ids_field_major is
 * [n_fields][capacity] (RAT_POOL_HOST: the first n_rows columns are the pool).  For every q the values, indices and lens equal
 * rat_bm25_topk over a contiguous copy of the logical rows [0, min(before[q], n)) with the same qry_idf, bit for bit: the scan scores
 * every row as rat_bm25_topk_split does and a row at or past the horizon then scores 0; the lists, the merge and the total order
 * (score descending, logical index ascending) are unchanged.  The IDF weights are the caller's: rat_bm25_query_prepare maps them from
 * the tables of the WHOLE live pool.  Ranges are cut over [0, n); splits = 0 is chosen from the capacity in every form, so a captured
 * launch never changes shape; workspace as rat_bm25_topk_split_workspace(n_qry, topk, splits). */
int rat_pool_gather_rows(const int32_t* pool_ids, const float* pool_labels, int pool_form, const int64_t* header_dev, int64_t n_rows,
                         int64_t capacity, const int64_t* indices, int32_t* out_ids, float* out_labels, int64_t* out_before,
                         int64_t n_indices, int row_len, void* stream);
int rat_bm25_topk_split_before(const int32_t* db_ids_field_major, int pool_form, const int64_t* header_dev, int64_t n_rows,
                               int64_t capacity, const int32_t* qry_ids, const double* qry_idf, const int64_t* before_dev,
                               double* out_values, int64_t* out_indices, int64_t* out_lens, void* workspace, size_t workspace_bytes,
                               int64_t n_qry, int n_fields, int topk, int splits, void* stream);

/* Neighbours restricted to rows equal on given columns (additive in ABI v9 as well): the reference's exact_match_col_indices
 * (fuxictr/datasets/data_utils.py:851-866, 895-938) on the request path, with no group numbers — db_ids_field_major holds every used
 * column, so the scan compares the query's ids on the exact columns with the row's.  exact_mask: bit f set = used column f (f <
 * n_fields) is an exact-match column; at least one bit, none at or past n_fields, and at least one used column left to score, or the
 * call fails.  A CANDIDATE of query q is a live row (below q's horizon) equal to q on every exact column.  All three take the pool in
 * the three forms above (pool_form, header_dev, n_rows, capacity; n clamped to [0, capacity], head to [0, capacity)) and an optional
 * before_dev [n_qry] int64 (device; NULL: no horizon), clamped to [0, n] as rat_bm25_topk_split_before clamps it.  They are chained
 *     rat_bm25_exact_count -> rat_bm25_exact_plan -> rat_bm25_query_prepare_seg (first_row) -> rat_bm25_topk_split_exact
 * on one stream with nothing read back, no allocation, no synchronisation and no floating-point atomics: capturable.  For one query
 * batch the result equals rat_amd/retrieval.py's BM25_topk_retrieval_v4(live[:, used], ids[:, used], exact_match_col_indices, qry_batch_
 * size = None) bit for bit, its two batch-wide rules included.
 *
 * rat_bm25_exact_count: out_counts[q] (int64 [n_qry]) = the number of candidates of query q.  ids [n_qry][row_stride] int32 are the
 * request's encoded rows and cols [n_fields] int32 the used columns inside them, as rat_bm25_query_prepare takes them (a column is
 * clamped to [0, row_stride)).  Work-group (tile of eight queries, range) counts range r = rows [r c, min((r + 1) c, n)), c = ceil(n /
 * groups), into workspace[q][r]; a second launch sums a query's partials in range order — integer sums, one result whatever the grid.
 * groups = 0: chosen from (n_qry, capacity) alone, at most RAT_BM25_EXACT_AUTO_GROUPS, so a captured launch never changes shape;
 * 1 .. 4096 forces that many (a range past the end is empty).  workspace: 8 n_qry groups bytes, 8-byte aligned (groups = 0:
 * 8 n_qry RAT_BM25_EXACT_AUTO_GROUPS always suffices).
 *
 * rat_bm25_exact_plan: one small launch over counts [n_qry].  first_row[q] (int64 [n_qry]) = the first query with a candidate, for
 * every q, or 0 when no query has one — the shape rat_bm25_query_prepare_seg consumes, so the dtype rule of the IDF mapping looks at
 * the first candidate-bearing query, as the offline path does after it has dropped the others.  listing_dev[0] (one int32) = 1 when
 * no count exceeds topk (the LISTING rule holds for the call), else 0.  The counts are only compared: whatever they hold, first_row
 * stays inside [0, n_qry) and the flag is 0 or 1.
 *
 * rat_bm25_topk_split_exact: rat_bm25_topk_split_before's two launches with the exact columns as a gate — in the field loop an exact
 * column adds no weight, and after it a candidate scores (sum over the other columns, f ascending) + 1 and any other row 0, as
 * rat_bm25_topk_grouped forms it; the horizon select, the lists, the merge and the total order (score descending, logical index
 * ascending) are unchanged.  lens[q] = min(candidates, topk).  A third launch reads listing_dev[0] (int32, device): when it is not 0
 * each query's entries are reordered by ascending logical index and their values set to 1.0 — every candidate is in the merged list
 * then, nothing is rescanned; when it is 0 nothing changes.  qry_idf of an exact column is not read.  splits and workspace as
 * rat_bm25_topk_split_before.  For ANY header, horizon, flag or weight content nothing outside the buffers is addressed. */
#define RAT_BM25_EXACT_AUTO_GROUPS 256
int rat_bm25_exact_count(const int32_t* db_ids_field_major, int pool_form, const int64_t* header_dev, int64_t n_rows, int64_t capacity,
                         const int32_t* ids, const int32_t* cols, uint32_t exact_mask, const int64_t* before_dev, int64_t* out_counts,
                         void* workspace, size_t workspace_bytes, int64_t n_qry, int row_stride, int n_fields, int groups, void* stream);
int rat_bm25_exact_plan(const int64_t* counts, int64_t* first_row, int32_t* listing_dev, int64_t n_qry, int topk, void* stream);
int rat_bm25_topk_split_exact(const int32_t* db_ids_field_major, int pool_form, const int64_t* header_dev, int64_t n_rows,
                              int64_t capacity, const int32_t* qry_ids, const double* qry_idf, uint32_t exact_mask,
                              const int64_t* before_dev, const int32_t* listing_dev, double* out_values, int64_t* out_indices,
                              int64_t* out_lens, void* workspace, size_t workspace_bytes, int64_t n_qry, int n_fields, int topk,
                              int splits, void* stream);

/* ---- K3: prediction head -----------------------------------------------------------------------------
 * Plain fp32 GEMM on MFMA for MLP_Layer's nn.Linear (deep.py:126-141) forward / dgrad / wgrad:
 * C[M][N] = op(A) op(B) (+ bias[N]) (+ beta*C), row-major with leading dimensions, op = transpose flag. */
int rat_sgemm(int trans_a, int trans_b, int M, int N, int K, const float* A, int lda, const float* B, int ldb,
              float* C, int ldc, const float* bias, float beta, void* stream);
/* Same product with a caller-owned workspace of rat_sgemm_workspace(M, N, K) bytes (0 = none needed): when the output
 * has few tiles and K is long (the weight gradients: K = batch), the k range is split across work-groups and the raw
 * partial tiles are summed in slice order by a second launch — deterministic, no atomics. */
size_t rat_sgemm_workspace(int M, int N, int K);
int rat_sgemm_ws(int trans_a, int trans_b, int M, int N, int K, const float* A, int lda, const float* B, int ldb,
                 float* C, int ldc, const float* bias, float beta, float* workspace, size_t workspace_bytes, void* stream);
/* ABI v4: the same with the arithmetic selectable — RAT_ARITH_BF16X3 runs the product on v_mfma_f32_16x16x32_bf16 with 3-way split
 * operands (fp32-class accuracy, see rat_attn_fwd_ex) when both operands allow 16-byte fetches and K >= 64; otherwise exact fp32. */
int rat_sgemm_arith(int trans_a, int trans_b, int M, int N, int K, const float* A, int lda, const float* B, int ldb,
                    float* C, int ldc, const float* bias, float beta, float* workspace, size_t workspace_bytes,
                    int arith, void* stream);
/* BatchNorm1d (train: batch stats, biased var; running stats momentum update with unbiased var; eval:
 * running stats) followed by the hidden layer's activation — deep.py:128-132.  use_bn=0 -> activation only.  z,a [M][N].
 * workspace: rat_bn_workspace(N) bytes (per-row-split partial sums; needed when use_bn && training, and by bwd).
 * act (ABI v6; every rat_bn_* entry point below takes it): the activation MLP_Layer puts behind the layer (deep.py:121-123,
 * torch_utils.get_activation, torch_utils.py:83-94) — the names stay "bn_relu" because ReLU is what every shipped config uses. */
#define RAT_ACT_RELU 0
#define RAT_ACT_NONE 1        /* no activation module (hidden_activations entry None / "") or nn.Identity */
#define RAT_ACT_SIGMOID 2
#define RAT_ACT_TANH 3
#define RAT_ACT_LEAKY_RELU 4  /* nn.LeakyReLU(): negative_slope 0.01 */
#define RAT_ACT_ELU 5         /* nn.ELU(): alpha 1.0 */
size_t rat_bn_workspace(int N);
int rat_bn_relu_fwd(const float* z, float* a, const float* gamma, const float* beta, float* running_mean,
                    float* running_var, float* save_mean, float* save_rstd, float* workspace, int M, int N,
                    int training, int use_bn, float eps, float momentum, int act, void* stream);
/* a = the forward output (the derivative of every supported activation is a function of it); dgamma/dbeta overwritten */
int rat_bn_relu_bwd(const float* z, const float* a, const float* da, float* dz, const float* gamma,
                    const float* save_mean, const float* save_rstd, float* dgamma, float* dbeta, float* workspace,
                    int M, int N, int use_bn, int act, void* stream);
/* ABI v7 — column-strip forms of the two calls above: ONE launch per layer and direction, no workspace, sums in a fixed order
 * (deterministic).  A work-group owns 8 columns for all M rows: batch statistics and their use share the launch, and the backward
 * also returns dbias_lin[N] = column sums of dz — the bias gradient of the nn.Linear in front (deep.py:126-127), i.e. rat_colsum of
 * its own output (nullptr = not wanted).  Need rat_bn_strip_ok(M, N) (N % 4 == 0) and 16-byte aligned pointers; same arithmetic
 * per element as rat_bn_relu_fwd / rat_bn_relu_bwd, batch sums in another (fixed) order. */
int rat_bn_strip_ok(int M, int N);
int rat_bn_act_fwd_strip(const float* z, float* a, const float* gamma, const float* beta, float* running_mean,
                         float* running_var, float* save_mean, float* save_rstd, int M, int N, int training, int use_bn,
                         float eps, float momentum, int act, void* stream);
int rat_bn_act_bwd_strip(const float* z, const float* a, const float* da, float* dz, const float* gamma,
                         const float* save_mean, const float* save_rstd, float* dgamma, float* dbeta, float* dbias_lin,
                         int M, int N, int use_bn, int act, void* stream);
/* The LAST hidden layer in front of the DNN's one-output Linear (deep.py:135-137): its incoming gradient is the outer product
 * da[r][c] = dl[r] * w[c] (dl = dlogit [M], w = that Linear's weight [N]) — formed inside the kernel — and dw[c] = sum_r dl[r] a[r][c]
 * (the Linear's weight gradient) comes back with it: replaces two rat_sgemm launches and the da matrix. */
int rat_bn_act_bwd_strip_outer(const float* z, const float* a, const float* dl, const float* w, float* dw, float* dz,
                               const float* gamma, const float* save_mean, const float* save_rstd, float* dgamma, float* dbeta,
                               float* dbias_lin, int M, int N, int use_bn, int act, void* stream);
/* SyncBN for data parallelism (deep.py:128-132 evaluated over the GLOBAL batch, i.e. exactly what the
 * reference's single-device BatchNorm1d sees).  The collectives between the calls belong to the caller (RCCL):
 *   fwd:  rat_bn_local_stats -> all_gather(stats, 2N+1 floats per rank) -> rat_bn_relu_fwd_sync
 *   bwd:  rat_bn_bwd_local_sums -> all_reduce_sum(copy of sums, 2N floats) -> rat_bn_relu_bwd_sync
 * stats = [mean_r (N) | sum (z-mean_r)^2 (N) | row count (1)]; all_stats = [world] such records, combined in rank order
 * (Chan's update: stable, the same bits on every rank).  dgamma / dbeta receive this rank's LOCAL sums (the gradient
 * bucket's all-reduce adds the ranks); the backward reads the global row count from the forward's all_stats.
 * workspace: rat_bn_workspace(N) bytes. */
int rat_bn_local_stats(const float* z, float* stats, float* workspace, int M, int N, void* stream);
int rat_bn_relu_fwd_sync(const float* z, float* a, const float* gamma, const float* beta, float* running_mean,
                         float* running_var, float* save_mean, float* save_rstd, const float* all_stats, int world,
                         int M, int N, float eps, float momentum, int act, void* stream);
int rat_bn_bwd_local_sums(const float* z, const float* a, const float* da, const float* save_mean, const float* save_rstd,
                          float* sums, float* workspace, int M, int N, int act, void* stream);
int rat_bn_relu_bwd_sync(const float* z, const float* a, const float* da, float* dz, const float* gamma,
                         const float* save_mean, const float* save_rstd, const float* local_sums, const float* global_sums,
                         float* dgamma, float* dbeta, const float* all_stats, int world, int M, int N, int act, void* stream);
/* column sums of a [M][N] matrix (bias gradients); workspace: rat_colsum_workspace(M, N) bytes (= rat_bn_workspace(N) up to
 * M = 65536 rows; more row splits beyond, for the token-sized matrices of the composed attention path) */
size_t rat_colsum_workspace(int M, int N);
int rat_colsum(const float* a, int lda, float* out, float* workspace, int M, int N, void* stream);

/* logit = fc(cls) + dnn_out + sum_f lr_table_f[idx] ; y_pred = sigmoid(logit)  (RAT_m2.py:138-150,
 * shallow.py:36-45); loss_sum += sum_b BCE(y_pred, y_true)/B with torch's log clamp at -100
 * (torch_utils.py:51-63, base_model.py:74-77).  cls rows are read at cls + b*cls_stride (floats); idx rows of
 * the TARGET sample at idx + b*idx_stride.  dnn_out / lr_fields_dev / loss_sum / y_true may be NULL.
 * head (ABI v6): RAT_HEAD_BINARY — the above; RAT_HEAD_REGRESSION — task = "regression" (base_model.py:286-292: no output
 * activation) with loss = "mse_loss": y_pred = logit, loss_sum += sum_b (y_pred - y_true)^2 / B. */
#define RAT_HEAD_BINARY 0
#define RAT_HEAD_REGRESSION 1
int rat_logit_fwd(const float* cls, int64_t cls_stride, const float* fc_w, const float* fc_b,
                  const float* dnn_out, const RatField* lr_fields_dev, int nfields, const int32_t* idx,
                  int64_t idx_stride, const float* y_true, float* y_pred, float* loss_sum, int B, int d,
                  int head, void* stream);
/* ABI v7: the same with the DNN's one-output Linear evaluated inside: logit = fc(cls) + (dnn_in[b] . dnn_w + dnn_b) + LR — dnn_in
 * [B][dnn_k] with leading dimension dnn_ld is the last hidden layer's output (formerly an N = 1 rat_sgemm launch into dnn_out). */
int rat_logit_fwd_dnn(const float* cls, int64_t cls_stride, const float* fc_w, const float* fc_b, const float* dnn_in,
                      int64_t dnn_ld, const float* dnn_w, const float* dnn_b, int dnn_k, const RatField* lr_fields_dev,
                      int nfields, const int32_t* idx, int64_t idx_stride, const float* y_true, float* y_pred,
                      float* loss_sum, int B, int d, int head, void* stream);
/* rat_logit_fwd / rat_logit_fwd_dnn for field sets with MaskedAveragePooling fields: the LR layer's own EmbeddingLayer applies the
 * same encoder (shallow.py:30, embedding.py:101), so an averaged field's wide term is sum_i w[id_i] / (#{w[id_i] != 0} + 1e-16f)
 * (sequence.py:24-29).  modes_dev: device int32 [nfields] as rat_gather_fwd_pool.  lr_den (nullable): float [B][nfields] <- each
 * (sample, field)'s denominator (1 for a summed field), what rat_logit_bwd_pool / rat_sparse_reduce_scalar_pool divide by.
 * modes_dev = NULL and lr_den = NULL: rat_logit_fwd / rat_logit_fwd_dnn exactly. */
int rat_logit_fwd_pool(const float* cls, int64_t cls_stride, const float* fc_w, const float* fc_b, const float* dnn_out,
                       const RatField* lr_fields_dev, const int32_t* modes_dev, int nfields, const int32_t* idx,
                       int64_t idx_stride, const float* y_true, float* y_pred, float* loss_sum, float* lr_den, int B, int d,
                       int head, void* stream);
int rat_logit_fwd_dnn_pool(const float* cls, int64_t cls_stride, const float* fc_w, const float* fc_b, const float* dnn_in,
                           int64_t dnn_ld, const float* dnn_w, const float* dnn_b, int dnn_k, const RatField* lr_fields_dev,
                           const int32_t* modes_dev, int nfields, const int32_t* idx, int64_t idx_stride, const float* y_true,
                           float* y_pred, float* loss_sum, float* lr_den, int B, int d, int head, void* stream);
/* dlogit[b] = gscale * (gscale_dev ? *gscale_dev : 1) * (y_pred - y_true)/B (x 2 for RAT_HEAD_REGRESSION) ; dcls row b (written at
 * dcls + b*dcls_stride) = dlogit*fc_w ; dfc_w, dfc_b and the LR grad tables are ACCUMULATED into (caller zeroes them).
 * gscale_dev (nullable): a DEVICE scalar — autograd's incoming loss gradient — so that backward needs no host read-back. */
int rat_logit_bwd(const float* y_pred, const float* y_true, const float* cls, int64_t cls_stride,
                  const float* fc_w, float* dlogit, float* dcls, int64_t dcls_stride, float* dfc_w,
                  float* dfc_b, const RatField* lr_grad_fields_dev, int nfields, const int32_t* idx,
                  int64_t idx_stride, float gscale, const float* gscale_dev, int B, int d, int head, void* stream);
/* ABI v7: rat_logit_bwd that also ACCUMULATES sum_b dlogit[b] into ddnn_b (the bias gradient of the DNN's one-output Linear) */
int rat_logit_bwd_dnn(const float* y_pred, const float* y_true, const float* cls, int64_t cls_stride, const float* fc_w,
                      float* dlogit, float* dcls, int64_t dcls_stride, float* dfc_w, float* dfc_b, float* ddnn_b,
                      const RatField* lr_grad_fields_dev, int nfields, const int32_t* idx, int64_t idx_stride, float gscale,
                      const float* gscale_dev, int B, int d, int head, void* stream);
/* rat_logit_bwd / rat_logit_bwd_dnn with averaged LR fields: field f of sample b scatters dlogit[b] / lr_den[b][f] (lr_den from
 * rat_logit_fwd_pool; a summed field's 1 leaves dlogit unchanged).  lr_den = NULL: rat_logit_bwd / rat_logit_bwd_dnn exactly;
 * ddnn_b NULL: rat_logit_bwd's form. */
int rat_logit_bwd_pool(const float* y_pred, const float* y_true, const float* cls, int64_t cls_stride, const float* fc_w,
                       float* dlogit, float* dcls, int64_t dcls_stride, float* dfc_w, float* dfc_b, float* ddnn_b,
                       const RatField* lr_grad_fields_dev, const float* lr_den, int nfields, const int32_t* idx, int64_t idx_stride,
                       float gscale, const float* gscale_dev, int B, int d, int head, void* stream);

/* ---- K1s: row-sparse / deterministic embedding gradients (BASELINE.json configs[3]; SURVEY.md §2a rows H/I, §7 hard parts 3, 7)
 * replaces, for tables too large for dense semantics, embedding_dense_backward + the dense clip/Adam pass over the tables
 * (embedding.py:158-178 with sparse=False; base_model.py:221-225; torch_utils.py:41-49) and, for every table size, the fp32
 * atomics of rat_gather_bwd by a bit-reproducible sorted segmented reduction.
 *   plan   : (sample, id column) pairs -> key = global row = (fields[f].table - flat_base)/width + id (padding ids, ids outside the
 *            vocabulary and columns with col2field < 0 take no part); stable radix sort; *count_out = number of unique rows U
 *            (device int32; never read back by the library).  target_only: only the t == 0 rows of idx (the LR tables).
 *   reduce : segment sums in sorted (= batch) order -> out_rows [U] int32, out_grads [U][d] (either may be NULL) and / or straight
 *            into a dense gradient block (dense_base + row*d; plain stores, untouched rows are the caller's zeros).
 *            _grid: source rows dgrid [B][T][1+nfields][d] (+ dflat [B][nfields*d] on target rows, as rat_gather_bwd);
 *            _rows: source = gathered lists of `world` ranks, each `cap` entries long with counts_dev[r] valid (all-gather);
 *            _scalar: width-1 tables, source = one value per sample (dlogit [B]; plan built with target_only).
 *   rat_sumsq_rows / rat_adam_rows: gradient-norm contribution and clip + Adam of the U listed rows only ("lazy" Adam: moments
 *            of untouched rows do not decay — declared deviation, exact when every row is touched every step).
 * workspace: rat_sparse_workspace(n) bytes for n = pairs (B*T*L, or B*L with target_only, or cap*world); the same workspace is
 * handed to the matching reduce call. */
/* deterministic gradient of the 3-row label table (RAT_m2.py:64-65): dlabel_table [3][d] += per-block partial sums combined in
 * block order (rat_gather_bwd's version reduces through LDS / global atomics).  workspace: rat_label_grad_workspace(d) bytes. */
size_t rat_label_grad_workspace(int d);
int rat_label_grad(const float* dgrid, const int32_t* label_ids, float* dlabel_table, float* workspace, int64_t nbt, int S,
                   int d, void* stream);
size_t rat_sparse_workspace(int64_t n);
int rat_sparse_plan_ids(const int32_t* idx, const RatField* fields_dev, const int32_t* col2field_dev, int nfields,
                        const float* flat_base, int width, int64_t total_rows, int B, int T, int L, int target_only,
                        void* workspace, size_t workspace_bytes, int32_t* count_out, void* stream);
int rat_sparse_plan_rows(const int32_t* rows, const int32_t* counts_dev, int64_t cap, int world, int64_t total_rows,
                         void* workspace, size_t workspace_bytes, int32_t* count_out, void* stream);
int rat_sparse_reduce_grid(const void* workspace, const int32_t* count_dev, const float* dgrid, const float* dflat,
                           const int32_t* col2field_dev, int B, int T, int L, int nfields, int d, int target_only,
                           int32_t* out_rows, float* out_grads, float* dense_base, void* stream);
int rat_sparse_reduce_rows(const void* workspace, const int32_t* count_dev, const float* src_rows, int64_t cap, int world,
                           int d, int32_t* out_rows, float* out_grads, void* stream);
int rat_sparse_reduce_scalar(const void* workspace, const int32_t* count_dev, const float* per_sample, int B, int L,
                             int32_t* out_rows, float* out_vals, float* dense_base, void* stream);
/* rat_sparse_reduce_scalar with averaged LR fields: entry (b, column c) contributes per_sample[b] / lr_den[b][col2field_dev[c]]
 * (lr_den [B][nfields] from rat_logit_fwd_pool).  lr_den = NULL: rat_sparse_reduce_scalar exactly. */
int rat_sparse_reduce_scalar_pool(const void* workspace, const int32_t* count_dev, const float* per_sample, const float* lr_den,
                                  const int32_t* col2field_dev, int nfields, int B, int L, int32_t* out_rows, float* out_vals,
                                  float* dense_base, void* stream);
int rat_sumsq_rows(const float* grads, const int32_t* count_dev, int64_t max_rows, int d, float* norm_sq_out, void* stream);
int rat_adam_rows(float* w_base, float* m_base, float* v_base, const int32_t* rows, const float* grads,
                  const int32_t* count_dev, int64_t max_rows, int d, const float* norm_sq, float max_norm, float lr,
                  float beta1, float beta2, float eps, int step, void* stream);

/* ---- K4/K5: regulariser + clip_grad_norm_ + Adam over flat buffers -----------------------------------
 * base_model.py:79-94,224-225; torch_utils.py:41-49,65-81.
 * rat_l2_reg: for i<n: g[i] += lambda*w[i]; reg_out += (lambda/2)*sum w^2   (the "embedding_layer" tensors);
 *             lambda is multiplied by *lambda_scale_dev when that (device scalar, nullable) is given.
 * rat_sumsq : norm_sq_out += sum g^2 (fp32 partials, fp64-free two-stage tree; caller zeroes the scalar).
 * rat_clip_adam: coef = min(1, max_norm/(sqrt(*norm_sq)+1e-6)); g*=coef; Adam(lr,b1,b2,eps,step), in place. */
int rat_l2_reg(const float* w, float* g, int64_t n, float lambda, const float* lambda_scale_dev, float* reg_out,
               void* stream);
int rat_sumsq(const float* g, int64_t n, float* norm_sq_out, void* stream);
int rat_clip_adam(float* w, const float* g, float* m, float* v, int64_t n, const float* norm_sq,
                  float max_norm, float lr, float beta1, float beta2, float eps, int step, void* stream);

/* ---- ABI v4: the optimizer half of one training iteration in two sweeps, capturable in a hipGraph --------------------
 * base_model.py:79-94 (add_regularization), :221 (clip_grad_norm_), :224 (Adam.step), :220 (zero_grad) — the four dense passes
 * of rat_l2_reg + rat_sumsq + rat_clip_adam + the next step's zero-fill become:
 * rat_sumsq_reg      : *norm_sq_out += sum_i (g[i] + lam(i) w[i])^2, lam(i) = lam_a for i < n_split ("embedding_layer" tensors,
 *                      base_model.py:86) else lam_b (net_regularizer), both multiplied by *lam_scale_dev when given;
 *                      *reg_out (nullable) += sum_i (lam(i)/2) w[i]^2 — the regulariser's VALUE with the unscaled lambdas.
 *                      g is NOT modified: the regulariser gradient only ever exists in registers.
 * rat_clip_adam_fused: coef as rat_clip_adam; g' = (g + lam w) coef; Adam with step size hyper_dev[0] = lr/(1-beta1^t) and
 *                      hyper_dev[1] = 1/sqrt(1-beta2^t); zero_g: g[i] = 0 afterwards (optimizer.zero_grad() of the next step).
 * rat_adam_tick      : the optimizer's clock on the device: *step_dev += 1, hyper_out[0..2] = {lr/(1-beta1^t), 1/sqrt(1-beta2^t),
 *                      lr} from *lr_dev (double arithmetic like torch.optim.Adam's host code) — a replayed graph needs no new
 *                      kernel arguments.
 * rat_adam_rows_dev  : rat_adam_rows with the two step scalars read from hyper_dev.
 * Every optimizer entry point takes beta1 / beta2 / alpha (p0) as floats and forms 1 - beta and beta^t in double from the double
 * with the float's shortest round-trip decimal (0.999f -> 0.999), as torch.optim forms them from its Python floats: 1 - 0.999f is
 * 1.3e-5 (relative) off 0.001. */
int rat_adam_tick(int32_t* step_dev, const float* lr_dev, float beta1, float beta2, float* hyper_out, void* stream);
/* ABI v7 — what a fused training iteration starts with, in one launch: rat_adam_tick, scalars[0 .. nscalars) = 0 (the step's
 * accumulators: BCE sum, clip norm^2, regulariser value) and counters[i] += 1 for i < ncounters (nn.BatchNorm1d.num_batches_tracked of
 * every BatchNorm layer, int64).  Either list may be empty. */
int rat_step_begin(int32_t* step_dev, const float* lr_dev, float beta1, float beta2, float* hyper_out, float* scalars, int nscalars,
                   int64_t* counters, int ncounters, void* stream);
int rat_sumsq_reg(const float* g, const float* w, int64_t n, int64_t n_split, float lam_a, float lam_b,
                  const float* lam_scale_dev, float* norm_sq_out, float* reg_out, void* stream);
int rat_clip_adam_fused(float* w, float* g, float* m, float* v, int64_t n, int64_t n_split, float lam_a, float lam_b,
                        const float* lam_scale_dev, const float* norm_sq, float max_norm, const float* hyper_dev,
                        float beta1, float beta2, float eps, int zero_g, void* stream);
/* ABI v6 — the optimizers torch_utils.get_optimizer (torch_utils.py:41-49) builds besides Adam: getattr(torch.optim, name)(params,
 * lr=lr), i.e. torch's default hyper-parameters.  kind: RAT_OPT_SGD  w -= lr g;  RAT_OPT_ADAGRAD  s += g g, w -= lr g / (sqrt(s) + eps)
 * (eps 1e-10);  RAT_OPT_RMSPROP  s = p0 s + (1 - p0) g g, w -= lr g / (sqrt(s) + eps) (p0 = alpha 0.99, eps 1e-8).  `state` is the one
 * fp32 buffer of the parameters' shape these keep (NULL for SGD).  rat_clip_opt is the counterpart of rat_clip_adam (gradient already
 * holds the regulariser term), rat_clip_opt_fused of rat_clip_adam_fused (g + lambda w formed in registers, g left zero; lr read from
 * hyper_dev[2], which rat_adam_tick keeps current). */
#define RAT_OPT_ADAM 0
#define RAT_OPT_SGD 1
#define RAT_OPT_ADAGRAD 2
#define RAT_OPT_RMSPROP 3
int rat_clip_opt(float* w, const float* g, float* state, int64_t n, const float* norm_sq, float max_norm, float lr, int kind,
                 float p0, float eps, void* stream);
int rat_clip_opt_fused(float* w, float* g, float* state, int64_t n, int64_t n_split, float lam_a, float lam_b,
                       const float* lam_scale_dev, const float* norm_sq, float max_norm, const float* hyper_dev, int kind,
                       float p0, float eps, int zero_g, void* stream);
/* rat_scatter_rows: dense_base[rows[s]*d + c] = grads[s*d + c] for s < *count_dev — the merged (unique rows, gradient rows)
 * lists of all ranks written into the (zeroed) dense gradient block, so that the dense-semantics optimizer (regulariser on every
 * row, base_model.py:79-94) runs unchanged after a row-list exchange. */
int rat_scatter_rows(float* dense_base, const int32_t* rows, const float* grads, const int32_t* count_dev, int64_t max_rows,
                     int d, void* stream);
/* ABI v6 — the same for `lists` lists of capacity `cap` each (rows [lists][cap], grads [lists][cap][d], counts_dev [lists]): what the
 * owner-partitioned exchange of the table gradients leaves on every rank (one reduced list per owner rank, disjoint row ranges). */
int rat_scatter_rows_lists(float* dense_base, const int32_t* rows, const float* grads, const int32_t* counts_dev, int64_t cap,
                           int lists, int d, void* stream);
int rat_adam_rows_dev(float* w_base, float* m_base, float* v_base, const int32_t* rows, const float* grads,
                      const int32_t* count_dev, int64_t max_rows, int d, const float* norm_sq, float max_norm,
                      const float* hyper_dev, float beta1, float beta2, float eps, void* stream);

/* ABI v8 — the owner-partitioned exchange of the table-gradient row lists under data parallelism (the reference
 * has no counterpart — its DataParallel-less loop, base_model.py:213-230, runs on one device; this is the exchange step the sharded
 * path adds).  Rank k owns the rows [k per, (k + 1) per) of a table family.
 *   rat_owner_counts : counts_out[k] = unique rows of a rat_sparse_plan_* plan (workspace, count_dev, n as given to the plan) inside
 *                      owner k's range.  A function of the batch's IDS alone: it runs at the start of the step, the N x N matrix of
 *                      all ranks' counts is all-gathered and copied to the host while the forward runs.
 *   rat_owner_pack   : this rank's sorted lists (A: rows_a / grads_a [.][d]; B, nullable: rows_b / vals_b, width 1) -> `wire`, one
 *                      chunk per owner: [rows A pad 4][gradient rows A][rows B pad 4][values B pad 4] (32-bit words).
 *                      mat_dev: int32 [world][2][world], mat[s][f][k] = rows of family f rank s holds for owner k.
 *   rat_owner_unpack : the chunks received from ranks 0 .. world-1 -> contiguous (rows, gradient rows) pairs in rank order,
 *                      totals[0..1] = pairs received per family; n_extra floats are copied from extra_src to extra_dst.
 *   rat_owner_scatter: `world` all-gathered lists, `stride` words apart, each [count A, count B, -, -][n_extra floats pad 4]
 *                      [rows A: cap_a][gradient rows A: cap_a x d][rows B: cap_b][values B: cap_b] -> dense_a[row * d + c],
 *                      dense_b[row] (plain stores: the owners' ranges are disjoint); extra_out[i] = sum over the lists, in order.
 * max_pairs only sizes the grid. */
int rat_owner_counts(const void* workspace, const int32_t* count_dev, int64_t n, int64_t rows_per_owner, int world,
                     int32_t* counts_out, void* stream);
int rat_owner_pack(const int32_t* mat_dev, int world, int rank, int d, const int32_t* rows_a, const float* grads_a,
                   const int32_t* rows_b, const float* vals_b, int64_t max_pairs, float* wire, void* stream);
int rat_owner_unpack(const int32_t* mat_dev, int world, int rank, int d, const float* wire, int64_t max_pairs, int32_t* rows_a,
                     float* grads_a, int32_t* rows_b, float* vals_b, int32_t* totals, const float* extra_src, float* extra_dst,
                     int n_extra, void* stream);
int rat_owner_scatter(float* dense_a, float* dense_b, float* extra_out, const float* lists, int64_t stride, int world,
                      int64_t cap_a, int64_t cap_b, int d, int n_extra, void* stream);

/* Inverted dropout (nn.Dropout; RAT_m2.py:83,135 emb_dropout, deep.py:133-134 net_dropout): y = keep(seed,i) ? x/(1-p) : 0
 * with a counter-based mask, so the backward pass calls the same function on the gradient with the same seed.
 * In place (y == x) is allowed. */
int rat_dropout(const float* x, float* y, int64_t n, float p, uint64_t seed, void* stream);
/* ABI v6 — the same with the seed read from device memory, and the once-per-training-step refresh of a model's seed words:
 * counter_dev[0] += 1; seeds_dev[i] = mix(base_seed, counter, i), i < n.  nn.Dropout draws from torch's generator on every call
 * (RAT_m2.py:135,186-189, deep.py:133-134); here the generator's state is (base_seed, counter) on the device, so forward and backward
 * of a step agree on the masks (backward reads the same words) and a captured step needs no host-drawn seed. */
/* ABI v6 — FeedForward WITH its two nn.Dropout layers (RAT_m1.py:151-161, RAT_m0.py:150-160: Linear, GELU, Dropout, Linear, Dropout),
 * training mode: y = Dropout2(W2 Dropout1(gelu(W1 x + b1)) + b2) + res, and its backward (dx = [dy +] chain; the residual takes the
 * unmasked dy).  p: the rate both layers share; seed1_dev / seed2_dev: their seed words (rat_dropout_seeds).  Arguments otherwise as
 * rat_ffn_fwd_res / rat_ffn_bwd_res; exact fp32 on the generic kernels (RAT_m2 / RAT_m3 build FeedForward without dropout). */
int rat_ffn_fwd_drop(const float* x, const float* res, float* y, const float* w1, const float* b1, const float* w2, const float* b2,
                     int64_t ntok, int d, int hidden, float p, const uint64_t* seed1_dev, const uint64_t* seed2_dev, void* stream);
int rat_ffn_bwd_drop(const float* x, const float* dy, float* dx, const float* w1, const float* b1, const float* w2, const float* b2,
                     float* dw1, float* db1, float* dw2, float* db2, float* workspace, size_t workspace_bytes, int64_t ntok, int d,
                     int hidden, int add_dy, float p, const uint64_t* seed1_dev, const uint64_t* seed2_dev, void* stream);
int rat_dropout_dev(const float* x, float* y, int64_t n, float p, const uint64_t* seed_dev, void* stream);
int rat_dropout_seeds(uint64_t* seeds_dev, int n, uint64_t base_seed, uint64_t* counter_dev, void* stream);

/* Evaluation metrics on the device (csrc/metrics.hip): logloss, AUC and the per-group GAUC of n predictions, replacing the reference's
 * host pass (fuxictr/metrics.py:22-41: sklearn log_loss / roc_auc_score over numpy copies; GAUC, fuxictr/metrics.py:29-39, is `pass`
 * there).  y_pred, y_true: fp32 [n]; group: int32 [n] or NULL (no GAUC) — any int32 is a legal group id, it is a sort key only.
 * 1 <= n <= 2^31 - 1.  The caller owns every buffer; nothing is allocated, synchronised or read back.
 *   out (float64 [8], device): [0] logloss = mean of -(y log p + (1 - y) log(1 - p)) in float64, p = clip(double(pred), 1e-7, 1 - 1e-7),
 *       summed over fixed 1024-row tiles in index order (independent of scheduling);
 *   [1] AUC = U2 / (2 pos neg), U2 = sum over runs of equal predictions, ascending, of pos_run (2 neg_before_run + neg_run) in int64
 *       (-0.0 ties with +0.0; pos means y_true == 1): exact, one division;
 *   [2] GAUC = sum_g n_g AUC_g / sum_g n_g over the groups that hold both classes, n_g = rows of group g (the definition later FuxiCTR
 *       releases use), summed in ascending group order through a fixed tree: independent of the order of the rows; NaN when group == NULL;
 *   [3] n_pos  [4] n_neg  [5] groups counted  [6] rows in the counted groups
 *   [7] status bits: 1 a prediction is NaN (logloss, AUC, GAUC = NaN), 2 a label is neither 0 nor 1 (AUC, GAUC = NaN), 4 only one class
 *       present (AUC, GAUC = NaN), 8 groups given and none holds both classes (GAUC = NaN).
 * workspace: rat_eval_metrics_workspace(n, group != NULL) bytes, 256-byte aligned.  -1 + rat_last_error() on a null pointer, n out of
 * range, a workspace too small or misaligned; nothing is launched then. */
size_t rat_eval_metrics_workspace(int64_t n, int grouped);
int rat_eval_metrics(const float* y_pred, const float* y_true, const int32_t* group, int64_t n, double* out, void* workspace,
                     size_t workspace_bytes, void* stream);

/* Ranking metrics on the device (csrc/rankmetrics.hip): NDCG@k, MRR@k and HitRate@k per group, as later FuxiCTR releases report them
 * beside gAUC (the reference checked out beside this project has none of them).  y_pred, y_true: fp32 [n], every label 0 or 1; group:
 * int32 [n], a sort key only — any int32 is legal; cutoffs: int32 [n_cutoffs] on the HOST, 1 <= n_cutoffs <= 8, 1 <= k <= 2^31 - 1 (a
 * cutoff k >= n means "no cutoff"); 1 <= n <= 2^31 - 1.  The caller owns every buffer; nothing is allocated, synchronised or read back.
 *   Order inside a group: np.argsort(-p_g, kind="stable") over the group's rows in input order — descending prediction, ties keep input
 *     order, -0.0 equal to +0.0 (the order rat_rank_seg documents).  A row's place r is 0-based.
 *   Counted groups: a group counts if it holds at least one positive (y == 1); a group without one is skipped.  Each metric is the
 *     unweighted mean over the counted groups.  For a counted group with P positives and f the place of its first positive:
 *       DCG@k = sum_{r < k, y_r = 1} 1 / log2(r + 2)     IDCG@k = sum_{j < min(P, k)} 1 / log2(j + 2)     NDCG@k = DCG@k / IDCG@k
 *       MRR@k = 1 / (f + 1) if f < k, else 0             HitRate@k = 1 if f < k, else 0.                   All arithmetic is float64.
 *   out (float64 [n_cutoffs][8], device), per cutoff: [0] NDCG  [1] MRR  [2] HitRate = hits / counted, one division of two exact
 *     integers  [3] groups counted  [4] groups seen  [5] hits, the counted groups with f < k  [6] k  [7] status bits: 1 a prediction is
 *     NaN, 2 a label is neither 0 nor 1 (as in rat_eval_metrics), 16 no group holds a positive — any of them makes [0..2] NaN.
 *   The sums run in sorted order through fixed trees and one bitwise-reproducible scan per call: the result is a function of the inputs
 *   alone (of n and the sorted rows), not of scheduling; a row of out does not depend on the other cutoffs of the call.
 * workspace: rat_eval_rank_metrics_workspace(n, n_cutoffs) bytes, 256-byte aligned.  -1 + rat_last_error() on a null pointer (group
 * included), n or n_cutoffs out of range, a cutoff < 1, a workspace too small or misaligned; nothing is launched then. */
size_t rat_eval_rank_metrics_workspace(int64_t n, int n_cutoffs);
int rat_eval_rank_metrics(const float* y_pred, const float* y_true, const int32_t* group, int64_t n, const int32_t* cutoffs, int n_cutoffs,
                          double* out, void* workspace, size_t workspace_bytes, void* stream);

/* The end of a request on the device (csrc/topn.hip; rat_amd/online.py: top_requests, top_candidates): a request is one user with a
 * slate of candidates, and the caller wants the best n of them.  Both entry points take first_row (int64 [B], device) — for every
 * batch row the row that opens its request, what rat_bm25_query_prepare_seg takes — and use f(b) = clamp(first_row[b], 0, B - 1):
 * row h is a HEAD iff f(h) == h, its segment is h .. e - 1 with e the smallest j > h with f(j) != h, or B.  For valid first_row the
 * segments are the requests; NO content of first_row (or of cols) leads to an address outside the buffers.  One launch each on
 * `stream`, no atomics, nothing allocated, synchronised or read back.  -1 + rat_last_error() on a null pointer, B < 1 (or > 2^31 - 1),
 * n, L or W out of range; nothing is launched then.
 *
 * rat_topn_seg: y fp32 [B] -> out_pos int32 [B][n], out_val fp32 [B][n], out_len int32 [B], 1 <= n <= RAT_MAX_TOPN.  At a head h:
 *   out_len[h] = min(n, e - h); out_pos[h][i], i < out_len[h]: the positions INSIDE the segment (0-based) of its largest values, in
 *   the order "a before b iff y[a] > y[b], or neither compares greater and a < b" with a NaN after every number — equal values (and
 *   -0.0 / +0.0) by ascending position, NaNs among themselves by position: np.argsort(-y_seg, kind="stable")[:n] for any input;
 *   out_val[h][i] = y[h + out_pos[h][i]], the same bits (y is only compared); the remaining entries are -1 and 0.0.  Every other row:
 *   out_len 0 and a row of -1 / 0.0.  Every output element is written by every launch; the result is a function of the inputs alone.
 *
 * rat_candidates_expand: out[b][l] (int32 [B][L]) = cand[b][w] (int32 [B][W]) where l == cols[w] (int32 [W], device; distinct, in
 *   [0, L) — an entry outside is skipped), otherwise ctx[f(b)][l] (int32 [B][L]: row h holds the context of the request that opens at
 *   h; no other row is read).  1 <= L, W <= 8192.  16-byte accesses when L % 4 == 0 and ctx / out are 16-byte aligned. */
#define RAT_MAX_TOPN 64
int rat_topn_seg(const float* y, const int64_t* first_row, int64_t B, int n, int32_t* out_pos, float* out_val, int32_t* out_len,
                 void* stream);
int rat_candidates_expand(const int32_t* ctx, const int32_t* cand, const int32_t* cols, const int64_t* first_row, int64_t B, int L,
                          int W, int32_t* out, void* stream);

/* Every request's WHOLE ranking on the device (csrc/rank.hip; rat_amd/online.py: rank_requests, rank_candidates) — rat_topn_seg
 * returns a page of n <= RAT_MAX_TOPN, this the full order.  first_row, f, heads and segments as above; row b is a MEMBER of segment h
 * iff h is a head and h <= b < e.  Segments are disjoint; for valid first_row every row is a member of its request's segment.
 *
 * rat_rank_seg: y fp32 [B] -> out_order int32 [B], out_val fp32 [B], out_rank int32 [B].  For a member b of segment h:
 *   out_rank[b] = the number of members of the segment that come before b in rat_topn_seg's total order — a before b iff
 *   y[a] > y[b], or neither compares greater and a < b; a NaN after every number, NaNs among themselves by position, -0.0 and +0.0
 *   tie: np.argsort(-y[h:e], kind="stable") for any input; out_order[h + out_rank[b]] = b - h, the position inside the segment;
 *   out_val[h + i] = y[h + out_order[h + i]], the same bits (y is only compared).  A row that is a member of no segment gets
 *   -1 / 0.0 / -1.  Every output element is written by every launch; the result is a function of the inputs alone.
 * Any segment length is served.  One launch on `stream`, no atomics, no workspace, nothing allocated, synchronised or read back; NO
 * content of first_row leads to an address outside the four buffers.  -1 + rat_last_error() on a null pointer, B < 1 or
 * B > 2^31 - 1; nothing is launched then. */
int rat_rank_seg(const float* y, const int64_t* first_row, int64_t B, int32_t* out_order, float* out_val, int32_t* out_rank,
                 void* stream);

/* A device-resident item catalogue (csrc/catalogue.hip; rat_amd/online.py: set_catalogue, top_items, rank_items, top_catalogue):
 * cat int32 [M][W] holds, for each of M items, the ids of the W columns `cols` of the encoded row, and a candidate is an INDEX into
 * it.  first_row, f, heads and segments as rat_topn_seg documents them.  One launch each on `stream`, no atomics, nothing allocated,
 * synchronised or read back; every output element is written by every launch; NO content of any argument — first_row, items, cols,
 * heads, the lists and their offsets, the pages and their lengths, item0 — leads to an address outside the buffers (rows, items, heads,
 * lengths and offsets are clamped before they index anything).  -1 + rat_last_error() on a null pointer, B, R or M < 1 (or > 2^31 - 1),
 * L, W or n out of range, E < 0, rows_per_request < 1; nothing is launched then.
 *
 * rat_catalogue_expand: out[b][l] (int32 [B][L]) = cat[i(b)][w] where l == cols[w] (int32 [W], device; distinct, in [0, L) — an entry
 *   outside is skipped), otherwise ctx[f(b)][l] (int32 [B][L]; head rows only are read).  items (int32 [B]) given:
 *   i(b) = clamp(items[b], 0, M - 1).  items == NULL, the SWEEP form: i(b) = clamp(item0 + (b - f(b)), 0, M - 1) — the k-th row of a
 *   request is catalogue item item0 + k.  1 <= L, W <= 8192.  16-byte accesses when L % 4 == 0 and ctx / out are 16-byte aligned.
 *
 * Exclusion lists: ex_items int32 [E], ex_offsets int64 [R + 1]; request r's list is ex_items[lo .. hi) with
 *   lo = clamp(ex_offsets[r], 0, E), hi = clamp(ex_offsets[r + 1], lo, E).  It is ASCENDING and searched by lower bound: an unsorted
 *   list gives a wrong answer but never a wrong address.  E == 0 allows ex_items == NULL.
 *
 * rat_topn_exclude: out_y[b] (fp32 [B]) = -inf when the catalogue item of row b, item0 + (b - f(b)), is in the list of request
 *   r = clamp(f(b) / rows_per_request, 0, R - 1), otherwise y[b] with the same bits.
 *
 * rat_topn_merge: merges a chunk's page into the running page of each of R requests, IN PLACE.  Running page: run_item int32 [R][n],
 *   run_val fp32 [R][n], run_len int32 [R] (clamped to [0, n]); the chunk's page: rat_topn_seg's pos / val / len ([B][n], [B][n],
 *   [B]) read at row clamp(heads[r], 0, B - 1) (heads int64 [R]), an entry's item = item0 + pos.  Chunk entries whose item is in
 *   request r's list are dropped first — by lookup, not by value; ex_items == NULL (then ex_offsets may be NULL too): nothing is
 *   dropped.  The merged order is rat_topn_seg's total order over (value, item): a before b iff val[a] > val[b], or neither compares
 *   greater and a stands first — a running entry before a chunk entry (a sweep visits items in ascending order), inside a page the
 *   lower slot; a NaN after every number, -0.0 ties with +0.0.  The first n survive, run_len = min(n, entries kept), the tail is
 *   -1 / 0.0.  Values are moved, never computed with.  1 <= n <= RAT_MAX_TOPN. */
int rat_catalogue_expand(const int32_t* ctx, const int32_t* cat, const int32_t* items, int64_t item0, const int32_t* cols,
                         const int64_t* first_row, int64_t B, int L, int W, int64_t M, int32_t* out, void* stream);
int rat_topn_exclude(const float* y, const int64_t* first_row, int64_t item0, int64_t rows_per_request, const int32_t* ex_items,
                     const int64_t* ex_offsets, int64_t E, int64_t R, int64_t B, float* out_y, void* stream);
int rat_topn_merge(int32_t* run_item, float* run_val, int32_t* run_len, const int32_t* pos, const float* val, const int32_t* len,
                   const int64_t* heads, int64_t item0, const int32_t* ex_items, const int64_t* ex_offsets, int64_t E, int64_t R,
                   int64_t B, int n, void* stream);

/* Candidate retrieval through posting lists (csrc/postings.hip; additive in ABI v9; rat_amd/online.py: build_postings,
 * retrieve_shared) for requests whose rows share a context: the rows of a request equal each other on every used column outside the
 * VARYING ones, vary_mask (bit f = used column f < n_fields varies; bits at or past n_fields are ignored).
 *
 * The index: post_ids / post_rows int32 [n_fields][capacity] hold, per used column, the ids and the rows of the pool rows
 * [0, n_sorted) sorted by (id, row); n_sorted_dev is one int64 in device memory, clamped to [0, n].  The pool is taken in form
 * RAT_POOL_HOST or RAT_POOL_DEV (db_ids_field_major [n_fields][capacity], capacity <= 2^31 - 1); RAT_POOL_RING is refused.
 * ctx_indices int64 [n_ctx][topk] (-1 padded) holds, per request, the topk best indexed rows under the weights with the varying
 * columns set to 0.0 — rat_bm25_topk_split_before over the requests' head rows with before = n_sorted —, and ctx_row int64 [n_qry]
 * names the list of query b (clamped to [0, n_ctx)).
 *
 * Per query the candidates are (1) for each varying column, ascending, the posting list of the query's id (the range between a
 * lower and an upper bound in post_ids), a row taken only if it equals the query in no earlier varying column; (2) the entries of
 * its context list that equal it in no varying column; (3) the tail rows [n_sorted, n).  Every candidate is scored in full as
 * rat_bm25_topk scores — fp64, (db == q) * idf, f ascending over all n_fields, score > 0 kept — and the outputs follow
 * rat_bm25_topk's contract (fp64 [n_qry][topk], int64 [n_qry][topk] with -1 / 0.0 padding, int64 [n_qry]; score descending, index
 * ascending).  With weights >= 0, the rows of a request equal outside the varying columns and the lists built as above, the result
 * equals rat_bm25_topk over the live rows with the same qry_idf bit for bit.
 *
 * One launch on `stream`: no atomics, nothing allocated, synchronised or read back.  A posting row or context index outside
 * [0, n_sorted) is skipped before it addresses anything: corrupt lists, counts or ctx_row give a wrong answer, never a wrong address.
 * -1 + rat_last_error() and no launch on a null pointer, RAT_POOL_RING, n_fields or topk outside [1, 32], n_qry < 1, n_ctx < 1. */
int rat_bm25_topk_postings(const int32_t* db_ids_field_major, int pool_form, const int64_t* header_dev, int64_t n_rows,
                           int64_t capacity, const int32_t* post_ids, const int32_t* post_rows, const int64_t* n_sorted_dev,
                           const int32_t* qry_ids, const double* qry_idf, uint32_t vary_mask, const int64_t* ctx_indices,
                           const int64_t* ctx_row, int64_t n_ctx, double* out_values, int64_t* out_indices, int64_t* out_lens,
                           int64_t n_qry, int n_fields, int topk, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RAT_HIP_H_ */
