/*
 * dsvg.h — C ABI of libdsvg_hip.so: the gfx950 (MI355X) kernels behind the DeepSVG
 * SVGTransformer forward/backward hot path.
 *
 * The reference (alexandre01/deepsvg) has no FFI for this path: every op is a stock aten op
 * reached through torch.nn / torch.nn.functional.  Each entry point below therefore cites the
 * reference call site (file:line under /root/reference) whose arithmetic it replaces.  The
 * Python host (deepsvg_amd/ops.py) binds these with ctypes; see INTEGRATION.md.
 *
 * Conventions
 *  - Every buffer is owned by the caller (PyTorch); the library allocates nothing persistent.
 *  - All work is enqueued on `stream` (a hipStream_t passed as void*); no implicit syncs.
 *  - Return 0 on success, <0 on error; dsvg_last_error() returns a thread-local message.
 *  - dtype: DSVG_F32 (parity path, exact-fp32 MFMA) or DSVG_BF16 (bf16 storage, fp32 accumulate).
 *  - "seed" is a device pointer to a uint64 so a captured hipGraph re-reads it on every replay.
 *  - Token-major activations: row index t = sequence * S + position; feature index contiguous.
 */
#ifndef DSVG_H
#define DSVG_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DSVG_F32 0
#define DSVG_BF16 1
#define DSVG_I64 2 /* an input dtype of dsvg_sample_points / dsvg_raster_segments / dsvg_canonicalize only */

/* ABI version: bumped on EVERY change of an exported signature (round 4: 2 - dsvg_ffn_bwd_one and
 * dsvg_attn_block_fwd_stages removed, round 3's signature changes of dsvg_defer_scope / dsvg_gather_groups /
 * dsvg_bcast_add_bwd / dsvg_loss_targets / dsvg_scatter_rows counted).  dsvg_version() returns the value the library was
 * built with; a caller compiled against another header must refuse to run (deepsvg_amd/lib.py does).
 * 3: dsvg_latent_chain_fwd / dsvg_latent_chain_bwd added.  4: seq_add_ld argument of dsvg_attn_block_fwd / dsvg_gs_layer_fwd.
 * 5 (round 5): dsvg_sample_rows / dsvg_head_sample (categorical sampling on the device), dsvg_layernorm_bwd_masked added.
 * 6: dsvg_pack_images, dsvg_defer_zero added; dg argument of dsvg_gs_layer_bwd.
 * 7 (round 6): the one-launch attention input gradient added (removed in 18); a layer of dsvg_attn_pack_bwd grew from 128 to
 *    512 fragments (in_proj_weight^T behind out_proj.weight^T).
 * 8 (round 6): dsvg_gs_stack_fwd / dsvg_gs_stack_bwd added (one launch per STACK of group-stage layers).
 * 9 (round 6): dg_ld argument of dsvg_bcast_add_bwd / dsvg_bcast_add_bwd_masked (dg as a column block of a wider buffer).
 * 10: dsvg_ffn_gate_dw2 added (the gated dpre GEMM and the dW2 split-K GEMM of the fused FFN backward as one launch).
 * 11: two-stage configs with paths of 65..256 tokens: dsvg_build_masks_lens, dsvg_pack_tokens_lens, dsvg_packed_mean_fwd /
 *     bwd, dsvg_attention_long_packed_fwd / bwd, dsvg_attention_long_mfma_fwd / bwd added.
 * 12: dsvg_ffn_bwd removed (the fully fused FFN backward: no caller since round 2; dsvg_ffn_bwd_dx is the FFN backward's kernel).
 * 13: dsvg_sample_points / dsvg_chamfer (+ dsvg_chamfer_workspace_bytes) added (reconstruction error of decoded icons, evaluation only); DSVG_I64.
 * 14: dsvg_chamfer_nn / dsvg_chamfer_bwd / dsvg_sample_points_bwd added (the gradient of the reconstruction error).
 * 15: dsvg_emd (+ dsvg_emd_workspace_bytes) / dsvg_emd_bwd / dsvg_polyline_length / dsvg_polyline_length_bwd added (the ordered
 *     point loss and the length losses of deepsvg/difflib/loss.py).
 * 16: dsvg_raster_segments (+ dsvg_raster_workspace_bytes) / dsvg_raster_sweep added (images of a decoded batch).
 * 17: dsvg_raster_sweep_nn / dsvg_raster_sweep_bwd / dsvg_raster_segments_bwd added (the gradient of an image).
 * 18: the one-launch attention input gradient of version 7 removed: its entry point, its workspace query and its debug clock
 *     (opt-in since round 6, never ahead of the two launches it replaced); a layer of dsvg_attn_pack_bwd is back to 128
 *     fragments (out_proj.weight^T only).
 * 19: dsvg_canonicalize added (the canonical path order of SVG.canonicalize for a whole batch).
 *     Still 19: dsvg_paths_expand added (split and arc conversion for a whole batch).  No exported signature changed, and a
 *     library built without it fails to load by the missing symbol; tests/test_paths_host.py pins 19 for the binding.
 *     Still 19: dsvg_paths_simplify (+ dsvg_paths_simplify_workspace_bytes) added (the Bezier fit of SVGPath.simplify for a
 *     whole batch), on the same terms.
 *     Still 19: dsvg_paths_transform / dsvg_assemble_augmented added (affine step programs for a whole batch, and batch
 *     assembly over a float32 store with the augmentation applied on load), on the same terms.
 *     Still 19: dsvg_raster_segments_layers / dsvg_raster_sweep_layers added (layered RGB images: per-group outline, fill and
 *     erase, colours and opacities), on the same terms.
 *     Still 19: dsvg_overlap_counts / dsvg_filling_from_counts added (filling of a decoded batch), on the same terms.
 *     Still 19: dsvg_raster_sweep_layers_nn / dsvg_raster_blend_bwd / dsvg_raster_sweep_layers_bwd /
 *     dsvg_raster_segments_layers_bwd added (the gradient of a layered image), on the same terms.
 *     Still 19: dsvg_svg_parse added (SVG path text to padded rows for a whole batch), on the same terms: four host tests pin 19
 *     for the bindings they cover, and no exported signature changed.
 *     Still 19: dsvg_svg_parse_exact added (the same call with the exact number rule), on the same terms; dsvg_svg_parse keeps
 *     its 16 parameters and its results. */
#define DSVG_ABI_VERSION 19

const char* dsvg_last_error(void);
int dsvg_version(void);

/* ------------------------------------------------------------------------------------------
 * GEMM with fused prologue/epilogue:  C = epi( sum_k A(m,k) * B(n,k) )
 *   epi(v) = [C +] [res +] drop( gate( act( v + bias [+ res if res_pre] ) ) )
 * Replaces aten::addmm / aten::mm of every nn.Linear on the path:
 *   deepsvg/model/layers/functional.py:92,249 (QKV, out-proj),
 *   deepsvg/model/layers/improved_transformer.py:52,131,139 (FFN, linear_global),
 *   deepsvg/model/model.py:50,183,197 (embed_fcn, VAE, bottleneck),
 *   deepsvg/model/basic_blocks.py:18,20,36-37,60-63 (heads, ResNet),
 * and the two backward matmuls autograd derives for each of them (deepsvg/train.py:98).
 * ------------------------------------------------------------------------------------------ */
typedef struct dsvg_gemm_desc {
    int32_t dtype;            /* element type of A, B, res, gate and (unless c_f32) C             */
    int32_t M, N, K;
    const void* A; int64_t lda; int32_t a_kc;   /* a_kc=1: A(m,k)=A[m*lda+k]  0: A[k*lda+m]      */
    const void* B; int64_t ldb; int32_t b_kc;   /* b_kc=1: B(n,k)=B[n*ldb+k]  0: B[k*ldb+n]      */
    void* C; int64_t ldc; int32_t c_f32;        /* C[m*ldc+n]; c_f32=1 forces fp32 output        */
    const float* bias;                          /* [N] fp32 or NULL                              */
    const void* res; int64_t ldres; int32_t res_pre; /* residual (may alias C)                   */
    int32_t act;                                /* 0 none, 1 relu                                */
    const void* gate; int64_t ldgate; float gate_scale; /* v *= gate_scale*(gate[m,n]>0)         */
    float drop_p; uint32_t drop_site;           /* epilogue dropout, element id = m*N+n          */
    float a_drop_p; uint32_t a_drop_site; int64_t a_drop_ld; /* dropout replay on operand A,
                                                   element id = storage_row*a_drop_ld+storage_col */
    const uint64_t* seed;                       /* device pointer (may be NULL when p==0)        */
    int32_t accumulate;                         /* C += result                                   */
    int32_t split_k; float* workspace; int64_t workspace_bytes; /* split over K (weight grads);
                                                   needs c_f32 output and no epilogue            */
    float* rowsum;                              /* optional fp32 [M]: rowsum[m] = sum_k A(m,k), i.e.
                                                   the bias gradient for free inside the weight-
                                                   gradient GEMM (only with split_k > 1)         */
    int32_t impl;                               /* 0 = best MFMA kernel, 1 = one-thread-per-output,
                                                   2 = register-staged MFMA kernel only, 3 / 4 = LDS-DMA
                                                   kernel with 2 / 1 LDS stages when eligible, 5 = weight-
                                                   stationary kernel when eligible, 6 = LDS-DMA kernel with
                                                   4 stages (asm DMA three K steps ahead; the default for
                                                   launches of <= 256 workgroups) (test knobs)      */
} dsvg_gemm_desc;

int dsvg_gemm(const dsvg_gemm_desc* d, void* stream);
/* workspace bytes dsvg_gemm needs for a given split_k (0 when split_k<=1) */
int64_t dsvg_gemm_workspace_bytes(int32_t M, int32_t N, int32_t split_k);

/* out[j] = (accumulate? out[j] : 0) + sum_{p<P} partial[p*n+j]   (fp32; deterministic order) */
int dsvg_reduce_partials(const float* partial, int64_t P, int64_t n, float* out, int32_t accumulate,
                         void* stream);

/* Deferred parameter-gradient reductions.  While a scope is open ON A STREAM (dsvg_defer_scope(1, s) ...
 * dsvg_defer_scope(0, s)) every partial-sum reduction this library is asked to launch on that stream (split-K slices of dsvg_gemm, the gamma/beta partials of
 * dsvg_layernorm_bwd, dsvg_colsum, dsvg_add_pos_bwd, dsvg_embed_scatter) whose data allows 16-byte accesses is queued
 * instead of launched: its destination is NOT valid and its workspace must stay untouched until dsvg_flush_deferred,
 * which performs all queued reductions in one launch per 64 of them (a backward pass of the benchmark model queues
 * ~130: the per-reduction launches were 0.85 ms of a 10.5 ms step).  A reduction whose destination overlaps a queued
 * one flushes the queue first, so write-after-write order is kept; reads of a queued destination are the caller's
 * responsibility (deepsvg_amd/trainer.py flushes right after loss.backward(), the reference's train.py:98).
 * The queue is keyed by the stream (hence by device): launches on other streams - another model, another trainer,
 * nn.DataParallel's per-device threads - are neither queued nor flushed by it, and the flush runs on the stream that
 * produced the queued partials, ordered behind them.  No state besides these per-stream queues is kept.
 * dsvg_defer_scope returns the number of reductions currently queued on that stream. */
int dsvg_defer_scope(int32_t on, void* stream);
/* out[0 .. n) = 0 (fp32): queued as a reduction over zero partial rows while a scope is open on the stream (the fill then costs
 * no launch of its own: the rows of a head's weight gradient that saw no loss term, functional.ArgsHeadLossFn), a plain
 * asynchronous memset otherwise.  Same ordering rules as the queued reductions. */
int dsvg_defer_zero(float* out, int64_t n, void* stream);
int dsvg_flush_deferred(void* stream);
/* Grouped weight-gradient launches.  While a group scope is open on a stream (dsvg_gemm_group_scope(1, s) ... (0, s)) every
 * split-K weight-gradient dsvg_gemm on that stream that would take the 4-stage LDS-DMA kernel (bf16, both operands
 * token-major, at most 256 workgroups) is queued, and closing the scope runs all of them as ONE launch (problem table in
 * the kernel arguments; each problem keeps its own grid, slices and workspace: bit-identical results).  The operands and
 * workspaces must stay alive and unchanged until the scope is closed; the split-K reductions of queued problems never run
 * before them (a flush of the deferred reductions, or an immediate reduction, launches the queued group first). */
int dsvg_gemm_group_scope(int32_t on, void* stream);

/* out[n] (+)= sum_m drop(A[m*lda+n])  — bias gradients (autograd of the `+ b` in every nn.Linear).
 * workspace: at least dsvg_colsum_workspace_bytes(M,N) bytes. */
int dsvg_colsum(int32_t dtype, const void* A, int64_t lda, int64_t M, int32_t N, float* out,
                int32_t accumulate, float drop_p, uint32_t drop_site, const uint64_t* seed,
                float* workspace, int64_t workspace_bytes, void* stream);
int64_t dsvg_colsum_workspace_bytes(int64_t M, int32_t N);

/* ------------------------------------------------------------------------------------------
 * LayerNorm over the last dimension (d % 4 == 0, d <= 1024), eps as given.
 * Replaces torch.nn.LayerNorm at deepsvg/model/layers/improved_transformer.py:43,51,127,138 and
 * deepsvg/model/layers/transformer.py:185-186,239-240.
 * bwd: dx = [res +] LN'(dy);  dgamma/dbeta partials go to workspace then are reduced into
 * dgamma/dbeta (fp32, overwritten unless accumulate).
 * ------------------------------------------------------------------------------------------ */
int dsvg_layernorm_fwd(int32_t dtype, const void* x, const float* gamma, const float* beta, void* y,
                       float* mean, float* rstd, int64_t rows, int32_t d, float eps, void* stream);
int dsvg_layernorm_bwd(int32_t dtype, const void* dy, const void* x, const float* mean,
                       const float* rstd, const float* gamma, const void* res, void* dx,
                       float* dgamma, float* dbeta, int32_t accumulate, int64_t rows, int32_t d,
                       float* workspace, int64_t workspace_bytes, void* stream);
int64_t dsvg_layernorm_bwd_workspace_bytes(int64_t rows, int32_t d);
/* the same with a second output: dx_masked = dsvg_drop_apply(dx, drop_p, drop_site) - the stored (rounded) dx with that
 * site's dropout mask replayed on it - from the same pass over the row (round 5: the FFN half of the layer below reads its
 * incoming gradient only through the mask of its residual dropout, deepsvg/model/layers/improved_transformer.py:53,140) */
int dsvg_layernorm_bwd_masked(int32_t dtype, const void* dy, const void* x, const float* mean, const float* rstd,
                              const float* gamma, const void* res, void* dx, float* dgamma, float* dbeta,
                              int32_t accumulate, int64_t rows, int32_t d, float* workspace, int64_t workspace_bytes,
                              void* dx_masked, float drop_p, uint32_t drop_site, const void* seed, void* stream);

/* ------------------------------------------------------------------------------------------
 * Multi-head self-attention core on packed QKV (after the in-projection):
 *   qkv[t, 0:d]=q, [d:2d]=k, [2d:3d]=v ; head h uses columns h*32..h*32+31 (head_dim must be 32);
 *   sequence b owns rows b*S..b*S+S-1 (S <= 64); key j of sequence b is visible iff bit j of
 *   key_mask[b] is set (NULL = all S keys).  q is scaled by `scale` after the bias add.
 *   out[t, h*32+c] = sum_j drop(softmax_j(scale*q_i.k_j))*v_j
 * Replaces deepsvg/model/layers/functional.py:168,197-248 (scale, reshape, bmm, masked_fill,
 * softmax, dropout, bmm, head merge).  bwd recomputes the probabilities (no S×S tensor in HBM).
 * Packed layout (seq_off != NULL, key_mask == NULL): sequence b owns rows seq_off[b]..seq_off[b+1]-1
 * (at most S of them, all visible); rows seq_off[n_seq]..total_rows-1 of out / dqkv are zero-filled.
 * Dense layout with total_rows > n_seq*S: rows n_seq*S..total_rows-1 of out / dqkv are zero-filled
 * (backward over a row prefix, see dsvg_visible_first); total_rows == 0: no tail.
 * tile_first (optional, packed layout only; from dsvg_attention_tiles): groups of consecutive sequences with
 * at most 32 rows in total are processed by one workgroup as a block-diagonal 32x32 score tile (bf16, S <= 32;
 * ignored by the other kernel variants).  Same results, ~3x fewer workgroups on the packed encoder.
 * ------------------------------------------------------------------------------------------ */
int dsvg_attention_fwd(int32_t dtype, const void* qkv, const uint64_t* key_mask, const int32_t* seq_off,
                       int64_t total_rows, const int32_t* tile_first, void* out, int64_t n_seq, int32_t S,
                       int32_t n_heads, float scale, float drop_p, uint32_t drop_site, const uint64_t* seed,
                       void* stream);
int dsvg_attention_bwd(int32_t dtype, const void* qkv, const uint64_t* key_mask, const int32_t* seq_off,
                       int64_t total_rows, const int32_t* tile_first, const void* dout, void* dqkv, int64_t n_seq,
                       int32_t S, int32_t n_heads, float scale, float drop_p, uint32_t drop_site,
                       const uint64_t* seed, void* stream);
/* tile_first: int32 [n_seq + 2]; tile j = sequences tile_first[j]..tile_first[j+1]-1 (sum of their lengths
 * <= max_rows; greedy inside segments of 64 consecutive sequences), tile_first[n_tiles] = n_seq,
 * tile_first[n_seq + 1] = n_tiles; scratch: int32 [ceil(n_seq / 64) * 64] */
int dsvg_attention_tiles(const int32_t* seq_off, int64_t n_seq, int32_t max_rows, int32_t* tile_first,
                         int32_t* scratch, void* stream);

/* ------------------------------------------------------------------------------------------
 * Masks from the command tensor (deepsvg/model/utils.py:7-66).  commands: float32 [n_seq, S]
 * (batch-first rows, values are command indices; EOS = eos_id).
 *   key_mask[b]   bit j set  <=>  no EOS at positions <= j   (complement of _get_key_padding_mask)
 *   seq_visible[b] = (#EOS in row b) < S-1                    (_get_visibility_mask)
 * and per group-of-G rows: group_mask[n] bit g = seq_visible[n*G+g]  (_get_key_visibility_mask)
 * ------------------------------------------------------------------------------------------ */
int dsvg_build_masks(const float* commands, int64_t n_seq, int32_t S, int32_t G, int32_t eos_id,
                     uint64_t* key_mask, int32_t* seq_visible, uint64_t* group_mask, void* stream);

/* ------------------------------------------------------------------------------------------
 * SVGEmbedding pieces (deepsvg/model/model.py:46-57):
 *  gather:  A[t, a*E:(a+1)*E] = arg_embed[args[t,a]+1]   (fp32 table -> dtype)  and
 *           R[t, :] = command_embed[commands[t]] (+ group_embed[groups[t]] when given)
 *  bwd:     d_arg_embed += scatter(dA), d_command_embed += scatter(dR), d_group_embed likewise.
 * ------------------------------------------------------------------------------------------ */
int dsvg_embed_gather(int32_t dtype, const float* commands, const float* args,
                      const float* command_embed, const float* arg_embed, const float* group_embed,
                      const int32_t* groups, void* A, void* R, int64_t T, int32_t n_args, int32_t E,
                      int32_t d, int32_t n_cmd, int32_t n_argvals, void* stream);
int dsvg_embed_scatter(int32_t dtype, const float* commands, const float* args,
                       const int32_t* groups, const void* dA, const void* dR, float* d_arg_embed,
                       float* d_command_embed, float* d_group_embed, int64_t T, int32_t n_args,
                       int32_t E, int32_t d, int32_t n_cmd, int32_t n_argvals, int32_t n_groups,
                       float* workspace, int64_t workspace_bytes, void* stream);
int64_t dsvg_embed_scatter_workspace_bytes(int64_t T, int32_t n_args, int32_t E, int32_t d,
                                           int32_t n_cmd, int32_t n_argvals, int32_t n_groups);
/* group index per token: groups[b*S+s] = #{ s' <= s : commands[b,s'] == m_id }  (utils.py:35-42) */
int dsvg_group_index(const float* commands, int64_t n_seq, int32_t S, int32_t m_id, int32_t* groups,
                     void* stream);
/* Visible-first order of the second decoder stage: its sequences are independent (one per group,
 * model/model.py:250-262) and SVGLoss excludes every position of an invisible target group (loss.py:36,51-54),
 * so those sequences have an identically zero backward pass; with the visible sequences first the backward
 * kernels run on a row prefix.  new_of_old / old_of_new: stable partition and its inverse. */
int dsvg_visible_first(const int32_t* visible, int64_t n, int32_t* new_of_old, int32_t* old_of_new,
                       int32_t* n_visible, void* stream);
/* dst[g*S + s, :] = src[idx[g]*S + s, :], g < n_groups: whole-sequence row gather (width % 4 == 0).  src holds n_src
 * groups: idx[g] >= n_src gives a zero sequence (the second decoder stage's forward runs on the visible sequences only;
 * the output rows of the others are zeros until somebody reads their logits), idx[g] < 0 (list padding) reads group 0 */
int dsvg_gather_groups(int32_t dtype, const void* src, const int32_t* idx, void* dst, int64_t n_groups,
                       int32_t S, int32_t width, int64_t n_src, void* stream);
/* Packed token layout of the first encoder stage: only keys are masked there (layers/functional.py:234-239)
 * and padded query rows are dropped by the mean-pool (model/model.py:137), so the encoder can run on the
 * valid tokens only, bit-for-bit safe.  seq_off[b] = exclusive scan of popcount(key_mask) (n_seq+1 entries,
 * seq_off[n_seq] = number of valid tokens); packed row seq_off[b]+s = token (b, s); rows past the total, up
 * to the capacity n_seq*S, replicate token 0.  packed_pos[row] = s (position index). */
int dsvg_pack_tokens(const float* commands, const float* args, const uint64_t* key_mask, int64_t n_seq,
                     int32_t S, int32_t n_args, int32_t* seq_off, float* packed_commands,
                     float* packed_args, int32_t* packed_pos, void* stream);

/* ------------------------------------------------------------------------------------------
 * y[t,:] = drop( (x ? x[t,:] : 0) + pos_embed[t % S, :] )
 * PositionalEncodingLUT.forward (deepsvg/model/layers/positional_encoding.py:40-43) and
 * ConstEmbedding.forward (deepsvg/model/model.py:70-73, x == NULL).
 * bwd: dx = dy*mask (if dx != NULL), d_pos[s,:] (+)= sum_b (dy*mask)[b*S+s,:]
 * ------------------------------------------------------------------------------------------ */
int dsvg_add_pos_fwd(int32_t dtype, const void* x, const float* pos, void* y, int64_t n_seq, int32_t S,
                     int32_t d, float drop_p, uint32_t drop_site, const uint64_t* seed, void* stream);
int dsvg_add_pos_bwd(int32_t dtype, const void* dy, void* dx, float* d_pos, int32_t accumulate,
                     int64_t n_seq, int32_t S, int32_t d, float drop_p, uint32_t drop_site,
                     const uint64_t* seed, float* workspace, int64_t workspace_bytes, void* stream);
int64_t dsvg_add_pos_bwd_workspace_bytes(int64_t n_seq, int32_t S, int32_t d);

/* ------------------------------------------------------------------------------------------
 * Masked mean over the sequence axis (deepsvg/model/model.py:137,161):
 *   out[b,:] = sum_{s in mask[b]} x[b*S+s,:] / popcount(mask[b])
 * Packed layout (seq_off != NULL): mean over rows seq_off[b]..seq_off[b+1]-1; bwd zero-fills the rows
 * seq_off[n_seq]..total_rows-1.
 * ------------------------------------------------------------------------------------------ */
int dsvg_masked_mean_fwd(int32_t dtype, const void* x, const uint64_t* mask, const int32_t* seq_off,
                         void* out, int64_t n_seq, int32_t S, int32_t d, void* stream);
int dsvg_masked_mean_bwd(int32_t dtype, const void* dout, const uint64_t* mask, const int32_t* seq_off,
                         int64_t total_rows, void* dx, int64_t n_seq, int32_t S, int32_t d, void* stream);

/* ------------------------------------------------------------------------------------------
 * x[t,:] += drop(g)[t / S, :]      "implicit broadcast" add of linear_global(z)
 * (deepsvg/model/layers/improved_transformer.py:131-136): the dropout acts on the per-sequence row BEFORE the
 * broadcast, as in the reference, so one mask element (id b*d + c) covers every position of sequence b.
 * bwd: dg[b,:] = mask[b,:] * sum_s dx[b*S+s,:] for b < n_seq; rows n_seq <= b < n_seq_out of dg are written as zeros (a
 *      backward pass restricted to a live prefix of the sequences: the others have zero gradient)
 * ------------------------------------------------------------------------------------------ */
int dsvg_bcast_add_fwd(int32_t dtype, void* x, const void* g, int64_t n_seq, int32_t S, int32_t d,
                       float drop_p, uint32_t drop_site, const uint64_t* seed, void* stream);
/* dg_ld (ABI 9): row stride (elements) of dg: d, or wider (bf16, d % 8 == 0, d <= 512, 16-byte aligned): dg is a column block of a
 * longer row - the layers of a decoder stack write their conditioning gradients side by side into ONE [n_seq_out, n_layers * d]
 * buffer, which is the concatenation GlobalCondFn's products read (no concatenation launch) */
int dsvg_bcast_add_bwd(int32_t dtype, const void* dx, void* dg, int64_t n_seq, int64_t n_seq_out, int32_t S, int32_t d,
                       float drop_p, uint32_t drop_site, const uint64_t* seed, int64_t dg_ld, void* stream);
/* bf16 only: dsvg_bcast_add_bwd AND dx_masked = dsvg_drop_apply(dx, drop_p, mask_site) over all `rows` rows of dx (n_seq * S <=
 * rows <= n_seq_out * S: a live row prefix may be rounded up past the summed sequences), from ONE read of dx (the large decoder
 * layers' backward needs both; d % 8 == 0, d <= 512, 16-byte aligned buffers, drop_p > 0) */
int dsvg_bcast_add_bwd_masked(const void* dx, void* dg, void* dx_masked, int64_t n_seq, int64_t n_seq_out, int32_t S, int32_t d,
                              int64_t rows, float drop_p, uint32_t drop_site, uint32_t mask_site, const uint64_t* seed,
                              int64_t dg_ld, void* stream);

/* ------------------------------------------------------------------------------------------
 * SVGLoss (deepsvg/model/loss.py:19-65).
 *  targets: from tgt_commands [n_seq,S1] / tgt_args [n_seq,S1,n_args] (float32, S1=S+1 incl. SOS)
 *    cmd_tgt[n_seq,S], cmd_w[n_seq,S] (extended padding mask x visibility, loss.py:35-36,49),
 *    arg_tgt[n_seq,S,n_args] (=arg+1), arg_w = CMD_ARGS_MASK[cmd] (loss.py:51), vis_tgt[n_seq];
 *    seq_perm (optional, int32 [n_seq]): the token-level outputs of sequence b are those of source sequence seq_perm[b]
 *    (the second decoder stage's visible-first order), vis_tgt stays in source order
 *  masked CE: logical row r of the [rows, C] matrix lives at logits + (r/group)*ld + (r%group)*C
 *    (group = n_args for args_logits, whose 11x257 slots are contiguous per token; 1 otherwise);
 *    lse per row, sum_count = {sum_r w_r*(lse_r - logit[r,target_r]), sum_r w_r}; rows with w==0
 *    are never read.  loss = sum/count is formed by the caller on device.
 *  ce_bwd: dlogits = w * (softmax - onehot) * coef * (*gscale) / count  [zeros where w == 0, and
 *    zeros in the [group*C, ld_d) row padding]
 * ------------------------------------------------------------------------------------------ */
int dsvg_loss_targets(const float* tgt_commands, const float* tgt_args, const float* cmd_args_mask,
                      int64_t n_seq, int32_t S1, int32_t n_args, int32_t n_cmd, int32_t eos_id,
                      int32_t* cmd_tgt, float* cmd_w, int32_t* arg_tgt, float* arg_w, int32_t* vis_tgt,
                      const int32_t* seq_perm, void* stream);
int dsvg_masked_ce_fwd(int32_t dtype, const void* logits, int64_t ld, int32_t group, const int32_t* target,
                       const float* w, int64_t rows, int32_t C, float* lse, float* sum_count,
                       float* workspace, int64_t workspace_bytes, const int32_t* tok_idx, void* stream);
int64_t dsvg_masked_ce_workspace_bytes(int64_t rows);
int dsvg_masked_ce_bwd(int32_t dtype, const void* logits, int64_t ld, int32_t group, const int32_t* target,
                       const float* w, const float* lse, const float* sum_count, const float* gscale,
                       float coef, void* dlogits, int64_t ld_d, int64_t rows, int32_t C,
                       const int32_t* tok_idx, int32_t logits_compact, void* stream);
/* The loss terms and their weighted total from the (sum, count) pairs of n <= 4 cross-entropies in one launch (host arrays
 * of device pointers / host weights): out[1 + i] = sum_i / count_i, out[0] = sum_i weights[i] * out[1 + i]
 * (deepsvg/model/loss.py:43-57), and its backward: dsum_count[2 i] = *dtotal * weights[i] + *dterms[i] (NULL pointers
 * count as zero), dsum_count[2 i + 1] = 0 - the value dsvg_masked_ce_bwd takes as `gscale`. */
int dsvg_loss_combine_fwd(const float* const* sum_count, const float* weights, int32_t n, float* out, void* stream);
int dsvg_loss_combine_bwd(const float* dtotal, const float* const* dterms, const float* weights, int32_t n,
                          float* dsum_count, void* stream);
/* tok_idx (optional): compact token list, output token i = source token tok_idx[i] (negative -> zero row / zero
 * weight), `rows` = listed tokens * group; targets and weights are always indexed by the source token.
 * fwd with tok_idx: `logits` and `lse` are compact (row i = listed token i): the loss of the argument head is
 * computed from logits of the loss-carrying tokens only.  bwd: logits_compact selects the same for its inputs.  dsvg_live_rows builds that list: the tokens with any non-zero weight among their
 * `group` rows, ascending, padded with -1 up to n_tok entries; *count = their number.  Rows the loss masks out
 * have exactly zero dlogits (deepsvg/model/loss.py:51-54), so the argument head's dX / dW need only those tokens. */
int dsvg_live_rows(const float* w, int64_t n_tok, int32_t group, int32_t* live, int32_t* count,
                   int32_t* workspace, int64_t workspace_bytes, void* stream);
int64_t dsvg_live_rows_workspace_bytes(int64_t n_tok);
/* dst[idx[i], :] = src[i, :] (accumulate: +=) for idx[i] >= 0 (width % 4 == 0, idx without duplicates); other rows of dst are
 * left untouched */
int dsvg_scatter_rows(int32_t dtype, const void* src, const int32_t* idx, void* dst, int64_t n_rows,
                      int32_t width, int32_t accumulate, void* stream);

/* ------------------------------------------------------------------------------------------
 * Flat-buffer optimizer step: clip_grad_norm_ (deepsvg/train.py:100) + AdamW
 * (deepsvg/config.py:64-65, torch.optim.AdamW defaults) on one contiguous fp32 parameter buffer.
 * ------------------------------------------------------------------------------------------ */
int dsvg_sumsq(const float* x, int64_t n, float* out /*[1]*/, float* workspace, int64_t workspace_bytes,
               void* stream);
int64_t dsvg_sumsq_workspace_bytes(int64_t n);
int dsvg_adamw_step(float* p, const float* g, float* m, float* v, int64_t n, const float* lr,
                    float beta1, float beta2, float eps, float weight_decay, const int64_t* step,
                    const float* gnorm_sq, float max_norm, float grad_scale, void* stream);
/* dst (dtype) = src (fp32), optional transposed copy: dst_t[c*rows+r] = src[r*cols+c] */
int dsvg_cast_weights(int32_t dtype, const float* src, void* dst, void* dst_t, int64_t rows,
                      int64_t cols, void* stream);
/* *counter += 1 ; *seed = hash(*seed)  — per-step dropout seed advance, graph-capturable */
int dsvg_advance_step(int64_t* counter, uint64_t* seed, void* stream);
/* Every per-step weight image of a bf16 model in ONE launch (csrc/pack_images.hip): what dsvg_cast_weights(DSVG_BF16, flat)
 * + dsvg_ffn_pack + dsvg_attn_pack + dsvg_attn_pack_bwd + dsvg_gs_pack + dsvg_advance_step write, bit for bit (the same
 * device code, csrc/pack_images.h), i.e. the `.to(bf16)` copies of the parameters an autocast forward of
 * deepsvg/model/model.py makes, laid out for the fused kernels.  n = elements of the flat buffers (a multiple of 8, both
 * 16-byte aligned).  A family with 0 layers is skipped; ffn_w2p, attn_bwd (only a backward pass reads it), counter and seed
 * may each be NULL (ffn_bwd, which only dsvg_ffn_bwd_dx reads, is required with the FFN family, as in dsvg_ffn_pack).
 * offs tables as in the stand-alone calls. */
int dsvg_pack_images(const float* flat_f32, void* flat_bf16, int64_t n,
                     const int64_t* ffn_offs, int32_t ffn_layers, void* ffn_fwd, void* ffn_bwd, float* ffn_b1f, void* ffn_w2p,
                     const int64_t* attn_offs, int32_t attn_layers, void* attn_img, void* attn_bwd,
                     const int64_t* gs_offs, int32_t gs_layers, void* gs_fwd, void* gs_bwd,
                     int64_t* counter, uint64_t* seed, void* stream);
/* n device-to-device copies dst[i][0 .. bytes[i]) = src[i][...] in one launch per 32 entries (the table travels in the kernel
 * arguments: capturable, no staging).  deepsvg_amd/trainer.py refreshes the static inputs and the layout plan of a hipGraph
 * step with it between two replays (they were ~20 separate copy launches). */
int dsvg_copy_many(const void* const* src, void* const* dst, const int64_t* bytes, int32_t n, void* stream);
/* out[i] = y[i] > 0 ? dy[i]*scale : 0 — backward of ReLU (basic_blocks.py:47-57) from the saved output */
int dsvg_gate_mul(int32_t dtype, const void* dy, const void* y, void* out, int64_t n, float scale, void* stream);
/* y[i] = x[i] * dropmask(seed, site, i): replay of an nn.Dropout mask on a gradient (n % 8 == 0) */
int dsvg_drop_apply(int32_t dtype, const void* x, void* y, int64_t n, float drop_p, uint32_t drop_site,
                    const uint64_t* seed, void* stream);
/* out[i] = a[i] + b[i] — the residual add of the latent ResNet (basic_blocks.py:59-65) */
int dsvg_add(int32_t dtype, const void* a, const void* b, void* out, int64_t n, void* stream);
/* Causal variant for the autoregressive decoder (pred_mode = "autoregressive": tgt_mask =
 * square_subsequent_mask, deepsvg/model/model.py:219-222,270; layers/functional.py:228-233): query row i attends the
 * keys j <= i that key_mask allows.  Dense layout only. */
int dsvg_attention_causal_fwd(int32_t dtype, const void* qkv, const uint64_t* key_mask, void* out, int64_t n_seq,
                              int32_t S, int32_t n_heads, float scale, float drop_p, uint32_t drop_site,
                              const uint64_t* seed, void* stream);
/* dsvg_attention_bwd with the out_proj backward inside (bf16, 8 heads of 32; dense sequences of 17 .. 32 rows, or the packed
 * tile layout): dx1m = gradient of the block's projected output with the residual dropout mask on it [rows, 256] (what
 * dsvg_drop_apply / dsvg_ffn_bwd_dx hand over), wo_packed_bwd = one layer of dsvg_attn_pack_bwd.  The head-output gradient
 * dO = dx1m . Wo is formed per tile on chip: replaces the `dao = dx1m @ out_proj.weight` GEMM launch (its 512 B / token
 * written and re-read) in front of dsvg_attention_bwd (autograd of layers/functional.py:248-249 + :197-247).
 * dsvg_attn_pack_bwd: offs[layer][1] = element offset of out_proj.weight in flat_f32 (the offs table of dsvg_attn_pack);
 * packed_bwd: dsvg_attn_pack_bwd_elems(n_layers) bf16 elements (128 x 512 per layer: the 128 fragments [head 8][K step 16] of
 * out_proj.weight^T; offs[layer][0] is not read). */
int dsvg_attention_bwd_outproj(const void* qkv, const uint64_t* key_mask, const int32_t* seq_off, int64_t total_rows,
                               const int32_t* tile_first, const void* dx1m, const void* wo_packed_bwd, void* dqkv,
                               int64_t n_seq, int32_t S, float scale, float drop_p, uint32_t drop_site,
                               const uint64_t* seed, void* stream);
int64_t dsvg_attn_pack_bwd_elems(int32_t n_layers);
int dsvg_attn_pack_bwd(const float* flat_f32, const int64_t* offs, int32_t n_layers, void* packed_bwd, void* stream);
int dsvg_attention_causal_bwd(int32_t dtype, const void* qkv, const uint64_t* key_mask, const void* dout, void* dqkv,
                              int64_t n_seq, int32_t S, int32_t n_heads, float scale, float drop_p,
                              uint32_t drop_site, const uint64_t* seed, void* stream);

/* ------------------------------------------------------------------------------------------
 * Sequences of more than 64 tokens (one-stage / autoregressive configs at the reference's default
 * max_total_len = 240, deepsvg/model/config.py:43,74-89).  The command masks are "before the first EOS"
 * (deepsvg/model/utils.py:7-32), i.e. a valid-prefix LENGTH per sequence instead of a 64-bit word:
 *   seq_lens:       lens[b] = index of the first EOS of commands[b, :] (S if there is none)
 *   attention_long: same contract as dsvg_attention_fwd/bwd on the dense layout (keys j < seq_len[b], NULL = all;
 *                   causal != 0: additionally j <= i), S <= 256, same dropout element ids; only_row >= 0 (forward,
 *                   causal): compute that query row alone (incremental decoding step), other rows of out untouched
 *   prefix_mean:    out[b,:] = mean_{s < lens[b]} x[b*S + s, :]  (deepsvg/model/model.py:137) and its backward
 * ------------------------------------------------------------------------------------------ */
int dsvg_seq_lens(const float* commands, int64_t n_seq, int32_t S, int32_t eos_id, int32_t* lens, void* stream);
int dsvg_attention_long_fwd(int32_t dtype, const void* qkv, const int32_t* seq_len, void* out, int64_t n_seq, int32_t S,
                            int32_t n_heads, float scale, int32_t causal, int32_t only_row, float drop_p,
                            uint32_t drop_site, const uint64_t* seed, void* stream);
int dsvg_attention_long_bwd(int32_t dtype, const void* qkv, const int32_t* seq_len, const void* dout, void* dqkv,
                            int64_t n_seq, int32_t S, int32_t n_heads, float scale, int32_t causal, float drop_p,
                            uint32_t drop_site, const uint64_t* seed, void* stream);
int dsvg_prefix_mean_fwd(int32_t dtype, const void* x, const int32_t* lens, void* out, int64_t n_seq, int32_t S, int32_t d,
                         void* stream);
int dsvg_prefix_mean_bwd(int32_t dtype, const void* dout, const int32_t* lens, void* dx, int64_t n_seq, int32_t S,
                         int32_t d, void* stream);

/* ------------------------------------------------------------------------------------------
 * Two-stage configs with paths of 65..256 tokens (max_seq_len + 2 <= 256): the path-level stages (first encoder stage,
 * second decoder stage) with lengths in place of the 64-bit masks.
 *   build_masks_lens:   lens[b] = first-EOS index (= dsvg_seq_lens), seq_visible[b] = (number of EOS < S - 1), and the
 *                       per-icon group bitmask (G <= 64), as dsvg_build_masks (deepsvg/model/model.py:128-131,
 *                       deepsvg/model/utils.py:7-32)
 *   pack_tokens_lens:   the packed layout of dsvg_pack_tokens driven by lens, S <= 256 (layers/functional.py:234-239,
 *                       model/model.py:137)
 *   packed_mean:        out[b,:] = mean of the packed rows seq_off[b] .. seq_off[b+1]-1 (model/model.py:137); the
 *                       backward zero-fills rows [seq_off[n_seq], total_rows)
 *   attention_long_packed:  the dsvg_attention_long_* VALU kernels on the packed layout (non-causal; rows past
 *                       seq_off[n_seq] up to total_rows zero-filled), dropout rows (b H + h) S + i as in the padded layout
 *                       (layers/functional.py:168,197-248)
 *   attention_long_mfma:    bf16 matrix-core kernels of the same contract, padded (lens: keys j < lens[b], NULL = all)
 *                       or packed (seq_off, lens NULL), head_dim 32, non-causal; same dropout element ids
 * ------------------------------------------------------------------------------------------ */
int dsvg_build_masks_lens(const float* commands, int64_t n_seq, int32_t S, int32_t G, int32_t eos_id, int32_t* lens,
                          int32_t* seq_visible, uint64_t* group_mask, void* stream);
int dsvg_pack_tokens_lens(const float* commands, const float* args, const int32_t* lens, int64_t n_seq, int32_t S,
                          int32_t n_args, int32_t* seq_off, float* packed_commands, float* packed_args,
                          int32_t* packed_pos, void* stream);
int dsvg_packed_mean_fwd(int32_t dtype, const void* x, const int32_t* seq_off, void* out, int64_t n_seq, int32_t d,
                         void* stream);
int dsvg_packed_mean_bwd(int32_t dtype, const void* dout, const int32_t* seq_off, int64_t total_rows, void* dx,
                         int64_t n_seq, int32_t d, void* stream);
int dsvg_attention_long_packed_fwd(int32_t dtype, const void* qkv, const int32_t* seq_off, int64_t total_rows, void* out,
                                   int64_t n_seq, int32_t S, int32_t n_heads, float scale, float drop_p,
                                   uint32_t drop_site, const uint64_t* seed, void* stream);
int dsvg_attention_long_packed_bwd(int32_t dtype, const void* qkv, const int32_t* seq_off, int64_t total_rows,
                                   const void* dout, void* dqkv, int64_t n_seq, int32_t S, int32_t n_heads, float scale,
                                   float drop_p, uint32_t drop_site, const uint64_t* seed, void* stream);
int dsvg_attention_long_mfma_fwd(const void* qkv, const int32_t* lens, const int32_t* seq_off, int64_t total_rows,
                                 void* out, int64_t n_seq, int32_t S, int32_t n_heads, float scale, float drop_p,
                                 uint32_t drop_site, const uint64_t* seed, void* stream);
int dsvg_attention_long_mfma_bwd(const void* qkv, const int32_t* lens, const int32_t* seq_off, int64_t total_rows,
                                 const void* dout, void* dqkv, int64_t n_seq, int32_t S, int32_t n_heads, float scale,
                                 float drop_p, uint32_t drop_site, const uint64_t* seed, void* stream);

/* ------------------------------------------------------------------------------------------
 * Hungarian self-matching (HierarchicalSelfMatching, deepsvg/model/config.py:101-108):
 * SVGTransformer.perfect_matching, deepsvg/model/model.py:311-350.
 *  match_costs: cost[n, g, p] = w_args * mean_{masked (s,a)} CE(args_logits[n,p,s,a,:], tgt_args[n,g,s+1,a] + 1)
 *                             + w_cmd  * mean_{extended valid s} CE(command_logits[n,p,s,:], tgt_commands[n,g,s+1])
 *                             + w_vis  * CE(visibility_logits[n,p,:], visible[n,g])            (:329-339; 2, 1, 1)
 *    logits: rows (n*Gp + p)*S + s (S = S1 - 1) with row strides ld_* (elements); targets are the float32
 *    tgt_commands [N,G,S1] / tgt_args [N,G,S1,n_args] including their SOS column; the masks are taken on the
 *    sequence without it, as the reference does (:388, :314-315); visible[n,g] is returned for match_assign.
 *    Groups without argument slots get 0/0 like the reference; they are invisible and never assigned.
 *  match_assign: scipy.optimize.linear_sum_assignment(cost[n][visible rows]) (:344) as an exhaustive search
 *    (G, Gp <= 8): assign[n, j] = prediction matched to the j-th visible target, then the unmatched predictions in
 *    ascending order (:345-347); idx[n*Gp + j] = n*Gp + assign[n, j] and its inverse `inv` are the whole-sequence
 *    gather lists for dsvg_gather_groups (:390-393). */
int dsvg_match_costs(int32_t dtype, const void* cmd_logits, int64_t ld_c, const void* args_logits, int64_t ld_a,
                     const void* vis_logits, int64_t ld_v, const float* tgt_commands, const float* tgt_args,
                     const float* cmd_args_mask, int64_t N, int32_t G, int32_t Gp, int32_t S1, int32_t n_args,
                     int32_t args_dim, int32_t n_cmd, int32_t eos_id, float w_args, float w_cmd, float w_vis,
                     float* cost, int32_t* visible, void* stream);
int dsvg_match_assign(const float* cost, const int32_t* visible, int64_t N, int32_t G, int32_t Gp,
                      int32_t* assign, int32_t* idx, int32_t* inv, void* stream);

/* out[r] = argmax_c logits(r, c) for the logical rows r of a [rows, C] matrix stored like the masked-CE operand
 * (row r at logits + (r / group) * ld + (r % group) * C); ties -> lowest class.  The temperature -> 0 limit of
 * _sample_categorical (deepsvg/model/utils.py:75-80), used by greedy_sample(temperature=0). */
int dsvg_argmax_rows(int32_t dtype, const void* logits, int64_t ld, int32_t group, int64_t rows, int32_t C,
                     int32_t* out, void* stream);
/* out[r] = a draw from softmax(logits(r, :) / temperature), temperature > 0: _sample_categorical itself
 * (deepsvg/model/utils.py:75-79, torch.distributions.Categorical(logits = logits / T).sample()) as a Gumbel arg-max
 * arg-max_c (logit_c + T g_c) with the noise of the counter hash (seed: 8 bytes of device memory, site: stream id) - no
 * softmax, no cumulative sum, no fp32 copy of the logits.  Same addressing as dsvg_argmax_rows; the noise of logical row r,
 * class c is that of element (r / group, (r % group) * C + c), shared with dsvg_head_sample. */
int dsvg_sample_rows(int32_t dtype, const void* logits, int64_t ld, int32_t group, int64_t rows, int32_t C,
                     float temperature, const void* seed, uint32_t site, int32_t* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Reconstruction error of decoded icons (csrc/metrics.hip): the forward pair, then its backward (below).
 *  sample_points: SVGTensor.sample_points (deepsvg/difflib/tensor.py:191-230), batched.  commands [B*G, L] and args
 *    [B*G, L, 11], both contiguous and both of dtype `itype` (DSVG_F32 as the dataset delivers them, DSVG_I64 as
 *    greedy_sample returns them; read as they are).  The G sequences of cloud b are concatenated in group order.  Per
 *    sequence: the start point of row i is the end position (args 9:11) of row i - 1 whatever it holds (PAD -1 included),
 *    (0, 0) on row 0 (tensor.py:75-82); `l` (1) gives p0 + z (p3 - p0) and `c` (2) the cubic Bezier of start, control1
 *    (5:7), control2 (7:9), end (9:11) at z_k = k / (n - 1); every such command contributes z_0 .. z_{n-2}, the last one of
 *    the sequence z_{n-1} too (:226-228): k (n - 1) + 1 points for k drawing commands, and - where the reference raises -
 *    0 points for k = 0.  m, a, z, SOS, EOS give nothing (:198-217).  2 <= n <= 64, G * L <= 2048.
 *    points fp32 [B, cap, 2] with cap = G * (L * (n - 1) + 1) (< 2^31); counts int32 [B]; entries past counts[b] are
 *    not written.
 *  chamfer: chamfer_loss (deepsvg/difflib/loss.py:5-7) without the torch.cdist matrix, batched over clouds of different
 *    sizes: out[b] = mean_i min_j |x_i - y_j| + mean_j min_i |x_i - y_j| (Euclidean) over the first nx[b] points of
 *    px [B, capx, 2] and the first ny[b] of py [B, capy, 2]; NaN where either count is 0 (torch's mean of nothing).
 *    One workgroup per (icon, direction, slice of 1,024 points) writes its sum to `workspace`
 *    (dsvg_chamfer_workspace_bytes(B, capx, capy): 16 bytes per icon and slice of the larger cap, 8-byte aligned), a
 *    second launch adds the slices in ascending order.  No atomics: bit-reproducible, chamfer(x, y) == chamfer(y, x) bit
 *    for bit, chamfer(x, x) == 0. */
int dsvg_sample_points(int32_t itype, const void* commands, const void* args, int64_t B, int32_t G, int32_t L, int32_t n,
                       float* points, int32_t* counts, void* stream);
int64_t dsvg_chamfer_workspace_bytes(int64_t B, int64_t capx, int64_t capy);
int dsvg_chamfer(const float* px, const int32_t* nx, int64_t capx, const float* py, const int32_t* ny, int64_t capy,
                 int64_t B, float* out, void* workspace, int64_t workspace_bytes, void* stream);

/* The gradient of the two above, as the reference's autograd gives it for SVGTensor.sample_points (two matmuls,
 * deepsvg/difflib/tensor.py:220-228) and chamfer_loss (torch.cdist and two mins, deepsvg/difflib/loss.py:5-7), which
 * notebooks/svgtensor.ipynb optimises Bezier parameters through.  No distance matrix, no atomics: bit-reproducible.
 *  chamfer_nn: dsvg_chamfer (the same `out` bit for bit, the same workspace) that also writes the arg-min indices
 *    idx_x int32 [B, capx]: idx_x[b, i] = argmin_j |x_i - y_j| and idx_y int32 [B, capy]: idx_y[b, j] = argmin_i
 *    |x_i - y_j|, for the points in use; of equidistant candidates the lowest index wins.  Entries past the counts, and
 *    those of an icon with an empty cloud, are not written.
 *  chamfer_bwd (loss.py:5-7 differentiated): with j*(i) = idx_x, i*(j) = idx_y and u(a, b) = (a - b) / |a - b|, u = 0
 *    where a == b (so chamfer(x, x) has an exactly zero gradient, where the reference's matmul-form cdist backward is
 *    undefined),
 *      dpx[b, i] = dout[b] * ( u(x_i, y_j*(i)) / nx[b]  -  sum over {j : i*(j) = i} of u(y_j, x_i) / ny[b] )
 *    and dpy symmetrically (the same code on swapped pointers: d chamfer(x, y) / dx == the second gradient of
 *    chamfer(y, x) bit for bit).  One launch, one workgroup per (icon, direction, slice of 1,024 points); the terms of a
 *    point are added in ascending j.  dpx fp32 [B, capx, 2], dpy fp32 [B, capy, 2]: ALL rows are written, zeros past the
 *    counts; an icon with an empty cloud (forward NaN) gets zero rows whatever dout[b] holds.  Indices are clamped into
 *    their cloud.
 *  sample_points_bwd (tensor.py:191-230 differentiated; DSVG_F32 commands only - integer inputs have no gradient):
 *    dpoints fp32 [B, cap, 2] laid out as dsvg_sample_points writes `points` (entries past the counts are not read) ->
 *    dargs fp32 [B*G, L, 11], every element written.  A drawing command at row t with its samples z_k = k / (n - 1)
 *    receives, for `c`: sum 3 (1 - z)^2 z dP in 5:7, sum 3 (1 - z) z^2 dP in 7:9, sum z^3 dP in 9:11; for `l`: sum z dP in
 *    9:11.  Its start point's share (sum (1 - z)^3 dP for `c`, sum (1 - z) dP for `l`) goes to columns 9:11 of row t - 1
 *    WHATEVER that row holds (tensor.py:75-82: an m or SOS row gets a gradient there); row 0 starts at the constant (0, 0).
 *    Everything else is zero.  Sums in float64.  Same limits as the forward: 2 <= n <= 64, G * L <= 2048. */
int dsvg_chamfer_nn(const float* px, const int32_t* nx, int64_t capx, const float* py, const int32_t* ny, int64_t capy,
                    int64_t B, float* out, int32_t* idx_x, int32_t* idx_y, void* workspace, int64_t workspace_bytes,
                    void* stream);
int dsvg_chamfer_bwd(const float* px, const int32_t* nx, int64_t capx, const float* py, const int32_t* ny, int64_t capy,
                     int64_t B, const int32_t* idx_x, const int32_t* idx_y, const float* dout, float* dpx, float* dpy,
                     void* stream);
int dsvg_sample_points_bwd(const float* commands, int64_t B, int32_t G, int32_t L, int32_t n, const float* dpoints,
                           float* dargs, void* stream);

/* The ordered point loss svg_emd_loss (deepsvg/difflib/loss.py:21-51), the loss notebooks/svgtensor.ipynb minimises, and the
 * polyline length behind svg_length_loss (:15-18) and continuity_loss (:10-12); clouds laid out as for dsvg_chamfer.  x is
 * the pred cloud (n = nx[b] points), y the target (m = ny[b]); the target is a constant: gradients are for x only.
 *  emd: (1) orientation (make_clockwise, utils.py:52-60): A = sum_{j<m-1} (y_j.x y_{j+1}.y - y_{j+1}.x y_j.y), the open
 *    polyline, in float64; y is kept if A > 0 and read reversed otherwise (A == 0 and NaN reverse).  (2) arc-length
 *    distribution (get_length_distribution, utils.py:72-81) of the oriented cloud y': D_0 = 0, D_j = (sum_{i<j} |y'_{i+1} -
 *    y'_i|) / total, lengths and prefix sums in float64 (the reference's fp32 cumsum cannot resolve near matches); total ==
 *    0 or m == 1: every point matches index 0 of y' (the reference divides by zero).  (3) matching (loss.py:32-36): u_i =
 *    i / (n - 1) in float64 (u_0 = 0 when n == 1), match_i = argmin_j |u_i - D_j|, the lowest j of a tie; t_i = y'[match_i].
 *    A binary search per pred point on chunks of 1,024 D values: no [n, m] matrix and nothing of size m is stored, so
 *    capy is any size below 2^31.  (4) shift (loss.py:39-46): S(s) = sum_k |x_k - t_{(k+s) mod n}| for s = 0 .. n - 1, fp32
 *    terms (one sqrtf each) added in float64 in ascending k; s* = the lowest s that attains the minimum (np.argmin); with
 *    first_point_weight the term k = 0 of S(s*) counts 10 times - the weight does not influence s*, as in the reference.
 *    out[b] = S(s*) / n fp32; shift[b] = s* int32; matched int32 [B, capx]: matched[b, k] = the index into y AS PASSED (not
 *    into y') of the point paired with x_k, i.e. reorder(matching, s*) of return_matched_indices mapped back through the
 *    reversal, -1 in rows past nx[b]; t fp32 [B, capx, 2]: t_i as gathered in (3), before the shift, rows past nx[b] not
 *    written - what dsvg_emd_bwd needs.  n == 0: out 0 (loss.py:25-26); n > 0 and m == 0: out NaN (the reference raises);
 *    both with shift 0 and matched -1.  capx <= 65536 (the shift search is quadratic in n; one workgroup per icon and 256
 *    shifts).  workspace: dsvg_emd_workspace_bytes(B, capx) bytes, 8-byte aligned; it is dead once the call's work is done.
 *    No atomics, fixed summation orders: bit-reproducible.  On integer coordinates every S(s) is exact, so two shifts
 *    with the same terms tie exactly and the lower one is returned.
 *  emd_bwd: dpx[b, k] = dout[b] w_k (x_k - t_{(k+s*) mod n}) / (|x_k - t_{(k+s*) mod n}| n) with w_0 = 10 under
 *    first_point_weight and w_k = 1 otherwise; exactly 0 where the two points coincide.  dpx fp32 [B, capx, 2]: ALL rows
 *    written, zeros past nx[b] and in every row of an icon with an empty cloud, whatever dout[b] holds.  Element-wise.
 *  polyline_length: out[b] = sum_{i < n-1} |p_{i+1} - p_i| (get_length, utils.py:67-69) over the first n[b] points of p
 *    [B, cap, 2], float64 inside in a fixed order, fp32 out; 0 for 0 or 1 point.  polyline_length_bwd: dp[b, i] = dout[b]
 *    (u(p_i, p_{i-1}) - u(p_{i+1}, p_i)) with u(a, b) = (a - b) / |a - b|, 0 on a zero-length segment; all rows written,
 *    zeros past n[b].  Both bit-reproducible. */
int64_t dsvg_emd_workspace_bytes(int64_t B, int64_t capx);
int dsvg_emd(const float* px, const int32_t* nx, int64_t capx, const float* py, const int32_t* ny, int64_t capy, int64_t B,
             int32_t first_point_weight, float* out, int32_t* shift, int32_t* matched, float* t, void* workspace,
             int64_t workspace_bytes, void* stream);
int dsvg_emd_bwd(const float* px, const int32_t* nx, int64_t capx, const int32_t* ny, const float* t, const int32_t* shift,
                 const float* dout, int32_t first_point_weight, int64_t B, float* dpx, void* stream);
int dsvg_polyline_length(const float* p, const int32_t* n, int64_t cap, int64_t B, float* out, void* stream);
int dsvg_polyline_length_bwd(const float* p, const int32_t* n, int64_t cap, int64_t B, const float* dout, float* dp,
                             void* stream);

/* ------------------------------------------------------------------------------------------
 * Images of a decoded batch (csrc/raster.hip): anti-aliased coverage images of the curves dsvg_sample_points samples, as
 * outlines or filled.  Replaces SVG.draw -> cairosvg on the host, one icon at a time (deepsvg/svglib/svg.py:172-204; a
 * filled path is drawn without a stroke, deepsvg/svglib/svg_primitive.py:34-38); the curves are those of
 * SVGTensor.sample_points (deepsvg/difflib/tensor.py:191-230).  There is no rasteriser to match bit for bit; this is the
 * definition (tests/raster_ref.py restates it in float64):
 *  geometry: inputs as for dsvg_sample_points (itype, [B*G, L] commands, [B*G, L, 11] args, G * L <= 2048, 2 <= n <= 64):
 *    `l` and `c` draw, nothing else does (`a` included, tensor.py:213); the start point of row i is the end position (args
 *    9:11) of row i - 1 whatever it holds, (0, 0) on row 0.  A command becomes n - 1 chords between the vertices at z_k =
 *    k / (n - 1): vertex 0 IS the start point and vertex n - 1 IS the row's end position, bit for bit (consecutive commands
 *    share vertices exactly); between them `c` is the power-basis Horner form of dsvg_sample_points and `l` is
 *    ((n - 1 - k) p0 + k p3) / (n - 1).
 *  pixels: the image is size x size over the view box 0..256 (Bbox(256)); pitch s = 256 / size; the centre of pixel (row r,
 *    column c) is ((c + 0.5) s, (r + 0.5) s): x is the column, y the row, y down as in SVG.
 *  distance to a chord a -> b from p: t = clamp(((p - a) . (b - a)) / |b - a|^2, 0, 1) (t = 0 on a zero-length chord), q =
 *    p - (a + t (b - a)), d^2 = q . q; the minimum is taken over d^2, one sqrt per pixel.
 *  stroke (flags without DSVG_RASTER_FILL): d = the distance to the nearest chord of the image; ink = clamp(0.5 +
 *    (stroke_width / 2 - d) / s, 0, 1).  An image without chords is all zeros.
 *  fill (DSVG_RASTER_FILL): a sub-path is a maximal run of consecutive drawing rows of a sequence; each is closed by one
 *    extra chord from its last vertex to its first.  A pixel is inside a sequence when its winding number with respect to
 *    the sequence's chords is not 0 (non-zero, the SVG default), counted on a ray towards +x with the half-open rule: a
 *    chord with ay <= cy < by counts +1, one with by <= cy < ay counts -1, each when its crossing lies at x > cx; inside
 *    the image = inside any of its sequences.  d over all chords, closing chords included; ink = clamp(0.5 + d / s, 0, 1)
 *    inside and clamp(0.5 - d / s, 0, 1) outside.
 *  raster_segments: one workgroup per image writes its chord records in drawing order to `segs` (caller-owned,
 *    dsvg_raster_workspace_bytes(B, G, L, n, fill) bytes, 4-byte aligned: cap = G * (L * (n - 1) + (fill ? (L + 1) / 2 : 0))
 *    records per image) and their number to seg_counts int32 [B].  A record is 5 words: ax, ay, bx - ax, by - ay (fp32) and
 *    a flags word: bit 0 = the first chord of a sequence; bits 1.. = on a closing chord, the number of records back to its
 *    sub-path's first chord, 0 elsewhere.  Closing chords are written only with fill != 0, behind their sub-path.
 *    What raster_sweep relies on in fill mode, for records from any producer: every record that is not a closing chord is
 *    FOLLOWED by a record that starts at its end vertex (the next chord of its sub-path, or the closing chord), and a
 *    closing chord ends at the start vertex of the record `back` records before it.  The sweep takes a chord's end y from
 *    that record, not from ay + (by - ay), so that a vertex two chords share is ONE number and the half-open crossing rule
 *    is watertight.  Where the rule is broken (a non-closing chord in the last record in use, or `back` larger than the
 *    record's index) the sweep reads nothing out of bounds and falls back to ay + (by - ay) for that chord without a
 *    diagnosis: the winding count is then watertight only up to rounding.
 *  raster_sweep: segs / seg_counts as written above (cap records per image; counts are clamped into 0..cap) -> out fp32
 *    [B, size, size], 1 = ink.  One workgroup per (image, tile of 32 x 32 pixels); 1 <= size <= 4096.  `flags` must
 *    carry DSVG_RASTER_FILL exactly when the records were written with fill.  DSVG_RASTER_CULL: a wave skips the distance
 *    work of a chord farther from its pixels than the distance at which ink saturates (stroke_width / 2 + s / 2, or s / 2 in
 *    fill mode, plus a margin); the image is bit-identical with and without.  No atomics: bit-reproducible. */
#define DSVG_RASTER_FILL 1
#define DSVG_RASTER_CULL 2
int64_t dsvg_raster_workspace_bytes(int64_t n_images, int32_t G, int32_t L, int32_t n, int32_t fill);
int dsvg_raster_segments(int32_t itype, const void* commands, const void* args, int64_t B, int32_t G, int32_t L, int32_t n,
                         int32_t fill, void* segs, int64_t segs_bytes, int32_t* seg_counts, void* stream);
int dsvg_raster_sweep(const void* segs, const int32_t* seg_counts, int64_t B, int64_t cap, int32_t size, float stroke_width,
                      int32_t flags, float* out, void* stream);
/* The gradient of an image with respect to the arguments (ABI 17).  A pixel's ink depends on the chords only through d, the
 * distance to its nearest chord j* (a -> b, closest point at the clamped parameter t, q = p - (a + t (b - a)), d = |q|):
 * d d / d a = -(1 - t) q / d and d d / d b = -t q / d (interior t: q is normal to b - a; clamped t: t is constant); d ink / d d
 * = -1 / s in stroke mode and in fill mode outside, +1 / s in fill mode inside (ink > 0.5), 0 where ink is clamped.  The
 * winding number is piecewise constant and carries no gradient.  Conventions: of chords at equal fp32 d^2 the lowest record
 * index takes the term; a pixel with d == 0 contributes nothing (the peak of the ink in stroke mode; in fill mode the limit
 * needs an orientation the sweep does not carry); saturation (ink == 0 or ink == 1) is read from the stored image.
 *  raster_sweep_nn: dsvg_raster_sweep that also writes idx int32 [B, size, size]: the record index of the pixel's nearest
 *    chord where 0 < out < 1, -1 everywhere else (every pixel of an image without chords included).  `out` has the bits of
 *    dsvg_raster_sweep, and idx is the same with and without DSVG_RASTER_CULL (a chord culled for a wave is out of reach of
 *    every unsaturated pixel of that wave).
 *  raster_sweep_bwd: the records, out and idx of raster_sweep_nn (same size, stroke_width and DSVG_RASTER_FILL) and dout
 *    fp32 [B, size, size] -> dsegs fp32 [B, cap, 4] (16-byte aligned): the gradient with respect to the VERTICES (ax, ay, bx,
 *    by) of every record - with respect to b, not to the stored difference b - a.  Rows below seg_counts[b] are all written,
 *    rows past it are not.  A gather: a group of 16 lanes (DSVG_RASTER_WIDE: of 64) per record walks the record's bounding
 *    box dilated by the culling reach in a fixed order; no atomics, bit-reproducible.
 *  raster_segments_bwd: the transpose of raster_segments (linear in args, so the fp32 commands are all it needs): dsegs and
 *    seg_counts as above, built with the same G, L, n, fill -> dargs fp32 [B*G, L, 11], every element written.  Vertex 0 of a
 *    command is the end position (args 9:11) of the row before it whatever that row holds (the constant (0, 0) on row 0: no
 *    gradient), vertex n - 1 the row's own; interior vertices carry the Bernstein weights (`c`) or ((n - 1 - q), q) / (n - 1)
 *    (`l`); a closing chord's a is its last row's end position, its b the sub-path's start point.  Columns 0-4, padding and
 *    rows that neither draw nor precede a drawing row get exact zeros.  Limits as raster_segments. */
#define DSVG_RASTER_WIDE 4
int dsvg_raster_sweep_nn(const void* segs, const int32_t* seg_counts, int64_t B, int64_t cap, int32_t size, float stroke_width,
                         int32_t flags, float* out, int32_t* idx, void* stream);
int dsvg_raster_sweep_bwd(const void* segs, const int32_t* seg_counts, const float* out, const int32_t* idx, const float* dout,
                          int64_t B, int64_t cap, int32_t size, float stroke_width, int32_t flags, float* dsegs, void* stream);
int dsvg_raster_segments_bwd(const float* commands, const float* dsegs, const int32_t* seg_counts, int64_t B, int32_t G,
                             int32_t L, int32_t n, int32_t fill, float* dargs, void* stream);
/* Layered images: the G groups of an icon painted one over the other into ONE RGB image, each as an outline, filled, or as
 * an erase path (the per-group `filling` of the reference's data path, deepsvg/svglib/svg_path.py:29-32), with a colour and
 * an opacity per group - what SVG.draw / draw_colored show (svglib/svg.py:172-221).  Geometry, pixels, the distance to a
 * chord and the half-open crossing rule are those of the section above; tests/raster_layers_ref.py restates the rest in
 * float64.  These two entry points carry no gradient ("Layered images: the gradient" below does).  The definition:
 *  layers: group g of an image is layer g; layers are painted in group order onto a canvas of three channels that starts at
 *    `background`; 1 = paper white, 0 = black.  A layer without chords is skipped.  All arithmetic is fp32.
 *  mode of a layer (modes int32 [B, G]): DSVG_LAYER_FILL, DSVG_LAYER_ERASE, every other value DSVG_LAYER_OUTLINE.
 *  coverage of layer g, with d_g the distance to the nearest chord of group g alone:
 *    OUTLINE: cov = clamp(0.5 + (stroke_width / 2 - d_g) / s, 0, 1); no closing chords.
 *    FILL, ERASE: every sub-path of the group is closed by one chord; w = the winding number with respect to the group's own
 *      chords; inside = w != 0, or w odd with DSVG_RASTER_EVENODD; cov = clamp(0.5 + d_g / s, 0, 1) inside and clamp(0.5 -
 *      d_g / s, 0, 1) outside.
 *  paint (paint fp32 [B, G, 4]: r, g, b, opacity; the kernel clamps every value into 0..1 and reads a NaN as 0): alpha =
 *    opacity * cov; p = the layer's colour, or `background` for an ERASE layer; per channel canvas = fmaf(alpha, p - canvas,
 *    canvas).  Black on white at opacity 1 gives fmaf(cov, -1, 1), the correctly rounded 1 - cov: a one-group image is
 *    1 - dsvg_raster_sweep's, bit for bit.
 *  DSVG_RASTER_COMPOUND: all groups of an image are ONE layer, as a single <path> with many sub-paths is drawn: w counts the
 *    chords of all groups, d runs over all of them, the mode is FILL with DSVG_RASTER_FILL and OUTLINE without, the paint is
 *    group 0's.  With DSVG_RASTER_FILL | DSVG_RASTER_EVENODD a sub-path inside another one is a hole.
 *  raster_segments_layers: dsvg_raster_segments with `fill` per group: closing chords behind the sub-paths of FILL and ERASE
 *    groups only.  Same record format; `segs` holds dsvg_raster_workspace_bytes(B, G, L, n, 1) bytes.  Also writes layer_first
 *    int32 [B, G + 1]: the record offset of each group's first chord, seg_counts[b] last; a group without chords has the
 *    entry of the group after it.  With modes all OUTLINE the records are those of dsvg_raster_segments(fill = 0), with all
 *    FILL those of fill = 1, bit for bit.
 *  raster_sweep_layers: segs / seg_counts / layer_first / modes as above and paint -> out fp32 [B, 3, size, size].  `cap` is the
 *    record capacity per image, G the number of groups (1..2048), `background` three HOST floats in 0..1.  flags:
 *    DSVG_RASTER_CULL (same bits with and without: an OUTLINE layer skips chords out of reach, FILL and ERASE layers skip
 *    their distance work only), DSVG_RASTER_EVENODD, DSVG_RASTER_COMPOUND (records from dsvg_raster_segments with the same
 *    fill; layer_first and modes are not read and may be null), DSVG_RASTER_FILL (with COMPOUND only).  The layer table of an
 *    image sits in LDS (20 bytes per group).  layer_first from any producer is clamped into 0..seg_counts[b]; layer g takes
 *    the records from the end of the layer before it to layer_first[g + 1] (the last one to the count), so no table leads out
 *    of bounds.  No atomics: bit-reproducible. */
#define DSVG_LAYER_OUTLINE 0
#define DSVG_LAYER_FILL 1
#define DSVG_LAYER_ERASE 2
#define DSVG_RASTER_EVENODD 8
#define DSVG_RASTER_COMPOUND 16
int dsvg_raster_segments_layers(int32_t itype, const void* commands, const void* args, int64_t B, int32_t G, int32_t L,
                                int32_t n, const int32_t* modes, void* segs, int64_t segs_bytes, int32_t* seg_counts,
                                int32_t* layer_first, void* stream);
int dsvg_raster_sweep_layers(const void* segs, const int32_t* seg_counts, const int32_t* layer_first, const int32_t* modes,
                             const float* paint, const float* background, int64_t B, int64_t cap, int32_t G, int32_t size,
                             float stroke_width, int32_t flags, float* out, void* stream);
/* Layered images: the gradient (still ABI 19: additions only; tests/raster_layers_grad_ref.py restates it in float64).
 * Per pixel, with the layers that have chords g = 1..K in group order: C_0 = background, alpha_g = opacity_g * cov_g, C_g =
 * fmaf(alpha_g, p_g - C_{g-1}, C_{g-1}) per channel, out = C_K; p_g is the layer's colour, or the background for an ERASE
 * layer.  With T_g = prod_{k > g} (1 - alpha_k) (a running product from the top layer down: nothing is ever divided by
 * 1 - alpha, which is 0 inside every opaque fill):
 *    d out_c / d alpha_g = T_g (p_g,c - C_{g-1,c}),   d out_c / d p_g,c = T_g alpha_g (an exact 0 for ERASE and skipped layers),
 *    d alpha_g / d cov_g = opacity_g,   d alpha_g / d opacity_g = cov_g.
 *  Colours and opacities are clamped by the kernel: the gradient passes where the given value lies in 0..1 and is an exact 0
 *  where it was clamped or is a NaN.  d cov / d d = -1 / s for OUTLINE, and for FILL and ERASE where cov <= 0.5, +1 / s for FILL
 *  and ERASE where cov > 0.5, 0 where the stored cov is 0 or 1.  d d / d a and d d / d b are those of dsvg_raster_sweep_bwd with
 *  the nearest chord taken among the layer's OWN chords (ties to the lowest record index, d == 0 contributes nothing).  The
 *  winding number carries no gradient under either fill rule.
 *  raster_sweep_layers_nn: dsvg_raster_sweep_layers (same arguments, `out` with the same bits, with and without
 *    DSVG_RASTER_CULL) that also writes cov fp32 [B, NL, size, size], the clamped coverage of every layer (0 for a layer without
 *    chords), and idx int32 [B, NL, size, size]: the image-wide record index of the layer's nearest chord where 0 < cov < 1, -1
 *    elsewhere; both are the same with and without DSVG_RASTER_CULL.  NL = G, or 1 with DSVG_RASTER_COMPOUND.
 *  raster_blend_bwd: cov as above, the tables, paint and background of the forward (same DSVG_RASTER_COMPOUND / _FILL) and dout
 *    fp32 [B, 3, size, size] -> dcov fp32 [B, NL, size, size] = dL / d cov, every element written (0 for a layer without
 *    chords), and dpaint fp32 [B, G, 4] (16-byte aligned) = dL / d (r, g, b, opacity) summed over the pixels of the image, every
 *    element written.  One workgroup per image; the pixel sums run in a fixed order without atomics: bit-reproducible.
 *  raster_sweep_layers_bwd: the records and tables, cov and idx of raster_sweep_layers_nn and dcov -> dsegs fp32 [B, cap, 4] as
 *    dsvg_raster_sweep_bwd writes it (rows below seg_counts[b] all written; DSVG_RASTER_WIDE as there).  The layer of a record
 *    is found from layer_first with the forward's clamping; its mode decides the sign rule and the reach.
 *  raster_segments_layers_bwd: dsvg_raster_segments_bwd with `fill` per group from modes: the transpose of
 *    dsvg_raster_segments_layers for fp32 inputs -> dargs fp32 [B*G, L, 11], every element written.  A compound image has the
 *    records of dsvg_raster_segments: its dsegs go to dsvg_raster_segments_bwd. */
int dsvg_raster_sweep_layers_nn(const void* segs, const int32_t* seg_counts, const int32_t* layer_first, const int32_t* modes,
                                const float* paint, const float* background, int64_t B, int64_t cap, int32_t G, int32_t size,
                                float stroke_width, int32_t flags, float* out, float* cov, int32_t* idx, void* stream);
int dsvg_raster_blend_bwd(const float* cov, const int32_t* seg_counts, const int32_t* layer_first, const int32_t* modes,
                          const float* paint, const float* background, const float* dout, int64_t B, int64_t cap, int32_t G,
                          int32_t size, int32_t flags, float* dcov, float* dpaint, void* stream);
int dsvg_raster_sweep_layers_bwd(const void* segs, const int32_t* seg_counts, const int32_t* layer_first, const int32_t* modes,
                                 const float* cov, const int32_t* idx, const float* dcov, int64_t B, int64_t cap, int32_t G,
                                 int32_t size, float stroke_width, int32_t flags, float* dsegs, void* stream);
int dsvg_raster_segments_layers_bwd(const float* commands, const float* dsegs, const int32_t* seg_counts, const int32_t* modes,
                                    int64_t B, int32_t G, int32_t L, int32_t n, float* dargs, void* stream);

/* ------------------------------------------------------------------------------------------
 * Canonical path order of a batch (csrc/paths.hip): SVG.canonicalize() (deepsvg/svglib/svg.py:333-349) applied to
 * SVG.from_tensors([group tensors]) and read back through to_tensor(concat_groups=False) (svg.py:141-166), optionally followed
 * by Point.numericalize (svglib/geom.py:182-183) - the form the encoder was trained on.  Replaces the host loop over icons of
 * the reference's preprocessing and of notebooks/animation.ipynb's permute / reverse by hand.  Every output value is a copy
 * of an input value; only the decisions are computed.  The definition (tests/paths_ref.py restates it in float64; arcs are out
 * of scope):
 *  rows: commands [N, G, S] / args [N, G, S, 11] of dtype `itype` (DSVG_F32 or DSVG_I64; the decisions read DSVG_I64
 *    coordinates as fp32, exact below 2^24, the values written are the int64 inputs), G * S <= 2048.  A group ends at its
 *    first EOS; the start point of a row is the end position (args 9:11) of the row before it; rows before the group's first
 *    `m` are ignored; an `m` opens a sub-path and ends the one before it; a `z` marks the open sub-path closed and ends it, and
 *    rows after it are ignored until the next `m`.  Every sub-path becomes a group of its own, in reading order
 *    (svglib/svg_path.py:118-157, split_paths).
 *  degenerate commands (filter_consecutives, svg_path.py:214-220): an `l` / `c` with |s - e| <= 1e-8 + 1e-5 |e| in both
 *    coordinates (float64) is dropped; a sub-path left without commands disappears.
 *  rotation (reorder, svg_path.py:295-315), closed sub-paths only: a running best over the commands in order; command i with
 *    start p replaces the best with start q when p.y == q.y ? p.x < q.x : (p.y < q.y || (the norms of p and q are close &&
 *    p.x < q.x)) (svg_command.py:170-176).  The norm is the fp32 sqrt(x * x + y * y) (products, sum and square root each rounded
 *    to fp32), the difference of the two norms is taken in fp32 and compared with 1e-8 + 1e-5 |norm q| in float64.  The
 *    commands are rotated to start at the best.  No closing line is inserted: a closed sub-path whose last end is not its
 *    first start loses the gap, as in the reference.
 *  order (svg.py:343): sub-paths are sorted by (start.y, start.x) of their first command, stable in reading order - BEFORE
 *    the orientation step, so the result is generally not sorted by its final start points.
 *  orientation (svg_path.py:244-273): a sub-path of one command is clockwise when (s.x, s.y) <= (e.x, e.y) lexicographically,
 *    any other when the float64 sum of s.x e.y - s.y e.x over its commands, in their order, is >= 0.  One that is not is
 *    reversed: commands in reverse order, start and end swapped, the control points of a `c` swapped.
 *  rows out: `m` with the first command's start, `l` with its end, `c` with control1, control2, end; never a `z`.
 *  numericalize = n > 0: every enabled slot of the written rows becomes clip(round-half-even(v), 0, n - 1) (DSVG_I64: clip),
 *    after all decisions.
 *  layout DSVG_PATHS_GROUPED: out_commands [N, G_out, S_out] / out_args [N, G_out, S_out, 11] of dtype `itype`; a group in use
 *    is SOS, m, ..., EOS...; an unused one SOS, EOS...; every slot CMD_ARGS_MASK does not enable is -1.
 *  layout DSVG_PATHS_CONCAT: out_commands [N, S_out] / out_args [N, S_out, 11]: SOS, all groups' rows back to back, EOS....
 *  n_groups int32 [N]; len_groups int32 [N, G_out]: rows of each output group, its `m` included, 0 where unused; source_group
 *    int32 [N, G_out]: the input group, -1 where unused; reversed uint8 [N, G_out]; valid uint8 [N]: 0 when the icon has more
 *    sub-paths than G_out, when a sub-path (concat: all of them together) has more than S_out - 2 rows, or when an `a` stands
 *    before its group's first EOS; such an icon is written as all-unused groups with n_groups = 0.
 *  One workgroup per icon: ballot prefix scans classify the rows, one lane per sub-path walks its commands for the rotation and
 *    the determinant sum, a stable rank sort orders the sub-paths, and every output row gathers the input rows it copies.  No
 *    atomics, no workspace, no device-to-host read: bit-reproducible, capturable. */
#define DSVG_PATHS_GROUPED 0
#define DSVG_PATHS_CONCAT 1
int dsvg_canonicalize(int32_t itype, const void* commands, const void* args, int64_t N, int32_t G, int32_t S, int32_t G_out,
                      int32_t S_out, int32_t layout, int32_t numericalize, void* out_commands, void* out_args,
                      int32_t* n_groups, int32_t* len_groups, int32_t* source_group, uint8_t* reversed, uint8_t* valid,
                      void* stream);

/* ------------------------------------------------------------------------------------------
 * Filling of a decoded batch (csrc/paths_fill.hip): which groups of an icon are filled, which are holes (erase
 * paths), and in what order to paint them - SVGPathGroup.compute_filling over overlap_graph (deepsvg/svglib/svg_primitive.py:
 * 392-441), which SVG.canonicalize_new calls on all sub-paths of an icon (svg.py:312-331).  The reference measures overlap
 * with shapely polygons; the measure here is this package's own, on the rasteriser's chord records and crossing rule.  The
 * result feeds the `modes` table of the layered rasteriser as it is.  tests/paths_fill_ref.py restates the definition in
 * float64.  Arcs are out of scope, as everywhere in the rasteriser; SVG.group_overlapping_paths (the regrouping into groups
 * of several sub-paths) is not provided: `parent` and `depth` are what it needs.
 *  overlap_counts: segs / seg_counts / layer_first of dsvg_raster_segments_layers with every group's mode DSVG_LAYER_FILL (every
 *    sub-path has its closing chord), cap records per icon, 1 <= G <= 32 groups, 8 <= samples = K <= 1024.  The samples are the
 *    K x K pixel centres of an image of size K: ((col + 0.5) s, (row + 0.5) s), s = 256 / K, the fp32 expressions of
 *    raster_sweep.  A sample is inside group i when its winding number with respect to the chords of group i alone (the
 *    half-open rule of "Images of a decoded batch", end y taken from the next record as raster_sweep takes it; the sign test
 *    is the sweeps' e = fmaf(dx, py, -p), p = fl(dy px), with the rounding residual of p taken out: e - fmaf(dy, px, -p), so
 *    that a sample ON a chord, whose crossing lies at x == cx, counts nothing - in the sweeps the residual decides there,
 *    unseen in an image, where the coverage is 0.5 on both sides) is not 0, or is odd when `evenodd` is set.  The counts may
 *    therefore differ from the pixels a sweep calls inside by pixels whose centre is on a chord, and lie between the pixels
 *    with ink > 0.5 and those with ink >= 0.5 of dsvg_raster_sweep.  area[b, i] int32 [B, G] += the samples inside
 *    group i, inter[b, i, j] int32 [B, G, G] += the samples inside both i and j: symmetric, its diagonal is area.  Both tables
 *    are ADDED to with integer atomics and must be zero on entry; integer sums do not depend on their order: bit-
 *    reproducible.  layer_first from any producer is clamped into 0..seg_counts[b] and made non-decreasing; a group without
 *    records counts nothing.  One workgroup per (icon, tile of 32 x 32 samples), no distance work.
 *  filling_from_counts: area / inter as above, commands [N, G, S] / args [N, G, S, 11] of dtype `itype` (DSVG_F32 or DSVG_I64,
 *    read as fp32 as dsvg_canonicalize reads them), G * S <= 2048, participating uint8 [N, G], 0 < threshold <= 1, rule.
 *    1. participation: group i participates when participating[b, i] != 0 and area[b, i] > 0.  Every other group gets filling
 *       0 (DSVG_LAYER_OUTLINE), depth -1, parent -1 and has no edges.
 *    2. edges: j -> i ("j covers i") when i != j, both participate and (double)inter[i][j] > threshold * (double)area[i].
 *    3. orientation: clockwise[b, i] is SVGPath.is_clockwise (svg_path.py:244-252) over the drawing rows (`l`, `c`) of the
 *       group as the rasteriser reads them (the start point of a row is the end position of the row before it, (0, 0) on row
 *       0), by the orientation step of dsvg_canonicalize: one command: (s.x, s.y) <= (e.x, e.y) lexicographically; any other
 *       number: the float64 sum of s.x e.y - s.y e.x, in row order, is >= 0 (so true without commands).  Closing chords are
 *       not part of it, as in the reference.
 *    4. traversal (svg_primitive.py:396-418): the roots are the participating groups without an in-edge at the start, taken in
 *       ascending index, each with its own walk that starts at current = [(d = 1, root)], level 0.  Per level, for (d, n) in
 *       current in ASCENDING n: filling[n] = d != 0 ? DSVG_LAYER_FILL : DSVG_LAYER_ERASE, depth[n] = the level, parent[n] = the
 *       group that visited n in the level before (-1 for a root); then every out-neighbour n2 of n that has not been
 *       removed and has not been visited in this level, in ascending order, is visited by n with d2 = d + (clockwise[n2] ==
 *       clockwise[n] ? 1 : -1) (DSVG_FILLING_ORIENTATION, the reference's rule) or d2 = 1 - d (DSVG_FILLING_EVENODD).  Then
 *       current is removed from the graph, and the next current is the visited groups that are left without an in-edge.  A
 *       group that is never reached (two groups that cover each other, for instance) keeps filling 0.  The reference
 *       iterates Python sets, so the order inside a level is the one place where this can differ from it: when two groups of
 *       one level reach the same group with different d2.
 *    5. paint order: paint_order[b, :] int64 is the groups sorted stably by (filling 0 last, depth, index): an ERASE never
 *       precedes the FILL it cuts.
 *    filling int64 [N, G], depth / parent int32 [N, G], clockwise uint8 [N, G], paint_order int64 [N, G]: every element is
 *    written.  One lane per icon; no atomics, nothing is read back. */
#define DSVG_FILLING_EVENODD 0
#define DSVG_FILLING_ORIENTATION 1
int dsvg_overlap_counts(const void* segs, const int32_t* seg_counts, const int32_t* layer_first, int64_t B, int64_t cap,
                        int32_t G, int32_t samples, int32_t evenodd, int32_t* area, int32_t* inter, void* stream);
int dsvg_filling_from_counts(int32_t itype, const int32_t* area, const int32_t* inter, const void* commands, const void* args,
                             const uint8_t* participating, int64_t N, int32_t G, int32_t S, double threshold, int32_t rule,
                             int64_t* filling, int32_t* depth, int32_t* parent, uint8_t* clockwise, int64_t* paint_order,
                             void* stream);

/* ------------------------------------------------------------------------------------------
 * Commands split and arcs converted, for a whole batch (csrc/paths_expand.hip): SVGPath.split (deepsvg/svglib/svg_path.py:
 * 615-630 with SVGCommandLine.split / SVGCommandBezier.split / .length, svg_command.py:255-270, 369-413) and
 * SVGPath.simplify_arcs (svg_path.py:280-293 with SVGCommandArc.to_beziers, svg_command.py:458-511) on the tensors themselves.
 * Every input row becomes 0..k output rows: a count per row, a prefix sum, a gather.  The definition
 * (tests/paths_expand_ref.py restates it in float64):
 *  rows: commands [N, G, S] / args [N, G, S, 11] fp32, G * S <= 2048.  Row 0 of a group is its frame (SOS) and is never read
 *    as a command; a group ends at its first EOS (a group whose row 0 is EOS is empty), rows at or behind it are dead and
 *    never read.  The start point of a row is the end position (args 9:11) of the row before it, whatever that row holds.  A
 *    live row that is not expanded (`m`, `z`, a SOS behind row 0, an `l` when include_lines = 0, every `l` / `c` in arc mode)
 *    passes through as one row.  A command outside 0..6 on a live row makes the icon invalid.
 *  arithmetic: float64, one IEEE operation at a time (no fused multiply-add), each written value rounded to fp32 once.  With
 *    lerp(a, b, t) = (1 - t) a + t b.  The last piece of an expanded row carries the input row's end position bit for bit;
 *    as the layout stores no start points, consecutive pieces join exactly.
 *  mode DSVG_EXPAND_SPLIT: the length of an `l` is sqrt(dx dx + dy dy) from its start to its end; of a `c` the sum, i = 1..99
 *    in order, of the distances between the points at z = (i - 1) / 99 and i / 99, a point being ((b0 p0 + b1 p1) + b2 p2) +
 *    b3 p3 with w = 1 - z, b0 = (w w) w, b1 = (3 (w w)) z, b2 = (3 w) (z z), b3 = (z z) z (the Bernstein form in float64: not
 *    the fp32 power basis of csrc/svg_seq.h, which is what sample_points draws).  k = n when n > 0, else max(ceil(length /
 *    max_dist), 1).  An `l` becomes k `l` rows with ends lerp(p0, p1, (i + 1) / k); a `c` becomes k `c` rows, row i holding
 *    the sub-curve on [a, b] = [i / k, (i + 1) / k] by its blossom: control1 = B(a, a, b), control2 = B(a, b, b), end =
 *    B(b, b, b), where B(u, v, w) runs de Casteljau's three lerp levels with u, then v, then w.  A row with k = 1 is copied.
 *    A live `a` makes the icon invalid (the reference raises).  lengths fp32 [N, G, S]: the length of every live `l` / `c`,
 *    0 elsewhere.
 *  mode DSVG_EXPAND_ARCS: a live `a` holds rx, ry (read as absolute values), phi in degrees, fA, fS (read as != 0) and its end.
 *    It is dropped when both radii are 0 or when start and end are close (|s - e| <= 1e-8 + 1e-5 |e| in both coordinates);
 *    with exactly one radius 0 it becomes one `l` to its end (SVG implementation note F.6.2; the reference divides by zero).
 *    Otherwise, formula by formula as SVGCommandArc._get_center_parametrization: h = (p1 - p2) / 2, m = (p1 + p2) / 2, (x', y')
 *    = h rotated by -phi, lambda = x'^2 / rx^2 + y'^2 / ry^2; when lambda > 1 both radii are multiplied by sqrt(lambda) and
 *    the centre coefficient is 0 (note F.6.6; the reference keeps the radii, and its sweep then rests on the sign of a
 *    rounded zero), else coefficient = sqrt(max((rx^2 ry^2 - rx^2 y'^2 - ry^2 x'^2) / (rx^2 y'^2 + ry^2 x'^2), 0)), negated
 *    when fA == fS; c' = coefficient (rx y' / ry, -ry x' / rx), centre = c' rotated by phi + m, d = (p' - c') / r, e = -(p' +
 *    c') / r, theta1 = the signed angle from (1, 0) to d, sweep = the signed angle from d to e in degrees (acos of the clipped
 *    dot product of the normalised vectors, negative when the determinant is < 0), plus 360 when negative, minus 360 when fS
 *    = 0 and it is > 0; when lambda > 1 the chord is a diameter and the sweep is 180 (fS) or -180.  The row becomes k = max(floor(|sweep| / 45), 1) `c` rows over equal parts of the sweep, eta_i =
 *    theta1 + (1 / k) (i sweep) in degrees; with t1, t2 the radians of a part, alpha = sin(t2 - t1) (sqrt(4 + 3 tan^2((t2 -
 *    t1) / 2)) - 1) / 3, P(t) = centre + (rx cos t, ry sin t) rotated by phi, P'(t) = (-rx sin t, ry cos t) rotated by phi:
 *    control1 = P(t1) + alpha P'(t1), control2 = P(t2) - alpha P'(t2), end = P(t2).
 *  validity: a live `l`, `c` or `a` whose start point, arguments in use, or computed length / sweep is not finite makes the
 *    icon invalid (no NaN is converted to a count; counts are clamped to S_out before the sum), and so does a group that
 *    needs more than S_out - 2 rows.  An invalid icon is written as SOS, EOS... in every group, len_groups 0, source_row -1.
 *  out_commands [N, G, S_out] / out_args [N, G, S_out, 11] fp32, G * S_out <= 2048: SOS, the rows, EOS to the end; every slot
 *    CMD_ARGS_MASK does not enable for the row's command is -1.  len_groups int32 [N, G]: rows between SOS and the first EOS.
 *    source_row int32 [N, G, S_out]: the input row (index in its group) an output row came from, -1 on SOS, EOS, padding.
 *    lengths: NULL in arc mode.  valid uint8 [N].
 *  One workgroup per icon: a ballot scan for the EOS rule, one lane per live row for its count, a prefix sum over the counts
 *    (each group's base subtracted), and every output row finds its input row by binary search in the prefix and computes its
 *    own piece.  No atomics, no workspace, no device-to-host read: bit-reproducible, capturable. */
#define DSVG_EXPAND_SPLIT 0
#define DSVG_EXPAND_ARCS 1
int dsvg_paths_expand(int32_t mode, const float* commands, const float* args, int64_t N, int32_t G, int32_t S, int32_t S_out,
                      int32_t n, double max_dist, int32_t include_lines, float* out_commands, float* out_args,
                      int32_t* len_groups, int32_t* source_row, float* lengths, uint8_t* valid, void* stream);

/* ------------------------------------------------------------------------------------------
 * Beziers fitted through the points of every sub-path, for a whole batch (csrc/paths_simplify.hip): SVGPath.simplify
 * (deepsvg/svglib/svg_path.py:391-613), the middle step of simplify_heuristic, on the tensors themselves.  The definition
 * (tests/paths_simplify_ref.py restates it in float64):
 *  1. rows and sub-paths: commands [N, G, S] / args [N, G, S, 11] fp32, G * S <= 2048, read by the EOS rule of
 *     dsvg_paths_expand (row 0 is the frame, a group ends at its first EOS).  A sub-path ("run") is a maximal run of live `l`
 *     / `c` rows; `m`, `z` and a SOS behind row 0 pass through in place and delimit runs.  The points of a run are the start
 *     of its first row (the end position of the row before it, whatever that row holds) and the end of every row.  Point k of
 *     an icon is the end position of its row k, read as fp32 and divided by `unit` in float64 at every use: the fit runs in
 *     the reference's units (its 24 box), because max(error, error^2) and the comparison of a squared distance with
 *     `tolerance` are not scale-invariant.
 *  2. segments (subdivide_indices): an `l` closes the open segment.  Between consecutive `c` rows, t1 = 3 (end - control2)
 *     of the first and t2 = -(3 (control1 - start)) of the second (every coordinate divided by unit first); the segment breaks
 *     when either norm is <= 1e-8 or when clip((t1x / |t1|) (t2x / |t2|) + (t1y / |t1|) (t2y / |t2|), -1, 1) > cos_threshold
 *     = cos(angle_threshold), computed by the caller in float64: no acos runs on the device.
 *  3. emission order (svg_path.py:593-609): RDP on the gap of `l` rows before the first segment, then per segment fitCubic
 *     followed by RDP on the gap behind it; a run without a `c` is one RDP.  An empty gap (first == last) emits a zero-length
 *     `l` as the reference does, so a group can grow: at most rows in + segments + 1 rows.  force_smooth: one fitCubic over
 *     the whole run, `l` rows included.
 *  4. formulas, float64, one IEEE operation at a time (no fused multiply-add), powers as products, |v| = sqrt(dx dx + dy dy):
 *     RDP(first, last): dist_i of the interior points i to the line: when the two ends are close (|a - b| <= 1e-8 + 1e-5 |b|
 *       in both coordinates) |P_i - P_first|, else |dx (ay - py) - dy (ax - px)| / |(dx, dy)| with (dx, dy) = P_last -
 *       P_first.  The largest, the largest index among equals (a NaN never counts); when it is > epsilon split there, left
 *       part first, else one `l` to P_last.
 *     fitCubic(first, last) with tangents t1, t2 (point 6): one interval: control1 = P_first + d t1, control2 = P_last + d t2,
 *       d = |P_first - P_last| / 3.  Else u_i = (L[first + i] - L[first]) / (L[last] - L[first]) (point 5a), limit =
 *       max(tolerance, tolerance^2), ordered = true, and at most 5 times: curve = generateBezier; (err, split) =
 *       computeMaxError; accept the curve when err < tolerance and ordered; stop when err >= limit; ordered = reparametrize;
 *       limit = err.  Not accepted: split at `split`, left part first.
 *     generateBezier: per point t = 1 - u, b = (3 u) t, b0 = (t t) t, b1 = b t, b2 = b u, b3 = (u u) u, a1 = t1 b1, a2 = t2 b2,
 *       tmp = (P_i - P_first (b0 + b1)) - P_last (b2 + b3); C00 = sum a1.a1, C01 = sum a1.a2, C11 = sum a2.a2, X0 = sum
 *       a1.tmp, X1 = sum a2.tmp (point 5b; a.b = ax bx + ay by).  det = C00 C11 - C01 C01; when |det| > 1e-12: alpha1 = (X0 C11
 *       - X1 C01) / det, alpha2 = (C00 X1 - C01 X0) / det; else with c0 = C00 + C01, c1 = C01 + C11 both are X0 / c0 when |c0|
 *       > 1e-12, else X1 / c1 when |c1| > 1e-12, else 0.  seg = |P_last - P_first|; when alpha1 or alpha2 < 1e-12 seg both
 *       become seg / 3; else when (t1 alpha1).line - (t2 alpha2).line > seg seg, line = P_last - P_first, too.  control1 =
 *       P_first + t1 alpha1, control2 = P_last + t2 alpha2.
 *     the curve at t: ((b0 p0 + b1 c1) + b2 c2) + b3 p3 with w = 1 - t, b0 = (w w) w, b1 = (3 (w w)) t, b2 = (3 w) (t t), b3 =
 *       (t t) t; its derivatives ((3 (w w)) (c1 - p0) + ((6 w) t) (c2 - c1)) + (3 (t t)) (p3 - c2) and (6 w) ((c2 - 2 c1) + p0)
 *       + (6 t) ((p3 - 2 c2) + c1).
 *     computeMaxError: over the interior points d = |curve(u_i) - P_i|, err_i = d d; the largest, the largest index among
 *       equals.  The accept test compares this SQUARED distance with tolerance, as the reference does.
 *     reparametrize: for every point, the ends included, f = curve(u) - P, num = f.curve'(u), den = curve'(u).curve'(u) +
 *       f.curve''(u); u stays when -1.12e-16 <= den <= 1.12e-16, else u - num / den.  ordered = no u_i <= u_(i-1).
 *  5. stated summation order: (a) chord lengths are accumulated once per run in ascending order into the table L, L = 0 at
 *     the run's first point; (b) each of the five sums is 64 strided partials - partial j adds the terms of i = j, j + 64,
 *     ... in ascending order, starting from 0.0 - combined by partial[j] += partial[j + d] for j < d, d = 32, 16, ..., 1.
 *  6. tangents are never stored: at the first point of a job (a top-level fitCubic) t1 = normalize(P[first + 1] - P[first]),
 *     at its last point t2 = normalize(P[last - 1] - P[last]); at a split index s the left part ends with c = normalize(P[s -
 *     1] - P[s + 1]) and the right part starts with -c.  normalize(v) = (vx / |v|, vy / |v|).
 *  validity: the cases of dsvg_paths_expand in split mode (a live `a`, a command outside 0..6, a live `l` / `c` whose start
 *     point or arguments in use are not finite), a group that needs more than S_out - 2 rows, a direction between two points
 *     at distance exactly 0 (the reference raises ZeroDivisionError in normalize), L[last] == L[first] in a fit, and a fit
 *     whose distances are all NaN.  An invalid icon is written as SOS, EOS... in every group, len_groups 0, source_row -1.
 *  out_commands [N, G, S_out] / out_args [N, G, S_out, 11] fp32, G * S_out <= 2048: SOS, the rows, EOS to the end; -1 in every
 *     slot CMD_ARGS_MASK does not enable.  Control points are multiplied by unit once, then rounded to fp32 once; end
 *     positions are copies of input values.  len_groups int32 [N, G].  source_row int32 [N, G, S_out]: for `m` / `z` the
 *     input row itself, for a written `l` / `c` the input row whose end position it carries bit for bit, -1 on SOS, EOS and
 *     padding.  valid uint8 [N].
 *  workspace: dsvg_paths_simplify_workspace_bytes(N, G, S) = 20 bytes per slot, 2 G S slots per icon, 16-byte aligned: the
 *     rows a job emitted until they are compacted.  tolerance, epsilon, unit finite and > 0; cos_threshold in [-1, 1].
 *  One workgroup per icon; csrc/paths_simplify.hip has the phases.  No atomics, no device-to-host read: bit-reproducible. */
int64_t dsvg_paths_simplify_workspace_bytes(int64_t N, int32_t G, int32_t S);
int dsvg_paths_simplify(const float* commands, const float* args, int64_t N, int32_t G, int32_t S, int32_t S_out,
                        double tolerance, double epsilon, double cos_threshold, int32_t force_smooth, double unit,
                        void* workspace, int64_t workspace_bytes, float* out_commands, float* out_args, int32_t* len_groups,
                        int32_t* source_row, uint8_t* valid, void* stream);

/* ------------------------------------------------------------------------------------------
 * The argument head fused with its consumers (csrc/head_fused.hip): args_fcn = Linear(256 -> n_args *
 * args_dim) of deepsvg/model/model.py:228-246 evaluated tile by tile on chip - the [tokens, group * C] logits never reach
 * memory.  bf16 x [rows, 256]; `packed` = dsvg_head_pack of the head's weight rows in use ([n_out, 256] bf16, row-major,
 * n_out = group * C with slots of C >= 64 consecutive outputs, n_out <= 3008); bias fp32 [n_out].
 *   dsvg_head_argmax   out_idx[row * group + slot] = argmax_c logits(row, slot, c), ties -> lowest class: the temperature
 *                      -> 0 limit of _sample_categorical (deepsvg/model/utils.py:75-80) without the logits (replaces
 *                      the head GEMM + dsvg_argmax_rows in greedy_sample(temperature=0)).
 *   dsvg_head_sample   the same at a temperature > 0: out_idx = a draw from softmax(logits(row, slot, :) / temperature), the
 *                      reference's default decoding (greedy_sample(temperature = 1e-4), deepsvg/model/model.py:414-418) as a
 *                      Gumbel arg-max on the on-chip logit tile; draws identical to dsvg_sample_rows on the dense logits.
 *   dsvg_head_lse      the masked cross-entropy forward of SVGLoss (deepsvg/model/loss.py:51-57) on the compact token list:
 *                      lse[row * group + slot] (0 where the weight is 0) and sum_count = (sum of w (lse - logit[target]),
 *                      sum of w).  target / w are indexed tok * group + slot with tok = tok_idx ? tok_idx[row] : row
 *                      (tok < 0: list padding, weight 0) exactly as dsvg_masked_ce_fwd takes them (replaces head GEMM +
 *                      dsvg_masked_ce_fwd).  workspace: dsvg_head_lse_workspace_bytes(rows).
 *   dsvg_head_dlogits  its backward: dlogits[row, c] = w g (softmax - onehot), g = coef * (gscale ? *gscale : 1) /
 *                      sum_count[1], bf16 [rows, ld_d], ld_d = n_out rounded up to a multiple of 8, padding columns zero
 *                      (replaces a second head GEMM + dsvg_masked_ce_bwd; the logits are recomputed on chip). */
int64_t dsvg_head_pack_elems(int32_t n_out);
int dsvg_head_pack(const void* weight_bf16, int32_t n_out, void* packed, void* stream);
int dsvg_head_argmax(const void* x, const void* packed, const float* bias, int64_t rows, int32_t n_out, int32_t C,
                     int32_t* out_idx, void* stream);
int dsvg_head_sample(const void* x, const void* packed, const float* bias, int64_t rows, int32_t n_out, int32_t C,
                     float temperature, const void* seed, uint32_t site, int32_t* out_idx, void* stream);
int64_t dsvg_head_lse_workspace_bytes(int64_t rows);
int dsvg_head_lse(const void* x, const void* packed, const float* bias, int64_t rows, int32_t n_out, int32_t C,
                  const int32_t* target, const float* w, const int32_t* tok_idx, float* lse, float* sum_count,
                  float* workspace, int64_t workspace_bytes, void* stream);
int dsvg_head_dlogits(const void* x, const void* packed, const float* bias, int64_t rows, int32_t n_out, int32_t C,
                      const int32_t* target, const float* w, const int32_t* tok_idx, const float* lse,
                      const float* sum_count, const float* gscale, float coef, void* dlogits, int64_t ld_d, void* stream);

/* ------------------------------------------------------------------------------------------
 * Device-side batch assembly.  Replaces, for a whole batch, the per-item chain of
 * SVGTensorDataset.get_data (deepsvg/svgtensor_dataset.py:164-205): SVGTensor.from_data(...).add_eos().add_sos()
 * .pad(seq_len) (deepsvg/difflib/tensor.py:85-88,108-116,125-143), .cmds()/.args()/.get_relative_args()
 * (tensor.py:155-162,172-189) and the DataLoader's default collate (deepsvg/train.py:27-28).
 *   rows     int16 [n_rows, 12]: (command, 11 arguments in SVGTensor.arg_keys order) per stored drawing command
 *   slot_off int32 [n_slots+1]:  row range of slot variant*G + group; a variant is one stored (icon, augmentation)
 *                                pair (the list entries of the .pkl "tensors", svgtensor_dataset.py:106-109,155-156)
 *   variant  int32 [n_items]:    which stored variant each batch item takes
 * grouped == 0: sequences (item, group), commands [n_items, G, L], args / args_rel [n_items, G, L, 11], L = S+2;
 * grouped != 0: one sequence per item over all its groups, commands [n_items, 1, L], L = max_total_len+2.
 * Each sequence is SOS, the stored rows, EOS, then EOS padding; argument slots of SOS/EOS/pad rows are pad_val.
 * args and args_rel are optional (NULL = not wanted); args_rel follows get_relative_args with ARGS_DIM=args_dim.
 * Sequences longer than L-2 are cut (the host refuses to build such a store). */
int dsvg_assemble_batch(const int16_t* rows, int64_t n_rows, const int32_t* slot_off, int64_t n_slots,
                        const int32_t* variant, int64_t n_items, int32_t G, int32_t grouped, int32_t L,
                        float pad_val, int32_t args_dim, float* commands, float* args, float* args_rel,
                        void* stream);

/* ------------------------------------------------------------------------------------------
 * Affine maps of a batch, and batches augmented as they are assembled (csrc/paths_transform.hip): SVG.translate / rotate /
 * zoom / normalize / numericalize (deepsvg/svglib/svg.py:268-300, 392-394) and SVGDataset._augment / preprocess
 * (deepsvg/svg_dataset.py:137-156) on the tensors themselves.  The reference transforms np.float32 points one in-place
 * operation at a time (svglib/geom.py:136-151), so the definition is a short program of float32 steps
 * (tests/paths_transform_ref.py restates it in numpy float32, one rounding per operation):
 *  a transform is a list of K steps, 1 <= K <= DSVG_MAX_STEPS.  The kinds are launch constants: `kinds` holds 2 bits per
 *    step, step k in bits 2k..2k+1.  The parameters are device memory, fp32 [N, K, 3], one set per item, so random draws
 *    never leave the device.  Every enabled coordinate pair (x, y) of a live row goes through the steps in order, every
 *    arithmetic operation rounded to fp32 once, never contracted to a fused multiply-add:
 *      DSVG_STEP_TRANSLATE (vx, vy, -):  x = x + vx; y = y + vy
 *      DSVG_STEP_SCALE     (f, -, -):    x = x * f;  y = y * f
 *      DSVG_STEP_ROTATE    (c, s, deg):  x' = fl(fl(c x) - fl(s y)); y' = fl(fl(s x) + fl(c y)), with c and s the cosine and
 *                                        sine of the angle, computed by the caller in float64 and rounded to fp32 as
 *                                        get_rotation_matrix does (geom.py:14-22)
 *  slots: `m`, `l`: the end position (9:11); `c`: control1, control2 and the end position (5:11); `a`: the end position takes
 *    every step, the radii (0:2) take scale steps only (Radius.translate is a no-op in the reference), a rotate step adds
 *    deg to slot 2 as one fp32 add, the flags are copied.  The reference cannot rotate an arc at all: the arc rule under
 *    rotation is this library's own.  SOS, EOS, `z`, commands outside 0..6 and every slot CMD_ARGS_MASK does not enable
 *    are copied unchanged.
 *  numericalize = n > 0 runs after the steps: every enabled slot of a live row becomes clip(round-half-even(v), 0, n - 1),
 *    the rule of dsvg_canonicalize.
 *  No step is ever elided or merged, not a scale by exactly 1 and not a translate pair that cancels: (p - 128) + 128 is
 *    not p in fp32, and the reference executes it.
 *  The reference's calls as step lists, with view-box size vb, centre c = vb / 2 and every constant an fp32:
 *    zoom(f, center) = T(-c), S(f), T(center); rotate(deg, center) = T(-c), R(deg), T(center); normalize(target) =
 *    zoom(fl(target / vb), target / 2); SVG.numericalize(n) = normalize(n), then round and clip; _augment = zoom(f), T(dx, dy).
 * dsvg_paths_transform: commands [N, G, S] / args [N, G, S, 11] fp32, G * S <= 2048 -> out_args of the same shape.  A group
 *    ends at its first EOS; rows at or behind it are copied unchanged.  No row is dropped or invalidated.  One workgroup
 *    per icon, one thread per row.
 * dsvg_assemble_augmented: dsvg_assemble_batch over a float32 row store [n_rows, 12] (16-byte aligned) with the same
 *    slot_off / variant addressing and the same outputs; item i of the batch runs parameter set i on every row it loads,
 *    then the rounding.  args_rel is formed from the transformed and rounded values (the reference calls get_relative_args
 *    on the numericalised tensor): the previous real command's end position is transformed too.
 * Both: no atomics, no workspace, no device-to-host read, every output element written: bit-reproducible, capturable. */
#define DSVG_STEP_TRANSLATE 0
#define DSVG_STEP_SCALE 1
#define DSVG_STEP_ROTATE 2
#define DSVG_MAX_STEPS 16
int dsvg_paths_transform(const float* commands, const float* args, int64_t N, int32_t G, int32_t S, int32_t K,
                         uint32_t kinds, const float* params, int32_t numericalize, float* out_args, void* stream);
int dsvg_assemble_augmented(const float* rows, int64_t n_rows, const int32_t* slot_off, int64_t n_slots,
                            const int32_t* variant, int64_t n_items, int32_t G, int32_t grouped, int32_t L,
                            float pad_val, int32_t args_dim, int32_t K, uint32_t kinds, const float* params,
                            int32_t numericalize, float* commands, float* args, float* args_rel, void* stream);

/* ------------------------------------------------------------------------------------------
 * SVG path text -> padded rows (csrc/svg_parse.hip): the reference's SVGPath.from_str(s).to_tensor() (svglib/svg_path.py:79-157,
 * svg_command.py:51-120) and the `points` lists of SVGPolyline / SVGPolygon (svg_primitive.py:196-207) for P strings at once.
 * tests/svgio_ref.py restates everything below in plain Python; tests/golden/svgio/parse.npz holds the reference's results.
 *  input: data uint8 [B], the UTF-8 bytes of the strings back to back; offsets int64 [P + 1] (clamped to [0, B] and to each
 *    other on the device: no offset can make a read leave the buffer); kind uint8 [P]: DSVG_SVG_PATH a `d` attribute,
 *    DSVG_SVG_POLYLINE / DSVG_SVG_POLYGON a `points` list (any other value reads as PATH); slot int32 [P]: the output group
 *    n * G + g the string fills, -1 = status only.
 *  tokens: a command letter is one of MmZzLlHhVvCcSsQqTtAa (kind PATH only; in a points list every letter is a separator).
 *    Numbers are what re.findall finds for [-+]?[0-9]*\.?[0-9]+(?:[eE][-+]?[0-9]+)? - leftmost, greedy, with backtracking -
 *    stated as an automaton over the byte classes digit, dot, sign, e/E, other (bytes >= 0x80 included) with the states
 *    IDLE, SIGN, DOT0 ([sign] dot, no digit yet), INT, INTDOT, FRAC, EXP0 (number, e), EXPSIGN (number, e, sign), EXPD:
 *                 digit   dot      sign      e      other
 *      IDLE       INT     DOT0     SIGN      IDLE   IDLE
 *      SIGN       INT     DOT0     SIGN      IDLE   IDLE
 *      DOT0       FRAC    DOT0     SIGN      IDLE   IDLE
 *      INT        INT     INTDOT   SIGN      EXP0   IDLE
 *      INTDOT     FRAC    DOT0     SIGN      IDLE   IDLE
 *      FRAC       FRAC    DOT0     SIGN      EXP0   IDLE
 *      EXP0       EXPD    DOT0     EXPSIGN   IDLE   IDLE
 *      EXPSIGN    EXPD    DOT0     SIGN      IDLE   IDLE
 *      EXPD       EXPD    DOT0     SIGN      IDLE   IDLE
 *    INT, FRAC and EXPD accept.  A number goes on from INT with digit / dot / e, from FRAC with digit / e, from EXP0 with
 *    digit / sign, from INTDOT, EXPSIGN and EXPD with a digit; on any other byte it ends at its last accepting byte (1 byte
 *    back from INTDOT and EXP0, 2 from EXPSIGN: `1.` is 1, `4e` is 4, `4e+` is 4) and the bytes behind that are read again as
 *    from IDLE, which the table's rows already say.  A number starts at a byte that leads to SIGN, to INT from IDLE, or to
 *    DOT0 from anything but SIGN; from EXPSIGN to DOT0 it starts one byte earlier (`4e+.5` is 4 and +.5).  So `1.5.5` is 1.5
 *    and .5, `10-2e1` is 10 and -20, and a sign not followed by a digit or .digit is skipped.  One separator is read behind
 *    the last byte.  Numbers in front of the first command letter are dropped unread.
 *  value: sign, then leading zeros and the trailing zeros of the fraction dropped, the remaining digits an integer w, e10 =
 *    exponent - fraction digits kept.  With w < 2^53 and |e10| <= 22 the value is (double)w * 10^e10 (e10 >= 0) or (double)w /
 *    10^-e10: one correctly rounded operation on exact operands, equal to strtod / Python's float() bit for bit; -0 keeps its
 *    sign.  Anything else (more digits, an accumulator past 2^64, a larger exponent) is DSVG_SVG_SLOW_NUMBER.  This is the
 *    FAST RULE, the rule of dsvg_svg_parse.
 *  value, the EXACT RULE (dsvg_svg_parse_exact; csrc/decimal_exact.h, restated in tests/svgio_exact_ref.py): the digit string
 *    (integer and fraction digits, the dot removed) is stripped of its leading zeros and of its trailing zeros, and every
 *    stripped trailing zero, integer or fractional, raises the exponent by one.  What is left is an integer w of nd digits
 *    and e10 = written exponent (saturated as above) - fraction digits + stripped trailing zeros.  w == 0 is a zero of the
 *    number's sign, whatever the exponent.  Otherwise, with nd <= DSVG_SVG_EXACT_DIGITS and DSVG_SVG_EXACT_E10_MIN <= e10 <=
 *    DSVG_SVG_EXACT_E10_MAX, the value is the float64 nearest to w * 10^e10, ties to even: strtod / Python's float() bit for
 *    bit, formed with integers only (w < 10^19 < 2^64 is one word, 5^38 and 5^64 fit 89 and 149 bits, every result is a normal
 *    float64 between 1e-64 and 1e57).  Anything else is DSVG_SVG_SLOW_NUMBER.  A number below the domain is zero in fp32 and one
 *    above it is infinite there: the domain holds every number of at most 19 significant digits whose fp32 value is finite and
 *    not zero.  Where the fast rule gives a value the exact rule gives the same one; it only turns some SLOW_NUMBERs into
 *    values.  Everything else - tokens, the first error in reading order, numbers in front of the first letter never
 *    converted, RANGE, the fp32 position arithmetic, the counts - is the same for both entries.
 *  commands: per letter with k numbers behind it.  z: k = 0, and the position returns to the sub-path's initial position.
 *    Any other letter: k > 0 and a multiple of its arity (m l t 2; h v 1; c 6; s q 4; a 7), k / arity commands; k = 0 is
 *    DSVG_SVG_ARG_COUNT like every other miscount (the reference indexes its empty command list and raises).  An m with more
 *    than 2 numbers is a move and then l on the rest.  ARITHMETIC IS FLOAT32: every number is rounded to fp32 when it becomes
 *    a coordinate (the reference's Point is a float32 array, svglib/geom.py:60-75), a lower-case letter then adds the current
 *    position in fp32, one rounding per add (Point.translate); radii, angle and flags are never translated, and a flag is
 *    trunc(value).  h and v take the other coordinate from the current position.  q is a c with both control points the
 *    quadratic's one (the reference's rule, not degree elevation).  s and t: control1 = fl(2 pos - control2 of the command
 *    before) when that was a Bezier of any letter, else pos; control2 is given (s) or equals control1 (t).
 *  rows (SVGPath.from_commands, allow_empty=False, add_closing=False): commands in front of the first move, and behind a z
 *    until the next move, move the position and write nothing; a move opens a sub-path, and a sub-path without a command
 *    writes nothing, neither m nor z; otherwise m (the move's target), its rows, and z when it was closed.  Arcs stay `a`
 *    rows.  POLYLINE / POLYGON: an even count of numbers, rows m p0, l p1, ... and z for a polygon (no closing line); fewer
 *    than 2 points leave no row.
 *  output, framed as dsvg_paths_expand frames its result: commands [N, G, S] / args [N, G, S, 11] fp32 (SOS, the rows, EOS...;
 *    -1 in every slot CMD_ARGS_MASK does not enable, a z row all -1; a group nobody fills is SOS, EOS...), len_groups int32
 *    [N, G], status int32 [P], valid uint8 [N].  status, in this order of precedence: BAD_SLOT (slot outside [-1, N G) or
 *    shared by two strings; such a string is not parsed); the first ARG_COUNT or SLOW_NUMBER in reading order; ROWS_OVERFLOW
 *    (more than S - 2 rows); RANGE (a written value is not finite in fp32); EMPTY (no row: not an error); OK.  An icon is
 *    valid when every string with a slot inside it is OK or EMPTY; an invalid icon is SOS, EOS... in every group with
 *    len_groups 0.  workspace: int32 [2 N G].  Five launches on one stream, no atomics, nothing read back, every output element
 *    written: bit-reproducible, capturable. */
#define DSVG_SVG_PATH 0
#define DSVG_SVG_POLYLINE 1
#define DSVG_SVG_POLYGON 2
#define DSVG_SVG_OK 0
#define DSVG_SVG_EMPTY 1
#define DSVG_SVG_ARG_COUNT 2
#define DSVG_SVG_SLOW_NUMBER 3
#define DSVG_SVG_ROWS_OVERFLOW 4
#define DSVG_SVG_BAD_SLOT 5
#define DSVG_SVG_RANGE 6
#define DSVG_SVG_TILE 64 /* bytes of a string one wave reads at a time */
int dsvg_svg_parse(const uint8_t* data, int64_t B, const int64_t* offsets, const uint8_t* kind, const int32_t* slot,
                   int64_t P, int64_t N, int32_t G, int32_t S, int32_t* workspace, float* commands, float* args,
                   int32_t* len_groups, int32_t* status, uint8_t* valid, void* stream);
/* The same call - arguments, launches, outputs - with the exact rule for the value of a number. */
#define DSVG_SVG_EXACT_DIGITS 19
#define DSVG_SVG_EXACT_E10_MIN (-64)
#define DSVG_SVG_EXACT_E10_MAX 38
int dsvg_svg_parse_exact(const uint8_t* data, int64_t B, const int64_t* offsets, const uint8_t* kind, const int32_t* slot,
                         int64_t P, int64_t N, int32_t G, int32_t S, int32_t* workspace, float* commands, float* args,
                         int32_t* len_groups, int32_t* status, uint8_t* valid, void* stream);

/* ------------------------------------------------------------------------------------------
 * Fused FFN sub-block, bf16, d_model = 256 / dim_feedforward = 512 (csrc/ffn_fused.hip):
 *     y = x + drop_r( linear2( drop_h( relu( linear1( LayerNorm(x) ) ) ) ) )
 * replaces norm2 + linear1 + activation + dropout + linear2 + dropout2 + the residual add of
 * deepsvg/model/layers/improved_transformer.py:51-53 (encoder layer) and :138-140 (decoder layer) in ONE launch;
 * the normalised rows and the hidden activations never reach HBM.
 *   dsvg_ffn_pack   once per optimiser step: re-lays linear1.weight [512,256] / linear2.weight [256,512] of n_layers
 *                   layers out as bf16 MFMA-fragment-major chunk images, straight from the fp32 master parameters
 *                   `flat_f32`; offs = int64 device array [n_layers][5] of element offsets of (linear1.weight,
 *                   linear1.bias, linear2.weight, norm.weight, norm.bias).  The LayerNorm's affine part is folded into
 *                   linear1: W1' = W1 diag(gamma), b1' = b1 + W1 beta (b1_folded, fp32 [n_layers][512]).
 *                   packed_fwd [n_layers][16][32 KiB], packed_bwd [n_layers][16][48 KiB] (dsvg_ffn_pack_bytes(n, 0 | 1));
 *                   of a packed_bwd chunk [W1' | W2^T | W1'^T] only the last 16 KiB have a reader, dsvg_ffn_bwd_dx.
 *                   w2p (optional, bf16 [n_layers][256][512]): linear2.weight with its columns in fragment order, the B
 *                   operand of the unfused input-gradient GEMM dpre = dym . W2p.
 *   dsvg_ffn_fwd    x, y bf16 [rows, 256] (row stride 256); packed_fwd_layer / b1_folded = that layer's slices; b2 fp32;
 *                   dropout sites / seed as everywhere else (draw scheme "v2", private to the fused kernels);
 *                   stages: 0 = default (workgroups of 128 rows up to 32,768 rows, of 256 rows above), 2 = 128-row
 *                   workgroups, 3 / 4 = 256-row workgroups with that many weight-ring slots (2 / 3 / 4: scalar
 *                   activation code, bit-identical to each other), 6 / 7 = 4 / 2 with the packed activation code (what 0
 *                   picks; rounding-level differences to 2 / 3 / 4).  Any other value is an error (5, the role-specialised
 *                   kernel of round 5, is removed).
 *                   Training calls pass h_out (bf16 [rows, 512], hidden columns in
 *                   FRAGMENT ORDER: position p(j) = j with bits 2 and 3 swapped), xh_out = (x - mean) * rstd (bf16
 *                   [rows, 256]) and rstd_out (fp32 [rows]) for the backward pass; inference passes NULL for all three.
 * Buffers are caller-owned; all work is enqueued on `stream`. */
int64_t dsvg_ffn_pack_bytes(int32_t n_layers, int32_t which);
int dsvg_ffn_pack(const float* flat_f32, const int64_t* offs, int32_t n_layers, int32_t d_model, int32_t d_ff,
                  void* packed_fwd, void* packed_bwd, float* b1_folded, void* w2p, void* stream);
int dsvg_ffn_fwd(const void* x, const void* packed_fwd_layer, const float* b1_folded, const float* b2, void* y,
                 void* h_out, void* xh_out, float* rstd_out, int64_t rows, float eps, float drop_p,
                 uint32_t site_hidden, uint32_t site_res, const void* seed, int32_t stages, void* stream);
/* Backward of the fused FFN sub-block (csrc/ffn_fused.hip), from what a training dsvg_ffn_fwd stored (h, xh, rstd):
 *   dym  = dy * residual-dropout mask (dsvg_drop_apply; dym == dy when drop_p == 0), bf16 [rows, 256];
 *   dpre = (dym . W2p) gated by h > 0, x 1 / (1 - drop_p): one dsvg_gemm with gate = h, or dsvg_ffn_gate_dw2; bf16 [rows, 512]
 *          with the hidden columns in FRAGMENT ORDER (position p(j) = j with bits 2 and 3 swapped), like h;
 *   dx   = dy + LayerNorm'(dpre . W1'): dsvg_ffn_bwd_dx, the only reader of packed_bwd (its W1'^T part).
 * The caller then runs G2p = dym^T h [256, 512], G1p = dpre^T xh [512, 256] (+ row sums db1p, and db2 = colsum(dym))
 * with dsvg_gemm, and dsvg_ffn_wgrad_finish turns (G1p, db1p, G2p) into the gradients of linear1.weight / bias,
 * linear2.weight and of the LayerNorm's gamma / beta (w1 = fp32 master linear1.weight [512, 256]).
 * Replaces the autograd backward of deepsvg/model/layers/improved_transformer.py:51-53 / :138-140.
 * dx_masked (optional): a second output, dx with the dropout mask (drop_p, drop_site, ids row * 256 + column) replayed on
 * it - exactly dsvg_drop_apply(dx) - for the attention sub-block's backward, which starts from it */
int dsvg_ffn_bwd_dx(const void* dpre, const void* x, const void* dy, const void* packed_bwd_layer, void* dx,
                    int64_t rows, float eps, void* dx_masked, float drop_p, uint32_t drop_site, const void* seed,
                    void* stream);
/* dpre and the linear2 weight gradient from one staging of their common operands (csrc/ffn_bwd_gate.hip):
 *   dpre = (dym . W2p) gated by hp > 0, x gate_scale     (bf16 [rows, 512], bit-identical to the dsvg_gemm with gate = hp)
 *   G2p = dym^T hp [256, 512] fp32, db2 = colsum(dym) [256] fp32
 * dym bf16 [rows, 256], hp bf16 [rows, 512] (the h dsvg_ffn_fwd stored), w2p bf16 [256, 512] (the packed W2 dsvg_gemm reads
 * with b_kc = 0); all row-major and dense.  G2p / db2 come as split_k (> 1) slices in the layout of dsvg_gemm(dym, hp, a_kc =
 * b_kc = 0, split_k, rowsum = db2) - workspace of dsvg_gemm_workspace_bytes(256, 512, split_k) - and are reduced the same way:
 * queued inside an open dsvg_defer_scope, valid after dsvg_flush_deferred. */
int dsvg_ffn_gate_dw2(const void* dym, const void* hp, const void* w2p, float gate_scale, void* dpre, int64_t rows,
                      int32_t split_k, float* g2p, float* db2, float* workspace, int64_t workspace_bytes, void* stream);
int dsvg_ffn_wgrad_finish(const float* g1p, const float* db1p, const float* g2p, const float* w1, const float* gamma,
                          const float* beta, float* dw1, float* db1, float* dw2, float* dgamma, float* dbeta,
                          void* stream);
/* the same for n_layers layers in one launch per 16: ptrs = n_layers x 11 pointers in the argument order of
 * dsvg_ffn_wgrad_finish (g1p, db1p, g2p, w1, gamma, beta, dw1, db1, dw2, dgamma, dbeta), a host array */
int dsvg_ffn_wgrad_finish_many(const void* const* ptrs, int32_t n_layers, void* stream);
/* development probe of dsvg_ffn_fwd: buf = device buffer of (workgroups x 8 waves x 4) uint64 time stamps (kernel start,
 * LayerNorm done, chunk loop done, stores issued) or NULL to switch it off (scripts/ffn_phase_probe.py) */
int dsvg_ffn_debug_clock(void* buf);
/* the same for dsvg_gs_layer_fwd: (workgroups * 8 * 8) uint64 - kernel start, LayerNorm 1, in_proj + attention, out_proj +
 * LayerNorm 2, linear1, linear2, stores issued (scripts/gs_phase_probe.py) */
int dsvg_gs_debug_clock(void* buf);

/* ------------------------------------------------------------------------------------------
 * Fused attention sub-block (d_model 256, 8 heads of 32, sequences of at most 32 tokens, bf16):
 *     x1 = x + drop_r( out_proj( MHA( LayerNorm(x) ) ) )
 * one launch instead of LayerNorm + in_proj GEMM + attention + out_proj GEMM
 * (deepsvg/model/layers/improved_transformer.py:43-46 and :127-131, layers/attention.py, layers/functional.py:168,197-248).
 * dsvg_attn_pack: bf16 MFMA-fragment images (dsvg_attn_pack_bytes(n_layers) bytes, 512 KiB per layer) of in_proj_weight
 *   and out_proj.weight straight from the fp32 master buffer; offs = int64 [n_layers][2] element offsets of
 *   (in_proj_weight, out_proj.weight).  Re-pack after every optimiser step.
 * dsvg_attn_block_fwd: x bf16 [rows, 256].  Layouts as dsvg_attention_fwd: dense (seq_off NULL: sequence b = rows
 *   b*S .. b*S+S-1, optional key_mask bit j = key j visible) or packed (seq_off + tile_first from dsvg_attention_tiles,
 *   block-diagonal attention inside each tile of <= 32 rows).  Rows behind the last sequence (bucket padding up to
 *   `rows`) get finite values.  Dropout: site_probs on the probabilities (same element ids as dsvg_attention_fwd),
 *   site_res on the residual branch (ids row*256 + col, replayable by dsvg_drop_apply).
 *   seq_add (optional, dense layouts): bf16 [n_seq, 256] with row stride seq_add_ld elements (256 = contiguous; a column block
 *   of a wider matrix otherwise: the conditioning rows of all the layers of a stack come from ONE GEMM), x1 += drop(seq_add[sequence]) with one mask element per
 *   (sequence, channel), site_seq_add - the decoder's linear_global(z) term (improved_transformer.py:131-136), same draws
 *   as dsvg_bcast_add_fwd, whose backward (dsvg_bcast_add_bwd) applies unchanged.
 *   Training outputs (all NULL for inference, all set otherwise) are what the unfused backward reads:
 *   xn_out = LayerNorm(x) bf16 [rows,256], qkv_out bf16 [rows,768], ao_out = head outputs bf16 [rows,256],
 *   mean_out / rstd_out fp32 [rows].
 * ------------------------------------------------------------------------------------------ */
int64_t dsvg_attn_pack_bytes(int32_t n_layers);
int dsvg_attn_pack(const float* flat_f32, const int64_t* offs, int32_t n_layers, int32_t d_model, int32_t n_heads,
                   void* packed, void* stream);
int dsvg_attn_block_fwd(const void* x, const void* packed_layer, const float* in_bias, const float* out_bias,
                        const float* gamma, const float* beta, const uint64_t* key_mask, const int32_t* seq_off,
                        const int32_t* tile_first, int64_t n_seq, int32_t S, int64_t rows, void* x1, void* xn_out,
                        void* qkv_out, void* ao_out, float* mean_out, float* rstd_out, float eps, float scale,
                        float drop_p, uint32_t site_probs, uint32_t site_res, const void* seed,
                        const void* seq_add, int64_t seq_add_ld, uint32_t site_seq_add, void* stream);
/* ------------------------------------------------------------------------------------------
 * One launch per layer and direction for the short-sequence ("group") stages: the whole pre-LN block
 *     x1 = x  + drop( out_proj( MHA( LayerNorm1(x) ) ) ) [+ drop( seq_add[sequence] )]
 *     x2 = x1 + drop( linear2( drop( relu( linear1( LayerNorm2(x1) ) ) ) ) )
 * of deepsvg/model/layers/improved_transformer.py:42-54 and :126-141 as used by hierarchical_encoder (model/model.py:153-161)
 * and hierarchical_decoder (:246-254): d_model 256, dim_ff 512, 8 heads, bf16, dense sequences of S tokens with 32 % S == 0,
 * rows = n_seq * S.  They replace ~15 (forward) / ~25 (backward) launches of 5-12 us each; what they read and write is
 * exactly what those launches read and write, with the same dropout draws (sites site0 + 0 probabilities, + 1 attention
 * residual, + 2 per-sequence term, + 3 hidden, + 4 FFN residual), so fused and unfused launches can be mixed freely.
 * dsvg_gs_pack: bf16 MFMA-fragment images (dsvg_gs_pack_bytes(n_layers) bytes = 1 MiB per layer, each) of the layer's four
 *   weight matrices for the forward and for the backward kernel, straight from the fp32 master buffer; offs = int64
 *   [n_layers][4] element offsets of (in_proj_weight, out_proj.weight, linear1.weight, linear2.weight).  Re-pack after
 *   every optimiser step.
 * dsvg_gs_layer_fwd: x bf16 [rows,256] -> x2.  key_mask (optional): bit j of key_mask[b] = key j of sequence b visible.
 *   seq_add (optional): bf16 [n_seq,256] (the decoder's linear_global(z) term, drawn like dsvg_bcast_add_fwd).
 *   Training outputs (all NULL for inference, all set otherwise) = what the backward pass reads, in the layouts of the
 *   unfused launches: mean1 / rstd1 / mean2 / rstd2 fp32 [rows], xn1 = LayerNorm1(x), ao (head outputs), x1,
 *   xn2 = LayerNorm2(x1) bf16 [rows,256], qkv bf16 [rows,768], h bf16 [rows,512] (after ReLU and dropout).
 *   The forward call also takes sequences of any length 1 .. 32 (32 / S whole sequences per tile) and a sequence offset:
 *   seq_base > 0 = the launch covers sequences seq_base .. seq_base + n_seq - 1 of a longer buffer (all pointers at their
 *   first row; dropout draws indexed from the buffer's first row), ffn_format != 0 = xn2 and h come out as the fused FFN
 *   kernels' backward reads them (xn2 without gamma / beta, h with fragment-ordered columns, dsvg_ffn_fwd).  Together: the
 *   training forward of a large dense stage runs the sequences that fill whole rounds of the chip on dsvg_attn_block_fwd +
 *   dsvg_ffn_fwd and the remainder on this kernel, into the same saved tensors.
 * dsvg_gs_layer_bwd: dx2 = dL/dx2 bf16 [rows,256] and the saved tensors -> dx = dL/dx, plus the token-major operands of
 *   the four weight-gradient GEMMs the caller runs afterwards - dym = dx2 * mask(site0+4) (with h: linear2), dpre (with
 *   xn2: linear1), dx1m = dx1 * mask(site0+1) (with ao: out_proj), dqkv (with xn1: in_proj); their column sums are the bias
 *   gradients - dx1 (optional, for dsvg_bcast_add_bwd of the per-sequence term) and the four LayerNorm parameter
 *   gradients (fp32 [256] each; reduced from per-tile partials in `workspace`, dsvg_gs_bwd_workspace_bytes(n_seq, S)
 *   bytes, through the deferred-reduction queue when a scope is open on the stream).
 *   dg (optional, bf16 [n_seq, 256]; ABI 6): the gradient of the per-sequence term, = dsvg_bcast_add_bwd(dx1, site0 + 2) bit
 *   for bit, formed from the tile while dx1 is on chip - that launch and the dx1 store (pass dx1 = NULL) are then not needed.
 * ------------------------------------------------------------------------------------------ */
int64_t dsvg_gs_pack_bytes(int32_t n_layers);
int dsvg_gs_pack(const float* flat_f32, const int64_t* offs, int32_t n_layers, int32_t d_model, int32_t d_ff,
                 int32_t n_heads, void* packed_fwd, void* packed_bwd, void* stream);
int dsvg_gs_layer_fwd(const void* x, const void* packed_fwd_layer, const float* in_bias, const float* out_bias,
                      const float* b1, const float* b2, const float* gamma1, const float* beta1, const float* gamma2,
                      const float* beta2, const uint64_t* key_mask, const void* seq_add, int64_t seq_add_ld, int64_t n_seq, int32_t S,
                      void* x2, float* mean1, float* rstd1, void* xn1, void* qkv, void* ao, void* x1, float* mean2,
                      float* rstd2, void* xn2, void* h, float eps, float scale, float drop_p, uint32_t site0,
                      const void* seed, int64_t seq_base, int32_t ffn_format, void* stream);
int64_t dsvg_gs_bwd_workspace_bytes(int64_t n_seq, int32_t S);
int dsvg_gs_layer_bwd(const void* dx2, const void* packed_bwd_layer, const void* x, const float* mean1, const float* rstd1,
                      const void* qkv, const void* x1, const float* mean2, const float* rstd2, const void* h,
                      const float* gamma1, const float* gamma2, const uint64_t* key_mask, int64_t n_seq, int32_t S,
                      void* dx, void* dx1, void* dym, void* dpre, void* dx1m, void* dqkv, float* dgamma2, float* dbeta2,
                      float* dgamma1, float* dbeta1, float scale, float drop_p, uint32_t site0, const void* seed,
                      void* workspace, int64_t workspace_bytes, void* dg, void* stream);
/* One launch per STACK and direction (ABI 8): the tiles (32 rows = whole sequences) are independent across the layers, so a
 * workgroup carries its rows through up to 4 layers - reference: the layer loops of deepsvg/model/layers/transformer.py:168-188
 * (TransformerEncoder.forward) and :214-242 (TransformerDecoder.forward) over the 4 layers of hierarchical_encoder /
 * hierarchical_decoder.  Same arithmetic, same stores and same dropout draws as n_layers calls of dsvg_gs_layer_fwd /
 * dsvg_gs_layer_bwd in a row (bit-identical; tests/test_kernels_gpu.py::test_gs_stack_*), minus the launch ramps, the
 * reloads of the rows between the layers, and the gradient stores between the layers of the backward pass.
 *   dsvg_gs_stack_fwd: x -> layers[n_layers - 1].x2.  Per layer: the arguments of dsvg_gs_layer_fwd; training outputs for every
 *     layer or for none; x2 of an inner layer may be NULL for inference.  seq_add of every layer has the row stride seq_add_ld
 *     (column blocks of one [n_seq, n_layers * 256] product).  seq_base = 0, ffn_format = 0.
 *   dsvg_gs_stack_bwd: dx2 = dL/d(layers[n_layers - 1].x2) -> layers[0].dx; `layers` in FORWARD order, walked from the last
 *     one.  Per layer: the arguments of dsvg_gs_layer_bwd; dx of layers 1 .. may be NULL (not stored); every layer's workspace
 *     has workspace_bytes >= dsvg_gs_bwd_workspace_bytes(n_seq, S); dg (optional) has the row stride dg_ld (column blocks of one
 *     [n_seq, n_layers * 256] buffer: the concatenated gradient of the conditioning product, no concatenation launch). */
typedef struct dsvg_gs_fwd_layer {
    const void* packed_fwd_layer;
    const float *in_bias, *out_bias, *b1, *b2, *gamma1, *beta1, *gamma2, *beta2;
    const void* seq_add;            /* or NULL */
    void* x2;
    float *mean1, *rstd1;
    void *xn1, *qkv, *ao, *x1;
    float *mean2, *rstd2;
    void *xn2, *h;
    uint32_t site0;
    uint32_t reserved_;
} dsvg_gs_fwd_layer;
typedef struct dsvg_gs_bwd_layer {
    const void* packed_bwd_layer;
    const void* x;
    const float *mean1, *rstd1;
    const void *qkv, *x1;
    const float *mean2, *rstd2;
    const void* h;
    const float *gamma1, *gamma2;
    void *dx, *dx1, *dym, *dpre, *dx1m, *dqkv, *dg;
    float *dgamma2, *dbeta2, *dgamma1, *dbeta1;
    void* workspace;
    uint32_t site0;
    uint32_t reserved_;
} dsvg_gs_bwd_layer;
int dsvg_gs_stack_fwd(const void* x, const dsvg_gs_fwd_layer* layers, int32_t n_layers, const uint64_t* key_mask,
                      int64_t seq_add_ld, int64_t n_seq, int32_t S, float eps, float scale, float drop_p, const void* seed,
                      void* stream);
int dsvg_gs_stack_bwd(const void* dx2, const dsvg_gs_bwd_layer* layers, int32_t n_layers, const uint64_t* key_mask,
                      int64_t n_seq, int32_t S, float scale, float drop_p, const void* seed, int64_t workspace_bytes,
                      int64_t dg_ld, void* stream);
/* test hook: raw ds_read_b64_tr_b16 on a 4 KiB LDS image img[i]=i, lane l reads at byte offset off[l] */
int dsvg_probe_trread(const int* off, short* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * The latent chain between the encoder and the decoder as ONE launch per direction (csrc/group_stage.hip):
 *     z_i = z_{i-1} + relu(W_i z_{i-1} + b_i), i = 1 .. n_res   (ResNet, deepsvg/model/basic_blocks.py:59-65)
 *     out = W_b z_{n_res} + b_b                                  (Bottleneck, deepsvg/model/model.py:193-198)
 * bf16, d_model = dim_z = 256, one row per icon.  weights / biases: host arrays of n_res + 1 device pointers (row-major bf16
 * [256, 256] / fp32 [256]; the final linear last); z_out / r_out: host arrays of n_res device pointers for the training
 * outputs z_1 .. z_n and the ReLU outputs r_1 .. r_n (bf16 [rows, 256]; pass NULL arrays for inference).
 * Backward: dout = dL/dout; dpre_out[i] = dz_{i+1} where r_{i+1} > 0 (the token-major operand of dW_{i+1} = dpre^T z_i; the
 * final linear's dW takes dout and z_n), dz0 = dL/dz0.  Replaces 2 launches per block forward and 3 backward (the autograd
 * backward of the same lines). */
int dsvg_latent_chain_fwd(const void* z0, const void* const* weights, const float* const* biases, int32_t n_res,
                          void* const* z_out, void* const* r_out, void* out, int64_t rows, void* stream);
int dsvg_latent_chain_bwd(const void* dout, const void* const* weights, const void* const* r, int32_t n_res,
                          void* const* dpre_out, void* dz0, int64_t rows, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DSVG_H */
