/* libmfvit_hip.so - C ABI of the MI355X-native (gfx950) Multi-Feature-ViT hot path.
 *
 * The reference (endiqq/Multi-Feature-ViT) is pure Python on stock PyTorch: it has no FFI.  Its drop-in boundary
 * is the Python constructor / train-step API.  This C ABI is the layer underneath that API: every
 * entry point replaces a group of ATen ops dispatched by a cited piece of reference Python, takes plain device
 * pointers and sizes, never allocates, never synchronises, launches on the given HIP stream, and returns
 * 0 or a negative errno-style code (MFVIT_E*).  The caller owns all memory.  Thread-safe and stream-ordered.
 *
 * Paths below are relative to the reference root; MOD = moco_pretraining/moco/model/module.py,
 * FUS = moco_pretraining/moco/model/crossvit_2vits_2additionaloutputs_..._std002_sum.py,
 * BLD = moco_pretraining/moco/moco/builder_vit_mocov3structure_mocov2loss.py, OPT = moco_pretraining/moco/moco/optimizer.py,
 * MAIN_CA / MAIN_SS / MAIN_MOCO = the three main_*.py drivers (SURVEY.md alias table).
 */
#ifndef MFVIT_H
#define MFVIT_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* mfvit_stream_t; /* hipStream_t */

#define MFVIT_OK 0
#define MFVIT_EINVAL (-22)
#define MFVIT_ENOSYS (-38)
#define MFVIT_ELAUNCH (-5)

#define MFVIT_F32 0  /* exact-f32 MFMA path (parity mode: logits within 1e-3 of the f32 CPU oracle) */
#define MFVIT_BF16 1 /* bf16 operands, f32 accumulate / residual / statistics (throughput mode) */
/* SPLIT bf16 ("bf16x3"): every MFMA operand is kept as hi = bf16(x), lo = bf16(x - hi) (16 mantissa bits) and every product runs as
 * three bf16 MFMAs (hi*hi + lo*hi + hi*lo) with f32 accumulation: f32-grade results (logits within 1e-3 of the f32 CPU path, the
 * reference's CA finetune is fp32: MAIN_CA:862-882 has no autocast) at a third of the bf16 MFMA rate instead of the f32 MFMA rate
 * (1/16).  Tensors of this dtype use the "I32" storage layout: a logical row-major [M][N] matrix (N % 32 == 0) is a bf16 [M][2N]
 * array, every group of 32 logical columns stored as [hi x 32 | lo x 32]; leading dimensions are in STORAGE elements (2 x logical). */
#define MFVIT_BF16X3 2
/* fp16 operands (v_mfma_f32_32x32x16_f16), f32 accumulate / residual / statistics: the arithmetic of the reference's autocast
 * pretraining (MAIN_MOCO:349,533); pair with mfvit_amp_unscale for the GradScaler semantics (MAIN_MOCO:546-548). */
#define MFVIT_F16 3
/* SPLIT fp16, ATTENTION OPERANDS ONLY (round 5): the qkv tensor of mfvit_attention_fwd / _bwd in the I32 layout with hi = f16(x),
 * lo = f16(x - hi) (|x| <= 65504; 22 mantissa bits above 2^-2, an absolute floor of 2^-25 below); out, dout and dqkv of those two calls
 * stay MFVIT_BF16X3.  This is what the encoder runs in bf16x3 mode wherever the whole-head kernels apply (head_dim 32, T <= 224):
 * mfvit_linear_fwd epilogue 5 writes the qkv projection in this form, and every MFMA of the attention core is the f16 one - the
 * probabilities and score gradients are split (or, in the backward, rounded) to fp16 with a third of the vector instructions the
 * bf16 split needs.  No other entry point accepts this tag. */
#define MFVIT_X3F16 4

/* ABI history: 3 = rounds 3 - 4.  4 (round 5, BREAKING): mfvit_linear_fwd_persistent / mfvit_linear_fwd_ws (dropped in round 4 without a
 * version bump) and mfvit_mhsa_fused_fwd are gone; MFVIT_X3F16, linear epilogue 5, mfvit_attention_qkv_dtype and mfvit_adam_step_dev are new.
 * 5 (round 6, BREAKING): mfvit_adam_step_dev is gone (the whole-step HIP graph it served was removed); mfvit_vit_cfg grew `stream_share` (the per-call form of
 * mfvit_set_stream_share); mfvit_prof_collect_tags is new. */
int mfvit_abi_version(void);
const char* mfvit_build_info(void);

/* ------------------------------------------------------------------------------------------------------------
 * ViT-S/16 encoder (the backbone the reference imports as `vits` / `vits_returnftrs`, ABSENT from its tree;
 * call sites MAIN_SS:276,711  MAIN_CA:289-290  FUS:80,83,128-135  BLD:29-30,164,174; spec SURVEY.md Appendix A).
 * ------------------------------------------------------------------------------------------------------------ */
typedef struct mfvit_vit_cfg {
    int dtype;           /* MFVIT_F32 | MFVIT_BF16 | MFVIT_BF16X3 | MFVIT_F16 : storage / MFMA operand type of activations and weight shadows */
    int batch;           /* images */
    int img_h, img_w;    /* multiples of 16 */
    int dim;             /* 384 (vit_small) */
    int depth;           /* 12 */
    int heads;           /* 12 -> head_dim 32 */
    int mlp_dim;         /* 1536 */
    int save_for_backward; /* 1: keep per-layer activations in the workspace */
    int stop_grad_conv1; /* 1: no gradient for patch_embed.proj.{weight,bias} (MAIN_MOCO:127-128,274) */
    float ln_eps;        /* 1e-6 */
    /* ---- token-input ("GPT") mode: the TransFuser fusion transformer of fuseattention.py:84-212 is the same pre-LN block stack
     * (separate query / key / value Linears = one packed [3 dim][dim] weight, ReLU MLP, LayerNorm eps 1e-5) fed with tokens
     * instead of image patches; mfvit_gpt_forward / mfvit_gpt_backward run it through the encoder's kernels. */
    int token_input;     /* 0: ViT-S/16 (patch embedding + cls token); 1: the input is a (batch, tokens, dim) f32 tensor */
    int tokens;          /* token_input: sequence length (394 = 2 x 197 joint CXR + ENH tokens) */
    int use_pos;         /* token_input: add the learnable pos_emb (args.pos_embed, fuseattention.py:186-189) */
    int act;             /* MLP activation: 0 erf-GELU (timm Block), 1 ReLU (fuseattention.py:67-72) */
    /* ---- token_input, training: the three dropout sites of the GPT (fuseattention.py:33-34,71,112; config.py:40-42 sets 0.1 each).
     * 0 = off (evaluation; ignored in image mode, whose sites are mfvit_vit_drop's).  Masks are counter-based hashes of (seed, site, element index), regenerated by the
     * backward from the same cfg (mfvit_attention_drop_fwd explains the scheme; sites: 1 = embedding, 16 l + 2 = attention of block l,
     * 16 l + 3 = after proj, 16 l + 4 = after the MLP).  The caller draws a fresh seed per forward. */
    float p_embd, p_attn, p_resid;
    uint32_t seed_lo, seed_hi;
    /* ---- launch-geometry hint of THIS call (round 6; ABI 5): how many independent kernel streams run side by side on the GPU while the call's kernels run
     * (the two-stream CA model: 2).  0 = the process-wide default of mfvit_set_stream_share.  Per call and thread-local inside the library: two models in one
     * process no longer share a setting.  Results do not depend on it beyond the summation order of the weight-gradient splits. */
    int stream_share;
} mfvit_vit_cfg;

/* Parameter arena: one contiguous f32 buffer, tensors in timm registration order
 *   cls_token, pos_embed, patch_embed.proj.weight, patch_embed.proj.bias,
 *   blocks.i.{norm1.weight, norm1.bias, attn.qkv.weight, attn.qkv.bias, attn.proj.weight, attn.proj.bias,
 *             norm2.weight, norm2.bias, mlp.fc1.weight, mlp.fc1.bias, mlp.fc2.weight, mlp.fc2.bias} (i = 0..depth-1),
 *   norm.weight, norm.bias          (the classifier `head` is NOT part of the arena: BLD:218-222 replaces it)
 * The gradient arena has the same layout. */
size_t mfvit_vit_param_count(const mfvit_vit_cfg* cfg);
/* offsets (in floats) of: [0] cls_token [1] pos_embed [2] pe.weight [3] pe.bias [4] blocks.0 [5] block stride
 * [6] norm.weight [7] norm.bias [8] total */
int mfvit_vit_param_layout(const mfvit_vit_cfg* cfg, int64_t out[9]);

/* Weight shadow: dtype-typed copies the MFMA kernels read (bf16: W and W^T of every Linear; f32: W^T only).
 * Must be refreshed (mfvit_vit_prepare_shadow) after every parameter update. */
size_t mfvit_vit_shadow_bytes(const mfvit_vit_cfg* cfg);
int mfvit_vit_prepare_shadow(const mfvit_vit_cfg* cfg, const float* params, void* shadow, mfvit_stream_t stream);

size_t mfvit_vit_workspace_bytes(const mfvit_vit_cfg* cfg);

/* features3D(img): (B,3,H,W) f32 NCHW -> tokens (B, 1+HW/256, dim) f32 after the final LayerNorm
 * (replaces patch_embed -> cat(cls) -> +pos_embed -> 12 x Block -> norm; FUS:128,133; crossvit.py:130-146). */
int mfvit_vit_forward(const mfvit_vit_cfg* cfg, const float* params, const void* shadow, const float* img, void* workspace,
                      float* features, mfvit_stream_t stream);

/* Backward of mfvit_vit_forward.  Stages are numbered depth (final norm), depth-1 .. 0 (blocks), -1 (patch embed +
 * cls token); [stage_hi .. stage_lo] are run in descending order so the host can interleave per-block gradient
 * all-reduce with the remaining backward.  dparams is ACCUMULATED into (zero it for a fresh gradient).
 * dfeatures: (B,T,dim) f32, read only when stage_hi == depth. */
int mfvit_vit_backward(const mfvit_vit_cfg* cfg, const float* params, const void* shadow, void* workspace, const float* dfeatures,
                       float* dparams, int stage_hi, int stage_lo, mfvit_stream_t stream);

/* Training-mode regularisation of the image encoder (cfg->token_input = 0): the dropout sites of timm 0.4.9's VisionTransformer that moco-v3's
 * vits.py passes on (drop_rate, attn_drop_rate, drop_path_rate).  Additive in ABI 5: mfvit_vit_cfg and the entry points above are unchanged
 * and run no dropout.  Sites (the mask scheme of mfvit_attention_drop_fwd; keep values scaled by 1 / (1 - p); l = block):
 *    1          pos_drop: x_0 = drop(cat(cls, patch_embed(x)) + pos_embed), cls rows included          rate `drop`      element (row * dim + n)
 *    16 l + 2   attn.attn_drop on the softmax probabilities                                          rate `attn_drop` ((b * H + h) * T + i) * T + j
 *    16 l + 3   attn.proj_drop on the output of proj                                                 rate `drop`      row * dim + n
 *    16 l + 4   the second mlp.drop, on the output of fc2                                            rate `drop`      row * dim + n
 *    16 l + 5   the first mlp.drop, after the GELU (before fc2; folded into the fc1 epilogue)        rate `drop`      row * mlp_dim + n
 *    16 l + 6   drop_path of the attention branch: x + s_b * (branch)                                 drop_path[l]     sample b = row / T
 *    16 l + 7   drop_path of the MLP branch                                                           drop_path[l]     sample b = row / T
 * (sites 1 - 4 are the GPT's numbers for the same places.)  mfvit_dropout_mask(p, seed, site, n) exports the keeps of any site - with
 * n = batch for the drop-path sites.  The backward takes the same struct and rebuilds the same masks; its workspace is
 * mfvit_vit_workspace_bytes_drop (a masked branch needs a scratch row block).  All rates in [0, 1); a rate > 0 needs a 16-bit dtype
 * (MFVIT_F32 gives MFVIT_EINVAL / 0 bytes).  All rates 0 runs the same kernels, with the same results, as mfvit_vit_forward / _backward. */
typedef struct mfvit_vit_drop {
    float drop;               /* pos_drop, attn.proj_drop, both mlp.drop sites */
    float attn_drop;          /* attn.attn_drop */
    const float* drop_path;   /* HOST array of cfg->depth per-block drop-path rates (timm: linspace(0, drop_path_rate, depth)), or NULL */
    uint64_t seed;            /* drawn afresh for every forward by the caller */
} mfvit_vit_drop;
size_t mfvit_vit_workspace_bytes_drop(const mfvit_vit_cfg* cfg, const mfvit_vit_drop* drop);
int mfvit_vit_forward_drop(const mfvit_vit_cfg* cfg, const mfvit_vit_drop* drop, const float* params, const void* shadow, const float* img,
                           void* workspace, float* features, mfvit_stream_t stream);
int mfvit_vit_backward_drop(const mfvit_vit_cfg* cfg, const mfvit_vit_drop* drop, const float* params, const void* shadow, void* workspace,
                            const float* dfeatures, float* dparams, int stage_hi, int stage_lo, mfvit_stream_t stream);

/* Image gradient and data-gradient-only backward of the image encoder (additive in ABI 5).
 * dimg: (B,3,H,W) f32 NCHW, OVERWRITTEN with d loss / d img, or NULL.  It needs image mode (cfg->token_input = 0; the token-input encoder
 *   returns its input gradient through mfvit_gpt_backward) and stage_lo == -1 (the call that runs the embedding stage).  The patch-embedding
 *   data gradient gx[patch rows] W_pe is one tile GEMM whose epilogue stores the image directly (the inverse of im2col: non-overlapping
 *   patches, every element written once, no sum).  W_pe takes part even under stop_grad_conv1.  The workspace must then have
 *   mfvit_vit_workspace_bytes_ex(cfg, drop, 1) bytes (the forward may run on it: its first mfvit_vit_workspace_bytes(_drop) bytes are the
 *   usual layout); the shadow is unchanged.
 * dparams: accumulated into as by mfvit_vit_backward, or NULL: then no parameter gradient of any stage is formed - the data-gradient chain
 *   alone (final LayerNorm, every block's data-gradient GEMMs, attention backward, LayerNorm backwards, dropout / drop-path masks), with no
 *   weight-gradient GEMM, no split-partial reduce, no bias / LayerNorm column sum and no side stream.  Needs dimg.
 * drop: the forward's mfvit_vit_drop, or NULL (no dropout site).  dimg == NULL && dparams != NULL is exactly mfvit_vit_backward(_drop).
 * MFVIT_EINVAL (before any HIP call): dimg in token-input mode, dimg with stage_lo != -1, dimg == dparams == NULL, and the checks of
 * mfvit_vit_backward(_drop).  mfvit_vit_workspace_bytes_ex returns 0 for an invalid cfg / drop, and for want_dimg in token-input mode or
 * without cfg->save_for_backward. */
size_t mfvit_vit_workspace_bytes_ex(const mfvit_vit_cfg* cfg, const mfvit_vit_drop* drop, int want_dimg);
int mfvit_vit_backward_ex(const mfvit_vit_cfg* cfg, const mfvit_vit_drop* drop, const float* params, const void* shadow, void* workspace,
                          const float* dfeatures, float* dparams, float* dimg, int stage_hi, int stage_lo, mfvit_stream_t stream);

/* Patch dropout (additive in ABI 5; mfvit_vit_cfg and mfvit_vit_drop keep their layout): timm >= 0.9 PatchDropout(prob, num_prefix_tokens = 1)
 * - Liu et al. 2022 "PatchDropout", FLIP.  In training mode the blocks run on cls and K = max(1, int(L (1 - prob))) of the L patch rows per image.
 *
 * (1) The image-mode stack on a GIVEN x_0.  cfg: an ordinary image-mode cfg (token_input = 0); params / shadow in the layouts of the full grid (the
 *   arena's pos_embed keeps 1 + gh gw rows, not read here); every activation, the workspace (mfvit_vit_workspace_bytes_x0) and every launch at
 *   `tokens` rows per image, 2 <= tokens <= 1 + gh gw.  x0: (batch, tokens, dim) f32 = cat(cls, kept patch embeddings) + their pos_embed rows; the
 *   forward's embedding stage is one LayerNorm row pass (drop->drop > 0: timm's pos_drop on the shortened rows, site 1), the blocks run exactly as in
 *   image mode, every site of mfvit_vit_drop and the drop path included (per-sample factors: sample = row / tokens).  features: (batch, tokens, dim).
 *   Backward: stages as mfvit_vit_backward; stage -1 forms NO parameter gradient, it writes dx0 (batch, tokens, dim) f32 = d loss / d x0 (required
 *   non-NULL in every call; written by the call with stage_lo == -1).  dparams == NULL: the data-gradient chain alone, as mfvit_vit_backward_ex.
 *   MFVIT_EINVAL before any HIP call (size query: 0) for tokens out of range, a token-input cfg, a cfg mfvit_vit_forward refuses for the full grid
 *   (the fp32 limit on the attention kernels' LDS below among them: a shorter sequence only needs less) or a NULL pointer. */
size_t mfvit_vit_workspace_bytes_x0(const mfvit_vit_cfg* cfg, const mfvit_vit_drop* drop, int tokens);
int mfvit_vit_forward_x0(const mfvit_vit_cfg* cfg, const mfvit_vit_drop* drop, int tokens, const float* params, const void* shadow, const float* x0,
                         void* workspace, float* features, mfvit_stream_t stream);
int mfvit_vit_backward_x0(const mfvit_vit_cfg* cfg, const mfvit_vit_drop* drop, int tokens, const float* params, const void* shadow, void* workspace,
                          const float* dfeatures, float* dparams, float* dx0, int stage_hi, int stage_lo, mfvit_stream_t stream);
/* (2) The front end of timm's PatchDropout: the embedding stage on the kept patches.  idx: (batch, keep) int64 patch indices in [0, L), L = (img_h /
 *   16)(img_w / 16), row-major over the grid, distinct per image (the caller's duty; timm: argsort(randn(B, L))[:, :keep]).
 *   mfvit_patch_keep_embed: the im2col rows of the kept patches only (batch keep x 768, operand type and column order of the encoder's im2col), the patch
 *   GEMM with bias, then x0[b, 1 + k] = row + pos_embed[1 + idx[b, k]] and x0[b, 0] = cls_token + pos_embed[0]; x0 (batch, 1 + keep, dim) f32.  pe_w: the
 *   f32 (dim, 768) weight (cast here).  save != 0: the workspace has mfvit_patch_keep_workspace_bytes(cfg, 1) bytes and keeps what the backward reads.
 *   mfvit_patch_keep_embed_bwd, from dx0 = d loss / d x0, on the forward's workspace: dcls += column sum of the cls rows, dpe_b += column sum of the kept
 *   rows, dpe_w (dim, 768) += dx0[kept]^T patches_kept, each NULL = skipped (stop_grad_conv1; a frozen backbone), and dimg (batch, 3, img_h, img_w) f32
 *   (or NULL) OVERWRITTEN with dx0[kept] W_pe put back through the inverse of the gather: dropped patches are exact zeros.  Every sum runs in a fixed
 *   order without float atomics: the same bits on every run.
 *   err: one int32 on the device, zero before the first call: an index outside [0, L) sets it to 1, its row is zeros and it never becomes an address;
 *   the caller reads the word when it likes.  MFVIT_EINVAL before any HIP call (size query: 0): dtype, batch <= 0, a size no multiple of 16, dim other
 *   than 384 / 768, keep outside [1, L], batch keep 768 >= 2^31, a NULL pointer. */
typedef struct mfvit_patch_keep_cfg {
    int dtype, batch, img_h, img_w, keep, dim;
} mfvit_patch_keep_cfg;
size_t mfvit_patch_keep_workspace_bytes(const mfvit_patch_keep_cfg* cfg, int backward);
int mfvit_patch_keep_embed(const mfvit_patch_keep_cfg* cfg, const float* img, const int64_t* idx, const float* cls_token, const float* pos_embed,
                           const float* pe_w, const float* pe_b, void* workspace, int save, float* x0, int32_t* err, mfvit_stream_t stream);
int mfvit_patch_keep_embed_bwd(const mfvit_patch_keep_cfg* cfg, const int64_t* idx, void* workspace, const float* dx0, float* dcls, float* dpe_w,
                               float* dpe_b, float* dimg, int32_t* err, mfvit_stream_t stream);

/* Block ranges of the image-mode stack (additive in ABI 5): blocks [block_lo, block_hi) of the model on a residual stream of `tokens` rows per
 * image - what token pruning between blocks, early exits and per-stage analysis are built from.  cfg, drop, params, shadow: the whole model's, as
 * for mfvit_vit_forward(_drop); the gradient arena too.  Only the workspace is the range's own (mfvit_vit_workspace_bytes_seg; activations of
 * block_hi - block_lo blocks at `tokens` rows).  The same launchers as the whole-stack entry points, no other kernel: the range [0, depth) with
 * image_in = 1 issues the launches of mfvit_vit_forward(_drop) / mfvit_vit_backward_ex, with image_in = 0 those of mfvit_vit_forward_x0 /
 * mfvit_vit_backward_x0.
 *   x_in   image_in = 1: the (B,3,H,W) f32 image (block_lo == 0 and tokens == 1 + gh gw only).  image_in = 0: x_{block_lo}, (B, tokens, dim) f32;
 *          the range enters through the row pass of mfvit_vit_forward_x0 (norm1 of block block_lo); pos_drop (site 1) applies when block_lo == 0 only.
 *   x_out  (B, tokens, dim) f32: the features behind the final LayerNorm when block_hi == depth, otherwise the raw residual stream x_{block_hi} (the
 *          LayerNorm output its last fc2 epilogue still forms goes to scratch).
 *   Dropout sites keep the model's numbers (16 l + k with l the block's index in the model; sample = row / tokens).
 *   Backward: dx_out = the gradient of whichever x_out was returned.  Stages are the model's numbers: block_hi (the final norm when block_hi ==
 *   depth, otherwise the entry of dx_out, which also adds its column sums to d fc2_b of block block_hi - 1), the blocks block_hi - 1 .. block_lo,
 *   and block_lo - 1: what feeds block block_lo - the embedding stage (image_in = 1: dparams / dimg as mfvit_vit_backward_ex) or dx_in (image_in = 0:
 *   (B, tokens, dim) f32 = d loss / d x_in, required non-NULL in every call, written by the call that runs that stage; no parameter gradient is
 *   formed there).  block_lo - 1 <= stage_lo <= stage_hi <= block_hi.  dparams == NULL: the data-gradient chain alone (image_in = 1: needs dimg).
 *   mfvit_vit_attn_layout_seg: where a forward of the range leaves the qkv tensor and log-sum-exp of its blocks: block l at workspace + out[0] +
 *   (l - block_lo) * out[2] bytes (qkv) and workspace + out[1] + (l - block_lo) * out[2] (lse), in the storage format of tag out[3].  Without
 *   cfg->save_for_backward out[2] = 0: the one copy holds the range's last block.
 * MFVIT_EINVAL before any HIP call (size query: 0): seg NULL, a range outside 0 <= block_lo < block_hi <= depth, tokens outside [2, 1 + gh gw],
 * image_in other than 0 / 1 or set with block_lo != 0 or a shortened sequence, want_dimg with image_in = 0 or without save_for_backward, a stage
 * outside the range's, a token-input cfg, and every check of mfvit_vit_forward_drop / mfvit_vit_backward_ex. */
typedef struct mfvit_vit_seg {
    int block_lo, block_hi;   /* blocks [block_lo, block_hi), 0 <= lo < hi <= cfg->depth */
    int tokens;               /* rows per image in this segment, 2 <= tokens <= 1 + gh gw */
    int image_in;             /* 1: x_in is the (B,3,H,W) image (block_lo == 0 and tokens == 1 + gh gw only); 0: (B,tokens,dim) f32 */
} mfvit_vit_seg;
size_t mfvit_vit_workspace_bytes_seg(const mfvit_vit_cfg* cfg, const mfvit_vit_drop* drop, const mfvit_vit_seg* seg, int want_dimg);
int mfvit_vit_attn_layout_seg(const mfvit_vit_cfg* cfg, const mfvit_vit_drop* drop, const mfvit_vit_seg* seg, int64_t out[4]);
int mfvit_vit_forward_seg(const mfvit_vit_cfg* cfg, const mfvit_vit_drop* drop, const mfvit_vit_seg* seg, const float* params, const void* shadow,
                          const float* x_in, void* workspace, float* x_out, mfvit_stream_t stream);
int mfvit_vit_backward_seg(const mfvit_vit_cfg* cfg, const mfvit_vit_drop* drop, const mfvit_vit_seg* seg, const float* params, const void* shadow,
                           void* workspace, const float* dx_out, float* dparams, float* dx_in, float* dimg, int stage_hi, int stage_lo,
                           mfvit_stream_t stream);

/* Hidden states of the image encoder (host only, additive in ABI 5).  Where the residual stream lies in the workspace after mfvit_vit_forward
 * with save_for_backward = 1: hidden state l (l = 0: cls + patch embedding + pos_embed, the input of block 0; l = 1 .. depth: the output of
 * block l - 1, before the final norm) is f32 [batch * tokens][dim], image-major, at workspace + out[0] + l * out[1] bytes.  f32 in every
 * precision.  MFVIT_EINVAL: invalid cfg, out NULL or save_for_backward == 0. */
int mfvit_vit_hidden_layout(const mfvit_vit_cfg* cfg, int64_t out[2]);

/* Attention state of the image encoder (host only, additive in ABI 5).  Where mfvit_vit_forward with save_for_backward = 1 leaves what
 * mfvit_attention_stats reads: block l's qkv tensor [batch][tokens][3][heads][head_dim] at workspace + out[0] + l * out[2] bytes, in the
 * storage format of tag out[3] (= mfvit_attention_qkv_dtype(cfg->dtype, tokens, head_dim)), and its natural-log log-sum-exp, f32
 * [batch][heads][tokens], at workspace + out[1] + l * out[2] bytes.  MFVIT_EINVAL: invalid cfg, out NULL, save_for_backward == 0 or
 * token-input mode. */
int mfvit_vit_attn_layout(const mfvit_vit_cfg* cfg, int64_t out[4]);

/* Attention maps of the image encoder (additive in ABI 5): an evaluation forward (no dropout site active) that writes the same `features` as
 * mfvit_vit_forward, on a workspace of mfvit_vit_workspace_bytes(cfg) bytes, plus the softmax probabilities of the requested blocks:
 *   P[b][h][i][j] = exp(scale q_i.k_j - lse_i),  scale = head_dim^-1/2,
 * recomputed after each block's attention forward from its qkv tensor and log-sum-exp, i.e. exactly as that forward's softmax normalised
 * them (f32; every row of a per-head map sums to 1).  Heads in timm's order (qkv.reshape(B, T, 3, heads, head_dim)); tokens: cls, then
 * the patches row by row.
 *   blocks    bit l: write block l's map into `maps` (bits at or above cfg->depth are invalid)
 *   fuse      0: per head [B][H][rows][T];  1 / 2 / 3: mean / max / min over the heads [B][rows][T]
 *   cls_only  1: the cls query's row only (rows = 1; the query axis is kept in the layout), 0: all T rows
 *   maps      the selected blocks in ascending order, each block's map contiguous; NULL iff blocks == 0
 *   rollout   NULL, or [B][T-1]: the cls row of the attention rollout (Abnar & Zuidema 2020) over ALL blocks, of the fused maps F_l (fuse
 *             1 - 3; its own full-row maps, whatever cls_only and blocks say):
 *               a_l = diag(c_l) (F_l / 2 + I / 2),  c_l = 1 / (s_l / 2 + 1 / 2),  s_l = the row sums of F_l,  R = a_{depth-1} ... a_0,
 *               rollout = R[0, 1:]  (patch order; not normalised).
 *             The row normalisation c_l matters for max / min fusion only: a mean-fused row sums to 1, a max-fused row to more, a min-fused
 *             row to less.  Needs T <= 8192.
 *   scratch   mfvit_vit_attn_scratch_bytes(cfg, req) bytes: with a rollout the depth fused maps [B][T][T] and their row sums [B][T]
 *             (4 depth B T (T + 1) bytes); 256 bytes otherwise.
 * MFVIT_EINVAL (before any HIP call), and 0 bytes from mfvit_vit_attn_scratch_bytes, for: token-input mode, a `blocks` bit at or above
 * cfg->depth, fuse outside 0 - 3, cls_only other than 0 / 1, a rollout with fuse 0, maps NULL with blocks != 0 (or set with blocks == 0), a
 * request that asks for nothing (blocks == 0, rollout NULL), and the checks of mfvit_vit_forward; mfvit_vit_forward_attn also for scratch
 * NULL.  With no such call the other entry points run exactly the launches they ran before. */
typedef struct mfvit_vit_attn_req {
    uint64_t blocks;   /* bit l: write the probabilities of block l into maps */
    int fuse;          /* 0 per head | 1 mean | 2 max | 3 min over heads */
    int cls_only;      /* 1: query row 0 only */
    float* maps;       /* selected blocks in ascending order, each [B][H or 1][T or 1][T] f32; NULL iff blocks == 0 */
    float* rollout;    /* NULL, or [B][T-1]: cls row of the rollout over all blocks (needs fuse 1..3) */
    void* scratch;     /* mfvit_vit_attn_scratch_bytes(cfg, req) bytes (rollout: the depth fused maps + row sums) */
} mfvit_vit_attn_req;
size_t mfvit_vit_attn_scratch_bytes(const mfvit_vit_cfg* cfg, const mfvit_vit_attn_req* req);
int mfvit_vit_forward_attn(const mfvit_vit_cfg* cfg, const mfvit_vit_attn_req* req, const float* params, const void* shadow,
                           const float* img, void* workspace, float* features, mfvit_stream_t stream);

/* Class-specific attention relevance of the image encoder (additive in ABI 5; Chefer, Gur & Wolf 2021, the self-attention rule).  Reads the
 * workspace of a mfvit_vit_forward with save_for_backward = 1 (no dropout) and runs the data-gradient chain of mfvit_vit_backward_ex(..,
 * dparams = NULL, dimg = NULL) from stage depth down to block 0 - no weight-gradient GEMM, split-partial reduce, column sum, side stream or
 * embedding stage - with one relevance step behind each block's attention backward, while the block's qkv, lse and proj data gradient are live
 * (block 0: the step takes the place of the attention backward, and the chain ends there).  The workspace's backward scratch is overwritten.
 * dfeatures = d y_t / d features (f32 [B][T][dim]; y_t the score of the target class, e.g. head(features[:, 0])[t]).  Per block l:
 *   P_h = softmax(scale q_h k_h^T),  dP_h = d y_t / d P_h = dO_h V_h^T  (dO = d y_t / d (attention output before proj)),
 *   A_l = (1/H) sum_h max(0, P_h o dP_h)  [B][T][T],  heads in timm's order; tokens: cls, then the patches row by row,
 * and R = (I + A_{depth-1}) ... (I + A_0) (Chefer's R = I; R += A_l R for l = 0 .. depth-1), of which the cls row is kept: v = e_0, then
 * v <- v + v A_l for l = depth-1 .. 0, i.e. in the backward's order, in O(B T) scratch.
 *   blocks     bit l: write A_l of block l into `maps` (bits at or above cfg->depth are invalid)
 *   maps       the selected blocks in ascending order, each [B][T][T] f32; NULL iff blocks == 0
 *   relevance  NULL, or [B][T-1] = R[0, 1:] (patch order; not normalised)
 *   scratch    mfvit_vit_rel_scratch_bytes(cfg, req) bytes: with a relevance v [B][T] and the per-32-query-tile row products [B][ceil(T/32)][T]
 *              (4 B T (ceil(T/32) + 1) bytes, whatever the depth); 256 bytes otherwise, never accessed.  No (T, T) map is formed anywhere
 *              for a relevance alone.
 * Evaluation only: every workspace tensor is read as the forward left it; no dropout site, no seed.  No atomics: repeated calls return the same bits.
 * MFVIT_EINVAL (before any HIP call), and 0 bytes from mfvit_vit_rel_scratch_bytes, for: token-input mode, save_for_backward == 0, a `blocks`
 * bit at or above cfg->depth, maps NULL with blocks != 0 (or set with blocks == 0), a request that asks for nothing (blocks == 0, relevance
 * NULL), T > 8192, and the checks of mfvit_vit_forward; mfvit_vit_backward_rel also for scratch or dfeatures NULL.  With no such call the
 * other entry points run exactly the launches they ran before. */
typedef struct mfvit_vit_rel_req {
    uint64_t blocks;    /* bit l: write A_l of block l into maps */
    float* maps;        /* selected blocks ascending, each [B][T][T] f32; NULL iff blocks == 0 */
    float* relevance;   /* NULL, or [B][T-1] = R[0, 1:] */
    void* scratch;      /* mfvit_vit_rel_scratch_bytes(cfg, req) bytes */
} mfvit_vit_rel_req;
size_t mfvit_vit_rel_scratch_bytes(const mfvit_vit_cfg* cfg, const mfvit_vit_rel_req* req);
int mfvit_vit_backward_rel(const mfvit_vit_cfg* cfg, const mfvit_vit_rel_req* req, const float* params, const void* shadow, void* workspace,
                           const float* dfeatures, mfvit_stream_t stream);

/* Low-rank adapters (LoRA, Hu et al. 2021) of the image encoder's Linear weights.  Additive: five new entry points and two structs, nothing
 * existing changes its signature, layout, launches or results, so the ABI number stays 5.
 *
 * An adapted Linear with frozen weight W [N][K] and adapters A [r][K], B [N][r] (f32, dense rows) runs on the MERGED weight
 *   W_eff = W + s B A        (s: the caller's scale, alpha / r or alpha / sqrt(r)),
 * so no forward kernel changes, and its backward is the exact chain rule through W_eff:
 *   dW_eff = dY^T X,   dB = s dW_eff A^T,   dA = s B^T dW_eff.
 *
 * mfvit_lora_merge: out[n][k] = w[n][k] + scale * sum_j b[n][j] a[j][k]   (w: row stride ldw, out: row stride ldo, floats).
 *   All arithmetic f32; acc = fmaf(b[n][j], a[j][k], acc) for j = 0 .. r-1 from acc = 0, then ONE multiply by scale and ONE add to w: the
 *   forward error is at most (r + 2) 2^-24 (|w| + |scale| sum_j |b a|).  An update that is exactly zero (b = 0) returns the bits of w.
 *   out == w (same pointer, same stride) is allowed: the in-place permanent merge.  Any other overlap of out with an input is undefined.
 * mfvit_lora_grad: da[j][k] = scale * sum_n b[n][j] dw[n][k]  ([r][K] dense),  db[n][j] = scale * sum_k dw[n][k] a[j][k]  ([N][r] dense);
 *   dw: row stride lddw.  Outputs are OVERWRITTEN.  Fixed summation orders (da: 16 interleaved row sequences n = i, i + 16, .., added
 *   0 .. 15; db: 64 interleaved sequences of 16-byte pieces, then an xor butterfly), no atomics: repeated calls return the same bits.
 * Domain of both - anything else is MFVIT_EINVAL before any HIP call: every pointer non-NULL; 1 <= r <= 64; N >= 1; K >= 4 and K % 4 == 0;
 *   row strides >= K and multiples of 4; w / dw, a, out / da 16-byte aligned (the kernels move 16 bytes along k). */
int mfvit_lora_merge(const float* w, long ldw, const float* a, const float* b, float scale, float* out, long ldo, int N, int K, int r,
                     mfvit_stream_t stream);
int mfvit_lora_grad(const float* dw, long lddw, const float* a, const float* b, float scale, float* da, float* db, int N, int K, int r,
                    mfvit_stream_t stream);

/* Adapters on the encoder.  Targets: the three row blocks of the fused attn.qkv.weight [3 dim][dim] (q, k, v: each its own A [r][dim],
 * B [dim][r]), attn.proj.weight, mlp.fc1.weight (A [r][dim], B [mlp_dim][r]) and mlp.fc2.weight (A [r][mlp_dim], B [dim][r]). */
#define MFVIT_LORA_Q 0
#define MFVIT_LORA_K 1
#define MFVIT_LORA_V 2
#define MFVIT_LORA_PROJ 3
#define MFVIT_LORA_FC1 4
#define MFVIT_LORA_FC2 5
typedef struct mfvit_lora_item {
    int block;          /* 0 .. cfg->depth - 1 */
    int target;         /* MFVIT_LORA_* */
    const float* a;     /* device, [rank][K] */
    const float* b;     /* device, [N][rank] */
    float* da;          /* device, [rank][K]: overwritten by the backward entries; not read by mfvit_vit_prepare_shadow_lora (may be NULL there) */
    float* db;          /* device, [N][rank]: likewise */
} mfvit_lora_item;
typedef struct mfvit_lora_req {
    int rank;           /* 1 .. 64, one rank for all items */
    float scale;        /* s */
    int n;              /* number of items (HOST array): 1 .. 6 depth, no (block, target) twice */
    const mfvit_lora_item* items;
} mfvit_lora_req;
/* mfvit_vit_prepare_shadow_lora: eff_params (mfvit_vit_param_count floats, must not overlap params) = params with every adapted weight
 *   replaced by its W_eff - one device copy of the arena and one batched merge launch (64 items per launch) - then the weight shadow of
 *   eff_params as mfvit_vit_prepare_shadow builds it.  The forward and backward entry points then take eff_params as `params`: the f32 mode
 *   reads weights from the arena, so the merged weights are what every kernel sees, not only the 16-bit shadows.  Every cfg->dtype is accepted
 *   here; whether a plain 16-bit shadow resolves a small update is the caller's concern (mfvit.lora refuses 'bf16' / 'fp16').
 * mfvit_vit_backward_lora: the data-gradient chain of mfvit_vit_backward_ex(.., dparams = NULL, ..) plus, in every block that has items,
 *   the weight-gradient GEMMs of the adapted Linears ONLY (the fused qkv gradient when any of q / k / v is adapted) - no bias, LayerNorm or
 *   cls column sum, no gradient of a Linear without adapters or of the embedding stage, no side stream.  dW_eff goes through the usual split
 *   partials and their fixed-order reduce into dw_scratch (mfvit_vit_param_count floats in the gradient-arena layout; the call zeroes the slices
 *   it uses, the rest is not touched), then one batched mfvit_lora_grad launch (64 items per launch) overwrites every item's da / db.
 *   params = the eff_params of mfvit_vit_prepare_shadow_lora.  dimg: as in mfvit_vit_backward_ex, or NULL - then stage_lo is raised to the
 *   lowest block with an item, and that block's LN1 data-gradient GEMM, whose result nobody reads, is not launched.  stage_hi = cfg->depth.
 * mfvit_vit_lora_grad: the batched contraction alone, on the adapted dW slices of a gradient arena that mfvit_vit_backward(_ex / _drop)
 *   has filled (adapters beside trainable base parameters: the full backward, then this; correct and slower than the selective entry).
 * MFVIT_EINVAL (before any HIP call): token-input mode; req NULL, n < 1 or an item outside the ranges above, twice, or with a NULL a / b
 *   (da / db: the two backward entries); rank outside 1 .. 64; a NULL eff_params / dw_scratch / dparams; stage_hi != cfg->depth; and the checks of
 *   mfvit_vit_prepare_shadow / mfvit_vit_backward_ex.  With no such call the other entry points run exactly the launches they ran before. */
int mfvit_vit_prepare_shadow_lora(const mfvit_vit_cfg* cfg, const float* params, const mfvit_lora_req* req, float* eff_params, void* shadow,
                                  mfvit_stream_t stream);
int mfvit_vit_backward_lora(const mfvit_vit_cfg* cfg, const mfvit_vit_drop* drop, const float* params, const void* shadow, void* workspace,
                            const float* dfeatures, const mfvit_lora_req* req, float* dw_scratch, float* dimg, int stage_hi, int stage_lo,
                            mfvit_stream_t stream);
int mfvit_vit_lora_grad(const mfvit_vit_cfg* cfg, const mfvit_lora_req* req, const float* dparams, mfvit_stream_t stream);

/* Token-input encoder (cfg->token_input = 1): the GPT of the TransFuser fusion (fuseattention.py:84-212), heads x head_dim with
 * head_dim in {32, 64, 96} (config.py: n_embd 384, n_head 4 -> 96), mlp_dim = block_exp * dim.
 * Parameter arena (f32): pos_emb [tokens][dim], then per block
 *   ln1.weight, ln1.bias, attn.{query,key,value}.weight as one [3 dim][dim] matrix, attn.{query,key,value}.bias [3 dim],
 *   attn.proj.weight, attn.proj.bias, ln2.weight, ln2.bias, mlp.0.weight, mlp.0.bias, mlp.2.weight, mlp.2.bias,
 * then ln_f.weight, ln_f.bias.  (mfvit_vit_param_layout: [0] = [1] = 0 pos_emb, [2] = [3] = first block, no patch embedding.)
 * forward : out = ln_f(blocks(tokens + pos_emb))   (B, tokens, dim) f32            (fuseattention.py:186-192; dropouts are identity)
 * backward: dtokens (B, tokens, dim) f32 = d loss / d tokens; dparams accumulated (pos_emb gradient = sum over the batch).
 * Domain (tests/test_gpt_edges_*.py): tokens >= 1; dim 384 or 768; head_dim 32 / 64 / 96; mlp_dim % 128 == 0; act 0 or 1; every dtype, except
 * that MFVIT_F32 has no head_dim 96, no dropout rate and - its exact attention kernels hold a head's K and V in LDS, the backward two [tokens]
 * vectors more - only 8 tokens head_dim + 8 tokens <= 160 KiB: tokens <= 315 at head_dim 64, <= 620 at head_dim 32.  The same limit holds for
 * T = 1 + patches in image mode.  Outside the domain: MFVIT_EINVAL before any HIP call from every entry point that takes the cfg, 0 from the
 * size queries.  Also MFVIT_EINVAL before any HIP call: a NULL pointer, save_for_backward == 0 in the backward, an image-mode cfg. */
int mfvit_gpt_forward(const mfvit_vit_cfg* cfg, const float* params, const void* shadow, const float* tokens, void* workspace, float* out,
                      mfvit_stream_t stream);
int mfvit_gpt_backward(const mfvit_vit_cfg* cfg, const float* params, const void* shadow, void* workspace, const float* dout, float* dparams,
                       float* dtokens, mfvit_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Single ops (exposed for parity tests and for the MoCo projector / predictor path).
 * ------------------------------------------------------------------------------------------------------------ */
/* y[M][N] = x[M][K] W[N][K]^T + bias   (nn.Linear forward; x, W, y of `dtype`; epilogue 0 bias, 1 bias+GELU(erf)
 * writing gelu'(pre-activation) to y (what the backward needs) and the activation to y2, 3 none, 5 bias with y written as
 * MFVIT_X3F16 (MFVIT_BF16X3 only: the qkv projection feeding mfvit_attention_fwd)).  N % 128 == 0, K % 64 == 0.
 * Epilogue 1: y may be NULL (no-grad forward: the derivative is not computed); for MFVIT_BF16X3 y is PLAIN fp16 [M][N] (ldy in
 * fp16 elements) - the derivative only ever multiplies a gradient, the split copy cost 155 MB of stores per fc1 launch. */
int mfvit_linear_fwd(int dtype, int epilogue, const void* x, int64_t ldx, const void* w, int64_t ldw, const float* bias, void* y,
                     int64_t ldy, void* y2, int64_t ldy2, int M, int N, int K, mfvit_stream_t stream);
/* dx[M][N] = (dy[M][K] Wt[N][K]^T) * act_grad[M][N]   (the fc2 data gradient of timm's Mlp fused with the GELU backward: Wt = W2^T,
 * act_grad = gelu'(pre-activation) as written by mfvit_linear_fwd epilogue 1 - for MFVIT_BF16X3 plain fp16, ldg in fp16 elements).
 * N % 128 == 0, K % 64 == 0 (MFVIT_BF16X3: K % 32 == 0). */
int mfvit_linear_dgrad_act(int dtype, const void* dy, int64_t lddy, const void* wt, int64_t ldwt, const void* act_grad, int64_t ldg,
                           void* dx, int64_t lddx, int M, int N, int K, mfvit_stream_t stream);
/* dW[N][K] (f32, accumulated) += dy[M][N]^T x[M][K]   (nn.Linear weight gradient).  N % 128 == 0, K % 128 == 0. */
int mfvit_linear_wgrad(int dtype, const void* dy, int64_t lddy, const void* x, int64_t ldx, float* dw, int64_t lddw, int M, int N, int K,
                       mfvit_stream_t stream);
/* Same, with caller-owned scratch for the partial sums of the M-splits (MFVIT_WGRAD_SCRATCH_FLOATS floats, may be NULL): the
 * partials then leave the kernel as plain stores and a second small kernel adds them into dW, instead of float atomics. */
#define MFVIT_WGRAD_SCRATCH_FLOATS (384 * 128 * 128)
int mfvit_linear_wgrad_ws(int dtype, const void* dy, int64_t lddy, const void* x, int64_t ldx, float* dw, int64_t lddw, int M, int N,
                          int K, float* scratch, mfvit_stream_t stream);
/* The widest single-launch form (additive): mfvit_linear_wgrad_ws plus
 *   dbias[N] (f32, accumulated; may be NULL) += column sums of dy - the nn.Linear bias gradient, taken from the same operand fragments;
 *   rows_in, rows_out, row_off: reduction row m reads dy row (m / rows_in) * rows_out + m % rows_in + row_off (x is read at row m).  The patch
 *   embedding's weight gradient reads the token rows 1 .. np of every image of a [B][np + 1][D] gradient this way (np, np + 1, 1).  All three 0:
 *   no remap; otherwise rows_in > 0, row_off >= 0 and rows_out >= rows_in + row_off, else MFVIT_EINVAL.
 * Alignment (every weight-gradient entry): dy, x and their row pitches are multiples of 16 bytes (lddy, ldx % 8 == 0 in 16-bit elements, % 4 == 0
 * in f32) - the kernels read 16-byte vectors; anything else returns MFVIT_EINVAL before a launch. */
int mfvit_linear_wgrad_ex(int dtype, const void* dy, int64_t lddy, const void* x, int64_t ldx, float* dw, int64_t lddw, int M, int N, int K,
                          float* scratch, float* dbias, int rows_in, int rows_out, int row_off, mfvit_stream_t stream);
/* Host only, no GPU needed (additive): what a weight-gradient launch of this shape decides before it launches, reported by the launchers' own
 * decision code under the same run-time switches (MFVIT_TN_GLDS, mfvit_set_stream_share).  N2 > 0: the paired launch of mfvit_linear_wgrad_pair
 * with a second gradient of N2 rows (lddy2, ldx2, lddw2: its leading dimensions; MFVIT_ENOSYS where the pair is refused); N2 == 0: a single launch
 * as mfvit_linear_wgrad_ex issues it.  flags: MFVIT_WGRAD_PLAN_* below.  plan[MFVIT_WGRAD_PLAN_INTS]:
 *   [0] kernel: 0 small f32 kernel, 1 register-staged tile kernel, 2 LDS-DMA kernel      [1] reduction rows per stage (0: kernel 0)
 *   [2] splits of the reduction     [3] rows per split (a multiple of [1])                 [4] rows of the last split
 *   [5] 1: tile partials as plain stores through the scratch, 0: float atomics onto dw    [6] 1: bias sums through the rows behind the tile partials,
 *   0: float atomics onto dbias     [7] 128 x 128 output tiles (kernel 1 on split bf16: storage tiles of 64 x 64 logical elements).
 * Returns what the launch would return for a shape outside the domain (MFVIT_EINVAL) and leaves plan untouched then. */
#define MFVIT_WGRAD_PLAN_BIAS 1            /* dbias given ... */
#define MFVIT_WGRAD_PLAN_BIAS_UNALIGNED 2  /* ... at an address that is not a multiple of 16 bytes */
#define MFVIT_WGRAD_PLAN_SCRATCH 4         /* scratch given */
#define MFVIT_WGRAD_PLAN_REMAP 8           /* rows remapped (rows_in > 0) */
#define MFVIT_WGRAD_PLAN_INTS 8
int mfvit_linear_wgrad_plan(int dtype, int M, int N, int K, int N2, int64_t lddy, int64_t ldx, int64_t lddw, int64_t lddy2, int64_t ldx2,
                            int64_t lddw2, int flags, int32_t* plan);
/* TWO weight gradients with the same reduction rows M and the same K in ONE launch (the encoder backward's default for dWqkv + dWproj,
 * the nn.Linear pair of the timm attention block, call sites crossvit_2vits_..._sum.py:128-135):
 *   dw_a[Na][K] += dy_a^T x_a ; dbias_a[Na] += column sums of dy_a (may be NULL) ; dw_b[Nb][K] += dy_b^T x_b.
 * 16-bit dtypes, M >= 2048, Na / Nb / K multiples of 128; anything else returns MFVIT_ENOSYS (the caller then issues two
 * mfvit_linear_wgrad calls). */
int mfvit_linear_wgrad_pair(int dtype, const void* dy_a, int64_t lddy_a, const void* x_a, int64_t ldx_a, float* dw_a, int64_t lddw_a, float* dbias_a,
                            int Na, const void* dy_b, int64_t lddy_b, const void* x_b, int64_t ldx_b, float* dw_b, int64_t lddw_b, int Nb, int M, int K,
                            mfvit_stream_t stream);
/* proj / fc2 (+ residual + following LayerNorm): x_out = a W^T + bias + res ; y = LN(x_out).  N == 384. */
int mfvit_linear_res_ln_fwd(int dtype, const void* a, int64_t lda, const void* w, int64_t ldw, const float* bias, const float* res,
                            int64_t ldres, float* x_out, void* y, int y_f32, const float* gamma, const float* beta, float eps,
                            float* mean, float* rstd, int M, int K, mfvit_stream_t stream);
/* dgrad of a Linear feeding a LayerNorm, fused with the LN backward and the residual-gradient add:
 *   dyln = dy W (W given transposed: wt[N=384][K]) ; dx = LNbwd(dyln; x, mean, rstd, gamma) + dres
 *   column sums (accumulated): dgamma, dbeta, dcol = sum_rows dx.  dx_t (dtype copy of dx) optional. */
int mfvit_linear_dgrad_ln_bwd(int dtype, const void* dy, int64_t lddy, const void* wt, int64_t ldwt, const float* x, const float* mean,
                              const float* rstd, const float* gamma, const float* dres, float* dx, void* dx_t, float* dgamma,
                              float* dbeta, float* dcol, int M, int K, mfvit_stream_t stream);
/* The same two with caller-owned scratch (MFVIT_ROWP_SCRATCH_FLOATS floats, 16-byte aligned; NULL = the calls above): at small M the tall-tile row
 * kernel then splits K over up to 4 workgroups per row tile - each streams its share of W[384][K] through its CU - and the workgroup that arrives last
 * adds the partial tiles from the scratch and runs the epilogue (csrc/gemm_rowp.hip; what the encoder does with its own workspace).  Round 5, additive. */
#define MFVIT_ROWP_SCRATCH_FLOATS (264 * 7 * 12 * 512)
int mfvit_linear_res_ln_fwd_ws(int dtype, const void* a, int64_t lda, const void* w, int64_t ldw, const float* bias, const float* res,
                               int64_t ldres, float* x_out, void* y, int y_f32, const float* gamma, const float* beta, float eps,
                               float* mean, float* rstd, int M, int K, float* scratch, mfvit_stream_t stream);
int mfvit_linear_dgrad_ln_bwd_ws(int dtype, const void* dy, int64_t lddy, const void* wt, int64_t ldwt, const float* x, const float* mean,
                                 const float* rstd, const float* gamma, const float* dres, float* dx, void* dx_t, float* dgamma,
                                 float* dbeta, float* dcol, int M, int K, float* scratch, mfvit_stream_t stream);
/* softmax(q k^T / sqrt(d)) v per (image, head); qkv [B][T][3][H][d], out [B][T][H*d], lse [B][H][T] (module.py:52-64 is the same math for
 * the cross-attention; the self-attention of the timm block: SURVEY Appendix A).  dtype MFVIT_X3F16: qkv split fp16, out / dout / dqkv
 * MFVIT_BF16X3.  mfvit_attention_qkv_dtype: the tag the encoder uses for the qkv tensor of an activation dtype at (T, head_dim) -
 * MFVIT_X3F16 for MFVIT_BF16X3 where the whole-head kernels apply, the dtype itself otherwise. */
int mfvit_attention_qkv_dtype(int dtype, int T, int head_dim);
int mfvit_attention_fwd(int dtype, const void* qkv, void* out, float* lse, int B, int T, int H, int head_dim, mfvit_stream_t stream);
int mfvit_attention_bwd(int dtype, const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv, float* dbias_qkv,
                        int B, int T, int H, int head_dim, mfvit_stream_t stream);
/* Host only, no GPU needed (additive): which kernel family mfvit_attention_fwd (backward == 0) or mfvit_attention_bwd (backward != 0) launches
 * for this dtype tag and shape, reported by the launchers' own decision code under the same run-time switch (MFVIT_ATTN_BWD_SP) and the
 * compute-unit count of the current device (256 where there is none).  plan[MFVIT_ATTN_PLAN_INTS]:
 *   [0] family (MFVIT_ATTN_* below)
 *   [1] 32-row tiles of one (image, head) pair, (T + 31) / 32; 0 for the exact kernels (one row per thread)
 *   [2] dynamic LDS bytes of the launch (streaming backward: of the dQ launch)      [3] workgroups      [4] threads per workgroup
 *   [5] dynamic LDS bytes of the streaming backward's second launch (dK / dV), else 0.
 * The column sums for dbias_qkv are a further launch behind every backward family but the exact one and are not part of the plan.
 * Returns what the launch would return for a refused shape (MFVIT_EINVAL, MFVIT_ENOSYS) and leaves plan untouched then. */
#define MFVIT_ATTN_EXACT 0          /* f32 arithmetic, one row per thread, K / V of a pair as f32 in LDS (csrc/attention.hip) */
#define MFVIT_ATTN_PAIR 1           /* forward, one workgroup per pair, whole head in LDS (attn_fwd_mfma_kernel) */
#define MFVIT_ATTN_FWD_PP 2         /* persistent forward with a producer wave (attn_fwd_pp_kernel; split types, B * H >= 2 x CUs, 5 - 7 tiles) */
#define MFVIT_ATTN_BWD_PADDED 3     /* two-phase backward, padded LDS images (attn_bwd_mfma_kernel<T, RB + 16>) */
#define MFVIT_ATTN_BWD_UNPADDED 4   /* two-phase backward, unpadded LDS images (attn_bwd_mfma_kernel<T, RB>; plain types, T = 417 .. 480) */
#define MFVIT_ATTN_BWD_SP 5         /* single-pass backward (attn_bwd_sp_kernel; 7 tiles, B * H >= 2 x CUs) */
#define MFVIT_ATTN_STREAM 6         /* streaming kernels, any T, head_dim 32 / 64 / 96 (csrc/attention_tiled.hip) */
#define MFVIT_ATTN_PLAN_INTS 6
int mfvit_attention_plan(int dtype, int B, int T, int H, int head_dim, int backward, int32_t* plan);
/* Per-head statistics of the attention probabilities (additive in ABI 5; mfvit.attnstats drives it): mean attention distance (Dosovitskiy et
 * al. 2021, Fig. 11; Raghu et al. 2021) and attention entropy of every head of `nblk` blocks, from each block's qkv tensor (storage tag
 * qkv_dtype: MFVIT_F32 / BF16 / F16 / BF16X3 / X3F16) and log-sum-exp as mfvit_attention_fwd leaves them.  The T x T maps never reach memory.
 *   P_ij = exp(scale q_i.k_j - lse_i), T = 1 + gh * gw tokens: cls, then the patches row by row; patch token i >= 1 at (y_i, x_i) =
 *   divmod(i - 1, gw);  d_ij = patch * sqrtf((float)((y_i-y_j)^2 + (x_i-x_j)^2)), `patch` the patch edge in pixels.
 * stats [nblk][B][H][MFVIT_ATTN_NSTAT], double:
 *   0 distance         (1/(T-1)) sum_{i>=1} sum_{j>=1} P_ij d_ij        (cls row and column dropped, not renormalised)
 *   1 distance_renorm  (1/(T-1)) sum_{i>=1} (sum_{j>=1} P_ij d_ij) / (sum_{j>=1} P_ij)
 *   2 entropy          (1/T) sum_i H(P_i),  H(P_i) = -sum_j P_ij ln P_ij  (nats; all rows, all columns)
 *   3 cls_entropy      H(P_0)
 *   4 cls_mass         (1/(T-1)) sum_{i>=1} P_i0                        (the mass the patches send to cls)
 *   5 self_mass        (1/T) sum_i P_ii
 * With T = 2 the two distances are 0.  ln P is the exponent the kernel holds (times ln 2), never a logarithm.
 * Block l's qkv / lse lie l * qkv_stride / l * lse_stride BYTES behind `qkv` / `lse` (mfvit_vit_attn_layout gives the encoder workspace's).
 * Sums: f32 along a row (a lane over its key tiles, the 32 lanes of a half, the four waves, in that order), double from the rows upward (rows
 * of a 32-query tile in order, tiles in order, then the factor).  No atomics; a (block, image, head) result depends on that head's data only
 * and has the same bits whatever else the call covers.  Two launches (the statistics of all blocks; the tile partials), asynchronous on `stream`.
 * work: mfvit_attention_stats_work_bytes(nblk, B, T, H) bytes (0 for arguments outside the domain), 8-byte aligned.
 * MFVIT_EINVAL before any HIP call: a NULL pointer; nblk, B, H, gh or gw < 1; T != 1 + gh * gw; a stride that is no multiple of 16; qkv not
 * 16-byte aligned; work_bytes too small; a grid (nblk * B * H * ceil(T / 32)) above 2^31 - 1; an unknown tag.  MFVIT_ENOSYS: head_dim other than
 * 32 / 64 / 96. */
#define MFVIT_ATTN_NSTAT 6
size_t mfvit_attention_stats_work_bytes(int nblk, int B, int T, int H);
int mfvit_attention_stats(int qkv_dtype, const void* qkv, const float* lse, int64_t qkv_stride, int64_t lse_stride, int nblk, int B, int T, int H,
                          int head_dim, int gh, int gw, float patch, double* stats, void* work, size_t work_bytes, mfvit_stream_t stream);
/* The same with dropout on the attention probabilities (TransFuser GPT, fuseattention.py:52 `att = self.attn_drop(att)`), streaming kernels
 * (16-bit dtypes; head_dim 32 / 64 / 96; B * H * T * T < 2^32).  The keep mask is a counter-based hash of (seed, site, element index
 * ((b * H + h) * T + i) * T + j) >= p * 2^32, regenerated by the backward - nothing is stored; kept values are scaled by 1 / (1 - p).
 * p = 0 is plain attention.  mfvit_dropout_mask writes the keep bytes (1 / 0) of the first n elements of a site: what the parity tests
 * feed the reference arithmetic with (the reference's own torch RNG stream cannot be reproduced). */
int mfvit_attention_drop_fwd(int dtype, const void* qkv, void* out, float* lse, int B, int T, int H, int head_dim, float p, uint64_t seed,
                             uint32_t site, mfvit_stream_t stream);
int mfvit_attention_drop_bwd(int dtype, const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv, int B, int T, int H,
                             int head_dim, float p, uint64_t seed, uint32_t site, mfvit_stream_t stream);
int mfvit_dropout_mask(float p, uint64_t seed, uint32_t site, int64_t n, uint8_t* keep, mfvit_stream_t stream);
/* LayerNorm over rows of width N in {384, 768} (f32 in; y of dtype or f32). */
int mfvit_layernorm_fwd(int dtype, const float* x, void* y, int y_f32, const float* gamma, const float* beta, float eps, float* mean,
                        float* rstd, int rows, int N, mfvit_stream_t stream);
int mfvit_layernorm_bwd(int dtype, const float* dy, const float* x, const float* mean, const float* rstd, const float* gamma,
                        const float* dres, float* dx, void* dx_t, float* dgamma, float* dbeta, float* dcol, int rows, int N,
                        mfvit_stream_t stream);
/* f32 [R][C] -> dtype [R][C] (dst, optional) and dtype [C][R] (dst_t, optional). */
int mfvit_cast_transpose(int dtype, const float* src, void* dst, void* dst_t, int R, int C, mfvit_stream_t stream);
/* classifier heads with a handful of classes (MAIN_CA:309-310, FUS:105-113): y = x W^T + b over rows x[m*ldx]. */
int mfvit_head_fwd(const float* x, int64_t ldx, const float* w, const float* b, float* y, int64_t ldy, int M, int N, int K, int accumulate,
                   mfvit_stream_t stream);
int mfvit_head_bwd(const float* dy, int64_t lddy, const float* x, int64_t ldx, const float* w, float* dx, int64_t lddx, int dx_accumulate,
                   float* dw, float* db, int M, int N, int K, mfvit_stream_t stream);
/* First maximum.  Wherever this header says "first-maximum argmax" or "as torch.max" (mfvit_cross_entropy, mfvit_cross_entropy_soft,
 * mfvit_eval_counts), the index of a row is torch.max(x, 1)[1] / np.argmax: the first NaN of the row if it holds one, otherwise the first of
 * its largest values (+0.0 and -0.0 are equal).  Rows [1, nan, 3], [nan, 2, 1], [3, 1, nan], [2, 5, 5] give 1, 0, 2, 1. */
/* nn.CrossEntropyLoss (mean) for C <= 64 classes (MAIN_CA:873, MAIN_SS:714): loss_mean[1] (a fixed-order sum: the same bits on every run),
 * dlogits = dloss/dlogits (or NULL), preds = first-maximum argmax (MAIN_CA:870; or NULL).  MFVIT_EINVAL (before any HIP call): C > 64, C < 1. */
int mfvit_cross_entropy(const float* logits, const int64_t* target, float* loss_mean, float* dlogits, int64_t* preds, int B, int C,
                        mfvit_stream_t stream);
/* Soft-target cross entropy (mean) for C <= 64 classes with label smoothing and a mixed target (timm's SoftTargetCrossEntropy over
 * mixup_target; the rest of the DeiT / MoCo-v3 fine-tune recipe next to drop_path_rate):
 *   y_i = lam_i s(t_i) + (1 - lam_i) s(t_partner_i),   s(t) = (1 - smoothing) onehot(t) + smoothing / C,
 *   loss_mean[1] = mean_i( - sum_c y_ic log softmax(logits_i)_c ),   dlogits = (softmax - y) / B (or NULL),
 *   preds = first-maximum argmax (or NULL).
 * partner (device int32 [B], indices into target) and lam (device f32 [B]) come together; both NULL is a plain, possibly smoothed,
 * hard target (smoothing 0: mfvit_cross_entropy's loss).  The [B][C] target matrix is never materialised, and the mean is a
 * fixed-order sum: repeated calls return the same bits.  MFVIT_EINVAL (before any HIP call): exactly one of partner / lam NULL,
 * C > 64, C < 1, B < 1, smoothing outside [0, 1). */
int mfvit_cross_entropy_soft(const float* logits, const int64_t* target, const int32_t* partner, const float* lam, float smoothing,
                             float* loss_mean, float* dlogits, int64_t* preds, int B, int C, mfvit_stream_t stream);

/* Random erasing + Mixup / CutMix of one or two image batches in one launch (timm.data.Mixup after RandomErasing(mode='const');
 * mfvit.mixup builds the tables).  a, out_a f32 [n][C][H][W]; b, out_b the second stream of the same shape (the enhanced twin of the CXR
 * image: same partner, coefficient and boxes), or both NULL.  lam: device f32 [n].
 *   desc : device int32 [n][12]: 0 partner index j in [0, n), 1 mode (0 copy, 1 mixup, 2 cutmix), 2..5 the cut box yl yh xl xh
 *          (half-open, 0 <= yl <= yh <= H, 0 <= xl <= xh <= W), 6 erase flag, 7..10 the erase box eyl eyh exl exh, 11 zero.
 * With E(x_k) = sample k with its OWN erase box filled with 0 (the dataset mean after Normalize; erasing runs in the loader, before the
 * batch is mixed, so the partner is read erased too):
 *   mode 0: out[i] = E(x_i)      mode 1: out[i] = lam_i E(x_i) + (1 - lam_i) E(x_j), one f32 expression per element
 *   mode 2: out[i] = E(x_j) inside the cut box, E(x_i) outside
 * Copy, erase and cutmix elements are moves and zeros (bit-exact).  Box and partner ranges are the caller's contract; reads are clamped to
 * the batch.  Out of place.  MFVIT_EINVAL (before any HIP call): an output overlapping an input or the other output (out_a == a,
 * out_b == b included), exactly one of b / out_b NULL, n, C, H or W <= 0, n > 65535, C * H * W > 2^30. */
int mfvit_batch_mix(const float* a, const float* b, float* out_a, float* out_b, const int32_t* desc, const float* lam, int n, int C, int H,
                    int W, mfvit_stream_t stream);

/* GPU-side input pipeline (replaces the torchvision / Pillow chain of aihc_utils/image_transform.py:50-84 run by
 * the DataLoader workers, moco/loader.py:121-137): Resize((S,S)) or Resize(S) (bilinear; shorter side S, aspect ratio kept) ->
 * horizontal flip -> rotation (nearest, fill 0) -> crop -> ToTensor -> Normalize, fused, bit-exact against Pillow's fixed-point arithmetic.
 *   src    : decoded uint8 HWC (3 channels, channel order as decoded) images of n samples, packed back to back, on the device
 *   desc   : device int64 [n][20]: 0 byte offset in src of the top-left pixel of the source window, 1 in_h, 2 in_w, 3 / 4 offsets (in int32 units) of the x / y
 *            resample tables, 5 / 6 their ksize, 7 flip (0/1), 8 rotation mode (0 none, 1 affine, 2/3/4 = transpose 90/180/270),
 *            9..14 the 16.16 fixed-point affine terms a0 a1 a2 a3 a4 a5 of libImaging's affine_fixed, 15 (crop_i << 32) | crop_j,
 *            16 source row pitch in bytes (3 * image width; a RandomResizedCrop box is a window of the image),
 *            17 the sample's resized frame (Sh << 32) | Sw, or 0 for the square S x S frame, 18..19 zero.
 *            Flip mirrors across Sw, the affine map tests Sw and Sh separately, the transposes 2 / 4 need Sh == Sw, and the crop window
 *            must lie inside the frame.
 *   tables : device int32: per axis one row per pixel of the frame along it (Sw rows for x, Sh rows for y) of
 *            [first source index, tap count, taps[ksize]] (22-bit fixed point)
 *   out    : float32 [n][3][crop][crop]
 * mfvit.input_pipeline builds desc / tables from image sizes and the random draws exactly as Pillow's Python / C code does. */
int mfvit_input_transform(const uint8_t* src, const int64_t* desc, const int32_t* tables, int n, int S, int crop, const float* mean3,
                          const float* std3, float* out, mfvit_stream_t stream);
/* The same transform with an out_h x out_w output window: float32 [n][3][out_h][out_w] (Resize(S) without a crop keeps a
 * non-square frame). */
int mfvit_input_transform_rect(const uint8_t* src, const int64_t* desc, const int32_t* tables, int n, int S, int out_h, int out_w,
                               const float* mean3, const float* std3, float* out, mfvit_stream_t stream);

/* The MoCo-v3 aug1 / aug2 chains (main_covid_mocov3based_single_img_type_5draws_mocov3structure_mocov2loss_vitsmall.py:388-413; blur:
 * moco/loader.py:25-34): RandomResizedCrop -> RandomApply(ColorJitter(0.4, 0.4, 0.2, 0.1)) -> RandomGrayscale -> GaussianBlur ->
 * [Solarize] -> flip -> ToTensor -> Normalize, bit-exact against Pillow (ImageEnhance / ImagingBlend in float32, Image.convert's L and HSV,
 * ImageFilter.GaussianBlur's three extended box passes per axis, ImageOps.solarize at 128).  src, desc, tables, mean3, std3 as for
 * mfvit_input_transform, with rotation mode 0, no crop and a zero slot 17: the geometric stage writes the flipped S x S uint8 frame (the
 * flip commutes with every operation here), and out is float32 [n][3][S][S].
 *   photo : device int32 [n][16], one descriptor per sample, so every sample of a launch may differ:
 *           0 the jitter operations in the order they run, one nibble each from bit 0: 0 none, 1 brightness, 2 contrast, 3 saturation, 4 hue
 *           1 / 2 / 3 the bits of the float32 brightness / contrast / saturation factor (ImageEnhance: 0 + f (v - 0), mean + f (v - mean)
 *             with mean = int(mean(L) + 0.5) over the image as contrast finds it, L + f (v - L))
 *           4 the hue shift int(hue * 255) mod 256 added to the 8-bit H of Pillow's HSV
 *           5 flags: 1 grayscale (L replicated), 2 blur, 4 solarize
 *           6 / 7 / 8 the box blur of one pass: r = (int)fr, ww = (uint32)(2^24 / (2 fr + 1)), fw = (2^24 - (2 r + 1) ww) / 2 with fr
 *             Pillow's float32 _gaussian_blur_radius(sigma, 3);  9..15 zero
 *   max_radius : the largest r of the batch.  The blur tile carries a halo of 3 (r + 1) pixels sized for r <= 1 (sigma <= 2.4494896; the
 *           reference draws sigma from [0.1, 2]): MFVIT_ENOSYS beyond that, before any HIP call.
 *   workspace : mfvit_input_photometric_workspace_bytes(n, S) bytes on the device (the uint8 frames and the per-sample L sums; 0 for an
 *           invalid n / S).  MFVIT_EINVAL: a NULL pointer, n <= 0, n > 65535, S <= 0, S * S > 2^30, max_radius < 0.
 * Four asynchronous operations on `stream` (a memset and three kernels), no host synchronisation. */
size_t mfvit_input_photometric_workspace_bytes(int n, int S);
int mfvit_input_photometric(const uint8_t* src, const int64_t* desc, const int32_t* tables, const int32_t* photo, int n, int S, int max_radius,
                            void* workspace, const float* mean3, const float* std3, float* out, mfvit_stream_t stream);

/* Epoch metrics on the device (replaces the per-batch .cpu() copies MAIN_CA:886-899 and the scikit-learn calls
 * MAIN_CA:901-911).  scores f32 [n][C] (row stride ld), labels int64 [n].  ACCUMULATES into caller-zeroed uint64 arrays:
 * confusion[t][p] (+ optional preds[n] = first-maximum argmax, as torch.max MAIN_CA:870), and per class c the pair counts of the
 * one-vs-rest ROC AUC: u2[c] = 2 #{(pos, neg): s_pos > s_neg} + #{s_pos == s_neg}, npos[c] = #{label == c}; AUC_c = u2 /
 * (2 npos (n - npos)) = the trapezoid area of sklearn's roc_curve.  The pair counts are over THIS call's n samples (call it
 * once on the whole epoch's scores); the confusion matrix may be accumulated batch by batch.  Either half may be NULL (preds is written by
 * the confusion half).  Labels are compared as 64-bit integers: one outside [0, C) is in no row of the confusion matrix and is a negative
 * of every class, as label_binarize makes it. */
int mfvit_eval_counts(const float* scores, int64_t ld, const int64_t* labels, int n, int C, uint64_t* confusion, int64_t* preds,
                      uint64_t* u2, uint64_t* npos, mfvit_stream_t stream);

/* Bootstrap replicates and DeLong components of the epoch metrics (mfvit.evalstats drives them; additive in ABI 5).  They replace the host
 * loop a user puts around MAIN_CA:886-911 / MAIN_SS:797-821 to get an interval for the AUC: R resamples, each three scikit-learn calls or
 * one O(n^2) mfvit_eval_counts.  Here every (model, class) column is ordered once and a replicate costs O(n) per column.
 *
 * scores f32 [M][n][C]: M score sets over the same n samples, row stride ld, model stride model_stride (in floats; unread for M = 1);
 * labels int64 [n], compared in 64 bits.  1 <= n <= 32768, 1 <= C <= 64, 1 <= M <= 8.  Every output element is OVERWRITTEN (no caller
 * zeroing) and all of them are integers: the same bits on every call.
 *   psi2(a, b) = 2 [a > b] + [a == b] as float compares: a NaN on either side gives 0, -0.0 == +0.0 (mfvit_eval_counts' pair rule);
 *   pred_m(i)  = the first maximum of row i of model m (see "First maximum").
 * Replicate r draws n samples with replacement; w_r[i] is how often sample i was drawn.  Replicate 0 is the sample itself (w_0 = 1).  For
 * r >= 1, with lowbias32 the hash of the dropout masks:
 *   key_r = lowbias32(lo32(seed) ^ lowbias32(hi32(seed) + 0x9E3779B9 * (r + 1)));   draw k = 0 .. n - 1 picks (lowbias32(k ^ key_r) * n) >> 32
 * (a 64-bit product).  stratified = 1: order the samples stably by stratum (label 0, 1, .., C - 1, then every label outside [0, C) as one
 * last stratum) into a list L; the draw for position q of L, whose stratum holds n_s samples from off_s on, picks
 * L[off_s + ((lowbias32(q ^ key_r) * n_s) >> 32)]: every stratum keeps its size.  Replicates are absolute: a call computes r = r0 .. r0 + R - 1,
 * so a result does not depend on how the caller chunks R.
 *   conf[r][m][t][p] = sum_i w_r[i] [label_i == t] [pred_m(i) == p]                      (uint64 [R][M][C][C]; outside labels add nothing)
 *   u2[r][m][c]      = sum_{i: label_i == c} sum_{j: label_j != c} w_r[i] w_r[j] psi2(s_m[i][c], s_m[j][c])        (uint64 [R][M][C])
 *   npos[r][c]       = sum_{label_i == c} w_r[i]                                         (uint64 [R][C]);  AUC = u2 / (2 npos (n - npos)).
 * At r = 0 these are mfvit_eval_counts' numbers.  conf may be NULL, or u2 and npos may both be NULL.
 * work: mfvit_boot_work_bytes(n, C, M, R) bytes on the device, 16-byte aligned (0 for an invalid shape or R < 1); its contents before and
 * after a call mean nothing.  MFVIT_EINVAL (before any HIP call): scores, labels or work NULL, n, C or M outside the limits, ld < C,
 * M > 1 with model_stride < (n - 1) ld + C, R < 1, r0 < 0, r0 + R > 2^31, stratified not 0 or 1, work_bytes too small, nothing to compute,
 * only one of u2 / npos. */
size_t mfvit_boot_work_bytes(int n, int C, int M, int64_t R);
int mfvit_boot_counts(const float* scores, int64_t ld, int64_t model_stride, const int64_t* labels, int n, int C, int M, uint64_t seed, int64_t r0,
                      int64_t R, int stratified, void* work, size_t work_bytes, uint64_t* conf, uint64_t* u2, uint64_t* npos, mfvit_stream_t stream);
/* mfvit_delong_counts: the structural components of DeLong, DeLong & Clarke-Pearson (1988) on the sample itself, as integers:
 *   v2[m][c][i] = sum_{j: label_j != c} psi2(s_m[i][c], s_m[j][c])  where label_i == c,
 *                 sum_{j: label_j == c} psi2(s_m[j][c], s_m[i][c])  otherwise                          (int32 [M][C][n]; may be NULL)
 *   pos_xy[c][m][m'] = sum_{label_i == c} v2[m][c][i] v2[m'][c][i];  neg_xy the same sum over the other samples   (uint64 [C][M][M])
 *   u2[m][c] = sum_{label_i == c} v2[m][c][i] (uint64 [M][C]);  npos[c] (uint64 [C]).
 * work: mfvit_boot_work_bytes(n, C, M, 1) bytes.  MFVIT_EINVAL as above, and for a NULL pos_xy, neg_xy, u2 or npos. */
int mfvit_delong_counts(const float* scores, int64_t ld, int64_t model_stride, const int64_t* labels, int n, int C, int M, void* work,
                        size_t work_bytes, int32_t* v2, uint64_t* pos_xy, uint64_t* neg_xy, uint64_t* u2, uint64_t* npos, mfvit_stream_t stream);

/* ROC / precision-recall curves, operating points and calibration of the epoch scores (mfvit.evalstats drives them; additive in ABI 5).  They
 * replace fpr, tpr, thresholds = metrics.roc_curve(...) per class (MAIN_CA:904-907) and the host loops a study puts around it for "sensitivity
 * at 95 % specificity" with an interval.  scores, labels, the limits on n, C, M and the work buffer are mfvit_boot_counts'; every output element
 * is OVERWRITTEN; the counts are integers and every floating sum has a fixed order: the same bits on every call.
 *
 * mfvit_curve_counts: per column (m, c) the distinct score values that are numbers, largest first, one entry per tie group (-0.0 and +0.0 are one
 * group; a float compare decides, denormals keep their order):
 *   thr[m][c][k]  = the group's score, as the FIRST sample of the group in index order holds it (so +0.0 or -0.0, whichever comes first)
 *   tp[m][c][k]   = #{i: label_i == c, s_m[i][c] >= thr},  fp[m][c][k] = #{i: label_i != c, s_m[i][c] >= thr}      (f32, uint32, uint32 [M][C][n])
 *   nthr[m][c]    = the number of valid entries (int32 [M][C]); entries k >= nthr hold thr = NaN, tp = fp = 0
 *   nnan[m][c]    = #{i: s_m[i][c] is NaN} (int32 [M][C]);   npos[c] = #{label_i == c} (uint64 [C]).
 * A NaN score is above no threshold (mfvit_eval_counts' "in no pair" rule) and still counts in npos / n - npos; a label outside [0, C) is a
 * negative of every class.  For a column without NaN, fp, tp and thr are sklearn's _binary_clf_curve (fps, tps, thresholds).
 * work: mfvit_boot_work_bytes(n, C, M, 1) bytes.  MFVIT_EINVAL (before any HIP call): as mfvit_boot_counts for scores, labels, the shape, the
 * strides and work, and for a NULL output.
 *
 * mfvit_boot_points: operating points of the replicates r = r0 .. r0 + R - 1, with mfvit_boot_counts' weights w_r for the same (seed, r,
 * stratified); replicate 0 is the sample itself.  With P_r = sum_{label_i == c} w_r[i] (NaN-scored samples included) and N_r = n - P_r, and for a
 * threshold t: TP_r(t) = sum_{label_i == c, s >= t} w_r[i], FP_r(t) the same over label_i != c (NaN is >= nothing).  The candidate thresholds are
 * the SAMPLE's distinct number scores (the thr of mfvit_curve_counts, whatever the replicate's weights) and one above everything (TP = FP = 0,
 * reported as +inf).  requests: DEVICE int32 [Q][3] = (kind, a, b), 1 <= Q <= 64:
 *   kind 0  the LOWEST candidate with FP_r <= floor(a N_r / b)        (0 <= a <= b, 1 <= b <= 2^20; the product in 64 bits)
 *   kind 1  the HIGHEST candidate with TP_r >= ceil(a P_r / b)        (same a, b).  Positives with NaN scores can put that out of reach of
 *           every candidate; then the lowest candidate is taken (all numbers predicted positive).  Without NaN the lowest always qualifies.
 *   kind 2  a holds the bits of a float tau: the samples with s >= tau as a float compare (NaN tau: none); b is not read.
 *   tp, fp [r][m][c][q] = TP_r, FP_r at the chosen threshold (uint32 [R][M][C][Q]);  thr [r][m][c][q] = the score of the lowest tie group
 *   included, by curve_counts' rule, or +inf when none is (f32);  npos[r][c] = P_r (uint64 [R][C], mfvit_boot_counts' npos).
 * A request whose kind is not 0, 1 or 2, or whose a, b break the bounds, yields tp = fp = 0 and thr = NaN (the requests live on the device and are
 * not inspected on the host).  One workgroup per (replicate, column): both weighted prefixes in one LDS word per place, a request is a bisection.
 * work: mfvit_boot_work_bytes(n, C, M, R) bytes.  MFVIT_EINVAL (before any HIP call): as mfvit_boot_counts for scores, labels, the shape, the
 * strides, work, R, r0 and stratified; Q < 1 or Q > 64; requests or an output NULL.
 *
 * mfvit_calib_sums: calibration of logits f32 [M][n][C] (strides as scores) at Kt temperatures in one launch.  temps: HOST f32 [Kt], each finite
 * and > 0; NB equal-width confidence bins.  Per row, in double from the f32 logits, with beta = 1 / (double)T, mx the row's maximum and
 * d_c = (double)z_c - (double)mx:  den = sum_c exp(beta d_c) (c ascending),  p_c = exp(beta d_c) / den,  top = the first maximum (independent
 * of T),  conf = 1 / den = p_top,  bin = min(NB - 1, max(0, (int)ceil(conf NB) - 1)): the bins (lo, hi] of Guo et al. 2017.
 *   bin_n, bin_hit [m][k][b] = rows in the bin, and those with top == label                           (uint64 [M][Kt][NB])
 *   bin_conf [m][k][b]       = the sum of conf over the bin's rows                                      (f64 [M][Kt][NB])
 *   sums [m][k][0..2]        = sum of -log p_y = log(den) - beta d_y;  sum of the Brier terms sum_c (p_c - [c == y])^2;
 *                              d NLL / d beta = sum of (sum_c p_c d_c - d_y)                            (f64 [M][Kt][3])
 *   skipped [m]              = rows with a non-finite logit or a label outside [0, C): they add nothing anywhere else  (uint64 [M])
 * One workgroup per (model, temperature); every thread adds its rows in index order, then a fixed tree; the bin counters are integer atomics in
 * LDS, the bins' double sums per-thread partials added in thread order (no float atomics).  1 <= Kt <= 16, 1 <= NB <= 64.
 * MFVIT_EINVAL (before any HIP call): a NULL pointer, n, C or M outside the limits, ld < C, M > 1 with model_stride < (n - 1) ld + C, Kt or NB
 * outside their limits, a temperature that is not finite or not > 0. */
int mfvit_curve_counts(const float* scores, int64_t ld, int64_t model_stride, const int64_t* labels, int n, int C, int M, void* work,
                       size_t work_bytes, float* thr, uint32_t* tp, uint32_t* fp, int32_t* nthr, int32_t* nnan, uint64_t* npos, mfvit_stream_t stream);
int mfvit_boot_points(const float* scores, int64_t ld, int64_t model_stride, const int64_t* labels, int n, int C, int M, uint64_t seed, int64_t r0,
                      int64_t R, int stratified, const int32_t* requests, int Q, void* work, size_t work_bytes, uint32_t* tp, uint32_t* fp, float* thr,
                      uint64_t* npos, mfvit_stream_t stream);
int mfvit_calib_sums(const float* logits, int64_t ld, int64_t model_stride, const int64_t* labels, int n, int C, int M, const float* temps, int Kt,
                     int NB, uint64_t* bin_n, uint64_t* bin_hit, double* bin_conf, double* sums, uint64_t* skipped, mfvit_stream_t stream);

/* Minibatch linear CKA (Kornblith et al. 2019; Nguyen, Raghu & Kornblith 2021; mfvit.similarity drives it): centred Gram matrices of a stack of
 * representations, and the HSIC sums between two stacks.  Asynchronous on `stream`; no atomics: repeated calls return the same bits.
 *
 * mfvit_gram_plan (host only): [0] columns per LDS stage  [1] splits of the column range  [2] columns per split (a multiple of [0])
 * [3] columns of the last split.  A function of (n, k) ONLY - not of reps, not of the device's state - so a representation computed in a call
 * with many has the bits of the same representation computed alone.  mfvit_gram_work_bytes: bytes of `work` (0 for an invalid shape).
 *
 * mfvit_gram_centered: g[r][i][j] (double [reps][n][n], overwritten, both triangles, g[r][i][j] and g[r][j][i] the same bits)
 *   = sum_c (x_r[i][c] - m_r[c]) (x_r[j][c] - m_r[c]),   x_r[i][c] = x[r * rep_stride + i * ld + c],  c < k,
 * m_r[c] = the f32 mean of column c over the n rows, summed in a fixed order.  One workgroup per (representation, split) holds all n rows of a
 * column stage in LDS: every element of x is fetched once, the means are taken and subtracted there, and the upper triangle of 32 x 32 tiles is
 * multiplied on v_mfma_f32_32x32x2_f32 (exact f32 products, f32 accumulation within a split).  The splits' partial tiles are added in double, in
 * split order.  Rows >= n and columns >= k contribute exactly zero; nothing outside the n x k views is read.  A NaN in x_r gives NaN in g[r] and
 * nowhere else.  Both HSIC estimators below are exactly invariant to the shift m.
 *
 * mfvit_hsic_accumulate: acc_ab[i][j] += HSIC(ga[i], gb[j]) (double [ra][rb]); acc_aa[i] += HSIC(ga[i], ga[i]); acc_bb[j] += HSIC(gb[j], gb[j]).
 * unbiased = 1 (n >= 4), Kt / Lt = K / L with zeroed diagonals (Song et al. 2012):
 *   HSIC1 = [ sum(Kt o Lt) + (1'Kt1)(1'Lt1) / ((n-1)(n-2)) - 2 / (n-2) * sum_a rowsum(Kt)_a rowsum(Lt)_a ] / (n (n-3))
 * unbiased = 0 (n >= 2):  HSIC0 = tr(K H L H) / (n-1)^2 from the same three sums with the diagonals kept.
 * ga, gb: symmetric double [r][n][n] (the output of mfvit_gram_centered); gb == ga is allowed.  All arithmetic in double, one workgroup per output
 * element, fixed order.
 *
 * Domain - anything else is MFVIT_EINVAL before any HIP call: every pointer non-NULL; 1 <= reps, ra, rb <= 64; 2 <= n <= MFVIT_GRAM_MAX_N
 * (n >= 4 with unbiased); k >= 1 (any k: the tail is masked); ld >= k; ld and rep_stride multiples of 4 and x 16-byte aligned; work_bytes >=
 * mfvit_gram_work_bytes(reps, n, k). */
#define MFVIT_GRAM_MAX_N 256
int mfvit_gram_plan(int n, int64_t k, int32_t plan[4]);
size_t mfvit_gram_work_bytes(int reps, int n, int64_t k);
int mfvit_gram_centered(const float* x, int64_t rep_stride, int64_t ld, int reps, int n, int64_t k, double* g, void* work, size_t work_bytes,
                        mfvit_stream_t stream);
int mfvit_hsic_accumulate(const double* ga, int ra, const double* gb, int rb, int n, int unbiased, double* acc_ab, double* acc_aa, double* acc_bb,
                          mfvit_stream_t stream);

/* The perturbation test for patch-relevance maps (Chefer, Gur & Wolf 2021 section 4, positive / negative perturbation; Petsiuk et al. 2018,
 * deletion / insertion; mfvit.perturb drives it): rank the patches, mask them a fraction at a time, score the model's output again.  Three
 * launches, one each, asynchronous on `stream`.
 *
 * mfvit_patch_rank: rel f32 [B][P] (row stride ld) -> rank int32 [B][P], the position of patch i when the patches of image b are ordered
 * most relevant first, by a total order that depends on the values and the indices only:
 *   rank[i] = #{j : rel[j] > rel[i], or rel[j] == rel[i] and j < i}.
 * NaN counts as below every number, -inf included, NaNs among themselves by index; -0.0 == +0.0 is a tie.  That is the inverse permutation
 * of np.argsort(-rel, kind="stable") - NOT of torch.argsort(descending=True, stable=True), which puts NaN first.  Exact (integers).
 * P <= 8192, the token limit.  MFVIT_EINVAL (before any HIP call): a NULL pointer, B <= 0, B > 65535, P <= 0, P > 8192, ld < P. */
int mfvit_patch_rank(const float* rel, int64_t ld, int32_t* rank, int B, int P, mfvit_stream_t stream);
/* mfvit_patch_perturb: img f32 [B][C][H][W], rank int32 [B][P] with P = (H / 16) (W / 16), patches row by row as the encoder numbers its
 * tokens, steps device int32 [S][2] (half-open rank ranges lo_s, hi_s), fill device f32 [C] -> out f32 [S][B][C][H][W]:
 *   out[s][b][c][y][x] = fill[c] if lo_s <= rank[b][(y / 16) (W / 16) + x / 16] < hi_s, else img[b][c][y][x].
 * Every element is a move or the fill value (bit-exact).  With k patches to remove: positive perturbation (most relevant first) is
 * [0, k), negative (least relevant first) [P - k, P), insertion (only the top k visible) [k, P).  The range values (0 <= lo <= hi <= P)
 * and the rank values are the caller's contract; they only enter comparisons.  Out of place.  MFVIT_EINVAL (before any HIP call): a NULL
 * pointer, H or W not a positive multiple of 16, P > 8192, B, C or S <= 0, B > 65535, S > 65535, C * H * W > 2^30, out overlapping img. */
int mfvit_patch_perturb(const float* img, const int32_t* rank, const int32_t* steps, const float* fill, float* out, int B, int C, int H,
                        int W, int S, mfvit_stream_t stream);
/* mfvit_perturb_score: logits f32 [S][B][C] (row stride ld, row s * B + b), target int64 [B].  ACCUMULATES into caller-zeroed correct
 * uint64 [S], sums f64 [S][2] and nonfinite uint64 [S]: per step the number of images whose first-maximum argmax (as torch.max, like
 * mfvit_eval_counts) equals the target, the sum of the target's softmax probability (computed in double from the f32 logits,
 * max-subtracted) in sums[s][0] and the sum of the target's raw logit in sums[s][1].  A row with a non-finite logit counts as wrong, adds 0
 * to both sums and 1 to nonfinite[s].  One workgroup per step and a fixed-order sum (every thread walks its images in index order, then a
 * fixed tree): called batch after batch, it gives the same bits on every run.  A target outside [0, C) is the caller's contract (such a
 * row is wrong and adds 0; nothing outside the row is read).  MFVIT_EINVAL (before any HIP call): a NULL pointer, S, B or C <= 0, ld < C. */
int mfvit_perturb_score(const float* logits, int64_t ld, const int64_t* target, int S, int B, int C, uint64_t* correct, double* sums,
                        uint64_t* nonfinite, mfvit_stream_t stream);

/* Gradient attribution (integrated gradients, SmoothGrad, saliency; mfvit.attribution drives it; additive in ABI 5): everything around the
 * model's forward and its data-gradient-only backward (mfvit_vit_backward_ex with dparams = NULL).  Three launches, one each, asynchronous on
 * `stream`; no atomics, every sum in a fixed order: the same bits on every run.  16-byte accesses where every image pointer is 16-byte
 * aligned (and hw % 4 == 0), a scalar path otherwise.
 *
 * mfvit_attr_inputs: x f32 [B][C][hw]; base f32 [C] (base_full = 0: one constant per channel) or [B][C][hw] (base_full = 1); alpha device
 * f32 [S]; sigma device f32 [B] or NULL; seed device uint64 [1] (read only when sigma is given) -> out f32 [S][B][C][hw]:
 *   v = base                               where alpha_s == 0          (a move: bit-exact)
 *   v = x                                  where alpha_s == 1          (a move: bit-exact)
 *   v = fmaf(alpha_s, x - base, base)      otherwise (the difference rounded to f32 first)
 *   out[s][b][e] = v, or fmaf(sigma_b, z, v) when sigma is given, e the element index inside the image.
 * z is a standard normal from a counter hash of (seed, gs = s0 + s, b, e); nothing is stored.  With lowbias32 the multiply-xorshift hash of
 * the dropout masks (x ^= x >> 16, x *= 0x7feb352d, x ^= x >> 15, x *= 0x846ca68b, x ^= x >> 16) and lowbias32b the same form with the
 * constants 0x21f0aaad, 0x735a2d97 and a last shift of 15:
 *   k   = lowbias32(lo32(seed) ^ lowbias32(hi32(seed) + 0x9E3779B9 * (gs + 1)));   key = lowbias32(k + 0x85EBCA6B * (b + 1))
 *   h1  = lowbias32(e ^ key);   h2 = lowbias32b(e ^ key)
 *   u1  = ((float)(h1 >> 8) + 0.5f) * 2^-24   (f32 arithmetic: in (0, 1], never 0);   u2 = (float)(h2 >> 8) * 2^-24   (in [0, 1))
 *   z   = sqrtf(-2 logf(u1)) * cospif(2 u2)   (the accurate device functions; every product rounded to f32).
 * s0 is the global index of the call's first sample: the noise of sample gs is the same however the samples are grouped into calls.
 * x = 0, base = 0, alpha = 1, sigma = 1 exports z itself.  Out of place.  MFVIT_EINVAL (before any HIP call): x, base, alpha or out NULL,
 * sigma without seed, S, B, C or hw <= 0, S > 65535, B > 65535, s0 < 0 or > 2^30, C * hw > 2^30, out overlapping x or a full base. */
int mfvit_attr_inputs(const float* x, const float* base, int base_full, const float* alpha, const float* sigma, const uint64_t* seed, int s0,
                      float* out, int S, int B, int C, int64_t hw, mfvit_stream_t stream);
/* mfvit_attr_accumulate: g f32 [k][B][n] (the image gradients of the group just run), w device f32 [k], acc f32 [B][n], zeroed by the caller
 * before the first group:  acc[b][i] += sum_s w_s g[s][b][i]^power, s ascending, one rounding per step: power 1 is a = fmaf(w_s, g, a);
 * power 2 is a = (float)fma(w_s g, g, a) evaluated in double, where w_s g is exact, so that the square enters unrounded.
 * MFVIT_EINVAL (before any HIP call): a NULL pointer, k, B or n <= 0, k > 65535, B > 65535, n > 2^30, power not 1 or 2, acc overlapping g. */
int mfvit_attr_accumulate(const float* g, const float* w, float* acc, int k, int B, int64_t n, int power, mfvit_stream_t stream);
/* mfvit_attr_finish: acc f32 [B][C][H][W]; with times_input x f32 [B][C][H][W] and base as in mfvit_attr_inputs (both unread otherwise) ->
 * pixels f32 [B][H][W] (or NULL), patches f32 [B][H / 16][W / 16], total f64 [B], all OVERWRITTEN:
 *   t_c    = acc_c * (x_c - base_c) (the difference, then the product, each rounded to f32), or acc_c without times_input
 *   pixel  = f(t_0) + f(t_1) + ..  in channel order, f the identity or fabsf (absval)
 *   patch  = the 256 pixels of a 16 x 16 patch: groups of four pixels of a row (a0 + a1) + (a2 + a3), the four groups of a patch row
 *            (q0 + q1) + (q2 + q3), then the 16 rows pairwise, ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)) plus the same of r8 .. r15:
 *            eight additions deep
 *   total  = the sum of the SIGNED t_c of the image (also with absval) in double: per thread in visiting order, then a fixed tree.
 * One workgroup per image: no output has two writers.  MFVIT_EINVAL (before any HIP call): acc, patches or total NULL, times_input without
 * x or base, H or W not a positive multiple of 16, B or C <= 0, C * H * W > 2^30, pixels overlapping an input. */
int mfvit_attr_finish(const float* acc, const float* x, const float* base, int base_full, int times_input, int absval, float* pixels,
                      float* patches, double* total, int B, int C, int H, int W, mfvit_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Two-stream fusion: bidirectional cls<->patch cross-attention exchange + heads (f32).
 * Replaces PreNorm / CrossAttention (MOD:15-21,108-137), MultiScaleTransformerEncoder.forward (FUS:35-65) and
 * Fus_CrossViT.forward (FUS:126-157).  dim 384 or 768 (vit_small / vit_base), heads 3, 6 or 12 (head_dim = dim / heads); any other
 * value gives MFVIT_EINVAL / 0 bytes.  mfvit_fusion_* run one exchange layer with pool='cls'; the mfvit_fusion_ex_* entry points below
 * add cross_attn_depth and pool='mean'.
 * Ranges: batch >= 1 (no upper limit), num_classes 1 .. 64, tokens 2 .. T_max(dim, heads).  T_max is set by the 160 KB of LDS a streaming
 * pass may request - per (sample, direction) the rows' statistics, scores and score gradients of all heads stay in LDS:
 *   backward          32 T + 160 dim bytes                                     (every head count)
 *   token gradient    4 (max(2 heads dim + 2 heads T, 16 dim) + 2 T) bytes     (heads 6 and 12 only)
 *   T_max:  dim 384: heads 3: 3200, 6: 2596, 12: 1220        dim 768: heads 3: 1280, 6: 1280, 12: 866
 * (vit_base at 384 x 384 pixels, tokens 577, fits at every head count.)  A larger token count is refused like any other value outside the
 * ranges: MFVIT_EINVAL before any HIP call from every entry point of this section, 0 from the *_param_count / *_workspace_bytes queries.
 * ------------------------------------------------------------------------------------------------------------ */
typedef struct mfvit_fusion_cfg {
    int batch;        /* >= 1 */
    int tokens;       /* 1 + patches (197 at 224^2): 2 .. T_max(dim, heads), see above */
    int dim;          /* 384 or 768 */
    int heads;        /* 3 (FUS:75), 6 or 12 -> head_dim = dim / heads */
    int num_classes;  /* 1 .. 64 (3 in the reference) */
    float eps_pre;    /* 1e-5: PreNorm's nn.LayerNorm default (MOD:18) */
    float eps_post;   /* 1e-6: FUS:26,31 */
} mfvit_fusion_cfg;

/* Parameter arena (f32), state-dict order of Fus_CrossViT (22 tensors, 8 D^2 + 10 D + 2 (C D + C) floats):
 *   cross_attn_layers.0.{0.norm.{weight,bias}, 0.fn.{wq,wk,wv}.weight, 0.fn.proj.{weight,bias}, 1.{weight,bias},
 *                        2.norm.{weight,bias}, 2.fn.{wq,wk,wv}.weight, 2.fn.proj.{weight,bias}, 3.{weight,bias}},
 *   mlp_head_cxr.0.{weight,bias}, mlp_head_enh.0.{weight,bias}.   The gradient arena has the same layout. */
size_t mfvit_fusion_param_count(const mfvit_fusion_cfg* cfg);
size_t mfvit_fusion_workspace_bytes(const mfvit_fusion_cfg* cfg);
/* f_cxr / f_enh: (B,T,dim) f32 tokens (features3D of each stream).  hw_* / hb_*: the backbones' own classifier heads
 * (C x dim, C) or NULL; when given, x_cxr / x_enh = head(f[:,0]) (FUS:131,135).  fused: (B,C) (FUS:147-155).
 * The workspace keeps what the backward needs. */
int mfvit_fusion_forward(const mfvit_fusion_cfg* cfg, const float* params, const float* f_cxr, const float* f_enh, const float* hw_cxr,
                         const float* hb_cxr, const float* hw_enh, const float* hb_enh, void* workspace, float* fused, float* x_cxr,
                         float* x_enh, mfvit_stream_t stream);
/* dparams, dhw_*, dhb_* are ACCUMULATED into.  df_cxr / df_enh: (B,T,dim) fully written, or both NULL when the
 * backbones are frozen (README default, MAIN_CA:298-305). */
int mfvit_fusion_backward(const mfvit_fusion_cfg* cfg, const float* params, const float* f_cxr, const float* f_enh, const float* hw_cxr,
                          const float* hw_enh, void* workspace, const float* dfused, const float* dx_cxr, const float* dx_enh,
                          float* dparams, float* df_cxr, float* df_enh, float* dhw_cxr, float* dhb_cxr, float* dhw_enh, float* dhb_enh,
                          mfvit_stream_t stream);

/* Fus_CrossViT with cross_attn_depth = L (1 .. 16) chained exchange layers and pool_mean = 0 ('cls') or 1 ('mean').
 * Parameter arena: the L layer blocks of ONE MultiScaleTransformerEncoder (each laid out as cross_attn_layers.0 above, 8 D^2 + 10 D
 * floats) followed by the two heads - L (8 D^2 + 10 D) + 2 (C D + C) floats.  In Fus_CrossViT's named_parameters() order this is the
 * contiguous tail of its arena when the LAST of its multi_scale_enc_depth encoders is passed: every encoder reads the backbone features
 * and only the last one's output is used (FUS:137-139), so the earlier ones have no effect and are not passed.
 * Layer l (FUS:40-63) reads X_l (X_0 = the features) and outputs, per stream, X_{l+1} = LN_1e-6([cls_l + CA(LN_1e-5([cls_l ; other
 * stream's patches of X_l])) ; own patches of X_l]) over ALL rows; both directions of a layer read the layer's input.
 * Pooling (FUS:141-145): 'cls' pools row 0 of X_0 + X_L, 'mean' averages all T rows of X_0 + X_L; x_cxr / x_enh stay on row 0 of X_0.
 * L = 1 with 'cls' is exactly mfvit_fusion_forward / _backward (same bits, same workspace).  Otherwise every layer's (2, B, T, dim)
 * output rows are kept in the workspace for the backward.  Arguments and accumulation rules as mfvit_fusion_forward / _backward;
 * every sum is taken in a fixed order. */
size_t mfvit_fusion_ex_param_count(const mfvit_fusion_cfg* cfg, int cross_attn_depth, int pool_mean);
size_t mfvit_fusion_ex_workspace_bytes(const mfvit_fusion_cfg* cfg, int cross_attn_depth, int pool_mean);
int mfvit_fusion_ex_forward(const mfvit_fusion_cfg* cfg, int cross_attn_depth, int pool_mean, const float* params, const float* f_cxr,
                            const float* f_enh, const float* hw_cxr, const float* hb_cxr, const float* hw_enh, const float* hb_enh,
                            void* workspace, float* fused, float* x_cxr, float* x_enh, mfvit_stream_t stream);
int mfvit_fusion_ex_backward(const mfvit_fusion_cfg* cfg, int cross_attn_depth, int pool_mean, const float* params, const float* f_cxr,
                             const float* f_enh, const float* hw_cxr, const float* hw_enh, void* workspace, const float* dfused,
                             const float* dx_cxr, const float* dx_enh, float* dparams, float* df_cxr, float* df_enh, float* dhw_cxr,
                             float* dhb_cxr, float* dhw_enh, float* dhb_enh, mfvit_stream_t stream);

/* Attention maps of the exchange (additive in ABI 5).  In exchange layer `layer` (0 .. cross_attn_depth - 1) the cls token of one stream is the
 * only query; its keys are row j = 0: its own pre-normed cls token, rows j = 1 .. T-1: the OTHER stream's pre-normed patch tokens of the layer's
 * input, row by row.  Direction d = 0 is the CXR cls query (block [0], reads ENH patches), d = 1 the ENH cls query (block [2], reads CXR patches);
 * heads in the order of the rows of wq / wk / wv.
 *
 * mfvit_fusion_ex_attention, after a mfvit_fusion_ex_forward (or mfvit_fusion_forward: depth 1, pool_mean 0) with the same cfg / depth / pool on
 * `workspace`: the softmax probabilities a^d_h[j] exactly as that forward normalised them (one copy kernel, nothing is recomputed).
 *   fuse  0: out [2][B][heads][T] (every row sums to 1);  1 / 2 / 3: mean / max / min over ALL heads, out [2][B][T].  max / min are not
 *         renormalised: a max-fused row sums to more than 1, a min-fused row to less.
 *
 * mfvit_fusion_ex_grad_attention, after a mfvit_fusion_ex_backward (or mfvit_fusion_backward) on that workspace, with the params / f_cxr / f_enh
 * of the forward: the gradient-weighted map of the score y the backward differentiated (dfused, dx_* = d y / d outputs),
 *   da^d_h[j] = d y / d a^d_h[j] = z_j . du^d_h,    abar[d][b][j] = (1 / heads) sum_h max(0, a^d_h[j] da^d_h[j]),    abar [2][B][T],
 * z_j the pre-normed key row (re-derived from the layer's input rows and the row statistics of the forward), du = d y / d u_h as the backward left
 * it; the heads are summed in head order (in one workgroup per (sample, direction), also across the chunks of 3 heads the exchange runs in).
 * What it reads of the workspace - the probabilities, the row statistics and du - is written by the forward, or by the backward's du GEMM, and by
 * nothing after: mfvit_fusion_ex_backward leaves all three intact, and both calls may be repeated.  Neither call writes the workspace.
 * No atomics: repeated calls return the same bits.
 * MFVIT_EINVAL (before any HIP call): a NULL pointer, layer outside 0 .. cross_attn_depth - 1, fuse outside 0 - 3, T > 8192, and the checks of
 * mfvit_fusion_ex_forward.  With no such call the other entry points run exactly the launches they ran before. */
int mfvit_fusion_ex_attention(const mfvit_fusion_cfg* cfg, int cross_attn_depth, int pool_mean, const void* workspace, int layer, int fuse,
                              float* out, mfvit_stream_t stream);
int mfvit_fusion_ex_grad_attention(const mfvit_fusion_cfg* cfg, int cross_attn_depth, int pool_mean, const float* params, const float* f_cxr,
                                   const float* f_enh, const void* workspace, int layer, float* abar, mfvit_stream_t stream);

/* Cross-stream relevance of a two-stream model with ONE exchange layer and cls pooling (additive in ABI 5; Chefer, Gur & Wolf 2021, the
 * self-attention rule inside each encoder, the co-attention rule across the exchange), all for the same score y.  Per image and stream s in
 * {c (cxr), e (enh)}, with A^s_l the encoder's relevance maps (mfvit_vit_backward_rel, every block: maps_s [depth_s][B][T][T]) and abar as above:
 *   R_s = (I + A^s_{L-1}) ... (I + A^s_0),  r_s = R_s[0, :],  n_s = R_s 1 - 1,
 *   Rbar_s[j, :] = (R_s[j, :] - e_j) / n_s[j] + e_j   (e_j where n_s[j] <= 0),
 *   direction 0:  w = (0, abar[0][1:]),  what[j] = w[j] / n_e[j]  (0 where n_e[j] <= 0),
 *     rel_cc = (1 + abar[0][0]) r_c[1:]                             cxr cls -> cxr patches
 *     rel_ce = Rbar_c[0,0] (what R_e - what + w)[1:]                cxr cls -> enh patches (= Rbar_c[0,0] w Rbar_e)
 *   direction 1, symmetric: rel_ee, rel_ec.
 *   out4 [4][B][T-1] = rel_cc | rel_ce | rel_ec | rel_ee  (patch order; not normalised).  The CXR image's total is rel_cc + rel_ec, the ENH
 *   image's rel_ee + rel_ce.
 * One workgroup per (image, stream), its vectors in LDS (T <= 8192): n_s as a column chain over blocks 0 .. L-1, then r_s and what R_s as two
 * row chains over blocks L-1 .. 0 in one read of the maps; a second, elementwise launch applies the other stream's Rbar[0,0].  Every vector is
 * carried as its difference from the chain's start, so n_s and r_s[0] - 1 are sums of non-negative terms.  The maps are read twice
 * (8 (depth_c + depth_e) B T^2 bytes of traffic).
 *   scratch  mfvit_bimodal_relevance_scratch_bytes(B, T) bytes (the two streams' Rbar[0,0], [2][B])
 * No atomics: repeated calls return the same bits.  MFVIT_EINVAL (before any HIP call), and 0 bytes of scratch, for B <= 0, T < 2, T > 8192;
 * mfvit_bimodal_relevance also for a depth <= 0 or a NULL pointer. */
size_t mfvit_bimodal_relevance_scratch_bytes(int B, int T);
int mfvit_bimodal_relevance(int B, int T, int depth_c, int depth_e, const float* maps_c, const float* maps_e, const float* abar, float* out4,
                            void* scratch, mfvit_stream_t stream);

/* Stand-alone PreNorm(CrossAttention) (MOD:15-21,108-137): out[b] = proj(attn(LN_1e-5([x_own[b,0] ; x_oth[b,1:]]))) -> (B, dim).
 * params = one block [norm.weight, norm.bias, fn.wq.weight, fn.wk.weight, fn.wv.weight, fn.proj.weight, fn.proj.bias]
 * (4 D^2 + 3 D floats).  x_own == x_oth reproduces PreNorm(dim, CrossAttention(...))(x) exactly.  cfg: batch, tokens, dim,
 * heads, eps_pre; workspace of mfvit_fusion_workspace_bytes(cfg).  Backward: dparams accumulated; dx_own receives row 0 only,
 * dx_oth rows 1.. only (the caller zero-fills both), or both NULL. */
int mfvit_prenorm_xattn_forward(const mfvit_fusion_cfg* cfg, const float* params, const float* x_own, const float* x_oth,
                                void* workspace, float* out, mfvit_stream_t stream);
int mfvit_prenorm_xattn_backward(const mfvit_fusion_cfg* cfg, const float* params, const float* x_own, const float* x_oth,
                                 void* workspace, const float* dout, float* dparams, float* dx_own, float* dx_oth,
                                 mfvit_stream_t stream);

/* Bare CrossAttention (MOD:123-137 without the PreNorm; the reference's live path never calls it that way, FUS:25,30):
 * out[b] = proj(attn(q = wq x[b,0], k / v = wk / wv x[b,:])) -> (B, dim).  params = [wq.weight, wk.weight, wv.weight, proj.weight,
 * proj.bias] (4 D^2 + D floats); cfg / workspace as above (eps_pre unused).  Backward: dparams accumulated, dx (B,T,dim) fully
 * written (zero-filled by the caller, or NULL). */
int mfvit_xattn_forward(const mfvit_fusion_cfg* cfg, const float* params, const float* x, void* workspace, float* out,
                        mfvit_stream_t stream);
int mfvit_xattn_backward(const mfvit_fusion_cfg* cfg, const float* params, const float* x, void* workspace, const float* dout,
                         float* dparams, float* dx, mfvit_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Opt-in kernel timing (HIP events on the launch stream), used by bench.py for the roofline of the dominant kernel.
 * Classes: 0 gemm_nt_tile 1 gemm_nt_row_res_ln 2 gemm_nt_row_lnbwd 3 gemm_tn_wgrad 4 attention_fwd 5 attention_bwd
 *          6 xattn_stream_fwd 7 xattn_stream_bwd 8 infonce 9 other.
 * mfvit_prof_collect waits for the recorded events and fills out[cls*4 + {0 launches, 1 ms, 2 algorithmic flops,
 * 3 algorithmic bytes}] (ncls <= 10), then clears the records. */
int mfvit_prof_enable(int class_mask); /* bit c set = time class c; 0 = off */
/* Weight-gradient GEMMs of mfvit_vit_backward run on a library-owned side stream beside the dgrad chain (default on: at 1,024 ... 4,096
 * token rows).  0 serialises them on the caller's stream - used by bench.py's attribution pass so that a kernel's
 * event-timed duration is its own, not a share of a co-scheduled GPU.  Results are identical either way. */
int mfvit_set_wgrad_stream(int enabled);
/* How many independent kernel streams the caller runs side by side on this GPU (default 1: a kernel may size its grid for the whole chip).  The
 * two-stream CA model sets 2 (both encoders at once, crossvit_2vits_..._sum.py:128-135 are independent): for SMALL problems the
 * one-workgroup-per-CU kernels (row-complete GEMMs, weight gradients) then launch about half as many, longer workgroups, and the two encoders'
 * kernels run beside each other.  A hint only: results do not depend on it beyond the summation order of the weight-gradient splits. */
int mfvit_set_stream_share(int n);
int mfvit_prof_collect(double* out, int ncls);
/* Sub-attribution of the records the last mfvit_prof_collect call consumed: out[tag*3 + {0 launches, 1 ms, 2 algorithmic flops}] for tag 1 = the qkv
 * projections and tag 2 = the output projections (+ residual + LayerNorm) of the encoder FORWARD - with class attention_fwd the three parts of the
 * fused multi-head self-attention figure BASELINE.json's metric names (Attention.forward, moco_pretraining/moco/model/module.py:52-64). */
int mfvit_prof_collect_tags(double* out, int ntags);
const char* mfvit_prof_class_name(int cls);

/* ------------------------------------------------------------------------------------------------------------
 * MoCo step pieces (BLD = moco/builder_vit_mocov3structure_mocov2loss.py).  The Linear layers of the projector /
 * predictor run on mfvit_linear_fwd / mfvit_linear_wgrad.
 * ------------------------------------------------------------------------------------------------------------ */
/* BatchNorm1d over the batch axis of x[n][C] (BLD:62-78; SyncBatchNorm semantics, MAIN_MOCO:297):
 *   mfvit_bn_stats   : rank-local per-column mean and M2 = sum (x - mean)^2
 *   mfvit_bn_combine : merge W (mean, M2, count) triples (all_gathered by the host) -> global mean, invstd; updates the
 *                      running statistics (momentum, unbiased variance; the biased one when the global count is 1) when given.  A rank
 *                      with count 0 is skipped, whatever its mean and M2 hold (an empty rank of SyncBatchNorm)
 *   mfvit_bn_apply   : y = (x - mean) * invstd [* gamma + beta] [-> ReLU]   (gamma == NULL: affine=False) */
int mfvit_bn_stats(int dtype, const void* x, int n, int C, float* mean, float* m2, mfvit_stream_t stream);
int mfvit_bn_combine(const float* means, const float* m2s, const float* counts, int W, int C, float eps, float momentum, float* mean,
                     float* invstd, float* running_mean, float* running_var, mfvit_stream_t stream);
int mfvit_bn_apply(int dtype, const void* x, const float* mean, const float* invstd, const float* gamma, const float* beta, int relu,
                   void* y, int n, int C, mfvit_stream_t stream);
/* backward: s1 = sum dy', s2 = sum dy' * xhat per column (dy' = dy masked by the fused ReLU via y); after the host has
 * summed s1, s2 over ranks: dx = gamma * invstd * (dy' - S1 * inv_count - xhat * S2 * inv_count).  dgamma = local s2, dbeta = local s1. */
int mfvit_bn_bwd_sums(int dtype, const void* dy, const void* x, const void* y, const float* mean, const float* invstd, int relu, int n,
                      int C, float* s1, float* s2, mfvit_stream_t stream);
int mfvit_bn_bwd_apply(int dtype, const void* dy, const void* x, const void* y, const float* mean, const float* invstd, const float* gamma,
                       int relu, const float* S1, const float* S2, float inv_count, void* dx, int n, int C, mfvit_stream_t stream);
/* F.normalize(x, dim=1) (BLD:165,175) and its backward (f32). */
int mfvit_l2norm_fwd(const float* x, float* y, float* inv_norm, int n, int C, float eps, mfvit_stream_t stream);
int mfvit_l2norm_bwd(const float* dy, const float* y, const float* inv_norm, float* dx, int n, int C, mfvit_stream_t stream);
/* out[r * ldo] = scale * (a[r] . b[r])   (l_pos, BLD:183).  a, b are dense (n, C); `out` and `ldo` need no alignment: with ldo = 1 + K the
 * result goes straight into column 0 of the (n, 1 + K) logits and nothing else of them is touched (tests/test_moco_rowops_gpu.py). */
int mfvit_rowdot(const float* a, const float* b, float* out, int64_t ldo, float scale, int n, int C, mfvit_stream_t stream);
/* nn.CrossEntropyLoss (mean) over wide rows, e.g. the (n, 1 + 65536) InfoNCE logits (MAIN_MOCO:330,535):
 * loss_mean[1]; optional per-row lse (given: the mean is taken over the rows in a fixed order - the same bits on every run; NULL: one float atomic per
 * row); optional dlogits = (softmax - onehot) / n.  Rows are `ld` (logits) / `ldd` (dlogits) floats apart, both >= C; neither the strides nor the
 * base pointers need any alignment beyond a float's (every row is split into a scalar head, 16-byte body and scalar tail by its own address, and
 * a gradient row of another phase is written with scalar stores), and only the [row, :C] windows are read or written
 * (tests/test_moco_rowops_gpu.py pins this down). */
int mfvit_cross_entropy_rows(const float* logits, int64_t ld, const int64_t* target, float* loss_mean, float* lse, float* dlogits,
                             int64_t ldd, int n, int C, mfvit_stream_t stream);
/* momentum update over a flat arena: dst = dst * m + src * (1 - m)   (BLD:83-89, one launch instead of ~157 x 3). */
int mfvit_ema_update(float* dst, const float* src, float m, int64_t n, mfvit_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Multi-tensor optimizer steps.  `table` is a DEVICE array of int64[nchunks][7]:
 *   [tensor_id, param_ptr, grad_ptr, state0_ptr, state1_ptr, count, flag]   (pointers to the chunk's first float)
 * LARS (OPT:10-43): flag = 1 for tensors with ndim > 1 (weight decay + trust ratio), 0 otherwise; state0 = mu;
 *   `norms` = device scratch float[2 * ntensors].
 * Adam / AdamW (torch.optim semantics; MAIN_CA:455-459, MAIN_MOCO:338-345): state0 = exp_avg, state1 = exp_avg_sq,
 *   flag bit 0 = decoupled weight decay (AdamW); `step` counts from 1.
 * SGD (MAIN_CA:445-448): state0 = momentum buffer; first_step = 1 initialises the buffer with the gradient. */
int mfvit_lars_step(const int64_t* table, int nchunks, int ntensors, float* norms, float lr, float weight_decay, float momentum,
                    float trust_coefficient, mfvit_stream_t stream);
int mfvit_adam_step(const int64_t* table, int nchunks, float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                    mfvit_stream_t stream);
int mfvit_sgd_step(const int64_t* table, int nchunks, float lr, float momentum, float weight_decay, int first_step,
                   mfvit_stream_t stream);
/* Group-aware Adam / AdamW / SGD steps (additive in ABI 5): ONE launch over the JOINED table of several param groups, each with
 * hyperparameters of its own (layer-wise learning-rate decay: ~55 groups on the two-stream model).  A row of the joined table names
 * its entry of `hyper` in the upper half of the flag column: entry = (uint64)flag >> 32; the lower half is not read (the decoupled bit
 * is the entry's).  Per row the arithmetic is that of mfvit_adam_step / mfvit_sgd_step (first_step = 0) with the entry's values - the
 * same bits.  `hyper` is a HOST array of `nentries` entries, read before the call returns: the entries travel by value in the kernel
 * arguments, MFVIT_OPTIM_GROUPS_PER_LAUNCH of them per launch (nothing is uploaded, no buffer outlives the call); more entries mean
 * ceil(nentries / MFVIT_OPTIM_GROUPS_PER_LAUNCH) launches, each over the whole table, each serving its window of entries (the rows
 * of the other windows return at once).  bc1 = 1 - beta1^step and bc2_sqrt = sqrt(1 - beta2^step) are computed per entry with the float
 * expressions of mfvit_adam_step.
 * A row whose entry index is >= nentries is SKIPPED: nothing of it is read or written, and the index never becomes an address.
 * MFVIT_EINVAL (before any HIP call): a NULL pointer, nchunks <= 0, nentries <= 0, an Adam entry with step <= 0. */
#define MFVIT_OPTIM_GROUPS_PER_LAUNCH 64
typedef struct mfvit_adam_group {
    float lr, beta1, beta2, eps, weight_decay;
    int32_t step;        /* counts from 1, as in mfvit_adam_step */
    int32_t decoupled;   /* != 0: AdamW */
    int32_t reserved;    /* 0 */
} mfvit_adam_group;
typedef struct mfvit_sgd_group {
    float lr, momentum, weight_decay;
    int32_t reserved;    /* 0 */
} mfvit_sgd_group;
int mfvit_adam_step_groups(const int64_t* table, int nchunks, const mfvit_adam_group* hyper, int nentries, mfvit_stream_t stream);
int mfvit_sgd_step_groups(const int64_t* table, int nchunks, const mfvit_sgd_group* hyper, int nentries, mfvit_stream_t stream);
/* torch.cuda.amp.GradScaler.unscale_ over the same chunk table (MAIN_MOCO:349,546-548: scaler.scale(loss).backward();
 * scaler.step(optimizer); scaler.update()): every gradient element is multiplied by inv_scale and *found_inf (device float,
 * cleared by the caller) is set to 1 when any element was inf / nan before the multiplication. */
int mfvit_amp_unscale(const int64_t* table, int nchunks, float inv_scale, float* found_inf, mfvit_stream_t stream);

/* Gradient-norm clipping over the same chunk tables (additive in ABI 5): the three calls together replace
 * torch.nn.utils.clip_grad_norm_(parameters, max_norm, norm_type) - its foreach norm, stack, norm, clamp and foreach multiply
 * (torch/nn/utils/clip_grad.py) - with every sum taken in a fixed order (no float atomics: the same inputs give the same bits).
 * Only the gradient column and the count of a row are read.  norm_kind: 0 = L2, 1 = inf (max |g|).
 *
 * mfvit_grad_norm_partials (torch's `_foreach_norm(grads, norm_type)`): partials[row] = the sum of squares (L2) or max |g| (inf) of the
 *   row's gradient elements, one float per table row; a NaN element gives a NaN partial for either kind.  The gradients are not
 *   written.  Several tables (param groups, optimizers) take part in one total by writing to consecutive ranges of one buffer.
 * mfvit_grad_clip_coef (torch's `vector_norm(stack(norms))`, `clip_coef = max_norm / (total_norm + 1e-6)`, `clamp(max=1.0)`): over
 *   `nrows` partials, accumulated in double in row order.  row_tensor[row] in [0, ntensors) names the tensor a row belongs to (rows of
 *   one tensor need not be adjacent).  out2[0] = total norm, out2[1] = min(1, max_norm / (total + 1e-6)), each rounded to float once;
 *   a NaN total gives a NaN coefficient, an infinite one 0, as torch's formula does.  per_tensor (NULL, or float[ntensors]) receives
 *   every tensor's norm; row_tensor is read only then and may be NULL otherwise.
 * mfvit_grad_scale (torch's `_foreach_mul_(grads, clip_coef_clamped)`): g *= *coef over every row; the coefficient is read from
 *   device memory, and a coefficient of exactly 1.0f leaves the gradients untouched (no memory traffic). */
int mfvit_grad_norm_partials(const int64_t* table, int nchunks, int norm_kind, float* partials, mfvit_stream_t stream);
int mfvit_grad_clip_coef(const float* partials, const int32_t* row_tensor, int nrows, int ntensors, int norm_kind, double max_norm,
                         float* per_tensor, float* out2, mfvit_stream_t stream);
int mfvit_grad_scale(const int64_t* table, int nchunks, const float* coef, mfvit_stream_t stream);

/* Sharpness-aware minimisation over the same chunk tables (additive in ABI 5): the perturb / restore pair of SAM (Foret et al. 2021,
 * e = rho g / |g|) and ASAM (Kwon et al. 2021, e = rho w^2 g / | |w| g |), as davda54/sam's first_step / second_step compute them.  state0 of a
 * row is old_p, the copy of the parameters the second step restores; flag bit 0 of a row says "adaptive".  No atomics, fixed summation order:
 * the same inputs give the same bits.
 *
 * mfvit_sam_norm_partials: partials[row] = the row's sum of g^2 (adaptive = 0: the bits of mfvit_grad_norm_partials with norm_kind 0) or of
 *   t^2 with t = |w| g rounded to float once (adaptive = 1), in the same summation order; a NaN element gives a NaN partial.  Nothing is
 *   written but the partials.  Several tables take part in one total by writing to consecutive ranges of one buffer.
 * mfvit_sam_scale: one total over `nrows` partials, accumulated in double in row order.  out2[0] = the norm, out2[1] = 1 / (norm + 1e-12),
 *   each rounded to float once - the group's rho is applied by mfvit_sam_perturb.  out2[1] = 0 exactly when the total is not finite, or when
 *   found_inf (NULL, or the device flag of mfvit_amp_unscale) is not NULL and *found_inf != 0.
 * mfvit_sam_perturb: inv points at out2[1] on the device.  *inv == 0: nothing is read or written.  Otherwise, per element, with every
 *   product and the sum rounded to float on its own (nothing contracts to an fma): s = rho * *inv; e = g * s, or ((w * w) * g) * s in an
 *   adaptive row; old_p = w; w = w + e.  The gradient is not written.
 * mfvit_sam_restore: w = old_p over every row, unless *inv == 0 (nothing was perturbed: nothing is read or written). */
int mfvit_sam_norm_partials(const int64_t* table, int nchunks, int adaptive, float* partials, mfvit_stream_t stream);
int mfvit_sam_scale(const float* partials, int nrows, const float* found_inf, float* out2, mfvit_stream_t stream);
int mfvit_sam_perturb(const int64_t* table, int nchunks, const float* inv, float rho, mfvit_stream_t stream);
int mfvit_sam_restore(const int64_t* table, int nchunks, const float* inv, mfvit_stream_t stream);

/* Attention-guided token pruning between blocks (additive in ABI 5; Liang et al. 2022, "Not All Patches Are What You Need" - EViT's token
 * reorganisation, here at a block boundary, with normalised weights that receive no gradient).  Behind block l of a sequence of T rows per image
 * (row 0 = cls): score the T - 1 other rows by the cls token's attention, keep the K best, fold the rest into one row.  Asynchronous on `stream`;
 * no atomics on memory and every sum in a fixed order: the same bits on every run.
 *
 * mfvit_token_score: qkv [B][T][3][H][HD] in the storage format of tag qkv_dtype (MFVIT_F32 .. MFVIT_X3F16, as mfvit_attention_qkv_dtype /
 *   mfvit_vit_attn_layout report it) and lse f32 [B][H][T] of block l -> score f32 [B][T-1]: score[b][j] = mean over the heads of
 *   P[b][h][0][1 + j].  The cls row of the launch behind mfvit_vit_forward_attn (fuse = 1, cls_only = 1) into probs (scratch, f32 [B][T]), then
 *   its cls column dropped: the bits of those maps.  MFVIT_EINVAL (before any HIP call): a NULL pointer, B <= 0, B > 65535, T < 2, T > 8193,
 *   H <= 0, head_dim other than 32 / 64 / 96, an unknown tag.
 * mfvit_token_select: score f32 [B][P] (row stride ld), 1 <= K <= P -> idx_keep int32 [B][K] = {j : rank[j] < K} in ascending j, with rank as
 *   mfvit_patch_rank defines it (ties to the lower index, NaN last); idx_drop int32 [B][P-K], the others, ascending; w f32 [B][P-K]:
 *   w[j] = score[idx_drop[j]] / s, s = the sum of the dropped scores in list order, one f32 addition each - or 1 / (P - K) for every j when s
 *   is zero or not finite.  One workgroup per image, exact integers.  K == P: nothing is dropped, idx_drop and w are not touched (may be
 *   NULL).  forced (NULL, or int32 [B][K], any order): the kept set is what it names instead of the ranking's - the lists and weights of a
 *   recorded selection, to the bit; err (needed with forced; the word of mfvit_token_reorg_fwd) is set by an index outside [0, P) or named
 *   twice; idx_keep then holds fewer than K rows and its tail is -1, and nothing is written outside the lists.  MFVIT_EINVAL (before any HIP call): a NULL pointer, B <= 0, B > 65535, P <= 0,
 *   P > 8192, ld < P, K outside [1, P], forced without err.
 * mfvit_token_reorg_fwd: x f32 [B][T][D] -> out f32 [B][1 + K + fuse][D]: row 0 = x[b][0]; row 1 + k = x[b][1 + idx_keep[b][k]] (moves:
 *   bit-exact); with fuse = 1 the last row = sum over j of w[b][j] x[b][1 + idx_drop[b][j]], per column a = w_0 x_0 (one product), then
 *   a = fma(w_j, x_j, a) in list order - a single dropped row with weight 1 comes back bit for bit.  fuse = 0: idx_drop (may be NULL) is only
 *   checked, w is not read.
 * mfvit_token_reorg_bwd: dout f32 [B][1 + K + fuse][D] -> dx f32 [B][T][D], OVERWRITTEN in full, every element written once: row 0 and the kept
 *   rows moved back, dropped row idx_drop[b][j] = w[b][j] * dout[b][1 + K] (one f32 product; fuse = 0: zeros), a row no list names: zeros.
 * err (both): one int32 on the device, zero before the first call.  An index outside [0, T - 1) sets it to 1, never becomes an address, and
 *   its row is zeros (forward, kept) / is skipped (fused sum; backward); an index named twice in keep and drop together sets it too (the
 *   backward then takes the later list entry).  The caller reads the word when it likes.
 * MFVIT_EINVAL (both, before any HIP call): a NULL or not 16-byte aligned x / out / dout / dx, in place, idx_keep or err NULL, B <= 0,
 *   B > 65535, T < 2, T > 8193, D other than 384 / 768, K outside [1, T - 1], B T D >= 2^31, fuse other than 0 / 1, fuse = 1 with K == T - 1
 *   or with idx_drop / w NULL. */
int mfvit_token_score(int qkv_dtype, const void* qkv, const float* lse, int B, int T, int H, int HD, float* probs, float* score,
                      mfvit_stream_t stream);
int mfvit_token_select(const float* score, int64_t ld, int B, int P, int K, const int32_t* forced, int32_t* idx_keep, int32_t* idx_drop, float* w,
                       int32_t* err, mfvit_stream_t stream);
int mfvit_token_reorg_fwd(const float* x, const int32_t* idx_keep, const int32_t* idx_drop, const float* w, float* out, int B, int T, int D, int K,
                          int fuse, int32_t* err, mfvit_stream_t stream);
int mfvit_token_reorg_bwd(const float* dout, const int32_t* idx_keep, const int32_t* idx_drop, const float* w, float* dx, int B, int T, int D, int K,
                          int fuse, int32_t* err, mfvit_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MFVIT_H */
