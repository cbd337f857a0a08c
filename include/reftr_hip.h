/*
 * reftr_hip.h — C ABI of libreftr_hip.so, the MI355X (gfx950) kernel library that sits under the
 * Python protocol of ubc-vision/RefTR's training hot path.
 *
 * The reference has NO FFI of its own: its boundary is the Python object protocol
 *   models/__init__.py:4-10          build_reftr(args) -> (model, criterion, postprocessors)
 *   models/reftr_transformer.py:159  model(samples) -> {'pred_boxes','phrase_mask','aux_outputs'}
 *   models/criterion.py:166          criterion(outputs, targets) -> {loss_bbox, loss_giou, ...}
 *   engine_vg.py:22-78               train_one_epoch(...)
 * and every arithmetic op underneath it is an implicit ATen/oneDNN/cuDNN call made by a torch.nn
 * module.  Each entry point below replaces one such implicit call; the comment on it names the
 * reference call site (file:line under /root/reference) whose arithmetic it carries.
 *
 * Conventions
 *   - plain pointers + sizes, no torch types; every pointer is DEVICE memory unless stated;
 *   - `stream` is a hipStream_t passed as void*; kernels are only enqueued, never synchronised;
 *   - no allocation inside the library: workspaces/outputs are caller-provided;
 *   - return value: 0 = ok, <0 = RT_ERR_* (argument/shape not supported), >0 = hipError_t;
 *   - activations are bf16 (NHWC for images, [rows, features] for tokens), statistics / residual
 *     streams / losses / optimizer state are fp32, masks are uint8 (1 = padded / ignore);
 *   - thread-compatible: one caller thread per device.
 */
#ifndef REFTR_HIP_H
#define REFTR_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* rt_stream_t; /* hipStream_t */

enum { RT_OK = 0, RT_ERR_BADARG = -1, RT_ERR_UNSUPPORTED = -2, RT_ERR_COMM = -3 };
enum { RT_ACT_NONE = 0, RT_ACT_RELU = 1, RT_ACT_GELU = 2, RT_ACT_TANH = 3 };

/* Library identity: returns the ABI version (bumped on any signature change). */
int rt_abi_version(void);
/* Writes the gfx arch string of device `dev` ("gfx950...") into buf; >0 hip error if no device. */
int rt_device_arch(int dev, char* buf, int buflen);

/* --------------------------------------------------------------------------------------------
 * rt_conv_gemm — bf16 MFMA implicit-GEMM: out[m, n] = epilogue( sum_k gather(src)[m, k] * wgt[n, k] )
 *
 * One kernel carries every dense contraction whose reduction axis is contiguous in both operands:
 *   - Conv2d forward, 1x1 / 3x3, stride 1|2 (torchvision ResNet bottlenecks reached through
 *     models/modeling/backbone.py:101-109,119-121; input_proj conv models/reftr_transformer.py:121-125);
 *     FrozenBatchNorm2d (backbone.py:70-80) is folded: scale into wgt, shift into `bias`;
 *     residual add + ReLU of the bottleneck tail fused (`res_bf16`, act);
 *   - Conv2d backward-data (transposed = 1, wgt = [Cin][KH][KW][Cout] re-layout) with the ReLU mask of
 *     the producer fused (`gate`), residual-branch gradient accumulated (`res_*`);
 *   - every nn.Linear forward / backward-data on the path (nn.MultiheadAttention in/out projections
 *     models/modeling/transformer.py:151,211-212; FFNs :153-155; BERT dense layers; mlp_mapping
 *     models/reftr_transformer.py:14-23; QueryEncoder :31-39; bbox MLP backbone.py:26-38) as a 1x1
 *     "conv" over B = rows, SH = SW = 1.
 *
 * src   bf16 [B, SH, SW, SC]  (NHWC)         wgt  bf16 [N][KH][KW][SC]
 * out   [B, DH, DW, N] written as bf16 (out_bf16) and/or fp32 (out_f32)
 * forward gather   : src pixel = (dy*stride - pad + kh*dil, dx*stride - pad + kw*dil)
 * transposed gather: src pixel = ((dy + pad - kh*dil)/stride, (dx + pad - kw*dil)/stride) where divisible
 * epilogue order   : +bias[n] -> store out_preact -> [+res if res_first] -> act -> dropout(drop_p, drop_seed; index (m*N+n) >> drop_shift)
 *                    -> [+res unless res_first] -> *gate -> *gelu'(preact) -> *(1-dtanh^2) -> out_f32, acc2_f32 +=, out_bf16
 * constraints      : SC % 64 == 0, N % 4 == 0, stride in {1,2}
 * ------------------------------------------------------------------------------------------ */
typedef struct rt_conv_gemm_desc {
    const void*  src;
    const void*  wgt;
    void*        out_bf16;
    float*       out_f32;
    const float* bias;      /* [N] or NULL */
    const float* res_f32;   /* [M, N] or NULL */
    const void*  res_bf16;  /* [M, N] or NULL */
    const void*  gate;      /* bf16 [M, N] or NULL: out *= (gate > 0 ? gate_scale : 0) */
    const void*  preact;    /* bf16 [M, N] or NULL: out *= gelu'(preact) */
    int32_t B, SH, SW, SC;
    int32_t DH, DW, N;
    int32_t KH, KW, stride, pad;
    int32_t transposed;
    int32_t act;
    float    gate_scale;
    float    drop_p;
    uint32_t drop_seed;
    int32_t  tile_hint;     /* 0 = auto (the product path); otherwise a tile / stage / schedule variant by number (csrc/rt_gemm.hip): the product library
                               answers RT_ERR_BADARG for the variants only the lab library (-DRT_LAB) instantiates */
    void*    out_preact;    /* bf16 [M, N] or NULL: value after +bias, BEFORE act (saved for GELU backward) */
    const void* dtanh;      /* bf16 [M, N] or NULL: out *= (1 - dtanh^2)  (backward of a tanh output, BERT pooler) */
    int32_t  res_first;     /* 1: add res_* BEFORE act (bottleneck tail relu(bn(conv) + identity)); 0: after dropout */
    const uint32_t* seed_dev; /* optional DEVICE word: effective dropout seed = hash(*seed_dev, drop_seed) (hipGraph replay) */
    int32_t drop_shift;       /* dropout granularity: one keep/drop decision per 2^drop_shift consecutive output features of a row
                                 (hash index = (m * N + n) >> drop_shift).  With drop_shift = log2(head_dim) this is
                                 nn.MultiheadAttention's probability dropout for a ONE-key softmax (decoder self-attention with one
                                 query per image, transformer.py:231-236): the attention launch folds into the V projection */
    float* acc2_f32;          /* optional second fp32 destination [M, N] that the result is ADDED to (out_f32 / out_bf16 still receive
                                 the result itself): the q/k-side input gradient of an attention layer is both passed on and summed into
                                 the gradient of `pos` / `query_pos`, which every layer re-adds (transformer.py:154-156,168-175) */
    int32_t dil;              /* dilation of the taps (0 / 1 = none): tap (kh, kw) reads the source pixel kh * dil, kw * dil away (`--dilation`,
                                 models/modeling/backbone.py:117-125: layer4's 3x3 convolutions with dilation 2, pad 2, stride 1).
                                 dil > 1 needs stride 1 and the LDS-DMA tiles (every tile_hint but 1-3). */
} rt_conv_gemm_desc;
int rt_conv_gemm(const rt_conv_gemm_desc* d, rt_stream_t stream);
/* rt_conv_gemm_grouped — n independent rt_conv_gemm problems (HOST array of descriptors).  Dense products with K < 1024 and
 * more than 16 rows (2 <= n <= 12) run as ONE launch whose descriptors travel by value in the kernel arguments; any other
 * mix is issued as n single launches in order.  The results are those of n rt_conv_gemm calls either way.  On the
 * transformer's dependency chains (models/modeling/transformer.py:168-252: q/k and v projections of a layer, the decoder's
 * cross-attention K / V projections of all layers, pairs of backward-data products) a launch costs ~4.5 us whatever it computes. */
int rt_conv_gemm_grouped(const rt_conv_gemm_desc* descs, int n, rt_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * rt_conv_wgrad — bf16 MFMA weight-gradient GEMM, reduction over rows (pixels / tokens):
 *   dw[n][kh][kw][c] += scale[n] * sum_m dy[m, n] * gather(x)[m, (kh,kw,c)]
 * Replaces the conv_backward(weight) / addmm(grad^T, input) calls autograd issues for every trainable
 * Conv2d (layer2-4, backbone.py:87-89; input_proj) and nn.Linear on the path.
 * dy  bf16 [B, DH, DW, N]     x  bf16 [B, SH, SW, SC]     dw  fp32 [N][KH][KW][SC] (accumulated; `overwrite`: assigned)
 * Both operands are staged in their natural row-major layout and turned into MFMA fragments with the
 * gfx950 LDS transpose read (ds_read_b64_tr_b16).  The M axis is split over blocks (`msplit`, 0=auto).
 * constraints: SC % 16 == 0, N % 4 == 0
 * ------------------------------------------------------------------------------------------ */
typedef struct rt_conv_wgrad_desc {
    const void*  dy;
    const void*  x;
    float*       dw;
    const float* scale;   /* [N] or NULL (FrozenBN scale of the conv's BN) */
    int32_t B, SH, SW, SC;
    int32_t DH, DW, N;
    int32_t KH, KW, stride, pad;
    int32_t msplit;
    float*  dbias;        /* optional [N]: dbias[n] += sum_m dy[m, n] (fused bias gradient; no scale applied) */
    int32_t variant;      /* 0 = library's choice; >0 pins a kernel variant (tuning / tests, see rt_wgrad.hip) */
    float*  workspace;    /* optional scratch for the split-M partial tiles (plain stores + one reduction pass instead of
                             fp32 atomics); must not be shared by launches on concurrent streams.  NULL: atomics */
    int64_t workspace_bytes;
    int32_t overwrite;    /* 1: dw = result instead of dw += result (the caller guarantees this is the first contribution to dw since
                             the gradient buffer was last consumed: no pre-zeroed memory is needed and the epilogue skips the read of
                             dw).  dbias always accumulates. */
    int32_t dil;          /* dilation of the taps (0 / 1 = none; > 1 needs stride 1), as in rt_conv_gemm_desc */
    float*  sqacc;        /* optional gradient-norm accumulator (RT_SQ_SLOTS x RT_SQ_STRIDE floats, see rt_sqnorm_finish): the launch adds
                             |dw after|^2 - |dw before|^2, so that the clip norm (engine_vg.py:62-63) needs no pass over dw */
    void*   g16;          /* optional bf16 twin of dw (same shape): every value written to dw is also written there, rounded -- the
                             data-parallel exchange buffer (bf16 on the xGMI links, main_vg.py:290-296's all-reduce), which otherwise
                             costs a 607 MB read + 304 MB write rounding pass per step */
} rt_conv_wgrad_desc;
int rt_conv_wgrad(const rt_conv_wgrad_desc* d, rt_stream_t stream);

/* rt_small_wgrad_grouped — dw_i[N,K] += dy_i[M,N]^T x_i[M,K], dbias_i[N] += colsum(dy_i) for up to any number of independent
 * Linear weight gradients with M <= 16 token rows (decoder / query-encoder / box-head layers, transformer.py:231-252) in one
 * launch per 64 problems; `jobs` is a HOST array, copied into the kernel arguments. */
typedef struct rt_small_wgrad_job {
    const void* dy; const void* x; float* dw; float* dbias;
    int32_t M, N, K, overwrite;      /* overwrite: as in rt_conv_wgrad_desc (dbias accumulates) */
    float* sqacc;                    /* optional gradient-norm accumulator, as in rt_conv_wgrad_desc */
    void*  g16;                      /* optional bf16 twin of dw, as in rt_conv_wgrad_desc */
} rt_small_wgrad_job;
int rt_small_wgrad_grouped(const rt_small_wgrad_job* jobs, int njobs, rt_stream_t stream);

/* rt_conv_wgrad_grouped — `n` independent weight gradients (HOST array of descriptors) queued during backward and launched
 * together: the plain Linear ones (1x1, N and SC >= 128, more than 16 rows, variant = msplit = 0) share ONE launch of the
 * 128x128 kernel per 24 problems (descriptors by value in the kernel arguments) plus one grouped reduction of their split
 * partials, carved out of `workspace`; every other descriptor is forwarded to rt_conv_wgrad unchanged.  Results equal the
 * individual launches.  A transformer layer's weight gradients are 50-250 workgroups each and off the backward-data
 * dependency chain: grouped they fill the 256 CUs instead of serialising ~20 us launches.  Not re-entrant per device. */
int rt_conv_wgrad_grouped(const rt_conv_wgrad_desc* descs, int n, float* workspace, int64_t workspace_bytes, rt_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * rt_gconv / rt_gconv_wgrad — grouped 3x3 convolution: conv2 of the ResNeXt bottlenecks (torchvision Bottleneck with groups > 1,
 * reached through models/modeling/backbone.py:112-125, which builds ANY torchvision ResNet by name: resnext50_32x4d,
 * resnext101_32x8d, resnext101_64x4d).  FrozenBatchNorm2d folded as in rt_conv_gemm (scale into wgt, shift into `bias`).
 * `groups` G splits the SC input channels into G groups of Cg = SC / G; output channel n reads group n / Cg only.
 *
 * rt_gconv reuses rt_conv_gemm_desc (same field meanings, same geometry in both directions):
 *   transposed = 0  forward      : out[m, n] = act(sum_{tap, c} gather(src)[m, tap, g(n) * Cg + c] * wgt[n][tap][c] + bias[n]) (* gate)
 *   transposed = 1  backward-data: src = dy, out = dx; the transposed gather of rt_conv_gemm, reading the FORWARD weight layout
 *                   (no [C][T][N] copy); `gate` fuses the ReLU mask of the tensor whose gradient is produced
 * wgt  bf16 [SC][3][3][Cg] (forward layout; torchvision's [Cout][Cg][3][3] channels-last)     out  bf16 and/or fp32 [M, N]
 * supported: KH = KW = 3, N = SC (square groups), Cg in {4, 8, 16, 32, 64}, SC % max(Cg, 32) == 0, stride 1 | 2, dil > 1 only
 *   at stride 1, act NONE | RELU, bias, gate (gate_scale); RT_ERR_UNSUPPORTED for res_*, preact, dtanh, out_preact, acc2_f32,
 *   dropout, tile_hint != 0 and any other Cg / geometry.
 *
 * rt_gconv_wgrad reuses rt_conv_wgrad_desc:
 *   dw[n][tap][c] (+)= scale[n] * sum_m dy[m, n] * gather(x)[m, tap, g(n) * Cg + c]       dw fp32 [N][3][3][Cg]
 *   The M axis is split over the chip (`msplit`, 0 = auto); the split partials go to `workspace` (REQUIRED: at least
 *   N * 9 * Cg floats; the split count is capped by its size) and one reduction launch applies scale, `overwrite`, the clip-norm
 *   contribution (`sqacc`) and the bf16 twin (`g16`), as rt_conv_wgrad does.  RT_ERR_UNSUPPORTED for dbias, variant != 0
 *   and the geometries rt_gconv refuses.
 * Both enqueue kernels only (capture-safe: no host synchronisation, no allocation).
 * ------------------------------------------------------------------------------------------ */
int rt_gconv(const rt_conv_gemm_desc* d, int groups, rt_stream_t stream);
int rt_gconv_wgrad(const rt_conv_wgrad_desc* d, int groups, rt_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * rt_layernorm_fwd / rt_layernorm_bwd — nn.LayerNorm over the last axis, fp32 statistics, one wave per row.
 * Replaces: encoder/decoder norm1-3 and decoder.norm (models/modeling/transformer.py:157-158,217-219,
 * 176-180,243-251,131-138), BERT LayerNorms (eps 1e-12), the LayerNorms inside mlp_mapping
 * (models/reftr_transformer.py:14-23) and QueryEncoder.context_out (:36-39).
 * Fused around it: post-norm ReLU (+dropout) of mlp_mapping, bf16 operand copy for the next GEMM,
 * bf16(y + pos) for the q/k input of the next attention (with_pos_embed, transformer.py:165-166,172).
 * Output rows can be re-mapped so that per-image token blocks land inside the [B, S, D] sequence buffer:
 *   out_row = (r / grp_rows) * grp_stride + grp_off + r % grp_rows      (grp_rows = 0: identity)
 * Backward: dx (fp32) plus bf16(dx * dropout2-mask) — the gradient entering the GEMM whose output was
 * dropped-out and added to the residual before this norm; dgamma/dbeta accumulated with atomics.
 * ------------------------------------------------------------------------------------------ */
typedef struct rt_layernorm_desc {
    const float* x;        /* [M, D] */
    const float* gamma;    /* [D] */
    const float* beta;     /* [D] */
    float*       y_f32;    /* row-mapped, or NULL */
    void*        y_bf16;   /* row-mapped, or NULL */
    const float* pos;      /* row-mapped like the outputs, or NULL */
    void*        ypos_bf16;/* bf16(y + pos), or NULL */
    float*       mean;     /* [M] or NULL */
    float*       rstd;     /* [M] or NULL */
    int32_t M, D;
    float   eps;
    int32_t act;           /* RT_ACT_NONE | RT_ACT_RELU (after the affine) */
    float    drop_p;       /* dropout after act, index r*D + c */
    uint32_t drop_seed;
    int32_t grp_rows, grp_stride, grp_off;
    const uint32_t* seed_dev;   /* optional, see rt_conv_gemm_desc */
} rt_layernorm_desc;
int rt_layernorm_fwd(const rt_layernorm_desc* d, rt_stream_t stream);

typedef struct rt_layernorm_bwd_desc {
    const float* dy;       /* row-mapped grad of the LN output */
    const float* dy2;      /* optional second grad (same mapping) added to dy, or NULL */
    const float* x;        /* [M, D] LN input */
    const float* gamma;
    const float* beta;     /* needed when act == RELU */
    const float* mean;
    const float* rstd;
    float*       dx_f32;   /* [M, D] or NULL */
    void*        dx_bf16;  /* [M, D] bf16(dx * mask2 / (1-p2)) or NULL */
    float*       dgamma;   /* [D] accumulated, or NULL */
    float*       dbeta;    /* [D] accumulated, or NULL */
    int32_t M, D;
    int32_t act;
    float    drop_p;  uint32_t drop_seed;    /* the LN's own post-act dropout */
    float    drop2_p; uint32_t drop2_seed;   /* dropout of the producing sub-layer (index r*D + c) */
    int32_t grp_rows, grp_stride, grp_off;
    const uint32_t* seed_dev;   /* optional, applies to both dropout seeds */
    float*   partials;     /* optional [n_blocks][2][D] scratch: per-workgroup dgamma / dbeta partial sums are STORED there
                              (no atomics); the caller reduces them later with rt_ln_param_grad_grouped.  dgamma / dbeta
                              are then not touched.  n_blocks is returned through *n_blocks_out. */
    int32_t* n_blocks_out; /* host pointer, written when partials != NULL */
} rt_layernorm_bwd_desc;
int rt_layernorm_bwd(const rt_layernorm_bwd_desc* d, rt_stream_t stream);

/* rt_ln_param_grad_grouped — dgamma_i[D] += sum_b partials_i[b][0][:], dbeta_i[D] += sum_b partials_i[b][1][:] for any number
 * of LayerNorm backward launches (HOST array, descriptors by value in the kernel arguments).  The LayerNorm parameter
 * gradients are off the backward-data dependency chain: one launch per 64 of them instead of ~2*D contended atomics per
 * workgroup inside every rt_layernorm_bwd. */
typedef struct rt_ln_pg_job {
    const float* partials; float* dgamma; float* dbeta;
    int32_t n_blocks, D;
} rt_ln_pg_job;
int rt_ln_param_grad_grouped(const rt_ln_pg_job* jobs, int n, rt_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * rt_groupnorm_fwd / rt_groupnorm_bwd — nn.GroupNorm(G, C) of input_proj (models/reftr_transformer.py:
 * 121-125,174) on the token-major image x[b][pixel][c]; statistics per (image, group) over HW * C/G values.
 * Output rows go to (b * out_rows_per_img + out_row_off + pixel) so the image tokens land behind the
 * language tokens of the [B, S, C] sequence (models/reftr.py:115-117).  stats/bstats: [B, G, 2] workspaces.
 * The forward statistics are reduced in a fixed order (per-chunk partial sums, then a fixed shuffle tree): no atomics, so
 * the eval-mode forward is bit-reproducible run to run like the reference's.
 * ------------------------------------------------------------------------------------------ */
typedef struct rt_groupnorm_desc {
    const float* x;        /* [B, HW, C] */
    const float* gamma; const float* beta;
    float*       stats;    /* [B, G, 2] workspace: sum, sumsq (kept for backward) */
    float*       y_f32; void* y_bf16;
    const float* pos; void* ypos_bf16;
    int32_t B, HW, C, G;
    float   eps;
    int32_t out_rows_per_img, out_row_off;
    float*  partials;      /* [B, chunks, G, 2] workspace: per-pixel-chunk sums, 1 <= chunks <= 64 */
    int32_t chunks;
} rt_groupnorm_desc;
int rt_groupnorm_fwd(const rt_groupnorm_desc* d, rt_stream_t stream);

typedef struct rt_groupnorm_bwd_desc {
    const float* dy; const float* dy2;   /* sequence-mapped like the forward outputs */
    const float* x; const float* gamma;
    const float* stats;    /* from forward */
    float*       bstats;   /* [B, G, 2] workspace */
    float*       dx_f32; void* dx_bf16;  /* [B, HW, C] */
    float*       dgamma; float* dbeta;
    int32_t B, HW, C, G;
    float   eps;
    int32_t out_rows_per_img, out_row_off;
} rt_groupnorm_bwd_desc;
int rt_groupnorm_bwd(const rt_groupnorm_bwd_desc* d, rt_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * RES head (RefTRSeg, models/reftr_segmentation.py).  The 3x3 / 1x1 convolutions of MaskHeadSmallConv (:216-238) and
 * the k/q projections of MHAttentionMap (:186-187) run through rt_conv_gemm / rt_conv_wgrad with channel counts padded
 * to multiples of 64 (zero weights / activations in the padding); the entry points below are everything around them.
 *
 * rt_gn_nhwc_fwd / _bwd — GroupNorm(8, C) + ReLU (:242-248,256-258,...) over x[b][p][c] (fp32 conv output, row stride
 *   ldx); writes the next convolution's bf16 operand with row stride ldy >= C, padding zero-filled.
 *   stats / bstats: [B, G, 2] workspaces (sum, sumsq) kept for backward.  dy fp32 (row stride lddy), dx bf16 (lddx).
 *   Forward statistics go through `partials` ([B, partial_blocks, G, 2], partial_blocks >= ceil(HW / ceil(16384 / C))) and
 *   are added in a fixed order (no atomics): the eval-mode mask logits are bit-reproducible run to run.
 * rt_upsample_add / _bwd — `cur_fpn + F.interpolate(x, size, mode="nearest")` (:253,262,271).  Backward returns the
 *   pixel-summed gradient of the coarse operand and a bf16 copy of dy (the adapter convolution's output gradient).
 * rt_attn_map_fwd / _bwd — MHAttentionMap.forward (:196-208): softmax over (heads, h, w) jointly of
 *   norm * <q_head, k_head>, padded pixels (mask != 0) -> -inf.  k rows: (b * k_rows_per_img + k_row_off + p) * ldk.
 *   The probabilities are also written (bf16) into columns concat_col.. of the mask head's input rows.
 * rt_seg_concat — torch.cat([img_src_proj, memory_visual, bbox_mask]) of refer_segmentation (:165) / mask_head (:241).
 * rt_mask_loss — CriterionVGOnePhraseSeg.loss_masks (:314-337): bilinear (align_corners=False) upsample of the logits
 *   to the padded target size + sigmoid_focal_loss(alpha .25, gamma 2) + dice_loss (modeling/segmentation.py:178-221).
 *   dpred == NULL: forward (sums [B,4] workspace, losses[2] = {focal, dice}); else backward, accumulating into dpred.
 * ------------------------------------------------------------------------------------------ */
typedef struct rt_gn_nhwc_desc {
    const float* x; const float* gamma; const float* beta;
    float* stats; void* y_bf16;
    int32_t B, HW, C, G, ldx, ldy, act;
    float eps;
    float* partials; int32_t partial_blocks;
} rt_gn_nhwc_desc;
int rt_gn_nhwc_fwd(const rt_gn_nhwc_desc* d, rt_stream_t stream);

typedef struct rt_gn_nhwc_bwd_desc {
    const float* dy; const float* x; const float* gamma; const float* beta;
    const float* stats; float* bstats;
    void* dx_bf16; float* dgamma; float* dbeta;
    int32_t B, HW, C, G, ldx, lddy, lddx, act;
    float eps;
} rt_gn_nhwc_bwd_desc;
int rt_gn_nhwc_bwd(const rt_gn_nhwc_bwd_desc* d, rt_stream_t stream);

typedef struct rt_upsample_add_desc {
    const float* fpn; const void* a_bf16; void* out_bf16;
    int32_t B, H, W, h, w, C, ldf, lda, ldo;
} rt_upsample_add_desc;
int rt_upsample_add(const rt_upsample_add_desc* d, rt_stream_t stream);

typedef struct rt_upsample_add_bwd_desc {
    const float* dy; float* da; void* dy_bf16;
    int32_t B, H, W, h, w, C, lddy, ldda, lddyb;
} rt_upsample_add_bwd_desc;
int rt_upsample_add_bwd(const rt_upsample_add_bwd_desc* d, rt_stream_t stream);

typedef struct rt_attn_map_desc {
    const float* q; const float* k; const uint8_t* mask;
    float* P; void* concat_bf16;
    int32_t B, HW, E, nh, ldk, k_rows_per_img, k_row_off, ld_concat, concat_col;
    float norm;
} rt_attn_map_desc;
int rt_attn_map_fwd(const rt_attn_map_desc* d, rt_stream_t stream);

typedef struct rt_attn_map_bwd_desc {
    const float* q; const float* k; const float* P; const float* dconcat;
    float* dq; float* dk;
    int32_t B, HW, E, nh, ldk, k_rows_per_img, k_row_off, ld_dconcat, concat_col;
    float norm;
} rt_attn_map_bwd_desc;
int rt_attn_map_bwd(const rt_attn_map_bwd_desc* d, rt_stream_t stream);

typedef struct rt_seg_concat_desc {
    const float* src; const float* mem; void* out_bf16;
    int32_t B, HW, E, nh, ldo, mem_rows_per_img, mem_row_off, src_rows_per_img, src_row_off;
} rt_seg_concat_desc;
int rt_seg_concat(const rt_seg_concat_desc* d, rt_stream_t stream);

typedef struct rt_mask_loss_desc {
    const float* pred; const uint8_t* target;
    float* sums; float* losses;
    float* dpred; const float* g_focal; const float* g_dice;
    int32_t B, h, w, Ht, Wt, ldp, lddp;
    float inv_norm;
    float* gbuf;           /* backward: scratch fp32 [B, Ht, Wt] (the per-target-pixel gradient between the two passes); forward, optional:
                              RT_MASK_LOSS_PARTIALS floats per image -- the workgroups' partial sums go there and are added in a fixed
                              order (the same loss bits from run to run) instead of through atomics */
} rt_mask_loss_desc;
#define RT_MASK_LOSS_PARTIALS 1024     /* 4 sums x at most 256 workgroups per image */
int rt_mask_loss(const rt_mask_loss_desc* d, rt_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * rt_attn_fwd / rt_attn_bwd — softmax(scale * Q K^T + key_padding_mask) V per (batch, head), the core of
 * nn.MultiheadAttention (models/modeling/transformer.py:174-175,234-246) and of HF BertSelfAttention.
 * Element (b, i, h, d) of q/k/v/out lives at ptr[(b*S + i)*ld + h*dh + d] so packed projection outputs are
 * consumed in place.  kpm: uint8 [B, Sk], 1 = ignore (-inf); a fully masked row yields NaN like the
 * reference.  Dropout acts on the probabilities (index ((b*H+h)*Sq + i)*Sk + j).  lse = log-sum-exp per row
 * (saved for backward); delta is a [B,H,Sq] fp32 workspace.  dh in {32, 64}; Sq, Sk <= 768.
 * ------------------------------------------------------------------------------------------ */
typedef struct rt_attn_desc {
    const void* q; const void* k; const void* v;
    void*  out;
    float* lse;            /* [B, H, Sq] or NULL */
    const uint8_t* kpm;    /* [B, Sk] or NULL */
    int32_t B, H, Sq, Sk, dh;
    int32_t ldq, ldk, ldv, ldo;
    float    scale;
    float    drop_p; uint32_t drop_seed;
    const uint32_t* seed_dev;   /* optional, see rt_conv_gemm_desc */
} rt_attn_desc;
int rt_attn_fwd(const rt_attn_desc* d, rt_stream_t stream);

typedef struct rt_attn_bwd_desc {
    const void* q; const void* k; const void* v; const void* out; const void* dout;
    const float* lse;
    float* delta;          /* [B, H, Sq] workspace */
    const uint8_t* kpm;
    void* dq; void* dk; void* dv;
    int32_t B, H, Sq, Sk, dh;
    int32_t ldq, ldk, ldv, ldo, lddq, lddk, lddv;
    float    scale;
    float    drop_p; uint32_t drop_seed;
    const uint32_t* seed_dev;
} rt_attn_bwd_desc;
int rt_attn_bwd(const rt_attn_bwd_desc* d, rt_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * Backbone-side kernels (models/modeling/backbone.py:83-125 + torchvision ResNet stem).
 * rt_img_pack        NCHW fp32 [B,3,H,W] -> NHWC4 bf16 [B,Hp,Wp,4] with a 3-pixel zero halo on top/left
 *                    (Hp >= H+6, Wp >= W+6; the 4th channel and the halo are zero)
 * rt_stem_conv       conv1 7x7/2 pad 3 + FrozenBN + ReLU on MFMA: per kernel row one K=32 step
 *                    (8 taps x 4 channels); w bf16 [64][7][8][4] (BN scale folded), bias = BN shift;
 *                    out bf16 NHWC [B,Ho,Wo,64]; needs Wp >= 32*ceil(Wo/16)+6, Hp >= 2*Ho+5
 * rt_maxpool3x3s2    nn.MaxPool2d(3, 2, 1) on NHWC bf16
 * rt_stem_pool       rt_stem_conv + rt_maxpool3x3s2 in one launch (torchvision ResNet.forward: conv1, bn1, relu, maxpool; all
 *                    frozen, backbone.py:87-89): out bf16 NHWC [B,(Ho-1)/2+1,(Wo-1)/2+1,64], bit-identical to the two launches;
 *                    the stem output itself is never written; needs Wp >= 2*Wo+6, Hp >= 2*Ho+5
 * rt_weight_prep     fp32 master weight [N][T][C] (T = KH*KW, channels-last) -> bf16 [N][T][C] (dst) and/or
 *                    bf16 [C][T][N] (dst_t, the backward-data operand), times scale[n] (FrozenBN) if given
 * rt_stem_weight_prep fp32 [64][7][7][3] -> bf16 [64][7][8][4]
 * rt_bn_fold         FrozenBatchNorm2d (backbone.py:70-80): scale = w*rsqrt(rv+eps), shift = b - rm*scale
 * ------------------------------------------------------------------------------------------ */
int rt_img_pack(const float* img, void* out, int B, int H, int W, int Hp, int Wp, rt_stream_t stream);
int rt_stem_conv(const void* xp, const void* w, const float* bias, void* out,
                 int B, int Hp, int Wp, int Ho, int Wo, rt_stream_t stream);
int rt_maxpool3x3s2(const void* x, void* y, int B, int H, int W, int C, int Ho, int Wo, rt_stream_t stream);
int rt_stem_pool(const void* xp, const void* w, const float* bias, void* out,
                 int B, int Hp, int Wp, int Ho, int Wo, rt_stream_t stream);
int rt_weight_prep(const float* src, const float* scale, void* dst, void* dst_t, int N, int T, int C, rt_stream_t stream);

/* rt_bottleneck_fwd — one FROZEN stride-1 bottleneck of layer1 in ONE launch (models/modeling/backbone.py:87-89 freezes conv1 and
 * layer1; torchvision Bottleneck v1.5 with FrozenBatchNorm2d :43-80): conv1 1x1 + BN + ReLU -> conv2 3x3 pad 1 + BN + ReLU ->
 * conv3 1x1 + BN (+ x | + downsample 1x1 + BN) -> ReLU.  The 64-channel intermediates never leave LDS.  NHWC bf16 activations;
 * weights bf16 with the BN scale folded (rt_weight_prep layout [N][T][C]), b* = BN shifts.  planes must be 64;
 * cin = 256 with wd = bd = NULL (identity shortcut) or cin = 64 with the downsample operands.  B*H*W*256 < 2^31. */
typedef struct rt_bottleneck_desc {
    const void*  x;        /* bf16 [B,H,W,cin] */
    const void*  w1;       /* bf16 [64][cin] */
    const void*  w2;       /* bf16 [64][9][64] */
    const void*  w3;       /* bf16 [256][64] */
    const void*  wd;       /* bf16 [256][cin] or NULL */
    const float* b1;       /* [64] */
    const float* b2;       /* [64] */
    const float* b3;       /* [256] */
    const float* bd;       /* [256] or NULL */
    void*        out;      /* bf16 [B,H,W,256] */
    int32_t B, H, W, cin, planes;
    int32_t form;          /* 0 or 1: one 8 x 16 tile per workgroup, weights through an LDS ring (the forms 2 / 3 of round 4 were removed: RT_ERR_UNSUPPORTED) */
} rt_bottleneck_desc;
int rt_bottleneck_fwd(const rt_bottleneck_desc* d, rt_stream_t stream);
/* rt_weight_prep_batched — every per-step operand refresh in ONE launch.  table: DEVICE int64 [njobs][8] =
 * {src, scale|0, dst|0, dst_t|0, N, T, C, first_tile}; a job's tiles are 32(n) x 32(c) per tap, tiles numbered
 * consecutively over jobs (total_tiles = sum).  Both outputs are written coalesced (LDS tile transpose). */
int rt_weight_prep_batched(const int64_t* table, int njobs, int total_tiles, rt_stream_t stream);
int rt_stem_weight_prep(const float* src, const float* scale, void* dst, rt_stream_t stream);
int rt_bn_fold(const float* w, const float* b, const float* rm, const float* rv, float eps,
               float* scale, float* shift, int n, rt_stream_t stream);

/* rt_mask_posenc — pad-mask nearest downsample (backbone.py:107, exact/integer) + PositionEmbeddingSine
 * (models/modeling/position_encoding.py:36-56: normalize, scale 2*pi, T=1e4, eps 1e-6) + add_vec[c]
 * (level_embed[0] + token_type_embeddings[1], models/reftr.py:60,70-73).  mask uint8 [B,H,W] (1 = pad).
 * kpm_out[b*kpm_stride + kpm_off + pix] = downsampled mask; pos_out row = b*pos_rows_per_img + pos_row_off + pix. */
typedef struct rt_mask_posenc_desc {
    const uint8_t* mask;
    uint8_t* kpm_out;
    float*   pos_out;
    const float* add_vec;   /* [C] or NULL */
    int32_t B, H, W, h, w, C;
    int32_t kpm_stride, kpm_off;
    int32_t pos_rows_per_img, pos_row_off;
} rt_mask_posenc_desc;
int rt_mask_posenc(const rt_mask_posenc_desc* d, rt_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * Small fused memory-bound kernels around the GEMMs.
 * rt_colsum          db[n] += sum_m dy[m,n]   (bias gradients of every nn.Linear / input_proj conv)
 * rt_rows_add        out[map_o(r)] (=|+=) alpha * (a[map_a(r)] + b[map_b(r)]), fp32 and/or bf16 out;
 *                    row maps as in rt_layernorm (grp_rows = 0: identity; grp_rows < 0: broadcast
 *                    (r / -grp_rows) * stride + off); accumulate = 2 uses atomics.  Used for with_pos_embed
 *                    (transformer.py:165-166), residual-gradient accumulation, CLS-row gather/scatter.
 * rt_bert_embed_*    HF BertEmbeddings lookup word[ids] + pos[l] + type[0] and its scatter-add backward
 * rt_context_mask    models/reftr_transformer.py:224-248 (bool only): context mask + query mask
 * rt_qenc_attn_*     QueryEncoder CLS-key attention (models/reftr_transformer.py:48-55), fp32
 * ------------------------------------------------------------------------------------------ */
int rt_colsum(const void* dy, int is_bf16, float* db, int M, int N, rt_stream_t stream);

typedef struct rt_rows_add_desc {
    const float* a_f32; const void* a_bf16; const float* b_f32;
    float* out_f32; void* out_bf16;
    int32_t rows, D;
    float   alpha;
    int32_t accumulate;     /* out_f32 += instead of = */
    int32_t a_grp_rows, a_grp_stride, a_grp_off;
    int32_t b_grp_rows, b_grp_stride, b_grp_off;
    int32_t o_grp_rows, o_grp_stride, o_grp_off;
} rt_rows_add_desc;
int rt_rows_add(const rt_rows_add_desc* d, rt_stream_t stream);

int rt_bert_embed_fwd(const int64_t* ids, const float* word, const float* pos, const float* type0,
                      float* out, int rows, int L, int D, const int32_t* pos_ids, rt_stream_t stream);
int rt_bert_embed_bwd(const int64_t* ids, const float* de, float* dword, float* dpos, float* dtype0,
                      int rows, int L, int D, const int32_t* pos_ids, rt_stream_t stream);
/* pos_ids (optional, int32 [rows]): explicit position ids; NULL = row % L (BERT).  rt_roberta_pos_ids fills them as HF
 * RobertaEmbeddings does (create_position_ids_from_input_ids: cumsum(ids != pad) * (ids != pad) + pad), exact integers. */
int rt_roberta_pos_ids(const int64_t* ids, int32_t* pos_ids, int B, int L, int pad_idx, rt_stream_t stream);
int rt_context_mask(const uint8_t* smask, const uint8_t* phrase_mask, const int64_t* pos_l, const int64_t* pos_r,
                    uint8_t* ctx, uint8_t* qmask, int B, int L, int P, int Lp, rt_stream_t stream);
int rt_qenc_attn_fwd(const float* k, const float* qs, const float* vs, const uint8_t* ctx, float* w, float* c,
                     int B, int P, int L, int E, rt_stream_t stream);
int rt_qenc_attn_bwd(const float* k, const float* qs, const float* vs, const float* w, const float* dc,
                     float* dk, float* dqs, float* dvs, int B, int P, int L, int E, rt_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * rt_box_loss — CriterionVGMultiPhrase.loss_boxes for all NL decoder layers at once
 * (models/criterion.py:113-202, util/box_ops.py:17-69).  logits fp32 [NL,B,P,K,4] (pre-sigmoid),
 * valid uint8 [B,P*K] (phrase_mask, 1 = valid), targets fp32 [sum n_b, 4] cxcywh with tgt_off int32 [B+1],
 * num_boxes: DEVICE fp32 scalar (already all-reduced / world, clamp >= 1 applied here).
 * losses[l*2+0] = loss_bbox of layer l, losses[l*2+1] = loss_giou; total = sum_l w_bbox*l1 + w_giou*giou;
 * dlogits = d total / d logits (0 for invalid phrases).  Selection/ordering is exact.
 * Both outputs are cleared by the call (they are accumulated with atomics); total == losses + 2*NL (one buffer) costs one clear.
 * ------------------------------------------------------------------------------------------ */
typedef struct rt_box_loss_desc {
    const float*   logits;
    const uint8_t* valid;
    const float*   targets;
    const int32_t* tgt_off;
    const float*   num_boxes;
    float* losses; float* total; float* dlogits;
    int32_t NL, B, P, K;
    float   w_bbox, w_giou;
    const float* weights;   /* optional DEVICE [NL,2] per-layer (bbox, giou) weights overriding w_bbox / w_giou */
} rt_box_loss_desc;
int rt_box_loss(const rt_box_loss_desc* d, rt_stream_t stream);

/* rt_small_dgrad — backward-data of a Linear with N <= 8 outputs (the 4-wide bbox_embed.layers.2,
 * backbone.py:26-38): dx[m,k] = sum_n dy[m,n] w[n,k], optional ReLU gate (gate > 0), bf16 out.
 * rt_pos_grad    — reduces the gradient of the `pos` sequence (models/reftr.py:60-89) onto
 * lang_pos_embeddings [L,E], token_type_embeddings [2,E] and level_embed [1,E] (accumulated). */
int rt_small_dgrad(const float* dy, const float* w, const void* gate, void* dx, int M, int N, int K, rt_stream_t stream);
int rt_pos_grad(const float* dpos, float* d_lang_pos, float* d_type, float* d_level, int B, int S, int L, int E,
                rt_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * Optimizer step over the flat parameter / gradient buffers (engine_vg.py:62-67, main_vg.py:234-268).
 * rt_sqnorm      out[0] = sum g^2
 * rt_adamw_flat  g' = g * grad_scale; total = sqrt(gnorm_sq) * grad_scale; coef = min(1, max_norm/(total+1e-6))
 *                (clip_grad_norm_, skipped when max_norm <= 0); AdamW with decoupled weight decay, bias
 *                correction at `step` (1-based); per-range lr / wd = the reference's param groups.
 *                span_begin < span_end restricts the pass to that element span (the update of one step may be issued as
 *                several launches on different streams, e.g. the BERT slice concurrently with the ResNet forward);
 *                `active` (DEVICE word, optional): the launch is a no-op while it is 0 (nothing pending under graph
 *                replay); `lr_dev` (DEVICE float[n_ranges], optional) overrides range_lr, so a replayed graph follows
 *                the learning-rate schedule without re-capture.
 * ------------------------------------------------------------------------------------------ */
int rt_sqnorm(const float* g, int64_t n, float* out, rt_stream_t stream);
/* the same over a bf16 gradient buffer (data-parallel runs exchange the gradients in bf16, reftr_amd/parallel.py) */
int rt_sqnorm_bf16(const void* g16, int64_t n, float* out, rt_stream_t stream);

typedef struct rt_adamw_desc {
    float* p; const float* g; float* m; float* v;
    int64_t n;
    const float* gnorm_sq;  /* device scalar from rt_sqnorm, or NULL */
    float* gnorm_out;       /* device scalar: total norm (after grad_scale), or NULL */
    float grad_scale, max_norm, beta1, beta2, eps;
    int32_t step, n_ranges;
    int64_t range_begin[8], range_end[8];
    float   range_lr[8], range_wd[8];
    const int32_t* step_dev;  /* optional DEVICE word overriding `step` (the optimizer step counter under hipGraph replay) */
    const int32_t* active;    /* optional DEVICE word: 0 = skip this launch */
    const float*   lr_dev;    /* optional DEVICE [n_ranges] learning rates overriding range_lr */
    int64_t span_begin, span_end;   /* element span to update (multiples of 4); 0, 0 = the whole buffer */
    const void* g16;          /* optional bf16 gradient buffer read INSTEAD of g (the exchanged gradients of a data-parallel run) */
} rt_adamw_desc;
int rt_adamw_flat(const rt_adamw_desc* d, rt_stream_t stream);
/* rt_sgd_flat — torch.optim.SGD(momentum, weight_decay), the reference's --sgd optimizer (main_vg.py:263-265), over the same flat
 * buffers and with the same descriptor: m = momentum buffer (zero-initialised), beta1 = momentum, v / beta2 / eps / step unused:
 *   g' = clip * grad_scale * g + wd * p;  m = beta1 * m + g';  p -= lr * m.   Clip coefficient and 1/world as in rt_adamw_flat. */
int rt_sgd_flat(const rt_adamw_desc* d, rt_stream_t stream);
/* rt_grad_accum — gradient accumulation over the micro-batches of one window (one update per k backward passes: the published
 * global batch on one GPU), over the flat fp32 gradient buffer `g` and an accumulator `acc` of the same size (both 4-byte aligned;
 * 16-byte accesses wherever the two reach a 16-byte boundary together, coalesced 4-byte accesses over the same grid where they never do):
 *   RT_ACCUM_FIRST   acc = g                        (first micro-batch: no clear of the accumulator is ever needed)
 *   RT_ACCUM_ADD     acc += g
 *   RT_ACCUM_FINISH  g = (acc + g) * s  and  out_sq[0] = sum of the squares of the values written -- what rt_sqnorm would return for
 *                    the averaged buffer, so the clip norm costs no further pass.  s = scale, or scale_dev[0] when `scale_dev` (DEVICE
 *                    float, optional) is given: one captured launch serves any window length, like lr_dev of rt_adamw_desc.
 * `partials` (FINISH only): RT_GRAD_ACCUM_SLOTS floats of workspace, one per workgroup; a second one-workgroup launch adds them in a
 * fixed order (no atomics: the same bits from run to run).  Nothing is allocated; FIRST / ADD are one launch. */
enum { RT_ACCUM_FIRST = 0, RT_ACCUM_ADD = 1, RT_ACCUM_FINISH = 2 };
#define RT_GRAD_ACCUM_SLOTS 2048
int rt_grad_accum(int mode, float* g, float* acc, int64_t n, float scale, const float* scale_dev, float* partials, float* out_sq,
                  rt_stream_t stream);
/* rt_zero_chunks — clears `n` chunks of an fp32 buffer in one launch: table (DEVICE, static) = n x {int64 element offset, int64
 * element count (<= 16384)}.  Used for the gradient tensors that are accumulated with atomics (biases, norm parameters,
 * embeddings) when the weight matrices are produced in overwrite mode and the full clear of the gradient buffer is skipped. */
int rt_zero_chunks(float* base, const int64_t* table, int n, rt_stream_t stream);
/* rt_sqnorm_finish — the clip norm without a pass over the weight gradients.  Every weight-gradient launch given `sqacc` has added
 * |dw after|^2 - |dw before|^2 of what it wrote to the accumulator's slots (RT_SQ_SLOTS words, RT_SQ_STRIDE floats apart: the caller
 * clears the RT_SQ_SLOTS * RT_SQ_STRIDE floats when it clears / re-arms the gradient buffer).  This call adds the squared norm of
 * the tensors no such launch produces -- biases, norm parameters, embeddings, accumulated with atomics: the chunks of `table`
 * (DEVICE int64 [nchunks][2] = {element offset in `base`, count <= 16384}) -- and writes out[0] = sum of the slots (+ extra[0]). */
#define RT_SQ_SLOTS 256
#define RT_SQ_STRIDE 32
int rt_sqnorm_finish(const float* base, const int64_t* table, int nchunks, float* slots, const float* extra, float* out, rt_stream_t stream);
/* rt_round_chunks — twin[i] = bf16(base[i]) over `n` chunks {element offset, count <= 16384} (DEVICE int64 table): the tensors of a
 * gradient slice that no weight-gradient launch writes (biases, norm parameters, embeddings) on their way into the bf16 exchange
 * buffer; the weight matrices arrive there through rt_conv_wgrad_desc.g16. */
int rt_round_chunks(const float* base, void* twin, const int64_t* table, int n, rt_stream_t stream);
/* rt_counter_add — *ctr += inc on the device (step / dropout-seed counters that must advance inside a captured graph). */
int rt_counter_add(int32_t* ctr, int32_t inc, rt_stream_t stream);
/* rt_counter_add_if_zero — the same, but only while the DEVICE word *cond is 0; otherwise *ctr is left alone (reset_else = 0) or
 * cleared (reset_else = 1).  The engine advances the optimizer step counter (left alone) and the "update pending" word (cleared) of
 * an iteration through it with cond = the cooperative decoder's failure word: an iteration whose launches reported a hand-off
 * timeout never arms its AdamW update (engine_vg.py:55-58 of the reference stops BEFORE the update when an iteration is bad; here
 * the decision is taken on the device, inside the captured graph). */
int rt_counter_add_if_zero(int32_t* ctr, int32_t inc, const uint32_t* cond, int reset_else, rt_stream_t stream);
/* rt_finish_step — both counters of an iteration's end in ONE launch, with the reference's second stop condition carried to the
 * device as well: *step += 1 and *active += 1 unless (*cond != 0, cond optional) or (*loss is not finite, loss optional: the
 * iteration's weighted total); otherwise *active = 0 and *step is left alone.  engine_vg.py:53-58 stops BEFORE the update when the
 * loss is not finite; with the decision on the device the host may launch iteration i + 1 before it has read iteration i's numbers
 * (a pipelined loop): a bad iteration's update is never applied, the host stops one read later. */
int rt_finish_step(int32_t* step, int32_t* active, const uint32_t* cond, const float* loss, rt_stream_t stream);
/* rt_finish_stats — rt_finish_step plus everything else the loop reads from an iteration, in the same one-thread launch: the total
 * gradient norm grad_norm[0] = sqrt(sq[0]) * norm_scale (clip_grad_norm_'s return value, engine_vg.py:62-66) and the iteration's stats
 * vector stats = [*src[0] ... *src[n_src-1] | float(*cond) if cond_in_stats | grad_norm] -- the unweighted losses the meters log
 * (engine_vg.py:46-53, util/misc.py:156-160) as device scalars wherever the criterion left them.  Replaces four launches at the end of
 * every replayed step (counters, sqrt, a dtype conversion, a concatenation). */
#define RT_STATS_MAX 40
typedef struct {
    int32_t *step, *active;  const uint32_t* cond;  const float* loss;          /* as rt_finish_step */
    const float* sq;  float norm_scale;  float* grad_norm;                      /* optional (sq = NULL: grad_norm untouched) */
    const float* src[RT_STATS_MAX];  int n_src;  int cond_in_stats;  float* stats;   /* optional (stats = NULL) */
} rt_finish_desc;
int rt_finish_stats(const rt_finish_desc* d, rt_stream_t stream);
/* rt_stamp — buf[idx] = the device's constant 100 MHz wall clock (s_memrealtime) when the stream reaches this point: a one-thread
 * kernel the measurement tools capture into the step's graph at phase boundaries of every stream (tools/concurrent_timeline.py),
 * because rocprofv3 serialises the graph's concurrent streams. */
int rt_stamp(uint64_t* buf, int idx, rt_stream_t stream);
/* rt_adamw_mat / rt_adamw_chunks — rt_adamw_flat's update (same descriptor, same arithmetic -- one definition in rt_optim.hip -- same
 * `active` / step / learning-rate device words; which products of the moment updates are fused into their adds differs between the
 * three kernels, so they agree to an ulp, not bit for bit: profiles/optim_unify_bits.txt), split into (a) the weight MATRICES, walked in tiles of 32 rows x 256 columns of [N][T*C] so that the kernel also writes the bf16
 * GEMM operands of the NEXT forward / backward from the registers that hold the new fp32 values -- what rt_weight_prep_batched
 * produced in a second pass over the masters -- and (b) everything else (biases, norm parameters, embeddings), in chunks.
 *   mat table (DEVICE int64 [njobs][8], static): {element offset of the matrix [N][T][C] in p / g / m / v, scale pointer | 0
 *     (FrozenBN scale[n] folded into the bf16 copies only), dst bf16 [N][T][C] | 0, dst_t bf16 [C][T][N] | 0, N, T, C, first tile};
 *     a job has ceil(N/32) * ceil(T*C/256) tiles; total_tiles = their sum; a matrix lies inside ONE learning-rate range.
 *     A job with dst = dst_t = 0 (an embedding table) may carry, in the scale slot, a DEVICE uint8 array [N][ceil(T*C/256)] of
 *     state bytes (0 = "m and v of this 256-column piece of row n are all zero"; start it at 1 = unknown; the kernel maintains
 *     it; reset it to 1 whenever m / v are written by anyone else).  A piece with byte 0 AND an all-zero gradient is skipped
 *     without reading p / m / v whenever (1 - lr * wd) rounds to 1.0f: with g = m = v = 0 the update is exactly that factor
 *     (torch.optim.AdamW's own fp32 no-op at the reference's lr_bert * weight_decay = 1e-9), so results are bit-identical.
 *   chunk table (DEVICE int64 [nchunks][2], static): {element offset, element count <= 16384}, both multiples of 4.
 * d->span_* are ignored (the tables say what is updated).  The caller makes jobs and chunks tile the parameters exactly once. */
int rt_adamw_mat(const rt_adamw_desc* d, const int64_t* table, int njobs, int total_tiles, rt_stream_t stream);
int rt_adamw_chunks(const rt_adamw_desc* d, const int64_t* table, int nchunks, rt_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * Host input pipeline on the device — integer / byte work, bit-exact.
 * rt_resample_u8 — one pass (axis 0 = vertical, 1 = horizontal) of Pillow's 8-bit ImagingResample, the resampler behind
 *   datasets/transforms.py:81-116 (torchvision F.resize of a PIL image, bilinear + antialias): src uint8 [n0][n1][C];
 *   out[o] = clip8((2^21 + sum_t src[lo_o + t] * k_o[t]) >> 22) with bounds[o] = {lo, taps} and coeffs[o][ksize] the 22-bit
 *   fixed-point taps (computed by the caller in double precision as Pillow does, reftr_amd/data/resample.py).
 * rt_img_collate_norm — ToTensor + Normalize (transforms.py:233-235,247-250) + nested_tensor_from_tensor_list
 *   (util/collate_fn.py:24-41): table[b] = {device pointer of image b (uint8 [h][w][3]), h, w} ->
 *   out fp32 [B,3,H,W] = (u8/255 - mean)/std zero-padded, mask uint8 [B,H,W] (1 = padding).
 * ------------------------------------------------------------------------------------------ */
int rt_resample_u8(const void* src, void* dst, const int32_t* bounds, const int32_t* coeffs, int n0, int n1, int C,
                   int out_len, int ksize, int axis, rt_stream_t stream);
int rt_img_collate_norm(const int64_t* table, float* out, uint8_t* mask, int B, int H, int W, const float* mean3,
                        const float* std3, rt_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * rt_batch_stage — one batch of any size into the fixed-size ("canvas") input buffers of a captured training step, ONE launch:
 *   img  fp32 [B,3,Hc,Wc]  <- src_img fp32 [B,3,hs,ws] (contiguous), zeros to the right and below;
 *   mask u8   [B,Hc,Wc]    <- src_mask u8 [B,hs,ws], 1 outside (NestedTensor convention: 1 = padding);
 *   boxes fp32 [B*boxes_per_image, 4] <- the B device arrays box_ptrs[b] (fp32 [box_counts[b], 4]) packed in image order, zeros behind;
 *   tgt_off int32 [B+1] = exclusive prefix sums of box_counts, num_boxes fp32 [1] = their sum (the loss kernels clamp it to >= 1);
 *   tgt_masks u8 [B,1,Hc,Wc] <- the B device arrays tm_ptrs[b] (u8 [tm_hw[2b], tm_hw[2b+1]]), zeros outside -- optional: tm_ptrs,
 *   tm_hw and tgt_masks are all NULL or all given.
 * Every byte of every destination is written by every call (the buffers hold the previous batch).  box_ptrs, box_counts, tm_ptrs and
 * tm_hw are HOST arrays of B entries: they and every size travel by value in the kernel's argument block -- no device table, no
 * host -> device copy, no synchronisation -- which bounds B by RT_BATCH_STAGE_MAX_B (RT_ERR_UNSUPPORTED above it, and for
 * B*3*Hc*Wc >= 2^32).  A box pointer may be NULL when its count is 0.  RT_ERR_BADARG, with nothing launched: a NULL required pointer,
 * a non-positive size, hs > Hc, ws > Wc, a target mask larger than the canvas, a count < 0 or > boxes_per_image.
 * 16-byte stores when Wc % 4 == 0 (fp32) / Wc % 16 == 0 (bytes) and the destination base is 16-byte aligned, element stores otherwise;
 * sources of any width and alignment.  No atomics: bit-identical from run to run.
 * ------------------------------------------------------------------------------------------ */
#define RT_BATCH_STAGE_MAX_B 64
int rt_batch_stage(const float* src_img, const uint8_t* src_mask, int B, int hs, int ws, float* img, uint8_t* mask,
                   int Hc, int Wc, const float* const* box_ptrs, const int32_t* box_counts, int boxes_per_image,
                   float* boxes, int32_t* tgt_off, float* num_boxes, const uint8_t* const* tm_ptrs, const int32_t* tm_hw,
                   uint8_t* tgt_masks, rt_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * rt_raw_stage — one batch of RAW images (decoded uint8 [h][w][3], any sizes) with boxes in pixels and raw-sized target masks into
 * the same canvas buffers, ONE launch: what rt_resample_u8 x 2 + rt_img_collate_norm(pad_to) + DeviceInputPipeline._target +
 * rt_batch_stage write, bit for bit.  Per image b (HOST values, all by value in the kernel's argument block like rt_batch_stage's):
 *   src[b] uint8 [h[b]][w[b]][3]; the resized size oh[b] x ow[b] (reftr_amd/data/resample.py size_with_aspect_ratio, <= the canvas);
 *   box_ptr[b] fp32 [box_n[b], 4] xyxy pixels of the raw frame (NULL when box_n[b] = 0); tm_ptr[b] one byte per pixel [h[b]][w[b]]
 *   (read only when tgt_masks is given); rw[b] = (float)((double)ow / w), rh[b] = (float)((double)oh / h).
 *   img fp32 [B,3,Hc,Wc]: Pillow's 8-bit bilinear resample (horizontal pass, clip8'd uint8 intermediate, vertical pass -- the filter
 *     taps are computed in the kernel, in double, operation for operation as reftr_amd/data/resample.py taps), then
 *     ((float)px / 255.0f - mean[c]) / std[c]; zeros outside oh x ow;
 *   mask u8 [B,Hc,Wc]: 0 inside oh x ow, 1 outside;
 *   tgt_masks u8 [B,1,Hc,Wc] | NULL: torch's `nearest` of the raw mask, src = min((int)floorf(dst * ((float)in / out)), in - 1) per
 *     axis, as 0 / 1 (non-zero source byte -> 1); zeros outside oh x ow;
 *   boxes fp32 [B*boxes_per_image, 4]: cxcywh normalised -- x * rw, y * rh, then (x0 + x1) / 2, x1 - x0, then / (float)ow, oh, no fused
 *     multiply-add -- packed in image order, zeros behind; tgt_off int32 [B+1]; num_boxes fp32 [1], as rt_batch_stage.
 * A workgroup owns one RT_RAW_STAGE_TILE_H x RT_RAW_STAGE_TILE_W tile of one image's canvas: it resamples horizontally, into LDS, the
 * source rows its tile's vertical taps need; the uint8 intermediate never exists in memory.  The LDS budget bounds the down-scale:
 * h > RT_RAW_STAGE_MAX_SCALE * oh or w > RT_RAW_STAGE_MAX_SCALE * ow on any image -> RT_ERR_UNSUPPORTED, nothing launched (also
 * B > RT_BATCH_STAGE_MAX_B, Hc * Wc >= 2^31).  RT_ERR_BADARG, nothing launched: a NULL required pointer, a non-positive size,
 * oh > Hc, ow > Wc, a count < 0 or > boxes_per_image.  Every byte of every destination is written by every call; 16-byte stores when
 * Wc % 4 == 0 (fp32) / Wc % 16 == 0 (bytes) and the base is 16-byte aligned, element stores otherwise; no atomics: the same bits
 * from run to run.
 * rt_resample_taps — the kernel's tap function alone, for tests: bounds int32 [out_size][2] = {first index, count}, coeffs int32
 *   [out_size][ksize] (zero behind the count); RT_ERR_BADARG for ksize < 2 * ceil(max(in / out, 1)) + 1.
 * ------------------------------------------------------------------------------------------ */
#define RT_RAW_STAGE_MAX_SCALE 4
#define RT_RAW_STAGE_TILE_H 32
#define RT_RAW_STAGE_TILE_W 64
typedef struct rt_raw_stage_args {
    float*   img;
    uint8_t* mask;
    uint8_t* tgt_masks;     /* | NULL */
    float*   boxes;
    int32_t* tgt_off;
    float*   num_boxes;
    int32_t  B, Hc, Wc, boxes_per_image;
    float    mean[3], std[3];
    const uint8_t* src[RT_BATCH_STAGE_MAX_B];
    const float*   box_ptr[RT_BATCH_STAGE_MAX_B];
    const uint8_t* tm_ptr[RT_BATCH_STAGE_MAX_B];
    int32_t h[RT_BATCH_STAGE_MAX_B], w[RT_BATCH_STAGE_MAX_B], oh[RT_BATCH_STAGE_MAX_B], ow[RT_BATCH_STAGE_MAX_B];
    int32_t box_n[RT_BATCH_STAGE_MAX_B];
    float   rw[RT_BATCH_STAGE_MAX_B], rh[RT_BATCH_STAGE_MAX_B];
} rt_raw_stage_args;
int rt_raw_stage(const rt_raw_stage_args* a, rt_stream_t stream);
int rt_resample_taps(int in_size, int out_size, int32_t* bounds, int32_t* coeffs, int ksize, rt_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * rt_hsv_jitter — the reference's RandomIntensitySaturation (datasets/transforms.py:266-285) on a batch of RAW images, in front of
 * rt_raw_stage, ONE launch: per image b, dst[b] = the 8-bit RGB -> HSV -> gains -> RGB round trip of src[b] (uint8 [h[b]][w[b]][3]),
 * the bytes of reftr_amd/data/jitter.py `apply`, bit for bit.  That module is the definition (OpenCV's scalar 8-bit paths restated
 * operation for operation; not pinned against a cv2 build):
 *   RGB -> HSV in integers, hsv_shift = 12: v = max, d = v - min, s = (d * sdiv[v] + 2048) >> 12, h = (h0 * hdiv[d] + 2048) >> 12
 *     (arithmetic shift; + 180 when negative; H in [0, 180)), sdiv[i] = rint((255 << 12) / (1.0 * i)), hdiv[i] = rint((180 << 12) /
 *     (6.0 * i)) in double, round half to even, both 0 at i = 0 -- the two tables are computed in the kernel, into LDS;
 *   gains: y = (float)x * gain, clipped to [0, 255] only when gain > 1, x' = (uint8)(int)y -- S with s_gain[b], V with v_gain[b]
 *     (the reference never scales S: its gain is 1; a gain of exactly 1 keeps the byte);
 *   HSV -> RGB in fp32 with NO fused multiply-add: hf = h * (6.f / 180.f), sf = s' * (1.f / 255.f), vf = v' * (1.f / 255.f), the four
 *     products {vf, vf * (1 - sf), vf * (1 - sf * f), vf * (1 - sf * (1 - f))} chosen by the sector, each channel
 *     clamp(rintf(c * 255.f), 0, 255), round half to even.
 * The round trip alone moves bytes: gains (1, 1) are not the identity.
 * Every per-image fact (HOST values) rides by value in the kernel's argument block, as rt_raw_stage's do.  An image is a flat run of
 * h * w pixels and a thread takes 16 consecutive ones (48 bytes): three 16-byte loads and three 16-byte stores where the unit lies
 * wholly inside the image and src[b] and dst[b] are 16-byte aligned, byte accesses otherwise; no byte at or behind 3 * h * w of an
 * image is read or written.  dst[b] == src[b] is allowed (a thread reads its unit before it writes it), a partial overlap is not.
 * No atomics: the same bits from run to run.  Nothing is launched on an error: RT_ERR_UNSUPPORTED for B > RT_BATCH_STAGE_MAX_B or
 * 3 * h * w >= 2^31; RT_ERR_BADARG for a NULL pointer, B <= 0, a non-positive size, a gain that is negative, NaN or infinite.
 * ------------------------------------------------------------------------------------------ */
typedef struct rt_hsv_jitter_args {
    int32_t B;
    const uint8_t* src[RT_BATCH_STAGE_MAX_B];   /* [h][w][3] */
    uint8_t*       dst[RT_BATCH_STAGE_MAX_B];   /* [h][w][3]; dst[b] == src[b] allowed, partial overlap not */
    int32_t h[RT_BATCH_STAGE_MAX_B], w[RT_BATCH_STAGE_MAX_B];
    float   s_gain[RT_BATCH_STAGE_MAX_B], v_gain[RT_BATCH_STAGE_MAX_B];
} rt_hsv_jitter_args;
int rt_hsv_jitter(const rt_hsv_jitter_args* a, rt_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * rt_cem_fwd / rt_cem_bwd — the CEM block of RefTRSeg (--ablation cem_loss, models/reftr_segmentation.py:16-41) for the one
 * query per image of RES: u_b = c3(hs_b) (hs bf16 [B, E] = last decoder output, w3 [16, E], b3 [16]), res bf16 [B*HW, ld] =
 * MaskHeadSmallConv's last feature map (16 channels in front of the padding), a_p = res_p . w2 + b2,
 *   energy_b = sum_p softmax_p(a)_p * clamp((cos(u_b, res_p) + 1) / 2, 1e-6, 1 - 1e-6),  loss = -sum_b log(energy_b + 1e-6) / B
 * (the softmax over the single query, c1, is the constant 1).  One workgroup per image, online softmax (one pass over the pixels).
 * Backward (g = d loss): dres fp32 [B*HW, lddr] += d res, dhs [B, E] = d hs, dw3 / db3 / dw2 += (d c2.bias = d c1 = 0 exactly).
 * ------------------------------------------------------------------------------------------ */
typedef struct rt_cem_desc {
    const void*  hs;        /* bf16 [B, E] */
    const float* w3;        /* [16, E] */
    const float* b3;        /* [16] */
    const void*  res;
    const float* w2;        /* [16] */
    const float* b2;        /* [1] */
    float* u;               /* [B, 16]: written by the forward, read by the backward */
    float* energy;          /* [B] */
    float* stats;           /* [B, 2] = {max_p a_p, sum_p exp(a_p - max)} */
    float* loss;            /* [1] */
    const float* g;         /* backward: device scalar d loss */
    float* dres; float* dhs; float* dw3; float* db3; float* dw2;
    int32_t B, HW, ld, lddr, E, reserved;
} rt_cem_desc;
int rt_cem_fwd(const rt_cem_desc* d, rt_stream_t stream);
int rt_cem_bwd(const rt_cem_desc* d, rt_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * Evaluation post-processing, exact decisions / selections.
 * rt_mask_postprocess — PostProcessSegm.forward (models/reftr_segmentation.py:282-302): pred fp32 [B*Q, h, w] mask logits ->
 *   masks uint8 [B, Q, max_h, max_w] = sigmoid(bilinear(pred -> max_h x max_w, align_corners=False)) > threshold inside the
 *   image's own (sizes[b] = {img_h, img_w}) top-left corner, 0 outside it (the reference's crop = the [:img_h, :img_w] view);
 *   masks_origin (optional) uint8, image b's block at origin_off[b] with shape [Q, orig_h, orig_w] (orig[b] = {orig_h, orig_w}) =
 *   nearest resize of the cropped mask (torch 'nearest': src = min(floor(dst * in / out), in - 1)); max_origin = max_b orig_h*orig_w.
 * rt_box_postprocess  — PostProcessVGMultiPhrase.forward (models/post_process.py:45-83): boxes fp32 [B,P,K,4] cxcywh, valid uint8
 *   [B,P,K] (phrase_mask) -> out fp32 [B,P,4]: row r of image b = xyxy of prediction 0 of its r-th VALID phrase (phrase order
 *   kept), times {w,h,w,h} when sizes (fp32 [B,2] = {img_h, img_w}) is given; counts int32 [B] = valid phrases per image.
 * ------------------------------------------------------------------------------------------ */
typedef struct rt_mask_post_desc {
    const float*   pred;
    const int32_t* sizes;
    const int32_t* orig;
    const int64_t* origin_off;
    uint8_t* masks;
    uint8_t* masks_origin;
    int32_t B, Q, h, w, max_h, max_w;
    int64_t max_origin;
    float   threshold;
} rt_mask_post_desc;
int rt_mask_postprocess(const rt_mask_post_desc* d, rt_stream_t stream);
typedef struct rt_box_post_desc {
    const float*   boxes;
    const uint8_t* valid;
    const float*   sizes;
    float*   out;
    int32_t* counts;
    int32_t B, P, K;
} rt_box_post_desc;
int rt_box_postprocess(const rt_box_post_desc* d, rt_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * rt_eval_metrics — the metric stage of engine_vg.evaluate (engine_vg.py:127-152) for one batch, running totals kept on the device.
 * Two launches on `stream`, no floating-point atomics, nothing the caller has to clear, the same bits from run to run:
 *   (a) mask partials (only when `masks` is given), grid (chunk, image): a workgroup counts I = sum(pred & tgt), U = sum(pred | tgt)
 *       as integers over its run of RT_EVAL_CHUNK pixels of the image's ih x iw (= sizes[b]) pixels -- pred = query 0 of image b in
 *       `masks` (uint8 [B, Q, max_h, max_w], what rt_mask_postprocess wrote), read at pitch max_w inside [:ih, :iw] only; the target at
 *       its own pitch -- and stores {I, U} to partials[b][chunk] (int32 workspace of B * ceil(max_h * max_w / RT_EVAL_CHUNK) * 2 words);
 *   (b) finish, ONE workgroup, image ascending then row ascending:
 *       boxes: the r-th VALID phrase of image b (rt_box_postprocess's ordered selection of pred_boxes fp32 [B, P, K, 4] cxcywh by valid
 *       uint8 [B, P, K]) is paired with target box r, at most n_b rows; IoU in fp32, every operation un-fused in util/box_ops.py's
 *       order (box_cxcywh_to_xyxy of both, then box_iou(target, pred): areas, max / min, clamp(min=0), inter = w * h,
 *       union = (a1 + a2) - inter, inter / union; 0 / 0 stays NaN) -> iou_det fp32 [B, P], unused rows 0;
 *       masks: the partials added in chunk order to int64 I_b, U_b -> iu int64 [B, 2] = {I_b, U_b}, iou_seg fp32 [B] =
 *       (float)I_b / (float)U_b (NaN when both are empty, as util/box_ops.py mask_iou); an image whose mask pointer is 0 is left out
 *       (iou_seg 0, iu 0, not counted);
 *       accumulators: `acc` = RT_EVAL_SLOTS words of 8 bytes, int64 but for the two double sums; hits are the samples whose fp32 IoU is
 *       STRICTLY greater than the fp32 value nearest 0.5, 0.6, 0.7, 0.8, 0.9 (a NaN is a miss, and leaves the sum NaN as torch's does).
 *       reset != 0: the accumulators start from zero in this same launch (the first batch of an evaluation).
 * table (DEVICE int64 [B][5]) = {pointer to image b's target boxes fp32 [n_b, 4] cxcywh, n_b, pointer to its target mask (1 byte per
 * pixel, non-zero = set, row pitch = its width; 0: none), mask height, mask width}.  masks == NULL: the box part only (sizes, partials,
 * iou_seg, iu may be NULL).  RT_ERR_UNSUPPORTED for max_h * max_w >= 2^31.
 * ------------------------------------------------------------------------------------------ */
enum { RT_EVAL_DET_N = 0, RT_EVAL_DET_HIT = 1 /* .. 5 */, RT_EVAL_SEG_N = 6, RT_EVAL_SEG_HIT = 7 /* .. 11 */, RT_EVAL_SEG_I = 12,
       RT_EVAL_SEG_U = 13, RT_EVAL_DET_SUM = 14 /* double */, RT_EVAL_SEG_SUM = 15 /* double */, RT_EVAL_SLOTS = 16 };
#define RT_EVAL_CHUNK 16384
typedef struct rt_eval_metrics_args {
    const float*   pred_boxes;
    const uint8_t* valid;
    const int64_t* table;
    const uint8_t* masks;
    const int32_t* sizes;
    int32_t* partials;
    float*   iou_det;
    float*   iou_seg;
    int64_t* iu;
    void*    acc;
    int32_t B, P, K, Q, max_h, max_w;
    int32_t reset;
} rt_eval_metrics_args;
int rt_eval_metrics(const rt_eval_metrics_args* a, rt_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * Evaluation on the batch canvas: the post-processing and metric tail of one canvas batch with every per-batch fact in DEVICE memory,
 * so that it can sit inside a captured graph and be replayed without an argument change.
 * rt_eval_facts — one small launch per batch, outside the graph: gathers the B device int64 arrays the loader delivers --
 *   size_ptrs[b] -> {img_h, img_w}, orig_ptrs[b] -> {orig_h, orig_w} (orig_ptrs NULL: the size), id_ptrs[b] -> the image id (id_ptrs
 *   NULL: -1) -- and the HOST int32 pairs tm_hw[2b], tm_hw[2b+1] (target mask height, width; NULL: 0, 0) into
 *   facts int32 [B, 6] = {img_h, img_w, orig_h, orig_w, mask_h, mask_w} and image_ids int64 [B].  The pointer arrays are HOST arrays
 *   of B entries that travel by value in the kernel's argument block, as rt_batch_stage's do (B <= RT_BATCH_STAGE_MAX_B, else
 *   RT_ERR_UNSUPPORTED; RT_ERR_BADARG for a NULL required pointer or entry, B <= 0).
 * rt_eval_canvas — two launches, replacing rt_box_postprocess + rt_mask_postprocess + rt_eval_metrics + the table copy:
 *   (a) mask partials (only when pred_masks is given), grid (chunk, image): for every pixel of the image's scored rectangle
 *       ({img_h, img_w} of `facts`, clamped to the target mask's own extent and to the canvas) the decision of query 0 is taken from the
 *       logits pred_masks fp32 [B, Q, h, w] by rt_mask_postprocess's own function with the canvas Hc x Wc as the frame, the target byte
 *       is read from tgt_masks uint8 [B, 1, Hc, Wc] (what rt_batch_stage wrote) at pitch Wc, and the integer {I, U} of the workgroup's
 *       RT_EVAL_CHUNK pixels go to partials[b][chunk] (int32, B * ceil(Hc * Wc / RT_EVAL_CHUNK) * 2 words).  No uint8 frame exists;
 *   (b) finish, ONE wave, rt_eval_metrics' finish in its order (image ascending, row ascending; un-fused box arithmetic; int64 counts,
 *       double sums) with the target boxes of image b = rows tgt_off[b] .. tgt_off[b+1] of tgt_boxes (rt_batch_stage's packed buffer of
 *       tgt_rows rows) -> iou_det [B, P], iou_seg [B], iu [B, 2], acc (never reset here: the caller zeroes acc once).  It also writes
 *       slot s = cursor[0] of a results ring: ring_boxes fp32 [slots, B, P, 4] = rt_box_postprocess's output scaled by {orig_w, orig_h}
 *       (unused rows 0), ring_counts int32 [slots, B] = valid phrases per image, ring_ids int64 [slots, B] = image_ids; then
 *       cursor[0] = s + 1.  s >= slots: nothing is written to the ring, cursor[1] = 1 (overflow) and cursor[0] stays.
 *   `cursor` is int32 [2] in device memory, zeroed by the caller with acc.  No atomics; the same bits from run to run.
 *   `veto` (optional): a device word read by the finish; non-zero -> this batch is NOT kept: acc, ring and cursor stay as they were
 *   (iou_det / iou_seg / iu are still written).  The evaluation loop hands the cooperative decoder's failure word, so that a batch
 *   whose forward is run again is counted once.
 *   RT_ERR_BADARG: a NULL required pointer, a non-positive size; RT_ERR_UNSUPPORTED: B > RT_BATCH_STAGE_MAX_B, Hc * Wc >= 2^31.
 * ------------------------------------------------------------------------------------------ */
int rt_eval_facts(const int64_t* const* size_ptrs, const int64_t* const* orig_ptrs, const int64_t* const* id_ptrs,
                  const int32_t* tm_hw, int B, int32_t* facts, int64_t* image_ids, rt_stream_t stream);
typedef struct rt_eval_canvas_args {
    const float*   pred_boxes;     /* fp32 [B, P, K, 4] cxcywh */
    const uint8_t* valid;          /* uint8 [B, P, K] */
    const float*   tgt_boxes;      /* fp32 [tgt_rows, 4] cxcywh, packed in image order */
    const int32_t* tgt_off;        /* int32 [B + 1] */
    const int32_t* facts;          /* int32 [B, 6] */
    const int64_t* image_ids;      /* int64 [B] */
    const float*   pred_masks;     /* fp32 [B, Q, h, w] | NULL: the box part only */
    const uint8_t* tgt_masks;      /* uint8 [B, 1, Hc, Wc] */
    int32_t* partials;
    float*   iou_det;
    float*   iou_seg;
    int64_t* iu;
    void*    acc;
    float*   ring_boxes;
    int32_t* ring_counts;
    int64_t* ring_ids;
    int32_t* cursor;
    const int32_t* veto;           /* int32 [1] | NULL */
    int32_t B, P, K, Q, h, w, Hc, Wc, tgt_rows, slots;
    float   threshold;
} rt_eval_canvas_args;
int rt_eval_canvas(const rt_eval_canvas_args* a, rt_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * Evaluation of RAW batches on the batch canvas (engine_vg.evaluate_raw): rt_eval_canvas runs unchanged behind rt_raw_stage, and the
 * predicted mask is scored a second time at the annotation's OWN resolution, against the raw target mask untouched.
 * rt_eval_raw_facts — one small launch per batch, outside the graph; what rt_eval_facts gathers from device tensors, from HOST values
 *   that travel by value in the kernel's argument block, as rt_predict_facts' do (B <= RT_BATCH_STAGE_MAX_B): per image b the resized
 *   size img_h[b], img_w[b] (<= the canvas Hc x Wc), the raw size orig_h[b], orig_w[b], image_id[b] (read when has_ids != 0) and
 *   tm_ptr[b], the device address of the raw target mask (one byte per pixel, [orig_h][orig_w]; read when mask_table is given).
 *   It writes facts int32 [B, 6] = {img_h, img_w, orig_h, orig_w, img_h, img_w} -- rt_eval_facts' layout; the mask extent words equal
 *   the resized size, the extent of what rt_raw_stage staged -- image_ids int64 [B] (-1 without ids) and, when given, mask_table
 *   int64 [B] = the addresses.  max_pixels: the bound rt_eval_orig's grid was sized for.
 *   RT_ERR_BADARG, nothing launched: a NULL required pointer, B <= 0, a non-positive size, img_h > Hc, img_w > Wc,
 *   orig_h * orig_w > max_pixels, mask_table given with a NULL tm_ptr[b].  RT_ERR_UNSUPPORTED: B > RT_BATCH_STAGE_MAX_B,
 *   max_pixels >= 2^31.
 * rt_eval_orig — two launches behind rt_eval_canvas, reading device memory only; no atomics, the same bits from run to run:
 *   (a) mask partials, grid (ceil(max_pixels / RT_EVAL_CHUNK), B) -- fixed by max_pixels, not by the batch (the facts change between
 *       replays): a workgroup whose chunk starts at or behind the image's orig_h * orig_w leaves at once and writes nothing.  Pixel
 *       i = y * orig_w + x of the raw frame: the prediction is rt_mask_postprocess's masks_origin with the canvas Hc x Wc as the frame
 *       (rt_predict_canvas (b)): its decision function on query 0 of pred_masks fp32 [B, Q, h, w] at the `nearest` sources of y in
 *       img_h and x in img_w; the target is byte i of the image's raw mask (mask_table[b]), non-zero = set, not resampled.  One
 *       thread per 16 consecutive bytes: it divides once, walks its pixels row by row and reads the target with ONE 16-byte load
 *       where the unit lies wholly inside orig_h * orig_w and its address is 16-byte aligned, byte loads otherwise; no byte at or
 *       behind orig_h * orig_w is read.  Integer {I, U} of the workgroup's RT_EVAL_CHUNK pixels -> partials[b][chunk] (int32
 *       [B, ceil(max_pixels / RT_EVAL_CHUNK), 2]).  Every logit index is clamped: foreign facts cannot direct a read outside image
 *       b's plane.  An image that cannot be scored -- a zero table entry, a non-positive size, orig_h * orig_w > max_pixels --
 *       contributes nothing;
 *   (b) finish, ONE wave, image ascending: the first ceil(orig_h * orig_w / RT_EVAL_CHUNK) partials of the image added to int64 ->
 *       iu int64 [B, 2] = {I_b, U_b}, iou_seg fp32 [B] = (float)I_b / (float)U_b (NaN when both are empty; an image that cannot be
 *       scored: 0, {0, 0}, not counted), and `acc` = RT_EVAL_ORIG_SLOTS words of 8 bytes, int64 but for the double sum, counted as
 *       rt_eval_metrics counts its mask samples (hits: fp32 IoU STRICTLY above the fp32 value nearest 0.5 .. 0.9; a NaN is a miss
 *       and leaves the sum NaN).  acc is never reset here.  `veto` (optional): non-zero -> acc stays as it was (iou_seg and iu are
 *       still written), as rt_eval_canvas.
 *   RT_ERR_BADARG: a NULL required pointer, a non-positive size; RT_ERR_UNSUPPORTED: B > RT_BATCH_STAGE_MAX_B, max_pixels, h * w or
 *   Hc * Wc >= 2^31.
 * ------------------------------------------------------------------------------------------ */
typedef struct rt_eval_raw_facts_args {
    int32_t* facts;                /* int32 [B, 6] */
    int64_t* image_ids;            /* int64 [B] */
    int64_t* mask_table;           /* int64 [B] | NULL */
    int64_t  max_pixels;
    int32_t  B, Hc, Wc, has_ids;
    int32_t  img_h[RT_BATCH_STAGE_MAX_B], img_w[RT_BATCH_STAGE_MAX_B], orig_h[RT_BATCH_STAGE_MAX_B], orig_w[RT_BATCH_STAGE_MAX_B];
    int64_t  image_id[RT_BATCH_STAGE_MAX_B];
    const uint8_t* tm_ptr[RT_BATCH_STAGE_MAX_B];
} rt_eval_raw_facts_args;
int rt_eval_raw_facts(const rt_eval_raw_facts_args* a, rt_stream_t stream);
/* rt_eval_orig's accumulator slots (macros, not enumerators: the RT_EVAL_* enum above is rt_eval_metrics' 16 slots and nothing else) */
#define RT_EVAL_ORIG_N 0
#define RT_EVAL_ORIG_HIT 1         /* .. 5 */
#define RT_EVAL_ORIG_I 6
#define RT_EVAL_ORIG_U 7
#define RT_EVAL_ORIG_SUM 8         /* double */
#define RT_EVAL_ORIG_SLOTS 9
typedef struct rt_eval_orig_args {
    const float*   pred_masks;     /* fp32 [B, Q, h, w] */
    const int32_t* facts;          /* int32 [B, 6] */
    const int64_t* mask_table;     /* int64 [B] */
    int32_t* partials;             /* int32 [B, ceil(max_pixels / RT_EVAL_CHUNK), 2] */
    float*   iou_seg;              /* fp32 [B] */
    int64_t* iu;                   /* int64 [B, 2] */
    void*    acc;                  /* RT_EVAL_ORIG_SLOTS words of 8 bytes */
    const int32_t* veto;           /* int32 [1] | NULL */
    int64_t  max_pixels;
    int32_t  B, Q, h, w, Hc, Wc;
    float    threshold;
} rt_eval_orig_args;
int rt_eval_orig(const rt_eval_orig_args* a, rt_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * Prediction on the batch canvas: the RESULT tail of one canvas batch -- boxes in original pixels and, for RES, the mask at the
 * original resolution (PostProcessSegm's masks_origin) -- with every per-batch fact in DEVICE memory, so that it sits inside a
 * captured graph behind the forward and is replayed without an argument change.
 * rt_predict_facts — one small launch per batch, outside the graph.  Per image b the HOST values img_h[b], img_w[b] (the resized
 *   size, <= the canvas Hc x Wc) and orig_h[b], orig_w[b] (the original size) travel by value in the kernel's argument block, as
 *   rt_raw_stage's do (B <= RT_BATCH_STAGE_MAX_B), with Q (mask queries per image; 0: a model without masks) and `capacity`, the
 *   size of the mask buffer in bytes.  Image b's mask block is Q * orig_h * orig_w bytes and starts at a 16-byte unit:
 *   off16[0] = 0, off16[b + 1] = off16[b] + ceil(Q * orig_h * orig_w / 16).  It writes
 *   facts int32 [B, RT_PREDICT_FACTS_WORDS] = {img_h, img_w, orig_h, orig_w, off16[b], off16[b + 1], off16[B], 0}.
 *   RT_ERR_UNSUPPORTED: B > RT_BATCH_STAGE_MAX_B, 16 * off16[B] >= 2^31.  RT_ERR_BADARG, nothing launched: a NULL pointer, B <= 0,
 *   Q < 0, capacity < 0, a non-positive size, img_h > Hc, img_w > Wc, 16 * off16[B] > capacity.
 * rt_predict_canvas — at most two launches, reading device memory only; no atomics, plain loads and stores, the same bits from run
 *   to run:
 *   (a) boxes, one wave per image: out_boxes fp32 [B, P, 4] = rt_box_postprocess's rows (the image's valid phrases in masked_select
 *       order, prediction 0 of each, cxcywh -> xyxy) times {orig_w, orig_h, orig_w, orig_h} of `facts`, unused rows 0 -- the rows
 *       rt_eval_canvas writes to its ring, by the same function; out_counts int32 [B] = valid phrases per image;
 *   (b) masks (only when pred_masks fp32 [B, Q, h, w] is given): byte i < Q * oh * ow of image b's block (out_masks + 16 * off16[b])
 *       is pixel (q, y, x) = (i / (oh * ow), (i / ow) % oh, i % ow) of the original frame: rt_mask_postprocess's masks_origin with the
 *       canvas Hc x Wc as the frame, i.e. its decision function on logits[b][q] at the `nearest` sources of y in img_h and x in
 *       img_w, as 0 / 1.  The bytes from Q * oh * ow to the end of the block's last 16-byte unit are written 0.  One thread per
 *       16-byte unit, ONE 16-byte store each (out_masks must be 16-byte aligned, else RT_ERR_BADARG); the thread divides once per
 *       unit and walks its sixteen pixels row by row.  Every byte of [0, 16 * off16[B]) is rewritten by every call (the buffer holds
 *       the previous batch); no byte at or past 16 * off16[B], and none past `capacity`, is touched, whatever `facts` holds.  The
 *       grid is fixed by `capacity`, not by the batch (facts change between replays): workgroups behind the total leave at once.
 *   RT_ERR_BADARG: a NULL required pointer, a non-positive size, capacity < 0, out_masks not 16-byte aligned; RT_ERR_UNSUPPORTED:
 *   B > RT_BATCH_STAGE_MAX_B, capacity >= 2^31, h * w or Hc * Wc >= 2^31.
 * ------------------------------------------------------------------------------------------ */
#define RT_PREDICT_FACTS_WORDS 8
typedef struct rt_predict_facts_args {
    int32_t* facts;                /* int32 [B, RT_PREDICT_FACTS_WORDS] */
    int64_t  capacity;             /* bytes of the mask buffer */
    int32_t  B, Q, Hc, Wc;
    int32_t  img_h[RT_BATCH_STAGE_MAX_B], img_w[RT_BATCH_STAGE_MAX_B], orig_h[RT_BATCH_STAGE_MAX_B], orig_w[RT_BATCH_STAGE_MAX_B];
} rt_predict_facts_args;
int rt_predict_facts(const rt_predict_facts_args* a, rt_stream_t stream);
typedef struct rt_predict_canvas_args {
    const float*   pred_boxes;     /* fp32 [B, P, K, 4] cxcywh */
    const uint8_t* valid;          /* uint8 [B, P, K] */
    const int32_t* facts;          /* int32 [B, RT_PREDICT_FACTS_WORDS] */
    const float*   pred_masks;     /* fp32 [B, Q, h, w] | NULL: the box part only */
    float*   out_boxes;            /* fp32 [B, P, 4] */
    int32_t* out_counts;           /* int32 [B] */
    uint8_t* out_masks;            /* `capacity` bytes, 16-byte aligned (with pred_masks) */
    int64_t  capacity;
    int32_t  B, P, K, Q, h, w, Hc, Wc;
    float    threshold;
} rt_predict_canvas_args;
int rt_predict_canvas(const rt_predict_canvas_args* a, rt_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * rt_comm_* — the data-parallel gradient exchange: what the reference gets from
 * torch.nn.parallel.DistributedDataParallel (main_vg.py:290-296) after util/misc.py:392-431 set up one process per GPU.
 * RCCL over xGMI, bound at run time (dlopen: the copy the process already holds -- torch.distributed's -- or the system's);
 * RT_ERR_UNSUPPORTED when no RCCL can be loaded, RT_ERR_COMM (+ a line on stderr) when RCCL reports an error.
 *   rt_comm_unique_id  rank 0 fills 128 opaque bytes; the caller carries them to every rank (any out-of-band channel);
 *   rt_comm_init       collective over all ranks (one process per GPU, the device current at the call is the rank's);
 *   rt_comm_allreduce  in-place SUM all-reduce of `n` buffers (device pointers, element counts) of one dtype, issued as one
 *                      group on `stream` -- asynchronous: ordered behind the work already enqueued on `stream`, the caller
 *                      joins its compute stream with an event;
 *   rt_comm_destroy    releases the communicator.
 * Thread-compatible: one caller thread per device.
 * ------------------------------------------------------------------------------------------ */
typedef void* rt_comm_t;
enum { RT_COMM_F32 = 0, RT_COMM_BF16 = 1 };
int rt_comm_unique_id(void* id128);
int rt_comm_init(const void* id128, int rank, int world, rt_comm_t* out);
int rt_comm_allreduce(rt_comm_t comm, void* const* bufs, const int64_t* counts, int n, int dtype, rt_stream_t stream);
int rt_comm_destroy(rt_comm_t comm);

/* --------------------------------------------------------------------------------------------
 * rt_decoder_fwd — the TransformerDecoder stack of the referring queries as ONE cooperative launch
 * (models/modeling/transformer.py:105-143 the stack, :231-252 one layer, forward_post; one query per image: M = B rows, the
 * self-attention over a single key is the V projection with its per-head probability dropout).  Equivalent, operation for
 * operation, to the launched chain  rt_conv_gemm (self_attn.v, out_proj) -> rt_layernorm_fwd -> rt_conv_gemm (multihead_attn.q) ->
 * rt_attn_fwd -> rt_conv_gemm (out_proj) -> rt_layernorm_fwd -> rt_conv_gemm (linear1, linear2) -> rt_layernorm_fwd  per layer:
 * the saved tensors it writes are the chain's (bit-identical), so the backward is unchanged.  Workgroups stay resident and hand
 * the row block from stage to stage through global memory as tagged 8-byte units (csrc/rt_decoder.hip).
 *   handoff: RT_DEC_HANDOFF_BYTES of device memory, zeroed ONCE by the caller and then owned by the launches (word 0 = launch
 *            epoch, advanced by every launch; word 1 is set to 1 if a consumer gave up waiting for its rows).  Launches that
 *            share a buffer must be ordered on one stream.
 *   K / V of layer l: bf16 [B * S, ldkv] (multihead_attn.k / .v of memory + pos / memory, computed beforehand for every layer).
 * Supported: width 256, 8 heads, F = 2048, M <= 16, S <= 768, n_layers <= RT_DEC_MAX_LAYERS; else RT_ERR_UNSUPPORTED.
 * ------------------------------------------------------------------------------------------ */
#define RT_DEC_MAX_LAYERS 8
#define RT_DEC_HANDOFF_BYTES (256 + 16 * 256 * 36 + 16 * 2048 * 4)
typedef struct rt_decoder_layer_fwd {
    const void *Wv, *Wo, *Wq, *Wo2, *W1, *W2;            /* bf16 [N][K]: self_attn v / out_proj, multihead_attn q / out_proj, linear1 / 2 */
    const float *bv, *bo, *bq, *bo2, *b1, *b2;
    const float *g1, *be1, *g2, *be2, *g3, *be3;         /* norm1..3 weight / bias */
    const void *k2, *v2;
    void *o, *t1q16, *q2, *o2, *t2_16, *hdn, *t3_16;      /* bf16 saved tensors: [M,256] (hdn: [M,F]) */
    float *u, *u2, *u3;                                   /* fp32 pre-norm sums [M,256] */
    float *mean1, *rstd1, *mean2, *rstd2, *mean3, *rstd3; /* [M] */
    float *lse2;                                          /* [B, H] */
    float *t3_f32;                                        /* norm3 output rows, fp32 [M,256] (the shared decoder norm's input) */
    uint32_t seed_ad, seed_d1, seed_ad2, seed_d2, seed_dh, seed_d3;   /* dropout sites, in the chain's order */
} rt_decoder_layer_fwd;
typedef struct rt_decoder_fwd_desc {
    rt_decoder_layer_fwd layer[RT_DEC_MAX_LAYERS];
    const float*   t32;        /* [M,256] the stack's input (tgt) */
    const void*    t16;        /* bf16 copy */
    const float*   qpos;       /* [M,256] query_pos */
    const uint8_t* kpm;        /* [B, S] key padding mask (1 = ignore) or NULL */
    uint32_t*      handoff;
    const uint32_t* seed_dev;  /* optional, see rt_conv_gemm_desc */
    int32_t n_layers, M, H, S, F, ldkv;
    float   drop_p, eps, scale;
} rt_decoder_fwd_desc;
int rt_decoder_fwd(const rt_decoder_fwd_desc* d, rt_stream_t stream);
/* rt_decoder_bwd -- the backward of the same stack as one cooperative launch: per layer LayerNorm backward (norm3, norm2, norm1,
 * recomputed by every consumer), the six M <= 16 backward-data products, the one-query attention backward; the launched chain
 * rt_layernorm_bwd -> rt_conv_gemm (linear2^T gate, linear1^T + res) -> rt_layernorm_bwd -> rt_conv_gemm (out_proj^T) -> rt_attn_bwd
 * -> rt_conv_gemm (q^T) -> rt_layernorm_bwd -> rt_conv_gemm (out_proj^T head mask, v^T + res) of transformer.py:231-252's backward.
 * It writes what the chain writes for the launches that stay outside: the bf16 dy operands of the (grouped) weight gradients, the
 * LayerNorm parameter-gradient partials (rt_ln_param_grad_grouped's format, (M+3)/4 blocks), dK / dV of the cross-attention (the
 * M = B*S memory-gradient products and weight gradients), the gradient w.r.t. the stack's input and query_pos.  Same hand-off buffer
 * and limits as rt_decoder_fwd. */
typedef struct rt_decoder_layer_bwd {
    const void *WT2, *WT1, *WTo2, *WTq, *WTo, *WTv;      /* bf16 backward-data operands [K_in][N_out]: linear2, linear1, multihead_attn.out_proj / q, self_attn.out_proj / v */
    const float *g1, *g2, *g3;                            /* norm1..3 weight */
    const float *u, *u2, *u3, *mean1, *rstd1, *mean2, *rstd2, *mean3, *rstd3;      /* saved by the forward */
    const void *hdn, *q2, *k2, *v2, *o2;
    const float *lse2;
    const float *dnorm;                                   /* [M,256]: gradient w.r.t. this layer's output through the shared decoder norm */
    void *du3b, *dhdn, *du2b, *dq2, *dub, *dv;            /* bf16 [M,256] (dhdn [M,F]): dy operands of the weight gradients */
    void *dk2, *dv2;                                      /* bf16 [B*S, ldkv] */
    void *dk2p, *dv2p;                                    /* optional second copy with row stride ldkvp (all layers packed side by side
                                                             for ONE K-concatenated memory-gradient product), or NULL */
    float *part1, *part2, *part3;                         /* [(M+3)/4][2][256] */
    uint32_t seed_ad, seed_d1, seed_ad2, seed_d2, seed_d3, reserved;
} rt_decoder_layer_bwd;
typedef struct rt_decoder_bwd_desc {
    rt_decoder_layer_bwd layer[RT_DEC_MAX_LAYERS];
    float*          dta;       /* out [M,256]: gradient w.r.t. the stack's input (tgt) */
    float*          dqpos;     /* [M,256], accumulated (+=): gradient w.r.t. query_pos */
    const uint8_t*  kpm;
    uint32_t*       handoff;
    const uint32_t* seed_dev;
    int32_t n_layers, M, H, S, F, ldkv;
    float   drop_p, scale, gate_scale;                    /* gate_scale = 1 / (1 - p) of linear1's dropout */
    int32_t ldkvp;
} rt_decoder_bwd_desc;
int rt_decoder_bwd(const rt_decoder_bwd_desc* d, rt_stream_t stream);
/* REFTR_DEC_TRACE=1 only: 1024 wall-clock stamps (100 MHz) of the last launch's stage boundaries, host buffer */
int rt_decoder_trace(uint32_t* out1024);
/* rt_decoder_supported — RT_OK when rt_decoder_fwd / rt_decoder_bwd may be used on the CURRENT device: their G spin-waiting
 * workgroups must be co-resident, which is checked with the occupancy query (>= 1 workgroup of each kernel per compute unit at its
 * LDS size) and a 2x margin of compute units over G; RT_ERR_UNSUPPORTED otherwise (the launchers answer the same, and the caller
 * keeps the launched chain).  rt_decoder_set_spin — polls a consumer makes before it gives up and raises the failure word
 * (<= 0: the default, 2^20 / REFTR_DEC_SPIN); tests force a timeout with 1. */
int rt_decoder_supported(int F);
int rt_decoder_set_spin(int spin);


/* --------------------------------------------------------------------------------------------
 * The few-row region between the encoder's forward and backward as three launches (round 5, csrc/rt_qregion.hip).
 * Rows: N = B * P phrase rows (P <= 16 phrases per image), L <= 96 language tokens, E = 256.  Every workgroup works alone (no
 * grid hand-off); the tensors listed as outputs are exactly what the launched chain (rt_conv_gemm + rt_layernorm_* + rt_rows_add +
 * rt_qenc_attn_* + rt_box_loss + rt_small_dgrad) leaves behind, in the same formats, so forward / backward may mix fused and
 * launched halves and the weight gradients stay with rt_small_wgrad_grouped / rt_conv_wgrad_grouped.
 *
 * rt_qenc_fwd  -- QueryEncoder.forward (models/reftr_transformer.py:41-66) + the query / query_pos split (:60-66), one workgroup
 *                 per image.  cat16 [N, 2E]: columns E.. hold map_phrase's output on entry, columns ..E are written here.
 * rt_head_loss -- decoder.norm on every layer's output (models/modeling/transformer.py:131-141), bbox_embed (models/modeling/
 *                 backbone.py:26-38, models/reftr_transformer.py:287), CriterionVGMultiPhrase's box losses for all layers
 *                 (models/criterion.py:113-153) with d total / d logits for the per-layer weights `weights` [NL][2], and the
 *                 backward-data of the MLP and of the norm: one workgroup per decoder layer; losses [NL][2] are WRITTEN (no clear
 *                 needed, no atomics: run-to-run reproducible).  Nothing is accumulated: the launch may run before the gradient clear.
 * rt_qenc_bwd  -- backward-data of rt_qenc_fwd: from ga (+ gb) = d tgt and dqpos = d query_pos down to d memory (language rows and
 *                 the CLS row of every image are accumulated in place; nothing else writes them while the launch runs), d
 *                 query_embed (accumulated, n_q = 1), the bf16 dy operands of the six Linear weight gradients, and per-workgroup
 *                 LayerNorm parameter-gradient partials [B][2][E] for rt_ln_param_grad_grouped.
 * ------------------------------------------------------------------------------------------ */
typedef struct rt_qenc_fwd_desc {
    const void*  mem16;  const float* mem32;  const uint8_t* ctx;     /* memory bf16 / fp32 [B*S, E]; context mask [B, P, L] */
    const void *W1, *W2, *W3, *Wc, *Wf0, *Wf4;                          /* bf16 [E][E] (Wf0: [E][2E]) */
    const float *b1, *b2, *b3, *bc, *bf0, *bf4;
    const float *gc, *betc, *g1, *bet1, *g5, *bet5;                     /* context_out.1, fuse_encoder_query.1 / .5 */
    const float* qembed;                                                /* query_embed.weight [nq, 2E] */
    const uint32_t* seed_dev;
    void *cls16, *lang16;  float *kq, *qs, *vs, *qw;                    /* saved: bf16 [B,E], [B*L,E]; fp32 [B,E], [B*L,E] x 2, [B,P,L] */
    void* c16;  float *co, *cmean, *crstd;                              /* bf16 [N,E]; fp32 [N,E], [N], [N] */
    void* cat16;                                                        /* bf16 [N, 2E] */
    float *t1, *m1, *r1;  void* a16;  float *t2, *m2, *r2;
    float* tgt32;  void* tgt16;  float* qpos;  void* tgtq16;            /* [N*nq, E] */
    int32_t B, S, L, P, nq, E;
    float   eps, drop_p;
    uint32_t drop_seed;  int32_t reserved;
} rt_qenc_fwd_desc;
int rt_qenc_fwd(const rt_qenc_fwd_desc* d, rt_stream_t stream);

typedef struct rt_head_loss_desc {
    const float* t3;                                                    /* fp32 [NL*N, E]: every decoder layer's output */
    const float *gn, *betn;                                             /* decoder.norm */
    const void *W0, *W1, *W2, *W0T, *W1T;                               /* bf16 [E][E], [E][E], [4][E]; backward-data operands [E][E] */
    const float *b0, *b1, *b2, *w2_f32;                                 /* fp32 biases; fp32 master of the last Linear [4][E] */
    const uint8_t* valid;  const float* targets;  const int32_t* tgt_off;  const float* num_boxes;  const float* weights;   /* as rt_box_loss */
    void *hs16, *y1, *y2;  float *hmean, *hrstd;                        /* saved: bf16 [NL*N, E] x 3; fp32 [NL*N] x 2 */
    float *logits, *losses, *dlogits;  void* dl16;                      /* fp32 [NL*N, 4], [NL][2], [NL*N, 4]; bf16 [NL*N, 4] */
    void *dy2, *dy1;  float *dhs, *dnorm;                               /* bf16 [NL*N, E] x 2; fp32 [NL*N, E] x 2 */
    float* db2_part;                                                    /* optional: [NL][2][4], row 0 of a pair = the layer's share of d bias of the last Linear (rt_ln_param_grad_grouped adds the pairs up) */
    float* part_n;                                                      /* [NL][2][E] */
    float* total;  int32_t* ticket;                                     /* optional: weighted total [1], written by the workgroup that draws the last ticket; *ticket must be 0 at the first launch and is left 0 */
    int32_t NL, B, P, K, E;
    float   eps;
    int32_t invert_valid;  int32_t reserved;                            /* invert_valid: `valid` holds 1 = ignore (the model's query mask) */
} rt_head_loss_desc;
int rt_head_loss(const rt_head_loss_desc* d, rt_stream_t stream);

typedef struct rt_qenc_bwd_desc {
    const float *ga, *gb, *dqpos;                                       /* fp32 [N, E]; gb optional */
    const float *t2, *m2, *r2, *g5, *bet5;
    const float *t1, *m1, *r1, *g1, *bet1;
    const float *co, *cmean, *crstd, *gc, *betc;
    const float *kq, *qs, *vs, *qw;
    const void *Wf4T, *Wf0T, *WcT, *W1T, *W2T, *W3T;                    /* bf16 backward-data operands [K][N] */
    const uint32_t* seed_dev;
    void *dt2b, *dt1b, *dcob, *dk16, *dqs16, *dvs16;                    /* bf16 dy operands of the weight gradients */
    float *da, *dcat, *dc;                                              /* fp32 scratch / outputs: [N,E], [N,2E], [N,E] */
    float* dmem;                                                        /* fp32 [B*S, E], accumulated */
    float* dqembed;                                                     /* optional: fp32 [2, E], accumulated */
    float *part5, *part1, *partc;                                       /* [B][2][E] each */
    int32_t B, S, L, P, E;
    float   drop_p;
    uint32_t drop_seed;  int32_t reserved;
} rt_qenc_bwd_desc;
int rt_qenc_bwd(const rt_qenc_bwd_desc* d, rt_stream_t stream);
/* Measurement aid: the stage stamps (100 MHz wall clock) workgroup 0 of the last rt_qenc_fwd / rt_head_loss / rt_qenc_bwd launch left,
 * [3][24] values copied to HOST memory (synchronises with the device). */
int rt_qregion_trace(unsigned long long* host_out);

#ifdef __cplusplus
}
#endif
#endif /* REFTR_HIP_H */
