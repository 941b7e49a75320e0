/*
 * endodav_hip.h — C ABI of libendodav_hip.so: the MI355X (gfx950) implementation of
 * EndoDAV's per-clip forward.
 *
 * The reference has no FFI / plugin registry for this path: its boundary is the Python
 * class surface models/endodav/__init__.py:1-2.  This header is the
 * boundary the build's own host module (endodav_amd/endodav.py, a mirror of
 * models/endodav/endodav.py:53-160) binds through ctypes; INTEGRATION.md shows the stub a
 * maintainer of the reference would add.  Rules of the ABI:
 *
 *   - plain C types only: device pointers, sizes, an opaque context; no torch types;
 *   - every pointer named *_dev is a device pointer on the CURRENT HIP device;
 *   - every call is stream-ordered on `stream` (a hipStream_t passed as void*; NULL = the
 *     legacy default stream) and performs no host/device synchronisation, except
 *     edv_create/edv_destroy and the first edv_forward at a new clip geometry, which
 *     allocate the activation workspace (hipMalloc);
 *   - return value 0 = ok, non-zero = error, text in edv_last_error(); nothing throws;
 *   - one context per device and per host thread (nn.DataParallel replicas each own one);
 *     the library keeps no global mutable state besides the thread-local error string.
 *
 * Data layout: activations are fp32, tokens-major [frames*tokens, D] in the
 * encoder and channels-last [frames, h, w, C] in the DPT head; the clip comes in as the
 * reference's [B, T, 3, H, W] and the disparities go out as [B*T, 1, h_s, w_s].
 */
#ifndef ENDODAV_HIP_H
#define ENDODAV_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EDV_ABI_VERSION 15 /* 15: edv_split_plan (test entry point: the stream-K planners without a device); 14: evaluation on the device (edv_metrics_workspace, edv_masked_median, edv_metrics_pred, edv_metrics_errors, edv_metrics_temporal); 13: test entry points for row-mapped GEMM / LayerNorm descriptors and the folds (edv_gemm_desc ... edv_bilinear_add); 12: edv_stitch_fit, edv_stitch_apply; 11: edv_set_bias_grads, edv_colsum_batch; 9: edv_trainer_loss; 8: edv_debug_fill_lds (test hook); 7: the split-bf16 experiment entry points left the library */

enum edv_lora_type { EDV_LORA_NONE = 0, EDV_LORA_LORA = 1, EDV_LORA_DVLORA = 2, EDV_LORA_SSB = 3, EDV_LORA_DASH = 4 };

/* Mirrors the constructor of the reference model, models/endodav/endodav.py:53-73, after the
 * encoder name has been resolved to dimensions (vision_transformer.py:352-398). */
typedef struct edv_config {
    int32_t abi_version;        /* EDV_ABI_VERSION */
    int32_t embed_dim;          /* 384 / 768 / 1024 */
    int32_t depth;              /* 12 / 12 / 24 */
    int32_t num_heads;          /* 6 / 12 / 16 (head dim must be 64) */
    int32_t taps[4];            /* intermediate_layer_idx, endodav.py:76-79 */
    int32_t features;           /* DPT `features` */
    int32_t out_channels[4];    /* DPT `out_channels` */
    int32_t image_h, image_w;   /* `image_shape`; multiples of 14 (patch_embed.py:72-73) */
    int32_t num_frames;         /* temporal_max_len; T <= num_frames (motion_module.py:197) */
    int32_t pos_tokens;         /* rows of pretrained.pos_embed (1370, or 257 for vitl) */
    int32_t lora_type;          /* enum edv_lora_type */
    int32_t lora_rank;          /* r */
    int32_t include_cls_token;  /* vision_transformer.py:229-230 */
    int32_t conv_head;          /* 1 = four HeadDepth heads (default), 0 = disable_conv_head */
    int32_t inv_sigmoid;        /* dpt_pyramid.py:104 */
    int32_t out_sigmoid;        /* dpt_pyramid.py:97-101 */
    int32_t temporal_lora;      /* endodav.py:119-137 */
    int32_t dash_active;        /* DashLinear past warm-up: add U_top diag(idx) Vt_top */
    int32_t use_clstoken;       /* DPT readout projections, dpt_pyramid.py:54-57 */
    uint32_t residual_mask;     /* bit i set: encoder block i carries a ResBottleneckBlock (block.py:146-150);
                                 * the reference hard-wires its grid to 16x20 patches = image_shape (224, 280) */
    int32_t use_bn;             /* eval-mode BatchNorm2d in the ResidualConvUnits (util/blocks.py:60-62,80-86), folded into the convolutions */
    int32_t pe_rope;            /* pe="rope" (motion_module.py:221-225,252-255): rotary q/k instead of the additive sinusoid;
                                 * needs a bound "<attention block>.freqs_cis" table [num_frames, C/2, 2] (cos, sin) per attention block */
} edv_config;

typedef struct edv_ctx edv_ctx;

/* ---- life cycle ------------------------------------------------------------------------ */
int edv_abi_version(void);
const char *edv_last_error(void);
int edv_create(const edv_config *cfg, edv_ctx **out);
int edv_destroy(edv_ctx *ctx);

/* Bind one entry of the model's state_dict (same key names as the reference)
 * to device memory owned by the caller; zero-copy, the pointer must stay valid. */
int edv_bind_param(edv_ctx *ctx, const char *name, const float *data_dev, const int64_t *shape, int32_t ndim);

/* Re-derive the packed weights from the bound parameters: LoRA folded into fc1/fc2
 * (mylora/layers.py:148-157,384-393,423-430), conv kernels repacked to [Cout][kh][kw][Cin],
 * q/k/v concatenated, the position table resampled (vision_transformer.py:186-217).
 * Call after every change of the bound tensors' contents. */
int edv_prepare(edv_ctx *ctx, void *stream);

/* The cheap form of edv_prepare for the fine-tune loop (trainer_end_to_end_video.py:427-431: only the optimizer writes, and only
 * into trainable tensors): re-folds the linears that carry LoRA factors (mlp.fc1/fc2 of every block and, with temporal_lora, ff.net.2
 * of the motion modules), re-packs the trainable convolutions (conv_depth_* or scratch.output_conv*, residual_*) and, once a backward
 * has run, their transposed / flipped copies, and rebuilds the packings that embed a copy of a bias (resize_layers.0/1, the fused
 * GEGLU weights of the motion modules, with use_bn the BatchNorm-folded ResidualConvUnit convolutions).  Everything else keeps its packing.  Valid only when no bound pointer changed and
 * only those tensors' contents did; otherwise call edv_prepare. */
int edv_refresh_lora(edv_ctx *ctx, void *stream);

/* endodav.forward (endodav.py:150-160).  x_dev: [B,T,3,H,W] fp32 in [0,1].  disp_dev[s] receives
 * ("disp", s): VDA head [B*T,1,ih,iw], [..ih/2..], ...; conv head [B*T,1,2*ph*8*.. see
 * edv_output_shape.  Requires T <= num_frames (motion_module.py:197) and T <= 32: the temporal-attention kernels are built for the
 * reference's window length (INFER_LEN = num_frames default = 32, endodav.py:47,62); a longer clip is refused before any work is
 * enqueued.  On an error the internal streams are drained before the call returns. */
int edv_forward(edv_ctx *ctx, const float *x_dev, int32_t B, int32_t T, int32_t H, int32_t W,
                float *const disp_dev[4], void *stream);
/* h/w of ("disp", s) for this configuration. */
int edv_output_shape(const edv_ctx *ctx, int32_t scale, int32_t *h, int32_t *w);
/* Debug taps: copy of an internal stage of the last edv_forward, for the per-stage parity
 * tests.  name in {"tokens","block0","tap0".."tap3","mm0","mm1","path4".."path1"}; head
 * stages are channels-last [frames,h,w,C].  Returns element count through *n (dst may be NULL). */
int edv_stage_copy(edv_ctx *ctx, const char *name, float *dst_dev, size_t *n, void *stream);
/* Debug: when on, edv_forward also snapshots the in-place residual stream ("tokens", "block0"). */
int edv_set_capture(edv_ctx *ctx, int on);
/* Live per-kernel timing for bench.py's roofline: bracket every launch of the selected kernel classes with a
 * HIP event pair on the launch stream.  Classes: 0 dense GEMM (Linear / 1x1 conv), 1 3x3 conv, 2 spatial
 * attention, 3 temporal attention, 4 LayerNorm, 5 other, 6 (read only; recorded with 0) the dense GEMMs of the encoder blocks,
 * 7 GroupNorm (statistics + apply), 8 bilinear resample, 9 GEGLU, 10 the final 1x1 convolution to one channel, 11 resize +
 * normalise + im2col of the input frames.  edv_profile_read waits for the recorded events, returns the number of launches and
 * their summed duration, and clears that class. */
int edv_profile_enable(edv_ctx *ctx, uint32_t class_mask);
/* Frames are independent in the encoder.  n = 0 (default): automatic -- two frame groups on internal streams while a block's
 * GEMMs are short (tokens x width <= 17 M: ViT-S up to T = 32, ViT-B up to T = 16), one otherwise; n = 1..4: that many.  With more than one group the attention of one
 * group runs beside the GEMMs of another, so per-kernel event brackets then measure time-shared launches: set 1 for the
 * steps whose kernels are being timed (bench.py does).  Environment EDV_ENC_STREAMS sets the initial value; n = -1 restores it. */
int edv_set_encoder_streams(edv_ctx *ctx, int32_t n);
/* Arithmetic of the encoder's linears (qkv, proj, fc1, fc2) in inference.  Inputs, outputs and accumulation are fp32 either way.
 *   EDV_PRODUCTS_F32     v_mfma_f32_32x32x2_f32: fp32 products on the fp32 matrix pipe (157 TFLOP/s peak)
 *   EDV_PRODUCTS_BF16X6  each operand split into three bf16 terms, six bf16 MFMAs per 16 k (gemm_x6.hip): per-term error below fp32's unit
 *                        roundoff (the three dropped cross terms are <= 2^-26 of a product), 192 instead of 512 matrix-pipe cycles.
 * The initial value comes from the environment variable EDV_PRODUCTS ("f32" | "bf16x6"), else F32.  Training forwards always use F32.
 * After edv_prepare the call builds the weights' bf16 planes on `stream` (+ 1.5 x the encoder linears' bytes). */
enum { EDV_PRODUCTS_F32 = 0, EDV_PRODUCTS_BF16X6 = 1 };
int edv_set_products(edv_ctx *ctx, int32_t products, void *stream);
int edv_get_products(const edv_ctx *ctx);
int edv_profile_set_mask(edv_ctx *ctx, uint32_t class_mask); /* change the bracketed classes, keep what was recorded */
int edv_profile_read(edv_ctx *ctx, int32_t kernel_class, int32_t *launches, double *total_ms);
/* Algorithmic work of the launches bracketed since edv_profile_enable / the last call: classes 0, 1, 6 book 2 M N K FLOP and every
 * operand once in bytes (4 (M K + N K + M N (+ M N per residual))); the bandwidth-bound classes 4, 7 .. 11 book bytes only (input
 * tensor(s) + output tensor, once each); 0 for classes that do not account. */
int edv_profile_work(edv_ctx *ctx, int32_t kernel_class, double *flops, double *bytes);
/* Bytes of device memory the context currently holds (packed weights + workspace). */
size_t edv_device_bytes(const edv_ctx *ctx);
/* Seconds spent in the dominant kernels are measured by the caller with HIP events; this
 * returns the number of kernel launches one edv_forward issued last time. */
int edv_last_launch_count(const edv_ctx *ctx);

/* ---- per-kernel entry points (unit tests, micro-benchmarks) --------------------------------
 * All tensors fp32, row-major, device pointers. */

/* y[m,:] = LN(x[m,:]) * w + b (+ pe[(m / rows_per_frame) % T, :] when pe_dev != NULL).
 * vision_transformer.py:97 (eps 1e-6), motion_module.py:155,161 (eps 1e-5) + :197. */
int edv_layernorm(const float *x_dev, const float *w_dev, const float *b_dev, float *y_dev, int64_t rows, int32_t dim,
                  float eps, const float *pe_dev, int32_t rows_per_frame, int32_t T, void *stream);

/* C[M,N] = epilogue(A[M,K] · W[N,K]ᵀ):  v = acc + bias[n]; v = act(v); v *= gamma[n]; v += R[m,n].
 * act: 0 none, 1 exact-erf GELU, 2 ReLU.  bias/gamma/R may be NULL.  K % 4 == 0.
 * F.linear / 1x1 conv with the epilogues of block.py:144-145, mlp.py:34-37. */
int edv_gemm(const float *A_dev, const float *W_dev, float *C_dev, int64_t M, int32_t N, int32_t K, const float *bias_dev,
             int32_t act, const float *gamma_dev, const float *R_dev, float *workspace_dev, size_t workspace_bytes, void *stream);
/* Stream-K workspace for edv_gemm, in BYTES (one size fits every shape on this device; one workspace per concurrently running
 * GEMM).  With a workspace the GEMM runs as persistent workgroups that split the last partial round of output tiles along K;
 * the last piece of a tile to arrive merges the pieces in a fixed order and applies the epilogue (no second launch; same
 * results up to fp32 summation order, reproducible run to run).  The workspace must be ZERO-FILLED once before its first use
 * (it starts with per-tile arrival counters, which every launch leaves at zero).  workspace_dev = NULL: one workgroup per tile. */
size_t edv_gemm_workspace(void);
/* The same GEMM with its products on the bf16 matrix pipe (EDV_PRODUCTS_BF16X6): split the weight once into planes_dev
 * (edv_gemm_x6_planes_bytes(N, K) bytes), then call edv_gemm_x6 with the planes in place of W.  K % 16 == 0, N >= 64.
 * Input domain (A and W alike; csrc/gemm_x6.hip has the measurements): the accuracy claim -- error no worse than edv_gemm's on the same
 * operands -- holds for finite values with 2^-100 <= |x| <= 2^100, or exactly 0; scaling an operand by a power of two inside that range scales
 * the result bit for bit.  Below it the result degrades gracefully (the lower bf16 terms go subnormal: equal to edv_gemm down to |x| ~ 2^-110,
 * 8 x its rms error at 2^-116, 120 x at 2^-120; always finite and within 2^-8 of sum |a w|).  A non-finite value, or a finite |x| >= 3.3962e38
 * (it rounds to a bf16 Inf), yields NaN where edv_gemm yields +-Inf / NaN: edv_gemm_x6_split writes Inf / NaN planes for such a weight row and
 * edv_gemm_x6 splits A the same way.  That NaN is confined: an entry of A row m reaches output row m only, one of W row n output column n
 * only; every other output element keeps the bits it has without it. */
size_t edv_gemm_x6_planes_bytes(int32_t N, int32_t K);
int edv_gemm_x6_split(const float *W_dev, void *planes_dev, int32_t N, int32_t K, void *stream);
int edv_gemm_x6(const float *A_dev, const void *planes_dev, float *C_dev, int64_t M, int32_t N, int32_t K, const float *bias_dev, int32_t act,
                const float *gamma_dev, const float *R_dev, float *workspace_dev, size_t workspace_bytes, void *stream);

/* GEGLU feed-forward input projection of the motion modules (motion_module.py: GEGLU.forward = x, gate = proj(h).chunk(2, -1); x * gelu(gate)),
 * fused: C[M, N/2] = (A W_v^T + b_v) * gelu(A W_g^T + b_g) in ONE launch -- the [M, N] projection is never written.  edv_pack_geglu interleaves the
 * Linear's [N, K] weight and [N] bias in 32-row blocks (value rows 32b.., then their gate rows N/2 + 32b..) so that a 64-column tile holds values
 * and gates of the same 32 outputs; edv_gemm_geglu takes the packed pair.  N = both halves (8 C), N % 64 == 0, K % 32 == 0. */
int edv_pack_geglu(const float *w_dev, const float *b_dev, float *wi_dev, float *bi_dev, int32_t N, int32_t K, void *stream);
int edv_gemm_geglu(const float *A_dev, const float *Wi_dev, const float *bi_dev, float *C_dev, int64_t M, int32_t N, int32_t K, void *stream);

/* 3x3 convolution, padding 1, stride 1 or 2, channels-last: x [F,H,W,Cin], w packed
 * [Cout][3][3][Cin], y [F,OH,OW,Cout]; optional ReLU on the input (util/blocks.py:79-85),
 * bias, ReLU on the output and up to two residual tensors shaped like y. */
int edv_conv3x3(const float *x_dev, const float *wpacked_dev, const float *bias_dev, float *y_dev, int32_t F, int32_t H, int32_t W,
                int32_t Cin, int32_t Cout, int32_t stride, int32_t pre_relu, int32_t post_relu, const float *R1_dev,
                const float *R2_dev, void *stream);
/* The same with a stream-K workspace (edv_gemm_workspace() bytes, zero-filled once, as for edv_gemm): grids that do not fill the part
 * (e.g. 384 -> 64 channels at 19x19: 46 tiles of 108 k-tiles) are split along K over the resident workgroups and merged in-kernel. */
int edv_conv3x3_ws(const float *x_dev, const float *wpacked_dev, const float *bias_dev, float *y_dev, int32_t F, int32_t H, int32_t W,
                   int32_t Cin, int32_t Cout, int32_t stride, int32_t pre_relu, int32_t post_relu, const float *R1_dev,
                   const float *R2_dev, float *workspace_dev, size_t workspace_bytes, void *stream);
/* Additive entry points (the ABI version stays as it is: the rule stated at edv_ingest_u8).
 * edv_conv3x3_dot: edv_conv3x3 followed by a 1x1 convolution to ONE channel and its activation, in one launch:
 *   y[f,oy,ox] = act2(sum_c w2[c] * act(conv(x)[f,oy,ox,c] + bias[c]) + b2[0]),   y [F,OH,OW]
 * -- the Cout-wide tensor is never written.  Cout <= 32, Cin % 32 == 0, no residuals; b2_dev may be NULL; act2: 0 none, 2 ReLU, 3 sigmoid(z),
 * 4 sigmoid(-z) (the modes of edv_dot_channels).  The sum over c is taken in a fixed order that differs from edv_dot_channels': the two agree to
 * within the rounding of a 32-term fp32 sum, not bit for bit.  A shape outside these limits, or a process in which the fused epilogue is switched
 * off (below), is an error: the caller runs edv_conv3x3 + edv_dot_channels instead.
 * edv_set_conv_impl: process-wide choice for the 3x3 convolutions and the engine's output heads.  0 = automatic (the default): the halo-tiled
 * kernel (conv_halo.hip: stride 1, Cin 32 or 64, Cout <= 32; bit-identical to the im2col kernel) for the shape classes where it measured
 * faster, the fused epilogue wherever it is supported; 1 = neither: every convolution runs the im2col kernel and stores its tile, the heads
 * run edv_dot_channels' kernel behind it; 2 = both wherever supported, whatever the table says (tests, A/B runs).  The environment variables
 * EDV_CONV_HALO=0 and EDV_CONV_DOT=0 switch either off for a whole process.  A training forward never fuses: the backward reads the
 * 32-channel tensor. */
int edv_set_conv_impl(int32_t mode);
int edv_conv3x3_dot(const float *x_dev, const float *wpacked_dev, const float *bias_dev, float *y_dev, int32_t F, int32_t H, int32_t W,
                    int32_t Cin, int32_t Cout, int32_t stride, int32_t pre_relu, int32_t post_relu, const float *w2_dev,
                    const float *b2_dev, int32_t act2, void *stream);
/* Repack a torch Conv2d weight [Cout,Cin,3,3] to [Cout][3][3][Cin]. */
int edv_pack_conv3x3(const float *w_dev, float *wpacked_dev, int32_t Cout, int32_t Cin, void *stream);

/* Encoder self-attention, layers/attention.py:56-69: qkv [F*N, 3*heads*64] as produced by the
 * qkv linear (columns ordered [3][heads][64]) -> out [F*N, heads*64].  The kernel runs as persistent workgroups
 * that split the last, partial round of (frame, head, query-block) tasks along the key axis; the pieces meet in a
 * device workspace of edv_attn_spatial_workspace(F, N, heads) BYTES (0 when nothing is split; 16-byte aligned,
 * owned by the caller, one per concurrently running call). */
size_t edv_attn_spatial_workspace(int32_t F, int32_t N, int32_t heads);
int edv_attn_spatial(const float *qkv_dev, float *out_dev, int32_t F, int32_t N, int32_t heads, float *workspace_dev,
                     size_t workspace_bytes, float *lse_dev, void *stream);
/* lse_dev (optional, [F, heads, N]): per-row log-sum-exp of the scaled scores in base 2, the only extra state the
 * backward needs.  edv_attn_spatial_bwd: dqkv [F*N, 3*heads*64] (like qkv) from qkv, out, dout [F*N, heads*64] and lse;
 * delta_dev is [F, heads, N] floats of scratch.
 * Accuracy: the probabilities are recomputed as 2^(S log2e - lse) from the fp32 lse, delta = dout . out comes from the forward's output.  Each
 * probability so carries a relative error of about sqrt(32) ulp(lse) ln2 / sqrt(12) the forward's did not have, and a row of dS sums to zero only
 * to that accuracy: per output column dq, dk, dv are within 4x of torch's fp32 autograd for |lse| up to about 16; with scores in the tens the
 * largest dq error is about 10x torch's; a component kbar common to all keys enters dq as kbar sum_j dS_ij (1e-3 of dq at a score offset of 500
 * with |kbar| = 62 |k - kbar|).  dk, dv and lse stay within 2x of torch.  Finite inputs; dout scaled by a power of two scales dqkv bit for bit;
 * a NaN in a dout or k row of (frame f, head h) stays in the (f, h) block of dq, dk and dv. */
/* The same attention with both products on the bf16 matrix pipe (EDV_PRODUCTS_BF16X6: three-term bf16 splits of q, k, v and of the probabilities,
 * six bf16 MFMAs per 16 k, fp32 accumulate and fp32 softmax; sequences longer than 128, shorter ones run the fp32 kernel).  Its own workspace size.
 * Input domain as for edv_gemm_x6: finite q, k, v with 2^-100 <= |x| <= 2^100 or exactly 0 (v scaled by a power of two scales the output bit for
 * bit; q scaled by 2^s and k by 2^-s leave it unchanged bit for bit).  A non-finite entry, or a finite |x| >= 3.3962e38, yields NaN where
 * edv_attn_spatial may yield +-Inf, and stays confined as there: one in a q row of head h makes that output row of head h non-finite and nothing
 * else; one in a k or v row of (frame f, head h) may make the output of that (f, h) block non-finite and leaves every other (frame, head) block
 * bit for bit as it is without it. */
size_t edv_attn_spatial_x6_workspace(int32_t F, int32_t N, int32_t heads);
int edv_attn_spatial_x6(const float *qkv_dev, float *out_dev, int32_t F, int32_t N, int32_t heads, float *workspace_dev, size_t workspace_bytes,
                        void *stream);
size_t edv_attn_spatial_bwd_workspace(int32_t F, int32_t N, int32_t heads); /* bytes; the backward splits its last partial round too */
int edv_attn_spatial_bwd(const float *qkv_dev, const float *out_dev, const float *dout_dev, const float *lse_dev, float *delta_dev,
                         float *dqkv_dev, int32_t F, int32_t N, int32_t heads, float *workspace_dev, size_t workspace_bytes, void *stream);

/* Temporal attention core, motion_module.py:230-297 + attention.py:182-211: qkv [B*T*P, 3C]
 * (q|k|v per row, 8 heads), softmax over the T frames of each pixel -> out [B*T*P, C]. */
int edv_attn_temporal(const float *qkv_dev, float *out_dev, int32_t B, int32_t T, int32_t P, int32_t C, int32_t heads, void *stream);

/* Rotary embedding of the temporal attention, attention.py:419-429: q|k of qkv [B*T*P, 3C] rotated in place, channel pairs
 * (2i, 2i+1) of a row of frame t by the angle whose (cos, sin) is table[t, i, :] (table [>=T, C/2, 2], attention.py:402-408).
 * transpose != 0 applies the adjoint (the gradient of the rotation with respect to its input). */
int edv_rope_qk(float *qkv_dev, const float *table_dev, int32_t B, int32_t T, int32_t P, int32_t C, int32_t transpose, void *stream);

/* GroupNorm(32 groups) on channels-last x [F,P,C] (motion_module.py:84,110).  With a workspace (edv_groupnorm_workspace bytes) the
 * statistics are taken in two coalesced stages (per 32-pixel chunk and channel, then merged per group with the parallel-variance
 * formula); with workspace_dev = NULL one workgroup per (frame, group) reads its strided slab twice.  Same values to fp32 rounding.
 * Both paths take the variance in the corrected two-pass form (sum d^2 - (sum d)^2 / n about the fp32 mean, which is then corrected by sum d / n),
 * so stats_dev = [F, groups, 2] (mean, rstd), which edv_groupnorm_bwd consumes, holds to fp32 rounding however far the mean is above the spread;
 * a slab of one value v (at most 12 significant bits, chunks of a power-of-two number of rows) gives mean = v, rstd = rsqrt(eps), y = b exactly. */
size_t edv_groupnorm_workspace(int32_t F, int32_t P, int32_t C);
int edv_groupnorm(const float *x_dev, const float *w_dev, const float *b_dev, float *y_dev, float *stats_dev /* [F*32*2] scratch */,
                  int32_t F, int32_t P, int32_t C, int32_t groups, float eps, float *workspace_dev, size_t workspace_bytes, void *stream);

/* GEGLU, attention.py:363-384: y[m, j] = x[m, j] * gelu(x[m, inner + j]), x [M, 2*inner]. */
int edv_geglu(const float *x_dev, float *y_dev, int64_t M, int32_t inner, void *stream);

/* Bilinear resize, align_corners=True, channels-last [F,H,W,C] -> [F,OH,OW,C]
 * (every F.interpolate of the model). */
/* Test hook: fills the whole LDS (160 KB) of every CU with `value`; LDS keeps its contents between kernels, so a kernel that depends on LDS bytes it
 * never wrote shows.  No reference counterpart. */
int edv_debug_fill_lds(float value, void *stream);

int edv_bilinear(const float *x_dev, float *y_dev, int32_t F, int32_t H, int32_t W, int32_t C, int32_t OH, int32_t OW, void *stream);

/* y[m] = act(x[m,:]·w + b) for the final 1x1 convs; act: 0 none, 2 ReLU, 3 sigmoid, 4 sigmoid(-v). */
int edv_dot_channels(const float *x_dev, const float *w_dev, const float *b_dev, float *y_dev, int64_t M, int32_t C, int32_t act, void *stream);

/* endodav.py:153-155 + patch_embed.py:75-77 staging: bilinear resize (align_corners) of
 * x [F,3,H,W] to [ih,iw], ImageNet normalisation, and im2col into rows
 * [F*(ih/14)*(iw/14), 588] ordered (c, ky, kx) like the Conv2d weight. */
int edv_patchify(const float *x_dev, float *cols_dev, int32_t F, int32_t H, int32_t W, int32_t ih, int32_t iw, void *stream);

/* ConvTranspose2d with kernel == stride == s (dpt.py:71-82), channels-last x [F,h,w,C] -> y [F,h*s,w*s,C];
 * w [C,C,s,s] and b [C] in torch layout; wpack [s*s*C*C] and bpack [s*s*C] are caller scratch. */
int edv_conv_transpose(const float *x_dev, const float *w_dev, const float *b_dev, float *wpack_dev, float *bpack_dev, float *y_dev, int32_t F, int32_t h,
              int32_t w, int32_t C, int32_t s, void *stream);

/* interpolate_pos_encoding's bicubic resample (vision_transformer.py:186-217): grid [S,S,D] -> out [oh,ow,D]
 * with scale factors (oh+0.1)/S, (ow+0.1)/S exactly as F.interpolate(scale_factor=...) receives them. */
int edv_bicubic_pos(const float *grid_dev, float *out_dev, int32_t S, int32_t D, int32_t oh, int32_t ow, double scale_h, double scale_w, void *stream);

/* Bicubic resize of `planes` images [H,W] -> [OH,OW] (Keys cubic a=-0.75, half-pixel centres, clamped
 * borders = cv2.INTER_CUBIC): the frame pre-resize of infer_video_depth (endodav.py:170-181,196). */
int edv_resize_bicubic(const float *x_dev, float *y_dev, int32_t planes, int32_t H, int32_t W, int32_t OH, int32_t OW, void *stream);

/* Frame ingest of streamed video (stream_video_depth): out[i] = frame slots[i] of src, uint8 HWC -> [0,1] fp32 planar
 * CHW, bicubically resized to OH x OW when (OH, OW) != (H, W).  src_dev [src_frames, H, W, 3] uint8; slots_host: n indices into src (host
 * memory, copied by value into the launch: no upload, no device allocation; NULL = 0..n-1); out_dev [n, 3, OH, OW] fp32.  1 <= n <= 64.
 * Bit for bit what the two-step path gives (uint8 -> float32 -> div_(255.0) by torch on the device, which multiplies by the fp32
 * reciprocal of 255, made contiguous planar, then edv_resize_bicubic).  Never reads outside [src_dev, src_dev + src_frames*H*W*3).  Null pointers, n outside
 * 1..64, a slot outside [0, src_frames) and sizes beyond edv_resize_bicubic's bound return non-zero and launch nothing.
 * Added without a version bump: an additive entry point leaves edv_config and every existing signature as they are, so EDV_ABI_VERSION
 * changes only when one of those does. */
int edv_ingest_u8(const uint8_t *src_dev, int32_t src_frames, const int32_t *slots_host, int32_t n, float *out_dev, int32_t H, int32_t W, int32_t OH,
                  int32_t OW, void *stream);

/* ---- colour-mapped depth on the device (render.colorize, infer_video_depth(render=...), stream_video_depth(render=...); the numpy of
 * utils/eval_utils.py:284-295 save_video, evaluate_depth_video.py:32-36 render_depth and test_simple.py:156-167) ----
 * Additive entry points: the ABI version stays as it is (the rule stated at edv_ingest_u8).  A clip is x_dev [n, h, w] fp32, h*w < 2^31.
 * Every operation is fp32, not contracted, in the order written here: the results are numpy's bits.  Inputs are finite: NaN is unsupported.
 * edv_render_range writes range_dev [n][2] = (lo, hi) per frame.
 *   mode 0 "frame":    the frame's minimum and maximum.
 *   mode 1 "video":    the minimum and maximum of all n*h*w elements (a 64-bit count), written to every one of the n rows.
 *   mode 2 "quantile": per frame the order statistics of rank rank_lo and rank_hi (0 <= rank_lo <= rank_hi < h*w, the same for every frame):
 *                      np.sort(frame.ravel())[rank].  Exact radix select on the order-preserving integer image of the float bits, four 8-bit
 *                      histogram passes, both statistics followed at once (one histogram until their prefixes part), LDS counters flushed
 *                      with 64-bit integer atomics.  Batched: one launch per pass for all frames of a chunk (the frame on blockIdx.y, a
 *                      select state per frame in the workspace): eight launches for up to 64 frames, whatever their number.
 *   All three compare those integer keys, so -0.0 orders below +0.0 (numpy leaves the choice between them open; no colour depends on it).
 *   rank_lo and rank_hi are ignored by modes 0 and 1.  Integer atomics only: the same input gives the same bits on every call.
 * edv_render_workspace(n): bytes edv_render_range needs for n frames, 16-byte aligned memory; frames go in chunks of 64, so it stops growing there.
 * edv_render_colorize: out[f, y, x, :] = lut[idx] with, per pixel of frame f and (lo, hi) = range_dev[f * range_stride + {0, 1}]
 *   (range_stride 2: a pair per frame; 0: one pair for all frames),
 *     den = (hi - lo) + eps;  t = (x - lo) / den  (IEEE division);  if clip: t = min(max(t, 0), 1);
 *     idx = den == 0 ? 0 : (uint8) trunc(t * 255.0f), clamped to 0..255.
 *   lut_dev [256][3] uint8; out_dev [n, h, w, 3] uint8 in the table's channel order.  With beside_dev [n, h, w, 3] uint8 (may be NULL)
 *   out_dev is [n, h, 2w, 3]: each row the row of beside_dev followed by the colour row (save_video's np.concatenate(..., axis=1)).
 *   When w % 4 == 0, x_dev is 16-byte and out_dev / beside_dev are 4-byte aligned, a thread reads four pixels in one 16-byte load and writes
 *   their 12 bytes as three whole dwords; one byte per store otherwise.  Never writes outside out_dev's n*h*w*3 (or n*h*2w*3) bytes.
 * Null pointers, n < 1, h or w < 1, h*w >= 2^31, an unknown mode or stride, rank_lo > rank_hi, a rank >= h*w, a workspace that is missing,
 * short or not 16-byte aligned return non-zero and launch nothing. */
size_t edv_render_workspace(int64_t n);
int edv_render_range(const float *x_dev, int64_t n, int32_t h, int32_t w, int32_t mode, int64_t rank_lo, int64_t rank_hi, float *range_dev,
                     void *workspace_dev, size_t workspace_bytes, void *stream);
int edv_render_colorize(const float *x_dev, int64_t n, int32_t h, int32_t w, const float *range_dev, int32_t range_stride, float eps, int32_t clip,
                        const uint8_t *lut_dev, const uint8_t *beside_dev, uint8_t *out_dev, void *stream);

/* ---- point clouds on the device (cloud.lift, model.video_point_cloud; the float64 numpy of get_point_cloud in the loaders
 * of tools/viser-rgbd/utils and of visualize_reconstruction.py) ----
 * Additive entry points: the ABI version stays as it is (the rule stated at edv_ingest_u8).  A clip of depth becomes world-space points with
 * the frames' colours, masked, subsampled and compacted in order: frame-major, then row-major over the kept output pixels of a frame.
 * edv_cloud_selection says which pixels are kept and at what depth; both calls take the same one.
 *   x_dev [n, h, w] fp32, 1 <= n <= 65535, h*w < 2^31; mask_dev uint8 or NULL, [h, w] (mask_stride 0) or [n, h, w] (mask_stride h*w), non-zero = keep.
 *   Output grid oh = ceil(h/step), ow = ceil(w/step).  Output pixel (oy, ox) samples source pixel sy = min(oy*step + step/2, h-1),
 *   sx = min(ox*step + step/2, w-1) (integer division): the pixel that holds the grid position ((ox+0.5)*step, (oy+0.5)*step).  Depth, mask
 *   and colour all come from that pixel.
 *   Depth in fp32, every operation rounded separately, IEEE division:
 *     mode 0 "depth":      z = x * gain
 *     mode 1 "disparity":  scaled = lo + span * x;  z = 1.0f / scaled;  z = z * gain      (disp_to_depth, then a scale)
 *   kept = (mask_dev == NULL || mask != 0) && z > near_z && z < far_z.  NaN fails both comparisons and +Inf fails z < far_z even for
 *   far_z = +Inf, so every point is finite whenever the cameras are.
 * cams_dev: 21 doubles per camera, Kinv[3][3], R[3][3], t[3], the matrices row-major; cam_stride 0: one camera for all frames, 21: one per frame.
 *   Geometry in fp64, every multiply and add rounded separately, in this order:
 *     u = (ox + 0.5) * step;  v = (oy + 0.5) * step
 *     l_i = (Kinv[i][0]*u + Kinv[i][1]*v) + Kinv[i][2]
 *     r_i = (R[i][0]*l_0 + R[i][1]*l_1) + R[i][2]*l_2
 *     p_i = (float)(t_i + r_i * (double)z)
 * edv_cloud_tile_pixels(): the output pixels one workgroup handles.  edv_cloud_workspace: 8 bytes per tile, n * ceil(oh*ow / tile) tiles, 8-byte
 *   aligned device memory; 0 for a shape the calls refuse.  It grows with n, so a whole video is one call.
 * edv_cloud_count (two launches): per-tile counts by wave ballot and popcount, the frame on blockIdx.y; then one workgroup scans them, 64-bit
 *   and exclusive, over all tiles in frame-major order, in place in the workspace, and fills offsets_dev [n+1] int64: offsets[f] = the points of
 *   the frames before f, offsets[n] = the total.  Reads 4 bytes (5 with a mask) per sampled pixel and nothing else.
 * edv_cloud_scatter (one launch; the workspace and offsets_dev as edv_cloud_count left them for the same selection): recomputes the predicate,
 *   ranks every kept pixel inside its tile, and writes point g = tile offset + rank only when g < capacity: points_dev [capacity][3] fp32 and,
 *   when frames_dev [n, h, w, 3] uint8 and colors_dev are both non-NULL, colors_dev [capacity][3] uint8.  Every store is one float or one byte
 *   of one point: never a byte outside capacity*12 or capacity*3, and never two workgroups in one dword.  capacity 0 launches nothing.
 * No atomics and no waiting between workgroups: the same input gives the same bits on every call.
 * Null required pointers, n outside 1..65535, h, w or step < 1, h*w >= 2^31, an unknown mode, cam_stride or mask_stride, a workspace that is
 * missing, short or not 8-byte aligned, and capacity < 0 return non-zero and launch nothing. */
typedef struct edv_cloud_selection {
    const float *x_dev;
    int64_t n;
    int32_t h, w, step, mode;
    float lo, span, gain, near_z, far_z;
    const uint8_t *mask_dev;
    int64_t mask_stride;
} edv_cloud_selection;
int32_t edv_cloud_tile_pixels(void);
size_t edv_cloud_workspace(int64_t n, int32_t h, int32_t w, int32_t step);
int edv_cloud_count(const edv_cloud_selection *sel, int64_t *offsets_dev, void *workspace_dev, size_t workspace_bytes, void *stream);
int edv_cloud_scatter(const edv_cloud_selection *sel, const double *cams_dev, int32_t cam_stride, const uint8_t *frames_dev, const int64_t *offsets_dev,
                      const void *workspace_dev, size_t workspace_bytes, float *points_dev, uint8_t *colors_dev, int64_t capacity, void *stream);

/* ---- surface fusion on the device (fusion.Tsdf, model.video_surface; not in the reference, whose 3d_reconstruction clouds concatenate the frames) ----
 * Additive entry points: the ABI version stays as it is (the rule stated at edv_ingest_u8).  A clip of depth with its cameras is folded into one
 * truncated signed distance (TSDF) volume, and the zero crossings of the volume come out as an ordered, compacted point list.
 * edv_tsdf_volume: nx * ny * nz voxels, x fastest, nx*ny*nz < 2^31.  tsdf_dev and weight_dev [nz, ny, nx] fp32, color_dev [nz, ny, nx, 3] fp32 or
 *   NULL.  A fresh volume is tsdf = 1, weight = 0, color = 0.  Voxel (i_x, i_y, i_z) has its centre at c_a = origin[a] + (i_a + 0.5) * voxel, fp64.
 * edv_tsdf_integrate (one launch for the whole clip): one thread owns one voxel, loads it once, takes the n frames of the selection in order with
 *   the voxel in registers, and stores it once, only if some frame updated it.  The selection is the cloud's, with step == 1; frames_dev
 *   [n, h, w, 3] uint8 goes with a coloured volume and NULL with an uncoloured one.
 *   cams_dev: 18 doubles per camera, W[3][4] = rows 0..2 of inv(T_world_camera), row-major, then K00 K01 K02 K10 K11 K12 (the last row of K is
 *   0 0 1); cam_stride 0: one camera for all frames, 18: one per frame.  Per frame, every multiply, add and divide rounded on its own:
 *     fp64  q_i = ((W[i][0]*c_x + W[i][1]*c_y) + W[i][2]*c_z) + W[i][3];   skip the frame unless q_2 > 0 (which also skips NaN)
 *     fp64  u = ((K00*q_0 + K01*q_1) + K02*q_2) / q_2;  v = ((K10*q_0 + K11*q_1) + K12*q_2) / q_2       (pixel centres at (x + 0.5, y + 0.5))
 *           skip unless u >= 0 && u < w && v >= 0 && v < h, tested in fp64 before any conversion;  px = (int)u, py = (int)v
 *     fp32  z and kept of pixel (py, px) exactly as in the selection above (depth or disparity rule, gain, mask, near_z < z < far_z,
 *           non-finite dropped);  skip the frame if the pixel is not kept
 *     fp64  sdf = (double)z - q_2;  skip if sdf < -trunc;  r = sdf / trunc;  d = (float)(r < 1 ? r : 1)
 *     fp32  wn = weight + 1;  tsdf = (tsdf * weight + d) / wn;  per channel color = (color * weight + (float)rgb) / wn;
 *           weight = wn < max_weight ? wn : max_weight
 * Extraction has the cloud's three steps.  Voxel a runs in linear order, axis k runs x, y, z, b = a + e_k is the neighbour along that axis and
 *   must lie inside the grid.  The pair emits a point when weight_a >= min_weight && weight_b >= min_weight && (tsdf_a < 0) != (tsdf_b < 0);
 *   0 and -0 count as non-negative.  Points are ordered voxel-major, axis-minor.
 *     fp32  t = tsdf_a / (tsdf_a - tsdf_b)                        (the signs differ, so the divisor is never zero)
 *     fp64  p_k = origin[k] + ((i_k + 0.5) + (double)t) * voxel;  the other two coordinates are the voxel centre's;  stored as float
 *     fp32  per channel c = c_a + t * (c_b - c_a);  colour = (uint8) min(255, max(0, floor(c + 0.5)))
 * edv_tsdf_tile_voxels(): the voxels one workgroup of the extraction handles.  edv_tsdf_workspace: 8 bytes per tile, ceil(nx*ny*nz / tile) tiles,
 *   8-byte aligned device memory; 0 for a shape the calls refuse.
 * edv_tsdf_count (two launches): per-tile counts by wave ballot and popcount, then one workgroup scans them, 64-bit and exclusive, in place in
 *   the workspace, and writes the number of points to total_dev[0].
 * edv_tsdf_extract (one launch; the workspace as edv_tsdf_count left it for the same volume and min_weight): recomputes the predicates, ranks
 *   every crossing inside its tile and writes point g = tile offset + rank only when g < capacity: points_dev [capacity][3] fp32 and, when
 *   colors_dev is not NULL (the volume must then be coloured), colors_dev [capacity][3] uint8.  Every store is one float or one byte of one
 *   point: never a byte outside capacity*12 or capacity*3, never two workgroups in one dword.  capacity 0 launches nothing.
 * No atomics and no waiting between workgroups: the same input gives the same bits on every call.
 * A null required pointer, a dimension below 1, nx*ny*nz >= 2^31, a voxel, trunc or max_weight that is not finite and positive, a selection the
 * cloud refuses or with step != 1, a cam_stride other than 0 or 18, frames given to a volume without colour or a coloured volume integrated
 * without frames, a workspace that is missing, short or not 8-byte aligned, and capacity < 0 return non-zero and launch nothing. */
typedef struct edv_tsdf_volume {
    float *tsdf_dev, *weight_dev, *color_dev;
    int32_t nx, ny, nz;
    double origin[3], voxel, trunc;
    float max_weight;
} edv_tsdf_volume;
int edv_tsdf_integrate(const edv_tsdf_volume *vol, const edv_cloud_selection *sel, const double *cams_dev, int32_t cam_stride, const uint8_t *frames_dev,
                       void *stream);
int32_t edv_tsdf_tile_voxels(void);
size_t edv_tsdf_workspace(int32_t nx, int32_t ny, int32_t nz);
int edv_tsdf_count(const edv_tsdf_volume *vol, float min_weight, int64_t *total_dev, void *workspace_dev, size_t workspace_bytes, void *stream);
int edv_tsdf_extract(const edv_tsdf_volume *vol, float min_weight, const void *workspace_dev, size_t workspace_bytes, float *points_dev, uint8_t *colors_dev,
                     int64_t capacity, void *stream);

/* ---- triangle meshes from the volume (fusion.Tsdf.mesh, model.video_surface(surface="mesh")) ----
 * Additive entry points: the ABI version stays as it is.  Marching tetrahedra on the Kuhn split of every cell: six tetrahedra around the body
 * diagonal, the same in every cell, so neighbouring cells agree on the diagonals of their shared faces.  A 16-case rule with no ambiguous case,
 * a watertight and consistently oriented mesh, up to 12 triangles a cell.  The volume is only read.
 * Corners and offsets: corner c in 0..7 of a cell has offset off(c) = (c & 1, c >> 1 & 1, c >> 2 & 1) in (x, y, z); off(d), d in 1..7, is also
 *   the linear hop.  Voxel a is observed when weight[a] >= min_weight and inside when tsdf[a] < 0; 0 and -0 are outside, as for the points.
 * Cells: the cell of voxel a exists when i_x + 1 < nx, i_y + 1 < ny and i_z + 1 < nz, and is valid when its eight corners are observed.  Only
 *   valid cells emit triangles.
 * Vertices: voxel a owns the seven edges a -> a + off(d), d = 1..7 (three axis edges, three face diagonals, the body diagonal).  Edge (a, d)
 *   carries a vertex when b = a + off(d) is in the grid, a and b are observed, inside(a) != inside(b), and a valid cell contains the edge: the
 *   cell of voxel a - off(s) for some s in 0..7 with (s & d) == 0 that lies in the grid.  Vertices are ordered voxel-major (x fastest), d-minor;
 *   none is left unreferenced.
 *     fp32  t = tsdf_a / (tsdf_a - tsdf_b)
 *     fp64  p_k = origin[k] + (d_k ? (i_k + 0.5) + (double)t : (i_k + 0.5)) * voxel;  stored as float
 *     fp32  per channel c = c_a + t * (c_b - c_a);  colour = (uint8) min(255, max(0, floor(c + 0.5)))          (exactly the points' colour)
 *     fp32  normal, every operation rounded on its own: the gradient of a voxel is g_k = tsdf[i_k -> min(i_k + 1, n_k - 1)] -
 *           tsdf[i_k -> max(i_k - 1, 0)], with no division (unobserved voxels contribute their stored value, a fresh one 1);
 *           n_k = g_k(a) + t * (g_k(b) - g_k(a));  s = (n_x*n_x + n_y*n_y) + n_z*n_z;  len = sqrt(s), correctly rounded;
 *           the normal is n_k / len if len > 0 and (0, 0, 0) otherwise.  It points to the positive side, free space, which the triangles face.
 * Tetrahedra: for the permutations (p, q, r) of (0, 1, 2) in lexicographic order the corners (c0, c1, c2, c3) = (0, 1 << p,
 *   (1 << p) | (1 << q), 7); bit i of the case mask m is set when corner c_i is inside.
 * Triangles per case, ins and outs being the corner positions i in ascending order: m = 0 or 15 gives none; one inside a the polygon
 *   [(a, o) for o in outs]; one outside o the polygon [(i, o) for i in ins]; two inside a < b and two outside c < d the polygon
 *   [(a, c), (a, d), (b, d), (b, c)].  With the polygon's points at the edge midpoints of the unit cube, the list is reversed when
 *   (P1 - P0) x (P2 - P0) . (mean of the outside corners - mean of the inside corners) < 0.  (P0, P1, P2) is emitted, and for a quad also
 *   (P0, P2, P3).  Polygon edge (i, j) is the cube edge between corners c_i and c_j: the smaller corner u is the owner's offset, d = v - u, and
 *   the triangle stores the index of that vertex.  Triangles are ordered cell-major (linear index of the cell's voxel), then tetrahedron, then
 *   the one or two triangles; indices are int32.
 * Degenerate cases stay as the rule gives them: tsdf_a == 0 gives t = 0, so several vertices coincide and some triangles have zero area; the
 *   topology is unaffected and nothing is filtered.
 * edv_tsdf_mesh_workspace: 16 bytes per tile of edv_tsdf_tile_voxels() voxels and 6 bytes per voxel, 8-byte aligned device memory; 0 for
 *   dimensions the volume check refuses.
 * edv_tsdf_mesh_count (five launches) fills the workspace: a flags byte per voxel (observed, inside, cell valid); from the flags the 7-bit mask
 *   of the edges of a voxel that carry a vertex and the triangles of its cell, summed per tile by wave ballot and popcount; two 64-bit exclusive
 *   scans; the u32 index of every voxel's first vertex.  totals_dev[0] is the number of vertices, totals_dev[1] the number of triangles.
 * edv_tsdf_mesh_extract (up to two launches) takes the workspace as edv_tsdf_mesh_count left it for the same volume and min_weight and only
 *   reads it (min_weight itself is not read again: the flags hold every comparison with it).  It writes vertex g only when
 *   g < vertex_capacity: vertices_dev [vertex_capacity][3] fp32 and, where not NULL, normals_dev [vertex_capacity][3] fp32 and colors_dev
 *   [vertex_capacity][3] uint8 (the volume must then be coloured); and triangle g only when g < triangle_capacity: triangles_dev
 *   [triangle_capacity][3] int32.  Every store is one float, one byte or one int of one vertex or triangle.  A capacity of 0 launches nothing
 *   for that output.  The caller compares totals_dev[0] with 2^31 before it extracts: a vertex_capacity of 2^31 or more is refused.
 * No atomics and no waiting between workgroups: the same input gives the same bits on every call.
 * A null volume, totals, vertices or triangles pointer, the volume refusals above, a workspace that is missing, short or not 8-byte aligned,
 * outputs that are not 4-byte aligned, a negative capacity, a vertex capacity of 2^31 or more, and colours asked of a volume that has none
 * return non-zero and launch nothing. */
size_t edv_tsdf_mesh_workspace(int32_t nx, int32_t ny, int32_t nz);
int edv_tsdf_mesh_count(const edv_tsdf_volume *vol, float min_weight, int64_t *totals_dev, void *workspace_dev, size_t workspace_bytes, void *stream);
int edv_tsdf_mesh_extract(const edv_tsdf_volume *vol, float min_weight, const void *workspace_dev, size_t workspace_bytes, float *vertices_dev,
                          float *normals_dev, uint8_t *colors_dev, int64_t vertex_capacity, int32_t *triangles_dev, int64_t triangle_capacity,
                          void *stream);

/* ---- views of the fused surface (fusion.Tsdf.raycast, model.video_surface(surface="views")) ----
 * An additive entry point: the ABI version stays as it is.  Every pixel of every view marches its ray through the volume in equal steps of
 * depth and stops where the interpolated distance changes from outside to inside between two neighbouring valid samples.  The volume is only
 * read.  fusion.TsdfHost.raycast is the numpy mirror, bit for bit.  Every operation below is rounded on its own (no contraction, no fast math).
 * cams_dev [views][21] doubles: per view Kinv [3][3], R [3][3] and t [3] of the point cloud (cloud.Cloud.cams), formed once on the host.
 * inv = 1.0 / voxel in fp64, formed once on the host.  steps = floor((far - near) / step) + 1 is the caller's, at most 65536.
 * Per pixel (x, y) of view f, in fp64:
 *     u = x + 0.5, v = y + 0.5;  l_i = (Kinv[i][0]*u + Kinv[i][1]*v) + Kinv[i][2]
 *     r_i = (R[i][0]*l_0 + R[i][1]*l_1) + R[i][2]*l_2                   (the cloud's ray: a point at depth z is t + r*z)
 *     o_i = (t_i - origin[i]) * inv - 0.5;  d_i = r_i * inv             (the ray in voxel-centre coordinates)
 * The sample at parameter z:
 *     fp64  g_i = o_i + d_i * z;  inside <=> 0 <= g_i <= n_i - 1 for i = x, y, z (NaN fails)
 *           c_i = min(max((int)g_i, 0), n_i - 2);  f_i = (float)(g_i - (double)c_i)
 *           valid <=> inside and the eight voxels c + off(0..7) all have weight >= min_weight
 *     fp32  along x: a00 = v000 + f_x*(v100 - v000), and a10, a01, a11 likewise for (y+1), (z+1), (y+1, z+1)
 *           along y: b0 = a00 + f_y*(a10 - a00), b1 = a01 + f_y*(a11 - a01);  along z: s = b0 + f_z*(b1 - b0)
 * The march, k = 0 .. steps-1 with z_k = near + (double)k * step in fp64 (not accumulated):
 *     sample k not valid: the previous sample is forgotten;  valid and not s < 0 (0 and -0 are outside, as everywhere here): (s, k) is
 *     remembered as the previous sample;  valid, s < 0 and sample k-1 remembered: a hit;  valid and s < 0 otherwise: the ray ends as a miss
 *     (it entered the surface from unobserved space, or started inside);  the steps run out: a miss.
 * The hit:
 *     fp32  t = s_prev / (s_prev - s)                                   (the divisor is positive)
 *     fp64  z* = z_{k-1} + (double)t * step;  depth = (float)z*
 *     (c, f) from z* by the formulas above (the clamp keeps them defined whatever the rounding); weights are not consulted again
 *     fp32  normal: the gradients of the eight corners (the mesh's, no division), each component interpolated in the order above;
 *           s = (n_x*n_x + n_y*n_y) + n_z*n_z;  len = sqrt(s), correctly rounded;  n_k / len if len > 0 and (0, 0, 0) otherwise
 *           colour: the eight stored colours interpolated per channel in the same order; (uint8) min(255, max(0, floor(c + 0.5)))
 * A miss writes depth 0, normal (0, 0, 0) and colour (0, 0, 0).  A volume with some n_i = 1 has no cell: every pixel is a miss.
 * depth_dev [views][h][w] fp32; normals_dev [views][h][w][3] fp32 or NULL; colors_dev [views][h][w][3] uint8 or NULL (not NULL only for a
 * coloured volume).  Every pixel of every output given is written exactly once, hit or miss, so nothing needs clearing.
 * One launch, one thread per pixel, a workgroup a 16 x 16 pixel tile.  Each ray skips the samples a slab test shows to lie outside the box
 * of voxel centres; the test inside the loop stays authoritative, so only samples the rule calls not valid are skipped.
 * No atomics and no waiting between workgroups: the same input gives the same bits on every call.
 * A null volume, cameras or depth pointer, the volume refusals above, cameras not 8-byte and depth or normals not 4-byte aligned, views, h or
 * w below 1, views*h*w >= 2^31, a step that is not finite and positive, a near that is not finite, steps outside 1..65536, and colours asked
 * of a volume that has none return non-zero and launch nothing. */
int edv_tsdf_raycast(const edv_tsdf_volume *vol, const double *cams_dev, int32_t views, int32_t h, int32_t w, double near, double step, int32_t steps,
                     float min_weight, float *depth_dev, float *normals_dev, uint8_t *colors_dev, void *stream);

/* ---- camera tracking against the fused surface (fusion.icp_sums, fusion.Tsdf.track, model.video_surface(track=...)) ----
 * Additive entry points: the ABI version stays as it is.  One step of frame-to-model point-to-plane ICP: a live depth frame, lifted through the
 * current estimate of its camera, is associated projectively with one view of edv_tsdf_raycast (the model's depth and normal maps seen from
 * the previous pose), and the normal equations of the twist are summed over the pairs.  Nothing but sums_dev and the workspace is written.
 * fusion.icp_sums_host is the numpy mirror, bit for bit.  Every multiply, add and divide below is rounded on its own.
 * sel and frame: the cloud's selection and one frame of it, 0 <= frame < sel->n.  The output grid is the cloud's, oh = ceil(h/step),
 *   ow = ceil(w/step); output pixel (oy, ox) samples the source pixel the selection names, and its z (fp32) and kept are the selection's.
 * live_cam_host: 21 doubles in host memory, Kinv[3][3], R[3][3], t[3] of the CURRENT estimate (a row of cloud.Cloud.cams).
 * model_cam_host: 39 doubles in host memory: the model view's own 21 as above (Kinv_m, R_m, t_m), then W[3][4] and K00 K01 K02 K10 K11 K12 of
 *   edv_tsdf_integrate for the same camera.  Both arrays are read before the call returns and travel in the launch arguments: the live pose
 *   changes with every iteration, and nothing is staged.
 * model_depth_dev [mh][mw] fp32 and model_normals_dev [mh][mw][3] fp32: one view of edv_tsdf_raycast.
 * Per kept output pixel, in fp64:
 *     u = (ox + 0.5) * step;  v = (oy + 0.5) * step;  l_i = (Kinv[i][0]*u + Kinv[i][1]*v) + Kinv[i][2]
 *     r_i = (R[i][0]*l_0 + R[i][1]*l_1) + R[i][2]*l_2;  rho_i = r_i * (double)z;  P_i = t_i + rho_i            (the cloud's point, kept in fp64)
 *     q_i = ((W[i][0]*P_x + W[i][1]*P_y) + W[i][2]*P_z) + W[i][3];   skip unless q_2 > 0 (which also skips NaN)
 *     um = ((K00*q_0 + K01*q_1) + K02*q_2) / q_2;  vm = ((K10*q_0 + K11*q_1) + K12*q_2) / q_2
 *     skip unless um >= 0 && um < mw && vm >= 0 && vm < mh, tested in fp64 before any conversion;  px = (int)um, py = (int)vm
 *     dm = model_depth[py][px];  skip unless dm > 0 (a miss is +0, NaN fails);  N = (double)model_normals[py][px][0..2]
 *     skip unless (N_x*N_x + N_y*N_y) + N_z*N_z > 0
 *     lm_i = (Kinv_m[i][0]*(px + 0.5) + Kinv_m[i][1]*(py + 0.5)) + Kinv_m[i][2];  rm_i = (R_m[i][0]*lm_0 + R_m[i][1]*lm_1) + R_m[i][2]*lm_2
 *     V_i = t_m,i + rm_i * (double)dm;  D_i = V_i - P_i;  skip unless (D_x*D_x + D_y*D_y) + D_z*D_z <= max_dist2
 *     e = (N_x*D_x + N_y*D_y) + N_z*D_z;  c = rho x N, each product rounded and then the difference: c_x = rho_y*N_z - rho_z*N_y, and so on
 *     J = (c_x, c_y, c_z, N_x, N_y, N_z): the twist (rotation, then translation) is about the live camera centre, which keeps the system well
 *     conditioned far from the world origin.
 *   The pixel's 29 terms: J_j*J_k for j <= k, the upper triangle row-major (21); J_j*e (6); e*e; 1.0.  A pixel that is skipped, not kept or
 *   past the grid contributes 29 times +0.0.
 * The sums, in fp64, in a fixed order, with no atomics: tile b holds output pixels 256*b .. 256*b + 255 in row-major order, a wave 64
 *   consecutive pixels.  Inside a wave a butterfly: for s = 32, 16, 8, 4, 2, 1 every lane x <- x + x[lane ^ s].  The tile's sum is
 *   ((w0 + w1) + w2) + w3 of its four waves, written to the workspace as [tile][29].  A second launch adds, for each of the 29 values, the tiles
 *   in index order starting from tile 0's value, and writes sums_dev[0..28].  sums_dev[28] is the number of pairs, sums_dev[27] their squared
 *   residuals.  Every workspace slot that is read and all 29 outputs are written on every call: neither needs clearing, and the same input
 *   gives the same bits on every call.
 * edv_icp_tile_pixels(): 256.  edv_icp_workspace: 29 * 8 bytes per tile, ceil(oh*ow / 256) tiles, 8-byte aligned device memory; 0 for a shape
 *   the call refuses.
 * The model is addressed only after the range test above and the live frame only inside its grid: a guess that looks anywhere reads nothing
 *   outside the arrays.
 * Null required pointers, a selection the cloud refuses (step < 1 among them), frame outside [0, sel->n), mh or mw < 1, mh*mw >= 2^31, model
 * maps not 4-byte aligned, a max_dist2 that is not finite or not >= 0, sums_dev not 8-byte aligned and a workspace that is missing, short or
 * not 8-byte aligned return non-zero and launch nothing. */
int32_t edv_icp_tile_pixels(void);
size_t edv_icp_workspace(int32_t h, int32_t w, int32_t step);
int edv_icp_sums(const edv_cloud_selection *sel, int64_t frame, const double *live_cam_host, const double *model_cam_host, const float *model_depth_dev,
                 const float *model_normals_dev, int32_t mh, int32_t mw, double max_dist2, double *sums_dev, void *workspace_dev, size_t workspace_bytes,
                 void *stream);

/* ---- the same step with the frame's depth scale as a seventh unknown (fusion.Track(scale=True), fusion.icp_sums(..., scale=True)) ----
 * Additive entry points: the ABI version stays as it is.  Monocular depth is fixed only up to a scale that wanders from frame to frame; a
 * tracker that takes every frame's depth in the volume's unit trades that scale for rotation and translation.  Here the scale is estimated
 * with the pose.
 * Where the scale lives: in the selection's gain, the one place the depth rule has for it.  For a scale factor sigma (a double on the host) the
 *   frame is read with gain = (float)(spec.gain * sigma), the product formed in doubles and rounded once, so z (fp32) and kept are the
 *   selection's for that gain, near and far applied to the scaled depth.  The call takes no new scalar, and edv_tsdf_integrate with the same
 *   gain sees exactly the z the tracker saw.
 * Per kept output pixel everything up to e and J_0..J_5 is edv_icp_sums' rule above, character for character.  The seventh column, in fp64,
 *   every operation rounded on its own:
 *     J_6 = (rho_x*N_x + rho_y*N_y) + rho_z*N_z
 *   Growing the scale by delta moves P by delta*rho, so e falls by delta*J_6: the sign convention of the translation columns.
 *   The pixel's 37 terms: [0..27] J_j*J_k for 0 <= j <= k <= 6, the upper triangle row-major; [28..34] J_j*e for j = 0..6; [35] e*e; [36] 1.0.
 *   A pixel without a pair contributes 37 times +0.0.
 * The sums exactly as above: tiles of 256 output pixels, a butterfly per wave, ((w0 + w1) + w2) + w3 to the workspace as [tile][37], then the
 *   tiles in index order from tile 0's value into sums_dev[0..36]; fp64, no atomics.  The 29 values that edv_icp_sums also has (the triangle's
 *   entries with k <= 5, [28..33], [35], [36]) come out with the same bits as it gives for the same inputs.  Every workspace slot that is read
 *   and all 37 outputs are written on every call.
 * On the host (fusion._track): x = (rotation vector, translation, delta) of the symmetric 7 x 7 system; T <- twist(T, x[0..5]);
 *   sigma <- sigma * (1.0 + x[6]).  The frame is lost as above, and also when sigma is not finite and positive or sigma / sigma_guess leaves
 *   [1/(1+m), 1+m], m = Track.max_scale_step.  A lost frame returns its guess, pose and factor 1.0.
 * edv_icp_scaled_workspace: 37 * 8 bytes per tile, 0 for a shape the call refuses.  edv_icp_scaled_sums: the arguments and the refusals of
 *   edv_icp_sums; it writes sums_dev[0..36]. */
size_t edv_icp_scaled_workspace(int32_t h, int32_t w, int32_t step);
int edv_icp_scaled_sums(const edv_cloud_selection *sel, int64_t frame, const double *live_cam_host, const double *model_cam_host, const float *model_depth_dev,
                        const float *model_normals_dev, int32_t mh, int32_t mw, double max_dist2, double *sums_dev, void *workspace_dev, size_t workspace_bytes,
                        void *stream);

/* ---- the same step with a photometric block (fusion.Track(colour=...), fusion.icp_colour_sums) ----
 * Additive entry points: the ABI version stays as it is.  Point-to-plane ICP sees nothing of a motion that slides the surface along itself: on
 * a plane, inside a lumen.  The volume is coloured and so is the live frame; here every geometric pair also compares the live pixel's intensity
 * with the model view's colour image, sampled bilinearly where the point projects, and a second block of sums holds the normal equations of
 * that residual.  One launch forms both blocks from one association.  fusion.icp_colour_sums_host is the numpy mirror, bit for bit.
 * frames_dev: uint8 [n][h][w][3], the clip's RGB frames.  model_colors_dev: uint8 [mh][mw][3], the colours of the same view of
 *   edv_tsdf_raycast as model_depth_dev and model_normals_dev.  cols: 6 (edv_icp_sums' columns) or 7 (edv_icp_scaled_sums', with J_6);
 *   T = 29 or 37.
 * Per kept output pixel everything through the distance test and e, J_0..J_5 (and J_6 with cols = 7) is edv_icp_sums' rule above, character for
 *   character.  A pixel without a geometric pair has no colour pair either.  A pixel with one continues, in fp64, every operation rounded on
 *   its own, with um, vm, q_0..q_2, rho, W, K the values that rule formed:
 *     gu = um - 0.5;  gv = vm - 0.5                                                             (the model's pixel centres lie at the integers)
 *     no colour pair unless mw >= 2 && mh >= 2 && 0 <= gu && gu <= mw-1 && 0 <= gv && gv <= mh-1, tested in fp64 before any conversion
 *     x0 = min((int)gu, mw-2);  y0 = min((int)gv, mh-2);  fx = gu - x0;  fy = gv - y0
 *     no colour pair unless model_depth[y0+j][x0+i] > 0 for i, j in {0, 1}: a miss's colour is (0, 0, 0), which is not a colour
 *     Y(R, G, B) = (0.299*R + 0.587*G) + 0.114*B of a uint8 triple, the constants the doubles nearest those decimals
 *     I00, I10, I01, I11 = Y(model_colors[y0][x0]), Y([y0][x0+1]), Y([y0+1][x0]), Y([y0+1][x0+1])
 *     Yl = Y(frames[frame] at the source pixel the depth was read from): step > 1 samples colour where it samples depth
 *     top = I00 + fx*(I10-I00);  bot = I01 + fx*(I11-I01);  Im = top + fy*(bot-top)
 *     Iu = (I10-I00) + fy*((I11-I01) - (I10-I00));  Iv = (I01-I00) + fx*((I11-I10) - (I01-I00))      (the interpolant's exact gradient)
 *     a = K00*q_0 + K01*q_1;  b = K10*q_0 + K11*q_1
 *     gq_0 = (Iu*K00 + Iv*K10) / q_2;  gq_1 = (Iu*K01 + Iv*K11) / q_2;  gq_2 = -((Iu*a + Iv*b) / (q_2*q_2))   (in the model camera's frame)
 *     g_j = (W[0][j]*gq_0 + W[1][j]*gq_1) + W[2][j]*gq_2,  j = 0..2                                            (in the world)
 *     r = Yl - Im.  Moving P by delta raises the model's intensity by g . delta, so r falls by g . delta: the sign convention of e and N.
 *     Jc = (rho x g, g), each product rounded and then the difference, exactly as for N;  with cols = 7, Jc_6 = (rho_x*g_x + rho_y*g_y) + rho_z*g_z
 *   The pixel's colour terms: the layout of the geometric block with Jc for J and r for e: the upper triangle row-major, Jc_j*r, r*r, 1.0.  A
 *   pixel without a colour pair contributes T times +0.0 to the colour block.
 * The sums: 2*T values, [0..T) the geometric block and [T..2T) the colour block; exactly as above, tiles of 256 output pixels, a butterfly per
 *   wave, ((w0 + w1) + w2) + w3 to the workspace as [tile][2*T], then per value the tiles in index order from tile 0's value into
 *   sums_dev[0..2T); fp64, no atomics.  The geometric block has the bits of edv_icp_sums (cols = 6) or edv_icp_scaled_sums (cols = 7) for the
 *   same inputs.  sums_dev[2T-1] is the number of colour pairs.  Every workspace slot that is read and all 2*T outputs are written on every call.
 * On the host (fusion._track) with the weight lambda = Track.colour, an intensity unit against a unit of length: A = A_g + lambda^2 * A_c,
 *   b = b_g + lambda^2 * b_c, formed in fp64 and solved as before; pairs, rms and the lost rules stay the geometric block's.
 * The model's colour image is addressed only after the fp64 range tests (0 <= x0 <= mw-2, 0 <= y0 <= mh-2) and the live image only inside its
 *   grid: a guess that looks anywhere reads nothing outside the arrays.
 * edv_icp_colour_workspace: 2*T * 8 bytes per tile; 0 for a shape the call refuses or cols outside {6, 7}.  edv_icp_colour_sums: the refusals
 *   of edv_icp_sums, and also null frames_dev, null model_colors_dev and cols outside {6, 7}; a refused call launches nothing. */
size_t edv_icp_colour_workspace(int32_t h, int32_t w, int32_t step, int32_t cols);
int edv_icp_colour_sums(const edv_cloud_selection *sel, int64_t frame, const uint8_t *frames_dev, const double *live_cam_host, const double *model_cam_host,
                        const float *model_depth_dev, const float *model_normals_dev, const uint8_t *model_colors_dev, int32_t mh, int32_t mw, double max_dist2,
                        int32_t cols, double *sums_dev, void *workspace_dev, size_t workspace_bytes, void *stream);

/* ---- robust tracking: live normal maps, a normal test and Huber weights (fusion.Track(min_cos=..., huber=..., huber_colour=...)) ----
 * Additive entry points: the ABI version stays as it is.  The steps above believe every pair that passes the distance test; a highlight, an
 * instrument or tissue that moved gives pairs that pass it and are wrong.  Two tests of a pair against the model: its orientation (the live
 * frame's own normal against the model's) and the size of its residual (a Huber weight).  fusion.frame_normals_host and
 * fusion.icp_robust_sums_host are the numpy mirrors, bit for bit.  All of it fp64, every operation rounded on its own.
 *
 * edv_frame_normals: the normal of every output pixel of frames first .. first + count - 1 of the selection, in the CAMERA's frame (it does not
 *   depend on the pose), into normals_dev [count][oh][ow][3] fp32 on the cloud's output grid.  cams_dev and cam_stride are edv_cloud_scatter's
 *   (device doubles, 21 a camera, stride 0 or 21); only Kinv is read.  One thread per output pixel and frame; every element is written once.
 *     vertex  of output pixel (oy, ox), with z (fp32) and kept the selection's:  u = (ox + 0.5) * step;  v = (oy + 0.5) * step;
 *             l_i = (Kinv[i][0]*u + Kinv[i][1]*v) + Kinv[i][2];  V_i = l_i * (double)z
 *     valid   when 1 <= ox <= ow-2 and 1 <= oy <= oh-2 and the pixel and its four neighbours (oy, ox-1), (oy, ox+1), (oy-1, ox), (oy+1, ox) are kept
 *     normal  a = V(oy, ox+1) - V(oy, ox-1);  b = V(oy+1, ox) - V(oy-1, ox);  c = b x a, each product rounded and then the difference:
 *             c_0 = b_1*a_2 - b_2*a_1, c_1 = b_2*a_0 - b_0*a_2, c_2 = b_0*a_1 - b_1*a_0.  With x right, y down and z forward c points towards
 *             the camera, the free side, as the model's normals do.  s = (c_0*c_0 + c_1*c_1) + c_2*c_2;  len = sqrt(s), correctly rounded;
 *             n_i = (float)(c_i / len) if len > 0 (NaN fails)
 *     A pixel that is not valid or has len = 0 gets (0, 0, 0).
 *   Null pointers, a selection the cloud refuses, cameras not 8-byte or normals not 4-byte aligned, a cam_stride other than 0 and 21, first < 0,
 *   count < 1 and first + count > sel->n return non-zero and launch nothing.
 *
 * edv_icp_robust_sums: edv_icp_sums (cols = 6) or edv_icp_scaled_sums (cols = 7), and with the colour block edv_icp_colour_sums, with the two
 *   tests.  The colour block is present exactly when frames_dev and model_colors_dev are both given; T = 29 or 37, and the sums are T or 2*T.
 *   live_normals_dev: [oh][ow][3] fp32, edv_frame_normals of frame `frame` alone (first = frame, count = 1); null: no normal test.
 *   huber, huber_colour: the thresholds of the geometric and of the colour residual, > 0; +inf turns a weight off.
 * Per kept output pixel q everything through the distance test, e and J is edv_icp_sums' rule above, character for character.  Then:
 *     normal test, when live_normals_dev is given:  nl = (double)live_normals[q][0..2];  skip unless (nl_0*nl_0 + nl_1*nl_1) + nl_2*nl_2 > 0;
 *             nw_i = (R[i][0]*nl_0 + R[i][1]*nl_1) + R[i][2]*nl_2 with R of the current estimate;  cos = (N_0*nw_0 + N_1*nw_1) + N_2*nw_2;
 *             skip unless cos >= min_cos.  A skipped pixel has no pair and no colour pair.
 *     weight  w = 1.0 if |e| <= huber, otherwise huber / |e| (IEEE division)
 *     terms   Jw_j = w * J_j;  Jw_j*J_k for j <= k in the order above;  Jw_j*e;  then e*e, UNWEIGHTED, and 1.0: the number of pairs and their rms
 *             keep their meaning and the layout stays 29 / 37.  Since 1.0 * x == x, a pair inside the threshold contributes the plain kernel's bits.
 *     colour  the colour pair by edv_icp_colour_sums' rule; w_c from |r| and huber_colour;  Jcw_j = w_c * Jc_j;  Jcw_j*Jc_k, Jcw_j*r, r*r, 1.0
 * The sums exactly as above: tiles of 256, the butterfly, ((w0 + w1) + w2) + w3 to the workspace, the tiles in index order; no atomics; every
 *   workspace slot that is read and every output is written on every call.  With no normals and both thresholds +inf the sums have the bits of
 *   edv_icp_sums, edv_icp_scaled_sums or edv_icp_colour_sums.
 * edv_icp_robust_workspace: T * 8 bytes per tile, twice that with colour = 1; 0 for a shape the call refuses, cols outside {6, 7} or colour
 *   outside {0, 1}.  edv_icp_robust_sums: the refusals of edv_icp_sums, and also cols outside {6, 7}, a min_cos that is not finite or outside
 *   [-1, 1] (with or without live normals), a threshold that is NaN or not > 0, and live normals not 4-byte aligned; a refused call launches
 *   nothing. */
int edv_frame_normals(const edv_cloud_selection *sel, const double *cams_dev, int32_t cam_stride, int64_t first, int64_t count, float *normals_dev, void *stream);
size_t edv_icp_robust_workspace(int32_t h, int32_t w, int32_t step, int32_t cols, int32_t colour);
int edv_icp_robust_sums(const edv_cloud_selection *sel, int64_t frame, const uint8_t *frames_dev, const double *live_cam_host, const double *model_cam_host,
                        const float *model_depth_dev, const float *model_normals_dev, const uint8_t *model_colors_dev, int32_t mh, int32_t mw, double max_dist2,
                        int32_t cols, const float *live_normals_dev, double min_cos, double huber, double huber_colour, double *sums_dev, void *workspace_dev,
                        size_t workspace_bytes, void *stream);

/* ---- coarse-to-fine tracking: depth and colour pyramids of the live frame (fusion.Track(pyramid=..., jump=...), fusion.depth_pyramid, fusion.rgb_pyramid) ----
 * Additive entry points: the ABI version stays as it is.  The steps above run at one resolution.  With a pyramid the tracker runs its first steps
 * on coarse copies of the live frame against the volume ray-cast at the same coarse size: a step at half size works on a quarter of the
 * pixels, and the same motion is a smaller displacement in large pixels.  The sums, the normals and the ray-cast take any grid size and any
 * intrinsics, so the device work that is new is what makes the levels.  fusion.depth_pyramid_host and fusion.rgb_pyramid_host are the numpy
 * mirrors, bit for bit.
 * Levels: level 0 is the frame, h_0 x w_0.  Level l+1 is (h_l / 2) x (w_l / 2), the division rounded down: an odd last row or column is
 *   dropped.  Every level must hold a pixel.  edv_pyramid_max_levels(): 6, level 0 included, so 1 <= levels <= 5 coarser levels a call.
 *   Pixel (y, x) of level l+1 is made from the block (2y, 2x), (2y, 2x+1), (2y+1, 2x), (2y+1, 2x+1) of level l, in that order.  With pixel
 *   centres at x + 0.5 the camera of level l is K_l = diag(2^-l, 2^-l, 1) K, exactly.
 * edv_depth_pyramid: the selection is the cloud's with step == 1, near_z >= 0 and gain > 0; frame is one frame of it.  All of it fp32, every
 *   operation rounded on its own:
 *     level 0   d = x (mode 0), or d = 1 / (lo + span*x) (mode 1): the selection's depth rule without its last multiply by gain.  The pixel is
 *               valid when the selection keeps it: mask != 0 and near_z < d*gain < far_z (NaN and Inf fail).  A valid d is > 0.
 *     level >=1 a pixel is valid when its stored value is not 0.
 *     reduce    m = the smallest valid value of the block;  a valid value is used when d <= m * one_plus_jump;  s = the used values added in
 *               block order, starting from the first used one;  c = their number;  the stored value is s / (float)c, or +0 where nothing is
 *               valid.  The nearest surface wins: a block across a depth edge is not smeared.  one_plus_jump = +inf uses every valid value,
 *               1 only those equal to m.
 *   The gain stays out of the stored values: a level is an ordinary mode-0 clip for the calls above with the gain of level 0, z = d * gain,
 *   and their near_z < z test drops the zeros.
 * edv_rgb_pyramid: frames_dev uint8 [n][h][w][3], frame one of them; per channel (a + b + c + d + 2) >> 2 over the same block, in integers.
 * The output of either call: levels 1 .. levels one behind the other, tightly, each row-major: level l starts offsets[l-1] pixels into the
 *   buffer, 4 bytes a pixel for depth and 3 for colour.  edv_pyramid_pixels returns the pixels of all levels together and, where offsets_host
 *   is not NULL, writes offsets_host[0 .. levels-1]; it returns 0, and writes nothing, for a shape the calls refuse.
 * One launch a call, all levels: a workgroup of 256 owns a 32 x 32 tile of level 0 (32 = 2^5: the tile holds whole blocks of every level),
 *   reads its pixels of level 0 once, stores level 1 and reduces on through LDS.  No atomics, no waiting between workgroups; every pixel of
 *   every level is written exactly once, zeros included, and nothing else is: the buffer needs no clearing and the same input gives the same bits.
 * A null pointer, a selection the cloud refuses or with step != 1, near_z < 0 or gain <= 0 (or NaN), frame outside the clip, one_plus_jump
 * below 1 or NaN, levels outside 1 .. 5, a level without a pixel, h*w >= 2^31 and a depth output that is not 4-byte aligned return non-zero and
 * launch nothing. */
int32_t edv_pyramid_max_levels(void);
size_t edv_pyramid_pixels(int32_t h, int32_t w, int32_t levels, int64_t *offsets_host);
int edv_depth_pyramid(const edv_cloud_selection *sel, int64_t frame, int32_t levels, float one_plus_jump, float *levels_dev, void *stream);
int edv_rgb_pyramid(const uint8_t *frames_dev, int64_t n, int32_t h, int32_t w, int64_t frame, int32_t levels, uint8_t *levels_dev, void *stream);

/* ---- whole-video stitching on the device (infer_video_depth(stitch="device"); endodav.py:213-254, utils/util.py:40-74) ----
 * disp_dev: one window's network-size disparity [32, ih, iw].  Both calls upsample it to the frame size [fh, fw] on the fly (bilinear,
 * align_corners=True, bit-identical to edv_bilinear), so the 32 frame-size maps are never materialised.
 * edv_stitch_fit: least-squares (s, t) with s*p + t ~ tail over the 8 overlap pairs (window slots 2..9 against tail_dev [8, fh, fw], the
 * already aligned last 8 frames of the output so far).  Sums and the 2x2 solve in fp64, reduced in a fixed order (same input, same bits);
 * det == 0 gives (1, 0).  st_dev [2] receives (s, t) rounded to fp32; nothing comes back to the host.
 * edv_stitch_apply: reads (s, t) from st_dev; writes max(p*s + t, 0) of slots 10..31 to new_dev [22, fh, fw] and the cross-fade
 * pre*(1 - f_i) + max(p*s + t, 0)*f_i of slots 2..9 in place over tail_dev (f_i = 0, 1/7, ..., 1 rounded to fp32).  Window 0:
 * st_dev = tail_dev = NULL, new_dev [32, fh, fw] receives the plain upsample of all 32 slots (no clamp).
 * 16-byte accesses when fh*fw is a multiple of 4 and tail_dev / new_dev are 16-byte aligned, one pixel per access otherwise. */
size_t edv_stitch_workspace(void); /* bytes; the same for every size */
int edv_stitch_fit(const float *disp_dev, int32_t ih, int32_t iw, const float *tail_dev, int32_t fh, int32_t fw, float *st_dev, void *workspace_dev,
                   size_t workspace_bytes, void *stream);
int edv_stitch_apply(const float *disp_dev, int32_t ih, int32_t iw, const float *st_dev, float *tail_dev, float *new_dev, int32_t fh, int32_t fw,
                     void *stream);

/* ---- video-depth evaluation on the device (evaluate_video(metrics="device"); evaluate_depth_video.py:163-215, utils/utils.py:112-133,
 * utils/layers.py:11-20, utils/eval_utils.py:63-143,265-282) ----
 * A clip is [n, h, w] fp32; results and scalars are doubles in device memory (an fp32 value or a count is held exactly) and nothing comes back to
 * the host.  Same input, same bits: sums are fp64 in a fixed order, the only atomics are integer ones.  No product is fused into a sum.
 * edv_masked_median: out_dev[0] = np.median (float32 semantics: the middle order statistic, or the fp32 mean of the two middle ones) of x[i]
 * over lo < gate[i] < hi, bit for bit; out_dev[1] = the number selected; none selected gives NaN.  Exact radix select (four 8-bit histogram
 * passes, 64-bit counts).  x may alias gate.  Inputs are finite: NaN in x is unsupported, NaN in gate fails the comparison.
 * edv_metrics_pred: pred = 1 / (1/max_depth + (1/min_depth - 1/max_depth) * disp); align 1 ("scale"): pred * (median gt / median pred);
 * align 2 ("scale_shift"): (pred - t_pred) * (s_gt / s_pred) + t_gt with t the medians and s the mean absolute deviations (summed in fp64,
 * rounded once to fp32), all over 1e-3 < gt < 150; then clip(pred * pred_depth_scale_factor, 1e-3, eval_max_depth).  fp32 operations in the
 * order of the host's; align 0 and 1 are bit-identical to it.  scalars_dev [8]: ratio, t_gt, s_gt, t_pred, s_pred, selected count, 2 spare.
 * edv_metrics_errors: out_dev [n][8] = valid count, abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3 of each frame over 1e-3 < gt < eval_max_depth:
 * fp32 terms as the host forms them, fp64 sums, divide and square root; a frame without a valid pixel gives NaN.
 * edv_metrics_temporal: out_dev [n-1][2] = (tae, tas) of each consecutive pair (tae not yet x 100).  mats_dev [n][2][16]: per frame
 * img2world = inv(K @ pose) and its inverse, row-major fp64, from the host.  fp64 geometry, every dot product a fixed left-to-right chain of
 * explicit fused multiply-adds (the accumulation of the host's dgemm, so rounding ties fall as they fall there); the splat is a
 * 64-bit atomic maximum of (source index + 1) << 32 | bits(float(z)), so the largest row-major source index wins a target pixel ("later
 * points overwrite earlier ones"); one splat per direction serves tae and tas.  An empty overlap gives NaN.  warp_dev (may be NULL)
 * [n-1][2][h][w] receives the resolved splats (a -> b, b -> a).  Pairs run in chunks of 4: the workspace does not grow with n.
 * edv_metrics_workspace(n, h, w): bytes for every call above on such a clip, 16-byte aligned; (0, 0, 0): all but edv_metrics_temporal. */
size_t edv_metrics_workspace(int64_t n, int32_t h, int32_t w);
int edv_masked_median(const float *x_dev, const float *gate_dev, int64_t count, float lo, float hi, double *out_dev, void *workspace_dev, size_t workspace_bytes,
                      void *stream);
int edv_metrics_pred(const float *disp_dev, const float *gt_dev, float *pred_dev, int64_t n, int32_t h, int32_t w, double min_depth, double max_depth, int32_t align,
                     float pred_depth_scale_factor, float eval_max_depth, double *scalars_dev, void *workspace_dev, size_t workspace_bytes, void *stream);
int edv_metrics_errors(const float *pred_dev, const float *gt_dev, int64_t n, int32_t h, int32_t w, float eval_max_depth, double *out_dev, void *workspace_dev,
                       size_t workspace_bytes, void *stream);
int edv_metrics_temporal(const float *pred_dev, const float *gt_dev, int64_t n, int32_t h, int32_t w, float eval_max_depth, const double *mats_dev, double *out_dev,
                         float *warp_dev, void *workspace_dev, size_t workspace_bytes, void *stream);

/* out = W + scale * (B∘V)(A∘U)  (U, V may be NULL): the LoRA / DV-LoRA fold of mylora/layers.py:148-157,384-393. */
int edv_fold_lora(const float *W_dev, const float *A_dev, const float *B_dev, const float *U_dev, const float *V_dev, float scale, float *out_dev,
                  int32_t nout, int32_t nin, int32_t r, void *stream);

/* ---- fine-tune step (trainer_end_to_end_video.py:731 forward, :427-431 backward/step) ----
 * edv_set_train(ctx, 1): edv_forward keeps the activations the backward needs (per encoder block: both residual-stream
 * values, the normed MLP input, q|k|v, the attention output and its log-sum-exp, the fc1 pre-activation; per motion module
 * and fusion block: the inputs of their norms and ReLUs; per output head its intermediates).  Every constructor option trains
 * (both output heads, lora_type none / lora / dvlora / ssb / dash in both of its phases, temporal_lora, use_clstoken, residual
 * blocks, inv_sigmoid, out_sigmoid, pe rope) except use_bn, whose train-mode BatchNorm (batch statistics) is not built: refused.
 * ONE set of activations per context: each training forward overwrites the previous one's and advances the context's generation
 * counter (edv_generation, read it right after the forward).
 * edv_backward(ctx, generation, disp0, grads): generation = the forward being differentiated (0 = do not check); a mismatch with
 * the kept activations is an error, never a silently wrong gradient.  disp0 = the ("disp", 0) map that forward wrote,
 * grads[k] = dL/d("disp", k), k = 0..3 (all four required, contiguous fp32).  Produces the gradients edv_set_grad_scope selects,
 * named like the state_dict: the LoRA factors of mlp.fc1 / mlp.fc2 ("pretrained.blocks.<i>.mlp.fc<j>.lora_{A,B,U,V,index}"), with
 * temporal_lora those of ff.net.2 in the motion modules, the output-head convolutions, the residual blocks, the biases -- the trainable sets
 * of endodav/layers.py:5-34 -- and, under edv_set_bias_grads, the biases (bias="all").  Where they land: a name listed in the caller's flat buffer (edv_grad_bind_flat) is written into its
 * slice there; any other into context-owned memory, read with edv_grad / edv_grad_copy.
 * After the optimizer step call edv_refresh_lora (or edv_prepare) before the next forward; edv_refresh_lora also covers any change of a
 * bias. */
int edv_set_train(edv_ctx *ctx, int32_t on);
/* Which gradients the next edv_backward has to produce.  The trainer alternates spatial and temporal tuning phases
 * (trainer_end_to_end_video.py:327-339); with encoder_factors = 0 the backward stops at the head (nothing below it is
 * trainable), with temporal_factors = 0 the ff.net.2 products are skipped.  head_convs != 0 adds the weight and bias gradients of
 * the output-head convolutions, named like the state_dict: "head.conv_depth_<k>.head.{0,2,4}.{weight,bias}" with the conv head
 * (trainable by default, endodav/layers.py:5-34), "head.scratch.output_conv1.*", "head.scratch.output_conv2.{0,2}.*" with the VDA
 * head (--train_output_conv).  residual_blocks != 0 adds every parameter of the ResBottleneckBlocks
 * ("pretrained.blocks.<i>.residual_.{conv1,conv2,conv3}.weight", ".norm{1,2,3}.{weight,bias}"; trainable by default in the reference,
 * block.py:146-150).  Default: both factor sets, nothing else. */
int edv_set_grad_scope(edv_ctx *ctx, int32_t encoder_factors, int32_t temporal_factors, int32_t head_convs, int32_t residual_blocks);
/* The bias gradients of mark_only_part_as_trainable(bias="all") (endodav/layers.py:5-34), on top of edv_set_grad_scope's sets.
 * encoder_biases != 0: every "pretrained.*bias" (patch_embed.proj, each block's norm1/2, attn.qkv/proj, mlp.fc1/fc2, residual_.norm1..3 if
 * present, the final norm); the backward then also runs block 0's attention and patch-embedding backward.  head_biases != 0: every
 * "head.*bias" the forward reaches (projects, resize_layers, readout_projects, the motion modules, refinenet* out_conv / resConfUnit
 * convolutions, conv_depth_* or output_conv*); refinenet4.resConfUnit1 is never reached and gets none.  With head_biases alone the
 * backward stops at the head.  Default 0 / 0.  Each bias gradient is one column sum of the dY of its operator (times the LayerScale
 * gamma for attn.proj / mlp.fc2), reduced in a fixed order: bit-reproducible. */
int edv_set_bias_grads(edv_ctx *ctx, int32_t encoder_biases, int32_t head_biases);
int edv_generation(const edv_ctx *ctx, uint64_t *generation);
int edv_backward(edv_ctx *ctx, uint64_t generation, const float *disp0_dev, const float *const grad_disp_dev[4], void *stream);
/* One contiguous gradient buffer owned by the caller, for the data-parallel step (the reference's nn.DataParallel reduce,
 * trainer_end_to_end_video.py:269-271; here ONE all-reduce over this buffer, in place).  names[i] / numels[i], i < n: the trainable
 * tensors in the caller's order.  offsets_out[0..n] receives each slice's offset in floats (slices start on 16-byte boundaries) and,
 * at [n], the total length.  flat_dev = NULL only computes the layout; otherwise flat_dev[flat_floats] must hold that total, and
 * from then on edv_backward writes the gradient of names[i] at flat_dev + offsets_out[i] -- the host's .grad tensors are views of
 * it, nothing is copied per tensor.  edv_backward fails if it produced no gradient for a listed name.  n = 0 unbinds. */
int edv_grad_bind_flat(edv_ctx *ctx, int32_t n, const char *const *names, const int64_t *numels, float *flat_dev, int64_t flat_floats,
                       int64_t *offsets_out);
int edv_grad(edv_ctx *ctx, const char *name, float **grad_dev, int64_t *numel);
int edv_grad_copy(edv_ctx *ctx, const char *name, float *dst_dev, int64_t numel, void *stream); /* stream-ordered copy into caller memory */

/* ---- the fine-tune step's loss ----
 * The trainer's photometric loss on the four disparity maps of B clips of T frames, and its gradient with respect to them, in one
 * call: per scale the map is resized to the frame size (bilinear, align_corners; trainer_end_to_end_video.py:813-817), turned into
 * depth (utils/layers.py:11-20), back-projected and projected into the previous / next frame of the clip (utils/layers.py:134-189),
 * the neighbour is sampled there (F.grid_sample, border padding, align_corners; trainer :853-857) and compared with the frame by
 * 0.85 SSIM + 0.15 L1 (trainer :899-911, utils/layers.py:276-306), plus disparity_smoothness / 2^s times the edge-aware smoothness
 * of the mean-normalised map (utils/layers.py:222-236, trainer :944-946); mean over the four scales (trainer :968).  The pose
 * network's outputs are inputs here: K, invK, Tprev, Tnext are [B*T, 4, 4] row-major (Tprev / Tnext: pose from frame i to frames
 * i-1 / i+1; the first / last frame of a clip has no such neighbour and is left out of that term).  frames [B*T, 3, H, W] in [0, 1];
 * disp_dev[s] [B*T, 1, disp_h[s], disp_w[s]]; loss_dev receives ONE float; grad_disp_dev[s] receives dL/d disp_dev[s] (same shape).
 * Deterministic (gathers and fixed-order two-stage sums, no float atomics).  T >= 2, H, W >= 3. */
size_t edv_photometric_loss_workspace(int32_t B, int32_t T, int32_t H, int32_t W); /* bytes */
int edv_photometric_loss(const float *frames_dev, const float *const disp_dev[4], const int32_t disp_h[4], const int32_t disp_w[4], int32_t B, int32_t T, int32_t H,
                         int32_t W, const float *K_dev, const float *invK_dev, const float *Tprev_dev, const float *Tnext_dev, float min_depth, float max_depth,
                         float disparity_smoothness, float *loss_dev, float *const grad_disp_dev[4], float *workspace_dev, size_t workspace_bytes, void *stream);

/* ---- the trainer's whole loss (round 3): generate_images_pred + compute_losses of trainer_end_to_end_video.py:808-971 with the side networks'
 * outputs as inputs, and every gradient the reference's autograd reaches.  N = B*T flattened frames (trainer :406-409), frame size H x W.
 *   color[s]            inputs[("color", 0, s)]            [N, 3, H >> s, W >> s]   (s = 0: the frame)
 *   color_nb[0 / 1]     inputs[("color", -1 / +1, 0)]      [N, 3, H, W]
 *   K, invK             [N, 4, 4] row-major (inputs[("K", 0)] or, with learn_intrinsics, outputs[("K", 0)]);  T[0 / 1] = outputs[("cam_T_cam", 0, -1 / +1)]
 *   refined[s][n], registration[s][n], transform[s][n] = outputs[("refined" | "registration", s, fid)], outputs[("transform", "high", s, fid)]   [N, 3, H, W]
 *   mask[n]             outputs[("occu_mask_backward", 0, fid)]   [N, 1, H, W];   position[s][n] = outputs[("position", "high", s, fid)] [N, 2, H, W]
 *                       (position may be NULL when depth_flow is 0 or tune_temporal is off)
 *   disp[s]             outputs[("disp", s)]   [N, 1, disp_h[s], disp_w[s]]
 * losses_dev receives 29 floats: for s = 0..3 {loss/s, loss_reprojection, loss_transform, loss_cvt, loss_smooth, loss_depth_reproj, loss_depth_flow}
 * (the trainer's per-scale entries, :960-966), then losses["loss"] (:968).  Gradients of losses["loss"]: grads->disp[s] are required; refined /
 * transform / K / invK / T are optional (NULL = not wanted); registration and the mask are detached in the reference.  Deterministic except for the
 * gradient the two depth-consistency terms scatter into the sampled depth map (float atomics, as ATen's grid_sampler backward); with the options'
 * defaults (depth_reproj = depth_flow = 0) no atomic runs.  H, W >= 16. */
typedef struct {
    const float *color[4];
    const float *color_nb[2];
    const float *K, *invK;
    const float *T[2];
    const float *refined[4][2], *registration[4][2], *transform[4][2];
    const float *mask[2];
    const float *position[4][2];
    const float *disp[4];
    int32_t disp_h[4], disp_w[4];
} edv_trainer_loss_inputs;
typedef struct {
    float disparity_smoothness, transform_constraint, transform_smoothness, depth_reproj, depth_flow; /* options.py:136-159 */
    int32_t tune_temporal;                                                                              /* trainer :951 temporal_weight */
    float min_depth, max_depth;
} edv_trainer_loss_weights;
typedef struct {
    float *disp[4];
    float *refined[4][2], *transform[4][2];
    float *K, *invK, *T[2];
} edv_trainer_loss_grads;
size_t edv_trainer_loss_workspace(int32_t N, int32_t H, int32_t W); /* bytes */
int edv_trainer_loss(const edv_trainer_loss_inputs *in, int32_t N, int32_t H, int32_t W, const edv_trainer_loss_weights *weights, float *losses_dev,
                     const edv_trainer_loss_grads *grads, float *workspace_dev, size_t workspace_bytes, void *stream);

/* ---- backward kernels (input gradients of the frozen operators, gradients of the LoRA factors): input gradients of the frozen operators and the gradients of the
 * LoRA factors, the only trainable tensors (endodav/layers.py:5-34).  Same layouts as the forward kernels. ---- */
/* LayerNorm (no affine gradient): dx (+)= dLN(x; w, eps)(dy);  rows x dim, dim % 4 == 0, dim <= 1024. */
int edv_layernorm_bwd(const float *x_dev, const float *w_dev, const float *dy_dev, float *dx_dev, int64_t rows, int32_t dim, float eps,
                      int32_t accumulate, void *stream);
/* out = f(d) + (add ? add : 0); mode 0: f = d; 1: d * gelu'(src) (exact erf form); 2: src > 0 ? d : 0.  n % 4 == 0. */
int edv_ew_bwd(const float *d_dev, const float *src_dev, const float *add_dev, float *out_dev, int64_t n, int32_t mode, void *stream);
/* GEGLU (attention.py:363-384): x [M, 2*inner] = [a | g], y = a * gelu(g); dx from dy [M, inner]. */
int edv_geglu_bwd(const float *x_dev, const float *dy_dev, float *dx_dev, int64_t M, int32_t inner, void *stream);
/* Wt[k, n] = W[n, k] * gamma[n] (gamma may be NULL): the NT-form weight of dX = (dY * gamma) W. */
int edv_transpose_scale(const float *W_dev, const float *gamma_dev, float *Wt_dev, int32_t N, int32_t K, void *stream);
/* LoRA / DV-LoRA factor gradients of y = gamma * (x (W + s (B*V)(A*U))^T + b) from x [M, nin] and G = dL/dy [M, nout]
 * (mylora/layers.py:148-157, 384-393): A [r, nin], B [nout, r], U [r, 1], V [nout, 1].  U/V NULL = plain LoRA; gamma may be
 * NULL; any output may be NULL.  r in {1,2,4,8}. */
size_t edv_lora_grads_workspace(int64_t M, int32_t nin, int32_t nout, int32_t r); /* bytes */
int edv_lora_grads(const float *x_dev, const float *g_dev, int64_t M, int32_t nin, int32_t nout, int32_t r, const float *A_dev, const float *B_dev,
                   const float *U_dev, const float *V_dev, float s, const float *gamma_dev, float *workspace_dev, size_t workspace_bytes, float *dA_dev,
                   float *dB_dev, float *dU_dev, float *dV_dev, void *stream);
/* bilinear align_corners=True, input gradient: dy [F,oh,ow,C] -> dx [F,ih,iw,C] (deterministic gather). */
int edv_bilinear_bwd(const float *dy_dev, float *dx_dev, int32_t F, int32_t ih, int32_t iw, int32_t C, int32_t oh, int32_t ow, int32_t accumulate,
                     void *stream);
/* final 1x1 conv to one channel + output activation on a post-ReLU input (dpt.py:121-123; endodav/layers.py:206-221 with the sigmoid
 * of dpt_pyramid.py:103-109):  gz[p] = dL/dz;  mode 0 (ReLU): disp > 0 ? g : 0;  mode 1 / 2 (sigmoid(z) / sigmoid(-z)): +-g disp (1 - disp);
 * d_o2[p,c] = gz[p] * w[c] * (o2[p,c] > 0).  gz_out_dev (optional, [npix]) keeps gz for the 1x1 conv's own weight / bias gradient. */
int edv_dot_channels_bwd(const float *g_dev, const float *disp_dev, const float *w_dev, const float *o2_dev, float *d_o2_dev, float *gz_out_dev,
                         int64_t npix, int32_t C, int32_t mode, void *stream);
/* Weight gradient of a 3x3 / stride 1 / padding 1 convolution (the trainable convolutions of the output heads, endodav/layers.py:5-34):
 * x [F,H,W,Cin] channels-last, dy [F,H,W,Cout] -> dw [Cout,Cin,3,3] (torch layout).   Deterministic (two stages). */
size_t edv_conv3x3_wgrad_workspace(int32_t F, int32_t H, int32_t W, int32_t Cin, int32_t Cout); /* bytes */
int edv_conv3x3_wgrad(const float *x_dev, const float *dy_dev, float *dw_dev, int32_t F, int32_t H, int32_t W, int32_t Cin, int32_t Cout,
                      float *workspace_dev, size_t workspace_bytes, int32_t accumulate, void *stream);
/* out[n] (+)= sum_m rowscale[m] * P[m,n] (rowscale may be NULL): bias gradients, and the 1x1 head's weight gradient with rowscale = gz.
 * N a power of two in 4..1024, or 1 (then M % 4 == 0 and no rowscale). */
size_t edv_colsum_workspace(int32_t N); /* bytes */
int edv_colsum_rows(const float *P_dev, const float *rowscale_dev, int64_t M, int32_t N, float *workspace_dev, size_t workspace_bytes, float *out_dev,
                    int32_t accumulate, void *stream);
/* Batched column sums (the bias gradients of bias="all"): for job k, dst[k][n] (+)= scale[k][n] * sum_m P_k[map_k(m), n] over rows[k] rows,
 * P_k = src[k] with leading dimension ld[k], n < cols[k] (any cols >= 1).  row_map (optional) = n triples (period, stride, offset): row m
 * reads physical row (m / period) * stride + offset + m % period (period 0 = identity).  scale (optional, entries may be NULL) and
 * accumulate (optional) per job.  Two launches for all jobs, fixed summation order (bit-reproducible), no atomics. */
size_t edv_colsum_batch_workspace(int32_t n, const int64_t *rows, const int32_t *cols); /* bytes */
int edv_colsum_batch(int32_t n, const float *const *src_dev, const int64_t *ld, const int64_t *rows, const int32_t *row_map, const int32_t *cols,
                     const float *const *scale_dev, float *const *dst_dev, const int32_t *accumulate, float *workspace_dev, size_t workspace_bytes, void *stream);
/* GroupNorm input gradient; stats = the forward's [F, groups, 2] (mean, rstd); sums = [F, groups, 2] scratch. */
int edv_groupnorm_bwd(const float *x_dev, const float *stats_dev, const float *w_dev, const float *dy_dev, float *sums_dev, float *dx_dev, int32_t F,
                      int32_t P, int32_t C, int32_t groups, int32_t accumulate, void *stream);
/* temporal attention core, backward: dqkv [B*T*P, 3C] from qkv and dout [B*T*P, C]. */
int edv_attn_temporal_bwd(const float *qkv_dev, const float *dout_dev, float *dqkv_dev, int32_t B, int32_t T, int32_t P, int32_t C, int32_t heads,
                          void *stream);
/* 3x3 convolution input gradient.  Stride 1: run edv_conv3x3 on dy with the weight repacked by edv_pack_conv3x3_bwd
 * ([Cout,Cin,3,3] -> [Cin][3][3][Cout], taps flipped).  Stride 2: direct kernel on the forward's packed weight. */
int edv_pack_conv3x3_bwd(const float *w_dev, float *wpacked_dev, int32_t Cout, int32_t Cin, void *stream);
int edv_conv3x3_s2_bwd(const float *dy_dev, const float *wpacked_dev, float *dx_dev, int32_t F, int32_t H, int32_t W, int32_t Cin, int32_t Cout,
                       void *stream);
/* The engine's form of the stride-2 input gradient: z [F,H,W,C] = dy [F,OH,OW,C] with zeros inserted (z[2oy,2ox] = dy[oy,ox]),
 * then the stride-1 recipe above on z. */
int edv_dilate2(const float *dy_dev, float *z_dev, int32_t F, int32_t H, int32_t W, int32_t C, void *stream);
/* ConvTranspose(k = s) input gradient = edv_gemm of the pixel-unshuffled dy [F*h*w, s*s*C] with the transposed packed weight. */
int edv_pixel_unshuffle(const float *dy_dev, float *A_dev, int32_t F, int32_t h, int32_t w, int32_t C, int32_t s, void *stream);

/* ---- test entry points (ABI 13): the operator forms only the engine used to reach.  No reference counterpart. ----
 * A row map is int32_t[4] = (period, stride, offset, inner): logical row m lives at physical row
 *   (m / period) * stride + offset + inner * (m % period);   period 0 (or a NULL map pointer) = identity.
 * stride 0 broadcasts one block over the frames, inner 0 one row per frame over that frame's rows. */
typedef struct edv_gemm_desc_t {
    const float *A;            /* [rows, lda], logical row m read at a_map(m) */
    int32_t lda;
    int32_t a_map[4];
    const float *W;            /* [N, ldw] (torch Linear layout); may point into a wider matrix */
    int32_t ldw;
    float *C;                  /* logical row m stored at c_map(m), columns 0..N-1 of a row of ldc floats */
    int32_t ldc;
    int32_t c_map[4];
    int64_t M;
    int32_t N, K;
    const float *bias;         /* [N] or NULL */
    int32_t act;               /* 0 none, 1 GELU, 2 ReLU */
    const float *gamma;        /* [N] or NULL */
    const float *R1;           /* residual read at r1_map(m), or NULL; may alias C */
    int32_t ldr1;
    int32_t r1_map[4];
    const float *R2;           /* second residual, read at the OUTPUT row c_map(m), or NULL */
    int32_t ldr2;
    const float *P1;           /* pre-activation addend read at p1_map(m), or NULL */
    int32_t ldp1;
    int32_t p1_map[4];
    float *workspace;          /* stream-K workspace (edv_gemm_workspace bytes) or NULL: plain grid */
    size_t workspace_bytes;
    const void *x6_planes;     /* bf16 planes of W (edv_gemm_x6_split) or NULL; used only where the bf16x6 kernel supports the descriptor */
} edv_gemm_desc_t;
/* C = epilogue(A W^T) through the same dispatcher the engine calls, dense loader and row store:
 *   v = acc + bias[n] + P1[p1_map(m), n];  v = act(v) * gamma[n];  v += R1[r1_map(m), n] + R2[c_map(m), n].
 * Refuses ldc / ldr1 / ldr2 / ldp1 < N, a map with period < 0, stride < 0, offset < 0 or inner outside {0, 1}, act outside 0..2. */
int edv_gemm_desc(const edv_gemm_desc_t *d, void *stream);
/* edv_layernorm with row maps (NULL = identity), an output activation (0 none, 1 GELU) and y += instead of y =. */
int edv_layernorm_mapped(const float *x_dev, const int32_t *in_map, const float *w_dev, const float *b_dev, float *y_dev, const int32_t *out_map,
                         int64_t rows, int32_t dim, float eps, const float *pe_dev, int32_t rows_per_frame, int32_t T, int32_t act, int32_t accumulate,
                         void *stream);
/* edv_layernorm_bwd with row maps on x, dy and dx (NULL = identity). */
int edv_layernorm_bwd_mapped(const float *x_dev, const int32_t *x_map, const float *w_dev, const float *dy_dev, const int32_t *dy_map, float *dx_dev,
                             const int32_t *dx_map, int64_t rows, int32_t dim, float eps, int32_t accumulate, void *stream);
/* Linear_SSB fold: out[n, k] = a[k] * W[n, k] * b[n]. */
int edv_fold_ssb(const float *W_dev, const float *a_dev, const float *b_dev, float *out_dev, int32_t nout, int32_t nin, void *stream);
/* Eval-mode BatchNorm folded into the preceding convolution, in place: w[n, :] *= s[n], bout[n] = (b[n] - mean[n]) * s[n] + beta[n],
 * s = gamma / sqrt(var + eps). */
int edv_fold_bn(float *w_dev, const float *b_dev, const float *gamma_dev, const float *beta_dev, const float *mean_dev, const float *var_dev, float eps,
                float *bout_dev, int32_t nout, int32_t K, void *stream);
/* DashLinear after warm-up, in place: inout += Utop [nout, r] diag(idx [r]) Vtop [r, nin]. */
int edv_fold_dash(const float *Utop_dev, const float *idx_dev, const float *Vtop_dev, float *inout_dev, int32_t nout, int32_t nin, int32_t r, void *stream);
/* out[n] = scale[n] * sum_m P[m, n] * Q[m, n]  (Q NULL: column sums of P; scale NULL: 1); part_dev: 64 * N floats of scratch.
 * Fixed summation order: bit-reproducible. */
int edv_col_dot(const float *P_dev, const float *Q_dev, int64_t M, int32_t N, const float *scale_dev, float *part_dev, float *out_dev, void *stream);
/* Linear_SSB backward preparation: Wa[n, k] = W[n, k] * a[k], gb[n] = b[n] * gamma[n] (gamma NULL: 1). */
int edv_ssb_prep(const float *W_dev, const float *a_dev, const float *b_dev, const float *gamma_dev, float *Wa_dev, float *gb_dev, int32_t nout,
                 int32_t nin, void *stream);
/* out = g * s * (1 - s), s = the sigmoid's output; any n. */
int edv_sigmoid_bwd(const float *g_dev, const float *s_dev, float *out_dev, int64_t n, void *stream);
/* edv_bilinear plus an addend shaped like the output (C % 4 == 0): y = up(x) + add. */
int edv_bilinear_add(const float *x_dev, const float *add_dev, float *y_dev, int32_t F, int32_t H, int32_t W, int32_t C, int32_t OH, int32_t OW,
                     void *stream);

/* ---- test entry point (ABI 15): the host planner of the persistent stream-K grids, with `slots` (resident workgroups) given instead of
 * queried.  Touches no device.  kind: 0 LDS-DMA GEMM, 1 bf16x6 GEMM, 2 3x3 convolution (tiles of k_tiles k-tiles), 3 spatial attention
 * forward / backward (tasks of k_tiles key tiles).  It runs the launch path's own policy (environment knobs included) as for a launch with
 * a workspace.  out = { 1 split / 0 plain, grid, whole_rounds, chunk, nsplit, stride (kind 3: leftover tasks), units,
 * workspace floats the plan needs (kinds 0-2; kind 3: pieces, to be multiplied by the caller's rows x columns) }.
 * Added later (additive): kind 4, the bf16x6 GEMM's remainder plan as edv_gemm_x6 would decide it.  slots = CUs; ON ENTRY out[0] = resident
 * workgroups per CU and out[1] = the mode of edv_set_x6_remainder (1 or 2).  out = { 1 remainder plan / 0 another plan (then all zero), grid,
 * first split tile = whole tiles, chunk, nsplit, split tiles, units, workspace floats }.  kind 5: the whole tile that raw block index
 * tiles_or_tasks computes in a remainder grid of `slots` workgroups whose first k_tiles own runs; out[0] = the tile. */
int edv_split_plan(int32_t kind, int64_t tiles_or_tasks, int32_t slots, int32_t k_tiles, int64_t out[8]);

/* Additive: process-wide switch of the bf16x6 GEMM's remainder plan, read at every edv_gemm_x6 / engine launch.  A plain grid that ends a few
 * tiles past a whole number of rounds of CUs splits only those tiles along k and starts their pieces first.  mode 0 = off, 1 = by policy (the
 * default: at most CUs / 16 tiles past a round, and the whole grid resident at once), 2 = wherever the walk is supported (tests, A/B runs).
 * cus > 0 plans for that many CUs instead of the device's (tests: ten-tile problems take the path at cus = 8); 0, or more than the device
 * has, = the device's count.  Tiles that are not split keep their bits in every mode. */
int edv_set_x6_remainder(int32_t mode, int32_t cus);

#ifdef __cplusplus
}
#endif
#endif /* ENDODAV_HIP_H */
