/*
 * sat_hip.h -- C ABI of libsat_hip.so: the MI355X (gfx950) implementation of the
 * diffusion-sampling hot path of stable-audio-tools (DiT denoiser + DPM-Solver++ update +
 * Oobleck VAE encode/decode).
 *
 * The reference (yukara-ikemiya/friendly-stable-audio-tools) is pure Python on stock
 * PyTorch ops and has NO FFI / plugin boundary of its own: the
 * boundary it exposes is its Python API.  This header is what a Python (ctypes), C++ or
 * any-other-language host binds *underneath* that API.  Each entry point names the
 * reference interface it replaces (paths relative to stable_audio_tools/ in the reference).
 *
 * Conventions
 *   - return 0 on success; negative SAT_E_* on invalid argument / unsupported config;
 *     positive = hipError_t of a failed HIP call.  Never throws, never exits.
 *     sat_last_error() gives a thread-local message for the last non-zero return.
 *   - all pointers named *_dev are DEVICE pointers owned by the caller (e.g. PyTorch
 *     storage); tensors are dense, row-major ("PyTorch contiguous"), fp32 unless noted.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).  All compute
 *     calls are asynchronous on that stream; no call synchronises the device.
 *   - no allocation on the hot calls (forward / denoise / step / decode / encode): the
 *     caller supplies the workspace; plans own only re-packed (bf16) weights and the
 *     per-generation cross-attention K/V cache (allocated in *_prepare_context).
 *   - a plan is not thread-safe; distinct plans are independent.  One process per GPU.
 */
#ifndef SAT_HIP_H
#define SAT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* The library is built with -fvisibility=hidden: exactly the functions declared in this header are exported (tests/test_cabi.py). */
#pragma GCC visibility push(default)

#define SAT_OK 0
#define SAT_E_INVALID (-1)      /* bad argument (NULL, shape, size) */
#define SAT_E_UNSUPPORTED (-2)  /* configuration outside the kernels' supported set */
#define SAT_E_MISSING (-3)      /* a required tensor was never set */
#define SAT_E_WORKSPACE (-4)    /* workspace too small */
#define SAT_E_STATE (-5)        /* call order violated (e.g. forward before finalize) */

typedef void* sat_stream_t;     /* hipStream_t */

/* ABI version: 6.  A loader MUST check it (stable_audio_tools/_hip.py does): the cfg structs grow at the END between versions.  Since version 6
 * the size of the caller's sat_dit_cfg travels with the call (sat_dit_plan_create_sized), so a struct laid out for another version is rejected
 * deterministically instead of being read past its end; sat_dit_plan_create keeps reading exactly the version-5 layout (14 int32 fields). */
int sat_version(void);
const char* sat_last_error(void);

/* ------------------------------------------------------------------------------------
 * DiT denoiser.  Replaces models/dit.py:135-364 (DiffusionTransformer._forward/.forward),
 * models/transformer.py:99-809 (ContinuousTransformer, TransformerBlock, Attention,
 * FeedForward, LayerNorm, RotaryEmbedding), models/diffusion.py:482-529 (DiTWrapper).
 * Supported set: transformer_type "continuous_transformer", global_cond_type "prepend"
 * or "adaLN", dim_heads 64 or 128, patch_size 1 or, through sat_dit_plan_set_patch, above,
 * non-causal or, through sat_dit_plan_set_attention_options, causal self-attention without cross-attention, or, through
 * sat_dit_plan_set_neighborhood_attention, NATTEN's 1-D neighbourhood (natten_kernel_size; no cross-attention; sat_dit_plan_set_neighborhood_attention_hdw off 64-channel heads), no masks (the reference discards
 * them at inference: models/dit.py:250-252; prepend_cond_mask never reaches the layers,
 * models/transformer.py:787-802).  Input-concat and prepend conditioning (dit.py:160-197)
 * through sat_dit_plan_set_extra_conditioning / sat_dit_prepare_extra_conditioning; prepend
 * conditioning with "adaLN" is rejected (the reference returns P + T frames there).
 * qk_norm, the sinusoidal / absolute position embeddings and rotary_pos_emb=False through
 * sat_dit_plan_set_transformer_options; a feed-forward without output bias by leaving the tensor out.
 * ---------------------------------------------------------------------------------- */
typedef struct sat_dit_plan sat_dit_plan;

#define SAT_GEMM_BF16 0
#define SAT_GEMM_FP8 1
#define SAT_GEMM_FP32X 2
#define SAT_GEMM_FP16 3
/* sat_dit_cfg.fp8_families */
#define SAT_FP8_QKV 1       /* self-attention to_qkv   (transformer.py:314), LayerNorm-fed: one scale per token */
#define SAT_FP8_CROSS_Q 2   /* cross-attention to_q    (transformer.py:311), LayerNorm-fed */
#define SAT_FP8_FF_IN 4     /* FF-in (SwiGLU)          (transformer.py:222), LayerNorm-fed */
#define SAT_FP8_FF_OUT 8    /* FF-out                  (transformer.py:270), MXFP8 A operand from the FF-in epilogue */
#define SAT_FP8_TO_OUT 16   /* to_out, self and cross  (transformer.py:319), MXFP8 A operand from the attention kernels */
#define SAT_FP8_ALL 31
#define SAT_FP8_DEFAULT (SAT_FP8_CROSS_Q | SAT_FP8_FF_IN | SAT_FP8_FF_OUT)

typedef struct sat_dit_cfg {
    int32_t io_channels;       /* config "io_channels" (64) */
    int32_t embed_dim;         /* "embed_dim" (1536); multiple of 128 */
    int32_t depth;             /* "depth" (24) */
    int32_t num_heads;         /* "num_heads" (24); embed_dim / num_heads must be 64, or 128 = the staged attention route: bf16 / fp16
                                  operands only, no LayerNorm fold, no fused cross-attention launch */
    int32_t cond_token_dim;    /* "cond_token_dim" (768); 0 = no cross-attention */
    int32_t cond_embed_dim;    /* cond_token_dim if project_cond_tokens=false else embed_dim */
    int32_t global_cond_dim;   /* "global_cond_dim" (1536); 0 = timestep embedding only */
    int32_t max_seq_len;       /* largest latent length T the plan will see (+1 prepend) */
    int32_t adaln;             /* 0: "global_cond_type": "prepend" (models/dit.py:186-197, the shipped configs);
                                  1: "adaLN" (models/dit.py:205-206, models/transformer.py:665-689): no prepend token, the
                                  global embedding drives per-layer scale/shift/gate of the self-attention and FF branches;
                                  needs "transformer.layers.N.to_scale_shift_gate.1.weight" [6*embed_dim, embed_dim] */
    int32_t gemm_dtype;        /* operand format of the block GEMMs and the attention kernels (fp32 accumulation throughout):
                                  0 (SAT_GEMM_BF16): bf16 operands everywhere (the C default of a zeroed struct; 3-4 % faster than fp16, 8x its operand rounding);
                                  3 (SAT_GEMM_FP16): IEEE fp16 operands everywhere (what the Python package selects by default and bench.py measures) -- the same
                                  kernels built on v_mfma_f32_*_f16, which
                                  gfx950 issues at the bf16 rate; three more significand bits (8x less operand rounding), and what the
                                  reference computes in on a GPU (inference/sampling.py:210 autocast, transformer.py:496-504).  Range
                                  policy: every fp32 -> fp16 conversion SATURATES at +-65504 (MODE.FP16_OVFL); values below 6e-8 flush;
                                  1 (SAT_GEMM_FP8): BASELINE config 5 -- the GEMMs fed by a LayerNorm (self-attention to_qkv, cross-attention
                                  to_q, FF-in; transformer.py:314, 311, 222) take OCP e4m3 operands with one scale per token
                                  (activations) and per output channel (weights), fp32 accumulation; FF-out (transformer.py:270)
                                  takes the SwiGLU output as MXFP8 (e4m3 + one E8M0 scale per 32 hidden channels, written by the
                                  FF-in epilogue, consumed as hardware block scales) and e4m3 weights; the attention kernels write
                                  MXFP8 too (one scale per half head) for the to_out projections (transformer.py:319); rest as 0;
                                  2 (SAT_GEMM_FP32X): fp32 VERIFICATION mode -- every contraction of the blocks on the exact fp32 MFMA
                                  (v_mfma_f32_32x32x2_f32), fp32 LayerNorm output, fp32 q / k / v / P, fp32 weights: same plan, data flow
                                  and index arithmetic, no operand rounding (~20x slower; meets 1e-3 vs the reference's outputs) */
    int32_t fp8_families;      /* gemm_dtype == 1 only: which GEMM families take e4m3 operands, an OR of SAT_FP8_* (0 = SAT_FP8_DEFAULT).  The
                                  full-size 12-step CFG-7 trajectory (tests/golden/traj_full.npz; tools/fp8_budget.py) prices each family's
                                  quantisation separately (rel-L2 vs fp32 after 12 steps; bf16 everywhere: 8e-3): the to_out projections
                                  on MXFP8 attention outputs 3.3e-1 -- that one family was round 3's whole fidelity problem --, to_qkv 6e-2
                                  (attention scores under CFG 7 do not tolerate 3-bit mantissas), cross to_q 1.2e-2, FF-in 9.5e-3, FF-out
                                  1.3e-2.  The default therefore quantises cross to_q, FF-in and FF-out (56 % of the block's FLOPs) and keeps
                                  to_qkv / to_out in bf16; SAT_FP8_ALL is round 3's mode.  SAT_FP8_FF_OUT needs SAT_FP8_FF_IN (the
                                  MXFP8 hidden state is written by the e4m3 FF-in epilogue) */
    int32_t ln_fold;           /* 1 (gemm_dtype 0 or 3, adaln == 0, embed_dim >= 256; ignored otherwise): no standalone LayerNorm launches
                                  after the first one.  LN(x) W^T = rstd (x (gamma.W)^T - mean rowsum(gamma.W)) + beta W^T: the GEMM
                                  that updates the residual stream (to_out, FF-out; transformer.py:692-700) also writes bf16(x) and
                                  per-row partial sums, the GEMM behind the LayerNorm (to_qkv, to_q, FF-in) multiplies bf16(x) with
                                  bf16(gamma.W) and finishes the normalisation on its fp32 accumulators.  Same arithmetic up to WHERE
                                  the one bf16 rounding of the activation happens (before instead of after the normalisation);
                                  0: three LayerNorm kernels per block */
    /* ---- version 5: the two A/B switches that used to be process-wide setters (sat_set_cross_attention_fusion, sat_gemm_set_wide_tile) are
     * per plan -- "distinct plans are independent" now also holds for them.  Appended at the END of the struct; sat_version() == 5. */
    int32_t cross_attention;   /* 0 (default): to_q projection + cross-attention core in ONE launch where the projection's 128 x 64 tiles fit one
                                  round of workgroups (one prompt; transformer.py:430-437 + 496-536), two kernels otherwise; 1: always two kernels */
    int32_t tile_policy;       /* 0 / 80 (default): the measured tile choice; A/B measurement switches: 22 = the 16-wave 256 x 256 tile of rounds
                                  1-2 instead of the 8-phase kernel, 81 = the 8-phase kernel also for fp32-output GEMMs with K < 4096, 82 = no
                                  two-K-group 128 x 128 tile.  The heads GEMMs of a qk_norm plan (sat_dit_plan_set_transformer_options) always run
                                  under 22 whatever stands here: their normalising epilogue exists in the ring tiles only (81 / 82 concern the
                                  fp32-output GEMMs and keep their meaning there) */
} sat_dit_cfg;
#define SAT_DIT_CFG_BYTES_V5 56          /* the layout sat_dit_plan_create reads: 14 int32 fields, up to and including tile_policy */

/* cfg_bytes = sizeof(sat_dit_cfg) of the header the CALLER was built against.  This version knows one layout (SAT_DIT_CFG_BYTES_V5: the version-5
 * layout, unchanged in version 6); any other size is SAT_E_INVALID -- a caller built against another header is told so instead of having its struct
 * read past its end.  When the struct grows again, the older sizes stay accepted and the new fields take their defaults.
 * sat_dit_plan_create(cfg, out) == sat_dit_plan_create_sized(cfg, SAT_DIT_CFG_BYTES_V5, out). */
int sat_dit_plan_create_sized(const sat_dit_cfg* cfg, size_t cfg_bytes, sat_dit_plan** out_plan);
int sat_dit_plan_create(const sat_dit_cfg* cfg, sat_dit_plan** out_plan);
/* Creation options that are not part of sat_dit_cfg (whose layout and size stay what version 5 fixed), following sat_oobleck_plan_create_ex.
 * head_widths: which attention head widths embed_dim / num_heads the plan admits.  0: 64 and 128 only -- exactly sat_dit_plan_create_sized;
 * 1: 32 and 96 as well.  A plan with 32- or 96-channel heads runs the staged route of the 128-channel heads (fp32-output projection, head
 * split, attention kernel: DESIGN.md section 7) with bf16 / fp16 operands (gemm_dtype 0 / 3, per block with sat_dit_plan_set_block_formats)
 * and, unlike 128, the fp32 verification mode (gemm_dtype 2); e4m3 (gemm_dtype 1), sat_dit_plan_set_block_options with an option on and
 * sat_dit_plan_set_ff_conv above kernel size 1 answer SAT_E_UNSUPPORTED with "dim_heads" in the message, any other width likewise.
 * options == NULL (options_bytes ignored) behaves as sat_dit_plan_create_sized; otherwise options_bytes must be sizeof(sat_dit_create_options)
 * of this version and head_widths 0 or 1 (SAT_E_INVALID). */
typedef struct {
    int32_t head_widths;
} sat_dit_create_options;
int sat_dit_plan_create_ex(const sat_dit_cfg* cfg, size_t cfg_bytes, const sat_dit_create_options* options, size_t options_bytes,
                           sat_dit_plan** out_plan);
void sat_dit_plan_destroy(sat_dit_plan* plan);

/* Hand one fp32 tensor of the reference state dict to the plan.  `name` is the key
 * RELATIVE to the DiffusionTransformer module ("model.model." stripped), e.g.
 * "transformer.layers.3.ff.ff.0.proj.weight" (models/dit.py, models/transformer.py module
 * tree).
 *
 * Lifetime rule of all four plan kinds (sat_dit_*, sat_oobleck_*, sat_t5_*, sat_roberta_*): *_plan_set_tensor only records
 * the pointer (setting a name again replaces it); the memory is read inside *_plan_finalize and nowhere else.
 * *_plan_finalize copies / re-packs everything into device memory the plan owns and synchronises `stream` before it
 * returns: after a successful finalize the caller may free or overwrite its fp32 tensors at once.  A finalize that fails
 * (SAT_E_MISSING, SAT_E_INVALID, a HIP error) leaves the plan unfinalized with its table intact: set what was missing and
 * finalize again, or destroy the plan. */
int sat_dit_plan_set_tensor(sat_dit_plan* plan, const char* name, const float* data_dev, int64_t numel);

/* Input-concat / prepend conditioning (models/dit.py:38,160-173,185-197), between create and finalize; a plan never given
 * this call has neither (input_concat_dim = prepend_cond_dim = 0).  input_concat_dim (config "input_concat_dim", e.g. 65
 * for "diffusion_cond_inpaint"): preprocess_conv is (io + Cc) x (io + Cc) and project_in [D, io + Cc]; prepend_cond_dim:
 * the tensors "to_prepend_embed.0.weight" / ".2.weight" are required; max_prepend_len: the most prepend tokens any
 * generation will bring (the RoPE table and sat_dit_workspace_bytes grow by it).  prepend_cond_dim and max_prepend_len
 * are both positive or both 0.  SAT_E_STATE after finalize, SAT_E_INVALID for negative values.  SAT_E_UNSUPPORTED for
 * prepend conditioning on an "adaLN" plan, and for two limits of this build that the reference does not have:
 * prepend_cond_dim must be a multiple of 4 (the prepend MLP's vector loads), and io_channels + input_concat_dim must be
 * at most 256. */
int sat_dit_plan_set_extra_conditioning(sat_dit_plan* plan, int32_t input_concat_dim, int32_t prepend_cond_dim,
                                        int32_t max_prepend_len);

/* ContinuousTransformer switches beyond the shipped configs (models/transformer.py:298,433-436 qk_norm; :50-96,740-746,796-797
 * use_sinusoidal_emb / use_abs_pos_emb; :737 rotary_pos_emb), between create and finalize; a plan never given this call has
 * {0, SAT_DIT_POS_NONE, 0, 1} and builds and launches exactly what it did before this call existed.
 *   qk_norm 1: q and k of the self-attention and of the cross-attention are L2-normalised per head over the 64 channels,
 *     x / max(|x|, 1e-12), on the fp32 accumulators of their projection (before the rotation and the 1/sqrt(64) scale; one
 *     16-bit rounding); the cross-attention keys once per generation in sat_dit_prepare_context.  gemm_dtype SAT_GEMM_FP8
 *     with qk_norm is SAT_E_UNSUPPORTED.
 *   pos_emb SAT_DIT_POS_SINUSOIDAL: cat(sin, cos)(pos * 10000^(-j / (D/2))) * scale is added to every row of the stream behind
 *     project_in and the prepend concat (position 0 = the first prepended row); needs "transformer.pos_emb.scale" [1].
 *     SAT_DIT_POS_ABSOLUTE: emb.weight[pos] * D^-0.5, needs "transformer.pos_emb.emb.weight" [abs_pos_max_len, D]; a forward
 *     whose sequence (prepend rows + global token + t_len) is longer than abs_pos_max_len fails with SAT_E_INVALID before
 *     any launch (the reference asserts).  The table is built once in finalize; one small launch per forward adds it.
 *   rotary 0: no "transformer.rotary_pos_emb.inv_freq" tensor, q / k are not rotated.
 * options_bytes = sizeof(sat_dit_transformer_options) of the caller's header; any other size is SAT_E_INVALID, a value outside the
 * ones above SAT_E_UNSUPPORTED, a call after finalize SAT_E_STATE.
 * Independent of this call, a state dict without "transformer.layers.N.ff.ff.2.bias" (ff_kwargs no_bias) runs FF-out without a bias. */
#define SAT_DIT_POS_NONE 0
#define SAT_DIT_POS_SINUSOIDAL 1
#define SAT_DIT_POS_ABSOLUTE 2
typedef struct sat_dit_transformer_options {
    int32_t qk_norm;           /* attn_kwargs {"qk_norm": true} */
    int32_t pos_emb;           /* SAT_DIT_POS_* */
    int32_t abs_pos_max_len;   /* "abs_pos_emb_max_length" (SAT_DIT_POS_ABSOLUTE only; ignored otherwise) */
    int32_t rotary;            /* "rotary_pos_emb" (1 in every shipped config) */
} sat_dit_transformer_options;
int sat_dit_plan_set_transformer_options(sat_dit_plan* plan, const sat_dit_transformer_options* options, size_t options_bytes);

/* TransformerBlock options beyond the shipped configs (models/transformer.py:557-591,645,680-681,697-698 conformer; :621,632,642
 * remove_norms; :259-268 ff_kwargs glu), between create and finalize; a plan never given this call has {0, 0, 1} and builds and launches
 * exactly what it did before this call existed.
 *   conformer 1: every block runs x += conformer(x) behind its cross-attention update (behind the self-attention update in a model without
 *     cross-attention) and in front of its feed-forward, on every sequence, not modulated by adaLN: in_norm + pointwise_conv (one
 *     LayerNorm-fed GEMM, 16-bit output), glu (Linear(D, 2D) + x * silu(gate), on that 16-bit output), the 17-tap depthwise_conv along the
 *     sequence [prepend rows | global token | frames] (zero-padded by 8 at both ends of each sequence) + mid_norm + SiLU in one pass,
 *     pointwise_conv_2 added to the fp32 stream.  Needs "transformer.layers.N.conformer.{in_norm,mid_norm}.{gamma,beta}" [D],
 *     ".pointwise_conv.weight" / ".pointwise_conv_2.weight" [D, D, 1], ".glu.proj.weight" [2D, D], ".glu.proj.bias" [2D] and
 *     ".depthwise_conv.weight" [D, 1, 17]; finalize names a missing one with SAT_E_MISSING.
 *   remove_norms 1: pre_norm, cross_attend_norm and ff_norm are the identity and have no tensors: to_qkv, the cross-attention to_q and the
 *     feed-forward read the residual row itself, rounded to the block's operand format -- under adaLN x * (1 + scale) + shift of the raw
 *     row.  The conformer's in_norm and mid_norm stay.  ln_fold changes nothing in the results of such a plan (the rounded row is then the
 *     image the previous residual epilogue wrote).
 *   ff_glu 0: ff.ff.0 is Linear(D, inner) + SiLU, tensors "transformer.layers.N.ff.ff.0.1.weight" [inner, D] and optionally ".0.1.bias"
 *     [inner] instead of ".0.proj.*"; inner must be a multiple of 128.  These FF-in GEMMs always run on the ring tiles (the 8-phase kernel
 *     has no plain-activation epilogue).
 * options_bytes = sizeof(sat_dit_block_options) of the caller's header; any other size is SAT_E_INVALID, a value outside 0 / 1
 * SAT_E_UNSUPPORTED, a call after finalize SAT_E_STATE.  SAT_E_UNSUPPORTED as well: any of the three options (conformer 1, remove_norms 1,
 * ff_glu 0) on a plan with gemm_dtype SAT_GEMM_FP8 or with 128-channel heads, and sat_dit_range_report on a plan with one of them.
 * A feed-forward built on a convolution (ff_kwargs use_conv) is a call of its own, sat_dit_plan_set_ff_conv below: this struct's size is
 * checked and does not grow. */
typedef struct sat_dit_block_options {
    int32_t conformer;      /* "conformer" */
    int32_t remove_norms;   /* "remove_norms" */
    int32_t ff_glu;         /* ff_kwargs "glu" (1 in every shipped config) */
} sat_dit_block_options;
int sat_dit_plan_set_block_options(sat_dit_plan* plan, const sat_dit_block_options* options, size_t options_bytes);

/* Convolutional feed-forward (ff_kwargs use_conv, models/transformer.py:211-287), between create and finalize; a plan never given this call
 * has kernel_size 1 (Linear) and builds and launches exactly what it did before this call existed.  With kernel_size k = 3, 5 or 7 the
 * output projection of every block's feed-forward is Conv1d(inner, D, k, padding = k / 2) along the sequence [prepend rows | global token |
 * frames]: tensors "transformer.layers.N.ff.ff.2.weight" [D, inner, k] and optionally ".ff.ff.2.bias" [D].  With ff_glu 0
 * (sat_dit_plan_set_block_options) the input projection is Conv1d(D, inner, k) + SiLU as well, "….ff.ff.0.1.weight" [inner, D, k] and
 * optionally ".0.1.bias" [inner]; under GLU it stays the Linear SwiGLU (the reference's GLU builds its own nn.Linear).  The window is
 * zero-padded by k / 2 at both ends of each sequence and never reaches into the neighbouring batch item.  Finalize packs each weight
 * tap-major into one [N, k * K] operand in the block's format (fp32 in the verification mode) and names a missing tensor with SAT_E_MISSING.
 * A convolution runs as one contraction of length k * K over k row-shifted reads of its dense A operand (16-bit MFMA, fp32 accumulation)
 * with the epilogue of the Linear it replaces: bias, adaLN gate and the add into the fp32 stream for FF-out, bias + SiLU and a 16-bit
 * output for FF-in.  The LayerNorm fold is off in such a plan (ln_fold is accepted without effect, as for adaLN).  The workspace grows in
 * the fp32 verification mode only, by the row gather in front of its GEMM.
 * options_bytes = sizeof(sat_dit_ff_conv_options) of the caller's header; any other size is SAT_E_INVALID, as is kernel_size < 1; a call
 * after finalize is SAT_E_STATE.  SAT_E_UNSUPPORTED: an even kernel_size (the reference's convolution then returns one row too many and its
 * own residual add fails), one above 7, and a kernel_size above 1 on a plan with gemm_dtype SAT_GEMM_FP8, with 128-channel heads or with
 * the range report on; sat_dit_range_report on such a plan likewise. */
typedef struct sat_dit_ff_conv_options {
    int32_t kernel_size;    /* ff_kwargs "conv_kernel_size" under "use_conv"; 1 = Linear */
} sat_dit_ff_conv_options;
int sat_dit_plan_set_ff_conv(sat_dit_plan* plan, const sat_dit_ff_conv_options* options, size_t options_bytes);

/* Patchified DiT (DiffusionTransformer patch_size, models/dit.py:38,88-89,119-120,197-224), between create and finalize; a plan never
 * given this call, or given patch_size 1, has a token per latent frame and builds and launches exactly what it did before this call existed.
 * With patch_size P >= 2 a token is P consecutive frames: "transformer.project_in.weight" is [D, (io_channels + input_concat_dim) * P] and
 * "transformer.project_out.weight" [io_channels * P, D], feature index c * P + p (channel-major, frame-minor: the reference's
 * "b (t p) c -> b t (c p)" and "b (c p) t -> b c (t p)"); "preprocess_conv.weight" and "postprocess_conv.weight" keep their per-frame
 * shapes and finalize folds them into the two projections inside each p.  Input-concat conditioning is resized to t_len FRAMES (nearest
 * source frame per frame, as at P = 1) before the patchify.  t_len stays in latent frames in sat_dit_workspace_bytes, sat_dit_forward,
 * sat_dit_denoise_cfg and against max_seq_len, and x / out keep their [bf, io_channels, t_len] layout; the sequence the blocks see is
 * [prepend rows | global token | t_len / P tokens], and the workspace, the rotary and position tables and abs_pos_max_len count those
 * rows.  A t_len that is not a multiple of P is SAT_E_INVALID in those three calls, before anything is launched (the reference fails
 * inside its rearrange).  Everything between the two projections is the P = 1 plan on fewer rows, in every gemm_dtype.
 * options_bytes = sizeof(sat_dit_patch_options) of the caller's header; any other size is SAT_E_INVALID, as is patch_size < 1 or one
 * above max_seq_len; a call after finalize is SAT_E_STATE.  SAT_E_UNSUPPORTED (the widths the two boundary kernels are built for, beside
 * io_channels <= 64, a multiple of 4, and io_channels + input_concat_dim <= 256 at P = 1): io_channels * P > 512, and
 * (io_channels + input_concat_dim) * P > 1024, checked by whichever of this call and sat_dit_plan_set_extra_conditioning comes second. */
typedef struct sat_dit_patch_options {
    int32_t patch_size;     /* "patch_size"; 1 = a token per frame */
} sat_dit_patch_options;
int sat_dit_plan_set_patch(sat_dit_plan* plan, const sat_dit_patch_options* options, size_t options_bytes);

/* Causal DiT (ContinuousTransformer causal, models/transformer.py:296,304,359-398 of the reference), between create and finalize; a plan
 * never given this call, or given causal 0, builds and launches exactly what it did before this call existed.  With causal 1 every
 * self-attention is causal over the sequence the blocks see, [prepend rows | global token | tokens]: row i attends to the rows j <= i of
 * its own sequence (what the reference computes through SDPA is_causal=True and through flash-attn with q_len == k_len).  The kernels walk
 * only the key tiles up to a workgroup's last query and compare per element only where the diagonal crosses a block of 32 keys.  No
 * tensor is added or renamed.  The convolutions of conformer and use_conv blocks stay non-causal, as in the reference.  Runs with
 * gemm_dtype bf16, fp16, per-block formats and the fp32 verification mode, at every head width the plan accepts.
 * options_bytes = sizeof(sat_dit_attention_options) of the caller's header; any other size is SAT_E_INVALID, as is a value outside 0 / 1; a
 * call after finalize is SAT_E_STATE.  SAT_E_UNSUPPORTED, with "causal" in the message: causal 1 on a plan with cross-attention
 * (cond_token_dim > 0: the reference fails with more context keys than queries and its backends disagree with fewer) or with gemm_dtype
 * SAT_GEMM_FP8 (the MXFP8 output form of the attention kernels has no causal variant). */
typedef struct sat_dit_attention_options {
    int32_t causal;         /* "causal" */
} sat_dit_attention_options;
int sat_dit_plan_set_attention_options(sat_dit_plan* plan, const sat_dit_attention_options* options, size_t options_bytes);

/* Neighbourhood-attention DiT (ContinuousTransformer attn_kwargs natten_kernel_size, models/transformer.py:299,324,479-493 of the reference),
 * between create and finalize; a plan never given this call, or given kernel_size 0, builds and launches exactly what it did before this
 * call existed.  With kernel_size K every self-attention is NATTEN's 1-D neighbourhood of K keys, dilation 1, over the sequence the blocks
 * see, n rows of [prepend rows | global token | tokens]: row i attends to the K rows start(i) .. start(i) + K - 1 of its own sequence,
 * start(i) = min(max(i - K / 2, 0), n - K) -- the window is shifted, not truncated, at both ends.  q and k are taken behind qk_norm and
 * the rotation, the softmax over the K logits runs in fp32, and the logits are NOT scaled by 1 / sqrt(dim_heads): the reference hands q to
 * natten1dqk as it is.  The kernels copy and walk only the key tiles that hold a workgroup's windows (csrc/attn_window.h).  No tensor is
 * added or renamed.  Runs with everything the 64-channel route runs with: bf16 / fp16 / per-block formats / SAT_GEMM_FP32X, both global
 * conditionings, prepend and input-concat conditioning, the transformer and block options, ff_conv and patch_size (the window counts tokens).
 * options_bytes = sizeof(sat_dit_neighborhood_options) of the caller's header; any other size is SAT_E_INVALID, as is a kernel_size that is
 * neither 0 nor odd and greater than 1 (what NATTEN rejects); a call after finalize is SAT_E_STATE.  SAT_E_UNSUPPORTED, with
 * "natten_kernel_size" in the message, for a kernel_size above 0 on a plan with cross-attention (cond_token_dim > 0: attn_kwargs reach
 * cross_attn too, where NATTEN fails on q and k of different lengths), on a causal plan (the reference ignores causal in this branch; the
 * causal call after this one is refused the same way), with gemm_dtype SAT_GEMM_FP8, or with dim_heads other than 64 (the staged widths are
 * a follow-up).  sat_dit_forward and the fused denoise answer SAT_E_INVALID before any launch when n < kernel_size. */
typedef struct sat_dit_neighborhood_options {
    int32_t kernel_size;    /* "natten_kernel_size"; 0 = full attention */
} sat_dit_neighborhood_options;
int sat_dit_plan_set_neighborhood_attention(sat_dit_plan* plan, const sat_dit_neighborhood_options* options, size_t options_bytes);
/* The same call for every built head width: dim_heads 64 as above, and 128, 32 and 96 (the staged route; csrc/attention_hdw_window.hip), in
 * bf16 / fp16 / per-block formats and, for 32 and 96, SAT_GEMM_FP32X.  Same struct, same checks and codes; SAT_E_UNSUPPORTED with a reason
 * if the library was built without those kernels.  What a staged plan is refused elsewhere stays refused: SAT_GEMM_FP32X at 128, the block
 * options and ff_conv off 64-channel heads.  sat_dit_plan_set_neighborhood_attention itself keeps refusing the staged widths. */
int sat_dit_plan_set_neighborhood_attention_hdw(sat_dit_plan* plan, const sat_dit_neighborhood_options* options, size_t options_bytes);

/* Operand format per block, between create and finalize: formats[l] is SAT_GEMM_FP16 or SAT_GEMM_BF16 for block l, n == depth.  A plan never
 * given this call, or given gemm_dtype in every entry, runs every block in gemm_dtype and builds and launches exactly what it did before this
 * call existed.  Block l then keeps its 16-bit weight images, every 16-bit activation buffer it writes (LayerNorm outputs, q / k / v, attention
 * outputs, the SwiGLU hidden state) and its slice of the cross-attention K / V cache in formats[l] and runs that build of the kernels; the range
 * report reads its buffers in that format.  The residual stream between blocks is fp32 in either case.  Meant for checkpoints where a few
 * blocks leave the fp16 range (sat_dit_range_report): those run in bf16, the rest keep fp16's 8x finer operand rounding.
 * Under ln_fold the first LayerNorm of a block whose format differs from the block before it runs as the standalone kernel (the image the
 * previous epilogue would write is in the writer's format): one more launch per format boundary, as block 0 has anyway.
 * Workspace and arena sizes do not change; with both formats in use sat_dit_prepare_context keeps a second 16-bit image of the context embedding.
 * The plan's gemm_dtype must be SAT_GEMM_BF16 or SAT_GEMM_FP16 (SAT_E_UNSUPPORTED otherwise); n != depth or any other value is SAT_E_INVALID,
 * a call after finalize SAT_E_STATE. */
int sat_dit_plan_set_block_formats(sat_dit_plan* plan, const int32_t* formats, int32_t n);

/* Checks that every required tensor was set, converts GEMM weights to bf16 (SwiGLU rows
 * interleaved), folds the 1x1 pre/post convs into the in/out projections, builds the RoPE
 * table.  Replaces nn.Module.load_state_dict for the DiT. */
int sat_dit_plan_finalize(sat_dit_plan* plan, sat_stream_t stream);

/* Bytes of caller workspace needed by sat_dit_forward / sat_dit_denoise_cfg for `bf`
 * sequences (bf = 2*B with CFG) of latent length `t_len`, for any prepend length up to the
 * plan's max_prepend_len. */
int sat_dit_workspace_bytes(const sat_dit_plan* plan, int32_t bf, int32_t t_len, size_t* out_bytes);

/* Per-generation constants (models/dit.py:150,154 to_cond_embed / to_global_embed and the
 * per-layer cross-attention to_kv projection, models/transformer.py:420-427): computed
 * once, reused by all sampler steps.  cross_attn_cond_dev [bf, lc, cond_token_dim] (NULL
 * if the model has no cross-attention), global_cond_dev [bf, global_cond_dim] or NULL. */
int sat_dit_prepare_context(sat_dit_plan* plan, const float* cross_attn_cond_dev, int32_t bf, int32_t lc,
                            const float* global_cond_dev, sat_stream_t stream);

/* Declares that sequences first_null_seq .. bf-1 of the prepared context are ALL-ZERO (the null embed of the
 * unconditional CFG half, models/dit.py:294-300).  Their cross-attention branch contributes exactly 0
 * (bias-free to_cond_embed / to_kv / to_out) and is skipped; results are unchanged.  -1 = none (default
 * after every sat_dit_prepare_context). */
int sat_dit_set_null_context_from(sat_dit_plan* plan, int32_t first_null_seq);

/* Per-generation extra conditioning, after sat_dit_prepare_context for the same bf (which discards that of the previous
 * generation); not part of the per-step work.  input_concat_dev [bf, input_concat_dim, concat_len] (both CFG halves carry
 * the same signal, models/dit.py:281-284) is copied and resized to each forward's t_len on the fly (F.interpolate
 * 'nearest', dit.py:170); it enters unscaled by the VDenoiser's c_in.  prepend_dev [bf, prepend_len, prepend_cond_dim]
 * (zeros for the unconditional half, dit.py:310-315) goes through to_prepend_embed here; 1 <= prepend_len <=
 * max_prepend_len, or NULL / 0.  Both NULL: no extra conditioning for this generation (the plain path).  Required (SAT_E_STATE at forward) when the model has input_concat_dim > 0.  With
 * prepend tokens the sequence is [P prepend | global token | T frames] and sat_dit_denoise_cfg applies CFG even without
 * cross-attention (dit.py:270). */
int sat_dit_prepare_extra_conditioning(sat_dit_plan* plan, const float* input_concat_dev, int32_t concat_len,
                                       const float* prepend_dev, int32_t prepend_len, int32_t bf, sat_stream_t stream);

/* DiffusionTransformer._forward (models/dit.py:135-226) on bf sequences:
 * x_dev [bf, io_channels, t_len], t_dev [bf] (timestep in [0,1]) -> out_dev [bf, io_channels, t_len]. */
int sat_dit_forward(sat_dit_plan* plan, const float* x_dev, const float* t_dev, float* out_dev,
                    int32_t bf, int32_t t_len, void* workspace_dev, size_t workspace_bytes, sat_stream_t stream);

/* One k-diffusion VDenoiser evaluation with batched CFG (k_diffusion.external.VDenoiser
 * called at inference/sampling.py:159 around DiTWrapper.forward; CFG models/dit.py:270-349):
 *   denoised = cfg(DiT(x*c_in, t(sigma))) * c_out + x * c_skip
 * x_dev, denoised_dev [b, io_channels, t_len]; the context prepared must hold bf = 2*b
 * sequences (cond half first, uncond half second) when cfg_scale != 1 and the model has
 * cross-attention or prepend tokens were prepared, else bf = b.
 * scale_phi: CFG rescale (models/dit.py:342-345); 0 = off. */
int sat_dit_denoise_cfg(sat_dit_plan* plan, const float* x_dev, float sigma, float cfg_scale, float scale_phi,
                        float* denoised_dev, int32_t b, int32_t t_len,
                        void* workspace_dev, size_t workspace_bytes, sat_stream_t stream);

/* Measurement hook for bench.py: while enabled, every forward brackets the FFN-in (SwiGLU) GEMM
 * launch of ONE transformer layer (depth/2) with a hipEvent pair on the launch stream (at most
 * 4096 pairs; enabling resets the count).  sat_dit_profile_read synchronises on the recorded
 * events and returns the summed elapsed time, the number of launches and the GEMM shape.  On a
 * plan with sat_dit_plan_set_ff_conv and glu=False the launch is the convolution GEMM and k is
 * kernel_size * embed_dim, the length of its contraction. */
int sat_dit_profile(sat_dit_plan* plan, int32_t enable);
int sat_dit_profile_read(sat_dit_plan* plan, double* total_ms, int32_t* launches, int64_t* m, int64_t* n, int64_t* k);

/* Diagnostics of the residual stream, for checkpoints this build could not be run on (the fp16 default rounds the UN-normalised
 * residual row to 16 bits for the LayerNorm fold and saturates at +-65504 -- models/transformer.py:692-700; real DiT checkpoints are known for
 * massive-activation channels, the synthetic weights of the test-suite have none).  While enabled (16-bit operand modes), every forward runs one
 * small reduction kernel behind each of the three residual updates of every block (self-attention to_out, cross-attention to_out, FF-out) and
 * keeps, over the rows of that update: [0] max |x|, [1] max over rows of |mean| / std (the common-mode ratio the fold's error grows with:
 * 3.7e-3 at 0, 2.1e-2 at 8, tests/test_gpu_kernels.py::test_ln_fold_rows_with_common_mode), [2] the number of elements beyond +-65504,
 * [3] max over rows of max |x| / rms.  sat_dit_debug_read copies the [depth][3][4] floats of the LAST forward to the host (synchronises the
 * stream).  Enabling allocates, disabling frees: not for the timed path.  What to do with it: see README "Checking a real checkpoint". */
int sat_dit_debug(sat_dit_plan* plan, int32_t enable);
int sat_dit_debug_read(sat_dit_plan* plan, float* out_host, int32_t capacity_floats, sat_stream_t stream);

/* fp16 range use of an activation buffer, accumulated on the device (csrc/range_stats.hip).  Every fp32 -> fp16 conversion of the fp16 build
 * SATURATES silently at +-65504; a record says how close a buffer came.  over_fp16: in an fp16 buffer the elements that sit AT the clamp
 * (|x| == 65504: clamped, or exactly there) or are non-finite; in a bf16 / fp32 buffer the elements fp16 WOULD clamp.  max_abs is the
 * largest finite |x|.  Maximum and integer sums do not depend on the order of accumulation: a record is bit-reproducible. */
typedef struct sat_range_record {
    float    max_abs;     /* max |x| over finite elements */
    uint32_t launches;    /* times this record was accumulated into */
    uint64_t over_fp16;   /* elements with |x| >= 65504 or non-finite */
    uint64_t nonfinite;   /* inf / NaN */
    uint64_t elements;    /* rows * cols summed over launches */
} sat_range_record;

/* Range report of the 16-bit buffers a DiT forward writes, beside sat_dit_debug (which reads the fp32 residual stream only and is not changed by
 * this; both may be on).  enable = 1: allocate depth * SAT_DIT_RANGE_SLOTS zeroed records (allowed before finalize); 0: free them (synchronises
 * the device); 2: zero the records and stay enabled.  While enabled, sat_dit_prepare_context and every forward / denoise launch one small
 * reduction behind each producer of a slot, and the records ACCUMULATE over all forwards until mode 2 or 0 -- a sampler run is covered as a
 * whole, not its last step.  Record (layer l, slot s) is at index l * SAT_DIT_RANGE_SLOTS + s; sat_dit_range_slot_name(s) names the slot (NULL
 * outside 0..SAT_DIT_RANGE_SLOTS-1):
 *   a_qkv, a_cross_q, a_ff     the A operand in front of to_qkv / cross to_q / FF-in: the LayerNorm output, or under ln_fold (every such GEMM
 *                              but layer 0's to_qkv) the 16-bit image of the residual rows written by the previous residual GEMM
 *   q, k, v                    the head-split buffers of self-attention
 *   attn_out, cross_attn_out   the attention outputs in front of the two to_out projections
 *   cross_q                    the cross branch's query buffer: only where the fused to_q + cross-attention launch is NOT taken
 *   ff_hidden                  the SwiGLU hidden state in front of FF-out
 *   cross_k, cross_v           the layer's context cache, once per sat_dit_prepare_context
 * `elements` counts the logical values (rows x channels of the model); the scan of q / k / v and of the context cache also covers the zero
 * pads of their layouts, which change neither max_abs nor a counter.  A slot the forward does not materialise keeps elements == 0.  The report
 * changes no decision of the forward (tile routing, the fused cross launch): outputs are bit-identical with it on and off, and a plan never given
 * the call launches exactly what it did before this entry point existed.  Toggling it changes what a forward ENQUEUES: a hipGraph captured
 * across a toggle (or a mode-2 reset expected inside it) is invalid -- capture with the report in the state it will replay in, or not at all.
 * 16-bit operand plans only: SAT_GEMM_FP8 (its A operands are e4m3) and SAT_GEMM_FP32X are SAT_E_UNSUPPORTED, as is a library built without
 * range_stats.hip.  sat_dit_range_report_read copies all depth * SAT_DIT_RANGE_SLOTS records to the host (synchronises the stream):
 * record_bytes = sizeof(sat_range_record) of the caller's header, any other size or too small a capacity is SAT_E_INVALID, a report that is
 * not enabled SAT_E_STATE. */
#define SAT_DIT_RANGE_SLOTS 12
int sat_dit_range_report(sat_dit_plan* plan, int32_t enable);
int sat_dit_range_report_read(sat_dit_plan* plan, sat_range_record* out_host, int32_t capacity_records, size_t record_bytes,
                              sat_stream_t stream);
const char* sat_dit_range_slot_name(int32_t slot);

/* Batched-CFG combine alone (models/dit.py:336-345): model_out_dev [2*b, c, t] (cond half, then
 * uncond half) -> out_dev [b, c, t] = uncond + (cond - uncond) * cfg_scale, with the optional
 * std rescale when scale_phi != 0. */
int sat_cfg_combine(const float* model_out_dev, float* out_dev, int32_t b, int32_t c, int32_t t,
                    float cfg_scale, float scale_phi, sat_stream_t stream);

/* One DPM-Solver++(3M) SDE update (k_diffusion.sampling.sample_dpmpp_3m_sde, called at
 * inference/sampling.py:228), fused elementwise over n elements:
 *   x <- a*x + b*d + c1*(d - d1) + c2*(d1 - d2) + cn*noise     (in place on x_dev)
 * The host computes the scalars from the sigma schedule (see the Python host code);
 * d1_dev / d2_dev / noise_dev may be NULL when their coefficient is 0.  A non-zero coefficient
 * with a NULL tensor is SAT_E_INVALID; c2 multiplies (d1 - d2), so c2 != 0 needs d1_dev as well
 * as d2_dev (the term is never dropped). */
int sat_dpmpp3m_update(float* x_dev, const float* d_dev, const float* d1_dev, const float* d2_dev,
                       const float* noise_dev, float a, float b, float c1, float c2, float cn,
                       int64_t n, sat_stream_t stream);

/* out <- c0*t0 + c1*t1 + c2*t2 + c3*t3 + c4*t4 over n floats; NULL terms are skipped, terms may alias out_dev.
 * State update of the single-step k-diffusion samplers selected at inference/sampling.py:212-225 (sample_heun, sample_lms,
 * sample_dpmpp_2s_ancestral, sample_dpm_2, sample_dpm_fast) and of sample_discrete_euler (:28-60): each is a linear
 * combination of the state, denoiser outputs and noise with host-computed scalars. */
int sat_lincomb(float* out_dev, const float* t0, float c0, const float* t1, float c1, const float* t2, float c2,
                const float* t3, float c3, const float* t4, float c4, int64_t n, sat_stream_t stream);

/* fp8 building blocks of gemm_dtype = 1, exported for the kernel-level parity tests:
 *   sat_quant_rows_fp8: x [rows, k] fp32 -> out8 [rows, k] OCP e4m3 bytes, row_scale[rows] = amax(row) / 448 (1 if the row is 0)
 *   sat_layernorm_fp8 : LayerNorm (eps 1e-5, transformer.py:205-206) fused with that row quantisation
 *   sat_gemm_fp8_f32  : c [m, n] (+)= (a8 . w8^T) * a_scale[m] * w_scale[n] (+ bias), k % 128 == 0, n % 128 == 0 */
int sat_quant_rows_fp8(const float* x_dev, void* out8_dev, float* row_scale_dev, int32_t rows, int32_t k, sat_stream_t stream);
int sat_layernorm_fp8(const float* x_dev, const float* gamma_dev, const float* beta_dev, void* y8_dev, float* row_scale_dev,
                      int32_t m, int32_t d, sat_stream_t stream);
int sat_gemm_fp8_f32(const void* a8_dev, const float* a_scale_dev, const void* w8_dev, const float* w_scale_dev,
                     const float* bias_dev, float* c_dev, int32_t m, int32_t n, int32_t k, int32_t accumulate, int32_t variant,
                     sat_stream_t stream);
/*   sat_quant_mx_rows_fp8: x [rows, k] fp32 -> MXFP8: out8 [rows, k] e4m3 bytes + scales [rows, k/32] E8M0 bytes
 *                          (scale = 2^ceil(log2(amax_block / 448)), byte = exponent + 127); k % 64 == 0
 *   sat_gemm_mxfp8_f32   : as sat_gemm_fp8_f32 with an MXFP8 A operand: the block scales are applied by the MFMA itself */
int sat_quant_mx_rows_fp8(const float* x_dev, void* out8_dev, void* scales_e8m0_dev, int32_t rows, int32_t k, sat_stream_t stream);
int sat_gemm_mxfp8_f32(const void* a8_dev, const void* a_scales_e8m0_dev, const void* w8_dev, const float* w_scale_dev,
                       const float* bias_dev, float* c_dev, int32_t m, int32_t n, int32_t k, int32_t accumulate, int32_t variant,
                       sat_stream_t stream);

/* Error estimate of one DPM-Solver adaptive step (k-diffusion sample_dpm_adaptive, inference/sampling.py:222-224):
 * partial_dev[j], j < n_partials, receive block-wise partial sums of ((x_low - x_high) / delta)^2 with
 * delta = max(atol, rtol * max(|x_low|, |x_prev|)); error = sqrt(sum(partials) / n), summed by the caller (fixed order). */
int sat_dpm_error_partials(const float* x_low_dev, const float* x_high_dev, const float* x_prev_dev, float atol, float rtol,
                           int64_t n, float* partial_dev, int32_t n_partials, sat_stream_t stream);

/* Inpainting re-injection (inference/sampling.py:98-103 get_bmask, :178-190 inpainting_callback, :168-172 initial mix):
 *   x[r, i] <- init[r, i] + noise[r, i] * sigma     wherever mask[i] <= strength      (in place on x_dev)
 * x/init/noise are [rows, t] (rows = batch * channels), mask is the [t] soft mask of generation.py:269-290 and
 * strength = (step + 1) / steps.  Called right after the denoiser evaluation of every step, as the reference's callback. */
int sat_inpaint_mix(float* x_dev, const float* init_dev, const float* noise_dev, const float* mask_dev,
                    float sigma, float strength, int64_t rows, int32_t t, sat_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Oobleck VAE.  Replaces models/autoencoders.py:45-194 (ResidualUnit, EncoderBlock,
 * DecoderBlock, OobleckEncoder, OobleckDecoder), models/blocks.py:318-358 (SnakeBeta),
 * dac.nn.layers.WNConv1d/WNConvTranspose1d (weight norm folded at finalize).
 * ---------------------------------------------------------------------------------- */
typedef struct sat_oobleck_plan sat_oobleck_plan;

typedef struct sat_oobleck_cfg {
    int32_t is_decoder;        /* 1 = OobleckDecoder, 0 = OobleckEncoder */
    int32_t io_channels;       /* decoder out_channels / encoder in_channels (2) */
    int32_t channels;          /* "channels" (128) */
    int32_t latent_dim;        /* decoder input (64) / encoder output (128) channels */
    int32_t n_blocks;          /* len(strides) (5) */
    int32_t c_mults[8];        /* WITHOUT the implicit leading 1: e.g. {1,2,4,8,16} */
    int32_t strides[8];        /* e.g. {2,4,4,8,8} */
    int32_t gemm_dtype;        /* SAT_GEMM_BF16 (0): bf16 activations / weights in the convolutions; SAT_GEMM_FP16 (3): IEEE fp16 (the
                                  reference's `model_half`, models/pretransforms.py:39-59: encoder / decoder in half precision) -- the
                                  fp16 build of the same kernels, same MFMA rate, saturating conversions; fp32 accumulation either way;
                                  SAT_GEMM_FP32X (2): fp32 activations / weights on the exact f32-input MFMA (the reference's
                                  `model_half=False` codec: no operand rounding, no fp16 range limit, 2x the workspace, 1/16 of the
                                  16-bit MFMA rate).  SAT_GEMM_FP8 is rejected (SAT_E_UNSUPPORTED). */
} sat_oobleck_cfg;

/* Snake, transposed-convolution upsampling, no final tanh (the Stable Audio VAEs); `channels` and a decoder's `latent_dim` must be
 * multiples of 64 (SAT_E_UNSUPPORTED otherwise).  == sat_oobleck_plan_create_ex(cfg, NULL, 0, out_plan) after that check. */
int sat_oobleck_plan_create(const sat_oobleck_cfg* cfg, sat_oobleck_plan** out_plan);

/* The other shapes of the reference's OobleckEncoder / OobleckDecoder (models/autoencoders.py:119-194). */
#define SAT_OOBLECK_ACT_SNAKE 0   /* use_snake=True: SnakeBeta, tensors "<...>.alpha" / "<...>.beta" */
#define SAT_OOBLECK_ACT_ELU 1     /* use_snake=False: nn.ELU(alpha=1), no tensors (set_tensor / finalize ask for none) */
typedef struct sat_oobleck_options {
    int32_t activation;        /* SAT_OOBLECK_ACT_*; fused into the producing convolution's epilogue either way */
    int32_t final_tanh;        /* decoder: 1 = tanh on the audio (final_tanh=True), in the last convolution's epilogue */
    int32_t nearest_upsample;  /* decoder: 1 = use_nearest_upsample=True: each block's upsampler is Upsample(nearest, stride) + a bias-free
                                  Conv1d(k = 2*stride, padding "same") with tensors "layers.<b>.layers.1.1.weight_g/_v"; runs as a
                                  three-tap polyphase convolution over the input rows m-1, m, m+1 (taps summed per phase at finalize) */
} sat_oobleck_options;

/* options_bytes = sizeof(sat_oobleck_options) of the header the CALLER was built against (any other size: SAT_E_INVALID, as
 * sat_dit_plan_create_sized); options == NULL takes the defaults {SNAKE, 0, 0}.  No rule on channel counts: `channels`, every
 * channels * c_mults[i] and `latent_dim` may be any positive integer.  The plan rounds each stage width up to a multiple of 64 and
 * zero-pads weights, biases and Snake parameters at finalize, so a narrow codec costs what the next multiple of 64 costs, and
 * sat_oobleck_workspace_bytes counts the padded widths.  An unknown option value is SAT_E_UNSUPPORTED.
 * Strides: 1..16, except where the reference's layer does not map L rows to L * stride (decoder) or L / stride (encoder) -- odd strides of
 * a transposed-convolution decoder (ConvTranspose1d yields L * stride - 1) and stride 1 of an encoder (L + 1) are SAT_E_UNSUPPORTED;
 * nearest_upsample decoders take every stride. */
int sat_oobleck_plan_create_ex(const sat_oobleck_cfg* cfg, const sat_oobleck_options* options, size_t options_bytes,
                               sat_oobleck_plan** out_plan);
/* antialias_activation=True of the reference (models/autoencoders.py:29-41): the activations the reference wraps in
 * alias_free_torch.Activation1d -- the one in front of every decoder block's upsampler and the one in front of the last convolution of either
 * direction; the ResidualUnits inside the blocks keep their plain activations, as the reference builds them -- run as 2x Kaiser-sinc
 * upsampling (12 taps, replicate padding), the activation at the doubled rate, low-pass and 2x decimation.  The convolution in front then
 * writes its un-activated result, in fp32 in every build, and one launch of a kernel of its own produces the tensor the next convolution
 * reads; sat_oobleck_workspace_bytes grows by the largest such fp32 tensor, with the option on only.  The 12 taps (cutoff 0.25, half-width 0.3) are constants of the kernel and no plan tensors; Snake parameters keep their names
 * ("layers.1.layers.0.act.alpha": the module tree puts the activation under ".act").  enable: 0 or 1 (SAT_E_UNSUPPORTED otherwise); allowed
 * between create and finalize (SAT_E_STATE afterwards).  A plan that never calls it, or calls it with 0, launches what it launched before the
 * option existed.  sat_oobleck_range_report(plan, 1) on a plan with the option on is SAT_E_UNSUPPORTED (no records for the added tensors). */
int sat_oobleck_plan_set_antialias(sat_oobleck_plan* plan, int32_t enable);
void sat_oobleck_plan_destroy(sat_oobleck_plan* plan);
/* `name` relative to the OobleckEncoder/OobleckDecoder module, e.g.
 * "layers.1.layers.2.layers.1.weight_v".  Pointer lifetime and the synchronising finalize: see sat_dit_plan_set_tensor. */
int sat_oobleck_plan_set_tensor(sat_oobleck_plan* plan, const char* name, const float* data_dev, int64_t numel);
int sat_oobleck_plan_finalize(sat_oobleck_plan* plan, sat_stream_t stream);
/* latent length `t_len` for both directions (audio length = t_len * prod(strides)). */
int sat_oobleck_workspace_bytes(const sat_oobleck_plan* plan, int32_t b, int32_t t_len, size_t* out_bytes);

/* OobleckDecoder.forward (models/autoencoders.py:193-194): z_dev [b, latent_dim, t_len]
 * -> audio_dev [b, io_channels, t_len * prod(strides)] fp32. */
int sat_oobleck_decode(sat_oobleck_plan* plan, const float* z_dev, float* audio_dev, int32_t b, int32_t t_len,
                       void* workspace_dev, size_t workspace_bytes, sat_stream_t stream);
/* OobleckEncoder.forward (models/autoencoders.py:152-153): audio_dev [b, io_channels, t_len*ratio]
 * -> out_dev [b, latent_dim, t_len] fp32 (for the VAE: mean | scale halves). */
int sat_oobleck_encode(sat_oobleck_plan* plan, const float* audio_dev, float* out_dev, int32_t b, int32_t t_len,
                       void* workspace_dev, size_t workspace_bytes, sat_stream_t stream);

/* Range report of the codec (sat_range_record, modes 0 / 1 / 2 and the hipGraph rule as sat_dit_range_report; all three builds, allowed before
 * finalize).  One record per activation tensor an encode / decode writes to its workspace, in launch order; the count depends on the plan's
 * blocks only.  sat_oobleck_range_report_name(plan, i) is the module path of the layer whose launch wrote tensor i, relative to the encoder /
 * decoder as in sat_oobleck_plan_set_tensor ("layers.3.layers.1.layers.1"), "input" for record 0 (the channels-last image of the decoder's
 * latents; the encoder reads its fp32 audio directly and has no such record), and path + ".raw" for the un-activated copy a launch keeps for
 * the next residual add beside the activated tensor.  NULL outside 0..count-1.  Pad channels of narrow stages are exact zeros and are scanned
 * and counted.  The fp32 build is the one to ask whether fp16 is safe: its over_fp16 is what the fp16 build would clamp.
 * While enabled, every ResidualUnit runs on the two-launch route (the one used above 256 channels and by the fp32 build), so that the tensor
 * between its two convolutions reaches memory and has a record; with the report off the fused kernel runs as before. */
int sat_oobleck_range_report(sat_oobleck_plan* plan, int32_t enable);
int sat_oobleck_range_report_count(const sat_oobleck_plan* plan, int32_t* out_records);
const char* sat_oobleck_range_report_name(const sat_oobleck_plan* plan, int32_t index);
int sat_oobleck_range_report_read(sat_oobleck_plan* plan, sat_range_record* out_host, int32_t capacity_records, size_t record_bytes,
                                  sat_stream_t stream);

/* One layer of the codec on the caller's tensors, for tests: the same weight packing (weight norm, polyphase forms, Snake parameters), the
 * same launch set-up and the same kernels a plan runs for that layer, nothing else.  Allocates and frees a temporary arena and synchronises
 * the stream before it returns: not for hot paths. */
#define SAT_OOBLECK_UNIT_CONV7 0        /* dilated k = 7 convolution + bias: in [b, t_len, Cp(c_in)] -> out_raw and / or out_snk [b, t_len, Cp(c_out)] */
#define SAT_OOBLECK_UNIT_CONV1_RES 1    /* 1 x 1 convolution + bias + res: out_raw (NULL, or == res: in place) and out_snk; c_in == c_out */
#define SAT_OOBLECK_UNIT_RESIDUAL 2     /* ResidualUnit: in = act(x), res = x -> out_raw (NULL or == res) = x + conv1(act2(conv7(in))), out_snk = act_next(that);
                                           conv7 = weight_g/_v/bias, act2 = alpha/beta, conv1 = weight_g2/_v2/bias2, act_next = alpha2/beta2; c_in == c_out.
                                           One fused launch where a plan fuses (16-bit builds, 128 or 256 channels) unless two_launch is set */
#define SAT_OOBLECK_UNIT_CONVT 3        /* ConvTranspose1d(k = 2 stride, stride, padding ceil(stride / 2)) + bias, weight_v [c_in, c_out, 2 stride]:
                                           in [b, t_len, Cp(c_in)] -> out_raw / out_snk [b, t_len * stride, Cp(c_out)]; even strides */
#define SAT_OOBLECK_UNIT_NEAREST 4      /* Upsample(nearest, stride) + Conv1d(k = 2 stride, "same"), no bias: shapes as CONVT, any stride */
#define SAT_OOBLECK_UNIT_STRIDED 5      /* encoder Conv1d(k = 2 stride, stride, padding ceil(stride / 2)) + bias: t_len (a multiple of stride >= 2) rows
                                           -> out_raw / out_snk [b, t_len / stride, Cp(c_out)] */
#define SAT_OOBLECK_UNIT_FIRST_CONV 6   /* encoder first convolution: in_cf [b, c_in <= 2, t_len] fp32 -> out_raw and out_snk [b, t_len, Cp(c_out)] */
#define SAT_OOBLECK_UNIT_FINAL_DEC 7    /* decoder last convolution, k = 7, no bias, tanh by final_tanh: -> out_cf [b, c_out, t_len] fp32 */
#define SAT_OOBLECK_UNIT_FINAL_ENC 8    /* encoder last convolution, k = 3, bias: -> out_cf [b, c_out, t_len] fp32 */
#define SAT_OOBLECK_UNIT_CF_TO_CL 9     /* in_cf [b, c_in, t_len] fp32 -> out_raw [b, t_len, Cp(c_in)], pad channels zero */
#define SAT_OOBLECK_UNIT_AA_ACT 11      /* the anti-aliased activation (sat_oobleck_plan_set_antialias): in [b, t_len, Cp(c_in)] -> out_snk of the same
                                           shape (not in place); activation, alpha / beta [c_in]; no weights, c_out ignored.  A plan hands the
                                           same kernel fp32 rows.  (10 stays unassigned and refused: the recorded launch list of
                                           tests/test_oobleck_launches_host.py pins "unknown kind 10") */
#define SAT_OOBLECK_AA_TIME_TILE 32     /* output rows one thread of that kernel walks: the seams of its time tiling (tests) */
typedef struct sat_oobleck_unit_desc {
    int32_t kind;              /* SAT_OOBLECK_UNIT_* */
    int32_t gemm_dtype;        /* as sat_oobleck_cfg: picks the bf16 / fp16 / fp32 build; the type of in, res, out_raw, out_snk */
    int32_t activation;        /* SAT_OOBLECK_ACT_*: the activation behind out_snk (and inside a ResidualUnit) */
    int32_t b, t_len;          /* batch items, input rows (time steps) per item */
    int32_t c_in, c_out;       /* channel counts of the reference layer; activations are Cp(c) = c rounded up to a multiple of 64 wide,
                                  pad channels of inputs zero */
    int32_t stride;            /* CONVT, NEAREST, STRIDED */
    int32_t dilation;          /* CONV7, RESIDUAL: 1, 3 or 9 */
    int32_t two_launch;        /* RESIDUAL: 1 = the two-launch route through memory whatever the width */
    int32_t final_tanh;        /* FINAL_DEC */
    int32_t reserved;          /* 0 */
    /* fp32 device tensors in the reference layout; bias NULL where the layer has none, alpha / beta NULL under ELU or without out_snk */
    const float *weight_g, *weight_v, *bias, *alpha, *beta;
    const float *weight_g2, *weight_v2, *bias2, *alpha2, *beta2;        /* RESIDUAL only */
    const void* in;            /* channels-last activations in the build's operand type */
    const float* in_cf;        /* FIRST_CONV, CF_TO_CL: channel-first fp32 input */
    const void* res;           /* CONV1_RES, RESIDUAL */
    void* out_raw;
    void* out_snk;
    float* out_cf;
} sat_oobleck_unit_desc;
/* desc_bytes = sizeof(sat_oobleck_unit_desc) of the caller's header (any other size: SAT_E_INVALID).  A kind, stride or dilation outside the
 * plan's repertoire is SAT_E_UNSUPPORTED, a missing pointer SAT_E_INVALID. */
int sat_oobleck_unit(const sat_oobleck_unit_desc* desc, size_t desc_bytes, sat_stream_t stream);

/* VAEBottleneck.encode / vae_sample (models/bottleneck.py:46-62) with the Gaussian noise
 * supplied by the caller: z = noise * (softplus(scale) + 1e-4) + mean.
 * mean_scale_dev [b, 2*c, t], noise_dev/z_dev [b, c, t]. */
int sat_vae_sample(const float* mean_scale_dev, const float* noise_dev, float* z_dev,
                   int32_t b, int32_t c, int32_t t, sat_stream_t stream);

/* float_to_int16_audio (utils/audio_utils.py:21-26) for one item of n samples:
 * peak = max|x| (device reduction), div = maximize ? peak : max(peak, 1),
 * out = (int16) trunc(x / div * 32767).  scratch_dev: >= 4 bytes (overwritten, need not be cleared).
 * All-zero input gives all-zero output under both settings of maximize. */
int sat_float_to_int16(const float* x_dev, int16_t* out_dev, int64_t n, int32_t maximize,
                       void* scratch_dev, sat_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Unit-level entry points (used by the parity tests and micro-benchmarks; the plans above
 * are built from exactly these kernels).
 * ---------------------------------------------------------------------------------- */
/* LayerNorm (models/transformer.py:205-206): x [m,d] fp32 -> y [m,d] bf16 (eps 1e-5). */
int sat_layernorm_bf16(const float* x_dev, const float* gamma_dev, const float* beta_dev, void* y_bf16_dev,
                       int32_t m, int32_t d, sat_stream_t stream);
/* fp32 -> bf16 (round to nearest even) */
int sat_cast_bf16(const float* x_dev, void* y_bf16_dev, int64_t n, sat_stream_t stream);
/* The reduction behind the range reports: accumulates the view x[r * pitch + c], r < rows, c < cols (elements; pitch >= cols; a 1-D buffer is
 * rows = 1) into *record_dev (sat_range_record, 8-byte aligned; the caller owns and zeroes it).  Elements cols..pitch-1 of a row are not
 * read into the statistics.  x of IEEE fp16, bf16 or fp32 elements. */
int sat_range_stats_f16(const void* x_dev, int64_t rows, int64_t cols, int64_t pitch, sat_range_record* record_dev, sat_stream_t stream);
int sat_range_stats_bf16(const void* x_dev, int64_t rows, int64_t cols, int64_t pitch, sat_range_record* record_dev, sat_stream_t stream);
int sat_range_stats_f32(const void* x_dev, int64_t rows, int64_t cols, int64_t pitch, sat_range_record* record_dev, sat_stream_t stream);
/* C[m,n] (fp32) = A[m,k] (bf16) * W[n,k]^T (bf16)  (+ bias[n]) ; accumulate != 0 adds into C.
 * n % 128 == 0, k % 64 == 0.  variant selects a tile configuration (0 = default). */
int sat_gemm_bf16_f32(const void* a_bf16_dev, const void* w_bf16_dev, const float* bias_dev, float* c_dev,
                      int32_t m, int32_t n, int32_t k, int32_t accumulate, int32_t variant, sat_stream_t stream);
/* The same GEMM with caller-supplied scratch: the 8-phase 256 x 256 tile cuts the remainder round of a long reduction (k >= 4096 behind
 * at least one whole round of tiles, e.g. FF-out at the SA-2.0 shape; or forced with variant bit 16) along K -- every partial K-range
 * stores its raw accumulators to a slab in `ws`, a second launch adds them in a fixed order.  sat_gemm_f32_workspace_bytes gives the
 * size (0: this shape does not split).  Without workspace (the entry above) nothing is ever split.  The DiT plan carves this scratch
 * out of the workspace the caller hands to sat_dit_forward: no call allocates, and plans on different streams never share scratch. */
int sat_gemm_f32_workspace_bytes(int32_t m, int32_t n, int32_t k, int32_t variant, size_t* out_bytes);
int sat_gemm_bf16_f32_ws(const void* a_bf16_dev, const void* w_bf16_dev, const float* bias_dev, float* c_dev,
                         int32_t m, int32_t n, int32_t k, int32_t accumulate, int32_t variant, void* ws_dev, size_t ws_bytes,
                         sat_stream_t stream);
/* SwiGLU GEMM (models/transformer.py:211-235): h[m,n/2] (bf16) = (A W_v^T + b_v) * silu(A W_g^T + b_g)
 * with W [n,k] in the REFERENCE row order (value rows then gate rows); re-packed internally
 * into wpack_dev [n,k] bf16 and bpack_dev [n] fp32 scratch. */
int sat_gemm_swiglu_bf16(const void* a_bf16_dev, const float* w_f32_dev, const float* bias_f32_dev,
                         void* wpack_dev, float* bpack_dev, void* h_bf16_dev,
                         int32_t m, int32_t n, int32_t k, int32_t variant, sat_stream_t stream);
/* Attention core (models/transformer.py:496-536): q [b,h,sq_pad,64], k [b,kvh,sk_pad,64],
 * vt [b,kvh,64,sk_pad] bf16 -> out [b*sq, h*64] bf16; softmax(q k^T / 8) v, GQA h/kvh.
 * Key-side layout: the sk keys of sequence i occupy rows (of k) / columns (of vt) [o_i, o_i + sk) with
 * o_i = (i*sk) & 3; everything outside must be finite (zero).  sq_pad % 128 == 0, sk_pad % 64 == 0,
 * sk_pad >= sk + 3.  (The shift lets the QKV GEMM epilogue store V^T with aligned 8-byte stores.)
 * Key order inside vt: every aligned group of 16 key columns is stored as [0-3, 8-11, 4-7, 12-15], i.e. key s sits at column
 * (s & ~12) | ((s & 4) << 1) | ((s & 8) >> 1) -- the order in which the second attention MFMA consumes the probabilities a lane
 * holds, so that a V^T tile is copied to LDS verbatim.  k keeps the natural order.  sat_qkv_rope_bf16 writes this layout. */
int sat_attention_bf16(const void* q_dev, const void* k_dev, const void* vt_dev, void* out_dev,
                       int32_t b, int32_t h, int32_t kvh, int32_t sq, int32_t sk, int32_t sq_pad, int32_t sk_pad,
                       sat_stream_t stream);
/* The same with q PRE-SCALED by its producer: q holds bf16(q_fp32 * log2(e) / 8), i.e. the scores come out of the first MFMA
 * in the log2 domain.  This is the layout the DiT plan runs (its QKV / to_q GEMM epilogues write it with one rounding); it lets
 * the single-KV-group kernel carry the softmax reference through the matrix pipe as a fifth K-step, which removes the per-score
 * multiply-add from the issue-bound VALU stream (attention). */
int sat_attention_prescaled_bf16(const void* q_dev, const void* k_dev, const void* vt_dev, void* out_dev,
                                 int32_t b, int32_t h, int32_t kvh, int32_t sq, int32_t sk, int32_t sq_pad, int32_t sk_pad,
                                 sat_stream_t stream);
/* ---- 128-channel heads (embed_dim == 128 * num_heads): the two kernels of the plan's staged route.
 * sat_attention_hd128_*: arguments and layouts of sat_attention_prescaled_* with 128 channels per head -- q [b, h, sq_pad, 128]
 * pre-scaled by log2(e) / sqrt(128), k [b, kvh, sk_pad, 128] and vt [b, kvh, 128, sk_pad] in the key-side layout (sequence i from row /
 * column (i * sk) & 3, vt's key index permuted inside aligned groups of 16 as [0-3, 8-11, 4-7, 12-15]), zero pads, sq_pad % 128 == 0,
 * sk_pad % 64 == 0, sk_pad >= sk + 3; out [b * sq, h * 128].  h and b above 65535 (the launch grid) are SAT_E_UNSUPPORTED. */
int sat_attention_hd128_bf16(const void* q_dev, const void* k_dev, const void* vt_dev, void* out_dev,
                             int32_t b, int32_t h, int32_t kvh, int32_t sq, int32_t sk, int32_t sq_pad, int32_t sk_pad,
                             sat_stream_t stream);
/* sat_head_split_hd128_*: x [b * s, parts * heads * 128] fp32 (the output of a bias-free projection), parts <= 3, part p -> dst_dev[p] with
 * kind[p] bits: 1 transposed [b, heads, 128, s_pad] with the key permutation above (no other bit but 4), else row-major [b, heads, s_pad, 128];
 * 2 rotate channels 0..63 in pairs (j, j + 32) by position * inv_freq[j] (inv_freq_dev: 32 floats; may be null when no part rotates);
 * 4 key-side: sequence i starts at row / column (i * s) & 3; 8 multiply by log2(e) / sqrt(128); 16 L2-normalise the 128 channels first,
 * x / max(|x|, 1e-12).  Order: normalise, rotate, scale, one rounding.  The destinations are zeroed first (pads), s_pad % 64 == 0,
 * s_pad >= s + 3; rope_scratch_dev: 2 * s * 32 floats. */
int sat_head_split_hd128_bf16(const float* x_dev, const float* inv_freq_dev, void* const* dst_dev, const int32_t* kind,
                              float* rope_scratch_dev, int32_t b, int32_t s, int32_t s_pad, int32_t heads, int32_t parts,
                              sat_stream_t stream);
/* ---- 32- and 96-channel heads (sat_dit_plan_create_ex, head_widths 1): the same two kernels for head_dim 32 or 96; any other head_dim is
 * SAT_E_UNSUPPORTED.  Test-only, as the 128-channel pair.
 * sat_attention_hdw_*: layouts of sat_attention_hd128_* with head_dim channels per head, q pre-scaled by log2(e) / sqrt(head_dim).  Rules
 * (SAT_E_INVALID otherwise): 16-byte aligned pointers, h % kvh == 0, sq_pad % 128 == 0, sq_pad >= sq, sk_pad >= sk + 3, and sk_pad a
 * multiple of the key tile -- 128 for head_dim 32, 64 for head_dim 96. */
int sat_attention_hdw_bf16(const void* q_dev, const void* k_dev, const void* vt_dev, void* out_dev, int32_t b, int32_t h, int32_t kvh,
                           int32_t head_dim, int32_t sq, int32_t sk, int32_t sq_pad, int32_t sk_pad, sat_stream_t stream);
/* sat_head_split_hdw_*: sat_head_split_hd128_* with head_dim channels per head.  Bit 2 of kind rotates as RotaryEmbedding(max(head_dim / 2, 32)):
 * head_dim 32: the whole head, pairs (j, j + 16), inv_freq_dev 16 floats; head_dim 96: channels 0..47, pairs (j, j + 24), inv_freq_dev 24
 * floats, channels 48..95 pass.  Bit 8 multiplies by log2(e) / sqrt(head_dim).  Rules (SAT_E_INVALID otherwise): s_pad % 64 == 0, s_pad >= s + 3,
 * x_dev and the destinations 16-byte aligned; rope_scratch_dev: 2 * s * 16 (32) or 2 * s * 24 (96) floats, 16-byte aligned. */
int sat_head_split_hdw_bf16(const float* x_dev, const float* inv_freq_dev, void* const* dst_dev, const int32_t* kind, float* rope_scratch_dev,
                            int32_t b, int32_t s, int32_t s_pad, int32_t heads, int32_t head_dim, int32_t parts, sat_stream_t stream);
/* ---- causal self-attention (sat_dit_plan_set_attention_options), test-only: query i of each of the b sequences of s rows sees the keys
 * j <= i.  head_dim 64: layouts and pad rules of sat_attention_bf16 (prescaled 0) / sat_attention_prescaled_bf16 (prescaled 1) with
 * sq == sk == s, sq_pad = s_pad_q, sk_pad = s_pad_k; head_dim 32 / 96 / 128: those of sat_attention_hdw_* / sat_attention_hd128_*, prescaled
 * must be 1.  Any other head_dim is SAT_E_UNSUPPORTED. */
int sat_attention_causal_bf16(const void* q_dev, const void* k_dev, const void* vt_dev, void* out_dev, int32_t b, int32_t h, int32_t kvh,
                              int32_t head_dim, int32_t s, int32_t s_pad_q, int32_t s_pad_k, int32_t prescaled, sat_stream_t stream);
/* ---- neighbourhood self-attention (sat_dit_plan_set_neighborhood_attention), test-only, 64-channel heads: query i of each of the b
 * sequences of s rows sees the kernel_size keys from min(max(i - kernel_size / 2, 0), s - kernel_size) on.  Layouts and pad rules of
 * sat_attention_causal_bf16 at head_dim 64.  score = q . k * score_scale with no other factor (1 / 8 reproduces scaled attention; the plan's
 * logits are unscaled).  SAT_E_INVALID for an even kernel_size, one of 1 or less, s < kernel_size, or a score_scale that is not a positive
 * finite number. */
int sat_attention_window_bf16(const void* q_dev, const void* k_dev, const void* vt_dev, void* out_dev, int32_t b, int32_t h, int32_t kvh,
                              int32_t s, int32_t s_pad_q, int32_t s_pad_k, int32_t kernel_size, float score_scale, sat_stream_t stream);
/* The same at head_dim 32, 96 or 128 (sat_dit_plan_set_neighborhood_attention_hdw), test-only.  Layouts and pad rules of sat_attention_hdw_bf16
 * (s_pad_k a multiple of 128 at head_dim 32, of 64 otherwise); there is no scale: score = q . k in the log2 domain, so the caller hands in q
 * times log2(e) times whatever factor it wants.  Any other head_dim is SAT_E_UNSUPPORTED. */
int sat_attention_hdw_window_bf16(const void* q_dev, const void* k_dev, const void* vt_dev, void* out_dev, int32_t b, int32_t h, int32_t kvh,
                                  int32_t head_dim, int32_t s, int32_t s_pad_q, int32_t s_pad_k, int32_t kernel_size, sat_stream_t stream);
/* Cross-attention query projection and attention core in one launch (models/transformer.py:430-437 + 496-536; what the DiT plan
 * runs per layer while the 128 x 64 GEMM tiles of the projection fit one round of workgroups, i.e. at one prompt):
 * out [b*s, d] bf16 = softmax((a wq^T) k^T / 8) v per head of 64, a [b*s, d] bf16, wq [d, d] bf16, k / vt in the key-side layout of
 * sat_attention_bf16 with sk + 3 <= 192 keys (they are staged in LDS as a whole); GQA d/64 over kvh.  Q never reaches memory. */
int sat_cross_attention_fused_bf16(const void* a_bf16_dev, const void* wq_bf16_dev, const void* k_dev, const void* vt_dev, void* out_dev,
                                   int32_t b, int32_t s, int32_t d, int32_t kvh, int32_t sk, int32_t sk_pad, sat_stream_t stream);
/* Fused QKV projection + partial RoPE + head split (models/transformer.py:430-452):
 * a [b*s, d] bf16, w_qkv [3d, d] bf16 -> q,k [b,h,s_pad,64], vt [b,h,64,s_pad] bf16 (k / vt in the key-side
 * layout of sat_attention_bf16; s_pad % 128 == 0, s_pad >= s + 3).
 * inv_freq_dev [16] fp32 (RotaryEmbedding.inv_freq, models/transformer.py:114-115). */
int sat_qkv_rope_bf16(const void* a_bf16_dev, const void* w_bf16_dev, const float* inv_freq_dev,
                      void* q_dev, void* k_dev, void* vt_dev, float* rope_scratch_dev,
                      int32_t b, int32_t s, int32_t s_pad, int32_t d, int32_t variant, sat_stream_t stream);
/* The same step of a qk_norm model (sat_dit_transformer_options.qk_norm; transformer.py:433-436): q and k are L2-normalised per head,
 * x / max(|x|, 1e-12), on the fp32 accumulators before the rotation, and q is written pre-scaled by log2(e) / 8 (the layout
 * sat_attention_prescaled_bf16 reads).  Ring tiles only: a variant that forces the 8-phase kernel is SAT_E_UNSUPPORTED. */
int sat_qkv_rope_qknorm_bf16(const void* a_bf16_dev, const void* w_bf16_dev, const float* inv_freq_dev,
                             void* q_dev, void* k_dev, void* vt_dev, float* rope_scratch_dev,
                             int32_t b, int32_t s, int32_t s_pad, int32_t d, int32_t variant, sat_stream_t stream);
/* LayerNorm folded into the GEMMs either side of it (sat_dit_cfg.ln_fold; models/transformer.py:692-700: x + f(LayerNorm(x))).
 * Producer = the GEMM that updates the residual stream (to_out, FF-out; transformer.py:319, 270):
 *   c [m, n] fp32 += a [m, k] . w [n, k]^T + bias; xb [m, n] bf16 = bf16(c); ln_part [m][n / 64][2] fp32 = per 64-column block
 *   (sum, sum of squares) of the rounded row.  n % 128 == 0, k % 64 == 0, k >= 192. */
int sat_gemm_resid_ln_bf16(const void* a_bf16_dev, const void* w_bf16_dev, const float* bias_dev, float* c_dev, void* xb_dev,
                           float* ln_part_dev, int32_t m, int32_t n, int32_t k, int32_t variant, sat_stream_t stream);
int sat_gemm_resid_ln_bf16_ws(const void* a_bf16_dev, const void* w_bf16_dev, const float* bias_dev, float* c_dev, void* xb_dev,
                              float* ln_part_dev, int32_t m, int32_t n, int32_t k, int32_t variant, void* ws_dev, size_t ws_bytes,
                              sat_stream_t stream);      /* with K-split scratch, as sat_gemm_bf16_f32_ws */
/* Consumers: xb / ln_part as written by the producer (k = its n).  SwiGLU FF-in (transformer.py:222, 232-235) of LayerNorm(x):
 * w_f32 [n, k], gamma / beta [k], bias [n] fp32 (reference layout: value rows then gate rows) -> h [m, n / 2] bf16.
 * wpack [n, k] bf16 and c12 [2 n] fp32 receive the re-packed operands: bf16(gamma (.) w) (value / gate rows interleaved by 32),
 * c1 = its row sums, c2 = w beta + bias; the epilogue computes rstd (acc - mean c1) + c2 before value * silu(gate). */
int sat_gemm_swiglu_ln_bf16(const void* xb_dev, const float* ln_part_dev, const float* w_f32_dev, const float* gamma_dev,
                            const float* beta_dev, const float* bias_f32_dev, void* wpack_dev, float* c12_dev, void* h_dev, int32_t m,
                            int32_t n, int32_t k, int32_t variant, sat_stream_t stream);
/* to_qkv + partial RoPE + head split of LayerNorm(x) (transformer.py:314, 430-452); outputs as sat_qkv_rope_bf16.
 * w_f32 [3d, d]; wpack [3d, d] bf16 and c12 [6 d] fp32 receive the re-packed operands. */
int sat_qkv_rope_ln_bf16(const void* xb_dev, const float* ln_part_dev, const float* w_f32_dev, const float* gamma_dev,
                         const float* beta_dev, void* wpack_dev, float* c12_dev, const float* inv_freq_dev, void* q_dev, void* k_dev,
                         void* vt_dev, float* rope_scratch_dev, int32_t b, int32_t s, int32_t s_pad, int32_t d, int32_t variant,
                         sat_stream_t stream);
/* ------------------------------------------------------------------------------------
 * The same unit-level entry points on IEEE fp16 operands (gemm_dtype = 3): identical signatures and layouts, every
 * "bf16" tensor holds fp16 instead, the kernels are the fp16 build of the same sources (v_mfma_f32_32x32x16_f16 /
 * v_mfma_f32_16x16x32_f16; conversions saturate at +-65504).
 * ---------------------------------------------------------------------------------- */
int sat_layernorm_f16(const float* x_dev, const float* gamma_dev, const float* beta_dev, void* y_f16_dev,
                      int32_t m, int32_t d, sat_stream_t stream);
int sat_cast_f16(const float* x_dev, void* y_f16_dev, int64_t n, sat_stream_t stream);
int sat_gemm_f16_f32(const void* a_f16_dev, const void* w_f16_dev, const float* bias_dev, float* c_dev,
                     int32_t m, int32_t n, int32_t k, int32_t accumulate, int32_t variant, sat_stream_t stream);
int sat_gemm_f16_f32_ws(const void* a_f16_dev, const void* w_f16_dev, const float* bias_dev, float* c_dev,
                        int32_t m, int32_t n, int32_t k, int32_t accumulate, int32_t variant, void* ws_dev, size_t ws_bytes,
                        sat_stream_t stream);
int sat_gemm_resid_ln_f16_ws(const void* a_f16_dev, const void* w_f16_dev, const float* bias_dev, float* c_dev, void* xb_dev,
                             float* ln_part_dev, int32_t m, int32_t n, int32_t k, int32_t variant, void* ws_dev, size_t ws_bytes,
                             sat_stream_t stream);
int sat_gemm_swiglu_f16(const void* a_f16_dev, const float* w_f32_dev, const float* bias_f32_dev,
                        void* wpack_dev, float* bpack_dev, void* h_f16_dev,
                        int32_t m, int32_t n, int32_t k, int32_t variant, sat_stream_t stream);
int sat_attention_f16(const void* q_dev, const void* k_dev, const void* vt_dev, void* out_dev,
                      int32_t b, int32_t h, int32_t kvh, int32_t sq, int32_t sk, int32_t sq_pad, int32_t sk_pad,
                      sat_stream_t stream);
int sat_attention_prescaled_f16(const void* q_dev, const void* k_dev, const void* vt_dev, void* out_dev,
                                int32_t b, int32_t h, int32_t kvh, int32_t sq, int32_t sk, int32_t sq_pad, int32_t sk_pad,
                                sat_stream_t stream);
int sat_attention_hd128_f16(const void* q_dev, const void* k_dev, const void* vt_dev, void* out_dev,
                            int32_t b, int32_t h, int32_t kvh, int32_t sq, int32_t sk, int32_t sq_pad, int32_t sk_pad,
                            sat_stream_t stream);
int sat_head_split_hd128_f16(const float* x_dev, const float* inv_freq_dev, void* const* dst_dev, const int32_t* kind,
                             float* rope_scratch_dev, int32_t b, int32_t s, int32_t s_pad, int32_t heads, int32_t parts,
                             sat_stream_t stream);
int sat_attention_hdw_f16(const void* q_dev, const void* k_dev, const void* vt_dev, void* out_dev, int32_t b, int32_t h, int32_t kvh,
                          int32_t head_dim, int32_t sq, int32_t sk, int32_t sq_pad, int32_t sk_pad, sat_stream_t stream);
int sat_head_split_hdw_f16(const float* x_dev, const float* inv_freq_dev, void* const* dst_dev, const int32_t* kind, float* rope_scratch_dev,
                           int32_t b, int32_t s, int32_t s_pad, int32_t heads, int32_t head_dim, int32_t parts, sat_stream_t stream);
int sat_attention_causal_f16(const void* q_dev, const void* k_dev, const void* vt_dev, void* out_dev, int32_t b, int32_t h, int32_t kvh,
                             int32_t head_dim, int32_t s, int32_t s_pad_q, int32_t s_pad_k, int32_t prescaled, sat_stream_t stream);
int sat_attention_window_f16(const void* q_dev, const void* k_dev, const void* vt_dev, void* out_dev, int32_t b, int32_t h, int32_t kvh,
                             int32_t s, int32_t s_pad_q, int32_t s_pad_k, int32_t kernel_size, float score_scale, sat_stream_t stream);
int sat_attention_hdw_window_f16(const void* q_dev, const void* k_dev, const void* vt_dev, void* out_dev, int32_t b, int32_t h, int32_t kvh,
                                 int32_t head_dim, int32_t s, int32_t s_pad_q, int32_t s_pad_k, int32_t kernel_size, sat_stream_t stream);
int sat_cross_attention_fused_f16(const void* a_f16_dev, const void* wq_f16_dev, const void* k_dev, const void* vt_dev, void* out_dev,
                                  int32_t b, int32_t s, int32_t d, int32_t kvh, int32_t sk, int32_t sk_pad, sat_stream_t stream);
int sat_qkv_rope_f16(const void* a_f16_dev, const void* w_f16_dev, const float* inv_freq_dev,
                     void* q_dev, void* k_dev, void* vt_dev, float* rope_scratch_dev,
                     int32_t b, int32_t s, int32_t s_pad, int32_t d, int32_t variant, sat_stream_t stream);
int sat_qkv_rope_qknorm_f16(const void* a_f16_dev, const void* w_f16_dev, const float* inv_freq_dev,
                            void* q_dev, void* k_dev, void* vt_dev, float* rope_scratch_dev,
                            int32_t b, int32_t s, int32_t s_pad, int32_t d, int32_t variant, sat_stream_t stream);

/* The two kernels of sat_dit_plan_set_block_options alone, for the parity tests (bf16 / fp16 operands).
 * sat_dwconv_ln_silu_*: y [b * s_len, d] = silu(LayerNorm_d(depthwise 17-tap convolution of x along each of the b sequences)), x and y
 *   16-bit, w [d, 17] / gamma / beta [d] fp32; d a multiple of 4, at most 2048.  variant 0: the kernel the plan runs (a 16-row tile and
 *   its 16 halo rows in registers).  1 to 3 are the designs it was measured against, with the same results: 1 one output row per
 *   workgroup, i.e. 17 reads of every input row out of L2; 2 a 32-row tile staged in LDS (d a multiple of 8, at most 1664); 3 the
 *   plan's kernel on an 8-row tile.
 * sat_gemm_act_*: h [m, n] (16-bit) = act(a [m, k] . w [n, k]^T + bias), act 0 identity / 1 SiLU, bias fp32 or NULL; variant as
 *   sat_gemm_bf16_f32 (a variant that forces the 8-phase kernel is SAT_E_UNSUPPORTED). */
int sat_dwconv_ln_silu_bf16(const void* x_bf16_dev, const float* w_dev, const float* gamma_dev, const float* beta_dev, void* y_bf16_dev,
                            int32_t b, int32_t s_len, int32_t d, int32_t variant, sat_stream_t stream);
int sat_dwconv_ln_silu_f16(const void* x_f16_dev, const float* w_dev, const float* gamma_dev, const float* beta_dev, void* y_f16_dev,
                           int32_t b, int32_t s_len, int32_t d, int32_t variant, sat_stream_t stream);
int sat_gemm_act_bf16(const void* a_bf16_dev, const void* w_bf16_dev, const float* bias_dev, void* h_bf16_dev, int32_t m, int32_t n,
                      int32_t k, int32_t act, int32_t variant, sat_stream_t stream);
int sat_gemm_act_f16(const void* a_f16_dev, const void* w_f16_dev, const float* bias_dev, void* h_f16_dev, int32_t m, int32_t n,
                     int32_t k, int32_t act, int32_t variant, sat_stream_t stream);

/* The convolution GEMM of sat_dit_plan_set_ff_conv alone, for the parity tests, through the plan's own packing and launches:
 *   acc[b, s, :] = sum_j w[:, :, j] . a[b, s + j - kernel_size / 2, :], rows outside [0, s_len) of sequence b zero.
 * format SAT_GEMM_BF16 / SAT_GEMM_FP16: a [b * s_len, k] in that format; SAT_GEMM_FP32X: a fp32 (row gather + sat_gemm_f32).  w [n, k,
 * kernel_size] (the Conv1d weight) and bias [n] or NULL are fp32.  epilogue 0, FF-out: out fp32 [b * s_len, n] += [gate[b] (.)] (acc + bias),
 * out holding the residual rows on entry; gate [b, n] fp32 or NULL.  epilogue 1, FF-in: out [b * s_len, n] = silu(acc + bias) in `format`
 * (fp32 under SAT_GEMM_FP32X); gate must be NULL.  ws of sat_ff_conv_workspace_bytes, 256-byte aligned: it starts with the tap-major weight
 * image [n, kernel_size * k] in `format`, which the call writes; every byte the kernels read of it the call has written.  w NULL: the
 * call packs nothing and runs on the image that an earlier call with the same format, n, k and kernel_size left in ws (the plan packs once,
 * at finalize: this times the convolution GEMM as the plan launches it).  k a multiple of 64, n of 128, kernel_size 1, 3, 5 or 7.  Returns
 * without synchronising, as every entry here. */
int sat_ff_conv_workspace_bytes(int32_t format, int32_t b, int32_t s_len, int32_t n, int32_t k, int32_t kernel_size, size_t* out_bytes);
int sat_ff_conv(int32_t format, const void* a_dev, const float* w_dev, const float* bias_dev, int32_t epilogue, void* out_dev,
                const float* gate_dev, int32_t b, int32_t s_len, int32_t n, int32_t k, int32_t kernel_size, void* ws, size_t ws_bytes,
                sat_stream_t stream);
int sat_gemm_resid_ln_f16(const void* a_f16_dev, const void* w_f16_dev, const float* bias_dev, float* c_dev, void* xb_dev,
                          float* ln_part_dev, int32_t m, int32_t n, int32_t k, int32_t variant, sat_stream_t stream);
int sat_gemm_swiglu_ln_f16(const void* xb_dev, const float* ln_part_dev, const float* w_f32_dev, const float* gamma_dev,
                           const float* beta_dev, const float* bias_f32_dev, void* wpack_dev, float* c12_dev, void* h_dev, int32_t m,
                           int32_t n, int32_t k, int32_t variant, sat_stream_t stream);
int sat_qkv_rope_ln_f16(const void* xb_dev, const float* ln_part_dev, const float* w_f32_dev, const float* gamma_dev,
                        const float* beta_dev, void* wpack_dev, float* c12_dev, const float* inv_freq_dev, void* q_dev, void* k_dev,
                        void* vt_dev, float* rope_scratch_dev, int32_t b, int32_t s, int32_t s_pad, int32_t d, int32_t variant,
                        sat_stream_t stream);

/* ------------------------------------------------------------------------------------
 * T5 encoder stack: the text front-end of the conditioner.  Replaces the transformers.T5EncoderModel call in
 * T5Conditioner.forward (models/conditioners.py:317-339): last_hidden_state for tokenised prompts.  The algorithm is
 * transformers' modeling_t5.py (T5Stack encoder: RMS T5LayerNorm, un-scaled attention with bucketed relative position bias shared
 * from block 0, ReLU or gated-GELU feed-forward); fp32 throughout (the reference runs it under fp16 autocast).
 * Tensors are named as in a Hugging Face T5 checkpoint: "shared.weight" (or "encoder.embed_tokens.weight"),
 * "encoder.block.N.layer.0.SelfAttention.{q,k,v,o}.weight", "encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight",
 * "encoder.block.N.layer.0.layer_norm.weight", "encoder.block.N.layer.1.DenseReluDense.{wi | wi_0,wi_1}.weight", "....wo.weight",
 * "encoder.block.N.layer.1.layer_norm.weight", "encoder.final_layer_norm.weight".
 * ---------------------------------------------------------------------------------- */
typedef struct sat_t5_plan sat_t5_plan;
typedef struct sat_t5_cfg {
    int32_t vocab_size;        /* T5Config.vocab_size (32128) */
    int32_t d_model;           /* 768 for t5-base */
    int32_t d_kv;              /* 64; inner dim = num_heads * d_kv */
    int32_t d_ff;              /* 3072 */
    int32_t num_layers;        /* 12 */
    int32_t num_heads;         /* 12 */
    int32_t rel_buckets;       /* relative_attention_num_buckets (32) */
    int32_t rel_max_distance;  /* relative_attention_max_distance (128) */
    int32_t gated_gelu;        /* feed_forward_proj: 0 = "relu" (t5-*), 1 = "gated-gelu" (flan-t5-*) */
    int32_t proj_dim;          /* > 0: Conditioner.proj_out = Linear(d_model, proj_dim) (conditioners.py:23) applied to the output,
                                  tensors "proj_out.weight" [proj_dim, d_model] / "proj_out.bias"; 0: identity */
    float eps;                 /* layer_norm_epsilon (1e-6) */
} sat_t5_cfg;
int sat_t5_plan_create(const sat_t5_cfg* cfg, sat_t5_plan** out_plan);
void sat_t5_plan_destroy(sat_t5_plan* plan);
/* (pointer lifetime and the synchronising finalize: see sat_dit_plan_set_tensor) */
int sat_t5_plan_set_tensor(sat_t5_plan* plan, const char* name, const float* data_dev, int64_t numel);
int sat_t5_plan_finalize(sat_t5_plan* plan, sat_stream_t stream);
int sat_t5_workspace_bytes(const sat_t5_plan* plan, int32_t b, int32_t l, size_t* out_bytes);
/* input_ids_dev / attention_mask_dev [b, l] int32 (tokenizer output, padding = mask 0) -> out_dev [b, l, proj_dim or d_model] fp32
 * = proj_out(model(input_ids, attention_mask)["last_hidden_state"]), and with mask_output != 0 multiplied by the mask
 * (conditioners.py:333-341); l <= 512 */
int sat_t5_encode(sat_t5_plan* plan, const int32_t* input_ids_dev, const int32_t* attention_mask_dev, float* out_dev, int32_t b,
                  int32_t l, int32_t mask_output, void* workspace_dev, size_t workspace_bytes, sat_stream_t stream);
/* HOST helper (no GPU): T5Attention._relative_position_bucket(key - query, bidirectional=True) for key - query in
 * [-(l-1), l-1] -> out_host[2l - 1] */
int sat_t5_relative_buckets(int32_t l, int32_t num_buckets, int32_t max_distance, int32_t* out_host);

/* ------------------------------------------------------------------------------------
 * RoBERTa encoder stack: the text branch of CLAP, front-end of the "clap_text" conditioner.  Replaces the
 * text_branch(input_ids, attention_mask, output_hidden_states=True)["hidden_states"][feature_layer_ix] call of
 * CLAPTextConditioner.get_clap_features (models/conditioners.py:162-171) and the proj_out after it (:182).  The algorithm is
 * transformers' modeling_roberta.py (BERT post-LayerNorm, absolute positions counted from the input ids, scaled attention with a
 * key mask, exact erf GELU); fp32 throughout (the reference runs it under fp16 autocast).
 * Tensors are named as in RobertaModel.state_dict(): "embeddings.{word,position,token_type}_embeddings.weight" (of the token-type
 * table only row 0 is used), "embeddings.LayerNorm.{weight,bias}", and per layer N < run_layers
 * "encoder.layer.N.attention.self.{query,key,value}.{weight,bias}", "encoder.layer.N.attention.output.{dense,LayerNorm}.{weight,bias}",
 * "encoder.layer.N.intermediate.dense.{weight,bias}", "encoder.layer.N.output.{dense,LayerNorm}.{weight,bias}".  Layers from
 * run_layers on and the pooler are never read.
 * ---------------------------------------------------------------------------------- */
typedef struct sat_roberta_plan sat_roberta_plan;
typedef struct sat_roberta_cfg {
    int32_t vocab_size;         /* RobertaConfig.vocab_size (50265) */
    int32_t hidden_size;        /* 768 for roberta-base */
    int32_t num_layers;         /* num_hidden_layers of the checkpoint (12) */
    int32_t run_layers;         /* layers evaluated: the output is hidden_states[run_layers], 0 = the embeddings, num_layers = the last
                                   hidden state; feature_layer_ix = -2 of roberta-base is 11 */
    int32_t num_heads;          /* 12; head dim = hidden_size / num_heads */
    int32_t intermediate_size;  /* 3072 */
    int32_t max_positions;      /* max_position_embeddings (514): rows of the position table */
    int32_t pad_id;             /* pad_token_id (1): positions are pad_id + 1, pad_id + 2, ... at non-pad tokens and pad_id at pad tokens */
    int32_t proj_dim;           /* > 0: Conditioner.proj_out = Linear(hidden_size, proj_dim) (conditioners.py:23) applied to the output,
                                   tensors "proj_out.weight" [proj_dim, hidden_size] / "proj_out.bias"; 0: identity */
    float eps;                  /* layer_norm_eps (1e-5) */
} sat_roberta_cfg;
int sat_roberta_plan_create(const sat_roberta_cfg* cfg, sat_roberta_plan** out_plan);
void sat_roberta_plan_destroy(sat_roberta_plan* plan);
/* (pointer lifetime and the synchronising finalize: see sat_dit_plan_set_tensor) */
int sat_roberta_plan_set_tensor(sat_roberta_plan* plan, const char* name, const float* data_dev, int64_t numel);
int sat_roberta_plan_finalize(sat_roberta_plan* plan, sat_stream_t stream);
/* l <= max_positions - pad_id - 1 (the position table) and l <= 512, else SAT_E_UNSUPPORTED; needs no finalized plan */
int sat_roberta_workspace_bytes(const sat_roberta_plan* plan, int32_t b, int32_t l, size_t* out_bytes);
/* input_ids_dev / attention_mask_dev [b, l] int32 (tokenizer output) -> out_dev [b, l, proj_dim or hidden_size] fp32
 * = proj_out(hidden_states[run_layers]).  Keys with attention_mask == 0 are excluded; padded rows are computed and NOT zeroed, as in
 * the reference.  Allocates nothing and does not synchronise. */
int sat_roberta_encode(sat_roberta_plan* plan, const int32_t* input_ids_dev, const int32_t* attention_mask_dev, float* out_dev,
                       int32_t b, int32_t l, void* workspace_dev, size_t workspace_bytes, sat_stream_t stream);

/* SnakeBeta (models/blocks.py:318-319): y = x + sin^2(x*exp(alpha_c)) / (exp(beta_c)+1e-9); x,y [b,c,t] fp32 */
int sat_snake_beta(const float* x_dev, const float* alpha_dev, const float* beta_dev, float* y_dev,
                   int32_t b, int32_t c, int32_t t, sat_stream_t stream);

/* Sample-rate conversion, polyphase windowed-sinc FIR = torchaudio.transforms.Resample with its defaults (inference/utils.py:25-27,
 * models/autoencoders.py:394-397, reconstruct_audios.py:34-35 of the reference).  x [rows, in_len] fp32 -> y [rows, out_len] fp32,
 * out_len <= ceil(in_len * new / orig); orig / new are the two rates divided by their gcd; bank [new, 2 * width + orig] fp32 is the
 * filter bank (row p = output phase p; built on the host, stable_audio_tools/inference/resample.py: sinc_resample_bank). */
int sat_resample_sinc(const float* x_dev, const float* bank_dev, float* y_dev, int32_t rows, int32_t in_len, int32_t out_len,
                      int32_t orig, int32_t new_rate, int32_t width, sat_stream_t stream);
/* Windowed overlap-add of the chunked codec paths, AudioAutoencoder.encode_audio / decode_audio / reconstruct_audio
 * (models/autoencoders.py:476-497, 548-571, 622-645): pieces_dev [batch, n_chunk, channels, chunk_len], chunk i placed at i * hop,
 * faded in / out over `overlap` samples with window_dev [2 * overlap] (torch.bartlett_window(2 * overlap)) except at the outer
 * edges of the first / last chunk -> out_dev [batch, channels, total_len] (every sample written). */
int sat_overlap_add(const float* pieces_dev, const float* window_dev, float* out_dev, int32_t batch, int32_t n_chunk, int32_t channels,
                    int32_t chunk_len, int32_t hop, int32_t overlap, int32_t total_len, sat_stream_t stream);

/* NumberConditioner.forward (models/conditioners.py:64-102) with its NumberEmbedder (models/adp.py:1495-1514, 680-694):
 *   x = (clamp(v, min_val, max_val) - min_val) / (max_val - min_val)
 *   out[b] = Linear(cat(x, sin(2 pi x w), cos(2 pi x w)))     w = embedder.embedding.0.weights [half_dim],
 *   linear_w = embedder.embedding.1.weight [features, 2*half_dim + 1], linear_b = ...bias [features]
 * values_dev [count] -> out_dev [count, features] (the caller adds the singleton token axis and the all-ones mask). */
int sat_number_embed(const float* values_dev, int32_t count, float min_val, float max_val, const float* pos_weights_dev,
                     int32_t half_dim, const float* linear_w_dev, const float* linear_b_dev, int32_t features, float* out_dev,
                     sat_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Unit entries of the fp32 path, the text-encoder kernels and the DiT glue: ONE kernel each on caller tensors, through the very launcher
 * (grid, LDS size, argument checks) the plans call.  For the parity tests (tests/test_gpu_fp32_kernels.py) and for probes; every pointer is
 * a device pointer, every tensor contiguous fp32 unless noted.  A NULL pointer or a non-positive / inconsistent dimension is SAT_E_INVALID,
 * a dimension outside the kernel's repertoire SAT_E_UNSUPPORTED; both are decided before anything is launched.
 * ---------------------------------------------------------------------------------- */
/* fp32 GEMM (gemm_dtype fp32x, both text encoders): C[m, :n] (row pitch ldc >= n) (+)= (A[m,k] W[n,k]^T + bias[n]) * gate[m / gate_rows][n]
 * (gate row pitch gate_ld; bias and gate may be NULL).  k % 16 == 0; A and W 16-byte aligned.  Columns n..ldc-1 of C are not touched. */
int sat_gemm_f32(const float* a_dev, const float* w_dev, const float* bias_dev, float* c_dev, int32_t m, int32_t n, int32_t k, int32_t ldc,
                 int32_t accumulate, const float* gate_dev, int32_t gate_rows, int32_t gate_ld, sat_stream_t stream);
/* LayerNorm x [m,d] -> y [m,d]: (x - mean) * rsqrt(var + eps) * gamma + beta (beta may be NULL), then, with scale_dev / shift_dev,
 * * scale[r / rows_per_seq][:] + shift[r / rows_per_seq][:] (row pitch ld >= d: the adaLN modulation). */
int sat_layernorm_f32(const float* x_dev, const float* gamma_dev, const float* beta_dev, float* y_dev, int32_t m, int32_t d,
                      const float* scale_dev, const float* shift_dev, int32_t rows_per_seq, int32_t ld, float eps, sat_stream_t stream);
/* src [b * s_len, parts * heads * 64] -> d0 / d1 / d2 [b, heads, s_len, 64] (parts = 1..3).  Parts in rope_mask (bit = part): partial rotary on
 * channels < 32, pairs (c, c + 16), with rope_cos / rope_sin [s_len, 16] from the caller; parts in norm_mask: L2-normalised per head. */
int sat_split_heads_f32(const float* src_dev, float* d0_dev, float* d1_dev, float* d2_dev, int32_t b, int32_t s_len, int32_t parts,
                        int32_t heads, int32_t rope_mask, const float* rope_cos_dev, const float* rope_sin_dev, int32_t norm_mask,
                        sat_stream_t stream);
/* hg [m, 2 * inner] (value | gate) -> h [m, inner] = value * silu(gate) */
int sat_swiglu_f32(const float* hg_dev, float* h_dev, int64_t m, int32_t inner, sat_stream_t stream);
/* softmax(q k^T / 8) v on 64-channel heads: q [b,h,sq,64], k / v [b,kvh,sk,64] (h % kvh == 0) -> out [b * sq, h * 64] */
int sat_attention_f32(const float* q_dev, const float* k_dev, const float* v_dev, float* out_dev, int32_t b, int32_t h, int32_t kvh,
                      int32_t sq, int32_t sk, sat_stream_t stream);
/* The two kernels above for heads of head_dim channels, 32, 64 or 96 (SAT_E_UNSUPPORTED otherwise; 64 is exactly the pair above): tensors
 * [.., head_dim]; the rotation is RotaryEmbedding(max(head_dim / 2, 32)) -- tables [s_len, 16] and pairs (c, c + 16) for 32 and 64, [s_len, 24]
 * and pairs (c, c + 24) for 96; scores scaled by 1 / sqrt(head_dim).  Pointer rules as above (q and out 16-byte aligned). */
int sat_split_heads_f32_hdw(const float* src_dev, float* d0_dev, float* d1_dev, float* d2_dev, int32_t b, int32_t s_len, int32_t parts,
                            int32_t heads, int32_t head_dim, int32_t rope_mask, const float* rope_cos_dev, const float* rope_sin_dev,
                            int32_t norm_mask, sat_stream_t stream);
int sat_attention_f32_hdw(const float* q_dev, const float* k_dev, const float* v_dev, float* out_dev, int32_t b, int32_t h, int32_t kvh,
                          int32_t head_dim, int32_t sq, int32_t sk, sat_stream_t stream);
/* The same attention, causal (sq == sk == s, query i sees the keys j <= i), for head_dim 32, 64 or 96 */
int sat_attention_f32_causal(const float* q_dev, const float* k_dev, const float* v_dev, float* out_dev, int32_t b, int32_t h, int32_t kvh,
                             int32_t head_dim, int32_t s, sat_stream_t stream);
/* The same attention over a neighbourhood of kernel_size keys (sat_attention_window_bf16's rule and errors), 64-channel heads, scores times
 * score_scale: q [b,h,s,64], k / v [b,kvh,s,64] -> out [b*s, h*64] */
int sat_attention_f32_window(const float* q_dev, const float* k_dev, const float* v_dev, float* out_dev, int32_t b, int32_t h, int32_t kvh,
                             int32_t s, int32_t kernel_size, float score_scale, sat_stream_t stream);
/* The same for head_dim 32 or 96 (any other is SAT_E_UNSUPPORTED): q [b,h,s,head_dim], k / v [b,kvh,s,head_dim] -> out [b*s, h*head_dim] */
int sat_attention_f32_window_w(const float* q_dev, const float* k_dev, const float* v_dev, float* out_dev, int32_t b, int32_t h, int32_t kvh,
                               int32_t head_dim, int32_t s, int32_t kernel_size, float score_scale, sat_stream_t stream);
/* Self-attention of the text encoders: qkv [b * l, 3 * h * dkv] (q | k | v) -> out [b * l, h * dkv] = softmax(scale * q k^T + pb + mask) v;
 * pb [h, 2l - 1] indexed by key - query + l - 1, or NULL; keys with mask [b, l] == 0 get finfo(float32).min added (an all-padding row is the
 * uniform average over all l keys).  l <= 512, dkv % 4 == 0, (dkv + l) * 4 bytes of LDS <= 64 KiB. */
int sat_enc_attention(const float* qkv_dev, const float* pb_dev, const int32_t* mask_dev, float* out_dev, int32_t b, int32_t l, int32_t h,
                      int32_t dkv, float scale, sat_stream_t stream);
/* The T5 kernels: embedding rows (ids clamped to [0, vocab)); T5LayerNorm x * rsqrt(mean(x^2) + eps) * w; pb[h][i] = relb[bucket[i]][h]
 * (relb [buckets, h], i < n); relu (gated = 0: g, h [rows, f], may alias) or gelu_new(g[:, :f]) * g[:, f:] (gated = 1: g [rows, 2f]);
 * rows with mask == 0 set to zero in place.  d % 4 == 0 for the first two. */
int sat_t5_embed(const int32_t* ids_dev, const float* emb_dev, float* out_dev, int32_t rows, int32_t d, int32_t vocab, sat_stream_t stream);
int sat_t5_rmsnorm(const float* x_dev, const float* w_dev, float* y_dev, int32_t m, int32_t d, float eps, sat_stream_t stream);
int sat_t5_position_bias(const float* relb_dev, const int32_t* bucket_dev, float* pb_dev, int32_t h, int32_t n, sat_stream_t stream);
int sat_t5_act(const float* g_dev, float* h_dev, int64_t rows, int32_t f, int32_t gated, sat_stream_t stream);
int sat_t5_mask_rows(float* y_dev, const int32_t* mask_dev, int64_t rows, int32_t d, sat_stream_t stream);
/* RobertaEmbeddings: y [b * l, d] = LayerNorm(word[id] + type0 + posw[pos]), pos = pad_id + (number of non-pad ids up to and including
 * the token) at non-pad tokens, pad_id at pad tokens; posw [max_positions, d], pad_id + l < max_positions.  Exact (erf) GELU in place. */
int sat_roberta_embed_ln(const int32_t* ids_dev, const float* word_dev, const float* posw_dev, const float* type0_dev, const float* gamma_dev,
                         const float* beta_dev, float* y_dev, int32_t b, int32_t l, int32_t d, int32_t vocab, int32_t pad_id,
                         int32_t max_positions, float eps, sat_stream_t stream);
int sat_roberta_gelu(float* h_dev, int64_t n, sat_stream_t stream);
/* y[r][:n] (row pitch ldy; out16 0: fp32, 1: bf16, 2: fp16) = act(x[r][:k] (pitch ldx) W[n,k]^T + bias) + add[r][:n] (pitch ldadd);
 * act 0: none, 1: SiLU before the add, 2: SiLU after it; bias / add may be NULL.  k % 4 == 0, ldx % 4 == 0. */
int sat_small_linear(const float* x_dev, int32_t ldx, const float* w_dev, const float* bias_dev, const float* add_dev, int32_t ldadd,
                     void* y_dev, int32_t ldy, int32_t r, int32_t n, int32_t k, int32_t act, int32_t out16, sat_stream_t stream);
/* ssg [n / (6 d), 6, d] in place: chunks 0 and 3 -> 1 + v, chunks 2 and 5 -> sigmoid(1 - v), the others unchanged */
int sat_adaln_finish(float* ssg_dev, int64_t n, int32_t d, sat_stream_t stream);
/* out [b, 2 * half_feat] = cat(cos f, sin f), f = 2 pi t w[j]; t = t_dev[b], or t_const for every b when t_dev is NULL */
int sat_fourier_features(const float* t_dev, float t_const, const float* w_dev, float* out_dev, int32_t b, int32_t half_feat,
                         sat_stream_t stream);
/* The folded projections, stored transposed: w_eff_t [c, d] = (W_in (I + W_pre))^T for W_in [d, c], W_pre [c, c];
 * w_eff_t [d, c] = ((I + W_post) W_out)^T for W_out [c, d], W_post [c, c]. */
int sat_fold_in(const float* w_in_dev, const float* w_pre_dev, float* w_eff_t_dev, int32_t d, int32_t c, sat_stream_t stream);
int sat_fold_out(const float* w_out_dev, const float* w_post_dev, float* w_eff_t_dev, int32_t d, int32_t c, sat_stream_t stream);
/* X [bf, s_len, d]: X[b, (s_len - t) + i, :] = xscale * w_eff_t[:c]^T x[b % xb, :, i] for x [xb, c, t], c <= 64; rows below s_len - t are
 * not touched.  _extra: + w_eff_t[c : c + cc]^T concat[b, :, src(i)] (concat [bf, cc, tc], src the nearest-neighbour frame of
 * F.interpolate, unscaled), and X[b, j, :] = prep[b, j, :] for j < p (prep [bf, p, d]); s_len = p + 1 + t, or t when p == 0;
 * row p, the global token's, is not touched. */
int sat_input_proj(const float* x_dev, const float* w_eff_t_dev, float* X_dev, int32_t bf, int32_t xb, int32_t c, int32_t t, int32_t s_len,
                   int32_t d, float xscale, sat_stream_t stream);
int sat_input_proj_extra(const float* x_dev, const float* w_eff_t_dev, float* X_dev, int32_t bf, int32_t xb, int32_t c, int32_t t,
                         int32_t s_len, int32_t d, float xscale, const float* concat_dev, int32_t cc, int32_t tc, const float* prep_dev,
                         int32_t p, sat_stream_t stream);
/* out [bf, c, t]: out[b, :, i] = w_eff_t^T X[b, (s_len - t) + i, :] for w_eff_t [d, c]; c % 4 == 0, c <= 64, d % 128 == 0, d <= 2048 */
int sat_output_proj(const float* X_dev, const float* w_eff_t_dev, float* out_dev, int32_t bf, int32_t c, int32_t t, int32_t s_len, int32_t d,
                    sat_stream_t stream);
/* The same four for a plan with sat_dit_plan_set_patch, patch_size P >= 2 (t a multiple of P, else SAT_E_INVALID; c * P <= 512 and
 * (c + cc) * P <= 1024, else SAT_E_UNSUPPORTED).  Folds: W_in [d, ci * P] -> w_eff_t [ci * P, d], W_out [c * P, d] -> w_eff_t [d, c * P],
 * feature index channel * P + p, W_pre [ci, ci] / W_post [c, c] applied inside each p.  sat_input_proj_patch: X [bf, s_len, d],
 * X[b, (s_len - t / P) + i, :] = xscale * sum_{ch, p} w_eff_t[ch * P + p] x[b % xb, ch, i * P + p] + the cc concat channels (rows
 * (c + j) * P + p of w_eff_t) read at the nearest-neighbour source frame of frame i * P + p, unscaled, and X[b, j, :] = prep[b, j, :]
 * for j < p; cc = 0 with concat NULL and p = 0 with prep NULL is the plain model.  sat_output_proj_patch: out [bf, c, t],
 * out[b, ch, i * P + p] = w_eff_t[:, ch * P + p]^T X[b, (s_len - t / P) + i, :]. */
int sat_fold_in_patch(const float* w_in_dev, const float* w_pre_dev, float* w_eff_t_dev, int32_t d, int32_t ci, int32_t patch_size,
                      sat_stream_t stream);
int sat_fold_out_patch(const float* w_out_dev, const float* w_post_dev, float* w_eff_t_dev, int32_t d, int32_t c, int32_t patch_size,
                       sat_stream_t stream);
int sat_input_proj_patch(const float* x_dev, const float* w_eff_t_dev, float* X_dev, int32_t bf, int32_t xb, int32_t c, int32_t patch_size,
                         int32_t t, int32_t s_len, int32_t d, float xscale, const float* concat_dev, int32_t cc, int32_t tc,
                         const float* prep_dev, int32_t p, sat_stream_t stream);
int sat_output_proj_patch(const float* X_dev, const float* w_eff_t_dev, float* out_dev, int32_t bf, int32_t c, int32_t patch_size, int32_t t,
                          int32_t s_len, int32_t d, sat_stream_t stream);
/* table [rows, d]: mode 1 cat(sin, cos)(pos * 10000^(-j / (d / 2))) * src[0]; mode 2 src[pos][:] * d^-0.5 (src [>= rows, d]).
 * X [bf, s_len, d] += table[s] (the caller's table, [>= s_len, d]); d % 4 == 0. */
int sat_pos_table(int32_t mode, const float* src_dev, float* table_dev, int32_t rows, int32_t d, sat_stream_t stream);
int sat_add_pos(float* X_dev, const float* table_dev, int32_t bf, int32_t s_len, int32_t d, sat_stream_t stream);
/* den [b,c,t] = g * c_out + x * c_skip; g = model_out[:b] without CFG, else u + (cond - u) * cfg_scale with cond = model_out[:b],
 * u = model_out[b:2b], times scale_phi * std_c(cond) / std_c(g) + 1 - scale_phi when scale_phi != 0 (sat_cfg_combine is c_out 1, c_skip 0) */
int sat_cfg_denoise(const float* model_out_dev, const float* x_dev, float* den_dev, int32_t b, int32_t c, int32_t t, int32_t use_cfg,
                    float cfg_scale, float scale_phi, float c_out, float c_skip, sat_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Local-attention transformer codec.  Replaces models/local_attention.py:17-282 (ContinuousLocalTransformer without conditioning, cross-attention
 * or causal masking; TransformerDownsampleBlock1D / TransformerUpsampleBlock1D; TransformerEncoder1D / TransformerDecoder1D), the codec that
 * models/autoencoders.py:709-712, 735-738 select with "type": "local_attn".  One plan per encoder or decoder.
 *   encoder: x [b, in_channels, t] -> out [b, out_channels, t / prod(ratios)];  decoder: x [b, in_channels, t] -> out [b, out_channels, t * prod(ratios)].
 * Stage i runs depths[i] layers of embed_dims[i] channels in heads[i] heads, every self-attention over NATTEN's 1-D neighbourhood of `window` keys
 * with unscaled logits, behind a rotary embedding of max(dim_heads / 2, 32) channels; ff_inner[i] = int(embed_dims[i] * ff_mult) is the SwiGLU's
 * hidden width.  The residual stream is fp32; gemm_dtype SAT_GEMM_BF16 / SAT_GEMM_FP16 / SAT_GEMM_FP32X selects the operands of every GEMM and of
 * the attention inside the stages (the two projections at the audio boundary are fp32 in every build).
 * Tensors (sat_local_attn_plan_set_tensor, the reference's state-dict names, fp32): project_in.weight, project_out.weight and per stage
 * layers.<i>.{project_in.weight (where embed_dims[i - 1] != embed_dims[i]), project_down.weight | project_up.weight,
 * transformer.rotary_pos_emb.inv_freq, transformer.layers.<l>.{0.gamma, 0.beta, 1.to_qkv.weight, 1.to_out.weight, 3.gamma, 3.beta,
 * 4.ff.0.proj.weight, 4.ff.0.proj.bias, 4.ff.2.weight}}; finalize names a missing one with SAT_E_MISSING.
 * sat_local_attn_plan_create: cfg_bytes = sizeof(sat_local_attn_cfg) of the caller's header, any other size is SAT_E_INVALID, as is an even window
 * or one of 1 or less (NATTEN's rule).  SAT_E_UNSUPPORTED: a stage whose embed_dim / heads is not 32, 64, 96 or 128; 128 with SAT_GEMM_FP32X; an
 * embed_dim that is no multiple of 128 or an ff_inner that is no multiple of 64 (the GEMM launchers: N % 128, K % 64); in_channels above 128.
 * sat_local_attn_workspace_bytes / sat_local_attn_forward answer SAT_E_INVALID, before anything is launched, to an encoder input whose length is no
 * multiple of prod(ratios) and to a stage whose rows per item are fewer than `window`.  The output depends on the weights and the input alone: the
 * workspace may hold anything when the call starts. */
#define SAT_LOCAL_ATTN_MAX_STAGES 16
typedef struct sat_local_attn_plan sat_local_attn_plan;
typedef struct sat_local_attn_cfg {
    int32_t is_decoder;
    int32_t in_channels, out_channels;
    int32_t n_stages;
    int32_t embed_dims[SAT_LOCAL_ATTN_MAX_STAGES];
    int32_t heads[SAT_LOCAL_ATTN_MAX_STAGES];
    int32_t depths[SAT_LOCAL_ATTN_MAX_STAGES];
    int32_t ratios[SAT_LOCAL_ATTN_MAX_STAGES];
    int32_t ff_inner[SAT_LOCAL_ATTN_MAX_STAGES];
    int32_t window;
    int32_t gemm_dtype;
} sat_local_attn_cfg;
int sat_local_attn_plan_create(const sat_local_attn_cfg* cfg, size_t cfg_bytes, sat_local_attn_plan** out_plan);
void sat_local_attn_plan_destroy(sat_local_attn_plan* plan);
int sat_local_attn_plan_set_tensor(sat_local_attn_plan* plan, const char* name, const float* data_dev, int64_t numel);
int sat_local_attn_plan_finalize(sat_local_attn_plan* plan, sat_stream_t stream);
int sat_local_attn_workspace_bytes(const sat_local_attn_plan* plan, int32_t b, int32_t t, size_t* out_bytes);
int sat_local_attn_forward(sat_local_attn_plan* plan, const float* x_dev, float* out_dev, int32_t b, int32_t t, void* workspace_dev, size_t workspace_bytes,
                           sat_stream_t stream);
/* The two boundary kernels alone (tests/test_gpu_local_attn_kernels.py), fp32: rows [b * t, d] = x [b, c_in, t]^T w [d, c_in]^T (d % 4 == 0,
 * c_in <= 128) and out [b, c_out, t] = (rows [b * t, d] w [c_out, d]^T)^T (d % 64 == 0). */
int sat_local_attn_project_in(const float* x_dev, const float* w_dev, float* rows_dev, int32_t b, int32_t c_in, int32_t t, int32_t d, sat_stream_t stream);
int sat_local_attn_project_out(const float* rows_dev, const float* w_dev, float* out_dev, int32_t b, int32_t c_out, int32_t t, int32_t d,
                               sat_stream_t stream);

/* ---- The Dance Diffusion U-Net: DiffusionAttnUnet1D of the reference's models/diffusion.py:376-479 (ResConvBlock, SelfAttention1d, SkipBlock,
 * Downsample1d("cubic"), Upsample1d("cubic") of models/blocks.py), what create_model_from_config builds for "model_type": "diffusion_uncond" with
 * "type": "DAU1d".  out [b, io, t] = net(cat([x * in_scale, planes(FourierFeatures(1, 16)(t_in))])), fp32 in and out; in_scale is the c_in of a
 * v-objective denoiser (1 for the plain forward).  Activations are channel-last rows inside; the residual / skip stream, the GroupNorm
 * statistics, the softmax and the two boundary layers are fp32; gemm_dtype SAT_GEMM_BF16 / SAT_GEMM_FP16 / SAT_GEMM_FP32X selects the operands
 * of every convolution between them and of the attention.  Outputs are a function of the weights and the inputs alone: no atomics.
 * Tensors (sat_unet_plan_set_tensor, the reference's state-dict names, fp32): timestep_embed.weight and, under "net.", per ResConvBlock
 * main.{0,3}.{weight,bias} (no bias with conv_bias 0), main.{1,4}.{weight,bias} (none at main.4 of the last block), skip.weight where the widths
 * differ; per SelfAttention1d norm.{weight,bias}, qkv_proj.{weight,bias}, out_proj.{weight,bias}.  The resamplers' `kernel` buffers are not read:
 * the cubic filter is a constant of the kernels (the Python module refuses any other).  finalize names a missing tensor with SAT_E_MISSING.
 * sat_unet_plan_create: cfg_bytes = sizeof(sat_unet_cfg) of the caller's header, any other size is SAT_E_INVALID, as is depth < 2 (the reference
 * fails there).  SAT_E_UNSUPPORTED, each with its reason: use_snake, learned_resample, cond_dim > 0 or cond_noise_aug, a kernel_size outside
 * 1 / 3 / 5 / 7, a channels entry that is no multiple of 128, depth > SAT_UNET_MAX_DEPTH, io_channels + 16 > 128, SAT_GEMM_FP8.
 * sat_unet_workspace_bytes / sat_unet_forward answer SAT_E_INVALID, before anything is launched, to a t that is no multiple of 2^(depth - 1) or
 * leaves fewer than 3 rows at the deepest level (the reference fails in F.pad or torch.cat there). */
#define SAT_UNET_MAX_DEPTH 16
typedef struct sat_unet_plan sat_unet_plan;
typedef struct sat_unet_cfg {
    int32_t io_channels;
    int32_t depth;
    int32_t n_attn_layers;
    int32_t kernel_size;
    int32_t conv_bias;         /* 0 / 1 */
    int32_t cond_dim;          /* must be 0 */
    int32_t cond_noise_aug;    /* must be 0 */
    int32_t learned_resample;  /* must be 0 */
    int32_t use_snake;         /* must be 0 */
    int32_t gemm_dtype;
    int32_t channels[SAT_UNET_MAX_DEPTH];
} sat_unet_cfg;
int sat_unet_plan_create(const sat_unet_cfg* cfg, size_t cfg_bytes, sat_unet_plan** out_plan);
void sat_unet_plan_destroy(sat_unet_plan* plan);
int sat_unet_plan_set_tensor(sat_unet_plan* plan, const char* name, const float* data_dev, int64_t numel);
int sat_unet_plan_finalize(sat_unet_plan* plan, sat_stream_t stream);
int sat_unet_workspace_bytes(const sat_unet_plan* plan, int32_t b, int32_t t, size_t* out_bytes);
int sat_unet_forward(sat_unet_plan* plan, const float* x_dev, const float* t_dev, float in_scale, float* out_dev, int32_t b, int32_t t,
                     void* workspace_dev, size_t workspace_bytes, sat_stream_t stream);
/* The U-Net's own kernels alone (tests/test_gpu_unet_kernels.py); fmt is SAT_GEMM_BF16 / SAT_GEMM_FP16 / SAT_GEMM_FP32X, the element type of an
 * operand image (fp32 for the last).  Rows are [b * rows, c], one item is rows * c contiguous floats; pointers 16-byte aligned.
 * groupnorm_stats: stats [b][2] = (mean, 1 / sqrt(biased variance + eps)) over the n = rows * c elements of each item (n % 4 == 0); part_dev holds
 *   b * sat_unet_groupnorm_partials(n) * 2 floats of per-tile (mean, M2) partials, combined in a fixed order.
 * groupnorm_apply: y = act((x - mean) rstd gamma[ch] + beta[ch]) + skip, act 1 = GELU (erf form), 0 = none; skip may be NULL; y goes to out32
 *   [b * rows, c] and / or out_op [b * rows, ld] (either may be NULL; out32 may alias x or skip).
 * cast_rows: out_op [m, ld][:, :c] = x [m, c].
 * downsample: Downsample1d("cubic"), [b * s, c] -> [b * s / 2, c] (s even, s > 3), fp32 and / or operand image.
 * upsample: Upsample1d("cubic"), [b * s, c] -> out_op [b * 2 s, ld] (s > 2).
 * input: x [b, io, t] * in_scale and the 16 planes of FourierFeatures(t_in [b]; w_embed [8]) through w_main [c, io + 16, taps] (+ b_main or NULL,
 *   zero padding of the concatenated tensor) -> y [b * t, c], and through w_skip [c, io + 16] -> sk [b * t, c].
 * output: out [b, io, t] = conv(h [b * t, c], w_main [io, c, taps]) + b_main (or NULL) + xin [b * t, c] w_skip [io, c]^T (c % 64 == 0). */
int sat_unet_groupnorm_partials(int64_t n);
int sat_unet_groupnorm_stats(const float* x_dev, float* part_dev, float* stats_dev, int32_t b, int64_t n, float eps, sat_stream_t stream);
int sat_unet_groupnorm_apply(const float* x_dev, const float* stats_dev, const float* gamma_dev, const float* beta_dev, const float* skip_dev,
                             float* out32_dev, void* out_op_dev, int32_t b, int32_t rows, int32_t c, int32_t ld, int32_t act, int32_t fmt, sat_stream_t stream);
int sat_unet_cast_rows(const float* x_dev, void* out_op_dev, int64_t m, int32_t c, int32_t ld, int32_t fmt, sat_stream_t stream);
int sat_unet_downsample(const float* x_dev, float* out32_dev, void* out_op_dev, int32_t b, int32_t s, int32_t c, int32_t fmt, sat_stream_t stream);
int sat_unet_upsample(const float* x_dev, void* out_op_dev, int32_t b, int32_t s, int32_t c, int32_t ld, int32_t fmt, sat_stream_t stream);
int sat_unet_input(const float* x_dev, const float* t_dev, float in_scale, const float* w_embed_dev, const float* w_main_dev, const float* b_main_dev,
                   const float* w_skip_dev, float* y_dev, float* sk_dev, int32_t b, int32_t io, int32_t t, int32_t c, int32_t taps, sat_stream_t stream);
int sat_unet_output(const float* h_dev, const float* xin_dev, const float* w_main_dev, const float* b_main_dev, const float* w_skip_dev, float* out_dev,
                    int32_t b, int32_t io, int32_t t, int32_t c, int32_t taps, sat_stream_t stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* SAT_HIP_H */
