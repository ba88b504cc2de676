// DiT plan: owns the re-packed weights and drives one DiffusionTransformer forward
// (models/dit.py:135-226 + models/transformer.py:764-809, 656-702 of the reference) as a
// fixed sequence of HIP kernel launches on the caller's stream.  Host-side C++ only; the
// arithmetic lives in gemm_bf16.hip / attention.hip / layernorm.hip / dit_glue.hip.
#include <math.h>
#include <stddef.h>
#include <string.h>

#include <string>
#include <vector>

#include "dit_glue.h"
#include "sat_common.h"
#include "plan_core.h"

// ------------------------------------------------------------------------------ plan
namespace {

// One Linear of a block as its GEMM sees it.  The kind is decided once (proj_kind), written by pack_proj and read by every launch
enum ProjKind {
    PROJ_PLAIN,        // w: 16-bit [n, k] (bf16, or fp16 in the fp16 build)
    PROJ_LN_FOLD,      // w: 16-bit gamma (.) W of the LayerNorm in front, finished in the epilogue with c1 / c2 (GemmArgs::ln_c1 / ln_c2; the bias is in c2)
    PROJ_FP8_ROW,      // w: e4m3 bytes, scale per output channel; A: e4m3 with one scale per row, written by the quantising LayerNorm
    PROJ_FP8_MX,       // w: as above; A: MXFP8, E8M0 block scales written by A's producer (attention kernels, FF-in epilogue)
    PROJ_F32,          // w: the reference's own fp32 weights, no re-packing (fp32 verification mode, f32_ref.hip)
};
struct Proj {
    op_t* w = nullptr;
    int n = 0, k = 0;
    ProjKind kind = PROJ_PLAIN;
    int f16 = 0;          // 16-bit kinds: the operand format of its block (layer_f16), 1 = IEEE fp16
    int taps = 1;         // sat_dit_plan_set_ff_conv: w is the tap-major image [n, taps * k] of a Conv1d weight [n, k, taps] (pack_conv)
    bool nonorm = false;  // remove_norms: no LayerNorm in front, A is the residual row itself, rounded (Forward::layernorm)
    bool image = false;   // ... and that rounding is already in A: the 16-bit image the previous residual epilogue wrote under ln_fold
    float *scale = nullptr, *c1 = nullptr, *c2 = nullptr, *bias = nullptr;
};
enum ProjFamily { FAM_QKV, FAM_O, FAM_CQ, FAM_CKV, FAM_CO, FAM_FF1, FAM_FF2, FAM_CPW1, FAM_CGLU, FAM_CPW2 };      // the last three: the conformer's GEMMs

struct LayerW {
    float *pre_g, *pre_b, *cross_g, *cross_b, *ff_g, *ff_b;
    Proj qkv, o, cq, ckv, co, ff1, ff2;
    // ConformerModule (transformer.py:557-591): in_norm, pointwise_conv, glu.proj, depthwise_conv [D, 17] fp32, mid_norm, pointwise_conv_2
    float *cin_g = nullptr, *cin_b = nullptr, *cmid_g = nullptr, *cmid_b = nullptr, *cdw = nullptr;
    Proj cpw1, cglu, cpw2;
};

}  // namespace

struct sat_dit_plan {
    sat_dit_cfg cfg;
    TensorTable tensors;
    bool finalized = false;
    int inner = 0;          // FF inner dim
    int kvh_cross = 0;
    int hd = 64;            // channels per attention head, embed_dim / num_heads: 64, or 128 / 32 / 96 = the staged route (Forward::block)
    bool staged() const { return hd != 64; }
    DevBuf arena;
    std::vector<LayerW> layers;
    float *ts_w, *te0_w, *te0_b, *te2_w, *te2_b;
    float *ce0_w, *ce2_w, *ge0_w, *ge2_w;
    float *win_eff, *wout_eff;
    float *rope_cos, *rope_sin, *inv_freq;
    int f16 = 0;                    // cfg.gemm_dtype == 3: every 16-bit operand buffer holds IEEE fp16 and the fp16 build of the kernels runs
    std::vector<int> block_f16;     // sat_dit_plan_set_block_formats: the same per block (layer_f16); empty = f16 for every block
    bool cross_fusion = true;       // cfg.cross_attention == 0: to_q + cross-attention core in one launch where it applies
    int tile_bits = 0;              // cfg.tile_policy as GemmArgs::variant bits (sat_tile_policy_bits)
    bool ln_fold = false;           // cfg.ln_fold, bf16 / fp16 operands, "prepend" conditioning: LayerNorms run inside the GEMM epilogues
    int fp8_mode = 2;               // 2: v_mfma_scale_f32_32x32x64_f8f6f4 (unit scales, 2x rate); 1: v_mfma_f32_32x32x16_fp8_fp8
    int fp8_families = 0;           // gemm_dtype == 1: which GEMM families take e4m3 operands (sat_dit_cfg.fp8_families; SAT_FP8_* bits); 0 in every other mode
    float* ssg_w = nullptr;         // adaLN: [depth * 6D, D] stacked to_scale_shift_gate weights
    // input-concat / prepend conditioning (sat_dit_plan_set_extra_conditioning): win_eff then spans io_channels + concat_dim input channels
    int concat_dim = 0, prepend_dim = 0, max_prep = 0;
    float *pe0_w = nullptr, *pe2_w = nullptr;      // to_prepend_embed.0 / .2 (dit.py:160-165)
    // ContinuousTransformer switches off the shipped configs' path (sat_dit_plan_set_transformer_options); the defaults change nothing
    bool qk_norm = false;           // attn_kwargs qk_norm: q / k L2-normalised per head in the projections' epilogues (HeadsEpi::kind bit 4)
    int pos_emb = SAT_DIT_POS_NONE; // use_sinusoidal_emb / use_abs_pos_emb: pos_table is added to the stream behind the input projection
    int abs_max = 0;                // abs_pos_emb_max_length
    bool rotary = true;             // rotary_pos_emb=False: no inv_freq tensor, the rotation table is the identity (cos 1, sin 0)
    float* pos_table = nullptr;     // [pos_rows, D] fp32, position = row of the sequence (0 = first prepended row)
    int pos_rows = 0;
    // TransformerBlock options off the shipped configs' path (sat_dit_plan_set_block_options); the defaults change nothing
    bool conformer = false;         // x += conformer(x) behind the cross-attention update (Forward::conformer)
    bool remove_norms = false;      // pre_norm / cross_attend_norm / ff_norm are the identity (Proj::nonorm)
    bool ff_glu = true;             // false: ff.ff.0 is Linear + SiLU, FF-in runs with the plain-activation epilogue (EPI_ACT16)
    bool block_options() const { return conformer || remove_norms || !ff_glu; }
    // ff_kwargs use_conv (sat_dit_plan_set_ff_conv): kernel size of the feed-forward's convolutions, 1 = Linear and nothing changes
    int ff_conv = 1;
    bool ln_fold_asked = false;     // what sat_dit_plan_create made of cfg.ln_fold; ln_fold is this and ff_conv == 1
    // patch_size (sat_dit_plan_set_patch): latent frames per token, 1 = a token per frame and nothing changes.  t_len stays in frames at the
    // ABI; rows, workspace, position tables count tokens (tokens()), and the two boundary launches are those of dit_patch.hip
    int patch = 1;
    int tokens(int t_len) const { return t_len / patch; }
    // ContinuousTransformer causal (sat_dit_plan_set_attention_options): every self-attention runs the causal launchers; false changes nothing
    bool causal = false;
    // attn_kwargs natten_kernel_size (sat_dit_plan_set_neighborhood_attention): every self-attention sees a window of this many keys and its
    // logits are not scaled by 1 / sqrt(dim_heads) (attention_window.hip); 0 = full attention and nothing changes
    int natten = 0;
    // per-generation context (sat_dit_prepare_context)
    DevBuf ctx_buf;
    int ctx_bf = 0, ctx_lc = 0, ctx_lcpad = 0;
    bool has_global = false;
    int ctx_null_from = -1;         // sequences >= this index have an all-zero context (sat_dit_set_null_context_from)
    float* ge = nullptr;            // [bf, D] projected global embedding
    op_t* kc = nullptr;           // [depth][bf, kvh, lcpad, 64]
    op_t* vct = nullptr;          // [depth][bf, kvh, 64, lcpad]
    float* kc32 = nullptr;          // fp32 verification mode: [depth][bf, kvh, lc, 64]
    float* vc32 = nullptr;
    // per-generation extra conditioning (sat_dit_prepare_extra_conditioning); reset by every sat_dit_prepare_context
    DevBuf ext_buf;
    bool ext_ready = false;
    const float* ext_concat = nullptr;   // [ctx_bf, concat_dim, ext_concat_len] (a copy in ext_buf)
    int ext_concat_len = 0;
    float* ext_prep = nullptr;           // [ctx_bf, ctx_prep, D] to_prepend_embed(prepend_cond)
    int ctx_prep = 0;                    // P: prepend tokens of the prepared generation
    // sat_dit_workspace_bytes of a plan with prepend conditioning maximises over P = 0..max_prep: the last (bf, t_len) asked is cached
    mutable int wsq_bf = -1, wsq_t = -1;
    mutable size_t wsq_bytes = 0;
    // optional HIP-event timing of the FFN-in (SwiGLU) GEMM of one layer per forward (sat_dit_profile)
    bool prof_on = false;
    int prof_n = 0;
    std::vector<hipEvent_t> prof_ev;   // pairs
    long long prof_m = 0, prof_nn = 0, prof_k = 0;
    // optional diagnostics of the residual stream (sat_dit_debug): [depth][3 updates][4] floats, overwritten by every forward while enabled
    DevBuf dbg_buf;
    float* dbg = nullptr;
    // optional fp16 range report of the 16-bit buffers (sat_dit_range_report): [depth][SAT_DIT_RANGE_SLOTS] records, accumulated by every forward
    // and sat_dit_prepare_context while enabled, until reset or disabled
    DevBuf rr_buf;
    sat_range_record* rr = nullptr;
};
static const int kProfMaxPairs = 4096;

namespace {

// Slots of the range report per layer, in the order of sat_dit_range_slot_name
enum RangeSlot { RS_A_QKV, RS_Q, RS_K, RS_V, RS_ATTN_OUT, RS_A_CROSS_Q, RS_CROSS_Q, RS_CROSS_K, RS_CROSS_V, RS_CROSS_ATTN_OUT, RS_A_FF, RS_FF_HIDDEN };
const char* const kRangeSlotNames[SAT_DIT_RANGE_SLOTS] = {"a_qkv", "q", "k", "v", "attn_out", "a_cross_q", "cross_q", "cross_k", "cross_v",
                                                           "cross_attn_out", "a_ff", "ff_hidden"};

// Operand format of block l: every 16-bit buffer the block writes or reads (weight images, A / AO / Q / K / V^T / Hh, its slice of the
// cross-attention cache) holds IEEE fp16 (1) or bf16 (0).  The residual stream between blocks is fp32, so neighbours may differ
int layer_f16(const sat_dit_plan* p, int l) { return p->block_f16.empty() ? p->f16 : p->block_f16[l]; }

// One reduction of the range report over `scanned` contiguous 16-bit elements at buf, into slot `slot` of layer l; `logical` of them are values
// of the model (the rest: zero pads of the layout).  Launched right behind the buffer's producer: the next layer reuses the buffer.  Nothing
// without the report
int range_stats(const sat_dit_plan* p, int l, int slot, const op_t* buf, size_t scanned, size_t logical, hipStream_t s) {
    if (!p->rr) return 0;
    return sat_launch_range_stats(buf, layer_f16(p, l) ? SAT_GEMM_FP16 : SAT_GEMM_BF16, 1, (int64_t)scanned, (int64_t)scanned, logical,
                                  p->rr + (size_t)l * SAT_DIT_RANGE_SLOTS + slot, s);
}

// Rows of one sequence in the residual stream: [P prepend tokens | global token | T latent frames] (dit.py:185-197), no global
// token under adaLN (P is 0 there: sat_dit_plan_set_extra_conditioning rejects adaLN + prepend)
int seq_len(const sat_dit_plan* p, int T, int P) { return P + T + (p->cfg.adaln ? 0 : 1); }

int get_tensor(sat_dit_plan* p, const std::string& name, int64_t numel, const float** out) { return p->tensors.get("dit", name, numel, out); }

int copy_f32(sat_dit_plan* p, Bump& ar, const std::string& name, int64_t numel, float** dst, hipStream_t s) {
    return p->tensors.place("dit", ar, name, numel, dst, s);
}

// A projection into attention heads, the same on both routes: q / k / v of to_qkv, q of the cross to_q, k / v of to_kv.  `he` says where and in
// which form the parts go.  64-channel heads: the heads epilogue of the GEMM itself (one head = one 64-column wave tile, gemm_bf16.hip).  The
// staged route (128-, 32-, 96-channel heads): a plain fp32-output GEMM into `staging` [g.M, g.N], then the head split at the plan's width
// (head_split_hdw.hip: qk_norm, rotation, pre-scale, one rounding) over the `seqs` sequences of the rows
int project_heads(const sat_dit_plan* p, GemmArgs g, const HeadsEpi& he, float* staging, int seqs, hipStream_t s) {
    if (!p->staged()) {
        g.heads = he;
        return sat_launch_gemm(EPI_HEADS, g, s);
    }
    g.C = staging; g.ldc = g.N;
    SAT_TRY(sat_launch_gemm(EPI_F32, g, s));
    return sat_launch_head_split_hdw(staging, he, p->hd, seqs, s, g.f16);
}

// fp32 verification mode: the head split and the attention of f32_ref.hip at the plan's head width (64: the kernels without one; the causal
// kernel takes any).  rope_mask 0: no rotation
int split_heads_f32(const sat_dit_plan* p, const float* src, float* d0, float* d1, float* d2, int M, int S, int parts, int H, int rope_mask,
                    int norm_mask, hipStream_t s) {
    const float *rc = rope_mask ? p->rope_cos : nullptr, *rs = rope_mask ? p->rope_sin : nullptr;
    if (p->hd == 64) return sat_launch_split_heads_f32(src, d0, d1, d2, M, S, parts, H, rope_mask, rc, rs, s, norm_mask);
    return sat_launch_split_heads_f32_w(src, d0, d1, d2, M, S, parts, H, p->hd, rope_mask, rc, rs, s, norm_mask);
}
// self: the self-attention of a block (sq == sk), which a causal or a neighbourhood plan runs on its own kernel (never both: the setters refuse)
int attention_f32(const sat_dit_plan* p, bool self, const float* q, const float* k, const float* v, float* out, int b, int h, int kvh, int sq, int sk,
                  hipStream_t s) {
    if (self && p->causal) return sat_launch_attention_f32_causal(q, k, v, out, b, h, kvh, p->hd, sq, s);
    if (self && p->natten && p->hd != 64) return sat_launch_attention_f32_window_w(q, k, v, out, b, h, kvh, p->hd, sq, p->natten, 1.0f, s);
    if (self && p->natten) return sat_launch_attention_f32_window(q, k, v, out, b, h, kvh, sq, p->natten, 1.0f, s);      // unscaled logits
    if (p->hd == 64) return sat_launch_attention_f32(q, k, v, out, b, h, kvh, sq, sk, s);
    return sat_launch_attention_f32_w(q, k, v, out, b, h, kvh, p->hd, sq, sk, s);
}

// Whether A holds the 16-bit image of the residual rows (and ln_part their statistics) when the projection of `family` in layer l runs: under
// the fold, except for layer 0's to_qkv, whose pre_norm reads rows written by the input projection, not by a GEMM epilogue.  The same for the
// first block of another operand format: the image the previous FF-out's epilogue could write would be in the writer's format
bool has_image(const sat_dit_plan* p, ProjFamily family, int l) {
    const bool own_ln = family == FAM_QKV && (l == 0 || layer_f16(p, l) != layer_f16(p, l - 1));
    return p->ln_fold && !own_ln;
}
// remove_norms takes the LayerNorm from in front of the block's three projections; the conformer's in_norm stays
bool norm_removed(const sat_dit_plan* p, ProjFamily family) {
    return p->remove_norms && (family == FAM_QKV || family == FAM_CQ || family == FAM_FF1);
}
// How the Linear of `family` in layer `l` runs.  e4m3 by the plan's families (to_kv has no e4m3 form: once per generation); the fold for the
// LayerNorm-fed ones where A holds the image (has_image)
ProjKind proj_kind(const sat_dit_plan* p, ProjFamily family, int l) {
    static const int fp8_bit[] = {SAT_FP8_QKV, SAT_FP8_TO_OUT, SAT_FP8_CROSS_Q, 0, SAT_FP8_TO_OUT, SAT_FP8_FF_IN, SAT_FP8_FF_OUT, 0, 0, 0};
    const bool ln_fed = family == FAM_QKV || family == FAM_CQ || family == FAM_FF1 || family == FAM_CPW1;
    if (p->cfg.gemm_dtype == 2) return PROJ_F32;
    if (p->fp8_families & fp8_bit[family]) return ln_fed ? PROJ_FP8_ROW : PROJ_FP8_MX;
    if (norm_removed(p, family)) return PROJ_PLAIN;
    return ln_fed && has_image(p, family, l) ? PROJ_LN_FOLD : PROJ_PLAIN;
}

// Tensors `pf + weight` [n, k] and, where `bias` is given, `pf + bias` [n] into the arena in the form of the projection's kind.  interleave: the
// SwiGLU row order of the FF-in epilogue (weight rows, bias, c1 / c2; the fp32 mode keeps the reference's order).  gamma / beta: the LayerNorm
// in front, read under the fold
int pack_proj(sat_dit_plan* p, Bump& ar, const std::string& pf, const char* weight, const char* bias, ProjFamily family, int l, int n, int k,
              int interleave, const float* gamma, const float* beta, Proj* out, hipStream_t s) {
    Proj& r = *out;
    r = Proj{};
    r.n = n; r.k = k; r.kind = proj_kind(p, family, l); r.f16 = layer_f16(p, l);
    r.nonorm = norm_removed(p, family);
    r.image = r.nonorm && r.kind == PROJ_PLAIN && has_image(p, family, l);
    const bool fp8 = r.kind == PROJ_FP8_ROW || r.kind == PROJ_FP8_MX;
    r.w = (op_t*)ar.take((size_t)n * k * (r.kind == PROJ_F32 ? 4 : fp8 ? 1 : 2));
    if (fp8) r.scale = (float*)ar.take((size_t)n * 4);
    if (r.kind == PROJ_LN_FOLD) {
        r.c1 = (float*)ar.take((size_t)n * 4);
        r.c2 = (float*)ar.take((size_t)n * 4);
    }
    if (bias) r.bias = (float*)ar.take((size_t)n * 4);
    if (ar.dry()) return 0;
    const float *src, *b = nullptr;
    SAT_TRY(get_tensor(p, pf + weight, (int64_t)n * k, &src));
    if (bias) SAT_TRY(get_tensor(p, pf + bias, n, &b));
    if (r.kind == PROJ_F32) SAT_HIP(hipMemcpyAsync(r.w, src, (size_t)n * k * 4, hipMemcpyDeviceToDevice, s));
    else if (fp8) SAT_TRY(sat_launch_quant_rows_fp8(src, r.w, r.scale, n, k, interleave, s));
    else if (r.kind == PROJ_LN_FOLD) SAT_TRY(sat_launch_pack_rows_ln(src, gamma, beta, b, r.w, r.c1, r.c2, n, k, interleave, s, r.f16));
    else SAT_TRY(sat_launch_pack_rows_bf16(src, r.w, n, k, interleave, s, r.f16));
    if (!bias) return 0;
    if (interleave && r.kind != PROJ_F32) return sat_launch_pack_bias(b, r.bias, n, interleave, s);
    SAT_HIP(hipMemcpyAsync(r.bias, b, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
    return 0;
}

// A feed-forward Conv1d (ff_kwargs use_conv): `pf + weight` [n, k, taps] as the tap-major image [n, taps * k] in the block's format (fp32 in the
// verification mode), the operand of the contraction over taps row-shifted copies of A (ff_conv.hip); `pf + bias` [n] as it is.  No fold: the
// row statistics of the LayerNorm in front would differ per tap
int pack_conv(sat_dit_plan* p, Bump& ar, const std::string& pf, const char* weight, const char* bias, ProjFamily family, int l, int n, int k,
              Proj* out, hipStream_t s) {
    Proj& r = *out;
    r = Proj{};
    r.n = n; r.k = k; r.taps = p->ff_conv; r.f16 = layer_f16(p, l);
    r.kind = p->cfg.gemm_dtype == 2 ? PROJ_F32 : PROJ_PLAIN;
    r.nonorm = norm_removed(p, family);
    const size_t numel = (size_t)n * k * r.taps;
    r.w = (op_t*)ar.take(numel * (r.kind == PROJ_F32 ? 4 : 2));
    if (bias) r.bias = (float*)ar.take((size_t)n * 4);
    if (ar.dry()) return 0;
    const float *src, *b = nullptr;
    SAT_TRY(get_tensor(p, pf + weight, (int64_t)numel, &src));
    if (bias) SAT_TRY(get_tensor(p, pf + bias, n, &b));
    SAT_TRY(sat_launch_pack_conv_taps(src, r.w, n, k, r.taps, r.kind == PROJ_F32 ? SAT_GEMM_FP32X : r.f16 ? SAT_GEMM_FP16 : SAT_GEMM_BF16, s));
    if (bias) SAT_HIP(hipMemcpyAsync(r.bias, b, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
    return 0;
}

int build(sat_dit_plan* p, Bump& ar, hipStream_t s) {
    const sat_dit_cfg& c = p->cfg;
    const int D = c.embed_dim, C = c.io_channels, Dc = c.cond_embed_dim, Dct = c.cond_token_dim, Dg = c.global_cond_dim;
    const int inner = p->inner;
    SAT_TRY(copy_f32(p, ar, "timestep_features.weight", 128, &p->ts_w, s));
    SAT_TRY(copy_f32(p, ar, "to_timestep_embed.0.weight", (int64_t)D * 256, &p->te0_w, s));
    SAT_TRY(copy_f32(p, ar, "to_timestep_embed.0.bias", D, &p->te0_b, s));
    SAT_TRY(copy_f32(p, ar, "to_timestep_embed.2.weight", (int64_t)D * D, &p->te2_w, s));
    SAT_TRY(copy_f32(p, ar, "to_timestep_embed.2.bias", D, &p->te2_b, s));
    if (Dct > 0) {
        SAT_TRY(copy_f32(p, ar, "to_cond_embed.0.weight", (int64_t)Dc * Dct, &p->ce0_w, s));
        SAT_TRY(copy_f32(p, ar, "to_cond_embed.2.weight", (int64_t)Dc * Dc, &p->ce2_w, s));
    }
    if (Dg > 0) {
        SAT_TRY(copy_f32(p, ar, "to_global_embed.0.weight", (int64_t)D * Dg, &p->ge0_w, s));
        SAT_TRY(copy_f32(p, ar, "to_global_embed.2.weight", (int64_t)D * D, &p->ge2_w, s));
    }
    if (p->prepend_dim > 0) {
        SAT_TRY(copy_f32(p, ar, "to_prepend_embed.0.weight", (int64_t)D * p->prepend_dim, &p->pe0_w, s));
        SAT_TRY(copy_f32(p, ar, "to_prepend_embed.2.weight", (int64_t)D * D, &p->pe2_w, s));
    }
    // RotaryEmbedding(max(dim_heads / 2, 32)): 16 frequencies for 64-channel heads; 32 for 128-channel ones, 16 for 32 and 24 for 96 (the
    // staged route: its frequencies and table are placed at the end of build)
    const bool staged = p->staged();
    const int pairs = sat_rope_pairs(p->hd);
    auto place_inv_freq = [&]() -> int {
        if (p->rotary) return copy_f32(p, ar, "transformer.rotary_pos_emb.inv_freq", pairs, &p->inv_freq, s);
        // frequencies 0: the rotation table comes out as cos 1 / sin 0 and the rotating epilogues are the identity
        p->inv_freq = (float*)ar.take(pairs * 4);
        if (!ar.dry()) SAT_HIP(hipMemsetAsync(p->inv_freq, 0, pairs * 4, s));
        return 0;
    };
    auto take_rope_tables = [&](int rows) {      // [rows][pairs] each
        p->rope_cos = (float*)ar.take((size_t)rows * pairs * 4);
        p->rope_sin = (float*)ar.take((size_t)rows * pairs * 4);
    };
    if (!staged) SAT_TRY(place_inv_freq());
    const int Ci = C + p->concat_dim;       // preprocess_conv / project_in see cat([x, input_concat_cond]) (dit.py:38,130,173)
    const int pt = p->patch;                // project_in [D, Ci pt], project_out [C pt, D]; the two 1x1 convs stay per frame (dit.py:88-89,119-120)
    p->win_eff = (float*)ar.take((size_t)D * Ci * pt * 4);
    p->wout_eff = (float*)ar.take((size_t)D * C * pt * 4);
    const int smax = seq_len(p, p->tokens(c.max_seq_len), p->max_prep);
    if (!staged) take_rope_tables(smax);
    // the absolute table has abs_pos_emb_max_length rows and no more: run_forward refuses longer sequences as the reference does
    p->pos_rows = p->pos_emb == SAT_DIT_POS_ABSOLUTE && p->abs_max < smax ? p->abs_max : smax;
    p->pos_table = p->pos_emb != SAT_DIT_POS_NONE ? (float*)ar.take((size_t)p->pos_rows * D * 4) : nullptr;
    if (!ar.dry()) {
        const float *win, *wpre, *wout, *wpost;
        SAT_TRY(get_tensor(p, "transformer.project_in.weight", (int64_t)D * Ci * pt, &win));
        SAT_TRY(get_tensor(p, "preprocess_conv.weight", (int64_t)Ci * Ci, &wpre));
        SAT_TRY(get_tensor(p, "transformer.project_out.weight", (int64_t)D * C * pt, &wout));
        SAT_TRY(get_tensor(p, "postprocess_conv.weight", (int64_t)C * C, &wpost));
        if (pt > 1) {
            SAT_TRY(glue_fold_in_patch(win, wpre, p->win_eff, D, Ci, pt, s));
            SAT_TRY(glue_fold_out_patch(wout, wpost, p->wout_eff, D, C, pt, s));
        } else {
            SAT_TRY(glue_fold_in(win, wpre, p->win_eff, D, Ci, s));
            SAT_TRY(glue_fold_out(wout, wpost, p->wout_eff, D, C, s));
        }
        if (!staged) SAT_TRY(sat_launch_rope_table(p->inv_freq, p->rope_cos, p->rope_sin, smax, s));
        if (p->pos_emb == SAT_DIT_POS_SINUSOIDAL) {     // inv_freq is not in the state dict (persistent=False), the learnt scale is
            const float* sc;
            SAT_TRY(get_tensor(p, "transformer.pos_emb.scale", 1, &sc));
            SAT_TRY(glue_pos_table(1, sc, p->pos_table, p->pos_rows, D, s));
        } else if (p->pos_emb == SAT_DIT_POS_ABSOLUTE) {
            const float* ew;
            SAT_TRY(get_tensor(p, "transformer.pos_emb.emb.weight", (int64_t)p->abs_max * D, &ew));
            SAT_TRY(glue_pos_table(2, ew, p->pos_table, p->pos_rows, D, s));
        }
    }
    if (c.adaln) p->ssg_w = (float*)ar.take((size_t)c.depth * 6 * D * D * 4);
    p->layers.resize(c.depth);
    for (int l = 0; l < c.depth; ++l) {
        LayerW& L = p->layers[l];
        const std::string pf = "transformer.layers." + std::to_string(l) + ".";
        auto pack = [&](const char* weight, const char* bias, ProjFamily family, int n, int k, int interleave, const float* gamma, const float* beta, Proj* out) {
            return pack_proj(p, ar, pf, weight, bias, family, l, n, k, interleave, gamma, beta, out, s);
        };
        if (c.adaln && !ar.dry()) {   // transformer.py:651-655: Sequential(SiLU, Linear(D, 6D, bias=False)) -> key "...1.weight"
            SAT_TRY(p->tensors.copy("dit", pf + "to_scale_shift_gate.1.weight", (int64_t)6 * D * D, p->ssg_w + (size_t)l * 6 * D * D, s));
        }
        L.pre_g = L.pre_b = L.cross_g = L.cross_b = L.ff_g = L.ff_b = nullptr;      // remove_norms (transformer.py:621,632,642): nn.Identity, no tensors
        if (!p->remove_norms) {
            SAT_TRY(copy_f32(p, ar, pf + "pre_norm.gamma", D, &L.pre_g, s));
            SAT_TRY(copy_f32(p, ar, pf + "pre_norm.beta", D, &L.pre_b, s));
            SAT_TRY(copy_f32(p, ar, pf + "ff_norm.gamma", D, &L.ff_g, s));
            SAT_TRY(copy_f32(p, ar, pf + "ff_norm.beta", D, &L.ff_b, s));
        }
        SAT_TRY(pack("self_attn.to_qkv.weight", nullptr, FAM_QKV, 3 * D, D, 0, L.pre_g, L.pre_b, &L.qkv));
        SAT_TRY(pack("self_attn.to_out.weight", nullptr, FAM_O, D, D, 0, nullptr, nullptr, &L.o));
        if (Dct > 0) {
            if (!p->remove_norms) {
                SAT_TRY(copy_f32(p, ar, pf + "cross_attend_norm.gamma", D, &L.cross_g, s));
                SAT_TRY(copy_f32(p, ar, pf + "cross_attend_norm.beta", D, &L.cross_b, s));
            }
            SAT_TRY(pack("cross_attn.to_q.weight", nullptr, FAM_CQ, D, D, 0, L.cross_g, L.cross_b, &L.cq));
            SAT_TRY(pack("cross_attn.to_kv.weight", nullptr, FAM_CKV, 2 * Dc, Dc, 0, nullptr, nullptr, &L.ckv));
            SAT_TRY(pack("cross_attn.to_out.weight", nullptr, FAM_CO, D, D, 0, nullptr, nullptr, &L.co));
        }
        if (p->conformer) {      // (behind the attention tensors in the arena; a plan without the option places nothing here)
            SAT_TRY(copy_f32(p, ar, pf + "conformer.in_norm.gamma", D, &L.cin_g, s));
            SAT_TRY(copy_f32(p, ar, pf + "conformer.in_norm.beta", D, &L.cin_b, s));
            SAT_TRY(copy_f32(p, ar, pf + "conformer.mid_norm.gamma", D, &L.cmid_g, s));
            SAT_TRY(copy_f32(p, ar, pf + "conformer.mid_norm.beta", D, &L.cmid_b, s));
            SAT_TRY(copy_f32(p, ar, pf + "conformer.depthwise_conv.weight", (int64_t)D * 17, &L.cdw, s));
            SAT_TRY(pack("conformer.pointwise_conv.weight", nullptr, FAM_CPW1, D, D, 0, L.cin_g, L.cin_b, &L.cpw1));
            SAT_TRY(pack("conformer.glu.proj.weight", "conformer.glu.proj.bias", FAM_CGLU, 2 * D, D, 1, nullptr, nullptr, &L.cglu));
            SAT_TRY(pack("conformer.pointwise_conv_2.weight", nullptr, FAM_CPW2, D, D, 0, nullptr, nullptr, &L.cpw2));
        }
        // ff_kwargs glu=False (transformer.py:262-268): Sequential(Identity, Linear(D, inner, bias=not no_bias), Identity, SiLU) -> keys "ff.ff.0.1.*"
        // ff_kwargs use_conv (transformer.py:222,262-287): the output projection is Conv1d(inner, D, k), without GLU the input one Conv1d(D, inner, k)
        // under the same keys; GLU builds its own Linear and stays one
        const bool conv = p->ff_conv > 1;
        const char* b1 = p->tensors.has(pf + "ff.ff.0.1.bias") ? "ff.ff.0.1.bias" : nullptr;
        if (conv && !p->ff_glu)
            SAT_TRY(pack_conv(p, ar, pf, "ff.ff.0.1.weight", b1, FAM_FF1, l, inner, D, &L.ff1, s));
        else if (!p->ff_glu)
            SAT_TRY(pack("ff.ff.0.1.weight", p->tensors.has(pf + "ff.ff.0.1.bias") ? "ff.ff.0.1.bias" : nullptr, FAM_FF1, inner, D, 0, L.ff_g, L.ff_b, &L.ff1));
        else
            SAT_TRY(pack("ff.ff.0.proj.weight", "ff.ff.0.proj.bias", FAM_FF1, 2 * inner, D, 1, L.ff_g, L.ff_b, &L.ff1));
        // ff_kwargs no_bias (transformer.py:270): the output Linear of the feed-forward has no bias tensor; FF-out then runs without one
        const char* b2 = p->tensors.has(pf + "ff.ff.2.bias") ? "ff.ff.2.bias" : nullptr;
        if (conv) SAT_TRY(pack_conv(p, ar, pf, "ff.ff.2.weight", b2, FAM_FF2, l, D, inner, &L.ff2, s));
        else SAT_TRY(pack("ff.ff.2.weight", b2, FAM_FF2, D, inner, 0, nullptr, nullptr, &L.ff2));
    }
    if (staged) {      // behind everything a 64-channel plan places: the frequencies and the [smax][pairs] table the head split rotates with
        SAT_TRY(place_inv_freq());      // 32 pairs (128-channel heads), 16 (32), 24 (96)
        take_rope_tables(smax);
        if (!ar.dry()) SAT_TRY(sat_launch_rope_table_hdw(p->inv_freq, p->rope_cos, p->rope_sin, smax, p->hd, s));
    }
    return 0;
}

struct Workspace {
    float* X;
    op_t *A, *AO, *Q, *K, *Vt, *Hh;
    float *ff, *h1, *mo;
    float* As;              // gemm_dtype: per-row scale of the quantised LayerNorm output in A
    unsigned char* Hs;      // gemm_dtype: E8M0 block scales of the MXFP8 hidden activation in Hh, [M][inner / 32]
    unsigned char* AOs;     // gemm_dtype: E8M0 block scales of the MXFP8 attention output in AO, [M][D / 32]
    float *gsum, *ssg;      // adaLN: silu(global + timestep embed) [bf, D]; per-layer modulation [bf, depth, 6, D]
    float* ln_part = nullptr;    // ln_fold: [M][D / 64][2] partial (sum, sum of squares) of the bf16 image of X kept in A
    float* f32_wide = nullptr;   // fp32 verification mode: [M, max(3D, 2 inner)] GEMM output before the head split / SwiGLU
    float* slab = nullptr;       // K-split scratch of the 8-phase FF-out GEMM (GemmArgs::slab), present where that schedule splits
    size_t slab_bytes = 0;
    float* f32_col = nullptr;    // fp32 verification mode of a plan with sat_dit_plan_set_ff_conv: [M, taps * max(D, inner)] row gather in front of sat_gemm_f32
    float* qkv32 = nullptr;      // staged route (128-, 32-, 96-channel heads): [M, 3D] fp32 output of to_qkv / [Mc, D] of the cross to_q in front of the head split
    size_t qkv_bytes;
    size_t total;
};

Workspace carve(const sat_dit_plan* p, int bf, int T, int P, char* base) {
    const sat_dit_cfg& c = p->cfg;
    const int D = c.embed_dim, H = c.num_heads;
    const int S = seq_len(p, p->tokens(T), P);      // T: latent frames (w.mo below is [bf, io_channels, T]); rows are tokens
    const size_t M = (size_t)bf * S;
    const int Spad = (int)round_up(S + 3, 128);
    const int hid = p->conformer && D > p->inner ? D : p->inner;      // Hh: the FF hidden state [M, inner]; the conformer's GLU output [M, D] as well
    const bool f32 = c.gemm_dtype == 2, fp8 = c.gemm_dtype == 1;
    const size_t el = f32 ? 4 : 2;      // fp32 verification mode: every intermediate is fp32
    Workspace w;
    Bump ws{base};
    w.X = (float*)ws.take(M * D * 4);
    w.A = (op_t*)ws.take(M * D * el);
    w.AO = (op_t*)ws.take(M * D * el);
    // q / k / v: padded heads [bf, H, Spad, hd]; un-padded [bf, H, S, hd] in the fp32 mode.  Contiguous so that one memset clears all pads
    w.qkv_bytes = f32 ? M * D * 4 : (size_t)bf * H * Spad * p->hd * 2;
    w.Q = (op_t*)ws.take(w.qkv_bytes);
    w.K = (op_t*)ws.take(w.qkv_bytes);
    w.Vt = (op_t*)ws.take(w.qkv_bytes);
    w.Hh = (op_t*)ws.take(M * (size_t)hid * el);
    if (f32) w.f32_wide = (float*)ws.take(M * (size_t)(2 * p->inner > 3 * D ? 2 * p->inner : 3 * D) * 4);     // [M, 3D] qkv / [M, 2 inner] FF-in
    w.ff = (float*)ws.take((size_t)bf * 256 * 4);
    w.h1 = (float*)ws.take((size_t)bf * D * 4);
    w.mo = (float*)ws.take((size_t)bf * c.io_channels * T * 4);
    w.As = fp8 ? (float*)ws.take(M * 4) : nullptr;
    w.Hs = fp8 ? (unsigned char*)ws.take(M * (size_t)(p->inner / 32)) : nullptr;
    w.AOs = fp8 ? (unsigned char*)ws.take(M * (size_t)(D / 32)) : nullptr;
    w.gsum = c.adaln ? (float*)ws.take((size_t)bf * D * 4) : nullptr;
    w.ssg = c.adaln ? (float*)ws.take((size_t)bf * c.depth * 6 * D * 4) : nullptr;
    w.ln_part = p->ln_fold ? (float*)ws.take(M * (size_t)(D / 64) * 2 * 4) : nullptr;      // (16-bit plans only: sat_dit_plan_create_ex)
    // FF-out (K = inner) is the one fp32-output GEMM with a reduction long enough for the 8-phase kernel's K-split of the remainder
    // round (SA-2.0 shape): its slabs live here, per workspace = per caller and stream
    w.slab_bytes = (c.gemm_dtype == 0 || c.gemm_dtype == 3) ? sat_gemm_ph8_slab_bytes(EPI_RESID, (int)M, D, p->inner) : 0;
    w.slab = w.slab_bytes ? (float*)ws.take(w.slab_bytes) : nullptr;
    if (p->staged() && !f32) w.qkv32 = (float*)ws.take(M * (size_t)(3 * D) * 4);      // behind every buffer a 64-channel plan carves
    if (f32 && p->ff_conv > 1) w.f32_col = (float*)ws.take(M * (size_t)p->ff_conv * (p->inner > D ? p->inner : D) * 4);      // behind everything a Linear plan carves
    w.total = ws.off;
    return w;
}

// One forward's constants and the launches of one block on them (transformer.py:656-702)
struct Forward {
    sat_dit_plan* p;
    Workspace w;
    hipStream_t s;
    int bf, S, M, Spad, D, H;
    int bc, Mc;           // cross-attention runs on the first bc sequences (Mc rows): see block()
    int ssg_ld;           // per-sequence stride of the adaLN modulation vectors

    const float* mod(int l) const { return p->cfg.adaln ? w.ssg + (size_t)l * 6 * D : nullptr; }      // + {0..5} * D: scale1p / shift / gate of self, then of ff

    // The GemmArgs fields that follow from the projection's kind; the launch site adds what its epilogue needs
    GemmArgs gemm(const Proj& r, const op_t* A, int rows) const {
        GemmArgs g{};
        g.f16 = r.f16; g.variant = p->tile_bits;
        g.A = A; g.W = r.w; g.M = rows; g.N = r.n; g.K = r.k;
        g.bias = r.kind == PROJ_LN_FOLD ? nullptr : r.bias;          // the fold has it in c2
        if (r.kind == PROJ_LN_FOLD) { g.ln_part = w.ln_part; g.ln_c1 = r.c1; g.ln_c2 = r.c2; g.ln_eps = 1e-5f; }
        if (r.kind == PROJ_FP8_ROW) { g.fp8 = p->fp8_mode; g.a_scale = w.As; g.w_scale = r.scale; }
        // MXFP8 A: the E8M0 scales its producer wrote beside it (attention kernels: AOs, FF-in epilogue: Hs)
        if (r.kind == PROJ_FP8_MX) { g.fp8 = 3; g.a_bscale = (const unsigned*)(A == w.AO ? w.AOs : w.Hs); g.w_scale = r.scale; }
        return g;
    }

    // The standalone LayerNorm of X into A in front of a projection: quantising for e4m3 operands, none under the fold (from the first to_out
    // on, A holds the 16-bit image of X and ln_part its row statistics, both written by the epilogue of the GEMM that last updated X; the
    // LayerNorms of transformer.py:692, 695, 700 are finished in the epilogues of their consumers).  modulated: the adaLN form (sc / sh may be null)
    int layernorm(const Proj& r, const float* gamma, const float* beta, int rows, bool modulated, const float* sc, const float* sh) const {
        if (r.kind == PROJ_LN_FOLD) return 0;
        if (r.nonorm) {      // remove_norms: the rounded row (modulated under adaLN, transformer.py:672,686); under the fold A already holds it
            if (r.image) return 0;
            return sat_launch_round_rows(w.X, w.A, rows, D, modulated ? sc : nullptr, sh, S, ssg_ld, r.f16 ? SAT_GEMM_FP16 : SAT_GEMM_BF16, s);
        }
        if (r.kind == PROJ_FP8_ROW)
            return sat_launch_layernorm_fp8(w.X, gamma, beta, w.A, w.As, rows, D, sc, sh, modulated ? S : 1, modulated ? ssg_ld : 0, s);
        if (modulated) return sat_launch_layernorm_mod(w.X, gamma, beta, w.A, rows, D, sc, sh, S, ssg_ld, s, r.f16);
        return sat_launch_layernorm(w.X, gamma, beta, w.A, rows, D, s, r.f16);
    }

    // X += [gate (.)] (A W^T + bias), update `slot` (0 self-attention, 1 cross-attention, 2 feed-forward) of block l.  feeds_ln: a LayerNorm reads
    // the new rows, so under the fold the epilogue also writes their 16-bit image and statistics
    int resid(const Proj& r, const op_t* A, int rows, const float* gate, bool feeds_ln, int l, int slot) const {
        GemmArgs g = gemm(r, A, rows);
        g.C = w.X; g.ldc = D; g.accumulate = 1;
        if (gate) { g.gate = gate; g.gate_rows = S; g.gate_ld = ssg_ld; }
        if (slot == 2) { g.slab = w.slab; g.slab_bytes = w.slab_bytes; }          // FF-out: the one reduction long enough to split (carve)
        if (feeds_ln && p->ln_fold) { g.xb = w.A; g.ln_part_out = w.ln_part; }
        SAT_TRY(sat_launch_gemm(EPI_RESID, g, s));
        return p->dbg && slot >= 0 ? glue_resid_stats(w.X, rows, D, p->dbg + ((size_t)l * 3 + slot) * 4, s) : 0;      // (slot -1: the conformer's update, not in the table)
    }

    int range(int l, int slot, const op_t* buf, size_t scanned, size_t logical) const { return range_stats(p, l, slot, buf, scanned, logical, s); }
    // q / k / v of `seqs` sequences behind their head split: the scan covers the Spad - S zero pad rows of every head
    int range_heads(int l, int slot, const op_t* buf, int seqs) const {
        return range(l, slot, buf, (size_t)seqs * H * Spad * p->hd, (size_t)seqs * S * D);
    }

    // sat_dit_profile: the event pair round the FF-in launch of block depth / 2
    bool profiled(int l) const { return p->prof_on && l == p->cfg.depth / 2 && p->prof_n < kProfMaxPairs; }
    int prof_begin() const {
        if ((int)p->prof_ev.size() < 2 * (p->prof_n + 1)) {
            hipEvent_t e0, e1;
            SAT_HIP(hipEventCreate(&e0));
            SAT_HIP(hipEventCreate(&e1));
            p->prof_ev.push_back(e0);
            p->prof_ev.push_back(e1);
        }
        SAT_HIP(hipEventRecord(p->prof_ev[2 * p->prof_n], s));
        return 0;
    }
    int prof_end(long long m, long long n, long long k) const {      // the launch's GEMM shape
        SAT_HIP(hipEventRecord(p->prof_ev[2 * p->prof_n + 1], s));
        p->prof_n++;
        p->prof_m = m; p->prof_nn = n; p->prof_k = k;
        return 0;
    }

    // log2(e) / sqrt(dim_heads), what the projections pre-scale q by (HeadsEpi kind bit 3): the constant the 64-channel kernels were built with
    // A neighbourhood plan (any head width, no cross-attention) does not scale its logits: log2(e) alone
    float qscale() const { return p->natten ? 1.4426950408889634f : p->staged() ? sat_attn_qscale(p->hd) : SAT_ATTN_QSCALE; }
    // AO = softmax(q k^T) v for `seqs` sequences of S queries against sk keys (pad sk_pad) in kvh heads: attention.hip at 64 channels per head,
    // attention_hdw.hip at the staged widths; the causal kernels for the self-attention of a causal plan (sk == S; never an e4m3 plan), the window
    // kernels (attention_window.hip, attention_hdw_window.hip) for that of a neighbourhood plan (never causal, never e4m3).  `out`: the
    // projection that reads AO; as an MXFP8 operand the kernel writes its block scales beside it (64 channels only)
    int attend(const op_t* q, const op_t* k, const op_t* vt, int seqs, int kvh, int sk, int sk_pad, int f16, const Proj& out, bool self) const {
        const bool causal = self && p->causal;
        if (p->staged()) {
            if (causal) return sat_launch_attention_hdw_causal(q, k, vt, w.AO, seqs, H, kvh, p->hd, S, Spad, sk_pad, s, f16);
            // the head split wrote Q times log2(e) (qscale): the kernel has no scale of its own
            if (self && p->natten) return sat_launch_attention_hdw_window(q, k, vt, w.AO, seqs, H, kvh, p->hd, S, Spad, sk_pad, p->natten, s, f16);
            return sat_launch_attention_hdw(q, k, vt, w.AO, seqs, H, kvh, p->hd, S, sk, Spad, sk_pad, s, f16);
        }
        if (causal) return sat_launch_attention_causal(q, k, vt, w.AO, seqs, H, kvh, S, Spad, sk_pad, s, 1.0f, f16);
        // the projection wrote Q times log2(e) (qscale): the kernel multiplies its scores by 1
        if (self && p->natten) return sat_launch_attention_window(q, k, vt, w.AO, seqs, H, kvh, S, Spad, sk_pad, p->natten, 1.0f, s, f16);
        return sat_launch_attention(q, k, vt, w.AO, seqs, H, kvh, S, sk, Spad, sk_pad, s, out.kind == PROJ_FP8_MX ? w.AOs : nullptr, 1.0f, f16);
    }

    int block(int l) const;
    int block_f32(int l) const;
    int conformer(int l) const;
    int feed_forward(int l) const;
    int feed_forward_conv(int l) const;
};

// fp32 verification mode: the same block on f32_ref.hip, fp32 everywhere
int Forward::block_f32(int l) const {
    const LayerW& L = p->layers[l];
    const float* m = mod(l);
    const int inner = p->inner;
    float *A32 = (float*)w.A, *AO32 = (float*)w.AO, *Q32 = (float*)w.Q, *K32 = (float*)w.K, *V32 = (float*)w.Vt, *H32 = (float*)w.Hh;
    auto W32 = [](const Proj& r) { return (const float*)r.w; };
    // the LayerNorm in front of a projection, or under remove_norms the row itself (modulated under adaLN)
    auto norm = [&](const float* gamma, const float* beta, int rows, const float* sc, const float* sh, int rps, int ld) {
        if (p->remove_norms) return sat_launch_round_rows(w.X, A32, rows, D, sc, sh, rps, ld, SAT_GEMM_FP32X, s);
        return sat_launch_layernorm_f32(w.X, gamma, beta, A32, rows, D, sc, sh, rps, ld, s);
    };
    SAT_TRY(norm(L.pre_g, L.pre_b, M, m, m ? m + D : nullptr, S, ssg_ld));
    SAT_TRY(sat_launch_gemm_f32(A32, W32(L.qkv), nullptr, w.f32_wide, M, 3 * D, D, 3 * D, 0, nullptr, 1, 0, s));
    SAT_TRY(split_heads_f32(p, w.f32_wide, Q32, K32, V32, M, S, 3, H, 3, p->qk_norm ? 3 : 0, s));
    SAT_TRY(attention_f32(p, true, Q32, K32, V32, AO32, bf, H, H, S, S, s));
    SAT_TRY(sat_launch_gemm_f32(AO32, W32(L.o), nullptr, w.X, M, D, D, D, 1, m ? m + 2 * D : nullptr, S, ssg_ld, s));
    if (bc > 0) {
        SAT_TRY(norm(L.cross_g, L.cross_b, Mc, nullptr, nullptr, 1, 0));
        SAT_TRY(sat_launch_gemm_f32(A32, W32(L.cq), nullptr, w.f32_wide, Mc, D, D, D, 0, nullptr, 1, 0, s));
        const size_t per_layer = (size_t)bf * p->kvh_cross * p->ctx_lc * p->hd;
        SAT_TRY(split_heads_f32(p, w.f32_wide, Q32, nullptr, nullptr, Mc, S, 1, H, 0, p->qk_norm ? 1 : 0, s));
        SAT_TRY(attention_f32(p, false, Q32, p->kc32 + l * per_layer, p->vc32 + l * per_layer, AO32, bc, H, p->kvh_cross, S, p->ctx_lc, s));
        SAT_TRY(sat_launch_gemm_f32(AO32, W32(L.co), nullptr, w.X, Mc, D, D, D, 1, nullptr, 1, 0, s));
    }
    if (p->conformer) {      // transformer.py:680-681, 697-698 (the launches of Forward::conformer in fp32)
        SAT_TRY(sat_launch_layernorm_f32(w.X, L.cin_g, L.cin_b, A32, M, D, nullptr, nullptr, 1, 0, s));
        SAT_TRY(sat_launch_gemm_f32(A32, W32(L.cpw1), nullptr, AO32, M, D, D, D, 0, nullptr, 1, 0, s));
        SAT_TRY(sat_launch_gemm_f32(AO32, W32(L.cglu), L.cglu.bias, w.f32_wide, M, 2 * D, D, 2 * D, 0, nullptr, 1, 0, s));
        SAT_TRY(sat_launch_swiglu_f32(w.f32_wide, H32, M, D, s));
        SAT_TRY(sat_launch_dwconv_ln_silu(H32, L.cdw, L.cmid_g, L.cmid_b, AO32, bf, S, D, SAT_GEMM_FP32X, s));
        SAT_TRY(sat_launch_gemm_f32(AO32, W32(L.cpw2), nullptr, w.X, M, D, D, D, 1, nullptr, 1, 0, s));
    }
    SAT_TRY(norm(L.ff_g, L.ff_b, M, m ? m + 3 * D : nullptr, m ? m + 4 * D : nullptr, S, ssg_ld));
    const int taps = p->ff_conv;
    if (!p->ff_glu && taps > 1) {      // Conv1d(D, inner, k) + SiLU: the rows of the window gathered side by side, then the same GEMM at K = k D
        SAT_TRY(sat_launch_im2col_rows_f32(A32, w.f32_col, bf, S, D, taps, s));
        SAT_TRY(sat_launch_gemm_f32(w.f32_col, W32(L.ff1), L.ff1.bias, H32, M, inner, taps * D, inner, 0, nullptr, 1, 0, s));
        SAT_TRY(sat_launch_silu_f32(H32, (int64_t)M * inner, s));
    } else if (!p->ff_glu) {      // Linear + SiLU
        SAT_TRY(sat_launch_gemm_f32(A32, W32(L.ff1), L.ff1.bias, H32, M, inner, D, inner, 0, nullptr, 1, 0, s));
        SAT_TRY(sat_launch_silu_f32(H32, (int64_t)M * inner, s));
    } else {
        SAT_TRY(sat_launch_gemm_f32(A32, W32(L.ff1), L.ff1.bias, w.f32_wide, M, 2 * inner, D, 2 * inner, 0, nullptr, 1, 0, s));
        SAT_TRY(sat_launch_swiglu_f32(w.f32_wide, H32, M, inner, s));
    }
    if (taps > 1) {
        SAT_TRY(sat_launch_im2col_rows_f32(H32, w.f32_col, bf, S, inner, taps, s));
        return sat_launch_gemm_f32(w.f32_col, W32(L.ff2), L.ff2.bias, w.X, M, D, taps * inner, D, 1, m ? m + 5 * D : nullptr, S, ssg_ld, s);
    }
    return sat_launch_gemm_f32(H32, W32(L.ff2), L.ff2.bias, w.X, M, D, inner, D, 1, m ? m + 5 * D : nullptr, S, ssg_ld, s);
}

// The two attention branches, the conformer and the feed-forward of one block.  The branches are the same launches at every head width but for
// the projections into heads (project_heads) and the attention kernel (attend): the staged widths (128, 32, 96) take two more launches and one
// fp32 round trip through qkv32 per attention than the 64-channel route, and neither the fused to_q + cross-attention launch nor the fold
int Forward::block(int l) const {
    const LayerW& L = p->layers[l];
    const float* m = mod(l);
    const int f16 = L.qkv.f16, qn = p->qk_norm ? 16 : 0;      // HeadsEpi::kind bit 4 on the q / k parts
    // ---- self-attention branch (transformer.py:692)
    SAT_TRY(layernorm(L.qkv, L.pre_g, L.pre_b, M, true, m, m ? m + D : nullptr));
    SAT_TRY(range(l, RS_A_QKV, w.A, (size_t)M * D, (size_t)M * D));
    HeadsEpi he{};
    he.out[0] = w.Q; he.out[1] = w.K; he.out[2] = w.Vt;
    he.kind[0] = 2 | 8 | qn; he.kind[1] = 2 | 4 | qn; he.kind[2] = 1 | 4; he.qscale = qscale();
    he.parts = 3; he.heads = H; he.S = S; he.Spad = Spad;
    he.rope_cos = p->rope_cos; he.rope_sin = p->rope_sin;
    SAT_TRY(project_heads(p, gemm(L.qkv, w.A, M), he, w.qkv32, bf, s));
    SAT_TRY(range_heads(l, RS_Q, w.Q, bf));
    SAT_TRY(range_heads(l, RS_K, w.K, bf));
    SAT_TRY(range_heads(l, RS_V, w.Vt, bf));
    SAT_TRY(attend(w.Q, w.K, w.Vt, bf, H, S, Spad, f16, L.o, true));
    SAT_TRY(range(l, RS_ATTN_OUT, w.AO, (size_t)M * D, (size_t)M * D));
    SAT_TRY(resid(L.o, w.AO, M, m ? m + 2 * D : nullptr, true, l, 0));
    // ---- cross-attention branch (transformer.py:694-695).  Sequences whose context is all-zero (the
    // unconditional CFG half, dit.py:294-300) get k = v = 0 from the bias-free to_cond_embed / to_kv, hence an
    // attention output of exactly 0 and, through the bias-free to_out, a branch contribution of exactly 0:
    // the branch runs only on the first `bc` sequences (rows are ordered by sequence).
    if (bc > 0) {
        SAT_TRY(layernorm(L.cq, L.cross_g, L.cross_b, Mc, false, nullptr, nullptr));
        SAT_TRY(range(l, RS_A_CROSS_Q, w.A, (size_t)Mc * D, (size_t)Mc * D));
        he = HeadsEpi{};
        he.out[0] = w.Q; he.kind[0] = 8 | qn; he.qscale = qscale();
        he.parts = 1; he.heads = H; he.S = S; he.Spad = Spad;
        const size_t per_layer = (size_t)bf * p->kvh_cross * p->ctx_lcpad * p->hd;
        const op_t *kc = p->kc + l * per_layer, *vct = p->vct + l * per_layer;
        // One launch for to_q + softmax(q k^T) v where the 128 x 64 tile is the choice anyway and its workgroups fit one round
        // (one prompt: 9 x 24 = 216): the projection's epilogue keeps Q in registers and attends to the <= 189 context keys
        // staged in LDS (gemm_bf16.hip, XA_OK).  Saves the attention launch and the Q round trip.  16-bit operands, 64-channel heads only.
        const bool fuse = !p->staged() && p->cross_fusion && L.cq.kind != PROJ_FP8_ROW && L.co.kind != PROJ_FP8_MX && D >= 192 &&
                          p->ctx_lc + 3 <= 192 && cdiv(Mc, 128) * (D / 64) <= 256;
        if (fuse) {
            he.xa_k = kc; he.xa_vt = vct; he.xa_out = w.AO;
            he.xa_kvh = p->kvh_cross; he.xa_sk = p->ctx_lc; he.xa_sk_pad = p->ctx_lcpad;
        }
        SAT_TRY(project_heads(p, gemm(L.cq, w.A, Mc), he, w.qkv32, bc, s));
        if (!fuse) {      // (the fused launch keeps Q in registers: its slot of the range report stays empty)
            SAT_TRY(range_heads(l, RS_CROSS_Q, w.Q, bc));
            SAT_TRY(attend(w.Q, kc, vct, bc, p->kvh_cross, p->ctx_lc, p->ctx_lcpad, f16, L.co, false));
        }
        SAT_TRY(range(l, RS_CROSS_ATTN_OUT, w.AO, (size_t)Mc * D, (size_t)Mc * D));
        SAT_TRY(resid(L.co, w.AO, Mc, nullptr, true, l, 1));
    }
    if (p->conformer) SAT_TRY(conformer(l));      // (64-channel heads only: sat_dit_plan_set_block_options)
    return feed_forward(l);
}

// ---- conformer branch (transformer.py:680-681, 697-698; ConformerModule :576-591): x += conformer(x) on every sequence, not modulated by adaLN.
// in_norm + pointwise_conv as one LayerNorm-fed GEMM with a 16-bit output (the fold applies as for to_qkv), glu as the FF-in SwiGLU GEMM at
// inner dim D on that 16-bit output (the reference rounds between the two), depthwise_conv + mid_norm + SiLU in one pass, pointwise_conv_2 with
// the residual epilogue of to_out.  Buffers: A -> AO -> Hh -> AO -> X
int Forward::conformer(int l) const {
    const LayerW& L = p->layers[l];
    const int f16 = L.cpw1.f16;
    SAT_TRY(layernorm(L.cpw1, L.cin_g, L.cin_b, M, false, nullptr, nullptr));
    GemmArgs g = gemm(L.cpw1, w.A, M);
    g.H = w.AO; g.act = 0;
    SAT_TRY(sat_launch_gemm(EPI_ACT16, g, s));
    g = gemm(L.cglu, w.AO, M);
    g.H = w.Hh;
    SAT_TRY(sat_launch_gemm(EPI_SWIGLU, g, s));
    SAT_TRY(sat_launch_dwconv_ln_silu(w.Hh, L.cdw, L.cmid_g, L.cmid_b, w.AO, bf, S, D, f16 ? SAT_GEMM_FP16 : SAT_GEMM_BF16, s));
    return resid(L.cpw2, w.AO, M, nullptr, true, l, -1);
}

// ---- feed-forward branch of a plan with sat_dit_plan_set_ff_conv (ff_kwargs use_conv, transformer.py:211-287): the standalone LayerNorm (or
// the rounded row) into A; FF-in as the Linear SwiGLU GEMM under GLU, else the convolution GEMM with the SiLU epilogue; FF-out as the
// convolution GEMM with the residual epilogue (bias, adaLN gate, += into the fp32 stream).  A -> Hh -> X, the dense buffers of the Linear plan:
// ff_conv.hip tests the sequence boundary where it stages a row
int Forward::feed_forward_conv(int l) const {
    const LayerW& L = p->layers[l];
    const float* m = mod(l);
    SAT_TRY(layernorm(L.ff1, L.ff_g, L.ff_b, M, true, m ? m + 3 * D : nullptr, m ? m + 4 * D : nullptr));
    FfConvArgs a{};
    a.fmt = L.ff2.f16 ? SAT_GEMM_FP16 : SAT_GEMM_BF16;
    a.B = bf; a.S = S; a.taps = p->ff_conv;
    const bool prof = profiled(l);
    if (prof) SAT_TRY(prof_begin());
    if (p->ff_glu) {
        GemmArgs g = gemm(L.ff1, w.A, M);
        g.H = w.Hh;
        SAT_TRY(sat_launch_gemm(EPI_SWIGLU, g, s));
        if (prof) SAT_TRY(prof_end(g.M, g.N, g.K));
    } else {
        a.A = w.A; a.W = L.ff1.w; a.bias = L.ff1.bias; a.N = L.ff1.n; a.K = L.ff1.k;
        a.epi = FFC_ACT16; a.H = w.Hh; a.act = 1;
        SAT_TRY(sat_launch_ff_conv(a, s));
        if (prof) SAT_TRY(prof_end(M, a.N, (long long)a.taps * a.K));      // the contraction runs over taps * K
    }
    a.A = w.Hh; a.W = L.ff2.w; a.bias = L.ff2.bias; a.N = L.ff2.n; a.K = L.ff2.k;
    a.epi = FFC_RESID; a.H = nullptr; a.act = 0; a.C = w.X; a.ldc = D; a.accumulate = 1;
    if (m) { a.gate = m + 5 * D; a.gate_rows = S; a.gate_ld = ssg_ld; }
    SAT_TRY(sat_launch_ff_conv(a, s));
    return p->dbg ? glue_resid_stats(w.X, M, D, p->dbg + ((size_t)l * 3 + 2) * 4, s) : 0;
}

// ---- feed-forward branch (transformer.py:700)
int Forward::feed_forward(int l) const {
    if (p->ff_conv > 1) return feed_forward_conv(l);
    const LayerW& L = p->layers[l];
    const float* m = mod(l);
    SAT_TRY(layernorm(L.ff1, L.ff_g, L.ff_b, M, true, m ? m + 3 * D : nullptr, m ? m + 4 * D : nullptr));
    SAT_TRY(range(l, RS_A_FF, w.A, (size_t)M * D, (size_t)M * D));
    GemmArgs g = gemm(L.ff1, w.A, M);
    g.H = w.Hh;
    if (L.ff2.kind == PROJ_FP8_MX) { g.H8 = (unsigned char*)w.Hh; g.Hs = w.Hs; }          // FF-out's MXFP8 operand; otherwise the e4m3 GEMM writes a 16-bit hidden state
    const bool prof = profiled(l);
    if (prof) SAT_TRY(prof_begin());
    if (!p->ff_glu) g.act = 1;      // ff_kwargs glu=False: H [M, inner] = silu(A W^T + bias)
    SAT_TRY(sat_launch_gemm(p->ff_glu ? EPI_SWIGLU : EPI_ACT16, g, s));
    if (prof) SAT_TRY(prof_end(g.M, g.N, g.K));
    SAT_TRY(range(l, RS_FF_HIDDEN, w.Hh, (size_t)M * p->inner, (size_t)M * p->inner));
    // nobody normalises the output of the last block, and a next block of another format normalises the fp32 rows itself (proj_kind)
    const bool feeds_ln = l + 1 < p->cfg.depth && layer_f16(p, l + 1) == layer_f16(p, l);
    return resid(L.ff2, w.Hh, M, m ? m + 5 * D : nullptr, feeds_ln, l, 2);
}

int run_forward(sat_dit_plan* p, const float* x, int xB, float xscale, const float* t_dev, float t_const, float* out, int bf,
                int T, void* ws, size_t ws_bytes, hipStream_t s) {
    SAT_CHECK_ARG(p && p->finalized, SAT_E_STATE, "dit forward: plan not finalized");
    const sat_dit_cfg& c = p->cfg;
    SAT_CHECK_ARG(x && out && ws && bf > 0 && T > 0, SAT_E_INVALID, "dit forward: bad arguments");
    SAT_CHECK_ARG(T <= c.max_seq_len, SAT_E_INVALID, "dit forward: t_len %d exceeds plan max_seq_len %d", T, c.max_seq_len);
    SAT_CHECK_ARG(T % p->patch == 0, SAT_E_INVALID, "dit forward: t_len %d is not a multiple of patch_size %d", T, p->patch);
    SAT_CHECK_ARG(((uintptr_t)ws & 255) == 0, SAT_E_INVALID, "dit forward: workspace must be 256-byte aligned");
    const bool cross = c.cond_token_dim > 0;
    SAT_CHECK_ARG(p->ctx_bf == bf, SAT_E_STATE, "dit forward: context prepared for %d sequences, forward called with %d",
                  p->ctx_bf, bf);
    SAT_CHECK_ARG(p->concat_dim == 0 || p->ext_ready, SAT_E_STATE,
                  "dit forward: the model has input_concat_dim %d: sat_dit_prepare_extra_conditioning must follow sat_dit_prepare_context", p->concat_dim);
    const int P = p->ctx_prep;
    Workspace w = carve(p, bf, T, P, (char*)ws);
    SAT_CHECK_ARG(ws_bytes >= w.total, SAT_E_WORKSPACE, "dit forward: workspace %zu < required %zu", ws_bytes, w.total);
    const int D = c.embed_dim, H = c.num_heads, C = c.io_channels;
    const bool adaln = c.adaln != 0, f32 = c.gemm_dtype == 2;
    const int S = seq_len(p, p->tokens(T), P), M = bf * S, Spad = (int)round_up(S + 3, 128);
    const int ssg_ld = c.depth * 6 * D;      // per-sequence stride of the adaLN modulation vectors
    // transformer.py:59-61, before anything is launched
    SAT_CHECK_ARG(p->pos_emb != SAT_DIT_POS_ABSOLUTE || S <= p->abs_max, SAT_E_INVALID,
                  "dit forward: you are passing in a sequence length of %d but your absolute positional embedding has a max sequence length of %d", S,
                  p->abs_max);
    // what NATTEN rejects, before anything is launched: the window does not fit the rows the blocks see
    SAT_CHECK_ARG(!p->natten || S >= p->natten, SAT_E_INVALID,
                  "dit forward: a sequence of %d rows (prepend rows + global token + tokens) is shorter than natten_kernel_size %d", S, p->natten);

    // pads of q/k/vt must be finite (zero): one memset per forward
    if (!f32) SAT_HIP(hipMemsetAsync(w.Q, 0, 3 * (size_t)round_up((int64_t)w.qkv_bytes, 256), s));

    // timestep embedding (dit.py:176) + global embed (dit.py:179-182) -> global token rows X[b,P,:] (behind the P prepend tokens)
    SAT_TRY(glue_fourier(t_dev, t_const, p->ts_w, w.ff, bf, 128, s));
    SAT_TRY(glue_small_linear(w.ff, 256, p->te0_w, p->te0_b, nullptr, 0, w.h1, D, bf, D, 256, 1, 0, s));
    if (!adaln) {
        SAT_TRY(glue_small_linear(w.h1, D, p->te2_w, p->te2_b, p->has_global ? p->ge : nullptr, D, w.X + (size_t)P * D, S * D, bf, D, D, 0, 0, s));
    } else {
        // dit.py:205-206: the summed embedding conditions every block instead of being prepended; transformer.py:667:
        // (scale, shift, gate) x (self, ff) = Linear(SiLU(global)) for all layers in one launch
        SAT_TRY(glue_small_linear(w.h1, D, p->te2_w, p->te2_b, p->has_global ? p->ge : nullptr, D, w.gsum, D, bf, D, D, 2, 0, s));
        SAT_TRY(glue_small_linear(w.gsum, D, p->ssg_w, nullptr, nullptr, 0, w.ssg, ssg_ld, bf, ssg_ld, D, 0, 0, s));
        SAT_TRY(glue_adaln_finish(w.ssg, (int64_t)bf * ssg_ld, D, s));
    }
    // preprocess_conv + residual + project_in (dit.py:197-199, transformer.py:778); with extra conditioning the same launch adds the
    // concat channels (dit.py:167-173, unscaled by c_in) and copies the prepared prepend rows X[b, 0..P-1, :]
    if (p->patch > 1)      // "b (t p) c -> b t (c p)" in front of project_in: one launch for the plain model and the extra conditioning
        SAT_TRY(glue_input_proj_patch(x, p->win_eff, w.X, bf, xB, C, p->patch, T, S, D, xscale, p->ext_ready ? p->ext_concat : nullptr,
                                      p->ext_ready ? p->concat_dim : 0, p->ext_concat_len, p->ext_ready ? p->ext_prep : nullptr, p->ext_ready ? P : 0, s));
    else if (p->ext_ready)
        SAT_TRY(glue_input_proj_extra(x, p->win_eff, w.X, bf, xB, C, T, S, D, xscale, p->ext_concat, p->concat_dim, p->ext_concat_len,
                                      p->ext_prep, P, s));
    else
        SAT_TRY(glue_input_proj(x, p->win_eff, w.X, bf, xB, C, T, S, D, xscale, s));
    // transformer.py:796-797: x + pos_emb(x) on every row behind project_in and the prepend concat; block 0's LayerNorm reads X itself
    if (p->pos_table) SAT_TRY(glue_add_pos(w.X, p->pos_table, bf, S, D, s));

    if (p->dbg) SAT_HIP(hipMemsetAsync(p->dbg, 0, (size_t)c.depth * 3 * 4 * sizeof(float), s));
    // cross-attention: not on the sequences behind ctx_null_from (Forward::block)
    const int bc = !cross ? 0 : (p->ctx_null_from >= 0 && p->ctx_null_from < bf) ? p->ctx_null_from : bf;
    const Forward f{p, w, s, bf, S, M, Spad, D, H, bc, bc * S, ssg_ld};
    for (int l = 0; l < c.depth; ++l) SAT_TRY(f32 ? f.block_f32(l) : f.block(l));
    // project_out + drop prepend + postprocess_conv + residual (transformer.py:807, dit.py:219-224)
    if (p->patch > 1) SAT_TRY(glue_output_proj_patch(w.X, p->wout_eff, out, bf, C, p->patch, T, S, D, s));      // + "b (c p) t -> b c (t p)"
    else SAT_TRY(glue_output_proj(w.X, p->wout_eff, out, bf, C, T, S, D, s));
    return 0;
}

}  // namespace

// ------------------------------------------------------------------------------ C ABI
extern "C" int sat_dit_plan_create(const sat_dit_cfg* cfg, sat_dit_plan** out_plan) {
    return sat_dit_plan_create_sized(cfg, SAT_DIT_CFG_BYTES_V5, out_plan);
}

extern "C" int sat_dit_plan_create_sized(const sat_dit_cfg* cfg_in, size_t cfg_bytes, sat_dit_plan** out_plan) {
    return sat_dit_plan_create_ex(cfg_in, cfg_bytes, nullptr, 0, out_plan);
}

extern "C" int sat_dit_plan_create_ex(const sat_dit_cfg* cfg_in, size_t cfg_bytes, const sat_dit_create_options* options, size_t options_bytes,
                                      sat_dit_plan** out_plan) {
    SAT_CHECK_ARG(cfg_in && out_plan, SAT_E_INVALID, "dit_plan_create: null argument");
    sat_dit_create_options opt{};
    if (options) {
        SAT_CHECK_ARG(options_bytes == sizeof(sat_dit_create_options), SAT_E_INVALID,
                      "dit_plan_create_ex: options_bytes %zu is not the size of this version's sat_dit_create_options (%zu)", options_bytes,
                      sizeof(sat_dit_create_options));
        opt = *options;
        SAT_CHECK_ARG(opt.head_widths == 0 || opt.head_widths == 1, SAT_E_INVALID, "dit_plan_create_ex: head_widths must be 0 (64 / 128) or 1 (32 and 96 as well)");
    }
    static_assert(sizeof(sat_dit_cfg) == SAT_DIT_CFG_BYTES_V5, "sat_dit_cfg layout");
    // (the one layout this library knows; when the struct grows again, the older sizes are accepted here and the fields behind them defaulted)
    SAT_CHECK_ARG(cfg_bytes == sizeof(sat_dit_cfg), SAT_E_INVALID, "dit_plan_create: sat_dit_cfg of %zu bytes; this library (ABI version %d) knows %zu",
                  cfg_bytes, sat_version(), sizeof(sat_dit_cfg));
    sat_dit_cfg cfg_local{};
    memcpy(&cfg_local, cfg_in, cfg_bytes);
    const sat_dit_cfg* cfg = &cfg_local;
    SAT_CHECK_ARG(cfg->embed_dim > 0 && cfg->num_heads > 0 && (cfg->embed_dim == cfg->num_heads * 64 || cfg->embed_dim == cfg->num_heads * 128 ||
                                                               (opt.head_widths && (cfg->embed_dim == cfg->num_heads * 32 || cfg->embed_dim == cfg->num_heads * 96))),
                  SAT_E_UNSUPPORTED, "dit_plan_create: dim_heads must be 64 or 128%s (embed_dim %d, heads %d)",
                  opt.head_widths ? ", 32 or 96" : "; 32 and 96 through sat_dit_plan_create_ex with head_widths 1", cfg->embed_dim, cfg->num_heads);
    const int hd = cfg->embed_dim / cfg->num_heads;
    const bool hdw = hd == 32 || hd == 96;
    SAT_CHECK_ARG(cfg->embed_dim % 128 == 0 && cfg->embed_dim <= 2048, SAT_E_UNSUPPORTED,
                  "dit_plan_create: embed_dim %d must be a multiple of 128 and <= 2048", cfg->embed_dim);
    // (the input / output projection kernels move 4 channels per lane: glue_output_proj checks the same at forward time)
    SAT_CHECK_ARG(cfg->io_channels > 0 && cfg->io_channels <= 64 && cfg->io_channels % 4 == 0, SAT_E_UNSUPPORTED,
                  "dit_plan_create: io_channels %d must be a multiple of 4 in 4..64", cfg->io_channels);
    SAT_CHECK_ARG(cfg->depth > 0 && cfg->max_seq_len > 0, SAT_E_INVALID, "dit_plan_create: depth/max_seq_len must be positive");
    if (cfg->cond_token_dim > 0) {
        SAT_CHECK_ARG(cfg->cond_embed_dim % hd == 0 && cfg->cond_embed_dim > 0 && cfg->cond_token_dim % 4 == 0, SAT_E_UNSUPPORTED,
                      "dit_plan_create: cond_embed_dim %d must be a multiple of %d", cfg->cond_embed_dim, hd);
        int kvh = cfg->cond_embed_dim / hd;
        SAT_CHECK_ARG(cfg->num_heads % kvh == 0, SAT_E_UNSUPPORTED, "dit_plan_create: %d query heads not divisible by %d kv heads",
                      cfg->num_heads, kvh);
    }
    SAT_CHECK_ARG(cfg->global_cond_dim % 4 == 0, SAT_E_UNSUPPORTED, "dit_plan_create: global_cond_dim must be a multiple of 4");
    SAT_CHECK_ARG(cfg->gemm_dtype >= 0 && cfg->gemm_dtype <= 3, SAT_E_INVALID,
                  "dit_plan_create: gemm_dtype must be 0 (bf16), 1 (e4m3), 2 (fp32 verification) or 3 (fp16)");
    // 32 / 96: the fp32 kernels take a head width, the MXFP8 attention output does not exist
    SAT_CHECK_ARG(!hdw || cfg->gemm_dtype != 1, SAT_E_UNSUPPORTED, "dit_plan_create: dim_heads %d does not run with e4m3 operands (gemm_dtype 1)", hd);
    SAT_CHECK_ARG(cfg->gemm_dtype != 1 || cfg->embed_dim % 256 == 0, SAT_E_UNSUPPORTED, "dit_plan_create: gemm_dtype needs embed_dim %% 256 == 0");
    // the e4m3 attention outputs (MXFP8) and the fp32 verification kernels (a head row in registers: f32_ref.hip) are built for 64 channels
    SAT_CHECK_ARG(hd != 128 || cfg->gemm_dtype == 0 || cfg->gemm_dtype == 3, SAT_E_UNSUPPORTED,
                  "dit_plan_create: dim_heads 128 runs with bf16 or fp16 operands only (gemm_dtype %d)", cfg->gemm_dtype);
    // (32 / 96 also run in the fp32 verification mode, on the kernels with a head width)
    SAT_CHECK_ARG(hd == 64 || (sat_launch_head_split_hdw && sat_launch_attention_hdw && sat_launch_rope_table_hdw &&
                               (!hdw || (sat_launch_split_heads_f32_w && sat_launch_attention_f32_w))),
                  SAT_E_UNSUPPORTED, "dit_plan_create: dim_heads %d: built without the %d-channel-head kernels", hd, hd);
    SAT_CHECK_ARG(cfg->gemm_dtype == 1 || cfg->fp8_families == 0, SAT_E_INVALID,
                  "dit_plan_create: fp8_families = 0x%x with gemm_dtype %d (a caller built against an older sat_dit_cfg layout?)", cfg->fp8_families, cfg->gemm_dtype);
    SAT_CHECK_ARG(cfg->cross_attention == 0 || cfg->cross_attention == 1, SAT_E_INVALID, "dit_plan_create: cross_attention must be 0 (fused where it applies) or 1 (two kernels)");
    SAT_CHECK_ARG(cfg->tile_policy == 0 || cfg->tile_policy == 22 || cfg->tile_policy == 80 || cfg->tile_policy == 81 || cfg->tile_policy == 82, SAT_E_INVALID,
                  "dit_plan_create: tile_policy must be 0 / 80 (default), 22, 81 or 82");
    const int fam = cfg->fp8_families ? cfg->fp8_families : SAT_FP8_DEFAULT;
    if (cfg->gemm_dtype == 1) {
        SAT_CHECK_ARG((fam & ~SAT_FP8_ALL) == 0, SAT_E_INVALID, "dit_plan_create: unknown bits in fp8_families 0x%x", fam);
        SAT_CHECK_ARG(!(fam & SAT_FP8_FF_OUT) || (fam & SAT_FP8_FF_IN), SAT_E_UNSUPPORTED,
                      "dit_plan_create: FF-out's MXFP8 operand is written by the e4m3 FF-in epilogue: SAT_FP8_FF_OUT needs SAT_FP8_FF_IN");
    }
    sat_dit_plan* p = new (std::nothrow) sat_dit_plan();
    SAT_CHECK_ARG(p, SAT_E_INVALID, "dit_plan_create: out of host memory");
    p->cfg = *cfg;
    p->hd = hd;
    p->kvh_cross = cfg->cond_token_dim > 0 ? cfg->cond_embed_dim / hd : 0;
    // the fold lives in the bf16 pipelined GEMM tiles (K >= 192); adaLN modulates between LayerNorm and GEMM per sequence, the e4m3
    // path quantises the LayerNorm output per token: both keep the standalone kernels
    p->f16 = cfg->gemm_dtype == 3 ? 1 : 0;
    p->fp8_families = cfg->gemm_dtype == 1 ? fam : 0;
    p->cross_fusion = cfg->cross_attention == 0;
    p->tile_bits = sat_tile_policy_bits(cfg->tile_policy);
    p->ln_fold = cfg->ln_fold != 0 && (cfg->gemm_dtype == 0 || cfg->gemm_dtype == 3) && !cfg->adaln && cfg->embed_dim >= 256 && hd == 64;
    p->ln_fold_asked = p->ln_fold;
    *out_plan = p;
    return 0;
}

extern "C" void sat_dit_plan_destroy(sat_dit_plan* p) {
    if (!p) return;
    for (hipEvent_t e : p->prof_ev) (void)hipEventDestroy(e);
    delete p;
}

extern "C" int sat_dit_plan_set_tensor(sat_dit_plan* p, const char* name, const float* data_dev, int64_t numel) {
    SAT_CHECK_ARG(p, SAT_E_INVALID, "dit_plan_set_tensor: bad argument");
    return p->tensors.set("dit", name, data_dev, numel);
}

extern "C" int sat_dit_plan_finalize(sat_dit_plan* p, sat_stream_t stream) {
    SAT_CHECK_ARG(p, SAT_E_INVALID, "dit_plan_finalize: null plan");
    hipStream_t s = (hipStream_t)stream;
    const int D = p->cfg.embed_dim;
    if (p->ff_glu) {
        const int64_t ff_numel = p->tensors.numel("transformer.layers.0.ff.ff.0.proj.weight");
        SAT_CHECK_ARG(ff_numel > 0, SAT_E_MISSING, "dit plan: tensor 'transformer.layers.0.ff.ff.0.proj.weight' was never set");
        SAT_CHECK_ARG(ff_numel % (2 * (int64_t)D) == 0, SAT_E_INVALID, "dit plan: FF weight size not divisible by 2*embed_dim");
        p->inner = (int)(ff_numel / (2 * (int64_t)D));
        SAT_CHECK_ARG(p->inner % 64 == 0, SAT_E_UNSUPPORTED, "dit plan: FF inner dim %d must be a multiple of 64", p->inner);
    } else {      // ff_glu 0: the input Linear is [inner, D] and all of its columns are outputs of the GEMM (N % 128)
        const int64_t ff_numel = p->tensors.numel("transformer.layers.0.ff.ff.0.1.weight");
        SAT_CHECK_ARG(ff_numel > 0, SAT_E_MISSING, "dit plan: tensor 'transformer.layers.0.ff.ff.0.1.weight' was never set");
        SAT_CHECK_ARG(ff_numel % ((int64_t)D * p->ff_conv) == 0, SAT_E_INVALID, "dit plan: FF weight size not divisible by embed_dim (x the kernel size %d)", p->ff_conv);
        p->inner = (int)(ff_numel / ((int64_t)D * p->ff_conv));
        SAT_CHECK_ARG(p->inner % 128 == 0, SAT_E_UNSUPPORTED, "dit plan: FF inner dim %d of a feed-forward without GLU must be a multiple of 128", p->inner);
    }
    if (p->conformer) {      // by name and before anything is allocated, as the FF weight above
        static const char* const names[] = {"in_norm.gamma", "in_norm.beta", "pointwise_conv.weight", "glu.proj.weight", "glu.proj.bias",
                                            "depthwise_conv.weight", "mid_norm.gamma", "mid_norm.beta", "pointwise_conv_2.weight"};
        for (int l = 0; l < p->cfg.depth; ++l)
            for (const char* n : names) {
                const std::string name = "transformer.layers." + std::to_string(l) + ".conformer." + n;
                SAT_CHECK_ARG(p->tensors.has(name), SAT_E_MISSING, "dit plan: tensor '%s' was never set", name.c_str());
            }
    }
    SAT_CHECK_ARG(p->cfg.gemm_dtype != 1 || p->inner % 128 == 0, SAT_E_UNSUPPORTED, "dit plan: gemm_dtype needs an FF inner dim that is a multiple of 128");
    if (p->ff_conv > 1) {      // by name and before anything is allocated; a Conv1d weight of another kernel size than the plan was told has another size
        for (int l = 0; l < p->cfg.depth; ++l) {
            const std::string name = "transformer.layers." + std::to_string(l) + ".ff.ff.2.weight";
            SAT_CHECK_ARG(p->tensors.has(name), SAT_E_MISSING, "dit plan: tensor '%s' was never set", name.c_str());
            SAT_CHECK_ARG(p->tensors.numel(name) == (int64_t)D * p->inner * p->ff_conv, SAT_E_INVALID,
                          "dit plan: tensor '%s' has %lld elements, a Conv1d(%d, %d, %d) weight has %lld", name.c_str(), (long long)p->tensors.numel(name),
                          p->inner, D, p->ff_conv, (long long)D * p->inner * p->ff_conv);
        }
    }
    p->wsq_bf = p->wsq_t = -1;
    return plan_finalize(p, s, [&](Bump& ar) { return build(p, ar, s); });
}

extern "C" int sat_dit_workspace_bytes(const sat_dit_plan* p, int32_t bf, int32_t t_len, size_t* out_bytes) {
    SAT_CHECK_ARG(p && out_bytes && bf > 0 && t_len > 0, SAT_E_INVALID, "dit_workspace_bytes: bad argument");
    SAT_CHECK_ARG(p->finalized, SAT_E_STATE, "dit_workspace_bytes: plan not finalized");
    SAT_CHECK_ARG(t_len % p->patch == 0, SAT_E_INVALID, "dit_workspace_bytes: t_len %d is not a multiple of patch_size %d", t_len, p->patch);
    // enough for any prepend length up to max_prepend_len (the layout is not monotonic in P: the FF-out K-split slab depends on M).
    // Host arithmetic only, once per (bf, t_len): the hot calls check carve() of the prepared P instead.
    if (p->max_prep == 0) {
        *out_bytes = carve(p, bf, t_len, 0, nullptr).total;
        return 0;
    }
    if (p->wsq_bf != bf || p->wsq_t != t_len) {
        size_t need = 0;
        for (int P = 0; P <= p->max_prep; ++P) {
            const size_t b = carve(p, bf, t_len, P, nullptr).total;
            need = b > need ? b : need;
        }
        p->wsq_bf = bf; p->wsq_t = t_len; p->wsq_bytes = need;
    }
    *out_bytes = p->wsq_bytes;
    return 0;
}

extern "C" int sat_dit_prepare_context(sat_dit_plan* p, const float* cond, int32_t bf, int32_t lc, const float* global_cond,
                                       sat_stream_t stream) {
    SAT_CHECK_ARG(p && p->finalized, SAT_E_STATE, "dit_prepare_context: plan not finalized");
    hipStream_t s = (hipStream_t)stream;
    const sat_dit_cfg& c = p->cfg;
    const int D = c.embed_dim, Dc = c.cond_embed_dim, Dct = c.cond_token_dim, Dg = c.global_cond_dim;
    const bool cross = Dct > 0;
    SAT_CHECK_ARG(bf > 0, SAT_E_INVALID, "dit_prepare_context: bf must be positive");
    SAT_CHECK_ARG(!cross || (cond && lc > 0), SAT_E_INVALID, "dit_prepare_context: model has cross-attention but no cond given");
    SAT_CHECK_ARG(!(global_cond && Dg == 0), SAT_E_INVALID, "dit_prepare_context: model has no global conditioning");
    // (a multiple of the attention kernel's key tile: 64 keys, 128 with 32-channel heads -- attn_hdw_tiles.h)
    const int lcpad = cross ? (int)round_up(lc + 3, sat_attn_hdw_key_tile(p->hd)) : 0;
    const int R = bf * lc;
    // layout of the context buffer
    Bump lay;
    const size_t o_ge = lay.take_off((size_t)bf * D * 4);
    const size_t o_gh = lay.take_off((size_t)bf * D * 4);
    const size_t o_ch = cross ? lay.take_off((size_t)R * Dc * 4) : 0;
    const size_t o_ce = cross ? lay.take_off((size_t)R * Dc * 2) : 0;
    const bool f32 = c.gemm_dtype == 2;
    const size_t kv_elems = cross ? (size_t)c.depth * bf * p->kvh_cross * (f32 ? lc : lcpad) * p->hd : 0;
    const size_t o_kc = lay.take_off(kv_elems * (f32 ? 4 : 2));
    const size_t o_vc = lay.take_off(kv_elems * (f32 ? 4 : 2));
    const size_t o_kv32 = (cross && f32) ? lay.take_off((size_t)R * 2 * Dc * 4) : 0;
    const size_t o_ce32 = (cross && f32) ? lay.take_off((size_t)R * Dc * 4) : 0;
    const size_t o_kv_staged = (cross && p->staged() && !f32) ? lay.take_off((size_t)R * 2 * Dc * 4) : 0;      // fp32 to_kv output in front of the head split
    // blocks of both operand formats (sat_dit_plan_set_block_formats): a second image of the context embedding, in the other format than layer 0's
    int mixed = 0;
    for (int l = 1; l < c.depth; ++l) mixed |= layer_f16(p, l) != layer_f16(p, 0);
    const size_t o_ce_other = (cross && !f32 && mixed) ? lay.take_off((size_t)R * Dc * 2) : 0;
    if (lay.off > p->ctx_buf.cap) SAT_HIP(hipStreamSynchronize(s));      // launches of the previous generation may still read the old buffer
    SAT_TRY(p->ctx_buf.reserve(lay.off));
    p->ge = (float*)(p->ctx_buf.ptr + o_ge);
    float* gh = (float*)(p->ctx_buf.ptr + o_gh);
    p->kc = (op_t*)(p->ctx_buf.ptr + o_kc);
    p->vct = (op_t*)(p->ctx_buf.ptr + o_vc);
    p->has_global = global_cond != nullptr;
    if (global_cond) {   // dit.py:154
        SAT_TRY(glue_small_linear(global_cond, Dg, p->ge0_w, nullptr, nullptr, 0, gh, D, bf, D, Dg, 1, 0, s));
        SAT_TRY(glue_small_linear(gh, D, p->ge2_w, nullptr, nullptr, 0, p->ge, D, bf, D, D, 0, 0, s));
    }
    if (cross && f32) {   // fp32 verification mode: fp32 context embedding, fp32 K / V [bf, kvh, lc, 64] per layer
        float* ch = (float*)(p->ctx_buf.ptr + o_ch);
        float* ce32 = (float*)(p->ctx_buf.ptr + o_ce32);
        float* kv32 = (float*)(p->ctx_buf.ptr + o_kv32);
        p->kc32 = (float*)(p->ctx_buf.ptr + o_kc);
        p->vc32 = (float*)(p->ctx_buf.ptr + o_vc);
        SAT_TRY(glue_small_linear(cond, Dct, p->ce0_w, nullptr, nullptr, 0, ch, Dc, R, Dc, Dct, 1, 0, s));
        SAT_TRY(glue_small_linear(ch, Dc, p->ce2_w, nullptr, nullptr, 0, ce32, Dc, R, Dc, Dc, 0, 0, s));
        const size_t per_layer = (size_t)bf * p->kvh_cross * lc * p->hd;
        for (int l = 0; l < c.depth; ++l) {
            SAT_TRY(sat_launch_gemm_f32(ce32, (const float*)p->layers[l].ckv.w, nullptr, kv32, R, 2 * Dc, Dc, 2 * Dc, 0, nullptr, 1, 0, s));
            SAT_TRY(split_heads_f32(p, kv32, p->kc32 + l * per_layer, p->vc32 + l * per_layer, nullptr, R, lc, 2, p->kvh_cross, 0, p->qk_norm ? 1 : 0, s));
        }
    } else if (cross) {   // dit.py:150 then per-layer to_kv (transformer.py:420-427)
        float* ch = (float*)(p->ctx_buf.ptr + o_ch);
        op_t* ce = (op_t*)(p->ctx_buf.ptr + o_ce);
        SAT_TRY(glue_small_linear(cond, Dct, p->ce0_w, nullptr, nullptr, 0, ch, Dc, R, Dc, Dct, 1, 0, s));
        const int f16_0 = layer_f16(p, 0);
        op_t* ce_other = mixed ? (op_t*)(p->ctx_buf.ptr + o_ce_other) : nullptr;
        SAT_TRY(glue_small_linear(ch, Dc, p->ce2_w, nullptr, nullptr, 0, ce, Dc, R, Dc, Dc, 0, f16_0 ? 2 : 1, s));
        if (mixed) SAT_TRY(glue_small_linear(ch, Dc, p->ce2_w, nullptr, nullptr, 0, ce_other, Dc, R, Dc, Dc, 0, f16_0 ? 1 : 2, s));
        SAT_HIP(hipMemsetAsync(p->kc, 0, kv_elems * 2, s));
        SAT_HIP(hipMemsetAsync(p->vct, 0, kv_elems * 2, s));
        const size_t per_layer = (size_t)bf * p->kvh_cross * lcpad * p->hd;
        float* kv32 = p->staged() ? (float*)(p->ctx_buf.ptr + o_kv_staged) : nullptr;
        for (int l = 0; l < c.depth; ++l) {      // k: normalised under qk_norm, v transposed
            GemmArgs g{};
            g.f16 = layer_f16(p, l);
            g.A = g.f16 == f16_0 ? ce : ce_other; g.W = p->layers[l].ckv.w; g.M = R; g.N = 2 * Dc; g.K = Dc;
            if (!p->staged()) g.variant = 1;
            HeadsEpi he{};
            he.out[0] = p->kc + l * per_layer; he.out[1] = p->vct + l * per_layer;
            he.kind[0] = 4 | (p->qk_norm ? 16 : 0); he.kind[1] = 1 | 4; he.parts = 2; he.heads = p->kvh_cross;
            he.S = lc; he.Spad = lcpad;
            SAT_TRY(project_heads(p, g, he, kv32, bf, s));
            // (the layer's whole cache: lcpad - lc zero pad keys per head beside the bf * lc * Dc values)
            SAT_TRY(range_stats(p, l, RS_CROSS_K, p->kc + l * per_layer, per_layer, (size_t)R * Dc, s));
            SAT_TRY(range_stats(p, l, RS_CROSS_V, p->vct + l * per_layer, per_layer, (size_t)R * Dc, s));
        }
    }
    p->ctx_bf = bf;
    p->ctx_null_from = -1;
    p->ext_ready = false;           // the extra conditioning belongs to the previous generation
    p->ext_concat = nullptr;
    p->ext_concat_len = 0;
    p->ext_prep = nullptr;
    p->ctx_prep = 0;
    p->ctx_lc = cross ? lc : 0;
    p->ctx_lcpad = lcpad;
    return 0;
}

extern "C" int sat_dit_set_null_context_from(sat_dit_plan* p, int32_t first_null_seq) {
    SAT_CHECK_ARG(p && p->finalized, SAT_E_STATE, "dit_set_null_context_from: plan not finalized");
    SAT_CHECK_ARG(first_null_seq >= -1 && first_null_seq <= p->ctx_bf, SAT_E_INVALID, "dit_set_null_context_from: %d not in [-1, %d]",
                  first_null_seq, p->ctx_bf);
    p->ctx_null_from = first_null_seq;
    return 0;
}

extern "C" int sat_dit_plan_set_extra_conditioning(sat_dit_plan* p, int32_t input_concat_dim, int32_t prepend_cond_dim, int32_t max_prepend_len) {
    SAT_CHECK_ARG(p, SAT_E_INVALID, "dit_plan_set_extra_conditioning: null plan");
    SAT_CHECK_ARG(!p->finalized, SAT_E_STATE, "dit_plan_set_extra_conditioning: plan already finalized (call it between create and finalize)");
    SAT_CHECK_ARG(input_concat_dim >= 0 && prepend_cond_dim >= 0 && max_prepend_len >= 0, SAT_E_INVALID,
                  "dit_plan_set_extra_conditioning: negative argument (%d, %d, %d)", input_concat_dim, prepend_cond_dim, max_prepend_len);
    SAT_CHECK_ARG((prepend_cond_dim > 0) == (max_prepend_len > 0), SAT_E_INVALID,
                  "dit_plan_set_extra_conditioning: max_prepend_len %d with prepend_cond_dim %d (both positive or both 0)", max_prepend_len,
                  prepend_cond_dim);
    // adaLN + prepend_cond: the reference sets prepend_length only in the "prepend" branch (models/dit.py:158,185-195) and so returns
    // P + T frames (:219); there is no working behaviour to reproduce
    SAT_CHECK_ARG(!(p->cfg.adaln && prepend_cond_dim > 0), SAT_E_UNSUPPORTED,
                  "dit_plan_set_extra_conditioning: prepend_cond with global_cond_type 'adaLN' (the reference drops the wrong rows there)");
    SAT_CHECK_ARG(prepend_cond_dim % 4 == 0, SAT_E_UNSUPPORTED, "dit_plan_set_extra_conditioning: prepend_cond_dim %d must be a multiple of 4",
                  prepend_cond_dim);
    SAT_CHECK_ARG(p->cfg.io_channels + input_concat_dim <= 256, SAT_E_UNSUPPORTED,
                  "dit_plan_set_extra_conditioning: io_channels + input_concat_dim = %d exceeds 256", p->cfg.io_channels + input_concat_dim);
    SAT_CHECK_ARG(p->patch == 1 || (int64_t)(p->cfg.io_channels + input_concat_dim) * p->patch <= 1024, SAT_E_UNSUPPORTED,
                  "dit_plan_set_extra_conditioning: (io_channels + input_concat_dim) * patch_size = %lld exceeds 1024",
                  (long long)(p->cfg.io_channels + input_concat_dim) * p->patch);
    SAT_CHECK_ARG((int64_t)p->cfg.max_seq_len + 1 + max_prepend_len <= (1 << 20), SAT_E_INVALID,
                  "dit_plan_set_extra_conditioning: max_prepend_len %d too large", max_prepend_len);
    p->concat_dim = input_concat_dim;
    p->prepend_dim = prepend_cond_dim;
    p->max_prep = max_prepend_len;
    return 0;
}

extern "C" int sat_dit_plan_set_transformer_options(sat_dit_plan* p, const sat_dit_transformer_options* o, size_t options_bytes) {
    SAT_CHECK_ARG(p && o, SAT_E_INVALID, "dit_plan_set_transformer_options: null argument");
    SAT_CHECK_ARG(options_bytes == sizeof(sat_dit_transformer_options), SAT_E_INVALID,
                  "dit_plan_set_transformer_options: sat_dit_transformer_options of %zu bytes; this library knows %zu", options_bytes,
                  sizeof(sat_dit_transformer_options));
    SAT_CHECK_ARG(!p->finalized, SAT_E_STATE, "dit_plan_set_transformer_options: plan already finalized (call it between create and finalize)");
    SAT_CHECK_ARG((o->qk_norm == 0 || o->qk_norm == 1) && (o->rotary == 0 || o->rotary == 1) && o->pos_emb >= SAT_DIT_POS_NONE &&
                      o->pos_emb <= SAT_DIT_POS_ABSOLUTE,
                  SAT_E_UNSUPPORTED, "dit_plan_set_transformer_options: unknown value (qk_norm %d, pos_emb %d, rotary %d)", o->qk_norm, o->pos_emb,
                  o->rotary);
    SAT_CHECK_ARG(o->pos_emb != SAT_DIT_POS_ABSOLUTE || (o->abs_pos_max_len > 0 && o->abs_pos_max_len <= (1 << 20)), SAT_E_INVALID,
                  "dit_plan_set_transformer_options: abs_pos_max_len %d with absolute position embeddings", o->abs_pos_max_len);
    // the e4m3 epilogues (per-token x per-channel scales, the 8-phase block-scaled build) carry no normalisation
    SAT_CHECK_ARG(!(o->qk_norm && p->cfg.gemm_dtype == 1), SAT_E_UNSUPPORTED,
                  "dit_plan_set_transformer_options: qk_norm with gemm_dtype fp8 is not built (use bf16, fp16 or the fp32 verification mode)");
    p->qk_norm = o->qk_norm != 0;
    p->pos_emb = o->pos_emb;
    p->abs_max = o->pos_emb == SAT_DIT_POS_ABSOLUTE ? o->abs_pos_max_len : 0;
    p->rotary = o->rotary != 0;
    return 0;
}

extern "C" int sat_dit_plan_set_block_options(sat_dit_plan* p, const sat_dit_block_options* o, size_t options_bytes) {
    SAT_CHECK_ARG(p && o, SAT_E_INVALID, "dit_plan_set_block_options: null argument");
    SAT_CHECK_ARG(options_bytes == sizeof(sat_dit_block_options), SAT_E_INVALID,
                  "dit_plan_set_block_options: sat_dit_block_options of %zu bytes; this library knows %zu", options_bytes, sizeof(sat_dit_block_options));
    SAT_CHECK_ARG(!p->finalized, SAT_E_STATE, "dit_plan_set_block_options: plan already finalized (call it between create and finalize)");
    SAT_CHECK_ARG((o->conformer == 0 || o->conformer == 1) && (o->remove_norms == 0 || o->remove_norms == 1) && (o->ff_glu == 0 || o->ff_glu == 1),
                  SAT_E_UNSUPPORTED, "dit_plan_set_block_options: unknown value (conformer %d, remove_norms %d, ff_glu %d)", o->conformer, o->remove_norms,
                  o->ff_glu);
    const bool any = o->conformer || o->remove_norms || !o->ff_glu;
    // the e4m3 epilogues and the quantising LayerNorm know neither a missing norm nor the plain activation; the staged route (128-, 32-
    // and 96-channel heads) keeps the standalone LayerNorms of the shipped block
    SAT_CHECK_ARG(!any || p->cfg.gemm_dtype != SAT_GEMM_FP8, SAT_E_UNSUPPORTED,
                  "dit_plan_set_block_options: conformer / remove_norms / ff_glu 0 with gemm_dtype fp8 is not built (use bf16, fp16 or the fp32 verification mode)");
    SAT_CHECK_ARG(!any || p->hd == 64, SAT_E_UNSUPPORTED, "dit_plan_set_block_options: conformer / remove_norms / ff_glu 0 with dim_heads %d is not built (64 only)", p->hd);
    SAT_CHECK_ARG(!any || (sat_launch_dwconv_ln_silu && sat_launch_round_rows && sat_launch_silu_f32), SAT_E_UNSUPPORTED,
                  "dit_plan_set_block_options: built without the block-option kernels");
    SAT_CHECK_ARG(!any || !p->rr, SAT_E_UNSUPPORTED, "dit_plan_set_block_options: the range report has no rows for the buffers of these options (sat_dit_range_report off first)");
    p->conformer = o->conformer != 0;
    p->remove_norms = o->remove_norms != 0;
    p->ff_glu = o->ff_glu != 0;
    return 0;
}

extern "C" int sat_dit_plan_set_attention_options(sat_dit_plan* p, const sat_dit_attention_options* o, size_t options_bytes) {
    SAT_CHECK_ARG(p && o, SAT_E_INVALID, "dit_plan_set_attention_options: null argument");
    SAT_CHECK_ARG(options_bytes == sizeof(sat_dit_attention_options), SAT_E_INVALID,
                  "dit_plan_set_attention_options: sat_dit_attention_options of %zu bytes; this library knows %zu", options_bytes,
                  sizeof(sat_dit_attention_options));
    SAT_CHECK_ARG(!p->finalized, SAT_E_STATE, "dit_plan_set_attention_options: plan already finalized (call it between create and finalize)");
    SAT_CHECK_ARG(o->causal == 0 || o->causal == 1, SAT_E_INVALID, "dit_plan_set_attention_options: causal %d is neither 0 nor 1", o->causal);
    // transformer.py:371, 530: with more context keys than queries the reference fails, with fewer its backends disagree on where the mask
    // sits; there is no working behaviour to reproduce
    SAT_CHECK_ARG(!(o->causal && p->cfg.cond_token_dim > 0), SAT_E_UNSUPPORTED,
                  "dit_plan_set_attention_options: causal with cross-attention (cond_token_dim %d): the reference has no working behaviour there",
                  p->cfg.cond_token_dim);
    // the MXFP8 output form of the attention kernels has no causal variant (gemm_dtype is fixed at create: no later call can make the plan e4m3)
    SAT_CHECK_ARG(!(o->causal && p->cfg.gemm_dtype == SAT_GEMM_FP8), SAT_E_UNSUPPORTED,
                  "dit_plan_set_attention_options: causal with gemm_dtype fp8 is not built (use bf16, fp16 or the fp32 verification mode)");
    SAT_CHECK_ARG(!o->causal || (sat_launch_attention_causal && sat_launch_attention_hdw_causal && sat_launch_attention_f32_causal), SAT_E_UNSUPPORTED,
                  "dit_plan_set_attention_options: built without the causal attention kernels");
    SAT_CHECK_ARG(!(o->causal && p->natten), SAT_E_UNSUPPORTED,
                  "dit_plan_set_attention_options: causal on a neighbourhood-attention plan: the reference ignores causal in that branch");
    p->causal = o->causal != 0;
    return 0;
}

extern "C" int sat_dit_plan_set_neighborhood_attention(sat_dit_plan* p, const sat_dit_neighborhood_options* o, size_t options_bytes) {
    SAT_CHECK_ARG(p && o, SAT_E_INVALID, "dit_plan_set_neighborhood_attention: null argument");
    SAT_CHECK_ARG(options_bytes == sizeof(sat_dit_neighborhood_options), SAT_E_INVALID,
                  "dit_plan_set_neighborhood_attention: sat_dit_neighborhood_options of %zu bytes; this library knows %zu", options_bytes,
                  sizeof(sat_dit_neighborhood_options));
    SAT_CHECK_ARG(!p->finalized, SAT_E_STATE, "dit_plan_set_neighborhood_attention: plan already finalized (call it between create and finalize)");
    const int ks = o->kernel_size;
    // 0: full attention (the reference tests the value's truth); else what NATTEN takes: odd and greater than 1
    SAT_CHECK_ARG(ks == 0 || (ks > 1 && (ks & 1)), SAT_E_INVALID,
                  "dit_plan_set_neighborhood_attention: kernel_size %d must be 0 (off) or odd and greater than 1", ks);
    // transformer.py:299, 324: attn_kwargs reach cross_attn too, where q and k differ in length and NATTEN fails: no behaviour to reproduce
    SAT_CHECK_ARG(!(ks && p->cfg.cond_token_dim > 0), SAT_E_UNSUPPORTED,
                  "dit_plan_set_neighborhood_attention: natten_kernel_size with cross-attention (cond_token_dim %d): the reference has no working behaviour there",
                  p->cfg.cond_token_dim);
    // transformer.py:479: the branch never looks at causal
    SAT_CHECK_ARG(!(ks && p->causal), SAT_E_UNSUPPORTED,
                  "dit_plan_set_neighborhood_attention: natten_kernel_size on a causal plan: the reference ignores causal in that branch");
    SAT_CHECK_ARG(!(ks && p->cfg.gemm_dtype == SAT_GEMM_FP8), SAT_E_UNSUPPORTED,
                  "dit_plan_set_neighborhood_attention: natten_kernel_size with gemm_dtype fp8 is not built (use bf16, fp16 or the fp32 verification mode)");
    SAT_CHECK_ARG(!(ks && p->hd != 64), SAT_E_UNSUPPORTED,
                  "dit_plan_set_neighborhood_attention: natten_kernel_size with dim_heads %d is not built (64 only; the staged widths are a follow-up)", p->hd);
    SAT_CHECK_ARG(!ks || (sat_launch_attention_window && sat_launch_attention_f32_window), SAT_E_UNSUPPORTED,
                  "dit_plan_set_neighborhood_attention: built without the neighbourhood attention kernels");
    p->natten = ks;
    return 0;
}

// The same call for every built head width: 64 as above, and the staged widths 128, 32 and 96 (attention_hdw_window.hip).  Its own entry, so
// that sat_dit_plan_set_neighborhood_attention keeps answering what it answered; the checks are that one's, but for the width
extern "C" int sat_dit_plan_set_neighborhood_attention_hdw(sat_dit_plan* p, const sat_dit_neighborhood_options* o, size_t options_bytes) {
    SAT_CHECK_ARG(p && o, SAT_E_INVALID, "dit_plan_set_neighborhood_attention_hdw: null argument");
    SAT_CHECK_ARG(options_bytes == sizeof(sat_dit_neighborhood_options), SAT_E_INVALID,
                  "dit_plan_set_neighborhood_attention_hdw: sat_dit_neighborhood_options of %zu bytes; this library knows %zu", options_bytes,
                  sizeof(sat_dit_neighborhood_options));
    SAT_CHECK_ARG(!p->finalized, SAT_E_STATE, "dit_plan_set_neighborhood_attention_hdw: plan already finalized (call it between create and finalize)");
    const int ks = o->kernel_size;
    // 0: full attention (the reference tests the value's truth); else what NATTEN takes: odd and greater than 1
    SAT_CHECK_ARG(ks == 0 || (ks > 1 && (ks & 1)), SAT_E_INVALID,
                  "dit_plan_set_neighborhood_attention_hdw: kernel_size %d must be 0 (off) or odd and greater than 1", ks);
    // transformer.py:299, 324: attn_kwargs reach cross_attn too, where q and k differ in length and NATTEN fails: no behaviour to reproduce
    SAT_CHECK_ARG(!(ks && p->cfg.cond_token_dim > 0), SAT_E_UNSUPPORTED,
                  "dit_plan_set_neighborhood_attention_hdw: natten_kernel_size with cross-attention (cond_token_dim %d): the reference has no working behaviour there",
                  p->cfg.cond_token_dim);
    // transformer.py:479: the branch never looks at causal
    SAT_CHECK_ARG(!(ks && p->causal), SAT_E_UNSUPPORTED,
                  "dit_plan_set_neighborhood_attention_hdw: natten_kernel_size on a causal plan: the reference ignores causal in that branch");
    SAT_CHECK_ARG(!(ks && p->cfg.gemm_dtype == SAT_GEMM_FP8), SAT_E_UNSUPPORTED,
                  "dit_plan_set_neighborhood_attention_hdw: natten_kernel_size with gemm_dtype fp8 is not built (use bf16, fp16 or the fp32 verification mode)");
    SAT_CHECK_ARG(!ks || (sat_launch_attention_window && sat_launch_attention_f32_window), SAT_E_UNSUPPORTED,
                  "dit_plan_set_neighborhood_attention_hdw: built without the neighbourhood attention kernels");
    SAT_CHECK_ARG(!(ks && p->staged()) || (sat_launch_attention_hdw_window && sat_launch_attention_f32_window_w), SAT_E_UNSUPPORTED,
                  "dit_plan_set_neighborhood_attention_hdw: natten_kernel_size with dim_heads %d: built without the neighbourhood attention kernels of the "
                  "staged widths", p->hd);
    p->natten = ks;
    return 0;
}

extern "C" int sat_dit_plan_set_patch(sat_dit_plan* p, const sat_dit_patch_options* o, size_t options_bytes) {
    SAT_CHECK_ARG(p && o, SAT_E_INVALID, "dit_plan_set_patch: null argument");
    SAT_CHECK_ARG(options_bytes == sizeof(sat_dit_patch_options), SAT_E_INVALID,
                  "dit_plan_set_patch: sat_dit_patch_options of %zu bytes; this library knows %zu", options_bytes, sizeof(sat_dit_patch_options));
    SAT_CHECK_ARG(!p->finalized, SAT_E_STATE, "dit_plan_set_patch: plan already finalized (call it between create and finalize)");
    const int pt = o->patch_size;
    SAT_CHECK_ARG(pt >= 1, SAT_E_INVALID, "dit_plan_set_patch: patch_size %d", pt);
    // the limits of the two boundary kernels (dit_patch.hip checks the same at launch); io_channels and the concat width: create / set_extra_conditioning
    const int64_t C = p->cfg.io_channels, Ci = C + p->concat_dim;
    SAT_CHECK_ARG(pt == 1 || C * pt <= 512, SAT_E_UNSUPPORTED, "dit_plan_set_patch: io_channels * patch_size = %lld exceeds 512", (long long)(C * pt));
    SAT_CHECK_ARG(pt == 1 || Ci * pt <= 1024, SAT_E_UNSUPPORTED,
                  "dit_plan_set_patch: (io_channels + input_concat_dim) * patch_size = %lld exceeds 1024", (long long)(Ci * pt));
    SAT_CHECK_ARG(pt == 1 || p->cfg.max_seq_len >= pt, SAT_E_INVALID, "dit_plan_set_patch: patch_size %d exceeds max_seq_len %d", pt, p->cfg.max_seq_len);
    SAT_CHECK_ARG(pt == 1 || (glue_fold_in_patch && glue_fold_out_patch && glue_input_proj_patch && glue_output_proj_patch), SAT_E_UNSUPPORTED,
                  "dit_plan_set_patch: built without the patch kernels");
    p->patch = pt;
    return 0;
}

extern "C" int sat_dit_plan_set_ff_conv(sat_dit_plan* p, const sat_dit_ff_conv_options* o, size_t options_bytes) {
    SAT_CHECK_ARG(p && o, SAT_E_INVALID, "dit_plan_set_ff_conv: null argument");
    SAT_CHECK_ARG(options_bytes == sizeof(sat_dit_ff_conv_options), SAT_E_INVALID,
                  "dit_plan_set_ff_conv: sat_dit_ff_conv_options of %zu bytes; this library knows %zu", options_bytes, sizeof(sat_dit_ff_conv_options));
    SAT_CHECK_ARG(!p->finalized, SAT_E_STATE, "dit_plan_set_ff_conv: plan already finalized (call it between create and finalize)");
    const int k = o->kernel_size;
    SAT_CHECK_ARG(k >= 1, SAT_E_INVALID, "dit_plan_set_ff_conv: kernel_size %d", k);
    // transformer.py:245,285: Conv1d(padding = k // 2) returns n + 1 rows for an even k and the reference's own residual add fails
    SAT_CHECK_ARG(k % 2 == 1, SAT_E_UNSUPPORTED, "dit_plan_set_ff_conv: kernel_size %d is even: the reference's convolution then returns one row more than it was given", k);
    SAT_CHECK_ARG(k <= 7, SAT_E_UNSUPPORTED, "dit_plan_set_ff_conv: kernel_size %d: the convolution GEMM is built for 1, 3, 5 and 7", k);
    // the e4m3 operands carry one scale per row or per 32 k of a row, which a row-shifted read would have to shift as well; the staged
    // route (128-, 32- and 96-channel heads) keeps the shipped block, as for sat_dit_plan_set_block_options
    SAT_CHECK_ARG(k == 1 || p->cfg.gemm_dtype != SAT_GEMM_FP8, SAT_E_UNSUPPORTED,
                  "dit_plan_set_ff_conv: a convolutional feed-forward with gemm_dtype fp8 is not built (use bf16, fp16 or the fp32 verification mode)");
    SAT_CHECK_ARG(k == 1 || p->hd == 64, SAT_E_UNSUPPORTED, "dit_plan_set_ff_conv: a convolutional feed-forward with dim_heads %d is not built (64 only)", p->hd);
    SAT_CHECK_ARG(k == 1 || (sat_launch_ff_conv && sat_launch_pack_conv_taps && sat_launch_im2col_rows_f32), SAT_E_UNSUPPORTED,
                  "dit_plan_set_ff_conv: built without the convolution GEMM");
    SAT_CHECK_ARG(k == 1 || !p->rr, SAT_E_UNSUPPORTED, "dit_plan_set_ff_conv: the range report has no rows for such a plan (sat_dit_range_report off first)");
    p->ff_conv = k;
    // FF-out's epilogue here writes no 16-bit image and no row statistics, and a convolutional FF-in could not use them (they differ per tap):
    // every LayerNorm of such a plan is the standalone kernel
    p->ln_fold = p->ln_fold_asked && k == 1;
    return 0;
}

extern "C" int sat_dit_plan_set_block_formats(sat_dit_plan* p, const int32_t* formats, int32_t n) {
    SAT_CHECK_ARG(p && formats, SAT_E_INVALID, "dit_plan_set_block_formats: null argument");
    SAT_CHECK_ARG(!p->finalized, SAT_E_STATE, "dit_plan_set_block_formats: plan already finalized (call it between create and finalize)");
    // e4m3 plans choose their operand formats per GEMM family, the fp32 verification mode has no 16-bit operand
    SAT_CHECK_ARG(p->cfg.gemm_dtype == SAT_GEMM_BF16 || p->cfg.gemm_dtype == SAT_GEMM_FP16, SAT_E_UNSUPPORTED,
                  "dit_plan_set_block_formats: per-block formats need a plan with gemm_dtype bf16 or fp16, this plan has gemm_dtype %d", p->cfg.gemm_dtype);
    SAT_CHECK_ARG(n == p->cfg.depth, SAT_E_INVALID, "dit_plan_set_block_formats: %d formats for a plan of depth %d", n, p->cfg.depth);
    for (int l = 0; l < n; ++l)
        SAT_CHECK_ARG(formats[l] == SAT_GEMM_BF16 || formats[l] == SAT_GEMM_FP16, SAT_E_INVALID,
                      "dit_plan_set_block_formats: formats[%d] = %d is neither SAT_GEMM_BF16 (%d) nor SAT_GEMM_FP16 (%d)", l, formats[l], SAT_GEMM_BF16,
                      SAT_GEMM_FP16);
    p->block_f16.resize(n);
    for (int l = 0; l < n; ++l) p->block_f16[l] = formats[l] == SAT_GEMM_FP16 ? 1 : 0;
    return 0;
}

extern "C" int sat_dit_prepare_extra_conditioning(sat_dit_plan* p, const float* concat, int32_t concat_len, const float* prepend,
                                                  int32_t prepend_len, int32_t bf, sat_stream_t stream) {
    SAT_CHECK_ARG(p && p->finalized, SAT_E_STATE, "dit_prepare_extra_conditioning: plan not finalized");
    SAT_CHECK_ARG(p->ctx_bf > 0 && p->ctx_bf == bf, SAT_E_STATE,
                  "dit_prepare_extra_conditioning: context prepared for %d sequences, called with %d (sat_dit_prepare_context first)", p->ctx_bf, bf);
    hipStream_t s = (hipStream_t)stream;
    const int D = p->cfg.embed_dim, Cc = p->concat_dim;
    SAT_CHECK_ARG(!concat || Cc > 0, SAT_E_INVALID, "dit_prepare_extra_conditioning: the model has no input_concat_dim");
    SAT_CHECK_ARG(Cc == 0 || (concat && concat_len > 0), SAT_E_INVALID,
                  "dit_prepare_extra_conditioning: the model has input_concat_dim %d and needs input_concat_cond (concat_len > 0)", Cc);
    SAT_CHECK_ARG(!prepend || p->prepend_dim > 0, SAT_E_INVALID, "dit_prepare_extra_conditioning: the model has no prepend_cond_dim");
    SAT_CHECK_ARG(prepend ? (prepend_len > 0 && prepend_len <= p->max_prep) : prepend_len == 0, SAT_E_INVALID,
                  "dit_prepare_extra_conditioning: prepend_len %d not in 1..max_prepend_len %d", prepend_len, p->max_prep);
    const size_t n_cat = Cc ? (size_t)bf * Cc * concat_len : 0;
    const size_t n_prep = prepend ? (size_t)bf * prepend_len * D : 0;
    Bump lay;
    const size_t o_cat = lay.take_off(n_cat * 4), o_h = lay.take_off(n_prep * 4), o_prep = lay.take_off(n_prep * 4);
    if (lay.off > p->ext_buf.cap) SAT_HIP(hipStreamSynchronize(s));
    SAT_TRY(p->ext_buf.reserve(lay.off));
    p->ext_ready = false;
    if (Cc) SAT_HIP(hipMemcpyAsync(p->ext_buf.ptr + o_cat, concat, n_cat * 4, hipMemcpyDeviceToDevice, s));
    if (prepend) {   // dit.py:160-165: Linear(prepend_cond_dim, D, bias=False), SiLU, Linear(D, D, bias=False)
        const int R = bf * prepend_len;
        float* h = (float*)(p->ext_buf.ptr + o_h);
        SAT_TRY(glue_small_linear(prepend, p->prepend_dim, p->pe0_w, nullptr, nullptr, 0, h, D, R, D, p->prepend_dim, 1, 0, s));
        SAT_TRY(glue_small_linear(h, D, p->pe2_w, nullptr, nullptr, 0, p->ext_buf.ptr + o_prep, D, R, D, D, 0, 0, s));
    }
    p->ext_concat = Cc ? (const float*)(p->ext_buf.ptr + o_cat) : nullptr;
    p->ext_concat_len = Cc ? concat_len : 0;
    p->ext_prep = prepend ? (float*)(p->ext_buf.ptr + o_prep) : nullptr;
    p->ctx_prep = prepend ? prepend_len : 0;
    p->ext_ready = Cc > 0 || prepend;       // neither: the plain path (P = 0), as after sat_dit_prepare_context
    return 0;
}

extern "C" int sat_dit_forward(sat_dit_plan* p, const float* x_dev, const float* t_dev, float* out_dev, int32_t bf, int32_t t_len,
                               void* ws, size_t ws_bytes, sat_stream_t stream) {
    SAT_CHECK_ARG(t_dev, SAT_E_INVALID, "dit_forward: t_dev is null");
    return run_forward(p, x_dev, bf, 1.0f, t_dev, 0.f, out_dev, bf, t_len, ws, ws_bytes, (hipStream_t)stream);
}

extern "C" int sat_dit_denoise_cfg(sat_dit_plan* p, const float* x_dev, float sigma, float cfg_scale, float scale_phi,
                                   float* denoised_dev, int32_t b, int32_t t_len, void* ws, size_t ws_bytes, sat_stream_t stream) {
    SAT_CHECK_ARG(p && p->finalized, SAT_E_STATE, "dit_denoise_cfg: plan not finalized");
    SAT_CHECK_ARG(x_dev && denoised_dev && b > 0 && t_len > 0 && ws, SAT_E_INVALID, "dit_denoise_cfg: bad arguments");
    SAT_CHECK_ARG(t_len % p->patch == 0, SAT_E_INVALID, "dit_denoise_cfg: t_len %d is not a multiple of patch_size %d", t_len, p->patch);
    hipStream_t s = (hipStream_t)stream;
    // models/dit.py:270: CFG only when cfg_scale != 1 and there is cross-attention or prepend conditioning
    const int use_cfg = (cfg_scale != 1.0f && (p->cfg.cond_token_dim > 0 || p->ctx_prep > 0)) ? 1 : 0;
    const int bf = use_cfg ? 2 * b : b;
    // k_diffusion.external.VDenoiser, sigma_data = 1
    const double sg = (double)sigma;
    const float c_skip = (float)(1.0 / (sg * sg + 1.0));
    const float c_out = (float)(-sg / sqrt(sg * sg + 1.0));
    const float c_in = (float)(1.0 / sqrt(sg * sg + 1.0));
    const float t = (float)(atan(sg) / M_PI * 2.0);
    Workspace w = carve(p, bf, t_len, p->ctx_prep, (char*)ws);      // the layout of the prepared prepend length P
    SAT_CHECK_ARG(ws_bytes >= w.total, SAT_E_WORKSPACE, "dit_denoise_cfg: workspace %zu < required %zu", ws_bytes, w.total);
    SAT_TRY(run_forward(p, x_dev, b, c_in, nullptr, t, w.mo, bf, t_len, ws, ws_bytes, s));
    return glue_cfg_denoise(w.mo, x_dev, denoised_dev, b, p->cfg.io_channels, t_len, use_cfg, cfg_scale, scale_phi, c_out, c_skip, s);
}

extern "C" int sat_dit_profile(sat_dit_plan* p, int32_t enable) {
    SAT_CHECK_ARG(p, SAT_E_INVALID, "dit_profile: null plan");
    p->prof_on = enable != 0;
    p->prof_n = 0;
    return 0;
}

extern "C" int sat_dit_profile_read(sat_dit_plan* p, double* total_ms, int32_t* launches, int64_t* m, int64_t* n, int64_t* k) {
    SAT_CHECK_ARG(p && total_ms && launches, SAT_E_INVALID, "dit_profile_read: null argument");
    double tot = 0.0;
    for (int i = 0; i < p->prof_n; ++i) {
        SAT_HIP(hipEventSynchronize(p->prof_ev[2 * i + 1]));
        float ms = 0.f;
        SAT_HIP(hipEventElapsedTime(&ms, p->prof_ev[2 * i], p->prof_ev[2 * i + 1]));
        tot += ms;
    }
    *total_ms = tot;
    *launches = p->prof_n;
    if (m) *m = p->prof_m;
    if (n) *n = p->prof_nn;
    if (k) *k = p->prof_k;
    return 0;
}

extern "C" int sat_dit_debug(sat_dit_plan* p, int32_t enable) {
    SAT_CHECK_ARG(p, SAT_E_INVALID, "dit_debug: null plan");
    if (enable && !p->dbg) {
        SAT_CHECK_ARG(p->cfg.gemm_dtype != 2, SAT_E_UNSUPPORTED, "dit_debug: the fp32 verification mode keeps no 16-bit image of the residual stream");
        SAT_TRY(p->dbg_buf.reserve((size_t)p->cfg.depth * 3 * 4 * sizeof(float)));
        p->dbg = (float*)p->dbg_buf.ptr;
        SAT_HIP(hipMemset(p->dbg, 0, (size_t)p->cfg.depth * 3 * 4 * sizeof(float)));
    } else if (!enable && p->dbg) {
        SAT_HIP(hipDeviceSynchronize());
        p->dbg_buf.release();
        p->dbg = nullptr;
    }
    return 0;
}

extern "C" int sat_dit_debug_read(sat_dit_plan* p, float* out_host, int32_t capacity_floats, sat_stream_t stream) {
    SAT_CHECK_ARG(p && out_host, SAT_E_INVALID, "dit_debug_read: null argument");
    SAT_CHECK_ARG(p->dbg, SAT_E_STATE, "dit_debug_read: diagnostics are not enabled (sat_dit_debug)");
    const int n = p->cfg.depth * 3 * 4;
    SAT_CHECK_ARG(capacity_floats >= n, SAT_E_INVALID, "dit_debug_read: room for %d floats, need %d", capacity_floats, n);
    SAT_HIP(hipMemcpyAsync(out_host, p->dbg, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, (hipStream_t)stream));
    SAT_HIP(hipStreamSynchronize((hipStream_t)stream));
    return 0;
}

extern "C" int sat_dit_range_report(sat_dit_plan* p, int32_t enable) {
    SAT_CHECK_ARG(p, SAT_E_INVALID, "dit_range_report: null plan");
    SAT_CHECK_ARG(enable >= 0 && enable <= 2, SAT_E_INVALID, "dit_range_report: enable must be 0 (off), 1 (on) or 2 (zero the records), got %d", enable);
    if (enable == 0) {
        if (!p->rr) return 0;
        SAT_HIP(hipDeviceSynchronize());          // launches in flight still accumulate into the records
        p->rr_buf.release();
        p->rr = nullptr;
        return 0;
    }
    // e4m3 plans quantise A / AO / Hh to bytes with scales beside them, the fp32 verification mode has no 16-bit buffer at all
    SAT_CHECK_ARG(p->cfg.gemm_dtype == SAT_GEMM_BF16 || p->cfg.gemm_dtype == SAT_GEMM_FP16, SAT_E_UNSUPPORTED,
                  "dit_range_report: the report reads 16-bit operand buffers (gemm_dtype bf16 or fp16), this plan has gemm_dtype %d", p->cfg.gemm_dtype);
    SAT_CHECK_ARG(sat_launch_range_stats, SAT_E_UNSUPPORTED, "dit_range_report: built without the range statistics kernel");
    SAT_CHECK_ARG(p->ff_conv == 1, SAT_E_UNSUPPORTED, "dit_range_report: no rows for a plan with a convolutional feed-forward (sat_dit_plan_set_ff_conv)");
    SAT_CHECK_ARG(!p->block_options(), SAT_E_UNSUPPORTED,
                  "dit_range_report: no rows for the 16-bit buffers of a plan with conformer / remove_norms / ff_glu 0 (sat_dit_plan_set_block_options)");
    const size_t bytes = (size_t)p->cfg.depth * SAT_DIT_RANGE_SLOTS * sizeof(sat_range_record);
    if (enable == 2) {
        SAT_CHECK_ARG(p->rr, SAT_E_STATE, "dit_range_report: the report is not enabled, there is nothing to zero");
        SAT_HIP(hipDeviceSynchronize());
        SAT_HIP(hipMemset(p->rr, 0, bytes));
        return 0;
    }
    if (p->rr) return 0;          // already on: the records keep accumulating
    SAT_TRY(p->rr_buf.reserve(bytes));
    SAT_HIP(hipMemset(p->rr_buf.ptr, 0, bytes));
    p->rr = (sat_range_record*)p->rr_buf.ptr;
    return 0;
}

extern "C" int sat_dit_range_report_read(sat_dit_plan* p, sat_range_record* out_host, int32_t capacity_records, size_t record_bytes,
                                         sat_stream_t stream) {
    SAT_CHECK_ARG(p && out_host, SAT_E_INVALID, "dit_range_report_read: null argument");
    SAT_CHECK_ARG(record_bytes == sizeof(sat_range_record), SAT_E_INVALID,
                  "dit_range_report_read: sat_range_record of %zu bytes; this library knows %zu", record_bytes, sizeof(sat_range_record));
    const int n = p->cfg.depth * SAT_DIT_RANGE_SLOTS;
    SAT_CHECK_ARG(capacity_records >= n, SAT_E_INVALID, "dit_range_report_read: room for %d records, need %d", capacity_records, n);
    SAT_CHECK_ARG(p->rr, SAT_E_STATE, "dit_range_report_read: the report is not enabled (sat_dit_range_report)");
    SAT_HIP(hipMemcpyAsync(out_host, p->rr, (size_t)n * sizeof(sat_range_record), hipMemcpyDeviceToHost, (hipStream_t)stream));
    SAT_HIP(hipStreamSynchronize((hipStream_t)stream));
    return 0;
}

extern "C" const char* sat_dit_range_slot_name(int32_t slot) { return slot >= 0 && slot < SAT_DIT_RANGE_SLOTS ? kRangeSlotNames[slot] : nullptr; }

extern "C" int sat_cfg_combine(const float* model_out_dev, float* out_dev, int32_t b, int32_t c, int32_t t, float cfg_scale,
                               float scale_phi, sat_stream_t stream) {
    SAT_CHECK_ARG(model_out_dev && out_dev && b > 0 && c > 1 && t > 0, SAT_E_INVALID, "cfg_combine: bad arguments");
    // denoise form with c_out = 1, c_skip = 0 (x is not read when c_skip == 0, but must be a valid pointer)
    return glue_cfg_denoise(model_out_dev, model_out_dev, out_dev, b, c, t, 1, cfg_scale, scale_phi, 1.0f, 0.0f, (hipStream_t)stream);
}
