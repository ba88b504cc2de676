// Host driver of tests/test_dit_launches_host.py: runs the DiT plan (csrc/dit_plan.hip, host code only) on the CPU and prints what it would
// launch.  This file and host_runtime.h define every symbol dit_plan.o leaves undefined: the HIP runtime calls work on host memory (hipMalloc is
// malloc, recorded in allocation order; copies and memsets are memcpy / memset, so finalize and the prepare calls really run and a host sanitizer
// sees every byte they move), every internal launcher appends one line -- its name and every scalar argument -- and the C-ABI return codes and
// error texts are printed in between.  Pointers are printed as null, alloc<k>+<offset>, ws+<offset> or in:<name>+<offset>.
// Built with hipcc --cuda-host-only (sat_common.h names the HIP types) and linked without the HIP runtime.
//   dit_launch_dump            every case, each behind a line "== <name>"
#include "dit_glue.h"
#include "host_runtime.h"

extern "C" {
hipError_t hipEventCreate(hipEvent_t* e) {
    static uintptr_t n = 0;
    *e = (hipEvent_t)(++n);
    return line("hipEventCreate"), hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t e) { return line("hipEventDestroy", (int)(uintptr_t)e), hipSuccess; }
hipError_t hipEventRecord(hipEvent_t e, hipStream_t) { return line("hipEventRecord", (int)(uintptr_t)e), hipSuccess; }
hipError_t hipEventSynchronize(hipEvent_t e) { return line("hipEventSynchronize", (int)(uintptr_t)e), hipSuccess; }
hipError_t hipEventElapsedTime(float* ms, hipEvent_t, hipEvent_t) {
    *ms = 1.0f;
    return hipSuccess;
}
int sat_version(void) { return 6; }
}

// ------------------------------------------------------------------------------ the launchers
#define V(p) (const void*)(p)
int glue_small_linear(const float* x, int ldx, const float* W, const float* bias, const float* add, int ldadd, void* y, int ldy, int R, int N,
                      int K, int act, int out16, hipStream_t) {
    return line("glue_small_linear", V(x), ldx, V(W), V(bias), V(add), ldadd, V(y), ldy, R, N, K, act, out16);
}
int glue_adaln_finish(float* ssg, int64_t n, int D, hipStream_t) { return line("glue_adaln_finish", V(ssg), (long long)n, D); }
int glue_fourier(const float* t, float t_const, const float* w, float* out, int B, int half_feat, hipStream_t) {
    return line("glue_fourier", V(t), (double)t_const, V(w), V(out), B, half_feat);
}
int glue_fold_in(const float* Win, const float* Wpre, float* Weff, int D, int C, hipStream_t) { return line("glue_fold_in", V(Win), V(Wpre), V(Weff), D, C); }
int glue_fold_out(const float* Wout, const float* Wpost, float* Weff, int D, int C, hipStream_t) {
    return line("glue_fold_out", V(Wout), V(Wpost), V(Weff), D, C);
}
int glue_input_proj(const float* x, const float* Weff, float* X, int Bf, int xB, int C, int T, int S, int D, float xscale, hipStream_t) {
    return line("glue_input_proj", V(x), V(Weff), V(X), Bf, xB, C, T, S, D, (double)xscale);
}
int glue_input_proj_extra(const float* x, const float* Weff, float* X, int Bf, int xB, int C, int T, int S, int D, float xscale,
                          const float* concat, int Cc, int Tc, const float* prep, int P, hipStream_t) {
    return line("glue_input_proj_extra", V(x), V(Weff), V(X), Bf, xB, C, T, S, D, (double)xscale, V(concat), Cc, Tc, V(prep), P);
}
int glue_pos_table(int mode, const float* src, float* table, int rows, int D, hipStream_t) { return line("glue_pos_table", mode, V(src), V(table), rows, D); }
int glue_add_pos(float* X, const float* table, int Bf, int S, int D, hipStream_t) { return line("glue_add_pos", V(X), V(table), Bf, S, D); }
int glue_output_proj(const float* X, const float* Weff, float* out, int Bf, int C, int T, int S, int D, hipStream_t) {
    return line("glue_output_proj", V(X), V(Weff), V(out), Bf, C, T, S, D);
}
int glue_cfg_denoise(const float* mo, const float* x, float* den, int B, int C, int T, int use_cfg, float cfg_scale, float scale_phi, float c_out,
                     float c_skip, hipStream_t) {
    return line("glue_cfg_denoise", V(mo), V(x), V(den), B, C, T, use_cfg, (double)cfg_scale, (double)scale_phi, (double)c_out, (double)c_skip);
}
int glue_resid_stats(const float* X, int M, int D, float* out, hipStream_t) { return line("glue_resid_stats", V(X), M, D, V(out)); }

namespace bf16 {
int sat_launch_gemm(int epi, const GemmArgs& a, hipStream_t) {
    const HeadsEpi& h = a.heads;
    return line("sat_launch_gemm", epi, "f16", a.f16, "A", V(a.A), "W", V(a.W), "bias", V(a.bias), "MNK", a.M, a.N, a.K, "variant", a.variant, "C", V(a.C),
                a.ldc, a.accumulate, "fp8", a.fp8, V(a.a_scale), V(a.w_scale), V(a.a_bscale), "H8", V(a.H8), V(a.Hs), "gate", V(a.gate), a.gate_rows,
                a.gate_ld, "H", V(a.H), "heads", V(h.out[0]), V(h.out[1]), V(h.out[2]), h.kind[0], h.kind[1], h.kind[2], (double)h.qscale, "xa",
                V(h.xa_k), V(h.xa_vt), V(h.xa_out), h.xa_kvh, h.xa_sk, h.xa_sk_pad, "parts", h.parts, h.heads, h.S, h.Spad, "rope", V(h.rope_cos),
                V(h.rope_sin), "fold", V(a.xb), V(a.ln_part_out), V(a.ln_part), V(a.ln_c1), V(a.ln_c2), (double)a.ln_eps, "slab", V(a.slab), a.slab_bytes);
}
// the K-split scratch of the 8-phase FF-out GEMM: present at one shape of the cases (bf = 2, no prepend rows, "prepend" global token) and absent at
// the others, so both states of GemmArgs::slab are in the lists
size_t sat_gemm_ph8_slab_bytes(int epi, int M, int N, int K) { return epi == EPI_RESID && M == 28 ? (size_t)4 * 65536 * sizeof(float) : 0; }
int sat_launch_attention(const op_t* q, const op_t* k, const op_t* vt, op_t* out, int b, int h, int kvh, int sq, int sk, int sq_pad, int sk_pad,
                         hipStream_t, unsigned char* out_scales, float q_scale, int f16) {
    return line("sat_launch_attention", V(q), V(k), V(vt), V(out), b, h, kvh, sq, sk, sq_pad, sk_pad, V(out_scales), (double)q_scale, f16);
}
}  // namespace bf16

int sat_launch_layernorm(const float* x, const float* gamma, const float* beta, op_t* y, int m, int d, hipStream_t, int f16) {
    return line("sat_launch_layernorm", V(x), V(gamma), V(beta), V(y), m, d, f16);
}
int sat_launch_layernorm_mod(const float* x, const float* gamma, const float* beta, op_t* y, int m, int d, const float* scale1p, const float* shift,
                             int rows_per_seq, int ld, hipStream_t, int f16) {
    return line("sat_launch_layernorm_mod", V(x), V(gamma), V(beta), V(y), m, d, V(scale1p), V(shift), rows_per_seq, ld, f16);
}
int sat_launch_layernorm_fp8(const float* x, const float* gamma, const float* beta, void* y8, float* row_scale, int m, int d, const float* scale1p,
                             const float* shift, int rows_per_seq, int ld, hipStream_t) {
    return line("sat_launch_layernorm_fp8", V(x), V(gamma), V(beta), V(y8), V(row_scale), m, d, V(scale1p), V(shift), rows_per_seq, ld);
}
int sat_launch_quant_rows_fp8(const float* w, void* out8, float* row_scale, int n, int k, int swiglu_interleave, hipStream_t) {
    return line("sat_launch_quant_rows_fp8", V(w), V(out8), V(row_scale), n, k, swiglu_interleave);
}
int sat_launch_gemm_f32(const float* A, const float* W, const float* bias, float* C, int M, int N, int K, int ldc, int accumulate, const float* gate,
                        int gate_rows, int gate_ld, hipStream_t) {
    return line("sat_launch_gemm_f32", V(A), V(W), V(bias), V(C), M, N, K, ldc, accumulate, V(gate), gate_rows, gate_ld);
}
int sat_launch_layernorm_f32(const float* x, const float* gamma, const float* beta, float* y, int m, int d, const float* sc, const float* sh, int rps,
                             int ld, hipStream_t, float eps) {
    return line("sat_launch_layernorm_f32", V(x), V(gamma), V(beta), V(y), m, d, V(sc), V(sh), rps, ld, (double)eps);
}
int sat_launch_split_heads_f32(const float* src, float* d0, float* d1, float* d2, int M, int S, int parts, int H, int rope_mask, const float* rope_cos,
                               const float* rope_sin, hipStream_t, int norm_mask) {
    return line("sat_launch_split_heads_f32", V(src), V(d0), V(d1), V(d2), M, S, parts, H, rope_mask, V(rope_cos), V(rope_sin), norm_mask);
}
int sat_launch_swiglu_f32(const float* hg, float* h, int64_t M, int inner, hipStream_t) { return line("sat_launch_swiglu_f32", V(hg), V(h), (long long)M, inner); }
int sat_launch_attention_f32(const float* q, const float* k, const float* v, float* out, int b, int h, int kvh, int sq, int sk, hipStream_t) {
    return line("sat_launch_attention_f32", V(q), V(k), V(v), V(out), b, h, kvh, sq, sk);
}
int sat_launch_pack_rows_bf16(const float* w, op_t* out, int n, int k, int swiglu_interleave, hipStream_t, int f16) {
    return line("sat_launch_pack_rows_bf16", V(w), V(out), n, k, swiglu_interleave, f16);
}
int sat_launch_pack_bias(const float* b, float* out, int n, int swiglu_interleave, hipStream_t) { return line("sat_launch_pack_bias", V(b), V(out), n, swiglu_interleave); }
int sat_launch_pack_rows_ln(const float* w, const float* gamma, const float* beta, const float* bias, op_t* out, float* c1, float* c2, int n, int k,
                            int swiglu_interleave, hipStream_t, int f16) {
    return line("sat_launch_pack_rows_ln", V(w), V(gamma), V(beta), V(bias), V(out), V(c1), V(c2), n, k, swiglu_interleave, f16);
}
int sat_launch_rope_table(const float* inv_freq, float* cos_t, float* sin_t, int s_len, hipStream_t) {
    return line("sat_launch_rope_table", V(inv_freq), V(cos_t), V(sin_t), s_len);
}

// ------------------------------------------------------------------------------ the cases
namespace {

// The smallest model that reaches every branch of the plan: embed_dim 256 (the e4m3 modes' and the fold's lower limit), 4 heads, depth 2 (layer 0
// never folds its first LayerNorm, the last FF-out feeds nobody), FF inner 256, cross-attention from 16 to 128 channels (2 kv heads), 8 global channels
const int D = 256, HEADS = 4, DEPTH = 2, C = 8, INNER = 256, DCT = 16, DC = 128, DG = 8, TMAX = 64, T = 13, PREPEND_DIM = 8, TC = 7;

struct Case {
    const char* name;
    int gemm_dtype;
    int fp8_families = 0, ln_fold = 0, adaln = 0;
    bool cross = true;
    int cross_attention = 0, lc = 5, tile_policy = 0;
    int qk_norm = 0, pos_emb = SAT_DIT_POS_NONE, abs_max = 0, rotary = 1;
    bool ff_bias = true;
    int concat = 0, max_prep = 0, P = 0;
    int null_from = -1;
    bool debug = false, profile = false;
    bool skip_extra = false;          // refused: forward on an input-concat model without sat_dit_prepare_extra_conditioning
};

Case make(const char* name, int gemm_dtype, int ln_fold = 0) {
    Case c{};
    c.name = name; c.gemm_dtype = gemm_dtype; c.ln_fold = ln_fold;
    return c;
}
template <class F>
Case with(Case c, F f) {
    f(c);
    return c;
}

std::vector<Case> cases() {
    const int BF16 = SAT_GEMM_BF16, F8 = SAT_GEMM_FP8, F32 = SAT_GEMM_FP32X, F16 = SAT_GEMM_FP16;
    return {
        make("bf16", BF16),
        make("fp16", F16),
        make("fp32", F32),
        make("bf16_fold", BF16, 1),
        make("fp16_fold", F16, 1),
        make("fp8_default", F8),
        with(make("fp8_all", F8), [](Case& c) { c.fp8_families = SAT_FP8_ALL; }),
        with(make("fp8_ff_in", F8), [](Case& c) { c.fp8_families = SAT_FP8_FF_IN; }),
        with(make("fp8_qkv_to_out", F8), [](Case& c) { c.fp8_families = SAT_FP8_QKV | SAT_FP8_TO_OUT; }),
        with(make("fp8_fold_ignored", F8, 1), [](Case& c) {}),
        with(make("bf16_adaln", BF16), [](Case& c) { c.adaln = 1; }),
        with(make("fp16_adaln_fold_ignored", F16, 1), [](Case& c) { c.adaln = 1; }),
        with(make("fp32_adaln", F32), [](Case& c) { c.adaln = 1; }),
        with(make("fp8_all_adaln", F8), [](Case& c) { c.adaln = 1; c.fp8_families = SAT_FP8_ALL; }),
        with(make("fp16_fold_no_cross", F16, 1), [](Case& c) { c.cross = false; }),
        with(make("fp32_no_cross", F32), [](Case& c) { c.cross = false; }),
        with(make("fp16_lc200", F16), [](Case& c) { c.lc = 200; }),
        with(make("fp16_fold_lc200", F16, 1), [](Case& c) { c.lc = 200; }),
        with(make("fp8_all_lc200", F8), [](Case& c) { c.lc = 200; c.fp8_families = SAT_FP8_ALL; }),
        with(make("fp16_fold_two_kernels", F16, 1), [](Case& c) { c.cross_attention = 1; }),
        with(make("fp16_fold_tile_policy_22", F16, 1), [](Case& c) { c.tile_policy = 22; }),
        with(make("bf16_qk_norm", BF16), [](Case& c) { c.qk_norm = 1; }),
        with(make("fp16_fold_qk_norm", F16, 1), [](Case& c) { c.qk_norm = 1; }),
        with(make("fp32_qk_norm", F32), [](Case& c) { c.qk_norm = 1; }),
        with(make("fp16_fold_sinusoidal", F16, 1), [](Case& c) { c.pos_emb = SAT_DIT_POS_SINUSOIDAL; }),
        with(make("fp16_absolute", F16), [](Case& c) { c.pos_emb = SAT_DIT_POS_ABSOLUTE; c.abs_max = 40; }),
        with(make("fp16_fold_no_rotary", F16, 1), [](Case& c) { c.rotary = 0; }),
        with(make("fp16_fold_ff_no_bias", F16, 1), [](Case& c) { c.ff_bias = false; }),
        with(make("fp32_ff_no_bias", F32), [](Case& c) { c.ff_bias = false; }),
        with(make("fp8_ff_no_bias", F8), [](Case& c) { c.ff_bias = false; }),
        with(make("fp16_fold_concat4", F16, 1), [](Case& c) { c.concat = 4; }),
        with(make("fp16_fold_prepend_P0", F16, 1), [](Case& c) { c.max_prep = 3; }),
        with(make("fp16_fold_prepend_P2", F16, 1), [](Case& c) { c.max_prep = 3; c.P = 2; }),
        with(make("fp32_concat4_prepend_P2", F32), [](Case& c) { c.concat = 4; c.max_prep = 3; c.P = 2; }),
        with(make("fp16_fold_null_from_1", F16, 1), [](Case& c) { c.null_from = 1; }),
        with(make("fp8_all_null_from_1", F8), [](Case& c) { c.null_from = 1; c.fp8_families = SAT_FP8_ALL; }),
        with(make("fp32_null_from_1", F32), [](Case& c) { c.null_from = 1; }),
        with(make("fp16_fold_null_from_0", F16, 1), [](Case& c) { c.null_from = 0; }),
        with(make("fp16_fold_debug", F16, 1), [](Case& c) { c.debug = true; }),
        with(make("fp16_fold_profile", F16, 1), [](Case& c) { c.profile = true; }),
        // refused configurations: the return codes are the record
        with(make("refused_qk_norm_fp8", F8), [](Case& c) { c.qk_norm = 1; }),
        with(make("refused_ff_out_without_ff_in", F8), [](Case& c) { c.fp8_families = SAT_FP8_FF_OUT; }),
        with(make("refused_forward_before_extra_conditioning", F16, 1), [](Case& c) { c.concat = 4; c.skip_extra = true; }),
        with(make("refused_absolute_position_too_long", F16), [](Case& c) { c.pos_emb = SAT_DIT_POS_ABSOLUTE; c.abs_max = 10; }),
    };
}

void set_tensors(sat_dit_plan* p, const Case& c, Inputs& in) {
    auto t = [&](const std::string& name, size_t n) { sat_dit_plan_set_tensor(p, name.c_str(), in.make(name, n), (int64_t)n); };
    const int Ci = C + c.concat;
    t("timestep_features.weight", 128);
    t("to_timestep_embed.0.weight", D * 256); t("to_timestep_embed.0.bias", D);
    t("to_timestep_embed.2.weight", D * D); t("to_timestep_embed.2.bias", D);
    if (c.cross) { t("to_cond_embed.0.weight", DC * DCT); t("to_cond_embed.2.weight", DC * DC); }
    t("to_global_embed.0.weight", D * DG); t("to_global_embed.2.weight", D * D);
    if (c.max_prep) { t("to_prepend_embed.0.weight", D * PREPEND_DIM); t("to_prepend_embed.2.weight", D * D); }
    if (c.rotary) t("transformer.rotary_pos_emb.inv_freq", 16);
    if (c.pos_emb == SAT_DIT_POS_SINUSOIDAL) t("transformer.pos_emb.scale", 1);
    if (c.pos_emb == SAT_DIT_POS_ABSOLUTE) t("transformer.pos_emb.emb.weight", (size_t)c.abs_max * D);
    t("transformer.project_in.weight", D * Ci); t("preprocess_conv.weight", Ci * Ci);
    t("transformer.project_out.weight", D * C); t("postprocess_conv.weight", C * C);
    for (int l = 0; l < DEPTH; ++l) {
        const std::string pf = "transformer.layers." + std::to_string(l) + ".";
        if (c.adaln) t(pf + "to_scale_shift_gate.1.weight", 6 * D * D);
        t(pf + "pre_norm.gamma", D); t(pf + "pre_norm.beta", D);
        t(pf + "ff_norm.gamma", D); t(pf + "ff_norm.beta", D);
        t(pf + "self_attn.to_qkv.weight", 3 * D * D); t(pf + "self_attn.to_out.weight", D * D);
        if (c.cross) {
            t(pf + "cross_attend_norm.gamma", D); t(pf + "cross_attend_norm.beta", D);
            t(pf + "cross_attn.to_q.weight", D * D); t(pf + "cross_attn.to_kv.weight", 2 * DC * DC); t(pf + "cross_attn.to_out.weight", D * D);
        }
        t(pf + "ff.ff.0.proj.weight", 2 * INNER * D); t(pf + "ff.ff.0.proj.bias", 2 * INNER);
        t(pf + "ff.ff.2.weight", D * INNER);
        if (c.ff_bias) t(pf + "ff.ff.2.bias", D);
    }
}

// one generation of `bf` sequences: the prepare calls, then sat_dit_forward (bf == 2 only) and sat_dit_denoise_cfg of one prompt
void generation(sat_dit_plan* p, const Case& c, int bf, float cfg_scale, bool forward) {
    Inputs in;
    hipStream_t s = (hipStream_t)(uintptr_t)0x100;
    RC(sat_dit_prepare_context, p, c.cross ? in.make("cond", (size_t)bf * c.lc * DCT) : nullptr, bf, c.cross ? c.lc : 0, in.make("global_cond", (size_t)bf * DG), s);
    if ((c.concat || c.max_prep) && !c.skip_extra)
        RC(sat_dit_prepare_extra_conditioning, p, c.concat ? in.make("input_concat", (size_t)bf * c.concat * TC) : nullptr, c.concat ? TC : 0,
                                              c.P ? in.make("prepend", (size_t)bf * c.P * PREPEND_DIM) : nullptr, c.P, bf, s);
    if (c.null_from >= 0 && c.null_from <= bf) RC(sat_dit_set_null_context_from, p, c.null_from);
    size_t bytes = 0;
    RC(sat_dit_workspace_bytes, p, bf, T, &bytes);
    line("workspace_bytes", bytes);
    void* ws = in.workspace(bytes);
    float* x = in.make("x", (size_t)bf * C * T);
    if (forward) RC(sat_dit_forward, p, x, in.make("t", bf), in.make("out", (size_t)bf * C * T), bf, T, ws, bytes, s);
    RC(sat_dit_denoise_cfg, p, x, 1.5f, cfg_scale, 0.25f, in.make("denoised", (size_t)C * T), 1, T, ws, bytes, s);
}

void run(const Case& c) {
    sat_dit_cfg cfg{};
    cfg.io_channels = C; cfg.embed_dim = D; cfg.depth = DEPTH; cfg.num_heads = HEADS;
    cfg.cond_token_dim = c.cross ? DCT : 0; cfg.cond_embed_dim = c.cross ? DC : 0; cfg.global_cond_dim = DG; cfg.max_seq_len = TMAX;
    cfg.adaln = c.adaln; cfg.gemm_dtype = c.gemm_dtype; cfg.fp8_families = c.fp8_families; cfg.ln_fold = c.ln_fold;
    cfg.cross_attention = c.cross_attention; cfg.tile_policy = c.tile_policy;
    sat_dit_plan* p = nullptr;
    if (RC(sat_dit_plan_create_sized, &cfg, sizeof cfg, &p), !p) return;
    Inputs weights;
    hipStream_t s = (hipStream_t)(uintptr_t)0x100;
    bool ok = true;
    if (c.concat || c.max_prep) RC(sat_dit_plan_set_extra_conditioning, p, c.concat, c.max_prep ? PREPEND_DIM : 0, c.max_prep);
    if (c.qk_norm || c.pos_emb || !c.rotary) {
        sat_dit_transformer_options o{c.qk_norm, c.pos_emb, c.abs_max, c.rotary};
        const int rc = sat_dit_plan_set_transformer_options(p, &o, sizeof o);
        line("rc sat_dit_plan_set_transformer_options", rc);
        ok = rc == 0;
    }
    if (ok) {
        set_tensors(p, c, weights);
        RC(sat_dit_plan_finalize, p, s);
        if (c.debug) RC(sat_dit_debug, p, 1);
        if (c.profile) RC(sat_dit_profile, p, 1);
        generation(p, c, 2, 3.0f, true);
        generation(p, c, 1, 1.0f, false);
        if (c.profile) {
            double ms = 0;
            int32_t n = 0;
            int64_t m = 0, nn = 0, k = 0;
            RC(sat_dit_profile_read, p, &ms, &n, &m, &nn, &k);
            line("profile", ms, (int)n, (long long)m, (long long)nn, (long long)k);
        }
        if (c.debug) RC(sat_dit_debug, p, 0);
    }
    sat_dit_plan_destroy(p);
}

}  // namespace

int main() {
    for (const Case& c : cases()) {
        g_allocs = 0;
        line("==", c.name);
        run(c);
    }
    return 0;
}
