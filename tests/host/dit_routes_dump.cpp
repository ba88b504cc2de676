// Host driver of tests/test_dit_routes_host.py: the routes of the DiT plan (csrc/dit_plan.hip) that dit_launch_dump.cpp cannot reach, on the CPU.
// That driver defines the launchers of the 64-channel routes and leaves the later ones -- declared weak in sat_common.h / dit_glue.h -- null, so a
// plan with 128-, 32- or 96-channel heads, causal attention, the range report, block options, a convolutional feed-forward or a patch size is
// refused there.  This one defines them, each as a function that prints its arguments, on top of the runtime and the launchers of
// dit_launch_dump.cpp, included below with its main() and its cases set aside: built and linked exactly like that driver (hipcc
// --cuda-host-only, no HIP runtime on the link line).
//   dit_routes_dump            every case, each behind a line "== <name>"
#define main dit_launch_dump_main
#include "dit_launch_dump.cpp"
#undef main

// ------------------------------------------------------------------------------ the launchers dit_launch_dump.cpp leaves null
namespace {
// the record of the range report a launch accumulates into, as (layer, slot): the plan's one buffer of [depth][SAT_DIT_RANGE_SLOTS] records
void put_record(std::string& o, const sat_range_record* rec) {
    for (const Range& r : g_ranges)
        if ((const char*)rec >= r.base && (const char*)rec < r.base + r.size) {
            const size_t i = (size_t)((const char*)rec - r.base) / sizeof(sat_range_record);
            o += " layer " + std::to_string(i / SAT_DIT_RANGE_SLOTS) + " slot " + sat_dit_range_slot_name((int32_t)(i % SAT_DIT_RANGE_SLOTS));
            return;
        }
    o += " layer unknown";
}
// RC that also hands the code back: the setters' refusals end a case
int rc_of(const char* name, int rc) {
    line(name, rc);
    return rc;
}
#define RC_OF(fn, ...) rc_of("rc " #fn, (int)fn(__VA_ARGS__))
}  // namespace

namespace bf16 {
int sat_launch_attention_hdw(const op_t* q, const op_t* k, const op_t* vt, op_t* out, int b, int h, int kvh, int head_dim, int sq, int sk, int sq_pad,
                             int sk_pad, hipStream_t, int f16) {
    return line("sat_launch_attention_hdw", V(q), V(k), V(vt), V(out), b, h, kvh, head_dim, sq, sk, sq_pad, sk_pad, "f16", f16);
}
int sat_launch_head_split_hdw(const float* x, const HeadsEpi& h, int head_dim, int b, hipStream_t, int f16) {
    return line("sat_launch_head_split_hdw", V(x), "heads", V(h.out[0]), V(h.out[1]), V(h.out[2]), h.kind[0], h.kind[1], h.kind[2], (double)h.qscale, "xa",
                V(h.xa_k), V(h.xa_vt), V(h.xa_out), h.xa_kvh, h.xa_sk, h.xa_sk_pad, "parts", h.parts, h.heads, h.S, h.Spad, "rope", V(h.rope_cos),
                V(h.rope_sin), "head_dim", head_dim, b, "f16", f16);
}
int sat_launch_attention_causal(const op_t* q, const op_t* k, const op_t* vt, op_t* out, int b, int h, int kvh, int s_len, int sq_pad, int sk_pad,
                                hipStream_t, float q_scale, int f16) {
    return line("sat_launch_attention_causal", V(q), V(k), V(vt), V(out), b, h, kvh, s_len, sq_pad, sk_pad, (double)q_scale, "f16", f16);
}
int sat_launch_attention_hdw_causal(const op_t* q, const op_t* k, const op_t* vt, op_t* out, int b, int h, int kvh, int head_dim, int s_len, int sq_pad,
                                    int sk_pad, hipStream_t, int f16) {
    return line("sat_launch_attention_hdw_causal", V(q), V(k), V(vt), V(out), b, h, kvh, head_dim, s_len, sq_pad, sk_pad, "f16", f16);
}
}  // namespace bf16

int sat_launch_rope_table_hdw(const float* inv_freq, float* cos_t, float* sin_t, int s_len, int head_dim, hipStream_t) {
    return line("sat_launch_rope_table_hdw", V(inv_freq), V(cos_t), V(sin_t), s_len, head_dim);
}
int sat_launch_range_stats(const void* x, int dtype, int64_t rows, int64_t cols, int64_t pitch, uint64_t counted, sat_range_record* rec, hipStream_t) {
    std::string where;
    put_record(where, rec);
    return line("sat_launch_range_stats", V(x), dtype, (long long)rows, (long long)cols, (long long)pitch, (size_t)counted, V(rec), where.c_str() + 1);
}
int sat_launch_dwconv_ln_silu(const void* x, const float* w, const float* gamma, const float* beta, void* y, int b, int s_len, int d, int fmt, hipStream_t) {
    return line("sat_launch_dwconv_ln_silu", V(x), V(w), V(gamma), V(beta), V(y), b, s_len, d, fmt);
}
int sat_launch_round_rows(const float* x, void* y, int m, int d, const float* scale1p, const float* shift, int rows_per_seq, int ld, int fmt, hipStream_t) {
    return line("sat_launch_round_rows", V(x), V(y), m, d, V(scale1p), V(shift), rows_per_seq, ld, fmt);
}
int sat_launch_silu_f32(float* h, int64_t n, hipStream_t) { return line("sat_launch_silu_f32", V(h), (long long)n); }
int sat_launch_ff_conv(const FfConvArgs& a, hipStream_t) {
    return line("sat_launch_ff_conv", "fmt", a.fmt, "A", V(a.A), "W", V(a.W), "bias", V(a.bias), "BSNK", a.B, a.S, a.N, a.K, "taps", a.taps, "epi", a.epi, "C",
                V(a.C), a.ldc, a.accumulate, "gate", V(a.gate), a.gate_rows, a.gate_ld, "H", V(a.H), "act", a.act);
}
int sat_launch_pack_conv_taps(const float* w, void* out, int n, int k, int taps, int fmt, hipStream_t) {
    return line("sat_launch_pack_conv_taps", V(w), V(out), n, k, taps, fmt);
}
int sat_launch_im2col_rows_f32(const float* a, float* out, int b, int s_len, int k, int taps, hipStream_t) {
    return line("sat_launch_im2col_rows_f32", V(a), V(out), b, s_len, k, taps);
}
int sat_launch_split_heads_f32_w(const float* src, float* d0, float* d1, float* d2, int M, int S, int parts, int H, int head_dim, int rope_mask,
                                 const float* rope_cos, const float* rope_sin, hipStream_t, int norm_mask) {
    return line("sat_launch_split_heads_f32_w", V(src), V(d0), V(d1), V(d2), M, S, parts, H, head_dim, rope_mask, V(rope_cos), V(rope_sin), norm_mask);
}
int sat_launch_attention_f32_w(const float* q, const float* k, const float* v, float* out, int b, int h, int kvh, int head_dim, int sq, int sk, hipStream_t) {
    return line("sat_launch_attention_f32_w", V(q), V(k), V(v), V(out), b, h, kvh, head_dim, sq, sk);
}
int sat_launch_attention_f32_causal(const float* q, const float* k, const float* v, float* out, int b, int h, int kvh, int head_dim, int s_len, hipStream_t) {
    return line("sat_launch_attention_f32_causal", V(q), V(k), V(v), V(out), b, h, kvh, head_dim, s_len);
}
int glue_fold_in_patch(const float* Win, const float* Wpre, float* Weff, int D, int Ci, int P, hipStream_t) {
    return line("glue_fold_in_patch", V(Win), V(Wpre), V(Weff), D, Ci, P);
}
int glue_fold_out_patch(const float* Wout, const float* Wpost, float* Weff, int D, int C, int P, hipStream_t) {
    return line("glue_fold_out_patch", V(Wout), V(Wpost), V(Weff), D, C, P);
}
int glue_input_proj_patch(const float* x, const float* Weff, float* X, int Bf, int xB, int C, int P, int T, int S, int D, float xscale, const float* concat,
                          int Cc, int Tc, const float* prep, int Pl, hipStream_t) {
    return line("glue_input_proj_patch", V(x), V(Weff), V(X), Bf, xB, C, P, T, S, D, (double)xscale, V(concat), Cc, Tc, V(prep), Pl);
}
int glue_output_proj_patch(const float* X, const float* Weff, float* out, int Bf, int C, int P, int T, int S, int D, hipStream_t) {
    return line("glue_output_proj_patch", V(X), V(Weff), V(out), Bf, C, P, T, S, D);
}

// ------------------------------------------------------------------------------ the cases
namespace {

// The smallest models that reach each branch, on the constants of dit_launch_dump.cpp (8 io channels, FF inner 256, context tokens of 16 channels, 8
// global channels, T = 13): 64-channel heads as there (embed_dim 256, 4 heads, context 128 = 2 kv heads); 128- and 32-channel heads at embed_dim
// 256 with 2 and 8 heads (context 128 = 1 and 4 kv heads); 96-channel heads at embed_dim 384 with 4 heads (context 192 = 2 kv heads).  Depth 2, or 3
// where a block format boundary is needed
struct Route {
    const char* name;
    int hd, gemm_dtype, ln_fold = 0;
    bool create_ex = false;           // sat_dit_plan_create_ex with head_widths 1 (what admits 32 and 96), else sat_dit_plan_create_sized
    std::vector<int32_t> formats;     // sat_dit_plan_set_block_formats: depth 3
    int adaln = 0;
    bool cross = true;
    int cross_attention = 0, lc = 5;
    int qk_norm = 0, rotary = 1;
    int concat = 0, max_prep = 0, P = 0;
    int null_from = -1;
    bool debug = false;
    int causal = 0;
    int range_report = 0;             // sat_dit_range_report(p, 1) behind finalize
    int conformer = 0, remove_norms = 0, ff_glu = 1;
    int ff_conv = 1;
    int patch = 1, t_len = T;

    int depth() const { return formats.empty() ? DEPTH : (int)formats.size(); }
    int dim() const { return hd == 96 ? 384 : 256; }
    int heads() const { return dim() / hd; }
    int dc() const { return hd == 96 ? 192 : 128; }
};

Route route(const char* name, int hd, int gemm_dtype, int ln_fold = 0) {
    Route r{};
    r.name = name; r.hd = hd; r.gemm_dtype = gemm_dtype; r.ln_fold = ln_fold;
    r.create_ex = hd == 32 || hd == 96;
    return r;
}
template <class F>
Route with(Route r, F f) {
    f(r);
    return r;
}

std::vector<Route> routes() {
    const int BF16 = SAT_GEMM_BF16, F8 = SAT_GEMM_FP8, F32 = SAT_GEMM_FP32X, F16 = SAT_GEMM_FP16;
    auto causal = [](Route& r) { r.causal = 1; r.cross = false; };
    return {
        // ---- staged widths, 16-bit operands
        route("hd128_fp16", 128, F16),
        route("hd128_bf16", 128, BF16),
        route("hd128_fp16_fold_ignored", 128, F16, 1),
        with(route("hd128_fp16_qk_norm", 128, F16), [](Route& r) { r.qk_norm = 1; }),
        with(route("hd128_fp16_no_rotary", 128, F16), [](Route& r) { r.rotary = 0; }),
        with(route("hd128_fp16_no_cross", 128, F16), [](Route& r) { r.cross = false; }),
        with(route("hd128_bf16_adaln", 128, BF16), [](Route& r) { r.adaln = 1; }),
        with(route("hd128_fp16_null_from_1", 128, F16), [](Route& r) { r.null_from = 1; }),
        with(route("hd128_fp16_lc200", 128, F16), [](Route& r) { r.lc = 200; }),
        with(route("hd128_fp16_debug", 128, F16), [](Route& r) { r.debug = true; }),
        route("hd32_fp16", 32, F16),
        route("hd96_bf16", 96, BF16),
        with(route("hd32_fp16_lc200", 32, F16), [](Route& r) { r.lc = 200; }),
        with(route("hd96_mixed_formats", 96, F16), [&](Route& r) { r.formats = {F16, BF16, F16}; }),
        // ---- staged widths, fp32 verification mode
        route("hd32_fp32", 32, F32),
        route("hd96_fp32", 96, F32),
        with(route("hd96_fp32_qk_norm", 96, F32), [](Route& r) { r.qk_norm = 1; }),
        with(route("hd32_fp32_no_cross", 32, F32), [](Route& r) { r.cross = false; }),
        // ---- causal
        with(route("causal_fp16_fold", 64, F16, 1), causal),
        with(route("causal_fp16", 64, F16), causal),
        with(route("causal_fp32", 64, F32), causal),
        with(route("causal_hd128_fp16", 128, F16), causal),
        with(route("causal_hd32_fp32", 32, F32), causal),
        with(route("causal_fp16_adaln", 64, F16), [&](Route& r) { causal(r); r.adaln = 1; }),
        with(route("causal_fp16_fold_prepend_P2", 64, F16, 1), [&](Route& r) { causal(r); r.max_prep = 3; r.P = 2; }),
        // ---- range report on
        with(route("range_fp16_fold_fused", 64, F16, 1), [](Route& r) { r.range_report = 1; }),
        with(route("range_fp16_fold_two_kernels", 64, F16, 1), [](Route& r) { r.range_report = 1; r.cross_attention = 1; }),
        with(route("range_hd128_fp16", 128, F16), [](Route& r) { r.range_report = 1; }),
        with(route("range_mixed_formats_fold", 64, F16, 1), [&](Route& r) { r.range_report = 1; r.formats = {F16, BF16, F16}; }),
        // ---- block options, 64-channel heads
        with(route("conformer_fp16_fold", 64, F16, 1), [](Route& r) { r.conformer = 1; }),
        with(route("remove_norms_fp16_fold", 64, F16, 1), [](Route& r) { r.remove_norms = 1; }),
        with(route("ff_glu0_fp16_fold", 64, F16, 1), [](Route& r) { r.ff_glu = 0; }),
        with(route("conformer_fp32", 64, F32), [](Route& r) { r.conformer = 1; }),
        with(route("remove_norms_fp32", 64, F32), [](Route& r) { r.remove_norms = 1; }),
        with(route("ff_glu0_fp32", 64, F32), [](Route& r) { r.ff_glu = 0; }),
        with(route("conformer_fp16_adaln", 64, F16), [](Route& r) { r.conformer = 1; r.adaln = 1; }),
        // ---- convolutional feed-forward
        with(route("ff_conv3_glu_fp16", 64, F16, 1), [](Route& r) { r.ff_conv = 3; }),
        with(route("ff_conv3_no_glu_bf16", 64, BF16), [](Route& r) { r.ff_conv = 3; r.ff_glu = 0; }),
        with(route("ff_conv3_glu_fp32", 64, F32), [](Route& r) { r.ff_conv = 3; }),
        with(route("ff_conv3_no_glu_fp32", 64, F32), [](Route& r) { r.ff_conv = 3; r.ff_glu = 0; }),
        // ---- patch
        with(route("patch2_fp16_fold", 64, F16, 1), [](Route& r) { r.patch = 2; r.t_len = 12; }),
        with(route("patch2_fp16_fold_concat4_prepend_P2", 64, F16, 1), [](Route& r) { r.patch = 2; r.t_len = 12; r.concat = 4; r.max_prep = 3; r.P = 2; }),
        with(route("patch2_fp32", 64, F32), [](Route& r) { r.patch = 2; r.t_len = 12; }),
        // ---- refused configurations: the return codes and the error texts are the record
        with(route("refused_hd32_create_sized", 32, F16), [](Route& r) { r.create_ex = false; }),
        route("refused_hd32_fp8", 32, F8),
        route("refused_hd128_fp8", 128, F8),
        route("refused_hd128_fp32", 128, F32),
        with(route("refused_block_options_hd128", 128, F16), [](Route& r) { r.conformer = 1; }),
        with(route("refused_block_options_hd96", 96, F16), [](Route& r) { r.ff_glu = 0; }),
        with(route("refused_ff_conv_hd32", 32, F16), [](Route& r) { r.ff_conv = 3; }),
        with(route("refused_causal_cross", 64, F16), [](Route& r) { r.causal = 1; }),
        with(route("refused_causal_fp8", 64, F8), causal),
        with(route("refused_range_report_conformer", 64, F16, 1), [](Route& r) { r.conformer = 1; r.range_report = 1; }),
        with(route("refused_t_len_not_multiple_of_patch", 64, F16, 1), [](Route& r) { r.patch = 2; }),
    };
}

void set_route_tensors(sat_dit_plan* p, const Route& c, Inputs& in) {
    auto t = [&](const std::string& name, size_t n) { sat_dit_plan_set_tensor(p, name.c_str(), in.make(name, n), (int64_t)n); };
    const int Dm = c.dim(), Dc = c.dc(), Ci = C + c.concat, k = c.ff_conv;
    t("timestep_features.weight", 128);
    t("to_timestep_embed.0.weight", Dm * 256); t("to_timestep_embed.0.bias", Dm);
    t("to_timestep_embed.2.weight", Dm * Dm); t("to_timestep_embed.2.bias", Dm);
    if (c.cross) { t("to_cond_embed.0.weight", Dc * DCT); t("to_cond_embed.2.weight", Dc * Dc); }
    t("to_global_embed.0.weight", Dm * DG); t("to_global_embed.2.weight", Dm * Dm);
    if (c.max_prep) { t("to_prepend_embed.0.weight", Dm * PREPEND_DIM); t("to_prepend_embed.2.weight", Dm * Dm); }
    if (c.rotary) t("transformer.rotary_pos_emb.inv_freq", sat_rope_pairs(c.hd));
    t("transformer.project_in.weight", Dm * Ci * c.patch); t("preprocess_conv.weight", Ci * Ci);
    t("transformer.project_out.weight", Dm * C * c.patch); t("postprocess_conv.weight", C * C);
    for (int l = 0; l < c.depth(); ++l) {
        const std::string pf = "transformer.layers." + std::to_string(l) + ".";
        if (c.adaln) t(pf + "to_scale_shift_gate.1.weight", 6 * Dm * Dm);
        if (!c.remove_norms) {
            t(pf + "pre_norm.gamma", Dm); t(pf + "pre_norm.beta", Dm);
            t(pf + "ff_norm.gamma", Dm); t(pf + "ff_norm.beta", Dm);
        }
        t(pf + "self_attn.to_qkv.weight", 3 * Dm * Dm); t(pf + "self_attn.to_out.weight", Dm * Dm);
        if (c.cross) {
            if (!c.remove_norms) { t(pf + "cross_attend_norm.gamma", Dm); t(pf + "cross_attend_norm.beta", Dm); }
            t(pf + "cross_attn.to_q.weight", Dm * Dm); t(pf + "cross_attn.to_kv.weight", 2 * Dc * Dc); t(pf + "cross_attn.to_out.weight", Dm * Dm);
        }
        if (c.conformer) {
            t(pf + "conformer.in_norm.gamma", Dm); t(pf + "conformer.in_norm.beta", Dm);
            t(pf + "conformer.mid_norm.gamma", Dm); t(pf + "conformer.mid_norm.beta", Dm);
            t(pf + "conformer.depthwise_conv.weight", Dm * 17);
            t(pf + "conformer.pointwise_conv.weight", Dm * Dm); t(pf + "conformer.pointwise_conv_2.weight", Dm * Dm);
            t(pf + "conformer.glu.proj.weight", 2 * Dm * Dm); t(pf + "conformer.glu.proj.bias", 2 * Dm);
        }
        if (c.ff_glu) { t(pf + "ff.ff.0.proj.weight", 2 * INNER * Dm); t(pf + "ff.ff.0.proj.bias", 2 * INNER); }
        else { t(pf + "ff.ff.0.1.weight", INNER * Dm * k); t(pf + "ff.ff.0.1.bias", INNER); }
        t(pf + "ff.ff.2.weight", Dm * INNER * k); t(pf + "ff.ff.2.bias", Dm);
    }
}

// one generation of two sequences, as generation() of dit_launch_dump.cpp: the prepare calls, then sat_dit_forward and sat_dit_denoise_cfg of
// one prompt at CFG 3 (a plan without cross-attention or prepend rows runs no CFG and refuses the one sequence: the code is the record)
void route_generation(sat_dit_plan* p, const Route& c) {
    const int bf = 2;
    Inputs in;
    hipStream_t s = (hipStream_t)(uintptr_t)0x100;
    const int Tl = c.t_len;
    RC(sat_dit_prepare_context, p, c.cross ? in.make("cond", (size_t)bf * c.lc * DCT) : nullptr, bf, c.cross ? c.lc : 0, in.make("global_cond", (size_t)bf * DG), s);
    if (c.concat || c.max_prep)
        RC(sat_dit_prepare_extra_conditioning, p, c.concat ? in.make("input_concat", (size_t)bf * c.concat * TC) : nullptr, c.concat ? TC : 0,
                                              c.P ? in.make("prepend", (size_t)bf * c.P * PREPEND_DIM) : nullptr, c.P, bf, s);
    if (c.null_from >= 0 && c.null_from <= bf) RC(sat_dit_set_null_context_from, p, c.null_from);
    size_t bytes = 0;
    RC(sat_dit_workspace_bytes, p, bf, Tl, &bytes);
    line("workspace_bytes", bytes);
    void* ws = in.workspace(bytes);
    float* x = in.make("x", (size_t)bf * C * Tl);
    RC(sat_dit_forward, p, x, in.make("t", bf), in.make("out", (size_t)bf * C * Tl), bf, Tl, ws, bytes, s);
    RC(sat_dit_denoise_cfg, p, x, 1.5f, 3.0f, 0.25f, in.make("denoised", (size_t)C * Tl), 1, Tl, ws, bytes, s);
}

// every setter the case asks for, in the order the Python package calls them; false behind the first refusal
bool set_options(sat_dit_plan* p, const Route& c) {
    if (!c.formats.empty() && RC_OF(sat_dit_plan_set_block_formats, p, c.formats.data(), (int32_t)c.formats.size())) return false;
    if ((c.concat || c.max_prep) && RC_OF(sat_dit_plan_set_extra_conditioning, p, c.concat, c.max_prep ? PREPEND_DIM : 0, c.max_prep)) return false;
    if (c.qk_norm || !c.rotary) {
        sat_dit_transformer_options o{c.qk_norm, SAT_DIT_POS_NONE, 0, c.rotary};
        if (RC_OF(sat_dit_plan_set_transformer_options, p, &o, sizeof o)) return false;
    }
    if (c.conformer || c.remove_norms || !c.ff_glu) {
        sat_dit_block_options o{c.conformer, c.remove_norms, c.ff_glu};
        if (RC_OF(sat_dit_plan_set_block_options, p, &o, sizeof o)) return false;
    }
    if (c.ff_conv > 1) {
        sat_dit_ff_conv_options o{c.ff_conv};
        if (RC_OF(sat_dit_plan_set_ff_conv, p, &o, sizeof o)) return false;
    }
    if (c.patch > 1) {
        sat_dit_patch_options o{c.patch};
        if (RC_OF(sat_dit_plan_set_patch, p, &o, sizeof o)) return false;
    }
    if (c.causal) {
        sat_dit_attention_options o{c.causal};
        if (RC_OF(sat_dit_plan_set_attention_options, p, &o, sizeof o)) return false;
    }
    return true;
}

void run_route(const Route& c) {
    sat_dit_cfg cfg{};
    cfg.io_channels = C; cfg.embed_dim = c.dim(); cfg.depth = c.depth(); cfg.num_heads = c.heads();
    cfg.cond_token_dim = c.cross ? DCT : 0; cfg.cond_embed_dim = c.cross ? c.dc() : 0; cfg.global_cond_dim = DG; cfg.max_seq_len = TMAX;
    cfg.adaln = c.adaln; cfg.gemm_dtype = c.gemm_dtype; cfg.ln_fold = c.ln_fold; cfg.cross_attention = c.cross_attention;
    sat_dit_plan* p = nullptr;
    sat_dit_create_options opt{1};
    if (c.create_ex) RC(sat_dit_plan_create_ex, &cfg, sizeof cfg, &opt, sizeof opt, &p);
    else RC(sat_dit_plan_create_sized, &cfg, sizeof cfg, &p);
    if (!p) return;
    hipStream_t s = (hipStream_t)(uintptr_t)0x100;
    if (set_options(p, c)) {
        {
            Inputs weights;
            set_route_tensors(p, c, weights);
            RC(sat_dit_plan_finalize, p, s);
        }
        if (c.debug) RC(sat_dit_debug, p, 1);
        if (c.range_report) RC(sat_dit_range_report, p, 1);
        route_generation(p, c);
        if (c.range_report) RC(sat_dit_range_report, p, 0);
        if (c.debug) RC(sat_dit_debug, p, 0);
    }
    sat_dit_plan_destroy(p);
}

}  // namespace

int main() {
    for (const Route& c : routes()) {
        g_allocs = 0;
        line("==", c.name);
        run_route(c);
    }
    return 0;
}
