// Host driver of tests/test_block_formats_host.py: a depth-3 DiT plan with an operand format per block (sat_dit_plan_set_block_formats) on the
// CPU.  The HIP runtime on host memory and every launcher of the plan are the ones of dit_launch_dump.cpp, included below with its main() and
// its cases set aside: built and linked exactly like that driver (hipcc --cuda-host-only, no HIP runtime on the link line).
//   block_formats_dump            every case, each behind a line "== <name>"
#define main dit_launch_dump_main
#include "dit_launch_dump.cpp"
#undef main

namespace {

const int DEPTH3 = 3;
const int F16 = SAT_GEMM_FP16, BF16 = SAT_GEMM_BF16;

struct FormatCase {
    const char* name;
    int gemm_dtype, ln_fold;
    std::vector<int32_t> formats;          // empty: the plan never gets the call
    int adaln = 0;
    int fp8_families = 0;
    bool after_finalize = false;           // the call once more behind finalize: SAT_E_STATE
};

// every tensor of a cross-attention "prepend" (or adaLN) plan of the constants above, DEPTH3 layers
void set_tensors3(sat_dit_plan* p, const FormatCase& c, Inputs& in) {
    auto t = [&](const std::string& name, size_t n) { sat_dit_plan_set_tensor(p, name.c_str(), in.make(name, n), (int64_t)n); };
    t("timestep_features.weight", 128);
    t("to_timestep_embed.0.weight", D * 256); t("to_timestep_embed.0.bias", D);
    t("to_timestep_embed.2.weight", D * D); t("to_timestep_embed.2.bias", D);
    t("to_cond_embed.0.weight", DC * DCT); t("to_cond_embed.2.weight", DC * DC);
    t("to_global_embed.0.weight", D * DG); t("to_global_embed.2.weight", D * D);
    t("transformer.rotary_pos_emb.inv_freq", 16);
    t("transformer.project_in.weight", D * C); t("preprocess_conv.weight", C * C);
    t("transformer.project_out.weight", D * C); t("postprocess_conv.weight", C * C);
    for (int l = 0; l < DEPTH3; ++l) {
        const std::string pf = "transformer.layers." + std::to_string(l) + ".";
        if (c.adaln) t(pf + "to_scale_shift_gate.1.weight", 6 * D * D);
        t(pf + "pre_norm.gamma", D); t(pf + "pre_norm.beta", D);
        t(pf + "ff_norm.gamma", D); t(pf + "ff_norm.beta", D);
        t(pf + "self_attn.to_qkv.weight", 3 * D * D); t(pf + "self_attn.to_out.weight", D * D);
        t(pf + "cross_attend_norm.gamma", D); t(pf + "cross_attend_norm.beta", D);
        t(pf + "cross_attn.to_q.weight", D * D); t(pf + "cross_attn.to_kv.weight", 2 * DC * DC); t(pf + "cross_attn.to_out.weight", D * D);
        t(pf + "ff.ff.0.proj.weight", 2 * INNER * D); t(pf + "ff.ff.0.proj.bias", 2 * INNER);
        t(pf + "ff.ff.2.weight", D * INNER); t(pf + "ff.ff.2.bias", D);
    }
}

void run3(const FormatCase& c) {
    sat_dit_cfg cfg{};
    cfg.io_channels = C; cfg.embed_dim = D; cfg.depth = DEPTH3; cfg.num_heads = HEADS;
    cfg.cond_token_dim = DCT; cfg.cond_embed_dim = DC; cfg.global_cond_dim = DG; cfg.max_seq_len = TMAX;
    cfg.adaln = c.adaln; cfg.gemm_dtype = c.gemm_dtype; cfg.fp8_families = c.fp8_families; cfg.ln_fold = c.ln_fold;
    sat_dit_plan* p = nullptr;
    if (RC(sat_dit_plan_create_sized, &cfg, sizeof cfg, &p), !p) return;
    hipStream_t s = (hipStream_t)(uintptr_t)0x100;
    if (!c.formats.empty()) {
        const int rc = sat_dit_plan_set_block_formats(p, c.formats.data(), (int32_t)c.formats.size());
        line("rc sat_dit_plan_set_block_formats", rc);
        if (rc) return sat_dit_plan_destroy(p);
    }
    {
        Inputs weights;
        set_tensors3(p, c, weights);
        RC(sat_dit_plan_finalize, p, s);
    }
    if (c.after_finalize) RC(sat_dit_plan_set_block_formats, p, c.formats.data(), (int32_t)c.formats.size());
    {
        const int bf = 2, lc = 5;
        Inputs in;
        RC(sat_dit_prepare_context, p, in.make("cond", (size_t)bf * lc * DCT), bf, lc, in.make("global_cond", (size_t)bf * DG), s);
        size_t bytes = 0;
        RC(sat_dit_workspace_bytes, p, bf, T, &bytes);
        line("workspace_bytes", bytes);
        void* ws = in.workspace(bytes);
        RC(sat_dit_forward, p, in.make("x", (size_t)bf * C * T), in.make("t", bf), in.make("out", (size_t)bf * C * T), bf, T, ws, bytes, s);
    }
    sat_dit_plan_destroy(p);
}

}  // namespace

int main() {
    const std::vector<FormatCase> all = {
        {"plain_fp16_fold", F16, 1, {}},
        {"uniform_fp16_fold", F16, 1, {F16, F16, F16}},
        {"plain_bf16_fold", BF16, 1, {}},
        {"uniform_bf16_fold", BF16, 1, {BF16, BF16, BF16}},
        {"all_bf16_on_fp16_plan_fold", F16, 1, {BF16, BF16, BF16}},
        {"mixed_fold", F16, 1, {F16, BF16, F16}},
        {"mixed_tail_fold", BF16, 1, {BF16, F16, F16}},
        {"plain_fp16", F16, 0, {}},
        {"mixed", F16, 0, {F16, BF16, F16}},
        {"plain_fp16_adaln", F16, 1, {}, 1},
        {"mixed_adaln", F16, 1, {F16, BF16, F16}, 1},
        {"after_finalize", F16, 1, {F16, BF16, F16}, 0, 0, true},
        {"wrong_n", F16, 1, {F16, BF16}},
        {"bad_value", F16, 1, {F16, SAT_GEMM_FP8, F16}},
        {"refused_fp8", SAT_GEMM_FP8, 0, {F16, BF16, F16}},
        {"refused_fp8_all", SAT_GEMM_FP8, 0, {F16, BF16, F16}, 0, SAT_FP8_ALL},
        {"refused_fp32x", SAT_GEMM_FP32X, 0, {F16, BF16, F16}},
    };
    for (const FormatCase& c : all) {
        g_allocs = 0;
        line("==", c.name);
        run3(c);
    }
    return 0;
}
