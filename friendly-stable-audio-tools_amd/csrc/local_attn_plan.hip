// The local-attention transformer codec on the device: TransformerEncoder1D / TransformerDecoder1D of the reference's models/local_attention.py
// (:193-282), the codec that create_encoder_from_config / create_decoder_from_config select with "type": "local_attn" (models/autoencoders.py:
// 709-712, 735-738).  One plan per encoder or decoder, composed from the launchers of sat_common.h as the T5 and RoBERTa plans are; the only
// kernels of its own are the two projections at the audio boundary (local_attn_io.hip) and the weight permutation below.
//
//   encoder  x [b, c_in, t] --project_in--> rows [b t, D_0];  per stage: [project_in D_{i-1} -> D_i] -> depth_i layers at S rows per item ->
//            "b (n r) c -> b n (c r)" + project_down;  rows --project_out--> [b, c_out, t / prod(ratios)]
//   decoder  z [b, c_in, t] --project_in--> rows [b t, D_0];  per stage: [project_in] -> project_up + "b n (c r) -> b (n r) c" -> depth_i layers;
//            rows --project_out--> [b, c_out, t * prod(ratios)]
//   layer    (ContinuousLocalTransformer, :51-101, without conditioning, cross-attention or causal masking)
//            x += to_out(natten(rope(to_qkv(LayerNorm(x)))));  x += ff.2(swiglu(ff.0.proj(LayerNorm(x))))
//
// The two rearranges move no data.  r consecutive rows of [M, C] ARE one row of [M / r, r C] with feature index j C + c, so project_down runs as
// one GEMM of contraction length r C on the weight with its columns permuted at finalize (W'[:, j C + c] = W[:, c r + j]); project_up is the
// mirror image, its rows permuted, its [M, r C] output read as [M r, C].  Linears that follow each other (the codec's project_in and a stage's,
// project_down and the next stage's project_in, project_in and project_up) run as written, none is folded.
//
// Launches per layer, 16-bit operands (fp16 / bf16; the residual stream is fp32): LayerNorm -> to_qkv -> [head split] -> window attention ->
// to_out (+= into the stream) -> LayerNorm -> FF-in (SwiGLU epilogue) -> FF-out (+= into the stream): 7 at 64-channel heads, where to_qkv's
// heads epilogue splits, rotates and pre-scales (q carries log2(e) only: the reference does not scale the logits of its NATTEN branch); 8 at
// 32, 96 and 128, where to_qkv writes fp32 and head_split_hdw.hip follows.  fp32 operands: the same on f32_ref.hip, 9 launches (the head split
// and the SwiGLU are launches of their own at every width; no 128-channel heads there).  Per stage: one rotation table, one clear of the q / k /
// v pads, and per Linear outside the layers a cast of its fp32 input and the fp32-output GEMM (fp32 operands: the GEMM alone).
#include <algorithm>
#include <string>
#include <vector>

#include "sat_common.h"
#include "plan_core.h"

namespace {

// out[o][j * c + ci][i] = in[o][ci * r + j][i]: the columns of project_down.weight (outer = rows, inner = 1), the rows of project_up.weight
// (outer = 1, inner = the row length)
__global__ __launch_bounds__(256) void local_attn_permute_kernel(const float* __restrict__ in, float* __restrict__ out, int64_t outer, int c, int r,
                                                                 int inner) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t units = (int64_t)c * r;
    if (idx >= outer * units * inner) return;
    const int i = (int)(idx % inner);
    const int64_t u = (idx / inner) % units, o = idx / (inner * units);
    const int j = (int)(u / c), ci = (int)(u - (int64_t)j * c);
    out[idx] = in[(o * units + (int64_t)ci * r + j) * inner + i];
}

int launch_permute(const float* in, float* out, int64_t outer, int c, int r, int inner, hipStream_t s) {
    const int64_t total = outer * c * r * inner;
    hipLaunchKernelGGL(local_attn_permute_kernel, dim3((unsigned)cdiv(total, 256)), dim3(256), 0, s, in, out, outer, c, r, inner);
    SAT_LAUNCH_CHECK();
    return 0;
}

struct Lin {      // y [M, n] = x [M, k] W^T; w: [n, k] in the plan's operand format (fp32 in the fp32 build); n == 0: the identity
    op_t* w = nullptr;
    float* bias = nullptr;
    int n = 0, k = 0;
};
struct LaLayer {
    float *g1, *b1, *g2, *b2;
    Lin qkv, o, ff1, ff2;
};
struct LaStage {
    int D, H, hd, inner, depth, r, prev;
    Lin pin, resample;      // project_in (identity where prev == D); project_down / project_up with the rearrange in the weight
    float* inv_freq;
    std::vector<LaLayer> layers;
};

}  // namespace

struct sat_local_attn_plan {
    sat_local_attn_cfg cfg;
    TensorTable tensors;
    bool finalized = false;
    DevBuf arena;
    bool f32 = false;
    int f16 = 0;
    int64_t ratio = 1;
    float *w_in = nullptr, *w_out = nullptr;      // fp32 in every build (local_attn_io.hip)
    std::vector<LaStage> stages;
};

extern "C" int sat_local_attn_plan_create(const sat_local_attn_cfg* cfg, size_t cfg_bytes, sat_local_attn_plan** out_plan) {
    SAT_CHECK_ARG(cfg && out_plan, SAT_E_INVALID, "local_attn_plan_create: null argument");
    SAT_CHECK_ARG(cfg_bytes == sizeof(sat_local_attn_cfg), SAT_E_INVALID, "local_attn_plan_create: sat_local_attn_cfg of %zu bytes, this library reads %zu",
                  cfg_bytes, sizeof(sat_local_attn_cfg));
    const sat_local_attn_cfg& c = *cfg;
    SAT_CHECK_ARG((c.is_decoder == 0 || c.is_decoder == 1) && c.in_channels > 0 && c.out_channels > 0, SAT_E_INVALID, "local_attn_plan_create: bad channels");
    SAT_CHECK_ARG(c.n_stages >= 1 && c.n_stages <= SAT_LOCAL_ATTN_MAX_STAGES, SAT_E_INVALID, "local_attn_plan_create: %d stages (1..%d)", c.n_stages,
                  SAT_LOCAL_ATTN_MAX_STAGES);
    SAT_CHECK_ARG(c.gemm_dtype == SAT_GEMM_BF16 || c.gemm_dtype == SAT_GEMM_FP16 || c.gemm_dtype == SAT_GEMM_FP32X, SAT_E_UNSUPPORTED,
                  "local_attn_plan_create: gemm_dtype %d (bf16, fp16 or the fp32 build)", c.gemm_dtype);
    SAT_CHECK_ARG(c.in_channels <= 128, SAT_E_UNSUPPORTED, "local_attn_plan_create: in_channels %d: the boundary kernel takes at most 128", c.in_channels);
    // NATTEN's rule
    SAT_CHECK_ARG(c.window > 1 && (c.window & 1), SAT_E_INVALID, "local_attn_plan_create: local_attn_window_size %d must be odd and greater than 1", c.window);
    int64_t ratio = 1;
    for (int i = 0; i < c.n_stages; ++i) {
        const int D = c.embed_dims[i], H = c.heads[i], inner = c.ff_inner[i];
        SAT_CHECK_ARG(D > 0 && H > 0 && c.depths[i] >= 0 && c.ratios[i] >= 1 && inner > 0, SAT_E_INVALID, "local_attn_plan_create: stage %d: bad sizes", i);
        const int hd = D / H;
        SAT_CHECK_ARG(hd == 32 || hd == 64 || hd == 96 || hd == 128, SAT_E_UNSUPPORTED,
                      "local_attn_plan_create: stage %d: dim_heads %d = embed_dim %d // heads %d (the attention kernels are built for 32, 64, 96 and 128)", i, hd, D, H);
        SAT_CHECK_ARG(H * hd == D, SAT_E_UNSUPPORTED, "local_attn_plan_create: stage %d: embed_dim %d is no multiple of heads %d", i, D, H);
        SAT_CHECK_ARG(hd != 128 || c.gemm_dtype != SAT_GEMM_FP32X, SAT_E_UNSUPPORTED,
                      "local_attn_plan_create: stage %d: dim_heads 128 runs with bf16 or fp16 operands only (no fp32 kernels at that width)", i);
        // the GEMM launchers: N %% 128 (to_qkv 3 D, to_out / FF-out / project_* D, FF-in 2 inner), K %% 64 (D, inner)
        SAT_CHECK_ARG(D % 128 == 0 && D <= 4096, SAT_E_UNSUPPORTED, "local_attn_plan_create: stage %d: embed_dim %d must be a multiple of 128 and <= 4096", i, D);
        SAT_CHECK_ARG(inner % 64 == 0, SAT_E_UNSUPPORTED, "local_attn_plan_create: stage %d: int(embed_dim * ff_mult) = %d must be a multiple of 64", i, inner);
        SAT_CHECK_ARG((int64_t)D * c.ratios[i] <= (1 << 20), SAT_E_UNSUPPORTED, "local_attn_plan_create: stage %d: embed_dim %d x ratio %d", i, D, c.ratios[i]);
        ratio *= c.ratios[i];
        SAT_CHECK_ARG(ratio <= (1 << 24), SAT_E_UNSUPPORTED, "local_attn_plan_create: the product of the ratios exceeds 2^24");
    }
    SAT_CHECK_ARG(sat_launch_head_split_hdw && sat_launch_rope_table_hdw && sat_launch_attention_window && sat_launch_attention_hdw_window &&
                      sat_launch_split_heads_f32_w && sat_launch_attention_f32_window && sat_launch_attention_f32_window_w,
                  SAT_E_UNSUPPORTED, "local_attn_plan_create: built without the neighbourhood attention kernels");
    sat_local_attn_plan* p = new (std::nothrow) sat_local_attn_plan();
    SAT_CHECK_ARG(p, SAT_E_INVALID, "local_attn_plan_create: out of host memory");
    p->cfg = c;
    p->f32 = c.gemm_dtype == SAT_GEMM_FP32X;
    p->f16 = c.gemm_dtype == SAT_GEMM_FP16;
    p->ratio = ratio;
    *out_plan = p;
    return 0;
}

extern "C" void sat_local_attn_plan_destroy(sat_local_attn_plan* p) { delete p; }

extern "C" int sat_local_attn_plan_set_tensor(sat_local_attn_plan* p, const char* name, const float* data_dev, int64_t numel) {
    SAT_CHECK_ARG(p, SAT_E_INVALID, "local_attn_plan_set_tensor: bad argument");
    return p->tensors.set("local_attn", name, data_dev, numel);
}

namespace {

// two passes over the same code (plan_finalize): sizes first (ar.dry()), then copies and re-packs
int la_build(sat_local_attn_plan* p, Bump& ar, hipStream_t s) {
    const sat_local_attn_cfg& c = p->cfg;
    const bool dec = c.is_decoder != 0;
    auto place = [&](const std::string& name, int64_t numel, float** dst) -> int { return p->tensors.place("local_attn", ar, name, numel, dst, s); };
    // the tensor `name` [n, k] (and `bias_name` [n]) in the plan's operand format; interleave: the SwiGLU row order of the FF-in epilogue
    // (16-bit operands; the fp32 build keeps the reference's order for sat_launch_swiglu_f32)
    auto linear = [&](const std::string& name, const char* bias_name, int n, int k, int interleave, Lin* out) -> int {
        const float *src = nullptr, *bias = nullptr;
        if (!ar.dry()) {
            SAT_TRY(p->tensors.get("local_attn", name, (int64_t)n * k, &src));
            if (bias_name) SAT_TRY(p->tensors.get("local_attn", bias_name, n, &bias));
        }
        out->n = n; out->k = k;
        out->w = (op_t*)ar.take((size_t)n * k * (p->f32 ? 4 : 2));
        out->bias = bias_name ? (float*)ar.take((size_t)n * 4) : nullptr;
        if (ar.dry()) return 0;
        if (p->f32) SAT_HIP(hipMemcpyAsync(out->w, src, (size_t)n * k * 4, hipMemcpyDeviceToDevice, s));
        else SAT_TRY(sat_launch_pack_rows_bf16(src, out->w, n, k, interleave, s, p->f16));
        if (!bias_name) return 0;
        if (interleave && !p->f32) return sat_launch_pack_bias(bias, out->bias, n, interleave, s);
        SAT_HIP(hipMemcpyAsync(out->bias, bias, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
        return 0;
    };
    SAT_TRY(place("project_in.weight", (int64_t)c.embed_dims[0] * c.in_channels, &p->w_in));
    SAT_TRY(place("project_out.weight", (int64_t)c.out_channels * c.embed_dims[c.n_stages - 1], &p->w_out));
    // the permuted fp32 image of one project_down / project_up weight at a time, in front of its re-pack (stream order keeps the stages apart)
    size_t perm_el = 0;
    for (int i = 0; i < c.n_stages; ++i) perm_el = std::max(perm_el, (size_t)c.embed_dims[i] * c.embed_dims[i] * c.ratios[i]);
    float* perm = (float*)ar.take(perm_el * 4);
    p->stages.resize(c.n_stages);
    for (int i = 0; i < c.n_stages; ++i) {
        LaStage& st = p->stages[i];
        st.D = c.embed_dims[i]; st.H = c.heads[i]; st.hd = st.D / st.H; st.inner = c.ff_inner[i]; st.depth = c.depths[i]; st.r = c.ratios[i];
        st.prev = i ? c.embed_dims[i - 1] : c.embed_dims[0];
        const int D = st.D, r = st.r;
        const std::string sp = "layers." + std::to_string(i) + ".";
        st.pin = Lin{};
        if (st.prev != D) SAT_TRY(linear(sp + "project_in.weight", nullptr, D, st.prev, 0, &st.pin));
        {
            const std::string name = sp + (dec ? "project_up.weight" : "project_down.weight");
            const int n = dec ? r * D : D, k = dec ? D : r * D;
            Lin& L = st.resample;
            L = Lin{};
            L.n = n; L.k = k;
            L.w = (op_t*)ar.take((size_t)n * k * (p->f32 ? 4 : 2));
            if (!ar.dry()) {
                const float* src;
                SAT_TRY(p->tensors.get("local_attn", name, (int64_t)n * k, &src));
                float* dst32 = p->f32 ? (float*)L.w : perm;
                SAT_TRY(dec ? launch_permute(src, dst32, 1, D, r, D, s) : launch_permute(src, dst32, D, D, r, 1, s));
                if (!p->f32) SAT_TRY(sat_launch_pack_rows_bf16(perm, L.w, n, k, 0, s, p->f16));
            }
        }
        SAT_TRY(place(sp + "transformer.rotary_pos_emb.inv_freq", sat_rope_pairs(st.hd), &st.inv_freq));
        st.layers.resize(st.depth);
        for (int l = 0; l < st.depth; ++l) {
            LaLayer& L = st.layers[l];
            const std::string lp = sp + "transformer.layers." + std::to_string(l) + ".";
            SAT_TRY(place(lp + "0.gamma", D, &L.g1));
            SAT_TRY(place(lp + "0.beta", D, &L.b1));
            SAT_TRY(linear(lp + "1.to_qkv.weight", nullptr, 3 * D, D, 0, &L.qkv));
            SAT_TRY(linear(lp + "1.to_out.weight", nullptr, D, D, 0, &L.o));
            SAT_TRY(place(lp + "3.gamma", D, &L.g2));
            SAT_TRY(place(lp + "3.beta", D, &L.b2));
            // GLU keeps the bias of its own nn.Linear (transformer.py:222); no_bias drops the one of ff.2 alone
            const std::string b1 = lp + "4.ff.0.proj.bias";
            SAT_TRY(linear(lp + "4.ff.0.proj.weight", b1.c_str(), 2 * st.inner, D, 1, &L.ff1));
            SAT_TRY(linear(lp + "4.ff.2.weight", nullptr, D, st.inner, 0, &L.ff2));
        }
    }
    return 0;
}

// The rows per batch item at which stage i's layers run, for an input of t time steps; 0 and a message where the plan refuses the length
int la_stage_rows(const sat_local_attn_plan* p, int t, int* rows) {
    const sat_local_attn_cfg& c = p->cfg;
    SAT_CHECK_ARG(c.is_decoder || t % p->ratio == 0, SAT_E_INVALID, "local_attn: an input of %d samples is no multiple of the product of the ratios, %lld", t,
                  (long long)p->ratio);
    SAT_CHECK_ARG(!c.is_decoder || (int64_t)t * p->ratio <= INT32_MAX, SAT_E_UNSUPPORTED, "local_attn: %d latents x %lld exceed 2^31 samples", t, (long long)p->ratio);
    int64_t S = t;
    for (int i = 0; i < c.n_stages; ++i) {
        if (c.is_decoder) S *= c.ratios[i];
        rows[i] = (int)S;
        SAT_CHECK_ARG(S >= c.window, SAT_E_INVALID, "local_attn: stage %d runs at %lld rows per item, fewer than local_attn_window_size %d", i, (long long)S,
                      c.window);
        if (!c.is_decoder) S /= c.ratios[i];
    }
    return 0;
}

struct LaWs {
    float *X0, *X1;
    op_t *A, *AO, *Q, *K, *Vt, *Hh;
    float *wide, *rc, *rs;      // wide: fp32 [M, 3 D] in front of a head split ([M, max(3 D, 2 inner)] in the fp32 build)
    size_t qkv_bytes;           // of each of Q, K, Vt, a multiple of 256: one clear covers the three
    size_t total;
};

int la_carve(const sat_local_attn_plan* p, int b, int t, char* base, LaWs* out) {
    const sat_local_attn_cfg& c = p->cfg;
    int rows[SAT_LOCAL_ATTN_MAX_STAGES];
    SAT_TRY(la_stage_rows(p, t, rows));
    const bool dec = c.is_decoder != 0, f32 = p->f32;
    const size_t el = f32 ? 4 : 2;
    size_t x_el = (size_t)b * t * c.embed_dims[0], a_el = 0, h_el = 0, qkv = 0, wide_el = 0, rope_el = 0;
    int64_t widest = 0;
    size_t M = (size_t)b * t;
    for (int i = 0; i < c.n_stages; ++i) {
        const size_t D = c.embed_dims[i], H = c.heads[i], hd = D / H, inner = c.ff_inner[i], prev = i ? c.embed_dims[i - 1] : c.embed_dims[0];
        if (prev != D) {      // project_in at the rows the stage receives
            a_el = std::max(a_el, M * prev);
            x_el = std::max(x_el, M * D);
        }
        if (dec) a_el = std::max(a_el, M * D);      // project_up's input
        M = (size_t)b * rows[i];
        x_el = std::max(x_el, M * D);
        a_el = std::max(a_el, M * D);               // the LayerNorm's output; project_down's input
        h_el = std::max(h_el, M * inner);
        const size_t Spad = (size_t)round_up(rows[i] + 3, 128);
        qkv = std::max(qkv, f32 ? M * D * 4 : (size_t)b * H * Spad * hd * 2);
        if (f32) wide_el = std::max(wide_el, M * std::max(3 * D, 2 * inner));
        else if (hd != 64) wide_el = std::max(wide_el, M * 3 * D);
        rope_el = std::max(rope_el, (size_t)rows[i] * sat_rope_pairs((int)hd));
        widest = std::max<int64_t>(widest, (int64_t)M * (int64_t)std::max(std::max(3 * D, 2 * inner), D * c.ratios[i]));
        if (!dec) M = (size_t)b * (rows[i] / c.ratios[i]);
    }
    SAT_CHECK_ARG(widest < (1ll << 31), SAT_E_UNSUPPORTED, "local_attn: %d items of %d time steps: a GEMM output of %lld elements exceeds 2^31 (use chunked=True)", b, t,
                  (long long)widest);
    Bump ws{base};
    LaWs w;
    w.X0 = (float*)ws.take(x_el * 4);
    w.X1 = (float*)ws.take(x_el * 4);
    w.A = (op_t*)ws.take(a_el * el);
    w.AO = (op_t*)ws.take(a_el * el);
    w.qkv_bytes = (size_t)round_up((int64_t)qkv, 256);
    w.Q = (op_t*)ws.take(w.qkv_bytes);
    w.K = (op_t*)ws.take(w.qkv_bytes);
    w.Vt = (op_t*)ws.take(w.qkv_bytes);
    w.Hh = (op_t*)ws.take(h_el * el);
    w.wide = wide_el ? (float*)ws.take(wide_el * 4) : nullptr;
    w.rc = (float*)ws.take(rope_el * 4);
    w.rs = (float*)ws.take(rope_el * 4);
    w.total = ws.off;
    *out = w;
    return 0;
}

struct LaRun {
    const sat_local_attn_plan* p;
    LaWs w;
    hipStream_t s;
    int b;

    GemmArgs gemm(const Lin& L, const op_t* A, int M) const {
        GemmArgs g{};
        g.f16 = p->f16;
        g.A = A; g.W = L.w; g.bias = L.bias; g.M = M; g.N = L.n; g.K = L.k;
        return g;
    }
    // y [M, L.n] = x [M, L.k] W^T, both fp32: the Linears outside the layers
    int linear(const Lin& L, const float* x, float* y, int M) const {
        if (p->f32) return sat_launch_gemm_f32(x, (const float*)L.w, nullptr, y, M, L.n, L.k, L.n, 0, nullptr, 1, 0, s);
        SAT_TRY(sat_launch_cast_bf16(x, w.A, (int64_t)M * L.k, s, p->f16));
        GemmArgs g = gemm(L, w.A, M);
        g.C = y; g.ldc = L.n;
        return sat_launch_gemm(EPI_F32, g, s);
    }
    // X [M, L.n] += A [M, L.k] W^T
    int resid(const Lin& L, const op_t* A, float* X, int M) const {
        GemmArgs g = gemm(L, A, M);
        g.C = X; g.ldc = L.n; g.accumulate = 1;
        return sat_launch_gemm(EPI_RESID, g, s);
    }
    // the rotation table and the zero pads of q / k / v for a stage whose layers run at S rows per item
    int begin_stage(const LaStage& st, int S) const {
        if (st.hd == 64) SAT_TRY(sat_launch_rope_table(st.inv_freq, w.rc, w.rs, S, s));
        else SAT_TRY(sat_launch_rope_table_hdw(st.inv_freq, w.rc, w.rs, S, st.hd, s));
        if (!p->f32) SAT_HIP(hipMemsetAsync(w.Q, 0, 3 * w.qkv_bytes, s));      // the pads must be finite: the head split writes the S valid rows only
        return 0;
    }
    int layer(const LaStage& st, const LaLayer& L, float* X, int S) const;
    int layer_f32(const LaStage& st, const LaLayer& L, float* X, int S) const;
};

int LaRun::layer(const LaStage& st, const LaLayer& L, float* X, int S) const {
    if (p->f32) return layer_f32(st, L, X, S);
    const int M = b * S, D = st.D, H = st.H, ks = p->cfg.window, f16 = p->f16;
    const int Spad = (int)round_up(S + 3, 128);
    SAT_TRY(sat_launch_layernorm(X, L.g1, L.b1, w.A, M, D, s, f16));
    HeadsEpi he{};
    he.out[0] = w.Q; he.out[1] = w.K; he.out[2] = w.Vt;
    he.kind[0] = 2 | 8; he.kind[1] = 2 | 4; he.kind[2] = 1 | 4;
    he.qscale = 1.4426950408889634f;      // log2(e) alone: the logits of the NATTEN branch are not scaled (transformer.py:486)
    he.parts = 3; he.heads = H; he.S = S; he.Spad = Spad;
    he.rope_cos = w.rc; he.rope_sin = w.rs;
    GemmArgs g = gemm(L.qkv, w.A, M);
    if (st.hd == 64) {
        g.heads = he;
        SAT_TRY(sat_launch_gemm(EPI_HEADS, g, s));
        SAT_TRY(sat_launch_attention_window(w.Q, w.K, w.Vt, w.AO, b, H, H, S, Spad, Spad, ks, 1.0f, s, f16));
    } else {
        g.C = w.wide; g.ldc = g.N;
        SAT_TRY(sat_launch_gemm(EPI_F32, g, s));
        SAT_TRY(sat_launch_head_split_hdw(w.wide, he, st.hd, b, s, f16));
        SAT_TRY(sat_launch_attention_hdw_window(w.Q, w.K, w.Vt, w.AO, b, H, H, st.hd, S, Spad, Spad, ks, s, f16));
    }
    SAT_TRY(resid(L.o, w.AO, X, M));
    SAT_TRY(sat_launch_layernorm(X, L.g2, L.b2, w.A, M, D, s, f16));
    g = gemm(L.ff1, w.A, M);
    g.H = w.Hh;
    SAT_TRY(sat_launch_gemm(EPI_SWIGLU, g, s));
    return resid(L.ff2, w.Hh, X, M);
}

int LaRun::layer_f32(const LaStage& st, const LaLayer& L, float* X, int S) const {
    const int M = b * S, D = st.D, H = st.H, inner = st.inner, ks = p->cfg.window;
    float *A = (float*)w.A, *AO = (float*)w.AO, *Q = (float*)w.Q, *K = (float*)w.K, *V = (float*)w.Vt, *Hh = (float*)w.Hh;
    auto W = [](const Lin& r) { return (const float*)r.w; };
    SAT_TRY(sat_launch_layernorm_f32(X, L.g1, L.b1, A, M, D, nullptr, nullptr, 1, 0, s));
    SAT_TRY(sat_launch_gemm_f32(A, W(L.qkv), nullptr, w.wide, M, 3 * D, D, 3 * D, 0, nullptr, 1, 0, s));
    SAT_TRY(sat_launch_split_heads_f32_w(w.wide, Q, K, V, M, S, 3, H, st.hd, 3, w.rc, w.rs, s, 0));
    if (st.hd == 64) SAT_TRY(sat_launch_attention_f32_window(Q, K, V, AO, b, H, H, S, ks, 1.0f, s));
    else SAT_TRY(sat_launch_attention_f32_window_w(Q, K, V, AO, b, H, H, st.hd, S, ks, 1.0f, s));
    SAT_TRY(sat_launch_gemm_f32(AO, W(L.o), nullptr, X, M, D, D, D, 1, nullptr, 1, 0, s));
    SAT_TRY(sat_launch_layernorm_f32(X, L.g2, L.b2, A, M, D, nullptr, nullptr, 1, 0, s));
    SAT_TRY(sat_launch_gemm_f32(A, W(L.ff1), L.ff1.bias, w.wide, M, 2 * inner, D, 2 * inner, 0, nullptr, 1, 0, s));
    SAT_TRY(sat_launch_swiglu_f32(w.wide, Hh, M, inner, s));
    return sat_launch_gemm_f32(Hh, W(L.ff2), nullptr, X, M, D, inner, D, 1, nullptr, 1, 0, s);
}

}  // namespace

extern "C" int sat_local_attn_plan_finalize(sat_local_attn_plan* p, sat_stream_t stream) {
    SAT_CHECK_ARG(p, SAT_E_INVALID, "local_attn_plan_finalize: null plan");
    hipStream_t s = (hipStream_t)stream;
    return plan_finalize(p, s, [&](Bump& ar) { return la_build(p, ar, s); });
}

extern "C" int sat_local_attn_workspace_bytes(const sat_local_attn_plan* p, int32_t b, int32_t t, size_t* out_bytes) {
    SAT_CHECK_ARG(p && out_bytes && b > 0 && t > 0, SAT_E_INVALID, "local_attn_workspace_bytes: bad arguments");
    LaWs w;
    SAT_TRY(la_carve(p, b, t, nullptr, &w));
    *out_bytes = w.total;
    return 0;
}

extern "C" int sat_local_attn_forward(sat_local_attn_plan* p, const float* x_dev, float* out_dev, int32_t b, int32_t t, void* ws, size_t ws_bytes,
                                      sat_stream_t stream) {
    SAT_CHECK_ARG(p && p->finalized, SAT_E_STATE, "local_attn_forward: plan not finalized");
    SAT_CHECK_ARG(x_dev && out_dev && ws && b > 0 && t > 0, SAT_E_INVALID, "local_attn_forward: bad arguments");
    SAT_CHECK_ARG(((uintptr_t)ws & 255) == 0, SAT_E_INVALID, "local_attn_forward: workspace must be 256-byte aligned");
    const sat_local_attn_cfg& c = p->cfg;
    // the length and the window are checked before anything is launched (la_stage_rows, inside the carve)
    LaRun run{p, {}, (hipStream_t)stream, b};
    SAT_TRY(la_carve(p, b, t, (char*)ws, &run.w));
    SAT_CHECK_ARG(ws_bytes >= run.w.total, SAT_E_WORKSPACE, "local_attn_forward: workspace %zu < required %zu", ws_bytes, run.w.total);
    int rows[SAT_LOCAL_ATTN_MAX_STAGES];
    SAT_TRY(la_stage_rows(p, t, rows));
    const bool dec = c.is_decoder != 0;
    hipStream_t s = run.s;
    float *cur = run.w.X0, *other = run.w.X1;
    SAT_TRY(sat_launch_local_attn_project_in(x_dev, p->w_in, cur, b, c.in_channels, t, c.embed_dims[0], s));
    int S = t;
    for (int i = 0; i < c.n_stages; ++i) {
        const LaStage& st = p->stages[i];
        if (st.pin.n) {
            SAT_TRY(run.linear(st.pin, cur, other, b * S));
            std::swap(cur, other);
        }
        if (dec) {      // project_up: [b S, D] -> [b S, r D], read as [b S r, D]
            SAT_TRY(run.linear(st.resample, cur, other, b * S));
            std::swap(cur, other);
        }
        S = rows[i];
        if (st.depth) SAT_TRY(run.begin_stage(st, S));
        for (int l = 0; l < st.depth; ++l) SAT_TRY(run.layer(st, st.layers[l], cur, S));
        if (!dec) {     // project_down: [b S, D] read as [b S / r, r D] -> [b S / r, D]
            S /= st.r;
            SAT_TRY(run.linear(st.resample, cur, other, b * S));
            std::swap(cur, other);
        }
    }
    return sat_launch_local_attn_project_out(cur, p->w_out, out_dev, b, c.out_channels, S, c.embed_dims[c.n_stages - 1], s);
}
