// RoBERTa encoder stack on the device: the text branch of CLAP, the "clap_text" conditioner of Stable Audio 2.0.
// Replaces the `text_branch(input_ids, attention_mask, output_hidden_states=True)["hidden_states"][feature_layer_ix]` call inside
// the reference's CLAPTextConditioner.get_clap_features (models/conditioners.py:162-171) and the proj_out that follows (:182).
// The algorithm is that of transformers' modeling_roberta.py (a third-party dependency of laion_clap, not vendored in the reference);
// BERT with post-LayerNorm:
//   RobertaEmbeddings = LayerNorm(word_embeddings[id] + position_embeddings[pos] + token_type_embeddings[0])
//                       pos = create_position_ids_from_input_ids: pad_id + cumsum(id != pad_id) at non-pad tokens, pad_id at pad tokens
//                       (from the INPUT IDS, not from the attention mask)
//   RobertaLayer      = h = LayerNorm(h + dense(SelfAttention(h)) + b)           (RobertaSelfOutput)
//                       h = LayerNorm(h + W2 gelu(W1 h + b1) + b2)               (RobertaIntermediate / RobertaOutput; exact erf GELU)
//   SelfAttention     = softmax(q k^T / sqrt(d_head) + mask) v, q / k / v = Linear with bias; mask = finfo(float32).min at keys with
//                       attention_mask == 0; padded QUERY rows are computed like any other row
//   LayerNorm         = (x - mean) * rsqrt(var + eps) * weight + bias
//   hidden_states[j]  = the stream after j layers (j = 0: the embeddings): a plan runs cfg.run_layers of them and stops; the pooler
//                       is never evaluated
// Runs once per generation on B x 77 tokens, so, like the T5 stack, everything is fp32 on the exact fp32 MFMA GEMM of f32_ref.hip:
// the reference runs the encoder under fp16 autocast; fp32 is the more accurate of the two and needs no second set of kernels.
#include <math.h>

#include <string>
#include <vector>

#include "enc_attention.h"
#include "sat_common.h"
#include "plan_core.h"

namespace {

// Gather, per-sequence position scan and LayerNorm in one launch: one wave per token row.  The position of token i is the number
// of non-pad ids in ids[b][0 .. i] (a ballot / popcount scan over at most L ids) + pad_id.  The caller guarantees pad_id + L <
// max_positions; ids outside [0, vocab) are clamped (the tokenizer never produces them).
__global__ __launch_bounds__(256) void roberta_embed_ln_kernel(const int* __restrict__ ids, const float* __restrict__ word,
                                                               const float* __restrict__ posw, const float* __restrict__ type0,
                                                               const float* __restrict__ gamma, const float* __restrict__ beta,
                                                               float* __restrict__ y, int M, int L, int D, int vocab, int pad_id, float eps) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= M) return;
    const int b = row / L, i = row - b * L;
    const int* seq = ids + (size_t)b * L;
    int count = 0;
    for (int j0 = 0; j0 <= i; j0 += 64) {
        const int j = j0 + lane;
        count += __popcll(__ballot(j <= i && seq[j <= i ? j : i] != pad_id));
    }
    int id = seq[i];
    const int pos = id != pad_id ? pad_id + count : pad_id;
    id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
    const float* wr = word + (size_t)id * D;
    const float* pr = posw + (size_t)pos * D;
    float* yr = y + (size_t)row * D;
    float s = 0.f;
    for (int c = lane; c < D; c += 64) {
        const float v = (wr[c] + type0[c]) + pr[c];          // the order of RobertaEmbeddings.forward
        yr[c] = v;                                           // staged in the output row: each lane re-reads only what it wrote
        s += v;
    }
    const float mean = wave_sum(s) / (float)D;
    float q = 0.f;
    for (int c = lane; c < D; c += 64) {
        const float a = yr[c] - mean;
        q += a * a;
    }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)D + eps);
    for (int c = lane; c < D; c += 64) yr[c] = (yr[c] - mean) * rstd * gamma[c] + beta[c];
}

// exact GELU (ACT2FN["gelu"] = x * 0.5 * (1 + erf(x / sqrt(2)))) in place
__global__ __launch_bounds__(256) void roberta_gelu_kernel(float* __restrict__ h, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float x = h[i];
    h[i] = 0.5f * x * (1.0f + erff(x * 0.7071067811865476f));
}

// ---- the launches: sat_roberta_encode and the unit entries at the end of this file share them
int roberta_launch_embed_ln(const int* ids, const float* word, const float* posw, const float* type0, const float* gamma, const float* beta,
                            float* y, int B, int L, int D, int vocab, int pad_id, int max_positions, float eps, hipStream_t s) {
    SAT_CHECK_ARG(ids && word && posw && type0 && gamma && beta && y && B > 0 && L > 0 && D > 0 && vocab > 0 && pad_id >= 0 && pad_id < vocab,
                  SAT_E_INVALID, "roberta_embed_ln: bad arguments");
    // the last token of a pad-free sequence sits at pad_id + L
    SAT_CHECK_ARG(pad_id + L < max_positions, SAT_E_UNSUPPORTED, "roberta_embed_ln: sequence length %d needs position %d of a table of %d", L,
                  pad_id + L, max_positions);
    const int M = B * L;
    hipLaunchKernelGGL(roberta_embed_ln_kernel, dim3(cdiv(M, 4)), dim3(256), 0, s, ids, word, posw, type0, gamma, beta, y, M, L, D, vocab, pad_id,
                       eps);
    SAT_LAUNCH_CHECK();
    return 0;
}

int roberta_launch_gelu(float* h, int64_t n, hipStream_t s) {
    SAT_CHECK_ARG(h && n > 0, SAT_E_INVALID, "roberta_gelu: bad arguments");
    hipLaunchKernelGGL(roberta_gelu_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, s, h, n);
    SAT_LAUNCH_CHECK();
    return 0;
}

struct RobertaLayer {
    float *wqkv, *bqkv, *wo, *bo, *ln1g, *ln1b, *w1, *b1, *w2, *b2, *ln2g, *ln2b;
};

}  // namespace

struct sat_roberta_plan {
    sat_roberta_cfg cfg;
    TensorTable tensors;
    bool finalized = false;
    DevBuf arena;
    float *word = nullptr, *posw = nullptr, *type0 = nullptr, *emb_g = nullptr, *emb_b = nullptr;
    float *proj_w = nullptr, *proj_b = nullptr;       // Conditioner.proj_out (conditioners.py:23) when cfg.proj_dim > 0
    std::vector<RobertaLayer> layers;                 // cfg.run_layers of them
};

extern "C" int sat_roberta_plan_create(const sat_roberta_cfg* cfg, sat_roberta_plan** out_plan) {
    SAT_CHECK_ARG(cfg && out_plan, SAT_E_INVALID, "roberta_plan_create: null argument");
    SAT_CHECK_ARG(cfg->vocab_size > 0 && cfg->hidden_size > 0 && cfg->num_layers > 0 && cfg->num_heads > 0 && cfg->intermediate_size > 0,
                  SAT_E_INVALID, "roberta_plan_create: bad sizes");
    SAT_CHECK_ARG(cfg->run_layers >= 0 && cfg->run_layers <= cfg->num_layers, SAT_E_INVALID,
                  "roberta_plan_create: run_layers %d outside [0, %d] (hidden_states has num_layers + 1 entries)", cfg->run_layers,
                  cfg->num_layers);
    SAT_CHECK_ARG(cfg->pad_id >= 0 && cfg->pad_id < cfg->vocab_size && cfg->max_positions > cfg->pad_id + 1, SAT_E_INVALID,
                  "roberta_plan_create: pad_id %d / max_positions %d: positions start at pad_id + 1", cfg->pad_id, cfg->max_positions);
    SAT_CHECK_ARG(cfg->hidden_size % cfg->num_heads == 0, SAT_E_INVALID, "roberta_plan_create: hidden_size %d is not a multiple of num_heads %d",
                  cfg->hidden_size, cfg->num_heads);
    const int dh = cfg->hidden_size / cfg->num_heads;
    SAT_CHECK_ARG(cfg->hidden_size % 16 == 0 && cfg->intermediate_size % 16 == 0 && dh % 16 == 0 && dh <= 256, SAT_E_UNSUPPORTED,
                  "roberta_plan_create: hidden_size %d / intermediate_size %d / head dim %d must be multiples of 16 (head dim <= 256)",
                  cfg->hidden_size, cfg->intermediate_size, dh);
    SAT_CHECK_ARG(cfg->eps > 0.f && cfg->proj_dim >= 0, SAT_E_INVALID, "roberta_plan_create: layer_norm_eps must be positive, proj_dim >= 0");
    sat_roberta_plan* p = new (std::nothrow) sat_roberta_plan();
    SAT_CHECK_ARG(p, SAT_E_INVALID, "roberta_plan_create: out of host memory");
    p->cfg = *cfg;
    *out_plan = p;
    return 0;
}

extern "C" void sat_roberta_plan_destroy(sat_roberta_plan* p) { delete p; }

extern "C" int sat_roberta_plan_set_tensor(sat_roberta_plan* p, const char* name, const float* data_dev, int64_t numel) {
    SAT_CHECK_ARG(p, SAT_E_INVALID, "roberta_plan_set_tensor: bad argument");
    return p->tensors.set("roberta", name, data_dev, numel);
}

namespace {

// the longest sequence the position table serves: the last token of a pad-free sequence sits at pad_id + l
int roberta_max_len(const sat_roberta_cfg& c) {
    const int by_table = c.max_positions - c.pad_id - 1, by_kernel = 64 * ENC_MAX_KEYS_PER_LANE;
    return by_table < by_kernel ? by_table : by_kernel;
}

// two passes over the same code (plan_finalize): sizes first (ar.dry()), then copies
int roberta_build(sat_roberta_plan* p, Bump& ar, hipStream_t s) {
    const sat_roberta_cfg& c = p->cfg;
    const int64_t D = c.hidden_size, F = c.intermediate_size;
    // the named tensor as part `part` of a buffer of equal parts stacked behind each other
    auto fill = [&](const std::string& name, int64_t numel, float* dst, int part) -> int {
        return ar.dry() ? 0 : p->tensors.copy("roberta", name, numel, dst + part * numel, s);
    };
    auto place = [&](const std::string& name, int64_t numel, float** dst, bool first_rows = false) -> int {
        return p->tensors.place("roberta", ar, name, numel, dst, s, first_rows);
    };
    SAT_TRY(place("embeddings.word_embeddings.weight", (int64_t)c.vocab_size * D, &p->word));
    SAT_TRY(place("embeddings.position_embeddings.weight", (int64_t)c.max_positions * D, &p->posw));
    // [type_vocab_size, D]; the encoder is called without token_type_ids, i.e. with zeros: row 0 only
    SAT_TRY(place("embeddings.token_type_embeddings.weight", D, &p->type0, true));
    SAT_TRY(place("embeddings.LayerNorm.weight", D, &p->emb_g));
    SAT_TRY(place("embeddings.LayerNorm.bias", D, &p->emb_b));
    if (c.proj_dim > 0) {
        SAT_TRY(place("proj_out.weight", (int64_t)c.proj_dim * D, &p->proj_w));
        SAT_TRY(place("proj_out.bias", c.proj_dim, &p->proj_b));
    }
    p->layers.resize(c.run_layers);
    for (int l = 0; l < c.run_layers; ++l) {          // the layers above run_layers are neither asked for nor uploaded
        RobertaLayer& L = p->layers[l];
        const std::string pf = "encoder.layer." + std::to_string(l) + ".";
        // query | key | value stacked into one [3D, D] weight and one [3D] bias: one GEMM
        L.wqkv = (float*)ar.take((size_t)(3 * D * D) * 4);
        L.bqkv = (float*)ar.take((size_t)(3 * D) * 4);
        const char* qkv[3] = {"query", "key", "value"};
        for (int i = 0; i < 3; ++i) {
            SAT_TRY(fill(pf + "attention.self." + qkv[i] + ".weight", D * D, L.wqkv, i));
            SAT_TRY(fill(pf + "attention.self." + qkv[i] + ".bias", D, L.bqkv, i));
        }
        SAT_TRY(place(pf + "attention.output.dense.weight", D * D, &L.wo));
        SAT_TRY(place(pf + "attention.output.dense.bias", D, &L.bo));
        SAT_TRY(place(pf + "attention.output.LayerNorm.weight", D, &L.ln1g));
        SAT_TRY(place(pf + "attention.output.LayerNorm.bias", D, &L.ln1b));
        SAT_TRY(place(pf + "intermediate.dense.weight", F * D, &L.w1));
        SAT_TRY(place(pf + "intermediate.dense.bias", F, &L.b1));
        SAT_TRY(place(pf + "output.dense.weight", D * F, &L.w2));
        SAT_TRY(place(pf + "output.dense.bias", D, &L.b2));
        SAT_TRY(place(pf + "output.LayerNorm.weight", D, &L.ln2g));
        SAT_TRY(place(pf + "output.LayerNorm.bias", D, &L.ln2b));
    }
    return 0;
}

struct RobertaWs {
    float *ha, *hb, *qkv, *att, *ff;
    size_t total;
};

RobertaWs roberta_carve(const sat_roberta_plan* p, int b, int l, char* base) {
    const sat_roberta_cfg& c = p->cfg;
    const size_t M = (size_t)b * l, D = c.hidden_size, F = c.intermediate_size;
    Bump ws{base};
    RobertaWs w;
    w.ha = (float*)ws.take(M * D * 4);
    w.hb = (float*)ws.take(M * D * 4);
    w.qkv = (float*)ws.take(M * 3 * D * 4);
    w.att = (float*)ws.take(M * D * 4);
    w.ff = (float*)ws.take(M * F * 4);
    w.total = ws.off;
    return w;
}

}  // namespace

extern "C" int sat_roberta_plan_finalize(sat_roberta_plan* p, sat_stream_t stream) {
    SAT_CHECK_ARG(p, SAT_E_INVALID, "roberta_plan_finalize: null plan");
    hipStream_t s = (hipStream_t)stream;
    return plan_finalize(p, s, [&](Bump& ar) { return roberta_build(p, ar, s); });
}

extern "C" int sat_roberta_workspace_bytes(const sat_roberta_plan* p, int32_t b, int32_t l, size_t* out_bytes) {
    SAT_CHECK_ARG(p && out_bytes && b > 0 && l > 0, SAT_E_INVALID, "roberta_workspace_bytes: bad arguments");
    SAT_CHECK_ARG(l <= roberta_max_len(p->cfg), SAT_E_UNSUPPORTED,
                  "roberta_workspace_bytes: sequence length %d > %d (max_positions %d - pad_id %d - 1, and at most %d keys)", l,
                  roberta_max_len(p->cfg), p->cfg.max_positions, p->cfg.pad_id, 64 * ENC_MAX_KEYS_PER_LANE);
    *out_bytes = roberta_carve(p, b, l, nullptr).total;
    return 0;
}

extern "C" int sat_roberta_encode(sat_roberta_plan* p, const int32_t* input_ids_dev, const int32_t* attention_mask_dev, float* out_dev,
                                  int32_t b, int32_t l, void* ws, size_t ws_bytes, sat_stream_t stream) {
    SAT_CHECK_ARG(p && p->finalized, SAT_E_STATE, "roberta_encode: plan not finalized");
    SAT_CHECK_ARG(input_ids_dev && attention_mask_dev && out_dev && ws && b > 0 && l > 0, SAT_E_INVALID, "roberta_encode: bad arguments");
    const sat_roberta_cfg& c = p->cfg;
    SAT_CHECK_ARG(l <= roberta_max_len(c), SAT_E_UNSUPPORTED,
                  "roberta_encode: sequence length %d > %d (max_positions %d - pad_id %d - 1, and at most %d keys)", l, roberta_max_len(c),
                  c.max_positions, c.pad_id, 64 * ENC_MAX_KEYS_PER_LANE);
    SAT_CHECK_ARG(((uintptr_t)ws & 255) == 0, SAT_E_INVALID, "roberta_encode: workspace must be 256-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    RobertaWs w = roberta_carve(p, b, l, (char*)ws);
    SAT_CHECK_ARG(ws_bytes >= w.total, SAT_E_WORKSPACE, "roberta_encode: workspace %zu < required %zu", ws_bytes, w.total);
    const int M = b * l, D = c.hidden_size, H = c.num_heads, dh = D / H, F = c.intermediate_size;
    const bool proj = c.proj_dim > 0;

    // hidden_states[run_layers] lands in `ha`; without layers and without proj_out the embeddings are the output
    float* ha = (c.run_layers == 0 && !proj) ? out_dev : w.ha;
    SAT_TRY(roberta_launch_embed_ln(input_ids_dev, p->word, p->posw, p->type0, p->emb_g, p->emb_b, ha, b, l, D, c.vocab_size, c.pad_id,
                                    c.max_positions, c.eps, s));
    const float scale = 1.0f / sqrtf((float)dh);
    for (int li = 0; li < c.run_layers; ++li) {
        const RobertaLayer& L = p->layers[li];
        const bool last = li == c.run_layers - 1;
        SAT_TRY(sat_launch_gemm_f32(ha, L.wqkv, L.bqkv, w.qkv, M, 3 * D, D, 3 * D, 0, nullptr, 1, 0, s));
        SAT_TRY(enc_attention_launch(w.qkv, nullptr, attention_mask_dev, w.att, b, l, H, dh, scale, s));
        // the residuals ride the GEMM's accumulate path: ha += att Wo^T + bo, then hb = LN(ha)
        SAT_TRY(sat_launch_gemm_f32(w.att, L.wo, L.bo, ha, M, D, D, D, 1, nullptr, 1, 0, s));
        SAT_TRY(sat_launch_layernorm_f32(ha, L.ln1g, L.ln1b, w.hb, M, D, nullptr, nullptr, 1, 0, s, c.eps));
        SAT_TRY(sat_launch_gemm_f32(w.hb, L.w1, L.b1, w.ff, M, F, D, F, 0, nullptr, 1, 0, s));
        SAT_TRY(roberta_launch_gelu(w.ff, (int64_t)M * F, s));
        SAT_TRY(sat_launch_gemm_f32(w.ff, L.w2, L.b2, w.hb, M, D, F, D, 1, nullptr, 1, 0, s));
        float* next = (last && !proj) ? out_dev : w.ha;
        SAT_TRY(sat_launch_layernorm_f32(w.hb, L.ln2g, L.ln2b, next, M, D, nullptr, nullptr, 1, 0, s, c.eps));
        ha = next;
    }
    // padded rows are NOT zeroed: the reference returns proj_out(text_features) as is (conditioners.py:182)
    if (proj) SAT_TRY(sat_launch_gemm_f32(ha, p->proj_w, p->proj_b, out_dev, M, c.proj_dim, D, c.proj_dim, 0, nullptr, 1, 0, s));
    return 0;
}

// ---- unit entries (include/sat_hip.h): one kernel each on caller tensors, through the launchers sat_roberta_encode uses
extern "C" int sat_roberta_embed_ln(const int32_t* ids, const float* word, const float* posw, const float* type0, const float* gamma,
                                    const float* beta, float* y, int32_t b, int32_t l, int32_t d, int32_t vocab, int32_t pad_id,
                                    int32_t max_positions, float eps, sat_stream_t stream) {
    return roberta_launch_embed_ln(ids, word, posw, type0, gamma, beta, y, b, l, d, vocab, pad_id, max_positions, eps, (hipStream_t)stream);
}
extern "C" int sat_roberta_gelu(float* h, int64_t n, sat_stream_t stream) { return roberta_launch_gelu(h, n, (hipStream_t)stream); }
