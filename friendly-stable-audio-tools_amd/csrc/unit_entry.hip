// Unit-level C entry points (include/sat_hip.h): one kernel launcher each, for tests, probes and callers that drive single
// operations; the bf16 / fp16 pairs share an _impl.  Host code only; no kernel, nothing of the DiT plan.
#include "sat_common.h"
#include "dit_glue.h"

// ------------------------------------------------------------------------------ unit-level entry points
static int layernorm_bf16_impl(int f16, const float* x, const float* gamma, const float* beta, void* y, int32_t m, int32_t d,
                                  sat_stream_t stream) {
    return sat_launch_layernorm(x, gamma, beta, (op_t*)y, m, d, (hipStream_t)stream, f16);
}
extern "C" int sat_layernorm_bf16(const float* x, const float* gamma, const float* beta, void* y, int32_t m, int32_t d,
                                  sat_stream_t stream) {
    return layernorm_bf16_impl(0, x, gamma, beta, y, m, d, stream);
}
extern "C" int sat_layernorm_f16(const float* x, const float* gamma, const float* beta, void* y, int32_t m, int32_t d,
                                  sat_stream_t stream) {
    return layernorm_bf16_impl(1, x, gamma, beta, y, m, d, stream);
}

static int cast_bf16_impl(int f16, const float* x, void* y, int64_t n, sat_stream_t stream) {
    return sat_launch_cast_bf16(x, (op_t*)y, n, (hipStream_t)stream, f16);
}
extern "C" int sat_cast_bf16(const float* x, void* y, int64_t n, sat_stream_t stream) {
    return cast_bf16_impl(0, x, y, n, stream);
}
extern "C" int sat_cast_f16(const float* x, void* y, int64_t n, sat_stream_t stream) {
    return cast_bf16_impl(1, x, y, n, stream);
}

static int range_stats_impl(int dtype, const void* x, int64_t rows, int64_t cols, int64_t pitch, sat_range_record* record, sat_stream_t stream) {
    SAT_CHECK_ARG(rows > 0 && cols > 0, SAT_E_INVALID, "range_stats: view of %lld x %lld", (long long)rows, (long long)cols);
    return sat_launch_range_stats(x, dtype, rows, cols, pitch, (uint64_t)rows * (uint64_t)cols, record, (hipStream_t)stream);
}
extern "C" int sat_range_stats_f16(const void* x, int64_t rows, int64_t cols, int64_t pitch, sat_range_record* record, sat_stream_t stream) {
    return range_stats_impl(SAT_GEMM_FP16, x, rows, cols, pitch, record, stream);
}
extern "C" int sat_range_stats_bf16(const void* x, int64_t rows, int64_t cols, int64_t pitch, sat_range_record* record, sat_stream_t stream) {
    return range_stats_impl(SAT_GEMM_BF16, x, rows, cols, pitch, record, stream);
}
extern "C" int sat_range_stats_f32(const void* x, int64_t rows, int64_t cols, int64_t pitch, sat_range_record* record, sat_stream_t stream) {
    return range_stats_impl(SAT_GEMM_FP32X, x, rows, cols, pitch, record, stream);
}

// ---- the fp32 verification path (f32_ref.hip), one kernel each: the launchers the DiT plan and both text encoders call
extern "C" int sat_gemm_f32(const float* a, const float* w, const float* bias, float* c, int32_t m, int32_t n, int32_t k, int32_t ldc,
                            int32_t accumulate, const float* gate, int32_t gate_rows, int32_t gate_ld, sat_stream_t stream) {
    SAT_CHECK_ARG(!gate || gate_rows > 0, SAT_E_INVALID, "gemm_f32: gate_rows %d", gate_rows);
    return sat_launch_gemm_f32(a, w, bias, c, m, n, k, ldc, accumulate, gate, gate_rows, gate_ld, (hipStream_t)stream);
}
extern "C" int sat_layernorm_f32(const float* x, const float* gamma, const float* beta, float* y, int32_t m, int32_t d, const float* scale,
                                 const float* shift, int32_t rows_per_seq, int32_t ld, float eps, sat_stream_t stream) {
    SAT_CHECK_ARG(!scale || rows_per_seq > 0, SAT_E_INVALID, "layernorm_f32: rows_per_seq %d", rows_per_seq);
    SAT_CHECK_ARG(eps > 0.f, SAT_E_INVALID, "layernorm_f32: eps must be positive");
    return sat_launch_layernorm_f32(x, gamma, beta, y, m, d, scale, shift, rows_per_seq, ld, (hipStream_t)stream, eps);
}
extern "C" int sat_split_heads_f32(const float* src, float* d0, float* d1, float* d2, int32_t b, int32_t s_len, int32_t parts, int32_t heads,
                                   int32_t rope_mask, const float* rope_cos, const float* rope_sin, int32_t norm_mask, sat_stream_t stream) {
    SAT_CHECK_ARG(b > 0 && s_len > 0 && (int64_t)b * s_len <= INT32_MAX, SAT_E_INVALID, "split_heads_f32: b %d, s_len %d", b, s_len);
    return sat_launch_split_heads_f32(src, d0, d1, d2, b * s_len, s_len, parts, heads, rope_mask, rope_cos, rope_sin, (hipStream_t)stream, norm_mask);
}
extern "C" int sat_swiglu_f32(const float* hg, float* h, int64_t m, int32_t inner, sat_stream_t stream) {
    return sat_launch_swiglu_f32(hg, h, m, inner, (hipStream_t)stream);
}
extern "C" int sat_attention_f32(const float* q, const float* k, const float* v, float* out, int32_t b, int32_t h, int32_t kvh, int32_t sq,
                                 int32_t sk, sat_stream_t stream) {
    return sat_launch_attention_f32(q, k, v, out, b, h, kvh, sq, sk, (hipStream_t)stream);
}

static int gemm_bf16_f32_impl(int f16, const void* a, const void* w, const float* bias, float* c, int32_t m, int32_t n, int32_t k,
                              int32_t accumulate, int32_t variant, void* ws, size_t ws_bytes, sat_stream_t stream) {
    SAT_CHECK_ARG(c, SAT_E_INVALID, "gemm: null output");
    GemmArgs g{};
    g.f16 = f16;
    g.A = (const op_t*)a; g.W = (const op_t*)w; g.bias = bias; g.M = m; g.N = n; g.K = k;
    g.C = c; g.ldc = n; g.accumulate = accumulate; g.variant = variant;
    g.slab = (float*)ws; g.slab_bytes = ws ? ws_bytes : 0;
    return sat_launch_gemm(EPI_F32, g, (hipStream_t)stream);
}
extern "C" int sat_gemm_bf16_f32(const void* a, const void* w, const float* bias, float* c, int32_t m, int32_t n, int32_t k,
                                 int32_t accumulate, int32_t variant, sat_stream_t stream) {
    return gemm_bf16_f32_impl(0, a, w, bias, c, m, n, k, accumulate, variant, nullptr, 0, stream);
}
extern "C" int sat_gemm_f16_f32(const void* a, const void* w, const float* bias, float* c, int32_t m, int32_t n, int32_t k,
                                int32_t accumulate, int32_t variant, sat_stream_t stream) {
    return gemm_bf16_f32_impl(1, a, w, bias, c, m, n, k, accumulate, variant, nullptr, 0, stream);
}
extern "C" int sat_gemm_bf16_f32_ws(const void* a, const void* w, const float* bias, float* c, int32_t m, int32_t n, int32_t k,
                                    int32_t accumulate, int32_t variant, void* ws, size_t ws_bytes, sat_stream_t stream) {
    return gemm_bf16_f32_impl(0, a, w, bias, c, m, n, k, accumulate, variant, ws, ws_bytes, stream);
}
extern "C" int sat_gemm_f16_f32_ws(const void* a, const void* w, const float* bias, float* c, int32_t m, int32_t n, int32_t k,
                                   int32_t accumulate, int32_t variant, void* ws, size_t ws_bytes, sat_stream_t stream) {
    return gemm_bf16_f32_impl(1, a, w, bias, c, m, n, k, accumulate, variant, ws, ws_bytes, stream);
}
extern "C" int sat_gemm_f32_workspace_bytes(int32_t m, int32_t n, int32_t k, int32_t variant, size_t* out_bytes) {
    SAT_CHECK_ARG(out_bytes && m > 0 && n > 0 && k > 0, SAT_E_INVALID, "gemm_f32_workspace_bytes: bad argument");
    const int cus = sat_device_cus();
    SAT_CHECK_ARG(cus > 0, SAT_E_INVALID, "gemm_f32_workspace_bytes: no device");
    // forced K-split (tests / measurements): one slab per workgroup; otherwise what the automatic schedule would use
    *out_bytes = sat_variant_has(variant, SAT_VARIANT_SPLIT_FORCE) ? (size_t)cus * 65536 * sizeof(float) : sat_gemm_ph8_slab_bytes(EPI_F32, m, n, k);
    return 0;
}

static int gemm_swiglu_bf16_impl(int f16, const void* a, const float* w_f32, const float* bias_f32, void* wpack, float* bpack,
                                    void* h, int32_t m, int32_t n, int32_t k, int32_t variant, sat_stream_t stream) {
    SAT_CHECK_ARG(w_f32 && wpack && bpack && h, SAT_E_INVALID, "gemm_swiglu: null pointer");
    hipStream_t s = (hipStream_t)stream;
    if (!sat_variant_has(variant, SAT_VARIANT_PACKED)) {     // wpack / bpack already hold the packed operands of a previous call (benchmarks)
        SAT_TRY(sat_launch_pack_rows_bf16(w_f32, (op_t*)wpack, n, k, 1, s, f16));
        if (bias_f32) SAT_TRY(sat_launch_pack_bias(bias_f32, bpack, n, 1, s));
    }
    GemmArgs g{};
    g.f16 = f16;
    g.A = (const op_t*)a; g.W = (const op_t*)wpack; g.bias = bias_f32 ? bpack : nullptr; g.M = m; g.N = n; g.K = k;
    g.H = (op_t*)h; g.variant = variant & ~SAT_VARIANT_PACKED;
    return sat_launch_gemm(EPI_SWIGLU, g, s);
}
extern "C" int sat_gemm_swiglu_bf16(const void* a, const float* w_f32, const float* bias_f32, void* wpack, float* bpack,
                                    void* h, int32_t m, int32_t n, int32_t k, int32_t variant, sat_stream_t stream) {
    return gemm_swiglu_bf16_impl(0, a, w_f32, bias_f32, wpack, bpack, h, m, n, k, variant, stream);
}
extern "C" int sat_gemm_swiglu_f16(const void* a, const float* w_f32, const float* bias_f32, void* wpack, float* bpack,
                                    void* h, int32_t m, int32_t n, int32_t k, int32_t variant, sat_stream_t stream) {
    return gemm_swiglu_bf16_impl(1, a, w_f32, bias_f32, wpack, bpack, h, m, n, k, variant, stream);
}

static int attention_bf16_impl(int f16, const void* q, const void* k, const void* vt, void* out, int32_t b, int32_t h, int32_t kvh,
                                  int32_t sq, int32_t sk, int32_t sq_pad, int32_t sk_pad, sat_stream_t stream) {
    return sat_launch_attention((const op_t*)q, (const op_t*)k, (const op_t*)vt, (op_t*)out, b, h, kvh, sq, sk, sq_pad,
                                sk_pad, (hipStream_t)stream, nullptr, SAT_ATTN_QSCALE, f16);
}
extern "C" int sat_attention_bf16(const void* q, const void* k, const void* vt, void* out, int32_t b, int32_t h, int32_t kvh,
                                  int32_t sq, int32_t sk, int32_t sq_pad, int32_t sk_pad, sat_stream_t stream) {
    return attention_bf16_impl(0, q, k, vt, out, b, h, kvh, sq, sk, sq_pad, sk_pad, stream);
}
extern "C" int sat_attention_f16(const void* q, const void* k, const void* vt, void* out, int32_t b, int32_t h, int32_t kvh,
                                  int32_t sq, int32_t sk, int32_t sq_pad, int32_t sk_pad, sat_stream_t stream) {
    return attention_bf16_impl(1, q, k, vt, out, b, h, kvh, sq, sk, sq_pad, sk_pad, stream);
}

// to_q projection + cross-attention in ONE launch (what the plan runs per layer at one prompt): out [b*s, d] = attention(a wq^T, k, v)
static int cross_attention_fused_bf16_impl(int f16, const void* a, const void* wq, const void* k, const void* vt, void* out, int32_t b, int32_t s_len,
                                              int32_t d, int32_t kvh, int32_t sk, int32_t sk_pad, sat_stream_t stream) {
    SAT_CHECK_ARG(a && wq && k && vt && out && b > 0 && s_len > 0 && d > 0 && d % 128 == 0 && kvh > 0, SAT_E_INVALID, "cross_attention_fused: bad argument");
    GemmArgs g{};
    g.f16 = f16;
    g.A = (const op_t*)a; g.W = (const op_t*)wq; g.M = b * s_len; g.N = d; g.K = d;
    g.heads.kind[0] = 8; g.heads.qscale = SAT_ATTN_QSCALE; g.heads.parts = 1; g.heads.heads = d / 64; g.heads.S = s_len; g.heads.Spad = s_len;
    g.heads.xa_k = (const op_t*)k; g.heads.xa_vt = (const op_t*)vt; g.heads.xa_out = (op_t*)out;
    g.heads.xa_kvh = kvh; g.heads.xa_sk = sk; g.heads.xa_sk_pad = sk_pad;
    return sat_launch_gemm(EPI_HEADS, g, (hipStream_t)stream);
}
extern "C" int sat_cross_attention_fused_bf16(const void* a, const void* wq, const void* k, const void* vt, void* out, int32_t b, int32_t s_len,
                                              int32_t d, int32_t kvh, int32_t sk, int32_t sk_pad, sat_stream_t stream) {
    return cross_attention_fused_bf16_impl(0, a, wq, k, vt, out, b, s_len, d, kvh, sk, sk_pad, stream);
}
extern "C" int sat_cross_attention_fused_f16(const void* a, const void* wq, const void* k, const void* vt, void* out, int32_t b, int32_t s_len,
                                              int32_t d, int32_t kvh, int32_t sk, int32_t sk_pad, sat_stream_t stream) {
    return cross_attention_fused_bf16_impl(1, a, wq, k, vt, out, b, s_len, d, kvh, sk, sk_pad, stream);
}

// The layout the DiT plan runs: Q pre-scaled by 1/sqrt(64) * log2(e) by its producer (the QKV / to_q GEMM epilogue)
static int attention_prescaled_bf16_impl(int f16, const void* q, const void* k, const void* vt, void* out, int32_t b, int32_t h, int32_t kvh,
                                            int32_t sq, int32_t sk, int32_t sq_pad, int32_t sk_pad, sat_stream_t stream) {
    return sat_launch_attention((const op_t*)q, (const op_t*)k, (const op_t*)vt, (op_t*)out, b, h, kvh, sq, sk, sq_pad,
                                sk_pad, (hipStream_t)stream, nullptr, 1.0f, f16);
}
extern "C" int sat_attention_prescaled_bf16(const void* q, const void* k, const void* vt, void* out, int32_t b, int32_t h, int32_t kvh,
                                            int32_t sq, int32_t sk, int32_t sq_pad, int32_t sk_pad, sat_stream_t stream) {
    return attention_prescaled_bf16_impl(0, q, k, vt, out, b, h, kvh, sq, sk, sq_pad, sk_pad, stream);
}
extern "C" int sat_attention_prescaled_f16(const void* q, const void* k, const void* vt, void* out, int32_t b, int32_t h, int32_t kvh,
                                            int32_t sq, int32_t sk, int32_t sq_pad, int32_t sk_pad, sat_stream_t stream) {
    return attention_prescaled_bf16_impl(1, q, k, vt, out, b, h, kvh, sq, sk, sq_pad, sk_pad, stream);
}

// ---- 32-, 96- and 128-channel heads: the attention kernel and the head split of the plan's staged route (attention_hdw.hip,
// head_split_hdw.hip), and the fp32 verification kernels with a head width.  The *_hd128_* entry points pass 128; the *_hdw_* ones take 32 or 96
static int attention_hdw_impl(int f16, const void* q, const void* k, const void* vt, void* out, int32_t b, int32_t h, int32_t kvh, int32_t head_dim,
                              int32_t sq, int32_t sk, int32_t sq_pad, int32_t sk_pad, sat_stream_t stream) {
    return sat_launch_attention_hdw((const op_t*)q, (const op_t*)k, (const op_t*)vt, (op_t*)out, b, h, kvh, head_dim, sq, sk, sq_pad, sk_pad,
                                    (hipStream_t)stream, f16);
}
extern "C" int sat_attention_hd128_bf16(const void* q, const void* k, const void* vt, void* out, int32_t b, int32_t h, int32_t kvh, int32_t sq,
                                        int32_t sk, int32_t sq_pad, int32_t sk_pad, sat_stream_t stream) {
    return attention_hdw_impl(0, q, k, vt, out, b, h, kvh, 128, sq, sk, sq_pad, sk_pad, stream);
}
extern "C" int sat_attention_hd128_f16(const void* q, const void* k, const void* vt, void* out, int32_t b, int32_t h, int32_t kvh, int32_t sq,
                                       int32_t sk, int32_t sq_pad, int32_t sk_pad, sat_stream_t stream) {
    return attention_hdw_impl(1, q, k, vt, out, b, h, kvh, 128, sq, sk, sq_pad, sk_pad, stream);
}
static int hdw_entry_width(const char* what, int32_t head_dim) {
    SAT_CHECK_ARG(head_dim == 32 || head_dim == 96, SAT_E_UNSUPPORTED, "%s: dim_heads %d (this entry point takes 32 and 96)", what, head_dim);
    return 0;
}
extern "C" int sat_attention_hdw_bf16(const void* q, const void* k, const void* vt, void* out, int32_t b, int32_t h, int32_t kvh, int32_t head_dim,
                                      int32_t sq, int32_t sk, int32_t sq_pad, int32_t sk_pad, sat_stream_t stream) {
    SAT_TRY(hdw_entry_width("attention_hdw", head_dim));
    return attention_hdw_impl(0, q, k, vt, out, b, h, kvh, head_dim, sq, sk, sq_pad, sk_pad, stream);
}
extern "C" int sat_attention_hdw_f16(const void* q, const void* k, const void* vt, void* out, int32_t b, int32_t h, int32_t kvh, int32_t head_dim,
                                     int32_t sq, int32_t sk, int32_t sq_pad, int32_t sk_pad, sat_stream_t stream) {
    SAT_TRY(hdw_entry_width("attention_hdw", head_dim));
    return attention_hdw_impl(1, q, k, vt, out, b, h, kvh, head_dim, sq, sk, sq_pad, sk_pad, stream);
}

static int head_split_hdw_impl(int f16, const float* x, const float* inv_freq, void* const* dst, const int32_t* kind, float* rope_scratch, int32_t b,
                               int32_t s_len, int32_t s_pad, int32_t heads, int32_t head_dim, int32_t parts, sat_stream_t stream) {
    SAT_CHECK_ARG(x && dst && kind && b > 0 && s_len > 0 && heads > 0 && parts >= 1 && parts <= 3, SAT_E_INVALID, "head_split_hdw: bad argument");
    SAT_CHECK_ARG(s_pad % 64 == 0 && s_pad >= s_len + 3, SAT_E_INVALID, "head_split_hdw: bad dims (s_pad >= s + 3, %% 64)");
    hipStream_t s = (hipStream_t)stream;
    const int pairs = sat_rope_pairs(head_dim);
    HeadsEpi he{};
    bool rope = false;
    for (int pt = 0; pt < parts; ++pt) {
        SAT_CHECK_ARG(dst[pt] && ((uintptr_t)dst[pt] & 15) == 0, SAT_E_INVALID, "head_split_hdw: destination %d null or not 16-byte aligned", pt);
        rope = rope || (kind[pt] & 2);
    }
    SAT_CHECK_ARG(((uintptr_t)x & 15) == 0, SAT_E_INVALID, "head_split_hdw: the input must be 16-byte aligned");
    SAT_CHECK_ARG(!rope || (inv_freq && rope_scratch && ((uintptr_t)rope_scratch & 15) == 0), SAT_E_INVALID,
                  "head_split_hdw: a rotating part needs inv_freq and a 16-byte aligned rope_scratch");
    for (int pt = 0; pt < parts; ++pt) {
        SAT_HIP(hipMemsetAsync(dst[pt], 0, (size_t)b * heads * s_pad * head_dim * 2, s));
        he.out[pt] = (op_t*)dst[pt];
        he.kind[pt] = kind[pt];
    }
    if (rope) {
        he.rope_cos = rope_scratch;
        he.rope_sin = rope_scratch + (size_t)s_len * pairs;
        SAT_TRY(sat_launch_rope_table_hdw(inv_freq, rope_scratch, rope_scratch + (size_t)s_len * pairs, s_len, head_dim, s));
    }
    he.qscale = sat_attn_qscale(head_dim); he.parts = parts; he.heads = heads; he.S = s_len; he.Spad = s_pad;
    return sat_launch_head_split_hdw(x, he, head_dim, b, s, f16);
}
extern "C" int sat_head_split_hd128_bf16(const float* x, const float* inv_freq, void* const* dst, const int32_t* kind, float* rope_scratch,
                                         int32_t b, int32_t s_len, int32_t s_pad, int32_t heads, int32_t parts, sat_stream_t stream) {
    return head_split_hdw_impl(0, x, inv_freq, dst, kind, rope_scratch, b, s_len, s_pad, heads, 128, parts, stream);
}
extern "C" int sat_head_split_hd128_f16(const float* x, const float* inv_freq, void* const* dst, const int32_t* kind, float* rope_scratch,
                                        int32_t b, int32_t s_len, int32_t s_pad, int32_t heads, int32_t parts, sat_stream_t stream) {
    return head_split_hdw_impl(1, x, inv_freq, dst, kind, rope_scratch, b, s_len, s_pad, heads, 128, parts, stream);
}
extern "C" int sat_head_split_hdw_bf16(const float* x, const float* inv_freq, void* const* dst, const int32_t* kind, float* rope_scratch, int32_t b,
                                       int32_t s_len, int32_t s_pad, int32_t heads, int32_t head_dim, int32_t parts, sat_stream_t stream) {
    SAT_TRY(hdw_entry_width("head_split_hdw", head_dim));
    return head_split_hdw_impl(0, x, inv_freq, dst, kind, rope_scratch, b, s_len, s_pad, heads, head_dim, parts, stream);
}
extern "C" int sat_head_split_hdw_f16(const float* x, const float* inv_freq, void* const* dst, const int32_t* kind, float* rope_scratch, int32_t b,
                                      int32_t s_len, int32_t s_pad, int32_t heads, int32_t head_dim, int32_t parts, sat_stream_t stream) {
    SAT_TRY(hdw_entry_width("head_split_hdw", head_dim));
    return head_split_hdw_impl(1, x, inv_freq, dst, kind, rope_scratch, b, s_len, s_pad, heads, head_dim, parts, stream);
}
extern "C" int sat_split_heads_f32_hdw(const float* src, float* d0, float* d1, float* d2, int32_t b, int32_t s_len, int32_t parts, int32_t heads,
                                       int32_t head_dim, int32_t rope_mask, const float* rope_cos, const float* rope_sin, int32_t norm_mask,
                                       sat_stream_t stream) {
    SAT_CHECK_ARG(head_dim == 32 || head_dim == 64 || head_dim == 96, SAT_E_UNSUPPORTED, "split_heads_f32: dim_heads %d (built for 32, 64 and 96)", head_dim);
    SAT_CHECK_ARG(b > 0 && s_len > 0 && (int64_t)b * s_len <= INT32_MAX, SAT_E_INVALID, "split_heads_f32: b %d, s_len %d", b, s_len);
    return sat_launch_split_heads_f32_w(src, d0, d1, d2, b * s_len, s_len, parts, heads, head_dim, rope_mask, rope_cos, rope_sin, (hipStream_t)stream,
                                        norm_mask);
}
extern "C" int sat_attention_f32_hdw(const float* q, const float* k, const float* v, float* out, int32_t b, int32_t h, int32_t kvh, int32_t head_dim,
                                     int32_t sq, int32_t sk, sat_stream_t stream) {
    SAT_CHECK_ARG(head_dim == 32 || head_dim == 64 || head_dim == 96, SAT_E_UNSUPPORTED, "attention_f32: dim_heads %d (built for 32, 64 and 96)", head_dim);
    return sat_launch_attention_f32_w(q, k, v, out, b, h, kvh, head_dim, sq, sk, (hipStream_t)stream);
}

// ---- causal self-attention alone (sat_dit_plan_set_attention_options): the three launchers Forward calls.  head_dim 64 is attention.hip
// (prescaled 0: a plain Q, scaled here; 1: a Q pre-scaled by log2(e) / 8), 32 / 96 / 128 attention_hdw.hip (Q always pre-scaled)
static int attention_causal_impl(int f16, const void* q, const void* k, const void* vt, void* out, int32_t b, int32_t h, int32_t kvh, int32_t head_dim,
                                 int32_t s, int32_t s_pad_q, int32_t s_pad_k, int32_t prescaled, sat_stream_t stream) {
    SAT_CHECK_ARG(head_dim == 32 || head_dim == 64 || head_dim == 96 || head_dim == 128, SAT_E_UNSUPPORTED,
                  "attention_causal: dim_heads %d (built for 32, 64, 96 and 128)", head_dim);
    SAT_CHECK_ARG(prescaled == 0 || prescaled == 1, SAT_E_INVALID, "attention_causal: prescaled %d is neither 0 nor 1", prescaled);
    SAT_CHECK_ARG(head_dim == 64 || prescaled == 1, SAT_E_UNSUPPORTED, "attention_causal: dim_heads %d takes a pre-scaled Q only", head_dim);
    if (head_dim == 64)
        return sat_launch_attention_causal((const op_t*)q, (const op_t*)k, (const op_t*)vt, (op_t*)out, b, h, kvh, s, s_pad_q, s_pad_k, (hipStream_t)stream,
                                           prescaled ? 1.0f : SAT_ATTN_QSCALE, f16);
    return sat_launch_attention_hdw_causal((const op_t*)q, (const op_t*)k, (const op_t*)vt, (op_t*)out, b, h, kvh, head_dim, s, s_pad_q, s_pad_k,
                                           (hipStream_t)stream, f16);
}
extern "C" int sat_attention_causal_bf16(const void* q, const void* k, const void* vt, void* out, int32_t b, int32_t h, int32_t kvh, int32_t head_dim,
                                         int32_t s, int32_t s_pad_q, int32_t s_pad_k, int32_t prescaled, sat_stream_t stream) {
    return attention_causal_impl(0, q, k, vt, out, b, h, kvh, head_dim, s, s_pad_q, s_pad_k, prescaled, stream);
}
extern "C" int sat_attention_causal_f16(const void* q, const void* k, const void* vt, void* out, int32_t b, int32_t h, int32_t kvh, int32_t head_dim,
                                        int32_t s, int32_t s_pad_q, int32_t s_pad_k, int32_t prescaled, sat_stream_t stream) {
    return attention_causal_impl(1, q, k, vt, out, b, h, kvh, head_dim, s, s_pad_q, s_pad_k, prescaled, stream);
}
extern "C" int sat_attention_f32_causal(const float* q, const float* k, const float* v, float* out, int32_t b, int32_t h, int32_t kvh, int32_t head_dim,
                                        int32_t s, sat_stream_t stream) {
    return sat_launch_attention_f32_causal(q, k, v, out, b, h, kvh, head_dim, s, (hipStream_t)stream);
}

// ---- neighbourhood self-attention alone (sat_dit_plan_set_neighborhood_attention): the two launchers Forward calls.  score_scale multiplies
// q . k and nothing else does; the kernel works in the log2 domain, so the 16-bit launcher gets score_scale * log2(e)
extern "C" int sat_attention_window_bf16(const void* q, const void* k, const void* vt, void* out, int32_t b, int32_t h, int32_t kvh, int32_t s,
                                         int32_t s_pad_q, int32_t s_pad_k, int32_t kernel_size, float score_scale, sat_stream_t stream) {
    return sat_launch_attention_window((const op_t*)q, (const op_t*)k, (const op_t*)vt, (op_t*)out, b, h, kvh, s, s_pad_q, s_pad_k, kernel_size,
                                       score_scale * 1.4426950408889634f, (hipStream_t)stream, 0);
}
extern "C" int sat_attention_window_f16(const void* q, const void* k, const void* vt, void* out, int32_t b, int32_t h, int32_t kvh, int32_t s,
                                        int32_t s_pad_q, int32_t s_pad_k, int32_t kernel_size, float score_scale, sat_stream_t stream) {
    return sat_launch_attention_window((const op_t*)q, (const op_t*)k, (const op_t*)vt, (op_t*)out, b, h, kvh, s, s_pad_q, s_pad_k, kernel_size,
                                       score_scale * 1.4426950408889634f, (hipStream_t)stream, 1);
}
extern "C" int sat_attention_f32_window(const float* q, const float* k, const float* v, float* out, int32_t b, int32_t h, int32_t kvh, int32_t s,
                                        int32_t kernel_size, float score_scale, sat_stream_t stream) {
    return sat_launch_attention_f32_window(q, k, v, out, b, h, kvh, s, kernel_size, score_scale, (hipStream_t)stream);
}
// the same at 32-, 96- and 128-channel heads (sat_dit_plan_set_neighborhood_attention_hdw): q arrives in the log2 domain, there is no scale
extern "C" int sat_attention_hdw_window_bf16(const void* q, const void* k, const void* vt, void* out, int32_t b, int32_t h, int32_t kvh,
                                             int32_t head_dim, int32_t s, int32_t s_pad_q, int32_t s_pad_k, int32_t kernel_size, sat_stream_t stream) {
    return sat_launch_attention_hdw_window((const op_t*)q, (const op_t*)k, (const op_t*)vt, (op_t*)out, b, h, kvh, head_dim, s, s_pad_q, s_pad_k,
                                           kernel_size, (hipStream_t)stream, 0);
}
extern "C" int sat_attention_hdw_window_f16(const void* q, const void* k, const void* vt, void* out, int32_t b, int32_t h, int32_t kvh,
                                            int32_t head_dim, int32_t s, int32_t s_pad_q, int32_t s_pad_k, int32_t kernel_size, sat_stream_t stream) {
    return sat_launch_attention_hdw_window((const op_t*)q, (const op_t*)k, (const op_t*)vt, (op_t*)out, b, h, kvh, head_dim, s, s_pad_q, s_pad_k,
                                           kernel_size, (hipStream_t)stream, 1);
}
extern "C" int sat_attention_f32_window_w(const float* q, const float* k, const float* v, float* out, int32_t b, int32_t h, int32_t kvh,
                                          int32_t head_dim, int32_t s, int32_t kernel_size, float score_scale, sat_stream_t stream) {
    return sat_launch_attention_f32_window_w(q, k, v, out, b, h, kvh, head_dim, s, kernel_size, score_scale, (hipStream_t)stream);
}

// qkn: q and k L2-normalised per head (qk_norm), q pre-scaled for the attention kernel as in the plan
static int qkv_rope_bf16_impl(int f16, const void* a, const void* w, const float* inv_freq, void* q, void* k, void* vt,
                                 float* rope_scratch, int32_t b, int32_t s_len, int32_t s_pad, int32_t d, int32_t variant,
                                 sat_stream_t stream, bool qkn = false) {
    SAT_CHECK_ARG(a && w && inv_freq && q && k && vt && rope_scratch, SAT_E_INVALID, "qkv_rope: null pointer");
    SAT_CHECK_ARG(d % 64 == 0 && s_pad >= s_len + 3 && s_pad % 128 == 0, SAT_E_INVALID, "qkv_rope: bad dims (s_pad >= s + 3, %% 128)");
    hipStream_t s = (hipStream_t)stream;
    const int H = d / 64;
    const size_t bytes = (size_t)b * H * s_pad * 64 * 2;
    SAT_HIP(hipMemsetAsync(q, 0, bytes, s));
    SAT_HIP(hipMemsetAsync(k, 0, bytes, s));
    SAT_HIP(hipMemsetAsync(vt, 0, bytes, s));
    float* cs = rope_scratch;
    float* sn = rope_scratch + (size_t)s_len * 16;
    SAT_TRY(sat_launch_rope_table(inv_freq, cs, sn, s_len, s));
    GemmArgs g{};
    g.f16 = f16;
    g.A = (const op_t*)a; g.W = (const op_t*)w; g.M = b * s_len; g.N = 3 * d; g.K = d; g.variant = variant;
    g.heads.out[0] = (op_t*)q; g.heads.out[1] = (op_t*)k; g.heads.out[2] = (op_t*)vt;
    g.heads.kind[0] = 2; g.heads.kind[1] = 2 | 4; g.heads.kind[2] = 1 | 4;
    if (qkn) { g.heads.kind[0] |= 8 | 16; g.heads.kind[1] |= 16; g.heads.qscale = SAT_ATTN_QSCALE; }
    g.heads.parts = 3; g.heads.heads = H; g.heads.S = s_len; g.heads.Spad = s_pad;
    g.heads.rope_cos = cs; g.heads.rope_sin = sn;
    return sat_launch_gemm(EPI_HEADS, g, s);
}
extern "C" int sat_qkv_rope_qknorm_bf16(const void* a, const void* w, const float* inv_freq, void* q, void* k, void* vt,
                                        float* rope_scratch, int32_t b, int32_t s_len, int32_t s_pad, int32_t d, int32_t variant,
                                        sat_stream_t stream) {
    return qkv_rope_bf16_impl(0, a, w, inv_freq, q, k, vt, rope_scratch, b, s_len, s_pad, d, variant, stream, true);
}
extern "C" int sat_qkv_rope_qknorm_f16(const void* a, const void* w, const float* inv_freq, void* q, void* k, void* vt,
                                       float* rope_scratch, int32_t b, int32_t s_len, int32_t s_pad, int32_t d, int32_t variant,
                                       sat_stream_t stream) {
    return qkv_rope_bf16_impl(1, a, w, inv_freq, q, k, vt, rope_scratch, b, s_len, s_pad, d, variant, stream, true);
}
extern "C" int sat_qkv_rope_bf16(const void* a, const void* w, const float* inv_freq, void* q, void* k, void* vt,
                                 float* rope_scratch, int32_t b, int32_t s_len, int32_t s_pad, int32_t d, int32_t variant,
                                 sat_stream_t stream) {
    return qkv_rope_bf16_impl(0, a, w, inv_freq, q, k, vt, rope_scratch, b, s_len, s_pad, d, variant, stream);
}
extern "C" int sat_qkv_rope_f16(const void* a, const void* w, const float* inv_freq, void* q, void* k, void* vt,
                                 float* rope_scratch, int32_t b, int32_t s_len, int32_t s_pad, int32_t d, int32_t variant,
                                 sat_stream_t stream) {
    return qkv_rope_bf16_impl(1, a, w, inv_freq, q, k, vt, rope_scratch, b, s_len, s_pad, d, variant, stream);
}

// ---- LayerNorm folded into the neighbouring GEMMs (sat_dit_cfg.ln_fold), one entry per role
static int gemm_resid_ln_bf16_impl(int f16, const void* a, const void* w, const float* bias, float* c, void* xb, float* ln_part, int32_t m,
                                   int32_t n, int32_t k, int32_t variant, void* ws, size_t ws_bytes, sat_stream_t stream) {
    SAT_CHECK_ARG(c && xb && ln_part, SAT_E_INVALID, "gemm_resid_ln: null output");
    GemmArgs g{};
    g.f16 = f16;
    g.A = (const op_t*)a; g.W = (const op_t*)w; g.bias = bias; g.M = m; g.N = n; g.K = k;
    g.C = c; g.ldc = n; g.accumulate = 1; g.variant = variant; g.xb = (op_t*)xb; g.ln_part_out = ln_part;
    g.slab = (float*)ws; g.slab_bytes = ws ? ws_bytes : 0;
    return sat_launch_gemm(EPI_RESID, g, (hipStream_t)stream);
}
extern "C" int sat_gemm_resid_ln_bf16(const void* a, const void* w, const float* bias, float* c, void* xb, float* ln_part, int32_t m,
                                      int32_t n, int32_t k, int32_t variant, sat_stream_t stream) {
    return gemm_resid_ln_bf16_impl(0, a, w, bias, c, xb, ln_part, m, n, k, variant, nullptr, 0, stream);
}
extern "C" int sat_gemm_resid_ln_f16(const void* a, const void* w, const float* bias, float* c, void* xb, float* ln_part, int32_t m,
                                     int32_t n, int32_t k, int32_t variant, sat_stream_t stream) {
    return gemm_resid_ln_bf16_impl(1, a, w, bias, c, xb, ln_part, m, n, k, variant, nullptr, 0, stream);
}
extern "C" int sat_gemm_resid_ln_bf16_ws(const void* a, const void* w, const float* bias, float* c, void* xb, float* ln_part, int32_t m,
                                         int32_t n, int32_t k, int32_t variant, void* ws, size_t ws_bytes, sat_stream_t stream) {
    return gemm_resid_ln_bf16_impl(0, a, w, bias, c, xb, ln_part, m, n, k, variant, ws, ws_bytes, stream);
}
extern "C" int sat_gemm_resid_ln_f16_ws(const void* a, const void* w, const float* bias, float* c, void* xb, float* ln_part, int32_t m,
                                        int32_t n, int32_t k, int32_t variant, void* ws, size_t ws_bytes, sat_stream_t stream) {
    return gemm_resid_ln_bf16_impl(1, a, w, bias, c, xb, ln_part, m, n, k, variant, ws, ws_bytes, stream);
}

static int gemm_swiglu_ln_bf16_impl(int f16, const void* xb, const float* ln_part, const float* w_f32, const float* gamma, const float* beta,
                                       const float* bias_f32, void* wpack, float* c12, void* h, int32_t m, int32_t n, int32_t k,
                                       int32_t variant, sat_stream_t stream) {
    SAT_CHECK_ARG(xb && ln_part && w_f32 && gamma && beta && wpack && c12 && h, SAT_E_INVALID, "gemm_swiglu_ln: null pointer");
    hipStream_t s = (hipStream_t)stream;
    if (!sat_variant_has(variant, SAT_VARIANT_PACKED))       // wpack / c12 already hold the packed operands of a previous call (benchmarks)
        SAT_TRY(sat_launch_pack_rows_ln(w_f32, gamma, beta, bias_f32, (op_t*)wpack, c12, c12 + n, n, k, 1, s, f16));
    GemmArgs g{};
    g.f16 = f16;
    g.A = (const op_t*)xb; g.W = (const op_t*)wpack; g.M = m; g.N = n; g.K = k; g.H = (op_t*)h; g.variant = variant & ~SAT_VARIANT_PACKED;
    g.ln_part = ln_part; g.ln_c1 = c12; g.ln_c2 = c12 + n; g.ln_eps = 1e-5f;
    return sat_launch_gemm(EPI_SWIGLU, g, s);
}
extern "C" int sat_gemm_swiglu_ln_bf16(const void* xb, const float* ln_part, const float* w_f32, const float* gamma, const float* beta,
                                       const float* bias_f32, void* wpack, float* c12, void* h, int32_t m, int32_t n, int32_t k,
                                       int32_t variant, sat_stream_t stream) {
    return gemm_swiglu_ln_bf16_impl(0, xb, ln_part, w_f32, gamma, beta, bias_f32, wpack, c12, h, m, n, k, variant, stream);
}
extern "C" int sat_gemm_swiglu_ln_f16(const void* xb, const float* ln_part, const float* w_f32, const float* gamma, const float* beta,
                                       const float* bias_f32, void* wpack, float* c12, void* h, int32_t m, int32_t n, int32_t k,
                                       int32_t variant, sat_stream_t stream) {
    return gemm_swiglu_ln_bf16_impl(1, xb, ln_part, w_f32, gamma, beta, bias_f32, wpack, c12, h, m, n, k, variant, stream);
}

static int qkv_rope_ln_bf16_impl(int f16, const void* xb, const float* ln_part, const float* w_f32, const float* gamma, const float* beta,
                                    void* wpack, float* c12, const float* inv_freq, void* q, void* k, void* vt, float* rope_scratch,
                                    int32_t b, int32_t s_len, int32_t s_pad, int32_t d, int32_t variant, sat_stream_t stream) {
    SAT_CHECK_ARG(xb && ln_part && w_f32 && gamma && beta && wpack && c12 && inv_freq && q && k && vt && rope_scratch, SAT_E_INVALID,
                  "qkv_rope_ln: null pointer");
    SAT_CHECK_ARG(d % 64 == 0 && s_pad >= s_len + 3 && s_pad % 128 == 0, SAT_E_INVALID, "qkv_rope_ln: bad dims (s_pad >= s + 3, %% 128)");
    hipStream_t s = (hipStream_t)stream;
    const int H = d / 64;
    const size_t bytes = (size_t)b * H * s_pad * 64 * 2;
    float* cs = rope_scratch;
    float* sn = rope_scratch + (size_t)s_len * 16;
    if (!sat_variant_has(variant, SAT_VARIANT_PACKED)) {     // pads, tables and packed operands are those of a previous call (benchmarks)
        SAT_HIP(hipMemsetAsync(q, 0, bytes, s));
        SAT_HIP(hipMemsetAsync(k, 0, bytes, s));
        SAT_HIP(hipMemsetAsync(vt, 0, bytes, s));
        SAT_TRY(sat_launch_rope_table(inv_freq, cs, sn, s_len, s));
        SAT_TRY(sat_launch_pack_rows_ln(w_f32, gamma, beta, nullptr, (op_t*)wpack, c12, c12 + 3 * d, 3 * d, d, 0, s, f16));
    }
    GemmArgs g{};
    g.f16 = f16;
    g.A = (const op_t*)xb; g.W = (const op_t*)wpack; g.M = b * s_len; g.N = 3 * d; g.K = d; g.variant = variant & ~SAT_VARIANT_PACKED;
    g.heads.out[0] = (op_t*)q; g.heads.out[1] = (op_t*)k; g.heads.out[2] = (op_t*)vt;
    g.heads.kind[0] = 2; g.heads.kind[1] = 2 | 4; g.heads.kind[2] = 1 | 4;
    g.heads.parts = 3; g.heads.heads = H; g.heads.S = s_len; g.heads.Spad = s_pad;
    g.heads.rope_cos = cs; g.heads.rope_sin = sn;
    g.ln_part = ln_part; g.ln_c1 = c12; g.ln_c2 = c12 + 3 * d; g.ln_eps = 1e-5f;
    return sat_launch_gemm(EPI_HEADS, g, s);
}
extern "C" int sat_qkv_rope_ln_bf16(const void* xb, const float* ln_part, const float* w_f32, const float* gamma, const float* beta,
                                    void* wpack, float* c12, const float* inv_freq, void* q, void* k, void* vt, float* rope_scratch,
                                    int32_t b, int32_t s_len, int32_t s_pad, int32_t d, int32_t variant, sat_stream_t stream) {
    return qkv_rope_ln_bf16_impl(0, xb, ln_part, w_f32, gamma, beta, wpack, c12, inv_freq, q, k, vt, rope_scratch, b, s_len, s_pad, d, variant, stream);
}
extern "C" int sat_qkv_rope_ln_f16(const void* xb, const float* ln_part, const float* w_f32, const float* gamma, const float* beta,
                                    void* wpack, float* c12, const float* inv_freq, void* q, void* k, void* vt, float* rope_scratch,
                                    int32_t b, int32_t s_len, int32_t s_pad, int32_t d, int32_t variant, sat_stream_t stream) {
    return qkv_rope_ln_bf16_impl(1, xb, ln_part, w_f32, gamma, beta, wpack, c12, inv_freq, q, k, vt, rope_scratch, b, s_len, s_pad, d, variant, stream);
}

extern "C" int sat_quant_rows_fp8(const float* x, void* out8, float* row_scale, int32_t rows, int32_t k, sat_stream_t stream) {
    return sat_launch_quant_rows_fp8(x, out8, row_scale, rows, k, 0, (hipStream_t)stream);
}

extern "C" int sat_layernorm_fp8(const float* x, const float* gamma, const float* beta, void* y8, float* row_scale, int32_t m,
                                 int32_t d, sat_stream_t stream) {
    return sat_launch_layernorm_fp8(x, gamma, beta, y8, row_scale, m, d, nullptr, nullptr, 1, 0, (hipStream_t)stream);
}

extern "C" int sat_gemm_fp8_f32(const void* a8, const float* a_scale, const void* w8, const float* w_scale, const float* bias,
                                float* c, int32_t m, int32_t n, int32_t k, int32_t accumulate, int32_t variant, sat_stream_t stream) {
    SAT_CHECK_ARG(a8 && w8 && a_scale && w_scale && c, SAT_E_INVALID, "gemm_fp8: null pointer");
    GemmArgs g{};
    g.A = (const op_t*)a8; g.W = (const op_t*)w8; g.bias = bias; g.M = m; g.N = n; g.K = k; g.variant = variant & ~SAT_VARIANT_FP8_PLAIN;
    g.C = c; g.ldc = n; g.accumulate = accumulate; g.a_scale = a_scale; g.w_scale = w_scale;
    g.fp8 = sat_variant_has(variant, SAT_VARIANT_FP8_PLAIN) ? 1 : 2;      // the plain 32x32x16 fp8 MFMA instead of the 2x-rate scaled 32x32x64
    return sat_launch_gemm(EPI_F32, g, (hipStream_t)stream);
}

extern "C" int sat_quant_mx_rows_fp8(const float* x, void* out8, void* scales, int32_t rows, int32_t k, sat_stream_t stream) {
    return sat_launch_quant_mx_rows(x, out8, scales, rows, k, (hipStream_t)stream);
}

extern "C" int sat_gemm_mxfp8_f32(const void* a8, const void* a_scales, const void* w8, const float* w_scale, const float* bias,
                                  float* c, int32_t m, int32_t n, int32_t k, int32_t accumulate, int32_t variant, sat_stream_t stream) {
    SAT_CHECK_ARG(a8 && w8 && a_scales && w_scale && c, SAT_E_INVALID, "gemm_mxfp8: null pointer");
    SAT_CHECK_ARG(((uintptr_t)a_scales & 3) == 0, SAT_E_INVALID, "gemm_mxfp8: the scale array must be 4-byte aligned");
    GemmArgs g{};
    g.A = (const op_t*)a8; g.W = (const op_t*)w8; g.bias = bias; g.M = m; g.N = n; g.K = k; g.variant = sat_variant_tile(variant);
    g.C = c; g.ldc = n; g.accumulate = accumulate; g.a_bscale = (const unsigned*)a_scales; g.w_scale = w_scale; g.fp8 = 3;
    return sat_launch_gemm(EPI_F32, g, (hipStream_t)stream);
}

// the kernels of sat_dit_plan_set_block_options alone
extern "C" int sat_dwconv_ln_silu_bf16(const void* x, const float* w, const float* gamma, const float* beta, void* y, int32_t b, int32_t s_len,
                                       int32_t d, int32_t variant, sat_stream_t stream) {
    return sat_launch_dwconv_ln_silu_variant(x, w, gamma, beta, y, b, s_len, d, SAT_GEMM_BF16, variant, (hipStream_t)stream);
}
extern "C" int sat_dwconv_ln_silu_f16(const void* x, const float* w, const float* gamma, const float* beta, void* y, int32_t b, int32_t s_len,
                                      int32_t d, int32_t variant, sat_stream_t stream) {
    return sat_launch_dwconv_ln_silu_variant(x, w, gamma, beta, y, b, s_len, d, SAT_GEMM_FP16, variant, (hipStream_t)stream);
}
static int gemm_act_impl(int f16, const void* a, const void* w, const float* bias, void* h, int32_t m, int32_t n, int32_t k, int32_t act,
                         int32_t variant, sat_stream_t stream) {
    SAT_CHECK_ARG(h, SAT_E_INVALID, "gemm_act: null output");
    GemmArgs g{};
    g.f16 = f16;
    g.A = (const op_t*)a; g.W = (const op_t*)w; g.bias = bias; g.M = m; g.N = n; g.K = k;
    g.H = (op_t*)h; g.act = act; g.variant = variant;
    return sat_launch_gemm(EPI_ACT16, g, (hipStream_t)stream);
}
extern "C" int sat_gemm_act_bf16(const void* a, const void* w, const float* bias, void* h, int32_t m, int32_t n, int32_t k, int32_t act,
                                 int32_t variant, sat_stream_t stream) {
    return gemm_act_impl(0, a, w, bias, h, m, n, k, act, variant, stream);
}
extern "C" int sat_gemm_act_f16(const void* a, const void* w, const float* bias, void* h, int32_t m, int32_t n, int32_t k, int32_t act,
                                int32_t variant, sat_stream_t stream) {
    return gemm_act_impl(1, a, w, bias, h, m, n, k, act, variant, stream);
}

// ---- the convolution GEMM of sat_dit_plan_set_ff_conv alone: the plan's packing launch, then the launches of Forward::feed_forward_conv (16-bit)
// or of Forward::block_f32 (row gather + sat_gemm_f32)
static size_t ff_conv_pack_bytes(int32_t format, int32_t n, int32_t k, int32_t taps) {
    return (size_t)round_up((int64_t)n * k * taps * (format == SAT_GEMM_FP32X ? 4 : 2), 256);
}
extern "C" int sat_ff_conv_workspace_bytes(int32_t format, int32_t b, int32_t s_len, int32_t n, int32_t k, int32_t kernel_size, size_t* out_bytes) {
    SAT_CHECK_ARG(out_bytes && b > 0 && s_len > 0 && n > 0 && k > 0 && kernel_size > 0, SAT_E_INVALID, "ff_conv_workspace_bytes: bad argument");
    SAT_CHECK_ARG(format == SAT_GEMM_BF16 || format == SAT_GEMM_FP16 || format == SAT_GEMM_FP32X, SAT_E_INVALID, "ff_conv_workspace_bytes: format %d", format);
    *out_bytes = ff_conv_pack_bytes(format, n, k, kernel_size) + (format == SAT_GEMM_FP32X ? (size_t)b * s_len * kernel_size * k * 4 : 0);
    return 0;
}
extern "C" int sat_ff_conv(int32_t format, const void* a, const float* w, const float* bias, int32_t epilogue, void* out, const float* gate, int32_t b,
                           int32_t s_len, int32_t n, int32_t k, int32_t kernel_size, void* ws, size_t ws_bytes, sat_stream_t stream) {
    SAT_CHECK_ARG(a && out && ws && b > 0 && s_len > 0 && (int64_t)b * s_len <= (1 << 30), SAT_E_INVALID, "ff_conv: bad argument");
    SAT_CHECK_ARG(epilogue == FFC_RESID || (epilogue == FFC_ACT16 && !gate), SAT_E_INVALID, "ff_conv: epilogue %d (0 residual, 1 SiLU without a gate)", epilogue);
    SAT_CHECK_ARG(kernel_size >= 1 && kernel_size <= 7 && (kernel_size & 1), SAT_E_UNSUPPORTED, "ff_conv: kernel size %d (odd, 1 to 7)", kernel_size);
    SAT_CHECK_ARG(k > 0 && k % 64 == 0 && n > 0 && n % 128 == 0, SAT_E_UNSUPPORTED, "ff_conv: k = %d must be a multiple of 64 and n = %d of 128", k, n);
    size_t need = 0;
    SAT_TRY(sat_ff_conv_workspace_bytes(format, b, s_len, n, k, kernel_size, &need));
    SAT_CHECK_ARG(ws_bytes >= need && ((uintptr_t)ws & 255) == 0, SAT_E_WORKSPACE, "ff_conv: workspace of %zu bytes (256-byte aligned), need %zu", ws_bytes, need);
    hipStream_t s = (hipStream_t)stream;
    if (w) SAT_TRY(sat_launch_pack_conv_taps(w, ws, n, k, kernel_size, format, s));      // (null: the image an earlier call left in ws)
    const int M = b * s_len;
    if (format == SAT_GEMM_FP32X) {
        float* col = (float*)((char*)ws + ff_conv_pack_bytes(format, n, k, kernel_size));
        SAT_TRY(sat_launch_im2col_rows_f32((const float*)a, col, b, s_len, k, kernel_size, s));
        SAT_TRY(sat_launch_gemm_f32(col, (const float*)ws, bias, (float*)out, M, n, kernel_size * k, n, epilogue == FFC_RESID, gate, s_len, n, s));
        return epilogue == FFC_ACT16 ? sat_launch_silu_f32((float*)out, (int64_t)M * n, s) : 0;
    }
    FfConvArgs g{};
    g.fmt = format; g.A = a; g.W = ws; g.bias = bias; g.B = b; g.S = s_len; g.N = n; g.K = k; g.taps = kernel_size; g.epi = epilogue;
    if (epilogue == FFC_RESID) { g.C = (float*)out; g.ldc = n; g.accumulate = 1; g.gate = gate; g.gate_rows = s_len; g.gate_ld = n; }
    else { g.H = out; g.act = 1; }
    return sat_launch_ff_conv(g, s);
}

// ---- the two boundary kernels of sat_dit_plan_set_patch alone (dit_patch.hip): the launchers Forward's run_forward calls, on folded weights
// of sat_fold_in_patch / sat_fold_out_patch, which are the launches of the plan's finalize
extern "C" int sat_fold_in_patch(const float* w_in, const float* w_pre, float* w_eff_t, int32_t d, int32_t ci, int32_t patch_size, sat_stream_t stream) {
    return glue_fold_in_patch(w_in, w_pre, w_eff_t, d, ci, patch_size, (hipStream_t)stream);
}
extern "C" int sat_fold_out_patch(const float* w_out, const float* w_post, float* w_eff_t, int32_t d, int32_t c, int32_t patch_size, sat_stream_t stream) {
    return glue_fold_out_patch(w_out, w_post, w_eff_t, d, c, patch_size, (hipStream_t)stream);
}
extern "C" int sat_input_proj_patch(const float* x, const float* w_eff_t, float* X, int32_t bf, int32_t xb, int32_t c, int32_t patch_size, int32_t t,
                                    int32_t s_len, int32_t d, float xscale, const float* concat, int32_t cc, int32_t tc, const float* prep, int32_t p,
                                    sat_stream_t stream) {
    return glue_input_proj_patch(x, w_eff_t, X, bf, xb, c, patch_size, t, s_len, d, xscale, concat, cc, tc, prep, p, (hipStream_t)stream);
}
extern "C" int sat_output_proj_patch(const float* X, const float* w_eff_t, float* out, int32_t bf, int32_t c, int32_t patch_size, int32_t t, int32_t s_len,
                                     int32_t d, sat_stream_t stream) {
    return glue_output_proj_patch(X, w_eff_t, out, bf, c, patch_size, t, s_len, d, (hipStream_t)stream);
}

// ---- the two projections at the audio boundary of the local-attention codec alone (local_attn_io.hip): the launchers sat_local_attn_forward calls
extern "C" int sat_local_attn_project_in(const float* x, const float* w, float* rows, int32_t b, int32_t c_in, int32_t t, int32_t d, sat_stream_t stream) {
    return sat_launch_local_attn_project_in(x, w, rows, b, c_in, t, d, (hipStream_t)stream);
}
extern "C" int sat_local_attn_project_out(const float* rows, const float* w, float* out, int32_t b, int32_t c_out, int32_t t, int32_t d,
                                          sat_stream_t stream) {
    return sat_launch_local_attn_project_out(rows, w, out, b, c_out, t, d, (hipStream_t)stream);
}

// ---- the Dance Diffusion U-Net's own kernels alone (unet_kernels.hip): the launchers sat_unet_forward calls
extern "C" int sat_unet_groupnorm_partials(int64_t n) { return n > 0 ? sat_unet_gn_tiles(n) : 0; }
extern "C" int sat_unet_groupnorm_stats(const float* x, float* part, float* stats, int32_t b, int64_t n, float eps, sat_stream_t stream) {
    return sat_launch_unet_gn_stats(x, part, stats, b, n, eps, (hipStream_t)stream);
}
extern "C" int sat_unet_groupnorm_apply(const float* x, const float* stats, const float* gamma, const float* beta, const float* skip, float* out32, void* out_op,
                                        int32_t b, int32_t rows, int32_t c, int32_t ld, int32_t act, int32_t fmt, sat_stream_t stream) {
    return sat_launch_unet_gn_apply(x, stats, gamma, beta, skip, out32, out_op, b, rows, c, ld, act, fmt, (hipStream_t)stream);
}
extern "C" int sat_unet_cast_rows(const float* x, void* out_op, int64_t m, int32_t c, int32_t ld, int32_t fmt, sat_stream_t stream) {
    return sat_launch_unet_cast_rows(x, out_op, m, c, ld, fmt, (hipStream_t)stream);
}
extern "C" int sat_unet_downsample(const float* x, float* out32, void* out_op, int32_t b, int32_t s_len, int32_t c, int32_t fmt, sat_stream_t stream) {
    return sat_launch_unet_downsample(x, out32, out_op, b, s_len, c, fmt, (hipStream_t)stream);
}
extern "C" int sat_unet_upsample(const float* x, void* out_op, int32_t b, int32_t s_len, int32_t c, int32_t ld, int32_t fmt, sat_stream_t stream) {
    return sat_launch_unet_upsample(x, out_op, b, s_len, c, ld, fmt, (hipStream_t)stream);
}
extern "C" int sat_unet_input(const float* x, const float* t_in, float in_scale, const float* w_embed, const float* w_main, const float* b_main,
                              const float* w_skip, float* y, float* sk, int32_t b, int32_t io, int32_t t, int32_t c, int32_t taps, sat_stream_t stream) {
    return sat_launch_unet_input(x, t_in, in_scale, w_embed, w_main, b_main, w_skip, y, sk, b, io, t, c, taps, (hipStream_t)stream);
}
extern "C" int sat_unet_output(const float* h, const float* xin, const float* w_main, const float* b_main, const float* w_skip, float* out, int32_t b,
                               int32_t io, int32_t t, int32_t c, int32_t taps, sat_stream_t stream) {
    return sat_launch_unet_output(h, xin, w_main, b_main, w_skip, out, b, io, t, c, taps, (hipStream_t)stream);
}
