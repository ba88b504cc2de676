// Neighbourhood self-attention for the DiT (attn_kwargs natten_kernel_size = K; models/transformer.py:479-493 of the reference): query i of a
// sequence of S >= K rows attends to the K keys start(i) .. start(i) + K - 1, start(i) = min(max(i - K / 2, 0), S - K) (attn_window.h has the
// ranges), softmax in fp32, 64-channel heads.  The score scale is the launcher's argument: the reference hands q to natten1dqk unscaled.
//
// The 16-bit kernel is the one-group layout of attention.hip -- 8 waves = 256 queries of one (batch, head), K / V^T tiles of 64 keys copied by
// LDS-DMA into a 3-stage ring shared by all waves (attn::walk3), both products transposed -- built from the pieces of attn_core.h: the
// per-wave step attn::tile with MASK_WINDOW, the ring walk, the output store.  What is the kernel's own:
//   * the workgroup copies and walks only the tiles [first_tile, last_tile] that hold the union of its queries' windows;
//   * inside a tile the step classes each 32-key block against the windows of the WAVE's 32 queries: SKIP (no MFMA, no softmax; the wave
//     still copies its pieces and joins every barrier), FULL (no compare) or EDGE (each lane masks the keys outside its own [k_lo, k_hi));
//   * a wave's first visible block is not its first tile, and the lanes of a wave meet their first key in different blocks: attn_core.h
//     says why the standing reference of -1e30 carries (m, l, O) = (-1e30, 0, 0) unharmed until a lane's window begins.
// The fp32 kernel (the fp32 verification mode) is one query per lane as in f32_ref.hip, over the keys of the wave's union.
#include "attn_core.h"
#include "attn_window.h"
#include "sat_common.h"

namespace {

constexpr int KV_TILE = attn::KV_TILE;
constexpr int QB = 256;                                   // queries per workgroup
constexpr int STAGE_BYTES = 2 * KV_TILE * 128;            // K tile + V^T tile
constexpr int WIN_LDS = 3 * STAGE_BYTES;                  // 48 KiB

// q [B,H,S_pad_q,64], k [B,KVH,Sk_pad,64] (rows shifted by ob), vt [B,KVH,64,Sk_pad] (vt_pos order) -> out [B*S, H*64]
__global__ __launch_bounds__(512, 2) void attention_window_kernel(const op_t* __restrict__ q, const op_t* __restrict__ k, const op_t* __restrict__ vt,
                                                                  op_t* __restrict__ out, int H, int KVH, int S, int Sq_pad, int Sk_pad, int KS,
                                                                  float scale_log2) {
    sat_f16_saturate();
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wq = __builtin_amdgcn_readfirstlane(tid >> 6);      // query sub-block of this wave
    const int half = lane >> 5;
    const int l31 = lane & 31;
    // XCD-aware placement as in attention.hip: consecutive logical ids (query blocks of one (batch, head)) share an XCD
    const int lin = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
    const int lid = xcd_remap(lin, gridDim.x * gridDim.y * gridDim.z);
    const int bx = lid % gridDim.x;
    const int h = (lid / gridDim.x) % gridDim.y, b = lid / (gridDim.x * gridDim.y);
    const int kvh = h / (H / KVH);
    const int qi = bx * QB + wq * 32 + l31;                // the last workgroup may reach beyond Sq_pad

    opx8 qf[4];
    {
        const op_t* qp = q + ((size_t)(b * H + h) * Sq_pad + (qi < Sq_pad ? qi : Sq_pad - 1)) * 64 + half * 8;
#pragma unroll
        for (int t = 0; t < 4; ++t) qf[t] = *reinterpret_cast<const opx8*>(qp + t * 16);
    }

    // K rows / V^T columns of sequence b start at ob = (b*S) & 3 (see EPI_HEADS in gemm_bf16.hip)
    const int ob = (b * S) & 3;
    const int t_first = attnw::first_tile(bx * QB, ob, KS, S, KV_TILE);                       // bx * QB < S: the grid is cdiv(S, QB) wide
    const int t_count = attnw::last_tile(bx * QB, QB, ob, KS, S, KV_TILE) - t_first + 1;      // >= 1; the last tile ends at or below Sk_pad

    // LDS-DMA pieces of this wave: piece wq (8 rows of 128 B) of the K tile and of the V^T tile, swizzle folded into the source address
    const op_t* ksrc;
    const op_t* vsrc;
    {
        const int row = wq * 8 + (lane >> 3);
        const int c = (lane & 7) ^ ((row >> 1) & 7);
        ksrc = k + (size_t)(b * KVH + kvh) * Sk_pad * 64 + (size_t)row * 64 + c * 8;          // + tile * 64 rows
        vsrc = vt + (size_t)(b * KVH + kvh) * 64 * Sk_pad + (size_t)row * Sk_pad + c * 8;     // + tile * 64 keys
    }
    auto stage_in = [&](int tile, int stage) {
        char* sk = smem + stage * STAGE_BYTES;
        char* sv = sk + KV_TILE * 128;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(ksrc + (size_t)tile * KV_TILE * 64),
                                         (__attribute__((address_space(3))) void*)(sk + wq * 1024), 16, 0, 0);
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(vsrc + (size_t)tile * KV_TILE),
                                         (__attribute__((address_space(3))) void*)(sv + wq * 1024), 16, 0, 0);
    };

    attn::State<1> st;
    st.init(half);

    // a wave whose 32 queries are all beyond S still copies tiles and joins the barriers, but skips the matrix and softmax work
    const int wq_first = __builtin_amdgcn_readfirstlane(bx * QB + wq * 32);
    const bool wave_active = wq_first < S;
    const attnw::Range wr = attnw::wave_range(wave_active ? wq_first : S - 1, 32, ob, KS, S);
    const int k_lo = attnw::key_lo(qi, ob, KS, S), k_hi = k_lo + KS;

    attn::walk3<2>(t_first, t_count, stage_in, [&](int tile, int stage) {
        if (!wave_active) return;
        const char* sk = smem + stage * STAGE_BYTES;
        attn::tile<1, 0, attn::MASK_WINDOW>(st, qf, sk, sk + KV_TILE * 128, false, tile * KV_TILE, k_lo, k_hi, false, scale_log2, l31, half, 0, 0, wr);
    });

    op_t* op = out + ((size_t)b * S + qi) * ((size_t)H * 64) + h * 64 + 8 * half;
    attn::store_out(st.oacc, 1.0f / attn::half_sum(st.l_run), op, qi < S);
}

#ifndef SAT_OPERAND_F16
// fp32: one query per lane, K / V rows are wave-uniform loads, online softmax over chunks of 8 keys from the first key of the wave's union to
// its last; a lane masks the keys outside its own window.  The running maximum starts at -1e30, not -inf: a chunk that shows a lane no key
// leaves (m, l, o) as they are (exp(-1e30 + 1e30) = 1, exp(-inf + 1e30) = 0).  q [B,H,S,64], k / v [B,KVH,S,64] -> out [B*S, H*64]
__global__ __launch_bounds__(64) void attention_window_f32_kernel(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                                                                  float* __restrict__ out, int H, int KVH, int S, int KS, float scale) {
    constexpr int W = 64;
    const int b = blockIdx.z, h = blockIdx.y;
    const int kvh = h / (H / KVH);
    const int qi = blockIdx.x * 64 + threadIdx.x;
    const int qc = qi < S ? qi : S - 1;
    float qr[W], o[W];
    const f32x4* qp = reinterpret_cast<const f32x4*>(q + (((size_t)b * H + h) * S + qc) * W);
#pragma unroll
    for (int t = 0; t < W / 4; ++t) {
        const f32x4 x = qp[t];
        qr[4 * t] = x[0] * scale;
        qr[4 * t + 1] = x[1] * scale;
        qr[4 * t + 2] = x[2] * scale;
        qr[4 * t + 3] = x[3] * scale;
    }
#pragma unroll
    for (int d = 0; d < W; ++d) o[d] = 0.f;
    float m_run = -1e30f, l_run = 0.f;
    const float* kb = k + ((size_t)b * KVH + kvh) * S * W;
    const float* vb = v + ((size_t)b * KVH + kvh) * S * W;
    const int j_lo = attnw::union_lo(blockIdx.x * 64, 0, KS, S), j_hi = attnw::union_hi(blockIdx.x * 64, 64, 0, KS, S);      // <= S
    const int lo = attnw::key_lo(qc, 0, KS, S), hi = lo + KS;
    for (int j0 = j_lo; j0 < j_hi; j0 += 8) {
        float sc[8];
        float mx = m_run;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int j = j0 + u;
            float s = -INFINITY;
            if (j < j_hi) {
                const float* kr = kb + (size_t)j * W;
                s = 0.f;
#pragma unroll
                for (int d = 0; d < W; ++d) s = fmaf(qr[d], kr[d], s);
                if (j < lo || j >= hi) s = -INFINITY;
            }
            sc[u] = s;
            mx = fmaxf(mx, s);
        }
        const float alpha = expf(m_run - mx);
        m_run = mx;
        l_run *= alpha;
#pragma unroll
        for (int d = 0; d < W; ++d) o[d] *= alpha;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int j = j0 + u;
            if (j < j_hi) {
                const float p = expf(sc[u] - mx);
                l_run += p;
                const float* vr = vb + (size_t)j * W;
#pragma unroll
                for (int d = 0; d < W; ++d) o[d] = fmaf(p, vr[d], o[d]);
            }
        }
    }
    if (qi < S) {
        const float inv = 1.0f / l_run;
        f32x4* op = reinterpret_cast<f32x4*>(out + ((size_t)b * S + qi) * ((size_t)H * W) + h * W);
#pragma unroll
        for (int t = 0; t < W / 4; ++t) op[t] = f32x4{o[4 * t] * inv, o[4 * t + 1] * inv, o[4 * t + 2] * inv, o[4 * t + 3] * inv};
    }
}
#endif

}  // namespace

// What NATTEN rejects: an even kernel size, one of 1 or less, a sequence shorter than the kernel
#define SAT_CHECK_WINDOW(what, ks, s_len)                                                                                              \
    SAT_CHECK_ARG((ks) > 1 && ((ks) & 1), SAT_E_INVALID, what ": kernel_size %d must be odd and greater than 1", (ks));                \
    SAT_CHECK_ARG((s_len) >= (ks), SAT_E_INVALID, what ": a sequence of %d rows is shorter than kernel_size %d", (s_len), (ks))

#ifdef SAT_OPERAND_F16
int sat_launch_attention_window_f16(const void* q, const void* k, const void* vt, void* out, int b, int h, int kvh, int s_len, int sq_pad, int sk_pad,
                                    int kernel_size, float score_scale, hipStream_t s) {
    return f16::sat_launch_attention_window((const op_t*)q, (const op_t*)k, (const op_t*)vt, (op_t*)out, b, h, kvh, s_len, sq_pad, sk_pad, kernel_size,
                                            score_scale, s, 1);
}
#endif

int SAT_OPNS::sat_launch_attention_window(const op_t* q, const op_t* k, const op_t* vt, op_t* out, int b, int h, int kvh, int s_len, int sq_pad,
                                          int sk_pad, int kernel_size, float score_scale, hipStream_t s, int f16) {
#ifndef SAT_OPERAND_F16
    if (f16) return sat_launch_attention_window_f16(q, k, vt, out, b, h, kvh, s_len, sq_pad, sk_pad, kernel_size, score_scale, s);
#else
    SAT_CHECK_ARG(f16, SAT_E_INVALID, "attention (window): the fp16 build takes fp16 tensors and writes fp16");
#endif
    SAT_CHECK_ATTENTION("attention (window)", "s", s_len, s_len, true, true);
    SAT_CHECK_WINDOW("attention (window)", kernel_size, s_len);
    SAT_CHECK_ARG(score_scale > 0.f && score_scale <= 1e6f, SAT_E_INVALID, "attention (window): score scale %g is not a positive finite number",
                  (double)score_scale);
    SAT_TRY(sat_ensure_dynamic_lds(reinterpret_cast<const void*>(attention_window_kernel), WIN_LDS));
    hipLaunchKernelGGL(attention_window_kernel, dim3(cdiv(s_len, QB), h, b), dim3(512), WIN_LDS, s, q, k, vt, out, h, kvh, s_len, sq_pad, sk_pad,
                       kernel_size, score_scale);
    SAT_LAUNCH_CHECK();
    return 0;
}

#ifndef SAT_OPERAND_F16
int sat_launch_attention_f32_window(const float* q, const float* k, const float* v, float* out, int b, int h, int kvh, int s_len, int kernel_size,
                                    float score_scale, hipStream_t s) {
    SAT_CHECK_ARG(q && k && v && out && b > 0 && h > 0 && kvh > 0 && h % kvh == 0 && s_len > 0, SAT_E_INVALID, "attention_f32 (window): bad args");
    SAT_CHECK_ARG((((uintptr_t)q | (uintptr_t)out) & 15) == 0, SAT_E_INVALID, "attention_f32 (window): q and out must be 16-byte aligned");
    SAT_CHECK_ARG(h <= 65535 && b <= 65535, SAT_E_UNSUPPORTED, "attention_f32 (window): %d heads / %d sequences exceed the grid", h, b);
    SAT_CHECK_WINDOW("attention_f32 (window)", kernel_size, s_len);
    SAT_CHECK_ARG(score_scale > 0.f && score_scale <= 1e6f, SAT_E_INVALID, "attention_f32 (window): score scale %g is not a positive finite number",
                  (double)score_scale);
    hipLaunchKernelGGL(attention_window_f32_kernel, dim3(cdiv(s_len, 64), h, b), dim3(64), 0, s, q, k, v, out, h, kvh, s_len, kernel_size, score_scale);
    SAT_LAUNCH_CHECK();
    return 0;
}
#endif
