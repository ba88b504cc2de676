// Neighbourhood self-attention for DiTs with 32-, 96- and 128-channel heads (attn_kwargs natten_kernel_size = K on the staged route of
// dit_plan.hip; models/transformer.py:479-493 of the reference): attention_window.hip at the widths of attention_hdw.hip.  Query i of a sequence
// of S >= K rows attends to the K keys start(i) .. start(i) + K - 1, start(i) = min(max(i - K / 2, 0), S - K) (attn_window.h), softmax in fp32.
//
// The 16-bit kernel attention_hdw_window_kernel<W> has the structure and the data conventions of attention_hdw_kernel<W, false>: 8 waves = 256
// queries of one (batch, head), attnw::Tiles<W> rings of three stages filled by LDS-DMA with the swizzles of attn_hdw_tiles.h folded into the
// source address, attn::walk3, XCD remap, attn::store_out.  Q arrives pre-scaled by the head split and there is no scale argument: the plan's
// qscale() is log2(e) alone for a neighbourhood plan, because the reference hands q to natten1dqk unscaled.  The ranges are those of
// attention_window_kernel: the workgroup copies and walks only the tiles first_tile .. last_tile at KT = Tiles<W>::KV_TILE (128 keys at W = 32,
// 64 at the other widths), and each wave classes every 32-key block with wave_range / block_class through attn::tile<1, 0, MASK_WINDOW,
// LayoutHdw<W>> with the lane's own [key_lo, key_hi).
//
// Two points that are new at these widths:
//  * W = 32: a tile holds FOUR blocks and a wave's union may begin in block 1-3 of its first tile and end in block 0-2 of its last, and for a
//    wave other than the workgroup's first or last the tile may hold no visible block at all; after a SKIP block of a tile a visible one can
//    follow (blocks 0-1 below the union, 2-3 inside).  MASK_WINDOW therefore `continue`s over SKIP blocks (attn_core.h), where MASK_CAUSAL and
//    the tail-pad test of MASK_NONE `break`.  tests/dit_natten_hdw_units.py has the mistake "dropped third block of a 128-key tile".
//  * W = 96: the hole lanes of a K piece fetch chunk 0 of THEIR OWN row, tile * KT + row with row < KT, and the spare V^T rows 96..127 fetch the
//    channel rows 64..95 at the keys tile * KT + 8 chunk .. + 8 of their own tile: both addresses lie inside the walked tile, whichever tile that
//    is.  Every walked tile lies inside the buffers: first_tile >= 0 and union_hi <= ob + S <= Sk_pad with Sk_pad % KT == 0 (the launcher
//    checks Sk_pad >= S + 3 and the multiple), so (last_tile + 1) * KT <= Sk_pad -- also when the first walked tile is not tile 0 and the last
//    is not the sequence's last.
//
// The fp32 kernel attention_hdw_window_f32_kernel<W> (W = 32, 96; bf16 build only) is attention_window_f32_kernel with the width as a template
// parameter; 128-channel heads have no fp32 verification mode, with or without the option.
#include "attn_core.h"
#include "attn_hdw_tiles.h"
#include "attn_window.h"
#include "sat_common.h"

namespace {

constexpr int Q_BLOCK = 256;          // queries per workgroup

// q [B,H,Sq_pad,W] (times log2(e)), k [B,KVH,Sk_pad,W] (rows shifted by ob), vt [B,KVH,W,Sk_pad] (vt_pos order) -> out [B*S, H*W]
template <int W>
__global__ __launch_bounds__(512) void attention_hdw_window_kernel(const op_t* __restrict__ q, const op_t* __restrict__ k, const op_t* __restrict__ vt,
                                                                   op_t* __restrict__ out, int H, int KVH, int S, int Sq_pad, int Sk_pad, int KS) {
    using T = attnw::Tiles<W>;
    constexpr int KT = T::KV_TILE, KSTEPS = W / 16, DB = W / 32;
    sat_f16_saturate();
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = lane >> 5;
    const int l31 = lane & 31;
    // consecutive LOGICAL workgroup ids (x = query block fastest) share an XCD and so one L2 copy of their K / V^T: attention.hip
    const int lin = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
    const int lid = xcd_remap(lin, gridDim.x * gridDim.y * gridDim.z);
    const int bx = lid % gridDim.x;
    const int h = (lid / gridDim.x) % gridDim.y, b = lid / (gridDim.x * gridDim.y);
    const int kvh = h / (H / KVH);
    const int qi = bx * Q_BLOCK + wave * 32 + l31;         // the last workgroup may reach beyond Sq_pad

    opx8 qf[KSTEPS];
    {
        const op_t* qp = q + ((size_t)(b * H + h) * Sq_pad + (qi < Sq_pad ? qi : Sq_pad - 1)) * W + half * 8;
#pragma unroll
        for (int t = 0; t < KSTEPS; ++t) qf[t] = *reinterpret_cast<const opx8*>(qp + t * 16);
    }

    // K rows / V^T columns of sequence b start at ob = (b*S) & 3 (head_split_hdw.hip, kind bit 2)
    const int ob = (b * S) & 3;
    const int t_first = attnw::first_tile(bx * Q_BLOCK, ob, KS, S, KT);                           // bx * Q_BLOCK < S: the grid is cdiv(S, Q_BLOCK) wide
    const int t_count = attnw::last_tile(bx * Q_BLOCK, Q_BLOCK, ob, KS, S, KT) - t_first + 1;      // >= 1; the last tile ends at or below Sk_pad

    // LDS-DMA pieces of this wave, exactly those of attention_hdw_kernel: the header says why the holes and the spare rows stay in bounds
    const op_t* kbase = k + (size_t)(b * KVH + kvh) * Sk_pad * W;
    const op_t* vbase = vt + (size_t)(b * KVH + kvh) * W * Sk_pad;
    const op_t* ksrc[T::K_PIECES];
    const op_t* vsrc[T::VT_PIECES];
#pragma unroll
    for (int i = 0; i < T::K_PIECES; ++i) {
        const int krow = T::k_dma_row(wave + 8 * i, lane);                              // < KT
        int chunk = T::k_dma_chunk(wave + 8 * i, lane);
        if constexpr (T::K_HOLES)
            if (chunk >= T::K_CHUNKS) chunk = 0;                                        // W = 96: a hole of the padded row
        ksrc[i] = kbase + (size_t)krow * W + (chunk << 3);                              // + tile * KT rows
    }
#pragma unroll
    for (int i = 0; i < T::VT_PIECES; ++i) {
        int vrow = T::vt_dma_row(wave + 8 * i, lane);
        const int chunk = T::vt_dma_chunk(wave + 8 * i, lane);                          // (of the LDS row it lands in)
        if constexpr (T::VT_SPARE)
            if (vrow >= W) vrow -= 32;                                                  // W = 96: the spare rows 96..127
        vsrc[i] = vbase + (size_t)vrow * Sk_pad + (chunk << 3);                         // + tile * KT keys
    }
    auto stage_in = [&](int tile, int stage) {
        char* sk = smem + stage * T::STAGE_BYTES;
        char* sv = sk + T::K_TILE_BYTES;
#pragma unroll
        for (int i = 0; i < T::K_PIECES; ++i)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(ksrc[i] + (size_t)tile * KT * W),
                                             (__attribute__((address_space(3))) void*)(sk + (wave + 8 * i) * 1024), 16, 0, 0);
#pragma unroll
        for (int i = 0; i < T::VT_PIECES; ++i)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(vsrc[i] + (size_t)tile * KT),
                                             (__attribute__((address_space(3))) void*)(sv + (wave + 8 * i) * 1024), 16, 0, 0);
    };

    attn::State<1, DB> st;
    st.init(half);

    // a wave whose 32 queries are all beyond S still copies tiles and joins the barriers, but skips the matrix and softmax work
    const int wq_first = __builtin_amdgcn_readfirstlane(bx * Q_BLOCK + wave * 32);
    const bool wave_active = wq_first < S;
    const attnw::Range wr = attnw::wave_range(wave_active ? wq_first : S - 1, 32, ob, KS, S);
    const int k_lo = attnw::key_lo(qi, ob, KS, S), k_hi = k_lo + KS;

    attn::walk3<T::K_PIECES + T::VT_PIECES>(t_first, t_count, stage_in, [&](int tile, int stage) {
        if (!wave_active) return;
        const char* sk = smem + stage * T::STAGE_BYTES;
        attn::tile<1, 0, attn::MASK_WINDOW, attn::LayoutHdw<W>>(st, qf, sk, sk + T::K_TILE_BYTES, false, tile * KT, k_lo, k_hi, false, 1.0f, l31, half, 0,
                                                                0, wr);
    });

    op_t* op = out + ((size_t)b * S + qi) * ((size_t)H * W) + h * W + 8 * half;
    attn::store_out(st.oacc, 1.0f / attn::half_sum(st.l_run), op, qi < S);
}

#ifndef SAT_OPERAND_F16
// fp32: attention_window_f32_kernel at W channels -- one query per lane, K / V rows are wave-uniform loads, online softmax over chunks of 8 keys
// from the first key of the wave's union to its last; a lane masks the keys outside its own window.  The running maximum starts at -1e30, not
// -inf: a chunk that shows a lane no key leaves (m, l, o) as they are.  q [B,H,S,W], k / v [B,KVH,S,W] -> out [B*S, H*W]
template <int W>
__global__ __launch_bounds__(64) void attention_hdw_window_f32_kernel(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                                                                      float* __restrict__ out, int H, int KVH, int S, int KS, float scale) {
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

template <int W>
int launch(const op_t* q, const op_t* k, const op_t* vt, op_t* out, int b, int h, int kvh, int s_len, int sq_pad, int sk_pad, int kernel_size,
           hipStream_t s) {
    using T = attnw::Tiles<W>;
    SAT_CHECK_ARG(sq_pad % 128 == 0 && sk_pad % T::KV_TILE == 0, SAT_E_INVALID,
                  "attention_hdw (window): with %d-channel heads sq_pad %% 128 and sk_pad %% %d must be 0 (got %d, %d)", W, T::KV_TILE, sq_pad, sk_pad);
    const auto kernel = attention_hdw_window_kernel<W>;
    SAT_TRY(sat_ensure_dynamic_lds(reinterpret_cast<const void*>(kernel), T::LDS_BYTES));
    hipLaunchKernelGGL(kernel, dim3(cdiv(s_len, Q_BLOCK), h, b), dim3(512), T::LDS_BYTES, s, q, k, vt, out, h, kvh, s_len, sq_pad, sk_pad, kernel_size);
    SAT_LAUNCH_CHECK();
    return 0;
}

}  // namespace

// What NATTEN rejects: an even kernel size, one of 1 or less, a sequence shorter than the kernel (as in attention_window.hip)
#define SAT_CHECK_WINDOW(what, ks, s_len)                                                                                              \
    SAT_CHECK_ARG((ks) > 1 && ((ks) & 1), SAT_E_INVALID, what ": kernel_size %d must be odd and greater than 1", (ks));                \
    SAT_CHECK_ARG((s_len) >= (ks), SAT_E_INVALID, what ": a sequence of %d rows is shorter than kernel_size %d", (s_len), (ks))

#ifdef SAT_OPERAND_F16
int sat_launch_attention_hdw_window_f16(const void* q, const void* k, const void* vt, void* out, int b, int h, int kvh, int head_dim, int s_len,
                                        int sq_pad, int sk_pad, int kernel_size, hipStream_t s) {
    return f16::sat_launch_attention_hdw_window((const op_t*)q, (const op_t*)k, (const op_t*)vt, (op_t*)out, b, h, kvh, head_dim, s_len, sq_pad, sk_pad,
                                                kernel_size, s, 1);
}
#endif

int SAT_OPNS::sat_launch_attention_hdw_window(const op_t* q, const op_t* k, const op_t* vt, op_t* out, int b, int h, int kvh, int head_dim, int s_len,
                                              int sq_pad, int sk_pad, int kernel_size, hipStream_t s, int f16) {
#ifndef SAT_OPERAND_F16
    if (f16) return sat_launch_attention_hdw_window_f16(q, k, vt, out, b, h, kvh, head_dim, s_len, sq_pad, sk_pad, kernel_size, s);
#else
    SAT_CHECK_ARG(f16, SAT_E_INVALID, "attention_hdw (window): the fp16 build takes fp16 tensors and writes fp16");
#endif
    SAT_CHECK_ARG(head_dim == 32 || head_dim == 96 || head_dim == 128, SAT_E_UNSUPPORTED,
                  "attention_hdw (window): dim_heads %d (this kernel is built for 32, 96 and 128)", head_dim);
    SAT_CHECK_ATTENTION("attention_hdw (window)", "s", s_len, s_len, true, false);
    SAT_CHECK_WINDOW("attention_hdw (window)", kernel_size, s_len);
    if (head_dim == 32) return launch<32>(q, k, vt, out, b, h, kvh, s_len, sq_pad, sk_pad, kernel_size, s);
    if (head_dim == 96) return launch<96>(q, k, vt, out, b, h, kvh, s_len, sq_pad, sk_pad, kernel_size, s);
    return launch<128>(q, k, vt, out, b, h, kvh, s_len, sq_pad, sk_pad, kernel_size, s);
}

#ifndef SAT_OPERAND_F16
int sat_launch_attention_f32_window_w(const float* q, const float* k, const float* v, float* out, int b, int h, int kvh, int head_dim, int s_len,
                                      int kernel_size, float score_scale, hipStream_t s) {
    SAT_CHECK_ARG(head_dim == 32 || head_dim == 96, SAT_E_UNSUPPORTED, "attention_f32 (window): dim_heads %d (this kernel is built for 32 and 96)",
                  head_dim);
    SAT_CHECK_ARG(q && k && v && out && b > 0 && h > 0 && kvh > 0 && h % kvh == 0 && s_len > 0, SAT_E_INVALID, "attention_f32 (window): bad args");
    SAT_CHECK_ARG((((uintptr_t)q | (uintptr_t)out) & 15) == 0, SAT_E_INVALID, "attention_f32 (window): q and out must be 16-byte aligned");
    SAT_CHECK_ARG(h <= 65535 && b <= 65535, SAT_E_UNSUPPORTED, "attention_f32 (window): %d heads / %d sequences exceed the grid", h, b);
    SAT_CHECK_WINDOW("attention_f32 (window)", kernel_size, s_len);
    SAT_CHECK_ARG(score_scale > 0.f && score_scale <= 1e6f, SAT_E_INVALID, "attention_f32 (window): score scale %g is not a positive finite number",
                  (double)score_scale);
    const dim3 grid(cdiv(s_len, 64), h, b);
    if (head_dim == 32)
        hipLaunchKernelGGL(attention_hdw_window_f32_kernel<32>, grid, dim3(64), 0, s, q, k, v, out, h, kvh, s_len, kernel_size, score_scale);
    else hipLaunchKernelGGL(attention_hdw_window_f32_kernel<96>, grid, dim3(64), 0, s, q, k, v, out, h, kvh, s_len, kernel_size, score_scale);
    SAT_LAUNCH_CHECK();
    return 0;
}
#endif
