// Head split for DiTs with 32-, 96- and 128-channel heads (the staged route of dit_plan.hip: the fused heads epilogues of gemm_bf16.hip /
// gemm_ph8.hip keep one head = one 64-column wave tile).  Input: the fp32 output [M, parts * H * W] of an EPI_F32 GEMM (to_qkv, cross to_q,
// to_kv: no bias).  Per part, with the meaning of the HeadsEpi::kind bits (sat_common.h), on fp32 and in this order:
//   bit 4  L2-normalise the head row over its W channels, x / max(|x|, 1e-12)                              (qk_norm, transformer.py:433-436)
//   bit 1  rotate as RotaryEmbedding(max(W / 2, 32)) does (transformer.py:99-183, 737): W = 32 rotates the whole head, pairs (j, j + 16), 16
//          angles per position; W = 96 rotates channels 0..47, pairs (j, j + 24), 24 angles, channels 48..95 pass; W = 128 rotates channels
//          0..63, pairs (j, j + 32), 32 angles, channels 64..127 pass
//   bit 3  multiply by the query pre-scale log2(e) / sqrt(W)
//   then round ONCE to the operand type and store:
//   row-major parts     [B, H, Spad, W]; key-side parts (bit 2) start sequence b at row (b * S) & 3
//   transposed part (bit 0, V)  [B, H, W, Spad], key index permuted by vt_pos
// Only valid rows are written on the row-major parts; the pads are the caller's memset.  Transposed blocks write zeros outside the sequence.
// One workgroup = 64 destination rows of one (batch, part, head).
// Row-major, W = 128: 16 lanes per row, 8 channels = one 16-byte store per lane; the norm is a sum over one DPP row of 16 lanes, the rotation
// partner (lane ^ 4) is re-read from the fp32 input instead of exchanged.  No LDS.
// Row-major, W = 32 and 96: the 64 x W block is staged in LDS as fp32 (a head row is 4 or 12 16-byte store items, no power of two for 96, so no
// lane-group owns a row); four lanes sum a row's squares, then each item of 8 channels reads its values and its rotation partners from LDS and
// leaves as one 16-byte store.  The two bodies sum a row's squares in different orders: each width keeps its own.
// Transposed: THROUGH LDS -- the 64 x W block is rounded, written to an LDS image [W][64 (+8 pad)] at the permuted key position (vt_pos
// permutes inside aligned groups of 16, so inside the tile) and leaves as 16-byte stores of 8 consecutive keys of one channel; rows of the block
// outside the sequence are written as zeros, which is what the pad holds anyway.  That image is all the LDS of W = 128 (18 KiB).
#include "sat_common.h"

namespace {

constexpr int ROWS = 64;          // destination rows per workgroup
constexpr int LDW = ROWS + 8;     // LDS row of the transposed image, in elements: 144 B keeps every 8-key group 16-byte aligned

struct SplitArgs {
    op_t* out[3];
    int kind[3];
    int parts, heads, S, Spad;
    float qscale;
    const float* rope_cos;        // [S][R / 2], R = max(W / 2, 32)
    const float* rope_sin;
};

template <int W>
__global__ __launch_bounds__(256) void head_split_hdw_kernel(const float* __restrict__ x, const SplitArgs a) {
    static_assert(W == 32 || W == 96 || W == 128, "head widths of the staged route");
    constexpr int RH = (W / 2 > 32 ? W / 2 : 32) / 2;      // rotation pairs (j, j + RH): 16, 24 or 32
    constexpr bool STAGED = W != 128;                       // row-major parts through an fp32 LDS block; W = 128 keeps a row in 16 lanes
    constexpr int LDX = W + 4;                              // fp32 staging row, in floats: 16-byte aligned, rows start 4 banks apart
    constexpr int XS_BYTES = STAGED ? ROWS * LDX * 4 : 0, TI_BYTES = W * LDW * 2;
    sat_f16_saturate();
    __shared__ __attribute__((aligned(16))) char smem[XS_BYTES > TI_BYTES ? XS_BYTES : TI_BYTES];
    const int tid = threadIdx.x;
    const int part = blockIdx.y / a.heads, hh = blockIdx.y % a.heads, b = blockIdx.z;
    const int kind = a.kind[part];
    const int S = a.S, Spad = a.Spad;
    const int ob = (kind & 4) ? (b * S) & 3 : 0;
    const int r0 = blockIdx.x * ROWS;
    if (r0 >= ob + S) return;                                   // block-uniform: nothing of the sequence in these rows
    const size_t ld = (size_t)a.parts * a.heads * W;
    const float* xh = x + (size_t)b * S * ld + (size_t)(part * a.heads + hh) * W;      // row s of the sequence at xh + s * ld
    op_t* dst = a.out[part] + (size_t)(b * a.heads + hh) * Spad * W;

    if (kind & 1) {
        // ---- transposed part: fp32 [64 rows][W ch] -> LDS [W ch][64 keys, permuted] -> 16-byte stores
        op_t* timg = reinterpret_cast<op_t*>(smem);
#pragma unroll
        for (int pass = 0; pass < ROWS * (W / 4) / 256; ++pass) {
            const int idx = pass * 256 + tid;
            const int rl = idx / (W / 4), ch4 = (idx % (W / 4)) * 4;
            const int s = r0 + rl - ob;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (s >= 0 && s < S) v = *reinterpret_cast<const f32x4*>(xh + (size_t)s * ld + ch4);
            const int col = vt_pos(rl);
#pragma unroll
            for (int e = 0; e < 4; ++e) timg[(ch4 + e) * LDW + col] = f32_to_op(v[e]);
        }
        __syncthreads();
#pragma unroll
        for (int pass = 0; pass < W * ROWS / 8 / 256; ++pass) {
            const int idx = pass * 256 + tid;
            const int ch = idx >> 3, kc = idx & 7;
            *reinterpret_cast<u32x4*>(dst + (size_t)ch * Spad + r0 + kc * 8) = *reinterpret_cast<const u32x4*>(&timg[ch * LDW + kc * 8]);
        }
        return;
    }

    if constexpr (!STAGED) {
        // ---- row-major parts in registers
        const int sub = tid & 15, rr = tid >> 4;
#pragma unroll
        for (int pass = 0; pass < ROWS / 16; ++pass) {
            const int r = r0 + pass * 16 + rr;
            const int s = r - ob;
            const bool valid = s >= 0 && s < S;
            const int sc = s < 0 ? 0 : (s < S ? s : S - 1);          // every lane computes (the norm is a 16-lane reduction), valid rows store
            const float* xr = xh + (size_t)sc * ld;
            float v[8];
            {
                const f32x4 lo = *reinterpret_cast<const f32x4*>(xr + sub * 8), hi = *reinterpret_cast<const f32x4*>(xr + sub * 8 + 4);
#pragma unroll
                for (int e = 0; e < 4; ++e) { v[e] = lo[e]; v[4 + e] = hi[e]; }
            }
            float inv = 1.0f;
            if (kind & 16) {
                float ss = 0.f;
#pragma unroll
                for (int e = 0; e < 8; ++e) ss = fmaf(v[e], v[e], ss);
                ss = row16_sum(ss);
                inv = 1.0f / fmaxf(sqrtf(ss), 1e-12f);
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] *= inv;
            }
            if ((kind & 2) && sub < 8) {
                // channels 8*sub .. +8 < 64: partner channels at 8 * (sub ^ 4), angle index j = channel & 31
                const float* xp = xr + (sub ^ 4) * 8;
                const f32x4 plo = *reinterpret_cast<const f32x4*>(xp), phi = *reinterpret_cast<const f32x4*>(xp + 4);
                const float* cs = a.rope_cos + (size_t)sc * 32 + (sub & 3) * 8;
                const float* sn = a.rope_sin + (size_t)sc * 32 + (sub & 3) * 8;
                const f32x4 clo = *reinterpret_cast<const f32x4*>(cs), chi = *reinterpret_cast<const f32x4*>(cs + 4);
                const f32x4 slo = *reinterpret_cast<const f32x4*>(sn), shi = *reinterpret_cast<const f32x4*>(sn + 4);
                const float sign = sub < 4 ? -1.0f : 1.0f;            // x1 cos - x2 sin | x2 cos + x1 sin
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float pv = (e < 4 ? plo[e] : phi[e - 4]) * inv;
                    const float c = e < 4 ? clo[e] : chi[e - 4], sgn_s = sign * (e < 4 ? slo[e] : shi[e - 4]);
                    v[e] = fmaf(pv, sgn_s, v[e] * c);
                }
            }
            if (kind & 8) {
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] *= a.qscale;
            }
            if (valid)
                *reinterpret_cast<u32x4*>(dst + (size_t)r * W + sub * 8) =
                    u32x4{pack_op2(v[0], v[1]), pack_op2(v[2], v[3]), pack_op2(v[4], v[5]), pack_op2(v[6], v[7])};
        }
        return;
    }

    // ---- row-major parts through LDS: stage the block (rows outside the sequence as zeros: they are computed and not stored)
    __shared__ float rinv[ROWS];
    float* xs = reinterpret_cast<float*>(smem);
#pragma unroll
    for (int pass = 0; pass < ROWS * (W / 4) / 256; ++pass) {
        const int idx = pass * 256 + tid;
        const int rl = idx / (W / 4), ch4 = (idx % (W / 4)) * 4;
        const int s = r0 + rl - ob;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (s >= 0 && s < S) v = *reinterpret_cast<const f32x4*>(xh + (size_t)s * ld + ch4);
        *reinterpret_cast<f32x4*>(&xs[rl * LDX + ch4]) = v;
    }
    __syncthreads();
    if (kind & 16) {      // (block-uniform) four lanes of a quad per row: channels q, q + 4, ...
        const int rl = tid >> 2, qd = tid & 3;
        float ss = 0.f;
#pragma unroll
        for (int c = 0; c < W / 4; ++c) {
            const float v = xs[rl * LDX + qd + 4 * c];
            ss = fmaf(v, v, ss);
        }
        ss += dpp_move<0xB1>(ss);          // quad_perm [1,0,3,2]
        ss += dpp_move<0x4E>(ss);          // quad_perm [2,3,0,1]
        if (qd == 0) rinv[rl] = 1.0f / fmaxf(sqrtf(ss), 1e-12f);
        __syncthreads();
    }
#pragma unroll
    for (int pass = 0; pass < ROWS * (W / 8) / 256; ++pass) {
        const int idx = pass * 256 + tid;
        const int rl = idx / (W / 8), ch0 = (idx % (W / 8)) * 8;
        const int r = r0 + rl, s = r - ob;
        if (s < 0 || s >= S) continue;
        const float inv = (kind & 16) ? rinv[rl] : 1.0f;
        const float* xr = xs + rl * LDX;
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = xr[ch0 + e] * inv;
        if ((kind & 2) && ch0 < 2 * RH) {
            // RH % 8 == 0: the 8 channels lie on one side of the pair.  x1 cos - x2 sin | x2 cos + x1 sin, angle index j = channel mod RH
            const bool low = ch0 < RH;
            const int j0 = low ? ch0 : ch0 - RH;
            const float* xp = xr + (low ? ch0 + RH : ch0 - RH);
            const float* cs = a.rope_cos + (size_t)s * RH + j0;
            const float* sn = a.rope_sin + (size_t)s * RH + j0;
            const float sign = low ? -1.0f : 1.0f;
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = fmaf(xp[e] * inv, sign * sn[e], v[e] * cs[e]);
        }
        if (kind & 8) {
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] *= a.qscale;
        }
        *reinterpret_cast<u32x4*>(dst + (size_t)r * W + ch0) =
            u32x4{pack_op2(v[0], v[1]), pack_op2(v[2], v[3]), pack_op2(v[4], v[5]), pack_op2(v[6], v[7])};
    }
}

#ifndef SAT_OPERAND_F16
__global__ void rope_table_hdw_kernel(const float* __restrict__ inv_freq, float* __restrict__ cos_t, float* __restrict__ sin_t, int s_len, int pairs) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= s_len * pairs) return;
    const float f = (float)(i / pairs) * inv_freq[i % pairs];
    cos_t[i] = cosf(f);
    sin_t[i] = sinf(f);
}
#endif

template <int W>
void launch(const float* x, const SplitArgs& a, int b, hipStream_t s) {
    hipLaunchKernelGGL(head_split_hdw_kernel<W>, dim3(cdiv(a.S + 3, ROWS), a.parts * a.heads, b), dim3(256), 0, s, x, a);
}

}  // namespace

#ifdef SAT_OPERAND_F16
int sat_launch_head_split_hdw_f16(const float* x, const void* heads_epi, int head_dim, int b, hipStream_t s) {
    return f16::sat_launch_head_split_hdw(x, *static_cast<const f16::HeadsEpi*>(heads_epi), head_dim, b, s, 1);
}
#else
// the [s_len][pairs] rotation table of RotaryEmbedding(2 * pairs): angle = position * inv_freq[j], as sat_launch_rope_table builds the [s_len][16] one
int sat_launch_rope_table_hdw(const float* inv_freq, float* cos_t, float* sin_t, int s_len, int head_dim, hipStream_t s) {
    SAT_CHECK_ARG(head_dim == 32 || head_dim == 96 || head_dim == 128, SAT_E_UNSUPPORTED, "rope_table_hdw: dim_heads %d (32, 96 or 128)", head_dim);
    SAT_CHECK_ARG(inv_freq && cos_t && sin_t && s_len > 0, SAT_E_INVALID, "rope_table_hdw: bad argument");
    const int pairs = sat_rope_pairs(head_dim);
    hipLaunchKernelGGL(rope_table_hdw_kernel, dim3(cdiv((int64_t)s_len * pairs, 256)), dim3(256), 0, s, inv_freq, cos_t, sin_t, s_len, pairs);
    SAT_LAUNCH_CHECK();
    return 0;
}
#endif

// he: out / kind / qscale / parts / heads / S / Spad / rope_cos / rope_sin ([S][sat_rope_pairs(head_dim)]) are read; the fused-attention fields are not
int SAT_OPNS::sat_launch_head_split_hdw(const float* x, const HeadsEpi& he, int head_dim, int b, hipStream_t s, int f16) {
#ifndef SAT_OPERAND_F16
    if (f16) return sat_launch_head_split_hdw_f16(x, &he, head_dim, b, s);
#else
    SAT_CHECK_ARG(f16, SAT_E_INVALID, "head_split_hdw: the fp16 build writes fp16");
#endif
    SAT_CHECK_ARG(head_dim == 32 || head_dim == 96 || head_dim == 128, SAT_E_UNSUPPORTED,
                  "head_split_hdw: dim_heads %d (this kernel is built for 32, 96 and 128)", head_dim);
    SAT_CHECK_ARG(x && b > 0 && he.parts >= 1 && he.parts <= 3 && he.heads > 0 && he.S > 0, SAT_E_INVALID, "head_split_hdw: bad argument");
    SAT_CHECK_ARG(b <= 65535 && he.parts * he.heads <= 65535, SAT_E_UNSUPPORTED, "head_split_hdw: %d heads / %d sequences exceed the grid", he.heads, b);
    SAT_CHECK_ARG(he.Spad % ROWS == 0 && he.Spad >= he.S + 3, SAT_E_INVALID, "head_split_hdw: s_pad %d must be a multiple of 64 and >= s + 3 = %d",
                  he.Spad, he.S + 3);
    SAT_CHECK_ARG(((uintptr_t)x & 15) == 0, SAT_E_INVALID, "head_split_hdw: the input must be 16-byte aligned");
    SplitArgs a{};
    bool rope = false;
    for (int pt = 0; pt < he.parts; ++pt) {
        SAT_CHECK_ARG(he.out[pt] && ((uintptr_t)he.out[pt] & 15) == 0, SAT_E_INVALID, "head_split_hdw: destination %d null or not 16-byte aligned", pt);
        SAT_CHECK_ARG((he.kind[pt] & ~31) == 0 && (!(he.kind[pt] & 1) || (he.kind[pt] & (2 | 8 | 16)) == 0), SAT_E_UNSUPPORTED,
                      "head_split_hdw: kind 0x%x of part %d (a transposed part takes no norm, rotation or pre-scale)", he.kind[pt], pt);
        a.out[pt] = he.out[pt];
        a.kind[pt] = he.kind[pt];
        rope = rope || (he.kind[pt] & 2);
    }
    SAT_CHECK_ARG(!rope || (he.rope_cos && he.rope_sin && (((uintptr_t)he.rope_cos | (uintptr_t)he.rope_sin) & 15) == 0), SAT_E_INVALID,
                  "head_split_hdw: a rotating part needs the 16-byte aligned [S][%d] tables", sat_rope_pairs(head_dim));
    a.parts = he.parts; a.heads = he.heads; a.S = he.S; a.Spad = he.Spad; a.qscale = he.qscale;
    a.rope_cos = he.rope_cos; a.rope_sin = he.rope_sin;
    if (head_dim == 32) launch<32>(x, a, b, s);
    else if (head_dim == 96) launch<96>(x, a, b, s);
    else launch<128>(x, a, b, s);
    SAT_LAUNCH_CHECK();
    return 0;
}
