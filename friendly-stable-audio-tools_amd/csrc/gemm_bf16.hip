// bf16 MFMA GEMM for the DiT projections and the SwiGLU FFN (SURVEY.md K2,K5,K6,K7,K8):
//     C[M,N] = A[M,K] . W[N,K]^T      A, W bf16 (K contiguous), fp32 accumulate
// replacing the nn.Linear calls at models/transformer.py:222,270,314,311-312,319 of the
// reference.  gfx950 only: v_mfma_f32_32x32x16_bf16, 64-wide wavefronts, LDS-staged tiles
// (XOR-swizzled, conflict-free ds_read_b128), register-staged double buffering with one
// barrier per K-tile, XCD-aware tile rasterisation.
//
// Fused epilogues
//   EPI_F32    C (fp32) = acc (+bias) (+C)           -> to_out / FF-out + residual add
//   EPI_SWIGLU H (bf16) = (acc_v+b_v) * silu(acc_g+b_g)   (W rows interleaved 32 value /
//              32 gate so both land in one wave tile; models/transformer.py:232-235)
//   EPI_HEADS  split into heads, partial RoPE (models/transformer.py:158-183,438-452) on
//              q/k, store q/k as [B,H,Spad,64] and v transposed as [B,H,64,Spad]
#include <stdlib.h>

#include <type_traits>

#include <algorithm>

#include "gemm_ring.h"

namespace {

// QKN: the alternative build of an epilogue.  EPI_HEADS: the instantiation behind EPI_HEADS_QKN -- parts with kind bit 4 are L2-normalised per
// head (qk_norm).  EPI_SWIGLU: the one behind EPI_ACT16 -- H [M, N] = act(acc + bias), no value / gate pairing (GemmArgs::act)
template <int EPI, int MI, int NI, bool LNC = false, bool QKN = false>
__device__ __forceinline__ void gemm_epilogue(const GemmArgs& g, f32x16 (&acc)[MI][NI], const int mw, const int nw, const int half,
                                              const int l31, const float2* ln = nullptr, const float* lc1 = nullptr,
                                              const float* lc2 = nullptr) {
    // LNC (bf16 pipelined kernels, EPI_HEADS / EPI_SWIGLU): out = rstd * (acc - mean * c1) + c2 with (mean, rstd) of the wave's TM
    // token rows at `ln` and the wave's 64 channel constants at lc1 / lc2, all in LDS -- the LayerNorm fold of GemmArgs, or
    // (0, 1), 0, bias without it
    const int M = g.M, N = g.N;
    (void)N;
    // acc[i][j][r]: row = i*32 + (r&3) + 8*(r>>2) + 4*half ; col = j*32 + l31   (guide section 3)

    if constexpr (EPI == EPI_F32) {
        float* __restrict__ C = g.C;
        const int ldc = g.ldc;
        float bia[NI];
#pragma unroll
        for (int j = 0; j < NI; ++j) bia[j] = g.bias ? g.bias[nw + j * 32 + l31] : 0.f;
        const bool accum = g.accumulate != 0;
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int rh = 0; rh < 2; ++rh) {
                // residual reads are issued as one batch per 16-row half block (16 loads in flight), then added
                float old[8][NI];
#pragma unroll
                for (int r8 = 0; r8 < 8; ++r8) {
                    const int r = rh * 8 + r8;
                    int m = mw + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
#pragma unroll
                    for (int j = 0; j < NI; ++j)
                        old[r8][j] = (accum && m < M) ? C[(size_t)m * ldc + nw + j * 32 + l31] : 0.f;
                }
#pragma unroll
                for (int r8 = 0; r8 < 8; ++r8) {
                    const int r = rh * 8 + r8;
                    int m = mw + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                    if (m < M) {
                        if (g.gate) {      // adaLN gated branch (transformer.py:674, 688): wave-uniform pointer test
                            const float* gr = g.gate + (size_t)(m / g.gate_rows) * g.gate_ld + nw + l31;
#pragma unroll
                            for (int j = 0; j < NI; ++j)
                                C[(size_t)m * ldc + nw + j * 32 + l31] = (acc[i][j][r] + bia[j]) * gr[j * 32] + old[r8][j];
                        } else {
#pragma unroll
                            for (int j = 0; j < NI; ++j) C[(size_t)m * ldc + nw + j * 32 + l31] = acc[i][j][r] + bia[j] + old[r8][j];
                        }
                    }
                }
            }
    } else if constexpr (EPI == EPI_SWIGLU && QKN) {      // EPI_ACT16 (the 2-stage kernels: no LayerNorm fold here)
        op_t* __restrict__ H = g.H;
        const bool silu = g.act != 0;
        float bia[NI];
#pragma unroll
        for (int j = 0; j < NI; ++j) bia[j] = g.bias ? g.bias[nw + j * 32 + l31] : 0.f;
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = mw + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                if (m < M) {
#pragma unroll
                    for (int j = 0; j < NI; ++j) {
                        const float v = acc[i][j][r] + bia[j];
                        H[(size_t)m * N + nw + j * 32 + l31] = f32_to_op(silu ? silu_f(v) : v);
                    }
                }
            }
    } else if constexpr (EPI == EPI_SWIGLU) {
        op_t* __restrict__ H = g.H;
        const int ldh = N >> 1;
        const float bv = g.bias ? g.bias[nw + l31] : 0.f;
        const float bg = g.bias ? g.bias[nw + 32 + l31] : 0.f;
        const int hc = (nw >> 1) + l31;
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                int m = mw + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                float hv = 0.f;
                if (m < M) {
                    float v = acc[i][0][r] + bv;
                    float gt = acc[i][1][r] + bg;
                    hv = v * silu_f(gt);
                }
                if (g.H8) {
                    // MXFP8: the 32 lanes of this half hold the 32 consecutive hidden columns of one block of row m.
                    // scale = 2^e with e = ceil(log2(amax / 448)) (so that amax / scale <= 448), stored as E8M0 = e + 127
                    const float am = half32_max(fabsf(hv));
                    const float t = am * (1.0f / 448.0f);
                    const unsigned tb = __float_as_uint(t);
                    int e = (int)((tb >> 23) & 0xff) - 127 + ((tb & 0x7fffff) ? 1 : 0);
                    e = am > 0.f ? (e < -127 ? -127 : (e > 127 ? 127 : e)) : -127;
                    const float inv = __uint_as_float((unsigned)(127 - e) << 23);          // 2^-e (e = -127 -> 2^254: only for an all-zero block)
                    const unsigned q = __builtin_amdgcn_cvt_pk_fp8_f32(hv * inv, 0.f, 0u, false);
                    if (m < M) {
                        g.H8[(size_t)m * ldh + hc] = (unsigned char)(q & 0xff);
                        if (l31 == 0) g.Hs[(size_t)m * (ldh >> 5) + (hc >> 5)] = (unsigned char)(e + 127);
                    }
                } else if (m < M) {
                    H[(size_t)m * ldh + hc] = f32_to_op(hv);
                }
            }
    } else {   // EPI_HEADS
        const HeadsEpi& he = g.heads;
        const int hp = he.heads * 64;
        const int part = nw / hp;
        const int head = (nw - part * hp) >> 6;
        const int kind = he.kind[part];
        op_t* __restrict__ dst = he.out[part];
        const int S = he.S, Spad = he.Spad;
        // K rows / V^T columns of sequence b are shifted by o_b = (b*S) & 3 (kind bit 2) so that the 4 consecutive
        // tokens a lane holds (rows 4q..4q+3 of the GEMM) land on an 8-byte aligned V^T span: one dwordx2 store
        // instead of four 2-byte scatters.  The attention kernel applies the same shift to its key index.
        const bool shift = (kind & 4) != 0;
        float c1a = 0.f, c1b = 0.f, c2a = 0.f, c2b = 0.f;
        if constexpr (LNC) {
            c1a = lc1[l31];
            c1b = lc1[32 + l31];
            c2a = lc2[l31];
            c2b = lc2[32 + l31];
        }
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int rq = 0; rq < 4; ++rq) {
                const int mb = mw + i * 32 + 8 * rq + 4 * half;          // first of 4 consecutive rows, multiple of 4
                float v0[4], v1[4];
                int bb[4], ss[4];
                f32x4 st01 = {0.f, 1.f, 0.f, 1.f}, st23 = {0.f, 1.f, 0.f, 1.f};      // (mean, rstd) of rows e = 0,1 / 2,3
                if constexpr (LNC) {
                    const f32x4* sp = reinterpret_cast<const f32x4*>(ln + i * 32 + 8 * rq + 4 * half);
                    st01 = sp[0];
                    st23 = sp[1];
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int r = rq * 4 + e;
                    int mm = mb + e;
                    mm = mm < M ? mm : M - 1;
                    bb[e] = mm / S;
                    ss[e] = mm - bb[e] * S;
                    v0[e] = acc[i][0][r];
                    v1[e] = acc[i][1][r];
                    if constexpr (LNC) {
                        const float mean = e < 2 ? st01[2 * e] : st23[2 * e - 4];
                        const float rstd = e < 2 ? st01[2 * e + 1] : st23[2 * e - 3];
                        v0[e] = rstd * (v0[e] - mean * c1a) + c2a;
                        v1[e] = rstd * (v1[e] - mean * c1b) + c2b;
                    }
                    if constexpr (QKN) {
                        if (kind & 16) {   // wave-uniform: the 64 channels of this head row sit in the 32 lanes of this half, two each
                            const float inv = rsqrtf(fmaxf(half32_sum(v0[e] * v0[e] + v1[e] * v1[e]), 1e-24f));      // 1 / max(|x|, 1e-12)
                            v0[e] *= inv;
                            v1[e] *= inv;
                        }
                    }
                    if (kind & 2) {   // wave-uniform: partial RoPE on d < 32 (pairs d, d^16)
                        float p = __shfl_xor(v0[e], 16, 64);
                        int jf = l31 & 15;
                        float cs = he.rope_cos[ss[e] * 16 + jf], sn = he.rope_sin[ss[e] * 16 + jf];
                        v0[e] = (l31 < 16) ? (v0[e] * cs - p * sn) : (v0[e] * cs + p * sn);
                    }
                }
                if (kind & 1) {
                    if (mb + 3 < M && bb[0] == bb[3]) {
                        const int ob = shift ? ((bb[0] * S) & 3) : 0;
                        const size_t hbase = ((size_t)(bb[0] * he.heads + head) * 64) * Spad;
                        const size_t base = hbase + vt_pos(ss[0] + ob);         // aligned group of 4 keys: stays a group of 4
                        opx4 p0, p1;
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            p0[e] = f32_to_op(v0[e]);
                            p1[e] = f32_to_op(v1[e]);
                        }
                        if (shift) {     // aligned: (ss[0] + ob) % 4 == mb % 4 == 0
                            *reinterpret_cast<opx4*>(dst + base + (size_t)l31 * Spad) = p0;
                            *reinterpret_cast<opx4*>(dst + base + (size_t)(32 + l31) * Spad) = p1;
                        } else {
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                const size_t pe = hbase + vt_pos(ss[0] + e);
                                dst[pe + (size_t)l31 * Spad] = p0[e];
                                dst[pe + (size_t)(32 + l31) * Spad] = p1[e];
                            }
                        }
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (mb + e < M) {
                                const int ob = shift ? ((bb[e] * S) & 3) : 0;
                                const size_t base = ((size_t)(bb[e] * he.heads + head) * 64) * Spad + vt_pos(ss[e] + ob);
                                dst[base + (size_t)l31 * Spad] = f32_to_op(v0[e]);
                                dst[base + (size_t)(32 + l31) * Spad] = f32_to_op(v1[e]);
                            }
                    }
                } else {
                    const float qs = (kind & 8) ? he.qscale : 1.0f;
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (mb + e < M) {
                            const int ob = shift ? ((bb[e] * S) & 3) : 0;
                            const size_t base = ((size_t)(bb[e] * he.heads + head) * Spad + ss[e] + ob) * 64;
                            dst[base + l31] = f32_to_op(v0[e] * qs);
                            dst[base + 32 + l31] = f32_to_op(v1[e] * qs);
                        }
                }
            }
    }
}

// ---------------------------------------------------------------------------------------------
// Epilogues on TRANSPOSED accumulators.  The deep-prefetch kernels issue their MFMAs with the operands swapped
// (W fragment as the A operand, activation fragment as the B operand), so a 32x32 block holds C^T: lane l31 owns TOKEN row
// m = mw + i*32 + l31, and its 16 registers are output channels n = nw + j*32 + 8*(r>>2) + 4*half + (r&3) -- four runs of
// four consecutive channels.  Everything a token needs is then lane-local:
//   * bf16 / e4m3 output: two runs are exchanged between the wave halves with v_permlane32_swap (lane l takes the partner's
//     low run, lane l+32 the high runs), so every lane writes 8 consecutive channels = one 16-byte (8-byte for e4m3) store
//     instead of sixteen 2-byte stores -- the epilogue is store-issue bound (guide T21), not bandwidth bound;
//   * RoPE: the rotation partner d^16 is register r^8 of the same lane, no cross-lane traffic, cos/sin are two 16-byte loads;
//   * SwiGLU / MXFP8 block maximum: value and gate, resp. the 32 channels of a block, sit in one lane pair.
// V^T (token-contiguous destination) and fp32 output keep the un-swapped orientation: the epilogue above, resp. the staged one below.
// ---------------------------------------------------------------------------------------------
// ROPE_PRE: the rotation table rows of all MI row blocks are fetched up front (not in the 128-register budget of the 16-wave tile)
template <int EPI, int MI, int NI, bool LNC = false, bool ROPE_PRE = true, bool QKN = false>
__device__ __forceinline__ void gemm_epilogue_t(const GemmArgs& g, f32x16 (&acc)[MI][NI], const int mw, const int nw, const int half,
                                                const int l31, const float2* ln = nullptr, const float* lc1 = nullptr,
                                                const float* lc2 = nullptr, unsigned (*qfrag)[8] = nullptr) {
    const int M = g.M, N = g.N;
    (void)N;
    static_assert(EPI == EPI_SWIGLU || EPI == EPI_HEADS, "fp32 output is never transposed");
    if constexpr (EPI == EPI_SWIGLU && QKN) {      // EPI_ACT16: lane = token row m, 16 channels of each 32-column block in its registers
        const bool silu = g.act != 0;
#pragma unroll
        for (int i = 0; i < MI; ++i) {
            const int m = mw + i * 32 + l31;
            float2 st = {0.f, 1.f};
            if constexpr (LNC) st = ln[i * 32 + l31];      // (mean, rstd) of the row under the LayerNorm fold, (0, 1) without it
#pragma unroll
            for (int j = 0; j < NI; ++j) {
                float hv[16];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int c = j * 32 + 4 * half + q * 8;
                    f32x4 c1 = {0.f, 0.f, 0.f, 0.f}, c2;
                    if constexpr (LNC) {      // lc2: ln_c2 under the fold (the bias is part of it), else the bias or zeros
                        c1 = *reinterpret_cast<const f32x4*>(lc1 + c);
                        c2 = *reinterpret_cast<const f32x4*>(lc2 + c);
                    } else {
                        c2 = g.bias ? *reinterpret_cast<const f32x4*>(g.bias + nw + c) : f32x4{0.f, 0.f, 0.f, 0.f};
                    }
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float v = st.y * (acc[i][j][4 * q + e] - st.x * c1[e]) + c2[e];
                        hv[4 * q + e] = silu ? silu_f(v) : v;
                    }
                }
                unsigned pk[8];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    pk[2 * q] = pack_op2(hv[4 * q], hv[4 * q + 1]);
                    pk[2 * q + 1] = pack_op2(hv[4 * q + 2], hv[4 * q + 3]);
                }
                half_swap(pk[0], pk[2]);      // 8 consecutive channels per lane: 16-byte stores (as the SwiGLU build below)
                half_swap(pk[1], pk[3]);
                half_swap(pk[4], pk[6]);
                half_swap(pk[5], pk[7]);
                if (m < M) {
                    op_t* hrow = g.H + (size_t)m * N + nw + j * 32 + 8 * half;
                    *reinterpret_cast<u32x4*>(hrow) = u32x4{pk[0], pk[1], pk[2], pk[3]};
                    *reinterpret_cast<u32x4*>(hrow + 16) = u32x4{pk[4], pk[5], pk[6], pk[7]};
                }
            }
        }
    } else if constexpr (EPI == EPI_SWIGLU) {
        static_assert(NI == 2, "value block + gate block");
        const int ldh = N >> 1;
        const int hc0 = nw >> 1;                       // first hidden column of this wave's 32
        [[maybe_unused]] f32x4 bv[LNC ? 1 : 4], bg[LNC ? 1 : 4];
        if constexpr (!LNC) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                bv[q] = g.bias ? *reinterpret_cast<const f32x4*>(g.bias + nw + 4 * half + q * 8) : f32x4{0.f, 0.f, 0.f, 0.f};
                bg[q] = g.bias ? *reinterpret_cast<const f32x4*>(g.bias + nw + 32 + 4 * half + q * 8) : f32x4{0.f, 0.f, 0.f, 0.f};
            }
        }
#pragma unroll
        for (int i = 0; i < MI; ++i) {
            const int m = mw + i * 32 + l31;
            float hv[16];
            if constexpr (LNC) {      // LayerNorm fold: finish the normalisation of token row m (bias is part of ln_c2)
                const float2 st = ln[i * 32 + l31];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int c = 4 * half + q * 8;
                    const f32x4 c1v = *reinterpret_cast<const f32x4*>(lc1 + c), c1g = *reinterpret_cast<const f32x4*>(lc1 + c + 32);
                    const f32x4 c2v = *reinterpret_cast<const f32x4*>(lc2 + c), c2g = *reinterpret_cast<const f32x4*>(lc2 + c + 32);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float v = st.y * (acc[i][0][4 * q + e] - st.x * c1v[e]) + c2v[e];
                        const float gt = st.y * (acc[i][1][4 * q + e] - st.x * c1g[e]) + c2g[e];
                        hv[4 * q + e] = m < M ? v * silu_f(gt) : 0.f;
                    }
                }
            } else {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float v = acc[i][0][r] + bv[r >> 2][r & 3];
                    const float gt = acc[i][1][r] + bg[r >> 2][r & 3];
                    hv[r] = m < M ? v * silu_f(gt) : 0.f;
                }
            }
            if (g.H8) {
                // MXFP8: the 32 hidden columns of this wave are ONE block of row m, held by the lane pair (l31, l31 + 32)
                float am = 0.f;
#pragma unroll
                for (int r = 0; r < 16; ++r) am = fmaxf(am, fabsf(hv[r]));
                {
                    unsigned a = __float_as_uint(am), b = a;
                    half_swap(a, b);                   // a: this value of the low half in both halves, b: of the high half
                    am = fmaxf(__uint_as_float(a), __uint_as_float(b));
                }
                const float t = am * (1.0f / 448.0f);
                const unsigned tb = __float_as_uint(t);
                int e = (int)((tb >> 23) & 0xff) - 127 + ((tb & 0x7fffff) ? 1 : 0);
                e = am > 0.f ? (e < -127 ? -127 : (e > 127 ? 127 : e)) : -127;
                const float inv = __uint_as_float((unsigned)(127 - e) << 23);          // 2^-e
                unsigned q8[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    unsigned w = __builtin_amdgcn_cvt_pk_fp8_f32(hv[4 * q] * inv, hv[4 * q + 1] * inv, 0u, false);
                    q8[q] = __builtin_amdgcn_cvt_pk_fp8_f32(hv[4 * q + 2] * inv, hv[4 * q + 3] * inv, w, true);
                }
                half_swap(q8[0], q8[1]);
                half_swap(q8[2], q8[3]);
                if (m < M) {
                    unsigned char* hrow = g.H8 + (size_t)m * ldh + hc0 + 8 * half;
                    *reinterpret_cast<u32x2*>(hrow) = u32x2{q8[0], q8[1]};
                    *reinterpret_cast<u32x2*>(hrow + 16) = u32x2{q8[2], q8[3]};
                    if (half == 0) g.Hs[(size_t)m * (ldh >> 5) + (hc0 >> 5)] = (unsigned char)(e + 127);
                }
            } else {
                unsigned pk[8];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    pk[2 * q] = pack_op2(hv[4 * q], hv[4 * q + 1]);
                    pk[2 * q + 1] = pack_op2(hv[4 * q + 2], hv[4 * q + 3]);
                }
                half_swap(pk[0], pk[2]);
                half_swap(pk[1], pk[3]);
                half_swap(pk[4], pk[6]);
                half_swap(pk[5], pk[7]);
                if (m < M) {
                    op_t* hrow = g.H + (size_t)m * ldh + hc0 + 8 * half;
                    *reinterpret_cast<u32x4*>(hrow) = u32x4{pk[0], pk[1], pk[2], pk[3]};
                    *reinterpret_cast<u32x4*>(hrow + 16) = u32x4{pk[4], pk[5], pk[6], pk[7]};
                }
            }
        }
    } else {   // EPI_HEADS, row-major destinations only ([B,H,Spad,64]: q, k); V^T takes the un-swapped orientation
        static_assert(NI == 2, "one head = two 32-column blocks");
        const HeadsEpi& he = g.heads;
        const int hp = he.heads * 64;
        const int part = nw / hp;
        const int head = (nw - part * hp) >> 6;
        const int kind = he.kind[part];
        op_t* __restrict__ dst = he.out[part];
        const int S = he.S, Spad = he.Spad;
        // the rotation table rows of ALL of the lane's row blocks up front: one round trip instead of one per row block behind the previous
        // block's stores (round 5)
        [[maybe_unused]] f32x4 rcs[MI][2], rsn[MI][2];
        if (ROPE_PRE && (kind & 2)) {
#pragma unroll
            for (int i = 0; i < MI; ++i) {
                const int m = mw + i * 32 + l31;
                const int s = (m < M ? m : M - 1) % S;
                rcs[i][0] = *reinterpret_cast<const f32x4*>(he.rope_cos + (size_t)s * 16 + 4 * half);
                rcs[i][1] = *reinterpret_cast<const f32x4*>(he.rope_cos + (size_t)s * 16 + 8 + 4 * half);
                rsn[i][0] = *reinterpret_cast<const f32x4*>(he.rope_sin + (size_t)s * 16 + 4 * half);
                rsn[i][1] = *reinterpret_cast<const f32x4*>(he.rope_sin + (size_t)s * 16 + 8 + 4 * half);
            }
        }
#pragma unroll
        for (int i = 0; i < MI; ++i) {
            const int m = mw + i * 32 + l31;
            const int mc = m < M ? m : M - 1;
            const int b = mc / S;
            const int s = mc - b * S;
            const int ob = (kind & 4) ? ((b * S) & 3) : 0;
            if constexpr (LNC) {         // LayerNorm fold (before the rotation: both are linear, this one is per channel)
                const float2 st = ln[i * 32 + l31];
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const f32x4 c1 = *reinterpret_cast<const f32x4*>(lc1 + j * 32 + q * 8 + 4 * half);
                        const f32x4 c2 = *reinterpret_cast<const f32x4*>(lc2 + j * 32 + q * 8 + 4 * half);
#pragma unroll
                        for (int e = 0; e < 4; ++e) acc[i][j][4 * q + e] = st.y * (acc[i][j][4 * q + e] - st.x * c1[e]) + c2[e];
                    }
            }
            if constexpr (QKN) {
                if (kind & 16) {   // qk_norm: the 64 channels of the lane's head row are its own 32 registers and those of lane ^ 32
                    float ss = 0.f;
#pragma unroll
                    for (int j = 0; j < 2; ++j)
#pragma unroll
                        for (int r = 0; r < 16; ++r) ss += acc[i][j][r] * acc[i][j][r];
                    unsigned a = __float_as_uint(ss), b = a;
                    half_swap(a, b);                   // a: the low half's sum in both halves, b: the high half's
                    const float inv = rsqrtf(fmaxf(__uint_as_float(a) + __uint_as_float(b), 1e-24f));      // 1 / max(|x|, 1e-12)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
#pragma unroll
                        for (int r = 0; r < 16; ++r) acc[i][j][r] *= inv;
                }
            }
            if (kind & 2) {   // partial RoPE on d < 32 (block j = 0): partner of d < 16 is d + 16 = register r + 8 of this lane
                if constexpr (!ROPE_PRE) {
                    rcs[i][0] = *reinterpret_cast<const f32x4*>(he.rope_cos + (size_t)s * 16 + 4 * half);
                    rcs[i][1] = *reinterpret_cast<const f32x4*>(he.rope_cos + (size_t)s * 16 + 8 + 4 * half);
                    rsn[i][0] = *reinterpret_cast<const f32x4*>(he.rope_sin + (size_t)s * 16 + 4 * half);
                    rsn[i][1] = *reinterpret_cast<const f32x4*>(he.rope_sin + (size_t)s * 16 + 8 + 4 * half);
                }
                const f32x4 cs0 = rcs[i][0], cs1 = rcs[i][1], sn0 = rsn[i][0], sn1 = rsn[i][1];
#pragma unroll
                for (int r = 0; r < 8; ++r) {
                    const float cs = (r < 4) ? cs0[r & 3] : cs1[r & 3];
                    const float sn = (r < 4) ? sn0[r & 3] : sn1[r & 3];
                    const float x1 = acc[i][0][r], x2 = acc[i][0][r + 8];
                    acc[i][0][r] = x1 * cs - x2 * sn;
                    acc[i][0][r + 8] = x2 * cs + x1 * sn;
                }
            }
            if (kind & 8) {   // query: pre-scaled for the attention kernel (one rounding, here)
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[i][j][r] *= he.qscale;
            }
            op_t* row = dst + ((size_t)(b * he.heads + head) * Spad + s + ob) * 64 + 8 * half;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                unsigned pk[8];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    pk[2 * q] = pack_op2(acc[i][j][4 * q], acc[i][j][4 * q + 1]);
                    pk[2 * q + 1] = pack_op2(acc[i][j][4 * q + 2], acc[i][j][4 * q + 3]);
                }
                half_swap(pk[0], pk[2]);
                half_swap(pk[1], pk[3]);
                half_swap(pk[4], pk[6]);
                half_swap(pk[5], pk[7]);
                if (qfrag) {       // fused cross-attention (MI == 1): channels [32 j + 8 half, +8) and [32 j + 16 + 8 half, +8) of the lane's row
                                   // ARE the B-operand fragments 2 j and 2 j + 1 of the score MFMA
#pragma unroll
                    for (int e = 0; e < 8; ++e) qfrag[j][e] = pk[e];
                    continue;
                }
                if (m < M) {
                    *reinterpret_cast<u32x4*>(row + j * 32) = u32x4{pk[0], pk[1], pk[2], pk[3]};
                    *reinterpret_cast<u32x4*>(row + j * 32 + 16) = u32x4{pk[4], pk[5], pk[6], pk[7]};
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// The two heads epilogues on 16 x 16 accumulator blocks (v_mfma_f32_16x16x32, the 12-wave tile: S16 in gemm_pipe_kernel), acc[i][j] = row
// block i, column block j of the wave's TM x 64 tile = one head.  The arithmetic and its order per element are those of gemm_epilogue_t /
// gemm_epilogue above; only which lane and register hold an element differs.
// ---------------------------------------------------------------------------------------------
// one dword of blocks j and j + 1 exchanged between the 16-lane rows of the wave (v_permlane16_swap: rows 1 and 3 of `a` against rows 0 and
// 2 of `b`): afterwards row 0 holds (a of row 0, a of row 1), row 1 (b of row 0, b of row 1), rows 2 and 3 the same of rows 2 and 3
__device__ __forceinline__ void row16_swap(unsigned& a, unsigned& b) {
    u32x2 r = __builtin_amdgcn_permlane16_swap(a, b, false, false);
    a = r[0];
    b = r[1];
}

// q / k (swapped operands, C^T): lane l & 15 owns TOKEN row m = mw + 16 i + (l & 15), its quarter qt = l >> 4 the channels 16 j + 4 qt + e.
// The rotation partner d + 16 of d < 16 is block 1 against block 0 in the same registers of the same lane; the table rows of all MB row
// blocks are fetched up front (8 registers each).  Rows of two sequences meet inside a row block, so position and key offset are per lane.
template <int MB, bool LNC>
__device__ __forceinline__ void gemm_heads16_t(const GemmArgs& g, f32x4 (&acc)[MB][4], const int mw, const int nw, const int lane,
                                               const float2* ln, const float* lc1, const float* lc2) {
    const int M = g.M;
    const int l15 = lane & 15, qt = lane >> 4;
    const HeadsEpi& he = g.heads;
    const int hp = he.heads * 64;
    const int part = nw / hp;
    const int head = (nw - part * hp) >> 6;
    const int kind = he.kind[part];
    op_t* __restrict__ dst = he.out[part];
    const int S = he.S, Spad = he.Spad;
    [[maybe_unused]] f32x4 rcs[MB], rsn[MB];
    if (kind & 2) {
#pragma unroll
        for (int i = 0; i < MB; ++i) {
            const int m = mw + i * 16 + l15;
            const int s = (m < M ? m : M - 1) % S;
            rcs[i] = *reinterpret_cast<const f32x4*>(he.rope_cos + (size_t)s * 16 + 4 * qt);
            rsn[i] = *reinterpret_cast<const f32x4*>(he.rope_sin + (size_t)s * 16 + 4 * qt);
        }
    }
    [[maybe_unused]] f32x4 c1[4], c2[4];
    if constexpr (LNC) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            c1[j] = *reinterpret_cast<const f32x4*>(lc1 + j * 16 + 4 * qt);
            c2[j] = *reinterpret_cast<const f32x4*>(lc2 + j * 16 + 4 * qt);
        }
    }
    // after the exchange a lane's two 16-byte runs are channels 16 (qt & 1) + 8 (qt >> 1) + [0, 8) of blocks 0 | 1 and of blocks 2 | 3
    // (measured and not kept: no exchange and four 8-byte stores per row block, 36.6 us against 36.3 for to_qkv in fp16, 35.5 against 35.2
    // in bf16.  Not built: W rows permuted at ld_ptr so that a block pair holds eight consecutive channels without an exchange -- the
    // rotation partner d + 16 would then sit in another lane quarter.)
    const int crun = 16 * (qt & 1) + 8 * (qt >> 1);
#pragma unroll
    for (int i = 0; i < MB; ++i) {
        const int m = mw + i * 16 + l15;
        const int mc = m < M ? m : M - 1;
        const int b = mc / S;
        const int s = mc - b * S;
        const int ob = (kind & 4) ? ((b * S) & 3) : 0;
        if constexpr (LNC) {         // LayerNorm fold (before the rotation: both are linear, this one is per channel)
            const float2 st = ln[i * 16 + l15];
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[i][j][e] = st.y * (acc[i][j][e] - st.x * c1[j][e]) + c2[j][e];
        }
        if (kind & 2) {   // partial RoPE on d < 32
            // x1 cs - x2 sn and x2 cs + x1 sn, with the roundings spelled out: which product of each sum is fused is the compiler's choice
            // in gemm_epilogue_t, and it is not the same for all of that epilogue's registers (r = 6, 7, the channels d = 10, 11, 14, 15,
            // get two products and an addition for the second sum).  The same forms here keep q and k bit-identical between the two MFMA
            // shapes (-DSAT_RING_MFMA_32X32); without them about one rotated element in 10^4 differs by an ulp.
#pragma clang fp contract(off)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float cs = rcs[i][e], sn = rsn[i][e];
                const float x1 = acc[i][0][e], x2 = acc[i][1][e];
                const float t = x2 * cs;
                float hi = __builtin_fmaf(x1, sn, t);
                if (e >= 2) {
                    const float u = x1 * sn;
                    hi = qt >= 2 ? t + u : hi;
                }
                acc[i][0][e] = __builtin_fmaf(x1, cs, -(x2 * sn));
                acc[i][1][e] = hi;
            }
        }
        if (kind & 8) {   // query: pre-scaled for the attention kernel (one rounding, here)
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[i][j][e] *= he.qscale;
        }
        op_t* row = dst + ((size_t)(b * he.heads + head) * Spad + s + ob) * 64 + crun;
#pragma unroll
        for (int jp = 0; jp < 2; ++jp) {
            unsigned a0 = pack_op2(acc[i][2 * jp][0], acc[i][2 * jp][1]), a1 = pack_op2(acc[i][2 * jp][2], acc[i][2 * jp][3]);
            unsigned b0 = pack_op2(acc[i][2 * jp + 1][0], acc[i][2 * jp + 1][1]), b1 = pack_op2(acc[i][2 * jp + 1][2], acc[i][2 * jp + 1][3]);
            row16_swap(a0, b0);
            row16_swap(a1, b1);
            if (m < M) *reinterpret_cast<u32x4*>(row + jp * 32) = u32x4{a0, a1, b0, b1};
        }
    }
}

// V^T (un-swapped): lane l & 15 owns CHANNEL column 16 j + (l & 15) of block j, its registers the token rows 16 i + 4 (l >> 4) + r: four
// consecutive tokens = one 8-byte store into the token-contiguous destination, with its key permutation (vt_pos) and key offset, exactly
// as the 32 x 32 epilogue writes it.  Pads are not touched (the forward's memset owns them).
template <int MB, bool LNC>
__device__ __forceinline__ void gemm_heads16_vt(const GemmArgs& g, f32x4 (&acc)[MB][4], const int mw, const int nw, const int lane,
                                                const float2* ln, const float* lc1, const float* lc2) {
    const int M = g.M;
    const int l15 = lane & 15, qt = lane >> 4;
    const HeadsEpi& he = g.heads;
    const int hp = he.heads * 64;
    const int part = nw / hp;
    const int head = (nw - part * hp) >> 6;
    const int kind = he.kind[part];
    op_t* __restrict__ dst = he.out[part];
    const int S = he.S, Spad = he.Spad;
    const bool shift = (kind & 4) != 0;
    [[maybe_unused]] float c1[4], c2[4];
    if constexpr (LNC) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            c1[j] = lc1[j * 16 + l15];
            c2[j] = lc2[j * 16 + l15];
        }
    }
#pragma unroll
    for (int i = 0; i < MB; ++i) {
        const int mb = mw + i * 16 + 4 * qt;          // first of 4 consecutive rows, multiple of 4
        float v[4][4];          // [column block][row]
        int bb[4], ss[4];
        f32x4 st01 = {0.f, 1.f, 0.f, 1.f}, st23 = {0.f, 1.f, 0.f, 1.f};      // (mean, rstd) of rows e = 0,1 / 2,3
        if constexpr (LNC) {
            const f32x4* sp = reinterpret_cast<const f32x4*>(ln + i * 16 + 4 * qt);
            st01 = sp[0];
            st23 = sp[1];
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            int mm = mb + e;
            mm = mm < M ? mm : M - 1;
            bb[e] = mm / S;
            ss[e] = mm - bb[e] * S;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                v[j][e] = acc[i][j][e];
                if constexpr (LNC) {
                    const float mean = e < 2 ? st01[2 * e] : st23[2 * e - 4];
                    const float rstd = e < 2 ? st01[2 * e + 1] : st23[2 * e - 3];
                    v[j][e] = rstd * (v[j][e] - mean * c1[j]) + c2[j];
                }
            }
            if (kind & 2) {   // wave-uniform: partial RoPE on d < 32, the partner d + 16 is block 1 of the same lane
                const float cs = he.rope_cos[ss[e] * 16 + l15], sn = he.rope_sin[ss[e] * 16 + l15];
                const float x1 = v[0][e], x2 = v[1][e];
                v[0][e] = x1 * cs - x2 * sn;
                v[1][e] = x2 * cs + x1 * sn;
            }
        }
        if (mb + 3 < M && bb[0] == bb[3]) {
            const int ob = shift ? ((bb[0] * S) & 3) : 0;
            const size_t hbase = ((size_t)(bb[0] * he.heads + head) * 64) * Spad;
            const size_t base = hbase + vt_pos(ss[0] + ob);         // aligned group of 4 keys: stays a group of 4
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                opx4 p;
#pragma unroll
                for (int e = 0; e < 4; ++e) p[e] = f32_to_op(v[j][e]);
                if (shift) {     // aligned: (ss[0] + ob) % 4 == mb % 4 == 0
                    *reinterpret_cast<opx4*>(dst + base + (size_t)(j * 16 + l15) * Spad) = p;
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) dst[hbase + vt_pos(ss[0] + e) + (size_t)(j * 16 + l15) * Spad] = p[e];
                }
            }
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (mb + e < M) {
                    const int ob = shift ? ((bb[e] * S) & 3) : 0;
                    const size_t base = ((size_t)(bb[e] * he.heads + head) * 64) * Spad + vt_pos(ss[e] + ob);
#pragma unroll
                    for (int j = 0; j < 4; ++j) dst[base + (size_t)(j * 16 + l15) * Spad] = f32_to_op(v[j][e]);
                }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// fp32 output / residual epilogue staged through LDS (un-swapped orientation, wave tile TM x 64).  Each wave writes one
// 32 x 64 fp32 block of its accumulators into a private 8 KiB LDS region (row-major, ds_write_b32: the 32 lanes of a half cover
// one 128-byte row segment, conflict-free) and reads it back as 16-byte pieces of whole rows, so that the read-modify-write of
// the residual stream becomes 8 + 8 fully coalesced 16-byte accesses per block (4 rows x 256 contiguous bytes per instruction)
// instead of 32 + 32 dword accesses.  The LDS ring is free at that point (the caller passes a barrier after the last K-tile).
// ---------------------------------------------------------------------------------------------
// PRE: the residual values were loaded at kernel start (`pre`, MI == 1 only): their HBM / L2 latency is then hidden behind
// the whole K loop instead of sitting between the last MFMA and the first store.
// The accumulators of the 32 x 64 row block i of a wave tile -> the wave's staging block ([32][64] floats), for the two MFMA shapes of
// the ring tiles.  32 x 32 x 16: lane = column l & 31 of column block j, register r = row (r & 3) + 8 (r >> 2) + 4 (l >> 5).
template <int MI>
__device__ __forceinline__ void stage_rows32(float* ep, const f32x16 (&acc)[MI][2], const int i, const int lane) {
    const int half = lane >> 5, l31 = lane & 31;
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) ep[((r & 3) + 8 * (r >> 2) + 4 * half) * 64 + j * 32 + l31] = acc[i][j][r];
}
// 16 x 16 x 32 (un-swapped: the activation rows are the MFMA's A operand), blocks [2 i + rb][cb]: lane = column l & 15 of column block
// cb, register r = row 4 (l >> 4) + r of row block rb.  As many dword stores as above.  (Swapped operands would give one 16-byte store
// per block, but a 16-byte store is served in groups of 8 consecutive lanes and those would hold 8 rows of one column, 256 bytes
// apart: an 8-way bank conflict.  Here lanes l and l + 16 of a 32-lane group share a bank, 2-way, which is the 4 cycles the store's
// register transfer takes anyway.)
template <int MB>
__device__ __forceinline__ void stage_rows32(float* ep, const f32x4 (&acc)[MB][4], const int i, const int lane) {
    const int l15 = lane & 15, q = lane >> 4;
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int cb = 0; cb < 4; ++cb)
#pragma unroll
            for (int r = 0; r < 4; ++r) ep[(rb * 16 + 4 * q + r) * 64 + cb * 16 + l15] = acc[2 * i + rb][cb][r];
}

template <int MI, bool PRE = false, typename Acc>
__device__ __forceinline__ void gemm_epilogue_f32_staged(const GemmArgs& g, Acc& acc, float* ep, const int mw, const int nw,
                                                         const int lane, const f32x4* pre = nullptr) {
    const int M = g.M;
    const int prow = lane >> 4;            // row of this lane inside a 4-row pass
    const int c4 = (lane & 15) * 4;        // first of its 4 columns
    const bool accum = g.accumulate != 0;
    const f32x4 bia = g.bias ? *reinterpret_cast<const f32x4*>(g.bias + nw + c4) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < MI; ++i) {
        stage_rows32(ep, acc, i, lane);
#pragma unroll
        for (int grp = 0; grp < 2; ++grp) {     // two batches of four passes: 16 registers of residual values in flight
            f32x4 old[4];
#pragma unroll
            for (int p4 = 0; p4 < 4; ++p4) {
                const int m = mw + i * 32 + (grp * 4 + p4) * 4 + prow;
                if constexpr (PRE) old[p4] = pre[grp * 4 + p4];
                else old[p4] = (accum && m < M) ? *reinterpret_cast<const f32x4*>(g.C + (size_t)m * g.ldc + nw + c4) : f32x4{0.f, 0.f, 0.f, 0.f};
            }
#pragma unroll
            for (int p4 = 0; p4 < 4; ++p4) {
                const int row = (grp * 4 + p4) * 4 + prow;
                const int m = mw + i * 32 + row;
                f32x4 v = *reinterpret_cast<const f32x4*>(ep + row * 64 + c4) + bia;
                if (m < M && g.gate) v *= *reinterpret_cast<const f32x4*>(g.gate + (size_t)(m / g.gate_rows) * g.gate_ld + nw + c4);
                v += old[p4];
                if (m < M) *reinterpret_cast<f32x4*>(g.C + (size_t)m * g.ldc + nw + c4) = v;
                if (g.xb) {
                    // LayerNorm fold, producer side (wave-uniform test): bf16 image of the updated row piece + the statistics of the
                    // ROUNDED values over this wave's 64-column block (the 16 lanes of a DPP row hold one row of the pass)
                    opx4 xr;
                    float sum = 0.f, sq = 0.f;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        xr[e] = f32_to_op(v[e]);
                        const float f = op_to_f32(xr[e]);
                        sum += f;
                        sq += f * f;
                    }
                    sum = row16_sum(sum);
                    sq = row16_sum(sq);
                    if (m < M) {
                        *reinterpret_cast<opx4*>(g.xb + (size_t)m * g.N + nw + c4) = xr;
                        if ((lane & 15) == 0)
                            *reinterpret_cast<float2*>(g.ln_part_out + ((size_t)m * (g.N >> 6) + (nw >> 6)) * 2) = make_float2(sum, sq);
                    }
                }
            }
        }
    }
}

template <int BM, int BN, int WM, int WN, int EPIX>
__global__ __launch_bounds__(WM * WN * 64) void gemm_kernel(GemmArgs g) {
    sat_f16_saturate();
    constexpr int EPI = EpiOf<EPIX>::EPI;
    constexpr bool QKN = EpiOf<EPIX>::QKN;
    constexpr int NT = WM * WN * 64;
    constexpr int TM = BM / WM;
    constexpr int TN = BN / WN;
    static_assert(TN == 64, "wave tile is TM x 64");
    constexpr int MI = TM / 32;
    constexpr int NI = 2;
    constexpr int A_CH = BM * 8 / NT;
    constexpr int B_CH = BN * 8 / NT;
    static_assert(A_CH >= 1 && B_CH >= 1, "tile too small for the block");
    constexpr int STAGE_BYTES = (BM + BN) * 128;

    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wm = wave / WN;
    const int wn = wave % WN;
    const int half = lane >> 5;
    const int l31 = lane & 31;

    const int M = g.M, N = g.N, K = g.K;
    const int tiles_m = (M + BM - 1) / BM;
    const int tiles_n = N / BN;
    const int bid = xcd_remap(blockIdx.x, gridDim.x);
    int tm, tn;
    if (tiles_m <= tiles_n) {   // M is the short dimension: m fastest, W panels stay in one XCD's L2
        tn = bid / tiles_m;
        tm = bid - tn * tiles_m;
    } else {
        tm = bid / tiles_n;
        tn = bid - tm * tiles_n;
    }
    const int m0 = tm * BM;
    const int n0 = tn * BN;

    const op_t* __restrict__ A = g.A;
    const op_t* __restrict__ W = g.W;

    // per-thread staging coordinates
    int a_row[A_CH], a_chk[A_CH];
    const op_t* a_ptr[A_CH];
#pragma unroll
    for (int i = 0; i < A_CH; ++i) {
        int id = i * NT + tid;
        a_row[i] = id >> 3;
        a_chk[i] = id & 7;
        int gm = m0 + a_row[i];
        gm = gm < M ? gm : M - 1;
        a_ptr[i] = A + (size_t)gm * K + a_chk[i] * 8;
    }
    int b_row[B_CH], b_chk[B_CH];
    const op_t* b_ptr[B_CH];
#pragma unroll
    for (int i = 0; i < B_CH; ++i) {
        int id = i * NT + tid;
        b_row[i] = id >> 3;
        b_chk[i] = id & 7;
        b_ptr[i] = W + (size_t)(n0 + b_row[i]) * K + b_chk[i] * 8;
    }

    f32x16 acc[MI][NI];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    u32x4 ra[A_CH], rb[B_CH];
    auto gload = [&](int kt) {
#pragma unroll
        for (int i = 0; i < A_CH; ++i) ra[i] = *reinterpret_cast<const u32x4*>(a_ptr[i] + kt * 64);
#pragma unroll
        for (int i = 0; i < B_CH; ++i) rb[i] = *reinterpret_cast<const u32x4*>(b_ptr[i] + kt * 64);
    };
    auto lstore = [&](int stage) {
        char* sa = smem + stage * STAGE_BYTES;
        char* sb = sa + BM * 128;
#pragma unroll
        for (int i = 0; i < A_CH; ++i) *reinterpret_cast<u32x4*>(sa + lds_tile_off(a_row[i], a_chk[i])) = ra[i];
#pragma unroll
        for (int i = 0; i < B_CH; ++i) *reinterpret_cast<u32x4*>(sb + lds_tile_off(b_row[i], b_chk[i])) = rb[i];
    };

    auto compute = [&](int stage) {
        const char* sa = smem + stage * STAGE_BYTES;
        const char* sb = sa + BM * 128;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            opx8 af[MI], bfr[NI];
#pragma unroll
            for (int i = 0; i < MI; ++i)
                af[i] = *reinterpret_cast<const opx8*>(sa + lds_tile_off(wm * TM + i * 32 + l31, ks * 2 + half));
#pragma unroll
            for (int j = 0; j < NI; ++j)
                bfr[j] = *reinterpret_cast<const opx8*>(sb + lds_tile_off(wn * TN + j * 32 + l31, ks * 2 + half));
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int j = 0; j < NI; ++j)
                    acc[i][j] = mfma_32x32x16(af[i], bfr[j], acc[i][j]);
        }
    };

    // register-staged double buffer, one barrier per K-tile; the last tile is peeled so that the
    // staging registers are written/read unconditionally (keeps them out of scratch)
    const int nk = K / 64;
    gload(0);
    lstore(0);
    __syncthreads();
    for (int kt = 0; kt < nk - 1; ++kt) {
        gload(kt + 1);
        compute(kt & 1);
        lstore((kt + 1) & 1);
        __syncthreads();
    }
    compute((nk - 1) & 1);

    gemm_epilogue<EPI, MI, NI, false, QKN>(g, acc, m0 + wm * TM, n0 + wn * TN, half, l31);
}

// ---------------------------------------------------------------------------------------------
// Direct-to-LDS variant: tiles are staged with global_load_lds_dwordx4 (LDS-DMA, no VGPR round
// trip, no ds_write pass).  The LDS image is the same XOR-swizzled one; because an LDS-DMA writes
// wave-uniform base + lane*16, the swizzle is applied to the per-lane SOURCE address (guide
// section 5.4 rule 21): lane l of the piece that covers rows 8p..8p+7 lands at row 8p + l/8,
// position l%8, so it fetches logical chunk (l%8) ^ ((row>>1)&7) of that row.
// ---------------------------------------------------------------------------------------------
template <int BM, int BN, int WM, int WN, int EPIX>
__global__ __launch_bounds__(WM * WN * 64) void gemm_glds_kernel(GemmArgs g) {
    sat_f16_saturate();
    constexpr int EPI = EpiOf<EPIX>::EPI;
    constexpr bool QKN = EpiOf<EPIX>::QKN;
    constexpr int NT = WM * WN * 64;
    constexpr int TM = BM / WM;
    constexpr int TN = BN / WN;
    static_assert(TN == 64, "wave tile is TM x 64");
    constexpr int MI = TM / 32;
    constexpr int NI = 2;
    constexpr int A_CH = BM * 8 / NT;
    constexpr int B_CH = BN * 8 / NT;
    constexpr int STAGE_BYTES = (BM + BN) * 128;

    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN;
    const int wn = wave % WN;
    const int half = lane >> 5;
    const int l31 = lane & 31;

    const int M = g.M, N = g.N, K = g.K;
    const int tiles_m = (M + BM - 1) / BM;
    const int tiles_n = N / BN;
    const int bid = xcd_remap(blockIdx.x, gridDim.x);
    int tm, tn;
    if (tiles_m <= tiles_n) {
        tn = bid / tiles_m;
        tm = bid - tn * tiles_m;
    } else {
        tm = bid / tiles_n;
        tn = bid - tm * tiles_n;
    }
    const int m0 = tm * BM;
    const int n0 = tn * BN;

    // per-lane source pointers (swizzle folded in); LDS destinations are wave-uniform
    const op_t* a_ptr[A_CH];
#pragma unroll
    for (int i = 0; i < A_CH; ++i) {
        int q = i * NT + tid;
        int row = q >> 3, pos = q & 7;
        int c = pos ^ ((row >> 1) & 7);
        int gm = m0 + row;
        gm = gm < M ? gm : M - 1;
        a_ptr[i] = g.A + (size_t)gm * K + c * 8;
    }
    const op_t* b_ptr[B_CH];
#pragma unroll
    for (int i = 0; i < B_CH; ++i) {
        int q = i * NT + tid;
        int row = q >> 3, pos = q & 7;
        int c = pos ^ ((row >> 1) & 7);
        b_ptr[i] = g.W + (size_t)(n0 + row) * K + c * 8;
    }

    f32x16 acc[MI][NI];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    auto stage_in = [&](int kt, int stage) {
        char* sa = smem + stage * STAGE_BYTES;
        char* sb = sa + BM * 128;
#pragma unroll
        for (int i = 0; i < A_CH; ++i)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(a_ptr[i] + kt * 64),
                                             (__attribute__((address_space(3))) void*)(sa + (i * NT + wave * 64) * 16), 16, 0, 0);
#pragma unroll
        for (int i = 0; i < B_CH; ++i)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(b_ptr[i] + kt * 64),
                                             (__attribute__((address_space(3))) void*)(sb + (i * NT + wave * 64) * 16), 16, 0, 0);
    };
    auto compute = [&](int stage) {
        const char* sa = smem + stage * STAGE_BYTES;
        const char* sb = sa + BM * 128;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            opx8 af[MI], bfr[NI];
#pragma unroll
            for (int i = 0; i < MI; ++i)
                af[i] = *reinterpret_cast<const opx8*>(sa + lds_tile_off(wm * TM + i * 32 + l31, ks * 2 + half));
#pragma unroll
            for (int j = 0; j < NI; ++j)
                bfr[j] = *reinterpret_cast<const opx8*>(sb + lds_tile_off(wn * TN + j * 32 + l31, ks * 2 + half));
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int j = 0; j < NI; ++j)
                    acc[i][j] = mfma_32x32x16(af[i], bfr[j], acc[i][j]);
        }
    };

    const int nk = K / 64;
    stage_in(0, 0);
    __syncthreads();          // hipcc emits s_waitcnt vmcnt(0) in front of the barrier while an LDS-DMA is in flight
    for (int kt = 0; kt < nk - 1; ++kt) {
        stage_in(kt + 1, (kt + 1) & 1);
        compute(kt & 1);
        __syncthreads();
    }
    compute((nk - 1) & 1);

    gemm_epilogue<EPI, MI, NI, false, QKN>(g, acc, m0 + wm * TM, n0 + wn * TN, half, l31);
}

// ---------------------------------------------------------------------------------------------
// Deep-prefetch variant: NS-stage LDS ring filled by LDS-DMA, prefetch distance NS-1, ONE raw
// s_barrier per K-tile and COUNTED s_waitcnt vmcnt (never 0 in steady state) so that NS-2 tiles
// stay in flight across every barrier (guide T3+T4).  This is what hides the L2/HBM -> LDS latency
// when only one workgroup fits a CU (B=1: 204..432 workgroups on 256 CUs).
//   iteration k:  wait(tile k landed) ; barrier ; issue tile k+NS-1 -> stage (k-1)%NS ; compute k
// BK = 64: 128-byte rows of 8 chunks, the image of lds_tile_off.  Every constant of a tile is a member of RingGeom (gemm_ring_geom.h),
// which the launcher reads as well; the pieces are those of gemm_ring.h.
// ---------------------------------------------------------------------------------------------
// (The ablation modes of rounds 1-2 -- no LDS-DMA / no ds_read / no barrier / no epilogue builds of this kernel -- are in the git
// history at 9661dcc; what they measured is in profiles/r01_gemm_ablation.txt, r02_gemm_ablation.txt.)
// FP8: A and W are e4m3 bytes.  The launcher hands the kernel K/2 "bf16 columns", so staging, LDS layout and swizzle are
// byte-for-byte those of the bf16 kernel (128-B rows now hold 128 k); a 16-B fragment is two 8-byte MFMA operands:
// v_mfma_f32_32x32x16_fp8_fp8 runs at the bf16 rate, but every LDS / L2 / HBM byte carries twice the k.
// KG = 2 (round 4, fp32 output): TWO K-groups of WM x WN waves work on the same BM x BN tile, group g on the k-half g of every
// 2 x BK slice (its own A / W rows in the stage), and exchange half of their partial sums through LDS at the end -- each group then
// finishes 32 of its waves' 64 rows with the 32 x 64 staged epilogue.  A one-round launch (<= one tile per CU) gets 8 waves of 64 x 64
// per CU instead of 8 waves of 32 x 64: a third less LDS fragment traffic per MFMA, which is what bounds the narrow tiles
// (profiles/r04_narrow_tiles_negative.txt: two co-resident 4-wave workgroups of 64 x 64 waves beat the 8-wave tile by 17-21 % wherever
// there are two workgroups per CU; at one prompt there is only one).
// (Measured and not kept, profiles/r04_kgroup_tile.txt: four PRODUCER waves -- one per SIMD, two per K-group -- that issue all of the LDS-DMA while the eight
// MFMA waves never touch the vector-memory queue.  Bit-identical results, FF-out 66.5 us against 53.7: the CU's vector-memory path takes one 1-KiB piece per
// ~16 clocks whoever issues it, and with a two-stage ring the issue of tile k + 1 can only start at boundary k and has to land by boundary k + 1 -- sixteen
// pieces in a row per producer wave stretch that chain, eight per wave in parallel with the MFMAs do not.  The ablation without any DMA runs 36.9 us.)
// DIL ("DMA in loop", bf16 / fp16 operands): the iteration's LDS-DMA pieces are issued inside compute(), behind the MFMAs of the first k-steps, instead of
// in front of it -- always on with K-groups; a per-tile choice otherwise (SatTile::dil, gemm_tiles.h)
template <int BM, int BN, int BK, int WM, int WN, int NS, int EPIX, int FP8 = 0, int KG = 1, bool DIL = false>
__global__ __launch_bounds__(KG * WM * WN * 64) void gemm_pipe_kernel(GemmArgs g) {
    sat_f16_saturate();
    using G = RingGeom<BM, BN, BK, WM, WN, NS, EPIX, FP8, KG, DIL>;
    constexpr int EPI = G::EPI, NT = G::NT, TM = G::TM, TN = G::TN, MI = G::MI, NI = G::NI, MB = G::MB, NW = G::NW, WLG = G::WLG, LPT = G::LPT;
    constexpr int ROWB = G::ROWB, SCALE_WAVES = G::SCALE_WAVES, GROUP_BYTES = G::GROUP_BYTES, STAGE_BYTES = G::STAGE_BYTES, D = G::D;
    constexpr int NDIL = G::NDIL, DIL_STEPS = G::DIL_STEPS, DIL_PER = G::DIL_PER, ORI = G::ORI;
    constexpr bool QKN = G::QKN, S16 = G::S16, UNIFORM = G::UNIFORM, MXA = G::MXA, DIL_ON = G::DIL_ON, LN_CONS = G::LN_CONS, PRE_RESID = G::PRE_RESID;

    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int grp = KG == 2 ? wave / (WM * WN) : 0;           // K-group
    const int wv = KG == 2 ? wave % (WM * WN) : wave;
    const int wm = wv / WN;
    const int wn = wv % WN;
    const int half = lane >> 5;
    const int l31 = lane & 31;

    const int M = g.M, N = g.N, K = g.K;
    const int tiles_m = (M + BM - 1) / BM;
    const int tiles_n = N / BN;
    const int bid = xcd_remap(blockIdx.x, gridDim.x);
    int tm, tn;
    if (tiles_m <= tiles_n) {
        tn = bid / tiles_m;
        tm = bid - tn * tiles_m;
    } else {
        tm = bid / tiles_n;
        tn = bid - tm * tiles_n;
    }
    const int m0 = tm * BM;
    const int n0 = tn * BN;
    // waves whose TM rows lie entirely beyond M (the M-tail tile: 2 valid rows of 256 at B=1) keep staging tiles and
    // joining barriers but skip their LDS reads, MFMAs and epilogue
    const bool wave_rows_valid = (m0 + wm * TM) < M;
    // Fused cross-attention (HeadsEpi::xa_k, 128 x 64 tile: one head per workgroup column, one 32-query block per wave): the K / V^T
    // tiles of the (sequence, kv-head) go to LDS behind the ring and the LayerNorm constants NOW -- they are the oldest entries of the
    // vector-memory queue, so every counted vmcnt wait of the K loop still holds, and the loop's barriers publish them.
    constexpr bool XA_OK = G::XA_OK;
    constexpr int XA_OFF = G::XA_OFF;
    [[maybe_unused]] bool xa_on = false;
    [[maybe_unused]] auto xa_stage = [&](int b) { xattn_stage_kv(g.heads, smem + XA_OFF, b, n0, wave, lane); };
    if constexpr (XA_OK) {
        xa_on = g.heads.xa_k != nullptr;
        if (xa_on) xa_stage(m0 / g.heads.S);
    }
    // fp32 residual epilogue of the small tiles (one 32-row block per wave, registers to spare): fetch the residual values NOW.
    // They are the oldest entries of the vector-memory queue, so every counted vmcnt wait of the K loop still holds.
    // K-groups: the 32 rows this wave finishes
    const int epi_m = m0 + wm * TM + (KG == 2 ? grp * 32 : 0);
    const bool epi_rows_valid = KG == 2 ? epi_m < M : wave_rows_valid;
    [[maybe_unused]] f32x4 resid[PRE_RESID ? 8 : 1];
    if constexpr (PRE_RESID) {
        const bool want = g.accumulate != 0 && epi_rows_valid;
#pragma unroll
        for (int ps = 0; ps < 8; ++ps) {
            const int m = epi_m + ps * 4 + (lane >> 4);
            resid[ps] = (want && m < M) ? *reinterpret_cast<const f32x4*>(g.C + (size_t)m * g.ldc + n0 + wn * TN + (lane & 15) * 4)
                                        : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }

    // LayerNorm fold, consumer side: mean and 1/std of the BM rows of this tile from the producer's per-block partial sums, into
    // LDS behind the ring (filled right after the prologue's LDS-DMA below, read by the epilogue).
    // LDS behind the ring: (mean, 1/std) of the BM rows, then the BN (c1, c2) pairs of this tile's output channels
    [[maybe_unused]] float2* lnst = reinterpret_cast<float2*>(smem + G::LN_OFF);
    [[maybe_unused]] float* lnc = reinterpret_cast<float*>(smem + G::LN_OFF + BM * 8);      // c1[BN] then c2[BN]
    const op_t* ld_ptr[LPT];
#pragma unroll
    for (int i = 0; i < LPT; ++i) {
        const int L = KG == 2 ? grp * WLG + i * (WM * WN) + wv : i * NW + wave;               // wave-uniform; K-groups: a group stages its own rows
        const int lg = KG == 2 ? grp : 0;
        const int Lg = KG == 2 ? i * (WM * WN) + wv : L;
        const bool is_a = Lg < G::WL_A;
        int q = (is_a ? Lg : Lg - G::WL_A) * 64 + lane;
        int row = q / G::CPR, pos = q % G::CPR;
        int c = pos ^ ((row >> 1) & 7);
        int gm = m0 + row;
        gm = gm < M ? gm : M - 1;
        int gn = n0 + row;
        gn = gn < N ? gn : N - 1;                  // only reachable by the unused slot of a short wave
        ld_ptr[i] = (is_a ? g.A + (size_t)gm * K + c * 8 : g.W + (size_t)gn * K + c * 8) + lg * BK;
    }
    const bool wave_full = UNIFORM || wave < G::N_FULL;
    [[maybe_unused]] const unsigned* sc_ptr = nullptr;
    if constexpr (MXA) {
        int gm = m0 + wave * 64 + lane;
        gm = gm < M ? gm : M - 1;
        sc_ptr = g.a_bscale + (size_t)gm * (K / BK);      // [M][K/128 bytes] dwords; K counts 16-bit columns here
    }

    f32x16 acc[MI][NI];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    // 16 x 16 x 32 builds (S16): MB 16-row blocks x four 16-column blocks instead (acc is dead there)
    [[maybe_unused]] f32x4 acc16[MB][4];
#pragma unroll
    for (int i = 0; i < MB; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc16[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    // The stager.  THE issue site of the ring's LDS-DMA pieces: piece i of K-tile kt, from ld_ptr[i] to this wave's i-th wave-load slot of
    // the stage at `sa`.  stage_in, the in-loop issues of the two 16-bit fragment loops and a ragged tile's extra piece all go through it,
    // and wait_steady below counts what it puts into the vector-memory queue.
    auto issue = [&](int i, int kt, char* sa) {
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(ld_ptr[i] + kt * (BK * KG)),
                                         (__attribute__((address_space(3))) void*)(sa + (KG == 2 ? grp * WLG + i * (WM * WN) + wv : i * NW + wave) * 1024), 16, 0, 0);
    };
    auto stage_in = [&](int kt, int stage) {
        char* sa = smem + stage * STAGE_BYTES;
#pragma unroll
        for (int i = 0; i < LPT; ++i)
            if (UNIFORM || i + 1 < LPT || wave_full) issue(i, kt, sa);
        if constexpr (MXA) {
            if (wave < SCALE_WAVES)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(sc_ptr + kt),
                                                 (__attribute__((address_space(3))) void*)(sa + (BM + BN) * ROWB + wave * 256), 4, 0, 0);
        }
    };
    // tiles k+1..k+D-1 may stay in flight: this wave issued LPT (or LPT-1) loads for each of them
    [[maybe_unused]] auto wait_steady = [&]() {
        if constexpr (MXA && D > 1) {
            if (wave < SCALE_WAVES) wait_vmcnt<(D - 1) * (LPT + 1)>();
            else wait_vmcnt<(D - 1) * LPT>();
        } else if constexpr (UNIFORM || D == 1) {
            wait_vmcnt<(D - 1) * LPT>();
        } else {
            if (wave_full) wait_vmcnt<(D - 1) * LPT>();
            else wait_vmcnt<(D - 1) * (LPT - 1)>();
        }
    };
    // fragments are double-buffered across the k-steps: the ds_reads of step ks+1 are issued BEFORE the MFMAs of
    // step ks, so the wave waits with a counted lgkmcnt and LDS latency hides behind the matrix pipe
    typedef long i64x2 __attribute__((ext_vector_type(2)));
    // TRc: operands swapped -> acc holds C^T (lane = token row), see gemm_epilogue_t
    auto compute = [&](int stage, auto trc, [[maybe_unused]] int kt_issue = -1, [[maybe_unused]] int st_issue = 0) {
        constexpr bool TRc = decltype(trc)::value;
        const char* sa = smem + stage * STAGE_BYTES + grp * GROUP_BYTES;
        const char* sb = sa + BM * ROWB;
        constexpr int KS = BK / 16;
        if constexpr (FP8 >= 2) {
            // v_mfma_scale_f32_32x32x64_f8f6f4: twice the MFMA rate of bf16 / plain fp8.  One instruction consumes 64 k = two scale
            // blocks of 32.  Measured layout (tools/mx_probe.cpp): the FIRST 16 bytes of every lane belong to block 0, the LAST 16 to
            // block 1, and block g takes its E8M0 scale from the lanes of half g.  So lane (row, half) loads the 16-byte chunks
            // `half` and `2 + half` of the 64-byte step (k = half*16.. and 32 + half*16..), identically for A and W.
            typedef int i32x8 __attribute__((ext_vector_type(8)));
            constexpr int KS2 = BK / 32;               // 64-byte steps per 128-byte row
            i32x8 af[2][MI], bfr[2][NI];
            auto frag = [&](int ks, int buf) {
#pragma unroll
                for (int i = 0; i < MI; ++i) {
                    const int row = wm * TM + i * 32 + l31;
                    u32x4 lo = *reinterpret_cast<const u32x4*>(sa + lds_tile_off(row, ks * 4 + half));
                    u32x4 hi = *reinterpret_cast<const u32x4*>(sa + lds_tile_off(row, ks * 4 + 2 + half));
                    af[buf][i] = i32x8{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
                }
#pragma unroll
                for (int j = 0; j < NI; ++j) {
                    const int row = wn * TN + j * 32 + l31;
                    u32x4 lo = *reinterpret_cast<const u32x4*>(sb + lds_tile_off(row, ks * 4 + half));
                    u32x4 hi = *reinterpret_cast<const u32x4*>(sb + lds_tile_off(row, ks * 4 + 2 + half));
                    bfr[buf][j] = i32x8{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
                }
            };
            // 16-wave workgroups have 128 VGPRs per lane: 64 accumulators + one set of 32-byte fragments (32) fit, two sets do not;
            // four waves per SIMD cover the fragment-read latency instead
            constexpr bool DBUF = NT < 1024;
            // MXFP8 A: dword of this row's four E8M0 block scales of the K-tile, shifted so that byte 0 / byte 2 are the blocks this
            // lane half feeds in 64-byte step 0 / 1 (block = 2 * step + half)
            [[maybe_unused]] int sdw[MI];
            if constexpr (MXA) {
                const char* ssc = sb + BN * ROWB;
#pragma unroll
                for (int i = 0; i < MI; ++i)
                    sdw[i] = (int)(*reinterpret_cast<const unsigned*>(ssc + (wm * TM + i * 32 + l31) * 4) >> (8 * half));
            }
            auto mx = [&](const i32x8& af_, const i32x8& bf_, f32x16 c_, int ks, int i) -> f32x16 {
                if constexpr (MXA) {
                    static_assert(!TRc, "MXFP8 A operand: block scales were probed on the A side only (tools/mx_probe.cpp)");
                    if (ks == 0) return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(af_, bf_, c_, 0, 0, 0, sdw[i], 0, 0x7F7F7F7F);
                    return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(af_, bf_, c_, 0, 0, 2, sdw[i], 0, 0x7F7F7F7F);
                } else if constexpr (TRc) {
                    return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(bf_, af_, c_, 0, 0, 0, 0x7F7F7F7F, 0, 0x7F7F7F7F);
                } else {
                    return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(af_, bf_, c_, 0, 0, 0, 0x7F7F7F7F, 0, 0x7F7F7F7F);
                }
            };
            if constexpr (!DBUF) {
#pragma unroll
                for (int ks = 0; ks < KS2; ++ks) {
                    frag(ks, 0);
#pragma unroll
                    for (int i = 0; i < MI; ++i)
#pragma unroll
                        for (int j = 0; j < NI; ++j)
                            acc[i][j] = mx(af[0][i], bfr[0][j], acc[i][j], ks, i);
                }
                return;
            }
            frag(0, 0);
            __builtin_amdgcn_sched_group_barrier(0x100, 2 * (MI + NI), 0);
#pragma unroll
            for (int ks = 0; ks < KS2; ++ks) {
                if (ks + 1 < KS2) frag(ks + 1, (ks + 1) & 1);
#pragma unroll
                for (int i = 0; i < MI; ++i)
#pragma unroll
                    for (int j = 0; j < NI; ++j)
                        acc[i][j] = mx(af[ks & 1][i], bfr[ks & 1][j], acc[i][j], ks, i);
                constexpr int NR = 2 * (MI + NI), NM = MI * NI;
                if (ks + 1 < KS2) sched_reads_behind_mfmas<NR, NM, NR / NM>();
                else sched_mfmas_only<NM>();
            }
            return;
        }
        if constexpr (FP8 == 1) {
            // fragment step ks = 32 k (two MFMAs): lane (row, half) holds bytes half*16 .. +15 of it, the first 8 feed one MFMA and
            // the last 8 the next -- A and W use the same k permutation, so the dot product is unchanged
            i64x2 af[2][MI], bfr[2][NI];
            auto frag = [&](int ks, int buf) {
#pragma unroll
                for (int i = 0; i < MI; ++i)
                    af[buf][i] = *reinterpret_cast<const i64x2*>(sa + lds_tile_off(wm * TM + i * 32 + l31, ks * 2 + half));
#pragma unroll
                for (int j = 0; j < NI; ++j)
                    bfr[buf][j] = *reinterpret_cast<const i64x2*>(sb + lds_tile_off(wn * TN + j * 32 + l31, ks * 2 + half));
            };
            frag(0, 0);
            __builtin_amdgcn_sched_group_barrier(0x100, MI + NI, 0);
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                if (ks + 1 < KS) frag(ks + 1, (ks + 1) & 1);
#pragma unroll
                for (int h2 = 0; h2 < 2; ++h2)
#pragma unroll
                    for (int i = 0; i < MI; ++i)
#pragma unroll
                        for (int j = 0; j < NI; ++j)
                            acc[i][j] = TRc ? __builtin_amdgcn_mfma_f32_32x32x16_fp8_fp8(bfr[ks & 1][j][h2], af[ks & 1][i][h2], acc[i][j], 0, 0, 0)
                                            : __builtin_amdgcn_mfma_f32_32x32x16_fp8_fp8(af[ks & 1][i][h2], bfr[ks & 1][j][h2], acc[i][j], 0, 0, 0);
                if (ks + 1 < KS) sched_reads_behind_mfmas<MI + NI, 2 * MI * NI>();
                else sched_mfmas_only<2 * MI * NI>();
            }
            return;
        }
        if constexpr (S16) {
            // v_mfma_f32_16x16x32: a step is 32 k = four 16-byte chunks of the row, lane (row l & 15, chunk l >> 4) -- the fragment the
            // 8-phase kernel reads from the same image (gemm_ph8.hip), conflict-free under the row-pair XOR.  Per step MB + 4 reads feed
            // 4 MB MFMAs of 16 matrix-pipe cycles: the reads, cycles and registers per k of the 32 x 32 x 16 loop below, in half as many steps.
            // TRc (heads, q / k): operands swapped, a block holds C^T -- lane l & 15 owns a token row, quarter l >> 4 four consecutive
            // channels of each 16-column block (gemm_heads16_t)
            static_assert(!TRc || EPI == EPI_HEADS, "16 x 16 x 32: fp32 output is un-swapped");
            constexpr int KS2 = BK / 32, NR = MB + 4, NM = MB * 4;
            const int l15 = lane & 15, q = lane >> 4;
            opx8 af[2][MB], bfr[2][4];
            auto frag = [&](int ks, int buf) {
#pragma unroll
                for (int i = 0; i < MB; ++i)
                    af[buf][i] = *reinterpret_cast<const opx8*>(sa + lds_tile_off(wm * TM + i * 16 + l15, ks * 4 + q));
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    bfr[buf][j] = *reinterpret_cast<const opx8*>(sb + lds_tile_off(wn * TN + j * 16 + l15, ks * 4 + q));
            };
            frag(0, 0);
            __builtin_amdgcn_sched_group_barrier(0x100, NR, 0);
#pragma unroll
            for (int ks = 0; ks < KS2; ++ks) {
                if (ks + 1 < KS2) frag(ks + 1, (ks + 1) & 1);
                if constexpr (KG == 2) {          // the iteration's LDS-DMA pieces ride in the MFMA stream of the first step (DIL_STEPS)
                    if (ks < DIL_STEPS && kt_issue >= 0) {
                        char* sdst = smem + st_issue * STAGE_BYTES;
#pragma unroll
                        for (int i = ks * DIL_PER; i < (ks + 1) * DIL_PER && i < NDIL; ++i) issue(i, kt_issue, sdst);
                    }
                }
#pragma unroll
                for (int i = 0; i < MB; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        acc16[i][j] = TRc ? mfma_16x16x32(bfr[ks & 1][j], af[ks & 1][i], acc16[i][j])
                                          : mfma_16x16x32(af[ks & 1][i], bfr[ks & 1][j], acc16[i][j]);
                // the pinned interleave, the patterns of the 32 x 32 x 16 loop re-counted in MFMAs of half the length
                if constexpr (KG == 2) {
                    if (ks + 1 < KS2) {
                        // the next step's reads behind the first two MFMAs (the same ~100 cycles of head start), then the iteration's DMA
                        // pieces two at a time through the rest of the step, which is the half in front of the mid-iteration barrier
                        // (measured and not kept: one read behind each of the first eight MFMAs, 51.9 us against 50.7 on FF-out; reads
                        // and pieces together behind the first eight, 54.6)
                        sched_reads_behind_mfmas<NR, 2, NR / 2>();
                        if (DIL_PER == 8 && NM == 16) {
                            sched_mfmas_only<1>();
                            sched_dma_pairs_behind_mfmas<4, 2>();
                            sched_mfmas_only<1>();
                        } else {
                            sched_mfmas_only<NM - 2>();
                        }
                    } else {
                        sched_mfmas_only<NM>();
                    }
                    if (ks == KS2 / 2 - 1) kgroup_mid_barrier();
                } else if (ks + 1 < KS2) {
                    // one read of the next step's fragments behind each of the first MFMAs
                    // (measured on the 12-wave heads tile and not kept: two reads behind each of the first four MFMAs, 37.2 us against 36.3
                    // for to_qkv in fp16, 35.8 against 35.2 in bf16)
                    sched_reads_behind_mfmas<NR, NM>();
                } else {
                    sched_mfmas_only<NM>();
                }
            }
            return;
        }
        opx8 af[2][MI], bfr[2][NI];
        auto frag = [&](int ks, int buf) {
#pragma unroll
            for (int i = 0; i < MI; ++i)
                af[buf][i] = *reinterpret_cast<const opx8*>(sa + lds_tile_off(wm * TM + i * 32 + l31, ks * 2 + half));
#pragma unroll
            for (int j = 0; j < NI; ++j)
                bfr[buf][j] = *reinterpret_cast<const opx8*>(sb + lds_tile_off(wn * TN + j * 32 + l31, ks * 2 + half));
        };
        frag(0, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, MI + NI, 0);        // the first fragments: DS reads only
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            if (ks + 1 < KS) frag(ks + 1, (ks + 1) & 1);
            if constexpr (DIL_ON) {
                // the iteration's LDS-DMA pieces ride in the MFMA stream of the first k-steps -- in front of the first MFMA they cost their
                // issue time, 60-180 cycles a piece
                if (ks < DIL_STEPS && kt_issue >= 0) {
                    char* sdst = smem + st_issue * STAGE_BYTES;
#pragma unroll
                    for (int i = ks * DIL_PER; i < (ks + 1) * DIL_PER && i < NDIL; ++i) issue(i, kt_issue, sdst);
                }
            }
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int j = 0; j < NI; ++j)
                    acc[i][j] = TRc ? mfma_32x32x16(bfr[ks & 1][j], af[ks & 1][i], acc[i][j])
                                    : mfma_32x32x16(af[ks & 1][i], bfr[ks & 1][j], acc[i][j]);
            // pin the interleave: one ds_read of the NEXT step's fragments behind each MFMA of this step
            if (ks + 1 < KS) {
                constexpr int NR = MI + NI, NM = MI * NI;
                if constexpr (KG == 2) {
                    // (measured on the 12-wave 256 x 192 tile as well: 42.9-43.4 us against 41.1-41.5 for one read per MFMA -- three waves per SIMD
                    // cover the trailing read, two do not)
                    // all of the next step's fragment reads behind the FIRST MFMA: they get three MFMAs (~100 cycles) of head start on the
                    // wait in front of the next step instead of one read trailing the last MFMA
                    sched_reads_behind_mfmas<NR, 1, NR>();
                    if (ks < KS / 2 && DIL_PER == 4) {
                        sched_dma_pairs_behind_mfmas<2, 0>();
                        sched_mfmas_only<1>();
                    } else {
                        sched_mfmas_only<NM - 1>();
                    }
                } else {
                    sched_reads_behind_mfmas<NR, NM>();
                    if (DIL_ON && ks < DIL_STEPS) __builtin_amdgcn_sched_group_barrier(0x20, DIL_PER, 0);          // this step's DMA pieces behind its MFMAs
                }
            } else {
                sched_mfmas_only<MI * NI>();
            }
            if constexpr (KG == 2) {
                if (ks == KS / 2 - 1) kgroup_mid_barrier();
            }
        }
    };

    const int nk = K / (BK * KG);
    // prologue: tiles 0..D-1 in flight (nk >= D is guaranteed by the launcher)
#pragma unroll
    for (int s = 0; s < D; ++s) stage_in(s, s);
    // (after the prologue's LDS-DMA: the constants' global-memory round trip overlaps the first tiles' instead of preceding it; the
    // K loop's barriers order these LDS writes before the epilogue's reads)
    if constexpr (LN_CONS) {
        // Without the fold the same epilogue runs on (mean, rstd) = (0, 1), c1 = 0, c2 = bias.
        const bool ln_fold = g.ln_part != nullptr;
        // TPR threads per row, each summing every TPR-th partial pair (independent loads, one round trip), combined with DPP
        constexpr int TPR = (NT / BM >= 4) ? 4 : (NT / BM >= 2 ? 2 : 1);
        const int np = K >> 6;
        const int r = tid / TPR, sub = tid % TPR;
        float sum = 0.f, sq = 0.f;
        if (ln_fold && r < BM) {
            int m = m0 + r;
            m = m < M ? m : M - 1;
            const float2* pp = reinterpret_cast<const float2*>(g.ln_part) + (size_t)m * np;
#pragma unroll 6
            for (int i = sub; i < np; i += TPR) {
                const float2 v = pp[i];
                sum += v.x;
                sq += v.y;
            }
        }
        if constexpr (TPR >= 2) {
            sum += dpp_move<0xB1>(sum);
            sq += dpp_move<0xB1>(sq);
        }
        if constexpr (TPR >= 4) {
            sum += dpp_move<0x4E>(sum);
            sq += dpp_move<0x4E>(sq);
        }
        if (r < BM && sub == 0) {
            const float inv_k = 1.0f / (float)K;
            const float mean = sum * inv_k;
            const float var = fmaxf(sq * inv_k - mean * mean, 0.f);
            lnst[r] = ln_fold ? make_float2(mean, rsqrtf(var + g.ln_eps)) : make_float2(0.f, 1.f);
        }
        // the last 2 BN / 4 threads bring in the channel constants, 16 bytes each
        const int ct = NT - 1 - tid;
        if (ct < BN / 2) {
            const bool first = ct < BN / 4;
            const float* src = ln_fold ? (first ? g.ln_c1 + n0 + ct * 4 : g.ln_c2 + n0 + (ct - BN / 4) * 4)
                                       : ((first || !g.bias) ? nullptr : g.bias + n0 + (ct - BN / 4) * 4);
            *reinterpret_cast<f32x4*>(lnc + ct * 4) = src ? *reinterpret_cast<const f32x4*>(src) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }

    int rd = 0;          // stage of tile k
    int wr = D;          // stage that receives tile k+D (== stage of tile k-1)
    // steady state: tiles k+1..k+D-1 stay in flight across the barrier
    // Orientation (per wave: a 64-column wave tile never straddles a q / k / v part, a workgroup's 192 columns may -- the two loops pass the
    // same barriers): transposed accumulators everywhere except
    // for a V^T destination (token-contiguous stores want lane = channel), the MXFP8 A operand and the fp32 output.
    // Measured (profiles/r02_epilogue_ab.txt): bf16 outputs gain 3-4 % (SwiGLU) / 13 % (heads) from the transposed orientation, the
    // fp32 residual epilogue LOSES 6-10 % at 8 prompts (a lane-per-token store instruction touches 32 cache lines; in the legacy
    // orientation every store instruction writes two full 128-byte lines) -> fp32 output stays un-swapped.
    // fp32 output therefore always takes the LDS-staged epilogue: to_out at one prompt 21.5 us staged / 22.8 direct dword stores / 23.1 transposed,
    // at 8 prompts 101 / 106 / 119 (profiles/r02_f32_epilogue_and_tile_quantisation.txt).
    // The orientation is fixed at compile time wherever it can be (ORI 0: un-swapped only -- fp32 output, MXFP8 A operand;
    // 1: transposed only -- SwiGLU; 2: per workgroup -- heads: q / k transposed, V^T un-swapped): one main loop instead of two keeps
    // the 128-VGPR kernels (16 waves, e4m3 fragments) out of scratch.
    bool tr = ORI != 0;
    if constexpr (EPI == EPI_HEADS) {
        const int hp = g.heads.heads * 64;
        tr = tr && !(g.heads.kind[(n0 + wn * TN) / hp] & 1);
    }
    auto main_loop = [&](auto trc) {
        // K-groups: a group stages and reads only its own rows, so every barrier only has to hold for the group -- group 1 runs half an
        // iteration behind group 0 (one barrier more up front, one less at the end; compute() passes one in mid-iteration), and on every
        // SIMD one wave is inside its MFMA stream while the other waits for its tile, issues the next and reads its first fragments
        if (KG == 2 && grp == 1) __builtin_amdgcn_s_barrier();
        for (int k = 0; k < nk - D; ++k) {
            wait_steady();
            __builtin_amdgcn_s_barrier();
            if constexpr (DIL_ON) {
                if (wave_rows_valid) {
                    if constexpr (!UNIFORM) {          // the extra piece of the first waves of a ragged tile
                        if (wave_full) issue(LPT - 1, k + D, smem + wr * STAGE_BYTES);
                    }
                    compute(rd, trc, k + D, wr);
                } else {
                    stage_in(k + D, wr);
                    if (KG == 2) __builtin_amdgcn_s_barrier();
                }
            } else {
                stage_in(k + D, wr);
                if (wave_rows_valid) compute(rd, trc);
                else if (KG == 2) __builtin_amdgcn_s_barrier();
            }
            rd = (rd + 1 == NS) ? 0 : rd + 1;
            wr = (wr + 1 == NS) ? 0 : wr + 1;
        }
        // drain: nothing left to issue
        for (int k = nk - D; k < nk; ++k) {
            wait_vmcnt<0>();
            __builtin_amdgcn_s_barrier();
            if (wave_rows_valid) compute(rd, trc);
            else if (KG == 2) __builtin_amdgcn_s_barrier();
            rd = (rd + 1 == NS) ? 0 : rd + 1;
        }
        if (KG == 2 && grp == 0) __builtin_amdgcn_s_barrier();
    };
    if constexpr (ORI == 0) {
        main_loop(std::false_type{});
    } else if constexpr (ORI == 1) {
        main_loop(std::true_type{});
    } else {
        if (tr) main_loop(std::true_type{});
        else main_loop(std::false_type{});
    }

    if constexpr (XA_OK) {
        if (xa_on) {
            const HeadsEpi& he = g.heads;
            unsigned qp[2][8];
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int e = 0; e < 8; ++e) qp[j][e] = 0u;
            if (wave_rows_valid) gemm_epilogue_t<EPI, MI, NI, LN_CONS, true, QKN>(g, acc, m0 + wm * TM, n0, half, l31, lnst + wm * TM, lnc, lnc + BN, qp);
            opx8 qf[4];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                qf[2 * j] = __builtin_bit_cast(opx8, u32x4{qp[j][0], qp[j][1], qp[j][2], qp[j][3]});
                qf[2 * j + 1] = __builtin_bit_cast(opx8, u32x4{qp[j][4], qp[j][5], qp[j][6], qp[j][7]});
            }
            const int S = he.S;
            const int m = m0 + wm * TM + l31;
            const int b_me = (m < M ? m : M - 1) / S;
            const int last = (m0 + BM - 1 < M ? m0 + BM - 1 : M - 1);
            const int b_lo = m0 / S, b_hi = last / S;
            const int wlast = (m0 + wm * TM + 31 < M ? m0 + wm * TM + 31 : M - 1);
            const int w_lo = (m0 + wm * TM) / S, w_hi = wlast / S;
            for (int bb = b_lo; bb <= b_hi; ++bb) {
                if (bb > b_lo) {        // the tile's rows straddle two sequences: second pass on the next sequence's keys
                    __builtin_amdgcn_s_barrier();
                    xa_stage(bb);
                    wait_vmcnt<0>();
                    __builtin_amdgcn_s_barrier();
                }
                if (!(wave_rows_valid && w_lo <= bb && bb <= w_hi)) continue;
                const int ob = (bb * he.xa_sk) & 3, k_end = ob + he.xa_sk;
                const int n_t = (k_end + 63) >> 6;
                attn::State<2> st;
                st.init(half);
                for (int t = 0; t < n_t; ++t) {
                    const char* sk = smem + XA_OFF + t * 16384;
                    const bool edge = (t == 0 && ob != 0) || (t == n_t - 1 && (k_end & 63) != 0);
                    attn::tile<2>(st, qf, sk, sk + 8192, edge, t * 64, ob, k_end, t == 0, 1.0f, l31, half);
                }
                const float inv = 1.0f / attn::half_sum(st.l_run);
                op_t* op = he.xa_out + (size_t)m * ((size_t)he.heads * 64) + n0 + 8 * half;      // out row = b * S + s = m
#pragma unroll
                for (int db = 0; db < 2; ++db) {
                    unsigned pk[8];
#pragma unroll
                    for (int rq = 0; rq < 4; ++rq) {
                        pk[2 * rq] = pack_op2(st.oacc[db][rq * 4] * inv, st.oacc[db][rq * 4 + 1] * inv);
                        pk[2 * rq + 1] = pack_op2(st.oacc[db][rq * 4 + 2] * inv, st.oacc[db][rq * 4 + 3] * inv);
                    }
                    half_swap(pk[0], pk[2]);            // 8 consecutive channels per lane: 16-byte stores
                    half_swap(pk[1], pk[3]);
                    half_swap(pk[4], pk[6]);
                    half_swap(pk[5], pk[7]);
                    if (m < M && b_me == bb) {
                        *reinterpret_cast<u32x4*>(op + db * 32) = u32x4{pk[0], pk[1], pk[2], pk[3]};
                        *reinterpret_cast<u32x4*>(op + db * 32 + 16) = u32x4{pk[4], pk[5], pk[6], pk[7]};
                    }
                }
            }
            return;
        }
    }
    if constexpr (FP8 != 0) {
        // dequantise: per-token scale of A x per-output-channel scale of W (kept out of the last K-tile's MFMA schedule)
        __builtin_amdgcn_sched_barrier(0);
        if (wave_rows_valid) {
            if (tr) {      // lane = token row, registers = channels 8*(r>>2) + 4*half + (r&3)
#pragma unroll
                for (int i = 0; i < MI; ++i) {
                    int row = m0 + wm * TM + i * 32 + l31;
                    row = row < M ? row : M - 1;
                    const float sa_r = g.a_scale[row];
#pragma unroll
                    for (int j = 0; j < NI; ++j)
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const f32x4 sw = *reinterpret_cast<const f32x4*>(g.w_scale + n0 + wn * TN + j * 32 + q * 8 + 4 * half);
#pragma unroll
                            for (int e = 0; e < 4; ++e) acc[i][j][4 * q + e] *= sa_r * sw[e];
                        }
                }
            } else {
                float sw[NI];
#pragma unroll
                for (int j = 0; j < NI; ++j) sw[j] = g.w_scale[n0 + wn * TN + j * 32 + l31];
#pragma unroll
                for (int i = 0; i < MI; ++i)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        int row = m0 + wm * TM + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                        row = row < M ? row : M - 1;
                        const float sa_r = MXA ? 1.0f : g.a_scale[row];
#pragma unroll
                        for (int j = 0; j < NI; ++j) acc[i][j][r] *= sa_r * sw[j];
                    }
            }
        }
    }
    if constexpr (KG == 2) {
        // exchange: group 0 keeps row block 0 of its 64 x 64 wave tile and sends block 1, group 1 the other way round; lane-contiguous
        // dwords, 8 KiB per wave in the first half of the (free) ring, the staged epilogue's areas in the second half
        __builtin_amdgcn_s_barrier();
        if constexpr (S16) {
            // the same split by 32-row block, in 16 x 16 blocks: rows 0-31 are acc16[0..1], rows 32-63 acc16[2..3]; lane-contiguous 16 bytes
            f32x4* mine = reinterpret_cast<f32x4*>(smem) + wave * 512;
#pragma unroll
            for (int rb = 0; rb < 2; ++rb)
#pragma unroll
                for (int cb = 0; cb < 4; ++cb) {
                    f32x4 v;
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = grp ? acc16[rb][cb][e] : acc16[2 + rb][cb][e];
                    mine[(rb * 4 + cb) * 64 + lane] = v;
                }
            __syncthreads();
            const f32x4* theirs = reinterpret_cast<const f32x4*>(smem) + (wave ^ (WM * WN)) * 512;
            f32x4 fin[2][4];
#pragma unroll
            for (int rb = 0; rb < 2; ++rb)
#pragma unroll
                for (int cb = 0; cb < 4; ++cb) {
                    const f32x4 t = theirs[(rb * 4 + cb) * 64 + lane];
#pragma unroll
                    for (int e = 0; e < 4; ++e) fin[rb][cb][e] = (grp ? acc16[2 + rb][cb][e] : acc16[rb][cb][e]) + t[e];
                }
            if (epi_rows_valid)
                gemm_epilogue_f32_staged<1, true>(g, fin, reinterpret_cast<float*>(smem + G::KG_STAGING_OFF) + wave * 2048, epi_m, n0 + wn * TN, lane, resid);
            return;
        }
        float* mine = reinterpret_cast<float*>(smem) + wave * 2048;
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) mine[(j * 16 + r) * 64 + lane] = grp ? acc[0][j][r] : acc[1][j][r];
        __syncthreads();
        const float* theirs = reinterpret_cast<const float*>(smem) + (wave ^ (WM * WN)) * 2048;
        f32x16 fin[1][2];
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) fin[0][j][r] = (grp ? acc[1][j][r] : acc[0][j][r]) + theirs[(j * 16 + r) * 64 + lane];
        if (epi_rows_valid)
            gemm_epilogue_f32_staged<1, true>(g, fin, reinterpret_cast<float*>(smem + G::KG_STAGING_OFF) + wave * 2048, epi_m, n0 + wn * TN, lane, resid);
        return;
    }
    if constexpr (EPI == EPI_F32) {
        __builtin_amdgcn_s_barrier();       // every wave is done reading the ring: it becomes the staging area
        if (wave_rows_valid) {
            if constexpr (S16 && PRE_RESID)
                gemm_epilogue_f32_staged<MI, true>(g, acc16, reinterpret_cast<float*>(smem) + wave * 2048, m0 + wm * TM, n0 + wn * TN, lane, resid);
            else if constexpr (S16)
                gemm_epilogue_f32_staged<MI>(g, acc16, reinterpret_cast<float*>(smem) + wave * 2048, m0 + wm * TM, n0 + wn * TN, lane);
            else if constexpr (PRE_RESID)
                gemm_epilogue_f32_staged<MI, true>(g, acc, reinterpret_cast<float*>(smem) + wave * 2048, m0 + wm * TM, n0 + wn * TN, lane, resid);
            else
                gemm_epilogue_f32_staged<MI>(g, acc, reinterpret_cast<float*>(smem) + wave * 2048, m0 + wm * TM, n0 + wn * TN, lane);
        }
    } else if constexpr (S16) {
        if (wave_rows_valid) {
            if (tr) gemm_heads16_t<MB, LN_CONS>(g, acc16, m0 + wm * TM, n0 + wn * TN, lane, lnst + wm * TM, lnc + wn * TN, lnc + BN + wn * TN);
            else gemm_heads16_vt<MB, LN_CONS>(g, acc16, m0 + wm * TM, n0 + wn * TN, lane, lnst + wm * TM, lnc + wn * TN, lnc + BN + wn * TN);
        }
    } else if (wave_rows_valid) {
        if (tr) gemm_epilogue_t<EPI, MI, NI, LN_CONS, (NT < 1024), QKN>(g, acc, m0 + wm * TM, n0 + wn * TN, half, l31, lnst + wm * TM, lnc + wn * TN, lnc + BN + wn * TN);
        else gemm_epilogue<EPI, MI, NI, LN_CONS, QKN>(g, acc, m0 + wm * TM, n0 + wn * TN, half, l31, lnst + wm * TM, lnc + wn * TN, lnc + BN + wn * TN);
    }
}

template <int BM, int BN, int BK, int WM, int WN, int NS, int EPIX, int FP8 = 0, int KG = 1, bool DIL = false>
int launch_pipe(const GemmArgs& a, hipStream_t stream) {
    using G = RingGeom<BM, BN, BK, WM, WN, NS, EPIX, FP8, KG, DIL>;          // the launch's NT, LDS bytes and what the build supports
    SAT_CHECK_ARG(G::LN_CONS || !a.ln_part, SAT_E_UNSUPPORTED, "gemm: LayerNorm fold needs bf16 operands and a SwiGLU / heads epilogue");
    SAT_CHECK_ARG((!a.xb && !a.ln_part_out) || (G::EPI == EPI_F32 && FP8 == 0 && a.xb && a.ln_part_out), SAT_E_UNSUPPORTED,
                  "gemm: the bf16 image / row statistics come from the bf16 fp32-output tiles with 64-column wave tiles");
    auto kern = gemm_pipe_kernel<BM, BN, BK, WM, WN, NS, EPIX, FP8, KG, DIL>;
    // fused cross-attention (HeadsEpi::xa_k): three K / V^T tiles of 64 keys behind the ring and the LayerNorm constants (G::XA_LDS)
    bool xa = false;
    if constexpr (G::EPI == EPI_HEADS) {
        xa = a.heads.xa_k != nullptr;
        if (xa) {
            const HeadsEpi& he = a.heads;
            SAT_CHECK_ARG(G::XA_OK, SAT_E_UNSUPPORTED, "gemm: the fused cross-attention epilogue lives in the 128 x 64 tile (variant 16)");
            SAT_CHECK_ARG(he.parts == 1 && (he.kind[0] & ~16) == 8 && he.qscale == SAT_ATTN_QSCALE && he.xa_vt && he.xa_out && he.xa_kvh > 0 &&
                              he.heads % he.xa_kvh == 0 && he.xa_sk > 0 && he.xa_sk + 3 <= 192 && he.xa_sk_pad >= he.xa_sk + 3 && he.xa_sk_pad % 64 == 0,
                          SAT_E_UNSUPPORTED, "gemm: fused cross-attention needs one pre-scaled row-major part and at most 189 keys (got %d)", he.xa_sk);
        }
    }
    SAT_TRY(sat_ensure_dynamic_lds(reinterpret_cast<const void*>(kern), G::XA_LDS));
    GemmArgs b = a;
    if (FP8) {
        SAT_CHECK_ARG(a.K % 128 == 0 && a.w_scale && (FP8 == 3 ? (const void*)a.a_bscale : (const void*)a.a_scale), SAT_E_UNSUPPORTED,
                      "gemm(fp8): K=%d must be a multiple of 128 and both scale vectors given", a.K);
        b.K = a.K / 2;       // the kernel counts 16-bit columns: 128-byte LDS rows = 128 e4m3
    }
    SAT_CHECK_ARG(b.N % BN == 0, SAT_E_UNSUPPORTED, "gemm: N=%d not a multiple of the %d-column tile", b.N, BN);
    SAT_CHECK_ARG(b.K % (BK * KG) == 0 && b.K / (BK * KG) >= NS, SAT_E_UNSUPPORTED, "gemm: K=%d too small for the %d-stage pipeline", a.K, NS);
    int tiles = cdiv(b.M, BM) * (b.N / BN);
    hipLaunchKernelGGL(kern, dim3(tiles), dim3(G::NT), xa ? G::XA_LDS : G::LDS, stream, b);
    SAT_LAUNCH_CHECK();
    return 0;
}

template <int BM, int BN, int WM, int WN, int EPI, bool GLDS = false>
int launch_cfg(const GemmArgs& a, hipStream_t stream) {
    constexpr int NT = WM * WN * 64;
    constexpr int LDS = 2 * (BM + BN) * 128;
    SAT_CHECK_ARG(!a.ln_part && !a.xb && !a.ln_part_out, SAT_E_UNSUPPORTED, "gemm: LayerNorm fold is built into the pipelined tiles only (K >= 192)");
    auto kern = GLDS ? gemm_glds_kernel<BM, BN, WM, WN, EPI> : gemm_kernel<BM, BN, WM, WN, EPI>;
    SAT_TRY(sat_ensure_dynamic_lds(reinterpret_cast<const void*>(kern), LDS));
    SAT_CHECK_ARG(a.N % BN == 0, SAT_E_UNSUPPORTED, "gemm: N=%d not a multiple of the %d-column tile", a.N, BN);
    int tiles = cdiv(a.M, BM) * (a.N / BN);
    hipLaunchKernelGGL(kern, dim3(tiles), dim3(NT), LDS, stream, a);
    SAT_LAUNCH_CHECK();
    return 0;
}

// tile id (the table in gemm_tiles.h) -> the template instantiation; F8 = e4m3 flavour of the operands (0: 16-bit)
template <int ID, int EPI, int F8>
int launch_tile(const GemmArgs& a, hipStream_t stream) {
    constexpr SatTile t = sat_tile_geom(ID);
    static_assert(!t.f32_only || EPI == EPI_F32, "tile built for the fp32-output epilogue only");
    if constexpr (t.family == SAT_GEMM_PIPE) return launch_pipe<t.bm, t.bn, t.bk, t.wm, t.wn, t.ns, EPI, F8, t.kg, t.dil && F8 == 0>(a, stream);
    else return launch_cfg<t.bm, t.bn, t.wm, t.wn, EPI, t.family == SAT_GEMM_DMA2>(a, stream);
}

// The ring tiles that are BUILT for (epilogue, operand flavour): sat_gemm_route hands out no others.
template <int EPI, int F8>
int launch_epi(int tile, const GemmArgs& a, hipStream_t stream) {
#define SAT_TILE_CASE(id) \
    case id: return launch_tile<id, EPI, F8>(a, stream);
    switch (tile) {
        SAT_TILE_CASE(SAT_TILE_128)
        SAT_TILE_CASE(SAT_TILE_128x64)
        SAT_TILE_CASE(SAT_TILE_256)
        SAT_TILE_CASE(SAT_TILE_256x192)
    }
    if constexpr (F8 == 0) {
        switch (tile) {
            SAT_TILE_CASE(SAT_TILE_REF_128)
            SAT_TILE_CASE(SAT_TILE_DMA_128)
        }
        if constexpr (EPI == EPI_F32) {
            switch (tile) {
                SAT_TILE_CASE(SAT_TILE_128_DEEP)
                SAT_TILE_CASE(SAT_TILE_128_KGROUP)
            }
        }
        if constexpr (EPI == EPI_HEADS || EPI == EPI_HEADS_QKN) {
            switch (tile) { SAT_TILE_CASE(SAT_TILE_128x64_XATTN) }
        }
    }
#undef SAT_TILE_CASE
    sat_set_error("gemm: tile %d is not built for epilogue %d, operand flavour %d", tile, EPI, F8);
    return SAT_E_INVALID;
}

template <int EPI>
int launch_flavour(const GemmRoute& r, const GemmArgs& a, hipStream_t stream) {
    switch (r.e4m3) {
        case 0: return launch_epi<EPI, 0>(r.tile, a, stream);
#ifndef SAT_OPERAND_F16          // e4m3 operands ride in the bf16 build (sat_launch_gemm rejects f16 && fp8): the fp16 build does not instantiate them
        case 1: return launch_epi<EPI, 1>(r.tile, a, stream);
        case 2: return launch_epi<EPI, 2>(r.tile, a, stream);      // block-scaled MFMA with unit scales: 2x the MFMA rate
        case 3:                                                      // MXFP8 A operand (hardware block scales), fp32 output only: FF-out, to_out
            if constexpr (EPI == EPI_F32) return launch_epi<EPI, 3>(r.tile, a, stream);
            break;
#endif
    }
    sat_set_error("gemm: no e4m3 flavour %d of epilogue %d in this build", r.e4m3, EPI);
    return SAT_E_INVALID;
}

}  // namespace

#ifdef SAT_OPERAND_F16
// entry of the fp16 build for the bf16 build's dispatcher (GemmArgs differs only in the pointer element type)
int sat_launch_gemm_f16(int epi, const void* gemm_args, hipStream_t stream) {
    return f16::sat_launch_gemm(epi, *static_cast<const f16::GemmArgs*>(gemm_args), stream);
}
#endif

int SAT_OPNS::sat_launch_gemm(int epi, const GemmArgs& a, hipStream_t stream) {
#ifndef SAT_OPERAND_F16
    if (a.f16) return sat_launch_gemm_f16(epi, &a, stream);
#else
    SAT_CHECK_ARG(a.f16, SAT_E_INVALID, "gemm: bf16 operands handed to the fp16 build");
#endif
    SAT_CHECK_ARG(a.A && a.W, SAT_E_INVALID, "gemm: null operand");
    SAT_CHECK_ARG(!a.f16 || !a.fp8, SAT_E_UNSUPPORTED, "gemm: e4m3 operands ride in the bf16 build (fp8 mode keeps bf16 for everything else)");
    SAT_CHECK_ARG(a.M > 0 && a.N > 0 && a.K > 0, SAT_E_INVALID, "gemm: bad shape %d %d %d", a.M, a.N, a.K);
    SAT_CHECK_ARG(a.K % (a.fp8 ? 128 : 64) == 0, SAT_E_UNSUPPORTED, "gemm: K=%d must be a multiple of %d", a.K, a.fp8 ? 128 : 64);
    SAT_CHECK_ARG(a.N % 128 == 0, SAT_E_UNSUPPORTED, "gemm: N=%d must be a multiple of 128", a.N);
    // the epilogues move 16 bytes per lane
    SAT_CHECK_ARG((((uintptr_t)a.bias | (uintptr_t)a.C | (uintptr_t)a.H | (uintptr_t)a.gate | (uintptr_t)a.w_scale) & 15) == 0 && a.ldc % 4 == 0 &&
                      a.gate_ld % 4 == 0,
                  SAT_E_INVALID, "gemm: bias / output / gate / scale pointers must be 16-byte aligned and ldc a multiple of 4");
    SAT_CHECK_ARG(!a.ln_part || (a.ln_c1 && a.ln_c2 && a.ln_eps > 0.f && !a.bias && !a.fp8 && a.K % 64 == 0 &&
                                 (((uintptr_t)a.ln_part | (uintptr_t)a.ln_c1 | (uintptr_t)a.ln_c2) & 15) == 0),
                  SAT_E_INVALID, "gemm: LayerNorm fold needs ln_c1 / ln_c2 / ln_eps, no separate bias (it is part of ln_c2), 16-byte aligned vectors");
    SAT_CHECK_ARG((((uintptr_t)a.xb | (uintptr_t)a.ln_part_out) & 15) == 0, SAT_E_INVALID, "gemm: xb / ln_part_out must be 16-byte aligned");
    // what runs is decided by sat_gemm_route (gemm_tiles.h) from these integers and flags alone
    const int cus = sat_device_cus();
    GemmShape s{};
    s.M = a.M; s.N = a.N; s.K = a.K; s.variant = a.variant; s.fp8 = a.fp8;
    s.h8 = a.H8 != nullptr; s.ln_part = a.ln_part != nullptr; s.gate = a.gate != nullptr;
    s.heads = a.heads.heads; s.xattn = a.heads.xa_k != nullptr;
    s.slab_ok = cus > 0 && a.slab && a.slab_bytes >= (size_t)cus * 65536 * sizeof(float);
    s.e4m3_built = !SAT_OP_IS_F16;
    // qk_norm (HeadsEpi::kind bit 4) is built into the ring tiles' heads epilogues: tile policy 22 keeps the 8-phase kernel out of the choice
    const bool qkn = epi == EPI_HEADS && ((a.heads.kind[0] | a.heads.kind[1] | a.heads.kind[2]) & 16);
    if (qkn) {
        SAT_CHECK_ARG(!a.fp8, SAT_E_UNSUPPORTED, "gemm: qk_norm with e4m3 operands is not built");
        for (int pt = 0; pt < a.heads.parts; ++pt)
            SAT_CHECK_ARG(!(a.heads.kind[pt] & 16) || !(a.heads.kind[pt] & 1), SAT_E_UNSUPPORTED, "gemm: qk_norm on a transposed destination");
        s.variant = (a.variant & ~(7 << SAT_TILE_POLICY_SHIFT)) | sat_tile_policy_bits(22);
    }
    // EPI_ACT16 is built into the ring tiles' SwiGLU kernels and routed as they are, with the 8-phase kernel out of the choice (as qk_norm)
    const bool act16 = epi == EPI_ACT16;
    if (act16) {
        SAT_CHECK_ARG(!a.fp8 && !a.H8 && a.H && (a.act == 0 || a.act == 1), SAT_E_UNSUPPORTED, "gemm: the plain-activation epilogue takes 16-bit operands and writes a 16-bit H (act %d)", a.act);
        s.variant = (a.variant & ~(7 << SAT_TILE_POLICY_SHIFT)) | sat_tile_policy_bits(22);
    }
    const GemmRoute r = sat_gemm_route(act16 ? EPI_SWIGLU : epi, s, cus);
    switch (r.msg) {
        case SAT_ROUTE_OK: break;
        case SAT_ROUTE_UNKNOWN_EPI: sat_set_error("gemm: unknown epilogue %d", epi); return SAT_E_INVALID;
        case SAT_ROUTE_XATTN_OPERANDS: sat_set_error("gemm: fused cross-attention needs bf16 operands and K >= 192"); return SAT_E_UNSUPPORTED;
        case SAT_ROUTE_NO_E4M3_TILE: sat_set_error("gemm(fp8): variant %d has no e4m3 build (15, 16, 22, 30)", r.tile); return SAT_E_INVALID;
        case SAT_ROUTE_PH8_NOT_BUILT: sat_set_error("gemm(8-phase): epilogue %d / ablation %d not built", epi, r.tile); return SAT_E_UNSUPPORTED;
        default: sat_set_error("gemm: unknown variant %d (or not built for this epilogue)", r.tile); return SAT_E_INVALID;
    }
    SAT_CHECK_ARG(!qkn || r.family != SAT_GEMM_PH8, SAT_E_UNSUPPORTED, "gemm(8-phase): no qk_norm epilogue (variant %d forces the kernel)", a.variant);
    SAT_CHECK_ARG(!act16 || r.family != SAT_GEMM_PH8, SAT_E_UNSUPPORTED, "gemm(8-phase): no plain-activation epilogue (variant %d forces the kernel)", a.variant);
    if (r.family == SAT_GEMM_PH8) return sat_launch_gemm_ph8(epi, r.ph8, a, stream);
    switch (epi) {
        case EPI_ACT16: return launch_epi<EPI_ACT16, 0>(r.tile, a, stream);
        case EPI_SWIGLU: return launch_flavour<EPI_SWIGLU>(r, a, stream);
        case EPI_HEADS: return qkn ? launch_epi<EPI_HEADS_QKN, 0>(r.tile, a, stream) : launch_flavour<EPI_HEADS>(r, a, stream);
        default: return launch_flavour<EPI_F32>(r, a, stream);          // EPI_F32, EPI_RESID
    }
}
