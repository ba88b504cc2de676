// Oobleck 1-D conv VAE on MI355X: every Conv1d / ConvTranspose1d of
// models/autoencoders.py:45-194 (reference) runs as ONE implicit-GEMM MFMA kernel over
// channels-last bf16 activations act[b][t][c]:
//     out[m][n] = sum_j sum_ci  in[m*stride + off0 + j*doff][ci] * W[j][n][ci]
//   * dilated k=7 conv      : stride 1, off0 = -3*dil, doff = dil          (autoencoders.py:56)
//   * k=1 / k=3 conv        : stride 1, off0 = 0 / -1, doff = 1            (:58, :147)
//   * strided encoder conv  : stride s, off0 = -ceil(s/2), doff = 1, 2s taps (:80-81)
//   * transposed conv k=2s  : polyphase -- N = s*Cout (phase-major), 2 taps at rows m, m-1;
//                             row m of the GEMM is the contiguous output span
//                             [(m*s - pad)*Cout, +s*Cout)                     (:102-105)
//   * nearest upsample + conv : Upsample(s) then Conv1d(k=2s, "same") (:95-99) in the same polyphase form with THREE taps at
//                             rows m-1, m, m+1 and per-phase sums of the 2s original taps (wn_pack_nearest_kernel); the
//                             upsampled tensor never exists
// Contiguous sample windows are loaded with coalesced 16-byte accesses ([t][c] rows are
// 128..4096 B) into XOR-swizzled LDS tiles; taps re-read the window through L2.
// SnakeBeta (models/blocks.py:318-319) is never a standalone pass: the PRODUCER's epilogue
// applies the consumer's Snake to the fp32 accumulator and stores the activated tensor
// (and the raw tensor only where a residual needs it).  Weight norm (dac WNConv1d) is
// folded once at plan finalize.  ELU (use_snake=False) takes Snake's place in the same epilogues, and the decoder's final tanh sits in
// the epilogue of its last convolution; both are wave-uniform run-time fields of ConvArgs, not further kernel instantiations.
// The one activation that is a pass of its own is the anti-aliased one (antialias_activation=True, aa_act_kernel below): it reads 11 rows
// per output row, so the convolution in front writes its un-activated result in fp32 (ConvArgs::out_cf with cf_channels == 0) instead.
// Stage widths that are not multiples of 64 are rounded up inside the plan: weights, biases and Snake parameters are zero-padded at
// finalize, so the pad channels of every activation tensor are written as exact zeros (act(0) = 0) and no kernel masks channels.
// This file holds what depends on the operand type: the kernels and the launchers that own grid, LDS size and tile choice.  It is built
// once per format (bf16, fp16, fp32) and exports SAT_OPNS::oob_kernels (oobleck_kernels.h) to the plan, oobleck_plan.hip, which is built once.
#include <math.h>

#include <type_traits>

#include "oobleck_kernels.h"      // ConvArgs, RuArgs (namespace SAT_OPNS, opened by sat_common.h), OobKernels

namespace {

// nn.ELU(alpha = 1) on the fp32 accumulator; elu(0) == 0 exactly in both forms, which keeps the pad channels zero
__device__ __forceinline__ float elu_f(float v) {
#if SAT_OP_IS_F32
    return v > 0.f ? v : expm1f(v);
#else
    return v > 0.f ? v : __expf(v) - 1.f;      // absolute error ~1e-7, below the rounding of the 16-bit store
#endif
}

__device__ __forceinline__ float snake_f(float v, float a, float ib) {
#if SAT_OP_IS_F32
    float s = sinf(v * a);      // reference-precision build: the error of __sinf grows with |v * a| and would dominate
#else
    float s = __sinf(v * a);
#endif
    return v + ib * (s * s);
}

// LDS rows of one 64-channel K-tile: 128 B (16-bit builds: eight 16-byte chunks, lds_tile_off) or 256 B (fp32 build: sixteen
// chunks).  The fp32 swizzle XORs the chunk with row & 15, so each 16-lane group of a fragment read (16 consecutive rows, one
// logical chunk) covers the 16 slots of a 256-byte bank row; LDS-DMA destinations stay linear, the swizzle picks the sources.
constexpr int ROW_B = 64 * (int)sizeof(op_t);
constexpr int ROW_CH = ROW_B / 16;              // 16-byte chunks per row
constexpr int CH_EL = 16 / (int)sizeof(op_t);   // elements per chunk
__device__ __forceinline__ int chunk_swz(int row) { return SAT_OP_IS_F32 ? (row & 15) : ((row >> 1) & 7); }
__device__ __forceinline__ int conv_tile_off(int row, int chunk) { return row * ROW_B + ((chunk ^ chunk_swz(row)) << 4); }

// 8 consecutive channels of one row: one 16-byte store of packed 16-bit values, or two 16-byte stores in the fp32 build
__device__ __forceinline__ void store_op8(op_t* p, const float (&x)[8]) {
#if SAT_OP_IS_F32
    *reinterpret_cast<f32x4*>(p) = f32x4{x[0], x[1], x[2], x[3]};
    *reinterpret_cast<f32x4*>(p + 4) = f32x4{x[4], x[5], x[6], x[7]};
#else
    *reinterpret_cast<u32x4*>(p) = u32x4{pack_op2(x[0], x[1]), pack_op2(x[2], x[3]), pack_op2(x[4], x[5]), pack_op2(x[6], x[7])};
#endif
}

// Epilogue on TRANSPOSED accumulators (the main loop issues its MFMAs with the weight fragment as the A operand, see
// gather_channel_runs in sat_common.h): lane l31 owns output row m = mw + i*32 + l31 and, after one exchange between the wave
// halves, two groups of 8 consecutive channels.  Residual reads and bf16 stores are 16 bytes per lane (round 1 moved 2 bytes per
// access: the unit's 1 x 1 convolution then spent its whole time issuing them), bias and Snake parameters come as float4 pairs.
// flat = m*N + out_shift + n addresses plain convolutions (shift 0) and the polyphase transposed ones (N = stride * Cout columns per
// input row, shifted by the padding); shift and limit are multiples of Cout, groups are 8-aligned: a group is in or out as a whole.
// ACT is the activation behind out_snk: ACT_RUNTIME in the convolution kernel, which tests the wave-uniform g.act at each group (one
// kernel per tile whatever the plan's options: 68 VGPRs in the 16-bit builds and 97 in the fp32 one, as before the options existed;
// a branch hoisted around two copies of the epilogue, and an activation template parameter, timed the same within the box's spread,
// profiles/codec_options_timing.txt), or a compile-time constant in the fused ResidualUnit kernel.
template <int MI, int ACT>
__device__ __forceinline__ void conv_epilogue(const ConvArgs& g, f32x16 (&acc)[MI][2], const int mw, const int nw, const int b,
                                              const int half, const int l31) {
    if (g.out_cf && g.cf_channels) {      // fp32 channel-first result of the last convolution: consecutive lanes = consecutive time steps
        float* __restrict__ o = g.out_cf + (size_t)b * g.cf_channels * g.M;
#pragma unroll
        for (int i = 0; i < MI; ++i) {
            const int m = mw + i * 32 + l31;
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int n = nw + j * 32 + 8 * (r >> 2) + 4 * half + (r & 3);
                    if (m < g.M && n < g.cf_channels) {
                        const float v = acc[i][j][r] + (g.bias ? g.bias[n % g.Cout] : 0.f);
                        o[(size_t)n * g.M + m] = g.tanh_out ? tanhf(v) : v;
                    }
                }
        }
        return;
    }
    const op_t* res = g.res ? g.res + (size_t)b * g.out_bstride : nullptr;
    op_t* oraw = g.out_raw ? g.out_raw + (size_t)b * g.out_bstride : nullptr;
    op_t* __restrict__ osnk = g.out_snk ? g.out_snk + (size_t)b * g.out_bstride : nullptr;
    // out_cf without cf_channels: the un-activated result once more, in fp32 and indexed as out_raw, for the anti-aliased activation
    // behind this convolution (aa_act_kernel), which would otherwise read it rounded to the operand format
    float* __restrict__ of32 = g.out_cf ? g.out_cf + (size_t)b * g.out_bstride : nullptr;
#pragma unroll
    for (int i = 0; i < MI; ++i) {
        const int m = mw + i * 32 + l31;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            float v[16];
            gather_channel_runs(acc[i][j], v);
#pragma unroll
            for (int grp = 0; grp < 2; ++grp) {
                const int n = nw + j * 32 + grp * 16 + 8 * half;
                const long long flat = (long long)m * g.N + g.out_shift + n;
                const bool ok = m < g.M && flat >= 0 && flat + 8 <= g.out_limit;
                const int co = n % g.Cout;
                float x[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) x[e] = v[grp * 8 + e];
                if (g.bias) {
                    const f32x4 b0 = *reinterpret_cast<const f32x4*>(g.bias + co), b1 = *reinterpret_cast<const f32x4*>(g.bias + co + 4);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        x[e] += b0[e];
                        x[4 + e] += b1[e];
                    }
                }
                if (res && ok) {
                    const opx8 rv = *reinterpret_cast<const opx8*>(res + flat);
#pragma unroll
                    for (int e = 0; e < 8; ++e) x[e] += op_to_f32(rv[e]);
                }
                if (oraw && ok) store_op8(oraw + flat, x);
                if (of32 && ok) {
                    *reinterpret_cast<f32x4*>(of32 + flat) = f32x4{x[0], x[1], x[2], x[3]};
                    *reinterpret_cast<f32x4*>(of32 + flat + 4) = f32x4{x[4], x[5], x[6], x[7]};
                }
                if (osnk) {
                    float y[8];
                    if (ACT == ACT_RUNTIME ? g.act == ACT_ELU : ACT == ACT_ELU) {
#pragma unroll
                        for (int e = 0; e < 8; ++e) y[e] = elu_f(x[e]);
                    } else {
                        const f32x4 a0 = *reinterpret_cast<const f32x4*>(g.sn_a + co), a1 = *reinterpret_cast<const f32x4*>(g.sn_a + co + 4);
                        const f32x4 i0 = *reinterpret_cast<const f32x4*>(g.sn_ib + co), i1 = *reinterpret_cast<const f32x4*>(g.sn_ib + co + 4);
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            y[e] = snake_f(x[e], a0[e], i0[e]);
                            y[4 + e] = snake_f(x[4 + e], a1[e], i1[e]);
                        }
                    }
                    if (ok) store_op8(osnk + flat, y);
                }
            }
        }
    }
}

// Main loop of the implicit-GEMM convolution: acc[i][j] (+)= the BM x BN output tile (rows m0.., columns n0..) of batch item b.
// NS-stage LDS ring filled by LDS-DMA, prefetch distance NS-1, one raw barrier per K-tile (= one tap x 64 input channels), counted
// vmcnt.  Returns with every load landed; the caller owns the barrier that frees the ring.
template <int BM, int BN, int WM, int WN, int NS>
__device__ __forceinline__ void conv_main_loop(const ConvArgs& g, char* smem, const int m0, const int n0, const int b,
                                               f32x16 (&acc)[BM / WM / 32][2]) {
    constexpr int NT = WM * WN * 64;
    constexpr int TM = BM / WM;
    constexpr int TN = BN / WN;
    static_assert(TN == 64, "wave tile is TM x 64");
    constexpr int MI = TM / 32;
    constexpr int NI = 2;
    constexpr int A_CH = BM * ROW_CH / NT;
    constexpr int B_CH = BN * ROW_CH / NT;
    constexpr int LPT = A_CH + B_CH;
    constexpr int STAGE_BYTES = (BM + BN) * ROW_B;
    constexpr int D = NS - 1;
    static_assert(A_CH >= 1 && B_CH >= 1 && (D > 0) && (D - 1) * LPT < 64, "bad pipeline geometry");

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const int half = lane >> 5, l31 = lane & 31;

    const int Cin = g.Cin, Tin = g.Tin;
    const int cpt = Cin >> 6;
    const int nk = g.taps * cpt;
    const op_t* __restrict__ inb = g.in + (size_t)b * Tin * Cin;

    int a_m[A_CH], a_coff[A_CH];
#pragma unroll
    for (int i = 0; i < A_CH; ++i) {
        int q = i * NT + tid;
        int row = q / ROW_CH, pos = q % ROW_CH;
        a_m[i] = (m0 + row) * g.stride;
        a_coff[i] = (pos ^ chunk_swz(row)) * CH_EL;
    }
    int b_off[B_CH];
#pragma unroll
    for (int i = 0; i < B_CH; ++i) {
        int q = i * NT + tid;
        int row = q / ROW_CH, pos = q % ROW_CH;
        b_off[i] = row * Cin + (pos ^ chunk_swz(row)) * CH_EL;
    }

    auto stage_in = [&](int kt, int stage) {
        const int tap = kt / cpt;
        const int ci0 = (kt - tap * cpt) << 6;
        const int off = g.off0 + tap * g.doff;
        char* sa = smem + stage * STAGE_BYTES;
        char* sb = sa + BM * ROW_B;
#pragma unroll
        for (int i = 0; i < A_CH; ++i) {
            const int r = a_m[i] + off;
            const op_t* src = (r >= 0 && r < Tin) ? inb + (size_t)r * Cin + ci0 + a_coff[i] : g.zero_page + a_coff[i];
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                             (__attribute__((address_space(3))) void*)(sa + (i * NT + wave * 64) * 16), 16, 0, 0);
        }
        const op_t* wt = g.W + ((size_t)tap * g.N + n0) * Cin + ci0;
#pragma unroll
        for (int i = 0; i < B_CH; ++i)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(wt + b_off[i]),
                                             (__attribute__((address_space(3))) void*)(sb + (i * NT + wave * 64) * 16), 16, 0, 0);
    };
#if SAT_OP_IS_F32
    // fp32 build, v_mfma_f32_32x32x2_f32 (K = 2): lane half h takes channels 32 h + 4 ks + e of its row (one 16-byte chunk per
    // fragment and ks, four MFMAs per chunk).  A and B use the same channel order, so the sum runs over the 64 channels exactly once.
    auto compute = [&](int stage) {
        const char* sa = smem + stage * STAGE_BYTES;
        const char* sb = sa + BM * ROW_B;
        f32x4 af[2][MI], bfr[2][NI];
        auto frag = [&](int ks, int buf) {
#pragma unroll
            for (int i = 0; i < MI; ++i)
                af[buf][i] = *reinterpret_cast<const f32x4*>(sa + conv_tile_off(wm * TM + i * 32 + l31, half * 8 + ks));
#pragma unroll
            for (int j = 0; j < NI; ++j)
                bfr[buf][j] = *reinterpret_cast<const f32x4*>(sb + conv_tile_off(wn * TN + j * 32 + l31, half * 8 + ks));
        };
        frag(0, 0);
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {
            if (ks + 1 < 8) frag(ks + 1, (ks + 1) & 1);
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int i = 0; i < MI; ++i)
#pragma unroll
                    for (int j = 0; j < NI; ++j)      // C^T: lane = output row
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(bfr[ks & 1][j][e], af[ks & 1][i][e], acc[i][j], 0, 0, 0);
        }
    };
#else
    auto compute = [&](int stage) {
        const char* sa = smem + stage * STAGE_BYTES;
        const char* sb = sa + BM * ROW_B;
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
        __builtin_amdgcn_sched_group_barrier(0x100, MI + NI, 0);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            if (ks + 1 < 4) frag(ks + 1, (ks + 1) & 1);
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int j = 0; j < NI; ++j)
                    acc[i][j] = mfma_32x32x16(bfr[ks & 1][j], af[ks & 1][i], acc[i][j]);      // C^T: lane = output row
            if (ks + 1 < 4) {
                constexpr int NR = MI + NI, NM = MI * NI;
#pragma unroll
                for (int r = 0; r < (NR < NM ? NR : NM); ++r) {
                    __builtin_amdgcn_sched_group_barrier(0x8, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                }
                if (NM > NR) __builtin_amdgcn_sched_group_barrier(0x8, NM - NR, 0);
                if (NR > NM) __builtin_amdgcn_sched_group_barrier(0x100, NR - NM, 0);
            } else {
                __builtin_amdgcn_sched_group_barrier(0x8, MI * NI, 0);
            }
        }
    };
#endif

#pragma unroll
    for (int s = 0; s < D; ++s) stage_in(s, s);       // nk >= D guaranteed by the launcher
    int rd = 0, wr = D;
    for (int k = 0; k < nk - D; ++k) {
        wait_vmcnt<(D - 1) * LPT>();
        __builtin_amdgcn_s_barrier();
        stage_in(k + D, wr);
        compute(rd);
        rd = (rd + 1 == NS) ? 0 : rd + 1;
        wr = (wr + 1 == NS) ? 0 : wr + 1;
    }
    for (int k = nk - D; k < nk; ++k) {
        wait_vmcnt<0>();
        __builtin_amdgcn_s_barrier();
        compute(rd);
        rd = (rd + 1 == NS) ? 0 : rd + 1;
    }
}

template <int BM, int BN, int WM, int WN, int NS>
__global__ __launch_bounds__(WM * WN * 64) void conv_pipe_kernel(ConvArgs g) {
    sat_f16_saturate();
    constexpr int TM = BM / WM;
    constexpr int TN = BN / WN;
    constexpr int MI = TM / 32;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const int b = blockIdx.y;
    const int tiles_n = g.N / BN;
    const int bid = xcd_remap(blockIdx.x, gridDim.x);
    const int tm = bid / tiles_n;
    const int tn = bid - tm * tiles_n;
    const int m0 = tm * BM, n0 = tn * BN;
    f32x16 acc[MI][2];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    conv_main_loop<BM, BN, WM, WN, NS>(g, smem, m0, n0, b, acc);
    conv_epilogue<MI, ACT_RUNTIME>(g, acc, m0 + wm * TM, n0 + wn * TN, b, lane >> 5, lane & 31);
}

// ---------------------------------------------------------------------------------------------
// One ResidualUnit (autoencoders.py:45-68: x + conv1(snake(conv7_dilated(snake(x))))) in ONE launch for the layers whose channel
// count fits one workgroup tile (C = BN).  The k = 7 convolution runs as above; its epilogue applies bias and the second Snake and
// leaves the 128 x C block in LDS (bf16, the swizzled 64-channel K-tiles the fragment reads expect) instead of HBM; the 1 x 1
// convolution is a second MFMA pass over that block with its C x C weights streamed through the freed ring; the final epilogue is the
// ordinary one (bias, raw residual, raw and / or Snake'd output).  Against two launches this removes one write and one read of the
// activation (537 MB each at the top decoder level), the <= 4-K-tile kernel whose time was all prologue and epilogue, and a launch.
// ---------------------------------------------------------------------------------------------
#if !SAT_OP_IS_F32

template <int BN, int WM, int WN, int NS, int ACT>      // ACT: the plan's activation (both Snakes / ELUs of the unit and the one behind it)
__global__ __launch_bounds__(WM * WN * 64) void ru_fused_kernel(RuArgs ga) {
    sat_f16_saturate();
    constexpr int BM = 128;
    constexpr int NT = WM * WN * 64;
    constexpr int TM = BM / WM;
    constexpr int TN = BN / WN;
    constexpr int MI = TM / 32;
    constexpr int KT1 = BN / 64;                       // K-tiles of the 1 x 1 convolution (64 channels each)
    constexpr int Y_BYTES = KT1 * BM * 128;            // the intermediate block: KT1 tiles of 128 rows x 128 B
    constexpr int W_TILE = BN * 128;                   // one K-tile of the 1 x 1 weights: BN rows x 64 channels
    constexpr int W_CH = BN * 8 / NT;                  // 16-byte pieces per thread per weight tile
    static_assert(Y_BYTES + 2 * W_TILE <= NS * (BM + BN) * 128, "the 1 x 1 stage must fit into the ring of the k = 7 stage");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const int half = lane >> 5, l31 = lane & 31;
    const int b = blockIdx.y;
    const int m0 = xcd_remap(blockIdx.x, gridDim.x) * BM;
    const ConvArgs& g7 = ga.c7;
    const ConvArgs& g1 = ga.c1;

    f32x16 acc[MI][2];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    conv_main_loop<BM, BN, WM, WN, NS>(g7, smem, m0, 0, b, acc);
    __builtin_amdgcn_s_barrier();                      // every wave is done with the ring

    // ---- the 1 x 1 weights, K-tiles 0 and 1, behind the intermediate block (same swizzle as every other tile)
    char* sw = smem + Y_BYTES;
    int w_off[W_CH];
#pragma unroll
    for (int i = 0; i < W_CH; ++i) {
        const int q = i * NT + tid;
        const int row = q >> 3, pos = q & 7;
        w_off[i] = row * BN + (pos ^ ((row >> 1) & 7)) * 8;
    }
    auto w_in = [&](int kt, int stage) {
#pragma unroll
        for (int i = 0; i < W_CH; ++i)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(g1.W + kt * 64 + w_off[i]),
                                             (__attribute__((address_space(3))) void*)(sw + stage * W_TILE + (i * NT + wave * 64) * 16), 16, 0, 0);
    };
    w_in(0, 0);
    w_in(1, 1);

    // ---- first epilogue: y = act(acc + bias) -> bf16 -> LDS, 8 channels (one 16-byte chunk of a K-tile row) per store
#pragma unroll
    for (int i = 0; i < MI; ++i) {
        const int row = wm * TM + i * 32 + l31;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            float v[16];
            gather_channel_runs(acc[i][j], v);
#pragma unroll
            for (int grp = 0; grp < 2; ++grp) {
                const int n = wn * TN + j * 32 + grp * 16 + 8 * half;
                const f32x4 b0 = *reinterpret_cast<const f32x4*>(g7.bias + n), b1 = *reinterpret_cast<const f32x4*>(g7.bias + n + 4);
                float y[8];
                if (ACT == ACT_ELU) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        y[e] = elu_f(v[grp * 8 + e] + b0[e]);
                        y[4 + e] = elu_f(v[grp * 8 + 4 + e] + b1[e]);
                    }
                } else {
                    const f32x4 a0 = *reinterpret_cast<const f32x4*>(g7.sn_a + n), a1 = *reinterpret_cast<const f32x4*>(g7.sn_a + n + 4);
                    const f32x4 i0 = *reinterpret_cast<const f32x4*>(g7.sn_ib + n), i1 = *reinterpret_cast<const f32x4*>(g7.sn_ib + n + 4);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        y[e] = snake_f(v[grp * 8 + e] + b0[e], a0[e], i0[e]);
                        y[4 + e] = snake_f(v[grp * 8 + 4 + e] + b1[e], a1[e], i1[e]);
                    }
                }
                *reinterpret_cast<u32x4*>(smem + (n >> 6) * (BM * 128) + lds_tile_off(row, (n & 63) >> 3)) =
                    u32x4{pack_op2(y[0], y[1]), pack_op2(y[2], y[3]), pack_op2(y[4], y[5]), pack_op2(y[6], y[7])};
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
        }
    }

    // ---- 1 x 1 convolution: acc = y . W1^T, K-tiles of 64 channels, weights in a 2-stage ring
#pragma unroll 1
    for (int kt = 0; kt < KT1; ++kt) {
        wait_vmcnt<0>();
        __syncthreads();                               // y written by everybody (first pass; waits for the ds_writes too), weight tile kt landed
        const char* sa_ = smem + kt * (BM * 128);
        const char* sb_ = sw + (kt & 1) * W_TILE;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            opx8 af[MI], bfr[2];
#pragma unroll
            for (int i = 0; i < MI; ++i) af[i] = *reinterpret_cast<const opx8*>(sa_ + lds_tile_off(wm * TM + i * 32 + l31, ks * 2 + half));
#pragma unroll
            for (int j = 0; j < 2; ++j) bfr[j] = *reinterpret_cast<const opx8*>(sb_ + lds_tile_off(wn * TN + j * 32 + l31, ks * 2 + half));
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = mfma_32x32x16(bfr[j], af[i], acc[i][j]);
        }
        if (kt + 2 < KT1) {
            __builtin_amdgcn_s_barrier();              // stage kt & 1 is free again
            w_in(kt + 2, kt & 1);
        }
    }
    conv_epilogue<MI, ACT>(g1, acc, m0 + wm * TM, wn * TN, b, half, l31);
}
#endif  // !SAT_OP_IS_F32

// z [B][C][T] fp32 (channel-first) -> [B][T][Cp] bf16, channels C..Cp-1 (the plan's padding to a multiple of 64) written as zeros
__global__ __launch_bounds__(256) void cf_to_cl_kernel(const float* __restrict__ x, op_t* __restrict__ y, int C, int Cp, int T) {
    sat_f16_saturate();
    __shared__ float tile[64][65];
    const int b = blockIdx.z, t0 = blockIdx.x * 64, c0 = blockIdx.y * 64;
    for (int i = threadIdx.x; i < 64 * 64; i += 256) {
        int c = i >> 6, t = i & 63;
        tile[c][t] = (c0 + c < C && t0 + t < T) ? x[((size_t)b * C + c0 + c) * T + t0 + t] : 0.f;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 64 * 64; i += 256) {
        int t = i >> 6, c = i & 63;
        if (c0 + c < Cp && t0 + t < T) y[((size_t)b * T + t0 + t) * Cp + c0 + c] = f32_to_op(tile[c][t]);
    }
}

// OobleckEncoder first conv (autoencoders.py:136): audio [B][Cin<=2][L] fp32 channel-first,
// k=7 pad 3 -> Cout channels; writes raw + activated channels-last bf16 rows of Cp >= Cout channels (pad channels: zeros).
// VALU (K = 14).  GENERAL = false is the Stable Audio case (Snake, Cp == Cout) with the tests for pad channels and ELU folded away, so
// that its code, and with it the rounding of its multiply-add chain, is what it was before those options existed.
template <bool GENERAL>
__global__ __launch_bounds__(256) void first_conv_kernel(const float* __restrict__ x, const float* __restrict__ w /*[Cout][Cin][7]*/,
                                                         const float* __restrict__ bias, const float* __restrict__ sn_a,
                                                         const float* __restrict__ sn_ib, int act, op_t* __restrict__ out_raw,
                                                         op_t* __restrict__ out_snk, int Cin, int Cout, int Cp, int L) {
    sat_f16_saturate();
    __shared__ float xs[2][64 + 6];
    const int b = blockIdx.y, t0 = blockIdx.x * 64;
    for (int i = threadIdx.x; i < 2 * 70; i += 256) {
        int c = i / 70, k = i - c * 70;
        int t = t0 + k - 3;
        xs[c][k] = (c < Cin && t >= 0 && t < L) ? x[((size_t)b * Cin + c) * L + t] : 0.f;
    }
    __syncthreads();
    for (int co = threadIdx.x; co < Cp; co += 256) {
        const bool real = !GENERAL || co < Cout;
        float wr[2][7];
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int k = 0; k < 7; ++k) wr[c][k] = (real && c < Cin) ? w[((size_t)co * Cin + c) * 7 + k] : 0.f;
        const float bv = real ? bias[co] : 0.f;
        const bool elu = GENERAL && act == ACT_ELU;
        const float a = elu ? 0.f : sn_a[co], ib = elu ? 0.f : sn_ib[co];      // [Cp], zero-padded
        for (int tt = 0; tt < 64; ++tt) {
            if (t0 + tt >= L) break;
            float acc = bv;
#pragma unroll
            for (int c = 0; c < 2; ++c)
#pragma unroll
                for (int k = 0; k < 7; ++k) acc += wr[c][k] * xs[c][tt + k];
            size_t o = ((size_t)b * L + t0 + tt) * Cp + co;
            out_raw[o] = f32_to_op(acc);
            out_snk[o] = f32_to_op(elu ? elu_f(acc) : snake_f(acc, a, ib));
        }
    }
}

// ---- the anti-aliased activation (antialias_activation=True: alias_free_torch.Activation1d around SnakeBeta / ELU, autoencoders.py:39-40)
// Per channel along time, with f the 12-tap Kaiser-windowed sinc (cutoff 0.25, half-width 0.3, sum 1; symmetric, f[j] == f[11 - j]):
//     u[m] = 2 sum_i xp[i] f[m + 15 - 2 i],  xp[i] = x[clamp(i - 5, 0, L - 1)]      (replicate pad 5, transposed convolution stride 2, cut 15)
//     v[m] = act(u[m]),  m = 0 .. 2 L - 1
//     y[t] = sum_j f[j] v[clamp(2 t + j - 5, 0, 2 L - 1)]                            (replicate pad 5 / 6 of the ACTIVATED signal, stride 2)
// so u[2 k] reads rows k - 3 .. k + 2 on the odd taps, u[2 k + 1] rows k - 2 .. k + 3 on the even ones, and y[t] the pairs t - 3 .. t + 3.
// One thread owns 16 bytes of channels and walks AA_TIME_TILE output rows in registers: a window of 7 input rows and 7 partial sums.  Step k
// computes the pair v[2 k], v[2 k + 1] once and scatters it into the sums of y[k - 3 .. k + 3]; y[k - 3] is then complete.  The clamp of the
// activated signal only ever repeats v[0] and v[2 L - 1]: their weights in y[t] are prefix / suffix sums of f, added at k == 0 / k == L - 1
// on top of the plain tap (for L < 6 both happen to the same sums).  Every row is read once per tile (plus the halo of 6 steps, from L2),
// every v computed once per tile; no LDS.  Reads stay inside [0, L) of the batch item by the clamps, writes inside the tile's rows.
constexpr int AA_CH = CH_EL;      // channels per thread: 8 (16-bit builds) or 4 (fp32)
typedef float aa_f2 __attribute__((ext_vector_type(2)));
typedef op_t aa_opv __attribute__((ext_vector_type(AA_CH)));
typedef float aa_f32v __attribute__((ext_vector_type(AA_CH)));
__host__ __device__ constexpr float aa_tap(int j) {
    constexpr float h[6] = {0.0020289664498962f, 0.0093894639440679f, -0.0255434640652947f, -0.0576573754753650f, 0.1285726090813288f, 0.4432098000653667f};
    return h[j < 6 ? j : 11 - j];
}
__host__ __device__ constexpr float aa_prefix(int n) {      // f[0] + ... + f[n]; by symmetry also f[11 - n] + ... + f[11]
    float s = 0.f;
    for (int j = 0; j <= n; ++j) s += aa_tap(j);
    return s;
}
__device__ __forceinline__ aa_f2 aa_activate(aa_f2 u, bool elu, aa_f2 a, aa_f2 ib) {
    if (elu) return aa_f2{elu_f(u[0]), elu_f(u[1])};
    return aa_f2{snake_f(u[0], a[0], ib[0]), snake_f(u[1], a[1], ib[1])};
}
template <typename V>
__device__ __forceinline__ void aa_unpack(const V r, aa_f2 (&x)[AA_CH / 2]) {
#pragma unroll
    for (int e = 0; e < AA_CH / 2; ++e) x[e] = aa_f2{(float)r[2 * e], (float)r[2 * e + 1]};
}
// IN_F32: the input rows are fp32 whatever the build -- what the plan's convolutions leave for this kernel (ConvArgs::out_cf without
// cf_channels), so that the un-activated tensor is not rounded to a 16-bit format on its way here; otherwise rows of the operand type
// ELU: the activation, a template parameter here -- as a run-time field the compiler evaluates Snake and ELU for every element and selects
template <bool IN_F32, bool ELU>
__global__ __launch_bounds__(256) void aa_act_kernel(const void* __restrict__ in_rows, op_t* __restrict__ out, const float* __restrict__ sn_a,
                                                     const float* __restrict__ sn_ib, int Cp, int L, int ntile, long long nwork) {
    using in_t = typename std::conditional<IN_F32, float, op_t>::type;
    using in_v = typename std::conditional<IN_F32, aa_f32v, aa_opv>::type;
    const in_t* __restrict__ in = static_cast<const in_t*>(in_rows);
    sat_f16_saturate();
    constexpr int TT = AA_TIME_TILE, P = AA_CH / 2;
    const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
    if (id >= nwork) return;
    const int G = Cp / AA_CH;
    const int cg = (int)(id % G);
    const long long tile = id / G;
    const int b = (int)(tile / ntile), t0 = (int)(tile % ntile) * TT, tend = min(t0 + TT, L);
    const in_t* __restrict__ x = in + (size_t)b * L * Cp + cg * AA_CH;
    op_t* __restrict__ y = out + (size_t)b * L * Cp + cg * AA_CH;
    constexpr bool elu = ELU;
    aa_f2 a[P], ib[P];
#pragma unroll
    for (int e = 0; e < P; ++e) {
        a[e] = elu ? aa_f2{0.f, 0.f} : *reinterpret_cast<const aa_f2*>(sn_a + cg * AA_CH + 2 * e);
        ib[e] = elu ? aa_f2{0.f, 0.f} : *reinterpret_cast<const aa_f2*>(sn_ib + cg * AA_CH + 2 * e);
    }
    auto row = [&](int r) { return *reinterpret_cast<const in_v*>(x + (size_t)min(max(r, 0), L - 1) * Cp); };
    // xw[d] = x[clamp(k - 3 + d)], acc[d] = the partial sum of y[k - 3 + d]; q0 / q1: rows k + 4, k + 5 on their way
    aa_f2 xw[7][P], acc[7][P];
#pragma unroll
    for (int d = 0; d < 7; ++d) {
        aa_unpack(row(t0 - 6 + d), xw[d]);
#pragma unroll
        for (int e = 0; e < P; ++e) acc[d][e] = aa_f2{0.f, 0.f};
    }
    in_v q0 = row(t0 + 1), q1 = row(t0 + 2);
    auto step = [&](const int k, in_v& q) {
        if (k >= 0 && k < L) {
#pragma unroll
            for (int e = 0; e < P; ++e) {
                aa_f2 ue = aa_tap(11) * xw[0][e], uo = aa_tap(10) * xw[1][e];
#pragma unroll
                for (int d = 1; d < 6; ++d) {
                    ue += aa_tap(11 - 2 * d) * xw[d][e];
                    uo += aa_tap(10 - 2 * d) * xw[d + 1][e];
                }
                const aa_f2 ve = aa_activate(2.f * ue, elu, a[e], ib[e]), vo = aa_activate(2.f * uo, elu, a[e], ib[e]);
#pragma unroll
                for (int d = 0; d < 6; ++d) {
                    acc[d][e] += aa_tap(11 - 2 * d) * ve;          // v[2 k] in y[k - 3 + d]: tap 2 k + 5 - 2 t
                    acc[d + 1][e] += aa_tap(10 - 2 * d) * vo;      // v[2 k + 1] in y[k - 2 + d]
                }
                if (k == 0) {          // v[0] also stands for v[-5 .. -1]: y[t] takes it on the taps 0 .. 5 - 2 t
#pragma unroll
                    for (int d = 3; d < 6; ++d) acc[d][e] += (aa_prefix(11 - 2 * d) - aa_tap(11 - 2 * d)) * ve;
                }
                if (k == L - 1) {      // v[2 L - 1] also stands for v[2 L .. 2 L + 5]: y[L - 3 + d] takes it on the taps 10 - 2 d .. 11
#pragma unroll
                    for (int d = 0; d < 3; ++d) acc[d + 1][e] += (aa_prefix(1 + 2 * d) - aa_tap(10 - 2 * d)) * vo;
                }
            }
        }
        const int t = k - 3;
        if (t >= t0 && t < tend) {
            aa_opv o;
#pragma unroll
            for (int e = 0; e < P; ++e) {
                o[2 * e] = f32_to_op(acc[0][e][0]);
                o[2 * e + 1] = f32_to_op(acc[0][e][1]);
            }
            *reinterpret_cast<aa_opv*>(y + (size_t)t * Cp) = o;
        }
#pragma unroll
        for (int d = 0; d < 6; ++d)
#pragma unroll
            for (int e = 0; e < P; ++e) {
                xw[d][e] = xw[d + 1][e];
                acc[d][e] = acc[d + 1][e];
            }
        aa_unpack(q, xw[6]);
#pragma unroll
        for (int e = 0; e < P; ++e) acc[6][e] = aa_f2{0.f, 0.f};
        q = row(k + 6);      // consumed two steps on, as row (k + 2) + 4
    };
    static_assert((TT + 6) % 2 == 0, "the walk below takes its steps in pairs");
#pragma unroll 1
    for (int k = t0 - 3; k < t0 + TT + 3; k += 2) {
        step(k, q0);
        step(k + 1, q1);
    }
}

// ---- weight-norm folding (dac WNConv1d == torch weight_norm dim 0): w = g * v / ||v||
__global__ __launch_bounds__(256) void wn_invnorm_kernel(const float* __restrict__ v, const float* __restrict__ gsc,
                                                         float* __restrict__ scale, int slice) {
    sat_f16_saturate();
    __shared__ float red[4];
    const int i = blockIdx.x;
    float s = 0.f;
    for (int k = threadIdx.x; k < slice; k += 256) {
        float x = v[(size_t)i * slice + k];
        s += x * x;
    }
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) scale[i] = gsc[i] / sqrtf(red[0] + red[1] + red[2] + red[3]);
}
// Conv1d v[co][ci][k] -> W[j][Npad][Kpad] bf16 (rows co >= Cout and columns ci >= Cin are zero)
__global__ void wn_pack_conv_kernel(const float* __restrict__ v, const float* __restrict__ scale, op_t* __restrict__ W,
                                    int Cout, int Cin, int k, int Npad, int Kpad) {
    sat_f16_saturate();
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)k * Npad * Kpad) return;
    int ci = (int)(i % Kpad);
    int n = (int)((i / Kpad) % Npad);
    int j = (int)(i / ((size_t)Kpad * Npad));
    W[i] = f32_to_op(n < Cout && ci < Cin ? v[((size_t)n * Cin + ci) * k + j] * scale[n] : 0.f);
}
// same, fp32, original layout (for the VALU first conv)
__global__ void wn_fold_f32_kernel(const float* __restrict__ v, const float* __restrict__ scale, float* __restrict__ w, int slice,
                                   size_t n) {
    sat_f16_saturate();
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) w[i] = v[i] * scale[i / slice];
}
// ConvTranspose1d v[ci][co][k=2s] -> W[j][phi*Np+co][Kp] = w[ci][co][phi + j*s]  (Np, Kp: Cout, Cin rounded up; the padding is zero)
__global__ void wn_pack_convT_kernel(const float* __restrict__ v, const float* __restrict__ scale, op_t* __restrict__ W,
                                     int Cin, int Cout, int s, int Kp, int Np) {
    sat_f16_saturate();
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int N = s * Np;
    if (i >= (size_t)2 * N * Kp) return;
    int ci = (int)(i % Kp);
    int n = (int)((i / Kp) % N);
    int j = (int)(i / ((size_t)Kp * N));
    int phi = n / Np, co = n - phi * Np;
    W[i] = f32_to_op(co < Cout && ci < Cin ? v[((size_t)ci * Cout + co) * (2 * s) + phi + j * s] * scale[ci] : 0.f);
}
// Upsample(scale_factor = s, nearest) + Conv1d v[co][ci][k=2s], padding "same" (s-1 left, s right): output sample m*s + phi reads the
// upsampled positions m*s + phi + j - (s-1), j = 0..2s-1, i.e. input rows m-1, m, m+1.  W[r+1][phi*Np+co][Kp] = the fp32 sum of the
// folded taps j with floor((phi + j - s + 1) / s) == r, r = -1, 0, 1.
__global__ void wn_pack_nearest_kernel(const float* __restrict__ v, const float* __restrict__ scale, op_t* __restrict__ W,
                                       int Cin, int Cout, int s, int Kp, int Np) {
    sat_f16_saturate();
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int N = s * Np;
    if (i >= (size_t)3 * N * Kp) return;
    int ci = (int)(i % Kp);
    int n = (int)((i / Kp) % N);
    int r = (int)(i / ((size_t)Kp * N)) - 1;
    int phi = n / Np, co = n - phi * Np;
    float acc = 0.f;
    if (co < Cout && ci < Cin) {
        // the taps of row r: (r*s + s - 1 - phi) <= j < ((r+1)*s + s - 1 - phi), clipped to [0, 2s)
        const int lo = max(0, r * s + s - 1 - phi), hi = min(2 * s, (r + 1) * s + s - 1 - phi);
        for (int j = lo; j < hi; ++j) acc += v[((size_t)co * Cin + ci) * (2 * s) + j] * scale[co];
    }
    W[i] = f32_to_op(acc);
}
// a / ib hold Cp >= C entries; the pad entries are zero (snake(0) = 0 + 0 * sin^2(0))
__global__ void snake_params_kernel(const float* __restrict__ alpha, const float* __restrict__ beta, float* __restrict__ a,
                                    float* __restrict__ ib, int C, int Cp) {
    sat_f16_saturate();
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Cp) return;
    a[i] = i < C ? expf(alpha[i]) : 0.f;
    ib[i] = i < C ? 1.0f / (expf(beta[i]) + 0.000000001f) : 0.f;
}

template <int BM, int BN, int WM, int WN, int NS>
int launch_conv_cfg(const ConvArgs& a, int B, hipStream_t s) {
    constexpr int LDS = NS * (BM + BN) * ROW_B;
    auto kern = conv_pipe_kernel<BM, BN, WM, WN, NS>;
    SAT_TRY(sat_ensure_dynamic_lds(reinterpret_cast<const void*>(kern), LDS));
    hipLaunchKernelGGL(kern, dim3(cdiv(a.M, BM) * (a.N / BN), B), dim3(WM * WN * 64), LDS, s, a);
    SAT_LAUNCH_CHECK();
    return 0;
}

int launch_conv(const void* conv_args, int B, hipStream_t s) {
    const ConvArgs& a = *static_cast<const ConvArgs*>(conv_args);
    SAT_CHECK_ARG(a.Cin % 64 == 0, SAT_E_UNSUPPORTED, "conv: Cin=%d must be a multiple of 64", a.Cin);
    SAT_CHECK_ARG(a.N % 64 == 0, SAT_E_UNSUPPORTED, "conv: N=%d must be a multiple of 64", a.N);
    SAT_CHECK_ARG(a.zero_page != nullptr, SAT_E_STATE, "conv: zero page missing");
    const int nk = a.taps * (a.Cin / 64);
#if SAT_OP_IS_F32
    // fp32: 256-byte rows double every stage, and at 1/16 of the 16-bit MFMA rate one K-tile of compute (1024 cycles per wave and
    // 32 x 64 block) hides a whole tile of loads: a 2-stage ring, 8 waves of 32 x 64 on 128 x 128 (128 KiB), 4 on 128 x 64 (96 KiB)
    (void)nk;
    if (a.N % 128 == 0) return launch_conv_cfg<128, 128, 4, 2, 2>(a, B, s);
    return launch_conv_cfg<128, 64, 4, 1, 2>(a, B, s);
#else
    if (a.N % 128 == 0) {
        if (nk >= 3) return launch_conv_cfg<128, 128, 4, 2, 3>(a, B, s);
        return launch_conv_cfg<128, 128, 4, 2, 2>(a, B, s);
    }
    if (nk >= 3) return launch_conv_cfg<256, 64, 8, 1, 3>(a, B, s);
    return launch_conv_cfg<256, 64, 8, 1, 2>(a, B, s);
#endif
}

int launch_cf_to_cl(const float* z, void* y, int C, int T, int B, hipStream_t s) {
    hipLaunchKernelGGL(cf_to_cl_kernel, dim3(cdiv(T, 64), pad64(C) / 64, B), dim3(256), 0, s, z, (op_t*)y, C, pad64(C), T);
    SAT_LAUNCH_CHECK();
    return 0;
}

// the encoder's first convolution (VALU): C channels out of Cin <= 2, raw and activated rows of pad64(C) channels
int launch_first_conv(const float* audio, const float* w_f32, const float* bias, const float* sn_a, const float* sn_ib, int act, void* raw,
                      void* snk, int Cin, int C, int L, int B, hipStream_t s) {
    const bool general = act != ACT_SNAKE || pad64(C) != C;
    hipLaunchKernelGGL(general ? first_conv_kernel<true> : first_conv_kernel<false>, dim3(cdiv(L, 64), B), dim3(256), 0, s, audio, w_f32,
                       bias, sn_a, sn_ib, act, (op_t*)raw, (op_t*)snk, Cin, C, pad64(C), L);
    SAT_LAUNCH_CHECK();
    return 0;
}

// the anti-aliased activation: one thread per 16 bytes of channels and AA_TIME_TILE output rows
int launch_aa_act(const void* in, int in_f32, void* out, const float* sn_a, const float* sn_ib, int act, int Cp, int L, int B, hipStream_t s) {
    SAT_CHECK_ARG(in && out && in != out, SAT_E_INVALID, "aa_act: needs an input and an output of its own (an output row reads 11 input rows)");
    SAT_CHECK_ARG(Cp > 0 && Cp % 64 == 0 && L > 0 && B > 0, SAT_E_INVALID, "aa_act: bad shape [%d][%d][%d]", B, L, Cp);
    SAT_CHECK_ARG(act == ACT_ELU || (act == ACT_SNAKE && sn_a && sn_ib), SAT_E_INVALID, "aa_act: Snake parameters missing or unknown activation %d", act);
    const int ntile = cdiv(L, AA_TIME_TILE);
    const long long nwork = (long long)B * ntile * (Cp / AA_CH);
    SAT_CHECK_ARG(nwork / 256 < 0x7fffffffLL, SAT_E_UNSUPPORTED, "aa_act: [%d][%d][%d] is more than one grid", B, L, Cp);
    const bool elu = act == ACT_ELU;
    auto kern = in_f32 ? (elu ? aa_act_kernel<true, true> : aa_act_kernel<true, false>) : (elu ? aa_act_kernel<false, true> : aa_act_kernel<false, false>);
    hipLaunchKernelGGL(kern, dim3((unsigned)((nwork + 255) / 256)), dim3(256), 0, s, in, (op_t*)out, sn_a, sn_ib, Cp, L, ntile, nwork);
    SAT_LAUNCH_CHECK();
    return 0;
}

#if !SAT_OP_IS_F32
template <int BN, int WM, int WN, int NS>
int launch_ru_fused(const RuArgs& a, int B, hipStream_t s) {
    constexpr int LDS = NS * (128 + BN) * 128;
    auto kern = a.c7.act == ACT_ELU ? ru_fused_kernel<BN, WM, WN, NS, ACT_ELU> : ru_fused_kernel<BN, WM, WN, NS, ACT_SNAKE>;
    SAT_TRY(sat_ensure_dynamic_lds(reinterpret_cast<const void*>(kern), LDS));
    hipLaunchKernelGGL(kern, dim3(cdiv(a.c7.M, 128), B), dim3(WM * WN * 64), LDS, s, a);
    SAT_LAUNCH_CHECK();
    return 0;
}
// the whole unit in one launch where its channel count is one workgroup tile; the intermediate never leaves LDS
int launch_ru(const void* ru_args, int B, hipStream_t s) {
    const RuArgs& a = *static_cast<const RuArgs*>(ru_args);
    SAT_CHECK_ARG(a.c7.N == 128 || a.c7.N == 256, SAT_E_UNSUPPORTED, "fused ResidualUnit: %d channels are neither 128 nor 256", a.c7.N);
    // C = 128: a 2-stage ring (64 KiB) puts two workgroups on a CU, so one's epilogues overlap the other's main loop
    if (a.c7.N == 128) return launch_ru_fused<128, 4, 2, 2>(a, B, s);
    return launch_ru_fused<256, 2, 4, 3>(a, B, s);
}
#endif

// ---- finalize: the launches behind each weight kind (weight norm folded: scale[i] = g[i] / ||v[i]||, one float per slice of v)
int launch_pack_conv(const float* v, const float* g, float* scale, void* W, int Cout, int Cin, int k, int Npad, int Kpad, hipStream_t s) {
    hipLaunchKernelGGL(wn_invnorm_kernel, dim3(Cout), dim3(256), 0, s, v, g, scale, Cin * k);
    size_t n = (size_t)k * Npad * Kpad;
    hipLaunchKernelGGL(wn_pack_conv_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, v, scale, (op_t*)W, Cout, Cin, k, Npad, Kpad);
    SAT_LAUNCH_CHECK();
    return 0;
}
int launch_fold_f32(const float* v, const float* g, float* scale, float* w, int Cout, int slice, hipStream_t s) {
    hipLaunchKernelGGL(wn_invnorm_kernel, dim3(Cout), dim3(256), 0, s, v, g, scale, slice);
    size_t n = (size_t)Cout * slice;
    hipLaunchKernelGGL(wn_fold_f32_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, v, scale, w, slice, n);
    SAT_LAUNCH_CHECK();
    return 0;
}
int launch_pack_convT(const float* v, const float* g, float* scale, void* W, int Cin, int Cout, int stride, int Kp, int Np, hipStream_t s) {
    hipLaunchKernelGGL(wn_invnorm_kernel, dim3(Cin), dim3(256), 0, s, v, g, scale, Cout * 2 * stride);
    size_t n = (size_t)2 * stride * Np * Kp;
    hipLaunchKernelGGL(wn_pack_convT_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, v, scale, (op_t*)W, Cin, Cout, stride, Kp, Np);
    SAT_LAUNCH_CHECK();
    return 0;
}
int launch_pack_nearest(const float* v, const float* g, float* scale, void* W, int Cin, int Cout, int stride, int Kp, int Np, hipStream_t s) {
    hipLaunchKernelGGL(wn_invnorm_kernel, dim3(Cout), dim3(256), 0, s, v, g, scale, Cin * 2 * stride);
    size_t n = (size_t)3 * stride * Np * Kp;
    hipLaunchKernelGGL(wn_pack_nearest_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, v, scale, (op_t*)W, Cin, Cout, stride, Kp, Np);
    SAT_LAUNCH_CHECK();
    return 0;
}
int launch_snake_params(const float* alpha, const float* beta, float* a, float* ib, int C, int Cp, hipStream_t s) {
    hipLaunchKernelGGL(snake_params_kernel, dim3(cdiv(Cp, 256)), dim3(256), 0, s, alpha, beta, a, ib, C, Cp);
    SAT_LAUNCH_CHECK();
    return 0;
}

}  // namespace

namespace SAT_OPNS {
const OobKernels* oob_kernels() {
    static const OobKernels k = {
        (int)sizeof(op_t),
        SAT_OP_IS_F32 ? SAT_GEMM_FP32X : SAT_OP_IS_F16 ? SAT_GEMM_FP16 : SAT_GEMM_BF16,
        launch_conv,
#if SAT_OP_IS_F32
        nullptr,      // the 128 x C intermediate would not fit next to the weight ring: two launches through memory
#else
        launch_ru,
#endif
        launch_cf_to_cl,
        launch_first_conv,
        launch_pack_conv,
        launch_fold_f32,
        launch_pack_convT,
        launch_pack_nearest,
        launch_snake_params,
        launch_aa_act,
    };
    return &k;
}
}  // namespace SAT_OPNS

