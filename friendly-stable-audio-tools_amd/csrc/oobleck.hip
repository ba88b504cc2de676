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
// Stage widths that are not multiples of 64 are rounded up inside the plan: weights, biases and Snake parameters are zero-padded at
// finalize, so the pad channels of every activation tensor are written as exact zeros (act(0) = 0) and no kernel masks channels.
#include <math.h>

#include <algorithm>
#include <string>
#include <vector>

#include <stdlib.h>

#include "sat_common.h"
#include "plan_core.h"

namespace {

struct ConvArgs {
    const op_t* in;        // [B][Tin][Cin]
    int Tin, Cin;
    const op_t* W;         // [taps][N][Cin]
    int taps, N, M;          // M GEMM rows per batch item
    int stride, off0, doff;
    const float* bias;       // [Cout] or null ; n -> bias[n % Cout]
    int Cout;
    const op_t* res;       // residual (raw), same indexing as out ; or null
    op_t* out_raw;         // or null
    op_t* out_snk;         // or null
    const float* sn_a;     // exp(alpha)[Cout]
    const float* sn_ib;      // 1/(exp(beta)+1e-9)[Cout]
    long long out_bstride;   // elements per batch item
    long long out_shift;     // flat = m*N + out_shift + n ; valid if 0 <= flat < out_limit
    long long out_limit;
    float* out_cf;           // channel-first fp32 output [B][cf_channels][M] (final convs) or null
    int cf_channels;
    const op_t* zero_page; // >= one K-tile row (ROW_B <= 256 B) of zeros: LDS-DMA source of the rows that fall into the conv padding
    // (the option fields come last: the fields above keep the offsets they had before the options existed)
    int act;                 // activation behind out_snk: ACT_SNAKE (sn_a / sn_ib) or ACT_ELU (no parameters)
    int tanh_out;            // out_cf only: tanh on the result (OobleckDecoder final_tanh)
};

enum { ACT_SNAKE = SAT_OOBLECK_ACT_SNAKE, ACT_ELU = SAT_OOBLECK_ACT_ELU, ACT_RUNTIME = -1 };

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
    if (g.out_cf) {      // fp32 channel-first result of the last convolution: consecutive lanes = consecutive time steps
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
struct RuArgs {
    ConvArgs c7;     // in = snake1(x); bias / sn_a / sn_ib: those of the k = 7 convolution and of the Snake behind it
    ConvArgs c1;     // W / bias of the 1 x 1 convolution, res = raw x, out_raw / out_snk (+ the next layer's Snake)
};

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

int launch_conv(const ConvArgs& a, int B, hipStream_t s) {
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

// the activation in front of a convolution: SnakeBeta with its folded parameters, or ELU (no parameters)
struct Snake {
    float *a = nullptr, *ib = nullptr;
    int act = ACT_SNAKE;
};
inline int pad64(int c) { return (int)round_up(c, 64); }
struct ConvW {
    op_t* W = nullptr;
    float* bias = nullptr;
    int Cin = 0, Cout = 0, taps = 0, N = 0;      // Cin / Cout: the padded widths the kernels see
    const op_t* zero = nullptr;   // the plan's zero page (LDS-DMA source for padding rows)
};

}  // namespace

namespace SAT_OPNS {
struct OobPlan {
    sat_oobleck_cfg cfg;          // first member: the C entry points read cfg.gemm_dtype through the opaque pointer to pick the build
    sat_oobleck_options opt;
    TensorTable tensors;
    bool finalized = false;
    DevBuf arena;
    int ratio = 1;
    std::vector<int> chans;   // channels after each stage, decoder order or encoder order
    // decoder / encoder share the block structure
    ConvW first, last;
    float* first_w_f32 = nullptr;   // encoder first conv (VALU)
    struct Block {
        Snake sn_in;             // decoder: block snake before convT ; encoder: snake before strided conv
        ConvW resample;          // convT (decoder) / strided conv (encoder)
        Snake ru_sn1[3], ru_sn2[3];
        ConvW ru_c7[3], ru_c1[3];
        int stride, cin, cout;   // cin / cout: padded to multiples of 64
    };
    std::vector<Block> blocks;
    Snake final_snake;
    op_t* zero_page = nullptr;
    // optional fp16 range report (sat_oobleck_range_report): one record per activation tensor a run writes to the workspace, in launch order;
    // the names are fixed by the blocks (oob_plan_create), the records exist while the report is on
    std::vector<std::string> rr_names;
    DevBuf rr_buf;
    sat_range_record* rr = nullptr;
};
}  // namespace SAT_OPNS
using SAT_OPNS::OobPlan;

namespace {

int get_tensor(OobPlan* p, const std::string& name, int64_t numel, const float** out) { return p->tensors.get("oobleck", name, numel, out); }

int make_snake(OobPlan* p, Bump& ar, const std::string& pfx, int C, Snake* sn, hipStream_t s) {
    sn->act = p->opt.activation;
    if (sn->act == ACT_ELU) return 0;        // nn.ELU has no tensors: nothing to ask for
    const int Cp = pad64(C);
    sn->a = (float*)ar.take((size_t)Cp * 4);
    sn->ib = (float*)ar.take((size_t)Cp * 4);
    if (ar.dry()) return 0;
    const float *al, *be;
    SAT_TRY(get_tensor(p, pfx + "alpha", C, &al));
    SAT_TRY(get_tensor(p, pfx + "beta", C, &be));
    hipLaunchKernelGGL(snake_params_kernel, dim3(cdiv(Cp, 256)), dim3(256), 0, s, al, be, sn->a, sn->ib, C, Cp);
    SAT_LAUNCH_CHECK();
    return 0;
}

// bias[Cp]: the tensor's C values, then zeros
int make_bias(OobPlan* p, Bump& ar, const std::string& name, int C, float** out, hipStream_t s) {
    const int Cp = pad64(C);
    *out = (float*)ar.take((size_t)Cp * 4);
    if (ar.dry()) return 0;
    if (Cp > C) SAT_HIP(hipMemsetAsync(*out + C, 0, (size_t)(Cp - C) * 4, s));
    return p->tensors.copy("oobleck", name, C, *out, s);
}

// Conv1d weight [Cout][Cin][k]
int make_conv(OobPlan* p, Bump& ar, const std::string& pfx, int Cin, int Cout, int k, bool has_bias, ConvW* cw,
              hipStream_t s, float** w_f32 = nullptr) {
    const int Npad = pad64(Cout), Kpad = pad64(Cin);
    cw->Cin = Kpad; cw->Cout = Npad; cw->taps = k; cw->N = Npad; cw->zero = p->zero_page;
    float* scale = (float*)ar.take((size_t)Cout * 4);
    if (w_f32) *w_f32 = (float*)ar.take((size_t)Cout * Cin * k * 4);
    else cw->W = (op_t*)ar.take((size_t)k * Npad * Kpad * sizeof(op_t));
    cw->bias = nullptr;
    if (has_bias) SAT_TRY(make_bias(p, ar, pfx + "bias", Cout, &cw->bias, s));
    if (ar.dry()) return 0;
    const float *g, *v;
    SAT_TRY(get_tensor(p, pfx + "weight_g", Cout, &g));
    SAT_TRY(get_tensor(p, pfx + "weight_v", (int64_t)Cout * Cin * k, &v));
    hipLaunchKernelGGL(wn_invnorm_kernel, dim3(Cout), dim3(256), 0, s, v, g, scale, Cin * k);
    if (w_f32) {
        size_t n = (size_t)Cout * Cin * k;
        hipLaunchKernelGGL(wn_fold_f32_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, v, scale, *w_f32, Cin * k, n);
    } else {
        size_t n = (size_t)k * Npad * Kpad;
        hipLaunchKernelGGL(wn_pack_conv_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, v, scale, cw->W, Cout, Cin, k, Npad,
                           Kpad);
    }
    SAT_LAUNCH_CHECK();
    return 0;
}

// ConvTranspose1d weight [Cin][Cout][2s]
int make_convT(OobPlan* p, Bump& ar, const std::string& pfx, int Cin, int Cout, int stride, ConvW* cw, hipStream_t s) {
    const int Kp = pad64(Cin), Np = pad64(Cout);
    cw->Cin = Kp; cw->Cout = Np; cw->taps = 2; cw->N = stride * Np; cw->zero = p->zero_page;
    float* scale = (float*)ar.take((size_t)Cin * 4);
    cw->W = (op_t*)ar.take((size_t)2 * cw->N * Kp * sizeof(op_t));
    SAT_TRY(make_bias(p, ar, pfx + "bias", Cout, &cw->bias, s));
    if (ar.dry()) return 0;
    const float *g, *v;
    SAT_TRY(get_tensor(p, pfx + "weight_g", Cin, &g));
    SAT_TRY(get_tensor(p, pfx + "weight_v", (int64_t)Cin * Cout * 2 * stride, &v));
    hipLaunchKernelGGL(wn_invnorm_kernel, dim3(Cin), dim3(256), 0, s, v, g, scale, Cout * 2 * stride);
    size_t n = (size_t)2 * cw->N * Kp;
    hipLaunchKernelGGL(wn_pack_convT_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, v, scale, cw->W, Cin, Cout, stride, Kp,
                       Np);
    SAT_LAUNCH_CHECK();
    return 0;
}

// Upsample(nearest, s) + bias-free Conv1d weight [Cout][Cin][2s] -> the three-tap polyphase form
int make_nearest(OobPlan* p, Bump& ar, const std::string& pfx, int Cin, int Cout, int stride, ConvW* cw, hipStream_t s) {
    const int Kp = pad64(Cin), Np = pad64(Cout);
    cw->Cin = Kp; cw->Cout = Np; cw->taps = 3; cw->N = stride * Np; cw->zero = p->zero_page;
    float* scale = (float*)ar.take((size_t)Cout * 4);
    cw->W = (op_t*)ar.take((size_t)3 * cw->N * Kp * sizeof(op_t));
    cw->bias = nullptr;
    if (ar.dry()) return 0;
    const float *g, *v;
    SAT_TRY(get_tensor(p, pfx + "weight_g", Cout, &g));
    SAT_TRY(get_tensor(p, pfx + "weight_v", (int64_t)Cout * Cin * 2 * stride, &v));
    hipLaunchKernelGGL(wn_invnorm_kernel, dim3(Cout), dim3(256), 0, s, v, g, scale, Cin * 2 * stride);
    size_t n = (size_t)3 * cw->N * Kp;
    hipLaunchKernelGGL(wn_pack_nearest_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, v, scale, cw->W, Cin, Cout, stride, Kp,
                       Np);
    SAT_LAUNCH_CHECK();
    return 0;
}

int make_ru(OobPlan* p, Bump& ar, const std::string& pfx, int C, OobPlan::Block& blk, int r, hipStream_t s) {
    SAT_TRY(make_snake(p, ar, pfx + "layers.0.", C, &blk.ru_sn1[r], s));
    SAT_TRY(make_conv(p, ar, pfx + "layers.1.", C, C, 7, true, &blk.ru_c7[r], s));
    SAT_TRY(make_snake(p, ar, pfx + "layers.2.", C, &blk.ru_sn2[r], s));
    SAT_TRY(make_conv(p, ar, pfx + "layers.3.", C, C, 1, true, &blk.ru_c1[r], s));
    return 0;
}

int build(OobPlan* p, Bump& ar, hipStream_t s) {
    const sat_oobleck_cfg& c = p->cfg;
    const int nb = c.n_blocks;
    p->blocks.resize(nb);
    p->zero_page = (op_t*)ar.take(256);
    if (!ar.dry()) SAT_HIP(hipMemsetAsync(p->zero_page, 0, 256, s));
    if (c.is_decoder) {
        // autoencoders.py:174-191: channel list c_mults=[1]+c_mults ; blocks from deepest to shallowest
        const int ctop = c.c_mults[nb - 1] * c.channels;
        SAT_TRY(make_conv(p, ar, "layers.0.", c.latent_dim, ctop, 7, true, &p->first, s));
        for (int bi = 0; bi < nb; ++bi) {
            const int i = nb - bi;   // reference loop index: range(depth-1, 0, -1)
            auto& blk = p->blocks[bi];
            const int cin = c.c_mults[i - 1] * c.channels;
            const int cout = (i - 2 >= 0 ? c.c_mults[i - 2] : 1) * c.channels;
            blk.cin = pad64(cin);
            blk.cout = pad64(cout);
            blk.stride = c.strides[i - 1];
            const std::string pf = "layers." + std::to_string(bi + 1) + ".";
            SAT_TRY(make_snake(p, ar, pf + "layers.0.", cin, &blk.sn_in, s));
            if (p->opt.nearest_upsample)      // Sequential(Upsample, WNConv1d): the convolution is layers.1.1
                SAT_TRY(make_nearest(p, ar, pf + "layers.1.1.", cin, cout, blk.stride, &blk.resample, s));
            else
                SAT_TRY(make_convT(p, ar, pf + "layers.1.", cin, cout, blk.stride, &blk.resample, s));
            for (int r = 0; r < 3; ++r) SAT_TRY(make_ru(p, ar, pf + "layers." + std::to_string(2 + r) + ".", cout, blk, r, s));
        }
        SAT_TRY(make_snake(p, ar, "layers." + std::to_string(nb + 1) + ".", c.channels, &p->final_snake, s));
        SAT_TRY(make_conv(p, ar, "layers." + std::to_string(nb + 2) + ".", c.channels, c.io_channels, 7, false, &p->last, s));
    } else {
        // autoencoders.py:131-151
        SAT_TRY(make_conv(p, ar, "layers.0.", c.io_channels, c.channels, 7, true, &p->first, s, &p->first_w_f32));
        for (int bi = 0; bi < nb; ++bi) {
            auto& blk = p->blocks[bi];
            const int cin = (bi == 0 ? 1 : c.c_mults[bi - 1]) * c.channels;
            const int cout = c.c_mults[bi] * c.channels;
            blk.cin = pad64(cin);
            blk.cout = pad64(cout);
            blk.stride = c.strides[bi];
            const std::string pf = "layers." + std::to_string(bi + 1) + ".";
            for (int r = 0; r < 3; ++r) SAT_TRY(make_ru(p, ar, pf + "layers." + std::to_string(r) + ".", cin, blk, r, s));
            SAT_TRY(make_snake(p, ar, pf + "layers.3.", cin, &blk.sn_in, s));
            SAT_TRY(make_conv(p, ar, pf + "layers.4.", cin, cout, 2 * blk.stride, true, &blk.resample, s));
        }
        const int ctop = c.c_mults[nb - 1] * c.channels;
        SAT_TRY(make_snake(p, ar, "layers." + std::to_string(nb + 1) + ".", ctop, &p->final_snake, s));
        SAT_TRY(make_conv(p, ar, "layers." + std::to_string(nb + 2) + ".", ctop, c.latent_dim, 3, true, &p->last, s));
    }
    return 0;
}

struct Bufs {
    op_t *R, *S0, *S1, *Y;
    size_t total;
};
Bufs carve(const OobPlan* p, int B, int T, char* base) {
    // largest channels-last tensor of the network (padded widths), in elements per batch item
    const sat_oobleck_cfg& c = p->cfg;
    size_t len = (size_t)T, mx = 0;
    if (c.is_decoder) {
        mx = std::max((size_t)T * pad64(c.latent_dim), (size_t)T * p->blocks[0].cin);
        for (auto& b : p->blocks) {
            len *= b.stride;
            mx = std::max(mx, len * b.cout);
        }
    } else {
        len = (size_t)T * p->ratio;
        mx = len * pad64(c.channels);
        for (auto& b : p->blocks) {
            mx = std::max(mx, len * b.cin);
            len /= b.stride;
            mx = std::max(mx, len * b.cout);
        }
    }
    size_t per = (size_t)round_up((int64_t)(mx * B * sizeof(op_t)), 256);
    Bufs o;
    o.R = (op_t*)(base ? base : nullptr);
    o.S0 = (op_t*)(base ? base + per : nullptr);
    o.S1 = (op_t*)(base ? base + 2 * per : nullptr);
    o.Y = (op_t*)(base ? base + 3 * per : nullptr);
    o.total = 4 * per;
    return o;
}

ConvArgs base_args(const ConvW& w, const op_t* in, int Tin, int M) {
    ConvArgs a{};
    a.zero_page = w.zero;
    a.in = in; a.Tin = Tin; a.Cin = w.Cin; a.W = w.W; a.taps = w.taps; a.N = w.N; a.M = M;
    a.stride = 1; a.off0 = 0; a.doff = 1; a.bias = w.bias; a.Cout = w.Cout;
    a.out_bstride = (long long)M * w.N; a.out_shift = 0; a.out_limit = (long long)M * w.N;
    return a;
}

// out = the activated copy of the result, for the consumer whose activation is sn
void set_act(ConvArgs& a, op_t* out, const Snake& sn) {
    a.out_snk = out; a.act = sn.act; a.sn_a = sn.a; a.sn_ib = sn.ib;
}

// ---- the ConvArgs of each layer kind.  oob_decode / oob_encode and the unit-level entry (oob_unit) both build their launches from these, so
// a test of one layer runs the very off0 / doff / stride / M / out_shift / out_limit / out_bstride the plan runs
// k-tap convolution over the rows' own length, padding k / 2: the decoder's first and last k = 7, the encoder's last k = 3
ConvArgs same_conv_args(const ConvW& w, const op_t* in, int L) {
    ConvArgs a = base_args(w, in, L, L);
    a.off0 = -(w.taps / 2);
    return a;
}
// the last convolution of either direction: fp32 channel-first result, the first `channels` columns; tanh by option (decoder)
ConvArgs final_conv_args(const ConvW& w, const op_t* in, int L, float* out_cf, int channels, int tanh_out) {
    ConvArgs a = same_conv_args(w, in, L);
    a.out_cf = out_cf; a.cf_channels = channels; a.tanh_out = tanh_out;
    return a;
}
// the dilated k = 7 convolution of a ResidualUnit (autoencoders.py:56)
ConvArgs ru_c7_args(const ConvW& w, const op_t* S, int L, int dil) {
    ConvArgs a = base_args(w, S, L, L);
    a.off0 = -3 * dil; a.doff = dil;
    return a;
}
// its 1 x 1 convolution: adds the raw x in R; the sum returns to R in place where a later unit needs it
ConvArgs ru_c1_args(const ConvW& w, const op_t* Y, int L, op_t* R, bool need_raw) {
    ConvArgs c = base_args(w, Y, L, L);
    c.res = R;
    c.out_raw = need_raw ? R : nullptr;   // in place: each thread reads then writes its own elements
    return c;
}
// a decoder block's upsampler, L rows -> L * st rows of w.Cout channels:
// transposed conv (autoencoders.py:102-105): rows m = 0..L, output row span (m*st - pad)*Cout, taps at rows m, m-1;
// nearest upsample + conv (:95-99): rows m = 0..L-1, output row span m*st*Cout, taps at rows m-1, m, m+1
ConvArgs upsample_args(const ConvW& w, const op_t* S, int L, int st, bool nearest) {
    const int pad = (st + 1) / 2;
    ConvArgs a = base_args(w, S, L, nearest ? L : L + 1);
    a.off0 = nearest ? -1 : 0; a.doff = nearest ? 1 : -1;
    a.out_bstride = (long long)L * st * w.Cout;
    a.out_shift = nearest ? 0 : -(long long)pad * w.Cout;
    a.out_limit = (long long)L * st * w.Cout;
    return a;
}
// an encoder block's strided convolution (autoencoders.py:80-81), L rows -> L / st rows
ConvArgs strided_args(const ConvW& w, const op_t* S, int L, int st) {
    ConvArgs a = base_args(w, S, L, L / st);
    a.stride = st; a.off0 = -((st + 1) / 2); a.doff = 1;
    return a;
}

// What the plan's length bookkeeping can run: a block turns L rows into L * st (decoder) or L / st (encoder).  The reference's
// ConvTranspose1d(k = 2 st, stride st, padding ceil(st / 2)) yields L * st + st - 2 ceil(st / 2) rows, which is L * st - 1 at odd st, and its
// encoder convolution yields L + 1 rows at st = 1; Upsample(st) + Conv1d("same") and the strided convolution at st >= 2 keep the plan's lengths.
bool resample_stride_ok(bool is_decoder, bool nearest, int st) {
    if (st < 1 || st > 16) return false;
    if (is_decoder) return nearest || st % 2 == 0;
    return st >= 2;
}

int launch_cf_to_cl(const float* z, op_t* y, int C, int T, int B, hipStream_t s) {
    hipLaunchKernelGGL(cf_to_cl_kernel, dim3(cdiv(T, 64), pad64(C) / 64, B), dim3(256), 0, s, z, y, C, pad64(C), T);
    SAT_LAUNCH_CHECK();
    return 0;
}

// the encoder's first convolution (VALU): C channels out of Cin <= 2, raw and activated (sn0) rows of pad64(C) channels
int launch_first_conv(const float* audio, const float* w_f32, const ConvW& first, const Snake& sn0, op_t* raw, op_t* snk, int Cin, int C,
                      int L, int B, hipStream_t s) {
    const bool general = sn0.act != ACT_SNAKE || pad64(C) != C;
    hipLaunchKernelGGL(general ? first_conv_kernel<true> : first_conv_kernel<false>, dim3(cdiv(L, 64), B), dim3(256), 0, s, audio, w_f32,
                       first.bias, sn0.a, sn0.ib, sn0.act, raw, snk, Cin, C, pad64(C), L);
    SAT_LAUNCH_CHECK();
    return 0;
}

// The range report of one run: the next record takes the contiguous tensor of n elements at buf, right behind the launch that wrote it (the
// four workspace buffers are reused all along).  The order of the calls is the order of range_names
struct Ranger {
    const OobPlan* p;
    hipStream_t s;
    int next = 0;
    bool unfused = false;      // the unit-level entry's switch: the two-launch route without a report
    bool on() const { return p->rr != nullptr; }
    bool two_launches() const { return on() || unfused; }
    int operator()(const op_t* buf, size_t n) {
        if (!on()) return 0;
        SAT_CHECK_ARG(next < (int)p->rr_names.size(), SAT_E_STATE, "oobleck range report: more tensors than records (%d)", next);
        return sat_launch_range_stats(buf, SAT_OP_IS_F32 ? SAT_GEMM_FP32X : SAT_OP_IS_F16 ? SAT_GEMM_FP16 : SAT_GEMM_BF16, 1, (int64_t)n, (int64_t)n, n,
                                      p->rr + next++, s);
    }
    int done() const {
        SAT_CHECK_ARG(!on() || next == (int)p->rr_names.size(), SAT_E_STATE, "oobleck range report: %d tensors for %d records", next, (int)p->rr_names.size());
        return 0;
    }
};

// The records of a plan in launch order (sat_oobleck_range_report_name): the module path of the layer whose launch writes the tensor -- the
// activated tensor the next convolution reads, then "<path>.raw" where the launch also keeps the un-activated sum for the next residual add
std::vector<std::string> range_names(const sat_oobleck_cfg& c, const sat_oobleck_options& o) {
    std::vector<std::string> n;
    auto both = [&](const std::string& path, bool raw) {
        n.push_back(path);
        if (raw) n.push_back(path + ".raw");
    };
    auto unit = [&](const std::string& ru, int r) {
        n.push_back(ru + "layers.1");
        both(ru + "layers.3", r < 2);
    };
    const int nb = c.n_blocks;
    if (c.is_decoder) {
        n.push_back("input");
        n.push_back("layers.0");
        for (int bi = 0; bi < nb; ++bi) {
            const std::string pf = "layers." + std::to_string(bi + 1) + ".";
            both(pf + (o.nearest_upsample ? "layers.1.1" : "layers.1"), true);
            for (int r = 0; r < 3; ++r) unit(pf + "layers." + std::to_string(2 + r) + ".", r);
        }
    } else {
        both("layers.0", true);
        for (int bi = 0; bi < nb; ++bi) {
            const std::string pf = "layers." + std::to_string(bi + 1) + ".";
            for (int r = 0; r < 3; ++r) unit(pf + "layers." + std::to_string(r) + ".", r);
            both(pf + "layers.4", bi + 1 < nb);
        }
    }
    return n;
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
#endif

// one ResidualUnit (autoencoders.py:45-68): in S (snaked x) + R (raw x) -> R (raw x') and/or Sout (snake_next(x'))
// With the range report on, every unit takes the two launches: the tensor between its convolutions then reaches memory (Y) and has a record
int run_ru(const OobPlan::Block& blk, int r, int C, int L, int B, op_t* R, const op_t* S, op_t* Y, op_t* Sout,
           const Snake& next, bool need_raw, hipStream_t s, Ranger& rg) {
    static const int dil[3] = {1, 3, 9};
    ConvArgs a = ru_c7_args(blk.ru_c7[r], S, L, dil[r]);
    set_act(a, Y, blk.ru_sn2[r]);
    ConvArgs c = ru_c1_args(blk.ru_c1[r], Y, L, R, need_raw);
    set_act(c, Sout, next);
#if !SAT_OP_IS_F32      // (fp32 build: the 128 x C intermediate would not fit next to the weight ring; two launches through Y)
    if ((C == 128 || C == 256) && !rg.two_launches()) {      // the whole unit in one launch, the intermediate never leaves LDS
        RuArgs f{a, c};
        f.c7.out_snk = nullptr;
        f.c1.in = nullptr;
        // C = 128: a 2-stage ring (64 KiB) puts two workgroups on a CU, so one's epilogues overlap the other's main loop
        if (C == 128) return launch_ru_fused<128, 4, 2, 2>(f, B, s);
        return launch_ru_fused<256, 2, 4, 3>(f, B, s);
    }
#endif
    const size_t n = (size_t)B * L * C;
    SAT_TRY(launch_conv(a, B, s));
    SAT_TRY(rg(Y, n));
    SAT_TRY(launch_conv(c, B, s));
    SAT_TRY(rg(Sout, n));
    return need_raw ? rg(R, n) : 0;
}

}  // namespace

namespace SAT_OPNS {

// (the options were validated by sat_oobleck_plan_create_ex; channel counts are free: the plan pads every width to a multiple of 64)
int oob_plan_create(const sat_oobleck_cfg* cfg, const sat_oobleck_options* opt, OobPlan** out_plan) {
    SAT_CHECK_ARG(cfg && opt && out_plan, SAT_E_INVALID, "oobleck_plan_create: null argument");
    SAT_CHECK_ARG(cfg->n_blocks >= 1 && cfg->n_blocks <= 8, SAT_E_UNSUPPORTED, "oobleck_plan_create: n_blocks %d not in 1..8", cfg->n_blocks);
    SAT_CHECK_ARG(cfg->channels > 0, SAT_E_UNSUPPORTED, "oobleck_plan_create: channels %d must be positive", cfg->channels);
    SAT_CHECK_ARG(cfg->io_channels >= 1 && cfg->io_channels <= 2, SAT_E_UNSUPPORTED, "oobleck_plan_create: io_channels must be 1 or 2");
    SAT_CHECK_ARG(cfg->latent_dim > 0, SAT_E_UNSUPPORTED, "oobleck_plan_create: latent_dim %d must be positive", cfg->latent_dim);
    OobPlan* p = new (std::nothrow) OobPlan();
    SAT_CHECK_ARG(p, SAT_E_INVALID, "oobleck_plan_create: out of host memory");
    p->cfg = *cfg;
    p->opt = *opt;
    p->rr_names = range_names(*cfg, *opt);
    p->ratio = 1;
    for (int i = 0; i < cfg->n_blocks; ++i) {
        SAT_CHECK_ARG(cfg->strides[i] >= 1 && cfg->strides[i] <= 16 && cfg->c_mults[i] >= 1, SAT_E_UNSUPPORTED, "oobleck_plan_create: bad stride/c_mult");
        SAT_CHECK_ARG(resample_stride_ok(cfg->is_decoder != 0, opt->nearest_upsample != 0, cfg->strides[i]), SAT_E_UNSUPPORTED,
                      "oobleck_plan_create: stride %d of block %d is not supported: the reference's %s", cfg->strides[i], i,
                      cfg->is_decoder ? "ConvTranspose1d yields L * stride - 1 samples at an odd stride, the plan L * stride (nearest_upsample takes odd strides)"
                                      : "stride-1 encoder convolution (k = 2, padding 1) yields L + 1 samples, the plan L");
        p->ratio *= cfg->strides[i];
    }
    *out_plan = p;
    return 0;
}

void oob_plan_destroy(OobPlan* p) { delete p; }

int oob_plan_set_tensor(OobPlan* p, const char* name, const float* data_dev, int64_t numel) {
    SAT_CHECK_ARG(p, SAT_E_INVALID, "oobleck_plan_set_tensor: bad argument");
    return p->tensors.set("oobleck", name, data_dev, numel);
}

int oob_plan_finalize(OobPlan* p, sat_stream_t stream) {
    SAT_CHECK_ARG(p, SAT_E_INVALID, "oobleck_plan_finalize: null plan");
    hipStream_t s = (hipStream_t)stream;
    return plan_finalize(p, s, [&](Bump& ar) { return build(p, ar, s); });
}

int oob_workspace_bytes(const OobPlan* p, int32_t b, int32_t t_len, size_t* out_bytes) {
    SAT_CHECK_ARG(p && out_bytes && b > 0 && t_len > 0, SAT_E_INVALID, "oobleck_workspace_bytes: bad argument");
    SAT_CHECK_ARG(p->finalized, SAT_E_STATE, "oobleck_workspace_bytes: plan not finalized");
    *out_bytes = carve(p, b, t_len, nullptr).total;
    return 0;
}

int oob_decode(OobPlan* p, const float* z, float* audio, int32_t B, int32_t T, void* ws, size_t ws_bytes,
                                  sat_stream_t stream) {
    SAT_CHECK_ARG(p && p->finalized && p->cfg.is_decoder, SAT_E_STATE, "oobleck_decode: not a finalized decoder plan");
    SAT_CHECK_ARG(z && audio && ws && B > 0 && T > 0, SAT_E_INVALID, "oobleck_decode: bad arguments");
    SAT_CHECK_ARG(((uintptr_t)ws & 255) == 0, SAT_E_INVALID, "oobleck_decode: workspace must be 256-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    Bufs bf = carve(p, B, T, (char*)ws);
    SAT_CHECK_ARG(ws_bytes >= bf.total, SAT_E_WORKSPACE, "oobleck_decode: workspace %zu < required %zu", ws_bytes, bf.total);
    const sat_oobleck_cfg& c = p->cfg;
    const int nb = c.n_blocks;
    // latents -> channels-last bf16 (in Y), first conv (autoencoders.py:175) -> S0 = snake_block1(x)
    SAT_TRY(launch_cf_to_cl(z, bf.Y, c.latent_dim, T, B, s));
    Ranger rg{p, s};
    SAT_TRY(rg(bf.Y, (size_t)B * T * pad64(c.latent_dim)));
    op_t* S = bf.S0;
    op_t* Sn = bf.S1;
    {
        ConvArgs a = same_conv_args(p->first, bf.Y, T);
        set_act(a, S, p->blocks[0].sn_in);
        SAT_TRY(launch_conv(a, B, s));
        SAT_TRY(rg(S, (size_t)B * T * p->first.Cout));
    }
    int L = T;
    for (int bi = 0; bi < nb; ++bi) {
        const auto& blk = p->blocks[bi];
        const int st = blk.stride;
        ConvArgs a = upsample_args(blk.resample, S, L, st, p->opt.nearest_upsample != 0);
        a.out_raw = bf.R;
        set_act(a, Sn, blk.ru_sn1[0]);
        SAT_TRY(launch_conv(a, B, s));
        std::swap(S, Sn);
        L *= st;
        SAT_TRY(rg(S, (size_t)B * L * blk.cout));
        SAT_TRY(rg(bf.R, (size_t)B * L * blk.cout));
        for (int r = 0; r < 3; ++r) {
            const Snake& next = r < 2 ? blk.ru_sn1[r + 1] : (bi + 1 < nb ? p->blocks[bi + 1].sn_in : p->final_snake);
            SAT_TRY(run_ru(blk, r, blk.cout, L, B, bf.R, S, bf.Y, Sn, next, r < 2, s, rg));
            std::swap(S, Sn);
        }
    }
    // final conv (autoencoders.py:187-188): no bias, tanh by option -> fp32 channel-first audio
    ConvArgs a = final_conv_args(p->last, S, L, audio, c.io_channels, p->opt.final_tanh);
    SAT_TRY(launch_conv(a, B, s));
    return rg.done();
}

int oob_encode(OobPlan* p, const float* audio, float* out, int32_t B, int32_t T, void* ws,
                                  size_t ws_bytes, sat_stream_t stream) {
    SAT_CHECK_ARG(p && p->finalized && !p->cfg.is_decoder, SAT_E_STATE, "oobleck_encode: not a finalized encoder plan");
    SAT_CHECK_ARG(audio && out && ws && B > 0 && T > 0, SAT_E_INVALID, "oobleck_encode: bad arguments");
    SAT_CHECK_ARG(((uintptr_t)ws & 255) == 0, SAT_E_INVALID, "oobleck_encode: workspace must be 256-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    Bufs bf = carve(p, B, T, (char*)ws);
    SAT_CHECK_ARG(ws_bytes >= bf.total, SAT_E_WORKSPACE, "oobleck_encode: workspace %zu < required %zu", ws_bytes, bf.total);
    const sat_oobleck_cfg& c = p->cfg;
    const int nb = c.n_blocks;
    int L = T * p->ratio;
    op_t* S = bf.S0;
    op_t* Sn = bf.S1;
    const Snake& sn0 = p->blocks[0].ru_sn1[0];
    SAT_TRY(launch_first_conv(audio, p->first_w_f32, p->first, sn0, bf.R, S, c.io_channels, c.channels, L, B, s));
    Ranger rg{p, s};
    SAT_TRY(rg(S, (size_t)B * L * pad64(c.channels)));
    SAT_TRY(rg(bf.R, (size_t)B * L * pad64(c.channels)));
    for (int bi = 0; bi < nb; ++bi) {
        const auto& blk = p->blocks[bi];
        for (int r = 0; r < 3; ++r) {
            const Snake& next = r < 2 ? blk.ru_sn1[r + 1] : blk.sn_in;
            SAT_TRY(run_ru(blk, r, blk.cin, L, B, bf.R, S, bf.Y, Sn, next, r < 2, s, rg));
            std::swap(S, Sn);
        }
        const int st = blk.stride;
        const int Lo = L / st;
        ConvArgs a = strided_args(blk.resample, S, L, st);
        const bool lastb = bi + 1 == nb;
        a.out_raw = lastb ? nullptr : bf.R;
        const Snake& nx = lastb ? p->final_snake : p->blocks[bi + 1].ru_sn1[0];
        set_act(a, Sn, nx);
        SAT_TRY(launch_conv(a, B, s));
        std::swap(S, Sn);
        L = Lo;
        SAT_TRY(rg(S, (size_t)B * L * blk.cout));
        if (!lastb) SAT_TRY(rg(bf.R, (size_t)B * L * blk.cout));
    }
    ConvArgs a = final_conv_args(p->last, S, L, out, c.latent_dim, 0);
    SAT_TRY(launch_conv(a, B, s));
    return rg.done();
}

// ---- sat_oobleck_range_report and its companions, per build
int oob_range_report(OobPlan* p, int32_t enable) {
    SAT_CHECK_ARG(enable >= 0 && enable <= 2, SAT_E_INVALID, "oobleck_range_report: enable must be 0 (off), 1 (on) or 2 (zero the records), got %d", enable);
    if (enable == 0) {
        if (!p->rr) return 0;
        SAT_HIP(hipDeviceSynchronize());          // launches in flight still accumulate into the records
        p->rr_buf.release();
        p->rr = nullptr;
        return 0;
    }
    SAT_CHECK_ARG(sat_launch_range_stats, SAT_E_UNSUPPORTED, "oobleck_range_report: built without the range statistics kernel");
    const size_t bytes = p->rr_names.size() * sizeof(sat_range_record);
    if (enable == 2) {
        SAT_CHECK_ARG(p->rr, SAT_E_STATE, "oobleck_range_report: the report is not enabled, there is nothing to zero");
        SAT_HIP(hipDeviceSynchronize());
        SAT_HIP(hipMemset(p->rr, 0, bytes));
        return 0;
    }
    if (p->rr) return 0;          // already on: the records keep accumulating
    SAT_TRY(p->rr_buf.reserve(bytes));
    SAT_HIP(hipMemset(p->rr_buf.ptr, 0, bytes));
    p->rr = (sat_range_record*)p->rr_buf.ptr;
    return 0;
}

int oob_range_report_count(OobPlan* p, int32_t* out_records) {
    SAT_CHECK_ARG(out_records, SAT_E_INVALID, "oobleck_range_report_count: null argument");
    *out_records = (int32_t)p->rr_names.size();
    return 0;
}

const char* oob_range_report_name(OobPlan* p, int32_t index) {
    return index >= 0 && index < (int32_t)p->rr_names.size() ? p->rr_names[index].c_str() : nullptr;
}

int oob_range_report_read(OobPlan* p, sat_range_record* out_host, int32_t capacity_records, size_t record_bytes, sat_stream_t stream) {
    SAT_CHECK_ARG(out_host, SAT_E_INVALID, "oobleck_range_report_read: null argument");
    SAT_CHECK_ARG(record_bytes == sizeof(sat_range_record), SAT_E_INVALID,
                  "oobleck_range_report_read: sat_range_record of %zu bytes; this library knows %zu", record_bytes, sizeof(sat_range_record));
    const int n = (int)p->rr_names.size();
    SAT_CHECK_ARG(capacity_records >= n, SAT_E_INVALID, "oobleck_range_report_read: room for %d records, need %d", capacity_records, n);
    SAT_CHECK_ARG(p->rr, SAT_E_STATE, "oobleck_range_report_read: the report is not enabled (sat_oobleck_range_report)");
    SAT_HIP(hipMemcpyAsync(out_host, p->rr, (size_t)n * sizeof(sat_range_record), hipMemcpyDeviceToHost, (hipStream_t)stream));
    SAT_HIP(hipStreamSynchronize((hipStream_t)stream));
    return 0;
}

// ---- sat_oobleck_unit: one layer on the caller's tensors (tests).  A plan object of its own holds the caller's fp32 tensors under fixed
// names ("conv." / "act.": the layer and the activation behind it; "conv2." / "act2.": a ResidualUnit's 1 x 1 convolution and the activation
// behind the unit), plan_finalize runs the make_* the plan's build() would run for that layer, and the launch goes through the helpers above
int oob_unit(const sat_oobleck_unit_desc* u, sat_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    const int kind = u->kind, B = u->b, L = u->t_len, Ci = u->c_in, Co = u->c_out, st = u->stride;
    SAT_CHECK_ARG(kind >= SAT_OOBLECK_UNIT_CONV7 && kind <= SAT_OOBLECK_UNIT_CF_TO_CL, SAT_E_UNSUPPORTED, "oobleck_unit: unknown kind %d", kind);
    SAT_CHECK_ARG(u->activation == ACT_SNAKE || u->activation == ACT_ELU, SAT_E_UNSUPPORTED, "oobleck_unit: unknown activation %d", u->activation);
    SAT_CHECK_ARG(B > 0 && L > 0 && Ci > 0 && (Co > 0 || kind == SAT_OOBLECK_UNIT_CF_TO_CL), SAT_E_INVALID, "oobleck_unit: b, t_len, c_in, c_out must be positive");
    const bool resample = kind == SAT_OOBLECK_UNIT_CONVT || kind == SAT_OOBLECK_UNIT_NEAREST || kind == SAT_OOBLECK_UNIT_STRIDED;
    const bool dilated = kind == SAT_OOBLECK_UNIT_CONV7 || kind == SAT_OOBLECK_UNIT_RESIDUAL;
    const bool residual = kind == SAT_OOBLECK_UNIT_CONV1_RES || kind == SAT_OOBLECK_UNIT_RESIDUAL;
    const bool from_cf = kind == SAT_OOBLECK_UNIT_FIRST_CONV || kind == SAT_OOBLECK_UNIT_CF_TO_CL;
    const bool to_cf = kind == SAT_OOBLECK_UNIT_FINAL_DEC || kind == SAT_OOBLECK_UNIT_FINAL_ENC;
    if (resample) {
        SAT_CHECK_ARG(resample_stride_ok(kind != SAT_OOBLECK_UNIT_STRIDED, kind == SAT_OOBLECK_UNIT_NEAREST, st), SAT_E_UNSUPPORTED,
                      "oobleck_unit: stride %d is outside what a plan runs for kind %d", st, kind);
        SAT_CHECK_ARG(kind != SAT_OOBLECK_UNIT_STRIDED || L % st == 0, SAT_E_INVALID, "oobleck_unit: t_len %d is no multiple of stride %d", L, st);
    }
    const int r = u->dilation == 1 ? 0 : u->dilation == 3 ? 1 : 2;
    SAT_CHECK_ARG(!dilated || u->dilation == 1 || u->dilation == 3 || u->dilation == 9, SAT_E_UNSUPPORTED, "oobleck_unit: dilation %d is not 1, 3 or 9", u->dilation);
    SAT_CHECK_ARG(!residual || (Ci == Co && u->res && (!u->out_raw || u->out_raw == u->res) && u->out_snk), SAT_E_INVALID,
                  "oobleck_unit: a residual layer needs c_in == c_out, res, out_snk, and out_raw NULL or == res");
    SAT_CHECK_ARG(kind != SAT_OOBLECK_UNIT_FIRST_CONV || (Ci <= 2 && u->out_raw && u->out_snk), SAT_E_INVALID,
                  "oobleck_unit: the first convolution takes 1 or 2 channels and writes out_raw and out_snk");
    SAT_CHECK_ARG(from_cf ? u->in_cf != nullptr : u->in != nullptr, SAT_E_INVALID, "oobleck_unit: input pointer missing");
    SAT_CHECK_ARG(to_cf ? u->out_cf != nullptr : (u->out_raw || u->out_snk), SAT_E_INVALID, "oobleck_unit: output pointer missing");
    SAT_CHECK_ARG(kind == SAT_OOBLECK_UNIT_CF_TO_CL || (u->weight_g && u->weight_v), SAT_E_INVALID, "oobleck_unit: weight_g / weight_v missing");
    const bool has_bias = kind != SAT_OOBLECK_UNIT_NEAREST && kind != SAT_OOBLECK_UNIT_FINAL_DEC && kind != SAT_OOBLECK_UNIT_CF_TO_CL;
    SAT_CHECK_ARG(!has_bias || u->bias, SAT_E_INVALID, "oobleck_unit: bias missing");
    const bool act_behind = u->out_snk != nullptr;      // the activation whose result out_snk holds
    const bool snake = u->activation == ACT_SNAKE;
    SAT_CHECK_ARG(!(act_behind && snake && kind != SAT_OOBLECK_UNIT_RESIDUAL) || (u->alpha && u->beta), SAT_E_INVALID, "oobleck_unit: alpha / beta missing");
    if (kind == SAT_OOBLECK_UNIT_RESIDUAL)
        SAT_CHECK_ARG(u->weight_g2 && u->weight_v2 && u->bias2 && (!snake || (u->alpha && u->beta && u->alpha2 && u->beta2)), SAT_E_INVALID,
                      "oobleck_unit: a ResidualUnit needs both convolutions and both activations");

    OobPlan p;
    p.cfg = sat_oobleck_cfg{};
    p.cfg.gemm_dtype = u->gemm_dtype;
    p.opt = sat_oobleck_options{u->activation, u->final_tanh, kind == SAT_OOBLECK_UNIT_NEAREST};
    auto set = [&](const char* name, const float* ptr, int64_t n) { return ptr ? p.tensors.set("oobleck", name, ptr, n) : 0; };
    const int ktaps = kind == SAT_OOBLECK_UNIT_CONV1_RES ? 1 : kind == SAT_OOBLECK_UNIT_FINAL_ENC ? 3 : resample ? 2 * st : 7;
    if (kind != SAT_OOBLECK_UNIT_CF_TO_CL) {
        const int gdim = kind == SAT_OOBLECK_UNIT_CONVT ? Ci : Co;      // weight norm runs over dim 0: ConvTranspose1d weights are [c_in, c_out, k]
        SAT_TRY(set("conv.weight_g", u->weight_g, gdim));
        SAT_TRY(set("conv.weight_v", u->weight_v, (int64_t)Ci * Co * ktaps));
        if (has_bias) SAT_TRY(set("conv.bias", u->bias, Co));
        SAT_TRY(set("act.alpha", u->alpha, Co));
        SAT_TRY(set("act.beta", u->beta, Co));
    }
    if (kind == SAT_OOBLECK_UNIT_RESIDUAL) {
        SAT_TRY(set("conv2.weight_g", u->weight_g2, Co));
        SAT_TRY(set("conv2.weight_v", u->weight_v2, (int64_t)Co * Co));
        SAT_TRY(set("conv2.bias", u->bias2, Co));
        SAT_TRY(set("act2.alpha", u->alpha2, Co));
        SAT_TRY(set("act2.beta", u->beta2, Co));
    }
    OobPlan::Block blk;
    ConvW cw;
    Snake sn, next;
    float* w_f32 = nullptr;
    op_t* Y = nullptr;
    SAT_TRY(plan_finalize(&p, s, [&](Bump& ar) -> int {
        p.zero_page = (op_t*)ar.take(256);
        if (!ar.dry()) SAT_HIP(hipMemsetAsync(p.zero_page, 0, 256, s));
        if (kind == SAT_OOBLECK_UNIT_CF_TO_CL) return 0;
        if (kind == SAT_OOBLECK_UNIT_RESIDUAL) {
            SAT_TRY(make_conv(&p, ar, "conv.", Ci, Co, 7, true, &blk.ru_c7[r], s));
            SAT_TRY(make_snake(&p, ar, "act.", Co, &blk.ru_sn2[r], s));
            SAT_TRY(make_conv(&p, ar, "conv2.", Co, Co, 1, true, &blk.ru_c1[r], s));
            SAT_TRY(make_snake(&p, ar, "act2.", Co, &next, s));
            Y = (op_t*)ar.take((size_t)B * L * pad64(Co) * sizeof(op_t));
            return 0;
        }
        if (act_behind) SAT_TRY(make_snake(&p, ar, "act.", Co, &sn, s));
        if (kind == SAT_OOBLECK_UNIT_CONVT) return make_convT(&p, ar, "conv.", Ci, Co, st, &cw, s);
        if (kind == SAT_OOBLECK_UNIT_NEAREST) return make_nearest(&p, ar, "conv.", Ci, Co, st, &cw, s);
        return make_conv(&p, ar, "conv.", Ci, Co, ktaps, has_bias, &cw, s, kind == SAT_OOBLECK_UNIT_FIRST_CONV ? &w_f32 : nullptr);
    }));

    const op_t* in = (const op_t*)u->in;
    op_t *res = (op_t*)const_cast<void*>(u->res), *out_raw = (op_t*)u->out_raw, *out_snk = (op_t*)u->out_snk;
    Ranger rg{&p, s};
    rg.unfused = u->two_launch != 0;
    ConvArgs a{};
    switch (kind) {
        case SAT_OOBLECK_UNIT_CF_TO_CL: SAT_TRY(launch_cf_to_cl(u->in_cf, out_raw ? out_raw : out_snk, Ci, L, B, s)); break;
        case SAT_OOBLECK_UNIT_FIRST_CONV: SAT_TRY(launch_first_conv(u->in_cf, w_f32, cw, sn, out_raw, out_snk, Ci, Co, L, B, s)); break;
        case SAT_OOBLECK_UNIT_RESIDUAL:
            SAT_TRY(run_ru(blk, r, pad64(Co), L, B, res, in, Y, out_snk, next, out_raw != nullptr, s, rg));
            break;
        case SAT_OOBLECK_UNIT_CONV7: a = ru_c7_args(cw, in, L, u->dilation); break;
        case SAT_OOBLECK_UNIT_CONV1_RES: a = ru_c1_args(cw, in, L, res, out_raw != nullptr); break;
        case SAT_OOBLECK_UNIT_CONVT: a = upsample_args(cw, in, L, st, false); break;
        case SAT_OOBLECK_UNIT_NEAREST: a = upsample_args(cw, in, L, st, true); break;
        case SAT_OOBLECK_UNIT_STRIDED: a = strided_args(cw, in, L, st); break;
        case SAT_OOBLECK_UNIT_FINAL_DEC: a = final_conv_args(cw, in, L, u->out_cf, Co, u->final_tanh != 0); break;
        default: a = final_conv_args(cw, in, L, u->out_cf, Co, 0); break;      // SAT_OOBLECK_UNIT_FINAL_ENC
    }
    if (a.W) {      // the kinds that are one launch of the convolution kernel
        if (!to_cf) {
            if (kind != SAT_OOBLECK_UNIT_CONV1_RES) a.out_raw = out_raw;
            if (out_snk) set_act(a, out_snk, sn);
        }
        SAT_TRY(launch_conv(a, B, s));
    }
    SAT_HIP(hipStreamSynchronize(s));      // the arena goes with p
    return 0;
}

}  // namespace SAT_OPNS

#if !defined(SAT_OPERAND_F16) && !defined(SAT_OPERAND_F32)
// ---- C ABI (bf16 build only): the plan's operand format (sat_oobleck_cfg.gemm_dtype, first member of every build's plan) picks the build
#define SAT_OOB_DECLARE(NS)                                                                                                       \
    namespace NS {                                                                                                                \
    struct OobPlan;                                                                                                               \
    int oob_plan_create(const sat_oobleck_cfg* cfg, const sat_oobleck_options* opt, OobPlan** out_plan);                          \
    void oob_plan_destroy(OobPlan* p);                                                                                            \
    int oob_plan_set_tensor(OobPlan* p, const char* name, const float* data_dev, int64_t numel);                                  \
    int oob_plan_finalize(OobPlan* p, sat_stream_t stream);                                                                       \
    int oob_workspace_bytes(const OobPlan* p, int32_t b, int32_t t_len, size_t* out_bytes);                                       \
    int oob_decode(OobPlan* p, const float* z, float* audio, int32_t B, int32_t T, void* ws, size_t ws_bytes, sat_stream_t stream); \
    int oob_encode(OobPlan* p, const float* audio, float* out, int32_t B, int32_t T, void* ws, size_t ws_bytes, sat_stream_t stream); \
    int oob_range_report(OobPlan* p, int32_t enable);                                                                             \
    int oob_range_report_count(OobPlan* p, int32_t* out_records);                                                                 \
    const char* oob_range_report_name(OobPlan* p, int32_t index);                                                                 \
    int oob_range_report_read(OobPlan* p, sat_range_record* out_host, int32_t capacity_records, size_t record_bytes, sat_stream_t stream); \
    int oob_unit(const sat_oobleck_unit_desc* u, sat_stream_t stream);                                                            \
    }
SAT_OOB_DECLARE(f16)
SAT_OOB_DECLARE(f32)
#undef SAT_OOB_DECLARE
static inline int32_t oob_dtype(const void* p) { return static_cast<const sat_oobleck_cfg*>(p)->gemm_dtype; }
// one call into the build that owns plan p (the same function name in namespaces bf16 / f16 / f32)
#define SAT_OOB_CALL(p, fn, ...)                                                                                                  \
    (oob_dtype(p) == SAT_GEMM_FP16    ? f16::fn(reinterpret_cast<f16::OobPlan*>(const_cast<sat_oobleck_plan*>(p)), __VA_ARGS__)   \
     : oob_dtype(p) == SAT_GEMM_FP32X ? f32::fn(reinterpret_cast<f32::OobPlan*>(const_cast<sat_oobleck_plan*>(p)), __VA_ARGS__)   \
                                      : bf16::fn(reinterpret_cast<bf16::OobPlan*>(const_cast<sat_oobleck_plan*>(p)), __VA_ARGS__))

extern "C" int sat_oobleck_plan_create_ex(const sat_oobleck_cfg* cfg, const sat_oobleck_options* options, size_t options_bytes,
                                          sat_oobleck_plan** out_plan) {
    SAT_CHECK_ARG(cfg && out_plan, SAT_E_INVALID, "oobleck_plan_create: null argument");
    sat_oobleck_options opt = {SAT_OOBLECK_ACT_SNAKE, 0, 0};      // options == NULL: the defaults of sat_oobleck_plan_create
    if (options) {
        SAT_CHECK_ARG(options_bytes == sizeof(sat_oobleck_options), SAT_E_INVALID,
                      "oobleck_plan_create_ex: options_bytes %zu is not the size of this version's sat_oobleck_options (%zu)", options_bytes,
                      sizeof(sat_oobleck_options));
        opt = *options;
    }
    SAT_CHECK_ARG(cfg->gemm_dtype == SAT_GEMM_BF16 || cfg->gemm_dtype == SAT_GEMM_FP16 || cfg->gemm_dtype == SAT_GEMM_FP32X,
                  SAT_E_UNSUPPORTED, "oobleck_plan_create: gemm_dtype must be 0 (bf16), 3 (fp16) or 2 (fp32)");
    SAT_CHECK_ARG(opt.activation == SAT_OOBLECK_ACT_SNAKE || opt.activation == SAT_OOBLECK_ACT_ELU, SAT_E_UNSUPPORTED,
                  "oobleck_plan_create_ex: activation %d is neither SAT_OOBLECK_ACT_SNAKE (0) nor SAT_OOBLECK_ACT_ELU (1)", opt.activation);
    SAT_CHECK_ARG((opt.final_tanh == 0 || opt.final_tanh == 1) && (opt.nearest_upsample == 0 || opt.nearest_upsample == 1), SAT_E_UNSUPPORTED,
                  "oobleck_plan_create_ex: final_tanh / nearest_upsample must be 0 or 1");
    SAT_CHECK_ARG(cfg->is_decoder || (!opt.final_tanh && !opt.nearest_upsample), SAT_E_UNSUPPORTED,
                  "oobleck_plan_create_ex: final_tanh / nearest_upsample are decoder options");
    switch (cfg->gemm_dtype) {
        case SAT_GEMM_FP16: return f16::oob_plan_create(cfg, &opt, reinterpret_cast<f16::OobPlan**>(out_plan));
        case SAT_GEMM_FP32X: return f32::oob_plan_create(cfg, &opt, reinterpret_cast<f32::OobPlan**>(out_plan));
        default: return bf16::oob_plan_create(cfg, &opt, reinterpret_cast<bf16::OobPlan**>(out_plan));
    }
}
// The original entry point and its contract: Snake, transposed convolutions, no tanh, channels and the decoder's latent_dim multiples of 64
extern "C" int sat_oobleck_plan_create(const sat_oobleck_cfg* cfg, sat_oobleck_plan** out_plan) {
    SAT_CHECK_ARG(cfg && out_plan, SAT_E_INVALID, "oobleck_plan_create: null argument");
    SAT_CHECK_ARG(cfg->gemm_dtype == SAT_GEMM_BF16 || cfg->gemm_dtype == SAT_GEMM_FP16 || cfg->gemm_dtype == SAT_GEMM_FP32X,
                  SAT_E_UNSUPPORTED, "oobleck_plan_create: gemm_dtype must be 0 (bf16), 3 (fp16) or 2 (fp32)");
    SAT_CHECK_ARG(cfg->channels % 64 == 0 && cfg->channels > 0, SAT_E_UNSUPPORTED,
                  "oobleck_plan_create: channels %d must be a multiple of 64 (sat_oobleck_plan_create_ex takes any)", cfg->channels);
    if (cfg->is_decoder)
        SAT_CHECK_ARG(cfg->latent_dim % 64 == 0, SAT_E_UNSUPPORTED,
                      "oobleck_plan_create: decoder latent_dim %d must be a multiple of 64 (sat_oobleck_plan_create_ex takes any)", cfg->latent_dim);
    return sat_oobleck_plan_create_ex(cfg, nullptr, 0, out_plan);
}
extern "C" void sat_oobleck_plan_destroy(sat_oobleck_plan* p) {
    if (!p) return;
    switch (oob_dtype(p)) {
        case SAT_GEMM_FP16: f16::oob_plan_destroy(reinterpret_cast<f16::OobPlan*>(p)); break;
        case SAT_GEMM_FP32X: f32::oob_plan_destroy(reinterpret_cast<f32::OobPlan*>(p)); break;
        default: bf16::oob_plan_destroy(reinterpret_cast<bf16::OobPlan*>(p));
    }
}
extern "C" int sat_oobleck_plan_set_tensor(sat_oobleck_plan* p, const char* name, const float* data_dev, int64_t numel) {
    SAT_CHECK_ARG(p, SAT_E_INVALID, "oobleck_plan_set_tensor: null plan");
    return SAT_OOB_CALL(p, oob_plan_set_tensor, name, data_dev, numel);
}
extern "C" int sat_oobleck_plan_finalize(sat_oobleck_plan* p, sat_stream_t stream) {
    SAT_CHECK_ARG(p, SAT_E_INVALID, "oobleck_plan_finalize: null plan");
    return SAT_OOB_CALL(p, oob_plan_finalize, stream);
}
extern "C" int sat_oobleck_workspace_bytes(const sat_oobleck_plan* p, int32_t b, int32_t t_len, size_t* out_bytes) {
    SAT_CHECK_ARG(p, SAT_E_INVALID, "oobleck_workspace_bytes: null plan");
    return SAT_OOB_CALL(p, oob_workspace_bytes, b, t_len, out_bytes);
}
extern "C" int sat_oobleck_decode(sat_oobleck_plan* p, const float* z_dev, float* audio_dev, int32_t b, int32_t t_len, void* ws, size_t ws_bytes,
                                  sat_stream_t stream) {
    SAT_CHECK_ARG(p, SAT_E_INVALID, "oobleck_decode: null plan");
    return SAT_OOB_CALL(p, oob_decode, z_dev, audio_dev, b, t_len, ws, ws_bytes, stream);
}
extern "C" int sat_oobleck_encode(sat_oobleck_plan* p, const float* audio_dev, float* out_dev, int32_t b, int32_t t_len, void* ws, size_t ws_bytes,
                                  sat_stream_t stream) {
    SAT_CHECK_ARG(p, SAT_E_INVALID, "oobleck_encode: null plan");
    return SAT_OOB_CALL(p, oob_encode, audio_dev, out_dev, b, t_len, ws, ws_bytes, stream);
}
extern "C" int sat_oobleck_range_report(sat_oobleck_plan* p, int32_t enable) {
    SAT_CHECK_ARG(p, SAT_E_INVALID, "oobleck_range_report: null plan");
    return SAT_OOB_CALL(p, oob_range_report, enable);
}
extern "C" int sat_oobleck_range_report_count(const sat_oobleck_plan* p, int32_t* out_records) {
    SAT_CHECK_ARG(p, SAT_E_INVALID, "oobleck_range_report_count: null plan");
    return SAT_OOB_CALL(p, oob_range_report_count, out_records);
}
extern "C" const char* sat_oobleck_range_report_name(const sat_oobleck_plan* p, int32_t index) {
    if (!p) return nullptr;
    return SAT_OOB_CALL(p, oob_range_report_name, index);
}
extern "C" int sat_oobleck_range_report_read(sat_oobleck_plan* p, sat_range_record* out_host, int32_t capacity_records, size_t record_bytes,
                                             sat_stream_t stream) {
    SAT_CHECK_ARG(p, SAT_E_INVALID, "oobleck_range_report_read: null plan");
    return SAT_OOB_CALL(p, oob_range_report_read, out_host, capacity_records, record_bytes, stream);
}
#undef SAT_OOB_CALL
// one layer alone (tests): the descriptor's gemm_dtype picks the build, as a plan's does
extern "C" int sat_oobleck_unit(const sat_oobleck_unit_desc* desc, size_t desc_bytes, sat_stream_t stream) {
    SAT_CHECK_ARG(desc, SAT_E_INVALID, "oobleck_unit: null descriptor");
    SAT_CHECK_ARG(desc_bytes == sizeof(sat_oobleck_unit_desc), SAT_E_INVALID,
                  "oobleck_unit: desc_bytes %zu is not the size of this version's sat_oobleck_unit_desc (%zu)", desc_bytes, sizeof(sat_oobleck_unit_desc));
    switch (desc->gemm_dtype) {
        case SAT_GEMM_BF16: return bf16::oob_unit(desc, stream);
        case SAT_GEMM_FP16: return f16::oob_unit(desc, stream);
        case SAT_GEMM_FP32X: return f32::oob_unit(desc, stream);
    }
    SAT_CHECK_ARG(false, SAT_E_UNSUPPORTED, "oobleck_unit: gemm_dtype must be 0 (bf16), 3 (fp16) or 2 (fp32)");
    return SAT_E_UNSUPPORTED;
}
#endif
