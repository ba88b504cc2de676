// The compile-time geometry of a ring GEMM tile (gemm_pipe_kernel, gemm_bf16.hip): every constant the kernel and its launcher
// (launch_pipe) need, derived once from the kernel's template arguments.  Plain C++17 without a HIP header, so
// tests/test_gemm_host.py prints it on the CPU for every built (tile, epilogue, flavour) and pins the dynamic LDS sizes.
#pragma once
#include "gemm_tiles.h"

// -DSAT_RING_MFMA_32X32: every ring tile on the 32 x 32 x 16 MFMA (A/B builds only; see RingGeom::S16)
#ifdef SAT_RING_MFMA_32X32
constexpr bool SAT_RING_MFMA_16 = false;
#else
constexpr bool SAT_RING_MFMA_16 = true;
#endif

// QKN: the alternative build of an epilogue.  EPI_HEADS_QKN: the heads kernel with the qk_norm epilogue; EPI_ACT16: the SwiGLU kernel
// with the plain-activation one (gemm_epilogue)
template <int EPIX>
struct EpiOf {
    static constexpr int EPI = EPIX == EPI_HEADS_QKN ? EPI_HEADS : EPIX == EPI_ACT16 ? EPI_SWIGLU : EPIX;
    static constexpr bool QKN = EPIX == EPI_HEADS_QKN || EPIX == EPI_ACT16;
};

template <int BM, int BN, int BK, int WM, int WN, int NS, int EPIX, int FP8 = 0, int KG = 1, bool DIL = false>
struct RingGeom {
    // the template arguments, for whoever is handed the geometry alone (tests/host/gemm_host_dump.cpp prints them)
    static constexpr int TILE_M = BM, TILE_N = BN, WAVES_M = WM, WAVES_N = WN, STAGES = NS, E4M3 = FP8, KGROUPS = KG;
    static constexpr int EPI = EpiOf<EPIX>::EPI;
    static constexpr bool QKN = EpiOf<EPIX>::QKN;
    static_assert(!QKN || FP8 == 0, "qk_norm / plain activation: 16-bit operands only");
    static_assert(BK == 64, "128-byte LDS rows (lds_tile_off)");
    static_assert(KG == 1 || (KG == 2 && EPI == EPI_F32 && FP8 == 0 && BM / WM == 64 && BN / WN == 64), "K-groups: fp32 output, 64 x 64 wave tiles");
    static constexpr int NT = KG * WM * WN * 64;
    static constexpr int TM = BM / WM;
    static constexpr int TN = BN / WN;
    // MFMA shape: the 8-wave fp32-output tiles with 16-bit operands (15, 44, 49) run v_mfma_f32_16x16x32 into 16 x 16 blocks (acc16),
    // every other build v_mfma_f32_32x32x16 (acc).  Same LDS image, fragment bytes, matrix-pipe cycles per k and bit-identical sums;
    // under the socket's power cap the smaller shape is the faster one on random data: FF-out 56.7 -> 50.4 us on tile 15, 53.3 -> 50.7
    // on tile 49, to_out 20.5 -> 19.8 (profiles/ring_mfma_shape_timing.txt).  Only the staged fp32 epilogue is shape-agnostic behind
    // its first line (stage_rows32).  The 4-wave tile 16 measured 1.5-2 % slower at its own shape (cross to_out, 14.55 -> 14.8 us) in
    // three interleaves of its reads and DMA pieces and keeps the old shape; the 16-wave tile has no room for two sets of the twice as
    // many fragments.
    // The 12-wave heads build of tile 30 (one-prompt to_qkv) runs it too, in both orientations (q / k swapped, V^T un-swapped: gemm_heads16_t,
    // gemm_heads16_vt); its qk_norm, SwiGLU, plain-activation, fp32 and e4m3 builds keep 32 x 32 x 16.  The product call (M = 2050,
    // d = 1536, LayerNorm fold) went 40.0 -> 36.3 us in fp16 and 38.1 -> 35.2 in bf16, 27 and 10 times the spread of one build, with
    // q, k and V^T bit-identical (profiles/qkv_mfma_shape_timing.txt); 164 VGPRs of the 168 that three waves per SIMD leave, no scratch.
    static constexpr bool S16 = SAT_RING_MFMA_16 && FP8 == 0 && ((EPI == EPI_F32 && NT == 512) || (EPI == EPI_HEADS && !QKN && NT == 768));
    // the fused epilogues need a whole head / a value-gate pair per wave, the staged fp32 epilogue a 64-column block
    static_assert(TN == 64, "wave tile is TM x 64");
    static constexpr int MI = TM / 32;
    static constexpr int NI = TN / 32;
    // 16 x 16 x 32 builds (S16): MB 16-row blocks x four 16-column blocks instead
    static constexpr int MB = S16 ? TM / 16 : 1;
    static constexpr int CPR = BK / 8;                    // 16-B chunks per row
    // One LDS-DMA instruction of one wave moves 64 chunks = 1 KiB.  A stage holds WL_A + WL_B of them (A rows first, then
    // W rows, contiguous); wave w issues wave-loads w, w+NW, w+2NW, ...  When NW does not divide WL (256x192 on 12 waves:
    // 56 wave-loads) the first WL%NW waves carry one more than the rest, and the counted vmcnt wait is per wave.
    static constexpr int NW = KG * WM * WN;                  // every wave loads
    static constexpr int WL_A = BM * CPR / 64;
    static constexpr int WLG = (BM + BN) * CPR / 64;         // wave-loads of one K-group's rows of a stage
    static constexpr int WL = KG * WLG;
    static constexpr int LPT = (WL + NW - 1) / NW;        // max LDS-DMA instructions per tile per wave
    static constexpr int N_FULL = WL - (LPT - 1) * NW;    // waves [0, N_FULL) issue LPT, the others LPT-1
    static constexpr bool UNIFORM = (WL % NW) == 0;
    static constexpr int ROWB = BK * 2;
    static constexpr bool MXA = FP8 == 3;                 // MXFP8 A operand: + one dword of E8M0 block scales per A row per stage
    static constexpr int SCALE_WAVES = MXA ? BM / 64 : 0; // the first BM/64 waves each DMA 64 scale dwords per stage
    static constexpr int GROUP_BYTES = (BM + BN) * ROWB + (MXA ? BM * 4 : 0);
    static constexpr int STAGE_BYTES = KG * GROUP_BYTES;
    static constexpr int D = NS - 1;                      // prefetch distance
    // DIL ("DMA in loop", 16-bit operands): the iteration's LDS-DMA pieces are issued inside the fragment loop, behind the MFMAs of the first
    // k-steps, instead of in front of it -- always on with K-groups; a per-tile choice otherwise (SatTile::dil, gemm_tiles.h)
    static constexpr bool DIL_ON = (DIL || KG == 2) && FP8 == 0;
    static constexpr int NDIL = !DIL_ON ? 0 : UNIFORM ? LPT : LPT - 1;          // pieces EVERY wave issues in the loop body (a ragged tile's extra piece stays in front)
    // k-steps that carry them (K-groups: the half in front of the mid-iteration barrier, which is one 32-k step of the 16 x 16 x 32 loop)
    static constexpr int DIL_STEPS = KG == 2 ? (S16 ? 1 : BK / 32) : BK / 16 - 1;
    static_assert(!S16 || KG == 2 || !DIL_ON, "16 x 16 x 32, one K-group: the LDS-DMA pieces are issued in front of the fragment loop");
    static constexpr int DIL_PER = (NDIL + DIL_STEPS - 1) / (DIL_STEPS > 0 ? DIL_STEPS : 1);
    static_assert(!MXA || D == 1 || UNIFORM, "MXFP8: counted waits are built for uniform tiles or 2-stage rings");
    static_assert((BM * CPR) % 64 == 0 && (BN * CPR) % 64 == 0 && (D - 1) * LPT < 64, "bad pipeline geometry");

    // LayerNorm fold, consumer side: (mean, 1/std) of the BM rows, then the BN (c1, c2) pairs of this tile's output channels, in LDS
    // behind the ring at LN_OFF
    static constexpr bool LN_CONS = (EPI == EPI_SWIGLU || EPI == EPI_HEADS) && FP8 == 0;
    static constexpr int LN_OFF = NS * STAGE_BYTES;
    // fp32 residual epilogue of the small tiles (one 32-row block per wave, registers to spare): the residual values are fetched at kernel start
    static constexpr bool PRE_RESID = EPI == EPI_F32 && (MI == 1 || KG == 2) && NI == 2 && NT <= 512;
    // Orientation of the accumulators, fixed at compile time wherever it can be (0: un-swapped only -- fp32 output, MXFP8 A operand;
    // 1: transposed only -- SwiGLU; 2: per wave -- heads: q / k transposed, V^T un-swapped)
    static constexpr int ORI = (MXA || EPI == EPI_F32) ? 0 : (EPI == EPI_SWIGLU ? 1 : 2);
    // Fused cross-attention (HeadsEpi::xa_k): one head per workgroup column, one 32-query block per wave; three K / V^T tiles of 64 keys
    // at XA_OFF, behind the ring and the LayerNorm constants.  With the asserts above this is the 128 x 64 geometry of 4 x 1 waves
    // (tiles 16 and 256) and nothing else.
    static constexpr bool XA_OK = EPI == EPI_HEADS && MI == 1 && NI == 2 && NW == 4 && BN == 64 && NS == 3 && FP8 == 0;
    static_assert(!XA_OK || (BM == 128 && WM == 4 && WN == 1 && KG == 1), "fused cross-attention: the 128 x 64 tile");
    static constexpr int XA_OFF = (LN_OFF + (BM + BN) * 8 + 1023) & ~1023;

    // dynamic LDS of a launch: the ring, + (mean, rstd) per row and (c1, c2) per column; with the fused cross-attention epilogue
    static constexpr int LDS = LN_OFF + (LN_CONS ? (BM + BN) * 8 : 0);
    static constexpr int XA_LDS = XA_OK ? XA_OFF + 3 * 16384 : LDS;
    static_assert(LDS <= 160 * 1024, "LDS ring exceeds 160 KiB");
    static_assert(XA_LDS <= 160 * 1024, "fused cross-attention: K / V^T tiles do not fit behind the ring");
    static_assert(EPI != EPI_F32 || LDS >= WM * WN * 8192, "the staged fp32 epilogue needs 8 KiB of LDS per wave");
    // K-groups: 8 KiB per wave of exchange area in the first half of the (free) ring, the staged epilogue's areas in the second half
    static constexpr int KG_STAGING_OFF = NW * 8192;
    static_assert(KG == 1 || LN_OFF >= 2 * NW * 8192, "exchange + staging areas");
};
