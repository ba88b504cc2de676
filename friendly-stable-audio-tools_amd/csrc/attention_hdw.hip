// Flash-style attention core for DiTs with 32-, 96- and 128-channel heads (the staged route of dit_plan.hip): softmax(q k^T / sqrt(W)) v,
// no mask, GQA by head index (models/transformer.py:303-308, 496-536 of the reference); non-causal (attention_hdw_kernel<W, false>) or, for
// the self-attention of a causal model, with query i seeing the keys j <= i of its sequence (attention_hdw_kernel<W, true>,
// sat_launch_attention_hdw_causal).  One kernel template over the head width W and the mask, built from the pieces of attn_core.h (the
// per-wave step attn::tile over LayoutHdw<W>, the ring walk attn::walk3, the output store attn::store_out): the structure attention.hip
// documents, at another width:
//
//  * both products transposed on v_mfma_f32_32x32x16_{bf16,f16}: S^T[key, q] = K[key, :] . Q[q, :] with Q in registers as the B operand
//    (W / 16 = 2, 6 or 8 K-steps), O^T[d, q] = V^T[d, key] . P^T[key, q] with the lane's own 16 probabilities as B; O^T is W / 32 = 1, 3 or
//    4 accumulator blocks of 32 channels.  A wave owns 32 queries (lane l and l ^ 32 share query l & 31), P is rounded once and never leaves
//    the lane, the online softmax advances in steps of 32 keys; V^T stores the key index permuted by vt_pos (sat_common.h).
//  * one workgroup = 8 waves = 256 queries of one (batch, head); every wave walks ALL the key tiles of one shared ring (the single-KV-group
//    layout of attention.hip; there is no two-group layout here) of three stages, prefetch distance 2, one raw
//    s_barrier per tile, counted vmcnt waits (never __syncthreads() with an LDS-DMA in flight).
//  * K / V^T tiles by LDS-DMA (global_load_lds, 16 bytes per lane, 1 KiB per wave and instruction) with the XOR swizzles of
//    attn_hdw_tiles.h folded into the per-lane SOURCE address.
//  * softmax recurrence: MODE 1 of attn_core.h over W / 32 output blocks, without the scale (Q arrives pre-scaled).  The first block of a
//    sequence always fails the overflow check and SETS the reference to the true row maximum, so rows whose log2-domain scores all lie
//    below -126 are safe (test_attention_hd128_all_scores_strongly_negative).
//  * CAUSAL: the ranges of attn_causal.h exactly as in attention.hip -- the workgroup walks the tiles up to the diagonal of its last query, a
//    wave skips the 32-key blocks above its own last query, masks per element where the diagonal crosses a block and runs the blocks below
//    it unmasked.
//  * data conventions: Q [B, H, Sq_pad, W] pre-scaled by log2(e) / sqrt(W) (head_split_hdw.hip, HeadsEpi kind bit 3), K [B, KVH, Sk_pad, W]
//    with sequence b starting at row (b * Sk) & 3, V^T [B, KVH, W, Sk_pad] with the vt_pos key permutation, output [B * Sq, H * W] in the
//    operand type as 16-byte stores (no MXFP8 output form), front and tail pad keys masked to -inf in the first and last tile only.
//
// What differs per width (attn_hdw_tiles.h has the maps):
//  * W = 128.  K tile 64 keys x 256 B (a row is exactly one bank row), V^T tile 128 channel rows x 128 B, 2 + 2 pieces per wave and tile,
//    no holes and no spare rows.  Ring of THREE 32-KiB stages (96 KiB).  Why three: a 64-register O^T accumulator puts the kernel above 128
//    VGPRs, so 8 waves of 512 threads fill the SIMDs' register files and ONE workgroup is resident per CU whatever the LDS use -- there is
//    no second workgroup whose MFMAs would cover this one's wait for a tile, the distance-2 prefetch has to, and 96 of the CU's 160 KiB are
//    free for it.
//  * W = 32.  A K row is 64 B: four rows share a 256-byte bank row and the XOR key is (row >> 2) & 3.  The key tile is 128 keys (K tile
//    128 x 64 B, V^T tile 32 x 256 B, 16 KiB per stage, 48 KiB per workgroup): a 64-key tile is two 32-key blocks of 2 + 2 MFMAs between
//    barriers, 128 keys halve the barriers per key and keep every wave at one 1-KiB piece per operand and tile.  32-key blocks of the last
//    tile that lie wholly behind the sequence are skipped (wave-uniform).  The kernel needs 16 accumulator registers and stays under 128
//    VGPRs (the compiler reports 90 in both builds, tests/test_dit_head_width_host.py gates 128), so two workgroups of 512 threads are
//    resident per CU and one covers the other's wait at the barrier.  Measured (profiles/dit_head_width_timing.txt, two sequences of
//    S = 1025, D 1536, fp16): 33.3 us at 48 heads of 32 against 24.9 us for the 64-channel kernel at 24 heads; a 64-key tile was not measured.
//  * W = 96.  A K row is 192 B in HBM, no power of two: the LDS row is padded to 256 B, where chunk ^ (row & 15) is a bijection onto the
//    16 slots; the four slots per row that no chunk maps to are filled by their DMA lanes with chunk 0 of the same row (in bounds, never
//    read).  64-key tile, V^T tile 96 rows x 128 B plus 32 spare rows that the second V^T piece of waves 4-7 fills from channel rows
//    64-95 again (never read): every wave issues 2 + 2 pieces per tile and one vmcnt count serves all.  32 KiB per stage, 96 KiB, one
//    workgroup per CU (48 accumulator + 24 Q registers put it above 128 VGPRs), exactly the ring of W = 128.
#include "attn_causal.h"
#include "attn_core.h"
#include "attn_hdw_tiles.h"
#include "sat_common.h"

namespace {

constexpr int Q_BLOCK = 256;          // queries per workgroup

template <int W, bool CAUSAL>
__global__ __launch_bounds__(512) void attention_hdw_kernel(const op_t* __restrict__ q, const op_t* __restrict__ k, const op_t* __restrict__ vt,
                                                            op_t* __restrict__ out, int H, int KVH, int Sq, int Sk, int Sq_pad, int Sk_pad) {
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

    // Q fragments (B operand of S^T): Q[qi][16t + 8*half .. +8]
    opx8 qf[KSTEPS];
    {
        const op_t* qp = q + ((size_t)(b * H + h) * Sq_pad + (qi < Sq_pad ? qi : Sq_pad - 1)) * W + half * 8;
#pragma unroll
        for (int t = 0; t < KSTEPS; ++t) qf[t] = *reinterpret_cast<const opx8*>(qp + t * 16);
    }

    // K rows / V^T columns of sequence b start at ob = (b*Sk) & 3 (head_split_hdw.hip, kind bit 2)
    const int ob = (b * Sk) & 3;
    const int k_end = ob + Sk;
    // n_tiles * KT <= Sk_pad: the launcher checks Sk_pad >= Sk + 3, Sk_pad % KT == 0 (CAUSAL: no more tiles than that)
    const int n_tiles = CAUSAL ? attnc::tiles_walked(bx * Q_BLOCK, Q_BLOCK, ob, Sk, KT) : (k_end + KT - 1) / KT;
    [[maybe_unused]] const int cq_first = CAUSAL ? __builtin_amdgcn_readfirstlane(bx * Q_BLOCK + wave * 32) : 0;      // CAUSAL: the wave's first query ...
    [[maybe_unused]] const int c_end = CAUSAL ? attnc::key_end(qi, ob, Sk) : 0;                                      // ... and one past the lane's last visible key

    // LDS-DMA pieces of this wave: pieces `wave + 8 i` of the K tile and of the V^T tile.  Lane l of a piece lands at byte 16 l of its KiB,
    // i.e. at row (piece KiB + 16 l) / ROW_BYTES, slot l % (ROW_BYTES / 16), and fetches the logical chunk slot ^ key(row) from HBM
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

    // a wave whose 32 queries are all beyond Sq still copies tiles and joins the barriers, but skips the matrix and softmax work
    const bool wave_active = __builtin_amdgcn_readfirstlane(bx * Q_BLOCK + wave * 32) < Sq;

    attn::walk3<T::K_PIECES + T::VT_PIECES>(0, n_tiles, stage_in, [&](int tile, int stage) {
        if (!wave_active) return;
        const char* sk = smem + stage * T::STAGE_BYTES;
        const bool edge = (tile == 0 && ob != 0) || (tile == n_tiles - 1 && (k_end & (KT - 1)) != 0);
        // front and tail pad keys are masked in the first and last tile only; CAUSAL: per block, against the lane's own last visible key
        attn::tile<1, 0, CAUSAL ? attn::MASK_CAUSAL : attn::MASK_NONE, attn::LayoutHdw<W>>(st, qf, sk, sk + T::K_TILE_BYTES, edge, tile * KT, ob,
                                                                                           CAUSAL ? c_end : k_end, false, 1.0f, l31, half, cq_first, Sk);
    });

    op_t* op = out + ((size_t)b * Sq + qi) * ((size_t)H * W) + h * W + 8 * half;
    attn::store_out(st.oacc, 1.0f / attn::half_sum(st.l_run), op, qi < Sq);
}

template <int W, bool CAUSAL = false>
int launch(const op_t* q, const op_t* k, const op_t* vt, op_t* out, int b, int h, int kvh, int sq, int sk, int sq_pad, int sk_pad, hipStream_t s) {
    using T = attnw::Tiles<W>;
    SAT_CHECK_ARG(sq_pad % 128 == 0 && sk_pad % T::KV_TILE == 0, SAT_E_INVALID,
                  "attention_hdw: with %d-channel heads sq_pad %% 128 and sk_pad %% %d must be 0 (got %d, %d)", W, T::KV_TILE, sq_pad, sk_pad);
    const auto kernel = attention_hdw_kernel<W, CAUSAL>;
    SAT_TRY(sat_ensure_dynamic_lds(reinterpret_cast<const void*>(kernel), T::LDS_BYTES));
    hipLaunchKernelGGL(kernel, dim3(cdiv(sq, Q_BLOCK), h, b), dim3(512), T::LDS_BYTES, s, q, k, vt, out, h, kvh, sq, sk, sq_pad, sk_pad);
    SAT_LAUNCH_CHECK();
    return 0;
}

}  // namespace

#ifdef SAT_OPERAND_F16
int sat_launch_attention_hdw_f16(const void* q, const void* k, const void* vt, void* out, int b, int h, int kvh, int head_dim, int sq, int sk,
                                 int sq_pad, int sk_pad, hipStream_t s) {
    return f16::sat_launch_attention_hdw((const op_t*)q, (const op_t*)k, (const op_t*)vt, (op_t*)out, b, h, kvh, head_dim, sq, sk, sq_pad, sk_pad, s, 1);
}
#endif

int SAT_OPNS::sat_launch_attention_hdw(const op_t* q, const op_t* k, const op_t* vt, op_t* out, int b, int h, int kvh, int head_dim, int sq, int sk,
                                       int sq_pad, int sk_pad, hipStream_t s, int f16) {
#ifndef SAT_OPERAND_F16
    if (f16) return sat_launch_attention_hdw_f16(q, k, vt, out, b, h, kvh, head_dim, sq, sk, sq_pad, sk_pad, s);
#else
    SAT_CHECK_ARG(f16, SAT_E_INVALID, "attention_hdw: the fp16 build takes fp16 tensors and writes fp16");
#endif
    SAT_CHECK_ARG(head_dim == 32 || head_dim == 96 || head_dim == 128, SAT_E_UNSUPPORTED,
                  "attention_hdw: dim_heads %d (this kernel is built for 32, 96 and 128)", head_dim);
    SAT_CHECK_ATTENTION("attention_hdw", "sk", sq, sk, true, false);
    if (head_dim == 32) return launch<32>(q, k, vt, out, b, h, kvh, sq, sk, sq_pad, sk_pad, s);
    if (head_dim == 96) return launch<96>(q, k, vt, out, b, h, kvh, sq, sk, sq_pad, sk_pad, s);
    return launch<128>(q, k, vt, out, b, h, kvh, sq, sk, sq_pad, sk_pad, s);
}

// Causal self-attention (sq == sk == s_len): the checks of sat_launch_attention_hdw, the CAUSAL instantiations
#ifdef SAT_OPERAND_F16
int sat_launch_attention_hdw_causal_f16(const void* q, const void* k, const void* vt, void* out, int b, int h, int kvh, int head_dim, int s_len,
                                        int sq_pad, int sk_pad, hipStream_t s) {
    return f16::sat_launch_attention_hdw_causal((const op_t*)q, (const op_t*)k, (const op_t*)vt, (op_t*)out, b, h, kvh, head_dim, s_len, sq_pad, sk_pad, s, 1);
}
#endif

int SAT_OPNS::sat_launch_attention_hdw_causal(const op_t* q, const op_t* k, const op_t* vt, op_t* out, int b, int h, int kvh, int head_dim, int s_len,
                                              int sq_pad, int sk_pad, hipStream_t s, int f16) {
#ifndef SAT_OPERAND_F16
    if (f16) return sat_launch_attention_hdw_causal_f16(q, k, vt, out, b, h, kvh, head_dim, s_len, sq_pad, sk_pad, s);
#else
    SAT_CHECK_ARG(f16, SAT_E_INVALID, "attention_hdw (causal): the fp16 build takes fp16 tensors and writes fp16");
#endif
    SAT_CHECK_ARG(head_dim == 32 || head_dim == 96 || head_dim == 128, SAT_E_UNSUPPORTED,
                  "attention_hdw (causal): dim_heads %d (this kernel is built for 32, 96 and 128)", head_dim);
    SAT_CHECK_ATTENTION("attention_hdw (causal)", "s", s_len, s_len, true, false);
    if (head_dim == 32) return launch<32, true>(q, k, vt, out, b, h, kvh, s_len, s_len, sq_pad, sk_pad, s);
    if (head_dim == 96) return launch<96, true>(q, k, vt, out, b, h, kvh, s_len, s_len, sq_pad, sk_pad, s);
    return launch<128, true>(q, k, vt, out, b, h, kvh, s_len, s_len, sq_pad, sk_pad, s);
}
