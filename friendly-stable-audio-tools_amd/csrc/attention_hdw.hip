// Flash-style attention core for DiTs with 32-, 96- and 128-channel heads (the staged route of dit_plan.hip): softmax(q k^T / sqrt(W)) v,
// non-causal, no mask, GQA by head index (models/transformer.py:303-308, 496-536 of the reference).  One kernel template over the head
// width W, the structure attention.hip documents, at another width:
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
//  * softmax recurrence: MODE 1 of attn_core.h restated for W / 32 output blocks (standing reference, the row sum is the overflow check).
//    The reference starts at -1e30, so the first block of a sequence always overflows its check and SETS the reference to the true row
//    maximum: rows whose log2-domain scores all lie below -126 are safe (test_attention_hd128_all_scores_strongly_negative).
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
#include "attn_core.h"
#include "attn_hdw_tiles.h"
#include "sat_common.h"

namespace {

using attn::half_sum;
using attn::half_max;

constexpr int Q_BLOCK = 256;          // queries per workgroup

template <int W>
__global__ __launch_bounds__(512) void attention_hdw_kernel(const op_t* __restrict__ q, const op_t* __restrict__ k, const op_t* __restrict__ vt,
                                                            op_t* __restrict__ out, int H, int KVH, int Sq, int Sk, int Sq_pad, int Sk_pad) {
    using T = attnw::Tiles<W>;
    constexpr int KT = T::KV_TILE, KSTEPS = W / 16, DB = W / 32, KB = KT / 32;
    constexpr int K_LPR = T::K_ROW_BYTES / 16, V_LPR = T::VT_ROW_BYTES / 16;      // DMA lanes per LDS row
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
    const int n_tiles = (k_end + KT - 1) / KT;       // n_tiles * KT <= Sk_pad: the launcher checks Sk_pad >= Sk + 3, Sk_pad % KT == 0

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
    constexpr int PIECES = T::K_PIECES + T::VT_PIECES;      // per wave and tile

    f32x16 oacc[DB];        // O^T: channels d = db*32 + 8*(r>>2) + 4*half + (r&3) of the lane's query
#pragma unroll
    for (int i = 0; i < DB; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[i][r] = 0.f;
    float m_run = -1e30f;   // reference, log2 units (Q is pre-scaled)
    float l_run = 0.f;      // this lane's partial row sum (its 16 of every 32 keys)

    // a wave whose 32 queries are all beyond Sq still copies tiles and joins the barriers, but skips the matrix and softmax work
    const bool wave_active = __builtin_amdgcn_readfirstlane(bx * Q_BLOCK + wave * 32) < Sq;

    auto process = [&](int tile, int stage) {
        const char* sk = smem + stage * T::STAGE_BYTES;
        const char* sv = sk + T::K_TILE_BYTES;
        const bool edge = (tile == 0 && ob != 0) || (tile == n_tiles - 1 && (k_end & (KT - 1)) != 0);
#pragma unroll
        for (int kb = 0; kb < KB; ++kb) {
            if (KB > 2 && tile * KT + kb * 32 >= k_end) break;      // the rest of the last tile is pad (wave-uniform); block 0 of a tile never is
            // ---- S^T = K Q^T for 32 keys
            f32x16 sacc;
#pragma unroll
            for (int r = 0; r < 16; ++r) sacc[r] = 0.f;
#pragma unroll
            for (int t = 0; t < KSTEPS; ++t) {
                const opx8 kf = *reinterpret_cast<const opx8*>(sk + T::k_tile_off(kb * 32 + l31, t * 2 + half));
                sacc = mfma_32x32x16(kf, qf[t], sacc);
            }
            // V^T fragments do not depend on the softmax: request them now, their LDS latency hides behind the VALU work
            opx8 vf[DB][2];
#pragma unroll
            for (int db = 0; db < DB; ++db)
#pragma unroll
                for (int u = 0; u < 2; ++u) vf[db][u] = *reinterpret_cast<const opx8*>(sv + T::vt_tile_off(db * 32 + l31, (kb * 2 + u) * 2 + half));
            // ---- mask the keys outside [ob, k_end) (wave-uniform branch: first and last tile only)
            if (edge) {
                const int key0 = tile * KT + kb * 32 + 4 * half;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int key = key0 + (r & 3) + 8 * (r >> 2);
                    if (key < ob || key >= k_end) sacc[r] = -INFINITY;
                }
            }
            // ---- online softmax step against the standing reference
            opx8 pb[2];
            float psum = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float p = __builtin_amdgcn_exp2f(sacc[r] - m_run);
                psum += p;
                pb[r >> 3][r & 7] = f32_to_op(p);
            }
            if (!__all(psum <= 4096.0f)) {      // wave-uniform; always in the sequence's first block (reference -1e30), later for a score > 12 octaves above it
                float mloc = sacc[0];
#pragma unroll
                for (int r = 1; r < 16; ++r) mloc = fmaxf(mloc, sacc[r]);
                const float m_new = fmaxf(m_run, half_max(mloc));
                const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
                m_run = m_new;
                l_run *= alpha;
#pragma unroll
                for (int i = 0; i < DB; ++i)
#pragma unroll
                    for (int r = 0; r < 16; ++r) oacc[i][r] *= alpha;
                psum = 0.f;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float p = __builtin_amdgcn_exp2f(sacc[r] - m_run);
                    psum += p;
                    pb[r >> 3][r & 7] = f32_to_op(p);
                }
            }
            l_run += psum;
            // ---- O^T += V^T P^T
#pragma unroll
            for (int db = 0; db < DB; ++db)
#pragma unroll
                for (int u = 0; u < 2; ++u) oacc[db] = mfma_32x32x16(vf[db][u], pb[u], oacc[db]);
        }
    };

    // tile it + 1 stays in flight across the barrier (counted vmcnt: this wave issued PIECES pieces for it); tile it + 2 goes into the stage
    // tile it - 1 occupied, which every wave left before this barrier
    stage_in(0, 0);
    if (n_tiles > 1) stage_in(1, 1);
    int st = 0;
    for (int it = 0; it < n_tiles; ++it) {
        if (it + 1 < n_tiles) wait_vmcnt<PIECES>();
        else wait_vmcnt<0>();
        __builtin_amdgcn_s_barrier();
        const int st2 = st >= 1 ? st - 1 : 2;                 // (it + 2) % 3
        if (it + 2 < n_tiles) stage_in(it + 2, st2);
        if (wave_active) process(it, st);
        st = st == 2 ? 0 : st + 1;
    }

    const float inv = 1.0f / half_sum(l_run);
    op_t* op = out + ((size_t)b * Sq + qi) * ((size_t)H * W) + h * W + 8 * half;
#pragma unroll
    for (int db = 0; db < DB; ++db) {
        unsigned pk[8];
#pragma unroll
        for (int rq = 0; rq < 4; ++rq) {
            pk[2 * rq] = pack_op2(oacc[db][rq * 4] * inv, oacc[db][rq * 4 + 1] * inv);
            pk[2 * rq + 1] = pack_op2(oacc[db][rq * 4 + 2] * inv, oacc[db][rq * 4 + 3] * inv);
        }
        half_swap(pk[0], pk[2]);            // 8 consecutive channels per lane: one 16-byte store instead of two 8-byte ones
        half_swap(pk[1], pk[3]);
        half_swap(pk[4], pk[6]);
        half_swap(pk[5], pk[7]);
        if (qi < Sq) {
            *reinterpret_cast<u32x4*>(op + db * 32) = u32x4{pk[0], pk[1], pk[2], pk[3]};
            *reinterpret_cast<u32x4*>(op + db * 32 + 16) = u32x4{pk[4], pk[5], pk[6], pk[7]};
        }
    }
}

template <int W>
int launch(const op_t* q, const op_t* k, const op_t* vt, op_t* out, int b, int h, int kvh, int sq, int sk, int sq_pad, int sk_pad, hipStream_t s) {
    using T = attnw::Tiles<W>;
    SAT_CHECK_ARG(sq_pad % 128 == 0 && sk_pad % T::KV_TILE == 0, SAT_E_INVALID,
                  "attention_hdw: with %d-channel heads sq_pad %% 128 and sk_pad %% %d must be 0 (got %d, %d)", W, T::KV_TILE, sq_pad, sk_pad);
    SAT_TRY(sat_ensure_dynamic_lds(reinterpret_cast<const void*>(attention_hdw_kernel<W>), T::LDS_BYTES));
    hipLaunchKernelGGL(attention_hdw_kernel<W>, dim3(cdiv(sq, Q_BLOCK), h, b), dim3(512), T::LDS_BYTES, s, q, k, vt, out, h, kvh, sq, sk, sq_pad, sk_pad);
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
    SAT_CHECK_ARG(q && k && vt && out, SAT_E_INVALID, "attention_hdw: null pointer");
    SAT_CHECK_ARG(b > 0 && h > 0 && kvh > 0 && h % kvh == 0, SAT_E_INVALID, "attention_hdw: bad heads %d/%d", h, kvh);
    SAT_CHECK_ARG(h <= 65535 && b <= 65535, SAT_E_UNSUPPORTED, "attention_hdw: %d heads / %d sequences exceed the grid", h, b);
    SAT_CHECK_ARG(sq > 0 && sk > 0 && sq_pad >= sq && sk_pad >= sk, SAT_E_INVALID, "attention_hdw: bad lengths");
    SAT_CHECK_ARG(sk_pad >= sk + 3, SAT_E_INVALID, "attention_hdw: sk_pad must be >= sk + 3 (key-side shift), got %d for sk=%d", sk_pad, sk);
    SAT_CHECK_ARG((((uintptr_t)q | (uintptr_t)k | (uintptr_t)vt | (uintptr_t)out) & 15) == 0, SAT_E_INVALID,
                  "attention_hdw: pointers must be 16-byte aligned");
    if (head_dim == 32) return launch<32>(q, k, vt, out, b, h, kvh, sq, sk, sq_pad, sk_pad, s);
    if (head_dim == 96) return launch<96>(q, k, vt, out, b, h, kvh, sq, sk, sq_pad, sk_pad, s);
    return launch<128>(q, k, vt, out, b, h, kvh, sq, sk, sq_pad, sk_pad, s);
}
