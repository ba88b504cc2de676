// Flash-style attention core for DiTs with 32-, 96- and 128-channel heads (the staged route of dit_plan.hip): softmax(q k^T / sqrt(W)) v,
// no mask, GQA by head index (models/transformer.py:303-308, 496-536 of the reference); non-causal (attention_hdw_kernel<W>) or, for the
// self-attention of a causal model, with query i seeing the keys j <= i of its sequence (attention_hdw_causal_kernel<W>,
// sat_launch_attention_hdw_causal).  Both are the one kernel text of attention_hdw_kernel.inc over the head width W, the structure
// attention.hip documents, at another width:
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
#include "attn_causal.h"
#include "attn_core.h"
#include "attn_hdw_tiles.h"
#include "sat_common.h"

namespace {

using attn::half_sum;
using attn::half_max;

constexpr int Q_BLOCK = 256;          // queries per workgroup

#define ATTN_HDW_KERNEL attention_hdw_kernel
#define ATTN_HDW_CAUSAL false
#include "attention_hdw_kernel.inc"
#undef ATTN_HDW_KERNEL
#undef ATTN_HDW_CAUSAL
#define ATTN_HDW_KERNEL attention_hdw_causal_kernel
#define ATTN_HDW_CAUSAL true
#include "attention_hdw_kernel.inc"
#undef ATTN_HDW_KERNEL
#undef ATTN_HDW_CAUSAL

template <int W, bool CAUSAL = false>
int launch(const op_t* q, const op_t* k, const op_t* vt, op_t* out, int b, int h, int kvh, int sq, int sk, int sq_pad, int sk_pad, hipStream_t s) {
    using T = attnw::Tiles<W>;
    SAT_CHECK_ARG(sq_pad % 128 == 0 && sk_pad % T::KV_TILE == 0, SAT_E_INVALID,
                  "attention_hdw: with %d-channel heads sq_pad %% 128 and sk_pad %% %d must be 0 (got %d, %d)", W, T::KV_TILE, sq_pad, sk_pad);
    const auto kernel = CAUSAL ? attention_hdw_causal_kernel<W> : attention_hdw_kernel<W>;
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
    SAT_CHECK_ARG(q && k && vt && out, SAT_E_INVALID, "attention_hdw (causal): null pointer");
    SAT_CHECK_ARG(b > 0 && h > 0 && kvh > 0 && h % kvh == 0, SAT_E_INVALID, "attention_hdw (causal): bad heads %d/%d", h, kvh);
    SAT_CHECK_ARG(h <= 65535 && b <= 65535, SAT_E_UNSUPPORTED, "attention_hdw (causal): %d heads / %d sequences exceed the grid", h, b);
    SAT_CHECK_ARG(s_len > 0 && sq_pad >= s_len && sk_pad >= s_len, SAT_E_INVALID, "attention_hdw (causal): bad lengths");
    SAT_CHECK_ARG(sk_pad >= s_len + 3, SAT_E_INVALID, "attention_hdw (causal): sk_pad must be >= s + 3 (key-side shift), got %d for s=%d", sk_pad, s_len);
    SAT_CHECK_ARG((((uintptr_t)q | (uintptr_t)k | (uintptr_t)vt | (uintptr_t)out) & 15) == 0, SAT_E_INVALID,
                  "attention_hdw (causal): pointers must be 16-byte aligned");
    if (head_dim == 32) return launch<32, true>(q, k, vt, out, b, h, kvh, s_len, s_len, sq_pad, sk_pad, s);
    if (head_dim == 96) return launch<96, true>(q, k, vt, out, b, h, kvh, s_len, s_len, sq_pad, sk_pad, s);
    return launch<128, true>(q, k, vt, out, b, h, kvh, s_len, s_len, sq_pad, sk_pad, s);
}
