// The pieces every attention kernel is built from -- attention.hip, the fused to_q + cross-attention epilogue of the 128 x 64 GEMM tile
// (gemm_bf16.hip), attention_hdw.hip (32-, 96-, 128-channel heads) and attention_window.hip (neighbourhood attention): the per-wave step
// attn::tile over a layout and a mask, the three-stage ring walk attn::walk3, the output store attn::store_out and, for the host side, the
// launchers' argument checks.  One wave = 32 queries (lane l and l ^ 32 share query l & 31), one call of the step = one LDS tile of 64 or
// 128 keys in blocks of 32.  Reference: models/transformer.py:496-536 (softmax(q k^T / sqrt(W)) v, fp32 softmax).
//
// Both products are computed transposed (see attention.hip): S^T = K Q^T with the K fragment from LDS as the A operand and Q in
// registers as B; O^T = V^T P^T with the V^T fragment from LDS as A and the lane's own 16 probabilities as B.
//
// Online softmax WITHOUT a per-block maximum.  Any per-query reference m_ref gives the same quotient sum(p v) / sum(p), p =
// 2^(s - m_ref), as long as nothing overflows; so the reference stands still and the row sum doubles as the overflow check (every p
// is <= its lane's sum).  Only when some lane's sum leaves [0, 2^12] -- always in the first block, later only for a score more than
// 12 octaves above the reference -- the block is redone the classic way (true maximum, accumulators rescaled).  The kernel is bound
// by VALU issue (profiles/r03_issue_rates.txt: 16 v_exp_f32 + 16 v_fma_f32 + 16 v_add_f32 + 8 v_cvt_pk_bf16_f32 per 32 keys against
// 8 MFMAs); this removes the 8 v_max3_f32, the exchange, the second exponential and -- for random scores in about every second
// tile -- the 32 accumulator multiplies of the textbook recurrence.
//   MODE 1: p = exp2(fma(s, scale_log2, -m_ref)).
//   MODE 2 (Q pre-scaled by scale_log2 by its producer): the reference rides in the matrix pipe -- a fifth K-step
//           [1, 0, ...] x [-m_ref, 0, ...] makes the accumulator come out as log2-domain score minus reference, p = exp2(acc): the 16
//           v_fma_f32 disappear from the VALU stream, the matrix pipe has the slack.  m_ref is kept representable in the operand type (bf16 / fp16).
#pragma once
#include "attn_causal.h"
#include "attn_hdw_tiles.h"
#include "attn_window.h"
#include "sat_common.h"

namespace attn {

constexpr int KV_TILE = 64;

__device__ __forceinline__ float half_max(float v) {     // max over the lane pair (l, l ^ 32), in both lanes
    unsigned a = __float_as_uint(v), b = a;
    u32x2 r = __builtin_amdgcn_permlane32_swap(a, b, false, false);
    return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
__device__ __forceinline__ float half_sum(float v) {
    unsigned a = __float_as_uint(v), b = a;
    u32x2 r = __builtin_amdgcn_permlane32_swap(a, b, false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

// Where a tile lies in LDS and how wide the head is.  KSTEPS K-steps of 16 channels, DB output blocks of 32 channels, KB blocks of 32 keys per
// tile; k_off / vt_off: byte offset of (row, 16-byte chunk) in the K tile / the V^T tile.  PRESCALED: Q arrives multiplied by log2(e) / sqrt(W),
// the scores are log2-domain as they leave the matrix pipe and scale_log2 is not read (MODE 1 only).
struct Layout64 {          // 64-channel heads, 64-key tiles of 128-byte rows: lds_tile_off of sat_common.h
    static constexpr int KSTEPS = 4, DB = 2, KB = 2;
    static constexpr bool PRESCALED = false;
    static __device__ __forceinline__ int k_off(int row, int chunk) { return lds_tile_off(row, chunk); }
    static __device__ __forceinline__ int vt_off(int row, int chunk) { return lds_tile_off(row, chunk); }
};
template <int W>
struct LayoutHdw {         // 32-, 96- and 128-channel heads: the tiles of attn_hdw_tiles.h
    using T = attnw::Tiles<W>;
    static constexpr int KSTEPS = W / 16, DB = W / 32, KB = T::KV_TILE / 32;
    static constexpr bool PRESCALED = true;
    static __device__ __forceinline__ int k_off(int row, int chunk) { return T::k_tile_off(row, chunk); }
    static __device__ __forceinline__ int vt_off(int row, int chunk) { return T::vt_tile_off(row, chunk); }
};

// Which keys of a tile a query sees
enum Mask {
    MASK_NONE = 0,        // all of [k_lo, k_hi), the same for every query: only the sequence's first and last tile have keys outside (`edge`)
    MASK_CAUSAL = 1,      // self-attention of a causal model: the block classes of attn_causal.h
    MASK_WINDOW = 2,      // neighbourhood attention: the block classes of attn_window.h
};

template <int MODE, int NDB = 2>
struct State {
    f32x16 oacc[NDB];       // O^T: channels d = db*32 + 8*(r>>2) + 4*half + (r&3) of the lane's query
    float m_run;            // reference, log2-scaled units
    float l_run;            // this lane's partial row sum (its 16 of every 32 keys)
    opx8 ones_a, mref_b;  // MODE 2: the fifth K-step

    __device__ __forceinline__ void init(int half) {
#pragma unroll
        for (int i = 0; i < NDB; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) oacc[i][r] = 0.f;
        m_run = MODE == 2 ? 0.f : -1e30f;
        l_run = 0.f;
        if constexpr (MODE == 2) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                ones_a[j] = f32_to_op(0.f);
                mref_b[j] = f32_to_op(0.f);
            }
            if (half == 0) ones_a[0] = f32_to_op(1.0f);
        }
    }
};

// One tile of 32 * L::KB keys at LDS addresses sk (K tile) / sv (V^T tile), both in the layout L.  key_base = the tile's first key.
// first: the sequence's first tile for this wave (MODE 2 fixes a real reference there whatever the sums say: underflow safety).
// DBG (experiments build, wrong results, Layout64): 1 no exp / max / sum; 3 no MFMA; 5 fragments not read from LDS.
// MASK_NONE: edge = some keys of the tile lie outside [k_lo, k_hi) and are masked.  A tile of more than two blocks ends at the first block that
// is all tail pad (wave-uniform; block 0 of a tile never is).
// MASK_CAUSAL (MODE 1 only): the wave owns the queries [cq_first, cq_first + 32) of a sequence of cS rows whose keys start at k_lo; each 32-key
// block is classed by attn_causal.h -- SKIP ends the tile (wave-uniform; the later blocks lie higher still), DIAG takes the edge path with the
// LANE's own k_hi (attnc::key_end of its query), FULL the unmasked path.  `edge` is not read.
// MASK_WINDOW (MODE 1 only): wr = attnw::wave_range of the wave's queries, [k_lo, k_hi) the LANE's own window in physical keys (pads lie outside
// every window); each block is classed by attn_window.h -- SKIP passes over the block, EDGE masks per element, FULL does not.  `edge` is not read.
// Masked lanes and the standing reference: the reference starts at -1e30, so a lane's first visible key gives p = exp2(s + 1e30) = inf, the row
// sum fails the overflow check and the block is redone with the true maximum -- also for rows whose log2-domain scores all lie below -126.  A
// lane that sees no key of a block has scores of -inf there, p = exp2(-inf - m) = 0; if it has met no key at all its maximum stays fmax(-1e30,
// -inf) = -1e30, the rescale is by exp2(0) = 1 and (m, l, O) = (-1e30, 0, 0) survives until its keys begin (causal: the first block of a
// sequence holds key k_lo, which every query sees; window: the lanes of a wave meet their first key in different blocks).
template <int MODE, int DBG = 0, int MASK = MASK_NONE, class L = Layout64>
__device__ __forceinline__ void tile(State<MODE, L::DB>& st, const opx8 (&qf)[L::KSTEPS], const char* sk, const char* sv, const bool edge,
                                     const int key_base, const int k_lo, const int k_hi, const bool first, const float scale_log2, const int l31,
                                     const int half, const int cq_first = 0, const int cS = 0, const attnw::Range& wr = attnw::Range{}) {
    static_assert(MASK == MASK_NONE || MODE == 1, "the masked walks are built for the standing-reference recurrence");
    static_assert(!L::PRESCALED || MODE == 1, "a pre-scaled layout runs the standing-reference recurrence without the scale");
    static_assert(DBG == 0 || L::KSTEPS == 4, "the ablations are written for the 64-channel layout");
    static_assert(int(attnc::SKIP) == int(attnw::SKIP) && int(attnc::DIAG) == int(attnw::EDGE), "one test serves both sets of block classes");
#pragma unroll
    for (int kb = 0; kb < L::KB; ++kb) {
        if (MASK == MASK_NONE && L::KB > 2 && key_base + kb * 32 >= k_hi) break;
        [[maybe_unused]] int cls = attnc::FULL;
        if constexpr (MASK == MASK_CAUSAL) {
            cls = attnc::block_class(key_base + kb * 32, cq_first, 32, k_lo, cS);
            if (cls == attnc::SKIP) break;
        }
        if constexpr (MASK == MASK_WINDOW) {
            cls = attnw::block_class(key_base + kb * 32, wr);      // wave-uniform
            if (cls == attnw::SKIP) continue;
        }
        // ---- S^T = K Q^T for 32 keys
        opx8 kf[L::KSTEPS];
#pragma unroll
        for (int t = 0; t < L::KSTEPS; ++t) {
            if constexpr (DBG == 5) kf[t] = qf[t];
            else kf[t] = *reinterpret_cast<const opx8*>(sk + L::k_off(kb * 32 + l31, t * 2 + half));
        }
        f32x16 sacc;
#pragma unroll
        for (int r = 0; r < 16; ++r) sacc[r] = DBG == 3 ? (float)kf[r & 3][r >> 2] : 0.f;
        if constexpr (DBG != 3) {
            if constexpr (MODE == 2) sacc = mfma_32x32x16(st.ones_a, st.mref_b, sacc);
#pragma unroll
            for (int t = 0; t < L::KSTEPS; ++t) sacc = mfma_32x32x16(kf[t], qf[t], sacc);
        }
        // V^T fragments do not depend on the softmax: request them now, their LDS latency hides behind the VALU work
        opx8 vf[L::DB][2];
#pragma unroll
        for (int db = 0; db < L::DB; ++db)
#pragma unroll
            for (int u = 0; u < 2; ++u)
                if constexpr (DBG == 5) vf[db][u] = qf[db * 2 + u];
                else vf[db][u] = *reinterpret_cast<const opx8*>(sv + L::vt_off(db * 32 + l31, (kb * 2 + u) * 2 + half));
        // ---- mask the keys outside [k_lo, k_hi) (wave-uniform branch; MASK_NONE: first and last tile only)
        if (MASK == MASK_NONE ? edge : cls == attnc::DIAG) {
            const int key0 = key_base + kb * 32 + 4 * half;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int key = key0 + (r & 3) + 8 * (r >> 2);
                if (key < k_lo || key >= k_hi) sacc[r] = -INFINITY;
            }
        }
        // ---- online softmax step (per query = per lane pair)
        // the exponent of a score against the standing reference (MODE 2: already subtracted by the matrix pipe)
        const auto expo = [&](float s) { return L::PRESCALED ? s - st.m_run : fmaf(s, scale_log2, -st.m_run); };
        opx8 pb[2];
        if constexpr (DBG == 1) {
#pragma unroll
            for (int r = 0; r < 16; ++r) pb[r >> 3][r & 7] = f32_to_op(sacc[r]);
            st.l_run += sacc[0];
        } else {
            // fast path: exponentials against the standing reference
            float psum = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float p = __builtin_amdgcn_exp2f(MODE == 2 ? sacc[r] : expo(sacc[r]));
                psum += p;
                pb[r >> 3][r & 7] = f32_to_op(p);
            }
            const bool redo = (MODE == 2 && first && kb == 0) || !__all(psum <= 4096.0f);       // wave-uniform; NaN-safe (inf - inf cannot arise)
            if (redo) {
                float mloc = sacc[0];
#pragma unroll
                for (int r = 1; r < 16; ++r) mloc = fmaxf(mloc, sacc[r]);
                float shift;              // what to add to the fast path's exponent
                if constexpr (MODE == 2) {
                    // the sequence's first block SETS the reference to the true maximum (the initial 0 is not a lower bound: a query whose
                    // log2-domain scores all lie below -126 would otherwise flush every p to 0 and divide by a zero row sum);
                    // later blocks only ever raise it
                    const float cand = half_max(mloc) + st.m_run;
                    const float m_new = op_to_f32(f32_to_op((first && kb == 0) ? cand : fmaxf(st.m_run, cand)));
                    shift = st.m_run - m_new;                      // <= 0 up to the operand-type rounding of m_new (first block: any sign)
                    st.m_run = m_new;
                    st.mref_b[0] = f32_to_op(half == 0 ? -m_new : 0.f);
                } else {
                    const float m_new = fmaxf(st.m_run, L::PRESCALED ? half_max(mloc) : half_max(mloc) * scale_log2);
                    shift = st.m_run - m_new;
                    st.m_run = m_new;
                }
                // (MODE 2, first block: nothing is accumulated yet and the shift may have either sign -- 0 * 2^shift must not become 0 * inf)
                const float alpha = (MODE == 2 && first && kb == 0) ? 1.0f : __builtin_amdgcn_exp2f(shift);
                st.l_run *= alpha;
#pragma unroll
                for (int i = 0; i < L::DB; ++i)
#pragma unroll
                    for (int r = 0; r < 16; ++r) st.oacc[i][r] *= alpha;
                psum = 0.f;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float p = __builtin_amdgcn_exp2f(MODE == 2 ? sacc[r] + shift : expo(sacc[r]));
                    psum += p;
                    pb[r >> 3][r & 7] = f32_to_op(p);
                }
            }
            st.l_run += psum;
        }
        // ---- O^T += V^T P^T
#pragma unroll
        for (int db = 0; db < L::DB; ++db)
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                if constexpr (DBG == 3) st.oacc[db][u] += (float)vf[db][u][0] * (float)pb[u][0];
                else st.oacc[db] = mfma_32x32x16(vf[db][u], pb[u], st.oacc[db]);
            }
    }
}

// The key walk of the one-ring kernels: the tiles [t_first, t_first + t_count) through a ring of THREE stages, prefetch distance 2, one raw
// s_barrier per tile (never __syncthreads() with an LDS-DMA in flight).  stage_in(tile, stage) issues this wave's PIECES LDS-DMA pieces of a
// tile, process(tile, stage) consumes one.  Tile it + 1 stays in flight across the barrier (counted vmcnt: this wave issued PIECES pieces for
// it); tile it + 2 goes into the stage tile it - 1 occupied, which every wave left before this barrier.
template <int PIECES, class StageIn, class Process>
__device__ __forceinline__ void walk3(const int t_first, const int t_count, StageIn&& stage_in, Process&& process) {
    stage_in(t_first, 0);
    if (t_count > 1) stage_in(t_first + 1, 1);
    int stg = 0;
    for (int it = 0; it < t_count; ++it) {
        if (it + 1 < t_count) wait_vmcnt<PIECES>();
        else wait_vmcnt<0>();
        __builtin_amdgcn_s_barrier();
        const int stg2 = stg >= 1 ? stg - 1 : 2;                 // (it + 2) % 3
        if (it + 2 < t_count) stage_in(t_first + it + 2, stg2);
        process(t_first + it, stg);
        stg = stg == 2 ? 0 : stg + 1;
    }
}

// The output rows of a wave in the operand type: O^T scaled by inv = 1 / row sum, 32 channels per block at op + 32 db (op: the lane's row,
// channel 8 * half of the head).  half_swap gives every lane 8 consecutive channels: one 16-byte store instead of two 8-byte ones.
template <int NDB>
__device__ __forceinline__ void store_out(const f32x16 (&oacc)[NDB], const float inv, op_t* op, const bool ok) {
#pragma unroll
    for (int db = 0; db < NDB; ++db) {
        unsigned pk[8];
#pragma unroll
        for (int rq = 0; rq < 4; ++rq) {
            pk[2 * rq] = pack_op2(oacc[db][rq * 4] * inv, oacc[db][rq * 4 + 1] * inv);
            pk[2 * rq + 1] = pack_op2(oacc[db][rq * 4 + 2] * inv, oacc[db][rq * 4 + 3] * inv);
        }
        half_swap(pk[0], pk[2]);
        half_swap(pk[1], pk[3]);
        half_swap(pk[4], pk[6]);
        half_swap(pk[5], pk[7]);
        if (ok) {
            *reinterpret_cast<u32x4*>(op + db * 32) = u32x4{pk[0], pk[1], pk[2], pk[3]};
            *reinterpret_cast<u32x4*>(op + db * 32 + 16) = u32x4{pk[4], pk[5], pk[6], pk[7]};
        }
    }
}

}  // namespace attn

// The argument checks of the attention launchers, over their own parameter names q, k, vt, out, b, h, kvh, sq_pad, sk_pad.  what: the prefix of
// the messages; sq, sk: the lengths (a self-attention launcher passes its s_len twice), sname how the message names the key length ("sk" |
// "s"); grid: also refuse what the grid's y and z cannot hold; tile64: also ask for the padding of the 64-channel kernels (attention_hdw.hip
// checks its per-width tile in launch<W>)
#define SAT_CHECK_ATTENTION(what, sname, sq, sk, grid, tile64)                                                                                     \
    SAT_CHECK_ARG(q && k && vt && out, SAT_E_INVALID, what ": null pointer");                                                                      \
    SAT_CHECK_ARG(b > 0 && h > 0 && kvh > 0 && h % kvh == 0, SAT_E_INVALID, what ": bad heads %d/%d", h, kvh);                                     \
    SAT_CHECK_ARG(!(grid) || (h <= 65535 && b <= 65535), SAT_E_UNSUPPORTED, what ": %d heads / %d sequences exceed the grid", h, b);               \
    SAT_CHECK_ARG((sq) > 0 && (sk) > 0 && sq_pad >= (sq) && sk_pad >= (sk), SAT_E_INVALID, what ": bad lengths");                                  \
    SAT_CHECK_ARG(!(tile64) || (sq_pad % 128 == 0 && sk_pad % 64 == 0), SAT_E_INVALID, what ": sq_pad %% 128 and sk_pad %% 64 must be 0 (got %d, %d)", \
                  sq_pad, sk_pad);                                                                                                                 \
    SAT_CHECK_ARG(sk_pad >= (sk) + 3, SAT_E_INVALID, what ": sk_pad must be >= " sname " + 3 (key-side shift), got %d for " sname "=%d", sk_pad, (sk)); \
    SAT_CHECK_ARG((((uintptr_t)q | (uintptr_t)k | (uintptr_t)vt | (uintptr_t)out) & 15) == 0, SAT_E_INVALID, what ": pointers must be 16-byte aligned")
