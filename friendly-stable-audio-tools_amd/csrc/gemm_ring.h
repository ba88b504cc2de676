// Device pieces of the DiT GEMM kernels of gemm_bf16.hip that have one text here instead of one per use: the pinned
// MFMA / DS-read / LDS-DMA interleaves of the ring kernel's fragment loops, the K-groups' mid-iteration barrier, and
// the staging of the fused cross-attention's K / V^T tiles.  The ring kernel's geometry is RingGeom (gemm_ring_geom.h).
// Every piece here leaves the instruction streams of all kernels as they were with the text in place (tools/kernel_identity.py);
// profiles/gemm_ring_fold.txt lists the pieces that did not and therefore stay in gemm_pipe_kernel.
#pragma once
#include "attn_core.h"
#include "gemm_ring_geom.h"
#include "sat_common.h"

namespace {

// ---- pinned interleaves (sched_group_barrier masks: 0x8 MFMA, 0x100 DS read, 0x20 vector-memory read = LDS-DMA piece) -----------
// NR reads of the next step's fragments, PER behind each of the first MFMAs of this step's NM, then what is left of either.
// <NR, NM>: one read behind each MFMA; <NR, 1, NR>: all reads behind the first MFMA; <NR, 2, NR / 2>: half behind each of the first two
template <int NR, int NM, int PER = 1>
__device__ __forceinline__ void sched_reads_behind_mfmas() {
    constexpr int N = NR / PER < NM ? NR / PER : NM;
#pragma unroll
    for (int r = 0; r < N; ++r) {
        __builtin_amdgcn_sched_group_barrier(0x8, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, PER, 0);
    }
    if (NM > N) __builtin_amdgcn_sched_group_barrier(0x8, NM - N, 0);
    if (NR > N * PER) __builtin_amdgcn_sched_group_barrier(0x100, NR - N * PER, 0);
}
template <int N>
__device__ __forceinline__ void sched_mfmas_only() {
    __builtin_amdgcn_sched_group_barrier(0x8, N, 0);
}
// the iteration's DMA pieces two at a time -- N times: one MFMA, two pieces, MF more MFMAs
template <int N, int MF>
__device__ __forceinline__ void sched_dma_pairs_behind_mfmas() {
#pragma unroll
    for (int r = 0; r < N; ++r) {
        __builtin_amdgcn_sched_group_barrier(0x8, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x20, 2, 0);
        if (MF) __builtin_amdgcn_sched_group_barrier(0x8, MF, 0);
    }
}

// ---- K-groups -------------------------------------------------------------------------------------------------------------------
// mid-iteration: the OTHER group's iteration boundary (it runs half an iteration out of phase)
__device__ __forceinline__ void kgroup_mid_barrier() {
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
}

// ---- fused cross-attention (HeadsEpi::xa_k; RingGeom::XA_OK) --------------------------------------------------------------------
// The K / V^T tiles of (sequence b, the kv-head of column n0) -> LDS at `xa` (RingGeom::XA_OFF): 16 KiB per 64 keys, K rows then V^T
// rows; four waves, two 1-KiB pieces each per tile
__device__ __forceinline__ void xattn_stage_kv(const HeadsEpi& he, char* xa, const int b, const int n0, const int wave, const int lane) {
    const int kvh = (n0 >> 6) / (he.heads / he.xa_kvh);
    const op_t* kbase = he.xa_k + (size_t)(b * he.xa_kvh + kvh) * he.xa_sk_pad * 64;
    const op_t* vbase = he.xa_vt + (size_t)(b * he.xa_kvh + kvh) * 64 * he.xa_sk_pad;
    const int n_t = (((b * he.xa_sk) & 3) + he.xa_sk + 63) >> 6;
    for (int t = 0; t < n_t; ++t)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int p = wave + 4 * i;                          // 1-KiB piece = 8 rows of 128 B
            const int row = p * 8 + (lane >> 3);
            const int c = (lane & 7) ^ ((row >> 1) & 7);         // source-side XOR swizzle (lds_tile_off)
            char* dst = xa + t * 16384 + p * 1024;
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(kbase + (size_t)(t * 64 + row) * 64 + c * 8),
                                             (__attribute__((address_space(3))) void*)dst, 16, 0, 0);
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(vbase + (size_t)row * he.xa_sk_pad + t * 64 + c * 8),
                                             (__attribute__((address_space(3))) void*)(dst + 8192), 16, 0, 0);
        }
}

}  // namespace
