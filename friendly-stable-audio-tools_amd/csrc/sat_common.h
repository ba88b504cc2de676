// Shared device/host helpers for libsat_hip (gfx950 / CDNA4 only).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string>

#include "../../include/sat_hip.h"
#include "gemm_tiles.h"          // host-only integer logic: cdiv / round_up, the GemmArgs::variant fields, tiles and their choice, xcd_remap (ph8_sched.h)

typedef __bf16 bf16_t;
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

// ---------------------------------------------------------------------------------------
// The 16-bit OPERAND type of the matrix kernels.  gemm_bf16.hip, gemm_ph8.hip, attention.hip (+ attn_core.h) and oobleck.hip are
// compiled TWICE (csrc/Makefile): once with op_t = bf16 and once with -DSAT_OPERAND_F16, op_t = IEEE fp16 -- gfx950 runs
// v_mfma_f32_*_f16 at exactly the rate of the bf16 instructions (MI355X_MICROARCH.md), fp16 carries three more significand bits
// (8x less operand rounding), and fp16 is what the reference itself computes in on a GPU (inference/sampling.py:210 autocast,
// models/transformer.py:496-504 flash-attn fp16, models/pretransforms.py:39-59 model_half).  Everything that names the element type
// in those files goes through op_t / opx8 / f32_to_op / mfma_*; the host-facing launchers of the two builds live in namespace
// bf16 / f16 (SAT_OPNS), the bf16 build owns the un-namespaced dispatchers and every extern "C" symbol.  Files compiled once
// (dit_plan.hip, oobleck_plan.hip, layernorm.hip, ...) see op_t = bf16 and treat operand buffers as opaque storage.
// fp16 range policy: conversions SATURATE at +-65504 (MODE.FP16_OVFL, set by sat_f16_saturate() at the top of every kernel of the
// fp16 build) instead of producing infinities; inf / NaN inputs still propagate.
// A third operand format exists for oobleck.hip only: -DSAT_OPERAND_F32, op_t = float (namespace f32), the convolutions on the
// exact f32-input MFMA (the reference's model_half=False codec).  The 16-bit helpers below (mfma_32x32x16, pack_op2, ...) are not
// defined in that build.  oobleck.hip holds kernels and launchers only and exports one table of launchers per build
// (SAT_OPNS::oob_kernels(), oobleck_kernels.h); the codec's plan and its extern "C" symbols are oobleck_plan.hip, compiled once.
#ifdef SAT_OPERAND_F16
typedef _Float16 op_t;
#define SAT_OPNS f16
#define SAT_OP_IS_F16 1
#elif defined(SAT_OPERAND_F32)
typedef float op_t;
#define SAT_OPNS f32
#define SAT_OP_IS_F16 0
#else
typedef __bf16 op_t;
#define SAT_OPNS bf16
#define SAT_OP_IS_F16 0
#endif
#ifdef SAT_OPERAND_F32
#define SAT_OP_IS_F32 1
#else
#define SAT_OP_IS_F32 0
#endif
typedef op_t opx8 __attribute__((ext_vector_type(8)));
typedef op_t opx4 __attribute__((ext_vector_type(4)));
typedef op_t opx2 __attribute__((ext_vector_type(2)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

void sat_set_error(const char* fmt, ...);

#define SAT_CHECK_ARG(cond, code, ...)            \
    do {                                          \
        if (!(cond)) {                            \
            sat_set_error(__VA_ARGS__);           \
            return (code);                        \
        }                                         \
    } while (0)

#define SAT_HIP(call)                                                                       \
    do {                                                                                    \
        hipError_t e__ = (call);                                                            \
        if (e__ != hipSuccess) {                                                            \
            sat_set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e__), __FILE__, __LINE__); \
            return (int)e__;                                                                \
        }                                                                                   \
    } while (0)

#define SAT_LAUNCH_CHECK()                                                                  \
    do {                                                                                    \
        hipError_t e__ = hipGetLastError();                                                 \
        if (e__ != hipSuccess) {                                                            \
            sat_set_error("kernel launch failed: %s (%s:%d)", hipGetErrorString(e__), __FILE__, __LINE__); \
            return (int)e__;                                                                \
        }                                                                                   \
    } while (0)

#define SAT_TRY(expr)            \
    do {                         \
        int rc__ = (expr);       \
        if (rc__ != 0) return rc__; \
    } while (0)

// hipFuncAttributeMaxDynamicSharedMemorySize is a per-DEVICE property of a kernel: raise it once per (kernel, device), not once
// per process (a second GPU in the same process would otherwise launch with the 64 KiB default and fail).  Thread-safe.
int sat_ensure_dynamic_lds(const void* kernel, int bytes);
int sat_device_cus();          // compute units of the current device (cached per device; 0 + sat_last_error on failure)

// ---------------------------------------------------------------------------------------
// device helpers
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ float bf16_to_f32(bf16_t v) { return (float)v; }
__device__ __forceinline__ bf16_t f32_to_bf16(float v) { return (bf16_t)v; }   // RNE
__device__ __forceinline__ float op_to_f32(op_t v) { return (float)v; }
__device__ __forceinline__ op_t f32_to_op(float v) { return (op_t)v; }          // RNE (fp16: saturating under sat_f16_saturate)

// fp16 build: overflowing float -> half conversions clamp to +-65504 (MODE.FP16_OVFL, bit 23 of the MODE register) instead of
// returning infinity.  One scalar instruction at kernel entry; a no-op in the bf16 build.
__device__ __forceinline__ void sat_f16_saturate_on() { asm volatile("s_setreg_imm32_b32 hwreg(HW_REG_MODE, 23, 1), 1"); }
__device__ __forceinline__ void sat_f16_saturate() {
#ifdef SAT_OPERAND_F16
    sat_f16_saturate_on();
#endif
}
// kernels templated on their 16-bit output type (layernorm.hip, dit_glue.hip: compiled once)
template <typename OT>
__device__ __forceinline__ void sat_saturate_for() {
    if constexpr (__is_same(OT, _Float16)) sat_f16_saturate_on();
}

#if !SAT_OP_IS_F32
// the two dense 16-bit MFMAs of gfx950 on the operand type of this build (same rate for bf16 and fp16)
__device__ __forceinline__ f32x16 mfma_32x32x16(opx8 a, opx8 b, f32x16 c) {
#ifdef SAT_OPERAND_F16
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
#else
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
#endif
}
__device__ __forceinline__ f32x4 mfma_16x16x32(opx8 a, opx8 b, f32x4 c) {
#ifdef SAT_OPERAND_F16
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
#else
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
#endif
}
#endif

__device__ __forceinline__ float silu_f(float x) { return x / (1.0f + __expf(-x)); }

// Wave-wide reductions without LDS traffic: four DPP steps reduce every row of 16 lanes (quad xor 1, quad xor 2, row_half_mirror,
// row_mirror), row_bcast:15 / row_bcast:31 fold the four rows into lane 63, v_readlane broadcasts the result through an SGPR.
// 7 VALU instructions instead of six ds_bpermute round trips (__shfl_xor).
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_move_masked(float v) {      // lanes outside ROW_MASK receive 0
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, ROW_MASK, 0xf, false));
}
template <int CTRL>
__device__ __forceinline__ float dpp_row_move(float v) {
    const int i = __float_as_int(v);
    return __int_as_float(__builtin_amdgcn_update_dpp(i, i, CTRL, 0xf, 0xf, false));
}
__device__ __forceinline__ float wave_sum(float v) {
    v += dpp_row_move<0xB1>(v);                    // quad_perm [1,0,3,2]
    v += dpp_row_move<0x4E>(v);                    // quad_perm [2,3,0,1]
    v += dpp_row_move<0x141>(v);                   // row_half_mirror
    v += dpp_row_move<0x140>(v);                   // row_mirror: every lane of a row holds the row sum
    v += dpp_move_masked<0x142, 0xA>(v);           // row_bcast:15 into rows 1 and 3
    v += dpp_move_masked<0x143, 0xC>(v);           // row_bcast:31 into rows 2 and 3: lane 63 holds the total
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}
__device__ __forceinline__ float wave_max(float v) {   // for non-negative inputs or any inputs: the masked moves use v itself as filler
    v = fmaxf(v, dpp_row_move<0xB1>(v));
    v = fmaxf(v, dpp_row_move<0x4E>(v));
    v = fmaxf(v, dpp_row_move<0x141>(v));
    v = fmaxf(v, dpp_row_move<0x140>(v));
    {
        const int i = __float_as_int(v);
        v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(i, i, 0x142, 0xA, 0xf, false)));
    }
    {
        const int i = __float_as_int(v);
        v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(i, i, 0x143, 0xC, 0xf, false)));
    }
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}

// max over the 32 lanes of a wave half (lanes 0-31 / 32-63), result in every lane: four DPP steps (quad xor 1, quad xor 2,
// row_half_mirror, row_mirror -> max of each row of 16) and one ds_swizzle that swaps the two rows of a half.  No address
// VGPRs, no ds_bpermute: 6 instructions against ~15 for five __shfl_xor steps.
template <int CTRL>
__device__ __forceinline__ float dpp_move(float v) {
    const int i = __float_as_int(v);
    return __int_as_float(__builtin_amdgcn_update_dpp(i, i, CTRL, 0xf, 0xf, false));
}
__device__ __forceinline__ float half32_max(float v) {
    v = fmaxf(v, dpp_move<0xB1>(v));       // quad_perm [1,0,3,2]
    v = fmaxf(v, dpp_move<0x4E>(v));       // quad_perm [2,3,0,1]
    v = fmaxf(v, dpp_move<0x141>(v));      // row_half_mirror
    v = fmaxf(v, dpp_move<0x140>(v));      // row_mirror
    return fmaxf(v, __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(v), 0x401F)));   // lane ^ 16
}

// sum over each aligned group of 16 lanes (one DPP row), result in all 16 lanes
__device__ __forceinline__ float row16_sum(float v) {
    v += dpp_move<0xB1>(v);
    v += dpp_move<0x4E>(v);
    v += dpp_move<0x141>(v);
    v += dpp_move<0x140>(v);
    return v;
}
// sum over the 32 lanes of a wave half, result in every lane (half32_max with +)
__device__ __forceinline__ float half32_sum(float v) {
    v = row16_sum(v);
    return v + __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(v), 0x401F));   // lane ^ 16
}

// Accumulators of a 32x32 MFMA block issued with the operands swapped (weight fragment first) hold C^T: lane l31 owns one output ROW,
// its 16 registers are channels 8*(r>>2) + 4*half + (r&3) -- four runs of four.  half_swap exchanges one dword of runs g and g+1
// between the wave halves (v_permlane32_swap): afterwards lanes 0-31 hold (run g of half 0, run g of half 1) = 8 consecutive
// channels from 8g, lanes 32-63 (run g+1 of half 0, run g+1 of half 1) = 8 consecutive channels from 8(g+1).
__device__ __forceinline__ void half_swap(unsigned& lo_run, unsigned& hi_run) {
    u32x2 r = __builtin_amdgcn_permlane32_swap(lo_run, hi_run, false, false);
    lo_run = r[0];
    hi_run = r[1];
}
__device__ __forceinline__ unsigned pack_bf16x2(float a, float b) {
    bf16x2 v;
    v[0] = f32_to_bf16(a);
    v[1] = f32_to_bf16(b);
    return __builtin_bit_cast(unsigned, v);
}
#if !SAT_OP_IS_F32
__device__ __forceinline__ unsigned pack_op2(float a, float b) {
    opx2 v;
    v[0] = f32_to_op(a);
    v[1] = f32_to_op(b);
    return __builtin_bit_cast(unsigned, v);
}
#endif
// the same exchange on the fp32 values of a whole block: afterwards v[0..7] are channels c0 .. c0+7 and v[8..15] channels
// c0+16 .. c0+23 of the lane's row, c0 = 8 * half (16-byte residual reads, 16-byte bf16 stores after packing)
__device__ __forceinline__ void gather_channel_runs(const f32x16& a, float (&v)[16]) {
#pragma unroll
    for (int g = 0; g < 4; g += 2)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            unsigned lo = __float_as_uint(a[4 * g + e]), hi = __float_as_uint(a[4 * (g + 1) + e]);
            half_swap(lo, hi);
            v[4 * g + e] = __uint_as_float(lo);
            v[4 * (g + 1) + e] = __uint_as_float(hi);
        }
}

// LDS tile layout used by the MFMA kernels: rows of 64 bf16 (128 B = eight 16-B chunks);
// chunk c of row r lives at chunk (c ^ ((r >> 1) & 7)).  With this XOR every 16-lane group
// of a ds_read_b128 fragment read (16 distinct rows, same logical chunk) covers all 16
// 16-B slots of the 256-B bank row: conflict-free; an 8-lane ds_write_b128 group (one row,
// 8 chunks) is conflict-free as well.
__device__ __forceinline__ int lds_tile_off(int row, int chunk) {
    return row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4);
}

// Position of key s inside V^T ([.., 64, Spad], key index contiguous): bits 2 and 3 of the index are swapped, i.e. every aligned
// group of 16 keys is stored as [0-3, 8-11, 4-7, 12-15].  That is the order in which the second attention MFMA consumes the
// probabilities a lane holds after the first one (attention.hip), so a V^T tile can be copied to LDS verbatim (LDS-DMA, 16-byte
// pieces) and read as fragments without any re-arrangement.  Involution; groups of 4 consecutive keys stay together.
__host__ __device__ __forceinline__ int vt_pos(int s) { return (s & ~12) | ((s & 4) << 1) | ((s & 8) >> 1); }

// counted wait on outstanding vector-memory operations (LDS-DMA pieces included); hipcc does not see inside the asm,
// which is the point: the compiler never drains the in-flight prefetch ring with a vmcnt(0)
template <int N>
__device__ __forceinline__ void wait_vmcnt() {
    static_assert(N >= 0 && N < 64, "vmcnt immediate is 6 bits");
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// ---------------------------------------------------------------------------------------
// internal launchers shared between translation units (EPI_F32 / EPI_RESID / EPI_SWIGLU / EPI_HEADS: gemm_tiles.h)
// ---------------------------------------------------------------------------------------

namespace SAT_OPNS {

struct HeadsEpi {
    op_t* out[3];      // per part destination
    int kind[3];         // bit0: transposed ([B,Hh,64,Spad]) else [B,Hh,Spad,64]; bit1: apply RoPE;
                         // bit2: key-side tensor (K / V^T): rows/columns of sequence b shifted by (b*S)&3
                         // bit3: query tensor written PRE-SCALED by `qscale` (row-major destinations only): the attention
                         //       kernel then gets log2-domain scores straight out of its first MFMA (SAT_ATTN_QSCALE)
                         // bit4: qk_norm (transformer.py:433-436): every head row is L2-normalised on the fp32 accumulators, x / max(|x|, 1e-12),
                         //       before the rotation and the pre-scale (row-major destinations, 16-bit operands).  Any part with this bit sends
                         //       the launch to the EPI_HEADS_QKN instantiations of the ring tiles; without it nothing changes
    float qscale;
    // Fused cross-attention (one part, row-major, pre-scaled, 128 x 64 tile = one head per workgroup column): the epilogue does not
    // store Q at all -- each wave keeps its 32 queries x 64 channels as MFMA fragments and runs softmax(q k^T) v against the
    // (batch, kv-head)'s keys / values, which the workgroup staged in LDS behind the GEMM ring at kernel start
    // (models/transformer.py:496-536 behind :430-437).  xa_k == nullptr: off.
    const op_t* xa_k;      // [B, kvh, sk_pad, 64], key-side layout of sat_attention_bf16
    const op_t* xa_vt;     // [B, kvh, 64, sk_pad]
    op_t* xa_out;          // [M, heads * 64]
    int xa_kvh, xa_sk, xa_sk_pad;
    int parts;           // N == parts * heads * 64
    int heads;           // heads per part
    int S;               // valid rows per sequence (row m -> b = m / S, s = m % S)
    int Spad;            // padded sequence length of the destination
    const float* rope_cos;   // [>=S][16]
    const float* rope_sin;
};

struct GemmArgs {
    int f16;             // operand format of A / W / H / xb / heads.*: 0 = bf16, 1 = IEEE fp16 (routes to the fp16 build of the kernels)
    const op_t* A;     // [M,K]
    const op_t* W;     // [N,K]
    const float* bias;   // [N] or nullptr
    int M, N, K;
    int variant;         // forced tile, 8-phase switches, tile policy: the table in gemm_tiles.h
    // EPI_F32 / EPI_RESID
    float* C;            // [M,ldc]
    int ldc;
    int accumulate;
    // fp8 (e4m3) operands: A and W hold one byte per element (row-major, K contiguous), the fp32 accumulator is multiplied by
    // a_scale[row] * w_scale[col] (per-token x per-output-channel scales) before the epilogue; K % 128 == 0
    int fp8;
    const float* a_scale;   // [M]
    const float* w_scale;   // [N]
    // fp8 == 3 (MXFP8 A operand): one E8M0 scale per 32 k of every A row, [M][K/32] bytes = [M][K/128] dwords, applied by the
    // block-scaled MFMA itself; a_scale is unused
    const unsigned* a_bscale;
    // EPI_SWIGLU with H8 != nullptr: the hidden activation is written as MXFP8 (e4m3 bytes [M, N/2] + E8M0 [M, N/64]) instead of bf16
    unsigned char* H8;
    unsigned char* Hs;
    const float* gate;   // adaLN: (acc + bias) * gate[(row / gate_rows) * gate_ld + col] before the residual add; or nullptr
    int gate_rows, gate_ld;
    // EPI_SWIGLU
    op_t* H;           // [M, N/2]
    // EPI_HEADS
    HeadsEpi heads;
    // ---- LayerNorm folded into the GEMMs either side of the residual stream (bf16 operands, pipelined tiles only).
    // LN(x) W^T = rstd * (x (gamma (.) W)^T - mean * rowsum(gamma (.) W)) + beta W^T: the GEMM that UPDATES the residual stream
    // (EPI_RESID, the "producer") also writes the bf16 image of the new rows and, per row and 64-column block, the sum and the
    // sum of squares of those rounded values; the GEMM that CONSUMES the normalised rows (EPI_SWIGLU / EPI_HEADS) takes the bf16
    // image as its A operand, gamma-scaled weights, and finishes the normalisation on its fp32 accumulators.
    op_t* xb;                // producer: [M, N] bf16(C after the update), or nullptr
    float* ln_part_out;        // producer: [M][N / 64][2]
    const float* ln_part;      // consumer: [M][K / 64][2] partial (sum, sum of squares) of A's rows, or nullptr (no fold)
    const float* ln_c1;        // consumer: [N] sum_k bf16(gamma_k W_nk), epilogue channel order
    const float* ln_c2;        // consumer: [N] sum_k beta_k W_nk (+ bias_n)
    float ln_eps;
    // ---- scratch of the 8-phase kernel's K-split (fp32 output, long reductions: FF-out at the SA-2.0 shape): raw accumulator images
    // of the remainder round's partial K-ranges, [workgroups][65536] floats, added up by a second launch.  Caller-owned (the plan's
    // workspace), used by this launch only; nullptr = the remainder round's tiles stay whole.
    float* slab;
    size_t slab_bytes;
    // EPI_ACT16: H [M, N] = act(acc + bias), 0 = identity, 1 = SiLU (gemm_tiles.h)
    int act;
};

// bf16 build: checks a.f16 and forwards fp16 work to sat_launch_gemm_f16 (the fp16 build of the same file)
int sat_launch_gemm(int epi, const GemmArgs& a, hipStream_t stream);
size_t sat_gemm_ph8_slab_bytes(int epi, int M, int N, int K);      // slab workspace with which the automatic schedule splits the remainder round along K (0: never for this shape)
int sat_launch_gemm_ph8(int epi, int build, const GemmArgs& a, hipStream_t stream);     // gemm_ph8.hip: the 8-wave / 8-phase 256x256 tile, build = SatPh8Build
// out_scales != nullptr: MXFP8 output (e4m3 bytes at `out`, E8M0 per 32 channels at out_scales [b*sq][h*2]) instead of bf16
// q_scale: what the kernel still has to multiply in -- SAT_ATTN_QSCALE = 1/sqrt(64) * log2(e) for a plain Q, 1.0f for a Q the
// producer already wrote pre-scaled (HeadsEpi kind bit 3): only then the single-KV-group kernel carries its softmax reference
// through the matrix pipe (a plain Q would have to be rounded to bf16 a second time).
// f16 != 0: q / k / vt / out hold IEEE fp16 (bf16 build: forwards to sat_launch_attention_f16)
#define SAT_ATTN_QSCALE (0.125f * 1.4426950408889634f)
int sat_launch_attention(const op_t* q, const op_t* k, const op_t* vt, op_t* out, int b, int h, int kvh,
                         int sq, int sk, int sq_pad, int sk_pad, hipStream_t s, unsigned char* out_scales = nullptr,
                         float q_scale = SAT_ATTN_QSCALE, int f16 = 0);
// ---- 32-, 96- and 128-channel heads (the staged route of dit_plan.hip): head_split_hdw.hip, attention_hdw.hip.  Declared WEAK: dit_plan.hip
// is also linked, host-only, into a test driver that defines every launcher the 64-channel routes call and knows nothing of these; there they
// resolve to null and are never reached, in libsat_hip.so they resolve at link time.  The plan answers SAT_E_UNSUPPORTED where one is null.
// Layouts as sat_launch_attention with head_dim channels per head; Q pre-scaled by sat_attn_qscale(head_dim); sk_pad a multiple of
// sat_attn_hdw_key_tile(head_dim); no MXFP8 output form
__attribute__((weak)) int sat_launch_attention_hdw(const op_t* q, const op_t* k, const op_t* vt, op_t* out, int b, int h, int kvh, int head_dim, int sq,
                                                   int sk, int sq_pad, int sk_pad, hipStream_t s, int f16 = 0);
// x: fp32 [b * S, parts * heads * head_dim]; he: out / kind / qscale / parts / heads / S / Spad and the [S][sat_rope_pairs(head_dim)] rotation tables
__attribute__((weak)) int sat_launch_head_split_hdw(const float* x, const HeadsEpi& he, int head_dim, int b, hipStream_t s, int f16 = 0);
// ---- causal self-attention (sat_dit_plan_set_attention_options): sq == sk == s_len, query i sees the keys j <= i of its sequence (attn_causal.h).
// Layouts, pads and q_scale as the launchers above; no MXFP8 output form.  WEAK as the staged-route launchers: null in the host test driver,
// where sat_dit_plan_set_attention_options answers SAT_E_UNSUPPORTED to causal = 1
__attribute__((weak)) int sat_launch_attention_causal(const op_t* q, const op_t* k, const op_t* vt, op_t* out, int b, int h, int kvh, int s_len, int sq_pad,
                                                      int sk_pad, hipStream_t s, float q_scale = SAT_ATTN_QSCALE, int f16 = 0);
__attribute__((weak)) int sat_launch_attention_hdw_causal(const op_t* q, const op_t* k, const op_t* vt, op_t* out, int b, int h, int kvh, int head_dim,
                                                          int s_len, int sq_pad, int sk_pad, hipStream_t s, int f16 = 0);
// ---- neighbourhood self-attention (sat_dit_plan_set_neighborhood_attention; attention_window.hip, attn_window.h): 64-channel heads, sq == sk ==
// s_len >= kernel_size, query i sees the kernel_size keys from min(max(i - kernel_size / 2, 0), s_len - kernel_size) on.  Layouts and pads as
// sat_launch_attention.  score_scale: what the scores are multiplied by in front of exp2 -- log2(e) for a plain Q (the reference does not scale
// the logits of this branch), 1 for a Q its producer wrote times log2(e).  WEAK as the causal launchers
__attribute__((weak)) int sat_launch_attention_window(const op_t* q, const op_t* k, const op_t* vt, op_t* out, int b, int h, int kvh, int s_len, int sq_pad,
                                                      int sk_pad, int kernel_size, float score_scale, hipStream_t s, int f16 = 0);
// the same at 32-, 96- and 128-channel heads (sat_dit_plan_set_neighborhood_attention_hdw; attention_hdw_window.hip): layouts and pads as
// sat_launch_attention_hdw; there is no scale argument, Q arrives times log2(e) from the head split.  WEAK as above
__attribute__((weak)) int sat_launch_attention_hdw_window(const op_t* q, const op_t* k, const op_t* vt, op_t* out, int b, int h, int kvh, int head_dim,
                                                          int s_len, int sq_pad, int sk_pad, int kernel_size, hipStream_t s, int f16 = 0);
}  // namespace SAT_OPNS
using namespace SAT_OPNS;
// RotaryEmbedding(max(dim_heads / 2, 32)) (transformer.py:737): pairs (j, j + sat_rope_pairs) rotate, one angle per pair -- 16 for 32- and
// 64-channel heads, 24 for 96, 32 for 128
inline int sat_rope_pairs(int head_dim) { return (head_dim / 2 > 32 ? head_dim / 2 : 32) / 2; }
inline float sat_attn_qscale(int head_dim) { return (float)(1.4426950408889634 / sqrt((double)head_dim)); }      // log2(e) / sqrt(dim_heads)
inline int sat_attn_hdw_key_tile(int head_dim) { return head_dim == 32 ? 128 : 64; }                                // attn_hdw_tiles.h: 32 | 96, 128
__attribute__((weak)) int sat_launch_rope_table_hdw(const float* inv_freq, float* cos_t, float* sin_t, int s_len, int head_dim, hipStream_t s);      // [s_len][sat_rope_pairs]
// range_stats.hip: the reduction of the range reports (sat_range_record) over x[r * pitch + c], r < rows, c < cols, of `dtype` elements
// (SAT_GEMM_BF16 / SAT_GEMM_FP16 / SAT_GEMM_FP32X).  `counted` is what the record's `elements` grows by: rows * cols, or the logical count of
// a view that also scans the zero pads of its layout.  WEAK for the same reason as the 128-channel-head launchers: null in the host test driver,
// where the plans answer SAT_E_UNSUPPORTED to the request for a report and never reach it
__attribute__((weak)) int sat_launch_range_stats(const void* x, int dtype, int64_t rows, int64_t cols, int64_t pitch, uint64_t counted,
                                                 sat_range_record* rec, hipStream_t s);
// ---- block options (sat_dit_plan_set_block_options): conformer.hip.  WEAK as the launchers above: null in the host test driver, where a plan
// with block options answers SAT_E_UNSUPPORTED.  fmt: SAT_GEMM_BF16 / SAT_GEMM_FP16 (16-bit rows) or SAT_GEMM_FP32X (fp32 rows, the verification mode)
// The conformer's depthwise_conv (17 taps along the sequence, zero-padded by 8 at both ends of each of the b sequences of s_len rows), mid_norm
// over d and SiLU in one pass: x [b * s_len, d] -> y [b * s_len, d], both of `fmt`; w [d, 17] fp32 (transformer.py:571-573, 583-586)
__attribute__((weak)) int sat_launch_dwconv_ln_silu(const void* x, const float* w, const float* gamma, const float* beta, void* y, int b, int s_len,
                                                    int d, int fmt, hipStream_t s);
int sat_launch_dwconv_ln_silu_variant(const void* x, const float* w, const float* gamma, const float* beta, void* y, int b, int s_len, int d, int fmt,
                                      int variant, hipStream_t s);      // unit_entry.hip only: 1 one row per workgroup, 2 LDS-staged tile (measurements)
// remove_norms: the A operand of a projection is the residual row itself, y = x, or x * scale1p[b] + shift[b] under adaLN (b = row / rows_per_seq,
// vectors ld apart; scale1p null: no modulation), rounded to `fmt`
__attribute__((weak)) int sat_launch_round_rows(const float* x, void* y, int m, int d, const float* scale1p, const float* shift, int rows_per_seq,
                                                int ld, int fmt, hipStream_t s);
__attribute__((weak)) int sat_launch_silu_f32(float* h, int64_t n, hipStream_t s);      // fp32 verification mode: h = silu(h) in place (ff_kwargs glu=False)
// ---- convolutional feed-forward (sat_dit_plan_set_ff_conv): ff_conv.hip.  WEAK as the launchers above: null in the host test driver, where
// sat_dit_plan_set_ff_conv answers SAT_E_UNSUPPORTED to a kernel size above 1.  out[b, s, :] = sum_j W_j A[b, s + j - taps / 2, :] with zero
// rows outside [0, S) of sequence b: one contraction of length taps * K, fp32 accumulation
enum { FFC_RESID = 0, FFC_ACT16 = 1 };
struct FfConvArgs {
    int fmt;             // SAT_GEMM_BF16 / SAT_GEMM_FP16: the element type of A, W and H
    const void* A;       // [B * S, K], dense rows
    const void* W;       // [N, taps * K], tap-major (sat_launch_pack_conv_taps)
    const float* bias;   // [N] or nullptr
    int B, S, N, K, taps;
    int epi;             // FFC_RESID: C [B * S, ldc] (+)= [gate (.)] (acc + bias), gate as GemmArgs::gate; FFC_ACT16: H [B * S, N] = act(acc + bias)
    float* C;
    int ldc, accumulate;
    const float* gate;
    int gate_rows, gate_ld;
    void* H;
    int act;             // 0 identity, 1 SiLU
};
__attribute__((weak)) int sat_launch_ff_conv(const FfConvArgs& a, hipStream_t s);
// Conv1d weight w [n, k, taps] fp32 -> out [n, taps * k] of `fmt` (SAT_GEMM_BF16 / SAT_GEMM_FP16 / SAT_GEMM_FP32X), out[n][j * k + c] = w[n][c][j]
__attribute__((weak)) int sat_launch_pack_conv_taps(const float* w, void* out, int n, int k, int taps, int fmt, hipStream_t s);
// fp32 verification mode: out [b * s_len, taps * k], out[m][j * k + c] = a[m + j - taps / 2][c], zero outside the row's sequence
__attribute__((weak)) int sat_launch_im2col_rows_f32(const float* a, float* out, int b, int s_len, int k, int taps, hipStream_t s);
int sat_launch_attention_hdw_f16(const void* q, const void* k, const void* vt, void* out, int b, int h, int kvh, int head_dim, int sq, int sk,
                                 int sq_pad, int sk_pad, hipStream_t s);
int sat_launch_head_split_hdw_f16(const float* x, const void* heads_epi, int head_dim, int b, hipStream_t s);
int sat_launch_attention_causal_f16(const void* q, const void* k, const void* vt, void* out, int b, int h, int kvh, int s_len, int sq_pad, int sk_pad,
                                    hipStream_t s, float q_scale);
int sat_launch_attention_hdw_causal_f16(const void* q, const void* k, const void* vt, void* out, int b, int h, int kvh, int head_dim, int s_len,
                                        int sq_pad, int sk_pad, hipStream_t s);
int sat_launch_attention_window_f16(const void* q, const void* k, const void* vt, void* out, int b, int h, int kvh, int s_len, int sq_pad, int sk_pad,
                                    int kernel_size, float score_scale, hipStream_t s);
int sat_launch_attention_hdw_window_f16(const void* q, const void* k, const void* vt, void* out, int b, int h, int kvh, int head_dim, int s_len,
                                        int sq_pad, int sk_pad, int kernel_size, hipStream_t s);
// entry points of the fp16 build for the dispatchers of the bf16 build (GemmArgs is layout-identical in both builds: the pointer
// element type is the only difference)
int sat_launch_gemm_f16(int epi, const void* gemm_args, hipStream_t stream);
int sat_launch_attention_f16(const void* q, const void* k, const void* vt, void* out, int b, int h, int kvh, int sq, int sk, int sq_pad,
                             int sk_pad, hipStream_t s, unsigned char* out_scales, float q_scale);

// f16 (last argument of the launchers below): the 16-bit output is IEEE fp16 (saturating) instead of bf16
int sat_launch_layernorm(const float* x, const float* gamma, const float* beta, op_t* y, int m, int d, hipStream_t s, int f16 = 0);
// adaLN: y = LN(x) * scale1p[b] + shift[b] with b = row / rows_per_seq and per-sequence vectors ld apart (transformer.py:671-672)
int sat_launch_layernorm_mod(const float* x, const float* gamma, const float* beta, op_t* y, int m, int d, const float* scale1p,
                             const float* shift, int rows_per_seq, int ld, hipStream_t s, int f16 = 0);
// LayerNorm (+ optional adaLN modulation) quantised per row to fp8 e4m3: y8 = rne(r / s), s = amax(r) / 448 -> row_scale[m]
int sat_launch_layernorm_fp8(const float* x, const float* gamma, const float* beta, void* y8, float* row_scale, int m, int d,
                             const float* scale1p, const float* shift, int rows_per_seq, int ld, hipStream_t s);
// rows of an fp32 matrix -> fp8 e4m3 with one scale per row (weights: per output channel; optional SwiGLU interleave)
int sat_launch_quant_rows_fp8(const float* w, void* out8, float* row_scale, int n, int k, int swiglu_interleave, hipStream_t s);
int sat_launch_quant_mx_rows(const float* x, void* out8, void* scales_e8m0, int rows, int k, hipStream_t s);
// fp32 verification path (f32_ref.hip)
int sat_launch_gemm_f32(const float* A, const float* W, const float* bias, float* C, int M, int N, int K, int ldc, int accumulate,
                        const float* gate, int gate_rows, int gate_ld, hipStream_t s);
int sat_launch_layernorm_f32(const float* x, const float* gamma, const float* beta, float* y, int m, int d, const float* sc,
                             const float* sh, int rps, int ld, hipStream_t s, float eps = 1e-5f);
int sat_launch_split_heads_f32(const float* src, float* d0, float* d1, float* d2, int M, int S, int parts, int H, int rope_mask,
                               const float* rope_cos, const float* rope_sin, hipStream_t s, int norm_mask = 0);      // norm_mask: parts L2-normalised per head (qk_norm)
int sat_launch_swiglu_f32(const float* hg, float* h, int64_t M, int inner, hipStream_t s);
int sat_launch_attention_f32(const float* q, const float* k, const float* v, float* out, int b, int h, int kvh, int sq, int sk,
                             hipStream_t s);
// the two kernels above for any built head width (32, 64, 96): head_dim channels per head, rotation tables [S][sat_rope_pairs(head_dim)], scores
// scaled by 1 / sqrt(head_dim).  WEAK as the staged-route launchers: the host test driver of the 64-channel routes does not define them
__attribute__((weak)) int sat_launch_split_heads_f32_w(const float* src, float* d0, float* d1, float* d2, int M, int S, int parts, int H, int head_dim,
                                                       int rope_mask, const float* rope_cos, const float* rope_sin, hipStream_t s, int norm_mask = 0);
__attribute__((weak)) int sat_launch_attention_f32_w(const float* q, const float* k, const float* v, float* out, int b, int h, int kvh, int head_dim,
                                                     int sq, int sk, hipStream_t s);
// causal self-attention in fp32 for head_dim 32 / 64 / 96 (sq == sk == s_len).  WEAK as above
__attribute__((weak)) int sat_launch_attention_f32_causal(const float* q, const float* k, const float* v, float* out, int b, int h, int kvh, int head_dim,
                                                          int s_len, hipStream_t s);
// neighbourhood self-attention in fp32, 64-channel heads; the scores are multiplied by score_scale (the plan passes 1).  WEAK as above
__attribute__((weak)) int sat_launch_attention_f32_window(const float* q, const float* k, const float* v, float* out, int b, int h, int kvh, int s_len,
                                                          int kernel_size, float score_scale, hipStream_t s);
// the same for head_dim 32 / 96 (attention_hdw_window.hip).  WEAK as above
__attribute__((weak)) int sat_launch_attention_f32_window_w(const float* q, const float* k, const float* v, float* out, int b, int h, int kvh,
                                                            int head_dim, int s_len, int kernel_size, float score_scale, hipStream_t s);
int sat_launch_cast_bf16(const float* x, op_t* y, int64_t n, hipStream_t s, int f16 = 0);
int sat_launch_pack_rows_bf16(const float* w, op_t* out, int n, int k, int swiglu_interleave, hipStream_t s, int f16 = 0);
int sat_launch_pack_bias(const float* b, float* out, int n, int swiglu_interleave, hipStream_t s);
// weights of a GEMM that absorbs the LayerNorm in front of it: out = bf16(gamma (.) w) (rows permuted like pack_rows),
// c1[n] = sum_k float(out[n][k]), c2[n] = sum_k beta[k] w[n][k] (+ bias[n])
int sat_launch_pack_rows_ln(const float* w, const float* gamma, const float* beta, const float* bias, op_t* out, float* c1, float* c2,
                            int n, int k, int swiglu_interleave, hipStream_t s, int f16 = 0);
int sat_launch_rope_table(const float* inv_freq, float* cos_t, float* sin_t, int s_len, hipStream_t s);
// ---- the audio boundary of the local-attention codec (local_attn_io.hip), fp32 in every build: x [b, c_in, t] channel-first through the bias-free
// w [d, c_in] into rows [b * t, d] (d % 4 == 0, c_in <= 128: a tile of the input is staged in LDS); rows [b * t, d] through the bias-free
// w [c_out, d] into out [b, c_out, t] channel-first (d % 64 == 0)
int sat_launch_local_attn_project_in(const float* x, const float* w, float* rows, int b, int c_in, int t, int d, hipStream_t s);
int sat_launch_local_attn_project_out(const float* rows, const float* w, float* out, int b, int c_out, int t, int d, hipStream_t s);
// ---- the Dance Diffusion U-Net (unet_kernels.hip), fp32 inside in every format; fmt (SAT_GEMM_BF16 / SAT_GEMM_FP16 / SAT_GEMM_FP32X) is the
// element type of the operand image a kernel leaves for the next convolution (fp32 in the verification mode).  Rows are [b * rows, c].
int sat_unet_gn_tiles(int64_t n);      // partials per item of n elements: part holds [b][tiles][2] floats
// GroupNorm(1, c) statistics of b items of n contiguous floats: stats [b][2] = (mean, 1 / sqrt(biased variance + eps)).  No atomics
int sat_launch_unet_gn_stats(const float* x, float* part, float* stats, int b, int64_t n, float eps, hipStream_t s);
// y = act((x - mean) rstd gamma + beta) (+ skip), act 1 = GELU (erf); y -> out32 [b * rows, c] and / or out_op [b * rows, ld]; out32 may alias x or skip
int sat_launch_unet_gn_apply(const float* x, const float* stats, const float* gamma, const float* beta, const float* skip, float* out32, void* out_op, int b,
                             int rows, int c, int ld, int act, int fmt, hipStream_t s);
int sat_launch_unet_cast_rows(const float* x, void* out, int64_t m, int c, int ld, int fmt, hipStream_t s);      // out [m, ld][:, :c] = x [m, c]
// Downsample1d("cubic") / Upsample1d("cubic") of blocks.py on rows, reflect indices computed in the kernel: [b * s_len, c] -> [b * s_len / 2, c]
// (fp32 and / or operand image) and [b * s_len, c] -> out [b * 2 s_len, ld] (operand image: the first half of the parent level's concat buffer)
int sat_launch_unet_downsample(const float* x, float* out32, void* out_op, int b, int s_len, int c, int fmt, hipStream_t s);
int sat_launch_unet_upsample(const float* x, void* out, int b, int s_len, int c, int ld, int fmt, hipStream_t s);
// x [b, io, t] * in_scale and the 16 timestep planes through w_main [c, io + 16, taps] (+ b_main) -> y [b * t, c] and w_skip [c, io + 16] -> sk
int sat_launch_unet_input(const float* x, const float* tval, float in_scale, const float* w_embed, const float* w_main, const float* b_main,
                          const float* w_skip, float* y, float* sk, int b, int io, int t, int c, int taps, hipStream_t s);
// out [b, io, t] = conv(h [b * t, c], w_main [io, c, taps]) + b_main + xin [b * t, c] w_skip [io, c]^T
int sat_launch_unet_output(const float* h, const float* xin, const float* w_main, const float* b_main, const float* w_skip, float* out, int b, int io, int t,
                           int c, int taps, hipStream_t s);
