// What the host decides for a DiT GEMM before anything is launched: the fields of GemmArgs::variant, the tile configurations, and
// the rule that picks one (sat_gemm_route).  Pure integer / flag logic in plain C++17 without a HIP header, no allocation and no
// state, so tests/test_gemm_host.py runs it on the CPU against tests/golden/gemm_routes.json; gemm_bf16.hip and gemm_ph8.hip only
// turn its answer into a template instantiation.
#pragma once
#include <stdint.h>

#include "ph8_sched.h"

static inline int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }
static inline int cdiv(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

// ---------------------------------------------------------------------------------------------------------------------------------
// GemmArgs::variant (and the `variant` argument of the unit-level C ABI: sat_gemm_bf16_f32 and friends).  The layout is ABI: tests
// and tools/*.py pass these numbers.  "exp" = read in the experiments build only (make -C csrc exp), ignored by the shipped one.
// Bits 12, 13, 15, 18, 19, 22 are unassigned and not read (retired variants: profiles/HISTORY.md names them, so they are not reused).
//   bits  0-7   SAT_VARIANT_TILE        forced tile id, 0 = let sat_gemm_route choose                    sat_gemm_route
//   bits  0-11  SAT_VARIANT_CODE        read as a decimal number: code % 100 = 80 / 81 forces the 8-phase kernel (81 was its retired
//                                       128 x 128 geometry and runs 80), code / 100 = 9: its timestamp build (exp)   sat_gemm_route
//   bit   8     SAT_VARIANT_FP8_PLAIN   sat_gemm_fp8_f32 only, stripped there: plain fp8 MFMA (GemmArgs::fp8 = 1) instead of the
//                                       2x-rate block-scaled one (2)                                      unit_entry.hip
//   bit  14     SAT_VARIANT_PACKED      unit-level SwiGLU / LayerNorm-fold entry points only, stripped there: the packed operands
//                                       are those of a previous call (benchmarks)                         unit_entry.hip
//   bit  16     SAT_VARIANT_SPLIT_FORCE     8-phase: cut the remainder round along K whatever the policy says (tests)
//   bit  17     SAT_VARIANT_SPLIT_OFF       8-phase: never                                                launch_ph8, sat_gemm_f32_workspace_bytes
//   bit  21     SAT_VARIANT_BALANCE_OFF     8-phase: no balanced rounds (A/B)                             launch_ph8
//   bit  23     SAT_VARIANT_NO_KGROUP   never the two-K-group 128 x 128 tile (49)                         sat_gemm_route
//   bit  27     SAT_VARIANT_HALF_ROWS_OFF   8-phase, 16-bit SwiGLU: no half-row schedule (ph8_half_rows_ints), i.e. the balanced
//                                       rounds it replaced (A/B, and the bit-equality test of the two)   launch_ph8
//   bits 24-26  tile policy (sat_tile_policy_bits / sat_wide_tile_of): sat_dit_cfg.tile_policy puts them there for every GEMM of a
//               plan; the unit-level entry points leave them 0                                            sat_gemm_route
// ---------------------------------------------------------------------------------------------------------------------------------
enum {
    SAT_VARIANT_TILE = 0xff,
    SAT_VARIANT_CODE = 0xfff,
    SAT_VARIANT_FP8_PLAIN = 0x100,
    SAT_VARIANT_PACKED = 0x4000,
    SAT_VARIANT_SPLIT_FORCE = 0x10000,
    SAT_VARIANT_SPLIT_OFF = 0x20000,
    SAT_VARIANT_BALANCE_OFF = 0x200000,
    SAT_VARIANT_NO_KGROUP = 0x800000,
    SAT_VARIANT_HALF_ROWS_OFF = 0x8000000,
};
static inline int sat_variant_tile(int variant) { return variant & SAT_VARIANT_TILE; }
static inline int sat_variant_ph8_code(int variant) { return (variant & SAT_VARIANT_CODE) % 100; }          // 80 / 81: the 8-phase kernel is forced
static inline int sat_variant_ablation(int variant) { return (variant & SAT_VARIANT_CODE) / 100; }
static inline bool sat_variant_has(int variant, int bit) { return (variant & bit) != 0; }
// bits 16 / 17 -> the `split` argument of ph8_schedule_ints
static inline int sat_variant_split(int variant) { return sat_variant_has(variant, SAT_VARIANT_SPLIT_FORCE) ? 1 : sat_variant_has(variant, SAT_VARIANT_SPLIT_OFF) ? 0 : -1; }

// Tile policy of a launch.  0 = the default (80); the others are A/B measurement switches:
//   22: the 16-wave 2-stage 256 x 256 tile of rounds 1-2 instead of the 8-phase kernel
//   81: the 8-phase kernel also for the fp32-output GEMMs with K < 4096        82: no two-K-group 128 x 128 tile
#define SAT_TILE_POLICY_SHIFT 24
static inline int sat_tile_policy_bits(int policy) { return (policy == 22 ? 1 : policy == 81 ? 2 : policy == 82 ? 3 : 0) << SAT_TILE_POLICY_SHIFT; }
static inline int sat_wide_tile_of(int variant) {
    const int p = (variant >> SAT_TILE_POLICY_SHIFT) & 7;
    return p == 1 ? 22 : p == 2 ? 81 : p == 3 ? 82 : 80;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Tiles.  The ids are the numbers of round 1 and part of the ABI.  Reserved, never to be reused (retired experiments that the files
// under profiles/ name by number): 2, 3, 7, 10, 12, 13, 39, 41-43, 45-48, 54-56, 60.
// ---------------------------------------------------------------------------------------------------------------------------------
enum SatGemmFamily {
    SAT_GEMM_NONE = 0,
    SAT_GEMM_REG,            // gemm_kernel: register-staged double buffer
    SAT_GEMM_DMA2,           // gemm_glds_kernel: LDS-DMA double buffer
    SAT_GEMM_PIPE,           // gemm_pipe_kernel: NS-stage LDS-DMA ring
    SAT_GEMM_PH8,            // gemm_ph8_kernel (gemm_ph8.hip): 8 waves, 8 phases, persistent workgroups
};
enum SatTileId {
    SAT_TILE_AUTO = 0,
    SAT_TILE_REF_128 = 1,          // 128x128, 4 waves, register-staged: the reference tile; tiny per-generation GEMMs (cross-attention to_kv)
    SAT_TILE_DMA_128 = 5,          // 128x128, 4 waves, LDS-DMA double buffer: K < 192, too short for a 3-stage ring
    SAT_TILE_128 = 15,             // 128x128x64, 8 waves, 3-stage ring: to_out at 1 prompt where tile 49 does not apply
    SAT_TILE_128x64 = 16,          // 128x64x64, 4 waves (one per SIMD), 3-stage ring, LDS-DMA pieces in the MFMA stream (15.1 vs 16.2 us,
                                   // cross to_out): cross-attention projections, M = 1025.  The e4m3 builds issue the pieces in front.
    SAT_TILE_256 = 22,             // 256x256x64, 16 waves, 2-stage ring: tile policy 22 and e4m3 flavours 1 / 3; the automatic choice of
                                   // 256x256 is the 8-phase kernel wherever sat_ph8_applies.  (The 4-stage BK = 32 variant with cross-tile
                                   // fragment prefetch and grouped raster of round 1 measured within 2 % of it at 8 prompts after the
                                   // epilogue rewrite -- profiles/r02_b8_tiles.txt -- and was removed)
    SAT_TILE_256x192 = 30,         // 256x192x64, 12 waves, 2-stage ring: to_qkv at 1 prompt
    SAT_TILE_128_DEEP = 44,        // tile 15 with a 4-stage ring, fp32 output only: K >= 4096 (FF-out at 1 prompt)
    SAT_TILE_128_KGROUP = 49,      // 128x128 on two K-groups of 2 x 2 waves (64 x 64 each), 2 x 64 k per stage, 2 stages, fp32 output only:
                                   // one round of 128x128 tiles (to_out / FF-out at 1 prompt)
    SAT_TILE_PH8 = 80,             // 256x256x64, 8 waves, 8-phase schedule: FF-in always, every wide GEMM from 4 prompts on
    SAT_TILE_128x64_XATTN = 256,   // tile 16 with the pieces in front of the loop body and the fused cross-attention epilogue (heads
                                   // epilogue only).  Not a value of the tile field: chosen by GemmArgs::heads.xa_k alone
};

struct SatTile {
    int family;
    int bm, bn, bk;          // (bk: ring tiles only)
    int wm, wn;              // waves along M / N
    int ns, kg;              // ring stages, K-groups
    bool dil;                // LDS-DMA pieces in the MFMA stream (16-bit operands; the e4m3 builds of a tile never interleave)
    bool f32_only;           // built for the fp32-output epilogue only
};
constexpr SatTile sat_tile_geom(int id) {
    switch (id) {
        case SAT_TILE_REF_128: return {SAT_GEMM_REG, 128, 128, 64, 2, 2, 2, 1, false, false};
        case SAT_TILE_DMA_128: return {SAT_GEMM_DMA2, 128, 128, 64, 2, 2, 2, 1, false, false};
        case SAT_TILE_128: return {SAT_GEMM_PIPE, 128, 128, 64, 4, 2, 3, 1, false, false};
        case SAT_TILE_128x64: return {SAT_GEMM_PIPE, 128, 64, 64, 4, 1, 3, 1, true, false};
        case SAT_TILE_128x64_XATTN: return {SAT_GEMM_PIPE, 128, 64, 64, 4, 1, 3, 1, false, false};
        case SAT_TILE_256: return {SAT_GEMM_PIPE, 256, 256, 64, 4, 4, 2, 1, false, false};
        case SAT_TILE_256x192: return {SAT_GEMM_PIPE, 256, 192, 64, 4, 3, 2, 1, false, false};
        case SAT_TILE_128_DEEP: return {SAT_GEMM_PIPE, 128, 128, 64, 4, 2, 4, 1, false, true};
        case SAT_TILE_128_KGROUP: return {SAT_GEMM_PIPE, 128, 128, 64, 2, 2, 2, 2, false, true};
        case SAT_TILE_PH8: return {SAT_GEMM_PH8, 256, 256, 64, 2, 4, 2, 1, false, false};
        default: return {SAT_GEMM_NONE, 0, 0, 0, 0, 0, 0, 0, false, false};
    }
}

// The builds of the 8-phase kernel (template arguments of gemm_ph8_kernel behind the epilogue)
enum SatPh8Build {
    SAT_PH8_PLAIN = 0,
    SAT_PH8_GATED,           // fp32 output with the adaLN gate
    SAT_PH8_E4M3,            // e4m3 operands on the block-scaled MFMA (SwiGLU / heads; bf16 build of the library only)
    SAT_PH8_TIMESTAMPS,      // experiments build only: ablation code 9
};
struct SatPh8Params {
    int dbg, fp8;
    bool gated;
};
constexpr SatPh8Params sat_ph8_params(int build) {
    switch (build) {
        case SAT_PH8_GATED: return {0, 0, true};
        case SAT_PH8_E4M3: return {0, 2, false};
        case SAT_PH8_TIMESTAMPS: return {9, 0, false};
        default: return {0, 0, false};
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The choice
// ---------------------------------------------------------------------------------------------------------------------------------
enum { EPI_F32 = 0, EPI_RESID = 1, EPI_SWIGLU = 2, EPI_HEADS = 3 };
// Template argument only, never a caller's `epi` (sat_gemm_route answers for EPI_HEADS): the heads epilogue built with the per-head L2
// normalisation of qk_norm (HeadsEpi::kind bit 4).  A separate instantiation so that the default heads kernels keep their code and registers.
enum { EPI_HEADS_QKN = 4 };
// A caller's `epi`, routed as EPI_SWIGLU on the ring tiles (the 8-phase kernel has no such build): H [M, N] (16-bit) = act(acc + bias), every
// column of the wave tile an output -- GemmArgs::act 0 the identity (the conformer's pointwise_conv), 1 SiLU (ff_kwargs glu=False,
// transformer.py:262-268).  Built as a separate instantiation of the SwiGLU kernels, as EPI_HEADS_QKN is of the heads kernels.
enum { EPI_ACT16 = 5 };

struct GemmShape {          // what the rule reads of a GemmArgs, the build and the device
    int M, N, K;
    int variant;
    int fp8;                 // GemmArgs::fp8: 0 = 16-bit operands, 1 plain fp8 MFMA, 2 block-scaled MFMA with unit scales, 3 MXFP8 A operand
    bool h8;                 // MXFP8 output of the SwiGLU epilogue (GemmArgs::H8)
    bool ln_part;            // consumer of the LayerNorm fold
    bool gate;               // adaLN gate
    int heads;               // heads.heads (heads epilogue)
    bool xattn;              // heads.xa_k: fused cross-attention
    bool slab_ok;            // GemmArgs::slab holds one accumulator image (65536 floats) per compute unit
    bool e4m3_built;         // this build of the library has the e4m3 instantiations (the fp16 build has none)
};
enum SatRouteMsg {
    SAT_ROUTE_OK = 0,
    SAT_ROUTE_UNKNOWN_EPI,         // SAT_E_INVALID      "gemm: unknown epilogue %d"
    SAT_ROUTE_XATTN_OPERANDS,      // SAT_E_UNSUPPORTED  "gemm: fused cross-attention needs bf16 operands and K >= 192"
    SAT_ROUTE_NO_E4M3_TILE,        // SAT_E_INVALID      "gemm(fp8): variant %d has no e4m3 build (15, 16, 22, 30)"
    SAT_ROUTE_UNKNOWN_TILE,        // SAT_E_INVALID      "gemm: unknown variant %d (or not built for this epilogue)"
    SAT_ROUTE_PH8_NOT_BUILT,       // SAT_E_UNSUPPORTED  "gemm(8-phase): epilogue %d / ablation %d not built"
};
struct GemmRoute {
    int msg;                 // SatRouteMsg; the fields below hold the message's arguments when it is not SAT_ROUTE_OK
    int family;              // SatGemmFamily
    int tile;                // SatTileId (message argument: the offending tile / the ablation code)
    int e4m3;                // ring tiles: the e4m3 flavour of the build (0: 16-bit operands, else GemmShape::fp8)
    int ph8;                 // SAT_GEMM_PH8: SatPh8Build
    bool splits;             // SAT_GEMM_PH8 chosen by the rule: its automatic schedule cuts the remainder round along K
};

#ifdef SAT_GEMM_EXPERIMENTS
constexpr bool SAT_GEMM_EXP = true;
#else
constexpr bool SAT_GEMM_EXP = false;
#endif

// Whether the automatic choice of the 256 x 256 tile is the 8-phase kernel (a forced code 80 always is)
inline bool sat_ph8_applies(int epi, const GemmShape& s) {
    if (s.N % 256 || s.K % 128 || (uint64_t)s.M * (uint64_t)s.K * 2u >= (1ull << 31)) return false;
    if (s.fp8 || s.h8) {      // e4m3: the LayerNorm-fed GEMMs (to_qkv, cross to_q, FF-in) with per-token scales
        if (s.fp8 != 2 || s.K % 256 || s.ln_part || !(epi == EPI_SWIGLU || epi == EPI_HEADS) || (s.h8 && epi != EPI_SWIGLU)) return false;
    }
    // fp32-output GEMMs with a short reduction (to_out, cross to_out: K = 1536) spend a third of their time in the residual
    // read-modify-write at HBM speed; persistent workgroups run those epilogues in lockstep, the 16-wave tile's independent workgroups
    // drift apart and overlap them with other tiles' main loops: measured 111 us against 122 at 8 prompts (profiles/r03_ph8_streamk.txt)
    if ((epi == EPI_F32 || epi == EPI_RESID) && s.K < 4096 && sat_wide_tile_of(s.variant) != 81) return false;          // (81: sat_dit_cfg.tile_policy, A/B)
    if (epi == EPI_HEADS) return (s.heads * 64) % 256 == 0;
    return true;
}

// which build of the 8-phase kernel a launch that goes there runs
inline GemmRoute sat_ph8_route(int epi, const GemmShape& s) {
    GemmRoute r{SAT_ROUTE_OK, SAT_GEMM_PH8, SAT_TILE_PH8, 0, SAT_PH8_PLAIN, false};
    const int dbg = sat_variant_ablation(s.variant);
    const bool f32 = epi == EPI_F32 || epi == EPI_RESID, swiglu = epi == EPI_SWIGLU, heads = epi == EPI_HEADS;
    if (dbg == 0 && (f32 || swiglu || heads)) {
        if (f32) r.ph8 = s.gate ? SAT_PH8_GATED : SAT_PH8_PLAIN;
        else r.ph8 = (s.e4m3_built && s.fp8) ? SAT_PH8_E4M3 : SAT_PH8_PLAIN;
        return r;
    }
    if (SAT_GEMM_EXP && dbg == 9 && (f32 || swiglu || heads)) r.ph8 = SAT_PH8_TIMESTAMPS;
    else {
        r.msg = SAT_ROUTE_PH8_NOT_BUILT;
        r.tile = dbg;
    }
    return r;
}

// Which kernel runs a GEMM on a device of `cus` compute units.  Tile choice = argmax over the tiles of
//     (fill of the last round of the device's CUs) x (measured in-kernel rate of the tile, relative to the 256 x 256 tile),
// then the overrides below.  At 1 prompt (M = 2050) this gives FF-in 256x256 (432 workgroups, 2 rounds), to_qkv 256x192 (216 instead
// of 162 workgroups), to_out / FF-out 128x128 (204) and the cross-attention projections (M = 1025) 128x64 (216); from 4 prompts on
// everything takes the 256x256 tile.
inline GemmRoute sat_gemm_route(int epi, const GemmShape& s, int cus_) {
    const long cus = cus_ > 1 ? cus_ : 1;
    const bool f32 = epi == EPI_F32 || epi == EPI_RESID;
    GemmRoute r{SAT_ROUTE_OK, SAT_GEMM_NONE, 0, 0, SAT_PH8_PLAIN, false};
    auto fail = [&](int msg, int arg) {
        r.msg = msg;
        r.tile = arg;
        return r;
    };
    auto tile = [&](int id) {
        r.family = sat_tile_geom(id).family;
        r.tile = id;
        return r;
    };
    // the 8-phase kernel takes the launch when the variant forces it, or when the rule below picked the 256 x 256 tile by itself,
    // the tile policy allows it and the kernel has this (epilogue, operand format, shape): THE one statement of that route
    const bool ph8_allowed = sat_wide_tile_of(s.variant) >= 80 && sat_ph8_applies(epi, s);
    const int forced = sat_variant_tile(s.variant);
    if (sat_variant_ph8_code(s.variant) == 80 || sat_variant_ph8_code(s.variant) == 81) return sat_ph8_route(epi, s);
    if (!(f32 || epi == EPI_SWIGLU || epi == EPI_HEADS)) return fail(SAT_ROUTE_UNKNOWN_EPI, epi);
    if (epi == EPI_HEADS && s.xattn) {       // fused cross-attention: built into the 128 x 64 tile only (the caller asks for it where that tile is the choice)
        if (s.fp8 || s.K < 192) return fail(SAT_ROUTE_XATTN_OPERANDS, 0);
        return tile(SAT_TILE_128x64_XATTN);
    }
    auto score = [&](int bm, int bn, double rate) {
        if (s.N % bn) return 0.0;
        long t = (long)cdiv(s.M, bm) * (s.N / bn);
        return rate * (double)t / (double)(((t + cus - 1) / cus) * cus);
    };
    const bool e4m3 = s.fp8 && s.e4m3_built;          // (e4m3 operands ride in the bf16 build: sat_launch_gemm rejects f16 && fp8)
    int v = forced;
    if (v == SAT_TILE_AUTO && (e4m3 || s.K >= 192)) {
        double s256 = score(256, 256, 1.0);
        if (!e4m3 && ph8_allowed) {
            // The 256 x 256 tile is the 8-phase kernel where it applies; its rate relative to the 16-wave tile, measured at 8 prompts
            // (profiles/r03_ph8_streamk.txt): SwiGLU 1.26, heads 1.07, fp32 output with a long reduction 1.02 -- and with the K-split of the
            // remainder round (ph8_auto_split) the last round costs ~0.35 of a round instead of 1.
            const double rate = epi == EPI_SWIGLU ? 1.26 : epi == EPI_HEADS ? 1.07 : 1.02;
            const long t = (long)cdiv(s.M, 256) * (s.N / 256);
            r.splits = s.slab_ok && ph8_auto_split(s.M, s.N, s.K, f32, (int)cus);
            const double rounds = r.splits ? (double)(t / cus) + 0.35 : (double)((t + cus - 1) / cus);
            s256 = rate * (double)t / (rounds * (double)cus);
        }
        const double s192 = score(256, 192, 0.95), s128 = score(128, 128, 0.7), s64 = score(128, 64, 0.6);
        const double best = s256 > s192 ? (s256 > s128 ? s256 : s128) : (s192 > s128 ? s192 : s128);
        if (best == 0.0 && s64 == 0.0 && !e4m3) v = SAT_TILE_128;      // N is not a tile multiple: let the launcher report it
        else if (s64 > best) v = SAT_TILE_128x64;
        else if (best == s256) v = SAT_TILE_256;
        else if (best == s192) v = SAT_TILE_256x192;
        else v = SAT_TILE_128;
        if (e4m3) {
            if (s.K < 384 && (v == SAT_TILE_128 || v == SAT_TILE_128x64)) v = SAT_TILE_256;     // the 3-stage tiles need K >= 384 bytes
        } else {
            // long reductions (FF-out: 96 K-tiles) gain 4 % from a fourth ring stage (prefetch distance 3); K = 1536 does not care
            if (v == SAT_TILE_128 && f32 && s.K >= 4096) v = SAT_TILE_128_DEEP;
            // one round of 128 x 128 tiles (to_out / FF-out at one prompt: 204 workgroups on 256 CUs): the two-K-group build puts 8 waves of
            // 64 x 64 on every CU instead of 8 waves of 32 x 64 -- FF-out 56.5 us against 60.7, to_out 20.6 against 21.4 (tools/ph8_probe.py narrow)
            if ((v == SAT_TILE_128 || v == SAT_TILE_128_DEEP) && f32 && !s.fp8 && s.K % 128 == 0 && s.K >= 256 &&
                (long)cdiv(s.M, 128) * (s.N / 128) <= cus && !sat_variant_has(s.variant, SAT_VARIANT_NO_KGROUP) && sat_wide_tile_of(s.variant) != 82)
                v = SAT_TILE_128_KGROUP;
        }
    } else if (v == SAT_TILE_AUTO) {
        v = SAT_TILE_DMA_128;
    }
    // (tile policy 22, sat_dit_cfg.tile_policy, brings the 16-wave 2-stage tile back for A/B measurements; e4m3 operands reach the
    // 8-phase kernel in the block-scaled flavour only)
    if (forced == SAT_TILE_AUTO && v == SAT_TILE_256 && ph8_allowed && (!e4m3 || s.fp8 == 2)) {
        const bool splits = r.splits;
        r = sat_ph8_route(epi, s);
        r.splits = splits;
        return r;
    }
    r.splits = false;
    const SatTile g = sat_tile_geom(v);
    if (e4m3) {
        r.e4m3 = s.fp8;
        const bool built = v == SAT_TILE_128 || v == SAT_TILE_128x64 || v == SAT_TILE_256 || v == SAT_TILE_256x192;
        if (!built || (s.fp8 == 3 && !f32)) return fail(SAT_ROUTE_NO_E4M3_TILE, v);          // MXFP8 A operand (hardware block scales): fp32 output only (FF-out, to_out)
        return tile(v);
    }
    if (g.family == SAT_GEMM_NONE || g.family == SAT_GEMM_PH8 || v == SAT_TILE_128x64_XATTN || (g.f32_only && !f32)) return fail(SAT_ROUTE_UNKNOWN_TILE, v);
    return tile(v);
}
