// What oobleck.hip (the codec's kernels and their launchers, built once per operand format: bf16, fp16, fp32) and oobleck_plan.hip (the plan,
// host code, built once) share: the argument blocks of the convolution kernels and the table of launchers each build exports to the plan.
#pragma once
#include <stddef.h>

#include "sat_common.h"

enum { ACT_SNAKE = SAT_OOBLECK_ACT_SNAKE, ACT_ELU = SAT_OOBLECK_ACT_ELU, ACT_RUNTIME = -1 };

static inline int pad64(int c) { return (int)round_up(c, 64); }

// The layout is the same in every build: the element type of the operand pointers is the only difference (as GemmArgs, sat_common.h).
// oobleck_plan.hip sees op_t = bf16 and treats operand buffers as opaque storage of OobKernels::elem_bytes per element.
namespace SAT_OPNS {

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
    float* out_cf;           // channel-first fp32 output [B][cf_channels][M] (final convs) or null; with cf_channels == 0: the un-activated
    int cf_channels;         // result in fp32, channels-last and indexed as out_raw (the input of an anti-aliased activation)
    const op_t* zero_page; // >= one K-tile row (ROW_B <= 256 B) of zeros: LDS-DMA source of the rows that fall into the conv padding
    // (the option fields come last: the fields above keep the offsets they had before the options existed)
    int act;                 // activation behind out_snk: ACT_SNAKE (sn_a / sn_ib) or ACT_ELU (no parameters)
    int tanh_out;            // out_cf only: tanh on the result (OobleckDecoder final_tanh)
};

// one ResidualUnit in one launch (ru_fused_kernel; the 16-bit builds)
struct RuArgs {
    ConvArgs c7;     // in = snake1(x); bias / sn_a / sn_ib: those of the k = 7 convolution and of the Snake behind it
    ConvArgs c1;     // W / bias of the 1 x 1 convolution, res = raw x, out_raw / out_snk (+ the next layer's Snake)
};

static_assert(sizeof(ConvArgs) == 160 && sizeof(RuArgs) == 320, "ConvArgs is a kernel argument: its layout is fixed");
static_assert(offsetof(ConvArgs, W) == 16 && offsetof(ConvArgs, bias) == 48 && offsetof(ConvArgs, res) == 64 &&
                  offsetof(ConvArgs, out_bstride) == 104 && offsetof(ConvArgs, out_cf) == 128 && offsetof(ConvArgs, zero_page) == 144 &&
                  offsetof(ConvArgs, act) == 152 && offsetof(ConvArgs, tanh_out) == 156,
              "ConvArgs is a kernel argument: its layout is fixed");

}  // namespace SAT_OPNS

// The launchers of one build.  conv_args / ru_args point to that build's ConvArgs / RuArgs; operand buffers are void*.
struct OobKernels {
    int elem_bytes;      // of one operand element: activations, packed weights, the zero page
    int dtype;           // SAT_GEMM_BF16 / SAT_GEMM_FP16 / SAT_GEMM_FP32X
    int (*conv)(const void* conv_args, int B, hipStream_t s);
    int (*ru_fused)(const void* ru_args, int B, hipStream_t s);      // c7.N = 128 or 256 channels; null in the fp32 build: two launches
    int (*cf_to_cl)(const float* z, void* y, int C, int T, int B, hipStream_t s);
    // the encoder's first convolution (VALU): C channels out of Cin <= 2, raw and activated rows of pad64(C) channels
    int (*first_conv)(const float* audio, const float* w_f32, const float* bias, const float* sn_a, const float* sn_ib, int act, void* raw,
                      void* snk, int Cin, int C, int L, int B, hipStream_t s);
    // finalize: weight norm folded (scale: scratch of one float per slice of v), then the re-packing of each weight kind
    int (*pack_conv)(const float* v, const float* g, float* scale, void* W, int Cout, int Cin, int k, int Npad, int Kpad, hipStream_t s);
    int (*fold_f32)(const float* v, const float* g, float* scale, float* w, int Cout, int slice, hipStream_t s);
    int (*pack_convT)(const float* v, const float* g, float* scale, void* W, int Cin, int Cout, int stride, int Kp, int Np, hipStream_t s);
    int (*pack_nearest)(const float* v, const float* g, float* scale, void* W, int Cin, int Cout, int stride, int Kp, int Np, hipStream_t s);
    int (*snake_params)(const float* alpha, const float* beta, float* a, float* ib, int C, int Cp, hipStream_t s);
    // the anti-aliased activation (alias_free_torch.Activation1d, sat_oobleck_plan_set_antialias): in [B][L][Cp] un-activated rows -> out, the
    // same shape, never in place (an output row reads 11 input rows); sn_a / sn_ib [Cp] as the convolution epilogues take them, null under ELU.
    // in_f32: the input rows are fp32 in every build (what a convolution writes through ConvArgs::out_cf with cf_channels == 0)
    int (*aa_act)(const void* in, int in_f32, void* out, const float* sn_a, const float* sn_ib, int act, int Cp, int L, int B, hipStream_t s);
};
enum { AA_TIME_TILE = SAT_OOBLECK_AA_TIME_TILE };      // output rows per thread of that kernel
namespace bf16 { const OobKernels* oob_kernels(); }
namespace f16 { const OobKernels* oob_kernels(); }
namespace f32 { const OobKernels* oob_kernels(); }
