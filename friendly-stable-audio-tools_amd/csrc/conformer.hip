// Kernels of the TransformerBlock options beyond the shipped configs (sat_dit_plan_set_block_options):
//   * the conformer's depthwise_conv -> mid_norm -> SiLU (models/transformer.py:571-573, 583-586 of the reference) in one pass;
//   * remove_norms (:621, 632, 642): the projection operand is the residual row itself, rounded (and modulated under adaLN, :672, 686);
//   * the SiLU of a feed-forward without GLU (:262-268) in the fp32 verification mode (the 16-bit modes have it in the GEMM epilogue).
// Compiled once: the 16-bit element type is a template argument, as in layernorm.hip.
#include "sat_common.h"

namespace {

template <typename T>
using Vec4 = T __attribute__((ext_vector_type(4)));      // one 8-byte (16-bit T) or 16-byte (float) access

// One workgroup = TR consecutive rows of ONE sequence x all d channels, one thread = 4 channels.  The thread loads its 4 channels of the
// TR + 16 input rows (8 rows of halo either side; rows outside the sequence are zeros, never a neighbour's) into registers once, forms the
// TR x 4 convolution sums in fp32 from them, and the workgroup reduces the LayerNorm statistics of the TR rows over d in two passes
// (mean, then centred squares) through LDS.  Every input element is read once per workgroup; the halo, (TR + 16) / TR of the rows, comes
// out of L2, where the neighbouring workgroup's read put it.
template <typename T, int TR>
__global__ __launch_bounds__(512) void dwconv_ln_silu_kernel(const T* __restrict__ x, const float* __restrict__ w, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, T* __restrict__ y, int S, int D, float eps) {
    sat_saturate_for<T>();
    __shared__ float red[2][8][TR];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
    const int c = tid * 4;
    const bool on = c < D;
    const int s0 = blockIdx.x * TR;
    const T* xb = x + (size_t)blockIdx.y * S * D;
    T* yb = y + (size_t)blockIdx.y * S * D;

    // the 4 x 17 taps of the thread's channels are 68 consecutive floats of w [d, 17], 16-byte aligned: 17 loads, and a wave reads one
    // contiguous 17 KiB span
    float wt[4][17];
#pragma unroll
    for (int i = 0; i < 17; ++i) {
        const f32x4 v = on ? reinterpret_cast<const f32x4*>(w + (size_t)c * 17)[i] : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 4; ++j) wt[(4 * i + j) / 17][(4 * i + j) % 17] = v[j];
    }
    Vec4<T> win[TR + 16];
#pragma unroll
    for (int i = 0; i < TR + 16; ++i) {
        const int s = s0 - 8 + i;
        if (on && s >= 0 && s < S) win[i] = *reinterpret_cast<const Vec4<T>*>(xb + (size_t)s * D + c);
        else win[i] = Vec4<T>{(T)0.f, (T)0.f, (T)0.f, (T)0.f};
    }
    // Conv1d is a cross-correlation: out[s] = sum_k w[k] * in[s + k - 8], and win[i] is row s0 - 8 + i
    float o[TR][4];
#pragma unroll
    for (int r = 0; r < TR; ++r)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float a = 0.f;
#pragma unroll
            for (int k = 0; k < 17; ++k) a = fmaf(wt[e][k], (float)win[r + k][e], a);
            o[r][e] = a;
        }
    // LayerNorm over d per row, fp32 statistics of the fp32 sums
#pragma unroll
    for (int r = 0; r < TR; ++r) {
        const float ps = wave_sum(o[r][0] + o[r][1] + o[r][2] + o[r][3]);          // (threads past d hold zeros)
        if (lane == 0) red[0][wave][r] = ps;
    }
    __syncthreads();
    float mean[TR];
#pragma unroll
    for (int r = 0; r < TR; ++r) {
        float t = 0.f;
        for (int v = 0; v < nw; ++v) t += red[0][v][r];
        mean[r] = t / (float)D;
        float q = 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e) q += (o[r][e] - mean[r]) * (o[r][e] - mean[r]);
        q = wave_sum(on ? q : 0.f);
        if (lane == 0) red[1][wave][r] = q;
    }
    __syncthreads();
    if (!on) return;
    const f32x4 g4 = *reinterpret_cast<const f32x4*>(gamma + c);
    const f32x4 b4 = beta ? *reinterpret_cast<const f32x4*>(beta + c) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < TR; ++r) {
        const int s = s0 + r;
        if (s >= S) continue;
        float t = 0.f;
        for (int v = 0; v < nw; ++v) t += red[1][v][r];
        const float rstd = 1.0f / sqrtf(t / (float)D + eps);
        Vec4<T> out;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float n = (o[r][e] - mean[r]) * rstd * g4[e] + b4[e];
            if constexpr (__is_same(T, float)) out[e] = n / (1.0f + expf(-n));
            else out[e] = (T)silu_f(n);
        }
        *reinterpret_cast<Vec4<T>*>(yb + (size_t)s * D + c) = out;
    }
}

// The same pass with the TR + 16 input rows staged in LDS by the whole workgroup (16-byte coalesced loads, zeros for the rows outside the
// sequence) instead of held in registers: the window is then not bounded by the register file, so TR = 32 fits (halo 1.5x instead of 2x),
// at the price of an LDS round trip per tap.  Output rows in groups of 8: 8 x 4 sums per thread, the two reductions, the store.
// A measurement variant (sat_dwconv_ln_silu_* variant 2): profiles/dit_block_options_verification.txt has the figures beside the shipped kernel's.
template <typename T, int TR>
__global__ __launch_bounds__(512) void dwconv_ln_silu_lds_kernel(const T* __restrict__ x, const float* __restrict__ w, const float* __restrict__ gamma,
                                                                 const float* __restrict__ beta, T* __restrict__ y, int S, int D, float eps) {
    static_assert(TR % 8 == 0 && sizeof(T) == 2, "groups of 8 rows, 16-bit rows");
    sat_saturate_for<T>();
    extern __shared__ __attribute__((aligned(16))) char smem[];
    T* tile = reinterpret_cast<T*>(smem);          // [TR + 16][D]
    __shared__ float red[2][8][8];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
    const int c = tid * 4;
    const bool on = c < D;
    const int s0 = blockIdx.x * TR;
    const T* xb = x + (size_t)blockIdx.y * S * D;
    T* yb = y + (size_t)blockIdx.y * S * D;
    const int d8 = D >> 3;
    for (int i = tid; i < (TR + 16) * d8; i += blockDim.x) {
        const int row = i / d8, cv = i - row * d8, s = s0 - 8 + row;
        u32x4 v = {0u, 0u, 0u, 0u};
        if (s >= 0 && s < S) v = *reinterpret_cast<const u32x4*>(xb + (size_t)s * D + cv * 8);
        *reinterpret_cast<u32x4*>(tile + (size_t)row * D + cv * 8) = v;
    }
    // the 4 x 17 taps of the thread's channels are 68 consecutive floats of w [d, 17], 16-byte aligned: 17 loads, and a wave reads one
    // contiguous 17 KiB span
    float wt[4][17];
#pragma unroll
    for (int i = 0; i < 17; ++i) {
        const f32x4 v = on ? reinterpret_cast<const f32x4*>(w + (size_t)c * 17)[i] : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 4; ++j) wt[(4 * i + j) / 17][(4 * i + j) % 17] = v[j];
    }
    const f32x4 g4 = on ? *reinterpret_cast<const f32x4*>(gamma + c) : f32x4{0.f, 0.f, 0.f, 0.f};
    const f32x4 b4 = on && beta ? *reinterpret_cast<const f32x4*>(beta + c) : f32x4{0.f, 0.f, 0.f, 0.f};
    __syncthreads();
    for (int r0 = 0; r0 < TR && s0 + r0 < S; r0 += 8) {          // (uniform over the workgroup)
        Vec4<T> win[24];
#pragma unroll
        for (int i = 0; i < 24; ++i) win[i] = on ? *reinterpret_cast<const Vec4<T>*>(tile + (size_t)(r0 + i) * D + c) : Vec4<T>{(T)0.f, (T)0.f, (T)0.f, (T)0.f};
        float o[8][4];
#pragma unroll
        for (int r = 0; r < 8; ++r)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float a = 0.f;
#pragma unroll
                for (int k = 0; k < 17; ++k) a = fmaf(wt[e][k], (float)win[r + k][e], a);
                o[r][e] = a;
            }
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const float ps = wave_sum(o[r][0] + o[r][1] + o[r][2] + o[r][3]);
            if (lane == 0) red[0][wave][r] = ps;
        }
        __syncthreads();
        float mean[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            float t = 0.f;
            for (int v = 0; v < nw; ++v) t += red[0][v][r];
            mean[r] = t / (float)D;
            float q = 0.f;
#pragma unroll
            for (int e = 0; e < 4; ++e) q += (o[r][e] - mean[r]) * (o[r][e] - mean[r]);
            q = wave_sum(on ? q : 0.f);
            if (lane == 0) red[1][wave][r] = q;
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int s = s0 + r0 + r;
            float t = 0.f;
            for (int v = 0; v < nw; ++v) t += red[1][v][r];
            const float rstd = 1.0f / sqrtf(t / (float)D + eps);
            Vec4<T> out;
#pragma unroll
            for (int e = 0; e < 4; ++e) out[e] = (T)silu_f((o[r][e] - mean[r]) * rstd * g4[e] + b4[e]);
            if (on && s < S) *reinterpret_cast<Vec4<T>*>(yb + (size_t)s * D + c) = out;
        }
    }
}

// y = x, or x * scale1p[b] + shift[b]; 4 elements per thread
template <typename T>
__global__ __launch_bounds__(256) void round_rows_kernel(const float* __restrict__ x, T* __restrict__ y, int64_t n4, int d, const float* __restrict__ sc,
                                                         const float* __restrict__ sh, int rps, int ld) {
    sat_saturate_for<T>();
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    const int64_t e = i * 4;
    f32x4 v = *reinterpret_cast<const f32x4*>(x + e);
    if (sc) {
        const int64_t row = e / d;
        const int col = (int)(e - row * d);
        const size_t off = (size_t)(row / rps) * ld + col;
        const f32x4 a = *reinterpret_cast<const f32x4*>(sc + off), b = *reinterpret_cast<const f32x4*>(sh + off);
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = v[k] * a[k] + b[k];
    }
    Vec4<T> out;
#pragma unroll
    for (int k = 0; k < 4; ++k) out[k] = (T)v[k];
    *reinterpret_cast<Vec4<T>*>(y + e) = out;
}

__global__ __launch_bounds__(256) void silu_f32_kernel(float* __restrict__ h, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float v = h[i];
    h[i] = v / (1.0f + expf(-v));
}

template <typename T, int TR>
int launch_dwconv(const void* x, const float* w, const float* gamma, const float* beta, void* y, int b, int s_len, int d, hipStream_t s) {
    const int threads = (int)round_up(d / 4, 64);
    hipLaunchKernelGGL((dwconv_ln_silu_kernel<T, TR>), dim3(cdiv(s_len, TR), b), dim3(threads), 0, s, (const T*)x, w, gamma, beta, (T*)y, s_len, d, 1e-5f);
    SAT_LAUNCH_CHECK();
    return 0;
}

template <typename T>
int launch_dwconv_lds(const void* x, const float* w, const float* gamma, const float* beta, void* y, int b, int s_len, int d, hipStream_t s) {
    constexpr int TR = 32;
    const int lds = (TR + 16) * d * 2;
    SAT_CHECK_ARG(d % 8 == 0 && lds <= 156 * 1024, SAT_E_UNSUPPORTED, "dwconv_ln_silu (LDS variant): d = %d must be a multiple of 8 and at most 1664", d);
    auto kern = dwconv_ln_silu_lds_kernel<T, TR>;
    SAT_TRY(sat_ensure_dynamic_lds(reinterpret_cast<const void*>(kern), lds));
    hipLaunchKernelGGL(kern, dim3(cdiv(s_len, TR), b), dim3((int)round_up(d / 4, 64)), lds, s, (const T*)x, w, gamma, beta, (T*)y, s_len, d, 1e-5f);
    SAT_LAUNCH_CHECK();
    return 0;
}

}  // namespace

// The measurement variants of the unit-level entry points (sat_dwconv_ln_silu_*, variant != 0); the plan runs sat_launch_dwconv_ln_silu
int sat_launch_dwconv_ln_silu_variant(const void* x, const float* w, const float* gamma, const float* beta, void* y, int b, int s_len, int d, int fmt,
                                      int variant, hipStream_t s) {
    if (variant == 0) return sat_launch_dwconv_ln_silu(x, w, gamma, beta, y, b, s_len, d, fmt, s);
    SAT_CHECK_ARG(x && w && gamma && y && b > 0 && b <= 65535 && s_len > 0 && d > 0 && d % 4 == 0 && d <= 2048, SAT_E_INVALID, "dwconv_ln_silu: bad arguments");
    SAT_CHECK_ARG((((uintptr_t)x | (uintptr_t)y | (uintptr_t)w | (uintptr_t)gamma | (uintptr_t)beta) & 15) == 0, SAT_E_INVALID, "dwconv_ln_silu: pointers must be 16-byte aligned");
    SAT_CHECK_ARG(variant >= 1 && variant <= 3 && (fmt == SAT_GEMM_BF16 || fmt == SAT_GEMM_FP16), SAT_E_UNSUPPORTED,
                  "dwconv_ln_silu: variant %d (1: one row per workgroup, 2: LDS-staged 32-row tile, 3: 8-row tile in registers) on 16-bit rows", variant);
    const bool f16 = fmt == SAT_GEMM_FP16;
    if (variant == 1)      // one output row per workgroup: all 17 rows of its window come out of L2 (or HBM), nothing is kept between rows
        return f16 ? launch_dwconv<_Float16, 1>(x, w, gamma, beta, y, b, s_len, d, s) : launch_dwconv<bf16_t, 1>(x, w, gamma, beta, y, b, s_len, d, s);
    if (variant == 3)      // the shipped design on half the tile: twice the workgroups, a 3x halo instead of 2x
        return f16 ? launch_dwconv<_Float16, 8>(x, w, gamma, beta, y, b, s_len, d, s) : launch_dwconv<bf16_t, 8>(x, w, gamma, beta, y, b, s_len, d, s);
    return f16 ? launch_dwconv_lds<_Float16>(x, w, gamma, beta, y, b, s_len, d, s) : launch_dwconv_lds<bf16_t>(x, w, gamma, beta, y, b, s_len, d, s);
}

int sat_launch_dwconv_ln_silu(const void* x, const float* w, const float* gamma, const float* beta, void* y, int b, int s_len, int d, int fmt,
                              hipStream_t s) {
    SAT_CHECK_ARG(x && w && gamma && y && b > 0 && s_len > 0, SAT_E_INVALID, "dwconv_ln_silu: bad arguments");
    SAT_CHECK_ARG(b <= 65535, SAT_E_UNSUPPORTED, "dwconv_ln_silu: %d sequences exceed the grid's 65535", b);
    // one thread per 4 channels (8- or 16-byte accesses), at most 512 threads = 8 waves per workgroup
    SAT_CHECK_ARG(d > 0 && d % 4 == 0 && d <= 2048, SAT_E_UNSUPPORTED, "dwconv_ln_silu: d = %d must be a multiple of 4 and <= 2048", d);
    SAT_CHECK_ARG((((uintptr_t)x | (uintptr_t)y | (uintptr_t)w | (uintptr_t)gamma | (uintptr_t)beta) & 15) == 0, SAT_E_INVALID, "dwconv_ln_silu: pointers must be 16-byte aligned");
    switch (fmt) {
        case SAT_GEMM_BF16: return launch_dwconv<bf16_t, 16>(x, w, gamma, beta, y, b, s_len, d, s);
        case SAT_GEMM_FP16: return launch_dwconv<_Float16, 16>(x, w, gamma, beta, y, b, s_len, d, s);
        case SAT_GEMM_FP32X: return launch_dwconv<float, 8>(x, w, gamma, beta, y, b, s_len, d, s);
    }
    sat_set_error("dwconv_ln_silu: unknown format %d", fmt);
    return SAT_E_INVALID;
}

int sat_launch_round_rows(const float* x, void* y, int m, int d, const float* scale1p, const float* shift, int rows_per_seq, int ld, int fmt,
                          hipStream_t s) {
    SAT_CHECK_ARG(x && y && m > 0 && d > 0 && d % 4 == 0 && (!scale1p || (shift && rows_per_seq > 0 && ld % 4 == 0)), SAT_E_INVALID, "round_rows: bad arguments");
    const int64_t n4 = (int64_t)m * d / 4;
    const dim3 grid((unsigned)cdiv(n4, 256)), block(256);
    switch (fmt) {
        case SAT_GEMM_BF16: hipLaunchKernelGGL(round_rows_kernel<bf16_t>, grid, block, 0, s, x, (bf16_t*)y, n4, d, scale1p, shift, rows_per_seq, ld); break;
        case SAT_GEMM_FP16: hipLaunchKernelGGL(round_rows_kernel<_Float16>, grid, block, 0, s, x, (_Float16*)y, n4, d, scale1p, shift, rows_per_seq, ld); break;
        case SAT_GEMM_FP32X: hipLaunchKernelGGL(round_rows_kernel<float>, grid, block, 0, s, x, (float*)y, n4, d, scale1p, shift, rows_per_seq, ld); break;
        default: sat_set_error("round_rows: unknown format %d", fmt); return SAT_E_INVALID;
    }
    SAT_LAUNCH_CHECK();
    return 0;
}

int sat_launch_silu_f32(float* h, int64_t n, hipStream_t s) {
    SAT_CHECK_ARG(h && n > 0, SAT_E_INVALID, "silu_f32: bad arguments");
    hipLaunchKernelGGL(silu_f32_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, s, h, n);
    SAT_LAUNCH_CHECK();
    return 0;
}
