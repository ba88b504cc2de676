// The kernels of the Dance Diffusion U-Net (DiffusionAttnUnet1D, reference models/diffusion.py:376-479 on models/blocks.py:14-159) that no other
// plan has: the whole-item GroupNorm(1, c) with its GELU and residual add, the cubic 2x resamplers with reflect padding, the concat copy and the
// two layers at the audio boundary.  Activations are channel-last rows [b * t_level, c]; one batch item is t_level * c contiguous floats.
// All of them are bandwidth kernels, fp32 inside in every operand format; the 16-bit (or, in the verification mode, fp32) operand of the next
// convolution is rounded once, on the way out.  Compiled once, templated on the output type as layernorm.hip / ff_conv.hip.
//
// Determinism: nothing here uses an atomic.  The GroupNorm statistics are per-tile (mean, M2) partials in the caller's workspace, each the
// result of a fixed reduction tree inside its workgroup, combined by one workgroup per item in a fixed order in double precision.
#include "sat_common.h"

namespace {

constexpr int GN_TILE = 4096;      // floats per partial: 256 threads x 16

// sum over the 256 threads of a workgroup, the same value in every thread; the order is fixed (DPP tree per wave, then waves 0..3)
__device__ __forceinline__ float block_sum_256(float v, float* red) {
    v = wave_sum(v);
    __syncthreads();      // red may still be read from the previous call
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// part [b][tiles][2]: the mean of the tile's elements and the sum of their squared distances from it.  Two passes over registers: no
// cancellation however far the mean lies from zero
__global__ __launch_bounds__(256) void unet_gn_partials_kernel(const float* __restrict__ x, float* __restrict__ part, int64_t n, int tiles) {
    __shared__ float red[4];
    const int tile = blockIdx.x, item = blockIdx.y;
    const int64_t e0 = (int64_t)tile * GN_TILE;
    const int count = (int)(n - e0 < GN_TILE ? n - e0 : GN_TILE);      // a multiple of 4
    const float* xi = x + (int64_t)item * n + e0;
    f32x4 v[4];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int o = (i * 256 + threadIdx.x) * 4;
        v[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (o < count) v[i] = *reinterpret_cast<const f32x4*>(xi + o);
        s += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
    }
    const float mean = block_sum_256(s, red) / (float)count;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int o = (i * 256 + threadIdx.x) * 4;
        if (o < count) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float d = v[i][e] - mean;
                q = fmaf(d, d, q);
            }
        }
    }
    const float m2 = block_sum_256(q, red);
    if (threadIdx.x == 0) {
        float* p = part + ((int64_t)item * tiles + tile) * 2;
        p[0] = mean;
        p[1] = m2;
    }
}

__device__ __forceinline__ double block_sum_256_f64(double v, double* red) {
    __syncthreads();
    red[threadIdx.x] = v;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    return red[0];
}

// stats [b][2] = (mean, 1 / sqrt(var + eps)) of the item, biased variance (nn.GroupNorm); one workgroup per item, Chan's combination of the
// partials in double, thread i taking tiles i, i + 256, ... in ascending order and the 256 sums meeting in a fixed tree
__global__ __launch_bounds__(256) void unet_gn_finish_kernel(const float* __restrict__ part, float* __restrict__ stats, int64_t n, int tiles, float eps) {
    __shared__ double red[256];
    const int item = blockIdx.x;
    const float* p = part + (int64_t)item * tiles * 2;
    auto count_of = [&](int tile) { const int64_t r = n - (int64_t)tile * GN_TILE; return (double)(r < GN_TILE ? r : GN_TILE); };
    double s = 0.0;
    for (int tile = threadIdx.x; tile < tiles; tile += 256) s += count_of(tile) * (double)p[tile * 2];
    const double mean = block_sum_256_f64(s, red) / (double)n;
    double q = 0.0;
    for (int tile = threadIdx.x; tile < tiles; tile += 256) {
        const double d = (double)p[tile * 2] - mean;
        q += (double)p[tile * 2 + 1] + count_of(tile) * d * d;
    }
    const double var = block_sum_256_f64(q, red) / (double)n;
    if (threadIdx.x == 0) {
        stats[item * 2] = (float)mean;
        stats[item * 2 + 1] = (float)(1.0 / sqrt(var + (double)eps));
    }
}

__device__ __forceinline__ float gelu_erf(float v) { return 0.5f * v * (1.0f + erff(v * 0.70710678118654752f)); }

template <typename T>
__device__ __forceinline__ void store4(T* dst, const f32x4& v) {
    if constexpr (__is_same(T, float)) {
        *reinterpret_cast<f32x4*>(dst) = v;
    } else {
        typedef T t4 __attribute__((ext_vector_type(4)));
        t4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = (T)v[e];
        *reinterpret_cast<t4*>(dst) = o;
    }
}

// y = gelu?((x - mean) * rstd * gamma[ch] + beta[ch]) (+ skip); y -> out32 [M, c] and / or out_op [M, ld] (the operand of the next convolution).
// out32 may be x or skip: every element is read and written by the same thread
template <typename T>
__global__ __launch_bounds__(256) void unet_gn_apply_kernel(const float* x, const float* __restrict__ stats, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, const float* skip, float* out32, T* __restrict__ out_op,
                                                            int64_t total4, int64_t n, int c, int ld, int act) {
    sat_saturate_for<T>();
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total4) return;
    const int64_t e = i * 4, row = e / c;
    const int item = (int)(e / n), ch = (int)(e - row * c);
    const float mean = stats[item * 2], rstd = stats[item * 2 + 1];
    const f32x4 xv = *reinterpret_cast<const f32x4*>(x + e);
    const f32x4 g = *reinterpret_cast<const f32x4*>(gamma + ch), bt = *reinterpret_cast<const f32x4*>(beta + ch);
    f32x4 y;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float v = (xv[k] - mean) * rstd * g[k] + bt[k];
        y[k] = act ? gelu_erf(v) : v;
    }
    if (skip) {
        const f32x4 sv = *reinterpret_cast<const f32x4*>(skip + e);
#pragma unroll
        for (int k = 0; k < 4; ++k) y[k] += sv[k];
    }
    if (out32) *reinterpret_cast<f32x4*>(out32 + e) = y;
    if (out_op) store4<T>(out_op + row * ld + ch, y);
}

// out [m, ld] (first c columns) = x [m, c] rounded to T: the skip half of a level's concat buffer, and the operand image of the stream
template <typename T>
__global__ __launch_bounds__(256) void unet_cast_rows_kernel(const float* __restrict__ x, T* __restrict__ out, int64_t total4, int c, int ld) {
    sat_saturate_for<T>();
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total4) return;
    const int64_t e = i * 4, row = e / c;
    store4<T>(out + row * ld + (int)(e - row * c), *reinterpret_cast<const f32x4*>(x + e));
}

// blocks.py:104-109: the 'cubic' kernel; the upsampler uses twice these values
__constant__ float kCubic[8] = {-0.01171875f, -0.03515625f, 0.11328125f, 0.43359375f, 0.43359375f, 0.11328125f, -0.03515625f, -0.01171875f};

__device__ __forceinline__ int reflect(int i, int s) { return i < 0 ? -i : (i >= s ? 2 * (s - 1) - i : i); }

// Downsample1d('cubic'): reflect pad 3, 8 taps, stride 2, per channel.  x [b * s, c] -> out32 [b * s / 2, c] and its operand image (s even, s > 3)
template <typename T>
__global__ __launch_bounds__(256) void unet_down_kernel(const float* __restrict__ x, float* __restrict__ out32, T* __restrict__ out_op, int64_t total4,
                                                        int s, int c) {
    sat_saturate_for<T>();
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total4) return;
    const int64_t e = i * 4, row = e / c;
    const int ch = (int)(e - row * c), so = s >> 1;
    const int item = (int)(row / so), p = (int)(row - (int64_t)item * so);
    const float* xi = x + (int64_t)item * s * c + ch;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(xi + (int64_t)reflect(2 * p + j - 3, s) * c);
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[k] = fmaf(kCubic[j], v[k], acc[k]);
    }
    if (out32) *reinterpret_cast<f32x4*>(out32 + e) = acc;
    if (out_op) store4<T>(out_op + e, acc);
}

// Upsample1d('cubic'): reflect pad 2, conv_transpose1d(2 * kernel, stride 2, padding 7).  Output position m of 2 s gathers the taps j with
// m + 7 - j even, from padded position (m + 7 - j) / 2, i.e. input position reflect((m + 7 - j) / 2 - 2).  x [b * s, c] -> out [b * 2 s, ld]
template <typename T>
__global__ __launch_bounds__(256) void unet_up_kernel(const float* __restrict__ x, T* __restrict__ out, int64_t total4, int s, int c, int ld) {
    sat_saturate_for<T>();
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total4) return;
    const int64_t e = i * 4, row = e / c;
    const int ch = (int)(e - row * c), so = s * 2;
    const int item = (int)(row / so), m = (int)(row - (int64_t)item * so);
    const float* xi = x + (int64_t)item * s * c + ch;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
        const int j = 2 * jj + ((m + 1) & 1);      // m even: the odd taps; m odd: the even ones
        const int src = reflect(((m + 7 - j) >> 1) - 2, s);
        const f32x4 v = *reinterpret_cast<const f32x4*>(xi + (int64_t)src * c);
        const float w = 2.0f * kCubic[j];
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[k] = fmaf(w, v[k], acc[k]);
    }
    store4<T>(out + row * ld + ch, acc);
}

// ---- the input boundary: cat([x * in_scale, planes(FourierFeatures(1, 16)(t))]) [b, io + 16, t] through net.0.main.0 (taps, zero padding of
// the CONCATENATED tensor: the timestep planes end with the sequence) and net.0.skip (1 x 1), both into rows [b * t, c].
// One workgroup = IN_TT time steps of one item x 128 output channels; thread = output channel, the input tile is broadcast from LDS.
constexpr int IN_TT = 32, IN_LD = IN_TT + 6;

__global__ __launch_bounds__(128) void unet_input_kernel(const float* __restrict__ x, const float* __restrict__ tval, float in_scale,
                                                         const float* __restrict__ w_embed, const float* __restrict__ w_main,
                                                         const float* __restrict__ b_main, const float* __restrict__ w_skip, float* __restrict__ y,
                                                         float* __restrict__ sk, int io, int t, int c, int taps) {
    __shared__ float xs[128 * IN_LD];
    __shared__ float emb[16];
    const int cin = io + 16, hw = taps >> 1;
    const int bi = blockIdx.z, t0 = blockIdx.x * IN_TT, n = blockIdx.y * 128 + threadIdx.x;
    if (threadIdx.x < 8) {
        // FourierFeatures.forward: f = (2 pi * t) @ weight.T in fp32, then cat([cos f, sin f])
        const float f = (tval[bi] * 6.283185307179586f) * w_embed[threadIdx.x];
        emb[threadIdx.x] = cosf(f);
        emb[8 + threadIdx.x] = sinf(f);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < cin * IN_LD; i += 128) {
        const int ci = i / IN_LD, tt = i - ci * IN_LD;
        const int pos = t0 + tt - hw;
        float v = 0.f;
        if (tt < IN_TT + 2 * hw && pos >= 0 && pos < t) v = ci < io ? x[((int64_t)bi * io + ci) * t + pos] * in_scale : emb[ci - io];
        xs[i] = v;
    }
    __syncthreads();
    if (n >= c) return;
    float acc[IN_TT], acc2[IN_TT];
#pragma unroll
    for (int tt = 0; tt < IN_TT; ++tt) acc[tt] = acc2[tt] = 0.f;
    for (int ci = 0; ci < cin; ++ci) {
        const float* xr = xs + ci * IN_LD;
        for (int j = 0; j < taps; ++j) {
            const float w = w_main[((int64_t)n * cin + ci) * taps + j];
#pragma unroll
            for (int tt = 0; tt < IN_TT; ++tt) acc[tt] = fmaf(w, xr[tt + j], acc[tt]);
        }
        const float w2 = w_skip[(int64_t)n * cin + ci];
#pragma unroll
        for (int tt = 0; tt < IN_TT; ++tt) acc2[tt] = fmaf(w2, xr[tt + hw], acc2[tt]);
    }
    const float bias = b_main ? b_main[n] : 0.f;
#pragma unroll
    for (int tt = 0; tt < IN_TT; ++tt) {
        if (t0 + tt < t) {
            const int64_t o = ((int64_t)bi * t + t0 + tt) * c + n;
            y[o] = acc[tt] + bias;
            sk[o] = acc2[tt];
        }
    }
}

// ---- the output boundary: the last block's main.3 (c -> io, taps, zero padding) on h plus its 1 x 1 skip on the block's input xin, both rows
// [b * t, c], written channel-first out [b, io, t].  One wave per time step, lanes over the channels, one fixed DPP tree per output
constexpr int OUT_TT = 64;

__global__ __launch_bounds__(256) void unet_output_kernel(const float* __restrict__ h, const float* __restrict__ xin, const float* __restrict__ w_main,
                                                          const float* __restrict__ b_main, const float* __restrict__ w_skip, float* __restrict__ out,
                                                          int io, int t, int c, int taps) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int bi = blockIdx.y, hw = taps >> 1;
    const int t_first = blockIdx.x * OUT_TT + wave * (OUT_TT / 4);
    for (int ts = t_first; ts < t_first + OUT_TT / 4 && ts < t; ++ts) {      // wave-uniform
        const float* hr = h + ((int64_t)bi * t + ts) * c;
        const float* xr = xin + ((int64_t)bi * t + ts) * c;
        for (int o = 0; o < io; ++o) {
            float acc = 0.f;
            for (int ci = lane; ci < c; ci += 64) {
                const float* w = w_main + ((int64_t)o * c + ci) * taps;
                for (int j = 0; j < taps; ++j) {
                    const int pos = ts + j - hw;
                    if (pos >= 0 && pos < t) acc = fmaf(w[j], hr[(int64_t)(j - hw) * c + ci], acc);
                }
                acc = fmaf(w_skip[(int64_t)o * c + ci], xr[ci], acc);
            }
            acc = wave_sum(acc);
            if (lane == 0) out[((int64_t)bi * io + o) * t + ts] = acc + (b_main ? b_main[o] : 0.f);
        }
    }
}

template <typename T>
int apply_t(const float* x, const float* stats, const float* gamma, const float* beta, const float* skip, float* out32, void* out_op, int b, int64_t n, int c,
            int ld, int act, hipStream_t s) {
    const int64_t total4 = (int64_t)b * n / 4;
    hipLaunchKernelGGL(unet_gn_apply_kernel<T>, dim3((unsigned)cdiv(total4, 256)), dim3(256), 0, s, x, stats, gamma, beta, skip, out32, (T*)out_op, total4, n, c,
                       ld, act);
    SAT_LAUNCH_CHECK();
    return 0;
}

bool fmt_ok(int fmt) { return fmt == SAT_GEMM_BF16 || fmt == SAT_GEMM_FP16 || fmt == SAT_GEMM_FP32X; }
bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

int sat_unet_gn_tiles(int64_t n) { return (int)cdiv(n, (int64_t)GN_TILE); }

int sat_launch_unet_gn_stats(const float* x, float* part, float* stats, int b, int64_t n, float eps, hipStream_t s) {
    SAT_CHECK_ARG(x && part && stats && b > 0 && b <= 65535 && n > 0 && n % 4 == 0 && aligned16(x), SAT_E_INVALID, "unet_gn_stats: bad arguments");
    SAT_CHECK_ARG(cdiv(n, (int64_t)GN_TILE) <= (1 << 24), SAT_E_UNSUPPORTED, "unet_gn_stats: %lld elements per item", (long long)n);
    const int tiles = sat_unet_gn_tiles(n);
    hipLaunchKernelGGL(unet_gn_partials_kernel, dim3(tiles, b), dim3(256), 0, s, x, part, n, tiles);
    SAT_LAUNCH_CHECK();
    hipLaunchKernelGGL(unet_gn_finish_kernel, dim3(b), dim3(256), 0, s, part, stats, n, tiles, eps);
    SAT_LAUNCH_CHECK();
    return 0;
}

int sat_launch_unet_gn_apply(const float* x, const float* stats, const float* gamma, const float* beta, const float* skip, float* out32, void* out_op, int b,
                             int rows, int c, int ld, int act, int fmt, hipStream_t s) {
    SAT_CHECK_ARG(x && stats && gamma && beta && (out32 || out_op) && b > 0 && rows > 0 && c > 0 && c % 4 == 0 && (!out_op || (ld >= c && ld % 8 == 0)) && fmt_ok(fmt),
                  SAT_E_INVALID, "unet_gn_apply: bad arguments");
    SAT_CHECK_ARG(aligned16(x) && aligned16(gamma) && aligned16(beta) && aligned16(skip) && aligned16(out32) && aligned16(out_op), SAT_E_INVALID,
                  "unet_gn_apply: pointers must be 16-byte aligned");
    const int64_t n = (int64_t)rows * c;
    if (fmt == SAT_GEMM_FP16) return apply_t<_Float16>(x, stats, gamma, beta, skip, out32, out_op, b, n, c, ld, act, s);
    if (fmt == SAT_GEMM_BF16) return apply_t<bf16_t>(x, stats, gamma, beta, skip, out32, out_op, b, n, c, ld, act, s);
    return apply_t<float>(x, stats, gamma, beta, skip, out32, out_op, b, n, c, ld, act, s);
}

int sat_launch_unet_cast_rows(const float* x, void* out, int64_t m, int c, int ld, int fmt, hipStream_t s) {
    SAT_CHECK_ARG(x && out && m > 0 && c > 0 && c % 4 == 0 && ld >= c && ld % 8 == 0 && fmt_ok(fmt) && aligned16(x) && aligned16(out), SAT_E_INVALID,
                  "unet_cast_rows: bad arguments");
    const int64_t total4 = m * c / 4;
    const dim3 grid((unsigned)cdiv(total4, 256)), block(256);
    if (fmt == SAT_GEMM_FP16) hipLaunchKernelGGL(unet_cast_rows_kernel<_Float16>, grid, block, 0, s, x, (_Float16*)out, total4, c, ld);
    else if (fmt == SAT_GEMM_BF16) hipLaunchKernelGGL(unet_cast_rows_kernel<bf16_t>, grid, block, 0, s, x, (bf16_t*)out, total4, c, ld);
    else hipLaunchKernelGGL(unet_cast_rows_kernel<float>, grid, block, 0, s, x, (float*)out, total4, c, ld);
    SAT_LAUNCH_CHECK();
    return 0;
}

int sat_launch_unet_downsample(const float* x, float* out32, void* out_op, int b, int s_len, int c, int fmt, hipStream_t s) {
    SAT_CHECK_ARG(x && (out32 || out_op) && b > 0 && c > 0 && c % 8 == 0 && fmt_ok(fmt) && aligned16(x) && aligned16(out32) && aligned16(out_op), SAT_E_INVALID,
                  "unet_downsample: bad arguments");
    SAT_CHECK_ARG(s_len > 3 && s_len % 2 == 0, SAT_E_INVALID, "unet_downsample: %d rows per item (even and above the reflect pad of 3)", s_len);
    const int64_t total4 = (int64_t)b * (s_len / 2) * c / 4;
    const dim3 grid((unsigned)cdiv(total4, 256)), block(256);
    if (fmt == SAT_GEMM_FP16) hipLaunchKernelGGL(unet_down_kernel<_Float16>, grid, block, 0, s, x, out32, (_Float16*)out_op, total4, s_len, c);
    else if (fmt == SAT_GEMM_BF16) hipLaunchKernelGGL(unet_down_kernel<bf16_t>, grid, block, 0, s, x, out32, (bf16_t*)out_op, total4, s_len, c);
    else hipLaunchKernelGGL(unet_down_kernel<float>, grid, block, 0, s, x, out32, (float*)out_op, total4, s_len, c);
    SAT_LAUNCH_CHECK();
    return 0;
}

int sat_launch_unet_upsample(const float* x, void* out, int b, int s_len, int c, int ld, int fmt, hipStream_t s) {
    SAT_CHECK_ARG(x && out && b > 0 && c > 0 && c % 8 == 0 && ld >= c && ld % 8 == 0 && fmt_ok(fmt) && aligned16(x) && aligned16(out), SAT_E_INVALID,
                  "unet_upsample: bad arguments");
    SAT_CHECK_ARG(s_len > 2 && s_len <= (1 << 29), SAT_E_INVALID, "unet_upsample: %d rows per item (above the reflect pad of 2)", s_len);
    const int64_t total4 = (int64_t)b * s_len * 2 * c / 4;
    const dim3 grid((unsigned)cdiv(total4, 256)), block(256);
    if (fmt == SAT_GEMM_FP16) hipLaunchKernelGGL(unet_up_kernel<_Float16>, grid, block, 0, s, x, (_Float16*)out, total4, s_len, c, ld);
    else if (fmt == SAT_GEMM_BF16) hipLaunchKernelGGL(unet_up_kernel<bf16_t>, grid, block, 0, s, x, (bf16_t*)out, total4, s_len, c, ld);
    else hipLaunchKernelGGL(unet_up_kernel<float>, grid, block, 0, s, x, (float*)out, total4, s_len, c, ld);
    SAT_LAUNCH_CHECK();
    return 0;
}

int sat_launch_unet_input(const float* x, const float* tval, float in_scale, const float* w_embed, const float* w_main, const float* b_main,
                          const float* w_skip, float* y, float* sk, int b, int io, int t, int c, int taps, hipStream_t s) {
    SAT_CHECK_ARG(x && tval && w_embed && w_main && w_skip && y && sk && b > 0 && b <= 65535 && io > 0 && t > 0 && c > 0, SAT_E_INVALID, "unet_input: bad arguments");
    SAT_CHECK_ARG(io + 16 <= 128, SAT_E_UNSUPPORTED, "unet_input: io_channels %d + 16 timestep planes exceed the 128 rows of the staged tile", io);
    SAT_CHECK_ARG(taps >= 1 && taps <= 7 && (taps & 1), SAT_E_UNSUPPORTED, "unet_input: kernel_size %d (1, 3, 5 or 7)", taps);
    SAT_CHECK_ARG(cdiv(c, 128) <= 65535, SAT_E_UNSUPPORTED, "unet_input: %d channels exceed the grid", c);
    hipLaunchKernelGGL(unet_input_kernel, dim3(cdiv(t, IN_TT), cdiv(c, 128), b), dim3(128), 0, s, x, tval, in_scale, w_embed, w_main, b_main, w_skip, y, sk, io, t,
                       c, taps);
    SAT_LAUNCH_CHECK();
    return 0;
}

int sat_launch_unet_output(const float* h, const float* xin, const float* w_main, const float* b_main, const float* w_skip, float* out, int b, int io, int t,
                           int c, int taps, hipStream_t s) {
    SAT_CHECK_ARG(h && xin && w_main && w_skip && out && b > 0 && b <= 65535 && io > 0 && t > 0 && c > 0, SAT_E_INVALID, "unet_output: bad arguments");
    SAT_CHECK_ARG(c % 64 == 0, SAT_E_UNSUPPORTED, "unet_output: %d channels (a multiple of 64: one wave walks a row)", c);
    SAT_CHECK_ARG(taps >= 1 && taps <= 7 && (taps & 1), SAT_E_UNSUPPORTED, "unet_output: kernel_size %d (1, 3, 5 or 7)", taps);
    hipLaunchKernelGGL(unet_output_kernel, dim3(cdiv(t, OUT_TT), b), dim3(256), 0, s, h, xin, w_main, b_main, w_skip, out, io, t, c, taps);
    SAT_LAUNCH_CHECK();
    return 0;
}
