// The two projections at the audio boundary of the local-attention codec (models/local_attention.py:226-236, 273-282 of the reference:
// rearrange "b c n -> b n c" + the bias-free project_in, the bias-free project_out + rearrange "b n c -> b c n").  The GEMM tiles of
// gemm_bf16.hip do not serve a contraction over 1 or 2 audio channels, nor a handful of output columns; both are bandwidth kernels (the
// row side moves d floats per time step, the channel-first side c), fp32 in every build of the codec, with both sides coalesced:
//   project_in   x [b, c_in, t] -> rows [b * t, d]      reads along t into LDS, writes 16 bytes per lane along d
//   project_out  rows [b * t, d] -> out [b, c_out, t]   reads 16 bytes per lane along d into LDS, writes along t
// Sums run over the contraction index in ascending order with one fused multiply-add per term.
#include "sat_common.h"

namespace {

constexpr int IO_ROWS = 64;       // time steps per tile
constexpr int IO_DK = 64;         // project_out: contraction chunk staged per round
constexpr int IO_LD = IO_DK + 1;  // its LDS row pitch: lane = row reads hit 64 distinct banks

// LDS: wt [c_in][dc] (the weight columns d0 .. d0 + dc of workgroup row blockIdx.y, transposed, staged once per workgroup) | xs [c_in][IO_ROWS].
// A workgroup walks tiles of IO_ROWS time steps of one batch item; lane -> (time step, four output channels).  dc % 4 == 0, c_in * dc <= 8192
__global__ __launch_bounds__(256) void local_attn_project_in_kernel(const float* __restrict__ x, const float* __restrict__ w, float* __restrict__ rows,
                                                                    int b, int c_in, int t, int d, int dc) {
    extern __shared__ __attribute__((aligned(16))) float io_lds[];
    float* wt = io_lds;
    float* xs = io_lds + (size_t)c_in * dc;
    const int d0 = blockIdx.y * dc, dn = d - d0 < dc ? d - d0 : dc;
    for (int i = threadIdx.x; i < c_in * dn; i += 256) {
        const int n = i / c_in, c = i - n * c_in;
        wt[c * dc + n] = w[(size_t)d0 * c_in + i];
    }
    const int d4 = dn / 4, tiles_t = (t + IO_ROWS - 1) / IO_ROWS;
    const long tiles = (long)b * tiles_t;
    for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int bi = (int)(tile / tiles_t), t0 = (int)(tile - (long)bi * tiles_t) * IO_ROWS;
        __syncthreads();      // wt staged; the previous tile's readers of xs are done
        for (int i = threadIdx.x; i < c_in * IO_ROWS; i += 256) {
            const int c = i / IO_ROWS, tt = i - c * IO_ROWS;
            xs[i] = t0 + tt < t ? x[((size_t)bi * c_in + c) * t + t0 + tt] : 0.f;
        }
        __syncthreads();
        for (int i = threadIdx.x; i < IO_ROWS * d4; i += 256) {
            const int tt = i / d4, q = i - tt * d4;
            if (t0 + tt >= t) break;      // (tt grows with i)
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            for (int c = 0; c < c_in; ++c) {
                const float xv = xs[c * IO_ROWS + tt];
                const f32x4 wv = reinterpret_cast<const f32x4*>(wt + (size_t)c * dc)[q];
                acc[0] = fmaf(xv, wv[0], acc[0]);
                acc[1] = fmaf(xv, wv[1], acc[1]);
                acc[2] = fmaf(xv, wv[2], acc[2]);
                acc[3] = fmaf(xv, wv[3], acc[3]);
            }
            reinterpret_cast<f32x4*>(rows + ((size_t)bi * t + t0 + tt) * d + d0)[q] = acc;
        }
    }
}

// One workgroup = IO_ROWS time steps of one batch item x up to 4 * NO output channels (blockIdx.y walks further groups of them: a codec's
// latent side has few rows and tens of channels, and the groups are what fills the device there).  The rows are staged IO_DK columns at a
// time; lane = time step, wave w owns the output channels o0 + w, o0 + w + 4, ...: the weight rows are wave-uniform
template <int NO>
__global__ __launch_bounds__(256) void local_attn_project_out_kernel(const float* __restrict__ rows, const float* __restrict__ w, float* __restrict__ out,
                                                                     int b, int c_out, int t, int d) {
    __shared__ float xs[IO_ROWS * IO_LD];
    const int tiles_t = (t + IO_ROWS - 1) / IO_ROWS;
    const int bi = blockIdx.x / tiles_t, t0 = (blockIdx.x - bi * tiles_t) * IO_ROWS;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int o0 = blockIdx.y * 4 * NO + wave;
    float acc[NO];
#pragma unroll
    for (int j = 0; j < NO; ++j) acc[j] = 0.f;
    for (int k0 = 0; k0 < d; k0 += IO_DK) {
        __syncthreads();
#pragma unroll
        for (int j = 0; j < IO_ROWS * IO_DK / 4 / 256; ++j) {
            const int i = threadIdx.x + j * 256, r = i / (IO_DK / 4), q = i - r * (IO_DK / 4);
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (t0 + r < t) v = reinterpret_cast<const f32x4*>(rows + ((size_t)bi * t + t0 + r) * d + k0)[q];
            float* dst = xs + r * IO_LD + 4 * q;
            dst[0] = v[0]; dst[1] = v[1]; dst[2] = v[2]; dst[3] = v[3];
        }
        __syncthreads();
        // a channel past c_out reads the last weight row and is not stored: the walk over k stays one loop for the wave's NO channels
        const float* wr[NO];
#pragma unroll
        for (int j = 0; j < NO; ++j) wr[j] = w + (size_t)(o0 + 4 * j < c_out ? o0 + 4 * j : c_out - 1) * d + k0;
#pragma unroll 16
        for (int k = 0; k < IO_DK; ++k) {
            const float xv = xs[lane * IO_LD + k];
#pragma unroll
            for (int j = 0; j < NO; ++j) acc[j] = fmaf(xv, wr[j][k], acc[j]);
        }
    }
    if (t0 + lane >= t) return;
#pragma unroll
    for (int j = 0; j < NO; ++j) {
        const int o = o0 + 4 * j;
        if (o < c_out) out[((size_t)bi * c_out + o) * t + t0 + lane] = acc[j];
    }
}

}  // namespace

int sat_launch_local_attn_project_in(const float* x, const float* w, float* rows, int b, int c_in, int t, int d, hipStream_t s) {
    SAT_CHECK_ARG(x && w && rows && b > 0 && c_in > 0 && t > 0 && d > 0, SAT_E_INVALID, "local_attn_project_in: bad arguments");
    SAT_CHECK_ARG(d % 4 == 0 && (((uintptr_t)rows) & 15) == 0, SAT_E_INVALID, "local_attn_project_in: d %d must be a multiple of 4 and the rows 16-byte aligned", d);
    SAT_CHECK_ARG(c_in <= 128, SAT_E_UNSUPPORTED, "local_attn_project_in: %d input channels: the kernel stages a tile of the input in LDS, c_in <= 128", c_in);
    // the weight columns one workgroup stages: at most 8192 floats (32 KiB) beside the at most 32 KiB of the input tile
    const int fit = (8192 / c_in) & ~3, dc = d < fit ? d : fit;
    const int lds = (c_in * dc + c_in * IO_ROWS) * 4;
    const int64_t tiles = (int64_t)b * cdiv(t, IO_ROWS);
    SAT_CHECK_ARG(cdiv(d, dc) <= 65535, SAT_E_UNSUPPORTED, "local_attn_project_in: d %d exceeds the grid", d);
    hipLaunchKernelGGL(local_attn_project_in_kernel, dim3((unsigned)(tiles < 2048 ? tiles : 2048), cdiv(d, dc)), dim3(256), lds, s, x, w, rows, b, c_in, t,
                       d, dc);
    SAT_LAUNCH_CHECK();
    return 0;
}

int sat_launch_local_attn_project_out(const float* rows, const float* w, float* out, int b, int c_out, int t, int d, hipStream_t s) {
    SAT_CHECK_ARG(rows && w && out && b > 0 && c_out > 0 && t > 0 && d > 0, SAT_E_INVALID, "local_attn_project_out: bad arguments");
    SAT_CHECK_ARG(d % IO_DK == 0 && (((uintptr_t)rows) & 15) == 0, SAT_E_INVALID,
                  "local_attn_project_out: d %d must be a multiple of %d and the rows 16-byte aligned", d, IO_DK);
    const int64_t tiles = (int64_t)b * cdiv(t, IO_ROWS);
    SAT_CHECK_ARG(tiles <= INT32_MAX && c_out <= 65535, SAT_E_UNSUPPORTED, "local_attn_project_out: %lld tiles / %d output channels exceed the grid",
                  (long long)tiles, c_out);
    if (c_out <= 4)
        hipLaunchKernelGGL(local_attn_project_out_kernel<1>, dim3((unsigned)tiles, 1), dim3(256), 0, s, rows, w, out, b, c_out, t, d);
    else
        hipLaunchKernelGGL(local_attn_project_out_kernel<2>, dim3((unsigned)tiles, cdiv(c_out, 8)), dim3(256), 0, s, rows, w, out, b, c_out, t, d);
    SAT_LAUNCH_CHECK();
    return 0;
}
