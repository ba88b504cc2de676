// The convolutional feed-forward of the DiT (ff_kwargs use_conv, reference models/transformer.py:211-287): a Linear that became
// Conv1d(k, padding = k / 2) along the sequence is ONE contraction of length k * K over k row-shifted copies of the A operand,
//     out[b, s, :] = sum_j W_j A[b, s + j - k / 2, :],      rows outside [0, S) of sequence b are zero,
// on the 16-bit MFMA with fp32 accumulation.  The weight arrives tap-major, [N, k * K] (pack_conv_taps_kernel): K-tile kt of the loop is
// columns (kt * 64) % K of tap (kt * 64) / K, and the A tile of that step is the same 128 x 64 tile with its row base moved by tap - k / 2.
// A stays in the plan's dense [B * S, K] layout: the lane that stages a 16-byte piece of row m tests 0 <= m % S + tap - k / 2 < S and
// stages zeros otherwise (one compare per 16-byte load; m % S is computed once per thread and row), so no producer writes guard rows and
// the workspace does not grow.  Compiled once, templated on the operand type, as layernorm.hip / conformer.hip.
//
// 128 x 128 tile, eight waves of 32 x 64 (1 x 2 blocks of v_mfma_f32_32x32x16), K-tile 64, two LDS stages (64 KiB) with the XOR-swizzled
// tile layout of sat_common.h (lds_tile_off), staged through TWO register sets: while tile kt is contracted out of LDS, tile kt + 1 sits in
// (or is on its way to) one set and the loads of tile kt + 2 are issued into the other, so a global load has a whole K-step and the
// contraction of another to arrive.  At one prompt the grid is one workgroup per CU: the eight waves are two per SIMD.  Epilogues: FFC_RESID -- C += [gate (.)] (acc + bias), the FF-out
// form of EPI_RESID; FFC_ACT16 -- H = act(acc + bias) rounded to the operand type, the FF-in form of EPI_ACT16.
#include "sat_common.h"

namespace {

template <typename T>
using Vec8 = T __attribute__((ext_vector_type(8)));

template <typename T>
__device__ __forceinline__ f32x16 mfma_op(Vec8<T> a, Vec8<T> b, f32x16 c) {
    if constexpr (__is_same(T, _Float16)) return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
    else return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}

constexpr int BM = 128, BN = 128, NT = 512, CH = BM * 8 / NT;      // CH: 16-byte pieces of each operand tile per thread
constexpr int STAGE_BYTES = (BM + BN) * 128;
constexpr int LDS_BYTES = 2 * STAGE_BYTES;

template <typename T, int EPI>
__global__ __launch_bounds__(NT) void ff_conv_kernel(FfConvArgs g) {
    sat_saturate_for<T>();
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, half = lane >> 5, l31 = lane & 31;      // wave tile: rows wm * 32, columns wn * 64
    const int S = g.S, M = g.B * g.S, N = g.N, K = g.K, taps = g.taps, hw = g.taps >> 1;
    const int tiles_m = (M + BM - 1) / BM;
    const int tn = blockIdx.x / tiles_m, tm = blockIdx.x - tn * tiles_m;      // m fastest: the workgroups of one W panel are neighbours
    const int m0 = tm * BM, n0 = tn * BN;
    const T* __restrict__ A = (const T*)g.A;
    const T* __restrict__ W = (const T*)g.W;
    const size_t ldw = (size_t)taps * K;

    int row[CH], chk[CH], pos[CH];      // pos: the row's position in its sequence; rows behind M get one no tap can bring into [0, S)
    const T* a_ptr[CH];
    const T* b_ptr[CH];
#pragma unroll
    for (int i = 0; i < CH; ++i) {
        const int id = i * NT + tid;
        row[i] = id >> 3;
        chk[i] = id & 7;
        const int gm = m0 + row[i];
        pos[i] = gm < M ? gm % S : -(1 << 20);
        a_ptr[i] = A + (ptrdiff_t)gm * K + chk[i] * 8;
        b_ptr[i] = W + (size_t)(n0 + row[i]) * ldw + chk[i] * 8;
    }

    f32x16 acc[2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;

    const int nk = taps * (K / 64);
    u32x4 ra0[CH], rb0[CH], ra1[CH], rb1[CH];      // the two register sets
    int tap = 0, kc = 0, next = 0;      // the K-tile the next gload fetches: tile `next`, columns kc .. kc + 63 of tap `tap`
    auto gload = [&](u32x4 (&ra)[CH], u32x4 (&rb)[CH]) {
        if (next >= nk) return;      // (workgroup-uniform) behind the last tile: the set keeps what it has, which nobody contracts
        ++next;
        const int shift = tap - hw;
#pragma unroll
        for (int i = 0; i < CH; ++i) {
            const bool in_seq = (unsigned)(pos[i] + shift) < (unsigned)S;      // the only read of A: a row of the tile's own sequence
            u32x4 v = {0u, 0u, 0u, 0u};
            if (in_seq) v = *reinterpret_cast<const u32x4*>(a_ptr[i] + (ptrdiff_t)shift * K + kc);
            ra[i] = v;
        }
#pragma unroll
        for (int i = 0; i < CH; ++i) rb[i] = *reinterpret_cast<const u32x4*>(b_ptr[i] + (size_t)tap * K + kc);
        kc += 64;
        if (kc == K) { kc = 0; ++tap; }
    };
    auto lstore = [&](int stage, const u32x4 (&ra)[CH], const u32x4 (&rb)[CH]) {
        char* sa = smem + stage * STAGE_BYTES;
        char* sb = sa + BM * 128;
#pragma unroll
        for (int i = 0; i < CH; ++i) *reinterpret_cast<u32x4*>(sa + lds_tile_off(row[i], chk[i])) = ra[i];
#pragma unroll
        for (int i = 0; i < CH; ++i) *reinterpret_cast<u32x4*>(sb + lds_tile_off(row[i], chk[i])) = rb[i];
    };
    auto compute = [&](int stage) {
        const char* sa = smem + stage * STAGE_BYTES;
        const char* sb = sa + BM * 128;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            Vec8<T> bf[2];
            const Vec8<T> af = *reinterpret_cast<const Vec8<T>*>(sa + lds_tile_off(wm * 32 + l31, ks * 2 + half));
#pragma unroll
            for (int j = 0; j < 2; ++j) bf[j] = *reinterpret_cast<const Vec8<T>*>(sb + lds_tile_off(wn * 64 + j * 32 + l31, ks * 2 + half));
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[j] = mfma_op<T>(af, bf[j], acc[j]);
        }
    };

    // At the top of step kt: LDS stage kt & 1 holds tile kt, one register set tile kt + 1.  The step issues tile kt + 2 into the other set,
    // contracts tile kt, stores tile kt + 1 into the other stage (last read in step kt - 1, behind that step's barrier) and meets the
    // barrier.  Two steps per trip so that the sets are named, not indexed; behind the last tile there is nothing to store (the set was
    // never loaded) and the loop ends on a workgroup-uniform test
    gload(ra0, rb0);
    lstore(0, ra0, rb0);
    __syncthreads();
    gload(ra0, rb0);
    for (int kt = 0; kt < nk; kt += 2) {
        gload(ra1, rb1);
        compute(0);
        if (kt + 1 >= nk) break;
        lstore(1, ra0, rb0);
        __syncthreads();
        gload(ra0, rb0);
        compute(1);
        if (kt + 2 >= nk) break;
        lstore(0, ra1, rb1);
        __syncthreads();
    }

    // acc[j][r]: row = (r & 3) + 8 * (r >> 2) + 4 * half, col = j * 32 + l31
    const int mw = m0 + wm * 32, nw = n0 + wn * 64;
    float bia[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) bia[j] = g.bias ? g.bias[nw + j * 32 + l31] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        {
            const int m = mw + (r & 3) + 8 * (r >> 2) + 4 * half;
            if (m >= M) continue;
            if constexpr (EPI == FFC_RESID) {
                float* __restrict__ c = g.C + (size_t)m * g.ldc + nw + l31;
                const float* gr = g.gate ? g.gate + (size_t)(m / g.gate_rows) * g.gate_ld + nw + l31 : nullptr;      // adaLN: wave-uniform test
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    float v = acc[j][r] + bia[j];
                    if (gr) v *= gr[j * 32];
                    c[j * 32] = g.accumulate ? c[j * 32] + v : v;
                }
            } else {
                T* __restrict__ h = (T*)g.H + (size_t)m * N + nw + l31;
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const float v = acc[j][r] + bia[j];
                    h[j * 32] = (T)(g.act ? silu_f(v) : v);
                }
            }
        }
    }
}

// w [n, k, taps] (Conv1d weight) -> out [n, taps * k], tap-major: out[n][j * k + c] = w[n][c][j]
template <typename T>
__global__ __launch_bounds__(256) void pack_conv_taps_kernel(const float* __restrict__ w, T* __restrict__ out, int64_t total, int k, int taps) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int64_t n = i / ((int64_t)taps * k);
    const int rem = (int)(i - n * taps * k), j = rem / k, c = rem - j * k;
    out[i] = (T)w[(n * k + c) * taps + j];
}

// fp32 verification mode: the row gather in front of sat_gemm_f32, out [b * s_len, taps * k], out[m][j * k + c] = a[m + j - taps / 2][c] or 0
__global__ __launch_bounds__(256) void im2col_rows_f32_kernel(const float* __restrict__ a, float* __restrict__ out, int64_t total4, int s_len, int k,
                                                               int taps) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total4) return;
    const int k4 = k >> 2;
    const int64_t m = i / ((int64_t)taps * k4);
    const int rem = (int)(i - m * taps * k4), j = rem / k4, c4 = rem - j * k4;
    const int p = (int)(m % s_len) + j - (taps >> 1);
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (p >= 0 && p < s_len) v = *reinterpret_cast<const f32x4*>(a + (m + j - (taps >> 1)) * k + c4 * 4);
    *reinterpret_cast<f32x4*>(out + i * 4) = v;
}

template <typename T>
int launch_ff_conv(const FfConvArgs& a, hipStream_t s) {
    const int M = a.B * a.S;
    const dim3 grid((unsigned)(cdiv(M, BM) * (a.N / BN)));
    if (a.epi == FFC_RESID) {
        auto kern = ff_conv_kernel<T, FFC_RESID>;
        SAT_TRY(sat_ensure_dynamic_lds(reinterpret_cast<const void*>(kern), LDS_BYTES));
        hipLaunchKernelGGL(kern, grid, dim3(NT), LDS_BYTES, s, a);
    } else {
        auto kern = ff_conv_kernel<T, FFC_ACT16>;
        SAT_TRY(sat_ensure_dynamic_lds(reinterpret_cast<const void*>(kern), LDS_BYTES));
        hipLaunchKernelGGL(kern, grid, dim3(NT), LDS_BYTES, s, a);
    }
    SAT_LAUNCH_CHECK();
    return 0;
}

}  // namespace

int sat_launch_ff_conv(const FfConvArgs& a, hipStream_t s) {
    SAT_CHECK_ARG(a.A && a.W && a.B > 0 && a.S > 0 && (int64_t)a.B * a.S <= (1 << 30), SAT_E_INVALID, "ff_conv: bad arguments");
    SAT_CHECK_ARG(a.taps >= 1 && a.taps <= 7 && (a.taps & 1), SAT_E_UNSUPPORTED, "ff_conv: kernel size %d (odd, 1 to 7)", a.taps);
    SAT_CHECK_ARG(a.K > 0 && a.K % 64 == 0 && a.N > 0 && a.N % BN == 0, SAT_E_UNSUPPORTED,
                  "ff_conv: K = %d must be a multiple of 64 and N = %d a multiple of %d", a.K, a.N, BN);
    SAT_CHECK_ARG((int64_t)cdiv(a.B * a.S, BM) * (a.N / BN) <= INT32_MAX, SAT_E_UNSUPPORTED, "ff_conv: grid too large");
    SAT_CHECK_ARG(a.epi == FFC_RESID ? (a.C && a.ldc >= a.N && (!a.gate || a.gate_rows > 0)) : (a.epi == FFC_ACT16 && a.H != nullptr), SAT_E_INVALID,
                  "ff_conv: epilogue %d without its output", a.epi);
    SAT_CHECK_ARG((((uintptr_t)a.A | (uintptr_t)a.W) & 15) == 0, SAT_E_INVALID, "ff_conv: operands must be 16-byte aligned");
    if (a.fmt == SAT_GEMM_FP16) return launch_ff_conv<_Float16>(a, s);
    if (a.fmt == SAT_GEMM_BF16) return launch_ff_conv<bf16_t>(a, s);
    sat_set_error("ff_conv: operand format %d is neither bf16 nor fp16", a.fmt);
    return SAT_E_UNSUPPORTED;
}

int sat_launch_pack_conv_taps(const float* w, void* out, int n, int k, int taps, int fmt, hipStream_t s) {
    SAT_CHECK_ARG(w && out && n > 0 && k > 0 && taps > 0, SAT_E_INVALID, "pack_conv_taps: bad arguments");
    const int64_t total = (int64_t)n * k * taps;
    const dim3 grid((unsigned)cdiv(total, 256)), block(256);
    switch (fmt) {
        case SAT_GEMM_BF16: hipLaunchKernelGGL(pack_conv_taps_kernel<bf16_t>, grid, block, 0, s, w, (bf16_t*)out, total, k, taps); break;
        case SAT_GEMM_FP16: hipLaunchKernelGGL(pack_conv_taps_kernel<_Float16>, grid, block, 0, s, w, (_Float16*)out, total, k, taps); break;
        case SAT_GEMM_FP32X: hipLaunchKernelGGL(pack_conv_taps_kernel<float>, grid, block, 0, s, w, (float*)out, total, k, taps); break;
        default: sat_set_error("pack_conv_taps: unknown format %d", fmt); return SAT_E_INVALID;
    }
    SAT_LAUNCH_CHECK();
    return 0;
}

int sat_launch_im2col_rows_f32(const float* a, float* out, int b, int s_len, int k, int taps, hipStream_t s) {
    SAT_CHECK_ARG(a && out && b > 0 && s_len > 0 && k > 0 && k % 4 == 0 && taps >= 1 && (taps & 1), SAT_E_INVALID, "im2col_rows_f32: bad arguments");
    const int64_t total4 = (int64_t)b * s_len * taps * (k / 4);
    hipLaunchKernelGGL(im2col_rows_f32_kernel, dim3((unsigned)cdiv(total4, 256)), dim3(256), 0, s, a, out, total4, s_len, k, taps);
    SAT_LAUNCH_CHECK();
    return 0;
}
