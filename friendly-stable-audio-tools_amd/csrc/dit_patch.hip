// The two fp32 boundary kernels of a patchified DiT (DiffusionTransformer patch_size P > 1, models/dit.py:197-224 of the reference) and the
// weight folds in front of them.  A token is P consecutive latent frames: "b (t p) c -> b t (c p)" behind preprocess_conv, feature index
// c * P + p (channel-major, frame-minor), and "b (c p) t -> b c (t p)" in front of postprocess_conv.  Both 1x1 convs act per frame, so they
// fold into the projections as they do at P = 1, with the channel mix applied inside each p:
//   WeffT_in[c' P + p][n] = W_in[n][c' P + p] + sum_c W_in[n][c P + p] W_pre[c][c']       ([Ci P][D], transposed as the kernel reads it)
//   WeffT_out[n][c' P + p] = W_out[c' P + p][n] + sum_c W_post[c'][c] W_out[c P + p][n]   ([D][C P])
// The P = 1 kernels of dit_glue.hip are not touched: a plan without sat_dit_plan_set_patch launches them as before.
#include "dit_glue.h"

namespace {

__global__ void fold_in_patch_kernel(const float* __restrict__ Win, const float* __restrict__ Wpre, float* __restrict__ WeffT, int D, int Ci, int P) {
    const int K = Ci * P;
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= D * K) return;
    const int n = i / K, j = i - n * K, c1 = j / P, p = j - c1 * P;
    float acc = Win[i];
    for (int c = 0; c < Ci; ++c) acc += Win[(size_t)n * K + c * P + p] * Wpre[c * Ci + c1];
    WeffT[(size_t)j * D + n] = acc;
}
__global__ void fold_out_patch_kernel(const float* __restrict__ Wout, const float* __restrict__ Wpost, float* __restrict__ WeffT, int D, int C, int P) {
    const int N = C * P;
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N * D) return;
    const int j = i / D, n = i - j * D, c1 = j / P, p = j - c1 * P;
    float acc = Wout[i];
    for (int c = 0; c < C; ++c) acc += Wpost[c1 * C + c] * Wout[(size_t)(c * P + p) * D + n];
    WeffT[(size_t)n * N + j] = acc;
}

// X[b, off + t', n] = xscale * sum_{c,p} WeffT[c P + p][n] * x[b % xB][c][t' P + p]  (+ the concat channels, unscaled), off = S - T'.
// The shape of input_proj_kernel (dit_glue.hip): one workgroup = IPP_TT tokens x 256 output channels, thread = output channel n with one
// accumulator per token, the weight read transposed (consecutive lanes, consecutive floats) and the inputs through wave-uniform addresses
// (scalar loads, no LDS: the P = 1 kernel's comment has the measurement).  Per input channel the IPP_TT tokens cover IPP_TT * P contiguous
// frames; with PT = P at compile time (2, 4, 8) both inner loops unroll and those frames arrive in wide scalar loads, PT = 0 runs any P.
// EXTRA as at P = 1: the Cc concat channels follow the C latent ones in WeffT, are added unscaled and are read at the nearest-neighbour
// source frame of F.interpolate(mode='nearest') to T FRAMES (the resize comes before the patchify, dit.py:170-173,198), computed per frame
// t = t' P + p: src = min(floor(t * scale), Tc - 1) with the fp32 scale = (float)Tc / T; workgroups behind the token chunks copy the Pl
// prepared prepend rows.
constexpr int IPP_TT = 8;
template <bool EXTRA, int PT>
__global__ __launch_bounds__(256) void input_proj_patch_kernel(const float* __restrict__ x, const float* __restrict__ WeffT,
                                                               float* __restrict__ X, int xB, int C, int Prt, int Tt, int S, int D, float xscale,
                                                               const float* __restrict__ cc, int Cc, int Tc, float cscale,
                                                               const float* __restrict__ prep, int Pl) {
    const int P = PT ? PT : Prt;
    const int T = Tt * P;
    const int b = blockIdx.z;
    const int n = blockIdx.y * 256 + threadIdx.x;
    if constexpr (EXTRA) {
        const int nt = (Tt + IPP_TT - 1) / IPP_TT;
        if ((int)blockIdx.x >= nt) {        // prepend rows
            const int p0 = (blockIdx.x - nt) * IPP_TT;
            if (n >= D) return;
#pragma unroll
            for (int pp = 0; pp < IPP_TT; ++pp)
                if (p0 + pp < Pl) X[((size_t)b * S + p0 + pp) * D + n] = prep[((size_t)b * Pl + p0 + pp) * D + n];
            return;
        }
    }
    const int t0 = blockIdx.x * IPP_TT;      // first token of the chunk
    if (n >= D) return;
    const float* __restrict__ xb = x + (size_t)(b % xB) * C * T;      // wave-uniform
    float acc[IPP_TT];
#pragma unroll
    for (int tt = 0; tt < IPP_TT; ++tt) acc[tt] = 0.f;
    if (t0 + IPP_TT <= Tt) {
        const float* __restrict__ xc = xb + (size_t)t0 * P;
        for (int c = 0; c < C; ++c) {
            const float* __restrict__ xr = xc + (size_t)c * T;
            const float* __restrict__ wr = WeffT + (size_t)c * P * D + n;
            if constexpr (PT != 0) {
#pragma unroll
                for (int p = 0; p < PT; ++p) {
                    const float w = wr[(size_t)p * D];
#pragma unroll
                    for (int tt = 0; tt < IPP_TT; ++tt) acc[tt] += w * xr[tt * PT + p];
                }
            } else {
                for (int p = 0; p < P; ++p) {
                    const float w = wr[(size_t)p * D];
#pragma unroll
                    for (int tt = 0; tt < IPP_TT; ++tt) acc[tt] += w * xr[tt * P + p];
                }
            }
        }
    } else {          // last chunk of a sequence whose token count is not a multiple of IPP_TT: tokens behind the end re-read the last one
        int fo[IPP_TT];
#pragma unroll
        for (int tt = 0; tt < IPP_TT; ++tt) fo[tt] = (t0 + tt < Tt ? t0 + tt : Tt - 1) * P;
        for (int c = 0; c < C; ++c) {
            const float* __restrict__ xr = xb + (size_t)c * T;
            const float* __restrict__ wr = WeffT + (size_t)c * P * D + n;
            for (int p = 0; p < P; ++p) {
                const float w = wr[(size_t)p * D];
#pragma unroll
                for (int tt = 0; tt < IPP_TT; ++tt) acc[tt] += w * xr[fo[tt] + p];
            }
        }
    }
    if constexpr (EXTRA) {
        float accc[IPP_TT];
#pragma unroll
        for (int tt = 0; tt < IPP_TT; ++tt) accc[tt] = 0.f;
        const float* __restrict__ cb = cc + (size_t)b * Cc * Tc;       // wave-uniform
        for (int p = 0; p < P; ++p) {      // p outside: the IPP_TT source frames of this p once for all Cc channels
            int src[IPP_TT];
#pragma unroll
            for (int tt = 0; tt < IPP_TT; ++tt) {
                const int t = (t0 + tt < Tt ? t0 + tt : Tt - 1) * P + p;
                const int si = Tc == T ? t : (int)floorf((float)t * cscale);
                src[tt] = si < Tc - 1 ? si : Tc - 1;
            }
            for (int c = 0; c < Cc; ++c) {
                const float w = WeffT[((size_t)(C + c) * P + p) * D + n];
                const float* __restrict__ cr = cb + (size_t)c * Tc;
#pragma unroll
                for (int tt = 0; tt < IPP_TT; ++tt) accc[tt] += w * cr[src[tt]];
            }
        }
#pragma unroll
        for (int tt = 0; tt < IPP_TT; ++tt)
            if (t0 + tt < Tt) X[((size_t)b * S + (S - Tt) + t0 + tt) * D + n] = acc[tt] * xscale + accc[tt];
        return;
    }
#pragma unroll
    for (int tt = 0; tt < IPP_TT; ++tt)
        if (t0 + tt < Tt) X[((size_t)b * S + (S - Tt) + t0 + tt) * D + n] = acc[tt] * xscale;
}

// out[b][c][t' P + p] = sum_n WeffT[n][c P + p] * X[b, (S-T') + t', n].  The scheme of output_proj_kernel (dit_glue.hip): OPP_TOK token rows of
// X staged in LDS once, the eight waves split the D input channels, lane = (4 output columns, 4 consecutive input channels) with 16-byte
// weight loads, partial sums folded through two lane exchanges and LDS.  The N = C P output columns go in groups of 64 on blockIdx.y (a
// group re-stages its rows: they come from L2).  The last group may hold fewer than 64 columns: its lanes beyond N recompute the group's
// first four.  The writing threads run over (channel, token, p) with p fastest, so that each channel receives OPP_TOK * P consecutive
// floats; a channel whose P columns straddle two groups (P no divisor of 64) is written by both, each its own columns.
constexpr int OPP_TOK = 8;
__global__ __launch_bounds__(512) void output_proj_patch_kernel(const float* __restrict__ X, const float* __restrict__ WeffT,
                                                                float* __restrict__ out, int Bf, int C, int P, int Tt, int S, int D) {
    extern __shared__ __attribute__((aligned(16))) char smem_opp[];
    float* xs = reinterpret_cast<float*>(smem_opp);         // [OPP_TOK][D]
    float* red = xs + (size_t)OPP_TOK * D;                  // [8 waves][64 columns][OPP_TOK]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int N = C * P;
    const int j0 = blockIdx.y * 64;                         // first column of the group (j0 < N)
    const int tok0 = blockIdx.x * OPP_TOK;                  // token index b * T' + t'
    const int total = Bf * Tt;
    for (int i = threadIdx.x; i < OPP_TOK * (D / 4); i += 512) {
        const int tk = i / (D / 4), q = i - tk * (D / 4);
        int row = tok0 + tk;
        row = row < total ? row : total - 1;
        const int b = row / Tt, t = row - b * Tt;
        reinterpret_cast<float4*>(xs + (size_t)tk * D)[q] = reinterpret_cast<const float4*>(X + ((size_t)b * S + (S - Tt) + t) * D)[q];
    }
    __syncthreads();
    const int cg = lane & 15, ns = lane >> 4;               // columns j0 + 4cg .. +3, input channels n0 + 4ns .. +3 of a step
    const int col0 = j0 + 4 * cg < N ? j0 + 4 * cg : j0;    // (N % 4 == 0 is checked by the launcher)
    float acc[4][OPP_TOK];
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int tk = 0; tk < OPP_TOK; ++tk) acc[e][tk] = 0.f;
    const int nq = D / 8;                                   // input channels per wave (D % 128 == 0: a multiple of 16)
    const float* wp = WeffT + (size_t)(wave * nq + 4 * ns) * N + col0;
    float4 w[4], wn[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) w[u] = *reinterpret_cast<const float4*>(wp + (size_t)u * N);
    for (int n0 = 0; n0 < nq; n0 += 16) {
        if (n0 + 16 < nq) {
#pragma unroll
            for (int u = 0; u < 4; ++u) wn[u] = *reinterpret_cast<const float4*>(wp + (size_t)(n0 + 16 + u) * N);
        }
        const float* xrow = xs + wave * nq + n0 + 4 * ns;
#pragma unroll
        for (int tk = 0; tk < OPP_TOK; ++tk) {
            const float4 xv = *reinterpret_cast<const float4*>(xrow + (size_t)tk * D);
            acc[0][tk] += (w[0].x * xv.x + w[1].x * xv.y) + (w[2].x * xv.z + w[3].x * xv.w);
            acc[1][tk] += (w[0].y * xv.x + w[1].y * xv.y) + (w[2].y * xv.z + w[3].y * xv.w);
            acc[2][tk] += (w[0].z * xv.x + w[1].z * xv.y) + (w[2].z * xv.z + w[3].z * xv.w);
            acc[3][tk] += (w[0].w * xv.x + w[1].w * xv.y) + (w[2].w * xv.z + w[3].w * xv.w);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) w[u] = wn[u];
    }
    // fold the four input-channel slices of the wave (lanes l, l+16, l+32, l+48), then the eight waves through LDS
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int tk = 0; tk < OPP_TOK; ++tk) {
            float v = acc[e][tk];
            v += __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(v), 0x401F));      // lane ^ 16
            unsigned a = __float_as_uint(v), bq = a;
            half_swap(a, bq);                                                                  // lane ^ 32
            v = __uint_as_float(a) + __uint_as_float(bq);
            if (lane < 16) red[((size_t)wave * 64 + 4 * cg + e) * OPP_TOK + tk] = v;
        }
    __syncthreads();
    const int jend = j0 + 64 < N ? j0 + 64 : N;             // columns [j0, jend) are this group's
    const int cfirst = j0 / P, nch = (jend - 1) / P - cfirst + 1;
    for (int i = threadIdx.x; i < nch * OPP_TOK * P; i += 512) {
        const int cl = i / (OPP_TOK * P), r = i - cl * (OPP_TOK * P);
        const int tk = r / P, p = r - tk * P;               // consecutive threads: the P frames of a token, then the next token of the channel
        const int ch = cfirst + cl, j = ch * P + p;
        const int row = tok0 + tk;
        if (j >= j0 && j < jend && row < total) {
            float v = 0.f;
#pragma unroll
            for (int wv = 0; wv < 8; ++wv) v += red[((size_t)wv * 64 + (j - j0)) * OPP_TOK + tk];
            const int b = row / Tt, t = row - b * Tt;
            out[((size_t)b * C + ch) * ((size_t)Tt * P) + (size_t)t * P + p] = v;
        }
    }
}

template <bool EXTRA>
void launch_input_patch(dim3 grid, hipStream_t s, const float* x, const float* Weff, float* X, int xB, int C, int P, int Tt, int S, int D, float xscale,
                        const float* cc, int Cc, int Tc, float cscale, const float* prep, int Pl) {
#define SAT_IPP(PT) hipLaunchKernelGGL((input_proj_patch_kernel<EXTRA, PT>), grid, dim3(256), 0, s, x, Weff, X, xB, C, P, Tt, S, D, xscale, cc, Cc, Tc, cscale, prep, Pl)
    switch (P) {
        case 2: SAT_IPP(2); break;
        case 4: SAT_IPP(4); break;
        case 8: SAT_IPP(8); break;
        default: SAT_IPP(0); break;
    }
#undef SAT_IPP
}

// what both launchers check of the patch geometry (the limits of include/sat_hip.h, sat_dit_plan_set_patch)
int check_patch(const char* who, int C, int Ci, int P, int T) {
    SAT_CHECK_ARG(P >= 2, SAT_E_INVALID, "%s: patch_size %d (the kernels of dit_glue.hip run patch_size 1)", who, P);
    SAT_CHECK_ARG(T % P == 0, SAT_E_INVALID, "%s: t_len %d is not a multiple of patch_size %d", who, T, P);
    SAT_CHECK_ARG(C <= 64 && C % 4 == 0 && Ci <= 256, SAT_E_UNSUPPORTED, "%s: io_channels %d (multiple of 4, <= 64), with concat %d (<= 256)", who, C, Ci);
    SAT_CHECK_ARG((int64_t)C * P <= 512, SAT_E_UNSUPPORTED, "%s: io_channels * patch_size = %lld exceeds 512", who, (long long)C * P);
    SAT_CHECK_ARG((int64_t)Ci * P <= 1024, SAT_E_UNSUPPORTED, "%s: (io_channels + input_concat_dim) * patch_size = %lld exceeds 1024", who, (long long)Ci * P);
    return 0;
}

}  // namespace

int glue_fold_in_patch(const float* Win, const float* Wpre, float* Weff, int D, int Ci, int P, hipStream_t s) {
    SAT_CHECK_ARG(Win && Wpre && Weff && D > 0 && Ci > 0 && P > 0 && (int64_t)D * Ci * P < (1ll << 31), SAT_E_INVALID, "fold_in_patch: bad arguments");
    hipLaunchKernelGGL(fold_in_patch_kernel, dim3(cdiv(D * Ci * P, 256)), dim3(256), 0, s, Win, Wpre, Weff, D, Ci, P);
    SAT_LAUNCH_CHECK();
    return 0;
}
int glue_fold_out_patch(const float* Wout, const float* Wpost, float* Weff, int D, int C, int P, hipStream_t s) {
    SAT_CHECK_ARG(Wout && Wpost && Weff && D > 0 && C > 0 && P > 0 && (int64_t)D * C * P < (1ll << 31), SAT_E_INVALID, "fold_out_patch: bad arguments");
    hipLaunchKernelGGL(fold_out_patch_kernel, dim3(cdiv(D * C * P, 256)), dim3(256), 0, s, Wout, Wpost, Weff, D, C, P);
    SAT_LAUNCH_CHECK();
    return 0;
}

int glue_input_proj_patch(const float* x, const float* Weff, float* X, int Bf, int xB, int C, int P, int T, int S, int D, float xscale,
                          const float* concat, int Cc, int Tc, const float* prep, int Pl, hipStream_t s) {
    SAT_CHECK_ARG(x && Weff && X && Bf > 0 && xB > 0 && C > 0 && T > 0 && D > 0 && Bf <= 65535 && Cc >= 0 && Pl >= 0, SAT_E_INVALID,
                  "input_proj_patch: bad arguments (Bf %d, xB %d, C %d, T %d, S %d, D %d, Cc %d)", Bf, xB, C, T, S, D, Cc);
    SAT_TRY(check_patch("input_proj_patch", C, C + Cc, P, T));
    const int Tt = T / P;
    SAT_CHECK_ARG(S >= Tt + Pl && (Cc == 0 || (concat && Tc > 0)) && (Pl == 0 || prep), SAT_E_INVALID,
                  "input_proj_patch: bad extra conditioning (S %d, prepend %d, tokens %d, Cc %d, Tc %d)", S, Pl, Tt, Cc, Tc);
    const float cscale = Cc ? (float)Tc / (float)T : 1.0f;      // F.interpolate(mode='nearest') to T frames: its fp32 scale
    if (Cc > 0 || Pl > 0)
        launch_input_patch<true>(dim3(cdiv(Tt, IPP_TT) + cdiv(Pl, IPP_TT), cdiv(D, 256), Bf), s, x, Weff, X, xB, C, P, Tt, S, D, xscale, concat, Cc,
                                 Cc ? Tc : 1, cscale, prep, Pl);
    else
        launch_input_patch<false>(dim3(cdiv(Tt, IPP_TT), cdiv(D, 256), Bf), s, x, Weff, X, xB, C, P, Tt, S, D, xscale, nullptr, 0, 1, 1.0f, nullptr, 0);
    SAT_LAUNCH_CHECK();
    return 0;
}

int glue_output_proj_patch(const float* X, const float* WeffT, float* out, int Bf, int C, int P, int T, int S, int D, hipStream_t s) {
    SAT_CHECK_ARG(X && WeffT && out && Bf > 0 && C > 0 && T > 0 && D > 0, SAT_E_INVALID,
                  "output_proj_patch: bad arguments (Bf %d, C %d, T %d, S %d, D %d)", Bf, C, T, S, D);
    SAT_TRY(check_patch("output_proj_patch", C, C, P, T));
    const int Tt = T / P;
    SAT_CHECK_ARG(S >= Tt && (int64_t)Bf * Tt < (1ll << 31) - OPP_TOK, SAT_E_INVALID, "output_proj_patch: bad arguments (Bf %d, tokens %d, S %d)", Bf, Tt, S);
    SAT_CHECK_ARG((((uintptr_t)X | (uintptr_t)WeffT) & 15) == 0, SAT_E_INVALID, "output_proj_patch: X and the weight must be 16-byte aligned");
    const int lds = (OPP_TOK * D + 8 * OPP_TOK * 64) * 4;
    SAT_CHECK_ARG(lds <= 160 * 1024 && D % 128 == 0, SAT_E_UNSUPPORTED, "output_proj_patch: embed_dim %d unsupported (multiple of 128, <= 2048)", D);
    SAT_TRY(sat_ensure_dynamic_lds(reinterpret_cast<const void*>(output_proj_patch_kernel), 160 * 1024));
    hipLaunchKernelGGL(output_proj_patch_kernel, dim3(cdiv((int64_t)Bf * Tt, OPP_TOK), cdiv(C * P, 64)), dim3(512), lds, s, X, WeffT, out, Bf, C, P, Tt, S, D);
    SAT_LAUNCH_CHECK();
    return 0;
}
