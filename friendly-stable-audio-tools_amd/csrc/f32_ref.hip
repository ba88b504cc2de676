// fp32 verification path of the DiT ("gemm_dtype = fp32x", sat_dit_cfg.fp8_gemm == 2): the same plan, data flow, index
// arithmetic, RoPE table, prepend token, GQA cross-attention and CFG batching as the bf16 path, but every contraction takes
// fp32 operands on the exact fp32 MFMA (v_mfma_f32_32x32x2_f32 = fmaf chains) and q / k / v / P stay fp32.  NOT a fast path
// (the f32 MFMA runs at 1/16 of the bf16 rate): it exists to show that what separates the bf16 path from the reference
// (3.5e-3 at full size) is operand rounding only -- this path meets north_star's 1e-3 against the reference's own outputs
// (tests/test_gpu_models.py: test_fp32x_mode_vs_reference_golden).
// Replaces the same reference code as gemm_bf16.hip / attention.hip / layernorm.hip (models/transformer.py:188-206, 158-183,
// 222-235, 270, 311-319, 496-536).
#include "attn_causal.h"
#include "sat_common.h"

namespace {

typedef float f32x2 __attribute__((ext_vector_type(2)));

// C[M,N] (+)= A[M,K] . W[N,K]^T (+ bias) (* gate): 128x128 tile, 4 waves (2x2) of 64x64, K-step 16, register-staged double
// buffer.  LDS rows hold 16 floats padded to 20 (80 B): conflict-free ds_read_b128.  A lane half h takes k = 8h .. 8h+7 of the
// K-step for BOTH operands (any k permutation shared by A and W leaves the dot product unchanged).
constexpr int F_BM = 128, F_BN = 128, F_BK = 16, F_LD = 20;

__global__ __launch_bounds__(256) void gemm_f32_kernel(const float* __restrict__ A, const float* __restrict__ W,
                                                       const float* __restrict__ bias, float* __restrict__ C, int M, int N, int K,
                                                       int ldc, int accumulate, const float* __restrict__ gate, int gate_rows,
                                                       int gate_ld) {
    __shared__ __attribute__((aligned(16))) float sA[2][F_BM * F_LD];
    __shared__ __attribute__((aligned(16))) float sW[2][F_BN * F_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, half = lane >> 5, l31 = lane & 31;
    const int tiles_n = (N + F_BN - 1) / F_BN;
    const int tm = blockIdx.x / tiles_n, tn = blockIdx.x - tm * tiles_n;
    const int m0 = tm * F_BM, n0 = tn * F_BN;

    // staging: 128 rows x 4 float4 per operand per K-step = 512 float4, two per thread
    int srow[2], sc4[2];
    const float *ap[2], *wp[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int id = i * 256 + tid;
        srow[i] = id >> 2;
        sc4[i] = id & 3;
        int gm = m0 + srow[i];
        gm = gm < M ? gm : M - 1;
        int gn = n0 + srow[i];
        gn = gn < N ? gn : N - 1;
        ap[i] = A + (size_t)gm * K + sc4[i] * 4;
        wp[i] = W + (size_t)gn * K + sc4[i] * 4;
    }
    f32x4 ra[2], rw[2];
    auto gload = [&](int kt) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            ra[i] = *reinterpret_cast<const f32x4*>(ap[i] + kt * F_BK);
            rw[i] = *reinterpret_cast<const f32x4*>(wp[i] + kt * F_BK);
        }
    };
    auto lstore = [&](int st) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            *reinterpret_cast<f32x4*>(&sA[st][srow[i] * F_LD + sc4[i] * 4]) = ra[i];
            *reinterpret_cast<f32x4*>(&sW[st][srow[i] * F_LD + sc4[i] * 4]) = rw[i];
        }
    };
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    auto compute = [&](int st) {
        f32x4 af[2][2], wf[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                af[i][q] = *reinterpret_cast<const f32x4*>(&sA[st][(wm * 64 + i * 32 + l31) * F_LD + half * 8 + q * 4]);
                wf[i][q] = *reinterpret_cast<const f32x4*>(&sW[st][(wn * 64 + i * 32 + l31) * F_LD + half * 8 + q * 4]);
            }
#pragma unroll
        for (int t = 0; t < 8; ++t)
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i][t >> 2][t & 3], wf[j][t >> 2][t & 3], acc[i][j], 0, 0, 0);
    };
    const int nk = K / F_BK;
    gload(0);
    lstore(0);
    __syncthreads();
    for (int kt = 0; kt < nk - 1; ++kt) {
        gload(kt + 1);
        compute(kt & 1);
        lstore((kt + 1) & 1);
        __syncthreads();
    }
    compute((nk - 1) & 1);
    // acc[i][j][r]: row = i*32 + (r&3) + 8*(r>>2) + 4*half, col = j*32 + l31
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int n = n0 + wn * 64 + j * 32 + l31;
            if (n >= N) continue;
            const float bv = bias ? bias[n] : 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                if (m >= M) continue;
                float v = acc[i][j][r] + bv;
                if (gate) v *= gate[(size_t)(m / gate_rows) * gate_ld + n];
                float* cp = C + (size_t)m * ldc + n;
                *cp = accumulate ? *cp + v : v;
            }
        }
}

// LayerNorm -> fp32 (one wave per row, any d % 4 == 0; optional adaLN modulation)
__global__ __launch_bounds__(256) void layernorm_f32_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, float* __restrict__ y, int m, int d,
                                                            const float* __restrict__ sc, const float* __restrict__ sh, int rps, int ld,
                                                            float eps) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= m) return;
    const float* xr = x + (size_t)row * d;
    float s = 0.f;
    for (int i = lane; i < d; i += 64) s += xr[i];
    const float mean = wave_sum(s) / (float)d;
    float q = 0.f;
    for (int i = lane; i < d; i += 64) {
        const float a = xr[i] - mean;
        q += a * a;
    }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)d + eps);
    const float* scr = sc ? sc + (size_t)(row / rps) * ld : nullptr;
    const float* shr = sc ? sh + (size_t)(row / rps) * ld : nullptr;
    for (int i = lane; i < d; i += 64) {
        float r = (xr[i] - mean) * rstd * gamma[i] + (beta ? beta[i] : 0.f);
        if (scr) r = r * scr[i] + shr[i];
        y[(size_t)row * d + i] = r;
    }
}

// [M, parts * H * 64] -> per part [B, H, S, 64] fp32; parts with rope: partial rotary on d < 32 (pairs d, d + 16); parts in norm_mask:
// L2-normalised per head first (qk_norm, transformer.py:433-436; F.normalize: x / max(|x|, 1e-12)).  One wave = the 64 channels of one head row.
__global__ __launch_bounds__(256) void split_heads_f32_kernel(const float* __restrict__ src, float* __restrict__ d0, float* __restrict__ d1,
                                                              float* __restrict__ d2, int M, int S, int parts, int H, int rope_mask,
                                                              const float* __restrict__ rope_cos, const float* __restrict__ rope_sin, int norm_mask) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t total = (int64_t)M * parts * H * 64;
    if (idx >= total) return;
    const int d = (int)(idx & 63);
    int64_t t = idx >> 6;
    const int h = (int)(t % H);
    t /= H;
    const int part = (int)(t % parts);
    const int m = (int)(t / parts);
    const int b = m / S, s = m - b * S;
    const float* row = src + (size_t)m * parts * H * 64 + (size_t)part * H * 64 + h * 64;
    float v = row[d];
    if (((rope_mask >> part) & 1) && d < 32) {
        const float cs = rope_cos[(size_t)s * 16 + (d & 15)], sn = rope_sin[(size_t)s * 16 + (d & 15)];
        v = d < 16 ? v * cs - row[d + 16] * sn : v * cs + row[d - 16] * sn;
    }
    // (the rotation is orthogonal: the norm of the rotated row is the norm of the row; total % 64 == 0, so whole waves get here)
    if ((norm_mask >> part) & 1) v /= fmaxf(sqrtf(wave_sum(v * v)), 1e-12f);
    float* dst = part == 0 ? d0 : (part == 1 ? d1 : d2);
    dst[(((size_t)b * H + h) * S + s) * 64 + d] = v;
}

// The same for heads of W channels that do not fill a wave (32, 96): [M, parts * H * W] -> per part [B, H, S, W]; rotation of the first 2 RH
// channels in pairs (d, d + RH) with RH = sat_rope_pairs(W) angles per position (RotaryEmbedding(max(W / 2, 32))).  One lane per element; a
// lane of a normalised part sums the squares of its head row itself (the verification path is no fast path), and normalises BEFORE the
// rotation as the reference does
__global__ __launch_bounds__(256) void split_heads_f32_w_kernel(const float* __restrict__ src, float* __restrict__ d0, float* __restrict__ d1,
                                                                float* __restrict__ d2, int M, int S, int parts, int H, int W, int RH, int rope_mask,
                                                                const float* __restrict__ rope_cos, const float* __restrict__ rope_sin, int norm_mask) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t total = (int64_t)M * parts * H * W;
    if (idx >= total) return;
    const int d = (int)(idx % W);
    int64_t t = idx / W;
    const int h = (int)(t % H);
    t /= H;
    const int part = (int)(t % parts);
    const int m = (int)(t / parts);
    const int b = m / S, s = m - b * S;
    const float* row = src + (size_t)m * parts * H * W + (size_t)part * H * W + (size_t)h * W;
    float inv = 1.0f;
    if ((norm_mask >> part) & 1) {
        float ss = 0.f;
        for (int c = 0; c < W; ++c) ss = fmaf(row[c], row[c], ss);
        inv = 1.0f / fmaxf(sqrtf(ss), 1e-12f);
    }
    float v = row[d] * inv;
    if (((rope_mask >> part) & 1) && d < 2 * RH) {
        const int j = d < RH ? d : d - RH;
        const float cs = rope_cos[(size_t)s * RH + j], sn = rope_sin[(size_t)s * RH + j];
        v = d < RH ? v * cs - row[d + RH] * inv * sn : v * cs + row[d - RH] * inv * sn;
    }
    float* dst = part == 0 ? d0 : (part == 1 ? d1 : d2);
    dst[(((size_t)b * H + h) * S + s) * W + d] = v;
}

// x, gate = chunk(2); x * silu(gate)  (transformer.py:232-235), fp32
__global__ __launch_bounds__(256) void swiglu_f32_kernel(const float* __restrict__ hg, float* __restrict__ h, int64_t M, int inner) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= M * inner) return;
    const int64_t m = idx / inner;
    const int c = (int)(idx - m * inner);
    const float v = hg[m * 2 * inner + c], g = hg[m * 2 * inner + inner + c];
    h[idx] = v * (g / (1.0f + expf(-g)));
}

// softmax(q k^T / sqrt(W)) v in fp32, one query per lane (q and the output row in registers), K / V rows are wave-uniform loads.
// Online softmax over chunks of 8 keys.  q [B,H,Sq,W], k / v [B,KVH,Sk,W] -> out [B*Sq, H*W].  W = 64 is the kernel the 64-channel plans
// have always run (scale 1/8); 32 and 96 are the widths of the staged route (attention_hdw.hip).  CAUSAL (Sq == Sk): the key loop ends with the
// chunk that holds the diagonal of the wave's last query (attn_causal.h at 8-key tiles, no key shift) and a lane masks the keys j > its query;
// key 0 is in the first chunk and visible to everybody, so the running maximum is finite from there on
template <int W, bool CAUSAL = false>
__global__ __launch_bounds__(64) void attention_f32_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                           const float* __restrict__ v, float* __restrict__ out, int H, int KVH, int Sq,
                                                           int Sk) {
    const int b = blockIdx.z, h = blockIdx.y;
    const int kvh = h / (H / KVH);
    const int qi = blockIdx.x * 64 + threadIdx.x;
    const int qc = qi < Sq ? qi : Sq - 1;
    constexpr float SCALE = W == 64 ? 0.125f : W == 32 ? 0.17677669529663687f : 0.10206207261596575f;      // 1 / sqrt(W)
    float qr[W], o[W];
    const f32x4* qp = reinterpret_cast<const f32x4*>(q + (((size_t)b * H + h) * Sq + qc) * W);
#pragma unroll
    for (int t = 0; t < W / 4; ++t) {
        const f32x4 x = qp[t];
        qr[4 * t] = x[0] * SCALE;
        qr[4 * t + 1] = x[1] * SCALE;
        qr[4 * t + 2] = x[2] * SCALE;
        qr[4 * t + 3] = x[3] * SCALE;
    }
#pragma unroll
    for (int d = 0; d < W; ++d) o[d] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;
    const float* kb = k + ((size_t)b * KVH + kvh) * Sk * W;
    const float* vb = v + ((size_t)b * KVH + kvh) * Sk * W;
    const int j_end = CAUSAL ? attnc::tiles_walked(blockIdx.x * 64, 64, 0, Sk, 8) * 8 : Sk;
    for (int j0 = 0; j0 < j_end; j0 += 8) {
        float sc[8];
        float mx = m_run;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int j = j0 + u;
            float s = -INFINITY;
            if (j < Sk) {
                const float* kr = kb + (size_t)j * W;
                s = 0.f;
#pragma unroll
                for (int d = 0; d < W; ++d) s = fmaf(qr[d], kr[d], s);
                if (CAUSAL && j > qc) s = -INFINITY;
            }
            sc[u] = s;
            mx = fmaxf(mx, s);
        }
        const float alpha = expf(m_run - mx);
        m_run = mx;
        l_run *= alpha;
#pragma unroll
        for (int d = 0; d < W; ++d) o[d] *= alpha;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int j = j0 + u;
            if (j < Sk) {
                const float p = expf(sc[u] - mx);
                l_run += p;
                const float* vr = vb + (size_t)j * W;
#pragma unroll
                for (int d = 0; d < W; ++d) o[d] = fmaf(p, vr[d], o[d]);
            }
        }
    }
    if (qi < Sq) {
        const float inv = 1.0f / l_run;
        f32x4* op = reinterpret_cast<f32x4*>(out + ((size_t)b * Sq + qi) * ((size_t)H * W) + h * W);
#pragma unroll
        for (int t = 0; t < W / 4; ++t) op[t] = f32x4{o[4 * t] * inv, o[4 * t + 1] * inv, o[4 * t + 2] * inv, o[4 * t + 3] * inv};
    }
}

}  // namespace

int sat_launch_gemm_f32(const float* A, const float* W, const float* bias, float* C, int M, int N, int K, int ldc, int accumulate,
                        const float* gate, int gate_rows, int gate_ld, hipStream_t s) {
    SAT_CHECK_ARG(A && W && C && M > 0 && N > 0 && K > 0 && ldc >= N && (!gate || gate_ld >= N), SAT_E_INVALID, "gemm_f32: bad arguments");
    SAT_CHECK_ARG((((uintptr_t)A | (uintptr_t)W) & 15) == 0, SAT_E_INVALID, "gemm_f32: operands must be 16-byte aligned");
    SAT_CHECK_ARG(K % F_BK == 0, SAT_E_UNSUPPORTED, "gemm_f32: K=%d must be a multiple of %d", K, F_BK);
    const int tiles = cdiv(M, F_BM) * cdiv(N, F_BN);
    hipLaunchKernelGGL(gemm_f32_kernel, dim3(tiles), dim3(256), 0, s, A, W, bias, C, M, N, K, ldc, accumulate, gate, gate_rows > 0 ? gate_rows : 1,
                       gate_ld);
    SAT_LAUNCH_CHECK();
    return 0;
}

int sat_launch_layernorm_f32(const float* x, const float* gamma, const float* beta, float* y, int m, int d, const float* sc,
                             const float* sh, int rps, int ld, hipStream_t s, float eps) {
    SAT_CHECK_ARG(x && gamma && y && m > 0 && d > 0 && (!sc || (sh && ld >= d)), SAT_E_INVALID, "layernorm_f32: bad args");
    hipLaunchKernelGGL(layernorm_f32_kernel, dim3(cdiv(m, 4)), dim3(256), 0, s, x, gamma, beta, y, m, d, sc, sh, rps > 0 ? rps : 1, ld, eps);
    SAT_LAUNCH_CHECK();
    return 0;
}

int sat_launch_split_heads_f32(const float* src, float* d0, float* d1, float* d2, int M, int S, int parts, int H, int rope_mask,
                               const float* rope_cos, const float* rope_sin, hipStream_t s, int norm_mask) {
    SAT_CHECK_ARG(src && d0 && parts >= 1 && parts <= 3 && (rope_mask == 0 || (rope_cos && rope_sin)), SAT_E_INVALID, "split_heads_f32: bad args");
    SAT_CHECK_ARG(M > 0 && S > 0 && M % S == 0 && H > 0 && (parts < 2 || d1) && (parts < 3 || d2) && rope_mask >= 0 && norm_mask >= 0 &&
                      (rope_mask >> parts) == 0 && (norm_mask >> parts) == 0,
                  SAT_E_INVALID, "split_heads_f32: bad dims (M %d, S %d, H %d, parts %d, rope_mask %d, norm_mask %d)", M, S, H, parts, rope_mask,
                  norm_mask);
    const int64_t total = (int64_t)M * parts * H * 64;
    hipLaunchKernelGGL(split_heads_f32_kernel, dim3(cdiv(total, 256)), dim3(256), 0, s, src, d0, d1, d2, M, S, parts, H, rope_mask, rope_cos,
                       rope_sin, norm_mask);
    SAT_LAUNCH_CHECK();
    return 0;
}

int sat_launch_swiglu_f32(const float* hg, float* h, int64_t M, int inner, hipStream_t s) {
    SAT_CHECK_ARG(hg && h && M > 0 && inner > 0, SAT_E_INVALID, "swiglu_f32: bad args");
    hipLaunchKernelGGL(swiglu_f32_kernel, dim3(cdiv(M * inner, 256)), dim3(256), 0, s, hg, h, M, inner);
    SAT_LAUNCH_CHECK();
    return 0;
}

int sat_launch_attention_f32(const float* q, const float* k, const float* v, float* out, int b, int h, int kvh, int sq, int sk,
                             hipStream_t s) {
    SAT_CHECK_ARG(q && k && v && out && b > 0 && h > 0 && kvh > 0 && h % kvh == 0 && sq > 0 && sk > 0, SAT_E_INVALID, "attention_f32: bad args");
    SAT_CHECK_ARG((((uintptr_t)q | (uintptr_t)out) & 15) == 0, SAT_E_INVALID, "attention_f32: q and out must be 16-byte aligned");
    SAT_CHECK_ARG(h <= 65535 && b <= 65535, SAT_E_UNSUPPORTED, "attention_f32: %d heads / %d sequences exceed the grid", h, b);
    hipLaunchKernelGGL(attention_f32_kernel<64>, dim3(cdiv(sq, 64), h, b), dim3(64), 0, s, q, k, v, out, h, kvh, sq, sk);
    SAT_LAUNCH_CHECK();
    return 0;
}

int sat_launch_split_heads_f32_w(const float* src, float* d0, float* d1, float* d2, int M, int S, int parts, int H, int head_dim, int rope_mask,
                                 const float* rope_cos, const float* rope_sin, hipStream_t s, int norm_mask) {
    if (head_dim == 64) return sat_launch_split_heads_f32(src, d0, d1, d2, M, S, parts, H, rope_mask, rope_cos, rope_sin, s, norm_mask);
    SAT_CHECK_ARG(head_dim == 32 || head_dim == 96, SAT_E_UNSUPPORTED, "split_heads_f32: dim_heads %d (built for 32, 64 and 96)", head_dim);
    SAT_CHECK_ARG(src && d0 && parts >= 1 && parts <= 3 && (rope_mask == 0 || (rope_cos && rope_sin)), SAT_E_INVALID, "split_heads_f32: bad args");
    SAT_CHECK_ARG(M > 0 && S > 0 && M % S == 0 && H > 0 && (parts < 2 || d1) && (parts < 3 || d2) && rope_mask >= 0 && norm_mask >= 0 &&
                      (rope_mask >> parts) == 0 && (norm_mask >> parts) == 0,
                  SAT_E_INVALID, "split_heads_f32: bad dims (M %d, S %d, H %d, parts %d, rope_mask %d, norm_mask %d)", M, S, H, parts, rope_mask,
                  norm_mask);
    const int64_t total = (int64_t)M * parts * H * head_dim;
    hipLaunchKernelGGL(split_heads_f32_w_kernel, dim3(cdiv(total, 256)), dim3(256), 0, s, src, d0, d1, d2, M, S, parts, H, head_dim,
                       sat_rope_pairs(head_dim), rope_mask, rope_cos, rope_sin, norm_mask);
    SAT_LAUNCH_CHECK();
    return 0;
}

int sat_launch_attention_f32_w(const float* q, const float* k, const float* v, float* out, int b, int h, int kvh, int head_dim, int sq, int sk,
                               hipStream_t s) {
    if (head_dim == 64) return sat_launch_attention_f32(q, k, v, out, b, h, kvh, sq, sk, s);
    SAT_CHECK_ARG(head_dim == 32 || head_dim == 96, SAT_E_UNSUPPORTED, "attention_f32: dim_heads %d (built for 32, 64 and 96)", head_dim);
    SAT_CHECK_ARG(q && k && v && out && b > 0 && h > 0 && kvh > 0 && h % kvh == 0 && sq > 0 && sk > 0, SAT_E_INVALID, "attention_f32: bad args");
    SAT_CHECK_ARG((((uintptr_t)q | (uintptr_t)out) & 15) == 0, SAT_E_INVALID, "attention_f32: q and out must be 16-byte aligned");
    SAT_CHECK_ARG(h <= 65535 && b <= 65535, SAT_E_UNSUPPORTED, "attention_f32: %d heads / %d sequences exceed the grid", h, b);
    if (head_dim == 32) hipLaunchKernelGGL(attention_f32_kernel<32>, dim3(cdiv(sq, 64), h, b), dim3(64), 0, s, q, k, v, out, h, kvh, sq, sk);
    else hipLaunchKernelGGL(attention_f32_kernel<96>, dim3(cdiv(sq, 64), h, b), dim3(64), 0, s, q, k, v, out, h, kvh, sq, sk);
    SAT_LAUNCH_CHECK();
    return 0;
}

// Causal self-attention in fp32 (sq == sk == s_len) at any built head width
int sat_launch_attention_f32_causal(const float* q, const float* k, const float* v, float* out, int b, int h, int kvh, int head_dim, int s_len,
                                    hipStream_t s) {
    SAT_CHECK_ARG(head_dim == 32 || head_dim == 64 || head_dim == 96, SAT_E_UNSUPPORTED, "attention_f32 (causal): dim_heads %d (built for 32, 64 and 96)",
                  head_dim);
    SAT_CHECK_ARG(q && k && v && out && b > 0 && h > 0 && kvh > 0 && h % kvh == 0 && s_len > 0, SAT_E_INVALID, "attention_f32 (causal): bad args");
    SAT_CHECK_ARG((((uintptr_t)q | (uintptr_t)out) & 15) == 0, SAT_E_INVALID, "attention_f32 (causal): q and out must be 16-byte aligned");
    SAT_CHECK_ARG(h <= 65535 && b <= 65535, SAT_E_UNSUPPORTED, "attention_f32 (causal): %d heads / %d sequences exceed the grid", h, b);
    const dim3 grid(cdiv(s_len, 64), h, b);
    if (head_dim == 32) hipLaunchKernelGGL((attention_f32_kernel<32, true>), grid, dim3(64), 0, s, q, k, v, out, h, kvh, s_len, s_len);
    else if (head_dim == 64) hipLaunchKernelGGL((attention_f32_kernel<64, true>), grid, dim3(64), 0, s, q, k, v, out, h, kvh, s_len, s_len);
    else hipLaunchKernelGGL((attention_f32_kernel<96, true>), grid, dim3(64), 0, s, q, k, v, out, h, kvh, s_len, s_len);
    SAT_LAUNCH_CHECK();
    return 0;
}
