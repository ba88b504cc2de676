// fp32 self-attention of the text encoders (t5_encoder.hip, roberta_encoder.hip): softmax(scale * q k^T + position_bias + key_mask) v.
// One kernel for both stacks; they differ in two arguments only:
//   T5      scale = 1 (T5Attention does not scale), pb = the bucketed relative-position table [H][2L - 1]
//   RoBERTa scale = 1 / sqrt(d_head), pb = nullptr (absolute positions live in the embeddings)
// A few hundred keys at most, once per generation: one wave per (query, head, sequence), scores in registers, no MFMA.
#pragma once
#include <math.h>

#include "sat_common.h"

namespace {

// qkv [B*L][3*inner] (q | k | v), out [B*L][inner].  Keys beyond the attention mask get finfo.min added, exactly as the transformers
// models do (so an all-padding row degenerates to the same uniform average).  Dynamic LDS: (dkv + L) floats.
constexpr int ENC_MAX_KEYS_PER_LANE = 8;      // L <= 512
__global__ __launch_bounds__(64) void enc_attention_kernel(const float* __restrict__ qkv, const float* __restrict__ pb,
                                                           const int* __restrict__ mask, float* __restrict__ out, int L, int H, int dkv,
                                                           float scale) {
    extern __shared__ float enc_sm[];         // q [dkv] then p [L]
    float* sq = enc_sm;
    float* sp = enc_sm + dkv;
    const int i = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
    const int lane = threadIdx.x;
    const int inner = H * dkv, ld = 3 * inner;
    const float* base = qkv + (size_t)b * L * ld;
    for (int d = lane; d < dkv; d += 64) sq[d] = base[(size_t)i * ld + h * dkv + d];
    __syncthreads();
    float sc[ENC_MAX_KEYS_PER_LANE];
    float mx = -INFINITY;
#pragma unroll
    for (int u = 0; u < ENC_MAX_KEYS_PER_LANE; ++u) {
        const int j = lane + u * 64;
        sc[u] = -INFINITY;
        if (j < L) {
            const float4* kr = reinterpret_cast<const float4*>(base + (size_t)j * ld + inner + h * dkv);
            float s = 0.f;
            for (int d4 = 0; d4 < dkv / 4; ++d4) {
                const float4 kv = kr[d4];
                const float4 qv = reinterpret_cast<const float4*>(sq)[d4];
                s += (qv.x * kv.x + qv.y * kv.y) + (qv.z * kv.z + qv.w * kv.w);
            }
            s *= scale;                       // exact for scale == 1
            if (pb) s += pb[(size_t)h * (2 * L - 1) + (j - i + L - 1)];
            if (!mask[(size_t)b * L + j]) s += -3.4028234663852886e38f;
            sc[u] = s;
            mx = fmaxf(mx, s);
        }
    }
    mx = wave_max(mx);
    float sum = 0.f;
#pragma unroll
    for (int u = 0; u < ENC_MAX_KEYS_PER_LANE; ++u) {
        const int j = lane + u * 64;
        if (j < L) {
            const float p = expf(sc[u] - mx);
            sp[j] = p;
            sum += p;
        }
    }
    sum = wave_sum(sum);
    __syncthreads();
    const float inv = 1.0f / sum;
    for (int d = lane; d < dkv; d += 64) {
        const float* vc = base + 2 * inner + h * dkv + d;
        float o = 0.f;
        for (int j = 0; j < L; ++j) o += sp[j] * vc[(size_t)j * ld];
        out[((size_t)b * L + i) * inner + h * dkv + d] = o * inv;
    }
}

// The one launch of the kernel: both encoders and the unit entry (sat_enc_attention) come through here.  The scores of a query live in
// ENC_MAX_KEYS_PER_LANE registers per lane (a longer sequence would silently lose its keys beyond 64 * that), K rows are read as float4.
int enc_attention_launch(const float* qkv, const float* pb, const int* mask, float* out, int B, int L, int H, int dkv, float scale,
                         hipStream_t s) {
    SAT_CHECK_ARG(qkv && mask && out && B > 0 && L > 0 && H > 0 && dkv > 0, SAT_E_INVALID, "enc_attention: bad arguments");
    SAT_CHECK_ARG(((uintptr_t)qkv & 15) == 0, SAT_E_INVALID, "enc_attention: qkv must be 16-byte aligned");
    SAT_CHECK_ARG(L <= 64 * ENC_MAX_KEYS_PER_LANE, SAT_E_UNSUPPORTED, "enc_attention: sequence length %d > %d", L, 64 * ENC_MAX_KEYS_PER_LANE);
    SAT_CHECK_ARG(dkv % 4 == 0, SAT_E_UNSUPPORTED, "enc_attention: head dim %d must be a multiple of 4", dkv);
    SAT_CHECK_ARG(H <= 65535 && B <= 65535, SAT_E_UNSUPPORTED, "enc_attention: %d heads / %d sequences exceed the grid", H, B);
    const size_t lds = (size_t)(dkv + L) * sizeof(float);
    SAT_CHECK_ARG(lds <= 64 * 1024, SAT_E_UNSUPPORTED, "enc_attention: head dim %d + %d keys need %zu bytes of LDS (64 KiB without opting in to more)",
                  dkv, L, lds);
    hipLaunchKernelGGL(enc_attention_kernel, dim3(L, H, B), dim3(64), lds, s, qkv, pb, mask, out, L, H, dkv, scale);
    SAT_LAUNCH_CHECK();
    return 0;
}

}  // namespace
