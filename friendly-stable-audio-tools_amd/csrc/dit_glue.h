#pragma once
#include "sat_common.h"

int glue_small_linear(const float* x, int ldx, const float* W, const float* bias, const float* add, int ldadd, void* y,
                      int ldy, int R, int N, int K, int act, int out16, hipStream_t s);      // out16: 0 fp32, 1 bf16, 2 fp16
int glue_adaln_finish(float* ssg, int64_t n, int D, hipStream_t s);
int glue_fourier(const float* t, float t_const, const float* w, float* out, int B, int half_feat, hipStream_t s);
int glue_fold_in(const float* Win, const float* Wpre, float* Weff, int D, int C, hipStream_t s);
int glue_fold_out(const float* Wout, const float* Wpost, float* Weff, int D, int C, hipStream_t s);
int glue_input_proj(const float* x, const float* Weff, float* X, int Bf, int xB, int C, int T, int S, int D, float xscale,
                    hipStream_t s);
// the same launch for a model with input-concat / prepend conditioning: + W_c concat (nearest-resized from Tc frames, unscaled) and the
// P prepared prepend rows copied to X[b, 0..P-1]; S = P + 1 + T
int glue_input_proj_extra(const float* x, const float* Weff, float* X, int Bf, int xB, int C, int T, int S, int D, float xscale,
                          const float* concat, int Cc, int Tc, const float* prep, int P, hipStream_t s);
// position embeddings added to the stream (ContinuousTransformer use_sinusoidal_emb / use_abs_pos_emb): the [rows, D] table once per plan
// (mode 1: sinusoidal, src = the learnt scale [1]; mode 2: absolute, src = emb.weight [>= rows, D]), then X[b, s, :] += table[s, :] per forward
int glue_pos_table(int mode, const float* src, float* table, int rows, int D, hipStream_t s);
int glue_add_pos(float* X, const float* table, int Bf, int S, int D, hipStream_t s);
int glue_output_proj(const float* X, const float* Weff, float* out, int Bf, int C, int T, int S, int D, hipStream_t s);
// ---- patchified DiT (sat_dit_plan_set_patch, patch_size P > 1): dit_patch.hip.  WEAK as the optional launchers of sat_common.h: null in the
// host test driver, where sat_dit_plan_set_patch answers SAT_E_UNSUPPORTED to a patch size above 1.  T stays in latent frames (a multiple
// of P), S counts token rows: prepend rows + (1 global token) + T / P.  Weights [D, Ci P] / [C P, D] with feature index c * P + p; the folds
// write [Ci P][D] and [D][C P].  The input projection is one entry: Cc = 0 and Pl = 0 is the plain model.
__attribute__((weak)) int glue_fold_in_patch(const float* Win, const float* Wpre, float* Weff, int D, int Ci, int P, hipStream_t s);
__attribute__((weak)) int glue_fold_out_patch(const float* Wout, const float* Wpost, float* Weff, int D, int C, int P, hipStream_t s);
__attribute__((weak)) int glue_input_proj_patch(const float* x, const float* Weff, float* X, int Bf, int xB, int C, int P, int T, int S, int D,
                                                float xscale, const float* concat, int Cc, int Tc, const float* prep, int Pl, hipStream_t s);
__attribute__((weak)) int glue_output_proj_patch(const float* X, const float* Weff, float* out, int Bf, int C, int P, int T, int S, int D,
                                                 hipStream_t s);
int glue_cfg_denoise(const float* mo, const float* x, float* den, int B, int C, int T, int use_cfg, float cfg_scale,
                     float scale_phi, float c_out, float c_skip, hipStream_t s);
// diagnostics of the residual stream (sat_dit_debug): per launch 4 floats at `out`, combined with atomics over the M rows:
// [0] max |x|, [1] max over rows of |mean| / std, [2] number of elements with |x| > 65504 (what an fp16 image saturates), [3] max over rows of max|x| / rms
int glue_resid_stats(const float* X, int M, int D, float* out, hipStream_t s);

