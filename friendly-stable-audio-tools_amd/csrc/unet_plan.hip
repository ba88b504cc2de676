// The Dance Diffusion U-Net on the device: DiffusionAttnUnet1D of the reference's models/diffusion.py (:376-479), built from ResConvBlock,
// SelfAttention1d, SkipBlock, Downsample1d and Upsample1d of models/blocks.py (:14-159) -- the network create_model_from_config selects with
// "model_type": "diffusion_uncond", "type": "DAU1d".  One plan on plan_core.h, composed from the launchers of sat_common.h; its own kernels are
// unet_kernels.hip.
//
//   input    cat([x * in_scale, planes(FourierFeatures(1, 16)(t))]) [b, io + 16, T] -> net.0.main.0 and net.0.skip, in fp32, into rows
//   level 0  (T rows per item, c_0 channels) three blocks, level 1, three blocks; the last one ends in the output boundary [b, io, T]
//   level i  (T / 2^i rows, c_i channels) SkipBlock: cat([Up(blocks(level i + 1(blocks(Down(x))))), x]) along the channels, main branch first
//   block    ResConvBlock: conv k -> GroupNorm(1, c) -> GELU -> conv k -> GroupNorm(1, c) -> GELU, + skip (identity, or a bias-free 1 x 1
//            convolution of the block's input where the widths differ); the last block of level 0 has no second norm / activation
//   attn     SelfAttention1d behind every block of the levels i >= depth - n_attn_layers - 1 (0-based), i > 0: x += out_proj(softmax(q k^T /
//            sqrt(32)) v) on qkv_proj(GroupNorm(1, c)(x)), 32-channel heads, no rotation
//
// Layout.  Activations are channel-last rows [b * t_i, c].  Between blocks a tensor lives twice: the fp32 stream X (the identity skip, the
// attention residual, what the norms read) and its image A in the plan's operand format (fp16 / bf16; fp32 in the verification mode), which
// is what the convolutions contract: k-tap convolutions on ff_conv.hip with the weight packed tap-major at finalize, 1 x 1 convolutions on
// the fp32-output GEMMs.  Every convolution writes fp32; the GroupNorm statistics, the softmax, the skip sums and both boundary layers are
// fp32 in every format.  Each level i >= 1 owns a concat buffer CAT_i [b * t_{i-1}, 2 c_{i-1}] in the operand format: on the way down the
// level's input is cast into its second half, on the way up the upsampler writes its first half, and the parent's next block -- always one
// with a 1 x 1 skip, 2 c -> c -- reads it as a dense operand.
//
// Launches, 16-bit operands.  Block: conv, stats (2), apply, conv, [skip GEMM], stats (2), apply = 8 or 9.  Attention: stats (2), apply,
// qkv GEMM, head split, attention, out_proj (+= into the stream), cast = 8.  Level: cast into CAT, downsample (and a copy of its fp32 output
// back into the stream buffer), a clear of the q / k / v pads on entry and again behind the inner level, six blocks (+ six attentions), upsample.  The verification mode adds a row gather in front of every k-tap convolution.
#include <algorithm>
#include <string>
#include <vector>

#include "sat_common.h"
#include "plan_core.h"

namespace {

struct UConv {      // w [n, taps * k] tap-major in the operand format; n == 0: absent
    void* w = nullptr;
    float* bias = nullptr;
    int n = 0, k = 0, taps = 1;
};
struct UBlock {
    UConv c1, c2, skip;
    float *g1 = nullptr, *b1 = nullptr, *g2 = nullptr, *b2 = nullptr;
    int cin = 0, cmid = 0, cout = 0;
};
struct UAttn {
    float *g = nullptr, *b = nullptr;
    UConv qkv, out;
    int c = 0;      // 0: nn.Identity
};
struct ULevel {
    int c = 0, c_prev = 0;
    UBlock blk[6];
    UAttn att[6];
};

}  // namespace

struct sat_unet_plan {
    sat_unet_cfg cfg;
    TensorTable tensors;
    bool finalized = false;
    DevBuf arena;
    int fmt = 0;
    bool f32 = false;
    std::vector<ULevel> levels;
    // the two boundary layers, fp32 in the reference's layout: net.0.main.0 / net.0.skip and net.6.main.3 / net.6.skip
    float *w_embed = nullptr, *w_in = nullptr, *b_in = nullptr, *w_in_skip = nullptr, *w_out = nullptr, *b_out = nullptr, *w_out_skip = nullptr;
};

extern "C" int sat_unet_plan_create(const sat_unet_cfg* cfg, size_t cfg_bytes, sat_unet_plan** out_plan) {
    SAT_CHECK_ARG(cfg && out_plan, SAT_E_INVALID, "unet_plan_create: null argument");
    SAT_CHECK_ARG(cfg_bytes == sizeof(sat_unet_cfg), SAT_E_INVALID, "unet_plan_create: sat_unet_cfg of %zu bytes, this library reads %zu", cfg_bytes,
                  sizeof(sat_unet_cfg));
    const sat_unet_cfg& c = *cfg;
    SAT_CHECK_ARG(c.io_channels > 0 && c.depth >= 1 && c.n_attn_layers >= 0 && c.kernel_size >= 1, SAT_E_INVALID, "unet_plan_create: bad sizes");
    SAT_CHECK_ARG(!c.use_snake, SAT_E_UNSUPPORTED, "unet_plan_create: use_snake: Snake1d comes from the dac library, which this build does not have");
    SAT_CHECK_ARG(!c.learned_resample, SAT_E_UNSUPPORTED, "unet_plan_create: learned_resample: only the fixed cubic resamplers are built");
    SAT_CHECK_ARG(c.cond_dim == 0 && !c.cond_noise_aug, SAT_E_UNSUPPORTED,
                  "unet_plan_create: cond_dim %d / cond_noise_aug %d: the reference's own forward fails on a conditioning tensor", c.cond_dim, c.cond_noise_aug);
    SAT_CHECK_ARG(c.kernel_size == 1 || c.kernel_size == 3 || c.kernel_size == 5 || c.kernel_size == 7, SAT_E_UNSUPPORTED,
                  "unet_plan_create: kernel_size %d (the convolution kernels take 1, 3, 5 and 7)", c.kernel_size);
    SAT_CHECK_ARG(c.depth >= 2, SAT_E_INVALID, "unet_plan_create: depth 1: the reference builds a block that reads 2 c channels behind an nn.Identity and fails");
    SAT_CHECK_ARG(c.depth <= SAT_UNET_MAX_DEPTH, SAT_E_UNSUPPORTED, "unet_plan_create: depth %d exceeds %d", c.depth, SAT_UNET_MAX_DEPTH);
    SAT_CHECK_ARG(c.io_channels + 16 <= 128, SAT_E_UNSUPPORTED, "unet_plan_create: io_channels %d + 16 timestep planes exceed the 128 the boundary kernel stages",
                  c.io_channels);
    for (int i = 0; i < c.depth; ++i)
        SAT_CHECK_ARG(c.channels[i] > 0 && c.channels[i] % 128 == 0 && c.channels[i] <= 8192, SAT_E_UNSUPPORTED,
                      "unet_plan_create: channels[%d] = %d must be a multiple of 128 (the GEMM launchers take N %% 128 == 0 and K %% 64 == 0)", i, c.channels[i]);
    SAT_CHECK_ARG(c.gemm_dtype == SAT_GEMM_BF16 || c.gemm_dtype == SAT_GEMM_FP16 || c.gemm_dtype == SAT_GEMM_FP32X, SAT_E_UNSUPPORTED,
                  "unet_plan_create: gemm_dtype %d (bf16, fp16 or the fp32 build)", c.gemm_dtype);
    SAT_CHECK_ARG(sat_launch_ff_conv && sat_launch_pack_conv_taps && sat_launch_im2col_rows_f32 && sat_launch_head_split_hdw && sat_launch_attention_hdw &&
                      sat_launch_split_heads_f32_w && sat_launch_attention_f32_w,
                  SAT_E_UNSUPPORTED, "unet_plan_create: built without the convolution or the staged attention kernels");
    sat_unet_plan* p = new (std::nothrow) sat_unet_plan();
    SAT_CHECK_ARG(p, SAT_E_INVALID, "unet_plan_create: out of host memory");
    p->cfg = c;
    p->fmt = c.gemm_dtype;
    p->f32 = c.gemm_dtype == SAT_GEMM_FP32X;
    *out_plan = p;
    return 0;
}

extern "C" void sat_unet_plan_destroy(sat_unet_plan* p) { delete p; }

extern "C" int sat_unet_plan_set_tensor(sat_unet_plan* p, const char* name, const float* data_dev, int64_t numel) {
    SAT_CHECK_ARG(p, SAT_E_INVALID, "unet_plan_set_tensor: bad argument");
    return p->tensors.set("unet", name, data_dev, numel);
}

namespace {

// SelfAttention1d follows the blocks of the reference's levels i >= depth - n_attn_layers (1-based, i > 1): 0-based level l = i - 1
bool level_has_attn(const sat_unet_cfg& c, int l) { return l >= 1 && c.n_attn_layers > 0 && l + 1 >= c.depth - c.n_attn_layers; }

int unet_build(sat_unet_plan* p, Bump& ar, hipStream_t s) {
    const sat_unet_cfg& c = p->cfg;
    const int taps = c.kernel_size;
    const size_t el = p->f32 ? 4 : 2;
    auto place = [&](const std::string& name, int64_t numel, float** dst) -> int { return p->tensors.place("unet", ar, name, numel, dst, s); };
    auto conv = [&](const std::string& mod, int n, int k, int tp, bool bias, UConv* out) -> int {
        out->n = n; out->k = k; out->taps = tp;
        out->w = ar.take((size_t)n * k * tp * el);
        out->bias = nullptr;
        if (!ar.dry()) {
            const float* src;
            SAT_TRY(p->tensors.get("unet", mod + ".weight", (int64_t)n * k * tp, &src));
            SAT_TRY(sat_launch_pack_conv_taps(src, out->w, n, k, tp, p->fmt, s));
        }
        if (bias) SAT_TRY(place(mod + ".bias", n, &out->bias));
        return 0;
    };
    // boundary: the first conv and skip of `first`, the second conv and skip of `last`, stay fp32 in the reference's layout
    auto block = [&](const std::string& pre, int cin, int cmid, int cout, int boundary, UBlock* B) -> int {
        B->cin = cin; B->cmid = cmid; B->cout = cout;
        if (boundary == 1) {
            SAT_TRY(place(pre + "main.0.weight", (int64_t)cmid * cin * taps, &p->w_in));
            if (c.conv_bias) SAT_TRY(place(pre + "main.0.bias", cmid, &p->b_in));
            SAT_TRY(place(pre + "skip.weight", (int64_t)cout * cin, &p->w_in_skip));
        } else {
            SAT_TRY(conv(pre + "main.0", cmid, cin, taps, c.conv_bias != 0, &B->c1));
        }
        SAT_TRY(place(pre + "main.1.weight", cmid, &B->g1));
        SAT_TRY(place(pre + "main.1.bias", cmid, &B->b1));
        if (boundary == 2) {
            SAT_TRY(place(pre + "main.3.weight", (int64_t)cout * cmid * taps, &p->w_out));
            if (c.conv_bias) SAT_TRY(place(pre + "main.3.bias", cout, &p->b_out));
            SAT_TRY(place(pre + "skip.weight", (int64_t)cout * cin, &p->w_out_skip));
            return 0;
        }
        SAT_TRY(conv(pre + "main.3", cout, cmid, taps, c.conv_bias != 0, &B->c2));
        SAT_TRY(place(pre + "main.4.weight", cout, &B->g2));
        SAT_TRY(place(pre + "main.4.bias", cout, &B->b2));
        B->skip = UConv{};
        if (cin != cout && boundary != 1) SAT_TRY(conv(pre + "skip", cout, cin, 1, false, &B->skip));
        return 0;
    };
    auto attn = [&](const std::string& pre, int ch, UAttn* A) -> int {
        A->c = ch;
        SAT_TRY(place(pre + "norm.weight", ch, &A->g));
        SAT_TRY(place(pre + "norm.bias", ch, &A->b));
        SAT_TRY(conv(pre + "qkv_proj", 3 * ch, ch, 1, true, &A->qkv));
        return conv(pre + "out_proj", ch, ch, 1, true, &A->out);
    };
    p->w_embed = p->w_in = p->b_in = p->w_in_skip = p->w_out = p->b_out = p->w_out_skip = nullptr;
    SAT_TRY(place("timestep_embed.weight", 8, &p->w_embed));
    p->levels.assign(c.depth, ULevel{});
    std::string pre = "net.";
    for (int l = 0; l < c.depth; ++l) {
        ULevel& L = p->levels[l];
        L.c = c.channels[l];
        L.c_prev = l ? c.channels[l - 1] : c.channels[0];
        const int ch = L.c, cp = L.c_prev;
        const bool deepest = l == c.depth - 1;
        const int up_in = deepest ? ch : 2 * ch;
        auto at = [&](int i) { return pre + std::to_string(i) + "."; };
        if (l == 0) {
            SAT_TRY(block(at(0), c.io_channels + 16, ch, ch, 1, &L.blk[0]));
            SAT_TRY(block(at(1), ch, ch, ch, 0, &L.blk[1]));
            SAT_TRY(block(at(2), ch, ch, ch, 0, &L.blk[2]));
            SAT_TRY(block(at(4), up_in, ch, ch, 0, &L.blk[3]));
            SAT_TRY(block(at(5), ch, ch, ch, 0, &L.blk[4]));
            SAT_TRY(block(at(6), ch, ch, c.io_channels, 2, &L.blk[5]));
            pre += "3.main.";
        } else {
            static const int bpos[6] = {1, 3, 5, 8, 10, 12};
            const int cins[6] = {cp, ch, ch, up_in, ch, ch}, couts[6] = {ch, ch, ch, ch, ch, cp};
            for (int i = 0; i < 6; ++i) {
                SAT_TRY(block(at(bpos[i]), cins[i], ch, couts[i], 0, &L.blk[i]));
                if (level_has_attn(c, l)) SAT_TRY(attn(at(bpos[i] + 1), couts[i], &L.att[i]));
            }
            pre += "7.main.";
        }
    }
    return 0;
}

struct UWs {
    float *X0, *X1, *Y, *Sk, *wide, *part, *stats, *im;
    char *A, *Amid, *Q, *K, *Vt;
    char* cat[SAT_UNET_MAX_DEPTH];
    size_t qkv_bytes, total;
};

int unet_check_length(const sat_unet_plan* p, int t) {
    const int d = p->cfg.depth;
    SAT_CHECK_ARG(t > 0 && (t % (1 << (d - 1))) == 0, SAT_E_INVALID, "unet: a length of %d samples is no multiple of 2^(depth - 1) = %d", t, 1 << (d - 1));
    SAT_CHECK_ARG((t >> (d - 1)) >= 3, SAT_E_INVALID, "unet: %d samples leave %d rows at the deepest level, fewer than the 3 the reflect padding needs", t,
                  t >> (d - 1));
    return 0;
}

int unet_carve(const sat_unet_plan* p, int b, int t, char* base, UWs* out) {
    const sat_unet_cfg& c = p->cfg;
    SAT_TRY(unet_check_length(p, t));
    const size_t el = p->f32 ? 4 : 2;
    const int taps = c.kernel_size;
    size_t x_el = 0, a_el = 0, wide_el = 0, qkv = 0, im_el = 0, part_el = 0;
    int64_t widest = 0;
    for (int l = 0; l < c.depth; ++l) {
        const size_t M = (size_t)b * (t >> l), ch = c.channels[l], cp = l ? c.channels[l - 1] : ch;
        const size_t cmax = std::max(ch, cp);
        x_el = std::max(x_el, M * cmax);
        a_el = std::max(a_el, M * cmax);
        im_el = std::max(im_el, M * std::max(2 * ch, cp) * taps);
        part_el = std::max(part_el, (size_t)b * sat_unet_gn_tiles((int64_t)(t >> l) * cmax) * 2);
        widest = std::max<int64_t>(widest, (int64_t)M * (int64_t)(2 * cmax));
        if (level_has_attn(c, l)) {
            wide_el = std::max(wide_el, M * 3 * cmax);
            const size_t Spad = (size_t)round_up((t >> l) + 3, 128);
            qkv = std::max(qkv, p->f32 ? M * cmax * 4 : (size_t)b * (cmax / 32) * Spad * 32 * 2);
            widest = std::max<int64_t>(widest, (int64_t)M * (int64_t)(3 * cmax));
        }
    }
    SAT_CHECK_ARG(widest < (1ll << 31) && (int64_t)b * t <= (1 << 30), SAT_E_UNSUPPORTED, "unet: %d items of %d samples: a GEMM output of %lld elements exceeds 2^31", b, t,
                  (long long)widest);
    Bump ws{base};
    UWs w{};
    w.X0 = (float*)ws.take(x_el * 4);
    w.X1 = (float*)ws.take(x_el * 4);
    w.Y = (float*)ws.take(x_el * 4);
    w.Sk = (float*)ws.take(x_el * 4);
    w.A = (char*)ws.take(a_el * el);
    w.Amid = (char*)ws.take(a_el * el);
    w.part = (float*)ws.take(part_el * 4);
    w.stats = (float*)ws.take((size_t)b * 2 * 4);
    w.im = p->f32 && taps > 1 ? (float*)ws.take(im_el * 4) : nullptr;
    w.wide = wide_el ? (float*)ws.take(wide_el * 4) : nullptr;
    w.qkv_bytes = (size_t)round_up((int64_t)qkv, 256);
    if (qkv) {
        w.Q = (char*)ws.take(w.qkv_bytes);
        w.K = (char*)ws.take(w.qkv_bytes);
        w.Vt = (char*)ws.take(w.qkv_bytes);
    }
    for (int l = 1; l < c.depth; ++l) w.cat[l] = (char*)ws.take((size_t)b * (t >> (l - 1)) * 2 * c.channels[l - 1] * el);
    w.total = ws.off;
    *out = w;
    return 0;
}

struct URun {
    const sat_unet_plan* p;
    UWs w;
    hipStream_t s;
    int b;

    // y [b * S, cv.n] (+)= conv(a [b * S, cv.k]), zero padding per item; a is dense in the operand format
    int conv(const UConv& cv, const void* a, int S, float* y, int accumulate = 0) const {
        const int M = b * S;
        if (p->f32) {
            const float* src = (const float*)a;
            if (cv.taps > 1) {
                SAT_TRY(sat_launch_im2col_rows_f32(src, w.im, b, S, cv.k, cv.taps, s));
                src = w.im;
            }
            return sat_launch_gemm_f32(src, (const float*)cv.w, cv.bias, y, M, cv.n, cv.taps * cv.k, cv.n, accumulate, nullptr, 1, 0, s);
        }
        if (cv.taps == 1) {
            GemmArgs g{};
            g.f16 = p->fmt == SAT_GEMM_FP16;
            g.A = (const op_t*)a; g.W = (const op_t*)cv.w; g.bias = cv.bias; g.M = M; g.N = cv.n; g.K = cv.k;
            g.C = y; g.ldc = cv.n; g.accumulate = accumulate;
            return sat_launch_gemm(accumulate ? EPI_RESID : EPI_F32, g, s);
        }
        FfConvArgs f{};
        f.fmt = p->fmt; f.A = a; f.W = cv.w; f.bias = cv.bias; f.B = b; f.S = S; f.N = cv.n; f.K = cv.k; f.taps = cv.taps;
        f.epi = FFC_RESID; f.C = y; f.ldc = cv.n; f.accumulate = accumulate;
        return sat_launch_ff_conv(f, s);
    }
    int stats(const float* x, int S, int ch) const { return sat_launch_unet_gn_stats(x, w.part, w.stats, b, (int64_t)S * ch, 1e-5f, s); }
    int apply(const float* x, const float* g, const float* bt, const float* skip, float* out32, void* out_op, int S, int ch, int act) const {
        return sat_launch_unet_gn_apply(x, w.stats, g, bt, skip, out32, out_op, b, S, ch, ch, act, p->fmt, s);
    }
    // the second half of a block, from the first convolution's output in Y: X [b * S, cout] and its image A leave; X holds the block's input when the
    // skip is the identity, `a_in` is its operand image (the 1 x 1 skip reads it)
    int block_tail(const UBlock& B, const void* a_in, const float* skip_ready, int S) const {
        SAT_TRY(stats(w.Y, S, B.cmid));
        SAT_TRY(apply(w.Y, B.g1, B.b1, nullptr, nullptr, w.Amid, S, B.cmid, 1));
        SAT_TRY(conv(B.c2, w.Amid, S, w.Y));
        const float* skip = skip_ready ? skip_ready : w.X0;
        if (!skip_ready && B.skip.n) {
            SAT_TRY(conv(B.skip, a_in, S, w.Sk));
            skip = w.Sk;
        }
        SAT_TRY(stats(w.Y, S, B.cout));
        return apply(w.Y, B.g2, B.b2, skip, w.X0, w.A, S, B.cout, 1);
    }
    int block(const UBlock& B, const void* a_in, int S) const {
        SAT_TRY(conv(B.c1, a_in, S, w.Y));
        return block_tail(B, a_in, nullptr, S);
    }
    int attention(const UAttn& at, int S) const {
        const int M = b * S, ch = at.c, H = ch / 32;
        SAT_TRY(stats(w.X0, S, ch));
        SAT_TRY(apply(w.X0, at.g, at.b, nullptr, nullptr, w.Amid, S, ch, 0));
        SAT_TRY(conv(at.qkv, w.Amid, S, w.wide));
        if (p->f32) {
            SAT_TRY(sat_launch_split_heads_f32_w(w.wide, (float*)w.Q, (float*)w.K, (float*)w.Vt, M, S, 3, H, 32, 0, nullptr, nullptr, s, 0));
            SAT_TRY(sat_launch_attention_f32_w((const float*)w.Q, (const float*)w.K, (const float*)w.Vt, (float*)w.Amid, b, H, H, 32, S, S, s));
        } else {
            const int f16 = p->fmt == SAT_GEMM_FP16, Spad = (int)round_up(S + 3, 128);
            HeadsEpi he{};
            he.out[0] = (op_t*)w.Q; he.out[1] = (op_t*)w.K; he.out[2] = (op_t*)w.Vt;
            he.kind[0] = 8; he.kind[1] = 4; he.kind[2] = 1 | 4;
            he.qscale = sat_attn_qscale(32);      // (q 32^-1/4)(k 32^-1/4)^T, in the log2 domain
            he.parts = 3; he.heads = H; he.S = S; he.Spad = Spad;
            SAT_TRY(sat_launch_head_split_hdw(w.wide, he, 32, b, s, f16));
            SAT_TRY(sat_launch_attention_hdw((const op_t*)w.Q, (const op_t*)w.K, (const op_t*)w.Vt, (op_t*)w.Amid, b, H, H, 32, S, S, Spad, Spad, s, f16));
        }
        SAT_TRY(conv(at.out, w.Amid, S, w.X0, 1));
        return sat_launch_unet_cast_rows(w.X0, w.A, (int64_t)M, ch, ch, p->fmt, s);
    }
    int level(int l, int S) const;
};

// enters with the level's input in X0 / A ([b * 2 S, c_prev]; level 0: the caller ran the input boundary), leaves with its output: for l >= 1 in
// CAT_l's first half, for level 0 in Y (the last block's activated first convolution) with the last block's input in X0
int URun::level(int l, int S) const {
    const sat_unet_cfg& c = p->cfg;
    const ULevel& L = p->levels[l];
    const bool deepest = l == c.depth - 1, att = level_has_attn(c, l);
    const size_t el = p->f32 ? 4 : 2;
    if (l >= 1) {
        const int cp = L.c_prev;
        SAT_TRY(sat_launch_unet_cast_rows(w.X0, w.cat[l] + (size_t)cp * el, (int64_t)b * 2 * S, cp, 2 * cp, p->fmt, s));
        SAT_TRY(sat_launch_unet_downsample(w.X0, w.X1, w.A, b, 2 * S, cp, p->fmt, s));
        SAT_HIP(hipMemcpyAsync(w.X0, w.X1, (size_t)b * S * cp * 4, hipMemcpyDeviceToDevice, s));
        if (att && !p->f32) SAT_HIP(hipMemsetAsync(w.Q, 0, 3 * w.qkv_bytes, s));      // the pads must be finite: the head split writes the valid rows only
    }
    for (int i = 0; i < 3; ++i) {
        if (l == 0 && i == 0) SAT_TRY(block_tail(L.blk[0], nullptr, w.Sk, S));
        else SAT_TRY(block(L.blk[i], w.A, S));
        if (L.att[i].c) SAT_TRY(attention(L.att[i], S));
    }
    const void* a_in = w.A;
    if (!deepest) {
        SAT_TRY(level(l + 1, S / 2));
        a_in = w.cat[l + 1];
        if (att && !p->f32) SAT_HIP(hipMemsetAsync(w.Q, 0, 3 * w.qkv_bytes, s));      // the inner level left its own rows there
    }
    for (int i = 3; i < 6; ++i) {
        if (l == 0 && i == 5) {      // the last block: its first half only, activated into Y in fp32; X0 keeps the block's input
            SAT_TRY(conv(L.blk[5].c1, w.A, S, w.Y));
            SAT_TRY(stats(w.Y, S, L.blk[5].cmid));
            return apply(w.Y, L.blk[5].g1, L.blk[5].b1, nullptr, w.Y, nullptr, S, L.blk[5].cmid, 1);
        }
        SAT_TRY(block(L.blk[i], i == 3 ? a_in : w.A, S));
        if (L.att[i].c) SAT_TRY(attention(L.att[i], S));
    }
    return sat_launch_unet_upsample(w.X0, w.cat[l], b, S, L.c_prev, 2 * L.c_prev, p->fmt, s);
}

}  // namespace

extern "C" int sat_unet_plan_finalize(sat_unet_plan* p, sat_stream_t stream) {
    SAT_CHECK_ARG(p, SAT_E_INVALID, "unet_plan_finalize: null plan");
    hipStream_t s = (hipStream_t)stream;
    return plan_finalize(p, s, [&](Bump& ar) { return unet_build(p, ar, s); });
}

extern "C" int sat_unet_workspace_bytes(const sat_unet_plan* p, int32_t b, int32_t t, size_t* out_bytes) {
    SAT_CHECK_ARG(p && out_bytes && b > 0 && t > 0, SAT_E_INVALID, "unet_workspace_bytes: bad arguments");
    UWs w;
    SAT_TRY(unet_carve(p, b, t, nullptr, &w));
    *out_bytes = w.total;
    return 0;
}

extern "C" int sat_unet_forward(sat_unet_plan* p, const float* x_dev, const float* t_dev, float in_scale, float* out_dev, int32_t b, int32_t t, void* ws,
                                size_t ws_bytes, sat_stream_t stream) {
    SAT_CHECK_ARG(p && p->finalized, SAT_E_STATE, "unet_forward: plan not finalized");
    SAT_CHECK_ARG(x_dev && t_dev && out_dev && ws && b > 0 && t > 0, SAT_E_INVALID, "unet_forward: bad arguments");
    SAT_CHECK_ARG(((uintptr_t)ws & 255) == 0, SAT_E_INVALID, "unet_forward: workspace must be 256-byte aligned");
    const sat_unet_cfg& c = p->cfg;
    // the length is checked before anything is launched (unet_check_length, inside the carve)
    URun run{p, {}, (hipStream_t)stream, b};
    SAT_TRY(unet_carve(p, b, t, (char*)ws, &run.w));
    SAT_CHECK_ARG(ws_bytes >= run.w.total, SAT_E_WORKSPACE, "unet_forward: workspace %zu < required %zu", ws_bytes, run.w.total);
    const int c0 = c.channels[0];
    SAT_TRY(sat_launch_unet_input(x_dev, t_dev, in_scale, p->w_embed, p->w_in, p->b_in, p->w_in_skip, run.w.Y, run.w.Sk, b, c.io_channels, t, c0, c.kernel_size,
                                  run.s));
    SAT_TRY(run.level(0, t));
    return sat_launch_unet_output(run.w.Y, run.w.X0, p->w_out, p->b_out, p->w_out_skip, out_dev, b, c.io_channels, t, c0, c.kernel_size, run.s);
}
