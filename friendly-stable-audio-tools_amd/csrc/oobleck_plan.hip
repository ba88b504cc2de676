// The Oobleck codec's plan (models/autoencoders.py:45-194 of the reference): weight set-up at finalize, the workspace, the launch lists of
// decode / encode, the range report and the unit-level entry.  Host code only; the kernels and the launchers that own grid, LDS size and tile
// choice are oobleck.hip, built once per operand format, and reach this file as one OobKernels table per build (oobleck_kernels.h), looked up
// once by gemm_dtype.  Operand buffers (activations, packed weights, the zero page) are opaque here: void* and OobKernels::elem_bytes.
#include <stdlib.h>

#include <algorithm>
#include <new>
#include <string>
#include <vector>

#include "oobleck_kernels.h"
#include "plan_core.h"

namespace {

using bf16::ConvArgs;      // the layout of every build (oobleck_kernels.h); the operand pointers are opaque here
using bf16::RuArgs;
inline op_t* opq(void* p) { return static_cast<op_t*>(p); }
inline const op_t* opq(const void* p) { return static_cast<const op_t*>(p); }

const OobKernels* kernels_of(int gemm_dtype) {
    switch (gemm_dtype) {
        case SAT_GEMM_BF16: return bf16::oob_kernels();
        case SAT_GEMM_FP16: return f16::oob_kernels();
        case SAT_GEMM_FP32X: return f32::oob_kernels();
    }
    return nullptr;
}

// the activation in front of a convolution: SnakeBeta with its folded parameters, or ELU (no parameters)
struct Snake {
    float *a = nullptr, *ib = nullptr;
    int act = ACT_SNAKE;
    bool aa = false;      // wrapped in Activation1d: a launch of its own (OobKernels::aa_act) behind the convolution, not that convolution's epilogue
};
struct ConvW {
    void* W = nullptr;
    float* bias = nullptr;
    int Cin = 0, Cout = 0, taps = 0, N = 0;      // Cin / Cout: the padded widths the kernels see
    const void* zero = nullptr;   // the plan's zero page (LDS-DMA source for padding rows)
};

}  // namespace

struct sat_oobleck_plan {
    const OobKernels* k = nullptr;      // the build of cfg.gemm_dtype
    sat_oobleck_cfg cfg;
    sat_oobleck_options opt;
    bool antialias = false;      // sat_oobleck_plan_set_antialias: the reference's antialias_activation=True
    TensorTable tensors;
    bool finalized = false;
    DevBuf arena;
    int ratio = 1;
    // decoder / encoder share the block structure
    ConvW first, last;
    float* first_w_f32 = nullptr;   // encoder first conv (VALU)
    struct Block {
        Snake sn_in;             // decoder: block snake before convT ; encoder: snake before strided conv
        ConvW resample;          // convT (decoder) / strided conv (encoder)
        Snake ru_sn1[3], ru_sn2[3];
        ConvW ru_c7[3], ru_c1[3];
        int stride, cin, cout;   // cin / cout: padded to multiples of 64
    };
    std::vector<Block> blocks;
    Snake final_snake;
    void* zero_page = nullptr;
    // optional fp16 range report (sat_oobleck_range_report): one record per activation tensor a run writes to the workspace, in launch order;
    // the names are fixed by the blocks (sat_oobleck_plan_create_ex), the records exist while the report is on
    std::vector<std::string> rr_names;
    DevBuf rr_buf;
    sat_range_record* rr = nullptr;
};
typedef sat_oobleck_plan OobPlan;

namespace {

int get_tensor(OobPlan* p, const std::string& name, int64_t numel, const float** out) { return p->tensors.get("oobleck", name, numel, out); }

// aa: one of the activations the reference builds with antialias=antialias_activation (get_activation, autoencoders.py:39-40).  Activation1d
// holds the activation as ".act"; its filter buffers are constants of the kernel and no plan tensors
int make_snake(OobPlan* p, Bump& ar, std::string pfx, int C, Snake* sn, hipStream_t s, bool aa = false) {
    sn->act = p->opt.activation;
    sn->aa = aa && p->antialias;
    if (sn->aa) pfx += "act.";
    if (sn->act == ACT_ELU) return 0;        // nn.ELU has no tensors: nothing to ask for
    const int Cp = pad64(C);
    sn->a = (float*)ar.take((size_t)Cp * 4);
    sn->ib = (float*)ar.take((size_t)Cp * 4);
    if (ar.dry()) return 0;
    const float *al, *be;
    SAT_TRY(get_tensor(p, pfx + "alpha", C, &al));
    SAT_TRY(get_tensor(p, pfx + "beta", C, &be));
    return p->k->snake_params(al, be, sn->a, sn->ib, C, Cp, s);
}

// bias[Cp]: the tensor's C values, then zeros
int make_bias(OobPlan* p, Bump& ar, const std::string& name, int C, float** out, hipStream_t s) {
    const int Cp = pad64(C);
    *out = (float*)ar.take((size_t)Cp * 4);
    if (ar.dry()) return 0;
    if (Cp > C) SAT_HIP(hipMemsetAsync(*out + C, 0, (size_t)(Cp - C) * 4, s));
    return p->tensors.copy("oobleck", name, C, *out, s);
}

// Conv1d weight [Cout][Cin][k]
int make_conv(OobPlan* p, Bump& ar, const std::string& pfx, int Cin, int Cout, int k, bool has_bias, ConvW* cw,
              hipStream_t s, float** w_f32 = nullptr) {
    const int Npad = pad64(Cout), Kpad = pad64(Cin);
    cw->Cin = Kpad; cw->Cout = Npad; cw->taps = k; cw->N = Npad; cw->zero = p->zero_page;
    float* scale = (float*)ar.take((size_t)Cout * 4);
    if (w_f32) *w_f32 = (float*)ar.take((size_t)Cout * Cin * k * 4);
    else cw->W = ar.take((size_t)k * Npad * Kpad * p->k->elem_bytes);
    cw->bias = nullptr;
    if (has_bias) SAT_TRY(make_bias(p, ar, pfx + "bias", Cout, &cw->bias, s));
    if (ar.dry()) return 0;
    const float *g, *v;
    SAT_TRY(get_tensor(p, pfx + "weight_g", Cout, &g));
    SAT_TRY(get_tensor(p, pfx + "weight_v", (int64_t)Cout * Cin * k, &v));
    if (w_f32) return p->k->fold_f32(v, g, scale, *w_f32, Cout, Cin * k, s);
    return p->k->pack_conv(v, g, scale, cw->W, Cout, Cin, k, Npad, Kpad, s);
}

// ConvTranspose1d weight [Cin][Cout][2s]
int make_convT(OobPlan* p, Bump& ar, const std::string& pfx, int Cin, int Cout, int stride, ConvW* cw, hipStream_t s) {
    const int Kp = pad64(Cin), Np = pad64(Cout);
    cw->Cin = Kp; cw->Cout = Np; cw->taps = 2; cw->N = stride * Np; cw->zero = p->zero_page;
    float* scale = (float*)ar.take((size_t)Cin * 4);
    cw->W = ar.take((size_t)2 * cw->N * Kp * p->k->elem_bytes);
    SAT_TRY(make_bias(p, ar, pfx + "bias", Cout, &cw->bias, s));
    if (ar.dry()) return 0;
    const float *g, *v;
    SAT_TRY(get_tensor(p, pfx + "weight_g", Cin, &g));
    SAT_TRY(get_tensor(p, pfx + "weight_v", (int64_t)Cin * Cout * 2 * stride, &v));
    return p->k->pack_convT(v, g, scale, cw->W, Cin, Cout, stride, Kp, Np, s);
}

// Upsample(nearest, s) + bias-free Conv1d weight [Cout][Cin][2s] -> the three-tap polyphase form
int make_nearest(OobPlan* p, Bump& ar, const std::string& pfx, int Cin, int Cout, int stride, ConvW* cw, hipStream_t s) {
    const int Kp = pad64(Cin), Np = pad64(Cout);
    cw->Cin = Kp; cw->Cout = Np; cw->taps = 3; cw->N = stride * Np; cw->zero = p->zero_page;
    float* scale = (float*)ar.take((size_t)Cout * 4);
    cw->W = ar.take((size_t)3 * cw->N * Kp * p->k->elem_bytes);
    cw->bias = nullptr;
    if (ar.dry()) return 0;
    const float *g, *v;
    SAT_TRY(get_tensor(p, pfx + "weight_g", Cout, &g));
    SAT_TRY(get_tensor(p, pfx + "weight_v", (int64_t)Cout * Cin * 2 * stride, &v));
    return p->k->pack_nearest(v, g, scale, cw->W, Cin, Cout, stride, Kp, Np, s);
}

int make_ru(OobPlan* p, Bump& ar, const std::string& pfx, int C, OobPlan::Block& blk, int r, hipStream_t s) {
    SAT_TRY(make_snake(p, ar, pfx + "layers.0.", C, &blk.ru_sn1[r], s));
    SAT_TRY(make_conv(p, ar, pfx + "layers.1.", C, C, 7, true, &blk.ru_c7[r], s));
    SAT_TRY(make_snake(p, ar, pfx + "layers.2.", C, &blk.ru_sn2[r], s));
    SAT_TRY(make_conv(p, ar, pfx + "layers.3.", C, C, 1, true, &blk.ru_c1[r], s));
    return 0;
}

// >= one K-tile row (<= 256 B) of zeros
int make_zero_page(OobPlan* p, Bump& ar, hipStream_t s) {
    p->zero_page = ar.take(256);
    if (!ar.dry()) SAT_HIP(hipMemsetAsync(p->zero_page, 0, 256, s));
    return 0;
}

int build(OobPlan* p, Bump& ar, hipStream_t s) {
    const sat_oobleck_cfg& c = p->cfg;
    const int nb = c.n_blocks;
    p->blocks.resize(nb);
    SAT_TRY(make_zero_page(p, ar, s));
    if (c.is_decoder) {
        // autoencoders.py:174-191: channel list c_mults=[1]+c_mults ; blocks from deepest to shallowest
        const int ctop = c.c_mults[nb - 1] * c.channels;
        SAT_TRY(make_conv(p, ar, "layers.0.", c.latent_dim, ctop, 7, true, &p->first, s));
        for (int bi = 0; bi < nb; ++bi) {
            const int i = nb - bi;   // reference loop index: range(depth-1, 0, -1)
            auto& blk = p->blocks[bi];
            const int cin = c.c_mults[i - 1] * c.channels;
            const int cout = (i - 2 >= 0 ? c.c_mults[i - 2] : 1) * c.channels;
            blk.cin = pad64(cin);
            blk.cout = pad64(cout);
            blk.stride = c.strides[i - 1];
            const std::string pf = "layers." + std::to_string(bi + 1) + ".";
            SAT_TRY(make_snake(p, ar, pf + "layers.0.", cin, &blk.sn_in, s, true));
            if (p->opt.nearest_upsample)      // Sequential(Upsample, WNConv1d): the convolution is layers.1.1
                SAT_TRY(make_nearest(p, ar, pf + "layers.1.1.", cin, cout, blk.stride, &blk.resample, s));
            else
                SAT_TRY(make_convT(p, ar, pf + "layers.1.", cin, cout, blk.stride, &blk.resample, s));
            for (int r = 0; r < 3; ++r) SAT_TRY(make_ru(p, ar, pf + "layers." + std::to_string(2 + r) + ".", cout, blk, r, s));
        }
        SAT_TRY(make_snake(p, ar, "layers." + std::to_string(nb + 1) + ".", c.channels, &p->final_snake, s, true));
        SAT_TRY(make_conv(p, ar, "layers." + std::to_string(nb + 2) + ".", c.channels, c.io_channels, 7, false, &p->last, s));
    } else {
        // autoencoders.py:131-151
        SAT_TRY(make_conv(p, ar, "layers.0.", c.io_channels, c.channels, 7, true, &p->first, s, &p->first_w_f32));
        for (int bi = 0; bi < nb; ++bi) {
            auto& blk = p->blocks[bi];
            const int cin = (bi == 0 ? 1 : c.c_mults[bi - 1]) * c.channels;
            const int cout = c.c_mults[bi] * c.channels;
            blk.cin = pad64(cin);
            blk.cout = pad64(cout);
            blk.stride = c.strides[bi];
            const std::string pf = "layers." + std::to_string(bi + 1) + ".";
            for (int r = 0; r < 3; ++r) SAT_TRY(make_ru(p, ar, pf + "layers." + std::to_string(r) + ".", cin, blk, r, s));
            SAT_TRY(make_snake(p, ar, pf + "layers.3.", cin, &blk.sn_in, s));
            SAT_TRY(make_conv(p, ar, pf + "layers.4.", cin, cout, 2 * blk.stride, true, &blk.resample, s));
        }
        const int ctop = c.c_mults[nb - 1] * c.channels;
        // (the reference's OobleckEncoder hands antialias_activation to this activation alone, autoencoders.py:139-148: its blocks are
        // built without it)
        SAT_TRY(make_snake(p, ar, "layers." + std::to_string(nb + 1) + ".", ctop, &p->final_snake, s, true));
        SAT_TRY(make_conv(p, ar, "layers." + std::to_string(nb + 2) + ".", ctop, c.latent_dim, 3, true, &p->last, s));
    }
    return 0;
}

struct Bufs {
    void *R, *S0, *S1, *Y;
    float* F;      // anti-aliased plans only: the fp32 un-activated tensor between a convolution and the activation's own kernel
    size_t total;
};
Bufs carve(const OobPlan* p, int B, int T, char* base) {
    // largest channels-last tensor of the network (padded widths), in elements per batch item
    const sat_oobleck_cfg& c = p->cfg;
    size_t len = (size_t)T, mx = 0, aa = 0;      // aa: the largest tensor in front of an anti-aliased activation
    if (c.is_decoder) {
        mx = std::max((size_t)T * pad64(c.latent_dim), (size_t)T * p->blocks[0].cin);
        aa = (size_t)T * p->blocks[0].cin;
        for (auto& b : p->blocks) {
            len *= b.stride;
            mx = std::max(mx, len * b.cout);
            aa = std::max(aa, len * b.cout);
        }
    } else {
        len = (size_t)T * p->ratio;
        mx = len * pad64(c.channels);
        for (auto& b : p->blocks) {
            mx = std::max(mx, len * b.cin);
            len /= b.stride;
            mx = std::max(mx, len * b.cout);
        }
        aa = len * p->blocks.back().cout;
    }
    size_t per = (size_t)round_up((int64_t)(mx * B * p->k->elem_bytes), 256);
    Bufs o;
    o.R = base ? base : nullptr;
    o.S0 = base ? base + per : nullptr;
    o.S1 = base ? base + 2 * per : nullptr;
    o.Y = base ? base + 3 * per : nullptr;
    o.total = 4 * per;
    o.F = nullptr;
    if (p->antialias) {      // the workspace grows only with the option on
        o.F = base ? (float*)(base + o.total) : nullptr;
        o.total += (size_t)round_up((int64_t)(aa * B * sizeof(float)), 256);
    }
    return o;
}

ConvArgs base_args(const ConvW& w, const void* in, int Tin, int M) {
    ConvArgs a{};
    a.zero_page = opq(w.zero);
    a.in = opq(in); a.Tin = Tin; a.Cin = w.Cin; a.W = opq(w.W); a.taps = w.taps; a.N = w.N; a.M = M;
    a.stride = 1; a.off0 = 0; a.doff = 1; a.bias = w.bias; a.Cout = w.Cout;
    a.out_bstride = (long long)M * w.N; a.out_shift = 0; a.out_limit = (long long)M * w.N;
    return a;
}

// out = the activated copy of the result, for the consumer whose activation is sn
void set_act(ConvArgs& a, void* out, const Snake& sn) {
    a.out_snk = opq(out); a.act = sn.act; a.sn_a = sn.a; a.sn_ib = sn.ib;
}
// The same where sn may be an anti-aliased activation: the convolution then writes its un-activated result in fp32 to `raw32` (Bufs::F: in
// the 16-bit builds the tensor would otherwise be rounded once more than in the fused epilogue, which the bf16 codec gate does not bear)
// and after_conv() turns it into `out` with one launch of the activation's own kernel
void set_act_or_raw(ConvArgs& a, void* out, float* raw32, const Snake& sn) {
    if (sn.aa) { a.out_cf = raw32; a.cf_channels = 0; }
    else set_act(a, out, sn);
}
int after_conv(const OobKernels* k, const Snake& sn, const float* raw32, void* out, int Cp, int L, int B, hipStream_t s) {
    return sn.aa ? k->aa_act(raw32, 1, out, sn.a, sn.ib, sn.act, Cp, L, B, s) : 0;
}

// ---- the ConvArgs of each layer kind.  decode / encode and the unit-level entry (sat_oobleck_unit) both build their launches from these, so
// a test of one layer runs the very off0 / doff / stride / M / out_shift / out_limit / out_bstride the plan runs
// k-tap convolution over the rows' own length, padding k / 2: the decoder's first and last k = 7, the encoder's last k = 3
ConvArgs same_conv_args(const ConvW& w, const void* in, int L) {
    ConvArgs a = base_args(w, in, L, L);
    a.off0 = -(w.taps / 2);
    return a;
}
// the last convolution of either direction: fp32 channel-first result, the first `channels` columns; tanh by option (decoder)
ConvArgs final_conv_args(const ConvW& w, const void* in, int L, float* out_cf, int channels, int tanh_out) {
    ConvArgs a = same_conv_args(w, in, L);
    a.out_cf = out_cf; a.cf_channels = channels; a.tanh_out = tanh_out;
    return a;
}
// the dilated k = 7 convolution of a ResidualUnit (autoencoders.py:56)
ConvArgs ru_c7_args(const ConvW& w, const void* S, int L, int dil) {
    ConvArgs a = base_args(w, S, L, L);
    a.off0 = -3 * dil; a.doff = dil;
    return a;
}
// its 1 x 1 convolution: adds the raw x in R; the sum returns to R in place where a later unit needs it
ConvArgs ru_c1_args(const ConvW& w, const void* Y, int L, void* R, bool need_raw) {
    ConvArgs c = base_args(w, Y, L, L);
    c.res = opq(R);
    c.out_raw = need_raw ? opq(R) : nullptr;   // in place: each thread reads then writes its own elements
    return c;
}
// a decoder block's upsampler, L rows -> L * st rows of w.Cout channels:
// transposed conv (autoencoders.py:102-105): rows m = 0..L, output row span (m*st - pad)*Cout, taps at rows m, m-1;
// nearest upsample + conv (:95-99): rows m = 0..L-1, output row span m*st*Cout, taps at rows m-1, m, m+1
ConvArgs upsample_args(const ConvW& w, const void* S, int L, int st, bool nearest) {
    const int pad = (st + 1) / 2;
    ConvArgs a = base_args(w, S, L, nearest ? L : L + 1);
    a.off0 = nearest ? -1 : 0; a.doff = nearest ? 1 : -1;
    a.out_bstride = (long long)L * st * w.Cout;
    a.out_shift = nearest ? 0 : -(long long)pad * w.Cout;
    a.out_limit = (long long)L * st * w.Cout;
    return a;
}
// an encoder block's strided convolution (autoencoders.py:80-81), L rows -> L / st rows
ConvArgs strided_args(const ConvW& w, const void* S, int L, int st) {
    ConvArgs a = base_args(w, S, L, L / st);
    a.stride = st; a.off0 = -((st + 1) / 2); a.doff = 1;
    return a;
}

// What the plan's length bookkeeping can run: a block turns L rows into L * st (decoder) or L / st (encoder).  The reference's
// ConvTranspose1d(k = 2 st, stride st, padding ceil(st / 2)) yields L * st + st - 2 ceil(st / 2) rows, which is L * st - 1 at odd st, and its
// encoder convolution yields L + 1 rows at st = 1; Upsample(st) + Conv1d("same") and the strided convolution at st >= 2 keep the plan's lengths.
bool resample_stride_ok(bool is_decoder, bool nearest, int st) {
    if (st < 1 || st > 16) return false;
    if (is_decoder) return nearest || st % 2 == 0;
    return st >= 2;
}

// The range report of one run: the next record takes the contiguous tensor of n elements at buf, right behind the launch that wrote it (the
// four workspace buffers are reused all along).  The order of the calls is the order of range_names
struct Ranger {
    const OobPlan* p;
    hipStream_t s;
    int next = 0;
    bool unfused = false;      // the unit-level entry's switch: the two-launch route without a report
    bool on() const { return p->rr != nullptr; }
    bool two_launches() const { return on() || unfused; }
    int operator()(const void* buf, size_t n) {
        if (!on()) return 0;
        SAT_CHECK_ARG(next < (int)p->rr_names.size(), SAT_E_STATE, "oobleck range report: more tensors than records (%d)", next);
        return sat_launch_range_stats(buf, p->k->dtype, 1, (int64_t)n, (int64_t)n, n, p->rr + next++, s);
    }
    int done() const {
        SAT_CHECK_ARG(!on() || next == (int)p->rr_names.size(), SAT_E_STATE, "oobleck range report: %d tensors for %d records", next, (int)p->rr_names.size());
        return 0;
    }
};

// The records of a plan in launch order (sat_oobleck_range_report_name): the module path of the layer whose launch writes the tensor -- the
// activated tensor the next convolution reads, then "<path>.raw" where the launch also keeps the un-activated sum for the next residual add
std::vector<std::string> range_names(const sat_oobleck_cfg& c, const sat_oobleck_options& o) {
    std::vector<std::string> n;
    auto both = [&](const std::string& path, bool raw) {
        n.push_back(path);
        if (raw) n.push_back(path + ".raw");
    };
    auto unit = [&](const std::string& ru, int r) {
        n.push_back(ru + "layers.1");
        both(ru + "layers.3", r < 2);
    };
    const int nb = c.n_blocks;
    if (c.is_decoder) {
        n.push_back("input");
        n.push_back("layers.0");
        for (int bi = 0; bi < nb; ++bi) {
            const std::string pf = "layers." + std::to_string(bi + 1) + ".";
            both(pf + (o.nearest_upsample ? "layers.1.1" : "layers.1"), true);
            for (int r = 0; r < 3; ++r) unit(pf + "layers." + std::to_string(2 + r) + ".", r);
        }
    } else {
        both("layers.0", true);
        for (int bi = 0; bi < nb; ++bi) {
            const std::string pf = "layers." + std::to_string(bi + 1) + ".";
            for (int r = 0; r < 3; ++r) unit(pf + "layers." + std::to_string(r) + ".", r);
            both(pf + "layers.4", bi + 1 < nb);
        }
    }
    return n;
}

// one ResidualUnit (autoencoders.py:45-68): in S (snaked x) + R (raw x) -> R (raw x') and/or Sout (snake_next(x'))
// With the range report on, every unit takes the two launches: the tensor between its convolutions then reaches memory (Y) and has a record
int run_ru(const OobPlan* p, const OobPlan::Block& blk, int r, int C, int L, int B, void* R, const void* S, void* Y, void* Sout, float* F,
           const Snake& next, bool need_raw, hipStream_t s, Ranger& rg) {
    static const int dil[3] = {1, 3, 9};
    ConvArgs a = ru_c7_args(blk.ru_c7[r], S, L, dil[r]);
    set_act(a, Y, blk.ru_sn2[r]);
    ConvArgs c = ru_c1_args(blk.ru_c1[r], Y, L, R, need_raw);
    set_act_or_raw(c, Sout, F, next);      // next.aa: the sum goes to F in fp32, the caller's after_conv() makes Sout of it
    // the whole unit in one launch where the build has the fused kernel and C is one of its tiles: the intermediate never leaves LDS
    if (p->k->ru_fused && (C == 128 || C == 256) && !rg.two_launches()) {
        RuArgs f{a, c};
        f.c7.out_snk = nullptr;
        f.c1.in = nullptr;
        return p->k->ru_fused(&f, B, s);
    }
    const size_t n = (size_t)B * L * C;
    SAT_TRY(p->k->conv(&a, B, s));
    SAT_TRY(rg(Y, n));
    SAT_TRY(p->k->conv(&c, B, s));
    SAT_TRY(rg(Sout, n));
    return need_raw ? rg(R, n) : 0;
}

// ---- sat_oobleck_unit: one layer on the caller's tensors (tests).  A plan object of its own holds the caller's fp32 tensors under fixed
// names ("conv." / "act.": the layer and the activation behind it; "conv2." / "act2.": a ResidualUnit's 1 x 1 convolution and the activation
// behind the unit), plan_finalize runs the make_* the plan's build() would run for that layer, and the launch goes through the helpers above
int oob_unit(const OobKernels* k, const sat_oobleck_unit_desc* u, sat_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    const int kind = u->kind, B = u->b, L = u->t_len, Ci = u->c_in, Co = u->c_out, st = u->stride;
    SAT_CHECK_ARG((kind >= SAT_OOBLECK_UNIT_CONV7 && kind <= SAT_OOBLECK_UNIT_CF_TO_CL) || kind == SAT_OOBLECK_UNIT_AA_ACT, SAT_E_UNSUPPORTED,
                  "oobleck_unit: unknown kind %d", kind);
    const bool aa = kind == SAT_OOBLECK_UNIT_AA_ACT, no_conv = aa || kind == SAT_OOBLECK_UNIT_CF_TO_CL;
    SAT_CHECK_ARG(u->activation == ACT_SNAKE || u->activation == ACT_ELU, SAT_E_UNSUPPORTED, "oobleck_unit: unknown activation %d", u->activation);
    SAT_CHECK_ARG(B > 0 && L > 0 && Ci > 0 && (Co > 0 || no_conv), SAT_E_INVALID, "oobleck_unit: b, t_len, c_in, c_out must be positive");
    const bool resample = kind == SAT_OOBLECK_UNIT_CONVT || kind == SAT_OOBLECK_UNIT_NEAREST || kind == SAT_OOBLECK_UNIT_STRIDED;
    const bool dilated = kind == SAT_OOBLECK_UNIT_CONV7 || kind == SAT_OOBLECK_UNIT_RESIDUAL;
    const bool residual = kind == SAT_OOBLECK_UNIT_CONV1_RES || kind == SAT_OOBLECK_UNIT_RESIDUAL;
    const bool from_cf = kind == SAT_OOBLECK_UNIT_FIRST_CONV || kind == SAT_OOBLECK_UNIT_CF_TO_CL;
    const bool to_cf = kind == SAT_OOBLECK_UNIT_FINAL_DEC || kind == SAT_OOBLECK_UNIT_FINAL_ENC;
    if (resample) {
        SAT_CHECK_ARG(resample_stride_ok(kind != SAT_OOBLECK_UNIT_STRIDED, kind == SAT_OOBLECK_UNIT_NEAREST, st), SAT_E_UNSUPPORTED,
                      "oobleck_unit: stride %d is outside what a plan runs for kind %d", st, kind);
        SAT_CHECK_ARG(kind != SAT_OOBLECK_UNIT_STRIDED || L % st == 0, SAT_E_INVALID, "oobleck_unit: t_len %d is no multiple of stride %d", L, st);
    }
    const int r = u->dilation == 1 ? 0 : u->dilation == 3 ? 1 : 2;
    SAT_CHECK_ARG(!dilated || u->dilation == 1 || u->dilation == 3 || u->dilation == 9, SAT_E_UNSUPPORTED, "oobleck_unit: dilation %d is not 1, 3 or 9", u->dilation);
    SAT_CHECK_ARG(!residual || (Ci == Co && u->res && (!u->out_raw || u->out_raw == u->res) && u->out_snk), SAT_E_INVALID,
                  "oobleck_unit: a residual layer needs c_in == c_out, res, out_snk, and out_raw NULL or == res");
    SAT_CHECK_ARG(kind != SAT_OOBLECK_UNIT_FIRST_CONV || (Ci <= 2 && u->out_raw && u->out_snk), SAT_E_INVALID,
                  "oobleck_unit: the first convolution takes 1 or 2 channels and writes out_raw and out_snk");
    SAT_CHECK_ARG(from_cf ? u->in_cf != nullptr : u->in != nullptr, SAT_E_INVALID, "oobleck_unit: input pointer missing");
    SAT_CHECK_ARG(to_cf ? u->out_cf != nullptr : (u->out_raw || u->out_snk), SAT_E_INVALID, "oobleck_unit: output pointer missing");
    SAT_CHECK_ARG(no_conv || (u->weight_g && u->weight_v), SAT_E_INVALID, "oobleck_unit: weight_g / weight_v missing");
    SAT_CHECK_ARG(!aa || (u->out_snk && u->out_snk != u->in), SAT_E_INVALID, "oobleck_unit: the anti-aliased activation writes out_snk, not in place");
    const bool has_bias = kind != SAT_OOBLECK_UNIT_NEAREST && kind != SAT_OOBLECK_UNIT_FINAL_DEC && !no_conv;
    SAT_CHECK_ARG(!has_bias || u->bias, SAT_E_INVALID, "oobleck_unit: bias missing");
    const bool act_behind = u->out_snk != nullptr;      // the activation whose result out_snk holds
    const bool snake = u->activation == ACT_SNAKE;
    SAT_CHECK_ARG(!(act_behind && snake && kind != SAT_OOBLECK_UNIT_RESIDUAL) || (u->alpha && u->beta), SAT_E_INVALID, "oobleck_unit: alpha / beta missing");
    if (kind == SAT_OOBLECK_UNIT_RESIDUAL)
        SAT_CHECK_ARG(u->weight_g2 && u->weight_v2 && u->bias2 && (!snake || (u->alpha && u->beta && u->alpha2 && u->beta2)), SAT_E_INVALID,
                      "oobleck_unit: a ResidualUnit needs both convolutions and both activations");

    OobPlan p;
    p.k = k;
    p.cfg = sat_oobleck_cfg{};
    p.cfg.gemm_dtype = u->gemm_dtype;
    p.opt = sat_oobleck_options{u->activation, u->final_tanh, kind == SAT_OOBLECK_UNIT_NEAREST};
    auto set = [&](const char* name, const float* ptr, int64_t n) { return ptr ? p.tensors.set("oobleck", name, ptr, n) : 0; };
    const int ktaps = kind == SAT_OOBLECK_UNIT_CONV1_RES ? 1 : kind == SAT_OOBLECK_UNIT_FINAL_ENC ? 3 : resample ? 2 * st : 7;
    if (aa) {
        p.antialias = true;
        SAT_TRY(set("act.alpha", u->alpha, Ci));
        SAT_TRY(set("act.beta", u->beta, Ci));
    } else if (kind != SAT_OOBLECK_UNIT_CF_TO_CL) {
        const int gdim = kind == SAT_OOBLECK_UNIT_CONVT ? Ci : Co;      // weight norm runs over dim 0: ConvTranspose1d weights are [c_in, c_out, k]
        SAT_TRY(set("conv.weight_g", u->weight_g, gdim));
        SAT_TRY(set("conv.weight_v", u->weight_v, (int64_t)Ci * Co * ktaps));
        if (has_bias) SAT_TRY(set("conv.bias", u->bias, Co));
        SAT_TRY(set("act.alpha", u->alpha, Co));
        SAT_TRY(set("act.beta", u->beta, Co));
    }
    if (kind == SAT_OOBLECK_UNIT_RESIDUAL) {
        SAT_TRY(set("conv2.weight_g", u->weight_g2, Co));
        SAT_TRY(set("conv2.weight_v", u->weight_v2, (int64_t)Co * Co));
        SAT_TRY(set("conv2.bias", u->bias2, Co));
        SAT_TRY(set("act2.alpha", u->alpha2, Co));
        SAT_TRY(set("act2.beta", u->beta2, Co));
    }
    OobPlan::Block blk;
    ConvW cw;
    Snake sn, next;
    float* w_f32 = nullptr;
    void* Y = nullptr;
    SAT_TRY(plan_finalize(&p, s, [&](Bump& ar) -> int {
        SAT_TRY(make_zero_page(&p, ar, s));
        if (kind == SAT_OOBLECK_UNIT_CF_TO_CL) return 0;
        if (aa) return make_snake(&p, ar, "", Ci, &sn, s, true);      // the plan's own packing; the tensors are "act.alpha" / "act.beta"
        if (kind == SAT_OOBLECK_UNIT_RESIDUAL) {
            SAT_TRY(make_conv(&p, ar, "conv.", Ci, Co, 7, true, &blk.ru_c7[r], s));
            SAT_TRY(make_snake(&p, ar, "act.", Co, &blk.ru_sn2[r], s));
            SAT_TRY(make_conv(&p, ar, "conv2.", Co, Co, 1, true, &blk.ru_c1[r], s));
            SAT_TRY(make_snake(&p, ar, "act2.", Co, &next, s));
            Y = ar.take((size_t)B * L * pad64(Co) * k->elem_bytes);
            return 0;
        }
        if (act_behind) SAT_TRY(make_snake(&p, ar, "act.", Co, &sn, s));
        if (kind == SAT_OOBLECK_UNIT_CONVT) return make_convT(&p, ar, "conv.", Ci, Co, st, &cw, s);
        if (kind == SAT_OOBLECK_UNIT_NEAREST) return make_nearest(&p, ar, "conv.", Ci, Co, st, &cw, s);
        return make_conv(&p, ar, "conv.", Ci, Co, ktaps, has_bias, &cw, s, kind == SAT_OOBLECK_UNIT_FIRST_CONV ? &w_f32 : nullptr);
    }));

    const void* in = u->in;
    void *res = const_cast<void*>(u->res), *out_raw = u->out_raw, *out_snk = u->out_snk;
    Ranger rg{&p, s};
    rg.unfused = u->two_launch != 0;
    ConvArgs a{};
    switch (kind) {
        case SAT_OOBLECK_UNIT_CF_TO_CL: SAT_TRY(k->cf_to_cl(u->in_cf, out_raw ? out_raw : out_snk, Ci, L, B, s)); break;
        case SAT_OOBLECK_UNIT_AA_ACT: SAT_TRY(k->aa_act(in, 0, out_snk, sn.a, sn.ib, sn.act, pad64(Ci), L, B, s)); break;
        case SAT_OOBLECK_UNIT_FIRST_CONV: SAT_TRY(k->first_conv(u->in_cf, w_f32, cw.bias, sn.a, sn.ib, sn.act, out_raw, out_snk, Ci, Co, L, B, s)); break;
        case SAT_OOBLECK_UNIT_RESIDUAL:
            SAT_TRY(run_ru(&p, blk, r, pad64(Co), L, B, res, in, Y, out_snk, nullptr, next, out_raw != nullptr, s, rg));
            break;
        case SAT_OOBLECK_UNIT_CONV7: a = ru_c7_args(cw, in, L, u->dilation); break;
        case SAT_OOBLECK_UNIT_CONV1_RES: a = ru_c1_args(cw, in, L, res, out_raw != nullptr); break;
        case SAT_OOBLECK_UNIT_CONVT: a = upsample_args(cw, in, L, st, false); break;
        case SAT_OOBLECK_UNIT_NEAREST: a = upsample_args(cw, in, L, st, true); break;
        case SAT_OOBLECK_UNIT_STRIDED: a = strided_args(cw, in, L, st); break;
        case SAT_OOBLECK_UNIT_FINAL_DEC: a = final_conv_args(cw, in, L, u->out_cf, Co, u->final_tanh != 0); break;
        default: a = final_conv_args(cw, in, L, u->out_cf, Co, 0); break;      // SAT_OOBLECK_UNIT_FINAL_ENC
    }
    if (a.W) {      // the kinds that are one launch of the convolution kernel
        if (!to_cf) {
            if (kind != SAT_OOBLECK_UNIT_CONV1_RES) a.out_raw = opq(out_raw);
            if (out_snk) set_act(a, out_snk, sn);
        }
        SAT_TRY(k->conv(&a, B, s));
    }
    SAT_HIP(hipStreamSynchronize(s));      // the arena goes with p
    return 0;
}

}  // namespace

// ---- C ABI
extern "C" int sat_oobleck_plan_create_ex(const sat_oobleck_cfg* cfg, const sat_oobleck_options* options, size_t options_bytes,
                                          sat_oobleck_plan** out_plan) {
    SAT_CHECK_ARG(cfg && out_plan, SAT_E_INVALID, "oobleck_plan_create: null argument");
    sat_oobleck_options opt = {SAT_OOBLECK_ACT_SNAKE, 0, 0};      // options == NULL: the defaults of sat_oobleck_plan_create
    if (options) {
        SAT_CHECK_ARG(options_bytes == sizeof(sat_oobleck_options), SAT_E_INVALID,
                      "oobleck_plan_create_ex: options_bytes %zu is not the size of this version's sat_oobleck_options (%zu)", options_bytes,
                      sizeof(sat_oobleck_options));
        opt = *options;
    }
    const OobKernels* k = kernels_of(cfg->gemm_dtype);
    SAT_CHECK_ARG(k, SAT_E_UNSUPPORTED, "oobleck_plan_create: gemm_dtype must be 0 (bf16), 3 (fp16) or 2 (fp32)");
    SAT_CHECK_ARG(opt.activation == SAT_OOBLECK_ACT_SNAKE || opt.activation == SAT_OOBLECK_ACT_ELU, SAT_E_UNSUPPORTED,
                  "oobleck_plan_create_ex: activation %d is neither SAT_OOBLECK_ACT_SNAKE (0) nor SAT_OOBLECK_ACT_ELU (1)", opt.activation);
    SAT_CHECK_ARG((opt.final_tanh == 0 || opt.final_tanh == 1) && (opt.nearest_upsample == 0 || opt.nearest_upsample == 1), SAT_E_UNSUPPORTED,
                  "oobleck_plan_create_ex: final_tanh / nearest_upsample must be 0 or 1");
    SAT_CHECK_ARG(cfg->is_decoder || (!opt.final_tanh && !opt.nearest_upsample), SAT_E_UNSUPPORTED,
                  "oobleck_plan_create_ex: final_tanh / nearest_upsample are decoder options");
    // (channel counts are free: the plan pads every width to a multiple of 64)
    SAT_CHECK_ARG(cfg->n_blocks >= 1 && cfg->n_blocks <= 8, SAT_E_UNSUPPORTED, "oobleck_plan_create: n_blocks %d not in 1..8", cfg->n_blocks);
    SAT_CHECK_ARG(cfg->channels > 0, SAT_E_UNSUPPORTED, "oobleck_plan_create: channels %d must be positive", cfg->channels);
    SAT_CHECK_ARG(cfg->io_channels >= 1 && cfg->io_channels <= 2, SAT_E_UNSUPPORTED, "oobleck_plan_create: io_channels must be 1 or 2");
    SAT_CHECK_ARG(cfg->latent_dim > 0, SAT_E_UNSUPPORTED, "oobleck_plan_create: latent_dim %d must be positive", cfg->latent_dim);
    int ratio = 1;
    for (int i = 0; i < cfg->n_blocks; ++i) {
        SAT_CHECK_ARG(cfg->strides[i] >= 1 && cfg->strides[i] <= 16 && cfg->c_mults[i] >= 1, SAT_E_UNSUPPORTED, "oobleck_plan_create: bad stride/c_mult");
        SAT_CHECK_ARG(resample_stride_ok(cfg->is_decoder != 0, opt.nearest_upsample != 0, cfg->strides[i]), SAT_E_UNSUPPORTED,
                      "oobleck_plan_create: stride %d of block %d is not supported: the reference's %s", cfg->strides[i], i,
                      cfg->is_decoder ? "ConvTranspose1d yields L * stride - 1 samples at an odd stride, the plan L * stride (nearest_upsample takes odd strides)"
                                      : "stride-1 encoder convolution (k = 2, padding 1) yields L + 1 samples, the plan L");
        ratio *= cfg->strides[i];
    }
    OobPlan* p = new (std::nothrow) OobPlan();
    SAT_CHECK_ARG(p, SAT_E_INVALID, "oobleck_plan_create: out of host memory");
    p->k = k;
    p->cfg = *cfg;
    p->opt = opt;
    p->rr_names = range_names(*cfg, opt);
    p->ratio = ratio;
    *out_plan = p;
    return 0;
}
// The original entry point and its contract: Snake, transposed convolutions, no tanh, channels and the decoder's latent_dim multiples of 64
extern "C" int sat_oobleck_plan_create(const sat_oobleck_cfg* cfg, sat_oobleck_plan** out_plan) {
    SAT_CHECK_ARG(cfg && out_plan, SAT_E_INVALID, "oobleck_plan_create: null argument");
    SAT_CHECK_ARG(kernels_of(cfg->gemm_dtype), SAT_E_UNSUPPORTED, "oobleck_plan_create: gemm_dtype must be 0 (bf16), 3 (fp16) or 2 (fp32)");
    SAT_CHECK_ARG(cfg->channels % 64 == 0 && cfg->channels > 0, SAT_E_UNSUPPORTED,
                  "oobleck_plan_create: channels %d must be a multiple of 64 (sat_oobleck_plan_create_ex takes any)", cfg->channels);
    if (cfg->is_decoder)
        SAT_CHECK_ARG(cfg->latent_dim % 64 == 0, SAT_E_UNSUPPORTED,
                      "oobleck_plan_create: decoder latent_dim %d must be a multiple of 64 (sat_oobleck_plan_create_ex takes any)", cfg->latent_dim);
    return sat_oobleck_plan_create_ex(cfg, nullptr, 0, out_plan);
}
extern "C" int sat_oobleck_plan_set_antialias(sat_oobleck_plan* p, int32_t enable) {
    SAT_CHECK_ARG(p, SAT_E_INVALID, "oobleck_plan_set_antialias: null plan");
    SAT_CHECK_ARG(!p->finalized, SAT_E_STATE, "oobleck_plan_set_antialias: the plan is finalized");
    SAT_CHECK_ARG(enable == 0 || enable == 1, SAT_E_UNSUPPORTED, "oobleck_plan_set_antialias: enable must be 0 or 1, got %d", enable);
    SAT_CHECK_ARG(!enable || !p->rr, SAT_E_UNSUPPORTED, "oobleck_plan_set_antialias: the range report is on and has no records for the anti-aliased tensors");
    p->antialias = enable != 0;
    return 0;
}
extern "C" void sat_oobleck_plan_destroy(sat_oobleck_plan* p) { delete p; }
extern "C" int sat_oobleck_plan_set_tensor(sat_oobleck_plan* p, const char* name, const float* data_dev, int64_t numel) {
    SAT_CHECK_ARG(p, SAT_E_INVALID, "oobleck_plan_set_tensor: null plan");
    return p->tensors.set("oobleck", name, data_dev, numel);
}
extern "C" int sat_oobleck_plan_finalize(sat_oobleck_plan* p, sat_stream_t stream) {
    SAT_CHECK_ARG(p, SAT_E_INVALID, "oobleck_plan_finalize: null plan");
    hipStream_t s = (hipStream_t)stream;
    return plan_finalize(p, s, [&](Bump& ar) { return build(p, ar, s); });
}
extern "C" int sat_oobleck_workspace_bytes(const sat_oobleck_plan* p, int32_t b, int32_t t_len, size_t* out_bytes) {
    SAT_CHECK_ARG(p, SAT_E_INVALID, "oobleck_workspace_bytes: null plan");
    SAT_CHECK_ARG(out_bytes && b > 0 && t_len > 0, SAT_E_INVALID, "oobleck_workspace_bytes: bad argument");
    SAT_CHECK_ARG(p->finalized, SAT_E_STATE, "oobleck_workspace_bytes: plan not finalized");
    *out_bytes = carve(p, b, t_len, nullptr).total;
    return 0;
}
extern "C" int sat_oobleck_decode(sat_oobleck_plan* p, const float* z, float* audio, int32_t B, int32_t T, void* ws, size_t ws_bytes,
                                  sat_stream_t stream) {
    SAT_CHECK_ARG(p, SAT_E_INVALID, "oobleck_decode: null plan");
    SAT_CHECK_ARG(p->finalized && p->cfg.is_decoder, SAT_E_STATE, "oobleck_decode: not a finalized decoder plan");
    SAT_CHECK_ARG(z && audio && ws && B > 0 && T > 0, SAT_E_INVALID, "oobleck_decode: bad arguments");
    SAT_CHECK_ARG(((uintptr_t)ws & 255) == 0, SAT_E_INVALID, "oobleck_decode: workspace must be 256-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    Bufs bf = carve(p, B, T, (char*)ws);
    SAT_CHECK_ARG(ws_bytes >= bf.total, SAT_E_WORKSPACE, "oobleck_decode: workspace %zu < required %zu", ws_bytes, bf.total);
    const sat_oobleck_cfg& c = p->cfg;
    const OobKernels* k = p->k;
    const int nb = c.n_blocks;
    // latents -> channels-last operand rows (in Y), first conv (autoencoders.py:175) -> S0 = snake_block1(x)
    SAT_TRY(k->cf_to_cl(z, bf.Y, c.latent_dim, T, B, s));
    Ranger rg{p, s};
    SAT_TRY(rg(bf.Y, (size_t)B * T * pad64(c.latent_dim)));
    void* S = bf.S0;
    void* Sn = bf.S1;
    {
        ConvArgs a = same_conv_args(p->first, bf.Y, T);
        set_act_or_raw(a, S, bf.F, p->blocks[0].sn_in);
        SAT_TRY(k->conv(&a, B, s));
        SAT_TRY(after_conv(k, p->blocks[0].sn_in, bf.F, S, p->first.Cout, T, B, s));
        SAT_TRY(rg(S, (size_t)B * T * p->first.Cout));
    }
    int L = T;
    for (int bi = 0; bi < nb; ++bi) {
        const auto& blk = p->blocks[bi];
        const int st = blk.stride;
        ConvArgs a = upsample_args(blk.resample, S, L, st, p->opt.nearest_upsample != 0);
        a.out_raw = opq(bf.R);
        set_act(a, Sn, blk.ru_sn1[0]);
        SAT_TRY(k->conv(&a, B, s));
        std::swap(S, Sn);
        L *= st;
        SAT_TRY(rg(S, (size_t)B * L * blk.cout));
        SAT_TRY(rg(bf.R, (size_t)B * L * blk.cout));
        for (int r = 0; r < 3; ++r) {
            const Snake& next = r < 2 ? blk.ru_sn1[r + 1] : (bi + 1 < nb ? p->blocks[bi + 1].sn_in : p->final_snake);
            SAT_TRY(run_ru(p, blk, r, blk.cout, L, B, bf.R, S, bf.Y, Sn, bf.F, next, r < 2, s, rg));
            SAT_TRY(after_conv(k, next, bf.F, Sn, blk.cout, L, B, s));
            std::swap(S, Sn);
        }
    }
    // final conv (autoencoders.py:187-188): no bias, tanh by option -> fp32 channel-first audio
    ConvArgs a = final_conv_args(p->last, S, L, audio, c.io_channels, p->opt.final_tanh);
    SAT_TRY(k->conv(&a, B, s));
    return rg.done();
}
extern "C" int sat_oobleck_encode(sat_oobleck_plan* p, const float* audio, float* out, int32_t B, int32_t T, void* ws, size_t ws_bytes,
                                  sat_stream_t stream) {
    SAT_CHECK_ARG(p, SAT_E_INVALID, "oobleck_encode: null plan");
    SAT_CHECK_ARG(p->finalized && !p->cfg.is_decoder, SAT_E_STATE, "oobleck_encode: not a finalized encoder plan");
    SAT_CHECK_ARG(audio && out && ws && B > 0 && T > 0, SAT_E_INVALID, "oobleck_encode: bad arguments");
    SAT_CHECK_ARG(((uintptr_t)ws & 255) == 0, SAT_E_INVALID, "oobleck_encode: workspace must be 256-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    Bufs bf = carve(p, B, T, (char*)ws);
    SAT_CHECK_ARG(ws_bytes >= bf.total, SAT_E_WORKSPACE, "oobleck_encode: workspace %zu < required %zu", ws_bytes, bf.total);
    const sat_oobleck_cfg& c = p->cfg;
    const OobKernels* k = p->k;
    const int nb = c.n_blocks;
    int L = T * p->ratio;
    void* S = bf.S0;
    void* Sn = bf.S1;
    const Snake& sn0 = p->blocks[0].ru_sn1[0];
    SAT_TRY(k->first_conv(audio, p->first_w_f32, p->first.bias, sn0.a, sn0.ib, sn0.act, bf.R, S, c.io_channels, c.channels, L, B, s));
    Ranger rg{p, s};
    SAT_TRY(rg(S, (size_t)B * L * pad64(c.channels)));
    SAT_TRY(rg(bf.R, (size_t)B * L * pad64(c.channels)));
    for (int bi = 0; bi < nb; ++bi) {
        const auto& blk = p->blocks[bi];
        for (int r = 0; r < 3; ++r) {
            const Snake& next = r < 2 ? blk.ru_sn1[r + 1] : blk.sn_in;
            SAT_TRY(run_ru(p, blk, r, blk.cin, L, B, bf.R, S, bf.Y, Sn, bf.F, next, r < 2, s, rg));
            std::swap(S, Sn);
        }
        const int st = blk.stride;
        const int Lo = L / st;
        ConvArgs a = strided_args(blk.resample, S, L, st);
        const bool lastb = bi + 1 == nb;
        a.out_raw = lastb ? nullptr : opq(bf.R);
        const Snake& nx = lastb ? p->final_snake : p->blocks[bi + 1].ru_sn1[0];
        set_act_or_raw(a, Sn, bf.F, nx);
        SAT_TRY(k->conv(&a, B, s));
        SAT_TRY(after_conv(k, nx, bf.F, Sn, blk.cout, Lo, B, s));
        std::swap(S, Sn);
        L = Lo;
        SAT_TRY(rg(S, (size_t)B * L * blk.cout));
        if (!lastb) SAT_TRY(rg(bf.R, (size_t)B * L * blk.cout));
    }
    ConvArgs a = final_conv_args(p->last, S, L, out, c.latent_dim, 0);
    SAT_TRY(k->conv(&a, B, s));
    return rg.done();
}

// ---- sat_oobleck_range_report and its companions
extern "C" int sat_oobleck_range_report(sat_oobleck_plan* p, int32_t enable) {
    SAT_CHECK_ARG(p, SAT_E_INVALID, "oobleck_range_report: null plan");
    SAT_CHECK_ARG(enable >= 0 && enable <= 2, SAT_E_INVALID, "oobleck_range_report: enable must be 0 (off), 1 (on) or 2 (zero the records), got %d", enable);
    if (enable == 0) {
        if (!p->rr) return 0;
        SAT_HIP(hipDeviceSynchronize());          // launches in flight still accumulate into the records
        p->rr_buf.release();
        p->rr = nullptr;
        return 0;
    }
    SAT_CHECK_ARG(sat_launch_range_stats, SAT_E_UNSUPPORTED, "oobleck_range_report: built without the range statistics kernel");
    SAT_CHECK_ARG(!p->antialias, SAT_E_UNSUPPORTED, "oobleck_range_report: no records for the tensors of an anti-aliased plan (sat_oobleck_plan_set_antialias)");
    const size_t bytes = p->rr_names.size() * sizeof(sat_range_record);
    if (enable == 2) {
        SAT_CHECK_ARG(p->rr, SAT_E_STATE, "oobleck_range_report: the report is not enabled, there is nothing to zero");
        SAT_HIP(hipDeviceSynchronize());
        SAT_HIP(hipMemset(p->rr, 0, bytes));
        return 0;
    }
    if (p->rr) return 0;          // already on: the records keep accumulating
    SAT_TRY(p->rr_buf.reserve(bytes));
    SAT_HIP(hipMemset(p->rr_buf.ptr, 0, bytes));
    p->rr = (sat_range_record*)p->rr_buf.ptr;
    return 0;
}
extern "C" int sat_oobleck_range_report_count(const sat_oobleck_plan* p, int32_t* out_records) {
    SAT_CHECK_ARG(p, SAT_E_INVALID, "oobleck_range_report_count: null plan");
    SAT_CHECK_ARG(out_records, SAT_E_INVALID, "oobleck_range_report_count: null argument");
    *out_records = (int32_t)p->rr_names.size();
    return 0;
}
extern "C" const char* sat_oobleck_range_report_name(const sat_oobleck_plan* p, int32_t index) {
    if (!p) return nullptr;
    return index >= 0 && index < (int32_t)p->rr_names.size() ? p->rr_names[index].c_str() : nullptr;
}
extern "C" int sat_oobleck_range_report_read(sat_oobleck_plan* p, sat_range_record* out_host, int32_t capacity_records, size_t record_bytes,
                                             sat_stream_t stream) {
    SAT_CHECK_ARG(p, SAT_E_INVALID, "oobleck_range_report_read: null plan");
    SAT_CHECK_ARG(out_host, SAT_E_INVALID, "oobleck_range_report_read: null argument");
    SAT_CHECK_ARG(record_bytes == sizeof(sat_range_record), SAT_E_INVALID,
                  "oobleck_range_report_read: sat_range_record of %zu bytes; this library knows %zu", record_bytes, sizeof(sat_range_record));
    const int n = (int)p->rr_names.size();
    SAT_CHECK_ARG(capacity_records >= n, SAT_E_INVALID, "oobleck_range_report_read: room for %d records, need %d", capacity_records, n);
    SAT_CHECK_ARG(p->rr, SAT_E_STATE, "oobleck_range_report_read: the report is not enabled (sat_oobleck_range_report)");
    SAT_HIP(hipMemcpyAsync(out_host, p->rr, (size_t)n * sizeof(sat_range_record), hipMemcpyDeviceToHost, (hipStream_t)stream));
    SAT_HIP(hipStreamSynchronize((hipStream_t)stream));
    return 0;
}
// one layer alone (tests): the descriptor's gemm_dtype picks the build, as a plan's does
extern "C" int sat_oobleck_unit(const sat_oobleck_unit_desc* desc, size_t desc_bytes, sat_stream_t stream) {
    SAT_CHECK_ARG(desc, SAT_E_INVALID, "oobleck_unit: null descriptor");
    SAT_CHECK_ARG(desc_bytes == sizeof(sat_oobleck_unit_desc), SAT_E_INVALID,
                  "oobleck_unit: desc_bytes %zu is not the size of this version's sat_oobleck_unit_desc (%zu)", desc_bytes, sizeof(sat_oobleck_unit_desc));
    const OobKernels* k = kernels_of(desc->gemm_dtype);
    SAT_CHECK_ARG(k, SAT_E_UNSUPPORTED, "oobleck_unit: gemm_dtype must be 0 (bf16), 3 (fp16) or 2 (fp32)");
    return oob_unit(k, desc, stream);
}
