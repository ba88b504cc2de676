"""The single-kernel cases of the fp32 path (csrc/f32_ref.hip), the text-encoder kernels (enc_attention.h, t5_encoder.hip, roberta_encoder.hip)
and the DiT glue (dit_glue.hip): shapes, seeded inputs, a restatement of every operation in plain PyTorch, and the gates.  The device test
(test_gpu_fp32_kernels.py) runs each kernel through its unit entry of include/sat_hip.h and compares with ``reference(case)`` in float64; the host
test (test_fp32_kernels_host.py) proves the references against the modules they stand for, shows that the same restatement evaluated in
float32 on the CPU passes every gate with a factor 4 to spare, and that the gates reject the faults these kernels can have.

``reference(case, dtype)`` is written from the operation, never from the kernel, and is generic in the dtype: float64 is the reference, float32
the CPU evaluation of the condition on the inputs.  It returns {output name: tensor}; for a contraction also "<name>:mag", the float64 magnitude
|A| |W|^T + |bias| + |C_in| (times |gate|) of the a-priori bound, and "<name>:n", the number of accumulated terms.

Gates (``check``), none of them tuned on a kernel:
  contraction  every element |got - want| <= (n + 4) 2^-24 mag, which holds for any summation order and for FMA chains; and every row and every
               32 x 32 block at 1e-5 (util.assert_close_sliced on rows and on util.blocks32)
  other fp32   1e-5 per slice (util.assert_close_sliced): per (batch, query, head) for attention, per row for the row kernels, per element --
               |err| <= 1e-5 max(|want|, rms(want)) -- for the elementwise ones.  1e-5 is the gate of the project's other fp32 kernels
  16 bit       at most one code of the format from the correctly rounded float64 result, at most 1 % of the elements different at all
  exact        torch.equal
``headroom`` scales the 1e-5 gates: 0.25 for the condition on the inputs.  The a-priori bound is not scaled: it is a theorem about every fp32
evaluation, the CPU's included, and a factor 4 cannot exist at n = 2, where the products, their sum and the scaling can each be a unit
(2^-24 of the magnitude) off: three against the bound's seven."""
import math
import zlib

import torch
import torch.nn.functional as F

from util import assert_close_sliced, blocks32

TOL = 1e-5
UNIT = 2.0 ** -24
MODEL_GATE = 1e-4          # the whole-tensor gate of the fp32x model test (test_gpu_models.py): what a planted fault has to stay under

LOG = []                   # (case name, output, what, figure, where): filled by check(), written out by the tests under SAT_PARITY_LOG


def _product(**axes):
    out = [{}]
    for k, vals in axes.items():
        out = [dict(o, **{k: v}) for o in out for v in vals]
    return out


def case_id(p):
    return "-".join(f"{k}{v}" for k, v in p.items()) or "only"


def _gen(kind, p):
    return torch.Generator().manual_seed(zlib.crc32(repr((kind, sorted(p.items()))).encode()))


def _rand(gen, *shape):
    return torch.randn(shape, generator=gen)


# ------------------------------------------------------------------------------------------------------------------------ the cases
# gemm_f32: tile 128 x 128, K-step 16, two LDS stages.  (130, 136, 48): a 2-row and an 8-column tail, three K-steps (both stages reused);
# (1, 8, 16): one row, one K-step (the loop body never runs); (128, 128, 32): exactly one tile; (257, 129, 512): 3 x 2 tiles with one-row /
# one-column tails.  gate_rows = 65 puts the m / gate_rows boundary inside a tile, gate_ld = 3 N
_GEMM_SHAPES = [(130, 136, 48), (1, 8, 16), (128, 128, 32), (257, 129, 512)]
_GEMM_MODES = [dict(bias=1, acc=0, gate=1), dict(bias=0, acc=1, gate=1), dict(bias=1, acc=1, gate=0), dict(bias=0, acc=0, gate=0)]
# small_linear: one wave per output column, 8 rows per wave, 256 k per pass.  (1, 5, 4): one lane works; (9, 7, 260): a second row block
# of one row, a second k pass of 4; (17, 130, 512): three row blocks, 33 column blocks
_SL_SHAPES = [(1, 5, 4), (9, 7, 260), (17, 130, 512)]
_SL_MODES = [dict(act=0, bias=1, add=1, out16=0), dict(act=1, bias=1, add=0, out16=0), dict(act=2, bias=1, add=1, out16=0),
             dict(act=0, bias=0, add=0, out16=0), dict(act=0, bias=1, add=0, out16=1), dict(act=0, bias=0, add=0, out16=2),
             dict(act=1, bias=1, add=1, out16=1), dict(act=2, bias=0, add=1, out16=2)]

CASES = {
    "gemm_f32": [dict(m=m, n=n, k=k, **mode) for (m, n, k) in _GEMM_SHAPES for mode in _GEMM_MODES],
    "layernorm_f32": ([dict(m=m, d=d, eps=eps, var=var) for (m, d) in ((5, 64), (7, 100), (37, 256)) for eps in (1e-5, 1e-6)
                       for var in ("plain", "nobeta", "mod")] + [dict(m=37, d=256, eps=1e-5, var="mean30")]),
    "split_heads_f32": [dict(parts=a, rope=b, norm=c) for (a, b, c) in ((3, 3, 0), (3, 3, 3), (2, 0, 0), (1, 0, 1))],
    "swiglu_f32": [dict(m=3, inner=100), dict(m=7, inner=330)],
    "attention_f32": ([dict(b=b, h=h, kvh=kvh, sq=sq, sk=sk, var="plain") for (b, h, kvh, sq, sk) in
                       ((2, 4, 2, 70, 77), (1, 2, 1, 1, 1), (1, 2, 2, 64, 8), (1, 4, 4, 129, 7))]
                      + [dict(b=2, h=4, kvh=2, sq=70, sk=77, var="max_last"), dict(b=2, h=4, kvh=2, sq=70, sk=77, var="negative")]),
    "enc_attention": _product(l=[1, 19, 64, 65, 130, 512], dkv=[64, 40], style=["t5", "roberta"], masks=["full+tail", "one+allpad"]),
    "t5_embed": [dict(rows=9, d=64)],
    "t5_rmsnorm": [dict(m=5, d=512), dict(m=3, d=768), dict(m=1, d=4)],
    "t5_position_bias": [dict(h=3, l=19)],
    "t5_act": [dict(rows=3, f=100, gated=0), dict(rows=3, f=100, gated=1), dict(rows=5, f=330, gated=1)],
    "t5_mask_rows": [dict(rows=11, d=100)],
    "roberta_embed_ln": [dict(table="random"), dict(table="onehot")],
    "roberta_gelu": [dict(n=1000), dict(n=77)],
    "small_linear": [dict(r=r, n=n, k=k, **mode) for (r, n, k) in _SL_SHAPES for mode in _SL_MODES],
    "adaln_finish": [dict(b=3, layers=2, d=100)],
    "fourier": [dict(t="per_batch"), dict(t="const")],
    "fold_in": _product(d=[128, 384], c=[2, 64]),
    "fold_out": _product(d=[128, 384], c=[2, 4, 64]),
    "input_proj": _product(c=[2, 64], t=[1, 8, 13, 77], d=[128, 384], pre=[0, 1]),
    "input_proj_extra": [dict(c=c, t=t, d=d, tc=tc, p=p, pre=pre) for c in (2, 64) for t in (1, 8, 13, 77) for d in (128, 384)
                         for tc in ("t", 5, 200) for p in (0, 3, 9) for pre in ((0, 1) if p == 0 else (1,))],
    "output_proj": _product(c=[4, 8, 64], d=[128, 256, 1536], pre=[0, 1, 4]),
    "pos_table": [dict(mode=1), dict(mode=2)],
    "add_pos": [dict(mode=1), dict(mode=2)],
    "cfg_denoise": _product(use_cfg=[0, 1], phi=[0.0, 0.6]),
}
KINDS = tuple(CASES)
CONTRACTIONS = ("gemm_f32", "small_linear", "input_proj", "input_proj_extra", "output_proj", "fold_in", "fold_out")
GATE_ROWS = 65


class Case:
    """kind + parameters -> seeded inputs ``t`` (CPU tensors: fp32, or int32 for ids / masks) and the dimensions ``dim`` the entry is called with."""

    def __init__(self, kind, p):
        self.kind, self.p = kind, dict(p)
        self.name = f"{kind} {case_id(p)}"
        self.t, self.dim = {}, {}
        getattr(self, "_" + kind)(_gen(kind, p), self.p, self.t, self.dim)
        # a scalar reaches its kernel as a float: the reference takes that fp32 image too (0.37 and fl32(0.37) are a whole unit apart)
        self.dim = {k: float(torch.tensor(v, dtype=torch.float32)) if isinstance(v, float) else v for k, v in self.dim.items()}

    def _gemm_f32(self, g, p, t, d):
        m, n, k = p["m"], p["n"], p["k"]
        t["a"], t["w"] = _rand(g, m, k), _rand(g, n, k) * 0.2
        t["bias"] = _rand(g, n) if p["bias"] else None
        t["c_in"] = _rand(g, m, n) * 2.0 if p["acc"] else None
        # |gate| in [0.5, 1.5]: (n + 4) |gate| >= 1, so the rounding of the final addition to C_in stays inside the bound as the issue states it
        gate = (0.5 + torch.rand((math.ceil(m / GATE_ROWS), 3 * n), generator=g)) * torch.where(torch.rand((1, 3 * n), generator=g) < 0.5, -1.0, 1.0)
        t["gate"] = gate if p["gate"] else None
        d.update(m=m, n=n, k=k, ldc=n + 8)

    def _layernorm_f32(self, g, p, t, d):
        m, dd = p["m"], p["d"]
        x = _rand(g, m, dd)
        if p["var"] == "mean30":
            # mean 30, std 1, on a grid of 2^-10: every fp32 partial sum of a row is exact in any order, so the case is about the formula (a
            # variance from E[x^2] - mean^2 loses five digits here) and not about how a mean near 30 happens to round (half a unit there is
            # 1e-6 of the row's std, which would leave the fp32 evaluation of the condition 3e-6 on some rows)
            x = torch.round((x + 30.0) * 1024.0) / 1024.0
        else:
            x = x * (0.5 + torch.rand((m, 1), generator=g) * 4.0) + _rand(g, m, 1)
        t["x"], t["gamma"] = x, 1.0 + 0.3 * _rand(g, dd)
        t["beta"] = None if p["var"] == "nobeta" else 0.3 * _rand(g, dd)
        rps, ld = 3, dd + 8
        if p["var"] == "mod":
            t["scale"], t["shift"] = 1.0 + 0.3 * _rand(g, math.ceil(m / rps), ld), 0.3 * _rand(g, math.ceil(m / rps), ld)
        else:
            t["scale"] = t["shift"] = None
        d.update(m=m, d=dd, rps=rps, ld=ld, eps=p["eps"])

    def _split_heads_f32(self, g, p, t, d):
        b, s, h = 2, 37, 3
        t["src"] = _rand(g, b * s, p["parts"] * h * 64)
        t["src"][b * s // 2:] *= 8.0            # item 1 is 8 x item 0: a row taken from the neighbouring sequence dominates
        ang = torch.arange(s, dtype=torch.float64)[:, None] * (10000.0 ** (-torch.arange(16, dtype=torch.float64) / 16.0))[None, :]
        t["cos"], t["sin"] = ang.cos().float(), ang.sin().float()
        d.update(b=b, s=s, h=h)

    def _swiglu_f32(self, g, p, t, d):
        hg = _rand(g, p["m"], 2 * p["inner"]) * 3.0
        hg[0, p["inner"]:p["inner"] + 8] = torch.tensor([-30.0, -14.0, -12.5, -8.0, 8.0, 12.5, 14.0, 30.0])
        t["hg"] = hg

    def _attention_f32(self, g, p, t, d):
        b, h, kvh, sq, sk = (p[k] for k in ("b", "h", "kvh", "sq", "sk"))
        q, k, v = _rand(g, b, h, sq, 64), _rand(g, b, kvh, sk, 64), _rand(g, b, kvh, sk, 64)
        if p["var"] == "max_last":
            # the LAST channel of every query and key is 22: every score is 22 * 22 / 8 = 60.5 plus the N(0, 1) of the other channels; key sk - 3
            # (the last chunk of 8) holds 25 there, 8.25 above the rest: the running maximum arrives last.  (The large product enters a sum of
            # small ones, so a score carries one rounding at 60 and not 64: that keeps the fp32 evaluation inside the condition on the inputs.)
            q[..., 63], k[..., 63] = 22.0, 22.0
            k[:, :, sk - 3, 63] = 25.0
        elif p["var"] == "negative":
            # all scores about -30: a running maximum that does not start at -inf loses every weight
            q[..., 0], k[..., 0] = 16.0, -15.0
        if p["var"] != "plain":
            v = v + 1.0
        if b > 1:
            v[1] = v[1] * 8.0            # a value row of the neighbouring sequence dominates
        t.update(q=q, k=k, v=v)

    def _enc_attention(self, g, p, t, d):
        b, l, h, dkv = 2, p["l"], 3, p["dkv"]
        inner = h * dkv
        qkv = _rand(g, b, l, 3 * inner) * 0.5
        mask = torch.ones((b, l), dtype=torch.int32)
        for i, kind in enumerate(p["masks"].split("+")):
            if kind == "tail":
                mask[i, (l + 1) // 2:] = 0            # (l = 1: nothing is padded)
            elif kind == "one":
                mask[i] = 0
                mask[i, l // 3] = 1
            elif kind == "allpad":
                mask[i] = 0
        # K and V rows of masked keys hold 1e4, so a leak shows -- except in an all-padding sequence, whose rows stay ordinary and distinct: there
        # every key counts, and only the uniform average over all l of them gives the expected row
        pad = ((mask == 0) & (mask.sum(dim=1, keepdim=True) > 0))[:, :, None].expand(b, l, 2 * inner)
        qkv[:, :, inner:] = torch.where(pad, torch.full((), 1e4), qkv[:, :, inner:])
        t["qkv"], t["mask"] = qkv, mask
        t["pb"] = _rand(g, h, 2 * l - 1) if p["style"] == "t5" else None
        d.update(b=b, l=l, h=h, dkv=dkv, scale=1.0 if p["style"] == "t5" else dkv ** -0.5)

    def _t5_embed(self, g, p, t, d):
        vocab = 13
        t["emb"] = _rand(g, vocab, p["d"])
        t["ids"] = torch.tensor([0, 12, 5, 5, -3, 13, 40, 7, 1], dtype=torch.int32)            # out-of-range ids are clamped
        d.update(vocab=vocab)

    def _t5_rmsnorm(self, g, p, t, d):
        t["x"] = _rand(g, p["m"], p["d"]) * (0.2 + 5.0 * torch.rand((p["m"], 1), generator=g))
        t["w"] = 1.0 + 0.3 * _rand(g, p["d"])
        d.update(eps=1e-6)

    def _t5_position_bias(self, g, p, t, d):
        buckets, n = 32, 2 * p["l"] - 1
        t["relb"] = _rand(g, buckets, p["h"])
        t["bucket"] = torch.randint(0, buckets, (n,), generator=g, dtype=torch.int32)

    def _t5_act(self, g, p, t, d):
        x = _rand(g, p["rows"], (2 if p["gated"] else 1) * p["f"]) * 3.0
        x[0, :8] = torch.tensor([-30.0, -14.0, -12.5, -4.0, 4.0, 12.5, 14.0, 30.0])
        t["g"] = x

    def _t5_mask_rows(self, g, p, t, d):
        t["y"] = _rand(g, p["rows"], p["d"])
        t["mask"] = torch.tensor([1, 1, 0, 1, 0, 0, 1, 1, 1, 0, 1], dtype=torch.int32)

    def _roberta_embed_ln(self, g, p, t, d):
        b, l, vocab, pad_id = 2, 130, 50, 1
        ids = torch.randint(2, vocab, (b, l), generator=g, dtype=torch.int32)
        ids[0, 100:] = pad_id            # tail padding behind token 64
        ids[1, 3] = ids[1, 40:47] = ids[1, 63] = ids[1, 64] = ids[1, 120] = ids[1, 127:129] = pad_id            # pads in the middle, across 64 and 128
        max_pos = pad_id + l + 3
        dd = 192 if p["table"] == "onehot" else 100
        if p["table"] == "onehot":
            # zero word / type rows and posw[q] = e_q: the largest channel of the output row IS the position index
            word, type0, posw = torch.zeros(vocab, dd), torch.zeros(dd), torch.eye(max_pos, dd)
            gamma, beta = torch.ones(dd), torch.zeros(dd)
        else:
            word, type0, posw = _rand(g, vocab, dd), _rand(g, dd) * 0.1, _rand(g, max_pos, dd) * 0.5
            gamma, beta = 1.0 + 0.3 * _rand(g, dd), 0.3 * _rand(g, dd)
        t.update(ids=ids, word=word, posw=posw, type0=type0, gamma=gamma, beta=beta)
        d.update(b=b, l=l, d=dd, vocab=vocab, pad_id=pad_id, max_pos=max_pos, eps=1e-5)

    def _roberta_gelu(self, g, p, t, d):
        x = _rand(g, p["n"]) * 3.0
        x[:8] = torch.tensor([-30.0, -14.0, -12.5, -4.0, 4.0, 12.5, 14.0, 30.0])
        t["h"] = x

    def _small_linear(self, g, p, t, d):
        r, n, k = p["r"], p["n"], p["k"]
        ldx, ldy, ldadd = k + 4, n + 3, n + 5
        t["x"], t["w"] = _rand(g, r, ldx), _rand(g, n, k) * (2.0 / math.sqrt(k))
        t["bias"] = _rand(g, n) if p["bias"] else None
        t["add"] = _rand(g, r, ldadd) if p["add"] else None
        d.update(r=r, n=n, k=k, ldx=ldx, ldy=ldy, ldadd=ldadd)

    def _adaln_finish(self, g, p, t, d):
        ssg = _rand(g, p["b"], p["layers"], 6, p["d"]) * 2.0
        ssg[0, 0, :, :6] = torch.tensor([-30.0, -13.0, -12.5, 12.5, 13.0, 30.0])
        t["ssg"] = ssg

    def _fourier(self, g, p, t, d):
        b, half = 3, 128
        t["w"] = _rand(g, half) * 0.3            # |2 pi t w| stays under ~10 rad (the condition on the inputs)
        t["t"] = torch.tensor([0.03, 0.5, 0.97]) if p["t"] == "per_batch" else None
        d.update(b=b, half=half, t_const=0.0 if p["t"] == "per_batch" else 0.71)

    def _fold_in(self, g, p, t, d):
        t["w"], t["wc"] = _rand(g, p["d"], p["c"]), _rand(g, p["c"], p["c"]) * 0.3

    def _fold_out(self, g, p, t, d):
        t["w"], t["wc"] = _rand(g, p["c"], p["d"]), _rand(g, p["c"], p["c"]) * 0.3

    def _input_proj(self, g, p, t, d, extra=False):
        bf, xb, c, tt, dd = 4, 2, p["c"], p["t"], p["d"]
        cc = 3 if extra else 0
        pp = p.get("p", 0)
        s = pp + p["pre"] + tt
        t["x"] = _rand(g, xb, c, tt)
        t["x"][1] *= 8.0            # b % xB: the second latent is 8 x the first
        t["weff_t"] = _rand(g, c + cc, dd) * 0.3
        if extra:
            tc = tt if p["tc"] == "t" else p["tc"]
            t["concat"] = _rand(g, bf, cc, tc) * (1.0 + torch.arange(bf, dtype=torch.float32)[:, None, None])
            t["prep"] = _rand(g, bf, pp, dd) if pp else None
            d.update(cc=cc, tc=tc, p=pp)
        d.update(bf=bf, xb=xb, c=c, t=tt, s=s, d=dd, xscale=0.37)

    def _input_proj_extra(self, g, p, t, d):
        self._input_proj(g, p, t, d, extra=True)

    def _output_proj(self, g, p, t, d):
        bf, tt, c, dd = 3, 13, p["c"], p["d"]
        s = tt + p["pre"]
        X = _rand(g, bf, s, dd)
        X[1] *= 8.0
        t["X"], t["weff_t"] = X, _rand(g, dd, c) * 0.2
        d.update(bf=bf, c=c, t=tt, s=s, d=dd)

    def _pos_table(self, g, p, t, d):
        rows, dd = 64, 128
        t["src"] = torch.tensor([dd ** -0.5 * 1.3]) if p["mode"] == 1 else _rand(g, rows + 9, dd)            # the absolute table is longer than the rows used
        d.update(rows=rows, d=dd, alloc_rows=rows + 6)

    def _add_pos(self, g, p, t, d):
        bf, s, dd = 3, 50, 128
        t["X"] = _rand(g, bf, s, dd)
        t["table"] = _rand(g, 64, dd) * 0.3
        d.update(bf=bf, s=s, d=dd)

    def _cfg_denoise(self, g, p, t, d):
        b, c, tt = 2, 8, 150
        t["mo"], t["x"] = _rand(g, 2 * b, c, tt), _rand(g, b, c, tt) * 3.0
        d.update(b=b, c=c, t=tt, cfg_scale=6.5, c_out=-0.8, c_skip=0.6, phi=p["phi"])


# ----------------------------------------------------------------------------------------------------------------- the restatements
def _c(x, dt):
    return None if x is None else x.to(dt)


def silu(v):
    return v * torch.sigmoid(v)


def gelu_new(x):
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x.pow(3))))


def gelu_erf(x):
    return x * 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0)))


def layer_norm(x, gamma, beta, eps):
    mean = x.mean(dim=-1, keepdim=True)
    var = (x - mean).pow(2).mean(dim=-1, keepdim=True)
    y = (x - mean) / torch.sqrt(var + eps) * gamma
    return y if beta is None else y + beta


def attention(q, k, v, scale, bias=None, keep=None):
    """softmax(scale q k^T + bias) v over the keys of ``keep`` [..., sk] (bool; None: all).  A query without a single kept key averages all of
    them uniformly -- what adding finfo(float32).min to every score does, in the kernel and in transformers.  q [..., sq, d], k / v [..., sk, d]."""
    s = torch.einsum("...id,...jd->...ij", q, k) * scale
    if bias is not None:
        s = s + bias
    if keep is not None:
        keep = keep.expand(s.shape[:-2] + (1, s.shape[-1])) if keep.dim() == s.dim() else keep
        none = ~keep.any(dim=-1, keepdim=True)
        s = torch.where(keep | none, s, torch.full((), -math.inf, dtype=s.dtype))
        s = torch.where(none, torch.zeros((), dtype=s.dtype), s)
    return torch.einsum("...ij,...jd->...id", torch.softmax(s, dim=-1), v)


def rope_partial(x, cos, sin):
    """Partial rotary on the first 32 of 64 channels, pairs (c, c + 16): x [b, h, s, 64], cos / sin [s, 16]."""
    x1, x2, rest = x[..., :16], x[..., 16:32], x[..., 32:]
    return torch.cat((x1 * cos - x2 * sin, x2 * cos + x1 * sin, rest), dim=-1)


def roberta_positions(ids, pad_id):
    keep = (ids != pad_id).long()
    return torch.cumsum(keep, dim=1) * keep + pad_id


def nearest_src(tc, t):
    """The source frame of every output frame of F.interpolate(mode="nearest") from tc to t frames, as PyTorch computes it on the CPU."""
    return F.interpolate(torch.arange(tc, dtype=torch.float32).view(1, 1, tc), size=t, mode="nearest").view(t).long()


def sinusoidal_angles(rows, d):
    """The angle as the reference model forms it: fp32 positions times the fp32 theta ** -(j / (d / 2))."""
    half = d // 2
    inv_freq = 10000.0 ** -(torch.arange(half, dtype=torch.float32) / half)
    return torch.arange(rows, dtype=torch.float32)[:, None] * inv_freq[None, :]


def _contract(out, key, val, mag, n):
    out[key], out[key + ":mag"], out[key + ":n"] = val, mag, n


def reference(case, dt=torch.float64):
    k, t, d, p = case.kind, case.t, case.dim, case.p
    f64 = torch.float64
    out = {}
    if k == "gemm_f32":
        a, w, bias, c_in, gate = (_c(t[x], dt) for x in ("a", "w", "bias", "c_in", "gate"))
        v = a @ w.T
        mag = t["a"].to(f64).abs() @ t["w"].to(f64).abs().T
        if bias is not None:
            v, mag = v + bias, mag + t["bias"].to(f64).abs()
        if c_in is not None:
            mag = mag + t["c_in"].to(f64).abs()
        if gate is not None:
            rows = torch.arange(d["m"]) // GATE_ROWS
            v = v * gate[rows, :d["n"]]
            mag = mag * t["gate"].to(f64).abs()[rows, :d["n"]]
        if c_in is not None:
            v = c_in + v
        _contract(out, "c", v, mag, d["k"])
    elif k == "layernorm_f32":
        y = layer_norm(_c(t["x"], dt), _c(t["gamma"], dt), _c(t["beta"], dt), d["eps"])
        if t["scale"] is not None:
            rows = torch.arange(d["m"]) // d["rps"]
            y = y * _c(t["scale"], dt)[rows, :d["d"]] + _c(t["shift"], dt)[rows, :d["d"]]
        out["y"] = y
    elif k == "split_heads_f32":
        b, s, h, parts = d["b"], d["s"], d["h"], p["parts"]
        src = _c(t["src"], dt).view(b, s, parts, h, 64).permute(2, 0, 3, 1, 4)            # [parts, b, h, s, 64]
        for i in range(parts):
            x = src[i]
            if (p["rope"] >> i) & 1:
                x = rope_partial(x, _c(t["cos"], dt), _c(t["sin"], dt))
            if (p["norm"] >> i) & 1:
                x = x / x.norm(dim=-1, keepdim=True).clamp_min(1e-12)
            out[f"d{i}"] = x.contiguous()
    elif k == "swiglu_f32":
        hg = _c(t["hg"], dt)
        out["h"] = hg[:, :p["inner"]] * silu(hg[:, p["inner"]:])
    elif k == "attention_f32":
        q, kk, v = (_c(t[x], dt) for x in ("q", "k", "v"))
        rep = p["h"] // p["kvh"]
        o = attention(q, kk.repeat_interleave(rep, dim=1), v.repeat_interleave(rep, dim=1), 0.125)            # [b, h, sq, 64]
        out["out"] = o.permute(0, 2, 1, 3).contiguous()            # [b, sq, h, 64] = [b * sq, h * 64]
    elif k == "enc_attention":
        b, l, h, dkv = d["b"], d["l"], d["h"], d["dkv"]
        q, kk, v = (x.view(b, l, h, dkv).permute(0, 2, 1, 3) for x in _c(t["qkv"], dt).chunk(3, dim=-1))
        bias = None
        if t["pb"] is not None:
            idx = torch.arange(l)[None, :] - torch.arange(l)[:, None] + l - 1            # [query, key] -> key - query + l - 1
            bias = _c(t["pb"], dt)[:, idx]            # [h, l, l]
        o = attention(q, kk, v, d["scale"], bias, (t["mask"] != 0).view(b, 1, 1, l))
        out["out"] = o.permute(0, 2, 1, 3).contiguous()            # [b, l, h, dkv]
    elif k == "t5_embed":
        out["out"] = t["emb"][t["ids"].long().clamp(0, d["vocab"] - 1)]
    elif k == "t5_rmsnorm":
        x = _c(t["x"], dt)
        out["y"] = x / torch.sqrt(x.pow(2).mean(dim=-1, keepdim=True) + d["eps"]) * _c(t["w"], dt)
    elif k == "t5_position_bias":
        out["pb"] = t["relb"][t["bucket"].long()].T.contiguous()
    elif k == "t5_act":
        g = _c(t["g"], dt)
        out["h"] = gelu_new(g[:, :p["f"]]) * g[:, p["f"]:] if p["gated"] else torch.relu(g)
    elif k == "t5_mask_rows":
        out["y"] = t["y"] * (t["mask"] != 0).float()[:, None]
    elif k == "roberta_embed_ln":
        pos = roberta_positions(t["ids"].long(), d["pad_id"])
        e = (_c(t["word"], dt)[t["ids"].long()] + _c(t["type0"], dt)) + _c(t["posw"], dt)[pos]
        out["y"] = layer_norm(e, _c(t["gamma"], dt), _c(t["beta"], dt), d["eps"])
        if p["table"] == "onehot":            # the largest channel of an output row is its position index
            out["pos"] = pos
    elif k == "roberta_gelu":
        out["h"] = gelu_erf(_c(t["h"], dt))
    elif k == "small_linear":
        x, w, bias, add = _c(t["x"], dt)[:, :d["k"]], _c(t["w"], dt), _c(t["bias"], dt), _c(t["add"], dt)
        v = x @ w.T
        mag = t["x"].to(f64)[:, :d["k"]].abs() @ t["w"].to(f64).abs().T
        if bias is not None:
            v, mag = v + bias, mag + t["bias"].to(f64).abs()
        if p["act"] == 1:
            v = silu(v)
        if add is not None:
            v, mag = v + add[:, :d["n"]], mag + t["add"].to(f64)[:, :d["n"]].abs()
        if p["act"] == 2:
            v = silu(v)
        _contract(out, "y", v, mag, d["k"])
    elif k == "adaln_finish":
        v = _c(t["ssg"], dt).clone()
        v[:, :, (0, 3)] = 1.0 + v[:, :, (0, 3)]
        v[:, :, (2, 5)] = torch.sigmoid(1.0 - v[:, :, (2, 5)])
        out["ssg"] = v
    elif k == "fourier":
        tv = torch.full((d["b"],), d["t_const"]) if t["t"] is None else t["t"]
        f = (2.0 * math.pi * _c(tv, dt))[:, None] * _c(t["w"], dt)[None, :]
        out["out"] = torch.cat((f.cos(), f.sin()), dim=-1)
    elif k == "fold_in":
        w, wc = _c(t["w"], dt), _c(t["wc"], dt)
        eye = torch.eye(p["c"], dtype=dt)
        _contract(out, "weff_t", (w @ (eye + wc)).T.contiguous(),
                  (t["w"].to(f64).abs() @ (torch.eye(p["c"], dtype=f64) + t["wc"].to(f64).abs())).T.contiguous(), p["c"] + 1)
    elif k == "fold_out":
        w, wc = _c(t["w"], dt), _c(t["wc"], dt)
        eye = torch.eye(p["c"], dtype=dt)
        _contract(out, "weff_t", ((eye + wc) @ w).T.contiguous(),
                  ((torch.eye(p["c"], dtype=f64) + t["wc"].to(f64).abs()) @ t["w"].to(f64).abs()).T.contiguous(), p["c"] + 1)
    elif k in ("input_proj", "input_proj_extra"):
        bf, xb, c, tt = d["bf"], d["xb"], d["c"], d["t"]
        item = torch.arange(bf) % xb
        x, w = _c(t["x"], dt)[item], _c(t["weff_t"], dt)
        v = torch.einsum("cn,bct->btn", w[:c], x) * d["xscale"]
        mag = torch.einsum("cn,bct->btn", t["weff_t"].to(f64)[:c].abs(), t["x"].to(f64)[item].abs()) * d["xscale"]
        n = c
        if k == "input_proj_extra":
            src = nearest_src(d["tc"], tt)
            v = v + torch.einsum("cn,bct->btn", w[c:], _c(t["concat"], dt)[:, :, src])
            mag = mag + torch.einsum("cn,bct->btn", t["weff_t"].to(f64)[c:].abs(), t["concat"].to(f64)[:, :, src].abs())
            n = c + d["cc"]
            if t["prep"] is not None:
                out["prep"] = t["prep"]
        _contract(out, "X", v, mag, n + 1)            # (+ 1: the multiplication by xscale)
    elif k == "output_proj":
        X = _c(t["X"], dt)[:, d["s"] - d["t"]:]
        _contract(out, "out", torch.einsum("nc,btn->bct", _c(t["weff_t"], dt), X),
                  torch.einsum("nc,btn->bct", t["weff_t"].to(f64).abs(), t["X"].to(f64)[:, d["s"] - d["t"]:].abs()), d["d"])
    elif k == "pos_table":
        if p["mode"] == 1:
            ang = sinusoidal_angles(d["rows"], d["d"]).to(dt)            # fp32 angles, sine and cosine in dt
            out["table"] = torch.cat((ang.sin(), ang.cos()), dim=-1) * _c(t["src"], dt)[0]
        else:
            out["table"] = _c(t["src"], dt)[:d["rows"]] * d["d"] ** -0.5
    elif k == "add_pos":
        out["X"] = _c(t["X"], dt) + _c(t["table"], dt)[:d["s"]][None]
    elif k == "cfg_denoise":
        b = d["b"]
        mo, x = _c(t["mo"], dt), _c(t["x"], dt)
        cond, unc = mo[:b], mo[b:]
        gsum = cond
        if p["use_cfg"]:
            gsum = unc + (cond - unc) * d["cfg_scale"]
            if d["phi"] != 0.0:
                gsum = gsum * (d["phi"] * (cond.std(dim=1, keepdim=True) / gsum.std(dim=1, keepdim=True)) + (1.0 - d["phi"]))
        out["den"] = gsum * d["c_out"] + x * d["c_skip"]
    else:
        raise ValueError(k)
    return out


# ----------------------------------------------------------------------------------------------------------------------- the gates
def _as_rows(case, key, x):
    """The 2-D view whose rows are what one wave / workgroup / token of the kernel owns (for the row and 32 x 32 block gates)."""
    if case.kind == "output_proj":
        return x.permute(0, 2, 1).reshape(-1, x.shape[1])            # [bf * t, c]: one row per token
    return x.reshape(-1, x.shape[-1])            # (input_proj: [bf * t, d])


def bound_share(got, want, mag, n):
    """|got - want| / ((n + 4) 2^-24 mag) per element, in float64 (mag == 0: the element has to be exact)."""
    err = (got.detach().to("cpu", torch.float64) - want.to(torch.float64)).abs()
    bound = (n + 4) * UNIT * mag
    return torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full((), math.inf, dtype=torch.float64), torch.zeros((), dtype=torch.float64)))


def code_distance(got16, want64, dtype):
    """Distance in codes of a 16-bit format between ``got16`` and the correctly rounded image of the float64 ``want64``."""
    def order(x):
        bits = x.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF
        return torch.where(bits >= 0x8000, -(bits - 0x8000), bits)            # sign-magnitude order; +0 and -0 coincide
    limit = 65504.0 if dtype == torch.float16 else 3.3895e38
    return (order(got16.cpu()) - order(want64.clamp(-limit, limit).to(dtype))).abs()


def _note(case, key, what, figure, where=""):
    LOG.append((case.name, key, what, float(figure), where))


def check(case, got, want=None, headroom=1.0):
    """Every output of ``got`` ({name: CPU tensor}) against ``want`` (reference(case) unless given) under the gates of the module docstring."""
    want = reference(case) if want is None else want
    k, p = case.kind, case.p
    tol = TOL * headroom
    for key, w in want.items():
        if ":" in key:
            continue
        g = got[key]
        name = f"{case.name} {key}"
        assert tuple(g.shape) == tuple(w.shape), f"{name}: shape {tuple(g.shape)}, expected {tuple(w.shape)}"
        if key in ("prep", "pos") or k in ("t5_embed", "t5_position_bias", "t5_mask_rows"):
            assert torch.equal(g.cpu(), w), f"{name}: not bit-identical to the expected values ({int((g.cpu() != w).sum())} elements differ)"
            continue
        if k == "small_linear" and p["out16"]:
            dist = code_distance(g, w, g.dtype)
            share = (dist != 0).double().mean().item()
            _note(case, key, "max code distance", dist.max().item())
            _note(case, key, "share of elements off the correctly rounded code", share)
            assert int(dist.max()) <= 1, f"{name}: {int((dist > 1).sum())} elements are more than one {g.dtype} code from the correctly rounded result"
            assert share <= 0.01, f"{name}: {share:.2%} of the elements differ from the correctly rounded result (limit 1 %)"
            continue
        assert torch.isfinite(g.float()).all(), f"{name}: non-finite values"
        if k in CONTRACTIONS:
            mag, n = want[key + ":mag"], want[key + ":n"]
            share = bound_share(g, w, mag, n)
            worst = int(share.reshape(-1).argmax())
            _note(case, key, "largest share of the a-priori bound", share.reshape(-1)[worst].item(),
                  str(tuple(int(i) for i in torch.unravel_index(torch.tensor(worst), share.shape))))
            bad = ~(share <= 1.0)
            assert not bool(bad.any()), (f"{name}: {int(bad.sum())} elements exceed the a-priori bound (n + 4) 2^-24 (|A| |W|^T + |bias| + |C_in|) |gate|"
                                         f", the worst {share.max().item():.3g} x at {tuple(int(i) for i in bad.nonzero()[0])}")
            gr, wr = _as_rows(case, key, g), _as_rows(case, key, w)
            r = assert_close_sliced(name + " per row", gr, wr, tol, (0,))
            _note(case, key, "worst row", r[0], str(r[1]))
            r = assert_close_sliced(name + " per 32x32 block", blocks32(gr), blocks32(wr), tol, (0, 2))
            _note(case, key, "worst 32x32 block", r[0], str(r[1]))
            continue
        if k in ("attention_f32", "enc_attention", "split_heads_f32"):
            # per (query, head) -- (head, row) for the head split -- inside every batch item: the floor of slice_errors is the item's own
            for b in range(w.shape[0]):
                r = assert_close_sliced(f"{name} item {b} per (row, head)", g[b], w[b], tol, (0, 1))
                _note(case, key, f"worst slice of item {b}", r[0], str(r[1]))
        elif k in ("layernorm_f32", "t5_rmsnorm", "roberta_embed_ln"):
            r = assert_close_sliced(name + " per row", g.reshape(-1, g.shape[-1]), w.reshape(-1, w.shape[-1]), tol, (0,))
            _note(case, key, "worst row", r[0], str(r[1]))
        else:            # elementwise: |err| <= tol max(|want|, rms(want))
            r = assert_close_sliced(name + " per element", g, w, tol, tuple(range(w.dim())))
            _note(case, key, "worst element", r[0], str(r[1]))
