"""Every kernel of the fp32 path (csrc/f32_ref.hip), of the two text encoders (enc_attention.h, t5_encoder.hip, roberta_encoder.hip) and of the
DiT glue (dit_glue.hip) alone, through its unit entry of include/sat_hip.h -- the launcher the plans call -- against float64 PyTorch on the
same fp32 inputs.

Gates (tests/fp32_units.py): contractions element by element under the a-priori bound (n + 4) 2^-24 (|A| |W|^T + |bias| + |C_in|) |gate| and per
row and 32 x 32 block at 1e-5; every other fp32 output at 1e-5 per (batch, query, head), per row or per element; the 16-bit outputs of
small_linear within one code of the correctly rounded result; copies, gathers and position indices bit for bit.  Every output sits in a NaN
guard band; what the contract leaves alone (the ldc - N and ldy - N columns, the rows below S - T and the global token's row of input_proj,
table rows beyond the ones asked for) must still hold the sentinel.  That the references are right, that the fp32 evaluation on the CPU passes
every 1e-5 gate four times over, and that the gates reject the faults these kernels can have: tests/test_fp32_kernels_host.py.  Figures:
profiles/fp32_kernels_verification.txt (written with SAT_PARITY_LOG set)."""
import pytest
import torch

import fp32_units as fu
from util import PARITY_LOG, guarded

pytestmark = pytest.mark.gpu


def _cases(kind):
    return pytest.mark.parametrize("p", fu.CASES[kind], ids=fu.case_id)


class _Call:
    """Uploads, guarded outputs and the call of one entry; ``done()`` synchronises and checks every guard band."""

    def __init__(self, dev):
        from stable_audio_tools import _hip
        self.hip, self.lib, self.dev, self.keep, self.outs = _hip, _hip.lib(), dev, [], []

    def up(self, t):
        """Device pointer of a copy of ``t`` (None -> NULL)."""
        if t is None:
            return None
        self.keep.append(t.contiguous().to(self.dev))
        return self.keep[-1].data_ptr()

    def out(self, shape, name, dtype=torch.float32, init=None, pitch=None):
        g = guarded(shape, dtype, self.dev, init=None if init is None else init.to(self.dev), name=name, pitch=pitch)
        self.outs.append(g)
        return g

    def call(self, entry, *args):
        self.hip.check(getattr(self.lib, entry)(*args, self.hip.stream()))
        torch.cuda.synchronize()
        for g in self.outs:
            g.check()


def _untouched(g, region, what):
    """``region`` (a view of the guarded interior) still holds the sentinel bit for bit."""
    if region.numel():
        bits = region.contiguous().view(g.bits)
        n = int((bits != g.sentinel).sum())
        assert n == 0, f"{g.name}: {n} elements of {what} were written; the contract leaves them alone"


def _finish(case, got):
    fu.LOG.clear()
    try:
        fu.check(case, {k: v.cpu() for k, v in got.items()})
    finally:
        if PARITY_LOG:
            with open(PARITY_LOG, "a") as f:
                for name, key, what, figure, where in fu.LOG:
                    f.write(f"fp32_units\t{name}\t{key}\t{what}\t{figure:.3e}\t{where}\n")


# ------------------------------------------------------------------------------------------------------------------- f32_ref.hip
@_cases("gemm_f32")
def test_gemm_f32(dev, p):
    """128 x 128 tiles with row and column tails, one to 32 K-steps, bias, accumulation into a prefilled C, and a gate whose row changes
    inside a tile; C has a row pitch of N + 8 and the 8 columns behind N stay untouched."""
    c = fu.Case("gemm_f32", p)
    t, d = c.t, c.dim
    k = _Call(dev)
    g = k.out((d["m"], d["ldc"]), "gemm_f32 C")
    if t["c_in"] is not None:
        g.t[:, :d["n"]].copy_(t["c_in"])
    k.call("sat_gemm_f32", k.up(t["a"]), k.up(t["w"]), k.up(t["bias"]), g.t.data_ptr(), d["m"], d["n"], d["k"], d["ldc"], p["acc"], k.up(t["gate"]),
           fu.GATE_ROWS, 3 * d["n"])
    g.assert_written(g.t[:, :d["n"]])
    _untouched(g, g.t[:, d["n"]:], "the columns behind N")
    _finish(c, {"c": g.t[:, :d["n"]]})


@_cases("layernorm_f32")
def test_layernorm_f32(dev, p):
    """One wave per row: d of one, one and a half and four passes of 64 lanes, a last workgroup of one row, beta NULL, both eps, the adaLN
    modulation of three rows per sequence from a table with a longer pitch, and rows whose mean is 30 times their spread."""
    c = fu.Case("layernorm_f32", p)
    t, d = c.t, c.dim
    k = _Call(dev)
    g = k.out((d["m"], d["d"]), "layernorm_f32 y")
    k.call("sat_layernorm_f32", k.up(t["x"]), k.up(t["gamma"]), k.up(t["beta"]), g.t.data_ptr(), d["m"], d["d"], k.up(t["scale"]), k.up(t["shift"]),
           d["rps"], d["ld"], d["eps"])
    g.assert_written()
    _finish(c, {"y": g.t})


@_cases("split_heads_f32")
def test_split_heads_f32(dev, p):
    """q | k | v (or fewer parts) of two sequences of 37 rows and 3 heads into [b, h, s, 64], with and without the partial rotary and the per-head
    L2 norm; sequence 1 is 8 x sequence 0, so a row or a table entry taken from the neighbour shows in its own slice."""
    c = fu.Case("split_heads_f32", p)
    t, d = c.t, c.dim
    k = _Call(dev)
    outs = [k.out((d["b"], d["h"], d["s"], 64), f"split_heads_f32 d{i}") for i in range(p["parts"])]
    ptrs = [g.t.data_ptr() for g in outs] + [None] * (3 - p["parts"])
    k.call("sat_split_heads_f32", k.up(t["src"]), *ptrs, d["b"], d["s"], p["parts"], d["h"], p["rope"], k.up(t["cos"]), k.up(t["sin"]), p["norm"])
    for g in outs:
        g.assert_written()
    _finish(c, {f"d{i}": g.t for i, g in enumerate(outs)})


@_cases("swiglu_f32")
def test_swiglu_f32(dev, p):
    c = fu.Case("swiglu_f32", p)
    k = _Call(dev)
    g = k.out((p["m"], p["inner"]), "swiglu_f32 h")
    k.call("sat_swiglu_f32", k.up(c.t["hg"]), g.t.data_ptr(), p["m"], p["inner"])
    g.assert_written()
    _finish(c, {"h": g.t})


@_cases("attention_f32")
def test_attention_f32(dev, p):
    """One query per lane, keys in chunks of 8: 77 and 7 keys (a last chunk of 5 and one of 7), one key, 70 / 129 queries (a partial last
    workgroup), grouped K / V heads, scores that are all about 60 with the row maximum in the last chunk, and scores that are all about -30."""
    c = fu.Case("attention_f32", p)
    t = c.t
    k = _Call(dev)
    g = k.out((p["b"] * p["sq"], p["h"] * 64), "attention_f32 out")
    k.call("sat_attention_f32", k.up(t["q"]), k.up(t["k"]), k.up(t["v"]), g.t.data_ptr(), p["b"], p["h"], p["kvh"], p["sq"], p["sk"])
    g.assert_written()
    _finish(c, {"out": g.t.view(p["b"], p["sq"], p["h"], 64)})


# ------------------------------------------------------------------------------------------------------------- the text encoders
@_cases("enc_attention")
def test_enc_attention(dev, p):
    """One wave per (query, head, sequence), keys at a lane stride of 64: 1 to 512 keys (one key, a partial first round, exactly one, one and a
    key, two and a bit, all eight), head dims 64 and 40, the T5 form (position bias, no scale) and the RoBERTa form; per sequence a full
    mask, tail padding, a single real key or none at all.  K and V rows of masked keys hold 1e4; an all-padding sequence keeps distinct
    rows, so only the uniform average over all of them passes."""
    c = fu.Case("enc_attention", p)
    t, d = c.t, c.dim
    k = _Call(dev)
    g = k.out((d["b"] * d["l"], d["h"] * d["dkv"]), "enc_attention out")
    k.call("sat_enc_attention", k.up(t["qkv"]), k.up(t["pb"]), k.up(t["mask"]), g.t.data_ptr(), d["b"], d["l"], d["h"], d["dkv"], d["scale"])
    g.assert_written()
    _finish(c, {"out": g.t.view(d["b"], d["l"], d["h"], d["dkv"])})


@_cases("t5_embed")
def test_t5_embed(dev, p):
    c = fu.Case("t5_embed", p)
    k = _Call(dev)
    g = k.out((p["rows"], p["d"]), "t5_embed out")
    k.call("sat_t5_embed", k.up(c.t["ids"]), k.up(c.t["emb"]), g.t.data_ptr(), p["rows"], p["d"], c.dim["vocab"])
    g.assert_written()
    _finish(c, {"out": g.t})


@_cases("t5_rmsnorm")
def test_t5_rmsnorm(dev, p):
    c = fu.Case("t5_rmsnorm", p)
    k = _Call(dev)
    g = k.out((p["m"], p["d"]), "t5_rmsnorm y")
    k.call("sat_t5_rmsnorm", k.up(c.t["x"]), k.up(c.t["w"]), g.t.data_ptr(), p["m"], p["d"], c.dim["eps"])
    g.assert_written()
    _finish(c, {"y": g.t})


@_cases("t5_position_bias")
def test_t5_position_bias(dev, p):
    c = fu.Case("t5_position_bias", p)
    n = 2 * p["l"] - 1
    k = _Call(dev)
    g = k.out((p["h"], n), "t5_position_bias pb")
    k.call("sat_t5_position_bias", k.up(c.t["relb"]), k.up(c.t["bucket"]), g.t.data_ptr(), p["h"], n)
    g.assert_written()
    _finish(c, {"pb": g.t})


@_cases("t5_act")
def test_t5_act(dev, p):
    """relu in place, and gelu_new(wi_0) * wi_1 from the stacked [rows, 2 f] GEMM output; sizes that are no multiple of 256, arguments to +-30."""
    c = fu.Case("t5_act", p)
    k = _Call(dev)
    if p["gated"]:
        g = k.out((p["rows"], p["f"]), "t5_act h")
        src = k.up(c.t["g"])
    else:
        g = k.out((p["rows"], p["f"]), "t5_act h (in place)", init=c.t["g"])
        src = g.t.data_ptr()
    k.call("sat_t5_act", src, g.t.data_ptr(), p["rows"], p["f"], p["gated"])
    g.assert_written()
    _finish(c, {"h": g.t})


@_cases("t5_mask_rows")
def test_t5_mask_rows(dev, p):
    c = fu.Case("t5_mask_rows", p)
    k = _Call(dev)
    g = k.out((p["rows"], p["d"]), "t5_mask_rows y", init=c.t["y"])
    k.call("sat_t5_mask_rows", g.t.data_ptr(), k.up(c.t["mask"]), p["rows"], p["d"])
    _finish(c, {"y": g.t})


@_cases("roberta_embed_ln")
def test_roberta_embed_ln(dev, p):
    """Gather, position scan and LayerNorm of two sequences of 130 ids with pads in the middle, at the tail and across tokens 64 and 128.  With
    unit vectors as the position table the largest channel of a row is its position, which has to equal cumsum(ids != pad) * (ids != pad) + pad."""
    c = fu.Case("roberta_embed_ln", p)
    t, d = c.t, c.dim
    k = _Call(dev)
    g = k.out((d["b"] * d["l"], d["d"]), "roberta_embed_ln y")
    k.call("sat_roberta_embed_ln", k.up(t["ids"]), k.up(t["word"]), k.up(t["posw"]), k.up(t["type0"]), k.up(t["gamma"]), k.up(t["beta"]),
           g.t.data_ptr(), d["b"], d["l"], d["d"], d["vocab"], d["pad_id"], d["max_pos"], d["eps"])
    g.assert_written()
    got = {"y": g.t.view(d["b"], d["l"], d["d"])}
    if p["table"] == "onehot":
        got["pos"] = got["y"].argmax(dim=-1)
    _finish(c, got)


@_cases("roberta_gelu")
def test_roberta_gelu(dev, p):
    c = fu.Case("roberta_gelu", p)
    k = _Call(dev)
    g = k.out((p["n"],), "roberta_gelu h", init=c.t["h"])
    k.call("sat_roberta_gelu", g.t.data_ptr(), p["n"])
    g.assert_written()
    _finish(c, {"h": g.t})


# ---------------------------------------------------------------------------------------------------------------- dit_glue.hip
@_cases("small_linear")
def test_small_linear(dev, p):
    """One wave per output column, 8 rows per wave: one row, a second row block of one row, three of them; K of one float4, of 260 (a second
    pass of one float4) and 512; row pitches above K and N for x, y and the addend; SiLU before or after the addend; fp32, bf16 and fp16 results."""
    c = fu.Case("small_linear", p)
    t, d = c.t, c.dim
    dtype = (torch.float32, torch.bfloat16, torch.float16)[p["out16"]]
    k = _Call(dev)
    g = k.out((d["r"], d["ldy"]), "small_linear y", dtype=dtype)
    k.call("sat_small_linear", k.up(t["x"]), d["ldx"], k.up(t["w"]), k.up(t["bias"]), k.up(t["add"]), d["ldadd"], g.t.data_ptr(), d["ldy"], d["r"],
           d["n"], d["k"], p["act"], p["out16"])
    g.assert_written(g.t[:, :d["n"]])
    _untouched(g, g.t[:, d["n"]:], "the columns behind N")
    _finish(c, {"y": g.t[:, :d["n"]]})


@_cases("adaln_finish")
def test_adaln_finish(dev, p):
    c = fu.Case("adaln_finish", p)
    k = _Call(dev)
    g = k.out(tuple(c.t["ssg"].shape), "adaln_finish ssg", init=c.t["ssg"], pitch=6 * p["d"])
    k.call("sat_adaln_finish", g.t.data_ptr(), c.t["ssg"].numel(), p["d"])
    g.assert_written()
    _finish(c, {"ssg": g.t})


@_cases("fourier")
def test_fourier_features(dev, p):
    c = fu.Case("fourier", p)
    d = c.dim
    k = _Call(dev)
    g = k.out((d["b"], 2 * d["half"]), "fourier out")
    k.call("sat_fourier_features", k.up(c.t["t"]), d["t_const"], k.up(c.t["w"]), g.t.data_ptr(), d["b"], d["half"])
    g.assert_written()
    _finish(c, {"out": g.t})


@_cases("fold_in")
def test_fold_in(dev, p):
    c = fu.Case("fold_in", p)
    k = _Call(dev)
    g = k.out((p["c"], p["d"]), "fold_in weff_t")
    k.call("sat_fold_in", k.up(c.t["w"]), k.up(c.t["wc"]), g.t.data_ptr(), p["d"], p["c"])
    g.assert_written()
    _finish(c, {"weff_t": g.t})


@_cases("fold_out")
def test_fold_out(dev, p):
    c = fu.Case("fold_out", p)
    k = _Call(dev)
    g = k.out((p["d"], p["c"]), "fold_out weff_t")
    k.call("sat_fold_out", k.up(c.t["w"]), k.up(c.t["wc"]), g.t.data_ptr(), p["d"], p["c"])
    g.assert_written()
    _finish(c, {"weff_t": g.t})


@_cases("input_proj")
def test_input_proj(dev, p):
    """8 time steps x 256 channels per workgroup: one step, exactly eight, 13 and 77 (a partial last chunk), one and two channel blocks, two
    latents under four sequences (b % xB; the second latent is 8 x the first), with and without a prepended row -- which is not written."""
    c = fu.Case("input_proj", p)
    t, d = c.t, c.dim
    k = _Call(dev)
    g = k.out((d["bf"], d["s"], d["d"]), "input_proj X")
    k.call("sat_input_proj", k.up(t["x"]), k.up(t["weff_t"]), g.t.data_ptr(), d["bf"], d["xb"], d["c"], d["t"], d["s"], d["d"], d["xscale"])
    pre = d["s"] - d["t"]
    g.assert_written(g.t[:, pre:])
    _untouched(g, g.t[:, :pre], "the rows below S - T")
    _finish(c, {"X": g.t[:, pre:]})


@_cases("input_proj_extra")
def test_input_proj_extra(dev, p):
    """The same with three concat channels at the latent's own length (the contiguous route), from 5 frames (upsampled) and from 200
    (downsampled) at the source frames of F.interpolate(mode="nearest"), and 0, 3 or 9 prepend rows copied by workgroups of 8 rows (none, one
    partial, one full and one partial).  The global token's row X[b, P] belongs to another kernel."""
    c = fu.Case("input_proj_extra", p)
    t, d = c.t, c.dim
    k = _Call(dev)
    g = k.out((d["bf"], d["s"], d["d"]), "input_proj_extra X")
    k.call("sat_input_proj_extra", k.up(t["x"]), k.up(t["weff_t"]), g.t.data_ptr(), d["bf"], d["xb"], d["c"], d["t"], d["s"], d["d"], d["xscale"],
           k.up(t["concat"]), d["cc"], d["tc"], k.up(t["prep"]), d["p"])
    pre = d["s"] - d["t"]
    g.assert_written(g.t[:, pre:])
    _untouched(g, g.t[:, d["p"]:pre], "the global token's row")
    got = {"X": g.t[:, pre:]}
    if d["p"]:
        got["prep"] = g.t[:, :d["p"]]
    _finish(c, got)


@_cases("output_proj")
def test_output_proj(dev, p):
    """8 tokens per workgroup over 3 x 13 tokens: workgroups straddle two sequences (the second is 8 x the others) and the last one holds 7;
    4, 8 and 64 output channels (lanes beyond C idle), embed dims of one, two and twelve steps per wave, 0, 1 and 4 prepended rows skipped."""
    c = fu.Case("output_proj", p)
    t, d = c.t, c.dim
    k = _Call(dev)
    g = k.out((d["bf"], d["c"], d["t"]), "output_proj out", pitch=d["c"] * d["t"])
    k.call("sat_output_proj", k.up(t["X"]), k.up(t["weff_t"]), g.t.data_ptr(), d["bf"], d["c"], d["t"], d["s"], d["d"])
    g.assert_written()
    _finish(c, {"out": g.t})


@_cases("pos_table")
def test_pos_table(dev, p):
    """The sinusoidal and the absolute table, 64 rows of 128 channels into a buffer of 70 rows (the rest is not written), the absolute one
    from an embedding of 73 rows."""
    c = fu.Case("pos_table", p)
    d = c.dim
    k = _Call(dev)
    g = k.out((d["alloc_rows"], d["d"]), "pos_table table")
    k.call("sat_pos_table", p["mode"], k.up(c.t["src"]), g.t.data_ptr(), d["rows"], d["d"])
    g.assert_written(g.t[:d["rows"]])
    _untouched(g, g.t[d["rows"]:], "the rows beyond the table")
    _finish(c, {"table": g.t[:d["rows"]]})


@_cases("add_pos")
def test_add_pos(dev, p):
    """X[b, s] += table[s] for 3 sequences of 50 rows from a table of 64: one addition, so also bit-identical to the fp32 sum."""
    c = fu.Case("add_pos", p)
    d = c.dim
    k = _Call(dev)
    g = k.out((d["bf"], d["s"], d["d"]), "add_pos X", init=c.t["X"])
    k.call("sat_add_pos", g.t.data_ptr(), k.up(c.t["table"]), d["bf"], d["s"], d["d"])
    g.assert_written()
    _finish(c, {"X": g.t})
    assert torch.equal(g.t.cpu(), c.t["X"] + c.t["table"][:d["s"]][None])


@_cases("cfg_denoise")
def test_cfg_denoise(dev, p):
    """Both kernels behind glue_cfg_denoise (the elementwise one, and the per-column one of the std rescale) with c_out = -0.8 and c_skip = 0.6,
    which sat_cfg_combine does not expose; 2 x 8 x 150 elements (a partial last workgroup in both)."""
    c = fu.Case("cfg_denoise", p)
    d = c.dim
    k = _Call(dev)
    g = k.out((d["b"], d["c"], d["t"]), "cfg_denoise den", pitch=d["c"] * d["t"])
    k.call("sat_cfg_denoise", k.up(c.t["mo"]), k.up(c.t["x"]), g.t.data_ptr(), d["b"], d["c"], d["t"], p["use_cfg"], d["cfg_scale"], d["phi"], d["c_out"],
           d["c_skip"])
    g.assert_written()
    _finish(c, {"den": g.t})
