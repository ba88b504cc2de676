"""The references and gates of tests/test_gpu_codec_kernels.py, proven on the CPU (pattern: test_parity_gates_host.py): the float64
restatements of codec_units agree with the oracle's layer functions and with PyTorch's own modules and output lengths; a correctly rounded
result passes every gate; each fault a codec kernel can have -- a wrong row at a tile seam, a tap missing on the rows around it, a row of the
next batch item read into the last window, a non-zero pad channel, a shifted first span of a transposed convolution -- is rejected, most of
them while the whole-tensor figure stays inside the gates of the encoder / decoder tests; the Snake arguments stay where __sinf is accurate;
and the strides the reference maps to other lengths than the plan are refused.  With SAT_PARITY_LOG set the measured figures are appended to
that file (profiles/codec_kernels_verification.txt)."""
import ctypes
import math
import os

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import codec_units as cu
from util import FORMATS, PARITY_LOG, rel_l2, slice_errors

BF16, F16 = FORMATS


def _fails(fn, *args, **kw):
    try:
        fn(*args, **kw)
    except AssertionError as e:
        return str(e)
    return None


def _log(line):
    if PARITY_LOG:
        with open(PARITY_LOG, "a") as f:
            f.write(f"{os.environ.get('PYTEST_CURRENT_TEST', '').split(' ')[0]}\t{line}\n")


def _close(a, b, tol=1e-6):
    e = ((a.double() - b.double()).norm() / b.double().norm()).item()
    assert e <= tol, f"rel-L2 {e:.3e} > {tol:.0e}"


# ------------------------------------------------------------------------------------------------------------ the references
def test_fold_and_snake_are_the_oracles():
    from oracle import oobleck as oob
    for kind, p in (("conv7", cu.CASES["conv7"][0]), ("convt", cu.CASES["convt"][0]), ("strided", cu.CASES["strided"][1])):
        c = cu.Case(kind, p)
        _close(cu.fold(c.weight_g, c.weight_v), oob.fold_weight_norm(c.weight_g.view(-1, 1, 1), c.weight_v))
        v = torch.randn((2, c.c_out, 9), generator=torch.Generator().manual_seed(3)) * 4.0
        _close(cu.snake(v.double(), c.alpha, c.beta), oob.snake_beta(v, c.alpha, c.beta))


@pytest.mark.parametrize("p", [p for p in cu.CASES["residual"] if p["act"] == "snake"], ids=cu.case_id)
def test_residual_reference_is_the_oracles_residual_unit(p):
    """oracle.residual_unit takes the raw x and applies the first Snake itself; the kernel's inputs are act(x) and x."""
    from oracle import oobleck as oob
    c = cu.Case("residual", p)
    v = c.res
    a0, b0 = c.alpha2 * 0.5, c.beta2 * 0.5
    c.x = oob.snake_beta(v, a0, b0)
    sd = {"layers.0.alpha": a0, "layers.0.beta": b0, "layers.1.weight_g": c.weight_g.view(-1, 1, 1), "layers.1.weight_v": c.weight_v,
          "layers.1.bias": c.bias, "layers.2.alpha": c.alpha, "layers.2.beta": c.beta, "layers.3.weight_g": c.weight_g2.view(-1, 1, 1),
          "layers.3.weight_v": c.weight_v2, "layers.3.bias": c.bias2}
    want = oob.residual_unit(sd, "", v, c.dilation)
    got = cu.reference(c, cu.F32)
    assert got["raw"].shape == (cu.BATCH, c.rows, c.c_out)
    _close(got["raw"], cu.to_cl(want, c.c_out))
    _close(got["snk"], cu.to_cl(oob.snake_beta(want, c.alpha2, c.beta2), c.c_out))


@pytest.mark.parametrize("p", cu.CASES["convt"], ids=cu.case_id)
def test_transposed_reference_is_the_oracles_upsample(p):
    from oracle import oobleck as oob
    c = cu.Case("convt", p)
    v = c.x.clone()
    a0, b0 = torch.zeros(c.c_in), torch.zeros(c.c_in)
    c.x = oob.snake_beta(v, a0, b0)
    sd = {"layers.0.alpha": a0, "layers.0.beta": b0, "layers.1.weight_g": c.weight_g.view(-1, 1, 1), "layers.1.weight_v": c.weight_v,
          "layers.1.bias": c.bias}
    want = oob.decoder_upsample(sd, "", v, c.stride)
    assert want.shape[-1] == c.out_rows == c.rows * c.stride
    _close(cu.reference(c, cu.F32)["raw"], cu.to_cl(want, c.c_out))


@pytest.mark.parametrize("p", cu.CASES["strided"], ids=cu.case_id)
def test_strided_reference_is_the_oracles_downsample(p):
    from oracle import oobleck as oob
    c = cu.Case("strided", p)
    v = c.x.clone()
    a0, b0 = torch.zeros(c.c_in), torch.zeros(c.c_in)
    c.x = oob.snake_beta(v, a0, b0)
    sd = {"layers.3.alpha": a0, "layers.3.beta": b0, "layers.4.weight_g": c.weight_g.view(-1, 1, 1), "layers.4.weight_v": c.weight_v,
          "layers.4.bias": c.bias}
    want = oob.encoder_downsample(sd, "", v, c.stride)
    assert want.shape[-1] == c.out_rows == 130
    _close(cu.reference(c, cu.F32)["raw"], cu.to_cl(want, c.c_out))


@pytest.mark.parametrize("p", cu.CASES["nearest"], ids=cu.case_id)
def test_nearest_reference_is_pytorchs_upsample_and_same_conv(p):
    """Against the reference's own modules, nn.Upsample + nn.Conv1d(padding="same"), and against the product's polyphase taps: the
    restatement is independent of both."""
    from stable_audio_tools.models.autoencoders import nearest_upsample_taps
    c = cu.Case("nearest", p)
    conv = nn.Conv1d(c.c_in, c.c_out, 2 * c.stride, bias=False, padding="same")
    w = cu.fold(c.weight_g, c.weight_v).float()
    with torch.no_grad():
        conv.weight.copy_(w)
        want = conv(nn.Upsample(scale_factor=c.stride, mode="nearest")(c.x))
    assert want.shape[-1] == c.out_rows == c.rows * c.stride
    got = cu.reference(c, cu.F32)["raw"]
    _close(got, cu.to_cl(want, c.c_out))
    taps = nearest_upsample_taps(w, c.stride).double()          # [stride, 3, Cout, Cin]
    xp = F.pad(c.x.double(), (1, 1))
    poly = torch.stack([sum(torch.einsum("oc,bct->bot", taps[ph, r], xp[:, :, r:r + c.rows]) for r in range(3)) for ph in range(c.stride)], dim=-1)
    _close(got, cu.to_cl(poly.reshape(cu.BATCH, c.c_out, -1), c.c_out))


def test_conv_lengths_and_the_odd_stride_question():
    """The lengths PyTorch produces for the reference's layers (autoencoders.py: EncoderBlock, DecoderBlock), against what the plan assumes: a
    decoder block L -> L * s, an encoder block L -> L / s.  ConvTranspose1d(k = 2s, stride s, padding ceil(s / 2)) gives L * s - 1 at odd s,
    the encoder's stride-1 convolution gives L + 1: those two are refused (below); the nearest form and the strided form at s >= 2 fit."""
    x = torch.zeros(1, 4, 24)
    for s in range(1, 17):
        up = nn.ConvTranspose1d(4, 4, 2 * s, stride=s, padding=math.ceil(s / 2))(x).shape[-1]
        assert up == 24 * s + s - 2 * math.ceil(s / 2) and (up == 24 * s) == (s % 2 == 0) and (s % 2 == 0 or up == 24 * s - 1)
        near = nn.Conv1d(4, 4, 2 * s, padding="same")(nn.Upsample(scale_factor=s, mode="nearest")(x)).shape[-1]
        assert near == 24 * s
        xin = torch.zeros(1, 4, 24 * s)
        down = nn.Conv1d(4, 4, 2 * s, stride=s, padding=math.ceil(s / 2))(xin).shape[-1]
        assert down == (25 if s == 1 else 24)
    for kind in ("convt", "nearest", "strided"):
        for p in cu.CASES[kind]:
            c = cu.Case(kind, p)
            assert cu.reference(c, cu.F32)["raw"].shape == (cu.BATCH, c.out_rows, cu.pad64(c.c_out))


def test_odd_transposed_strides_and_encoder_stride_one_are_refused():
    """sat_oobleck_plan_create_ex answers SAT_E_UNSUPPORTED, the modules NotImplementedError; nearest-upsample decoders keep odd strides."""
    from stable_audio_tools import _hip
    from stable_audio_tools.models.autoencoders import OobleckDecoder, OobleckEncoder
    lib = _hip.lib()

    def create(is_decoder, strides, nearest=0):
        cfg = _hip.SatOobleckCfg()
        cfg.is_decoder, cfg.io_channels, cfg.channels, cfg.latent_dim, cfg.n_blocks = is_decoder, 2, 64, 64, len(strides)
        for i, s in enumerate(strides):
            cfg.c_mults[i], cfg.strides[i] = 1, s
        opt = _hip.SatOobleckOptions(_hip.OOBLECK_ACT_SNAKE, 0, nearest)
        plan = ctypes.c_void_p()
        rc = lib.sat_oobleck_plan_create_ex(ctypes.byref(cfg), ctypes.byref(opt), ctypes.sizeof(opt), ctypes.byref(plan))
        if rc == 0:
            lib.sat_oobleck_plan_destroy(plan)
        return rc

    assert create(1, [2, 4, 8, 16]) == 0 and create(0, [2, 3, 5, 16]) == 0 and create(1, [1, 3, 5], nearest=1) == 0
    for is_decoder, strides in ((1, [2, 3]), (1, [1, 2]), (1, [4, 15]), (0, [2, 1]), (0, [1])):
        assert create(is_decoder, strides) == -2, (is_decoder, strides)
        assert b"stride" in lib.sat_last_error()
    OobleckDecoder(channels=64, c_mults=[1, 1], strides=[3, 5], use_nearest_upsample=True, final_tanh=False)
    OobleckEncoder(channels=64, c_mults=[1, 1], strides=[3, 5])
    with pytest.raises(NotImplementedError, match="odd stride"):
        OobleckDecoder(channels=64, c_mults=[1, 1], strides=[2, 3], final_tanh=False)
    with pytest.raises(NotImplementedError, match="stride-1"):
        OobleckEncoder(channels=64, c_mults=[1, 1], strides=[2, 1])


# ------------------------------------------------------------------------------------------------------------------ the gates
@pytest.mark.parametrize("fmt", FORMATS, ids=repr)
@pytest.mark.parametrize("kind", [k for k in cu.KINDS if k != "cf_to_cl"])
def test_correctly_rounded_results_pass_every_gate(kind, fmt):
    """The gates ask nothing of a correct kernel that the output format does not give: the float64 reference rounded once to the format
    passes whole, per row, per block and per window, on every shape of the GPU tests."""
    for p in cu.CASES[kind]:
        c = cu.Case(kind, p)
        want = cu.reference(c, fmt)
        for key, w in want.items():
            if key == "cf":
                cu.gate_cf(f"{kind} {cu.case_id(p)}", w.float(), w, fmt)
            else:
                got = fmt.round(w.float())
                cu.assert_pad_zero(kind, got.to(fmt.dtype), c.c_out)
                cu.gate_cl(f"{kind} {cu.case_id(p)} {key}", got, w, fmt)


@pytest.mark.parametrize("fmt", FORMATS, ids=repr)
def test_intermediate_rounding_of_the_residual_unit(fmt):
    """What rounding the tensor between a unit's convolutions moves: the float64 reference with and without it, whole and worst row.  The
    GPU reference rounds as the kernels do, so this is not part of its gate; it is the figure a wider gate would be built on (twice it),
    and it is below the gate in every case, so none was needed."""
    worst = 0.0
    for p in cu.CASES["residual"]:
        c = cu.Case("residual", p)
        a, b = cu.reference(c, fmt)["raw"], cu.reference(c, fmt, round_mid=False)["raw"]
        whole = rel_l2(a, b)
        rows = max(slice_errors(a[i], b[i], (0,)).max().item() for i in range(cu.BATCH))
        _log(f"residual {cu.case_id(p)} {fmt}: float64 reference with vs without the intermediate rounding: whole={whole:.3e}\tworst row={rows:.3e}\tgate={cu.tol(fmt):.3e}")
        worst = max(worst, rows)
    assert worst < cu.tol(fmt), f"intermediate rounding alone moves a row by {worst:.3e}"


@pytest.mark.parametrize("fmt", FORMATS, ids=repr)
def test_snake_arguments_stay_where_fast_sine_is_accurate(fmt):
    """The 16-bit builds evaluate Snake with __sinf (v_sin_f32 on x / 2 pi).  Error model: |x| * 2^-22 from the scaled argument plus 2^-20
    absolute, valid inside the instruction's range of 256 revolutions.  The perturbation it can cause in v + ib sin^2(a v) is 2 ib times that;
    per output row it stays below a tenth of the gate in every case, so the gates measure the kernels, not the sine."""
    peak, share = 0.0, 0.0
    for kind in cu.KINDS:
        for p in cu.CASES[kind]:
            c = cu.Case(kind, p)
            for av, ib, y in cu.snake_arguments(c, fmt):
                peak = max(peak, av.max().item())
                err = 2.0 * ib.view(1, -1, 1) * (av * 2.0 ** -22 + 2.0 ** -20)
                row = err.pow(2).sum(dim=1).sqrt() / y.pow(2).sum(dim=1).sqrt().clamp_min(y.pow(2).sum(dim=1).mean(dim=1, keepdim=True).sqrt())
                share = max(share, row.max().item() / cu.tol(fmt))
    _log(f"snake arguments {fmt}: max |e^alpha v| = {peak:.1f} rad; worst row share of the gate taken by the fast-sine error model = {share:.3f}")
    assert peak < 256 * 2 * math.pi / 4, peak
    assert share < 0.1, share


# The planted faults whose whole-tensor rel-L2 stays inside the gate of the encoder / decoder tests, on these 300- and 520-row outputs
# (a property of the references and the faults alone, measured here on the CPU; a fault's share of the whole falls with the square root of
# the row count, so on the encoder / decoder tests' outputs of thousands of rows all of them do)
PASS_THE_CODEC_GATE = {"bf16": {"one wrong row at row 128", "one tap missing on rows 125-130",
                                "first pad * Cout elements of a transposed output shifted by one row"},
                       "f16": set()}


def _gate_msg(c, fmt, got, want, parts=("whole", "rows", "blocks")):
    return _fails(cu.gate_cl, c.kind, got, want, fmt, parts)


@pytest.mark.parametrize("fmt", FORMATS, ids=repr)
def test_planted_faults_are_rejected(fmt):
    """Each fault goes into a correctly rounded copy of a reference output of the GPU tests' own shapes.  The gates of codec_units reject it;
    the whole-tensor rel-L2 the encoder / decoder tests gate (1.5e-2 bf16, 3.75e-3 fp16) is computed beside it, and asserted to let the
    fault through where it does."""
    codec_gate = cu.CODEC_GATE[fmt.name]
    seen = {}

    def planted(name, c, got, want):
        msg, blk = _gate_msg(c, fmt, got, want, ("rows",)), _gate_msg(c, fmt, got, want, ("blocks",))
        whole = rel_l2(got, want)
        _log(f"planted fault, {fmt}: {name}: per-row gate {'REJECTS' if msg else 'passes'}, per-block gate {'REJECTS' if blk else 'passes'}; "
             f"whole-tensor rel-L2 {whole:.3e} {'<=' if whole <= codec_gate else '>'} codec gate {codec_gate:.2e}")
        assert msg and "slice (" in msg, f"{name}: the per-row gate lets it through"
        assert (whole <= codec_gate) == (name in PASS_THE_CODEC_GATE[fmt.name]), f"{name}: whole-tensor {whole:.3e} against {codec_gate:.2e}"
        seen[name] = msg

    # the k = 7 convolution at dilation 1, 64 channels, 300 rows: a seam at row 256 of the 256 x 64 tile, at 128 of the other tiles
    c = cu.Case("conv7", dict(c=64, rows=300, dilation=1, act="snake"))
    want = cu.reference(c, fmt)["raw"]
    good = fmt.round(want.float())
    assert _gate_msg(c, fmt, good, want) is None
    got = good.clone()
    got[0, 128] = got[0, 127]
    planted("one wrong row at row 128", c, got, want)
    assert "item 0 per row" in seen["one wrong row at row 128"] and "slice (128,)" in seen["one wrong row at row 128"]
    got = good.clone()
    got[0, 125:131] = fmt.round(cu.reference(c, fmt, drop_tap=0)["raw"].float())[0, 125:131]
    planted("one tap missing on rows 125-130", c, got, want)
    # item 0's last row reads one row too far: row 0 of item 1 follows it in memory (tap 4 of row 299 reads row 300)
    w = fmt.round(cu.fold(c.weight_g, c.weight_v).float()).double()
    x = fmt.round(c.x).double()
    got = good.clone()
    got[0, 299, :c.c_out] = fmt.round((want[0, 299, :c.c_out] + w[:, :, 4] @ x[1, :, 0]).float())
    planted("one row of item 1 added into item 0's last window", c, got, want)
    # the transposed convolution at stride 4: pad = 2, the first 2 * Cout elements are rows 0 and 1
    c = cu.Case("convt", dict(rows=130, stride=4))
    want = cu.reference(c, fmt)["raw"]
    good = fmt.round(want.float())
    got = good.clone()
    got[0, 0:2] = good[0, 1:3]
    planted("first pad * Cout elements of a transposed output shifted by one row", c, got, want)
    # a pad channel of the 48-wide first convolution: the bitwise check, whatever the size of the value
    c = cu.Case("first_conv", dict(c_out=48, c_in=2, act="elu"))
    want = cu.reference(c, fmt)["snk"]
    got = fmt.round(want.float()).to(fmt.dtype)
    cu.assert_pad_zero("first_conv", got, 48)
    got[0, 7, 50] = 2.0 ** -20
    msg = _fails(cu.assert_pad_zero, "first_conv", got, 48)
    _log(f"planted fault, {fmt}: non-zero pad channel (2^-20 at [0, 7, 50]): bitwise pad check {'REJECTS' if msg else 'passes'}; "
         f"sliced gate {'rejects' if _gate_msg(c, fmt, got.float(), want) else 'passes'}; whole-tensor rel-L2 {rel_l2(got, want):.3e}")
    assert msg and "pad-channel" in msg
