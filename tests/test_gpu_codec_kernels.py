"""Every kernel of the Oobleck codec alone (csrc/oobleck.hip through ``sat_oobleck_unit``: one layer, the plan's own weight packing, launch
set-up and kernels) against a float64 restatement on the same rounded operands, in the bf16, fp16 and fp32 builds.

Gates: the whole tensor, then per (batch item, time row) and per 32 x 32 accumulator block per batch item, per (batch item, channel,
64-sample window) for the channel-first fp32 results; 16-bit builds at the kernel-test tolerance of q / k (4e-3 bf16, 1e-3 fp16), the fp32
build at the 1e-5 of test_gpu_codec_fp32.py.  Every output sits in a NaN guard band, pad channels are compared bitwise with zero.  Shapes,
inputs and references: tests/codec_units.py; that the gates reject a single wrong row, a missing tap at a tile seam, a leaked row, a
shifted first span and a non-zero pad channel, and that the references are right: tests/test_codec_kernels_host.py."""
import ctypes

import pytest
import torch

import codec_units as cu
from util import guarded

pytestmark = pytest.mark.gpu


def _params(kind):
    return pytest.mark.parametrize("p", cu.CASES[kind], ids=cu.case_id)


_fmts = pytest.mark.parametrize("fmt", cu.ALL_FORMATS, ids=repr)


def _run(dev, case, fmt, two_launch=False):
    """One ``sat_oobleck_unit`` call; returns the guarded outputs {"raw", "snk", "cf"} that the layer writes (and "res" where the residual
    is not overwritten, to check that it was left alone)."""
    from stable_audio_tools import _hip
    c, k = case, case.kind
    d = _hip.SatOobleckUnitDesc()
    d.kind = cu.KINDS.index(k)
    d.gemm_dtype = cu.GEMM_CODE[fmt.name]
    d.activation = _hip.OOBLECK_ACT_SNAKE if c.act == "snake" else _hip.OOBLECK_ACT_ELU
    d.b, d.t_len, d.c_in, d.c_out = cu.BATCH, c.rows, c.c_in, c.c_out
    d.stride, d.dilation, d.two_launch, d.final_tanh = c.stride, c.dilation, int(two_launch), c.tanh
    keep = []

    def up(t):
        if t is None:
            return None
        keep.append(t.contiguous().to(dev))
        return keep[-1].data_ptr()

    snake = c.act == "snake"
    if k != "cf_to_cl":
        d.weight_g, d.weight_v, d.bias = up(c.weight_g), up(c.weight_v), up(c.bias)
        if snake and k not in ("final_dec", "final_enc"):
            d.alpha, d.beta = up(c.alpha), up(c.beta)
    if k == "residual":
        d.weight_g2, d.weight_v2, d.bias2 = up(c.weight_g2), up(c.weight_v2), up(c.bias2)
        if snake:
            d.alpha2, d.beta2 = up(c.alpha2), up(c.beta2)
    if k in ("first_conv", "cf_to_cl"):
        d.in_cf = up(c.x)
    else:
        d.in_ = up(c.x_cl(fmt))
    out = {}
    cp = cu.pad64(c.c_out)
    if k in ("final_dec", "final_enc"):
        out["cf"] = guarded((cu.BATCH, c.c_out, c.rows), torch.float32, dev, name=f"{k} out_cf")
        d.out_cf = out["cf"].t.data_ptr()
    else:
        shape = (cu.BATCH, c.out_rows, cp)
        if c.res is not None:
            res = c.res_cl(fmt)
            if c.want_raw:          # in place, as run_ru has it: res == out_raw
                out["raw"] = guarded(shape, fmt.dtype, dev, init=res.to(dev), name=f"{k} out_raw")
                d.res = out["raw"].t.data_ptr()
            else:
                out["res"] = guarded(shape, fmt.dtype, dev, init=res.to(dev), name=f"{k} res")
                d.res = out["res"].t.data_ptr()
        elif c.want_raw:
            out["raw"] = guarded(shape, fmt.dtype, dev, name=f"{k} out_raw")
        if "raw" in out:
            d.out_raw = out["raw"].t.data_ptr()
        if k != "cf_to_cl":
            out["snk"] = guarded(shape, fmt.dtype, dev, name=f"{k} out_snk")
            d.out_snk = out["snk"].t.data_ptr()
    _hip.check(_hip.lib().sat_oobleck_unit(ctypes.byref(d), ctypes.sizeof(d), _hip.stream()))
    torch.cuda.synchronize()
    for g in out.values():
        g.check().assert_written()
    return out


def _check(name, case, fmt, out, want):
    """Guards were checked by _run; pad channels, then the gates of codec_units for every output the layer wrote."""
    for key in ("raw", "snk"):
        if key in out:
            got = out[key].t.cpu()
            cu.assert_pad_zero(f"{name} out_{key}", got, case.c_out)
            cu.gate_cl(f"{name} {fmt} out_{key}", got, want[key], fmt)
    if "cf" in out:
        cu.gate_cf(f"{name} {fmt} out_cf", out["cf"].t.cpu(), want["cf"], fmt)
    if "res" in out:
        assert torch.equal(out["res"].t.cpu(), case.res_cl(fmt)), f"{name}: the residual was written although no raw output was asked for"


def _one(dev, kind, p, fmt):
    case = cu.Case(kind, p)
    out = _run(dev, case, fmt)
    _check(f"{kind} {cu.case_id(p)}", case, fmt, out, cu.reference(case, fmt))
    return case, out


@_fmts
@_params("conv7")
def test_dilated_conv7(dev, p, fmt):
    """The implicit-GEMM convolution at seven dilated taps: both tile shapes, a tile seam with the halo across it, windows clipped at both
    ends; the linear out_raw carries the leaked-row check (item 1 is 8 x item 0), out_snk the activation."""
    _one(dev, "conv7", p, fmt)


@_fmts
@_params("conv1_res")
def test_conv1_with_inplace_residual(dev, p, fmt):
    """One and two K-tiles (the 2-stage rings), the residual read and written in place, and the activated output alone."""
    _one(dev, "conv1_res", p, fmt)


@_fmts
@_params("residual")
def test_residual_unit_fused_and_two_launch(dev, p, fmt):
    """A whole ResidualUnit: the fused kernel where a plan fuses (16-bit builds; the fp32 build takes two launches either way) and the forced
    two-launch route on the same inputs, each against float64 with the tensor between the convolutions rounded as the kernels round it."""
    case = cu.Case("residual", p)
    want = cu.reference(case, fmt)
    name = f"residual {cu.case_id(p)}"
    fused = _run(dev, case, fmt)
    _check(f"{name} {'two launches (fp32)' if fmt.name == 'f32' else 'fused'}", case, fmt, fused, want)
    two = _run(dev, case, fmt, two_launch=True)
    _check(f"{name} two launches", case, fmt, two, want)
    same = all(torch.equal(fused[k].t, two[k].t) for k in ("raw", "snk"))
    print(f"\n[{name} {fmt}] fused and two-launch routes bit-equal: {same}")


@_fmts
@_params("convt")
def test_transposed_conv(dev, p, fmt):
    """The polyphase transposed convolution against F.conv_transpose1d: phase-major packing, the lone row M = L + 1 in the second tile, the first
    pad * Cout elements and the last span clipped by out_shift / out_limit."""
    _one(dev, "convt", p, fmt)


@_fmts
@_params("nearest")
def test_nearest_upsample_conv(dev, p, fmt):
    """The three-tap polyphase form against F.interpolate(nearest) + a "same" convolution, odd stride included."""
    _one(dev, "nearest", p, fmt)


@_fmts
@_params("strided")
def test_strided_encoder_conv(dev, p, fmt):
    """Conv1d(k = 2 s, stride s, padding ceil(s / 2)), 64 -> 128 channels, 130 output rows, odd stride included."""
    _one(dev, "strided", p, fmt)


@_fmts
@_params("first_conv")
def test_encoder_first_conv(dev, p, fmt):
    """The VALU first convolution in both builds, 1 and 2 input channels; the 16 pad channels of the 48-wide case are exact zeros."""
    _one(dev, "first_conv", p, fmt)


@_fmts
@_params("final_dec")
def test_decoder_final_conv(dev, p, fmt):
    """k = 7 without bias into channel-first fp32, one and two channels of a 64-column tile, tanh on and off."""
    _one(dev, "final_dec", p, fmt)


@_fmts
def test_encoder_final_conv(dev, fmt):
    """k = 3 with bias, 256 -> 40 channels of a 64-column tile, channel-first fp32."""
    _one(dev, "final_enc", {}, fmt)


@_fmts
def test_cf_to_cl(dev, fmt):
    """fp32 [b, 20, 70] -> channels-last [b, 70, 64]: a rounding and a transpose, so the result is exact."""
    case, out = _one(dev, "cf_to_cl", {}, fmt)
    want = fmt.round(cu.to_cl(case.x, 64)).to(fmt.dtype)
    assert torch.equal(out["raw"].t.cpu(), want)


@_fmts
def test_unit_refuses_what_a_plan_refuses(dev, fmt):
    """Odd strides on the transposed route and stride 1 in the encoder: the reference yields L * s - 1 and L + 1 samples there, the plan's
    bookkeeping L * s and L (tests/test_codec_kernels_host.py has the arithmetic), so neither the entry point nor a plan runs them."""
    from stable_audio_tools import _hip
    lib = _hip.lib()
    for kind, p in (("convt", dict(rows=130, stride=3)), ("convt", dict(rows=130, stride=1)), ("strided", dict(stride=1))):
        case = cu.Case(kind, p)
        with pytest.raises(_hip.SatError, match="stride"):
            _run(dev, case, fmt)
    d = _hip.SatOobleckUnitDesc()
    assert lib.sat_oobleck_unit(ctypes.byref(d), ctypes.sizeof(d) - 8, None) == -1 and b"desc_bytes" in lib.sat_last_error()
