"""The single-layer cases of the codec kernel tests (test_gpu_codec_kernels.py on the device, test_codec_kernels_host.py on the CPU): shapes,
seeded inputs, the float64 restatement of every layer kind on the operands the kernels see, and the gates.

A case is one layer of the Oobleck codec as ``sat_oobleck_unit`` runs it: weights in the reference layout in fp32 (weight_g / weight_v / bias,
alpha / beta of the activation behind the layer), activations channels-last [b, t, Cp] in the build's operand type, Cp the channel count rounded
up to a multiple of 64 with zero pad channels.  The references are plain PyTorch in float64 -- F.conv1d, F.conv_transpose1d, F.interpolate +
a "same" convolution -- and never the polyphase forms the kernels use, which are what is under test.

Batch 2 throughout.  Item 1 is ITEM1_SCALE times item 0, so one row of item 1 read into item 0's last window (or item 0's first output rows
written from item 1's) dominates it, and every sliced gate is taken per batch item: the floor of util.slice_errors (the rms row norm) is then
the item's own and item 0 keeps its sharpness.  One input row of item 0 is all zeros."""
import math
import zlib

import torch
import torch.nn.functional as F

from util import FORMATS, assert_close_sliced, blocks32

ITEM1_SCALE = 8.0
BATCH = 2


class _F32:
    """The fp32 build beside util.FORMATS: no operand rounding, the gate of test_gpu_codec_fp32.py."""
    name, f16, dtype, gemm_dtype = "f32", False, torch.float32, "fp32"

    @staticmethod
    def round(x):
        return x.to(torch.float32)

    def __repr__(self):
        return self.name


F32 = _F32()
ALL_FORMATS = list(FORMATS) + [F32]
GEMM_CODE = {"bf16": 0, "f16": 3, "f32": 2}          # include/sat_hip.h: SAT_GEMM_BF16 / SAT_GEMM_FP16 / SAT_GEMM_FP32X
CODEC_GATE = {"bf16": 1.5e-2, "f16": 3.75e-3}        # the whole-tensor gates of the encoder / decoder tests (test_gpu_models.py)

KINDS = ("conv7", "conv1_res", "residual", "convt", "nearest", "strided", "first_conv", "final_dec", "final_enc", "cf_to_cl")


def tol(fmt):
    """16-bit builds: the kernel-test gate of q / k and of the depthwise kernel.  fp32: TOL of test_gpu_codec_fp32.py."""
    if fmt.name == "f32":
        from test_gpu_codec_fp32 import TOL
        return TOL
    return fmt.tol(4e-3)


def out_round(fmt):
    return None if fmt.name == "f32" else fmt.round


def pad64(c):
    return (c + 63) // 64 * 64


def _product(**axes):
    out = [{}]
    for k, vals in axes.items():
        out = [dict(o, **{k: v}) for o in out for v in vals]
    return out


# The smallest shapes that reach every seam (rows = t_len, the GEMM's M unless noted):
#   conv7     C = 64: the 256 x 64 tile, 3 stages; C = 128: 128 x 128, 3 stages.  300 rows: a seam and a 44-row tail, at dilation 9 a 27-row halo
#             across the seam; 5 rows: every window is clipped at both ends
#   conv1_res C = 64: one K-tile; C = 128: two, the 2-stage rings.  With and without the raw output
#   residual  the fused kernel's two instantiations per activation; the same inputs go through the two-launch route
#   convt     L = 130: M = 131, the extra row reads tap m - 1 only and sits alone in the second tile; L = 1; the first pad * Cout elements and
#             the last span are clipped by out_shift / out_limit
#   first_conv  Cout = 64 Snake: the fast build; Cout = 48 or ELU: the general one; 130 samples: a 64-sample tile seam and a 2-sample tail
CASES = {
    "conv7": _product(c=[64, 128], rows=[300, 5], dilation=[1, 3, 9], act=["snake", "elu"]),
    "conv1_res": _product(c=[64, 128], rows=[300], raw=[True, False], act=["snake", "elu"]),
    "residual": _product(c=[128, 256], rows=[300, 5], dilation=[1, 3, 9], act=["snake", "elu"]),
    "convt": _product(rows=[130, 1], stride=[2, 4, 8]),
    "nearest": _product(rows=[130, 1], stride=[2, 3, 4]),
    "strided": _product(stride=[2, 3, 4, 8]),
    "first_conv": _product(c_out=[64, 48], c_in=[1, 2], act=["snake", "elu"]),
    "final_dec": _product(c_out=[1, 2], tanh=[0, 1]),
    "final_enc": [{}],
    "cf_to_cl": [{}],
}


def case_id(p):
    return "-".join(f"{k}{v}" for k, v in p.items()) or "only"


def _rand(gen, *shape):
    return torch.randn(shape, generator=gen)


class Case:
    """kind + parameters -> shapes and seeded fp32 tensors (the same for every format; activations are rounded to the format on use)."""

    def __init__(self, kind, p):
        self.kind, self.p = kind, dict(p)
        gen = torch.Generator().manual_seed(zlib.crc32(repr((kind, sorted(p.items()))).encode()))
        self.act = p.get("act", "snake")
        self.stride = p.get("stride", 0)
        self.dilation = p.get("dilation", 0)
        self.tanh = p.get("tanh", 0)
        self.want_raw = p.get("raw", True)
        k = kind
        if k in ("conv7", "conv1_res", "residual"):
            self.c_in = self.c_out = p["c"]
            self.rows = p["rows"]
            self.taps = 1 if k == "conv1_res" else 7
        elif k in ("convt", "nearest"):
            self.c_in, self.c_out, self.rows, self.taps = 128, 64, p["rows"], 2 * self.stride
        elif k == "strided":
            self.c_in, self.c_out, self.rows, self.taps = 64, 128, 130 * self.stride, 2 * self.stride
        elif k == "first_conv":
            self.c_in, self.c_out, self.rows, self.taps = p["c_in"], p["c_out"], 130, 7
        elif k == "final_dec":
            self.c_in, self.c_out, self.rows, self.taps = 64, p["c_out"], 300, 7
        elif k == "final_enc":
            self.c_in, self.c_out, self.rows, self.taps = 256, 40, 300, 3
        else:
            self.c_in, self.c_out, self.rows, self.taps = 20, 20, 70, 0
        self.out_rows = {"convt": self.rows * self.stride, "nearest": self.rows * self.stride,
                         "strided": self.rows // self.stride if self.stride else 0}.get(k, self.rows)
        ci, co, L = self.c_in, self.c_out, self.rows
        # input [b, c, t] fp32: item 1 scaled, one zero row in item 0
        x = _rand(gen, BATCH, ci, L) * (0.4 if k == "first_conv" else 1.0)
        x[1] *= ITEM1_SCALE
        if L > 4:
            x[0, :, 3] = 0.0
        self.x = x
        self.res = None
        if k in ("conv1_res", "residual"):
            self.res = _rand(gen, BATCH, co, L)
            self.res[1] *= ITEM1_SCALE
        if k == "cf_to_cl":
            return
        wshape = (ci, co, self.taps) if k == "convt" else (co, ci, self.taps)
        self.weight_v = _rand(gen, *wshape) * 0.1
        self.weight_g = 0.6 + 0.8 * torch.rand((wshape[0],), generator=gen)
        self.bias = None if k in ("nearest", "final_dec") else _rand(gen, co) * 0.3
        self.alpha, self.beta = _rand(gen, co) * 0.3, _rand(gen, co) * 0.3
        if k == "residual":
            self.weight_v2 = _rand(gen, co, co, 1) * 0.1
            self.weight_g2 = 0.6 + 0.8 * torch.rand((co,), generator=gen)
            self.bias2 = _rand(gen, co) * 0.3
            self.alpha2, self.beta2 = _rand(gen, co) * 0.3, _rand(gen, co) * 0.3

    # ---- what the kernels are handed
    def x_cl(self, fmt):
        """[b, t, Cp] in the operand type, pad channels zero (channel-first fp32 for first_conv / cf_to_cl: ``x`` itself)."""
        return fmt.round(to_cl(self.x, pad64(self.c_in))).to(fmt.dtype)

    def res_cl(self, fmt):
        return fmt.round(to_cl(self.res, pad64(self.c_out))).to(fmt.dtype)

    def operand(self, t, fmt):
        """The float64 image of what the kernel reads of an activation tensor."""
        return t if self.kind in ("first_conv", "cf_to_cl") and t is self.x else fmt.round(t)


def to_cl(y, cp):
    """[b, c, t] -> [b, t, cp], pad channels zero."""
    b, c, t = y.shape
    out = y.new_zeros((b, t, cp))
    out[:, :, :c] = y.transpose(1, 2)
    return out


# ------------------------------------------------------------------------------------------------------- float64 restatements
def fold(g, v):
    """weight_norm over dim 0 (dac WNConv1d / WNConvTranspose1d): w = g v / ||v||, float64."""
    v = v.double()
    norm = v.flatten(1).norm(dim=1).view(-1, *([1] * (v.dim() - 1)))
    return v * (g.double().view_as(norm) / norm)


def snake(v, alpha, beta):
    """SnakeBeta, alpha_logscale: v + sin^2(e^alpha v) / (e^beta + 1e-9); v [b, c, t]."""
    a, b = torch.exp(alpha.double()).view(1, -1, 1), torch.exp(beta.double()).view(1, -1, 1)
    return v + torch.sin(a * v).pow(2) / (b + 1e-9)


def activation(v, act, alpha, beta):
    return snake(v, alpha, beta) if act == "snake" else F.elu(v)


def reference(case, fmt, round_mid=True, drop_tap=None):
    """{"raw": the linear result, "snk": the activated one} as [b, t, Cp] float64, or {"cf": [b, c, t]} for the last convolutions.
    Weights are folded in float64 and rounded to the format where the kernel rounds the very same number (not for the nearest form, whose
    kernel rounds per-phase SUMS of taps: the reference keeps the exact taps there, and for the first convolution, whose weights stay fp32).
    round_mid=False leaves the tensor between a ResidualUnit's convolutions unrounded (the figure behind a wider gate, were one needed);
    drop_tap zeroes one tap of the (first) convolution: the planted fault of the host test."""
    k, c = case.kind, case
    rnd = lambda t: fmt.round(t.float()).double() if fmt.name != "f32" else t.float().double()
    x = c.operand(c.x, fmt).double()
    if k == "cf_to_cl":
        return {"raw": to_cl(x, pad64(c.c_in))}
    w = fold(c.weight_g, c.weight_v)
    if k not in ("nearest", "first_conv"):
        w = rnd(w)
    if drop_tap is not None:
        w = w.clone()
        w[:, :, drop_tap] = 0.0
    bias = None if c.bias is None else c.bias.double()
    if k == "conv7":
        y = F.conv1d(x, w, bias, dilation=c.dilation, padding=3 * c.dilation)
    elif k == "conv1_res":
        y = F.conv1d(x, w, bias) + rnd(c.res)
    elif k == "residual":
        h = activation(F.conv1d(x, w, bias, dilation=c.dilation, padding=3 * c.dilation), c.act, c.alpha, c.beta)
        if round_mid:
            h = rnd(h)
        y = F.conv1d(h, rnd(fold(c.weight_g2, c.weight_v2)), c.bias2.double()) + rnd(c.res)
        return {"raw": to_cl(y, pad64(c.c_out)), "snk": to_cl(activation(y, c.act, c.alpha2, c.beta2), pad64(c.c_out))}
    elif k == "convt":
        y = F.conv_transpose1d(x, w, bias, stride=c.stride, padding=math.ceil(c.stride / 2))
    elif k == "nearest":
        y = F.conv1d(F.interpolate(x, scale_factor=c.stride, mode="nearest"), w, None, padding="same")
    elif k == "strided":
        y = F.conv1d(x, w, bias, stride=c.stride, padding=math.ceil(c.stride / 2))
    elif k == "first_conv":
        y = F.conv1d(x, w, bias, padding=3)
    elif k == "final_dec":
        y = F.conv1d(x, w, None, padding=3)
        return {"cf": torch.tanh(y) if c.tanh else y}
    elif k == "final_enc":
        return {"cf": F.conv1d(x, w, bias, padding=1)}
    else:
        raise ValueError(k)
    return {"raw": to_cl(y, pad64(c.c_out)), "snk": to_cl(activation(y, c.act, c.alpha, c.beta), pad64(c.c_out))}


def snake_arguments(case, fmt):
    """Every Snake the case evaluates: [(|e^alpha v| [b, c, t], 1 / (e^beta + 1e-9) [c], the Snake's result [b, c, t]), ...]."""
    if case.act != "snake" or case.kind in ("final_dec", "final_enc", "cf_to_cl"):
        return []
    c = case
    rnd = lambda t: fmt.round(t.float()).double() if fmt.name != "f32" else t.float().double()
    x = c.operand(c.x, fmt).double()
    w = fold(c.weight_g, c.weight_v)
    out = []
    arg = lambda v, al, be: ((torch.exp(al.double()).view(1, -1, 1) * v).abs(), 1.0 / (torch.exp(be.double()) + 1e-9), snake(v, al, be))
    if c.kind == "residual":
        h = F.conv1d(x, rnd(w), c.bias.double(), dilation=c.dilation, padding=3 * c.dilation)
        out.append(arg(h, c.alpha, c.beta))
        ref = reference(c, fmt)
        out.append(arg(ref["raw"][:, :, :c.c_out].transpose(1, 2), c.alpha2, c.beta2))
    else:
        ref = reference(c, fmt)
        out.append(arg(ref["raw"][:, :, :c.c_out].transpose(1, 2), c.alpha, c.beta))
    return out


# ------------------------------------------------------------------------------------------------------------------- the gates
def gate_cl(name, got, want, fmt, parts=("whole", "rows", "blocks")):
    """A channels-last output [b, t, Cp]: the whole tensor, then per (batch item, time row) and per 32 x 32 block per batch item
    (``parts``: the host test asks for one of the three at a time)."""
    t, rnd = tol(fmt), out_round(fmt)
    assert got.shape == want.shape, f"{name}: shape {tuple(got.shape)}, expected {tuple(want.shape)}"
    if "whole" in parts:
        assert_close_sliced(f"{name} whole", got, want, t, (), rnd)
    for b in range(want.shape[0]):
        if "rows" in parts:
            assert_close_sliced(f"{name} item {b} per row", got[b], want[b], t, (0,), rnd)
        if "blocks" in parts:
            assert_close_sliced(f"{name} item {b} per 32x32 block", blocks32(got[b]), blocks32(want[b]), t, (0, 2), rnd)


def windows64(x):
    """[c, m] -> [c, ceil(m / 64), 64], the tail padded with zeros (which add nothing to either norm)."""
    x = x.detach().to("cpu", torch.float64)
    c, m = x.shape
    mp = (m + 63) // 64 * 64
    out = torch.zeros((c, mp), dtype=torch.float64)
    out[:, :m] = x
    return out.view(c, mp // 64, 64)


def gate_cf(name, got, want, fmt):
    """A channel-first fp32 output [b, c, m]: the whole tensor, then per (batch item, channel, 64-sample window)."""
    t = tol(fmt)
    assert got.shape == want.shape, f"{name}: shape {tuple(got.shape)}, expected {tuple(want.shape)}"
    assert_close_sliced(f"{name} whole", got, want, t, ())
    for b in range(want.shape[0]):
        assert_close_sliced(f"{name} item {b} per channel and 64-sample window", windows64(got[b]), windows64(want[b]), t, (0, 1))


def assert_pad_zero(name, got, c):
    """Pad channels c.. of a [b, t, Cp] tensor are zero bit for bit (the next layer's zero-padded weights rely on nothing, its Snake does)."""
    pad = got[:, :, c:]
    if pad.numel():
        bits = pad.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[pad.element_size()])
        n = int((bits != 0).sum())
        assert n == 0, f"{name}: {n} pad-channel elements are not bitwise zero"
