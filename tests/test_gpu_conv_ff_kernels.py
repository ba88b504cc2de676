"""The convolution GEMM of the convolutional feed-forward (sat_dit_plan_set_ff_conv; csrc/ff_conv.hip) alone, through sat_ff_conv -- the plan's
own packing and launches -- against the float64 restatement of tests/conv_ff_units.py on the same rounded operands, in bf16, fp16 and fp32.

Gates.  16-bit operands: the tolerances of the GEMM unit tests of tests/test_gpu_kernels.py, whole, per row and per 32 x 32 accumulator block --
the fp32-output epilogue (FF-out: bias + residual) at 1e-3 (bf16) / 1e-5 (fp16) as test_gemm_f32 (same operands in, fp32 accumulation: only
the summation order differs), the 16-bit SiLU epilogue (FF-in) at fmt.tol(4e-3) with the output rounding's spread as test_gemm_silu_epilogue.
fp32: element by element under the a-priori bound (n + 4) 2^-24 (|A| |W|^T + |bias| + |C_in|), n = k K, as tests/test_gpu_fp32_kernels.py,
and per row / block at 1e-5; behind the SiLU the bound is multiplied by 1.1 (max |silu'| = 1.0998) and 8 units of |silu(x)| + 2^-24 are added
for the device's expf and division.

Shapes, K = 128: (2, 78) k 3 a sequence seam mid-tile; (4, 78) k 3 is 312 rows, the 128-row tile seams 128 and 256 fall inside sequences 1
and 3 (first row 234); (3, 1) and (3, 2) k 5: every tap but the centre is partly or wholly padding; (1, 300) k 7.  Every sequence has its own
scale (x 1, 10, 100, ...), so one leaked row of a neighbour dominates the window it enters.  Outputs sit in NaN guard bands; the workspace
is poisoned with NaN before the call (whatever the kernels read of it, the call must have written) and guarded as well; the tap-major weight
image at its start must equal conv_ff_units.pack_taps bit for bit."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import conv_ff_units as cu
from util import FORMATS, assert_close, assert_close_rows_blocks, guarded

pytestmark = pytest.mark.gpu

K = 128
SHAPES = [(2, 78, 3), (4, 78, 3), (3, 1, 5), (3, 2, 5), (1, 300, 7)]
EPILOGUES = [(0, 128), (1, 256)]          # (epilogue, N): FF-out with the residual, FF-in with SiLU
GEMM_FORMAT = {"bf16": 0, "f16": 3, "fp32": 2}          # SAT_GEMM_BF16 / SAT_GEMM_FP16 / SAT_GEMM_FP32X


def _operands(b, s, k, n, bias, dtype):
    gen = torch.Generator().manual_seed(10000 * b + 100 * s + 10 * k + n)
    a = torch.randn((b, s, K), generator=gen) * (10.0 ** torch.arange(b, dtype=torch.float32))[:, None, None]
    a = a.to(dtype)
    # every tap has its own weights and offset, so a dropped, repeated or reversed tap cannot pass
    w = torch.randn((n, K, k), generator=gen) * 0.05 + torch.linspace(-0.02, 0.03, k)[None, None, :]
    bv = torch.randn((n,), generator=gen) if bias else None
    c0 = torch.randn((b * s, n), generator=gen)
    return a, w, bv, c0


def _call(dev, fmt_name, dtype, a, w, bv, epi, out, gate=None):
    from stable_audio_tools import _hip
    lib = _hip.lib()
    b, s, _ = a.shape
    n, _, k = w.shape
    need = ctypes.c_size_t()
    _hip.check(lib.sat_ff_conv_workspace_bytes(GEMM_FORMAT[fmt_name], b, s, n, K, k, ctypes.byref(need)))
    ws = guarded(((need.value + 3) // 4,), torch.float32, dev, name="workspace", pitch=64)          # NaN inside and around
    ad = a.reshape(b * s, K).contiguous().to(dev)
    wd, bd = w.contiguous().to(dev), None if bv is None else bv.to(dev)
    _hip.check(lib.sat_ff_conv(GEMM_FORMAT[fmt_name], _hip.ptr(ad), _hip.ptr(wd), _hip.ptr(bd), epi, _hip.ptr(out.t), _hip.ptr(gate), b, s, n, K, k,
                               _hip.ptr(ws.t), need.value, _hip.stream()))
    torch.cuda.synchronize()
    ws.check()
    out.check().assert_written()
    # the packed image the kernels contracted with: tap-major, in the operand format
    item = torch.empty((), dtype=dtype).element_size()
    packed = ws.t.view(torch.uint8)[:n * k * K * item].view(dtype).view(n, k * K).cpu()
    want = cu.pack_taps(w).to(dtype)
    assert torch.equal(packed.view(torch.uint8), want.view(torch.uint8)), "the plan's tap-major packing differs from conv_ff_units.pack_taps"


@pytest.mark.parametrize("fmt", FORMATS, ids=repr)
@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("epi, n", EPILOGUES, ids=["ffout_resid", "ffin_silu"])
@pytest.mark.parametrize("b, s, k", SHAPES)
def test_ff_conv_16bit(dev, b, s, k, epi, n, bias, fmt):
    a, w, bv, c0 = _operands(b, s, k, n, bias, fmt.dtype)
    wr = w.to(fmt.dtype)
    pre = cu.conv_gemm(a, wr, bv)
    name = f"ff_conv {fmt} ({b}, {s}) k {k} n {n} epi {epi} {'bias' if bias else 'no bias'}"
    if epi == 0:
        out = guarded((b * s, n), torch.float32, dev, init=c0, name="residual rows")
        _call(dev, fmt.name, fmt.dtype, a, w, bv, epi, out)
        want, tol = (pre + c0.double()).float(), (1e-3 if not fmt.f16 else 1e-5)
        e = assert_close(name, out.t, want, tol)
        assert_close_rows_blocks(name, out.t, want, tol)
    else:
        out = guarded((b * s, n), fmt.dtype, dev, name="hidden rows")
        _call(dev, fmt.name, fmt.dtype, a, w, bv, epi, out)
        want, tol = F.silu(pre).float(), fmt.tol(4e-3)
        e = assert_close(name, out.t, want, tol)
        assert_close_rows_blocks(name, out.t, want, tol, fmt.round)
    print(f"\n[{name}] rel-L2 {e:.2e} (gate {tol:.1e})")


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("epi, n", EPILOGUES, ids=["ffout_resid", "ffin_silu"])
@pytest.mark.parametrize("b, s, k", SHAPES)
def test_ff_conv_fp32(dev, b, s, k, epi, n, bias):
    a, w, bv, c0 = _operands(b, s, k, n, bias, torch.float32)
    pre = cu.conv_gemm(a, w, bv)
    name = f"ff_conv fp32 ({b}, {s}) k {k} n {n} epi {epi} {'bias' if bias else 'no bias'}"
    steps = k * K + 4
    out = guarded((b * s, n), torch.float32, dev, init=c0 if epi == 0 else None, name="fp32 output")
    _call(dev, "fp32", torch.float32, a, w, bv, epi, out)
    if epi == 0:
        want = pre + c0.double()
        bound = steps * cu.UNIT * cu.magnitude(a, w, bv, c0)
    else:
        want = F.silu(pre)
        bound = 1.1 * steps * cu.UNIT * cu.magnitude(a, w, bv) + 8 * cu.UNIT * (want.abs() + cu.UNIT)
    err = (out.t.cpu().double() - want).abs()
    share = float((err / bound).max())
    print(f"\n[{name}] worst share of the a-priori bound {share:.3f}")
    assert share <= 1.0, f"{name}: element error at {share:.2f} of the a-priori bound ({steps} steps)"
    assert_close_rows_blocks(name, out.t, want.float(), 1e-5)


@pytest.mark.parametrize("fmt", ["bf16", "f16", "fp32"])
def test_ff_conv_gate(dev, fmt):
    """The adaLN gate of the FF-out epilogue: one vector per sequence, multiplied in before the residual add."""
    dtype = {"bf16": torch.bfloat16, "f16": torch.float16, "fp32": torch.float32}[fmt]
    b, s, k, n = 2, 78, 3, 128
    a, w, bv, c0 = _operands(b, s, k, n, True, dtype)
    gate = torch.randn((b, n), generator=torch.Generator().manual_seed(5))
    want = (cu.conv_gemm(a, w.to(dtype), bv).view(b, s, n) * gate.double()[:, None, :]).view(b * s, n) + c0.double()
    out = guarded((b * s, n), torch.float32, dev, init=c0, name="residual rows")
    _call(dev, fmt, dtype, a, w, bv, 0, out, gate=gate.to(dev))
    tol = {"bf16": 1e-3, "f16": 1e-5, "fp32": 1e-5}[fmt]
    assert_close(f"ff_conv gate {fmt}", out.t, want.float(), tol)
    assert_close_rows_blocks(f"ff_conv gate {fmt}", out.t, want.float(), tol)


@pytest.mark.parametrize("fmt", ["bf16", "f16", "fp32"])
def test_ff_conv_on_the_packed_image(dev, fmt):
    """w NULL: the call packs nothing and contracts with the image the first call left in the workspace -- the same bits out."""
    from stable_audio_tools import _hip
    lib = _hip.lib()
    dtype = {"bf16": torch.bfloat16, "f16": torch.float16, "fp32": torch.float32}[fmt]
    b, s, k, n = 2, 78, 3, 128
    a, w, bv, c0 = _operands(b, s, k, n, True, dtype)
    need = ctypes.c_size_t()
    _hip.check(lib.sat_ff_conv_workspace_bytes(GEMM_FORMAT[fmt], b, s, n, K, k, ctypes.byref(need)))
    ws = guarded(((need.value + 3) // 4,), torch.float32, dev, name="workspace", pitch=64)
    ad, wd, bd = a.reshape(b * s, K).contiguous().to(dev), w.contiguous().to(dev), bv.to(dev)
    outs = []
    for wp in (_hip.ptr(wd), None):
        out = guarded((b * s, n), torch.float32, dev, init=c0, name="residual rows")
        _hip.check(lib.sat_ff_conv(GEMM_FORMAT[fmt], _hip.ptr(ad), wp, _hip.ptr(bd), 0, _hip.ptr(out.t), None, b, s, n, K, k, _hip.ptr(ws.t), need.value,
                                   _hip.stream()))
        torch.cuda.synchronize()
        ws.check()
        out.check().assert_written()
        outs.append(out.t)
    assert torch.equal(outs[0], outs[1]), "the call on the packed image gives other bits than the call that packed it"


def test_ff_conv_refusals(dev):
    from stable_audio_tools import _hip
    lib = _hip.lib()
    z = torch.zeros(4096, device=dev)
    call = lambda fmt, epi, n, kk, k, ws_bytes: lib.sat_ff_conv(fmt, _hip.ptr(z), _hip.ptr(z), None, epi, _hip.ptr(z), None, 1, 2, n, kk, k, _hip.ptr(z),
                                                                 ws_bytes, _hip.stream())
    assert call(0, 0, 128, 128, 4, 1 << 20) == -2 and b"odd" in lib.sat_last_error()
    assert call(0, 0, 128, 128, 9, 1 << 20) == -2
    assert call(0, 0, 96, 128, 3, 1 << 20) == -2
    assert call(0, 0, 128, 96, 3, 1 << 20) == -2
    assert call(0, 2, 128, 128, 3, 1 << 20) == -1
    assert call(0, 0, 128, 128, 3, 16) == -4
    torch.cuda.synchronize()
