"""The half-row schedule of the 8-phase SwiGLU GEMM (csrc/ph8_sched.h: ph8_half_rows_ints; csrc/gemm_ph8.hip): one full 256 x 256 tile and at
most one 128-row half tile per workgroup, the M tail of <= 16 rows as the extended block of a half tile.  Through the unit-level SwiGLU entry
points with and without the LayerNorm fold, both operand formats, variant 80 (the 8-phase kernel) against 80 | bit 27 (the same kernel on the
schedule this one replaces): bit-equal outputs, the test_gemm_swiglu gate against fp32 torch on the same rounded operands, and nothing written
at or beyond row M (the output sits in a NaN-filled allocation with 256 guard rows on each side).

Shapes (256 CUs):
  2050 x 12288 x 256   FF-in's tile pattern -- 256 full + 256 half tiles, 48 of them extended -- on the shortest K walk (two K-tiles: the
                       last-two-tiles path of the main loop only)
  1538 x 11008 x 384   t = 258 full tiles: two more than CUs, but the 2-row tail needs an extended half tile in each of the 43 columns, so 43 row
                       tiles are cut (86 half tiles); 170 workgroups hold a full tile only, 41 a half tile only
  2048 x 12288 x 256   no tail, no extended tile
  2064 x 12288 x 256   a full 16-row tail block
  2065 x 12288 x 256   tail of 17 rows: not eligible, both variants run the previous schedule"""
import pytest
import torch
import torch.nn.functional as F

from util import FORMATS, assert_close, assert_close_rows_blocks, guarded

pytestmark = pytest.mark.gpu

PH8 = 80                         # the 8-phase kernel, forced (gemm_tiles.h)
HALF_ROWS_OFF = 0x8000000        # SAT_VARIANT_HALF_ROWS_OFF
SHAPES = [(2050, 12288, 256), (1538, 11008, 384), (2048, 12288, 256), (2064, 12288, 256), (2065, 12288, 256)]


def _lib():
    from stable_audio_tools import _hip
    return _hip, _hip.lib()


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g) * scale


_CASES = {}


def _case(m, n, k, fmt, fold):
    """Operands and the fp32 reference of one case: computed once, shared, never modified."""
    key = (m, n, k, fmt.name, fold)
    if key not in _CASES:
        # rows distinct in scale and offset, weights asymmetric: a swapped or mis-based 128-row band cannot pass
        a = ((_rand((m, k), 9) * (0.5 + torch.linspace(0.0, 1.0, m)[:, None]) + torch.linspace(-0.3, 0.3, m)[:, None])).to(fmt.dtype)
        w = _rand((n, k), 10) * 0.08 + torch.linspace(-0.01, 0.01, n)[:, None]
        bias = _rand((n,), 11) * 0.1
        c = {"a": a, "w": w, "bias": bias}
        if fold:
            c["gamma"] = 0.8 + 0.2 * _rand((k,), 12)
            c["beta"] = 0.1 * _rand((k,), 13)
            blocks = a.float().view(m, k // 64, 64)
            c["part"] = torch.stack([blocks.sum(-1), (blocks * blocks).sum(-1)], dim=-1).contiguous()
            # what the consumer computes, in fp32 on the same rounded operands: rstd (xb (gamma w)^T - mean c1) + c2
            x = a.float()
            mean = x.mean(-1, keepdim=True)
            rstd = torch.rsqrt((x * x).mean(-1, keepdim=True) - mean * mean + 1e-5)
            wp = fmt.round(c["gamma"] * w)
            h = rstd * (x @ wp.T - mean * wp.sum(-1)) + ((w * c["beta"]).sum(-1) + bias)
        else:
            h = F.linear(a.float(), fmt.round(w), bias)
        val, gate = h.chunk(2, dim=-1)
        c["want"] = val * F.silu(gate)
        _CASES.clear()          # (one case's operands at a time)
        _CASES[key] = c
    return _CASES[key]


def _run(dev, c, m, n, k, fmt, fold, variant):
    _hip, lib = _lib()
    og = guarded((m, n // 2), fmt.dtype, dev, name="out")
    wp = torch.empty((n, k), dtype=fmt.dtype, device=dev)
    ad, wd, bd = c["a"].to(dev), c["w"].to(dev), c["bias"].to(dev)
    if fold:
        c12 = torch.empty((2 * n,), dtype=torch.float32, device=dev)
        pd, gd, btd = c["part"].to(dev), c["gamma"].to(dev), c["beta"].to(dev)
        _hip.check(fmt.fn(lib, "sat_gemm_swiglu_ln_bf16")(_hip.ptr(ad), _hip.ptr(pd), _hip.ptr(wd), _hip.ptr(gd), _hip.ptr(btd), _hip.ptr(bd), _hip.ptr(wp),
                                                          _hip.ptr(c12), _hip.ptr(og.t), m, n, k, variant, _hip.stream()))
    else:
        bp = torch.empty((n,), dtype=torch.float32, device=dev)
        _hip.check(fmt.fn(lib, "sat_gemm_swiglu_bf16")(_hip.ptr(ad), _hip.ptr(wd), _hip.ptr(bd), _hip.ptr(wp), _hip.ptr(bp), _hip.ptr(og.t), m, n, k,
                                                       variant, _hip.stream()))
    torch.cuda.synchronize()
    return og


@pytest.mark.parametrize("fmt", FORMATS, ids=repr)
@pytest.mark.parametrize("fold", [False, True], ids=["plain", "ln_fold"])
@pytest.mark.parametrize("m,n,k", SHAPES)
def test_half_rows_swiglu(dev, m, n, k, fold, fmt):
    c = _case(m, n, k, fmt, fold)
    new = _run(dev, c, m, n, k, fmt, fold, PH8)
    old = _run(dev, c, m, n, k, fmt, fold, PH8 | HALF_ROWS_OFF)
    for og in (new, old):
        og.check().assert_written()          # no row at or beyond M (nor in front of row 0) was written; every row below M was
    assert torch.equal(new.t, old.t), "the half-row schedule must reproduce the previous schedule bit for bit"
    name = f"swiglu half rows {m}x{n}x{k}" + (" ln-fold" if fold else "")
    assert_close(name, new.t, c["want"], fmt.tol(4e-3))
    assert_close_rows_blocks(name, new.t, c["want"], fmt.tol(4e-3), fmt.round)
