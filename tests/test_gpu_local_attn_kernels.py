"""The two boundary kernels of the local-attention codec (csrc/local_attn_io.hip) alone, through their unit entries, against float64 PyTorch on
the same fp32 inputs: element by element under the a-priori bound of an fp32 contraction, (n + 4) 2^-24 |A| |W|^T (tests/fp32_units.py, the
bound tests/test_gpu_fp32_kernels.py uses), every output inside a guard band that must come back untouched.

Shapes: 1 and 2 input channels, 3 and 32 output channels (the one- and the two-accumulator build of project_out, one and four groups of
channels), d 128 and 384, t 1, 255
and 257 (less than one 64-step tile, a ragged last tile, one step into a fifth tile), batch 1 and 3 (tiles must not cross items)."""
import pytest
import torch

import fp32_units as fu
from util import guarded

pytestmark = pytest.mark.gpu

SHAPES = [(b, t, d) for b in (1, 3) for t in (1, 255, 257) for d in (128, 384)]


def _inputs(tag, *shapes):
    from stable_audio_tools import synthetic
    return [synthetic.synth_input(f"local_attn_kernels_{tag}_{i}", s, 23) for i, s in enumerate(shapes)]


def _check(name, got, want, mag, n):
    share = fu.bound_share(got, want, mag, n)
    worst = float(share.max())
    print(f"\n[{name}] worst element at {worst:.3f} of the bound (n + 4) 2^-24 |A| |W|^T, n = {n}")
    assert worst <= 1.0, f"{name}: an element is {worst:.2f} times its a-priori bound, the first at {tuple(int(i) for i in (share > 1).nonzero()[0])}"


@pytest.mark.parametrize("c_in", [1, 2])
@pytest.mark.parametrize("b,t,d", SHAPES)
def test_project_in(dev, b, t, d, c_in):
    from stable_audio_tools import _hip
    x, w = _inputs(f"in_{b}_{t}_{d}_{c_in}", (b, c_in, t), (d, c_in))
    out = guarded((b * t, d), torch.float32, dev, name="project_in rows")
    xd, wd = x.to(dev), w.to(dev)
    _hip.check(_hip.lib().sat_local_attn_project_in(_hip.ptr(xd), _hip.ptr(wd), _hip.ptr(out.t), b, c_in, t, d, _hip.stream()))
    torch.cuda.synchronize()
    out.check().assert_written()
    x64, w64 = x.double(), w.double()
    want = torch.einsum("bct,dc->btd", x64, w64).reshape(b * t, d)
    mag = torch.einsum("bct,dc->btd", x64.abs(), w64.abs()).reshape(b * t, d)
    _check(f"project_in b={b} c_in={c_in} t={t} d={d}", out.t, want, mag, c_in)


def test_project_in_walks_column_tiles(dev):
    """40 latent channels into 384 columns: the weight no longer fits one workgroup's LDS share (40 * 384 > 8192 floats) and the columns are
    walked in tiles of 204 and 180"""
    from stable_audio_tools import _hip
    b_, c_in, t, d = 2, 40, 130, 384
    x, w = _inputs("in_tiled", (b_, c_in, t), (d, c_in))
    out = guarded((b_ * t, d), torch.float32, dev, name="project_in rows")
    xd, wd = x.to(dev), w.to(dev)
    _hip.check(_hip.lib().sat_local_attn_project_in(_hip.ptr(xd), _hip.ptr(wd), _hip.ptr(out.t), b_, c_in, t, d, _hip.stream()))
    torch.cuda.synchronize()
    out.check().assert_written()
    want = torch.einsum("bct,dc->btd", x.double(), w.double()).reshape(b_ * t, d)
    mag = torch.einsum("bct,dc->btd", x.double().abs(), w.double().abs()).reshape(b_ * t, d)
    _check("project_in b=2 c_in=40 t=130 d=384", out.t, want, mag, c_in)


@pytest.mark.parametrize("c_out", [3, 32])
@pytest.mark.parametrize("b,t,d", SHAPES)
def test_project_out(dev, b, t, d, c_out):
    from stable_audio_tools import _hip
    rows, w = _inputs(f"out_{b}_{t}_{d}_{c_out}", (b * t, d), (c_out, d))
    out = guarded((b, c_out, t), torch.float32, dev, name="project_out audio")
    rd, wd = rows.to(dev), w.to(dev)
    _hip.check(_hip.lib().sat_local_attn_project_out(_hip.ptr(rd), _hip.ptr(wd), _hip.ptr(out.t), b, c_out, t, d, _hip.stream()))
    torch.cuda.synchronize()
    out.check().assert_written()
    r64, w64 = rows.double().view(b, t, d), w.double()
    want = torch.einsum("btd,od->bot", r64, w64)
    mag = torch.einsum("btd,od->bot", r64.abs(), w64.abs())
    _check(f"project_out b={b} c_out={c_out} t={t} d={d}", out.t, want, mag, d)


def test_entries_refuse_what_the_kernels_cannot_do(dev):
    from stable_audio_tools import _hip
    lib = _hip.lib()
    x = torch.zeros(4096, device=dev)
    p = _hip.ptr(x)
    assert lib.sat_local_attn_project_in(p, p, p, 1, 2, 8, 130, _hip.stream()) == -1 and b"multiple of 4" in lib.sat_last_error()
    assert lib.sat_local_attn_project_in(p, p, p, 1, 129, 8, 128, _hip.stream()) == -2 and b"c_in <= 128" in lib.sat_last_error()
    assert lib.sat_local_attn_project_out(p, p, p, 1, 2, 8, 96, _hip.stream()) == -1 and b"multiple of 64" in lib.sat_last_error()
    assert lib.sat_local_attn_project_out(p, None, p, 1, 2, 8, 128, _hip.stream()) == -1
