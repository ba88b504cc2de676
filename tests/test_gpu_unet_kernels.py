"""The U-Net's own kernels (csrc/unet_kernels.hip) alone, through their unit entries, against float64 PyTorch on the same fp32 inputs
(tests/unet_units.py), every output inside a guard band that must come back untouched.

GroupNorm statistics and apply: 3 x 128, 1064 x 128 and 2051 x 512 rows per item (a fraction of one partial tile; 33 and a quarter; 257 with a
short last one, more partials than the finish has threads), two items of different statistics, common-mode ratio |mean| / std 0 and 8.  fp32
outputs 1e-5 per element relative to max(|want|, the row's rms); 16-bit outputs within one code of the format plus that fp32 gate of the
float64 result (unet_units.rounded_share says why the code is counted on the absolute scale).  The fp32 restatement on the CPU passes the
1e-5 gate with a factor 5 to spare at both ratios (worst element 0.20 of the gate, at ratio 8), so the gate stands as stated.
Resamplers: lengths 4 (downsample only: the upsampler's smallest input is 3), 6, 24 and 1064, element by element under
(8 + 4) 2^-24 sum |k| |x|, the reflected rows at both ends on their own.  Boundary kernels: under the a-priori bound of an fp32 contraction,
(n + 4) 2^-24 |A| |W|^T (tests/fp32_units.py), the first and last k // 2 rows -- where the timestep planes are clipped -- on their own."""
import pytest
import torch
import torch.nn.functional as F

import fp32_units as fu
import unet_units as UU
from util import guarded

pytestmark = pytest.mark.gpu


def _lib():
    from stable_audio_tools import _hip
    return _hip, _hip.lib()


def _stats(dev, x):
    _hip, lib = _lib()
    b, n = x.shape[0], x[0].numel()
    tiles = lib.sat_unet_groupnorm_partials(n)
    part = guarded((b * tiles, 2), torch.float32, dev, name="GroupNorm partials")
    stats = guarded((b, 2), torch.float32, dev, name="GroupNorm statistics")
    _hip.check(lib.sat_unet_groupnorm_stats(_hip.ptr(x), _hip.ptr(part.t), _hip.ptr(stats.t), b, n, 1e-5, _hip.stream()))
    torch.cuda.synchronize()
    part.check().assert_written()
    stats.check().assert_written()
    return stats.t


@pytest.mark.parametrize("ratio", UU.GN_RATIOS)
@pytest.mark.parametrize("rows,c", UU.GN_SHAPES)
def test_groupnorm_stats_and_apply(dev, rows, c, ratio):
    _hip, lib = _lib()
    x = UU.gn_input(rows, c, ratio)
    g = torch.Generator().manual_seed(rows + c)
    gamma, beta = 1 + 0.2 * torch.randn(c, generator=g), 0.05 * torch.randn(c, generator=g)
    skip = torch.randn(x.shape, generator=g)
    xd, gd, bd, sd = (v.to(dev).contiguous() for v in (x, gamma, beta, skip))
    stats = _stats(dev, xd)
    want_stats, _ = UU.gn_reference(x, gamma, beta, None, 0)
    # mean to 1e-5 of the item's scale (std, or |mean| where that is larger), rstd to 1e-5 relative
    std = 1.0 / want_stats[:, 1]
    e_mean = ((stats[:, 0].cpu().double() - want_stats[:, 0]).abs() / torch.maximum(std, want_stats[:, 0].abs())).max().item()
    e_rstd = ((stats[:, 1].cpu().double() - want_stats[:, 1]).abs() / want_stats[:, 1]).max().item()
    print(f"\n[groupnorm {rows}x{c} ratio {ratio}] mean off by {e_mean:.2e} of the item's scale, rstd by {e_rstd:.2e}")
    assert e_mean <= 1e-5 and e_rstd <= 1e-5, (e_mean, e_rstd)
    for act, with_skip in ((1, True), (0, False)):
        _, want = UU.gn_reference(x, gamma, beta, skip if with_skip else None, act)
        for fmt in ("fp32", "fp16", "bf16"):
            dt = UU.TORCH_DTYPE[fmt]
            ld = c + 8
            out32 = guarded(x.shape, torch.float32, dev, name="apply fp32 stream")
            out_op = guarded((x.shape[0] * rows, ld), dt, dev, name=f"apply {fmt} operand")
            out_op.t.zero_()
            _hip.check(lib.sat_unet_groupnorm_apply(_hip.ptr(xd), _hip.ptr(stats), _hip.ptr(gd), _hip.ptr(bd), _hip.ptr(sd) if with_skip else None,
                                                    _hip.ptr(out32.t), _hip.ptr(out_op.t), x.shape[0], rows, c, ld, act, UU.FMT[fmt], _hip.stream()))
            torch.cuda.synchronize()
            out32.check().assert_written()
            out_op.check()
            share = UU.elementwise_share(out32.t.cpu(), want)
            assert share <= 1.0, f"apply fp32 act {act}: an element is {share:.2f} times 1e-5 of its scale"
            op = out_op.t[:, :c].cpu().reshape(x.shape)
            assert bool((out_op.t[:, c:] == 0).all()), "the apply wrote past the c columns of a row of ld"
            if fmt == "fp32":
                assert torch.equal(op, out32.t.cpu())
            else:
                scale = torch.maximum(want.abs(), want.pow(2).mean(dim=-1, keepdim=True).sqrt())
                dist = UU.rounded_share(op, want, dt, 1e-5 * scale)
                assert dist <= 1.0, f"apply {fmt} act {act}: an element is {dist:.2f} times one code plus the fp32 gate from the float64 result"
    print(f"    apply: fp32 within 1e-5 per element, fp16 / bf16 within one code")


def test_groupnorm_fp32_restatement_passes_with_margin():
    """The condition on the inputs: the same arithmetic in fp32 on the CPU (a two-pass mean / variance) passes the gates with a factor 4 to
    spare at ratio 0 and at ratio 8 -- the gates are not an artefact of float64."""
    for rows, c in UU.GN_SHAPES:
        for ratio in UU.GN_RATIOS:
            x = UU.gn_input(rows, c, ratio)
            gamma, beta = torch.ones(c), torch.zeros(c)
            _, want = UU.gn_reference(x, gamma, beta, None, 1)
            _, got = UU.gn_reference(x, gamma, beta, None, 1, dtype=torch.float32)
            assert UU.elementwise_share(got, want) <= 0.25, (rows, c, ratio, UU.elementwise_share(got, want))


@pytest.mark.parametrize("length", UU.RESAMPLE_LENGTHS)
@pytest.mark.parametrize("up", [False, True])
def test_resamplers(dev, length, up):
    _hip, lib = _lib()
    if up and length == 4:
        length = 3      # the upsampler's smallest input: the deepest level of a legal length
    b, c = 2, 128
    g = torch.Generator().manual_seed(length + 7 * up)
    x = torch.randn(b, c, length, generator=g)                 # channel-first for the reference
    rows = x.transpose(1, 2).contiguous().to(dev)              # [b * s, c]
    out_len = length * 2 if up else length // 2
    want = (UU.upsample if up else UU.downsample)(x.double())
    bound = UU.resample_bound(x, up)
    for fmt in ("fp32", "fp16"):
        dt = UU.TORCH_DTYPE[fmt]
        if up:
            ld = 2 * c
            out = guarded((b * out_len, ld), dt, dev, name="upsample concat half")
            out.t.zero_()
            _hip.check(lib.sat_unet_upsample(_hip.ptr(rows), _hip.ptr(out.t), b, length, c, ld, UU.FMT[fmt], _hip.stream()))
            torch.cuda.synchronize()
            out.check()
            assert bool((out.t[:, c:] == 0).all()), "the upsampler wrote into the skip half of the concat buffer"
            got = out.t[:, :c]
        else:
            out32 = guarded((b * out_len, c), torch.float32, dev, name="downsample fp32")
            out = guarded((b * out_len, c), dt, dev, name="downsample operand")
            _hip.check(lib.sat_unet_downsample(_hip.ptr(rows), _hip.ptr(out32.t), _hip.ptr(out.t), b, length, c, UU.FMT[fmt], _hip.stream()))
            torch.cuda.synchronize()
            out32.check().assert_written()
            out.check().assert_written()
            got = out.t if fmt == "fp32" else None
            if fmt != "fp32":
                assert UU.rounded_share(out.t, want.transpose(1, 2).reshape(b * out_len, c), dt, bound.transpose(1, 2).reshape(b * out_len, c)) <= 1.0
                got = out32.t
        got = got.cpu().float().view(b, out_len, c).transpose(1, 2)
        if fmt == "fp32" or not up:
            share = ((got.double() - want).abs() / bound.clamp_min(1e-300))
            edge = 4 if up else 2                                  # output positions that read a reflected row
            ends = torch.cat([share[..., :edge], share[..., -edge:]], dim=-1).max().item()
            print(f"\n[{'up' if up else 'down'}sample {length} {fmt}] worst element at {share.max().item():.3f} of the bound, reflected ends {ends:.3f}")
            assert ends <= 1.0, f"a reflected row is {ends:.2f} times its bound"
            assert share.max().item() <= 1.0
        else:
            assert UU.rounded_share(got, want, dt, bound) <= 1.0


def _bound_check(name, got, want, mag, n, rows_of_interest):
    share = fu.bound_share(got, want, mag, n)
    worst, ends = float(share.max()), float(share[rows_of_interest].max())
    print(f"\n[{name}] worst element at {worst:.3f} of (n + 4) 2^-24 |A| |W|^T, n = {n}; clipped rows {ends:.3f}")
    assert ends <= 1.0, f"{name}: a clipped row is {ends:.2f} times its bound"
    assert worst <= 1.0, f"{name}: an element is {worst:.2f} times its a-priori bound"


@pytest.mark.parametrize("taps,bias", [(5, True), (3, False), (7, True), (1, True)])
@pytest.mark.parametrize("b,io,t,c", [(2, 2, 24, 128), (1, 1, 1064, 256), (3, 2, 6, 128), (1, 112, 33, 128)])
def test_input_boundary(dev, b, io, t, c, taps, bias):
    _hip, lib = _lib()
    g = torch.Generator().manual_seed(b * 1000 + t + taps)
    cin, hw = io + 16, taps // 2
    x, ts = torch.randn(b, io, t, generator=g), torch.rand(b, generator=g)
    w_embed = torch.randn(8, 1, generator=g)
    w_main, b_main, w_skip = torch.randn(c, cin, taps, generator=g) / 8, torch.randn(c, generator=g) / 8, torch.randn(c, cin, 1, generator=g) / 4
    in_scale = 0.7
    y = guarded((b * t, c), torch.float32, dev, name="input boundary main")
    sk = guarded((b * t, c), torch.float32, dev, name="input boundary skip")
    d = lambda v: v.to(dev).contiguous()
    xd, td, wed, wmd, bmd, wsd = d(x), d(ts), d(w_embed), d(w_main), d(b_main), d(w_skip)
    _hip.check(lib.sat_unet_input(_hip.ptr(xd), _hip.ptr(td), in_scale, _hip.ptr(wed), _hip.ptr(wmd), _hip.ptr(bmd) if bias else None, _hip.ptr(wsd),
                                  _hip.ptr(y.t), _hip.ptr(sk.t), b, io, t, c, taps, _hip.stream()))
    torch.cuda.synchronize()
    y.check().assert_written()
    sk.check().assert_written()
    # the concatenated input as the kernel forms it: x * in_scale in fp32, the planes from fp32 cos / sin (their argument error is the
    # embedding's own, not the contraction's: the reference here takes the fp32 planes as given)
    planes = UU.timestep_planes({"timestep_embed.weight": w_embed}, ts, t, torch.float32)
    inp = torch.cat([(x * in_scale), planes], dim=1).double()
    wm, ws = w_main.double(), w_skip.double()
    bias64 = b_main.double() if bias else None
    rows = lambda v: v.transpose(1, 2).reshape(b * t, c)
    want = rows(F.conv1d(inp, wm, bias64, padding=hw))
    mag = rows(F.conv1d(inp.abs(), wm.abs(), bias64.abs() if bias else None, padding=hw))
    # fp32 cos / sin of an argument up to |2 pi w| ~ 20 differ between implementations by a few 2^-24 of the ARGUMENT: allow the planes 32
    # units each, i.e. add their share of the magnitude 32 / (n + 4) times over
    n = cin * taps
    pl = torch.cat([torch.zeros_like(x), torch.ones_like(planes)], dim=1).double()
    mag_main = mag + rows(F.conv1d(pl, wm.abs(), None, padding=hw)) * 32 / (n + 4)
    clipped = torch.zeros(b, t, dtype=torch.bool)
    clipped[:, :max(hw, 1)] = True
    clipped[:, t - max(hw, 1):] = True
    _bound_check(f"input main b={b} io={io} t={t} c={c} k={taps}", y.t, want, mag_main, n, clipped.flatten())
    want_s, mag_s = rows(F.conv1d(inp, ws)), rows(F.conv1d(inp.abs(), ws.abs()) + F.conv1d(pl, ws.abs()) * 32 / (cin + 4))
    _bound_check(f"input skip b={b} io={io} t={t} c={c}", sk.t, want_s, mag_s, cin, clipped.flatten())


@pytest.mark.parametrize("taps,bias", [(5, True), (3, False)])
@pytest.mark.parametrize("b,io,t,c", [(2, 2, 24, 128), (1, 1, 1064, 256), (3, 2, 6, 128), (1, 7, 65, 128)])
def test_output_boundary(dev, b, io, t, c, taps, bias):
    _hip, lib = _lib()
    g = torch.Generator().manual_seed(b * 1000 + t + taps + 1)
    h, xin = torch.randn(b, c, t, generator=g), torch.randn(b, c, t, generator=g)
    w_main, b_main, w_skip = torch.randn(io, c, taps, generator=g) / 16, torch.randn(io, generator=g) / 8, torch.randn(io, c, 1, generator=g) / 8
    out = guarded((b, io, t), torch.float32, dev, name="output boundary")
    rows = lambda v: v.transpose(1, 2).contiguous().view(b * t, c).to(dev)
    hd, xd, wmd, bmd, wsd = rows(h), rows(xin), w_main.to(dev), b_main.to(dev), w_skip.to(dev).contiguous()
    _hip.check(lib.sat_unet_output(_hip.ptr(hd), _hip.ptr(xd), _hip.ptr(wmd), _hip.ptr(bmd) if bias else None, _hip.ptr(wsd), _hip.ptr(out.t), b, io, t, c,
                                   taps, _hip.stream()))
    torch.cuda.synchronize()
    out.check().assert_written()
    bias64 = b_main.double() if bias else None
    want = F.conv1d(h.double(), w_main.double(), bias64, padding=taps // 2) + F.conv1d(xin.double(), w_skip.double())
    mag = F.conv1d(h.double().abs(), w_main.double().abs(), bias64.abs() if bias else None, padding=taps // 2) + F.conv1d(xin.double().abs(), w_skip.double().abs())
    share = fu.bound_share(out.t, want, mag, c * taps + c)
    print(f"\n[output b={b} io={io} t={t} c={c} k={taps}] worst element at {float(share.max()):.3f} of the bound")
    assert float(share.max()) <= 1.0


def test_cast_rows(dev):
    _hip, lib = _lib()
    x = torch.randn(37, 128, generator=torch.Generator().manual_seed(1))
    xd = x.to(dev)
    for fmt in ("fp32", "fp16", "bf16"):
        dt = UU.TORCH_DTYPE[fmt]
        out = guarded((37, 256), dt, dev, name="concat skip half")
        out.t.zero_()
        view = out.t[:, 128:]
        _hip.check(lib.sat_unet_cast_rows(_hip.ptr(xd), ctypes_ptr(view), 37, 128, 256, UU.FMT[fmt], _hip.stream()))
        torch.cuda.synchronize()
        out.check()
        assert bool((out.t[:, :128] == 0).all()) and torch.equal(out.t[:, 128:].cpu(), x.to(dt))


def ctypes_ptr(view):
    import ctypes
    return ctypes.c_void_p(view.data_ptr())


def test_entries_refuse_what_the_kernels_cannot_do(dev):
    _hip, lib = _lib()
    x = torch.zeros(4096, device=dev)
    p, s = _hip.ptr(x), _hip.stream()
    assert lib.sat_unet_groupnorm_stats(p, p, p, 1, 6, 1e-5, s) == -1
    assert lib.sat_unet_downsample(p, p, None, 1, 3, 128, 2, s) == -1 and b"reflect" in lib.sat_last_error()
    assert lib.sat_unet_upsample(p, p, 1, 2, 128, 128, 2, s) == -1 and b"reflect" in lib.sat_last_error()
    assert lib.sat_unet_input(p, p, 1.0, p, p, p, p, p, p, 1, 113, 8, 128, 5, s) == -2 and b"128" in lib.sat_last_error()
    assert lib.sat_unet_input(p, p, 1.0, p, p, p, p, p, p, 1, 2, 8, 128, 4, s) == -2 and b"kernel_size" in lib.sat_last_error()
    assert lib.sat_unet_output(p, p, p, p, p, p, 1, 2, 8, 96, 5, s) == -2 and b"multiple of 64" in lib.sat_last_error()
    assert lib.sat_unet_groupnorm_apply(p, p, p, p, None, None, None, 1, 3, 128, 128, 1, 2, s) == -1
