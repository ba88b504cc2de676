"""The boundary kernels of a patchified DiT (csrc/dit_patch.hip) alone, through their unit entries of include/sat_hip.h -- the launchers the
plan calls -- against float64 PyTorch on the same fp32 inputs (tests/dit_patch_units.py).

Gates, those of tests/test_gpu_fp32_kernels.py (fp32_units.check): every element under the a-priori bound (n + 4) 2^-24 |W| |x| with n the
contraction length, every row and 32 x 32 block at 1e-5; the copied prepend rows bit for bit.  Every output sits in a NaN guard band; what
the contract leaves alone (the global token's row) must still hold the sentinel.  That the references are right and that the gates reject an
(p c) feature order, a frame or row off by one, a per-token concat source and a scaled concat signal: tests/test_dit_patch_host.py."""
import pytest
import torch

import dit_patch_units as pu
import fp32_units as fu
from test_gpu_fp32_kernels import _Call, _untouched
from util import PARITY_LOG

pytestmark = pytest.mark.gpu
E_INVALID, E_UNSUPPORTED = -1, -2            # SAT_E_* of include/sat_hip.h


def _shapes(f):
    return pytest.mark.parametrize("p", pu.SHAPES, ids=pu.shape_id)(f)


def _check(case, got):
    fu.LOG.clear()
    try:
        fu.check(case, {k: v.cpu() for k, v in got.items()}, want=pu.reference(case))
    finally:
        if PARITY_LOG:
            with open(PARITY_LOG, "a") as f:
                for name, key, what, figure, where in fu.LOG:
                    f.write(f"dit_patch_units\t{name}\t{key}\t{what}\t{figure:.3e}\t{where}\n")


@_shapes
def test_fold_in_patch(dev, p):
    c = pu.Case("fold_in", p)
    t, d = c.t, c.dim
    ci = d["c"] + d["cc"]
    k = _Call(dev)
    g = k.out((ci * d["P"], d["d"]), "fold_in_patch weff_t")
    k.call("sat_fold_in_patch", k.up(t["w_in"]), k.up(t["w_pre"]), g.t.data_ptr(), d["d"], ci, d["P"])
    g.assert_written()
    _check(c, {"weff_t": g.t})


@_shapes
def test_fold_out_patch(dev, p):
    c = pu.Case("fold_out", p)
    t, d = c.t, c.dim
    k = _Call(dev)
    g = k.out((d["d"], d["c"] * d["P"]), "fold_out_patch weff_t")
    k.call("sat_fold_out_patch", k.up(t["w_out"]), k.up(t["w_post"]), g.t.data_ptr(), d["d"], d["c"], d["P"])
    g.assert_written()
    _check(c, {"weff_t": g.t})


@_shapes
def test_input_proj_patch(dev, p):
    """8 tokens x 256 channels per workgroup, P frames per token: one token, 9 (a partial last chunk), 19 at P = 4 on one and a half channel
    blocks, P = 8 and P = 3 (the kernel for any P), concat channels resized from a third of the frames and at the latent's own length with
    three prepend rows copied, two latents under four sequences, and xscale."""
    c = pu.Case("input_proj", p)
    t, d = c.t, c.dim
    k = _Call(dev)
    g = k.out((d["bf"], d["s"], d["d"]), "input_proj_patch X")
    k.call("sat_input_proj_patch", k.up(t["x"]), k.up(t["weff_in_t"]), g.t.data_ptr(), d["bf"], d["xb"], d["c"], d["P"], d["t"], d["s"], d["d"],
           d["xscale"], k.up(t["concat"]), d["cc"], d["tc"], k.up(t["prep"]), d["pl"])
    pre = d["s"] - d["tt"]
    g.assert_written(g.t[:, pre:])
    _untouched(g, g.t[:, d["pl"]:pre], "the global token's row")
    got = {"X": g.t[:, pre:]}
    if d["pl"]:
        got["prep"] = g.t[:, :d["pl"]]
    _check(c, got)


@_shapes
def test_output_proj_patch(dev, p):
    """8 tokens per workgroup and 64 output columns per column group: workgroups that straddle two sequences (the second is 8 x the others),
    partial last workgroups, one to four column groups, a partial one (P = 8, C = 8 is exactly 64; C = 4, P = 2 is 8 columns), channels whose
    columns lie in two groups (P = 3), prepended rows skipped."""
    c = pu.Case("output_proj", p)
    t, d = c.t, c.dim
    k = _Call(dev)
    g = k.out((d["bf"], d["c"], d["t"]), "output_proj_patch out", pitch=d["c"] * d["t"])
    k.call("sat_output_proj_patch", k.up(t["X"]), k.up(t["weff_out_t"]), g.t.data_ptr(), d["bf"], d["c"], d["P"], d["t"], d["s"], d["d"])
    g.assert_written()
    _check(c, {"out": g.t})


def test_patch_limits_are_refused_before_any_launch(dev):
    """C P = 516 > 512 is SAT_E_UNSUPPORTED in both launchers, a T that is no multiple of P SAT_E_INVALID, and nothing is written."""
    from stable_audio_tools import _hip
    lib = _hip.lib()
    k = _Call(dev)
    C, P, D = 4, 129, 128
    x, w_in, w_out = torch.zeros(1, C, P), torch.zeros(C * P, D), torch.zeros(D, C * P)
    gX = k.out((1, 1, D), "X of a refused input_proj_patch")
    go = k.out((1, C, P), "out of a refused output_proj_patch")
    X = torch.zeros(1, 1, D)
    assert lib.sat_input_proj_patch(k.up(x), k.up(w_in), gX.t.data_ptr(), 1, 1, C, P, P, 1, D, 1.0, None, 0, 0, None, 0, _hip.stream()) == E_UNSUPPORTED
    assert b"512" in lib.sat_last_error()
    assert lib.sat_output_proj_patch(k.up(X), k.up(w_out), go.t.data_ptr(), 1, C, P, P, 1, D, _hip.stream()) == E_UNSUPPORTED
    assert lib.sat_input_proj_patch(k.up(x), k.up(w_in), gX.t.data_ptr(), 1, 1, C, 2, 3, 1, D, 1.0, None, 0, 0, None, 0, _hip.stream()) == E_INVALID
    assert lib.sat_output_proj_patch(k.up(X), k.up(w_out), go.t.data_ptr(), 1, C, 2, 3, 1, D, _hip.stream()) == E_INVALID
    torch.cuda.synchronize()
    for g in (gX, go):
        g.check()
        _untouched(g, g.t, "the output of a refused call")
