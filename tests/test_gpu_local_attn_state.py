"""The output of a local-attention codec call depends on weights and inputs only (tests/test_gpu_state_independence.py states the property for
the other plans): case A's encode and decode give the same bits on a workspace filled with each pattern of util.WORKSPACE_FILLS (the q / k /
v pads, the fp32 staging of the head split, the rotation tables and the ping-pong rows of the stream all live there), behind a larger call
that leaves its rows in the grown workspace, and behind a call on all-NaN input, against a fresh module."""
import os
import sys

import pytest
import torch

from util import assert_bit_equal
from test_gpu_state_independence import _sync, check_poisoned_workspace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
import local_attn_cases as LC  # noqa: E402
from test_gpu_local_attn import codec  # noqa: E402

pytestmark = pytest.mark.gpu

FMTS = ["fp16", "bf16", "fp32"]


def _inputs(dev):
    return LC.audio("A").to(dev), LC.load()["A_enc"].to(dev)


@pytest.mark.parametrize("fmt", FMTS)
def test_ignores_workspace_contents(dev, fmt):
    x, z = _inputs(dev)
    enc, dec = codec("A", "enc", dev, fmt), codec("A", "dec", dev, fmt)
    check_poisoned_workspace(f"local_attn A encode ({fmt})", lambda: enc(x), enc)
    check_poisoned_workspace(f"local_attn A decode ({fmt})", lambda: dec(z), dec)


@pytest.mark.parametrize("fmt", FMTS)
def test_forgets_larger_and_nan_calls(dev, fmt):
    from stable_audio_tools import synthetic
    x, z = _inputs(dev)
    fresh = codec("A", "enc", dev, fmt), codec("A", "dec", dev, fmt)
    want = _sync(fresh[0](x)), _sync(fresh[1](z))
    assert all(bool(torch.isfinite(w).all()) for w in want)
    big_x = synthetic.synth_input("local_attn_state_big_audio", (3, 2, 2112), 5, 0.5).to(dev)
    big_z = synthetic.synth_input("local_attn_state_big_latents", (3, 8, 528), 5).to(dev)
    for what, first in (("a larger call (batch 3, 2112 samples)", (big_x, big_z)),
                        ("an all-NaN call", (torch.full_like(x, float("nan")), torch.full_like(z, float("nan"))))):
        used = codec("A", "enc", dev, fmt), codec("A", "dec", dev, fmt)
        for m, inp in zip(used, first):
            _sync(m(inp))
        ws = used[0]._ws, used[1]._ws
        got = _sync(used[0](x)), _sync(used[1](z))
        assert used[0]._ws is ws[0] and used[1]._ws is ws[1], "the second call replaced the workspace the first one left"
        if first[0] is big_x:
            assert ws[0].numel() > fresh[0]._ws.numel() and ws[1].numel() > fresh[1]._ws.numel()
        assert_bit_equal(f"local_attn A encode behind {what} ({fmt}), against a fresh module", got[0], want[0])
        assert_bit_equal(f"local_attn A decode behind {what} ({fmt}), against a fresh module", got[1], want[1])
