"""The output of a U-Net call depends on weights and inputs only (tests/test_gpu_state_independence.py states the property for the other
plans): case A's forward gives the same bits twice, on a workspace filled with each pattern of util.WORKSPACE_FILLS (the GroupNorm partials
and statistics, the q / k / v pads, the concat buffers and the streams all live there), behind a larger call that leaves its rows in the
grown workspace, and behind a call on all-NaN input, against a fresh module.  Case B repeats the two-call check where the GroupNorm partials
come from many tiles and the attention walks several key tiles."""
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
import unet_cases as UC  # noqa: E402
from test_gpu_unet import unet  # noqa: E402

pytestmark = pytest.mark.gpu

FMTS = ["fp16", "bf16", "fp32"]


@pytest.mark.parametrize("fmt", FMTS)
def test_ignores_workspace_contents(dev, fmt):
    x, t = (v.to(dev) for v in UC.inputs("A"))
    m = unet("A", dev, fmt)
    check_poisoned_workspace(f"unet A forward ({fmt})", lambda: m(x, t), m)


@pytest.mark.parametrize("fmt", ["fp16", "fp32"])
def test_many_tile_case_repeats_bit_for_bit(dev, fmt):
    x, t = (v.to(dev) for v in UC.inputs("B"))
    m = unet("B", dev, fmt)
    first = _sync(m(x, t))
    assert_bit_equal(f"unet B forward ({fmt}): two identical calls", _sync(m(x, t)), first)


@pytest.mark.parametrize("fmt", FMTS)
def test_forgets_larger_and_nan_calls(dev, fmt):
    from stable_audio_tools import synthetic
    x, t = (v.to(dev) for v in UC.inputs("A"))
    fresh = unet("A", dev, fmt)
    want = _sync(fresh(x, t))
    assert bool(torch.isfinite(want).all())
    big_x = synthetic.synth_input("unet_state_big", (3, 2, 48), 5).to(dev)
    big_t = torch.tensor([0.1, 0.5, 0.9], device=dev)
    for what, (fx, ft) in (("a larger call (batch 3, 48 samples)", (big_x, big_t)), ("an all-NaN call", (torch.full_like(x, float("nan")), t))):
        used = unet("A", dev, fmt)
        _sync(used(fx, ft))
        ws = used._ws
        got = _sync(used(x, t))
        assert used._ws is ws, "the second call replaced the workspace the first one left"
        if fx is big_x:
            assert ws.numel() > fresh._ws.numel()
        assert_bit_equal(f"unet A forward behind {what} ({fmt}), against a fresh module", got, want)
