"""Cases of the Dance Diffusion U-Net (``DiffusionAttnUnet1D``, "model_type": "diffusion_uncond" / "type": "DAU1d"): configs, seeded weights
and inputs, and the gate figures the generator measured on the reference (tests/golden/make_golden_unet.py writes unet_small.npz and
unet_state_dict_keys.json; tests/test_gpu_unet.py and tests/test_unet_host.py read them).

Stored: the REFERENCE's outputs ``DiffusionAttnUnet1D(**config)(x, t)`` in fp32, with the input and the weight of every nn.Conv1d rounded to
fp16 / bf16 (``<case>__r16_<fmt>``, the yardstick of the 16-bit gates) and in float64 (``<case>__f64``, the yardstick of the fp32 gate).
Weights and inputs are regenerated from seeds.

The cases sit at the seams of the plan (csrc/unet_plan.hip):
  A   depth 4, channels [128, 128, 256, 256], n_attn_layers 2, batch 2, 24 samples: 24 / 12 / 6 / 3 rows per level -- a row tail under every
      tile, a batch seam, attention over 12, 6 and 3 keys (mostly pad keys), reflect pads at a 3-row level, both widths, the 1 x 1 skip and
      the 2 c concat convolution.  The reference fails at 16 samples.
  B   depth 3, channels [128, 256, 512], n_attn_layers 2, batch 1, 1064 samples: 1064 / 532 / 266 rows -- attention over 532 keys (several
      128-key tiles; 8 heads) and 266 keys (16 heads), GroupNorm partials from many tiles, K = 2560 with a 512-wide output.
  C   depth 2, channels [128, 128], no attention, kernel_size 3, conv_bias False, batch 3, 6 samples: the smallest legal shape.
"""
import math
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import cases  # noqa: E402  (puts the package on sys.path)
from stable_audio_tools import synthetic  # noqa: E402

STEM = "unet_small"
KEYS_PATH = os.path.join(HERE, "unet_state_dict_keys.json")
SEED = 17
FORMATS = ("fp16", "bf16", "fp32")

# case -> (constructor kwargs, batch, samples)
CASES = {
    "A": (dict(io_channels=2, depth=4, n_attn_layers=2, channels=[128, 128, 256, 256]), 2, 24),
    "B": (dict(io_channels=2, depth=3, n_attn_layers=2, channels=[128, 256, 512]), 1, 1064),
    "C": (dict(io_channels=2, depth=2, n_attn_layers=0, channels=[128, 128], kernel_size=3, conv_bias=False), 3, 6),
}


# ------------------------------------------------------------------------------------------------------------------ weights and inputs
# Every tensor is drawn, uniform in +-gain / sqrt(fan_in) with gain sqrt(3) (keeps the variance of a unit-variance input): a convolution
# in front of a GroupNorm is scale-free, so the gain matters for the 1 x 1 skips, qkv_proj, out_proj and the last convolution.  Stated
# gains: qkv_proj 0.5, out_proj 1; the GroupNorm weights of the blocks 0.5 (1 +- 0.2), so that a block adds a quarter of the stream's
# variance and the network stays residual -- with 1 +- 0.2 there, the reference's own bf16 figure of case B was 2.6e-2, above R16_LIMIT,
# whatever the attention gains; the attention norms keep 1 +- 0.2.  Every bias +-0.05, timestep_embed.weight standard normal as the
# reference draws it.  The resamplers' `kernel` buffers keep the module's values.  The generator asserts that every branch still moves
# the output by 5 % or more.
GAIN = math.sqrt(3.0)
GAINS = {"qkv_proj": 0.5, "out_proj": 1.0}
NORM_GAIN = 0.5


def weights(template_sd, seed=SEED):
    out = {}
    for key, t in template_sd.items():
        g = synthetic._gen(seed, key)
        u = lambda bound: (torch.rand(tuple(t.shape), generator=g, dtype=torch.float32) * 2 - 1) * bound
        if key.endswith(".kernel"):
            out[key] = t.clone().float()
        elif key == "timestep_embed.weight":
            out[key] = torch.randn(tuple(t.shape), generator=g, dtype=torch.float32)
        elif t.dim() == 1:
            out[key] = u(0.05) if key.endswith(".bias") else (1.0 if key.endswith("norm.weight") else NORM_GAIN) * (1.0 + u(0.2))
        else:
            gain = next((v for k, v in GAINS.items() if k in key), GAIN)
            out[key] = u(gain / math.sqrt(t.shape[1] * t.shape[2]))
    return out


def zeroed(sd, what):
    """The same state dict with one kind of branch silenced: "out_proj" (every attention) or "main.3" (every block's second convolution)"""
    return {k: (torch.zeros_like(v) if f".{what}." in k else v) for k, v in sd.items()}


def inputs(name):
    kw, b, t = CASES[name]
    x = synthetic.synth_input(f"unet_{name}_x", (b, kw["io_channels"], t), SEED)
    ts = torch.rand(b, generator=synthetic._gen(SEED, f"unet_{name}_t"), dtype=torch.float32)
    return x, ts


def load():
    return cases.load(STEM)


# ------------------------------------------------------------------------------------------------------------------ gates
# Measured by the generator on the reference alone (CPU) and copied here; tests/test_unet_host.py recomputes them from the stored tensors.
#   R16[case][fmt]  rel-L2 between the reference with every nn.Conv1d's input and weight rounded to fmt and the reference in fp32.  The GPU
#                   gate of (case, fmt) is TWICE this figure; every figure is below R16_LIMIT (the generator asserts it), no case is dropped.
#   F64[case]       rel-L2 between the reference in fp32 and in float64.  The fp32 gate is FOUR times this figure.
# Per output time step ([b, :, t], util.assert_close_sliced over dims (0, 2)) the gate is the whole-tensor gate times ROW_FACTOR = 8, the
# factor and the reasoning of local_attn_cases.py.
ROW_FACTOR = 8.0
R16_LIMIT = 2e-2          # == local_attn_cases.R16_LIMIT
R16 = {
    "A": {"fp16": 4.854e-04, "bf16": 5.200e-03},
    "B": {"fp16": 1.032e-03, "bf16": 9.387e-03},
    "C": {"fp16": 4.288e-04, "bf16": 5.639e-03},
}
F64 = {"A": 6.422e-07, "B": 1.082e-06, "C": 4.720e-07}


def gate(name, fmt):
    return 4.0 * F64[name] if fmt == "fp32" else 2.0 * R16[name][fmt]
