"""Cases of the local-attention codec family (``"type": "local_attn"``): configs, seeded weights and inputs, and the gate figures the
generator measured on the reference (tests/golden/make_golden_local_attn.py writes local_attn_small*.npz and
local_attn_state_dict_keys.json; tests/test_gpu_local_attn.py and tests/test_local_attn_host.py read them).

Stored: the REFERENCE's outputs (fp32), its outputs with the operands of every nn.Linear rounded to fp16 / bf16 (``<entry>__r16_<fmt>``, the
yardstick of the 16-bit gates) and its float64 outputs (``<entry>__f64``, the yardstick of the fp32 gate).  Weights and inputs are
regenerated from seeds; a decoder's input is the stored fp32 output of its encoder.

The cases sit at the seams of the plan (csrc/local_attn_plan.hip):
  A   embed_dims [128, 256], heads [4, 4] (32- and 64-channel heads: the staged route and the heads epilogue), depths [1, 2], ratios [2, 2],
      window 7, two input channels, batch 2, 1056 samples.  Stages at 1056 and 528 rows: four 256-query workgroups and a 32-row tail, and a
      batch seam the shifted windows must not cross.  264 latents; the mirrored decoder from them.
  B   embed_dims [128, 384], heads [1, 4] (128- and 96-channel heads), ratios [2, 4], window 65 (more than two 32-key blocks), one input
      channel, batch 1, 1040 samples; the mirrored decoder.  fp16 and bf16 only: there are no fp32 kernels at 128-channel heads (the DiT
      plan refuses that combination as well), and set_gemm_dtype("fp32") on it is one of the tested refusals.
  B32 B for the fp32 build, as the issue provides where a launcher's width limits rule a stage width out: the same structure with heads
      [2, 4], i.e. 64 in place of 128, the nearest width an embed_dim of 128 admits (96 does not divide it).  Runs in all three formats.
  C   the window equal to the sequence, a ratio that is no power of two: one stage, ratios [3], window 33, 33 samples, 11 latents, batch 2;
      the decoder's only stage runs at exactly 33 rows.  Depth 1: tests/test_local_attn_host.py restates this model in float64.
  D   a whole AudioAutoencoder from a config dict (create_autoencoder_from_config): local_attn on both sides, "vae" bottleneck with injected
      noise; encode_audio / decode_audio plain and chunked=True (chunk_size 32, overlap 4, 100 latents: four chunks), the chunked results
      against the reference's chunked results.
"""
import math
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import cases  # noqa: E402  (puts the package on sys.path)
from stable_audio_tools import synthetic  # noqa: E402

STEM = "local_attn_small"
KEYS_PATH = os.path.join(HERE, "local_attn_state_dict_keys.json")
SEED = 11
FORMATS = ("fp16", "bf16", "fp32")


def _codec(in_ch, latent, embed_dims, heads, depths, ratios, window, ff_mult=2):
    """(encoder kwargs, mirrored decoder kwargs)"""
    enc = dict(in_channels=in_ch, out_channels=latent, embed_dims=embed_dims, heads=heads, depths=depths, ratios=ratios,
               local_attn_window_size=window, ff_mult=ff_mult)
    dec = dict(in_channels=latent, out_channels=in_ch, embed_dims=embed_dims[::-1], heads=heads[::-1], depths=depths[::-1], ratios=ratios[::-1],
               local_attn_window_size=window, ff_mult=ff_mult)
    return enc, dec


# case -> (encoder kwargs, decoder kwargs, batch, samples, formats)
CODECS = {
    "A": _codec(2, 8, [128, 256], [4, 4], [1, 2], [2, 2], 7) + (2, 1056, FORMATS),
    "B": _codec(1, 6, [128, 384], [1, 4], [1, 1], [2, 4], 65) + (1, 1040, ("fp16", "bf16")),
    "B32": _codec(1, 6, [128, 384], [2, 4], [1, 1], [2, 4], 65) + (1, 1040, FORMATS),
    "C": _codec(2, 4, [128], [2], [1], [3], 33) + (2, 33, FORMATS),
}

D_ENC, D_DEC = _codec(2, 8, [128, 256], [2, 4], [1, 1], [2, 4], 9)
D_DEC["in_channels"] = 4          # the vae bottleneck halves the encoder's 8 channels
D_CONFIG = {
    "model_type": "autoencoder", "sample_rate": 16000,
    "model": {"encoder": {"type": "local_attn", "config": D_ENC}, "decoder": {"type": "local_attn", "config": D_DEC},
              "bottleneck": {"type": "vae"}, "latent_dim": 4, "downsampling_ratio": 8, "io_channels": 2},
}
D_BATCH, D_SAMPLES, D_CHUNK = 2, 800, dict(chunk_size=32, overlap=4, max_batch_size=1)
D_ENTRIES = ("D_encode", "D_decode", "D_encode_chunked", "D_decode_chunked")


def entries():
    """entry -> the formats it runs in; an entry is one golden tensor"""
    out = {}
    for name, (_, _, _, _, fmts) in CODECS.items():
        out[f"{name}_enc"] = fmts
        out[f"{name}_dec"] = fmts
    out.update({e: FORMATS for e in D_ENTRIES})
    return out


# ------------------------------------------------------------------------------------------------------------------ weights and inputs
# The reference zero-initialises to_out and ff.2, which would leave every layer the identity: every tensor is drawn, uniform in
# +-gain / sqrt(fan_in) -- gain sqrt(3) keeps the variance of a unit-variance input.  Stated gains: projections (project_in / _down / _up /
# _out) sqrt(3); to_qkv 1 (the logits are not scaled: with up to 128 channels per head they stay within a few units; at 1.5 the
# reference's own bf16 figure of A_enc was 2.9e-2, above R16_LIMIT); to_out and ff.2 sqrt(3), so that both branches
# move the stream (the generator asserts it); ff.0.proj sqrt(3), its bias +-0.05; LayerNorm gamma 1 +- 0.2, beta +-0.05.
GAINS = {"to_qkv": 1.0}


def weights(template_sd, seed=SEED):
    out = {}
    for key, t in template_sd.items():
        g = synthetic._gen(seed, key)
        leaf = key.rsplit(".", 1)[-1]
        u = lambda bound: (torch.rand(tuple(t.shape), generator=g, dtype=torch.float32) * 2 - 1) * bound
        if key.endswith("inv_freq"):
            out[key] = t.clone().float()
        elif leaf == "gamma":
            out[key] = 1.0 + u(0.2)
        elif leaf in ("beta", "bias"):
            out[key] = u(0.05)
        else:
            gain = next((v for k, v in GAINS.items() if k in key), math.sqrt(3.0))
            out[key] = u(gain / math.sqrt(t.shape[1]))
    return out


def zeroed_branches(sd):
    """The same state dict as the reference initialises its branches: to_out and ff.2 zero"""
    return {k: (torch.zeros_like(v) if k.endswith(("to_out.weight", "ff.2.weight")) else v) for k, v in sd.items()}


def audio(name):
    _, _, b, samples, _ = CODECS[name]
    return synthetic.synth_input(f"local_attn_{name}_audio", (b, CODECS[name][0]["in_channels"], samples), SEED, 0.5)


def d_audio():
    return synthetic.synth_input("local_attn_D_audio", (D_BATCH, 2, D_SAMPLES), SEED, 0.5)


def d_noise(shape):
    """The Gaussian of the vae bottleneck for a call of this shape (the chunked path draws it per chunk: the same tensor every time)"""
    return synthetic.synth_input("local_attn_D_noise", tuple(shape), SEED)


def load():
    return cases.load(STEM)


# ------------------------------------------------------------------------------------------------------------------ gates
# Measured by the generator on the reference alone (CPU) and copied here; tests/test_local_attn_host.py recomputes them from the stored tensors.
#   R16[entry][fmt]  rel-L2 between the reference with every nn.Linear's input and weight rounded to fmt and the reference in fp32.  The GPU
#                    gate of (entry, fmt) is TWICE this figure.  A pair runs only where the figure is finite and below 2e-2 (DROPPED lists
#                    the others by name: at most one of A-C in bf16, none in fp16).
#   F64[entry]       rel-L2 between the reference in fp32 and in float64.  The fp32 gate is FOUR times this figure.
# Per output row (one time step of one item, all channels; util.assert_close_sliced over dims (0, 2)) the gate is the whole-tensor gate times
# ROW_FACTOR.  Reasoning: were the error of every element an independent Gaussian of one variance, the worst of N rows of c channels would
# sit sqrt(chi2_c quantile (1 - 1/N) / c) above the whole figure: 3.7 for the 1040 one-channel rows of B_dec, 2.8 for the 2112 two-channel rows
# of A_dec, 2.1 for the 528 eight-channel rows of A_enc.  Rounding error is not uniform over rows (a row behind a sharp softmax moves more; a
# row of small norm is floored at the rms row norm by slice_errors): twice the largest of those, 8.  The generator asserts that the reference's
# own rounded-operand and float64 figures pass this row gate (their worst rows sit 1.7 - 6.1 times above their whole figures).  A row computed
# from the wrong keys, or from another item's rows across the batch seam, is off by its own norm: 1 against at most 8 * 2 * 2e-2 = 0.32.
ROW_FACTOR = 8.0
R16_LIMIT = 2e-2
R16 = {
    "A_enc": {"fp16": 2.112e-03, "bf16": 1.495e-02},
    "A_dec": {"fp16": 1.156e-03, "bf16": 8.694e-03},
    "B_enc": {"fp16": 1.192e-03, "bf16": 1.287e-02},
    "B_dec": {"fp16": 1.280e-03, "bf16": 1.031e-02},
    "B32_enc": {"fp16": 1.438e-03, "bf16": 9.280e-03},
    "B32_dec": {"fp16": 1.172e-03, "bf16": 9.440e-03},
    "C_enc": {"fp16": 1.036e-03, "bf16": 7.622e-03},
    "C_dec": {"fp16": 7.889e-04, "bf16": 7.464e-03},
    "D_encode": {"fp16": 1.187e-03, "bf16": 9.339e-03},
    "D_decode": {"fp16": 8.699e-04, "bf16": 6.895e-03},
    "D_encode_chunked": {"fp16": 1.214e-03, "bf16": 9.373e-03},
    "D_decode_chunked": {"fp16": 8.682e-04, "bf16": 6.890e-03},
}
F64 = {"A_enc": 5.179e-06, "A_dec": 1.653e-06, "B_enc": 1.815e-06, "B_dec": 2.727e-06, "B32_enc": 1.267e-06, "B32_dec": 1.807e-06, "C_enc": 6.073e-07,
       "C_dec": 6.378e-07, "D_encode": 1.750e-06, "D_decode": 1.020e-06, "D_encode_chunked": 9.216e-07, "D_decode_chunked": 7.485e-07}
DROPPED = []          # (entry, format) pairs at or above R16_LIMIT: none with these gains


def gate(entry, fmt):
    return 4.0 * F64[entry] if fmt == "fp32" else 2.0 * R16[entry][fmt]


def runs(entry, fmt):
    return fmt in entries()[entry] and (entry, fmt) not in DROPPED
