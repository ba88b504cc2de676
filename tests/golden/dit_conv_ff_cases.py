"""The convolutional feed-forward of the reduced DiT -- ff_kwargs use_conv (reference models/transformer.py:211-287) -- that
tests/golden/make_golden_dit_families.py (reference side) and tests/test_dit_conv_ff_host.py / tests/test_gpu_dit_conv_ff.py (product side)
share: configs, forward cases and the gain on the synthetic weights.  Weights and inputs come from (seed, name) through
``stable_audio_tools.synthetic`` (dit_family.py)."""
import torch

import cases
import dit_family
from stable_audio_tools import synthetic

PREPEND_DIM = dit_family.PREPEND_DIM
ADALN = dict(global_cond_type="adaLN")
CONV = {"use_conv": True}
# name -> the reference's DiffusionTransformer kwargs (the product's take both opt-ins on top: PRODUCT_KWARGS)
CONFIGS = {
    "conv": dict(cases.SMALL_DIT, ff_kwargs=dict(CONV)),                                                  # glu, k = 3: only FF-out is a convolution
    "conv_adaln": dict(cases.SMALL_DIT, ff_kwargs=dict(CONV), **ADALN),
    "conv_silu": dict(cases.SMALL_DIT, ff_kwargs=dict(CONV, glu=False)),                                  # both are convolutions
    "conv_silu_k5_nobias": dict(cases.SMALL_DIT, ff_kwargs=dict(CONV, glu=False, conv_kernel_size=5, no_bias=True)),
    "conv_mult2": dict(cases.SMALL_DIT, ff_kwargs=dict(CONV, mult=2)),
    "conv_prepend": dict(cases.SMALL_DIT, prepend_cond_dim=PREPEND_DIM, ff_kwargs=dict(CONV)),           # P = 3: the window crosses prepend, global and frame rows
    "conv_nonorm": dict(cases.SMALL_DIT, remove_norms=True, ff_kwargs=dict(CONV, glu=False)),
    "conv_all_adaln": dict(cases.SMALL_DIT, conformer=True, remove_norms=True, ff_kwargs=dict(CONV, glu=False), **ADALN),
}
PRODUCT_KWARGS = dict(allow_block_options=True, allow_conv_ff=True)

# synth_state_dict draws the Conv1d weights like every other transformer weight.  With it the off-centre taps of the feed-forward convolutions
# move the output of the glu=False configs (two convolutions per block) by 1.5e-1 - 2.1e-1 rel-L2, but that of the glu configs (FF-out only)
# by 1.9e-2 - 2.6e-2: under the 5e-2 the generator asks of every case, so that a kernel which reads only the centre row cannot pass.
# Generator and tests multiply the off-centre taps of ff.ff.2.weight of the glu configs by this gain after synth_state_dict, as
# dit_block_options_cases.GAINS does for the conformer: the smallest power of two with which the generator's assertion holds for every
# case (its output has the figures).  The glu=False configs keep the weights as drawn: they need no gain, and one would only raise the
# share of the feed-forward branch in the output's rounding noise above that of the models the reduced-DiT gates were set on.
OFF_CENTRE_GAIN = 4.0
# the conformer's gain of dit_block_options_cases.py, for conv_all_adaln
GAINS = {"conformer.pointwise_conv_2.weight": 4.0}


def is_ff_conv_weight(key, tensor):
    return tensor.dim() == 3 and (key.endswith(".ff.ff.2.weight") or key.endswith(".ff.ff.0.1.weight"))


def synth_weights(template_sd, seed=0):
    sd = dit_family.scaled(synthetic.synth_state_dict(template_sd, seed), dit_family.suffix_gain(GAINS))

    def off_centre(k, v):
        if k.endswith(".ff.ff.2.weight") and v.dim() == 3 and k[:-len("2.weight")] + "0.proj.weight" in sd:     # glu: FF-in is the Linear SwiGLU
            g = torch.full((v.shape[2],), OFF_CENTRE_GAIN)
            g[v.shape[2] // 2] = 1.0
            return g
    return dit_family.scaled(sd, off_centre)


def centre_taps_only(sd):
    """The same weights with every off-centre tap of every feed-forward convolution set to zero: what a kernel computes that reads only the
    row itself.  Every case must differ from this model by FAMILY.min_effect (make_golden_dit_families.py)."""
    out = dict(sd)
    for k, v in sd.items():
        if is_ff_conv_weight(k, v):
            keep = torch.zeros(v.shape[2])
            keep[v.shape[2] // 2] = 1.0
            out[k] = v * keep
    return out


# forward cases: name -> (config, t_len, prepend length P or None, cfg_scale).  Batch 2, 130 context tokens.  T = 77 on a "prepend" model
# is S = 78 rows per sequence: an M tail in every tile, and the second sequence starts mid-tile -- a window that leaks across sequences
# shows; T = 64 is S = 65
CASES = {}
for _c in CONFIGS:
    _p = 3 if _c == "conv_prepend" else None
    CASES[f"{_c}_cfg1_T64"] = (_c, 64, _p, 1.0)
    CASES[f"{_c}_cfg7_T77"] = (_c, 77, _p, 7.0)


FAMILY = dit_family.Family(
    title="dit conv ff", stem="dit_conv_ff_small", keys_file="dit_conv_ff_state_dict_keys.json", configs=CONFIGS, cases=CASES,
    product_kwargs=PRODUCT_KWARGS, weights=lambda cfg_name, template_sd, seed=0: synth_weights(template_sd, seed), r16=True,
    effect_of=f"the off-centre taps (OFF_CENTRE_GAIN {OFF_CENTRE_GAIN})",
    baseline=lambda cfg_name: ("the centre taps alone", CONFIGS[cfg_name], centre_taps_only))
