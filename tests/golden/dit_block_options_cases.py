"""The TransformerBlock options of the reduced DiT -- conformer, remove_norms, ff_kwargs glu=False (reference models/transformer.py:557-591,
621-645, 259-268) -- that tests/golden/make_golden_dit_families.py (reference side) and tests/test_dit_block_options_host.py /
tests/test_gpu_dit_block_options.py (product side) share: configs, forward cases and the gains on the synthetic weights.  Weights
and inputs come from (seed, name) through ``stable_audio_tools.synthetic`` (dit_family.py)."""
import cases
import dit_family
from stable_audio_tools import synthetic

PREPEND_DIM = dit_family.PREPEND_DIM
CONF, NONORM, SILU = dict(conformer=True), dict(remove_norms=True), dict(ff_kwargs={"glu": False})
ADALN = dict(global_cond_type="adaLN")
# name -> the reference's DiffusionTransformer kwargs (the product's take allow_block_options=True on top: PRODUCT_KWARGS)
CONFIGS = {
    "conf": dict(cases.SMALL_DIT, **CONF),
    "conf_adaln": dict(cases.SMALL_DIT, **CONF, **ADALN),
    "nonorm": dict(cases.SMALL_DIT, **NONORM),
    "nonorm_adaln": dict(cases.SMALL_DIT, **NONORM, **ADALN),
    "silu": dict(cases.SMALL_DIT, **SILU),
    "silu_nobias": dict(cases.SMALL_DIT, ff_kwargs={"glu": False, "no_bias": True}),
    "all3": dict(cases.SMALL_DIT, **CONF, **NONORM, **SILU),
    "all3_adaln": dict(cases.SMALL_DIT, **CONF, **NONORM, **SILU, **ADALN),
    "conf_prepend": dict(cases.SMALL_DIT, prepend_cond_dim=PREPEND_DIM, **CONF),      # P = 3: the conv window crosses prepend, global and frame rows
    "conf_qk": dict(cases.SMALL_DIT, attn_kwargs={"qk_norm": True}, **CONF),
    "silu_mult2": dict(cases.SMALL_DIT, ff_kwargs={"glu": False, "mult": 2}),
}
PRODUCT_KWARGS = dict(allow_block_options=True)
# what the generator compares every case with: the same model without the option(s).  ff_kwargs loses its "glu" only
OPTION_KEYS = ("conformer", "remove_norms")


def without_options(cfg):
    out = {k: v for k, v in cfg.items() if k not in OPTION_KEYS}
    if "ff_kwargs" in out:
        out["ff_kwargs"] = {k: v for k, v in out["ff_kwargs"].items() if k != "glu"}
    return out


# synth_state_dict draws the conformer's weights like every other transformer weight, which leaves its branch at 4.5e-2 rel-L2 of the output
# (conf at CFG 1), under the 5e-2 the generator asks of every case so that a kernel which skips the branch cannot pass.  Generator and tests
# multiply the branch's output projection by this gain after synth_state_dict, as POS_EMB_GAIN does for the position embeddings; the other
# two options move the output by far more than that without help.
GAINS = {"conformer.pointwise_conv_2.weight": 4.0}


def synth_weights(template_sd, seed=0):
    return dit_family.scaled(synthetic.synth_state_dict(template_sd, seed), dit_family.suffix_gain(GAINS))


# forward cases: name -> (config, t_len, prepend length P or None, cfg_scale).  Batch 2, 130 context tokens.  T = 77 on a "prepend" model
# is S = 78 rows per sequence: an M tail in every tile, and the second sequence starts mid-tile -- a conv window that leaks across
# sequences shows; T = 64 is S = 65
CASES = {}
for _c in CONFIGS:
    _p = 3 if _c == "conf_prepend" else None
    CASES[f"{_c}_cfg1_T64"] = (_c, 64, _p, 1.0)
    CASES[f"{_c}_cfg7_T77"] = (_c, 77, _p, 7.0)


FAMILY = dit_family.Family(
    title="dit block options", stem="dit_block_options_small", keys_file="dit_block_options_state_dict_keys.json", configs=CONFIGS, cases=CASES,
    product_kwargs=PRODUCT_KWARGS, weights=lambda cfg_name, template_sd, seed=0: synth_weights(template_sd, seed), r16=True,
    baseline=lambda cfg_name: ("the model without the option", without_options(CONFIGS[cfg_name]), None))
