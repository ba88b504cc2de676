"""The ContinuousTransformer options of the reduced DiT that tests/golden/make_golden_dit_families.py (reference side) and
tests/test_dit_options_host.py / tests/test_gpu_dit_options.py (product side) share: configs, forward cases and the gain on the
position-embedding tensors.  Weights and inputs come from (seed, name) through ``stable_audio_tools.synthetic`` (dit_family.py)."""
import cases
import dit_family
from stable_audio_tools import synthetic

PREPEND_DIM, CONCAT_DIM = dit_family.PREPEND_DIM, 65
QK = {"attn_kwargs": {"qk_norm": True}}
ABS = dict(use_abs_pos_emb=True, abs_pos_emb_max_length=256, prepend_cond_dim=PREPEND_DIM)      # (prepend_cond_dim: one case brings 3 prepend tokens)
# name -> DiffusionTransformer kwargs
CONFIGS = {
    "qk": dict(cases.SMALL_DIT, **QK),
    "qk_adaln": dict(cases.SMALL_DIT, global_cond_type="adaLN", **QK),
    "qk_prepend_only": dict(cases.SMALL_DIT, cond_token_dim=0, prepend_cond_dim=PREPEND_DIM, **QK),
    "sin": dict(cases.SMALL_DIT, use_sinusoidal_emb=True),
    "abs": dict(cases.SMALL_DIT, **ABS),
    "abs_norope": dict(cases.SMALL_DIT, rotary_pos_emb=False, **ABS),
    "nobias": dict(cases.SMALL_DIT, ff_kwargs={"no_bias": True}),
    "all": dict(cases.SMALL_DIT, use_sinusoidal_emb=True, ff_kwargs={"no_bias": True}, **QK),
}
BASIC = tuple(CONFIGS)          # every one of these runs at (CFG 1, T 64) and (CFG 7, T 77)
# one case each: qk_norm behind the input-concat projection, the sinusoidal table under prepended rows, a feed-forward of another width
CONFIGS.update({
    "qk_concat": dict(cases.SMALL_DIT, input_concat_dim=CONCAT_DIM, **QK),
    "sin_prepend": dict(cases.SMALL_DIT, use_sinusoidal_emb=True, prepend_cond_dim=PREPEND_DIM),
    "mult2": dict(cases.SMALL_DIT, ff_kwargs={"mult": 2, "no_bias": True}),
})
# what the generator compares every case with: the same model without the option(s)
OPTION_KEYS = ("attn_kwargs", "ff_kwargs", "use_sinusoidal_emb", "use_abs_pos_emb", "abs_pos_emb_max_length", "rotary_pos_emb")

# synth_state_dict draws transformer.pos_emb.scale from +-0.05 and emb.weight from +-0.03 (times D^-0.5 in the model): the embedding would
# move the output by 3e-3 .. 8e-3 rel-L2, the size of the 16-bit gates.  Both generator and tests multiply the transformer.pos_emb.*
# tensors by this factor after synth_state_dict, which puts every case >= 5e-2 away from the model without the option.
POS_EMB_GAIN = 40.0


def synth_weights(template_sd, seed=0):
    return dit_family.scaled(synthetic.synth_state_dict(template_sd, seed), lambda k, v: POS_EMB_GAIN if k.startswith("transformer.pos_emb.") else None)


def without_options(cfg):
    return {k: v for k, v in cfg.items() if k not in OPTION_KEYS}


# forward cases: name -> (config, t_len, prepend length P or None, cfg_scale).  Batch 2, 130 context tokens.  T = 77 on a "prepend" model is
# S = 78 rows per sequence: an M tail in every tile and the key shift (b * S) & 3 = 2 of the second sequence; T = 64 is S = 65.
CASES = {}
for _c in BASIC:
    _p = 4 if _c == "qk_prepend_only" else None         # CFG needs cross-attention or prepend tokens (dit.py:270)
    CASES[f"{_c}_cfg1_T64"] = (_c, 64, _p, 1.0)
    CASES[f"{_c}_cfg7_T77"] = (_c, 77, _p, 7.0)
CASES["qk_cfg1_T77"] = ("qk", 77, None, 1.0)
CASES["abs_P3_cfg1_T77"] = ("abs", 77, 3, 1.0)           # position 0 is the first prepended row, latent frame t sits at P + 1 + t
CASES["abs_norope_P3_cfg7_T64"] = ("abs_norope", 64, 3, 7.0)
CASES["qk_concat_cfg7_T77"] = ("qk_concat", 77, None, 7.0)
CASES["sin_prepend_P3_cfg7_T77"] = ("sin_prepend", 77, 3, 7.0)
CASES["mult2_cfg1_T77"] = ("mult2", 77, None, 1.0)


# the concat tensor has the latent's length, seed 200 + T
FAMILY = dit_family.Family(
    title="dit options", stem="dit_options_small", keys_file="dit_options_state_dict_keys.json", configs=CONFIGS, cases=CASES,
    weights=lambda cfg_name, template_sd, seed=0: synth_weights(template_sd, seed), concat=lambda t_len: ((CONCAT_DIM, t_len), 200 + t_len),
    baseline=lambda cfg_name: ("the model without the option", without_options(CONFIGS[cfg_name]), None))
