"""The reduced causal DiTs (ContinuousTransformer causal=True: query row i of the sequence [prepend rows | global token | tokens] sees the
rows j <= i) that tests/golden/make_golden_dit_causal.py (reference side) and tests/test_dit_causal_host.py / tests/test_gpu_dit_causal.py
(product side) share: configs and forward cases, by the scheme of dit_head_width_cases.py.  Weights come from (seed, name) through
``dit_options_cases.synth_weights`` with the conformer gain of dit_block_options_cases, inputs through ``stable_audio_tools.synthetic``
(dit_family.py).

Every config has cond_token_dim = 0: the reference has no working causal cross-attention (its mask helper is missing on the module with
more context keys than queries, and its attention backends place the mask differently with fewer)."""
import cases
import dit_block_options_cases as BO
import dit_family
import dit_head_dim_cases as HC
import dit_head_width_cases as WC
import dit_options_cases as OC

PREPEND_DIM, CONCAT_DIM = OC.PREPEND_DIM, OC.CONCAT_DIM
CAUSAL = dict(causal=True, cond_token_dim=0)
PREPEND = dict(prepend_cond_dim=PREPEND_DIM, **CAUSAL)          # CFG needs cross-attention or prepend tokens (dit.py:270): here the tokens
# name -> the reference's DiffusionTransformer kwargs
CONFIGS = {
    "plain": dict(cases.SMALL_DIT, **PREPEND),          # 64-channel heads, prepend-only
    "qk": dict(cases.SMALL_DIT, **PREPEND, **OC.QK),
    "adaln": dict(cases.SMALL_DIT, global_cond_type="adaLN", **CAUSAL),          # (adaLN takes no prepend tokens: CFG 1 only)
    "norope_sin": dict(cases.SMALL_DIT, rotary_pos_emb=False, use_sinusoidal_emb=True, **PREPEND),
    "concat": dict(cases.SMALL_DIT, input_concat_dim=CONCAT_DIM, **PREPEND),
    "conf": dict(cases.SMALL_DIT, conformer=True, **PREPEND),          # the conformer's convolution stays non-causal, as in the reference
    "hd128": dict(HC.HD128, **PREPEND),
    "hd32": dict(WC.HD32, **PREPEND),
    "hd96": dict(WC.HD96, **PREPEND),
    "hd32_patch2": dict(WC.HD32, patch_size=2, **PREPEND),
}
WIDTH = {name: cfg["embed_dim"] // cfg["num_heads"] for name, cfg in CONFIGS.items()}


def without_causal(cfg):
    """The same model with full attention: what the generator compares every case with."""
    return dict(cfg, causal=False)


def synth_weights(template_sd, seed=0):
    return dit_family.scaled(OC.synth_weights(template_sd, seed), dit_family.suffix_gain(BO.GAINS))


# forward cases: name -> (config, t_len, prepend length P or None, cfg_scale).  Batch 2, P = 4 prepend tokens.  CFG 7 is four sequences;
# S = 4 + 1 + 296 = 301 rows per sequence puts their keys at the shifts (b * S) & 3 = 0, 1, 2, 3, in five 64-key tiles (three of 128) under
# two (256-query) or three (128-query) workgroups per head; S = 645 > 512 sends the 64-channel launcher to its two-group layout.  The
# patchified model reaches S = 301 with 592 frames
CASES = {}
for _c in CONFIGS:
    if _c == "adaln":
        CASES["adaln_cfg1_T64"] = ("adaln", 64, None, 1.0)
        CASES["adaln_cfg1_T301"] = ("adaln", 301, None, 1.0)
        continue
    _t = 592 if CONFIGS[_c].get("patch_size", 1) == 2 else 296
    CASES[f"{_c}_cfg1_T64"] = (_c, 64, 4, 1.0)
    CASES[f"{_c}_cfg7_T{_t}"] = (_c, _t, 4, 7.0)
CASES["plain_cfg7_T640"] = ("plain", 640, 4, 7.0)


FAMILY = dit_family.Family(
    title="dit causal", stem="dit_causal_small", keys_file="dit_causal_state_dict_keys.json", configs=CONFIGS, cases=CASES,
    weights=lambda cfg_name, template_sd, seed=0: synth_weights(template_sd, seed), concat=OC.FAMILY.concat, min_effect=5e-2,
    effect_of="the causal mask", r16=True,
    product_kwargs=dict(allow_causal=True, allow_head_widths=True, allow_patch_size=True, allow_block_options=True),
    baseline=lambda cfg_name: ("the same model with causal=False", without_causal(CONFIGS[cfg_name]), None))
