"""The reduced DiT with 128-channel attention heads (embed_dim == 128 * num_heads) that tests/golden/make_golden_dit_families.py
(reference side) and tests/test_dit_head_dim_host.py / tests/test_gpu_dit_head_dim.py (product side) share: configs and forward cases.
Weights come from (seed, name) through ``dit_options_cases.synth_weights``, inputs through ``stable_audio_tools.synthetic`` (dit_family.py)."""
import cases
import dit_family
import dit_options_cases as OC

PREPEND_DIM, CONCAT_DIM = OC.PREPEND_DIM, OC.CONCAT_DIM
HD128 = dict(cases.SMALL_DIT, num_heads=2)          # 256 / 2: two heads of 128, one kv head (cond_embed_dim 128)
# name -> DiffusionTransformer kwargs
CONFIGS = {
    "hd128": dict(HD128),
    "hd128_qk": dict(HD128, **OC.QK),
    "hd128_adaln": dict(HD128, global_cond_type="adaLN"),
    "hd128_wide": dict(cases.SMALL_DIT, embed_dim=512, num_heads=4, cond_token_dim=256),          # two kv heads, GQA 2:1: the kv-head index is not constant
    "hd128_prepend_only": dict(HD128, cond_token_dim=0, prepend_cond_dim=PREPEND_DIM),
    "hd128_norope": dict(HD128, rotary_pos_emb=False, use_sinusoidal_emb=True),
}
BASIC = tuple(CONFIGS)          # every one of these runs at (CFG 1, T 64) and (CFG 7, T 77)
CONFIGS["hd128_qk_concat"] = dict(HD128, input_concat_dim=CONCAT_DIM, **OC.QK)

synth_weights = OC.synth_weights


def with_64_channel_heads(cfg):
    """The same model with twice the heads of half the width: what the generator compares every case with."""
    return dict(cfg, num_heads=cfg["embed_dim"] // 64)


# forward cases: name -> (config, t_len, prepend length P or None, cfg_scale).  Batch 2, 130 context tokens (130 + 3 keys: three key tiles).
# T = 77 on a "prepend" model is S = 78 rows per sequence: an M tail in every tile and the key shift (b * S) & 3 = 2 of the second sequence
CASES = {}
for _c in BASIC:
    _p = 4 if _c == "hd128_prepend_only" else None         # CFG needs cross-attention or prepend tokens (dit.py:270)
    CASES[f"{_c}_cfg1_T64"] = (_c, 64, _p, 1.0)
    CASES[f"{_c}_cfg7_T77"] = (_c, 77, _p, 7.0)
CASES["hd128_qk_concat_cfg7_T77"] = ("hd128_qk_concat", 77, None, 7.0)


# 3e-2, not the 5e-2 of the other families: what halving the head width moves the least case by
FAMILY = dit_family.Family(
    title="dit head dim", stem="dit_head_dim_small", keys_file="dit_head_dim_state_dict_keys.json", configs=CONFIGS, cases=CASES,
    weights=OC.FAMILY.weights, concat=OC.FAMILY.concat, min_effect=3e-2, effect_of="the head width",
    baseline=lambda cfg_name: ("the model with 64-channel heads", with_64_channel_heads(CONFIGS[cfg_name]), None))
