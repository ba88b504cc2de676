"""The reduced DiTs with 32- and 96-channel attention heads (embed_dim == 32 or 96 times num_heads) that
tests/golden/make_golden_dit_head_width.py (reference side) and tests/test_dit_head_width_host.py / tests/test_gpu_dit_head_width.py (product
side) share: configs and forward cases, by the scheme of dit_head_dim_cases.py.  Weights come from (seed, name) through
``dit_options_cases.synth_weights``, inputs through ``stable_audio_tools.synthetic`` (dit_family.py)."""
import cases
import dit_family
import dit_options_cases as OC

PREPEND_DIM, CONCAT_DIM = OC.PREPEND_DIM, OC.CONCAT_DIM
HD32 = dict(cases.SMALL_DIT, num_heads=8)                                              # 256 / 8: 8 query heads, 4 kv heads (cond_embed_dim 128), GQA 2:1
HD96 = dict(cases.SMALL_DIT, embed_dim=384, num_heads=4, cond_token_dim=192)           # 384 / 4: 4 query heads, 2 kv heads
# name -> DiffusionTransformer kwargs
CONFIGS = {}
for _w, _base, _mha in (("hd32", HD32, 256), ("hd96", HD96, 384)):
    CONFIGS.update({
        _w: dict(_base),
        f"{_w}_qk": dict(_base, **OC.QK),
        f"{_w}_mha": dict(_base, cond_token_dim=_mha),          # as many kv heads as query heads
        f"{_w}_adaln": dict(_base, global_cond_type="adaLN"),
        f"{_w}_prepend_only": dict(_base, cond_token_dim=0, prepend_cond_dim=PREPEND_DIM),
        f"{_w}_norope": dict(_base, rotary_pos_emb=False, use_sinusoidal_emb=True),
    })
BASIC = tuple(CONFIGS)          # every one of these runs at (CFG 1, T 64) and (CFG 7, T 77)
CONFIGS["hd96_qk_concat"] = dict(HD96, input_concat_dim=CONCAT_DIM, **OC.QK)
CONFIGS["hd32_patch2"] = dict(HD32, patch_size=2)          # the patch kernels sit outside the blocks: the widths combine with them
WIDTH = {name: cfg["embed_dim"] // cfg["num_heads"] for name, cfg in CONFIGS.items()}


def with_64_channel_heads(cfg):
    """The same model with heads of 64 channels: what the generator compares every case with."""
    return dict(cfg, num_heads=cfg["embed_dim"] // 64)


# forward cases: name -> (config, t_len, prepend length P or None, cfg_scale).  Batch 2, 130 context tokens (130 + 3 keys: three 64-key tiles,
# two 128-key tiles).  T = 77 on a "prepend" model is S = 78 rows per sequence: the key shift (b * S) & 3 = 2 of the second sequence
CASES = {}
for _c in BASIC:
    _p = 4 if _c.endswith("prepend_only") else None         # CFG needs cross-attention or prepend tokens (dit.py:270)
    CASES[f"{_c}_cfg1_T64"] = (_c, 64, _p, 1.0)
    CASES[f"{_c}_cfg7_T77"] = (_c, 77, _p, 7.0)
CASES["hd96_qk_concat_cfg7_T77"] = ("hd96_qk_concat", 77, None, 7.0)
CASES["hd32_patch2_cfg7_T78"] = ("hd32_patch2", 78, None, 7.0)          # 39 tokens + the global token


FAMILY = dit_family.Family(
    title="dit head width", stem="dit_head_width_small", keys_file="dit_head_width_state_dict_keys.json", configs=CONFIGS, cases=CASES,
    weights=OC.FAMILY.weights, concat=OC.FAMILY.concat, min_effect=3e-2, effect_of="the head width", r16=True,
    product_kwargs=dict(allow_head_widths=True, allow_patch_size=True),
    baseline=lambda cfg_name: ("the model with 64-channel heads", with_64_channel_heads(CONFIGS[cfg_name]), None))
