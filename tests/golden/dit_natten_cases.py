"""The reduced neighbourhood-attention DiTs (ContinuousTransformer attn_kwargs natten_kernel_size = K: query row i of the n rows
[prepend rows | global token | tokens] sees the K rows from min(max(i - K // 2, 0), n - K) on, logits unscaled) that
tests/golden/make_golden_dit_natten.py (reference side) and tests/test_dit_natten_host.py / tests/test_gpu_dit_natten.py (product side)
share: configs and forward cases, by the scheme of dit_causal_cases.py.  Weights come from (seed, name) through
``dit_options_cases.synth_weights`` with the conformer gain of dit_block_options_cases and the q / k gain below, inputs through
``stable_audio_tools.synthetic`` (dit_family.py).

Every config has cond_token_dim = 0: attn_kwargs reach the reference's cross_attn too, where NATTEN fails on q and k of different lengths.
The reference side runs with tests/golden/natten_standin.py in NATTEN's place."""
import cases
import dit_block_options_cases as BO
import dit_family
import dit_options_cases as OC

PREPEND_DIM, CONCAT_DIM = OC.PREPEND_DIM, OC.CONCAT_DIM


def natten(k, **attn):
    return dict(attn_kwargs=dict(natten_kernel_size=k, **attn), cond_token_dim=0)


def prepend(k, **attn):          # CFG needs cross-attention or prepend tokens (dit.py:270): here the tokens
    return dict(prepend_cond_dim=PREPEND_DIM, **natten(k, **attn))


# name -> the reference's DiffusionTransformer kwargs.  K = 69 is K == n at T = 64 with P = 4 (every query sees every key: full attention
# without the 1 / 8); the option configs run K = 33
CONFIGS = {f"k{k}": dict(cases.SMALL_DIT, **prepend(k)) for k in (7, 33, 129, 255, 69)}
CONFIGS.update({
    "qk": dict(cases.SMALL_DIT, **prepend(33, qk_norm=True)),
    "adaln": dict(cases.SMALL_DIT, global_cond_type="adaLN", **natten(33)),          # (adaLN takes no prepend tokens: CFG 1 only)
    "adaln_k65": dict(cases.SMALL_DIT, global_cond_type="adaLN", **natten(65)),          # K == n at T = 65: no prepend rows, no global token
    "norope_sin": dict(cases.SMALL_DIT, rotary_pos_emb=False, use_sinusoidal_emb=True, **prepend(33)),
    "concat": dict(cases.SMALL_DIT, input_concat_dim=CONCAT_DIM, **prepend(33)),
    "conf": dict(cases.SMALL_DIT, conformer=True, **prepend(33)),
    "patch2": dict(cases.SMALL_DIT, patch_size=2, **prepend(33)),          # the window counts tokens
})
KERNEL = {name: cfg["attn_kwargs"]["natten_kernel_size"] for name, cfg in CONFIGS.items()}


def without_natten(cfg):
    """The same model with full (scaled) attention: what the generator compares every case with."""
    return dict(cfg, attn_kwargs={k: v for k, v in cfg["attn_kwargs"].items() if k != "natten_kernel_size"})


# The reference does not scale the logits of this branch by dim_heads ** -0.5 = 1 / 8.  synth_state_dict's to_qkv gives the causal family a
# logit spread that is the synthetic weights' times 1 / 8; the q rows and the k rows of to_qkv.weight ([q | k | v] along dim 0) are each
# multiplied by 8 ** -0.5 here, so that q . k of this family IS q . k / 8 of that one: the same spread into the softmax, hence the same
# sensitivity of the output to 16-bit operands.  (With qk_norm the rows are normalised behind the projection and the gain drops out.)
QK_GAIN = 8.0 ** -0.5


def _gain(key, tensor):
    g = dit_family.suffix_gain(BO.GAINS)(key, tensor)
    if g is None and key.endswith("self_attn.to_qkv.weight"):
        import torch
        d = tensor.shape[0] // 3
        g = torch.cat([torch.full((2 * d, 1), QK_GAIN), torch.ones(d, 1)]).to(tensor.dtype)
    return g


def synth_weights(template_sd, seed=0):
    return dit_family.scaled(OC.synth_weights(template_sd, seed), _gain)


# forward cases: name -> (config, t_len, prepend length P or None, cfg_scale).  Batch 2, P = 4 prepend tokens.  CFG 7 is four sequences;
# S = 4 + 1 + 296 = 301 rows per sequence puts their keys at the shifts (b * S) & 3 = 0, 1, 2, 3, in five 64-key tiles under two 256-query
# workgroups per head; S = 645 is three workgroups, whose middle one walks neither the first nor the last tile at K = 129.  The patchified
# model reaches S = 301 with 592 frames
CASES = {
    "k7_cfg1_T64": ("k7", 64, 4, 1.0), "k7_cfg7_T296": ("k7", 296, 4, 7.0),
    "k33_cfg1_T64": ("k33", 64, 4, 1.0), "k33_cfg7_T296": ("k33", 296, 4, 7.0),
    "k129_cfg7_T296": ("k129", 296, 4, 7.0), "k129_cfg7_T640": ("k129", 640, 4, 7.0),
    "k255_cfg7_T296": ("k255", 296, 4, 7.0), "k255_cfg7_T640": ("k255", 640, 4, 7.0),
    "k69_cfg1_T64": ("k69", 64, 4, 1.0), "k69_cfg7_T64": ("k69", 64, 4, 7.0),
    "adaln_cfg1_T64": ("adaln", 64, None, 1.0), "adaln_cfg1_T301": ("adaln", 301, None, 1.0),
    "adaln_k65_cfg1_T65": ("adaln_k65", 65, None, 1.0),
    "patch2_cfg1_T128": ("patch2", 128, 4, 1.0), "patch2_cfg7_T592": ("patch2", 592, 4, 7.0),
}
for _c in ("qk", "norope_sin", "concat", "conf"):
    CASES[f"{_c}_cfg1_T64"] = (_c, 64, 4, 1.0)
    CASES[f"{_c}_cfg7_T296"] = (_c, 296, 4, 7.0)


FAMILY = dit_family.Family(
    title="dit natten", stem="dit_natten_small", keys_file="dit_natten_state_dict_keys.json", configs=CONFIGS, cases=CASES,
    weights=lambda cfg_name, template_sd, seed=0: synth_weights(template_sd, seed), concat=OC.FAMILY.concat, min_effect=5e-2,
    effect_of="the neighbourhood", r16=True,
    product_kwargs=dict(allow_natten=True, allow_patch_size=True, allow_block_options=True),
    baseline=lambda cfg_name: ("the same model with natten_kernel_size=None", without_natten(CONFIGS[cfg_name]), None))
