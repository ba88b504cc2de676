"""The reduced neighbourhood-attention DiTs with 128-, 32- and 96-channel heads (attn_kwargs natten_kernel_size = K behind allow_natten and
allow_natten_head_widths; csrc/attention_hdw_window.hip) that tests/golden/make_golden_dit_natten_hdw.py (reference side) and
tests/test_dit_natten_hdw_host.py / tests/test_gpu_dit_natten_hdw.py (product side) share: configs and forward cases, by the scheme of
dit_natten_cases.py.  Weights come from (seed, name) through ``dit_options_cases.synth_weights`` with the q / k gain below, inputs through
``stable_audio_tools.synthetic`` (dit_family.py).

Every config has cond_token_dim = 0 (attn_kwargs reach the reference's cross_attn too, where NATTEN fails).  The reference side runs with
tests/golden/natten_standin.py in NATTEN's place.  This family is not listed in dit_family.FAMILY_MODULES: the test files hand FAMILY to the
harness themselves."""
import cases
import dit_family
import dit_natten_cases as NC
import dit_options_cases as OC

PREPEND_DIM = OC.PREPEND_DIM
BASE = {128: dict(cases.SMALL_DIT, num_heads=2),                       # 256 / 2
        32: dict(cases.SMALL_DIT, num_heads=8),                        # 256 / 8
        96: dict(cases.SMALL_DIT, embed_dim=384, num_heads=4)}         # 384 / 4

# name -> the reference's DiffusionTransformer kwargs.  K = 7, 33 and 129 at every width, each with prepend tokens; the option configs run K = 33
CONFIGS = {f"hd{w}_k{k}": dict(BASE[w], **NC.prepend(k)) for w in (128, 32, 96) for k in (7, 33, 129)}
CONFIGS.update({
    "hd32_qk": dict(BASE[32], **NC.prepend(33, qk_norm=True)),
    "hd96_adaln": dict(BASE[96], global_cond_type="adaLN", **NC.natten(33)),          # (adaLN takes no prepend tokens: CFG 1 only)
    "hd128_patch2": dict(BASE[128], patch_size=2, **NC.prepend(33)),                  # the window counts tokens
    "hd32_k69": dict(BASE[32], **NC.prepend(69)),                                     # K == n at T = 64 with P = 4: every query sees every key
})
WIDTH = {name: cfg["embed_dim"] // cfg["num_heads"] for name, cfg in CONFIGS.items()}
KERNEL = {name: cfg["attn_kwargs"]["natten_kernel_size"] for name, cfg in CONFIGS.items()}
without_natten = NC.without_natten


# dit_natten_cases.QK_GAIN at every width: the reference does not scale the logits of this branch by W ** -0.5, so the q rows and the k rows
# of to_qkv.weight ([q | k | v] along dim 0) are each multiplied by W ** -0.25 -- q . k of this family is q . k / sqrt(W) of the scaled one,
# the same spread into the softmax.  (With qk_norm the rows are normalised behind the projection and the gain drops out.)
def qk_gain(width):
    return float(width) ** -0.25


def synth_weights(cfg_name, template_sd, seed=0):
    import torch
    g = qk_gain(WIDTH[cfg_name])

    def gain(key, tensor):
        if not key.endswith("self_attn.to_qkv.weight"):
            return None
        d = tensor.shape[0] // 3
        return torch.cat([torch.full((2 * d, 1), g), torch.ones(d, 1)]).to(tensor.dtype)

    return dit_family.scaled(OC.synth_weights(template_sd, seed), gain)


# forward cases: name -> (config, t_len, prepend length P or None, cfg_scale).  Batch 2, P = 4 prepend tokens.  CFG 7 is four sequences; S = 4
# + 1 + 296 = 301 rows per sequence puts their keys at the shifts (b * S) & 3 = 0, 1, 2, 3, in five 64-key tiles (three 128-key tiles at W =
# 32) under two 256-query workgroups per head; S = 645 is three workgroups, whose middle one walks neither the first nor the last tile at K =
# 129.  The patchified model reaches S = 301 with 592 frames
CANDIDATES = {}
for _w in (128, 32, 96):
    for _k in (7, 33, 129):
        # K = 129 does not fit the 69 rows of T = 64 (the reference raises): its CFG 1 case runs T = 124, 129 rows, K == n once more
        _t = 64 if _k <= 69 else 124
        CANDIDATES[f"hd{_w}_k{_k}_cfg1_T{_t}"] = (f"hd{_w}_k{_k}", _t, 4, 1.0)
        CANDIDATES[f"hd{_w}_k{_k}_cfg7_T296"] = (f"hd{_w}_k{_k}", 296, 4, 7.0)
CANDIDATES.update({
    "hd32_k129_cfg7_T640": ("hd32_k129", 640, 4, 7.0), "hd128_k129_cfg7_T640": ("hd128_k129", 640, 4, 7.0),
    "hd32_qk_cfg1_T64": ("hd32_qk", 64, 4, 1.0), "hd32_qk_cfg7_T296": ("hd32_qk", 296, 4, 7.0),
    "hd96_adaln_cfg1_T64": ("hd96_adaln", 64, None, 1.0), "hd96_adaln_cfg1_T301": ("hd96_adaln", 301, None, 1.0),
    "hd128_patch2_cfg1_T128": ("hd128_patch2", 128, 4, 1.0), "hd128_patch2_cfg7_T592": ("hd128_patch2", 592, 4, 7.0),
    "hd32_k69_cfg1_T64": ("hd32_k69", 64, 4, 1.0), "hd32_k69_cfg7_T64": ("hd32_k69", 64, 4, 7.0), "hd32_k69_cfg7_T296": ("hd32_k69", 296, 4, 7.0),
})

# What the generator measured and left out, {format: {case: the reference's own figure with operands rounded to that format}}: a case is
# run in a format only where that figure is below the harness gate of the format (dit_family_gpu.Harness.gate), so that the reference alone
# passes.  make_golden_dit_natten_hdw.py asserts that this table is what it measures; profiles/dit_natten_hdw_verification.txt has every figure
DROPPED = {
    "fp16": {},
    # every CFG 1 case (3.6e-3 - 4.6e-3 against the gate 2.5e-3, as the rounded reference of the 64-channel family), K = 129 at S = 301 and
    # K == n at CFG 7 (gate 1.2e-2)
    "bf16": {"hd128_k7_cfg1_T64": 0.00436, "hd128_k33_cfg1_T64": 0.00389, "hd128_k129_cfg1_T124": 0.0036, "hd128_k129_cfg7_T296": 0.0133,
             "hd32_k7_cfg1_T64": 0.00438, "hd32_k33_cfg1_T64": 0.0039, "hd32_k129_cfg1_T124": 0.00363, "hd32_k129_cfg7_T296": 0.0132,
             "hd96_k7_cfg1_T64": 0.00456, "hd96_k33_cfg1_T64": 0.00392, "hd96_k129_cfg1_T124": 0.00379, "hd96_k129_cfg7_T296": 0.0134,
             "hd32_qk_cfg1_T64": 0.00386, "hd96_adaln_cfg1_T64": 0.0038, "hd96_adaln_cfg1_T301": 0.00374, "hd128_patch2_cfg1_T128": 0.00394,
             "hd32_k69_cfg1_T64": 0.00382, "hd32_k69_cfg7_T64": 0.0177},
}
# the cases the goldens hold: every candidate that runs in at least one format
CASES = {n: c for n, c in CANDIDATES.items() if not all(n in d for d in DROPPED.values())}


def cases_of(gemm_dtype):
    """The names of the cases that run in the operand format `gemm_dtype` ("fp16" | "bf16"); the fp32 verification mode runs all of CASES."""
    return [n for n in CASES if n not in DROPPED.get(gemm_dtype, {})]


FAMILY = dit_family.Family(
    title="dit natten hdw", stem="dit_natten_hdw_small", keys_file="dit_natten_hdw_state_dict_keys.json", configs=CONFIGS, cases=CASES,
    weights=synth_weights, min_effect=5e-2, effect_of="the neighbourhood", r16=True,
    product_kwargs=dict(allow_natten=True, allow_natten_head_widths=True, allow_head_widths=True, allow_patch_size=True),
    baseline=lambda cfg_name: ("the same model with natten_kernel_size=None", without_natten(CONFIGS[cfg_name]), None))
