"""The patchified reduced DiT -- DiffusionTransformer patch_size > 1 (reference models/dit.py:38,88-89,119-120,168-173,197-224) -- that
tests/golden/make_golden_dit_families.py (reference side) and tests/test_dit_patch_host.py / tests/test_gpu_dit_patch.py (product side) share:
configs, forward cases, and the mistakes every case must be able to tell from the model.  Weights and inputs come from
(seed, name) through ``stable_audio_tools.synthetic`` (dit_family.py); synth_state_dict draws non-zero preprocess / postprocess convs."""
import torch

import cases
import dit_family
from stable_audio_tools import synthetic

PREPEND_DIM = dit_family.PREPEND_DIM
CONCAT_DIM = 8
# name -> the reference's DiffusionTransformer kwargs (the product's take the opt-ins on top: PRODUCT_KWARGS)
CONFIGS = {
    "p2": dict(cases.SMALL_DIT, patch_size=2),
    "p4": dict(cases.SMALL_DIT, patch_size=4),                                      # C P = 256: four output column groups
    "p3": dict(cases.SMALL_DIT, patch_size=3),                                      # P no power of two, 192 columns
    "p8_c8": dict(cases.SMALL_DIT, patch_size=8, io_channels=8),                    # one column group
    "p2_adaln": dict(cases.SMALL_DIT, patch_size=2, global_cond_type="adaLN"),
    "p2_prepend": dict(cases.SMALL_DIT, patch_size=2, prepend_cond_dim=PREPEND_DIM),
    "p2_concat": dict(cases.SMALL_DIT, patch_size=2, input_concat_dim=CONCAT_DIM),
    "p2_hd128": dict(cases.SMALL_DIT, patch_size=2, num_heads=2),
    # with the block options and the convolutional feed-forward of the other opt-ins (weights: dit_conv_ff_cases.synth_weights)
    "p2_conformer_conv": dict(cases.SMALL_DIT, patch_size=2, conformer=True, ff_kwargs={"use_conv": True}),
}
PRODUCT_KWARGS = dict(allow_block_options=True, allow_conv_ff=True, allow_patch_size=True)

# forward cases: name -> (config, t_len in latent frames, prepend length or None, cfg_scale).  Batch 2, 130 context tokens.
# T = 78 at P = 2 on a "prepend" model is S = 40 rows per sequence: a token tail in both boundary kernels (39 = 4 * 8 + 7) and the second
# sequence starts mid-tile; T = 64 is S = 33
CASES = {
    "p2_cfg1_T64": ("p2", 64, None, 1.0),
    "p2_cfg7_T78": ("p2", 78, None, 7.0),
    "p4_cfg7_T76": ("p4", 76, None, 7.0),               # 19 tokens
    "p3_cfg1_T63": ("p3", 63, None, 1.0),
    "p8_c8_cfg7_T72": ("p8_c8", 72, None, 7.0),         # 9 tokens
    "p2_adaln_cfg7_T78": ("p2_adaln", 78, None, 7.0),
    "p2_prepend_cfg7_T78": ("p2_prepend", 78, 3, 7.0),
    "p2_concat_cfg7_T78": ("p2_concat", 78, None, 7.0), # concat length T // 3 = 26: resized to 78 frames before the patchify
    "p2_hd128_cfg7_T78": ("p2_hd128", 78, None, 7.0),
    "p2_conformer_conv_cfg7_T78": ("p2_conformer_conv", 78, None, 7.0),
}


def synth_weights(cfg_name, template_sd, seed=0):
    if cfg_name == "p2_conformer_conv":
        import dit_conv_ff_cases as CC
        return CC.synth_weights(template_sd, seed)
    return synthetic.synth_state_dict(template_sd, seed)


# ---- the mistakes a boundary kernel can make, as state dicts: a model with these weights computes what the mistaken kernel would
def _cols(w, P, f):
    """project_in.weight [D, Ci P] seen as [D, Ci, P], through f, back."""
    d, k = w.shape
    return f(w.reshape(d, k // P, P)).reshape(d, k).contiguous()


def _rows(w, P, f):
    """project_out.weight [C P, D] seen as [C, P, D], through f, back."""
    n, d = w.shape
    return f(w.reshape(n // P, P, d)).reshape(n, d).contiguous()


def in_columns_pc(sd, P):
    """project_in columns read as (p c): column c P + p takes the weight the reference keeps at p Ci + c."""
    out = dict(sd)
    w = sd["transformer.project_in.weight"]
    d, k = w.shape
    out["transformer.project_in.weight"] = w.reshape(d, P, k // P).transpose(1, 2).reshape(d, k).contiguous()
    return out


def out_rows_pc(sd, P):
    """project_out rows read as (p c)."""
    out = dict(sd)
    w = sd["transformer.project_out.weight"]
    n, d = w.shape
    out["transformer.project_out.weight"] = w.reshape(P, n // P, d).transpose(0, 1).reshape(n, d).contiguous()
    return out


def frames_reversed(sd, P):
    """Frame P - 1 - p where p belongs, inside every patch, at the input."""
    out = dict(sd)
    out["transformer.project_in.weight"] = _cols(sd["transformer.project_in.weight"], P, lambda w: w.flip(2))
    return out


def frames_reversed_out(sd, P):
    """... and at the output."""
    out = dict(sd)
    out["transformer.project_out.weight"] = _rows(sd["transformer.project_out.weight"], P, lambda w: w.flip(1))
    return out


def convs_dropped(sd, P):
    """Both 1x1 convs dropped: x + 0, out + 0."""
    out = dict(sd)
    for k in ("preprocess_conv.weight", "postprocess_conv.weight"):
        out[k] = torch.zeros_like(sd[k])
    return out


MISTAKES = {"project_in columns as (p c)": in_columns_pc, "project_out rows as (p c)": out_rows_pc, "frames reversed inside a patch (input)": frames_reversed,
            "frames reversed inside a patch (output)": frames_reversed_out, "both 1x1 convs dropped": convs_dropped}

# the concat tensor has a third of the latent's length (the model resizes it), seed 400
FAMILY = dit_family.Family(
    title="dit patch", stem="dit_patch_small", keys_file="dit_patch_state_dict_keys.json", configs=CONFIGS, cases=CASES,
    product_kwargs=PRODUCT_KWARGS, weights=synth_weights, concat=lambda t_len: ((CONCAT_DIM, t_len // 3), 400), mistakes=MISTAKES, r16=True)
