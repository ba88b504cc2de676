"""What the DiT option families (dit_*_cases.py) have in common: the record that describes a family, the builder of a case's inputs and the
gain step of the synthetic weights.  make_golden_dit_families.py (reference side) and tests/dit_family_gpu.py, tests/dit_family_host.py
(product side) both import it, so it does not import the reference.

A new family is a dit_<name>_cases.py that exports one FAMILY, a line in FAMILY_MODULES below, and test files that hand the FAMILY to
``dit_family_gpu.Harness`` / ``dit_family_host``."""
import importlib
import os
from dataclasses import dataclass, field
from typing import Callable, Optional

import torch

import cases
from stable_audio_tools import synthetic

PREPEND_DIM = 48          # prepend_cond_dim of every config that takes prepend tokens
FAMILY_MODULES = {"options": "dit_options_cases", "head_dim": "dit_head_dim_cases", "block_options": "dit_block_options_cases",
                  "conv_ff": "dit_conv_ff_cases", "patch": "dit_patch_cases"}


@dataclass(frozen=True)
class Family:
    title: str                      # what the tests print in front of a case: "dit conv ff"
    stem: str                       # tests/golden/<stem>.npz or <stem>.part*.npz
    keys_file: str                  # tests/golden/<keys_file>: {config: {state-dict key: shape}} of the reference's modules
    configs: dict                   # name -> the reference's DiffusionTransformer kwargs
    cases: dict                     # name -> (config, t_len, prepend length P or None, cfg_scale)
    weights: Callable               # (cfg_name, template state dict, seed) -> state dict
    product_kwargs: dict = field(default_factory=dict)          # the opt-ins the product's constructor takes on top of a config
    concat: Optional[Callable] = None          # t_len -> ((channels, length), seed) of input_concat_cond, for the configs with input_concat_dim
    # the generator's side: what every case must differ from, by min_effect (rel-L2)
    baseline: Optional[Callable] = None        # cfg_name -> (what it is, in the printed line; kwargs; state-dict change or None)
    effect_of: str = "the option"              # the assertion's subject: "<case>: <effect_of> moves the output by ... only"
    mistakes: dict = field(default_factory=dict)          # what -> f(state dict, patch_size): models that are wrong on purpose
    min_effect: float = 5e-2
    r16: bool = False               # the golden holds <case>__r16_fp16 / __r16_bf16, the reference with rounded operands

    def keys_path(self):
        return os.path.join(cases.GOLDEN_DIR, self.keys_file)


def family(name):
    return importlib.import_module(FAMILY_MODULES[name]).FAMILY


def scaled(sd, gain_of):
    """sd with every tensor multiplied by gain_of(key, tensor), where that is not None."""
    for k in sd:
        g = gain_of(k, sd[k])
        if g is not None:
            sd[k] = sd[k] * g
    return sd


def suffix_gain(gains):
    """gain_of for {key suffix: factor}."""
    return lambda k, v: next((g for suffix, g in gains.items() if k.endswith(suffix)), None)


def case_inputs(family, name):
    """(x, t, kwargs of DiffusionTransformer.forward) of a case.  Batch 2, 130 context tokens of cond_token_dim channels (no context where that
    is 0), P prepend tokens from seed 300 + P, the concat tensor by the family's rule."""
    cfg_name, t_len, p, cfg_scale = family.cases[name]
    cfg = family.configs[cfg_name]
    _, t, c, g = cases.dit_inputs(2, t_len, cfg["cond_token_dim"] or 128, 96, 1)
    x = synthetic.synth_input("x", (2, cfg["io_channels"], t_len), 1)
    cat = None
    if cfg.get("input_concat_dim"):
        shape, seed = family.concat(t_len)
        cat = synthetic.synth_input("concat", (2,) + shape, seed)
    return x, t, dict(cross_attn_cond=c if cfg["cond_token_dim"] else None, global_embed=g,
                      prepend_cond=synthetic.synth_input("prepend", (2, p, PREPEND_DIM), 300 + p) if p else None,
                      prepend_cond_mask=torch.ones(2, p) if p else None,          # (the reference concatenates it, dit.py:193; it never reaches the layers)
                      input_concat_cond=cat, cfg_scale=cfg_scale)
