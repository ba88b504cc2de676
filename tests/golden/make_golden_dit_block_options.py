"""Generates tests/golden/dit_block_options_small.npz and dit_block_options_state_dict_keys.json: the reduced DiT with the TransformerBlock
options beyond the shipped configs -- conformer (reference models/transformer.py:557-591, 645, 680-681, 697-698), remove_norms (:621, 632,
642) and a feed-forward without GLU (:259-268) -- by running the REFERENCE with the placeholder modules of _ref_import.py.

Runs only in the build container (the reference does not travel).  Usage:
    python tests/golden/make_golden_dit_block_options.py
Stored: reference OUTPUTS only (fp32 .npz); weights and inputs are regenerated from seeds (dit_block_options_cases.py).  Beside every case
``<case>``: ``<case>__r16_fp16`` and ``<case>__r16_bf16``, the reference's output with the input and the weight of every nn.Linear /
nn.Conv1d rounded to that format (forward pre-hooks) -- what 16-bit GEMM operands alone cost the reference on this model, the yardstick of
the 16-bit gates of tests/test_gpu_dit_block_options.py.
"""
import copy
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as MG  # noqa: E402  (imports the reference through _ref_import.py)
import cases  # noqa: E402
import dit_block_options_cases as BC  # noqa: E402

rdit = MG.rdit
MIN_EFFECT = 5e-2          # every case must differ at least this much (rel-L2) from the same model without the option(s)
ROUND = {"fp16": lambda x: x.clamp(-65504.0, 65504.0).to(torch.float16).to(torch.float32),
         "bf16": lambda x: x.to(torch.bfloat16).to(torch.float32)}


def _model(kwargs):
    m = rdit.DiffusionTransformer(**kwargs)
    m.load_state_dict(BC.synth_weights(m.state_dict(), 0))
    return m.eval()


def _rounded(model, fmt):
    """A copy of the model whose nn.Linear / nn.Conv1d see their input and their weight rounded to fmt (the bias stays fp32)."""
    rnd = ROUND[fmt]
    m = copy.deepcopy(model)
    for mod in m.modules():
        if isinstance(mod, (torch.nn.Linear, torch.nn.Conv1d)):
            mod.weight.data = rnd(mod.weight.data)
            mod.register_forward_pre_hook(lambda _, args: (rnd(args[0]),) + tuple(args[1:]))
    return m


@torch.no_grad()
def gen_cases():
    out, models, plain, r16 = {}, {}, {}, {}
    for name, (cfg_name, _, _, cfg_scale) in BC.CASES.items():
        if cfg_name not in models:
            models[cfg_name] = _model(BC.CONFIGS[cfg_name])
            plain[cfg_name] = _model(BC.without_options(BC.CONFIGS[cfg_name]))
            r16[cfg_name] = {fmt: _rounded(models[cfg_name], fmt) for fmt in ROUND}
        x, t, c, g, pc, pm = BC.case_inputs(name)
        kw = dict(cross_attn_cond=c, global_embed=g, prepend_cond=pc, prepend_cond_mask=pm, cfg_scale=cfg_scale)
        out[name] = models[cfg_name](x, t, **kw)
        base = plain[cfg_name](x, t, **kw)
        effect = float((out[name] - base).norm() / base.norm())
        line = f"{name}: {tuple(out[name].shape)} std {float(out[name].std()):.3f}, rel-L2 vs the model without the option {effect:.2e}"
        for fmt in ROUND:
            out[f"{name}__r16_{fmt}"] = r16[cfg_name][fmt](x, t, **kw)
            line += f", rounded operands {fmt} {float((out[f'{name}__r16_{fmt}'] - out[name]).norm() / out[name].norm()):.2e}"
        print(line)
        assert effect >= MIN_EFFECT, f"{name}: the option moves the output by {effect:.2e} only"
    MG.save("dit_block_options_small", **out)


def gen_keys():
    keys = {name: {k: list(v.shape) for k, v in rdit.DiffusionTransformer(**c).state_dict().items()} for name, c in BC.CONFIGS.items()}
    path = os.path.join(cases.GOLDEN_DIR, "dit_block_options_state_dict_keys.json")
    json.dump(keys, open(path, "w"), sort_keys=True)
    print("wrote", path, {k: len(v) for k, v in keys.items()})


if __name__ == "__main__":
    torch.set_num_threads(min(16, os.cpu_count()))
    gen_keys()
    gen_cases()
