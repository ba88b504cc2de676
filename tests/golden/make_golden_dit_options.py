"""Generates tests/golden/dit_options_small.npz and dit_options_state_dict_keys.json: the reduced DiT with the ContinuousTransformer
switches beyond the shipped configs -- qk_norm (reference models/transformer.py:433-436), the sinusoidal / absolute position embeddings
(:50-96, 796-797), rotary_pos_emb=False and a bias-free feed-forward (:270) -- by running the REFERENCE with the placeholder modules of
_ref_import.py.

Runs only in the build container (the reference does not travel).  Usage:
    python tests/golden/make_golden_dit_options.py
Stored: reference OUTPUTS only (fp32 .npz); weights and inputs are regenerated from seeds (dit_options_cases.py).
"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as MG  # noqa: E402  (imports the reference through _ref_import.py)
import cases  # noqa: E402
import dit_options_cases as OC  # noqa: E402

rdit = MG.rdit
MIN_EFFECT = 5e-2          # every case must differ at least this much (rel-L2) from the same model without the option


def _model(kwargs):
    m = rdit.DiffusionTransformer(**kwargs)
    m.load_state_dict(OC.synth_weights(m.state_dict(), 0))
    return m.eval()


@torch.no_grad()
def gen_cases():
    out, models, plain = {}, {}, {}
    for name, (cfg_name, _, _, cfg_scale) in OC.CASES.items():
        if cfg_name not in models:
            models[cfg_name] = _model(OC.CONFIGS[cfg_name])
            plain[cfg_name] = _model({k: v for k, v in OC.CONFIGS[cfg_name].items() if k not in OC.OPTION_KEYS})
        x, t, c, g, pc, pm, cc = OC.case_inputs(name)
        kw = dict(cross_attn_cond=c, global_embed=g, prepend_cond=pc, prepend_cond_mask=pm, input_concat_cond=cc, cfg_scale=cfg_scale)
        out[name] = models[cfg_name](x, t, **kw)
        base = plain[cfg_name](x, t, **kw)
        effect = float((out[name] - base).norm() / base.norm())
        print(f"{name}: {tuple(out[name].shape)} std {float(out[name].std()):.3f}, rel-L2 vs the model without the option {effect:.2e}")
        assert effect >= MIN_EFFECT, f"{name}: the option moves the output by {effect:.2e} only"
    MG.save("dit_options_small", **out)


def gen_keys():
    keys = {name: {k: list(v.shape) for k, v in rdit.DiffusionTransformer(**c).state_dict().items()} for name, c in OC.CONFIGS.items()}
    path = os.path.join(cases.GOLDEN_DIR, "dit_options_state_dict_keys.json")
    json.dump(keys, open(path, "w"), sort_keys=True)
    print("wrote", path, {k: len(v) for k, v in keys.items()})


if __name__ == "__main__":
    torch.set_num_threads(min(16, os.cpu_count()))
    gen_keys()
    gen_cases()
