"""Generates tests/golden/dit_head_dim_small.npz and dit_head_dim_state_dict_keys.json: the reduced DiT with 128-channel attention heads
(reference models/transformer.py:303-308, 517, 737: heads of dim_heads channels, score scale dim_heads ** -0.5, cross-attention kv heads
dim_context // dim_heads, RotaryEmbedding(max(dim_heads // 2, 32)) = a rotation of the first 64 channels in pairs (j, j + 32)) by running
the REFERENCE with the placeholder modules of _ref_import.py.

Runs only in the build container (the reference does not travel).  Usage:
    python tests/golden/make_golden_dit_head_dim.py
Stored: reference OUTPUTS only (fp32 .npz); weights and inputs are regenerated from seeds (dit_head_dim_cases.py).
"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as MG  # noqa: E402  (imports the reference through _ref_import.py)
import cases  # noqa: E402
import dit_head_dim_cases as HC  # noqa: E402

rdit = MG.rdit
MIN_EFFECT = 3e-2          # every case must differ at least this much (rel-L2) from the same model with 64-channel heads


def _model(kwargs):
    m = rdit.DiffusionTransformer(**kwargs)
    m.load_state_dict(HC.synth_weights(m.state_dict(), 0))
    return m.eval()


@torch.no_grad()
def gen_cases():
    out, models, narrow = {}, {}, {}
    for name, (cfg_name, _, _, cfg_scale) in HC.CASES.items():
        if cfg_name not in models:
            models[cfg_name] = _model(HC.CONFIGS[cfg_name])
            narrow[cfg_name] = _model(HC.with_64_channel_heads(HC.CONFIGS[cfg_name]))
        x, t, c, g, pc, pm, cc = HC.case_inputs(name)
        kw = dict(cross_attn_cond=c, global_embed=g, prepend_cond=pc, prepend_cond_mask=pm, input_concat_cond=cc, cfg_scale=cfg_scale)
        out[name] = models[cfg_name](x, t, **kw)
        base = narrow[cfg_name](x, t, **kw)
        effect = float((out[name] - base).norm() / base.norm())
        print(f"{name}: {tuple(out[name].shape)} std {float(out[name].std()):.3f}, rel-L2 vs the model with 64-channel heads {effect:.2e}")
        assert effect >= MIN_EFFECT, f"{name}: the head width moves the output by {effect:.2e} only"
    MG.save("dit_head_dim_small", **out)


def gen_keys():
    keys = {name: {k: list(v.shape) for k, v in rdit.DiffusionTransformer(**c).state_dict().items()} for name, c in HC.CONFIGS.items()}
    path = os.path.join(cases.GOLDEN_DIR, "dit_head_dim_state_dict_keys.json")
    json.dump(keys, open(path, "w"), sort_keys=True)
    print("wrote", path, {k: len(v) for k, v in keys.items()})


if __name__ == "__main__":
    torch.set_num_threads(min(16, os.cpu_count()))
    gen_keys()
    gen_cases()
