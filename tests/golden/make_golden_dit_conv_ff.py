"""Generates tests/golden/dit_conv_ff_small*.npz and dit_conv_ff_state_dict_keys.json: the reduced DiT with convolutional feed-forwards
(ff_kwargs use_conv, reference models/transformer.py:211-287) by running the REFERENCE with the placeholder modules of _ref_import.py.

Runs only in the build container (the reference does not travel).  Usage:
    python tests/golden/make_golden_dit_conv_ff.py
Stored: reference OUTPUTS only (fp32 .npz); weights and inputs are regenerated from seeds (dit_conv_ff_cases.py).  Beside every case
``<case>``: ``<case>__r16_fp16`` and ``<case>__r16_bf16``, the reference's output with the input and the weight of every nn.Linear /
nn.Conv1d rounded to that format (forward pre-hooks) -- what 16-bit GEMM operands alone cost the reference on this model, the yardstick of
the 16-bit gates of tests/test_gpu_dit_conv_ff.py.
"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as MG  # noqa: E402  (imports the reference through _ref_import.py)
import cases  # noqa: E402
import dit_conv_ff_cases as CC  # noqa: E402
from make_golden_dit_block_options import ROUND, _rounded  # noqa: E402

rdit = MG.rdit
MIN_EFFECT = 5e-2          # every case must differ at least this much (rel-L2) from the same model with the off-centre taps zeroed


def _model(kwargs, centre_only=False):
    m = rdit.DiffusionTransformer(**kwargs)
    sd = CC.synth_weights(m.state_dict(), 0)
    m.load_state_dict(CC.centre_taps_only(sd) if centre_only else sd)
    return m.eval()


@torch.no_grad()
def gen_cases():
    out, models, centre, r16 = {}, {}, {}, {}
    for name, (cfg_name, _, _, cfg_scale) in CC.CASES.items():
        if cfg_name not in models:
            models[cfg_name] = _model(CC.CONFIGS[cfg_name])
            centre[cfg_name] = _model(CC.CONFIGS[cfg_name], centre_only=True)
            r16[cfg_name] = {fmt: _rounded(models[cfg_name], fmt) for fmt in ROUND}
        x, t, c, g, pc, pm = CC.case_inputs(name)
        kw = dict(cross_attn_cond=c, global_embed=g, prepend_cond=pc, prepend_cond_mask=pm, cfg_scale=cfg_scale)
        out[name] = models[cfg_name](x, t, **kw)
        base = centre[cfg_name](x, t, **kw)
        effect = float((out[name] - base).norm() / base.norm())
        line = f"{name}: {tuple(out[name].shape)} std {float(out[name].std()):.3f}, rel-L2 vs the centre taps alone {effect:.2e}"
        for fmt in ROUND:
            out[f"{name}__r16_{fmt}"] = r16[cfg_name][fmt](x, t, **kw)
            line += f", rounded operands {fmt} {float((out[f'{name}__r16_{fmt}'] - out[name]).norm() / out[name].norm()):.2e}"
        print(line)
        assert effect >= MIN_EFFECT, f"{name}: the off-centre taps move the output by {effect:.2e} only (OFF_CENTRE_GAIN {CC.OFF_CENTRE_GAIN})"
    MG.save("dit_conv_ff_small", **out)


def gen_keys():
    keys = {name: {k: list(v.shape) for k, v in rdit.DiffusionTransformer(**c).state_dict().items()} for name, c in CC.CONFIGS.items()}
    path = os.path.join(cases.GOLDEN_DIR, "dit_conv_ff_state_dict_keys.json")
    json.dump(keys, open(path, "w"), sort_keys=True)
    print("wrote", path, {k: len(v) for k, v in keys.items()})


if __name__ == "__main__":
    torch.set_num_threads(min(16, os.cpu_count()))
    gen_keys()
    gen_cases()
