"""Generates tests/golden/dit_patch_small*.npz and dit_patch_state_dict_keys.json: the patchified reduced DiT (DiffusionTransformer
patch_size > 1, reference models/dit.py:38,88-89,119-120,197-224) by running the REFERENCE with the placeholder modules of _ref_import.py.

Runs only in the build container (the reference does not travel).  Usage:
    python tests/golden/make_golden_dit_patch.py
Stored: reference OUTPUTS only (fp32 .npz); weights and inputs are regenerated from seeds (dit_patch_cases.py).  Beside every case
``<case>``: ``<case>__r16_fp16`` and ``<case>__r16_bf16``, the reference's output with the input and the weight of every nn.Linear /
nn.Conv1d rounded to that format -- the yardstick of the 16-bit gates of tests/test_gpu_dit_patch.py.

Asserted per case: each mistake of dit_patch_cases.MISTAKES (feature order (p c) at either end, frames reversed inside a patch, both 1x1
convs dropped) moves the reference's output by at least MIN_EFFECT, so that a kernel with that mistake cannot pass a gate.  And once: the
plain-torch restatement of the two rearranges that the kernel references use (tests/dit_patch_units.py) equals einops on these shapes.
"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import make_golden as MG  # noqa: E402  (imports the reference through _ref_import.py)
import cases  # noqa: E402
import dit_patch_cases as PC  # noqa: E402
from make_golden_dit_block_options import ROUND, _rounded  # noqa: E402

rdit = MG.rdit
MIN_EFFECT = 5e-2          # every case must differ at least this much (rel-L2) from the same model with each mistake built in


def _model(cfg_name, mistake=None):
    kwargs = PC.CONFIGS[cfg_name]
    m = rdit.DiffusionTransformer(**kwargs)
    sd = PC.synth_weights(cfg_name, m.state_dict(), 0)
    m.load_state_dict(mistake(sd, kwargs["patch_size"]) if mistake else sd)
    return m.eval()


@torch.no_grad()
def gen_cases():
    out, models, wrong, r16 = {}, {}, {}, {}
    for name, (cfg_name, _, _, _) in PC.CASES.items():
        if cfg_name not in models:
            models[cfg_name] = _model(cfg_name)
            wrong[cfg_name] = {what: _model(cfg_name, f) for what, f in PC.MISTAKES.items()}
            r16[cfg_name] = {fmt: _rounded(models[cfg_name], fmt) for fmt in ROUND}
        x, t, kw = PC.forward_kwargs(name)
        out[name] = models[cfg_name](x, t, **kw)
        line = f"{name}: {tuple(out[name].shape)} std {float(out[name].std()):.3f}"
        for fmt in ROUND:
            out[f"{name}__r16_{fmt}"] = r16[cfg_name][fmt](x, t, **kw)
            line += f", rounded operands {fmt} {float((out[f'{name}__r16_{fmt}'] - out[name]).norm() / out[name].norm()):.2e}"
        print(line)
        for what, m in wrong[cfg_name].items():
            effect = float((m(x, t, **kw) - out[name]).norm() / out[name].norm())
            print(f"    {what}: moves the output by {effect:.2e}")
            assert effect >= MIN_EFFECT, f"{name}: '{what}' moves the output by {effect:.2e} only"
    MG.save("dit_patch_small", **out)


def gen_keys():
    keys = {name: {k: list(v.shape) for k, v in rdit.DiffusionTransformer(**c).state_dict().items()} for name, c in PC.CONFIGS.items()}
    path = os.path.join(cases.GOLDEN_DIR, "dit_patch_state_dict_keys.json")
    json.dump(keys, open(path, "w"), sort_keys=True)
    print("wrote", path, {k: len(v) for k, v in keys.items()})


def check_rearranges():
    """tests/dit_patch_units.py restates the reference's two einops patterns with reshape / permute: bit for bit the same on every case shape."""
    from einops import rearrange
    import dit_patch_units as PU
    for name, (cfg_name, t_len, _, _) in PC.CASES.items():
        cfg = PC.CONFIGS[cfg_name]
        P, ci, c = cfg["patch_size"], cfg["io_channels"] + cfg.get("input_concat_dim", 0), cfg["io_channels"]
        a = torch.randn(2, t_len, ci)
        assert torch.equal(PU.patchify(a, P), rearrange(a, "b (t p) c -> b t (c p)", p=P)), name
        o = torch.randn(2, c * P, t_len // P)
        assert torch.equal(PU.unpatchify(o, P), rearrange(o, "b (c p) t -> b c (t p)", p=P)), name
    print("patchify / unpatchify of tests/dit_patch_units.py equal the reference's einops patterns on", len(PC.CASES), "case shapes")


if __name__ == "__main__":
    torch.set_num_threads(min(16, os.cpu_count()))
    check_rearranges()
    gen_keys()
    gen_cases()
