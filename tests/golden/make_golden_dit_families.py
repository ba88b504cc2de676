"""Generates the goldens of the DiT option families (dit_family.FAMILY_MODULES): tests/golden/<stem>*.npz and <family>_state_dict_keys.json,
by running the REFERENCE with the placeholder modules of _ref_import.py on every case of the family's dit_*_cases.py.

Runs only in the build container (the reference does not travel).  Usage:
    python tests/golden/make_golden_dit_families.py [family ...]          (no argument: all of them)
Stored: reference OUTPUTS only (fp32 .npz); weights and inputs are regenerated from seeds (dit_family.py).  Where the family has them
(Family.r16), beside every case ``<case>``: ``<case>__r16_fp16`` and ``<case>__r16_bf16``, the reference's output with the input and the
weight of every nn.Linear / nn.Conv1d rounded to that format (forward pre-hooks) -- what 16-bit GEMM operands alone cost the reference on
this model, the yardstick of the family's 16-bit gates.

Asserted per case, so that a kernel which skips the option or makes the mistake cannot pass a gate: the output differs by Family.min_effect
(rel-L2) from the family's baseline model (the same config without the option, with 64-channel heads, with the centre taps alone) and from
each model of Family.mistakes (patch: feature order (p c) at either end, frames reversed inside a patch, both 1x1 convs dropped).  With
the patch family, once: the plain-torch restatement of the two rearranges that the kernel references use (tests/dit_patch_units.py) equals
einops on these shapes.
"""
import copy
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import make_golden as MG  # noqa: E402  (imports the reference through _ref_import.py)
import dit_family  # noqa: E402

rdit = MG.rdit
ROUND = {"fp16": lambda x: x.clamp(-65504.0, 65504.0).to(torch.float16).to(torch.float32),
         "bf16": lambda x: x.to(torch.bfloat16).to(torch.float32)}


def _model(family, cfg_name, kwargs=None, change=None):
    m = rdit.DiffusionTransformer(**(kwargs or family.configs[cfg_name]))
    sd = family.weights(cfg_name, m.state_dict(), 0)
    m.load_state_dict(change(sd) if change else sd)
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


def _rel(a, b):
    return float((a - b).norm() / b.norm())


def _models(family, cfg_name):
    """(the model, (what the baseline is, the baseline model) or None, {mistake: model}, {format: the model with rounded operands})"""
    m, baseline = _model(family, cfg_name), None
    if family.baseline:
        what, kwargs, change = family.baseline(cfg_name)
        baseline = (what, _model(family, cfg_name, kwargs, change))
    P = family.configs[cfg_name].get("patch_size")
    wrong = {what: _model(family, cfg_name, change=lambda sd, f=f: f(sd, P)) for what, f in family.mistakes.items()}
    return m, baseline, wrong, ({fmt: _rounded(m, fmt) for fmt in ROUND} if family.r16 else {})


@torch.no_grad()
def gen_cases(family):
    out, models = {}, {}
    for name, (cfg_name, _, _, _) in family.cases.items():
        if cfg_name not in models:
            models[cfg_name] = _models(family, cfg_name)
        m, baseline, wrong, r16 = models[cfg_name]
        x, t, kw = dit_family.case_inputs(family, name)
        out[name] = m(x, t, **kw)
        line = f"{name}: {tuple(out[name].shape)} std {float(out[name].std()):.3f}"
        effects = {}
        if baseline:
            effects[family.effect_of] = _rel(out[name], baseline[1](x, t, **kw))
            line += f", rel-L2 vs {baseline[0]} {effects[family.effect_of]:.2e}"
        for fmt, rm in r16.items():
            out[f"{name}__r16_{fmt}"] = rm(x, t, **kw)
            line += f", rounded operands {fmt} {_rel(out[f'{name}__r16_{fmt}'], out[name]):.2e}"
        print(line)
        for what, wm in wrong.items():
            e = effects[f"'{what}'"] = _rel(wm(x, t, **kw), out[name])
            print(f"    {what}: moves the output by {e:.2e}")
        for what, effect in effects.items():
            assert effect >= family.min_effect, f"{name}: {what} moves the output by {effect:.2e} only"
    MG.save(family.stem, **out)


def gen_keys(family):
    keys = {name: {k: list(v.shape) for k, v in rdit.DiffusionTransformer(**c).state_dict().items()} for name, c in family.configs.items()}
    json.dump(keys, open(family.keys_path(), "w"), sort_keys=True)
    print("wrote", family.keys_path(), {k: len(v) for k, v in keys.items()})


def check_rearranges(family):
    """tests/dit_patch_units.py restates the reference's two einops patterns with reshape / permute: bit for bit the same on every case shape."""
    from einops import rearrange
    import dit_patch_units as PU
    for name, (cfg_name, t_len, _, _) in family.cases.items():
        cfg = family.configs[cfg_name]
        P, ci, c = cfg["patch_size"], cfg["io_channels"] + cfg.get("input_concat_dim", 0), cfg["io_channels"]
        a = torch.randn(2, t_len, ci)
        assert torch.equal(PU.patchify(a, P), rearrange(a, "b (t p) c -> b t (c p)", p=P)), name
        o = torch.randn(2, c * P, t_len // P)
        assert torch.equal(PU.unpatchify(o, P), rearrange(o, "b (c p) t -> b c (t p)", p=P)), name
    print("patchify / unpatchify of tests/dit_patch_units.py equal the reference's einops patterns on", len(family.cases), "case shapes")


if __name__ == "__main__":
    torch.set_num_threads(min(16, os.cpu_count()))
    for which in sys.argv[1:] or list(dit_family.FAMILY_MODULES):
        fam = dit_family.family(which)
        if which == "patch":
            check_rearranges(fam)
        gen_keys(fam)
        gen_cases(fam)
