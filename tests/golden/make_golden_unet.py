"""Generates the goldens of the Dance Diffusion U-Net (unet_cases.py): tests/golden/unet_small.npz and unet_state_dict_keys.json, by running the
REFERENCE's DiffusionAttnUnet1D (models/diffusion.py:376-479, imported through the aliased package of _ref_import.py, which stays as it is) on
the CPU.  The class is the pinned boundary: the reference's factory and generator for this model do not run (README, "Dance Diffusion
configurations").  No reference text changes.

Per case, beside the fp32 output: ``__r16_fp16`` / ``__r16_bf16``, the output with the input and the weight of every nn.Conv1d rounded to that
format (forward pre-hooks), and ``__f64``, the output of the same module in float64.

Asserted: every figure is finite; every output moves by at least 5 % when every attention out_proj, and separately every block's second
convolution, is zeroed; every rounded-operand figure is below unet_cases.R16_LIMIT in both formats (no case is dropped); the yardsticks
themselves pass the per-time-step gate; case C's length is accepted by the reference and case A's config fails at 16 samples.  The figures are
printed as the literals of unet_cases.R16 / F64.

Runs only where the reference is present.  Usage:
    python tests/golden/make_golden_unet.py
"""
import copy
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import _ref_import  # noqa: E402
import cases  # noqa: E402
import unet_cases as UC  # noqa: E402
import util  # noqa: E402

rdf = _ref_import.ref("models.diffusion")

ROUND = {"fp16": util.fp16_round, "bf16": util.bf16_round}


def rounded(model, fmt):
    """A copy of the model whose nn.Conv1d see their input and their weight rounded to fmt (the bias stays fp32)."""
    rnd = ROUND[fmt]
    m = copy.deepcopy(model)
    for mod in m.modules():
        if isinstance(mod, torch.nn.Conv1d):
            mod.weight.data = rnd(mod.weight.data)
            mod.register_forward_pre_hook(lambda _, args: (rnd(args[0]),) + tuple(args[1:]))
    return m


def build(name, sd_fn=None):
    model = rdf.DiffusionAttnUnet1D(**copy.deepcopy(UC.CASES[name][0]))
    sd = UC.weights(model.state_dict())
    model.load_state_dict(sd_fn(sd) if sd_fn else sd, strict=True)
    return model.eval()


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


@torch.no_grad()
def generate():
    out, keys, r16, f64 = {}, {}, {}, {}
    for name in UC.CASES:
        model = build(name)
        keys[name] = {k: list(v.shape) for k, v in model.state_dict().items()}
        x, t = UC.inputs(name)
        want = out[name] = model(x, t)
        for fmt in ROUND:
            out[f"{name}__r16_{fmt}"] = rounded(model, fmt)(x, t)
        out[f"{name}__f64"] = copy.deepcopy(model).double()(x.double(), t.double())
        assert out[f"{name}__f64"].dtype == torch.float64
        for what in ("out_proj", "main.3"):
            if what == "out_proj" and UC.CASES[name][0]["n_attn_layers"] == 0:
                continue
            effect = rel(want, build(name, lambda sd: UC.zeroed(sd, what))(x, t))
            print(f"{name}: {tuple(want.shape)} std {float(want.std()):.3f}, rel-L2 vs the model with every {what} zeroed {effect:.2e}")
            assert effect >= 0.05, f"{name}: {what} moves the output by {effect:.2e} only"
        r16[name] = {fmt: rel(out[f"{name}__r16_{fmt}"], want) for fmt in ROUND}
        f64[name] = rel(want, out[f"{name}__f64"])
        assert all(torch.isfinite(v).all() for k, v in out.items() if k.startswith(name))
        for fmt in ROUND:
            assert r16[name][fmt] < UC.R16_LIMIT, (name, fmt, r16[name][fmt])
            rows = util.slice_errors(out[f"{name}__r16_{fmt}"], want, (0, 2)).max().item()
            assert rows <= UC.ROW_FACTOR * 2.0 * r16[name][fmt], (name, fmt, rows, r16[name][fmt])
            print(f"{name} {fmt}: rounded operands {r16[name][fmt]:.3e} (gate {2 * r16[name][fmt]:.3e}), worst time step {rows:.3e}")
        rows = util.slice_errors(want, out[f"{name}__f64"], (0, 2)).max().item()
        assert rows <= UC.ROW_FACTOR * 4.0 * f64[name], (name, rows, f64[name])
        print(f"{name} fp32: vs float64 {f64[name]:.3e} (gate {4 * f64[name]:.3e}), worst time step {rows:.3e}")
    # the length rule: the reference runs case A's model at 24 samples (above) and fails at 16
    try:
        build("A")(torch.zeros(1, 2, 16), torch.zeros(1))
        raise AssertionError("the reference accepted 16 samples at depth 4")
    except RuntimeError as e:
        print("A at 16 samples: the reference fails:", str(e).splitlines()[0][:100])
    return out, keys, r16, f64


if __name__ == "__main__":
    torch.set_num_threads(min(16, os.cpu_count()))
    out, keys, r16, f64 = generate()
    json.dump(keys, open(UC.KEYS_PATH, "w"), sort_keys=True)
    paths = cases.save(UC.STEM, {k: v.detach().cpu().numpy() for k, v in out.items()})
    print("wrote", UC.KEYS_PATH, {k: len(v) for k, v in keys.items()})
    print("wrote", ", ".join(f"{p} ({os.path.getsize(p) // 1024} KiB)" for p in paths))
    fmt = lambda d: "{" + ", ".join(f'"{k}": {v:.3e}' for k, v in d.items()) + "}"
    print("R16 = {\n" + "\n".join(f'    "{e}": {fmt(v)},' for e, v in r16.items()) + "\n}")
    print("F64 = " + fmt(f64))
