"""Generates the goldens of the neighbourhood-attention family at 128-, 32- and 96-channel heads (dit_natten_hdw_cases.py):
tests/golden/dit_natten_hdw_small*.npz and dit_natten_hdw_state_dict_keys.json, with the generator of the other DiT option families
(make_golden_dit_families.py) and, as make_golden_dit_natten.py, tests/golden/natten_standin.py set in the place of the NATTEN library the
reference's transformer module failed to import.  No reference text changes.

Per candidate case it prints the reference's own figure with the operands of every Linear rounded to fp16 and to bf16 (__r16_*), beside the
harness gate of that format (dit_family_gpu.Harness.gate).  A case runs in a format only where the figure is BELOW the gate, so that the
reference alone passes: the others are what dit_natten_hdw_cases.DROPPED must list, and the generator fails (after printing the table that
belongs there) when it does not.  Gates and gains are not moved to meet a figure.  Only the cases of CASES are written.

Runs only in the build container (the reference does not travel).  Usage:
    python tests/golden/make_golden_dit_natten_hdw.py
"""
import dataclasses
import os

import torch

import make_golden_dit_families as MF
import dit_family
import dit_natten_hdw_cases as HC
import natten_standin
from make_golden_dit_natten import GATES


def harness_gate(name, fmt):
    return GATES[fmt] * (2.5e-3 if HC.CANDIDATES[name][3] == 1.0 else 1.2e-2)          # dit_family_gpu.Harness.gate


@torch.no_grad()
def gen_candidates():
    """MF.gen_cases over the candidates, kept in memory: {key: output}, and {format: {case: figure}} of the cases at or above their gate."""
    family = dataclasses.replace(HC.FAMILY, cases=HC.CANDIDATES)
    out, models, over = {}, {}, {fmt: {} for fmt in GATES}
    for name, (cfg_name, _, _, _) in family.cases.items():
        if cfg_name not in models:
            models[cfg_name] = MF._models(family, cfg_name)
        m, baseline, _, r16 = models[cfg_name]
        x, t, kw = dit_family.case_inputs(family, name)
        out[name] = m(x, t, **kw)
        effect = MF._rel(out[name], baseline[1](x, t, **kw))
        line = f"{name}: {tuple(out[name].shape)} std {float(out[name].std()):.3f}, rel-L2 vs {baseline[0]} {effect:.2e}"
        assert effect >= family.min_effect, f"{name}: {family.effect_of} moves the output by {effect:.2e} only"
        for fmt, rm in r16.items():
            out[f"{name}__r16_{fmt}"] = rm(x, t, **kw)
            e, gate = MF._rel(out[f"{name}__r16_{fmt}"], out[name]), harness_gate(name, fmt)
            line += f"; rounded operands {fmt} {e:.2e} (gate {gate:.2e}, ratio {e / gate:.2f}{'' if e < gate else ', DROPPED'})"
            if not e < gate:
                over[fmt][name] = float(f"{e:.2e}")
        print(line, flush=True)
    return out, over


if __name__ == "__main__":
    torch.set_num_threads(min(16, os.cpu_count()))
    rtf = MF.rdit.ContinuousTransformer.__init__.__globals__          # the namespace of the reference's models/transformer.py as imported
    assert "natten" in rtf and rtf["natten"] is None, "the reference's transformer module no longer keeps the (missing) library as `natten`"
    rtf["natten"] = natten_standin
    MF.gen_keys(HC.FAMILY)
    out, over = gen_candidates()
    print("DROPPED =", over)
    assert over == HC.DROPPED, "dit_natten_hdw_cases.DROPPED is not what was measured: put the table above there and run again"
    MF.MG.save(HC.FAMILY.stem, **{k: v for k, v in out.items() if k.split("__")[0] in HC.CASES})
