"""Generates the goldens of the neighbourhood-attention family (dit_natten_cases.py): tests/golden/dit_natten_small*.npz and
dit_natten_state_dict_keys.json, with the generator of the other DiT option families (make_golden_dit_families.py): the REFERENCE's
outputs, its outputs with rounded operands, and the assertion that every case differs from the same model with natten_kernel_size=None.

NATTEN is not installed where this runs.  The reference's transformer module holds the library as the module attribute ``natten`` (None
after its failed import); tests/golden/natten_standin.py -- this project's own statement of natten1dqk / natten1dav, checked against a
float64 masked softmax by tests/test_dit_natten_host.py -- is set in its place.  The goldens are therefore pinned by the stand-in, not by
the library.  No reference text changes.

Asserted at the end, over all cases and both formats: the reference's own rounded-operand figure (__r16_*) is at most half the harness gate
(dit_family_gpu.Harness.gate) of the case.  The goldens are written first.  As the gates stand the assertion FAILS, here as it would on
every family without a window: at CFG 1 the figure is 4.4e-4 - 5.6e-4 in fp16 (gate 6.25e-4) and 3.6e-3 - 4.4e-3 in bf16 (gate 2.5e-3),
whatever the q / k gain -- the rounding of the other GEMMs' operands alone gives it (profiles/dit_natten_verification.txt has every figure).
The product rounds at fewer points than this yardstick and passes the gates; neither the gates nor the gains were moved to meet it.

Runs only in the build container (the reference does not travel).  Usage:
    python tests/golden/make_golden_dit_natten.py
"""
import os

import torch

import make_golden_dit_families as MF
import dit_natten_cases as NC
import natten_standin

GATES = {"bf16": 1.0, "fp16": 0.25}          # util.OperandFormat.tol_scale


def harness_gate(name, fmt):
    return GATES[fmt] * (2.5e-3 if NC.CASES[name][3] == 1.0 else 1.2e-2)          # dit_family_gpu.Harness.gate


def check_r16():
    import cases
    gold = cases.load(NC.FAMILY.stem)
    worst = []
    for name in NC.CASES:
        for fmt in GATES:
            e = float((gold[f"{name}__r16_{fmt}"] - gold[name]).norm() / gold[name].norm())
            gate = harness_gate(name, fmt)
            print(f"{name} {fmt}: reference with rounded operands {e:.2e}, harness gate {gate:.2e}, ratio {e / gate:.2f}")
            if e > 0.5 * gate:
                worst.append((name, fmt, e, gate))
    assert not worst, "rounded-operand figure above half the harness gate: " + ", ".join(f"{n} {f} {e:.2e} / {g:.2e}" for n, f, e, g in worst)


if __name__ == "__main__":
    torch.set_num_threads(min(16, os.cpu_count()))
    rtf = MF.rdit.ContinuousTransformer.__init__.__globals__          # the namespace of the reference's models/transformer.py as imported
    assert "natten" in rtf and rtf["natten"] is None, "the reference's transformer module no longer keeps the (missing) library as `natten`"
    rtf["natten"] = natten_standin
    MF.gen_keys(NC.FAMILY)
    MF.gen_cases(NC.FAMILY)
    check_r16()
