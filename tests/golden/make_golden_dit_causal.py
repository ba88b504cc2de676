"""Generates the goldens of the causal family (dit_causal_cases.py): tests/golden/dit_causal_small*.npz and dit_causal_state_dict_keys.json,
with the generator of the other DiT option families (make_golden_dit_families.py): the REFERENCE's outputs, its outputs with rounded
operands, and the assertion that every case differs from the same model with causal=False.

On the CPU the reference's attention takes its einsum branch, which fails for causal=True (it calls a mask helper the module does not
have).  Its SDPA branch -- the one it takes on a GPU without flash-attn -- runs on the CPU as well and is chosen per instance with the
attribute ``use_pt_flash``: the model builder is wrapped to set it on every Attention module after construction.  No reference text changes.

Runs only in the build container (the reference does not travel).  Usage:
    python tests/golden/make_golden_dit_causal.py
"""
import os

import torch

import make_golden_dit_families as MF
import dit_causal_cases as CC

_rdit = MF.rdit


class _SdpaDit:
    """Stands in for the reference's dit module inside make_golden_dit_families: the same DiffusionTransformer on the SDPA branch."""

    @staticmethod
    def DiffusionTransformer(**kwargs):
        m = _rdit.DiffusionTransformer(**kwargs)
        n = 0
        for mod in m.modules():
            if type(mod).__name__ == "Attention":
                mod.use_pt_flash = True
                n += 1
        assert n == kwargs["depth"], "one self-attention per block (cond_token_dim = 0)"
        return m


if __name__ == "__main__":
    torch.set_num_threads(min(16, os.cpu_count()))
    MF.rdit = _SdpaDit
    MF.gen_keys(CC.FAMILY)
    MF.gen_cases(CC.FAMILY)
