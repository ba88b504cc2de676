"""Generates the goldens of the 32- / 96-channel-head family (dit_head_width_cases.py): tests/golden/dit_head_width_small*.npz and
dit_head_width_state_dict_keys.json, with the generator of the other DiT option families (make_golden_dit_families.py): the REFERENCE's
outputs, its outputs with rounded operands, and the assertion that every case differs from the model with 64-channel heads.

Runs only in the build container (the reference does not travel).  Usage:
    python tests/golden/make_golden_dit_head_width.py
"""
import os

import torch

import make_golden_dit_families as MF
import dit_head_width_cases as WC

if __name__ == "__main__":
    torch.set_num_threads(min(16, os.cpu_count()))
    MF.gen_keys(WC.FAMILY)
    MF.gen_cases(WC.FAMILY)
