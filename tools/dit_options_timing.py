"""What the ContinuousTransformer options cost per sampler step at the SA-Open shape: the full-size DiT (24 blocks, D = 1536), one prompt
with CFG 7 (two sequences of 1 + 1024 rows, 130 context tokens), `denoise` = one sat_dit_denoise_cfg call.

For the shipped config and for qk_norm, the sinusoidal and the absolute position embedding, and qk_norm + sinusoidal + no_bias: windows
of --window back-to-back steps between one pair of device events, median / min / max per step over --reps windows after --warmup
steps.  Weights are the synthetic ones of the benchmark (the time does not depend on the values).  Needs a HIP device; prints and, with
--out, writes the report.

    python tools/dit_options_timing.py --out profiles/dit_options_timing.txt
"""
import argparse

import torch

import dit_step_timing as ST          # (puts the package on sys.path)

VARIANTS = {
    "shipped config": {},
    "qk_norm": {"attn_kwargs": {"qk_norm": True}},
    "use_sinusoidal_emb": {"use_sinusoidal_emb": True},
    "use_abs_pos_emb (max 2048)": {"use_abs_pos_emb": True, "abs_pos_emb_max_length": 2048},
    "qk_norm + sinusoidal + no_bias": {"attn_kwargs": {"qk_norm": True}, "use_sinusoidal_emb": True, "ff_kwargs": {"no_bias": True}},
}


def main():
    a = ST.add_common_args(argparse.ArgumentParser()).parse_args()
    dev = torch.device("cuda:0")
    lines, ref = [], None
    for name, extra in VARIANTS.items():
        med, lo, hi = ST.step_windows(dev, a, extra)
        ref = med if ref is None else ref
        lines.append(f"{name:34s} {med:8.3f} ms / step  (min {lo:.3f}, max {hi:.3f})   {1e3 * (med - ref):+8.1f} us vs the shipped config"
                     f"  ({100 * (med / ref - 1):+.2f} %)")
        print(lines[-1], flush=True)
    head = (f"DiT options, cost per sampler step: full-size DiT, T = {a.t_len}, one prompt, CFG 7 (2 sequences), gemm_dtype "
            f"{a.dtype or 'package default'}, {torch.cuda.get_device_name(0)}\n{a.window} steps per event pair, median of {a.reps} windows\n")
    ST.write_report(a.out, head, lines)


if __name__ == "__main__":
    main()
