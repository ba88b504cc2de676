"""What a format boundary costs: one sampler step (`denoise` = one sat_dit_denoise_cfg call) of the full-size DiT (24 blocks, D 1536),
T = 1024, one prompt with CFG 7, as the uniform fp16 plan, the uniform bf16 plan and a plan with --bf16-blocks (default 11,12: two
neighbouring blocks in bf16, 22 in fp16, two boundaries) -- each boundary is one more LayerNorm launch, and the FF-out in front of it no
longer writes the 16-bit image (csrc/dit_plan.hip, proj_kind).  --bf16-blocks 5,17 has four boundaries.

The plans are three modules on the same weights; their windows alternate (--reps rounds of one window of --window back-to-back steps each,
between one pair of device events), so drift of the clocks lands on all of them alike.  Median / min / max per plan.  Synthetic weights and
inputs (the time does not depend on the values).  Needs a HIP device; --out appends.

    python tools/block_formats_timing.py --out profiles/block_formats_verification.txt
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "friendly-stable-audio-tools_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bf16-blocks", default="11,12")
    ap.add_argument("--t-len", type=int, default=1024)
    ap.add_argument("--window", type=int, default=20)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    from stable_audio_tools import model_configs as MC, synthetic
    from stable_audio_tools.models import _init
    from stable_audio_tools.models.dit import DiffusionTransformer
    base = MC.stable_audio_open_1_0()["model"]["diffusion"]["config"]
    x = synthetic.synth_input("x", (1, 64, a.t_len), 1).to(dev)
    c = synthetic.synth_input("c", (1, 130, base["cond_token_dim"]), 2).to(dev)
    g = synthetic.synth_input("g", (1, base["global_cond_dim"]), 3).to(dev)
    with _init.skip_init():
        template = DiffusionTransformer(**base)
    sd = synthetic.synth_state_dict(template.state_dict(), 0)
    moved = sorted(int(v) for v in a.bf16_blocks.split(","))
    mixed = ["bf16" if l in moved else "fp16" for l in range(base["depth"])]
    boundaries = sum(mixed[l] != mixed[l - 1] for l in range(1, len(mixed)))
    plans = {"uniform fp16": ("fp16", None), "uniform bf16": ("bf16", None), f"bf16 in blocks {moved}, fp16 in {len(mixed) - len(moved)}": ("fp16", mixed)}
    steps = {}
    for name, (dtype, formats) in plans.items():
        with _init.skip_init():
            m = DiffusionTransformer(**base)
        m.load_state_dict(sd)
        m = m.to(dev).eval().set_gemm_dtype(dtype).set_block_gemm_dtypes(formats)
        m.prepare_generation(c, g, 7.0)
        steps[name] = (lambda m=m: m.denoise(x, 1.0, cfg_scale=7.0))
        for _ in range(a.warmup):
            steps[name]()
    per = {name: [] for name in steps}
    for _ in range(a.reps):
        for name, fn in steps.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.window):
                fn()
            e1.record()
            e1.synchronize()
            per[name].append(e0.elapsed_time(e1) / a.window)
    rows = [f"dit step, T {a.t_len}, one prompt CFG 7, {a.reps} alternating windows of {a.window} steps; {boundaries} format boundaries in the mixed plan"]
    for name, v in per.items():
        rows.append(f"  {name:44s} {statistics.median(v):8.3f} ms  (min {min(v):.3f}, max {max(v):.3f})")
    f16, mix = statistics.median(per["uniform fp16"]), statistics.median(list(per.values())[2])
    rows.append(f"  mixed - uniform fp16: {1e3 * (mix - f16):+.1f} us per step, {1e3 * (mix - f16) / max(boundaries, 1):+.1f} us per boundary")
    print("\n".join(rows), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    main()
