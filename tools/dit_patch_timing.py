"""What a patchified DiT (patch_size P, sat_dit_plan_set_patch) costs and saves: (1) the two boundary kernels alone at the full-size shape --
two sequences (one prompt with CFG), 64 latent channels, T = --t-len frames, D = 1536 -- the P = 1 kernels of dit_glue.hip (sat_input_proj,
sat_output_proj) beside the patch kernels of dit_patch.hip (sat_input_proj_patch, sat_output_proj_patch) at P = 2 and 4, on "prepend" rows
(S = 1 + T / P); (2) one sampler step (`denoise` = one sat_dit_denoise_cfg call) of the full-depth SA-Open-shape DiT (24 blocks, D 1536) at
P = 1 (what the parent commit runs), 2 and 4, one prompt with CFG 7.

Windows of --window back-to-back launches / steps between one pair of device events, median / min / max over --reps windows after --warmup.
Synthetic weights and random operands (the time does not depend on the values).  Needs a HIP device.

    python tools/dit_patch_timing.py --out profiles/dit_patch_timing.txt
"""
import argparse
import gc
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "friendly-stable-audio-tools_amd"))


def _windows(fn, a):
    for _ in range(a.warmup):
        fn()
    per = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.window):
            fn()
        e1.record()
        e1.synchronize()
        per.append(e0.elapsed_time(e1) / a.window)
    return statistics.median(per), min(per), max(per)


def kernel_rows(a, dev):
    from stable_audio_tools import _hip
    lib = _hip.lib()
    bf, xb, c, t, d = 2, 1, 64, a.t_len, 1536
    gen = torch.Generator().manual_seed(5)
    x = torch.randn((xb, c, t), generator=gen).to(dev)
    out = torch.empty((bf, c, t), device=dev)
    rows, ref = [], {}
    for P in (1, 2, 4):
        s = 1 + t // P
        X = torch.randn((bf, s, d), generator=gen).to(dev)
        w_in = (torch.randn((c * P, d), generator=gen) * 0.1).to(dev)
        w_out = (torch.randn((d, c * P), generator=gen) * 0.1).to(dev)
        if P == 1:
            fin = lambda: _hip.check(lib.sat_input_proj(_hip.ptr(x), _hip.ptr(w_in), _hip.ptr(X), bf, xb, c, t, s, d, 0.5, _hip.stream()))
            fout = lambda: _hip.check(lib.sat_output_proj(_hip.ptr(X), _hip.ptr(w_out), _hip.ptr(out), bf, c, t, s, d, _hip.stream()))
        else:
            fin = lambda: _hip.check(lib.sat_input_proj_patch(_hip.ptr(x), _hip.ptr(w_in), _hip.ptr(X), bf, xb, c, P, t, s, d, 0.5, None, 0, 0, None, 0,
                                                              _hip.stream()))
            fout = lambda: _hip.check(lib.sat_output_proj_patch(_hip.ptr(X), _hip.ptr(w_out), _hip.ptr(out), bf, c, P, t, s, d, _hip.stream()))
        for what, fn in (("input projection", fin), ("output projection", fout)):
            med, lo, hi = _windows(fn, a)
            ref.setdefault(what, med)
            rows.append(f"{what:18s} P {P}  {t // P:5d} tokens x {bf} sequences, {c * P:4d} features, D {d}   {1e3 * med:7.1f} us / launch  "
                        f"(min {1e3 * lo:.1f}, max {1e3 * hi:.1f})   {med / ref[what]:.2f} x the P = 1 kernel")
            print(rows[-1], flush=True)
    return rows


def step_rows(a, dev):
    from stable_audio_tools import model_configs as MC, synthetic
    from stable_audio_tools.models import _init
    from stable_audio_tools.models.dit import DiffusionTransformer
    full = MC.stable_audio_open_1_0()["model"]["diffusion"]["config"]
    t_len, lc = a.t_len, 130
    x = synthetic.synth_input("x", (1, 64, t_len), 1).to(dev)
    c = synthetic.synth_input("c", (1, lc, full["cond_token_dim"]), 2).to(dev)
    g = synthetic.synth_input("g", (1, full["global_cond_dim"]), 3).to(dev)
    rows, ref = [], None
    for P in (1, 2, 4):
        with _init.skip_init():
            m = DiffusionTransformer(**dict(full, patch_size=P), allow_patch_size=True)
        m.load_state_dict(synthetic.synth_state_dict(m.state_dict(), 0))
        m = m.to(dev).eval()
        if a.dtype:
            m.set_gemm_dtype(a.dtype)
        m.prepare_generation(c, g, 7.0)
        med, lo, hi = _windows(lambda: m.denoise(x, 1.0, cfg_scale=7.0), a)
        ref = ref or med
        rows.append(f"step  full-depth DiT (24 blocks, D 1536)  T {t_len:5d}  patch_size {P}  ({1 + t_len // P:4d} rows per sequence)  {med:8.3f} ms  "
                    f"(min {lo:.3f}, max {hi:.3f})   {med / ref:.2f} x the P = 1 step")
        print(rows[-1], flush=True)
        del m
        gc.collect()
        torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--t-len", type=int, default=1024)
    ap.add_argument("--window", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--dtype", default=None, help="gemm_dtype of the step rows (default: the package default)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = kernel_rows(a, dev) + step_rows(a, dev)
    head = (f"Patchified DiT, cost: {torch.cuda.get_device_name(0)}; {a.window} launches / steps per event pair, median of {a.reps} windows; "
            f"step rows: one prompt, CFG 7 (2 sequences), gemm_dtype {a.dtype or 'package default'}\n")
    if a.out:
        with open(a.out, "w") as f:
            f.write(head + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
