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

import torch

import dit_step_timing as ST          # (puts the package on sys.path)


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
            med, lo, hi = ST.windows(fn, a)
            ref.setdefault(what, med)
            rows.append(f"{what:18s} P {P}  {t // P:5d} tokens x {bf} sequences, {c * P:4d} features, D {d}   {1e3 * med:7.1f} us / launch  "
                        f"(min {1e3 * lo:.1f}, max {1e3 * hi:.1f})   {med / ref[what]:.2f} x the P = 1 kernel")
            print(rows[-1], flush=True)
    return rows


def step_rows(a, dev):
    t_len = a.t_len
    rows, ref = [], None
    for P in (1, 2, 4):
        med, lo, hi = ST.step_windows(dev, a, dict(patch_size=P), dict(allow_patch_size=True))
        ref = ref or med
        rows.append(f"step  full-depth DiT (24 blocks, D 1536)  T {t_len:5d}  patch_size {P}  ({1 + t_len // P:4d} rows per sequence)  {med:8.3f} ms  "
                    f"(min {lo:.3f}, max {hi:.3f})   {med / ref:.2f} x the P = 1 step")
        print(rows[-1], flush=True)
    return rows


def main():
    a = ST.add_common_args(argparse.ArgumentParser()).parse_args()
    dev = torch.device("cuda:0")
    lines = kernel_rows(a, dev) + step_rows(a, dev)
    head = (f"Patchified DiT, cost: {torch.cuda.get_device_name(0)}; {a.window} launches / steps per event pair, median of {a.reps} windows; "
            f"step rows: one prompt, CFG 7 (2 sequences), gemm_dtype {a.dtype or 'package default'}\n")
    ST.write_report(a.out, head, lines)


if __name__ == "__main__":
    main()
