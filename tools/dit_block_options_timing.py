"""What the TransformerBlock options cost: (1) the conformer's depthwise-conv + mid_norm + SiLU kernel at the full-size shape, two sequences
of S = 1025 rows of D = 1536 (M = 2050), in the four designs of sat_dwconv_ln_silu_* -- variant 0, the one the plan runs (16-row tile and
its 16 halo rows in registers), variant 1 (one output row per workgroup: every input row is read 17 times, out of L2), variant 2 (32-row
tile staged in LDS) and variant 3 (the plan's design on an 8-row tile) -- beside the 4 M D bytes the pass has to move; (2) one sampler step (`denoise` = one sat_dit_denoise_cfg call) of the
full-depth DiT (24 blocks, D 1536) at T = 1024, one prompt with CFG 7, as shipped and with each of conformer / glu=False / remove_norms.

Windows of --window back-to-back launches / steps between one pair of device events, median / min / max over --reps windows after --warmup.
Synthetic weights and random operands (the time does not depend on the values).  Needs a HIP device.

    python tools/dit_block_options_timing.py --out profiles/dit_block_options_timing.txt
"""
import argparse

import torch

import dit_step_timing as ST          # (puts the package on sys.path)


def dwconv_rows(a, dev):
    from stable_audio_tools import _hip
    lib = _hip.lib()
    b, s, d = 2, 1025, 1536
    gen = torch.Generator().manual_seed(5)
    w = (torch.randn((d, 17), generator=gen) * 0.3).to(dev)
    gamma, beta = (0.5 + torch.rand((d,), generator=gen)).to(dev), (torch.randn((d,), generator=gen) * 0.3).to(dev)
    nbytes = 4.0 * b * s * d
    rows = []
    for sfx, dtype in (("f16", torch.float16), ("bf16", torch.bfloat16)):
        x = torch.randn((b * s, d), generator=gen).to(dtype).to(dev)
        y = torch.empty_like(x)
        fn = getattr(lib, f"sat_dwconv_ln_silu_{sfx}")
        for variant, name in ((0, "16-row tile + halo in registers (the plan's)"), (1, "one row per workgroup (17 reads out of L2)"), (2, "32-row tile + halo staged in LDS"),
                              (3, "8-row tile + halo in registers")):
            call = lambda: _hip.check(fn(_hip.ptr(x), _hip.ptr(w), _hip.ptr(gamma), _hip.ptr(beta), _hip.ptr(y), b, s, d, variant, _hip.stream()))
            med, lo, hi = ST.windows(call, a)
            rows.append(f"dwconv_ln_silu {sfx:4s} M {b * s} D {d}  {name:46s} {1e3 * med:7.1f} us / launch  (min {1e3 * lo:.1f}, max {1e3 * hi:.1f})   "
                        f"{nbytes / med / 1e6:7.1f} GB/s of the {nbytes / 1e6:.1f} MB it has to move")
            print(rows[-1], flush=True)
    return rows


def step_rows(a, dev):
    rows, ref = [], None
    for name, extra in (("as shipped", {}), ("conformer=True", dict(conformer=True)), ('ff_kwargs={"glu": False}', dict(ff_kwargs={"glu": False})),
                        ("remove_norms=True", dict(remove_norms=True))):
        med, lo, hi = ST.step_windows(dev, a, extra, dict(allow_block_options=True))
        ref = med if ref is None else ref
        rows.append(f"step  {name:26s} {med:8.3f} ms  (min {lo:.3f}, max {hi:.3f})   {1e3 * (med - ref):+8.1f} us vs as shipped ({100 * (med / ref - 1):+.2f} %)")
        print(rows[-1], flush=True)
    return rows


def main():
    a = ST.add_common_args(argparse.ArgumentParser()).parse_args()
    dev = torch.device("cuda:0")
    lines = dwconv_rows(a, dev) + step_rows(a, dev)
    head = (f"TransformerBlock options, cost: {torch.cuda.get_device_name(0)}; {a.window} launches / steps per event pair, median of {a.reps} windows; step rows: "
            f"full-depth DiT (24 blocks, D 1536), T = {a.t_len}, one prompt, CFG 7 (2 sequences), gemm_dtype {a.dtype or 'package default'}\n")
    ST.write_report(a.out, head, lines)


if __name__ == "__main__":
    main()
