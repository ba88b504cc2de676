"""What a convolutional feed-forward (ff_kwargs use_conv, sat_dit_plan_set_ff_conv) costs: (1) the convolution GEMM alone (sat_ff_conv, FF-out
epilogue) at the full-size shape M = 2050 (two sequences of S = 1025 rows), N = 1536, K = 6144, kernel sizes 1 and 3, beside the Linear
FF-out GEMM of the shipped plan (sat_gemm_f16_f32 / sat_gemm_bf16_f32, its route's own tile choice) at the same M, N, K; (2) one sampler
step (`denoise` = one sat_dit_denoise_cfg call) of the reduced DiT (3 blocks, D 256, T = 64) and of the full-depth DiT (24 blocks, D 1536,
T = --t-len), one prompt with CFG 7, with Linear feed-forwards (what the parent commit runs) and with use_conv, k = 3, under both glu settings.

Windows of --window back-to-back launches / steps between one pair of device events, median / min / max over --reps windows after --warmup.
Synthetic weights and random operands (the time does not depend on the values).  Needs a HIP device.

    python tools/dit_conv_ff_timing.py --out profiles/dit_conv_ff_timing.txt
"""
import argparse
import ctypes
import os
import sys

import torch

import dit_step_timing as ST          # (puts the package on sys.path)

sys.path.insert(0, os.path.join(ST.ROOT, "tests", "golden"))


def gemm_rows(a, dev):
    from stable_audio_tools import _hip
    lib = _hip.lib()
    b, s, n, k = 2, 1025, 1536, 6144
    m = b * s
    gen = torch.Generator().manual_seed(5)
    rows = []
    for sfx, fmt, dtype in (("f16", 3, torch.float16), ("bf16", 0, torch.bfloat16)):
        x = torch.randn((m, k), generator=gen).to(dtype).to(dev)
        c = torch.zeros((m, n), device=dev)
        bias = torch.randn((n,), generator=gen).to(dev)
        w16 = (torch.randn((n, k), generator=gen) * 0.02).to(dtype).to(dev)
        need = ctypes.c_size_t()
        _hip.check(lib.sat_gemm_f32_workspace_bytes(m, n, k, 0, ctypes.byref(need)))
        slab = torch.empty(max(need.value, 256), dtype=torch.uint8, device=dev)
        fn = getattr(lib, f"sat_gemm_{sfx}_f32_ws")
        lin = lambda: _hip.check(fn(_hip.ptr(x), _hip.ptr(w16), _hip.ptr(bias), _hip.ptr(c), m, n, k, 1, 0, _hip.ptr(slab), need.value, _hip.stream()))
        med, lo, hi = ST.windows(lin, a)
        ref = med
        rows.append(f"FF-out {sfx:4s} M {m} N {n} K {k}  Linear, the shipped plan's GEMM route          {1e3 * med:8.1f} us / launch  (min {1e3 * lo:.1f}, max {1e3 * hi:.1f})   "
                    f"{2.0 * m * n * k / med / 1e9:7.1f} TFLOP/s")
        print(rows[-1], flush=True)
        for taps in (1, 3):
            w = (torch.randn((n, k, taps), generator=gen) * 0.02).to(dev)
            _hip.check(lib.sat_ff_conv_workspace_bytes(fmt, b, s, n, k, taps, ctypes.byref(need)))
            ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
            # the plan packs the weight once, at finalize: one call with the weight leaves its image in ws, the timed calls pass none and
            # launch the convolution GEMM alone
            call = lambda wp: _hip.check(lib.sat_ff_conv(fmt, _hip.ptr(x), wp, _hip.ptr(bias), 0, _hip.ptr(c), None, b, s, n, k, taps, _hip.ptr(ws),
                                                         need.value, _hip.stream()))
            call(_hip.ptr(w))
            med, lo, hi = ST.windows(lambda: call(None), a)
            rows.append(f"FF-out {sfx:4s} M {m} N {n} K {k}  convolution GEMM k = {taps}, weight packed once          {1e3 * med:8.1f} us / launch  (min {1e3 * lo:.1f}, max {1e3 * hi:.1f})   "
                        f"{2.0 * m * n * k * taps / med / 1e9:7.1f} TFLOP/s, {med / ref:.2f} x the Linear")
            print(rows[-1], flush=True)
    return rows


def step_rows(a, dev):
    import cases
    from stable_audio_tools import model_configs as MC
    full = MC.stable_audio_open_1_0()["model"]["diffusion"]["config"]
    rows = []
    for label, base, t_len in (("reduced DiT (3 blocks, D 256)", dict(cases.SMALL_DIT), 64), ("full-depth DiT (24 blocks, D 1536)", full, a.t_len)):
        ref = {}
        for name, ff in (("Linear, glu (as shipped)", {}), ("use_conv k 3, glu", dict(use_conv=True)), ("Linear, glu=False", dict(glu=False)),
                         ("use_conv k 3, glu=False", dict(use_conv=True, glu=False))):
            med, lo, hi = ST.step_windows(dev, a, dict(ff_kwargs=ff), dict(allow_block_options=True, allow_conv_ff=True), base=base, t_len=t_len)
            glu = ff.get("glu", True)
            ref.setdefault(glu, med)
            rows.append(f"step  {label:36s} T {t_len:5d}  {name:26s} {med:8.3f} ms  (min {lo:.3f}, max {hi:.3f})   "
                        f"{1e3 * (med - ref[glu]):+9.1f} us vs the Linear model ({100 * (med / ref[glu] - 1):+.1f} %)")
            print(rows[-1], flush=True)
    return rows


def main():
    a = ST.add_common_args(argparse.ArgumentParser()).parse_args()
    dev = torch.device("cuda:0")
    lines = gemm_rows(a, dev) + step_rows(a, dev)
    head = (f"Convolutional feed-forward, cost: {torch.cuda.get_device_name(0)}; {a.window} launches / steps per event pair, median of {a.reps} windows; "
            f"step rows: one prompt, CFG 7 (2 sequences), gemm_dtype {a.dtype or 'package default'}\n")
    ST.write_report(a.out, head, lines)


if __name__ == "__main__":
    main()
