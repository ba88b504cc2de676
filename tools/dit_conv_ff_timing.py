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
import gc
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "friendly-stable-audio-tools_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))


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
        med, lo, hi = _windows(lin, a)
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
            med, lo, hi = _windows(lambda: call(None), a)
            rows.append(f"FF-out {sfx:4s} M {m} N {n} K {k}  convolution GEMM k = {taps}, weight packed once          {1e3 * med:8.1f} us / launch  (min {1e3 * lo:.1f}, max {1e3 * hi:.1f})   "
                        f"{2.0 * m * n * k * taps / med / 1e9:7.1f} TFLOP/s, {med / ref:.2f} x the Linear")
            print(rows[-1], flush=True)
    return rows


def step_rows(a, dev):
    import cases
    from stable_audio_tools import model_configs as MC, synthetic
    from stable_audio_tools.models import _init
    from stable_audio_tools.models.dit import DiffusionTransformer
    full = MC.stable_audio_open_1_0()["model"]["diffusion"]["config"]
    rows = []
    for label, base, t_len, lc in (("reduced DiT (3 blocks, D 256)", dict(cases.SMALL_DIT), 64, 130), ("full-depth DiT (24 blocks, D 1536)", full, a.t_len, 130)):
        x = synthetic.synth_input("x", (1, 64, t_len), 1).to(dev)
        c = synthetic.synth_input("c", (1, lc, base["cond_token_dim"]), 2).to(dev)
        g = synthetic.synth_input("g", (1, base["global_cond_dim"]), 3).to(dev)
        ref = {}
        for name, ff in (("Linear, glu (as shipped)", {}), ("use_conv k 3, glu", dict(use_conv=True)), ("Linear, glu=False", dict(glu=False)),
                         ("use_conv k 3, glu=False", dict(use_conv=True, glu=False))):
            with _init.skip_init():
                m = DiffusionTransformer(**dict(base, ff_kwargs=ff), allow_block_options=True, allow_conv_ff=True)
            m.load_state_dict(synthetic.synth_state_dict(m.state_dict(), 0))
            m = m.to(dev).eval()
            if a.dtype:
                m.set_gemm_dtype(a.dtype)
            m.prepare_generation(c, g, 7.0)
            med, lo, hi = _windows(lambda: m.denoise(x, 1.0, cfg_scale=7.0), a)
            glu = ff.get("glu", True)
            ref.setdefault(glu, med)
            rows.append(f"step  {label:36s} T {t_len:5d}  {name:26s} {med:8.3f} ms  (min {lo:.3f}, max {hi:.3f})   "
                        f"{1e3 * (med - ref[glu]):+9.1f} us vs the Linear model ({100 * (med / ref[glu] - 1):+.1f} %)")
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
    lines = gemm_rows(a, dev) + step_rows(a, dev)
    head = (f"Convolutional feed-forward, cost: {torch.cuda.get_device_name(0)}; {a.window} launches / steps per event pair, median of {a.reps} windows; "
            f"step rows: one prompt, CFG 7 (2 sequences), gemm_dtype {a.dtype or 'package default'}\n")
    if a.out:
        with open(a.out, "w") as f:
            f.write(head + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
