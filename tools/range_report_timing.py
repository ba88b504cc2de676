"""What the fp16 range reports cost, and that they cost nothing when off.

    --what dit     one sampler step (`denoise` = one sat_dit_denoise_cfg call) of the full-size DiT (24 blocks, D 1536), T = 1024, one prompt
                   with CFG 7, with activation_range_report off and on
    --what codec   a 1024-frame decode of the full-size Oobleck decoder with the report off and on (on: every ResidualUnit as two launches),
                   and whether the two routes give the same bits

--lib PATH times another build of the library instead of lib/libsat_hip.so -- the parent commit's, say, on the same box in the same job:
entry points that build lacks are dropped from the binding table, and the "on" rows are skipped when the report is among them.

Windows of --window back-to-back calls between one pair of device events, median / min / max over --reps windows after --warmup.  Synthetic
weights and inputs (the time does not depend on the values).  Needs a HIP device; --out appends.

    python tools/range_report_timing.py --what dit --out profiles/range_report_timing.txt
"""
import argparse
import ctypes
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


def _use_library(path):
    """Binds `path` instead of the tree's library; returns whether it has the range reports."""
    from stable_audio_tools import _hip
    _hip.LIB_PATH = os.path.abspath(path)
    handle = ctypes.CDLL(_hip.LIB_PATH)
    missing = [n for n in _hip._SIGNATURES if not hasattr(handle, n)]
    for n in missing:
        del _hip._SIGNATURES[n]
    print(f"library {_hip.LIB_PATH}: {len(missing)} entry points of this tree's table are not in it {missing[:4]}", flush=True)
    return "sat_dit_range_report" not in missing


def dit_rows(a, dev, has_report, tag):
    from stable_audio_tools import model_configs as MC, synthetic
    from stable_audio_tools.models import _init
    from stable_audio_tools.models.dit import DiffusionTransformer
    base = MC.stable_audio_open_1_0()["model"]["diffusion"]["config"]
    x = synthetic.synth_input("x", (1, 64, a.t_len), 1).to(dev)
    c = synthetic.synth_input("c", (1, 130, base["cond_token_dim"]), 2).to(dev)
    g = synthetic.synth_input("g", (1, base["global_cond_dim"]), 3).to(dev)
    with _init.skip_init():
        m = DiffusionTransformer(**base)
    m.load_state_dict(synthetic.synth_state_dict(m.state_dict(), 0))
    m = m.to(dev).eval()
    if a.dtype:
        m.set_gemm_dtype(a.dtype)
    m.prepare_generation(c, g, 7.0)
    step = lambda: m.denoise(x, 1.0, cfg_scale=7.0)
    rows = []
    off = _windows(step, a)
    rows.append(f"dit step   {tag:28s} report off  {off[0]:8.3f} ms  (min {off[1]:.3f}, max {off[2]:.3f})")
    print(rows[-1], flush=True)
    if has_report:
        out_off = step().clone()
        m.activation_range_report(True)
        on = _windows(step, a)
        same = torch.equal(step(), out_off)
        table = m.activation_range_report(False)
        launches = sum(1 for r in table if r["launches"])
        rows.append(f"dit step   {tag:28s} report on   {on[0]:8.3f} ms  (min {on[1]:.3f}, max {on[2]:.3f})   {100 * (on[0] / off[0] - 1):+.2f} %, "
                    f"{launches} of {len(table)} slots written per step, output bit-identical to off: {same}")
        print(rows[-1], flush=True)
        again = _windows(step, a)
        rows.append(f"dit step   {tag:28s} off again   {again[0]:8.3f} ms  (min {again[1]:.3f}, max {again[2]:.3f})")
        print(rows[-1], flush=True)
    return rows


def codec_rows(a, dev, has_report, tag):
    import cases
    from stable_audio_tools import synthetic
    from stable_audio_tools.models import _init
    from stable_audio_tools.models.autoencoders import OobleckDecoder
    with _init.skip_init():
        dec = OobleckDecoder(**cases.vae_kwargs(cases.FULL_VAE, True))
    dec.load_state_dict(synthetic.synth_state_dict(dec.state_dict(), 0))
    dec = dec.to(dev).eval()
    z = synthetic.synth_input("z_full", (1, 64, a.frames), 1).to(dev)
    rows = []
    for fmt in ("fp16", "bf16"):
        dec.set_gemm_dtype(fmt)
        run = lambda: dec(z)
        off = _windows(run, a)
        rows.append(f"codec decode {a.frames} frames {fmt} {tag:20s} report off  {off[0]:8.3f} ms  (min {off[1]:.3f}, max {off[2]:.3f})")
        print(rows[-1], flush=True)
        if not has_report:
            continue
        out_off = run().clone()
        dec.activation_range_report(True)
        on = _windows(run, a)
        same = torch.equal(run(), out_off)
        diff = (run() - out_off).abs().max().item() / out_off.abs().max().item()
        table = dec.activation_range_report(False)
        rows.append(f"codec decode {a.frames} frames {fmt} {tag:20s} report on   {on[0]:8.3f} ms  (min {on[1]:.3f}, max {on[2]:.3f})   {100 * (on[0] / off[0] - 1):+.2f} %, "
                    f"{len(table)} records; two-launch ResidualUnits bit-equal to the fused route: {same} (max |diff| / max |audio| {diff:.2e})")
        print(rows[-1], flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=("dit", "codec"), required=True)
    ap.add_argument("--lib", default=None, help="another build of libsat_hip.so to time instead of the tree's")
    ap.add_argument("--tag", default=None, help="label of the rows (default: 'this tree' / the --lib path)")
    ap.add_argument("--t-len", type=int, default=1024)
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--window", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--dtype", default=None, help="gemm_dtype of the DiT rows (default: the package default)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    has_report = _use_library(a.lib) if a.lib else True
    tag = a.tag or (a.lib if a.lib else "this tree")
    dev = torch.device("cuda:0")
    lines = dit_rows(a, dev, has_report, tag) if a.what == "dit" else codec_rows(a, dev, has_report, tag)
    if a.out:
        with open(a.out, "a") as f:
            f.write(f"# {torch.cuda.get_device_name(0)}; {a.window} calls per event pair, median of {a.reps} windows after {a.warmup} warm-up calls\n")
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
