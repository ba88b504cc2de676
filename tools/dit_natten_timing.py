"""What the neighbourhood window saves: (1) the window launch of csrc/attention_window.hip beside the full-attention launch of
csrc/attention.hip -- the unchanged kernel, the yardstick -- on the SAME tensors: 24 heads of 64, fp16, pre-scaled Q, two sequences of
S = 1025 (one prompt with CFG) and one of S = 6145, kernel sizes 63, 255 and 1023; the launches are timed alternately, window by window, in
one process.  (2) one sampler step (`denoise` = one sat_dit_denoise_cfg call) of the full-depth embed_dim 1536 DiT without cross-attention,
with 4 prepend tokens (so that CFG 7 runs two sequences), natten_kernel_size 255 (allow_natten) beside the same model with full attention.
Recorded, not gated.

Windows of --window back-to-back launches / steps between one pair of device events, median / min / max over --reps windows after --warmup.
Synthetic weights and random operands (the time does not depend on the values).  Needs a HIP device.

    python tools/dit_natten_timing.py --out profiles/dit_natten_timing.txt
"""
import argparse

import torch

import dit_step_timing as ST          # (puts the package on sys.path)
from dit_causal_timing import ATTENTION_WINDOWS, alternating

KERNEL_SIZES = (63, 255, 1023)
STEP_KERNEL = 255


def attention_rows(a, dev):
    from stable_audio_tools import _hip
    lib = _hip.lib()
    h, hd, rows = 24, 64, []
    for b, s in ((2, 1025), (1, 6145)):
        s_pad = (s + 127) // 128 * 128          # (>= s + 3 and a multiple of the 64-key tile as well)
        gen = torch.Generator().manual_seed(s)
        q = (torch.randn((b, h, s_pad, hd), generator=gen) * 0.2).to(torch.float16).to(dev)
        k = torch.randn((b, h, s_pad, hd), generator=gen).to(torch.float16).to(dev)
        vt = torch.randn((b, h, hd, s_pad), generator=gen).to(torch.float16).to(dev)
        out = torch.empty((b * s, h * hd), dtype=torch.float16, device=dev)
        p = [_hip.ptr(t) for t in (q, k, vt, out)]
        calls = {"full": lambda: _hip.check(lib.sat_attention_prescaled_f16(*p, b, h, h, s, s, s_pad, s_pad, _hip.stream()))}
        for ks in KERNEL_SIZES:          # (score_scale ln 2: times log2(e) in the entry point, the 1.0 the plan launches with)
            calls[f"K {ks}"] = lambda ks=ks: _hip.check(lib.sat_attention_window_f16(*p, b, h, h, s, s_pad, s_pad, ks, 0.6931471805599453, _hip.stream()))
        res = alternating(calls, a, scale=ATTENTION_WINDOWS)
        ref = res["full"][0]
        for name, (med, lo, hi) in res.items():
            rows.append(f"attention f16  hd64 H 24  {b} x S {s:4d}  {name:7s}: {1e3 * med:8.1f} us / launch  (min {1e3 * lo:.1f}, max {1e3 * hi:.1f})   "
                        f"{med / ref:5.2f} x the full launch")
            print(rows[-1], flush=True)
    return rows


def step_rows(a, dev):
    from stable_audio_tools import model_configs as MC, synthetic
    from stable_audio_tools.models import _init
    from stable_audio_tools.models.dit import DiffusionTransformer
    base = dict(MC.stable_audio_open_1_0()["model"]["diffusion"]["config"], cond_token_dim=0, prepend_cond_dim=48)
    x = synthetic.synth_input("x", (1, 64, a.t_len), 1).to(dev)
    g = synthetic.synth_input("g", (1, base["global_cond_dim"]), 3).to(dev)
    pre = synthetic.synth_input("prepend", (1, 4, 48), 4).to(dev)
    calls = {}
    for name, ks in (("full attention", None), (f"natten_kernel_size={STEP_KERNEL}", STEP_KERNEL)):
        with _init.skip_init():
            m = DiffusionTransformer(**dict(base, attn_kwargs={"natten_kernel_size": ks}), allow_natten=True)
        m.load_state_dict(synthetic.synth_state_dict(m.state_dict(), 0))
        m = m.to(dev).eval()
        if a.dtype:
            m.set_gemm_dtype(a.dtype)
        m.prepare_generation(None, g, 7.0, prepend_cond=pre)          # (each model has its own plan and context)
        calls[name] = lambda m=m: m.denoise(x, 1.0, cfg_scale=7.0)
    res = alternating(calls, a)
    ref = res["full attention"][0]
    rows = []
    for name, (med, lo, hi) in res.items():
        rows.append(f"step  prepend-only DiT, {name:22s} {med:8.3f} ms  (min {lo:.3f}, max {hi:.3f})   {1e3 * (med - ref):+8.1f} us vs full attention "
                    f"({100 * (med / ref - 1):+.2f} %)")
        print(rows[-1], flush=True)
    return rows


def main():
    a = ST.add_common_args(argparse.ArgumentParser()).parse_args()
    dev = torch.device("cuda:0")
    lines = attention_rows(a, dev) + step_rows(a, dev)
    head = (f"neighbourhood self-attention, cost: {torch.cuda.get_device_name(0)}; {ATTENTION_WINDOWS * a.window} launches / {a.window} steps per event pair, the variants in turn, "
            f"median of {a.reps} windows; step rows: full-depth DiT (24 blocks, D 1536) without cross-attention, 4 prepend tokens, T = {a.t_len}, CFG 7 "
            f"(2 sequences), gemm_dtype {a.dtype or 'package default'}\n")
    ST.write_report(a.out, head, lines)


if __name__ == "__main__":
    main()
