"""What 128-channel attention heads cost: (1) the attention kernel of csrc/attention_hdw.hip at W = 128 beside the 64-channel one at the same FLOPs and
bytes -- two sequences of S = 1025, H = 12 heads of 128 against H = 24 heads of 64 (D 1536), and H = 8 heads of 128 (D 1024); (2) one
sampler step (`denoise` = one sat_dit_denoise_cfg call) of a full-depth embed_dim 1536 / num_heads 12 DiT at T = 1024, one prompt with CFG 7,
beside the shipped 24-head model with set_layernorm_fusion(False).set_cross_attention_fusion(False) -- the like-for-like route: what is left
is the fp32 round trip and the two extra launches per attention of the staged route -- and beside the shipped model as it runs by default.

Windows of --window back-to-back launches / steps between one pair of device events, median / min / max over --reps windows after --warmup.
Synthetic weights and random operands (the time does not depend on the values).  Needs a HIP device.

    python tools/dit_head_dim_timing.py --out profiles/dit_head_dim_timing.txt
"""
import argparse

import torch

import dit_step_timing as ST          # (puts the package on sys.path)


def attention_rows(a, dev, f16):
    from stable_audio_tools import _hip
    lib = _hip.lib()
    dtype = torch.float16 if f16 else torch.bfloat16
    sfx = "f16" if f16 else "bf16"
    b, s = 2, 1025
    s_pad, k_pad = (s + 127) // 128 * 128, (s + 3 + 63) // 64 * 64
    rows = []
    for name, fn_name, h, hd in ((f"hd128  H 12 (D 1536)", f"sat_attention_hd128_{sfx}", 12, 128),
                                 (f"hd64   H 24 (D 1536)", f"sat_attention_prescaled_{sfx}", 24, 64),
                                 (f"hd128  H  8 (D 1024)", f"sat_attention_hd128_{sfx}", 8, 128)):
        gen = torch.Generator().manual_seed(h)
        q = (torch.randn((b, h, s_pad, hd), generator=gen) * 0.2).to(dtype).to(dev)
        k = torch.randn((b, h, k_pad, hd), generator=gen).to(dtype).to(dev)
        vt = torch.randn((b, h, hd, k_pad), generator=gen).to(dtype).to(dev)
        out = torch.empty((b * s, h * hd), dtype=dtype, device=dev)
        fn = getattr(lib, fn_name)
        call = lambda: _hip.check(fn(_hip.ptr(q), _hip.ptr(k), _hip.ptr(vt), _hip.ptr(out), b, h, h, s, s, s_pad, k_pad, _hip.stream()))
        med, lo, hi = ST.windows(call, a)
        flops = 4.0 * b * h * s * s * hd
        rows.append(f"attention {sfx}  {name}  2 x S 1025: {1e3 * med:8.1f} us / launch  (min {1e3 * lo:.1f}, max {1e3 * hi:.1f})   {flops / med / 1e9:7.1f} TFLOP/s")
        print(rows[-1], flush=True)
    return rows


def step_rows(a, dev):
    rows, ref = [], None
    for name, heads, fused in (("24 heads of 64, fusions off (like for like)", 24, False), ("12 heads of 128 (staged route)", 12, False),
                               ("24 heads of 64 as shipped (fold + fused cross)", 24, True)):
        med, lo, hi = ST.step_windows(dev, a, dict(num_heads=heads), before_plan=lambda m: m.set_layernorm_fusion(fused).set_cross_attention_fusion(fused))
        ref = med if ref is None else ref
        rows.append(f"step  {name:48s} {med:8.3f} ms  (min {lo:.3f}, max {hi:.3f})   {1e3 * (med - ref):+8.1f} us vs like for like ({100 * (med / ref - 1):+.2f} %)")
        print(rows[-1], flush=True)
    return rows


def main():
    a = ST.add_common_args(argparse.ArgumentParser()).parse_args()
    dev = torch.device("cuda:0")
    lines = attention_rows(a, dev, True) + attention_rows(a, dev, False) + step_rows(a, dev)
    head = (f"128-channel heads, cost: {torch.cuda.get_device_name(0)}; {a.window} launches / steps per event pair, median of {a.reps} windows; step rows: "
            f"full-depth DiT (24 blocks, D 1536), T = {a.t_len}, one prompt, CFG 7 (2 sequences), gemm_dtype {a.dtype or 'package default'}\n")
    ST.write_report(a.out, head, lines)


if __name__ == "__main__":
    main()
