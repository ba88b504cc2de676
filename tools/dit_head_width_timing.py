"""What 32- and 96-channel attention heads cost: (1) the attention kernel of csrc/attention_hdw.hip beside the 64-channel one at the same FLOPs
and bytes -- two sequences of S = 1025 at D 1536: H = 48 heads of 32 and H = 16 heads of 96 against H = 24 heads of 64; (2) one sampler step
(`denoise` = one sat_dit_denoise_cfg call) of the full-depth embed_dim 1536 DiT with num_heads 48 and 16 (allow_head_widths) at T = 1024, one
prompt with CFG 7, beside the shipped 24-head model with set_layernorm_fusion(False).set_cross_attention_fusion(False) -- the like-for-like
route: what is left is the fp32 round trip and the two extra launches per attention of the staged route -- and beside the shipped model as it
runs by default.  Recorded, not gated.

Windows of --window back-to-back launches / steps between one pair of device events, median / min / max over --reps windows after --warmup.
Synthetic weights and random operands (the time does not depend on the values).  Needs a HIP device.

    python tools/dit_head_width_timing.py --out profiles/dit_head_width_timing.txt
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
    s_pad = (s + 127) // 128 * 128
    rows = []
    for h, hd in ((48, 32), (16, 96), (24, 64)):
        tile = 128 if hd == 32 else 64          # the kernel's key tile: sk_pad is a multiple of it
        k_pad = (s + 3 + tile - 1) // tile * tile
        gen = torch.Generator().manual_seed(h)
        q = (torch.randn((b, h, s_pad, hd), generator=gen) * 0.2).to(dtype).to(dev)
        k = torch.randn((b, h, k_pad, hd), generator=gen).to(dtype).to(dev)
        vt = torch.randn((b, h, hd, k_pad), generator=gen).to(dtype).to(dev)
        out = torch.empty((b * s, h * hd), dtype=dtype, device=dev)
        if hd == 64:
            fn = getattr(lib, f"sat_attention_prescaled_{sfx}")
            call = lambda: _hip.check(fn(_hip.ptr(q), _hip.ptr(k), _hip.ptr(vt), _hip.ptr(out), b, h, h, s, s, s_pad, k_pad, _hip.stream()))
        else:
            fn = getattr(lib, f"sat_attention_hdw_{sfx}")
            call = lambda: _hip.check(fn(_hip.ptr(q), _hip.ptr(k), _hip.ptr(vt), _hip.ptr(out), b, h, h, hd, s, s, s_pad, k_pad, _hip.stream()))
        med, lo, hi = ST.windows(call, a)
        flops = 4.0 * b * h * s * s * hd
        rows.append(f"attention {sfx}  hd{hd:<3d} H {h:2d} (D 1536)  2 x S 1025: {1e3 * med:8.1f} us / launch  (min {1e3 * lo:.1f}, max {1e3 * hi:.1f})   "
                    f"{flops / med / 1e9:7.1f} TFLOP/s")
        print(rows[-1], flush=True)
    return rows


def step_rows(a, dev):
    rows, ref = [], None
    for name, heads, fused in (("24 heads of 64, fusions off (like for like)", 24, False), ("48 heads of 32 (staged route)", 48, False),
                               ("16 heads of 96 (staged route)", 16, False), ("24 heads of 64 as shipped (fold + fused cross)", 24, True)):
        med, lo, hi = ST.step_windows(dev, a, dict(num_heads=heads), product_kwargs=dict(allow_head_widths=True),
                                      before_plan=lambda m: m.set_layernorm_fusion(fused).set_cross_attention_fusion(fused))
        ref = med if ref is None else ref
        rows.append(f"step  {name:48s} {med:8.3f} ms  (min {lo:.3f}, max {hi:.3f})   {1e3 * (med - ref):+8.1f} us vs like for like ({100 * (med / ref - 1):+.2f} %)")
        print(rows[-1], flush=True)
    return rows


def main():
    a = ST.add_common_args(argparse.ArgumentParser()).parse_args()
    dev = torch.device("cuda:0")
    lines = attention_rows(a, dev, True) + attention_rows(a, dev, False) + step_rows(a, dev)
    head = (f"32- and 96-channel heads, cost: {torch.cuda.get_device_name(0)}; {a.window} launches / steps per event pair, median of {a.reps} windows; step "
            f"rows: full-depth DiT (24 blocks, D 1536), T = {a.t_len}, one prompt, CFG 7 (2 sequences), gemm_dtype {a.dtype or 'package default'}\n")
    ST.write_report(a.out, head, lines)


if __name__ == "__main__":
    main()
