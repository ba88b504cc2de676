"""What the neighbourhood window saves at 128-, 32- and 96-channel heads: per width, the K = 255 window launch of
csrc/attention_hdw_window.hip beside the full-attention launch of csrc/attention_hdw.hip -- the unchanged kernel, the yardstick -- on the SAME
tensors: D 1536 in heads of that width (12 x 128, 48 x 32, 16 x 96), fp16, pre-scaled Q, two sequences of S = 1025 (one prompt with CFG) and
one of S = 6145; the two launches are timed alternately, window by window, in one process.  Beside each row the key tiles the launch walks,
summed over the workgroups of one (sequence, head), as csrc/attn_window.h predicts them (first_tile .. last_tile per 256-query workgroup at
the key tile of the width) against the tiles of the full walk.  Recorded, not gated.

Windows of --window back-to-back launches between one pair of device events, median / min / max over --reps windows after --warmup.  Random
operands (the time does not depend on the values).  Needs a HIP device.

    python tools/dit_natten_hdw_timing.py --out profiles/dit_natten_hdw_timing.txt
"""
import argparse

import torch

import dit_step_timing as ST          # (puts the package on sys.path)
from dit_causal_timing import ATTENTION_WINDOWS, alternating

KERNEL = 255
WIDTHS = {128: 12, 32: 48, 96: 16}          # head width -> heads of D 1536
KEY_TILE = {128: 64, 32: 128, 96: 64}       # csrc/attn_hdw_tiles.h


def tiles_walked(s, ks, kt, ob=0, qb=256):
    """(tiles the window launch walks, tiles the full launch walks), summed over the workgroups of one (sequence, head): csrc/attn_window.h"""
    start = lambda i: min(max(min(i, s - 1) - ks // 2, 0), s - ks)
    walked = full = 0
    for q0 in range(0, s, qb):
        q1 = min(q0 + qb - 1, s - 1)
        walked += (ob + start(q1) + ks - 1) // kt - (ob + start(q0)) // kt + 1
        full += (ob + s + kt - 1) // kt
    return walked, full


def attention_rows(a, dev):
    from stable_audio_tools import _hip
    lib = _hip.lib()
    rows = []
    for w, h in WIDTHS.items():
        for b, s in ((2, 1025), (1, 6145)):
            s_pad = (s + 127) // 128 * 128          # (>= s + 3 and a multiple of both key tiles)
            gen = torch.Generator().manual_seed(s + w)
            q = (torch.randn((b, h, s_pad, w), generator=gen) * 0.2).to(torch.float16).to(dev)
            k = torch.randn((b, h, s_pad, w), generator=gen).to(torch.float16).to(dev)
            vt = torch.randn((b, h, w, s_pad), generator=gen).to(torch.float16).to(dev)
            out = torch.empty((b * s, h * w), dtype=torch.float16, device=dev)
            p = [_hip.ptr(t) for t in (q, k, vt, out)]
            # (the unit entry of the full launch at 128 channels is older than the one that takes a width: the same launcher behind both)
            full = ((lambda: lib.sat_attention_hd128_f16(*p, b, h, h, s, s, s_pad, s_pad, _hip.stream())) if w == 128 else
                    (lambda: lib.sat_attention_hdw_f16(*p, b, h, h, w, s, s, s_pad, s_pad, _hip.stream())))
            calls = {"full": lambda: _hip.check(full()),
                     f"K {KERNEL}": lambda: _hip.check(lib.sat_attention_hdw_window_f16(*p, b, h, h, w, s, s_pad, s_pad, KERNEL, _hip.stream()))}
            res = alternating(calls, a, scale=ATTENTION_WINDOWS)
            ref = res["full"][0]
            walked, full = tiles_walked(s, KERNEL, KEY_TILE[w])
            for name, (med, lo, hi) in res.items():
                tiles = full if name == "full" else walked
                rows.append(f"attention f16  hd{w:<3d} H {h:2d}  {b} x S {s:4d}  {name:5s}: {1e3 * med:8.1f} us / launch  (min {1e3 * lo:.1f}, max {1e3 * hi:.1f})   "
                            f"{med / ref:5.2f} x the full launch   {tiles:4d} of {full} {KEY_TILE[w]}-key tiles per (sequence, head)")
                print(rows[-1], flush=True)
    return rows


def main():
    a = ST.add_common_args(argparse.ArgumentParser()).parse_args()
    dev = torch.device("cuda:0")
    lines = attention_rows(a, dev)
    head = (f"neighbourhood self-attention at 128-, 32- and 96-channel heads, cost: {torch.cuda.get_device_name(0)}; {ATTENTION_WINDOWS * a.window} "
            f"launches per event pair, the two launches in turn, median of {a.reps} windows\n")
    ST.write_report(a.out, head, lines)


if __name__ == "__main__":
    main()
