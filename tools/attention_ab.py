"""Same-box A/B of the attention kernels built from csrc/attn_core.h outside attention.hip -- attention_hdw.hip (32, 96, 128 channels, with and
without the causal mask) and the 16-bit kernel of attention_window.hip: the PARENT commit's library against this tree's, both loaded into one
process (as tools/codec_ab.py does).  Developer tool; not part of the product or the tests.

(1) Same bits: both launchers on the same device inputs at the shapes of the unit tests (b = 2, GQA h = 4 / kvh = 2, S = 63 and 573; the window
    kernel with K = 3 at both and K = 65 at S = 573), both operand formats; the output buffers must be bytewise equal.
(2) Same time: the attention rows of tools/dit_head_width_timing.py, dit_head_dim_timing.py, dit_causal_timing.py (at the wide heads) and
    dit_natten_timing.py, measured parent / branch / parent / branch.  Per row P1, P2 = the parent's two medians, spread = the larger of
    |P1 - P2| and the parent's own median-to-max window distance; both branch medians must be at most max(P1, P2) + spread.

The parent's library (git-ignored like every .so): built from a git archive of the parent, copied to tools/ab/libsat_hip_parent.so.
usage: python tools/attention_ab.py [--out file]      (AB_OLD_LIB = path of the parent's library; exit code 1 when a row fails)"""
import argparse
import os
import sys

import torch

import dit_step_timing as ST          # (puts the package on sys.path)
from codec_ab import ROOT, load_parent
from dit_causal_timing import ATTENTION_WINDOWS

from stable_audio_tools import _hip

LN2 = 0.6931471805599453          # window score scale: times log2(e) in the entry point, the 1.0 the plan launches with


def operands(b, h, kvh, hd, s, dtype, dev, seed):
    tile = 128 if hd == 32 else 64
    s_pad, k_pad = (s + 127) // 128 * 128, (s + 3 + tile - 1) // tile * tile
    gen = torch.Generator().manual_seed(seed)
    q = (torch.randn((b, h, s_pad, hd), generator=gen) * 0.2).to(dtype).to(dev)
    k = torch.randn((b, kvh, k_pad, hd), generator=gen).to(dtype).to(dev)
    vt = torch.randn((b, kvh, hd, k_pad), generator=gen).to(dtype).to(dev)
    return q, k, vt, s_pad, k_pad


def launcher(lib, kind, sfx, q, k, vt, out, b, h, kvh, hd, s, s_pad, k_pad, ks=0):
    p = [_hip.ptr(t) for t in (q, k, vt, out)]

    def check(rc):          # (the message lies in the library that set it)
        assert rc == 0, (rc, lib.sat_last_error())
    if kind == "hdw" and hd == 128:
        return lambda: check(getattr(lib, f"sat_attention_hd128_{sfx}")(*p, b, h, kvh, s, s, s_pad, k_pad, _hip.stream()))
    if kind == "hdw":
        return lambda: check(getattr(lib, f"sat_attention_hdw_{sfx}")(*p, b, h, kvh, hd, s, s, s_pad, k_pad, _hip.stream()))
    if kind == "causal":
        return lambda: check(getattr(lib, f"sat_attention_causal_{sfx}")(*p, b, h, kvh, hd, s, s_pad, k_pad, 1, _hip.stream()))
    return lambda: check(getattr(lib, f"sat_attention_window_{sfx}")(*p, b, h, kvh, s, s_pad, k_pad, ks, LN2, _hip.stream()))


def same_bits(old, new, dev):
    rows, bad = [], 0
    b, h, kvh = 2, 4, 2
    for sfx, dtype in (("f16", torch.float16), ("bf16", torch.bfloat16)):
        cases = [(kind, hd, s, 0) for kind in ("hdw", "causal") for hd in (32, 96, 128) for s in (63, 573)]
        cases += [("window", 64, 63, 3), ("window", 64, 573, 3), ("window", 64, 573, 65)]
        for kind, hd, s, ks in cases:
            q, k, vt, s_pad, k_pad = operands(b, h, kvh, hd, s, dtype, dev, 1000 * hd + s)
            outs = []
            for lib in (old, new):
                out = torch.full((b * s, h * hd), 7.0, dtype=dtype, device=dev)
                launcher(lib, kind, sfx, q, k, vt, out, b, h, kvh, hd, s, s_pad, k_pad, ks)()
                torch.cuda.synchronize()
                outs.append(out.view(torch.int16).cpu())
            eq = torch.equal(outs[0], outs[1])
            finite = bool(torch.isfinite(outs[1].view(dtype).float()).all())
            bad += not (eq and finite)
            rows.append(f"bits {sfx:4s} {kind:6s} hd{hd:<3d} b 2 h 4/2 S {s:3d}" + (f" K {ks:2d}" if ks else "     ") +
                        f": {'bytewise equal' if eq else 'DIFFERENT: %d of %d elements' % (int((outs[0] != outs[1]).sum()), outs[0].numel())}"
                        f"{'' if finite else ', NOT FINITE'}")
            print(rows[-1], flush=True)
    return rows, bad


def same_time(old, new, a, dev):
    rows, bad = [], 0
    a.window *= ATTENTION_WINDOWS          # a launch is tens of microseconds
    for sfx, dtype in (("f16", torch.float16), ("bf16", torch.bfloat16)):
        cases = [("hdw", 48, 32, 2, 1025, 0), ("hdw", 16, 96, 2, 1025, 0), ("hdw", 12, 128, 2, 1025, 0), ("hdw", 8, 128, 2, 1025, 0),
                 ("causal", 48, 32, 2, 1025, 0), ("causal", 16, 96, 2, 1025, 0), ("causal", 12, 128, 2, 1025, 0)]
        cases += [("window", 24, 64, b, s, ks) for b, s in ((2, 1025), (1, 6145)) for ks in (63, 255, 1023)]
        for kind, h, hd, b, s, ks in cases:
            q, k, vt, s_pad, k_pad = operands(b, h, h, hd, s, dtype, dev, h)
            out = torch.empty((b * s, h * hd), dtype=dtype, device=dev)
            res = [ST.windows(launcher(lib, kind, sfx, q, k, vt, out, b, h, h, hd, s, s_pad, k_pad, ks), a) for lib in (old, new, old, new)]
            (p1, _, p1max), (b1, _, _), (p2, _, p2max), (b2, _, _) = res
            spread = max(abs(p1 - p2), p1max - p1, p2max - p2)
            ok = max(b1, b2) <= max(p1, p2) + spread
            bad += not ok
            rows.append(f"time {sfx:4s} {kind:6s} hd{hd:<3d} H {h:2d}  {b} x S {s:4d}" + (f" K {ks:4d}" if ks else "       ") +
                        f": parent {1e3 * p1:7.1f} / {1e3 * p2:7.1f} us (spread {1e3 * spread:5.1f})  branch {1e3 * b1:7.1f} / {1e3 * b2:7.1f} us  "
                        f"bound {1e3 * (max(p1, p2) + spread):7.1f}  {'ok' if ok else 'ABOVE by %.1f us' % (1e3 * (max(b1, b2) - max(p1, p2) - spread))}")
            print(rows[-1], flush=True)
    return rows, bad


def main():
    a = ST.add_common_args(argparse.ArgumentParser()).parse_args()
    dev = torch.device("cuda:0")
    new = _hip.lib()
    old = load_parent(os.environ.get("AB_OLD_LIB", os.path.join(ROOT, "tools", "ab", "libsat_hip_parent.so")))
    bits, bad_bits = same_bits(old, new, dev)
    times, bad_times = same_time(old, new, a, dev)
    head = (f"attention kernels, parent library against this tree's in one process: {torch.cuda.get_device_name(0)}; time rows: medians of {a.reps} "
            f"windows of {a.window} launches, parent / branch / parent / branch; {bad_bits} bit rows and {bad_times} time rows fail\n")
    ST.write_report(a.out, head, bits + times)
    return 1 if bad_bits or bad_times else 0


if __name__ == "__main__":
    sys.exit(main())
