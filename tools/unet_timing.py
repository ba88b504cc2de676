"""Cost of the Dance Diffusion U-Net (DiffusionAttnUnet1D, default config: depth 14, 221.4 M parameters) on the device.

    python tools/unet_timing.py time                       device-event times: one forward at batch 1 and 8 (fp16, bf16), a 100-step
                                                           generate_diffusion_uncond at batch 1 (65536 samples)
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/unet_timing.py trace --batch B --calls N
                                                           N forwards after one warm-up, for a kernel trace in a run of its own
    python tools/unet_timing.py summarize <kernel_stats.csv> --batch B --calls N
                                                           the trace by launch class: launches and time per forward, TFLOP/s of the convolution
                                                           GEMMs against their algorithmic FLOPs, GB/s of the bandwidth kernels against the bytes
                                                           they must move (both counted here, from the config, by walking the plan's launch list)
Weights are synthetic (the seeded generator of tests/golden/unet_cases.py); the cost does not depend on them.
"""
import argparse
import csv
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "friendly-stable-audio-tools_amd"), os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)

T = 65536
DEFAULT = dict(io_channels=2, depth=14, n_attn_layers=6, channels=[128, 128, 256, 256] + [512] * 10, kernel_size=5)


def build(dev, fmt="fp16", cfg=None):
    import torch
    import unet_cases as UC
    from stable_audio_tools.models import _init
    from stable_audio_tools.models.diffusion import DiffusionAttnUnet1D
    with _init.skip_init():
        m = DiffusionAttnUnet1D(**(cfg or {}))
    m.load_state_dict(UC.weights(m.state_dict()), strict=True)
    return m.to(dev).eval().set_gemm_dtype(fmt)


def inputs(dev, b):
    import torch
    g = torch.Generator().manual_seed(1)
    return torch.randn(b, 2, T, generator=g).to(dev), torch.rand(b, generator=g).to(dev)


def events_ms(fn, iters, repeats=3, warmup=2):
    import torch
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / iters)
    return out


def cmd_time(args):
    import torch
    from stable_audio_tools.inference.generation import generate_diffusion_uncond
    from stable_audio_tools.models.diffusion import DiffusionModelWrapper
    dev = torch.device("cuda:0")
    print(f"default config (depth 14, channels 128 128 256 256 512 x 10, n_attn_layers 6, kernel_size 5), {T} samples; ms per forward, device events "
          "round `iters` forwards after 2 warm-up calls, three repeats")
    for fmt in ("fp16", "bf16"):
        m = build(dev, fmt)
        for b, iters in ((1, 10), (8, 3)):
            x, t = inputs(dev, b)
            r = events_ms(lambda: m(x, t), iters)
            print(f"{fmt} batch {b}: {min(r):.2f} ms per forward (repeats {', '.join(f'{v:.2f}' for v in r)}; {iters} forwards each), "
                  f"workspace {m._ws.numel() / 2**20:.0f} MiB")
        if fmt == "fp16":
            model = DiffusionModelWrapper(m, io_channels=2, sample_size=T, sample_rate=48000, min_input_length=1)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            generate_diffusion_uncond(model, steps=100, batch_size=1, sample_size=T, seed=1, device="cuda:0", sampler_type="dpmpp-3m-sde",
                                      sigma_min=0.3, sigma_max=500)
            torch.cuda.synchronize()
            print(f"fp16 batch 1: generate_diffusion_uncond, 100 steps of dpmpp-3m-sde, {T} samples: {time.perf_counter() - t0:.3f} s wall clock")
        del m


def cmd_trace(args):
    import torch
    dev = torch.device("cuda:0")
    m = build(dev, args.format)
    x, t = inputs(dev, args.batch)
    m(x, t)
    torch.cuda.synchronize()
    for _ in range(args.calls):
        m(x, t)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------ the launch list, counted
def account(cfg, b, t, el=2):
    """class -> [launches, flops, bytes] of one forward, following csrc/unet_plan.hip (16-bit operands of `el` bytes)"""
    acc = {}

    def add(cls, flops=0, nbytes=0, n=1):
        a = acc.setdefault(cls, [0, 0, 0])
        a[0] += n; a[1] += flops; a[2] += nbytes

    k, depth, ch, io = cfg["kernel_size"], cfg["depth"], cfg["channels"], cfg["io_channels"]
    has_attn = lambda l: l >= 1 and cfg["n_attn_layers"] > 0 and l + 1 >= depth - cfg["n_attn_layers"]

    def conv(M, n, kk, taps):
        cls = "k-tap convolution GEMMs" if taps > 1 else "1 x 1 GEMMs"
        add(cls, 2 * M * n * kk * taps, M * kk * el + n * kk * taps * el + M * n * 4)

    def norm(M, c, skip, out32, out_op):
        add("GroupNorm statistics", 0, M * c * 4, 2)
        add("GroupNorm apply", 0, M * c * 4 * (1 + skip + out32) + M * c * el * out_op)

    def block(M, cin, cmid, cout, first=False):
        if not first:
            conv(M, cmid, cin, k)
        norm(M, cmid, 0, 0, 1)
        conv(M, cout, cmid, k)
        if cin != cout and not first:
            conv(M, cout, cin, 1)
        norm(M, cout, 1, 1, 1)

    def attention(M, S, c):
        norm(M, c, 0, 0, 1)
        conv(M, 3 * c, c, 1)
        add("head split", 0, M * 3 * c * (4 + el))
        add("attention", 4 * M * S * c, M * 4 * c * el)
        conv(M, c, c, 1)
        add("casts and concat copies", 0, M * c * (4 + el))

    def level(l, S):
        M, c, cp = b * S, ch[l], ch[l - 1] if l else ch[0]
        if l:
            add("casts and concat copies", 0, 2 * M * cp * (4 + el))
            add("resamplers", 0, 2 * M * cp * 4 + M * cp * (4 + el))
            add("stream copy behind the downsampler", 0, 2 * M * cp * 4)
            if has_attn(l):
                add("q / k / v pad clears", 0, 0, 2 if l < depth - 1 else 1)
        up_in = c if l == depth - 1 else 2 * c
        shapes = [(cp if l else io + 16, c, c), (c, c, c), (c, c, c), (up_in, c, c), (c, c, c), (c, c, cp if l else io)]
        for i, (cin, cmid, cout) in enumerate(shapes):
            if i == 3 and l < depth - 1:
                level(l + 1, S // 2)
            if l == 0 and i == 0:
                add("boundary kernels", 2 * M * (io + 16) * c * (k + 1), b * io * t * 4 + 2 * M * c * 4)
                block(M, cin, cmid, cout, first=True)
            elif l == 0 and i == 5:
                conv(M, cmid, cin, k)
                norm(M, cmid, 0, 1, 0)
                add("boundary kernels", 2 * M * c * io * (k + 1), 2 * M * c * 4 + b * io * t * 4)
            else:
                block(M, cin, cmid, cout)
                if has_attn(l):
                    attention(M, S, cout)
        if l:
            add("resamplers", 0, M * cp * 4 + 2 * M * cp * el)

    level(0, t)
    return acc


CLASSES = [("ff_conv_kernel", "k-tap convolution GEMMs"), ("unet_gn_partials", "GroupNorm statistics"), ("unet_gn_finish", "GroupNorm statistics"),
           ("unet_gn_apply", "GroupNorm apply"), ("unet_down", "resamplers"), ("unet_up", "resamplers"), ("unet_cast_rows", "casts and concat copies"),
           ("unet_input", "boundary kernels"), ("unet_output", "boundary kernels"), ("head_split", "head split"), ("attention", "attention"),
           ("gemm", "1 x 1 GEMMs"), ("fill", "q / k / v pad clears"), ("memset", "q / k / v pad clears"), ("copyBuffer", "stream copy behind the downsampler")]
SKIP = ("pack_conv_taps", "pack_", "elementwise", "distribution", "random")      # plan build and input generation


def cmd_summarize(args):
    rows = list(csv.DictReader(open(args.csv)))
    got = {}
    other = []
    for r in rows:
        name, calls, ns = r["Name"], int(r["Calls"]), float(r["TotalDurationNs"])
        if any(s in name for s in SKIP):
            continue
        cls = next((c for key, c in CLASSES if key in name), None)
        if cls is None:
            other.append((name, calls, ns))
            continue
        g = got.setdefault(cls, [0, 0.0])
        g[0] += calls; g[1] += ns
    per = args.calls + 1          # the warm-up forward is in the trace as well
    acc = account(DEFAULT, args.batch, T)
    total = sum(v[1] for v in got.values()) / per
    flops = sum(v[1] for c, v in acc.items() if "GEMM" in c)
    print(f"batch {args.batch}, {T} samples, {args.format}: {sum(v[0] for v in got.values()) // per} launches, {total / 1e6:.2f} ms of kernel time per forward; "
          f"algorithmic FLOPs of the convolutions {flops / 1e12:.3f} TFLOP per forward (k-tap {acc['k-tap convolution GEMMs'][1] / 1e12:.3f}, "
          f"1 x 1 {acc['1 x 1 GEMMs'][1] / 1e12:.3f}), attention {acc.get('attention', [0, 0, 0])[1] / 1e12:.4f}")
    print(f"  {'class':38s} {'launches':>8s} {'counted':>8s} {'us':>10s} {'%':>6s}   rate against the algorithmic count")
    for cls, (calls, ns) in sorted(got.items(), key=lambda kv: -kv[1][1]):
        us = ns / per / 1e3
        n, fl, by = acc.get(cls, [0, 0, 0])
        rate = f"{fl / (us * 1e-6) / 1e12:8.1f} TFLOP/s" if fl and ("GEMM" in cls or cls == "attention") else (f"{by / (us * 1e-6) / 1e9:8.0f} GB/s" if by else "")
        print(f"  {cls:38s} {calls // per:8d} {n:8d} {us:10.1f} {100 * ns / per / total:6.1f}   {rate}")
    print("  (the copy row also holds the device-to-device copies of the plan's finalize, once per plan; `counted` is the forward's own)")
    for name, calls, ns in sorted(other, key=lambda r: -r[2])[:8]:
        print(f"  (unclassified) {name[:90]}: {calls} calls, {ns / 1e3:.1f} us in the whole trace")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["time", "trace", "summarize"])
    ap.add_argument("csv", nargs="?")
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--format", default="fp16")
    a = ap.parse_args()
    {"time": cmd_time, "trace": cmd_trace, "summarize": cmd_summarize}[a.mode](a)
