"""Time of one sat_roberta_encode call at the shape the clap_text conditioner of Stable Audio 2.0 runs: roberta-base, 11 of 12 layers
(feature_layer_ix = -2), L = 77, no proj_out, for B = 1 and B = 8.

Device events around single calls, median / min / max over --reps calls after --warmup calls per shape; a second pass times
windows of --window back-to-back calls (one event pair per window) so that a per-call figure without the event and launch gaps
stands next to it.  Weights are random tensors of the roberta-base shapes (the time does not depend on the values).  Needs a HIP
device; prints and, with --out, writes the report.

    python tools/clap_text_timing.py --out profiles/clap_text_timing.txt
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "friendly-stable-audio-tools_amd"))

SHAPE = {"vocab_size": 50265, "hidden_size": 768, "num_layers": 12, "intermediate_size": 3072, "max_positions": 514, "num_heads": 12,
         "pad_id": 1, "eps": 1e-5}


def random_state_dict(shape, seed):
    g = torch.Generator().manual_seed(seed)
    d, f = shape["hidden_size"], shape["intermediate_size"]
    r = lambda *s: 0.02 * torch.randn(*s, generator=g)
    sd = {"embeddings.word_embeddings.weight": r(shape["vocab_size"], d), "embeddings.position_embeddings.weight": r(shape["max_positions"], d),
          "embeddings.token_type_embeddings.weight": r(1, d), "embeddings.LayerNorm.weight": torch.ones(d), "embeddings.LayerNorm.bias": r(d)}
    for n in range(shape["num_layers"]):
        pf = f"encoder.layer.{n}."
        for lin, (o, i) in {"attention.self.query": (d, d), "attention.self.key": (d, d), "attention.self.value": (d, d),
                            "attention.output.dense": (d, d), "intermediate.dense": (f, d), "output.dense": (d, f)}.items():
            sd[pf + lin + ".weight"], sd[pf + lin + ".bias"] = r(o, i), r(o)
        for ln in ("attention.output.LayerNorm", "output.LayerNorm"):
            sd[pf + ln + ".weight"], sd[pf + ln + ".bias"] = torch.ones(d), r(d)
    return sd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--window", type=int, default=50)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("clap_text_timing: needs a HIP device (a CPU run says nothing about the MI355X)")
    from stable_audio_tools.models.conditioners import RobertaEncoderPlan
    dev = torch.device("cuda:0")
    run_layers, length = 11, 77
    plan = RobertaEncoderPlan(random_state_dict(SHAPE, 0), SHAPE, run_layers, dev)
    d, f = SHAPE["hidden_size"], SHAPE["intermediate_size"]
    lines = [f"sat_roberta_encode, roberta-base shape (hidden {d}, 12 heads, FFN {f}), {run_layers} of 12 layers (feature_layer_ix = -2), L = {length}, fp32,",
             f"no proj_out; {torch.cuda.get_device_name(0)}; device events; {args.warmup} warm-up calls, {args.reps} timed calls per shape,",
             f"then {args.reps // args.window} windows of {args.window} back-to-back calls.  The call includes the host-to-device copy of ids and mask.", ""]
    g = torch.Generator().manual_seed(1)
    for b in (1, 8):
        ids = torch.randint(3, SHAPE["vocab_size"], (b, length), generator=g)
        mask = torch.ones(b, length, dtype=torch.long)
        if b > 1:                      # prompts of mixed length, as a batch of texts has
            for n in range(1, b):
                real = 4 + 9 * n
                ids[n, real:], mask[n, real:] = SHAPE["pad_id"], 0
        ids, mask = ids.to(dev), mask.to(dev)
        for _ in range(args.warmup):
            plan.encode(ids, mask)
        torch.cuda.synchronize()
        single = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            plan.encode(ids, mask)
            e1.record()
            e1.synchronize()
            single.append(e0.elapsed_time(e1))
        windows = []
        for _ in range(max(args.reps // args.window, 1)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.window):
                plan.encode(ids, mask)
            e1.record()
            e1.synchronize()
            windows.append(e0.elapsed_time(e1) / args.window)
        m = b * length
        flop = run_layers * 2 * m * (4 * d * d + 2 * d * f) + run_layers * 4 * b * length * length * d
        med = statistics.median(single)
        lines.append(f"B = {b}: single call  median {med:.3f} ms  (min {min(single):.3f}, max {max(single):.3f});  "
                     f"per call in a window of {args.window}: median {statistics.median(windows):.3f} ms  (min {min(windows):.3f}, max {max(windows):.3f});  "
                     f"{flop / 1e9:.2f} GFLOP per call -> {flop / (statistics.median(windows) * 1e-3) / 1e12:.2f} TFLOP/s fp32 (whole call, not a kernel's share of peak)")
    plan.close()
    report = "\n".join(lines)
    print(report)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(report + "\n")


if __name__ == "__main__":
    main()
