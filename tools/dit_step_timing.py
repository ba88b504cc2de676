"""What the step-timing tools of the DiT option families (tools/dit_*_timing.py) share: the command line, the event-pair window loop, the
DiT under test prepared for one prompt at CFG 7, and the cleanup between variants.  Each tool keeps its variants and its row text."""
import gc
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "friendly-stable-audio-tools_amd"))


def add_common_args(parser):
    parser.add_argument("--t-len", type=int, default=1024)
    parser.add_argument("--window", type=int, default=10)
    parser.add_argument("--reps", type=int, default=7)
    parser.add_argument("--warmup", type=int, default=5)
    parser.add_argument("--dtype", default=None, help="gemm_dtype of the step rows (default: the package default)")
    parser.add_argument("--out", default=None)
    return parser


def windows(fn, a):
    """(median, min, max) ms per call of fn: a.reps windows of a.window back-to-back calls between one pair of device events, after a.warmup calls."""
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


def full_dit(dev, overrides, product_kwargs, dtype, t_len, base=None, before_plan=None):
    """The full-size SA-Open DiT (or `base`) with `overrides` in its config and synthetic weights, prepared for one prompt of 130 context tokens
    at CFG 7; `before_plan(model)` sets what has to be set before the plan is built.  Returns (model, step), step() = one `denoise` call."""
    from stable_audio_tools import model_configs as MC, synthetic
    from stable_audio_tools.models import _init
    from stable_audio_tools.models.dit import DiffusionTransformer
    base = base or MC.stable_audio_open_1_0()["model"]["diffusion"]["config"]
    with _init.skip_init():
        m = DiffusionTransformer(**dict(base, **overrides), **product_kwargs)
    m.load_state_dict(synthetic.synth_state_dict(m.state_dict(), 0))
    m = m.to(dev).eval()
    if dtype:
        m.set_gemm_dtype(dtype)
    if before_plan:
        before_plan(m)
    x = synthetic.synth_input("x", (1, 64, t_len), 1).to(dev)
    c = synthetic.synth_input("c", (1, 130, base["cond_token_dim"]), 2).to(dev)
    g = synthetic.synth_input("g", (1, base["global_cond_dim"]), 3).to(dev)
    m.prepare_generation(c, g, 7.0)
    return m, lambda: m.denoise(x, 1.0, cfg_scale=7.0)


def release():
    """Frees what the last variant held on the device, once the caller has dropped its references to the model."""
    gc.collect()
    torch.cuda.empty_cache()


def step_windows(dev, a, overrides, product_kwargs=None, base=None, t_len=None, before_plan=None):
    """windows() of one sampler step of full_dit(...) at T = t_len (default a.t_len); the model is gone afterwards."""
    m, step = full_dit(dev, overrides, product_kwargs or {}, a.dtype, t_len or a.t_len, base, before_plan)
    try:
        return windows(step, a)
    finally:
        del m, step
        release()


def write_report(path, head, lines):
    if path:
        with open(path, "w") as f:
            f.write(head + "\n".join(lines) + "\n")
