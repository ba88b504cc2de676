"""Developer probe: full-size Oobleck decode (1024 latent frames) and encode (the same audio back) alone, for rocprofv3 / A-B runs
of the codec kernels.  Not part of the product or the tests.
Usage: python tools/codec_only.py [fp16|bf16|fp32]   (operand format of the codec kernels; default: the package default).
CODEC_CONFIG picks the shape: full (default, the Stable Audio VAE), full_nearest (the same with use_nearest_upsample=True: three-tap
polyphase upsamplers), small16 (16 channels, stage widths 16 ... 256, padded to 64 ... 256 inside the plan) or small64 (64 channels,
same depth: what small16 is padded towards in its narrow stages)."""
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "friendly-stable-audio-tools_amd"))
import torch

import stable_audio_tools as S
from stable_audio_tools import model_configs as MC, synthetic
from stable_audio_tools.models import _init

from stable_audio_tools import _hip

dev = torch.device("cuda:0")
config = MC.stable_audio_vae()
which = os.environ.get("CODEC_CONFIG", "full")
if which == "full_nearest":
    config["model"]["decoder"]["config"]["use_nearest_upsample"] = True
elif which in ("small16", "small64"):
    for part in ("encoder", "decoder"):
        config["model"][part]["config"]["channels"] = 16 if which == "small16" else 64
elif which != "full":
    raise SystemExit(f"unknown CODEC_CONFIG {which}")
with _init.skip_init():
    vae = S.create_model_from_config(config)
vae.load_state_dict(synthetic.synth_state_dict(vae.state_dict(), 3))
vae = vae.to(dev).eval()
if len(sys.argv) > 1:
    vae.set_gemm_dtype(sys.argv[1])
print(f"codec operands: {vae.decoder.gemm_dtype}, config: {which}", flush=True)
z = torch.randn(1, 64, int(os.environ.get("FRAMES", "1024")), device=dev)


def timeit(fn, iters):
    fn()
    torch.cuda.synchronize()
    t0 = time.time()
    for _ in range(iters):
        out = fn()
    torch.cuda.synchronize()
    return (time.time() - t0) / iters * 1e3, out


ms, audio = timeit(lambda: vae.decode(z), 5)
print(f"decode {z.shape[-1]} frames: {ms:.2f} ms", flush=True)
ms, lat = timeit(lambda: vae.encode(audio), 5)
print(f"encode {audio.shape[-1]} samples: {ms:.2f} ms", flush=True)
ws = {}
for name, part in (("decode", vae.decoder), ("encode", vae.encoder)):
    need = ctypes.c_size_t()
    _hip.check(_hip.lib().sat_oobleck_workspace_bytes(part._plan, 1, z.shape[-1], ctypes.byref(need)))
    ws[name] = need.value
print(f"workspace: decode {ws['decode'] / 2**30:.2f} GiB, encode {ws['encode'] / 2**30:.2f} GiB", flush=True)
