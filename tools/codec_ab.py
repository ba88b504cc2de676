"""Same-box A/B of the full-size Oobleck codec: the PARENT commit's library against this tree's library, timed INTERLEAVED in one
process: 1024-frame decode and the encode of that audio.  Each library runs AB_INSTANCES (default 3) models of its own (own weights
and workspace): the range of the parent's instance medians is the spread of the box, which the branch's instances must lie within.
Also checks that both libraries give the same bits.  Developer tool; not part of the product or the tests.

The parent's library (git-ignored like every .so):
    git worktree add /tmp/sat_parent HEAD~1 && make -C /tmp/sat_parent/friendly-stable-audio-tools_amd/csrc -j8
    mkdir -p tools/ab && cp /tmp/sat_parent/friendly-stable-audio-tools_amd/lib/libsat_hip.so tools/ab/libsat_hip_parent.so
usage: python tools/codec_ab.py [fp16 bf16 fp32 ...]      (AB_ROUNDS=8 rounds, AB_OLD_LIB=path of the parent's library,
AB_EXTRA=name:path,... further builds of this tree)"""
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "friendly-stable-audio-tools_amd"))
import torch  # noqa: E402

from stable_audio_tools import _hip  # noqa: E402

dev = torch.device("cuda:0")


def load_parent(path):
    """the parent's library behind this tree's Python: it has no sat_oobleck_plan_create_ex, and the default options are its only mode"""
    h = ctypes.CDLL(path)
    for name, (res, args) in _hip._SIGNATURES.items():
        if hasattr(h, name):
            fn = getattr(h, name)
            fn.restype, fn.argtypes = res, args
    if not hasattr(h, "sat_oobleck_plan_create_ex"):
        h.sat_oobleck_plan_create_ex = lambda cfg, opt, size, out: h.sat_oobleck_plan_create(cfg, out)
    return h


def timeit(fn, iters, warm=1):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    import stable_audio_tools as S
    from stable_audio_tools import model_configs as MC, synthetic
    from stable_audio_tools.models import _init
    new = _hip.lib()
    old = load_parent(os.environ.get("AB_OLD_LIB", os.path.join(ROOT, "tools", "ab", "libsat_hip_parent.so")))
    n_inst = int(os.environ.get("AB_INSTANCES", "3"))
    entries = {}
    for i in range(n_inst):          # alternating, so that neither library has the earlier allocations or the earlier slot of a round
        entries[f"parent_{i}"] = old
        entries[f"branch_{i}"] = new
    for item in filter(None, os.environ.get("AB_EXTRA", "").split(",")):      # name:path of further builds of this tree
        name, _, path = item.partition(":")
        entries[name] = load_parent(os.path.join(ROOT, path))
    print(torch.cuda.get_device_name(0), flush=True)
    vaes = {}
    for name, h in entries.items():
        _hip._lib = h
        with _init.skip_init():
            vae = S.create_model_from_config(MC.stable_audio_vae())
        vae.load_state_dict(synthetic.synth_state_dict(vae.state_dict(), 3))
        vaes[name] = vae.to(dev).eval()
    z = synthetic.synth_input("z", (1, 64, int(os.environ.get("FRAMES", "1024"))), 1).to(dev)
    rounds = int(os.environ.get("AB_ROUNDS", "8"))
    for fmt in sys.argv[1:] or ["fp16", "fp32"]:
        iters = 2 if fmt == "fp32" else 5
        outs = {}
        for name, h in entries.items():
            _hip._lib = h
            vaes[name].set_gemm_dtype(fmt)
            audio = vaes[name].decode(z)
            outs[name] = (audio, vaes[name].encoder(audio))
        same = all(torch.equal(a, b) for n in entries for a, b in zip(outs[n], outs["parent_0"]))
        res = {(n, w): [] for n in entries for w in ("decode", "encode")}
        for _ in range(rounds):
            for name, h in entries.items():
                _hip._lib = h
                res[name, "decode"].append(timeit(lambda: vaes[name].decode(z), iters))
                res[name, "encode"].append(timeit(lambda: vaes[name].encoder(outs[name][0]), iters))
        for what in ("decode", "encode"):
            med = {n: statistics.median(res[n, what]) for n in entries}
            base = statistics.median(med[n] for n in entries if n.startswith("parent_"))
            print(f"{what} {z.shape[-1]} frames, {fmt}, median of {rounds} rounds per instance (min .. max of its rounds):", flush=True)
            for n in entries:
                print(f"    {n:10s} {med[n]:8.3f} ms ({min(res[n, what]):.3f} .. {max(res[n, what]):.3f})  {100 * (med[n] / base - 1):+.2f} %", flush=True)
            for grp in ("parent_", "branch_") + tuple(n for n in entries if not n.startswith(("parent_", "branch_"))):
                ms = [med[n] for n in entries if n.startswith(grp)]
                print(f"  {grp.rstrip('_'):8s} instance medians {min(ms):.3f} .. {max(ms):.3f} ms = {100 * (min(ms) / base - 1):+.2f} .. "
                      f"{100 * (max(ms) / base - 1):+.2f} % of the parent's middle instance", flush=True)
        print(f"{fmt}: every instance's decode and encode output bit-identical to parent_0's: {same}", flush=True)
    for name, vae in vaes.items():          # every plan goes back to the library that made it
        for part in (vae.encoder, vae.decoder):
            if part._plan is not None:
                entries[name].sat_oobleck_plan_destroy(part._plan)
                part._plan = None
    _hip._lib = new


if __name__ == "__main__":
    main()
