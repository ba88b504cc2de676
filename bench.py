"""Headline benchmark (BASELINE.json): audio-seconds/sec @ 44.1 kHz stereo, 100-step DPM-Solver++(3M) SDE,
Stable-Audio-Open-1.0 shape, synthetic random-init weights + random T5 embeddings.

    python bench.py --gpus N --steps K --warmup W            (any N: for N > 1 it re-executes itself under torch.distributed.run)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N --steps K --warmup W

One "step" = one full ``generate_diffusion_cond`` call on this rank's prompts: conditioning -> 100 sampler steps
(each = one CFG-batched DiT evaluation + the fused DPM++ update) -> Oobleck decode -> int16 quantisation, and for
N > 1 one RCCL all-gather of the int16 audio.  Prompts are sharded rank-strided (reference generate.py:119-120),
one full model replica per GPU, no collective on the data path except that final gather -> weak scaling.
Rank 0 prints ONE JSON line.

A plain run sets up, warms up, times the K steps and prints the line (``ms_per_step`` = wall milliseconds of one timed step).
``--dump-outputs DIR`` writes what the last timed step returned (the int16 audio, as float32 .npy) for output-for-output comparisons of
two builds: the weights, prompts and seeds depend only on the arguments.  ``--full`` adds what takes runs of its own: the FFN-in
GEMM's roofline figures (a HIP-event profiled pass after the timed steps) and, at one GPU, the CPU baseline.
"""
import argparse
import ctypes
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "friendly-stable-audio-tools_amd"))

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

SAMPLE_SIZE = 2097152
SAMPLE_RATE = 44100
SAMPLER = dict(sampler_type="dpmpp-3m-sde", sigma_min=0.3, sigma_max=500)
CFG_SCALE = 7.0
DIT_STEPS = 100
# developer smoke test of the RCCL path on a 1-GPU box: run under torch.distributed.run --nproc-per-node 1 with this set, and the
# process group, barrier, all-reduce and the final all-gather are exercised with world_size 1
FORCE_DIST = os.environ.get("SAT_BENCH_FORCE_DIST") == "1"
BF16_MFMA_PEAK_TFLOPS = 2500.0    # dense, /opt/skills/guides/MI355X_MICROARCH.md
FP8_MFMA_PEAK_TFLOPS = 5000.0     # dense e4m3 (the FF-in GEMM of --dtype fp8 runs v_mfma_scale_f32_16x16x128_f8f6f4)


# --workload sa2_a2a = BASELINE config 4: Stable Audio 2.0 shape (285-s context, T = 6144 latent frames, S = 6145), audio-to-audio:
# VAE encode of the init audio + 100 sampler steps + decode.  Not the headline; an extra measured point.
WORKLOAD = {"name": "sa_open"}


def build_model(dev):
    import stable_audio_tools as S
    from stable_audio_tools import model_configs as MC, synthetic
    from stable_audio_tools.models import _init
    with _init.skip_init():
        model = S.create_model_from_config(MC.stable_audio_2_0() if WORKLOAD["name"] == "sa2_a2a" else MC.stable_audio_open_1_0())
    sd = synthetic.synth_state_dict(model.state_dict(), 0)
    model.load_state_dict(sd)
    return model.to(dev).eval(), sd


def conditioning(model, prompt_ids, dev):
    """Random 'T5' embeddings (seeded per prompt id) + the model's own number conditioners."""
    from stable_audio_tools import synthetic
    cond = model.conditioner([{"seconds_start": 0, "seconds_total": int(SAMPLE_SIZE / SAMPLE_RATE)} for _ in prompt_ids])
    emb = torch.stack([synthetic.synth_input(f"prompt{i}", (128, 768), 2) for i in prompt_ids]).to(dev)
    cond["prompt"] = (emb, torch.ones(len(prompt_ids), 128, device=dev))
    return {k: cond[k] for k in ("prompt", "seconds_start", "seconds_total")}


def one_generation(model, cond, seed, dev, world):
    from stable_audio_tools import _hip
    from stable_audio_tools.inference.generation import generate_diffusion_cond
    extra = dict(SAMPLER)
    if WORKLOAD["name"] == "sa2_a2a":
        extra.update(init_audio=(SAMPLE_RATE, WORKLOAD["init_audio"]), init_noise_level=7.0)
    audio = generate_diffusion_cond(model, steps=DIT_STEPS, cfg_scale=CFG_SCALE, conditioning_tensors=cond, sample_size=SAMPLE_SIZE,
                                    seed=seed, device=str(dev), **extra)
    # per-item int16 quantisation on the device (reference generate.py:142-151 / audio_utils.py:21-26)
    b, c, n = audio.shape
    out = torch.empty((b, c, n), dtype=torch.int16, device=dev)
    scratch = torch.empty(1, dtype=torch.int32, device=dev)
    for i in range(b):
        _hip.check(_hip.lib().sat_float_to_int16(_hip.ptr(audio[i]), _hip.ptr(out[i]), c * n, 0, _hip.ptr(scratch), _hip.stream()))
    if world > 1 or FORCE_DIST:
        from stable_audio_tools.inference.distributed import gather_sharded
        out = gather_sharded(out, world * b)           # the single RCCL collective (xGMI)
    # the reference's float_to_int16_audio ends in .cpu() (utils/audio_utils.py:21-26) and every rank writes its OWN prompts' files
    # (generate.py:119-120, 142-151): each rank takes its own shard off the device inside the timed step (8.4 MB per prompt); the gathered
    # batch stays in HBM on every rank.  (Until round 5 rank 0 copied the whole gathered batch -- 537 MB of pageable D2H per step on
    # config 3 -- while the others copied 1/8 of that: a built-in scaling loss under the MAX-over-ranks clock.)
    rank = int(os.environ.get("RANK", "0"))
    return (out[rank::world] if world > 1 else out).cpu()


def cpu_baseline(sd):
    """The oracle (torch fp32 restatement == the reference's CPU path) on the host cores, bounded sample:
    ONE CFG denoiser evaluation at full SA-Open size per thread count of a small sweep + decode of 43 latent frames at the best
    count, extrapolated to 100 steps + 1024 frames.  The line reports the best count, every count tried, os.cpu_count() and the
    affinity mask size ("core count printed")."""
    from oracle import dit as odit, oobleck as oob
    from stable_audio_tools import synthetic
    try:
        avail = len(os.sched_getaffinity(0))
    except AttributeError:
        avail = os.cpu_count() or 1
    # (never "all logical CPUs" of a 256-thread host: measured 177 s per evaluation there against 6.1 s on 32 threads)
    counts = sorted({c for c in (8, 16, 32, 64) if 1 <= c <= avail} | ({avail} if avail < 8 else set()))
    dsd = {k[len("model.model."):]: v for k, v in sd.items() if k.startswith("model.model.")}
    vsd = {k[len("pretransform.model.decoder."):]: v for k, v in sd.items() if k.startswith("pretransform.model.decoder.")}
    x = synthetic.synth_input("x", (1, 64, 1024), 1)
    c = synthetic.synth_input("c", (1, 130, 768), 2)
    g = synthetic.synth_input("g", (1, 1536), 3)
    t = torch.tensor([0.5])
    sweep = {}
    with torch.no_grad():
        for n in counts:
            torch.set_num_threads(n)
            t0 = time.perf_counter()
            odit.dit_forward(dsd, x, t, c, g, 24, 24, cfg_scale=CFG_SCALE)
            sweep[n] = time.perf_counter() - t0
            if sweep[n] > 2.0 * min(sweep.values()):      # more threads only get slower from here (oversubscribed / cgroup-limited host)
                break
        best = min(sweep, key=sweep.get)
        torch.set_num_threads(best)
        t_step = sweep[best]
        z = synthetic.synth_input("z", (1, 64, 43), 4)
        oob.oobleck_decoder(vsd, z)      # warm-up
        t0 = time.perf_counter()
        oob.oobleck_decoder(vsd, z)
        t_dec = time.perf_counter() - t0
    total = DIT_STEPS * t_step + t_dec * (1024 / 43)
    return {"value": (SAMPLE_SIZE / SAMPLE_RATE) / total, "unit": "audio-seconds/sec", "cores": best, "kind": "port",
            "host_logical_cpus": os.cpu_count(), "affinity_cpus": avail,
            "thread_sweep_s_per_cfg_step": {str(k): round(v, 3) for k, v in sweep.items()},
            "sample": f"1 CFG DiT evaluation at full size per thread count (best: {best} threads, {t_step:.2f} s) x100 + Oobleck decode of "
                      f"43 frames ({t_dec:.2f} s) x(1024/43), extrapolated"}


def roofline(args, tot_ms, launches, m, n, k):
    """--full: the FFN-in GEMM's figures from the profiled pass (total HIP-event milliseconds over `launches` launches of M x N x K)"""
    avg_ms = tot_ms / max(launches, 1)
    flops = 2.0 * m * n * k          # algorithmic FLOPs of one launch (ff_in 38.69 GFLOP/seq/layer)
    achieved = flops / (avg_ms * 1e-3) / 1e12 if avg_ms > 0 else 0.0
    # HBM traffic of the dominant kernel cannot be measured inside a timed run (PMC passes serialise the kernels): it is the
    # figure of the latest committed rocprofv3 --pmc pass of this same command (FETCH_SIZE x2 + WRITE_SIZE, separate passes)
    traffic, traffic_source = None, None
    import glob
    for tpath in sorted(glob.glob(os.path.join(ROOT, "profiles", "r[0-9][0-9]_ffn_traffic.json")), reverse=True):          # newest round first
        tname = os.path.basename(tpath)
        if os.path.exists(tpath) and args.batch == 1 and args.dtype in ("bf16", "fp16") and args.workload == "sa_open":
            traffic = json.load(open(tpath)).get("hbm_bytes_per_launch")
            traffic_source = f"profiles/{tname} (rocprofv3 --pmc passes of this command, not measured in this run)"
            break
    mfma_peak = FP8_MFMA_PEAK_TFLOPS if args.dtype.startswith("fp8") else BF16_MFMA_PEAK_TFLOPS          # fp16 and bf16 MFMAs: the same dense peak
    # The dense peak is quoted at 2.4 GHz; under the 1400 W cap this launch runs at the EFFECTIVE clock of the latest committed GRBM_GUI_ACTIVE pass
    # (profiles/rNN_clock.json: a counter pass serialises the kernels, so it cannot be taken inside a timed run): the fraction is reported at both
    eff_clock, clock_source = None, None
    for cpath in sorted(glob.glob(os.path.join(ROOT, "profiles", "r[0-9][0-9]_clock.json")), reverse=True):
        cj = json.load(open(cpath))
        if args.workload == "sa_open" and args.dtype in ("bf16", "fp16") and str(args.batch) in cj.get("ffn_in_effective_clock_ghz", {}):
            eff_clock = cj["ffn_in_effective_clock_ghz"][str(args.batch)] / cj.get("peak_clock_ghz", 2.4)
            clock_source = f"profiles/{os.path.basename(cpath)} (effective clock {cj['ffn_in_effective_clock_ghz'][str(args.batch)]} GHz of {cj.get('peak_clock_ghz', 2.4)}; not measured in this run)"
        break
    return {"bound": "mfma", "kernel": f"FFN-in SwiGLU GEMM M={m} N={n} K={k} ({args.dtype} MFMA, fp32 acc)", "achieved": achieved,
            "peak": mfma_peak, "unit": "TFLOP/s", "frac": achieved / mfma_peak,
            "frac_at_effective_clock": (achieved / (mfma_peak * eff_clock)) if eff_clock else None, "effective_clock_source": clock_source, "traffic": traffic,
            "traffic_source": traffic_source, "avg_launch_us": avg_ms * 1e3, "launches_timed": launches}


# ---- the multi-rank logic, in functions of its own so that the CPU test (tests/test_bench_ranks.py, gloo, world size 2) runs exactly
# what an 8-GPU launch runs, with the generation stubbed out
def shard_prompts(world, rank, batch):
    """rank-strided prompt ids, as the reference's generate.py:119-120"""
    return list(range(world * batch))[rank::world]


def timed_steps(step_fn, steps, use_dist, sync, device):
    """K steps bracketed by barrier + device sync on both sides; returns the MAX over ranks of the elapsed seconds"""
    if use_dist:
        dist.barrier()
    sync()
    t0 = time.perf_counter()
    for i in range(steps):
        step_fn(2000 + i)
    if use_dist:
        dist.barrier()
    sync()
    elapsed = time.perf_counter() - t0
    if use_dist:
        t = torch.tensor([elapsed], device=device, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    return elapsed


def stub_generation(prompt_ids, seed, dev):
    """SAT_BENCH_STUB=1 (CPU test of the rank plumbing): int16 'audio' that encodes (prompt id, seed), 2 x 64 samples per prompt"""
    rows = [torch.full((2, 64), (pid * 131 + seed) % 30000, dtype=torch.int16) + torch.arange(64, dtype=torch.int16) for pid in prompt_ids]
    return torch.stack(rows).to(dev)


DUMP_BYTES = 64 * 10**6


def dump_outputs(out_dir, arrays):
    """--dump-outputs: each array as DIR/<name>.npy in float32, so that two builds can be compared output for output.  Past DUMP_BYTES
    in all, an array keeps a share of its elements at fixed indices (seeded: the same on every run), written flat, with the flat indices
    in DIR/<name>_index.npy (float64, exact)."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    total = sum(a.numel() for a in arrays.values()) * 4
    for name, a in arrays.items():
        a = a.detach().cpu().to(torch.float32)
        if total > DUMP_BYTES:
            keep = a.numel() * ((DUMP_BYTES - 4096) // 3) // total          # 4 bytes of value + 8 of index per element kept
            g = torch.Generator().manual_seed(20241016)
            idx = torch.unique(torch.randint(a.numel(), (keep,), generator=g))
            np.save(os.path.join(out_dir, f"{name}_index.npy"), idx.to(torch.float64).numpy())
            a = a.reshape(-1)[idx]
        np.save(os.path.join(out_dir, f"{name}.npy"), a.numpy())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batch", type=int, default=None,
                    help="prompts per GPU; default 1 at --gpus 1 (BASELINE config 2) and 8 at --gpus > 1 (config 3: 64 prompts on 8 GPUs)")
    ap.add_argument("--full", action="store_true",
                    help="after the headline, also measure what takes runs of its own: the FFN-in GEMM's roofline figures (a HIP-event "
                         "profiled pass of --steps generations) and, at one GPU, the CPU baseline (the oracle on the host cores)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: leave out the CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step returned (rank 0's int16 audio) to DIR/audio.npy as float32; a fixed, seeded "
                         f"sample of it (DIR/audio.npy + DIR/audio_index.npy) if it exceeds {DUMP_BYTES // 10**6} MB")
    ap.add_argument("--dtype", choices=("bf16", "fp16", "fp8", "fp8-all"), default="fp16",
                    help="GEMM / attention / codec operand type: fp16 (default: the reference's own GPU arithmetic and the build that meets the "
                         "1e-3 target against its fp32 outputs), bf16 (the same kernels on the bf16 MFMAs: 3-4 %% faster, 8x the operand "
                         "rounding) fp8 = BASELINE config 5 (e4m3 cross to_q / FF-in / FF-out, rest bf16) or fp8-all (every block GEMM e4m3: round 3's mode)")
    ap.add_argument("--layernorm", choices=("fused", "standalone"), default="fused",
                    help="LayerNorms of the blocks inside the GEMM epilogues (sat_dit_cfg.ln_fold, default) or as three kernels per block")
    ap.add_argument("--cross-attention", choices=("fused", "separate"), default="fused",
                    help="A/B: to_q + cross-attention core as one launch (where it applies: one prompt per GPU) or as two kernels")
    ap.add_argument("--workload", choices=("sa_open", "sa2_a2a"), default="sa_open",
                    help="sa_open: the headline (BASELINE config 2/3); sa2_a2a: config 4, SA-2.0 shape, audio-to-audio, 1 GPU")
    ap.add_argument("--dry-run", action="store_true", help="check the arguments and print the rank -> prompt plan as JSON; touches no GPU")
    args = ap.parse_args()
    if args.batch is None:
        args.batch = 1 if args.gpus == 1 else 8
    if args.gpus < 1 or args.batch < 1 or args.steps < 1 or args.warmup < 0:
        raise SystemExit("bench.py: --gpus / --batch / --steps must be >= 1 and --warmup >= 0")
    if args.dry_run:
        print(json.dumps({"dry_run": True, "n_gpus": args.gpus, "prompts_per_gpu": args.batch, "global_batch": args.gpus * args.batch,
                          "prompt_ids_per_rank": [shard_prompts(args.gpus, r, args.batch) for r in range(args.gpus)],
                          "collectives_per_step": 1 if args.gpus > 1 else 0, "launch": "python -m torch.distributed.run --nnodes=1 "
                          f"--nproc-per-node {args.gpus} --master-addr 127.0.0.1 --master-port P bench.py --gpus {args.gpus} --steps {args.steps} "
                          f"--warmup {args.warmup} --batch {args.batch}"}))
        return
    global SAMPLE_SIZE
    WORKLOAD["name"] = args.workload
    if args.workload == "sa2_a2a":
        SAMPLE_SIZE = 12582912

    if "WORLD_SIZE" not in os.environ and (args.gpus > 1 or FORCE_DIST):
        # plain `python bench.py --gpus N`: start the N ranks ourselves (one process per GPU over RCCL), exactly the command line
        # the driver would use; rank 0 of the child job prints the JSON line on our stdout
        import socket
        import subprocess
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        env = dict(os.environ)
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
               "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
        sys.exit(subprocess.run(cmd, env=env).returncode)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world} (launched with a different --nproc-per-node?)")
    use_dist = world > 1 or FORCE_DIST
    if os.environ.get("SAT_BENCH_STUB") == "1":
        # CPU test of the rank plumbing: same sharding, barriers, max-reduced clock, gather and JSON line; gloo instead of RCCL and a
        # stub instead of the model.  Never a benchmark: the line says so.
        from stable_audio_tools.inference.distributed import gather_sharded
        dev = torch.device("cpu")
        if use_dist:
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            os.environ.setdefault("MASTER_PORT", "29533")
            dist.init_process_group("gloo", rank=rank, world_size=world)
        prompt_ids = shard_prompts(world, rank, args.batch)
        last = {}

        def step(seed):
            out = stub_generation(prompt_ids, seed, dev)
            last["audio"] = gather_sharded(out, world * args.batch) if use_dist else out

        for i in range(args.warmup):
            step(1000 + i)
        elapsed = timed_steps(step, args.steps, use_dist, lambda: None, dev)
        if rank == 0:
            audio = last["audio"]
            if args.dump_outputs:                          # what the real step returns on rank 0: its own prompts of the gathered batch
                dump_outputs(args.dump_outputs, {"audio": audio[rank::world] if world > 1 else audio})
            print(json.dumps({"stub": True, "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": elapsed / args.steps * 1e3,
                              "rccl_ranks": world if use_dist else 0, "gathered_shape": list(audio.shape),
                              "gathered_first_samples": [int(v) for v in audio[:, 0, 0]], "prompt_ids_rank0": prompt_ids}), flush=True)
        if use_dist:
            dist.destroy_process_group()
        return
    if torch.cuda.device_count() <= local:
        raise SystemExit(f"bench.py: rank {rank} wants GPU {local}, only {torch.cuda.device_count()} visible")
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if use_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        # RCCL prints a version banner on the C-level stdout when its communicator comes up: keep stdout = the ONE JSON line by
        # pointing fd 1 at stderr until the first collective has run
        sys.stdout.flush()
        saved_fd = os.dup(1)
        os.dup2(2, 1)
        try:
            dist.init_process_group("nccl", device_id=dev, rank=rank, world_size=world)
            dist.barrier()
            torch.cuda.synchronize()
        finally:
            sys.stdout.flush()
            os.dup2(saved_fd, 1)
            os.close(saved_fd)

    model, sd = build_model(dev)
    if args.workload == "sa2_a2a":
        g = torch.Generator(device="cpu").manual_seed(11)
        WORKLOAD["init_audio"] = (torch.rand(2, SAMPLE_SIZE, generator=g) - 0.5).to(dev)
        args.no_cpu_baseline = True
    cpu_base = args.full and world == 1 and not args.no_cpu_baseline
    if rank != 0 or not cpu_base:
        sd = None
    # rank-strided prompt sharding, as the reference's generate.py:119-120
    prompt_ids = shard_prompts(world, rank, args.batch)
    cond = conditioning(model, prompt_ids, dev)
    dit = model.model.model
    dit.set_gemm_dtype(args.dtype)
    from stable_audio_tools import _config
    codec_dtype = _config.codec_gemm_dtype(args.dtype)        # one rule, shared with generate.py (fp16 = the reference's model_half)
    model.pretransform.model.set_gemm_dtype(codec_dtype)
    dit.set_layernorm_fusion(args.layernorm == "fused")
    dit.set_cross_attention_fusion(args.cross_attention == "fused")

    from stable_audio_tools import _hip
    lib = _hip.lib()
    for i in range(args.warmup):
        one_generation(model, cond, 1000 + i, dev, world)
    last = {}

    def step(seed):
        last["audio"] = one_generation(model, cond, seed, dev, world)

    elapsed = timed_steps(step, args.steps, use_dist, torch.cuda.synchronize, dev)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, last)

    if args.full:
        # dominant kernel: FFN-in SwiGLU GEMM, timed live with HIP events on the launch stream (one layer per forward), in a pass of
        # --steps generations of its own after the headline's timed steps (the events stay out of the headline)
        dit._ensure_plan()                              # --warmup 0: the plan is otherwise built lazily by the first generation
        _hip.check(lib.sat_dit_profile(dit._plan, 1))
        for i in range(args.steps):
            one_generation(model, cond, 3000 + i, dev, world)
        tot = ctypes.c_double()
        cnt = ctypes.c_int32()
        m, n, k = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        _hip.check(lib.sat_dit_profile_read(dit._plan, ctypes.byref(tot), ctypes.byref(cnt), ctypes.byref(m), ctypes.byref(n), ctypes.byref(k)))
        _hip.check(lib.sat_dit_profile(dit._plan, 0))

    if rank == 0:
        audio_seconds = world * args.batch * (SAMPLE_SIZE / SAMPLE_RATE) * args.steps
        line = {
            "metric": "audio-seconds/sec @44.1kHz stereo, 100-step DPM++, SA-Open-1.0 shape" if args.workload == "sa_open" else
                      "audio-seconds/sec @44.1kHz stereo, 100-step DPM++, SA-2.0 shape audio-to-audio (encode + sample + decode)",
            "value": audio_seconds / elapsed,
            "unit": "audio-seconds/sec",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1e3,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": args.dtype if not args.dtype.startswith("fp8") else
                     {"fp8": "fp8 e4m3 (cross to_q, FF-in, FF-out; per-token / MX-32 x per-channel scales) + bf16, fp32 accumulate",
                      "fp8-all": "fp8 e4m3 (every GEMM of the blocks) + bf16, fp32 accumulate"}[args.dtype],
            "data": "synthetic (random-init weights of the SA-Open-1.0 / SA-2.0 DiT + Oobleck architecture, random text embeddings)",
            "config": {"workload": ("Stable-Audio-Open-1.0 DiT shape (24 layers, D=1536, S=1025, CFG 7 -> 2 sequences/prompt) + Oobleck decode, "
                                    f"{args.batch} prompt(s)/GPU x 47.55 s, 100 DPM-Solver++(3M) SDE steps") if args.workload == "sa_open" else
                                   ("Stable Audio 2.0 shape (24 layers, D=1536, S=6145, CFG 7) audio-to-audio: Oobleck encode of 285.3 s init audio + "
                                    f"100 DPM-Solver++(3M) SDE steps from sigma 7 + decode, {args.batch} prompt(s)/GPU"), "prompts_per_gpu": args.batch,
                       "codec_dtype": codec_dtype, "sampler_steps": DIT_STEPS, "cfg_scale": CFG_SCALE, "layernorm": args.layernorm, "cross_attention": args.cross_attention, "sample_size": SAMPLE_SIZE, "parallelism": f"dp{world} (rank-strided prompts, one all-gather)"},
            **({"roofline": roofline(args, tot.value, cnt.value, m.value, n.value, k.value)} if args.full else {}),
            "rccl_ranks": world if use_dist else 0,
        }
        if cpu_base:
            line["cpu_baseline"] = cpu_baseline(sd)
        print(json.dumps(line), flush=True)
    if use_dist:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
