"""The fp32 build of the Oobleck codec (``set_gemm_dtype("fp32")``, sat_oobleck_cfg.gemm_dtype = SAT_GEMM_FP32X): fp32 activations and
weights through every convolution on the exact f32-input MFMA, the reference's ``model_half=False`` arithmetic.

What separates it from the fp32 oracle / the reference's fp32 outputs is summation order (fmaf chains grouped differently) and
``sinf`` against torch's sin: ~1e-6.  Gates are 1e-5 everywhere, against 7e-4 (fp16) / 7e-3 (bf16) for the 16-bit builds.

The reference goldens ``small_decode`` / ``small_encode`` and ``vae_chunked.npz`` come from a 16-channel codec, which no build of the HIP
codec runs (channels must be a multiple of 64); the chunked paths are compared with the fp32 oracle on the reduced 64-channel VAE instead."""
import json
import math
import os
import runpy
import sys

import pytest
import torch
import torch.nn.functional as F

from util import SUITE, assert_close, rel_l2

pytestmark = pytest.mark.gpu

TOL = 1e-5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "friendly-stable-audio-tools_amd")


def _sub(sd, prefix):
    return {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}


def _build(cfg, seed, dev):
    import stable_audio_tools as S
    from stable_audio_tools import synthetic
    from stable_audio_tools.models import _init
    with _init.skip_init():
        model = S.create_model_from_config(cfg)
    sd = synthetic.synth_state_dict(model.state_dict(), seed)
    model.load_state_dict(sd)
    return model.to(dev).eval(), sd


@pytest.fixture(scope="module")
def vae32(dev):
    """The reduced VAE of test_gpu_models.py (same config and seed), switched to the fp32 codec."""
    from stable_audio_tools import model_configs as MC
    cfg = MC.reduced(MC.stable_audio_vae())
    model, sd = _build(cfg, 3, dev)
    model.set_gemm_dtype("fp32")
    yield cfg, model, sd
    model.set_gemm_dtype(SUITE.gemm_dtype)


@pytest.mark.parametrize("b,t_len", [(1, 43), (2, 8), (1, 1)])
def test_decode_fp32_vs_oracle(dev, vae32, b, t_len):
    from oracle import oobleck as oob
    from stable_audio_tools import synthetic
    cfg, model, sd = vae32
    z = synthetic.synth_input("z", (b, 64, t_len), 11)
    got = model.decode(z.to(dev))
    want = oob.oobleck_decoder(_sub(sd, "decoder."), z, strides=cfg["model"]["decoder"]["config"]["strides"])
    assert got.shape == want.shape
    e = assert_close("fp32 decode vs fp32 oracle", got, want, TOL)
    print(f"\n[fp32 decode b={b} T={t_len}] rel-L2 vs fp32 oracle {e:.2e}")


@pytest.mark.parametrize("b,t_len", [(1, 21), (2, 4)])
def test_encode_fp32_and_vae_sample_vs_oracle(dev, vae32, b, t_len):
    from oracle import oobleck as oob
    from stable_audio_tools import synthetic
    cfg, model, sd = vae32
    ratio = cfg["model"]["downsampling_ratio"]
    audio = synthetic.synth_input("a", (b, 2, t_len * ratio), 12, 0.4)
    want = oob.oobleck_encoder(_sub(sd, "encoder."), audio, strides=cfg["model"]["encoder"]["config"]["strides"])
    noise = synthetic.synth_input("vn", (b, 64, t_len), 13)
    got = model.encoder(audio.to(dev))
    z = model.encode(audio.to(dev), noise=noise.to(dev))
    e = assert_close("fp32 encode vs fp32 oracle", got, want, TOL)
    e2 = assert_close("fp32 encode + vae_sample", z, oob.vae_sample(want, noise), TOL)
    print(f"\n[fp32 encode b={b} T={t_len}] rel-L2 vs fp32 oracle {e:.2e}, after vae_sample {e2:.2e}")


def test_full_size_codec_fp32_vs_reference_golden(dev):
    """BASELINE config 1 shape, the reference's own fp32 outputs (tests/golden/vae.npz): decode z[1,64,43] -> [1,2,88064] and
    encode 16 latent frames of audio.  The 16-bit builds sit at 7.4e-4 / 7.0e-4 (fp16) here (test_gpu_models.py)."""
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import cases
    from stable_audio_tools import synthetic
    from stable_audio_tools.models import _init
    from stable_audio_tools.models.autoencoders import OobleckDecoder, OobleckEncoder
    g = cases.load("vae")
    with _init.skip_init():
        dec = OobleckDecoder(**cases.vae_kwargs(cases.FULL_VAE, True))
    dec.load_state_dict(synthetic.synth_state_dict(dec.state_dict(), 0))
    dec = dec.to(dev)
    z = synthetic.synth_input("z_full", (1, 64, 43), 1).to(dev)
    e16 = rel_l2(dec.set_gemm_dtype("fp16")(z), g["full_decode_T43"])
    e = assert_close("full-size fp32 decode vs reference", dec.set_gemm_dtype("fp32")(z), g["full_decode_T43"], TOL)
    with _init.skip_init():
        enc = OobleckEncoder(**cases.vae_kwargs(cases.FULL_VAE, False))
    enc.load_state_dict(synthetic.synth_state_dict(enc.state_dict(), 0))
    enc = enc.to(dev)
    a = synthetic.synth_input("a_full", (1, 2, 2048 * 16), 2, 0.3).to(dev)
    e2_16 = rel_l2(enc.set_gemm_dtype("fp16")(a), g["full_encode_T16"])
    e2 = assert_close("full-size fp32 encode vs reference", enc.set_gemm_dtype("fp32")(a), g["full_encode_T16"], TOL)
    print(f"\n[full codec vs the reference's fp32 output] decode fp32 {e:.2e} (fp16 {e16:.2e}), encode fp32 {e2:.2e} (fp16 {e2_16:.2e})")


def test_chunked_codec_paths_fp32_vs_oracle(dev, vae32):
    """AudioAutoencoder.decode_audio (chunked and not), encode_audio (chunked) and reconstruct_audio in fp32, VAE noise injected."""
    from oracle import oobleck as oob
    from stable_audio_tools import synthetic
    cfg, vae, sd = vae32
    ratio = cfg["model"]["downsampling_ratio"]
    dsd, esd = _sub(sd, "decoder."), _sub(sd, "encoder.")
    estr = cfg["model"]["encoder"]["config"]["strides"]
    dec = lambda z: oob.oobleck_decoder(dsd, z, strides=cfg["model"]["decoder"]["config"]["strides"])
    z = synthetic.synth_input("zc", (2, 64, 23), 51)
    got = vae.decode_audio(z.to(dev), chunked=True, chunk_size=8, overlap=2, max_batch_size=3)
    e_dc = assert_close("fp32 decode_audio chunked", got, oob.decode_audio_chunked(dec, z, 8, 2, ratio), TOL)
    e_du = assert_close("fp32 decode_audio unchunked", vae.decode_audio(z.to(dev)), dec(z), TOL)

    audio = synthetic.synth_input("ac", (1, 2, 19 * ratio), 52, 0.3)
    noises = [synthetic.synth_input(f"vn{i}", (2, 64, 8), 60 + i) for i in range(4)]
    calls = {"i": 0}
    orig_encode = vae.bottleneck.encode

    def encode_with_noise(x, return_info=False, **kw):
        nz = noises[calls["i"]][: x.shape[0]].to(x.device)
        calls["i"] += 1
        return orig_encode(x, return_info=return_info, noise=nz)

    vae.bottleneck.encode = encode_with_noise
    try:
        got = vae.encode_audio(audio.to(dev), chunked=True, chunk_size=8, overlap=2, max_batch_size=2)
        calls["i"] = 0
        rec = vae.reconstruct_audio(audio.to(dev), chunked=True, chunk_size=8, overlap=2, max_batch_size=2)
    finally:
        vae.bottleneck.encode = orig_encode
    it = {"i": 0}

    def enc_chunks(chunks):
        outs = []
        for i in range(0, len(chunks), 2):
            grp = torch.cat(chunks[i:i + 2], dim=0)
            outs += list(oob.vae_sample(oob.oobleck_encoder(esd, grp, strides=estr), noises[it["i"]][: grp.shape[0]]).split(1, dim=0))
            it["i"] += 1
        return outs

    cs, hop = 8 * ratio, 6 * ratio
    n_chunk = int(math.ceil((audio.shape[-1] - cs) / hop)) + 1
    padded = F.pad(audio, (0, cs + hop * (n_chunk - 1) - audio.shape[-1]))
    zs = iter(enc_chunks([padded[..., i * hop: i * hop + cs] for i in range(n_chunk)]))
    e_ec = assert_close("fp32 encode_audio chunked", got, oob.encode_audio_chunked(lambda c: next(zs), audio, 8, 2, ratio, 64), TOL)
    it["i"] = 0
    padded = F.pad(audio, (0, cs + hop * n_chunk - audio.shape[-1]))
    outs = iter([dec(zz) for zz in enc_chunks([padded[..., i * hop: i * hop + cs] for i in range(n_chunk)])])
    e_rc = assert_close("fp32 reconstruct_audio chunked", rec, oob.reconstruct_audio_chunked(lambda c, i: next(outs), audio, 8, 2, ratio), TOL)
    print(f"\n[fp32 chunked] decode {e_dc:.2e}, unchunked decode {e_du:.2e}, encode {e_ec:.2e}, reconstruct {e_rc:.2e}")


def test_switching_formats_is_clean(dev):
    from stable_audio_tools import model_configs as MC, synthetic
    cfg = MC.reduced(MC.stable_audio_vae())
    model, sd = _build(cfg, 4, dev)
    z = synthetic.synth_input("zs", (1, 64, 9), 14).to(dev)
    first = model.decode(z)
    mid = model.set_gemm_dtype("fp32").decode(z)
    last = model.set_gemm_dtype(SUITE.gemm_dtype).decode(z)
    assert torch.equal(first, last), "switching back from fp32 must restore the suite's format bit for bit"
    assert not torch.equal(first, mid)
    import ctypes
    from stable_audio_tools import _hip
    need = {}
    for fmt in ("fp16", "fp32"):
        model.set_gemm_dtype(fmt).decode(z)
        n = ctypes.c_size_t()
        _hip.check(_hip.lib().sat_oobleck_workspace_bytes(model.decoder._plan, 1, 9, ctypes.byref(n)))
        need[fmt] = n.value
    model.set_gemm_dtype(SUITE.gemm_dtype)
    assert 2 * need["fp16"] - 1024 <= need["fp32"] <= 2 * need["fp16"], need


def test_fp32_codec_keeps_activations_past_fp16_range(dev):
    """A checkpoint whose activations leave the fp16 range: the last ResidualUnit's 1 x 1 convolution scaled up so that the stream entering
    the final Snake reaches ~1e5 (and the folded weights ~7e4).  The fp16 build saturates at 65504 and misses the oracle; fp32 matches it."""
    from oracle import oobleck as oob
    from stable_audio_tools import model_configs as MC, synthetic
    cfg = MC.reduced(MC.stable_audio_vae())
    model, sd = _build(cfg, 3, dev)
    key = "decoder.layers.3.layers.4.layers.3.weight_g"
    sd = dict(sd)
    sd[key] = sd[key] * 5e5
    model.load_state_dict(sd)
    dsd = _sub(sd, "decoder.")
    strides = cfg["model"]["decoder"]["config"]["strides"]
    z = synthetic.synth_input("zr", (1, 64, 12), 31)
    peak = [0.0]

    def track(x):
        peak[0] = max(peak[0], x.abs().max().item())
        return x

    want = oob.oobleck_decoder(dsd, z, strides=strides, rnd=track)
    assert peak[0] > 1.5 * 65504, peak
    got16 = model.set_gemm_dtype("fp16").decode(z.to(dev))
    got32 = model.set_gemm_dtype("fp32").decode(z.to(dev))
    model.set_gemm_dtype(SUITE.gemm_dtype)
    e16 = rel_l2(got16, want)
    e32 = assert_close("fp32 decode past the fp16 range", got32, want, TOL)
    print(f"\n[range] activation peak {peak[0]:.3g}: fp16 build rel-L2 {e16:.2e}, fp32 build {e32:.2e}")
    assert e16 > 1e-2, f"the fp16 build was expected to saturate (rel-L2 {e16:.2e})"


def test_generate_with_fp32_codec(dev):
    """generate_diffusion_cond on the reduced SA-Open model with ``pretransform.model.set_gemm_dtype("fp32")``: the decoded audio is the
    fp32 oracle decode of the very latents the sampler produced."""
    from oracle import oobleck as oob
    from stable_audio_tools import model_configs as MC, synthetic
    from stable_audio_tools.inference.generation import generate_diffusion_cond
    cfg = MC.reduced(MC.stable_audio_open_1_0())
    model, sd = _build(cfg, 0, dev)
    model.pretransform.model.set_gemm_dtype("fp32")
    dc = cfg["model"]["diffusion"]["config"]
    b, t_len = 2, 16
    ratio = cfg["model"]["pretransform"]["config"]["downsampling_ratio"]
    cond = model.conditioner([{"seconds_start": 0, "seconds_total": 10 + i} for i in range(b)])
    cond["prompt"] = (synthetic.synth_input("prompt", (b, 128, dc["cond_token_dim"]), 31).to(dev), torch.ones(b, 128, device=dev))
    cond = {k: cond[k] for k in ("prompt", "seconds_start", "seconds_total")}
    kw = dict(steps=3, cfg_scale=7.0, conditioning_tensors=cond, sample_size=t_len * ratio, seed=9, device=str(dev),
              sampler_type="dpmpp-3m-sde", sigma_min=0.3, sigma_max=500)
    lat = generate_diffusion_cond(model, return_latents=True, **kw)
    audio = generate_diffusion_cond(model, **kw)
    strides = cfg["model"]["pretransform"]["config"]["decoder"]["config"]["strides"]
    want = oob.oobleck_decoder(_sub(sd, "pretransform.model.decoder."), lat.cpu() * model.pretransform.scale, strides=strides)
    e = assert_close("generate, fp32 codec vs fp32 oracle decode", audio, want, TOL)
    print(f"\n[generate, fp32 codec] audio rel-L2 vs fp32 oracle decode of the same latents {e:.2e}")


def _run_script(name, argv):
    old = sys.argv
    sys.argv = [name] + argv
    try:
        runpy.run_path(os.path.join(PKG, name), run_name="__main__")
    finally:
        sys.argv = old


def test_scripts_with_fp32_codec(dev, tmp_path):
    """reconstruct_audios.py and generate.py with --codec-dtype fp32 on the reduced configs: the WAVs are the in-process fp32 results."""
    import stable_audio_tools as S
    import yaml
    from safetensors.torch import save_file
    from stable_audio_tools import model_configs as MC, synthetic
    from stable_audio_tools.data.modification import Stereo
    from stable_audio_tools.inference.generation import generate_diffusion_cond
    from stable_audio_tools.models import _init
    from stable_audio_tools.utils.audio_utils import float_to_int16_audio
    from stable_audio_tools.utils.wav_io import load_wav, save_wav_float

    # ---- reconstruct_audios.py
    cfg = MC.reduced(MC.stable_audio_vae())
    cfg_path, ckpt_path = tmp_path / "vae.json", tmp_path / "vae.safetensors"
    json.dump(cfg, open(cfg_path, "w"))
    with _init.skip_init():
        model = S.create_model_from_config(cfg)
    sd = synthetic.synth_state_dict(model.state_dict(), 12)
    save_file({k: v.contiguous() for k, v in sd.items()}, str(ckpt_path))
    model.load_state_dict(sd)
    model = model.to(dev).eval().set_gemm_dtype("fp32")
    sr, ratio = model.sample_rate, model.downsampling_ratio
    in_dir = tmp_path / "in"
    in_dir.mkdir()
    x = synthetic.synth_input("wav_a", (2, 7000), 1, 0.2)
    save_wav_float(in_dir / "a.wav", x, sr)
    out_dir = tmp_path / "rec" / "reconstructed"
    torch.manual_seed(21)
    _run_script("reconstruct_audios.py", ["--audio-dir", str(in_dir), "--output-dir", str(out_dir), "--model-config", str(cfg_path),
                                          "--ckpt-path", str(ckpt_path), "--frame-duration", str((16 * ratio + 0.5) / sr), "--overlap-rate", "0.1",
                                          "--batch-size", "3", "--codec-dtype", "fp32"])
    torch.manual_seed(21)
    xin, _ = load_wav(in_dir / "a.wav")
    rec = model.reconstruct_audio(Stereo()(xin).unsqueeze(0).to(dev), chunked=True, chunk_size=16, overlap=1, max_batch_size=3).squeeze(0)
    got, got_sr = load_wav(out_dir / "a.wav")
    want = (rec.cpu().float().clamp(-1, 1) * 32767.0).round().to(torch.int16)
    diff = ((got * 32768.0).round().to(torch.int16).int() - want.int()).abs().max().item()
    assert got_sr == sr and got.shape == (2, 7000) and diff <= 1, f"reconstruct_audios.py --codec-dtype fp32 differs by {diff} LSB"

    # ---- generate.py
    cfg = MC.reduced(MC.stable_audio_open_1_0())
    cfg_path, ckpt_path = tmp_path / "model_config.json", tmp_path / "model.safetensors"
    json.dump(cfg, open(cfg_path, "w"))
    with _init.skip_init():
        model = S.create_model_from_config(cfg)
    sd = synthetic.synth_state_dict(model.state_dict(), 11)
    save_file({k: v.contiguous() for k, v in sd.items()}, str(ckpt_path))
    model.load_state_dict(sd)
    model = model.to(dev).eval()
    model.pretransform.model.set_gemm_dtype("fp32")
    cond_dim = cfg["model"]["conditioning"]["cond_dim"]
    yaml.safe_dump({"demo": {"pad": {"prompt": "warm analog pad", "seconds_start": 0, "seconds_total": 0.04}}}, open(tmp_path / "c.yaml", "w"))
    emb = synthetic.synth_input("emb", (7, cond_dim), 50)
    torch.save({"warm analog pad": emb}, tmp_path / "embeds.pt")
    out_dir = tmp_path / "gen"
    _run_script("generate.py", ["--output-dir", str(out_dir), "--cond-yaml-path", str(tmp_path / "c.yaml"), "--model-config", str(cfg_path),
                                "--ckpt-path", str(ckpt_path), "--text-embeds", str(tmp_path / "embeds.pt"), "--sample-steps", "3",
                                "--batch-size", "2", "--n-sample-per-cond", "1", "--clip-length", "--seed", "3", "--cfg-scale", "7.0",
                                "--codec-dtype", "fp32"])
    cond = model.conditioner([{"seconds_start": 0, "seconds_total": 0.04}])
    cond["prompt"] = (emb.unsqueeze(0).to(dev), torch.ones(1, 7, device=dev))
    cond = {k: cond[k] for k in ("prompt", "seconds_start", "seconds_total")}
    audio = generate_diffusion_cond(model, steps=3, cfg_scale=7.0, conditioning_tensors=cond, sample_size=cfg["sample_size"], sigma_min=0.3,
                                    sigma_max=500, sampler_type="dpmpp-3m-sde", device=str(dev), seed=3)
    want = float_to_int16_audio(audio[0])[:, : int(0.04 * cfg["sample_rate"])]
    got, _ = load_wav(out_dir / "demo" / "pad_item-1.wav")
    diff = ((got * 32768.0).round().to(torch.int16).int() - want.int()).abs().max().item()
    assert got.shape == want.shape and diff <= 1, f"generate.py --codec-dtype fp32 differs by {diff} LSB"
