"""The Oobleck configurations beside the Stable Audio VAE on the device, in all three operand formats: ELU, nearest-neighbour upsampling
(three-tap polyphase form), the final tanh and channel counts that are not multiples of 64, against the REFERENCE's fp32 outputs
(tests/golden/codec_options.npz, written by tests/golden/make_golden_codec_options.py); and, for the first time on the device, the
reference's 16-channel goldens ``vae.npz`` small_decode / small_encode and ``vae_chunked.npz``.

Gates are the project's codec gates against fp32 reference output: 1.5e-2 (bf16) and 3.75e-3 (fp16) from ``CODEC`` in
tests/test_gpu_models.py, 1e-5 (fp32) from ``TOL`` in tests/test_gpu_codec_fp32.py."""
import ctypes
import os
import sys

import pytest
import torch

from util import NAN_BYTE, WORKSPACE_FILLS, assert_bit_equal, assert_close, rel_l2
from test_gpu_codec_fp32 import TOL as TOL_FP32
from test_gpu_models import CODEC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
import cases  # noqa: E402
import make_golden_codec_options as GO  # noqa: E402  (case table and seeds; does not import the reference)

pytestmark = pytest.mark.gpu

GATE = {"bf16": CODEC["bf16"][1], "fp16": CODEC["fp16"][1], "fp32": TOL_FP32}
FMTS = ["fp16", "bf16", "fp32"]
NAMES = sorted(GO.CONFIGS)


def _codec(name, dev, fmt):
    """AudioAutoencoder of config `name` as a user gets it: final_tanh=False in the config, set_final_tanh(True) afterwards."""
    import stable_audio_tools as S
    from stable_audio_tools.models import _init
    with _init.skip_init():
        model = S.create_model_from_config(GO.model_config(name))
    model.decoder.load_state_dict(GO.synth_decoder_sd(name, model.decoder.state_dict()))
    model.encoder.load_state_dict(GO.synth_encoder_sd(name, model.encoder.state_dict()))
    model = model.to(dev).eval().set_gemm_dtype(fmt)
    if GO.CONFIGS[name]["final_tanh"]:
        model.set_final_tanh(True)
    return model


@pytest.fixture(scope="module")
def golden():
    return cases.load("codec_options")


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("name", NAMES)
def test_decode_and_encode_vs_reference(dev, golden, name, fmt):
    model = _codec(name, dev, fmt)
    z, z1, audio = GO.inputs(name)
    tol = GATE[fmt]
    got = model.decode(z.to(dev))
    got1 = model.decode(z1.to(dev))
    lat = model.encoder(audio.to(dev))
    figures = {k: rel_l2(g, golden[f"{name}/{k}"]) for k, g in (("decode", got), ("decode_T1", got1), ("encode", lat))}
    print(f"\n[{name}, {fmt}] rel-L2 vs the reference's fp32 output: " + ", ".join(f"{k} {v:.2e}" for k, v in figures.items()))
    for k, g in (("decode", got), ("decode_T1", got1), ("encode", lat)):
        assert g.shape == golden[f"{name}/{k}"].shape
        assert_close(f"{name} {k} ({fmt})", g, golden[f"{name}/{k}"], tol)
    if GO.CONFIGS[name]["final_tanh"]:
        assert got.abs().max().item() <= 1.0 and got1.abs().max().item() <= 1.0
        # set_final_tanh(False) gives the un-squashed audio back: far from the golden, and its tanh is the golden again
        raw = model.set_final_tanh(False).decode(z.to(dev))
        assert raw.abs().max().item() > 1.0
        assert rel_l2(raw, golden[f"{name}/decode"]) >= 0.5 * GO.MIN_TANH_EFFECT
        assert_close(f"{name} tanh(un-squashed) ({fmt})", torch.tanh(raw), golden[f"{name}/decode"], tol)
        model.set_final_tanh(True)
        assert torch.equal(model.decode(z.to(dev)), got)


@pytest.mark.parametrize("fmt", FMTS)
def test_pad_channels_do_not_read_stale_workspace(dev, golden, fmt):
    """narrow_all (widths 48 / 96 / 144, latent 20) pads every tensor of the workspace; the pad channels must be WRITTEN as zeros by
    the producers, not inherited: with the cached workspace filled with NaN patterns before the call the gate still holds -- and, under
    every fill of util.WORKSPACE_FILLS, the outputs are the bits of the un-poisoned run of the same module (the gate alone dilutes one stale
    pad row among all the correct ones)."""
    name = "narrow_all"
    model = _codec(name, dev, fmt)
    z, _, audio = GO.inputs(name)
    clean_d = model.decode(z.to(dev))
    clean_e = model.encoder(audio.to(dev))
    assert_bit_equal(f"narrow_all decode twice ({fmt}): the call is not repeatable", model.decode(z.to(dev)), clean_d)
    assert_bit_equal(f"narrow_all encode twice ({fmt}): the call is not repeatable", model.encoder(audio.to(dev)), clean_e)
    for byte in WORKSPACE_FILLS:
        for part in (model.decoder, model.encoder):
            assert part._ws is not None and part._ws.dtype == torch.uint8
            part._ws.fill_(byte)
        ws_d, ws_e = model.decoder._ws, model.encoder._ws
        got = model.decode(z.to(dev))
        lat = model.encoder(audio.to(dev))
        assert model.decoder._ws is ws_d and model.encoder._ws is ws_e      # the poisoned buffers are the ones that ran
        if byte == NAN_BYTE:
            e = assert_close(f"narrow_all decode on a NaN workspace ({fmt})", got, golden[f"{name}/decode"], GATE[fmt])
            e2 = assert_close(f"narrow_all encode on a NaN workspace ({fmt})", lat, golden[f"{name}/encode"], GATE[fmt])
            print(f"\n[narrow_all on a NaN-filled workspace, {fmt}] decode {e:.2e}, encode {e2:.2e}")
        assert_bit_equal(f"narrow_all decode on a workspace of 0x{byte:02X} bytes ({fmt})", got, clean_d)
        assert_bit_equal(f"narrow_all encode on a workspace of 0x{byte:02X} bytes ({fmt})", lat, clean_e)


# ------------------------------------------------------------------------------- the reference's 16-channel goldens, on the device
def _small_vae(dev, fmt):
    from stable_audio_tools import synthetic
    from stable_audio_tools.models import _init
    from stable_audio_tools.models.autoencoders import AudioAutoencoder, OobleckDecoder, OobleckEncoder
    from stable_audio_tools.models.bottleneck import VAEBottleneck
    with _init.skip_init():
        dec = OobleckDecoder(**cases.vae_kwargs(cases.SMALL_VAE, True))
        enc = OobleckEncoder(**cases.vae_kwargs(cases.SMALL_VAE, False))
    dec.load_state_dict(synthetic.synth_state_dict(dec.state_dict(), 5))
    enc.load_state_dict(synthetic.synth_state_dict(enc.state_dict(), 6))
    ae = AudioAutoencoder(enc, dec, latent_dim=64, downsampling_ratio=2048, sample_rate=44100, io_channels=2, bottleneck=VAEBottleneck())
    return ae.to(dev).eval().set_gemm_dtype(fmt)


@pytest.mark.parametrize("fmt", FMTS)
def test_small_vae_reference_goldens(dev, fmt):
    """vae.npz small_decode / small_encode (cases.SMALL_VAE: 16 channels, stage widths 16 ... 256), inputs as make_golden.py gen_vae."""
    from stable_audio_tools import synthetic
    g = cases.load("vae")
    ae = _small_vae(dev, fmt)
    z = synthetic.synth_input("z", (2, 64, 9), 7)
    a = synthetic.synth_input("a", (2, 2, 2048 * 5), 8, 0.3)
    e = assert_close(f"small_decode ({fmt})", ae.decoder(z.to(dev)), g["small_decode"], GATE[fmt])
    e2 = assert_close(f"small_encode ({fmt})", ae.encoder(a.to(dev)), g["small_encode"], GATE[fmt])
    print(f"\n[16-channel VAE vs the reference, {fmt}] decode {e:.2e}, encode {e2:.2e}")


def _reference_vae_draws(seed, batch_sizes, frames):
    """The reference's VAE noise: manual_seed, then one ``randn_like(mean)`` per encode batch in chunk-batch order (CPU generator; mean
    is the first half of the encoder output, as in tests/test_oracle_golden.py::test_chunked_codec_paths)."""
    torch.manual_seed(seed)
    return [torch.randn_like(torch.empty(bs, 128, frames)[:, :64]) for bs in batch_sizes]


@pytest.mark.parametrize("fmt", FMTS)
def test_chunked_paths_vs_reference_goldens(dev, fmt):
    """All four arrays of vae_chunked.npz through AudioAutoencoder.reconstruct_audio / encode_audio / decode_audio with the chunk
    settings of make_golden.py gen_vae; the reference's Gaussian draws are reproduced on the CPU and injected into the bottleneck."""
    from stable_audio_tools import synthetic
    g = cases.load("vae_chunked")
    ae = _small_vae(dev, fmt)
    tol = GATE[fmt]
    sig = synthetic.synth_input("sig", (1, 2, 2048 * 11 + 700), 9, 0.3)[..., : 2048 * 11].contiguous()
    orig_encode = ae.bottleneck.encode
    state = {}

    def encode_with_noise(x, return_info=False, **kw):
        nz = state["draws"][state["i"]]
        state["i"] += 1
        assert nz.shape[0] == x.shape[0] and nz.shape[2] == x.shape[2]
        return orig_encode(x, return_info=return_info, noise=nz.to(x.device))

    ae.bottleneck.encode = encode_with_noise
    try:
        state.update(draws=_reference_vae_draws(77, [3, 1], 4), i=0)      # 4 windows of 4 frames, batches of 3
        rec = ae.reconstruct_audio(sig.to(dev), chunked=True, chunk_size=4, overlap=1, max_batch_size=3)
        assert state["i"] == 2
        state.update(draws=_reference_vae_draws(78, [2, 2], 4), i=0)      # 4 windows, batches of 2
        enc = ae.encode_audio(sig.to(dev), chunked=True, chunk_size=4, overlap=1, max_batch_size=2)
        assert state["i"] == 2
    finally:
        ae.bottleneck.encode = orig_encode
    zz = synthetic.synth_input("zz", (1, 64, 11), 10)
    dc = ae.decode_audio(zz.to(dev), chunked=True, chunk_size=4, overlap=1, max_batch_size=2)
    du = ae.decode_audio(zz.to(dev), chunked=False)
    got = {"reconstruct_chunked": rec, "encode_chunked": enc, "decode_chunked": dc, "decode_unchunked": du}
    print(f"\n[16-channel VAE, chunked paths vs the reference, {fmt}] " + ", ".join(f"{k} {rel_l2(v, g[k]):.2e}" for k, v in got.items()))
    for k, v in got.items():
        assert v.shape == g[k].shape, k
        assert_close(f"{k} ({fmt})", v, g[k], tol)


# ------------------------------------------------------------------------------- the default path is untouched
@pytest.mark.parametrize("fmt", FMTS)
def test_old_entry_point_and_default_options_are_bit_identical(dev, fmt):
    """The full-size Stable Audio decoder and encoder through sat_oobleck_plan_create and through sat_oobleck_plan_create_ex with default
    options (what the Python package calls): the same bits."""
    from stable_audio_tools import _hip, synthetic
    from stable_audio_tools.models import _init
    from stable_audio_tools.models.autoencoders import _CODEC_GEMM_DTYPES, OobleckDecoder, OobleckEncoder
    lib = _hip.lib()

    def through_old_entry(mod, x, out_shape, t_len):
        cfg = _hip.SatOobleckCfg()
        cfg.is_decoder, cfg.io_channels, cfg.channels, cfg.latent_dim = int(mod._is_decoder), mod.io_channels, mod.channels, mod.latent_dim
        cfg.n_blocks = len(mod.strides)
        for i, (c, s) in enumerate(zip(mod.c_mults, mod.strides)):
            cfg.c_mults[i], cfg.strides[i] = c, s
        cfg.gemm_dtype = _CODEC_GEMM_DTYPES[fmt]
        plan = ctypes.c_void_p()
        _hip.check(lib.sat_oobleck_plan_create(ctypes.byref(cfg), ctypes.byref(plan)))
        try:
            keep = [(n, t.detach().float().contiguous()) for n, t in mod.state_dict().items()]
            for n, t in keep:
                _hip.check(lib.sat_oobleck_plan_set_tensor(plan, n.encode(), _hip.ptr(t), t.numel()))
            _hip.check(lib.sat_oobleck_plan_finalize(plan, _hip.stream()))
            need = ctypes.c_size_t()
            _hip.check(lib.sat_oobleck_workspace_bytes(plan, x.shape[0], t_len, ctypes.byref(need)))
            ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
            out = torch.empty(out_shape, dtype=torch.float32, device=dev)
            fn = lib.sat_oobleck_decode if mod._is_decoder else lib.sat_oobleck_encode
            _hip.check(fn(plan, _hip.ptr(x), _hip.ptr(out), x.shape[0], t_len, _hip.ptr(ws), ws.numel(), _hip.stream()))
            torch.cuda.synchronize()
            return out
        finally:
            lib.sat_oobleck_plan_destroy(plan)

    with _init.skip_init():
        dec = OobleckDecoder(**cases.vae_kwargs(cases.FULL_VAE, True))
        enc = OobleckEncoder(**cases.vae_kwargs(cases.FULL_VAE, False))
    dec.load_state_dict(synthetic.synth_state_dict(dec.state_dict(), 0))
    enc.load_state_dict(synthetic.synth_state_dict(enc.state_dict(), 0))
    dec, enc = dec.to(dev).set_gemm_dtype(fmt), enc.to(dev).set_gemm_dtype(fmt)
    z = synthetic.synth_input("z_full", (1, 64, 43), 1).to(dev)
    a = synthetic.synth_input("a_full", (1, 2, 2048 * 16), 2, 0.3).to(dev)
    new_d, new_e = dec(z), enc(a)
    assert torch.equal(through_old_entry(dec, z, new_d.shape, 43), new_d)
    assert torch.equal(through_old_entry(enc, a, new_e.shape, 16), new_e)
    g = cases.load("vae")
    assert_close(f"full-size decode ({fmt})", new_d, g["full_decode_T43"], GATE[fmt])
    assert_close(f"full-size encode ({fmt})", new_e, g["full_encode_T16"], GATE[fmt])


# ------------------------------------------------------------------------------- through generate_diffusion_cond
@pytest.mark.parametrize("fmt", FMTS)
def test_generate_with_a_narrow_pretransform(dev, fmt):
    """generate_diffusion_cond on a reduced model whose pretransform is narrow_all (20 latent channels, ELU, nearest upsampling, tanh):
    the plumbing from the sampler's 20-channel latents to audio.  What is checked is shape, finiteness, |audio| <= 1 (the tanh ran) and
    that the audio is not silent.  The last comparison, with the pretransform's decode of the latents of a second identical run, only
    shows that the two runs agree: it would pass for a wrong decode.  That narrow_all decodes correctly is the business of
    test_decode_and_encode_vs_reference and test_pad_channels_do_not_read_stale_workspace above (the fixtures store no reference
    decode of sampled latents)."""
    import stable_audio_tools as S
    from stable_audio_tools import model_configs as MC, synthetic
    from stable_audio_tools.inference.generation import generate_diffusion_cond
    from stable_audio_tools.models import _init
    name = "narrow_all"
    cfg = MC.reduced(MC.stable_audio_open_1_0())
    vae = GO.model_config(name)["model"]
    latent = vae["latent_dim"]
    cfg["model"]["pretransform"]["config"] = vae
    cfg["model"]["io_channels"] = latent
    cfg["model"]["diffusion"]["config"]["io_channels"] = latent
    with _init.skip_init():
        model = S.create_model_from_config(cfg)
    model.load_state_dict(synthetic.synth_state_dict(model.state_dict(), 4))
    codec = model.pretransform.model
    codec.decoder.load_state_dict(GO.synth_decoder_sd(name, codec.decoder.state_dict()))
    model = model.to(dev).eval()
    codec.set_gemm_dtype(fmt).set_final_tanh(True)
    dc = cfg["model"]["diffusion"]["config"]
    b, steps, t_len = 2, 3, 16
    ratio = GO.ratio(name)
    cond = model.conditioner([{"seconds_start": 0, "seconds_total": 12}] * b)
    cond["prompt"] = (synthetic.synth_input("prompt", (b, 128, dc["cond_token_dim"]), 1).to(dev), torch.ones(b, 128, device=dev))
    cond = {k: cond[k] for k in ("prompt", "seconds_start", "seconds_total")}
    noise = synthetic.synth_input("noise", (b, latent, t_len), 2)

    def run(**kw):
        draws = iter([synthetic.synth_input(f"sn{i}", (b, latent, t_len), 10 + i) for i in range(steps)])
        return generate_diffusion_cond(model, steps=steps, cfg_scale=7.0, conditioning_tensors=cond, sample_size=t_len * ratio, seed=3,
                                       device="cuda:0", sampler_type="dpmpp-3m-sde", sigma_min=0.3, sigma_max=500, noise=noise,
                                       noise_sampler=lambda s, sn: next(draws).to(dev), **kw)

    audio = run()
    lat = run(return_latents=True)
    assert audio.shape == (b, 2, t_len * ratio) and lat.shape == (b, latent, t_len)
    assert torch.isfinite(audio).all() and audio.abs().max().item() <= 1.0
    assert audio.abs().max().item() > 1e-3
    assert_close(f"generate vs decode of its own latents ({fmt})", audio, model.pretransform.decode(lat), GATE[fmt])
