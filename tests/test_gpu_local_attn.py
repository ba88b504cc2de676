"""The local-attention transformer codec ("type": "local_attn") on the device, in all three operand formats, against the REFERENCE's outputs
(tests/golden/local_attn_small.npz, written by tests/golden/make_golden_local_attn.py with tests/golden/natten_standin.py in NATTEN's place).

Gates (tests/golden/local_attn_cases.py, measured on the reference alone): fp16 / bf16 twice the reference's own figure with every Linear's
operands rounded to the format; fp32 four times the figure between the reference in fp32 and in float64; per output row (one time step of
one item) the same figure times ROW_FACTOR.  Cases: A (32- and 64-channel heads, a 32-row tail, a batch seam), B (128- and 96-channel heads,
window 65; fp16 / bf16) and B32 (its fp32 stand-in, 64 and 96), C (window = sequence, ratio 3), D (an AudioAutoencoder from a config dict,
vae bottleneck, plain and chunked)."""
import copy
import functools
import json
import os
import sys

import pytest
import torch

from util import assert_close, assert_close_sliced, rel_l2, slice_errors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
import local_attn_cases as LC  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return LC.load()


def codec(name, side, dev, fmt=None):
    """The encoder or decoder of case `name` with the case's seeded weights, loaded strictly under the reference's names"""
    from stable_audio_tools.models.local_attention import TransformerDecoder1D, TransformerEncoder1D
    enc_kw, dec_kw = LC.CODECS[name][:2]
    m = TransformerEncoder1D(**enc_kw) if side == "enc" else TransformerDecoder1D(**dec_kw)
    m.load_state_dict(LC.weights(m.state_dict()), strict=True)
    m = m.to(dev).eval()
    return m.set_gemm_dtype(fmt) if fmt else m


def autoencoder(dev, fmt=None):
    import stable_audio_tools as S
    model = S.create_model_from_config(copy.deepcopy(LC.D_CONFIG))
    model.load_state_dict(LC.weights(model.state_dict()), strict=True)
    model = model.to(dev).eval()
    return model.set_gemm_dtype(fmt) if fmt else model


def check(entry, fmt, got, golden):
    """The whole-output gate and the per-row gate of (entry, fmt); prints every figure before it asserts"""
    want, gate = golden[entry], LC.gate(entry, fmt)
    assert got.shape == want.shape, (entry, tuple(got.shape), tuple(want.shape))
    rows = float(slice_errors(got, want, (0, 2)).max())
    print(f"\n[{entry}, {fmt}] rel-L2 vs the reference {rel_l2(got, want):.3e} (gate {gate:.3e}), worst row {rows:.3e} (gate {LC.ROW_FACTOR * gate:.3e})")
    assert_close(f"{entry} ({fmt})", got, want, gate)
    assert_close_sliced(f"{entry} ({fmt}) per time step", got, want, LC.ROW_FACTOR * gate, (0, 2))


CODEC_PARAMS = [(name, fmt) for name in LC.CODECS for fmt in LC.FORMATS if LC.runs(f"{name}_enc", fmt) and LC.runs(f"{name}_dec", fmt)]


@pytest.mark.parametrize("name,fmt", CODEC_PARAMS, ids=[f"{n}-{f}" for n, f in CODEC_PARAMS])
def test_encoder_and_decoder_vs_reference(dev, golden, name, fmt):
    z = codec(name, "enc", dev, fmt)(LC.audio(name).to(dev))
    check(f"{name}_enc", fmt, z, golden)
    y = codec(name, "dec", dev, fmt)(golden[f"{name}_enc"].to(dev))      # from the reference's latents, as the golden was
    check(f"{name}_dec", fmt, y, golden)


def test_every_issue_case_runs_in_every_format():
    """No (case, format) pair is dropped but B in fp32, which B32 stands in for"""
    assert LC.DROPPED == []
    missing = [(n, f) for n in LC.CODECS for f in LC.FORMATS if (n, f) not in CODEC_PARAMS]
    assert missing == [("B", "fp32")] and ("B32", "fp32") in CODEC_PARAMS


@pytest.mark.parametrize("fmt", LC.FORMATS)
def test_autoencoder_from_config_vs_reference(dev, golden, fmt):
    """Case D: encode_audio / decode_audio of an AudioAutoencoder built by create_model_from_config, plain and chunked; the chunked results
    against the reference's chunked results.  The vae bottleneck's Gaussian is injected (per chunk: the same tensor, as in the generator)."""
    model = autoencoder(dev, fmt)
    x = LC.d_audio().to(dev)
    z = model.encode_audio(x, noise=LC.d_noise((LC.D_BATCH, 4, LC.D_SAMPLES // 8)).to(dev))
    check("D_encode", fmt, z, golden)
    z_ref = golden["D_encode"].to(dev)
    check("D_decode", fmt, model.decode_audio(z_ref), golden)
    check("D_decode_chunked", fmt, model.decode_audio(z_ref, chunked=True, **LC.D_CHUNK), golden)
    plain = model.bottleneck.encode
    model.bottleneck.encode = functools.partial(plain, noise=LC.d_noise((1, 4, LC.D_CHUNK["chunk_size"])).to(dev))
    try:
        check("D_encode_chunked", fmt, model.encode_audio(x, chunked=True, **LC.D_CHUNK), golden)
    finally:
        model.bottleneck.encode = plain
    # iterate_batch: item by item, the same bits as the batch (every kernel treats the items alike)
    one = model.decode(z_ref, iterate_batch=1)
    assert torch.equal(one, model.decode(z_ref))


def test_pretransform_wraps_the_codec(dev, golden):
    from stable_audio_tools.models.pretransforms import AutoencoderPretransform
    model = autoencoder(dev)
    pre = AutoencoderPretransform(model, scale=2.0, model_half=True)
    assert model.encoder.gemm_dtype == model.decoder.gemm_dtype == "fp16" and pre.downsampling_ratio == 8 and pre.encoded_channels == 4
    z_ref = golden["D_encode"].to(dev)
    check("D_decode", "fp16", pre.decode(z_ref / 2.0), golden)


def test_state_dict_matches_the_reference(dev):
    want = json.load(open(LC.KEYS_PATH))
    for name in LC.CODECS:
        for side in ("enc", "dec"):
            m = codec(name, side, dev)
            assert {k: list(v.shape) for k, v in m.state_dict().items()} == want[f"{name}_{side}"], f"{name}_{side}"
    model = autoencoder(dev)
    assert {k: list(v.shape) for k, v in model.state_dict().items()} == want["D"]
    for key in ("layers.0.transformer.layers.0.0.gamma", "layers.0.transformer.layers.0.1.to_qkv.weight", "layers.0.transformer.layers.0.1.to_out.weight",
                "layers.0.transformer.layers.0.4.ff.0.proj.weight", "layers.0.project_down.weight", "layers.1.project_in.weight", "project_in.weight",
                "project_out.weight"):
        assert key in want["A_enc"], key
    assert "layers.0.project_up.weight" in want["A_dec"]


def test_plan_is_rebuilt_after_load_state_dict(dev, golden):
    m = codec("C", "enc", dev, "fp32")
    x = LC.audio("C").to(dev)
    first = m(x)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    sd["project_out.weight"] = sd["project_out.weight"] * 2.0
    m.load_state_dict(sd, strict=True)
    assert rel_l2(m(x), 2.0 * first) < 1e-6


# ---------------------------------------------------------------------------------------------------------------------------- refusals
def test_length_and_window_refusals_come_before_any_launch(dev):
    """ValueError for a length that is no multiple of the ratios' product and for a stage shorter than the window, with the workspace still
    unallocated and no plan built: nothing was launched"""
    enc = codec("A", "enc", dev)
    with pytest.raises(ValueError, match="multiple of the product of the ratios"):
        enc(torch.zeros(1, 2, 1054, device=dev))
    with pytest.raises(ValueError, match="fewer than local_attn_window_size"):
        enc(torch.zeros(1, 2, 12, device=dev))          # stage 1 would run at 6 rows, window 7
    assert enc._ws is None and enc._plan is None
    dec = codec("B", "dec", dev)
    with pytest.raises(ValueError, match="fewer than local_attn_window_size"):
        dec(torch.zeros(1, 6, 8, device=dev))           # stage 0 would run at 32 rows, window 65
    assert dec._ws is None and dec._plan is None
    # the library refuses the same by itself (a caller of the C ABI gets SAT_E_INVALID from the workspace query and from the forward)
    import ctypes
    from stable_audio_tools import _hip
    plan = enc._ensure_plan()
    need = ctypes.c_size_t()
    assert _hip.lib().sat_local_attn_workspace_bytes(plan, 1, 1054, ctypes.byref(need)) == -1 and b"multiple" in _hip.lib().sat_last_error()
    assert _hip.lib().sat_local_attn_workspace_bytes(plan, 1, 12, ctypes.byref(need)) == -1 and b"window" in _hip.lib().sat_last_error()
    x, out, ws = torch.zeros(1, 2, 12, device=dev), torch.full((1, 8, 3), 7.0, device=dev), torch.zeros(1 << 20, dtype=torch.uint8, device=dev)
    assert _hip.lib().sat_local_attn_forward(plan, _hip.ptr(x), _hip.ptr(out), 1, 12, _hip.ptr(ws), ws.numel(), _hip.stream()) == -1
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


def test_format_and_report_refusals(dev):
    b = codec("B", "enc", dev)
    with pytest.raises(NotImplementedError, match="128-channel heads"):
        b.set_gemm_dtype("fp32")
    with pytest.raises(ValueError):
        b.set_gemm_dtype("fp8")
    model = autoencoder(dev)
    with pytest.raises(NotImplementedError, match="local_attn"):
        model.activation_range_report(True)
    with pytest.raises(NotImplementedError, match="local_attn"):
        model.encoder.activation_range_report(True)


def test_construction_refusals_on_the_device_build():
    """The construction-time refusals of tests/test_local_attn_host.py, here as well: each raises its exception before a plan exists"""
    from test_local_attn_host import check_construction_refusals
    check_construction_refusals()


def test_mixed_codec_runs(dev):
    """A local_attn encoder with an Oobleck decoder (README, "Local-attention configurations"): the two plans are independent"""
    import stable_audio_tools as S
    cfg = copy.deepcopy(LC.D_CONFIG)
    cfg["model"]["decoder"] = {"type": "oobleck", "config": dict(out_channels=2, channels=16, c_mults=[1, 2], strides=[2, 4], latent_dim=4,
                                                                 use_snake=True, final_tanh=False)}
    model = S.create_model_from_config(cfg)
    model.encoder.load_state_dict(LC.weights(model.encoder.state_dict()), strict=True)
    model = model.to(dev).eval().set_gemm_dtype("bf16")
    assert model.encoder.gemm_dtype == model.decoder.gemm_dtype == "bf16"
    z = model.encode(LC.d_audio().to(dev))
    y = model.decode(z)
    assert z.shape == (2, 4, 100) and y.shape == (2, 2, 800) and bool(torch.isfinite(z).all()) and bool(torch.isfinite(y).all())
