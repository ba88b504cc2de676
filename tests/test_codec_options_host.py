"""Host side of the Oobleck configurations beside the Stable Audio VAE: ELU (``use_snake=False``), nearest-neighbour upsampling
(``use_nearest_upsample=True``), the final tanh (``set_final_tanh``) and channel counts that are not multiples of 64.  Module trees and
state-dict keys against the reference's recorded lists (tests/golden/codec_options_state_dict_keys.json), plan creation through
``sat_oobleck_plan_create_ex`` (host-only), and the three-tap folding of the nearest-upsample convolution.  No GPU needed."""
import copy
import ctypes
import json
import os
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
import make_golden_codec_options as GO  # noqa: E402  (case table and seeds; does not import the reference)

NAMES = sorted(GO.CONFIGS)


def _ref_keys(name):
    with open(os.path.join(GOLDEN, "codec_options_state_dict_keys.json")) as f:
        return json.load(f)[name]


def _create(cfg):
    import stable_audio_tools as S
    from stable_audio_tools.models import _init
    with _init.skip_init():
        return S.create_model_from_config(cfg)


@pytest.mark.parametrize("name", NAMES)
def test_autoencoder_constructs_with_reference_state_dict(name):
    from stable_audio_tools.models.autoencoders import AudioAutoencoder
    model = _create(GO.model_config(name))
    assert isinstance(model, AudioAutoencoder)
    got = {k: list(v.shape) for k, v in model.state_dict().items()}
    want = _ref_keys(name)
    assert set(got) == set(want), sorted(set(got) ^ set(want))
    assert got == want
    c = GO.CONFIGS[name]
    if not c["use_snake"]:
        assert not any(k.endswith((".alpha", ".beta")) for k in got), "an ELU codec has no Snake parameters"
    if c["use_nearest_upsample"]:
        assert "decoder.layers.1.layers.1.1.weight_v" in got and "decoder.layers.1.layers.1.1.bias" not in got
    assert model.decoder.use_snake == c["use_snake"] and model.encoder.use_snake == c["use_snake"]
    assert model.decoder.use_nearest_upsample == c["use_nearest_upsample"]


@pytest.mark.parametrize("name", NAMES)
def test_constructs_as_pretransform_of_a_diffusion_model(name):
    from stable_audio_tools import model_configs as MC
    from stable_audio_tools.models.autoencoders import AudioAutoencoder
    cfg = MC.reduced(MC.stable_audio_open_1_0())
    vae = GO.model_config(name)["model"]
    cfg["model"]["pretransform"]["config"] = vae
    cfg["model"]["io_channels"] = vae["latent_dim"]
    cfg["model"]["diffusion"]["config"]["io_channels"] = vae["latent_dim"]
    model = _create(cfg)
    assert isinstance(model.pretransform.model, AudioAutoencoder)
    got = {k[len("pretransform.model."):]: list(v.shape) for k, v in model.state_dict().items() if k.startswith("pretransform.model.")}
    assert got == _ref_keys(name)
    assert model.pretransform.downsampling_ratio == GO.ratio(name)


def test_set_final_tanh_is_the_way_to_the_tanh():
    from stable_audio_tools.models.autoencoders import AudioAutoencoder, OobleckDecoder
    cfg = GO.model_config("ref_defaults")
    model = _create(cfg)
    dec = model.decoder
    assert dec.final_tanh is False and isinstance(dec.layers[-1], torch.nn.Identity)
    keys = list(model.state_dict())
    dec._plan_version = "built"
    assert model.set_final_tanh(True) is model
    assert dec.final_tanh is True and isinstance(dec.layers[-1], torch.nn.Tanh) and dec._plan_version is None   # rebuilt on next use
    assert list(model.state_dict()) == keys                  # a tanh has no parameters: the checkpoint layout does not move
    dec._plan_version = "built"
    assert dec.set_final_tanh(True) is dec and dec._plan_version == "built"       # no change, no rebuild
    assert dec.set_final_tanh(False) is dec and dec.final_tanh is False and dec._plan_version is None
    assert callable(getattr(OobleckDecoder, "set_final_tanh")) and callable(getattr(AudioAutoencoder, "set_final_tanh"))
    # the constructor keeps rejecting the key (tests/test_host_logic.py pins that) and says where to go instead
    bad = copy.deepcopy(cfg)
    bad["model"]["decoder"]["config"]["final_tanh"] = True
    with pytest.raises(NotImplementedError) as ei:
        _create(bad)
    msg = str(ei.value)
    assert "final_tanh=False" in msg and "set_final_tanh(True)" in msg


def test_antialias_activation_still_raises():
    from stable_audio_tools.models.autoencoders import OobleckDecoder, OobleckEncoder
    for name in ("nearest_snake", "narrow_all"):
        with pytest.raises(NotImplementedError, match="antialias_activation"):
            OobleckDecoder(**dict(GO.decoder_kwargs(name, final_tanh=False), antialias_activation=True))
        with pytest.raises(NotImplementedError, match="antialias_activation"):
            OobleckEncoder(**dict(GO.encoder_kwargs(name), antialias_activation=True))
        cfg = GO.model_config(name)
        cfg["model"]["decoder"]["config"]["antialias_activation"] = True
        with pytest.raises(NotImplementedError):
            _create(cfg)


# ------------------------------------------------------------------------------------------------ C ABI (plan creation is host-only)
def _cfg(channels=128, latent_dim=64, is_decoder=1, gemm_dtype=3):
    from stable_audio_tools import _hip
    c = _hip.SatOobleckCfg()
    c.is_decoder, c.io_channels, c.channels, c.latent_dim, c.n_blocks = is_decoder, 2, channels, latent_dim, 3
    for i, (m, s) in enumerate(zip((1, 2, 3), (2, 4, 4))):
        c.c_mults[i], c.strides[i] = m, s
    c.gemm_dtype = gemm_dtype
    return c


def _opt(activation=0, final_tanh=0, nearest_upsample=0):
    from stable_audio_tools import _hip
    o = _hip.SatOobleckOptions()
    o.activation, o.final_tanh, o.nearest_upsample = activation, final_tanh, nearest_upsample
    return o


def _create_ex(cfg, opt, size=None):
    from stable_audio_tools import _hip
    lib = _hip.lib()
    plan = ctypes.c_void_p()
    rc = lib.sat_oobleck_plan_create_ex(ctypes.byref(cfg), ctypes.byref(opt) if opt is not None else None,
                                        ctypes.sizeof(opt) if size is None else size, ctypes.byref(plan))
    if rc == 0:
        need = ctypes.c_size_t()
        assert lib.sat_oobleck_workspace_bytes(plan, 1, 16, ctypes.byref(need)) == -5      # the build's own state check: not finalized
        lib.sat_oobleck_plan_destroy(plan)
    return rc


@pytest.mark.parametrize("gemm_dtype", [0, 3, 2], ids=["bf16", "fp16", "fp32"])
def test_plan_create_ex_lifts_the_channel_rule(gemm_dtype):
    from stable_audio_tools import _hip
    lib = _hip.lib()
    for channels, latent, is_decoder in ((16, 64, 1), (100, 64, 1), (128, 20, 1), (48, 20, 1), (16, 128, 0), (100, 40, 0)):
        for opt in (_opt(), _opt(activation=1), _opt(1, 1, 1) if is_decoder else _opt(1)):
            assert _create_ex(_cfg(channels, latent, is_decoder, gemm_dtype), opt) == 0, (channels, latent, lib.sat_last_error())
    assert _create_ex(_cfg(100, 20, 1, gemm_dtype), None, 0) == 0          # NULL options: the defaults, still no channel rule
    # the original entry point keeps its rule
    plan = ctypes.c_void_p()
    assert lib.sat_oobleck_plan_create(ctypes.byref(_cfg(100, 64, 1, gemm_dtype)), ctypes.byref(plan)) == -2
    assert b"multiple of 64" in lib.sat_last_error()
    assert lib.sat_oobleck_plan_create(ctypes.byref(_cfg(128, 20, 1, gemm_dtype)), ctypes.byref(plan)) == -2
    assert lib.sat_oobleck_plan_create(ctypes.byref(_cfg(128, 64, 1, gemm_dtype)), ctypes.byref(plan)) == 0
    lib.sat_oobleck_plan_destroy(plan)


def test_plan_create_ex_rejects_bad_options():
    from stable_audio_tools import _hip
    lib = _hip.lib()
    for bad in (2, -1, 7):
        assert _create_ex(_cfg(), _opt(activation=bad)) == -2, bad          # SAT_E_UNSUPPORTED
        assert b"activation" in lib.sat_last_error()
    assert _create_ex(_cfg(), _opt(final_tanh=2)) == -2
    assert _create_ex(_cfg(), _opt(nearest_upsample=-1)) == -2
    assert _create_ex(_cfg(latent_dim=128, is_decoder=0), _opt(final_tanh=1)) == -2        # decoder options on an encoder
    assert _create_ex(_cfg(latent_dim=128, is_decoder=0), _opt(nearest_upsample=1)) == -2
    good = ctypes.sizeof(_opt())
    assert good == 12
    for size in (0, 8, good - 1, good + 4):
        assert _create_ex(_cfg(), _opt(), size) == -1, size                 # SAT_E_INVALID: a struct of another layout is not read
        assert b"options_bytes" in lib.sat_last_error()
    assert _create_ex(_cfg(channels=0), _opt()) == -2
    assert _create_ex(_cfg(latent_dim=0), _opt()) == -2
    assert _create_ex(_cfg(gemm_dtype=1), _opt()) == -2
    assert lib.sat_oobleck_plan_create_ex(None, None, 0, None) == -1


# ------------------------------------------------------------------------------------------------ the three-tap form
@pytest.mark.parametrize("stride", [2, 3, 4, 8])
def test_nearest_upsample_three_tap_folding(stride):
    """Upsample(nearest, s) + Conv1d(k = 2s, padding "same") == a polyphase convolution with taps at rows m-1, m, m+1 whose weights are
    per-phase sums of the original taps.  fp32 on both sides: the difference is summation order (the issue measured 2e-6 ... 8e-6)."""
    from stable_audio_tools.models.autoencoders import nearest_upsample_taps
    g = torch.Generator().manual_seed(stride)
    c_in, c_out, t = 24, 10, 13
    w = torch.randn(c_out, c_in, 2 * stride, generator=g) / (c_in * 2 * stride) ** 0.5
    x = torch.randn(2, c_in, t, generator=g)
    want = F.conv1d(F.interpolate(x, scale_factor=stride, mode="nearest"), w, padding="same")
    taps = nearest_upsample_taps(w, stride)
    assert taps.shape == (stride, 3, c_out, c_in)
    # every original tap lands in exactly one (phase, row) slot
    assert torch.allclose(taps.sum(dim=1), w.sum(dim=2).expand(stride, -1, -1), atol=1e-6)
    xp = F.pad(x, (1, 1))
    got = torch.empty(2, c_out, t, stride)
    for p in range(stride):
        got[..., p] = sum(torch.einsum("oc,bct->bot", taps[p, r], xp[..., r:r + t]) for r in range(3))
    got = got.reshape(2, c_out, t * stride)
    assert want.shape == got.shape
    assert (got - want).abs().max().item() < 2e-5


@pytest.mark.parametrize("name,required", [
    ("generate.py", ["--output-dir", "o", "--cond-yaml-path", "c.yaml"]),
    ("reconstruct_audios.py", ["--audio-dir", "a", "--output-dir", "o"]),
])
def test_scripts_reach_the_final_tanh(name, required, monkeypatch):
    import runpy
    mod = runpy.run_path(os.path.join(ROOT, "friendly-stable-audio-tools_amd", name), run_name="script_under_test")
    monkeypatch.setattr(sys, "argv", [name] + required)
    assert mod["get_args"]().codec_final_tanh is False
    monkeypatch.setattr(sys, "argv", [name] + required + ["--codec-final-tanh"])
    assert mod["get_args"]().codec_final_tanh is True
