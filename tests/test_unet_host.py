"""Host-side checks of the Dance Diffusion U-Net family: the module tree against the reference's state-dict keys (kernel buffers included), the
factory on the four shipped dance_diffusion configs, every refusal with its reason, the length rule, the float64 restatement of
tests/unet_units.py against goldens A-C, the gate figures recomputed from the stored tensors, and the planted mistakes each gate must
reject."""
import copy
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
import unet_cases as UC  # noqa: E402
import unet_units as UU  # noqa: E402
from util import rel_l2, slice_errors  # noqa: E402

from stable_audio_tools.models import _init  # noqa: E402
from stable_audio_tools.models.diffusion import DiffusionAttnUnet1D, DiffusionModelWrapper, create_diffusion_uncond_from_config  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    return UC.load()


@pytest.mark.parametrize("name", list(UC.CASES))
def test_state_dict_matches_the_reference(name):
    want = json.load(open(UC.KEYS_PATH))[name]
    with _init.skip_init():
        m = DiffusionAttnUnet1D(**copy.deepcopy(UC.CASES[name][0]))
    got = {k: list(v.shape) for k, v in m.state_dict().items()}
    assert got == want, sorted(set(got) ^ set(want))
    assert any(k.endswith("main.0.kernel") for k in got) and any(k.endswith("main.14.kernel") for k in got)
    m.load_state_dict(UC.weights(m.state_dict()), strict=True)


# the "model" blocks of the reference's configs/model_configs/dance_diffusion/*.json (a file of settings each; only these fields matter here)
SHIPPED = {
    "dance_diffusion_base": dict(sample_size=65536, sample_rate=48000),
    "dance_diffusion_base_16k": dict(sample_size=65536, sample_rate=16000),
    "dance_diffusion_base_44k": dict(sample_size=65536, sample_rate=44100),
    "dance_diffusion_large": dict(sample_size=131072, sample_rate=48000),
}


@pytest.mark.parametrize("name", list(SHIPPED))
def test_factory_builds_the_shipped_configs(name):
    import stable_audio_tools as S
    cfg = {"model_type": "diffusion_uncond", **SHIPPED[name], "model": {"type": "DAU1d", "config": {"n_attn_layers": 5}}}
    with torch.device("meta"):
        model = S.create_model_from_config(cfg)
    assert isinstance(model, DiffusionModelWrapper) and isinstance(model.model, DiffusionAttnUnet1D)
    assert model.diffusion_objective == "v" and model.sample_size == cfg["sample_size"] and model.sample_rate == cfg["sample_rate"]
    assert model.io_channels == 2 and model.min_input_length == 1 and model.pretransform is None
    n = sum(p.numel() for p in model.model.parameters())
    assert abs(n - 221.4e6) < 0.2e6, n                      # the default network
    sd = model.model.state_dict()
    # attention at the reference's levels i >= depth - n_attn_layers = 9, i.e. from the eighth SkipBlock down
    deep = "net.3.main." + "7.main." * 7
    assert deep + "2.qkv_proj.weight" in sd and ("net.3.main." + "7.main." * 6 + "2.qkv_proj.weight") not in sd
    assert sd["net.0.main.0.weight"].shape == (128, 18, 5) and sd["net.6.main.3.weight"].shape == (2, 128, 5)
    model.model.check_length(cfg["sample_size"])


def test_factory_refuses_the_other_uncond_types():
    import stable_audio_tools as S
    for kind, word in (("dit", "unconditional DiT"), ("adp_uncond_1d", "third-party"), ("nope", "Unknown model type")):
        with pytest.raises(NotImplementedError, match=word):
            S.create_model_from_config({"model_type": "diffusion_uncond", "sample_size": 8, "sample_rate": 8, "model": {"type": kind, "config": {}}})
    for kind in ("lm", "diffusion_prior", "diffusion_autoencoder"):
        with pytest.raises(NotImplementedError, match="outside this build"):
            S.create_model_from_config({"model_type": kind})


@pytest.mark.parametrize("kw,exc,word", [
    (dict(use_snake=True), NotImplementedError, "Snake1d"),
    (dict(learned_resample=True), NotImplementedError, "learned_resample"),
    (dict(cond_dim=4), NotImplementedError, "forward fails"),
    (dict(cond_noise_aug=True), NotImplementedError, "forward fails"),
    (dict(kernel_size=9), NotImplementedError, "kernel_size"),
    (dict(kernel_size=4), NotImplementedError, "kernel_size"),
    (dict(channels=[128, 192]), NotImplementedError, "multiple of 128"),
    (dict(depth=17, channels=[128] * 17, strides=[2] * 16), NotImplementedError, "at most 16"),
    (dict(io_channels=113), NotImplementedError, "io_channels"),
    (dict(strides=[4]), ValueError, "stride 2"),
    (dict(depth=1), ValueError, "depth"),
])
def test_refusals(kw, exc, word):
    base = dict(depth=2, channels=[128, 128], n_attn_layers=0)
    with _init.skip_init(), pytest.raises(exc, match=word):
        DiffusionAttnUnet1D(**{**base, **kw})


def test_module_refusals():
    with _init.skip_init():
        m = DiffusionAttnUnet1D(**copy.deepcopy(UC.CASES["C"][0]))
    with pytest.raises(ValueError, match="fp16"):
        m.set_gemm_dtype("fp8")
    with pytest.raises(NotImplementedError):
        m.activation_range_report()
    with pytest.raises(RuntimeError, match="no standalone forward"):
        m.net[0](torch.zeros(1, 18, 6))
    from stable_audio_tools.models.blocks import Downsample1d, Upsample1d
    for cls in (Downsample1d, Upsample1d):
        with pytest.raises(NotImplementedError, match="cubic"):
            cls("linear")
        r = cls("cubic")
        r.check_kernel()
        r.kernel[3] += 2e-6
        with pytest.raises(ValueError, match="cubic filter"):
            r.check_kernel("net.3.main.0.kernel")
    assert torch.equal(Upsample1d("cubic").kernel, 2 * Downsample1d("cubic").kernel)


def test_length_rule_is_a_value_error():
    with _init.skip_init():
        a = DiffusionAttnUnet1D(**copy.deepcopy(UC.CASES["A"][0]))
        c = DiffusionAttnUnet1D(**copy.deepcopy(UC.CASES["C"][0]))
    a.check_length(24)
    c.check_length(6)
    for m, length, word in ((a, 20, "multiple"), (a, 16, "reflect"), (a, 0, "multiple"), (c, 4, "reflect"), (c, 7, "multiple")):
        with pytest.raises(ValueError, match=word):
            m.check_length(length)
    # forward refuses before it looks for a device
    with pytest.raises(ValueError, match="multiple"):
        a(torch.zeros(1, 2, 20), torch.zeros(1))


def _weights(name):
    with _init.skip_init():
        m = DiffusionAttnUnet1D(**copy.deepcopy(UC.CASES[name][0]))
    return UC.weights(m.state_dict())


@pytest.fixture(scope="module")
def restated():
    """the float64 restatement of every case, computed once"""
    out = {}
    for name, (kw, _, _) in UC.CASES.items():
        x, t = UC.inputs(name)
        out[name] = UU.forward(_weights(name), kw, x, t)
    return out


@pytest.mark.parametrize("name", list(UC.CASES))
def test_restatement_reproduces_the_float64_golden(golden, restated, name):
    err = rel_l2(restated[name], golden[f"{name}__f64"])
    assert err <= 1e-10, err


@pytest.mark.parametrize("name", list(UC.CASES))
def test_gate_figures_are_the_stored_tensors(golden, name):
    want = golden[name]
    assert all(bool(torch.isfinite(v).all()) for v in golden.values())
    for fmt in ("fp16", "bf16"):
        fig = rel_l2(golden[f"{name}__r16_{fmt}"], want)
        assert abs(fig - UC.R16[name][fmt]) <= 2e-3 * fig and fig < UC.R16_LIMIT, (name, fmt, fig)
        assert float(slice_errors(golden[f"{name}__r16_{fmt}"], want, (0, 2)).max()) <= UC.ROW_FACTOR * UC.gate(name, fmt)
    fig = rel_l2(want, golden[f"{name}__f64"])
    assert abs(fig - UC.F64[name]) <= 2e-3 * fig
    assert float(slice_errors(want, golden[f"{name}__f64"], (0, 2)).max()) <= UC.ROW_FACTOR * UC.gate(name, "fp32")


@pytest.mark.parametrize("plant", UU.PLANTS)
def test_gates_reject_planted_mistakes(golden, plant):
    """Each mistake, planted into the float64 restatement, misses the fp32 gate of every case it can show in (whole output or worst time
    step), by a factor of 10 or more; the structural ones miss the 16-bit gates as well."""
    shown = 0
    for name, (kw, _, _) in UC.CASES.items():
        if plant == "scale_once" and kw["n_attn_layers"] == 0:
            continue
        x, t = UC.inputs(name)
        got = UU.forward(_weights(name), kw, x, t, plant=plant)
        whole = rel_l2(got, golden[name])
        rows = float(slice_errors(got, golden[name], (0, 2)).max())
        gate = UC.gate(name, "fp32")
        assert whole > 10 * gate or rows > 10 * UC.ROW_FACTOR * gate, (plant, name, whole, rows, gate)
        if plant in ("concat_order", "per_channel_norm", "zero_pad", "unclipped_time"):
            g16 = UC.gate(name, "bf16")
            assert whole > g16 or rows > UC.ROW_FACTOR * g16, (plant, name, whole, rows, g16)
        shown += 1
    assert shown >= 2
