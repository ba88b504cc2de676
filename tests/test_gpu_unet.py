"""The Dance Diffusion U-Net (DiffusionAttnUnet1D, "model_type": "diffusion_uncond") on the device, in all three operand formats, against the
REFERENCE's outputs (tests/golden/unet_small.npz, written by tests/golden/make_golden_unet.py from the reference's class on the CPU).

Gates (tests/golden/unet_cases.py, measured on the reference alone): fp16 / bf16 twice the reference's own figure with every Conv1d's operands
rounded to the format; fp32 four times the figure between the reference in fp32 and in float64; per output time step ([b, :, t]) eight times
either.  Then the surfaces built on the forward: the config factory, ``denoise`` (k-diffusion's VDenoiser), ``sample_k`` against a host loop
over ``denoise``, and ``generate_diffusion_uncond``."""
import copy
import math
import os
import sys

import pytest
import torch

from util import assert_close, assert_close_sliced, rel_l2, slice_errors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
import unet_cases as UC  # noqa: E402
import unet_units as UU  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return UC.load()


def unet(name, dev, fmt=None):
    """Case `name`'s model with the case's seeded weights, loaded strictly under the reference's names"""
    from stable_audio_tools.models.diffusion import DiffusionAttnUnet1D
    m = DiffusionAttnUnet1D(**copy.deepcopy(UC.CASES[name][0]))
    m.load_state_dict(UC.weights(m.state_dict()), strict=True)
    m = m.to(dev).eval()
    return m.set_gemm_dtype(fmt) if fmt else m


def check(name, fmt, got, golden, what="forward"):
    """The whole-output gate and the per-time-step gate of (case, fmt); prints every figure before it asserts"""
    want, gate = golden[name], UC.gate(name, fmt)
    assert got.shape == want.shape and got.dtype == torch.float32, (name, tuple(got.shape), got.dtype)
    rows = float(slice_errors(got, want, (0, 2)).max())
    print(f"\n[{name}, {fmt}, {what}] rel-L2 vs the reference {rel_l2(got, want):.3e} (gate {gate:.3e}), worst time step {rows:.3e} "
          f"(gate {UC.ROW_FACTOR * gate:.3e})")
    assert_close(f"{name} ({fmt})", got, want, gate)
    assert_close_sliced(f"{name} ({fmt}) per time step", got, want, UC.ROW_FACTOR * gate, (0, 2))


PARAMS = [(n, f) for n in UC.CASES for f in UC.FORMATS]


@pytest.mark.parametrize("name,fmt", PARAMS, ids=[f"{n}-{f}" for n, f in PARAMS])
def test_forward_vs_reference(dev, golden, name, fmt):
    x, t = UC.inputs(name)
    check(name, fmt, unet(name, dev, fmt)(x.to(dev), t.to(dev)), golden)


def _config_a():
    """dance_diffusion_base.json's "model" block (type DAU1d, config {n_attn_layers}) reduced to case A's sizes"""
    return {"model_type": "diffusion_uncond", "sample_size": 24, "sample_rate": 48000,
            "model": {"type": "DAU1d", "config": copy.deepcopy(UC.CASES["A"][0])}}


def wrapper(dev, fmt=None):
    import stable_audio_tools as S
    model = S.create_model_from_config(_config_a())
    model.model.load_state_dict(UC.weights(model.model.state_dict()), strict=True)
    model = model.to(dev).eval()
    if fmt:
        model.model.set_gemm_dtype(fmt)
    return model


@pytest.mark.parametrize("fmt", UC.FORMATS)
def test_model_from_config_vs_reference(dev, golden, fmt):
    model = wrapper(dev, fmt)
    assert model.diffusion_objective == "v" and model.io_channels == 2 and model.sample_size == 24 and model.pretransform is None
    x, t = UC.inputs("A")
    check("A", fmt, model(x.to(dev), t.to(dev)), golden, "create_model_from_config")


def test_forward_refuses_cond_and_bad_lengths(dev):
    m = unet("A", dev)
    x, t = (v.to(dev) for v in UC.inputs("A"))
    with pytest.raises(NotImplementedError, match="cond"):
        m(x, t, cond=x)
    for length, word in ((20, "multiple"), (16, "reflect")):
        with pytest.raises(ValueError, match=word):
            m(torch.zeros(2, 2, length, device=dev), t)
    assert m._ws is None, "a refused length allocated a workspace"


@pytest.mark.parametrize("sigma", [0.3, 1.0, 80.0])
def test_denoise_is_vdenoiser_of_forward(dev, sigma):
    """denoise(x, sigma) against the VDenoiser formula on forward's own output at the scaled input.  x * c_in is the same fp32 product in the
    boundary kernel and in torch, so v is the same; the combination c_out v + c_skip x rounds the two scalars, the two products and the sum:
    element by element within 5 * 2^-24 (|c_out v| + |c_skip x|)"""
    m = unet("A", dev, "fp32")
    x = UC.inputs("A")[0].to(dev) * (1.0 + sigma)
    c_in, c_out, c_skip = 1.0 / math.sqrt(sigma * sigma + 1.0), -sigma / math.sqrt(sigma * sigma + 1.0), 1.0 / (sigma * sigma + 1.0)
    t = torch.full((x.shape[0],), math.atan(sigma) * 2 / math.pi, device=dev)
    v = m(x * c_in, t)
    want = UU.vdenoise(v.double(), x.double(), sigma)
    out = torch.full_like(x, float("nan"))
    got = m.denoise(x, sigma, out=out)
    assert got is out
    share = ((got.double() - want).abs() / (5 * UU.UNIT * ((c_out * v.double()).abs() + (c_skip * x.double()).abs()))).max().item()
    print(f"\n[denoise sigma {sigma}] rel-L2 {rel_l2(got, want):.3e}, worst element at {share:.3f} of 5 * 2^-24 (|c_out v| + |c_skip x|)")
    assert share <= 1.0, share


def _host_loop(m, sampler, x0, sigmas, noises):
    """The sampler restated on the host in float64 over m.denoise and the module's own coefficient functions.  Returns the result and the sum
    S_i of the absolute coefficients of every step's update, with its number of terms."""
    from stable_audio_tools.inference import sampling as SP
    x = x0.double()
    den = lambda xx, s: m.denoise(xx.float().contiguous(), s).double()
    sums = []
    if sampler == "dpmpp-3m-sde":
        d1 = d2 = None
        for i, (a, b, c1, c2, cn) in enumerate(SP.dpmpp3m_coefficients(sigmas)):
            d = den(x, sigmas[i])
            x = a * x + b * d + (c1 * (d - d1) if d1 is not None else 0) + (c2 * (d1 - d2) if d2 is not None else 0) + (cn * noises[i].double() if cn else 0)
            d1, d2 = d, d1
            sums.append((abs(a) + abs(b) + 2 * abs(c1) + 2 * abs(c2) + abs(cn), 7))
        return x, sums
    assert sampler == "k-heun"
    for i in range(len(sigmas) - 1):
        s_i, s_n = sigmas[i], sigmas[i + 1]
        d = (x - den(x, s_i)) / s_i
        dt = s_n - s_i
        if s_n == 0:
            x = x + dt * d
            sums.append((1 + 2 * abs(dt / s_i), 3))
        else:
            x2 = x + dt * d
            x = x + dt / 2 * (d + (x2 - den(x2, s_n)) / s_n)
            # x2 is itself an update of x (1 + 2 |dt / s_i|), and enters with |dt / (2 s_n)| twice (as itself and through the denoiser)
            sums.append((1 + 2 * abs(dt / (2 * s_i)) + 2 * abs(dt / (2 * s_n)) * (1 + 2 * abs(dt / s_i)), 8))
    return x, sums


@pytest.mark.parametrize("sampler", ["dpmpp-3m-sde", "k-heun"])
def test_sample_k_drives_the_unet(dev, sampler):
    """3 steps with injected noise, fp32 mode, against the host loop in float64.  Bound, from the coefficients: every term of an update is the
    state, a denoised estimate of it or unit noise, so in units of the largest state (the initial one, sigma_max times unit noise) step i
    rounds by at most (terms_i + 1) S_i 2^-24, S_i the sum of its absolute coefficients; an error already in the state passes through a
    later step multiplied by at most S_j (the VDenoiser of a v-network maps a perturbation of the state to one no larger: c_skip +
    |c_out| c_in <= 1.21).  The gate is sum_i (terms_i + 1) S_i prod_{j > i} S_j 2^-24, relative to the norm of the initial state."""
    from stable_audio_tools.inference import sampling as SP
    from stable_audio_tools import synthetic
    m = unet("A", dev, "fp32")
    steps, smin, smax = 3, 0.5, 10.0
    sigmas = SP.get_sigmas_polyexponential(steps, smin, smax)
    noise = synthetic.synth_input("unet_sample_noise", (2, 2, 24), 5).to(dev)
    sn = [synthetic.synth_input(f"unet_sample_step{i}", (2, 2, 24), 5).to(dev) for i in range(steps)]
    it = iter(sn)
    got = SP.sample_k(m, noise.clone(), steps=steps, sampler_type=sampler, sigma_min=smin, sigma_max=smax, noise_sampler=lambda a, b: next(it))
    want, sums = _host_loop(m, sampler, noise * sigmas[0], sigmas, sn)
    gate = 0.0
    for i, (s_i, terms) in enumerate(sums):
        carried = (terms + 1) * s_i
        for s_j, _ in sums[i + 1:]:
            carried *= max(s_j, 1.0)
        gate += carried * UU.UNIT
    err = float((got.double() - want).norm() / (noise.double() * sigmas[0]).norm())
    print(f"\n[sample_k {sampler}] error over the initial state's norm {err:.3e} (gate {gate:.3e}); rel-L2 of the result {rel_l2(got, want):.3e}")
    assert torch.isfinite(got).all() and err <= gate, (err, gate)


def test_sample_k_refuses_conditioning_and_masks(dev):
    from stable_audio_tools.inference import sampling as SP
    m = unet("C", dev)
    noise = torch.zeros(1, 2, 6, device=dev)
    with pytest.raises(NotImplementedError, match="unconditional"):
        SP.sample_k(m, noise, steps=2, cross_attn_cond=torch.zeros(1, 4, 8, device=dev))
    with pytest.raises(NotImplementedError, match="mask"):
        SP.sample_k(m, noise, init_data=noise, mask=torch.ones(6), steps=2)


def test_generate_diffusion_uncond(dev):
    from stable_audio_tools.inference.generation import generate_diffusion_uncond
    model = wrapper(dev)
    kw = dict(steps=3, batch_size=2, sample_size=24, device="cuda:0", sampler_type="dpmpp-3m-sde", sigma_min=0.5, sigma_max=10.0)
    a = generate_diffusion_uncond(model, seed=7, **kw)
    assert a.shape == (2, 2, 24) and a.dtype == torch.float32 and torch.isfinite(a).all()
    b = generate_diffusion_uncond(model, seed=7, **kw)
    assert torch.equal(a, b), "the same seed gave another result"
    c = generate_diffusion_uncond(model, seed=8, **kw)
    assert not torch.equal(a, c)
    assert torch.equal(model.generate(seed=7, **kw), a)
    # a variation: init audio at the model's rate, sigma_max = init_noise_level; at a tiny noise level the result stays near the init
    init = 0.1 * UC.inputs("A")[0][:1]
    v = generate_diffusion_uncond(model, seed=7, init_audio=(48000, init[0]), init_noise_level=0.6, return_latents=True,
                                  **{k: val for k, val in kw.items() if k != "sigma_max"})
    assert v.shape == (2, 2, 24) and torch.isfinite(v).all() and not torch.equal(v, a)
    with pytest.raises(ValueError, match="multiple"):
        generate_diffusion_uncond(model, seed=7, **dict(kw, sample_size=20))
