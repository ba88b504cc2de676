"""Convolutional feed-forwards (ff_kwargs use_conv, reference models/transformer.py:211-287) on the HIP DiT against the REFERENCE's own
outputs (tests/golden/dit_conv_ff_small*.npz: tests/golden/make_golden_dit_conv_ff.py).

* the suite's operand format at the reduced-DiT gates of test_gpu_dit_block_options.py: T(2.5e-3) at CFG 1, T(1.2e-2) at CFG 7;
* the fp32 verification mode (gemm_dtype "fp32x") at 1e-4: what separates an indexing error (a window off by one row or leaking into the
  neighbouring sequence, taps in the wrong order) from rounding;
* four cases again with the LayerNorm fusion switched off and with the fused to_q + cross-attention launch off, and through the fused
  sampler step;
* conv_all_adaln with per-block operand formats;
* one config-driven generation, which must differ from the same model with the off-centre taps zeroed.
Measured errors, the reference's own rounded-operand figures (``<case>__r16_*``) and the gates: profiles/dit_conv_ff_verification.txt.
The reference with only the operands of its Linears and Conv1ds rounded is at 4.4e-4 - 4.9e-4 (CFG 1) / 2.2e-3 - 2.3e-3 (CFG 7) in fp16 and
3.6e-3 - 3.9e-3 / 1.7e-2 - 1.9e-2 in bf16 on these cases, the figures of the block-option cases those gates already serve.
"""
import copy
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import cases  # noqa: E402
import dit_conv_ff_cases as CC  # noqa: E402
from util import FORMATS, SUITE, assert_close, rel_l2  # noqa: E402

T = SUITE.tol
pytestmark = pytest.mark.gpu

_MODELS = {}
_GOLD = []


def _gold():
    if not _GOLD:
        _GOLD.append(cases.load("dit_conv_ff_small"))
    return _GOLD[0]


def _model(cfg_name, dev):
    if cfg_name not in _MODELS:
        from stable_audio_tools.models import _init
        from stable_audio_tools.models.dit import DiffusionTransformer
        with _init.skip_init():
            m = DiffusionTransformer(**CC.CONFIGS[cfg_name], **CC.PRODUCT_KWARGS)
        m.load_state_dict(CC.synth_weights(m.state_dict(), 0), strict=True)
        _MODELS[cfg_name] = m.to(dev).eval()
    return _MODELS[cfg_name]


def _inputs(name, dev):
    to = lambda v: None if v is None else v.to(dev)
    return tuple(to(v) for v in CC.case_inputs(name))


def _run(name, dev, dtype, ln_fold=True, cross_fusion=True, formats=None):
    cfg_name, _, _, cfg_scale = CC.CASES[name]
    m = _model(cfg_name, dev)
    m.set_gemm_dtype(dtype).set_layernorm_fusion(ln_fold).set_cross_attention_fusion(cross_fusion).set_block_gemm_dtypes(formats)
    try:
        x, t, c, g, pc, pm = _inputs(name, dev)
        out = m(x, t, cross_attn_cond=c, global_embed=g, prepend_cond=pc, prepend_cond_mask=pm, cfg_scale=cfg_scale)
        torch.cuda.synchronize()
    finally:
        m.set_block_gemm_dtypes(None).set_gemm_dtype(SUITE.gemm_dtype).set_layernorm_fusion(True).set_cross_attention_fusion(True)
    return out


def _gate(name, fmt=SUITE):
    return fmt.tol(2.5e-3) if CC.CASES[name][3] == 1.0 else fmt.tol(1.2e-2)


def _r16(name, fmt=SUITE):
    """What 16-bit operands of the Linears / convs alone cost the REFERENCE on this case (computed on the CPU by the generator)."""
    return rel_l2(_gold()[f"{name}__r16_{fmt.gemm_dtype}"], _gold()[name])


@pytest.mark.parametrize("name", list(CC.CASES))
def test_conv_ff_vs_reference(dev, name):
    got = _run(name, dev, SUITE.gemm_dtype)
    e = rel_l2(got, _gold()[name])
    print(f"\n[dit conv ff {name}, {SUITE.gemm_dtype}] rel-L2 vs reference {e:.2e} (gate {_gate(name):.1e}; reference with rounded operands {_r16(name):.2e})")
    assert_close(f"{name} ({SUITE.gemm_dtype}) vs reference", got, _gold()[name], _gate(name))


@pytest.mark.parametrize("name", list(CC.CASES))
def test_conv_ff_fp32_vs_reference(dev, name):
    got = _run(name, dev, "fp32x")
    e = rel_l2(got, _gold()[name])
    print(f"\n[dit conv ff {name}, fp32x] rel-L2 vs reference {e:.2e} (gate 1.0e-04)")
    assert_close(f"{name} (fp32x) vs reference", got, _gold()[name], 1e-4)


OTHER_PATHS = ["conv_cfg7_T77", "conv_silu_cfg7_T77", "conv_prepend_cfg7_T77", "conv_all_adaln_cfg7_T77"]


@pytest.mark.parametrize("path", ["ln_fold_off", "cross_fusion_off"])
@pytest.mark.parametrize("name", OTHER_PATHS)
def test_conv_ff_on_the_other_launch_paths(dev, name, path):
    got = _run(name, dev, SUITE.gemm_dtype, ln_fold=path != "ln_fold_off", cross_fusion=path != "cross_fusion_off")
    e = rel_l2(got, _gold()[name])
    print(f"\n[dit conv ff {name}, {SUITE.gemm_dtype}, {path}] rel-L2 vs reference {e:.2e} (gate {_gate(name):.1e})")
    assert_close(f"{name} ({SUITE.gemm_dtype}, {path}) vs reference", got, _gold()[name], _gate(name))


@pytest.mark.parametrize("dtype", ["suite", "fp32x"])
@pytest.mark.parametrize("name", OTHER_PATHS)
def test_fused_denoise_matches_forward(dev, name, dtype):
    """prepare_generation + denoise (one sat_dit_denoise_cfg per step) == VDenoiser(forward), at the gates of test_gpu_dit_block_options.py:
    1e-5 in fp32; T(2e-2) in the suite's format, where the two round c_in * x at different points and CFG 7 amplifies the roundings that flip."""
    cfg_name, _, _, cfg_scale = CC.CASES[name]
    fmt = SUITE.gemm_dtype if dtype == "suite" else dtype
    gate = T(2e-2) if dtype == "suite" else 1e-5
    m = _model(cfg_name, dev)
    m.set_gemm_dtype(fmt)
    try:
        x, _, c, g, pc, _ = _inputs(name, dev)
        for sigma in (0.7, 12.0):
            c_skip, c_out, c_in = 1.0 / (sigma ** 2 + 1), -sigma / (sigma ** 2 + 1) ** 0.5, 1.0 / (sigma ** 2 + 1) ** 0.5
            t = torch.full((x.shape[0],), float(torch.atan(torch.tensor(sigma, dtype=torch.float64)) / torch.pi * 2), device=dev)
            want = m(x * c_in, t, cross_attn_cond=c, global_embed=g, prepend_cond=pc, cfg_scale=cfg_scale) * c_out + x * c_skip
            m.prepare_generation(c, g, cfg_scale, prepend_cond=pc)
            got = m.denoise(x, sigma, cfg_scale=cfg_scale)
            torch.cuda.synchronize()
            e = rel_l2(got, want)
            print(f"\n[fused denoise {name}, {fmt}, sigma {sigma}] rel-L2 vs VDenoiser(forward) {e:.2e} (gate {gate:.1e})")
            assert torch.isfinite(got).all()
            assert e <= gate, f"{name} {fmt} sigma {sigma}: fused denoise vs VDenoiser(forward) rel-L2 {e:.3e} > {gate:.1e}"
    finally:
        m.set_gemm_dtype(SUITE.gemm_dtype)


@pytest.mark.parametrize("name", ["conv_all_adaln_cfg1_T64", "conv_all_adaln_cfg7_T77"])
def test_conv_ff_with_per_block_formats(dev, name):
    """[fp16, bf16, fp16]: block 1 keeps its tap-major weight images and the SiLU hidden state in bf16.  Gated at the bf16 gates, the
    coarsest format in the plan."""
    bf16 = FORMATS[0]
    got = _run(name, dev, "fp16", formats=["fp16", "bf16", "fp16"])
    e = rel_l2(got, _gold()[name])
    print(f"\n[dit conv ff {name}, fp16 / bf16 / fp16] rel-L2 vs reference {e:.2e} (gate {_gate(name, bf16):.1e})")
    assert_close(f"{name} (fp16 / bf16 / fp16) vs reference", got, _gold()[name], _gate(name, bf16))
    uniform = _run(name, dev, "fp16")
    assert not torch.equal(got, uniform), "the per-block formats changed no bit: block 1 did not run in bf16"


def test_conv_ff_c_abi_after_finalize_and_range_report(dev):
    import ctypes
    from stable_audio_tools import _hip
    lib = _hip.lib()
    m = _model("conv", dev)
    plan = m._ensure_plan()
    opts = _hip.SatDitFfConvOptions(3)
    assert lib.sat_dit_plan_set_ff_conv(plan, ctypes.byref(opts), ctypes.sizeof(opts)) == -5 and b"finalized" in lib.sat_last_error()
    assert lib.sat_dit_range_report(plan, 1) == -2 and b"sat_dit_plan_set_ff_conv" in lib.sat_last_error()
    with pytest.raises(NotImplementedError, match="activation_range_report"):
        m.activation_range_report(True)


@pytest.mark.parametrize("cfg_name", ["conv", "conv_silu"])
def test_profile_hook_brackets_ff_in(dev, cfg_name):
    """sat_dit_profile on such a plan: one event pair per forward round FF-in of block depth / 2 -- the Linear SwiGLU GEMM under glu, else the
    convolution GEMM, whose contraction is kernel_size * embed_dim long."""
    import ctypes
    from stable_audio_tools import _hip
    lib = _hip.lib()
    m = _model(cfg_name, dev)
    _hip.check(lib.sat_dit_profile(m._ensure_plan(), 1))
    try:
        _run(f"{cfg_name}_cfg1_T64", dev, SUITE.gemm_dtype)
        tot, cnt = ctypes.c_double(), ctypes.c_int32()
        mm, n, k = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        _hip.check(lib.sat_dit_profile_read(m._ensure_plan(), ctypes.byref(tot), ctypes.byref(cnt), ctypes.byref(mm), ctypes.byref(n), ctypes.byref(k)))
    finally:
        _hip.check(lib.sat_dit_profile(m._ensure_plan(), 0))
    d = CC.CONFIGS[cfg_name]["embed_dim"]
    want = (2 * 65, 8 * d, d) if cfg_name == "conv" else (2 * 65, 4 * d, 3 * d)      # (batch 2, S = 65; SwiGLU: value and gate halves)
    assert cnt.value == 1 and tot.value > 0
    assert (mm.value, n.value, k.value) == want


def test_config_driven_model_generates(dev):
    """A config with "allow_conv_ff": true builds through create_model_from_config, loads a reference-layout state dict with strict=True and
    generates through generate_diffusion_cond; the same seed with the off-centre taps zeroed gives another result."""
    import stable_audio_tools as S
    from stable_audio_tools import model_configs as MC
    from stable_audio_tools.inference.generation import generate_diffusion_cond
    from stable_audio_tools.models import _init
    cfg = copy.deepcopy(MC.reduced(MC.stable_audio_open_1_0()))
    dc = cfg["model"]["diffusion"]["config"]
    dc.update(ff_kwargs={"use_conv": True}, allow_conv_ff=True)
    with _init.skip_init():
        model = S.create_model_from_config(cfg)
    sd = CC.synth_weights(model.state_dict(), 0)
    assert any(k.endswith(".ff.ff.2.weight") and v.dim() == 3 and v.shape[2] == 3 for k, v in sd.items())
    b, steps, t_len = 1, 4, 16
    ratio = cfg["model"]["pretransform"]["config"]["downsampling_ratio"]
    audio = []
    for weights in (sd, CC.centre_taps_only(sd)):
        model.load_state_dict(weights, strict=True)
        model = model.to(dev).eval()
        cond = model.conditioner([{"seconds_start": 0, "seconds_total": 12}])
        from stable_audio_tools import synthetic
        cond["prompt"] = (synthetic.synth_input("prompt", (b, 128, dc["cond_token_dim"]), 1).to(dev), torch.ones(b, 128, device=dev))
        cond = {k: cond[k] for k in ("prompt", "seconds_start", "seconds_total")}
        audio.append(generate_diffusion_cond(model, steps=steps, cfg_scale=7.0, conditioning_tensors=cond, sample_size=t_len * ratio, seed=3,
                                             device=str(dev), sampler_type="dpmpp-3m-sde", sigma_min=0.3, sigma_max=500))
        torch.cuda.synchronize()
        assert audio[-1].shape == (b, 2, t_len * ratio) and torch.isfinite(audio[-1]).all() and float(audio[-1].abs().max()) > 0
    e = rel_l2(audio[0], audio[1])
    print(f"\n[dit conv ff generate, 4 steps] rel-L2 between the model and its centre taps alone {e:.2e}")
    assert e > 1e-3, f"zeroing the off-centre taps moved the audio by {e:.2e} only: the convolution reads the centre row alone"
