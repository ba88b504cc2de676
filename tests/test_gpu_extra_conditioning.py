"""Input-concat and prepend conditioning on the HIP DiT (reference models/dit.py:160-197, 270-315) against the REFERENCE's own outputs
(tests/golden/dit_extra_small.npz, generate_inpaint.npz: tests/golden/make_golden_extra.py).

* the suite's operand format at the reduced-DiT gates of test_gpu_models.py: T(2.5e-3) at CFG 1, T(1.2e-2) at CFG 7;
* the fp32 verification mode (gemm_dtype "fp32x") at 1e-4: what separates an indexing error (token order, RoPE offset, the global row,
  the concat signal scaled by c_in) from rounding.
"""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import cases  # noqa: E402
from test_extra_conditioning_host import CONCAT_DIM, CONFIGS, PREPEND_DIM, inpaint_config  # noqa: E402
from util import SUITE, assert_close, rel_l2  # noqa: E402

T = SUITE.tol
pytestmark = pytest.mark.gpu

# name -> (config, t_len, concat length Tc or None, prepend length P or None, cfg_scale, scale_phi, partly-zero prepend mask);
# the cases of make_golden_extra.py
CASES = {
    "concat_cfg1_T64": ("concat", 64, 64, None, 1.0, 0.0, False),
    "concat_cfg1_T77": ("concat", 77, 77, None, 1.0, 0.0, False),
    "concat_cfg7_T77": ("concat", 77, 77, None, 7.0, 0.0, False),
    "concat_resize_cfg1_T77": ("concat", 77, 50, None, 1.0, 0.0, False),
    "prepend_P3_cfg1_T64": ("prepend", 64, None, 3, 1.0, 0.0, False),
    "prepend_P3_cfg7_T64": ("prepend", 64, None, 3, 7.0, 0.0, False),
    "prepend_P70_cfg1_T64": ("prepend", 64, None, 70, 1.0, 0.0, False),
    "prepend_P3_masked_cfg7_T64": ("prepend", 64, None, 3, 7.0, 0.0, True),
    "both_cfg7_phi04_T77": ("both", 77, 77, 5, 7.0, 0.4, False),
    "prepend_only_cfg7_T64": ("prepend_only", 64, None, 4, 7.0, 0.0, False),
    # prepend models called without prepend tokens (no CFG batch on the prepend-only model: dit.py:270)
    "prepend_none_cfg1_T64": ("prepend", 64, None, None, 1.0, 0.0, False),
    "prepend_only_none_cfg7_T64": ("prepend_only", 64, None, None, 7.0, 0.0, False),
}


def _inputs(name, dev):
    from stable_audio_tools import synthetic
    cfg_name, t_len, tc, p, _, _, masked = CASES[name]
    x, t, c, g = cases.dit_inputs(2, t_len, 128, 96, 1)
    if CONFIGS[cfg_name]["cond_token_dim"] == 0:
        c = None
    cc = synthetic.synth_input("concat", (2, CONCAT_DIM, tc), 200 + tc) if tc else None
    pc = synthetic.synth_input("prepend", (2, p, PREPEND_DIM), 300 + p) if p else None
    pm = None
    if pc is not None:
        pm = torch.ones(2, p)
        if masked:
            pm[1, 1:] = 0
    to = lambda v: None if v is None else v.to(dev)
    return to(x), to(t), to(c), to(g), to(cc), to(pc), to(pm)


_MODELS = {}


def _model(cfg_name, dev):
    if cfg_name not in _MODELS:
        from stable_audio_tools import synthetic
        from stable_audio_tools.models import _init
        from stable_audio_tools.models.dit import DiffusionTransformer
        with _init.skip_init():
            m = DiffusionTransformer(**CONFIGS[cfg_name])
        m.load_state_dict(synthetic.synth_state_dict(m.state_dict(), 0))
        _MODELS[cfg_name] = m.to(dev).eval()
    return _MODELS[cfg_name]


def _run(name, dev, dtype):
    cfg_name, _, _, _, cfg_scale, phi, _ = CASES[name]
    m = _model(cfg_name, dev)
    m.set_gemm_dtype(dtype)
    x, t, c, g, cc, pc, pm = _inputs(name, dev)
    out = m(x, t, cross_attn_cond=c, global_embed=g, input_concat_cond=cc, prepend_cond=pc, prepend_cond_mask=pm, cfg_scale=cfg_scale,
            scale_phi=phi)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_extra_conditioning_vs_reference(dev, name):
    gold = cases.load("dit_extra_small")
    got = _run(name, dev, SUITE.gemm_dtype)
    gate = T(2.5e-3) if CASES[name][4] == 1.0 else T(1.2e-2)
    if name == "prepend_P70_cfg1_T64":
        # 70 prepend tokens (S = 135): measured 2.7e-3 with bf16 operands, 3.0e-4 with fp16, 5.8e-7 in fp32 -- operand rounding of the
        # longer sequence, not indexing (the fp32x test pins that at 1e-4)
        gate = T(4e-3)
    e = assert_close(f"{name} ({SUITE.gemm_dtype}) vs reference", got, gold[name], gate)
    print(f"\n[extra conditioning {name}, {SUITE.gemm_dtype}] rel-L2 vs reference {e:.2e} (gate {gate:.1e})")


@pytest.mark.parametrize("name", list(CASES))
def test_extra_conditioning_fp32_vs_reference(dev, name):
    gold = cases.load("dit_extra_small")
    try:
        got = _run(name, dev, "fp32x")
    finally:
        _model(CASES[name][0], dev).set_gemm_dtype(SUITE.gemm_dtype)
    e = assert_close(f"{name} (fp32x) vs reference", got, gold[name], 1e-4)
    print(f"\n[extra conditioning {name}, fp32x] rel-L2 vs reference {e:.2e}")


def test_prepend_mask_has_no_effect(dev):
    """prepend_cond_mask never reaches the layers (reference transformer.py:787-802): all-ones and partly-zero masks, same bits."""
    a = _run("prepend_P3_cfg7_T64", dev, SUITE.gemm_dtype)
    b = _run("prepend_P3_masked_cfg7_T64", dev, SUITE.gemm_dtype)
    assert torch.equal(a, b)


@pytest.mark.parametrize("dtype", ["suite", "fp32x"])
@pytest.mark.parametrize("name", ["concat_cfg7_T77", "both_cfg7_phi04_T77", "prepend_only_cfg7_T64", "concat_resize_cfg1_T77"])
def test_fused_denoise_matches_forward(dev, name, dtype):
    """prepare_generation + denoise (one sat_dit_denoise_cfg per step) == VDenoiser(forward): c_in scales x only, the concat
    signal and the prepend tokens enter unscaled.  In fp32 (no operand rounding) the two agree to 1e-5; a concat signal scaled by
    c_in would be off by O(1) at sigma 12.  In the suite's format the two round c_in * x at different points, and CFG 7 amplifies the
    16-bit roundings that flip (measured at sigma 12: 1.3e-3 with fp16 operands, 9.7e-3 with bf16)."""
    cfg_name, _, _, _, cfg_scale, phi, _ = CASES[name]
    fmt = SUITE.gemm_dtype if dtype == "suite" else dtype
    gate = T(2e-2) if dtype == "suite" else 1e-5
    m = _model(cfg_name, dev)
    m.set_gemm_dtype(fmt)
    try:
        x, _, c, g, cc, pc, _ = _inputs(name, dev)
        for sigma in (0.7, 12.0):
            c_skip, c_out, c_in = 1.0 / (sigma ** 2 + 1), -sigma / (sigma ** 2 + 1) ** 0.5, 1.0 / (sigma ** 2 + 1) ** 0.5
            t = torch.full((x.shape[0],), float(torch.atan(torch.tensor(sigma, dtype=torch.float64)) / torch.pi * 2), device=dev)
            want = m(x * c_in, t, cross_attn_cond=c, global_embed=g, input_concat_cond=cc, prepend_cond=pc, cfg_scale=cfg_scale,
                     scale_phi=phi) * c_out + x * c_skip
            m.prepare_generation(c, g, cfg_scale, input_concat_cond=cc, prepend_cond=pc)
            got = m.denoise(x, sigma, cfg_scale=cfg_scale, scale_phi=phi)
            torch.cuda.synchronize()
            e = rel_l2(got, want)
            print(f"\n[fused denoise {name}, {fmt}, sigma {sigma}] rel-L2 vs VDenoiser(forward) {e:.2e}")
            assert e <= gate, f"{name} {fmt} sigma {sigma}: fused denoise vs VDenoiser(forward) rel-L2 {e:.3e} > {gate:.1e}"
    finally:
        m.set_gemm_dtype(SUITE.gemm_dtype)


def test_call_without_prepend_after_one_with_it(dev):
    """A call without prepend tokens right after one with them, on the SAME cross / global tensors (the prepared context is then
    reused): it must run the plain sequence [global | T], not keep the earlier call's P tokens -- forward, and the fused
    prepare_generation + denoise path, where on the prepend-only model the earlier CFG batch must not linger either."""
    gold = cases.load("dit_extra_small")
    m = _model("prepend", dev)
    m.set_gemm_dtype(SUITE.gemm_dtype)
    x, t, c, g, _, pc, _ = _inputs("prepend_P3_cfg1_T64", dev)
    m(x, t, cross_attn_cond=c, global_embed=g, prepend_cond=pc)
    got = m(x, t, cross_attn_cond=c, global_embed=g)
    e = assert_close("forward without prepend after one with it vs reference", got, gold["prepend_none_cfg1_T64"], T(2.5e-3))
    sigma = 0.7
    c_skip, c_out, c_in = 1.0 / (sigma ** 2 + 1), -sigma / (sigma ** 2 + 1) ** 0.5, 1.0 / (sigma ** 2 + 1) ** 0.5
    tt = torch.full((x.shape[0],), float(torch.atan(torch.tensor(sigma, dtype=torch.float64)) / torch.pi * 2), device=dev)
    want = m(x * c_in, tt, cross_attn_cond=c, global_embed=g) * c_out + x * c_skip
    m.prepare_generation(c, g, 1.0, prepend_cond=pc)
    m.prepare_generation(c, g, 1.0)
    d1 = rel_l2(m.denoise(x, sigma), want)
    m2 = _model("prepend_only", dev)
    m2.set_gemm_dtype(SUITE.gemm_dtype)
    x, t, _, g, _, pc, _ = _inputs("prepend_only_cfg7_T64", dev)
    got = m2(x, t, global_embed=g, cfg_scale=7.0)
    e2 = assert_close("prepend-only model without prepend, CFG 7 (no CFG batch) vs reference", got, gold["prepend_only_none_cfg7_T64"],
                      T(2.5e-3))
    want = m2(x * c_in, tt, global_embed=g, cfg_scale=7.0) * c_out + x * c_skip
    m2.prepare_generation(None, g, 7.0, prepend_cond=pc)
    m2.prepare_generation(None, g, 7.0)
    d2 = rel_l2(m2.denoise(x, sigma, cfg_scale=7.0), want)
    torch.cuda.synchronize()
    print(f"\n[no prepend after prepend] forward vs reference {e:.2e}, prepend-only CFG 7 {e2:.2e}; fused vs forward {d1:.2e}, {d2:.2e}")
    assert d1 <= T(2.5e-3) and d2 <= T(2.5e-3), (d1, d2)


def test_generate_inpaint_model_vs_reference(dev):
    """generate_diffusion_cond of a reduced "diffusion_cond_inpaint" model (input_concat_ids = [inpaint_mask, inpaint_masked_input],
    one-element-list conditioning entries) against the reference's own 8-step DPM-Solver++(3M) SDE run with recorded draws; gate of
    the reference-generate tests (test_reference_generate.py: latents 3e-3 for bf16 operands)."""
    import stable_audio_tools as S
    from stable_audio_tools import synthetic
    from stable_audio_tools.inference.generation import generate_diffusion_cond
    from stable_audio_tools.models import _init
    gold = cases.load("generate_inpaint")
    cfg = inpaint_config()
    with _init.skip_init():
        model = S.create_model_from_config(cfg)
    model.load_state_dict(synthetic.synth_state_dict(model.state_dict(), 0))
    model = model.to(dev).eval()
    model.model.model.set_gemm_dtype(SUITE.gemm_dtype)
    dc = cfg["model"]["diffusion"]["config"]
    ratio = cfg["model"]["pretransform"]["config"]["downsampling_ratio"]
    b, t_len = 2, 24
    cond = model.conditioner([{"seconds_start": 0, "seconds_total": 10 + i} for i in range(b)])
    cond["prompt"] = [synthetic.synth_input("prompt", (b, 128, dc["cond_token_dim"]), 41).to(dev), torch.ones(b, 128, device=dev)]
    cond = {k: cond[k] for k in ("prompt", "seconds_start", "seconds_total")}
    mask = torch.ones(b, 1, t_len)
    mask[0, :, 6:15] = 0
    mask[1, :, 12:] = 0
    cond["inpaint_mask"] = [mask.to(dev)]
    cond["inpaint_masked_input"] = [(synthetic.synth_input("inpaint_latents", (b, 64, t_len), 42) * mask).to(dev)]
    step = []
    while f"step{len(step)}" in gold:
        step.append(gold[f"step{len(step)}"])
    it = iter(step)
    lat = generate_diffusion_cond(model, steps=8, cfg_scale=7.0, conditioning_tensors=cond, sample_size=t_len * ratio, seed=11, device=str(dev),
                                  sampler_type="dpmpp-3m-sde", sigma_min=0.3, sigma_max=500, return_latents=True, noise=gold["noise"],
                                  noise_sampler=lambda s, sn: next(it).to(dev))
    e = assert_close("inpaint-model generation vs reference", lat, gold["latents"], T(3e-3))
    print(f"\n[inpaint-model generate_diffusion_cond, {SUITE.gemm_dtype}] rel-L2 latents vs reference {e:.2e}")
