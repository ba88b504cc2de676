"""Patchified DiTs (DiffusionTransformer patch_size > 1, reference models/dit.py:38,88-89,119-120,197-224) on the HIP DiT against the
REFERENCE's own outputs (tests/golden/dit_patch_small*.npz: tests/golden/make_golden_dit_families.py patch).  Gates: the harness,
tests/dit_family_gpu.py.

* the suite's operand format at the reduced-DiT gates;
* the fp32 verification mode (gemm_dtype "fp32x"): what separates an indexing error (feature order, a frame or a row off by one, a
  concat source frame per token) from rounding.  The generator asserts that each such mistake moves the output by at least 5e-2;
* four cases again with the LayerNorm fusion off and with the fused to_q + cross-attention launch off, and through the fused sampler step;
* per-block operand formats, conformer + convolutional feed-forward under the three opt-ins, fp8;
* one config-driven generation, which must differ from the same weights with the project_in columns in (p c) order;
* the C ABI: sat_dit_plan_set_patch after finalize, a t_len that is no multiple of the patch size.
Measured errors, the reference's own rounded-operand figures (``<case>__r16_*``) and the gates: profiles/dit_patch_verification.txt.
"""
import ctypes
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import dit_patch_cases as PC  # noqa: E402
from dit_family_gpu import FP32X_GATE, Harness, generate, reduced_model  # noqa: E402
from util import SUITE, rel_l2  # noqa: E402

pytestmark = pytest.mark.gpu
H = Harness(PC.FAMILY)


@pytest.mark.parametrize("name", list(PC.CASES))
def test_patch_vs_reference(dev, name):
    """Measured (profiles/dit_patch_verification.txt): fp16 2.2e-4 - 2.7e-4 at CFG 1 (gate 6.3e-4), 8.0e-4 - 1.7e-3 at CFG 7 (gate 3.0e-3); bf16
    1.9e-3 - 2.1e-3 (gate 2.5e-3) and 6.5e-3 - 1.15e-2 (gate 1.2e-2) -- except p8_c8_cfg7_T72, which under SAT_TEST_DTYPE=bf16 is at 1.41e-2
    and MISSES the 1.2e-2 gate (it passes in fp16, 1.68e-3, and in fp32x, 3.4e-6, so no index is wrong).  The figure does not move with the
    LayerNorm or the cross-attention fusion; without CFG this 8-channel, 10-rows-per-sequence model is 3.06e-3 from its own fp32x output in
    bf16 against 1.99e-3 for p2: 1.5 times as sensitive to operand rounding, in fp16 alike, and CFG 7 multiplies it (the reference with
    bf16-rounded operands: 1.96e-2).  The gate is the one set for this test and is kept."""
    H.check_vs_reference(dev, name, SUITE.gemm_dtype, H.gate(name), rounded=True)


@pytest.mark.parametrize("name", list(PC.CASES))
def test_patch_fp32_vs_reference(dev, name):
    if PC.CASES[name][0] == "p2_hd128":
        # the fp32 verification kernels keep 64-channel heads, with or without patches (DiffusionTransformer._check_options): the
        # 128-channel-head case has its 16-bit gates above and the boundary kernels their fp32 gates on every other case
        with pytest.raises(NotImplementedError, match="dim_heads=128"):
            H.run(name, dev, "fp32x")
        return
    H.check_vs_reference(dev, name, "fp32x", FP32X_GATE)


OTHER_PATHS = ["p2_cfg7_T78", "p2_adaln_cfg7_T78", "p2_prepend_cfg7_T78", "p2_concat_cfg7_T78"]


@pytest.mark.parametrize("path", ["ln_fold_off", "cross_fusion_off"])
@pytest.mark.parametrize("name", OTHER_PATHS)
def test_patch_on_the_other_launch_paths(dev, name, path):
    H.check_vs_reference(dev, name, SUITE.gemm_dtype, H.gate(name), path, ln_fold=path != "ln_fold_off", cross_fusion=path != "cross_fusion_off")


@pytest.mark.parametrize("dtype", ["suite", "fp32x"])
@pytest.mark.parametrize("name", OTHER_PATHS)
def test_fused_denoise_matches_forward(dev, name, dtype):
    """c_in scales the latent channels only: on p2_concat an xscale on the concat channels shows here."""
    H.check_fused_denoise(dev, name, dtype)


def test_patch_with_per_block_formats(dev):
    """[fp16, bf16, fp16] on p2 at CFG 7."""
    H.check_per_block_formats(dev, "p2_cfg7_T78")


@pytest.mark.parametrize("mode", ["fp8", "fp8-all"])
def test_patch_fp8(dev, mode):
    """The e4m3 modes take a patchified model (the block kernels are the P = 1 plan's on half the rows).  Gate: what
    tests/test_gpu_models.py::test_dit_fp8_gemm_mode applies to the reduced DiT against the fp32 reference without CFG, 3e-2."""
    name = "p2_cfg1_T64"
    assert torch.isfinite(H.check_vs_reference(dev, name, mode, 3e-2)).all()


def test_range_and_residual_reports_run_on_a_patch_plan(dev):
    name = "p2_cfg1_T64"
    m = H.model("p2", dev)
    base = H.run(name, dev, SUITE.gemm_dtype)
    m.activation_range_report(True)
    m.residual_stream_report(True)
    try:
        got = H.run(name, dev, SUITE.gemm_dtype)
    finally:
        resid = m.residual_stream_report(False)
        rows = m.activation_range_report(False)
    assert torch.equal(got, base), "the reports changed the output"
    assert len(resid) == 3 * m.depth and all(r["max_abs"] > 0 for r in resid)
    # the reports count token rows: S = 1 + 64 / 2 = 33 rows per sequence, two sequences
    a_qkv = [r for r in rows if r["buffer"] == "a_qkv"]
    assert len(a_qkv) == m.depth and all(r["elements"] == 2 * 33 * m.embed_dim * r["launches"] for r in a_qkv)


def test_patch_c_abi_state_and_bad_length(dev):
    """sat_dit_plan_set_patch after finalize is SAT_E_STATE; t_len 77 on a P = 2 plan is SAT_E_INVALID in all three calls that take one, and
    not a bit of `out` is written."""
    from stable_audio_tools import _hip
    lib = _hip.lib()
    m = H.model("p2", dev)
    x, t, kw = H.inputs("p2_cfg1_T64", dev)
    m(x, t, **kw)            # plan, context and workspace for bf = 2
    plan = m._plan
    opts = _hip.SatDitPatchOptions(2)
    assert lib.sat_dit_plan_set_patch(plan, ctypes.byref(opts), ctypes.sizeof(opts)) == -5 and b"finalized" in lib.sat_last_error()
    nbytes = ctypes.c_size_t()
    assert lib.sat_dit_workspace_bytes(plan, 2, 77, ctypes.byref(nbytes)) == -1 and b"patch_size 2" in lib.sat_last_error()
    ws = m._workspace(2, 78)
    x77 = x[:, :, :1].expand(2, 64, 77).contiguous()
    out = torch.full((2, 64, 77), 123.25, device=dev)
    before = out.clone()
    rc = lib.sat_dit_forward(plan, _hip.ptr(x77), _hip.ptr(t), _hip.ptr(out), 2, 77, _hip.ptr(ws), ws.numel(), _hip.stream())
    assert rc == -1 and b"77" in lib.sat_last_error() and b"patch_size 2" in lib.sat_last_error()
    rc = lib.sat_dit_denoise_cfg(plan, _hip.ptr(x77), 1.0, 1.0, 0.0, _hip.ptr(out), 2, 77, _hip.ptr(ws), ws.numel(), _hip.stream())
    assert rc == -1 and b"patch_size 2" in lib.sat_last_error()
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), before.view(torch.int32)), "a refused call wrote to out"
    with pytest.raises(ValueError, match="T = 77.*patch_size = 2"):
        m(x77, t, **kw)


def test_config_driven_model_generates(dev):
    """A config with patch_size 2 and "allow_patch_size": true builds through create_model_from_config, loads a reference-layout state dict
    with strict=True and generates through generate_diffusion_cond; the same seed with the project_in columns in (p c) order gives another
    result, and a sample_size that is no whole number of patches is refused before sampling."""
    from stable_audio_tools import synthetic
    from stable_audio_tools.inference.generation import generate_diffusion_cond
    cfg, model = reduced_model(patch_size=2, allow_patch_size=True)
    sd = synthetic.synth_state_dict(model.state_dict(), 0)
    assert sd["model.model.transformer.project_in.weight"].shape[1] == 2 * cfg["model"]["diffusion"]["config"]["io_channels"]
    wrong = dict(sd)
    wrong["model.model.transformer.project_in.weight"] = PC.in_columns_pc(
        {"transformer.project_in.weight": sd["model.model.transformer.project_in.weight"]}, 2)["transformer.project_in.weight"]
    steps, t_len = 8, 16
    ratio = cfg["model"]["pretransform"]["config"]["downsampling_ratio"]
    assert model.min_input_length == 2 * ratio
    (a0, cond), (a1, _) = (generate(model, cfg, dev, weights, steps=steps, seed=3, t_len=t_len) for weights in (sd, wrong))
    e = rel_l2(a0, a1)
    print(f"\n[dit patch generate, 8 steps] rel-L2 between the model and its project_in columns in (p c) order {e:.2e}")
    assert e > 1e-3, f"permuting the project_in columns moved the audio by {e:.2e} only"
    with pytest.raises(ValueError, match="patch_size = 2"):
        generate_diffusion_cond(model, steps=steps, cfg_scale=7.0, conditioning_tensors=cond, sample_size=(t_len + 1) * ratio, seed=3, device=str(dev))
