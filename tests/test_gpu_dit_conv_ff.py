"""Convolutional feed-forwards (ff_kwargs use_conv, reference models/transformer.py:211-287) on the HIP DiT against the REFERENCE's own
outputs (tests/golden/dit_conv_ff_small*.npz: tests/golden/make_golden_dit_families.py conv_ff).  Gates: the harness, tests/dit_family_gpu.py.

* the suite's operand format at the reduced-DiT gates;
* the fp32 verification mode (gemm_dtype "fp32x"): what separates an indexing error (a window off by one row or leaking into the
  neighbouring sequence, taps in the wrong order) from rounding;
* four cases again with the LayerNorm fusion switched off and with the fused to_q + cross-attention launch off, and through the fused
  sampler step;
* conv_all_adaln with per-block operand formats;
* one config-driven generation, which must differ from the same model with the off-centre taps zeroed.
Measured errors, the reference's own rounded-operand figures (``<case>__r16_*``) and the gates: profiles/dit_conv_ff_verification.txt.
The reference with only the operands of its Linears and Conv1ds rounded is at 4.4e-4 - 4.9e-4 (CFG 1) / 2.2e-3 - 2.3e-3 (CFG 7) in fp16 and
3.6e-3 - 3.9e-3 / 1.7e-2 - 1.9e-2 in bf16 on these cases, the figures of the block-option cases those gates already serve.
"""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import dit_conv_ff_cases as CC  # noqa: E402
from dit_family_gpu import FP32X_GATE, Harness, generate, reduced_model  # noqa: E402
from util import SUITE, rel_l2  # noqa: E402

pytestmark = pytest.mark.gpu
H = Harness(CC.FAMILY)


@pytest.mark.parametrize("name", list(CC.CASES))
def test_conv_ff_vs_reference(dev, name):
    H.check_vs_reference(dev, name, SUITE.gemm_dtype, H.gate(name), rounded=True)


@pytest.mark.parametrize("name", list(CC.CASES))
def test_conv_ff_fp32_vs_reference(dev, name):
    H.check_vs_reference(dev, name, "fp32x", FP32X_GATE)


OTHER_PATHS = ["conv_cfg7_T77", "conv_silu_cfg7_T77", "conv_prepend_cfg7_T77", "conv_all_adaln_cfg7_T77"]


@pytest.mark.parametrize("path", ["ln_fold_off", "cross_fusion_off"])
@pytest.mark.parametrize("name", OTHER_PATHS)
def test_conv_ff_on_the_other_launch_paths(dev, name, path):
    H.check_vs_reference(dev, name, SUITE.gemm_dtype, H.gate(name), path, ln_fold=path != "ln_fold_off", cross_fusion=path != "cross_fusion_off")


@pytest.mark.parametrize("dtype", ["suite", "fp32x"])
@pytest.mark.parametrize("name", OTHER_PATHS)
def test_fused_denoise_matches_forward(dev, name, dtype):
    H.check_fused_denoise(dev, name, dtype)


@pytest.mark.parametrize("name", ["conv_all_adaln_cfg1_T64", "conv_all_adaln_cfg7_T77"])
def test_conv_ff_with_per_block_formats(dev, name):
    """[fp16, bf16, fp16]: block 1 keeps its tap-major weight images and the SiLU hidden state in bf16."""
    H.check_per_block_formats(dev, name)


def test_conv_ff_c_abi_after_finalize_and_range_report(dev):
    import ctypes
    from stable_audio_tools import _hip
    lib = _hip.lib()
    m = H.model("conv", dev)
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
    m = H.model(cfg_name, dev)
    _hip.check(lib.sat_dit_profile(m._ensure_plan(), 1))
    try:
        H.run(f"{cfg_name}_cfg1_T64", dev, SUITE.gemm_dtype)
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
    cfg, model = reduced_model(ff_kwargs={"use_conv": True}, allow_conv_ff=True)
    sd = CC.synth_weights(model.state_dict(), 0)
    assert any(k.endswith(".ff.ff.2.weight") and v.dim() == 3 and v.shape[2] == 3 for k, v in sd.items())
    audio = [generate(model, cfg, dev, weights, steps=4, seed=3)[0] for weights in (sd, CC.centre_taps_only(sd))]
    e = rel_l2(audio[0], audio[1])
    print(f"\n[dit conv ff generate, 4 steps] rel-L2 between the model and its centre taps alone {e:.2e}")
    assert e > 1e-3, f"zeroing the off-centre taps moved the audio by {e:.2e} only: the convolution reads the centre row alone"
