"""conformer, remove_norms and ff_kwargs glu=False on the HIP DiT (reference models/transformer.py:557-591, 621-645, 259-268, 680-700)
against the REFERENCE's own outputs (tests/golden/dit_block_options_small*.npz: tests/golden/make_golden_dit_families.py block_options).
Gates: the harness, tests/dit_family_gpu.py.

* the suite's operand format at the reduced-DiT gates;
* the fp32 verification mode (gemm_dtype "fp32x"): what separates an indexing error (a conv window off by one row or leaking
  into the neighbouring sequence, the chunk order of the GLU, a norm applied where it was removed) from rounding;
* four cases again with the LayerNorm fold off and with the fused to_q + cross-attention launch off, and through the fused sampler step;
* all three options with per-block operand formats;
* the depthwise-conv + mid_norm + SiLU kernel and the plain-activation GEMM epilogue alone, against float64 restatements.
Measured errors, the reference's own rounded-operand figures (``<case>__r16_*``) and the gates: profiles/dit_block_options_verification.txt.
"""
import ctypes
import os
import sys

import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import dit_block_options_cases as BC  # noqa: E402
from dit_family_gpu import FP32X_GATE, Harness, generate, reduced_model  # noqa: E402
from util import FORMATS, SUITE, assert_close, assert_close_rows_blocks, assert_close_sliced, guarded, rel_l2  # noqa: E402

pytestmark = pytest.mark.gpu
H = Harness(BC.FAMILY)


@pytest.mark.parametrize("name", list(BC.CASES))
def test_block_options_vs_reference(dev, name):
    H.check_vs_reference(dev, name, SUITE.gemm_dtype, H.gate(name), rounded=True)


@pytest.mark.parametrize("name", list(BC.CASES))
def test_block_options_fp32_vs_reference(dev, name):
    H.check_vs_reference(dev, name, "fp32x", FP32X_GATE)


OTHER_PATHS = ["conf_cfg7_T77", "nonorm_adaln_cfg7_T77", "all3_cfg7_T77", "conf_prepend_cfg7_T77"]


@pytest.mark.parametrize("path", ["ln_fold_off", "cross_fusion_off"])
@pytest.mark.parametrize("name", OTHER_PATHS)
def test_block_options_on_the_other_launch_paths(dev, name, path):
    """The standalone LayerNorm in front of pointwise_conv and the rounding launch of remove_norms instead of the residual image; to_q +
    attention core as two kernels."""
    H.check_vs_reference(dev, name, SUITE.gemm_dtype, H.gate(name), path, ln_fold=path != "ln_fold_off", cross_fusion=path != "cross_fusion_off")


def test_remove_norms_results_do_not_depend_on_the_layernorm_fusion(dev):
    """With remove_norms the A operand is the rounded residual row either way: written by the previous residual epilogue under the fold,
    by the rounding launch without it.  Same bits in, same kernels behind: same bits out."""
    a = H.run("nonorm_cfg7_T77", dev, SUITE.gemm_dtype, ln_fold=True)
    b = H.run("nonorm_cfg7_T77", dev, SUITE.gemm_dtype, ln_fold=False)
    assert torch.equal(a, b), f"remove_norms: fold on / off differ, rel-L2 {rel_l2(a, b):.3e}"


@pytest.mark.parametrize("dtype", ["suite", "fp32x"])
@pytest.mark.parametrize("name", OTHER_PATHS)
def test_fused_denoise_matches_forward(dev, name, dtype):
    H.check_fused_denoise(dev, name, dtype)


@pytest.mark.parametrize("name", ["all3_cfg1_T64", "all3_cfg7_T77"])
def test_all_three_options_with_per_block_formats(dev, name):
    """[fp16, bf16, fp16]: block 1 keeps its weight images, the conformer's three 16-bit buffers and the SiLU hidden state in bf16, and its
    to_qkv rounds the fp32 rows itself (no image from block 0's FF-out in its format)."""
    H.check_per_block_formats(dev, name)


def test_block_options_c_abi_after_finalize_and_range_report(dev):
    """sat_dit_plan_set_block_options is refused once the plan is finalized; the range report has no rows for these plans."""
    from stable_audio_tools import _hip
    lib = _hip.lib()
    m = H.model("conf", dev)
    plan = m._ensure_plan()
    opts = _hip.SatDitBlockOptions(0, 0, 1)
    assert lib.sat_dit_plan_set_block_options(plan, ctypes.byref(opts), ctypes.sizeof(opts)) == -5 and b"finalized" in lib.sat_last_error()
    assert lib.sat_dit_range_report(plan, 1) == -2 and b"sat_dit_plan_set_block_options" in lib.sat_last_error()
    with pytest.raises(NotImplementedError, match="activation_range_report"):
        m.activation_range_report(True)


def test_config_driven_model_generates(dev):
    """A config with all three options builds through create_model_from_config, loads a reference-layout state dict with strict=True
    and generates through generate_diffusion_cond."""
    from stable_audio_tools import synthetic
    cfg, model = reduced_model(conformer=True, remove_norms=True, ff_kwargs={"glu": False})
    sd = synthetic.synth_state_dict(model.state_dict(), 0)
    assert any(".conformer.depthwise_conv.weight" in k for k in sd) and any(".ff.ff.0.1.weight" in k for k in sd) and not any("pre_norm" in k for k in sd)
    generate(model, cfg, dev, sd, steps=2, seed=3)


# ------------------------------------------------------------------------------------------------------------ the two kernels alone
@pytest.mark.parametrize("fmt", FORMATS, ids=repr)
@pytest.mark.parametrize("variant", [0, 1, 2, 3], ids=["tile16_registers", "one_row", "tile32_lds", "tile8_registers"])
@pytest.mark.parametrize("b, s, d", [(2, 78, 256), (3, 5, 256), (1, 17, 320)])
def test_dwconv_ln_silu(dev, b, s, d, variant, fmt):
    """sat_dwconv_ln_silu_*: silu(LayerNorm_d(depthwise 17-tap conv along each sequence)) against float64 on the same rounded input.
    (2, 78, 256): five row tiles with a tail, the second sequence starts mid-tile; (3, 5, 256): every window is clipped at both ends;
    (1, 17, 320): row 8 is the first whose window is whole, and d is no multiple of 256.  Every sequence but the first is scaled by 100 (the
    LayerNorm hides a sequence's own scale; one leaked row of a neighbour dominates the window it enters), one input row is all zeros,
    gamma and beta are non-trivial.  Gated per row at the q / k tolerance of the kernel tests; the output is guarded and finite.
    variant 0 is the kernel the plan runs, 1 to 3 the designs it was measured against (tools/dit_block_options_timing.py)."""
    from stable_audio_tools import _hip
    lib = _hip.lib()
    gen = torch.Generator().manual_seed(1000 * b + 10 * s + d)
    x = torch.randn((b, s, d), generator=gen)
    x[1:] *= 100.0
    x[0, min(3, s - 1)] = 0.0
    x = x.to(fmt.dtype)
    w = torch.randn((d, 1, 17), generator=gen) * 0.3
    gamma = 0.5 + torch.rand((d,), generator=gen)
    beta = torch.randn((d,), generator=gen) * 0.3
    conv = F.conv1d(x.double().transpose(1, 2), w.double(), padding=8, groups=d).transpose(1, 2)          # [b, s, d]
    want = F.silu(F.layer_norm(conv, (d,), gamma.double(), beta.double(), eps=1e-5))
    out = guarded((b * s, d), fmt.dtype, dev, name="dwconv output")
    xd, wd, gd, bd = x.reshape(b * s, d).contiguous().to(dev), w.reshape(d, 17).contiguous().to(dev), gamma.to(dev), beta.to(dev)
    fn = fmt.fn(lib, "sat_dwconv_ln_silu_bf16")
    _hip.check(fn(_hip.ptr(xd), _hip.ptr(wd), _hip.ptr(gd), _hip.ptr(bd), _hip.ptr(out.t), b, s, d, variant, _hip.stream()))
    torch.cuda.synchronize()
    out.check().assert_written()
    want = want.reshape(b * s, d).float()
    e = assert_close(f"dwconv_ln_silu {fmt} ({b}, {s}, {d})", out.t, want, fmt.tol(4e-3))
    assert_close_sliced(f"dwconv_ln_silu {fmt} ({b}, {s}, {d}) per row", out.t, want, fmt.tol(4e-3), (0,), fmt.round)
    print(f"\n[dwconv_ln_silu {fmt} ({b}, {s}, {d}) variant {variant}] rel-L2 {e:.2e}")


# forced tiles: 1 / 5 the two 128 x 128 kernels with the un-swapped epilogue, 15 / 16 / 22 the ring tiles (transposed epilogue); 0 = the
# route's choice.  Tile 30 is 192 columns wide and cannot take N = 1024: it runs at N = 768
@pytest.mark.parametrize("fmt", FORMATS, ids=repr)
@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("variant, n", [(0, 1024), (1, 1024), (5, 1024), (15, 1024), (16, 1024), (22, 1024), (30, 768)])
def test_gemm_silu_epilogue(dev, variant, n, bias, fmt):
    """sat_gemm_act_*: h = silu(a w^T + bias) (and the identity, the conformer's pointwise_conv) against float64 on the same rounded
    operands, per row and per 32 x 32 accumulator block.  M = 156: a tail in every tile height."""
    from stable_audio_tools import _hip
    lib = _hip.lib()
    m, k = 156, 256
    gen = torch.Generator().manual_seed(17 + n)
    a = torch.randn((m, k), generator=gen).to(fmt.dtype)
    w = (torch.randn((n, k), generator=gen) * 0.1).to(fmt.dtype)
    bv = torch.randn((n,), generator=gen) if bias else None
    pre = a.double() @ w.double().T + (bv.double() if bias else 0.0)
    ad, wd, bd = a.to(dev), w.to(dev), (bv.to(dev) if bias else None)
    fn = fmt.fn(lib, "sat_gemm_act_bf16")
    for act, want in ((1, F.silu(pre)), (0, pre)):
        out = guarded((m, n), fmt.dtype, dev, name="gemm_act output")
        _hip.check(fn(_hip.ptr(ad), _hip.ptr(wd), _hip.ptr(bd), _hip.ptr(out.t), m, n, k, act, variant, _hip.stream()))
        torch.cuda.synchronize()
        out.check().assert_written()
        e = assert_close(f"gemm_act {fmt} act {act} variant {variant}", out.t, want.float(), fmt.tol(4e-3))
        assert_close_rows_blocks(f"gemm_act {fmt} act {act} variant {variant}", out.t, want.float(), fmt.tol(4e-3), fmt.round)
        print(f"\n[gemm_act {fmt} act {act} variant {variant} n {n} {'bias' if bias else 'no bias'}] rel-L2 {e:.2e}")


def test_gemm_act_refuses_the_8_phase_kernel(dev):
    """The plain-activation epilogue lives in the ring tiles: a variant that forces the 8-phase kernel is an error, not a SwiGLU run."""
    from stable_audio_tools import _hip
    lib = _hip.lib()
    z16 = lambda *shape: torch.zeros(shape, dtype=torch.bfloat16, device=dev)
    a, w, h = z16(256, 256), z16(1024, 256), z16(256, 1024)
    rc = lib.sat_gemm_act_bf16(_hip.ptr(a), _hip.ptr(w), None, _hip.ptr(h), 256, 1024, 256, 1, 80, _hip.stream())
    assert rc == -2 and b"plain-activation" in lib.sat_last_error()
    torch.cuda.synchronize()
