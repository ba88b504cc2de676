"""Convolutional feed-forwards (ff_kwargs use_conv) without a GPU: the option needs its own opt-in (allow_conv_ff, by keyword, by config key
or by generate.py --allow-conv-ff), the modules hold the reference's parameter names and shapes, the combinations outside the HIP path raise
with a reason, sat_dit_plan_set_ff_conv checks its arguments, the float64 restatement of the convolution GEMM (tests/conv_ff_units.py) is
F.conv1d, and the per-row / 32 x 32-block gate of tests/util.py rejects the faults this kernel can have.
(That the plan's tap-major packing equals the restatement's is shown on the device, where the packing runs: tests/test_gpu_conv_ff_kernels.py.)"""
import ctypes
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import cases  # noqa: E402
import conv_ff_units as cu  # noqa: E402
import dit_conv_ff_cases as CC  # noqa: E402
from dit_family_host import build as _build, check_state_dict_keys, model_config as _model_config  # noqa: E402
from util import assert_close_rows_blocks, bf16_round  # noqa: E402


# ------------------------------------------------------------------------------------------------------------------- construction
@pytest.mark.parametrize("ff", [dict(use_conv=True), dict(use_conv=True, glu=False), dict(use_conv=True, conv_kernel_size=5)])
def test_use_conv_needs_allow_conv_ff(ff):
    for kw in (dict(), dict(allow_block_options=True)):
        with pytest.raises(NotImplementedError, match="use_conv") as e:
            _build(**dict(cases.SMALL_DIT, ff_kwargs=ff), **kw)
        assert "allow_block_options" in str(e.value) and "allow_conv_ff" in str(e.value)
    m = _build(**dict(cases.SMALL_DIT, ff_kwargs=ff), **CC.PRODUCT_KWARGS)
    assert m.transformer.ff_conv_kernel == ff.get("conv_kernel_size", 3)
    if ff.get("glu", True):          # under GLU only FF-out is a convolution and allow_block_options is not needed
        _build(**dict(cases.SMALL_DIT, ff_kwargs=ff), allow_conv_ff=True)
    else:
        with pytest.raises(NotImplementedError, match="allow_block_options"):
            _build(**dict(cases.SMALL_DIT, ff_kwargs=ff), allow_conv_ff=True)


def test_the_config_key_reaches_the_constructor():
    import stable_audio_tools as S
    from stable_audio_tools.models import _init
    from stable_audio_tools.models.diffusion import DiTWrapper
    with _init.skip_init(), pytest.raises(NotImplementedError, match="use_conv"):
        S.create_model_from_config(_model_config(ff_kwargs={"use_conv": True}))          # DiTWrapper does not default the opt-in
    with _init.skip_init(), pytest.raises(NotImplementedError, match="use_conv"):
        DiTWrapper(**dict(cases.SMALL_DIT, ff_kwargs={"use_conv": True}))
    with _init.skip_init():
        model = S.create_model_from_config(_model_config(ff_kwargs={"use_conv": True, "glu": False, "conv_kernel_size": 5}, allow_conv_ff=True))
    tr = model.model.model.transformer
    assert tr.ff_conv_kernel == 5 and tr.block_options == (0, 0, 0)
    assert tuple(tr.layers[0].ff.ff[2].weight.shape) == (tr.dim, 4 * tr.dim, 5)


def test_generate_flag_sets_the_config_key(monkeypatch):
    import generate
    import stable_audio_tools as S
    from stable_audio_tools.models import _init
    base = ["generate.py", "--output-dir", "o", "--cond-yaml-path", "c"]
    monkeypatch.setattr(sys, "argv", base)
    cfg = generate.apply_config_flags(generate.get_args(), _model_config(ff_kwargs={"use_conv": True}))
    assert "allow_conv_ff" not in cfg["model"]["diffusion"]["config"]
    monkeypatch.setattr(sys, "argv", base + ["--allow-conv-ff"])
    cfg = generate.apply_config_flags(generate.get_args(), _model_config(ff_kwargs={"use_conv": True}))
    assert cfg["model"]["diffusion"]["config"]["allow_conv_ff"] is True
    with _init.skip_init():
        model = S.create_model_from_config(cfg)
    assert model.model.model.transformer.ff_conv_kernel == 3
    # a pretrained model is built from its own config, which the flag never reaches: refused when the arguments are read
    monkeypatch.setattr(sys, "argv", base + ["--allow-conv-ff", "--model-name", "some/model"])
    with pytest.raises(SystemExit):
        generate.get_args()


@pytest.mark.parametrize("name", list(CC.CONFIGS))
def test_state_dict_keys_and_shapes_are_the_references(name):
    m, got = check_state_dict_keys(CC.FAMILY, name)
    k = CC.CONFIGS[name]["ff_kwargs"].get("conv_kernel_size", 3)
    assert m.transformer.ff_conv_kernel == k and got["transformer.layers.0.ff.ff.2.weight"][2] == k
    # the gain touches the off-centre taps of FF-out only, and centre_taps_only zeroes them in both convolutions
    sd = CC.synth_weights(m.state_dict(), 0)
    centre = CC.centre_taps_only(sd)
    for key, v in sd.items():
        if CC.is_ff_conv_weight(key, v):
            off = [j for j in range(k) if j != k // 2]
            assert torch.equal(centre[key][:, :, k // 2], v[:, :, k // 2]) and not bool(centre[key][:, :, off].any()) and bool(v[:, :, off].any())
        else:
            assert torch.equal(centre[key], v)


# ------------------------------------------------------------------------------------------------------------------------- refusals
def test_kernel_sizes():
    for k in (1, 3, 5, 7):
        assert _build(**dict(cases.SMALL_DIT, ff_kwargs=dict(use_conv=True, conv_kernel_size=k)), **CC.PRODUCT_KWARGS).transformer.ff_conv_kernel == k
    for k in (2, 4, 0):
        with pytest.raises(ValueError, match="even kernel size"):          # the reference's own forward fails there
            _build(**dict(cases.SMALL_DIT, ff_kwargs=dict(use_conv=True, conv_kernel_size=k)), **CC.PRODUCT_KWARGS)
    with pytest.raises(NotImplementedError, match="conv_kernel_size=9"):
        _build(**dict(cases.SMALL_DIT, ff_kwargs=dict(use_conv=True, conv_kernel_size=9)), **CC.PRODUCT_KWARGS)


def test_inner_dim_rules_stay():
    with pytest.raises(NotImplementedError, match="multiple of 64"):
        _build(**dict(cases.SMALL_DIT, ff_kwargs=dict(use_conv=True, mult=0.3)), **CC.PRODUCT_KWARGS)
    with pytest.raises(NotImplementedError, match="multiple of 128"):
        _build(**dict(cases.SMALL_DIT, ff_kwargs=dict(use_conv=True, glu=False, mult=0.75)), **CC.PRODUCT_KWARGS)


def test_dim_heads_128_raises():
    with pytest.raises(NotImplementedError, match="dim_heads"):
        _build(**dict(cases.SMALL_DIT, num_heads=2, ff_kwargs=dict(use_conv=True)), **CC.PRODUCT_KWARGS)


@pytest.mark.parametrize("dtype", ["fp8", "fp8-all"])
@pytest.mark.parametrize("name", ["conv", "conv_silu"])
def test_fp8_raises(name, dtype):
    m = _build(**CC.CONFIGS[name], **CC.PRODUCT_KWARGS)
    with pytest.raises(NotImplementedError, match="gemm_dtype"):
        m.set_gemm_dtype(dtype)
    for ok in ("fp16", "bf16", "fp32x"):
        m.set_gemm_dtype(ok)
    m.set_layernorm_fusion(False).set_layernorm_fusion(True)


def test_range_report_raises():
    m = _build(**CC.CONFIGS["conv"], **CC.PRODUCT_KWARGS)
    with pytest.raises(NotImplementedError, match="activation_range_report"):
        m.activation_range_report(True)


def test_ff_conv_entry_point_validates_without_gpu():
    from stable_audio_tools import _hip
    lib = _hip.lib()
    O = _hip.SatDitFfConvOptions
    size = ctypes.sizeof(O)
    assert size == 4 and ctypes.sizeof(_hip.SatDitBlockOptions) == 12          # a call of its own: the block options did not grow
    plan = ctypes.c_void_p()
    cfg = _hip.SatDitCfg(64, 256, 2, 4, 128, 128, 96, 128)
    assert lib.sat_dit_plan_create(ctypes.byref(cfg), ctypes.byref(plan)) == 0
    try:
        ok = O(3)
        assert lib.sat_dit_plan_set_ff_conv(None, ctypes.byref(ok), size) == -1
        assert lib.sat_dit_plan_set_ff_conv(plan, None, size) == -1
        for wrong in (0, 8, 12):          # wrong size: SAT_E_INVALID
            assert lib.sat_dit_plan_set_ff_conv(plan, ctypes.byref(ok), wrong) == -1 and b"bytes" in lib.sat_last_error()
        for bad in (0, -3):
            assert lib.sat_dit_plan_set_ff_conv(plan, ctypes.byref(O(bad)), size) == -1
        for even in (2, 4, 6):            # SAT_E_UNSUPPORTED, with the reason
            assert lib.sat_dit_plan_set_ff_conv(plan, ctypes.byref(O(even)), size) == -2 and b"even" in lib.sat_last_error()
        for large in (9, 11):
            assert lib.sat_dit_plan_set_ff_conv(plan, ctypes.byref(O(large)), size) == -2 and b"1, 3, 5 and 7" in lib.sat_last_error()
        for good in (1, 3, 5, 7):
            assert lib.sat_dit_plan_set_ff_conv(plan, ctypes.byref(O(good)), size) == 0, lib.sat_last_error()
    finally:
        lib.sat_dit_plan_destroy(plan)
    # e4m3 operands and 128-channel heads: SAT_E_UNSUPPORTED above kernel size 1
    for cfg, word in ((_hip.SatDitCfg(64, 256, 2, 4, 128, 128, 96, 128, 0, 1), b"fp8"), (_hip.SatDitCfg(64, 256, 2, 2, 128, 128, 96, 128), b"dim_heads")):
        assert lib.sat_dit_plan_create(ctypes.byref(cfg), ctypes.byref(plan)) == 0
        try:
            for k in (3, 5, 7):
                assert lib.sat_dit_plan_set_ff_conv(plan, ctypes.byref(O(k)), size) == -2 and word in lib.sat_last_error()
            assert lib.sat_dit_plan_set_ff_conv(plan, ctypes.byref(O(1)), size) == 0
        finally:
            lib.sat_dit_plan_destroy(plan)
    assert lib.sat_version() == 6


def test_finalize_names_a_missing_conv_tensor():
    """The Conv1d weights are checked by name and size before anything is allocated: no device needed."""
    from stable_audio_tools import _hip
    lib = _hip.lib()
    plan = ctypes.c_void_p()
    cfg = _hip.SatDitCfg(64, 256, 2, 4, 128, 128, 96, 128)
    fake = ctypes.c_void_p(0x1000)
    D, inner = 256, 1024
    assert lib.sat_dit_plan_create(ctypes.byref(cfg), ctypes.byref(plan)) == 0
    try:
        o = _hip.SatDitFfConvOptions(3)
        assert lib.sat_dit_plan_set_ff_conv(plan, ctypes.byref(o), ctypes.sizeof(o)) == 0
        assert lib.sat_dit_plan_set_tensor(plan, b"transformer.layers.0.ff.ff.0.proj.weight", fake, 2 * inner * D) == 0
        assert lib.sat_dit_plan_set_tensor(plan, b"transformer.layers.0.ff.ff.2.weight", fake, D * inner * 3) == 0
        assert lib.sat_dit_plan_finalize(plan, None) == -3          # SAT_E_MISSING
        assert b"'transformer.layers.1.ff.ff.2.weight' was never set" in lib.sat_last_error()
        assert lib.sat_dit_plan_set_tensor(plan, b"transformer.layers.1.ff.ff.2.weight", fake, D * inner) == 0          # a Linear's weight
        assert lib.sat_dit_plan_finalize(plan, None) == -1 and b"Conv1d(1024, 256, 3)" in lib.sat_last_error()
    finally:
        lib.sat_dit_plan_destroy(plan)


# --------------------------------------------------------------------------------------------------------------------- restatements
@pytest.mark.parametrize("b, s, k", [(2, 78, 3), (4, 78, 3), (3, 1, 5), (3, 2, 5), (1, 300, 7), (2, 5, 1)])
@pytest.mark.parametrize("bias", [True, False])
def test_restatement_is_conv1d(b, s, k, bias):
    gen = torch.Generator().manual_seed(100 * b + s + k)
    a = torch.randn((b, s, 32), generator=gen, dtype=torch.float64)
    w = torch.randn((48, 32, k), generator=gen, dtype=torch.float64)
    bv = torch.randn((48,), generator=gen, dtype=torch.float64) if bias else None
    got, want = cu.conv_gemm(a, w, bv), cu.conv1d_reference(a, w, bv)
    assert got.shape == (b * s, 48)
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    # tap-major: column j * K + c of the packed weight is w[:, c, j]
    p = cu.pack_taps(w)
    for j in range(k):
        assert torch.equal(p[:, j * 32:(j + 1) * 32], w[:, :, j])


# ------------------------------------------------------------------------------------------------------ the gates see these faults
def _fault_case():
    gen = torch.Generator().manual_seed(7)
    b, s, kk, n, k = 3, 78, 128, 128, 3
    a = bf16_round(torch.randn((b, s, kk), generator=gen) * (10.0 ** torch.arange(b, dtype=torch.float32))[:, None, None])
    w = bf16_round(torch.randn((n, kk, k), generator=gen) * 0.05 + torch.linspace(-0.02, 0.03, k)[None, None, :])
    return a, w, cu.conv_gemm(a, w).float()


def _shift_rows(x, by):
    out = torch.zeros_like(x)
    out[by:] = x[:-by]
    return out


FAULTS = {
    "a dropped tap": lambda a, w: cu.conv_gemm(a, w * torch.tensor([1.0, 1.0, 0.0], dtype=w.dtype)),
    "taps in reversed order": lambda a, w: cu.conv_gemm(a, w, order=[2, 1, 0]),
    "a window that leaks one row from the neighbouring sequence": lambda a, w: cu.conv_gemm(a, w, leak=True),
    "a non-zero guard row": lambda a, w: cu.conv_gemm(a, w, guard=1.0),
    "an output row written one row off": lambda a, w: _shift_rows(cu.conv_gemm(a, w), 1),
}


def test_the_gate_passes_the_correct_result():
    a, w, want = _fault_case()
    assert_close_rows_blocks("correct, fp32 evaluation", cu.conv_gemm(a, w, dt=torch.float32), want, 1e-5)


@pytest.mark.parametrize("fault", list(FAULTS))
def test_the_gate_rejects(fault):
    """At the loosest tolerance the GPU test uses on this output (1e-3, bf16 operands into fp32)."""
    a, w, want = _fault_case()
    got = FAULTS[fault](a, w).float()
    with pytest.raises(AssertionError, match="slice"):
        assert_close_rows_blocks(fault, got, want, 1e-3)


def test_one_leaked_row_alone_is_rejected():
    """Only the first row of the last sequence reads its neighbour: one row in 234 is wrong, and the per-row gate still sees it."""
    a, w, want = _fault_case()
    got = want.clone()
    leaked = cu.conv_gemm(a, w, leak=True).float()
    got[2 * 78] = leaked[2 * 78]
    assert not torch.equal(got, want)
    with pytest.raises(AssertionError, match="slice"):
        assert_close_rows_blocks("one leaked row", got, want, 1e-3)
