"""qk_norm, the sinusoidal / absolute position embeddings, rotary_pos_emb=False and bias-free feed-forwards of the DiT (reference
models/transformer.py:50-96, 244-276, 298, 433-436, 718-746), host side: the modules hold the reference's parameter names and shapes,
the options that stay outside the HIP path still raise with a reason, and sat_dit_plan_set_transformer_options checks its arguments.
(Its SAT_E_STATE answer after finalize needs a finalized plan, i.e. a device: tests/test_gpu_dit_options.py.)"""
import ctypes
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import cases  # noqa: E402
import dit_options_cases as OC  # noqa: E402
from dit_family_host import build as _build, check_state_dict_keys  # noqa: E402


@pytest.mark.parametrize("name", sorted(OC.CONFIGS))
def test_dit_state_dict_matches_reference(name):
    check_state_dict_keys(OC.FAMILY, name)


def test_option_keys_that_come_and_go():
    sd = {name: set(_build(**cfg).state_dict()) for name, cfg in OC.CONFIGS.items()}
    plain = set(_build(**cases.SMALL_DIT).state_dict())
    assert sd["qk"] == plain                                                    # qk_norm has no parameters
    assert sd["sin"] - plain == {"transformer.pos_emb.scale"}                   # inv_freq is not persistent in the reference
    assert "transformer.pos_emb.emb.weight" in sd["abs"] and "transformer.rotary_pos_emb.inv_freq" in sd["abs"]
    assert "transformer.rotary_pos_emb.inv_freq" not in sd["abs_norope"]
    assert plain - sd["nobias"] == {f"transformer.layers.{i}.ff.ff.2.bias" for i in range(3)}      # the GLU projection keeps its bias
    assert all(f"transformer.layers.{i}.ff.ff.0.proj.bias" in sd["nobias"] for i in range(3))


def test_transformer_options_of_the_module():
    from stable_audio_tools import _hip
    assert _build(**cases.SMALL_DIT).transformer_options() == (0, _hip.DIT_POS_NONE, 0, 1)
    assert _build(**OC.CONFIGS["qk"]).transformer_options() == (1, _hip.DIT_POS_NONE, 0, 1)
    assert _build(**OC.CONFIGS["sin"]).transformer_options() == (0, _hip.DIT_POS_SINUSOIDAL, 0, 1)
    assert _build(**OC.CONFIGS["abs_norope"]).transformer_options() == (0, _hip.DIT_POS_ABSOLUTE, 256, 0)
    assert _build(**OC.CONFIGS["all"]).transformer_options() == (1, _hip.DIT_POS_SINUSOIDAL, 0, 1)


def test_ff_mult_follows_the_inner_dim_rule():
    m = _build(**dict(cases.SMALL_DIT, ff_kwargs={"mult": 2}))
    assert tuple(m.transformer.layers[0].ff.ff[0].proj.weight.shape) == (2 * 512, 256)
    with pytest.raises(NotImplementedError, match="multiple of 64"):
        _build(**dict(cases.SMALL_DIT, ff_kwargs={"mult": 0.3}))      # inner dim 76


@pytest.mark.parametrize("kwargs, match", [
    (dict(attn_kwargs={"natten_kernel_size": 7}), "natten_kernel_size"),
    (dict(causal=True), "causal"),
    (dict(conformer=True), "conformer"),
    (dict(remove_norms=True), "remove_norms"),
    (dict(ff_kwargs={"glu": False}), "glu"),
    (dict(ff_kwargs={"use_conv": True}), "use_conv"),
    (dict(num_heads=8), "dim_heads"),            # 256 / 8 = 32 channels per head
    (dict(patch_size=2), "patch_size"),
])
def test_refused_options_still_raise(kwargs, match):
    with pytest.raises(NotImplementedError, match=match):
        _build(**dict(cases.SMALL_DIT, **kwargs))


def test_both_position_embeddings_is_the_reference_assertion():
    with pytest.raises(AssertionError, match="sinusoidal/abs"):
        _build(**dict(cases.SMALL_DIT, use_sinusoidal_emb=True, use_abs_pos_emb=True))


@pytest.mark.parametrize("dtype", ["fp8", "fp8-all"])
def test_fp8_with_qk_norm_raises(dtype):
    m = _build(**OC.CONFIGS["qk"])
    with pytest.raises(NotImplementedError, match=r"qk_norm.*gemm_dtype"):
        m.set_gemm_dtype(dtype)
    _build(**OC.CONFIGS["sin"]).set_gemm_dtype(dtype)          # the position embeddings do not care


def test_transformer_options_entry_point_validates_without_gpu():
    from stable_audio_tools import _hip
    lib = _hip.lib()
    O = _hip.SatDitTransformerOptions
    size = ctypes.sizeof(O)
    assert size == 16
    plan = ctypes.c_void_p()
    cfg = _hip.SatDitCfg(64, 256, 2, 4, 128, 128, 96, 128)
    assert lib.sat_dit_plan_create(ctypes.byref(cfg), ctypes.byref(plan)) == 0
    try:
        ok = O(1, _hip.DIT_POS_ABSOLUTE, 256, 0)
        assert lib.sat_dit_plan_set_transformer_options(None, ctypes.byref(ok), size) == -1
        assert lib.sat_dit_plan_set_transformer_options(plan, None, size) == -1
        for wrong in (0, 12, 20):          # wrong size: SAT_E_INVALID
            assert lib.sat_dit_plan_set_transformer_options(plan, ctypes.byref(ok), wrong) == -1 and b"bytes" in lib.sat_last_error()
        for bad in (O(2, 0, 0, 1), O(-1, 0, 0, 1), O(0, 3, 0, 1), O(0, -1, 0, 1), O(0, 0, 0, 2)):      # unknown value: SAT_E_UNSUPPORTED
            assert lib.sat_dit_plan_set_transformer_options(plan, ctypes.byref(bad), size) == -2, tuple(getattr(bad, f) for f, _ in O._fields_)
            assert b"unknown value" in lib.sat_last_error()
        for bad in (O(0, _hip.DIT_POS_ABSOLUTE, 0, 1), O(0, _hip.DIT_POS_ABSOLUTE, -4, 1)):
            assert lib.sat_dit_plan_set_transformer_options(plan, ctypes.byref(bad), size) == -1 and b"abs_pos_max_len" in lib.sat_last_error()
        for good in (ok, O(0, 0, 0, 1), O(1, _hip.DIT_POS_SINUSOIDAL, 0, 1), O(0, _hip.DIT_POS_NONE, 77, 1)):
            assert lib.sat_dit_plan_set_transformer_options(plan, ctypes.byref(good), size) == 0, lib.sat_last_error()
    finally:
        lib.sat_dit_plan_destroy(plan)
    # e4m3 operands + qk_norm: SAT_E_UNSUPPORTED; the other options go with every operand format
    cfg = _hip.SatDitCfg(64, 256, 2, 4, 128, 128, 96, 128, 0, 1)
    assert lib.sat_dit_plan_create(ctypes.byref(cfg), ctypes.byref(plan)) == 0
    try:
        qk = O(1, 0, 0, 1)
        assert lib.sat_dit_plan_set_transformer_options(plan, ctypes.byref(qk), size) == -2 and b"qk_norm" in lib.sat_last_error()
        sin = O(0, _hip.DIT_POS_SINUSOIDAL, 0, 0)
        assert lib.sat_dit_plan_set_transformer_options(plan, ctypes.byref(sin), size) == 0
    finally:
        lib.sat_dit_plan_destroy(plan)
    assert lib.sat_version() == 6
