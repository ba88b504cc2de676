"""conformer, remove_norms and ff_kwargs glu=False of the DiT (reference models/transformer.py:557-591, 621-645, 259-268), host side: the
modules hold the reference's parameter names and shapes, the options come in through the allow_block_options opt-in only (which the config
factory passes), the combinations outside the HIP path raise with a reason, and sat_dit_plan_set_block_options checks its arguments.
(Its SAT_E_STATE answer after finalize needs a finalized plan, i.e. a device: tests/test_gpu_dit_block_options.py.)"""
import ctypes
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import cases  # noqa: E402
import dit_block_options_cases as BC  # noqa: E402
from dit_family_host import build as _build, check_state_dict_keys, model_config as _model_config  # noqa: E402

OPTIONS = [dict(conformer=True), dict(remove_norms=True), dict(ff_kwargs={"glu": False})]


@pytest.mark.parametrize("name", sorted(BC.CONFIGS))
def test_dit_state_dict_matches_reference(name):
    check_state_dict_keys(BC.FAMILY, name)


def test_option_keys_that_come_and_go():
    sd = {name: {k: tuple(v.shape) for k, v in _build(**cfg, **BC.PRODUCT_KWARGS).state_dict().items()} for name, cfg in BC.CONFIGS.items()}
    plain = {k: tuple(v.shape) for k, v in _build(**cases.SMALL_DIT).state_dict().items()}
    layer = lambda i, rest: f"transformer.layers.{i}.{rest}"
    D = 256
    conformer = {"in_norm.gamma": (D,), "in_norm.beta": (D,), "pointwise_conv.weight": (D, D, 1), "glu.proj.weight": (2 * D, D), "glu.proj.bias": (2 * D,),
                 "depthwise_conv.weight": (D, 1, 17), "mid_norm.gamma": (D,), "mid_norm.beta": (D,), "pointwise_conv_2.weight": (D, D, 1)}
    want = dict(plain, **{layer(i, "conformer." + k): v for i in range(3) for k, v in conformer.items()})
    assert sd["conf"] == want and sd["conf_qk"] == want
    # remove_norms: the three norms of every block are nn.Identity, nothing else changes; the conformer keeps its two
    norms = {layer(i, f"{n}.{p}") for i in range(3) for n in ("pre_norm", "cross_attend_norm", "ff_norm") for p in ("gamma", "beta")}
    assert set(plain) - set(sd["nonorm"]) == norms and set(sd["nonorm"]) <= set(plain)
    assert set(sd["conf"]) - set(sd["all3"]) >= norms and all(layer(i, "conformer.mid_norm.gamma") in sd["all3"] for i in range(3))
    # glu=False: ff.ff.0 is Sequential(Identity, Linear, Identity, SiLU); no_bias drops both biases
    gone = {layer(i, f"ff.ff.0.proj.{p}") for i in range(3) for p in ("weight", "bias")}
    come = {layer(i, f"ff.ff.0.1.{p}") for i in range(3) for p in ("weight", "bias")}
    assert set(plain) - set(sd["silu"]) == gone and set(sd["silu"]) - set(plain) == come
    assert sd["silu"][layer(0, "ff.ff.0.1.weight")] == (4 * D, D) and sd["silu"][layer(0, "ff.ff.0.1.bias")] == (4 * D,)
    assert sd["silu_mult2"][layer(0, "ff.ff.0.1.weight")] == (2 * D, D) and sd["silu_mult2"][layer(0, "ff.ff.2.weight")] == (D, 2 * D)
    assert set(sd["silu"]) - set(sd["silu_nobias"]) == {layer(i, f"ff.ff.{j}.bias") for i in range(3) for j in ("0.1", "2")}


def test_block_options_of_the_module():
    assert _build(**cases.SMALL_DIT).transformer.block_options == (0, 0, 1)
    assert _build(**BC.CONFIGS["conf"], **BC.PRODUCT_KWARGS).transformer.block_options == (1, 0, 1)
    assert _build(**BC.CONFIGS["nonorm_adaln"], **BC.PRODUCT_KWARGS).transformer.block_options == (0, 1, 1)
    assert _build(**BC.CONFIGS["silu_nobias"], **BC.PRODUCT_KWARGS).transformer.block_options == (0, 0, 0)
    m = _build(**BC.CONFIGS["all3"], **BC.PRODUCT_KWARGS)
    assert m.transformer.block_options == (1, 1, 0)
    blk = m.transformer.layers[1]
    assert type(blk.pre_norm).__name__ == "Identity" and type(blk.ff_norm).__name__ == "Identity" and type(blk.cross_attend_norm).__name__ == "Identity"
    assert type(blk.conformer).__name__ == "ConformerModule" and _build(**cases.SMALL_DIT).transformer.layers[1].conformer is None


@pytest.mark.parametrize("kwargs, match", [(OPTIONS[0], "conformer"), (OPTIONS[1], "remove_norms"), (OPTIONS[2], "glu")])
def test_the_options_need_the_opt_in(kwargs, match):
    for allow in ({}, dict(allow_block_options=False)):
        with pytest.raises(NotImplementedError, match=match) as e:
            _build(**dict(cases.SMALL_DIT, **kwargs), **allow)
        assert "allow_block_options" in str(e.value)
    _build(**dict(cases.SMALL_DIT, **kwargs), allow_block_options=True)


@pytest.mark.parametrize("allow", [False, True])
def test_use_conv_raises_on_both_paths(allow):
    with pytest.raises(NotImplementedError, match="use_conv") as e:
        _build(**dict(cases.SMALL_DIT, ff_kwargs={"use_conv": True}), allow_block_options=allow)
    assert "allow_block_options" in str(e.value)
    with pytest.raises(NotImplementedError, match="use_conv"):
        _build(**dict(cases.SMALL_DIT, ff_kwargs={"use_conv": True, "glu": False}), allow_block_options=allow)


@pytest.mark.parametrize("kwargs", OPTIONS + [dict(conformer=True, remove_norms=True, ff_kwargs={"glu": False, "no_bias": True})])
def test_the_config_factory_passes_the_opt_in(kwargs):
    import stable_audio_tools as S
    from stable_audio_tools.models import _init
    with _init.skip_init():
        model = S.create_model_from_config(_model_config(**kwargs))
    tr = model.model.model.transformer
    assert tr.block_options == (1 if kwargs.get("conformer") else 0, 1 if kwargs.get("remove_norms") else 0, 0 if "ff_kwargs" in kwargs else 1)
    with _init.skip_init(), pytest.raises(NotImplementedError, match="use_conv"):
        S.create_model_from_config(_model_config(ff_kwargs={"use_conv": True}))


@pytest.mark.parametrize("kwargs", OPTIONS)
def test_dim_heads_128_raises_with_each_option(kwargs):
    with pytest.raises(NotImplementedError, match="dim_heads"):
        _build(**dict(cases.SMALL_DIT, num_heads=2, **kwargs), allow_block_options=True)
    _build(**dict(cases.SMALL_DIT, num_heads=2))          # 128-channel heads alone are fine


@pytest.mark.parametrize("dtype", ["fp8", "fp8-all"])
@pytest.mark.parametrize("name", ["conf", "nonorm", "silu"])
def test_fp8_raises_with_each_option(name, dtype):
    m = _build(**BC.CONFIGS[name], **BC.PRODUCT_KWARGS)
    with pytest.raises(NotImplementedError, match="gemm_dtype"):
        m.set_gemm_dtype(dtype)
    for ok in ("fp16", "bf16", "fp32x"):
        m.set_gemm_dtype(ok)
    m.set_layernorm_fusion(False).set_layernorm_fusion(True)          # accepted with remove_norms as well


def test_range_report_raises_with_the_options():
    m = _build(**BC.CONFIGS["conf"], **BC.PRODUCT_KWARGS)
    with pytest.raises(NotImplementedError, match="activation_range_report"):
        m.activation_range_report(True)


def test_glu_false_inner_dim_rule():
    with pytest.raises(NotImplementedError, match="multiple of 64"):
        _build(**dict(cases.SMALL_DIT, ff_kwargs={"glu": False, "mult": 0.3}), allow_block_options=True)
    with pytest.raises(NotImplementedError, match="multiple of 128"):
        _build(**dict(cases.SMALL_DIT, ff_kwargs={"glu": False, "mult": 0.75}), allow_block_options=True)          # inner dim 192


def test_block_options_entry_point_validates_without_gpu():
    from stable_audio_tools import _hip
    lib = _hip.lib()
    O = _hip.SatDitBlockOptions
    size = ctypes.sizeof(O)
    assert size == 12 and ctypes.sizeof(_hip.SatDitTransformerOptions) == 16
    plan = ctypes.c_void_p()
    cfg = _hip.SatDitCfg(64, 256, 2, 4, 128, 128, 96, 128)
    assert lib.sat_dit_plan_create(ctypes.byref(cfg), ctypes.byref(plan)) == 0
    try:
        ok = O(1, 1, 0)
        assert lib.sat_dit_plan_set_block_options(None, ctypes.byref(ok), size) == -1
        assert lib.sat_dit_plan_set_block_options(plan, None, size) == -1
        for wrong in (0, 8, 16):          # wrong size: SAT_E_INVALID
            assert lib.sat_dit_plan_set_block_options(plan, ctypes.byref(ok), wrong) == -1 and b"bytes" in lib.sat_last_error()
        for bad in (O(2, 0, 1), O(-1, 0, 1), O(0, 2, 1), O(0, 0, 2), O(0, 0, -1)):      # unknown value: SAT_E_UNSUPPORTED
            assert lib.sat_dit_plan_set_block_options(plan, ctypes.byref(bad), size) == -2, tuple(getattr(bad, f) for f, _ in O._fields_)
            assert b"unknown value" in lib.sat_last_error()
        for good in (ok, O(0, 0, 1), O(1, 0, 1), O(0, 1, 1), O(0, 0, 0)):
            assert lib.sat_dit_plan_set_block_options(plan, ctypes.byref(good), size) == 0, lib.sat_last_error()
    finally:
        lib.sat_dit_plan_destroy(plan)
    # e4m3 operands and 128-channel heads: SAT_E_UNSUPPORTED with any of the three, the defaults pass
    for cfg, word in ((_hip.SatDitCfg(64, 256, 2, 4, 128, 128, 96, 128, 0, 1), b"fp8"), (_hip.SatDitCfg(64, 256, 2, 2, 128, 128, 96, 128), b"dim_heads")):
        assert lib.sat_dit_plan_create(ctypes.byref(cfg), ctypes.byref(plan)) == 0
        try:
            for o in (O(1, 0, 1), O(0, 1, 1), O(0, 0, 0)):
                assert lib.sat_dit_plan_set_block_options(plan, ctypes.byref(o), size) == -2 and word in lib.sat_last_error()
            assert lib.sat_dit_plan_set_block_options(plan, ctypes.byref(O(0, 0, 1)), size) == 0
        finally:
            lib.sat_dit_plan_destroy(plan)
    assert lib.sat_version() == 6


def test_finalize_names_a_missing_block_option_tensor():
    """The tensors the options add are checked by name before anything is allocated: no device needed.  (set_tensor keeps the pointer and
    does not read it.)"""
    from stable_audio_tools import _hip
    lib = _hip.lib()
    plan = ctypes.c_void_p()
    cfg = _hip.SatDitCfg(64, 256, 2, 4, 128, 128, 96, 128)
    fake = ctypes.c_void_p(0x1000)
    D = 256

    def fresh(options):
        assert lib.sat_dit_plan_create(ctypes.byref(cfg), ctypes.byref(plan)) == 0
        assert lib.sat_dit_plan_set_block_options(plan, ctypes.byref(options), ctypes.sizeof(options)) == 0

    conformer = {"in_norm.gamma": D, "in_norm.beta": D, "pointwise_conv.weight": D * D, "glu.proj.weight": 2 * D * D, "glu.proj.bias": 2 * D,
                 "depthwise_conv.weight": D * 17, "mid_norm.gamma": D, "mid_norm.beta": D, "pointwise_conv_2.weight": D * D}
    fresh(_hip.SatDitBlockOptions(1, 0, 1))
    try:
        assert lib.sat_dit_plan_set_tensor(plan, b"transformer.layers.0.ff.ff.0.proj.weight", fake, 2 * 1024 * D) == 0
        for l in range(2):
            for k, n in conformer.items():
                if (l, k) != (1, "depthwise_conv.weight"):
                    assert lib.sat_dit_plan_set_tensor(plan, f"transformer.layers.{l}.conformer.{k}".encode(), fake, n) == 0
        assert lib.sat_dit_plan_finalize(plan, None) == -3          # SAT_E_MISSING
        assert b"'transformer.layers.1.conformer.depthwise_conv.weight' was never set" in lib.sat_last_error()
    finally:
        lib.sat_dit_plan_destroy(plan)
    # ff_glu 0: the inner dim comes from ff.ff.0.1.weight, and ff.ff.0.proj.weight is not asked for
    fresh(_hip.SatDitBlockOptions(0, 0, 0))
    try:
        assert lib.sat_dit_plan_set_tensor(plan, b"transformer.layers.0.ff.ff.0.proj.weight", fake, 2 * 1024 * D) == 0
        assert lib.sat_dit_plan_finalize(plan, None) == -3
        assert b"'transformer.layers.0.ff.ff.0.1.weight' was never set" in lib.sat_last_error()
        assert lib.sat_dit_plan_set_tensor(plan, b"transformer.layers.0.ff.ff.0.1.weight", fake, 192 * D) == 0
        assert lib.sat_dit_plan_finalize(plan, None) == -2 and b"multiple of 128" in lib.sat_last_error()
    finally:
        lib.sat_dit_plan_destroy(plan)
