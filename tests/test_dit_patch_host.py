"""Patchified DiTs (patch_size > 1) without a GPU: the option needs its own opt-in (allow_patch_size, by keyword, by config key or by
generate.py --allow-patch-size), the modules hold the reference's parameter names and shapes, a latent length that holds no whole number
of patches is a ValueError before the library is touched, sat_dit_plan_set_patch checks its arguments, the float64 restatements of the two
boundary kernels (tests/dit_patch_units.py) are the reference's modules run in plain PyTorch, and the gates of tests/fp32_units.py reject the
faults these kernels can have."""
import ctypes
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import cases  # noqa: E402
import dit_patch_cases as PC  # noqa: E402
from dit_family_host import build as _build, check_state_dict_keys, model_config as _model_config  # noqa: E402
import dit_patch_units as pu  # noqa: E402
import fp32_units as fu  # noqa: E402


# ------------------------------------------------------------------------------------------------------------------- construction
@pytest.mark.parametrize("P", [2, 3, 8])
def test_patch_size_needs_allow_patch_size(P):
    for kw in (dict(), dict(allow_block_options=True, allow_conv_ff=True)):
        with pytest.raises(NotImplementedError, match="patch_size") as e:
            _build(**dict(cases.SMALL_DIT, patch_size=P), **kw)
        assert "allow_patch_size" in str(e.value)
    m = _build(**dict(cases.SMALL_DIT, patch_size=P), allow_patch_size=True)
    assert m.patch_size == P
    assert tuple(m.transformer.project_in.weight.shape) == (256, 64 * P) and tuple(m.transformer.project_out.weight.shape) == (64 * P, 256)
    assert tuple(m.preprocess_conv.weight.shape) == (64, 64, 1) and tuple(m.postprocess_conv.weight.shape) == (64, 64, 1)
    assert _build(**cases.SMALL_DIT, allow_patch_size=True).patch_size == 1          # the opt-in alone changes nothing


def test_limits_of_the_boundary_kernels():
    with pytest.raises(NotImplementedError, match="512"):
        _build(**dict(cases.SMALL_DIT, patch_size=9), allow_patch_size=True)          # 64 * 9 = 576 output columns
    with pytest.raises(NotImplementedError, match="1024"):
        _build(**dict(cases.SMALL_DIT, patch_size=8, input_concat_dim=68), allow_patch_size=True)
    with pytest.raises(ValueError, match="patch_size"):
        _build(**dict(cases.SMALL_DIT, patch_size=0), allow_patch_size=True)
    _build(**dict(cases.SMALL_DIT, patch_size=8, input_concat_dim=64), allow_patch_size=True)


def test_the_config_key_reaches_the_constructor():
    import stable_audio_tools as S
    from stable_audio_tools.models import _init
    from stable_audio_tools.models.diffusion import DiTWrapper
    with _init.skip_init(), pytest.raises(NotImplementedError, match="patch_size"):
        S.create_model_from_config(_model_config(patch_size=2))          # DiTWrapper does not default the opt-in
    with _init.skip_init(), pytest.raises(NotImplementedError, match="patch_size"):
        DiTWrapper(**dict(cases.SMALL_DIT, patch_size=2))
    with _init.skip_init():
        model = S.create_model_from_config(_model_config(patch_size=4, allow_patch_size=True))
    assert model.model.model.patch_size == 4
    # models/diffusion.py:627 of the reference: the shortest input is one token
    assert model.min_input_length == 4 * model.pretransform.downsampling_ratio
    with _init.skip_init():
        assert S.create_model_from_config(_model_config()).min_input_length == model.pretransform.downsampling_ratio


def test_generate_flag_sets_the_config_key(monkeypatch):
    import generate
    import stable_audio_tools as S
    from stable_audio_tools.models import _init
    base = ["generate.py", "--output-dir", "o", "--cond-yaml-path", "c"]
    monkeypatch.setattr(sys, "argv", base)
    cfg = generate.apply_config_flags(generate.get_args(), _model_config(patch_size=2))
    assert "allow_patch_size" not in cfg["model"]["diffusion"]["config"]
    monkeypatch.setattr(sys, "argv", base + ["--allow-patch-size"])
    cfg = generate.apply_config_flags(generate.get_args(), _model_config(patch_size=2))
    assert cfg["model"]["diffusion"]["config"]["allow_patch_size"] is True and "allow_conv_ff" not in cfg["model"]["diffusion"]["config"]
    with _init.skip_init():
        assert S.create_model_from_config(cfg).model.model.patch_size == 2
    # a pretrained model is built from its own config, which the flag never reaches: refused when the arguments are read
    monkeypatch.setattr(sys, "argv", base + ["--allow-patch-size", "--model-name", "some/model"])
    with pytest.raises(SystemExit):
        generate.get_args()


@pytest.mark.parametrize("name", list(PC.CONFIGS))
def test_state_dict_keys_and_shapes_are_the_references(name):
    m, got = check_state_dict_keys(PC.FAMILY, name)
    _build(**PC.CONFIGS[name], **PC.PRODUCT_KWARGS).load_state_dict({k: torch.zeros(shape) for k, shape in got.items()}, strict=True)          # a reference-shaped state dict
    cfg = PC.CONFIGS[name]
    P, c, ci = cfg["patch_size"], cfg["io_channels"], cfg["io_channels"] + cfg.get("input_concat_dim", 0)
    assert got["transformer.project_in.weight"] == [256, ci * P] and got["transformer.project_out.weight"] == [c * P, 256]
    assert got["preprocess_conv.weight"] == [ci, ci, 1] and got["postprocess_conv.weight"] == [c, c, 1]
    assert bool(m.preprocess_conv.weight.any()) and bool(m.postprocess_conv.weight.any())          # the synthetic convs are not zero


def test_every_mistake_changes_the_weights():
    m = _build(**PC.CONFIGS["p3"], **PC.PRODUCT_KWARGS)
    sd = PC.synth_weights("p3", m.state_dict(), 0)
    for what, f in PC.MISTAKES.items():
        wrong = f(sd, 3)
        changed = [k for k in sd if not torch.equal(sd[k], wrong[k])]
        assert len(changed) in (1, 2) and all(wrong[k].shape == sd[k].shape for k in sd), what
    w = sd["transformer.project_in.weight"]
    assert torch.equal(PC.in_columns_pc(sd, 3)["transformer.project_in.weight"][:, 1 * 3 + 2], w[:, 2 * 64 + 1])          # column c P + p <- p Ci + c


# ------------------------------------------------------------------------------------------------------- a bad T, without the library
def _no_library(monkeypatch):
    from stable_audio_tools import _hip

    def boom(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_hip, "lib", boom)


def test_bad_latent_length_is_a_value_error_before_the_library(monkeypatch):
    _no_library(monkeypatch)
    m = _build(**PC.CONFIGS["p2"], **PC.PRODUCT_KWARGS)
    x, t = torch.zeros(2, 64, 77), torch.zeros(2)
    with pytest.raises(ValueError, match=r"T = 77 is not a multiple of patch_size = 2"):
        m(x, t, cross_attn_cond=torch.zeros(2, 4, 128))
    with pytest.raises(ValueError, match=r"T = 77 is not a multiple of patch_size = 2"):
        m(x, t, cross_attn_cond=torch.zeros(2, 4, 128), cfg_scale=7.0)
    with pytest.raises(ValueError, match=r"T = 77 is not a multiple of patch_size = 2"):
        m._forward(x, t)
    with pytest.raises(ValueError, match=r"T = 77 is not a multiple of patch_size = 2"):
        m.denoise(x, 1.0)
    m3 = _build(**PC.CONFIGS["p3"], **PC.PRODUCT_KWARGS)
    with pytest.raises(ValueError, match=r"T = 64 is not a multiple of patch_size = 3"):
        m3.denoise(torch.zeros(1, 64, 64), 1.0)


def test_bad_sample_size_is_a_value_error_before_sampling(monkeypatch):
    import stable_audio_tools as S
    from stable_audio_tools.inference.generation import generate_diffusion_cond
    from stable_audio_tools.models import _init
    _no_library(monkeypatch)
    with _init.skip_init():
        model = S.create_model_from_config(_model_config(patch_size=2, allow_patch_size=True))
    ratio = model.pretransform.downsampling_ratio
    with pytest.raises(ValueError, match=r"T = 17 .*patch_size = 2"):
        generate_diffusion_cond(model, steps=2, conditioning=[{"prompt": "x", "seconds_start": 0, "seconds_total": 1}], sample_size=17 * ratio, device="cpu")
    with pytest.raises(ValueError, match=r"T = 17 .*patch_size = 2"):          # sample_size // ratio, as the generation rounds it
        generate_diffusion_cond(model, steps=2, conditioning=[{"prompt": "x", "seconds_start": 0, "seconds_total": 1}], sample_size=17 * ratio + 5, device="cpu")


def test_abs_pos_length_counts_tokens():
    m = _build(**dict(cases.SMALL_DIT, patch_size=2, use_abs_pos_emb=True, abs_pos_emb_max_length=40), **PC.PRODUCT_KWARGS)
    m._check_seq_len(78, 0)            # 1 + 39 rows
    with pytest.raises(AssertionError, match="sequence length of 41"):
        m._check_seq_len(80, 0)


# ------------------------------------------------------------------------------------------------------------------------ the C ABI
def test_patch_entry_point_validates_without_gpu():
    from stable_audio_tools import _hip
    lib = _hip.lib()
    O = _hip.SatDitPatchOptions
    size = ctypes.sizeof(O)
    assert size == 4 and ctypes.sizeof(_hip.SatDitBlockOptions) == 12 and ctypes.sizeof(_hip.SatDitFfConvOptions) == 4
    plan = ctypes.c_void_p()
    cfg = _hip.SatDitCfg(64, 256, 2, 4, 128, 128, 96, 128)
    assert lib.sat_dit_plan_create(ctypes.byref(cfg), ctypes.byref(plan)) == 0
    try:
        ok = O(2)
        assert lib.sat_dit_plan_set_patch(None, ctypes.byref(ok), size) == -1
        assert lib.sat_dit_plan_set_patch(plan, None, size) == -1
        for wrong in (0, 8, 12):          # wrong size: SAT_E_INVALID
            assert lib.sat_dit_plan_set_patch(plan, ctypes.byref(ok), wrong) == -1 and b"bytes" in lib.sat_last_error()
        for bad in (0, -3):
            assert lib.sat_dit_plan_set_patch(plan, ctypes.byref(O(bad)), size) == -1 and b"patch_size" in lib.sat_last_error()
        assert lib.sat_dit_plan_set_patch(plan, ctypes.byref(O(9)), size) == -2 and b"512" in lib.sat_last_error()          # 64 * 9 columns
        assert lib.sat_dit_plan_set_patch(plan, ctypes.byref(O(256)), size) == -2
        for good in (1, 2, 3, 4, 8, 1):
            assert lib.sat_dit_plan_set_patch(plan, ctypes.byref(O(good)), size) == 0, lib.sat_last_error()
        # (io_channels + input_concat_dim) * P <= 1024, whichever call comes second
        assert lib.sat_dit_plan_set_patch(plan, ctypes.byref(O(8)), size) == 0
        assert lib.sat_dit_plan_set_extra_conditioning(plan, 68, 0, 0) == -2 and b"1024" in lib.sat_last_error()
        assert lib.sat_dit_plan_set_extra_conditioning(plan, 64, 0, 0) == 0
        assert lib.sat_dit_plan_set_patch(plan, ctypes.byref(O(8)), size) == 0
        assert lib.sat_dit_plan_set_patch(plan, ctypes.byref(O(1)), size) == 0
        assert lib.sat_dit_plan_set_extra_conditioning(plan, 100, 0, 0) == 0
        assert lib.sat_dit_plan_set_patch(plan, ctypes.byref(O(8)), size) == -2 and b"1024" in lib.sat_last_error()
    finally:
        lib.sat_dit_plan_destroy(plan)
    assert lib.sat_version() == 6


def test_finalize_expects_the_patch_widths():
    """project_in is [D, Ci P]: a plan told P = 2 refuses the P = 1 weight by size, before anything is allocated."""
    from stable_audio_tools import _hip
    lib = _hip.lib()
    plan = ctypes.c_void_p()
    cfg = _hip.SatDitCfg(64, 256, 1, 4, 0, 0, 0, 128)
    fake = ctypes.c_void_p(0x1000)
    D, inner = 256, 1024
    assert lib.sat_dit_plan_create(ctypes.byref(cfg), ctypes.byref(plan)) == 0
    try:
        o = _hip.SatDitPatchOptions(2)
        assert lib.sat_dit_plan_set_patch(plan, ctypes.byref(o), ctypes.sizeof(o)) == 0
        assert lib.sat_dit_plan_set_tensor(plan, b"transformer.project_in.weight", fake, D * 64) == 0
        assert lib.sat_dit_plan_set_tensor(plan, b"transformer.layers.0.ff.ff.0.proj.weight", fake, 2 * inner * D) == 0
        rc = lib.sat_dit_plan_finalize(plan, None)
        assert rc != 0
    finally:
        lib.sat_dit_plan_destroy(plan)


# ------------------------------------------------------------------------------------------ the references of the kernel test
@pytest.mark.parametrize("p", pu.SHAPES, ids=pu.shape_id)
def test_references_are_the_modules_in_plain_pytorch(p):
    """fold + projection in float64 == cat / 1x1 conv / rearrange / Linear in fp32, within the kernels' gates four times over (headroom 0.25);
    the a-priori bound is checked against the float64 evaluation of the same modules (it is a statement about one contraction on given
    operands, and the fp32 pipeline rounds the conv's output in between)."""
    ci, co = pu.Case("input_proj", p), pu.Case("output_proj", p)
    for case, key, torch_fn in ((ci, "X", pu.torch_input), (co, "out", pu.torch_output)):
        want = pu.reference(case)
        got32, got64 = torch_fn(case, torch.float32), torch_fn(case, torch.float64)
        rows = lambda x: fu._as_rows(case, key, x)
        fu.assert_close_sliced(f"{case.name} fp32 modules per row", rows(got32), rows(want[key]), 0.25 * fu.TOL, (0,))
        fu.assert_close_sliced(f"{case.name} fp32 modules per 32x32 block", fu.blocks32(rows(got32)), fu.blocks32(rows(want[key])), 0.25 * fu.TOL, (0, 2))
        # (the folded weights the kernel is given are fp32 roundings of the float64 fold: a unit per term, inside the bound)
        share = fu.bound_share(got64, want[key], want[key + ":mag"], want[key + ":n"])
        assert float(share.max()) <= 1.0
    for kind in ("fold_in", "fold_out", "input_proj", "output_proj"):          # the fp32 evaluation of each restatement passes its own gates
        case = pu.Case(kind, p)
        got = {k: v for k, v in pu.reference(case, torch.float32).items() if ":" not in k}
        fu.check(case, got, want=pu.reference(case), headroom=0.25)


def _faults_for(case):
    d = case.dim
    if case.what == "input_proj":
        out = ["in_pc", "frame_off_by_one", "prepend_off_by_one"]
        if d["cc"]:
            out.append("xscale_on_concat" if d["xscale"] != 1.0 else None)
            if d["tc"] != d["t"]:
                out.append("concat_src_per_token")
        return [f for f in out if f]
    return ["out_pc", "frame_off_by_one", "prepend_off_by_one"]


@pytest.mark.parametrize("kind", ["input_proj", "output_proj"])
@pytest.mark.parametrize("p", [s for s in pu.SHAPES if s["t"] // s["P"] > 1], ids=pu.shape_id)
def test_the_gates_reject_the_faults(p, kind):
    case = pu.Case(kind, p)
    want = pu.reference(case)
    for fault in _faults_for(case):
        got = {k: v.float() for k, v in pu.reference(case, fault=fault).items() if ":" not in k}
        with pytest.raises(AssertionError):
            fu.check(case, got, want=want)


def test_the_gates_reject_a_scaled_concat_signal_and_a_per_token_source():
    """On a concat shape with xscale 0.37 (what the fused denoise step passes as c_in)."""
    p = dict(bf=2, c=64, cc=8, P=2, t=78, d=256, pl=3, tc=26, xscale=0.37)
    case = pu.Case("input_proj", p)
    want = pu.reference(case)
    assert sorted(_faults_for(case)) == sorted(["in_pc", "frame_off_by_one", "prepend_off_by_one", "xscale_on_concat", "concat_src_per_token"])
    # the source frame per frame differs from the one per token on some frames of this shape, or the fault would be invisible
    src = fu.nearest_src(26, 78)
    assert bool((src != src[(torch.arange(78) // 2) * 2]).any())
    for fault in ("xscale_on_concat", "concat_src_per_token"):
        got = {k: v.float() for k, v in pu.reference(case, fault=fault).items() if ":" not in k}
        with pytest.raises(AssertionError):
            fu.check(case, got, want=want)
    fu.check(case, {k: v.float() for k, v in pu.reference(case, torch.float32).items() if ":" not in k}, want=want, headroom=0.25)
