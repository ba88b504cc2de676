"""The fp16 range reports (sat_dit_range_report, sat_oobleck_range_report, stable_audio_tools/inference/preflight.py) as far as they go
without a device: the entry points' argument validation on the real library, the record layout and slot names, the codec's record names
against the module tree, the Python lifecycle (flag on the module, re-applied on a plan rebuild, off after a failed read) against the
recording stand-in of tests/test_plan_lifecycle.py, and the verdict of check_fp16_range on canned tables.  The kernel and the numbers:
tests/test_gpu_range_report.py."""
import ctypes
import math

import pytest
import torch

from golden import cases
from test_plan_lifecycle import FakeLib

ISSUE_SLOTS = {"a_qkv", "a_cross_q", "a_ff", "q", "k", "v", "attn_out", "cross_attn_out", "cross_q", "ff_hidden", "cross_k", "cross_v"}


def _records(n):
    from stable_audio_tools import _hip
    return (_hip.SatRangeRecord * n)()


def _dit_plan(lib, gemm_dtype, fp8_families=0):
    from stable_audio_tools import _hip
    cfg = _hip.SatDitCfg(64, 256, 2, 4, 128, 128, 64, 128, 0, gemm_dtype, fp8_families, 1, 0, 0)
    plan = ctypes.c_void_p()
    assert lib.sat_dit_plan_create(ctypes.byref(cfg), ctypes.byref(plan)) == 0, lib.sat_last_error()
    return plan


def test_record_layout_and_slot_names():
    from stable_audio_tools import _hip
    lib = _hip.lib()
    assert ctypes.sizeof(_hip.SatRangeRecord) == 32
    assert [(f, getattr(_hip.SatRangeRecord, f).offset) for f, _ in _hip.SatRangeRecord._fields_] == [
        ("max_abs", 0), ("launches", 4), ("over_fp16", 8), ("nonfinite", 16), ("elements", 24)]
    names = [lib.sat_dit_range_slot_name(i) for i in range(_hip.DIT_RANGE_SLOTS)]
    assert _hip.DIT_RANGE_SLOTS == 12 and all(n is not None for n in names)
    names = tuple(n.decode() for n in names)
    assert names == _hip.DIT_RANGE_SLOT_NAMES and set(names) == ISSUE_SLOTS and len(set(names)) == 12
    assert lib.sat_dit_range_slot_name(12) is None and lib.sat_dit_range_slot_name(-1) is None


def test_dit_entry_points_validate_without_a_device():
    from stable_audio_tools import _hip
    lib = _hip.lib()
    buf = _records(24)
    assert lib.sat_dit_range_report(None, 1) == -1
    assert lib.sat_dit_range_report_read(None, buf, 24, 32, None) == -1
    plan = _dit_plan(lib, 3)            # fp16, depth 2: 24 records
    try:
        assert lib.sat_dit_range_report_read(plan, buf, 24, 32, None) == -5 and b"not enabled" in lib.sat_last_error()      # read before enable
        assert lib.sat_dit_range_report_read(plan, buf, 23, 32, None) == -1 and b"24" in lib.sat_last_error()               # capacity
        assert lib.sat_dit_range_report_read(plan, buf, 24, 24, None) == -1 and b"bytes" in lib.sat_last_error()            # another header's record
        assert lib.sat_dit_range_report_read(plan, None, 24, 32, None) == -1
        assert lib.sat_dit_range_report(plan, 3) == -1
        assert lib.sat_dit_range_report(plan, 2) == -5          # nothing to zero
        assert lib.sat_dit_range_report(plan, 0) == 0           # off when it is off: nothing to do
    finally:
        lib.sat_dit_plan_destroy(plan)
    for gemm_dtype, fam in ((1, 0), (1, 31), (2, 0)):          # fp8, fp8-all, fp32x
        plan = _dit_plan(lib, gemm_dtype, fam)
        try:
            assert lib.sat_dit_range_report(plan, 1) == -2, (gemm_dtype, fam)
            assert b"16-bit" in lib.sat_last_error()
            assert lib.sat_dit_range_report_read(plan, buf, 24, 32, None) == -5
        finally:
            lib.sat_dit_plan_destroy(plan)


def _codec_plan(lib, decoder, gemm_dtype):
    from stable_audio_tools import _hip
    v = cases.SMALL_VAE
    cfg = _hip.SatOobleckCfg()
    cfg.is_decoder, cfg.io_channels, cfg.channels, cfg.latent_dim, cfg.n_blocks = int(decoder), 2, v["channels"], 64 if decoder else 128, 5
    for i, (c, s) in enumerate(zip(v["c_mults"], v["strides"])):
        cfg.c_mults[i], cfg.strides[i] = c, s
    cfg.gemm_dtype = gemm_dtype
    plan = ctypes.c_void_p()
    assert lib.sat_oobleck_plan_create_ex(ctypes.byref(cfg), None, 0, ctypes.byref(plan)) == 0, lib.sat_last_error()
    return plan


@pytest.mark.parametrize("gemm_dtype", [3, 0, 2], ids=["fp16", "bf16", "fp32"])
@pytest.mark.parametrize("decoder", [True, False], ids=["decoder", "encoder"])
def test_codec_entry_points_and_names_without_a_device(decoder, gemm_dtype):
    """Every build answers; the names are unique, in launch order, and each is the path of a convolution of the Python module tree."""
    from stable_audio_tools import _hip
    from stable_audio_tools.models import autoencoders as AE
    lib = _hip.lib()
    n = ctypes.c_int32()
    assert lib.sat_oobleck_range_report(None, 1) == -1
    assert lib.sat_oobleck_range_report_count(None, ctypes.byref(n)) == -1
    assert lib.sat_oobleck_range_report_name(None, 0) is None
    assert lib.sat_oobleck_range_report_read(None, _records(1), 1, 32, None) == -1
    plan = _codec_plan(lib, decoder, gemm_dtype)
    try:
        assert lib.sat_oobleck_range_report_count(plan, ctypes.byref(n)) == 0
        assert lib.sat_oobleck_range_report_count(plan, None) == -1
        # decoder: input + first conv + 5 x (upsample: 2, units: 3 + 3 + 2); encoder: first conv: 2, 5 x (units: 8, downsample: 2), the last without raw
        assert n.value == (52 if decoder else 51)
        names = [lib.sat_oobleck_range_report_name(plan, i).decode() for i in range(n.value)]
        assert lib.sat_oobleck_range_report_name(plan, n.value) is None and lib.sat_oobleck_range_report_name(plan, -1) is None
        assert len(set(names)) == len(names)
        buf = _records(n.value)
        assert lib.sat_oobleck_range_report_read(plan, buf, n.value, 32, None) == -5
        assert lib.sat_oobleck_range_report_read(plan, buf, n.value - 1, 32, None) == -1
        assert lib.sat_oobleck_range_report_read(plan, buf, n.value, 40, None) == -1
        assert lib.sat_oobleck_range_report(plan, 2) == -5 and lib.sat_oobleck_range_report(plan, 0) == 0 and lib.sat_oobleck_range_report(plan, 7) == -1
    finally:
        lib.sat_oobleck_plan_destroy(plan)
    module = (AE.OobleckDecoder if decoder else AE.OobleckEncoder)(**cases.vae_kwargs(cases.SMALL_VAE, decoder))
    assert (names[0] == "input") == decoder
    convs = []
    for name in names[1 if decoder else 0:]:
        path = name[:-4] if name.endswith(".raw") else name
        assert isinstance(module.get_submodule(path), (AE.WNConv1d, AE.WNConvTranspose1d)), name
        if not name.endswith(".raw"):
            convs.append(path)
        else:
            assert convs[-1] == path          # the raw copy follows the activated tensor of the same launch
    # launch order = module order, and every convolution but the last (whose result leaves as fp32) has its record
    in_tree = [k for k, m in module.named_modules() if isinstance(m, (AE.WNConv1d, AE.WNConvTranspose1d))]
    assert convs == in_tree[:-1]
    assert ("layers.3.layers.1.layers.1" in names) == (not decoder)          # (the example of the header: an encoder unit's dilated convolution)


# ------------------------------------------------------------------------------------------------ Python lifecycle on the recording library
@pytest.fixture
def fake(monkeypatch):
    from stable_audio_tools import _hip
    lib = FakeLib()
    monkeypatch.setattr(_hip, "_lib", lib)
    monkeypatch.setattr(_hip, "ptr", lambda t: t)
    monkeypatch.setattr(_hip, "stream", lambda: "stream")
    return lib


def _cpu_dit(monkeypatch):
    from stable_audio_tools.models.dit import DiffusionTransformer
    monkeypatch.setattr(DiffusionTransformer, "_plan_device", lambda self: torch.device("cpu"))
    return DiffusionTransformer(**cases.SMALL_DIT)


def _toggles(lib, name):
    return [args[1] for n, args in lib.calls if n == name]


def test_dit_flag_survives_a_plan_rebuild(fake, monkeypatch):
    dit = _cpu_dit(monkeypatch)
    assert dit.activation_range_report(True) is None
    first = dit._plan
    # the plan is built with the report on, inside configure: between create and the first set_tensor
    names = fake.names()
    assert names.index("sat_dit_range_report") < names.index("sat_dit_plan_set_tensor") < names.index("sat_dit_plan_finalize")
    dit.set_layernorm_fusion(False)
    fake.calls.clear()
    rows = dit.activation_range_report(False)
    names = fake.names()
    assert dit._plan is not first and names[0] == "sat_dit_plan_destroy"
    i = names.index("sat_dit_plan_create_sized")
    assert names[i + 1] == "sat_dit_range_report" and fake.calls[i + 1][1] == (dit._plan, 1)          # re-applied to the new plan
    assert names[-2:] == ["sat_dit_range_report_read", "sat_dit_range_report"] and fake.calls[-1][1] == (dit._plan, 0)
    plan, buf, cap, size, stream = fake.calls[-2][1]
    assert plan is dit._plan and cap == 3 * 12 == len(buf) and size == 32 and stream == "stream"
    assert dit._range_report is False
    assert len(rows) == 36 and [r["buffer"] for r in rows[:12]] == list(dit_slots()) and rows[35]["layer"] == 2
    assert set(rows[0]) == {"layer", "buffer", "max_abs", "over_fp16", "nonfinite", "elements", "launches", "holds"}
    # fusion is off now: every a_* buffer holds a LayerNorm output, the others nothing of the kind
    assert {r["holds"] for r in rows if r["buffer"].startswith("a_")} == {"layernorm output"}
    assert {r["holds"] for r in rows if not r["buffer"].startswith("a_")} == {None}
    # a later rebuild no longer enables it
    dit.set_layernorm_fusion(True)
    fake.calls.clear()
    dit._ensure_plan()
    assert "sat_dit_range_report" not in fake.names()


def dit_slots():
    from stable_audio_tools import _hip
    return _hip.DIT_RANGE_SLOT_NAMES


def test_dit_holds_follows_the_fold(fake, monkeypatch):
    dit = _cpu_dit(monkeypatch)          # fp16 / bf16 suite default, fusion on, 64-channel heads, embed_dim 256: the fold applies
    dit.activation_range_report(True)
    rows = {(r["layer"], r["buffer"]): r["holds"] for r in dit.activation_range_report(False)}
    assert rows[(0, "a_qkv")] == "layernorm output"          # layer 0's pre_norm reads rows of the input projection
    assert rows[(1, "a_qkv")] == rows[(0, "a_cross_q")] == rows[(0, "a_ff")] == rows[(2, "a_ff")] == "residual image"


def test_dit_report_is_off_after_a_failed_read(fake, monkeypatch):
    from stable_audio_tools import _hip
    dit = _cpu_dit(monkeypatch)
    dit.activation_range_report(True)
    fake.fail, fake.fail_at = {"sat_dit_range_report_read": -5}, 0
    with pytest.raises(_hip.SatError, match="error -5"):
        dit.activation_range_report(False)
    assert fake.calls[-1] == ("sat_dit_range_report", (dit._plan, 0)) and dit._range_report is False
    assert _toggles(fake, "sat_dit_range_report") == [1, 1, 0]
    # a refused enable (an fp8 plan, say) does not leave the flag behind either
    fake.fail, fake.fail_at = {"sat_dit_range_report": -2}, 3
    with pytest.raises(_hip.SatError, match="error -2"):
        dit.activation_range_report(True)
    assert dit._range_report is False
    with pytest.raises(_hip.SatError, match="not enabled"):
        dit.reset_activation_range_report()


def test_dit_reset_is_mode_two(fake, monkeypatch):
    dit = _cpu_dit(monkeypatch)
    dit.activation_range_report(True)
    dit.reset_activation_range_report()
    assert fake.calls[-1] == ("sat_dit_range_report", (dit._plan, 2)) and dit._range_report is True


def test_codec_flag_survives_a_rebuild_and_a_failed_read(fake, monkeypatch):
    from stable_audio_tools import _hip
    from stable_audio_tools.models import autoencoders as AE
    monkeypatch.setattr(AE._OobleckHip, "_plan_device", lambda self: torch.device("cpu"))
    dec = AE.OobleckDecoder(**cases.vae_kwargs(cases.SMALL_VAE, True))
    dec.activation_range_report(True)
    names = fake.names()
    assert names.index("sat_oobleck_range_report") < names.index("sat_oobleck_plan_set_tensor")
    dec.set_gemm_dtype("fp32" if dec.gemm_dtype != "fp32" else "bf16")
    fake.calls.clear()
    dec._ensure_plan()
    names = fake.names()
    i = names.index("sat_oobleck_plan_create_ex")
    assert names[i + 1] == "sat_oobleck_range_report" and fake.calls[i + 1][1] == (dec._plan, 1)
    fake.fail, fake.fail_at = {"sat_oobleck_range_report_read": -5}, 0
    with pytest.raises(_hip.SatError, match="error -5"):
        dec.activation_range_report(False)
    assert fake.calls[-1] == ("sat_oobleck_range_report", (dec._plan, 0)) and dec._range_report is False


# ------------------------------------------------------------------------------------------------ check_fp16_range on canned tables
def _dit_row(layer, buffer, max_abs, over=0, elements=1000):
    return dict(layer=layer, buffer=buffer, holds=None, max_abs=max_abs, over_fp16=over, nonfinite=0, elements=elements, launches=2)


def _codec_row(part, name, max_abs, over=0, elements=1000):
    return dict(part=part, index=0, name=name, max_abs=max_abs, over_fp16=over, nonfinite=0, elements=elements, launches=1)


class _Reporting:
    def __init__(self, rows, log, tag):
        self.rows, self.log, self.tag = rows, log, tag

    def activation_range_report(self, enable=True):
        self.log.append((self.tag, bool(enable)))
        return None if enable else self.rows


def _stub_model(dit_rows, codec_rows, log):
    ns = type("NS", (), {})
    model, wrapper, pre = ns(), ns(), ns()
    wrapper.model = _Reporting(dit_rows, log, "dit")
    pre.model = _Reporting(codec_rows, log, "codec")
    model.model, model.pretransform = wrapper, pre
    return model


CANNED = [
    # DiT rows, codec rows, advice about (DiT, codec), headroom, where it is
    ([_dit_row(0, "ff_hidden", 1000.0), _dit_row(1, "q", 20.0)], [_codec_row("decoder", "layers.0", 4.0)], (False, False), 65.504, ("dit", "ff_hidden")),
    ([_dit_row(0, "q", 3.0), _dit_row(1, "ff_hidden", 65504.0, over=7)], [_codec_row("decoder", "layers.0", 4.0)], (True, False), 1.0, ("dit", "ff_hidden")),
    ([_dit_row(0, "q", 3.0)], [_codec_row("encoder", "layers.0", 2.0), _codec_row("decoder", "layers.5.layers.4.layers.3", 7e4, over=1)],
     (False, True), 65504.0 / 7e4, ("codec", "layers.5.layers.4.layers.3")),
    ([_dit_row(0, "k", 65504.0, over=2)], [_codec_row("decoder", "layers.1", 131008.0, over=3)], (True, True), 0.5, ("codec", "layers.1")),
    # a buffer that was never written (cross_q under the fused launch) and an all-zero one do not set the headroom
    ([_dit_row(0, "cross_q", 0.0, elements=0), _dit_row(0, "v", 0.0)], [], (False, False), math.inf, None),
]


@pytest.mark.parametrize("dit_rows,codec_rows,advised,headroom,where", CANNED)
def test_check_fp16_range_verdict(monkeypatch, dit_rows, codec_rows, advised, headroom, where):
    from stable_audio_tools.inference import generation, preflight
    log = []
    monkeypatch.setattr(generation, "generate_diffusion_cond", lambda model, **kw: log.append(("generate", kw)))
    model = _stub_model(dit_rows, codec_rows, log)
    got = preflight.check_fp16_range(model, steps=3, cfg_scale=7.0)
    # both reports on around exactly one generation with the caller's arguments, both off afterwards
    assert log == [("dit", True), ("codec", True), ("generate", dict(steps=3, cfg_scale=7.0)), ("codec", False), ("dit", False)]
    assert got["dit"] == dit_rows and got["codec"] == codec_rows
    assert got["headroom"] == pytest.approx(headroom)
    assert (any("bf16" in a for a in got["advice"]), any("fp32" in a for a in got["advice"])) == advised and len(got["advice"]) == sum(advised)
    if where is None:
        assert got["tightest"] is None
    else:
        assert got["tightest"]["where"] == where[0] and where[1] in (got["tightest"].get("buffer"), got["tightest"].get("name"))
    assert all(isinstance(line, str) for line in preflight.format_fp16_range(got))


def test_check_fp16_range_switches_the_reports_off_when_the_generation_fails(monkeypatch):
    from stable_audio_tools.inference import generation, preflight
    log = []

    def boom(model, **kw):
        raise RuntimeError("sampler failed")

    monkeypatch.setattr(generation, "generate_diffusion_cond", boom)
    with pytest.raises(RuntimeError, match="sampler failed"):
        preflight.check_fp16_range(_stub_model([], [], log))
    assert log == [("dit", True), ("codec", True), ("codec", False), ("dit", False)]
