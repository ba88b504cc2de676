"""Operand format per DiT block (sat_dit_plan_set_block_formats, DiffusionTransformer.set_block_gemm_dtypes, preflight.choose_block_formats),
host side.  The entry point's argument checks run on a plan that is never finalized; what a finalized plan launches is read off
tests/host/block_formats_dump.cpp, built like the driver of tests/test_dit_launches_host.py (csrc/dit_plan.hip compiled host-only, every
launcher a function that prints its arguments): a depth-3 plan with formats [fp16, bf16, fp16].  No GPU."""
import ctypes
import os
import shutil
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

import cases  # noqa: E402

CSRC = os.path.join(ROOT, "friendly-stable-audio-tools_amd", "csrc")
HOST = os.path.join(HERE, "host")
HIPCC = "/opt/rocm/bin/hipcc"
SET_RC = "rc sat_dit_plan_set_block_formats "
EPI_RESID, EPI_SWIGLU, EPI_HEADS = 1, 2, 3


# ------------------------------------------------------------------------------ the C ABI on a plan that is never finalized
def _plan(lib, _hip, gemm_dtype=3, fp8_families=0, depth=3):
    plan = ctypes.c_void_p()
    cfg = _hip.SatDitCfg(64, 256, depth, 4, 128, 128, 96, 128, 0, gemm_dtype, fp8_families)
    assert lib.sat_dit_plan_create(ctypes.byref(cfg), ctypes.byref(plan)) == 0, lib.sat_last_error()
    return plan


def _formats(*v):
    return (ctypes.c_int32 * len(v))(*v)


def test_entry_point_validates_without_gpu():
    from stable_audio_tools import _hip
    lib = _hip.lib()
    F16, BF16 = 3, 0
    ok = _formats(F16, BF16, F16)
    assert lib.sat_dit_plan_set_block_formats(None, ok, 3) == -1 and b"null" in lib.sat_last_error()
    for gemm_dtype in (F16, BF16):
        plan = _plan(lib, _hip, gemm_dtype)
        try:
            assert lib.sat_dit_plan_set_block_formats(plan, None, 3) == -1
            for n in (0, 2, 4, -1):          # n != depth: SAT_E_INVALID with the two numbers
                assert lib.sat_dit_plan_set_block_formats(plan, ok, n) == -1
                assert b"depth 3" in lib.sat_last_error(), lib.sat_last_error()
            for bad in (1, 2, 4, -1):        # e4m3, fp32x and numbers that name nothing
                assert lib.sat_dit_plan_set_block_formats(plan, _formats(F16, bad, F16), 3) == -1
                assert b"formats[1]" in lib.sat_last_error(), lib.sat_last_error()
            for good in (ok, _formats(BF16, BF16, BF16), _formats(F16, F16, F16), _formats(BF16, F16, F16)):
                assert lib.sat_dit_plan_set_block_formats(plan, good, 3) == 0, lib.sat_last_error()
        finally:
            lib.sat_dit_plan_destroy(plan)
    # e4m3 plans (both family sets) and the fp32 verification mode: SAT_E_UNSUPPORTED
    for gemm_dtype, families in ((1, 0), (1, 31), (2, 0)):
        plan = _plan(lib, _hip, gemm_dtype, families)
        try:
            assert lib.sat_dit_plan_set_block_formats(plan, ok, 3) == -2
            assert b"gemm_dtype" in lib.sat_last_error()
        finally:
            lib.sat_dit_plan_destroy(plan)


def test_layouts_are_the_ones_before_the_call_existed():
    from stable_audio_tools import _hip
    assert ctypes.sizeof(_hip.SatDitCfg) == 56 and ctypes.sizeof(_hip.SatDitTransformerOptions) == 16
    assert _hip.lib().sat_version() == 6


# ------------------------------------------------------------------------------ the module
def _build(**kwargs):
    from stable_audio_tools.models import _init
    from stable_audio_tools.models.dit import DiffusionTransformer
    with _init.skip_init():
        return DiffusionTransformer(**kwargs)


def test_setter_reads_back_and_invalidates_the_plan():
    m = _build(**cases.SMALL_DIT).set_gemm_dtype("fp16")
    assert m.block_gemm_dtypes == ["fp16"] * 3
    m._plan_version = "built"
    assert m.set_block_gemm_dtypes(["fp16", "bf16", "fp16"]) is m
    assert m.block_gemm_dtypes == ["fp16", "bf16", "fp16"] and m._plan_version is None and m.gemm_dtype == "fp16"
    m._plan_version = "built"
    m.set_block_gemm_dtypes(("fp16", "bf16", "fp16"))          # the same list again: the plan stays
    assert m._plan_version == "built"
    m.block_gemm_dtypes.append("bf16")                         # a copy is read back
    assert m.block_gemm_dtypes == ["fp16", "bf16", "fp16"]
    assert m.set_block_gemm_dtypes(None) is m
    assert m.block_gemm_dtypes == ["fp16"] * 3 and m._plan_version is None
    m.set_gemm_dtype("bf16")
    assert m.block_gemm_dtypes == ["bf16"] * 3


def test_setter_errors():
    m = _build(**cases.SMALL_DIT).set_gemm_dtype("fp16")
    for wrong in ([], ["fp16"] * 2, ["fp16"] * 4):
        with pytest.raises(ValueError, match="depth 3"):
            m.set_block_gemm_dtypes(wrong)
    for bad in ("fp8", "fp32x", "fp32", "FP16", 3, None):
        with pytest.raises(ValueError, match="'fp16' or 'bf16'"):
            m.set_block_gemm_dtypes(["fp16", bad, "fp16"])
    assert m.block_gemm_dtypes == ["fp16"] * 3 and m._block_gemm_dtypes is None          # a refused list changes nothing
    for dtype in ("fp8", "fp8-all", "fp32x"):
        m.set_gemm_dtype(dtype)
        with pytest.raises(NotImplementedError, match="gemm_dtype"):
            m.set_block_gemm_dtypes(["fp16", "bf16", "fp16"])
        assert m.set_block_gemm_dtypes(None) is m               # clearing is always accepted


@pytest.mark.parametrize("later", ["fp16", "bf16", "fp8", "fp32x"])
def test_set_gemm_dtype_clears_the_list(later):
    m = _build(**cases.SMALL_DIT).set_gemm_dtype("fp16").set_block_gemm_dtypes(["fp16", "bf16", "fp16"])
    m._plan_version = "built"
    m.set_gemm_dtype(later)                                     # "fp16": the same dtype as before still clears, and rebuilds
    assert m._block_gemm_dtypes is None and m.block_gemm_dtypes == [later] * 3 and m._plan_version is None


# ------------------------------------------------------------------------------ the chooser and the verdict, on hand-made rows
def _row(layer, buffer, max_abs, over=0, elements=1000, fmt=None):
    r = dict(layer=layer, buffer=buffer, holds=None, max_abs=max_abs, over_fp16=over, nonfinite=0, elements=elements, launches=1)
    if fmt is not None:
        r["format"] = fmt
    return r


def test_choose_block_formats():
    from stable_audio_tools.inference import preflight
    rows = [_row(0, "q", 10.0), _row(0, "ff_hidden", 30000.0), _row(1, "q", 3.0), _row(1, "ff_hidden", 65504.0, over=7), _row(2, "ff_hidden", 16000.0),
            _row(3, "attn_out", 65504.0), _row(4, "cross_q", 0.0, elements=0)]
    before = [dict(r) for r in rows]
    summary = preflight.summarize_fp16_range(rows, [dict(part="decoder", name="layers.0", max_abs=7e4, over_fp16=3, nonfinite=0, elements=10, launches=1)])
    assert preflight.choose_block_formats(summary) == ["fp16", "bf16", "fp16", "bf16", "fp16"]          # over_fp16 > 0; max_abs at the limit
    assert preflight.choose_block_formats(summary, min_headroom=2.0) == ["fp16", "bf16", "fp16", "bf16", "fp16"]       # 30000 * 2 < 65504
    assert preflight.choose_block_formats(summary, min_headroom=2.5) == ["bf16", "bf16", "fp16", "bf16", "fp16"]
    assert preflight.choose_block_formats(summary, min_headroom=5.0) == ["bf16", "bf16", "bf16", "bf16", "fp16"]
    assert rows == before                                                                                # changes nothing
    # a bf16 block whose values fp16 would clamp stays where it is; the codec's rows never move a block
    rows = [_row(0, "q", 10.0, fmt="fp16"), _row(1, "ff_hidden", 3e5, over=9, fmt="bf16"), _row(2, "q", 1.0, fmt="fp16")]
    assert preflight.choose_block_formats(preflight.summarize_fp16_range(rows, [])) == ["fp16", "bf16", "fp16"]
    assert preflight.choose_block_formats(preflight.summarize_fp16_range([], [])) == []


def test_summary_counts_a_bf16_block_as_handled():
    from stable_audio_tools.inference import preflight
    clamped = [_row(0, "q", 10.0, fmt="fp16"), _row(1, "ff_hidden", 65504.0, over=9, fmt="fp16"), _row(2, "q", 1.0, fmt="fp16")]
    got = preflight.summarize_fp16_range(clamped, [])
    assert len(got["advice"]) == 1 and "bf16" in got["advice"][0] and got["handled"] == 0 and got["headroom"] == 1.0
    fixed = [_row(0, "q", 10.0, fmt="fp16"), _row(1, "ff_hidden", 3e5, over=9, fmt="bf16"), _row(2, "q", 100.0, fmt="fp16")]
    got = preflight.summarize_fp16_range(fixed, [])
    assert got["advice"] == [] and got["handled"] == 1
    assert got["headroom"] == pytest.approx(655.04) and got["tightest"]["layer"] == 2          # the fp16 blocks' headroom: bf16 has the range
    text = "\n".join(preflight.format_fp16_range(got))
    assert "[1] run in bf16" in text and "advice" not in text
    # rows without a format (a model that never set per-block formats) are judged as before
    got = preflight.summarize_fp16_range([_row(1, "ff_hidden", 3e5, over=9)], [])
    assert len(got["advice"]) == 1 and got["handled"] == 0
    # one fp16 block still over: the advice stays, next to the handled one
    got = preflight.summarize_fp16_range(fixed + [_row(2, "ff_hidden", 65504.0, over=1, fmt="fp16")], [])
    assert len(got["advice"]) == 1 and got["handled"] == 1


def test_apply_fp16_range_fix_checks_applies_and_checks_again(monkeypatch):
    from stable_audio_tools.inference import preflight
    log = []

    class Dit:
        formats = None

        def set_block_gemm_dtypes(self, formats):
            log.append(("set", list(formats)))
            self.formats = list(formats)
            return self

    dit = Dit()
    ns = type("NS", (), {})
    model, wrapper = ns(), ns()
    wrapper.model, model.model = dit, wrapper

    def check(m, steps=8, **kw):
        log.append(("check", steps, kw))
        if dit.formats is None:
            return preflight.summarize_fp16_range([_row(0, "q", 5.0), _row(1, "ff_hidden", 65504.0, over=4), _row(2, "q", 5.0)], [])
        return preflight.summarize_fp16_range([_row(l, "ff_hidden", 2e5 if f == "bf16" else 5.0, over=4 if f == "bf16" else 0, fmt=f)
                                               for l, f in enumerate(dit.formats)], [])

    monkeypatch.setattr(preflight, "check_fp16_range", check)
    before, after = preflight.apply_fp16_range_fix(model, steps=3, cfg_scale=7.0)
    assert log == [("check", 3, dict(cfg_scale=7.0)), ("set", ["fp16", "bf16", "fp16"]), ("check", 3, dict(cfg_scale=7.0))]
    assert len(before["advice"]) == 1 and after["advice"] == [] and after["handled"] == 1
    assert not any(r["over_fp16"] > 0 for r in after["dit"] if r["format"] == "fp16")


# ------------------------------------------------------------------------------ what a finalized plan launches
@pytest.fixture(scope="module")
def dumped(tmp_path_factory):
    """{case name: [lines]} of tests/host/block_formats_dump.cpp linked against the tree's dit_plan.hip."""
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    work = str(tmp_path_factory.mktemp("block_formats"))
    cc = [HIPCC, "--offload-arch=gfx950", "-std=c++17", "-fPIC", "--cuda-host-only", "-I", CSRC, "-I", HOST]
    plan, drv, exe = (os.path.join(work, n) for n in ("dit_plan.o", "block_formats_dump.o", "block_formats_dump"))
    jobs = [subprocess.Popen(cc + ["-c", os.path.join(CSRC, "dit_plan.hip"), "-o", plan], stderr=subprocess.PIPE, text=True),
            subprocess.Popen(cc + ["-Wall", "-Wno-unused-function", "-x", "hip", "-c", os.path.join(HOST, "block_formats_dump.cpp"), "-o", drv],
                             stderr=subprocess.PIPE, text=True)]
    for j in jobs:
        err = j.communicate()[1]
        assert j.returncode == 0, err
    link = shutil.which("g++") or "/opt/rocm/lib/llvm/bin/clang++"          # no HIP runtime on the link line: the driver is the runtime
    subprocess.run([link, plan, drv, "-lm", "-o", exe], check=True, capture_output=True)
    out, name = {}, None
    for ln in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split("\n")[:-1]:
        if ln.startswith("== "):
            name = ln[3:]
            out[name] = []
        else:
            out[name].append(ln)
    return out


def _between(lines, after, until):
    i = next(k for k, ln in enumerate(lines) if ln.startswith(after))
    j = next(k for k, ln in enumerate(lines) if ln.startswith(until))
    assert i < j
    return lines[i + 1:j]


def _forward(lines):
    return _between(lines, "workspace_bytes", "rc sat_dit_forward")


def _blocks(forward):
    """The forward's launches per block: a block ends behind its third residual GEMM (self to_out, cross to_out, FF-out)."""
    out, cur, resid = [], [], 0
    started = False
    for ln in forward:
        tok = ln.split()
        if not started and tok[0] not in ("sat_launch_layernorm", "sat_launch_layernorm_mod", "sat_launch_gemm"):
            continue          # the embeddings and the input projection in front of block 0
        started = True
        cur.append(ln)
        if tok[0] == "sat_launch_gemm" and int(tok[1]) == EPI_RESID:
            resid += 1
            if resid == 3:
                out.append(cur)
                cur, resid = [], 0
    return out          # (the output projection stays behind in cur)


def _f16_of(ln):
    tok = ln.split()
    if tok[0] == "sat_launch_gemm":
        return int(tok[tok.index("f16") + 1])
    assert tok[0] in ("sat_launch_layernorm", "sat_launch_layernorm_mod", "sat_launch_attention", "sat_launch_pack_rows_bf16", "sat_launch_pack_rows_ln")
    return int(tok[-1])


def _carries_format(ln):
    return ln.split()[0] in ("sat_launch_gemm", "sat_launch_layernorm", "sat_launch_layernorm_mod", "sat_launch_attention")


def _fold_fields(ln):
    """(xb, ln_part_out, ln_part) of a sat_launch_gemm line."""
    tok = ln.split()
    i = tok.index("fold")
    return tok[i + 1], tok[i + 2], tok[i + 3]


def _without_set_rc(lines):
    assert sum(ln.startswith(SET_RC) for ln in lines) == 1 and SET_RC + "0" in lines
    return [ln for ln in lines if not ln.startswith(SET_RC)]


@pytest.mark.parametrize("uniform, plain", [("uniform_fp16_fold", "plain_fp16_fold"), ("uniform_bf16_fold", "plain_bf16_fold"),
                                            ("all_bf16_on_fp16_plan_fold", "plain_bf16_fold")])
def test_uniform_vector_prints_what_the_plan_without_the_call_prints(dumped, uniform, plain):
    """Every allocation, copy, offset, launch argument and return code, finalize and prepare_context included."""
    assert all(ln.startswith("rc ") and ln.endswith(" 0") for ln in dumped[plain] if ln.startswith("rc "))
    assert _without_set_rc(dumped[uniform]) == dumped[plain]
    assert len(_blocks(_forward(dumped[plain]))) == 3


@pytest.mark.parametrize("mixed, plain, want", [("mixed_fold", "plain_fp16_fold", [1, 0, 1]), ("mixed_tail_fold", "plain_bf16_fold", [0, 1, 1]),
                                                ("mixed", "plain_fp16", [1, 0, 1]), ("mixed_adaln", "plain_fp16_adaln", [1, 0, 1])])
def test_every_launch_of_a_block_carries_its_format(dumped, mixed, plain, want):
    lines = dumped[mixed]
    assert SET_RC + "0" in lines and "rc sat_dit_forward 0" in lines and "rc sat_dit_plan_finalize 0" in lines
    blocks = _blocks(_forward(lines))
    assert len(blocks) == 3
    for l, blk in enumerate(blocks):
        flagged = [ln for ln in blk if _carries_format(ln)]
        assert len(flagged) >= 7 and {_f16_of(ln) for ln in flagged} == {want[l]}, (l, blk)
        assert sum(int(ln.split()[1]) == EPI_SWIGLU for ln in blk if ln.startswith("sat_launch_gemm ")) == 1
    # the weight images made at finalize: per layer 7 Linears (to_qkv, to_out, cross to_q / to_kv / to_out, FF-in, FF-out) in the layer's format
    packs = [_f16_of(ln) for ln in _between(lines, "rc sat_dit_plan_set_block_formats", "rc sat_dit_plan_finalize") if ln.startswith("sat_launch_pack_rows_")]
    assert packs == [f for f in want for _ in range(7)]
    # the cross K / V cache: one to_kv GEMM per layer in its format, each reading the context embedding written in that format
    ctx = _between(lines, "rc sat_dit_plan_finalize", "rc sat_dit_prepare_context")
    kv = [ln for ln in ctx if ln.startswith("sat_launch_gemm ")]
    assert [_f16_of(ln) for ln in kv] == want
    embeds = {int(ln.split()[-1]): ln.split()[7] for ln in ctx if ln.startswith("glue_small_linear ") and int(ln.split()[-1]) != 0}
    assert set(embeds) == {1, 2} and embeds[1] != embeds[2]          # out16 1 = bf16, 2 = fp16, two buffers
    for ln, f in zip(kv, want):
        assert ln.split()[ln.split().index("A") + 1] == embeds[2 if f else 1]
    # nothing grows but the context buffer's second embedding: the same arena and workspace as the plan without the call
    size_of = lambda ls, k: [ln for ln in ls if ln.startswith("hipMalloc ")][k].split()[-1]
    # (under the fold a block behind a format change keeps no c1 / c2 for its to_qkv, [3 * 256] floats each: the arena is that much smaller)
    boundaries = sum(want[l] != want[l - 1] for l in (1, 2)) if mixed.endswith("_fold") else 0
    assert int(size_of(lines, 0)) == int(size_of(dumped[plain], 0)) - boundaries * 2 * 3 * 256 * 4
    assert [ln for ln in lines if ln.startswith("workspace_bytes")] == [ln for ln in dumped[plain] if ln.startswith("workspace_bytes")]
    assert int(size_of(lines, 1)) > int(size_of(dumped[plain], 1))


def _standalone_layernorms(blk):
    # (the first LayerNorm of a block goes through the launcher that also takes the adaLN vectors, null here)
    return [ln for ln in blk if ln.split()[0] in ("sat_launch_layernorm", "sat_launch_layernorm_mod")]


@pytest.mark.parametrize("mixed, plain, want", [("mixed_fold", "plain_fp16_fold", [1, 0, 1]), ("mixed_tail_fold", "plain_bf16_fold", [0, 1, 1])])
def test_one_standalone_layernorm_per_format_boundary(dumped, mixed, plain, want):
    """Under the fold block 0 alone runs a LayerNorm kernel.  A block behind a format change does the same for its first LayerNorm, takes the
    non-fold to_qkv, and the FF-out in front of it writes no 16-bit image; everything else keeps the fold."""
    base = _blocks(_forward(dumped[plain]))
    assert [len(_standalone_layernorms(b)) for b in base] == [1, 0, 0]
    blocks = _blocks(_forward(dumped[mixed]))
    boundary = [l > 0 and want[l] != want[l - 1] for l in range(3)]
    assert [len(_standalone_layernorms(b)) for b in blocks] == [1] + [int(b) for b in boundary[1:]]
    assert sum(len(b) for b in blocks) == sum(len(b) for b in base) + sum(boundary)          # one more launch per boundary, nothing else
    for l, blk in enumerate(blocks):
        gemms = [ln for ln in blk if ln.startswith("sat_launch_gemm ")]
        qkv, ff_out = gemms[0], gemms[-1]
        assert int(qkv.split()[1]) == EPI_HEADS and int(ff_out.split()[1]) == EPI_RESID
        own_ln = l == 0 or boundary[l]
        if own_ln:
            ln = _standalone_layernorms(blk)[0]
            assert blk[0] == ln and _f16_of(ln) == want[l] and ln.split()[1] == "ws+0"          # reads the fp32 residual rows
            assert _fold_fields(qkv)[2] == "null"
        else:
            assert _fold_fields(qkv)[2] != "null"
        # the FF-out feeds a folded LayerNorm only when the next block has its format
        feeds = l + 1 < 3 and not boundary[l + 1]
        assert (_fold_fields(ff_out)[0] != "null") == feeds and (_fold_fields(ff_out)[1] != "null") == feeds
        # cross to_q and FF-in keep the fold in every block
        consumers = [g for g in gemms[1:] if int(g.split()[1]) in (EPI_HEADS, EPI_SWIGLU)]
        assert len(consumers) == 2 and all(_fold_fields(g)[2] != "null" for g in consumers)
        # and the fold's weights were packed for exactly those
    packs = [ln.split()[0] for ln in _between(dumped[mixed], "rc sat_dit_plan_set_block_formats", "rc sat_dit_plan_finalize")
             if ln.startswith("sat_launch_pack_rows_")]
    per_layer = [packs[7 * l:7 * l + 7] for l in range(3)]
    for l in range(3):
        assert (per_layer[l][0] == "sat_launch_pack_rows_ln") == (not (l == 0 or boundary[l]))
        assert per_layer[l].count("sat_launch_pack_rows_ln") == (2 if l == 0 or boundary[l] else 3)


@pytest.mark.parametrize("mixed, plain", [("mixed", "plain_fp16"), ("mixed_adaln", "plain_fp16_adaln")])
def test_without_the_fold_only_the_format_flags_differ(dumped, mixed, plain):
    got, base = _blocks(_forward(dumped[mixed])), _blocks(_forward(dumped[plain]))
    assert [[ln.split()[0] for ln in b] for b in got] == [[ln.split()[0] for ln in b] for b in base]
    assert got[0] == base[0] and got[2] == base[2] and got[1] != base[1]          # (same offsets: both formats are 2 bytes)


def test_refusals_of_the_driver(dumped):
    after = dumped["after_finalize"]
    assert after.count(SET_RC + "0") == 1 and after.count(SET_RC + "-5") == 1
    assert any(ln.startswith("error:") and "already finalized" in ln for ln in after)
    assert after.index(SET_RC + "-5") > after.index("rc sat_dit_plan_finalize 0")
    # the refused call changed nothing: the forward behind it is the mixed plan's
    assert _forward(after) == _forward(dumped["mixed_fold"])
    for name, rc, text in (("wrong_n", -1, "2 formats for a plan of depth 3"), ("bad_value", -1, "formats[1] = 1"), ("refused_fp8", -2, "gemm_dtype 1"),
                           ("refused_fp8_all", -2, "gemm_dtype 1"), ("refused_fp32x", -2, "gemm_dtype 2")):
        lines = dumped[name]
        assert SET_RC + str(rc) in lines and any(ln.startswith("error:") and text in ln for ln in lines), lines
