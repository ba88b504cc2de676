"""Causal DiTs (ContinuousTransformer causal=True; reference models/transformer.py:296,304,359-398), host side: refused without
``allow_causal`` and built with it under the reference's parameter names and shapes, the combinations outside the feature still raise with a
reason, the config key and the command-line flag arrive, sat_dit_plan_set_attention_options and the unit entries validate before they touch
a device, csrc/attn_causal.h agrees with brute force, the causal kernels keep their register budgets, and -- on the float64 references the
GPU tests compare against (tests/dit_causal_units.py) -- the gates of tests/test_gpu_dit_causal.py reject the mistakes such kernels can make.
No GPU."""
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import cases  # noqa: E402
import dit_causal_cases as CC  # noqa: E402
import dit_causal_units as CU  # noqa: E402
from dit_family_host import build as _build, check_state_dict_keys, model_config  # noqa: E402
from util import FORMATS, assert_close, assert_close_sliced, rel_l2  # noqa: E402

CSRC = os.path.join(os.path.dirname(HERE), "friendly-stable-audio-tools_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
OPT = CC.FAMILY.product_kwargs
INVALID, UNSUPPORTED, STATE = -1, -2, -5


# ------------------------------------------------------------------------------- the modules
@pytest.mark.parametrize("name", sorted(CC.CONFIGS))
def test_dit_state_dict_matches_reference(name):
    """``causal`` adds no parameter: the keys are those of the reference's module, and of the same model with causal=False."""
    m, got = check_state_dict_keys(CC.FAMILY, name)
    assert m.transformer.causal and all(l.self_attn.causal for l in m.transformer.layers)
    plain = _build(**CC.without_causal(CC.CONFIGS[name]), **OPT)
    assert {k: list(v.shape) for k, v in plain.state_dict().items()} == got and not plain.transformer.causal


def test_refused_without_the_opt_in_and_built_with_it():
    with pytest.raises(NotImplementedError, match="causal") as e:
        _build(**CC.CONFIGS["plain"])
    assert "allow_causal=True" in str(e.value) and '"allow_causal": true' in str(e.value)          # the keyword and the config key
    assert _build(**CC.CONFIGS["plain"], allow_causal=True).transformer.causal
    assert not _build(**cases.SMALL_DIT, allow_causal=True).transformer.causal          # the opt-in alone changes nothing


def test_cross_attention_is_refused_with_a_reason():
    with pytest.raises(NotImplementedError, match=r"causal.*cross-attention") as e:
        _build(**dict(cases.SMALL_DIT, causal=True), allow_causal=True)
    assert "cond_token_dim" in str(e.value)


def test_operand_formats():
    m = _build(**CC.CONFIGS["plain"], **OPT)
    for dtype in ("fp8", "fp8-all"):
        with pytest.raises(NotImplementedError, match=r"causal.*gemm_dtype"):
            m.set_gemm_dtype(dtype)
    assert m.set_gemm_dtype("bf16").set_gemm_dtype("fp32x").set_gemm_dtype("fp16").gemm_dtype == "fp16"
    m.set_block_gemm_dtypes(["fp16", "bf16", "fp16"]).set_block_gemm_dtypes(None)
    m.set_layernorm_fusion(False).set_cross_attention_fusion(False)
    # what the head width refuses today stays refused
    with pytest.raises(NotImplementedError, match="dim_heads"):
        _build(**CC.CONFIGS["hd128"], **OPT).set_gemm_dtype("fp32x")
    _build(**CC.CONFIGS["hd32"], **OPT).set_gemm_dtype("fp32x")
    with pytest.raises(NotImplementedError, match="dim_heads"):
        _build(**dict(CC.CONFIGS["hd32"], conformer=True), **OPT)


def test_forward_keeps_the_reference_assertion():
    m = _build(**CC.CONFIGS["plain"], **OPT)
    with pytest.raises(AssertionError, match="Causal mode"):
        m(torch.zeros(1, 64, 8), torch.zeros(1), causal=True)


def test_the_flag_is_part_of_the_plan_options():
    """A model whose ``causal`` differs needs another plan: the flag is in the tuple that ``_ensure_plan`` compares."""
    import inspect
    from stable_audio_tools.models.dit import DiffusionTransformer
    src = inspect.getsource(DiffusionTransformer._ensure_plan)
    assert "self.transformer.causal" in src and "sat_dit_plan_set_attention_options" in src


def test_config_key_and_command_line_flag(monkeypatch):
    """DiTWrapper passes "allow_causal": true of model.diffusion.config through; generate.py --allow-causal writes the key and is an error
    with --model-name."""
    import stable_audio_tools as S
    from stable_audio_tools.models import _init
    keys = dict(causal=True, cond_token_dim=0)
    with _init.skip_init():
        with pytest.raises(NotImplementedError, match="allow_causal"):
            S.create_model_from_config(_causal_config())
        assert S.create_model_from_config(_causal_config(allow_causal=True)).model.model.transformer.causal
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "friendly-stable-audio-tools_amd"))
    import generate as G
    base = ["generate.py", "--output-dir", "o", "--cond-yaml-path", "c"]
    monkeypatch.setattr(sys, "argv", base)
    assert "allow_causal" not in G.apply_config_flags(G.get_args(), model_config(**keys))["model"]["diffusion"]["config"]
    monkeypatch.setattr(sys, "argv", base + ["--allow-causal"])
    assert G.apply_config_flags(G.get_args(), model_config(**keys))["model"]["diffusion"]["config"]["allow_causal"] is True
    monkeypatch.setattr(sys, "argv", base + ["--allow-causal", "--model-name", "some/model"])
    with pytest.raises(SystemExit):
        G.get_args()


def _causal_config(**more):
    """The reduced SA-Open config without cross-attention (the timing numbers stay as global conditioning) and with causal=True."""
    cfg = model_config(causal=True, cond_token_dim=0, **more)
    cfg["model"]["diffusion"]["cross_attention_cond_ids"] = []
    return cfg


# ------------------------------------------------------------------------------- the C ABI
def _plan(*cfg):
    from stable_audio_tools import _hip
    lib = _hip.lib()
    plan = ctypes.c_void_p()
    c = _hip.SatDitCfg(*cfg)
    assert lib.sat_dit_plan_create_sized(ctypes.byref(c), ctypes.sizeof(c), ctypes.byref(plan)) == 0, lib.sat_last_error()
    return _hip, lib, plan


def _set(lib, plan, o, size=None):
    rc = lib.sat_dit_plan_set_attention_options(plan, ctypes.byref(o), ctypes.sizeof(o) if size is None else size)
    return rc, (lib.sat_last_error() if rc else b"")


NO_CROSS = (64, 256, 2, 4, 0, 0, 96, 128)          # io, embed, depth, heads, cond_token_dim, cond_embed_dim, global_cond_dim, max_seq_len


def test_attention_options_entry_point_validates_without_gpu():
    _hip, lib, plan = _plan(*NO_CROSS)
    O = _hip.SatDitAttentionOptions
    try:
        assert ctypes.sizeof(O) == 4 and lib.sat_version() == 6 and ctypes.sizeof(_hip.SatDitCfg) == 56
        assert ctypes.sizeof(_hip.SatDitCreateOptions) == 4 and ctypes.sizeof(_hip.SatDitTransformerOptions) == 16          # the pinned sizes
        assert _set(lib, plan, O(1)) == (0, b"") and _set(lib, plan, O(0)) == (0, b"") and _set(lib, plan, O(1)) == (0, b"")
        for size in (0, 3, 8):
            rc, msg = _set(lib, plan, O(1), size)
            assert rc == INVALID and b"sat_dit_attention_options" in msg, (size, rc, msg)
        for value in (2, -1):
            rc, msg = _set(lib, plan, O(value))
            assert rc == INVALID and b"causal" in msg, (value, rc, msg)
        assert lib.sat_dit_plan_set_attention_options(plan, None, 4) == INVALID
        assert lib.sat_dit_plan_set_attention_options(None, ctypes.byref(O(1)), 4) == INVALID
    finally:
        lib.sat_dit_plan_destroy(plan)


@pytest.mark.parametrize("cfg, why", [((64, 256, 2, 4, 128, 128, 96, 128), b"cross-attention"), ((64, 256, 2, 4, 0, 0, 96, 128, 0, 1), b"fp8")],
                         ids=["cross-attention", "e4m3"])
def test_attention_options_refuses_cross_attention_and_e4m3(cfg, why):
    _hip, lib, plan = _plan(*cfg)
    try:
        rc, msg = _set(lib, plan, _hip.SatDitAttentionOptions(1))
        assert rc == UNSUPPORTED and b"causal" in msg and why in msg, (rc, msg)
        assert _set(lib, plan, _hip.SatDitAttentionOptions(0)) == (0, b"")          # the default passes on every plan
    finally:
        lib.sat_dit_plan_destroy(plan)


def test_attention_options_after_finalize_is_a_state_error():
    """plan_finalize needs a device; the state check is the first thing behind the size check, so the text of the entry point pins it here and
    tests/test_gpu_dit_causal.py makes the call on a finalized plan."""
    text = open(os.path.join(CSRC, "dit_plan.hip")).read()
    body = text[text.index('extern "C" int sat_dit_plan_set_attention_options'):]
    body = body[:body.index("\n}\n")]
    assert re.search(r"SAT_CHECK_ARG\(!p->finalized, SAT_E_STATE", body)
    assert body.index("SAT_E_STATE") < body.index("o->causal == 0")


def test_unit_entries_validate_without_gpu():
    from stable_audio_tools import _hip
    lib = _hip.lib()
    p = ctypes.c_void_p(1 << 20)          # never dereferenced: every call below fails its checks
    for fn in (lib.sat_attention_causal_bf16, lib.sat_attention_causal_f16):
        for w in (48, 0, 160):
            assert fn(p, p, p, p, 1, 2, 2, w, 78, 128, 128, 1, None) == UNSUPPORTED and b"dim_heads" in lib.sat_last_error(), w
        for w in (32, 96, 128):
            assert fn(p, p, p, p, 1, 2, 2, w, 78, 128, 128, 0, None) == UNSUPPORTED          # these widths take a pre-scaled Q only
        assert fn(p, p, p, p, 1, 2, 2, 64, 78, 128, 128, 2, None) == INVALID               # prescaled
        assert fn(p, p, p, p, 1, 2, 2, 32, 78, 128, 192, 1, None) == INVALID               # s_pad_k % 128 with 32-channel heads
        for w in (64, 96, 128):
            assert fn(p, p, p, p, 1, 2, 2, w, 78, 128, 96, 1, None) == INVALID             # s_pad_k % 64
            assert fn(p, p, p, p, 1, 2, 2, w, 78, 64, 128, 1, None) == INVALID             # s_pad_q % 128
            assert fn(p, p, p, p, 1, 2, 2, w, 126, 128, 128, 1, None) == INVALID           # s_pad_k >= s + 3
            assert fn(p, p, p, p, 1, 3, 2, w, 78, 128, 128, 1, None) == INVALID            # 3 query heads over 2 kv heads
            assert fn(p, ctypes.c_void_p((1 << 20) + 8), p, p, 1, 2, 2, w, 78, 128, 128, 1, None) == INVALID          # alignment
            assert fn(p, p, p, p, 1, 2, 2, w, 0, 128, 128, 1, None) == INVALID
    for w in (128, 48):
        assert lib.sat_attention_f32_causal(p, p, p, p, 1, 2, 2, w, 8, None) == UNSUPPORTED and b"dim_heads" in lib.sat_last_error()
    assert lib.sat_attention_f32_causal(p, p, p, p, 1, 3, 2, 32, 8, None) == INVALID
    assert lib.sat_attention_f32_causal(p, p, p, p, 1, 2, 2, 64, 0, None) == INVALID


# ------------------------------------------------------------------------------- the ranges
def test_causal_ranges_agree_with_brute_force(tmp_path):
    line = CU.check_ranges(str(tmp_path), 700)
    print("\n" + line)
    skipped, diag, full = (int(x) for x in re.search(r"skipped (\d+) diagonal (\d+) full (\d+)", line).groups())
    assert skipped > 0 and diag > 0 and full > diag          # most of what is walked runs without a compare


def test_every_kernel_takes_its_ranges_from_the_header():
    for src, calls in (("attention.hip", ("attnc::tiles_walked", "attnc::key_end")), ("attn_core.h", ("attnc::block_class",)),
                       ("attention_hdw.hip", ("attnc::tiles_walked", "attnc::key_end")),          # (its blocks are classed by attn_core.h's step)
                       ("f32_ref.hip", ("attnc::tiles_walked",))):
        text = open(os.path.join(CSRC, src)).read()
        for c in calls:
            assert c in text, (src, c)


# ------------------------------------------------------------------------------- the kernels, compiled and inspected
def _kernels(src, defines, tmp):
    out = os.path.join(tmp, "k.s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", os.path.join(CSRC, src), "-o", out] + defines,
                   check=True, capture_output=True)
    meta = {}
    for blk in open(out).read().split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        meta[name] = {k: int(re.search(rf"\.{k}:\s+(\d+)", blk).group(1)) for k in ("vgpr_count", "vgpr_spill_count", "private_segment_fixed_size")}
    return meta


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
@pytest.mark.parametrize("defines", [[], ["-DSAT_OPERAND_F16"]], ids=["bf16", "f16"])
def test_causal_kernels_keep_their_register_budgets(defines, tmp_path):
    """The causal twins stay where their non-causal kernels are gated: 128 VGPRs for the two 64-channel layouts (four waves per SIMD) and for
    32-channel heads (two workgroups per CU), 256 for 96 and 128; no spill, no scratch."""
    meta = _kernels("attention.hip", defines, str(tmp_path))
    causal = {n: m for n, m in meta.items() if "attention_kernel" in n and n.split("attention_kernelILb")[1].startswith("0ELi0ELi") and "ELb1EE" in n}
    assert len(causal) == 2, sorted(meta)          # one group and two groups, MODE 1
    for n, m in causal.items():
        assert "ELi1ELb1EE" in n, n                # MODE 1
        assert m["vgpr_count"] <= 128 and m["vgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, (n, m)
    meta = _kernels("attention_hdw.hip", defines, str(tmp_path))
    twins = {n: m for n, m in meta.items() if "attention_hdw_kernelILi" in n and "ELb1EE" in n}
    assert len(twins) == 3, sorted(meta)
    for n, m in twins.items():
        budget = 128 if "kernelILi32E" in n else 256
        assert m["vgpr_count"] <= budget and m["vgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, (n, m)
    print("\n" + "\n".join(f"{n}: {m['vgpr_count']} VGPRs" for n, m in {**causal, **twins}.items()))


# ------------------------------------------------------------------------------- the gates bite
def _gates(fmt, got, want, h):
    """The unit gates of tests/test_gpu_dit_causal.py on a [b, s, h * W] result; returns the failure text or None."""
    b, s, _ = want.shape
    try:
        assert_close("causal attention", got, want, fmt.tol(5e-3))
        assert_close_sliced("causal attention per (sequence, query, head)", got.view(b, s, h, -1), want.view(b, s, h, -1), fmt.tol(5e-3), (0, 1, 2),
                            fmt.round)
    except AssertionError as e:
        return str(e)
    return None


@pytest.mark.parametrize("fmt", FORMATS, ids=repr)
@pytest.mark.parametrize("w", [32, 64])
def test_unit_gates_pass_the_reference_and_reject_the_mistakes(fmt, w):
    """At b = 4, s = 301 (key shifts 0..3): the float32 evaluation of the matched-rounding reference, rounded to the output format, passes;
    an off-by-one diagonal in either direction, a mask that ignores the key shift, a dropped last tile and leaked pad keys do not."""
    b, h, kvh, s = 4, 4, 2, 301
    q, q_eff, k, v = CU.unit_tensors(fmt, w, b, h, kvh, s)
    want = CU.causal_attention(q_eff, k, v, rnd=fmt.round)
    assert _gates(fmt, fmt.round(want.float()), want.float(), h) is None
    assert rel_l2(want, CU.causal_attention(q_eff, k, v)) < fmt.tol(1e-2)          # matched rounding against exact: the third gate of the GPU test
    for mistake in CU.MISTAKES:
        wrong = fmt.round(CU.causal_attention(q_eff, k, v, rnd=fmt.round, mistake=mistake).float())
        msg = _gates(fmt, wrong, want.float(), h)
        assert msg is not None, f"{mistake}: the gates accept it (whole-tensor rel-L2 {rel_l2(wrong, want):.3e})"


def test_the_reference_is_attention_core_with_the_mask():
    """Without a mask to apply (s = 1) and against an explicit -inf mask in float32, the restatement is oracle.dit.attention_core."""
    from oracle import dit as odit
    fmt = FORMATS[1]
    q, q_eff, k, v = CU.unit_tensors(fmt, 64, 2, 4, 2, 1)
    assert rel_l2(CU.causal_attention(q_eff, k, v, rnd=fmt.round), odit._merge(odit.attention_core(q_eff, k.float(), v.float(), rnd=fmt.round))) < 1e-6
    q, q_eff, k, v = CU.unit_tensors(fmt, 64, 2, 4, 2, 70)
    kk, vv = (t.float().repeat_interleave(2, dim=1) for t in (k, v))
    dots = torch.einsum("bhid,bhjd->bhij", q_eff, kk) / 8.0
    dots = dots.masked_fill(~torch.tril(torch.ones(70, 70, dtype=torch.bool)), float("-inf"))
    want = odit._merge(torch.softmax(dots, dim=-1) @ vv)
    assert rel_l2(CU.causal_attention(q_eff, k, v), want) < 1e-6
    want = odit._merge(torch.nn.functional.scaled_dot_product_attention(q_eff, kk, vv, is_causal=True))          # what the reference calls
    assert rel_l2(CU.causal_attention(q_eff, k, v), want) < 1e-6
