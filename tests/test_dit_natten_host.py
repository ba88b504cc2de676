"""Neighbourhood-attention DiTs (ContinuousTransformer attn_kwargs natten_kernel_size; reference models/transformer.py:299,324,479-493),
host side: refused without ``allow_natten`` and built with it under the reference's parameter names and shapes, the combinations outside
the feature raise with a reason, the config key and the command-line flag arrive, sat_dit_plan_set_neighborhood_attention and the unit
entries validate before they touch a device, csrc/attn_window.h agrees with brute force, the new kernels keep their register budgets, the
NATTEN stand-in of the goldens (tests/golden/natten_standin.py) is a float64 masked softmax, the reference with K == n is its own full
attention with q * 8, and -- on the float64 references the GPU tests compare against (tests/dit_natten_units.py) -- the gates of
tests/test_gpu_dit_natten.py reject the mistakes such kernels can make.  No GPU."""
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
import dit_natten_cases as NC  # noqa: E402
import dit_natten_units as NU  # noqa: E402
import natten_standin  # noqa: E402
from dit_family_host import build as _build, check_state_dict_keys, model_config  # noqa: E402
from util import FORMATS, assert_close, assert_close_sliced, rel_l2  # noqa: E402

CSRC = os.path.join(os.path.dirname(HERE), "friendly-stable-audio-tools_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
OPT = NC.FAMILY.product_kwargs
INVALID, UNSUPPORTED, STATE = -1, -2, -5
PLAIN = NC.CONFIGS["k33"]


# ------------------------------------------------------------------------------- the modules
@pytest.mark.parametrize("name", sorted(NC.CONFIGS))
def test_dit_state_dict_matches_reference(name):
    """``natten_kernel_size`` adds no parameter: the keys are those of the reference's module, and of the same model with full attention."""
    m, got = check_state_dict_keys(NC.FAMILY, name)
    assert m.transformer.natten_kernel_size == NC.KERNEL[name]
    assert all(l.self_attn.natten_kernel_size == NC.KERNEL[name] for l in m.transformer.layers)
    plain = _build(**NC.without_natten(NC.CONFIGS[name]), **OPT)
    assert {k: list(v.shape) for k, v in plain.state_dict().items()} == got and plain.transformer.natten_kernel_size == 0


def test_refused_without_the_opt_in_and_built_with_it():
    with pytest.raises(NotImplementedError, match="natten_kernel_size") as e:
        _build(**PLAIN)
    assert "allow_natten=True" in str(e.value) and '"allow_natten": true' in str(e.value)          # the keyword and the config key
    assert _build(**PLAIN, allow_natten=True).transformer.natten_kernel_size == 33
    assert _build(**cases.SMALL_DIT, allow_natten=True).transformer.natten_kernel_size == 0          # the opt-in alone changes nothing
    # reference :479 tests the value's truth: None and 0 are full attention (0 is refused without the opt-in, as before)
    for off in (None, 0):
        assert _build(**dict(cases.SMALL_DIT, attn_kwargs={"natten_kernel_size": off}), allow_natten=True).transformer.natten_kernel_size == 0
    with pytest.raises(NotImplementedError, match="natten_kernel_size"):
        _build(**dict(cases.SMALL_DIT, attn_kwargs={"natten_kernel_size": 0}))


@pytest.mark.parametrize("k", [4, 1, -3, 32])
def test_kernel_sizes_natten_rejects(k):
    with pytest.raises(ValueError, match="natten_kernel_size"):
        _build(**dict(PLAIN, attn_kwargs={"natten_kernel_size": k}), allow_natten=True)


def test_refusals_with_a_reason():
    A = dict(allow_natten=True, allow_causal=True, allow_head_widths=True)
    with pytest.raises(NotImplementedError, match=r"natten_kernel_size.*cross-attention") as e:
        _build(**dict(cases.SMALL_DIT, attn_kwargs={"natten_kernel_size": 7}), **A)
    assert "cond_token_dim" in str(e.value)
    with pytest.raises(NotImplementedError, match=r"natten_kernel_size.*causal"):
        _build(**dict(PLAIN, causal=True), **A)
    for heads, width in ((2, 128), (8, 32)):
        with pytest.raises(NotImplementedError, match=r"natten_kernel_size.*dim_heads") as e:
            _build(**dict(PLAIN, num_heads=heads), **A)
        assert "follow-up" in str(e.value) and str(width) in str(e.value)
    with pytest.raises(NotImplementedError, match=r"natten_kernel_size.*dim_heads"):
        _build(**dict(PLAIN, embed_dim=384, num_heads=4), **A)          # 96


def test_operand_formats():
    m = _build(**PLAIN, **OPT)
    for dtype in ("fp8", "fp8-all"):
        with pytest.raises(NotImplementedError, match=r"natten_kernel_size.*gemm_dtype"):
            m.set_gemm_dtype(dtype)
    assert m.set_gemm_dtype("bf16").set_gemm_dtype("fp32x").set_gemm_dtype("fp16").gemm_dtype == "fp16"
    m.set_block_gemm_dtypes(["fp16", "bf16", "fp16"]).set_block_gemm_dtypes(None)
    m.set_layernorm_fusion(False).set_cross_attention_fusion(False)


def test_a_sequence_shorter_than_the_kernel_is_a_value_error_before_any_launch():
    """forward and denoise check prepend rows + global token + tokens on the host (no plan is built: this runs without a device)."""
    m = _build(**PLAIN, **OPT)
    with pytest.raises(ValueError, match=r"27 rows.*natten_kernel_size=33"):
        m(torch.zeros(2, 64, 26), torch.zeros(2))
    with pytest.raises(ValueError, match=r"32 rows"):
        m(torch.zeros(2, 64, 27), torch.zeros(2), prepend_cond=torch.zeros(2, 4, NC.PREPEND_DIM))
    m._check_seq_len(28, 4)          # 33 rows fit
    m._gen_prepend_len = 2
    with pytest.raises(ValueError, match=r"natten_kernel_size=33"):
        m.denoise(torch.zeros(2, 64, 29), 1.0)
    p = _build(**NC.CONFIGS["patch2"], **OPT)
    with pytest.raises(ValueError, match=r"32 rows"):
        p._check_seq_len(54, 4)          # the window counts tokens: 4 + 1 + 27
    a = _build(**NC.CONFIGS["adaln"], **OPT)
    with pytest.raises(ValueError, match=r"32 rows"):
        a._check_seq_len(32, 0)          # no global token under adaLN
    a._check_seq_len(33, 0)


def test_generate_checks_the_length_before_sampling():
    import inspect
    from stable_audio_tools.inference import generation
    src = inspect.getsource(generation.generate_diffusion_cond)
    assert src.index("_check_seq_len") < src.index("torch.randn")


def test_the_kernel_size_is_part_of_the_plan_options():
    import inspect
    from stable_audio_tools.models.dit import DiffusionTransformer
    src = inspect.getsource(DiffusionTransformer._ensure_plan)
    assert "self.transformer.natten_kernel_size" in src and "sat_dit_plan_set_neighborhood_attention" in src


def _natten_config(**more):
    """The reduced SA-Open config without cross-attention (the timing numbers stay as global conditioning) and with a window of 7."""
    cfg = model_config(attn_kwargs={"natten_kernel_size": 7}, cond_token_dim=0, **more)
    cfg["model"]["diffusion"]["cross_attention_cond_ids"] = []
    return cfg


def test_config_key_and_command_line_flag(monkeypatch):
    """DiTWrapper passes "allow_natten": true of model.diffusion.config through; generate.py --allow-natten writes the key and is an error
    with --model-name."""
    import stable_audio_tools as S
    from stable_audio_tools.models import _init
    keys = dict(attn_kwargs={"natten_kernel_size": 7}, cond_token_dim=0)
    with _init.skip_init():
        with pytest.raises(NotImplementedError, match="allow_natten"):
            S.create_model_from_config(_natten_config())
        assert S.create_model_from_config(_natten_config(allow_natten=True)).model.model.transformer.natten_kernel_size == 7
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "friendly-stable-audio-tools_amd"))
    import generate as G
    base = ["generate.py", "--output-dir", "o", "--cond-yaml-path", "c"]
    monkeypatch.setattr(sys, "argv", base)
    assert "allow_natten" not in G.apply_config_flags(G.get_args(), model_config(**keys))["model"]["diffusion"]["config"]
    monkeypatch.setattr(sys, "argv", base + ["--allow-natten"])
    assert G.apply_config_flags(G.get_args(), model_config(**keys))["model"]["diffusion"]["config"]["allow_natten"] is True
    monkeypatch.setattr(sys, "argv", base + ["--allow-natten", "--model-name", "some/model"])
    with pytest.raises(SystemExit):
        G.get_args()


# ------------------------------------------------------------------------------- the C ABI
def _plan(*cfg, head_widths=0):
    from stable_audio_tools import _hip
    lib = _hip.lib()
    plan = ctypes.c_void_p()
    c = _hip.SatDitCfg(*cfg)
    if head_widths:
        o = _hip.SatDitCreateOptions(1)
        rc = lib.sat_dit_plan_create_ex(ctypes.byref(c), ctypes.sizeof(c), ctypes.byref(o), ctypes.sizeof(o), ctypes.byref(plan))
    else:
        rc = lib.sat_dit_plan_create_sized(ctypes.byref(c), ctypes.sizeof(c), ctypes.byref(plan))
    assert rc == 0, lib.sat_last_error()
    return _hip, lib, plan


def _set(lib, plan, o, size=None):
    rc = lib.sat_dit_plan_set_neighborhood_attention(plan, ctypes.byref(o), ctypes.sizeof(o) if size is None else size)
    return rc, (lib.sat_last_error() if rc else b"")


NO_CROSS = (64, 256, 2, 4, 0, 0, 96, 128)          # io, embed, depth, heads, cond_token_dim, cond_embed_dim, global_cond_dim, max_seq_len


def test_entry_point_validates_without_gpu():
    _hip, lib, plan = _plan(*NO_CROSS)
    O = _hip.SatDitNeighborhoodOptions
    try:
        assert ctypes.sizeof(O) == 4 and lib.sat_version() == 6 and ctypes.sizeof(_hip.SatDitCfg) == 56
        assert ctypes.sizeof(_hip.SatDitAttentionOptions) == 4          # the pinned sizes
        for ok in (7, 0, 255, 3):
            assert _set(lib, plan, O(ok)) == (0, b""), ok
        for size in (0, 3, 8):
            rc, msg = _set(lib, plan, O(7), size)
            assert rc == INVALID and b"sat_dit_neighborhood_options" in msg, (size, rc, msg)
        for value in (4, 1, -1, -7, 256):
            rc, msg = _set(lib, plan, O(value))
            assert rc == INVALID and b"kernel_size" in msg, (value, rc, msg)
        assert lib.sat_dit_plan_set_neighborhood_attention(plan, None, 4) == INVALID
        assert lib.sat_dit_plan_set_neighborhood_attention(None, ctypes.byref(O(7)), 4) == INVALID
    finally:
        lib.sat_dit_plan_destroy(plan)


@pytest.mark.parametrize("cfg, head_widths, why", [
    ((64, 256, 2, 4, 128, 128, 96, 128), 0, b"cross-attention"),
    ((64, 256, 2, 4, 0, 0, 96, 128, 0, 1), 0, b"fp8"),
    ((64, 256, 2, 2, 0, 0, 96, 128), 0, b"dim_heads 128"),
    ((64, 256, 2, 8, 0, 0, 96, 128), 1, b"dim_heads 32"),
    ((64, 384, 2, 4, 0, 0, 96, 128), 1, b"dim_heads 96"),
], ids=["cross-attention", "e4m3", "hd128", "hd32", "hd96"])
def test_entry_point_unsupported_reasons(cfg, head_widths, why):
    _hip, lib, plan = _plan(*cfg, head_widths=head_widths)
    try:
        rc, msg = _set(lib, plan, _hip.SatDitNeighborhoodOptions(7))
        assert rc == UNSUPPORTED and b"natten_kernel_size" in msg and why in msg, (rc, msg)
        assert _set(lib, plan, _hip.SatDitNeighborhoodOptions(0)) == (0, b"")          # the default passes on every plan
    finally:
        lib.sat_dit_plan_destroy(plan)


def test_entry_point_and_causal_refuse_each_other():
    _hip, lib, plan = _plan(*NO_CROSS)
    try:
        a1, a0 = _hip.SatDitAttentionOptions(1), _hip.SatDitAttentionOptions(0)
        assert lib.sat_dit_plan_set_attention_options(plan, ctypes.byref(a1), 4) == 0
        rc, msg = _set(lib, plan, _hip.SatDitNeighborhoodOptions(7))
        assert rc == UNSUPPORTED and b"natten_kernel_size" in msg and b"causal" in msg
        assert lib.sat_dit_plan_set_attention_options(plan, ctypes.byref(a0), 4) == 0
        assert _set(lib, plan, _hip.SatDitNeighborhoodOptions(7)) == (0, b"")
        assert lib.sat_dit_plan_set_attention_options(plan, ctypes.byref(a1), 4) == UNSUPPORTED and b"neighbourhood" in lib.sat_last_error()
        assert lib.sat_dit_plan_set_attention_options(plan, ctypes.byref(a0), 4) == 0
    finally:
        lib.sat_dit_plan_destroy(plan)


def test_after_finalize_is_a_state_error():
    """plan_finalize needs a device; the state check is the first thing behind the size check, so the text of the entry point pins it here and
    tests/test_gpu_dit_natten.py makes the call on a finalized plan."""
    text = open(os.path.join(CSRC, "dit_plan.hip")).read()
    body = text[text.index('extern "C" int sat_dit_plan_set_neighborhood_attention'):]
    body = body[:body.index("\n}\n")]
    assert re.search(r"SAT_CHECK_ARG\(!p->finalized, SAT_E_STATE", body)
    assert body.index("SAT_E_STATE") < body.index("o->kernel_size")


def test_unit_entries_validate_without_gpu():
    from stable_audio_tools import _hip
    lib = _hip.lib()
    p = ctypes.c_void_p(1 << 20)          # never dereferenced: every call below fails its checks
    for fn in (lib.sat_attention_window_bf16, lib.sat_attention_window_f16):
        for ks in (4, 1, 0, -3, 79):          # even, too small, longer than the sequence
            assert fn(p, p, p, p, 1, 2, 2, 78, 128, 128, ks, 1.0, None) == INVALID and b"kernel_size" in lib.sat_last_error(), ks
        for scale in (0.0, -1.0, float("nan"), float("inf")):
            assert fn(p, p, p, p, 1, 2, 2, 78, 128, 128, 7, scale, None) == INVALID and b"scale" in lib.sat_last_error(), scale
        assert fn(p, p, p, p, 1, 2, 2, 78, 128, 96, 7, 1.0, None) == INVALID             # s_pad_k % 64
        assert fn(p, p, p, p, 1, 2, 2, 78, 64, 128, 7, 1.0, None) == INVALID             # s_pad_q % 128
        assert fn(p, p, p, p, 1, 2, 2, 126, 128, 128, 7, 1.0, None) == INVALID           # s_pad_k >= s + 3
        assert fn(p, p, p, p, 1, 3, 2, 78, 128, 128, 7, 1.0, None) == INVALID            # 3 query heads over 2 kv heads
        assert fn(p, ctypes.c_void_p((1 << 20) + 8), p, p, 1, 2, 2, 78, 128, 128, 7, 1.0, None) == INVALID          # alignment
        assert fn(p, p, p, p, 1, 2, 2, 0, 128, 128, 7, 1.0, None) == INVALID
        assert fn(None, p, p, p, 1, 2, 2, 78, 128, 128, 7, 1.0, None) == INVALID
    f32 = lib.sat_attention_f32_window
    for ks in (4, 1, 9):
        assert f32(p, p, p, p, 1, 2, 2, 8, ks, 1.0, None) == INVALID and b"kernel_size" in lib.sat_last_error(), ks
    assert f32(p, p, p, p, 1, 3, 2, 8, 7, 1.0, None) == INVALID
    assert f32(p, p, p, p, 1, 2, 2, 0, 7, 1.0, None) == INVALID
    assert f32(p, p, p, p, 1, 2, 2, 8, 7, 0.0, None) == INVALID and b"scale" in lib.sat_last_error()


# ------------------------------------------------------------------------------- the ranges
def test_window_ranges_agree_with_brute_force(tmp_path):
    line = NU.check_ranges(str(tmp_path), 700)
    print("\n" + line)
    skipped, edge, full = (int(x) for x in re.search(r"skipped (\d+) edge (\d+) full (\d+)", line).groups())
    walked, of = (int(x) for x in re.search(r"tiles walked (\d+) of (\d+)", line).groups())
    assert skipped > 0 and edge > 0 and full > 0 and walked < of


def test_the_kernels_take_their_ranges_from_the_header():
    text = open(os.path.join(CSRC, "attention_window.hip")).read()
    for c in ("attnw::first_tile", "attnw::last_tile", "attnw::wave_range", "attnw::key_lo", "attnw::union_lo", "attnw::union_hi"):
        assert c in text, c
    assert "attn::MASK_WINDOW" in text and "attnw::block_class" in open(os.path.join(CSRC, "attn_core.h")).read()      # the shared step classes the blocks


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
def test_window_kernels_keep_their_register_budgets(defines, tmp_path):
    """The 16-bit kernel stays within 128 VGPRs (four waves per SIMD at 512 threads, two workgroups per CU) with no spill and no scratch in
    both builds; the fp32 kernel exists in the bf16 build only and spills no vector register."""
    meta = _kernels("attention_window.hip", defines, str(tmp_path))
    win = {n: m for n, m in meta.items() if "attention_window_kernel" in n}
    assert len(win) == 1, sorted(meta)
    for n, m in win.items():
        assert m["vgpr_count"] <= 128 and m["vgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, (n, m)
    f32 = {n: m for n, m in meta.items() if "attention_window_f32_kernel" in n}
    assert len(f32) == (0 if defines else 1) and len(meta) == len(win) + len(f32), sorted(meta)
    for n, m in f32.items():
        assert m["vgpr_spill_count"] == 0, (n, m)
    print("\n" + "\n".join(f"{n}: {m['vgpr_count']} VGPRs" for n, m in {**win, **f32}.items()))


# ------------------------------------------------------------------------------- the stand-in and the reference
def _masked_softmax(q, k, v, ks, scale=1.0):
    """float64, from the definition: every (i, j) logit, -inf outside the window, softmax, times v"""
    n = q.shape[-2]
    i, j = torch.arange(n)[:, None], torch.arange(n)[None, :]
    lo = torch.minimum(torch.clamp(i - ks // 2, min=0), torch.tensor(n - ks))
    d = torch.einsum("bhid,bhjd->bhij", q.double(), k.double()) * scale
    d = d.masked_fill(~((j >= lo) & (j < lo + ks))[None, None], float("-inf"))
    return torch.softmax(d, dim=-1) @ v.double()


@pytest.mark.parametrize("n,ks", [(9, 3), (33, 7), (69, 33), (69, 69), (70, 69), (301, 129)])
def test_the_stand_in_is_a_masked_softmax(n, ks):
    rand = lambda shape, sd: torch.randn(shape, generator=torch.Generator().manual_seed(sd), dtype=torch.float64)
    q, k, v = rand((2, 3, n, 16), 1), rand((2, 3, n, 16), 2), rand((2, 3, n, 16), 3)
    f = natten_standin.functional
    attn = f.natten1dqk(q, k, kernel_size=ks, dilation=1)
    assert attn.shape == (2, 3, n, ks)
    # the logits are the window's, in key order, unscaled
    st = natten_standin.window_start(n, ks)
    for i in (0, 1, ks // 2, ks // 2 + 1, n // 2, n - ks // 2 - 1, n - 1):
        assert torch.allclose(attn[:, :, i], torch.einsum("bhd,bhkd->bhk", q[:, :, i], k[:, :, st[i]:st[i] + ks]), rtol=1e-12, atol=1e-12), i
    assert st[0] == 0 and st[n - 1] == n - ks and (st[1:] >= st[:-1]).all() and st[n // 2] == min(max(n // 2 - ks // 2, 0), n - ks)
    out = f.natten1dav(torch.softmax(attn, dim=-1), v, kernel_size=ks, dilation=1)
    assert rel_l2(out, _masked_softmax(q, k, v, ks)) < 1e-12


def test_the_stand_in_raises_where_natten_does():
    f = natten_standin.functional
    q = torch.zeros(1, 1, 8, 4)
    for ks in (4, 1, 0, -3, 9):
        with pytest.raises(ValueError):
            f.natten1dqk(q, q, kernel_size=ks, dilation=1)
    with pytest.raises(ValueError):
        f.natten1dqk(q, torch.zeros(1, 1, 9, 4), kernel_size=3, dilation=1)          # cross-attention: q and k of different lengths
    with pytest.raises(ValueError):
        f.natten1dav(torch.zeros(1, 1, 8, 5), q, kernel_size=3, dilation=1)
    with pytest.raises(ValueError):
        f.natten1dqk(q, q, kernel_size=3, dilation=2)


def test_reference_with_the_whole_sequence_is_its_full_attention_with_q_times_8():
    """The reference's NATTEN branch does not scale its logits.  adaln_k65_cfg1_T65 is K == n (65 rows under adaLN, no global token): every
    query sees every key, and the REFERENCE's output (the golden) is what the restated full-attention model (oracle.dit, pinned against the
    reference's own goldens by the oracle's tests) gives on the same weights with the q rows of every to_qkv multiplied by
    dim_heads ** 0.5 = 8 -- and not what it gives on the weights as they are."""
    import dit_family
    from oracle import dit as odit
    name = "adaln_k65_cfg1_T65"
    cfg = NC.CONFIGS[NC.CASES[name][0]]
    assert NC.KERNEL[NC.CASES[name][0]] == 65 == NC.CASES[name][1] and cfg["global_cond_type"] == "adaLN"
    sd = NC.FAMILY.weights("adaln_k65", _build(**cfg, **OPT).state_dict(), 0)
    x, t, kw = dit_family.case_inputs(NC.FAMILY, name)
    want = cases.load(NC.FAMILY.stem)[name]
    d = cfg["embed_dim"]
    sd8 = {k: (torch.cat([v[:d] * 8.0, v[d:]]) if k.endswith("self_attn.to_qkv.weight") else v) for k, v in sd.items()}
    run = lambda w: odit.dit_forward(w, x, t, None, kw["global_embed"], cfg["depth"], cfg["num_heads"], adaln=True)
    with torch.no_grad():
        e8, e1 = rel_l2(run(sd8), want), rel_l2(run(sd), want)
    print(f"\n[{name}] reference (K == n) vs full attention with q * 8: {e8:.2e}; vs full attention as it is: {e1:.2e}")
    assert e8 < 1e-5 and e1 > 5e-2


# ------------------------------------------------------------------------------- the gates bite
def _gates(fmt, got, want, h):
    """The unit gates of tests/test_gpu_dit_natten.py on a [b, s, h * 64] result; returns the failure text or None."""
    b, s, _ = want.shape
    try:
        assert_close("window attention", got, want, fmt.tol(5e-3))
        assert_close_sliced("window attention per (sequence, query, head)", got.view(b, s, h, -1), want.view(b, s, h, -1), fmt.tol(5e-3), (0, 1, 2),
                            fmt.round)
    except AssertionError as e:
        return str(e)
    return None


@pytest.mark.parametrize("fmt", FORMATS, ids=repr)
@pytest.mark.parametrize("ks", [7, 65])
def test_unit_gates_pass_the_reference_and_reject_the_mistakes(fmt, ks):
    """At b = 4, s = 301 (key shifts 0..3, two workgroups) on the unscaled tensors: the float32 evaluation of the matched-rounding reference,
    rounded to the output format, passes; each mistake of dit_natten_units.MISTAKES does not."""
    b, h, kvh, s = 4, 4, 2, 301
    q, k, v, scale = NU.unit_tensors(fmt, b, h, kvh, s, unscaled=True)
    want = NU.window_attention(q, k, v, ks, scale, rnd=fmt.round)
    assert _gates(fmt, fmt.round(want.float()), want.float(), h) is None
    assert rel_l2(want, NU.window_attention(q, k, v, ks, scale)) < fmt.tol(1e-2)          # matched rounding against exact: the third gate of the GPU test
    for mistake in NU.MISTAKES:
        wrong = fmt.round(NU.window_attention(q, k, v, ks, scale, rnd=fmt.round, mistake=mistake).float())
        msg = _gates(fmt, wrong, want.float(), h)
        assert msg is not None, f"{mistake}: the gates accept it (whole-tensor rel-L2 {rel_l2(wrong, want):.3e})"


def test_the_unit_reference_is_the_stand_in():
    """dit_natten_units.window_attention with scale 1 equals the softmax over natten_standin's logits, and with K = s and scale 1 / 8 it is
    oracle.dit.attention_core."""
    from oracle import dit as odit
    fmt = FORMATS[1]
    q, k, v, scale = NU.unit_tensors(fmt, 2, 4, 2, 70, unscaled=True)
    kk, vv = (t.float().repeat_interleave(2, dim=1) for t in (k, v))
    f = natten_standin.functional
    for ks in (7, 33, 69):
        attn = torch.softmax(f.natten1dqk(q.float(), kk, kernel_size=ks), dim=-1)
        want = odit._merge(f.natten1dav(attn, vv, kernel_size=ks))
        assert rel_l2(NU.window_attention(q, k, v, ks, scale), want) < 1e-5
    q, k, v, scale = NU.unit_tensors(fmt, 2, 4, 2, 69, unscaled=False)
    assert scale == 0.125
    want = odit._merge(odit.attention_core(q.float(), k.float(), v.float()))          # (float32: its own rounding is the bound)
    assert rel_l2(NU.window_attention(q, k, v, 69, scale), want) < 1e-6
