"""Neighbourhood-attention DiTs at 128-, 32- and 96-channel heads (attn_kwargs natten_kernel_size behind allow_natten and
allow_natten_head_widths), host side: refused without the new opt-in with what was raised before plus the name of the opt-in, built with
it under the reference's parameter names, the config key and the command-line flag arrive, what stays refused is refused with a reason,
sat_dit_plan_set_neighborhood_attention_hdw and the three unit entries validate before they touch a device while the old entry answers
the staged plans what it answered, csrc/attn_window.h agrees with brute force at the 128-key tile of W = 32, the kernels of
csrc/attention_hdw_window.hip keep their register budgets, and -- on the float64 references the GPU tests compare against -- the unit gates
of tests/test_gpu_dit_natten_hdw.py reject the mistakes such kernels can make, among them one that only a four-block tile allows.  No GPU."""
import ctypes
import inspect
import os
import re
import subprocess
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import dit_natten_hdw_cases as HC  # noqa: E402
import dit_natten_hdw_units as HU  # noqa: E402
from dit_family_host import build as _build, check_state_dict_keys, model_config  # noqa: E402
from util import FORMATS, assert_close, assert_close_sliced, rel_l2  # noqa: E402

CSRC = os.path.join(os.path.dirname(HERE), "friendly-stable-audio-tools_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
OPT = HC.FAMILY.product_kwargs
INVALID, UNSUPPORTED = -1, -2
PLAIN = {w: HC.CONFIGS[f"hd{w}_k33"] for w in HU.WIDTHS}


# ------------------------------------------------------------------------------- the modules
@pytest.mark.parametrize("name", sorted(HC.CONFIGS))
def test_dit_state_dict_matches_reference(name):
    """The keys are those of the reference's module, and of the same model without the option."""
    m, got = check_state_dict_keys(HC.FAMILY, name)
    assert m.transformer.natten_kernel_size == HC.KERNEL[name] and m.transformer.dim_heads == HC.WIDTH[name]
    plain = _build(**HC.without_natten(HC.CONFIGS[name]), allow_head_widths=True, allow_patch_size=True)
    assert {k: list(v.shape) for k, v in plain.state_dict().items()} == got and plain.transformer.natten_kernel_size == 0


@pytest.mark.parametrize("w", HU.WIDTHS)
def test_refused_without_the_opt_in_and_built_with_it(w):
    """Without allow_natten_head_widths: the sentence that was raised before, and behind it the keyword and the config key."""
    before = dict(allow_natten=True, allow_head_widths=True)
    with pytest.raises(NotImplementedError, match=r"natten_kernel_size.*dim_heads") as e:
        _build(**PLAIN[w], **before)
    msg = str(e.value)
    assert "follow-up" in msg and str(w) in msg and "allow_natten_head_widths=True" in msg and '"allow_natten_head_widths": true' in msg
    m = _build(**PLAIN[w], **before, allow_natten_head_widths=True)
    assert m.transformer.natten_kernel_size == 33 and m.transformer.dim_heads == w and m.allow_natten_head_widths
    assert all(l.self_attn.natten_kernel_size == 33 for l in m.transformer.layers)
    # the new opt-in replaces neither of the two others
    with pytest.raises(NotImplementedError, match="allow_natten"):
        _build(**PLAIN[w], allow_head_widths=True, allow_natten_head_widths=True)
    if w != 128:
        with pytest.raises(NotImplementedError, match="allow_head_widths"):
            _build(**PLAIN[w], allow_natten=True, allow_natten_head_widths=True)
    # and alone it changes nothing
    assert _build(**HC.without_natten(PLAIN[128]), allow_natten_head_widths=True).transformer.natten_kernel_size == 0


def test_what_stays_refused():
    A = dict(OPT, allow_causal=True, allow_block_options=True, allow_conv_ff=True)
    for w in HU.WIDTHS:
        with pytest.raises(NotImplementedError, match=r"natten_kernel_size.*cross-attention"):
            _build(**dict(PLAIN[w], cond_token_dim=128 if w != 96 else 192), **A)
        with pytest.raises(NotImplementedError, match=r"natten_kernel_size.*causal"):
            _build(**dict(PLAIN[w], causal=True), **A)
        for k in (4, 1, -3, 32):
            with pytest.raises(ValueError, match="natten_kernel_size"):
                _build(**dict(PLAIN[w], attn_kwargs={"natten_kernel_size": k}), **A)
        for more in (dict(conformer=True), dict(remove_norms=True), dict(ff_kwargs={"glu": False}), dict(ff_kwargs={"use_conv": True})):
            with pytest.raises(NotImplementedError, match=rf"dim_heads={w}"):
                _build(**dict(PLAIN[w], **more), **A)


@pytest.mark.parametrize("w", HU.WIDTHS)
def test_operand_formats(w):
    m = _build(**PLAIN[w], **OPT)
    for dtype in ("fp8", "fp8-all"):
        with pytest.raises(NotImplementedError, match="gemm_dtype"):
            m.set_gemm_dtype(dtype)
    if w == 128:
        with pytest.raises(NotImplementedError, match=r"dim_heads=128.*gemm_dtype"):
            m.set_gemm_dtype("fp32x")
    else:
        m.set_gemm_dtype("fp32x")
    assert m.set_gemm_dtype("bf16").set_gemm_dtype("fp16").gemm_dtype == "fp16"
    m.set_block_gemm_dtypes(["fp16", "bf16", "fp16"]).set_block_gemm_dtypes(None)


def test_a_sequence_shorter_than_the_kernel_is_a_value_error_before_any_launch():
    """forward and denoise check prepend rows + global token + tokens on the host (no plan is built: this runs without a device)."""
    m = _build(**PLAIN[32], **OPT)
    with pytest.raises(ValueError, match=r"27 rows.*natten_kernel_size=33"):
        m(torch.zeros(2, 64, 26), torch.zeros(2))
    with pytest.raises(ValueError, match=r"32 rows"):
        m(torch.zeros(2, 64, 27), torch.zeros(2), prepend_cond=torch.zeros(2, 4, HC.PREPEND_DIM))
    m._check_seq_len(28, 4)          # 33 rows fit
    m._gen_prepend_len = 2
    with pytest.raises(ValueError, match=r"natten_kernel_size=33"):
        m.denoise(torch.zeros(2, 64, 29), 1.0)
    p = _build(**HC.CONFIGS["hd128_patch2"], **OPT)
    with pytest.raises(ValueError, match=r"32 rows"):
        p._check_seq_len(54, 4)          # the window counts tokens: 4 + 1 + 27
    a = _build(**HC.CONFIGS["hd96_adaln"], **OPT)
    with pytest.raises(ValueError, match=r"32 rows"):
        a._check_seq_len(32, 0)          # no global token under adaLN
    a._check_seq_len(33, 0)


def test_only_a_model_that_opted_in_calls_the_new_entry():
    """_ensure_plan picks the entry from the opt-in and the head width; every other model makes the call it made."""
    from stable_audio_tools.models.dit import DiffusionTransformer
    src = inspect.getsource(DiffusionTransformer._ensure_plan)
    assert "self.allow_natten_head_widths and self.transformer.dim_heads != 64" in src
    assert "sat_dit_plan_set_neighborhood_attention_hdw if hdw else lib.sat_dit_plan_set_neighborhood_attention" in src
    import dit_natten_cases as NC
    assert not _build(**NC.CONFIGS["k33"], **NC.FAMILY.product_kwargs).allow_natten_head_widths


def test_config_key_and_command_line_flag(monkeypatch):
    """DiTWrapper passes "allow_natten_head_widths": true of model.diffusion.config through; generate.py --allow-natten-head-widths writes
    the key and is an error with --model-name."""
    import stable_audio_tools as S
    from stable_audio_tools.models import _init
    keys = dict(attn_kwargs={"natten_kernel_size": 7}, cond_token_dim=0, num_heads=2, allow_natten=True)

    def config(**more):
        cfg = model_config(**keys, **more)
        cfg["model"]["diffusion"]["cross_attention_cond_ids"] = []
        return cfg

    with _init.skip_init():
        with pytest.raises(NotImplementedError, match="allow_natten_head_widths"):
            S.create_model_from_config(config())
        tr = S.create_model_from_config(config(allow_natten_head_widths=True)).model.model.transformer
        assert tr.natten_kernel_size == 7 and tr.dim_heads == 128
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "friendly-stable-audio-tools_amd"))
    import generate as G
    base = ["generate.py", "--output-dir", "o", "--cond-yaml-path", "c"]
    monkeypatch.setattr(sys, "argv", base)
    assert "allow_natten_head_widths" not in G.apply_config_flags(G.get_args(), config())["model"]["diffusion"]["config"]
    monkeypatch.setattr(sys, "argv", base + ["--allow-natten-head-widths"])
    assert G.apply_config_flags(G.get_args(), config())["model"]["diffusion"]["config"]["allow_natten_head_widths"] is True
    monkeypatch.setattr(sys, "argv", base + ["--allow-natten-head-widths", "--model-name", "some/model"])
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


def _set(fn, plan, o, size=None):
    from stable_audio_tools import _hip
    rc = fn(plan, ctypes.byref(o), ctypes.sizeof(o) if size is None else size)
    return rc, (_hip.lib().sat_last_error() if rc else b"")


# io, embed, depth, heads, cond_token_dim, cond_embed_dim, global_cond_dim, max_seq_len; create_ex for 32 and 96
PLANS = {64: ((64, 256, 2, 4, 0, 0, 96, 128), 0), 128: ((64, 256, 2, 2, 0, 0, 96, 128), 0), 32: ((64, 256, 2, 8, 0, 0, 96, 128), 1),
         96: ((64, 384, 2, 4, 0, 0, 96, 128), 1)}


@pytest.mark.parametrize("w", sorted(PLANS))
def test_new_entry_validates_without_gpu(w):
    cfg, hw = PLANS[w]
    _hip, lib, plan = _plan(*cfg, head_widths=hw)
    O, new, old = _hip.SatDitNeighborhoodOptions, lib.sat_dit_plan_set_neighborhood_attention_hdw, lib.sat_dit_plan_set_neighborhood_attention
    try:
        assert ctypes.sizeof(O) == 4 and lib.sat_version() == 6          # the same struct, the same ABI version
        for ok in (7, 0, 255):
            assert _set(new, plan, O(ok)) == (0, b""), ok
        for size in (0, 3, 8):
            rc, msg = _set(new, plan, O(7), size)
            assert rc == INVALID and b"sat_dit_neighborhood_options" in msg, (size, rc, msg)
        for value in (4, 1, -1, -7, 256):
            rc, msg = _set(new, plan, O(value))
            assert rc == INVALID and b"kernel_size" in msg and b"_hdw" in msg, (value, rc, msg)
        assert new(plan, None, 4) == INVALID and new(None, ctypes.byref(O(7)), 4) == INVALID
        # causal and the window refuse each other through the new entry as through the old one
        a1, a0 = _hip.SatDitAttentionOptions(1), _hip.SatDitAttentionOptions(0)
        assert _set(new, plan, O(0)) == (0, b"") and lib.sat_dit_plan_set_attention_options(plan, ctypes.byref(a1), 4) == 0
        rc, msg = _set(new, plan, O(7))
        assert rc == UNSUPPORTED and b"natten_kernel_size" in msg and b"causal" in msg
        assert lib.sat_dit_plan_set_attention_options(plan, ctypes.byref(a0), 4) == 0 and _set(new, plan, O(7)) == (0, b"")
        assert lib.sat_dit_plan_set_attention_options(plan, ctypes.byref(a1), 4) == UNSUPPORTED and b"neighbourhood" in lib.sat_last_error()
        # the old entry answers a staged plan what it answered
        assert _set(new, plan, O(0)) == (0, b"")
        rc, msg = _set(old, plan, O(7))
        if w == 64:
            assert (rc, msg) == (0, b"")
        else:
            assert rc == UNSUPPORTED and b"natten_kernel_size" in msg and f"dim_heads {w}".encode() in msg and b"follow-up" in msg
    finally:
        lib.sat_dit_plan_destroy(plan)


@pytest.mark.parametrize("cfg, head_widths, why", [
    ((64, 256, 2, 2, 128, 128, 96, 128), 0, b"cross-attention"),
    ((64, 256, 2, 8, 128, 128, 96, 128), 1, b"cross-attention"),
    ((64, 256, 2, 4, 0, 0, 96, 128, 0, 1), 0, b"fp8"),
], ids=["cross-attention hd128", "cross-attention hd32", "e4m3"])
def test_new_entry_unsupported_reasons(cfg, head_widths, why):
    _hip, lib, plan = _plan(*cfg, head_widths=head_widths)
    try:
        rc, msg = _set(lib.sat_dit_plan_set_neighborhood_attention_hdw, plan, _hip.SatDitNeighborhoodOptions(7))
        assert rc == UNSUPPORTED and b"natten_kernel_size" in msg and why in msg, (rc, msg)
        assert _set(lib.sat_dit_plan_set_neighborhood_attention_hdw, plan, _hip.SatDitNeighborhoodOptions(0)) == (0, b"")
    finally:
        lib.sat_dit_plan_destroy(plan)


def test_new_entry_after_finalize_is_a_state_error():
    """plan_finalize needs a device: the text of the entry point pins the order here, tests/test_gpu_dit_natten_hdw.py makes the call."""
    text = open(os.path.join(CSRC, "dit_plan.hip")).read()
    body = text[text.index('extern "C" int sat_dit_plan_set_neighborhood_attention_hdw'):]
    body = body[:body.index("\n}\n")]
    assert re.search(r"SAT_CHECK_ARG\(!p->finalized, SAT_E_STATE", body) and body.index("SAT_E_STATE") < body.index("o->kernel_size")
    assert "sat_launch_attention_hdw_window && sat_launch_attention_f32_window_w" in body          # a build without the kernels answers UNSUPPORTED


def test_unit_entries_validate_without_gpu():
    from stable_audio_tools import _hip
    lib = _hip.lib()
    p = ctypes.c_void_p(1 << 20)          # never dereferenced: every call below fails its checks
    for fn in (lib.sat_attention_hdw_window_bf16, lib.sat_attention_hdw_window_f16):
        for w, pad in ((32, 128), (96, 128), (128, 128)):
            for ks in (4, 1, 0, -3, 79):          # even, too small, longer than the sequence
                assert fn(p, p, p, p, 1, 2, 2, w, 78, 128, pad, ks, None) == INVALID and b"kernel_size" in lib.sat_last_error(), (w, ks)
            assert fn(p, p, p, p, 1, 2, 2, w, 78, 64, pad, 7, None) == INVALID             # s_pad_q % 128
            assert fn(p, p, p, p, 1, 2, 2, w, 126, 128, 128, 7, None) == INVALID           # s_pad_k >= s + 3
            assert fn(p, p, p, p, 1, 3, 2, w, 78, 128, pad, 7, None) == INVALID            # 3 query heads over 2 kv heads
            assert fn(p, ctypes.c_void_p((1 << 20) + 8), p, p, 1, 2, 2, w, 78, 128, pad, 7, None) == INVALID          # alignment
            assert fn(p, p, p, p, 1, 2, 2, w, 0, 128, pad, 7, None) == INVALID
            assert fn(None, p, p, p, 1, 2, 2, w, 78, 128, pad, 7, None) == INVALID
            assert fn(p, p, p, None, 1, 2, 2, w, 78, 128, pad, 7, None) == INVALID
        assert fn(p, p, p, p, 1, 2, 2, 32, 78, 128, 192, 7, None) == INVALID and b"128" in lib.sat_last_error()          # s_pad_k % 128 at W = 32
        assert fn(p, p, p, p, 1, 2, 2, 96, 78, 128, 96, 7, None) == INVALID                # s_pad_k % 64
        for w in (64, 48, 0, 256):
            assert fn(p, p, p, p, 1, 2, 2, w, 78, 128, 128, 7, None) == UNSUPPORTED and b"dim_heads" in lib.sat_last_error(), w
    f32 = lib.sat_attention_f32_window_w
    for w in (32, 96):
        for ks in (4, 1, 9):
            assert f32(p, p, p, p, 1, 2, 2, w, 8, ks, 1.0, None) == INVALID and b"kernel_size" in lib.sat_last_error(), ks
        assert f32(p, p, p, p, 1, 3, 2, w, 8, 7, 1.0, None) == INVALID
        assert f32(p, p, p, p, 1, 2, 2, w, 0, 7, 1.0, None) == INVALID
        assert f32(None, p, p, p, 1, 2, 2, w, 8, 7, 1.0, None) == INVALID
        assert f32(ctypes.c_void_p((1 << 20) + 4), p, p, p, 1, 2, 2, w, 8, 7, 1.0, None) == INVALID
        assert f32(p, p, p, p, 1, 2, 2, w, 8, 7, 0.0, None) == INVALID and b"scale" in lib.sat_last_error()
    for w in (128, 64, 48):          # 128-channel heads have no fp32 verification mode; 64 has its own launcher
        assert f32(p, p, p, p, 1, 2, 2, w, 8, 7, 1.0, None) == UNSUPPORTED and b"dim_heads" in lib.sat_last_error(), w


# ------------------------------------------------------------------------------- the ranges
def test_window_ranges_agree_with_brute_force_at_both_key_tiles(tmp_path):
    line = HU.check_ranges(str(tmp_path), 700)
    print("\n" + line)
    for kt in (64, 128):
        walked, of, inner, behind = (int(x) for x in re.search(rf"KT {kt}: tiles walked (\d+) of (\d+), inner (\d+), visible behind skipped (\d+)", line).groups())
        assert 0 < walked < of and inner > 0 and behind > 0, kt          # tiles that are neither the first nor the last are walked
    assert int(re.search(r"third block behind skipped (\d+)", line).group(1)) > 0          # what a `break` at a SKIP block would lose at W = 32


def test_the_kernels_take_their_ranges_from_the_header():
    text = open(os.path.join(CSRC, "attention_hdw_window.hip")).read()
    for c in ("attnw::first_tile", "attnw::last_tile", "attnw::wave_range", "attnw::key_lo", "attnw::union_lo", "attnw::union_hi", "attn::MASK_WINDOW",
              "attn::LayoutHdw<W>", "attn::walk3", "attn::store_out", "xcd_remap", "T::KV_TILE"):
        assert c in text, c
    core = open(os.path.join(CSRC, "attn_core.h")).read()
    step = core[core.index("if constexpr (MASK == MASK_WINDOW) {"):]
    assert "if (cls == attnw::SKIP) continue;" in step[:step.index("}")]          # passes over a skipped block, does not end the tile


# ------------------------------------------------------------------------------- the kernels, compiled and inspected
KEYS = ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")


def _kernels(src, defines, tmp):
    out = os.path.join(tmp, "k.s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", os.path.join(CSRC, src), "-o", out] + defines,
                   check=True, capture_output=True)
    meta = {}
    for blk in open(out).read().split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        meta[name] = {k: int(re.search(rf"\.{k}:\s+(\d+)", blk).group(1)) for k in KEYS}
    return meta


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
@pytest.mark.parametrize("defines", [[], ["-DSAT_OPERAND_F16"]], ids=["bf16", "f16"])
def test_hdw_window_kernels_keep_their_register_budgets(defines, tmp_path):
    """Three 16-bit kernels in each build: W = 32 within 128 VGPRs (two workgroups of 512 threads per CU), 96 and 128 within 256, no spill,
    no scratch, static LDS within 64 KiB (none: the ring of 48 or 96 KiB is dynamic).  The two fp32 kernels
    exist in the bf16 build only and spill no vector register -- like attention_window_f32_kernel, whose twin they are, they hold K rows in
    scalar registers and the compiler parks some of those in vector lanes (counted, printed, not a memory spill)."""
    meta = _kernels("attention_hdw_window.hip", defines, str(tmp_path))
    win = {int(re.search(r"attention_hdw_window_kernelILi(\d+)E", n).group(1)): m for n, m in meta.items() if "attention_hdw_window_kernel" in n}
    f32 = {int(re.search(r"attention_hdw_window_f32_kernelILi(\d+)E", n).group(1)): m for n, m in meta.items() if "attention_hdw_window_f32_kernel" in n}
    assert sorted(win) == [32, 96, 128] and sorted(f32) == ([] if defines else [32, 96]) and len(meta) == len(win) + len(f32), sorted(meta)
    print("\n" + "\n".join(f"attention_hdw_window_kernel<{w}>: {m}" for w, m in sorted(win.items())))
    print("\n".join(f"attention_hdw_window_f32_kernel<{w}>: {m}" for w, m in sorted(f32.items())))
    for w, m in win.items():
        assert m["vgpr_count"] <= (128 if w == 32 else 256), (w, m)
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, (w, m)
        assert m["group_segment_fixed_size"] <= 64 * 1024, (w, m)
    for w, m in f32.items():
        assert m["vgpr_spill_count"] == 0 and m["group_segment_fixed_size"] == 0, (w, m)


# ------------------------------------------------------------------------------- the gates bite
def _gates(fmt, got, want, h):
    """The unit gates of tests/test_gpu_dit_natten_hdw.py on a [b, s, h * W] result; returns the failure text or None."""
    b, s, _ = want.shape
    try:
        assert_close("window attention", got, want, fmt.tol(5e-3))
        assert_close_sliced("window attention per (sequence, query, head)", got.view(b, s, h, -1), want.view(b, s, h, -1), fmt.tol(5e-3), (0, 1, 2),
                            fmt.round)
    except AssertionError as e:
        return str(e)
    return None


@pytest.mark.parametrize("fmt", FORMATS, ids=repr)
@pytest.mark.parametrize("w,ks", [(32, 7), (32, 65), (128, 7), (128, 65)])
def test_unit_gates_pass_the_reference_and_reject_the_mistakes(fmt, w, ks):
    """At b = 4, s = 301 (key shifts 0..3, two workgroups, three 128-key tiles at W = 32) on the kernel's unit tensors: the float32 evaluation
    of the matched-rounding reference, rounded to the output format, passes; each mistake of dit_natten_hdw_units.MISTAKES does not --
    "drop_third_block" among them at W = 32."""
    b, h, kvh, s = 4, 4, 2, 301
    _, q_eff, k, v, scale = HU.unit_tensors(fmt, w, b, h, kvh, s)
    want = HU.window_attention(q_eff, k, v, ks, scale, rnd=fmt.round)
    assert _gates(fmt, fmt.round(want.float()), want.float(), h) is None
    assert rel_l2(want, HU.window_attention(q_eff, k, v, ks, scale)) < fmt.tol(1e-2)          # matched rounding against exact: the third gate of the GPU test
    for mistake in HU.MISTAKES:
        if mistake == "drop_third_block" and w != 32:
            continue
        wrong = fmt.round(HU.window_attention(q_eff, k, v, ks, scale, rnd=fmt.round, mistake=mistake).float())
        msg = _gates(fmt, wrong, want.float(), h)
        assert msg is not None, f"W {w} K {ks} {mistake}: the gates accept it (whole-tensor rel-L2 {rel_l2(wrong, want):.3e})"
