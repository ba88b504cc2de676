"""DiTs with 32- and 96-channel attention heads (embed_dim == 32 or 96 times num_heads; reference models/transformer.py:303-308, 517, 737), host
side: refused without ``allow_head_widths`` and built with it under the reference's parameter names and shapes, the operand formats and
block options outside the route still raise with a reason, sat_dit_plan_create_ex admits the two widths and nothing else new, the unit
entries refuse other widths and bad paddings before they touch a device, the LDS tile maps of the attention kernel are bijections free of
bank conflicts, the new kernels keep their register budget without scratch, and -- on float64 restatements of what the GPU tests compare
against -- the gates of tests/test_gpu_dit_head_width.py catch the mistakes such kernels can make.  No GPU."""
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
import dit_head_width_cases as WC  # noqa: E402
import dit_head_width_units as WU  # noqa: E402
from dit_family_host import build as _build, check_state_dict_keys  # noqa: E402
from util import FORMATS, rel_l2, slice_errors  # noqa: E402

CSRC = os.path.join(os.path.dirname(HERE), "friendly-stable-audio-tools_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
OPT = dict(allow_head_widths=True)


# ------------------------------------------------------------------------------- the modules
@pytest.mark.parametrize("name", sorted(WC.CONFIGS))
def test_dit_state_dict_matches_reference(name):
    _, got = check_state_dict_keys(WC.FAMILY, name)
    if WC.CONFIGS[name].get("rotary_pos_emb", True):
        assert got["transformer.rotary_pos_emb.inv_freq"] == [WU.rope_pairs(WC.WIDTH[name])]          # RotaryEmbedding(max(W // 2, 32)): 16 / 24


@pytest.mark.parametrize("name", ["hd32", "hd96"])
def test_refused_without_the_opt_in_and_built_with_it(name):
    with pytest.raises(NotImplementedError, match="dim_heads") as e:
        _build(**WC.CONFIGS[name])
    assert "allow_head_widths=True" in str(e.value) and '"allow_head_widths": true' in str(e.value)          # the keyword and the config key
    m = _build(**WC.CONFIGS[name], **OPT)
    assert m.transformer.dim_heads == WC.WIDTH[name] and m.allow_head_widths


def test_head_counts_follow_the_head_width():
    a = _build(**WC.CONFIGS["hd32"], **OPT).transformer.layers[0]
    assert (a.self_attn.dim_heads, a.self_attn.num_heads, a.cross_attn.num_heads, a.cross_attn.kv_heads) == (32, 8, 8, 4)
    assert tuple(a.cross_attn.to_kv.weight.shape) == (256, 128)          # [2 * cond_embed_dim, cond_embed_dim]
    a = _build(**WC.CONFIGS["hd96"], **OPT).transformer.layers[0]
    assert (a.self_attn.dim_heads, a.self_attn.num_heads, a.cross_attn.num_heads, a.cross_attn.kv_heads) == (96, 4, 4, 2)
    assert tuple(a.cross_attn.to_kv.weight.shape) == (384, 192)
    assert _build(**WC.CONFIGS["hd32_mha"], **OPT).transformer.layers[0].cross_attn.kv_heads == 8
    assert _build(**WC.CONFIGS["hd96_mha"], **OPT).transformer.layers[0].cross_attn.kv_heads == 4


def test_other_head_widths_raise_with_the_opt_in_too():
    for embed, heads in ((1024, 64), (640, 4), (1000, 10)):          # 16, 160, 100
        with pytest.raises(NotImplementedError, match="dim_heads"):
            _build(**dict(cases.SMALL_DIT, embed_dim=embed, num_heads=heads), **OPT)
    _build(**cases.SMALL_DIT, **OPT)          # 64 and 128: the opt-in changes nothing
    _build(**dict(cases.SMALL_DIT, num_heads=2), **OPT)


def test_context_width_must_split_into_heads():
    """embed_dim 384 / 4 heads of 96 with cond_embed_dim 128: the reference builds the model and fails inside einsum at the first forward."""
    with pytest.raises(ValueError, match=r"128.*96"):
        _build(**dict(cases.SMALL_DIT, embed_dim=384, num_heads=4), **OPT)


@pytest.mark.parametrize("name", ["hd32", "hd96"])
def test_operand_formats(name):
    m = _build(**WC.CONFIGS[name], **OPT)
    for dtype in ("fp8", "fp8-all"):
        with pytest.raises(NotImplementedError, match="dim_heads"):
            m.set_gemm_dtype(dtype)
    assert m.set_gemm_dtype("bf16").set_gemm_dtype("fp32x").set_gemm_dtype("fp16").gemm_dtype == "fp16"          # fp32x works, unlike 128
    m.set_block_gemm_dtypes(["fp16", "bf16", "fp16"]).set_block_gemm_dtypes(None)
    # accepted, without effect on such a plan
    m.set_layernorm_fusion(True).set_cross_attention_fusion(True).set_layernorm_fusion(False).set_cross_attention_fusion(False)


@pytest.mark.parametrize("kwargs", [dict(conformer=True), dict(remove_norms=True), dict(ff_kwargs={"glu": False})], ids=["conformer", "remove_norms", "no_glu"])
@pytest.mark.parametrize("name", ["hd32", "hd96"])
def test_block_options_still_raise(name, kwargs):
    with pytest.raises(NotImplementedError, match="dim_heads"):
        _build(**WC.CONFIGS[name], allow_block_options=True, **OPT, **kwargs)


@pytest.mark.parametrize("name", ["hd32", "hd96"])
def test_use_conv_still_raises(name):
    with pytest.raises(NotImplementedError, match="dim_heads"):
        _build(**WC.CONFIGS[name], ff_kwargs={"use_conv": True}, allow_conv_ff=True, **OPT)


def test_config_key_and_command_line_flag(monkeypatch):
    """DiTWrapper passes "allow_head_widths": true of model.diffusion.config through; generate.py --allow-head-widths writes the key and is an
    error with --model-name."""
    import stable_audio_tools as S
    from dit_family_host import model_config
    from stable_audio_tools.models import _init
    with _init.skip_init():
        with pytest.raises(NotImplementedError, match="allow_head_widths"):
            S.create_model_from_config(model_config(num_heads=8))
        assert S.create_model_from_config(model_config(num_heads=8, allow_head_widths=True)).model.model.transformer.dim_heads == 32
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "friendly-stable-audio-tools_amd"))
    import generate as G
    base = ["generate.py", "--output-dir", "o", "--cond-yaml-path", "c"]
    monkeypatch.setattr(sys, "argv", base)
    assert "allow_head_widths" not in G.apply_config_flags(G.get_args(), model_config(num_heads=8))["model"]["diffusion"]["config"]
    monkeypatch.setattr(sys, "argv", base + ["--allow-head-widths"])
    assert G.apply_config_flags(G.get_args(), model_config(num_heads=8))["model"]["diffusion"]["config"]["allow_head_widths"] is True
    monkeypatch.setattr(sys, "argv", base + ["--allow-head-widths", "--model-name", "some/model"])
    with pytest.raises(SystemExit):
        G.get_args()


# ------------------------------------------------------------------------------- the C ABI
def _create_ex(cfg, head_widths=1, options=True, options_bytes=None):
    from stable_audio_tools import _hip
    lib = _hip.lib()
    plan = ctypes.c_void_p()
    c = _hip.SatDitCfg(*cfg)
    o = _hip.SatDitCreateOptions(head_widths)
    rc = lib.sat_dit_plan_create_ex(ctypes.byref(c), ctypes.sizeof(c), ctypes.byref(o) if options else None,
                                    ctypes.sizeof(o) if options_bytes is None else options_bytes, ctypes.byref(plan))
    return rc, (lib.sat_last_error() if rc else b""), plan


def test_plan_create_ex_admits_32_and_96():
    from stable_audio_tools import _hip
    lib = _hip.lib()

    def create(*cfg, **kw):
        rc, msg, plan = _create_ex(cfg, **kw)
        if rc == 0:
            lib.sat_dit_plan_destroy(plan)
        return rc, msg

    hd32, hd96 = (64, 256, 2, 8, 128, 128, 96, 128), (64, 384, 2, 4, 192, 192, 96, 128)
    for cfg in (hd32, hd96):
        for gemm_dtype in (0, 2, 3):
            for adaln in (0, 1):
                assert create(*cfg, adaln, gemm_dtype) == (0, b""), (cfg, adaln, gemm_dtype)
        rc, msg = create(*cfg, 0, 1)          # e4m3 (embed_dim 256 passes the e4m3 shape rule: the head width refuses)
        assert rc == -2 and b"dim_heads" in msg, (cfg, rc, msg)
        for kw in (dict(head_widths=0), dict(options=False)):
            rc, msg = create(*cfg, **kw)
            assert rc == -2 and b"dim_heads" in msg, (cfg, kw, rc, msg)
        rc, msg = lib.sat_dit_plan_create(ctypes.byref(_hip.SatDitCfg(*cfg)), ctypes.byref(ctypes.c_void_p())), lib.sat_last_error()
        assert rc == -2 and b"dim_heads" in msg
    assert create(64, 256, 2, 8, 0, 0, 96, 128) == (0, b"")
    assert create(64, 256, 2, 4, 128, 128, 96, 128) == (0, b"") and create(64, 256, 2, 2, 128, 128, 96, 128) == (0, b"")          # 64, 128
    assert create(64, 256, 2, 4, 128, 128, 96, 128, options=False, options_bytes=12345) == (0, b"")          # NULL options: the size is not read
    rc, msg = create(64, 1000, 2, 10, 0, 0, 96, 128)
    assert rc == -2 and b"dim_heads" in msg
    rc, msg = create(64, 384, 2, 4, 128, 128, 96, 128)          # 128 / 96 kv heads
    assert rc == -2 and b"cond_embed_dim" in msg
    rc, msg = create(64, 768, 2, 24, 160, 160, 96, 128)          # 24 query heads over 5 kv heads
    assert rc == -2 and b"kv heads" in msg
    for size in (0, 3, 8):
        rc, msg = create(*hd32, options_bytes=size)
        assert rc == -1 and b"options_bytes" in msg, (size, rc, msg)
    for value in (2, -1):
        rc, msg = create(*hd32, head_widths=value)
        assert rc == -1 and b"head_widths" in msg, (value, rc, msg)
    assert ctypes.sizeof(_hip.SatDitCreateOptions) == 4 and lib.sat_version() == 6 and ctypes.sizeof(_hip.SatDitCfg) == 56


@pytest.mark.parametrize("cfg", [(64, 256, 2, 8, 128, 128, 96, 128), (64, 384, 2, 4, 192, 192, 96, 128)], ids=["32", "96"])
def test_block_options_and_ff_conv_are_refused_on_such_a_plan(cfg):
    from stable_audio_tools import _hip
    lib = _hip.lib()
    rc, _, plan = _create_ex(cfg)
    assert rc == 0
    try:
        for opts in ((1, 0, 1), (0, 1, 1), (0, 0, 0)):
            b = _hip.SatDitBlockOptions(*opts)
            assert lib.sat_dit_plan_set_block_options(plan, ctypes.byref(b), ctypes.sizeof(b)) == -2 and b"dim_heads" in lib.sat_last_error(), opts
        b = _hip.SatDitBlockOptions(0, 0, 1)
        assert lib.sat_dit_plan_set_block_options(plan, ctypes.byref(b), ctypes.sizeof(b)) == 0          # the defaults pass
        c = _hip.SatDitFfConvOptions(3)
        assert lib.sat_dit_plan_set_ff_conv(plan, ctypes.byref(c), ctypes.sizeof(c)) == -2 and b"dim_heads" in lib.sat_last_error()
        c = _hip.SatDitFfConvOptions(1)
        assert lib.sat_dit_plan_set_ff_conv(plan, ctypes.byref(c), ctypes.sizeof(c)) == 0
    finally:
        lib.sat_dit_plan_destroy(plan)


def test_unit_entries_refuse_other_widths_and_bad_paddings():
    """Before anything touches a device: SAT_E_UNSUPPORTED (-2) for a width without a kernel, SAT_E_INVALID (-1) for the padding and
    alignment rules of include/sat_hip.h."""
    from stable_audio_tools import _hip
    lib = _hip.lib()
    p = ctypes.c_void_p(1 << 20)          # never dereferenced: every call below fails its checks
    for fn in (lib.sat_attention_hdw_bf16, lib.sat_attention_hdw_f16):
        for w in (64, 128, 48, 0):
            assert fn(p, p, p, p, 1, 2, 2, w, 78, 78, 128, 128, None) == -2 and b"dim_heads" in lib.sat_last_error(), w
        assert fn(p, p, p, p, 1, 2, 2, 32, 78, 78, 128, 192, None) == -1          # sk_pad % 128 with 32-channel heads
        assert fn(p, p, p, p, 1, 2, 2, 96, 78, 78, 128, 96, None) == -1           # sk_pad % 64
        assert fn(p, p, p, p, 1, 2, 2, 96, 78, 78, 64, 128, None) == -1           # sq_pad % 128
        assert fn(p, p, p, p, 1, 2, 2, 96, 126, 126, 128, 128, None) == -1        # sk_pad >= sk + 3
        assert fn(p, p, p, p, 1, 3, 2, 96, 78, 78, 128, 128, None) == -1          # 3 query heads over 2 kv heads
        assert fn(p, ctypes.c_void_p((1 << 20) + 8), p, p, 1, 2, 2, 96, 78, 78, 128, 128, None) == -1          # alignment
    dst = (ctypes.c_void_p * 3)(1 << 20, 1 << 20, 1 << 20)
    kind = (ctypes.c_int32 * 3)(2 | 8, 2 | 4, 1 | 4)
    for fn in (lib.sat_head_split_hdw_bf16, lib.sat_head_split_hdw_f16):
        for w in (64, 128, 48):
            assert fn(p, p, dst, kind, p, 2, 78, 128, 2, w, 3, None) == -2 and b"dim_heads" in lib.sat_last_error(), w
        assert fn(p, p, dst, kind, p, 2, 78, 96, 2, 96, 3, None) == -1            # s_pad % 64
        assert fn(p, p, dst, kind, p, 2, 78, 64, 2, 32, 3, None) == -1            # s_pad >= s + 3
        assert fn(p, p, dst, kind, p, 2, 78, 128, 2, 32, 4, None) == -1           # parts
        assert fn(p, None, dst, kind, p, 2, 78, 128, 2, 32, 3, None) == -1        # a rotating part without inv_freq
    for w in (128, 48):
        assert lib.sat_attention_f32_hdw(p, p, p, p, 1, 2, 2, w, 8, 8, None) == -2 and b"dim_heads" in lib.sat_last_error()
        assert lib.sat_split_heads_f32_hdw(p, p, p, p, 1, 8, 3, 2, w, 0, None, None, 0, None) == -2 and b"dim_heads" in lib.sat_last_error()
    assert lib.sat_attention_f32_hdw(p, p, p, p, 1, 3, 2, 32, 8, 8, None) == -1
    assert lib.sat_split_heads_f32_hdw(p, p, p, p, 1, 8, 4, 2, 96, 0, None, None, 0, None) == -1


# ------------------------------------------------------------------------------- the kernels, compiled and inspected
def _kernels(src, defines, tmp_path):
    out = os.path.join(tmp_path, "k.s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", os.path.join(CSRC, src), "-o", out] + defines,
                   check=True, capture_output=True)
    meta = {}
    for blk in open(out).read().split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        meta[name] = {k: int(re.search(rf"\.{k}:\s+(\d+)", blk).group(1))
                      for k in ("vgpr_count", "vgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")}
    return meta


# VGPR budgets: 512 threads per workgroup = 256 at most; the 32-channel attention kernel must stay at 128 or below, which is what lets a second
# workgroup be resident on the CU (its ring is 48 KiB); the head split runs 256 threads and asks for no more than 128 either
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
@pytest.mark.parametrize("defines", [[], ["-DSAT_OPERAND_F16"]], ids=["bf16", "f16"])
@pytest.mark.parametrize("src, kernels", [("attention_hdw.hip", {"attention_hdw_kernelILi32ELb0E": 128, "attention_hdw_kernelILi96ELb0E": 256}),
                                          ("head_split_hdw.hip", {"head_split_hdw_kernelILi32E": 128, "head_split_hdw_kernelILi96E": 128})],
                         ids=["attention", "head_split"])
def test_hdw_kernels_use_no_scratch(src, kernels, defines, tmp_path):
    meta = _kernels(src, defines, str(tmp_path))
    # 32, 96 and 128 (the gates of the last: tests/test_dit_head_dim_host.py; of the causal instantiations: tests/test_dit_causal_host.py)
    assert len([name for name in meta if src[:-4] + "_kernelILi" in name and "ELb1EE" not in name]) == 3, sorted(meta)
    for kernel, budget in kernels.items():
        found = [m for name, m in meta.items() if kernel in name]
        assert len(found) == 1, (kernel, sorted(meta))          # every instantiation is there
        assert found[0]["vgpr_count"] <= budget, f"{kernel}: {found[0]}"
    for name, m in meta.items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, f"{name}: {m}"
        assert m["group_segment_fixed_size"] <= 64 * 1024, f"{name}: {m}"          # (the attention ring is dynamic LDS: attn_hdw_tiles.h)


def test_lds_tile_maps_are_bijections_and_conflict_free(tmp_path):
    """WU.check_lds_tile_maps on csrc/attn_hdw_tiles.h for both widths and both tiles; the four hole slots of each of the 64 padded 96-channel
    K rows and the 32 spare V^T rows of 8 slots are the only DMA lanes without a chunk."""
    tiles = WU.check_lds_tile_maps(CSRC, str(tmp_path), (32, 96))
    assert [(t["kind"], t["w"], t["rows"], t["chunks"], t["row_bytes"], t["size"], t["pieces"]) for t in tiles] == [
        ("K", 32, 128, 4, 64, 8192, 1), ("V", 32, 32, 16, 256, 8192, 1), ("K", 96, 64, 12, 256, 16384, 2), ("V", 96, 96, 8, 128, 16384, 2)]
    assert [t["holes"] for t in tiles] == [0, 0, 64 * 4, 32 * 8]


# ------------------------------------------------------------------------------- the gates bite
def _rand(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("fmt", FORMATS, ids=repr)
@pytest.mark.parametrize("w", [32, 96])
def test_head_split_gate_catches_rotation_and_scale_mistakes(w, fmt):
    """The head-split test's construction (two sequences of 78 rows, rows over three decades) in float64: the right answer, rounded to the
    operand format, passes fmt.tol(4e-3); a wrong pair offset (96: j + 32 instead of j + 24), a wrong rotation width (32: the 16 frequencies
    of RotaryEmbedding(64) instead of RotaryEmbedding(32) -- a head of 32 has no channel j + 32 to pair with), rotated pass-through channels
    (96: 48..95) and the pre-scale of 64-channel heads (1 / 8 instead of W ** -0.5) each fail it."""
    b, s, h = 2, 78, 2
    gen = torch.Generator().manual_seed(171)
    x = torch.randn((b * s, 3 * h * w), generator=gen)
    x = x * (10.0 ** (torch.rand((b * s, 1), generator=gen) * 3.0 - 2.0))
    gate, inv = fmt.tol(4e-3), WU.inv_freq_of(w)
    for qk_norm in (False, True):
        q, k, _ = WU.head_split_reference(x, b, s, h, w, inv, qk_norm)
        assert rel_l2(fmt.round(q.float()), q.float()) < gate and rel_l2(fmt.round(k.float()), k.float()) < gate
        wrong = {"the pre-scale of 64-channel heads": dict(scale=WU.LOG2E / 8.0)}
        if w == 96:
            wrong["pairs (j, j + 32)"] = dict(pair_offset=32)
            wrong["channels 48..95 rotated"] = dict(rotate_all=True)
        for what, kw in wrong.items():
            qw, kw_, _ = WU.head_split_reference(x, b, s, h, w, inv, qk_norm, **kw)
            assert max(rel_l2(qw.float(), q.float()), rel_l2(kw_.float(), k.float())) > 10 * gate, what
        qw, kw_, _ = WU.head_split_reference(x, b, s, h, w, WU.inv_freq_of(w, rotary_dim=64 if w == 32 else 96), qk_norm)
        assert min(rel_l2(qw.float(), q.float()), rel_l2(kw_.float(), k.float())) > 10 * gate, "the frequencies of another rotation width"


@pytest.mark.parametrize("fmt", FORMATS, ids=repr)
@pytest.mark.parametrize("w", [32, 96])
def test_attention_gate_catches_head_index_scale_and_pad_key_mistakes(w, fmt):
    """The attention test's GQA construction in float64: a kv-head index h % KVH instead of h / (H / KVH) and the scale 1 / 8 instead of
    W ** -0.5 fail fmt.tol(5e-3); on the mask-edge case, an attended front pad key fails NEG_GATE in the sequences that have one."""
    import mask_edge
    h, kvh = (8, 4) if w == 32 else (4, 2)
    q, k, v = _rand((2, h, 78, w), 12) * 1.5, _rand((2, kvh, 130, w), 13) * 1.5, _rand((2, kvh, 130, w), 14)
    want = WU.attention_reference(q, k, v, w)
    gate = fmt.tol(5e-3)
    assert rel_l2(fmt.round(want.float()), want.float()) < gate
    assert rel_l2(WU.attention_reference(q, k, v, w, kv_index=lambda i, h_, kvh_: i % kvh_), want) > 10 * gate
    assert rel_l2(WU.attention_reference(q, k, v, w, scale=0.125), want) > 10 * gate
    case = mask_edge.self_attention_case(fmt, w, 63, prescaled=True)
    bad = mask_edge.with_front_pads_attended(case, fmt)
    errs = slice_errors(bad.view(case["b"], case["sq"], case["h"], w), case["want"].view(case["b"], case["sq"], case["h"], w), (0,))
    assert errs[0] <= mask_edge.NEG_GATE[fmt.name] and all(e > 10 * mask_edge.NEG_GATE[fmt.name] for e in errs[1:]), errs
