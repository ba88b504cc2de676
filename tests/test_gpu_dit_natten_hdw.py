"""Neighbourhood-attention DiTs with 128-, 32- and 96-channel heads (natten_kernel_size behind allow_natten and allow_natten_head_widths) on
the device: the launchers of csrc/attention_hdw_window.hip alone (sat_attention_hdw_window_* / sat_attention_f32_window_w) against the
float64 references of tests/dit_natten_units.py at the gates of test_attention_window, that no key outside a query's window reaches its
output, then the plan against the REFERENCE's own outputs (tests/golden/dit_natten_hdw_small*.npz: make_golden_dit_natten_hdw.py, with
natten_standin.py in NATTEN's place) through the family harness, the reports, poisoned workspaces, call history and generate_diffusion_cond.

Kernel instantiations: three 16-bit kernels per build (W = 32 with 128-key tiles of four blocks, W = 96 with padded K rows and spare V^T rows,
W = 128) and two fp32 kernels (32, 96).  S = 33 is one workgroup with one active wave and a tail wave, 65 one key past a 64-key tile, 129 one
past a 128-key tile, 257 one past two of them (and a second workgroup of one query), 301 two workgroups, 645 three (the middle one walks
neither end of the keys at K <= 129); K = 3 and 7 leave most blocks of a tile skipped -- at W = 32 also the first two of a tile in front of a
visible third -- 33 and 65 give blocks of all three classes, 129 and K = S full blocks."""
import ctypes
import functools
import math
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import dit_natten_hdw_cases as HC  # noqa: E402
import dit_natten_hdw_units as HU  # noqa: E402
import dit_natten_units as NU  # noqa: E402
from dit_family_gpu import FP32X_GATE, Harness  # noqa: E402
from dit_head_width_units import _pad_heads, _vt_perm  # noqa: E402
from util import FORMATS, SUITE, assert_bit_equal, assert_close, assert_close_sliced, guarded, rel_l2  # noqa: E402

pytestmark = pytest.mark.gpu
H = Harness(HC.FAMILY)
B, HEADS, KVH = 4, 4, 2          # four sequences: the key shifts (b * s) & 3 take every value for an odd s; GQA 2:1
UNIT_CASES = [(s, ks) for s in HU.SEQ_LENS for ks in NU.kernel_sizes(s)]
SUITE_CASES = HC.cases_of(SUITE.gemm_dtype)          # the cases whose reference alone passes the gate of the suite's format
F32_WIDTHS = (32, 96)


def _lib():
    from stable_audio_tools import _hip
    return _hip, _hip.lib()


def _attention(dev, fmt, q, k, v, ks):
    """q [b, h, s, W] in the log2 domain, k / v [b, kvh, s, W], all in fmt.dtype -> [b, s, h * W] between guard bands"""
    _hip, lib = _lib()
    (b, h, s, w), kvh = q.shape, k.shape[1]
    sq_pad = (s + 127) // 128 * 128
    kt = HU.KEY_TILE[w]
    sk_pad = (s + 3 + kt - 1) // kt * kt
    qd = _pad_heads(q, sq_pad).to(dev)
    kd = _pad_heads(k, sk_pad, key_side=True).to(dev)
    vtd = _pad_heads(v, sk_pad, key_side=True).transpose(2, 3)[..., _vt_perm(sk_pad)].contiguous().to(dev)
    og = guarded((b * s, h * w), fmt.dtype, dev, name="out")
    _hip.check(fmt.fn(lib, "sat_attention_hdw_window_bf16")(_hip.ptr(qd), _hip.ptr(kd), _hip.ptr(vtd), _hip.ptr(og.t), b, h, kvh, w, s, sq_pad, sk_pad,
                                                            ks, _hip.stream()))
    torch.cuda.synchronize()
    og.check().assert_written()
    return og.t.view(b, s, h * w)


def _attention_f32(dev, q, k, v, ks, scale):
    _hip, lib = _lib()
    (b, h, s, w), kvh = q.shape, k.shape[1]
    og = guarded((b * s, h * w), torch.float32, dev, name="out")
    qd, kd, vd = (t.to(dev) for t in (q, k, v))
    _hip.check(lib.sat_attention_f32_window_w(_hip.ptr(qd), _hip.ptr(kd), _hip.ptr(vd), _hip.ptr(og.t), b, h, kvh, w, s, ks, scale, _hip.stream()))
    torch.cuda.synchronize()
    og.check().assert_written()
    return og.t.view(b, s, h * w)


def _per_query(x, h):
    b, s, _ = x.shape
    return x.view(b, s, h, -1)          # keep_dims (0, 1, 2): one slice per (sequence, query, head)


@functools.lru_cache(maxsize=4)
def _unit(fmt, w, s):
    return HU.unit_tensors(fmt, w, B, HEADS, KVH, s)


@functools.lru_cache(maxsize=4)
def _unit_f32(w, s):
    rand = lambda shape, sd: torch.randn(shape, generator=torch.Generator().manual_seed(sd))
    g = float(w) ** -0.25          # the logit spread of the scaled family, as dit_natten_hdw_cases.qk_gain
    q, k, v = rand((B, HEADS, s, w), 21) * g, rand((B, KVH, s, w), 22) * g, rand((B, KVH, s, w), 23)
    v[1] *= 8.0          # a row taken from the neighbouring sequence dominates
    return q, k, v


# ------------------------------------------------------------------------------- the launchers alone
@pytest.mark.parametrize("fmt", FORMATS, ids=repr)
@pytest.mark.parametrize("s,ks", UNIT_CASES)
@pytest.mark.parametrize("w", HU.WIDTHS)
def test_attention_hdw_window(dev, w, s, ks, fmt):
    """The gates of test_attention_window, unchanged: fmt.tol(5e-3) against the matched-rounding reference, whole and per (sequence, query,
    head), and fmt.tol(1e-2) against the exact one."""
    q, q_eff, k, v, scale = _unit(fmt, w, s)
    want = NU.window_attention(q_eff, k, v, ks, scale, rnd=fmt.round).float()
    exact = NU.window_attention(q_eff, k, v, ks, scale).float()
    out = _attention(dev, fmt, q, k, v, ks)
    e, ex = rel_l2(out, want), rel_l2(out, exact)
    print(f"\n[attention_hdw_window W={w} K={ks} {fmt} {B}x{HEADS}/{KVH}x{s}] rel-L2 vs matched rounding {e:.2e} (gate {fmt.tol(5e-3):.1e}), "
          f"vs exact {ex:.2e} (gate {fmt.tol(1e-2):.1e})")
    assert_close(f"attention_hdw_window W={w} K={ks} s={s}", out, want, fmt.tol(5e-3))
    assert_close_sliced(f"attention_hdw_window W={w} K={ks} s={s} per (sequence, query, head)", _per_query(out, HEADS), _per_query(want, HEADS),
                        fmt.tol(5e-3), (0, 1, 2), fmt.round)
    assert ex < fmt.tol(1e-2)


@pytest.mark.parametrize("s,ks", UNIT_CASES)
@pytest.mark.parametrize("w", F32_WIDTHS)
def test_attention_f32_window_w(dev, w, s, ks):
    """sat_attention_f32_window_w against float64 at the 1e-5 gate of the fp32 suite, whole and per (sequence, query, head)."""
    q, k, v = _unit_f32(w, s)
    want = NU.window_attention(q, k, v, ks, 1.0).float()
    out = _attention_f32(dev, q, k, v, ks, 1.0)
    e = assert_close(f"attention_f32_window_w W={w} K={ks} s={s}", out, want, 1e-5)
    assert_close_sliced(f"attention_f32_window_w W={w} K={ks} s={s} per (sequence, query, head)", _per_query(out, HEADS), _per_query(want, HEADS), 1e-5,
                        (0, 1, 2))
    print(f"\n[attention_f32_window_w W={w} K={ks} s={s}] rel-L2 vs float64 {e:.2e} (gate 1.0e-05)")


# queries [a, b] of s = 645 at K: the bounds sit at the edge of a wave (32), of a 32-key block, of a 64-key tile, of a 128-key tile and of a
# workgroup (256); the first six are those of the 64-channel suite
RANGES = [(33, 32, 63), (33, 64, 127), (7, 96, 159), (129, 256, 511), (65, 0, 255), (7, 512, 644), (33, 128, 255), (7, 384, 511), (129, 128, 383)]


def _rewritten(k, v, s, ks, a, b, dtype):
    """K and V of every key outside the windows of the queries [a, b] rewritten with large finite values"""
    st = NU.start(s, ks)
    lo, hi = int(st[a]), int(st[b]) + ks
    outside = torch.ones(s, dtype=torch.bool)
    outside[lo:hi] = False
    rand = lambda shape, sd: torch.randn(shape, generator=torch.Generator().manual_seed(sd))
    k2, v2 = k.clone(), v.clone()
    k2[:, :, outside] = (rand(k2[:, :, outside].shape, 77) * 40.0).to(dtype)          # large scores: a leaked key would take the row
    v2[:, :, outside] = (rand(v2[:, :, outside].shape, 78) * 100.0).to(dtype)
    return k2, v2, lo, hi


@pytest.mark.parametrize("fmt", FORMATS, ids=repr)
@pytest.mark.parametrize("ks,a,b", RANGES)
@pytest.mark.parametrize("w", HU.WIDTHS)
def test_keys_outside_the_windows_do_not_reach_the_output(dev, w, ks, a, b, fmt):
    s = 645
    q, _, k, v, _ = _unit(fmt, w, s)
    first = _attention(dev, fmt, q, k, v, ks)
    k2, v2, lo, hi = _rewritten(k, v, s, ks, a, b, fmt.dtype)
    second = _attention(dev, fmt, q, k2, v2, ks)
    assert_bit_equal(f"attention_hdw_window W={w} K={ks}: queries {a}..{b} after the keys outside [{lo}, {hi}) changed", second[:, a:b + 1],
                     first[:, a:b + 1])
    rest = torch.ones(s, dtype=torch.bool)
    rest[a:b + 1] = False
    assert not torch.equal(second[:, rest], first[:, rest])          # the other queries did see them


@pytest.mark.parametrize("w", F32_WIDTHS)
def test_f32_keys_outside_the_windows_do_not_reach_the_output(dev, w):
    s, ks, a, b = 301, 33, 64, 127
    q, k, v = _unit_f32(w, s)
    first = _attention_f32(dev, q, k, v, ks, 1.0)
    k2, v2, lo, hi = _rewritten(k, v, s, ks, a, b, torch.float32)
    second = _attention_f32(dev, q, k2, v2, ks, 1.0)
    assert_bit_equal(f"attention_f32_window_w W={w}: queries {a}..{b} after the keys outside [{lo}, {hi}) changed", second[:, a:b + 1], first[:, a:b + 1])
    assert not torch.equal(second[:, :a], first[:, :a])


# ------------------------------------------------------------------------------- the plan
@pytest.mark.parametrize("name", SUITE_CASES)
def test_dit_natten_hdw_vs_reference(dev, name):
    """The harness gates, unchanged, on the cases whose reference with rounded operands passes them in the suite's format
    (dit_natten_hdw_cases.DROPPED lists the others with their figures: none in fp16; in bf16 every CFG 1 case, K = 129 at S = 301 and K == n at
    CFG 7).  Measured (profiles/dit_natten_hdw_verification.txt has every figure): fp16 1.4e-4 - 3.8e-4 at CFG 1 (gate 6.3e-4) and 6.0e-4 -
    1.1e-3 at CFG 7 (gate 3.0e-3); under SAT_TEST_DTYPE=bf16 4.9e-3 - 8.6e-3 on the 11 CFG 7 cases that run (gate 1.2e-2).  Measured only: of
    the 18 cases left out in bf16 the product is below the gate on 15 and at 2.75e-3 - 3.05e-3 against 2.5e-3 on the three K = 7, CFG 1 ones."""
    H.check_vs_reference(dev, name, SUITE.gemm_dtype, H.gate(name), rounded=True)


@pytest.mark.parametrize("name", [n for n in HC.CASES if HC.WIDTH[HC.CASES[n][0]] in F32_WIDTHS])
def test_dit_natten_hdw_fp32x_vs_reference(dev, name):
    """The fp32 verification mode on the fp32 window kernels (32- and 96-channel heads; 128 has no fp32 mode): an indexing error does not hide
    behind 16-bit rounding.  Every case of those widths, whatever its 16-bit figure."""
    H.check_vs_reference(dev, name, "fp32x", FP32X_GATE)


def test_fp32x_stays_refused_at_128(dev):
    m = H.model("hd128_k33", dev)
    with pytest.raises(NotImplementedError, match=r"dim_heads=128.*gemm_dtype"):
        m.set_gemm_dtype("fp32x")
    assert m.gemm_dtype == SUITE.gemm_dtype


@pytest.mark.parametrize("name", ["hd128_k33_cfg7_T296", "hd32_k129_cfg7_T640", "hd96_k7_cfg7_T296"])
def test_per_block_formats(dev, name):
    """[fp16, bf16, fp16] at the bf16 gate of the case (cases whose rounded reference passes that gate)."""
    assert name not in HC.DROPPED["bf16"]
    H.check_per_block_formats(dev, name)


@pytest.mark.parametrize("name,dtype", [("hd128_k33_cfg7_T296", "suite"), ("hd32_k33_cfg7_T296", "suite"), ("hd32_k129_cfg7_T640", "fp32x"),
                                        ("hd96_adaln_cfg1_T301", "suite"), ("hd96_k7_cfg7_T296", "fp32x")])
def test_fused_denoise_matches_forward(dev, name, dtype):
    H.check_fused_denoise(dev, name, dtype)


def test_the_window_is_not_the_full_attention(dev):
    """The same weights with natten_kernel_size=None give another output: the option reaches the kernels."""
    name = "hd128_k33_cfg1_T64"
    from stable_audio_tools.models import _init
    from stable_audio_tools.models.dit import DiffusionTransformer
    with _init.skip_init():
        full = DiffusionTransformer(**HC.without_natten(HC.CONFIGS["hd128_k33"]), **HC.FAMILY.product_kwargs)
    full.load_state_dict(H.model("hd128_k33", dev).state_dict(), strict=True)
    full = full.to(dev).eval()
    x, t, kw = H.inputs(name, dev)
    assert rel_l2(full(x, t, **kw), H.gold()[name]) > 0.15          # (the generator measured 0.29)


def test_a_short_sequence_is_refused_before_any_launch(dev):
    """27 tokens + the global token + 4 prepend rows = 32 < 33: ValueError from forward, and the plan keeps running."""
    m = H.model("hd32_k33", dev)
    x, t, kw = H.inputs("hd32_k33_cfg1_T64", dev)
    want = m(x, t, **kw)
    with pytest.raises(ValueError, match="natten_kernel_size=33"):
        m(x[:, :, :27].contiguous(), t, **kw)
    assert_bit_equal("after the refused call", m(x, t, **kw), want)


@pytest.mark.parametrize("cfg_name", ["hd128_k33", "hd32_k33", "hd96_k33"])
def test_reports(dev, cfg_name):
    """residual_stream_report and activation_range_report(True) return finite rows on a staged neighbourhood plan, and the output is
    bit-identical with the range report on."""
    m = H.model(cfg_name, dev)
    x, t, kw = H.inputs(f"{cfg_name}_cfg7_T296", dev)
    want = m(x, t, **kw)
    m.residual_stream_report(True)
    m(x, t, **kw)
    rows = m.residual_stream_report(False)
    assert len(rows) == 3 * 3
    for r in rows:          # (no cross-attention update in such a model: its rows stay empty)
        assert math.isfinite(r["max_abs"]) and r["saturated"] == 0, r
        assert r["update"] == "cross_attn.to_out" or (r["max_abs"] > 0 and math.isfinite(r["crest"])), r
    m.activation_range_report(True)
    try:
        got = m(x, t, **kw)
        torch.cuda.synchronize()
    finally:
        rows = m.activation_range_report(False)
    assert_bit_equal(f"{cfg_name}: the output with the range report on", got, want)
    assert rows
    for r in rows:
        assert math.isfinite(r["max_abs"]) and r["nonfinite"] == 0 and r["over_fp16"] == 0, r
        if not r["buffer"].startswith(("cross_", "a_cross")):
            assert r["elements"] > 0 and r["max_abs"] > 0, r


WORKSPACE_ROWS = [("hd128_k7_cfg7_T296", "suite"), ("hd128_k129_cfg7_T640", "suite"), ("hd32_k7_cfg7_T296", "suite"), ("hd32_k33_cfg7_T296", "fp32x"),
                  ("hd32_k129_cfg7_T640", "suite"), ("hd96_k33_cfg7_T296", "suite"), ("hd96_k129_cfg7_T296", "fp32x")]


@pytest.mark.parametrize("name,dtype", WORKSPACE_ROWS)
def test_workspace_contents_do_not_matter(dev, name, dtype):
    """Every fill of util.WORKSPACE_FILLS in the workspace before the call, bit for bit: a tile that is not walked, a skipped block, a hole
    of a padded K row or a spare V^T row must not turn into a read of what the buffer held."""
    from test_gpu_state_independence import check_poisoned_workspace
    m = H.model(HC.CASES[name][0], dev)
    x, t, kw = H.inputs(name, dev)
    try:
        m.set_gemm_dtype(SUITE.gemm_dtype if dtype == "suite" else dtype)
        check_poisoned_workspace(f"{name} ({dtype})", lambda: m(x, t, **kw), m)
    finally:
        m.set_gemm_dtype(SUITE.gemm_dtype)


@pytest.mark.parametrize("nan", [False, True], ids=["a longer call", "an all-NaN longer call"])
@pytest.mark.parametrize("cfg_name,small,large,dtype", [("hd128_k129", "hd128_k129_cfg7_T296", "hd128_k129_cfg7_T640", "suite"),
                                                        ("hd32_k129", "hd32_k129_cfg7_T296", "hd32_k129_cfg7_T640", "suite"),
                                                        ("hd32_k33", "hd32_k33_cfg1_T64", "hd32_k33_cfg7_T296", "fp32x"),
                                                        ("hd96_k33", "hd96_k33_cfg1_T64", "hd96_k33_cfg7_T296", "suite")])
def test_behind_a_longer_call(dev, cfg_name, small, large, dtype, nan):
    """The small case, the longer case of the same model (more sequences, more rows: every buffer of the workspace is left full of its values
    -- or, with x, the global embedding and the prepend tokens all NaN, full of NaN -- beyond the small case's pads and unwalked tiles), the
    small case again: the same bits."""
    m = H.model(cfg_name, dev)
    xs, ts, kws = H.inputs(small, dev)
    xl, tl, kwl = H.inputs(large, dev)
    if nan:
        poison = lambda v: torch.full_like(v, float("nan")) if torch.is_tensor(v) and v.is_floating_point() and v.dim() == 3 else v
        xl, kwl = poison(xl), {k: (poison(v) if k != "prepend_cond_mask" else v) for k, v in kwl.items()}
        kwl["global_embed"] = torch.full_like(kwl["global_embed"], float("nan"))
    try:
        m.set_gemm_dtype(SUITE.gemm_dtype if dtype == "suite" else dtype)
        want = m(xs, ts, **kws).clone()
        out_l = m(xl, tl, **kwl)
        torch.cuda.synchronize()
        assert bool(torch.isnan(out_l).all()) if nan else bool(torch.isfinite(out_l).all())
        got = m(xs, ts, **kws)
        torch.cuda.synchronize()
        assert_bit_equal(f"{small} ({dtype}) behind {large}{' of NaN' if nan else ''}", got, want)
    finally:
        m.set_gemm_dtype(SUITE.gemm_dtype)


def test_neighborhood_attention_hdw_after_finalize(dev):
    """SAT_E_STATE on a finalized plan from both entries, and the plan keeps running."""
    _hip, lib = _lib()
    m = H.model("hd128_k33", dev)
    x, t, kw = H.inputs("hd128_k33_cfg1_T64", dev)
    want = m(x, t, **kw)
    o = _hip.SatDitNeighborhoodOptions(0)
    for fn in (lib.sat_dit_plan_set_neighborhood_attention_hdw, lib.sat_dit_plan_set_neighborhood_attention):
        assert fn(m._ensure_plan(), ctypes.byref(o), ctypes.sizeof(o)) == -5
        assert b"finalized" in lib.sat_last_error()
    assert_bit_equal("after the refused calls", m(x, t, **kw), want)


def test_generate_diffusion_cond_with_a_128_channel_neighbourhood_model(dev):
    """generate_diffusion_cond on a reduced config-built model with 128-channel heads and natten_kernel_size 7 behind "allow_natten": true and
    "allow_natten_head_widths": true, no cross-attention: 4 steps of dpmpp-3m-sde; finite audio of the right shape, two runs with one seed are
    bit-identical, the same weights with full attention give other audio, and a sample too short for the window is a ValueError."""
    import stable_audio_tools as S
    from dit_family_host import model_config
    from stable_audio_tools import synthetic
    from stable_audio_tools.inference.generation import generate_diffusion_cond
    from stable_audio_tools.models import _init

    def build(**keys):
        cfg = model_config(cond_token_dim=0, num_heads=2, **keys)
        cfg["model"]["diffusion"]["cross_attention_cond_ids"] = []
        with _init.skip_init():
            return cfg, S.create_model_from_config(cfg)

    cfg, model = build(attn_kwargs={"natten_kernel_size": 7}, allow_natten=True, allow_natten_head_widths=True)
    tr = model.model.model.transformer
    assert tr.natten_kernel_size == 7 and tr.dim_heads == 128
    sd = synthetic.synth_state_dict(model.state_dict(), 0)
    ratio = cfg["model"]["pretransform"]["config"]["downsampling_ratio"]

    def run(mod, t_len=16):
        mod.load_state_dict(sd, strict=True)
        mod = mod.to(dev).eval()
        cond = mod.conditioner([{"seconds_start": 0, "seconds_total": 12}])
        audio = generate_diffusion_cond(mod, steps=4, cfg_scale=7.0, conditioning_tensors=cond, sample_size=t_len * ratio, seed=3, device=str(dev),
                                        sampler_type="dpmpp-3m-sde", sigma_min=0.3, sigma_max=500)
        torch.cuda.synchronize()
        assert audio.shape == (1, 2, t_len * ratio) and torch.isfinite(audio).all() and float(audio.abs().max()) > 0
        return audio

    a0, a1 = run(model), run(model)
    assert torch.equal(a0, a1)
    assert not torch.equal(run(build()[1]), a0)
    with pytest.raises(ValueError, match="natten_kernel_size=7"):
        run(model, t_len=5)          # 5 frames + the global token
