"""Neighbourhood-attention DiTs (ContinuousTransformer attn_kwargs natten_kernel_size behind allow_natten) on the device: the two window
launchers alone (csrc/attention_window.hip through sat_attention_window_* / sat_attention_f32_window) against the float64 references of
tests/dit_natten_units.py at the gates of the full-attention unit tests, that no key outside a query's window reaches its output, the
softmax reference when a block shows some queries of a wave no key, then the plan against the REFERENCE's own outputs
(tests/golden/dit_natten_small*.npz: tests/golden/make_golden_dit_natten.py, with tests/golden/natten_standin.py in NATTEN's place) through
the family harness, the reports, poisoned workspaces and generate_diffusion_cond.

Kernel instantiations: the launcher has one 16-bit kernel per build (256 queries per workgroup, one key ring) and one fp32 kernel; every
case of test_attention_window reaches the first in the build of its format, every case of test_attention_f32_window the second.  Inside
the kernel, S = 33 is one workgroup with one active wave and a tail wave, 64 / 65 a full tile and one key past it, 129 two tiles with every
wave active in none of them alone, 301 two workgroups (the second with a tail), 645 three (the middle one walks neither end of the keys at
K <= 129); K = 3 and 7 leave most 32-key blocks of a tile skipped, 33 and 65 give blocks of all three classes, 129 and K = S full blocks."""
import ctypes
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import dit_natten_cases as NC  # noqa: E402
import dit_natten_units as NU  # noqa: E402
from dit_family_gpu import FP32X_GATE, Harness  # noqa: E402
from dit_head_width_units import _pad_heads, _vt_perm  # noqa: E402
from util import FORMATS, SUITE, assert_bit_equal, assert_close, assert_close_sliced, guarded, rel_l2  # noqa: E402

pytestmark = pytest.mark.gpu
H = Harness(NC.FAMILY)
B, HEADS, KVH, W = 4, 4, 2, 64          # four sequences: the key shifts (b * s) & 3 take every value for an odd s; GQA 2:1
UNIT_CASES = [(s, ks) for s in NU.SEQ_LENS for ks in NU.kernel_sizes(s)]


def _lib():
    from stable_audio_tools import _hip
    return _hip, _hip.lib()


def _attention(dev, fmt, q, k, v, ks, scale):
    """q [b, h, s, 64], k / v [b, kvh, s, 64], all in fmt.dtype -> [b, s, h * 64] between guard bands"""
    _hip, lib = _lib()
    (b, h, s, w), kvh = q.shape, k.shape[1]
    sq_pad = (s + 127) // 128 * 128
    sk_pad = (s + 3 + 63) // 64 * 64
    qd = _pad_heads(q, sq_pad).to(dev)
    kd = _pad_heads(k, sk_pad, key_side=True).to(dev)
    vtd = _pad_heads(v, sk_pad, key_side=True).transpose(2, 3)[..., _vt_perm(sk_pad)].contiguous().to(dev)
    og = guarded((b * s, h * w), fmt.dtype, dev, name="out")
    _hip.check(fmt.fn(lib, "sat_attention_window_bf16")(_hip.ptr(qd), _hip.ptr(kd), _hip.ptr(vtd), _hip.ptr(og.t), b, h, kvh, s, sq_pad, sk_pad, ks,
                                                        scale, _hip.stream()))
    torch.cuda.synchronize()
    og.check().assert_written()
    return og.t.view(b, s, h * w)


def _attention_f32(dev, q, k, v, ks, scale):
    _hip, lib = _lib()
    (b, h, s, w), kvh = q.shape, k.shape[1]
    og = guarded((b * s, h * w), torch.float32, dev, name="out")
    qd, kd, vd = (t.to(dev) for t in (q, k, v))
    _hip.check(lib.sat_attention_f32_window(_hip.ptr(qd), _hip.ptr(kd), _hip.ptr(vd), _hip.ptr(og.t), b, h, kvh, s, ks, scale, _hip.stream()))
    torch.cuda.synchronize()
    og.check().assert_written()
    return og.t.view(b, s, h * w)


def _per_query(x, h):
    b, s, _ = x.shape
    return x.view(b, s, h, -1)          # keep_dims (0, 1, 2): one slice per (sequence, query, head)


# ------------------------------------------------------------------------------- the launchers alone
@pytest.mark.parametrize("fmt", FORMATS, ids=repr)
@pytest.mark.parametrize("unscaled", [False, True], ids=["scale_1/8", "scale_1"])
@pytest.mark.parametrize("s,ks", UNIT_CASES)
def test_attention_window(dev, s, ks, unscaled, fmt):
    """The gates of test_attention, unchanged: fmt.tol(5e-3) against the matched-rounding reference, whole and per (sequence, query, head),
    and fmt.tol(1e-2) against the exact one."""
    q, k, v, scale = NU.unit_tensors(fmt, B, HEADS, KVH, s, unscaled)
    want = NU.window_attention(q, k, v, ks, scale, rnd=fmt.round).float()
    exact = NU.window_attention(q, k, v, ks, scale).float()
    out = _attention(dev, fmt, q, k, v, ks, scale)
    e, ex = rel_l2(out, want), rel_l2(out, exact)
    print(f"\n[attention_window K={ks} scale {scale:g} {fmt} {B}x{HEADS}/{KVH}x{s}] rel-L2 vs matched rounding {e:.2e} "
          f"(gate {fmt.tol(5e-3):.1e}), vs exact {ex:.2e} (gate {fmt.tol(1e-2):.1e})")
    assert_close(f"attention_window K={ks} s={s}", out, want, fmt.tol(5e-3))
    assert_close_sliced(f"attention_window K={ks} s={s} per (sequence, query, head)", _per_query(out, HEADS), _per_query(want, HEADS), fmt.tol(5e-3),
                        (0, 1, 2), fmt.round)
    assert ex < fmt.tol(1e-2)


@pytest.mark.parametrize("scale", [1.0, 0.125])
@pytest.mark.parametrize("s,ks", UNIT_CASES)
def test_attention_f32_window(dev, s, ks, scale):
    """sat_attention_f32_window against float64 at the 1e-5 gate of the fp32 suite, whole and per (sequence, query, head)."""
    rand = lambda shape, sd: torch.randn(shape, generator=torch.Generator().manual_seed(sd))
    g = 1.0 if scale != 1.0 else 8.0 ** -0.5          # the same logit spread under both scales
    q, k, v = rand((B, HEADS, s, W), 21) * g, rand((B, KVH, s, W), 22) * g, rand((B, KVH, s, W), 23)
    v[1] *= 8.0          # a row taken from the neighbouring sequence dominates
    want = NU.window_attention(q, k, v, ks, scale).float()
    out = _attention_f32(dev, q, k, v, ks, scale)
    e = assert_close(f"attention_f32_window K={ks} s={s}", out, want, 1e-5)
    assert_close_sliced(f"attention_f32_window K={ks} s={s} per (sequence, query, head)", _per_query(out, HEADS), _per_query(want, HEADS), 1e-5, (0, 1, 2))
    print(f"\n[attention_f32_window K={ks} s={s} scale {scale:g}] rel-L2 vs float64 {e:.2e} (gate 1.0e-05)")


# queries [a, b] of s = 645 at K: the bounds sit at the edge of a wave (32), of a 32-key block, of a tile (64) and of a workgroup (256)
RANGES = [(33, 32, 63), (33, 64, 127), (7, 96, 159), (129, 256, 511), (65, 0, 255), (7, 512, 644)]


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
def test_keys_outside_the_windows_do_not_reach_the_output(dev, ks, a, b, fmt):
    s = 645
    q, k, v, scale = NU.unit_tensors(fmt, B, HEADS, KVH, s, unscaled=True)
    first = _attention(dev, fmt, q, k, v, ks, scale)
    k2, v2, lo, hi = _rewritten(k, v, s, ks, a, b, fmt.dtype)
    second = _attention(dev, fmt, q, k2, v2, ks, scale)
    assert_bit_equal(f"attention_window K={ks}: queries {a}..{b} after the keys outside [{lo}, {hi}) changed", second[:, a:b + 1], first[:, a:b + 1])
    rest = torch.ones(s, dtype=torch.bool)
    rest[a:b + 1] = False
    assert not torch.equal(second[:, rest], first[:, rest])          # the other queries did see them


def test_f32_keys_outside_the_windows_do_not_reach_the_output(dev):
    s, ks, a, b = 301, 33, 64, 127
    rand = lambda shape, sd: torch.randn(shape, generator=torch.Generator().manual_seed(sd))
    q, k, v = rand((B, HEADS, s, W), 21) * 0.35, rand((B, KVH, s, W), 22) * 0.35, rand((B, KVH, s, W), 23)
    first = _attention_f32(dev, q, k, v, ks, 1.0)
    k2, v2, lo, hi = _rewritten(k, v, s, ks, a, b, torch.float32)
    second = _attention_f32(dev, q, k2, v2, ks, 1.0)
    assert_bit_equal(f"attention_f32_window: queries {a}..{b} after the keys outside [{lo}, {hi}) changed", second[:, a:b + 1], first[:, a:b + 1])
    assert not torch.equal(second[:, :a], first[:, :a])


@pytest.mark.parametrize("fmt", FORMATS, ids=repr)
@pytest.mark.parametrize("ks", [7, 129])
def test_attention_window_all_scores_strongly_negative(dev, ks, fmt):
    """test_attention_all_scores_strongly_negative under the window, at s = 645.  Queries 0..31 and 400..431 are anti-aligned with every key
    (logits below -88): the first block a lane sees has to SET its softmax reference, or every p flushes to 0 and the row divides by a zero
    sum.  That block is not the wave's first: at K = 7 the waves of the queries 384..447 walk blocks that show some of their lanes no key
    at all -- their (m, l, O) = (-1e30, 0, 0) has to survive the redo that the other lanes' first keys trigger; at K = 129 the rows
    400..414 meet their maximum (key 350) in an earlier tile than their own."""
    b, h, kvh, s = 2, 2, 2, 645
    rand = lambda shape, sd: torch.randn(shape, generator=torch.Generator().manual_seed(sd))
    base = F.normalize(rand((W,), 300), dim=0)
    k = (base[None, None, None, :] * 12.0 + 0.03 * rand((b, kvh, s, W), 301)).to(fmt.dtype)
    q = rand((b, h, s, W), 302) * 1.5
    neg = torch.cat([torch.arange(32), torch.arange(400, 432)])
    q[:, :, neg] = -base * 150.0 + 0.03 * rand((b, h, 64, W), 303)
    if ks == 129:
        k[0, :, 350] = k[0, :, 350] * 0.62          # the maximum of the rows 400..414 of sequence 0 (their windows start at 336..350)
    v = rand((b, kvh, s, W), 304).to(fmt.dtype)
    q = q.to(fmt.dtype)
    scores = torch.einsum("bhid,bhjd->bhij", q.float(), k.float()) / math.sqrt(W)
    assert scores[:, :, neg].max().item() < -88, "the negative rows must have every logit below -87 (2^-126 in the log2 domain)"
    if ks == 129:
        assert int(scores[0, 0, 400, 336:465].argmax()) + 336 == 350
    want = NU.window_attention(q, k, v, ks, 0.125, rnd=fmt.round).float()
    out = _attention(dev, fmt, q, k, v, ks, 0.125)
    rest = torch.ones(s, dtype=torch.bool)
    rest[neg] = False
    gate_neg = 2e-2 if not fmt.f16 else 5e-3          # (the gates of the full-attention test)
    e0 = assert_close(f"attention_window K={ks}, all-negative rows", out[:, neg], want[:, neg], gate_neg)
    e1 = assert_close(f"attention_window K={ks}, ordinary rows", out[:, rest], want[:, rest], fmt.tol(5e-3))
    got4, want4 = _per_query(out, h), _per_query(want, h)
    assert_close_sliced(f"attention_window K={ks}, all-negative rows per (sequence, query, head)", got4[:, neg], want4[:, neg], gate_neg, (0, 1, 2), fmt.round)
    assert_close_sliced(f"attention_window K={ks}, ordinary rows per (sequence, query, head)", got4[:, rest], want4[:, rest], fmt.tol(5e-3), (0, 1, 2),
                        fmt.round)
    print(f"\n[attention_window K={ks} {fmt} strongly negative] rel-L2 negative rows {e0:.2e}, ordinary rows {e1:.2e}")


# ------------------------------------------------------------------------------- the plan
@pytest.mark.parametrize("name", list(NC.CASES))
def test_dit_natten_vs_reference(dev, name):
    """Measured (profiles/dit_natten_verification.txt): fp16 1.2e-4 - 3.6e-4 at CFG 1 (gate 6.3e-4), 5.2e-4 - 1.2e-3 at CFG 7 (gate 3.0e-3); fp32x
    5e-7 - 3.2e-6.  Under SAT_TEST_DTYPE=bf16: 8.8e-4 - 2.3e-3 at CFG 1 and 4.1e-3 - 9.1e-3 at CFG 7 (gates 2.5e-3, 1.2e-2) -- except
    k7_cfg1_T64 at 2.84e-3, which MISSES the 2.5e-3 gate in bf16 (it passes in fp16 and in fp32x, so no index is wrong; the reference itself
    with bf16-rounded operands is 4.42e-3 from its fp32 output on this case, against 3.6e-3 - 4.0e-3 on the others at CFG 1: a row averages
    over 7 keys, so operand rounding is diluted less -- what the first rows of the causal family show).  The gates are the harness's and are
    kept."""
    H.check_vs_reference(dev, name, SUITE.gemm_dtype, H.gate(name), rounded=True)


@pytest.mark.parametrize("name", ["k7_cfg7_T296", "k33_cfg7_T296", "k129_cfg7_T640", "k255_cfg7_T640", "k69_cfg7_T64", "qk_cfg1_T64", "adaln_cfg1_T301",
                                  "adaln_k65_cfg1_T65", "conf_cfg7_T296", "patch2_cfg7_T592", "norope_sin_cfg7_T296", "concat_cfg7_T296"])
def test_dit_natten_fp32x_vs_reference(dev, name):
    """The fp32 verification mode on the fp32 window kernel: an indexing error does not hide behind 16-bit rounding."""
    H.check_vs_reference(dev, name, "fp32x", FP32X_GATE)


@pytest.mark.parametrize("name", ["k33_cfg7_T296", "k129_cfg7_T640"])
def test_per_block_formats(dev, name):
    H.check_per_block_formats(dev, name)


@pytest.mark.parametrize("dtype", ["suite", "fp32x"])
@pytest.mark.parametrize("name", ["k33_cfg7_T296", "adaln_cfg1_T301", "k255_cfg7_T640"])
def test_fused_denoise_matches_forward(dev, name, dtype):
    H.check_fused_denoise(dev, name, dtype)


@pytest.mark.parametrize("name", ["k33_cfg7_T296", "concat_cfg7_T296"])
def test_both_layernorm_routes(dev, name):
    """The LayerNorm fold and the standalone kernels both pass the case's gate."""
    a = H.check_vs_reference(dev, name, SUITE.gemm_dtype, H.gate(name), label="LayerNorm fold")
    b = H.check_vs_reference(dev, name, SUITE.gemm_dtype, H.gate(name), label="standalone LayerNorms", ln_fold=False)
    assert not torch.equal(a, b)


def test_the_window_is_not_the_full_attention(dev):
    """The same weights with natten_kernel_size=None give another output: the option reaches the kernels."""
    name = "k33_cfg1_T64"
    from stable_audio_tools.models import _init
    from stable_audio_tools.models.dit import DiffusionTransformer
    with _init.skip_init():
        full = DiffusionTransformer(**NC.without_natten(NC.CONFIGS["k33"]), **NC.FAMILY.product_kwargs)
    full.load_state_dict(H.model("k33", dev).state_dict(), strict=True)
    full = full.to(dev).eval()
    x, t, kw = H.inputs(name, dev)
    assert rel_l2(full(x, t, **kw), H.gold()[name]) > 0.15          # (the generator measured 0.28)


def test_a_short_sequence_is_refused_before_any_launch(dev):
    """27 tokens + the global token + 4 prepend rows = 32 < 33: ValueError from forward, and the plan keeps running."""
    m = H.model("k33", dev)
    x, t, kw = H.inputs("k33_cfg1_T64", dev)
    want = m(x, t, **kw)
    with pytest.raises(ValueError, match="natten_kernel_size=33"):
        m(x[:, :, :27].contiguous(), t, **kw)
    assert_bit_equal("after the refused call", m(x, t, **kw), want)


def test_reports(dev):
    """residual_stream_report and activation_range_report(True) return finite rows on a neighbourhood plan, and the output is bit-identical
    with the range report on."""
    m = H.model("k33", dev)
    x, t, kw = H.inputs("k33_cfg7_T296", dev)
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
    assert_bit_equal("k33: the output with the range report on", got, want)
    assert len(rows) == 3 * 12
    for r in rows:
        assert math.isfinite(r["max_abs"]) and r["nonfinite"] == 0 and r["over_fp16"] == 0, r
        if not r["buffer"].startswith(("cross_", "a_cross")):
            assert r["elements"] > 0 and r["max_abs"] > 0, r


@pytest.mark.parametrize("name,dtype", [(n, d) for n in ("k7_cfg7_T296", "k33_cfg7_T296", "k129_cfg7_T640") for d in ("suite", "fp32x")])
def test_workspace_contents_do_not_matter(dev, name, dtype):
    """Every fill of util.WORKSPACE_FILLS in the workspace before the call, and the call behind a larger one, bit for bit: a tile that is
    not walked or a skipped block must not turn into a read of what the buffer held."""
    from test_gpu_state_independence import check_poisoned_workspace
    m = H.model(NC.CASES[name][0], dev)
    x, t, kw = H.inputs(name, dev)
    try:
        m.set_gemm_dtype(SUITE.gemm_dtype if dtype == "suite" else dtype)
        check_poisoned_workspace(f"{name} ({dtype})", lambda: m(x, t, **kw), m)
    finally:
        m.set_gemm_dtype(SUITE.gemm_dtype)


@pytest.mark.parametrize("dtype", ["suite", "fp32x"])
@pytest.mark.parametrize("cfg_name,small,large", [("k33", "k33_cfg1_T64", "k33_cfg7_T296"), ("k129", "k129_cfg7_T296", "k129_cfg7_T640")])
def test_behind_a_larger_call(dev, cfg_name, small, large, dtype):
    """The small case, the larger case of the same model (more sequences, more rows: every buffer of the workspace is left full of its
    values, beyond the small case's pads and unwalked tiles), the small case again: the same bits."""
    m = H.model(cfg_name, dev)
    xs, ts, kws = H.inputs(small, dev)
    xl, tl, kwl = H.inputs(large, dev)
    try:
        m.set_gemm_dtype(SUITE.gemm_dtype if dtype == "suite" else dtype)
        want = m(xs, ts, **kws).clone()
        m(xl, tl, **kwl)
        got = m(xs, ts, **kws)
        torch.cuda.synchronize()
        assert_bit_equal(f"{small} ({dtype}) behind {large}", got, want)
    finally:
        m.set_gemm_dtype(SUITE.gemm_dtype)


def test_neighborhood_attention_after_finalize(dev):
    """SAT_E_STATE on a finalized plan, and the plan keeps running."""
    _hip, lib = _lib()
    m = H.model("k33", dev)
    x, t, kw = H.inputs("k33_cfg1_T64", dev)
    want = m(x, t, **kw)
    o = _hip.SatDitNeighborhoodOptions(0)
    assert lib.sat_dit_plan_set_neighborhood_attention(m._ensure_plan(), ctypes.byref(o), ctypes.sizeof(o)) == -5
    assert b"finalized" in lib.sat_last_error()
    assert_bit_equal("after the refused call", m(x, t, **kw), want)


def test_generate_diffusion_cond_with_a_neighbourhood_model(dev):
    """generate_diffusion_cond on a reduced config-built model with natten_kernel_size 7 behind "allow_natten": true and no cross-attention
    (the timing numbers stay as global conditioning): 4 steps of dpmpp-3m-sde; finite audio of the right shape, two runs with one seed are
    bit-identical, the same weights with full attention give other audio, and a sample too short for the window is a ValueError."""
    import stable_audio_tools as S
    from dit_family_host import model_config
    from stable_audio_tools import synthetic
    from stable_audio_tools.inference.generation import generate_diffusion_cond
    from stable_audio_tools.models import _init

    def build(**keys):
        cfg = model_config(cond_token_dim=0, **keys)
        cfg["model"]["diffusion"]["cross_attention_cond_ids"] = []
        with _init.skip_init():
            return cfg, S.create_model_from_config(cfg)

    cfg, model = build(attn_kwargs={"natten_kernel_size": 7}, allow_natten=True)
    assert model.model.model.transformer.natten_kernel_size == 7
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
