"""Causal DiTs (ContinuousTransformer causal=True behind allow_causal) on the device: the three causal attention launchers alone
(csrc/attention.hip, attention_hdw.hip, f32_ref.hip through sat_attention_causal_* / sat_attention_f32_causal) against the float64 references
of tests/dit_causal_units.py at the gates of the non-causal unit tests of the same kernels, that no key above the diagonal reaches an
output, the softmax reference when a wave group meets queries without a visible key, then the plan against the REFERENCE's own outputs
(tests/golden/dit_causal_small*.npz: tests/golden/make_golden_dit_causal.py) through the family harness, the reports, poisoned workspaces
and generate_diffusion_cond."""
import ctypes
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import dit_causal_cases as CC  # noqa: E402
import dit_causal_units as CU  # noqa: E402
from dit_family_gpu import FP32X_GATE, Harness  # noqa: E402
from dit_head_width_units import _pad_heads, _vt_perm  # noqa: E402
from util import FORMATS, SUITE, assert_bit_equal, assert_close, assert_close_sliced, guarded, rel_l2  # noqa: E402

pytestmark = pytest.mark.gpu
WIDTHS = (32, 64, 96, 128)
H = Harness(CC.FAMILY)
B, HEADS, KVH = 4, 4, 2          # four sequences: the key shifts (b * s) & 3 take every value for an odd s; GQA 2:1


def _lib():
    from stable_audio_tools import _hip
    return _hip, _hip.lib()


def _attention(dev, fmt, q, k, v, prescaled=True):
    """q [b, h, s, W] as the producer stores it, k / v [b, kvh, s, W], all in fmt.dtype -> [b, s, h * W] between guard bands"""
    _hip, lib = _lib()
    (b, h, s, w), kvh = q.shape, k.shape[1]
    sq_pad = (s + 127) // 128 * 128
    kt = CU.KEY_TILE[w]
    sk_pad = (s + 3 + kt - 1) // kt * kt
    qd = _pad_heads(q, sq_pad).to(dev)
    kd = _pad_heads(k, sk_pad, key_side=True).to(dev)
    vtd = _pad_heads(v, sk_pad, key_side=True).transpose(2, 3)[..., _vt_perm(sk_pad)].contiguous().to(dev)
    og = guarded((b * s, h * w), fmt.dtype, dev, name="out")
    _hip.check(fmt.fn(lib, "sat_attention_causal_bf16")(_hip.ptr(qd), _hip.ptr(kd), _hip.ptr(vtd), _hip.ptr(og.t), b, h, kvh, w, s, sq_pad, sk_pad,
                                                        1 if prescaled else 0, _hip.stream()))
    torch.cuda.synchronize()
    og.check().assert_written()
    return og.t.view(b, s, h * w)


def _per_query(x, h):
    b, s, _ = x.shape
    return x.view(b, s, h, -1)          # keep_dims (0, 1, 2): one slice per (sequence, query, head)


# ------------------------------------------------------------------------------- the launchers alone
@pytest.mark.parametrize("fmt", FORMATS, ids=repr)
@pytest.mark.parametrize("s", CU.SEQ_LENS)
@pytest.mark.parametrize("w,prescaled", [(32, True), (64, True), (64, False), (96, True), (128, True)], ids=lambda v: str(v))
def test_attention_causal(dev, w, prescaled, s, fmt):
    """The gates of test_attention / test_attention_hdw / test_attention_hd128, unchanged: fmt.tol(5e-3) against the matched-rounding
    reference, whole and per (sequence, query, head), and fmt.tol(1e-2) against the exact one."""
    q, q_eff, k, v = CU.unit_tensors(fmt, w, B, HEADS, KVH, s, prescaled=prescaled)
    want = CU.causal_attention(q_eff, k, v, rnd=fmt.round).float()
    exact = CU.causal_attention(q_eff, k, v).float()
    out = _attention(dev, fmt, q, k, v, prescaled)
    e, ex = rel_l2(out, want), rel_l2(out, exact)
    print(f"\n[attention_causal W={w} {'pre-scaled' if prescaled else 'plain'} Q {fmt} {B}x{HEADS}/{KVH}x{s}] rel-L2 vs matched rounding {e:.2e} "
          f"(gate {fmt.tol(5e-3):.1e}), vs exact {ex:.2e} (gate {fmt.tol(1e-2):.1e})")
    assert_close(f"attention_causal W={w} s={s}", out, want, fmt.tol(5e-3))
    assert_close_sliced(f"attention_causal W={w} s={s} per (sequence, query, head)", _per_query(out, HEADS), _per_query(want, HEADS), fmt.tol(5e-3),
                        (0, 1, 2), fmt.round)
    assert ex < fmt.tol(1e-2)


@pytest.mark.parametrize("s", CU.SEQ_LENS)
@pytest.mark.parametrize("w", [32, 64, 96])
def test_attention_f32_causal(dev, w, s):
    """sat_attention_f32_causal against float64 at the 1e-5 gate of the fp32 suite, whole and per (sequence, query, head)."""
    _hip, lib = _lib()
    rand = lambda shape, sd: torch.randn(shape, generator=torch.Generator().manual_seed(sd))
    q, k, v = rand((B, HEADS, s, w), 21), rand((B, KVH, s, w), 22), rand((B, KVH, s, w), 23)
    v[1] *= 8.0          # a row taken from the neighbouring sequence dominates
    want = CU.causal_attention(q, k, v).float()
    og = guarded((B * s, HEADS * w), torch.float32, dev, name="out")
    qd, kd, vd = (t.to(dev) for t in (q, k, v))
    _hip.check(lib.sat_attention_f32_causal(_hip.ptr(qd), _hip.ptr(kd), _hip.ptr(vd), _hip.ptr(og.t), B, HEADS, KVH, w, s, _hip.stream()))
    torch.cuda.synchronize()
    og.check().assert_written()
    out = og.t.view(B, s, HEADS * w)
    e = assert_close(f"attention_f32_causal W={w} s={s}", out, want, 1e-5)
    assert_close_sliced(f"attention_f32_causal W={w} s={s} per (sequence, query, head)", _per_query(out, HEADS), _per_query(want, HEADS), 1e-5, (0, 1, 2))
    print(f"\n[attention_f32_causal W={w} s={s}] rel-L2 vs float64 {e:.2e} (gate 1.0e-05)")


@pytest.mark.parametrize("fmt", FORMATS, ids=repr)
@pytest.mark.parametrize("w", WIDTHS)
@pytest.mark.parametrize("s,i0", [(301, 31), (301, 127), (301, 255), (645, 383)])
def test_no_leak_from_the_future(dev, s, i0, w, fmt):
    """K and V of the keys above i0 (i0 + 1 a multiple of 32: the edge of a wave, of a key block and, at 127 / 255 / 383, of a tile and a
    workgroup) rewritten with other finite values: the outputs of the queries <= i0 keep every bit."""
    q, _, k, v = CU.unit_tensors(fmt, w, B, HEADS, KVH, s)
    first = _attention(dev, fmt, q, k, v)
    k2, v2 = k.clone(), v.clone()
    rand = lambda shape, sd: torch.randn(shape, generator=torch.Generator().manual_seed(sd))
    k2[:, :, i0 + 1:] = (rand(k2[:, :, i0 + 1:].shape, 77) * 40.0).to(fmt.dtype)          # large scores: a leaked key would take the row
    v2[:, :, i0 + 1:] = (rand(v2[:, :, i0 + 1:].shape, 78) * 100.0).to(fmt.dtype)
    second = _attention(dev, fmt, q, k2, v2)
    assert_bit_equal(f"attention_causal W={w} s={s}: queries <= {i0} after the keys above them changed", second[:, :i0 + 1], first[:, :i0 + 1])
    assert not torch.equal(second[:, i0 + 1:], first[:, i0 + 1:])          # the later queries did see them


def test_f32_no_leak_from_the_future(dev):
    _hip, lib = _lib()
    w, s, i0 = 64, 301, 127
    rand = lambda shape, sd: torch.randn(shape, generator=torch.Generator().manual_seed(sd))
    q, k, v = rand((B, HEADS, s, w), 21), rand((B, KVH, s, w), 22), rand((B, KVH, s, w), 23)
    outs = []
    for rewrite in (False, True):
        if rewrite:
            k, v = k.clone(), v.clone()
            k[:, :, i0 + 1:] = rand(k[:, :, i0 + 1:].shape, 77) * 40.0
            v[:, :, i0 + 1:] = rand(v[:, :, i0 + 1:].shape, 78) * 100.0
        og = guarded((B * s, HEADS * w), torch.float32, dev, name="out")
        qd, kd, vd = (t.to(dev) for t in (q, k, v))
        _hip.check(lib.sat_attention_f32_causal(_hip.ptr(qd), _hip.ptr(kd), _hip.ptr(vd), _hip.ptr(og.t), B, HEADS, KVH, w, s, _hip.stream()))
        torch.cuda.synchronize()
        outs.append(og.check().assert_written().t.view(B, s, HEADS * w).clone())
    assert_bit_equal("attention_f32_causal: queries <= 127 after the keys above them changed", outs[1][:, :i0 + 1], outs[0][:, :i0 + 1])


@pytest.mark.parametrize("fmt", FORMATS, ids=repr)
@pytest.mark.parametrize("w", WIDTHS)
def test_attention_causal_all_scores_strongly_negative(dev, w, fmt):
    """test_attention_hdw_all_scores_strongly_negative under the mask, at s = 645: with 64-channel heads the launcher splits the walked tiles
    over two wave groups, and group 1 of the first workgroup meets queries that see none of its keys -- its (m, l, O) = (-1e30, 0, 0) has to
    merge to group 0's result.  Queries 0..31 are anti-aligned with every key (logits below -88): the first block of the sequence has to SET
    the softmax reference, or every p flushes to 0 and the row divides by a zero sum; queries 400..431 likewise, with their maximum at key
    150, in an earlier tile than their own."""
    b, h, kvh, s = 2, 2, 2, 645
    rand = lambda shape, sd: torch.randn(shape, generator=torch.Generator().manual_seed(sd))
    base = F.normalize(rand((w,), 300), dim=0)
    k = (base[None, None, None, :] * 12.0 + 0.03 * rand((b, kvh, s, w), 301)).to(fmt.dtype)
    q = rand((b, h, s, w), 302) * 1.5
    neg = torch.cat([torch.arange(32), torch.arange(400, 432)])
    q[:, :, neg] = -base * 150.0 + 0.03 * rand((b, h, 64, w), 303)
    k[0, :, 150] = k[0, :, 150] * 0.62          # the maximum of the rows 400..431 of sequence 0
    v = rand((b, kvh, s, w), 304).to(fmt.dtype)
    q = (q * CU.qscale(w)).to(fmt.dtype)
    q_eff = q.float() / CU.qscale(w)
    scores = torch.einsum("bhid,bhjd->bhij", q_eff, k.float()) / math.sqrt(w)
    assert scores[:, :, neg].max().item() < -88, "the negative rows must have every logit below -87 (2^-126 in the log2 domain)"
    assert int(scores[0, 0, 400, :401].argmax()) == 150
    want = CU.causal_attention(q_eff, k, v, rnd=fmt.round).float()
    out = _attention(dev, fmt, q, k, v)
    rest = torch.ones(s, dtype=torch.bool)
    rest[neg] = False
    gate_neg = 2e-2 if not fmt.f16 else 5e-3          # (the gates of the non-causal test)
    e0 = assert_close(f"attention_causal W={w}, all-negative rows", out[:, neg], want[:, neg], gate_neg)
    e1 = assert_close(f"attention_causal W={w}, ordinary rows", out[:, rest], want[:, rest], fmt.tol(5e-3))
    got4, want4 = _per_query(out, h), _per_query(want, h)
    assert_close_sliced(f"attention_causal W={w}, all-negative rows per (sequence, query, head)", got4[:, neg], want4[:, neg], gate_neg, (0, 1, 2), fmt.round)
    assert_close_sliced(f"attention_causal W={w}, ordinary rows per (sequence, query, head)", got4[:, rest], want4[:, rest], fmt.tol(5e-3), (0, 1, 2),
                        fmt.round)
    print(f"\n[attention_causal W={w} {fmt} strongly negative] rel-L2 negative rows {e0:.2e}, ordinary rows {e1:.2e}")


# ------------------------------------------------------------------------------- the plan
@pytest.mark.parametrize("name", list(CC.CASES))
def test_dit_causal_vs_reference(dev, name):
    """Measured (profiles/dit_causal_verification.txt): fp16 1.4e-4 - 3.8e-4 at CFG 1 (gate 6.3e-4), 6.1e-4 - 9.4e-4 at CFG 7 (gate 3.0e-3); fp32x
    5e-7 - 1.8e-6.  Under SAT_TEST_DTYPE=bf16: 1.0e-3 - 2.5e-3 at CFG 1 and 4.6e-3 - 7.7e-3 at CFG 7 (gates 2.5e-3, 1.2e-2) -- except
    norope_sin_cfg1_T64 at 2.60e-3, hd96_cfg1_T64 at 3.30e-3 and hd32_patch2_cfg1_T64 at 2.69e-3, which MISS the 2.5e-3 gate in bf16 (they
    pass in fp16 at 3.0e-4 / 3.7e-4 / 3.4e-4 and in fp32x, so no index is wrong; the reference itself with bf16-rounded operands is 4.49e-3 /
    4.78e-3 / 4.61e-3 from its fp32 output on these cases, against 3.6e-3 - 3.8e-3 on the non-causal families: the first rows of a causal
    sequence average over a handful of keys, so operand rounding is diluted less).  The gates are the harness's and are kept."""
    H.check_vs_reference(dev, name, SUITE.gemm_dtype, H.gate(name), rounded=True)


@pytest.mark.parametrize("name", ["plain_cfg7_T296", "qk_cfg1_T64", "adaln_cfg1_T301", "conf_cfg7_T296", "hd32_cfg7_T296", "hd96_cfg7_T296",
                                  "plain_cfg7_T640"])
def test_dit_causal_fp32x_vs_reference(dev, name):
    """The fp32 verification mode on the causal f32_ref kernel: an indexing error does not hide behind 16-bit rounding."""
    H.check_vs_reference(dev, name, "fp32x", FP32X_GATE)


@pytest.mark.parametrize("name", ["plain_cfg7_T296", "hd32_cfg7_T296", "hd128_cfg7_T296"])
def test_per_block_formats(dev, name):
    H.check_per_block_formats(dev, name)


@pytest.mark.parametrize("dtype", ["suite", "fp32x"])
@pytest.mark.parametrize("name", ["plain_cfg7_T296", "adaln_cfg1_T301", "hd96_cfg7_T296"])
def test_fused_denoise_matches_forward(dev, name, dtype):
    H.check_fused_denoise(dev, name, dtype)


@pytest.mark.parametrize("name", ["plain_cfg7_T296", "concat_cfg7_T296"])
def test_both_layernorm_routes(dev, name):
    """The LayerNorm fold and the standalone kernels both pass the case's gate (64-channel heads, "prepend": the plans that fold)."""
    a = H.check_vs_reference(dev, name, SUITE.gemm_dtype, H.gate(name), label="LayerNorm fold")
    b = H.check_vs_reference(dev, name, SUITE.gemm_dtype, H.gate(name), label="standalone LayerNorms", ln_fold=False)
    assert not torch.equal(a, b)


def test_causal_is_not_the_full_attention(dev):
    """The same weights with causal=False give another output: the flag reaches the kernels."""
    name = "plain_cfg1_T64"
    from stable_audio_tools.models import _init
    from stable_audio_tools.models.dit import DiffusionTransformer
    with _init.skip_init():
        full = DiffusionTransformer(**CC.without_causal(CC.CONFIGS["plain"]), **CC.FAMILY.product_kwargs)
    full.load_state_dict(H.model("plain", dev).state_dict(), strict=True)
    full = full.to(dev).eval()
    x, t, kw = H.inputs(name, dev)
    assert rel_l2(full(x, t, **kw), H.gold()[name]) > 0.3          # (the generator measured 0.51)


@pytest.mark.parametrize("cfg_name", ["plain", "hd32"])
def test_reports(dev, cfg_name):
    """residual_stream_report and activation_range_report(True) return finite rows on a causal plan, and the output is bit-identical with the
    range report on."""
    m = H.model(cfg_name, dev)
    x, t, kw = H.inputs(f"{cfg_name}_cfg7_T296", dev)
    want = m(x, t, **kw)
    m.residual_stream_report(True)
    m(x, t, **kw)
    rows = m.residual_stream_report(False)
    assert len(rows) == 3 * 3
    for r in rows:          # (no cross-attention update in a causal model: its rows stay empty)
        assert math.isfinite(r["max_abs"]) and r["saturated"] == 0, r
        assert r["update"] == "cross_attn.to_out" or (r["max_abs"] > 0 and math.isfinite(r["crest"])), r
    m.activation_range_report(True)
    try:
        got = m(x, t, **kw)
        torch.cuda.synchronize()
    finally:
        rows = m.activation_range_report(False)
    assert_bit_equal(f"{cfg_name}: the output with the range report on", got, want)
    assert len(rows) == 3 * 12
    for r in rows:
        assert math.isfinite(r["max_abs"]) and r["nonfinite"] == 0 and r["over_fp16"] == 0, r
        if not r["buffer"].startswith(("cross_", "a_cross")):          # no cross-attention in a causal model
            assert r["elements"] > 0 and r["max_abs"] > 0, r


@pytest.mark.parametrize("name,dtype", [(n, d) for n in ("plain_cfg7_T296", "plain_cfg7_T640", "hd32_cfg7_T296", "hd96_cfg7_T296", "hd128_cfg7_T296")
                                        for d in ("suite", "fp32x") if not (d == "fp32x" and n.startswith("hd128"))])          # (128: no fp32 kernels)
def test_workspace_contents_do_not_matter(dev, name, dtype):
    """Every fill of util.WORKSPACE_FILLS in the workspace before the call, bit for bit: a skipped tile or block must not turn into a read of
    what the buffer held."""
    from test_gpu_state_independence import check_poisoned_workspace
    m = H.model(CC.CASES[name][0], dev)
    x, t, kw = H.inputs(name, dev)
    try:
        m.set_gemm_dtype(SUITE.gemm_dtype if dtype == "suite" else dtype)
        check_poisoned_workspace(f"{name} ({dtype})", lambda: m(x, t, **kw), m)
    finally:
        m.set_gemm_dtype(SUITE.gemm_dtype)


def test_attention_options_after_finalize(dev):
    """SAT_E_STATE on a finalized plan, and the plan keeps running."""
    _hip, lib = _lib()
    m = H.model("plain", dev)
    x, t, kw = H.inputs("plain_cfg1_T64", dev)
    want = m(x, t, **kw)
    o = _hip.SatDitAttentionOptions(0)
    assert lib.sat_dit_plan_set_attention_options(m._ensure_plan(), ctypes.byref(o), ctypes.sizeof(o)) == -5
    assert b"finalized" in lib.sat_last_error()
    assert_bit_equal("after the refused call", m(x, t, **kw), want)


def test_generate_diffusion_cond_with_a_causal_model(dev):
    """generate_diffusion_cond on a reduced config-built model with "causal": true behind "allow_causal": true and no cross-attention (the
    timing numbers stay as global conditioning): 4 steps of dpmpp-3m-sde; finite audio of the right shape, two runs with one seed are
    bit-identical, and the same weights with causal=False give other audio."""
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

    cfg, model = build(causal=True, allow_causal=True)
    assert model.model.model.transformer.causal
    sd = synthetic.synth_state_dict(model.state_dict(), 0)
    ratio, t_len = cfg["model"]["pretransform"]["config"]["downsampling_ratio"], 16

    def run(mod):
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
