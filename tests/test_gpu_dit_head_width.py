"""DiTs with 32- and 96-channel attention heads (embed_dim == 32 or 96 times num_heads, behind allow_head_widths) on the device: the attention
kernel (csrc/attention_hdw.hip), the head split (csrc/head_split_hdw.hip) and the fp32 verification kernels with a head width alone, then the
plan's staged route against the REFERENCE's own outputs (tests/golden/dit_head_width_small*.npz: tests/golden/make_golden_dit_head_width.py)
at the reduced-DiT gates of the harness (tests/dit_family_gpu.py), the fp32 verification mode, per-block formats, the fused
prepare_generation + denoise step and generate_diffusion_cond.  Modelled on test_gpu_dit_head_dim.py; the attention and head-split gates are
those of the 128-channel tests (the same rounding points, the same score spread)."""
import ctypes
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import dit_head_width_cases as WC  # noqa: E402
import mask_edge  # noqa: E402
from dit_family_gpu import FP32X_GATE, Harness, generate, reduced_model  # noqa: E402
from dit_head_width_units import KEY_TILE, _pad_heads, _vt_perm, head_split_reference, qscale, rope_pairs  # noqa: E402
from util import FORMATS, SUITE, assert_close, assert_close_sliced, guarded, rel_l2  # noqa: E402

pytestmark = pytest.mark.gpu
WIDTHS = (32, 96)
H = Harness(WC.FAMILY)


def _lib():
    from stable_audio_tools import _hip
    return _hip, _hip.lib()


def _rand(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def _attention(dev, fmt, q, k, v):
    """q [b, h, sq, W] pre-scaled, k / v [b, kvh, sk, W], all in fmt.dtype -> [b, sq, h * W]"""
    _hip, lib = _lib()
    (b, h, sq, w), kvh, sk = q.shape, k.shape[1], k.shape[2]
    sq_pad = (sq + 127) // 128 * 128
    kt = KEY_TILE[w]
    sk_pad = (sk + 3 + kt - 1) // kt * kt
    qd = _pad_heads(q, sq_pad).to(dev)
    kd = _pad_heads(k, sk_pad, key_side=True).to(dev)
    vtd = _pad_heads(v, sk_pad, key_side=True).transpose(2, 3)[..., _vt_perm(sk_pad)].contiguous().to(dev)
    og = guarded((b * sq, h * w), fmt.dtype, dev, name="out")          # between guard bands, NaN where the kernel has not written
    out = og.t
    _hip.check(fmt.fn(lib, "sat_attention_hdw_bf16")(_hip.ptr(qd), _hip.ptr(kd), _hip.ptr(vtd), _hip.ptr(out), b, h, kvh, w, sq, sk, sq_pad,
                                                     sk_pad, _hip.stream()))
    torch.cuda.synchronize()
    og.check().assert_written()
    return out.view(b, sq, h * w)


def _per_query(x, h):
    b, sq, _ = x.shape
    return x.view(b, sq, h, -1)          # keep_dims (0, 1, 2): one slice per (sequence, query, head)


# Against the key tile KT (128 keys for W = 32, 64 for 96) and the query block of 256:
# (3, 4, 2, 200, 61)     a single key tile with first-tile masking at the key shifts 0, 1, 2
# (2, 2, 2, 78, 78)      self-attention, the second sequence at the shift (b * S) & 3 = 2
# (2, H, H/2, 78, 130)   GQA, the kv-head index is not constant; 2 (W = 32) / 3 (W = 96) key tiles
# (1, 4, 2, 40, 450)     3 / 7 full key tiles and a partial one; W = 32: the last tile's fourth 32-key block is skipped, its third is partial
# (1, 2, 2, 1025, 1025)  9 / 17 tiles, a one-row query tail past four query blocks
def _shapes(w):
    return [(3, 4, 2, 200, 61), (2, 2, 2, 78, 78), (2, 8, 4, 78, 130) if w == 32 else (2, 4, 2, 78, 130), (1, 4, 2, 40, 450), (1, 2, 2, 1025, 1025)]


@pytest.mark.parametrize("fmt", FORMATS, ids=repr)
@pytest.mark.parametrize("w,shape", [(w, s) for w in WIDTHS for s in _shapes(w)], ids=lambda v: str(v).replace(" ", ""))
def test_attention_hdw(dev, w, shape, fmt):
    """Built like test_gpu_dit_head_dim.py::test_attention_hd128 with W channels: the same rounding points and the same score spread
    (1.5 * 1.5 = 2.25 per unit of q . k / sqrt(d)), hence the same gates."""
    from oracle import dit as odit
    b, h, kvh, sq, sk = shape
    q = (_rand((b, h, sq, w), 12) * 1.5).to(fmt.dtype)
    k = (_rand((b, kvh, sk, w), 13) * 1.5).to(fmt.dtype)
    v = _rand((b, kvh, sk, w), 14).to(fmt.dtype)
    k[0, 0, sk - 1] = q[0, 0, min(5, sq - 1)] * 3          # the running max jumps late in the sequence (rescale branch)
    q = (q.float() * qscale(w)).to(fmt.dtype)              # what the producer stores ...
    q_eff = q.float() / qscale(w)                          # ... and the query it stands for
    want = odit._merge(odit.attention_core(q_eff, k.float(), v.float(), rnd=fmt.round))
    exact = odit._merge(odit.attention_core(q_eff, k.float(), v.float()))
    out = _attention(dev, fmt, q, k, v)
    e, ex = rel_l2(out, want), rel_l2(out, exact)
    print(f"\n[attention_hdw W={w} {fmt} {b}x{h}/{kvh}x{sq}x{sk}] rel-L2 vs matched rounding {e:.2e} (gate {fmt.tol(5e-3):.1e}), vs exact {ex:.2e} "
          f"(gate {fmt.tol(1e-2):.1e})")
    assert_close(f"attention_hdw W={w} {b}x{h}x{sq}x{sk}", out, want, fmt.tol(5e-3))
    assert_close_sliced(f"attention_hdw W={w} {b}x{h}x{sq}x{sk} per (sequence, query, head)", _per_query(out, h), _per_query(want, h), fmt.tol(5e-3),
                        (0, 1, 2), fmt.round)
    assert ex < fmt.tol(1e-2)


@pytest.mark.parametrize("fmt", FORMATS, ids=repr)
@pytest.mark.parametrize("w", WIDTHS)
def test_attention_hdw_all_scores_strongly_negative(dev, w, fmt):
    """test_attention_hd128_all_scores_strongly_negative with W channels: queries 0..31 anti-aligned with every key (logits below -88,
    log2-domain scores below -126), their maximum at key 150, in a later key tile than the first.  The first block of a sequence has to SET
    the softmax reference, or every p flushes to 0 and the row divides by a zero sum."""
    from oracle import dit as odit
    b, h, kvh, sq, sk = 1, 2, 2, 96, 200
    base = F.normalize(_rand((w,), 300), dim=0)
    k = (base[None, None, None, :] * 12.0 + 0.03 * _rand((b, kvh, sk, w), 301)).to(fmt.dtype)
    q = _rand((b, h, sq, w), 302) * 1.5
    q[:, :, :32] = -base * 150.0 + 0.03 * _rand((b, h, 32, w), 303)          # q . k / sqrt(W) ~ -318 (32), -184 (96)
    k[0, :, 150] = k[0, :, 150] * 0.62                                       # the negative rows' maximum
    v = _rand((b, kvh, sk, w), 304).to(fmt.dtype)
    q = (q * qscale(w)).to(fmt.dtype)
    q_eff = q.float() / qscale(w)
    scores = torch.einsum("bhid,bhjd->bhij", q_eff, k.float()) / math.sqrt(w)
    assert scores[:, :, :32].max().item() < -88, "the first 32 queries must have every logit below -87 (2^-126 in the log2 domain)"
    assert int(scores[0, 0, 0].argmax()) == 150
    want = odit._merge(odit.attention_core(q_eff, k.float(), v.float(), rnd=fmt.round))
    out = _attention(dev, fmt, q, k, v)
    e0 = assert_close(f"attention_hdw W={w}, all-negative rows", out[:, :32], want[:, :32], 2e-2 if not fmt.f16 else 5e-3)
    e1 = assert_close(f"attention_hdw W={w}, ordinary rows", out[:, 32:], want[:, 32:], fmt.tol(5e-3))
    got4, want4 = _per_query(out, h), _per_query(want, h)
    assert_close_sliced(f"attention_hdw W={w}, all-negative rows per (sequence, query, head)", got4[:, :32], want4[:, :32],
                        2e-2 if not fmt.f16 else 5e-3, (0, 1, 2), fmt.round)
    assert_close_sliced(f"attention_hdw W={w}, ordinary rows per (sequence, query, head)", got4[:, 32:], want4[:, 32:], fmt.tol(5e-3), (0, 1, 2),
                        fmt.round)
    print(f"\n[attention_hdw W={w} {fmt} strongly negative] rel-L2 negative rows {e0:.2e}, ordinary rows {e1:.2e}")


@pytest.mark.parametrize("fmt", FORMATS, ids=repr)
@pytest.mark.parametrize("sk", [63, 573])
@pytest.mark.parametrize("w", WIDTHS)
def test_attention_hdw_masks_front_pad_keys(dev, w, sk, fmt):
    """mask_edge.py: four sequences at the key shifts 0, 1, 2, 3 (one key tile at 63 keys -- two for the shifts 2 and 3 with W = 96 --, five or
    nine at 573), every real logit strongly negative -- an attended front pad key (score 0, V = 0) takes its whole row.  Gates of the
    all-strongly-negative test, whole and per (sequence, query, head)."""
    case = mask_edge.self_attention_case(fmt, w, sk, prescaled=True)
    out = _attention(dev, fmt, case["q"], case["k"], case["v"])
    gate, h = mask_edge.NEG_GATE[fmt.name], case["h"]
    assert_close(f"attention_hdw W={w}, mask edge, {sk} keys", out, case["want"], gate)
    assert_close_sliced(f"attention_hdw W={w}, mask edge, {sk} keys per (sequence, query, head)", _per_query(out, h), _per_query(case["want"], h), gate,
                        (0, 1, 2), fmt.round)


@pytest.mark.parametrize("fmt", FORMATS, ids=repr)
@pytest.mark.parametrize("qk_norm", [False, True], ids=["plain", "qk_norm"])
@pytest.mark.parametrize("w", WIDTHS)
def test_head_split_hdw(dev, w, fmt, qk_norm):
    """sat_head_split_hdw_*: q, k = rope(normalize(x)) per head of W (32: the whole head in pairs (j, j + 16); 96: channels 0..47 in pairs
    (j, j + 24), 48..95 pass), q times log2(e) / sqrt(W), V^T untouched -- against float64.  Two sequences of 78 rows (the second sequence's
    keys shifted by 2), rows scaled over three decades and one all-zero row; destinations pre-filled with NaN."""
    _hip, lib = _lib()
    b, s, s_pad, h = 2, 78, 128, 2
    d, rh = h * w, rope_pairs(w)
    gen = torch.Generator().manual_seed(171)
    x = torch.randn((b * s, 3 * d), generator=gen)
    x = x * (10.0 ** (torch.rand((b * s, 1), generator=gen) * 3.0 - 2.0))          # row scales 1e-2 .. 1e1
    x[5] = 0.0
    inv_freq = 1.0 / (10000 ** (torch.arange(0, 2 * rh, 2).float() / (2 * rh)))    # RotaryEmbedding(2 rh): rh entries
    q, k, v = head_split_reference(x, b, s, h, w, inv_freq, qk_norm)
    xd, fd = x.to(dev), inv_freq.to(dev)
    guards = (guarded((b, h, s_pad, w), fmt.dtype, dev, name="q"), guarded((b, h, s_pad, w), fmt.dtype, dev, name="k"),
              guarded((b, h, w, s_pad), fmt.dtype, dev, name="v^T"), guarded((2 * s * rh,), torch.float32, dev, name="rope scratch"))
    qd, kd, vtd, scratch = (g_.t for g_ in guards)
    qn = 16 if qk_norm else 0
    dst = (ctypes.c_void_p * 3)(qd.data_ptr(), kd.data_ptr(), vtd.data_ptr())
    kind = (ctypes.c_int32 * 3)(2 | 8 | qn, 2 | 4 | qn, 1 | 4)          # what the plan passes for to_qkv
    _hip.check(fmt.fn(lib, "sat_head_split_hdw_bf16")(_hip.ptr(xd), _hip.ptr(fd), dst, kind, _hip.ptr(scratch), b, s, s_pad, h, w, 3, _hip.stream()))
    torch.cuda.synchronize()
    for g_ in guards:
        g_.check()
    for name, buf in (("q", qd), ("k", kd), ("v^T", vtd)):
        assert torch.isfinite(buf.float()).all(), f"non-finite values in the padded {name} buffer"
    gate = fmt.tol(4e-3)
    eq = assert_close("head split q", qd[:, :, :s], q.float(), gate)
    assert_close_sliced("head split q per (sequence, head, token)", qd[:, :, :s], q.float(), gate, (0, 1, 2), fmt.round)
    assert (qd[:, :, s:] == 0).all(), "Q pads must be zero"
    vtd = vtd[..., _vt_perm(s_pad).to(vtd.device)]
    ek = ev = 0.0
    for i in range(b):
        ob = (i * s) & 3
        ek = max(ek, assert_close("head split k", kd[i, :, ob:ob + s], k[i].float(), gate))
        ev = max(ev, assert_close("head split v^T", vtd[i, :, :, ob:ob + s], v[i].transpose(1, 2).float(), gate))
        assert_close_sliced("head split k per (head, token)", kd[i, :, ob:ob + s], k[i].float(), gate, (0, 1), fmt.round)
        assert_close_sliced("head split v^T per (head, key column)", vtd[i, :, :, ob:ob + s], v[i].transpose(1, 2).float(), gate, (0, 2), fmt.round)
        assert (kd[i, :, :ob] == 0).all() and (kd[i, :, ob + s:] == 0).all(), "K pads must be zero"
        assert (vtd[i, :, :, :ob] == 0).all() and (vtd[i, :, :, ob + s:] == 0).all(), "V^T pads must be zero"
    assert (qd[0, :, 5] == 0).all() and (kd[0, :, 5] == 0).all()          # the all-zero row stays zero (0 / max(0, 1e-12))
    if qk_norm:
        norms = kd[0, :, :s].float().norm(dim=-1)
        norms[:, 5] = 1.0
        assert (norms - 1.0).abs().max() < (4e-3 if fmt.f16 else 2e-2), norms
    if w == 96:
        # channels 48..95 are the normalised (q: pre-scaled) input, untouched by the rotation ...
        xin = x.double().view(b, s, 3, h, w).permute(2, 0, 3, 1, 4)
        if qk_norm:
            xin = xin / xin.norm(dim=-1, keepdim=True).clamp_min(1e-12)
        assert_close("head split q, pass-through channels 48..95", qd[:, :, :s, 48:], (xin[0][..., 48:] * qscale(96)).float(), gate)
        assert_close("head split k, pass-through channels 48..95", kd[0, :, :s, 48:], xin[1][0][..., 48:].float(), gate)
        # ... and the rotation pairs channel j with j + 24: the output is far from the one that pairs j with j + 32
        wrong = head_split_reference(x, b, s, h, w, inv_freq, qk_norm, pair_offset=32)[0]
        assert rel_l2(qd[:, :, :s, :48], wrong.float()[..., :48]) > 25 * gate
    print(f"\n[head_split_hdw W={w} {fmt} qk_norm={qk_norm}] rel-L2 q {eq:.2e} k {ek:.2e} v^T {ev:.2e} (gate {gate:.1e})")


# ------------------------------------------------------------------------------- the fp32 verification kernels with a head width
@pytest.mark.parametrize("w", WIDTHS)
def test_attention_f32_with_head_width(dev, w):
    """sat_attention_f32_hdw against float64 at the 1e-5 per (batch, query, head) gate of tests/fp32_units.py; GQA 4 / 2, two sequences, the
    second one's values 8 times larger (a row taken from the neighbouring sequence dominates)."""
    _hip, lib = _lib()
    b, h, kvh, sq, sk = 2, 4, 2, 78, 130
    q, k, v = _rand((b, h, sq, w), 21), _rand((b, kvh, sk, w), 22), _rand((b, kvh, sk, w), 23)
    v[1] *= 8.0
    kk, vv = (t.double().repeat_interleave(h // kvh, dim=1) for t in (k, v))
    want = torch.softmax(torch.einsum("bhid,bhjd->bhij", q.double(), kk) / math.sqrt(w), dim=-1) @ vv
    want = want.permute(0, 2, 1, 3).reshape(b, sq, h * w)
    og = guarded((b * sq, h * w), torch.float32, dev, name="out")
    qd, kd, vd = (t.to(dev) for t in (q, k, v))
    _hip.check(lib.sat_attention_f32_hdw(_hip.ptr(qd), _hip.ptr(kd), _hip.ptr(vd), _hip.ptr(og.t), b, h, kvh, w, sq, sk, _hip.stream()))
    torch.cuda.synchronize()
    og.check().assert_written()
    out = og.t.view(b, sq, h * w)
    e = assert_close(f"attention_f32 W={w}", out, want.float(), 1e-5)
    assert_close_sliced(f"attention_f32 W={w} per (batch, query, head)", _per_query(out, h), _per_query(want.float(), h), 1e-5, (0, 1, 2))
    print(f"\n[attention_f32 W={w}] rel-L2 vs float64 {e:.2e} (gate 1.0e-05)")


@pytest.mark.parametrize("qk_norm", [False, True], ids=["plain", "qk_norm"])
@pytest.mark.parametrize("w", WIDTHS)
def test_split_heads_f32_with_head_width(dev, w, qk_norm):
    """sat_split_heads_f32_hdw against float64 at 1e-5 per (batch, head, token): q and k rotated (and normalised), v plain."""
    _hip, lib = _lib()
    b, s, h, rh = 2, 37, 3, rope_pairs(w)
    x = _rand((b * s, 3 * h * w), 31)
    x[b * s // 2:] *= 8.0
    inv_freq = 1.0 / (10000 ** (torch.arange(0, 2 * rh, 2).double() / (2 * rh)))
    ang = torch.arange(s, dtype=torch.float64)[:, None] * inv_freq[None, :]
    q, k, v = head_split_reference(x, b, s, h, w, inv_freq, qk_norm, scale=1.0)
    gs = [guarded((b, h, s, w), torch.float32, dev, name=n) for n in "qkv"]
    xd, cs, sn = x.to(dev), ang.cos().float().to(dev), ang.sin().float().to(dev)
    _hip.check(lib.sat_split_heads_f32_hdw(_hip.ptr(xd), *(_hip.ptr(g_.t) for g_ in gs), b, s, 3, h, w, 3, _hip.ptr(cs), _hip.ptr(sn),
                                           3 if qk_norm else 0, _hip.stream()))
    torch.cuda.synchronize()
    for g_, want, name in zip(gs, (q, k, v), "qkv"):
        g_.check().assert_written()
        assert_close(f"split_heads_f32 W={w} {name}", g_.t, want.float(), 1e-5)
        assert_close_sliced(f"split_heads_f32 W={w} {name} per (batch, head, token)", g_.t, want.float(), 1e-5, (0, 1, 2))


# ------------------------------------------------------------------------------- the plan
@pytest.mark.parametrize("name", list(WC.CASES))
def test_dit_head_width_vs_reference(dev, name):
    H.check_vs_reference(dev, name, SUITE.gemm_dtype, H.gate(name), rounded=True)


@pytest.mark.parametrize("name", [f"hd{w}{c}" for w in WIDTHS for c in ("_cfg7_T77", "_qk_cfg1_T64", "_adaln_cfg7_T77", "_mha_cfg7_T77")])
def test_dit_head_width_fp32x_vs_reference(dev, name):
    """The fp32 verification mode on the width-taking f32_ref kernels: an indexing error does not hide behind 16-bit rounding."""
    H.check_vs_reference(dev, name, "fp32x", FP32X_GATE)


@pytest.mark.parametrize("name", ["hd32_cfg7_T77", "hd96_cfg7_T77"])
def test_per_block_formats(dev, name):
    H.check_per_block_formats(dev, name)


@pytest.mark.parametrize("dtype", ["suite", "fp32x"])
@pytest.mark.parametrize("name", [f"hd{w}{c}_cfg7_T77" for w in WIDTHS for c in ("", "_adaln", "_prepend_only")])
def test_fused_denoise_matches_forward(dev, name, dtype):
    H.check_fused_denoise(dev, name, dtype)


@pytest.mark.parametrize("cfg_name", ["hd32", "hd96"])
def test_fusion_switches_change_nothing(dev, cfg_name):
    """set_layernorm_fusion / set_cross_attention_fusion are accepted and have no effect on a plan with 32- or 96-channel heads."""
    name = f"{cfg_name}_cfg7_T77"
    assert torch.equal(H.run(name, dev, SUITE.gemm_dtype), H.run(name, dev, SUITE.gemm_dtype, ln_fold=False, cross_fusion=False))


@pytest.mark.parametrize("cfg_name", ["hd32", "hd96"])
def test_reports(dev, cfg_name):
    """residual_stream_report and activation_range_report(True) return finite rows on such a plan, and the output is bit-identical with the
    range report on."""
    m = H.model(cfg_name, dev)
    x, t, kw = H.inputs(f"{cfg_name}_cfg1_T64", dev)
    c, g = kw["cross_attn_cond"], kw["global_embed"]
    want = m(x, t, cross_attn_cond=c, global_embed=g)
    m.residual_stream_report(True)
    m(x, t, cross_attn_cond=c, global_embed=g)
    rows = m.residual_stream_report(False)
    assert len(rows) == 3 * 3 and all(r["max_abs"] > 0 and math.isfinite(r["crest"]) and r["saturated"] == 0 for r in rows), rows
    m.activation_range_report(True)
    try:
        got = m(x, t, cross_attn_cond=c, global_embed=g)
        torch.cuda.synchronize()
    finally:
        rows = m.activation_range_report(False)
    assert torch.equal(got, want)
    assert len(rows) == 3 * 12
    for r in rows:
        assert math.isfinite(r["max_abs"]) and r["nonfinite"] == 0 and r["over_fp16"] == 0, r
        if r["buffer"] not in ("cross_k", "cross_v"):          # (the cache is scanned when a generation is prepared, the others by every forward)
            assert r["elements"] > 0 and r["max_abs"] > 0, r          # the staged route materialises every buffer, cross_q included


def test_generate_diffusion_cond_with_32_channel_heads(dev):
    """generate_diffusion_cond on a reduced diffusion_cond model with dim_heads 32 behind "allow_head_widths": true in its config: 4 steps of
    dpmpp-3m-sde at CFG 7; finite audio of the right shape, and two runs with one seed are bit-identical."""
    from stable_audio_tools import synthetic
    cfg, model = reduced_model(num_heads=8, allow_head_widths=True)          # embed_dim 256
    assert model.model.model.transformer.dim_heads == 32
    sd = synthetic.synth_state_dict(model.state_dict(), 0)
    run = lambda: generate(model, cfg, dev, sd, steps=4, seed=3)[0]
    a0, a1 = run(), run()
    assert torch.equal(a0, a1)
