"""DiTs with 128-channel attention heads (embed_dim == 128 * num_heads) on the device: the attention kernel (csrc/attention_hdw.hip) and
the head split (csrc/head_split_hdw.hip) at that width alone, then the plan's staged route against the REFERENCE's own outputs
(tests/golden/dit_head_dim_small.npz: tests/golden/make_golden_dit_families.py head_dim) at the reduced-DiT gates of the harness
(tests/dit_family_gpu.py), the fused prepare_generation + denoise step and generate_diffusion_cond."""
import ctypes
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import dit_head_dim_cases as HC  # noqa: E402
import mask_edge  # noqa: E402
from dit_family_gpu import Harness, generate, reduced_model  # noqa: E402
from dit_head_width_units import _pad_heads, _vt_perm  # noqa: E402
from util import FORMATS, SUITE, assert_close, assert_close_sliced, guarded, rel_l2  # noqa: E402

pytestmark = pytest.mark.gpu
QSCALE = 1.4426950408889634 / math.sqrt(128.0)          # log2(e) / sqrt(128): what the head split multiplies into Q
H = Harness(HC.FAMILY)


def _lib():
    from stable_audio_tools import _hip
    return _hip, _hip.lib()


def _rand(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def _attention(dev, fmt, q, k, v):
    """q [b, h, sq, 128] pre-scaled, k / v [b, kvh, sk, 128], all in fmt.dtype -> [b, sq, h * 128]"""
    _hip, lib = _lib()
    (b, h, sq, _), kvh, sk = q.shape, k.shape[1], k.shape[2]
    sq_pad = (sq + 127) // 128 * 128
    sk_pad = (sk + 3 + 63) // 64 * 64
    qd = _pad_heads(q, sq_pad).to(dev)
    kd = _pad_heads(k, sk_pad, key_side=True).to(dev)
    vtd = _pad_heads(v, sk_pad, key_side=True).transpose(2, 3)[..., _vt_perm(sk_pad)].contiguous().to(dev)
    og = guarded((b * sq, h * 128), fmt.dtype, dev, name="out")          # between guard bands, NaN where the kernel has not written
    out = og.t
    _hip.check(fmt.fn(lib, "sat_attention_hd128_bf16")(_hip.ptr(qd), _hip.ptr(kd), _hip.ptr(vtd), _hip.ptr(out), b, h, kvh, sq, sk, sq_pad,
                                                       sk_pad, _hip.stream()))
    torch.cuda.synchronize()
    og.check().assert_written()
    return out.view(b, sq, h * 128)


def _per_query(x, h):
    b, sq, _ = x.shape
    return x.view(b, sq, h, 128)          # keep_dims (0, 1, 2): one slice per (sequence, query, head)


# (3, 2, 1, 200, 61): a single tile with first-tile masking at the key shifts 0, 1, 2; (1, 2, 2, 1025, 1025): 17 tiles, a one-row query tail
@pytest.mark.parametrize("fmt", FORMATS, ids=repr)
@pytest.mark.parametrize("b,h,kvh,sq,sk", [(2, 2, 2, 78, 78), (2, 4, 2, 78, 130), (3, 2, 1, 200, 61), (1, 2, 2, 1025, 1025)])
def test_attention_hd128(dev, b, h, kvh, sq, sk, fmt):
    """Built like test_gpu_kernels.py::test_attention in its pre-scaled form, with 128 channels: the same rounding points and the same
    score spread (1.5 * 1.5 = 2.25 per unit of q . k / sqrt(d)), hence the same gates."""
    from oracle import dit as odit
    q = (_rand((b, h, sq, 128), 12) * 1.5).to(fmt.dtype)
    k = (_rand((b, kvh, sk, 128), 13) * 1.5).to(fmt.dtype)
    v = _rand((b, kvh, sk, 128), 14).to(fmt.dtype)
    k[0, 0, sk - 1] = q[0, 0, min(5, sq - 1)] * 3          # the running max jumps late in the sequence (rescale branch)
    q = (q.float() * QSCALE).to(fmt.dtype)                # what the producer stores ...
    q_eff = q.float() / QSCALE                            # ... and the query it stands for
    want = odit._merge(odit.attention_core(q_eff, k.float(), v.float(), rnd=fmt.round))
    exact = odit._merge(odit.attention_core(q_eff, k.float(), v.float()))
    out = _attention(dev, fmt, q, k, v)
    e, ex = rel_l2(out, want), rel_l2(out, exact)
    print(f"\n[attention_hd128 {fmt} {b}x{h}/{kvh}x{sq}x{sk}] rel-L2 vs matched rounding {e:.2e} (gate {fmt.tol(5e-3):.1e}), vs exact {ex:.2e} "
          f"(gate {fmt.tol(1e-2):.1e})")
    assert_close(f"attention_hd128 {b}x{h}x{sq}x{sk}", out, want, fmt.tol(5e-3))
    assert_close_sliced(f"attention_hd128 {b}x{h}x{sq}x{sk} per (sequence, query, head)", _per_query(out, h), _per_query(want, h), fmt.tol(5e-3),
                        (0, 1, 2), fmt.round)
    assert ex < fmt.tol(1e-2)


@pytest.mark.parametrize("fmt", FORMATS, ids=repr)
def test_attention_hd128_all_scores_strongly_negative(dev, fmt):
    """test_gpu_kernels.py::test_attention_all_scores_strongly_negative with 128 channels: queries 0..31 anti-aligned with every key
    (logits below -88, log2-domain scores below -126), their maximum in the third key tile.  The first block of a sequence has to SET
    the softmax reference, or every p flushes to 0 and the row divides by a zero sum."""
    from oracle import dit as odit
    b, h, kvh, sq, sk = 1, 2, 2, 96, 200
    base = F.normalize(_rand((128,), 300), dim=0)
    k = (base[None, None, None, :] * 12.0 + 0.03 * _rand((b, kvh, sk, 128), 301)).to(fmt.dtype)
    q = _rand((b, h, sq, 128), 302) * 1.5
    q[:, :, :32] = -base * 150.0 + 0.03 * _rand((b, h, 32, 128), 303)          # q . k / sqrt(128) ~ -159
    k[0, :, 150] = k[0, :, 150] * 0.62                                         # the negative rows' maximum (~ -99) sits in the third KV tile
    v = _rand((b, kvh, sk, 128), 304).to(fmt.dtype)
    q = (q * QSCALE).to(fmt.dtype)
    q_eff = q.float() / QSCALE
    scores = torch.einsum("bhid,bhjd->bhij", q_eff, k.float()) / math.sqrt(128.0)
    assert scores[:, :, :32].max().item() < -88, "the first 32 queries must have every logit below -87 (2^-126 in the log2 domain)"
    assert int(scores[0, 0, 0].argmax()) == 150
    want = odit._merge(odit.attention_core(q_eff, k.float(), v.float(), rnd=fmt.round))
    out = _attention(dev, fmt, q, k, v)
    e0 = assert_close("attention_hd128, all-negative rows", out[:, :32], want[:, :32], 2e-2 if not fmt.f16 else 5e-3)
    e1 = assert_close("attention_hd128, ordinary rows", out[:, 32:], want[:, 32:], fmt.tol(5e-3))
    got4, want4 = _per_query(out, h), _per_query(want, h)
    assert_close_sliced("attention_hd128, all-negative rows per (sequence, query, head)", got4[:, :32], want4[:, :32], 2e-2 if not fmt.f16 else 5e-3,
                        (0, 1, 2), fmt.round)
    assert_close_sliced("attention_hd128, ordinary rows per (sequence, query, head)", got4[:, 32:], want4[:, 32:], fmt.tol(5e-3), (0, 1, 2), fmt.round)
    print(f"\n[attention_hd128 {fmt} strongly negative] rel-L2 negative rows {e0:.2e}, ordinary rows {e1:.2e}")


@pytest.mark.parametrize("fmt", FORMATS, ids=repr)
@pytest.mark.parametrize("sk", [63, 573])
def test_attention_hd128_masks_front_pad_keys(dev, sk, fmt):
    """mask_edge.py: four sequences at the key shifts 0, 1, 2, 3 (one and two key tiles at 63 keys, nine at 573), every real logit near
    -159 -- an attended front pad key (score 0, V = 0) takes its whole row.  Gates of the all-strongly-negative test, whole and per
    (sequence, query, head)."""
    case = mask_edge.self_attention_case(fmt, 128, sk, prescaled=True)
    out = _attention(dev, fmt, case["q"], case["k"], case["v"])
    gate, h = mask_edge.NEG_GATE[fmt.name], case["h"]
    assert_close(f"attention_hd128, mask edge, {sk} keys", out, case["want"], gate)
    assert_close_sliced(f"attention_hd128, mask edge, {sk} keys per (sequence, query, head)", _per_query(out, h), _per_query(case["want"], h), gate,
                        (0, 1, 2), fmt.round)


@pytest.mark.parametrize("fmt", FORMATS, ids=repr)
@pytest.mark.parametrize("qk_norm", [False, True], ids=["plain", "qk_norm"])
def test_head_split_hd128(dev, fmt, qk_norm):
    """sat_head_split_hd128_*: q, k = rope(normalize(x)) per head of 128 (rotation of channels 0..63 in pairs (j, j + 32)), q times
    log2(e) / sqrt(128), V^T untouched -- against float64.  Two sequences of 78 rows (the second sequence's keys shifted by 2), rows scaled
    over three decades and one all-zero row; destinations pre-filled with NaN."""
    _hip, lib = _lib()
    b, s, s_pad, d = 2, 78, 128, 256
    h = d // 128
    gen = torch.Generator().manual_seed(171)
    x = torch.randn((b * s, 3 * d), generator=gen)
    x = x * (10.0 ** (torch.rand((b * s, 1), generator=gen) * 3.0 - 2.0))          # row scales 1e-2 .. 1e1
    x[5] = 0.0
    inv_freq = 1.0 / (10000 ** (torch.arange(0, 64, 2).float() / 64))              # RotaryEmbedding(64): 32 entries
    qkv = x.double().view(b, s, 3, h, 128).permute(2, 0, 3, 1, 4)                  # [3][b, h, s, 128]
    q, k, v = qkv[0], qkv[1], qkv[2]
    ang = torch.arange(s, dtype=torch.float64)[:, None] * inv_freq.double()[None, :]          # [s, 32]
    cs, sn = ang.cos(), ang.sin()

    def norm_rope(t):
        if qk_norm:
            t = t / t.norm(dim=-1, keepdim=True).clamp_min(1e-12)          # F.normalize
        x1, x2 = t[..., :32], t[..., 32:64]
        return torch.cat([x1 * cs - x2 * sn, x2 * cs + x1 * sn, t[..., 64:]], dim=-1)

    q, k = norm_rope(q) * QSCALE, norm_rope(k)
    xd, fd = x.to(dev), inv_freq.to(dev)
    guards = (guarded((b, h, s_pad, 128), fmt.dtype, dev, name="q"), guarded((b, h, s_pad, 128), fmt.dtype, dev, name="k"),
              guarded((b, h, 128, s_pad), fmt.dtype, dev, name="v^T"), guarded((2 * s * 32,), torch.float32, dev, name="rope scratch"))
    qd, kd, vtd, scratch = (g_.t for g_ in guards)
    qn = 16 if qk_norm else 0
    dst = (ctypes.c_void_p * 3)(qd.data_ptr(), kd.data_ptr(), vtd.data_ptr())
    kind = (ctypes.c_int32 * 3)(2 | 8 | qn, 2 | 4 | qn, 1 | 4)          # what the plan passes for to_qkv
    _hip.check(fmt.fn(lib, "sat_head_split_hd128_bf16")(_hip.ptr(xd), _hip.ptr(fd), dst, kind, _hip.ptr(scratch), b, s, s_pad, h, 3, _hip.stream()))
    torch.cuda.synchronize()
    for g_ in guards:
        g_.check()
    for name, buf in (("q", qd), ("k", kd), ("v^T", vtd)):
        assert torch.isfinite(buf.float()).all(), f"non-finite values in the padded {name} buffer"
    eq = assert_close("head split q", qd[:, :, :s], q.float(), fmt.tol(4e-3))
    assert_close_sliced("head split q per (sequence, head, token)", qd[:, :, :s], q.float(), fmt.tol(4e-3), (0, 1, 2), fmt.round)
    assert (qd[:, :, s:] == 0).all(), "Q pads must be zero"
    vtd = vtd[..., _vt_perm(s_pad).to(vtd.device)]
    ek = ev = 0.0
    for i in range(b):
        ob = (i * s) & 3
        ek = max(ek, assert_close("head split k", kd[i, :, ob:ob + s], k[i].float(), fmt.tol(4e-3)))
        ev = max(ev, assert_close("head split v^T", vtd[i, :, :, ob:ob + s], v[i].transpose(1, 2).float(), fmt.tol(4e-3)))
        assert_close_sliced("head split k per (head, token)", kd[i, :, ob:ob + s], k[i].float(), fmt.tol(4e-3), (0, 1), fmt.round)
        assert_close_sliced("head split v^T per (head, key column)", vtd[i, :, :, ob:ob + s], v[i].transpose(1, 2).float(), fmt.tol(4e-3), (0, 2), fmt.round)
        assert (kd[i, :, :ob] == 0).all() and (kd[i, :, ob + s:] == 0).all(), "K pads must be zero"
        assert (vtd[i, :, :, :ob] == 0).all() and (vtd[i, :, :, ob + s:] == 0).all(), "V^T pads must be zero"
    assert (qd[0, :, 5] == 0).all() and (kd[0, :, 5] == 0).all()          # the all-zero row stays zero (0 / max(0, 1e-12))
    if qk_norm:
        norms = kd[0, :, :s].float().norm(dim=-1)
        norms[:, 5] = 1.0
        assert (norms - 1.0).abs().max() < (4e-3 if fmt.f16 else 2e-2), norms
    print(f"\n[head_split_hd128 {fmt} qk_norm={qk_norm}] rel-L2 q {eq:.2e} k {ek:.2e} v^T {ev:.2e} (gate {fmt.tol(4e-3):.1e})")


# ------------------------------------------------------------------------------- the plan
@pytest.mark.parametrize("name", list(HC.CASES))
def test_dit_head_dim_vs_reference(dev, name):
    H.check_vs_reference(dev, name, SUITE.gemm_dtype, H.gate(name))


def test_fusion_switches_change_nothing(dev):
    """set_layernorm_fusion / set_cross_attention_fusion are accepted and have no effect on a plan with 128-channel heads (as for adaLN)."""
    name = "hd128_cfg7_T77"
    m = H.model("hd128", dev)
    x, t, kw = H.inputs(name, dev)
    c, g = kw["cross_attn_cond"], kw["global_embed"]
    want = m(x, t, cross_attn_cond=c, global_embed=g, cfg_scale=7.0)
    m.set_layernorm_fusion(False).set_cross_attention_fusion(False)
    try:
        got = m(x, t, cross_attn_cond=c, global_embed=g, cfg_scale=7.0)
        torch.cuda.synchronize()
    finally:
        m.set_layernorm_fusion(True).set_cross_attention_fusion(True)
    assert torch.equal(got, want)


def test_residual_stream_report(dev):
    m = H.model("hd128", dev)
    x, t, kw = H.inputs("hd128_cfg1_T64", dev)
    m.residual_stream_report(True)
    m(x, t, cross_attn_cond=kw["cross_attn_cond"], global_embed=kw["global_embed"])
    rows = m.residual_stream_report(False)
    assert len(rows) == 3 * 3 and all(r["max_abs"] > 0 and math.isfinite(r["crest"]) and r["saturated"] == 0 for r in rows), rows


@pytest.mark.parametrize("name", ["hd128_cfg7_T77", "hd128_adaln_cfg7_T77", "hd128_prepend_only_cfg7_T77"])
def test_fused_denoise_matches_forward(dev, name):
    H.check_fused_denoise(dev, name, "suite")


def test_generate_diffusion_cond_with_128_channel_heads(dev):
    """generate_diffusion_cond on a reduced diffusion_cond model with num_heads=2 (two heads of 128, one kv head): 4 steps of
    dpmpp-3m-sde at CFG 7; finite audio of the right shape, and two runs with one seed are bit-identical."""
    from stable_audio_tools import synthetic
    cfg, model = reduced_model(num_heads=2)
    assert model.model.model.transformer.dim_heads == 128
    sd = synthetic.synth_state_dict(model.state_dict(), 0)
    run = lambda: generate(model, cfg, dev, sd, steps=4, seed=3)[0]
    a0, a1 = run(), run()
    assert torch.equal(a0, a1)
