"""qk_norm, sinusoidal / absolute position embeddings, rotary_pos_emb=False and bias-free feed-forwards on the HIP DiT (reference
models/transformer.py:50-96, 270, 433-436, 796-797) against the REFERENCE's own outputs (tests/golden/dit_options_small.npz:
tests/golden/make_golden_dit_families.py options).  Gates: the harness, tests/dit_family_gpu.py.

* the suite's operand format at the reduced-DiT gates;
* the fp32 verification mode (gemm_dtype "fp32x"): what separates an indexing error (the position of a prepended row, a
  normalisation over the wrong 64 channels, a key shift) from rounding;
* the qk_norm cases again with the LayerNorm fold off and with the fused to_q + cross-attention launch off;
* the normalising QKV step alone (sat_qkv_rope_qknorm_*) against a float64 restatement.
"""
import ctypes
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import dit_options_cases as OC  # noqa: E402
from dit_family_gpu import FP32X_GATE, Harness  # noqa: E402
from util import FORMATS, SUITE, assert_close, assert_close_sliced, guarded  # noqa: E402

pytestmark = pytest.mark.gpu
H = Harness(OC.FAMILY)


@pytest.mark.parametrize("name", list(OC.CASES))
def test_dit_options_vs_reference(dev, name):
    H.check_vs_reference(dev, name, SUITE.gemm_dtype, H.gate(name))


@pytest.mark.parametrize("name", list(OC.CASES))
def test_dit_options_fp32_vs_reference(dev, name):
    H.check_vs_reference(dev, name, "fp32x", FP32X_GATE)


@pytest.mark.parametrize("path", ["ln_fold_off", "cross_fusion_off"])
@pytest.mark.parametrize("name", [n for n, c in OC.CASES.items() if "attn_kwargs" in OC.CONFIGS[c[0]]])
def test_qk_norm_on_the_other_launch_paths(dev, name, path):
    """The standalone LayerNorms in front of the normalising projections, and to_q + attention core as two kernels (the normalised Q
    then goes through memory instead of staying in the fused launch's registers)."""
    H.check_vs_reference(dev, name, SUITE.gemm_dtype, H.gate(name), path, ln_fold=path != "ln_fold_off", cross_fusion=path != "cross_fusion_off")


@pytest.mark.parametrize("dtype", ["suite", "fp32x"])
@pytest.mark.parametrize("name", ["qk_cfg7_T77", "qk_adaln_cfg7_T77", "qk_prepend_only_cfg7_T77", "all_cfg7_T77", "abs_norope_P3_cfg7_T64"])
def test_fused_denoise_matches_forward(dev, name, dtype):
    H.check_fused_denoise(dev, name, dtype)


@pytest.mark.parametrize("name", ["abs_P3_cfg1_T77", "abs_cfg7_T77"])
def test_abs_table_longer_than_the_plan(dev, name):
    """abs_pos_emb_max_length 256 on a plan of max_seq_len 100 (at most 64 + 1 + 100 rows): the table then has the plan's rows, not the
    embedding's -- same weights, same golden as the plan of the default max_seq_len, whose table stops at the embedding's 256 rows."""
    H.check_vs_reference(dev, name, SUITE.gemm_dtype, H.gate(name), "max_seq_len 100", max_seq_len=100)

def test_sequence_longer_than_abs_pos_emb_max_length(dev):
    """The reference's AssertionError (transformer.py:59-61), on the host: forward and the fused path; the C entry point answers
    SAT_E_INVALID with the same sentence before it launches anything; and the options call is refused once the plan is finalized."""
    from stable_audio_tools import _hip
    m = H.model("abs", dev)
    x, t, kw = H.inputs("abs_P3_cfg1_T77", dev)
    c, g, pc, pm = kw["cross_attn_cond"], kw["global_embed"], kw["prepend_cond"], kw["prepend_cond_mask"]
    m(x, t, cross_attn_cond=c, global_embed=g, prepend_cond=pc, prepend_cond_mask=pm)          # 3 + 1 + 77 rows: fine
    long = torch.zeros(2, 64, 255, device=dev)                                                 # 1 + 255 = 256 rows: the last that fits
    assert torch.isfinite(m(long, t, cross_attn_cond=c, global_embed=g)).all()
    with pytest.raises(AssertionError, match="sequence length of 257 .* max sequence length of 256"):
        m(torch.zeros(2, 64, 256, device=dev), t, cross_attn_cond=c, global_embed=g)
    with pytest.raises(AssertionError, match="sequence length of 257 .* max sequence length of 256"):
        m(torch.zeros(2, 64, 253, device=dev), t, cross_attn_cond=c, global_embed=g, prepend_cond=pc, prepend_cond_mask=pm)       # 3 + 1 + 253 rows
    m.prepare_generation(c, g, 1.0, prepend_cond=pc)
    with pytest.raises(AssertionError, match="max sequence length of 256"):
        m.denoise(torch.zeros(2, 64, 253, device=dev), 1.0)
    # the C ABI itself
    lib = _hip.lib()
    m.prepare_generation(c, g, 1.0)
    xl = torch.zeros(2, 64, 256, device=dev)
    out = torch.empty_like(xl)
    ws = m._workspace(2, 256)
    rc = lib.sat_dit_forward(m._plan, _hip.ptr(xl), _hip.ptr(t), _hip.ptr(out), 2, 256, _hip.ptr(ws), ws.numel(), _hip.stream())
    assert rc == -1 and b"sequence length of 257" in lib.sat_last_error()
    opts = _hip.SatDitTransformerOptions(0, 0, 0, 1)
    assert lib.sat_dit_plan_set_transformer_options(m._plan, ctypes.byref(opts), ctypes.sizeof(opts)) == -5
    assert b"finalized" in lib.sat_last_error()
    torch.cuda.synchronize()


def _vt_perm(n):
    p = torch.arange(n)
    return (p & ~12) | ((p & 4) << 1) | ((p & 8) >> 1)


# forced tiles: 1 / 5 the two 128 x 128 kernels with the un-swapped heads epilogue, 15 / 16 / 22 / 30 the ring tiles (transposed epilogue
# for q and k, un-swapped for V^T); 0 = the route's choice
@pytest.mark.parametrize("fmt", FORMATS, ids=repr)
@pytest.mark.parametrize("variant", [0, 1, 5, 15, 16, 22, 30])
def test_qkv_rope_qknorm(dev, variant, fmt):
    """sat_qkv_rope_qknorm_*: q, k = rope(normalize(x W^T)) per head of 64, q times log2(e) / 8, V^T untouched -- against float64 on the
    same rounded operands, at the q / k gate of test_gpu_kernels.py::test_qkv_rope.  Two sequences of 78 rows (an M tail in every tile,
    the second sequence's keys shifted by 2), input rows scaled over three decades and one all-zero row: the normalisation must neither
    depend on the row's scale nor write a non-finite value anywhere in the padded buffers."""
    from stable_audio_tools import _hip
    lib = _hip.lib()
    b, s, s_pad, d = 2, 78, 128, 256
    h = d // 64
    gen = torch.Generator().manual_seed(71)
    a = torch.randn((b * s, d), generator=gen)
    a = a * (10.0 ** (torch.rand((b * s, 1), generator=gen) * 3.0 - 2.0))          # row scales 1e-2 .. 1e1
    a[5] = 0.0
    a = a.to(fmt.dtype)
    w = (torch.randn((3 * d, d), generator=gen) * 0.1).to(fmt.dtype)
    inv_freq = 1.0 / (10000 ** (torch.arange(0, 32, 2).float() / 32))

    qkv = (a.double() @ w.double().T).view(b, s, 3, h, 64).permute(2, 0, 3, 1, 4)          # [3][b, h, s, 64]
    q, k, v = qkv[0], qkv[1], qkv[2]
    ang = torch.arange(s, dtype=torch.float64)[:, None] * inv_freq.double()[None, :]          # [s, 16]
    cs, sn = ang.cos(), ang.sin()

    def norm_rope(x):
        x = x / x.norm(dim=-1, keepdim=True).clamp_min(1e-12)          # F.normalize
        x1, x2 = x[..., :16], x[..., 16:32]
        return torch.cat([x1 * cs - x2 * sn, x2 * cs + x1 * sn, x[..., 32:]], dim=-1)

    q, k = norm_rope(q) * (1.4426950408889634 / 8.0), norm_rope(k)
    ad, wd, fd = a.to(dev), w.to(dev), inv_freq.to(dev)
    guards = (guarded((b, h, s_pad, 64), fmt.dtype, dev, name="q"), guarded((b, h, s_pad, 64), fmt.dtype, dev, name="k"),
              guarded((b, h, 64, s_pad), fmt.dtype, dev, name="v^T"), guarded((2 * s * 16,), torch.float32, dev, name="rope scratch"))
    qd, kd, vtd, scratch = (g_.t for g_ in guards)
    fn = fmt.fn(lib, "sat_qkv_rope_qknorm_bf16")
    _hip.check(fn(_hip.ptr(ad), _hip.ptr(wd), _hip.ptr(fd), _hip.ptr(qd), _hip.ptr(kd), _hip.ptr(vtd), _hip.ptr(scratch), b, s, s_pad, d, variant,
                  _hip.stream()))
    torch.cuda.synchronize()
    for g_ in guards:
        g_.check()
    for name, buf in (("q", qd), ("k", kd), ("v^T", vtd)):
        assert torch.isfinite(buf.float()).all(), f"non-finite values in the padded {name} buffer"
    eq = assert_close("qk_norm q", qd[:, :, :s], q.float(), fmt.tol(4e-3))
    assert_close_sliced("qk_norm q per (sequence, head, token)", qd[:, :, :s], q.float(), fmt.tol(4e-3), (0, 1, 2), fmt.round)
    assert (qd[:, :, s:] == 0).all(), "Q pads must be zero"
    vtd = vtd[..., _vt_perm(s_pad).to(vtd.device)]
    ek = 0.0
    for i in range(b):
        ob = (i * s) & 3
        ek = max(ek, assert_close("qk_norm k", kd[i, :, ob:ob + s], k[i].float(), fmt.tol(4e-3)))
        assert_close("v^T", vtd[i, :, :, ob:ob + s], v[i].transpose(1, 2).float(), fmt.tol(4e-3))
        assert_close_sliced("qk_norm k per (head, token)", kd[i, :, ob:ob + s], k[i].float(), fmt.tol(4e-3), (0, 1), fmt.round)
        assert_close_sliced("qk_norm v^T per (head, key column)", vtd[i, :, :, ob:ob + s], v[i].transpose(1, 2).float(), fmt.tol(4e-3), (0, 2), fmt.round)
        assert (kd[i, :, :ob] == 0).all() and (kd[i, :, ob + s:] == 0).all(), "K pads must be zero"
        assert (vtd[i, :, :, :ob] == 0).all() and (vtd[i, :, :, ob + s:] == 0).all(), "V^T pads must be zero"
    # the all-zero input row stays zero (0 / max(0, 1e-12)), every other head row has unit norm
    assert (qd[0, :, 5] == 0).all() and (kd[0, :, 5] == 0).all()
    norms = kd[0, :, :s].float().norm(dim=-1)
    norms[:, 5] = 1.0
    assert (norms - 1.0).abs().max() < (4e-3 if fmt.f16 else 2e-2), norms
    print(f"\n[qkv_rope_qknorm {fmt} variant {variant}] rel-L2 q {eq:.2e} k {ek:.2e}")


def test_qkv_rope_qknorm_refuses_the_8_phase_kernel(dev):
    """The normalising epilogue lives in the ring tiles: a variant that forces the 8-phase kernel is an error, not a silent un-normalised run."""
    from stable_audio_tools import _hip
    lib = _hip.lib()
    b, s, s_pad, d = 1, 128, 256, 256
    z16 = lambda *shape: torch.zeros(shape, dtype=torch.bfloat16, device=dev)
    a, w, q, k, vt = z16(b * s, d), z16(3 * d, d), z16(b, 4, s_pad, 64), z16(b, 4, s_pad, 64), z16(b, 4, 64, s_pad)
    f = torch.zeros(16, device=dev)
    scratch = torch.empty(2 * s * 16, device=dev)
    rc = lib.sat_qkv_rope_qknorm_bf16(_hip.ptr(a), _hip.ptr(w), _hip.ptr(f), _hip.ptr(q), _hip.ptr(k), _hip.ptr(vt), _hip.ptr(scratch), b, s, s_pad, d, 80,
                                      _hip.stream())
    assert rc == -2 and b"qk_norm" in lib.sat_last_error()
    torch.cuda.synchronize()
