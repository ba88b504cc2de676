"""The sliced gates and the guard bands of tests/util.py bite (CPU only, oracle outputs only): a correctly rounded result passes every
one of them, and each localised defect a kernel can have -- a row, one 32 x 32 accumulator block, one head of one query, an unwritten
tail tile, a store past the output, an attended front pad key -- fails the new check.  Where the whole-tensor gate of assert_close lets
the defect through, that is asserted as well: it records the gap the sliced gates close."""
import math

import pytest
import torch
import torch.nn.functional as F

import mask_edge
from util import FORMATS, assert_close, assert_close_rows_blocks, assert_close_sliced, blocks32, guarded, rel_l2, slice_errors, slice_spread

BF16, F16 = FORMATS


def _rand(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def _fails(fn, *args, **kw):
    try:
        fn(*args, **kw)
    except AssertionError as e:
        return str(e)
    return None


_ATTN = {}


def _attention_layout():
    """The (8, 64, 8, 300, 700) layout of test_gpu_kernels.py::test_attention, [b, sq, h, 64], with a cheap synthetic answer: softmax
    averages of ~700 unit-variance values have a small, query-dependent norm (here 0.02 .. 0.2 per channel)."""
    if not _ATTN:
        b, h, sq = 8, 64, 300
        _ATTN["want"] = _rand((b, sq, h, 64), 600) * (0.02 + 0.18 * torch.rand((b, sq, h, 1), generator=torch.Generator().manual_seed(601)))
    return _ATTN["want"]


def test_slice_errors_definition():
    want = torch.tensor([[3.0, 4.0], [0.0, 0.0], [0.3, 0.4]])
    got = torch.tensor([[3.0, 4.5], [0.1, 0.0], [0.3, 0.4]])
    floor = math.sqrt((25.0 + 0.0 + 0.25) / 3)                     # rms over the slices of ||want_s||
    e = slice_errors(got, want, (0,))
    assert e.shape == (3,)
    assert torch.allclose(e, torch.tensor([0.5 / 5.0, 0.1 / floor, 0.0], dtype=torch.float64))
    # a NaN makes its slice fail whatever the gate, and the message names the slice
    got[2, 1] = float("nan")
    msg = _fails(assert_close_sliced, "t", got, want, 1.0, (0,))
    assert msg and "slice (2,)" in msg
    # ragged 32 x 32 blocks are slices of their own
    x = _rand((70, 100), 1)
    assert blocks32(x).shape == (3, 32, 4, 32)
    e = slice_errors(blocks32(x * 1.01), blocks32(x), (0, 2))
    assert e.shape == (3, 4) and bool((e > 0).all())
    assert slice_spread(x, (0,), None) == 1.0


@pytest.mark.parametrize("fmt", FORMATS, ids=repr)
def test_correctly_rounded_results_pass_every_sliced_gate(fmt):
    """With F_ref as defined the rounding noise of the output format passes per row, per block and per (sequence, query, head), at the
    whole-tensor rel-L2 of that noise as the tolerance -- the tightest tolerance a correct result can be given (1.001: rel_l2 works in fp32)."""
    want = F.layer_norm(_rand((2050, 1536), 1, 2.0) + 0.3, (1536,))
    got = fmt.round(want)
    assert_close_rows_blocks("layernorm-like", got, want, 1.001 * rel_l2(got, want), fmt.round)
    want = _attention_layout()
    got = fmt.round(want)
    _, _, f_ref, _ = assert_close_sliced("attention-like", got, want, 1.001 * rel_l2(got, want), (0, 1, 2), fmt.round)
    assert 1.0 < f_ref < 2.0, f"64-element slices: the rounding noise's worst slice sits {f_ref:.2f}x above the whole"


def test_one_row_replaced_by_its_neighbour():
    want = F.layer_norm(_rand((2050, 1536), 1, 2.0) + 0.3, (1536,))
    got = BF16.round(want)
    got[2049] = got[2048]                                           # the one-row tail of the last 256-row tile
    msg = _fails(assert_close_rows_blocks, "row", got, want, 4e-3, BF16.round)
    assert msg and "slice (2049,)" in msg


def test_one_accumulator_block_scaled():
    a, w = _rand((2050, 256), 5), _rand((1536, 256), 6) * 0.05 + torch.linspace(-0.02, 0.03, 1536)[:, None]
    want = a @ w.T + _rand((1536,), 7)
    got = want.clone()
    got[2048:2050, 1504:1536] *= 1.05                               # a ragged (2-row) block at the corner ...
    msg = _fails(assert_close_sliced, "block", blocks32(got), blocks32(want), 1e-3, (0, 2))
    assert msg and "slice (64, 47)" in msg
    assert _fails(assert_close_rows_blocks, "block", got, want, 1e-3) is not None
    assert_close("block", got, want, 1e-3)                          # ... the whole-tensor gate does not see it
    got = want.clone()
    got[640:672, 320:352] *= 1.05                                   # a full one in the middle
    msg = _fails(assert_close_sliced, "block", blocks32(got), blocks32(want), 1e-3, (0, 2))
    assert msg and "slice (20, 10)" in msg
    assert_close("block", got, want, 1e-3)


def test_one_head_of_one_query_wrong():
    want = _attention_layout()
    for fmt in FORMATS:
        got = fmt.round(want)
        got[5, 299, 17] = got[5, 298, 17]                           # the last query of a sequence takes its neighbour's answer
        msg = _fails(assert_close_sliced, "attention", got, want, fmt.tol(5e-3), (0, 1, 2), fmt.round)
        assert msg and "slice (5, 299, 17)" in msg
    got = BF16.round(want)
    got[5, 299, 17] = got[5, 298, 17]
    assert_close("attention", got.view(8, 300, 4096), want.view(8, 300, 4096), BF16.tol(5e-3))          # 1 of 153 600 slices: invisible at the bf16 gate


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_unwritten_tail_tile_and_guard_bands(dtype):
    m, n = 300, 96
    want = _rand((m, n), 9)
    out = guarded((m, n), dtype, "cpu", name="y")
    assert out.t.data_ptr() % 256 == 0 and out.off >= 256 * n and out.raw.numel() - out.off - out.n >= 256 * n
    # ln_part [m, d / 64, 2]: a row of the GEMM is 2 * d / 64 elements, not the last dimension -- the guard is 256 of THOSE rows
    part = guarded((m, 1536 // 64, 2), dtype, "cpu", name="ln_part", pitch=2 * (1536 // 64))
    assert part.guard == 256 * 48 and part.off >= 256 * 48 and part.raw.numel() - part.off - part.n >= 256 * 48
    part.raw[part.off - 256 * 48] = 0                               # a store a whole 256-row tile in front of the output
    assert "guard" in _fails(part.check)
    assert bool(torch.isnan(out.raw.float()).all())
    out.t[:256] = want[:256].to(dtype)                              # a "kernel" that forgets the 44-row tail tile
    out.check()
    msg = _fails(out.assert_written)
    assert msg and "(256, 0)" in msg
    assert _fails(assert_close_sliced, "y", out.t, want, 1e-2, (0,)) is not None
    out.t[256:] = want[256:].to(dtype)
    out.check().assert_written()
    # one sentinel byte changed in a guard, on either side
    for pos in (out.off - 1, out.off + out.n, 0, out.raw.numel() - 1):
        saved = out.raw[pos].clone()
        out.raw.view(torch.uint8)[pos * out.raw.element_size()] ^= 1
        msg = _fails(out.check)
        assert msg and "guard" in msg, pos
        out.raw[pos] = saved
        out.check()


@pytest.mark.parametrize("dtype", [torch.uint8, torch.int16])
def test_byte_outputs_carry_0xa5(dtype):
    out = guarded((37, 256), dtype, "cpu")
    assert bool((out.raw.view(torch.uint8) == 0xA5).all())
    out.t.zero_()
    out.check()
    out.raw.view(torch.uint8)[(out.off + out.n) * out.raw.element_size() + 5] = 0xA4
    assert "guard" in _fails(out.check)


def test_residual_inputs_keep_their_data():
    c0 = _rand((130, 256), 8)
    out = guarded(c0.shape, torch.float32, "cpu", init=c0)
    assert torch.equal(out.t, c0)
    out.check().assert_written()


@pytest.mark.parametrize("fmt", FORMATS, ids=repr)
@pytest.mark.parametrize("dh,sk,prescaled", [(64, 63, False), (64, 63, True), (64, 573, True), (128, 63, True), (128, 573, True), ("fused", 63, True)])
def test_mask_edge_inputs(fmt, dh, sk, prescaled):
    """The inputs of the mask-edge GPU tests: the matched-rounding oracle, rounded to the output format, stays inside their gates against
    the exact oracle (whole and per query) -- the gates ask nothing of a correct kernel that its own arithmetic does not give --, and an
    attended front pad key fails both by two orders of magnitude."""
    case = mask_edge.fused_cross_attention_case(fmt, sk) if dh == "fused" else mask_edge.self_attention_case(fmt, dh, sk, prescaled)
    b, h, sq, d = case["b"], case["h"], case["sq"], case["dh"]
    gate = mask_edge.NEG_GATE[fmt.name]
    want, exact = case["want"], case["exact"]
    assert case["scores_max"] < -88
    view = lambda x: x.view(b, sq, h, d)
    good = fmt.round(want)
    assert_close("matched vs exact", good, exact, gate)
    assert_close_sliced("matched vs exact", view(good), view(exact), gate, (0, 1, 2), fmt.round)
    assert_close_sliced("rounded vs matched", view(good), view(want), gate, (0, 1, 2), fmt.round)
    bad = mask_edge.with_front_pads_attended(case, fmt)
    assert torch.equal(bad[0], good[0]), "sequence 0 has no front pad"
    errs = slice_errors(view(bad), view(want), (0, 1, 2))
    assert errs[1:].min().item() > 0.5, "an attended pad key takes every row of the sequences 1, 2, 3"
    assert _fails(assert_close, "pads", bad, want, gate) is not None
    msg = _fails(assert_close_sliced, "pads", view(bad), view(want), gate, (0, 1, 2), fmt.round)
    assert msg and "slice (" in msg


def test_pad_key_at_ordinary_scores_passes_the_whole_tensor_gate():
    """The gap: test_gpu_dit_head_dim.py::test_attention_hd128 at (3, 2, 1, 200, 61), the shape meant to cover the first-tile mask, in bf16.
    With the front pads attended the whole-tensor error stays inside the 5e-3 gate; the per-query gate does not let it through."""
    from oracle import dit as odit
    fmt, (b, h, kvh, sq, sk) = BF16, (3, 2, 1, 200, 61)
    qs = mask_edge.LOG2E / math.sqrt(128.0)
    q = (_rand((b, h, sq, 128), 12) * 1.5).to(fmt.dtype)
    k = (_rand((b, kvh, sk, 128), 13) * 1.5).to(fmt.dtype)
    v = _rand((b, kvh, sk, 128), 14).to(fmt.dtype)
    k[0, 0, sk - 1] = q[0, 0, 5] * 3
    q_eff = (q.float() * qs).to(fmt.dtype).float() / qs
    case = {"b": b, "sk": sk, "k": k, "v": v, "q_eff": q_eff}
    want = odit._merge(odit.attention_core(q_eff, k.float(), v.float(), rnd=fmt.round))
    bad = mask_edge.with_front_pads_attended(case, fmt)
    assert_close("attention_hd128 with attended pads", bad, want, fmt.tol(5e-3))
    msg = _fails(assert_close_sliced, "attention_hd128 with attended pads", bad.view(b, sq, h, 128), want.view(b, sq, h, 128), fmt.tol(5e-3), (0, 1, 2),
                 fmt.round)
    assert msg and "slice (" in msg


# ------------------------------------------------------------------------------------ bit equality and the workspace fill patterns
def test_workspace_fill_patterns_decode_to_what_they_claim():
    """WORKSPACE_FILLS, read as the formats the plans keep in a workspace."""
    from util import NAN_BYTE, WORKSPACE_FILLS, fill_pattern
    assert sorted(WORKSPACE_FILLS) == [0x00, 0x3C, 0x7B, 0xFF] and NAN_BYTE == 0xFF
    assert all(isinstance(reason, str) and reason and "\n" not in reason for reason in WORKSPACE_FILLS.values())
    value = lambda byte, dtype: fill_pattern(byte, dtype, 3).double()
    for dtype in (torch.float16, torch.bfloat16, torch.float32):
        assert fill_pattern(0x00, dtype, 3).shape == (3,)
        assert torch.equal(value(0x00, dtype), torch.zeros(3, dtype=torch.float64)) and not torch.signbit(fill_pattern(0x00, dtype)).any()
        assert torch.isnan(value(0xFF, dtype)).all()
        assert torch.isfinite(value(0x7B, dtype)).all() and torch.isfinite(value(0x3C, dtype)).all()
    # 0x7B7B: 2^15 (1 + 891 / 1024) as fp16, 2^119 (1 + 123 / 128) as bf16, 2^119 (1 + 0x7B7B7B / 2^23) as fp32
    assert value(0x7B, torch.float16)[0].item() == 61280.0
    assert value(0x7B, torch.bfloat16)[0].item() == 2.0 ** 119 * (1 + 123 / 128)
    assert value(0x7B, torch.float32)[0].item() == 2.0 ** 119 * (1 + 0x7B7B7B / 2 ** 23)
    assert 1.3e36 < value(0x7B, torch.bfloat16)[0].item() < 1.31e36 and 1.3e36 < value(0x7B, torch.float32)[0].item() < 1.31e36
    # one multiply by itself overflows each of them
    for dtype in (torch.float16, torch.bfloat16, torch.float32):
        assert torch.isinf(fill_pattern(0x7B, dtype) * fill_pattern(0x7B, dtype)).all()
    # 0x3C3C: 1 + 60 / 1024 as fp16, 2^-7 (1 + 60 / 128) as bf16, 2^-7 (1 + 0x3C3C3C / 2^23) as fp32
    assert value(0x3C, torch.float16)[0].item() == 1 + 60 / 1024
    assert value(0x3C, torch.bfloat16)[0].item() == 2.0 ** -7 * (1 + 60 / 128)
    assert value(0x3C, torch.float32)[0].item() == 2.0 ** -7 * (1 + 0x3C3C3C / 2 ** 23)
    if hasattr(torch, "float8_e4m3fn"):
        assert torch.isnan(value(0xFF, torch.float8_e4m3fn)).all() and value(0x7B, torch.float8_e4m3fn)[0].item() == 352.0


def test_assert_bit_equal_accepts_a_clone_and_names_one_flipped_bit():
    from util import assert_bit_equal
    for dtype in (torch.float32, torch.float16, torch.bfloat16):
        x = _rand((1000, 1000), 70).to(dtype)
        x[3, 5], x[999, 999], x[0, 0] = float("nan"), float("inf"), -0.0
        assert_bit_equal("clone", x.clone(), x)          # NaNs with the same bits are equal
        bits = {4: torch.int32, 2: torch.int16}[x.element_size()]
        y = x.clone()
        y.view(bits)[617, 283] ^= 1          # the lowest mantissa bit of one element in 10^6
        assert x[617, 283].item() != y[617, 283].item()
        msg = _fails(assert_bit_equal, "one ulp", y, x)
        assert msg and "1 of 1000000 elements differ" in msg and "the first at (617, 283)" in msg, msg
        assert repr(y[617, 283].item()) in msg and repr(x[617, 283].item()) in msg and "largest absolute difference" in msg
        ulp = abs(y[617, 283].double().item() - x[617, 283].double().item())
        assert f"{ulp:.3e}" in msg
    # a NaN whose payload differs is a difference; so is a NaN against a number
    a = torch.tensor([1.0, float("nan")])
    b = a.clone()
    b.view(torch.int32)[1] ^= 1
    assert torch.isnan(b[1]) and _fails(assert_bit_equal, "payload", b, a)
    assert "largest absolute difference inf" in _fails(assert_bit_equal, "nan", torch.tensor([1.0, 2.0]), a)
    # integer images (e4m3 bytes) compare as they are
    assert_bit_equal("bytes", torch.arange(256, dtype=torch.uint8), torch.arange(256, dtype=torch.uint8))
    assert _fails(assert_bit_equal, "bytes", torch.zeros(4, dtype=torch.uint8), torch.tensor([0, 0, 1, 0], dtype=torch.uint8))


def test_assert_bit_equal_tells_the_two_zeros_apart():
    from util import assert_bit_equal
    assert torch.equal(torch.tensor([0.0]), torch.tensor([-0.0]))          # what torch.equal would let through
    msg = _fails(assert_bit_equal, "zeros", torch.tensor([1.0, -0.0]), torch.tensor([1.0, 0.0]))
    assert msg and "1 of 2 elements differ" in msg and "the first at (1,)" in msg and "-0.0" in msg
    with pytest.raises(AssertionError):
        assert_bit_equal("dtype", torch.zeros(2), torch.zeros(2, dtype=torch.float16))
