"""The one-prompt to_qkv tile (30: 256 x 192 on twelve waves of 64 x 64) and the MFMA shape its heads build runs (csrc/gemm_bf16.hip, S16),
forced through the unit C ABI in both operand formats.  On v_mfma_f32_16x16x32 a wave's head is sixteen 16 x 16 blocks: q / k waves issue
the MFMA with swapped operands (lane = token row, lane quarter = four channels of each block) and exchange 8-byte runs between lane
quarters for 16-byte stores, V^T waves keep the un-swapped orientation (lane = channel, registers = four consecutive tokens).  These tests
hold either shape to the same results.

d = 256 gives N = 768 = four column tiles q | q + k | k + v | v: one tile mixes the two orientations, one mixes q and k; K = 256 is four
K-tiles of the ring.  Rows (two sequences): s = 129 -> M = 258, a 2-row tail tile whose wave rows 1-3 have no valid rows, the sequence
boundary at row 129 inside a 16-row block, key offset 1 for sequence 1; s = 197 -> M = 394; s = 5 -> M = 10, every row block holds both
sequences."""
import pytest
import torch

from test_gpu_kernels import _check_qkv_outputs, _ln_fold_producer, _ln_fold_reference, _qkv_outputs, _vt_perm
from util import FORMATS, assert_close, assert_close_sliced, guarded

pytestmark = pytest.mark.gpu

TILE = 30
B, D = 2, 256
ROWS = [(129, 256), (197, 256), (5, 128)]          # (s, s_pad)


def _lib():
    from stable_audio_tools import _hip
    return _hip, _hip.lib()


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g) * scale


def _qkv_rope(dev, fmt, a, w, inv_freq, s, s_pad):
    """to_qkv + RoPE + head split of a [B s, d] x w [3 d, d] on the forced tile -> (q, k, V^T with its key permutation undone, the rotation
    table the device wrote as (cos, sin) [s, 16]), on the host; guards and pads checked."""
    _hip, lib = _lib()
    d = a.shape[1]
    h = d // 64
    ad, wd, fd = a.to(dev), w.to(dev), inv_freq.to(dev)
    guards, (qd, kd, vtd, scratch) = _qkv_outputs(dev, fmt, B, h, s, s_pad, 64)
    _hip.check(fmt.fn(lib, "sat_qkv_rope_bf16")(_hip.ptr(ad), _hip.ptr(wd), _hip.ptr(fd), _hip.ptr(qd), _hip.ptr(kd), _hip.ptr(vtd),
                                                _hip.ptr(scratch), B, s, s_pad, d, TILE, _hip.stream()))
    _check_qkv_outputs(guards)
    q, k, vt = qd.cpu(), kd.cpu(), vtd.cpu()[..., _vt_perm(s_pad)]
    _check_pads(q, k, vt, s)
    table = scratch.cpu().double()
    return q, k, vt, (table[:s * 16].view(s, 16), table[s * 16:].view(s, 16))


def _check_pads(q, k, vt, s):
    assert (q[:, :, s:] == 0).all(), "Q pads must be zero"
    for i in range(B):          # key-side tensors of sequence i start at row / column (i s) & 3
        ob = (i * s) & 3
        assert (k[i, :, :ob] == 0).all() and (k[i, :, ob + s:] == 0).all(), "K pads must be zero"
        assert (vt[i, :, :, :ob] == 0).all() and (vt[i, :, :, ob + s:] == 0).all(), "V^T pads must be zero"


def _split(qkv, s):
    """[B s, 3 d] -> q, k, v as [B, h, s, 64]"""
    d = qkv.shape[1] // 3
    return tuple(t.reshape(B, s, d // 64, 64).transpose(1, 2) for t in qkv.view(B, s, 3 * d).chunk(3, dim=-1))


def _one_hot(rows, k):
    x = torch.zeros(rows, k)
    idx = (7 * torch.arange(rows) + 3) % k          # 7 is a unit mod 256: consecutive rows select distinct k
    x[torch.arange(rows), idx] = 1.0
    return x, idx


@pytest.mark.parametrize("fmt", FORMATS, ids=repr)
@pytest.mark.parametrize("one_hot", ["a", "w"])
@pytest.mark.parametrize("s,s_pad", ROWS)
def test_selection_exact(dev, s, s_pad, one_hot, fmt):
    """inv_freq = 0 makes the table cos = 1, sin = 0: the rotation is the identity whatever the compiler contracts.  A one-hot operand
    then turns the whole launch into a selection of the other operand's 16-bit values, which every rounding keeps: q, k (at their key
    offsets) and V^T (key permutation undone) equal the selected values bit for bit, so a permuted row, column, head, k index or lane
    quarter shows."""
    m = B * s
    if one_hot == "a":
        a, idx = _one_hot(m, D)
        w = (_rand((3 * D, D), 11) * 0.1).to(fmt.dtype)
        a = a.to(fmt.dtype)
        want = w[:, idx].T.contiguous()          # qkv[m, n] = w[n, idx[m]]
    else:
        w, idx = _one_hot(3 * D, D)
        a = _rand((m, D), 12).to(fmt.dtype)
        w = w.to(fmt.dtype)
        want = a[:, idx].contiguous()            # qkv[m, n] = a[m, idx[n]]
    q, k, vt, (cos, sin) = _qkv_rope(dev, fmt, a, w, torch.zeros(16), s, s_pad)
    assert bool((cos == 1).all()) and bool((sin == 0).all()), "inv_freq = 0: the table must be the identity rotation"
    wq, wk, wv = _split(want, s)
    for name, got, ref in (("q", q[:, :, :s], wq),):
        bad = (got != ref).nonzero()
        assert torch.equal(got, ref), f"{name}, one-hot {one_hot}: {bad.shape[0]} elements differ, the first at {tuple(bad[0].tolist())}"
    for i in range(B):
        ob = (i * s) & 3
        for name, got, ref in (("k", k[i, :, ob:ob + s], wk[i]), ("v^T", vt[i, :, :, ob:ob + s], wv[i].transpose(1, 2))):
            bad = (got != ref).nonzero()
            assert torch.equal(got, ref), (f"{name} of sequence {i}, one-hot {one_hot}: {bad.shape[0]} elements differ, the first at "
                                           f"{tuple(bad[0].tolist())}")


def _half_ulp(x, fmt):
    """half a unit in the last place of the output format at |x| (fp16: the subnormal step 2^-24 as the floor of the unit)"""
    mant, emin = (10, -14) if fmt.f16 else (7, -126)
    e = torch.floor(torch.log2(x.abs().clamp_min(2.0 ** emin))).clamp_min(emin)
    return 0.5 * torch.pow(torch.tensor(2.0, dtype=torch.float64), e - mant)


# random operands of the rotation test, one set per format at the tallest M; the M cases take its first rows (rows are independent)
_OPS = {}


def _operands(fmt):
    if fmt.name not in _OPS:
        a = _rand((B * max(s for s, _ in ROWS), D), 15).to(fmt.dtype)
        w = (_rand((3 * D, D), 16) * 0.1).to(fmt.dtype)
        _OPS[fmt.name] = (a, w, a.double() @ w.double().T, a.double().abs() @ w.double().abs().T)
    return _OPS[fmt.name]


@pytest.mark.parametrize("fmt", FORMATS, ids=repr)
@pytest.mark.parametrize("s,s_pad", ROWS)
def test_rotation_partner_and_table_row(dev, s, s_pad, fmt):
    """Random operands, the real inv_freq, against float64 built from the table the device itself wrote (so the table's own rounding is
    not in the comparison).  Bound per element = bound on the fp32 result + the one output rounding:
      fp32 result: (K + 4) 2^-24 (sum|a w| of the channel x |cos| + sum|a w| of its partner x |sin|) -- products of 16-bit operands are
        exact in fp32, any summation order of K terms stays inside K - 1 units, rotation and scale round three more times;
      output: half an ulp of the format at the value being rounded (the reference's magnitude plus the fp32 bound), with the fp16
        subnormal step as a floor.
    A swapped rotation partner or the table row of another position is an error of the order of the value itself."""
    a, w, prod, mag = _operands(fmt)
    m = B * s
    a, prod, mag = a[:m], prod[:m], mag[:m]
    inv_freq = 1.0 / (10000 ** (torch.arange(0, 32, 2).float() / 32))
    q, k, vt, (cos, sin) = _qkv_rope(dev, fmt, a, w, inv_freq, s, s_pad)

    def rotate(x, xmag):          # [B, h, s, 64] float64: value and its bound's magnitude term
        c, sn = cos[None, None], sin[None, None]
        x1, x2 = x[..., :16], x[..., 16:32]
        val = torch.cat([x1 * c - x2 * sn, x2 * c + x1 * sn, x[..., 32:]], -1)
        m1, m2 = xmag[..., :16], xmag[..., 16:32]
        magn = torch.cat([m1 * c.abs() + m2 * sn.abs(), m2 * c.abs() + m1 * sn.abs(), xmag[..., 32:]], -1)
        return val, magn

    (pq, pk, pv), (mq, mk, mv) = _split(prod, s), _split(mag, s)
    wq, gq = rotate(pq, mq)
    wk, gk = rotate(pk, mk)
    cases = [("q", q[:, :, :s], wq, gq)]
    for i in range(B):
        ob = (i * s) & 3
        cases.append((f"k of sequence {i}", k[i, :, ob:ob + s], wk[i], gk[i]))
        cases.append((f"v^T of sequence {i}", vt[i, :, :, ob:ob + s], pv[i].transpose(1, 2), mv[i].transpose(1, 2)))
    for name, got, want, magn in cases:
        b32 = (D + 4) * 2.0 ** -24 * magn
        bound = b32 + _half_ulp(want.abs() + b32, fmt)
        excess = (got.double() - want).abs() / bound
        at = tuple(int(i) for i in torch.unravel_index(excess.argmax(), excess.shape))
        print(f"tile {TILE} {fmt} s={s} {name}: worst |error| / bound {float(excess.max()):.3f} at {at}")
        assert float(excess.max()) <= 1.0, f"{name}, s = {s}: element {at} is {float(excess.max()):.2f} x the bound off the float64 rotation"


@pytest.mark.parametrize("fmt", FORMATS, ids=repr)
@pytest.mark.parametrize("d", [256, 768])
def test_ln_fold_behind_both_layouts(dev, d, fmt):
    """LayerNorm folded into to_qkv: producer tile 49 -> consumer 30 at M = 258 (s = 129).  d = 256: the column tiles straddle q | k | v;
    d = 768: tile-aligned parts as in the model.  Row 140 (sequence 1, token 11) carries a common-mode offset of 8 on top of the producer's
    output: (mean, rstd) are per token row, which is a lane in the q / k layout and a register in the V^T layout.  Compared with the same
    arithmetic in float64 at the gate of test_ln_fold_qkv_rope, per (sequence, head, token) for q and per (head, token) / (head, key column)
    for k and V^T."""
    from oracle import dit as odit
    _hip, lib = _lib()
    s, s_pad = 129, 256
    h = d // 64
    cd, xb, part = _ln_fold_producer(dev, B * s, d, 256, 49, seed=60, fmt=fmt)
    row = 140
    xb[row] = (cd[row] + 8.0).clamp(-65504.0, 65504.0).to(fmt.dtype)
    blocks = xb[row].float().view(d // 64, 64)
    part[row] = torch.stack([blocks.sum(-1), (blocks * blocks).sum(-1)], -1)
    w = _rand((3 * d, d), 70) * 0.06
    gamma = 0.8 + 0.2 * _rand((d,), 71)
    beta = 0.1 * _rand((d,), 72)
    inv_freq = 1.0 / (10000 ** (torch.arange(0, 32, 2).float() / 32))
    freqs = odit.rotary_freqs(inv_freq, s)
    q, k, v = (odit._heads(t, h) for t in _ln_fold_reference(xb, w, gamma, beta, None, fmt).view(B, s, 3 * d).chunk(3, dim=-1))
    q, k = odit.apply_rotary(q, freqs), odit.apply_rotary(k, freqs)
    wd, gd, bd, fd = w.to(dev), gamma.to(dev), beta.to(dev), inv_freq.to(dev)
    wpg, cg = guarded((3 * d, d), fmt.dtype, dev, name="wp"), guarded((6 * d,), torch.float32, dev, name="c12")
    guards, (qd, kd, vtd, scratch) = _qkv_outputs(dev, fmt, B, h, s, s_pad, 64)
    _hip.check(fmt.fn(lib, "sat_qkv_rope_ln_bf16")(_hip.ptr(xb), _hip.ptr(part), _hip.ptr(wd), _hip.ptr(gd), _hip.ptr(bd), _hip.ptr(wpg.t),
                                                   _hip.ptr(cg.t), _hip.ptr(fd), _hip.ptr(qd), _hip.ptr(kd), _hip.ptr(vtd), _hip.ptr(scratch),
                                                   B, s, s_pad, d, TILE, _hip.stream()))
    for g_ in (wpg, cg):
        g_.check().assert_written()
    _check_qkv_outputs(guards)
    qh, kh, vth = qd.cpu(), kd.cpu(), vtd.cpu()[..., _vt_perm(s_pad)]
    _check_pads(qh, kh, vth, s)
    tol = fmt.tol(4e-3)
    assert_close("ln-fold q", qh[:, :, :s], q, tol)
    assert_close_sliced("ln-fold q per (sequence, head, token)", qh[:, :, :s], q, tol, (0, 1, 2), fmt.round)
    for i in range(B):
        ob = (i * s) & 3
        assert_close("ln-fold k", kh[i, :, ob:ob + s], k[i], tol)
        assert_close("ln-fold v^T", vth[i, :, :, ob:ob + s], v[i].transpose(1, 2), tol)
        assert_close_sliced("ln-fold k per (head, token)", kh[i, :, ob:ob + s], k[i], tol, (0, 1), fmt.round)
        assert_close_sliced("ln-fold v^T per (head, key column)", vth[i, :, :, ob:ob + s], v[i].transpose(1, 2), tol, (0, 2), fmt.round)
