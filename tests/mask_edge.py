"""Inputs that make an attended pad key loud (shared by test_gpu_kernels.py, test_gpu_dit_head_dim.py and test_parity_gates_host.py).

Key-side tensors of sequence b start at row (b * Sk) & 3 of their padded buffer, so the first key tile of every sequence with a non-zero
shift begins with 1..3 pad rows (K = 0, V^T = 0: score 0, value 0) that the kernels have to mask.  With ordinary scores one such key
among dozens moves a row by a fraction of the gate.  Here EVERY real logit lies far below 0 (about -150), so an attended pad key (score 0)
takes the whole softmax row and the output collapses to V = 0: an error of order 1 in every row of that sequence.

b = 4 gives the shifts 0, 1, 2, 3 (Sk odd).  Sk = 63: key ends 63, 66, 65, 64 -- sequences of one and of two key tiles in one launch, one
ending exactly on a tile.  Sk = 573: key ends 573, 574, 575, 576 -- nine tiles each, the last sequence filling its ninth to the end; more than 512 keys (the
two-key-group layout at small grids)."""
import math

import torch
import torch.nn.functional as F

LOG2E = 1.4426950408889634
B, H, KVH, SQ = 4, 2, 1, 96
NEG_GATE = {"bf16": 2e-2, "f16": 5e-3}          # the gates of the all-strongly-negative tests, against the matched oracle

_CACHE = {}


def _rand(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def _urand(shape, seed):
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed))


def _keys(fmt, b, kvh, sk, dh, base):
    # every key along +base, its length spread over 3 % (logits spread over ~4.5: a softmax over many keys, not a one-hot row)
    k = base * 12.0 * (1.0 - 0.03 * _urand((b, kvh, sk, 1), 501)) + 0.03 * _rand((b, kvh, sk, dh), 502)
    v = _rand((b, kvh, sk, dh), 503)
    return k.to(fmt.dtype), v.to(fmt.dtype)


def _finish(case, q_eff, k, v, fmt):
    from oracle import dit as odit
    dh = q_eff.shape[-1]
    scores = torch.einsum("bhid,bhjd->bhij", q_eff, k.float().repeat_interleave(q_eff.shape[1] // k.shape[1], dim=1)) / math.sqrt(dh)
    assert scores.max().item() < -88, "every real logit must lie below -87 (2^-126 in the log2 domain): a pad key at score 0 then takes the row"
    case["q_eff"], case["scores_max"] = q_eff, scores.max().item()
    case["want"] = odit._merge(odit.attention_core(q_eff, k.float(), v.float(), rnd=fmt.round))
    case["exact"] = odit._merge(odit.attention_core(q_eff, k.float(), v.float()))
    return case


def self_attention_case(fmt, dh, sk, prescaled=True):
    """q (as stored: pre-scaled by log2(e) / sqrt(dh) if ``prescaled``), k, v in fmt.dtype, and the oracle's answers [b, sq, h * dh]:
    want (matched rounding) and exact."""
    key = ("self", fmt.name, dh, sk, prescaled)
    if key not in _CACHE:
        base = F.normalize(_rand((dh,), 500), dim=0)
        amp = 100.0 if dh == 64 else 150.0                                       # q . k / sqrt(dh) ~ -150 / -159
        q = (-base * amp * (1.0 + 0.05 * _urand((B, H, SQ, 1), 504)) + 0.03 * _rand((B, H, SQ, dh), 505)).to(fmt.dtype)
        k, v = _keys(fmt, B, KVH, sk, dh, base)
        q_eff = q.float()
        if prescaled:
            c = LOG2E / math.sqrt(dh)
            q = (q.float() * c).to(fmt.dtype)               # what the producer stores ...
            q_eff = q.float() / c                           # ... and the query it stands for
        _CACHE[key] = _finish({"q": q, "k": k, "v": v, "b": B, "h": H, "kvh": KVH, "sq": SQ, "sk": sk, "dh": dh}, q_eff, k, v, fmt)
    return _CACHE[key]


FUSED_D = 256          # the fused entry needs K = d >= 192 and d % 128 == 0: four heads of 64 is its smallest shape (not the two of the self-attention cases)


def fused_cross_attention_case(fmt, sk=63):
    """a [b * s, d], w_q [d, d] built so that the projected queries are anti-aligned with every key: a lies along one unit vector u, every
    head's rows of w_q are -100 base u^T plus noise."""
    key = ("fused", fmt.name, sk)
    if key not in _CACHE:
        d, h = FUSED_D, FUSED_D // 64
        base = F.normalize(_rand((64,), 500), dim=0)
        u = F.normalize(_rand((d,), 506), dim=0)
        a = (u * (1.0 + 0.05 * _urand((B * SQ, 1), 507)) + 0.02 / d ** 0.5 * _rand((B * SQ, d), 508)).to(fmt.dtype)
        wq = ((-100.0 * base).repeat(h)[:, None] * u[None, :] + 0.03 * _rand((d, d), 509)).to(fmt.dtype)
        k, v = _keys(fmt, B, KVH, sk, 64, base)
        c = 0.125 * LOG2E
        q = (a.float() @ wq.float().T).view(B, SQ, h, 64).permute(0, 2, 1, 3)
        q_eff = (q * c).to(fmt.dtype).float() / c                               # the epilogue stores q pre-scaled, rounded once
        _CACHE[key] = _finish({"a": a, "wq": wq, "k": k, "v": v, "b": B, "h": h, "kvh": KVH, "sq": SQ, "sk": sk, "dh": 64, "d": d}, q_eff, k, v, fmt)
    return _CACHE[key]


def with_front_pads_attended(case, fmt):
    """What a kernel without the first-tile mask computes: the (b * Sk) & 3 pad rows in front of sequence b's keys (K = 0, V = 0) join the
    softmax with score 0.  [b, sq, h * dh], matched rounding, rounded once to the output format."""
    from oracle import dit as odit
    out = []
    for i in range(case["b"]):
        ob = (i * case["sk"]) & 3
        k, v = case["k"][i:i + 1].float(), case["v"][i:i + 1].float()
        zeros = torch.zeros((1, k.shape[1], ob, k.shape[3]))
        out.append(odit._merge(odit.attention_core(case["q_eff"][i:i + 1], torch.cat([zeros, k], 2), torch.cat([zeros, v], 2), rnd=fmt.round)))
    return fmt.round(torch.cat(out, 0))
