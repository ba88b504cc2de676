"""References that the GPU tests of the 32- / 96-channel-head kernels (tests/test_gpu_dit_head_width.py) compare against, in float64 torch, with
the mistakes a kernel could make as keyword arguments: tests/test_dit_head_width_host.py shows on the CPU that the gates of the GPU tests
catch each of them."""
import math

import torch

LOG2E = 1.4426950408889634
KEY_TILE = {32: 128, 96: 64}          # csrc/attn_hdw_tiles.h: sk_pad is a multiple of it


def qscale(w):
    return LOG2E / math.sqrt(w)          # what the head split multiplies into Q


def rope_pairs(w):
    return max(w // 2, 32) // 2          # RotaryEmbedding(max(W // 2, 32)): 16 pairs (j, j + 16) for 32, 24 pairs (j, j + 24) for 96


def _vt_perm(n):
    p = torch.arange(n)
    return (p & ~12) | ((p & 4) << 1) | ((p & 8) >> 1)


def _pad_heads(x, s_pad, key_side=False):
    # [B,H,S,W] -> zero-padded [B,H,s_pad,W]; key-side tensors (K, V) of sequence b start at row (b*S) & 3
    b, h, s, d = x.shape
    out = torch.zeros((b, h, s_pad, d), dtype=x.dtype)
    for i in range(b):
        ob = (i * s) & 3 if key_side else 0
        out[i, :, ob:ob + s] = x[i]
    return out


def inv_freq_of(w, rotary_dim=None):
    """RotaryEmbedding(max(W // 2, 32)).inv_freq: 16 entries for 32, 24 for 96.  rotary_dim: the frequencies of another rotation width."""
    r = 2 * rope_pairs(w) if rotary_dim is None else rotary_dim
    return (1.0 / (10000 ** (torch.arange(0, r, 2).double() / r)))[:rope_pairs(w)]


def head_split_reference(x, b, s, h, w, inv_freq, qk_norm, pair_offset=None, rotate_all=False, scale=None):
    """float64: q, k = rope(normalize(x)) per head of W, q times log2(e) / sqrt(W); v untouched.  [b, h, s, W] each.  Mistakes: pair_offset
    (the partner of channel j is j + pair_offset instead of j + rope_pairs(W); W = 96 only, a head of 32 has no channel j + 32),
    rotate_all (W = 96: channels 48..95 are rotated like 0..47), scale (instead of log2(e) / sqrt(W))."""
    n = rope_pairs(w)
    rh = n if pair_offset is None else pair_offset
    qkv = x.double().view(b, s, 3, h, w).permute(2, 0, 3, 1, 4)
    ang = torch.arange(s, dtype=torch.float64)[:, None] * inv_freq.double()[None, :]
    cs, sn = ang.cos(), ang.sin()

    def rot(t, lo):
        x1, x2 = t[..., lo:lo + n], t[..., lo + rh:lo + rh + n]
        t = t.clone()
        t[..., lo:lo + n] = x1 * cs - x2 * sn
        t[..., lo + rh:lo + rh + n] = x2 * cs + x1 * sn
        return t

    def norm_rope(t):
        if qk_norm:
            t = t / t.norm(dim=-1, keepdim=True).clamp_min(1e-12)          # F.normalize
        t = rot(t, 0)
        if rotate_all and w == 96:
            t = rot(t, 48)
        return t

    return norm_rope(qkv[0]) * (qscale(w) if scale is None else scale), norm_rope(qkv[1]), qkv[2]


def attention_reference(q, k, v, w, kv_index=None, scale=None, attended_front_pads=0):
    """float64 softmax(q k^T * scale) v with GQA: q [b, h, sq, W], k / v [b, kvh, sk, W] -> [b, sq, h * W].  kv_index(h_index, h, kvh): the
    kv head of a query head, default h_index // (h // kvh); scale: default W ** -0.5; attended_front_pads: that many all-zero keys (score 0,
    V = 0) join the softmax, what a kernel without the first-tile mask computes."""
    b, h, sq, _ = q.shape
    kvh = k.shape[1]
    idx = [(kv_index or (lambda i, h_, kvh_: i // (h_ // kvh_)))(i, h, kvh) for i in range(h)]
    kk, vv = k.double()[:, idx], v.double()[:, idx]
    if attended_front_pads:
        z = torch.zeros((b, h, attended_front_pads, w), dtype=torch.float64)
        kk, vv = torch.cat((z, kk), dim=2), torch.cat((z, vv), dim=2)
    s = torch.einsum("bhid,bhjd->bhij", q.double(), kk) * (w ** -0.5 if scale is None else scale)
    return (torch.softmax(s, dim=-1) @ vv).permute(0, 2, 1, 3).reshape(b, sq, h * w)
