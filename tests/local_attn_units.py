"""A float64 restatement of the local-attention codec (reference models/local_attention.py) for single-stage models, on plain torch and
tests/golden/natten_standin.py: the yardstick tests/test_local_attn_host.py holds against the reference's golden of case C, and the carrier
of the deliberately wrong variants the per-row gate has to reject.

``wrong``: None, or one of
  "truncated_window"   a query sees the keys within window // 2 of itself and no others: the window is cut at the ends instead of shifted
  "scaled_logits"      the logits are multiplied by dim_head ** -0.5 (the reference does not scale them in its NATTEN branch)
  "contiguous_down"    project_down.weight is applied, un-permuted, to r consecutive rows laid side by side (feature index j * C + c where
                       the rearrange "b (n r) c -> b n (c r)" gives c * r + j)
"""
import os
import sys

import torch
from torch.nn import functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
import natten_standin  # noqa: E402

WRONG = ("truncated_window", "scaled_logits", "contiguous_down")


def _rotate(t, inv_freq):
    """apply_rotary_pos_emb (transformer.py:164-183) on [b, h, n, d]: the first 2 * len(inv_freq) channels in pairs (j, j + len(inv_freq))"""
    n, half = t.shape[-2], inv_freq.shape[0]
    freqs = torch.arange(n, dtype=torch.float64)[:, None] * inv_freq[None, :]
    freqs = torch.cat((freqs, freqs), dim=-1)
    rot, rest = t[..., :2 * half], t[..., 2 * half:]
    x1, x2 = rot[..., :half], rot[..., half:]
    rot = rot * freqs.cos() + torch.cat((-x2, x1), dim=-1) * freqs.sin()
    return torch.cat((rot, rest), dim=-1)


def layer(x, sd, prefix, heads, window, inv_freq, wrong=None):
    """One ContinuousLocalTransformer layer on x [b, n, d] (local_attention.py:81-101, no conditioning)"""
    b, n, d = x.shape
    dh = d // heads
    h = F.layer_norm(x, (d,), sd[prefix + "0.gamma"], sd[prefix + "0.beta"])
    q, k, v = ((h @ sd[prefix + "1.to_qkv.weight"].T).chunk(3, dim=-1))
    q, k, v = (t.reshape(b, n, heads, dh).transpose(1, 2) for t in (q, k, v))
    q, k = _rotate(q, inv_freq), _rotate(k, inv_freq)
    if wrong == "truncated_window":
        i = torch.arange(n)
        seen = (i[:, None] - i[None, :]).abs() <= window // 2
        attn = torch.einsum("bhid,bhjd->bhij", q, k).masked_fill(~seen, float("-inf")).softmax(dim=-1)
        out = torch.einsum("bhij,bhjd->bhid", attn, v)
    else:
        attn = natten_standin.natten1dqk(q, k, window)
        if wrong == "scaled_logits":
            attn = attn * dh ** -0.5
        out = natten_standin.natten1dav(attn.softmax(dim=-1), v, window)
    x = x + out.transpose(1, 2).reshape(b, n, d) @ sd[prefix + "1.to_out.weight"].T
    h = F.layer_norm(x, (d,), sd[prefix + "3.gamma"], sd[prefix + "3.beta"])
    a, gate = (h @ sd[prefix + "4.ff.0.proj.weight"].T + sd[prefix + "4.ff.0.proj.bias"]).chunk(2, dim=-1)
    return x + (a * F.silu(gate)) @ sd[prefix + "4.ff.2.weight"].T


def encoder(x, sd, heads, depth, ratio, window, wrong=None):
    """A one-stage TransformerEncoder1D (local_attention.py:229-236, 133-146) on x [b, c, n]; sd: float64 state dict"""
    x = x.transpose(1, 2) @ sd["project_in.weight"].T
    for l in range(depth):
        x = layer(x, sd, f"layers.0.transformer.layers.{l}.", heads, window, sd["layers.0.transformer.rotary_pos_emb.inv_freq"], wrong)
    b, n, c = x.shape
    if wrong == "contiguous_down":
        x = x.reshape(b, n // ratio, ratio * c)
    else:
        x = x.reshape(b, n // ratio, ratio, c).transpose(2, 3).reshape(b, n // ratio, c * ratio)          # "b (n r) c -> b n (c r)"
    x = x @ sd["layers.0.project_down.weight"].T
    return (x @ sd["project_out.weight"].T).transpose(1, 2)


def decoder(z, sd, heads, depth, ratio, window, wrong=None):
    """A one-stage TransformerDecoder1D (local_attention.py:276-282, 176-190) on z [b, c, n]"""
    x = z.transpose(1, 2) @ sd["project_in.weight"].T
    x = x @ sd["layers.0.project_up.weight"].T
    b, n, cr = x.shape
    x = x.reshape(b, n, cr // ratio, ratio).transpose(2, 3).reshape(b, n * ratio, cr // ratio)                # "b n (c r) -> b (n r) c"
    for l in range(depth):
        x = layer(x, sd, f"layers.0.transformer.layers.{l}.", heads, window, sd["layers.0.transformer.rotary_pos_emb.inv_freq"], wrong)
    return (x @ sd["project_out.weight"].T).transpose(1, 2)
