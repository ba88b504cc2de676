"""What the tests of the staged-route kernels (csrc/attention_hdw.hip, csrc/head_split_hdw.hip: 32-, 96- and 128-channel heads) share.  The
references that tests/test_gpu_dit_head_width.py compares against, in float64 torch, with the mistakes a kernel could make as keyword
arguments: tests/test_dit_head_width_host.py shows on the CPU that the gates of the GPU tests catch each of them.  The layout helpers of
both GPU test files, and the host check of the attention kernel's LDS tile maps (csrc/attn_hdw_tiles.h) for any of the three widths."""
import math
import os
import shutil
import subprocess

import torch

LOG2E = 1.4426950408889634
KEY_TILE = {32: 128, 96: 64, 128: 64}          # csrc/attn_hdw_tiles.h: sk_pad is a multiple of it


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


# ------------------------------------------------------------------------------- csrc/attn_hdw_tiles.h on the host
_TILE_DUMP = r"""
#include <stdio.h>
#include "attn_hdw_tiles.h"
using namespace attnw;
template <int W> void dump() {
    using T = Tiles<W>;
    static_assert(T::STAGE_BYTES == (W == 32 ? 16 : 32) * 1024 && T::LDS_BYTES == T::STAGES * T::STAGE_BYTES, "ring");
    static_assert((W == 32 ? 2 : 1) * T::LDS_BYTES <= 160 * 1024, "workgroups per CU");
    static_assert(T::k_tile_off(0, 0) == 0 && T::vt_tile_off(0, 0) == 0, "constexpr in host code");
    printf("K %d %d %d %d %d %d\n", W, T::KV_TILE, T::K_CHUNKS, T::K_ROW_BYTES, T::K_TILE_BYTES, T::K_PIECES);
    for (int r = 0; r < T::KV_TILE; ++r) for (int c = 0; c < T::K_CHUNKS; ++c) printf("%d %d %d\n", r, c, T::k_tile_off(r, c));
    for (int p = 0; p < T::K_TILE_BYTES / 1024; ++p) for (int l = 0; l < 64; ++l) printf("D %d %d %d %d\n", p, l, T::k_dma_row(p, l), T::k_dma_chunk(p, l));
    printf("V %d %d %d %d %d %d\n", W, W, T::KV_TILE / 8, T::VT_ROW_BYTES, T::VT_TILE_BYTES, T::VT_PIECES);
    for (int r = 0; r < W; ++r) for (int c = 0; c < T::KV_TILE / 8; ++c) printf("%d %d %d\n", r, c, T::vt_tile_off(r, c));
    for (int p = 0; p < T::VT_TILE_BYTES / 1024; ++p) for (int l = 0; l < 64; ++l) printf("D %d %d %d %d\n", p, l, T::vt_dma_row(p, l), T::vt_dma_chunk(p, l));
}
int main() { WIDTHS }
"""
# lanes of the four 16-lane groups one ds_read_b128 is served in (gfx950)
_B128_GROUPS = [[0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27], [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31]]
_B128_GROUPS += [[l + 32 for l in g] for g in _B128_GROUPS]


def check_lds_tile_maps(csrc, tmp_path, widths):
    """attn_hdw_tiles.h compiled as plain host C++ (g++), for the K and the V^T tile of every width: every (row, 16-byte chunk) that holds data
    has its own 16-byte-aligned slot inside the tile, a row's chunks stay inside the row (the LDS-DMA writes whole rows), the LDS-DMA lane that
    lands on a slot fetches the chunk the map puts there (only the four hole slots of a padded 96-channel K row and the spare V^T rows of 96
    belong to no chunk), and the fragment reads of the kernel (lane l: row 32 kb + (l & 31), chunk 2 t + (l >> 5)) put the 16 lanes of every
    ds_read_b128 group on 16 different slots of the 256-byte bank row.  Returns the tiles, K then V^T per width: kind, w, rows, chunks,
    row_bytes, size, pieces (1-KiB LDS-DMA pieces per wave), holes (DMA lanes that land on no chunk)."""
    cxx = shutil.which("g++") or "/opt/rocm/lib/llvm/bin/clang++"
    src, exe = os.path.join(tmp_path, "tiles.cpp"), os.path.join(tmp_path, "tiles")
    with open(src, "w") as f:
        f.write(_TILE_DUMP.replace("WIDTHS", " ".join(f"dump<{w}>();" for w in widths)))
    subprocess.run([cxx, "-std=c++17", "-I", csrc, src, "-o", exe], check=True, capture_output=True)
    lines = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split("\n")[:-1]
    tiles, cur = [], None
    for ln in lines:
        f = ln.split()
        if f[0] in "KV":
            cur = dict(kind=f[0], w=int(f[1]), rows=int(f[2]), chunks=int(f[3]), row_bytes=int(f[4]), size=int(f[5]), pieces=int(f[6]), off={}, dma={})
            tiles.append(cur)
        elif f[0] == "D":
            cur["dma"][(int(f[1]), int(f[2]))] = (int(f[3]), int(f[4]))
        else:
            cur["off"][(int(f[0]), int(f[1]))] = int(f[2])
    assert [(t["kind"], t["w"]) for t in tiles] == [(kind, w) for w in widths for kind in "KV"]
    for t in tiles:
        off, rb = t["off"], t["row_bytes"]
        assert len(off) == t["rows"] * t["chunks"]
        assert all(o % 16 == 0 and 0 <= o <= t["size"] - 16 for o in off.values())
        assert len(set(off.values())) == len(off)
        assert all(o // rb == r for (r, _), o in off.items())          # the LDS-DMA writes whole rows
        # the DMA lane at byte 1024 p + 16 l carries the chunk whose slot that is, or a hole / spare row (nothing maps there)
        at = {o: rc for rc, o in off.items()}
        assert len(t["dma"]) == t["size"] // 16
        t["holes"] = 0
        for (p, l), (row, chunk) in t["dma"].items():
            o = 1024 * p + 16 * l
            assert row == o // rb and 0 <= chunk < rb // 16
            assert at.get(o) == ((row, chunk) if o in at else None), (t["kind"], t["w"], p, l)
            if o not in at:
                assert (t["kind"] == "K" and t["w"] == 96 and chunk >= 12) or (t["kind"] == "V" and t["w"] == 96 and row >= 96), (p, l, row, chunk)
                t["holes"] += 1
        for first_row in range(0, t["rows"], 32):
            for chunk_pair in range(t["chunks"] // 2):
                for group in _B128_GROUPS:
                    slots = {off[(first_row + (l & 31), 2 * chunk_pair + (l >> 5))] % 256 // 16 for l in group}
                    assert len(slots) == 16, (t["kind"], t["w"], first_row, chunk_pair, group)
    return tiles
