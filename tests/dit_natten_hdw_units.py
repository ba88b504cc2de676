"""References and host-side helpers of the neighbourhood self-attention tests at 128-, 32- and 96-channel heads
(tests/test_dit_natten_hdw_host.py, tests/test_gpu_dit_natten_hdw.py; csrc/attention_hdw_window.hip).

The float64 reference is ``dit_natten_units.window_attention`` as it is -- it takes any head width.  What is added here: the unit tensors in
the kernel's conventions (Q as the head split stores it for a neighbourhood plan's kernel, in the log2 domain; there is no scale argument),
the mistakes of ``dit_natten_units.MISTAKES`` that depend on the key tile at the tile of the width (128 keys at W = 32), one more mistake
that only a tile of four 32-key blocks can make, and ``check_ranges`` for tests/host/attn_window_kt_dump.cpp."""
import os
import shutil
import subprocess

import torch

import dit_causal_units as CU
import dit_natten_units as NU

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = NU.CSRC
WIDTHS = (32, 96, 128)
KEY_TILE = CU.KEY_TILE                          # {32: 128, 96: 64, 128: 64}
SEQ_LENS = (33, 65, 129, 257, 301, 645)         # one wave and a tail wave; one key past a 64-key tile; past a 128-key tile; past two; two workgroups; three
QUERY_BLOCK = NU.QUERY_BLOCK
LOG2E = 1.4426950408889634
MISTAKES = NU.MISTAKES + ("drop_third_block",)          # the last one at W = 32 only


def visible(b, s, ks, w, mistake=None):
    """dit_natten_units.visible with the key tile of head width w.  One more mistake:
      drop_third_block   W = 32: block 2 (keys 64..95) of every 128-key tile is passed over -- a walk that ends a tile at its first
                         skipped block loses it for the waves whose union begins there
    (a row that would lose every key keeps its window)"""
    kt = KEY_TILE[w]
    if mistake not in ("drop_first_tile", "drop_last_tile", "drop_third_block"):
        return NU.visible(b, s, ks, mistake)
    i = torch.arange(s)[:, None]
    j = torch.arange(s)[None, :]
    m = NU.visible(b, s, ks)
    ob = NU.key_shift(b, s)
    if mistake == "drop_third_block":
        assert kt == 128, "a 64-key tile has no third block"
        wrong = m & (((ob + j) % kt) // 32 != 2)
    else:
        q0 = (i // QUERY_BLOCK) * QUERY_BLOCK
        q1 = (q0 + QUERY_BLOCK - 1).clamp(max=s - 1)
        st = NU.start(s, ks)
        t_first = (ob + st[q0]) // kt
        t_last = (ob + st[q1] + ks - 1) // kt
        wrong = m & ((ob + j) // kt != (t_first if mistake == "drop_first_tile" else t_last))
    return torch.where(wrong.any(dim=1, keepdim=True), wrong, m)


def window_attention(q, k, v, ks, scale, rnd=None, mistake=None):
    """dit_natten_units.window_attention; the tile mistakes at the key tile of the tensors' head width."""
    if mistake not in ("drop_first_tile", "drop_last_tile", "drop_third_block"):
        return NU.window_attention(q, k, v, ks, scale, rnd=rnd, mistake=mistake)
    b, h, s, w = q.shape
    kvh = k.shape[1]
    qd, kd, vd = q.double(), k.double().repeat_interleave(h // kvh, dim=1), v.double().repeat_interleave(h // kvh, dim=1)
    dots = torch.einsum("bhid,bhjd->bhij", qd, kd) * scale
    out = torch.empty((b, h, s, w), dtype=torch.float64)
    for bi in range(b):
        d = dots[bi].masked_fill(~visible(bi, s, ks, w, mistake)[None], float("-inf"))
        p = torch.exp(d - d.amax(dim=-1, keepdim=True))
        pr = p if rnd is None else rnd(p.float()).double()
        out[bi] = torch.einsum("hij,hjd->hid", pr, vd[bi]) / p.sum(dim=-1, keepdim=True)
    return out.permute(0, 2, 1, 3).reshape(b, s, h * w)


def unit_tensors(fmt, w, b, h, kvh, s, seed=0):
    """(q as the kernel reads it, the query q_eff it stands for, k, v, the score scale of the reference): the unit tensors of the full-attention
    tests at width w.  q is q_eff * log2(e) / sqrt(w) rounded to fmt -- what the head split of a neighbourhood plan stores is its unscaled
    query times log2(e), and that query is q_eff / sqrt(w) here, so the logit spread is the scaled family's (the argument of
    dit_natten_hdw_cases.qk_gain).  The reference runs on (q_eff, k, v) with the scale w ** -0.5."""
    q, q_eff, k, v = CU.unit_tensors(fmt, w, b, h, kvh, s, seed=seed, prescaled=True)
    return q, q_eff, k, v, w ** -0.5


def check_ranges(tmp_path, s_max=700):
    """tests/host/attn_window_kt_dump.cpp against csrc/attn_window.h and the key tiles of csrc/attn_hdw_tiles.h: exit status 0 and its line."""
    cxx = shutil.which("g++") or "/opt/rocm/lib/llvm/bin/clang++"
    exe = os.path.join(tmp_path, "attn_window_kt_dump")
    subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-Werror", "-I", CSRC, os.path.join(HERE, "host", "attn_window_kt_dump.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe, str(s_max)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout.strip()
