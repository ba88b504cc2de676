"""References and host-side helpers of the neighbourhood self-attention tests (tests/test_dit_natten_host.py, tests/test_gpu_dit_natten.py).

``window_attention`` is ``oracle.dit.attention_core`` restated in float64 with the mask of csrc/attn_window.h -- query i of a sequence of s
rows sees the K keys from start(i) = min(max(i - K // 2, 0), s - K) on -- a score scale of the caller's choice (the reference's NATTEN branch
has none) and the same matched rounding: P = exp(s - max) is rounded to the operand format before P V, the normaliser is the sum of the
un-rounded P.  ``MISTAKES`` are the masks (and the one scale) of kernels that are wrong on purpose; the host test shows that the gates of
the GPU test reject each of them.  ``check_ranges`` compiles attn_window.h with the host compiler (tests/host/attn_window_dump.cpp) and
compares it with brute force."""
import os
import shutil
import subprocess

import torch

import dit_causal_units as CU

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "friendly-stable-audio-tools_amd", "csrc")
SEQ_LENS = (33, 64, 65, 129, 301, 645)          # one wave and a bit; a full tile; one key past it; two tiles; two workgroups; three
KERNELS = (3, 7, 33, 65, 129)                   # and the whole sequence (kernel_sizes)
QUERY_BLOCK, KEY_TILE = 256, 64                 # attention_window.hip
key_shift = CU.key_shift


def kernel_sizes(s):
    """The kernel sizes of the unit tests at sequence length s: KERNELS up to s, and s itself (s - 1 when s is even)."""
    return tuple(sorted({k for k in KERNELS if k <= s} | {s if s % 2 else s - 1}))


def start(s, ks):
    """[s] long: the first key of every query's window"""
    return (torch.arange(s) - ks // 2).clamp(min=0, max=s - ks)


def visible(b, s, ks, mistake=None):
    """[s, s] bool, element (i, j): query i of sequence b sees key j.  mistake: a kernel that is wrong on purpose
      start_minus      the window starts one key early        start_plus     one key late
      truncated_start  the window is i - K // 2 .. i + K // 2 cut at key 0 (not shifted) for the first rows
      truncated_end    the same at the last rows
      k_plus_one       K + 1 keys (one more at the end, where there is one)
      ignore_shift     the compare runs on physical rows and forgets the shift (b * s) & 3 of the sequence's keys
      drop_first_tile  the first 64-key tile a 256-query workgroup walks is not walked        drop_last_tile  the last one
    (a row that would lose every key keeps its window: a row without keys has no softmax)"""
    i = torch.arange(s)[:, None]
    j = torch.arange(s)[None, :]
    lo = start(s, ks)[:, None]
    ob = key_shift(b, s)
    m = (j >= lo) & (j < lo + ks)
    if mistake in (None, "pad_leak", "scaled"):
        return m
    if mistake == "start_minus":
        w = (j >= lo - 1) & (j < lo - 1 + ks)
    elif mistake == "start_plus":
        w = (j >= lo + 1) & (j < lo + 1 + ks)
    elif mistake == "truncated_start":
        w = torch.where(i < ks // 2, (j >= 0) & (j <= i + ks // 2), m)
    elif mistake == "truncated_end":
        w = torch.where(i > s - 1 - ks // 2, (j >= i - ks // 2) & (j < s), m)
    elif mistake == "k_plus_one":
        w = (j >= lo) & (j < lo + ks + 1)
    elif mistake == "ignore_shift":
        w = (j >= lo - ob) & (j < lo - ob + ks)
    elif mistake in ("drop_first_tile", "drop_last_tile"):
        q0 = (i // QUERY_BLOCK) * QUERY_BLOCK
        q1 = (q0 + QUERY_BLOCK - 1).clamp(max=s - 1)
        st = start(s, ks)
        t_first = (ob + st[q0]) // KEY_TILE
        t_last = (ob + st[q1] + ks - 1) // KEY_TILE
        w = m & ((ob + j) // KEY_TILE != (t_first if mistake == "drop_first_tile" else t_last))
    else:
        raise ValueError(mistake)
    return torch.where(w.any(dim=1, keepdim=True), w, m)


MISTAKES = ("start_minus", "start_plus", "truncated_start", "truncated_end", "k_plus_one", "ignore_shift", "drop_first_tile", "drop_last_tile",
            "pad_leak", "scaled")


def window_attention(q, k, v, ks, scale, rnd=None, mistake=None):
    """float64 softmax(mask(q k^T * scale)) v with GQA by repeat_interleave: q [b, h, s, W], k / v [b, kvh, s, W] -> [b, s, h * W].
    rnd: the matched rounding of oracle.dit.attention_core.  mistake: see ``visible``; "pad_leak" lets the front pad keys of a shifted
    sequence (score 0, V = 0) into the softmax of the rows whose window starts at key 0, what a kernel computes that tests the window's end and
    forgets the rows below the shift; "scaled" multiplies the logits by W ** -0.5 once more, what the full-attention kernels do."""
    b, h, s, w = q.shape
    kvh = k.shape[1]
    qd, kd, vd = q.double(), k.double().repeat_interleave(h // kvh, dim=1), v.double().repeat_interleave(h // kvh, dim=1)
    dots = torch.einsum("bhid,bhjd->bhij", qd, kd) * (scale * (w ** -0.5 if mistake == "scaled" else 1.0))
    out = torch.empty((b, h, s, w), dtype=torch.float64)
    for bi in range(b):
        d = dots[bi].masked_fill(~visible(bi, s, ks, mistake)[None], float("-inf"))
        vv = vd[bi]
        if mistake == "pad_leak" and key_shift(bi, s):
            pads = key_shift(bi, s)
            lead = torch.zeros((h, s, pads), dtype=torch.float64).masked_fill((start(s, ks) > 0)[None, :, None], float("-inf"))
            d = torch.cat([lead, d], dim=-1)
            vv = torch.cat([torch.zeros((h, pads, w), dtype=torch.float64), vv], dim=1)
        m = d.amax(dim=-1, keepdim=True)
        p = torch.exp(d - m)
        l = p.sum(dim=-1, keepdim=True)
        pr = p if rnd is None else rnd(p.float()).double()
        out[bi] = torch.einsum("hij,hjd->hid", pr, vv) / l
    return out.permute(0, 2, 1, 3).reshape(b, s, h * w)


def unit_tensors(fmt, b, h, kvh, s, unscaled, seed=0):
    """(q, k, v, score scale) in fmt, 64 channels per head.  unscaled False: the standard unit tensors of the attention tests (a plain Q) with
    the scale 1 / 8; True: q and k each shrunk by 8 ** -0.5 in front of the rounding -- the same logit spread -- with the scale 1, what the plan
    runs."""
    q, _, k, v = CU.unit_tensors(fmt, 64, b, h, kvh, s, seed=seed, prescaled=False)
    if not unscaled:
        return q, k, v, 0.125
    g = 8.0 ** -0.5
    return (q.float() * g).to(fmt.dtype), (k.float() * g).to(fmt.dtype), v, 1.0


def check_ranges(tmp_path, s_max=700):
    """tests/host/attn_window_dump.cpp against csrc/attn_window.h: exit status 0 and its one summary line."""
    cxx = shutil.which("g++") or "/opt/rocm/lib/llvm/bin/clang++"
    exe = os.path.join(tmp_path, "attn_window_dump")
    subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-Werror", "-I", CSRC, os.path.join(HERE, "host", "attn_window_dump.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe, str(s_max)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout.strip()
