"""References and host-side helpers of the causal self-attention tests (tests/test_dit_causal_host.py, tests/test_gpu_dit_causal.py).

``causal_attention`` is ``oracle.dit.attention_core`` restated in float64 with the mask of csrc/attn_causal.h -- query i of a sequence sees
the keys j <= i of the same sequence -- and the same matched rounding: P = exp(s - max) is rounded to the operand format before P V, the
normaliser is the sum of the un-rounded P.  ``MISTAKES`` are the masks of kernels that are wrong on purpose; the host test shows that the
gates of the GPU test reject each of them.  ``check_ranges`` compiles attn_causal.h with the host compiler (tests/host/attn_causal_dump.cpp)
and compares it with brute force."""
import math
import os
import shutil
import subprocess

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "friendly-stable-audio-tools_amd", "csrc")
LOG2E = 1.4426950408889634
KEY_TILE = {32: 128, 64: 64, 96: 64, 128: 64}          # sk_pad is a multiple of it
SEQ_LENS = (1, 33, 64, 65, 129, 301, 645)              # one block; a diagonal block only; a full tile; one key past it; 2-3 query blocks; two groups


def qscale(w):
    return LOG2E / math.sqrt(w)          # what the producer multiplies into a pre-scaled Q


def key_shift(b, s):
    return (b * s) & 3          # the physical row of sequence b's key 0


def visible(b, s, mistake=None):
    """[s, s] bool, element (i, j): query i of sequence b sees key j.  mistake: a kernel that is wrong on purpose
      strict        j < i (row 0 keeps key 0: a row without keys has no softmax)
      plus_one      j <= i + 1
      ignore_shift  the compare runs on physical rows and forgets the shift: physical key p <= i, i.e. j <= i - (b * s & 3)
      drop_last     the 64-key tile that holds the diagonal of the sequence's last query is not walked (its queries lose their newest keys)"""
    i = torch.arange(s)[:, None]
    j = torch.arange(s)[None, :]
    ob = key_shift(b, s)
    if mistake is None or mistake == "pad_leak":
        m = j <= i
    elif mistake == "strict":
        m = j < i.clamp_min(1)
    elif mistake == "plus_one":
        m = j <= i + 1
    elif mistake == "ignore_shift":
        m = j <= (i - ob).clamp_min(0)
    elif mistake == "drop_last":
        last_tile = (ob + s - 1) // 64
        m = (j <= i) & (((ob + j) // 64 != last_tile) | (j == 0))
    else:
        raise ValueError(mistake)
    return m


MISTAKES = ("strict", "plus_one", "ignore_shift", "drop_last", "pad_leak")


def causal_attention(q, k, v, rnd=None, mistake=None):
    """float64 softmax(mask(q k^T / sqrt(W))) v with GQA by repeat_interleave: q [b, h, s, W], k / v [b, kvh, s, W] -> [b, s, h * W].
    rnd: the matched rounding of oracle.dit.attention_core.  mistake: see ``visible``; "pad_leak" lets the front pad keys of a shifted
    sequence (score 0, V = 0) into the softmax, what a kernel computes that masks the diagonal and forgets the rows below the shift."""
    b, h, s, w = q.shape
    kvh = k.shape[1]
    qd, kd, vd = q.double(), k.double().repeat_interleave(h // kvh, dim=1), v.double().repeat_interleave(h // kvh, dim=1)
    dots = torch.einsum("bhid,bhjd->bhij", qd, kd) / math.sqrt(w)
    out = torch.empty((b, h, s, w), dtype=torch.float64)
    for bi in range(b):
        d = dots[bi].masked_fill(~visible(bi, s, mistake)[None], float("-inf"))
        vv = vd[bi]
        if mistake == "pad_leak" and key_shift(bi, s):
            pads = key_shift(bi, s)
            d = torch.cat([torch.zeros((h, s, pads), dtype=torch.float64), d], dim=-1)
            vv = torch.cat([torch.zeros((h, pads, w), dtype=torch.float64), vv], dim=1)
        m = d.amax(dim=-1, keepdim=True)
        p = torch.exp(d - m)
        l = p.sum(dim=-1, keepdim=True)
        pr = p if rnd is None else rnd(p.float()).double()
        out[bi] = torch.einsum("hij,hjd->hid", pr, vv) / l
    return out.permute(0, 2, 1, 3).reshape(b, s, h * w)


def unit_tensors(fmt, w, b, h, kvh, s, seed=0, prescaled=True):
    """q (as the producer stores it: times log2(e) / sqrt(W) when prescaled), the query q_eff it stands for, k, v -- rounded to fmt, built like
    tests/test_gpu_dit_head_width.py::test_attention_hdw: the same score spread, and a late key that takes one row's maximum."""
    rand = lambda shape, sd: torch.randn(shape, generator=torch.Generator().manual_seed(sd))
    q = (rand((b, h, s, w), 12 + seed) * 1.5).to(fmt.dtype)
    k = (rand((b, kvh, s, w), 13 + seed) * 1.5).to(fmt.dtype)
    v = rand((b, kvh, s, w), 14 + seed).to(fmt.dtype)
    if s > 8:
        k[0, 0, s - 2] = q[0, 0, s - 1] * 3          # the running max of the last query jumps in its last block (rescale branch)
    if prescaled:
        q = (q.float() * qscale(w)).to(fmt.dtype)
        return q, q.float() / qscale(w), k, v
    return q, q.float(), k, v


def check_ranges(tmp_path, s_max=700):
    """tests/host/attn_causal_dump.cpp against csrc/attn_causal.h: exit status 0 and its one summary line."""
    cxx = shutil.which("g++") or "/opt/rocm/lib/llvm/bin/clang++"
    exe = os.path.join(tmp_path, "attn_causal_dump")
    subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-Werror", "-I", CSRC, os.path.join(HERE, "host", "attn_causal_dump.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe, str(s_max)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout.strip()
