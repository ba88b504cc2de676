"""float64 restatement of the convolution GEMM of the convolutional feed-forward (sat_dit_plan_set_ff_conv, csrc/ff_conv.hip), shared by
tests/test_dit_conv_ff_host.py (CPU: the restatement is F.conv1d, the gates see the faults) and tests/test_gpu_conv_ff_kernels.py (GPU: the
kernel against it).

    acc[b, s, :] = sum_j w[:, :, j] . a[b, s + j - k // 2, :],   rows outside [0, S) of sequence b are zero

as ONE contraction of length k * K: the rows of the window side by side (gather_rows) times the tap-major weight (pack_taps)."""
import torch
import torch.nn.functional as F

UNIT = 2.0 ** -24


def pack_taps(w):
    """Conv1d weight [N, K, k] -> tap-major [N, k * K]: out[n, j * K + c] = w[n, c, j] (what finalize packs)."""
    n, kk, k = w.shape
    return w.permute(0, 2, 1).reshape(n, k * kk)


def gather_rows(a, taps=None, order=None, leak=False, guard=0.0):
    """a [B, S, K] -> [B * S, k * K]: row (b, s) holds a[b, s + j - k // 2] for j = 0..k-1, zeros outside the sequence.
    The faults of the host test: ``order`` another tap order, ``leak`` rows outside the sequence taken from the neighbouring sequence (the
    flat [B * S] buffer) instead of zero, ``guard`` a non-zero value in the rows outside."""
    b, s, kk = a.shape
    k = taps
    order = list(range(k)) if order is None else order
    flat = a.reshape(b * s, kk)
    cols = []
    for j in order:
        sh = j - k // 2
        pos = torch.arange(s) + sh
        ok = ((pos >= 0) & (pos < s)).repeat(b)
        m = torch.arange(b * s) + sh
        inside = (m >= 0) & (m < b * s)
        rows = flat[m.clamp(0, b * s - 1)]
        out = torch.where(ok[:, None], rows, torch.full_like(rows, guard))
        if leak:
            out = torch.where((~ok & inside)[:, None], rows, out)
        cols.append(out)
    return torch.cat(cols, dim=1)


def conv_gemm(a, w, bias=None, dt=torch.float64, **fault):
    """[B * S, N] = gather_rows(a) @ pack_taps(w)^T (+ bias), evaluated in dt."""
    a, w = a.to(dt), w.to(dt)
    out = gather_rows(a, taps=w.shape[2], **fault) @ pack_taps(w).T
    return out if bias is None else out + bias.to(dt)


def conv1d_reference(a, w, bias=None, dt=torch.float64):
    """The same through F.conv1d on [B, K, S], padding k // 2: what the reference's FeedForward runs."""
    k = w.shape[2]
    y = F.conv1d(a.to(dt).transpose(1, 2), w.to(dt), None if bias is None else bias.to(dt), padding=k // 2)
    return y.transpose(1, 2).reshape(-1, w.shape[0])


def magnitude(a, w, bias=None, c_in=None):
    """|A| |W|^T + |bias| + |C_in| of the contraction: the scale of the a-priori fp32 bound (n + 4) 2^-24 x this, n = k * K."""
    mag = conv_gemm(a.abs(), w.abs())
    if bias is not None:
        mag = mag + bias.abs().double()
    if c_in is not None:
        mag = mag + c_in.abs().double()
    return mag
