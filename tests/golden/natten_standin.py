"""A stand-in for the two NATTEN functions the reference's attention calls (``natten.functional.natten1dqk`` / ``natten1dav``, models/
transformer.py:486, 493), for machines where the library is not installed: a gather over NATTEN's 1-D neighbourhood, dilation 1 (all n x n logits are formed and
the window's are gathered from them; the weights are scattered back to their keys for the value product).

Query i of a sequence of n rows owns the kernel_size keys ``start(i) .. start(i) + kernel_size - 1`` with
``start(i) = min(max(i - kernel_size // 2, 0), n - kernel_size)``: the window is shifted, not truncated, at both ends.  ``natten1dqk``
returns the logits of those keys in that order, [b, h, n, kernel_size], unscaled; ``natten1dav`` the weighted sum of the same value rows.
ValueError where NATTEN refuses: an even kernel size, one of 1 or less, another dilation than the one this stand-in has, a sequence shorter
than the kernel, q and k of different lengths.

tests/golden/make_golden_dit_natten.py sets ``natten_standin`` as the ``natten`` attribute of the imported reference transformer module; the
goldens of the family are therefore pinned by this file, not by the library.  tests/test_dit_natten_host.py checks it against a float64
masked softmax."""
import types

import torch


def window_start(n, kernel_size):
    """[n] long: the first key of every query's window"""
    i = torch.arange(n)
    return (i - kernel_size // 2).clamp(min=0, max=n - kernel_size)


def _check(kernel_size, dilation, n):
    if not isinstance(kernel_size, int) or kernel_size <= 1 or kernel_size % 2 == 0:
        raise ValueError(f"natten: kernel_size must be an odd integer greater than 1, got {kernel_size}")
    if dilation != 1:
        raise ValueError(f"natten stand-in: dilation {dilation} is not provided (the reference passes 1)")
    if n < kernel_size:
        raise ValueError(f"natten: the sequence ({n}) is shorter than kernel_size * dilation ({kernel_size})")


def _index(n, kernel_size, device):
    return (window_start(n, kernel_size)[:, None] + torch.arange(kernel_size)[None, :]).to(device)          # [n, K]


def natten1dqk(query, key, kernel_size, dilation=1):
    """query, key [b, h, n, d] -> logits [b, h, n, kernel_size], logit (i, t) = query[i] . key[start(i) + t]"""
    if query.shape != key.shape:
        raise ValueError(f"natten: query {tuple(query.shape)} and key {tuple(key.shape)} must have the same shape")
    n = query.shape[-2]
    _check(kernel_size, dilation, n)
    dots = torch.einsum("bhid,bhjd->bhij", query, key)
    return dots.gather(-1, _index(n, kernel_size, key.device).expand(*dots.shape[:-1], kernel_size))


def natten1dav(attn, value, kernel_size, dilation=1):
    """attn [b, h, n, kernel_size], value [b, h, n, d] -> [b, h, n, d] = sum_t attn[i, t] value[start(i) + t]"""
    n = value.shape[-2]
    _check(kernel_size, dilation, n)
    if attn.shape[-2] != n or attn.shape[-1] != kernel_size:
        raise ValueError(f"natten: attention weights {tuple(attn.shape)} do not fit {n} rows of kernel_size {kernel_size}")
    full = torch.zeros(*attn.shape[:-1], n, dtype=attn.dtype, device=attn.device)
    full.scatter_(-1, _index(n, kernel_size, attn.device).expand(*attn.shape), attn)          # the windows' weights at their keys, 0 elsewhere
    return torch.einsum("bhij,bhjd->bhid", full, value)


functional = types.SimpleNamespace(natten1dqk=natten1dqk, natten1dav=natten1dav)
