"""This project's own statement of ``alias_free_torch.Activation1d`` (alias_free_torch 0.0.6), for the golden generator of the
anti-aliased Oobleck codecs (make_golden_codec_antialias.py) and the host tests.  The library is not installed where the goldens are made;
the reference holds it as the module attribute ``Activation1d`` of its ``models.autoencoders``, and this class is set in its place.  The
goldens of ``antialias_activation=True`` are therefore pinned by this stand-in, not by the library.

Written from the operation's definition, not from the library's text:

    Activation1d(act), up_ratio = down_ratio = 2, 12 taps each way, per channel along time, x of T >= 1 samples
      f       the 12-tap Kaiser-windowed sinc kaiser_sinc_filter1d(cutoff=0.25, half_width=0.3, kernel_size=12), normalised to sum 1
      up      replicate-pad x by 5 samples on both sides, 2 * conv_transpose1d(stride 2) with f, cut 15 samples from each end: 2 T samples
      act     SnakeBeta or ELU on the doubled rate
      down    replicate-pad the ACTIVATED signal by 5 (left) and 6 (right), conv1d(stride 2) with f: T samples

Module tree and buffer names -- ``act``, ``upsample.filter``, ``downsample.lowpass.filter``, persistent buffers of shape [1, 1, 12] -- are
those of alias_free_torch 0.0.6 as remembered: they could not be verified against the library (README, "Oobleck configurations").
tests/test_codec_antialias_host.py holds this file against a float64 brute-force statement of the three steps and, where ``transformers``
is installed, against an independent implementation of the same operation."""
import math

import torch
import torch.nn.functional as F
from torch import nn

TAPS, CUTOFF, HALF_WIDTH = 12, 0.25, 0.3


def kaiser_sinc_filter1d(cutoff=CUTOFF, half_width=HALF_WIDTH, kernel_size=TAPS, dtype=torch.float32):
    """[1, 1, kernel_size]: sinc(2 cutoff t) under a Kaiser window at the half-sample times of an even kernel, normalised to sum 1.  The
    window's beta follows Kaiser's design formulas from the attenuation 2.285 (kernel_size / 2 - 1) pi (4 half_width) + 7.95 dB."""
    assert kernel_size % 2 == 0, "the stand-in states the even-length filter Activation1d uses"
    half = kernel_size // 2
    atten = 2.285 * (half - 1) * math.pi * 4 * half_width + 7.95
    if atten > 50.0:
        beta = 0.1102 * (atten - 8.7)
    elif atten >= 21.0:
        beta = 0.5842 * (atten - 21.0) ** 0.4 + 0.07886 * (atten - 21.0)
    else:
        beta = 0.0
    window = torch.kaiser_window(kernel_size, periodic=False, beta=beta, dtype=torch.float64)
    time = torch.arange(-half, half, dtype=torch.float64) + 0.5
    taps = 2 * cutoff * window * torch.sinc(2 * cutoff * time)
    return (taps / taps.sum()).to(dtype).view(1, 1, kernel_size)


class UpSample1d(nn.Module):
    def __init__(self):
        super().__init__()
        self.register_buffer("filter", kaiser_sinc_filter1d())

    def forward(self, x):          # [B, C, T] -> [B, C, 2 T]
        c = x.shape[1]
        x = F.pad(x, (5, 5), mode="replicate")
        x = 2 * F.conv_transpose1d(x, self.filter.to(x.dtype).expand(c, -1, -1), stride=2, groups=c)
        return x[..., 15:-15]


class LowPassFilter1d(nn.Module):
    def __init__(self):
        super().__init__()
        self.register_buffer("filter", kaiser_sinc_filter1d())

    def forward(self, x):          # [B, C, 2 T] -> [B, C, T]
        c = x.shape[1]
        x = F.pad(x, (5, 6), mode="replicate")
        return F.conv1d(x, self.filter.to(x.dtype).expand(c, -1, -1), stride=2, groups=c)


class DownSample1d(nn.Module):
    def __init__(self):
        super().__init__()
        self.lowpass = LowPassFilter1d()

    def forward(self, x):
        return self.lowpass(x)


class Activation1d(nn.Module):
    def __init__(self, activation):
        super().__init__()
        self.act = activation
        self.upsample = UpSample1d()
        self.downsample = DownSample1d()

    def forward(self, x):
        return self.downsample(self.act(self.upsample(x)))
