"""``FourierFeatures`` and ``SnakeBeta`` parameter containers (reference ``models/blocks.py:88-97,
318-358``).  FourierFeatures is evaluated inside ``sat_dit_forward``; SnakeBeta is fused into
the conv epilogues of the Oobleck kernels.  ``SnakeBeta.forward`` exposes the standalone HIP
kernel (``sat_snake_beta``) for parity tests.

``ResConvBlock``, ``SelfAttention1d``, ``SkipBlock``, ``Downsample1d`` and ``Upsample1d`` (reference ``models/blocks.py:14-159``) hold the
parameters of the Dance Diffusion U-Net with the reference's tree and names; they run inside ``sat_unet_forward``
(``models/diffusion.py``: ``DiffusionAttnUnet1D``) and have no forward of their own."""
import torch
from torch import nn

from .. import _hip
from . import _init


class FourierFeatures(nn.Module):
    def __init__(self, in_features, out_features, std=1.0):
        super().__init__()
        assert out_features % 2 == 0
        self.weight = nn.Parameter(torch.randn([out_features // 2, in_features]) * std)


class SnakeBeta(nn.Module):
    def __init__(self, in_features, alpha=1.0, alpha_trainable=True, alpha_logscale=True):
        super().__init__()
        if not alpha_logscale:
            raise NotImplementedError("SnakeBeta: only alpha_logscale=True (the Oobleck setting) is supported")
        self.in_features = in_features
        self.alpha_logscale = alpha_logscale
        self.alpha = nn.Parameter(torch.zeros(in_features) * alpha)
        self.beta = nn.Parameter(torch.zeros(in_features) * alpha)
        self.alpha.requires_grad = alpha_trainable
        self.beta.requires_grad = alpha_trainable
        self.no_div_by_zero = 0.000000001

    @torch.no_grad()
    def forward(self, x):
        x = x.contiguous().float()
        y = torch.empty_like(x)
        b, c, t = x.shape
        _hip.check(_hip.lib().sat_snake_beta(_hip.ptr(x), _hip.ptr(self.alpha.data), _hip.ptr(self.beta.data), _hip.ptr(y),
                                             b, c, t, _hip.stream()))
        return y


def _no_standalone_forward(module):
    raise RuntimeError(f"{type(module).__name__} has no standalone forward in this build: it runs inside DiffusionAttnUnet1D (one "
                       "sat_unet_forward call); there is no CPU/eager path")


class ResidualBlock(nn.Module):
    def __init__(self, main, skip=None):
        super().__init__()
        self.main = nn.Sequential(*main)
        self.skip = skip if skip else nn.Identity()

    def forward(self, *args, **kwargs):
        _no_standalone_forward(self)


class ResConvBlock(ResidualBlock):
    def __init__(self, c_in, c_mid, c_out, is_last=False, kernel_size=5, conv_bias=True, use_snake=False):
        if use_snake:
            raise NotImplementedError("use_snake=True: Snake1d comes from the dac library, which this build does not have")
        skip = None if c_in == c_out else _init.conv1d(c_in, c_out, 1, bias=False)
        super().__init__([
            _init.conv1d(c_in, c_mid, kernel_size, padding=kernel_size // 2, bias=conv_bias),
            nn.GroupNorm(1, c_mid),
            nn.GELU(),
            _init.conv1d(c_mid, c_out, kernel_size, padding=kernel_size // 2, bias=conv_bias),
            nn.GroupNorm(1, c_out) if not is_last else nn.Identity(),
            nn.GELU() if not is_last else nn.Identity(),
        ], skip)


class SelfAttention1d(nn.Module):
    def __init__(self, c_in, n_head=1, dropout_rate=0.):
        super().__init__()
        assert c_in % n_head == 0
        if c_in // n_head != 32:
            raise NotImplementedError(f"SelfAttention1d({c_in}, {n_head}): the U-Net plan runs 32-channel heads (what DiffusionAttnUnet1D builds)")
        if dropout_rate:
            raise NotImplementedError("SelfAttention1d: dropout is not built (inference only)")
        self.norm = nn.GroupNorm(1, c_in)
        self.n_head = n_head
        self.qkv_proj = _init.conv1d(c_in, c_in * 3, 1)
        self.out_proj = _init.conv1d(c_in, c_in, 1)
        self.dropout = nn.Dropout(dropout_rate, inplace=True)

    def forward(self, *args, **kwargs):
        _no_standalone_forward(self)


class SkipBlock(nn.Module):
    def __init__(self, *main):
        super().__init__()
        self.main = nn.Sequential(*main)

    def forward(self, *args, **kwargs):
        _no_standalone_forward(self)


_kernels = {
    "cubic": [-0.01171875, -0.03515625, 0.11328125, 0.43359375, 0.43359375, 0.11328125, -0.03515625, -0.01171875],
}


class _Resample1d(nn.Module):
    """The persistent ``kernel`` buffer is part of the tree so that a reference state dict loads with ``strict=True``; the device kernels carry
    the cubic filter as a constant, and ``check_kernel`` (called when the plan is built) refuses a buffer that holds anything else."""
    _gain = 1.0

    def __init__(self, kernel="linear", pad_mode="reflect", channels_last=False):
        super().__init__()
        if kernel != "cubic" or pad_mode != "reflect" or channels_last:
            raise NotImplementedError(f"{type(self).__name__}(kernel={kernel!r}, pad_mode={pad_mode!r}, channels_last={channels_last}): the HIP "
                                      "resamplers are built for the cubic kernel with reflect padding on channel-first input")
        self.pad_mode = pad_mode
        kernel_1d = torch.tensor(_kernels[kernel]) * self._gain
        self.pad = kernel_1d.shape[0] // 2 - 1
        self.register_buffer("kernel", kernel_1d)
        self.channels_last = channels_last

    def check_kernel(self, name="kernel"):
        want = torch.tensor(_kernels["cubic"], dtype=torch.float64) * self._gain
        have = self.kernel.detach().double().cpu()
        if have.shape != want.shape or not bool(((have - want).abs() <= 1e-6).all()):
            raise ValueError(f"{name}: the buffer is not the cubic filter{' times 2' if self._gain != 1 else ''} (to 1e-6); the HIP resamplers "
                             "carry that filter as a constant and cannot honour another")

    def forward(self, *args, **kwargs):
        _no_standalone_forward(self)


class Downsample1d(_Resample1d):
    pass


class Upsample1d(_Resample1d):
    _gain = 2.0
