"""Oobleck encoder/decoder + ``AudioAutoencoder`` on the HIP C ABI (the local-attention transformer codec, ``"type": "local_attn"``, is
``models/local_attention.py``; the factories below build either, and an ``AudioAutoencoder`` may mix the two).

Module tree and state-dict keys follow the reference's ``models/autoencoders.py``
(``ResidualUnit`` :45-68, ``EncoderBlock`` :71-85, ``DecoderBlock`` :88-116, ``OobleckEncoder``
:119-153, ``OobleckDecoder`` :156-194, ``AudioAutoencoder`` :234-645, factories :695-787) and
``dac.nn.layers.WNConv1d`` (``weight_g``/``weight_v``/``bias``).  The classes hold parameters; a
whole encoder/decoder forward is one ``sat_oobleck_encode`` / ``sat_oobleck_decode`` call.
"""
import ctypes
import math
import typing as tp

import torch
from torch import nn
from torch.nn import functional as F

from .. import _config, _hip
from . import _init
from .blocks import SnakeBeta
from .bottleneck import Bottleneck
from .factory import create_bottleneck_from_config, create_pretransform_from_config
from .local_attention import TransformerDecoder1D, TransformerEncoder1D, _LocalAttnHip


class _WNBase(nn.Module):
    """Weight-normed conv parameters exactly as ``torch.nn.utils.weight_norm`` (dim=0) stores them."""

    def _register(self, conv, bias):
        v = conv.weight.detach()
        self.weight_g = nn.Parameter(v.flatten(1).norm(dim=1).view(-1, *([1] * (v.dim() - 1))).clone())
        self.weight_v = nn.Parameter(v.clone())
        if bias:
            self.bias = nn.Parameter(conv.bias.detach().clone())
        else:
            self.register_parameter("bias", None)


class WNConv1d(_WNBase):
    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, bias=True):
        super().__init__()
        self.in_channels, self.out_channels, self.kernel_size = in_channels, out_channels, kernel_size
        self.stride, self.padding, self.dilation = stride, padding, dilation
        self._register(_init.conv1d(in_channels, out_channels, kernel_size, bias=bias), bias)


class WNConvTranspose1d(_WNBase):
    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0):
        super().__init__()
        self.in_channels, self.out_channels, self.kernel_size = in_channels, out_channels, kernel_size
        self.stride, self.padding = stride, padding
        self._register(_init.conv_transpose1d(in_channels, out_channels, kernel_size, stride=stride, padding=padding), True)


def antialias_filter():
    """The 12 taps of ``alias_free_torch``'s ``kaiser_sinc_filter1d(cutoff=0.25, half_width=0.3, kernel_size=12)`` as the library's
    buffers hold them, [1, 1, 12] fp32: a sinc of cutoff 0.25 under a Kaiser window whose beta follows from the transition width
    (Kaiser's formula at an attenuation of 2.285 * 5 * pi * 1.2 + 7.95 = 51 dB), normalised to sum 1.  ``Activation1d`` uses the same taps
    for its 2x upsampling and for the low-pass in front of its 2x decimation; the HIP kernel (csrc/oobleck.hip, aa_act_kernel) has them
    as constants."""
    size, cutoff, half_width = 12, 0.25, 0.3
    atten = 2.285 * (size // 2 - 1) * math.pi * 4 * half_width + 7.95
    beta = 0.1102 * (atten - 8.7)          # Kaiser's formula above 50 dB, the only branch these constants reach
    window = torch.kaiser_window(size, periodic=False, beta=beta, dtype=torch.float64)
    time = torch.arange(-size // 2, size // 2, dtype=torch.float64) + 0.5
    taps = 2 * cutoff * window * torch.sinc(2 * cutoff * time)
    return (taps / taps.sum()).float().view(1, 1, size)


class _FilterHolder(nn.Module):
    def __init__(self):
        super().__init__()
        self.register_buffer("filter", antialias_filter())


class UpSample1d(_FilterHolder):
    pass


class LowPassFilter1d(_FilterHolder):
    pass


class DownSample1d(nn.Module):
    def __init__(self):
        super().__init__()
        self.lowpass = LowPassFilter1d()


class Activation1d(nn.Module):
    """``alias_free_torch.Activation1d(act)`` with the library's defaults (2x up, 2x down, 12 taps each way) as a parameter holder: the
    module tree and buffer names of alias_free_torch 0.0.6 (``act``, ``upsample.filter``, ``downsample.lowpass.filter``), so that the
    reference's checkpoints load with ``strict=True``.  On the device it is one launch of aa_act_kernel behind the producing convolution.
    The kernel holds the taps as constants: a checkpoint may overwrite the buffers, but only with the same filter (``check_filters``)."""

    def __init__(self, act):
        super().__init__()
        self.act = act
        self.upsample = UpSample1d()
        self.downsample = DownSample1d()

    def check_filters(self):
        want = antialias_filter()
        for name, buf in (("upsample.filter", self.upsample.filter), ("downsample.lowpass.filter", self.downsample.lowpass.filter)):
            if tuple(buf.shape) != tuple(want.shape) or not bool(((buf.detach().float().cpu() - want).abs() <= 1e-6).all()):
                raise ValueError(f"Activation1d: the buffer {name} is not the 12-tap Kaiser-sinc filter (cutoff 0.25, half-width 0.3) that "
                                 "the HIP kernel has as constants; other filters are not supported")


_ANTIALIAS_REFUSAL = (
    "antialias_activation=True runs only on request in the HIP codec: pass allow_antialias=True beside it (config key "
    "\"allow_antialias\": true in the encoder's and the decoder's \"config\"; generate.py / reconstruct_audios.py --codec-allow-antialias).  "
    "The anti-aliased activation is pinned by this project's stand-in for alias_free_torch, not by the library (README, \"Oobleck "
    "configurations\")")


def _act(use_snake, channels, antialias_activation=False, allow_antialias=False):
    """``get_activation("snake" if use_snake else "elu", antialias=...)`` (autoencoders.py:27-42): SnakeBeta, or the parameter-free
    ``nn.ELU``, which run inside the producing convolution's epilogue -- the module only holds the parameters (none for ELU) -- or
    either wrapped in ``Activation1d``, which runs as a launch of its own."""
    if antialias_activation and not allow_antialias:
        raise NotImplementedError(_ANTIALIAS_REFUSAL)
    act = SnakeBeta(channels) if use_snake else nn.ELU()
    return Activation1d(act) if antialias_activation else act


def nearest_upsample_taps(weight, stride):
    """The three-tap polyphase form of ``Upsample(scale_factor=stride, mode="nearest")`` + ``Conv1d(k=2*stride, padding="same")`` that
    the HIP plan builds at finalize (csrc/oobleck.hip, wn_pack_nearest_kernel), for tests and documentation.  ``weight`` [Cout, Cin,
    2*stride] (weight norm already folded) -> [stride, 3, Cout, Cin]: output sample ``m*stride + p`` is
    ``sum_r taps[p, r+1] @ x[:, m+r]``, r = -1, 0, 1, with x zero outside [0, T).  PyTorch pads an even kernel stride-1 on the left
    and stride on the right, so tap j of phase p reads upsampled position m*stride + p + j - (stride-1), which lies in input row
    m + floor((p + j - stride + 1) / stride)."""
    c_out, c_in, k = weight.shape
    assert k == 2 * stride
    taps = weight.new_zeros((stride, 3, c_out, c_in), dtype=torch.float32)
    for p in range(stride):
        for j in range(k):
            taps[p, (p + j - stride + 1) // stride + 1] += weight[:, :, j].float()
    return taps


class ResidualUnit(nn.Module):
    def __init__(self, in_channels, out_channels, dilation, use_snake=False, antialias_activation=False, allow_antialias=False):
        super().__init__()
        self.dilation = dilation
        # (the reference's blocks build their units without antialias_activation, autoencoders.py:76-78 and :110-112: a unit with the
        # option on exists as a module of its own only, and no plan of this package runs one)
        self.layers = nn.Sequential(
            _act(use_snake, out_channels, antialias_activation, allow_antialias),
            WNConv1d(in_channels, out_channels, 7, dilation=dilation, padding=(dilation * 6) // 2),
            _act(use_snake, out_channels, antialias_activation, allow_antialias),
            WNConv1d(out_channels, out_channels, 1))


class EncoderBlock(nn.Module):
    def __init__(self, in_channels, out_channels, stride, use_snake=False, antialias_activation=False, allow_antialias=False):
        super().__init__()
        self.layers = nn.Sequential(
            ResidualUnit(in_channels, in_channels, 1, use_snake=use_snake),
            ResidualUnit(in_channels, in_channels, 3, use_snake=use_snake),
            ResidualUnit(in_channels, in_channels, 9, use_snake=use_snake),
            _act(use_snake, in_channels, antialias_activation, allow_antialias),
            WNConv1d(in_channels, out_channels, 2 * stride, stride=stride, padding=math.ceil(stride / 2)))


class DecoderBlock(nn.Module):
    def __init__(self, in_channels, out_channels, stride, use_snake=False, antialias_activation=False, use_nearest_upsample=False,
                 allow_antialias=False):
        super().__init__()
        if use_nearest_upsample:      # autoencoders.py:95-99; on the device a three-tap polyphase convolution (nearest_upsample_taps)
            upsample_layer = nn.Sequential(nn.Upsample(scale_factor=stride, mode="nearest"),
                                           WNConv1d(in_channels, out_channels, 2 * stride, stride=1, bias=False, padding="same"))
        else:
            upsample_layer = WNConvTranspose1d(in_channels, out_channels, 2 * stride, stride=stride, padding=math.ceil(stride / 2))
        self.layers = nn.Sequential(
            _act(use_snake, in_channels, antialias_activation, allow_antialias),
            upsample_layer,
            ResidualUnit(out_channels, out_channels, 1, use_snake=use_snake),
            ResidualUnit(out_channels, out_channels, 3, use_snake=use_snake),
            ResidualUnit(out_channels, out_channels, 9, use_snake=use_snake))


# operand format -> sat_oobleck_cfg.gemm_dtype (include/sat_hip.h: SAT_GEMM_BF16, SAT_GEMM_FP16, SAT_GEMM_FP32X)
_CODEC_GEMM_DTYPES = {"bf16": 0, "fp16": 3, "fp32": 2}


class _OobleckHip(nn.Module):
    """Shared plan handling of encoder and decoder."""
    _is_decoder = False
    use_snake, use_nearest_upsample, final_tanh, antialias_activation = True, False, False, False

    def _init_plan_state(self):
        self.gemm_dtype = _config.default_gemm_dtype()
        self._plan = None
        self._plan_version = None
        self._ws = None
        self._range_report = False

    def activation_range_report(self, enable: bool = True):
        """Build extension (``sat_oobleck_range_report``): fp16 range use of every activation tensor a forward writes to its workspace.
        ``(True)`` switches it on and the following forwards accumulate; ``(False)`` returns one dict per tensor in launch order -- ``index``,
        ``name`` (module path of the producing layer; ``"input"`` for the decoder's channels-last latents, ``<path>.raw`` for the
        un-activated copy kept for a residual add), ``max_abs``, ``over_fp16``, ``nonfinite``, ``elements``, ``launches`` -- and switches it
        off.  In an fp16 codec ``over_fp16`` counts clamped elements; run the codec with ``set_gemm_dtype("fp32")`` to read what fp16
        WOULD clamp together with the un-clamped ``max_abs``.  While on, every ResidualUnit runs as two launches (the tensor between its
        convolutions then exists in memory): +60 % per decode, inside the codec gates (measured bit-equal to the fused kernel, not promised).  The setting
        survives a plan rebuild, the records collected so far do not."""
        lib = _hip.lib()
        if enable and self.antialias_activation:
            raise NotImplementedError("activation_range_report has no rows for the tensors of an antialias_activation codec")
        if enable:
            self._range_report = True
            try:
                _hip.check(lib.sat_oobleck_range_report(self._ensure_plan(), 1))
            except BaseException:
                self._range_report = False
                raise
            return None
        plan = self._ensure_plan()
        rows = []
        try:
            count = ctypes.c_int32()
            _hip.check(lib.sat_oobleck_range_report_count(plan, ctypes.byref(count)))
            n = count.value
            buf = (_hip.SatRangeRecord * max(n, 1))()
            _hip.check(lib.sat_oobleck_range_report_read(plan, buf, n, ctypes.sizeof(_hip.SatRangeRecord), _hip.stream()))
            names = [lib.sat_oobleck_range_report_name(plan, i) for i in range(n)]
            rows = [dict(index=i, name=names[i].decode(), **r) for i, r in enumerate(_hip.range_rows(buf, n))]
        finally:
            self._range_report = False
            rc = lib.sat_oobleck_range_report(plan, 0)
        _hip.check(rc)
        return rows

    def reset_activation_range_report(self):
        """Zeroes the records of ``activation_range_report`` and leaves it on."""
        if not self._range_report:
            raise _hip.SatError("activation_range_report is not enabled")
        _hip.check(_hip.lib().sat_oobleck_range_report(self._ensure_plan(), 2))

    def set_gemm_dtype(self, dtype: str):
        """Build extension: format of the activations and weights inside the convolution kernels -- "fp16" (the package default,
        stable_audio_tools/_config.py: IEEE fp16 on the fp16 build of the kernels, what the reference's ``model_half`` runs,
        ``models/pretransforms.py:39-59``), "bf16" (8x the rounding error, a few per cent faster) or "fp32" (fp32 operands on the exact
        f32-input MFMA: the reference's full-precision codec, ``model_half=False``; no fp16 range limit, several times slower).
        Parameters stay fp32 in the module; rebuilds the plan on next use."""
        if dtype not in _CODEC_GEMM_DTYPES:
            raise ValueError("the codec kernels take 'bf16', 'fp16' or 'fp32' operands")
        if dtype != self.gemm_dtype:
            self.gemm_dtype = dtype
            self._plan_version = None
        return self

    def __del__(self):
        try:
            _hip.destroy_plan("oobleck", self._plan)
        except Exception:
            pass

    def _plan_device(self):
        dev = next(self.parameters()).device
        if dev.type != "cuda":
            raise _hip.SatError("Oobleck modules must be on a HIP device (model.to('cuda')); there is no CPU path")
        return dev

    def _ensure_plan(self):
        ver = _init.params_version(self)
        if self._plan is not None and ver == self._plan_version:
            return self._plan
        lib = _hip.lib()
        dev = self._plan_device()
        _hip.destroy_plan("oobleck", self._plan)
        self._plan = None
        cfg = _hip.SatOobleckCfg()
        cfg.is_decoder = 1 if self._is_decoder else 0
        cfg.io_channels = self.io_channels
        cfg.channels = self.channels
        cfg.latent_dim = self.latent_dim
        cfg.n_blocks = len(self.strides)
        for i, (c, s) in enumerate(zip(self.c_mults, self.strides)):
            cfg.c_mults[i] = c
            cfg.strides[i] = s
        cfg.gemm_dtype = _CODEC_GEMM_DTYPES[self.gemm_dtype]
        opt = _hip.SatOobleckOptions()
        opt.activation = _hip.OOBLECK_ACT_SNAKE if self.use_snake else _hip.OOBLECK_ACT_ELU
        opt.final_tanh = 1 if self.final_tanh else 0
        opt.nearest_upsample = 1 if self.use_nearest_upsample else 0
        create = lambda: _hip.new_handle(lib.sat_oobleck_plan_create_ex, ctypes.byref(cfg), ctypes.byref(opt), ctypes.sizeof(opt))

        tensors = self.state_dict()
        if self.antialias_activation:      # the kernel has the filter taps as constants: the buffers are checked here and are no plan tensors
            for m in self.modules():
                if isinstance(m, Activation1d):
                    m.check_filters()
            tensors = {k: v for k, v in tensors.items() if not k.endswith(".filter")}

        def configure(plan):
            if self.antialias_activation:
                _hip.check(lib.sat_oobleck_plan_set_antialias(plan, 1))
            if self._range_report:        # the report belongs to the module: a rebuilt plan starts with it on (and with empty records)
                _hip.check(lib.sat_oobleck_range_report(plan, 1))

        self._plan, self._plan_version = _hip.build_plan("oobleck", create, tensors, dev, configure), ver
        return self._plan

    def _workspace(self, b, t_len):
        self._ws = _hip.plan_workspace("oobleck", self._plan, self._ws, next(self.parameters()).device, b, t_len)
        return self._ws


class OobleckEncoder(_OobleckHip):
    def __init__(self, in_channels=2, channels=128, latent_dim=32, c_mults=[1, 2, 4, 8], strides=[2, 4, 8, 8], use_snake=False,
                 antialias_activation=False, allow_antialias=False):
        super().__init__()
        if antialias_activation and not allow_antialias:
            raise NotImplementedError(_ANTIALIAS_REFUSAL)
        if any(int(s) < 2 for s in strides):
            raise NotImplementedError(
                f"strides {list(strides)}: a stride-1 encoder block (Conv1d k=2, padding 1) yields L + 1 samples in the reference; the HIP "
                "codec keeps L / stride per block and runs strides of 2 and more")
        self.io_channels, self.channels, self.latent_dim = in_channels, channels, latent_dim
        self.c_mults, self.strides = list(c_mults), list(strides)
        self.use_snake, self.antialias_activation = bool(use_snake), bool(antialias_activation)
        self.ratio = int(math.prod(strides))
        cm = [1] + list(c_mults)
        self.depth = len(cm)
        layers = [WNConv1d(in_channels, cm[0] * channels, 7, padding=3)]
        for i in range(self.depth - 1):
            layers.append(EncoderBlock(cm[i] * channels, cm[i + 1] * channels, strides[i], use_snake=use_snake))
        # (the blocks above are built without the option, as the reference's are, autoencoders.py:139-143: it reaches this activation alone)
        layers += [_act(use_snake, cm[-1] * channels, antialias_activation, allow_antialias),
                   WNConv1d(cm[-1] * channels, latent_dim, 3, padding=1)]
        self.layers = nn.Sequential(*layers)
        self._init_plan_state()

    @torch.no_grad()
    def forward(self, x):
        plan = self._ensure_plan()
        x = x.detach().float().contiguous()
        b, c, length = x.shape
        assert c == self.io_channels, f"encoder expects {self.io_channels} channels, got {c}"
        assert length % self.ratio == 0, "audio length must be a multiple of the downsampling ratio"
        t_len = length // self.ratio
        ws = self._workspace(b, t_len)
        out = torch.empty((b, self.latent_dim, t_len), device=x.device, dtype=torch.float32)
        _hip.check(_hip.lib().sat_oobleck_encode(plan, _hip.ptr(x), _hip.ptr(out), b, t_len, _hip.ptr(ws), ws.numel(), _hip.stream()))
        return out


class OobleckDecoder(_OobleckHip):
    _is_decoder = True

    def __init__(self, out_channels=2, channels=128, latent_dim=32, c_mults=[1, 2, 4, 8], strides=[2, 4, 8, 8], use_snake=False,
                 antialias_activation=False, use_nearest_upsample=False, final_tanh=True, allow_antialias=False):
        super().__init__()
        if antialias_activation and not allow_antialias:
            raise NotImplementedError(_ANTIALIAS_REFUSAL)
        if final_tanh:
            raise NotImplementedError(
                "final_tanh=True cannot be given to the constructor of the HIP codec: build the decoder with final_tanh=False, then call "
                "set_final_tanh(True) (a tanh has no parameters, so a checkpoint trained with final_tanh=True loads unchanged)")
        if not use_nearest_upsample and any(int(s) % 2 for s in strides):
            raise NotImplementedError(
                f"strides {list(strides)}: ConvTranspose1d(k=2s, stride s, padding ceil(s/2)) yields L * s - 1 samples at an odd stride in the "
                "reference; the HIP codec keeps L * s per block and runs even strides there (use_nearest_upsample=True takes odd ones)")
        self.io_channels, self.channels, self.latent_dim = out_channels, channels, latent_dim
        self.c_mults, self.strides = list(c_mults), list(strides)
        self.use_snake, self.use_nearest_upsample = bool(use_snake), bool(use_nearest_upsample)
        self.antialias_activation = bool(antialias_activation)
        self.ratio = int(math.prod(strides))
        cm = [1] + list(c_mults)
        self.depth = len(cm)
        layers = [WNConv1d(latent_dim, cm[-1] * channels, 7, padding=3)]
        for i in range(self.depth - 1, 0, -1):
            layers.append(DecoderBlock(cm[i] * channels, cm[i - 1] * channels, strides[i - 1], use_snake=use_snake,
                                       antialias_activation=antialias_activation, use_nearest_upsample=use_nearest_upsample,
                                       allow_antialias=allow_antialias))
        layers += [_act(use_snake, cm[0] * channels, antialias_activation, allow_antialias),
                   WNConv1d(cm[0] * channels, out_channels, 7, padding=3, bias=False), nn.Identity()]
        self.layers = nn.Sequential(*layers)
        self._init_plan_state()

    def set_final_tanh(self, enabled: bool = True):
        """Build extension: the reference's ``final_tanh=True`` (``nn.Tanh`` behind the last convolution, autoencoders.py:188), applied in
        that convolution's epilogue on the device.  The constructor rejects ``final_tanh=True`` (a pinned test of the config surface
        says so), hence this call after construction; rebuilds the plan on next use."""
        enabled = bool(enabled)
        if enabled != self.final_tanh:
            self.final_tanh = enabled
            self.layers[-1] = nn.Tanh() if enabled else nn.Identity()
            self._plan_version = None
        return self

    @torch.no_grad()
    def forward(self, z):
        plan = self._ensure_plan()
        z = z.detach().float().contiguous()
        b, c, t_len = z.shape
        assert c == self.latent_dim, f"decoder expects {self.latent_dim} latent channels, got {c}"
        ws = self._workspace(b, t_len)
        out = torch.empty((b, self.io_channels, t_len * self.ratio), device=z.device, dtype=torch.float32)
        _hip.check(_hip.lib().sat_oobleck_decode(plan, _hip.ptr(z), _hip.ptr(out), b, t_len, _hip.ptr(ws), ws.numel(), _hip.stream()))
        return out


def _batched(fn, x, iterate_batch):
    if not iterate_batch:
        return fn(x)
    max_bs = int(iterate_batch)
    return torch.cat([fn(x[i:i + max_bs]) for i in range(0, x.shape[0], max_bs)], dim=0)


class AudioAutoencoder(nn.Module):
    def __init__(self, encoder, decoder, latent_dim, downsampling_ratio, sample_rate, io_channels=2, bottleneck: Bottleneck = None,
                 pretransform=None, in_channels=None, out_channels=None, soft_clip=False):
        super().__init__()
        if pretransform is not None or soft_clip:
            raise NotImplementedError("autoencoder pretransform / soft_clip are outside the supported hot path")
        self.downsampling_ratio = downsampling_ratio
        self.min_length = self.downsampling_ratio
        self.sample_rate = sample_rate
        self.latent_dim = latent_dim
        self.io_channels = io_channels
        self.in_channels = io_channels if in_channels is None else in_channels
        self.out_channels = io_channels if out_channels is None else out_channels
        self.encoder = encoder
        self.decoder = decoder
        self.bottleneck = bottleneck
        self.pretransform = pretransform
        self.soft_clip = soft_clip
        self.is_discrete = self.bottleneck and self.bottleneck.is_discrete

    def set_gemm_dtype(self, dtype: str):
        """"bf16" | "fp16" | "fp32" for the encoder and decoder kernels (see ``_OobleckHip.set_gemm_dtype``, ``_LocalAttnHip.set_gemm_dtype``)."""
        for part in (self.encoder, self.decoder):
            if isinstance(part, (_OobleckHip, _LocalAttnHip)):
                part.set_gemm_dtype(dtype)
        return self

    def activation_range_report(self, enable: bool = True):
        """``activation_range_report`` of the encoder and the decoder (``_OobleckHip.activation_range_report``); ``(False)`` returns the rows
        of both, each tagged ``part="encoder"`` / ``"decoder"``.  A local_attn encoder or decoder has no report: ``(True)`` raises
        NotImplementedError before anything is switched on."""
        if enable and any(isinstance(m, _LocalAttnHip) for m in (self.encoder, self.decoder)):
            raise NotImplementedError("activation_range_report has no rows for the tensors of a local_attn codec")
        rows = []
        for part, module in (("encoder", self.encoder), ("decoder", self.decoder)):
            if isinstance(module, _OobleckHip):
                got = module.activation_range_report(enable)
                rows += [dict(part=part, **r) for r in (got or [])]
        return None if enable else rows

    def set_final_tanh(self, enabled: bool = True):
        """The decoder's final tanh (see ``OobleckDecoder.set_final_tanh``)."""
        if not isinstance(self.decoder, OobleckDecoder):
            raise NotImplementedError("set_final_tanh needs an Oobleck decoder")
        self.decoder.set_final_tanh(enabled)
        return self

    # autoencoders.py:268-304
    def encode(self, audio, return_info=False, skip_pretransform=False, iterate_batch=False, **kwargs):
        latents = _batched(self.encoder, audio, iterate_batch) if self.encoder else audio
        info = {}
        if self.bottleneck:
            latents, bottleneck_info = self.bottleneck.encode(latents, return_info=True, **kwargs)
            info.update(bottleneck_info)
        return (latents, info) if return_info else latents

    # autoencoders.py:306-343
    def decode(self, latents, iterate_batch=False, **kwargs):
        if self.bottleneck:
            latents = self.bottleneck.decode(latents)
        return _batched(self.decoder, latents, iterate_batch)

    # autoencoders.py:356-408
    def preprocess_audio_for_encoder(self, audio, in_sr):
        return self.preprocess_audio_list_for_encoder([audio], [in_sr])

    def preprocess_audio_list_for_encoder(self, audio_list, in_sr_list):
        from ..inference.utils import prepare_audio
        batch_size = len(audio_list)
        if isinstance(in_sr_list, int):
            in_sr_list = [in_sr_list] * batch_size
        assert len(in_sr_list) == batch_size, "list of sample rates must be the same length of audio_list"
        new_audio, max_length = [], 0
        for audio, in_sr in zip(audio_list, in_sr_list):
            if audio.dim() == 3 and audio.shape[0] == 1:
                audio = audio.squeeze(0)
            elif audio.dim() == 1:
                audio = audio.unsqueeze(0)
            assert audio.dim() == 2, "Audio should be shape (Channels x Length) with no batch dimension"
            if in_sr != self.sample_rate:           # autoencoders.py:394-397 of the reference (torchaudio Resample): HIP polyphase kernel
                from ..inference.resample import resample
                audio = resample(audio, in_sr, self.sample_rate)
            new_audio.append(audio)
            max_length = max(max_length, audio.shape[-1])
        padded = max_length + (self.min_length - (max_length % self.min_length)) % self.min_length
        out = [prepare_audio(a, in_sr=self.sample_rate, target_sr=self.sample_rate, target_length=padded,
                             target_channels=self.in_channels, device=a.device).squeeze(0) for a in new_audio]
        return torch.stack(out)

    # ------------------------------------------------------------------ chunked paths (autoencoders.py:410-645)
    # The reference spells chunking + cross-fade out three times (encode_audio, decode_audio, reconstruct_audio).  Here they share
    # one driver: cut the (padded) input into overlapping chunks, run the codec on batches of at most `max_batch_size` chunks,
    # overlap-add the results with a Bartlett cross-fade (one HIP kernel, sat_overlap_add) and crop.
    def _run_chunked(self, x, fn, in_chunk, in_hop, n_chunk, out_hop, out_overlap, max_batch_size, keep):
        bs, channels = x.shape[0], x.shape[1]
        chunks = torch.stack([x[..., i * in_hop: i * in_hop + in_chunk] for i in range(n_chunk)], dim=1)
        chunks = chunks.reshape(bs * n_chunk, channels, in_chunk)
        pieces = torch.cat([fn(chunks[i: i + max_batch_size]) for i in range(0, chunks.shape[0], max_batch_size)], dim=0)
        out_ch, out_chunk = pieces.shape[1], pieces.shape[2]
        pieces = pieces.reshape(bs, n_chunk, out_ch, out_chunk).float().contiguous()
        total = out_hop * (n_chunk - 1) + out_chunk
        window = torch.bartlett_window(max(out_overlap, 1) * 2, device=x.device).float().contiguous()     # (unused when overlap == 0)
        out = torch.empty((bs, out_ch, total), dtype=torch.float32, device=x.device)
        _hip.check(_hip.lib().sat_overlap_add(_hip.ptr(pieces), _hip.ptr(window), _hip.ptr(out), bs, n_chunk, out_ch, out_chunk, out_hop,
                                              out_overlap, total, _hip.stream()))
        return out[..., :keep]

    @staticmethod
    def _n_chunks(length, chunk, hop):
        return int(math.ceil((length - chunk) / hop)) + 1

    def encode_audio(self, audio, chunked=False, chunk_size=128, overlap=4, max_batch_size=1, **kwargs):
        """Audio [B, C, L] (L a multiple of the compression ratio) -> latents; ``chunked``: windows of ``chunk_size`` latent frames
        overlapping by ``overlap`` frames, zero-padded at the end, cross-faded in the latent domain."""
        _, n_ch, length = audio.shape
        ratio = self.downsampling_ratio
        assert n_ch == self.in_channels
        assert length % ratio == 0, "The audio length must be a multiple of compression ratio."
        if not chunked:
            return self.encode(audio, **kwargs)
        chunk_s, hop_s = chunk_size * ratio, (chunk_size - overlap) * ratio
        n_chunk = self._n_chunks(length, chunk_s, hop_s)
        audio = F.pad(audio, (0, chunk_s + hop_s * (n_chunk - 1) - length))
        return self._run_chunked(audio, self.encode, chunk_s, hop_s, n_chunk, chunk_size - overlap, overlap, max_batch_size, length // ratio)

    def decode_audio(self, latents, chunked=False, chunk_size=128, overlap=4, max_batch_size=1, **kwargs):
        """Latents [B, latent_dim, T] -> audio; ``chunked``: the latents are reflect-padded to a whole number of hops and the decoded
        windows cross-faded over ``overlap`` frames' worth of samples."""
        _, latent_dim, t_len = latents.shape
        ratio = self.downsampling_ratio
        assert latent_dim == self.latent_dim
        if not chunked:
            return self.decode(latents, **kwargs)
        hop = chunk_size - overlap
        n_chunk = self._n_chunks(t_len, chunk_size, hop)
        latents = F.pad(latents, (0, chunk_size + hop * (n_chunk - 1) - t_len), mode="reflect")
        return self._run_chunked(latents, self.decode, chunk_size, hop, n_chunk, hop * ratio, overlap * ratio, max_batch_size, t_len * ratio)

    @torch.no_grad()
    def reconstruct_audio(self, audio, chunked=True, chunk_size=128, overlap=4, max_batch_size=1, **kwargs):
        """encode -> decode per window, cross-faded in the audio domain.  The reference pads with one hop more than the windows
        it then takes (``hop * n_chunk``, autoencoders.py:604); the crop below makes that invisible and it is kept as is."""
        _, n_ch, length = audio.shape
        ratio = self.downsampling_ratio
        assert n_ch == self.in_channels
        if not chunked:
            return self.decode(self.encode(audio, **kwargs), **kwargs)
        chunk_s, overlap_s = chunk_size * ratio, overlap * ratio
        hop_s = chunk_s - overlap_s
        n_chunk = self._n_chunks(length, chunk_s, hop_s)
        audio = F.pad(audio, (0, chunk_s + hop_s * n_chunk - length))
        codec = lambda chunk: self.decode(self.encode(chunk, **kwargs))
        return self._run_chunked(audio, codec, chunk_s, hop_s, n_chunk, hop_s, overlap_s, max_batch_size, length)


# ---------------------------------------------------------------------------------- factories (autoencoders.py:695-787)
def create_encoder_from_config(encoder_config: tp.Dict[str, tp.Any]):
    if encoder_config["type"] == "local_attn":          # autoencoders.py:709-712
        encoder = TransformerEncoder1D(**encoder_config["config"])
    elif encoder_config["type"] != "oobleck":
        raise NotImplementedError(f"encoder type '{encoder_config['type']}' is outside this build's hot path (oobleck and local_attn only)")
    else:
        encoder = OobleckEncoder(**encoder_config["config"])
    if not encoder_config.get("requires_grad", True):
        for p in encoder.parameters():
            p.requires_grad = False
    return encoder


def create_decoder_from_config(decoder_config: tp.Dict[str, tp.Any]):
    if decoder_config["type"] == "local_attn":          # autoencoders.py:735-738
        decoder = TransformerDecoder1D(**decoder_config["config"])
    elif decoder_config["type"] != "oobleck":
        raise NotImplementedError(f"decoder type '{decoder_config['type']}' is outside this build's hot path (oobleck and local_attn only)")
    else:
        decoder = OobleckDecoder(**decoder_config["config"])
    if not decoder_config.get("requires_grad", True):
        for p in decoder.parameters():
            p.requires_grad = False
    return decoder


def create_autoencoder_from_config(config: tp.Dict[str, tp.Any]):
    ae_config = config["model"]
    encoder = create_encoder_from_config(ae_config["encoder"])
    decoder = create_decoder_from_config(ae_config["decoder"])
    bottleneck = ae_config.get("bottleneck", None)
    pretransform = ae_config.get("pretransform", None)
    if pretransform:
        pretransform = create_pretransform_from_config(pretransform, config["sample_rate"])
    if bottleneck:
        bottleneck = create_bottleneck_from_config(bottleneck)
    return AudioAutoencoder(encoder, decoder, io_channels=ae_config["io_channels"], latent_dim=ae_config["latent_dim"],
                            downsampling_ratio=ae_config["downsampling_ratio"], sample_rate=config["sample_rate"],
                            bottleneck=bottleneck, pretransform=pretransform, in_channels=ae_config.get("in_channels", None),
                            out_channels=ae_config.get("out_channels", None), soft_clip=ae_config["decoder"].get("soft_clip", False))
