"""``DiTWrapper`` / ``ConditionedDiffusionModelWrapper`` / ``create_diffusion_cond_from_config``
(reference ``models/diffusion.py:34-209, 482-529, 585-655``), and the unconditional Dance Diffusion family: ``DiffusionAttnUnet1D`` /
``DiffusionModelWrapper`` / ``create_diffusion_uncond_from_config`` (:28-52, 376-479, 552-582)."""
import ctypes
import math
import typing as tp
from functools import partial

import torch
from torch import nn

from .. import _config, _hip
from . import _init
from .blocks import Downsample1d, FourierFeatures, ResConvBlock, SelfAttention1d, SkipBlock, Upsample1d
from .conditioners import MultiConditioner, create_multi_conditioner_from_conditioning_config
from .dit import DiffusionTransformer
from .factory import create_pretransform_from_config
from .pretransforms import Pretransform


class ConditionedDiffusionModel(nn.Module):
    def __init__(self, *args, supports_cross_attention: bool = False, supports_input_concat: bool = False,
                 supports_global_cond: bool = False, supports_prepend_cond: bool = False, **kwargs):
        super().__init__(*args, **kwargs)
        self.supports_cross_attention = supports_cross_attention
        self.supports_input_concat = supports_input_concat
        self.supports_global_cond = supports_global_cond
        self.supports_prepend_cond = supports_prepend_cond


class DiTWrapper(ConditionedDiffusionModel):
    """reference models/diffusion.py:482-529.  Parameters are multiplied by 0.5 after
    construction, as the reference does (:487-489), unless built under ``skip_init``."""

    def __init__(self, *args, **kwargs):
        super().__init__(supports_cross_attention=True, supports_global_cond=False, supports_input_concat=False)
        # config-driven construction: the TransformerBlock options off the shipped configs' path (conformer, remove_norms, glu=False) are accepted
        kwargs.setdefault("allow_block_options", True)
        # ... ff_kwargs use_conv is not: a config opts in with "allow_conv_ff": true, which arrives here in kwargs and is passed on as it is
        # ... nor is patch_size > 1: "allow_patch_size": true, likewise
        # ... nor are 32- / 96-channel attention heads: "allow_head_widths": true, likewise
        # ... nor is causal=True: "allow_causal": true, likewise
        # ... nor is attn_kwargs natten_kernel_size: "allow_natten": true, likewise
        # ... nor is it off 64-channel heads: "allow_natten_head_widths": true next to it, likewise
        self.model = DiffusionTransformer(*args, **kwargs)
        from . import _init
        if not _init._SKIP:
            with torch.no_grad():
                for param in self.model.parameters():
                    param *= 0.5

    def forward(self, x, t, cross_attn_cond=None, cross_attn_mask=None, negative_cross_attn_cond=None,
                negative_cross_attn_mask=None, input_concat_cond=None, negative_input_concat_cond=None, global_cond=None,
                negative_global_cond=None, prepend_cond=None, prepend_cond_mask=None, cfg_scale=1.0,
                cfg_dropout_prob: float = 0.0, batch_cfg: bool = True, rescale_cfg: bool = False, scale_phi: float = 0.0,
                **kwargs):
        assert batch_cfg, "batch_cfg must be True for DiTWrapper"
        # rescale_cfg is accepted and ignored, exactly like the reference
        return self.model(x, t, cross_attn_cond=cross_attn_cond, cross_attn_cond_mask=cross_attn_mask,
                          negative_cross_attn_cond=negative_cross_attn_cond, negative_cross_attn_mask=negative_cross_attn_mask,
                          input_concat_cond=input_concat_cond, prepend_cond=prepend_cond, prepend_cond_mask=prepend_cond_mask,
                          cfg_scale=cfg_scale, cfg_dropout_prob=cfg_dropout_prob, scale_phi=scale_phi, global_embed=global_cond,
                          **kwargs)


class ConditionedDiffusionModelWrapper(nn.Module):
    """A diffusion model that takes in conditioning (reference models/diffusion.py:90-209)."""

    def __init__(self, model: ConditionedDiffusionModel, conditioner: MultiConditioner, io_channels, sample_rate,
                 min_input_length: int, diffusion_objective: str = "v", pretransform: tp.Optional[Pretransform] = None,
                 cross_attn_cond_ids: tp.List[str] = [], global_cond_ids: tp.List[str] = [], input_concat_ids: tp.List[str] = [],
                 prepend_cond_ids: tp.List[str] = []):
        super().__init__()
        self.model = model
        self.conditioner = conditioner
        self.io_channels = io_channels
        self.sample_rate = sample_rate
        self.diffusion_objective = diffusion_objective
        self.pretransform = pretransform
        self.cross_attn_cond_ids = cross_attn_cond_ids
        self.global_cond_ids = global_cond_ids
        self.input_concat_ids = input_concat_ids
        self.prepend_cond_ids = prepend_cond_ids
        self.min_input_length = min_input_length

    def get_conditioning_inputs(self, conditioning_tensors: tp.Dict[str, tp.Any], negative=False):
        """Assemble the denoiser's keyword arguments from the per-id ``(tensor, mask)`` pairs (counterpart of the reference's
        models/diffusion.py:123-203; host-side concatenation only): cross-attention ids are joined along the token axis
        (per-item vectors [B, C] count as one token), global ids along the channel axis (a singleton token axis is dropped),
        input-concat ids along channels, prepend ids along tokens."""

        def pairs(ids):
            return [conditioning_tensors[i] for i in ids]

        def as_tokens(tensor, mask):
            return (tensor[:, None], mask[:, None]) if tensor.dim() == 2 else (tensor, mask)

        cross = cross_mask = global_cond = concat = prepend = prepend_mask = None
        if self.cross_attn_cond_ids:
            tokens = [as_tokens(t, m) for t, m in pairs(self.cross_attn_cond_ids)]
            cross = torch.cat([t for t, _ in tokens], dim=1)
            cross_mask = torch.cat([m for _, m in tokens], dim=1)
        if self.global_cond_ids:
            global_cond = torch.cat([t for t, _ in pairs(self.global_cond_ids)], dim=-1)
            if global_cond.dim() == 3:
                global_cond = global_cond.squeeze(1)
        if self.input_concat_ids:
            # entries may be one-element lists ([tensor], reference training/diffusion.py:754): only [0] is read (:172)
            concat = torch.cat([conditioning_tensors[i][0] for i in self.input_concat_ids], dim=1)
        if self.prepend_cond_ids:
            prepend = torch.cat([t for t, _ in pairs(self.prepend_cond_ids)], dim=1)
            prepend_mask = torch.cat([m for _, m in pairs(self.prepend_cond_ids)], dim=1)
        if negative:       # the negative set has no prepend entries in the reference either (:186-191)
            return {"negative_cross_attn_cond": cross, "negative_cross_attn_mask": cross_mask, "negative_global_cond": global_cond,
                    "negative_input_concat_cond": concat}
        return {"cross_attn_cond": cross, "cross_attn_mask": cross_mask, "global_cond": global_cond, "input_concat_cond": concat,
                "prepend_cond": prepend, "prepend_cond_mask": prepend_mask}

    def forward(self, x: torch.Tensor, t: torch.Tensor, cond: tp.Dict[str, tp.Any], **kwargs):
        return self.model(x, t, **self.get_conditioning_inputs(cond), **kwargs)

    def generate(self, *args, **kwargs):
        from ..inference.generation import generate_diffusion_cond
        return generate_diffusion_cond(self, *args, **kwargs)


def create_diffusion_cond_from_config(config: tp.Dict[str, tp.Any]):
    """``model_type`` "diffusion_cond" / "diffusion_cond_inpaint" with a DiT denoiser (counterpart of the reference's
    models/diffusion.py:585-655): denoiser, conditioner set and (optional) autoencoder pretransform from one config dict."""
    if config["model_type"] not in ("diffusion_cond", "diffusion_cond_inpaint"):
        raise NotImplementedError(f"model_type '{config['model_type']}' is outside this build's hot path")
    model_cfg = config["model"]
    diffusion_cfg = model_cfg["diffusion"]
    if diffusion_cfg["type"] != "dit":
        raise NotImplementedError(f"diffusion model type '{diffusion_cfg['type']}' is outside this build's hot path (DiT only)")
    denoiser = DiTWrapper(**diffusion_cfg["config"])
    conditioning = model_cfg.get("conditioning")
    conditioner = create_multi_conditioner_from_conditioning_config(conditioning) if conditioning else None
    pretransform = model_cfg.get("pretransform")
    if pretransform:
        pretransform = create_pretransform_from_config(pretransform, config["sample_rate"])
    # shortest input the model accepts: one latent frame (x patch size)
    min_input_length = (pretransform.downsampling_ratio if pretransform else 1) * denoiser.model.patch_size
    id_lists = {name: diffusion_cfg.get(key, []) for name, key in (("cross_attn_cond_ids", "cross_attention_cond_ids"),
                                                                    ("global_cond_ids", "global_cond_ids"),
                                                                    ("input_concat_ids", "input_concat_ids"),
                                                                    ("prepend_cond_ids", "prepend_cond_ids"))}
    return ConditionedDiffusionModelWrapper(denoiser, conditioner, io_channels=model_cfg["io_channels"], sample_rate=config["sample_rate"],
                                            min_input_length=min_input_length, pretransform=pretransform,
                                            diffusion_objective=diffusion_cfg.get("diffusion_objective", "v"), **id_lists)


_UNET_GEMM_DTYPES = {"bf16": 0, "fp16": 3, "fp32": 2}      # include/sat_hip.h: SAT_GEMM_BF16, SAT_GEMM_FP16, SAT_GEMM_FP32X


class DiffusionModelWrapper(nn.Module):
    """reference models/diffusion.py:28-52.  The reference never sets ``diffusion_objective`` although its ``generate_diffusion_uncond``
    reads it; every unconditional model it builds is trained on the v objective, which is what this attribute says."""

    def __init__(self, model, io_channels, sample_size, sample_rate, min_input_length, pretransform=None):
        super().__init__()
        self.io_channels = io_channels
        self.sample_size = sample_size
        self.sample_rate = sample_rate
        self.min_input_length = min_input_length
        self.diffusion_objective = "v"
        self.model = model
        self.pretransform = pretransform if pretransform else None

    def forward(self, x, t, **kwargs):
        return self.model(x, t, **kwargs)

    def generate(self, *args, **kwargs):
        from ..inference.generation import generate_diffusion_uncond
        return generate_diffusion_uncond(self, *args, **kwargs)


class DiffusionAttnUnet1D(nn.Module):
    """The Dance Diffusion U-Net (reference models/diffusion.py:376-479) on the HIP C ABI: the reference's constructor, module tree and
    state-dict names (``net.0.main.0.weight``, ``net.3.main.7.main.0.kernel``, ``net.3.main.2.qkv_proj.weight``, ...), one
    ``sat_unet_forward`` call per forward on a plan (csrc/unet_plan.hip) built on first use and rebuilt when a parameter changes.  There is
    no eager or CPU forward.  ``forward(x, t)`` is the reference's; ``cond=`` raises (the reference's own forward fails on a tensor there:
    ``if cond:``).  ``denoise(x, sigma, out=)`` is k-diffusion's ``VDenoiser`` around it, what ``sample_k`` drives.

    Refused with ``NotImplementedError``, each with its reason: ``use_snake``, ``learned_resample``, ``cond_dim > 0``, ``cond_noise_aug``,
    a ``kernel_size`` outside 1 / 3 / 5 / 7, a ``channels`` entry that is no multiple of 128, ``depth`` above 16, ``io_channels + 16 > 128``,
    a stride other than 2.  ``ValueError`` before anything is launched: a length that is no multiple of ``2 ** (depth - 1)`` or leaves fewer
    than 3 rows at the deepest level (the reference fails in ``F.pad`` / ``torch.cat`` there)."""

    def __init__(self, io_channels=2, depth=14, n_attn_layers=6, channels=[128, 128, 256, 256] + [512] * 10, cond_dim=0, cond_noise_aug=False,
                 kernel_size=5, learned_resample=False, strides=[2] * 13, conv_bias=True, use_snake=False):
        super().__init__()
        if use_snake:
            raise NotImplementedError("use_snake=True: Snake1d comes from the dac library, which this build does not have")
        if learned_resample:
            raise NotImplementedError("learned_resample=True: only the fixed cubic resamplers are built (Downsample1d_2 / Upsample1d_2 are not)")
        if cond_dim > 0 or cond_noise_aug:
            raise NotImplementedError(f"cond_dim={cond_dim}, cond_noise_aug={cond_noise_aug}: the conditioned U-Net is not built -- the reference's own "
                                      "forward fails on a conditioning tensor (`if cond:` on a tensor)")
        if kernel_size not in (1, 3, 5, 7):
            raise NotImplementedError(f"kernel_size={kernel_size}: the convolution kernels take 1, 3, 5 and 7")
        if depth < 2:
            raise ValueError(f"depth={depth}: the reference builds a block that reads 2 c channels behind an nn.Identity and fails in its forward")
        if depth > _hip.UNET_MAX_DEPTH:
            raise NotImplementedError(f"depth={depth}: the plan holds at most {_hip.UNET_MAX_DEPTH} levels")
        if len(channels) < depth or len(strides) < depth - 1:
            raise ValueError(f"channels / strides of {len(channels)} / {len(strides)} entries for depth {depth}: one width per level, one stride between levels")
        if any(int(c) <= 0 or int(c) % 128 for c in channels[:depth]):
            raise NotImplementedError(f"channels={list(channels[:depth])}: every width must be a multiple of 128 (the GEMM launchers take N % 128 == 0 "
                                      "and K % 64 == 0)")
        if io_channels + 16 > 128:
            raise NotImplementedError(f"io_channels={io_channels}: the input boundary kernel stages io_channels + 16 <= 128 rows")
        if any(int(s) != 2 for s in strides[:depth - 1]):
            if any(int(s) > 2 for s in strides[:depth - 1]):
                raise ValueError("Must have stride 2 without learned resampling")
            raise NotImplementedError(f"strides={list(strides[:depth - 1])}: a stride of 1 selects the learned Downsample1d_2, which is not built")
        self.cond_noise_aug = cond_noise_aug
        self.io_channels = io_channels
        self.depth, self.n_attn_layers, self.kernel_size, self.conv_bias = depth, n_attn_layers, kernel_size, bool(conv_bias)
        self.channels = [int(c) for c in channels[:depth]]
        self.timestep_embed = FourierFeatures(1, 16)
        attn_layer = depth - n_attn_layers
        conv_block = partial(ResConvBlock, kernel_size=kernel_size, conv_bias=conv_bias, use_snake=use_snake)
        block = nn.Identity()
        for i in range(depth, 0, -1):
            c = channels[i - 1]
            if i > 1:
                c_prev = channels[i - 2]
                add_attn = i >= attn_layer and n_attn_layers > 0
                attn = lambda width: SelfAttention1d(width, width // 32) if add_attn else nn.Identity()
                block = SkipBlock(
                    Downsample1d("cubic"),
                    conv_block(c_prev, c, c), attn(c),
                    conv_block(c, c, c), attn(c),
                    conv_block(c, c, c), attn(c),
                    block,
                    conv_block(c * 2 if i != depth else c, c, c), attn(c),
                    conv_block(c, c, c), attn(c),
                    conv_block(c, c, c_prev), attn(c_prev),
                    Upsample1d(kernel="cubic"))
            else:
                block = nn.Sequential(
                    conv_block(io_channels + cond_dim + 16, c, c),
                    conv_block(c, c, c),
                    conv_block(c, c, c),
                    block,
                    conv_block(c * 2, c, c),
                    conv_block(c, c, c),
                    conv_block(c, c, io_channels, is_last=True))
        self.net = block
        if not _init._SKIP:
            with torch.no_grad():
                for param in self.net.parameters():
                    param *= 0.5
        self.gemm_dtype = _config.default_gemm_dtype()
        self._plan = None
        self._plan_version = None
        self._ws = None

    # ------------------------------------------------------------------ plan
    def set_gemm_dtype(self, dtype: str):
        """Build extension: operand format of the convolutions and the attention -- "fp16" (the package default), "bf16" or "fp32" (fp32 operands:
        the verification mode).  The residual stream, the GroupNorm statistics, the softmax and the two boundary layers are fp32 in every
        format.  Parameters stay fp32 in the module; rebuilds the plan on next use."""
        if dtype not in _UNET_GEMM_DTYPES:
            raise ValueError("the U-Net kernels take 'bf16', 'fp16' or 'fp32' operands")
        if dtype != self.gemm_dtype:
            self.gemm_dtype = dtype
            self._plan_version = None
        return self

    def activation_range_report(self, enable: bool = True):
        if enable:
            raise NotImplementedError("activation_range_report has no rows for the tensors of the U-Net")
        return []

    def __del__(self):
        try:
            _hip.destroy_plan("unet", self._plan)
        except Exception:
            pass

    def check_length(self, length):
        """What the reference fails on inside its forward, as a ValueError before anything is launched or allocated."""
        unit = 2 ** (self.depth - 1)
        if length <= 0 or length % unit:
            raise ValueError(f"a length of {length} samples is no multiple of 2 ** (depth - 1) = {unit}: the reference fails in torch.cat on the way up")
        if length // unit < 3:
            raise ValueError(f"{length} samples leave {length // unit} rows at the deepest level, fewer than the 3 its reflect padding needs: the "
                             "reference fails in F.pad")

    def _ensure_plan(self):
        ver = _init.params_version(self)
        if self._plan is not None and ver == self._plan_version:
            return self._plan
        lib = _hip.lib()
        dev = next(self.parameters()).device
        if dev.type != "cuda":
            raise _hip.SatError("DiffusionAttnUnet1D must be on a HIP device (model.to('cuda')); there is no CPU path")
        for name, module in self.named_modules():
            if isinstance(module, (Downsample1d, Upsample1d)):
                module.check_kernel(f"{name}.kernel")
        _hip.destroy_plan("unet", self._plan)
        self._plan = None
        cfg = _hip.SatUnetCfg()
        cfg.io_channels, cfg.depth, cfg.n_attn_layers, cfg.kernel_size = self.io_channels, self.depth, self.n_attn_layers, self.kernel_size
        cfg.conv_bias = 1 if self.conv_bias else 0
        cfg.gemm_dtype = _UNET_GEMM_DTYPES[self.gemm_dtype]
        for i, c in enumerate(self.channels):
            cfg.channels[i] = c
        tensors = {k: v for k, v in self.state_dict().items() if not k.endswith(".kernel")}
        create = lambda: _hip.new_handle(lib.sat_unet_plan_create, ctypes.byref(cfg), ctypes.sizeof(cfg))
        self._plan, self._plan_version = _hip.build_plan("unet", create, tensors, dev), ver
        return self._plan

    def _run(self, x, t, in_scale, out=None):
        x = x.detach().float().contiguous()
        b, c, length = x.shape
        assert c == self.io_channels, f"DiffusionAttnUnet1D expects {self.io_channels} channels, got {c}"
        self.check_length(length)
        t = t.detach().to(x.device, torch.float32).reshape(-1).contiguous()
        assert t.numel() == b, f"t holds {t.numel()} timesteps for a batch of {b}"
        plan = self._ensure_plan()
        self._ws = _hip.plan_workspace("unet", plan, self._ws, x.device, b, length)
        if out is None:
            out = torch.empty_like(x)
        _hip.check(_hip.lib().sat_unet_forward(plan, _hip.ptr(x), _hip.ptr(t), float(in_scale), _hip.ptr(out), b, length, _hip.ptr(self._ws),
                                               self._ws.numel(), _hip.stream()))
        return out

    @torch.no_grad()
    def forward(self, x, t, cond=None, cond_aug_scale=None):
        if cond is not None:
            raise NotImplementedError("cond=: the conditioned U-Net is not built (the reference's own forward fails on a conditioning tensor)")
        return self._run(x, t, 1.0)

    # ------------------------------------------------------------------ the denoiser protocol of sample_k
    def prepare_generation(self, *conds, **kw_conds):
        """Nothing to prepare; any conditioning handed to an unconditional model is an error."""
        if any(c is not None for c in conds[:2] + conds[3:]) or any(v is not None for v in kw_conds.values()):
            raise NotImplementedError("DiffusionAttnUnet1D is unconditional: sample_k was handed a conditioning tensor")

    @torch.no_grad()
    def denoise(self, x, sigma, out=None, **ignored):
        """k-diffusion's VDenoiser (sigma_data = 1) around ``forward``: ``net(x * c_in, atan(sigma) * 2 / pi) * c_out + x * c_skip``.  ``c_in`` is
        applied inside the input boundary kernel (the plan's ``in_scale``), the combination is one ``sat_lincomb`` launch."""
        sigma = float(sigma)
        c_skip = 1.0 / (sigma * sigma + 1.0)
        c_out = -sigma / math.sqrt(sigma * sigma + 1.0)
        c_in = 1.0 / math.sqrt(sigma * sigma + 1.0)
        x = x.detach().float().contiguous()
        t = torch.full((x.shape[0],), math.atan(sigma) * 2.0 / math.pi, dtype=torch.float32, device=x.device)
        v = self._run(x, t, c_in)
        if out is None:
            out = torch.empty_like(x)
        _hip.check(_hip.lib().sat_lincomb(_hip.ptr(out), _hip.ptr(v), c_out, _hip.ptr(x), c_skip, None, 0.0, None, 0.0, None, 0.0, out.numel(),
                                          _hip.stream()))
        return out


def create_diffusion_uncond_from_config(config: tp.Dict[str, tp.Any]):
    """``model_type`` "diffusion_uncond" (counterpart of the reference's models/diffusion.py:552-582, which indexes ``config.get[...]`` and so
    cannot run: what it evidently intends, ``config["sample_size"]`` / ``config["sample_rate"]``, is what happens here)."""
    model_cfg = config["model"]
    model_type = model_cfg["type"]
    pretransform = model_cfg.get("pretransform", None)
    sample_size, sample_rate = config["sample_size"], config["sample_rate"]
    min_input_length = 1
    if model_type == "DAU1d":
        model = DiffusionAttnUnet1D(**model_cfg.get("config", {}))
    elif model_type == "adp_uncond_1d":
        raise NotImplementedError("diffusion_uncond type 'adp_uncond_1d': the audio-diffusion-pytorch U-Net is a third-party library this build does not have")
    elif model_type == "dit":
        raise NotImplementedError("diffusion_uncond type 'dit': the unconditional DiT wrapper is not built (use diffusion_cond with a DiT)")
    else:
        raise NotImplementedError(f"Unknown model type: {model_type}")
    if pretransform:
        pretransform = create_pretransform_from_config(pretransform, sample_rate)
        min_input_length = pretransform.downsampling_ratio
    return DiffusionModelWrapper(model, io_channels=model.io_channels, sample_size=sample_size, sample_rate=sample_rate, pretransform=pretransform,
                                 min_input_length=min_input_length)
