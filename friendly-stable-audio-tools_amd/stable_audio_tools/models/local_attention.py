"""The local-attention transformer codec (``"type": "local_attn"``) on the HIP C ABI.

Module tree and state-dict keys follow the reference's ``models/local_attention.py`` (``ContinuousLocalTransformer`` :17-103,
``TransformerDownsampleBlock1D`` :106-146, ``TransformerUpsampleBlock1D`` :149-190, ``TransformerEncoder1D`` :193-236,
``TransformerDecoder1D`` :239-282), so a reference checkpoint loads with ``strict=True``.  The classes hold parameters (fp32); a whole
encoder or decoder forward is one ``sat_local_attn_forward`` call on a plan of its own (csrc/local_attn_plan.hip), built lazily and
rebuilt when a parameter changes.  There is no eager or CPU forward.

What runs: LayerNorm'd blocks of NATTEN's 1-D neighbourhood attention (``local_attn_window_size`` keys, unscaled logits, rotary embedding
of ``max(dim_head // 2, 32)`` channels) and a bias-free SwiGLU feed-forward, at 32-, 64-, 96- or 128-channel heads.  What is refused, each
with its reason: an even window or one of 1 or less (``ValueError``, NATTEN's rule -- the reference's default of 64 is such a value);
``cond_dim`` / ``cross_attn_cond_dim`` / ``causal`` / ``dim_in`` / ``dim_out`` (``NotImplementedError``: the AdaRMSNorm, cross-attending,
causal and biased-projection variants, which neither codec class reaches except through ``**kwargs``); other head widths; an ``embed_dim``
that is no multiple of 128 or an ``int(embed_dim * ff_mult)`` that is no multiple of 64 (the GEMM launchers take N % 128 == 0 and
K % 64 == 0).  Other keyword arguments are ignored, as the reference's ``ContinuousLocalTransformer`` ignores them.
"""
import ctypes
import math

import torch
from torch import nn

from .. import _config, _hip
from . import _init
from .transformer import Attention, FeedForward, LayerNorm, RotaryEmbedding

HEAD_WIDTHS = (32, 64, 96, 128)
_GEMM_DTYPES = {"bf16": 0, "fp16": 3, "fp32": 2}      # include/sat_hip.h: SAT_GEMM_BF16, SAT_GEMM_FP16, SAT_GEMM_FP32X


def check_window(local_attn_window_size):
    k = local_attn_window_size
    if not isinstance(k, int) or isinstance(k, bool) or k <= 1 or k % 2 == 0:
        raise ValueError(f"local_attn_window_size={k!r}: NATTEN takes odd kernel sizes greater than 1 (the reference's default of 64 fails inside "
                         "its first forward)")
    return k


def _no_standalone_forward(module):
    raise RuntimeError(f"{type(module).__name__} has no standalone forward in this build: the stack runs inside TransformerEncoder1D / "
                       "TransformerDecoder1D (one sat_local_attn_forward call); there is no CPU/eager path")


class ContinuousLocalTransformer(nn.Module):
    def __init__(self, *, dim, depth, dim_in=None, dim_out=None, causal=False, local_attn_window_size=64, heads=8, ff_mult=2, cond_dim=0,
                 cross_attn_cond_dim=0, **kwargs):
        super().__init__()
        self.local_attn_window_size = check_window(local_attn_window_size)
        if cond_dim > 0:
            raise NotImplementedError(f"cond_dim={cond_dim}: the AdaRMSNorm-conditioned ContinuousLocalTransformer is not built (neither codec class "
                                      "passes a condition to it)")
        if cross_attn_cond_dim > 0:
            raise NotImplementedError(f"cross_attn_cond_dim={cross_attn_cond_dim}: the cross-attending ContinuousLocalTransformer is not built "
                                      "(neither codec class passes a context to it)")
        if causal:
            raise NotImplementedError("causal=True: the reference's NATTEN branch ignores causal (transformer.py:479-493); the HIP codec does not "
                                      "take the flag")
        if dim_in is not None or dim_out is not None:
            raise NotImplementedError("dim_in / dim_out: the biased projections of a standalone ContinuousLocalTransformer are not built (the codec "
                                      "classes build it without them)")
        dim_head = dim // heads
        if dim_head not in HEAD_WIDTHS or dim_head * heads != dim:
            raise NotImplementedError(f"embed_dim {dim} // heads {heads} = {dim_head}: the neighbourhood attention kernels are built for heads of "
                                      "32, 64, 96 and 128 channels")
        inner = int(dim * ff_mult)
        if dim % 128 or inner <= 0 or inner % 64:
            raise NotImplementedError(f"embed_dim {dim}, int(embed_dim * ff_mult) = {inner}: the GEMM launchers take output widths that are multiples "
                                      "of 128 and contraction lengths that are multiples of 64, hence an embed_dim that is a multiple of 128 and an "
                                      "int(embed_dim * ff_mult) that is a multiple of 64")
        self.dim, self.depth, self.heads, self.dim_head, self.ff_inner = dim, depth, heads, dim_head, inner
        self.cond_dim, self.cross_attn_cond_dim = cond_dim, cross_attn_cond_dim
        self.layers = nn.ModuleList([])
        self.project_in = nn.Identity()
        self.project_out = nn.Identity()
        self.rotary_pos_emb = RotaryEmbedding(max(dim_head // 2, 32))
        for _ in range(depth):
            self.layers.append(nn.ModuleList([
                LayerNorm(dim),
                Attention(dim=dim, dim_heads=dim_head, zero_init_output=True, natten_kernel_size=self.local_attn_window_size, allow_natten=True,
                          allow_natten_head_widths=True, allow_head_widths=True),
                nn.Identity(),
                LayerNorm(dim),
                FeedForward(dim=dim, mult=ff_mult, no_bias=True)]))

    def forward(self, *args, **kwargs):
        _no_standalone_forward(self)


class TransformerDownsampleBlock1D(nn.Module):
    def __init__(self, in_channels, embed_dim=768, depth=3, heads=12, downsample_ratio=2, local_attn_window_size=64, **kwargs):
        super().__init__()
        self.downsample_ratio = downsample_ratio
        self.transformer = ContinuousLocalTransformer(dim=embed_dim, depth=depth, heads=heads, local_attn_window_size=local_attn_window_size, **kwargs)
        self.project_in = _init.linear(in_channels, embed_dim, bias=False) if in_channels != embed_dim else nn.Identity()
        self.project_down = _init.linear(embed_dim * self.downsample_ratio, embed_dim, bias=False)

    def forward(self, *args, **kwargs):
        _no_standalone_forward(self)


class TransformerUpsampleBlock1D(nn.Module):
    def __init__(self, in_channels, embed_dim, depth=3, heads=12, upsample_ratio=2, local_attn_window_size=64, **kwargs):
        super().__init__()
        self.upsample_ratio = upsample_ratio
        self.transformer = ContinuousLocalTransformer(dim=embed_dim, depth=depth, heads=heads, local_attn_window_size=local_attn_window_size, **kwargs)
        self.project_in = _init.linear(in_channels, embed_dim, bias=False) if in_channels != embed_dim else nn.Identity()
        self.project_up = _init.linear(embed_dim, embed_dim * self.upsample_ratio, bias=False)

    def forward(self, *args, **kwargs):
        _no_standalone_forward(self)


def permute_project_down(weight, ratio):
    """``project_down.weight`` [D, D * r] as the plan's finalize re-orders it: ``W'[:, j * D + c] = W[:, c * r + j]``.  ``r`` consecutive rows of
    the [M, D] stream are one row of [M / r, r * D] with feature index ``j * D + c``, so ``rearrange("b (n r) c -> b n (c r)")`` followed by
    the Linear is one GEMM on those rows with this weight, and no data moves (tests/test_local_attn_host.py)."""
    d = weight.shape[0]
    return weight.reshape(d, d, ratio).transpose(1, 2).reshape(d, ratio * d)


def permute_project_up(weight, ratio):
    """``project_up.weight`` [D * r, D] likewise: ``W'[j * D + c, :] = W[c * r + j, :]``; the GEMM's [M, r * D] output read as [M * r, D] is the
    Linear followed by ``rearrange("b n (c r) -> b (n r) c")``."""
    d = weight.shape[1]
    return weight.reshape(d, ratio, d).transpose(0, 1).reshape(ratio * d, d)


class _LocalAttnHip(nn.Module):
    """Shared plan handling of encoder and decoder."""
    _is_decoder = False

    def _build(self, block, ratio_name, in_channels, out_channels, embed_dims, heads, depths, ratios, local_attn_window_size, kwargs):
        n = len(depths)
        if not (len(embed_dims) >= n and len(heads) >= n and len(ratios) >= n and 1 <= n <= _hip.LOCAL_ATTN_MAX_STAGES):
            raise ValueError(f"embed_dims / heads / depths / ratios of {len(embed_dims)} / {len(heads)} / {len(depths)} / {len(ratios)} entries: one "
                             f"per stage, at most {_hip.LOCAL_ATTN_MAX_STAGES} stages")
        check_window(local_attn_window_size)
        if any(int(r) < 1 for r in ratios[:n]):
            raise ValueError(f"ratios {list(ratios)}: every ratio is at least 1")
        if in_channels > 128:
            raise NotImplementedError(f"in_channels {in_channels}: the boundary kernel stages a tile of the input in LDS and takes in_channels <= 128")
        self.io = (in_channels, out_channels)
        self.embed_dims, self.heads, self.depths, self.ratios = (list(v[:n]) for v in (embed_dims, heads, depths, ratios))
        self.local_attn_window_size = local_attn_window_size
        self.ratio = int(math.prod(self.ratios))
        layers = []
        for i in range(n):
            prev_dim = embed_dims[i - 1] if i > 0 else embed_dims[0]
            layers.append(block(in_channels=prev_dim, embed_dim=embed_dims[i], heads=heads[i], depth=depths[i],
                                local_attn_window_size=local_attn_window_size, **{ratio_name: ratios[i]}, **kwargs))
        self.layers = nn.Sequential(*layers)
        self.project_in = _init.linear(in_channels, embed_dims[0], bias=False)
        self.project_out = _init.linear(self.embed_dims[-1], out_channels, bias=False)
        self.gemm_dtype = _config.default_gemm_dtype()
        self._plan = None
        self._plan_version = None
        self._ws = None

    def stage_rows(self, length):
        """Rows per batch item at which each stage's layers run for an input of ``length`` time steps."""
        rows, s = [], length
        for r in self.ratios:
            if self._is_decoder:
                s *= r
            rows.append(s)
            if not self._is_decoder:
                s //= r
        return rows

    def check_length(self, length):
        """What the reference fails on inside its forward (einops on a length that does not divide, NATTEN on a sequence shorter than its
        kernel), as ValueErrors before anything is launched or allocated."""
        if not self._is_decoder and length % self.ratio:
            raise ValueError(f"an input of {length} samples is no multiple of the product of the ratios {self.ratios}, {self.ratio}")
        for i, s in enumerate(self.stage_rows(length)):
            if s < self.local_attn_window_size:
                raise ValueError(f"stage {i} runs at {s} rows per item, fewer than local_attn_window_size {self.local_attn_window_size}: NATTEN "
                                 "refuses a sequence shorter than its kernel")

    def set_gemm_dtype(self, dtype: str):
        """Build extension: operand format of the GEMMs and the attention inside the stages -- "fp16" (the package default), "bf16" or "fp32"
        (fp32 operands on the exact f32-input MFMA and the fp32 attention kernels; not at 128-channel heads).  The residual stream, the
        LayerNorm statistics, the softmax and the two projections at the audio boundary are fp32 in every format.  Parameters stay fp32 in
        the module; rebuilds the plan on next use."""
        if dtype not in _GEMM_DTYPES:
            raise ValueError("the codec kernels take 'bf16', 'fp16' or 'fp32' operands")
        if dtype == "fp32" and any(d // h == 128 for d, h in zip(self.embed_dims, self.heads)):
            raise NotImplementedError("set_gemm_dtype('fp32'): a stage with 128-channel heads runs with bf16 or fp16 operands only (there are no "
                                      "fp32 kernels at that width)")
        if dtype != self.gemm_dtype:
            self.gemm_dtype = dtype
            self._plan_version = None
        return self

    def activation_range_report(self, enable: bool = True):
        if enable:
            raise NotImplementedError("activation_range_report has no rows for the tensors of a local_attn codec")
        return []

    def __del__(self):
        try:
            _hip.destroy_plan("local_attn", self._plan)
        except Exception:
            pass

    def _ensure_plan(self):
        ver = _init.params_version(self)
        if self._plan is not None and ver == self._plan_version:
            return self._plan
        lib = _hip.lib()
        dev = next(self.parameters()).device
        if dev.type != "cuda":
            raise _hip.SatError("local_attn modules must be on a HIP device (model.to('cuda')); there is no CPU path")
        _hip.destroy_plan("local_attn", self._plan)
        self._plan = None
        cfg = _hip.SatLocalAttnCfg()
        cfg.is_decoder = 1 if self._is_decoder else 0
        cfg.in_channels, cfg.out_channels = self.io
        cfg.n_stages = len(self.depths)
        for i, stage in enumerate(self.layers):
            cfg.embed_dims[i], cfg.heads[i], cfg.depths[i], cfg.ratios[i] = self.embed_dims[i], self.heads[i], self.depths[i], self.ratios[i]
            cfg.ff_inner[i] = stage.transformer.ff_inner
        cfg.window = self.local_attn_window_size
        cfg.gemm_dtype = _GEMM_DTYPES[self.gemm_dtype]
        create = lambda: _hip.new_handle(lib.sat_local_attn_plan_create, ctypes.byref(cfg), ctypes.sizeof(cfg))
        self._plan, self._plan_version = _hip.build_plan("local_attn", create, self.state_dict(), dev), ver
        return self._plan

    @torch.no_grad()
    def forward(self, x):
        x = x.detach().float().contiguous()
        b, c, length = x.shape
        assert c == self.io[0], f"{type(self).__name__} expects {self.io[0]} channels, got {c}"
        self.check_length(length)
        plan = self._ensure_plan()
        self._ws = _hip.plan_workspace("local_attn", plan, self._ws, x.device, b, length)
        out_len = length * self.ratio if self._is_decoder else length // self.ratio
        out = torch.empty((b, self.io[1], out_len), device=x.device, dtype=torch.float32)
        _hip.check(_hip.lib().sat_local_attn_forward(plan, _hip.ptr(x), _hip.ptr(out), b, length, _hip.ptr(self._ws), self._ws.numel(), _hip.stream()))
        return out


class TransformerEncoder1D(_LocalAttnHip):
    def __init__(self, in_channels, out_channels, embed_dims=[96, 192, 384, 768], heads=[12, 12, 12, 12], depths=[3, 3, 3, 3], ratios=[2, 2, 2, 2],
                 local_attn_window_size=64, **kwargs):
        super().__init__()
        self._build(TransformerDownsampleBlock1D, "downsample_ratio", in_channels, out_channels, embed_dims, heads, depths, ratios,
                    local_attn_window_size, kwargs)


class TransformerDecoder1D(_LocalAttnHip):
    _is_decoder = True

    def __init__(self, in_channels, out_channels, embed_dims=[768, 384, 192, 96], heads=[12, 12, 12, 12], depths=[3, 3, 3, 3], ratios=[2, 2, 2, 2],
                 local_attn_window_size=64, **kwargs):
        super().__init__()
        self._build(TransformerUpsampleBlock1D, "upsample_ratio", in_channels, out_channels, embed_dims, heads, depths, ratios,
                    local_attn_window_size, kwargs)
