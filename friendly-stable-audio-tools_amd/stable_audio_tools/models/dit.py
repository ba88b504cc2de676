"""``DiffusionTransformer`` (reference ``models/dit.py:14-364``) on the HIP C ABI.

The module holds the reference's parameters (same names/shapes, so reference checkpoints
load) and owns a ``sat_dit_plan``: bf16 re-packed weights, RoPE table and the per-generation
cross-attention K/V cache.  ``forward`` keeps the reference semantics
(``x, t, cross_attn_cond, global_embed, cfg_scale, scale_phi ...`` -> model output with
batched CFG, dit.py:228-364); ``denoise`` is the fused k-diffusion ``VDenoiser`` evaluation
the sampler loop uses (one ``sat_dit_denoise_cfg`` call per step).
"""
import ctypes
import typing as tp

import torch
from torch import nn

from .. import _config, _hip
from . import _init
from .blocks import FourierFeatures
from .transformer import ContinuousTransformer


PATCH_SIZE_HINT = ("pass allow_patch_size=True to DiffusionTransformer, or write \"allow_patch_size\": true into the model config's "
                   "model.diffusion.config (generate.py --allow-patch-size does): the patchified model then runs on the HIP plan "
                   "(sat_dit_plan_set_patch)")


GEMM_DTYPES = {"bf16": 0, "fp8": 1, "fp8-all": 1, "fp32x": 2, "fp16": 3}      # sat_dit_cfg.gemm_dtype (include/sat_hip.h)
# sat_dit_cfg.fp8_families (SAT_FP8_*): "fp8" = cross to_q + FF-in + FF-out in e4m3 (the subset whose quantisation the 12-step trajectory
# tolerates: tools/fp8_budget.py), "fp8-all" = every GEMM of the blocks (round 3's mode: to_qkv and the to_out projections as well)
FP8_FAMILIES = {"fp8": 2 | 4 | 8, "fp8-all": 31}


class DiffusionTransformer(nn.Module):
    def __init__(self, io_channels: int = 32, patch_size: int = 1, embed_dim: int = 768, cond_token_dim: int = 0,
                 project_cond_tokens: bool = True, global_cond_dim: int = 0, project_global_cond: bool = True,
                 input_concat_dim: int = 0, prepend_cond_dim: int = 0, depth: int = 12, num_heads: int = 8,
                 transformer_type: str = "x-transformers", global_cond_type: str = "prepend", max_seq_len: int = 8192,
                 allow_block_options: bool = False, allow_conv_ff: bool = False, allow_patch_size: bool = False, allow_head_widths: bool = False,
                 allow_causal: bool = False, allow_natten: bool = False, allow_natten_head_widths: bool = False, **kwargs):
        """``allow_block_options``: the TransformerBlock options ``conformer``, ``remove_norms`` and ``ff_kwargs={"glu": False}`` are off the
        shipped configs' path and refused unless this is set; ``create_model_from_config`` and every other config-driven path set it.
        ``allow_conv_ff``: likewise for ``ff_kwargs={"use_conv": True}`` (``sat_dit_plan_set_ff_conv``); no path sets it by default, a config
        asks for it with ``"allow_conv_ff": true`` in ``model.diffusion.config``.
        ``allow_patch_size``: likewise for ``patch_size`` above 1 (``sat_dit_plan_set_patch``): a token is then ``patch_size`` consecutive
        latent frames, ``x`` and the output keep their ``[B, io_channels, T]`` layout and ``T`` must be a multiple of ``patch_size``; a config
        asks for it with ``"allow_patch_size": true``.
        ``allow_head_widths``: likewise for attention heads of 32 or 96 channels (``embed_dim // num_heads``; ``sat_dit_plan_create_ex``), next
        to the 64- and 128-channel ones that need no opt-in; a config asks for it with ``"allow_head_widths": true``.  Such a model runs
        with 'fp16', 'bf16' (also per block) and 'fp32x' operands; 'fp8', the block options and ``use_conv`` keep 64-channel heads.
        ``allow_causal``: likewise for ``causal=True`` (``sat_dit_plan_set_attention_options``): every self-attention is then causal over the
        sequence ``[prepend rows | global token | tokens]``, row i attends to the rows j <= i; a config asks for it with
        ``"allow_causal": true``.  Such a model has no cross-attention (``cond_token_dim=0``; the reference has no working behaviour there) and
        runs with 'fp16', 'bf16' (also per block) and 'fp32x' operands at every head width; it adds no parameter.
        ``allow_natten``: likewise for ``attn_kwargs={"natten_kernel_size": K}`` (``sat_dit_plan_set_neighborhood_attention``): row i of the
        n rows ``[prepend rows | global token | tokens]`` attends to the K rows from ``min(max(i - K // 2, 0), n - K)`` on, and the logits
        are not scaled by ``dim_heads ** -0.5`` (the reference hands q to NATTEN as it is); a config asks for it with
        ``"allow_natten": true``.  K is odd and greater than 1 and no sequence may be shorter than K (``ValueError``).  Such a model has
        64-channel heads and no cross-attention, is not causal, and runs with 'fp16', 'bf16' (also per block) and 'fp32x' operands.
        ``allow_natten_head_widths``: next to ``allow_natten`` (and to ``allow_head_widths`` for 32 / 96), the same neighbourhood at 128-,
        32- and 96-channel heads (``sat_dit_plan_set_neighborhood_attention_hdw``); a config asks for it with
        ``"allow_natten_head_widths": true``.  Such a model runs with 'fp16' and 'bf16' (also per block) operands and, at 32 and 96,
        'fp32x'; what the staged widths are refused without the window they are refused with it ('fp8', 'fp32x' at 128, the block options
        and ``use_conv``), and cross-attention and ``causal`` stay refused as at 64."""
        super().__init__()
        if transformer_type != "continuous_transformer":
            raise NotImplementedError("only transformer_type='continuous_transformer' is implemented (the shipped DiT configs)")
        if global_cond_type not in ("prepend", "adaLN"):
            raise ValueError(f"Unknown global_cond_type: {global_cond_type}")
        if patch_size < 1:
            raise ValueError(f"patch_size must be >= 1, got {patch_size}")
        if patch_size != 1 and not allow_patch_size:
            raise NotImplementedError(f"patch_size={patch_size} (patch_size>1) is behind an opt-in: {PATCH_SIZE_HINT}")
        if patch_size != 1 and (io_channels * patch_size > 512 or (io_channels + input_concat_dim) * patch_size > 1024):
            raise NotImplementedError(f"patch_size={patch_size} with io_channels {io_channels} and input_concat_dim {input_concat_dim}: the two "
                                      "boundary kernels are built for io_channels * patch_size <= 512 and (io_channels + input_concat_dim) * "
                                      "patch_size <= 1024")
        if prepend_cond_dim > 0 and global_cond_type == "adaLN":
            # the reference sets prepend_length only in the "prepend" branch (dit.py:158,185-195) and so returns P + T frames (:219)
            raise NotImplementedError("prepend_cond_dim with global_cond_type='adaLN' has no working reference behaviour (reference dit.py:158,"
                                      "185-195,219 return prepend_len + T frames); use global_cond_type='prepend'")
        if input_concat_dim < 0 or prepend_cond_dim < 0:
            raise ValueError("input_concat_dim / prepend_cond_dim must be >= 0")
        if not project_global_cond and global_cond_dim > 0:
            raise NotImplementedError("project_global_cond=False is not supported")
        self.patch_size = patch_size
        self.io_channels = io_channels
        self.embed_dim = embed_dim
        self.depth = depth
        self.num_heads = num_heads
        self.cond_token_dim = cond_token_dim
        self.global_cond_dim = global_cond_dim
        self.input_concat_dim = input_concat_dim
        self.prepend_cond_dim = prepend_cond_dim
        self.max_prepend_len = 64 if prepend_cond_dim > 0 else 0     # grows (plan rebuild) when a generation brings more tokens
        self.max_seq_len = max_seq_len
        self.allow_head_widths = bool(allow_head_widths)
        self.allow_natten_head_widths = bool(allow_natten_head_widths)
        self.transformer_type = transformer_type
        self.global_cond_type = global_cond_type

        self.timestep_features = FourierFeatures(1, 256)
        self.to_timestep_embed = nn.Sequential(_init.linear(256, embed_dim), nn.SiLU(), _init.linear(embed_dim, embed_dim))
        if cond_token_dim > 0:
            cond_embed_dim = cond_token_dim if not project_cond_tokens else embed_dim
            self.to_cond_embed = nn.Sequential(_init.linear(cond_token_dim, cond_embed_dim, bias=False), nn.SiLU(),
                                               _init.linear(cond_embed_dim, cond_embed_dim, bias=False))
        else:
            cond_embed_dim = 0
        self.cond_embed_dim = cond_embed_dim
        if global_cond_dim > 0:
            self.to_global_embed = nn.Sequential(_init.linear(global_cond_dim, embed_dim, bias=False), nn.SiLU(),
                                                 _init.linear(embed_dim, embed_dim, bias=False))
        if prepend_cond_dim > 0:      # dit.py:160-165
            self.to_prepend_embed = nn.Sequential(_init.linear(prepend_cond_dim, embed_dim, bias=False), nn.SiLU(),
                                                  _init.linear(embed_dim, embed_dim, bias=False))
        dim_in = io_channels + input_concat_dim      # dit.py:38: the input projection sees cat([x, input_concat_cond])
        # dit.py:119-120: the transformer sees tokens of patch_size frames, "b (t p) c -> b t (c p)"; the two 1x1 convs below stay per frame
        self.transformer = ContinuousTransformer(dim=embed_dim, depth=depth, dim_heads=embed_dim // num_heads,
                                                 dim_in=dim_in * patch_size, dim_out=io_channels * patch_size, cross_attend=cond_token_dim > 0,
                                                 cond_token_dim=cond_embed_dim,
                                                 global_cond_dim=embed_dim if global_cond_type == "adaLN" else None,
                                                 allow_block_options=allow_block_options, allow_conv_ff=allow_conv_ff,
                                                 allow_head_widths=allow_head_widths, allow_causal=allow_causal,
                                                 allow_natten=allow_natten, allow_natten_head_widths=allow_natten_head_widths, **kwargs)
        self.preprocess_conv = _init.conv1d(dim_in, dim_in, 1, bias=False, zero=True)
        self.postprocess_conv = _init.conv1d(io_channels, io_channels, 1, bias=False, zero=True)

        self._plan = None
        self._plan_version = None
        self._plan_options = None
        self._gen_prepend_len = 0
        self._ws = None
        self._ctx_key = None
        self._ext_key = None
        self._gen_prepend = False
        self.gemm_dtype = _config.default_gemm_dtype()
        self._block_gemm_dtypes = None      # set_block_gemm_dtypes: None = gemm_dtype in every block
        self.layernorm_fusion = True
        self.cross_attention_fusion = True
        self.tile_policy = 0
        self._range_report = False      # activation_range_report: lives here, not in the plan, so that a plan rebuild keeps it
        self._check_options(self.gemm_dtype)

    def transformer_options(self):
        """``(qk_norm, pos_emb, abs_pos_max_len, rotary)`` of ``self.transformer`` as ``sat_dit_plan_set_transformer_options`` takes them."""
        tr = self.transformer
        pos = _hip.DIT_POS_SINUSOIDAL if tr.use_sinusoidal_emb else _hip.DIT_POS_ABSOLUTE if tr.use_abs_pos_emb else _hip.DIT_POS_NONE
        return (1 if tr.qk_norm else 0, pos, tr.pos_emb.max_seq_len if tr.use_abs_pos_emb and not tr.use_sinusoidal_emb else 0,
                0 if tr.rotary_pos_emb is None else 1)

    def _check_options(self, gemm_dtype):
        if self.transformer.ff_conv_kernel > 1 and GEMM_DTYPES[gemm_dtype] == 1:
            raise NotImplementedError(f"ff_kwargs use_conv with gemm_dtype={gemm_dtype!r}: the e4m3 operands carry one scale per row or per 32 "
                                      "columns of a row, which the row-shifted reads of the convolution GEMM do not move; use gemm_dtype 'fp16', "
                                      "'bf16' or 'fp32x'")
        if self.transformer.block_options != (0, 0, 1) and GEMM_DTYPES[gemm_dtype] == 1:
            raise NotImplementedError(f"conformer / remove_norms / glu=False with gemm_dtype={gemm_dtype!r}: the e4m3 epilogues and the quantising "
                                      "LayerNorm know neither a missing norm nor the plain SiLU; use gemm_dtype 'fp16', 'bf16' or 'fp32x'")
        if self.transformer.qk_norm and GEMM_DTYPES[gemm_dtype] == 1:
            raise NotImplementedError(f"attn_kwargs qk_norm=True with gemm_dtype={gemm_dtype!r}: the e4m3 projections have no normalising epilogue; "
                                      "use gemm_dtype 'fp16', 'bf16' or 'fp32x' for a qk_norm model")
        if self.transformer.causal and GEMM_DTYPES[gemm_dtype] == 1:
            raise NotImplementedError(f"causal=True with gemm_dtype={gemm_dtype!r}: the MXFP8 output form of the attention kernels has no causal "
                                      "variant; use gemm_dtype 'fp16', 'bf16' or 'fp32x'")
        if self.transformer.natten_kernel_size and GEMM_DTYPES[gemm_dtype] == 1:
            raise NotImplementedError(f"natten_kernel_size={self.transformer.natten_kernel_size} with gemm_dtype={gemm_dtype!r}: the MXFP8 output "
                                      "form of the attention kernels has no neighbourhood variant; use gemm_dtype 'fp16', 'bf16' or 'fp32x'")
        if self.transformer.dim_heads == 128 and GEMM_DTYPES[gemm_dtype] in (1, 2):
            raise NotImplementedError(f"dim_heads=128 (embed_dim {self.embed_dim} / num_heads {self.num_heads}) with gemm_dtype={gemm_dtype!r}: the "
                                      "128-channel-head route (fp32 projection, head split, attention) is built for 'fp16' and 'bf16' operands; the "
                                      "e4m3 attention outputs and the fp32 verification kernels keep 64-channel heads")
        if self.transformer.dim_heads in (32, 96) and GEMM_DTYPES[gemm_dtype] == 1:
            raise NotImplementedError(f"dim_heads={self.transformer.dim_heads} (embed_dim {self.embed_dim} / num_heads {self.num_heads}) with "
                                      f"gemm_dtype={gemm_dtype!r}: the staged route (fp32 projection, head split, attention) runs 'fp16', 'bf16' "
                                      "and 'fp32x' operands; the e4m3 attention outputs keep 64-channel heads")

    def _check_t_len(self, t_len):
        """``T`` must hold whole patches: the reference fails inside its rearrange (dit.py:198); here before anything is launched."""
        if t_len % self.patch_size != 0:
            raise ValueError(f"latent length T = {t_len} is not a multiple of patch_size = {self.patch_size}")

    def _check_seq_len(self, t_len, prepend_len):
        """The reference's ``AbsolutePositionalEmbedding`` assertion (transformer.py:59-61), on the host before anything is launched."""
        pe = self.transformer.pos_emb
        if self.transformer.natten_kernel_size:      # what NATTEN rejects: a window that does not fit the rows the blocks see
            seq_len = prepend_len + t_len // self.patch_size + (0 if self.global_cond_type == "adaLN" else 1)
            if seq_len < self.transformer.natten_kernel_size:
                raise ValueError(f"a sequence of {seq_len} rows (prepend rows + global token + tokens) is shorter than "
                                 f"natten_kernel_size={self.transformer.natten_kernel_size}")
        if self.transformer.use_abs_pos_emb and not self.transformer.use_sinusoidal_emb:
            seq_len = prepend_len + t_len // self.patch_size + (0 if self.global_cond_type == "adaLN" else 1)
            assert seq_len <= pe.max_seq_len, \
                f"you are passing in a sequence length of {seq_len} but your absolute positional embedding has a max sequence length of {pe.max_seq_len}"

    def residual_stream_report(self, enable: bool = True):
        """Build extension (``sat_dit_debug``), for checkpoints this build was never run on.  ``residual_stream_report(True)`` switches the
        diagnostics on; every forward / ``denoise`` then leaves, per block and residual update (self-attention to_out, cross-attention to_out,
        FF-out), the statistics of the fp32 residual rows that update wrote: ``max_abs``, ``common_mode`` = max over rows of |mean| / std (the
        LayerNorm fold rounds the UN-normalised row to 16 bits: its error grows with this ratio -- ``set_layernorm_fusion(False)`` from ~8 on),
        ``saturated`` = elements beyond +-65504 (what the fp16 image clamps -- ``set_gemm_dtype("bf16")`` if not 0) and ``crest`` = max |x| / rms.
        ``residual_stream_report(False)`` returns the table of the LAST forward as a list of dicts and switches the diagnostics off."""
        import ctypes as _ct
        lib = _hip.lib()
        plan = self._ensure_plan()
        if enable:
            _hip.check(lib.sat_dit_debug(plan, 1))
            return None
        n = self.depth * 3 * 4
        buf = (_ct.c_float * n)()
        _hip.check(lib.sat_dit_debug_read(plan, buf, n, _hip.stream()))
        _hip.check(lib.sat_dit_debug(plan, 0))
        names = ("self_attn.to_out", "cross_attn.to_out", "ff.out")
        return [dict(layer=l, update=names[j], max_abs=buf[(l * 3 + j) * 4], common_mode=buf[(l * 3 + j) * 4 + 1],
                     saturated=int(buf[(l * 3 + j) * 4 + 2]), crest=buf[(l * 3 + j) * 4 + 3]) for l in range(self.depth) for j in range(3)]

    def activation_range_report(self, enable: bool = True):
        """Build extension (``sat_dit_range_report``): fp16 range use of the 16-bit buffers of the blocks, which ``residual_stream_report``
        never reads -- the GEMM operand ``A`` (LayerNorm output or, under the LayerNorm fold, the 16-bit image of the residual rows), ``q`` /
        ``k`` / ``v``, the two attention outputs, the SwiGLU hidden state and the per-generation cross K / V cache.  ``(True)`` switches it on;
        from then on ``prepare_generation`` and every forward / ``denoise`` ACCUMULATE, so a whole sampler run is covered, not its last step.
        ``(False)`` returns one dict per layer and buffer -- ``layer``, ``buffer``, ``max_abs``, ``format`` ("fp16" / "bf16": the operand format of the row's block; only on a
        model with ``set_block_gemm_dtypes`` in effect, every other model has ``gemm_dtype`` in all rows), ``over_fp16`` (fp16 block: elements that were clamped at +-65504; bf16 block: elements fp16 would clamp),
        ``nonfinite``, ``elements`` (0: this plan does not materialise the buffer),
        ``launches``, ``holds`` ("layernorm output" / "residual image" for the ``a_*`` buffers, else None) -- and switches it off.  Outputs are
        bit-identical with the report on and off.  The setting survives a plan rebuild (``set_gemm_dtype`` ...), the records collected so far
        do not.  fp16 / bf16 plans only."""
        lib = _hip.lib()
        if enable and self.transformer.ff_conv_kernel > 1:
            raise NotImplementedError("activation_range_report on a model with a convolutional feed-forward (ff_kwargs use_conv): the report has "
                                      "no rows for such a plan")
        if enable and self.transformer.block_options != (0, 0, 1):
            raise NotImplementedError("activation_range_report on a model with conformer / remove_norms / glu=False: the report has no rows for the "
                                      "16-bit buffers these options add (the conformer's three, the SiLU hidden state)")
        if enable:
            self._range_report = True
            try:
                _hip.check(lib.sat_dit_range_report(self._ensure_plan(), 1))      # (a plan built just now already has it on: no-op then)
            except BaseException:
                self._range_report = False
                raise
            return None
        plan = self._ensure_plan()
        n = self.depth * _hip.DIT_RANGE_SLOTS
        buf = (_hip.SatRangeRecord * n)()
        try:
            _hip.check(lib.sat_dit_range_report_read(plan, buf, n, ctypes.sizeof(_hip.SatRangeRecord), _hip.stream()))
        finally:
            self._range_report = False
            rc = lib.sat_dit_range_report(plan, 0)
        _hip.check(rc)
        # which a_* buffers hold the un-normalised residual image: sat_dit_plan_create's ln_fold rule and proj_kind (csrc/dit_plan.hip)
        fold = (self.layernorm_fusion and self.gemm_dtype in ("fp16", "bf16") and self.global_cond_type != "adaLN" and self.embed_dim >= 256
                and self.transformer.dim_heads == 64)
        formats = self.block_gemm_dtypes
        rows = []
        for i, r in enumerate(_hip.range_rows(buf, n)):
            layer, name = divmod(i, _hip.DIT_RANGE_SLOTS)
            name = _hip.DIT_RANGE_SLOT_NAMES[name]
            holds = None
            if name.startswith("a_"):
                own_ln = name == "a_qkv" and (layer == 0 or formats[layer] != formats[layer - 1])      # a format boundary: as block 0
                holds = "residual image" if fold and not own_ln else "layernorm output"
            rows.append(dict(layer=layer, buffer=name, holds=holds, **r))
            if self._block_gemm_dtypes is not None:
                rows[-1]["format"] = formats[layer]
        return rows

    def reset_activation_range_report(self):
        """Zeroes the records of ``activation_range_report`` and leaves it on (between two generations, say)."""
        if not self._range_report:
            raise _hip.SatError("activation_range_report is not enabled")
        _hip.check(_hip.lib().sat_dit_range_report(self._ensure_plan(), 2))

    def set_cross_attention_fusion(self, on: bool):
        """Build extension, A/B switch: the to_q projection + cross-attention core as ONE launch where it applies (one prompt; the default) or
        always as two kernels (``sat_dit_cfg.cross_attention``).  Per model; rebuilds the plan on next use."""
        if bool(on) != self.cross_attention_fusion:
            self.cross_attention_fusion = bool(on)
            self._plan_version = None
        return self

    def set_tile_policy(self, policy: int):
        """Build extension, A/B measurement switch (``sat_dit_cfg.tile_policy``): 0 / 80 the measured tile choice, 22 the 16-wave 256 x 256 tile
        of rounds 1-2, 81 the 8-phase kernel for every fp32-output GEMM, 82 no two-K-group 128 x 128 tile.  Per model; rebuilds the plan."""
        if policy not in (0, 22, 80, 81, 82):
            raise ValueError("tile_policy must be 0, 22, 80, 81 or 82")
        if policy != self.tile_policy:
            self.tile_policy = policy
            self._plan_version = None
        return self

    def set_layernorm_fusion(self, on: bool):
        """Build extension: run the LayerNorms of the blocks (transformer.py:692-700) inside the epilogues of the GEMMs either side of
        them (``sat_dit_cfg.ln_fold``; bf16 / "prepend" models) or as standalone kernels.  Rebuilds the plan on next use.  Accepted
        without effect by an adaLN model and by one with 128-, 32- or 96-channel heads (as ``set_cross_attention_fusion``): their plans keep the
        standalone kernels."""
        if bool(on) != self.layernorm_fusion:
            self.layernorm_fusion = bool(on)
            self._plan_version = None
        return self

    def set_gemm_dtype(self, dtype: str):
        """Build extension: operand format of the block GEMMs and attention kernels (accumulation is fp32 in all of them).
        "fp16" (the package default, stable_audio_tools/_config.py) -- IEEE fp16 operands on the fp16 build of the kernels: the same MFMA rate on gfx950, three more
        significand bits, and the arithmetic the reference itself uses on a GPU (``torch.cuda.amp.autocast`` in
        ``inference/sampling.py:210``, fp16 flash attention in ``models/transformer.py:496-504``); conversions saturate at +-65504;
        "bf16" -- the bf16 build: 3-4 % faster, 8x the operand rounding error;
        "fp8" (BASELINE config 5: OCP e4m3 / MXFP8 operands for cross to_q, FF-in and FF-out -- 56 % of the block's FLOPs, the families
        whose quantisation the sampler trajectory tolerates; the rest bf16), "fp8-all" (every GEMM of the blocks in e4m3: round 3's mode,
        3e-1 off after 12 steps -- the to_out projections on MXFP8 attention outputs are what breaks it); "fp32x" -- the fp32 verification mode (exact fp32
        MFMA, fp32 q / k / v / P; ~20x slower): the same plan and data flow with no operand rounding.  Rebuilds the plan on next use."""
        if dtype not in GEMM_DTYPES:
            raise ValueError(f"gemm_dtype must be one of {sorted(GEMM_DTYPES)}")
        self._check_options(dtype)
        if dtype != self.gemm_dtype or self._block_gemm_dtypes is not None:
            self.gemm_dtype = dtype
            self._block_gemm_dtypes = None
            self._plan_version = None
        return self

    def set_block_gemm_dtypes(self, formats):
        """Build extension (``sat_dit_plan_set_block_formats``): the operand format per block, a list of ``depth`` names "fp16" / "bf16", or
        ``None`` for ``gemm_dtype`` in every block again.  For a checkpoint where a few blocks leave the fp16 range
        (``inference.preflight.choose_block_formats`` names them): those run in bf16, every other block keeps fp16's 8x finer operand rounding.
        The residual stream between blocks is fp32; under the LayerNorm fusion a block behind a format change runs its first LayerNorm as the
        standalone kernel (one more launch per change).  ``gemm_dtype`` must be "fp16" or "bf16"; a later ``set_gemm_dtype`` clears the list.
        Rebuilds the plan on next use."""
        if formats is not None:
            if GEMM_DTYPES[self.gemm_dtype] not in (0, 3):
                raise NotImplementedError(f"per-block operand formats with gemm_dtype={self.gemm_dtype!r}: the e4m3 modes choose their formats per GEMM "
                                          "family and the fp32 verification mode has no 16-bit operand; set_gemm_dtype('fp16') or 'bf16' first")
            formats = list(formats)
            if len(formats) != self.depth:
                raise ValueError(f"set_block_gemm_dtypes: {len(formats)} formats for a model of depth {self.depth}")
            for f in formats:
                if f not in ("fp16", "bf16"):
                    raise ValueError(f"set_block_gemm_dtypes: every format must be 'fp16' or 'bf16', got {f!r}")
        if formats != self._block_gemm_dtypes:
            self._block_gemm_dtypes = formats
            self._plan_version = None
        return self

    @property
    def block_gemm_dtypes(self):
        """The operand format every block runs in, a list of ``depth`` names: what ``set_block_gemm_dtypes`` set, else ``gemm_dtype``."""
        return list(self._block_gemm_dtypes) if self._block_gemm_dtypes is not None else [self.gemm_dtype] * self.depth

    # ------------------------------------------------------------------ plan management
    def __del__(self):
        try:
            _hip.destroy_plan("dit", self._plan)
        except Exception:
            pass

    def _plan_device(self):
        dev = self.timestep_features.weight.device
        if dev.type != "cuda":
            raise _hip.SatError("DiffusionTransformer must be on a HIP device (model.to('cuda')); there is no CPU path")
        return dev

    def _ensure_plan(self):
        ver = _init.params_version(self)
        options = (self.transformer_options() + self.transformer.block_options
                   + (self.transformer.ff_conv_kernel, self.patch_size, 1 if self.transformer.causal else 0, self.transformer.natten_kernel_size))
        if self._plan is not None and ver == self._plan_version and options == self._plan_options:
            return self._plan
        self._check_options(self.gemm_dtype)
        lib = _hip.lib()
        dev = self._plan_device()
        _hip.destroy_plan("dit", self._plan)
        self._plan = None
        cfg = _hip.SatDitCfg(self.io_channels, self.embed_dim, self.depth, self.num_heads, self.cond_token_dim,
                             self.cond_embed_dim, self.global_cond_dim, self.max_seq_len,
                             1 if self.global_cond_type == "adaLN" else 0, GEMM_DTYPES[self.gemm_dtype], FP8_FAMILIES.get(self.gemm_dtype, 0),
                             1 if self.layernorm_fusion else 0, 0 if self.cross_attention_fusion else 1, self.tile_policy)

        def configure(plan):
            if self.input_concat_dim > 0 or self.prepend_cond_dim > 0:
                _hip.check(lib.sat_dit_plan_set_extra_conditioning(plan, self.input_concat_dim, self.prepend_cond_dim, self.max_prepend_len))
            if options[:4] != (0, _hip.DIT_POS_NONE, 0, 1):       # a model with none of these switches never makes the call
                opts = _hip.SatDitTransformerOptions(*options[:4])
                _hip.check(lib.sat_dit_plan_set_transformer_options(plan, ctypes.byref(opts), ctypes.sizeof(opts)))
            if options[4:7] != (0, 0, 1):       # conformer / remove_norms / glu=False; likewise
                bopts = _hip.SatDitBlockOptions(*options[4:7])
                _hip.check(lib.sat_dit_plan_set_block_options(plan, ctypes.byref(bopts), ctypes.sizeof(bopts)))
            if options[7] > 1:       # ff_kwargs use_conv; likewise
                copts = _hip.SatDitFfConvOptions(options[7])
                _hip.check(lib.sat_dit_plan_set_ff_conv(plan, ctypes.byref(copts), ctypes.sizeof(copts)))
            if options[8] > 1:       # patch_size; likewise
                popts = _hip.SatDitPatchOptions(options[8])
                _hip.check(lib.sat_dit_plan_set_patch(plan, ctypes.byref(popts), ctypes.sizeof(popts)))
            if options[9]:       # causal; likewise
                aopts = _hip.SatDitAttentionOptions(1)
                _hip.check(lib.sat_dit_plan_set_attention_options(plan, ctypes.byref(aopts), ctypes.sizeof(aopts)))
            if options[10]:       # natten_kernel_size; likewise
                nopts = _hip.SatDitNeighborhoodOptions(options[10])
                # only a model that opted in and has staged heads calls the entry that takes them
                hdw = self.allow_natten_head_widths and self.transformer.dim_heads != 64
                setter = lib.sat_dit_plan_set_neighborhood_attention_hdw if hdw else lib.sat_dit_plan_set_neighborhood_attention
                _hip.check(setter(plan, ctypes.byref(nopts), ctypes.sizeof(nopts)))
            if self._block_gemm_dtypes is not None:       # a model that never set them never makes the call
                fm = (ctypes.c_int32 * self.depth)(*[GEMM_DTYPES[f] for f in self._block_gemm_dtypes])
                _hip.check(lib.sat_dit_plan_set_block_formats(plan, fm, self.depth))
            if self._range_report:        # the report belongs to the module: a rebuilt plan starts with it on (and with empty records)
                _hip.check(lib.sat_dit_range_report(plan, 1))

        if self.allow_head_widths and self.transformer.dim_heads in (32, 96):       # only a model that opted in and needs it makes this call
            copt = _hip.SatDitCreateOptions(1)
            create = lambda: _hip.new_handle(lib.sat_dit_plan_create_ex, ctypes.byref(cfg), ctypes.sizeof(cfg), ctypes.byref(copt), ctypes.sizeof(copt))
        else:
            create = lambda: _hip.new_handle(lib.sat_dit_plan_create_sized, ctypes.byref(cfg), ctypes.sizeof(cfg))
        plan = self._plan = _hip.build_plan("dit", create, self.state_dict(), dev, configure)
        self._plan_version = ver
        self._plan_options = options
        self._ctx_key = None
        self._ext_key = None
        return plan

    def _workspace(self, bf, t_len):
        self._ws = _hip.plan_workspace("dit", self._plan, self._ws, self.timestep_features.weight.device, bf, t_len)
        return self._ws

    def prepare_context(self, cross_attn_cond, global_embed, null_from=-1):
        """Per-generation constants (cond/global MLPs + per-layer cross K/V).  ``cross_attn_cond``
        [bf, Lc, cond_token_dim] and ``global_embed`` [bf, global_cond_dim] already hold the
        CFG-doubled batch (cond half first, null/negative half second).  ``null_from``: index of the
        first sequence whose context is the all-zero null embed (its cross-attention is exactly 0)."""
        plan = self._ensure_plan()
        key = tuple((t.data_ptr(), t._version, tuple(t.shape)) if t is not None else None for t in (cross_attn_cond, global_embed))
        key = key + (null_from,)
        if key == self._ctx_key:
            return
        self._ext_key = None          # sat_dit_prepare_context discards the extra conditioning of the previous generation
        c = None if cross_attn_cond is None else cross_attn_cond.detach().float().contiguous()
        g = None if global_embed is None else global_embed.detach().float().contiguous()
        bf = c.shape[0] if c is not None else (g.shape[0] if g is not None else 0)
        lc = c.shape[1] if c is not None else 0
        if c is not None and c.shape[2] != self.cond_token_dim:
            raise ValueError(f"cross_attn_cond has {c.shape[2]} channels, model expects {self.cond_token_dim}")
        _hip.check(_hip.lib().sat_dit_prepare_context(plan, _hip.ptr(c), bf, lc, _hip.ptr(g), _hip.stream()))
        if null_from >= 0 and c is not None:
            _hip.check(_hip.lib().sat_dit_set_null_context_from(plan, int(null_from)))
        self._ctx_key = key
        self._ctx_nseq = bf
        self._ctx_keep = (cross_attn_cond, global_embed)

    def prepare_context_bf(self, bf):
        """Context for a model without cross-attention / global conditioning."""
        plan = self._ensure_plan()
        _hip.check(_hip.lib().sat_dit_prepare_context(plan, None, bf, 0, None, _hip.stream()))
        self._ctx_key = ("bf", bf)
        self._ctx_nseq = bf
        self._ext_key = None

    def _reserve_prepend(self, prepend_cond):
        """Grow the plan's max_prepend_len (a plan rebuild) when ``prepend_cond`` brings more tokens than it was built for."""
        if prepend_cond is None:
            return
        if self.prepend_cond_dim == 0:
            raise ValueError("prepend_cond given to a DiT without prepend_cond_dim")
        if prepend_cond.shape[-1] != self.prepend_cond_dim:
            raise ValueError(f"prepend_cond has {prepend_cond.shape[-1]} channels, model expects {self.prepend_cond_dim}")
        if prepend_cond.shape[1] > self.max_prepend_len:
            self.max_prepend_len = -(-prepend_cond.shape[1] // 64) * 64
            self._plan_version = None

    def prepare_extra(self, input_concat_cond, prepend_cond, bf):
        """Per-generation input-concat signal [bf, input_concat_dim, Tc] and prepend tokens [bf, P, prepend_cond_dim] (dit.py:160-173),
        both already CFG-doubled; after ``prepare_context`` for the same ``bf``."""
        if input_concat_cond is None and prepend_cond is None:
            if self.input_concat_dim > 0:
                raise ValueError(f"this DiT has input_concat_dim {self.input_concat_dim}: input_concat_cond is required")
            if self.prepend_cond_dim == 0:
                return
        # (the absence of prepend tokens is part of the key: a cached context must not keep those of an earlier call)
        key = tuple((t.data_ptr(), t._version, tuple(t.shape)) if t is not None else None for t in (input_concat_cond, prepend_cond)) + (bf,)
        if key == self._ext_key:
            return
        c = None if input_concat_cond is None else input_concat_cond.detach().float().contiguous()
        pc = None if prepend_cond is None else prepend_cond.detach().float().contiguous()
        if c is not None and (c.dim() != 3 or c.shape[0] != bf or c.shape[1] != self.input_concat_dim):
            raise ValueError(f"input_concat_cond of shape {tuple(c.shape)}, model expects [{bf}, {self.input_concat_dim}, T]")
        if pc is not None and (pc.dim() != 3 or pc.shape[0] != bf):
            raise ValueError(f"prepend_cond of shape {tuple(pc.shape)}, model expects [{bf}, P, {self.prepend_cond_dim}]")
        _hip.check(_hip.lib().sat_dit_prepare_extra_conditioning(self._plan, _hip.ptr(c), 0 if c is None else c.shape[2], _hip.ptr(pc),
                                                                   0 if pc is None else pc.shape[1], bf, _hip.stream()))
        self._ext_key = key
        self._ext_keep = (input_concat_cond, prepend_cond, c, pc)

    # ------------------------------------------------------------------ reference-semantics forward
    @torch.no_grad()
    def _forward(self, x, t, cross_attn_cond=None, global_embed=None, null_from=-1, input_concat_cond=None, prepend_cond=None, **ignored):
        """dit.py:135-226 on the given batch (no CFG logic)."""
        self._check_t_len(x.shape[2])
        self._check_seq_len(x.shape[2], 0 if prepend_cond is None else prepend_cond.shape[1])      # (host only: before the plan is built)
        self._reserve_prepend(prepend_cond)
        self._ensure_plan()
        x = x.detach().float().contiguous()
        t = t.detach().float().contiguous()
        bf, _, t_len = x.shape
        if cross_attn_cond is None and global_embed is None:
            self.prepare_context_bf(bf)
        else:
            self.prepare_context(cross_attn_cond, global_embed, null_from)
        self.prepare_extra(input_concat_cond, prepend_cond, bf)
        ws = self._workspace(bf, t_len)
        out = torch.empty_like(x)
        _hip.check(_hip.lib().sat_dit_forward(self._plan, _hip.ptr(x), _hip.ptr(t), _hip.ptr(out), bf, t_len, _hip.ptr(ws),
                                              ws.numel(), _hip.stream()))
        return out

    @torch.no_grad()
    def forward(self, x, t, cross_attn_cond=None, cross_attn_cond_mask=None, negative_cross_attn_cond=None,
                negative_cross_attn_mask=None, input_concat_cond=None, global_embed=None, prepend_cond=None,
                prepend_cond_mask=None, cfg_scale=1.0, cfg_dropout_prob=0.0, causal=False, scale_phi=0.0, mask=None,
                return_info=False, **kwargs):
        assert not causal, "Causal mode is not supported for DiffusionTransformer"
        if return_info:
            raise NotImplementedError("return_info is outside the supported hot path")
        self._check_t_len(x.shape[2])
        # masks are discarded exactly as the reference does at inference (dit.py:250-252); prepend_cond_mask never reaches
        # the layers there either (transformer.py:787-802)
        if cfg_scale != 1.0 and (cross_attn_cond is not None or prepend_cond is not None):
            b = x.shape[0]
            bc, bg, bcat, bpre = self._cfg_batch(cross_attn_cond, global_embed, negative_cross_attn_cond, negative_cross_attn_mask,
                                                 input_concat_cond, prepend_cond)
            out = self._forward(torch.cat([x, x], dim=0), torch.cat([t, t], dim=0), bc, bg,
                                null_from=b if (cross_attn_cond is not None and negative_cross_attn_cond is None) else -1,
                                input_concat_cond=bcat, prepend_cond=bpre)
            res = torch.empty_like(out[:b])
            # CFG combine (+ optional std rescale), dit.py:336-345, as a HIP kernel: denoise form with c_out=1, c_skip=0
            _hip.check(_hip.lib().sat_cfg_combine(_hip.ptr(out), _hip.ptr(res), b, out.shape[1], out.shape[2], float(cfg_scale),
                                                  float(scale_phi), _hip.stream()))
            return res
        return self._forward(x, t, cross_attn_cond, global_embed, input_concat_cond=input_concat_cond, prepend_cond=prepend_cond)

    @staticmethod
    def _cfg_batch(cross_attn_cond, global_embed, negative_cross_attn_cond=None, negative_cross_attn_mask=None, input_concat_cond=None,
                   prepend_cond=None):
        """cat([cond, null]) / cat([global, global]) / cat([concat, concat]) / cat([prepend, 0]) (dit.py:273-315)."""
        bc = None
        if cross_attn_cond is not None:
            null = torch.zeros_like(cross_attn_cond)
            if negative_cross_attn_cond is not None:
                if negative_cross_attn_mask is not None:
                    m = negative_cross_attn_mask.to(torch.bool).unsqueeze(2)
                    negative_cross_attn_cond = torch.where(m, negative_cross_attn_cond, null)
                null = negative_cross_attn_cond
            bc = torch.cat([cross_attn_cond, null], dim=0)
        bg = None if global_embed is None else torch.cat([global_embed, global_embed], dim=0)
        bcat = None if input_concat_cond is None else torch.cat([input_concat_cond, input_concat_cond], dim=0)
        bpre = None if prepend_cond is None else torch.cat([prepend_cond, torch.zeros_like(prepend_cond)], dim=0)
        return bc, bg, bcat, bpre

    # ------------------------------------------------------------------ fused sampler-step path
    @torch.no_grad()
    def prepare_generation(self, cross_attn_cond, global_embed, cfg_scale, negative_cross_attn_cond=None,
                           negative_cross_attn_mask=None, input_concat_cond=None, prepend_cond=None):
        """Once per ``generate_diffusion_cond`` call: everything that is constant over the steps."""
        self._reserve_prepend(prepend_cond)
        self._ensure_plan()
        use_cfg = cfg_scale != 1.0 and (cross_attn_cond is not None or prepend_cond is not None)
        if use_cfg:
            bc, bg, bcat, bpre = self._cfg_batch(cross_attn_cond, global_embed, negative_cross_attn_cond, negative_cross_attn_mask,
                                                 input_concat_cond, prepend_cond)
        else:
            bc, bg, bcat, bpre = cross_attn_cond, global_embed, input_concat_cond, prepend_cond
        if bc is None and bg is None and bcat is None and bpre is None:
            raise ValueError("prepare_generation needs conditioning tensors")
        if bc is None and bg is None:
            self.prepare_context_bf((bcat if bcat is not None else bpre).shape[0])
        else:
            null_from = cross_attn_cond.shape[0] if (use_cfg and cross_attn_cond is not None and negative_cross_attn_cond is None) else -1
            self.prepare_context(bc, bg, null_from)
        self.prepare_extra(bcat, bpre, self._ctx_nseq)
        self._gen_prepend = prepend_cond is not None
        self._gen_prepend_len = 0 if prepend_cond is None else prepend_cond.shape[1]

    @torch.no_grad()
    def denoise(self, x, sigma: float, cfg_scale: float = 1.0, scale_phi: float = 0.0, out=None):
        """k-diffusion VDenoiser(DiT with batched CFG)(x, sigma) -- ``sat_dit_denoise_cfg``."""
        b, _, t_len = x.shape
        self._check_t_len(t_len)
        self._check_seq_len(t_len, self._gen_prepend_len)
        use_cfg = cfg_scale != 1.0 and (self.cond_token_dim > 0 or self._gen_prepend)
        ws = self._workspace(2 * b if use_cfg else b, t_len)
        if out is None:
            out = torch.empty_like(x)
        _hip.check(_hip.lib().sat_dit_denoise_cfg(self._plan, _hip.ptr(x), float(sigma), float(cfg_scale), float(scale_phi),
                                                  _hip.ptr(out), b, t_len, _hip.ptr(ws), ws.numel(), _hip.stream()))
        return out
