"""``ContinuousTransformer`` and its parts -- state-dict compatible parameter containers.

Mirror of the module tree of the reference's ``models/transformer.py`` (``LayerNorm`` :188-206,
``GLU``/``FeedForward`` :211-287, ``Attention`` :290-554, ``TransformerBlock`` :594-702,
``RotaryEmbedding`` :99-155, ``AbsolutePositionalEmbedding`` / ``ScaledSinusoidalEmbedding`` :50-96,
``ContinuousTransformer`` :705-809) restricted to the options the HIP plan runs: those of the shipped DiT
configs plus causal self-attention (behind ``allow_causal``), neighbourhood self-attention (``natten_kernel_size``, behind ``allow_natten``; off 64-channel heads also behind ``allow_natten_head_widths``), 128-channel heads (and, behind ``allow_head_widths``, 32- and 96-channel ones), ``qk_norm``, the sinusoidal / absolute position embeddings, ``rotary_pos_emb=False``,
bias-free / ``mult``-sized feed-forwards and, behind the ``allow_block_options`` opt-in, ``conformer`` (:557-591), ``remove_norms``
and feed-forwards without GLU, and behind ``allow_conv_ff`` convolutional feed-forwards (``ff_kwargs use_conv``).  These classes only *hold* parameters under the reference's
names; the forward pass of the whole stack is one C-ABI call (``sat_dit_forward`` /
``sat_dit_denoise_cfg``) issued by ``models/dit.py``.  Unsupported options raise.
"""
import torch
from torch import nn

from . import _init


class LayerNorm(nn.Module):
    def __init__(self, dim, bias=False, fix_scale=False):
        super().__init__()
        if fix_scale:
            self.register_buffer("gamma", torch.ones(dim))
        else:
            self.gamma = nn.Parameter(torch.ones(dim))
        if bias:
            self.beta = nn.Parameter(torch.zeros(dim))
        else:
            self.register_buffer("beta", torch.zeros(dim))


class RotaryEmbedding(nn.Module):
    def __init__(self, dim, base=10000):
        super().__init__()
        inv_freq = 1.0 / (base ** (torch.arange(0, dim, 2).float() / dim))
        self.register_buffer("inv_freq", inv_freq)


class AbsolutePositionalEmbedding(nn.Module):
    """``emb.weight[pos] * dim ** -0.5`` added to the stream (reference :50-71); the plan builds the table once."""

    def __init__(self, dim, max_seq_len):
        super().__init__()
        self.scale = dim ** -0.5
        self.max_seq_len = max_seq_len
        self.emb = nn.Embedding(max_seq_len, dim)


class ScaledSinusoidalEmbedding(nn.Module):
    """``cat(sin, cos)(pos * theta ** -(j / (dim / 2))) * scale`` (reference :74-96).  ``inv_freq`` is not persistent there, so only
    ``scale`` is in the state dict."""

    def __init__(self, dim, theta=10000):
        super().__init__()
        assert (dim % 2) == 0, "dimension must be divisible by 2"
        self.scale = nn.Parameter(torch.ones(1) * dim ** -0.5)


class GLU(nn.Module):
    def __init__(self, dim_in, dim_out):
        super().__init__()
        self.proj = _init.linear(dim_in, dim_out * 2)


BLOCK_OPTIONS_HINT = ("pass allow_block_options=True to DiffusionTransformer (create_model_from_config and every config-driven path do): "
                      "the option then runs on the HIP plan (sat_dit_plan_set_block_options)")


CONV_FF_HINT = ("pass allow_conv_ff=True to DiffusionTransformer, or write \"allow_conv_ff\": true into the model config's model.diffusion.config "
                "(generate.py --allow-conv-ff does): the convolutions then run on the HIP plan (sat_dit_plan_set_ff_conv)")


HEAD_WIDTHS_HINT = ("pass allow_head_widths=True to DiffusionTransformer, or write \"allow_head_widths\": true into the model config's "
                    "model.diffusion.config (generate.py --allow-head-widths does): 32- and 96-channel heads then run on the HIP plan "
                    "(sat_dit_plan_create_ex)")


CAUSAL_HINT = ("pass allow_causal=True to DiffusionTransformer, or write \"allow_causal\": true into the model config's model.diffusion.config "
               "(generate.py --allow-causal does): every self-attention then runs causal on the HIP plan (sat_dit_plan_set_attention_options)")


NATTEN_HINT = ("pass allow_natten=True to DiffusionTransformer, or write \"allow_natten\": true into the model config's model.diffusion.config "
               "(generate.py --allow-natten does): every self-attention then runs NATTEN's 1-D neighbourhood on the HIP plan "
               "(sat_dit_plan_set_neighborhood_attention)")


NATTEN_HEAD_WIDTHS_HINT = ("pass allow_natten_head_widths=True to DiffusionTransformer, or write \"allow_natten_head_widths\": true into the model "
                           "config's model.diffusion.config (generate.py --allow-natten-head-widths does), next to allow_natten (and to "
                           "allow_head_widths for 32 / 96): the neighbourhood then runs at 128-, 32- and 96-channel heads on the HIP plan "
                           "(sat_dit_plan_set_neighborhood_attention_hdw)")


class FeedForward(nn.Module):
    def __init__(self, dim, mult=4, glu=True, no_bias=False, use_conv=False, conv_kernel_size=3, zero_init_output=True, allow_block_options=False,
                 allow_conv_ff=False, **unsupported):
        super().__init__()
        if unsupported or (use_conv and not allow_conv_ff):
            raise NotImplementedError("FeedForward options not supported by the HIP path, with or without allow_block_options (use_conv is behind "
                                      f"an opt-in of its own: {CONV_FF_HINT}): use_conv={use_conv} {sorted(unsupported)}")
        if use_conv:
            if conv_kernel_size < 1 or conv_kernel_size % 2 == 0:
                # reference :245,285: Conv1d(padding=k // 2) returns n + 1 rows for an even k and the block's residual add does not fit
                raise ValueError(f"FeedForward conv_kernel_size={conv_kernel_size}: the reference's own forward fails for an even kernel size "
                                 "(its convolution returns one row more than it was given)")
            if conv_kernel_size > 7:
                raise NotImplementedError(f"FeedForward conv_kernel_size={conv_kernel_size}: the HIP convolution GEMM is built for kernel sizes 1, 3, 5 and 7")
        if not glu and not allow_block_options:
            raise NotImplementedError(f"FeedForward glu={glu} (use_conv={use_conv}) is off the shipped configs' path: {BLOCK_OPTIONS_HINT}")
        inner_dim = int(dim * mult)
        if inner_dim <= 0 or inner_dim % 64:
            raise NotImplementedError(f"FeedForward mult={mult}: the HIP plan needs an inner dim that is a multiple of 64, got {inner_dim}")
        if not glu and inner_dim % 128:
            raise NotImplementedError(f"FeedForward mult={mult} with glu=False: every column of the input Linear is an output of the GEMM, whose N "
                                      f"must be a multiple of 128, got inner dim {inner_dim}")
        self.no_bias, self.glu = no_bias, bool(glu)
        self.conv_kernel_size = conv_kernel_size if use_conv else 1      # 1: Linears (a use_conv model with kernel size 1 keeps Conv1d-shaped weights)
        self.use_conv = bool(use_conv)
        # reference :222,270: GLU builds its own nn.Linear and keeps the bias; no_bias only drops the one of the output projection.
        # Without GLU (:262-268) the input Linear follows no_bias as well
        # use_conv (:222,262-287): both become Conv1d(k, padding=k // 2) along the sequence under the same keys; GLU is built without use_conv
        # and keeps its Linear
        if use_conv:
            proj = lambda i, o, zero=False: _init.conv1d(i, o, conv_kernel_size, bias=not no_bias, padding=conv_kernel_size // 2, zero=zero)
        else:
            proj = lambda i, o, zero=False: _init.linear(i, o, bias=not no_bias, zero=zero)
        linear_out = proj(inner_dim, dim, zero=zero_init_output)
        linear_in = GLU(dim, inner_dim) if glu else nn.Sequential(nn.Identity(), proj(dim, inner_dim), nn.Identity(), nn.SiLU())
        self.ff = nn.Sequential(linear_in, nn.Identity(), linear_out, nn.Identity())


class Attention(nn.Module):
    def __init__(self, dim, dim_heads=64, dim_context=None, causal=False, zero_init_output=True, qk_norm=False, natten_kernel_size=None,
                 allow_head_widths=False, allow_causal=False, allow_natten=False, allow_natten_head_widths=False, **unsupported):
        super().__init__()
        if (natten_kernel_size is not None and not allow_natten) or unsupported:
            raise NotImplementedError("Attention options not supported by the HIP path (full attention, non-causal or behind allow_causal causal; "
                                      f"natten_kernel_size is behind an opt-in of its own: {NATTEN_HINT}): "
                                      f"natten_kernel_size={natten_kernel_size} {sorted(unsupported)}")
        # reference :479: the value's truth decides, None and 0 are full attention
        self.natten_kernel_size = int(natten_kernel_size) if natten_kernel_size else 0
        if self.natten_kernel_size:
            k = self.natten_kernel_size
            if k <= 1 or k % 2 == 0:
                raise ValueError(f"natten_kernel_size={k}: NATTEN takes odd kernel sizes greater than 1")
            if dim_context:
                # reference :299, 324: attn_kwargs reach cross_attn too, where q and k differ in length and natten1dqk fails
                raise NotImplementedError(f"natten_kernel_size={k} with cross-attention (cond_token_dim > 0) has no working reference behaviour "
                                          "(attn_kwargs reach cross_attn, where NATTEN fails on q and k of different lengths); use cond_token_dim=0")
            if causal:
                raise NotImplementedError(f"natten_kernel_size={k} with causal=True: the reference silently ignores causal in its NATTEN branch "
                                          "(transformer.py:479-493); drop one of the two")
            if dim_heads != 64 and not allow_natten_head_widths:
                raise NotImplementedError(f"natten_kernel_size={k} with dim_heads={dim_heads}: the neighbourhood kernels are built for 64-channel "
                                          f"heads; the staged widths (128, 32, 96) are a follow-up behind an opt-in: {NATTEN_HEAD_WIDTHS_HINT}")
        if causal and not allow_causal:
            raise NotImplementedError(f"causal={causal} is behind an opt-in: {CAUSAL_HINT}")
        if causal and dim_context:
            # reference :371, 530: more context keys than queries fail inside create_causal_mask, which Attention does not have; with fewer
            # SDPA aligns the mask top-left, flash-attn >= 2.1 bottom-right and the einsum path would give uniform rows
            raise NotImplementedError("causal=True with cross-attention (cond_token_dim > 0) has no working reference behaviour (reference "
                                      "transformer.py:371,530 fail with more context keys than queries, and its attention backends disagree with "
                                      "fewer); use cond_token_dim=0")
        self.causal = bool(causal)
        if dim_heads in (32, 96) and not allow_head_widths:
            raise NotImplementedError(f"the HIP attention kernels run dim_heads 64 and 128 (embed_dim / num_heads) by default, got dim_heads={dim_heads}: "
                                      f"{HEAD_WIDTHS_HINT}")
        if dim_heads not in (32, 64, 96, 128):
            raise NotImplementedError("the HIP attention kernels are built for dim_heads 64 and 128 (embed_dim / num_heads), and 32 and 96 behind "
                                      f"allow_head_widths, got dim_heads={dim_heads}")
        self.dim, self.dim_heads = dim, dim_heads
        self.qk_norm = bool(qk_norm)
        dim_kv = dim_context if dim_context else dim
        if dim_heads in (32, 96) and dim_kv % dim_heads:
            # the reference builds such a model (kv_heads = dim_kv // dim_heads) and fails inside its first forward, where to_kv's output does
            # not split into heads
            raise ValueError(f"Attention: the context width {dim_kv} (cond_embed_dim) is no multiple of dim_heads={dim_heads}")
        self.num_heads = dim // dim_heads
        self.kv_heads = dim_kv // dim_heads
        if dim_context:
            self.to_q = _init.linear(dim, dim, bias=False)
            self.to_kv = _init.linear(dim_kv, dim_kv * 2, bias=False)
        else:
            self.to_qkv = _init.linear(dim, dim * 3, bias=False)
        self.to_out = _init.linear(dim, dim, bias=False, zero=zero_init_output)


class ConformerModule(nn.Module):
    """Parameters of the reference's ``ConformerModule`` (:557-591): ``in_norm`` -> ``pointwise_conv`` (1 x 1) -> ``glu`` -> 17-tap
    ``depthwise_conv`` along the sequence -> ``mid_norm`` -> SiLU -> ``pointwise_conv_2``."""

    def __init__(self, dim, norm_kwargs={}):
        super().__init__()
        self.dim = dim
        self.in_norm = LayerNorm(dim, **norm_kwargs)
        self.pointwise_conv = _init.conv1d(dim, dim, 1, bias=False)
        self.glu = GLU(dim, dim)
        self.depthwise_conv = _init.conv1d(dim, dim, 17, bias=False, groups=dim, padding=8)
        self.mid_norm = LayerNorm(dim, **norm_kwargs)
        self.swish = nn.SiLU()
        self.pointwise_conv_2 = _init.conv1d(dim, dim, 1, bias=False)


class TransformerBlock(nn.Module):
    def __init__(self, dim, dim_heads=64, cross_attend=False, dim_context=None, global_cond_dim=None, causal=False,
                 zero_init_branch_outputs=True, conformer=False, layer_ix=-1, remove_norms=False, attn_kwargs={}, ff_kwargs={},
                 norm_kwargs={}, allow_block_options=False, allow_conv_ff=False, allow_head_widths=False, allow_causal=False,
                 allow_natten=False, allow_natten_head_widths=False):
        super().__init__()
        if (conformer or remove_norms) and not allow_block_options:
            raise NotImplementedError(f"conformer={conformer} / remove_norms={remove_norms} are off the shipped configs' path: {BLOCK_OPTIONS_HINT}")
        if dim_heads != 64 and (conformer or remove_norms or not ff_kwargs.get("glu", True)):
            raise NotImplementedError(f"conformer / remove_norms / glu=False with dim_heads={dim_heads}: the staged route of the 128-channel heads "
                                      "(and of the 32- / 96-channel ones) keeps the shipped block (standalone LayerNorms, SwiGLU feed-forward); these options run with dim_heads=64")
        if dim_heads != 64 and ff_kwargs.get("use_conv", False) and allow_conv_ff:
            raise NotImplementedError(f"ff_kwargs use_conv with dim_heads={dim_heads}: the staged route of the 128-channel heads (and of the 32- / 96-channel ones) "
                                      "keeps the shipped block; "
                                      "a convolutional feed-forward runs with dim_heads=64")
        self.dim, self.dim_heads, self.cross_attend, self.dim_context = dim, dim_heads, cross_attend, dim_context
        self.layer_ix = layer_ix
        self.remove_norms = bool(remove_norms)
        norm = (lambda: nn.Identity()) if remove_norms else (lambda: LayerNorm(dim, **norm_kwargs))      # reference :621,632,642
        self.pre_norm = norm()
        self.self_attn = Attention(dim, dim_heads=dim_heads, causal=causal, zero_init_output=zero_init_branch_outputs,
                                   allow_head_widths=allow_head_widths, allow_causal=allow_causal, allow_natten=allow_natten,
                                   allow_natten_head_widths=allow_natten_head_widths, **attn_kwargs)
        if cross_attend:
            self.cross_attend_norm = norm()
            self.cross_attn = Attention(dim, dim_heads=dim_heads, dim_context=dim_context, causal=causal,
                                        zero_init_output=zero_init_branch_outputs, allow_head_widths=allow_head_widths, allow_causal=allow_causal,
                                        allow_natten=allow_natten, allow_natten_head_widths=allow_natten_head_widths, **attn_kwargs)
        self.ff_norm = norm()
        self.ff = FeedForward(dim, zero_init_output=zero_init_branch_outputs, allow_block_options=allow_block_options, allow_conv_ff=allow_conv_ff,
                              **ff_kwargs)
        self.conformer = ConformerModule(dim, norm_kwargs=norm_kwargs) if conformer else None      # its two norms stay under remove_norms
        self.global_cond_dim = global_cond_dim
        if global_cond_dim:
            # adaLN (reference transformer.py:650-656): SiLU -> Linear(global_cond_dim, 6*dim, no bias), zero-initialised;
            # the HIP plan stacks the 24 weights and evaluates them in one launch per forward
            if global_cond_dim != dim:
                raise NotImplementedError("adaLN: the HIP plan expects global_cond_dim == dim (DiffusionTransformer always passes embed_dim)")
            self.to_scale_shift_gate = nn.Sequential(nn.SiLU(), _init.linear(global_cond_dim, dim * 6, bias=False, zero=True))


class ContinuousTransformer(nn.Module):
    def __init__(self, dim, depth, *, dim_in=None, dim_out=None, dim_heads=64, cross_attend=False, cond_token_dim=None,
                 global_cond_dim=None, causal=False, rotary_pos_emb=True, zero_init_branch_outputs=True, conformer=False,
                 use_sinusoidal_emb=False, use_abs_pos_emb=False, abs_pos_emb_max_length=10000, **kwargs):
        super().__init__()
        assert not (use_sinusoidal_emb and use_abs_pos_emb), "Can't select both of sinusoidal/abs positional embedding type."
        self.dim, self.depth, self.causal, self.dim_heads = dim, depth, bool(causal), dim_heads      # causal: sat_dit_plan_set_attention_options
        self.project_in = _init.linear(dim_in, dim, bias=False) if dim_in else nn.Identity()
        self.project_out = _init.linear(dim, dim_out, bias=False) if dim_out else nn.Identity()
        self.rotary_pos_emb = RotaryEmbedding(max(dim_heads // 2, 32)) if rotary_pos_emb else None
        self.use_sinusoidal_emb, self.use_abs_pos_emb = use_sinusoidal_emb, use_abs_pos_emb
        self.pos_emb = None
        if use_sinusoidal_emb:
            self.pos_emb = ScaledSinusoidalEmbedding(dim)
        elif use_abs_pos_emb:
            self.pos_emb = AbsolutePositionalEmbedding(dim, abs_pos_emb_max_length)
        self.layers = nn.ModuleList([
            TransformerBlock(dim, dim_heads=dim_heads, cross_attend=cross_attend, dim_context=cond_token_dim,
                             global_cond_dim=global_cond_dim, causal=causal, zero_init_branch_outputs=zero_init_branch_outputs,
                             conformer=conformer, layer_ix=i, **kwargs)
            for i in range(depth)
        ])
        # one attn_kwargs for every block and both attentions of it: the plan takes a single flag
        self.qk_norm = bool(kwargs.get("attn_kwargs", {}).get("qk_norm", False))
        # one window for every block (sat_dit_plan_set_neighborhood_attention, or its _hdw twin off 64-channel heads); 0 = full attention
        self.natten_kernel_size = self.layers[0].self_attn.natten_kernel_size if depth else 0
        # likewise one conformer / remove_norms / glu for every block (sat_dit_plan_set_block_options)
        self.block_options = (1 if conformer else 0, 1 if kwargs.get("remove_norms", False) else 0,
                              1 if kwargs.get("ff_kwargs", {}).get("glu", True) else 0)
        # and one conv_kernel_size (sat_dit_plan_set_ff_conv); 1 = Linear feed-forwards
        self.ff_conv_kernel = self.layers[0].ff.conv_kernel_size
        assert all(a.qk_norm == self.qk_norm for l in self.layers for a in (l.self_attn, getattr(l, "cross_attn", l.self_attn)))

    def forward(self, *args, **kwargs):
        raise RuntimeError("ContinuousTransformer has no standalone forward in this build: the stack runs inside "
                           "DiffusionTransformer (one sat_dit_forward call); there is no CPU/eager path")
