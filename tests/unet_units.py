"""The Dance Diffusion U-Net restated in plain PyTorch, written from the operation and generic in the dtype (float64: the reference of the kernel
tests and the restatement test_unet_host.py holds against the goldens; float32: the CPU evaluation of the same arithmetic), and the
references, shapes and gates of its single kernels (csrc/unet_kernels.hip; tests/test_gpu_unet_kernels.py).

``forward(sd, cfg, x, t, plant=...)`` is ``DiffusionAttnUnet1D(**cfg)(x, t)`` on a state dict with the reference's names.  ``plant`` names one
deliberate mistake, for the tests that show the gates reject it:
  "concat_order"     cat([x, main(x)]) instead of cat([main(x), x])
  "zero_pad"         zero instead of reflect padding in the resamplers
  "unclipped_time"   the timestep planes continue past the ends of the sequence instead of being zero-padded with the audio
  "per_channel_norm" GroupNorm(c, c) instead of GroupNorm(1, c)
  "tanh_gelu"        the tanh approximation instead of the erf form
  "scale_once"       logits scaled by 32^-1/4 once instead of on q and on k
"""
import math

import torch
import torch.nn.functional as F

CUBIC = [-0.01171875, -0.03515625, 0.11328125, 0.43359375, 0.43359375, 0.11328125, -0.03515625, -0.01171875]
PLANTS = ("concat_order", "zero_pad", "unclipped_time", "per_channel_norm", "tanh_gelu", "scale_once")
UNIT = 2.0 ** -24


def downsample(x, plant=None):
    c = x.shape[1]
    w = torch.tensor(CUBIC, dtype=x.dtype).view(1, 1, 8).repeat(c, 1, 1)
    x = F.pad(x, (3, 3)) if plant == "zero_pad" else F.pad(x, (3, 3), "reflect")
    return F.conv1d(x, w, stride=2, groups=c)


def upsample(x, plant=None):
    c = x.shape[1]
    w = (2 * torch.tensor(CUBIC, dtype=x.dtype)).view(1, 1, 8).repeat(c, 1, 1)
    x = F.pad(x, (2, 2)) if plant == "zero_pad" else F.pad(x, (2, 2), "reflect")
    return F.conv_transpose1d(x, w, stride=2, padding=7, groups=c)


def group_norm(x, w, b, plant=None):
    return F.group_norm(x, x.shape[1] if plant == "per_channel_norm" else 1, w, b, 1e-5)


def gelu(x, plant=None):
    return F.gelu(x, approximate="tanh" if plant == "tanh_gelu" else "none")


def _conv(sd, pre, x, dt, pad):
    bias = sd.get(pre + ".bias")
    return F.conv1d(x, sd[pre + ".weight"].to(dt), None if bias is None else bias.to(dt), padding=pad)


def res_conv_block(sd, pre, x, k, is_last, plant=None, first_padded=None):
    dt = x.dtype
    h = _conv(sd, pre + "main.0", x, dt, k // 2) if first_padded is None else _conv(sd, pre + "main.0", first_padded, dt, 0)
    h = gelu(group_norm(h, sd[pre + "main.1.weight"].to(dt), sd[pre + "main.1.bias"].to(dt), plant), plant)
    h = _conv(sd, pre + "main.3", h, dt, k // 2)
    if not is_last:
        h = gelu(group_norm(h, sd[pre + "main.4.weight"].to(dt), sd[pre + "main.4.bias"].to(dt), plant), plant)
    skip = _conv(sd, pre + "skip", x, dt, 0) if pre + "skip.weight" in sd else x
    return h + skip


def self_attention(sd, pre, x, plant=None):
    dt = x.dtype
    n, c, s = x.shape
    heads = c // 32
    qkv = _conv(sd, pre + "qkv_proj", F.group_norm(x, 1, sd[pre + "norm.weight"].to(dt), sd[pre + "norm.bias"].to(dt), 1e-5), dt, 0)
    q, k, v = qkv.view(n, 3 * heads, 32, s).transpose(2, 3).chunk(3, dim=1)
    scale = 32 ** -0.25
    att = ((q * scale) @ (k.transpose(2, 3) * (1.0 if plant == "scale_once" else scale))).softmax(3)
    y = (att @ v).transpose(2, 3).contiguous().view(n, c, s)
    return x + _conv(sd, pre + "out_proj", y, dt, 0)


def _level(sd, cfg, pre, x, i, plant):
    """the reference's level i (1-based, i >= 2): a SkipBlock whose children live under pre"""
    depth, k = cfg["depth"], cfg.get("kernel_size", 5)
    attn = cfg["n_attn_layers"] > 0 and i >= depth - cfg["n_attn_layers"]
    at = lambda j: f"{pre}{j}."
    h = downsample(x, plant)
    for j in (1, 3, 5):
        h = res_conv_block(sd, at(j), h, k, False, plant)
        if attn:
            h = self_attention(sd, at(j + 1), h, plant)
    if i < depth:
        h = _level(sd, cfg, at(7) + "main.", h, i + 1, plant)
    for j in (8, 10, 12):
        h = res_conv_block(sd, at(j), h, k, False, plant)
        if attn:
            h = self_attention(sd, at(j + 1), h, plant)
    h = upsample(h, plant)
    return torch.cat([x, h] if plant == "concat_order" else [h, x], dim=1)


def timestep_planes(sd, t, length, dt):
    f = 2 * math.pi * t.to(dt)[:, None] @ sd["timestep_embed.weight"].to(dt).T
    return torch.cat([f.cos(), f.sin()], dim=-1)[..., None].repeat(1, 1, length)


def forward(sd, cfg, x, t, dtype=torch.float64, plant=None):
    assert plant is None or plant in PLANTS
    depth, k = cfg["depth"], cfg.get("kernel_size", 5)
    x = x.to(dtype)
    planes = timestep_planes(sd, t, x.shape[2], dtype)
    h = torch.cat([x, planes], dim=1)
    padded = None
    if plant == "unclipped_time":
        padded = torch.cat([F.pad(x, (k // 2, k // 2)), timestep_planes(sd, t, x.shape[2] + 2 * (k // 2), dtype)], dim=1)
    h = res_conv_block(sd, "net.0.", h, k, False, plant, first_padded=padded)
    h = res_conv_block(sd, "net.1.", h, k, False, plant)
    h = res_conv_block(sd, "net.2.", h, k, False, plant)
    if depth > 1:
        h = _level(sd, cfg, "net.3.main.", h, 2, plant)
    h = res_conv_block(sd, "net.4.", h, k, False, plant)
    h = res_conv_block(sd, "net.5.", h, k, False, plant)
    return res_conv_block(sd, "net.6.", h, k, True, plant)


def vdenoise(v, x, sigma):
    """k-diffusion's VDenoiser (sigma_data = 1) applied to v = net(x * c_in, atan(sigma) * 2 / pi)"""
    return v * (-sigma / math.sqrt(sigma * sigma + 1.0)) + x * (1.0 / (sigma * sigma + 1.0))


# ------------------------------------------------------------------------------------------------------------------ single kernels
FMT = {"bf16": 0, "fp16": 3, "fp32": 2}      # include/sat_hip.h: SAT_GEMM_BF16, SAT_GEMM_FP16, SAT_GEMM_FP32X
TORCH_DTYPE = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}

# (rows per item, channels): one 3-row item (a fraction of one 4096-element tile), 1064 x 128 (33 tiles and a quarter), 2048 x 512 + 3 rows
# (257 tiles, the last one short): the finish walks more partials than it has threads
GN_SHAPES = [(3, 128), (1064, 128), (2051, 512)]
GN_RATIOS = [0.0, 8.0]      # |mean| / std of an item
GN_BATCH = 2
RESAMPLE_LENGTHS = [4, 6, 24, 1064]


def gn_input(rows, c, ratio, seed=3):
    g = torch.Generator().manual_seed(seed * 1000003 + rows * 131 + c + int(ratio))
    x = torch.randn(GN_BATCH, rows, c, generator=g)
    x[1] *= 3.0                               # the items have statistics of their own
    return (x + ratio * x.std(dim=(1, 2), keepdim=True)).float()


def gn_reference(x, gamma, beta, skip, act, dtype=torch.float64):
    """x [b, rows, c] -> ((mean, rstd) [b, 2], y [b, rows, c]) as nn.GroupNorm(1, c) + GELU + skip compute them, in dtype"""
    x, gamma, beta = x.to(dtype), gamma.to(dtype), beta.to(dtype)
    mean = x.mean(dim=(1, 2), keepdim=True)
    var = ((x - mean) ** 2).mean(dim=(1, 2), keepdim=True)
    rstd = 1.0 / torch.sqrt(var + 1e-5)
    y = (x - mean) * rstd * gamma + beta
    if act:
        y = F.gelu(y)
    if skip is not None:
        y = y + skip.to(dtype)
    return torch.stack([mean.flatten(), rstd.flatten()], dim=1), y


def elementwise_share(got, want, tol=1e-5):
    """the largest |got - want| over tol * max(|want|, rms of the element's row): 1 is the gate"""
    want = want.double()
    scale = torch.maximum(want.abs(), want.pow(2).mean(dim=-1, keepdim=True).sqrt())
    return float(((got.double() - want).abs() / (tol * scale)).max())


def code_spacing(want64, dtype):
    """the distance between neighbouring codes of the 16-bit format at |want| (the subnormal spacing below the normal range)"""
    mant, emin = (10, -14) if dtype == torch.float16 else (7, -126)
    e = torch.floor(torch.log2(want64.abs().clamp_min(2.0 ** emin)))
    return torch.exp2(e - mant)


def rounded_share(got16, want64, dtype, slack):
    """|got - want| over (one code of the format at |want| + slack), the largest: 1 is the gate.  slack is what the fp32 value may be off before
    it is rounded (the fp32 gate of the same output).  Stated on the absolute scale because "codes from the correctly rounded result" is not
    a property fp32 arithmetic has where a result cancels to near zero: the fp32 restatement of the GroupNorm apply on the CPU sits up to 22
    fp16 codes and 27 k bf16 codes from the correctly rounded float64 result there, with every element inside 0.2 of the 1e-5 gate."""
    want64 = want64.double()
    err = (got16.detach().cpu().double() - want64).abs()
    return float((err / (code_spacing(want64, dtype) + slack)).max())


def resample_bound(x, up):
    """(8 + 4) 2^-24 sum_j |k_j| |x_j| per output element, from the float64 magnitudes (x [b, c, s])"""
    return _abs_resample(x.double().abs(), up) * 12 * UNIT


def _abs_resample(xa, up):
    c = xa.shape[1]
    k = torch.tensor(CUBIC, dtype=xa.dtype).abs() * (2 if up else 1)
    w = k.view(1, 1, 8).repeat(c, 1, 1)
    if up:
        return F.conv_transpose1d(F.pad(xa, (2, 2), "reflect"), w, stride=2, padding=7, groups=c)
    return F.conv1d(F.pad(xa, (3, 3), "reflect"), w, stride=2, groups=c)
