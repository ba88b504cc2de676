"""The fp16 range reports on the device: the reduction kernel (csrc/range_stats.hip) against torch on the host, field by field and exactly;
sat_dit_range_report on the reduced DiT (bit-identical outputs, an exactly restated slot, an overflow planted in one buffer and found there,
fp16 against bf16, accumulation, the slot the fused cross launch does not materialise); sat_oobleck_range_report on the 16-channel VAE of
the reference goldens in all three builds; and stable_audio_tools.inference.preflight.check_fp16_range on the reduced SA-Open model.
Host-side validation and the Python lifecycle: tests/test_range_report_host.py."""
import ctypes
import os
import struct
import sys

import pytest
import torch
import torch.nn.functional as F

from util import FORMATS, SUITE, assert_close
from test_gpu_codec_options import GATE, _small_vae

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
import cases  # noqa: E402
import dit_head_dim_cases as HC  # noqa: E402

pytestmark = pytest.mark.gpu

FP16_MAX = 65504.0
DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16, "fp32": torch.float32}
# one rounding of the operand format, relative (unit roundoff 2^-11 / 2^-8 with a factor 2 for the value rounding the other way)
ONE_ROUNDING = {"fp16": 2.0 ** -10, "bf16": 2.0 ** -7}


# ------------------------------------------------------------------------------------------------------------------------ 1. the kernel
def _read_record(rec):
    torch.cuda.synchronize()
    max_abs, launches, over, nonfinite, elements = struct.unpack("<fIQQQ", rec.cpu().numpy().tobytes())
    return dict(max_abs=max_abs, launches=launches, over_fp16=over, nonfinite=nonfinite, elements=elements)


def _host_record(valid):
    v = valid.float().cpu()
    fin = torch.isfinite(v)
    return dict(max_abs=v[fin].abs().max().item() if bool(fin.any()) else 0.0, launches=1,
                over_fp16=int(((v.abs() >= FP16_MAX) | ~fin).sum()), nonfinite=int((~fin).sum()), elements=v.numel())


@pytest.mark.parametrize("fmt", ["fp16", "bf16", "fp32"])
@pytest.mark.parametrize("rows,cols,pitch", [(1, 1, 1), (3, 65, 128), (257, 200, 200), (1, 2 ** 20 + 3, 2 ** 20 + 3), (1, 2 ** 22 + 5, 2 ** 22 + 5)],
                         ids=["1x1", "3x65_pitch128", "257x200", "1d_2^20+3", "1d_2^22+5"])
def test_kernel_matches_torch_exactly(dev, rows, cols, pitch, fmt):
    """(1, 1): one scalar; (3, 65) at pitch 128: 16-byte body and a one-element tail per row, 63 pad columns of NaN / 1e30 that must not
    count; (257, 200) at pitch 200: contiguous rows that start unaligned (fp16 / bf16: 400 bytes); 2^20 + 3: a tail behind 257 workgroups'
    worth of vectors; 2^22 + 5: 1025 workgroups' worth against a grid cap of 2 x CUs.  Planted: 65504 in the last element, one inf, one
    NaN, and -7e4 where the format holds it.  Every field equal; a second call doubles elements and launches, adds the counts, keeps max_abs."""
    from stable_audio_tools import _hip
    dtype = DTYPES[fmt]
    n = rows * cols
    g = torch.Generator().manual_seed(rows * 131 + cols)
    valid = (torch.randn(rows, cols, generator=g) * 100.0).to(dtype)
    flat = valid.view(-1)
    flat[n - 1] = FP16_MAX
    if n >= 8:
        flat[1], flat[n // 3] = float("inf"), float("nan")
        if fmt != "fp16":
            flat[n // 2] = -7e4
    buf = torch.empty(rows, pitch, dtype=dtype)
    if pitch > cols:          # pad columns: NaN and 1e30 (inf in fp16) in turn
        buf[:, cols:] = torch.tensor([float("nan"), 1e30]).to(dtype).repeat(pitch)[: pitch - cols]
    buf[:, :cols] = valid
    want = _host_record(valid)
    assert want["over_fp16"] >= 1 and want["elements"] == n
    if n >= 8:
        assert want["nonfinite"] == 2 and want["max_abs"] == (7e4 if fmt == "fp32" else float(torch.tensor(7e4).to(dtype)) if fmt == "bf16" else FP16_MAX)
    x = buf.to(dev)
    rec = torch.zeros(4, dtype=torch.int64, device=dev)
    fn = getattr(_hip.lib(), {"fp16": "sat_range_stats_f16", "bf16": "sat_range_stats_bf16", "fp32": "sat_range_stats_f32"}[fmt])
    _hip.check(fn(_hip.ptr(x), rows, cols, pitch, _hip.ptr(rec), _hip.stream()))
    got = _read_record(rec)
    assert got == want, (got, want)
    _hip.check(fn(_hip.ptr(x), rows, cols, pitch, _hip.ptr(rec), _hip.stream()))
    twice = _read_record(rec)
    assert twice == dict(max_abs=want["max_abs"], launches=2, over_fp16=2 * want["over_fp16"], nonfinite=2 * want["nonfinite"], elements=2 * n)


def test_kernel_rejects_bad_views(dev):
    from stable_audio_tools import _hip
    lib = _hip.lib()
    x = torch.zeros(64, device=dev)
    rec = torch.zeros(4, dtype=torch.int64, device=dev)
    assert lib.sat_range_stats_f32(_hip.ptr(x), 2, 8, 4, _hip.ptr(rec), _hip.stream()) == -1          # pitch < cols
    assert lib.sat_range_stats_f32(_hip.ptr(x), 0, 8, 8, _hip.ptr(rec), _hip.stream()) == -1
    assert lib.sat_range_stats_f32(None, 1, 8, 8, _hip.ptr(rec), _hip.stream()) == -1
    assert lib.sat_range_stats_f32(_hip.ptr(x), 1, 8, 8, None, _hip.stream()) == -1
    assert _read_record(rec)["launches"] == 0


# ------------------------------------------------------------------------------------------------------------------------ 2. the DiT
B, T_LEN, CFG, SIGMA = 2, 77, 7.0, 3.7          # S = 78 rows per sequence, four sequences, key shift 2 on the second
_DITS = {}


def _dit(dev, cfg_name="small"):
    """The reduced DiT (cases.SMALL_DIT) or a 128-channel-head config of dit_head_dim_cases.py, seed-0 weights; returns (module, fp32 state dict)"""
    if cfg_name not in _DITS:
        from stable_audio_tools.models import _init
        from stable_audio_tools.models.dit import DiffusionTransformer
        with _init.skip_init():
            m = DiffusionTransformer(**(cases.SMALL_DIT if cfg_name == "small" else HC.CONFIGS[cfg_name]))
        sd = HC.synth_weights(m.state_dict(), 0)
        m.load_state_dict(sd)
        _DITS[cfg_name] = (m.to(dev).eval(), {k: v.clone() for k, v in sd.items()})
    m, sd = _DITS[cfg_name]
    m.load_state_dict(sd)          # (a test that planted weights leaves none behind)
    return m.set_layernorm_fusion(True).set_cross_attention_fusion(True), sd


def _inputs():
    x, _, c, g = cases.dit_inputs(B, T_LEN, 128, 96, 1)
    return x, c, g


_ON_DEVICE = {}


def _step(m, dev, fresh_context=True):
    """One sampler step on the shared inputs: prepare_generation (once per generation: the conditioning MLPs and the cross K / V cache, hence the
    cross_k / cross_v records) + denoise; fresh_context=False is a further step of the same generation, denoise alone, as the sampler loop runs it."""
    if "inputs" not in _ON_DEVICE:
        x, c, g = _inputs()
        _ON_DEVICE["inputs"] = ((x * SIGMA).to(dev), c.to(dev), g.to(dev))
    x, c, g = _ON_DEVICE["inputs"]
    if fresh_context:
        m._ctx_key = None
        m.prepare_generation(c, g, CFG)
    return m.denoise(x, SIGMA, cfg_scale=CFG)


def _table(rows):
    return {(r["layer"], r["buffer"]): r for r in rows}


def _cross_kv_restated(sd, c, fmt, depth):
    """to_cond_embed -> to_kv -> chunk of every layer in fp32 on the CFG batch (conditional half, then the all-zero null half), with the
    operands the device GEMM reads -- the context embedding and the weight rounded once to the operand format -- and fp64 sums: what is
    left between this and the stored k / v is the one rounding of the store."""
    from oracle import dit as odit
    rnd = lambda v: v.to(DTYPES[fmt]).double()
    bc = torch.cat([c, torch.zeros_like(c)], dim=0)
    ce = rnd(odit._mlp(sd, "to_cond_embed.", bc, bias=False))
    out = []
    for l in range(depth):
        k, v = (ce @ rnd(sd[f"transformer.layers.{l}.cross_attn.to_kv.weight"]).T).chunk(2, dim=-1)
        out.append((k.abs().max().item(), v.abs().max().item()))
    return out


def _expected_elements(m, fused_cross):
    d, inner = m.embed_dim, m.transformer.layers[0].ff.ff[0].proj.weight.shape[0] // 2
    rows, rows_c = 2 * B * (T_LEN + 1), B * (T_LEN + 1)
    e = {"a_qkv": rows * d, "q": rows * d, "k": rows * d, "v": rows * d, "attn_out": rows * d, "a_cross_q": rows_c * d,
         "cross_q": 0 if fused_cross else rows_c * d, "cross_attn_out": rows_c * d, "a_ff": rows * d, "ff_hidden": rows * inner,
         "cross_k": 2 * B * 130 * m.cond_embed_dim, "cross_v": 2 * B * 130 * m.cond_embed_dim}
    return e


DIT_CASES = [("small", fmt, fold, fuse) for fmt in ("fp16", "bf16") for fold in (True, False) for fuse in (True, False)] + \
            [("hd128", "fp16", True, True), ("hd128", "bf16", True, True)]


@pytest.mark.parametrize("cfg_name,fmt,fold,fuse", DIT_CASES, ids=lambda v: str(v))
def test_dit_report_changes_no_bit_and_fills_its_slots(dev, cfg_name, fmt, fold, fuse):
    m, sd = _dit(dev, cfg_name)
    m.set_gemm_dtype(fmt).set_layernorm_fusion(fold).set_cross_attention_fusion(fuse)
    x, c, g = _inputs()
    try:
        off = _step(m, dev).clone()
        m.activation_range_report(True)
        on = _step(m, dev).clone()
        rows = m.activation_range_report(False)
        after = _step(m, dev)
    finally:
        m.set_gemm_dtype(SUITE.gemm_dtype)
    assert torch.isfinite(off).all()
    assert torch.equal(on, off), "the range report changed the output"
    assert torch.equal(after, off)
    assert len(rows) == m.depth * 12
    t = _table(rows)
    hd128 = cfg_name != "small"
    want_elements = _expected_elements(m, fused_cross=fuse and not hd128)          # (the 128-channel-head route has no fused cross launch)
    restated = _cross_kv_restated(sd, c, fmt, m.depth)
    for l in range(m.depth):
        for name, n in want_elements.items():
            r = t[(l, name)]
            assert r["elements"] == n, (l, name, r, n)
            assert r["launches"] == (1 if n else 0) and r["nonfinite"] == 0 and r["over_fp16"] == 0, (l, name, r)
            assert (r["max_abs"] > 0) == (n > 0), (l, name, r)
        fold_here = fold and not hd128
        assert t[(l, "a_ff")]["holds"] == ("residual image" if fold_here else "layernorm output")
        assert t[(l, "a_qkv")]["holds"] == ("residual image" if fold_here and l > 0 else "layernorm output")
        # the exact slot: the layer's context cache against its restatement, to one rounding of the store
        for name, want in zip(("cross_k", "cross_v"), restated[l]):
            got = t[(l, name)]["max_abs"]
            print(f"[{cfg_name} {fmt} fold={fold} fuse={fuse}] layer {l} {name}: max_abs {got:.6g}, restated {want:.6g}, rel {abs(got - want) / want:.2e}")
            assert abs(got - want) <= ONE_ROUNDING[fmt] * want, (l, name, got, want)


def _ff_in_rows(sd, x, t, c, g, heads, layer):
    """fp32 restatement, from the oracle's pieces, of the rows the FF-in GEMM of `layer` reads: ff_norm of the residual stream behind the
    layer's two attention branches (transformer.py:692-700)"""
    from oracle import dit as odit
    context = odit._mlp(sd, "to_cond_embed.", c, bias=False)
    ge = odit._mlp(sd, "to_global_embed.", g, bias=False) + odit._mlp(sd, "to_timestep_embed.", odit.fourier_features(sd["timestep_features.weight"], t[:, None]), bias=True)
    h = (F.conv1d(x, sd["preprocess_conv.weight"]) + x).transpose(1, 2)
    h = torch.cat((ge.unsqueeze(1), F.linear(h, sd["transformer.project_in.weight"])), dim=-2)
    dim_heads = h.shape[-1] // heads
    freqs = odit.rotary_freqs(sd["transformer.rotary_pos_emb.inv_freq"], h.shape[1])
    for i in range(layer):
        h = odit.transformer_block(sd, f"transformer.layers.{i}.", h, context, freqs, heads, dim_heads, first=i == 0)
    p = f"transformer.layers.{layer}."
    h = h + odit.self_attention(sd, p + "self_attn.", odit.layer_norm(h, sd[p + "pre_norm.gamma"], sd[p + "pre_norm.beta"]), freqs, heads)
    a = odit.layer_norm(h, sd[p + "cross_attend_norm.gamma"], sd[p + "cross_attend_norm.beta"])
    h = h + odit.cross_attention(sd, p + "cross_attn.", a, context, heads, dim_heads)
    return odit.layer_norm(h, sd[p + "ff_norm.gamma"], sd[p + "ff_norm.beta"])


def _plant_ff_overflow(sd, rows, layer=1, prefix=""):
    """The factor (a power of two, exact in every format) on ``layers.<layer>.ff.ff.0.proj.{weight, bias}`` with which the SwiGLU hidden state
    of the restated GEMM passes 4 x 65504 -- the margin covers the 16-bit operands of the device GEMM (1e-2 at most) many times over --
    and the state dict with it applied.  Returns (planted state dict, factor, restated peak)."""
    wk, bk = f"{prefix}transformer.layers.{layer}.ff.ff.0.proj.weight", f"{prefix}transformer.layers.{layer}.ff.ff.0.proj.bias"
    val, gate = F.linear(rows, sd[wk], sd[bk]).chunk(2, dim=-1)
    peak = lambda s: (s * val * F.silu(s * gate)).abs().max().item()
    assert peak(1.0) < FP16_MAX / 16, "the un-planted hidden state is expected far inside the range"
    s = 2.0
    while peak(s) <= 4 * FP16_MAX:
        s *= 2.0
    planted = dict(sd)
    planted[wk], planted[bk] = sd[wk] * s, sd[bk] * s
    return planted, s, peak(s)


def test_dit_report_localises_a_planted_overflow(dev):
    """ff.ff.0.proj of layer 1 scaled until the restated hidden state passes the fp16 range: (1, ff_hidden) says so in fp16 (clamped
    elements) and in bf16 (elements fp16 would clamp), every slot of layer 0 stays at 0, and nothing is non-finite anywhere."""
    m, sd = _dit(dev)
    x, c, g = _inputs()
    sigma = torch.full((B,), SIGMA)
    t = torch.atan(sigma) / torch.pi * 2                     # k-diffusion VDenoiser, as sat_dit_denoise_cfg
    rows = _ff_in_rows(sd, x * SIGMA / (SIGMA ** 2 + 1) ** 0.5, t, c, g, m.num_heads, 1)          # the conditional half of the CFG batch
    planted, s, peak = _plant_ff_overflow(sd, rows)
    assert peak > FP16_MAX
    print(f"\n[planted FF overflow] factor {s:g}, restated hidden peak {peak:.4g}")
    m.load_state_dict(planted)
    try:
        for fmt in ("fp16", "bf16"):
            m.set_gemm_dtype(fmt)
            m.activation_range_report(True)
            _step(m, dev)
            t_ = _table(m.activation_range_report(False))
            hid = t_[(1, "ff_hidden")]
            print(f"  {fmt}: (1, ff_hidden) {hid}")
            assert hid["over_fp16"] > 0, (fmt, hid)
            assert hid["max_abs"] == FP16_MAX if fmt == "fp16" else hid["max_abs"] > FP16_MAX, (fmt, hid)
            assert all(r["over_fp16"] == 0 for (l, _), r in t_.items() if l == 0), [r for (l, _), r in t_.items() if l == 0 and r["over_fp16"]]
            assert all(r["nonfinite"] == 0 for r in t_.values()), [r for r in t_.values() if r["nonfinite"]]
    finally:
        m.load_state_dict(sd)
        m.set_gemm_dtype(SUITE.gemm_dtype)


@pytest.mark.parametrize("cfg_name", ["small", "hd128"])
def test_dit_report_fp16_and_bf16_agree(dev, cfg_name):
    """max_abs of every materialised slot within 5 % between the two formats.  The bound is for a wrong buffer, stride or row count, which
    shows as a factor; it is loose against the project's own bf16 forward gate of 1.2e-2.  The worst ratio is printed
    (profiles/range_report_verification.txt)."""
    m, _ = _dit(dev, cfg_name)
    tables = {}
    try:
        for fmt in ("fp16", "bf16"):
            m.set_gemm_dtype(fmt)
            m.activation_range_report(True)
            _step(m, dev)
            tables[fmt] = _table(m.activation_range_report(False))
    finally:
        m.set_gemm_dtype(SUITE.gemm_dtype)
    worst, where = 1.0, None
    for key, r16 in tables["fp16"].items():
        rb = tables["bf16"][key]
        assert (r16["elements"] > 0) == (rb["elements"] > 0) and r16["elements"] == rb["elements"], key
        if r16["elements"] == 0:
            continue
        ratio = max(r16["max_abs"], rb["max_abs"]) / min(r16["max_abs"], rb["max_abs"])
        if ratio > worst:
            worst, where = ratio, key
    print(f"\n[{cfg_name}] worst fp16 / bf16 max_abs ratio over {len(tables['fp16'])} slots: {worst:.5f} at {where}")
    assert worst <= 1.05, (worst, where, tables["fp16"][where], tables["bf16"][where])


def test_dit_report_accumulates_resets_and_leaves_sat_dit_debug_alone(dev):
    m, _ = _dit(dev)
    m.set_gemm_dtype(SUITE.gemm_dtype)
    # residual_stream_report without the new report ...
    m.residual_stream_report(True)
    _step(m, dev)
    alone = m.residual_stream_report(False)
    # ... and beside it
    m.activation_range_report(True)
    m.residual_stream_report(True)
    _step(m, dev)
    beside = m.residual_stream_report(False)
    assert beside == alone, "sat_dit_debug's figures changed with the range report on"
    _step(m, dev, fresh_context=False)          # a second denoise of the same generation: the context is not prepared again
    once_twice = _table(m.activation_range_report(False))
    m.activation_range_report(True)
    _step(m, dev)
    one = _table(m.activation_range_report(False))
    for key, r in one.items():
        per_generation = key[1] in ("cross_k", "cross_v")
        k = 1 if per_generation else 2
        assert once_twice[key]["launches"] == k * r["launches"] and once_twice[key]["elements"] == k * r["elements"], (key, once_twice[key], r)
        assert once_twice[key]["max_abs"] == r["max_abs"]          # the same step twice
    # mode 2: everything back to zero, still enabled
    m.activation_range_report(True)
    _step(m, dev)
    m.reset_activation_range_report()
    zero = m.activation_range_report(False)
    assert all(r["max_abs"] == 0 and r["launches"] == 0 and r["elements"] == 0 and r["over_fp16"] == 0 and r["nonfinite"] == 0 for r in zero)
    m.activation_range_report(True)
    m.reset_activation_range_report()
    _step(m, dev)
    again = _table(m.activation_range_report(False))
    assert again == one


def test_dit_cross_q_slot_follows_the_fused_launch(dev):
    """One prompt without CFG (one sequence of 78 rows): the fused to_q + cross-attention launch keeps Q in registers and the slot stays
    empty; with the fusion switched off the separate projection writes Q and the slot is filled.  The outputs are bit-identical there
    (tests/test_gpu_models.py::test_cross_attention_fusion_on_off), and so is every other slot's max_abs."""
    m, _ = _dit(dev)
    m.set_gemm_dtype(SUITE.gemm_dtype)
    x, _, c, g = cases.dit_inputs(1, T_LEN, 128, 96, 1)
    tables = {}
    try:
        for fuse in (True, False):
            m.set_cross_attention_fusion(fuse)
            m.activation_range_report(True)
            m._ctx_key = None
            m.prepare_generation(c.to(dev), g.to(dev), 1.0)
            m.denoise((x * SIGMA).to(dev), SIGMA, cfg_scale=1.0)
            tables[fuse] = _table(m.activation_range_report(False))
    finally:
        m.set_cross_attention_fusion(True)
    for l in range(m.depth):
        assert tables[True][(l, "cross_q")]["elements"] == 0 and tables[True][(l, "cross_q")]["launches"] == 0
        assert tables[False][(l, "cross_q")]["elements"] == (T_LEN + 1) * m.embed_dim and tables[False][(l, "cross_q")]["max_abs"] > 0
    for key, r in tables[True].items():
        if key[1] != "cross_q":
            assert r == tables[False][key], (key, r, tables[False][key])


# ------------------------------------------------------------------------------------------------------------------------ 3. the codec
FRAMES = 7


def _codec_inputs():
    from stable_audio_tools import synthetic
    return synthetic.synth_input("z7", (2, 64, FRAMES), 41), synthetic.synth_input("a7", (2, 2, 2048 * FRAMES), 42, 0.3)


@pytest.mark.parametrize("fmt", ["fp16", "bf16", "fp32"])
def test_codec_report(dev, fmt):
    """The 16-channel VAE of the reference goldens (widths 16 ... 256: padded, two-launch and fused ResidualUnits), batch 2, 7 latent
    frames.  The comparison with the reference's goldens runs on the goldens' own inputs (9 frames decoded, 5 encoded: what
    tests/test_gpu_codec_options.py::test_small_vae_reference_goldens uses) with the report ON, under that test's gates."""
    from stable_audio_tools import _hip, synthetic
    never = _small_vae(dev, fmt)
    ae = _small_vae(dev, fmt)
    z, a = _codec_inputs()
    z, a = z.to(dev), a.to(dev)
    base_d, base_e = never.decoder(z), never.encoder(a)
    assert ae.activation_range_report(True) is None
    on_d, on_e = ae.decoder(z), ae.encoder(a)
    n = ctypes.c_int32()
    counts = {}
    for part in ("encoder", "decoder"):
        _hip.check(_hip.lib().sat_oobleck_range_report_count(getattr(ae, part)._plan, ctypes.byref(n)))
        counts[part] = n.value
    rows = ae.activation_range_report(False)
    for part in ("encoder", "decoder"):
        mine = [r for r in rows if r["part"] == part]
        assert len(mine) == counts[part] and len({r["name"] for r in mine}) == len(mine)
        assert [r["index"] for r in mine] == list(range(len(mine)))
        assert all(r["launches"] == 1 and r["elements"] > 0 and r["nonfinite"] == 0 and r["over_fp16"] == 0 and 0 < r["max_abs"] < FP16_MAX for r in mine), \
            [r for r in mine if not (r["launches"] == 1 and 0 < r["max_abs"] < FP16_MAX)]
    dec = [r for r in rows if r["part"] == "decoder"]
    # record 0 is the channels-last image of the input: max |z| rounded to the operand format, exactly; 64 latent channels, no padding
    assert dec[0]["name"] == "input" and dec[0]["elements"] == 2 * FRAMES * 64
    assert dec[0]["max_abs"] == z.cpu().to(DTYPES[fmt]).float().abs().max().item()
    # the widest tensors: [2, 7 * 2048 samples, 16 channels padded to 64]
    assert max(r["elements"] for r in dec) == 2 * FRAMES * 2048 * 64
    # after disabling: the bits of a model that never enabled it (the fused ResidualUnits are back)
    assert torch.equal(ae.decoder(z), base_d) and torch.equal(ae.encoder(a), base_e)
    equal_d, equal_e = torch.equal(on_d, base_d), torch.equal(on_e, base_e)
    print(f"\n[codec report, {fmt}] two-launch ResidualUnits bit-equal to the fused route: decode {equal_d}, encode {equal_e}")
    # with the report on, inside the gates of the same model against the same goldens
    g = cases.load("vae")
    ae.activation_range_report(True)
    try:
        zg = synthetic.synth_input("z", (2, 64, 9), 7)
        ag = synthetic.synth_input("a", (2, 2, 2048 * 5), 8, 0.3)
        e = assert_close(f"small_decode with the report on ({fmt})", ae.decoder(zg.to(dev)), g["small_decode"], GATE[fmt])
        e2 = assert_close(f"small_encode with the report on ({fmt})", ae.encoder(ag.to(dev)), g["small_encode"], GATE[fmt])
    finally:
        ae.activation_range_report(False)
    print(f"  vs the reference with the report on: decode {e:.2e}, encode {e2:.2e} (gate {GATE[fmt]:.1e})")


def _last_unit_activated(sd, x, part, rnd):
    """Restatement from the oracle's pieces (oracle/oobleck.py, its matched-rounding convention: tensors travel un-rounded, every consumer
    sees ``rnd`` of them, the folded weights are rounded once) of the tensor the last ResidualUnit's 1 x 1 convolution writes: the unit's
    output behind the activation of its consumer, before the store rounds it."""
    import math
    from oracle import oobleck as oob
    r = (lambda v: v) if rnd is None else rnd
    strides = cases.SMALL_VAE["strides"]
    depth = len(strides)
    if part == "decoder":
        v = F.conv1d(r(x), oob._wconv(sd, "layers.0.", rnd), sd["layers.0.bias"], padding=3)
        for bi in range(depth):
            stride, pfx = strides[depth - 1 - bi], f"layers.{bi + 1}."
            h = r(oob.snake_beta(v, sd[pfx + "layers.0.alpha"], sd[pfx + "layers.0.beta"]))
            v = F.conv_transpose1d(h, oob._wconv(sd, pfx + "layers.1.", rnd), sd[pfx + "layers.1.bias"], stride=stride, padding=math.ceil(stride / 2))
            for ri, dil in enumerate((1, 3, 9)):
                v = oob.residual_unit(sd, f"{pfx}layers.{2 + ri}.", v, dil, rnd)
        return oob.snake_beta(v, sd[f"layers.{depth + 1}.alpha"], sd[f"layers.{depth + 1}.beta"])
    v = F.conv1d(x, oob.fold_weight_norm(sd["layers.0.weight_g"], sd["layers.0.weight_v"]), sd["layers.0.bias"], padding=3)
    for bi in range(depth):
        stride, pfx = strides[bi], f"layers.{bi + 1}."
        for ri, dil in enumerate((1, 3, 9)):
            v = oob.residual_unit(sd, f"{pfx}layers.{ri}.", v, dil, rnd)
        if bi + 1 == depth:
            return oob.snake_beta(v, sd[pfx + "layers.3.alpha"], sd[pfx + "layers.3.beta"])
        h = r(oob.snake_beta(v, sd[pfx + "layers.3.alpha"], sd[pfx + "layers.3.beta"]))
        v = F.conv1d(h, oob._wconv(sd, pfx + "layers.4.", rnd), sd[pfx + "layers.4.bias"], stride=stride, padding=math.ceil(stride / 2))


def _plant_codec_overflow(sd, x, part, fmt):
    """Scales the last ResidualUnit's 1 x 1 convolution as tests/test_gpu_codec_fp32.py::test_fp32_codec_keeps_activations_past_fp16_range
    does (``weight_g``, from that test's order of magnitude, 2^19 = 5.2e5, in powers of two), and its bias with it: in the fp16 build the
    folded weights themselves clamp at 65504, and with ``weight_g`` alone the restated activation of this 16-channel decoder levels off at
    6.3e4 -- inside the range, nothing for a report to find.  With the bias the planting is "the convolution's output times the factor" in
    every build.  The factor grows until the restatement with the build's own rounding passes 2 x 65504 (the 16-bit builds sit within
    1.5e-2 of it: the codec gates).  Returns (planted state dict, factor, restated peak)."""
    from util import bf16_round, fp16_round
    rnd = {"fp16": fp16_round, "bf16": bf16_round, "fp32": None}[fmt]
    unit = CODEC_UNIT[part]

    def planted(f):
        out = dict(sd)
        out[unit + ".weight_g"], out[unit + ".bias"] = sd[unit + ".weight_g"] * f, sd[unit + ".bias"] * f
        return out

    peak = lambda f: _last_unit_activated(planted(f), x, part, rnd).abs().max().item()
    assert peak(1.0) < FP16_MAX / 16, "the un-planted codec is expected far inside the range"
    f = 2.0 ** 19
    while peak(f) <= 2 * FP16_MAX:
        f *= 2.0
        assert f <= 2.0 ** 30
    return planted(f), f, peak(f)


CODEC_UNIT = {"decoder": "layers.5.layers.4.layers.3", "encoder": "layers.5.layers.2.layers.3"}


@pytest.mark.parametrize("fmt", ["fp16", "bf16", "fp32"])
@pytest.mark.parametrize("part", ["decoder", "encoder"])
def test_codec_report_localises_a_planted_overflow(dev, part, fmt):
    """The 1 x 1 convolution of the last ResidualUnit scaled until its restated output passes the fp16 range (_plant_codec_overflow): the
    first record that reports it is that convolution's, every earlier one has 0, nothing is non-finite; the fp16 build shows the clamp
    (max_abs == 65504), the bf16 and fp32 builds the un-clamped maximum, and the fp32 build's output stays finite."""
    ae = _small_vae(dev, fmt)
    module = getattr(ae, part)
    unit = CODEC_UNIT[part]
    sd = {k: v.detach().cpu().clone() for k, v in module.state_dict().items()}
    z, a = _codec_inputs()
    x = z if part == "decoder" else a
    planted, f, peak = _plant_codec_overflow(sd, x, part, fmt)
    assert peak > FP16_MAX
    module.load_state_dict(planted)
    module.activation_range_report(True)
    out = module(x.to(dev))
    rows = module.activation_range_report(False)
    over = [r for r in rows if r["over_fp16"] > 0]
    print(f"\n[codec planted overflow, {part} {fmt}] factor 2^{int(torch.tensor(f).log2())}, restated peak {peak:.4g}; first record over: {over[0] if over else None}")
    assert over and over[0]["name"] == unit, (over[:2], unit)
    assert all(r["over_fp16"] == 0 for r in rows[:over[0]["index"]])
    assert all(r["nonfinite"] == 0 for r in rows)
    if fmt == "fp16":
        assert over[0]["max_abs"] == FP16_MAX          # clamped
    else:
        assert over[0]["max_abs"] > FP16_MAX
        assert abs(over[0]["max_abs"] - peak) <= 3e-2 * peak          # the restated peak, to the codec gate (twice 1.5e-2)
    if fmt == "fp32":
        assert torch.isfinite(out).all()


# ------------------------------------------------------------------------------------------------------------------------ 4. check_fp16_range
def test_check_fp16_range_on_the_reduced_model(dev):
    import stable_audio_tools as S
    from stable_audio_tools import model_configs as MC, synthetic
    from stable_audio_tools.inference.preflight import check_fp16_range
    from stable_audio_tools.models import _init
    cfg = MC.reduced(MC.stable_audio_open_1_0())
    with _init.skip_init():
        model = S.create_model_from_config(cfg)
    sd = synthetic.synth_state_dict(model.state_dict(), 0)
    model.load_state_dict(sd)
    model = model.to(dev).eval()
    dc = cfg["model"]["diffusion"]["config"]
    b, t_len = 1, 16
    ratio = cfg["model"]["pretransform"]["config"]["downsampling_ratio"]
    cond = model.conditioner([{"seconds_start": 0, "seconds_total": 12}])
    cond["prompt"] = (synthetic.synth_input("prompt", (b, 128, dc["cond_token_dim"]), 1).to(dev), torch.ones(b, 128, device=dev))
    cond = {k: cond[k] for k in ("prompt", "seconds_start", "seconds_total")}
    noise = synthetic.synth_input("noise", (b, 64, t_len), 2)
    kw = dict(cfg_scale=7.0, conditioning_tensors=cond, sample_size=t_len * ratio, seed=3, device="cuda:0", sampler_type="dpmpp-3m-sde",
              sigma_min=0.3, sigma_max=500, noise=noise)
    dit, codec = model.model.model, model.pretransform.model
    before = (dit.gemm_dtype, codec.decoder.gemm_dtype)
    calls, denoise = [], dit.denoise
    dit.denoise = lambda *a, **k: (calls.append(1), denoise(*a, **k))[1]
    try:
        got = check_fp16_range(model, steps=2, **kw)
    finally:
        del dit.denoise
    assert len(calls) >= 2
    assert (dit.gemm_dtype, codec.decoder.gemm_dtype) == before and not dit._range_report and not codec.decoder._range_report
    assert len(got["dit"]) == dc["depth"] * 12 and got["codec"] and {r["part"] for r in got["codec"]} == {"encoder", "decoder"}
    used = [r for r in got["dit"] if r["elements"]]
    assert used and all(r["launches"] == (1 if r["buffer"] in ("cross_k", "cross_v") else len(calls)) for r in used), used[:3]          # every step, one context
    assert all(r["launches"] == 1 for r in got["codec"] if r["part"] == "decoder") and all(r["launches"] == 0 for r in got["codec"] if r["part"] == "encoder")
    assert 1.0 < got["headroom"] < float("inf") and got["tightest"] is not None and got["advice"] == []
    print(f"\n[check_fp16_range, reduced SA-Open] headroom {got['headroom']:.4g} at {got['tightest']}")
    # the planted FF scale of test 2, on the first sampler step's input (conditional half)
    ci = model.get_conditioning_inputs(cond)
    sig0 = 500.0
    xin = (noise * sig0) / (sig0 ** 2 + 1) ** 0.5
    t = torch.atan(torch.full((b,), sig0)) / torch.pi * 2
    dsd = {k[len("model.model."):]: v for k, v in sd.items() if k.startswith("model.model.")}
    rows = _ff_in_rows(dsd, xin, t, ci["cross_attn_cond"].cpu().float(), ci["global_cond"].cpu().float(), dc["num_heads"], 1)
    planted, s, peak = _plant_ff_overflow(dsd, rows)
    assert peak > FP16_MAX
    dit.load_state_dict(planted)
    got = check_fp16_range(model, steps=2, **kw)
    hid = [r for r in got["dit"] if (r["layer"], r["buffer"]) == (1, "ff_hidden")][0]
    print(f"  planted factor {s:g} (restated peak {peak:.4g}): {hid}; advice {got['advice']}")
    assert hid["over_fp16"] > 0 and any("bf16" in adv for adv in got["advice"]) and got["headroom"] <= 1.0
