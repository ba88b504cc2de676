"""The output of a plan call depends on weights and inputs only -- not on the bytes its workspace holds when the call starts, and not on what
earlier calls on the same plan and workspace computed (larger shapes, other conditioning, NaN inputs).

Every plan here (DiT, Oobleck codec, T5, RoBERTa) runs on memory it does not own for the length of a call: a caller-supplied grow-only
workspace (``_ws`` of the Python modules; _hip.plan_workspace hands the same tensor back while it is large enough) and plan-held grow-only
buffers (the DiT's ctx_buf, whose layout is recomputed from bf and lc at every sat_dit_prepare_context: a short context after a long one
lands at other offsets of memory that still holds the previous generation).  The kernels rely on zero pads of q / k / v^T and of the cross
K / V cache, on hole and spare-row fix-ups of the 96-channel heads, on GEMM tiles reading operand rows past M, on the K-split slabs, the MX
scale arrays, ln_part, qkv32 and the conv windows at sequence edges being either written by the call or never reaching an output.

The compute path has no atomics and the K-split reduce is bit-deterministic, so the property is checked EXACTLY: util.assert_bit_equal, no
tolerance; one ulp in one element fails.  Every test first asserts that two identical calls give identical bits, under a message of its own,
so that non-determinism is not mistaken for state dependence.

A new plan or launch route adds its row here: a line in FORWARD_ROWS (and FUSED_CASES / HISTORY_ROWS where it has a fused step or plan-held
state) for the DiT, else a test after the pattern of the encoder and codec tests below."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import cases  # noqa: E402
import dit_block_options_cases as BC  # noqa: E402
import dit_conv_ff_cases as CC  # noqa: E402
import dit_family  # noqa: E402
import dit_head_dim_cases as HC  # noqa: E402
import dit_head_width_cases as WC  # noqa: E402
import dit_options_cases as OC  # noqa: E402
import dit_patch_cases as PC  # noqa: E402
from dit_family_gpu import Harness  # noqa: E402
from stable_audio_tools import synthetic  # noqa: E402
from util import FORMATS, SUITE, WORKSPACE_FILLS, assert_bit_equal, guarded  # noqa: E402

pytestmark = pytest.mark.gpu

# the reduced DiT of dit_small.npz (cases.SMALL_DIT, seed-0 weights, cases.dit_inputs) in the shape of a family, so that the harness serves it
PLAIN = dit_family.Family(title="dit small", stem="dit_small", keys_file="", configs={"small": dict(cases.SMALL_DIT)},
                          cases={"cfg1_T64": ("small", 64, None, 1.0), "cfg7_T77": ("small", 77, None, 7.0)},
                          weights=lambda cfg_name, template_sd, seed=0: synthetic.synth_state_dict(template_sd, seed))
FAMILIES = {"plain": PLAIN, "options": OC.FAMILY, "head_dim": HC.FAMILY, "head_width": WC.FAMILY, "block_options": BC.FAMILY,
            "conv_ff": CC.FAMILY, "patch": PC.FAMILY}
HARNESS = {k: Harness(f) for k, f in FAMILIES.items()}
MIXED = ["fp16", "bf16", "fp16"]
SIGMA, CFG = 0.7, 7.0


def _configure(m, dtype, ln_fold=True, cross_fusion=True, formats=None):
    m.set_gemm_dtype(dtype).set_layernorm_fusion(ln_fold).set_cross_attention_fusion(cross_fusion).set_block_gemm_dtypes(formats)
    return m


def _restore(m):
    m.set_block_gemm_dtypes(None).set_gemm_dtype(SUITE.gemm_dtype).set_layernorm_fusion(True).set_cross_attention_fusion(True)


def _sync(out):
    torch.cuda.synchronize()
    return out


def check_poisoned_workspace(label, call, holder, ws_of=lambda h: h._ws):
    """The three steps of every workspace test: ``call()`` once; again, the same bits (determinism); then once per fill of
    util.WORKSPACE_FILLS on the holder's cached workspace, which must be the tensor that ran, the same bits again.  ``call`` returns a tensor
    or a tuple of tensors."""
    as_tuple = lambda v: v if isinstance(v, tuple) else (v,)
    first = as_tuple(_sync(call()))
    for i, (a, b) in enumerate(zip(as_tuple(_sync(call())), first)):
        assert_bit_equal(f"{label}: two identical calls differ (output {i}): the call is not deterministic, nothing below would mean anything", a, b)
        assert torch.isfinite(b.float()).all(), f"{label}: non-finite values in the un-poisoned output {i}"
    for byte in WORKSPACE_FILLS:
        ws = ws_of(holder)
        assert ws is not None and ws.dtype == torch.uint8 and ws.numel() > 0
        ws.fill_(byte)
        got = as_tuple(_sync(call()))
        assert ws_of(holder) is ws, f"{label}: the call replaced the workspace: the poisoned buffer is not the one that ran"
        for i, (a, b) in enumerate(zip(got, first)):
            assert_bit_equal(f"{label} on a workspace of 0x{byte:02X} bytes (output {i})", a, b)
    return first


# ---------------------------------------------------------------------------------------------- (a) DiT forward on a poisoned workspace
# One row per launch route: (family, case, formats, switches).  "suite" is SUITE.gemm_dtype.  The cases are the smallest of the family tables
# that reach the route; T = 77 behind the global row is S = 78, which leaves an M tail in every tile and 50 pad rows of q / k / v^T.
FORWARD_ROWS = [
    # plain 64-channel heads, CFG 1, and CFG 7 with null_from: every operand format (fp8: the MX scale arrays As / Hs, fp8-all: AOs as well)
    ("plain", "cfg1_T64", ["fp16", "bf16", "fp32x", "fp8", "fp8-all"], {}),
    ("plain", "cfg7_T77", ["fp16", "bf16", "fp32x", "fp8", "fp8-all"], {}),
    ("plain", "cfg1_T64", ["fp16", "bf16"], dict(ln_fold=False)),
    ("plain", "cfg7_T77", ["fp16", "bf16"], dict(ln_fold=False)),
    ("plain", "cfg1_T64", ["fp16", "bf16"], dict(cross_fusion=False)),
    ("plain", "cfg7_T77", ["fp16", "bf16"], dict(cross_fusion=False)),
    # per-block formats: the second context image ce_other
    ("plain", "cfg1_T64", ["fp16"], dict(formats=MIXED)),
    ("plain", "cfg7_T77", ["fp16"], dict(formats=MIXED)),
    ("options", "qk_adaln_cfg7_T77", ["suite"], {}),                              # adaLN
    ("options", "sin_prepend_P3_cfg7_T77", ["suite", "fp32x"], {}),               # prepend rows, P = 3
    ("options", "qk_concat_cfg7_T77", ["suite"], {}),                             # input concat
    ("options", "abs_P3_cfg1_T77", ["suite"], {}),                                # absolute positions
    ("head_dim", "hd128_wide_cfg7_T77", ["fp16", "bf16"], {}),                    # staged route, 128-wide, GQA 2:1
    ("head_width", "hd96_qk_concat_cfg7_T77", ["fp16", "bf16", "fp32x"], {}),     # staged route, 96-wide: padded K rows, hole fix-ups
    ("head_width", "hd32_patch2_cfg7_T78", ["fp16", "bf16", "fp32x"], {}),        # staged route, 32-wide (128-key tile) with patch 2
    ("block_options", "all3_adaln_cfg7_T77", ["suite", "fp32x"], {}),             # conformer + norm-free + SiLU under adaLN
    ("block_options", "conf_prepend_cfg7_T77", ["suite"], {}),                    # conformer window across prepend / global / frame rows
    ("conv_ff", "conv_silu_k5_nobias_cfg7_T77", ["suite", "fp32x"], {}),          # both convs, k = 5 (fp32x: f32_col)
    ("conv_ff", "conv_prepend_cfg7_T77", ["suite"], {}),                          # conv feed-forward across prepend rows
    ("patch", "p8_c8_cfg7_T72", ["suite"], {}),                                   # patch 8: 9 tokens
    ("patch", "p3_cfg1_T63", ["suite"], {}),                                      # patch 3
]


def _row_id(fam, case, dtype, sw):
    tags = [t for t, on in (("noln", sw.get("ln_fold") is False), ("nofuse", sw.get("cross_fusion") is False), ("mixed", bool(sw.get("formats")))) if on]
    return "-".join([case, dtype] + tags)


FORWARD_PARAMS = [pytest.param(fam, case, dtype, sw, id=_row_id(fam, case, dtype, sw)) for fam, case, dtypes, sw in FORWARD_ROWS for dtype in dtypes]


@pytest.mark.parametrize("fam,case,dtype,switches", FORWARD_PARAMS)
def test_dit_forward_ignores_workspace_contents(dev, fam, case, dtype, switches):
    h = HARNESS[fam]
    assert h.family.cases[case][1] <= 78
    m = h.model(h.family.cases[case][0], dev)
    x, t, kw = h.inputs(case, dev)
    try:
        _configure(m, SUITE.gemm_dtype if dtype == "suite" else dtype, **switches)
        check_poisoned_workspace(f"{case} forward ({_row_id(fam, case, dtype, switches)})", lambda: m(x, t, **kw), m)
    finally:
        _restore(m)


# ----------------------------------------------------------------------------------------- (b) fused sampler step on a poisoned workspace
FUSED_CASES = [("plain", "cfg7_T77"), ("head_width", "hd96_qk_concat_cfg7_T77"), ("patch", "p2_prepend_cfg7_T78"), ("conv_ff", "conv_silu_k5_nobias_cfg7_T77")]


@pytest.mark.parametrize("fam,case", FUSED_CASES, ids=[c for _, c in FUSED_CASES])
def test_fused_denoise_ignores_workspace_contents(dev, fam, case):
    """prepare_generation + denoise (sat_dit_denoise_cfg) at sigma 0.7 and CFG 7, in the suite's format."""
    h = HARNESS[fam]
    m = h.model(h.family.cases[case][0], dev)
    x, _, kw = h.inputs(case, dev)
    cond = dict(prepend_cond=kw["prepend_cond"], input_concat_cond=kw["input_concat_cond"])

    def step():
        m.prepare_generation(kw["cross_attn_cond"], kw["global_embed"], CFG, **cond)
        return m.denoise(x, SIGMA, cfg_scale=CFG)

    try:
        _configure(m, SUITE.gemm_dtype)
        check_poisoned_workspace(f"{case} fused denoise ({SUITE.gemm_dtype})", step, m)
    finally:
        _restore(m)


# --------------------------------------------------------------------------------------------- (c) history independence of the DiT plan
# Module H runs call A, then B; module F (same config, same weights) runs B only.  A dirties everything B later reads as padding: three
# prompts at CFG 7 (bf 6, null_from 3) against B's two sequences at CFG 1; the longest T the plan admits against T <= 78; 130 context tokens
# against 7 (the pad-key tails of kc / vct and the recomputed ctx_buf offsets fall on A's data); prepend tokens and a longer concat signal
# where the config takes them, none (prepend) in B.  In the second variant A's x, cross_attn_cond and global_embed are all NaN: a NaN
# forward is no fault, and it fills every buffer a generation writes -- ctx_buf cannot be poisoned from Python in another way.
HIST_MAX_SEQ = 512           # max_seq_len of the two modules: A runs at the largest T <= it that holds whole patches
HISTORY_ROWS = [
    ("plain", "cfg1_T64", ["fp16", "bf16", "fp32x", "fp8"], None),
    ("plain", "cfg7_T77", ["fp16"], MIXED),                                    # per-block formats: ce_other
    ("head_width", "hd96_qk_concat_cfg7_T77", ["fp16", "bf16"], None),         # staged: o_kv128
    ("head_width", "hd32_patch2_cfg7_T78", ["fp16", "bf16"], None),
    ("head_dim", "hd128_wide_cfg7_T77", ["fp16", "bf16"], None),
    ("block_options", "conf_prepend_cfg7_T77", ["suite"], None),
    ("conv_ff", "conv_prepend_cfg7_T77", ["suite"], None),
    ("options", "sin_prepend_P3_cfg7_T77", ["suite"], None),                   # prepend tokens in A, none in B
    ("options", "qk_concat_cfg7_T77", ["suite"], None),                        # a longer concat signal in A
]
HISTORY_PARAMS = [pytest.param(fam, case, dtype, formats, id="-".join([case, dtype] + (["mixed"] if formats else [])))
                  for fam, case, dtypes, formats in HISTORY_ROWS for dtype in dtypes]


def _fresh_dit(family, cfg_name, dev):
    from stable_audio_tools.models import _init
    from stable_audio_tools.models.dit import DiffusionTransformer
    with _init.skip_init():
        m = DiffusionTransformer(**family.configs[cfg_name], **family.product_kwargs, max_seq_len=HIST_MAX_SEQ)
    m.load_state_dict(family.weights(cfg_name, m.state_dict(), 0), strict=True)
    return m.to(dev).eval()


def _history_call(family, cfg_name, dev, batch, t_len, lc, prepend, cfg_scale, seed, nan=False):
    """(x, t, forward kwargs) for a config, by the scheme of dit_family.case_inputs."""
    cfg = family.configs[cfg_name]
    x = synthetic.synth_input("x", (batch, cfg["io_channels"], t_len), seed)
    c = synthetic.synth_input("c", (batch, lc, cfg["cond_token_dim"]), seed + 1)
    g = synthetic.synth_input("g", (batch, 96), seed + 2)
    t = (torch.arange(batch, dtype=torch.float32) + 1) / (batch + 1)
    if nan:
        x, c, g = (torch.full_like(v, float("nan")) for v in (x, c, g))
    cat = None
    if cfg.get("input_concat_dim"):
        shape, cat_seed = family.concat(t_len)
        cat = synthetic.synth_input("concat", (batch,) + shape, cat_seed + seed)
    pre = synthetic.synth_input("prepend", (batch, prepend, dit_family.PREPEND_DIM), 300 + prepend) if prepend and cfg.get("prepend_cond_dim") else None
    to = lambda v: None if v is None else v.to(dev)
    return to(x), to(t), dict(cross_attn_cond=to(c), global_embed=to(g), prepend_cond=to(pre), input_concat_cond=to(cat), cfg_scale=cfg_scale)


@pytest.mark.parametrize("fam,case,dtype,formats", HISTORY_PARAMS)
def test_dit_plan_forgets_earlier_calls(dev, fam, case, dtype, formats):
    family = FAMILIES[fam]
    cfg_name, t_b = family.cases[case][:2]
    patch = family.configs[cfg_name].get("patch_size", 1)
    t_a = HIST_MAX_SEQ // patch * patch
    dtype = SUITE.gemm_dtype if dtype == "suite" else dtype
    fresh, used = (_configure(_fresh_dit(family, cfg_name, dev), dtype, formats=formats) for _ in range(2))
    xb, tb, kwb = _history_call(family, cfg_name, dev, batch=2, t_len=t_b, lc=7, prepend=0, cfg_scale=1.0, seed=1)
    run_b = lambda m: _sync(m(xb, tb, **kwb))
    want = run_b(fresh)
    assert torch.isfinite(want).all()
    assert_bit_equal(f"{case} ({dtype}): two identical calls on the fresh module differ: not deterministic", run_b(fresh), want)
    for variant, nan in (("a larger call", False), ("an all-NaN larger call", True)):
        xa, ta, kwa = _history_call(family, cfg_name, dev, batch=3, t_len=t_a, lc=130, prepend=5, cfg_scale=CFG, seed=11, nan=nan)
        out_a = _sync(used(xa, ta, **kwa))
        assert bool(torch.isnan(out_a).all()) if nan else bool(torch.isfinite(out_a).all()), f"{case} ({dtype}): call A ({variant}) gave unexpected values"
        ws = used._ws
        got = run_b(used)
        assert used._ws is ws and ws.numel() > fresh._ws.numel()          # B ran inside the workspace A left behind
        assert_bit_equal(f"{case} ({dtype}) after {variant} on the same plan and workspace, against a fresh module", got, want)
        key = used._ctx_key
        again = run_b(used)          # the same tensors: prepare_context returns early, the cached context serves
        assert used._ctx_key is key
        assert_bit_equal(f"{case} ({dtype}) after {variant}, second run on the cached context", again, want)


# ------------------------------------------------------------------------------------------------------------------ (d) text encoders
def _t5(dev):
    from stable_audio_tools.models.conditioners import T5Conditioner
    from test_t5 import _hf_encoder
    model = _hf_encoder("t5", 3)
    conds = []
    for _ in range(2):
        c = T5Conditioner(model.config.d_model, "t5-base").load_encoder(model.state_dict(), model.config)
        c.set_device(dev)
        conds.append(c)
    return model.config, conds


def _t5_batch(vocab, b, length, seed):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, vocab, (b, length), generator=g)
    mask = torch.ones(b, length, dtype=torch.long)
    if b > 1:          # padded prompts, as tests/test_t5.py lays them out
        mask[1, max(1, length // 3):] = 0
        mask[2, 1:] = 0
    return ids * mask, mask


def test_t5_encoder_ignores_workspace_contents_and_history(dev):
    cfg, (fresh, used) = _t5(dev)
    ids, mask = _t5_batch(cfg.vocab_size, 1, 19, 5)
    want = check_poisoned_workspace("T5 encoder, length 19", lambda: fresh.encode_ids(ids, mask)[0], fresh, lambda c: c.__dict__["_ws"])[0]
    long_ids, long_mask = _t5_batch(cfg.vocab_size, 3, 128, 6)
    # NaN-free but maximal: the last id of the vocabulary in every position, no position masked
    for what, (i, k) in (("ordinary ids", (long_ids, long_mask)), ("the largest id everywhere under an all-ones mask", (torch.full((3, 128), cfg.vocab_size - 1), torch.ones(3, 128, dtype=torch.long)))):
        assert torch.isfinite(_sync(used.encode_ids(i, k)[0])).all()
        ws = used.__dict__["_ws"]
        got = _sync(used.encode_ids(ids, mask)[0])
        assert used.__dict__["_ws"] is ws and ws.numel() > fresh.__dict__["_ws"].numel()
        assert_bit_equal(f"T5 encoder, length 19 after batch 3 at length 128 ({what}), against a fresh module", got, want)


def test_roberta_encoder_ignores_workspace_contents_and_history(dev):
    from stable_audio_tools.models.conditioners import RobertaEncoderPlan, roberta_encoder_tensors
    from test_clap_text import ENCODER_CASES, SHAPES, _batch, _hf_roberta
    layers = lambda c: c[3] if c[3] >= 0 else SHAPES[c[0]]["num_hidden_layers"] + 1 + c[3]          # hidden_states[ix] is behind this many layers
    shape, length, real, ix, with_proj = min(ENCODER_CASES, key=lambda c: (SHAPES[c[0]]["hidden_size"] * c[1], layers(c)))
    assert (shape, length, ix, with_proj) == ("reduced", 24, 1, True)
    model = _hf_roberta(shape, 3)
    cfg = model.config
    ix = layers((shape, length, real, ix))
    g = torch.Generator().manual_seed(7)
    proj = (torch.randn(192, cfg.hidden_size, generator=g) / cfg.hidden_size ** 0.5, 0.5 * torch.randn(192, generator=g))
    sd, meta = roberta_encoder_tensors({k: v.float() for k, v in model.state_dict().items()}, cfg)
    fresh, used = (RobertaEncoderPlan(sd, meta, ix, dev, proj) for _ in range(2))
    try:
        ids, mask = _batch(shape, length, real, 5)
        want = check_poisoned_workspace(f"RoBERTa encoder ({shape}, length {length})", lambda: fresh.encode(ids, mask), fresh)[0]
        longest = cfg.max_position_embeddings - 2          # the longest sequence the position table admits
        long_ids, long_mask = _batch(shape, longest, (longest, 19, 2), 6)
        for what, (i, k) in (("ordinary ids", (long_ids, long_mask)), ("the largest id everywhere under an all-ones mask", (torch.full((3, longest), cfg.vocab_size - 1), torch.ones(3, longest, dtype=torch.long)))):
            assert torch.isfinite(_sync(used.encode(i, k))).all()
            ws = used._ws
            got = _sync(used.encode(ids, mask))
            assert used._ws is ws and ws.numel() > fresh._ws.numel()
            assert_bit_equal(f"RoBERTa encoder, length {length} after batch 3 at length {longest} ({what}), against a fresh module", got, want)
    finally:
        fresh.close()
        used.close()


# ---------------------------------------------------------------------------------------------------------------------------- (e) codec
@pytest.mark.parametrize("fmt", ["fp16", "bf16", "fp32"])
@pytest.mark.parametrize("name", ["narrow_all", "small_vae"])
def test_codec_forgets_longer_calls(dev, name, fmt):
    """Decode at the golden's T, then at T = 1; encode of the long clip, then of the shortest clip the strides admit (one latent frame): the
    short calls give the bits of a fresh module.  narrow_all pads every tensor of the workspace; small_vae is cases.SMALL_VAE, 16 channels."""
    import make_golden_codec_options as GO
    from test_gpu_codec_options import _codec, _small_vae
    if name == "narrow_all":
        fresh, used = (_codec(name, dev, fmt) for _ in range(2))
        z, z1, audio = GO.inputs(name)
        ratio = GO.ratio(name)
    else:
        fresh, used = (_small_vae(dev, fmt) for _ in range(2))
        z = synthetic.synth_input("z", (2, 64, 9), 7)
        audio = synthetic.synth_input("a", (2, 2, 2048 * 5), 8, 0.3)
        z1, ratio = z[..., :1].contiguous(), 2048
    a1 = audio[..., :ratio].contiguous()
    z, z1, audio, a1 = (v.to(dev) for v in (z, z1, audio, a1))
    want_d, want_e = _sync(fresh.decoder(z1)), _sync(fresh.encoder(a1))
    assert torch.isfinite(want_d).all() and torch.isfinite(want_e).all() and want_e.shape[-1] == 1
    assert_bit_equal(f"{name} decode_T1 twice ({fmt}): not deterministic", fresh.decoder(z1), want_d)
    assert_bit_equal(f"{name} encode of one frame twice ({fmt}): not deterministic", fresh.encoder(a1), want_e)
    used.decoder(z)
    used.encoder(audio)
    ws_d, ws_e = used.decoder._ws, used.encoder._ws
    got_d, got_e = _sync(used.decoder(z1)), _sync(used.encoder(a1))
    assert used.decoder._ws is ws_d and used.encoder._ws is ws_e
    assert ws_d.numel() > fresh.decoder._ws.numel() and ws_e.numel() > fresh.encoder._ws.numel()
    assert_bit_equal(f"{name} decode at T = 1 after T = {z.shape[-1]} ({fmt}), against a fresh module", got_d, want_d)
    assert_bit_equal(f"{name} encode of one frame after {audio.shape[-1] // ratio} frames ({fmt}), against a fresh module", got_e, want_e)


# ------------------------------------------------------------------------------------------------ (f) the K-split slabs, kernel level
# The small DiT configs never take the split: without this the slab has no coverage for stale contents.
SPLIT_SHAPE = (257, 768, 1536)


def _split_operands(dev, fmt, seed):
    from test_gpu_kernels import _rand
    m, n, k = SPLIT_SHAPE
    a = _rand((m, k), seed).to(fmt.dtype)
    w = (_rand((n, k), seed + 1) * 0.05 + torch.linspace(-0.02, 0.03, n)[:, None]).to(fmt.dtype)
    return a.to(dev), w.to(dev), _rand((n,), seed + 2).to(dev), _rand((m, n), seed + 3, 2.0) + 0.3


def _slab_fills(ws):
    """The slab as the allocator left it, the same again (determinism), then every fill."""
    yield "as allocated", None
    yield "as the first call left it", None
    for byte in WORKSPACE_FILLS:
        ws.fill_(byte)
        yield f"filled with 0x{byte:02X} bytes", byte


@pytest.mark.parametrize("fmt", FORMATS, ids=repr)
def test_k_split_gemm_ignores_slab_contents(dev, fmt):
    from stable_audio_tools import _hip
    from test_gpu_kernels import SPLIT, _split_ws
    lib = _hip.lib()
    m, n, k = SPLIT_SHAPE
    a, w, bias, c0 = _split_operands(dev, fmt, 5)
    ws, ws_bytes = _split_ws(dev, m, n, k, SPLIT)
    assert ws is not None and ws_bytes == ws.numel() > 0
    first = None
    for what, _ in _slab_fills(ws):
        cg = guarded((m, n), torch.float32, dev, init=c0, name="c")
        _hip.check(fmt.fn(lib, "sat_gemm_bf16_f32_ws")(_hip.ptr(a), _hip.ptr(w), _hip.ptr(bias), _hip.ptr(cg.t), m, n, k, 1, SPLIT, _hip.ptr(ws), ws_bytes,
                                                       _hip.stream()))
        cg.check().assert_written()
        if first is None:
            first = cg.t.clone()
        assert_bit_equal(f"forced K-split GEMM {SPLIT_SHAPE} ({fmt}), slab {what}", cg.t, first)


@pytest.mark.parametrize("fmt", FORMATS, ids=repr)
def test_k_split_layernorm_producer_ignores_slab_contents(dev, fmt):
    from stable_audio_tools import _hip
    from test_gpu_kernels import SPLIT, _split_ws
    lib = _hip.lib()
    m, d, k = SPLIT_SHAPE
    a, w, bias, x0 = _split_operands(dev, fmt, 40)
    ws, ws_bytes = _split_ws(dev, m, d, k, SPLIT)
    assert ws is not None and ws_bytes == ws.numel() > 0
    first = None
    for what, _ in _slab_fills(ws):
        cg = guarded((m, d), torch.float32, dev, init=x0, name="c")
        xg, pg = guarded((m, d), fmt.dtype, dev, name="xb"), guarded((m, d // 64, 2), torch.float32, dev, name="ln_part", pitch=2 * (d // 64))
        _hip.check(fmt.fn(lib, "sat_gemm_resid_ln_bf16_ws")(_hip.ptr(a), _hip.ptr(w), _hip.ptr(bias), _hip.ptr(cg.t), _hip.ptr(xg.t), _hip.ptr(pg.t), m, d, k,
                                                            SPLIT, _hip.ptr(ws), ws_bytes, _hip.stream()))
        for g_ in (cg, xg, pg):
            g_.check().assert_written()
        if first is None:
            first = tuple(g_.t.clone() for g_ in (cg, xg, pg))
        for label, g_, ref in zip(("c", "xb", "ln_part"), (cg, xg, pg), first):
            assert_bit_equal(f"forced K-split LayerNorm producer {SPLIT_SHAPE} ({fmt}), {label}, slab {what}", g_.t, ref)
