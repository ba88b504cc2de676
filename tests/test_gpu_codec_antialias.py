"""Anti-aliased Oobleck codecs (``antialias_activation=True``) on the device, in all three operand formats.

The kernel alone (csrc/oobleck.hip aa_act_kernel through ``sat_oobleck_unit`` kind AA_ACT: the plan's own parameter packing and launcher)
against float64 on the same rounded input, through codec_units.gate_cl -- whole tensor, per (batch item, row), per 32 x 32 block -- at
codec_units.tol(fmt), inside NaN guard bands, pad channels bitwise zero.  Shapes, inputs and the reference: tests/codec_antialias_units.py;
that the gates reject zero padding, a dropped clamp, a missing gain, swapped phases, a dropped tap, a shifted window, the plain activation
and a neighbouring channel's alpha, and that the reference is the stand-in's operation: tests/test_codec_antialias_host.py.

The whole codec: decode, decode_T1 and encode of the three configs of tests/golden/make_golden_codec_antialias.py against the REFERENCE's
fp32 outputs (tests/golden/codec_antialias.npz; the reference ran with this project's stand-in for alias_free_torch) at the project's codec
gates -- 1.5e-2 (bf16) and 3.75e-3 (fp16) from ``CODEC`` in tests/test_gpu_models.py, 1e-5 (fp32) from ``TOL`` in
tests/test_gpu_codec_fp32.py -- and bit for bit under every workspace fill and behind a call of another length."""
import ctypes
import os
import sys

import pytest
import torch

import codec_antialias_units as au
import codec_units as cu
from util import NAN_BYTE, WORKSPACE_FILLS, assert_bit_equal, assert_close, guarded, rel_l2
from test_gpu_codec_fp32 import TOL as TOL_FP32
from test_gpu_models import CODEC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
import cases  # noqa: E402
import make_golden_codec_antialias as GA  # noqa: E402  (case table and seeds; does not import the reference)

pytestmark = pytest.mark.gpu

GATE = {"bf16": CODEC["bf16"][1], "fp16": CODEC["fp16"][1], "fp32": TOL_FP32}
FMTS = ["fp16", "bf16", "fp32"]
NAMES = sorted(GA.CONFIGS)


# ------------------------------------------------------------------------------------------------------------ the kernel alone
def _run_unit(dev, case, fmt):
    from stable_audio_tools import _hip
    d = _hip.SatOobleckUnitDesc()
    d.kind = _hip.OOBLECK_UNIT_AA_ACT
    d.gemm_dtype = cu.GEMM_CODE[fmt.name]
    d.activation = _hip.OOBLECK_ACT_SNAKE if case.act == "snake" else _hip.OOBLECK_ACT_ELU
    d.b, d.t_len, d.c_in, d.c_out = cu.BATCH, case.rows, case.c, case.c
    keep = [case.x_cl(fmt).contiguous().to(dev)]
    d.in_ = keep[0].data_ptr()
    if case.act == "snake":
        keep += [case.alpha.contiguous().to(dev), case.beta.contiguous().to(dev)]
        d.alpha, d.beta = keep[1].data_ptr(), keep[2].data_ptr()
    out = guarded((cu.BATCH, case.rows, cu.pad64(case.c)), fmt.dtype, dev, name="aa_act out_snk")
    d.out_snk = out.t.data_ptr()
    _hip.check(_hip.lib().sat_oobleck_unit(ctypes.byref(d), ctypes.sizeof(d), _hip.stream()))
    torch.cuda.synchronize()
    out.check().assert_written()
    assert torch.equal(keep[0].cpu(), case.x_cl(fmt)), "the input was written"
    return out.t.cpu()


@pytest.mark.parametrize("fmt", cu.ALL_FORMATS, ids=repr)
@pytest.mark.parametrize("p", au.CASES, ids=au.case_id)
def test_antialiased_activation_kernel(dev, p, fmt):
    """Rows 1 .. 11: both clamps, overlapping below 6 rows; one row less than, exactly and one more than a time tile, two tiles and three rows:
    the seams of the walk; 16 channels: 48 pad channels that stay bitwise zero; 192: three channel groups per row."""
    case = au.Case(p)
    got = _run_unit(dev, case, fmt)
    name = f"aa_act {au.case_id(p)}"
    cu.assert_pad_zero(name, got, case.c)
    cu.gate_cl(f"{name} {fmt}", got, au.reference(case, fmt), fmt)


def test_unit_refuses_in_place_and_missing_parameters(dev):
    from stable_audio_tools import _hip
    lib = _hip.lib()
    x = torch.zeros((2, 8, 64), dtype=torch.float16, device=dev)
    d = _hip.SatOobleckUnitDesc()
    d.kind, d.gemm_dtype, d.activation, d.b, d.t_len, d.c_in = _hip.OOBLECK_UNIT_AA_ACT, 3, _hip.OOBLECK_ACT_ELU, 2, 8, 64
    d.in_ = d.out_snk = x.data_ptr()
    assert lib.sat_oobleck_unit(ctypes.byref(d), ctypes.sizeof(d), _hip.stream()) == -1 and b"in place" in lib.sat_last_error()
    d.out_snk = torch.empty_like(x).data_ptr()
    d.activation = _hip.OOBLECK_ACT_SNAKE
    assert lib.sat_oobleck_unit(ctypes.byref(d), ctypes.sizeof(d), _hip.stream()) == -1 and b"alpha" in lib.sat_last_error()


# ------------------------------------------------------------------------------------------------------------ the whole codec
def _codec(name, dev, fmt):
    import stable_audio_tools as S
    from stable_audio_tools.models import _init
    with _init.skip_init():
        model = S.create_model_from_config(GA.model_config(name))
    model.decoder.load_state_dict(GA.synth_decoder_sd(name, model.decoder.state_dict()))
    model.encoder.load_state_dict(GA.synth_encoder_sd(name, model.encoder.state_dict()))
    return model.to(dev).eval().set_gemm_dtype(fmt)


@pytest.fixture(scope="module")
def golden():
    return cases.load("codec_antialias")


def _three(model, name, dev):
    z, z1, audio = GA.inputs(name)
    return {"decode": model.decode(z.to(dev)), "decode_T1": model.decode(z1.to(dev)), "encode": model.encoder(audio.to(dev))}


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("name", NAMES)
def test_decode_and_encode_vs_reference(dev, golden, name, fmt):
    model = _codec(name, dev, fmt)
    got = _three(model, name, dev)
    figures = {k: rel_l2(g, golden[f"{name}/{k}"]) for k, g in got.items()}
    print(f"\n[antialias {name}, {fmt}] rel-L2 vs the reference's fp32 output: " + ", ".join(f"{k} {v:.2e}" for k, v in figures.items()))
    for k, g in got.items():
        assert g.shape == golden[f"{name}/{k}"].shape
        assert_close(f"{name} {k} ({fmt})", g, golden[f"{name}/{k}"], GATE[fmt])


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("name", NAMES)
def test_outputs_depend_on_inputs_only(dev, golden, name, fmt):
    """The same bits under every workspace fill (the added launches read nothing they did not write; the pad channels of elu_narrow are
    written, not inherited), and for a T = 1 decode behind the T = 11 calls against a fresh module's."""
    model = _codec(name, dev, fmt)
    clean = _three(model, name, dev)
    for byte in WORKSPACE_FILLS:
        for part in (model.decoder, model.encoder):
            assert part._ws is not None and part._ws.dtype == torch.uint8
            part._ws.fill_(byte)
        ws_d, ws_e = model.decoder._ws, model.encoder._ws
        got = _three(model, name, dev)
        assert model.decoder._ws is ws_d and model.encoder._ws is ws_e          # the poisoned buffers are the ones that ran
        for k in got:
            if byte == NAN_BYTE:
                assert_close(f"{name} {k} on a NaN workspace ({fmt})", got[k], golden[f"{name}/{k}"], GATE[fmt])
            assert_bit_equal(f"{name} {k} on a workspace of 0x{byte:02X} bytes ({fmt})", got[k], clean[k])
    _, z1, _ = GA.inputs(name)
    fresh = _codec(name, dev, fmt).decode(z1.to(dev))
    assert_bit_equal(f"{name} decode_T1 of a fresh module vs behind the T = 11 calls ({fmt})", clean["decode_T1"], fresh)


@pytest.mark.parametrize("fmt", FMTS)
def test_final_tanh_and_iterate_batch_combine(dev, golden, fmt):
    name = "elu_narrow"
    model = _codec(name, dev, fmt)
    z, _, audio = GA.inputs(name)
    whole = model.decode(z.to(dev))
    assert_bit_equal(f"iterate_batch decode ({fmt})", model.decode(z.to(dev), iterate_batch=1), whole)
    assert_bit_equal(f"encode of item 0 alone ({fmt})", model.encoder(audio.to(dev)[:1].contiguous()), model.encoder(audio.to(dev))[:1])
    squashed = model.set_final_tanh(True).decode(z.to(dev))
    assert_close(f"tanh(decode) ({fmt})", squashed, torch.tanh(golden[f"{name}/decode"]), GATE[fmt])
    assert_close(f"tanh in the last epilogue vs tanh of the un-squashed audio ({fmt})", squashed, torch.tanh(whole), 1e-5)


# ------------------------------------------------------------------------------------------------------------ the option off
def _through_c_abi(mod, x, out_shape, t_len, fmt, set_zero):
    from stable_audio_tools import _hip
    from stable_audio_tools.models.autoencoders import _CODEC_GEMM_DTYPES
    lib = _hip.lib()
    cfg = _hip.SatOobleckCfg()
    cfg.is_decoder, cfg.io_channels, cfg.channels, cfg.latent_dim = int(mod._is_decoder), mod.io_channels, mod.channels, mod.latent_dim
    cfg.n_blocks = len(mod.strides)
    for i, (c, s) in enumerate(zip(mod.c_mults, mod.strides)):
        cfg.c_mults[i], cfg.strides[i] = c, s
    cfg.gemm_dtype = _CODEC_GEMM_DTYPES[fmt]
    opt = _hip.SatOobleckOptions()
    opt.activation = _hip.OOBLECK_ACT_SNAKE if mod.use_snake else _hip.OOBLECK_ACT_ELU
    opt.nearest_upsample = int(mod.use_nearest_upsample)
    plan = ctypes.c_void_p()
    _hip.check(lib.sat_oobleck_plan_create_ex(ctypes.byref(cfg), ctypes.byref(opt), ctypes.sizeof(opt), ctypes.byref(plan)))
    try:
        if set_zero:
            _hip.check(lib.sat_oobleck_plan_set_antialias(plan, 0))
        keep = [(n, t.detach().float().contiguous()) for n, t in mod.state_dict().items()]
        for n, t in keep:
            _hip.check(lib.sat_oobleck_plan_set_tensor(plan, n.encode(), _hip.ptr(t), t.numel()))
        _hip.check(lib.sat_oobleck_plan_finalize(plan, _hip.stream()))
        assert lib.sat_oobleck_plan_set_antialias(plan, 1) == -5 and b"finalized" in lib.sat_last_error()          # SAT_E_STATE
        assert lib.sat_oobleck_plan_set_antialias(plan, 0) == -5
        need = ctypes.c_size_t()
        _hip.check(lib.sat_oobleck_workspace_bytes(plan, x.shape[0], t_len, ctypes.byref(need)))
        ws = torch.empty(need.value, dtype=torch.uint8, device=x.device)
        out = torch.empty(out_shape, dtype=torch.float32, device=x.device)
        fn = lib.sat_oobleck_decode if mod._is_decoder else lib.sat_oobleck_encode
        _hip.check(fn(plan, _hip.ptr(x), _hip.ptr(out), x.shape[0], t_len, _hip.ptr(ws), ws.numel(), _hip.stream()))
        torch.cuda.synchronize()
        return out, need.value
    finally:
        lib.sat_oobleck_plan_destroy(plan)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("name", ["snake_128", "elu_narrow"])
def test_option_off_is_bit_identical_to_a_plan_that_never_heard_of_it(dev, name, fmt):
    """The same codec without antialias_activation: a plan on which sat_oobleck_plan_set_antialias(plan, 0) was called, a plan that never
    calls the setter and the Python module give the same bits; and the setter answers SAT_E_STATE once the plan is finalized."""
    from stable_audio_tools.models import _init
    from stable_audio_tools.models.autoencoders import OobleckDecoder, OobleckEncoder
    with _init.skip_init():
        dec = OobleckDecoder(**GA.decoder_kwargs(name, antialias=False))
        enc = OobleckEncoder(**GA.encoder_kwargs(name, antialias=False))
    ref_dec = GA.synth_decoder_sd(name, OobleckDecoder(**dict(GA.decoder_kwargs(name), allow_antialias=True)).state_dict())
    ref_enc = GA.synth_encoder_sd(name, OobleckEncoder(**dict(GA.encoder_kwargs(name), allow_antialias=True)).state_dict())
    dec.load_state_dict(GA.plain_sd(ref_dec))
    enc.load_state_dict(GA.plain_sd(ref_enc))
    dec, enc = dec.to(dev).set_gemm_dtype(fmt), enc.to(dev).set_gemm_dtype(fmt)
    z, _, audio = GA.inputs(name)
    z, audio = z.to(dev), audio.to(dev)
    d_mod, e_mod = dec(z), enc(audio)
    for mod, x, want, t_len in ((dec, z, d_mod, GA.T_LEN), (enc, audio, e_mod, GA.T_LEN)):
        never, need_never = _through_c_abi(mod, x, want.shape, t_len, fmt, set_zero=False)
        zero, need_zero = _through_c_abi(mod, x, want.shape, t_len, fmt, set_zero=True)
        assert need_never == need_zero
        assert_bit_equal(f"{name}: set_antialias(0) vs no call ({fmt})", zero, never)
        assert_bit_equal(f"{name}: the module vs the C ABI ({fmt})", want, never)
