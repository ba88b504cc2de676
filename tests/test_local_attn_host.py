"""The local-attention codec without a GPU: the weight permutations that replace the two rearranges, the goldens and their recorded gate
figures, the float64 restatement the GPU tests trust (tests/local_attn_units.py) against the reference's golden of case C and three
deliberately wrong variants of it against the per-row gate, the factories, and the construction-time refusals."""
import copy
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

from util import assert_close_sliced, rel_l2, slice_errors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
import local_attn_cases as LC  # noqa: E402
import local_attn_units as LU  # noqa: E402

from stable_audio_tools.models import local_attention as LA  # noqa: E402
from stable_audio_tools.models.autoencoders import (AudioAutoencoder, OobleckDecoder, create_autoencoder_from_config,  # noqa: E402
                                                    create_decoder_from_config, create_encoder_from_config)


@pytest.fixture(scope="module")
def golden():
    return LC.load()


# ------------------------------------------------------------------------------------------------------------ the weight permutations
@pytest.mark.parametrize("r", [1, 2, 3, 4])
def test_weight_permutations_replace_the_rearranges(r):
    """numpy: rows [b n r, C] read as [b n, r C] times the permuted project_down.weight = rearrange + the Linear; the permuted project_up.weight's
    output [b n, r C] read as [b n r, C] = the Linear + rearrange.  The permutations are written out index by index, as the plan's kernel has
    them (csrc/local_attn_plan.hip: out[j * C + c] = in[c * r + j]), and equal the package's permute_project_down / permute_project_up."""
    from einops import rearrange
    rng = np.random.default_rng(r)
    b, n, c = 2, 5, 6
    x = rng.standard_normal((b, n * r, c))
    w_down = rng.standard_normal((c, c * r))
    perm = np.empty_like(w_down)
    for j in range(r):
        for ch in range(c):
            perm[:, j * c + ch] = w_down[:, ch * r + j]
    want = rearrange(x, "b (n r) c -> b n (c r)", r=r) @ w_down.T
    got = x.reshape(b * n, r * c) @ perm.T          # no data moves: the same buffer, read with rows r times as long
    np.testing.assert_allclose(got.reshape(b, n, c), want, rtol=0, atol=1e-12)
    np.testing.assert_array_equal(LA.permute_project_down(torch.from_numpy(w_down), r).numpy(), perm)
    if r > 1:
        assert not np.allclose(x.reshape(b * n, r * c) @ w_down.T, want.reshape(b * n, c))          # the un-permuted weight is another map

    y = rng.standard_normal((b, n, c))
    w_up = rng.standard_normal((c * r, c))
    perm = np.empty_like(w_up)
    for j in range(r):
        for ch in range(c):
            perm[j * c + ch, :] = w_up[ch * r + j, :]
    want = rearrange(y @ w_up.T, "b n (c r) -> b (n r) c", r=r)
    got = (y.reshape(b * n, c) @ perm.T).reshape(b, n * r, c)
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)
    np.testing.assert_array_equal(LA.permute_project_up(torch.from_numpy(w_up), r).numpy(), perm)


# --------------------------------------------------------------------------------------------------------------- goldens and their gates
def test_goldens_load_and_recorded_figures_hold(golden):
    entries = LC.entries()
    assert set(LC.R16) == set(LC.F64) == set(entries)
    for entry, fmts in entries.items():
        want = golden[entry]
        assert want.dtype == torch.float32 and bool(torch.isfinite(want).all())
        assert golden[f"{entry}__f64"].dtype == torch.float64
        for fmt in ("fp16", "bf16"):
            figure = rel_l2(golden[f"{entry}__r16_{fmt}"], want)
            assert math.isfinite(figure) and abs(figure - LC.R16[entry][fmt]) <= 2e-3 * figure, (entry, fmt, figure, LC.R16[entry][fmt])
            if LC.runs(entry, fmt):
                assert figure < LC.R16_LIMIT, (entry, fmt, figure)
            # the yardstick itself passes the per-row gate it sets
            assert float(slice_errors(golden[f"{entry}__r16_{fmt}"], want, (0, 2)).max()) <= LC.ROW_FACTOR * 2.0 * figure
        f64 = golden[f"{entry}__f64"]
        figure = float((want.double() - f64).norm() / f64.norm())
        assert abs(figure - LC.F64[entry]) <= 2e-3 * figure and figure < 1e-4, (entry, figure, LC.F64[entry])
        assert float(slice_errors(want, f64, (0, 2)).max()) <= LC.ROW_FACTOR * 4.0 * figure
    # what may be dropped: at most one of A - C in bf16, nothing in fp16 or fp32 (B's fp32 runs as B32: local_attn_cases.py)
    assert all(fmt == "bf16" and entry[0] in "ABC" for entry, fmt in LC.DROPPED)
    assert len({entry.split("_")[0] for entry, _ in LC.DROPPED}) <= 1
    for name in ("A", "B32", "C"):
        assert entries[f"{name}_enc"] == entries[f"{name}_dec"] == LC.FORMATS
    assert entries["B_enc"] == ("fp16", "bf16")
    # shapes of the issue's cases: 264 latents from 1056 samples, 130 from 1040, 11 from 33
    assert golden["A_enc"].shape == (2, 8, 264) and golden["A_dec"].shape == (2, 2, 1056)
    assert golden["B_enc"].shape == (1, 6, 130) and golden["B_dec"].shape == (1, 1, 1040)
    assert golden["C_enc"].shape == (2, 4, 11) and golden["C_dec"].shape == (2, 2, 33)
    assert golden["D_encode"].shape == golden["D_encode_chunked"].shape == (2, 4, 100)
    assert golden["D_decode"].shape == golden["D_decode_chunked"].shape == (2, 2, 800)


def test_state_dict_keys_equal_the_reference():
    want = json.load(open(LC.KEYS_PATH))
    for name, (enc_kw, dec_kw, _, _, _) in LC.CODECS.items():
        for side, m in (("enc", LA.TransformerEncoder1D(**enc_kw)), ("dec", LA.TransformerDecoder1D(**dec_kw))):
            assert {k: list(v.shape) for k, v in m.state_dict().items()} == want[f"{name}_{side}"], f"{name}_{side}"
            m.load_state_dict(LC.weights(m.state_dict()), strict=True)
    model = create_autoencoder_from_config(copy.deepcopy(LC.D_CONFIG))
    assert {k: list(v.shape) for k, v in model.state_dict().items()} == want["D"]


# --------------------------------------------------------------------------------------------------------------- the float64 restatement
def _case_c(side):
    enc_kw, dec_kw = LC.CODECS["C"][:2]
    kw = enc_kw if side == "enc" else dec_kw
    m = LA.TransformerEncoder1D(**kw) if side == "enc" else LA.TransformerDecoder1D(**kw)
    sd = {k: v.double() for k, v in LC.weights(m.state_dict()).items()}
    fn = LU.encoder if side == "enc" else LU.decoder
    return lambda x, wrong=None: fn(x.double(), sd, kw["heads"][0], kw["depths"][0], kw["ratios"][0], kw["local_attn_window_size"], wrong)


def test_restatement_agrees_with_the_reference(golden):
    """Case C, encoder and decoder: 1e-6 against the reference's fp32 output (as the issue sets it), 1e-9 against its float64 output"""
    x, z = LC.audio("C"), golden["C_enc"]
    for entry, got in (("C_enc", _case_c("enc")(x)), ("C_dec", _case_c("dec")(z))):
        assert rel_l2(got, golden[entry]) <= 1e-6, (entry, rel_l2(got, golden[entry]))
        f64 = golden[f"{entry}__f64"]
        assert float((got - f64).norm() / f64.norm()) <= 1e-9, entry
        assert_close_sliced(f"{entry} restated, per time step", got, golden[entry], LC.ROW_FACTOR * LC.gate(entry, "fp32"), (0, 2))


@pytest.mark.parametrize("wrong", LU.WRONG)
def test_wrong_variants_are_rejected_by_the_row_gate(golden, wrong):
    """Each mistake fails the per-row gate of case C in EVERY format, the widest (bf16) included"""
    got = _case_c("enc")(LC.audio("C"), wrong)
    for fmt in LC.FORMATS:
        with pytest.raises(AssertionError, match="slice"):
            assert_close_sliced(f"C_enc with {wrong}", got, golden["C_enc"], LC.ROW_FACTOR * LC.gate("C_enc", fmt), (0, 2))


# ------------------------------------------------------------------------------------------------------------ factories and refusals
def test_factories_build_local_attn():
    enc_kw, dec_kw = LC.CODECS["A"][:2]
    enc = create_encoder_from_config({"type": "local_attn", "config": copy.deepcopy(enc_kw)})
    dec = create_decoder_from_config({"type": "local_attn", "config": copy.deepcopy(dec_kw), "requires_grad": False})
    assert isinstance(enc, LA.TransformerEncoder1D) and isinstance(dec, LA.TransformerDecoder1D)
    assert enc.ratio == dec.ratio == 4 and not any(p.requires_grad for p in dec.parameters())
    assert enc.stage_rows(1056) == [1056, 528] and dec.stage_rows(264) == [528, 1056]
    model = create_autoencoder_from_config(copy.deepcopy(LC.D_CONFIG))
    assert isinstance(model, AudioAutoencoder) and isinstance(model.encoder, LA.TransformerEncoder1D)
    model.set_gemm_dtype("bf16")
    assert model.encoder.gemm_dtype == model.decoder.gemm_dtype == "bf16"
    # a mixed codec is built as well (README, "Local-attention configurations")
    cfg = copy.deepcopy(LC.D_CONFIG)
    cfg["model"]["decoder"] = {"type": "oobleck", "config": dict(out_channels=2, channels=16, c_mults=[1, 2], strides=[2, 4], latent_dim=4,
                                                                 use_snake=True, final_tanh=False)}
    mixed = create_autoencoder_from_config(cfg)
    assert isinstance(mixed.encoder, LA.TransformerEncoder1D) and isinstance(mixed.decoder, OobleckDecoder)
    with pytest.raises(NotImplementedError, match="outside this build's hot path"):
        create_encoder_from_config({"type": "dac", "config": {}})
    # no eager or CPU forward
    from stable_audio_tools import _hip
    with pytest.raises(_hip.SatError, match="HIP device"):
        enc(torch.zeros(1, 2, 1056))
    with pytest.raises(RuntimeError, match="no standalone forward"):
        enc.layers[0](torch.zeros(1, 1056, 128))


def check_construction_refusals():
    enc_kw = LC.CODECS["A"][0]
    E = lambda **kw: LA.TransformerEncoder1D(**dict(copy.deepcopy(enc_kw), **kw))
    D = lambda **kw: LA.TransformerDecoder1D(**dict(copy.deepcopy(LC.CODECS["A"][1]), **kw))
    # NATTEN's rule; the reference's default window of 64 is such a value
    for bad in (64, 8, 1, 0, -3):
        with pytest.raises(ValueError, match="odd kernel sizes greater than 1"):
            E(local_attn_window_size=bad)
        with pytest.raises(ValueError, match="odd kernel sizes greater than 1"):
            D(local_attn_window_size=bad)
    with pytest.raises(ValueError, match="odd kernel sizes greater than 1"):
        LA.TransformerEncoder1D(2, 8, embed_dims=[128], heads=[2], depths=[1], ratios=[2])          # the default window
    for kw, what in ((dict(cond_dim=64), "cond_dim"), (dict(cross_attn_cond_dim=64), "cross_attn_cond_dim"), (dict(causal=True), "causal")):
        with pytest.raises(NotImplementedError, match=what):
            E(**kw)
        with pytest.raises(NotImplementedError, match=what):
            D(**kw)
    with pytest.raises(NotImplementedError, match="32, 64, 96 and 128"):
        E(heads=[8, 4])                       # 128 // 8 = 16
    with pytest.raises(NotImplementedError, match="32, 64, 96 and 128"):
        E(embed_dims=[128, 512], heads=[4, 2])          # 256-channel heads
    with pytest.raises(NotImplementedError, match="multiple of 128"):
        E(embed_dims=[192, 256], heads=[2, 4])          # 96-channel heads, but 3 * 192 is no multiple of 128
    with pytest.raises(NotImplementedError, match="multiple of 64"):
        E(ff_mult=0.3)                                   # int(128 * 0.3) = 38
    with pytest.raises(NotImplementedError, match="in_channels"):
        E(in_channels=130)
    with pytest.raises(NotImplementedError, match="128-channel heads"):
        E(embed_dims=[128, 256], heads=[1, 4]).set_gemm_dtype("fp32")
    with pytest.raises(NotImplementedError, match="local_attn"):
        E().activation_range_report(True)
    assert E().activation_range_report(False) == []
    model = create_autoencoder_from_config(copy.deepcopy(LC.D_CONFIG))
    with pytest.raises(NotImplementedError, match="local_attn"):
        model.activation_range_report(True)
    # the length and window refusals need no device either: they come before the plan
    enc = E()
    with pytest.raises(ValueError, match="multiple of the product of the ratios"):
        enc(torch.zeros(1, 2, 1054))
    with pytest.raises(ValueError, match="fewer than local_attn_window_size"):
        enc(torch.zeros(1, 2, 12))
    assert enc._ws is None and enc._plan is None


def test_construction_refusals():
    check_construction_refusals()


def test_library_refuses_bad_configs_without_gpu():
    """sat_local_attn_plan_create answers SAT_E_* with a message instead of building a plan it cannot run"""
    import ctypes
    from stable_audio_tools import _hip
    lib = _hip.lib()

    def cfg(**kw):
        c = _hip.SatLocalAttnCfg()
        c.is_decoder, c.in_channels, c.out_channels, c.n_stages, c.window, c.gemm_dtype = 0, 2, 8, 1, 7, 3
        c.embed_dims[0], c.heads[0], c.depths[0], c.ratios[0], c.ff_inner[0] = 128, 2, 1, 2, 256
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(c, k)[0] = v[0]
            else:
                setattr(c, k, v)
        return c

    plan = ctypes.c_void_p()
    ok = cfg()
    assert lib.sat_local_attn_plan_create(ctypes.byref(ok), ctypes.sizeof(ok), ctypes.byref(plan)) == 0
    need = ctypes.c_size_t()
    assert lib.sat_local_attn_workspace_bytes(plan, 1, 9, ctypes.byref(need)) == -1 and b"multiple" in lib.sat_last_error()
    assert lib.sat_local_attn_workspace_bytes(plan, 1, 6, ctypes.byref(need)) == -1 and b"window" in lib.sat_last_error()
    assert lib.sat_local_attn_workspace_bytes(plan, 2, 64, ctypes.byref(need)) == 0 and need.value > 0 and need.value % 256 == 0
    assert lib.sat_local_attn_forward(plan, None, None, 2, 64, None, 0, None) == -5          # not finalized
    lib.sat_local_attn_plan_destroy(plan)
    assert lib.sat_local_attn_plan_create(ctypes.byref(ok), ctypes.sizeof(ok) - 4, ctypes.byref(plan)) == -1 and b"bytes" in lib.sat_last_error()
    for bad, code, word in ((cfg(window=64), -1, b"odd"), (cfg(window=1), -1, b"odd"), (cfg(heads=(8,)), -2, b"dim_heads"),
                            (cfg(heads=(1,), gemm_dtype=2), -2, b"dim_heads 128"), (cfg(embed_dims=(192,), heads=(2,)), -2, b"multiple of 128"),
                            (cfg(ff_inner=(100,)), -2, b"multiple of 64"), (cfg(gemm_dtype=1), -2, b"gemm_dtype"), (cfg(n_stages=17), -1, b"stages"),
                            (cfg(in_channels=200), -2, b"in_channels")):
        assert lib.sat_local_attn_plan_create(ctypes.byref(bad), ctypes.sizeof(bad), ctypes.byref(plan)) == code, lib.sat_last_error()
        assert word in lib.sat_last_error(), lib.sat_last_error()
