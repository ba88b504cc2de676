"""The shared plan lifecycle (csrc/plan_core.h) through the C ABI, once per kind of plan: a plan whose finalize first fails for a
missing tensor (-3), then for a mis-sized one (-1), and then succeeds, needs the same workspace and computes the same bits as a plan
built in one go.  The failures are argument errors answered with return codes.  Smallest models that reach every path of the core:
stacked q | k | v and wi_0 | wi_1 (T5), stacked weights and biases and the first-rows token-type table (RoBERTa), re-packed weights
(DiT, codec)."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu


def _synth(shapes, seed):
    """name -> fp32 tensor from stable_audio_tools.synthetic; norm weights around 1 instead of around 0"""
    from stable_audio_tools import synthetic
    out = {}
    for k, shp in shapes.items():
        t = synthetic.synth_tensor(k, shp, seed)
        out[k] = 1.0 + t if "norm" in k.lower() and k.endswith("weight") else t
    return out


def _dit(dev):
    import stable_audio_tools as S
    from stable_audio_tools import _hip, model_configs as MC, synthetic
    from stable_audio_tools.models import _init
    from stable_audio_tools.models.dit import FP8_FAMILIES, GEMM_DTYPES
    cfg = MC.reduced(MC.stable_audio_open_1_0())
    with _init.skip_init():
        m = S.create_model_from_config(cfg).model.model
    fmt = S.default_gemm_dtype()
    c = _hip.SatDitCfg(m.io_channels, m.embed_dim, m.depth, m.num_heads, m.cond_token_dim, m.cond_embed_dim, m.global_cond_dim, m.max_seq_len,
                       1 if m.global_cond_type == "adaLN" else 0, GEMM_DTYPES[fmt], FP8_FAMILIES.get(fmt, 0), int(m.layernorm_fusion),
                       0 if m.cross_attention_fusion else 1, m.tile_policy)
    lib = _hip.lib()
    bf, t_len, lc = 2, 64, 5
    x = synthetic.synth_input("x", (bf, m.io_channels, t_len), 1).to(dev)
    t = torch.tensor([0.3, 0.8], device=dev)
    cond = synthetic.synth_input("cond", (bf, lc, m.cond_token_dim), 2).to(dev)
    glob = synthetic.synth_input("glob", (bf, m.global_cond_dim), 3).to(dev)

    def run(plan, ws):
        out = torch.empty_like(x)
        _hip.check(lib.sat_dit_prepare_context(plan, _hip.ptr(cond), bf, lc, _hip.ptr(glob), _hip.stream()))
        _hip.check(lib.sat_dit_forward(plan, _hip.ptr(x), _hip.ptr(t), _hip.ptr(out), bf, t_len, _hip.ptr(ws), ws.numel(), _hip.stream()))
        return out
    create = lambda: _hip.new_handle(lib.sat_dit_plan_create_sized, ctypes.byref(c), ctypes.sizeof(c))
    return create, synthetic.synth_state_dict(m.state_dict(), 4), f"transformer.layers.{m.depth - 1}.ff.ff.2.weight", (bf, t_len), run


def _oobleck(dev):
    import stable_audio_tools as S
    from stable_audio_tools import _hip, model_configs as MC, synthetic
    from stable_audio_tools.models import _init
    from stable_audio_tools.models.autoencoders import _CODEC_GEMM_DTYPES
    with _init.skip_init():
        dec = S.create_model_from_config(MC.reduced(MC.stable_audio_vae())).decoder
    c = _hip.SatOobleckCfg()
    c.is_decoder, c.io_channels, c.channels, c.latent_dim, c.n_blocks = 1, dec.io_channels, dec.channels, dec.latent_dim, len(dec.strides)
    for i, (cm, st) in enumerate(zip(dec.c_mults, dec.strides)):
        c.c_mults[i], c.strides[i] = cm, st
    c.gemm_dtype = _CODEC_GEMM_DTYPES[S.default_gemm_dtype()]
    lib = _hip.lib()
    b, t_len = 1, 8
    z = synthetic.synth_input("z", (b, dec.latent_dim, t_len), 5).to(dev)

    def run(plan, ws):
        out = torch.empty((b, dec.io_channels, t_len * dec.ratio), dtype=torch.float32, device=dev)
        _hip.check(lib.sat_oobleck_decode(plan, _hip.ptr(z), _hip.ptr(out), b, t_len, _hip.ptr(ws), ws.numel(), _hip.stream()))
        return out
    create = lambda: _hip.new_handle(lib.sat_oobleck_plan_create, ctypes.byref(c))
    return create, synthetic.synth_state_dict(dec.state_dict(), 6), f"layers.{len(dec.strides) + 2}.weight_v", (b, t_len), run


def _t5(dev):
    from stable_audio_tools import _hip
    from test_t5 import T5_CONFIGS
    k = T5_CONFIGS["flan"]
    V, D, F, H, NL, NB = k["vocab_size"], k["d_model"], k["d_ff"], k["num_heads"], k["num_layers"], k["relative_attention_num_buckets"]
    inner = H * k["d_kv"]
    shapes = {"shared.weight": (V, D), "encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight": (NB, H),
              "encoder.final_layer_norm.weight": (D,)}
    for n in range(NL):
        pf = f"encoder.block.{n}.layer."
        shapes.update({pf + "0.layer_norm.weight": (D,), pf + "0.SelfAttention.q.weight": (inner, D), pf + "0.SelfAttention.k.weight": (inner, D),
                       pf + "0.SelfAttention.v.weight": (inner, D), pf + "0.SelfAttention.o.weight": (D, inner), pf + "1.layer_norm.weight": (D,),
                       pf + "1.DenseReluDense.wi_0.weight": (F, D), pf + "1.DenseReluDense.wi_1.weight": (F, D),
                       pf + "1.DenseReluDense.wo.weight": (D, F)})
    c = _hip.SatT5Cfg(V, D, k["d_kv"], F, NL, H, NB, k["relative_attention_max_distance"], 1, 0, 1e-6)
    lib = _hip.lib()
    b, l = 2, 8
    ids = torch.randint(0, V, (b, l), generator=torch.Generator().manual_seed(7), dtype=torch.int32).to(dev)
    mask = torch.ones(b, l, dtype=torch.int32)
    mask[1, 5:] = 0
    mask = mask.to(dev)

    def run(plan, ws):
        out = torch.empty((b, l, D), dtype=torch.float32, device=dev)
        _hip.check(lib.sat_t5_encode(plan, _hip.ptr(ids), _hip.ptr(mask), _hip.ptr(out), b, l, 1, _hip.ptr(ws), ws.numel(), _hip.stream()))
        return out
    create = lambda: _hip.new_handle(lib.sat_t5_plan_create, ctypes.byref(c))
    return create, _synth(shapes, 8), f"encoder.block.{NL - 1}.layer.1.DenseReluDense.wi_1.weight", (b, l), run


def _roberta(dev):
    from stable_audio_tools import _hip
    from test_clap_text import BOS, EOS, PAD, SHAPES
    k = SHAPES["reduced"]
    V, D, F, H, NL, P = (k["vocab_size"], k["hidden_size"], k["intermediate_size"], k["num_attention_heads"], k["num_hidden_layers"],
                         k["max_position_embeddings"])
    run_layers = 2
    shapes = {"embeddings.word_embeddings.weight": (V, D), "embeddings.position_embeddings.weight": (P, D),
              "embeddings.token_type_embeddings.weight": (2, D),          # two rows: the plan takes the first
              "embeddings.LayerNorm.weight": (D,), "embeddings.LayerNorm.bias": (D,)}
    for n in range(run_layers):
        pf = f"encoder.layer.{n}."
        for lin, (o, i) in {"attention.self.query": (D, D), "attention.self.key": (D, D), "attention.self.value": (D, D),
                            "attention.output.dense": (D, D), "intermediate.dense": (F, D), "output.dense": (D, F)}.items():
            shapes[pf + lin + ".weight"], shapes[pf + lin + ".bias"] = (o, i), (o,)
        for ln in ("attention.output.LayerNorm", "output.LayerNorm"):
            shapes[pf + ln + ".weight"] = shapes[pf + ln + ".bias"] = (D,)
    c = _hip.SatRobertaCfg(V, D, NL, run_layers, H, F, P, PAD, 0, 1e-5)
    lib = _hip.lib()
    b, l = 2, 9
    ids = torch.randint(3, V, (b, l), generator=torch.Generator().manual_seed(9), dtype=torch.int32)
    mask = torch.ones(b, l, dtype=torch.int32)
    ids[:, 0], ids[0, l - 1], ids[1, 4], ids[1, 5:], mask[1, 5:] = BOS, EOS, EOS, PAD, 0          # one row padded
    ids, mask = ids.to(dev), mask.to(dev)

    def run(plan, ws):
        out = torch.empty((b, l, D), dtype=torch.float32, device=dev)
        _hip.check(lib.sat_roberta_encode(plan, _hip.ptr(ids), _hip.ptr(mask), _hip.ptr(out), b, l, _hip.ptr(ws), ws.numel(), _hip.stream()))
        return out
    create = lambda: _hip.new_handle(lib.sat_roberta_plan_create, ctypes.byref(c))
    return create, _synth(shapes, 10), f"encoder.layer.{run_layers - 1}.output.dense.weight", (b, l), run


@pytest.mark.parametrize("kind", ["roberta", "t5", "oobleck", "dit"])
def test_finalize_after_missing_and_missized_tensor_matches_a_plan_built_in_one_go(dev, kind):
    from stable_audio_tools import _hip
    lib = _hip.lib()
    create, tensors, withheld, dims, run = {"dit": _dit, "oobleck": _oobleck, "t5": _t5, "roberta": _roberta}[kind](dev)
    assert withheld in tensors
    staged = {n: t.detach().to(dev, torch.float32).contiguous() for n, t in tensors.items()}
    set_tensor, finalize = getattr(lib, f"sat_{kind}_plan_set_tensor"), getattr(lib, f"sat_{kind}_plan_finalize")
    error = lambda: lib.sat_last_error().decode()

    def workspace(plan):
        need = ctypes.c_size_t()
        _hip.check(getattr(lib, f"sat_{kind}_workspace_bytes")(plan, *dims, ctypes.byref(need)))
        return need.value

    a, b = create(), create()
    try:
        for n, t in staged.items():
            _hip.check(set_tensor(a, n.encode(), _hip.ptr(t), t.numel()))
        _hip.check(finalize(a, _hip.stream()))
        need_a = workspace(a)
        ws = torch.empty(need_a, dtype=torch.uint8, device=dev)
        out_a = run(a, ws)
        torch.cuda.synchronize()
        assert torch.isfinite(out_a).all() and out_a.abs().max() > 0

        w = staged[withheld]
        for n, t in staged.items():
            if n != withheld:
                _hip.check(set_tensor(b, n.encode(), _hip.ptr(t), t.numel()))
        assert finalize(b, _hip.stream()) == -3
        assert f"'{withheld}'" in error() and "never set" in error()
        _hip.check(set_tensor(b, withheld.encode(), _hip.ptr(w), w.numel() - 1))
        assert finalize(b, _hip.stream()) == -1
        assert f"'{withheld}'" in error() and "expected" in error()
        _hip.check(set_tensor(b, withheld.encode(), _hip.ptr(w), w.numel()))
        assert finalize(b, _hip.stream()) == 0
        assert workspace(b) == need_a
        out_b = run(b, torch.empty(need_a, dtype=torch.uint8, device=dev))
        torch.cuda.synchronize()
        assert torch.equal(out_b, out_a)
    finally:
        getattr(lib, f"sat_{kind}_plan_destroy")(a)
        getattr(lib, f"sat_{kind}_plan_destroy")(b)
