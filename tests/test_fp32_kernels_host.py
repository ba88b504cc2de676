"""The references and gates of tests/test_gpu_fp32_kernels.py, proven on the CPU (pattern: test_codec_kernels_host.py): the restatements of
fp32_units agree with the modules they stand for -- the oracle's DiT pieces, torch.nn.functional's layer_norm, scaled_dot_product_attention and
interpolate, transformers' T5LayerNorm, NewGELUActivation and RoBERTa position ids; the same restatements evaluated in float32 by PyTorch on the
CPU pass every 1e-5 gate with a factor 4 to spare (the condition on the inputs) and the a-priori bound as it stands; every fault these kernels
can have is rejected by its gate while the whole-tensor rel-L2 stays under the 1e-4 of the fp32x model test; and the unit entries refuse, before
any launch, what their kernels cannot do.  With SAT_PARITY_LOG set the figures are appended to that file."""
import os

import pytest
import torch
import torch.nn.functional as F

import fp32_units as fu
from util import PARITY_LOG, rel_l2

F64 = torch.float64


def _fails(fn, *args, **kw):
    try:
        fn(*args, **kw)
    except AssertionError as e:
        return str(e)
    return None


def _log(line):
    if PARITY_LOG:
        with open(PARITY_LOG, "a") as f:
            f.write(f"{os.environ.get('PYTEST_CURRENT_TEST', '').split(' ')[0]}\t{line}\n")


def _close(a, b, tol=1e-12):
    e = ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300)).item()
    assert e <= tol, f"rel-L2 {e:.3e} > {tol:.0e}"


def _outputs(ref):
    return {k: v for k, v in ref.items() if ":" not in k}


# ------------------------------------------------------------------------------------------------ the condition on the inputs
def _cpu32(case):
    """The restatement in float32 on the CPU, rounded to the output format where the kernel rounds."""
    got = _outputs(fu.reference(case, torch.float32))
    if case.kind == "small_linear" and case.p["out16"]:
        got["y"] = got["y"].to((None, torch.bfloat16, torch.float16)[case.p["out16"]])
    return got


@pytest.mark.parametrize("kind", fu.KINDS)
def test_fp32_cpu_evaluation_passes_every_gate_four_times_over(kind):
    """Inputs for which a gate would be meaningless -- sine arguments of tens of radians, near-constant LayerNorm rows, scores whose own fp32
    rounding moves the softmax -- do not get in: PyTorch's float32 evaluation of the reference has to sit under a quarter of each 1e-5 gate,
    under the a-priori bound itself, and inside the code limits of the 16-bit outputs."""
    for p in fu.CASES[kind]:
        case = fu.Case(kind, p)
        fu.LOG.clear()
        fu.check(case, _cpu32(case), headroom=0.25)
        for name, key, what, figure, where in fu.LOG:
            _log(f"fp32 CPU\t{name}\t{key}\t{what}\t{figure:.3e}\t{where}")


def test_case_lists_hold_the_seams():
    """The shapes the gates are taken at: every seam named in the device test is in the lists."""
    gemm = {(p["m"], p["n"], p["k"]) for p in fu.CASES["gemm_f32"]}
    assert gemm == {(130, 136, 48), (1, 8, 16), (128, 128, 32), (257, 129, 512)}
    assert {(p["bias"], p["acc"]) for p in fu.CASES["gemm_f32"]} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert {p["l"] for p in fu.CASES["enc_attention"]} == {1, 19, 64, 65, 130, 512}
    assert {(p["c"], p["d"], p["pre"]) for p in fu.CASES["output_proj"]} == {(c, d, s) for c in (4, 8, 64) for d in (128, 256, 1536) for s in (0, 1, 4)}
    assert {(p["tc"], p["p"]) for p in fu.CASES["input_proj_extra"]} == {(tc, pp) for tc in ("t", 5, 200) for pp in (0, 3, 9)}
    assert {(p["act"], p["out16"]) for p in fu.CASES["small_linear"]} >= {(a, 0) for a in (0, 1, 2)} | {(0, 1), (0, 2)}
    ids = fu.Case("roberta_embed_ln", dict(table="onehot")).t["ids"]
    pad = ids == 1
    assert pad[0, 100:].all() and pad[1, 63] and pad[1, 64] and pad[1, 127] and not pad[1, 129] and not pad[1, 65]


# ------------------------------------------------------------------------------------------------------------ the references
def test_layernorm_reference_is_f_layer_norm():
    for p in fu.CASES["layernorm_f32"]:
        c = fu.Case("layernorm_f32", p)
        if p["var"] == "mod":
            continue
        t = c.t
        want = F.layer_norm(t["x"].double(), (p["d"],), t["gamma"].double(), None if t["beta"] is None else t["beta"].double(), c.dim["eps"])
        _close(fu.reference(c)["y"], want)
    from oracle import dit as odit
    c = fu.Case("layernorm_f32", dict(m=7, d=100, eps=1e-5, var="plain"))
    _close(fu.reference(c)["y"], odit.layer_norm(c.t["x"].double(), c.t["gamma"].double(), c.t["beta"].double()))


def test_modulated_layernorm_is_the_oracles_adaln_line():
    """oracle.transformer_block: h = layer_norm(x) * (1 + scale) + shift per sequence; the kernel is handed 1 + scale (adaln_finish)."""
    c = fu.Case("layernorm_f32", dict(m=37, d=256, eps=1e-5, var="mod"))
    t, d = c.t, c.dim
    x = F.pad(t["x"].double(), (0, 0, 0, 2)).view(13, 3, 256)            # 37 rows -> 13 sequences of 3 (the last one short)
    h = F.layer_norm(x, (256,), t["gamma"].double(), t["beta"].double(), d["eps"]) * t["scale"].double()[:, None, :256] + t["shift"].double()[:, None, :256]
    _close(fu.reference(c)["y"], h.view(39, 256)[:37])


def test_attention_reference_is_sdpa_and_the_oracles_core():
    from oracle import dit as odit
    for p in fu.CASES["attention_f32"]:
        c = fu.Case("attention_f32", p)
        q, k, v = (c.t[x].double() for x in ("q", "k", "v"))
        rep = p["h"] // p["kvh"]
        want = F.scaled_dot_product_attention(q, k.repeat_interleave(rep, 1), v.repeat_interleave(rep, 1))
        got = fu.reference(c)["out"]
        _close(got, want.permute(0, 2, 1, 3), 1e-10)
        _close(got, odit.attention_core(c.t["q"], c.t["k"], c.t["v"]).permute(0, 2, 1, 3), 1e-5)            # (the oracle's softmax is float32)


@pytest.mark.parametrize("p", [p for p in fu.CASES["enc_attention"] if p["l"] in (19, 130)], ids=fu.case_id)
def test_enc_attention_reference_is_the_additive_mask_of_transformers(p):
    """transformers adds (1 - mask) * finfo(float32).min to the scores and takes the softmax in float32; in float32 that sum absorbs the score,
    so masked keys weigh exactly zero and an all-padding row is the uniform average.  The restatement excludes and averages instead; both agree."""
    c = fu.Case("enc_attention", p)
    t, d = c.t, c.dim
    b, l, h, dkv = d["b"], d["l"], d["h"], d["dkv"]
    q, k, v = (x.view(b, l, h, dkv).permute(0, 2, 1, 3) for x in t["qkv"].chunk(3, dim=-1))
    s = torch.einsum("bhid,bhjd->bhij", q, k) * d["scale"]
    if t["pb"] is not None:
        idx = torch.arange(l)[None, :] - torch.arange(l)[:, None] + l - 1
        s = s + t["pb"][:, idx]
    s = s + (1.0 - t["mask"].float()).view(b, 1, 1, l) * torch.finfo(torch.float32).min
    want = torch.einsum("bhij,bhjd->bhid", torch.softmax(s, dim=-1), v).permute(0, 2, 1, 3)
    got = fu.reference(c)["out"]
    for item in range(b):            # float32 against float64: the figure is fp32's, the agreement is in what is excluded
        assert rel_l2(want[item], got[item]) < 2e-6
    pad_item = [i for i, m in enumerate(p["masks"].split("+")) if m == "allpad"]
    for item in pad_item:
        _close(got[item], v.double().mean(dim=2)[item][None].expand(l, h, dkv), 1e-12)


def test_rope_reference_is_the_oracles_partial_rotary():
    from oracle import dit as odit
    c = fu.Case("split_heads_f32", dict(parts=3, rope=3, norm=0))
    d = c.dim
    inv_freq = 10000.0 ** (-torch.arange(16, dtype=F64) / 16.0)
    ang = torch.arange(d["s"], dtype=F64)[:, None] * inv_freq[None, :]
    freqs = torch.cat((ang, ang), dim=-1)
    src = c.t["src"].double().view(d["b"], d["s"], 3, d["h"], 64)
    ref = fu.reference(c)
    # the tables the kernel is handed are the fp32 images of cos / sin: 6e-8 from the float64 ones
    for i in range(2):
        _close(ref[f"d{i}"], odit.apply_rotary(src[:, :, i].permute(0, 2, 1, 3), freqs), 2e-7)
    _close(ref["d2"], src[:, :, 2].permute(0, 2, 1, 3))
    n = fu.reference(fu.Case("split_heads_f32", dict(parts=1, rope=0, norm=1)))["d0"]
    c1 = fu.Case("split_heads_f32", dict(parts=1, rope=0, norm=1))
    _close(n, F.normalize(c1.t["src"].double().view(2, 37, 3, 64).permute(0, 2, 1, 3), dim=-1))


def test_swiglu_and_fourier_references_are_the_oracles():
    from oracle import dit as odit
    c = fu.Case("swiglu_f32", fu.CASES["swiglu_f32"][1])
    val, gate = c.t["hg"].double().chunk(2, dim=-1)
    _close(fu.reference(c)["h"], val * F.silu(gate))
    for p in fu.CASES["fourier"]:
        c = fu.Case("fourier", p)
        tv = c.t["t"] if c.t["t"] is not None else torch.full((3,), c.dim["t_const"])
        _close(fu.reference(c)["out"], odit.fourier_features(c.t["w"].double()[:, None], tv.double()[:, None]))


def test_fold_and_projection_references_are_the_oracles_convolutions():
    """dit_inner_forward: x = conv1d(x, preprocess) + x, then project_in; project_out, then out = conv1d(out, postprocess) + out."""
    cin = fu.Case("fold_in", dict(d=128, c=64))
    x = torch.randn(2, 64, 13, generator=torch.Generator().manual_seed(1)).double()
    w_in, w_pre = cin.t["w"].double(), cin.t["wc"].double()
    want = F.linear((F.conv1d(x, w_pre[:, :, None]) + x).transpose(1, 2), w_in)
    _close(torch.einsum("cn,bct->btn", fu.reference(cin)["weff_t"], x), want)
    cout = fu.Case("fold_out", dict(d=128, c=64))
    X = torch.randn(2, 13, 128, generator=torch.Generator().manual_seed(2)).double()
    w_out, w_post = cout.t["w"].double(), cout.t["wc"].double()
    o = F.linear(X, w_out).transpose(1, 2)
    _close(torch.einsum("nc,btn->bct", fu.reference(cout)["weff_t"], X), F.conv1d(o, w_post[:, :, None]) + o)
    # the projections on a folded weight: rows (S - T).. of X, sequence b reads latent b % xB
    c = fu.Case("input_proj", dict(c=64, t=13, d=128, pre=1))
    got = fu.reference(c)["X"]
    for b in range(4):
        _close(got[b], c.dim["xscale"] * F.linear(c.t["x"][b % 2].double().T, c.t["weff_t"].double().T))
    c = fu.Case("output_proj", dict(c=8, d=128, pre=4))
    _close(fu.reference(c)["out"], F.linear(c.t["X"].double()[:, 4:], c.t["weff_t"].double().T).transpose(1, 2))


@pytest.mark.parametrize("tc,t", [(5, 13), (200, 13), (5, 77), (200, 77), (200, 8), (5, 1), (13, 13), (200, 1), (77, 200)])
def test_nearest_source_frames_are_f_interpolates(tc, t):
    """Index for index: a signal that holds its own frame number comes back as the source indices, and the concat part of the reference
    is F.interpolate + a 1 x 1 convolution."""
    src = fu.nearest_src(tc, t)
    sig = torch.arange(tc, dtype=F64).view(1, 1, tc) * 3.0 + 1.0
    assert torch.equal(F.interpolate(sig, size=t, mode="nearest").view(t), src.double() * 3.0 + 1.0)
    scale = torch.tensor(tc, dtype=torch.float32) / torch.tensor(t, dtype=torch.float32)
    formula = torch.clamp(torch.floor(torch.arange(t, dtype=torch.float32) * scale).long(), max=tc - 1)
    assert torch.equal(src, formula)


def test_input_proj_extra_reference_is_interpolate_cat_project():
    c = fu.Case("input_proj_extra", dict(c=2, t=13, d=128, tc=200, p=3, pre=1))
    t, d = c.t, c.dim
    x = t["x"].double()[torch.arange(4) % 2] * d["xscale"]
    cat = torch.cat((x, F.interpolate(t["concat"].double(), size=13, mode="nearest")), dim=1)
    ref = fu.reference(c)
    _close(ref["X"], F.linear(cat.transpose(1, 2), t["weff_t"].double().T))
    assert torch.equal(ref["prep"], t["prep"])


def test_position_table_references():
    """ScaledSinusoidalEmbedding: cat(sin, cos)(pos * theta ** -(j / half)) * scale with float32 angles; AbsolutePositionalEmbedding:
    emb(pos) * dim ** -0.5."""
    c = fu.Case("pos_table", dict(mode=1))
    half = 64
    inv_freq = 10000 ** -(torch.arange(half).float() / half)
    emb = torch.einsum("i,j->ij", torch.arange(64).float(), inv_freq)
    want32 = torch.cat((emb.sin(), emb.cos()), dim=-1) * c.t["src"]
    assert rel_l2(fu.reference(c, torch.float32)["table"], want32) == 0.0
    assert rel_l2(fu.reference(c)["table"], want32) < 1e-6            # sine and cosine of the SAME float32 angles
    c = fu.Case("pos_table", dict(mode=2))
    emb = torch.nn.Embedding(73, 128)
    with torch.no_grad():
        emb.weight.copy_(c.t["src"])
        _close(fu.reference(c)["table"], emb(torch.arange(64)).double() * 128 ** -0.5)


def test_cfg_reference_is_the_oracles_combine():
    """oracle.dit_forward: cfg = uncond + (cond - uncond) * scale; with scale_phi: phi * (cfg * cond_std / cfg_std) + (1 - phi) * cfg."""
    c = fu.Case("cfg_denoise", dict(use_cfg=1, phi=0.6))
    d = c.dim
    mo, x = c.t["mo"].double(), c.t["x"].double()
    cond, unc = mo[:2], mo[2:]
    cfg = unc + (cond - unc) * d["cfg_scale"]
    cfg = d["phi"] * (cfg * (cond.std(dim=1, keepdim=True) / cfg.std(dim=1, keepdim=True))) + (1 - d["phi"]) * cfg
    _close(fu.reference(c)["den"], cfg * d["c_out"] + x * d["c_skip"])


def test_adaln_reference_is_the_oracles_block():
    """oracle.transformer_block: h * (1 + scale) + shift, branch * sigmoid(1 - gate); chunks (scale, shift, gate) x (self, ff)."""
    c = fu.Case("adaln_finish", fu.CASES["adaln_finish"][0])
    v = c.t["ssg"].double()
    got = fu.reference(c)["ssg"]
    for ch in range(6):
        want = 1 + v[:, :, ch] if ch in (0, 3) else (torch.sigmoid(1 - v[:, :, ch]) if ch in (2, 5) else v[:, :, ch])
        _close(got[:, :, ch], want)


def test_encoder_formulas():
    """What fp32_units restates for the encoders, from the formulas alone (no transformers needed): T5LayerNorm x * rsqrt(mean(x^2) + eps) * w,
    gelu_new, the exact GELU, and RoBERTa's position ids pad + cumsum(ids != pad) * (ids != pad)."""
    c = fu.Case("t5_rmsnorm", dict(m=5, d=512))
    x = c.t["x"].double()
    _close(fu.reference(c)["y"], c.t["w"].double() * (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + c.dim["eps"])))
    x = torch.linspace(-14, 14, 401, dtype=F64)
    _close(fu.gelu_erf(x), F.gelu(x))
    _close(fu.gelu_new(x), F.gelu(x, approximate="tanh"))
    c = fu.Case("t5_act", dict(rows=3, f=100, gated=1))
    g = c.t["g"].double()
    _close(fu.reference(c)["h"], F.gelu(g[:, :100], approximate="tanh") * g[:, 100:])
    ids = torch.tensor([[5, 1, 7, 7, 1, 1, 9]])
    assert fu.roberta_positions(ids, 1).tolist() == [[2, 1, 3, 4, 1, 1, 5]]
    want = [[0] * 130 for _ in range(2)]            # the scan, id by id
    all_ids = fu.Case("roberta_embed_ln", dict(table="onehot")).t["ids"]
    for b in range(2):
        seen = 0
        for i in range(130):
            seen += int(all_ids[b, i] != 1)
            want[b][i] = 1 + seen if all_ids[b, i] != 1 else 1
    assert fu.roberta_positions(all_ids.long(), 1).tolist() == want


def test_encoder_references_are_transformers_modules():
    """The same against T5LayerNorm, NewGELUActivation and RoBERTa's create_position_ids_from_input_ids where transformers is installed."""
    tr = pytest.importorskip("transformers")
    from transformers.activations import NewGELUActivation
    from transformers.models.t5.modeling_t5 import T5LayerNorm
    try:
        from transformers.models.roberta.modeling_roberta import create_position_ids_from_input_ids as pos_ids
    except ImportError:
        pos_ids = lambda ids, pad: tr.models.roberta.modeling_roberta.RobertaEmbeddings.create_position_ids_from_input_ids(ids, pad)
    c = fu.Case("t5_rmsnorm", dict(m=5, d=512))
    ln = T5LayerNorm(512, eps=c.dim["eps"]).double()
    with torch.no_grad():
        ln.weight.copy_(c.t["w"])
        _close(fu.reference(c)["y"], ln(c.t["x"].double()), 1e-6)            # (T5LayerNorm takes its variance in float32)
    x = torch.linspace(-14, 14, 401, dtype=F64)
    _close(fu.gelu_new(x), NewGELUActivation()(x))
    c = fu.Case("roberta_embed_ln", dict(table="onehot"))
    assert torch.equal(fu.roberta_positions(c.t["ids"].long(), 1), pos_ids(c.t["ids"].long(), 1))
    c = fu.Case("t5_act", dict(rows=3, f=100, gated=1))
    g = c.t["g"].double()
    _close(fu.reference(c)["h"], NewGELUActivation()(g[:, :100]) * g[:, 100:])


def test_roberta_embedding_reference_is_gather_add_layer_norm():
    c = fu.Case("roberta_embed_ln", dict(table="random"))
    t, d = c.t, c.dim
    ids = t["ids"].long()
    pos = torch.cumsum((ids != 1).long(), dim=1) * (ids != 1).long() + 1
    e = F.embedding(ids, t["word"].double()) + t["type0"].double() + F.embedding(pos, t["posw"].double())
    _close(fu.reference(c)["y"], F.layer_norm(e, (d["d"],), t["gamma"].double(), t["beta"].double(), d["eps"]))
    assert int(pos.max()) < d["max_pos"] and int(pos[0, 99]) == 101 and int(pos[0, 100]) == 1


# ------------------------------------------------------------------------------------------------------------ planted faults
def _rejected(case, faulty, want, what):
    """``faulty`` fails the case's gates although its whole-tensor rel-L2 stays under the model tests' gate."""
    whole = max(rel_l2(faulty[k].double(), want[k].double()) for k in faulty if want[k].is_floating_point())
    msg = _fails(fu.check, case, faulty, want)
    _log(f"planted\t{what}\twhole rel-L2 {whole:.3e}\trejected: {bool(msg)}")
    assert whole < fu.MODEL_GATE, f"{what}: whole-tensor rel-L2 {whole:.3e} would not pass the model test either"
    assert msg is not None, f"{what}: the gates accept it (whole-tensor rel-L2 {whole:.3e})"
    return msg


def _correct(case):
    """A correct result to plant a fault into: the float32 evaluation, which passes (test above)."""
    want = fu.reference(case)
    got = _cpu32(case)
    fu.check(case, got, want)
    return got, want


def test_rejects_a_wrong_row_behind_a_tile_edge():
    case = fu.Case("gemm_f32", dict(m=257, n=129, k=512, bias=1, acc=0, gate=1))
    got, want = _correct(case)
    for row in (128, 256):            # the first row of the second tile, the lone row of the third
        bad = {"c": got["c"].clone()}
        bad["c"][row] *= 1.0 + 1e-3
        _rejected(case, bad, want, f"gemm_f32 row {row} off by 1e-3")


def _drop_one_product(want, key, n_terms, products, where):
    """The element of ``where`` (an index tuple with one slice) whose dropped product is closest to ten times its bound: small against the
    tensor, far over the bound.  Returns (full index, product)."""
    bound = (n_terms + 4) * fu.UNIT * want[key + ":mag"][where]
    col = int((products.double().abs() / bound - 10.0).abs().argmin())
    assert products[col].abs() > 3 * bound[col]
    return tuple(col if isinstance(i, slice) else i for i in where), products[col]


def test_rejects_one_dropped_product():
    """One product missing from a sum of 512 is over the a-priori bound in nearly every element it can be missing from; one that is missing
    from a single element -- far under every norm-wise gate, 1e-5 of the tensor -- is rejected all the same."""
    case = fu.Case("gemm_f32", dict(m=257, n=129, k=512, bias=0, acc=0, gate=0))
    got, want = _correct(case)
    row, kk = 200, 300
    products = case.t["a"][row, kk] * case.t["w"][:, kk]
    share = fu.bound_share(got["c"][row] - products, want["c"][row], want["c:mag"][row], 512)
    ok_share = fu.bound_share(got["c"], want["c"], want["c:mag"], 512).max().item()
    _log(f"dropped product: {float((share > 1).double().mean()):.3f} of the row's elements over the bound; a correct fp32 result uses {ok_share:.3f} of it")
    assert float((share > 1).double().mean()) >= 0.9 and ok_share < 0.25
    idx, prod = _drop_one_product(want, "c", 512, products, (row, slice(None)))
    bad = {"c": got["c"].clone()}
    bad["c"][idx] -= prod
    assert "a-priori bound" in _rejected(case, bad, want, "gemm_f32 one product of 512 dropped from one element")
    # the same in the glue contractions: the last channel of 64 of the input projection at the last time step, one of 128 of the output projection
    case = fu.Case("input_proj", dict(c=64, t=13, d=128, pre=1))
    got, want = _correct(case)
    idx, prod = _drop_one_product(want, "X", 65, case.dim["xscale"] * case.t["weff_t"][63] * case.t["x"][0, 63, 12], (2, 12, slice(None)))
    bad = {"X": got["X"].clone()}
    bad["X"][idx] -= prod
    assert "a-priori bound" in _rejected(case, bad, want, "input_proj last channel dropped at the last time step, one element")
    case = fu.Case("output_proj", dict(c=64, d=128, pre=1))
    got, want = _correct(case)
    idx, prod = _drop_one_product(want, "out", 128, case.t["weff_t"][127] * case.t["X"][0, 1 + 12, 127], (0, slice(None), 12))
    bad = {"out": got["out"].clone()}
    bad["out"][idx] -= prod
    assert "a-priori bound" in _rejected(case, bad, want, "output_proj last input channel dropped for one token, one element")


def test_rejects_a_gate_row_from_the_neighbouring_sequence():
    """Neighbouring sequences' gates differ by 1e-3 here (the two halves of a CFG batch are that close): row 65, the first of sequence 1,
    multiplied with the gate of sequence 0."""
    case = fu.Case("gemm_f32", dict(m=257, n=129, k=512, bias=1, acc=0, gate=1))
    g = torch.Generator().manual_seed(5)
    case.t["gate"][1] = case.t["gate"][0] * (1.0 + 1e-3 * torch.randn(case.t["gate"].shape[1], generator=g))
    got, want = _correct(case)
    bad = {"c": got["c"].clone()}
    bad["c"][65] = got["c"][65] / case.t["gate"][1, :129] * case.t["gate"][0, :129]
    _rejected(case, bad, want, "gemm_f32 gate row of the neighbouring sequence")


def _with_weak_keys(case, keys, offset):
    """Channel 0 of every query is 8 and of the given keys -offset: their scores sit about `offset` below the others', so that what they
    contribute is small against the whole tensor and large against 1e-5."""
    case.t["q"][..., 0] = 8.0
    case.t["k"][..., 0] = 0.0
    case.t["k"][:, :, keys, 0] = -float(offset)


def test_rejects_a_dropped_last_key_chunk():
    case = fu.Case("attention_f32", dict(b=2, h=4, kvh=2, sq=70, sk=77, var="plain"))
    _with_weak_keys(case, slice(72, 77), 6.0)
    got, want = _correct(case)
    q, k, v = (case.t[x].double() for x in ("q", "k", "v"))
    bad = {"out": got["out"].clone()}
    b, i, h = 0, 69, 3            # the last query of the partial workgroup, one head: keys 72.. never read
    bad["out"][b, i, h] = fu.attention(q[b, h, i:i + 1], k[b, h // 2, :72], v[b, h // 2, :72], 0.125)[0].float()
    assert "per (row, head)" in _rejected(case, bad, want, "attention_f32 last chunk of 5 keys dropped for one (query, head)")


def test_rejects_one_leaked_pad_key():
    case = fu.Case("enc_attention", dict(l=130, dkv=64, style="roberta", masks="full+tail"))
    t, d = case.t, case.dim
    inner = d["h"] * d["dkv"]
    g = torch.Generator().manual_seed(6)
    t["qkv"][1, 65:, inner:] = torch.randn((65, 2 * inner), generator=g) * 0.5            # ordinary K / V rows under the padding
    qkv = t["qkv"].view(2, 130, 3, d["h"], 64)
    qkv[:, :, 0, :, 0] = 8.0            # (scale 1 / 8: the leaked key's channel 0 moves its score by 8 * -6 / 8)
    qkv[:, :, 1, :, 0] = 0.0
    qkv[1, 65, 1, :, 0] = -6.0            # the first padded key of sequence 1 scores about 6 below the real ones
    got, want = _correct(case)
    q, k, v = (x.double() for x in (qkv[1, :, 0], qkv[1, :, 1], qkv[1, :, 2]))            # [l, h, 64]
    bad = {"out": got["out"].clone()}
    i, h = 64, 1
    bad["out"][1, i, h] = fu.attention(q[i:i + 1, h], k[:66, h], v[:66, h], d["scale"])[0].float()            # keys 0..64 and the leaked 65
    assert "per (row, head)" in _rejected(case, bad, want, "enc_attention one padded key leaked into one (query, head)")


def test_rejects_one_rope_pair_with_the_wrong_sign():
    case = fu.Case("split_heads_f32", dict(parts=3, rope=3, norm=0))
    got, want = _correct(case)
    b, h, s, pair = 0, 2, 1, 15            # position 1, the slowest pair: an angle of 1.8e-4
    src = case.t["src"].view(2, 37, 3, 3, 64)[b, s, 1, h]
    cs, sn = case.t["cos"][s, pair], case.t["sin"][s, pair]
    bad = {k: v.clone() for k, v in got.items()}
    bad["d1"][b, h, s, pair] = src[pair] * cs + src[pair + 16] * sn            # + instead of -
    msg = _rejected(case, bad, want, "split_heads_f32 one rotary pair of k with the wrong sign")
    assert "d1" in msg


def test_rejects_a_source_frame_off_by_one():
    case = fu.Case("input_proj_extra", dict(c=64, t=77, d=128, tc=200, p=3, pre=1))
    tc = 200
    case.t["concat"] = (1.0 + 1e-3 * torch.arange(tc, dtype=torch.float32)).view(1, 1, tc) * torch.tensor([1.0, -2.0, 0.5]).view(1, 3, 1) * \
        (1.0 + torch.arange(4, dtype=torch.float32)).view(4, 1, 1)            # a slow ramp: neighbouring frames differ by 1e-3
    got, want = _correct(case)
    src = fu.nearest_src(tc, 77)
    b, i = 1, 40
    bad = {k: v.clone() for k, v in got.items()}
    bad["X"][b, i] += torch.einsum("cn,c->n", case.t["weff_t"][64:], case.t["concat"][b, :, src[i] + 1] - case.t["concat"][b, :, src[i]])
    _rejected(case, bad, want, "input_proj_extra concat frame src + 1 at one time step")


def test_rejects_a_prepend_row_shifted_by_one():
    case = fu.Case("input_proj_extra", dict(c=64, t=77, d=128, tc="t", p=9, pre=1))
    g = torch.Generator().manual_seed(7)
    case.t["prep"] = case.t["prep"][:, :1] * (1.0 + 1e-3 * torch.randn((4, 9, 1), generator=g))            # rows that differ by 1e-3
    got, want = _correct(case)
    bad = {k: v.clone() for k, v in got.items()}
    bad["prep"][2, 7] = got["prep"][2, 8]            # the row across IP_TT = 8 read one too far
    assert "bit-identical" in _rejected(case, bad, want, "input_proj_extra prepend row 7 holds row 8")


def test_rejects_a_token_written_to_the_next_batch_items_slot():
    case = fu.Case("output_proj", dict(c=8, d=128, pre=1))
    g = torch.Generator().manual_seed(8)
    X = case.t["X"]
    X[1] = X[0] * (1.0 + 3e-4 * torch.randn(X[0].shape, generator=g))            # neighbouring sequences 3e-4 apart
    got, want = _correct(case)
    bad = {"out": got["out"].clone()}
    bad["out"][1, :, 2] = got["out"][0, :, 2]            # token 15 = (b 1, t 2) of the workgroup that straddles items 0 and 1
    _rejected(case, bad, want, "output_proj token (0, 2) written to (1, 2)")


def test_rejects_a_position_index_off_by_one_after_token_64():
    case = fu.Case("roberta_embed_ln", dict(table="onehot"))
    got, want = _correct(case)
    got["pos"] = want["pos"].clone()
    bad = dict(got, pos=want["pos"].clone())
    bad["pos"][1, 70] += 1            # the second ballot round of the scan counts one id too many
    msg = _fails(fu.check, case, bad, want)
    assert msg and "pos" in msg
    # under a smooth position table the same slip is invisible to the model test's figure
    smooth = fu.Case("roberta_embed_ln", dict(table="random"))
    smooth.t["posw"] = smooth.t["posw"][:1] * (1.0 + 1e-3 * torch.randn((smooth.dim["max_pos"], 1), generator=torch.Generator().manual_seed(9)))
    ok = fu.reference(smooth)["y"]
    ids = smooth.t["ids"].long()
    e = (smooth.t["word"].double()[ids] + smooth.t["type0"].double()) + smooth.t["posw"].double()[bad["pos"]]
    slipped = fu.layer_norm(e, smooth.t["gamma"].double(), smooth.t["beta"].double(), 1e-5)
    assert rel_l2(slipped, ok) < fu.MODEL_GATE


def test_sentinel_columns_and_16_bit_codes_are_gated():
    """small_linear's 16-bit results: two codes off in one element, or one code off in 2 % of them, is rejected."""
    case = fu.Case("small_linear", dict(r=17, n=130, k=512, act=0, bias=1, add=0, out16=1))
    got, want = _correct(case)
    bits = got["y"].view(torch.int16).clone()
    bits[3, 5] += 2
    assert "more than one" in _fails(fu.check, case, {"y": bits.view(torch.bfloat16)}, want)
    bits = got["y"].view(torch.int16).clone()
    bits.view(-1)[::40] += 1
    assert "1 %" in _fails(fu.check, case, {"y": bits.view(torch.bfloat16)}, want)


# -------------------------------------------------------------------------------------------------------------- the refusals
def test_entries_refuse_what_their_kernels_cannot_do():
    """Decided before any launch, so without a device: SAT_E_INVALID (-1) for NULL pointers and impossible dimensions, SAT_E_UNSUPPORTED (-2)
    for dimensions outside a kernel's repertoire -- 513 keys (a lane holds 8 scores), a head dim that is no multiple of 4, 6 or 192 channels in
    the output projection (float4 weight loads, 16 channels per wave and step), K = 24 in the fp32 GEMM (K-steps of 16), K or a row pitch of 6 in
    small_linear (float4 loads)."""
    from stable_audio_tools import _hip
    lib = _hip.lib()
    # a non-NULL, aligned pointer that no call below gets to read.  With a device present it is a real zeroed buffer that covers every shape probed
    # here, so that a check that ever stopped refusing would end in a failed assertion and not in a kernel on a stray address
    keep = torch.zeros(16 << 20, dtype=torch.uint8, device="cuda") if torch.cuda.is_available() else None
    P = keep.data_ptr() if keep is not None else 1 << 20
    assert P % 256 == 0
    INVALID, UNSUPPORTED = -1, -2

    def rc(entry, *args):
        return getattr(lib, entry)(*args, None)

    assert rc("sat_enc_attention", P, None, P, P, 2, 513, 3, 64, 1.0) == UNSUPPORTED and b"513" in lib.sat_last_error()
    assert rc("sat_enc_attention", P, None, P, P, 2, 512, 3, 42, 1.0) == UNSUPPORTED
    assert rc("sat_enc_attention", P, None, None, P, 2, 64, 3, 64, 1.0) == INVALID
    assert rc("sat_enc_attention", P, None, P, P, 0, 64, 3, 64, 1.0) == INVALID
    assert rc("sat_output_proj", P, P, P, 3, 6, 13, 13, 128) == UNSUPPORTED
    assert rc("sat_output_proj", P, P, P, 3, 8, 13, 13, 192) == UNSUPPORTED
    assert rc("sat_output_proj", P, P, P, 3, 68, 13, 13, 128) == UNSUPPORTED
    assert rc("sat_output_proj", P, P, P, 3, 8, 13, 13, 8192) == UNSUPPORTED            # 8 staged rows beyond the LDS
    assert rc("sat_output_proj", P, P, P, 3, 8, 13, 12, 128) == INVALID            # S < T
    assert rc("sat_output_proj", None, P, P, 3, 8, 13, 13, 128) == INVALID
    assert rc("sat_gemm_f32", P, P, None, P, 8, 8, 24, 8, 0, None, 1, 0) == UNSUPPORTED and b"K=24" in lib.sat_last_error()
    assert rc("sat_gemm_f32", P, P, None, P, 8, 8, 16, 4, 0, None, 1, 0) == INVALID            # ldc < N
    assert rc("sat_gemm_f32", P, P, None, P, 8, 8, 16, 8, 0, P, 0, 8) == INVALID            # a gate without rows per gate
    assert rc("sat_gemm_f32", P, None, None, P, 8, 8, 16, 8, 0, None, 1, 0) == INVALID
    assert rc("sat_small_linear", P, 8, P, None, None, 0, P, 8, 2, 8, 6, 0, 0) == UNSUPPORTED
    assert rc("sat_small_linear", P, 6, P, None, None, 0, P, 8, 2, 8, 4, 0, 0) == UNSUPPORTED
    assert rc("sat_small_linear", P, 8, P, None, None, 0, P, 4, 2, 8, 8, 0, 0) == INVALID            # ldy < N
    assert rc("sat_small_linear", P, 8, P, None, None, 0, P, 8, 2, 8, 8, 3, 0) == INVALID            # act
    assert rc("sat_small_linear", P, 8, P, None, None, 0, P, 8, 2, 8, 8, 0, 3) == INVALID            # out16
    assert rc("sat_small_linear", P, 8, None, None, None, 0, P, 8, 2, 8, 8, 0, 0) == INVALID
    assert rc("sat_input_proj", P, P, P, 4, 2, 65, 13, 13, 128, 1.0) == UNSUPPORTED
    assert rc("sat_input_proj", P, P, P, 4, 0, 64, 13, 13, 128, 1.0) == INVALID
    assert rc("sat_input_proj_extra", P, P, P, 4, 2, 64, 13, 16, 128, 1.0, P, 3, 13, P, 3) == INVALID            # S != P + 1 + T
    assert rc("sat_input_proj_extra", P, P, P, 4, 2, 64, 13, 17, 128, 1.0, P, 3, 13, None, 3) == INVALID            # prepend rows without a tensor
    assert rc("sat_layernorm_f32", P, P, None, P, 4, 64, P, None, 3, 72, 1e-5) == INVALID            # a scale without a shift
    assert rc("sat_layernorm_f32", P, P, None, P, 4, 64, P, P, 3, 60, 1e-5) == INVALID            # ld < d
    assert rc("sat_split_heads_f32", P, P, None, None, 2, 37, 2, 3, 0, None, None, 0) == INVALID            # two parts, one destination
    assert rc("sat_split_heads_f32", P, P, P, P, 2, 37, 3, 3, 3, None, None, 0) == INVALID            # rotary without tables
    assert rc("sat_split_heads_f32", P, P, None, None, 2, 37, 1, 3, 2, P, P, 0) == INVALID            # a mask bit beyond the parts
    assert rc("sat_swiglu_f32", P, None, 4, 64) == INVALID
    assert rc("sat_attention_f32", P, P, P, P, 1, 4, 3, 8, 8) == INVALID            # h % kvh
    assert rc("sat_t5_rmsnorm", P, P, P, 3, 6, 1e-6) == UNSUPPORTED
    assert rc("sat_t5_embed", P, P, P, 3, 6, 10) == UNSUPPORTED
    assert rc("sat_t5_act", P, P, 3, 8, 2) == INVALID
    assert rc("sat_t5_mask_rows", P, None, 3, 8) == INVALID
    assert rc("sat_t5_position_bias", P, P, P, 0, 5) == INVALID
    assert rc("sat_roberta_embed_ln", P, P, P, P, P, P, P, 2, 130, 64, 50, 1, 131, 1e-5) == UNSUPPORTED            # position 131 of a table of 131
    assert rc("sat_roberta_embed_ln", P, P, P, P, P, P, P, 2, 130, 64, 50, 50, 400, 1e-5) == INVALID            # pad_id outside the vocabulary
    assert rc("sat_roberta_gelu", None, 8) == INVALID
    assert rc("sat_adaln_finish", P, 100, 8) == INVALID            # not whole (scale, shift, gate) x 2 groups
    assert rc("sat_fourier_features", None, 0.5, None, P, 3, 128) == INVALID
    assert rc("sat_fold_in", P, None, P, 128, 64) == INVALID and rc("sat_fold_out", P, P, P, 0, 64) == INVALID
    assert rc("sat_pos_table", 3, P, P, 64, 128) == INVALID and rc("sat_pos_table", 1, P, P, 64, 127) == INVALID
    assert rc("sat_add_pos", P, P, 3, 50, 126) == UNSUPPORTED and rc("sat_add_pos", P, None, 3, 50, 128) == INVALID
    assert rc("sat_cfg_denoise", P, P, None, 2, 8, 150, 1, 6.5, 0.6, 1.0, 0.0) == INVALID
    assert rc("sat_cfg_denoise", P, P, P, 2, 1, 150, 1, 6.5, 0.6, 1.0, 0.0) == INVALID            # the unbiased std of one channel


def test_encoders_share_one_attention_launcher():
    """enc_attention.h holds the only launch of enc_attention_kernel; both encoders and the unit entry call it."""
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "friendly-stable-audio-tools_amd", "csrc")
    launches = {}
    for name in os.listdir(csrc):
        if name.endswith((".hip", ".h")):
            text = open(os.path.join(csrc, name)).read()
            launches[name] = (text.count("hipLaunchKernelGGL(enc_attention_kernel"), text.count("enc_attention_launch("))
    assert {n for n, (k, _) in launches.items() if k} == {"enc_attention.h"} and launches["enc_attention.h"][0] == 1
    assert launches["t5_encoder.hip"][1] == 2 and launches["roberta_encoder.hip"][1] == 1            # (the T5 file also holds the unit entry)
