"""The references and gates of tests/test_gpu_sampler_kernels.py, proven on the CPU (pattern: test_fp32_kernels_host.py): the restatements of
sampler_units agree with what they stand for -- the oracle's sampler, codec, conditioner and resampler, and plain loops of the Bartlett
cross-fade; the same restatements evaluated in float32 by PyTorch on the CPU pass every 1e-5 gate with a factor 4 to spare and every a-priori
bound as it stands; every fault these kernels can have is rejected by its gate, with a message that names kind, case and index, while the
whole-tensor rel-L2 stays under 1e-4; and the entries refuse, before any launch, what their kernels cannot do.  With SAT_PARITY_LOG set the
figures are appended to that file (profiles/sampler_kernels_verification.txt)."""
import math

import pytest
import torch
import torch.nn.functional as F

import sampler_units as su
from test_fp32_kernels_host import _close, _fails, _log, _outputs

F64 = torch.float64


def _cpu32(case):
    """The restatement in float32 on the CPU."""
    return _outputs(su.reference(case, torch.float32))


# ------------------------------------------------------------------------------------------------ the condition on the inputs
@pytest.mark.parametrize("kind", su.KINDS)
def test_fp32_cpu_evaluation_passes_every_gate(kind):
    """PyTorch's float32 evaluation of every case sits under a quarter of each 1e-5 gate, under the a-priori bound itself, under the derived
    bound of the error norm, and is bit-exact where the gate is: no case is there for which a gate would be meaningless."""
    for p in su.CASES[kind]:
        case = su.Case(kind, p)
        su.LOG.clear()
        su.check(case, _cpu32(case), headroom=0.25)
        for name, key, what, figure, where in su.LOG:
            _log(f"fp32 CPU\t{name}\t{key}\t{what}\t{figure:.3e}\t{where}")


def test_case_lists_hold_the_seams():
    """The shapes the gates are taken at: every seam the device test names is in the lists."""
    C, big = su.CASES, su.BIG
    assert big == 2048 * 256 + 257
    assert {len(p["terms"]) for p in C["lincomb"]} == {0, 1, 2, 3, 5}
    assert {p["n"] for p in C["lincomb"]} == {1, 255, 256, 257, big}
    assert {(p["n"], p["alias"]) for p in C["lincomb"] if p["alias"] != "-"} == {(n, a) for n in (257, big) for a in ("t0", "t3")}
    for p in C["lincomb"]:            # a NULL term carries a non-zero coefficient, the first of them NaN
        coef = su.Case("lincomb", dict(p, n=1)).dim["coef"]
        null = [coef[i] for i in range(5) if str(i) not in p["terms"]]
        assert all(c != 0.0 for c in null) and (not null or math.isnan(null[0]))
    assert {(p["n"], p["step"]) for p in C["dpmpp3m_update"]} == {(n, s) for n in (77, big) for s in ("first", "second", "steady", "last")}
    last = su.Case("dpmpp3m_update", dict(n=77, step="last"))
    assert last.dim["cn"] == 0.0 and last.t["noise"] is None and last.t["d1"] is not None and last.t["d2"] is not None
    first = su.Case("dpmpp3m_update", dict(n=77, step="first"))
    assert first.t["d1"] is None and first.t["d2"] is None and first.dim["c1"] == 0.0 and first.dim["c2"] == 0.0 and first.dim["cn"] != 0.0
    second = su.Case("dpmpp3m_update", dict(n=77, step="second"))
    assert second.t["d1"] is not None and second.t["d2"] is None and second.dim["c1"] != 0.0 and second.dim["c2"] == 0.0
    assert {(p["rows"], p["t"]) for p in C["inpaint_mix"]} == {(1, 1), (16, 77), (3, -(-524288 // 3) + 257)}
    assert {p["steps"] for p in C["inpaint_mix"]} == {3, 7, 100} and 3 * (-(-524288 // 3) + 257) > 524288
    for p in C["inpaint_mix"]:
        if p["t"] > 1:
            c = su.Case("inpaint_mix", p)
            below, at, above = su.mask_boundary(p["i"], p["steps"])
            assert below < at < above and at == c.dim["strength"]
            vals = set(c.t["mask"].tolist())
            assert {0.0, 1.0, below, at, above} <= vals
            assert c.t["mask"][-1].item() == at and c.t["mask"][-3].item() == below and c.t["mask"][-2].item() == above
    assert {(p["n"], p["parts"]) for p in C["dpm_error_partials"]} >= {(n, k) for n in (1, 1232, 256 * 64 + 5, big) for k in (1, 64, 1024, 4096)}
    assert {p["var"] for p in C["dpm_error_partials"]} == {"mixed", "atol", "rtol"}
    for var in ("atol", "rtol", "mixed"):
        c = su.Case("dpm_error_partials", dict(n=1232, parts=64, var=var))
        lo, prev = c.t["x_low"].abs(), c.t["x_prev"].abs()
        by_rtol = (c.dim["rtol"] * torch.maximum(lo, prev) > c.dim["atol"]).float().mean().item()
        assert by_rtol == {"atol": 0.0, "rtol": 1.0}.get(var, by_rtol) and (var != "mixed" or 0.2 < by_rtol < 0.98)
        assert 0.3 < (prev > lo).float().mean().item() < 0.7
    assert {(p["b"], p["c"], p["t"]) for p in C["cfg_combine"]} == {(1, 2, 1), (2, 8, 77), (3, 64, 257)}
    assert {(p["phi"], p["scale"]) for p in C["cfg_combine"]} == {(phi, s) for phi in (0.0, 0.6) for s in (1.0, 7.0)}
    assert {(p["b"], p["c"], p["t"]) for p in C["vae_sample"]} == {(1, 1, 1), (2, 4, 50), (3, 5, 333)}
    for p in C["vae_sample"]:
        c = su.Case("vae_sample", p)
        scale = c.t["ms"][:, p["c"]:]
        for pos, v in c.dim["planted"]:
            assert scale[pos].item() == torch.tensor(v, dtype=torch.float32).item()
        if p["s"] == "all":
            assert {v for _, v in c.dim["planted"]} == {-100.0, -20.0, 0.0, 19.999, 20.0, 20.001, 60.0}
    assert {p["s"] for p in C["vae_sample"] if p["t"] == 1} == {-100.0, -20.0, 0.0, 19.999, 20.0, 20.001, 60.0}
    assert {(p["b"], p["c"], p["t"], p["beta"]) for p in C["snake_beta"]} == {(b, c, t, be) for (b, c, t) in ((1, 1, 1), (3, 1, 7), (2, 5, 333), (1, 3, 1))
                                                                            for be in (-30.0, 0.0, 3.0)}
    for p in C["snake_beta"]:
        c = su.Case("snake_beta", p)
        assert c.t["beta"][0].item() == p["beta"] and (c.t["x"] * c.t["alpha"].exp().view(1, -1, 1)).abs().max() < 8.0
    assert {(p["count"], p["half"], p["features"]) for p in C["number_embed"]} == {(n, h, f) for n in (1, 5) for (h, f) in ((1, 1), (128, 768), (300, 257))}
    c = su.Case("number_embed", dict(count=5, half=128, features=768))
    v, lo, hi = c.t["values"], c.dim["min_val"], c.dim["max_val"]
    assert v[0] < lo and v[1] == lo and lo < v[2] < hi and v[3] == hi and v[4] > hi
    assert {p["n"] for p in C["float_to_int16"]} == {1, 4099, big}
    assert {(p["maximize"], p["peak"]) for p in C["float_to_int16"] if p["where"] != "zero"} == {(m, pk) for m in (0, 1) for pk in (0.3, 2.5)}
    assert {p["maximize"] for p in C["float_to_int16"] if p["where"] == "zero"} == {0, 1}
    c = su.Case("float_to_int16", dict(n=big, maximize=1, peak=2.5, where="last"))
    assert c.t["x"][-1].item() == -2.5 and c.t["x"][:-1].abs().max().item() < 2.5
    assert {(p["batch"], p["chunks"], p["c"], p["l"], p["hop"], p["ov"]) for p in C["overlap_add"]} == {
        (1, 1, 1, 16, 16, 4), (2, 3, 2, 32, 24, 8), (1, 4, 1, 32, 32, 0), (1, 3, 1, 32, 40, 4), (2, 5, 2, 64, 48, 16)}
    for p in C["overlap_add"]:
        assert su.Case("overlap_add", p).dim["total"] == p["hop"] * (p["chunks"] - 1) + p["l"] + p["extra"]
    assert {p["extra"] for p in C["overlap_add"]} == {0, 5}
    assert {(p["orig_sr"], p["new_sr"], p["rows"], p["in_len"]) for p in C["resample_sinc"]} == {
        (48000, 44100, 1, 1), (48000, 44100, 5, 159), (48000, 44100, 5, 161), (22050, 44100, 3, 100), (44100, 16000, 7, 883)}
    assert [p["short"] for p in C["resample_sinc"]].count(3) == 1
    for p in C["resample_sinc"]:
        d = su.Case("resample_sinc", p).dim
        assert d["out_len"] == math.ceil(p["in_len"] * d["new"] / d["orig"]) - p["short"] and d["out_len"] > 0


# ------------------------------------------------------------------------------------------------------------ the references
def test_dpmpp3m_reference_is_the_oracles_solver_step_by_step():
    """Five steps of oracle.sampler.sample_dpmpp_3m_sde on recorded denoiser outputs and injected noise: the state after every step is the
    update formula with the scalars of dpmpp3m_coefficients -- the first, second, steady and last pointer patterns of sample_k."""
    from oracle import sampler as osamp
    from stable_audio_tools.inference.sampling import dpmpp3m_coefficients
    g = torch.Generator().manual_seed(3)
    n, steps = 77, 5
    sig = osamp.get_sigmas_polyexponential(steps, 0.3, 80.0).double()
    den = [torch.randn(1, n, generator=g, dtype=F64) for _ in range(steps)]
    nz = [torch.randn(1, n, generator=g, dtype=F64) for _ in range(steps)]
    states = []
    it = iter(den)
    x0 = torch.randn(1, n, generator=g, dtype=F64) * 80.0
    osamp.sample_dpmpp_3m_sde(lambda x, s: next(it), x0, sig, lambda i, s, sn: nz[i], callback=lambda a: states.append(a["x"].clone()))
    it = iter(den)
    final = osamp.sample_dpmpp_3m_sde(lambda x, s: next(it), x0, sig, lambda i, s, sn: nz[i])
    states.append(final)
    coeffs = dpmpp3m_coefficients([float(s) for s in sig])
    seen = set()
    for i in range(steps):
        a, b, c1, c2, cn = coeffs[i]
        case = su.Case("dpmpp3m_update", dict(n=n, step="steady"))
        case.t.update(x=states[i][0], d=den[i][0], d1=den[i - 1][0] if i >= 1 else None, d2=den[i - 2][0] if i >= 2 else None,
                      noise=nz[i][0] if cn != 0.0 else None)
        case.dim.update(a=a, b=b, c1=c1, c2=c2, cn=cn)            # (float64 scalars: the formula, not its fp32 arguments)
        _close(su.reference(case)["x"], states[i + 1][0], 1e-12)
        seen.add((i >= 1 and c1 != 0.0, i >= 2 and c2 != 0.0, cn != 0.0))
    assert seen == {(False, False, True), (True, False, True), (True, True, True), (False, False, False)}


def test_cfg_reference_is_the_oracles_combine():
    """oracle.dit.dit_forward: cfg = uncond + (cond - uncond) * scale; with scale_phi: phi * (cfg * cond_std / cfg_std) + (1 - phi) * cfg."""
    for p in su.CASES["cfg_combine"]:
        c = su.Case("cfg_combine", p)
        d = c.dim
        mo = c.t["mo"].double()
        cond, unc = mo[:d["b"]], mo[d["b"]:]
        cfg = unc + (cond - unc) * d["cfg_scale"]
        if d["phi"] != 0.0:
            cfg = d["phi"] * (cfg * (cond.std(dim=1, keepdim=True) / cfg.std(dim=1, keepdim=True))) + (1 - d["phi"]) * cfg
        _close(su.reference(c)["out"], cfg)


def test_inpaint_reference_is_get_bmask_and_the_oracles_callback():
    """get_bmask of the reference, torch.where(mask <= (i + 1) / steps, 1, 0) on the float32 mask, element for element -- the boundary value
    and its two float32 neighbours included -- and the callback's x <- (init + noise sigma) bm + x (1 - bm)."""
    from oracle import sampler as osamp
    for p in su.CASES["inpaint_mix"]:
        if p["t"] > 1000:
            continue
        c = su.Case("inpaint_mix", p)
        t, d = c.t, c.dim
        bm = osamp.get_bmask(p["i"], p["steps"], t["mask"])
        ref = su.reference(c)
        assert torch.equal(bm.bool().view(1, -1).expand(p["rows"], p["t"]), ref["x:keep"])
        below, at, above = su.mask_boundary(p["i"], p["steps"])
        for v, kept in ((below, 1), (at, 1), (above, 0), (0.0, 1)):
            assert int(osamp.get_bmask(p["i"], p["steps"], torch.tensor([v], dtype=torch.float32))) == kept
        x = t["x"].double().view(1, p["rows"], p["t"]).clone()
        _, callback = osamp.inpainting_start_and_callback(t["init"].double()[None], torch.zeros(1, p["rows"], p["t"], dtype=F64), t["mask"], p["steps"], lambda i: t["noise"].double()[None])
        callback({"i": p["i"], "x": x, "sigma": d["sigma"]})
        _close(ref["x"], x[0])


def test_snake_and_vae_references_are_the_oracles():
    from oracle import oobleck as oob
    for p in su.CASES["snake_beta"]:
        c = su.Case("snake_beta", p)
        _close(su.reference(c)["y"], oob.snake_beta(c.t["x"].double(), c.t["alpha"].double(), c.t["beta"].double()))
    for p in su.CASES["vae_sample"]:
        c = su.Case("vae_sample", p)
        _close(su.reference(c)["z"], oob.vae_sample(c.t["ms"].double(), c.t["noise"].double()))
    x = torch.tensor([-100.0, -20.0, 0.0, 19.999, 20.0, 20.001, 60.0, 100.0], dtype=F64)
    assert torch.equal(su.softplus(x), F.softplus(x))


def test_number_embed_reference_is_the_oracles_conditioner():
    from oracle import conditioners as ocond
    for p in su.CASES["number_embed"]:
        c = su.Case("number_embed", p)
        sd = {"embedder.embedding.0.weights": c.t["w"].double(), "embedder.embedding.1.weight": c.t["lw"].double(),
              "embedder.embedding.1.bias": c.t["lb"].double()}
        old = torch.get_default_dtype()
        torch.set_default_dtype(F64)            # (the oracle builds its value tensor in the default dtype)
        try:
            emb, mask = ocond.number_conditioner(sd, "", c.t["values"].tolist(), c.dim["min_val"], c.dim["max_val"])
        finally:
            torch.set_default_dtype(old)
        assert emb.shape == (p["count"], 1, p["features"]) and bool((mask == 1).all())
        _close(su.reference(c)["out"], emb[:, 0])


def test_resample_reference_is_the_oracles_resampler():
    from oracle import resample as oresample
    for p in su.CASES["resample_sinc"]:
        c = su.Case("resample_sinc", p)
        want = torch.from_numpy(oresample.resample(c.t["x"].numpy(), p["orig_sr"], p["new_sr"]))
        assert want.shape[-1] == c.dim["out_len"] + p["short"]
        _close(su.reference(c)["y"], want[:, :c.dim["out_len"]], 1e-12)
        assert c.t["bank"].shape == (c.dim["new"], 2 * c.dim["width"] + c.dim["orig"])


def _crossfade_loop(pieces, hop, ov, total):
    """The Bartlett cross-fade sample by sample: out[t] = sum over the chunks that cover t of piece[t - i hop] times its fade."""
    b, n, c, l = pieces.shape
    win = torch.bartlett_window(2 * ov, dtype=F64) if ov else None
    out = torch.zeros((b, c, total), dtype=F64)
    for t in range(total):
        for i in range(n):
            off = t - i * hop
            if 0 <= off < l:
                w = 1.0
                if i != 0 and off < ov:
                    w *= float(win[off])
                if i != n - 1 and off >= l - ov:
                    w *= float(win[ov + off - (l - ov)])
                out[:, :, t] += pieces[:, i, :, off].double() * w
    return out


def test_overlap_add_reference_is_the_crossfade_loop():
    for p in su.CASES["overlap_add"]:
        c = su.Case("overlap_add", p)
        ref = su.reference(c)
        _close(ref["out"], _crossfade_loop(c.t["pieces"], p["hop"], p["ov"], c.dim["total"]))
        covered = ref["out:n"] > 0
        assert bool((ref["out"][~covered] == 0).all()) and int(ref["out:n"].max()) <= 2
        assert bool((~covered).any()) == (p["extra"] > 0 or p["hop"] > p["l"])


@pytest.mark.parametrize("chunk,overlap,length,ratio", [(8, 2, 8, 4), (8, 2, 20, 4), (8, 2, 21, 1), (16, 4, 100, 2), (8, 4, 30, 3), (6, 1, 6, 2), (8, 0, 24, 2)])
def test_overlap_add_reference_is_the_chunked_codec(chunk, overlap, length, ratio):
    """What AudioAutoencoder._run_chunked hands to the entry -- hop = chunk - overlap, total = hop (n_chunk - 1) + chunk, in latent frames or in
    samples -- for the three chunked paths of the oracle (decode_audio, encode_audio, reconstruct_audio) with a codec that returns recorded pieces."""
    from oracle import oobleck as oob
    g = torch.Generator().manual_seed(chunk * 100 + length)
    hop = chunk - overlap
    n_chunk = int(math.ceil((length - chunk) / hop)) + 1
    if overlap:
        # decode: latents [2, 3, length] -> audio of `ratio` samples per frame
        pieces = torch.randn(2, n_chunk, 2, chunk * ratio, generator=g, dtype=F64)
        calls = iter(range(n_chunk))
        if (chunk + hop * (n_chunk - 1) - length) < length:            # (reflect padding needs a pad shorter than the signal)
            got = oob.decode_audio_chunked(lambda z: pieces[:, next(calls)], torch.zeros(2, 3, length), chunk, overlap, ratio)
            win = torch.bartlett_window(2 * overlap * ratio, dtype=F64)
            want = su.overlap_add(pieces, win, hop * ratio, overlap * ratio, hop * ratio * (n_chunk - 1) + chunk * ratio)[..., :length * ratio]
            _close(got, want.float(), 1e-6)
        # encode: audio [2, 2, length * ratio] -> latents
        pieces = torch.randn(2, n_chunk, 3, chunk, generator=g, dtype=F64)
        calls = iter(range(n_chunk))
        got = oob.encode_audio_chunked(lambda a: pieces[:, next(calls)], torch.zeros(2, 2, length * ratio), chunk, overlap, ratio, 3)
        want = su.overlap_add(pieces, torch.bartlett_window(2 * overlap, dtype=F64), hop, overlap, hop * (n_chunk - 1) + chunk)[..., :length]
        _close(got, want.float(), 1e-6)
        # reconstruct: audio -> audio, chunk * ratio samples per window
        cs, ov_s = chunk * ratio, overlap * ratio
        hop_s = cs - ov_s
        n_s = int(math.ceil((length * ratio - cs) / hop_s)) + 1
        pieces = torch.randn(2, n_s, 2, cs, generator=g, dtype=F64)
        got = oob.reconstruct_audio_chunked(lambda a, i: pieces[:, i], torch.zeros(2, 2, length * ratio), chunk, overlap, ratio)
        want = su.overlap_add(pieces, torch.bartlett_window(2 * ov_s, dtype=F64), hop_s, ov_s, hop_s * (n_s - 1) + cs)[..., :length * ratio]
        _close(got, want.float(), 1e-6)
    else:
        # no overlap: the chunks abut, the window (bartlett_window(2), which _run_chunked still uploads) is never applied
        pieces = torch.randn(2, n_chunk, 2, chunk, generator=g, dtype=F64)
        want = su.overlap_add(pieces, torch.bartlett_window(2, dtype=F64), hop, 0, hop * (n_chunk - 1) + chunk)
        assert torch.equal(want, pieces.permute(0, 2, 1, 3).reshape(2, 2, n_chunk * chunk))


def test_dpm_error_reference_is_the_oracles_norm():
    """oracle.sampler.sample_dpm_adaptive: error = ||(x_low - x_high) / max(atol, rtol max(|x_low|, |x_prev|))|| / sqrt(n) = sqrt(sum(partials) / n)."""
    for p in su.CASES["dpm_error_partials"]:
        if p["n"] > 20000:
            continue
        c = su.Case("dpm_error_partials", p)
        lo, hi, prev = (c.t[k].double() for k in ("x_low", "x_high", "x_prev"))
        delta = torch.maximum(torch.tensor(c.dim["atol"], dtype=F64), c.dim["rtol"] * torch.maximum(lo.abs(), prev.abs()))
        error = torch.linalg.norm((lo - hi) / delta) / p["n"] ** 0.5
        part = su.reference(c)["partial"]
        assert part.shape == (p["parts"],)
        assert abs(math.sqrt(part.sum().item() / p["n"]) - error.item()) <= 1e-12 * error.item()
        assert bool((part[-(-p["n"] // 256):] == 0).all())
        last = ((lo[-1] - hi[-1]) / delta[-1]).pow(2).item()
        assert p["n"] == 1 or 0.05 < last / part.sum().item() < 0.2            # dropping the last element moves the sum far beyond any bound here


def test_dpm_error_bound_figures():
    """The derived bound at the shapes of the list: 24 units without a chain (one element per thread at most), 2073 for one block over BIG."""
    assert su.dpm_error_bound(1, 4096) == pytest.approx(1.01 * 24 * 2.0 ** -24)
    assert su.dpm_error_bound(su.BIG, 1) == pytest.approx(1.01 * (23 + 2050) * 2.0 ** -24)
    assert su.dpm_error_bound(su.BIG, 1024) == pytest.approx(1.01 * 26 * 2.0 ** -24)
    for p in su.CASES["dpm_error_partials"]:
        _log(f"derived dpm_error bound\t{su.case_id(p)}\t{su.dpm_error_bound(p['n'], p['parts']):.3e}")


def test_int16_reference_truncates_and_silence_is_zero():
    c = su.Case("float_to_int16", dict(n=4099, maximize=1, peak=2.5, where="last"))
    want = su.reference(c)["out"]
    assert want[-1].item() == -32767 and want.abs().max().item() == 32767
    exact = c.t["x"].double() / 2.5 * 32767
    assert bool(((want.double() - exact).abs() < 1.0 + 1e-2).all()) and bool((want.double().abs() <= exact.abs() + 1e-2).all())
    for m in (0, 1):
        c = su.Case("float_to_int16", dict(n=4099, maximize=m, peak=0.0, where="zero"))
        assert not su.reference(c)["out"].any()
    c = su.Case("float_to_int16", dict(n=4099, maximize=0, peak=0.3, where="rand"))
    assert su.reference(c)["out"].abs().max().item() == int(0.3 * 32767)


# ------------------------------------------------------------------------------------------------------------ planted faults
def _whole(faulty, want):
    return max(((faulty[k].double() - want[k].double()).norm() / want[k].double().norm().clamp_min(1e-300)).item() for k in faulty)


def _rejected(case, faulty, want, what, needle=None):
    """``faulty`` fails the case's gates, with a message that names kind, case and an index, although its whole-tensor rel-L2 stays under
    the model tests' gate."""
    whole = _whole(faulty, want)
    msg = _fails(su.check, case, faulty, want)
    _log(f"planted\t{what}\twhole rel-L2 {whole:.3e}\trejected: {bool(msg)}\t{(msg or '')[:160]}")
    assert whole < su.MODEL_GATE, f"{what}: whole-tensor rel-L2 {whole:.3e} would not pass a whole-tensor gate either"
    assert msg is not None, f"{what}: the gates accept it (whole-tensor rel-L2 {whole:.3e})"
    assert case.name in msg and any(ch.isdigit() for ch in msg.split(case.name, 1)[1]), f"{what}: the message names no case or index: {msg}"
    if needle:
        assert needle in msg, msg
    return msg


def _correct(case):
    """A correct result to plant a fault into: the float32 evaluation, which passes."""
    want = su.reference(case)
    got = _cpu32(case)
    su.check(case, got, want)
    return got, want


def test_rejects_a_stale_last_element_of_the_strided_pass():
    """out aliases t0 and the update is small (c0 = 1): the very last element, the tail of the second pass, keeps what it held."""
    case = su.Case("lincomb", dict(n=su.BIG, terms="01234", alias="t0"))
    case.dim["coef"] = tuple(su._f32(c) for c in (1.0, 0.01, 0.005, -0.003, 0.002))
    got, want = _correct(case)
    bad = {"out": got["out"].clone()}
    bad["out"][-1] = case.t["t0"][-1]
    assert str(su.BIG - 1) in _rejected(case, bad, want, "lincomb last tail element stale", "a-priori bound")
    # the same in the in-place solver update
    case = su.Case("dpmpp3m_update", dict(n=su.BIG, step="steady"))
    case.dim.update({k: su._f32(v) for k, v in dict(a=1.0, b=0.01, c1=0.004, c2=-0.003, cn=0.002).items()})
    got, want = _correct(case)
    bad = {"x": got["x"].clone()}
    bad["x"][-1] = case.t["x"][-1]
    assert str(su.BIG - 1) in _rejected(case, bad, want, "dpmpp3m_update last tail element stale", "a-priori bound")


def test_rejects_less_than_at_the_mask_boundary():
    """x is 1e-4 from what the mix gives: a kernel that keeps `mask < strength` leaves the frames AT the boundary as they were."""
    case = su.Case("inpaint_mix", dict(rows=16, t=77, steps=7, i=2))
    t, d = case.t, case.dim
    t["x"] = t["init"] + t["noise"] * d["sigma"] + 1e-4 * torch.randn(16, 77, generator=torch.Generator().manual_seed(11))
    got, want = _correct(case)
    at = t["mask"] == torch.tensor(d["strength"], dtype=torch.float32)
    assert int(at.sum()) == 3
    bad = {"x": got["x"].clone()}
    bad["x"][:, at] = t["x"][:, at]
    _rejected(case, bad, want, "inpaint_mix < instead of <= at the boundary", "a-priori bound")
    # and the other way round: a frame one float32 above the boundary overwritten
    above = t["mask"] == su.mask_boundary(2, 7)[2]
    bad = {"x": got["x"].clone()}
    bad["x"][3, above] = (t["init"] + t["noise"] * d["sigma"])[3, above]
    _rejected(case, bad, want, "inpaint_mix a frame above the boundary overwritten")


def _quiet_fades(case):
    """The faded regions of every chunk are 1e-4 of the rest, so that a wrong fade stays far below any whole-tensor figure."""
    ov, l = case.p["ov"], case.p["l"]
    case.t["pieces"][..., :ov] *= 1e-4
    case.t["pieces"][..., l - ov:] *= 1e-4


def test_rejects_a_fade_on_the_first_chunk_and_a_fade_index_off_by_one():
    case = su.Case("overlap_add", dict(batch=2, chunks=3, c=2, l=32, hop=24, ov=8, extra=0))
    _quiet_fades(case)
    got, want = _correct(case)
    d, win = case.dim, case.t["window"]
    faded = case.t["pieces"].clone()
    faded[:, 0, :, :8] *= win[:8]
    bad = {"out": su.overlap_add(faded, win, d["hop"], d["ov"], d["total"])}
    msg = _rejected(case, bad, want, "overlap_add fade-in applied to the first chunk", "a-priori bound")
    assert "first at (0, 0, 0)" in msg
    faded = case.t["pieces"].clone()
    faded[:, 2, :, 24:] *= win[8:]
    bad = {"out": su.overlap_add(faded, win, d["hop"], d["ov"], d["total"])}
    _rejected(case, bad, want, "overlap_add fade-out applied to the last chunk", "a-priori bound")
    shifted = win.clone()
    shifted[:8] = win[1:9]
    bad = {"out": su.overlap_add(case.t["pieces"], shifted, d["hop"], d["ov"], d["total"])}
    _rejected(case, bad, want, "overlap_add fade-in index off by one", "a-priori bound")


def _smooth_rows(case):
    """A very slow sinusoid per row: neighbouring outputs (one filter phase, 160 / 147 of a sample, apart) differ by a few 1e-4 of it."""
    rows, n = case.p["rows"], case.p["in_len"]
    i = torch.arange(n, dtype=torch.float32)
    case.t["x"] = torch.stack([torch.sin(2 * math.pi * i / (9000.0 + 700 * r) + r) for r in range(rows)])


def test_rejects_a_neighbouring_phase_and_a_neighbouring_row():
    case = su.Case("resample_sinc", dict(orig_sr=48000, new_sr=44100, rows=5, in_len=161, short=0))
    _smooth_rows(case)
    got, want = _correct(case)
    d = case.dim
    args = (d["in_len"], d["out_len"], d["orig"], d["new"], d["width"])
    other = su.resample_frames(case.t["x"], case.t["bank"].roll(-1, 0), *args)
    diff = (other[2] - got["y"][2]).abs()
    diff[:20], diff[120:] = 0.0, 0.0            # (away from the two ends, where the signal is cut off and nothing is smooth)
    j = int(diff.argmax())
    bad = {"y": got["y"].clone()}
    bad["y"][2, j] = other[2, j]
    assert f"(2, {j})" in _rejected(case, bad, want, f"resample_sinc the next phase's filter used for output {j} of one row", "a-priori bound")
    case.t["x"][3] = case.t["x"][2] * (1.0 + 1.5e-4)
    got, want = _correct(case)
    bad = {"y": got["y"].clone()}
    bad["y"][3] = got["y"][2]
    assert "(3," in _rejected(case, bad, want, "resample_sinc row 3 read from row 2", "a-priori bound")


def test_rejects_a_clamped_sample_behind_the_last_one():
    case = su.Case("resample_sinc", dict(orig_sr=48000, new_sr=44100, rows=5, in_len=161, short=0))
    _smooth_rows(case)
    case.t["x"][:, -1] = 2e-3
    got, want = _correct(case)
    d = case.dim
    ext = d["width"] + d["orig"]
    clamped = torch.cat((case.t["x"], case.t["x"][:, -1:].expand(5, ext)), dim=1)
    bad = {"y": su.resample_frames(clamped, case.t["bank"], d["in_len"] + ext, d["out_len"], d["orig"], d["new"], d["width"])}
    assert int((bad["y"] != got["y"]).sum()) > 0
    _rejected(case, bad, want, "resample_sinc zero padding behind the signal replaced by the last sample", "a-priori bound")
    # the same in front of sample 0
    case.t["x"][:, 0] = 2e-3
    got, want = _correct(case)
    clamped = torch.cat((case.t["x"][:, :1].expand(5, d["width"]), case.t["x"]), dim=1)
    taps = 2 * d["width"] + d["orig"]
    bad = {"y": got["y"].clone()}
    bad["y"][:, :d["new"]] = torch.einsum("rt,pt->rp", F.pad(clamped, (0, taps))[:, :taps], case.t["bank"])            # frame 0 is the only one that starts before sample 0
    _rejected(case, bad, want, "resample_sinc zero padding in front of the signal replaced by the first sample", "a-priori bound")


def test_rejects_rounding_and_a_peak_that_misses_the_last_element():
    case = su.Case("float_to_int16", dict(n=4099, maximize=1, peak=2.5, where="rand"))
    g = torch.Generator().manual_seed(12)
    case.t["x"] = (torch.rand(4099, generator=g) * 2.0 - 1.0) * 2.5
    got, want = _correct(case)
    div = case.t["x"].abs().max().item()
    bad = {"out": case.t["x"].div(div).mul(32767).round().to(torch.int16)}
    _rejected(case, bad, want, "float_to_int16 round-to-nearest instead of truncation", "samples differ")
    case = su.Case("float_to_int16", dict(n=4099, maximize=1, peak=2.5, where="last"))
    x = case.t["x"]
    x[:-1] *= (2.5 / (1.0 + 5e-5)) / x[:-1].abs().max()            # the last element is the peak by 5e-5 only
    got, want = _correct(case)
    div = x[:-1].abs().max().item()
    bad = {"out": x.div(div).mul(32767).clamp(-32767, 32767).to(torch.int16)}
    _rejected(case, bad, want, "float_to_int16 peak taken without the last element", "samples differ")


def test_rejects_a_snake_channel_taken_from_the_wrong_index():
    case = su.Case("snake_beta", dict(b=2, c=5, t=333, beta=0.0))
    case.t["alpha"][:] = 0.1
    case.t["beta"] = 6e-5 * torch.arange(5, dtype=torch.float32)            # neighbouring channels 6e-5 apart
    got, want = _correct(case)
    x = case.t["x"]
    ch = (torch.arange(x.numel()) % 5).view(x.shape)            # i % C in place of (i / T) % C
    bad = {"y": x + torch.sin(x * case.t["alpha"].exp()[ch]).pow(2) / (case.t["beta"].exp()[ch] + 1e-9)}
    _rejected(case, bad, want, "snake_beta channel i % C", "per element")


def test_rejects_a_softplus_that_treats_60_as_below_its_threshold():
    """A softplus that clamps its argument to the threshold, exp(min(scale, 20)), reads 60 as 20.  (Dropping the threshold altogether cannot be
    seen at 60: float32 holds exp(60), and log1p of it is 60 to the last bit -- that form only breaks where exp overflows, beyond 88.)"""
    case = su.Case("vae_sample", dict(b=3, c=5, t=333, s="all"))
    at60 = [pos for pos, v in case.dim["planted"] if v == 60.0]
    for pos in at60:
        case.t["noise"][pos] = 1e-4            # its deviation of 60 times a noise of 1e-4: tiny against the tensor, large against 1e-5
    got, want = _correct(case)
    mean, scale = case.t["ms"].chunk(2, dim=1)
    bad = {"z": case.t["noise"] * (torch.log1p(torch.exp(scale.clamp(max=20.0))) + 1e-4) + mean}
    assert int((bad["z"] != got["z"]).sum()) <= 2 + len(at60)
    msg = _rejected(case, bad, want, "vae_sample softplus clamped at its threshold, scale 60", "per element")
    assert str(at60[0]) in msg or str(at60[1]) in msg
    naive = torch.log1p(torch.exp(torch.tensor(60.0)))
    _log(f"softplus without a threshold at 60 in float32: {naive.item()!r} (differs from 60 by {abs(naive.item() - 60.0):.1e})")
    assert naive.item() == 60.0


def test_rejects_an_idle_partial_left_as_it_was_and_a_dropped_last_element():
    case = su.Case("dpm_error_partials", dict(n=1232, parts=64, var="mixed"))
    got, want = _correct(case)
    bad = {"partial": got["partial"].clone()}
    bad["partial"][40] = 1e-30            # block 40 of 64 owns no element of 1232: whatever the buffer held is still there
    assert "partial 40" in _rejected(case, bad, want, "dpm_error_partials idle partial stale", "without an element")
    bad["partial"][40] = math.nan
    assert "not written" in _fails(su.check, case, bad, want)
    case = su.Case("dpm_error_partials", dict(n=su.BIG, parts=1024, var="mixed"))
    got, want = _correct(case)
    lo, hi, prev = (case.t[k] for k in ("x_low", "x_high", "x_prev"))
    delta = torch.clamp(case.dim["rtol"] * torch.maximum(lo[-1].abs(), prev[-1].abs()), min=case.dim["atol"])
    bad = {"partial": got["partial"].clone()}
    bad["partial"][(su.BIG - 1) // 256 % 1024] -= ((lo[-1] - hi[-1]) / delta).pow(2)
    msg = _fails(su.check, case, bad, want)
    _log(f"planted\tdpm_error_partials last element dropped\t{msg}")
    assert msg and "derived bound" in msg and case.name in msg


def test_rejects_a_dropped_c2_term():
    case = su.Case("dpmpp3m_update", dict(n=77, step="steady"))
    case.dim["c2"] = su._f32(3e-5)
    got, want = _correct(case)
    t, d = case.t, case.dim
    bad = {"x": d["a"] * t["x"] + d["b"] * t["d"] + d["c1"] * (t["d"] - t["d1"]) + d["cn"] * t["noise"]}
    _rejected(case, bad, want, "dpmpp3m_update c2 term dropped", "a-priori bound")


# -------------------------------------------------------------------------------------------------------------- the refusals
def test_entries_refuse_what_their_kernels_cannot_do():
    """Decided before any launch, so without a device: SAT_E_INVALID (-1) for NULL pointers, non-positive sizes, more than 4096 partials, an
    output longer than ceil(in_len new / orig), an overlap longer than the chunk, max_val <= min_val, a non-zero coefficient without its
    tensor -- and c2 != 0 without d1, whose term (d1 - d2) the kernel would otherwise drop."""
    from stable_audio_tools import _hip
    lib = _hip.lib()
    keep = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda") if torch.cuda.is_available() else None
    P = keep.data_ptr() if keep is not None else 1 << 20
    INVALID = -1

    def rc(entry, *args):
        return getattr(lib, entry)(*args, None)

    def each_null(entry, args, pointers):
        for i in pointers:
            a = list(args)
            a[i] = None
            assert rc(entry, *a) == INVALID, (entry, i)

    def each_bad(entry, args, sizes, values=(0, -1)):
        for i in sizes:
            for v in values:
                a = list(args)
                a[i] = v
                assert rc(entry, *a) == INVALID, (entry, i, v)

    lin = [P, P, 1.0, None, 0.0, None, 0.0, None, 0.0, None, 0.0, 10]
    each_null("sat_lincomb", lin, [0])
    each_bad("sat_lincomb", lin, [11])
    upd = [P, P, P, P, P, 0.5, 0.5, 0.1, 0.1, 0.1, 10]
    each_null("sat_dpmpp3m_update", upd, [0, 1, 2, 3, 4])
    each_bad("sat_dpmpp3m_update", upd, [10])
    assert rc("sat_dpmpp3m_update", P, P, None, P, P, 0.5, 0.5, 0.0, 0.1, 0.1, 10) == INVALID            # c2 (d1 - d2) without d1
    assert b"c2" in lib.sat_last_error() and b"d1" in lib.sat_last_error()
    mix = [P, P, P, P, 1.0, 0.5, 4, 16]
    each_null("sat_inpaint_mix", mix, [0, 1, 2, 3])
    each_bad("sat_inpaint_mix", mix, [6, 7])
    err = [P, P, P, 0.01, 0.01, 10, P, 64]
    each_null("sat_dpm_error_partials", err, [0, 1, 2, 6])
    each_bad("sat_dpm_error_partials", err, [5, 7])
    each_bad("sat_dpm_error_partials", err, [7], (4097, 1 << 20))
    cfg = [P, P, 2, 8, 16, 7.0, 0.0]
    each_null("sat_cfg_combine", cfg, [0, 1])
    each_bad("sat_cfg_combine", cfg, [2, 3, 4])
    vae = [P, P, P, 2, 4, 16]
    each_null("sat_vae_sample", vae, [0, 1, 2])
    each_bad("sat_vae_sample", vae, [3, 4, 5])
    snake = [P, P, P, P, 2, 4, 16]
    each_null("sat_snake_beta", snake, [0, 1, 2, 3])
    each_bad("sat_snake_beta", snake, [4, 5, 6])
    num = [P, 2, 0.0, 512.0, P, 8, P, P, 16, P]
    each_null("sat_number_embed", num, [0, 4, 6, 7, 9])
    each_bad("sat_number_embed", num, [1, 5, 8])
    each_bad("sat_number_embed", num, [3], (0.0, -1.0))            # max_val == min_val, max_val < min_val
    i16 = [P, P, 10, 0, P]
    each_null("sat_float_to_int16", i16, [0, 1, 4])
    each_bad("sat_float_to_int16", i16, [2])
    ola = [P, P, P, 1, 3, 2, 32, 24, 8, 80]
    each_null("sat_overlap_add", ola, [0, 1, 2])
    each_bad("sat_overlap_add", ola, [3, 4, 5, 6, 7, 9])
    each_bad("sat_overlap_add", ola, [8], (33, -1))            # overlap > chunk_len
    rs = [P, P, P, 2, 161, 148, 160, 147, 7]
    each_null("sat_resample_sinc", rs, [0, 1, 2])
    each_bad("sat_resample_sinc", rs, [3, 4, 5, 6, 7])
    each_bad("sat_resample_sinc", rs, [5], (149, 1 << 20))            # ceil(161 * 147 / 160) = 148
    assert b"148" in lib.sat_last_error()
    each_bad("sat_resample_sinc", rs, [8], (-1,))
