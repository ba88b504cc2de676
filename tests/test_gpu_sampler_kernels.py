"""Every kernel that runs outside the DiT blocks -- in the sampler loop (lincomb, dpmpp3m_update, inpaint_mix, dpm_error_partials, cfg_combine),
in the conditioning (number_embed, vae_sample, snake_beta) and at the audio boundary (float_to_int16, overlap_add, resample_sinc) -- alone,
through its entry of include/sat_hip.h, against float64 PyTorch on the same fp32 inputs.

Gates (tests/sampler_units.py): linear forms element by element under the a-priori bound (n + 4) 2^-24 sum |c| |t|; the error norm's partials
under the bound derived there, every partial written and the idle ones exactly 0.0; the transcendental kernels at 1e-5 per element and per
(batch, channel) row; the int16 samples and everything a kernel must leave alone bit for bit.  Every output sits in a NaN (0xA5 for int16) guard
band; an entry that works in place gets a copy of the input.  The sizes include 2048 x 256 + 257 elements, where the kernels that cap their
grid at 2048 workgroups walk a second, partial pass.  That the references are right, that the fp32 evaluation on the CPU passes every gate and
that the gates reject the faults these kernels can have: tests/test_sampler_kernels_host.py.  Figures: profiles/sampler_kernels_verification.txt
(written with SAT_PARITY_LOG set).  The whole file, 135 cases, takes 2.3 s on an MI355X, 1.2 s of it the first call's device start-up."""
import pytest
import torch

import sampler_units as su
from test_gpu_fp32_kernels import _Call
from util import PARITY_LOG, assert_bit_equal

pytestmark = pytest.mark.gpu

PITCH = 16            # flat outputs: guard bands of 256 x 16 elements


def _cases(kind):
    return pytest.mark.parametrize("p", su.CASES[kind], ids=su.case_id)


def _finish(case, got):
    su.LOG.clear()
    try:
        su.check(case, {k: v.cpu() for k, v in got.items()})
    finally:
        if PARITY_LOG:
            with open(PARITY_LOG, "a") as f:
                for name, key, what, figure, where in su.LOG:
                    f.write(f"sampler_units\tdevice\t{name}\t{key}\t{what}\t{figure:.3e}\t{where}\n")


# ------------------------------------------------------------------------------------------------------------------ sampler loop
@_cases("lincomb")
def test_lincomb(dev, p):
    """0 to 5 terms with NULLs in between (whose coefficients, NaN among them, must not count), out aliasing the first or the fourth term, one
    element to 2048 x 256 + 257."""
    c = su.Case("lincomb", p)
    t, d = c.t, c.dim
    k = _Call(dev)
    alias = p["alias"] if p["alias"] != "-" else None
    g = k.out((d["n"],), "lincomb out", init=t[alias] if alias else None, pitch=PITCH)
    args = []
    for i in range(5):
        args += [g.t.data_ptr() if alias == f"t{i}" else k.up(t[f"t{i}"]), d["coef"][i]]
    k.call("sat_lincomb", g.t.data_ptr(), *args, d["n"])
    g.assert_written()
    _finish(c, {"out": g.t})


@_cases("dpmpp3m_update")
def test_dpmpp3m_update(dev, p):
    """The four pointer patterns of sample_k (no history, one, two, and the step onto sigma = 0 without noise), in place on a copy of x."""
    c = su.Case("dpmpp3m_update", p)
    t, d = c.t, c.dim
    k = _Call(dev)
    g = k.out((d["n"],), "dpmpp3m_update x", init=t["x"], pitch=PITCH)
    k.call("sat_dpmpp3m_update", g.t.data_ptr(), k.up(t["d"]), k.up(t["d1"]), k.up(t["d2"]), k.up(t["noise"]), d["a"], d["b"], d["c1"], d["c2"],
           d["cn"], d["n"])
    g.assert_written()
    _finish(c, {"x": g.t})


@_cases("inpaint_mix")
def test_inpaint_mix(dev, p):
    """Masks that hold 0, 1, the float32 of (i + 1) / steps and its two neighbours at the front, in the middle and in the last frames; what the
    mask does not keep is bit-identical to the input."""
    c = su.Case("inpaint_mix", p)
    t, d = c.t, c.dim
    k = _Call(dev)
    g = k.out((d["rows"], d["t"]), "inpaint_mix x", init=t["x"], pitch=PITCH)
    k.call("sat_inpaint_mix", g.t.data_ptr(), k.up(t["init"]), k.up(t["noise"]), k.up(t["mask"]), d["sigma"], d["strength"], d["rows"], d["t"])
    g.assert_written()
    _finish(c, {"x": g.t})


@_cases("dpm_error_partials")
def test_dpm_error_partials(dev, p):
    """1 to 4096 partials over 1 to 2048 x 256 + 257 elements into a NaN-filled buffer: every partial written, the idle ones exactly 0.0."""
    c = su.Case("dpm_error_partials", p)
    t, d = c.t, c.dim
    k = _Call(dev)
    g = k.out((d["parts"],), "dpm_error_partials partial", pitch=PITCH)
    k.call("sat_dpm_error_partials", k.up(t["x_low"]), k.up(t["x_high"]), k.up(t["x_prev"]), d["atol"], d["rtol"], d["n"], g.t.data_ptr(), d["parts"])
    _finish(c, {"partial": g.t})


@_cases("cfg_combine")
def test_cfg_combine(dev, p):
    c = su.Case("cfg_combine", p)
    d = c.dim
    k = _Call(dev)
    g = k.out((d["b"], d["c"], d["t"]), "cfg_combine out", pitch=d["t"])
    k.call("sat_cfg_combine", k.up(c.t["mo"]), g.t.data_ptr(), d["b"], d["c"], d["t"], d["cfg_scale"], d["phi"])
    g.assert_written()
    _finish(c, {"out": g.t})


# ------------------------------------------------------------------------------------------------------------------ conditioning
@_cases("vae_sample")
def test_vae_sample(dev, p):
    """[b, 2c, t] split into mean and scale at three layouts, scales at -100, -20, 0, 19.999, 20, 20.001 and 60 in known places."""
    c = su.Case("vae_sample", p)
    d = c.dim
    k = _Call(dev)
    g = k.out((d["b"], d["c"], d["t"]), "vae_sample z", pitch=d["t"])
    k.call("sat_vae_sample", k.up(c.t["ms"]), k.up(c.t["noise"]), g.t.data_ptr(), d["b"], d["c"], d["t"])
    g.assert_written()
    _finish(c, {"z": g.t})


@_cases("snake_beta")
def test_snake_beta(dev, p):
    c = su.Case("snake_beta", p)
    d = c.dim
    k = _Call(dev)
    g = k.out((d["b"], d["c"], d["t"]), "snake_beta y", pitch=d["t"])
    k.call("sat_snake_beta", k.up(c.t["x"]), k.up(c.t["alpha"]), k.up(c.t["beta"]), g.t.data_ptr(), d["b"], d["c"], d["t"])
    g.assert_written()
    _finish(c, {"y": g.t})


@_cases("number_embed")
def test_number_embed(dev, p):
    """One value and five (below, at and above the range), 1, 128 and 300 frequencies (a second pass of 44), 1, 768 and 257 features."""
    c = su.Case("number_embed", p)
    t, d = c.t, c.dim
    k = _Call(dev)
    g = k.out((d["count"], d["features"]), "number_embed out")
    k.call("sat_number_embed", k.up(t["values"]), d["count"], d["min_val"], d["max_val"], k.up(t["w"]), d["half"], k.up(t["lw"]), k.up(t["lb"]),
           d["features"], g.t.data_ptr())
    g.assert_written()
    _finish(c, {"out": g.t})


# ---------------------------------------------------------------------------------------------------------------- audio boundary
@_cases("float_to_int16")
def test_float_to_int16(dev, p):
    """Bit-exact against the CPU; the peak negative and in the very last element, scratch full of 0xFF, silence under both settings."""
    c = su.Case("float_to_int16", p)
    d = c.dim
    k = _Call(dev)
    g = k.out((d["n"],), "float_to_int16 out", dtype=torch.int16, pitch=PITCH)
    scratch = torch.full((64,), -1, dtype=torch.int32, device=dev)
    k.call("sat_float_to_int16", k.up(c.t["x"]), g.t.data_ptr(), d["n"], d["maximize"], scratch.data_ptr())
    assert bool((scratch[1:] == -1).all()), "float_to_int16 wrote beyond the 4 bytes of its scratch"
    _finish(c, {"out": g.t})


@_cases("overlap_add")
def test_overlap_add(dev, p):
    c = su.Case("overlap_add", p)
    t, d = c.t, c.dim
    k = _Call(dev)
    g = k.out((d["batch"], d["c"], d["total"]), "overlap_add out", pitch=d["total"])
    k.call("sat_overlap_add", k.up(t["pieces"]), k.up(t["window"]), g.t.data_ptr(), d["batch"], d["chunks"], d["c"], d["l"], d["hop"], d["ov"],
           d["total"])
    g.assert_written()
    _finish(c, {"out": g.t})


@_cases("resample_sinc")
def test_resample_sinc(dev, p):
    c = su.Case("resample_sinc", p)
    t, d = c.t, c.dim
    k = _Call(dev)
    g = k.out((d["rows"], d["out_len"]), "resample_sinc y")
    k.call("sat_resample_sinc", k.up(t["x"]), k.up(t["bank"]), g.t.data_ptr(), d["rows"], d["in_len"], d["out_len"], d["orig"], d["new"], d["width"])
    g.assert_written()
    _finish(c, {"y": g.t})


def test_dpmpp3m_update_refuses_c2_without_d1(dev):
    """c2 multiplies (d1 - d2): without d1 the entry refuses and leaves x as it was (it used to drop the term)."""
    c = su.Case("dpmpp3m_update", dict(n=77, step="steady"))
    t, d = c.t, c.dim
    k = _Call(dev)
    g = k.out((77,), "dpmpp3m_update x", init=t["x"], pitch=PITCH)
    rc = k.lib.sat_dpmpp3m_update(g.t.data_ptr(), k.up(t["d"]), None, k.up(t["d2"]), k.up(t["noise"]), d["a"], d["b"], 0.0, d["c2"], d["cn"], 77,
                                  k.hip.stream())
    torch.cuda.synchronize()
    assert rc == -1 and b"d1" in k.lib.sat_last_error()
    assert_bit_equal("x after the refused call", g.t.cpu(), t["x"])


# ------------------------------------------------------------------------------------------------------------------ the wrappers
def test_python_wrappers_at_a_seam_each(dev):
    """The wrappers' own arithmetic -- argument order, output length, window and totals: _lin with out aliasing a term beyond the grid cap,
    resample at a second frame of one phase, float_to_int16_audio with the peak in the last sample, _run_chunked around a stub codec."""
    from stable_audio_tools.inference.resample import resample
    from stable_audio_tools.inference.sampling import _lin
    from stable_audio_tools.models.autoencoders import AudioAutoencoder
    from stable_audio_tools.utils.audio_utils import float_to_int16_audio
    c = su.Case("lincomb", dict(n=su.BIG, terms="01234", alias="t3"))
    dv = {k: v.to(dev) for k, v in c.t.items()}
    out = _lin(dv["t3"], [(c.dim["coef"][i], dv[f"t{i}"]) for i in range(5)])
    assert out.data_ptr() == dv["t3"].data_ptr()
    su.check(c, {"out": out.cpu()})
    c = su.Case("lincomb", dict(n=257, terms="03", alias="-"))            # two terms: the wrapper fills the other three with NULL
    out = _lin(torch.full((257,), float("nan"), device=dev), [(c.dim["coef"][0], c.t["t0"].to(dev)), (c.dim["coef"][3], c.t["t3"].to(dev))])
    su.check(c, {"out": out.cpu()})

    c = su.Case("resample_sinc", dict(orig_sr=48000, new_sr=44100, rows=5, in_len=161, short=0))
    y = resample(c.t["x"].view(1, 5, 161).to(dev), 48000, 44100)
    assert y.shape == (1, 5, 148)
    su.check(c, {"y": y.view(5, 148).cpu()})

    c = su.Case("float_to_int16", dict(n=4099, maximize=1, peak=2.5, where="last"))
    got = float_to_int16_audio(c.t["x"].view(1, 4099).to(dev), maximize=True)
    assert got.shape == (1, 4099) and got.device.type == "cpu"
    su.check(c, {"out": got.view(4099)})

    # decode_audio's call: 3 windows of 8 latent frames, hop 6, 4 samples per frame; the stub codec repeats every frame 4 times
    p = dict(batch=2, chunks=3, c=2, l=32, hop=24, ov=8, extra=0)
    c = su.Case("overlap_add", p)
    lat = torch.randn(2, 2, 20, generator=torch.Generator().manual_seed(5))
    fn = lambda z: z.repeat_interleave(4, dim=-1)
    got = AudioAutoencoder._run_chunked(None, lat.to(dev), fn, 8, 6, 3, 24, 8, 4, 77)
    assert got.shape == (2, 2, 77)
    c.t["pieces"] = torch.stack([fn(lat[..., i * 6:i * 6 + 8]) for i in range(3)], dim=1)
    want = su.reference(c)
    got_full = torch.cat((got.cpu(), want["out"][..., 77:].float()), dim=-1)            # (the wrapper crops to `keep`)
    su.check(c, {"out": got_full}, want)
