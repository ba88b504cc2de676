"""Generates the goldens of the local-attention codec family (local_attn_cases.py): tests/golden/local_attn_small*.npz and
local_attn_state_dict_keys.json, by running the REFERENCE's TransformerEncoder1D / TransformerDecoder1D (models/local_attention.py, imported
through the aliased package of _ref_import.py, which stays as it is) and, for case D, its create_autoencoder_from_config, on the CPU.

NATTEN is not installed where this runs: tests/golden/natten_standin.py is set as the ``natten`` attribute of the reference's transformer
module, exactly as make_golden_dit_natten.py does.  No reference text changes.

Per entry, beside the fp32 output: ``__r16_fp16`` / ``__r16_bf16``, the output with the input and the weight of every nn.Linear rounded to that
format (forward pre-hooks), and ``__f64``, the output of the same modules in float64.  The reference's NATTEN branch and its rotary embedding
name torch.float32 outright (transformer.py:140, 444-446, 484, 491); for the float64 run alone the ``torch`` name of that module is a proxy
whose float32 is float64, so that the yardstick of the fp32 gate is float64 throughout.

Asserted: every encoder / decoder output moves by at least 5 % when to_out and ff.2 are zeroed as the reference initialises them; every
(entry, format) figure is finite; the pairs at or above local_attn_cases.R16_LIMIT are at most one of A-C in bf16 and none in fp16; the
yardstick itself passes the per-row gate.  The figures are printed as the literals of local_attn_cases.R16 / F64 / DROPPED.

Runs only in the build container (the reference does not travel).  Usage:
    python tests/golden/make_golden_local_attn.py
"""
import contextlib
import copy
import importlib
import json
import os
import sys
from unittest import mock

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import _ref_import  # noqa: E402
import cases  # noqa: E402
import local_attn_cases as LC  # noqa: E402
import natten_standin  # noqa: E402
import util  # noqa: E402

_ref_import.import_reference()
rla = importlib.import_module("ref_stable_audio_tools.models.local_attention")
rae = _ref_import.ref("models.autoencoders")
rtf = _ref_import.ref("models.transformer")

ROUND = {"fp16": util.fp16_round, "bf16": util.bf16_round}


def rounded(model, fmt):
    """A copy of the model whose nn.Linear see their input and their weight rounded to fmt (the bias stays fp32)."""
    rnd = ROUND[fmt]
    m = copy.deepcopy(model)
    for mod in m.modules():
        if isinstance(mod, torch.nn.Linear):
            mod.weight.data = rnd(mod.weight.data)
            mod.register_forward_pre_hook(lambda _, args: (rnd(args[0]),) + tuple(args[1:]))
    return m


class _TorchF64:
    """``torch`` with float32 = float64, for the module namespace of the reference's transformer.py during the float64 run"""
    float32 = torch.float64

    def __getattr__(self, name):
        return getattr(torch, name)


@contextlib.contextmanager
def float64_attention():
    default = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)          # (the chunked paths accumulate into torch.zeros / window with torch.bartlett_window)
    try:
        with mock.patch.object(rtf, "torch", _TorchF64()):
            yield
    finally:
        torch.set_default_dtype(default)


def load(model, sd_fn=None):
    sd = LC.weights(model.state_dict())
    model.load_state_dict(sd_fn(sd) if sd_fn else sd, strict=True)
    return model.eval()


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def variants(out, entry, run, model):
    """out[entry] and its yardsticks; run(model, double) evaluates the entry on a model"""
    out[entry] = run(model, False)
    for fmt in ROUND:
        out[f"{entry}__r16_{fmt}"] = run(rounded(model, fmt), False)
    with float64_attention():
        out[f"{entry}__f64"] = run(copy.deepcopy(model).double(), True)
    assert out[f"{entry}__f64"].dtype == torch.float64
    return out[entry]


@torch.no_grad()
def gen_codecs(out, keys):
    for name, (enc_kw, dec_kw, _, _, _) in LC.CODECS.items():
        enc, dec = load(rla.TransformerEncoder1D(**enc_kw)), load(rla.TransformerDecoder1D(**dec_kw))
        keys[f"{name}_enc"] = {k: list(v.shape) for k, v in enc.state_dict().items()}
        keys[f"{name}_dec"] = {k: list(v.shape) for k, v in dec.state_dict().items()}
        x = LC.audio(name)
        z = variants(out, f"{name}_enc", lambda m, dbl: m(x.double() if dbl else x), enc)
        y = variants(out, f"{name}_dec", lambda m, dbl: m(z.double() if dbl else z), dec)
        for entry, model, cls, kw, inp, got in ((f"{name}_enc", enc, rla.TransformerEncoder1D, enc_kw, x, z),
                                                (f"{name}_dec", dec, rla.TransformerDecoder1D, dec_kw, z, y)):
            identity = load(cls(**kw), LC.zeroed_branches)(inp)
            effect = rel(got, identity)
            print(f"{entry}: {tuple(got.shape)} std {float(got.std()):.3f}, rel-L2 vs the model with to_out / ff.2 zeroed {effect:.2e}")
            assert effect >= 0.05, f"{entry}: the two branches move the output by {effect:.2e} only"


@torch.no_grad()
def gen_autoencoder(out, keys):
    model = load(rae.create_autoencoder_from_config(copy.deepcopy(LC.D_CONFIG)))
    keys["D"] = {k: list(v.shape) for k, v in model.state_dict().items()}
    x = LC.d_audio()
    # the vae bottleneck draws with torch.randn_like (bottleneck.py:50): the injected Gaussian of the call's shape in its place
    noise = lambda like: LC.d_noise(like.shape).to(like.dtype)

    def run(fn_name, inp, **kw):
        def go(m, dbl):
            with mock.patch.object(torch, "randn_like", noise):
                return getattr(m, fn_name)(inp.double() if dbl else inp, **kw)
        return go
    z = variants(out, "D_encode", run("encode_audio", x), model)
    variants(out, "D_decode", run("decode_audio", z), model)
    variants(out, "D_encode_chunked", run("encode_audio", x, chunked=True, **LC.D_CHUNK), model)
    variants(out, "D_decode_chunked", run("decode_audio", z, chunked=True, **LC.D_CHUNK), model)
    print(f"D: chunked encode differs from plain by {rel(out['D_encode_chunked'], out['D_encode']):.2e}, chunked decode by "
          f"{rel(out['D_decode_chunked'], out['D_decode']):.2e}")


def figures(out):
    r16, f64, dropped = {}, {}, []
    for entry, fmts in LC.entries().items():
        want = out[entry]
        r16[entry] = {fmt: rel(out[f"{entry}__r16_{fmt}"], want) for fmt in ROUND}
        f64[entry] = rel(want, out[f"{entry}__f64"])
        assert all(torch.isfinite(torch.tensor(v)) for v in r16[entry].values()), (entry, r16[entry])
        for fmt in ROUND:
            if fmt in fmts and not r16[entry][fmt] < LC.R16_LIMIT:
                dropped.append((entry, fmt))
        # the yardstick itself under the per-row gate (rows: one time step of one item)
        for fmt in ROUND:
            rows = util.slice_errors(out[f"{entry}__r16_{fmt}"], want, (0, 2)).max().item()
            assert rows <= LC.ROW_FACTOR * 2.0 * r16[entry][fmt], (entry, fmt, rows, r16[entry][fmt])
            print(f"{entry} {fmt}: rounded operands {r16[entry][fmt]:.3e} (gate {2 * r16[entry][fmt]:.3e}), worst row {rows:.3e} "
                  f"(row gate {LC.ROW_FACTOR * 2 * r16[entry][fmt]:.3e})")
        rows = util.slice_errors(want, out[f"{entry}__f64"], (0, 2)).max().item()
        assert rows <= LC.ROW_FACTOR * 4.0 * f64[entry], (entry, rows, f64[entry])
        print(f"{entry} fp32: vs float64 {f64[entry]:.3e} (gate {4 * f64[entry]:.3e}), worst row {rows:.3e}")
    assert not [d for d in dropped if d[1] == "fp16"], f"fp16 pairs at or above {LC.R16_LIMIT}: {dropped}"
    assert len({e.split('_')[0] for e, f in dropped if f == "bf16" and e[0] in "ABC"}) <= 1 and not [d for d in dropped if d[0][0] == "D"], dropped
    return r16, f64, dropped


if __name__ == "__main__":
    torch.set_num_threads(min(16, os.cpu_count()))
    assert rtf.natten is None, "the reference's transformer module no longer keeps the (missing) library as `natten`"
    rtf.natten = natten_standin
    out, keys = {}, {}
    gen_codecs(out, keys)
    gen_autoencoder(out, keys)
    r16, f64, dropped = figures(out)
    json.dump(keys, open(LC.KEYS_PATH, "w"), sort_keys=True)
    paths = cases.save(LC.STEM, {k: v.detach().cpu().numpy() for k, v in out.items()})
    print("wrote", LC.KEYS_PATH, {k: len(v) for k, v in keys.items()})
    print("wrote", ", ".join(f"{p} ({os.path.getsize(p) // 1024} KiB)" for p in paths))
    fmt = lambda d: "{" + ", ".join(f'"{k}": {v:.3e}' for k, v in d.items()) + "}"
    print("R16 = {\n" + "\n".join(f'    "{e}": {fmt(v)},' for e, v in r16.items()) + "\n}")
    print("F64 = " + fmt(f64))
    print("DROPPED =", dropped)
