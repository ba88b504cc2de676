"""Generates tests/golden/codec_antialias.npz and codec_antialias_state_dict_keys.json: Oobleck codecs with ``antialias_activation=True``,
by running the REFERENCE's OobleckEncoder / OobleckDecoder (pattern and helpers of make_golden_codec_options.py).

``alias_free_torch`` is not installed where this runs.  The reference's ``models.autoencoders`` holds the library's ``Activation1d`` as a
module attribute (the import-only placeholder of _ref_import.py sets it to ``object``); tests/golden/alias_free_standin.py -- this project's
own statement of the operation, held against a float64 brute-force form and an independent implementation by
tests/test_codec_antialias_host.py -- is set in its place after ``import_reference()``.  No reference text changes.  The goldens are therefore
pinned by the stand-in, not by the library.

What the reference builds: ``antialias_activation`` reaches the activation in front of every DecoderBlock's upsampler and the activation in
front of the last convolution of either direction.  Its blocks construct their ResidualUnits -- and OobleckEncoder its EncoderBlocks --
without the option (autoencoders.py:76-78, :110-112, :139-143), so those activations stay plain; the key lists written here show it.

Runs only in the build container (the reference does not travel).  Usage:
    python tests/golden/make_golden_codec_antialias.py
Stored: reference OUTPUTS (fp32 .npz) and state-dict key / shape lists only; weights and inputs are regenerated from seeds by
``stable_audio_tools.synthetic`` (CONFIGS / helpers below, which the tests import: importing this module does not import the reference).
Asserted here: every output differs from the same weights with the option off by at least MIN_EFFECT rel-L2, which is what makes "ran the
plain activation instead" fail the gates of tests/test_gpu_codec_antialias.py."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cases  # noqa: E402
from stable_audio_tools import synthetic  # noqa: E402

CONFIGS = {
    # Snake, transposed-convolution upsampling, widths 64 / 128 / 256
    "snake_convt": dict(channels=64, c_mults=[1, 2, 4], strides=[2, 4, 4], latent=64, use_snake=True, use_nearest_upsample=False),
    # ELU, nearest upsampling, widths 48 / 96 / 144 and a 20-channel latent: every tensor has pad channels
    "elu_narrow": dict(channels=48, c_mults=[1, 2, 3], strides=[2, 4, 4], latent=20, use_snake=False, use_nearest_upsample=True),
    # width 128 / 256: the ResidualUnits are the ones the 16-bit builds run as one fused launch
    "snake_128": dict(channels=128, c_mults=[1, 2], strides=[2, 4], latent=64, use_snake=True, use_nearest_upsample=False),
}
T_LEN = 11
DEC_SEED, ENC_SEED = 31, 32
# SnakeBeta's log-scale parameters as synthetic draws them (0.2 randn) give e^alpha ~ 1 and 1 / e^beta ~ 1.  The wrapped Snakes get
# e^alpha ~ 2.7 and 1 / e^beta ~ 1.6 on top: the sin^2 term then bends the doubled-rate signal visibly
AA_ALPHA_SHIFT, AA_BETA_SHIFT = 1.0, -0.5
MIN_EFFECT = 5e-2          # rel-L2 between the reference with the option on and off, same weights, every stored output


def ratio(name):
    r = 1
    for s in CONFIGS[name]["strides"]:
        r *= s
    return r


def decoder_kwargs(name, antialias=True):
    c = CONFIGS[name]
    return dict(out_channels=2, channels=c["channels"], c_mults=list(c["c_mults"]), strides=list(c["strides"]), latent_dim=c["latent"],
                use_snake=c["use_snake"], use_nearest_upsample=c["use_nearest_upsample"], final_tanh=False, antialias_activation=antialias)


def encoder_kwargs(name, antialias=True):
    c = CONFIGS[name]
    return dict(in_channels=2, channels=c["channels"], c_mults=list(c["c_mults"]), strides=list(c["strides"]), latent_dim=2 * c["latent"],
                use_snake=c["use_snake"], antialias_activation=antialias)


def model_config(name, allow=True):
    """The config as a user writes it for ``create_model_from_config`` ("autoencoder"): the reference's keys plus this package's opt-in."""
    c = CONFIGS[name]
    opt_in = {"allow_antialias": True} if allow else {}
    return {"model_type": "autoencoder", "sample_size": 64 * ratio(name), "sample_rate": 44100, "audio_channels": 2,
            "model": {"encoder": {"type": "oobleck", "config": dict(encoder_kwargs(name), **opt_in)},
                      "decoder": {"type": "oobleck", "config": dict(decoder_kwargs(name), **opt_in)},
                      "bottleneck": {"type": "vae"}, "latent_dim": c["latent"], "downsampling_ratio": ratio(name), "io_channels": 2}}


def _synth(template_sd, seed):
    sd = synthetic.synth_state_dict(template_sd, seed)
    for k in sd:
        if k.endswith(".filter"):              # Activation1d's buffers are the filter, not weights to draw
            sd[k] = template_sd[k].detach().clone().float()
        elif k.endswith(".act.alpha"):
            sd[k] = sd[k] + AA_ALPHA_SHIFT
        elif k.endswith(".act.beta"):
            sd[k] = sd[k] + AA_BETA_SHIFT
    return sd


def synth_decoder_sd(name, template_sd):
    """Decoder weights of config `name` (keys relative to the OobleckDecoder, built with the option on)."""
    return _synth(template_sd, DEC_SEED)


def synth_encoder_sd(name, template_sd):
    return _synth(template_sd, ENC_SEED)


def plain_sd(sd):
    """The same weights for the module built with the option off: ``<path>.act.alpha`` -> ``<path>.alpha``, no filter buffers."""
    return {k.replace(".act.", "."): v for k, v in sd.items() if not k.endswith(".filter")}


def inputs(name):
    """(z [2, latent, T_LEN], z1 [2, latent, 1], audio [2, 2, T_LEN * ratio])"""
    c = CONFIGS[name]
    z = synthetic.synth_input("aa_z_" + name, (2, c["latent"], T_LEN), 33)
    z1 = synthetic.synth_input("aa_z1_" + name, (2, c["latent"], 1), 34)
    a = synthetic.synth_input("aa_a_" + name, (2, 2, T_LEN * ratio(name)), 35, 0.3)
    return z, z1, a


@torch.no_grad()
def main():
    import _ref_import as R
    import alias_free_standin
    R.import_reference()
    rae = R.ref("models.autoencoders")
    assert rae.Activation1d is object, "the reference's autoencoders module no longer holds the (placeholder) library class as `Activation1d`"
    rae.Activation1d = alias_free_standin.Activation1d
    rel = lambda a, b: ((a - b).norm() / b.norm()).item()
    out, keys = {}, {}
    for name in CONFIGS:
        dec = rae.OobleckDecoder(**decoder_kwargs(name)).eval()
        dsd = synth_decoder_sd(name, dec.state_dict())
        dec.load_state_dict(dsd)
        enc = rae.OobleckEncoder(**encoder_kwargs(name)).eval()
        esd = synth_encoder_sd(name, enc.state_dict())
        enc.load_state_dict(esd)
        dec0 = rae.OobleckDecoder(**decoder_kwargs(name, antialias=False)).eval()
        dec0.load_state_dict(plain_sd(dsd))
        enc0 = rae.OobleckEncoder(**encoder_kwargs(name, antialias=False)).eval()
        enc0.load_state_dict(plain_sd(esd))
        z, z1, a = inputs(name)
        for k, on, off, x in (("decode", dec, dec0, z), ("decode_T1", dec, dec0, z1), ("encode", enc, enc0, a)):
            y = on(x)
            effect = rel(off(x), y)
            n_aa = sum(isinstance(m, alias_free_standin.Activation1d) for m in on.modules())
            print(f"{name}/{k}: {tuple(y.shape)}, {n_aa} anti-aliased activations, option off differs by {effect:.3f} rel-L2")
            assert effect >= MIN_EFFECT, (name, k, effect)
            out[f"{name}/{k}"] = y
        keys[name] = {**{"encoder." + k: list(v.shape) for k, v in enc.state_dict().items()},
                      **{"decoder." + k: list(v.shape) for k, v in dec.state_dict().items()}}
    paths = cases.save("codec_antialias", {k: v.detach().cpu().numpy() for k, v in out.items()})
    print("wrote", paths, [os.path.getsize(p) for p in paths])
    kp = os.path.join(cases.GOLDEN_DIR, "codec_antialias_state_dict_keys.json")
    with open(kp, "w") as f:
        json.dump(keys, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote", kp, os.path.getsize(kp))


if __name__ == "__main__":
    main()
