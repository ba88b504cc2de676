"""Generates tests/golden/codec_options.npz and codec_options_state_dict_keys.json: the Oobleck shapes beside the Stable Audio VAE
(ELU instead of Snake, nearest-neighbour upsampling, final tanh, channel counts that are not multiples of 64), by running the
REFERENCE's OobleckEncoder / OobleckDecoder with the placeholder modules of _ref_import.py.

Runs only in the build container (the reference does not travel).  Usage:
    python tests/golden/make_golden_codec_options.py
Stored: reference OUTPUTS (fp32 .npz) and state-dict key / shape lists only; weights and inputs are regenerated from seeds by
``stable_audio_tools.synthetic`` (CONFIGS / helpers below, which the tests import: importing this module does not import the reference).
"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cases  # noqa: E402
from stable_audio_tools import synthetic  # noqa: E402

# name -> the reference's constructor options.  `latent` is the decoder's latent_dim; the encoder emits 2 * latent (mean | scale).
CONFIGS = {
    # the reference's own defaults apart from the width (autoencoders.py:120-127, :157-167)
    "ref_defaults": dict(channels=32, c_mults=[1, 2, 4, 8], strides=[2, 4, 8, 8], latent=32, use_snake=False,
                         use_nearest_upsample=False, final_tanh=True),
    "nearest_snake": dict(channels=64, c_mults=[1, 2, 4], strides=[2, 4, 4], latent=64, use_snake=True,
                          use_nearest_upsample=True, final_tanh=False),
    # stage widths 48, 96, 144 and a 20-channel latent: nothing is a multiple of 64
    "narrow_all": dict(channels=48, c_mults=[1, 2, 3], strides=[2, 4, 4], latent=20, use_snake=False,
                       use_nearest_upsample=True, final_tanh=True),
}
T_LEN = 11                 # frames of the batched decode / encode cases
DEC_SEED, ENC_SEED = 1, 22    # (decoder seed: one whose draws meet the two reference-only assertions of main() in both tanh configs)
# With the synthetic weights as drawn the audio peaks at 0.15-0.27, where tanh is the identity to 1 % -- below the bf16 gate, so a
# kernel without the tanh would pass.  The tanh configs scale the last convolution's weight_g by this factor (peaks 1.1 and 1.8).
TANH_GAIN = 8.0
MIN_TANH_EFFECT = 0.15     # rel-L2 between the reference with and without its final tanh, asserted below
MIN_ELU_NEGATIVE = 0.20    # share of negative values entering the decoder's last ELU, asserted below


def ratio(name):
    r = 1
    for s in CONFIGS[name]["strides"]:
        r *= s
    return r


def decoder_kwargs(name, final_tanh=None):
    c = CONFIGS[name]
    return dict(out_channels=2, channels=c["channels"], c_mults=list(c["c_mults"]), strides=list(c["strides"]), latent_dim=c["latent"],
                use_snake=c["use_snake"], use_nearest_upsample=c["use_nearest_upsample"],
                final_tanh=c["final_tanh"] if final_tanh is None else final_tanh)


def encoder_kwargs(name):
    c = CONFIGS[name]
    return dict(in_channels=2, channels=c["channels"], c_mults=list(c["c_mults"]), strides=list(c["strides"]), latent_dim=2 * c["latent"],
                use_snake=c["use_snake"])


def model_config(name):
    """The config as a user writes it for ``create_model_from_config`` ("autoencoder").  final_tanh is False in the JSON: the HIP
    package takes the tanh through ``set_final_tanh(True)`` after construction (README, "Oobleck configurations")."""
    c = CONFIGS[name]
    return {"model_type": "autoencoder", "sample_size": 64 * ratio(name), "sample_rate": 44100, "audio_channels": 2,
            "model": {"encoder": {"type": "oobleck", "config": encoder_kwargs(name)},
                      "decoder": {"type": "oobleck", "config": decoder_kwargs(name, final_tanh=False)},
                      "bottleneck": {"type": "vae"}, "latent_dim": c["latent"], "downsampling_ratio": ratio(name), "io_channels": 2}}


def synth_decoder_sd(name, template_sd):
    """Decoder weights of config `name` (keys relative to the OobleckDecoder)."""
    sd = synthetic.synth_state_dict(template_sd, DEC_SEED)
    if CONFIGS[name]["final_tanh"]:
        last = f"layers.{len(CONFIGS[name]['strides']) + 2}.weight_g"
        sd[last] = sd[last] * TANH_GAIN
    return sd


def synth_encoder_sd(name, template_sd):
    return synthetic.synth_state_dict(template_sd, ENC_SEED)


def inputs(name):
    """(z [2, latent, T_LEN], z1 [2, latent, 1], audio [2, 2, T_LEN * ratio])"""
    c = CONFIGS[name]
    z = synthetic.synth_input("z_" + name, (2, c["latent"], T_LEN), 23)
    z1 = synthetic.synth_input("z1_" + name, (2, c["latent"], 1), 24)
    a = synthetic.synth_input("a_" + name, (2, 2, T_LEN * ratio(name)), 25, 0.3)
    return z, z1, a


@torch.no_grad()
def main():
    import _ref_import as R
    R.import_reference()
    rae = R.ref("models.autoencoders")
    rel = lambda a, b: ((a - b).norm() / b.norm()).item()
    out, keys = {}, {}
    for name, c in CONFIGS.items():
        dec = rae.OobleckDecoder(**decoder_kwargs(name)).eval()
        dec.load_state_dict(synth_decoder_sd(name, dec.state_dict()))
        enc = rae.OobleckEncoder(**encoder_kwargs(name)).eval()
        enc.load_state_dict(synth_encoder_sd(name, enc.state_dict()))
        z, z1, a = inputs(name)
        seen = {}
        if not c["use_snake"]:      # the last ELU is layers[-3]
            hook = dec.layers[-3].register_forward_hook(lambda m, i, o: seen.update(neg=(i[0] < 0).float().mean().item()))
        out[name + "/decode"] = dec(z)
        if not c["use_snake"]:
            hook.remove()
            assert seen["neg"] >= MIN_ELU_NEGATIVE, (name, seen)
            print(f"{name}: {100 * seen['neg']:.0f} % of the values entering the last ELU are negative")
        out[name + "/decode_T1"] = dec(z1)
        out[name + "/encode"] = enc(a)
        if c["final_tanh"]:
            pre = dec.layers[:-1](z)
            effect = rel(out[name + "/decode"], pre)
            print(f"{name}: final tanh changes the output by {effect:.3f} rel-L2 (pre-tanh peak {pre.abs().max().item():.2f})")
            assert effect >= MIN_TANH_EFFECT, (name, effect)
        keys[name] = {**{"encoder." + k: list(v.shape) for k, v in enc.state_dict().items()},
                      **{"decoder." + k: list(v.shape) for k, v in dec.state_dict().items()}}
        for k in ("decode", "decode_T1", "encode"):
            print(f"{name}/{k}: {tuple(out[name + '/' + k].shape)}")
    paths = cases.save("codec_options", {k: v.detach().cpu().numpy() for k, v in out.items()})
    print("wrote", paths, [os.path.getsize(p) for p in paths])
    kp = os.path.join(cases.GOLDEN_DIR, "codec_options_state_dict_keys.json")
    with open(kp, "w") as f:
        json.dump(keys, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote", kp, os.path.getsize(kp))


if __name__ == "__main__":
    main()
