"""Generates tests/golden/dit_extra_small.npz, generate_inpaint.npz and extra_state_dict_keys.json: input-concat and prepend
conditioning (reference models/dit.py:160-197) on the reduced DiT, and a short generate_diffusion_cond of a reduced
"diffusion_cond_inpaint" model, by running the REFERENCE with the placeholder modules of _ref_import.py.

Runs only in the build container (the reference does not travel).  Usage:
    python tests/golden/make_golden_extra.py
Stored: reference OUTPUTS and recorded Gaussian draws only (fp32 .npz); weights and inputs are regenerated from seeds by
``stable_audio_tools.synthetic`` (EXTRA below).
"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as MG  # noqa: E402  (imports the reference through _ref_import.py)
import cases  # noqa: E402
from stable_audio_tools import synthetic  # noqa: E402

R = MG.R
rdit = MG.rdit

CONCAT_DIM, PREPEND_DIM = 65, 48
# reduced-DiT configs of the fixtures: name -> DiffusionTransformer kwargs
CONFIGS = {
    "concat": dict(cases.SMALL_DIT, input_concat_dim=CONCAT_DIM),
    "prepend": dict(cases.SMALL_DIT, prepend_cond_dim=PREPEND_DIM),
    "both": dict(cases.SMALL_DIT, input_concat_dim=CONCAT_DIM, prepend_cond_dim=PREPEND_DIM),
    "prepend_only": dict(cases.SMALL_DIT, cond_token_dim=0, prepend_cond_dim=PREPEND_DIM),
}
# forward cases: name -> (config, t_len, concat length Tc or None, prepend length P or None, cfg_scale, scale_phi, partly-zero prepend mask)
CASES = {
    "concat_cfg1_T64": ("concat", 64, 64, None, 1.0, 0.0, False),
    "concat_cfg1_T77": ("concat", 77, 77, None, 1.0, 0.0, False),
    "concat_cfg7_T77": ("concat", 77, 77, None, 7.0, 0.0, False),
    "concat_resize_cfg1_T77": ("concat", 77, 50, None, 1.0, 0.0, False),
    "prepend_P3_cfg1_T64": ("prepend", 64, None, 3, 1.0, 0.0, False),
    "prepend_P3_cfg7_T64": ("prepend", 64, None, 3, 7.0, 0.0, False),
    "prepend_P70_cfg1_T64": ("prepend", 64, None, 70, 1.0, 0.0, False),
    "prepend_P3_masked_cfg7_T64": ("prepend", 64, None, 3, 7.0, 0.0, True),
    "both_cfg7_phi04_T77": ("both", 77, 77, 5, 7.0, 0.4, False),
    "prepend_only_cfg7_T64": ("prepend_only", 64, None, 4, 7.0, 0.0, False),
    # prepend models called without prepend tokens (no CFG batch on the prepend-only model: dit.py:270)
    "prepend_none_cfg1_T64": ("prepend", 64, None, None, 1.0, 0.0, False),
    "prepend_only_none_cfg7_T64": ("prepend_only", 64, None, None, 7.0, 0.0, False),
}
# generate_diffusion_cond of the reduced inpaint model
GEN = dict(t_len=24, steps=8, cfg_scale=7.0, seed=11, sampler_type="dpmpp-3m-sde", sigma_min=0.3, sigma_max=500)


def case_inputs(name):
    """(x, t, cross_attn_cond or None, global_embed, input_concat_cond or None, prepend_cond or None, prepend_cond_mask or None)"""
    cfg_name, t_len, tc, p, _, _, masked = CASES[name]
    cfg = CONFIGS[cfg_name]
    x, t, c, g = cases.dit_inputs(2, t_len, 128, 96, 1)
    if cfg["cond_token_dim"] == 0:
        c = None
    cc = synthetic.synth_input("concat", (2, CONCAT_DIM, tc), 200 + tc) if tc else None
    pc = synthetic.synth_input("prepend", (2, p, PREPEND_DIM), 300 + p) if p else None
    pm = None
    if pc is not None:
        pm = torch.ones(2, p)
        if masked:
            pm[1, 1:] = 0
    return x, t, c, g, cc, pc, pm


def inpaint_config():
    """The reduced SA-Open model as a "diffusion_cond_inpaint" model: the DiT also sees cat([inpaint_mask, inpaint_masked_input])
    (reference training/diffusion.py:680-756)."""
    from stable_audio_tools import model_configs as MC
    cfg = MC.reduced(MC.stable_audio_open_1_0())
    cfg["model_type"] = "diffusion_cond_inpaint"
    d = cfg["model"]["diffusion"]
    d["input_concat_ids"] = ["inpaint_mask", "inpaint_masked_input"]
    d["config"]["input_concat_dim"] = 1 + cfg["model"]["io_channels"]
    return cfg


def inpaint_conditioning(model, b, t_len, dev="cpu"):
    """Conditioning tensors of the inpaint generation; the input-concat entries are one-element lists, as the reference's training
    wrapper builds them (training/diffusion.py:754)."""
    dc = inpaint_config()["model"]["diffusion"]["config"]
    cond = model.conditioner([{"seconds_start": 0, "seconds_total": 10 + i} for i in range(b)])
    cond["prompt"] = [synthetic.synth_input("prompt", (b, 128, dc["cond_token_dim"]), 41).to(dev), torch.ones(b, 128, device=dev)]
    cond = {k: cond[k] for k in ("prompt", "seconds_start", "seconds_total")}
    mask = torch.ones(b, 1, t_len)
    mask[0, :, 6:15] = 0
    mask[1, :, 12:] = 0
    masked = synthetic.synth_input("inpaint_latents", (b, 64, t_len), 42) * mask
    cond["inpaint_mask"] = [mask.to(dev)]
    cond["inpaint_masked_input"] = [masked.to(dev)]
    return cond


@torch.no_grad()
def gen_extra():
    out = {}
    models = {}
    for name, (cfg_name, *_rest) in CASES.items():
        if cfg_name not in models:
            models[cfg_name] = MG.load_synth(rdit.DiffusionTransformer(**CONFIGS[cfg_name]), 0)
        m = models[cfg_name]
        _, _, _, _, cfg_scale, phi, _ = CASES[name]
        x, t, c, g, cc, pc, pm = case_inputs(name)
        out[name] = m(x, t, cross_attn_cond=c, global_embed=g, input_concat_cond=cc, prepend_cond=pc, prepend_cond_mask=pm,
                      cfg_scale=cfg_scale, scale_phi=phi)
        print(name, tuple(out[name].shape), float(out[name].std()))
    MG.save("dit_extra_small", **out)


@torch.no_grad()
def gen_generate_inpaint():
    holder = {}
    MG._install_kdiffusion_standin(lambda: holder["rec"])
    cfg = inpaint_config()
    model = R.ref("models.factory").create_model_from_config(cfg)
    model.load_state_dict(synthetic.synth_state_dict(model.state_dict(), 0))
    model.eval()
    ratio = cfg["model"]["pretransform"]["config"]["downsampling_ratio"]
    b, t_len = 2, GEN["t_len"]
    cond = inpaint_conditioning(model, b, t_len)
    kw = {k: v for k, v in GEN.items() if k != "t_len"}
    with MG._DrawRecorder() as rec:
        holder["rec"] = rec
        y = MG.rgen.generate_diffusion_cond(model, conditioning_tensors=cond, sample_size=t_len * ratio, device="cpu", return_latents=True, **kw)
    assert len(rec.randn) == 1 and not rec.randn_like
    out = {"latents": y, "noise": rec.randn[0]}
    for i, t in enumerate(rec.step):
        out[f"step{i}"] = t
    print("inpaint generate: steps drawn", len(rec.step), tuple(y.shape), float(y.std()))
    MG.save("generate_inpaint", **out)


def gen_keys():
    keys = {name: {k: list(v.shape) for k, v in rdit.DiffusionTransformer(**c).state_dict().items()} for name, c in CONFIGS.items()}
    m = R.ref("models.factory").create_model_from_config(inpaint_config())
    keys["inpaint_model"] = {k: list(v.shape) for k, v in m.state_dict().items()}
    path = os.path.join(cases.GOLDEN_DIR, "extra_state_dict_keys.json")
    json.dump(keys, open(path, "w"), sort_keys=True)
    print("wrote", path, {k: len(v) for k, v in keys.items()})


if __name__ == "__main__":
    torch.set_num_threads(min(16, os.cpu_count()))
    gen_keys()
    gen_extra()
    gen_generate_inpaint()
