"""The harness of the DiT option-family parity suites (tests/test_gpu_dit_*.py): one ``Harness(FAMILY)`` per test file, with the family's
golden, its cached models, a forward run under the launch-path switches, and the checks every family repeats.  The numbers live here once:

* against the REFERENCE's own outputs in a 16-bit operand format: ``fmt.tol(2.5e-3)`` at CFG 1, ``fmt.tol(1.2e-2)`` at CFG 7 (``gate``);
* in the fp32 verification mode (gemm_dtype "fp32x"): FP32X_GATE, what separates an indexing error from rounding;
* the fused sampler step against VDenoiser(forward): ``T(2e-2)`` in the suite's format, 1e-5 in fp32x (``check_fused_denoise``);
* per-block operand formats [fp16, bf16, fp16]: the bf16 gate, the coarsest format in the plan (``check_per_block_formats``).
A plain module, imported by the test files as ``util`` is."""
import torch

import cases
import dit_family
from dit_family_host import model_config
from util import FORMATS, SUITE, assert_close, rel_l2

T = SUITE.tol
FP32X_GATE = 1e-4


class Harness:
    def __init__(self, family):
        self.family = family
        self._models = {}
        self._gold = None

    def gold(self):
        if self._gold is None:
            self._gold = cases.load(self.family.stem)
        return self._gold

    def model(self, cfg_name, dev, **more):
        """The product's module of a config with the family's synthetic weights, cached per (config, extra constructor kwargs)."""
        key = (cfg_name, tuple(sorted(more.items())))
        if key not in self._models:
            from stable_audio_tools.models import _init
            from stable_audio_tools.models.dit import DiffusionTransformer
            with _init.skip_init():
                m = DiffusionTransformer(**self.family.configs[cfg_name], **self.family.product_kwargs, **more)
            m.load_state_dict(self.family.weights(cfg_name, m.state_dict(), 0), strict=True)
            self._models[key] = m.to(dev).eval()
        return self._models[key]

    def inputs(self, name, dev):
        """(x, t, forward kwargs) of a case, on the device."""
        x, t, kw = dit_family.case_inputs(self.family, name)
        to = lambda v: v.to(dev) if torch.is_tensor(v) else v
        return to(x), to(t), {k: to(v) for k, v in kw.items()}

    def run(self, name, dev, dtype, ln_fold=True, cross_fusion=True, formats=None, **more):
        """The case's forward with the four switches set; they are back at the suite's defaults afterwards, whatever happened."""
        m = self.model(self.family.cases[name][0], dev, **more)
        try:
            m.set_gemm_dtype(dtype).set_layernorm_fusion(ln_fold).set_cross_attention_fusion(cross_fusion).set_block_gemm_dtypes(formats)
            x, t, kw = self.inputs(name, dev)
            out = m(x, t, **kw)
            torch.cuda.synchronize()
        finally:
            m.set_block_gemm_dtypes(None).set_gemm_dtype(SUITE.gemm_dtype).set_layernorm_fusion(True).set_cross_attention_fusion(True)
        return out

    def gate(self, name, fmt=SUITE):
        return fmt.tol(2.5e-3) if self.family.cases[name][3] == 1.0 else fmt.tol(1.2e-2)

    def r16(self, name, fmt=SUITE):
        """What 16-bit operands of the Linears / convs alone cost the REFERENCE on this case (computed on the CPU by the generator)."""
        return rel_l2(self.gold()[f"{name}__r16_{fmt.gemm_dtype}"], self.gold()[name])

    def check_vs_reference(self, dev, name, dtype, gate, label="", rounded=False, **run):
        """Runs the case (``run``: what ``self.run`` takes), prints its rel-L2 against the golden and gates it; returns the output.
        ``label`` names the launch path where it is not the default; ``rounded`` adds the reference's own rounded-operand figure."""
        got = self.run(name, dev, dtype, **run)
        how = " / ".join(run["formats"]) if run.get("formats") else dtype
        how += f", {label}" if label else ""
        e = rel_l2(got, self.gold()[name])
        note = f"; reference with rounded operands {self.r16(name):.2e}" if rounded else ""
        print(f"\n[{self.family.title} {name}, {how}] rel-L2 vs reference {e:.2e} (gate {gate:.1e}{note})")
        assert_close(f"{name} ({how}) vs reference", got, self.gold()[name], gate)
        return got

    def check_fused_denoise(self, dev, name, dtype):
        """prepare_generation + denoise (one sat_dit_denoise_cfg per step) == VDenoiser(forward) at a small and a large sigma: 1e-5 in
        fp32x; T(2e-2) in the suite's format (dtype "suite"), where the two round c_in * x at different points and CFG 7 amplifies the
        16-bit roundings that flip.  c_in scales the latent channels only: an xscale on concat channels shows here."""
        cfg_name, _, _, cfg_scale = self.family.cases[name]
        fmt = SUITE.gemm_dtype if dtype == "suite" else dtype
        gate = T(2e-2) if dtype == "suite" else 1e-5
        m = self.model(cfg_name, dev)
        try:
            m.set_gemm_dtype(fmt)
            x, _, kw = self.inputs(name, dev)
            c, g, cond = kw["cross_attn_cond"], kw["global_embed"], dict(prepend_cond=kw["prepend_cond"], input_concat_cond=kw["input_concat_cond"])
            for sigma in (0.7, 12.0):
                c_skip, c_out, c_in = 1.0 / (sigma ** 2 + 1), -sigma / (sigma ** 2 + 1) ** 0.5, 1.0 / (sigma ** 2 + 1) ** 0.5
                t = torch.full((x.shape[0],), float(torch.atan(torch.tensor(sigma, dtype=torch.float64)) / torch.pi * 2), device=dev)
                want = m(x * c_in, t, cross_attn_cond=c, global_embed=g, cfg_scale=cfg_scale, **cond) * c_out + x * c_skip
                m.prepare_generation(c, g, cfg_scale, **cond)
                got = m.denoise(x, sigma, cfg_scale=cfg_scale)
                torch.cuda.synchronize()
                e = rel_l2(got, want)
                print(f"\n[fused denoise {name}, {fmt}, sigma {sigma}] rel-L2 vs VDenoiser(forward) {e:.2e} (gate {gate:.1e})")
                assert torch.isfinite(got).all()
                assert e <= gate, f"{name} {fmt} sigma {sigma}: fused denoise vs VDenoiser(forward) rel-L2 {e:.3e} > {gate:.1e}"
        finally:
            m.set_gemm_dtype(SUITE.gemm_dtype)

    def check_per_block_formats(self, dev, name):
        """[fp16, bf16, fp16] at the bf16 gate of the case, and not one bit like fp16 in every block: block 1 did run in bf16."""
        got = self.check_vs_reference(dev, name, "fp16", self.gate(name, FORMATS[0]), formats=["fp16", "bf16", "fp16"])
        assert not torch.equal(got, self.run(name, dev, "fp16")), "the per-block formats changed no bit: block 1 did not run in bf16"


def reduced_model(**dit_kwargs):
    """(config, module) of the reduced SA-Open model with these keys in its diffusion config, built by create_model_from_config."""
    import stable_audio_tools as S
    from stable_audio_tools.models import _init
    cfg = model_config(**dit_kwargs)
    with _init.skip_init():
        return cfg, S.create_model_from_config(cfg)


def generate(model, cfg, dev, state_dict, steps, seed, t_len=16):
    """Loads the reference-layout state dict with strict=True and generates one prompt at CFG 7 through generate_diffusion_cond
    (dpmpp-3m-sde); asserts shape, finiteness and a non-zero result.  Returns (audio, the conditioning tensors it used)."""
    from stable_audio_tools import synthetic
    from stable_audio_tools.inference.generation import generate_diffusion_cond
    model.load_state_dict(state_dict, strict=True)
    model = model.to(dev).eval()
    ratio = cfg["model"]["pretransform"]["config"]["downsampling_ratio"]
    cond = model.conditioner([{"seconds_start": 0, "seconds_total": 12}])
    cond["prompt"] = (synthetic.synth_input("prompt", (1, 128, cfg["model"]["diffusion"]["config"]["cond_token_dim"]), 1).to(dev), torch.ones(1, 128, device=dev))
    cond = {k: cond[k] for k in ("prompt", "seconds_start", "seconds_total")}
    audio = generate_diffusion_cond(model, steps=steps, cfg_scale=7.0, conditioning_tensors=cond, sample_size=t_len * ratio, seed=seed,
                                    device=str(dev), sampler_type="dpmpp-3m-sde", sigma_min=0.3, sigma_max=500)
    torch.cuda.synchronize()
    assert audio.shape == (1, 2, t_len * ratio) and torch.isfinite(audio).all() and float(audio.abs().max()) > 0
    return audio, cond
