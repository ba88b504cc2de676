"""Input-concat and prepend conditioning of the DiT (reference models/dit.py:38,160-197), host side: model construction under the
reference's parameter names and shapes, the conditioning-tensor convention, and the C ABI's argument / call-order checks."""
import ctypes
import json
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import cases  # noqa: E402

CONCAT_DIM, PREPEND_DIM = 65, 48
CONFIGS = {      # the configs of tests/golden/make_golden_extra.py
    "concat": dict(cases.SMALL_DIT, input_concat_dim=CONCAT_DIM),
    "prepend": dict(cases.SMALL_DIT, prepend_cond_dim=PREPEND_DIM),
    "both": dict(cases.SMALL_DIT, input_concat_dim=CONCAT_DIM, prepend_cond_dim=PREPEND_DIM),
    "prepend_only": dict(cases.SMALL_DIT, cond_token_dim=0, prepend_cond_dim=PREPEND_DIM),
}


def inpaint_config():
    from stable_audio_tools import model_configs as MC
    cfg = MC.reduced(MC.stable_audio_open_1_0())
    cfg["model_type"] = "diffusion_cond_inpaint"
    d = cfg["model"]["diffusion"]
    d["input_concat_ids"] = ["inpaint_mask", "inpaint_masked_input"]
    d["config"]["input_concat_dim"] = 1 + cfg["model"]["io_channels"]
    return cfg


def _keys():
    return json.load(open(os.path.join(HERE, "golden", "extra_state_dict_keys.json")))


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_dit_state_dict_matches_reference(name):
    from stable_audio_tools.models import _init
    from stable_audio_tools.models.dit import DiffusionTransformer
    with _init.skip_init():
        m = DiffusionTransformer(**CONFIGS[name])
    got = {k: list(v.shape) for k, v in m.state_dict().items()}
    assert got == _keys()[name]


def test_inpaint_model_builds_with_reference_keys():
    import stable_audio_tools as S
    from stable_audio_tools.models import _init
    with _init.skip_init():
        model = S.create_model_from_config(inpaint_config())
    got = {k: list(v.shape) for k, v in model.state_dict().items()}
    assert got == _keys()["inpaint_model"]
    dit = model.model.model
    assert dit.input_concat_dim == 65
    assert tuple(dit.preprocess_conv.weight.shape) == (129, 129, 1)
    assert tuple(dit.postprocess_conv.weight.shape) == (64, 64, 1)
    assert model.input_concat_ids == ["inpaint_mask", "inpaint_masked_input"]


def test_prepend_config_builds_through_factory():
    import stable_audio_tools as S
    from stable_audio_tools.models import _init
    cfg = inpaint_config()
    cfg["model"]["diffusion"]["config"]["prepend_cond_dim"] = PREPEND_DIM
    with _init.skip_init():
        model = S.create_model_from_config(cfg)
    sd = model.state_dict()
    assert tuple(sd["model.model.to_prepend_embed.0.weight"].shape) == (256, PREPEND_DIM)
    assert tuple(sd["model.model.to_prepend_embed.2.weight"].shape) == (256, 256)


def test_adaln_with_prepend_cond_is_rejected():
    from stable_audio_tools.models.dit import DiffusionTransformer
    with pytest.raises(NotImplementedError, match="adaLN"):
        DiffusionTransformer(**CONFIGS["prepend"], global_cond_type="adaLN")
    DiffusionTransformer(**CONFIGS["concat"], global_cond_type="adaLN")      # input concat alone is fine with adaLN


def test_get_conditioning_inputs_reads_one_element_lists():
    import stable_audio_tools as S
    from stable_audio_tools.models import _init
    with _init.skip_init():
        model = S.create_model_from_config(inpaint_config())
    b, t_len = 2, 24
    mask = torch.ones(b, 1, t_len)
    masked = torch.randn(b, 64, t_len)
    cond = {"prompt": (torch.randn(b, 128, 768), torch.ones(b, 128)), "seconds_start": (torch.randn(b, 1, 768), torch.ones(b, 1)),
            "seconds_total": (torch.randn(b, 1, 768), torch.ones(b, 1)), "inpaint_mask": [mask], "inpaint_masked_input": [masked]}
    ci = model.get_conditioning_inputs(cond)
    assert torch.equal(ci["input_concat_cond"], torch.cat([mask, masked], dim=1))
    assert ci["prepend_cond"] is None
    neg = model.get_conditioning_inputs(cond, negative=True)
    assert torch.equal(neg["negative_input_concat_cond"], ci["input_concat_cond"])


def test_extra_conditioning_entry_points_validate_without_gpu():
    from stable_audio_tools import _hip
    lib = _hip.lib()
    plan = ctypes.c_void_p()
    cfg = _hip.SatDitCfg(64, 256, 2, 4, 128, 128, 96, 128)
    assert lib.sat_dit_plan_create(ctypes.byref(cfg), ctypes.byref(plan)) == 0
    try:
        assert lib.sat_dit_plan_set_extra_conditioning(None, 65, 0, 0) == -1
        assert lib.sat_dit_plan_set_extra_conditioning(plan, -1, 0, 0) == -1 and b"negative" in lib.sat_last_error()
        assert lib.sat_dit_plan_set_extra_conditioning(plan, 0, 48, -3) == -1
        assert lib.sat_dit_plan_set_extra_conditioning(plan, 0, 48, 0) == -1 and b"max_prepend_len" in lib.sat_last_error()
        assert lib.sat_dit_plan_set_extra_conditioning(plan, 0, 0, 8) == -1
        assert lib.sat_dit_plan_set_extra_conditioning(plan, 0, 47, 8) == -2          # prepend_cond_dim must be a multiple of 4
        assert lib.sat_dit_plan_set_extra_conditioning(plan, 65, 48, 70) == 0
        # per-generation data before finalize: call order
        assert lib.sat_dit_prepare_extra_conditioning(plan, None, 0, None, 0, 2, None) == -5
        assert b"not finalized" in lib.sat_last_error()
        need = ctypes.c_size_t()
        assert lib.sat_dit_workspace_bytes(plan, 2, 64, ctypes.byref(need)) == -5
    finally:
        lib.sat_dit_plan_destroy(plan)
    assert lib.sat_dit_prepare_extra_conditioning(None, None, 0, None, 0, 2, None) == -5
    # adaLN + prepend conditioning: the reference returns P + T frames there (models/dit.py:158,185-195,219)
    cfg = _hip.SatDitCfg(64, 256, 2, 4, 128, 128, 96, 128, 1)
    assert lib.sat_dit_plan_create(ctypes.byref(cfg), ctypes.byref(plan)) == 0
    try:
        assert lib.sat_dit_plan_set_extra_conditioning(plan, 0, 48, 8) == -2 and b"adaLN" in lib.sat_last_error()
        assert lib.sat_dit_plan_set_extra_conditioning(plan, 65, 0, 0) == 0
    finally:
        lib.sat_dit_plan_destroy(plan)
