"""What the host tests of the DiT option families (tests/test_dit_*_host.py) share: building a module without initialising it, the reduced
SA-Open config with a family's keys in its diffusion config, and the state-dict-keys check against the reference's recorded shapes."""
import copy
import json


def build(**kwargs):
    from stable_audio_tools.models import _init
    from stable_audio_tools.models.dit import DiffusionTransformer
    with _init.skip_init():
        return DiffusionTransformer(**kwargs)


def model_config(**dit_kwargs):
    from stable_audio_tools import model_configs as MC
    cfg = copy.deepcopy(MC.reduced(MC.stable_audio_open_1_0()))
    cfg["model"]["diffusion"]["config"].update(dit_kwargs)
    return cfg


def check_state_dict_keys(family, name):
    """The product's module of config `name` has the reference's state-dict keys and shapes (Family.keys_file) and loads the family's
    synthetic weights with strict=True; returns (module, {key: shape}) for the family's own assertions."""
    want = json.load(open(family.keys_path()))[name]
    m = build(**family.configs[name], **family.product_kwargs)
    got = {k: list(v.shape) for k, v in m.state_dict().items()}
    assert got == want
    m.load_state_dict(family.weights(name, m.state_dict(), 0), strict=True)
    return m, got
