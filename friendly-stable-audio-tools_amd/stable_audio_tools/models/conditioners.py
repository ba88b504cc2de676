"""The conditioner front-end of a conditioned diffusion model, as far as this build computes it itself.

Counterparts of ``Conditioner`` / ``NumberConditioner`` / ``MultiConditioner`` / ``create_multi_conditioner_from_conditioning_config``
(reference ``models/conditioners.py:18-102, 506-599``) and of the ``NumberEmbedder`` they embed numbers with
(``models/adp.py:680-701, 1495-1514``): same module tree and parameter names, so reference checkpoints load.

``NumberConditioner`` runs on the HIP C ABI (``sat_number_embed``: clamp, normalise, Fourier features and the Linear in one
launch per call); like the rest of the package it has no CPU path.  ``T5Conditioner`` (conditioners.py:261-346) runs the T5 encoder
stack on the C ABI as well (``sat_t5_*``, csrc/t5_encoder.hip); its weights and tokenizer are not part of a stable-audio checkpoint
-- the reference downloads them -- so it is registered only when they are in the local Hugging Face cache (or handed over with
``load_encoder``).  ``CLAPTextConditioner`` (conditioners.py:105-193) with ``use_text_features=True`` is a RoBERTa encoder and runs
on the C ABI too (``sat_roberta_*``, csrc/roberta_encoder.hip); it is registered when the file at ``clap_ckpt_path`` exists.  The other
encoder-backed types (the pooled CLAP embedding, CLAP audio, phonemes, ...) and a text encoder without weights are recorded in
``MultiConditioner.external_ids``: the caller supplies those entries through ``conditioning_tensors=`` -- the "random T5 embeds"
configuration of BASELINE.json.
"""
import ctypes
import os
import re
import typing as tp

import torch
from torch import nn

from .. import _hip

# conditioner types whose tensors must come from outside (encoders this build does not ship; "clap_text" without its checkpoint file)
_EXTERNAL_TYPES = ("clap_text", "clap_audio", "phoneme", "lut", "pretransform", "int")


class Conditioner(nn.Module):
    def __init__(self, dim: int, output_dim: int, project_out: bool = False):
        super().__init__()
        self.dim, self.output_dim = dim, output_dim
        self.proj_out = nn.Linear(dim, output_dim) if (project_out or dim != output_dim) else nn.Identity()

    def set_device(self, device: tp.Any) -> None:
        raise NotImplementedError()


class LearnedPositionalEmbedding(nn.Module):
    """Parameter holder of adp.py:680-694 (``weights`` [dim / 2]); evaluated inside ``sat_number_embed``."""

    def __init__(self, dim: int):
        super().__init__()
        if dim % 2:
            raise ValueError("LearnedPositionalEmbedding needs an even dim")
        self.weights = nn.Parameter(torch.randn(dim // 2))


class NumberEmbedder(nn.Module):
    """Parameter holder of adp.py:1495-1514: ``embedding.0`` = LearnedPositionalEmbedding(dim), ``embedding.1`` = Linear(dim + 1, features)."""

    def __init__(self, features: int, dim: int = 256):
        super().__init__()
        self.features = features
        self.embedding = nn.Sequential(LearnedPositionalEmbedding(dim), nn.Linear(dim + 1, features))

    def forward(self, values: torch.Tensor, min_val: float = 0.0, max_val: float = 1.0) -> torch.Tensor:
        """values [B] (raw numbers, clamped to [min_val, max_val] and normalised by the kernel) -> [B, features]."""
        pos, lin = self.embedding[0].weights, self.embedding[1]
        values = values.to(pos.device, torch.float32).contiguous()
        out = torch.empty((values.numel(), self.features), dtype=torch.float32, device=pos.device)
        _hip.check(_hip.lib().sat_number_embed(_hip.ptr(values), values.numel(), float(min_val), float(max_val),
                                               _hip.ptr(pos.detach().float().contiguous()), pos.numel(),
                                               _hip.ptr(lin.weight.detach().float().contiguous()), _hip.ptr(lin.bias.detach().float().contiguous()),
                                               self.features, _hip.ptr(out), _hip.stream()))
        return out


class NumberConditioner(Conditioner):
    """A list of numbers -> ``[B, 1, output_dim]`` embeddings and an all-ones ``[B, 1]`` mask (conditioners.py:64-102)."""

    def __init__(self, output_dim: int, min_val: float = 0, max_val: float = 1):
        super().__init__(output_dim, output_dim)
        self.min_val, self.max_val = min_val, max_val
        self.embedder = NumberEmbedder(features=output_dim)

    @property
    def device(self):
        return next(self.embedder.parameters()).device

    def set_device(self, device):
        self.to(device)

    @torch.no_grad()
    def forward(self, floats: tp.List[float]) -> tp.Any:
        values = torch.tensor([float(v) for v in floats], dtype=torch.float32)
        embeds = self.embedder(values, self.min_val, self.max_val).unsqueeze(1)
        return [embeds, torch.ones(embeds.shape[0], 1, device=embeds.device)]


class T5Conditioner(Conditioner):
    """Prompts -> ``[B, max_length, output_dim]`` T5 encoder states (zero at padding) and the boolean attention mask
    (conditioners.py:261-346).  The encoder (``transformers.T5EncoderModel`` in the reference, under fp16 autocast) runs in fp32 on
    ``sat_t5_encode``; ``proj_out`` and the final mask multiply happen in the same call.  As in the reference the encoder weights
    live outside the module's state dict."""

    T5_MODEL_DIMS = {"t5-small": 512, "t5-base": 768, "t5-large": 1024, "t5-3b": 1024, "t5-11b": 1024,
                     "google/flan-t5-small": 512, "google/flan-t5-base": 768, "google/flan-t5-large": 1024,
                     "google/flan-t5-xl": 2048, "google/flan-t5-xxl": 4096}

    def __init__(self, output_dim: int, t5_model_name: str = "t5-base", max_length: int = 128, enable_grad: bool = False,
                 project_out: bool = False):
        if t5_model_name not in self.T5_MODEL_DIMS:
            raise ValueError(f"Unknown T5 model name: {t5_model_name}")
        if enable_grad:
            raise NotImplementedError("T5Conditioner: the HIP encoder is inference-only (enable_grad=True is a training option)")
        super().__init__(self.T5_MODEL_DIMS[t5_model_name], output_dim, project_out=project_out)
        self.t5_model_name, self.max_length = t5_model_name, max_length
        self.tokenizer = None
        self.__dict__["_enc"] = None          # (plan handle, device, params_version of proj_out) -- not a submodule, not in state_dict
        self.__dict__["_enc_src"] = None      # (state dict on the host, config) kept to rebuild the plan after .to(device) / a weight load
        self.__dict__["_ws"] = None
        self._device = "cpu"

    # ---------------------------------------------------------------- encoder weights
    @classmethod
    def cached_locally(cls, t5_model_name: str) -> bool:
        """True when tokenizer and encoder weights of ``t5_model_name`` can be loaded without a download."""
        try:
            from huggingface_hub import try_to_load_from_cache
            from transformers import AutoConfig, AutoTokenizer
            AutoConfig.from_pretrained(t5_model_name, local_files_only=True)
            AutoTokenizer.from_pretrained(t5_model_name, local_files_only=True)
            # a cache that holds only config.json would register the conditioner and then fail at the first forward: probe the weights
            return any(isinstance(try_to_load_from_cache(t5_model_name, f), str)
                       for f in ("model.safetensors", "pytorch_model.bin", "model.safetensors.index.json", "pytorch_model.bin.index.json"))
        except Exception:
            return False

    def load_encoder(self, state_dict: tp.Dict[str, torch.Tensor], config: tp.Any, tokenizer: tp.Any = None) -> "T5Conditioner":
        """Hand over a Hugging Face T5 encoder: ``state_dict`` with the checkpoint's key names (``T5EncoderModel.state_dict()``),
        ``config`` with the ``T5Config`` attributes, ``tokenizer`` a callable with the ``transformers`` tokenizer interface."""
        if config.d_model != self.dim:
            raise ValueError(f"T5 config d_model {config.d_model} != {self.dim} expected for {self.t5_model_name}")
        act = getattr(config, "feed_forward_proj", "relu")
        if act not in ("relu", "gated-gelu"):
            raise NotImplementedError(f"T5 feed_forward_proj {act!r} (supported: 'relu', 'gated-gelu')")
        keep = {k: v.detach().to("cpu", torch.float32) for k, v in state_dict.items() if k.startswith("encoder.") or k == "shared.weight"}
        self.__dict__["_enc_src"] = (keep, config)
        self._drop_plan()
        if tokenizer is not None:
            self.tokenizer = tokenizer
        return self

    def _load_from_cache(self):
        from transformers import AutoTokenizer, T5EncoderModel
        try:
            tokenizer = AutoTokenizer.from_pretrained(self.t5_model_name, local_files_only=True)
            model = T5EncoderModel.from_pretrained(self.t5_model_name, local_files_only=True)
        except Exception as e:
            raise _hip.SatError(f"T5Conditioner: '{self.t5_model_name}' is not in the local Hugging Face cache ({type(e).__name__}); "
                                "call load_encoder(state_dict, config, tokenizer) or pass the embeddings through conditioning_tensors=") from e
        self.load_encoder(model.state_dict(), model.config, tokenizer)

    def _drop_plan(self):
        enc = self.__dict__.get("_enc")
        _hip.destroy_plan("t5", enc and enc[0])
        self.__dict__["_enc"] = None

    def __del__(self):
        try:
            self._drop_plan()
        except Exception:
            pass

    def _plan(self):
        from . import _init
        dev = torch.device(self._device)
        if dev.type != "cuda":
            raise _hip.SatError("T5Conditioner must be on a HIP device (set_device('cuda')); there is no CPU path")
        ver = _init.params_version(self)
        enc = self.__dict__["_enc"]
        if enc is not None and enc[1] == dev and enc[2] == ver:
            return enc[0]
        self._drop_plan()
        if self.__dict__["_enc_src"] is None:
            self._load_from_cache()
        sd, config = self.__dict__["_enc_src"]
        lib = _hip.lib()
        has_proj = isinstance(self.proj_out, nn.Linear)
        cfg = _hip.SatT5Cfg(config.vocab_size, config.d_model, config.d_kv, config.d_ff, config.num_layers, config.num_heads,
                            config.relative_attention_num_buckets, getattr(config, "relative_attention_max_distance", 128),
                            1 if getattr(config, "feed_forward_proj", "relu") == "gated-gelu" else 0,
                            self.output_dim if has_proj else 0, float(config.layer_norm_epsilon))
        tensors = dict(sd)
        if has_proj:
            tensors["proj_out.weight"], tensors["proj_out.bias"] = self.proj_out.weight, self.proj_out.bias
        plan = _hip.build_plan("t5", lambda: _hip.new_handle(lib.sat_t5_plan_create, ctypes.byref(cfg)), tensors, dev)
        self.__dict__["_enc"] = (plan, dev, ver)
        return plan

    # ---------------------------------------------------------------- Conditioner interface
    def set_device(self, device):
        self.to(device)
        self._device = str(device)

    @torch.no_grad()
    def encode_ids(self, input_ids: torch.Tensor, attention_mask: torch.Tensor) -> tp.Tuple[torch.Tensor, torch.Tensor]:
        """Tokenised prompts ``[B, L]`` -> (``[B, L, output_dim]`` fp32, boolean mask), the tail of conditioners.py:326-343."""
        plan = self._plan()
        dev = torch.device(self._device)
        ids = input_ids.to(dev, torch.int32).contiguous()
        mask = attention_mask.to(dev, torch.int32).contiguous()
        b, l = ids.shape
        ws = self.__dict__["_ws"] = _hip.plan_workspace("t5", plan, self.__dict__["_ws"], dev, b, l)
        out = torch.empty((b, l, self.output_dim), dtype=torch.float32, device=dev)
        _hip.check(_hip.lib().sat_t5_encode(plan, _hip.ptr(ids), _hip.ptr(mask), _hip.ptr(out), b, l, 1, _hip.ptr(ws), ws.numel(), _hip.stream()))
        return out, mask.to(torch.bool)

    def forward(self, texts: tp.List[str]) -> tp.Tuple[torch.Tensor, torch.Tensor]:
        if self.tokenizer is None:
            self._load_from_cache()
        encoded = self.tokenizer(texts, truncation=True, max_length=self.max_length, padding="max_length", return_tensors="pt")
        return self.encode_ids(encoded["input_ids"], encoded["attention_mask"])


class RobertaEncoderPlan:
    """A finalized ``sat_roberta_plan`` on one device: ``hidden_states[run_layers]`` of a Hugging Face ``RobertaModel`` (+ an optional
    ``proj_out``) for tokenised prompts.  ``state_dict`` holds ``RobertaModel.state_dict()`` keys; only the embeddings and the first
    ``run_layers`` layers are uploaded."""

    def __init__(self, state_dict: tp.Dict[str, torch.Tensor], shape: tp.Dict[str, tp.Any], run_layers: int, device: tp.Any,
                 proj: tp.Optional[tp.Tuple[torch.Tensor, torch.Tensor]] = None):
        dev = torch.device(device)
        if dev.type != "cuda":
            raise _hip.SatError("the RoBERTa encoder must be on a HIP device (set_device('cuda')); there is no CPU path")
        lib = _hip.lib()
        self.out_dim = proj[0].shape[0] if proj is not None else shape["hidden_size"]
        cfg = _hip.SatRobertaCfg(shape["vocab_size"], shape["hidden_size"], shape["num_layers"], run_layers, shape["num_heads"],
                                 shape["intermediate_size"], shape["max_positions"], shape["pad_id"],
                                 self.out_dim if proj is not None else 0, float(shape["eps"]))
        self.handle, self.device, self._ws = None, dev, None
        wanted = lambda k: k.startswith("embeddings.") or int(k.split(".")[2]) < run_layers
        tensors = {k: v for k, v in state_dict.items() if wanted(k)}
        if proj is not None:
            tensors["proj_out.weight"], tensors["proj_out.bias"] = proj
        self.handle = _hip.build_plan("roberta", lambda: _hip.new_handle(lib.sat_roberta_plan_create, ctypes.byref(cfg)), tensors, dev)

    def close(self):
        _hip.destroy_plan("roberta", self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @torch.no_grad()
    def encode(self, input_ids: torch.Tensor, attention_mask: torch.Tensor) -> torch.Tensor:
        """``[B, L]`` ids and mask -> ``[B, L, out_dim]`` fp32 (padded rows are computed, not zeroed)."""
        dev = self.device
        ids = input_ids.to(dev, torch.int32).contiguous()
        mask = attention_mask.to(dev, torch.int32).contiguous()
        b, l = ids.shape
        self._ws = _hip.plan_workspace("roberta", self.handle, self._ws, dev, b, l)
        out = torch.empty((b, l, self.out_dim), dtype=torch.float32, device=dev)
        _hip.check(_hip.lib().sat_roberta_encode(self.handle, _hip.ptr(ids), _hip.ptr(mask), _hip.ptr(out), b, l, _hip.ptr(self._ws),
                                          self._ws.numel(), _hip.stream()))
        return out


_ROBERTA_PREFIXES = ("", "text_branch.", "module.text_branch.")
_ROBERTA_SKIP = ("embeddings.position_ids", "embeddings.token_type_ids")


def roberta_encoder_tensors(state_dict: tp.Dict[str, torch.Tensor], config: tp.Any = None):
    """Picks the RoBERTa encoder out of ``state_dict`` -- ``RobertaModel`` keys, bare or behind ``text_branch.`` /
    ``module.text_branch.`` (a laion_clap checkpoint) -- and reads its sizes from the tensor shapes.  Everything else (audio branch,
    projections, ``logit_scale_*``, ``embeddings.position_ids``, ``pooler.*``) is ignored.  Returns (tensors on the host in fp32, shape dict).
    ``config`` (``RobertaConfig`` attributes) supplies what shapes cannot: heads (default hidden // 64), pad id (1), eps (1e-5)."""
    prefix = next((p for p in _ROBERTA_PREFIXES if p + "embeddings.word_embeddings.weight" in state_dict), None)
    if prefix is None:
        raise ValueError("no RoBERTa encoder in the state dict: 'embeddings.word_embeddings.weight' not found bare, behind "
                         "'text_branch.' or behind 'module.text_branch.'")
    sd = {}
    for k, v in state_dict.items():
        if not k.startswith(prefix):
            continue
        k = k[len(prefix):]
        if (k.startswith("embeddings.") and k not in _ROBERTA_SKIP) or re.match(r"encoder\.layer\.\d+\.", k):
            sd[k] = v.detach().to("cpu", torch.float32)
    vocab, hidden = sd["embeddings.word_embeddings.weight"].shape
    layers = 1 + max((int(k.split(".")[2]) for k in sd if k.startswith("encoder.layer.")), default=-1)
    if layers < 1:
        raise ValueError("the RoBERTa state dict has no 'encoder.layer.N.' tensors")
    inter = sd["encoder.layer.0.intermediate.dense.weight"].shape[0]
    shape = {"vocab_size": vocab, "hidden_size": hidden, "num_layers": layers, "intermediate_size": inter,
             "max_positions": sd["embeddings.position_embeddings.weight"].shape[0],
             "num_heads": getattr(config, "num_attention_heads", None) or hidden // 64,
             "pad_id": 1 if getattr(config, "pad_token_id", None) is None else config.pad_token_id,
             "eps": getattr(config, "layer_norm_eps", None) or 1e-5}
    want = {"embeddings.word_embeddings.weight": (vocab, hidden), "embeddings.position_embeddings.weight": (shape["max_positions"], hidden),
            "embeddings.LayerNorm.weight": (hidden,), "embeddings.LayerNorm.bias": (hidden,)}
    for n in range(layers):
        pf = f"encoder.layer.{n}."
        for lin, (o, i) in {"attention.self.query": (hidden, hidden), "attention.self.key": (hidden, hidden),
                            "attention.self.value": (hidden, hidden), "attention.output.dense": (hidden, hidden),
                            "intermediate.dense": (inter, hidden), "output.dense": (hidden, inter)}.items():
            want[pf + lin + ".weight"], want[pf + lin + ".bias"] = (o, i), (o,)
        for ln in ("attention.output.LayerNorm", "output.LayerNorm"):
            want[pf + ln + ".weight"] = want[pf + ln + ".bias"] = (hidden,)
    for k, shp in want.items():
        if k not in sd:
            raise ValueError(f"RoBERTa state dict: '{prefix}{k}' is missing")
        if tuple(sd[k].shape) != shp:
            raise ValueError(f"RoBERTa state dict: '{prefix}{k}' has shape {tuple(sd[k].shape)}, expected {shp}")
    tt = sd.get("embeddings.token_type_embeddings.weight")
    if tt is None or tt.ndim != 2 or tt.shape[1] != hidden:
        raise ValueError(f"RoBERTa state dict: '{prefix}embeddings.token_type_embeddings.weight' must be [type_vocab_size, {hidden}]")
    return sd, shape


class CLAPTextConditioner(Conditioner):
    """Prompts -> ``[B, 77, output_dim]`` per-token features of CLAP's text branch and the tokenizer's attention mask
    (conditioners.py:105-193 with ``use_text_features=True``): tokenizer -> RoBERTa ``hidden_states[feature_layer_ix]`` -> ``proj_out``.
    The encoder (``laion_clap``'s ``text_branch``, a ``transformers.RobertaModel``, under fp16 autocast in the reference) runs in fp32
    on ``sat_roberta_encode``, which evaluates only the layers below ``feature_layer_ix`` and applies ``proj_out`` in the same call.
    Padded rows are returned as computed, not zeroed, as in the reference.  As in the reference the encoder weights live outside
    the module's state dict, which holds ``proj_out.*`` only.

    The weights come from ``load_encoder`` or, lazily at the first call, from the laion_clap checkpoint at ``clap_ckpt_path``
    (``torch.load`` -> ``["state_dict"]`` -> ``module.text_branch.*``, what laion_clap's ``load_state_dict`` does in
    conditioners.py:131-141).  That loading path is written against the reference's usage and has NOT been run on a real
    ``music_audioset_epoch_15_esc_90.14.pt``: none is available offline; the tests use a synthetic file of the same layout.

    Refused: ``finetune=True`` (training) and ``use_text_features=False`` (the pooled 512-d embedding goes through laion_clap's
    ``text_projection`` and normalisation, which this build cannot pin against anything; such an entry stays an external id).
    ``audio_model_type`` / ``enable_fusion`` describe the audio branch, which the text conditioner deletes: accepted and unused."""

    MAX_LENGTH = 77                # laion_clap's tokenizer call (hook.py: max_length=77)
    TOKENIZER_NAME = "roberta-base"

    def __init__(self, output_dim: int, clap_ckpt_path: str, use_text_features: bool = False, feature_layer_ix: int = -1,
                 audio_model_type: str = "HTSAT-base", enable_fusion: bool = True, project_out: bool = False, finetune: bool = False):
        if finetune:
            raise NotImplementedError("CLAPTextConditioner: the HIP encoder is inference-only (finetune=True is a training option)")
        if not use_text_features:
            raise NotImplementedError("CLAPTextConditioner: use_text_features=False (the pooled, projected and normalised 512-d CLAP "
                                      "embedding) is not computed by this build; pass that embedding through conditioning_tensors=")
        super().__init__(768 if use_text_features else 512, output_dim, project_out=project_out)
        self.clap_ckpt_path, self.use_text_features, self.feature_layer_ix = clap_ckpt_path, use_text_features, feature_layer_ix
        self.finetune = finetune
        self.tokenizer = None
        self.__dict__["_enc"] = None          # (RobertaEncoderPlan, params_version of proj_out) -- not a submodule, not in state_dict
        self.__dict__["_enc_src"] = None      # (state dict on the host, shape dict) kept to rebuild the plan after .to(device) / a weight load
        self._device = "cpu"

    # ---------------------------------------------------------------- encoder weights
    def load_encoder(self, state_dict: tp.Dict[str, torch.Tensor], config: tp.Any = None, tokenizer: tp.Any = None) -> "CLAPTextConditioner":
        """Hand over the text branch: ``state_dict`` with ``RobertaModel.state_dict()`` keys, bare or behind ``text_branch.`` /
        ``module.text_branch.`` (unrelated keys are ignored); sizes are read from the shapes, ``config`` (optional, ``RobertaConfig``
        attributes) gives heads / pad id / eps; ``tokenizer`` is a callable with the ``transformers`` tokenizer interface."""
        sd, shape = roberta_encoder_tensors(state_dict, config)
        if shape["hidden_size"] != self.dim:
            raise ValueError(f"RoBERTa hidden size {shape['hidden_size']} != {self.dim}, the feature width of CLAPTextConditioner")
        n = self.feature_layer_ix if self.feature_layer_ix >= 0 else shape["num_layers"] + 1 + self.feature_layer_ix
        if not 0 <= n <= shape["num_layers"]:
            raise ValueError(f"feature_layer_ix {self.feature_layer_ix} is outside the {shape['num_layers'] + 1} hidden states of the encoder")
        self.__dict__["_enc_src"] = (sd, shape, n)
        self._drop_plan()
        if tokenizer is not None:
            self.tokenizer = tokenizer
        return self

    def _load_from_ckpt(self):
        if not (self.clap_ckpt_path and os.path.exists(self.clap_ckpt_path)):
            raise _hip.SatError(f"CLAPTextConditioner: no CLAP checkpoint at '{self.clap_ckpt_path}'; call load_encoder(state_dict, ...) "
                                "or pass the embeddings through conditioning_tensors=")
        ckpt = torch.load(self.clap_ckpt_path, map_location="cpu", weights_only=True)
        if isinstance(ckpt, dict) and "state_dict" in ckpt:
            ckpt = ckpt["state_dict"]
        # laion_clap strips a leading "module." (DataParallel); load_encoder accepts the key with or without it
        self.load_encoder(ckpt)

    def _load_tokenizer(self):
        try:
            from transformers import AutoTokenizer
            self.tokenizer = AutoTokenizer.from_pretrained(self.TOKENIZER_NAME, local_files_only=True)
        except Exception as e:
            raise _hip.SatError(f"CLAPTextConditioner: the '{self.TOKENIZER_NAME}' tokenizer is not in the local Hugging Face cache "
                                f"({type(e).__name__}) and nothing is downloaded; hand one over with load_encoder(..., tokenizer=)") from e

    def _drop_plan(self):
        enc = self.__dict__.get("_enc")
        if enc is not None:
            enc[0].close()
        self.__dict__["_enc"] = None

    def __del__(self):
        try:
            self._drop_plan()
        except Exception:
            pass

    def _plan(self) -> RobertaEncoderPlan:
        from . import _init
        dev = torch.device(self._device)
        if dev.type != "cuda":
            raise _hip.SatError("CLAPTextConditioner must be on a HIP device (set_device('cuda')); there is no CPU path")
        ver = _init.params_version(self)
        enc = self.__dict__["_enc"]
        if enc is not None and enc[0].device == dev and enc[1] == ver:
            return enc[0]
        self._drop_plan()
        if self.__dict__["_enc_src"] is None:
            self._load_from_ckpt()
        sd, shape, n = self.__dict__["_enc_src"]
        proj = (self.proj_out.weight, self.proj_out.bias) if isinstance(self.proj_out, nn.Linear) else None
        plan = RobertaEncoderPlan(sd, shape, n, dev, proj)
        self.__dict__["_enc"] = (plan, ver)
        return plan

    # ---------------------------------------------------------------- Conditioner interface
    def set_device(self, device):
        self.to(device)
        self._device = str(device)

    @torch.no_grad()
    def encode_ids(self, input_ids: torch.Tensor, attention_mask: torch.Tensor) -> tp.List[torch.Tensor]:
        """Tokenised prompts ``[B, L]`` -> [``[B, L, output_dim]`` fp32, the attention mask on the device with the dtype it came in]."""
        plan = self._plan()
        return [plan.encode(input_ids, attention_mask), attention_mask.to(plan.device)]

    def forward(self, texts: tp.List[str]) -> tp.List[torch.Tensor]:
        """The reference encodes ``[texts[0], ""]`` for a single prompt and drops the second row (a laion_clap work-around,
        conditioners.py:175-178); sequences are independent here, so the one prompt is encoded alone with the same result."""
        if self.tokenizer is None:
            self._load_tokenizer()
        encoded = self.tokenizer(list(texts), padding="max_length", truncation=True, max_length=self.MAX_LENGTH, return_tensors="pt")
        return self.encode_ids(encoded["input_ids"], encoded["attention_mask"])


class MultiConditioner(nn.Module):
    """Applies each conditioner to its entry of the per-item metadata dicts (conditioners.py:506-549)."""

    def __init__(self, conditioners: tp.Dict[str, Conditioner], default_keys: tp.Dict[str, str] = {}):
        super().__init__()
        self.conditioners = nn.ModuleDict(conditioners)
        self.default_keys = default_keys
        self.external_ids: tp.List[str] = []

    def set_device(self, device):
        for conditioner in self.conditioners.values():
            conditioner.set_device(device)

    def forward(self, batch_metadata: tp.List[tp.Dict[str, tp.Any]]) -> tp.Dict[str, tp.Any]:
        out = {}
        for key, conditioner in self.conditioners.items():
            lookup, inputs = key, []
            for item in batch_metadata:
                if lookup not in item:
                    if lookup not in self.default_keys:
                        raise ValueError(f"Conditioner key {lookup} not found in batch metadata")
                    lookup = self.default_keys[lookup]        # sticks for the rest of the batch, as in the reference (:533-538)
                value = item[lookup]
                # the reference unwraps ANY list, but a tuple only when it has exactly one element (operator precedence, :541)
                if isinstance(value, list) or (isinstance(value, tuple) and len(value) == 1):
                    value = value[0]
                inputs.append(value)
            out[key] = conditioner(inputs)
        return out


def create_multi_conditioner_from_conditioning_config(config: tp.Dict[str, tp.Any]) -> MultiConditioner:
    """conditioners.py:552-599 for the conditioner types this build evaluates: "number", "t5" when its weights are in the local
    Hugging Face cache, and "clap_text" when it asks for text features and the file at ``clap_ckpt_path`` exists; the other
    encoder-backed types are listed in ``external_ids`` instead of being instantiated."""
    built, external = {}, []
    for entry in config["configs"]:
        kind = entry["type"]
        if kind == "number":
            built[entry["id"]] = NumberConditioner(**{"output_dim": config["cond_dim"], **entry["config"]})
        elif kind == "t5" and T5Conditioner.cached_locally(entry["config"].get("t5_model_name", "t5-base")):
            built[entry["id"]] = T5Conditioner(**{"output_dim": config["cond_dim"], **entry["config"]})
        elif (kind == "clap_text" and entry["config"].get("use_text_features", False) and not entry["config"].get("finetune", False)
              and os.path.exists(entry["config"].get("clap_ckpt_path") or "")):
            built[entry["id"]] = CLAPTextConditioner(**{"output_dim": config["cond_dim"], **entry["config"]})
        elif kind == "t5" or kind in _EXTERNAL_TYPES:
            external.append(entry["id"])
        else:
            raise ValueError(f"Unknown conditioner type: {kind}")
    multi = MultiConditioner(built, default_keys=config.get("default_keys", {}))
    multi.external_ids = external
    return multi
