"""NunchakuT5EncoderModel: the 4-bit (AWQ W4A16, group 128) T5 text encoder of the FLUX pipelines, loaded from one local
``.safetensors`` file (role of the reference's ``nunchaku/models/text_encoders/t5_encoder.py``).  Every ``nn.Linear`` with a
``<name>.qweight`` entry in the file becomes a :class:`W4Linear`; everything else is transformers' ``T5EncoderModel``.
transformers is imported when this module is."""

import json
import os

import torch
from torch import nn
from transformers import T5Config, T5EncoderModel

from .linear import W4Linear

__all__ = ["NunchakuT5EncoderModel"]

# tied embedding of T5EncoderModel: a file that stores one of the two names serves both
_TIED = ("shared.weight", "encoder.embed_tokens.weight")


def _read_safetensors(path: str) -> tuple[dict, dict]:
    from safetensors import safe_open

    tensors = {}
    with safe_open(path, framework="pt", device="cpu") as f:
        meta = f.metadata() or {}
        for k in f.keys():
            tensors[k] = f.get_tensor(k)
    return tensors, meta


class NunchakuT5EncoderModel(T5EncoderModel):
    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path: str | os.PathLike, **kwargs) -> T5EncoderModel:
        """``pretrained_model_name_or_path``: a local ``.safetensors`` file whose metadata entry ``config`` holds the T5 config
        as JSON (hub names are not resolved).  ``torch_dtype`` (default bfloat16) is the compute dtype, ``device`` (default
        ``"cuda"``) where the model is materialised.  The model is built on the meta device, its quantised linears swapped
        for W4Linear (group 128), then materialised and loaded with ``strict=True``."""
        path = os.fspath(pretrained_model_name_or_path)
        if not os.path.isfile(path):
            raise FileNotFoundError(f"NunchakuT5EncoderModel.from_pretrained: {path!r} is not a local .safetensors file "
                                    "(download the checkpoint first; hub names are not resolved)")
        state_dict, meta = _read_safetensors(path)
        if "config" not in meta:
            raise ValueError(f"{path}: no 'config' entry in the safetensors metadata")
        config = T5Config(**json.loads(meta["config"]))
        dtype = kwargs.get("torch_dtype", torch.bfloat16)
        with torch.device("meta"):
            model = T5EncoderModel(config).to(dtype)
        model.eval()
        modules = dict(model.named_modules())
        for name, module in list(modules.items()):
            if isinstance(module, nn.Linear) and f"{name}.qweight" in state_dict:
                q = W4Linear.from_linear(module, group_size=128, init_only=True)
                parent, child = name.rsplit(".", 1)
                setattr(modules[parent], child, q)
        for a, b in (_TIED, _TIED[::-1]):
            if a not in state_dict and b in state_dict:
                state_dict[a] = state_dict[b]
        device = torch.device(kwargs.get("device", "cuda"))
        model.to_empty(device=device)
        model.load_state_dict(state_dict, strict=True)
        return model
