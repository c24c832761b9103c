"""IP-Adapter for the FLUX transformer (reference: nunchaku/models/ip_adapter/utils.py, diffusers_adapters/flux.py).

The adapter is state on the engine -- ``transformer.ip_adapter``, an :class:`IPAdapter` -- not a replacement of its blocks: the
per-block image-prompt projections ``ip_k_projs`` / ``ip_v_projs`` (dense 16-bit ``nn.Linear(cross_dim -> dim)``), the strength
``ip_adapter_scale`` and the stored ``image_embeds``.  ``FluxEngineMixin._run_joint`` runs the adapter's step behind every joint block
(models/flux.py ``_ip_query`` / ``_ip_add``): the query is the block's OUTPUT image stream pushed through this
block's ``norm1`` modulation, ``to_qkv``, ``norm_q`` and RoPE a second time, as the reference's ``forward_layer_ip_adapter`` does.

``k_img`` / ``v_img`` depend on the image embeddings only, not on the timestep: they are projected once per embeddings tensor and kept
(:meth:`IPAdapter.kv`; the reference runs the 2 x blocks GEMMs every step)."""

from __future__ import annotations

import os
import re

import torch
from torch import nn

_KEY = re.compile(r"^(\d+)\.processor\.ip_adapter_double_stream_([kv])_proj\.(weight|bias)$")


def _read_state_dict(source, filename: str = "ip_adapter.safetensors") -> dict:
    """``source``: a state dict, a local ``.safetensors`` file, a directory holding ``filename`` -- or, only when the string names no
    existing path, a Hugging Face hub repository id (``hf_hub_download``; needs network access)."""
    if isinstance(source, dict):
        return source
    path = os.fspath(source)
    if os.path.isdir(path):
        path = os.path.join(path, filename)
        if not os.path.isfile(path):
            raise FileNotFoundError(path)
    elif not os.path.isfile(path):
        from huggingface_hub import hf_hub_download

        path = hf_hub_download(repo_id=path, filename=filename)
    from safetensors import safe_open

    sd = {}
    with safe_open(path, framework="pt", device="cpu") as f:
        for k in f.keys():
            sd[k] = f.get_tensor(k)
    return sd


def _embeds_version(t: torch.Tensor):
    """version counter of the embeddings tensor, or None when it tracks none (inference tensors raise on ``._version``)"""
    try:
        return None if t.is_inference() else t._version
    except RuntimeError:
        return None


class IPAdapter(nn.Module):
    """Per-block image-prompt K / V projections, the strength and the stored embeddings of one transformer."""

    def __init__(self, ip_adapter_scale: float = 1.0):
        super().__init__()
        self.ip_adapter_scale = float(ip_adapter_scale)
        self.ip_k_projs = nn.ModuleList()
        self.ip_v_projs = nn.ModuleList()
        self.image_embeds = None
        self.cross_dim = self.dim = 0
        self._kv_cache = None  # (embeds tensor, its version, [(k_img, v_img)] per block)

    @torch.no_grad()
    def load_ip_adapter_weights_per_layer(self, source, prefix: str = "double_blocks.", *, num_blocks: int | None = None,
                                          dim: int | None = None, dtype: torch.dtype = torch.bfloat16, device="cuda",
                                          filename: str = "ip_adapter.safetensors"):
        """Keys ``{prefix}{i}.processor.ip_adapter_double_stream_{k,v}_proj.{weight,bias}`` (the reference's).  ``cross_dim`` and ``dim``
        come from the weights' shapes and the block count from the keys; ``num_blocks`` / ``dim`` (the transformer's) must agree."""
        sd = _read_state_dict(source, filename)
        layers: dict = {}
        for key, t in sd.items():
            if not key.startswith(prefix):
                continue
            m = _KEY.match(key[len(prefix):])
            if m is not None:
                layers.setdefault(int(m.group(1)), {})[m.group(2) + "." + m.group(3)] = t
        if not layers:
            raise KeyError(f"no '{prefix}<i>.processor.ip_adapter_double_stream_k_proj.weight' keys: not an IP-Adapter file")
        ids = sorted(layers)
        if ids != list(range(len(ids))):
            raise KeyError(f"IP-Adapter blocks {ids} are not 0 .. {len(ids) - 1}")
        for i in ids:
            missing = [n for n in ("k.weight", "k.bias", "v.weight", "v.bias") if n not in layers[i]]
            if missing:
                raise KeyError(f"IP-Adapter block {i}: missing " + ", ".join(
                    f"{prefix}{i}.processor.ip_adapter_double_stream_{n[0]}_proj.{n[2:]}" for n in missing))
        if num_blocks is not None and len(ids) != num_blocks:
            raise ValueError(f"the IP-Adapter file has {len(ids)} blocks, the transformer {num_blocks} joint blocks")
        out_dim, cross_dim = layers[0]["k.weight"].shape
        if dim is not None and out_dim != dim:
            raise ValueError(f"the IP-Adapter projects to {out_dim} channels, the transformer has {dim}")
        ks, vs = nn.ModuleList(), nn.ModuleList()
        for i in ids:
            for name, lst in (("k", ks), ("v", vs)):
                w, b = layers[i][name + ".weight"], layers[i][name + ".bias"]
                if tuple(w.shape) != (out_dim, cross_dim) or tuple(b.shape) != (out_dim,):
                    raise ValueError(f"IP-Adapter block {i} {name}_proj: expected weight [{out_dim}, {cross_dim}] and bias [{out_dim}], "
                                     f"got {tuple(w.shape)} and {tuple(b.shape)}")
                lin = nn.Linear(cross_dim, out_dim, bias=True, device=device, dtype=dtype)
                lin.weight.copy_(w)
                lin.bias.copy_(b)
                lst.append(lin)
        self.ip_k_projs, self.ip_v_projs = ks, vs
        self.cross_dim, self.dim = cross_dim, out_dim
        self._kv_cache = None
        return self

    def set_ip_hidden_states(self, image_embeds, negative_image_embeds=None):
        """Store the image embeddings used when a call passes none (``negative_image_embeds`` is accepted and unused, as in the reference)."""
        self.image_embeds = image_embeds

    def resolve(self, ip_hidden_states=None) -> torch.Tensor:
        """The embeddings tensor of a step: the call's (the pipeline's list: element 0) or the stored one."""
        x = ip_hidden_states if ip_hidden_states is not None else self.image_embeds
        if isinstance(x, (list, tuple)):
            x = x[0] if len(x) else None
        if x is None:
            raise ValueError("an IP-Adapter is attached but there are no image embeddings: pass joint_attention_kwargs['ip_hidden_states'] "
                             "or call set_ip_hidden_states(image_embeds) first")
        return x

    def _project(self, x: torch.Tensor) -> list:
        """``[(k_img, v_img)]`` per block, each ``[N_ip, dim]``: all leading axes of ``x`` are image-prompt tokens"""
        w = self.ip_k_projs[0].weight
        x2 = x.to(device=w.device, dtype=w.dtype).reshape(-1, x.shape[-1])
        return [(k(x2), v(x2)) for k, v in zip(self.ip_k_projs, self.ip_v_projs)]

    @torch.no_grad()
    def kv(self, embeds: torch.Tensor) -> list:
        """The projections of ``embeds``, computed once per tensor: one entry, keyed on the tensor OBJECT (held, so "the same object"
        cannot be a recycled address) and its version counter (an in-place edit projects again).  Not cached: a tensor without a
        readable version, and while the stream is capturing (the graph's pool owns what is made under capture; a graph must not bake
        in pointers that only this one-entry cache keeps alive)."""
        ver = _embeds_version(embeds)
        capturing = self.ip_k_projs[0].weight.is_cuda and torch.cuda.is_current_stream_capturing()
        use_cache = ver is not None and not capturing
        c = self._kv_cache if use_cache else None
        if c is not None and c[0] is embeds and c[1] == ver:
            return c[2]
        kv = self._project(embeds)
        if use_cache:
            self._kv_cache = (embeds, ver, kv)
        return kv


def attach(transformer, source, ip_adapter_scale: float = 1.0) -> IPAdapter:
    """Load ``source`` (see :func:`_read_state_dict`) and make it ``transformer.ip_adapter``.  A captured step has to be captured
    again afterwards (new launches; the strength is a kernel argument)."""
    ad = IPAdapter(ip_adapter_scale)
    p = transformer.proj_out.weight
    ad.load_ip_adapter_weights_per_layer(source, num_blocks=len(transformer.transformer_blocks), dim=transformer.dim,
                                         dtype=getattr(transformer, "dtype_", p.dtype), device=p.device)
    transformer.ip_adapter = ad
    transformer._is_IPA = True
    return ad


def detach(transformer):
    """Remove the adapter (``undo_all_mods_on_transformer``)."""
    if getattr(transformer, "ip_adapter", None) is not None:
        del transformer.ip_adapter
    if getattr(transformer, "_is_IPA", False):
        transformer._is_IPA = False
    return transformer


def apply_IPA_on_transformer(transformer, *, ip_adapter_scale: float = 1.0, repo_id):
    """reference: diffusers_adapters/flux.py ``apply_IPA_on_transformer``.  ``repo_id``: a local ``.safetensors`` file, a directory
    holding ``ip_adapter.safetensors``, a state dict, or a hub repository id.  Works with First-Block Cache applied before or after
    (the adapter's step lives in the stage both forwards share).  Adds ``transformer.set_ip_hidden_states``."""
    from .flux import FluxEngineMixin

    if not isinstance(transformer, FluxEngineMixin):
        raise TypeError(f"apply_IPA_on_transformer: {type(transformer).__name__} is not a FLUX transformer of this library")
    ad = attach(transformer, repo_id, ip_adapter_scale)
    transformer.set_ip_hidden_states = ad.set_ip_hidden_states
    return transformer


def apply_IPA_on_pipe(pipe, **kwargs):
    """reference: diffusers_adapters/flux.py ``apply_IPA_on_pipe``"""
    apply_IPA_on_transformer(pipe.transformer, **kwargs)
    return pipe


def undo_all_mods_on_transformer(transformer):
    """reference: utils.py ``undo_all_mods_on_transformer`` -- here: detach the adapter (nothing else was modified)."""
    detach(transformer)
    if "set_ip_hidden_states" in getattr(transformer, "__dict__", {}):
        del transformer.__dict__["set_ip_hidden_states"]
    return transformer


def resize_numpy_image_long(image, resize_long_edge: int = 768):
    """reference: utils.py ``resize_numpy_image_long`` (OpenCV is imported here, not with the module)."""
    h, w = image.shape[:2]
    if max(h, w) <= resize_long_edge:
        return image
    import cv2

    k = resize_long_edge / max(h, w)
    return cv2.resize(image, (int(w * k), int(h * k)), interpolation=cv2.INTER_LANCZOS4)
