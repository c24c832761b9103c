"""PuLID for the FLUX transformer: the identity cross-attention modules and their place in the engine (reference:
nunchaku/models/pulid/encoders_transformer.py ``PerceiverAttentionCA``, nunchaku/models/pulid/pulid_forward.py, src/FluxModel.cpp
``residual_callback``).

After every second joint block and every fourth single block the image stream gets ``hidden += id_weight * pulid_ca[k](id_embeddings,
hidden)``.  The modules are state on the engine -- ``transformer.pulid_ca``, a ``ModuleList`` -- and ``FluxEngineMixin._run_joint`` /
``_run_single`` apply them (models/flux.py ``_pulid_add``).  ``id_embeddings`` is an input: the face stack that makes
it (EVA-CLIP, insightface, facexlib, the ``IDFormer`` encoder, ``PuLIDFluxPipeline``) is not part of this library.

K and V of a module depend on the identity embeddings only, and there are at most 32 identity tokens per head against a head dimension of
128: :meth:`PerceiverAttentionCA.fold` multiplies ``to_q`` into the keys and ``to_out`` into the values once per embeddings tensor, and
the step runs ``svdq_pulid_ca`` on the un-normalised stream (``ops.pulid_ca``)."""

from __future__ import annotations

import math
import re
from types import MethodType

import torch
from torch import nn

from .ip_adapter import _embeds_version, _read_state_dict

FOLD_TOKENS = 32  # identity tokens a head's folded key tile holds


class PulidFold:
    """``to_q`` folded into the keys and ``to_out`` into the values of one module for one embeddings tensor (row ``32 h + n``: head ``h``,
    identity token ``n``; rows with ``n >= tokens`` are zeros and are never read):
    ``a_fold`` / ``b_fold`` ``[heads * 32, dim]`` 16-bit, ``colsum`` / ``cbias`` ``[heads * 32]`` float32."""

    __slots__ = ("a_fold", "b_fold", "colsum", "cbias", "tokens")

    def __init__(self, a_fold, b_fold, colsum, cbias, tokens):
        self.a_fold, self.b_fold, self.colsum, self.cbias, self.tokens = a_fold, b_fold, colsum, cbias, int(tokens)


def fold_terms(k, v, wq, wo, w2, b2, heads: int):
    """The unrounded fold in the dtype of the arguments (float32 in the module, float64 in the tests): ``k`` / ``v`` ``[N, heads * d]``,
    ``wq`` ``[heads * d, dim]``, ``wo`` ``[dim, heads * d]``, ``w2`` / ``b2`` ``[dim]`` (``norm2``) ->
    ``a [heads, N, dim]``, ``cbias [heads, N]``, ``b [heads, N, dim]`` with
    ``scores_h = LN(x) . a_h^T + cbias_h`` and ``out = sum_h softmax(scores_h) . b_h``."""
    n = k.shape[0]
    d = k.shape[1] // heads
    g = torch.einsum("nhd,hdc->hnc", k.reshape(n, heads, d), wq.reshape(heads, d, -1)) / math.sqrt(d)
    b = torch.einsum("nhd,chd->hnc", v.reshape(n, heads, d), wo.reshape(-1, heads, d))
    return g * w2, g @ b2, b


class PerceiverAttentionCA(nn.Module):
    """reference: encoders_transformer.py ``PerceiverAttentionCA`` -- same children (``norm1``, ``norm2``, ``to_q``, ``to_kv``, ``to_out``),
    so a PuLID file's ``pulid_ca.<k>.*`` keys load as they are.  ``forward`` is the reference's torch-op sequence (the CPU arm and the
    non-fused arm); ``forward_fused`` runs ``svdq_pulid_ca`` on the fold of ``x``."""

    def __init__(self, *, dim=3072, dim_head=128, heads=16, kv_dim=2048, dtype=None, device=None):
        super().__init__()
        self.scale = dim_head ** -0.5
        self.dim_head = dim_head
        self.heads = heads
        inner_dim = dim_head * heads
        kw = dict(dtype=dtype, device=device)
        self.norm1 = nn.LayerNorm(dim if kv_dim is None else kv_dim, **kw)
        self.norm2 = nn.LayerNorm(dim, **kw)
        self.to_q = nn.Linear(dim, inner_dim, bias=False, **kw)
        self.to_kv = nn.Linear(dim if kv_dim is None else kv_dim, inner_dim * 2, bias=False, **kw)
        self.to_out = nn.Linear(inner_dim, dim, bias=False, **kw)
        self._fold_cache = None  # (embeddings tensor, its version, PulidFold)

    def forward(self, x, latents):
        """``x``: identity embeddings ``[B, N, kv_dim]``; ``latents``: the image stream ``[B, T, dim]`` -> ``[B, T, dim]``"""
        x = self.norm1(x)
        latents = self.norm2(latents)
        b, seq_len, _ = latents.shape
        q = self.to_q(latents)
        k, v = self.to_kv(x).chunk(2, dim=-1)
        heads = lambda t: t.view(t.shape[0], t.shape[1], self.heads, -1).transpose(1, 2)
        q, k, v = heads(q), heads(k), heads(v)
        scale = 1 / math.sqrt(math.sqrt(self.dim_head))
        weight = (q * scale) @ (k * scale).transpose(-2, -1)
        weight = torch.softmax(weight.float(), dim=-1).type(weight.dtype)
        out = weight @ v
        out = out.permute(0, 2, 1, 3).reshape(b, seq_len, -1)
        return self.to_out(out)

    def _make_fold(self, x: torch.Tensor) -> PulidFold:
        w = self.to_q.weight
        x2 = x.to(device=w.device, dtype=w.dtype).reshape(-1, x.shape[-1])
        n = x2.shape[0]
        if not 1 <= n <= FOLD_TOKENS:
            raise NotImplementedError(f"PuLID: {n} identity tokens: the folded kernel holds 1 .. {FOLD_TOKENS} per head (the reference's "
                                      "IDFormer makes 32); use the module's forward for other counts")
        k, v = self.to_kv(self.norm1(x2)).chunk(2, dim=-1)  # 16-bit, as the reference makes them
        f32 = lambda t: t.float()
        a, cb, b = fold_terms(f32(k), f32(v), f32(self.to_q.weight), f32(self.to_out.weight), f32(self.norm2.weight), f32(self.norm2.bias),
                              self.heads)
        dim, J = w.shape[1], self.heads * FOLD_TOKENS
        a_fold = torch.zeros(self.heads, FOLD_TOKENS, dim, dtype=w.dtype, device=w.device)
        b_fold = torch.zeros_like(a_fold)
        cbias = torch.zeros(self.heads, FOLD_TOKENS, dtype=torch.float32, device=w.device)
        a_fold[:, :n], b_fold[:, :n], cbias[:, :n] = a.to(w.dtype), b.to(w.dtype), cb  # rounded once
        # summed over the ROUNDED keys: the kernel's mean subtraction is then exact for the operands it multiplies
        colsum = a_fold.float().sum(dim=-1)
        return PulidFold(a_fold.view(J, dim), b_fold.view(J, dim), colsum.view(J).contiguous(), cbias.view(J), n)

    @torch.no_grad()
    def fold(self, x: torch.Tensor) -> PulidFold:
        """The fold of the embeddings ``x`` (``[N, kv_dim]`` or ``[1, N, kv_dim]``: all leading axes are identity tokens), computed once
        per tensor: one entry, keyed on the tensor OBJECT and its version counter, never while the stream is capturing -- the rule of
        ``IPAdapter.kv`` (a graph must not bake in pointers that only this one-entry cache keeps alive)."""
        ver = _embeds_version(x)
        capturing = self.to_q.weight.is_cuda and torch.cuda.is_current_stream_capturing()
        use_cache = ver is not None and not capturing
        c = self._fold_cache if use_cache else None
        if c is not None and c[0] is x and c[1] == ver:
            return c[2]
        f = self._make_fold(x)
        if use_cache:
            self._fold_cache = (x, ver, f)
        return f

    def forward_fused(self, x, latents, out_scale: float = 1.0, stats=None):
        """``out_scale * forward(x, latents)`` on the folded kernel: ``latents`` is the UN-normalised stream ``[T, dim]`` / ``[1, T, dim]``
        (``norm2`` runs inside the score epilogue; ``stats``: its (mean, rstd) rows for eps = 1e-5, or None)."""
        from ..ops.attention import pulid_ca

        if self.norm2.eps != 1e-5:
            raise NotImplementedError("PuLID: the folded kernel's statistics are formed for norm2.eps = 1e-5")
        return pulid_ca(latents, self.fold(x), out_scale=out_scale, stats=stats)

    def _load_from_state_dict(self, *args, **kwargs):
        self._fold_cache = None  # new weights: the entry is dropped
        return super()._load_from_state_dict(*args, **kwargs)


_KEY = re.compile(r"^pulid_ca\.(\d+)\.(.+)$")


def pulid_module_count(transformer) -> int:
    """``ceil(joint / 2) + ceil(single / 4)``: a module behind every second joint and every fourth single block (20 for FLUX.1-dev)"""
    return (len(transformer.transformer_blocks) + 1) // 2 + (len(transformer.single_transformer_blocks) + 3) // 4


@torch.no_grad()
def attach_pulid(transformer, source, filename: str = "pulid_flux_v0.9.1.safetensors") -> nn.ModuleList:
    """Load the ``pulid_ca.<k>.*`` tensors of ``source`` (a state dict, a ``.safetensors`` file or a directory holding ``filename``, read as
    ``ip_adapter._read_state_dict`` reads; ``pulid_encoder.*`` -- the IDFormer -- is ignored) into ``transformer.pulid_ca``.  Every module
    loads ``strict=True``; the module count must be the transformer's (:func:`pulid_module_count`).  A captured step has to be captured
    again afterwards."""
    sd = _read_state_dict(source, filename)
    layers: dict = {}
    for key, t in sd.items():
        m = _KEY.match(key)
        if m is not None:
            layers.setdefault(int(m.group(1)), {})[m.group(2)] = t
    if not layers:
        raise KeyError("no 'pulid_ca.<k>.to_q.weight' keys: not a PuLID file")
    ids = sorted(layers)
    if ids != list(range(len(ids))):
        raise KeyError(f"PuLID modules {ids} are not 0 .. {len(ids) - 1}")
    want = pulid_module_count(transformer)
    if len(ids) != want:
        raise ValueError(f"the PuLID file has {len(ids)} modules, the transformer needs {want} "
                         f"(ceil({len(transformer.transformer_blocks)} / 2) + ceil({len(transformer.single_transformer_blocks)} / 4))")
    p = transformer.proj_out.weight
    dtype, device = getattr(transformer, "dtype_", p.dtype), p.device
    mods = nn.ModuleList()
    for i in ids:
        for name in ("to_q.weight", "to_kv.weight"):
            if name not in layers[i]:
                raise KeyError(f"PuLID module {i}: missing pulid_ca.{i}.{name}")
        inner, dim = layers[i]["to_q.weight"].shape
        kv_dim = layers[i]["to_kv.weight"].shape[1]
        if dim != transformer.dim:
            raise ValueError(f"PuLID module {i} works on {dim} channels, the transformer has {transformer.dim}")
        if inner % 128:
            raise ValueError(f"PuLID module {i}: inner width {inner} is no multiple of the head dimension 128")
        mod = PerceiverAttentionCA(dim=dim, dim_head=128, heads=inner // 128, kv_dim=kv_dim, dtype=dtype, device=device)
        mod.load_state_dict(layers[i], strict=True)
        mods.append(mod)
    transformer.pulid_ca = mods
    return mods


def detach_pulid(transformer):
    """Remove the modules.  A captured step has to be captured again."""
    if getattr(transformer, "pulid_ca", None) is not None:
        del transformer.pulid_ca
    return transformer


def pulid_forward(self, hidden_states, id_embeddings=None, id_weight=None, encoder_hidden_states=None, pooled_projections=None,
                  timestep=None, img_ids=None, txt_ids=None, guidance=None, joint_attention_kwargs=None, controlnet_block_samples=None,
                  controlnet_single_block_samples=None, return_dict: bool = True, controlnet_blocks_repeat: bool = False,
                  start_timestep: float | None = None, end_timestep: float | None = None):
    """reference: pulid_forward.py ``pulid_forward`` (bound to the transformer as its ``forward``): the step with ``id_embeddings`` applied
    behind the blocks.  ``start_timestep`` / ``end_timestep`` gate the embeddings by comparing with the timestep ON THE HOST, as the
    reference's ``.item()`` does: that synchronises the stream, so a gate raises while the stream is being captured."""
    if id_embeddings is not None and (start_timestep is not None or end_timestep is not None):
        if timestep.is_cuda and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("pulid_forward: start_timestep / end_timestep read the timestep on the host, which synchronises the stream: "
                               "not possible while the stream is being captured (decide outside and pass id_embeddings or None)")
        t = timestep.flatten()[0].item()
        if (start_timestep is not None and start_timestep > t) or (end_timestep is not None and end_timestep < t):
            id_embeddings = None
    if joint_attention_kwargs:
        raise NotImplementedError("pulid_forward: joint_attention_kwargs are not supported")
    ids = lambda t: t[0] if t is not None and t.ndim == 3 else t
    out = self.engine_forward(hidden_states, encoder_hidden_states, pooled_projections, timestep, ids(img_ids), ids(txt_ids), guidance,
                              controlnet_block_samples, controlnet_single_block_samples, controlnet_blocks_repeat,
                              id_embeddings=id_embeddings, id_weight=1.0 if id_weight is None else id_weight)
    if not return_dict:
        return (out,)
    try:
        from diffusers.models.modeling_outputs import Transformer2DModelOutput
    except ImportError:
        return (out,)
    return Transformer2DModelOutput(sample=out)


def apply_pulid_forward(transformer):
    """Bind :func:`pulid_forward` as ``transformer.forward`` (the reference's ``MethodType(pulid_forward, transformer)``)."""
    transformer.forward = MethodType(pulid_forward, transformer)
    return transformer
