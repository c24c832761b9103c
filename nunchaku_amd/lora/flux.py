"""diffusers / PEFT LoRA state dicts for the FLUX engine (reference role: nunchaku/lora/flux/{diffusers_converter,nunchaku_converter,
compose}.py behind ``update_lora_params(path_or_state_dict)``, transformer_flux.py:783-831).

Everything here is index work on the LOGICAL factors -- ``A = lora_A.weight [r, in]``, ``B = lora_B.weight [out, r]``,
``delta W = (alpha / r) * B @ A`` -- and runs on the CPU; the kernel layouts are the layers' business (``set_lora``).  Only the
diffusers / PEFT key format is read: ``[transformer.]<diffusers module>.lora_A.weight`` / ``.lora_B.weight``, optionally ``.alpha`` (a
scalar, folded into ``B`` as ``alpha / r``), and 1-D bias deltas ``.diff_b`` / ``.lora_B.bias`` / ``.bias``.

The FLUX engine keeps diffusers' module names except where it fuses projections:

* ``attn.to_q | to_k | to_v`` -> ``attn.to_qkv`` and ``attn.add_q_proj | add_k_proj | add_v_proj`` -> ``attn.add_qkv_proj``:
  ``down = cat(A_q, A_k, A_v)`` ``[3r, in]``, ``up`` block-diagonal ``[3 dim, 3r]`` (a missing member: zero blocks);
* a single block's ``proj_mlp`` -> ``mlp_fc1`` and ``proj_out`` (input ``[attention | mlp]``) -> ``attn.to_out`` with ``(A[:, :dim], B)`` and
  ``mlp_fc2`` with ``(A[:, dim:], B)``: the engine adds the two projections' outputs;
* everything else (``attn.to_out.0``, ``ff.net.0.proj``, ``norm1.linear``, ``x_embedder`` ...) under its own name.

The target names are read off the model (``named_modules``), not from a table.  The modulation layers' ``up`` keeps the checkpoint's
(interleaved) row order: the de-interleaving is the GEMV's ``out_chunks``.
"""

from __future__ import annotations

import os
import re

import torch
from torch import nn

from ..models.linear import AWQW4A16Linear, SVDQW4A4Linear

# the largest total rank (checkpoint rank + attached ranks, padded to 16) of an SVDQW4A4Linear this converter hands out: the W4A4 path (quantiser
# with the low-rank down projection, the GEMM epilogues, the attention-side quantiser) is verified against the oracle up to 176
# (tests/test_gpu_parity.py); the C ABI accepts up to 256 but nothing beyond 176 is tested, so nothing beyond it is served here.
W4A4_TOTAL_RANK_MAX = 176

_SUFFIXES = (".lora_A.weight", ".lora_B.weight", ".alpha", ".diff_b", ".lora_B.bias", ".bias")


def _pad16(r: int) -> int:
    return (r + 15) // 16 * 16


def is_nunchaku_format(state_dict) -> bool:
    """Keys of a LoRA already converted for the reference engine (packed ``lora_down`` / ``lora_up``, or a checkpoint's ``qweight``)."""
    return any(k.endswith((".lora_down", ".lora_up", ".qweight")) or ".lora_down." in k or ".lora_up." in k for k in state_dict)


def is_peft_format(state_dict) -> bool:
    return any(isinstance(k, str) and (".lora_A." in k or ".lora_B." in k) for k in state_dict)


def load_state_dict(path_or_dict) -> dict:
    """A ``.safetensors`` file (``str`` / ``os.PathLike``) or a dict of tensors -> dict of CPU tensors."""
    if isinstance(path_or_dict, (str, os.PathLike)):
        from safetensors.torch import load_file

        return load_file(os.fspath(path_or_dict), device="cpu")
    return dict(path_or_dict)


def _parse(state_dict) -> dict:
    """``{diffusers module: {"A": ..., "B": ..., "alpha": ..., "bias": ...}}``; B carries alpha / r.  Unknown keys: KeyError."""
    if is_nunchaku_format(state_dict):
        raise NotImplementedError("this is a nunchaku-format LoRA (lora_down / lora_up / qweight keys): only the diffusers / PEFT format "
                                  "(<module>.lora_A.weight / <module>.lora_B.weight [/ <module>.alpha]) is supported")
    mods: dict = {}
    unknown = []
    for key, t in state_dict.items():
        k = key[len("transformer."):] if key.startswith("transformer.") else key
        for suf in _SUFFIXES:
            if k.endswith(suf):
                field = {".lora_A.weight": "A", ".lora_B.weight": "B", ".alpha": "alpha"}.get(suf, "bias")
                if (field in ("A", "B") and t.dim() != 2) or (field == "bias" and t.dim() != 1) or (field == "alpha" and t.numel() != 1):
                    unknown.append(key)
                else:
                    mods.setdefault(k[: -len(suf)], {})[field] = t
                break
        else:
            unknown.append(key)
    if unknown:
        raise KeyError(f"LoRA keys that are not diffusers / PEFT LoRA entries: {sorted(unknown)}")
    for name, m in mods.items():
        if ("A" in m) != ("B" in m):
            raise KeyError(f"LoRA module {name}: lora_A.weight and lora_B.weight must come together")
        if "A" in m:
            r = m["A"].shape[0]
            if m["B"].shape[1] != r:
                raise ValueError(f"LoRA module {name}: lora_A {tuple(m['A'].shape)} and lora_B {tuple(m['B'].shape)} disagree on the rank")
            if "alpha" in m:
                m["B"] = m["B"] * (float(m["alpha"]) / r)
        elif "alpha" in m:
            raise KeyError(f"LoRA module {name}: alpha without factors")
    return mods


def _fuse(members, outs):
    """``members``: the parsed entries of the projections a fused layer concatenates along its output (``None``: missing), ``outs`` their output
    widths -> (down [sum r, in], up block-diagonal [sum outs, sum r], bias delta [sum outs]); each ``None`` when no member brings it."""
    members = [m or {} for m in members]
    down = up = bias = None
    with_factors = [m for m in members if "A" in m]
    if with_factors:
        ranks = [m["A"].shape[0] if "A" in m else 0 for m in members]
        down = torch.cat([m["A"] for m in with_factors], dim=0)
        up = torch.zeros(sum(outs), sum(ranks), dtype=with_factors[0]["B"].dtype)
        r0 = o0 = 0
        for m, r, o in zip(members, ranks, outs):
            if r:
                up[o0:o0 + o, r0:r0 + r] = m["B"]
            r0, o0 = r0 + r, o0 + o
    with_bias = [m["bias"] for m in members if "bias" in m]
    if with_bias:
        bias = torch.cat([m["bias"] if "bias" in m else torch.zeros(o, dtype=with_bias[0].dtype) for m, o in zip(members, outs)])
    return down, up, bias


def to_engine_lora(state_dict, model) -> dict:
    """diffusers / PEFT LoRA ``state_dict`` -> ``{engine module name: (down [r, in], up [out, r])}`` for ``model``
    (a ``FluxEngineMixin``), in logical layout and the source's dtype; a bias delta comes as ``{"<module name>.bias": delta [out]}``.
    Targets: ``SVDQW4A4Linear`` / ``AWQW4A16Linear`` (attached with ``set_lora``) and ``nn.Linear`` (merged)."""
    mods = _parse(state_dict)
    names = {id(m): n for n, m in model.named_modules()}
    by_name = dict(model.named_modules())
    out: dict = {}
    used = set()

    def put(layer, down, up, bias, what):
        name = names[id(layer)]
        if down is not None:
            if down.shape[1] < layer.in_features and isinstance(layer, nn.Linear):  # the reference zero-pads (x_embedder of a narrower base model)
                down = torch.cat([down, torch.zeros(down.shape[0], layer.in_features - down.shape[1], dtype=down.dtype)], dim=1)
            if down.shape[1] != layer.in_features or up.shape[0] != layer.out_features:
                raise ValueError(f"LoRA for {what}: factors {tuple(up.shape)} x {tuple(down.shape)} do not fit {name} "
                                 f"({layer.out_features} x {layer.in_features})")
            if isinstance(layer, SVDQW4A4Linear):
                base = layer._base_lowrank[2] if layer._base_lowrank is not None else layer.rank
                if base + _pad16(down.shape[0]) > W4A4_TOTAL_RANK_MAX:
                    raise ValueError(f"LoRA for {what}: {name} would run at total rank {base} + {_pad16(down.shape[0])} = {base + _pad16(down.shape[0])}; "
                                     f"the W4A4 path serves at most {W4A4_TOTAL_RANK_MAX}")
            elif isinstance(layer, AWQW4A16Linear) and _pad16(down.shape[0]) > AWQW4A16Linear.LORA_RANK_MAX:
                raise ValueError(f"LoRA for {what}: rank {down.shape[0]} exceeds the {AWQW4A16Linear.LORA_RANK_MAX} ranks of {name}'s low-rank branch")
            out[name] = (down, up)
        if bias is not None:
            if layer.bias is None or bias.numel() != layer.out_features:
                raise ValueError(f"LoRA for {what}: a bias delta of {bias.numel()} elements does not fit {name}")
            out[name + ".bias"] = bias

    def take(src):
        m = mods.get(src)
        if m is not None:
            used.add(src)
        return m

    def direct(src, layer):
        m = take(src)
        if m is not None:
            put(layer, m.get("A"), m.get("B"), m.get("bias"), src)

    def fused(prefix, parts, layer):
        members = [take(f"{prefix}.{p}") for p in parts]
        if any(m is not None for m in members):
            o = layer.out_features // len(parts)
            put(layer, *_fuse(members, [o] * len(parts)), f"{prefix}.{{{'|'.join(parts)}}}")

    for i, b in enumerate(getattr(model, "transformer_blocks", [])):
        p = f"transformer_blocks.{i}"
        fused(f"{p}.attn", ("to_q", "to_k", "to_v"), b.attn.to_qkv)
        fused(f"{p}.attn", ("add_q_proj", "add_k_proj", "add_v_proj"), b.attn.add_qkv_proj)
        for src, layer in ((f"{p}.attn.to_out.0", b.attn.out_proj), (f"{p}.attn.to_add_out", b.attn.to_add_out),
                           (f"{p}.ff.net.0.proj", b.ff.fc1), (f"{p}.ff.net.2", b.ff.fc2),
                           (f"{p}.ff_context.net.0.proj", b.ff_context.fc1), (f"{p}.ff_context.net.2", b.ff_context.fc2),
                           (f"{p}.norm1.linear", b.mod), (f"{p}.norm1_context.linear", b.mod_context)):
            direct(src, layer)
    for i, b in enumerate(getattr(model, "single_transformer_blocks", [])):
        p = f"single_transformer_blocks.{i}"
        fused(f"{p}.attn", ("to_q", "to_k", "to_v"), b.attn.to_qkv)
        direct(f"{p}.proj_mlp", b.mlp_fc1)
        direct(f"{p}.norm.linear", b.mod)
        m = take(f"{p}.proj_out")
        if m is not None:  # input [attention (dim) | mlp (4 dim)]: the engine's two projections, whose outputs it adds
            dim = b.attn.out_proj.in_features
            if "A" in m:
                if m["A"].shape[1] != dim + b.mlp_fc2.in_features:
                    raise ValueError(f"LoRA for {p}.proj_out: lora_A must be [r, {dim + b.mlp_fc2.in_features}]")
                put(b.attn.out_proj, m["A"][:, :dim], m["B"], m.get("bias"), f"{p}.proj_out")  # (the bias delta is added once: here)
                put(b.mlp_fc2, m["A"][:, dim:], m["B"], None, f"{p}.proj_out")
            else:
                put(b.attn.out_proj, None, None, m.get("bias"), f"{p}.proj_out")
    for src in list(mods):
        if src not in used and isinstance(by_name.get(src), nn.Linear) and not re.match(r"(single_)?transformer_blocks\.", src):
            direct(src, by_name[src])  # the unquantised layers keep diffusers' names
    left = sorted(set(mods) - used)
    if left:
        raise KeyError(f"LoRA modules with no counterpart in this model: {left}")
    return out


def compose_lora(loras) -> dict:
    """``[(path_or_state_dict, strength), ...]`` -> one diffusers / PEFT state dict whose delta W is ``sum_i strength_i * delta W_i``
    (reference: lora/flux/compose.py): per module, ``lora_A`` concatenated along the rank axis and ``lora_B`` along its rank axis with
    ``strength_i * alpha_i / r_i`` folded in (no ``alpha`` key is written); bias deltas are summed with their strengths."""
    acc: dict = {}
    for src, strength in loras:
        for name, m in _parse(load_state_dict(src)).items():
            a = acc.setdefault(name, {"A": [], "B": [], "bias": None})
            if "A" in m:
                a["A"].append(m["A"])
                a["B"].append(m["B"] * float(strength))
            if "bias" in m:
                a["bias"] = m["bias"] * float(strength) if a["bias"] is None else a["bias"] + m["bias"] * float(strength)
    out = {}
    for name, a in acc.items():
        if a["A"]:
            if len({t.shape[1] for t in a["A"]}) > 1:  # (a narrower x_embedder next to a wider one: zero-padded, as on the engine side)
                w = max(t.shape[1] for t in a["A"])
                a["A"] = [torch.cat([t, torch.zeros(t.shape[0], w - t.shape[1], dtype=t.dtype)], dim=1) for t in a["A"]]
            out[f"{name}.lora_A.weight"] = torch.cat(a["A"], dim=0)
            out[f"{name}.lora_B.weight"] = torch.cat([b.to(a["B"][0].dtype) for b in a["B"]], dim=1)
        if a["bias"] is not None:
            out[f"{name}.diff_b"] = a["bias"]
    return out
