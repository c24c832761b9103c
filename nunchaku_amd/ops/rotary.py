"""Qwen-Image's rotary tables in one launch (``svdq_qwen_rotary``, csrc/qwen_rotary.hip)."""

from __future__ import annotations

import torch

QWEN_ROTARY_TABLES = ("img", "txt", "all", "img_cs", "txt_cs")


def qwen_text_start(grids, scale_rope: bool = True) -> int:
    """Position of the first text token (diffusers ``QwenEmbedRope.forward``): behind the largest half extent of ANY grid when the image
    positions are centred, behind the largest extent otherwise."""
    return max(max(h // 2, w // 2) if scale_rope else max(h, w) for _, h, w in grids)


def qwen_rotary_shapes(grids, txt_len: int) -> dict:
    """shape of every table of :func:`qwen_rotary` (what ``models.qwenimage.pack_qwen_rotary`` returns for these grids)"""
    t_img = sum(f * h * w for f, h, w in grids)
    pad = lambda n: n + -n % 256
    return {"img": (1, pad(t_img), 128), "txt": (1, pad(txt_len), 128), "all": (1, pad(txt_len) + pad(t_img), 128),
            "img_cs": (t_img, 64, 2), "txt_cs": (txt_len, 64, 2)}


def qwen_rotary(pos_cs: torch.Tensor, neg_cs: torch.Tensor, grids, txt_len: int, *, axes_dim=(16, 56, 56), scale_rope: bool = True,
                txt_start: int | None = None, tables=QWEN_ROTARY_TABLES, out: dict | None = None) -> dict:
    """The rotary tables of a Qwen-Image step -- ``grids``: one to eight ``(frames, height, width)`` latent grids whose tokens follow each
    other in the image stream (the noise latents, then the reference images of an Edit pipeline); ``txt_len`` text tokens -- gathered in ONE
    launch from the axis tables ``pos_cs`` / ``neg_cs`` (``models.qwenimage.qwen_rope_axis_tables``: float32 ``[4096, 64, 2]`` (cos, sin) of
    positions ``0 .. 4095`` and ``-1 .. -4096``, row ``k`` of ``neg_cs`` holding position ``-(k + 1)``).

    -> ``{name: tensor}`` for every name in ``tables``, with the shapes, the order and -- on the same device -- the bits of
    ``pack_qwen_rotary(*qwen_rope_freqs_multi(grids, txt_len, ...))``: ``"img"`` / ``"txt"`` / ``"all"`` packed (sin, cos) for the fused QKV
    epilogue (256-row padding per stream, zeros in the padding rows), ``"img_cs"`` / ``"txt_cs"`` plain (cos, sin).  ``out``: tensors to write
    into, by name (uninitialised memory will do: every byte is written); the others are allocated.  ``txt_start``: the first text position
    (default: diffusers' rule, :func:`qwen_text_start`).  Safe under stream capture (one kernel node, no host synchronisation)."""
    from .._C import ops

    grids = [tuple(int(v) for v in g) for g in grids]
    axes_dim = tuple(int(d) for d in axes_dim)
    if len(axes_dim) != 3 or any(d < 0 or d % 2 for d in axes_dim) or sum(axes_dim) != 128:
        raise ValueError(f"qwen_rotary: axes_dim={axes_dim} must be three even numbers that add up to the head dimension 128")
    unknown = [n for n in tables if n not in QWEN_ROTARY_TABLES]
    if unknown or not tables:
        raise ValueError(f"qwen_rotary: tables={tuple(tables)} must name some of {QWEN_ROTARY_TABLES}")
    if not grids or any(len(g) != 3 for g in grids):
        raise ValueError(f"qwen_rotary: grids must be a list of (frames, height, width), got {grids}")
    if txt_start is None:
        txt_start = qwen_text_start(grids, scale_rope)
    given = dict(out or {})
    if len(grids) <= 8 and all(min(g) >= 1 for g in grids) and txt_len >= 0:  # (what is not: refused by the library, nothing to allocate for)
        shapes = qwen_rotary_shapes(grids, int(txt_len))
        for name in tables:
            if given.get(name) is None:
                given[name] = torch.empty(shapes[name], dtype=torch.float32, device=pos_cs.device)
    # (the packed tables carry pack_rotemb's leading batch axis of 1; the library takes the [rows, 128] view)
    arg = {n: None if n not in tables or given.get(n) is None else given[n].squeeze(0) if n in ("img", "txt", "all") and given[n].dim() == 3
           else given[n] for n in QWEN_ROTARY_TABLES}
    ops.qwen_rotary(pos_cs, neg_cs, grids, int(txt_len), int(txt_start), bool(scale_rope), axes_dim[0] // 2, axes_dim[1] // 2,
                    arg["img"], arg["txt"], arg["all"], arg["img_cs"], arg["txt_cs"])
    return {n: given[n] for n in tables}
