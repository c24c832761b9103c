"""Qwen-Image-Edit's rotary tables without a GPU: ``qwen_rope_freqs_multi`` against ``qwen_rope_freqs`` (one grid) and against a loop written
here from diffusers' rule (several grids), the model's handling of the three spellings of ``img_shapes``, and the validation of
``svdq_qwen_rotary`` (nothing is launched).

Every comparison of table entries is ``torch.equal``: both sides form the same fp32 angle (one product of the same two numbers) and pass it
through ``torch.polar``, which computes an element from that element alone.

The model-level tests run ``NunchakuQwenImageTransformer2DModel.forward`` itself on the CPU -- embedders, ``_prologue``, the block loop,
``_tail`` -- with the quantised blocks (which have no CPU path) replaced by ``_TorchBlock``, a dual-stream attention block in torch ops that
reads the step's tables through the model's own ``_rotate``, with ``fused_norm`` and ``padded_tokens`` off as the torch-op path wants.
``tests/golden/qwen_edit_rotary_single_grid.npz`` holds the output of ``_single_grid_forward`` run with the commit before the several-grid
tables (its ``qwenimage.py``, this file's stand-in block, float32 on one CPU thread)."""

import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

from nunchaku_amd import _lib
from nunchaku_amd.models import qwenimage as Q

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "qwen_edit_rotary_single_grid.npz")
AXES, THETA = (16, 56, 56), 10000.0


# ---- the rule, written out --------------------------------------------------------------------------------------------------------------
def _inv(d):
    return 1.0 / THETA ** (torch.arange(0, d, 2, dtype=torch.float32) / d)


def _entry(pos: int, inv_j: torch.Tensor) -> torch.Tensor:
    return torch.polar(torch.ones(()), torch.tensor(float(pos), dtype=torch.float32) * inv_j)


def _positions(n: int, scale_rope: bool):
    return list(range(-(n - n // 2), 0)) + list(range(0, n // 2)) if scale_rope else list(range(n))


def loop_freqs(grids, txt_len, scale_rope=True):
    """diffusers' rule, positions as Python integers, one polar per entry -> (img [rows, 64], txt [txt_len, 64], the text start)"""
    inv = [_inv(d) for d in AXES]
    rows = []
    for idx, (frame, height, width) in enumerate(grids):
        for f in range(idx, idx + frame):
            for h in _positions(height, scale_rope):
                for w in _positions(width, scale_rope):
                    rows.append(torch.stack([_entry(p, inv[a][j]) for a, p in enumerate((f, h, w)) for j in range(AXES[a] // 2)]))
    start = max(max(h // 2, w // 2) if scale_rope else max(h, w) for _, h, w in grids)
    txt = [torch.stack([_entry(start + t, inv[a][j]) for a in range(3) for j in range(AXES[a] // 2)]) for t in range(txt_len)]
    return torch.stack(rows), (torch.stack(txt) if txt else torch.zeros(0, 64, dtype=torch.complex64)), start


# ---- the tables ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale_rope", [True, False])
@pytest.mark.parametrize("grid", [(1, 4, 6), (1, 5, 3), (2, 3, 3)])
def test_single_grid_equals_qwen_rope_freqs(grid, scale_rope):
    for L in (5, 1):
        img, txt = Q.qwen_rope_freqs_multi([grid], L, scale_rope=scale_rope)
        ref_img, ref_txt = Q.qwen_rope_freqs(grid, L, scale_rope=scale_rope)
        assert img.dtype == torch.complex64 and img.shape == (grid[0] * grid[1] * grid[2], 64) and txt.shape == (L, 64)
        assert torch.equal(img, ref_img) and torch.equal(txt, ref_txt)


@pytest.mark.parametrize("scale_rope", [True, False])
def test_several_grids_follow_the_rule(scale_rope):
    grids, L = [(1, 4, 6), (1, 5, 3), (1, 2, 7)], 5
    img, txt = Q.qwen_rope_freqs_multi(grids, L, scale_rope=scale_rope)
    ref_img, ref_txt, start = loop_freqs(grids, L, scale_rope)
    assert img.shape == (53, 64) and txt.shape == (5, 64) and ref_img.shape == (53, 64)
    assert torch.equal(img, ref_img) and torch.equal(txt, ref_txt)
    # the frame axis (channels 0 .. 7) of a grid's rows holds the grid's number
    inv0 = _inv(16)
    for rows, idx in ((slice(0, 24), 0), (slice(24, 39), 1), (slice(39, 53), 2)):
        want = torch.stack([_entry(idx, inv0[j]) for j in range(8)])
        assert torch.equal(img[rows, :8], want.expand(rows.stop - rows.start, 8)), idx
    assert not torch.equal(img[24, :8], img[0, :8]) and not torch.equal(img[39, :8], img[24, :8])
    # the text starts behind the largest half extent of any grid
    assert start == (max(6 // 2, 5 // 2, 7 // 2) if scale_rope else 7) and max(6 // 2, 5 // 2, 7 // 2) == 3
    assert torch.equal(txt[0], torch.stack([_entry(start, _inv(AXES[a])[j]) for a in range(3) for j in range(AXES[a] // 2)]))


def test_the_text_start_comes_from_the_largest_grid_not_the_first():
    """a table built from the first grid alone starts the text at position 1"""
    grids, L = [(1, 2, 2), (1, 8, 2)], 3
    img, txt = Q.qwen_rope_freqs_multi(grids, L)
    ref_img, ref_txt, start = loop_freqs(grids, L)
    assert start == 4 and img.shape == (20, 64)
    assert torch.equal(img, ref_img) and torch.equal(txt, ref_txt)
    first_alone = Q.qwen_rope_freqs(grids[0], L)[1]
    assert not torch.equal(txt, first_alone)
    assert torch.equal(txt[:, :8], torch.stack([torch.stack([_entry(4 + t, _inv(16)[j]) for j in range(8)]) for t in range(L)]))


def test_axis_tables_hold_both_signs_and_gather_to_the_same_bits():
    """pos_cs[k] = position k, neg_cs[k] = position -(k + 1); a gather from them is bit-equal to the direct computation (the argument the
    kernel's bit-equality rests on, here on the CPU)"""
    pos_cs, neg_cs = Q.qwen_rope_axis_tables(AXES, THETA, "cpu")
    assert pos_cs.shape == neg_cs.shape == (4096, 64, 2) and pos_cs.dtype == torch.float32 and pos_cs.is_contiguous() and neg_cs.is_contiguous()
    inv = torch.cat([_inv(d) for d in AXES])
    for k in (0, 1, 7, 4095):
        for c in (0, 7, 8, 35, 36, 63):
            e = _entry(k, inv[c])
            assert pos_cs[k, c, 0] == e.real and pos_cs[k, c, 1] == e.imag
            e = _entry(-(k + 1), inv[c])
            assert neg_cs[k, c, 0] == e.real and neg_cs[k, c, 1] == e.imag
    assert torch.equal(pos_cs[0], torch.tensor([1.0, 0.0]).expand(64, 2))
    grid = (2, 5, 3)
    img, txt = Q.qwen_rope_freqs(grid, 4)
    hpos, wpos = _positions(5, True), _positions(3, True)
    rows = [(f, h, w) for f in range(2) for h in hpos for w in wpos]
    look = lambda p, c: pos_cs[p, c] if p >= 0 else neg_cs[-p - 1, c]
    gathered = torch.stack([torch.stack([look(r[0 if c < 8 else 1 if c < 36 else 2], c) for c in range(64)]) for r in rows])
    assert torch.equal(gathered, torch.view_as_real(img))
    assert torch.equal(torch.stack([pos_cs[2 + t] for t in range(4)]), torch.view_as_real(txt))  # the text starts at max(5 // 2, 3 // 2) = 2


def test_latent_grids_spellings():
    assert Q.latent_grids([(1, 4, 6)], 24) == [(1, 4, 6)]
    assert Q.latent_grids([[(1, 4, 6)]], 24) == [(1, 4, 6)]
    assert Q.latent_grids([[[1, 4, 6], [1, 5, 3]]], 39) == [(1, 4, 6), (1, 5, 3)]
    assert Q.latent_grids(None, 16) == [(1, 4, 4)]
    assert Q.latent_grids([(1, 4, 6)], 99) == [(1, 4, 6)]  # one grid: nothing is checked that was not checked before
    with pytest.raises(ValueError, match=r"39 image tokens.*has 38"):
        Q.latent_grids([[(1, 4, 6), (1, 5, 3)]], 38)


# ---- the model --------------------------------------------------------------------------------------------------------------------------
CFG = dict(num_layers=1, num_attention_heads=2, attention_head_dim=128, in_channels=64, out_channels=16, joint_attention_dim=128, patch_size=2,
           axes_dims_rope=[16, 56, 56])


class _TorchBlock(nn.Module):
    """joint attention over [text; image] in torch ops, with the step's tables applied by the model's ``_rotate``; records the tables it was given"""

    def __init__(self, dim, heads):
        super().__init__()
        self.heads, self.seen = heads, []
        self.attn = nn.Module()
        self.attn.head_dim = dim // heads
        self.img_qkv, self.txt_qkv = nn.Linear(dim, 3 * dim), nn.Linear(dim, 3 * dim)

    def forward(self, hidden_states, encoder_hidden_states, encoder_hidden_states_mask=None, temb=None, image_rotary_emb=None,
                joint_attention_kwargs=None, kv_valid=None):
        assert kv_valid is None
        self.seen.append(image_rotary_emb)
        shp = (hidden_states.shape[0], -1, self.heads, self.attn.head_dim)
        t_txt = encoder_hidden_states.shape[1]

        def stream(x, lin, cs):
            q, k, v = (t.view(shp) for t in lin(F.layer_norm(x, x.shape[-1:])).chunk(3, dim=-1))
            return Q._rotate(q, cs), Q._rotate(k, cs), v

        t = stream(encoder_hidden_states, self.txt_qkv, image_rotary_emb["txt_cs"])
        i = stream(hidden_states, self.img_qkv, image_rotary_emb["img_cs"])
        q, k, v = (torch.cat(p, dim=1).transpose(1, 2) for p in zip(t, i))
        o = F.scaled_dot_product_attention(q, k, v).transpose(1, 2).flatten(2, 3)
        return encoder_hidden_states + o[:, :t_txt], hidden_states + o[:, t_txt:]


def _model():
    torch.manual_seed(7)
    model = Q.NunchakuQwenImageTransformer2DModel(**CFG, torch_dtype=torch.float32, device="cpu")
    model.transformer_blocks = nn.ModuleList([_TorchBlock(256, 2)])
    torch.manual_seed(7)
    with torch.no_grad():
        for name, p in model.named_parameters():
            p.copy_(torch.randn(p.shape) * (0.3 if p.dim() > 1 else 0.1) + (1.0 if name == "txt_norm.weight" else 0.0))
    model.fused_norm, model.padded_tokens = False, False  # the torch-op path, unpadded: the blocks have no CPU kernels to pad for
    return model.eval()


def _inputs(t_img, t_txt=5, seed=3):
    g = torch.Generator().manual_seed(seed)
    return dict(hidden_states=torch.randn(1, t_img, 64, generator=g), encoder_hidden_states=torch.randn(1, t_txt, 128, generator=g),
                timestep=torch.tensor([0.6]))


def _single_grid_forward(model=None):
    """the seeded single-grid step whose output the golden file holds"""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)  # (the file was recorded on one thread: no dependence on how a reduction is split)
    try:
        model = model or _model()
        with torch.no_grad():
            return model(**_inputs(12), img_shapes=[(1, 4, 3)], return_dict=False)[0]
    finally:
        torch.set_num_threads(threads)


def _forward_with_tables(model, monkeypatch, inputs, grids, t_txt):
    """the same forward with the tables of this file's loop patched in for whatever the model builds"""
    img, txt, _ = loop_freqs(grids, t_txt)
    tables = Q.pack_qwen_rotary(img, txt)
    monkeypatch.setattr(Q, "pack_qwen_rotary", lambda *a, **k: tables)
    model.__dict__.pop("_rot_cache", None)
    with torch.no_grad():
        out = model(**inputs, img_shapes=[grids], return_dict=False)[0]
    monkeypatch.undo()
    model.__dict__.pop("_rot_cache", None)
    return out, tables


def test_model_forward_with_two_grids(monkeypatch):
    model, inputs, grids = _model(), _inputs(12), [(1, 2, 3), (1, 3, 2)]
    with torch.no_grad():
        out = model(**inputs, img_shapes=[grids], return_dict=False)[0]
    assert out.shape == (1, 12, 64) and torch.isfinite(out).all()
    seen = model.transformer_blocks[0].seen[-1]
    want, tables = _forward_with_tables(model, monkeypatch, inputs, grids, 5)
    assert torch.equal(out, want)
    assert sorted(seen) == sorted(tables) and all(torch.equal(seen[k], tables[k]) for k in tables)
    assert seen["img_cs"].shape == (12, 64, 2) and seen["all"].shape == (1, 512, 128)
    # the tables matter: those of the first grid alone, stretched over the stream, give another output
    other, _ = _forward_with_tables(model, monkeypatch, inputs, [(1, 2, 3), (1, 2, 3)], 5)
    assert not torch.equal(out, other)
    # list spellings of the same grids are the same step
    with torch.no_grad():
        assert torch.equal(model(**inputs, img_shapes=[[list(g) for g in grids]], return_dict=False)[0], out)


def test_model_refuses_grids_that_do_not_fit_the_stream():
    model = _model()
    called = []
    model.img_in.register_forward_hook(lambda *a: called.append(1))
    with pytest.raises(ValueError, match=r"12 image tokens.*has 11"):
        model(**_inputs(11), img_shapes=[[(1, 2, 3), (1, 3, 2)]])
    assert not called  # refused before the first embedder runs


def test_single_grid_forward_is_what_it_was():
    out = _single_grid_forward()
    want = torch.from_numpy(np.load(GOLDEN)["out"])
    assert out.shape == want.shape == (1, 12, 64) and torch.equal(out, want)
    model = _model()
    with torch.no_grad():  # the nested spelling of one grid is the same step
        assert torch.equal(model(**_inputs(12), img_shapes=[[(1, 4, 3)]], return_dict=False)[0], _single_grid_forward(model))


def test_axis_tables_are_not_in_the_state_dict():
    model = _model()
    before = set(model.state_dict())
    a = model._rope_axis_tables("cpu")
    assert model._rope_axis_tables("cpu") is a and a[0].shape == (4096, 64, 2)
    assert set(model.state_dict()) == before and not any("rope" in k for k in before)
    assert not any(b is a[0] or b is a[1] for b in model.buffers())


# ---- svdq_qwen_rotary: validation (no launch) -------------------------------------------------------------------------------------------------
P = 1 << 20  # made-up, aligned addresses: validation looks at NULL and alignment, never at what a pointer points to


def _args(grids=((1, 4, 6),), txt_len=5, txt_start=3, scale_rope=1, **kw):
    a = _lib.QwenRotaryArgs()
    a.pos_cs, a.neg_cs, a.img, a.txt, a.all, a.img_cs, a.txt_cs = P, 2 * P, 3 * P, 4 * P, 5 * P, 6 * P, 7 * P
    for k, v in enumerate(v for g in grids[:8] for v in g):
        a.grids[k] = v
    a.count, a.txt_len, a.txt_start, a.scale_rope, a.c_frame, a.c_height = len(grids), txt_len, txt_start, scale_rope, 8, 28
    for k, v in kw.items():
        setattr(a, k, v)
    return a


REFUSED = [
    (dict(grids=((1, 1, 1),) * 9), b"count=9"),
    (dict(grids=()), b"count=0"),
    (dict(grids=((1, 0, 6),)), b"every extent must be >= 1"),
    (dict(grids=((1, 4, 6), (0, 2, 2))), b"grid 1"),
    (dict(grids=((1, 4, -6),)), b"every extent must be >= 1"),
    (dict(grids=((1, 4097, 6),), scale_rope=0), b"at or beyond 4096"),       # height position 4096
    (dict(grids=((1, 4, 8193),)), b"at or beyond 4096"),                     # width position -4097
    (dict(grids=((4097, 1, 1),)), b"at or beyond 4096"),                     # frame position 4096
    (dict(grids=((1, 2, 2), (4096, 1, 1))), b"at or beyond 4096"),           # grid 1's last frame: 1 + 4095
    (dict(txt_len=5, txt_start=4092), b"txt_start"),                         # text position 4096
    (dict(txt_len=-1), b"txt_len"),
    (dict(pos_cs=None), b"pos_cs and neg_cs are required"),
    (dict(neg_cs=None), b"pos_cs and neg_cs are required"),
    (dict(pos_cs=None, neg_cs=None), b"pos_cs and neg_cs are required"),
    (dict(img=None, txt=None, all=None, img_cs=None, txt_cs=None), b"is required"),
    (dict(all=5 * P + 8), b"16-byte aligned"),
    (dict(neg_cs=2 * P + 4), b"16-byte aligned"),
    (dict(c_frame=40, c_height=28), b"c_frame"),
    (dict(grids=((4096, 4096, 4),)), b"addressed in 32 bits"),               # 2^26 rows
]


def test_header_binding_and_sources_agree():
    import re

    from nunchaku_amd import build as svdq_build, ops
    from nunchaku_amd._C import ops as c_ops

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "svdq_amd.h")).read()
    assert "int svdq_qwen_rotary(const svdq_qwen_rotary_args *args, void *stream);" in text
    assert re.search(r"^#define SVDQ_ABI_VERSION 24$", text, re.M) and _lib.ABI_VERSION == 24
    assert _lib.EXPORTS.get("svdq_qwen_rotary") == (C.c_int, [C.POINTER(_lib.QwenRotaryArgs), C.c_void_p])
    assert "qwen_rotary.hip" in svdq_build.SOURCES and os.path.exists(os.path.join(svdq_build.CSRC, "qwen_rotary.hip"))
    assert callable(ops.qwen_rotary) and callable(c_ops.qwen_rotary)
    for macro, value in (("SVDQ_QWEN_ROTARY_MAX_GRIDS", _lib.QWEN_ROTARY_MAX_GRIDS), ("SVDQ_QWEN_ROTARY_POSITIONS", _lib.QWEN_ROTARY_POSITIONS)):
        assert re.search(rf"^#define {macro} {value}$", text, re.M), macro


def test_struct_layout_matches_the_header(tmp_path):
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{os.path.join(root, "include", "svdq_amd.h")}"', "int main(void) {",
             'printf("size %zu\\n", sizeof(svdq_qwen_rotary_args));']
    lines += [f'printf("{f} %zu\\n", offsetof(svdq_qwen_rotary_args, {f}));' for f, _ in _lib.QwenRotaryArgs._fields_]
    lines.append("return 0; }")
    (tmp_path / "layout.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c99", "-o", str(tmp_path / "layout"), str(tmp_path / "layout.c")], check=True)
    got = dict(l.split() for l in subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(_lib.QwenRotaryArgs)
    assert [f for f, _ in _lib.QwenRotaryArgs._fields_] == [k for k in got if k != "size"]
    for f, _ in _lib.QwenRotaryArgs._fields_:
        assert int(got[f]) == getattr(_lib.QwenRotaryArgs, f).offset, f


def test_validation_refuses_before_any_launch(built_lib):
    """every refusal is the library's validation error (SVDQ_E_INVALID = 1) with a message that names the entry point; the pointers are made
    up, so a launch would not come back with a code"""
    lib = _lib.load()
    assert lib.svdq_qwen_rotary(None, None) == 1 and b"NULL" in lib.svdq_last_error()
    for changes, text in REFUSED:
        rc = lib.svdq_qwen_rotary(C.byref(_args(**changes)), None)
        msg = lib.svdq_last_error()
        assert rc == 1 and text in msg and b"svdq_qwen_rotary" in msg, (changes, rc, msg)


def test_wrapper_checks_shapes_and_hands_refusals_on(built_lib, monkeypatch):
    """the Python wrapper: wrong table shapes are refused before the library is called; what the library refuses arrives as ValueError"""
    from nunchaku_amd import _C, ops

    monkeypatch.setattr(_C, "_stream", lambda: 0)
    monkeypatch.setattr(_C, "_ptr", lambda t, laid_out=False: None if t is None else P)
    tab = torch.zeros(4096, 64, 2)
    with pytest.raises(ValueError, match="count=9"):
        ops.qwen_rotary(tab, tab, [(1, 1, 1)] * 9, 4)
    with pytest.raises(ValueError, match="every extent must be >= 1"):
        ops.qwen_rotary(tab, tab, [(1, 0, 3)], 4)
    with pytest.raises(ValueError, match="at or beyond 4096"):
        ops.qwen_rotary(tab, tab, [(1, 4097, 3)], 4, scale_rope=False, txt_start=0)
    with pytest.raises(ValueError, match=r"pos_cs must be a contiguous float32 \[4096, 64, 2\]"):
        ops.qwen_rotary(tab[:100], tab, [(1, 2, 3)], 4)
    with pytest.raises(ValueError, match=r"img_cs must be a contiguous float32 \[6, 64, 2\]"):
        ops.qwen_rotary(tab, tab, [(1, 2, 3)], 4, out={"img_cs": torch.zeros(7, 64, 2)})
    with pytest.raises(ValueError, match="tables="):
        ops.qwen_rotary(tab, tab, [(1, 2, 3)], 4, tables=("image",))
