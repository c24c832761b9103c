"""SANA's cross-attention, the parts that need no GPU: the C ABI (header, bindings, exported symbol, validation without a launch), the CPU
restatement the GPU tests compare against (tests/xattn_ref.py), the op wrapper's checks and the module's names and shapes."""

import ctypes as C
import json
import os
import re
import subprocess

import pytest
import torch

from nunchaku_amd import _lib
from nunchaku_amd import build as svdq_build
from tests.xattn_ref import clamp_ranges, xattn_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_KEYS = 320


# ---- C ABI --------------------------------------------------------------------------------------------------------------------------
def test_header_bindings_and_sources_agree_and_the_abi_version_stays():
    text = open(os.path.join(ROOT, "include", "svdq_amd.h")).read()
    assert re.search(r"^int svdq_cross_attention\(const svdq_cross_attention_args \*args, void \*stream\);", text, re.M)
    assert re.search(r"^} svdq_cross_attention_args;", text, re.M)
    assert re.search(r"^#define SVDQ_ABI_VERSION 24$", text, re.M)
    assert _lib.ABI_VERSION == 24
    assert _lib.EXPORTS.get("svdq_cross_attention") == (C.c_int, [C.POINTER(_lib.CrossAttentionArgs), C.c_void_p])
    assert "cross_attention.hip" in svdq_build.SOURCES and os.path.exists(os.path.join(svdq_build.CSRC, "cross_attention.hip"))
    from nunchaku_amd.ops.attention import CROSS_ATTENTION_MAX_KEYS

    src = open(os.path.join(svdq_build.CSRC, "cross_attention.hip")).read()
    assert CROSS_ATTENTION_MAX_KEYS == MAX_KEYS and re.search(rf"constexpr int XA_MAX_KEYS = {MAX_KEYS};", src)


def test_struct_layout_matches_header(built_lib, tmp_path):
    cname, cls = "svdq_cross_attention_args", _lib.CrossAttentionArgs
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{os.path.join(ROOT, "include", "svdq_amd.h")}"', "int main(void) {",
             f'printf("{cname} %zu\\n", sizeof({cname}));']
    lines += [f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));' for f, _ in cls._fields_]
    lines.append("return 0; }")
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(src)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got[cname]) == C.sizeof(cls)
    for f, _ in cls._fields_:
        assert int(got[f"{cname}.{f}"]) == getattr(cls, f).offset, f"offsetof({cname}, {f})"


B, T, H, D = 2, 40, 3, 112
HD = H * D


def _args(**over):
    """a call that would pass validation (the pointers are made up: no test below lets it reach a launch)"""
    a = _lib.CrossAttentionArgs()
    a.q, a.k, a.v, a.out = 0x100000, 0x200000, 0x200000 + 2 * HD, 0x300000
    a.key_offsets, a.key_counts = 0x400000, 0x400100
    a.ldq, a.ldk, a.ldv, a.ldo = 384, 2 * HD, 2 * HD, 384
    a.B, a.T, a.H, a.head_dim, a.Nrows, a.max_keys = B, T, H, D, 600, 300
    a.dtype, a.scale = _lib.SVDQ_BF16, D ** -0.5
    for k, v in over.items():
        setattr(a, k, v)
    return a


INVALID, UNSUPPORTED = 1, 2
REFUSED = [
    (dict(q=None), INVALID, b"are required"),
    (dict(k=None), INVALID, b"are required"),
    (dict(v=None), INVALID, b"are required"),
    (dict(out=None), INVALID, b"are required"),
    (dict(key_offsets=None), INVALID, b"are required"),
    (dict(key_counts=None), INVALID, b"are required"),
    (dict(B=0), INVALID, b"B=0"),
    (dict(T=0), INVALID, b"T=0"),
    (dict(H=-1), INVALID, b"H=-1"),
    (dict(max_keys=-1), INVALID, b"max_keys=-1"),
    (dict(Nrows=-1), INVALID, b"Nrows=-1"),
    (dict(ldq=HD - 8), INVALID, b"row strides"),
    (dict(ldk=HD - 8), INVALID, b"row strides"),
    (dict(ldv=HD - 8), INVALID, b"row strides"),
    (dict(ldo=HD - 8), INVALID, b"row strides"),
    (dict(q=0x100000 + 8), INVALID, b"16-byte aligned"),
    (dict(k=0x200000 + 2), INVALID, b"16-byte aligned"),
    (dict(v=0x200000 + 4), INVALID, b"16-byte aligned"),
    (dict(out=0x300000 + 8), INVALID, b"16-byte aligned"),
    (dict(ldq=HD + 4), INVALID, b"16-byte aligned"),
    (dict(ldk=2 * HD + 2), INVALID, b"16-byte aligned"),
    (dict(ldv=2 * HD + 1), INVALID, b"16-byte aligned"),
    (dict(ldo=HD + 4), INVALID, b"16-byte aligned"),
    (dict(key_offsets=0x400002), INVALID, b"4-byte aligned"),
    (dict(key_counts=0x400101), INVALID, b"4-byte aligned"),
    (dict(dtype=7), INVALID, b"unknown dtype 7"),
    (dict(head_dim=64, ldq=512, ldo=512), UNSUPPORTED, b"head_dim=64"),
    (dict(head_dim=120, ldq=512, ldo=512), UNSUPPORTED, b"head_dim=120"),
    (dict(head_dim=0), UNSUPPORTED, b"head_dim=0"),
    (dict(max_keys=MAX_KEYS + 1), UNSUPPORTED, b"max_keys=321: at most 320"),
    (dict(head_dim=72, max_keys=MAX_KEYS + 1), UNSUPPORTED, b"max_keys=321: at most 320"),
    (dict(head_dim=128, ldq=512, ldo=512, max_keys=MAX_KEYS + 1), UNSUPPORTED, b"max_keys=321: at most 320"),
    (dict(scale=0.0), INVALID, b"scale must be positive and finite"),
    (dict(scale=-0.1), INVALID, b"scale must be positive and finite"),
    (dict(scale=float("inf")), INVALID, b"scale must be positive and finite"),
    (dict(scale=float("nan")), INVALID, b"scale must be positive and finite"),
    (dict(B=21846, H=3), INVALID, b"exceed the grid"),
    (dict(T=(1 << 30) + 1), INVALID, b"exceed the grid"),
]


def test_exported_and_every_validation_error_is_returned_without_a_launch(built_lib):
    raw = C.CDLL(built_lib)
    assert hasattr(raw, "svdq_cross_attention")
    lib = _lib.load()
    assert lib.svdq_abi_version() == 24
    assert lib.svdq_cross_attention(None, None) == 1 and b"NULL" in lib.svdq_last_error()
    for over, want, needle in REFUSED:
        rc = lib.svdq_cross_attention(C.byref(_args(**over)), None)
        msg = lib.svdq_last_error()
        assert rc == want and needle in msg, f"{over}: returned {rc}, {msg!r}"


# ---- the CPU restatement --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("heads,head_dim", [(2, 72), (3, 112), (1, 128)])
def test_restatement_equals_a_dense_masked_softmax_in_float64(heads, head_dim):
    """one dense [B, H, T, Nrows] score matrix with -inf outside the sample's range, float64 softmax: the restatement's per-sample slices in
    fp32 agree to fp32 rounding (a softmax over <= 300 terms and a dot product over them: a few 2^-24 relative to max |v|)"""
    g = torch.Generator().manual_seed(5)
    counts, Bq, Tq = [7, 0, 300, 33], 4, 19
    offs = [0, 7, 7, 307]
    nrows, hd = 345, heads * head_dim  # (five rows in no range)
    q = torch.randn(Bq, Tq, hd + 8, generator=g).bfloat16()
    k, v = torch.randn(nrows, hd, generator=g).bfloat16(), torch.randn(nrows, hd, generator=g).bfloat16()
    ref = xattn_ref(q, k, v, heads, head_dim, offs, counts)
    assert ref.dtype == torch.float32 and tuple(ref.shape) == (Bq, Tq, hd)
    q4 = q[..., :hd].double().view(Bq, Tq, heads, head_dim).transpose(1, 2)
    k3, v3 = k.double().view(nrows, heads, head_dim).transpose(0, 1), v.double().view(nrows, heads, head_dim).transpose(0, 1)
    s = head_dim ** -0.5 * (q4 @ k3.transpose(1, 2))                                       # [B, H, T, Nrows]
    rows = torch.arange(nrows)
    mask = torch.stack([(rows >= o) & (rows < o + n) for o, n in zip(offs, counts)])       # [B, Nrows]
    s = s.masked_fill(~mask[:, None, None, :], float("-inf"))
    p = torch.softmax(s, dim=-1).nan_to_num(0.0)                                           # (an empty range: all -inf -> zeros)
    dense = (p @ v3).transpose(1, 2).reshape(Bq, Tq, hd)
    assert torch.equal(ref[1], torch.zeros_like(ref[1]))
    err = (ref.double() - dense).abs().max().item()
    assert err <= 16 * 2.0 ** -24 * v.double().abs().max().item(), err
    assert xattn_ref(q, k, v, heads, head_dim, offs, counts, dtype=torch.float64).sub(dense).abs().max().item() < 1e-12


def test_clamp_restatement():
    assert clamp_ranges([0, 5, 9, -1, 10, 8], [3, -2, 9, 4, 1, 50], nrows=10, max_keys=6) == [(0, 3), (5, 0), (9, 1), (-1, 0), (10, 0), (8, 2)]


# ---- the op wrapper -------------------------------------------------------------------------------------------------------------------
def test_wrapper_refuses_mismatched_arguments_and_cpu_tensors(built_lib):
    from nunchaku_amd.ops import cross_attention
    from nunchaku_amd.ops.attention import cross_attention as same

    assert cross_attention is same
    q = torch.zeros(2, 10, 256, dtype=torch.bfloat16)          # 2 heads x 112 = 224 columns of 256-wide rows
    kv = torch.zeros(50, 448, dtype=torch.bfloat16)
    k, v = kv[:, :224], kv[:, 224:]
    cu = torch.tensor([0, 20, 50], dtype=torch.int32)
    off, cnt = cu[:-1], cu[1:] - cu[:-1]
    with pytest.raises(ValueError, match="q must be a GPU tensor"):
        cross_attention(q, k, v, 2, 112, cu_seqlens=cu)
    with pytest.raises(ValueError, match="q must be a GPU tensor"):
        cross_attention(q.view(20, 256), k, v, 2, 112, cu_seqlens=cu, out=torch.zeros(20, 224, dtype=torch.bfloat16))
    with pytest.raises(TypeError, match="q must be bfloat16 or float16"):
        cross_attention(q.float(), k, v, 2, 112, cu_seqlens=cu)
    with pytest.raises(TypeError, match="must have q's dtype"):
        cross_attention(q, k.half(), v, 2, 112, cu_seqlens=cu)
    with pytest.raises(TypeError, match="must have q's dtype"):
        cross_attention(q, k, v.half(), 2, 112, cu_seqlens=cu)
    with pytest.raises(TypeError, match="cu_seqlens must be an int32 tensor"):
        cross_attention(q, k, v, 2, 112, cu_seqlens=cu.long())
    with pytest.raises(TypeError, match="key_counts must be an int32 tensor"):
        cross_attention(q, k, v, 2, 112, key_offsets=off, key_counts=cnt.long())
    with pytest.raises(TypeError, match="key_offsets must be an int32 tensor"):
        cross_attention(q, k, v, 2, 112, key_offsets=[0, 20], key_counts=cnt)
    with pytest.raises(ValueError, match="cu_seqlens must live on q's device"):
        cross_attention(q, k, v, 2, 112, cu_seqlens=cu.to("meta"))
    with pytest.raises(ValueError, match="key_counts must live on q's device"):
        cross_attention(q, k, v, 2, 112, key_offsets=off, key_counts=cnt.to("meta"))
    with pytest.raises(ValueError, match="exactly one of the two forms"):
        cross_attention(q, k, v, 2, 112)
    with pytest.raises(ValueError, match="exactly one of the two forms"):
        cross_attention(q, k, v, 2, 112, cu_seqlens=cu, key_offsets=off, key_counts=cnt)
    with pytest.raises(ValueError, match="exactly one of the two forms"):
        cross_attention(q, k, v, 2, 112, cu_seqlens=cu, key_counts=cnt)
    with pytest.raises(ValueError, match="go together"):
        cross_attention(q, k, v, 2, 112, key_offsets=off)
    with pytest.raises(ValueError, match=r"must both be \[B\]"):
        cross_attention(q, k, v, 2, 112, key_offsets=off, key_counts=cnt[:1])
    with pytest.raises(ValueError, match=r"q must be \[B, T"):
        cross_attention(q, k, v, 2, 112, cu_seqlens=cu[:2])                      # B = 1 against a q of two samples
    with pytest.raises(ValueError, match=r"q must be \[B, T"):
        cross_attention(q.view(20, 256), k, v, 2, 112, key_offsets=off, key_counts=cnt)  # a flat q needs cu_seqlens
    with pytest.raises(ValueError, match="at least heads \\* head_dim = 224 columns"):
        cross_attention(q[..., :128], k, v, 2, 112, cu_seqlens=cu)
    with pytest.raises(ValueError, match="k and v must be"):
        cross_attention(q, k, v[:40], 2, 112, cu_seqlens=cu)
    with pytest.raises(ValueError, match="k and v must be"):
        cross_attention(q, kv, kv, 2, 112, cu_seqlens=cu)
    for bad in (torch.zeros(2, 10, 256, dtype=torch.bfloat16), torch.zeros(2, 9, 224, dtype=torch.bfloat16), torch.zeros(2, 10, 224, dtype=torch.float16),
                torch.zeros(2, 10, 224, dtype=torch.bfloat16, device="meta"), torch.zeros(20, 224, dtype=torch.bfloat16)):
        with pytest.raises(ValueError, match="out must be a torch.bfloat16 tensor of shape \\(2, 10, 224\\)"):
            cross_attention(q, k, v, 2, 112, cu_seqlens=cu, out=bad)


# ---- the module -----------------------------------------------------------------------------------------------------------------------
def test_module_names_shapes_and_padding_match_the_reference_layer(golden_dir):
    from nunchaku.models.sana import SanaCrossAttention as Mirrored
    from nunchaku.models.sana import convert_sana_cross_attention_state_dict as mirrored_convert
    from nunchaku_amd.models import SanaCrossAttention, convert_sana_cross_attention_state_dict
    from nunchaku_amd.models.linear import SVDQW4A4Linear

    assert Mirrored is SanaCrossAttention and mirrored_convert is convert_sana_cross_attention_state_dict
    big = SanaCrossAttention(20, 112, device="meta")          # SANA-1.6B: 2240 -> 2304
    assert (big.dim, big.dim_pad) == (2240, 2304)
    assert (big.q_linear.in_features, big.q_linear.out_features, big.out_proj.in_features, big.out_proj.out_features) == (2304,) * 4
    assert tuple(big.kv_linear.weight.shape) == (4480, 2240) and tuple(big.kv_linear.bias.shape) == (4480,)  # (the 16-bit GEMM is not padded)
    m = SanaCrossAttention(16, 72, device="meta")             # SANA-0.6B: 1152 is a multiple of 128
    assert (m.dim, m.dim_pad) == (1152, 1152)
    assert [n for n, _ in m.named_children()] == ["q_linear", "kv_linear", "out_proj"]
    assert isinstance(m.q_linear, SVDQW4A4Linear) and isinstance(m.out_proj, SVDQW4A4Linear) and type(m.kv_linear) is torch.nn.Linear
    assert m.q_linear.bias is not None and m.out_proj.bias is not None and m.kv_linear.weight.dtype == torch.bfloat16
    assert SanaCrossAttention(2, 112, torch_dtype=torch.float16, device="meta").kv_linear.bias.dtype == torch.float16
    with pytest.raises(ValueError, match="head_dim=64"):
        SanaCrossAttention(4, 64, device="meta")
    golden = json.load(open(os.path.join(golden_dir, "sana_cross_attention_keys.json")))
    sd = m.state_dict()
    assert {k: list(v.shape) for k, v in sd.items()} == golden

    legacy = {}
    for k, v in sd.items():
        k = k.replace("proj_down", "lora_down").replace("proj_up", "lora_up").replace("smooth_factor_orig", "smooth_orig").replace("smooth_factor", "smooth")
        legacy[k] = torch.empty(v.shape, dtype=v.dtype)
    assert {"q_linear.lora_down", "out_proj.lora_up", "out_proj.smooth", "q_linear.smooth_orig", "kv_linear.weight", "kv_linear.bias"} <= set(legacy)
    assert not any(s in k for k in legacy for s in ("proj_down", "proj_up", "smooth_factor"))
    conv = convert_sana_cross_attention_state_dict(legacy)
    assert set(conv) == set(sd) and conv["kv_linear.weight"] is legacy["kv_linear.weight"] and conv["kv_linear.bias"] is legacy["kv_linear.bias"]
    assert convert_sana_cross_attention_state_dict(conv).keys() == conv.keys()  # names that are already converted pass through
    cpu = SanaCrossAttention(16, 72)
    cpu.load_state_dict(conv, strict=True)
    with pytest.raises(RuntimeError):
        cpu.load_state_dict(legacy, strict=True)


def test_forward_rejects_shapes_it_cannot_use():
    from nunchaku_amd.models import SanaCrossAttention

    m = SanaCrossAttention(2, 112, device="meta")
    mk = lambda *s, dtype=torch.bfloat16: torch.empty(*s, dtype=dtype, device="meta")
    x, cond, cu = mk(2, 12, 224), mk(50, 224), mk(3, dtype=torch.int32)
    with pytest.raises(ValueError, match="expected x"):
        m(x[..., :128], cond, None, cu)
    with pytest.raises(ValueError, match="expected x"):
        m(x[0], cond, None, cu)
    with pytest.raises(ValueError, match="expected cond"):
        m(x, mk(2, 25, 224), None, cu)
    with pytest.raises(ValueError, match="expected cond"):
        m(x, mk(50, 256), None, cu)
    with pytest.raises(ValueError, match="cu_seqlens_txt must be"):
        m(x, cond, None, cu[:2])
    with pytest.raises(ValueError, match="cu_seqlens_txt must be"):
        m(x, cond, None, None)
    with pytest.raises(ValueError, match="cu_seqlens_img must be"):
        m(x, cond, cu[:2], cu)
    with pytest.raises(ValueError, match="expected x"):
        m.forward_padded(x[..., :128], mk(2, 25, 224), mk(2, dtype=torch.int32))
    with pytest.raises(ValueError, match="expected cond"):
        m.forward_padded(x, cond, mk(2, dtype=torch.int32))
    with pytest.raises(ValueError, match="expected cond"):
        m.forward_padded(x, mk(3, 25, 224), mk(2, dtype=torch.int32))
    with pytest.raises(ValueError, match="L=321 text tokens per sample: at most 320"):
        m.forward_padded(x, mk(2, 321, 224), mk(2, dtype=torch.int32))
    with pytest.raises(ValueError, match="key_counts must be"):
        m.forward_padded(x, mk(2, 25, 224), mk(3, dtype=torch.int32))
