"""SANA's ReLU linear attention, the parts that need no GPU: the C ABI (header, bindings, exported symbols, validation without a launch),
the CPU restatements the GPU tests compare against (tests/litela_ref.py), and the module's parameter names and shapes."""

import ctypes as C
import json
import os
import re
import subprocess

import pytest
import torch

from nunchaku_amd import _lib
from nunchaku_amd import build as svdq_build
from tests.litela_ref import litela_ones_row, litela_ref32, litela_ref64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- C ABI --------------------------------------------------------------------------------------------------------------------------
def test_header_bindings_and_sources_agree_and_the_abi_version_stays():
    text = open(os.path.join(ROOT, "include", "svdq_amd.h")).read()
    assert re.search(r"^int svdq_linear_attention\(const svdq_linear_attention_args \*args, void \*stream\);", text, re.M)
    assert re.search(r"^int64_t svdq_linear_attention_workspace_bytes\(const svdq_linear_attention_args \*args\);", text, re.M)
    assert re.search(r"^#define SVDQ_ABI_VERSION 24$", text, re.M)
    assert _lib.ABI_VERSION == 24
    assert "svdq_linear_attention" in _lib.EXPORTS and "svdq_linear_attention_workspace_bytes" in _lib.EXPORTS
    assert "linear_attention.hip" in svdq_build.SOURCES and os.path.exists(os.path.join(svdq_build.CSRC, "linear_attention.hip"))


def test_struct_layout_matches_header(built_lib, tmp_path):
    cname, cls = "svdq_linear_attention_args", _lib.LinearAttentionArgs
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


B, T, H = 2, 300, 3
NEED = B * H * (2 + 1) * 33 * 32 * 4  # two chunks of 256 tokens + the sums, [33, 32] fp32 each


def _args(**over):
    """a call that would pass validation (the pointers are made up: no test below lets it reach a launch)"""
    a = _lib.LinearAttentionArgs()
    a.q, a.kv, a.out, a.vk, a.workspace = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000
    a.workspace_bytes = NEED
    a.B, a.T, a.H, a.head_dim, a.dtype, a.eps = B, T, H, 32, _lib.SVDQ_BF16, 1e-6
    a.ldq, a.ldkv, a.ldo = H * 32, H * 64, H * 32
    a.q_bs, a.kv_bs, a.out_bs = T * H * 32, T * H * 64, T * H * 32
    for k, v in over.items():
        setattr(a, k, v)
    return a


REFUSED = [
    (dict(kv=None), 1, b"kv and workspace are required"),
    (dict(workspace=None), 1, b"kv and workspace are required"),
    (dict(out=None), 1, b"go together"),
    (dict(q=None), 1, b"go together"),
    (dict(q=None, out=None, vk=None), 1, b"vk is required"),
    (dict(T=0), 1, b"T=0"),
    (dict(H=0), 1, b"H=0"),
    (dict(B=0), 1, b"B=0"),
    (dict(ldq=H * 32 - 8), 1, b"row strides"),
    (dict(ldkv=H * 64 - 8), 1, b"row strides"),
    (dict(ldo=H * 32 - 8), 1, b"row strides"),
    (dict(q_bs=(T - 1) * H * 32), 1, b"batch strides"),
    (dict(kv_bs=0), 1, b"batch strides"),
    (dict(out_bs=(T - 1) * H * 32 + 88), 1, b"batch strides"),
    (dict(q=0x10000 + 8), 1, b"16-byte aligned"),
    (dict(kv=0x20000 + 2), 1, b"16-byte aligned"),
    (dict(out=0x30000 + 4), 1, b"16-byte aligned"),
    (dict(vk=0x40000 + 4), 1, b"16-byte aligned"),
    (dict(workspace=0x50000 + 8), 1, b"16-byte aligned"),
    (dict(ldq=H * 32 + 4, q_bs=T * (H * 32 + 4)), 1, b"multiple of 8"),
    (dict(ldkv=H * 64 + 2, kv_bs=T * (H * 64 + 2)), 1, b"multiple of 8"),
    (dict(out_bs=T * H * 32 + 4), 1, b"multiple of 8"),
    (dict(dtype=7), 1, b"unknown dtype 7"),
    (dict(eps=-1.0), 1, b"eps"),
    (dict(eps=float("nan")), 1, b"eps"),
    (dict(workspace_bytes=NEED - 1), 1, str(NEED).encode()),
    (dict(head_dim=64), 2, b"head_dim=64"),  # SVDQ_E_UNSUPPORTED
    (dict(head_dim=128), 2, b"head_dim=128"),
]


def test_exported_and_every_validation_error_is_returned_without_a_launch(built_lib):
    raw = C.CDLL(built_lib)
    assert hasattr(raw, "svdq_linear_attention") and hasattr(raw, "svdq_linear_attention_workspace_bytes")
    lib = _lib.load()
    assert lib.svdq_abi_version() == 24
    assert lib.svdq_linear_attention(None, None) == 1 and b"NULL" in lib.svdq_last_error()
    assert lib.svdq_linear_attention_workspace_bytes(C.byref(_args())) == NEED
    assert lib.svdq_linear_attention_workspace_bytes(C.byref(_args(T=256))) == B * H * 2 * 33 * 32 * 4
    assert lib.svdq_linear_attention_workspace_bytes(C.byref(_args(T=0))) == 0 and lib.svdq_linear_attention_workspace_bytes(None) == 0
    for over, code, needle in REFUSED:
        rc = lib.svdq_linear_attention(C.byref(_args(**over)), None)
        msg = lib.svdq_last_error()
        assert rc == code and needle in msg, f"{over}: returned {rc}, {msg!r}"
    # only vk: q and out are not looked at -- but everything else still is
    rc = lib.svdq_linear_attention(C.byref(_args(q=None, out=None, ldq=0, ldo=0, q_bs=0, out_bs=0, workspace_bytes=NEED - 1)), None)
    assert rc == 1 and str(NEED).encode() in lib.svdq_last_error()


def test_wrappers_refuse_cpu_tensors_and_mismatched_arguments(built_lib):
    from nunchaku_amd._C import ops
    from nunchaku_amd.ops.attention import linear_attention

    qkv = torch.zeros(2, 8, 3 * 2 * 32, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="GPU tensors"):
        linear_attention(qkv, 2)
    with pytest.raises(ValueError, match="multiple of tokens"):
        linear_attention(qkv.view(16, -1), 2, tokens=5)
    with pytest.raises(ValueError, match="expected qkv"):
        linear_attention(qkv[..., :190], 2)
    with pytest.raises(ValueError, match="out must be"):
        linear_attention(qkv, 2, out=torch.zeros(2, 8, 32, dtype=torch.bfloat16))
    q, kv = qkv[..., :64].unflatten(-1, (2, 32)), qkv[..., 64:].unflatten(-1, (2, 64))
    with pytest.raises(ValueError, match="go together"):
        ops.linear_attention(q, kv, None)
    with pytest.raises(ValueError, match="nothing to compute"):
        ops.linear_attention(None, kv, None)
    with pytest.raises(ValueError, match="unit channel stride"):
        ops.linear_attention(q.transpose(2, 3), kv, torch.zeros_like(q))


# ---- the CPU restatements -----------------------------------------------------------------------------------------------------------
def test_reference_on_a_hand_computed_case():
    """T = 2, H = 1; only channels 0..2 are non-zero:
    K = [(2, -1), (1, 3)] -> relu K = [(2, 0), (1, 3)], column sums (3, 3);  V (channels 0 and 2) = [(1, 4), (-2, 0.5)]
    vk[0] = (1*2 - 2*1, 1*0 - 2*3) = (0, -6);   vk[2] = (4*2 + 0.5*1, 0.5*3) = (8.5, 1.5)
    Q[0] = (1, 2): numerators (0 - 12, 8.5 + 3) = (-12, 11.5), denominator 3 + 6 = 9 (+ eps);   Q[1] = (-1, 0): relu gives zeros"""
    qkv = torch.zeros(1, 2, 96, dtype=torch.float64)
    q, k, v = qkv[..., :32], qkv[..., 32:64], qkv[..., 64:]
    k[0, 0, :2], k[0, 1, :2] = torch.tensor([2.0, -1.0]), torch.tensor([1.0, 3.0])
    v[0, 0, 0], v[0, 0, 2], v[0, 1, 0], v[0, 1, 2] = 1.0, 4.0, -2.0, 0.5
    q[0, 0, :2], q[0, 1, 0] = torch.tensor([1.0, 2.0]), -1.0
    out, vk = litela_ref64(qkv, 1)
    want_vk = torch.zeros(33, 32, dtype=torch.float64)
    want_vk[0, 1], want_vk[2, 0], want_vk[2, 1], want_vk[32, 0], want_vk[32, 1] = -6.0, 8.5, 1.5, 3.0, 3.0
    assert torch.equal(vk[0, 0], want_vk)
    want = torch.zeros(2, 32, dtype=torch.float64)
    want[0, 0], want[0, 2] = -12.0 / (9.0 + 1e-6), 11.5 / (9.0 + 1e-6)
    assert torch.equal(out[0], want)
    o32, vk32 = litela_ref32(qkv.to(torch.bfloat16), 1)
    assert o32.dtype == torch.bfloat16 and torch.equal(o32[0], want.to(torch.bfloat16)) and torch.equal(vk32.double()[0, 0], want_vk)


def test_reference_equals_the_ones_row_formulation_and_its_zero_cases_are_exact():
    g = torch.Generator().manual_seed(3)
    Bq, Tq, Hq = 2, 37, 3
    qkv = torch.randn(Bq, Tq, 3 * Hq * 32, generator=g).to(torch.bfloat16)
    qkv[0, 5, : Hq * 32] = -qkv[0, 5, : Hq * 32].abs()          # a row whose Q is all <= 0 (every head)
    qkv[1, :, Hq * 32 + 64: Hq * 32 + 96] = -qkv[1, :, Hq * 32 + 64: Hq * 32 + 96].abs()  # batch 1, head 1: K all <= 0
    qkv[1, 3, Hq * 32 + 70] = 0.0
    out, vk = litela_ref64(qkv, Hq)
    out1, vk1 = litela_ones_row(qkv, Hq)
    assert torch.allclose(out, out1, rtol=1e-12, atol=0) and torch.allclose(vk, vk1, rtol=1e-12, atol=0)
    o32, vk32 = litela_ref32(qkv, Hq)
    for o in (out, o32.double()):
        assert (o[0, 5] == 0).all() and (o[1, :, 32:64] == 0).all()
        assert torch.isfinite(o).all() and (o[0, 4] != 0).any() and (o[1, :, :32] != 0).any()
    assert (vk[1, 1] == 0).all() and (vk32[1, 1] == 0).all()


# ---- the module -----------------------------------------------------------------------------------------------------------------------
def test_module_names_and_shapes_match_the_reference_layer(golden_dir):
    from nunchaku.models.sana import SanaLinearAttention as Mirrored
    from nunchaku_amd.models import SanaLinearAttention, convert_sana_attention_state_dict
    from nunchaku_amd.models.linear import SVDQW4A4Linear

    assert Mirrored is SanaLinearAttention
    m = SanaLinearAttention(2240, pag=True, device="meta")
    assert (m.dim, m.dim_pad, m.heads) == (2240, 2304, 72)
    assert [n for n, _ in m.named_children()] == ["qkv_proj", "out_proj", "pag_to_v"] and all(isinstance(c, SVDQW4A4Linear) for c in m.children())
    assert (m.qkv_proj.in_features, m.qkv_proj.out_features) == (2304, 6912) and m.qkv_proj.bias is None
    golden = json.load(open(os.path.join(golden_dir, "sana_attention_keys.json")))
    sd = m.state_dict()
    assert {k: list(v.shape) for k, v in sd.items()} == golden
    assert SanaLinearAttention(1152, device="meta").pag_to_v is None and SanaLinearAttention(1152, device="meta").heads == 36

    legacy = {}
    for k, v in sd.items():
        k = k.replace("proj_down", "lora_down").replace("proj_up", "lora_up").replace("smooth_factor_orig", "smooth_orig").replace("smooth_factor", "smooth")
        legacy[k] = torch.empty(v.shape, dtype=v.dtype)
    assert {"qkv_proj.lora_down", "out_proj.lora_up", "pag_to_v.smooth", "qkv_proj.smooth_orig"} <= set(legacy)
    assert not any(s in k for k in legacy for s in ("proj_down", "proj_up", "smooth_factor"))
    conv = convert_sana_attention_state_dict(legacy)
    assert set(conv) == set(sd) and all(conv[k.replace("lora_down", "proj_down")] is v for k, v in legacy.items() if "lora_down" in k)
    assert convert_sana_attention_state_dict(conv).keys() == conv.keys()  # names that are already converted pass through
    cpu = SanaLinearAttention(2240, pag=True)
    cpu.load_state_dict(conv, strict=True)
    with pytest.raises(RuntimeError):
        cpu.load_state_dict(legacy, strict=True)


def test_forward_pag_rejects_batches_it_cannot_split():
    from nunchaku_amd.models import SanaLinearAttention

    m = SanaLinearAttention(256, pag=True, device="meta")
    x = torch.empty(4, 16, 256, dtype=torch.bfloat16, device="meta")
    with pytest.raises(ValueError, match="multiple of 3"):
        m.forward_pag(x, True)
    with pytest.raises(ValueError, match="multiple of 2"):
        m.forward_pag(x[:3], False)
    with pytest.raises(RuntimeError, match="pag_to_v"):
        SanaLinearAttention(256, device="meta").forward_pag(x, False)
    with pytest.raises(ValueError, match="expected x"):
        m.forward(x[..., :128])
