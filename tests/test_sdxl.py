"""Stable Diffusion XL, the parts that need no GPU: the C ABI of ``svdq_attention_d64`` (header, bindings, exported symbol, validation without
a launch), the CPU restatements the GPU tests compare against (tests/attention_d64_ref.py), the module tree's names and shapes, the
checkpoint converter and the U-Net class in both of its builds."""

import ctypes as C
import json
import os
import re
import subprocess
import sys
import textwrap

import pytest
import torch

from nunchaku_amd import _lib
from nunchaku_amd import build as svdq_build
from tests.attention_d64_ref import attention_d64_ref, kernel_order_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- C ABI --------------------------------------------------------------------------------------------------------------------------
def test_header_bindings_and_sources_agree_and_the_abi_version_stays():
    text = open(os.path.join(ROOT, "include", "svdq_amd.h")).read()
    assert re.search(r"^int svdq_attention_d64\(const svdq_attention_d64_args \*args, void \*stream\);", text, re.M)
    assert re.search(r"^} svdq_attention_d64_args;", text, re.M)
    assert re.search(r"^#define SVDQ_ABI_VERSION 24$", text, re.M)
    assert _lib.ABI_VERSION == 24
    assert _lib.EXPORTS.get("svdq_attention_d64") == (C.c_int, [C.POINTER(_lib.AttentionD64Args), C.c_void_p])
    assert "attention_d64.hip" in svdq_build.SOURCES and os.path.exists(os.path.join(svdq_build.CSRC, "attention_d64.hip"))
    src = open(os.path.join(svdq_build.CSRC, "attention_d64.hip")).read()
    assert re.search(r"void attention_d64_kernel\(", src)  # (a 20-character name: the hot ledger's attention_kernel counts do not see it)


def test_struct_layout_matches_header(built_lib, tmp_path):
    cname, cls = "svdq_attention_d64_args", _lib.AttentionD64Args
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


B, T, H, N = 2, 40, 3, 77
HD = H * 64
LDP = 3 * HD                       # q, k, v as the thirds of packed rows
Q_BS, K_BS, O_BS = T * LDP, N * LDP, T * HD
Q_NEED, K_NEED, O_NEED = (T - 1) * LDP + HD, (N - 1) * LDP + HD, (T - 1) * HD + HD
PQ, PK, PV, PO = 0x100000, 0x200000, 0x300000, 0x400000


def _args(**over):
    """a call that would pass validation (the pointers are made up: no test below lets it reach a launch)"""
    a = _lib.AttentionD64Args()
    a.q, a.k, a.v, a.out = PQ, PK, PV, PO
    a.ldq, a.ldk, a.ldv, a.ldo = LDP, LDP, LDP, HD
    a.q_bs, a.k_bs, a.v_bs, a.out_bs = Q_BS, K_BS, K_BS, O_BS
    a.B, a.T, a.H, a.N, a.head_dim = B, T, H, N, 64
    a.dtype, a.scale = _lib.SVDQ_BF16, 64 ** -0.5
    for k, v in over.items():
        setattr(a, k, v)
    return a


INVALID, UNSUPPORTED = 1, 2
REFUSED = [
    (dict(q=None), INVALID, b"are required"),
    (dict(k=None), INVALID, b"are required"),
    (dict(v=None), INVALID, b"are required"),
    (dict(out=None), INVALID, b"are required"),
    (dict(B=0), INVALID, b"B=0"),
    (dict(T=0), INVALID, b"T=0"),
    (dict(H=-1), INVALID, b"H=-1"),
    (dict(N=0), INVALID, b"N=0"),
    (dict(N=-5), INVALID, b"N=-5"),
    (dict(B=21846, H=3), INVALID, b"exceed the grid"),
    (dict(T=(1 << 30) + 1), INVALID, b"exceed the grid"),
    (dict(N=(1 << 30) + 1), INVALID, b"exceed the grid"),
    (dict(ldq=HD - 8), INVALID, b"row strides"),
    (dict(ldk=HD - 8), INVALID, b"row strides"),
    (dict(ldv=HD - 8), INVALID, b"row strides"),
    (dict(ldo=HD - 8), INVALID, b"row strides"),
    (dict(ldq=LDP + 4), INVALID, b"16-byte aligned"),
    (dict(ldk=LDP + 2), INVALID, b"16-byte aligned"),
    (dict(ldv=LDP + 1), INVALID, b"16-byte aligned"),
    (dict(ldo=HD + 4), INVALID, b"16-byte aligned"),
    (dict(q=PQ + 8), INVALID, b"16-byte aligned"),
    (dict(k=PK + 2), INVALID, b"16-byte aligned"),
    (dict(v=PV + 4), INVALID, b"16-byte aligned"),
    (dict(out=PO + 8), INVALID, b"16-byte aligned"),
    (dict(q_bs=Q_NEED - 8), INVALID, b"batch strides (q_bs=%d" % (Q_NEED - 8)),
    (dict(k_bs=K_NEED - 8), INVALID, b"must be at least"),
    (dict(v_bs=K_NEED - 8), INVALID, b"must be at least"),
    (dict(out_bs=O_NEED - 8), INVALID, b"must be at least"),
    (dict(out_bs=0), INVALID, b"must be at least"),
    (dict(q_bs=Q_BS + 4), INVALID, b"must be a multiple of 8"),
    (dict(k_bs=K_BS + 2), INVALID, b"must be a multiple of 8"),
    (dict(v_bs=K_BS + 1), INVALID, b"must be a multiple of 8"),
    (dict(out_bs=O_BS + 4), INVALID, b"must be a multiple of 8"),
    (dict(dtype=7), INVALID, b"unknown dtype 7"),
    (dict(scale=0.0), INVALID, b"scale must be positive and finite"),
    (dict(scale=-0.1), INVALID, b"scale must be positive and finite"),
    (dict(scale=float("inf")), INVALID, b"scale must be positive and finite"),
    (dict(scale=float("nan")), INVALID, b"scale must be positive and finite"),
    (dict(out=PQ), INVALID, b"out overlaps q"),
    (dict(out=PQ + 2 * (Q_BS + Q_NEED) - 16), INVALID, b"out overlaps q"),       # the last 16 bytes of q
    (dict(out=PK + 2 * HD), INVALID, b"out overlaps k"),                          # the next third of k's packed rows
    (dict(out=PV - 2 * O_BS), INVALID, b"out overlaps v"),                        # its second sample reaches v's first row
    (dict(head_dim=128), UNSUPPORTED, b"head_dim=128"),
    (dict(head_dim=72), UNSUPPORTED, b"head_dim=72"),
    (dict(head_dim=32), UNSUPPORTED, b"head_dim=32"),
    (dict(head_dim=0), UNSUPPORTED, b"head_dim=0"),
]


def test_exported_and_every_validation_error_is_returned_without_a_launch(built_lib):
    raw = C.CDLL(built_lib)
    assert hasattr(raw, "svdq_attention_d64")
    lib = _lib.load()
    assert lib.svdq_abi_version() == 24
    assert lib.svdq_attention_d64(None, None) == 1 and b"NULL" in lib.svdq_last_error()
    for over, want, needle in REFUSED:
        rc = lib.svdq_attention_d64(C.byref(_args(**over)), None)
        msg = lib.svdq_last_error()
        assert rc == want and needle in msg, f"{over}: returned {rc}, {msg!r}"


def test_an_output_that_ends_where_an_input_begins_is_not_an_overlap(built_lib):
    """the extents are half-open: out's last byte directly before q's first is refused for nothing (here: for the scale, checked later)"""
    lib = _lib.load()
    out_bytes = 2 * (O_BS + O_NEED)
    rc = lib.svdq_attention_d64(C.byref(_args(out=PQ - out_bytes, scale=0.0)), None)
    assert rc == INVALID and b"scale" in lib.svdq_last_error()
    rc = lib.svdq_attention_d64(C.byref(_args(out=PQ - out_bytes + 16)), None)
    assert rc == INVALID and b"out overlaps q" in lib.svdq_last_error()


# ---- the CPU restatements -------------------------------------------------------------------------------------------------------------
def test_restatement_equals_a_dense_softmax_in_float64_and_the_kernel_order_agrees_with_it():
    g = torch.Generator().manual_seed(11)
    Bq, Tq, heads, Nk = 2, 19, 3, 150
    hd = heads * 64
    q = torch.randn(Bq, Tq, hd + 8, generator=g).bfloat16()
    kv = torch.randn(Bq, Nk, 2 * hd, generator=g).bfloat16()
    k, v = kv[..., :hd], kv[..., hd:]
    ref = attention_d64_ref(q, k, v, heads)
    assert ref.dtype == torch.float32 and tuple(ref.shape) == (Bq, Tq, hd)
    q4 = q[..., :hd].double().view(Bq, Tq, heads, 64).transpose(1, 2)
    k4, v4 = k.double().reshape(Bq, Nk, heads, 64).transpose(1, 2), v.double().reshape(Bq, Nk, heads, 64).transpose(1, 2)
    dense = (torch.softmax(0.125 * (q4 @ k4.transpose(2, 3)), dim=-1) @ v4).transpose(1, 2).reshape(Bq, Tq, hd)
    vmax = v.double().abs().max().item()
    assert (ref.double() - dense).abs().max().item() <= 16 * 2.0 ** -24 * vmax
    # the kernel's order of operations (three chunks, the last one of 22 keys): what separates it from the dense softmax is the rounding of P to
    # bf16, 2^-9 relative per probability; numerator and denominator carry the same rounded values, so the quotient moves by at most 2 * 2^-9
    for b in range(Bq):
        got = kernel_order_ref(q[b, :, :hd], k[b], v[b], heads)
        assert (got.double() - dense[b]).abs().max().item() <= 2 * 2.0 ** -9 * vmax
    # a dominant key: its V row comes back exactly
    q1 = torch.zeros(1, 64)
    q1[0, 0] = 400.0
    k1 = torch.zeros(70, 64)
    k1[64, 0] = 1.0
    v1 = torch.randn(70, 64, generator=g).bfloat16()
    assert torch.equal(kernel_order_ref(q1.bfloat16(), k1.bfloat16(), v1, 1), v1[64:65].float())


# ---- the op wrapper -------------------------------------------------------------------------------------------------------------------
def test_wrapper_refuses_mismatched_arguments_and_cpu_tensors(built_lib):
    from nunchaku_amd.ops import attention_d64
    from nunchaku_amd.ops.attention import attention_d64 as same

    assert attention_d64 is same
    qkv = torch.zeros(2, 10, 3 * 128, dtype=torch.bfloat16)
    q, k, v = qkv[..., :128], qkv[..., 128:256], qkv[..., 256:]
    with pytest.raises(ValueError, match="q must be a GPU tensor"):
        attention_d64(q, k, v, 2)
    with pytest.raises(NotImplementedError, match="head_dim=128"):
        attention_d64(q, k, v, 1)
    with pytest.raises(NotImplementedError, match="head_dim=32"):
        attention_d64(q, k, v, 4)
    with pytest.raises(ValueError, match="not a multiple of heads=3"):
        attention_d64(q, k, v, 3)
    with pytest.raises(TypeError, match="q must be bfloat16 or float16"):
        attention_d64(q.float(), k, v, 2)
    with pytest.raises(TypeError, match="must have q's dtype"):
        attention_d64(q, k.half(), v, 2)
    with pytest.raises(ValueError, match="all be"):
        attention_d64(q[0], k, v, 2)
    with pytest.raises(ValueError, match="expected q"):
        attention_d64(q, k[:, :5], v, 2)
    with pytest.raises(ValueError, match="expected q"):
        attention_d64(q, k[:1], v[:1], 2)
    for bad in (torch.zeros(2, 10, 256, dtype=torch.bfloat16), torch.zeros(2, 9, 128, dtype=torch.bfloat16), torch.zeros(2, 10, 128, dtype=torch.float16),
                torch.zeros(2, 10, 128, dtype=torch.bfloat16, device="meta")):
        with pytest.raises(ValueError, match="out must be a torch.bfloat16 tensor of shape \\(2, 10, 128\\)"):
            attention_d64(q, k, v, 2, out=bad)


# ---- the modules ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,heads", [(640, 10), (1280, 20)])
def test_block_names_and_shapes_match_the_reference_tree(golden_dir, dim, heads):
    from nunchaku.models.attention_processors.sdxl import NunchakuSDXLFA2Processor as MirroredProcessor
    from nunchaku.models.unets import NunchakuSDXLAttention as MirroredAttention
    from nunchaku.models.unets.unet_sdxl import NunchakuSDXLFeedForward, NunchakuSDXLTransformerBlock
    from nunchaku_amd.models import sdxl
    from nunchaku_amd.models.linear import SVDQW4A4Linear

    assert NunchakuSDXLTransformerBlock is sdxl.NunchakuSDXLTransformerBlock and MirroredAttention is sdxl.NunchakuSDXLAttention
    assert MirroredProcessor is sdxl.NunchakuSDXLFA2Processor
    blk = NunchakuSDXLTransformerBlock(dim, heads, 2048, rank=32, device="meta")
    assert [n for n, _ in blk.named_children()] == ["norm1", "norm2", "norm3", "attn1", "attn2", "ff"]
    assert all(type(n) is torch.nn.LayerNorm and n.normalized_shape == (dim,) for n in (blk.norm1, blk.norm2, blk.norm3))
    assert (blk.norm_type, blk.pos_embed, blk.only_cross_attention) == ("layer_norm", None, False)
    a1, a2 = blk.attn1, blk.attn2
    assert [n for n, _ in a1.named_children()] == ["to_qkv", "to_out"] and [n for n, _ in a2.named_children()] == ["to_q", "to_k", "to_v", "to_out"]
    assert (a1.heads, a1.is_cross_attention, a1.rescale_output_factor) == (heads, False, 1.0) and a2.is_cross_attention and a2.heads == heads
    assert isinstance(a1.to_qkv, SVDQW4A4Linear) and (a1.to_qkv.in_features, a1.to_qkv.out_features, a1.to_qkv.bias) == (dim, 3 * dim, None)
    assert isinstance(a2.to_q, SVDQW4A4Linear) and type(a2.to_k) is torch.nn.Linear and type(a2.to_v) is torch.nn.Linear
    assert a2.to_k.bias is None and tuple(a2.to_v.weight.shape) == (dim, 2048)
    for a in (a1, a2):
        assert isinstance(a.to_out, torch.nn.ModuleList) and isinstance(a.to_out[0], SVDQW4A4Linear) and type(a.to_out[1]) is torch.nn.Dropout
        assert isinstance(a.processor, sdxl.NunchakuSDXLFA2Processor)
        with pytest.raises(ValueError, match="Processor nunchaku-fp16 is not supported"):
            a.set_processor("nunchaku-fp16")
    assert isinstance(blk.ff, NunchakuSDXLFeedForward) and isinstance(blk.ff.net, torch.nn.ModuleList) and len(blk.ff.net) == 3
    proj = blk.ff.net[0].proj
    assert isinstance(proj, SVDQW4A4Linear) and (proj.in_features, proj.out_features) == (dim, 8 * dim) and type(blk.ff.net[1]) is torch.nn.Dropout
    assert isinstance(blk.ff.net[2], SVDQW4A4Linear) and (blk.ff.net[2].in_features, blk.ff.net[2].out_features) == (4 * dim, dim)
    golden = json.load(open(os.path.join(golden_dir, "sdxl_block_keys.json")))[str(dim)]
    assert {k: list(v.shape) for k, v in blk.state_dict().items()} == golden
    assert NunchakuSDXLTransformerBlock(dim, heads, 2048, torch_dtype=torch.float16, device="meta").attn2.to_k.weight.dtype == torch.float16
    assert tuple(NunchakuSDXLTransformerBlock(dim, heads, 2048, rank=64, device="meta").ff.net[2].proj_down.shape) == (4 * dim, 64)
    for precision in ("fp4", "nvfp4"):
        with pytest.raises(NotImplementedError, match="NVFP4"):
            NunchakuSDXLTransformerBlock(dim, heads, 2048, precision=precision, device="meta")


def test_forward_refuses_masks_other_norms_and_only_cross_attention():
    from nunchaku_amd.models.sdxl import NunchakuSDXLTransformerBlock

    blk = NunchakuSDXLTransformerBlock(128, 2, 256, device="meta")
    x, enc = torch.empty(1, 8, 128, dtype=torch.bfloat16, device="meta"), torch.empty(1, 5, 256, dtype=torch.bfloat16, device="meta")
    with pytest.raises(NotImplementedError, match="attention_mask is not supported"):
        blk(x, attention_mask=torch.empty(1, 8, device="meta"), encoder_hidden_states=enc)
    with pytest.raises(NotImplementedError, match="attention_mask is not supported"):
        blk.attn2(x, encoder_hidden_states=enc, attention_mask=torch.empty(1, 5, device="meta"))
    blk.only_cross_attention = True
    with pytest.raises(ValueError, match="only_cross_attention cannot be True"):
        blk(x, encoder_hidden_states=enc)
    blk.only_cross_attention, blk.norm_type = False, "ada_norm"
    with pytest.raises(ValueError, match="Incorrect norm"):
        blk(x, encoder_hidden_states=enc)


def _legacy(name: str) -> str:
    return (name.replace("proj_down", "lora_down").replace("proj_up", "lora_up").replace("smooth_factor_orig", "smooth_orig")
            .replace("smooth_factor", "smooth"))


def test_convert_sdxl_state_dict():
    from nunchaku.models.unets.unet_sdxl import convert_sdxl_state_dict as mirrored
    from nunchaku_amd.models.sdxl import NunchakuSDXLTransformerBlock, convert_sdxl_state_dict

    assert mirrored is convert_sdxl_state_dict
    blk = NunchakuSDXLTransformerBlock(128, 2, 256)
    pre = "down_blocks.1.attentions.0.transformer_blocks.0."
    legacy = {pre + _legacy(k): torch.empty(v.shape, dtype=v.dtype) for k, v in blk.state_dict().items()}
    assert {pre + "attn1.to_qkv.lora_down", pre + "attn1.to_out.0.lora_up", pre + "ff.net.2.smooth", pre + "ff.net.0.proj.smooth_orig"} <= set(legacy)
    assert not any(s in k for k in legacy for s in ("proj_down", "proj_up", "smooth_factor"))
    outside = {"down_blocks.0.resnets.0.conv1.smooth": torch.zeros(1), "mid_block.resnets.0.lora_down": torch.zeros(1),
               "time_embedding.linear_1.smooth_orig": torch.zeros(1), "conv_in.weight": torch.zeros(1)}
    conv = convert_sdxl_state_dict({**legacy, **outside})
    assert all(conv[k] is v for k, v in outside.items())                       # untouched, by name and by tensor
    assert conv[pre + "ff.net.0.proj.smooth_factor_orig"] is legacy[pre + "ff.net.0.proj.smooth_orig"]   # not "smooth_factor_orig" via "smooth"
    assert conv[pre + "ff.net.0.proj.smooth_factor"] is legacy[pre + "ff.net.0.proj.smooth"]
    assert conv[pre + "attn2.to_q.proj_down"] is legacy[pre + "attn2.to_q.lora_down"] and conv[pre + "attn2.to_q.proj_up"] is legacy[pre + "attn2.to_q.lora_up"]
    assert conv[pre + "attn2.to_k.weight"] is legacy[pre + "attn2.to_k.weight"]
    inner = {k[len(pre):]: v for k, v in conv.items() if k.startswith(pre)}
    assert set(inner) == set(blk.state_dict())
    assert convert_sdxl_state_dict(conv).keys() == conv.keys()                  # names that are already converted pass through
    blk.load_state_dict(inner, strict=True)
    with pytest.raises(RuntimeError):
        blk.load_state_dict({k[len(pre):]: v for k, v in legacy.items()}, strict=True)


# ---- the U-Net class ------------------------------------------------------------------------------------------------------------------
PREFIXES = ["down_blocks.1.attentions.0.transformer_blocks.0", "down_blocks.1.attentions.0.transformer_blocks.1",
            "mid_block.attentions.0.transformer_blocks.0", "up_blocks.0.attentions.0.transformer_blocks.0"]
DIMS = {PREFIXES[0]: 128, PREFIXES[1]: 128, PREFIXES[2]: 256, PREFIXES[3]: 128}
CROSS, RANK = 192, 16
TINY = dict(block_out_channels=[64, 128, 256], cross_attention_dim=CROSS, in_channels=4)


def _fill_(module, seed=0):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in module.parameters():
            p.copy_(torch.randint(-100, 100, p.shape, generator=g) if p.dtype in (torch.int8, torch.int32) else torch.randn(p.shape, generator=g))
    return module


def _tiny_checkpoint(path, legacy=True, dtype=torch.bfloat16, extra=None):
    """four quantised blocks of two widths under the module paths of an SDXL checkpoint, in the checkpoint's (legacy) names, plus the tensors
    ``extra`` that belong to the rest of the U-Net (default: the two of ``conv_in``)"""
    from safetensors.torch import save_file

    from nunchaku_amd.models.sdxl import NunchakuSDXLTransformerBlock

    blocks, sd = {}, {}
    for i, pre in enumerate(PREFIXES):
        blocks[pre] = _fill_(NunchakuSDXLTransformerBlock(DIMS[pre], DIMS[pre] // 64, CROSS, rank=RANK, torch_dtype=dtype), seed=i)
        for k, v in blocks[pre].state_dict().items():
            sd[pre + "." + (_legacy(k) if legacy else k)] = v.contiguous()
    g = torch.Generator().manual_seed(99)
    for k, shape in (extra or {"conv_in.weight": (64, 4, 3, 3), "conv_in.bias": (64,)}).items():
        sd[k] = torch.randn(tuple(shape), generator=g).to(dtype)
    save_file(sd, path, metadata={"config": json.dumps(TINY), "quantization_config": json.dumps({"rank": RANK})})
    return blocks, sd


def test_diffusers_free_build_loads_the_blocks_and_refuses_forward_fp4_and_offload(tmp_path):
    try:
        import diffusers  # noqa: F401

        return  # the real build is the one in use
    except ImportError:
        pass
    from nunchaku.models.unets import NunchakuSDXLUNet2DConditionModel as Mirrored
    from nunchaku_amd.models import sdxl

    cls = sdxl.NunchakuSDXLUNet2DConditionModel
    assert Mirrored is cls and not sdxl.HAVE_DIFFUSERS and issubclass(cls, torch.nn.Module)
    path = str(tmp_path / "tiny.safetensors")
    blocks, sd = _tiny_checkpoint(path)
    m = cls.from_pretrained(path, device="cpu")
    assert m.dtype == torch.bfloat16 and m.device.type == "cpu" and m.config.cross_attention_dim == CROSS
    assert m.transformer_block_names == PREFIXES
    for pre in PREFIXES:
        blk = m.transformer_block(pre)
        assert isinstance(blk, sdxl.NunchakuSDXLTransformerBlock) and blk.attn1.heads == DIMS[pre] // 64 and blk.attn1.to_qkv.rank == RANK
        a, b = blocks[pre].state_dict(), blk.state_dict()
        assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)
    assert set(m.state_dict()) == {k for k in sdxl.convert_sdxl_state_dict(sd) if ".transformer_blocks." in k}
    assert set(m.unquantized_state_dict) == {"conv_in.weight", "conv_in.bias"}
    assert torch.equal(m.unquantized_state_dict["conv_in.bias"], sd["conv_in.bias"])
    with pytest.raises(RuntimeError, match="diffusers"):
        m(torch.zeros(1, 4, 8, 8), 0, torch.zeros(1, 77, CROSS))
    for precision in ("fp4", "nvfp4"):
        with pytest.raises(NotImplementedError, match="NVFP4"):
            cls.from_pretrained(path, device="cpu", precision=precision)
    with pytest.raises(NotImplementedError, match="Offload is not supported"):
        cls.from_pretrained(path, device="cpu", offload=True)
    with pytest.raises(ValueError, match="Only safetensors are supported"):
        cls.from_pretrained(str(tmp_path / "tiny.bin"), device="cpu")
    assert cls.from_pretrained(path, device="cpu", torch_dtype=torch.float16).dtype == torch.float16
    # a checkpoint that is already in this package's names loads the same way
    path2 = str(tmp_path / "converted.safetensors")
    _tiny_checkpoint(path2, legacy=False)
    m2 = cls.from_pretrained(path2, device="cpu")
    assert all(torch.equal(v, m2.state_dict()[k]) for k, v in m.state_dict().items())


FAKE_DIFFUSERS = {
    "__init__.py": '''
        import inspect
        import torch
        from torch import nn
        from .models.attention import BasicTransformerBlock

        class FrozenDict(dict):
            def __getattr__(self, k):
                try: return self[k]
                except KeyError: raise AttributeError(k)

        class _Transformer2DModel(nn.Module):
            def __init__(self, dim, heads, cross, layers):
                super().__init__()
                self.proj_in = nn.Linear(dim, dim)
                self.transformer_blocks = nn.ModuleList([BasicTransformerBlock(dim, heads, cross) for _ in range(layers)])

        class _Stage(nn.Module):
            """a down / up / mid block: resnets (stood in for by a convolution) and, for the cross-attention kinds, attentions"""
            def __init__(self, ch, cross, attentions, layers):
                super().__init__()
                self.resnets = nn.ModuleList([nn.Conv2d(ch, ch, 3)])
                if attentions:
                    self.attentions = nn.ModuleList([_Transformer2DModel(ch, ch // 64, cross, layers) for _ in range(attentions)])

        class UNet2DConditionModel(nn.Module):
            """the shape of diffusers' class that matters here: config registration, from_config, down_blocks / up_blocks / mid_block whose
            attentions hold full-size BasicTransformerBlocks"""
            def __init__(self, in_channels=4, block_out_channels=(320, 640, 1280), cross_attention_dim=2048):
                super().__init__()
                self.config = FrozenDict(in_channels=in_channels, block_out_channels=block_out_channels, cross_attention_dim=cross_attention_dim)
                c0, c1, c2 = block_out_channels
                self.conv_in = nn.Conv2d(in_channels, c0, 3)
                self.down_blocks = nn.ModuleList([_Stage(c0, cross_attention_dim, 0, 0), _Stage(c1, cross_attention_dim, 1, 2)])
                self.mid_block = _Stage(c2, cross_attention_dim, 1, 1)
                self.up_blocks = nn.ModuleList([_Stage(c1, cross_attention_dim, 1, 1), _Stage(c0, cross_attention_dim, 0, 0)])

            @classmethod
            def from_config(cls, config):
                expected = set(inspect.signature(cls.__init__).parameters) - {"self", "kwargs"}
                return cls(**{k: v for k, v in config.items() if k in expected})

            @property
            def dtype(self):
                return self.conv_in.weight.dtype

            @property
            def device(self):
                return self.conv_in.weight.device
        ''',
    "models/__init__.py": "",
    "models/attention.py": '''
        from torch import nn
        from .attention_processor import Attention

        class GEGLU(nn.Module):
            def __init__(self, dim_in, dim_out):
                super().__init__()
                self.proj = nn.Linear(dim_in, dim_out * 2)

        class FeedForward(nn.Module):
            def __init__(self, dim, mult=4):
                super().__init__()
                self.net = nn.ModuleList([GEGLU(dim, dim * mult), nn.Dropout(0.0), nn.Linear(dim * mult, dim)])

        class BasicTransformerBlock(nn.Module):
            def __init__(self, dim, num_attention_heads, cross_attention_dim):
                super().__init__()
                self.norm_type, self.pos_embed, self.only_cross_attention = "layer_norm", None, False
                self.norm1 = nn.LayerNorm(dim)
                self.attn1 = Attention(dim, None, num_attention_heads)
                self.norm2 = nn.LayerNorm(dim)
                self.attn2 = Attention(dim, cross_attention_dim, num_attention_heads)
                self.norm3 = nn.LayerNorm(dim)
                self.ff = FeedForward(dim)
        ''',
    "models/attention_processor.py": '''
        from torch import nn

        class Attention(nn.Module):
            def __init__(self, query_dim, cross_attention_dim, heads):
                super().__init__()
                self.is_cross_attention = cross_attention_dim is not None
                self.heads, self.rescale_output_factor = heads, 1.0
                kv = cross_attention_dim if self.is_cross_attention else query_dim
                self.to_q = nn.Linear(query_dim, query_dim, bias=False)
                self.to_k = nn.Linear(kv, query_dim, bias=False)
                self.to_v = nn.Linear(kv, query_dim, bias=False)
                self.to_out = nn.ModuleList([nn.Linear(query_dim, query_dim), nn.Dropout(0.0)])
        ''',
}

DIFFUSERS_SCRIPT = '''
import json, sys, torch
sys.path.insert(0, sys.argv[2])
import diffusers
from diffusers.models.attention import BasicTransformerBlock, FeedForward
from nunchaku_amd.models import sdxl
from tests.test_sdxl import CROSS, PREFIXES, RANK, TINY, _tiny_checkpoint
assert sdxl.HAVE_DIFFUSERS
cls = sdxl.NunchakuSDXLUNet2DConditionModel
assert issubclass(cls, diffusers.UNet2DConditionModel) and issubclass(cls, sdxl.NunchakuModelLoaderMixin)
assert issubclass(sdxl.NunchakuSDXLTransformerBlock, BasicTransformerBlock) and issubclass(sdxl.NunchakuSDXLFeedForward, FeedForward)
with torch.device("meta"):  # what a full checkpoint holds besides the blocks: every other tensor of the U-Net
    rest = {k: v.shape for k, v in diffusers.UNet2DConditionModel(**TINY).state_dict().items() if ".transformer_blocks." not in k}
blocks, sd = _tiny_checkpoint(sys.argv[1], extra=rest)
m = cls.from_pretrained(sys.argv[1], device="cpu")
assert isinstance(m, diffusers.UNet2DConditionModel) and m.config.cross_attention_dim == CROSS and m.dtype == torch.bfloat16
assert not any(p.is_meta for p in m.parameters()), "a meta-device parameter of the diffusers skeleton survived"
found = [n for n, mod in m.named_modules() if isinstance(mod, BasicTransformerBlock)]
assert found == PREFIXES, found                                              # every block of down / mid / up, and nothing else
assert all(type(m.get_submodule(n)) is sdxl.NunchakuSDXLTransformerBlock for n in found), "_patch_model left a diffusers block in place"
assert set(m.state_dict()) == set(sdxl.convert_sdxl_state_dict(sd))          # the converted checkpoint's keys, all of them and no others
for pre in PREFIXES:
    blk = m.get_submodule(pre)
    assert blk.attn1.to_qkv.rank == RANK and type(blk.ff.net[0]) is sdxl.NunchakuSDXLGEGLU and type(blk.attn2.to_k) is torch.nn.Linear
    a, b = blocks[pre].state_dict(), blk.state_dict()
    assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)
assert torch.equal(m.conv_in.weight, sd["conv_in.weight"]) and torch.equal(m.mid_block.resnets[0].bias, sd["mid_block.resnets.0.bias"])
assert not hasattr(m, "unquantized_state_dict")
for kw in (dict(precision="fp4"), dict(offload=True)):
    try:
        cls.from_pretrained(sys.argv[1], device="cpu", **kw)
        raise SystemExit(f"{kw} was not refused")
    except NotImplementedError:
        pass
print("OK")
'''


def test_real_subclass_build_against_a_stand_in_diffusers(tmp_path):
    for name, text in FAKE_DIFFUSERS.items():
        f = tmp_path / "diffusers" / name
        f.parent.mkdir(parents=True, exist_ok=True)
        f.write_text(textwrap.dedent(text))
    script = tmp_path / "run.py"
    script.write_text(textwrap.dedent(DIFFUSERS_SCRIPT))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([str(tmp_path), ROOT, os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, str(script), str(tmp_path / "tiny.safetensors"), ROOT], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr
