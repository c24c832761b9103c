"""Z-Image, the parts that need no GPU: the C ABI of ``svdq_sandwich_norm`` and ``svdq_qk_norm_rope`` (header, bindings, exported symbols,
validation without a launch), the CPU restatements the GPU tests compare against (tests/zimage_ref.py) held to the 16-bit torch-op sequences
they restate, the module tree's names and shapes and the model class."""

import ctypes as C
import json
import os
import re
import subprocess

import pytest
import torch

from nunchaku_amd import _lib
from nunchaku_amd import build as svdq_build
from tests import zimage_ref as Z

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = ["bf16", "fp16"]


# ---- C ABI --------------------------------------------------------------------------------------------------------------------------
def test_header_bindings_and_sources_agree_and_the_abi_version_stays():
    text = open(os.path.join(ROOT, "include", "svdq_amd.h")).read()
    for fn, struct, cls, src, kernel in (("svdq_sandwich_norm", "svdq_sandwich_norm_args", _lib.SandwichNormArgs, "sandwich_norm.hip", "sandwich_norm_kernel"),
                                         ("svdq_qk_norm_rope", "svdq_qk_norm_rope_args", _lib.QkNormRopeArgs, "qk_norm_rope.hip", "qk_norm_rope_kernel")):
        assert re.search(rf"^int {fn}\(const {struct} \*args, void \*stream\);", text, re.M)
        assert re.search(rf"^}} {struct};", text, re.M)
        assert _lib.EXPORTS.get(fn) == (C.c_int, [C.POINTER(cls), C.c_void_p])
        assert src in svdq_build.SOURCES and os.path.exists(os.path.join(svdq_build.CSRC, src))
        assert re.search(rf"void {kernel}\(", open(os.path.join(svdq_build.CSRC, src)).read())
    assert re.search(r"^#define SVDQ_ABI_VERSION 24$", text, re.M) and _lib.ABI_VERSION == 24


def test_struct_layouts_match_header(built_lib, tmp_path):
    structs = {"svdq_sandwich_norm_args": _lib.SandwichNormArgs, "svdq_qk_norm_rope_args": _lib.QkNormRopeArgs}
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{os.path.join(ROOT, "include", "svdq_amd.h")}"', "int main(void) {"]
    for cname, cls in structs.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        lines += [f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));' for f, _ in cls._fields_]
    lines.append("return 0; }")
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(src)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for cname, cls in structs.items():
        assert int(got[cname]) == C.sizeof(cls)
        for f, _ in cls._fields_:
            assert int(got[f"{cname}.{f}"]) == getattr(cls, f).offset, f"offsetof({cname}, {f})"


INVALID, UNSUPPORTED = 1, 2
P = [0x100000 * (i + 1) for i in range(10)]  # made-up addresses: no test below lets a call reach a launch


def _sandwich(**over):
    """a call that would pass validation"""
    a = _lib.SandwichNormArgs()
    a.res, a.a, a.w_post, a.gate, a.w_pre, a.scale, a.out, a.out_mod, a.stats = P[:9]
    a.M, a.T, a.C, a.dtype, a.eps = 10, 5, 3840, _lib.SVDQ_BF16, 1e-5
    a.ld_res = a.ld_a = a.ld_out = a.ld_mod = 3840 + 24
    a.gate_bs = a.scale_bs = 4 * 3840
    for k, v in over.items():
        setattr(a, k, v)
    return a


SANDWICH_REFUSED = [
    (dict(res=None), INVALID, b"res and one of out / out_mod / stats are required"),
    (dict(out=None, out_mod=None, stats=None), INVALID, b"one of out / out_mod / stats"),             # no output
    (dict(a=None), INVALID, b"gate needs a"),                                                          # gate without a
    (dict(w_post=None), INVALID, b"a needs w_post"),
    (dict(w_pre=None), INVALID, b"out_mod needs w_pre"),
    (dict(res=P[0] + 8), INVALID, b"16-byte aligned"),                                                 # a misaligned pointer
    (dict(gate=P[3] + 2), INVALID, b"16-byte aligned"),
    (dict(stats=P[8] + 4), INVALID, b"8-byte aligned"),
    (dict(ld_res=3840 - 8), INVALID, b"ld=3832 >= C"),                                                 # a stride below the width
    (dict(ld_a=3840 - 8), INVALID, b"ld=3832 >= C"),
    (dict(ld_out=8), INVALID, b"ld=8 >= C"),
    (dict(ld_mod=3840 + 4), INVALID, b"ld=3844 >= C and a multiple of 8"),
    (dict(C=3836, ld_res=3840), INVALID, b"C=3836 a multiple of 8"),
    (dict(M=0), INVALID, b"M=0 > 0"),
    (dict(T=0), INVALID, b"T=0"),
    (dict(T=4), INVALID, b"not whole samples of T=4"),
    (dict(gate_bs=3832), INVALID, b"gate_bs=3832"),
    (dict(scale_bs=3844), INVALID, b"scale_bs=3844"),
    (dict(dtype=7), INVALID, b"unknown dtype 7"),
    (dict(eps=-1.0), INVALID, b"eps must be finite"),
    (dict(eps=float("nan")), INVALID, b"eps must be finite"),
    (dict(C=4608, ld_res=4608, ld_a=4608, ld_out=4608, ld_mod=4608, gate_bs=4608, scale_bs=4608), UNSUPPORTED, b"C=4608: ceil(C/512) must be one of"),
]


def _qk(**over):
    a = _lib.QkNormRopeArgs()
    a.qkv, a.norm_q, a.norm_k, a.freqs, a.vt, a.rstd = P[:6]
    a.T, a.L_pad, a.H, a.head_dim, a.ld, a.ldvt = 130, 256, 3, 128, 3 * 3 * 128 + 64, 256 + 128
    a.dtype, a.eps = _lib.SVDQ_FP16, 1e-5
    for k, v in over.items():
        setattr(a, k, v)
    return a


QK_REFUSED = [
    (dict(qkv=None), INVALID, b"qkv is required"),
    (dict(H=0), INVALID, b"H=0"),
    (dict(T=0), INVALID, b"T=0"),
    (dict(H=70000, ld=3 * 70000 * 128), INVALID, b"H=70000"),
    (dict(ld=3 * 3 * 128 - 8), INVALID, b"ld=1144 must be at least 3 * H * 128 = 1152"),                # a stride below the width
    (dict(ld=3 * 3 * 128 + 4), INVALID, b"a multiple of 8"),
    (dict(L_pad=128), INVALID, b"L_pad=128 must be at least T=130"),                                    # L_pad < T
    (dict(L_pad=200), INVALID, b"a multiple of 128"),
    (dict(ldvt=248), INVALID, b"ldvt=248 must be at least L_pad=256"),                                  # ldvt < L_pad
    (dict(ldvt=260), INVALID, b"ldvt=260"),
    (dict(qkv=P[0] + 8), INVALID, b"16-byte aligned"),                                                  # a misaligned pointer
    (dict(freqs=P[3] + 8), INVALID, b"16-byte aligned"),
    (dict(vt=P[4] + 2), INVALID, b"16-byte aligned"),
    (dict(rstd=P[5] + 2), INVALID, b"4-byte aligned"),
    (dict(dtype=-1), INVALID, b"unknown dtype -1"),
    (dict(eps=float("inf")), INVALID, b"eps must be finite"),
    (dict(head_dim=64), UNSUPPORTED, b"head_dim=64"),
]


def test_exported_and_every_validation_error_is_returned_without_a_launch(built_lib):
    raw = C.CDLL(built_lib)
    assert hasattr(raw, "svdq_sandwich_norm") and hasattr(raw, "svdq_qk_norm_rope")
    lib = _lib.load()
    assert lib.svdq_abi_version() == 24
    for fn, make, refused in ((lib.svdq_sandwich_norm, _sandwich, SANDWICH_REFUSED), (lib.svdq_qk_norm_rope, _qk, QK_REFUSED)):
        assert fn(None, None) == INVALID and b"args is NULL" in lib.svdq_last_error()      # a NULL struct
        for over, want, needle in refused:
            rc = fn(C.byref(make(**over)), None)
            msg = lib.svdq_last_error()
            assert rc == want and needle in msg, f"{over}: returned {rc}, {msg!r}"
    # without vt neither L_pad nor ldvt is looked at: the next complaint is the one planted behind them
    rc = lib.svdq_qk_norm_rope(C.byref(_qk(vt=None, L_pad=0, ldvt=0, dtype=9)), None)
    assert rc == INVALID and b"unknown dtype 9" in lib.svdq_last_error()


def test_wrappers_refuse_mismatched_arguments_and_cpu_tensors(built_lib):
    from nunchaku_amd import ops
    from nunchaku_amd.ops.attention import qk_norm_rope
    from nunchaku_amd.ops.elementwise import sandwich_norm

    assert ops.sandwich_norm is sandwich_norm and ops.qk_norm_rope is qk_norm_rope
    x = torch.zeros(2, 5, 256, dtype=torch.bfloat16)
    w = torch.ones(256, dtype=torch.bfloat16)
    g = torch.ones(2, 256, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="res must be a GPU tensor"):
        sandwich_norm(x, x, w_post=w, w_pre=w)
    with pytest.raises(ValueError, match="nothing to do"):
        sandwich_norm(x)
    with pytest.raises(ValueError, match="a gate needs a"):
        sandwich_norm(x, gate=g, w_pre=w)
    with pytest.raises(ValueError, match="a needs w_post"):
        sandwich_norm(x, x)
    with pytest.raises(ValueError, match="out_mod needs w_pre"):
        sandwich_norm(x, out_mod=True)
    with pytest.raises(ValueError, match="scale needs out_mod"):
        sandwich_norm(x, x, w_post=w, scale=g)
    with pytest.raises(TypeError, match="bfloat16 or float16"):
        sandwich_norm(x.float(), w_pre=w)
    with pytest.raises(TypeError, match="a must be a torch.bfloat16 tensor"):
        sandwich_norm(x, x.half(), w_post=w)
    with pytest.raises(ValueError, match=r"a must be \[2, 5, 256\]"):
        sandwich_norm(x, x[:, :4], w_post=w)
    with pytest.raises(ValueError, match=r"gate must be a torch.bfloat16 \[2, 256\]"):
        sandwich_norm(x, x, w_post=w, gate=g[:1])
    with pytest.raises(ValueError, match=r"w_pre must be a contiguous torch.bfloat16 \[256\]"):
        sandwich_norm(x, w_pre=w[:128])
    with pytest.raises(ValueError, match="a multiple of 8"):
        sandwich_norm(x[..., :12], w_pre=w[:12])
    qkv = torch.zeros(128, 3 * 2 * 128, dtype=torch.float16)
    n = torch.ones(128, dtype=torch.float16)
    with pytest.raises(ValueError, match="qkv must be a GPU tensor"):
        qk_norm_rope(qkv, 2, 100, norm_q=n, norm_k=n)
    with pytest.raises(NotImplementedError, match="head_dim 128 is implemented"):
        qk_norm_rope(qkv, 3)
    with pytest.raises(ValueError, match="tokens=129"):
        qk_norm_rope(qkv, 2, 129)
    with pytest.raises(ValueError, match=r"norm_q must be a torch.float16 \[128\]"):
        qk_norm_rope(qkv, 2, norm_q=n.bfloat16())
    with pytest.raises(ValueError, match="freqs_cis must be complex64"):
        qk_norm_rope(qkv, 2, 100, freqs_cis=torch.zeros(99, 64, dtype=torch.complex64))
    with pytest.raises(ValueError, match=r"vt must be a torch.float16 \[256, >= 128\]"):
        qk_norm_rope(qkv, 2, 100, vt=torch.zeros(256, 64, dtype=torch.float16))
    with pytest.raises(ValueError, match="not a multiple of 128"):
        qk_norm_rope(qkv[:100], 2, vt=torch.zeros(256, 128, dtype=torch.float16))
    with pytest.raises(TypeError, match="bfloat16 or float16"):
        qk_norm_rope(qkv.float(), 2)


# ---- the CPU restatements against the torch-op sequences ------------------------------------------------------------------------------
def _vals(shape, dtype, g, scale=1.0):
    return (torch.randn(shape, generator=g) * scale).to(Z.TD[dtype])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C_", [256, 520, 3840])
def test_sandwich_restatement_equals_the_torch_op_sequence(C_, dtype):
    B, T = 2, 5
    g = torch.Generator().manual_seed(C_)
    res, a = _vals((B, T, C_), dtype, g), _vals((B, T, C_), dtype, g, 3.0)
    w_post, w_pre = (1 + _vals((C_,), dtype, g, 0.2).float()).to(Z.TD[dtype]), (1 + _vals((C_,), dtype, g, 0.2).float()).to(Z.TD[dtype])
    gate, scale = _vals((B, C_), dtype, g).tanh(), 1.0 + _vals((B, C_), dtype, g, 0.3)
    f = lambda t: None if t is None else t.float()
    for use_a in (True, False):
        for use_gate in ((True, False) if use_a else (False,)):
            for use_scale in (True, False):
                kw = dict(w_post=w_post if use_a else None, gate=gate if use_gate else None, w_pre=w_pre, scale=scale if use_scale else None)
                y, m = Z.torch_sandwich(res, a if use_a else None, **kw)
                assert y.dtype == Z.TD[dtype] and m.dtype == Z.TD[dtype]
                ry, rm = Z.sandwich_ref(f(res), f(a) if use_a else None, **{k: f(v) for k, v in kw.items()},
                                        rstd_a=Z.torch_rstd(a) if use_a else None, rstd_y=Z.torch_rstd(y), dtype=dtype)
                what = f"C={C_} {dtype} a={use_a} gate={use_gate} scale={use_scale}"
                assert torch.equal(ry, y.float()), what
                assert torch.equal(rm, m.float()), what
    # a pass that only closes: no w_pre, no out_mod
    y, m = Z.torch_sandwich(res, a, w_post=w_post, gate=gate)
    ry, rm = Z.sandwich_ref(f(res), f(a), w_post=f(w_post), gate=f(gate), rstd_a=Z.torch_rstd(a), dtype=dtype)
    assert m is None and rm is None and torch.equal(ry, y.float())
    # torch's rstd is within the kernel tests' bound of the float64 one
    assert ((Z.torch_rstd(a).double() - Z.rstd64(a)).abs() / Z.rstd64(a)).max().item() <= (8 * -(-C_ // 512) + 12) * 2.0 ** -24


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T,H", [(1, 1), (65, 3), (130, 3)])
def test_qk_restatement_equals_the_torch_op_sequence(T, H, dtype):
    g = torch.Generator().manual_seed(T * 7 + H)
    x = _vals((1, T, H, 128), dtype, g, 2.0)
    w = (1 + _vals((128,), dtype, g, 0.2).float()).to(Z.TD[dtype])
    ang = torch.rand(1, T, 64, generator=g) * 6.2831853
    fc = torch.polar(torch.ones_like(ang), ang)
    assert fc.dtype == torch.complex64
    fr = torch.view_as_real(fc)[0]
    for use_w in (True, False):
        for use_f in (True, False):
            want = Z.torch_qk(x, w if use_w else None, fc if use_f else None)
            assert want.dtype == Z.TD[dtype]
            got = Z.qk_ref(x[0].float(), w.float() if use_w else None, Z.torch_rstd(x)[0] if use_w else None, fr if use_f else None, dtype)
            assert torch.equal(got, want[0].float()), f"T={T} H={H} {dtype} norm={use_w} rope={use_f}"
    # the two rotations the GPU test uses as fixed points
    n = Z.qk_ref(x[0].float(), w.float(), Z.torch_rstd(x)[0], None, dtype)
    one, zero = torch.ones(T, 64), torch.zeros(T, 64)
    assert torch.equal(Z.qk_ref(x[0].float(), w.float(), Z.torch_rstd(x)[0], torch.stack([one, zero], -1), dtype), n)
    quarter = Z.qk_ref(x[0].float(), w.float(), Z.torch_rstd(x)[0], torch.stack([zero, one], -1), dtype)
    assert torch.equal(quarter[..., 0::2], -n[..., 1::2]) and torch.equal(quarter[..., 1::2], n[..., 0::2])


# ---- the modules ----------------------------------------------------------------------------------------------------------------------
def test_block_names_and_shapes_and_the_mirrors_resolve():
    import nunchaku
    from nunchaku.models.attention_processors.zimage import NunchakuZSingleStreamAttnProcessor as MirroredProcessor
    from nunchaku.models.transformers import NunchakuZImageTransformer2DModel as FromTransformers
    from nunchaku.models.transformers.transformer_zimage import (NunchakuZImageAttention, NunchakuZImageFeedForward,
                                                                NunchakuZImageTransformer2DModel)
    from nunchaku_amd.models import zimage
    from nunchaku_amd.models.linear import SVDQW4A4Linear

    assert nunchaku.NunchakuZImageTransformer2DModel is FromTransformers is NunchakuZImageTransformer2DModel is zimage.NunchakuZImageTransformer2DModel
    assert "NunchakuZImageTransformer2DModel" in nunchaku.__all__ and "Z-Image is not part" not in nunchaku.__doc__
    assert MirroredProcessor is zimage.NunchakuZSingleStreamAttnProcessor and NunchakuZImageAttention is zimage.NunchakuZImageAttention
    dim, heads, hidden = 256, 2, 512
    blk = zimage.NunchakuZImageTransformerBlock(dim, heads, hidden, device="meta")
    assert [n for n, _ in blk.named_children()] == ["attention", "feed_forward", "attention_norm1", "ffn_norm1", "attention_norm2", "ffn_norm2",
                                                    "adaLN_modulation"]
    a = blk.attention
    assert [n for n, _ in a.named_children()] == ["norm_q", "norm_k", "to_qkv", "to_out"] and a.heads == heads
    assert type(a.norm_q) is torch.nn.RMSNorm and a.norm_q.eps == 1e-5 and tuple(a.norm_k.weight.shape) == (128,)
    assert isinstance(a.to_qkv, SVDQW4A4Linear) and (a.to_qkv.in_features, a.to_qkv.out_features, a.to_qkv.bias) == (dim, 3 * dim, None)
    assert isinstance(a.to_out, torch.nn.ModuleList) and isinstance(a.to_out[0], SVDQW4A4Linear) and a.to_out[0].bias is None
    assert type(a.to_out[1]) is torch.nn.Dropout and isinstance(a.processor, zimage.NunchakuZSingleStreamAttnProcessor)
    with pytest.raises(ValueError, match="Processor nunchaku-fp16 is not supported"):
        a.set_processor("nunchaku-fp16")
    ff = blk.feed_forward
    assert isinstance(ff, NunchakuZImageFeedForward) and isinstance(ff.net, torch.nn.ModuleList) and len(ff.net) == 3
    assert isinstance(ff.net[0].proj, SVDQW4A4Linear) and (ff.net[0].proj.in_features, ff.net[0].proj.out_features, ff.net[0].proj.bias) == (dim, 2 * hidden, None)
    assert type(ff.net[1]) is torch.nn.Dropout and (ff.net[2].in_features, ff.net[2].out_features, ff.net[2].bias) == (hidden, dim, None)
    for n in (blk.attention_norm1, blk.attention_norm2, blk.ffn_norm1, blk.ffn_norm2):
        assert type(n) is torch.nn.RMSNorm and n.eps == 1e-5 and tuple(n.weight.shape) == (dim,)
    assert type(blk.adaLN_modulation[0]) is torch.nn.Linear and tuple(blk.adaLN_modulation[0].weight.shape) == (4 * dim, 256)
    shapes = {k: tuple(v.shape) for k, v in blk.state_dict().items()}
    lin = lambda p, i, o, r=32: {f"{p}.qweight": (o, i // 2), f"{p}.wscales": (i // 64, o), f"{p}.smooth_factor": (i,), f"{p}.smooth_factor_orig": (i,),
                                 f"{p}.proj_down": (i, r), f"{p}.proj_up": (o, r)}
    want = {"attention.norm_q.weight": (128,), "attention.norm_k.weight": (128,), "attention_norm1.weight": (dim,), "attention_norm2.weight": (dim,),
            "ffn_norm1.weight": (dim,), "ffn_norm2.weight": (dim,), "adaLN_modulation.0.weight": (4 * dim, 256), "adaLN_modulation.0.bias": (4 * dim,),
            **lin("attention.to_qkv", dim, 3 * dim), **lin("attention.to_out.0", dim, dim), **lin("feed_forward.net.0.proj", dim, 2 * hidden),
            **lin("feed_forward.net.2", hidden, dim)}
    assert shapes == want
    plain = zimage.NunchakuZImageTransformerBlock(dim, heads, hidden, modulation=False, rank=64, torch_dtype=torch.float16, device="meta")
    assert not hasattr(plain, "adaLN_modulation") and tuple(plain.feed_forward.net[2].proj_down.shape) == (hidden, 64)
    assert plain.attention_norm1.weight.dtype == torch.float16 and plain.modulate(None) == (None, None, None, None)
    with pytest.raises(ValueError, match="needs adaln_input"):
        blk.modulate(None)
    with pytest.raises(ValueError, match="not heads=3"):
        zimage.NunchakuZImageAttention(256, 3, device="meta")
    for precision in ("fp4", "nvfp4"):
        with pytest.raises(NotImplementedError, match="NVFP4"):
            zimage.NunchakuZImageTransformerBlock(dim, heads, hidden, precision=precision, device="meta")


def test_masks_other_than_a_leading_key_padding_mask_are_refused():
    from nunchaku_amd.models.zimage import valid_token_counts

    m = torch.tensor([[True, True, True, False], [True, True, True, True]])
    assert valid_token_counts(None, 2, 4) == [4, 4] and valid_token_counts(m, 2, 4) == [3, 4]
    for bad in (m.float(), m[:, None, None, :], m[:1], torch.tensor([[True, False, True, False], [True, True, True, True]])):
        with pytest.raises(NotImplementedError, match="attention_mask|come first"):
            valid_token_counts(bad, 2, 4)
    with pytest.raises(ValueError, match="without real tokens"):
        valid_token_counts(torch.tensor([[False, False], [True, True]]), 2, 2)


DIM, HEADS, HIDDEN, RANK = 256, 2, 512, 16
COUNTS = {"noise_refiner": 1, "context_refiner": 1, "layers": 2}


def _fill_(module, seed=0):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in module.parameters():
            p.copy_(torch.randint(-100, 100, p.shape, generator=g) if p.dtype in (torch.int8, torch.int32) else torch.randn(p.shape, generator=g))
    return module


def _tiny_checkpoint(path, skip_refiners=False, dtype=torch.bfloat16):
    """quantised blocks under the module paths and key names of a Z-Image checkpoint (context_refiner without modulation), the refiners in
    diffusers' own 16-bit names when ``skip_refiners``, plus two tensors that belong to the rest of the transformer"""
    from safetensors.torch import save_file

    from nunchaku_amd.models.zimage import NunchakuZImageTransformerBlock

    blocks, sd = {}, {}
    for s, (stack, n) in enumerate(COUNTS.items()):
        for i in range(n):
            pre = f"{stack}.{i}"
            if skip_refiners and stack != "layers":
                for k, shape in (("attention.to_q.weight", (DIM, DIM)), ("feed_forward.net.0.proj.weight", (2 * HIDDEN, DIM)), ("attention_norm1.weight", (DIM,))):
                    sd[f"{pre}.{k}"] = torch.zeros(shape, dtype=dtype)
                continue
            blocks[pre] = _fill_(NunchakuZImageTransformerBlock(DIM, HEADS, HIDDEN, modulation=stack != "context_refiner", rank=RANK, torch_dtype=dtype),
                                 seed=10 * s + i)
            for k, v in blocks[pre].state_dict().items():
                sd[f"{pre}.{k}"] = v.contiguous()
    g = torch.Generator().manual_seed(99)
    sd["cap_embedder.1.weight"] = torch.randn(DIM, 64, generator=g).to(dtype)
    sd["x_pad_token"] = torch.randn(1, DIM, generator=g).to(dtype)
    qcfg = {"rank": RANK, "skip_refiners": True} if skip_refiners else {"rank": RANK}
    save_file(sd, path, metadata={"config": json.dumps(dict(dim=DIM, n_heads=HEADS, n_layers=2, norm_eps=1e-5)), "quantization_config": json.dumps(qcfg)})
    return blocks, sd


def test_diffusers_free_build_loads_the_blocks_and_refuses_forward_fp4_and_offload(tmp_path):
    from nunchaku_amd.models import zimage

    if zimage.HAVE_DIFFUSERS:
        return  # the real subclass is the one in use
    cls = zimage.NunchakuZImageTransformer2DModel
    assert issubclass(cls, torch.nn.Module)
    path = str(tmp_path / "tiny.safetensors")
    blocks, sd = _tiny_checkpoint(path)
    m = cls.from_pretrained(path, device="cpu")
    assert m.dtype == torch.bfloat16 and m.device.type == "cpu" and m.config.dim == DIM
    assert m.block_names == ["noise_refiner.0", "context_refiner.0", "layers.0", "layers.1"]
    for pre, src in blocks.items():
        blk = m.get_submodule(pre)
        assert isinstance(blk, zimage.NunchakuZImageTransformerBlock) and blk.attention.heads == HEADS and blk.attention.to_qkv.rank == RANK
        assert blk.modulation == (not pre.startswith("context_refiner"))
        a, b = src.state_dict(), blk.state_dict()
        assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)
    assert set(m.state_dict()) == {k for k in sd if k.split(".")[0] in COUNTS}                      # strict=True: every key, no others
    assert set(m.unquantized_state_dict) == {"cap_embedder.1.weight", "x_pad_token"}
    assert torch.equal(m.unquantized_state_dict["x_pad_token"], sd["x_pad_token"])
    assert isinstance(m.stack("layers"), zimage.ZImageBlockStack) and len(m.stack("layers").blocks) == 2 and len(m.stack("noise_refiner").blocks) == 1
    with pytest.raises(RuntimeError, match="diffusers"):
        m(torch.zeros(1, 16, 8, 8), torch.zeros(1), torch.zeros(1, 5, 64))
    for precision in ("fp4", "nvfp4"):
        with pytest.raises(NotImplementedError, match="NVFP4"):
            cls.from_pretrained(path, device="cpu", precision=precision)
    with pytest.raises(NotImplementedError, match="Offload is not supported"):
        cls.from_pretrained(path, device="cpu", offload=True)
    with pytest.raises(ValueError, match="Only safetensors are supported"):
        cls.from_pretrained(str(tmp_path / "tiny.bin"), device="cpu")
    assert cls.from_pretrained(path, device="cpu", torch_dtype=torch.float16).dtype == torch.float16
    # skip_refiners: only `layers` is quantised, the refiners' 16-bit tensors stay with the rest
    path2 = str(tmp_path / "skip.safetensors")
    blocks2, sd2 = _tiny_checkpoint(path2, skip_refiners=True)
    m2 = cls.from_pretrained(path2, device="cpu")
    assert m2.block_names == ["layers.0", "layers.1"] and not hasattr(m2, "noise_refiner")
    assert {"noise_refiner.0.attention.to_q.weight", "context_refiner.0.feed_forward.net.0.proj.weight", "x_pad_token"} <= set(m2.unquantized_state_dict)
    with pytest.raises(KeyError, match="noise_refiner"):
        m2.stack("noise_refiner")
    # a checkpoint that lacks a tensor of a block does not load
    from safetensors.torch import save_file

    broken = {k: v for k, v in sd.items() if k != "layers.1.ffn_norm2.weight"}
    path3 = str(tmp_path / "broken.safetensors")
    save_file(broken, path3, metadata={"config": "{}", "quantization_config": json.dumps({"rank": RANK})})
    with pytest.raises(KeyError, match="layers.1.ffn_norm2.weight"):
        cls.from_pretrained(path3, device="cpu")


FAKE_DIFFUSERS = {
    "__init__.py": "",
    "models/__init__.py": "",
    "models/transformers/__init__.py": "",
    "models/transformers/transformer_z_image.py": '''
        import inspect
        import torch
        from torch import nn

        class FrozenDict(dict):
            def __getattr__(self, k):
                try: return self[k]
                except KeyError: raise AttributeError(k)

        class Attention(nn.Module):
            def __init__(self, dim, heads):
                super().__init__()
                self.inner_dim = self.query_dim = self.out_dim = dim
                self.use_bias, self.dropout, self.heads, self.rescale_output_factor, self.is_cross_attention = False, 0.0, heads, 1.0, False
                self.norm_q, self.norm_k = nn.RMSNorm(dim // heads, eps=1e-5), nn.RMSNorm(dim // heads, eps=1e-5)
                self.to_q, self.to_k, self.to_v = (nn.Linear(dim, dim, bias=False) for _ in range(3))
                self.to_out = nn.ModuleList([nn.Linear(dim, dim, bias=False), nn.Dropout(0.0)])

        class FeedForward(nn.Module):
            def __init__(self, dim, hidden):
                super().__init__()
                self.w1, self.w2, self.w3 = nn.Linear(dim, hidden, bias=False), nn.Linear(hidden, dim, bias=False), nn.Linear(dim, hidden, bias=False)

        class ZImageTransformerBlock(nn.Module):
            def __init__(self, dim, n_heads, hidden, norm_eps, modulation=True):
                super().__init__()
                self.attention, self.feed_forward = Attention(dim, n_heads), FeedForward(dim, hidden)
                self.attention_norm1, self.ffn_norm1 = nn.RMSNorm(dim, eps=norm_eps), nn.RMSNorm(dim, eps=norm_eps)
                self.attention_norm2, self.ffn_norm2 = nn.RMSNorm(dim, eps=norm_eps), nn.RMSNorm(dim, eps=norm_eps)
                self.modulation = modulation
                if modulation:
                    self.adaLN_modulation = nn.Sequential(nn.Linear(min(dim, 256), 4 * dim, bias=True))

        class ZImageTransformer2DModel(nn.Module):
            """the shape of diffusers' class that matters here: config registration, from_config, the three stacks of full-size blocks"""
            def __init__(self, dim=3840, n_heads=30, n_layers=30, n_refiner_layers=2, hidden=10240, norm_eps=1e-5, cap_feat_dim=2560):
                super().__init__()
                self.config = FrozenDict(dim=dim, n_heads=n_heads, n_layers=n_layers, n_refiner_layers=n_refiner_layers, hidden=hidden, norm_eps=norm_eps)
                blk = lambda mod: ZImageTransformerBlock(dim, n_heads, hidden, norm_eps, modulation=mod)
                self.noise_refiner = nn.ModuleList([blk(True) for _ in range(n_refiner_layers)])
                self.context_refiner = nn.ModuleList([blk(False) for _ in range(n_refiner_layers)])
                self.layers = nn.ModuleList([blk(True) for _ in range(n_layers)])
                self.cap_embedder = nn.Sequential(nn.RMSNorm(cap_feat_dim), nn.Linear(cap_feat_dim, dim, bias=False))
                self.x_pad_token = nn.Parameter(torch.empty(1, dim))

            @classmethod
            def from_config(cls, config):
                expected = set(inspect.signature(cls.__init__).parameters) - {"self"}
                return cls(**{k: v for k, v in config.items() if k in expected})

            @property
            def dtype(self):
                return self.x_pad_token.dtype
        ''',
}

DIFFUSERS_SCRIPT = '''
import json, sys, torch
sys.path.insert(0, sys.argv[2])
from diffusers.models.transformers import transformer_z_image as dz
from safetensors.torch import save_file
from nunchaku_amd.models import zimage
from nunchaku_amd.models.linear import SVDQW4A4Linear
assert zimage.HAVE_DIFFUSERS
cls = zimage.NunchakuZImageTransformer2DModel
assert issubclass(cls, dz.ZImageTransformer2DModel) and issubclass(cls, zimage.NunchakuModelLoaderMixin)
CONFIG = dict(dim=256, n_heads=2, n_layers=2, n_refiner_layers=1, hidden=512, cap_feat_dim=64)
for skip in (False, True):
    # the checkpoint: the state dict of a model patched the same way, filled with random values
    src = cls.from_config(CONFIG).to(torch.bfloat16)._patch_model(skip_refiners=skip, rank=16)
    g = torch.Generator().manual_seed(int(skip))
    sd = {k: (torch.randint(-100, 100, v.shape, generator=g).to(v.dtype) if v.dtype == torch.int8 else torch.randn(v.shape, generator=g).to(v.dtype))
          for k, v in src.state_dict().items()}
    assert "layers.1.feed_forward.net.0.proj.qweight" in sd and "context_refiner.0.attention_norm1.weight" in sd
    assert ("noise_refiner.0.feed_forward.net.0.proj.weight" in sd and "noise_refiner.0.attention.to_q.weight" in sd) == skip
    path = sys.argv[1] + str(int(skip)) + ".safetensors"
    save_file(sd, path, metadata={"config": json.dumps(CONFIG), "quantization_config": json.dumps({"rank": 16, "skip_refiners": skip})})
    m = cls.from_pretrained(path, device="cpu")
    assert isinstance(m, dz.ZImageTransformer2DModel) and m.config.dim == 256 and m.dtype == torch.bfloat16
    assert not any(p.is_meta for p in m.parameters()), "a meta-device parameter of the diffusers skeleton survived"
    assert set(m.state_dict()) == set(sd) and all(torch.equal(v, m.state_dict()[k]) for k, v in sd.items())
    for name, stack in (("layers", m.layers), ("noise_refiner", m.noise_refiner), ("context_refiner", m.context_refiner)):
        for blk in stack:
            assert type(blk) is dz.ZImageTransformerBlock                      # diffusers' block, its attention and feed-forward swapped
            if skip and name != "layers":
                assert type(blk.attention) is dz.Attention and type(blk.feed_forward) is zimage.ZImageSwiGLUFeedForward
                assert type(blk.feed_forward.net[0].proj) is torch.nn.Linear and tuple(blk.feed_forward.net[0].proj.weight.shape) == (1024, 256)
            else:
                assert type(blk.attention) is zimage.NunchakuZImageAttention and type(blk.feed_forward) is zimage.NunchakuZImageFeedForward
                assert blk.attention.to_qkv.rank == 16 and blk.attention.heads == 2 and isinstance(blk.feed_forward.net[2], SVDQW4A4Linear)
                assert blk.attention.norm_q.weight.shape == (128,) and not hasattr(blk.attention, "to_q")
    assert not hasattr(m, "unquantized_state_dict")
    for kw in (dict(precision="fp4"), dict(offload=True)):
        try:
            cls.from_pretrained(path, device="cpu", **kw)
            raise SystemExit(f"{kw} was not refused")
        except NotImplementedError:
            pass
print("OK")
'''


def test_real_subclass_build_against_a_stand_in_diffusers(tmp_path):
    import sys
    import textwrap

    for name, text in FAKE_DIFFUSERS.items():
        f = tmp_path / "diffusers" / name
        f.parent.mkdir(parents=True, exist_ok=True)
        f.write_text(textwrap.dedent(text))
    script = tmp_path / "run.py"
    script.write_text(textwrap.dedent(DIFFUSERS_SCRIPT))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([str(tmp_path), ROOT, os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, str(script), str(tmp_path / "tiny"), ROOT], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr
