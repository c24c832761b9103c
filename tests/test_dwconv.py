"""SANA's depthwise 3x3 convolution and GLU-MBConv, the parts that need no GPU: the C ABI (header, bindings, exported symbol, validation without a
launch), the CPU restatements the GPU tests compare against (tests/dwconv_ref.py), the op wrapper's checks and the module's names and shapes."""

import ctypes as C
import json
import os
import re
import subprocess

import pytest
import torch
import torch.nn.functional as F

from nunchaku_amd import _lib
from nunchaku_amd import build as svdq_build
from tests.dwconv_ref import abs_terms, dwconv_16bit, dwconv_ref32, dwconv_ref64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TD = {"bf16": torch.bfloat16, "fp16": torch.float16}
HALF_ULP = {"bf16": -9, "fp16": -12}


def half_ulp(v, dtype):
    """half a unit in the last place of the 16-bit format at |v| (normal numbers): with |v| = m * 2^e, 0.5 <= m < 1, the format's 8 (bf16) or 11
    (fp16) significant bits end at 2^(e - 8) / 2^(e - 11), so half of that is 2^-9 / 2^-12 times 2^e -- |v| rounded up to a power of two.
    (2^-9 * |v| itself, without the rounding up, is what a correctly rounded value just above a power of two misses by up to a factor 2.)"""
    _, e = torch.frexp(v.abs())
    return torch.ldexp(torch.ones_like(v), e + HALF_ULP[dtype])


# ---- C ABI --------------------------------------------------------------------------------------------------------------------------
def test_header_bindings_and_sources_agree_and_the_abi_version_stays():
    text = open(os.path.join(ROOT, "include", "svdq_amd.h")).read()
    assert re.search(r"^int svdq_dwconv3x3\(const svdq_dwconv3x3_args \*args, void \*stream\);", text, re.M)
    assert re.search(r"^} svdq_dwconv3x3_args;", text, re.M)
    assert re.search(r"^#define SVDQ_ABI_VERSION 24$", text, re.M)
    assert _lib.ABI_VERSION == 24
    assert "svdq_dwconv3x3" in _lib.EXPORTS and _lib.EXPORTS["svdq_dwconv3x3"] == (C.c_int, [C.POINTER(_lib.Dwconv3x3Args), C.c_void_p])
    assert "dwconv.hip" in svdq_build.SOURCES and os.path.exists(os.path.join(svdq_build.CSRC, "dwconv.hip"))


def test_struct_layout_matches_header(built_lib, tmp_path):
    cname, cls = "svdq_dwconv3x3_args", _lib.Dwconv3x3Args
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


B, H, W, CH = 2, 5, 6, 16
LD = 24


def _args(**over):
    """a call that would pass validation (the pointers are made up: no test below lets it reach a launch)"""
    a = _lib.Dwconv3x3Args()
    a.x, a.weight, a.bias, a.out = 0x100000, 0x20000, 0x30000, 0x200000
    a.B, a.H, a.W, a.C, a.dtype = B, H, W, CH, _lib.SVDQ_BF16
    a.ldx, a.ldo = LD, CH
    a.x_bs, a.out_bs = H * W * LD + 8, H * W * CH
    for k, v in over.items():
        setattr(a, k, v)
    return a


X_BYTES = 2 * ((B - 1) * (H * W * LD + 8) + (H * W - 1) * LD + CH)  # the span of x in bytes
REFUSED = [
    (dict(x=None), b"x, weight and out are required"),
    (dict(weight=None), b"x, weight and out are required"),
    (dict(out=None), b"x, weight and out are required"),
    (dict(B=0), b"B=0"),
    (dict(H=0), b"H=0"),
    (dict(W=-1), b"W=-1"),
    (dict(C=0), b"C=0"),
    (dict(C=12, ldx=16, ldo=16), b"C=12 must be a multiple of 8"),
    (dict(ldx=CH - 8), b"row strides"),
    (dict(ldo=CH - 8), b"row strides"),
    (dict(ldx=LD + 4), b"row strides"),
    (dict(ldo=CH + 2), b"row strides"),
    (dict(x_bs=H * W * LD - 8), b"batch strides"),
    (dict(out_bs=0), b"batch strides"),
    (dict(out_bs=H * W * CH + 4), b"batch strides"),
    (dict(x=0x100000 + 8), b"16-byte aligned"),
    (dict(weight=0x20000 + 2), b"16-byte aligned"),
    (dict(bias=0x30000 + 4), b"16-byte aligned"),
    (dict(out=0x200000 + 8), b"16-byte aligned"),
    (dict(dtype=7), b"unknown dtype 7"),
    (dict(out=0x100000), b"overlap"),                        # in place
    (dict(out=0x100000 + X_BYTES - 16), b"overlap"),          # the last piece of x
    (dict(out=0x100000 - 2 * (B * H * W * CH) + 16), b"overlap"),  # out ends inside x
    (dict(B=65536, out=0x7f0000000000), b"exceeds the grid"),
]


def test_exported_and_every_validation_error_is_returned_without_a_launch(built_lib):
    raw = C.CDLL(built_lib)
    assert hasattr(raw, "svdq_dwconv3x3")
    lib = _lib.load()
    assert lib.svdq_abi_version() == 24
    assert lib.svdq_dwconv3x3(None, None) == 1 and b"NULL" in lib.svdq_last_error()
    for over, needle in REFUSED:
        rc = lib.svdq_dwconv3x3(C.byref(_args(**over)), None)
        msg = lib.svdq_last_error()
        assert rc == 1 and needle in msg, f"{over}: returned {rc}, {msg!r}"
    # a tile count beyond the grid: 2^16 x 2^16 pixels of 2^15 channels are 2^14 * 2^13 * 2^6 tiles
    rc = lib.svdq_dwconv3x3(C.byref(_args(B=1, H=1 << 16, W=1 << 16, C=1 << 15, ldx=1 << 15, ldo=1 << 15)), None)
    assert rc == 1 and b"exceeds the grid" in lib.svdq_last_error()


# ---- the CPU restatements -----------------------------------------------------------------------------------------------------------
def _random_case(shape, dtype, seed, bias=True):
    """inputs inside the normal range: |x| and |w| in [2^-6, 2^3], random signs"""
    Bq, Hq, Wq, Cq = shape
    g = torch.Generator().manual_seed(seed)

    def mag(*s):
        return (torch.exp2(torch.rand(*s, generator=g) * 9 - 6) * torch.sign(torch.randn(*s, generator=g))).to(TD[dtype])

    return mag(Bq, Hq, Wq, Cq), mag(Cq, 3, 3, 1), mag(Cq) if bias else None


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("bias", [True, False])
def test_ref32_is_within_the_derived_bound_of_ref64(dtype, bias):
    """|ref32 - ref64| <= half_ulp(|ref64|) + 10 * 2^-24 * (|bias| + sum |w x|): the final rounding plus ten fp32 additions at first order"""
    x, w, b = _random_case((2, 7, 9, 24), dtype, 11, bias)
    r32, r64 = dwconv_ref32(x, w, b), dwconv_ref64(x, w, b)
    assert r32.dtype == TD[dtype] and r64.dtype == torch.float64 and r32.shape == x.shape
    bound = half_ulp(r64, dtype) + 10 * 2.0 ** -24 * abs_terms(x, w, b)
    err = (r32.double() - r64).abs()
    assert (err <= bound).all(), f"worst error / bound {(err / bound).max().item():.3g}"
    assert (err > 0).any()  # (the inputs are not a case where nothing rounds)
    e16 = (dwconv_16bit(x, w, b).double() - r64).abs().max().item()
    print(f"{dtype}: max error of one rounding {err.max().item():.3g}, of a rounding per tap {e16:.3g}")
    assert e16 >= err.max().item()


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_ref_has_the_orientation_and_padding_of_conv2d(dtype):
    """cross-correlation, not convolution: equal to F.conv2d(groups=C, padding=1) in float64 on the NCHW view; an asymmetric kernel and a
    non-square image make a flipped or transposed restatement fail"""
    x, w, b = _random_case((2, 5, 8, 16), dtype, 5)
    want = F.conv2d(x.double().permute(0, 3, 1, 2), w.double().reshape(16, 1, 3, 3), b.double(), padding=1, groups=16).permute(0, 2, 3, 1)
    got = dwconv_ref64(x, w, b)
    scale = abs_terms(x, w, b)
    assert (got - want).abs().le(16 * 2.0 ** -53 * scale).all()  # (float64 sums in another order)
    flipped = dwconv_ref64(x, w.flip(1, 2), b)
    transposed = dwconv_ref64(x, w.transpose(1, 2), b)
    assert (flipped - want).abs().max() > 1e-3 and (transposed - want).abs().max() > 1e-3


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_integer_inputs_are_exact_in_every_restatement(dtype):
    """x in [-4, 4], w and bias in [-2, 2], integers: every partial sum is an integer below 256: no rounding anywhere"""
    g = torch.Generator().manual_seed(2)
    x = torch.randint(-4, 5, (2, 6, 7, 16), generator=g).to(TD[dtype])
    w = torch.randint(-2, 3, (16, 3, 3, 1), generator=g).to(TD[dtype])
    b = torch.randint(-2, 3, (16,), generator=g).to(TD[dtype])
    r64 = dwconv_ref64(x, w, b)
    assert r64.abs().max() <= 74 and torch.equal(r64, r64.round())
    assert torch.equal(dwconv_ref32(x, w, b).double(), r64) and torch.equal(dwconv_16bit(x, w, b).double(), r64)
    assert torch.equal(dwconv_ref32(x, w).double(), dwconv_ref64(x, w))


# ---- the op wrapper -------------------------------------------------------------------------------------------------------------------
def test_wrapper_refuses_mismatched_arguments_and_cpu_tensors(built_lib):
    from nunchaku_amd.ops import dwconv3x3
    from nunchaku_amd.ops.conv import dwconv3x3 as same, grid_of

    assert dwconv3x3 is same
    x = torch.zeros(2, 12, 16, dtype=torch.bfloat16)
    w, b = torch.zeros(16, 3, 3, 1, dtype=torch.bfloat16), torch.zeros(16, dtype=torch.bfloat16)
    assert grid_of(16) == (4, 4) and grid_of(12, 3) == (3, 4) and grid_of(12, None, 2) == (6, 2) and grid_of(12, 4, 3) == (4, 3)
    assert grid_of(12, 0, 3) == (4, 3) and grid_of(9, -1, -1) == (3, 3)  # (the reference's "not given": <= 0)
    for kw in (dict(), dict(height=5), dict(width=7), dict(height=3, width=5)):  # 12 is no square; 5 and 7 do not divide it; 3 * 5 != 12
        with pytest.raises(ValueError, match="does not hold 12 tokens"):
            dwconv3x3(x, w, b, **kw)
    with pytest.raises(ValueError, match="contradict"):
        dwconv3x3(x.view(2, 3, 4, 16), w, b, height=4, width=3)
    with pytest.raises(ValueError, match="share one 16-bit dtype"):
        dwconv3x3(x, w.half(), b, height=3)
    with pytest.raises(ValueError, match="share one 16-bit dtype"):
        dwconv3x3(x, w, b.float(), height=3)
    with pytest.raises(ValueError, match="share one 16-bit dtype"):
        dwconv3x3(x.float(), w.float(), b.float(), height=3)
    with pytest.raises(ValueError, match="multiple of 8"):
        dwconv3x3(torch.zeros(2, 12, 12, dtype=torch.bfloat16), w[:12], b[:12], height=3)
    for bad in (w.view(16, 9), w.view(16, 1, 3, 3), w[:8], torch.zeros(16, 3, 3, 2, dtype=torch.bfloat16)):
        with pytest.raises(ValueError, match=r"weight must be \[C, 3, 3, 1\]"):
            dwconv3x3(x, bad, b, height=3)
    with pytest.raises(ValueError, match="weight must be"):
        dwconv3x3(x, w, b[:8], height=3)
    with pytest.raises(ValueError, match="out must be"):
        dwconv3x3(x, w, b, height=3, out=torch.zeros(2, 12, 8, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="expected x"):
        dwconv3x3(x[0], w, b)
    with pytest.raises(RuntimeError, match="GPU tensors"):
        dwconv3x3(x, w, b, height=3)


# ---- the module -----------------------------------------------------------------------------------------------------------------------
def test_module_names_shapes_and_padding_match_the_reference_layer(golden_dir):
    from nunchaku.models.sana import SanaGLUMBConv as Mirrored
    from nunchaku_amd.models import SanaDepthwiseConv, SanaGLUMBConv, convert_sana_ff_state_dict
    from nunchaku_amd.models.linear import SVDQW4A4Linear

    assert Mirrored is SanaGLUMBConv
    big = SanaGLUMBConv(2240, 5600, device="meta")          # SANA-1.6B
    assert (big.in_pad, big.c_gemm, big.hid_pad) == (2304, 11264, 5632) and 2 * big.hid_pad == big.c_gemm
    m = SanaGLUMBConv(1152, 2880, device="meta")            # SANA-0.6B: the convolution's channels end 128 columns before the GLU's
    assert (m.in_pad, m.c_gemm, m.hid_pad) == (1152, 5760, 2944) and 2 * m.hid_pad == m.c_gemm + 128
    assert [n for n, _ in m.named_children()] == ["inverted_conv", "depth_conv", "point_conv"]
    assert isinstance(m.inverted_conv, SVDQW4A4Linear) and isinstance(m.point_conv, SVDQW4A4Linear) and isinstance(m.depth_conv, SanaDepthwiseConv)
    assert (m.inverted_conv.in_features, m.inverted_conv.out_features) == (1152, 5760) and m.inverted_conv.bias is not None
    assert (m.point_conv.in_features, m.point_conv.out_features) == (2944, 1152) and m.point_conv.bias is None
    assert tuple(big.depth_conv.weight.shape) == (11264, 3, 3, 1) and tuple(big.depth_conv.bias.shape) == (11264,)
    golden = json.load(open(os.path.join(golden_dir, "sana_ff_keys.json")))
    sd = m.state_dict()
    assert {k: list(v.shape) for k, v in sd.items()} == golden

    legacy = {}
    for k, v in sd.items():
        k = k.replace("proj_down", "lora_down").replace("proj_up", "lora_up").replace("smooth_factor_orig", "smooth_orig").replace("smooth_factor", "smooth")
        legacy[k] = torch.empty(v.shape, dtype=v.dtype)
    assert {"inverted_conv.lora_down", "point_conv.lora_up", "point_conv.smooth", "inverted_conv.smooth_orig", "depth_conv.weight", "depth_conv.bias"} <= set(legacy)
    assert not any(s in k for k in legacy for s in ("proj_down", "proj_up", "smooth_factor"))
    conv = convert_sana_ff_state_dict(legacy)
    assert set(conv) == set(sd) and conv["depth_conv.weight"] is legacy["depth_conv.weight"] and conv["depth_conv.bias"] is legacy["depth_conv.bias"]
    assert convert_sana_ff_state_dict(conv).keys() == conv.keys()  # names that are already converted pass through
    cpu = SanaGLUMBConv(1152, 2880)
    cpu.load_state_dict(conv, strict=True)
    with pytest.raises(RuntimeError):
        cpu.load_state_dict(legacy, strict=True)


def test_forward_rejects_inputs_and_grids_it_cannot_use():
    from nunchaku_amd.models import SanaGLUMBConv

    m = SanaGLUMBConv(256, 384, device="meta")
    x = torch.empty(2, 12, 256, dtype=torch.bfloat16, device="meta")
    with pytest.raises(ValueError, match="expected x"):
        m(x[..., :128])
    with pytest.raises(ValueError, match="does not hold 12 tokens"):
        m(x)
    with pytest.raises(ValueError, match="does not hold 12 tokens"):
        m(x, 5, 2)


def test_linear_keywords_default_to_the_existing_behaviour():
    import inspect

    from nunchaku_amd.models.linear import SVDQW4A4Linear

    q, f = inspect.signature(SVDQW4A4Linear.quantize).parameters, inspect.signature(SVDQW4A4Linear.forward_quant).parameters
    assert q["fuse_glu"].default is False and list(q)[:5] == ["self", "x", "pad_size", "ln", "pool"]
    assert f["fuse_silu"].default is False and list(f)[:5] == ["self", "quantized_x", "ascales", "lora_act", "output"]
    assert callable(SVDQW4A4Linear.forward_silu)
