"""svdq_dwconv3x3 on the GPU: SANA's depthwise 3x3 convolution against the restatements of tests/dwconv_ref.py, and the SanaGLUMBConv module.

The kernel's arithmetic is specified operation by operation (fp32, bias first, nine taps in row-major order, one rounding), so the comparison with
``dwconv_ref32`` is ``torch.equal``: there is no tolerance anywhere in this file.  The kernel's tile is 4 rows x 8 columns x 512 channels: the
shapes end below, on and just beyond each of those edges."""

import functools

import pytest
import torch
import torch.nn.functional as F

from tests.dwconv_ref import dwconv_16bit, dwconv_ref32, dwconv_ref64

pytestmark = pytest.mark.gpu

TD = {"bf16": torch.bfloat16, "fp16": torch.float16}
DTYPES = ["bf16", "fp16"]
SHAPES = [(1, 1, 1, 8), (1, 1, 5, 8), (2, 5, 1, 16), (1, 3, 3, 72), (3, 7, 9, 256), (1, 16, 16, 520), (2, 33, 20, 64), (1, 32, 32, 1288),
          (1, 4, 8, 512), (1, 5, 9, 520)]  # (B, H, W, C); the last two: exactly one tile, and one past it in rows, columns and channels


@functools.lru_cache(maxsize=None)
def _case(B, H, W, C, dtype):
    """x randn with the top-left quarter of the image x 8, weights randn / 3, bias randn -- on the CPU, with the references, computed once"""
    g = torch.Generator().manual_seed(1000003 * B + 10007 * H + 101 * W + C)
    x = torch.randn(B, H, W, C, generator=g)
    x[:, : (H + 1) // 2, : (W + 1) // 2] *= 8.0
    x = x.to(TD[dtype])
    w = (torch.randn(C, 3, 3, 1, generator=g) / 3).to(TD[dtype])
    b = torch.randn(C, generator=g).to(TD[dtype])
    return x, w, b, {True: dwconv_ref32(x, w, b), False: dwconv_ref32(x, w, None)}


@functools.lru_cache(maxsize=None)
def _integer_case(B, H, W, C, dtype):
    g = torch.Generator().manual_seed(7 + H * W + C)
    x = torch.randint(-4, 5, (B, H, W, C), generator=g).to(TD[dtype])
    w = torch.randint(-2, 3, (C, 3, 3, 1), generator=g).to(TD[dtype])
    b = torch.randint(-2, 3, (C,), generator=g).to(TD[dtype])
    return x, w, b, dwconv_ref64(x, w, b)


def _conv(x, w, b=None, **kw):
    from nunchaku_amd.ops.conv import dwconv3x3

    return dwconv3x3(x.cuda(), w.cuda(), None if b is None else b.cuda(), **kw)


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,H,W,C", SHAPES)
def test_bit_equal_to_the_fp32_restatement(B, H, W, C, dtype, bias):
    x, w, b, ref = _case(B, H, W, C, dtype)
    b = b if bias else None
    out = _conv(x, w, b)
    assert out.shape == x.shape and out.dtype == TD[dtype]
    r64 = dwconv_ref64(x, w, b)
    print(f"({B},{H},{W},{C}) {dtype} bias={bias}: max |kernel - ref64| {(out.cpu().double() - r64).abs().max().item():.3g}, "
          f"of the reference's 16-bit accumulator {(dwconv_16bit(x, w, b).double() - r64).abs().max().item():.3g} (max |ref64| {r64.abs().max().item():.3g})")
    assert torch.equal(out.cpu(), ref[bias])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,H,W,C", SHAPES)
def test_integer_inputs_give_the_float64_result(B, H, W, C, dtype):
    x, w, b, r64 = _integer_case(B, H, W, C, dtype)
    assert torch.equal(_conv(x, w, b).cpu().double(), r64)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,H,W,C", SHAPES)
def test_calls_are_bit_equal_and_the_two_input_forms_agree(B, H, W, C, dtype):
    x, w, b, ref = _case(B, H, W, C, dtype)
    x, w, b = x.cuda(), w.cuda(), b.cuda()
    out = _conv(x, w, b)
    assert torch.equal(_conv(x, w, b), out)
    flat = _conv(x.view(B, H * W, C), w, b, height=H, width=W)
    assert flat.shape == (B, H * W, C) and torch.equal(flat.view(B, H, W, C), out)
    assert torch.equal(_conv(x.view(B, H * W, C), w, b, height=H), flat) and torch.equal(_conv(x.view(B, H * W, C), w, b, width=W), flat)
    if H == W:
        assert torch.equal(_conv(x.view(B, H * W, C), w, b), flat)  # a missing pair: the square grid
    elif H > 1 and W > 1:
        swapped = _conv(x.view(B, H * W, C), w, b, height=W, width=H)
        assert not torch.equal(swapped, flat)  # the same tokens on the transposed grid have other neighbours
        assert torch.equal(swapped.cpu(), dwconv_ref32(x.view(B, W, H, C), w, b).view(B, H * W, C))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,H,W,C", SHAPES)
def test_nothing_outside_the_operands_is_read_or_written(B, H, W, C, dtype):
    """x sits in a NaN-filled buffer with a wider row stride, a larger batch stride and extra token rows behind every batch element; out is a
    column slice of a sentinel-filled buffer."""
    x, w, b, ref = _case(B, H, W, C, dtype)
    T = H * W
    big = torch.full((B, T + 5, C + 64), float("nan"), device="cuda", dtype=TD[dtype])
    big[:, :T, :C] = x.view(B, T, C).cuda()
    sentinel = -77.0
    big_o = torch.full((B, T + 3, C + 128), sentinel, device="cuda", dtype=TD[dtype])
    out = big_o[:, :T, 64:64 + C]
    got = _conv(big[:, :T, :C].unflatten(1, (H, W)), w, b, out=out)
    assert got is out and torch.equal(out.cpu().view(B, H, W, C), ref[True])
    assert (big_o[:, T:] == sentinel).all() and (big_o[:, :T, :64] == sentinel).all() and (big_o[:, :T, 64 + C:] == sentinel).all()
    assert torch.isnan(big[:, T:]).all() and torch.isnan(big[:, :, C:]).all() and torch.equal(big[:, :T, :C].cpu(), x.view(B, T, C))


@pytest.mark.parametrize("dtype", DTYPES)
def test_borders_of_an_all_ones_image(dtype):
    """all-ones x and weights, no bias: the output counts the taps inside the image"""
    C = 16
    w = torch.ones(C, 3, 3, 1, dtype=TD[dtype])
    for H, W in ((3, 3), (4, 5), (6, 18), (1, 1), (1, 6), (7, 1), (2, 2)):
        out = _conv(torch.ones(2, H, W, C, dtype=TD[dtype]), w).cpu().float()
        rows = torch.tensor([min(h + 1, H - 1) - max(h - 1, 0) + 1 for h in range(H)], dtype=torch.float32)
        cols = torch.tensor([min(c + 1, W - 1) - max(c - 1, 0) + 1 for c in range(W)], dtype=torch.float32)
        assert torch.equal(out, (rows[:, None] * cols[None, :])[None, :, :, None].expand(2, H, W, C)), (H, W)
        if H >= 3 and W >= 3:
            assert out[0, 0, 0, 0] == 4 and out[0, 0, W - 1, 0] == 4 and out[0, H - 1, 0, 0] == 4 and out[0, H - 1, W - 1, 0] == 4
            assert (out[0, 0, 1:W - 1] == 6).all() and (out[0, 1:H - 1, 0] == 6).all() and (out[0, 1:H - 1, 1:W - 1] == 9).all()
    assert _conv(torch.ones(1, 1, 1, C, dtype=TD[dtype]), w).cpu().float().unique().tolist() == [1.0]
    assert _conv(torch.ones(1, 1, 4, C, dtype=TD[dtype]), w).cpu().float()[0, 0, :, 0].tolist() == [2.0, 3.0, 3.0, 2.0]
    assert _conv(torch.ones(1, 4, 1, C, dtype=TD[dtype]), w).cpu().float()[0, :, 0, 0].tolist() == [2.0, 3.0, 3.0, 2.0]


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_single_pixel_reproduces_the_flipped_footprint(dtype):
    """nine distinct power-of-two weights: a one at (py, px) puts w[ky, kx] at (py + 1 - ky, px + 1 - kx) -- cross-correlation -- wherever that is
    inside the 5 x 6 image"""
    H, W, C = 5, 6, 8
    w = (2.0 ** torch.arange(9.0)).view(1, 3, 3, 1).expand(C, 3, 3, 1).contiguous().to(TD[dtype])
    for py, px in ((0, 0), (0, 5), (4, 0), (4, 5), (0, 2), (2, 0), (4, 3), (2, 5), (2, 3)):
        x = torch.zeros(1, H, W, C, dtype=TD[dtype])
        x[0, py, px] = 1.0
        want = torch.zeros(H, W)
        for ky in range(3):
            for kx in range(3):
                h, c = py + 1 - ky, px + 1 - kx
                if 0 <= h < H and 0 <= c < W:
                    want[h, c] = 2.0 ** (3 * ky + kx)
        out = _conv(x, w).cpu().float()
        assert torch.equal(out, want[None, :, :, None].expand(1, H, W, C)), (py, px)


@pytest.mark.parametrize("dtype", DTYPES)
def test_channels_are_independent(dtype):
    B, H, W, C = 1, 5, 6, 520
    g = torch.Generator().manual_seed(9)
    x, w, b = (torch.randn(*s, generator=g).to(TD[dtype]) for s in ((B, H, W, C), (C, 3, 3, 1), (C,)))
    base = _conv(x, w, b)
    for c in (3, 515):
        for which in range(3):
            x2, w2, b2 = x.clone(), w.clone(), b.clone()
            (x2[..., c], w2[c], b2[c:c + 1])[which].mul_(-2.0).add_(0.5)
            out = _conv(x2, w2, b2)
            others = [i for i in range(C) if i != c]
            assert torch.equal(out[..., others], base[..., others]) and not torch.equal(out[..., c], base[..., c]), (c, which)


def test_fp16_partial_sums_beyond_the_format_stay_finite_and_final_ones_are_infinite():
    """x = 1024 everywhere; taps (64, 64, 64 / -64, -64, -64 / 1, 0, 0): inside the image the partial sums reach 196608 = 3 x 65504 and return
    to 1024 -- finite only because the accumulator is fp32; in the top row the first three taps fall outside and the sum ends at -195584: -inf,
    as the restatement rounds it"""
    H, W, C = 4, 5, 8
    x = torch.full((1, H, W, C), 1024.0, dtype=torch.float16)
    w = torch.tensor([64.0, 64, 64, -64, -64, -64, 1, 0, 0]).view(1, 3, 3, 1).expand(C, 3, 3, 1).contiguous().half()
    out = _conv(x, w).cpu()
    assert torch.equal(out, dwconv_ref32(x, w))
    assert (out[0, 1:H - 1, 1:W - 1] == 1024).all() and torch.isfinite(out[0, 1:]).all()
    assert (out[0, 0, 1:W - 1] == float("-inf")).all()
    assert not torch.isfinite(dwconv_16bit(x, w)[0, 1:H - 1, 1:W - 1]).any()  # (what a 16-bit accumulator makes of it)
    assert (_conv(x, -w).cpu()[0, 0, 1:W - 1] == float("inf")).all()


def test_wrapper_checks_on_gpu_tensors():
    from nunchaku_amd._C import ops

    x = torch.zeros(2, 3, 4, 16, device="cuda", dtype=torch.bfloat16)
    w, b = torch.zeros(16, 3, 3, 1, device="cuda", dtype=torch.bfloat16), torch.zeros(16, device="cuda", dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="unit channel stride"):
        _conv(torch.zeros(2, 3, 16, 4, device="cuda", dtype=torch.bfloat16).transpose(2, 3), w, b)
    with pytest.raises(ValueError, match="stride"):   # a [B, H, W, C] crop whose rows are not W tokens apart
        _conv(torch.zeros(2, 3, 6, 16, device="cuda", dtype=torch.bfloat16)[:, :, :4], w, b)
    with pytest.raises(ValueError, match="overlap"):
        _conv(x, w, b, out=x)
    with pytest.raises(ValueError, match="overlap"):
        buf = torch.zeros(2 * 12 * 16 + 16, device="cuda", dtype=torch.bfloat16)
        ops.dwconv3x3(buf[:384].view(2, 3, 4, 16), w, b, buf[16:].view(2, 3, 4, 16))
    with pytest.raises(ValueError, match="share one 16-bit dtype"):
        _conv(x, w.half(), b)
    with pytest.raises(ValueError, match="share one 16-bit dtype"):
        _conv(x, w, b, out=torch.zeros(2, 3, 4, 16, device="cuda", dtype=torch.float16))
    with pytest.raises(ValueError, match="weight must be"):
        _conv(x, w.view(16, 1, 3, 3), b)
    with pytest.raises(ValueError, match="multiple of 8"):  # rows that are not 16-byte aligned
        _conv(torch.zeros(2, 3, 4, 20, device="cuda", dtype=torch.bfloat16)[..., :16], w, b)


# ---- the module -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def strict_mode():
    from nunchaku_amd import mode

    with mode.deterministic_mode("strict"):
        yield


def _layer(K, N, seed, bias, prefix):
    from oracle import svdq_oracle as O
    from tests.helpers import reference_state_dict

    L = O.make_svdq_layer(K, N, 32, seed=seed, dtype="bf16", bias=bias, cheap=True)
    return {prefix + k: v for k, v in reference_state_dict(L, "bf16").items()}


@pytest.mark.parametrize("features,hidden", [(256, 384), (320, 320)])
def test_module_equals_its_composition_from_the_public_pieces(features, hidden, strict_mode):
    from nunchaku_amd.models import SanaGLUMBConv
    from nunchaku_amd.ops.conv import dwconv3x3
    from nunchaku_amd.ops.gemm import svdq_gemm_w4a4_cuda
    from nunchaku_amd.ops.quantize import svdq_quantize_w4a4_act_fuse_lora_cuda

    B, H, W = 2, 7, 9
    T = H * W
    m = SanaGLUMBConv(features, hidden, device="cuda")
    ip, cg, hp = m.in_pad, m.c_gemm, m.hid_pad
    assert (ip, cg, hp) == ((256, 768, 384) if features == 256 else (384, 640, 384))
    g = torch.Generator().manual_seed(features)
    sd = {**_layer(ip, cg, 21, True, "inverted_conv."), **_layer(hp, ip, 22, False, "point_conv."),
          "depth_conv.weight": (torch.randn(cg, 3, 3, 1, generator=g) / 3).to(torch.bfloat16), "depth_conv.bias": torch.randn(cg, generator=g).to(torch.bfloat16)}
    m.load_state_dict(sd, strict=True)
    x = torch.randn(B, T, features, generator=g).to(torch.bfloat16).cuda()

    y = m(x, H, W)
    assert y.shape == (B, T, features) and y.dtype == torch.bfloat16 and torch.isfinite(y).all()
    assert torch.equal(m(x, H, W), y)                                 # a second call
    assert torch.equal(m(x, H), y) and torch.equal(m(x, None, W), y)  # one side derived from the other

    # the hand composition: quantise -> GEMM with the SiLU epilogue -> convolution -> GLU quantiser -> GEMM -> slice
    ic, pc = m.inverted_conv, m.point_conv
    qx, asc, la = ic.quantize(F.pad(x, (0, ip - features)).view(B * T, ip))
    mid = torch.empty(B * T, cg, device="cuda", dtype=torch.bfloat16)
    svdq_gemm_w4a4_cuda(act=qx, wgt=ic.qweight, out=mid, ascales=asc, wscales=ic.wscales, lora_act_in=la, lora_up=ic.proj_up, bias=ic.bias,
                        act_unsigned=ic.act_unsigned, fuse_silu=True)
    wide = torch.zeros(B, T, 2 * hp, device="cuda", dtype=torch.bfloat16)
    dwconv3x3(mid.view(B, T, cg), m.depth_conv.weight, m.depth_conv.bias, height=H, width=W, out=wide[..., :cg])
    qx2, asc2, la2 = svdq_quantize_w4a4_act_fuse_lora_cuda(wide.view(B * T, 2 * hp), lora_down=pc.proj_down, smooth=pc.smooth_factor, fuse_glu=True)
    hand = torch.empty(B * T, ip, device="cuda", dtype=torch.bfloat16)
    svdq_gemm_w4a4_cuda(act=qx2, wgt=pc.qweight, out=hand, ascales=asc2, wscales=pc.wscales, lora_act_in=la2, lora_up=pc.proj_up, bias=pc.bias,
                        act_unsigned=pc.act_unsigned)
    assert torch.equal(y, hand.view(B, T, ip)[..., :features])

    # the convolution inside the module, on the module's own GEMM output
    gated = m.gated_input(x, H, W)
    assert gated.shape == (B, T, 2 * hp) and torch.equal(gated, wide)
    want = dwconv_ref32(mid.view(B, H, W, cg), m.depth_conv.weight, m.depth_conv.bias)
    assert torch.equal(gated[..., :cg].cpu().view(B, H, W, cg), want) and want.float().abs().max() > 0.1
    if 2 * hp != cg:  # the zero tail, after two (here: several) calls
        assert 2 * hp - cg == 128 and (m.gated_input(x, H, W)[..., cg:] == 0).all() and (gated[..., cg:] == 0).all()

    # grid arguments
    sq = x[:, :49].contiguous()
    assert torch.equal(m(sq), m(sq, 7, 7)) and not torch.equal(m(x, W, H), y)
    with pytest.raises(ValueError, match="does not hold"):
        m(x)
    with pytest.raises(ValueError, match="does not hold"):
        m(x, 8, 8)
