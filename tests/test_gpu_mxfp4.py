"""The MXFP4 quantiser, GEMM and module on the GPU against the float64 restatement of tests/test_mxfp4_format.py."""

import numpy as np
import pytest
import torch

from tests.helpers import ulp16_of
from tests.test_mxfp4_format import DT, constructed_blocks, mxfp4_ref, nibbles

pytestmark = pytest.mark.gpu


def _x(M, K, dtype, seed):
    """random rows with the constructed blocks in the first and the last block of rows 0 .. and of the last real row"""
    x = torch.randn(M, K, generator=torch.Generator().manual_seed(seed)).to(DT[dtype])
    blocks = constructed_blocks(dtype)
    for i in range(len(blocks)):
        x[min(i, M - 1), :32], x[M - 1 - min(i, M - 1), K - 32:] = blocks[i], blocks[-1 - i]
    x[M - 1, :32] = blocks[0]
    return x


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("smoothed", [False, True])
@pytest.mark.parametrize("R", [0, 32, 48])
@pytest.mark.parametrize("M,K", [(M, K) for M in (1, 33, 257) for K in (128, 384)] + [(33, 640)])  # K = 640: two K slices (atomics, the clearing kernel)
def test_quantiser_bit_for_bit(M, K, R, smoothed, dtype):
    """smooth holds powers of two and other values.  smooth_div16 is round16(x * rcp(smooth)) with the hardware reciprocal (1 ulp) and an fp32
    product (half an ulp): within 2 * 2^-24 |q| (+ 2^-148, the fp32 subnormal step) of q = x / smooth.  An element is kept where q lies farther
    than twice that from a 16-bit rounding boundary, so that round16(q) in float64 is what the kernel must have encoded; the others are zeroed."""
    from nunchaku_amd.ops import svdq_quantize_mxfp4
    from nunchaku_amd.quantization.mxfp4 import unpack_scales_mxfp4

    g = torch.Generator().manual_seed(M + K + R)
    x = _x(M, K, dtype, M + K)
    top = float(torch.finfo(DT[dtype]).max)
    smooth = torch.tensor([0.5, 1.0, 2.0, 3.0, 1.5, 0.75, 5.0, 1.375])[torch.randint(0, 8, (K,), generator=g)].to(DT[dtype]) if smoothed else None
    if smoothed:
        q = x.double() / smooth.double()
        r16 = q.to(DT[dtype]).double()  # overflows to inf
        half = torch.from_numpy(ulp16_of(q.nan_to_num(0.0, 0.0, 0.0).numpy(), dtype)) / 2  # a boundary lies half a spacing from a 16-bit number
        near = half - (q - r16).abs() <= 4 * 2.0 ** -24 * q.abs() + 2.0 ** -147
        keep = ~q.isfinite() | torch.where(r16.isfinite(), ~near, q.abs() > top * 1.01)
        x = torch.where(keep, x, torch.zeros_like(x))
        assert keep.float().mean() > 0.9
    down = (torch.randn(K, R, generator=g) / 8).to(DT[dtype]) if R else None
    wide = torch.full((M, K + 8), 3.0, dtype=DT[dtype])
    wide[:, :K] = x
    act, asc, la = svdq_quantize_mxfp4(wide.cuda()[:, :K], lora_down=None if down is None else down.cuda(), smooth=None if smooth is None else smooth.cuda())
    M_pad = -(-M // 256) * 256
    assert tuple(act.shape) == (M_pad, K // 2) and tuple(asc.shape) == (K // 128, M_pad, 4) and tuple(la.shape) == (M_pad, R)
    v = x.double().numpy() if smooth is None else torch.where(keep, r16, torch.zeros_like(r16)).numpy()
    ref_c, ref_s = mxfp4_ref(v, top)
    got_c, got_s = nibbles(act), unpack_scales_mxfp4(asc).cpu().numpy().T
    assert np.array_equal(got_c[:M], ref_c) and np.array_equal(got_s[:M], ref_s)
    assert not got_c[M:].any() and not got_s[M:].any() and not la[M:].any()
    if R:
        xf = np.nan_to_num(x.double().numpy(), nan=0.0, posinf=0.0, neginf=0.0)
        finite = np.isfinite(x.double().numpy()).all(1)
        ref = xf @ down.double().numpy()
        bound = 2e-5 * (np.abs(xf) @ np.abs(down.double().numpy())) + 1e-6  # the existing quantiser tests' bound (tests/test_gpu_quantize_glu.py)
        err = np.abs(la[:M].cpu().double().numpy() - ref)
        assert np.all(err[finite] <= bound[finite]), f"lora_act: worst err / bound = {(err[finite] / bound[finite]).max():.2f}"


def _gemm_case(a, w, M, R, bias, dtype, seed, ld_extra=8):
    """a [M, K], w [N, K] 16-bit values -> (got float64 [M, N], ref, bound) of one svdq_gemm_mxfp4 launch on host-encoded operands"""
    from nunchaku_amd.ops import svdq_gemm_mxfp4
    from nunchaku_amd.quantization.mxfp4 import dequantize_mxfp4, pack_scales_mxfp4, quantize_weight_mxfp4

    g = torch.Generator().manual_seed(seed)
    K, N, M_pad = a.shape[1], w.shape[0], -(-M // 256) * 256
    a_pad = torch.zeros(M_pad, K, dtype=a.dtype)
    a_pad[:M] = a
    ac, asc = quantize_weight_mxfp4(a_pad)
    wc, wsc = quantize_weight_mxfp4(w)
    la = torch.zeros(M_pad, R)
    la[:M] = torch.randn(M, R, generator=g)
    lu = (torch.randn(N, R, generator=g) / 4).to(DT[dtype])
    b = torch.randn(N, generator=g).to(DT[dtype]) if bias else None
    scales = [1.0, 0.5, 1.0][:R // 16] if R else None  # (a power of two: the fp32 product is exact, so one rounding or two agree)
    out = torch.full((M, N + ld_extra), 7.0, dtype=DT[dtype], device="cuda")
    args = (ac.cuda(), wc.cuda(), pack_scales_mxfp4(asc).cuda(), wsc.cuda())
    kw = dict(lora_act_in=la.cuda() if R else None, lora_up=lu.cuda() if R else None, bias=None if b is None else b.cuda(), lora_scales=scales, rows=M)
    svdq_gemm_mxfp4(*args, out=out[:, :N], **kw)
    again = svdq_gemm_mxfp4(*args, **kw) if R or bias else svdq_gemm_mxfp4(*args, out=torch.empty(M, N, dtype=DT[dtype], device="cuda"), **kw)
    assert torch.equal(again, out[:, :N]) and bool((out[:, N:] == 7.0).all())
    A, W = dequantize_mxfp4(ac, asc)[:M].numpy(), dequantize_mxfp4(wc, wsc).numpy()
    la16 = (la[:M] * torch.tensor(scales or [1.0]).repeat_interleave(16)[:R]).to(DT[dtype]).double().numpy() if R else np.zeros((M, 0))
    lu64, b64 = lu.double().numpy(), np.zeros(N) if b is None else b.double().numpy()
    ref = A @ W.T + la16 @ lu64.T + b64
    mag = np.abs(A) @ np.abs(W).T + np.abs(la16) @ np.abs(lu64).T + np.abs(b64)
    return out[:, :N].cpu().double().numpy(), ref, ulp16_of(ref, dtype) + (K + R + 2) * 2.0 ** -24 * mag


def _held(got, ref, bound):
    worst = (np.abs(got - ref) / bound).max()
    print(f"worst |got - ref| / bound = {worst:.3f}")
    assert np.isfinite(got).all() and worst <= 1.0


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("R", [0, 32, 48])
@pytest.mark.parametrize("N", [128, 384])
@pytest.mark.parametrize("K", [128, 384])
@pytest.mark.parametrize("M", [1, 32, 33, 257])
def test_gemm_within_the_derived_bound(M, K, N, R, bias, dtype):
    g = torch.Generator().manual_seed(M * K + N)
    a, w = torch.randn(M, K, generator=g).to(DT[dtype]), (torch.randn(N, K, generator=g) / 8).to(DT[dtype])
    _held(*_gemm_case(a, w, M, R, bias, dtype, seed=R + M))


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_gemm_block_exponents_reach_the_mfma_on_both_operands(dtype):
    """In every row of both operands: a block at max / 4 (elements up to the dtype's maximum: the largest scale byte the encoder produces) opposite a
    block of subnormals of the other operand, in both directions, and ordinary blocks between them.  Every product is max / 4 * subnormal ~ 1."""
    from nunchaku_amd.quantization.mxfp4 import quantize_weight_mxfp4

    fi, g = torch.finfo(DT[dtype]), torch.Generator().manual_seed(5)
    M, K, N = 33, 384, 128
    level = torch.ones(K, dtype=torch.float64)
    level[:32], level[64:96], level[-32:] = fi.max / 4, fi.smallest_normal / 4, fi.smallest_normal / 2
    a = (torch.randn(M, K, generator=g).clamp(-3.9, 3.9).double() * level).to(DT[dtype])
    w = (torch.randn(N, K, generator=g).clamp(-3.9, 3.9).double() * level.flip(0)).to(DT[dtype])
    a[:, 0], w[:, K - 1] = fi.max, -fi.max
    for t in (a, w):
        s = quantize_weight_mxfp4(t)[1]
        assert int(s.max()) == (252 if dtype == "bf16" else 140) and int(s.min()) <= (1 if dtype == "bf16" else 111)
    _held(*_gemm_case(a, w, M, 32, True, dtype, seed=9))


def test_gemm_pairs_every_scale_byte_with_its_own_block():
    """K = 384, one non-zero block per row at block 0, 5 or 11 (row % 3), every block of the other operand at its own power of two"""
    M, K, N = 33, 384, 128
    g = torch.Generator().manual_seed(6)
    a = torch.zeros(M, K)
    for m in range(M):
        blk = (0, 5, 11)[m % 3]
        a[m, 32 * blk:32 * blk + 32] = torch.randn(32, generator=g) * 2.0 ** (m % 7)
    w = torch.randn(N, K, generator=g) * (2.0 ** (torch.arange(K) // 32 * 3 - 16))
    _held(*_gemm_case(a.bfloat16(), w.bfloat16(), M, 0, False, "bf16", seed=1))


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_module_is_the_two_ops_and_lora_round_trips(dtype):
    from nunchaku_amd.models.linear import SVDQW4A4Linear
    from nunchaku_amd.ops import svdq_gemm_mxfp4, svdq_quantize_mxfp4
    from nunchaku_amd.quantization.mxfp4 import dequantize_mxfp4, unpack_scales_mxfp4

    g = torch.Generator().manual_seed(3)
    K, N, R = 256, 128, 32
    w, b = (torch.randn(N, K, generator=g) / 16).to(DT[dtype]), torch.randn(N, generator=g).to(DT[dtype])
    smooth = (2.0 ** torch.randint(-1, 2, (K,), generator=g)).to(DT[dtype])
    down, up = (torch.randn(K, R, generator=g) / 8).to(DT[dtype]), (torch.randn(N, R, generator=g) / 8).to(DT[dtype])
    lin = SVDQW4A4Linear.from_float(w, bias=b, smooth=smooth, proj_down=down, proj_up=up).cuda()
    sd = {k: v.clone() for k, v in lin.state_dict().items()}
    x = torch.randn(2, 33, K, generator=g).to(DT[dtype]).cuda()
    y = lin(x)
    assert tuple(y.shape) == (2, 33, N) and torch.equal(lin(x.reshape(66, K)), y.reshape(66, N))
    assert all(torch.equal(v.cpu(), lin.state_dict()[k].cpu()) for k, v in sd.items())  # the repacked layer exports the checkpoint layout
    act, asc, la = svdq_quantize_mxfp4(x.reshape(66, K), lora_down=down.cuda(), smooth=smooth.cuda())
    two = svdq_gemm_mxfp4(act, lin.qweight, asc, sd["wscales"].cuda(), lora_act_in=la, lora_up=up.cuda(), bias=b.cuda(), rows=66)
    assert torch.equal(two, y.reshape(66, N))
    A = dequantize_mxfp4(act.cpu(), unpack_scales_mxfp4(asc.cpu()))[:66].numpy()
    W = dequantize_mxfp4(sd["qweight"].cpu(), sd["wscales"].cpu()).numpy()
    la16, up64, b64 = la[:66].to(DT[dtype]).cpu().double().numpy(), up.double().numpy(), b.double().numpy()
    ref = A @ W.T + la16 @ up64.T + b64
    mag = np.abs(A) @ np.abs(W).T + np.abs(la16) @ np.abs(up64).T + np.abs(b64)
    _held(y.reshape(66, N).cpu().double().numpy(), ref, ulp16_of(ref, dtype) + (K + R + 2) * 2.0 ** -24 * mag)
    lin.set_lora(torch.randn(4, K, generator=g), torch.randn(N, 4, generator=g), strength=0.5)
    assert lin.rank == 48 and not torch.equal(lin(x), y)
    lin.reset_lora()
    assert torch.equal(lin(x), y)


def test_refusals_come_before_any_launch():
    from nunchaku_amd.models.linear import SVDQW4A4Linear
    from nunchaku_amd.ops import svdq_gemm_mxfp4, svdq_quantize_mxfp4

    with pytest.raises(ValueError, match="multiple of 128"):
        svdq_quantize_mxfp4(torch.zeros(4, 192, dtype=torch.bfloat16, device="cuda"))
    z = lambda *s: torch.zeros(*s, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="wscales"):
        svdq_gemm_mxfp4(z(256, 64), z(128, 64), z(1, 256, 4), z(3, 128))
    lin = SVDQW4A4Linear(128, 128, precision="mxfp4", device="cuda")
    with pytest.raises(NotImplementedError, match="MXFP4"):
        lin(torch.zeros(1, 4, 128, dtype=torch.bfloat16, device="cuda"), ln=(None, None, None))
