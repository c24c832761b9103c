"""The MXFP4 GEMM's GELU_QUANT epilogue and fused_gelu_mlp on two MXFP4 layers: the 16-bit activation against float64, the
codes / scales / low-rank activations against the pinned quantiser run on that activation."""

import numpy as np
import pytest
import torch

from tests.helpers import ulp16_of
from tests.test_mxfp4_format import DT, nibbles

pytestmark = pytest.mark.gpu
SMOOTH = [0.5, 1.0, 2.0, 3.0, 1.5, 0.75, 5.0, 1.375]  # powers of two and other values


def gelu_tanh64(x):
    return 0.5 * x * (1.0 + np.tanh(0.7978845608028654 * (x + 0.044715 * x ** 3)))


def _fused(a, w, M, R, bias, dtype, R_next, zeroed, seed, smooth=None):
    """one GELU_QUANT launch on host-encoded operands (a [M, K], w [N, K]; ``bias``: bool or the vector) -> the first check (g against float64,
    the padding columns of a wider out untouched), then the second (codes, scales and lora_act_out against svdq_quantize_mxfp4 on that g)"""
    from nunchaku_amd.ops import svdq_gemm_mxfp4, svdq_quantize_mxfp4
    from nunchaku_amd.quantization.mxfp4 import dequantize_mxfp4, pack_scales_mxfp4, quantize_weight_mxfp4, unpack_scales_mxfp4

    g, dt = torch.Generator().manual_seed(seed), DT[dtype]
    K, N, M_pad = a.shape[1], w.shape[0], -(-M // 256) * 256
    a_pad = torch.zeros(M_pad, K, dtype=dt)
    a_pad[:M] = a
    (ac, asc), (wc, wsc) = quantize_weight_mxfp4(a_pad), quantize_weight_mxfp4(w)
    la = torch.zeros(M_pad, R)
    la[:M] = torch.randn(M, R, generator=g)
    lu = (torch.randn(N, R, generator=g) / 4).to(dt)
    b = bias if torch.is_tensor(bias) else torch.randn(N, generator=g).to(dt) if bias else None
    smooth = (torch.tensor(SMOOTH)[torch.randint(0, 8, (N,), generator=g)] if smooth is None else smooth).to(dt)
    down = (torch.randn(N, R_next, generator=g) / 8).to(dt).cuda() if R_next else None
    out = torch.full((M, N + 8), 7.0, dtype=dt, device="cuda")
    qout, osc = torch.full((M_pad, N // 2), 0x55, dtype=torch.uint8, device="cuda"), torch.full((N // 128, M_pad, 4), 9, dtype=torch.uint8, device="cuda")
    lao = (torch.zeros if zeroed else torch.ones)(M_pad, R_next, device="cuda") if R_next else None
    svdq_gemm_mxfp4(ac.cuda(), wc.cuda(), pack_scales_mxfp4(asc).cuda(), wsc.cuda(), out=out[:, :N], lora_act_in=la.cuda() if R else None,
                    lora_up=lu.cuda() if R else None, bias=None if b is None else b.cuda(), rows=M, qout=qout, oscales=osc, lora_down=down,
                    lora_act_out=lao, smooth_factor=smooth.cuda(), lora_act_zeroed=zeroed)
    A, W = dequantize_mxfp4(ac, asc)[:M].numpy(), dequantize_mxfp4(wc, wsc).numpy()
    la16, lu64, b64 = la[:M].to(dt).double().numpy(), lu.double().numpy(), np.zeros(N) if b is None else b.double().numpy()
    ref = gelu_tanh64(A @ W.T + la16 @ lu64.T + b64)
    mag = np.abs(A) @ np.abs(W).T + np.abs(la16) @ np.abs(lu64).T + np.abs(b64)
    got = out[:, :N].cpu().double().numpy()
    worst = (np.abs(got - ref) / (ulp16_of(ref, dtype) + 1.13 * (K + R + 2) * 2.0 ** -24 * mag)).max()
    print(f"worst |g - gelu(ref)| / bound = {worst:.3f}")
    assert np.isfinite(got).all() and worst <= 1.0 and bool((out[:, N:] == 7.0).all())
    act, asc2, la2 = svdq_quantize_mxfp4(out[:, :N], lora_down=down, smooth=smooth.cuda())
    codes, scales = nibbles(qout), unpack_scales_mxfp4(osc).cpu().numpy().T
    assert np.array_equal(codes[:M], nibbles(act)[:M]) and np.array_equal(scales[:M], unpack_scales_mxfp4(asc2).cpu().numpy().T[:M])
    assert not codes[M:].any() and not scales[M:].any()
    if R_next:
        d64 = down.cpu().double().numpy()
        err = np.abs(lao[:M].cpu().double().numpy() - got @ d64) / (2e-5 * (np.abs(got) @ np.abs(d64)) + 1e-6)
        print(f"worst lora_act_out err / bound = {err.max():.3f}")
        assert err.max() <= 1.0 and not lao[M:].any()
    return got, codes, scales


SHAPES = [(M, K, N) for M in (1, 33, 257) for K in (128, 384) for N in (128, 384)]
OPTIONS = [(0, False, 32, False), (32, True, 48, True), (32, False, 0, False), (0, True, 32, True), (32, True, 32, False), (0, False, 48, False)]


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("M,K,N,R,bias,R_next,zeroed", [s + OPTIONS[(i + j) % 6] for i, s in enumerate(SHAPES) for j in (0, 3)])
def test_activation_codes_scales_and_low_rank(M, K, N, R, bias, R_next, zeroed, dtype):
    """The bound on g is derived: one 16-bit rounding of gelu (a full spacing: half of it is the rounding, the other half, >= 2^-12 relative, covers
    the fp32 evaluation of gelu near 2^-22) plus the plain GEMM's fp32 accumulation bound through |gelu'| <= 1.13."""
    g = torch.Generator().manual_seed(M * K + N)
    a, w = torch.randn(M, K, generator=g).to(DT[dtype]), (torch.randn(N, K, generator=g) / 8).to(DT[dtype])
    _fused(a, w, M, R, bias, dtype, R_next, zeroed, seed=R + M)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_constructed_blocks_through_the_bias(dtype):
    """all-zero activation codes: h32 = bias[n] exactly, in every row.  Blocks 5 (tile 1, ni 1), 6, 9 (tile 2) and 11 of N = 384"""
    M, K, N, top = 33, 128, 384, float(torch.finfo(DT[dtype]).max)
    bias = torch.zeros(N, dtype=torch.float64)
    bias[164:168] = torch.tensor([1.0, 2.0, 3.0, 0.5])             # block 5: non-zero in columns 4 .. 7 only -- half 1's lanes
    bias[192:224] = -30.0                                          # block 6: deep in the negative tail, every value rounds to zero
    bias[288:292], bias[292:320] = torch.tensor([8.0, 1.0, -3.0, 0.75]), -30.0  # block 9: gelu(8) = 8, a power of two, next to the tail
    bias[352:356] = torch.tensor([top, -top / 2, top / 4, top / 16])  # block 11: the dtype's maximum
    smooth = torch.tensor(SMOOTH * 48)
    smooth[160:192], smooth[288:320] = 1.0, 2.0  # (powers of two where the codes are asserted below)
    got, codes, scales = _fused(torch.zeros(M, K, dtype=DT[dtype]), torch.randn(N, K).to(DT[dtype]), M, 0, bias.to(DT[dtype]), dtype, 32, False, 1, smooth)
    assert np.all(got[:, 288] == 8.0) and np.all(got[:, 352] == top) and not got[:, 192:224].any()
    assert not codes[:M, 192:224].any() and not scales[:M, 6].any() and not codes[:M, 292:320].any()  # code 0, never 8 (-0); scale byte 0
    assert np.all(codes[:M, 288] == 6) and np.all(scales[:M, 9] == 127) and codes[:M, 164:168].all() and not codes[:M, 160:164].any()


def _mlp(dtype, rank, precision=("mxfp4", "mxfp4")):
    from nunchaku_amd.models.linear import SVDQW4A4Linear

    g, dt = torch.Generator().manual_seed(4), DT[dtype]
    layers = []
    for (k, n), prec in zip(((256, 384), (384, 128)), precision):
        if prec == "int4":
            layers.append(SVDQW4A4Linear(k, n, torch_dtype=dt, device="cuda"))
            continue
        down, up = (torch.randn(k, rank, generator=g) / 8).to(dt), (torch.randn(n, rank, generator=g) / 8).to(dt)
        down[128:] = 0  # the low-rank sum of a row meets in atomics over the 128-column tiles: with one tile non-zero their order cannot matter
        layers.append(SVDQW4A4Linear.from_float((torch.randn(n, k, generator=g) / 16).to(dt), bias=torch.randn(n, generator=g).to(dt),
                                                smooth=torch.tensor(SMOOTH)[torch.randint(0, 8, (k,), generator=g)].to(dt),
                                                proj_down=down if rank else None, proj_up=up if rank else None).cuda())
    return layers, torch.randn(2, 33, 256, generator=g).to(dt).cuda()


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("rank", [0, 32])
def test_fused_gelu_mlp(rank, dtype):
    from nunchaku_amd.ops import svdq_gemm_mxfp4
    from nunchaku_amd.ops.fused import fused_gelu_mlp
    from nunchaku_amd.quantization.mxfp4 import dequantize_mxfp4, unpack_scales_mxfp4

    (fc1, fc2), x = _mlp(dtype, rank)
    y = fused_gelu_mlp(x, fc1, fc2)
    assert tuple(y.shape) == (2, 33, 128)
    qx, asc, la = fc1.quantize(x.reshape(66, 256))  # the three ops by hand
    qh, sh = torch.empty(256, 192, dtype=torch.uint8, device="cuda"), torch.empty(3, 256, 4, dtype=torch.uint8, device="cuda")
    lh = torch.empty(256, rank, device="cuda") if rank else None
    svdq_gemm_mxfp4(qx, fc1.qweight, asc, fc1.wscales, lora_act_in=la if rank else None, lora_up=fc1.proj_up if rank else None, bias=fc1.bias, rows=66,
                    qout=qh, oscales=sh, lora_down=fc2.proj_down if rank else None, lora_act_out=lh, smooth_factor=fc2.smooth_factor)
    hand = svdq_gemm_mxfp4(qh, fc2.qweight, sh, fc2.wscales, lora_act_in=lh, lora_up=fc2.proj_up if rank else None, bias=fc2.bias, rows=66)
    assert torch.equal(y.reshape(66, 128), hand)
    sd = fc2.state_dict()
    A, W = dequantize_mxfp4(qh.cpu(), unpack_scales_mxfp4(sh.cpu()))[:66].numpy(), dequantize_mxfp4(sd["qweight"].cpu(), sd["wscales"].cpu()).numpy()
    la16 = lh[:66].to(DT[dtype]).cpu().double().numpy() if rank else np.zeros((66, 0))
    up64, b64 = sd["proj_up"].cpu().double().numpy(), sd["bias"].cpu().double().numpy()
    ref = A @ W.T + la16 @ up64.T + b64
    mag = np.abs(A) @ np.abs(W).T + np.abs(la16) @ np.abs(up64).T + np.abs(b64)
    worst = (np.abs(y.reshape(66, 128).cpu().double().numpy() - ref) / (ulp16_of(ref, dtype) + (384 + rank + 2) * 2.0 ** -24 * mag)).max()
    print(f"worst |y - ref| / bound = {worst:.3f}")
    assert worst <= 1.0


def test_refusals_come_before_any_launch():
    from nunchaku_amd.ops import svdq_gemm_mxfp4
    from nunchaku_amd.ops.fused import fused_gelu_mlp

    z = lambda *s, dt=torch.uint8: torch.zeros(*s, dtype=dt, device="cuda")
    args = (z(256, 64), z(128, 64), z(1, 256, 4), z(4, 128))
    ok = dict(qout=z(256, 64), oscales=z(1, 256, 4), rows=4)
    for match, kw in (("oscales", dict(ok, oscales=None)), ("come together", dict(ok, lora_down=z(128, 32, dt=torch.bfloat16))),
                      ("multiple of 16", dict(ok, lora_down=z(128, 24, dt=torch.bfloat16), lora_act_out=z(256, 24, dt=torch.float32))),
                      ("qout must be", dict(ok, qout=z(256, 96))), ("give qout", dict(oscales=z(1, 256, 4)))):
        with pytest.raises(ValueError, match=match):
            svdq_gemm_mxfp4(*args, **kw)
    (fc1, fc2), x = _mlp("bf16", 0)
    with pytest.raises(NotImplementedError, match="MXFP4"):
        fused_gelu_mlp(x, fc1, fc2, ln=(None, None, None))
    for precision in (("mxfp4", "int4"), ("int4", "mxfp4")):
        with pytest.raises(ValueError, match="share one precision"):
            fused_gelu_mlp(x, *_mlp("bf16", 0, precision)[0])
