"""The MXFP4 GEMM's GLU_QUANT epilogue and fused_glu_feed_forward on two MXFP4 layers: x = value * act(gate) against float64
on the plain launch's own 16-bit columns, the codes / scales / low-rank activations against the pinned quantiser run on that x."""

import numpy as np
import pytest
import torch

from tests.glu_halves_ref import act64
from tests.helpers import ulp16_of
from tests.test_mxfp4_format import DT, nibbles

pytestmark = pytest.mark.gpu
SMOOTH = [0.5, 1.0, 2.0, 3.0, 1.5, 0.75, 5.0, 1.375]  # powers of two and other values


def _fused(a, w, M, R, bias, dtype, act, R_next, zeroed, seed, smooth=None):
    """one GLU_QUANT and one plain launch on the same host-encoded operands (a [M, K], w [2 Hd, K]; ``bias``: bool or the vector) -> x against float64 on
    the plain launch's columns (the spare columns of a wider out untouched), then codes, scales and lora_act_out against svdq_quantize_mxfp4 on that x"""
    from nunchaku_amd.ops import svdq_gemm_mxfp4, svdq_quantize_mxfp4
    from nunchaku_amd.quantization.mxfp4 import pack_scales_mxfp4, quantize_weight_mxfp4, unpack_scales_mxfp4

    g, dt = torch.Generator().manual_seed(seed), DT[dtype]
    K, N, Hd, M_pad = a.shape[1], w.shape[0], w.shape[0] // 2, -(-M // 256) * 256
    a_pad = torch.zeros(M_pad, K, dtype=dt)
    a_pad[:M] = a
    (ac, asc), (wc, wsc) = quantize_weight_mxfp4(a_pad), quantize_weight_mxfp4(w)
    la = torch.zeros(M_pad, R)
    la[:M] = torch.randn(M, R, generator=g)
    lu = (torch.randn(N, R, generator=g) / 4).to(dt)
    b = bias if torch.is_tensor(bias) else torch.randn(N, generator=g).to(dt) if bias else None
    smooth = (torch.tensor(SMOOTH)[torch.randint(0, 8, (Hd,), generator=g)] if smooth is None else smooth).to(dt)
    down = (torch.randn(Hd, R_next, generator=g) / 8).to(dt).cuda() if R_next else None
    out = torch.full((M, Hd + 8), 7.0, dtype=dt, device="cuda")
    qout, osc = torch.full((M_pad, Hd // 2), 0x55, dtype=torch.uint8, device="cuda"), torch.full((Hd // 128, M_pad, 4), 9, dtype=torch.uint8, device="cuda")
    lao = (torch.zeros if zeroed else torch.ones)(M_pad, R_next, device="cuda") if R_next else None
    ops = (ac.cuda(), wc.cuda(), pack_scales_mxfp4(asc).cuda(), wsc.cuda())
    kw = dict(lora_act_in=la.cuda() if R else None, lora_up=lu.cuda() if R else None, bias=None if b is None else b.cuda(), rows=M)
    svdq_gemm_mxfp4(*ops, out=out[:, :Hd], qout=qout, oscales=osc, lora_down=down, lora_act_out=lao, smooth_factor=smooth.cuda(),
                    lora_act_zeroed=zeroed, glu=act, **kw)
    y = svdq_gemm_mxfp4(*ops, out=torch.empty(M, N, dtype=dt, device="cuda"), **kw).cpu().double().numpy()
    v, a64 = y[:, :Hd], act64(y[:, Hd:], act)
    ref, got = v * a64, out[:, :Hd].cpu().double().numpy()
    worst = (np.abs(got - ref) / (ulp16_of(ref, dtype) + np.abs(v) * ulp16_of(a64, dtype))).max()
    print(f"worst |x - v act(g)| / bound = {worst:.3f}")
    assert np.isfinite(got).all() and worst <= 1.0 and bool((out[:, Hd:] == 7.0).all())
    qa, qs, _ = svdq_quantize_mxfp4(out[:, :Hd], lora_down=down, smooth=smooth.cuda())
    codes, scales = nibbles(qout), unpack_scales_mxfp4(osc).cpu().numpy().T
    assert np.array_equal(codes[:M], nibbles(qa)[:M]) and np.array_equal(scales[:M], unpack_scales_mxfp4(qs).cpu().numpy().T[:M])
    assert not codes[M:].any() and not scales[M:].any()
    if R_next:
        d64 = down.cpu().double().numpy()
        err = np.abs(lao[:M].cpu().double().numpy() - got @ d64) / (2e-5 * (np.abs(got) @ np.abs(d64)) + 1e-6)
        print(f"worst lora_act_out err / bound = {err.max():.3f}")
        assert err.max() <= 1.0 and not lao[M:].any()
    return got, codes, scales


SHAPES = [(M, K, Hd) for M in (1, 33, 257) for K in (128, 384) for Hd in (128, 384)]
OPTIONS = [(0, False, 32, False), (32, True, 48, True), (32, False, 0, False), (0, True, 32, True), (32, True, 32, False), (0, False, 48, False)]


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("act", ["silu", "gelu"])
@pytest.mark.parametrize("M,K,Hd,R,bias,R_next,zeroed", [s + OPTIONS[(i + j) % 6] for i, s in enumerate(SHAPES) for j in (0, 3)])
def test_activation_codes_scales_and_low_rank(M, K, Hd, R, bias, R_next, zeroed, act, dtype):
    """The bound on x is derived: v and g are the library's own 16-bit columns, so nothing comes from the GEMM's accumulation; one full 16-bit
    spacing for the product's rounding plus one full spacing of act(g), scaled by |v|, for the rounding of a (half of each is the rounding itself,
    the other half, >= 2^-12 relative, covers the fp32 evaluation of the activation)."""
    g = torch.Generator().manual_seed(M * K + Hd)
    a, w = torch.randn(M, K, generator=g).to(DT[dtype]), (torch.randn(2 * Hd, K, generator=g) / 8).to(DT[dtype])
    _fused(a, w, M, R, bias, dtype, act, R_next, zeroed, seed=R + M)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("act", ["silu", "gelu"])
def test_constructed_blocks_through_the_bias(act, dtype):
    """all-zero activation codes: h32 = bias exactly, in every row.  Blocks 5 (tile 2, second block), 6, 8 and 11 of Hd = 384.  A gate of -30
    rounds to zero under gelu and in fp16, but silu(-30) = -2.8e-12 is an ordinary bf16 number: block 6 (gate -30) is asserted to be zero where the
    float64 activation is below half the dtype's smallest subnormal, and block 8 (gate -100) is zero under every activation and dtype."""
    M, K, Hd, top = 33, 128, 384, float(torch.finfo(DT[dtype]).max)
    bias = torch.zeros(2 * Hd, dtype=torch.float64)
    bias[160:164], bias[Hd + 160:Hd + 192] = torch.tensor([2.0, -1.0, 0.5, 0.0]), 30.0  # block 5: act(30) = 30; x = 60, -30, 15 under smooth 2
    bias[192:224], bias[Hd + 192:Hd + 224] = 3.0, -30.0  # block 6
    bias[256:288], bias[Hd + 256:Hd + 288] = -3.0, -100.0           # block 8: deep in the negative tail, every product rounds to (-)zero
    bias[352:356], bias[Hd + 352:Hd + 384] = torch.tensor([top, -top / 2, top / 4, top / 16]), 1.0  # block 11: the dtype's maximum times act(1) < 1
    smooth = torch.tensor(SMOOTH * 48)
    smooth[160:192], smooth[352:384] = 2.0, 1.0  # (powers of two where the codes are asserted below)
    got, codes, scales = _fused(torch.zeros(M, K, dtype=DT[dtype]), torch.randn(2 * Hd, K).to(DT[dtype]), M, 0, bias.to(DT[dtype]), dtype, act, 32, False, 1, smooth)
    # block 5: amax 30 -> byte floor(log2 30) - 2 + 127 = 129, scale 4: 7.5 saturates to 6 (code 7), -3.75 -> -4 (code 8 | 6), 1.875 -> 2 (code 4)
    assert np.all(got[:, 160:164] == [60.0, -30.0, 15.0, 0.0]) and np.all(scales[:M, 5] == 129)
    assert np.all(codes[:M, 160:164] == [7, 14, 4, 0]) and not codes[:M, 164:192].any()
    tiny = 2.0 ** (-134 if dtype == "bf16" else -25)  # half the smallest subnormal
    for blk, gate in ((6, -30.0), (8, -100.0)):
        if abs(act64(np.array([gate]), act)[0]) < tiny:  # code 0, never 8 (-0); scale byte 0
            assert not got[:, 32 * blk:32 * blk + 32].any() and not codes[:M, 32 * blk:32 * blk + 32].any() and not scales[:M, blk].any()
    assert abs(act64(np.array([-100.0]), act)[0]) < tiny and (abs(act64(np.array([-30.0]), act)[0]) < tiny) == ((act, dtype) != ("silu", "bf16"))
    amax = top * act64(np.array([1.0]), act)[0]  # (0.73 or 0.84 of the maximum: far from a power of two)
    assert np.isfinite(got[:, 352:384]).all() and np.all(scales[:M, 11] == np.floor(np.log2(amax)) - 2 + 127) and np.all(codes[:M, 352] > 0)


def _feed_forward(kind, dtype, rank):
    from nunchaku_amd.models.linear import SVDQW4A4Linear
    from nunchaku_amd.models.sdxl import NunchakuSDXLFeedForward
    from nunchaku_amd.models.zimage import NunchakuZImageFeedForward

    g, dt = torch.Generator().manual_seed(4), DT[dtype]
    kw = dict(rank=rank, precision="mxfp4", torch_dtype=dt)
    ff = NunchakuZImageFeedForward(256, 384, **kw) if kind == "zimage" else NunchakuSDXLFeedForward(128, **kw)
    for lin in (ff.net[0].proj, ff.net[2]):
        k, n = lin.in_features, lin.out_features
        down, up = (torch.randn(k, rank, generator=g) / 8).to(dt), (torch.randn(n, rank, generator=g) / 8).to(dt)
        down[64:] = 0  # the low-rank sum of a row meets in atomics over the 64-channel tiles: with one tile non-zero their order cannot matter
        src = SVDQW4A4Linear.from_float((torch.randn(n, k, generator=g) / 16).to(dt), bias=torch.randn(n, generator=g).to(dt) if lin.bias is not None else None,
                                        smooth=torch.tensor(SMOOTH)[torch.randint(0, 8, (k,), generator=g)].to(dt),
                                        proj_down=down if rank else None, proj_up=up if rank else None)
        lin.load_state_dict(src.state_dict())
    return ff.cuda(), torch.randn(2, 33, ff.net[0].proj.in_features, generator=g).to(dt).cuda()


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("kind,act,rank", [("zimage", "silu", 0), ("zimage", "silu", 32), ("sdxl", "gelu", 32)])
def test_fused_glu_feed_forward(kind, act, rank, dtype):
    from nunchaku_amd.ops import svdq_gemm_mxfp4
    from nunchaku_amd.quantization.mxfp4 import dequantize_mxfp4, unpack_scales_mxfp4

    ff, x = _feed_forward(kind, dtype, rank)
    proj, fc2, ff.fused_glu = ff.net[0].proj, ff.net[2], True
    Hd, C = fc2.in_features, fc2.out_features
    y = ff(x).reshape(66, C)
    qx, asc, la = proj.quantize(x.reshape(66, -1))  # the three ops by hand
    qh, sh = torch.empty(256, Hd // 2, dtype=torch.uint8, device="cuda"), torch.empty(Hd // 128, 256, 4, dtype=torch.uint8, device="cuda")
    lh = torch.empty(256, rank, device="cuda") if rank else None
    svdq_gemm_mxfp4(qx, proj.qweight, asc, proj.wscales, lora_act_in=la if rank else None, lora_up=proj.proj_up if rank else None, bias=proj.bias, rows=66,
                    qout=qh, oscales=sh, lora_down=fc2.proj_down if rank else None, lora_act_out=lh, smooth_factor=fc2.smooth_factor, glu=act)
    hand = svdq_gemm_mxfp4(qh, fc2.qweight, sh, fc2.wscales, out=torch.empty(66, C, dtype=DT[dtype], device="cuda"), lora_act_in=lh,
                           lora_up=fc2.proj_up if rank else None, bias=fc2.bias, rows=66)
    assert torch.equal(y, hand)
    sd = fc2.state_dict()
    A, W = dequantize_mxfp4(qh.cpu(), unpack_scales_mxfp4(sh.cpu()))[:66].numpy(), dequantize_mxfp4(sd["qweight"].cpu(), sd["wscales"].cpu()).numpy()
    la16 = lh[:66].to(DT[dtype]).cpu().double().numpy() if rank else np.zeros((66, 0))
    up64, b64 = sd["proj_up"].cpu().double().numpy(), sd["bias"].cpu().double().numpy() if "bias" in sd else np.zeros(C)
    ref = A @ W.T + la16 @ up64.T + b64
    mag = np.abs(A) @ np.abs(W).T + np.abs(la16) @ np.abs(up64).T + np.abs(b64)
    worst = (np.abs(y.cpu().double().numpy() - ref) / (ulp16_of(ref, dtype) + (Hd + rank + 2) * 2.0 ** -24 * mag)).max()
    print(f"worst |y - ref| / bound = {worst:.3f}")
    assert worst <= 1.0


def test_refusals_come_before_any_launch():
    from nunchaku_amd.models.linear import SVDQW4A4Linear, fused_glu_feed_forward
    from nunchaku_amd.ops import svdq_gemm_mxfp4

    z = lambda *s, dt=torch.uint8: torch.zeros(*s, dtype=dt, device="cuda")
    args = (z(256, 64), z(256, 64), z(1, 256, 4), z(4, 256))
    ok = dict(qout=z(256, 64), oscales=z(1, 256, 4), rows=4, glu="silu")
    for match, kw in (("needs qout", dict(glu="silu", rows=4)), ("one of", dict(ok, glu="relu")), ("qout must be", dict(ok, qout=z(256, 128))),
                      ("not combine", dict(ok, out_vt=z(128, 8, dt=torch.bfloat16))), ("not combine", dict(ok, norm_q=z(128, dt=torch.bfloat16))),
                      ("not combine", dict(ok, rotary_emb=z(256, 128, dt=torch.float32)))):
        with pytest.raises(ValueError, match=match):
            svdq_gemm_mxfp4(*args, **kw)
    ff, x = _feed_forward("zimage", "bf16", 0)
    for mixed in ((SVDQW4A4Linear(256, 768, bias=False, device="cuda"), ff.net[2]), (ff.net[0].proj, SVDQW4A4Linear(384, 256, bias=False, device="cuda"))):
        ff.net[0].proj, ff.net[2] = mixed
        with pytest.raises(ValueError, match="share one precision"):
            fused_glu_feed_forward(ff.net, x, "silu")
