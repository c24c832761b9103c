"""The MXFP4 GEMM's RMSNorm + RoPE epilogue and fused_qkv_norm_rottary on an MXFP4 layer: Q and K against float64, V and the
side outputs against the plain launch, a constructed exact case through the bias, the module path against the hand composition."""

from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests.helpers import ulp16_of
from tests.test_mxfp4_format import DT

pytestmark = pytest.mark.gpu


def _launch(ops, rope=True, **kw):
    """one svdq_gemm_mxfp4 launch (``rope``: under the RMSNorm + RoPE epilogue) into columns [0, N) of a wider buffer of sevens -> (those columns,
    ops).  ``ops``: the host-encoded operands of an earlier call, or what to build them from: dict(M, K, N, R, bias (bool or the vector), dtype,
    seed[, a (the activation), nat (the table, natural [M_pad, 64, (sin, cos)]), nq, nk])"""
    from nunchaku_amd.models.embeddings import pack_rotemb
    from nunchaku_amd.ops import svdq_gemm_mxfp4
    from nunchaku_amd.quantization.mxfp4 import pack_scales_mxfp4, quantize_weight_mxfp4

    if "act" not in ops:
        M, K, N, R, dt = ops["M"], ops["K"], ops["N"], ops["R"], DT[ops["dtype"]]
        g, M_pad = torch.Generator().manual_seed(ops["seed"]), -(-M // 256) * 256
        a_pad = torch.zeros(M_pad, K, dtype=dt)
        a_pad[:M] = ops["a"] if "a" in ops else torch.randn(M, K, generator=g).to(dt)
        (ac, asc), (wc, wsc) = quantize_weight_mxfp4(a_pad), quantize_weight_mxfp4((torch.randn(N, K, generator=g) / 8).to(dt))
        la = torch.zeros(M_pad, R)
        la[:M] = torch.randn(M, R, generator=g)
        lu, b = (torch.randn(N, R, generator=g) / 4).to(dt), ops["bias"]
        b = b if torch.is_tensor(b) else torch.randn(N, generator=g).to(dt) if b else None
        ang = torch.rand(M_pad, 64, generator=g) * 6.283185
        ops = dict(dict(nat=torch.stack([ang.sin(), ang.cos()], -1), nq=(torch.rand(128, generator=g) + 0.5).to(dt), nk=(torch.rand(128, generator=g) + 0.5).to(dt)),
                   **ops, ac=ac, asc=asc, wc=wc, wsc=wsc, la=la, lu=lu, b=b, act=ac.cuda(), wgt=wc.cuda(), ascales=pack_scales_mxfp4(asc).cuda(), wscales=wsc.cuda())
        ops["rope"] = dict(norm_q=ops["nq"].cuda(), norm_k=ops["nk"].cuda(), rotary_emb=pack_rotemb(ops["nat"].reshape(1, M_pad, 64, 1, 2))[0].cuda())
    M, N, R = ops["M"], ops["N"], ops["R"]
    out = torch.full((M, N + 8), 7.0, dtype=DT[ops["dtype"]], device="cuda")
    svdq_gemm_mxfp4(ops["act"], ops["wgt"], ops["ascales"], ops["wscales"], out=out[:, :N], lora_act_in=ops["la"].cuda() if R else None,
                    lora_up=ops["lu"].cuda() if R else None, bias=None if ops["b"] is None else ops["b"].cuda(), rows=M, **(ops["rope"] if rope else {}), **kw)
    assert bool((out[:, N:] == 7.0).all())
    return out[:, :N], ops


def _ref64(h, e, w, nat, dtype):
    """float64 rope(rmsnorm(h)) of one third h [M, H * 128] with norm weights w [128] and the natural table nat [M, 64, (sin, cos)] -> (ref, bound):
    see test_q_k_against_float64_v_and_side_outputs"""
    M = h.shape[0]
    h, e = h.reshape(M, -1, 128), e.reshape(M, -1, 128)
    coef = 1.0 / np.sqrt((h * h).mean(-1, keepdims=True) + 1e-6)
    y = (h * coef * w).reshape(M, -1, 64, 2)
    ey = (coef * np.abs(w) * e + np.abs(h * w) * coef ** 3 / 128 * (np.abs(h) * e).sum(-1, keepdims=True)).reshape(M, -1, 64, 2)
    s, c = nat[:, None, :, 0], nat[:, None, :, 1]
    rot = lambda v, s, c, sg: np.stack([v[..., 0] * c - sg * v[..., 1] * s, v[..., 0] * s + v[..., 1] * c], -1).reshape(M, -1)
    ref = rot(y, s, c, 1)
    return ref, ulp16_of(ref, dtype) + rot(ey, np.abs(s), np.abs(c), -1) + 24 * 2.0 ** -24 * rot(np.abs(y), np.abs(s), np.abs(c), -1)


SHAPES = [(M, K, N) for M in (1, 33, 257) for K in (128, 384) for N in (384, 768)]
OPTIONS = [(0, False), (32, True), (32, False), (0, True)]


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("M,K,N,R,bias", [s + OPTIONS[(i + j) % 4] for i, s in enumerate(SHAPES) for j in (0, 1)])
def test_q_k_against_float64_v_and_side_outputs(M, K, N, R, bias, dtype):
    """Bound on Q and K, every term from reference quantities: one 16-bit spacing of the reference (its rounding), plus the plain GEMM's accumulation
    bound e_c = (K + R + 2) 2^-24 mag_c carried to first order through the norm -- coef |w_c| e_c + |h_c w_c| coef^3 / 128 sum_j |h_j| e_j -- and
    through the rotation as |cos|- and |sin|-weighted sums, plus 24 * 2^-24 of |y_2j cos| + |y_2j+1 sin| for the epilogue's own fp32 work: the sum of
    squares in two chains of 32 fused multiply-adds a lane, their sum and the half-wave exchange (34 roundings of a positive sum, halved by the
    square root: 17), the + 1e-6 (1/2), the hardware rsqrt (1 ulp = 2), coef * q_scale, * w, * h, the rounded product and the fused add (5/2)."""
    from nunchaku_amd.quantization.mxfp4 import dequantize_mxfp4

    got, o = _launch(dict(M=M, K=K, N=N, R=R, bias=bias, dtype=dtype, seed=M * K + N + R))
    T, ld = N // 3, -(-(M + 1) // 8) * 8
    A, W = dequantize_mxfp4(o["ac"], o["asc"])[:M].numpy(), dequantize_mxfp4(o["wc"], o["wsc"]).numpy()
    la16, lu64, b64 = o["la"][:M].to(DT[dtype]).double().numpy(), o["lu"].double().numpy(), np.zeros(N) if o["b"] is None else o["b"].double().numpy()
    h = A @ W.T + la16 @ lu64.T + b64
    e = (K + R + 2) * 2.0 ** -24 * (np.abs(A) @ np.abs(W).T + np.abs(la16) @ np.abs(lu64).T + np.abs(b64))
    g64, nat = got.cpu().double().numpy(), o["nat"][:M].double().numpy()
    assert np.isfinite(g64).all()
    for third, w in ((slice(0, T), o["nq"]), (slice(T, 2 * T), o["nk"])):
        ref, bound = _ref64(h[:, third], e[:, third], w.double().numpy(), nat, dtype)
        worst = (np.abs(g64[:, third] - ref) / bound).max()
        print(f"worst |out - rope(rmsnorm(ref))| / bound = {worst:.3f}")
        assert worst <= 1.0
    assert torch.equal(got, _launch(o)[0])  # deterministic
    plain = _launch(o, rope=False)[0]
    assert torch.equal(got[:, 2 * T:], plain[:, 2 * T:])
    vt = torch.full((T, ld), 7.0, dtype=DT[dtype], device="cuda")
    half = _launch(o, out_vt=vt, q_scale=0.5)[0]
    assert torch.equal(vt[:, :M], plain[:, 2 * T:].t()) and bool((vt[:, M:] == 7.0).all()) and bool((half[:, 2 * T:] == 7.0).all())
    normal = got[:, :T].abs() >= 2.0 ** -13  # (halving an fp16 result below 2^-13 rounds a second time: there, within one subnormal spacing)
    assert torch.equal(half[:, :T][normal], (got[:, :T] * 0.5)[normal]) and bool(((half[:, :T].float() - got[:, :T].float() * 0.5).abs() <= 2.0 ** -24).all())
    assert torch.equal(half[:, T:2 * T], got[:, T:2 * T]) and torch.equal(_launch(o, q_scale=1.0)[0], got)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_constructed_signs_through_the_bias(dtype):
    """all-zero activation codes: h32 = bias = +-2, so 2 rsqrt(4 + 1e-6) rounds to exactly 1.0 and Q is +-1, K (norm_k = 2) +-2.  The table is the
    identity where row + pair is even and a quarter turn where it is odd: (x, y) -> (-y, x)."""
    M, K, N, dt = 257, 128, 768, DT[dtype]
    sign = torch.where(torch.randint(0, 2, (N,), generator=torch.Generator().manual_seed(5)) == 1, 1.0, -1.0)
    odd = ((torch.arange(512)[:, None] + torch.arange(64)[None, :]) % 2).float()  # [M_pad, 64]
    got, _ = _launch(dict(M=M, K=K, N=N, R=0, bias=(2 * sign).to(dt), dtype=dtype, seed=3, a=torch.zeros(M, K, dtype=dt), nat=torch.stack([odd, 1 - odd], -1),
                          nq=torch.ones(128, dtype=dt), nk=torch.full((128,), 2.0, dtype=dt)))
    y = (sign * torch.tensor([1.0, 2.0, 0.0]).repeat_interleave(N // 3)).expand(M, N).reshape(M, N // 2, 2)
    turn = odd[:M].bool().repeat(1, N // 128)  # [M, N / 2]: pair j of every head
    want = torch.where(turn[..., None], torch.stack([-y[..., 1], y[..., 0]], -1), y).reshape(M, N)
    assert torch.equal(got[:, :512].cpu().float(), want[:, :512])


def test_module_path_and_refusals():
    from nunchaku_amd.models.embeddings import pack_rotemb
    from nunchaku_amd.models.linear import SVDQW4A4Linear
    from nunchaku_amd.ops import svdq_gemm_mxfp4
    from nunchaku_amd.ops.fused import fused_qkv_norm_rottary

    g, dt = torch.Generator().manual_seed(4), torch.bfloat16
    proj = SVDQW4A4Linear.from_float((torch.randn(768, 256, generator=g) / 16).to(dt), bias=torch.randn(768, generator=g).to(dt),
                                     proj_down=(torch.randn(256, 32, generator=g) / 8).to(dt), proj_up=(torch.randn(768, 32, generator=g) / 8).to(dt)).cuda()
    x = torch.randn(2, 33, 256, generator=g).to(dt).cuda()
    nq, nk = (SimpleNamespace(weight=(torch.rand(128, generator=g) + 0.5).to(dt).cuda()) for _ in range(2))
    ang = torch.rand(256, 64, generator=g)
    rot = pack_rotemb(torch.stack([ang.sin(), ang.cos()], -1).reshape(1, 256, 64, 1, 2)).cuda()
    vt, vt2 = torch.zeros(256, 72, dtype=dt, device="cuda"), torch.zeros(256, 72, dtype=dt, device="cuda")
    y = fused_qkv_norm_rottary(x, proj, nq, nk, rot, out_vt=vt, q_scale=0.25)
    qx, asc, la = proj.quantize(x.reshape(66, 256))
    hand = torch.zeros(66, 768, dtype=dt, device="cuda")
    svdq_gemm_mxfp4(qx, proj.qweight, asc, proj.wscales, out=hand, lora_act_in=la, lora_up=proj.proj_up, bias=proj.bias, rows=66,
                    norm_q=nq.weight, norm_k=nk.weight, rotary_emb=rot.reshape(256, 128), out_vt=vt2, q_scale=0.25)
    assert tuple(y.shape) == (2, 33, 768) and torch.equal(y.reshape(66, 768)[:, :512], hand[:, :512]) and torch.equal(vt, vt2) and bool(vt[:, :66].any())
    with pytest.raises(NotImplementedError, match="MXFP4"):
        fused_qkv_norm_rottary(x, proj, nq, nk, rot, output=(None, None, None))
    with pytest.raises(NotImplementedError, match="MXFP4"):
        fused_qkv_norm_rottary(x, proj, nq, nk, rot, ln=(None, None, None))
    z = lambda *s: torch.zeros(*s, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="qout"):
        svdq_gemm_mxfp4(qx, proj.qweight, asc, proj.wscales, rows=66, qout=z(256, 384), oscales=z(6, 256, 4), norm_q=nq.weight)
    with pytest.raises(ValueError, match="multiple of 384"):
        svdq_gemm_mxfp4(qx, proj.qweight[:640], asc, z(8, 640), rows=66, norm_q=nq.weight, norm_k=nk.weight, rotary_emb=rot.reshape(256, 128))
