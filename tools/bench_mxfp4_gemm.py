"""Time the MXFP4 GEMM and quantiser against their INT4 counterparts: svdq_gemm_mxfp4 vs svdq_gemm_w4a4 (plain epilogue, rank 32, bf16) and
svdq_quantize_mxfp4 vs svdq_quantize_w4a4_act_fuse_lora.  One process on one device; every arm is captured into a graph of `--launches`
launches and replayed (a timed window is 2 to 17 ms), the arms alternate, the figure is the median over `--rounds` replays per launch.  `--mlp`
times fc1 of an MLP instead (M 4608, K 3072, N 12288): (a) the MXFP4 GELU_QUANT launch, (b) what produces the same operands without it -- plain
svdq_gemm_mxfp4, torch's tanh GELU, svdq_quantize_mxfp4 with fc2's lora_down and smooth -- and (c) the INT4 GELU_QUANT launch.  `--qkv` times
a QKV projection (M 4608, K 3072, N 9216): (a) the MXFP4 RMSNorm + RoPE launch with out_vt and q_scale, (b) plain svdq_gemm_mxfp4 plus the torch
ops for the per-head norm, the rotation and the V transpose, (c) the INT4 RMSNORM_ROPE launch.  `--glu` times the gated projection of a SwiGLU /
GEGLU feed-forward at three (M, K, 2 Hd) shapes: (a) the MXFP4 GLU_QUANT launch, (b) plain svdq_gemm_mxfp4, torch's chunk / activation / product,
svdq_quantize_mxfp4 with the second projection's lora_down and smooth, (c) the INT4 pair svdq_gemm_w4a4 + svdq_quantize_glu_halves.  At every
timed GEMM shape the MXFP4 output is also compared with the fp32 product of the dequantised operands (`mxfp4_max_err_over_max_ref`; the INT4 arm
is only checked to be finite: its operands are another format, its result another number).  Prints one JSON line per row.

    python tools/bench_mxfp4_gemm.py [--rounds 15] [--launches 100] > profiles/mxfp4_gemm.txt
    python tools/bench_mxfp4_gemm.py --mlp > profiles/mxfp4_gelu_quant.txt
    python tools/bench_mxfp4_gemm.py --qkv > profiles/mxfp4_qkv.txt
    python tools/bench_mxfp4_gemm.py --glu > profiles/mxfp4_glu_quant.txt

Not measured here: hardware counters (a run of their own), end-to-end models (no model class runs MXFP4).
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nunchaku_amd.models.linear import SVDQW4A4Linear  # noqa: E402
from nunchaku_amd.quantization.mxfp4 import dequantize_mxfp4, unpack_scales_mxfp4  # noqa: E402

GEMM_SHAPES = [(4608, 3072, 3072), (4608, 12288, 3072), (1536, 3072, 3072)]  # (M, K, N)
QUANT_SHAPES = [(4608, 3072), (4608, 12288)]  # (M, K)
RANK = 32


def layers(K, N):
    g = torch.Generator(device="cuda").manual_seed(0)
    int4 = SVDQW4A4Linear(K, N, rank=RANK, device="cuda")
    with torch.no_grad():
        from nunchaku_amd.models.linear import synthetic_codes_
        synthetic_codes_(int4.qweight, int4.wscales, K, g)
        for t in (int4.bias, int4.proj_down, int4.proj_up):
            t.copy_(torch.randn(t.shape, generator=g, device="cuda") * 0.05)
        int4.smooth_factor.fill_(1.0)
    w = torch.randn(N, K, generator=g, device="cuda").bfloat16() * K ** -0.5
    mx = SVDQW4A4Linear.from_float(w, bias=torch.randn(N, generator=g, device="cuda").bfloat16(),
                                   proj_down=(torch.randn(K, RANK, generator=g, device="cuda") * 0.05).bfloat16(),
                                   proj_up=(torch.randn(N, RANK, generator=g, device="cuda") * 0.05).bfloat16())
    return int4, mx


def captured(fn, launches):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(launches):
            fn()
    return graph


def alternate(arms, rounds, launches):
    """arms: {name: graph} -> {name: median microseconds per launch}"""
    times = {k: [] for k in arms}
    for g in arms.values():
        g.replay()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for name, g in arms.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            g.replay()
            e.record()
            e.synchronize()
            times[name].append(s.elapsed_time(e) * 1e3 / launches)
    return {k: statistics.median(v) for k, v in times.items()}, {k: (min(v), max(v)) for k, v in times.items()}


MLP_SHAPE = (4608, 3072, 12288)  # (M, K, N) of fc1


def mlp(a):
    from nunchaku_amd.ops import svdq_gemm_mxfp4, svdq_quantize_mxfp4
    from nunchaku_amd.mode import alloc_lora_act
    from nunchaku_amd.ops.gemm import svdq_gemm_w4a4_cuda

    M, K, N = MLP_SHAPE
    (i1, m1), (i2, m2) = layers(K, N), layers(N, K)
    for lin in (i1, i2, m1, m2):
        lin._ensure_layout()
    x = torch.randn(M, K, device="cuda").bfloat16()
    qi, qm = i1.quantize(x), m1.quantize(x)
    dev = x.device
    qh, sh, lh = torch.empty(M, N // 2, dtype=torch.uint8, device=dev), torch.empty(N // 128, M, 4, dtype=torch.uint8, device=dev), torch.empty(M, RANK, device=dev)
    hid = torch.empty(M, N, dtype=torch.bfloat16, device=dev)
    qh_i, sh_i = torch.empty(M, N * 3 // 4, dtype=torch.uint8, device=dev), torch.empty(N // 64, M, dtype=torch.bfloat16, device=dev)
    common = dict(lora_act_in=qm[2], lora_up=m1.proj_up, bias=m1.bias, rows=M)

    def fused():
        svdq_gemm_mxfp4(qm[0], m1.qweight, qm[1], m1.wscales, qout=qh, oscales=sh, lora_down=m2.proj_down, lora_act_out=lh, smooth_factor=m2.smooth_factor, **common)

    def unfused():
        svdq_gemm_mxfp4(qm[0], m1.qweight, qm[1], m1.wscales, out=hid, **common)
        return svdq_quantize_mxfp4(torch.nn.functional.gelu(hid, approximate="tanh"), lora_down=m2.proj_down, smooth=m2.smooth_factor)

    def int4():  # as ops.fused.fused_gelu_mlp launches it
        lh_i, zeroed = alloc_lora_act(M, RANK, dev, None)
        svdq_gemm_w4a4_cuda(act=qi[0], wgt=i1.qweight, qout=qh_i, ascales=qi[1], wscales=i1.wscales, oscales=sh_i, lora_act_in=qi[2], lora_up=i1.proj_up,
                            lora_down=i2.proj_down, lora_act_out=lh_i, bias=i1.bias, smooth_factor=i2.smooth_factor, lora_scales=getattr(i1, "lora_scales", None), lora_act_zeroed=zeroed)

    fused()
    ref = unfused()  # the fused launch rounds gelu once from fp32, this path twice: the codes agree except next to a rounding boundary
    agree = float((qh == ref[0]).float().mean())
    assert agree > 0.98 and bool(lh.isfinite().all()), agree
    arms = {"mxfp4_fused": captured(fused, a.launches), "mxfp4_gemm_gelu_quantize": captured(unfused, a.launches), "int4_fused": captured(int4, a.launches)}
    med, span = alternate(arms, a.rounds, a.launches)
    row = {"op": "fc1_gelu_quant", "M": M, "K": K, "N": N, "code_bytes_equal_to_unfused": round(agree, 4)}
    for k in arms:
        row[k + "_us"], row[k + "_min_max_us"] = round(med[k], 2), [round(v, 2) for v in span[k]]
    row["fused_over_unfused"], row["fused_over_int4"] = round(med["mxfp4_fused"] / med["mxfp4_gemm_gelu_quantize"], 3), round(med["mxfp4_fused"] / med["int4_fused"], 3)
    print(json.dumps(row), flush=True)


QKV_SHAPE = (4608, 3072, 9216)  # (M, K, N): 24 heads


def qkv(a):
    from nunchaku_amd.models.embeddings import pack_rotemb
    from nunchaku_amd.ops import svdq_gemm_mxfp4
    from nunchaku_amd.ops.gemm import svdq_gemm_w4a4_cuda

    M, K, N = QKV_SHAPE
    int4, mx = layers(K, N)
    for lin in (int4, mx):
        lin._ensure_layout()
    dev, H = torch.device("cuda"), N // 384
    x = torch.randn(M, K, device=dev).bfloat16()
    qi, qm = int4.quantize(x), mx.quantize(x)
    ang = torch.rand(M, 64, device=dev) * 6.283185
    nat = torch.stack([ang.sin(), ang.cos()], dim=-1)  # [M, 64, (sin, cos)]
    rot = pack_rotemb(nat.reshape(1, M, 64, 1, 2)).reshape(M, 128)
    nq, nk = (torch.rand(128, device=dev) + 0.5).bfloat16(), (torch.rand(128, device=dev) + 0.5).bfloat16()
    out, out_i, hid = (torch.empty(M, N, dtype=torch.bfloat16, device=dev) for _ in range(3))
    vt, vt_i, vt_u = (torch.empty(N // 3, M, dtype=torch.bfloat16, device=dev) for _ in range(3))
    common = dict(lora_act_in=qm[2], lora_up=mx.proj_up, bias=mx.bias, rows=M)
    sin, cos = nat[None, :, :, 0], nat[None, :, :, 1]  # [1, M, 64]

    def fused():
        svdq_gemm_mxfp4(qm[0], mx.qweight, qm[1], mx.wscales, out=out, norm_q=nq, norm_k=nk, rotary_emb=rot, out_vt=vt, q_scale=0.125, **common)

    def unfused():  # the 16-bit torch ops a caller without the epilogue runs: per-head RMSNorm, rotation, the V^T copy attention reads
        svdq_gemm_mxfp4(qm[0], mx.qweight, qm[1], mx.wscales, out=hid, **common)
        res = []
        for third, w, s in ((hid[:, :N // 3], nq, 0.125), (hid[:, N // 3:2 * N // 3], nk, 1.0)):
            t = third.view(M, H, 128).float()
            t = (t * torch.rsqrt(t.pow(2).mean(-1, keepdim=True) + 1e-6) * (w.float() * s)).view(M, H, 64, 2).permute(1, 0, 2, 3)
            res.append(torch.stack([t[..., 0] * cos - t[..., 1] * sin, t[..., 0] * sin + t[..., 1] * cos], dim=-1).bfloat16())
        vt_u.copy_(hid[:, 2 * N // 3:].t())
        return res  # [H, M, 64, 2] each

    def int4_fused():  # as ops.fused.fused_qkv_norm_rottary launches it
        svdq_gemm_w4a4_cuda(act=qi[0], wgt=int4.qweight, out=out_i, ascales=qi[1], wscales=int4.wscales, lora_act_in=qi[2], lora_up=int4.proj_up, bias=int4.bias,
                            norm_q=nq, norm_k=nk, rotary_emb=rot, out_vt=vt_i, lora_scales=getattr(int4, "lora_scales", None), q_scale=0.125)

    fused()
    ref = unfused()  # rounds the projection to bf16 before the norm, the fused launch does not: a few bf16 spacings apart at most
    got = out.view(M, 3, H, 64, 2).permute(1, 2, 0, 3, 4).float()
    err = max(float((got[i] - ref[i].float()).abs().max() / ref[i].float().abs().max()) for i in range(2))
    assert err < 2.0 ** -5 and torch.equal(vt, vt_u), err
    arms = {"mxfp4_fused": captured(fused, a.launches), "mxfp4_gemm_torch_norm_rope_vt": captured(unfused, a.launches), "int4_fused": captured(int4_fused, a.launches)}
    med, span = alternate(arms, a.rounds, a.launches)
    row = {"op": "qkv_rmsnorm_rope", "M": M, "K": K, "N": N, "max_err_over_max_ref_vs_unfused": round(err, 5), "vt_equal_to_unfused": True}
    for k in arms:
        row[k + "_us"], row[k + "_min_max_us"] = round(med[k], 2), [round(v, 2) for v in span[k]]
    row["fused_over_unfused"], row["fused_over_int4"] = round(med["mxfp4_fused"] / med["mxfp4_gemm_torch_norm_rope_vt"], 3), round(med["mxfp4_fused"] / med["int4_fused"], 3)
    print(json.dumps(row), flush=True)


GLU_SHAPES = [(4096, 3840, 20480, "silu"), (4096, 640, 5120, "gelu"), (1024, 1280, 10240, "gelu")]  # (M, K, 2 Hd, act): Z-Image, SDXL 640 / 1280


def glu(a):
    from nunchaku_amd.ops import svdq_gemm_mxfp4, svdq_quantize_mxfp4

    for M, K, N, act in GLU_SHAPES:
        Hd = N // 2
        (i1, m1), (i2, m2) = layers(K, N), layers(Hd, K)
        for lin in (i1, i2, m1, m2):
            lin._ensure_layout()
        dev = torch.device("cuda")
        x = torch.randn(M, K, device=dev).bfloat16()
        qi, qm = i1.quantize(x), m1.quantize(x)
        qh, sh, lh = torch.empty(M, Hd // 2, dtype=torch.uint8, device=dev), torch.empty(Hd // 128, M, 4, dtype=torch.uint8, device=dev), torch.empty(M, RANK, device=dev)
        hid, hid_i = torch.empty(M, N, dtype=torch.bfloat16, device=dev), torch.empty(M, N, dtype=torch.bfloat16, device=dev)
        common = dict(lora_act_in=qm[2], lora_up=m1.proj_up, bias=m1.bias, rows=M)
        fn = torch.nn.functional.silu if act == "silu" else torch.nn.functional.gelu

        def fused():
            svdq_gemm_mxfp4(qm[0], m1.qweight, qm[1], m1.wscales, qout=qh, oscales=sh, lora_down=m2.proj_down, lora_act_out=lh, smooth_factor=m2.smooth_factor,
                            glu=act, **common)

        def unfused():
            svdq_gemm_mxfp4(qm[0], m1.qweight, qm[1], m1.wscales, out=hid, **common)
            v, g = hid.chunk(2, dim=-1)
            return svdq_quantize_mxfp4(v * fn(g), lora_down=m2.proj_down, smooth=m2.smooth_factor)

        def int4():  # as fused_glu_feed_forward launches it on INT4 layers
            i1.forward_quant(*qi, hid_i)
            return i2.quantize_glu(hid_i, act)

        fused()
        ref = unfused()  # torch's activation is another fp32 expression: the codes agree except next to a rounding boundary
        agree = float((qh == ref[0]).float().mean())
        assert agree > 0.98 and bool(lh.isfinite().all()) and bool(int4()[2].isfinite().all()), agree
        arms = {"mxfp4_fused": captured(fused, a.launches), "mxfp4_gemm_torch_glu_quantize": captured(unfused, a.launches), "int4_gemm_quantize_glu": captured(int4, a.launches)}
        med, span = alternate(arms, a.rounds, a.launches)
        row = {"op": "glu_quant", "act": act, "M": M, "K": K, "N": N, "code_bytes_equal_to_unfused": round(agree, 4)}
        for k in arms:
            row[k + "_us"], row[k + "_min_max_us"] = round(med[k], 2), [round(v, 2) for v in span[k]]
        row["fused_over_unfused"], row["fused_over_int4"] = round(med["mxfp4_fused"] / med["mxfp4_gemm_torch_glu_quantize"], 3), round(med["mxfp4_fused"] / med["int4_gemm_quantize_glu"], 3)
        row["fused_tflops"] = round(2.0 * M * K * N / med["mxfp4_fused"] / 1e6, 1)
        print(json.dumps(row), flush=True)
        del arms, hid, hid_i


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--mlp", action="store_true")
    ap.add_argument("--qkv", action="store_true")
    ap.add_argument("--glu", action="store_true")
    a = ap.parse_args()
    print(json.dumps({"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "launches_per_replay": a.launches, "rank": RANK, "dtype": "bf16"}))
    if a.mlp:
        return mlp(a)
    if a.qkv:
        return qkv(a)
    if a.glu:
        return glu(a)
    for M, K, N in GEMM_SHAPES:
        int4, mx = layers(K, N)
        x = torch.randn(M, K, device="cuda").bfloat16()
        qi, qm = int4.quantize(x), mx.quantize(x)
        oi, om = torch.empty(M, N, dtype=torch.bfloat16, device="cuda"), torch.empty(M, N, dtype=torch.bfloat16, device="cuda")
        arms = {"int4": captured(lambda: int4.forward_quant(*qi, oi), a.launches), "mxfp4": captured(lambda: mx.forward_quant(*qm, om), a.launches)}
        med, span = alternate(arms, a.rounds, a.launches)
        with torch.no_grad():
            A, W = dequantize_mxfp4(qm[0], unpack_scales_mxfp4(qm[1]))[:M].float(), dequantize_mxfp4(mx.qweight, mx.state_dict()["wscales"]).float()
            ref = A @ W.t() + qm[2][:M].bfloat16().float() @ mx.proj_up.float().t() + mx.bias.float()
            err = float((om.float() - ref).abs().max() / ref.abs().max())
        assert bool(oi.isfinite().all()) and err < 2.0 ** -7, err  # one bf16 rounding of the largest output is 2^-9 of it
        del A, W, ref
        print(json.dumps({"op": "gemm", "mxfp4_max_err_over_max_ref": round(err, 5), "M": M, "K": K, "N": N, "int4_us": round(med["int4"], 2), "mxfp4_us": round(med["mxfp4"], 2),
                          "mxfp4_over_int4": round(med["mxfp4"] / med["int4"], 3), "mxfp4_tflops": round(2.0 * M * K * N / med["mxfp4"] / 1e6, 1),
                          "int4_min_max_us": [round(v, 2) for v in span["int4"]], "mxfp4_min_max_us": [round(v, 2) for v in span["mxfp4"]]}), flush=True)
    for M, K in QUANT_SHAPES:
        int4, mx = layers(K, 128)
        x = torch.randn(M, K, device="cuda").bfloat16()
        arms = {"int4": captured(lambda: int4.quantize(x), a.launches), "mxfp4": captured(lambda: mx.quantize(x), a.launches)}
        med, span = alternate(arms, a.rounds, a.launches)
        print(json.dumps({"op": "quantize", "M": M, "K": K, "int4_us": round(med["int4"], 2), "mxfp4_us": round(med["mxfp4"], 2),
                          "mxfp4_over_int4": round(med["mxfp4"] / med["int4"], 3), "mxfp4_in_GBps": round(2.0 * M * K / med["mxfp4"] / 1e3, 1),
                          "int4_min_max_us": [round(v, 2) for v in span["int4"]], "mxfp4_min_max_us": [round(v, 2) for v in span["mxfp4"]]}), flush=True)


if __name__ == "__main__":
    main()
