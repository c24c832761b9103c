"""Time the MXFP4 GEMM and quantiser against their INT4 counterparts: svdq_gemm_mxfp4 vs svdq_gemm_w4a4 (plain epilogue, rank 32, bf16) and
svdq_quantize_mxfp4 vs svdq_quantize_w4a4_act_fuse_lora.  One process on one device; every arm is captured into a graph of `--launches`
launches and replayed (a timed window is 2 to 17 ms), the arms alternate, the figure is the median over `--rounds` replays per launch.  At every
timed GEMM shape the MXFP4 output is also compared with the fp32 product of the dequantised operands (`mxfp4_max_err_over_max_ref`; the INT4 arm
is only checked to be finite: its operands are another format, its result another number).  Prints one JSON line per row.

    python tools/bench_mxfp4_gemm.py [--rounds 15] [--launches 100] > profiles/mxfp4_gemm.txt

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--launches", type=int, default=100)
    a = ap.parse_args()
    print(json.dumps({"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "launches_per_replay": a.launches, "rank": RANK, "dtype": "bf16"}))
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
