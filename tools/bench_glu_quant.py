"""Timings of the gated feed-forward's middle on one MI355X (bench.py stays the flagship benchmark and is not involved).

``svdq_quantize_glu_halves`` (one launch: both halves of the projection output read in place, activation, product, low-rank down projection and
4-bit quantisation) against the sequence it replaces -- ``value, gate = y.chunk(2, -1)``, ``act(gate)``, the product, then
``svdq_quantize_w4a4_act_fuse_lora`` on the 16-bit result -- at (T, K) = (4096, 10240) (Z-Image, silu), (4096, 2560) and (1024, 5120) (SDXL, gelu),
rank 32, bf16 and fp16.  Both versions are timed as replays of a captured graph of ``--inner`` calls, alternating inside one process, the whole
round repeated: min / median / max per version, next to the byte bound 4.75 T K bytes at the project's copy figure of 6.29 TB/s.
(The sequence's K-sliced low-rank accumulator is cleared by a copy of zeros and passed as already zero: a memset is not recorded into a graph.)

    python tools/bench_glu_quant.py [--repeats 7] [--inner 20] [--out profiles/glu_quant.txt]
"""

import argparse
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from tools.bench_sdxl_attention import alternate, line  # noqa: E402

SHAPES = [(4096, 10240, "silu"), (4096, 2560, "gelu"), (1024, 5120, "gelu")]  # (T, K, act)
COPY_TBS = 6.29


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from nunchaku_amd.models.linear import SVDQW4A4Linear
    from nunchaku_amd.ops.quantize import svdq_quantize_w4a4_act_fuse_lora_cuda

    if not torch.cuda.is_available():
        raise SystemExit("bench_glu_quant: no GPU: a timing needs the MI355X (nothing is measured on the CPU)")
    torch.cuda.set_device(0)
    lines = []

    def emit(s):
        lines.append(s)
        print(s, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    emit(f"# tools/bench_glu_quant.py --repeats {args.repeats} --inner {args.inner}: ms per call, captured replays, versions alternated")
    for dtype in (torch.bfloat16, torch.float16):
        for T, K, act in SHAPES:
            torch.manual_seed(0)
            lin = SVDQW4A4Linear(K, 128, rank=32, bias=False, torch_dtype=dtype, device="cuda")
            with torch.no_grad():
                lin.proj_down.copy_(torch.randn_like(lin.proj_down.float()) * 0.02)
                lin.smooth_factor.copy_(torch.rand_like(lin.smooth_factor.float()) + 0.5)
            y = torch.randn(T, 2 * K, device="cuda").to(dtype)
            fn = F.silu if act == "silu" else F.gelu
            la = torch.empty(T, 32, dtype=torch.float32, device="cuda")
            zeros = torch.zeros_like(la)

            def sequence():
                value, gate = y.chunk(2, dim=-1)
                x = value * fn(gate)
                la.copy_(zeros)
                return svdq_quantize_w4a4_act_fuse_lora_cuda(x, lora_down=lin.proj_down, smooth=lin.smooth_factor, lora_act_out=la, lora_act_zeroed=True)

            def fused():
                return lin.quantize_glu(y, act)

            lin._ensure_layout()
            res = alternate({"sequence": sequence, "fused": fused}, args.repeats, args.inner, graph=True)
            bound = 4.75 * T * K / (COPY_TBS * 1e12) * 1e3
            emit(f"{str(dtype).split('.')[1]} T={T} K={K} {act}: byte bound {bound:.4f} ms")
            for k, xs in res.items():
                emit(line(f"  {k}", xs, f"  {min(xs) / bound:5.2f} x the bound"))
            emit(f"  fused / sequence (medians) = {sorted(res['fused'])[len(res['fused']) // 2] / sorted(res['sequence'])[len(res['sequence']) // 2]:.3f}")


if __name__ == "__main__":
    main()
