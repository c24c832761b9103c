"""Timings of the back half of SANA's feed-forward on one MI355X (bench.py stays the flagship benchmark and is not involved).

``svdq_quantize_dwconv_glu`` (one launch: the depthwise 3x3 convolution, the interleaved GLU, the low-rank down projection and the 4-bit
quantisation) against the two launches it replaces on the same buffers -- ``dwconv3x3`` into the ``2K``-wide buffer, then
``svdq_quantize_w4a4_act_fuse_lora(fuse_glu=True)`` -- bf16, rank 32: C = 11264 / K = 5632 (SANA-1.6B) at 32x32, 64x64 and 128x128 tokens with
B = 1 and 2, and C = 5760 / K = 2944 (SANA-0.6B) at 64x64 with B = 2.  Both arms are timed as replays of a captured graph of ``--inner`` calls,
alternating inside one process, the whole round repeated: min / median / max per arm, next to the byte bound
``2 B T C + 0.75 M_pad K + scales + lora_act`` at the project's copy figure of 6.29 TB/s.
(The two-launch arm's K-sliced low-rank accumulator is cleared by a copy of zeros and passed as already zero: a memset is not recorded into a graph.)

    python tools/bench_sana_conv_quant.py [--repeats 7] [--inner 20] [--out profiles/sana_conv_quant.txt]
"""

import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from tools.bench_sdxl_attention import alternate, line  # noqa: E402

SHAPES = [(11264, 5632, s, B) for s in (32, 64, 128) for B in (1, 2)] + [(5760, 2944, 64, 2)]  # (C, K, grid side, B)
COPY_TBS = 6.29
RANK = 32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from nunchaku_amd.models.linear import SVDQW4A4Linear
    from nunchaku_amd.ops.conv import dwconv3x3
    from nunchaku_amd.ops.quantize import svdq_quantize_w4a4_act_fuse_lora_cuda

    if not torch.cuda.is_available():
        raise SystemExit("bench_sana_conv_quant: no GPU: a timing needs the MI355X (nothing is measured on the CPU)")
    torch.cuda.set_device(0)
    lines = []

    def emit(s):
        lines.append(s)
        print(s, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    emit(f"# tools/bench_sana_conv_quant.py --repeats {args.repeats} --inner {args.inner}: ms per call, captured replays, arms alternated, bf16, rank {RANK}")
    dtype = torch.bfloat16
    for C, K, side, B in SHAPES:
        torch.manual_seed(0)
        T = side * side
        M = B * T
        M_pad = (M + 255) // 256 * 256
        lin = SVDQW4A4Linear(K, 128, rank=RANK, bias=False, torch_dtype=dtype, device="cuda")
        with torch.no_grad():
            lin.proj_down.copy_(torch.randn_like(lin.proj_down.float()) * 0.02)
            lin.smooth_factor.copy_(torch.rand_like(lin.smooth_factor.float()) + 0.5)
        y = torch.randn(B, T, C, device="cuda").to(dtype)
        w = (torch.randn(C, 3, 3, 1, device="cuda") / 3).to(dtype)
        b = torch.randn(C, device="cuda").to(dtype)
        wide = torch.zeros(B, T, 2 * K, dtype=dtype, device="cuda")
        la = torch.empty(M_pad, RANK, dtype=torch.float32, device="cuda")
        zeros = torch.zeros_like(la)

        def two_launches():
            dwconv3x3(y, w, b, height=side, width=side, out=wide[..., :C])
            la.copy_(zeros)
            return svdq_quantize_w4a4_act_fuse_lora_cuda(wide.view(M, 2 * K), lora_down=lin.proj_down, smooth=lin.smooth_factor, fuse_glu=True,
                                                         lora_act_out=la, lora_act_zeroed=True)

        def fused():
            return lin.quantize_dwconv_glu(y, w, b, side, side)

        lin._ensure_layout()
        same = all(torch.equal(p, q) for p, q in zip(two_launches()[:2], fused()[:2]))
        res = alternate({"two launches": two_launches, "fused": fused}, args.repeats, args.inner, graph=True)
        nbytes = 2 * B * T * C + 0.75 * M_pad * K + 2 * M_pad * (K // 64) + 4 * M_pad * RANK
        bound = nbytes / (COPY_TBS * 1e12) * 1e3
        emit(f"C={C} K={K} {side}x{side} B={B}: byte bound {bound:.4f} ms, codes and scales equal in both arms: {same}")
        for k, xs in res.items():
            emit(line(f"  {k}", xs, f"  {min(xs) / bound:5.2f} x the bound"))
        med = {k: sorted(xs)[len(xs) // 2] for k, xs in res.items()}
        emit(f"  fused / two launches (medians) = {med['fused'] / med['two launches']:.3f}" + ("  SLOWER" if med["fused"] > med["two launches"] else ""))
        del y, wide, la, zeros, lin
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
