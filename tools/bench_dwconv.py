"""Timings of SANA's depthwise 3x3 convolution on one MI355X (bench.py stays the flagship benchmark and is not involved).

``svdq_dwconv3x3`` (one launch; x and out are the [B, H*W, C] token rows of the feed-forward's first GEMM, bf16) at SANA-1.6B's C = 11264 with
H x W in {32x32, 64x64, 128x128} and B in {1, 2}, and at SANA-0.6B's C = 5760 with 32x32 and 64x64, against

  (a) ``torch.nn.functional.conv2d(groups=C, padding=1)`` with the bias on the channels_last view of the same tensor;
  (b) its byte bound: 4*B*H*W*C bytes (x read and out written once, 16-bit) at the chip's measured copy figure.

Outputs of the kernel and of (a) are compared at every size before anything is timed.

Event-bracketed, warm; the versions alternate inside one process and the whole round is repeated: min / median / max per version.

    python tools/bench_dwconv.py [--repeats 7] [--inner 20] [--out profiles/dwconv.txt]
"""

import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

COPY_TBS = 6.29  # float4 copy on MI355X
SIZES = [(11264, 32, 32), (11264, 64, 64), (11264, 128, 128), (5760, 32, 32), (5760, 64, 64)]  # (C, H, W)


def timed(fn, inner):
    """ms per call of ``inner`` back-to-back calls between two events"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def alternate(versions: dict, repeats: int, inner: int) -> dict:
    for fn in versions.values():  # warm
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in versions}
    for _ in range(repeats):
        for k, fn in versions.items():
            out[k].append(timed(fn, inner))
    return out


def line(name, xs, extra=""):
    return f"{name:<44} min {min(xs):9.4f}  median {statistics.median(xs):9.4f}  max {max(xs):9.4f} ms  (n={len(xs)}){extra}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--batches", type=int, nargs="+", default=(1, 2))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from nunchaku_amd.ops.conv import dwconv3x3

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    lines = []

    def emit(s):
        lines.append(s)
        print(s, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    emit(f"device: {torch.cuda.get_device_name(dev)}; repeats {args.repeats} x inner {args.inner}, versions alternated")
    emit(f"depthwise 3x3 convolution, stride 1, zero padding 1, channels-last [B, H, W, C], bf16, with bias; one launch per call; "
         f"byte bound = 4*B*H*W*C bytes at {COPY_TBS} TB/s")
    g = torch.Generator(device=dev).manual_seed(0)
    for C, H, W in SIZES:
        for B in args.batches:
            x = torch.randn(B, H, W, C, device=dev, generator=g).bfloat16()
            w = (torch.randn(C, 3, 3, 1, device=dev, generator=g) / 3).bfloat16()
            b = torch.randn(C, device=dev, generator=g).bfloat16()
            out = torch.empty_like(x)
            x_nchw, w_nchw = x.permute(0, 3, 1, 2), w.view(C, 1, 3, 3)  # (the channels_last view of the same memory)
            assert x_nchw.is_contiguous(memory_format=torch.channels_last)

            def torch_conv():
                return F.conv2d(x_nchw, w_nchw, b, padding=1, groups=C)

            ref = torch_conv().permute(0, 2, 3, 1)
            diff = (dwconv3x3(x, w, b, out=out).float() - ref.float()).abs().max().item()
            t = alternate({"kernel": lambda: dwconv3x3(x, w, b, out=out), "torch": torch_conv}, args.repeats, args.inner)
            med = {k: statistics.median(xs) for k, xs in t.items()}
            bound_ms = 4 * B * H * W * C / (COPY_TBS * 1e12) * 1e3
            emit(f"C = {C}, H x W = {H} x {W}, B = {B}: byte bound {bound_ms:.4f} ms; max |kernel - torch conv2d| = {diff:.3g} "
                 f"(max |ref| {ref.float().abs().max().item():.3g})")
            emit(line("  svdq_dwconv3x3 (1 launch)", t["kernel"],
                      f"  {med['kernel'] / bound_ms:.2f} x the byte bound ({bound_ms / med['kernel']:.2f} of it); kernel / torch = {med['kernel'] / med['torch']:.3f}"))
            emit(line("  torch conv2d(groups=C), channels_last + bias", t["torch"]))
            del x, out, ref


if __name__ == "__main__":
    main()
