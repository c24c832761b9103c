"""Timings of SANA's ReLU linear attention on one MI355X (bench.py stays the flagship benchmark and is not involved).

``svdq_linear_attention`` (3 launches per call: chunk reduction, finishing sum, apply; Q, K and V read in place from the packed
[B, T, 3*H*32] output of the QKV projection) at T in {1024, 4096, 16384}, H in {36, 72}, B in {1, 2}, bf16, against

  (a) the torch-op restatement a user would run without it: relu, fp32 einsums for vk and the products with Q, divide, cast;
  (b) its byte bound: B*T*H*256 bytes (Q, K, V read and out written once, 16-bit) at the chip's measured copy figure.

The vk-only call (2 launches: what the compatibility path of ``ops.gemm_w4a4(out_vk=...)`` uses) is timed beside it: the share of the
reduction.  Outputs of the kernel and of (a) are compared at every size before anything is timed.

Event-bracketed, warm; the versions alternate inside one process and the whole round is repeated: min / median / max per version.

    python tools/bench_linear_attention.py [--repeats 7] [--inner 40] [--out profiles/linear_attention.txt]
"""

import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

COPY_TBS = 6.29  # float4 copy on MI355X
LAUNCHES = 3


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


def torch_restatement(qkv, H, eps=1e-6):
    B, T, W = qkv.shape
    hd = W // 3
    q = torch.relu(qkv[..., :hd]).float().view(B, T, H, 32)
    kv = qkv[..., hd:].view(B, T, H, 64)
    k, v = torch.relu(kv[..., :32]).float(), kv[..., 32:].float()
    vk = torch.einsum("bthi,bthj->bhij", v, k)
    ksum = k.sum(dim=1)
    num = torch.einsum("bthj,bhij->bthi", q, vk)
    den = torch.einsum("bthj,bhj->bth", q, ksum) + eps
    return (num / den[..., None]).to(qkv.dtype).reshape(B, T, hd)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=40)
    ap.add_argument("--tokens", type=int, nargs="+", default=(1024, 4096, 16384))
    ap.add_argument("--heads", type=int, nargs="+", default=(36, 72))
    ap.add_argument("--batches", type=int, nargs="+", default=(1, 2))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from nunchaku_amd._C import ops
    from nunchaku_amd.ops.attention import linear_attention

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    lines = [f"device: {torch.cuda.get_device_name(dev)}; repeats {args.repeats} x inner {args.inner}, versions alternated",
             f"ReLU linear attention, head dim 32, bf16, Q / K / V inside a packed [B, T, 3*H*32] buffer; {LAUNCHES} launches per call "
             f"(2 for vk alone); byte bound = B*T*H*256 bytes at {COPY_TBS} TB/s"]
    g = torch.Generator(device=dev).manual_seed(0)
    for T in args.tokens:
        for H in args.heads:
            for B in args.batches:
                hd = H * 32
                qkv = torch.randn(B, T, 3 * hd, device=dev, generator=g).bfloat16()
                out = torch.empty(B, T, hd, device=dev, dtype=torch.bfloat16)
                vk = torch.empty(B, H, 33, 32, device=dev)
                kv = qkv[..., hd:].unflatten(-1, (H, 64))
                ref = torch_restatement(qkv, H)
                diff = (linear_attention(qkv, H, out=out).float() - ref.float()).abs().max().item()
                t = alternate({"kernel": lambda: linear_attention(qkv, H, out=out), "vk": lambda: ops.linear_attention(None, kv, None, vk=vk),
                               "torch": lambda: torch_restatement(qkv, H)}, args.repeats, args.inner)
                med = {k: statistics.median(xs) for k, xs in t.items()}
                bound_ms = B * T * H * 256 / (COPY_TBS * 1e12) * 1e3
                lines.append(f"T = {T}, H = {H}, B = {B}: byte bound {bound_ms:.4f} ms; max |kernel - torch restatement| = {diff:.3g} "
                             f"(max |ref| {ref.float().abs().max().item():.3g})")
                lines.append(line(f"  svdq_linear_attention ({LAUNCHES} launches)", t["kernel"],
                                  f"  {med['kernel'] / bound_ms:.2f} x the byte bound; kernel / torch = {med['kernel'] / med['torch']:.3f}"))
                lines.append(line("  vk alone (2 launches)", t["vk"]))
                lines.append(line("  torch-op restatement (fp32 einsums)", t["torch"]))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
