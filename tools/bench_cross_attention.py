"""Timings of SANA's cross-attention on one MI355X (bench.py stays the flagship benchmark and is not involved).

``svdq_cross_attention`` (one launch; Q read in place from the ceil128(H*D)-wide rows of q_linear, K / V from the two column halves of
kv_linear's output, the key ranges read on the device; bf16) at SANA-1.6B's 20 x 112 and SANA-0.6B's 16 x 72 heads, T in {1024, 4096, 16384}
image tokens, B in {2, 3}, with 300 text tokens for every sample and with a ragged set ((300, 37) / (300, 37, 120)), against

  (a) the torch restatement of the same run: per sample ``scaled_dot_product_attention`` on the sliced keys, with the copies and transposes
      it needs (Q's column slice to [1, H, T, D], K / V slices to [1, H, n, D], the result back to token-major rows of the output);
  (b) its byte bound: Q read, out written and the samples' K / V rows read once (16-bit) at the chip's measured copy figure.

Outputs of the kernel and of (a) are compared at every size before anything is timed.

Event-bracketed, warm; the versions alternate inside one process and the whole round is repeated: min / median / max per version.

    python tools/bench_cross_attention.py [--repeats 7] [--inner 20] [--out profiles/cross_attention.txt]

``--key-series`` times the kernel alone against the number of keys per sample (64 .. 320, every sample the same count) at T = 16384, B = 3 and
T = 4096, B = 2 for 20 x 112, 16 x 72 and 18 x 128 heads: what a 64-key chunk costs and what does not depend on the chunks.  A CU holds one
workgroup at every point of the series (8 waves of 134 - 172 VGPRs: registers, not the LDS image) (``--out profiles/cross_attention_key_series.txt``).
"""

import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

COPY_TBS = 6.29  # float4 copy on MI355X
HEADS = [(20, 112), (16, 72)]
TOKENS = [1024, 4096, 16384]
RAGGED = (300, 37, 120)


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


def key_series(cross_attention, dev, args, emit):
    emit("svdq_cross_attention alone, bf16, every sample with the same key count; LDS = keys rounded up to 64 x (K row + 2 D) bytes; "
         "one workgroup (2 waves per SIMD) per CU at every size, by registers")
    g = torch.Generator(device=dev).manual_seed(0)
    for H, D in HEADS + [(18, 128)]:
        hd = H * D
        for T, B in ((16384, 3), (4096, 2)):
            q = torch.randn(B, T, (hd + 127) // 128 * 128, device=dev, generator=g).bfloat16()
            out = torch.empty(B, T, hd, device=dev, dtype=torch.bfloat16)
            for n in (64, 128, 192, 256, 320):
                kv = torch.randn(B * n, 2 * hd, device=dev, generator=g).bfloat16()
                cu = torch.arange(0, (B + 1) * n, n, dtype=torch.int32, device=dev)
                t = alternate({"kernel": lambda: cross_attention(q, kv[:, :hd], kv[:, hd:], H, D, cu_seqlens=cu, max_keys=n, out=out)}, args.repeats, args.inner)
                lds = n * ((D + 15) // 16 * 32 + 2 * D)
                emit(line(f"  {H} x {D}, T = {T}, B = {B}, {n} keys each", t["kernel"],
                          f"  {n // 64} chunks, LDS {lds / 1024:.0f} KiB"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--batches", type=int, nargs="+", default=(2, 3))
    ap.add_argument("--out", default=None)
    ap.add_argument("--key-series", action="store_true")
    args = ap.parse_args()

    from nunchaku_amd.ops import cross_attention

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
    if args.key_series:
        return key_series(cross_attention, dev, args, emit)
    emit(f"cross-attention over per-sample key ranges, bf16, one launch per call; byte bound = 2 * (2*B*T + 2*sum(counts)) * H*D bytes at {COPY_TBS} TB/s; "
         "no counter run was made")
    g = torch.Generator(device=dev).manual_seed(0)
    for H, D in HEADS:
        hd = H * D
        width = (hd + 127) // 128 * 128
        for T in TOKENS:
            for B in args.batches:
                for counts in ((300,) * B, RAGGED[:B]):
                    q = torch.randn(B, T, width, device=dev, generator=g).bfloat16()
                    kv = torch.randn(sum(counts), 2 * hd, device=dev, generator=g).bfloat16()
                    k, v = kv[:, :hd], kv[:, hd:]
                    offs = [sum(counts[:b]) for b in range(B)]
                    cu = torch.tensor(offs + [sum(counts)], dtype=torch.int32, device=dev)
                    out = torch.empty(B, T, hd, device=dev, dtype=torch.bfloat16)
                    ref = torch.empty_like(out)

                    def kernel():
                        return cross_attention(q, k, v, H, D, cu_seqlens=cu, max_keys=max(counts), out=out)

                    def torch_sdpa():
                        for b, (off, n) in enumerate(zip(offs, counts)):
                            qb = q[b, :, :hd].view(1, T, H, D).transpose(1, 2)
                            kb = k[off:off + n].view(1, n, H, D).transpose(1, 2)
                            vb = v[off:off + n].view(1, n, H, D).transpose(1, 2)
                            ref[b].copy_(F.scaled_dot_product_attention(qb, kb, vb).transpose(1, 2).reshape(T, hd))
                        return ref

                    diff = (kernel().float() - torch_sdpa().float()).abs().max().item()
                    t = alternate({"kernel": kernel, "torch": torch_sdpa}, args.repeats, args.inner)
                    med = {k_: statistics.median(xs) for k_, xs in t.items()}
                    bound_ms = 2 * (2 * B * T + 2 * sum(counts)) * hd / (COPY_TBS * 1e12) * 1e3
                    emit(f"H x D = {H} x {D}, T = {T}, B = {B}, keys {counts}: byte bound {bound_ms:.4f} ms; max |kernel - torch SDPA| = {diff:.3g} "
                         f"(max |ref| {ref.float().abs().max().item():.3g})")
                    emit(line("  svdq_cross_attention (1 launch)", t["kernel"],
                              f"  {med['kernel'] / bound_ms:.2f} x the byte bound ({bound_ms / med['kernel']:.2f} of it); kernel / torch = {med['kernel'] / med['torch']:.3f}"))
                    emit(line("  torch SDPA per sample + copies", t["torch"]))
                    del q, kv, out, ref


if __name__ == "__main__":
    main()
