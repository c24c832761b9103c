"""Timings of Stable Diffusion XL's attention on one MI355X (bench.py stays the flagship benchmark and is not involved).

``svdq_attention_d64`` (one launch; Q, K, V read in place: for self-attention the three column thirds of the packed ``[B, T, 3*H*64]`` output of
``to_qkv``, for cross-attention the outputs of ``to_q`` / ``to_k`` / ``to_v``; ``out`` token-major) at SDXL's shapes
(B, T, H, N) = (2, 4096, 10, 4096), (2, 1024, 20, 1024), (2, 4096, 10, 77), (2, 1024, 20, 77) and the same at B = 1, in bf16 and fp16, against

  (a) the torch sequence it replaces, in the same run: ``view`` / ``transpose`` of the same operands to ``[B, H, T|N, 64]``,
      ``F.scaled_dot_product_attention`` and the ``transpose`` + ``reshape`` copy back to token-major rows (the reference's processor);
  (b) the bf16 / fp16 MFMA rate: ``4*B*H*T*N*64`` FLOP at 2.5 PFLOP/s (the dense spec figure), stated as a fraction.

Outputs of the kernel and of (a) are compared at every shape before anything is timed.

Event-bracketed, warm; the two versions alternate inside one process and the whole round is repeated: min / median / max per version.

    python tools/bench_sdxl_attention.py [--repeats 7] [--inner 20] [--out profiles/sdxl_attention.txt]

``--graph`` times each version as the replay of a captured graph of ``inner`` calls instead: the host's time to issue a call (the op's checks, the
ctypes call; torch's dispatch) is then outside the measurement, and what remains is the kernels' time on the device
(``--out profiles/sdxl_attention_graph.txt``).
"""

import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

MFMA_PFLOPS = 2.5  # dense bf16 / fp16, spec
SHAPES = [(4096, 10, 4096), (1024, 20, 1024), (4096, 10, 77), (1024, 20, 77)]  # (T, H, N)


def timed(fn, inner):
    """ms per call of ``inner`` back-to-back calls between two events"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def captured(fn, inner):
    """a callable that replays a captured graph of ``inner`` back-to-back calls of ``fn``"""
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(inner):
            fn()
    return graph.replay


def alternate(versions: dict, repeats: int, inner: int, graph: bool = False) -> dict:
    for fn in versions.values():  # warm
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    if graph:
        replays = {k: captured(fn, inner) for k, fn in versions.items()}
        for fn in replays.values():
            fn()
    out = {k: [] for k in versions}
    for _ in range(repeats):
        for k, fn in versions.items():
            out[k].append(timed(replays[k], 1) / inner if graph else timed(fn, inner))
    return out


def line(name, xs, extra=""):
    return f"{name:<44} min {min(xs):9.4f}  median {statistics.median(xs):9.4f}  max {max(xs):9.4f} ms  (n={len(xs)}){extra}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--batches", type=int, nargs="+", default=(2, 1))
    ap.add_argument("--out", default=None)
    ap.add_argument("--graph", action="store_true", help="time replays of a captured graph of --inner calls (device time without the host's issue time)")
    args = ap.parse_args()

    from nunchaku_amd.ops import attention_d64

    if not torch.cuda.is_available():
        raise SystemExit("bench_sdxl_attention: no GPU: a timing needs the MI355X (nothing is measured on the CPU)")
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
    emit(f"attention at head dimension 64, one launch per call; MFMA bound = 4*B*H*T*N*64 FLOP at {MFMA_PFLOPS} PFLOP/s (dense 16-bit spec); "
         + ("times are replays of a captured graph of the calls, per call: the device's time without the host's issue time; " if args.graph else
            "times are call times between device events, not kernel times from a trace; ") + "no counter run was made")
    g = torch.Generator(device=dev).manual_seed(0)
    for dtype in (torch.bfloat16, torch.float16):
        for T, H, N in SHAPES:
            for B in args.batches:
                hd = H * 64
                if N == T:  # self-attention: the packed QKV projection
                    qkv = torch.randn(B, T, 3 * hd, device=dev, generator=g).to(dtype)
                    q, k, v = qkv[..., :hd], qkv[..., hd:2 * hd], qkv[..., 2 * hd:]
                else:       # cross-attention: to_q on the image tokens, to_k / to_v on the text
                    q = torch.randn(B, T, hd, device=dev, generator=g).to(dtype)
                    k = torch.randn(B, N, hd, device=dev, generator=g).to(dtype)
                    v = torch.randn(B, N, hd, device=dev, generator=g).to(dtype)
                out = torch.empty(B, T, hd, device=dev, dtype=dtype)

                def kernel():
                    return attention_d64(q, k, v, H, out=out)

                def torch_sdpa():
                    qh = q.reshape(B, -1, H, 64).transpose(1, 2)   # (the reference's .view on its chunk: a strided view, no copy yet)
                    kh = k.reshape(B, -1, H, 64).transpose(1, 2)
                    vh = v.reshape(B, -1, H, 64).transpose(1, 2)
                    return F.scaled_dot_product_attention(qh, kh, vh, dropout_p=0.0, is_causal=False).transpose(1, 2).reshape(B, -1, hd)

                ref = torch_sdpa()
                diff = (kernel().float() - ref.float()).abs().max().item()
                t = alternate({"kernel": kernel, "torch": torch_sdpa}, args.repeats, args.inner, args.graph)
                med = {k_: statistics.median(xs) for k_, xs in t.items()}
                flop = 4.0 * B * H * T * N * 64
                bound_ms = flop / (MFMA_PFLOPS * 1e15) * 1e3
                name = {torch.bfloat16: "bf16", torch.float16: "fp16"}[dtype]
                emit(f"{name} (B, T, H, N) = ({B}, {T}, {H}, {N}): {flop / 1e9:.2f} GFLOP, MFMA bound {bound_ms:.4f} ms; max |kernel - torch SDPA| = {diff:.3g} "
                     f"(max |ref| {ref.float().abs().max().item():.3g})")
                emit(line("  svdq_attention_d64 (1 launch)", t["kernel"],
                          f"  {bound_ms / med['kernel']:.3f} of the MFMA rate ({flop / med['kernel'] / 1e9:.0f} TFLOP/s); kernel / torch = {med['kernel'] / med['torch']:.3f}"))
                emit(line("  torch: view / transpose + SDPA + copy back", t["torch"]))
                del q, k, v, out, ref


if __name__ == "__main__":
    main()
