"""Timings of the IP-Adapter path on one MI355X (bench.py stays the flagship benchmark and is not involved).

1. ``svdq_ip_attention`` at T = 4096, H = 24, N in {4, 128, 256}, bf16, Q read in place from a packed [T, 3*H*128] buffer, against the
   reference's torch-op sequence on the same tensors (a contiguous copy of Q, the three view-transposes, SDPA, the transpose-reshape copy
   and the multiply of the scaled add), with the achieved TB/s of the kernel's compulsory bytes (Q read + output written; K and V are
   N * H * 256 bytes each and stay in cache) against the chip's copy figure.
2. A FLUX.1-dev-shaped 1024 x 1024 step with synthetic weights in the default mode: plain, with an adapter (N_ip = 4, as one CLIP
   image prompt projects to, and 128) on the fused path, with the adapter's step forced onto the torch-op sequence inside the fused
   blocks, with the second QKV projection alone (the adapter's add skipped), and the whole torch-op arm (``fused_norm`` off) with and
   without the adapter.

Event-bracketed, warm; the versions alternate inside one process and the whole round is repeated: min / median / max per version.

    python tools/bench_ip_attention.py [--repeats 7] [--inner 3] [--layers 19 38] [--out profiles/ip_adapter.txt]
"""

import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

COPY_TBS = 6.29  # float4 copy on MI355X


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


def adapter_state_dict(blocks, cross_dim, dim, seed=0):
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for i in range(blocks):
        for n in ("k", "v"):
            base = f"double_blocks.{i}.processor.ip_adapter_double_stream_{n}_proj"
            sd[base + ".weight"] = (torch.randn(dim, cross_dim, generator=g) * (0.5 / cross_dim ** 0.5)).bfloat16()
            sd[base + ".bias"] = torch.zeros(dim).bfloat16()
    return sd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--layers", type=int, nargs=2, default=(19, 38))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from nunchaku_amd.models.flux import FluxTransformerAMD
    from nunchaku_amd.models.ip_adapter import apply_IPA_on_transformer, undo_all_mods_on_transformer
    from nunchaku_amd.ops.attention import ip_attention

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    lines = [f"device: {torch.cuda.get_device_name(dev)}; repeats {args.repeats} x inner {args.inner} (kernel: x 20), versions alternated"]

    # ---- 1. the kernel ------------------------------------------------------------------------------------------------------------
    T, H = 4096, 24
    hd = H * 128
    g = torch.Generator(device=dev).manual_seed(0)
    qkv = torch.randn(T, 3 * hd, device=dev, generator=g).bfloat16()
    out = torch.empty(T, hd, device=dev, dtype=torch.bfloat16)
    scale = 0.7
    lines.append(f"image-prompt cross-attention, T = {T}, H = {H}, head dim 128, bf16, Q inside a packed [T, {3 * hd}] buffer, out_scale {scale}")
    for N in (4, 128, 256):
        k = torch.randn(N, hd, device=dev, generator=g).bfloat16()
        v = torch.randn(N, hd, device=dev, generator=g).bfloat16()

        def torch_sequence():  # ip_adapter/utils.py:361-372 (up to, not including, the add)
            q = qkv[:, :hd].contiguous().view(1, -1, H, 128).transpose(1, 2)
            o = F.scaled_dot_product_attention(q, k.view(1, -1, H, 128).transpose(1, 2), v.view(1, -1, H, 128).transpose(1, 2),
                                               attn_mask=None, dropout_p=0.0, is_causal=False)
            return scale * o.transpose(1, 2).reshape(1, -1, hd)

        t = alternate({"kernel": lambda: ip_attention(qkv, k, v, H, out=out, out_scale=scale), "torch": torch_sequence},
                      args.repeats, args.inner * 20)
        med = statistics.median(t["kernel"])
        tbs = 2 * T * hd * 2 / (med * 1e-3) / 1e12
        flops = 4.0 * T * hd * ((N + 31) // 32 * 32)
        lines.append(line(f"  N = {N:3d}  svdq_ip_attention (1 launch)", t["kernel"],
                          f"  {tbs:.2f} TB/s of Q + out ({100 * tbs / COPY_TBS:.0f} % of the copy figure {COPY_TBS}); {flops / (med * 1e-3) / 1e12:.0f} TFLOP/s of padded MFMA work"))
        lines.append(line(f"  N = {N:3d}  torch-op sequence", t["torch"], f"  kernel / torch = {med / statistics.median(t['torch']):.2f}"))

    # ---- 2. the step --------------------------------------------------------------------------------------------------------------
    nj, ns = args.layers
    model = FluxTransformerAMD(num_layers=nj, num_single_layers=ns, device=dev).init_synthetic_(seed=0, codes="residual").eval()
    gh = gw = 64
    t_img, t_txt = gh * gw, 512
    g = torch.Generator(device=dev).manual_seed(1234)
    lat = torch.randn(1, t_img, 64, generator=g, device=dev, dtype=torch.bfloat16)
    enc = torch.randn(1, t_txt, 4096, generator=g, device=dev, dtype=torch.bfloat16)
    pooled = torch.randn(1, 768, generator=g, device=dev, dtype=torch.bfloat16)
    img_ids = torch.zeros(t_img, 3, device=dev)
    img_ids[:, 1] = torch.arange(gh, device=dev).repeat_interleave(gw)
    img_ids[:, 2] = torch.arange(gw, device=dev).repeat(gh)
    inputs = (lat, enc, pooled, torch.tensor([0.5], device=dev), img_ids, torch.zeros(t_txt, 3, device=dev), torch.full((1,), 3.5, device=dev))
    sd = adapter_state_dict(nj, 4096, model.dim)
    lines.append(f"FLUX.1-dev-shaped step, {nj} + {ns} blocks, 1024 x 1024, {t_txt} text tokens, bf16, synthetic weights, default mode")

    def forward():
        return model.engine_forward(*inputs)

    def with_flags(fn, **flags):  # run fn with attributes of the model set for the call
        def run():
            saved = {k: getattr(model, k) for k in flags}
            for k, v_ in flags.items():
                setattr(model, k, v_)
            try:
                return fn()
            finally:
                for k, v_ in saved.items():
                    setattr(model, k, v_)
        return run

    with torch.no_grad():
        plain = alternate({"plain": forward, "plain, torch-op arm (fused_norm off)": with_flags(forward, fused_norm=False)}, args.repeats, args.inner)
        for k_, xs in plain.items():
            lines.append(line("  " + k_, xs))
        for n_ip in (4, 128):
            apply_IPA_on_transformer(model, ip_adapter_scale=scale, repo_id=sd)
            model.set_ip_hidden_states(torch.randn(1, n_ip, 4096, generator=g, device=dev, dtype=torch.bfloat16))
            skip_add = lambda st, i, qkv_: None
            versions = {
                "plain (adapter detached)": with_flags(forward, ip_adapter=None),
                "adapter, fused path": forward,
                "adapter, second QKV projection only": with_flags(forward, _ip_add=skip_add),
                "adapter, torch-op step in fused blocks": with_flags(forward, _ip_fused=lambda st, attn: False),
                "adapter, torch-op arm (fused_norm off)": with_flags(forward, fused_norm=False),
            }
            t = alternate(versions, args.repeats, args.inner)
            lines.append(f"  adapter attached, N_ip = {n_ip}, scale {scale} (K / V projected once per embeddings tensor: not in the step)")
            for k_, xs in t.items():
                lines.append(line("    " + k_, xs))
            med = {k_: statistics.median(xs) for k_, xs in t.items()}
            base = med["plain (adapter detached)"]
            lines.append(f"    cost over the plain step (medians): fused path {med['adapter, fused path'] - base:+.3f} ms, of which the second QKV "
                         f"projection {med['adapter, second QKV projection only'] - base:+.3f} ms; torch-op step in fused blocks "
                         f"{med['adapter, torch-op step in fused blocks'] - base:+.3f} ms; torch-op arm over its own plain step "
                         f"{med['adapter, torch-op arm (fused_norm off)'] - statistics.median(plain['plain, torch-op arm (fused_norm off)']):+.3f} ms; "
                         f"spread of plain (max - min) {max(t['plain (adapter detached)']) - min(t['plain (adapter detached)']):.3f} ms")
            undo_all_mods_on_transformer(model)
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
