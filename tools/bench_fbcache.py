"""Timings of First-Block Cache on one MI355X (bench.py stays the flagship benchmark and is not involved).

1. The similarity pass ``svdq_residual_diff`` at (4096, 3072) bf16 against the torch-op sequence the reference runs for the same result
   (two subtractions, two ``abs``, two ``mean``, a division), with the achieved GB/s of the kernel's 8 bytes per element.
2. A FLUX.1-dev-shaped 1024 x 1024 step with synthetic weights in the default mode: uncached, cached miss and cached hit.

Event-bracketed, warm; the versions alternate inside one process and the whole round is repeated: min / median / max per version.

    python tools/bench_fbcache.py [--repeats 7] [--inner 5] [--layers 19 38] [--out profiles/fbcache.txt]
"""

import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


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
    return f"{name:<34} min {min(xs):9.4f}  median {statistics.median(xs):9.4f}  max {max(xs):9.4f} ms  (n={len(xs)}){extra}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--layers", type=int, nargs=2, default=(19, 38))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from nunchaku_amd.caching import fbcache
    from nunchaku_amd.caching.diffusers_adapters.flux_v2 import apply_cache_on_transformer
    from nunchaku_amd.models.flux import FluxTransformerAMD
    from nunchaku_amd.ops.elementwise import residual_diff

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    lines = [f"device: {torch.cuda.get_device_name(dev)}; repeats {args.repeats} x inner {args.inner}, versions alternated"]

    # ---- 1. the similarity pass ---------------------------------------------------------------------------------------------------
    M, C = 4096, 3072
    g = torch.Generator(device=dev).manual_seed(0)
    base, prev = (torch.randn(M, C, device=dev, generator=g).bfloat16() for _ in range(2))
    cur = base + prev + (0.05 * torch.randn(M, C, device=dev, generator=g)).bfloat16()
    out = torch.empty_like(cur)

    def torch_sequence():  # utils_v2.py:133 + fbcache.py:275-277
        r = cur - base
        return (prev - r).abs().mean() / prev.abs().mean()

    t = alternate({"kernel": lambda: residual_diff(cur, base, prev, out), "torch": torch_sequence}, args.repeats, args.inner * 10)
    gbs = M * C * 8 / (statistics.median(t["kernel"]) * 1e-3) / 1e9
    lines.append(f"similarity pass ({M}, {C}) bf16: r = cur - base, mean|prev - r| / mean|prev|")
    lines.append(line("  svdq_residual_diff (2 launches)", t["kernel"], f"  {gbs:.0f} GB/s of 8 B/element (copy figure of the chip: 6290 GB/s)"))
    lines.append(line("  torch-op sequence (7 launches)", t["torch"]))

    # ---- 2. the step --------------------------------------------------------------------------------------------------------------
    nj, ns = args.layers
    model = FluxTransformerAMD(num_layers=nj, num_single_layers=ns, device=dev).init_synthetic_(seed=0, codes="residual").eval()
    gh = gw = 64
    t_img, t_txt = gh * gw, 512
    g = torch.Generator(device=dev).manual_seed(1234)
    lat = torch.randn(1, t_img, 64, generator=g, device=dev, dtype=torch.bfloat16)
    lat2 = torch.randn(1, t_img, 64, generator=g, device=dev, dtype=torch.bfloat16)
    enc = torch.randn(1, t_txt, 4096, generator=g, device=dev, dtype=torch.bfloat16)
    pooled = torch.randn(1, 768, generator=g, device=dev, dtype=torch.bfloat16)
    img_ids = torch.zeros(t_img, 3, device=dev)
    img_ids[:, 1] = torch.arange(gh, device=dev).repeat_interleave(gw)
    img_ids[:, 2] = torch.arange(gw, device=dev).repeat(gh)
    rest = (enc, pooled, torch.tensor([0.5], device=dev), img_ids, torch.zeros(t_txt, 3, device=dev), torch.full((1,), 3.5, device=dev))
    uncached = model.forward
    apply_cache_on_transformer(model, residual_diff_threshold=0.12)
    flip = [0]

    def miss():  # alternating latents: every call differs from the stored step (checked below)
        flip[0] ^= 1
        return model(lat2 if flip[0] else lat, *rest)

    with torch.no_grad(), fbcache.cache_context(fbcache.create_cache_context()) as _:
        ctx = fbcache.get_current_cache_context()
        model(lat, *rest)
        first = ctx.get_buffer("first_multi_hidden_states_residual")
        model(lat2, *rest)
        assert ctx.get_buffer("first_multi_hidden_states_residual") is not first, "fresh latents must be a miss"
        # hit: the stored step is `lat`'s; calling with `lat` again never replaces it
        model(lat, *rest)
        stored = ctx.get_buffer("first_multi_hidden_states_residual")

        def hit():
            return model(lat, *rest)

        hit()
        assert ctx.get_buffer("first_multi_hidden_states_residual") is stored, "the same latents must be a hit"
        hit_ctx = ctx
        t_hit = None
        miss_ctx = fbcache.create_cache_context()

        def in_ctx(c, fn):
            def run():
                with fbcache.cache_context(c):
                    return fn()
            return run

        t = alternate({"uncached": lambda: uncached(lat, *rest), "miss": in_ctx(miss_ctx, miss), "hit": in_ctx(hit_ctx, hit)},
                      args.repeats, args.inner)
        assert hit_ctx.get_buffer("first_multi_hidden_states_residual") is stored
    lines.append(f"FLUX.1-dev-shaped step, {nj} + {ns} blocks, 1024 x 1024, {t_txt} text tokens, bf16, synthetic weights, default mode")
    for k in ("uncached", "miss", "hit"):
        lines.append(line("  " + k + " step", t[k]))
    lines.append(f"  miss - uncached (medians): {statistics.median(t['miss']) - statistics.median(t['uncached']):+.4f} ms; "
                 f"spread of uncached (max - min): {max(t['uncached']) - min(t['uncached']):.4f} ms")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
