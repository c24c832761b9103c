"""Timings of TeaCache on one MI355X (bench.py stays the flagship benchmark and is not involved).

1. The decision pass ``svdq_modulated_diff`` at (4096, 3072) bf16 -- statistics given, modulate, store over the previous step's modulated input
   and compare in the same pass -- against the torch-op restatement of the reference (``layer_norm``, ``*``, ``+``, ``-``, ``abs``, two
   ``mean``, ``/``), with the achieved GB/s of the kernel's 6 bytes per element.
2. A FLUX.1-dev-shaped 1024 x 1024 step with synthetic weights in the default mode: uncached, as a computed TeaCache step and as a skipped one.

Event-bracketed, warm; the versions alternate inside one process and the whole round is repeated: min / median / max per version.

    python tools/bench_teacache.py [--repeats 7] [--inner 5] [--layers 19 38] [--out profiles/teacache.txt]
"""

import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

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
    return f"{name:<38} min {min(xs):9.4f}  median {statistics.median(xs):9.4f}  max {max(xs):9.4f} ms  (n={len(xs)}){extra}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--layers", type=int, nargs=2, default=(19, 38))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from nunchaku_amd.caching.teacache import TeaCache, resolve_coefficients, teacache_decide
    from nunchaku_amd.models.flux import FluxTransformerAMD
    from nunchaku_amd.ops.elementwise import modulated_diff, residual_gate_stats

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    lines = [f"device: {torch.cuda.get_device_name(dev)}; repeats {args.repeats} x inner {args.inner}, versions alternated"]

    # ---- 1. the decision pass -----------------------------------------------------------------------------------------------------
    M, C = 4096, 3072
    g = torch.Generator(device=dev).manual_seed(0)
    x = (torch.randn(M, C, device=dev, generator=g) * 2).bfloat16()
    scale = (1 + 0.3 * torch.randn(C, device=dev, generator=g)).bfloat16()
    shift = (0.5 * torch.randn(C, device=dev, generator=g)).bfloat16()
    stats = residual_gate_stats(x)[1]  # (the engine has them anyway on the fused path: not part of the timed pass)
    buf = modulated_diff(x, stats, scale, shift)[0]
    buf = (buf.float() + 0.05 * torch.randn(M, C, device=dev, generator=g)).bfloat16()
    prev_t = buf.clone()

    def torch_sequence():  # teacache.py:187 (norm1's modulated input) + :199-200
        m = F.layer_norm(x, (C,), eps=1e-6) * scale + shift
        return (m - prev_t).abs().mean() / prev_t.abs().mean()

    t = alternate({"kernel": lambda: modulated_diff(x, stats, scale, shift, prev=buf, out=buf), "torch": torch_sequence},
                  args.repeats, args.inner * 10)
    gbs = M * C * 6 / (statistics.median(t["kernel"]) * 1e-3) / 1e9
    lines.append(f"decision pass ({M}, {C}) bf16: m = LayerNorm(x) * scale + shift (stored in place over prev), mean|prev - m| / mean|prev|")
    lines.append(line("  svdq_modulated_diff (2 launches)", t["kernel"], f"  {gbs:.0f} GB/s of 6 B/element (copy figure of the chip: 6290 GB/s)"))
    lines.append(line("  torch-op sequence (9 launches)", t["torch"]))

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
    # The engine's TeaCache forward driven by the state machine itself, on one long run (num_steps beyond every call made here): step 0 computes and
    # stores the residual; afterwards every step reads the record on the host and the threshold decides -- 0: computed, huge: skipped.
    coeffs = resolve_coefficients("flux")
    kinds = []

    def step(thresh):
        def decide(ratio_fn):
            kinds.append(teacache_decide(model, ratio_fn, num_steps=10 ** 9, rel_l1_thresh=thresh, skip_steps=0, coefficients=coeffs))
            return kinds[-1]
        return lambda: model.teacache_forward(*inputs, decide=decide)

    computed, skipped = step(0.0), step(1e30)
    with torch.no_grad(), TeaCache(model, num_steps=10 ** 9):
        model(*inputs)  # step 0 of the run
        kinds.clear()
        t = alternate({"uncached": lambda: model.engine_forward(*inputs), "computed": computed, "skipped": skipped}, args.repeats, args.inner)
    per_version = 3 + args.repeats * args.inner
    assert kinds.count((True, True)) == per_version and kinds.count((False, True)) == per_version, "every timed call must be what its name says"
    lines.append(f"FLUX.1-dev-shaped step, {nj} + {ns} blocks, 1024 x 1024, {t_txt} text tokens, bf16, synthetic weights, default mode")
    for k in ("uncached", "computed", "skipped"):
        lines.append(line("  " + k + " step", t[k]))
    lines.append(f"  computed - uncached (medians): {statistics.median(t['computed']) - statistics.median(t['uncached']):+.4f} ms; "
                 f"spread of uncached (max - min): {max(t['uncached']) - min(t['uncached']):.4f} ms")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
