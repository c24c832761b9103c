"""Timings of First-Block Cache for Qwen-Image and SANA on one MI355X (a sibling of tools/bench_fbcache.py; bench.py stays the flagship
benchmark and is not involved).

Three arms per shape, alternated inside one process, event-bracketed, warm; min / median / max per arm:
  uncached  the plain step
  miss      the cached step with inputs that differ from the stored step's (checked: the stored first residual is replaced)
  hit       the cached step with the stored step's inputs (checked: the stored first residual stays)

Qwen-Image: 60 blocks, synthetic weights, bf16, 512 text tokens, 1024 x 1024 (4096 image tokens) and 1664 x 928 (6032), ``first_blocks``
1 and 8.  SANA-1.6B's stack: 20 blocks, B = 2, 32 x 32 and 64 x 64 tokens, 300 text tokens with key counts (300, 37).  No hit rate is
measured: that depends on real checkpoints.

    python tools/bench_fbcache_qwen_sana.py [--model qwen|sana|all] [--repeats 7] [--inner 3] [--out profiles/fbcache_qwen_sana.txt]
"""

import argparse
import math
import os
import statistics
import sys
from types import SimpleNamespace

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_fbcache import alternate, line  # noqa: E402

FIRST = "first_multi_hidden_states_residual"


def arms(uncached, cached, same, other, ctx_name, repeats, inner):
    """``cached(x)`` runs in the active context.  -> times of the three arms; the hit and the miss arm each keep a context of their own"""
    from nunchaku_amd.caching import fbcache

    hit_ctx, miss_ctx = fbcache.create_cache_context(), fbcache.create_cache_context()
    flip = [0]

    def in_ctx(c, fn):
        def run():
            with fbcache.cache_context(c):
                return fn()
        return run

    def miss():
        flip[0] ^= 1
        return cached(other if flip[0] else same)

    in_ctx(hit_ctx, lambda: cached(same))()
    stored = hit_ctx.get_buffer(ctx_name)
    in_ctx(miss_ctx, lambda: cached(same))()
    before = miss_ctx.get_buffer(ctx_name)
    in_ctx(miss_ctx, miss)()
    assert miss_ctx.get_buffer(ctx_name) is not before, "other inputs must be a miss"
    t = alternate({"uncached": lambda: uncached(same), "miss": in_ctx(miss_ctx, miss), "hit": in_ctx(hit_ctx, lambda: cached(same))},
                  repeats, inner)
    assert hit_ctx.get_buffer(ctx_name) is stored, "the same inputs must be a hit"
    return t


def report(lines, t):
    for k in ("uncached", "miss", "hit"):
        lines.append(line("    " + k + " step", t[k]))
    med = {k: statistics.median(v) for k, v in t.items()}
    lines.append(f"    miss - uncached (medians): {med['miss'] - med['uncached']:+.4f} ms; spread of uncached (max - min): "
                 f"{max(t['uncached']) - min(t['uncached']):.4f} ms; hit / uncached: {med['hit'] / med['uncached']:.3f}")


def bench_qwen(dev, args, lines):
    from nunchaku_amd.models.qwenimage import NunchakuQwenImageTransformer2DModel

    model = NunchakuQwenImageTransformer2DModel(num_layers=args.qwen_layers, device=dev).init_synthetic_(seed=0, codes="residual").eval()
    plain = NunchakuQwenImageTransformer2DModel.forward
    t_txt = 512
    for width, height in ((1024, 1024), (1664, 928)):
        gh, gw = height // 16, width // 16
        g = torch.Generator(device=dev).manual_seed(1234)
        lat, lat2 = (torch.randn(1, gh * gw, 64, generator=g, device=dev, dtype=torch.bfloat16) for _ in range(2))
        enc = torch.randn(1, t_txt, 3584, generator=g, device=dev, dtype=torch.bfloat16)
        rest = (enc, None, torch.tensor([0.5], device=dev), [(1, gh, gw)])
        for fb in (1, 8):
            if fb >= args.qwen_layers:
                continue
            t = arms(lambda x: plain(model, x, *rest, return_dict=False),
                     lambda x: model.forward_cached(x, *rest, return_dict=False, residual_diff_threshold=0.12, first_blocks=fb),
                     lat, lat2, FIRST + "_0", args.repeats, args.inner)
            lines.append(f"  Qwen-Image-shaped step, {args.qwen_layers} blocks, {width} x {height} ({gh * gw} image + {t_txt} text tokens), "
                         f"first_blocks={fb}, bf16, synthetic weights, default mode")
            report(lines, t)
    del model
    torch.cuda.empty_cache()


@torch.no_grad()
def sana_synthetic_(m, seed):
    """random weights for the SANA stack on the device: the 4-bit layers as models/blocks.py ``init_synthetic_`` fills them, the 16-bit
    parameters small (the scales tests/test_gpu_sana_block.py uses)"""
    from nunchaku_amd.models.linear import SVDQW4A4Linear, synthetic_codes_

    dev = m.transformer_blocks[0].scale_shift_table.device
    g = torch.Generator(device=dev).manual_seed(seed)
    rnd = lambda shape, scale: torch.randn(shape, generator=g, device=dev) * scale
    done = set()
    for mod in m.modules():
        if isinstance(mod, SVDQW4A4Linear):
            K = mod.in_features
            synthetic_codes_(mod.qweight, mod.wscales, K, g, "residual")
            if mod.bias is not None:
                mod.bias.copy_(rnd(mod.bias.shape, 0.02))
            mod.smooth_factor.copy_(torch.rand((K,), generator=g, device=dev) + 0.5)
            mod.smooth_factor_orig.copy_(mod.smooth_factor)
            mod.proj_down.copy_(rnd(mod.proj_down.shape, 0.5 / math.sqrt(K)))
            mod.proj_up.copy_(rnd(mod.proj_up.shape, 0.5 / math.sqrt(mod.rank)))
            mod._amd_layout = False
            done.update(id(p) for p in mod.parameters())
    for name, p in m.named_parameters():
        if id(p) in done:
            continue
        scale = p.shape[-1] ** -0.5 if name.endswith("kv_linear.weight") else 1 / 3 if name.endswith("depth_conv.weight") \
            else 0.5 if name.endswith("scale_shift_table") else 0.1
        p.copy_(rnd(p.shape, scale))
    return m


def bench_sana(dev, args, lines):
    from nunchaku_amd.caching.utils import SanaCachedTransformerBlocks
    from nunchaku_amd.models import SanaModel
    from nunchaku_amd.models.transformer_sana import NunchakuSanaTransformerBlocks

    cfg = dict(num_layers=args.sana_layers, num_attention_heads=70, attention_head_dim=32, num_cross_attention_heads=20, mlp_ratio=2.5)
    dim, B, L, counts = 2240, 2, 300, (300, 37)
    stack = NunchakuSanaTransformerBlocks(sana_synthetic_(SanaModel(cfg, pag_layers=[], device=dev), seed=0), torch.bfloat16, dev)
    cached = SanaCachedTransformerBlocks(transformer=SimpleNamespace(transformer_blocks=torch.nn.ModuleList([stack])), residual_diff_threshold=0.12)
    for side in (32, 64):
        g = torch.Generator(device=dev).manual_seed(4321)
        x, x2 = (torch.randn(B, side * side, dim, generator=g, device=dev).bfloat16() for _ in range(2))
        cond = torch.randn(B, L, dim, generator=g, device=dev).bfloat16()
        ts = (0.5 * torch.randn(B, 6 * dim, generator=g, device=dev)).bfloat16()
        mask = torch.full((B, 1, L), -10000.0, device=dev, dtype=torch.bfloat16)
        for i, n in enumerate(counts):
            mask[i, 0, :n] = 0
        rest = (None, cond, mask, ts, side, side)
        out = stack(x, *rest)
        assert torch.isfinite(out.float()).all(), "synthetic SANA weights gave a non-finite stream"
        t = arms(lambda h: stack(h, *rest), lambda h: cached(h, *rest), x, x2, FIRST, args.repeats, args.inner)
        lines.append(f"  SANA-1.6B-shaped stack, {args.sana_layers} blocks, B = {B}, {side} x {side} tokens, {L} text tokens (keys {counts}), bf16, "
                     "synthetic weights, default mode")
        report(lines, t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", choices=["qwen", "sana", "all"], default="all")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--qwen-layers", type=int, default=60)
    ap.add_argument("--sana-layers", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    lines = [f"device: {torch.cuda.get_device_name(dev)}; repeats {args.repeats} x inner {args.inner}, arms alternated; ms per step"]
    with torch.no_grad():
        if args.model in ("qwen", "all"):
            bench_qwen(dev, args, lines)
        if args.model in ("sana", "all"):
            bench_sana(dev, args, lines)
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
